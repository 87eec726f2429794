"""like_kernel and gauss_q_kernel (bayhunter_amd/csrc/like_kernel.hip) through the C ABI -- bh_likelihood_batch,
bh_likelihood_stage, bh_likelihood_sets -- against the extended-precision reference and the DERIVED bounds of
tests/likelihood_hp.py, over the table of cases that tests/test_likelihood_hp.py has proven well-posed on the CPU:
target lengths 1 .. LIKE_NMAX around the 64-lane strides and the 16-column tiles, the real pinv / inv matrices
and an asymmetric one, batches around the 8-model workgroup, the 16-model tile and the split/fused switch,
1 to 6 targets of every form in every position with gaps, padding and err-flag columns, correlations up to
+-0.999999, sigma down to 1e-5, scaled errors up to 1e6, observation sets, and NaN / Inf rows.

Every case runs with the matrix-core workspace ('ws'), without it ('nows': the vector path) and in the two
stages ('staged') where it holds a dense target.  Batches above likelihood_hp.SAMPLE_ABOVE rows are compared on
likelihood_hp.sample_rows (at most 456 rows: the first and last 64, the 64 on each side of the switch, 200
random ones); all their rows must be finite.  Each comparison prints its worst error / bound ratio.

Measured on an MI355X (270 comparisons, the file takes 9 s): largest error / bound of logL and of a misfit per
form -- nocorr 0.15 / 0.13, scaled 0.13 / 0.18, exp 0.11 / 0.17, gauss 0.15 / 0.11, mixed targets 0.16 / 0.21 --
the same figures as plain fp64 numpy on the CPU (0.16 / 0.21): no term of the derivation is near its limit.

Seeded faults in like_kernel.hip (built from a scratch copy, never committed) and the cases that went red:
  n for n - 1 in the exponential log-determinant   46: len_exp_* (all with a corr != 0), batch_*, layout_*, noise_edges*, sets_*
  end diagonal applied at i == n - 2               44: len_exp_* from n = 2, batch_*, layout_*, noise_edges, sets_*
  last column tile of a group skipped              56: dense_* from n = 63 (the first with a fourth tile), batch_* incl. the fused forms, layout_*
  yobs of set 0 in gauss_q_kernel's reduction       5: sets_7_random, sets_7_oob, sets_1000_random / _own / _oob
  tg.off ignored for the second target             36: batch_*, layout_* (T >= 2), noise_edges*, scaled_wide_*, sets_*
  sum misfit column written at index T - 1        123: every case
  R^-1 read transposed, both paths                  0: d^T R^-1 d is a scalar and equals d^T (R^-1)^T d for ANY matrix,
      so a consistently transposed read is the same function and no test of the outputs can tell it apart.  What an
      asymmetric matrix does catch is an operand transposed in part: the matrix-core B fragment read transposed
      inside its 16 x 16 tile turns 62 cases red (every dense_* from n = 17 incl. the symmetric pinv, batch_*, layout_*).
"""
import numpy as np
import pytest

import likelihood_hp as hp


def run_gpu(lib, k, mode):
    import torch
    from bayhunter_amd import _lib
    dev = torch.device('cuda')
    B, T, stride = k['B'], k['T'], k['stride']
    t = {a: None if k[a] is None else torch.from_numpy(np.ascontiguousarray(k[a])).to(dev)
         for a in ('out', 'yobs', 'noise', 'aux', 'err', 'obs_id', 'set_scale', 'set_logdet')}
    p = {a: None if v is None else v.data_ptr() for a, v in t.items()}
    desc = (_lib.LikeTarget * T)(*[_lib.LikeTarget(*tg) for tg in k['targets']])
    need = lib.bh_likelihood_workspace_bytes(B, T, desc)
    groups = max([((tg.n + 15) // 16 + 3) // 4 for tg in k['targets'] if tg.cov == hp.COV_GAUSS] or [0])
    assert need == T * B * 2 * 8 * groups
    assert mode != 'staged' or need > 0
    ws = torch.full((max(need // 8, 1),), float('nan'), dtype=torch.float64, device=dev)
    wsp, wsn = (ws.data_ptr(), need) if mode != 'nows' and need else (None, 0)
    logL = torch.full((B,), float('nan'), dtype=torch.float64, device=dev)
    mis = torch.full((B, T + 1), float('nan'), dtype=torch.float64, device=dev)
    sets_api = k['nsets'] > 1 or k['obs_id'] is not None or k['set_scale'] is not None
    for st in ((1, 2) if mode == 'staged' else (3,)):
        if sets_api:
            rc = lib.bh_likelihood_sets(st, B, T, desc, p['out'], stride, p['err'], k['nflags'], k['nsets'], p['obs_id'],
                                        p['yobs'], stride, p['set_scale'], p['set_logdet'], p['noise'], p['aux'],
                                        logL.data_ptr(), mis.data_ptr(), wsp, wsn, None)
        elif mode == 'staged':
            rc = lib.bh_likelihood_stage(st, B, T, desc, p['out'], stride, p['err'], k['nflags'], p['yobs'], p['noise'],
                                         p['aux'], logL.data_ptr(), mis.data_ptr(), wsp, wsn, None)
        else:
            rc = lib.bh_likelihood_batch(B, T, desc, p['out'], stride, p['err'], k['nflags'], p['yobs'], p['noise'],
                                         p['aux'], logL.data_ptr(), mis.data_ptr(), wsp, wsn, None)
        _lib.check(rc)
    torch.cuda.synchronize()
    return logL.cpu().numpy(), mis.cpu().numpy()


def same_class(got, want, bound):
    """got against a reference value that may be NaN or +-Inf: NaN for NaN, the same infinity for an infinity,
    within the bound otherwise."""
    want = float(want)
    if np.isnan(want):
        return bool(np.isnan(got))
    if np.isinf(want):
        return got == want
    return abs(hp.LD(got) - hp.LD(want)) <= bound


@pytest.mark.gpu
@pytest.mark.parametrize('name', hp.CASE_NAMES)
def test_gpu_likelihood_within_derived_bounds(lib, name):
    """Every compared row is within the derived bounds of the extended-precision value in logL and in every
    misfit column; failed rows (an err flag in any column, a set index out of range) are exactly -1e15 / 1e15.

    Isolation (cases poison_*): a row that holds a NaN, +Inf or -Inf in one column leaves all other rows -- the
    15 models of its matrix-core tile, the 7 of its like_kernel workgroup -- inside their bounds.  The row itself
    is compared with what the reference's formulas give for such data (likelihood_hp.evaluate on the same row).
    Found on the MI355X, the same with and without the workspace and staged, and equal to the reference in all
    27 rows: a NaN gives logL = NaN and a NaN misfit of its target and of the sum column; +-Inf in a dense target
    gives logL = NaN (infinite terms of both signs) with misfit and sum column +Inf; +-Inf in an exponential-law
    target gives logL = NaN in 5 rows and -Inf in one (row 94: both cross terms on the side of the diagonal
    term), misfit and sum column +Inf; the misfits of the row's clean targets stay inside their bounds."""
    k = hp.build_case(hp.CASES[hp.CASE_NAMES.index(name)])
    ref = hp.reference(k)
    clean = np.ones(k['B'], dtype=bool)
    clean[k['poisoned']] = False
    for mode in k['case']['modes']:
        logL, mis = run_gpu(lib, k, mode)
        rl, rm, msg = hp.judge(k, logL, mis, ref=ref)
        print('HP-RATIO gpu %s %s forms=%s rows=%d/%d logL=%.3f misfit=%.3f'
              % (name, mode, ','.join(hp.FORM_NAMES[f] for f in k['case']['forms']), len(k['rows']), k['B'], rl, rm))
        assert msg is None, (mode, msg)
        assert np.isfinite(logL[clean]).all() and np.isfinite(mis[clean]).all(), mode
        if k['poisoned']:
            pl, pm, pbl, pbm = hp.reference(k, rows=np.array(k['poisoned']))
            for i, b in enumerate(k['poisoned']):
                print('HP-POISON %s %s row %d: logL %r (reference %r) misfits %r (reference %r)'
                      % (name, mode, b, logL[b], float(pl[i]), mis[b].tolist(), pm[i].astype(float).tolist()))
                assert not np.isfinite(logL[b]) and same_class(logL[b], pl[i], pbl[i]), (mode, b)
                for t in range(k['T'] + 1):
                    assert same_class(mis[b, t], pm[i, t], pbm[i, t]), (mode, b, t)
