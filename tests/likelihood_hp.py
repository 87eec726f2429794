"""Extended-precision reference of the fused likelihood, its error bounds, and the table of cases that
tests/test_likelihood_hp.py (CPU) and tests/test_gpu_likelihood_hp.py (GPU) share.  No torch.

What is restated: JointTarget.evaluate (src/Targets.py:314-347) with the covariance models of Valuation
(src/Targets.py:105-173) and get_rms (src/Targets.py:100-103), in np.longdouble (x87: 64-bit mantissa), for
exactly the inputs bh_likelihood_batch / _stage / _sets receive: out, yobs (or the per-set tables), noise, aux,
the LikeTarget descriptors, the err flags and obs_id.  Per target of n points, with d = ymod - yobs:

    NOCORR         q = sum d_i^2                                   C^-1 = I / sigma^2           (:113-114)
    NOCORR_SCALED  q = sum d_i^2 / se_i                            C^-1 = diag(1/(se sigma^2))  (:125-128)
    EXP            q = sum w_i d_i^2 - 2 corr sum d_i d_{i+1},     w = 1 + corr^2, w_0 = w_{n-1} = 1 (:133-136)
                   madist = q / (sigma^2 (1 - corr^2)),  logdet += (n - 1) log(1 - corr^2)      (:145-146)
    GAUSS          q = d^T R^-1 d with the fixed dense R^-1 of aux  (:171-172)
    madist = q / sigma^2,  logdet = 2 n log(sigma) + logdet_extra                               (:114,128,172)
    logL  += -0.5 (n log(2 pi) + logdet) - madist / 2                                           (:341-344)
    misfit_t = sqrt(mean(d^2)), last column their sum                                           (:102,310-312)
    any err flag set, or a set index outside [0, nsets): logL = -1e15, every misfit 1e15        (:325-328)

RESIDUALS.  d = out - yobs is formed in fp64 first -- the one IEEE subtraction the device performs -- and only
then widened: the cancellation in that subtraction is the forward kernels' business, not the likelihood's.

BOUNDS (derived, not tuned).  u = 2^-53; every bound is first order in u.  The reference's own error is
2^-11 of each figure (64- against 53-bit mantissa) and is not added.

  q      Any fp64 evaluation of a sum of products -- any order, tree or chain, fused or not -- is within
         gamma * sum|terms| of the exact value, gamma = (roundings per term + depth of the summation) u.
           closed forms: gamma = (n + 6) u over the form's own terms (d_i^2; d_i^2/se_i; w_i d_i^2 and
             2 corr d_i d_{i+1}).  A term has at most 4 roundings (corr^2, 1 + corr^2, d_i^2, their product), a
             wave adds <= ceil(2n/64) terms per lane and 6 shuffle levels, a serial sum n - 1.
           dense form:   gamma = (2n + 4) u over |d|^T |R^-1| |d|: n fused or unfused multiply-adds for
             y_j = sum_i d_i R_ij, one product y_j d_j, n additions over j, plus the partial sums of the
             column-tile groups.
  1-c^2  fl(1 - fl(c^2)) = (1 - c^2 (1 + e1)) (1 + e2): relative error <= u (1 + c^2) / (1 - c^2) =: eps_c.
         It enters madist through 1 / (sigma^2 (1 - c^2)) relatively, and log(1 - c^2) absolutely: the
         log-determinant moves by (n - 1) eps_c.  At |corr| = 0.999999 eps_c = 1e6 u.
  madist |madist - exact| <= bound(q) / denominator + (eps_c + 4 u) |madist|  (sigma^2, the product with
         1 - c^2, the division, one spare).
  logL   per target: bound(madist) / 2 + (n - 1) eps_c / 2
                     + (LOG_ULP + 4) u (|n log 2 pi| + |2 n log sigma| + |logdet_extra| + |madist / 2|),
         logdet_extra being (n - 1) log(1 - c^2) for EXP.  Each magnitude carries the error of its logarithm
         (LOG_ULP), the rounding of its product with n, and at most three additions on the way to the target's
         part.  Summing T parts adds T u sum(magnitudes).
         LOG_ULP = 3: the device `log` is OCML's, which implements the accuracy table of the OpenCL C
         specification (7.4, relative error as ULPs: log <= 3 ulp in double precision); the HIP math API
         reference lists the same function with a maximum error of 1 ulp.  The larger documented figure is used.
         log(2 pi) takes the fp64 product 2 * 3.141592653589793 as its argument, as device and reference do.
  misfit (n + 4) u relative per target: n roundings in sum d^2 (positive terms: the bound is relative), the
         division by n, the square root (which halves what came before), two spare.  The sum column adds the
         targets' bounds and T u times itself.
  failed rows: exactly -1e15 / 1e15, bound 0.

tests/test_likelihood_hp.py proves the restatement against the golden vectors and the host mirror, and that a
plain fp64 numpy evaluation of every case below stays inside these bounds (they are not too tight for a
correct implementation).
"""
import collections
import functools
import os
import re
import zlib

import numpy as np

LD = np.longdouble
U = LD(2) ** -53
LOG_ULP = 3
COV_NOCORR, COV_NOCORR_SCALED, COV_EXP, COV_GAUSS = 0, 1, 2, 3
FORM_NAMES = {0: 'nocorr', 1: 'scaled', 2: 'exp', 3: 'gauss'}
FAIL_LOGL, FAIL_MISFIT = -1e15, 1e15

Target = collections.namedtuple('Target', 'n off cov aux_off logdet_extra')


def evaluate(out, yobs, noise, aux, targets, err=None, obs_id=None, nsets=1, set_scale=None, set_logdet=None,
             rows=None):
    """(logL[R], misfits[R, T+1], bound_logL[R], bound_misfits[R, T+1]) in np.longdouble for the rows `rows`
    (all when None) of out[B, out_stride].  yobs[nsets, set_stride] (or one row), noise[B, 2T], aux flat,
    err[B, nflags] or None, obs_id[B] or None, set_scale[nsets, set_stride] / set_logdet[nsets, T] or None."""
    out = np.asarray(out, dtype=np.float64)
    yobs = np.atleast_2d(np.asarray(yobs, dtype=np.float64))
    noise = np.asarray(noise, dtype=np.float64)
    rows = np.arange(out.shape[0]) if rows is None else np.asarray(rows)
    R, T = len(rows), len(targets)
    sets = np.zeros(R, dtype=np.int64) if obs_id is None else np.asarray(obs_id)[rows].astype(np.int64)
    bad = (sets < 0) | (sets >= nsets)
    if err is not None and np.asarray(err).size:
        bad |= (np.asarray(err).reshape(out.shape[0], -1)[rows] != 0).any(axis=1)
    sets = np.where(bad, 0, sets)
    log2pi = np.log(LD(2 * np.pi))
    K = LD(LOG_ULP + 4)
    logL, bl, mags = np.zeros(R, LD), np.zeros(R, LD), np.zeros(R, LD)
    mis, bm = np.zeros((R, T + 1), LD), np.zeros((R, T + 1), LD)
    with np.errstate(all='ignore'):
        for t, tg in enumerate(targets):
            n, sl = tg.n, slice(tg.off, tg.off + tg.n)
            d = (out[rows, sl] - yobs[sets, sl]).astype(LD)          # fp64 subtraction, then widened
            corr, sigma = noise[rows, 2 * t].astype(LD), noise[rows, 2 * t + 1].astype(LD)
            s2 = (d * d).sum(axis=1)
            denom, eps_c, extra = sigma * sigma, LD(0), LD(tg.logdet_extra)
            gamma = (n + 6) * U
            if tg.cov == COV_NOCORR:
                q = qabs = s2
            elif tg.cov == COV_NOCORR_SCALED:
                if set_scale is not None:
                    se = np.asarray(set_scale, dtype=np.float64)[sets, sl].astype(LD)
                    extra = np.asarray(set_logdet, dtype=np.float64)[sets, t].astype(LD)
                else:
                    se = np.asarray(aux, dtype=np.float64)[tg.aux_off:tg.aux_off + n].astype(LD)[None, :]
                q = qabs = (d * d / se).sum(axis=1)
            elif tg.cov == COV_EXP:
                w = np.repeat((1 + corr * corr)[:, None], n, axis=1)
                w[:, 0] = w[:, -1] = 1
                cross = d[:, :-1] * d[:, 1:]
                q = (w * d * d).sum(axis=1) - 2 * corr * cross.sum(axis=1)
                qabs = (w * d * d).sum(axis=1) + 2 * np.abs(corr) * np.abs(cross).sum(axis=1)
                om = 1 - corr * corr
                eps_c = U * (1 + corr * corr) / om
                denom = denom * om
                extra = (n - 1) * np.log(om)
            else:
                Rinv = np.asarray(aux, dtype=np.float64)[tg.aux_off:tg.aux_off + n * n].reshape(n, n).astype(LD)
                q = (np.matmul(d, Rinv) * d).sum(axis=1)
                qabs = (np.matmul(np.abs(d), np.abs(Rinv)) * np.abs(d)).sum(axis=1)
                gamma = (2 * n + 4) * U
            madist = q / denom
            b_mad = gamma * qabs / denom + (eps_c + 4 * U) * np.abs(madist)
            logdet_sigma = (2 * n) * np.log(sigma)
            logL = logL + (-0.5 * (n * log2pi + (logdet_sigma + extra)) - madist / 2)
            mag = n * log2pi + np.abs(logdet_sigma) + np.abs(extra) + np.abs(madist / 2)
            mags = mags + mag
            bl = bl + b_mad / 2 + (n - 1) * eps_c / 2 + K * U * mag
            mis[:, t] = np.sqrt(s2 / n)
            bm[:, t] = (n + 4) * U * mis[:, t]
        mis[:, T] = mis[:, :T].sum(axis=1)
        bm[:, T] = bm[:, :T].sum(axis=1) + T * U * mis[:, T]
        bl = bl + T * U * mags
    logL[bad], bl[bad] = FAIL_LOGL, 0
    mis[bad], bm[bad] = FAIL_MISFIT, 0
    return logL, mis, bl, bm


# ------------------------------------------------------------------------------------------------ the cases
def _source_constant(name, pattern):
    """An integer the kernels are built with, read from the library's sources so that the table follows them."""
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'bayhunter_amd', 'csrc', name)
    with open(src) as fh:
        m = re.search(pattern, fh.read())
    assert m, '%s no longer holds /%s/: the case table cannot find the edge it probes' % (name, pattern)
    return int(m.group(1))


# largest batch that takes the split form of the dense product (launch_like), longest target, models per workgroup
SWITCH = _source_constant('like_kernel.hip', r'A\.B\s*<=\s*(\d+)')
LIKE_NMAX = _source_constant('kernels.h', r'constexpr\s+int\s+LIKE_NMAX\s*=\s*(\d+)')
LIKE_M = _source_constant('kernels.h', r'constexpr\s+int\s+LIKE_M\s*=\s*(\d+)')
CLOSED_N = (1, 2, 3, 63, 64, 65, 127, 128, 129, 201, 255, 256, 257, LIKE_NMAX - 1, LIKE_NMAX)
DENSE_N = (1, 15, 16, 17, 63, 64, 65, 201, 208, 209, LIKE_NMAX)
BATCHES = (1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 1000, SWITCH, SWITCH + 1, 40000)
CORRS = (0.0, 0.3, -0.3, 0.9, 0.99, 0.999999, -0.999999)
SIGMAS = (1e-5, 0.012, 2.0)
ALL_MODES = ('ws', 'nows', 'staged')          # with the matrix-core workspace, without, stages 1 then 2
SAMPLE_ABOVE = 2000                           # larger batches are judged on a sample of rows (sample_rows)


@functools.lru_cache(maxsize=None)
def dense_matrix(kind, n):
    """'pinv0.9' / 'pinv0.98': the real pinv(corr**(lag^2), rcond=1e-5) (src/Targets.py:151-156);
    'inv0.9': inv, rcond None (:158); 'asym': a random matrix that is NOT symmetric (a transposed operand shows)."""
    if kind == 'asym':
        return np.random.RandomState(n).normal(size=(n, n)) / n
    corr = float(kind.split('v')[1])
    lag = np.abs(np.subtract.outer(np.arange(n), np.arange(n))).astype(float)
    rmatrix = corr ** (lag ** 2)
    m = np.linalg.pinv(rmatrix, rcond=1e-5) if kind.startswith('pinv') else np.linalg.inv(rmatrix)
    assert np.isfinite(m).all(), (kind, n)
    return np.ascontiguousarray(m)


def _case(name, B, forms, ns, **kw):
    c = dict(name=name, B=B, forms=tuple(forms), ns=tuple(ns), gaps=None, pad=0, nflags=0, failed=(), nsets=1,
             obs=None, tables=False, dense='pinv0.98', noise='std', se='std', aux_pad=0, poison=(), modes=ALL_MODES,
             zero_row=None)
    assert set(kw) <= set(c), kw
    c.update(kw)
    return c


def _cases():
    cs = []
    # 1. target length, closed forms: one target per case, so that an error / bound ratio belongs to one form;
    #    the batch walks through the edge sizes of the 8-model workgroup
    for i, n in enumerate(CLOSED_N):
        for cov in (0, 1, 2):
            cs.append(_case('len_%s_n%d' % (FORM_NAMES[cov], n), BATCHES[(i + cov) % 10], [cov], [n], gaps=[i % 3],
                            pad=(i + cov) % 2, modes=('nows',), noise='edges' if cov == 2 else 'std'))
    # 2. target length and matrix, dense form: matrix-core path, vector path and the two stages
    for i, n in enumerate(DENSE_N):
        kinds = ['pinv0.9', 'pinv0.98', 'asym'] + (['inv0.9'] if n <= 17 else [])
        for j, kind in enumerate(kinds):
            cs.append(_case('dense_%s_n%d' % (kind, n), (37, 64, 65, 17, 130)[(i + j) % 5], [3], [n], gaps=[(i + j) % 4],
                            dense=kind, aux_pad=(i * 7 + j) % 5))
    # 3. batch size: exponential + real dense target at a non-zero offset; above SAMPLE_ABOVE on a sample
    for B in BATCHES:
        cs.append(_case('batch_%d' % B, B, [2, 3], [21, 201], gaps=[2, 3], pad=1, nflags=1,
                        failed=(0, B - 1) if B > 2 else ()))
    # the fused form's other instantiations: 4 and 8 column tiles in one pass (n = 40 and 60 -- three tiles and all
    # four of the group --, n = 100), 12 per pass (n = 1024)
    cs.append(_case('batch_%d_n60' % (SWITCH + 1), SWITCH + 1, [3], [60], dense='asym', modes=('ws', 'staged')))
    cs.append(_case('batch_%d_n40' % (SWITCH + 1), SWITCH + 1, [3], [40], gaps=[1], dense='pinv0.98', modes=('ws', 'staged')))
    cs.append(_case('batch_%d_n100' % (SWITCH + 1), SWITCH + 1, [3], [100], gaps=[2], dense='pinv0.9', modes=('ws', 'staged')))
    cs.append(_case('batch_%d_n%d' % (SWITCH + 1, LIKE_NMAX), SWITCH + 1, [3], [LIKE_NMAX], dense='asym', modes=('ws', 'staged')))
    cs.append(_case('batch_40000_closed', 40000, [0, 1, 2], [65, 21, 129], gaps=[1, 0, 5], modes=('nows',)))
    # 4. layout: 1 to 6 targets, every form in every position (the four rotations), gaps, pad, aux_off, err flags
    order = [0, 1, 2, 3]
    for r in range(4):
        rot = order[r:] + order[:r]
        cs.append(_case('layout_rot%d' % r, 29 + r, rot, [(33, 21, 65, 201)[f] for f in rot], gaps=[3, 0, 7, 1],
                        pad=r, aux_pad=r + 1, nflags=(0, 1, 3, 3)[r], failed=(0, LIKE_M - 1, LIKE_M, 2 * LIKE_M - 1, 2 * LIKE_M, 28 + r) if r else ()))
    for T in (1, 2, 3, 5, 6):
        forms = [(3, 2, 1, 0, 3, 2)[k] for k in range(T)]
        cs.append(_case('layout_T%d' % T, 64 + T, forms, [(130, 40, 21, 7, 17, 1)[k] for k in range(T)],
                        gaps=[(k * 5 + 1) % 4 for k in range(T)], pad=T, aux_pad=3, nflags=(T % 2) * 3,
                        failed=(7, 8, 63, 64, 63 + T) if T % 2 else (), dense='pinv0.9'))
    # 5. noise edges: every (corr, sigma) pair, residuals from 1e-8 to 1e2, a row of exact zeros
    cs.append(_case('noise_edges', 3 * len(CORRS) * len(SIGMAS) + 1, [2, 2, 0, 3], [201, 2, 64, 65], gaps=[0, 1, 0, 2],
                    noise='edges', zero_row=5))
    cs.append(_case('noise_edges_n1', 45, [2, 1], [1, 3], noise='edges', zero_row=44, modes=('nows',)))
    # 6. scaled errors: exact 1.0 and ratios up to 1e6, through aux and through the per-set tables
    cs.append(_case('scaled_wide_aux', 77, [1, 1], [21, 130], gaps=[1, 2], se='wide', aux_pad=2, modes=('nows',)))
    cs.append(_case('scaled_wide_tables', 77, [1, 0, 1], [21, 9, 130], gaps=[1, 0, 2], se='wide', nsets=7, obs='random',
                    tables=True, modes=('nows',)))
    cs.append(_case('scaled_tables_one_set', 19, [1, 3], [21, 40], se='wide', nsets=1, tables=True))
    # 7. observation sets
    for nsets, obs, B in ((1, 'random', 100), (7, 'random', 333), (7, 'oob', 333), (1000, 'random', 1500),
                          (1000, 'own', 1000), (1000, 'oob', 1000)):
        cs.append(_case('sets_%d_%s' % (nsets, obs), B, [2, 1, 3], [21, 11, 65], gaps=[0, 2, 1], pad=2, nsets=nsets,
                        obs=obs, tables=True, nflags=1, failed=(8, B - 1)))
    # 8. isolation: NaN, +Inf, -Inf at the first, middle and last column of one model per 16-model tile
    for name, forms, ns, tt in (('dense', [0, 3], [21, 201], 1), ('dense209', [3], [209], 0), ('exp', [2, 3, 1], [65, 40, 9], 0)):
        n = ns[tt]
        poison = tuple((16 * k + (0, 15, 7, 8, 1, 14, 5, 10, 3)[k], tt, (0, n // 2, n - 1)[k % 3],
                        (np.nan, np.inf, -np.inf)[k // 3]) for k in range(9))
        cs.append(_case('poison_' + name, 160, forms, ns, gaps=[1] * len(ns), poison=poison,
                        modes=ALL_MODES if 3 in forms else ('nows',)))
    names = [c['name'] for c in cs]
    assert len(set(names)) == len(names)
    return cs


CASES = _cases()
CASE_NAMES = [c['name'] for c in CASES]


def sample_rows(B, seed=0):
    """Rows of a large batch that are compared: the first and last 64, the 64 on each side of the split/fused
    switch, and 200 random ones drawn from the rows outside those (at most 456 in all)."""
    if B <= SAMPLE_ABOVE:
        return np.arange(B)
    edge = np.unique(np.r_[0:64, B - 64:B, max(SWITCH - 64, 0):min(SWITCH + 64, B)])
    rest = np.setdiff1d(np.arange(B), edge)
    return np.unique(np.r_[edge, np.random.RandomState(seed).choice(rest, 200, replace=False)])


def build_case(c):
    """The arrays of a case, as the C ABI takes them (host side, fp64 / int32), plus the rows to compare."""
    rs = np.random.RandomState(zlib.crc32(c['name'].encode()) & 0x7fffffff)
    B, T, nsets = c['B'], len(c['forms']), c['nsets']
    gaps = c['gaps'] or [0] * T
    offs, pos = [], 0
    for g, n in zip(gaps, c['ns']):
        offs.append(pos + g)
        pos += g + n
    stride = pos + c['pad']
    yobs = rs.standard_normal((nsets, stride))
    scale = 10.0 ** rs.uniform(-3, 0, B)
    noise = np.empty((B, 2 * T))
    for t in range(T):
        noise[:, 2 * t] = rs.uniform(-0.95, 0.95, B)
        noise[:, 2 * t + 1] = rs.uniform(0.005, 2.0, B)
    if c['noise'] == 'edges':
        pairs = [(a, s) for a in CORRS for s in SIGMAS]
        for t in range(T):
            k = (np.arange(B) + 5 * t) % len(pairs)
            noise[:, 2 * t] = np.array([p[0] for p in pairs])[k]
            noise[:, 2 * t + 1] = np.array([p[1] for p in pairs])[k]
        scale = 10.0 ** (np.arange(B) * 7 % 11 - 8.0)              # 1e-8 ... 1e2
    obs_id = None
    if c['obs'] == 'random':
        obs_id = rs.randint(0, nsets, B).astype(np.int32)
    elif c['obs'] == 'own':
        obs_id = rs.permutation(B).astype(np.int32) % nsets
    elif c['obs'] == 'oob':
        obs_id = rs.randint(0, nsets, B).astype(np.int32)
        obs_id[[0, 7, 17, B - 2]] = [-1, nsets, 2 ** 31 - 1, -2 ** 31]
    out = rs.standard_normal((B, stride))
    out *= scale[:, None]
    out += yobs[0] if obs_id is None else yobs[np.clip(obs_id, 0, nsets - 1)]
    if c['zero_row'] is not None:
        out[c['zero_row']] = yobs[0] if obs_id is None else yobs[np.clip(obs_id[c['zero_row']], 0, nsets - 1)]
    aux, targets = [rs.standard_normal(c['aux_pad'])], []
    set_scale = np.full((nsets, stride), np.nan) if c['tables'] else None
    set_logdet = np.full((nsets, T), np.nan) if c['tables'] else None
    aux_off = c['aux_pad']
    for t, (cov, n, off) in enumerate(zip(c['forms'], c['ns'], offs)):
        extra, a = 0.0, None
        if cov == COV_NOCORR_SCALED:
            def draw():
                # np.prod(se) must stay finite: the reference's log(prod(scaled_err)) overflows to inf beyond that
                # (src/Targets.py:128), which is a property of its formula and no business of the kernel
                se = rs.uniform(1.0, 4.0 if n <= 300 else 1.6, n)
                if c['se'] == 'wide':
                    se = 10.0 ** rs.uniform(0, 1, n)
                    se[rs.choice(n, n // 8 + 1, replace=False)] = 10.0 ** rs.uniform(1, 6, n // 8 + 1)
                se[rs.randint(n)] = 1.0                             # yerr / yerr.min(): the smallest is exactly 1
                if c['se'] == 'wide' and n > 1:
                    se[(np.argmin(se) + 1) % n] = 1e6
                return se
            a = draw()
            extra = float(np.log(np.prod(a)))                       # as targets.batch_layout hands it over
            if c['tables']:
                for s in range(nsets):
                    se = draw()
                    set_scale[s, off:off + n] = se
                    set_logdet[s, t] = np.log(np.prod(se))
        elif cov == COV_GAUSS:
            a = dense_matrix(c['dense'], n).ravel()
            extra = 1.25 + t
        targets.append(Target(n, off, cov, aux_off if a is not None else 0, extra))
        if a is not None:
            aux.append(a)
            aux_off += a.size
    aux = np.ascontiguousarray(np.concatenate(aux + [np.zeros(1)]))
    err = None
    if c['nflags']:
        err = np.zeros((B, c['nflags']), dtype=np.int32)
        for k, b in enumerate(c['failed']):
            err[b, k % c['nflags']] = 1 + k
    for b, t, col, val in c['poison']:
        out[b, offs[t] + col] = val
    return dict(case=c, B=B, T=T, stride=stride, out=out, yobs=yobs, noise=noise, aux=aux, targets=targets, err=err,
                nflags=c['nflags'], nsets=nsets, obs_id=obs_id, set_scale=set_scale, set_logdet=set_logdet,
                rows=sample_rows(B), poisoned=sorted(set(p[0] for p in c['poison'])))


def reference(k, rows=None):
    return evaluate(k['out'], k['yobs'], k['noise'], k['aux'], k['targets'], err=k['err'], obs_id=k['obs_id'],
                    nsets=k['nsets'], set_scale=k['set_scale'], set_logdet=k['set_logdet'],
                    rows=k['rows'] if rows is None else rows)


def judge(k, logL, mis, ref=None):
    """Compare logL[B], mis[B, T+1] of an implementation with the reference on the case's rows.  Returns
    (worst logL error / bound, worst misfit error / bound, message or None); rows holding a NaN or Inf of their
    own (case['poison']) are left to the caller.  A zero bound asks for equality."""
    rows = k['rows']
    rl, rm, bl, bm = reference(k) if ref is None else ref
    keep = ~np.isin(rows, k['poisoned'])
    with np.errstate(invalid='ignore'):
        el = np.abs(np.asarray(logL)[rows].astype(LD) - rl)[keep]
        em = np.abs(np.asarray(mis)[rows].astype(LD) - rm)[keep]
    bl, bm, rws = bl[keep], bm[keep], rows[keep]
    msg = None
    okl, okm = el <= bl, (em <= bm).all(axis=1)           # a NaN fails both
    if not okl.all():
        i = int(np.argmin(okl))
        msg = '%s: logL of row %d is %.6e from the reference %.17g, bound %.3e (%d rows outside)' % (
            k['case']['name'], rws[i], float(el[i]), float(rl[keep][i]), float(bl[i]), int((~okl).sum()))
    elif not okm.all():
        i = int(np.argmin(okm))
        msg = '%s: misfits of row %d are %s from the reference %s, bounds %s' % (
            k['case']['name'], rws[i], em[i].astype(float), rm[keep][i].astype(float), bm[i].astype(float))
    def worst(e, b):
        with np.errstate(all='ignore'):
            r = np.where(b > 0, e / b, np.where(e == 0, 0.0, np.inf)).astype(np.float64)
        return float(np.max(np.nan_to_num(r, nan=np.inf), initial=0.0))
    return worst(el, bl), worst(em, bm), msg
