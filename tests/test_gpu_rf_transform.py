"""Phase 4 of rf_kernel on the GPU, per call (bh_selftest_rf_transform: the kernel of csrc/rf_probe.hip, which runs
rf_kernel's statements from "P4" on with rf_kernel's functions -- rf_block_fft of rf_fft.h among them -- in rf_kernel's
workgroup: 256 threads striding over M buffers at the pitch of rf_layout, one barrier per pass).

a. Bit for bit against the host twin (tests/hostsim/rf_transform_sim.cpp), which tests/test_rf_transform.py holds to
   (16 log2 n + 4) u ||y||_2 of an extended-precision reference: every accepted length, the full-band spectra of
   tests/rf_transform_cases.py, single and paired, four workgroup shapes (two with a partial last workgroup, one whose
   pitch the layer records set), three output lengths.  A shape that needs more than 160 KiB of LDS is refused with
   BH_ERR_ARG, and that is asserted.
b. A buffer's bits depend neither on M, on B, on its slot in the workgroup nor on a NaN buffer next to it.
c. bh_synrf's three traces against the oracle at the lengths the GPU tier did not run: 8, 64, 2048, 4096
   (tests/test_gpu_rf_floor.py::test_transform_lengths runs bh_rf_batch at all ten)."""
import functools

import numpy as np
import pytest

import rf_transform_cases as tc
from tolerances import TOL_RF

pytestmark = pytest.mark.gpu

SHAPES = [(10, 1, 1), (10, 3, 7), (10, 8, 17), (100, 2, 5)]           # (Lmax, M, B)
FORMS = ['single', 'paired']


@functools.lru_cache(maxsize=None)
def _specs(n, form):
    if form == 'single':
        return [(name, x) for name, x in tc.spectra(n)]
    return [(name, np.stack((x1, x2))) for name, x1, x2 in tc.pairs(n)]


@functools.lru_cache(maxsize=None)
def _twin(n, form, Lmax):
    """the host twin's full-length output of every spectrum, once per (length, form, Lmax)"""
    return [np.atleast_2d(tc.host(n, x, Lmax=Lmax)) for name, x in _specs(n, form)]


def _run(lib, n, Lmax, M, specs, nout, paired):
    from bayhunter_amd import _lib
    rc, out = tc.device_rc(lib, n, Lmax, M, np.stack(specs), nout, paired)
    _lib.check(rc)
    return out


@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('n', tc.LENGTHS)
def test_device_equals_the_host_twin_bit_for_bit(lib, n, form):
    from bayhunter_amd import _lib
    paired = form == 'paired'
    specs = _specs(n, form)
    N = len(specs)
    bad = calls = 0
    refused = []
    for Lmax, M, B in SHAPES:
        if tc.lds_bytes(n, Lmax, M, paired) > tc.LDS_LIMIT:
            rc, _ = tc.device_rc(lib, n, Lmax, M, np.stack([specs[k % N][1] for k in range(B)]), 1, paired)
            assert rc == _lib.BH_ERR_ARG, (n, form, Lmax, M, B, rc)
            refused.append((Lmax, M, B))
            continue
        want = _twin(n, form, Lmax)
        for nout in sorted({1, min(201, n), n}):
            for start in range(0, N, B):
                ids = [(start + k) % N for k in range(B)]
                got = _run(lib, n, Lmax, M, [specs[i][1] for i in ids], nout, paired)
                calls += 1
                for k, i in enumerate(ids):
                    d = int((got[k].view(np.int64) != np.ascontiguousarray(want[i][:, :nout]).view(np.int64)).sum())
                    assert d == 0, (n, form, (Lmax, M, B), nout, specs[i][0], 'buffer %d' % k, d)
                    bad += d
    print('gpu rf transform: n = %d %s, %d values differ from the host twin over %d calls; refused for LDS: %s'
          % (n, form, bad, calls, refused))
    assert bad == 0
    # what is refused is what does not fit, and the smallest shape always runs
    assert (10, 1, 1) not in refused


def _fitting(n, paired, shapes):
    return [(M, B) for M, B in shapes if tc.lds_bytes(n, 10, M, paired) <= tc.LDS_LIMIT]


@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('n', tc.LENGTHS)
def test_bits_do_not_depend_on_M_B_or_the_slot(lib, n, form):
    """The 'normal' spectrum alone in a launch, then among other spectra at slot 0 of the first workgroup, at a middle
    slot of a middle workgroup and in the partial last workgroup."""
    paired = form == 'paired'
    specs = _specs(n, form)
    key = [k for k, (name, x) in enumerate(specs) if name.startswith('normal')][0]
    x = specs[key][1]
    others = [s for k, (nm, s) in enumerate(specs) if k != key]
    alone = _run(lib, n, 10, 1, [x], n, paired)[0]
    assert np.isfinite(alone).all()
    shapes = _fitting(n, paired, [(1, 3), (2, 5), (3, 7), (8, 17)])
    assert shapes
    runs = 0
    for M, B in shapes:
        for slot in sorted({0, M + M // 2 if M + M // 2 < B else B // 2, B - 1}):
            batch = [others[(3 * k + slot) % len(others)] for k in range(B)]
            batch[slot] = x
            got = _run(lib, n, 10, M, batch, n, paired)
            assert np.array_equal(got[slot].view(np.int64), alone.view(np.int64)), (n, form, M, B, slot)
            runs += 1
    print('gpu rf transform: n = %d %s, the same bits in %d launches of shapes (M, B) %s' % (n, form, runs, shapes))


@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('n', tc.LENGTHS)
def test_nan_buffer_leaves_its_neighbours_alone(lib, n, form):
    """A buffer of NaN, and one with a single NaN bin, in the middle of a workgroup: itself NaN (every sample, since every
    sample sums every bin), the finite buffers of the launch the bits they have without it."""
    paired = form == 'paired'
    shapes = _fitting(n, paired, [(8, 17), (3, 7), (2, 5)])
    if not shapes:
        # one buffer per workgroup is all that fits (the paired form at 4096): there are no neighbours in LDS
        assert n == 4096 and paired
        shapes = [(1, 3)]
    M, B = shapes[0]
    specs = _specs(n, form)
    batch = [specs[(5 * k + 2) % len(specs)][1] for k in range(B)]
    good = _run(lib, n, 10, M, batch, n, paired)
    assert np.isfinite(good).all()
    for kind in ('all', 'one bin'):
        slot = 1 if M > 1 else 0
        poisoned = [b.copy() for b in batch]
        if kind == 'all':
            poisoned[slot][...] = np.nan
        else:
            poisoned[slot][..., n // 4] = np.nan
        got = _run(lib, n, 10, M, poisoned, n, paired)
        assert np.isnan(got[slot]).all(), (n, form, kind)
        keep = np.arange(B) != slot
        assert np.array_equal(got[keep].view(np.int64), good[keep].view(np.int64)), (n, form, kind)
    print('gpu rf transform: n = %d %s, NaN buffer at slot 1 of %d in workgroups of %d: neighbours unchanged' % (n, form, B, M))


@pytest.mark.parametrize('nsamp', [8, 64, 2048, 4096])
def test_synrf_traces_at_the_shortest_and_longest_lengths(lib, oracle, nsamp):
    """bh_synrf's fz, fr, rf (the trace form: the single transform, then the paired one; at 4096 one model takes 131 KB
    of LDS) against the oracle, as test_gpu_parity.py::test_synrf_dropin_returns_all_three_traces compares them at 256
    and 512, at its tolerance.  tshift as test_gpu_rf_floor.py::test_transform_lengths shortens it for short traces."""
    from bayhunter_amd import _lib
    from bayhunter_amd.synthetic import draw_models
    H, VP, VS, RHO, nl = draw_models(2, (3, 9), seed=17, sorted_vs=False)
    tshift = min(5.0, nsamp / 25.0)
    worst = 0.0
    for b in range(2):
        n = nl[b]
        z = np.ascontiguousarray(np.concatenate(([0], np.cumsum(H[b, :n])[:-1])))
        vp, vs, rh = (np.ascontiguousarray(a[b, :n]) for a in (VP, VS, RHO))
        qp, qs = np.full(n, 450.), np.full(n, 200.)
        if b >= 1:
            qp, qs = qp + 35. * np.arange(n), qs - 12. * np.arange(n)
        for wn in (0, 1):
            want = oracle.synrf(z, vp, vs, rh, qp, qs, 6.4, 1.5, nsamp, 5.0, tshift, 3.1, 0.27, wn)
            fz, fr, rf = np.zeros(nsamp), np.zeros(nsamp), np.zeros(nsamp)
            _lib.check(lib.bh_synrf(nsamp, 5.0, tshift, 6.4, 1.5, 3.1, 0.27, wn, n, z.ctypes.data,
                                    vp.ctypes.data, vs.ctypes.data, rh.ctypes.data, qp.ctypes.data,
                                    qs.ctypes.data, fz.ctypes.data, fr.ctypes.data, rf.ctypes.data))
            for name, got, w in zip(('fz', 'fr', 'rf'), (fz, fr, rf), want):
                assert np.isfinite(w).all() and np.abs(w).max() > 0
                rel = np.abs(got - w).max() / max(1.0, np.abs(w).max())
                worst = max(worst, rel)
                print('gpu rf transform: bh_synrf nsamp = %d model %d waveno %d %s: %.3e of the scale' % (nsamp, b, wn, name, rel))
                assert rel <= TOL_RF, (nsamp, b, wn, name, rel)
    print('gpu rf transform: bh_synrf nsamp = %d worst %.3e (tolerance %.1e)' % (nsamp, worst, TOL_RF))
