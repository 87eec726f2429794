"""Phase 4 of rf_kernel -- the Hermitian extension, the bit reversal with its 1/sqrt(n) scale, the radix-2 stage of an
odd log2 n, the radix-4 passes, the scaled output and the trace form's paired transform -- as the host twin of
bh_selftest_rf_transform runs it (tests/hostsim/rf_transform_sim.cpp: the functions of rf_core.h the device runs),
at every accepted length, on full-band spectra, against an extended-precision restatement of the reference's lines and
the bound derived in tests/rf_transform_cases.py: (16 log2 n + 4) u ||y||_2.  The GPU tier
(tests/test_gpu_rf_transform.py) then holds the device to this twin bit for bit.

Each test prints its worst figure in units of u ||y||_2 before it asserts.  Host twin against long double, worst
spectrum per length (single form / paired form), as measured when the tests were written:

    n        8     16    32    64    128   256   512   1024  2048  4096
    single   1.22  1.05  1.30  1.50  1.97  2.29  2.57  2.79  3.11  3.33
    paired   2.16  1.68  2.42  3.09  3.25  3.77  3.98  4.54  4.77  5.38
    bound    52    68    84    100   116   132   148   164   180   196

(the bound is the theorem's worst case; the measured growth is the sqrt(log2 n) of rounding errors that do not conspire).
"""
import functools

import numpy as np
import pytest

import rf_transform_cases as tc
from rf_transform_cases import LD, U


@functools.lru_cache(maxsize=None)
def _cases(n):
    """per length, computed once: [(name, spec, y long double, twin output)] single and paired"""
    single = [(name, x, tc.reference(x), tc.host(n, x)) for name, x in tc.spectra(n)]
    paired = [(name, np.stack((x1, x2)), tc.reference(np.stack((x1, x2))), tc.host(n, np.stack((x1, x2))))
              for name, x1, x2 in tc.pairs(n)]
    return single, paired


def test_twiddle_table_is_within_the_derived_error():
    """mu of the bound: |tw[l + m] - exp(i pi m / l)| <= 10.3 u at every length, for the table the library's host code
    builds (bh_rf_twiddles: what the device reads and the twin is given) and for rf_fill_twiddles as g++ builds it into the
    twin.  The two builds may differ in the last bit of an entry; the number of such entries is printed."""
    worst, differ = 0.0, 0
    for n in tc.LENGTHS:
        own = np.zeros(2 * n)
        tc.transform_sim().hs_rf_twiddles(n, own.ctypes.data)
        lib_tw = tc.library_table(n)
        differ += int((own.view(np.int64) != lib_tw.view(np.int64)).sum())
        for tw in (lib_tw, own):
            assert tw[0] == 0.0 and tw[1] == 0.0
            l = 1
            while l < n:
                m = np.arange(l)
                ang = tc.PI_LD * m.astype(LD) / LD(l)
                er = tw[2 * (l + m)].astype(LD) - np.cos(ang)
                ei = tw[2 * (l + m) + 1].astype(LD) - np.sin(ang)
                worst = max(worst, float(np.sqrt(er * er + ei * ei).max() / LD(U)))
                l *= 2
    print('rf transform: twiddle tables worst error %.3f u (bound %.1f u; the exact quotient by l gives 7.1 u); %d doubles '
          'differ between the library\'s build and the twin\'s' % (worst, tc.MU_BOUND, differ))
    assert worst <= tc.MU_BOUND


@pytest.mark.parametrize('n', [n for n in tc.LENGTHS if n <= tc.DIRECT_MAX])
def test_long_double_fft_equals_the_direct_sum(n):
    """The two restatements of the reference agree to long-double rounding: per component, |fft - direct| <= (n + 16
    log2 n + 8) 2^-64 sum_j |x[j]| / n -- n additions of the direct sum, Theorem 24.2 for the FFT, the roots' own error."""
    worst = 0.0
    for name, x in tc.spectra(n) + [(nm, np.stack((a, b))) for nm, a, b in tc.pairs(n)]:
        yd, yf = tc.reference(x, direct=True), tc.reference(x)
        full = tc.mirror(x)
        l1 = np.abs(full).sum() if x.ndim == 1 else np.abs(full).sum(axis=-1).sum()
        worst = max(worst, float(np.abs(yd - yf).max() / (LD(2.0) ** -64 * l1 / n)))
    limit = n + 16 * np.log2(n) + 8
    print('rf transform: n = %d long-double FFT against the direct sum, worst %.2f (bound %.0f) x 2^-64 sum|x| / n' % (n, worst, limit))
    assert worst <= limit


@pytest.mark.parametrize('form', ['single', 'paired'])
@pytest.mark.parametrize('n', tc.LENGTHS)
def test_host_twin_is_within_the_bound_of_long_double(n, form):
    cases = _cases(n)[form == 'paired']
    errs = [(tc.error_in_u(got, y), name) for name, x, y, got in cases]
    worst, name = max(errs)
    print('rf transform: n = %d %s, host twin against long double: worst %.3f u ||y||_2 at "%s" (bound %.0f)'
          % (n, form, worst, name, tc.bound_u(n)))
    for e, nm in errs:
        assert e <= tc.bound_u(n), (n, form, nm, e)
    # component by component the same figure
    for name, x, y, got in cases:
        f = y.real if form == 'single' else np.stack((y.real, y.imag))
        comp = float(np.abs(got.astype(LD) - f).max() / (LD(U) * np.sqrt(np.sum(np.abs(y) ** 2))))
        assert comp <= tc.bound_u(n), (n, form, name, comp)


@pytest.mark.parametrize('n', tc.LENGTHS)
def test_radix4_plan_equals_radix2_stages_on_full_band_spectra(n):
    single, paired = _cases(n)
    bad = 0
    for name, x, y, got in single + paired:
        r2 = tc.host(n, x, radix4=False)
        bad += int((r2.view(np.int64) != got.view(np.int64)).sum())
    print('rf transform: n = %d, %d values differ between the radix-4 plan and the radix-2 stages' % (n, bad))
    assert bad == 0


@pytest.mark.parametrize('n', tc.LENGTHS)
def test_scaling_by_a_power_of_two_is_exact(n):
    single, paired = _cases(n)
    bad = 0
    for name, x, y, got in single + paired:
        for s in (2.0 ** 40, 2.0 ** -40):
            bad += int(((tc.host(n, x * s)).view(np.int64) != (got * s).view(np.int64)).sum())
    print('rf transform: n = %d, %d values are not the exact multiple under 2^+-40' % (n, bad))
    assert bad == 0


@pytest.mark.parametrize('n', tc.LENGTHS)
def test_paired_channels_equal_their_single_transforms(n):
    """f1 = single(x1) - (Im x2[0] + (-1)^k Im x2[n/2]) / n and f2 = single(x2) + (Im x1[0] + (-1)^k Im x1[n/2]) / n
    (greens.cpp:175-190 keeps the imaginary parts of the DC and Nyquist bins, which iftr's real part drops).  Both sides
    are within the bound of their own exact value, so they differ by at most bound x u x (||y_pair||_2 + ||y_c||_2)."""
    single, paired = _cases(n)
    by_spec = {x.tobytes(): (y, got) for name, x, y, got in single}
    sign = (-1.0) ** np.arange(n)
    worst = 0.0
    for name, x, y, got in paired:
        for c in (0, 1):
            yc, one = by_spec[x[c].tobytes()]
            o = x[1 - c]
            leak = (LD(o[0].imag) + sign.astype(LD) * LD(o[n // 2].imag)) / LD(n)
            want = one.astype(LD) + (-leak if c == 0 else leak)
            e = np.sqrt(np.sum((got[c].astype(LD) - want) ** 2))
            scale = LD(U) * (np.sqrt(np.sum(np.abs(y) ** 2)) + np.sqrt(np.sum(np.abs(yc) ** 2)))
            worst = max(worst, float(e / scale))
            assert e <= tc.bound_u(n) * scale, (n, name, c, float(e / scale))
    print('rf transform: n = %d paired channel against its single transform: worst %.3f u (||y_pair|| + ||y_c||) (bound %.0f)'
          % (n, worst, tc.bound_u(n)))


def test_probe_kernel_is_built_without_scratch():
    import os
    import sys
    sys.path.insert(0, os.path.join(tc.ROOT, 'tools'))
    from kernel_resources import kernel_resources
    r = kernel_resources('rf_probe.hip')
    assert len(r) == 1 and 'rf_probe_kernel' in list(r)[0], sorted(r)
    assert all(v['scratch'] == 0 and v['lds'] == 0 for v in r.values()), r


def test_selftest_rf_transform_validates_its_arguments(lib):
    """nsamp no power of two in 8 .. 4096, Lmax outside 1 .. 100, M outside 1 .. 8, nout outside 1 .. nsamp, a null
    pointer, more LDS than a launch may take: BH_ERR_ARG before any device work."""
    from bayhunter_amd import _lib
    a, out = np.zeros((8, 2, 2049, 2)), np.zeros((8, 2, 4096))
    pa, po = a.ctypes.data, out.ctypes.data
    bad = [(4, 10, 1, 1, 0, pa, 1, po), (8192, 10, 1, 1, 0, pa, 1, po), (48, 10, 1, 1, 0, pa, 1, po), (0, 10, 1, 1, 0, pa, 1, po),
           (64, 0, 1, 1, 0, pa, 1, po), (64, 101, 1, 1, 0, pa, 1, po), (64, 10, 0, 1, 0, pa, 1, po), (64, 10, 9, 1, 0, pa, 1, po),
           (64, 10, 1, 1, 0, pa, 0, po), (64, 10, 1, 1, 0, pa, 65, po), (64, 10, 1, -1, 0, pa, 1, po),
           (64, 10, 1, 1, 0, None, 1, po), (64, 10, 1, 1, 0, pa, 1, None),
           (4096, 10, 3, 1, 0, pa, 1, po), (4096, 10, 2, 1, 1, pa, 1, po), (2048, 10, 8, 1, 0, pa, 1, po), (1024, 10, 8, 1, 1, pa, 1, po)]
    for args in bad:
        assert lib.bh_selftest_rf_transform(*args) == _lib.BH_ERR_ARG, args[:5]
    for n, p in ((4, po), (8192, po), (48, po), (64, None)):
        assert lib.bh_rf_twiddles(n, p) == _lib.BH_ERR_ARG, n
    # the LDS rule is rf_lds_bytes against 160 KiB: the twin's layout says the same for the shapes above and these
    for n, L, M, paired, fits in ((4096, 10, 3, 0, False), (4096, 10, 2, 0, True), (4096, 10, 1, 1, True), (4096, 10, 2, 1, False),
                                  (2048, 10, 8, 0, False), (1024, 10, 8, 0, True), (1024, 10, 8, 1, False), (8, 100, 2, 0, True)):
        assert (tc.lds_bytes(n, L, M, paired) <= tc.LDS_LIMIT) == fits, (n, L, M, paired)
    import bayhunter_amd as bh
    if bh.device_count() == 0:
        assert lib.bh_selftest_rf_transform(64, 10, 1, 1, 0, pa, 64, po) == _lib.BH_ERR_NO_DEVICE
        assert lib.bh_selftest_rf_transform(4096, 10, 1, 8, 1, pa, 4096, po) == _lib.BH_ERR_NO_DEVICE
