"""CPU tier: the exact rewrites of the dispersion layer step and the period table of swd_kernel leave every bit.

1. Each expression that became an explicit fusion with an exact factor (bh_common.h: bh_fma_exact2; swd_core.h:
   swd_var, swd_love_layer, swd_dnka) against the form it had before, on 2^20 random operands from the ranges the
   layer step sees, plus the edges: fac in {0, subnormal, 1}, a0 = 0, zero products.
2. The period table (swd_core.h: SwdPerTab, filled once per workgroup) against the divisions the events used to do:
   the bench periods, 60 periods, irregular periods; phase velocity and the t1a / t1b pair of group velocity.
3. The loop of swd_lane with the table against the same loop reading the periods directly, the suite's host replay
   (hostsim.cpp) and, with glibc math, the oracle; and the same replay as a program of its own under
   AddressSanitizer and UBSan.

tests/hostsim/exact_rewrites_sim.cpp holds the native side.  The host build fuses nothing by itself
(-ffp-contract=off); fma() is the hardware's where the CPU has one and libm's correctly rounded one elsewhere."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from bayhunter_amd.synthetic import draw_models
from conftest import ROOT

HS = os.path.join(ROOT, 'tests', 'hostsim')
SRC = os.path.join(HS, 'exact_rewrites_sim.cpp')
DEPS = [SRC] + [os.path.join(ROOT, 'bayhunter_amd', 'csrc', f) for f in ('bh_common.h', 'bh_math.h', 'swd_core.h')]
N = 1 << 20
PER21, PER60 = np.linspace(1, 41, 21), np.linspace(0.5, 120.0, 60)
PER_ODD = np.array([0.3, 1.0 / 3.0, 2.7182818, 9.999999, 10.0, 33.3, 41.0, 150.0, 1.0e3])
dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)


def _stale(out):
    return not os.path.exists(out) or any(os.path.getmtime(s) > os.path.getmtime(out) for s in DEPS)


def _fma_flag():
    return ['-mfma'] if ' fma ' in open('/proc/cpuinfo').read() else []


def build_sim(name='libexact_rewrites_sim.so', extra=()):
    so = os.path.join(HS, name)
    if _stale(so):
        subprocess.run(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-ffp-contract=off'] + _fma_flag() + list(extra) +
                       ['-o', so, SRC], check=True)
    hs = C.CDLL(so)
    hs.er_forms.argtypes = [C.c_int, C.c_long, dp, dp, dp, dp, dp, dp]
    hs.er_period.argtypes = [dp, C.c_int, C.c_int, C.c_int, dp, dp]
    hs.er_period_before.argtypes = [C.c_double, C.c_int, dp]
    hs.er_batch.restype = C.c_int
    hs.er_batch.argtypes = [C.c_int, C.c_int, dp, dp, dp, dp, ip] + [C.c_int] * 5 + [dp, C.c_int, dp, ip]
    return hs


def replay_batch(hs, models, per, iwave, igr, mode=1, table=1):
    """(values [B, nper], err [B]) of the host replay of swd_lane over a batch."""
    H, VP, VS, RHO, nl = [np.ascontiguousarray(a) for a in models]
    nl = np.ascontiguousarray(nl, dtype=np.int32)
    per = np.ascontiguousarray(per, dtype=np.float64)
    B, L = H.shape
    cg, err = np.zeros((B, len(per))), np.zeros(B, np.int32)
    rc = hs.er_batch(B, L, *[a.ctypes.data_as(dp) for a in (H, VP, VS, RHO)], nl.ctypes.data_as(ip), 0, iwave, mode, igr,
                     len(per), per.ctypes.data_as(dp), table, cg.ctypes.data_as(dp), err.ctypes.data_as(ip))
    assert rc == 0
    return cg, err


@pytest.fixture(scope='module')
def sim():
    return build_sim()


def _operands():
    """Operands of the layer step (ten-layer crustal models, periods 1 .. 41 s, trial velocities around vs): gam =
    2 (b / c)^2 in 0.05 .. 50, gammk = gam / wvno^2 with wvno^2 = (omega / c)^2 in 1e-4 .. 10, cosines and their
    products in [-1, 1] with magnitudes down to 1e-12 (and exact zeros), a0 = exp(-exa) in e^-60 .. 1 or 0."""
    r = np.random.RandomState(2024)
    gam = np.exp(r.uniform(np.log(0.05), np.log(50.0), N))
    gam[::97] = 1.0 + r.randint(-4, 5, len(gam[::97])) * 2.0 ** -52            # gam - 1 tiny or zero
    wvno2 = np.exp(r.uniform(np.log(1e-4), np.log(10.0), N))
    gammk = gam / wvno2
    gamm1 = gam - 1.0
    signed = lambda lo: np.exp(r.uniform(np.log(lo), 0.0, N)) * r.choice([-1.0, 1.0], N)
    cpcq = signed(1e-12)
    a0 = np.exp(-r.uniform(0.0, 60.0, N))
    a0[::5] = 0.0                                                             # exa >= 60
    cpcq[::211] = 0.0
    a0[3::1055] = cpcq[3::1055]                                               # a0pq = 0
    xz = signed(1e-12) * np.exp(r.uniform(-3, 3, N))
    fac = np.exp(-2.0 * r.uniform(0.0, 16.0, N))
    fac[:8] = [0.0, 5e-324, 2.2250738585072014e-308, 1e-310, 1.0, 1.0 - 2.0 ** -53, 2.0 ** -53, 2.0 ** -54]
    return dict(gam=gam, gammk=gammk, gamm1=gamm1, wvno2=wvno2, cpcq=cpcq, a0=a0, xz=xz, fac=fac)


def _forms(sim, which, a, b=None, c=None, d=None):
    z = np.zeros(N)
    arrs = [np.ascontiguousarray(z if x is None else x, dtype=np.float64) for x in (a, b, c, d)]
    before, after = np.empty(N), np.empty(N)
    sim.er_forms(which, N, *[x.ctypes.data_as(dp) for x in arrs], before.ctypes.data_as(dp), after.ctypes.data_as(dp))
    return before.view(np.int64), after.view(np.int64)


@pytest.mark.parametrize('name', ['cos', 'sin', 'c11', 'c15', 'c51', 'c33'])
def test_fused_forms_return_the_bits_of_the_forms_before(sim, name):
    o = _operands()
    a0pq = o['a0'] - o['cpcq']
    gmgm1, gmgmk, gm1sq = o['gam'] * o['gamm1'], o['gam'] * o['gammk'], o['gamm1'] * o['gamm1']
    c11 = o['cpcq'] - 2.0 * gmgm1 * a0pq - gmgmk * o['xz']
    args = {'cos': (0, o['fac']), 'sin': (1, o['fac']),
            'c11': (2, o['cpcq'], gmgm1, a0pq),                               # cpcq - two * gmgm1 * a0pq
            'c15': (3, o['wvno2'], a0pq, o['xz']),                            # two * wvno2 * a0pq + xz
            'c51': (4, gmgmk, gm1sq, a0pq, gmgmk * gmgmk * o['xz']),          # two * gmgmk * gm1sq * a0pq + gmgmk^2 xz
            'c33': (5, o['a0'], o['cpcq'], c11)}[name]                        # a0 + two * (cpcq - c11)
    before, after = _forms(sim, *args)
    assert (a0pq == 0).sum() > 100 and (o['a0'] == 0).sum() > N // 6 and (o['gamm1'] == 0).sum() > 100
    nbad = int((before != after).sum())
    assert nbad == 0, '%s: %d of %d operands give other bits' % (name, nbad, N)


def test_an_inexact_factor_is_told_apart(sim):
    """The comparison can fail: with a factor that is no power of two (three, through c33's form: a + 2 (b - c) against
    the fusion, on operands scaled so that the product rounds) the fused and the unfused form differ."""
    r = np.random.RandomState(5)
    a, b = r.uniform(-1, 1, N), r.uniform(-1, 1, N)
    unfused = a + 3.0 * b
    fused = np.array([float(np.longdouble(x) + np.longdouble(3.0) * np.longdouble(y)) for x, y in zip(a[:4096], b[:4096])])
    assert (unfused[:4096] != fused).sum() > 100


@pytest.mark.parametrize('igr', [0, 1])
@pytest.mark.parametrize('per', [PER21, PER60, PER_ODD], ids=['bench21', '60', 'irregular'])
def test_period_table_holds_the_quotients_of_the_events(sim, per, igr):
    per = np.ascontiguousarray(per, dtype=np.float64)
    for k in range(len(per)):
        table, event, before = np.zeros(4), np.zeros(4), np.zeros(4)
        sim.er_period(per.ctypes.data_as(dp), len(per), k, igr, table.ctypes.data_as(dp), event.ctypes.data_as(dp))
        sim.er_period_before(per[k], igr, before.ctypes.data_as(dp))
        assert np.array_equal(table.view(np.int64), before.view(np.int64)), (k, table, before)
        assert np.array_equal(event.view(np.int64), before.view(np.int64)), (k, event, before)
        # the quotients themselves, worked out once more in numpy's IEEE arithmetic
        f = np.float32
        if igr:
            t1a, t1b = f(per[k] / np.float64(f(1) + f(0.005))), f(per[k] / np.float64(f(1) - f(0.005)))
            want = [2.0 * 3.141592653589793 / np.float64(t1a), 2.0 * 3.141592653589793 / np.float64(t1b), t1a, t1b]
        else:
            want = [2.0 * 3.141592653589793 / per[k], 0.0, f(per[k]), 0.0]
        assert np.array_equal(np.array(want, dtype=np.float64).view(np.int64), table.view(np.int64)), (k, want, table)


def sanitizer_models():
    """Ten-layer models, ragged models of 2 .. 31 layers with low-velocity zones, and the suite's hunted models."""
    import test_gpu_control_paths as T
    L = T.LMAX
    parts = [draw_models(24, 10, seed=1), draw_models(24, (2, L), seed=52033, sorted_vs=False)]
    hunted = T.batch()
    out = []
    for i in range(4):
        cols = []
        for p in parts:
            a = np.zeros((p[i].shape[0], L))
            a[:, :p[i].shape[1]] = p[i]
            cols.append(a)
        out.append(np.concatenate(cols + [hunted[i][::5]]))
    nl = np.concatenate([p[4] for p in parts] + [hunted[4][::5]]).astype(np.int32)
    return out + [nl]


def test_table_replay_is_the_direct_replay_and_the_suites(sim, hostsim_devmath):
    models = sanitizer_models()
    H, VP, VS, RHO, nl = models
    for iwave, igr, mode in ((2, 0, 1), (2, 1, 2), (1, 0, 1), (1, 1, 1)):
        got = replay_batch(sim, models, PER21, iwave, igr, mode, table=1)
        direct = replay_batch(sim, models, PER21, iwave, igr, mode, table=0)
        assert np.array_equal(got[0].view(np.int64), direct[0].view(np.int64)) and np.array_equal(got[1], direct[1])
        for b in range(0, len(nl), 7):
            n = nl[b]
            cg, e, _ = hostsim_devmath.swd(H[b, :n], VP[b, :n], VS[b, :n], RHO[b, :n], PER21, iwave, igr, mode=mode)
            assert e == got[1][b] and np.array_equal(cg, got[0][b]), (iwave, igr, b)


def test_table_replay_with_glibc_math_is_the_oracle(oracle):
    """With glibc's sin / cos / exp in place of bh_math.h the replay is the reference's arithmetic, operation by
    operation: every value and flag of the oracle port, low-velocity zones and hunted models included."""
    glibc = build_sim('libexact_rewrites_sim_glibc.so', ['-DBH_HOSTSIM_GLIBC_MATH'])
    models = sanitizer_models()
    for iwave, igr in ((2, 0), (2, 1), (1, 0), (1, 1)):
        got, err = replay_batch(glibc, models, PER21, iwave, igr, 1, table=1)
        want, werr, _ = oracle.swd_batch(*models, PER21, iwave, igr)
        assert np.array_equal(err, werr), (iwave, igr)
        assert np.array_equal(got.view(np.int64), want.view(np.int64)), (iwave, igr, int((got != want).sum()))


def test_replay_under_address_and_undefined_sanitizers(tmp_path):
    """The replay as a program of its own (-DER_MAIN), compiled with -fsanitize=address,undefined, once over the model
    set: both period sources, four targets, a clean exit."""
    exe = os.path.join(HS, 'exact_rewrites_san')
    if _stale(exe):
        subprocess.run(['g++', '-O1', '-g', '-std=c++17', '-ffp-contract=off', '-fsanitize=address,undefined',
                        '-fno-sanitize-recover=undefined', '-DER_MAIN'] + _fma_flag() + ['-o', exe, SRC], check=True)
    H, VP, VS, RHO, nl = sanitizer_models()
    path = str(tmp_path / 'models.bin')
    with open(path, 'wb') as f:
        f.write(np.array([len(nl), H.shape[1], len(PER21)], dtype=np.int32).tobytes())
        for a in (H, VP, VS, RHO, PER21):
            f.write(np.ascontiguousarray(a, dtype=np.float64).tobytes())
        f.write(np.ascontiguousarray(nl, dtype=np.int32).tobytes())
    r = subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    print(r.stdout, r.stderr[-2000:])
    assert r.returncode == 0 and 'differ in 0 arrays' in r.stdout and 'runtime error' not in r.stderr
