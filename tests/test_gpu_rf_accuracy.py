"""rf_kernel through bh_rf_batch and bh_rf_batch_sets on the table of tests/rf_accuracy_cases.py, which
tests/test_rf_accuracy.py has shown well-posed on the CPU: the device trace G against the fp64 oracle O, and against the
host replay R, both held to a fraction of the oracle's own distance from the same algorithm in long double (the judge
is described in rf_accuracy_cases.py).  No test here compares against the fixed receiver-function tolerance.

Each test prints its family's two lines (RF-RATIO gpu G-O ..., RF-RATIO gpu G-R ...) before it asserts.

Measured on an MI355X when the constants were frozen (29 families, 371 models; the file takes 4 s, the slowest family
0.6 s), d / Y worst | family median:

    family     G against O        G against R          family     G against O        G against R
    batch      0.0120 | 0.0033    0.0074 | 0.0022      n4096      0.0023 | 0.0014    0.0036 | 0.0012
    L2         0.0149 | 0.0032    0.0115 | 0.0021      P_4to8     0.0114 | 0.0031    0.0074 | 0.0024
    L10        0.0055 | 0.0041    0.0052 | 0.0031      SV_4to8    0.0128 | 0.0031    0.0088 | 0.0027
    L31        0.0087 | 0.0052    0.0053 | 0.0044      SV_14      0.0210 | 0.0119    0.0252 | 0.0103
    L100       0.0146 | 0.0115    0.0102 | 0.0086      P_14       0.0055 | 0.0052    0.0042 | 0.0037  (2 of 7 rows finite)
    ragged     0.0176 | 0.0039    0.0083 | 0.0029      a0.8       0.0059 | 0.0040    0.0054 | 0.0025
    n8         0.0130 | 0.0043    0.0051 | 0.0013      a1         0.0049 | 0.0035    0.0048 | 0.0024
    n16        0.0097 | 0.0042    0.0041 | 0.0030      a1.21      0.0046 | 0.0032    0.0044 | 0.0022
    n32        0.0091 | 0.0034    0.0077 | 0.0029      a2.5       0.0048 | 0.0025    0.0039 | 0.0022
    n64        0.0098 | 0.0055    0.0030 | 0.0021      nsv        0.0050 | 0.0015    0.0050 | 0.0013
    n128       0.0070 | 0.0020    0.0036 | 0.0013      lvz20_sv   0.0429 | 0.0016    0.0433 | 0.0017
    n256       0.0067 | 0.0038    0.0062 | 0.0028      sets_P     0.0144 | 0.0040    0.0108 | 0.0049
    n512       0.0060 | 0.0037    0.0052 | 0.0035      sets_SV    0.0055 | 0.0033    0.0046 | 0.0023
    n1024      0.0026 | 0.0013    0.0035 | 0.0012      lowq       0.0021 | 0.0012    0.0017 | 0.0009
    n2048      0.0034 | 0.0023    0.0031 | 0.0015

(lvz20_sv's worst is row 47, the third ill-conditioned fixture.)  The host replay against O on the same table: worst
0.0474 (lvz20_sv row 46, the second fixture), largest family median 0.0136 (SV_14).
RF_TIGHT_MAX = 0.2 and RF_TIGHT_MED = 0.06 are four times the larger figure of the two tiers, rounded up to one
significant digit (tests/tolerances.py).

Seeded faults (scratch copies of rf_core.h / rf_host.h / bh_common.h, never committed; the host replay compiles the
same headers, so the CPU tier stands for both) and the families of the 29 that turned red:

  sine of the layer phase factors times 1 + 1e-12 (rf_cexp_pair)         29: every family, all on the per-model bound
      (the replay moves to 2e-13 ... 1.2e-11 of the oracle: inside the fixed tolerance of 1e-10 everywhere)
  one twiddle, the real part of exp(i pi / 4), off by 1e-13               25: all but n128, n1024, n2048, lvz20_sv -- 15
      on the per-model bound (d / Y 0.24 ... 0.66), 10 on the family median (0.063 ... 0.113); the replay stays within
      4.3e-14 of the oracle, four orders inside the fixed tolerance.  lvz20_sv (e_ref median 5.9e-13) and three
      lengths keep the 1e-14 this fault moves a trace by under 0.2 Y: a fault of that size is inside their noise
  1e-11 of the last layer's attenuation exponent dropped                  23: batch, L2, L10, ragged, n8 (median), n16,
      (e11, e22 of layer nlay - 2 times 1 - 1e-11 x, x the exponent)          n64 ... n4096, P_4to8, SV_4to8, SV_14
      (d / Y 13), a0.8 ... a2.5, lvz20_sv, sets_P, lowq (d / Y 20); not L31, L100 (the last of many layers is thin
      or deep and x small), n32, P_14, nsv, sets_SV.  The replay stays within 2.2e-14 of the oracle on the bench
      models and 2.1e-12 on resonant low-Q models; of the tests at the fixed tolerance only the ill-conditioned
      fixtures' rf_bound (half the oracle's own error) notices it
  Smith's quotient of bh_common.h contracted, which the sources forbid     0: it changes no bit -- complex quotients
      occur in the set-up only, with a real divisor or a real dividend on every model of the table, where the fused
      and the rounded product are the same number
  cmul of the layer step with the other product of each component fused    0: bits change, the ratios do not (worst
      0.0474, medians as before): a reordering of roundings is no loss of accuracy, and the bound is not meant to
      trip on one

The CPU tier's older figure-against-the-parent assertions (test_rf_floor.py: twice the parent's deviation, 2.8e-16 ...
6.4e-15) also notice the first three on the host replay; nothing on the device did before this file.
"""
import numpy as np
import pytest

import rf_accuracy_cases as ac
from tolerances import RF_TIGHT_MAX, RF_TIGHT_MED

pytestmark = pytest.mark.gpu


def _gpu(lib, launch):
    """one launch of the table through bh_rf_batch, or bh_rf_batch_sets where it has a table of slownesses; the
    output rows are pre-filled so that a sample the kernel does not write shows"""
    import torch
    from bayhunter_amd import _lib
    dev = torch.device('cuda')
    par = launch['par']
    B, L = launch['H'].shape

    def up(a, dt=np.float64):
        return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
    d = [up(launch[k]) for k in ('H', 'VP', 'VS', 'RHO', 'QP', 'QS')]
    ptr = [None if x is None else x.data_ptr() for x in d]
    dn = up(launch['nl'], np.int32)
    nout = par['nout']
    out = torch.full((B, nout), 7.0, dtype=torch.float64, device=dev)
    c = _lib.RfParams(par['p'], par['gauss'], par['fsamp'], par['tshift'], -1.0 if par['nsv'] is None else par['nsv'],
                      par['nsamp'], par['waveno'], nout, 0)
    if launch['sets'] is None:
        _lib.check(lib.bh_rf_batch(B, L, L, dn.data_ptr(), *ptr, c, out.data_ptr(), nout, None, 0, None))
    else:
        t, i = up(launch['sets'][0]), up(launch['sets'][1], np.int32)
        _lib.check(lib.bh_rf_batch_sets(B, L, L, dn.data_ptr(), *ptr, c, len(launch['sets'][0]), t.data_ptr(),
                                        i.data_ptr(), out.data_ptr(), nout, None, 0, None))
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize('name', ac.NAMES)
def test_gpu_rf_within_a_fraction_of_the_oracles_own_error(lib, name):
    """Every model of the family: |G - O| and |G - R| within RF_TIGHT_MAX of Y, the family medians within
    RF_TIGHT_MED, G finite exactly where O is (P_14: the NaN rows of the oracle are NaN rows of the device)."""
    assert ac.well_posed(name) is None, ac.well_posed(name)
    G = [row for launch in ac.FAMILIES[name] for row in _gpu(lib, launch)]
    w_o, m_o, msg_o = ac.judge(name, G, RF_TIGHT_MAX, RF_TIGHT_MED, tag='gpu G-O')
    w_r, m_r, msg_r = ac.judge(name, G, RF_TIGHT_MAX, RF_TIGHT_MED, against=ac.host_replay(name), tag='gpu G-R')
    assert msg_o is None, (name, 'G against O', msg_o)
    assert msg_r is None, (name, 'G against R', msg_r)
