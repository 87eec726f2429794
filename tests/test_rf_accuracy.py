"""The host replay of rf_kernel (rf_host.h: rf_host_replay, the phase functions of rf_core.h with the device math of
bh_math.h) against the fp64 oracle, held to a fraction of the oracle's own distance from the same algorithm in long
double -- the judge, the families and the three traces are described in tests/rf_accuracy_cases.py; the two constants
and the measurements behind them in tests/tolerances.py (RF_TIGHT_MAX, RF_TIGHT_MED).  This tier shows that the table
is well-posed before a GPU sees it: every family has an oracle error that can be measured, finite rows where it needs
them, and the replay inside the bounds.  tests/test_gpu_rf_accuracy.py judges the device on the same table and lists
the seeded faults that this tier catches (the replay compiles the headers the kernel compiles).

Each test prints its family's line (RF-RATIO cpu ...) before it asserts."""
import numpy as np
import pytest

import rf_accuracy_cases as ac
from tolerances import RF_TIGHT_MAX, RF_TIGHT_MED


def test_constants_stay_orders_below_the_fixed_tolerance():
    """rf_bound() asserts half the oracle's own error on an ill-conditioned model; the tight bound may not ask less
    than that, and the family median must be the stricter of the two."""
    assert 0 < RF_TIGHT_MED < RF_TIGHT_MAX <= 0.5


def test_table_covers_what_it_claims():
    F = ac.FAMILIES
    assert [len(l['nl']) for l in F['batch']] == [1, 2, 3, 4, 7]
    assert sorted(l['par']['nsamp'] for n in ac.LENGTHS for l in F['n%d' % n]) == ac.LENGTHS
    assert [l['par']['p'] for l in F['P_4to8']] == ac.SLOWNESSES == [l['par']['p'] for l in F['SV_4to8']]
    assert {l['par']['waveno'] for l in F['SV_4to8'] + F['SV_14'] + F['lvz20_sv'] + F['sets_SV']} == {1}
    assert set(F['ragged'][0]['nl']) >= {2, 15} and F['L100'][0]['H'].shape[1] == 100
    for name in ('sets_P', 'sets_SV'):
        ids = np.asarray(F[name][0]['sets'][1])
        assert all(len(set(ids[k:k + 3])) == 2 for k in (0, 3))          # both slownesses in each full workgroup
    assert all(l['par']['nout'] == l['par']['nsamp'] for launches in F.values() for l in launches)
    assert [len(l['nl']) for l in F['lvz20_sv']] == [ac.N_LVZ, 1, 1, 1] and F['lvz20_sv'][0]['H'].shape[1] == 20
    assert F['lowq'][0]['QS'].min() == 5.0 and F['nsv'][0]['par']['nsv'] > 0


@pytest.mark.parametrize('name', ac.NAMES)
def test_host_replay_within_a_fraction_of_the_oracles_own_error(name):
    assert ac.well_posed(name) is None, ac.well_posed(name)
    worst, med, msg = ac.judge(name, ac.host_replay(name), RF_TIGHT_MAX, RF_TIGHT_MED, tag='cpu')
    assert msg is None, (name, msg)
