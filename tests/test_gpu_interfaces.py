"""GPU tier of the discontinuity statistics (bh_interfaces_sets, bayhunter_amd/interfaces.py, ChainPool.interfaces,
StationPool.interfaces) against the host twin (tests/hostsim/interfaces_sim.cpp) and the numpy restatement
(tests/interfaces_ref.py).

Sets of 0, 1, 255, 257 and 3 000 rows of width 42 in one call (the last one takes two blocks), float32 and float64,
over a table that fits a block's LDS (20 x 8 bins) and one that does not (400 x 64: four groups of depth bins).  Every
integer field equals the twin; the two float sums are bit-identical between two runs, between a set in the call and the
set's rows alone, and to the twin, which adds in the kernels' order; the jump mean and standard deviation lie within
the derived bound (tests/interfaces_tolerances.py) of the longdouble restatement.

Worst error over bound as measured on one MI355X: 20 x 8 bins jump_mean 0.0061 (float32 rows) / 0.0098 (float64),
jump_std 0.016 / 0.096; 400 x 64 bins jump_mean 0.26 / 0.63, jump_std 0.18 / 0.62 (bins of one or two addends, where
the bound is about one rounding).
"""
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'scenarios'))
import interfaces_ref as ref  # noqa: E402
from test_interfaces import assert_counts, assert_same_bits, built_cases, load_sim, moment_errors, twin  # noqa: E402

pytestmark = pytest.mark.gpu
WIDTH = 42
SIZES = [0, 1, 255, 257, 3000]
START = np.concatenate(([0], np.cumsum(SIZES))).astype(np.int64)
# (0 .. 50 km over models that reach 60 km: interfaces lie outside too; every edge is an exact multiple of its step,
# so that each coarse edge is a fine edge bit for bit)
TABLES = {'small': (np.arange(21) * 2.5, -2. + np.arange(9) * 0.5),              # 20 x 8: one group
          'large': (np.arange(401) * 0.125, -2. + np.arange(65) * 0.0625)}       # 400 x 64: four groups
FIELDS = ref.COUNTS + ('hist',)
FP = ('jsum', 'jsq')

_cases, _twins = {}, {}


@pytest.fixture(scope='module')
def isim():
    return load_sim()


def case(dtype):
    """(rows, weights): random depth-sorted models, the CPU tier's built cases inside the last set."""
    key = np.dtype(dtype).name
    if key not in _cases:
        rs = np.random.RandomState(31 if key == 'float32' else 32)
        rows = ref.random_rows(rs, START[-1], WIDTH, dtype)
        w = rs.randint(0, 6, START[-1]).astype(np.int32)
        brows, bw, _ = built_cases(dtype)
        rows[START[4] + 100:START[4] + 100 + len(brows)] = brows
        w[START[4] + 100:START[4] + 100 + len(brows)] = bw
        w[0] = 3                                          # the one-row set has weight
        _cases[key] = (rows, w)
    return _cases[key]


def twin_of(isim, dtype, table):
    key = (np.dtype(dtype).name, table)
    if key not in _twins:
        rows, w = case(dtype)
        _twins[key] = twin(isim, rows, w, START, *TABLES[table])
    return _twins[key]


def device(rows, w, start, dedges, jedges):
    """interfaces._reduce on the device: the dict of arrays with one row per set."""
    import torch
    from bayhunter_amd import _device, interfaces
    dev, t, tw, _ = _device.device_rows(rows, w, per_row="one weight per row")
    assert t.dtype == (torch.float32 if rows.dtype == np.float32 else torch.float64)
    return interfaces._reduce(dev, t, tw, np.ascontiguousarray(start, dtype=np.int64), dedges, jedges)


@pytest.mark.parametrize('table', ['small', 'large'])
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_sets_equal_the_twin_and_their_rows_alone(lib, isim, dtype, table):
    from bayhunter_amd import interfaces
    dedges, jedges = TABLES[table]
    assert (isim.ifs_group(dedges.size - 1, jedges.size - 1) < dedges.size - 1) == (table == 'large')
    rows, w = case(dtype)
    want = twin_of(isim, dtype, table)
    got = device(rows, w, START, dedges, jedges)
    again = device(rows, w, START, dedges, jedges)
    assert np.array_equal(got['total'], want['total'])
    for k in FIELDS:
        assert got[k].dtype == np.int64 and np.array_equal(got[k], want[k]), k
        assert np.array_equal(got[k], again[k]), k
    for k in FP:
        assert_same_bits(got[k], again[k])                 # two runs
        assert_same_bits(got[k], want[k])                  # the twin adds in the kernels' order
    assert got['total'][0] == 0 and np.isnan(got['jsum'][0]).all() and np.isnan(got['jsq'][0]).all()
    worst = [0., 0.]
    for z, n in enumerate(SIZES):
        if not n:
            continue
        a, b = START[z], START[z + 1]
        alone = device(rows[a:b], w[a:b], [0, n], dedges, jedges)
        assert alone['total'][0] == got['total'][z]
        for k in FIELDS:
            assert np.array_equal(alone[k][0], got[k][z]), (z, k)
        for k in FP:
            assert_same_bits(alone[k][0], got[k][z])       # float fields included
        r = ref.summarize(rows[a:b], w[a:b], dedges, jedges)
        assert_counts(got, z, r, 'set %d' % z)
        e = moment_errors(interfaces._result(got, z, dedges, jedges), r)
        worst = [max(worst[0], e[0]), max(worst[1], e[1])]
    print('%s %s: worst error / bound: jump_mean %.3g, jump_std %.3g' % (np.dtype(dtype).name, table, worst[0], worst[1]))
    assert worst[0] <= 1. and worst[1] <= 1., worst


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_the_two_tables_count_the_same(lib, dtype):
    """The large table is the small one refined 20 x 8: summed back over the refinement its counts are the small
    table's (the `models*` fields count runs per bin and do not add up)."""
    rows, w = case(dtype)
    small = device(rows, w, START, *TABLES['small'])
    large = device(rows, w, START, *TABLES['large'])
    S = len(SIZES)
    assert np.array_equal(small['total'], large['total'])
    for k in ('count', 'neg', 'pos'):
        assert np.array_equal(large[k].reshape(S, 20, 20).sum(axis=2), small[k]), k
    # (the last edges are closed in both, and every coarse edge is a fine edge)
    assert np.array_equal(large['hist'].reshape(S, 20, 20, 8, 8).sum(axis=(2, 4)), small['hist'])


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_summarize_and_the_posteriors_interface_histogram(lib, dtype):
    from bayhunter_amd import interfaces, posterior
    rows, w = case(dtype)
    a, b = START[4], START[5]
    got = interfaces.summarize(rows[a:b], w[a:b])
    post = posterior.summarize(rows[a:b], w[a:b])
    assert np.array_equal(got['dep_edges'], post['interfaces'][1]) and np.array_equal(got['jump_edges'], np.linspace(-2, 2, 41))
    assert got['count'].dtype == np.int64 and np.array_equal(got['count'], post['interfaces'][0])
    assert got['count'].sum() > 0 and got['total'] == w[a:b].sum()
    r = ref.summarize(rows[a:b], w[a:b], got['dep_edges'], got['jump_edges'])
    for k in FIELDS:
        assert np.array_equal(got[k], r[k]), k
    assert np.array_equal(got['p_interface'], r['models'] / float(r['total']))
    assert np.array_equal(got['p_neg'], r['models_neg'] / float(r['total']))
    assert np.array_equal(got['p_pos'], r['models_pos'] / float(r['total']))
    e = moment_errors(got, r)
    assert e[0] <= 1. and e[1] <= 1., e
    # the sets form: the same dicts, a set without weight left out
    sets = interfaces.summarize_sets(rows, START, w, strict=False)
    assert sorted(sets.failed) == [0] and sets[0] is None
    for k in got:
        assert np.array_equal(sets[4][k], got[k], equal_nan=True), k
    with pytest.raises(ValueError, match='set 0'):
        interfaces.summarize_sets(rows, START, w)
    sec = sets.section()
    assert sec['p_interface'].shape == (5, 100) and np.isnan(sec['count'][0]).all()
    assert np.array_equal(sec['p_neg'][4], got['p_neg']) and np.array_equal(sec['count'][4], got['count'])


def test_a_negative_weight_on_the_device_fails_the_call(lib):
    import torch
    from bayhunter_amd import _lib, interfaces
    rows, w = case(np.float32)
    w = w.copy()
    w[START[3] + 17] = -1
    with pytest.raises(_lib.BayHunterAmdError, match='negative weight'):
        interfaces.summarize_sets(rows, START, torch.from_numpy(w).cuda(), strict=False)


@pytest.fixture(scope='module')
def station_pool(lib):
    from bayhunter_amd.stations import StationPool
    from chain_scenario import CASES
    from station_scenario import make_stations
    case_ = CASES['tutorial']
    ip = dict(case_['initparams'], iter_burnin=150, iter_main=100)
    stations = make_stations(os.path.join(GOLDEN, 'tutorial_observed'), 3, refs=case_.get('refs', ('rdispph', 'prf')), yerr=True)
    with StationPool(dict(zip(['AAA', 'BBB', 'CCC'], stations)), ip, case_['priors'], chains_per_station=4,
                     random_seeds=[21, 22, 23], nmodels=251) as pool:
        pool.run()
    return pool


def assert_same_result(one, other):
    assert sorted(one) == sorted(other)
    for k in one:
        assert np.array_equal(one[k], other[k], equal_nan=True), k


def test_station_pool_interfaces_equal_every_station_views(station_pool):
    from bayhunter_amd import interfaces
    pool = station_pool
    dedges = np.linspace(0., 60., 25)
    for kw in (dict(), dict(dep_edges=dedges, jump_edges=np.linspace(-1., 1., 5), selection='saved'),
               dict(dep_edges=dedges, exclude_outliers=False)):
        res = pool.interfaces(dev=0.5, **kw)
        nbd = res.dep_edges.size - 1
        assert res.names == ['AAA', 'BBB', 'CCC'] and not res.failed and sorted(res.stations) == res.names
        for k in interfaces.SECTION:
            assert getattr(res, k).shape == (3, nbd) and getattr(res, k).dtype == np.float64
        assert res.count.sum() > 0
        for s, name in enumerate(res.names):
            one = pool.station(name).interfaces(dev=0.5, **kw)        # ChainPool.interfaces on the station's view
            assert_same_result(one, res.stations[name])
            assert one['count'].sum() > 0 and one['total'] > 0 and (one['p_interface'] <= 1.).all()
            for k in interfaces.SECTION:
                assert np.array_equal(getattr(res, k)[s], one[k], equal_nan=True), (name, k)


def test_a_station_without_rows_is_a_row_of_nan(station_pool):
    pool = station_pool
    inner = pool.pool
    keep = inner.iter[8:12].copy()
    inner.iter[8:12] = -1                                   # station CCC: no main-phase row
    try:
        res = pool.interfaces(dev=0.5)
        assert list(res.failed) == ['CCC'] and sorted(res.stations) == ['AAA', 'BBB']
        assert res.p_interface.shape == (3, 100)
        for k in ('p_interface', 'p_neg', 'p_pos', 'jump_mean', 'count'):
            assert np.isnan(getattr(res, k)[2]).all() and not np.isnan(getattr(res, k)[:2]).all(), k
        with pytest.raises(ValueError, match='empty selection'):
            pool.station('CCC').interfaces(dev=0.5)
        assert_same_result(pool.station('AAA').interfaces(dev=0.5), res.stations['AAA'])
    finally:
        inner.iter[8:12] = keep
