"""The refusals summarize_sets and rf_summarize_sets share (bayhunter_amd/sensitivity.py): one table of bad arguments
against both, each row with the ValueError's text.  Every row is refused before a device is touched (device='cpu'), so
no GPU is needed."""
import numpy as np
import pytest

ROWS, START = np.zeros((10, 4)), [0, 4, 10]
SET_START = 'set_start: [sets + 1], ascending from 0 to the number of rows'
EDGES_COUNT, EDGES_ORDER = 'dep_edges: 2 to 1025 edges', 'dep_edges: finite and ascending'
TABLE = [
    (dict(models=np.zeros(10)), 'models: [rows, 2*maxlayers]'),
    (dict(models=np.zeros((2, 5, 4))), 'models: [rows, 2*maxlayers]'),
    (dict(set_start=[0, 6, 4, 10]), SET_START),
    (dict(set_start=[0, 4, 9]), SET_START),
    (dict(set_start=[1, 10]), SET_START),
    (dict(set_start=[0]), SET_START),
    (dict(vpvs=np.full(9, 1.73)), 'vpvs: one per row, or a scalar'),
    (dict(weights=np.ones(9, dtype=np.int32)), 'one weight per row'),
    (dict(weights=np.array([1] * 9 + [-1])), 'negative weight'),
    (dict(max_rows=0), 'max_rows >= 1'),
    (dict(dep_edges=[0., 1., 1.]), EDGES_ORDER),
    (dict(dep_edges=[2., 1.]), EDGES_ORDER),
    (dict(dep_edges=[0.]), EDGES_COUNT),
    (dict(dep_edges=[0., np.nan]), EDGES_ORDER),
    (dict(dep_edges=[0., np.inf]), EDGES_ORDER),
    (dict(dep_edges=np.arange(1026.)), EDGES_COUNT),
    (dict(kind='h'), "kind 'h': 'vp', 'vs', 'rho' or 'vs_total' (dc/dh is an interface derivative, not a depth density)"),
    (dict(models=np.zeros((0, 4)), set_start=[0, 0, 0]), 'set 0: empty selection: no models'),
]
RF_TABLE = [
    (dict(every=0), 'every >= 1'),
    (dict(t=(50., 60.)), 't, every: no sample of the trace is selected'),
    (dict(p=[6.4, 6.5, 6.6]), 'p: a number, or one per set'),
]


def _call(name, **kw):
    from bayhunter_amd import sensitivity as sens
    kw = dict(dict(models=ROWS, set_start=START, vpvs=1.73, device='cpu'), **kw)
    if name == 'rf':
        return sens.rf_summarize_sets({'obsx': np.linspace(-5, 35, 401)}, **kw)
    return sens.summarize_sets(np.array([5., 10.]), 'rayleigh', **kw)


@pytest.mark.parametrize('name', ['swd', 'rf'])
def test_summarize_sets_refuses_the_table(name):
    for kw, text in TABLE + (RF_TABLE if name == 'rf' else []):
        with pytest.raises(ValueError) as e:
            _call(name, **kw)
        assert str(e.value) == text, kw
    # without rows and not strict: every set is None, with its message
    res = _call(name, models=np.zeros((0, 4)), set_start=[0, 0, 0], strict=False)
    assert list(res) == [None, None] and res.failed == {0: 'empty selection: no models', 1: 'empty selection: no models'}
