"""Golden vectors of the velocity-depth posterior, produced by the REFERENCE's own src/Models.py
(ModelMatrix.get_singlemodels) and src/Plotting.py (PlotFromStorage._plot_bestmodels_hist,
PlotFromStorage.get_outliers), loaded file-wise in the development container.

    python tests/golden/make_golden_posterior.py        (needs /root/reference)

Plotting.py is loaded with a stand-in `BayHunter` package that provides the reference's own Model /
ModelMatrix (from Models.py) and empty `utils` / `Targets` modules; `PyPDF2` is stubbed.  NumPy 2 refuses
`np.array` of ragged sequences (src/Models.py:205, src/Plotting.py:485 and :530 build such arrays), so both
modules get a module-level `np` proxy whose `array` falls back to dtype=object for ragged input -- what
NumPy < 1.24 did -- and which records the results of `histogram2d`; the interface histogram is read from
the (counts, edges, patches) tuple the proxy sees at Plotting.py:530.  Rows are float32 values; weights
are realised by repeating rows (np.repeat), as get_weightedvalues does.  Nothing of the reference is stored.
Output posterior.npz: per case the rows, weights, misfits, dep_int and the reference's results.
"""
import glob
import importlib.util
import os
import sys
import tempfile
import types

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
REF = '/root/reference/src'


class NpProxy(object):
    def __init__(self):
        self.h2d, self.ragged = [], []

    def __getattr__(self, name):
        return getattr(np, name)

    def array(self, obj, *a, **k):
        try:
            return np.array(obj, *a, **k)
        except ValueError:
            self.ragged.append(obj)
            return np.array(obj, *a, dtype=object, **k)

    def histogram2d(self, *a, **k):
        r = np.histogram2d(*a, **k)
        self.h2d.append(r)
        return r


def load(name, fname, proxy):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, fname))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.np = proxy
    return mod


def rows_set(rs):
    """rows float32 [R, 2*21] in the reference layout: chain rows, random 1..20-nucleus models (one-nucleus
    ones included), models with interfaces on grid points, all-NaN rows"""
    width = 42
    out = []
    g = np.load(os.path.join(OUT, 'chains_golden.npz'))
    for k in sorted(g.keys()):
        if k.endswith('/models'):
            m = g[k][::7]
            r = np.full((m.shape[0], width), np.nan, dtype=np.float32)
            r[:, :m.shape[1]] = m
            out.append(r)
    for _ in range(400):
        n = rs.randint(1, 21) if rs.rand() > 0.1 else 1
        r = np.full(width, np.nan, dtype=np.float32)
        r[:n] = rs.uniform(1.0, 5.0, n)
        r[n:2 * n] = np.sort(rs.uniform(0, 70, n))
        out.append(r[None])
    for _ in range(60):                    # z_disc on the 0.5 / 1 / 2.5 km grids: integer nuclei of equal parity
        n = rs.randint(2, 12)
        z = np.sort(rs.choice(np.arange(0, 80, 2), n, replace=False)).astype(np.float32)
        r = np.full(width, np.nan, dtype=np.float32)
        r[:n] = np.round(rs.uniform(1.0, 5.0, n) * 40) / 40
        r[n:2 * n] = z
        out.append(r[None])
    out.append(np.full((5, width), np.nan, dtype=np.float32))
    rows = np.concatenate(out)
    return rows[rs.permutation(rows.shape[0])]


def main():
    import matplotlib
    matplotlib.use('Agg')
    sys.modules.setdefault('PyPDF2', types.ModuleType('PyPDF2'))
    if not hasattr(np, 'int'):
        np.int = int
    proxy = NpProxy()
    models = load('ref_models', 'Models.py', proxy)
    pkg = types.ModuleType('BayHunter')
    pkg.Model, pkg.ModelMatrix = models.Model, models.ModelMatrix
    pkg.utils, pkg.Targets = types.ModuleType('BayHunter.utils'), types.ModuleType('BayHunter.Targets')
    sys.modules['BayHunter'] = pkg
    sys.modules['BayHunter.utils'], sys.modules['BayHunter.Targets'] = pkg.utils, pkg.Targets
    plotting = load('ref_plotting', 'Plotting.py', proxy)
    PFS = plotting.PlotFromStorage
    import matplotlib.pyplot as plt

    rs = np.random.RandomState(2024)
    rows = rows_set(rs)
    R = rows.shape[0]
    d = dict(rows=rows)
    grids = dict(default=None, deep=np.arange(-5., 181., 2.5), models2d=np.arange(0, 60 + 1, 1))
    for case, dep_int in grids.items():
        w = rs.randint(0, 5, size=R).astype(np.int32)
        w[rs.rand(R) < 0.5] = 1
        misfits = rs.uniform(0.1, 3.0, R).round(3)
        wm = np.repeat(rows.astype(np.float64), w, axis=0)
        wmis = np.repeat(misfits, w)
        sm = models.ModelMatrix.get_singlemodels(wm, dep_int, wmis)
        proxy.h2d, proxy.ragged = [], []
        fig, axes = PFS._plot_bestmodels_hist(wm, dep_int)
        plt.close(fig)
        # histogram2d calls: get_singlemodels(models, depbins) inside, then the density (Plotting.py:501)
        h2, xe, ye = proxy.h2d[-1]
        ifc = [r for r in proxy.ragged if isinstance(r, tuple) and len(r) == 3][-1]
        keep = wm[~np.isnan(wm).all(axis=1)]
        layers = np.array([(m[~np.isnan(m)].size / 2 - 1) for m in keep])          # Plotting.py:611-614
        lbins = np.arange(np.min(layers), np.max(layers) + 2) - 0.5
        d.update({
            case + '/weights': w, case + '/misfits': misfits,
            case + '/dep_int': np.linspace(0, 100, 201) if dep_int is None else dep_int,
            case + '/mean': sm['mean'][0], case + '/median': sm['median'][0], case + '/minmax': sm['minmax'][0],
            case + '/stdminmax': sm['stdminmax'][0], case + '/mode_vs': sm['mode'][0], case + '/mode_dep': sm['mode'][1],
            case + '/minmisfit_vs': sm['minmisfit'][0], case + '/minmisfit_dep': sm['minmisfit'][1],
            case + '/hist2d': h2.astype(np.int64), case + '/hist2d_vs': xe, case + '/hist2d_dep': ye,
            case + '/interfaces': np.asarray(ifc[0]).astype(np.int64), case + '/interfaces_edges': np.asarray(ifc[1]),
            case + '/nlayers': np.histogram(layers, lbins)[0], case + '/nlayers_first': np.min(layers),
            case + '/nmodels': keep.shape[0]})
        print(case, 'expanded rows', wm.shape[0], 'hist2d', h2.shape)
    # get_outliers on a small file set
    with tempfile.TemporaryDirectory() as td:
        nch = 7
        for c in range(nch):
            n = rs.randint(20, 60)
            likes = rs.normal(-200.0 if c != 3 else -260.0, 3.0, n).astype(np.float32)
            if c == 5:
                likes = likes[:rs.randint(2, 5) * 2]
            np.save(os.path.join(td, 'c%03d_p2likes.npy' % (c + 10)), likes)
            d['outliers/likes%d' % c] = likes
        me = types.SimpleNamespace(datapath=td, likefiles=[[], sorted(glob.glob(os.path.join(td, 'c???_p2likes.npy')))])
        me._return_c_p_t = lambda f: PFS._return_c_p_t(me, f)
        d['outliers/result'] = np.asarray(PFS.get_outliers(me, 0.05))
        d['outliers/first'] = np.array(10)
        print('outliers', d['outliers/result'])
    np.savez_compressed(os.path.join(OUT, 'posterior.npz'), **d)


if __name__ == '__main__':
    main()
