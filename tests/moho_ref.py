"""Numpy restatement, written anew, of what PlotFromStorage.plot_moho_crustvel_tradeoff (src/Plotting.py:761-804,
813-865) computes with Model.get_vp_vs_h (src/Models.py:16-24, 40-52): a loop over the models in which numpy
evaluates every expression on the row in its own dtype, then np.repeat by the weights, np.median, np.std,
np.histogram and np.histogram2d.  The oracle of bayhunter_amd/moho.py and csrc/moho_core.h; nothing here is shared
with them.  tests/test_moho.py ties vs_h to the reference's own function where the reference tree exists."""
import numpy as np

NAMES = ('moho', 'vs_crust', 'vs_last', 'vs_jump')
TRADEOFF = ('vs_last', 'vs_crust', 'vs_jump')          # the x axes of Plotting.py:830, in its order


def vs_h(model):
    """(vs, h) of one row as Model.get_vp_vs_h gives them (src/Models.py:16-24, 40-52), in the row's dtype where the
    reference stays in it: the nuclei are the non-NaN entries, the first half Vs and the second half depths; an
    interface lies halfway between two neighbouring nuclei (a sum and a half in the row's dtype); the thicknesses
    are the differences of the interface depths from 0 on, in float64 because the reference prepends a Python-list
    zero (an int64 array) before it subtracts; the half-space gets thickness 0."""
    nuclei = model[~np.isnan(model)]
    n = nuclei.size // 2
    vs, z = nuclei[:n], nuclei[nuclei.size - n:]
    halfway = (z[:-1] + z[1:]) / 2. if n > 1 else z[:0]
    above = np.concatenate((np.zeros(1, dtype=np.int64), halfway[:-1]))
    h = np.append(halfway - above, 0.) if n > 1 else np.zeros(1)
    return vs, h


def derive(models, moho, mohovs):
    """What Plotting.py:766-798 stores per model, then its filter (:800-804: a model whose vs_jump is NaN leaves all
    four lists) -> D [rows, 4] float64 = (moho, vs_crust, vs_last, vs_jump), a row of NaN without a Moho.

    The Moho is the first interface inside the open depth window whose lower layer is faster than `mohovs` (numpy
    compares a float32 array with a Python float in float32).  The last cumsum entry repeats the deepest interface
    (the half-space's thickness 0) and has no layer below it, so the candidates are ifaces[:-1] against vs[1:]."""
    zlo, zhi = moho
    D = np.full((len(models), 4), np.nan)
    for r, model in enumerate(models):
        vs, h = vs_h(model)
        ifaces = np.cumsum(h)
        hit = np.flatnonzero((ifaces[:-1] > zlo) & (ifaces[:-1] < zhi) & (vs[1:] > mohovs))
        if hit.size == 0:
            continue
        i = hit[0]
        jump = np.diff(vs)[i]
        if np.isnan(jump):
            continue
        m = i + 1                                         # crustal layers
        D[r] = (ifaces[i], np.sum(vs[:m] * h[:m]) / ifaces[i], vs[i], jump)
    return D


def statistics(D, weights=None, nbins=50):
    """Plotting.py:813-865 on D with every row repeated `weight` times -> the dict moho.summarize returns: per
    quantity np.median, np.mean, np.std, min, max and np.histogram(bins=nbins); per x quantity np.histogram2d
    against the Moho depth and the centres of its first fullest cell (argmax over the flattened counts, x index
    first).  ValueError when no row has a Moho."""
    D = np.asarray(D, dtype=np.float64)
    w = np.ones(len(D), dtype=np.int64) if weights is None else np.asarray(weights, dtype=np.int64)
    E = np.repeat(D, w, axis=0)
    keep = ~np.isnan(E[:, 3])
    nex = int((~keep).sum())
    E = E[keep]
    if E.shape[0] == 0:
        raise ValueError("no model with a Moho")
    res = dict(nmodels=int(E.shape[0]), nexcluded=nex, tradeoff={})
    col = {name: E[:, c] for c, name in enumerate(NAMES)}
    for name in NAMES:
        x = col[name]
        res[name] = dict(median=np.median(x), mean=np.mean(x), std=np.std(x), min=np.min(x), max=np.max(x),
                         hist=np.histogram(x, bins=nbins))
    for name in TRADEOFF:
        counts, xedges, yedges = np.histogram2d(col[name], col['moho'], bins=nbins)
        ix, iy = divmod(int(np.argmax(counts)), counts.shape[1])
        centre = lambda e, k: (e[k] + e[k + 1]) / 2.
        res['tradeoff'][name] = dict(counts=counts.astype(np.int64), xedges=xedges, yedges=yedges,
                                     mode=(centre(xedges, ix), centre(yedges, iy)))
    return res


def summarize(models, weights=None, moho=(0., 60.), mohovs=4.2, nbins=50):
    return statistics(derive(models, moho, mohovs), weights, nbins)


# ---- rows for the tests ---------------------------------------------------------------------------------------

def layered_row(vs, ifaces, width, dtype):
    """A row whose interfaces are (up to rounding) `ifaces`: nuclei mirrored about them, the first at ifaces[0] / 2."""
    vs, ifaces = np.asarray(vs, dtype=np.float64), np.asarray(ifaces, dtype=np.float64)
    n = vs.size
    z = np.zeros(n)
    z[0] = ifaces[0] / 2. if n > 1 else 1.0
    for k in range(1, n):
        z[k] = 2 * ifaces[k - 1] - z[k - 1]
    row = np.full(width, np.nan)
    row[:n], row[n:2 * n] = vs, z
    return row.astype(dtype)


def random_rows(rs, R, width, dtype, nmax=None):
    """R rows of 1 .. nmax nuclei: depths ascending in 0 .. 80 km, Vs rising with depth from about 2 to 5 km/s
    with scatter, so that a window of (20, 50) km and mohovs = 4.1 find a Moho in a good part of them."""
    nmax = width // 2 if nmax is None else nmax
    rows = np.full((R, width), np.nan)
    ns = rs.randint(1, nmax + 1, R)
    for r in range(R):
        n = ns[r]
        z = np.sort(rs.uniform(0, 80, n))
        vs = 2.0 + 3.0 * z / 80. + rs.normal(0, 0.35, n)
        rows[r, :n], rows[r, n:2 * n] = vs, z
    return rows.astype(dtype)


def built_cases(dtype, width=40, moho=(20., 50.), mohovs=4.1):
    """The edge cases of the per-row derivation -> (rows [cases, width], names).  `mohovs` is rounded to `dtype` as
    numpy does when it compares."""
    dt = np.dtype(dtype)
    zlo, zhi = moho
    lim = dt.type(mohovs)
    above = np.nextafter(lim, dt.type(np.inf), dtype=dt.type)
    rows, names = [], []

    def add(name, vs, ifaces):
        rows.append(layered_row(vs, ifaces, width, np.float64).astype(dt))
        names.append(name)

    add('n1', [4.5], [])
    add('n2', [3.0, 4.5], [30.])
    add('n2 no jump', [3.0, 3.5], [30.])
    for m in (7, 8, 9, 19):                               # a crust of exactly m layers: the Moho is interface m - 1
        vs = list(np.linspace(2.0, 3.6, m) + 0.0123 * np.arange(m)) + [4.6]
        add('crust of %d' % m, vs, list(np.linspace(2.1, 35.3, m)))
    for m in (3, 9):                                      # products that are all -0: np.sum gives +0 from its identity
        add('minus zero crust of %d' % m, [-0.0] * m + [4.6], list(np.linspace(2.1, 35.3, m)))
    add('two qualify', [3.0, 4.3, 3.9, 4.4], [25., 30., 35.])
    add('velocity below an interface outside', [3.0, 4.5, 4.0, 4.6], [10., 30., 40.])
    add('window empty', [3.0, 4.5, 4.6], [10., 60.])
    rows.append(np.full(width, np.nan, dtype=dt))
    names.append('all NaN')
    # an interface exactly on zlo / zhi: nuclei whose mean is the bound exactly in either dtype
    for bound, nm in ((zlo, 'on zlo'), (zhi, 'on zhi')):
        row = np.full(width, np.nan)
        row[:2], row[2:4] = (3.0, 4.5), (bound - 8., bound + 8.)
        rows.append(row.astype(dt))
        names.append('interface ' + nm)
    # vs[i+1] == mohovs as rounded (no Moho), one ulp above (a Moho)
    for v, nm in ((lim, 'equal'), (above, 'one ulp above')):
        row = layered_row([3.0, 4.0], [30.], width, np.float64).astype(dt)
        row[1] = v
        rows.append(row)
        names.append('vs %s mohovs' % nm)
    # z pairs whose mean in the row's dtype is not the double mean (float32: the sum rounds)
    # 20 + k 2^-19 with k odd is a float32; its sum with a value in 32 .. 64 is not (the sum's ulp is 2^-18)
    for a, b in ((20. + 2. ** -19, 40.), (20. + 3 * 2. ** -19, 40. + 2. ** -18), (24. + 5 * 2. ** -19, 37.5)):
        row = np.full(width, np.nan)
        row[:3], row[3:6] = (3.0, 4.5, 4.7), (a, b, 70.)
        rows.append(row.astype(dt))
        names.append('z pair %r' % ((a, b),))
    return np.stack(rows), names
