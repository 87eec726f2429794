"""Numpy restatement, written anew, of the discontinuity statistics (bayhunter_amd/interfaces.py, csrc/interfaces_core.h):
per row its own cumsum of the interface depths (what posterior.stepmodel forms, Models.py:55-70) and the float64
differences of its Vs values; the weights expanded with np.repeat; np.histogram and np.histogram2d for the counts, a
per-row np.unique of the depth bins for the `models*` fields, numpy.longdouble for the jump moments.  Nothing here is
shared with the code under test."""
import numpy as np

COUNTS = ('count', 'models', 'neg', 'pos', 'models_neg', 'models_pos')


def row_interfaces(row):
    """(depths, jumps) of one row's interfaces, float64 [n - 1] each (empty for fewer than two nuclei)."""
    model = np.asarray(row, dtype=np.float64)
    model = model[~np.isnan(model)]
    n = model.size // 2
    if n < 2:
        return np.zeros(0), np.zeros(0)
    vs, z = model[:n], model[model.size - n:]
    z_disc = (z[:n - 1] + z[1:n]) / 2.
    h = z_disc - np.concatenate(([0], z_disc[:-1]))
    return np.cumsum(h), vs[1:] - vs[:-1]


def bins_of(values, edges):
    """numpy's histogram rule: edges[i] <= v < edges[i + 1], the last bin closed, -1 outside."""
    b = np.searchsorted(edges, values, side='right') - 1
    b[values == edges[-1]] = edges.size - 2
    b[(values < edges[0]) | (values > edges[-1]) | np.isnan(values)] = -1
    return b


def summarize(models, weights, dedges, jedges):
    """-> dict(total, count, models, neg, pos, models_neg, models_pos [nbd], hist [nbd, nbj] (int64), jump_mean,
    jump_std [nbd] (longdouble, NaN where count is 0), addends [nbd] (rows' interfaces of positive weight in the bin,
    not expanded) and absum [nbd] = sum w |J| (longdouble): what the bound of the float sums is made of)."""
    dedges, jedges = np.asarray(dedges, dtype=np.float64), np.asarray(jedges, dtype=np.float64)
    nbd, nbj = dedges.size - 1, jedges.size - 1
    w = np.ones(len(models), dtype=np.int64) if weights is None else np.asarray(weights, dtype=np.int64)
    out = {k: np.zeros(nbd, dtype=np.int64) for k in COUNTS}
    out['total'] = int(w.sum())
    addends = np.zeros(nbd, dtype=np.int64)
    D, J = [], []
    for row, wr in zip(models, w):
        d, j = row_interfaces(row)
        if wr == 0 or d.size == 0:
            continue
        b = bins_of(d, dedges)
        for name, keep in (('models', b >= 0), ('models_neg', (b >= 0) & (j < 0)), ('models_pos', (b >= 0) & (j > 0))):
            out[name][np.unique(b[keep])] += wr
        np.add.at(addends, b[b >= 0], 1)
        D.append(np.repeat(d, wr))
        J.append(np.repeat(j, wr))
    D = np.concatenate(D) if D else np.zeros(0)
    J = np.concatenate(J) if J else np.zeros(0)
    out['count'] = np.histogram(D, bins=dedges)[0].astype(np.int64)
    out['neg'] = np.histogram(D[J < 0], bins=dedges)[0].astype(np.int64)
    out['pos'] = np.histogram(D[J > 0], bins=dedges)[0].astype(np.int64)
    out['hist'] = np.histogram2d(D, J, bins=(dedges, jedges))[0].astype(np.int64)
    b = bins_of(D, dedges)
    mean, std, absum = (np.full(nbd, np.nan, dtype=np.longdouble) for _ in range(3))
    for d in range(nbd):
        x = J[b == d].astype(np.longdouble)
        absum[d] = np.abs(x).sum()
        if x.size:
            mean[d] = x.sum() / x.size
            std[d] = np.sqrt(((x - mean[d]) ** 2).sum() / x.size)
    out.update(jump_mean=mean, jump_std=std, addends=addends, absum=absum)
    return out


def layered_row(vs, interfaces, width, dtype):
    """A row whose interfaces lie at the given depths: nuclei mirrored about them (the first nucleus at half the first
    interface's depth), so that the midpoints of neighbouring nuclei are the interfaces (up to rounding)."""
    n = len(vs)
    z = np.zeros(n)
    if n > 1:
        z[0] = interfaces[0] / 2.
        for k in range(1, n):
            z[k] = 2. * interfaces[k - 1] - z[k - 1]
    row = np.full(width, np.nan)
    row[:n], row[n:2 * n] = vs, z
    return row.astype(dtype)


def random_rows(rs, nrows, width, dtype, zmax=60., nmax=None):
    """Depth-sorted random models with 1 .. nmax (default width / 2) nuclei, Vs in [1, 5) with velocity inversions,
    every twentieth row all NaN."""
    nmax = width // 2 if nmax is None else nmax
    rows = np.full((nrows, width), np.nan)
    for r in range(nrows):
        if r % 20 == 19:
            continue
        n = rs.randint(1, nmax + 1)
        rows[r, :n] = rs.uniform(1., 5., n)
        rows[r, n:2 * n] = np.sort(rs.uniform(0., zmax, n))
    return rows.astype(dtype)
