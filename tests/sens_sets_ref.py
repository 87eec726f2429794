"""The depth-binned sensitivity statistics restated in numpy.longdouble on the expanded matrix (every row repeated
`weight` times), from the definitions in include/bayhunter_amd.h (bh_sens_sets_*) and not from csrc/sens_sets_core.h.

Only the layer tops are float64 (the definition says so: the sequential fp64 cumsum of h); the layer values, the overlap
fractions, the cells and every sum are longdouble.
"""
import numpy as np

LD = np.longdouble
KINDS = {'vp': 1, 'vs': 2, 'rho': 3, 'vs_total': 4}


def layer_values(K, q, kind, drho_dvp=0.32):
    """G [nper, L] of one row: K [nper, 4, L], q [L] or None."""
    K = np.asarray(K, dtype=LD)
    if kind == 'vs_total':
        return K[:, 2, :] + np.asarray(q, dtype=LD)[None, :] * (K[:, 1, :] + LD(drho_dvp) * K[:, 3, :])
    return K[:, KINDS[kind], :]


def cells(h, nlay, G, edges):
    """x [nper, nb + 1] of one row with nlay layers: the bins, then the half-space."""
    h = np.asarray(h, dtype=np.float64)[:nlay]
    edges = np.asarray(edges, dtype=np.float64)
    top = np.zeros(nlay)
    for l in range(1, nlay):
        top[l] = top[l - 1] + h[l - 1]                      # fp64, sequential
    x = np.zeros((G.shape[0], edges.size), dtype=LD)
    for j in range(edges.size - 1):
        for l in range(nlay - 1):
            if not h[l] > 0:
                continue
            d = min(LD(top[l + 1]), LD(edges[j + 1])) - max(LD(top[l]), LD(edges[j]))
            if d > 0:
                x[:, j] += d / LD(h[l]) * G[:, l]
    x[:, -1] = G[:, nlay - 1]
    return x


def row_cells(nlay, h, q, K, c, edges, kind, drho_dvp=0.32):
    """Per row r: x [R, nper, nb + 1] (longdouble, 0 where the row has no model) and model [R]: 2 <= nlay <= Lmax."""
    R, nper, _, Lmax = K.shape
    x = np.zeros((R, nper, len(edges)), dtype=LD)
    model = (nlay >= 2) & (nlay <= Lmax)
    for r in np.nonzero(model)[0]:
        n = int(nlay[r])
        G = layer_values(K[r][:, :, :n], None if q is None else q[r, :n], kind, drho_dvp)
        with np.errstate(invalid='ignore'):
            x[r] = cells(h[r], n, G, edges)
    return x, model


def summarize(nlay, h, q, K, c, w, edges, kind, drho_dvp=0.32):
    """One set -> dict(total, excluded, n [nper] (int64; n: the rows that count), mean, var, absmean, sqmean, min, max
    [nper, nb + 1] (longdouble; absmean = sum w |x| / W, sqmean = sum w x^2 / W; NaN for a period without weight))."""
    nlay, w = np.asarray(nlay), (np.ones(len(nlay), dtype=np.int64) if w is None else np.asarray(w, dtype=np.int64))
    R, nper = c.shape
    x, model = row_cells(nlay, h, q, K, c, edges, kind, drho_dvp)
    counts = (w > 0)[:, None] & model[:, None] & ~np.isnan(c)                  # [R, nper]
    out = dict(total=np.zeros(nper, dtype=np.int64), excluded=np.zeros(nper, dtype=np.int64), n=np.zeros(nper, dtype=np.int64))
    for k in ('mean', 'var', 'absmean', 'sqmean', 'min', 'max'):
        out[k] = np.full((nper, len(edges)), np.nan, dtype=LD)
    for p in range(nper):
        rows = np.nonzero(counts[:, p])[0]
        out['excluded'][p] = w[(w > 0) & ~counts[:, p]].sum()
        out['n'][p] = rows.size
        X = np.repeat(x[rows, p, :], w[rows], axis=0)                            # the expanded matrix
        out['total'][p] = X.shape[0]
        if X.shape[0]:
            W = LD(X.shape[0])
            out['mean'][p] = X.sum(axis=0) / W
            out['sqmean'][p] = (X * X).sum(axis=0) / W
            out['var'][p] = out['sqmean'][p] - out['mean'][p] ** 2
            out['absmean'][p] = np.abs(X).sum(axis=0) / W
            out['min'][p], out['max'][p] = X.min(axis=0), X.max(axis=0)
    return out
