"""Depth sensitivity kernels of the fundamental-mode phase velocity: dc/dh, dc/dvp, dc/dvs, dc/drho per layer and
period, for Rayleigh and Love waves (csrc/sens_core.h).

    batch(periods, H, VP, VS, RHO, nlay, wave)   the device search and the pass for a batch of models
    vs_total(K, dvp_dvs)                         the derivative with vp tied to vs and rho to vp, BayHunter's parameters
    group_velocity(c, dc_dT, T)                  the analytic group velocity
    to_depth(K, h, edges)                        a layer kernel spread over depth bins

Per model: plugins.SurfDisp.sensitivity; on an engine's own phase velocities: ForwardEngine.sensitivity.

Over an ensemble -- where in depth the data look across all sampled models, and how much that varies between them:

    summarize(periods, wave, models, vpvs, ...)          mean, spread, minimum and maximum of the depth-binned kernel
    summarize_sets(periods, wave, models, set_start, ..) the same for every set of rows (a station) in one pass
    from_sums(total, s1, s2, vmin, vmax)                 the rules, without a device
    ChainPool.sensitivity / StationPool.sensitivity      over a pool's rows (pool_sensitivity, stations_sensitivity)

Per row the device runs the search, the pass (bh_sens_batch) and the reduction bh_sens_sets_* (csrc/sens_sets_core.h);
K never leaves the device.

The same for the group velocity (csrc/sens_group_core.h): U = c / (1 + (T / c) dc/dT) is the
analytic group velocity of the polished root, not the finite difference of two real*4 solves a group target returns, and
K^U = dU/dm follows from the phase kernels at T and at two neighbouring periods.

    group_batch(periods, H, VP, VS, RHO, nlay, wave)     the device search and the group pass for a batch of models
    summarize / summarize_sets (velocity='group')        the depth-binned dU/dm over an ensemble
    ChainPool.group_sensitivity / StationPool.group_sensitivity      (pool_sensitivity, stations_sensitivity)

And for the Rayleigh-wave ellipticity (csrc/ell_sens_core.h): E is H/V at the polished root and
K^E = dE/dm = G_m + G_c dc/dm, the change of H/V per km/s of the layer (per g/cm^3 for 'rho').

    ell_batch(periods, H, VP, VS, RHO, nlay, absolute)   the device search and the ellipticity pass for a batch of models
    summarize / summarize_sets (velocity='ellipticity')  the depth-binned dE/dm over an ensemble
    ChainPool.ell_sensitivity / StationPool.ell_sensitivity          (pool_sensitivity, stations_sensitivity)

And for the receiver function (csrc/rf_sens_core.h): K[t] = dRF(t)/dm, central differences of two
perturbed traces per entry, formed in LDS.  Time samples sit where the other kernels have periods, so vs_total and
to_depth apply unchanged.  Over an ensemble the reduction is bh_rf_sens_sets_* (csrc/rf_sens_sets_core.h; DESIGN.md
section 7k): bh_sens_sets' sums at a selection of the trace's samples, a row counting for all samples or for none.

    rf_batch(rfparams, H, VP, VS, RHO, nlay, ref)        the pass for a batch of models
    plugins.RFminiModRF.sensitivity / ForwardEngine.rf_sensitivity
    rf_summarize(rfparams, models, vpvs, ...)            the depth-binned dRF(t)/dm over an ensemble
    rf_summarize_sets(rfparams, models, set_start, ...)  the same for every set of rows, each at its own ray parameter
    ChainPool.rf_sensitivity / StationPool.rf_sensitivity            (pool_rf_sensitivity, stations_rf_sensitivity)
"""
import collections

import numpy as np

from . import _lib, selection as sel

KINDS = ('h', 'vp', 'vs', 'rho')          # K's kind axis
REFS = {'rayleigh': 'rdispph', 'love': 'ldispph'}
GROUP_REFS = {'rayleigh': 'rdispgr', 'love': 'ldispgr'}
# per velocity: the engine's pass, the key of the value that counts a (row, period), and the doubles per (row, period) the
# pass holds beyond the phase pass's besides its K_phase (None: no K_phase either) -- group: U and the five further
# doubles of workspace; ellipticity: E and the two further doubles of workspace
PASSES = {'phase': ('sensitivity', 'c', None), 'group': ('group_sensitivity', 'U', 6), 'ellipticity': ('ell_sensitivity', 'E', 3)}
VELOCITIES = tuple(PASSES)


def _batch(eng, method, H, VP, VS, RHO, nlay):
    """The search and pass `method` of engine `eng` for B models, every result as a numpy array, plus err [B]."""
    import torch
    models = eng.upload(H, VP, VS, RHO, np.asarray(nlay, dtype=np.int32))
    out, err = eng.run(models)
    res = getattr(eng, method)(models, out=out, err=err)
    torch.cuda.synchronize(eng.device)
    res = {k: v.cpu().numpy() for k, v in res.items()}
    res['err'] = err.cpu().numpy()[:, 0]
    return res


def _phase_engine(periods, wave):
    from .engine import ForwardEngine, SwdSpec
    if wave not in REFS:
        raise ValueError("wave %r: 'rayleigh' or 'love'" % (wave,))
    return ForwardEngine(swd=[SwdSpec(REFS[wave], periods)])


def batch(periods, H, VP, VS, RHO, nlay, wave='rayleigh'):
    """Search and pass on the device for B models ([B, Lmax] arrays, nlay [B]) at up to 60 periods: dict of numpy
    arrays c [B, nper] (the polished phase velocity), dc_dT [B, nper], K [B, nper, 4, Lmax] (KINDS), err [B] (the
    search's flag).  A (model, period) without a value is NaN."""
    return _batch(_phase_engine(periods, wave), 'sensitivity', H, VP, VS, RHO, nlay)


def group_batch(periods, H, VP, VS, RHO, nlay, wave='rayleigh'):
    """batch() for the group velocity: dict of numpy arrays U [B, nper] (the analytic group velocity), dU_dT, c [B, nper],
    K [B, nper, 4, Lmax] = dU/dm (KINDS), K_phase (batch()'s K), err [B] (the phase search's flag).  A (model, period)
    without a value is NaN in all of them."""
    return _batch(_phase_engine(periods, wave), 'group_sensitivity', H, VP, VS, RHO, nlay)


def ell_batch(periods, H, VP, VS, RHO, nlay, absolute=True):
    """batch() for the Rayleigh-wave ellipticity: dict of numpy arrays E [B, nper] (H/V at the polished root; |H/V| with
    absolute), dE_dT, c [B, nper], K [B, nper, 4, Lmax] = dE/dm (KINDS), K_phase (batch()'s K for Rayleigh waves), err [B]
    (the phase search's flag).  A (model, period) without a value is NaN in all of them."""
    from .engine import EllSpec, ForwardEngine
    return _batch(ForwardEngine(ell=[EllSpec('rellip', periods, 0, absolute)]), 'ell_sensitivity', H, VP, VS, RHO, nlay)


def rf_batch(rfparams, H, VP, VS, RHO, nlay, ref='prf'):
    """The receiver-function pass on the device for B models ([B, Lmax] arrays, nlay [B]): dict of numpy arrays
    K [B, nt, 4, Lmax] = dRF(t)/dm (KINDS), rf [B, nt] (the trace, bh_rf_batch's bits) and t [nt].  rfparams: a dict with
    'obsx', the uniformly sampled time axis of the target, and optionally 'gauss' (1.0), 'p' [s/deg] (6.4) and 'nsv'
    (None: the top layer's vs) -- plugins.RFminiModRF's modelparams; ref 'prf' | 'seis' (incident P) or 'srf' (SV).
    NaN in the layers a model does not have, and throughout for a model without a trace."""
    import torch
    from .engine import ForwardEngine
    eng = ForwardEngine(rf=[_rf_spec(rfparams, ref)])
    res = eng.rf_sensitivity(eng.upload(H, VP, VS, RHO, np.asarray(nlay, dtype=np.int32)))
    torch.cuda.synchronize(eng.device)
    return {'K': res['K'].cpu().numpy(), 'rf': res['rf'].cpu().numpy(), 't': res['t']}


def vs_total(K, dvp_dvs, drho_dvp=0.32):
    """dc/dvs per layer when vp = dvp_dvs vs and rho = 0.77 + drho_dvp vp move with vs (BayHunter's parameterisation):
    K_vs + dvp_dvs (K_vp + drho_dvp K_rho).  K [..., 4, L]; dvp_dvs a number or an array that broadcasts against
    [..., L] (a Vp/Vs per model or per layer)."""
    K = np.asarray(K)
    return K[..., 2, :] + np.asarray(dvp_dvs) * (K[..., 1, :] + drho_dvp * K[..., 3, :])


def group_velocity(c, dc_dT, T):
    """U = c / (1 + (T / c) dc/dT), from U = d omega / dk with omega = 2 pi / T and k = omega / c."""
    c, dc_dT, T = (np.asarray(x, dtype=np.float64) for x in (c, dc_dT, T))
    return c / (1.0 + (T / c) * dc_dT)


def to_depth(K, h, edges):
    """A per-layer kernel on depth bins: K [..., L] of a model with thicknesses h [L] (the last entry, the
    half-space's, is ignored) -> (binned [..., nbins], half-space [...]).  Each layer's value is spread over the bins in
    proportion to the overlap of the layer with the bin; what lies outside edges[0] .. edges[-1] is dropped, so the sum
    over the bins and the half-space is the sum over the layers when the edges cover the stack."""
    K = np.asarray(K, dtype=np.float64)
    h = np.asarray(h, dtype=np.float64)
    edges = np.asarray(edges, dtype=np.float64)
    n = h.size
    top = np.concatenate(([0.0], np.cumsum(h[:n - 1])))[:n - 1]
    bot = top + h[:n - 1]
    lo = np.maximum(top[:, None], edges[None, :-1])
    hi = np.minimum(bot[:, None], edges[None, 1:])
    with np.errstate(divide='ignore', invalid='ignore'):
        w = np.where(h[:n - 1, None] > 0, np.clip(hi - lo, 0.0, None) / h[:n - 1, None], 0.0)      # [L-1, nbins]
    return K[..., :n - 1] @ w, K[..., n - 1]


# ---- over an ensemble: the depth-binned kernel's moments per set of rows ---------------------------------------------

_EMPTY = "empty selection (no row with a value at any period)"


def from_sums(total, s1, s2, vmin, vmax):
    """Mean and population standard deviation from bh_sens_sets_finish's sums: total [..., nper] = sum w, s1 = sum w x,
    s2 = sum w x^2, vmin, vmax [..., nper, cells] -> (mean, std) [..., nper, cells]:

        mean = s1 / W,  std = sqrt(max(0, s2 / W - mean^2))

    The variance is exactly 0 where vmin == vmax (every row agrees), whatever the rounding left in s2.  A period with
    W == 0 is NaN."""
    W = np.asarray(total, dtype=np.float64)[..., None]
    s1, s2 = np.asarray(s1, dtype=np.float64), np.asarray(s2, dtype=np.float64)
    with np.errstate(invalid='ignore', divide='ignore'):
        mean = np.where(W > 0, s1 / W, np.nan)
        var = np.maximum(0.0, s2 / W - mean * mean)
    var = np.where(np.asarray(vmin) == np.asarray(vmax), 0.0, var)
    return mean, np.where(W > 0, np.sqrt(var), np.nan)


def default_edges():
    """The depth edges interfaces.summarize uses by default: 1 km bins to 100 km."""
    from .posterior import hist_grids
    return hist_grids(None)[1]


def _check_edges(dep_edges):
    e = np.ascontiguousarray(default_edges() if dep_edges is None else dep_edges, dtype=np.float64)
    if e.ndim != 1 or e.size < 2 or e.size > _lib.SENS_SETS_MAX_BINS + 1:
        raise ValueError("dep_edges: 2 to %d edges" % (_lib.SENS_SETS_MAX_BINS + 1))
    if not np.all(np.isfinite(e)) or np.any(np.diff(e) <= 0):
        raise ValueError("dep_edges: finite and ascending")
    return e


def _check_kind(kind):
    if kind not in _lib.SENS_KINDS:
        raise ValueError("kind %r: 'vp', 'vs', 'rho' or 'vs_total' (dc/dh is an interface derivative, not a depth density)"
                         % (kind,))
    return _lib.SENS_KINDS[kind]


def split_runs(set_start, max_rows):
    """The rows of set_start cut into runs (lo, hi) of at most max_rows rows that bh_sens_sets_add accepts one after the
    other: whole sets as long as they fit; a set larger than max_rows is split at multiples of the block
    (_lib.SENS_SETS_BLOCK_ROWS rows from its first row; one block at least)."""
    set_start = np.asarray(set_start, dtype=np.int64)
    blk, R, max_rows = _lib.SENS_SETS_BLOCK_ROWS, int(set_start[-1]), max(1, int(max_rows))
    runs, lo = [], 0
    while lo < R:
        fits = set_start[(set_start > lo) & (set_start <= lo + max_rows)]
        if fits.size:
            hi = int(fits[-1])
        else:                                   # the set lo lies in does not fit: whole blocks of it
            z = int(np.searchsorted(set_start, lo, side='right')) - 1
            first, end = int(set_start[z]), int(set_start[z + 1])
            hi = min(end, first + max(blk, (lo + max_rows - first) // blk * blk))
            if hi <= lo:
                hi = min(end, lo + blk)
        runs.append((lo, hi))
        lo = hi
    return runs


class _SetsHandle(object):
    """One handle of a depth-binned reduction bh_<name>_*: a subclass creates it and adds run after run, then finish()."""

    def _create(self, name, set_start, own, counts, nitems, edges, kind, drho_dvp, stream):
        """bh_<name>_create with the arguments `own` between the sets and the edges; finish() returns total and excluded
        [sets] + counts and the sums [sets, nitems, bins + 1]."""
        import ctypes as C
        self.lib, self.name, self.stream = _lib.load(), name, stream
        self.set_start = np.ascontiguousarray(set_start, dtype=np.int64)
        self.nsets, self.edges = self.set_start.size - 1, np.ascontiguousarray(edges, dtype=np.float64)
        self.shapes = (self.nsets,) + counts, (self.nsets, nitems, self.edges.size)
        self.h = C.c_void_p()
        _lib.check(getattr(self.lib, 'bh_%s_create' % name)(
            C.byref(self.h), self.set_start.ctypes.data, self.nsets, *own, self.edges.ctypes.data, self.edges.size, int(kind),
            float(drho_dvp), stream))

    def _add(self, row0, models, q, weights, K, *own):
        _lib.check(getattr(self.lib, 'bh_%s_add' % self.name)(
            self.h, int(row0), models.B, models.Lmax, 4 * models.Lmax, models.nlay.data_ptr(), models.H.data_ptr(),
            None if q is None else q.data_ptr(), 0 if q is None else q.stride(0), K.data_ptr(), *own,
            None if weights is None else weights.data_ptr()))

    def finish(self):
        """-> dict(total, excluded int64, s1, s2, vmin, vmax float64): SensSets [sets, nper] and [sets, nper, bins + 1],
        RfSensSets [sets] and [sets, samples, bins + 1]"""
        out = dict(total=np.zeros(self.shapes[0], dtype=np.int64), excluded=np.zeros(self.shapes[0], dtype=np.int64))
        for k in ('s1', 's2', 'vmin', 'vmax'):
            out[k] = np.zeros(self.shapes[1])
        _lib.check(getattr(self.lib, 'bh_%s_finish' % self.name)(self.h, *[out[k].ctypes.data for k in
                                                                         ('total', 'excluded', 's1', 's2', 'vmin', 'vmax')]))
        return out

    def close(self):
        if self.h:
            getattr(self.lib, 'bh_%s_destroy' % self.name)(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class SensSets(_SetsHandle):
    """One bh_sens_sets handle: add(row0, models, K, c, q, weights) run after run, then finish()."""

    def __init__(self, set_start, nper, edges, kind, drho_dvp, stream):
        self.nper = int(nper)
        self._create('sens_sets', set_start, (self.nper,), (self.nper,), self.nper, edges, kind, drho_dvp, stream)

    def add(self, row0, models, K, c, q=None, weights=None):
        """Rows row0 .. of the numbering: models an engine.DeviceModels, K and c what ForwardEngine.sensitivity returned
        for them, q [B, Lmax] float64 or None, weights int32 [B] or None -- device tensors."""
        self._add(row0, models, q, weights, K, c.data_ptr())


def _set_result(sums, z, axes, edges, kind):
    """The dict of set z from a handle's sums, or None for a set without a counting row: summarize()'s with the counts
    [nper] and axes = {'periods': }, rf_summarize()'s with integer counts and axes = {'t': , 'samples': }."""
    total = sums['total'][z]
    if not np.any(total):
        return None
    count = np.copy if np.ndim(total) else int
    mean, std = from_sums(total, sums['s1'][z], sums['s2'][z], sums['vmin'][z], sums['vmax'][z])
    res = {'mean': mean[:, :-1], 'std': std[:, :-1], 'min': sums['vmin'][z][:, :-1].copy(),
           'max': sums['vmax'][z][:, :-1].copy(), 'halfspace_mean': mean[:, -1], 'halfspace_std': std[:, -1],
           'nmodels': count(total), 'nexcluded': count(sums['excluded'][z])}
    res.update(axes, edges=edges, kind=kind)
    return res


# What differs between the two reductions, for _summarize_sets:
#   check(Z)                         the pass's own checks that need the number of sets, before a device is touched
#   engine(dev)                      its ForwardEngine
#   row_bytes(eng, Lmax)             the device bytes a row takes in the pass, for the default max_rows
#   runs(set_start, max_rows)        the runs of rows in order, (lo, hi, ...)
#   handle(set_start, stream)        its SensSets or RfSensSets
#   add(handle, eng, run, dm, q, w)  the pass for the run's models dm, and handle.add
#   result(sums, z)                  the dict of set z, or None
#   empty                            the message of a set whose rows do not count
_Pass = collections.namedtuple('_Pass', 'check engine row_bytes runs handle add result empty')


def _summarize_sets(ps, models, set_start, vpvs, weights, kind, mantle, device, max_rows, strict):
    """summarize_sets and rf_summarize_sets behind their own checks: the checks of the rows, then per run of the _Pass
    `ps` the upload, the layers, q = vp / vs and the pass, and every set's result."""
    import torch
    from . import _device, datafits as df
    from .models import layers_from_voronoi
    shape = getattr(models, 'shape', None) or np.asarray(models).shape
    if len(shape) != 2:
        raise ValueError("models: [rows, 2*maxlayers]")
    R = shape[0]
    set_start, Z = sel.check_set_start(set_start, R)
    vp = None if np.ndim(vpvs) == 0 else vpvs
    if vp is not None and len(vp) != R:
        raise ValueError("vpvs: one per row, or a scalar")
    if weights is not None and len(weights) != R:
        raise ValueError("one weight per row")
    if weights is not None and not hasattr(weights, 'is_cuda') and np.any(np.asarray(weights) < 0):
        raise ValueError("negative weight")
    if max_rows is not None and int(max_rows) < 1:
        raise ValueError("max_rows >= 1")
    ps.check(Z)
    results, failed = [None] * Z, {}
    if R == 0:
        failed = {z: "empty selection: no models" for z in range(Z)}
        sel.raise_first_failed(failed, strict, "set")
        return sel.SetList(results, failed)
    dev = _device.torch_device(device)
    with torch.cuda.device(dev):
        eng = ps.engine(dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        Lmax = shape[1] // 2
        if max_rows is None:       # half of the free device memory: the pass's arrays, the row, its layers (packed, nuclei, q)
            per_row = ps.row_bytes(eng, Lmax) + 8 * (shape[1] + 8 * Lmax) + 16
            max_rows = max(1, int(torch.cuda.mem_get_info(dev)[0] // (2 * per_row)))
        with ps.handle(set_start, stream) as handle:
            for run in ps.runs(set_start, max_rows):
                lo, hi = run[:2]
                rows = _device.to_device(models[lo:hi], torch.float64, dev)
                v = vpvs if vp is None else vp[lo:hi]
                v = _device.to_device(np.broadcast_to(np.asarray(v, dtype=np.float64), (hi - lo,)).copy()
                                      if not isinstance(v, torch.Tensor) else v, torch.float64, dev)
                w = None if weights is None else _device.to_device(weights[lo:hi], torch.int32, dev)
                vsn, zv, nl = df._layers(rows, dev)
                dm, _ = layers_from_voronoi(vsn, zv, nl, v, df._OPEN_PRIORS, mantle=mantle, device=dev)
                ps.add(handle, eng, run, dm, (dm.VP / dm.VS).contiguous() if kind == 'vs_total' else None, w)
            sums = handle.finish()
    for z in range(Z):
        results[z] = ps.result(sums, z)
        if results[z] is None:
            failed[z] = "empty selection: no models" if set_start[z] == set_start[z + 1] else ps.empty
    sel.raise_first_failed(failed, strict, "set")
    return sel.SetList(results, failed)


def summarize_sets(periods, wave, models, set_start, vpvs, weights=None, dep_edges=None, kind='vs_total', mantle=None,
                   device=None, max_rows=None, strict=True, drho_dvp=0.32, velocity='phase', absolute=True):
    """summarize() of every set of rows in one pass: set s is models[set_start[s]:set_start[s + 1]] (set_start
    [sets + 1], ascending from 0 to the number of rows; a set may be empty) with its vpvs and weights.

    periods, wave   up to 60 periods of the fundamental-mode phase velocity; 'rayleigh' or 'love'
    models          [rows, 2*maxlayers], the reference's layout (float32 or float64; numpy or a torch tensor)
    vpvs, mantle    one vp/vs per row, or a scalar; the prior's (vs, vpvs) mantle rule, as for datacov.summarize
    weights         integers >= 0, default 1 each
    dep_edges       depth bin edges shared by all sets (default: interfaces.summarize's, 1 km bins to 100 km)
    kind            'vs_total' (dc/dvs with vp = vpvs vs and rho = 0.77 + drho_dvp vp moving along), 'vp', 'vs' or 'rho'
    max_rows        the rows are taken in runs of whole sets that fit max_rows, a larger set in whole blocks (default:
                    what half of the free device memory holds); per run the layers, the search, the pass
                    (ForwardEngine.sensitivity), q = vp / vs and bh_sens_sets_add; no result depends on it
    velocity        'phase' (dc/dm), or 'group': the pass is ForwardEngine.group_sensitivity, the reduction receives dU/dm
                    and counts a (row, period) by its U, and the dicts carry 'velocity': 'group'; or 'ellipticity'
                    (wave 'rayleigh' only): the pass is ForwardEngine.ell_sensitivity, the reduction receives dE/dm --
                    of |H/V| with `absolute`, else of the signed ratio -- and counts a (row, period) by its E; the
                    values are then changes of H/V per km/s (per g/cm^3), and the dicts carry 'velocity': 'ellipticity'
                    (its 'vs_total' is formed per layer in vs_total()'s own operation order, bh_ell_sens_vs_total: the
                    two parts cancel at short periods)

    -> a selection.SetList of dicts(mean, std, min, max [nper, bins]: km/s per km/s (per g/cm^3 for 'rho') of the layer
    kernel that falls into the bin; halfspace_mean, halfspace_std [nper]; nmodels, nexcluded [nper] (weighted rows that
    count; left out: no model, a failed search, no root); periods, edges, kind), every field bit for bit what summarize
    returns for the set's rows alone.  A set without a row that counts at any period raises a ValueError naming the
    first such set -- or, with strict=False, has the entry None and its message in the list's `failed`."""
    from .engine import EllSpec, ForwardEngine, SwdSpec
    if wave not in REFS:
        raise ValueError("wave %r: 'rayleigh' or 'love'" % (wave,))
    if velocity not in VELOCITIES:
        raise ValueError("velocity %r: 'phase', 'group' or 'ellipticity'" % (velocity,))
    if velocity == 'ellipticity' and wave != 'rayleigh':
        raise ValueError("velocity 'ellipticity': wave %r; the ellipticity is the Rayleigh wave's" % (wave,))
    method, counted, extra = PASSES[velocity]
    code, edges = _check_kind(kind), _check_edges(dep_edges)
    periods = np.ascontiguousarray(periods, dtype=np.float64)
    nper = periods.size
    # The ellipticity's K_vs and (vp / vs) K_vp cancel to 1e-7 of their size at short periods: its 'vs_total' is formed
    # per layer in vs_total()'s own operation order (bh_ell_sens_vs_total, in place of K_vs) and reduced as kind 'vs'
    plain_total = velocity == 'ellipticity' and kind == 'vs_total'
    if plain_total:
        code = _lib.SENS_KINDS['vs']

    def check(Z):
        if periods.ndim != 1 or nper < 1:
            raise ValueError("periods: one at least")
        if SwdSpec(REFS[wave], periods).resample:
            raise ValueError("sensitivity: target '%s' has more than %d periods"
                             % ('rellip' if velocity == 'ellipticity' else REFS[wave], _lib.MAX_PERIODS))

    def engine(dev):
        if velocity == 'ellipticity':          # its phase velocities are a hidden 'rdispph' target's, as in an inversion
            return ForwardEngine(ell=[EllSpec('rellip', periods, 0, absolute)], device=dev)
        return ForwardEngine(swd=[SwdSpec(REFS[wave], periods)], device=dev)

    def row_bytes(eng, Lmax):                  # K, c, dc/dT and the workspace; a second K and the pass's own beyond the phase's
        return 8 * (4 * nper * Lmax + 3 * nper + eng.row + (0 if extra is None else 4 * nper * Lmax + extra * nper))

    def add(handle, eng, run, dm, q, w):
        out, err = eng.run(dm)
        res = getattr(eng, method)(dm, out=out, err=err)
        K = res['K']
        if plain_total:
            _lib.check(handle.lib.bh_ell_sens_vs_total(dm.B, dm.Lmax, nper, K.data_ptr(), q.data_ptr(), q.stride(0),
                                                       float(drho_dvp), K.data_ptr(), handle.stream))
            q = None
        handle.add(run[0], dm, K, res[counted], q, w)

    def result(sums, z):
        res = _set_result(sums, z, {'periods': periods}, edges, kind)
        if res is not None and velocity != 'phase':                     # (the phase result keeps the keys it had)
            res['velocity'] = velocity
        return res
    return _summarize_sets(_Pass(check, engine, row_bytes, split_runs,
                                 lambda set_start, stream: SensSets(set_start, nper, edges, code, drho_dvp, stream), add,
                                 result, _EMPTY),
                           models, set_start, vpvs, weights, kind, mantle, device, max_rows, strict)


def summarize(periods, wave, models, vpvs, weights=None, dep_edges=None, kind='vs_total', mantle=None, device=None,
              max_rows=None, drho_dvp=0.32, velocity='phase', absolute=True):
    """The depth-binned sensitivity kernel over one set of sampled models: summarize_sets' dict for all rows (see there).
    ValueError for an empty selection."""
    shape = getattr(models, 'shape', None) or np.asarray(models).shape
    res = summarize_sets(periods, wave, models, [0, shape[0] if len(shape) == 2 else 0], vpvs, weights, dep_edges, kind,
                         mantle, device, max_rows, strict=False, drho_dvp=drho_dvp, velocity=velocity, absolute=absolute)
    if res[0] is None:
        raise ValueError(res.failed[0])
    return res[0]


# ---- chain pools ----------------------------------------------------------------------------------------------------------

def pool_target(targets, ref=None, velocity='phase'):
    """The dispersion target of a JointTarget the kernels are formed for -> (wave, periods, ref).  ref None: its only
    fundamental-mode phase target -- for velocity 'group' its only fundamental-mode group target, and a ValueError when
    there is none (a phase target is served when it is named).  ValueError for a pool
    without a dispersion target, an ambiguous choice, and -- in ForwardEngine.sensitivity's words -- a target the pass
    does not serve.  The group pass serves phase and group targets alike: the wave type and the periods matter.
    velocity 'ellipticity': the pool's ellipticity target (ref None: its only one) -> ('rayleigh', periods, ref);
    ValueError for a pool without one, for flsph = 1 and for more than 60 periods."""
    from .layout import SWD_REFS
    if velocity == 'ellipticity':
        spec = _ell_spec(targets, ref)
        return 'rayleigh', spec.periods, spec.ref
    specs = targets.batch_layout(ell=True)['layout'].swd
    if not specs:
        raise ValueError("sensitivity: the pool has no dispersion target")
    if ref is None:
        served = [sp for sp in specs if sp.igr == (1 if velocity == 'group' else 0) and sp.mode == 1]
        if len(served) > 1:
            raise ValueError("sensitivity: ref is one of %s" % ', '.join(repr(sp.ref) for sp in served))
        if velocity == 'group' and not served:
            raise ValueError("sensitivity: the pool has no fundamental-mode group target; name one of %s as ref"
                             % ', '.join(repr(sp.ref) for sp in specs))
        spec = served[0] if served else specs[0]
    else:
        if ref not in SWD_REFS or not any(sp.ref == ref for sp in specs):
            raise ValueError("sensitivity: no dispersion target %r (there are %s)" % (ref, ', '.join(sp.ref for sp in specs)))
        spec = next(sp for sp in specs if sp.ref == ref)
    if spec.igr != 0 and velocity != 'group':
        raise ValueError("sensitivity: target '%s' has igr = %d; group-velocity targets are not served" % (spec.ref, spec.igr))
    if spec.mode != 1:
        raise ValueError("sensitivity: target '%s' has mode = %d; only the fundamental mode is served" % (spec.ref, spec.mode))
    if spec.flsph != 0:
        raise ValueError("sensitivity: target '%s' has flsph = %d; only a flat earth is served" % (spec.ref, spec.flsph))
    if spec.resample:
        raise ValueError("sensitivity: target '%s' has more than %d periods" % (spec.ref, _lib.MAX_PERIODS))
    return {1: 'love', 2: 'rayleigh'}[spec.iwave], spec.periods, spec.ref


def _ell_spec(targets, ref=None):
    """The EllSpec of a JointTarget's ellipticity target `ref` (None: its only one), checked for what the pass serves."""
    from .layout import ELL_REFS
    specs = targets.batch_layout(ell=True)['layout'].ell
    if not specs:
        raise ValueError("sensitivity: the pool has no ellipticity target")
    if ref is None:
        if len(specs) > 1:
            raise ValueError("sensitivity: ref is one of %s" % ', '.join(repr(sp.ref) for sp in specs))
        spec = specs[0]
    else:
        if ref not in ELL_REFS or not any(sp.ref == ref for sp in specs):
            raise ValueError("sensitivity: no ellipticity target %r (there are %s)" % (ref, ', '.join(sp.ref for sp in specs)))
        spec = next(sp for sp in specs if sp.ref == ref)
    if spec.flsph != 0:
        raise ValueError("sensitivity: target '%s' has flsph = %d; only a flat earth is served" % (spec.ref, spec.flsph))
    if spec.periods.size > _lib.MAX_PERIODS:
        raise ValueError("sensitivity: target '%s' has more than %d periods" % (spec.ref, _lib.MAX_PERIODS))
    return spec


def _pool_absolute(targets, tref, velocity):
    return _ell_spec(targets, tref).absolute if velocity == 'ellipticity' else True


def pool_sensitivity(pool, ref=None, dep_edges=None, kind='vs_total', selection='weighted', dev=0.05,
                     exclude_outliers=True, device=None, max_rows=None, velocity='phase'):
    """ChainPool.sensitivity (velocity 'group': ChainPool.group_sensitivity; 'ellipticity': ChainPool.ell_sensitivity,
    with the target's `absolute`): summarize() over the rows
    ChainPool.posterior uses, plus 'ref' and 'chains' (global indices used)."""
    wave, periods, tref = pool_target(pool.targets, ref, velocity)
    ci, ri, w = sel.pool_rows(pool, selection, dev, exclude_outliers)
    res = summarize(periods, wave, pool.models[ci, ri], pool.vpvs[ci, ri].astype(np.float64), w.astype(np.int32),
                    dep_edges, kind, pool.priors.get('mantle'), device, max_rows, velocity=velocity,
                    absolute=_pool_absolute(pool.targets, tref, velocity))
    res['ref'] = tref
    res['chains'] = np.unique(ci) + pool.first
    return res


class _StationArrays(sel.StationResult):
    """What StationSensitivity and StationRfSensitivity share: `stations`, ref, edges, kind, and the per-station arrays
    of n periods or samples -- the counts [nstations] + counts -- filled from the stations' dicts."""

    def __init__(self, names, results, failed, ref, edges, kind, n, counts):
        sel.StationResult.__init__(self, names, failed)
        self.stations = {name: r for name, r in zip(names, results) if r is not None}
        self.ref, self.edges, self.kind = ref, edges, kind
        Z, nb = len(results), edges.size - 1
        for k in ('mean', 'std', 'min', 'max'):
            setattr(self, k, np.full((Z, n, nb), np.nan))
        self.halfspace_mean, self.halfspace_std = np.full((Z, n), np.nan), np.full((Z, n), np.nan)
        self.nmodels, self.nexcluded = np.zeros((Z,) + counts, dtype=np.int64), np.zeros((Z,) + counts, dtype=np.int64)
        for z, r in enumerate(results):
            if r is not None:
                for k in ('mean', 'std', 'min', 'max', 'halfspace_mean', 'halfspace_std', 'nmodels', 'nexcluded'):
                    getattr(self, k)[z] = r[k]


def _finish_stations(spool, res, failed, strict, ref, ci, set_start):
    """The end of both station calls: the sets' failures join the stations' (raised with `strict`), and every station's
    dict gets 'ref' and 'chains'."""
    for z, msg in res.failed.items():
        failed.setdefault(z, msg)
    sel.raise_first_failed(failed, strict, "station", spool.names)
    for z, r in enumerate(res):
        if r is not None:
            r['ref'] = ref
            r['chains'] = sel.station_chains(ci, set_start, z, spool.chains_per_station)


class StationSensitivity(_StationArrays):
    """StationPool.sensitivity's result, every array in the pool's station order.

    names, failed    the stations; {station name: message} (such a station is NaN throughout)
    stations         {station name: the dict pool.station(name).sensitivity(...) returns}, failed stations left out
    ref, periods, edges, kind   the target, its periods and the depth edges all stations share
    mean, std, min, max [nstations, nper, bins], halfspace_mean, halfspace_std [nstations, nper] (float64, NaN for a
    failed station), nmodels, nexcluded [nstations, nper] (0 for a failed station)"""

    velocity = 'phase'      # 'group' on StationPool.group_sensitivity's result, 'ellipticity' on ell_sensitivity's

    def __init__(self, names, results, failed, ref, periods, edges, kind):
        self.periods = periods
        _StationArrays.__init__(self, names, results, failed, ref, edges, kind, periods.size, (periods.size,))


def stations_sensitivity(spool, ref=None, dep_edges=None, kind='vs_total', selection='weighted', dev=0.05,
                         exclude_outliers=True, device=None, max_rows=None, strict=False, velocity='phase'):
    """StationPool.sensitivity (velocity 'group': StationPool.group_sensitivity; 'ellipticity':
    StationPool.ell_sensitivity): summarize_sets() over every station's main-phase rows."""
    pool, c = spool.pool, spool.chains_per_station
    wave, periods, tref = pool_target(spool.stations[0], ref, velocity)
    edges = _check_edges(dep_edges)
    ci, ri, w, set_start, failed = sel.station_rows(pool, c, selection, dev, exclude_outliers)
    res = summarize_sets(periods, wave, pool.models[ci, ri], set_start, pool.vpvs[ci, ri].astype(np.float64),
                         w.astype(np.int32), edges, kind, pool.priors.get('mantle'), device, max_rows, strict=False,
                         velocity=velocity, absolute=_pool_absolute(spool.stations[0], tref, velocity))
    _finish_stations(spool, res, failed, strict, tref, ci, set_start)
    out = StationSensitivity(spool.names, res, failed, tref, periods, edges, kind)
    if velocity != 'phase':
        out.velocity = velocity
    return out


# ---- the receiver function over an ensemble: depth-binned dRF(t)/dm per set of rows and selected sample --------------------

_RF_EMPTY = "empty selection (no row with a trace)"


def _rf_spec(rfparams, ref='prf'):
    """rf_batch's rfparams (or a layout.RfSpec) -> layout.RfSpec"""
    from .layout import RfSpec
    if isinstance(rfparams, RfSpec):
        return rfparams
    unknown = set(rfparams) - {'obsx', 'gauss', 'p', 'nsv', 'water', 'wtype'}
    if 'obsx' not in rfparams or unknown:
        raise ValueError("rfparams: a dict with 'obsx' and optionally 'gauss', 'p', 'nsv' (unknown: %s)" % sorted(unknown))
    return RfSpec(ref, rfparams['obsx'], rfparams.get('gauss', 1.0), rfparams.get('p', 6.4), rfparams.get('nsv'),
                  wtype=rfparams.get('wtype'))


def rf_time_axis(spec):
    """The time of every sample of K and of the trace that ForwardEngine.rf_sensitivity returns for `spec`."""
    return (np.arange(int(spec.nsamp)) / spec.fsamp - spec.tshft)[:spec.obsx.size]


def rf_samples(taxis, t=None, every=1):
    """The samples rf_summarize reads: those with t[0] <= time <= t[1] (None: all), every `every`-th of them."""
    every = int(every)
    if every < 1:
        raise ValueError("every >= 1")
    idx = np.arange(taxis.size)
    if t is not None:
        if len(t) != 2 or not t[0] <= t[1]:
            raise ValueError("t: (tmin, tmax)")
        idx = idx[(taxis >= t[0]) & (taxis <= t[1])]
    idx = idx[::every]
    if idx.size < 1:
        raise ValueError("t, every: no sample of the trace is selected")
    return np.ascontiguousarray(idx, dtype=np.int32)


class RfSensSets(_SetsHandle):
    """One bh_rf_sens_sets handle: add(row0, models, K, rf, q, weights) run after run, then finish()."""

    def __init__(self, set_start, nout, samples, edges, kind, drho_dvp, stream):
        self.nout, self.samples = int(nout), np.ascontiguousarray(samples, dtype=np.int32)
        self._create('rf_sens_sets', set_start, (self.nout, self.samples.ctypes.data, self.samples.size), (),
                     self.samples.size, edges, kind, drho_dvp, stream)

    def add(self, row0, models, K, rf, q=None, weights=None):
        """Rows row0 .. of the numbering: models an engine.DeviceModels, K and rf what ForwardEngine.rf_sensitivity
        returned for them, q [B, Lmax] float64 or None, weights int32 [B] or None -- device tensors."""
        self._add(row0, models, q, weights, K, K.stride(0), rf.data_ptr(), rf.stride(0))


def _p_runs(runs, set_start, p):
    """split_runs' runs cut further wherever the ray parameter changes between sets -> [(lo, hi, p)]."""
    out = []
    for lo, hi in runs:
        z = int(np.searchsorted(set_start, lo, side='right')) - 1      # the set row lo lies in (the empty ones before it skipped)
        a, pa = lo, p[z]
        while True:
            end = min(hi, int(set_start[z + 1]))
            if end >= hi:
                out.append((a, hi, pa))
                break
            z = int(np.searchsorted(set_start, end, side='right')) - 1
            if p[z] != pa:
                out.append((a, end, pa))
                a, pa = end, p[z]
    return out


def rf_summarize_sets(rfparams, models, set_start, vpvs, weights=None, dep_edges=None, kind='vs_total', ref='prf', t=None,
                      every=1, mantle=None, device=None, max_rows=None, drho_dvp=0.32, p=None, strict=True):
    """rf_summarize() of every set of rows in one pass: set s is models[set_start[s]:set_start[s + 1]] with its vpvs and
    weights (set_start as for summarize_sets).

    rfparams        rf_batch's: a dict with 'obsx', the target's time axis, and optionally 'gauss', 'p', 'nsv', 'wtype'
    models, vpvs, mantle, weights, dep_edges, kind, drho_dvp     as for summarize_sets
    ref             'prf' | 'seis' (incident P) or 'srf' (SV)
    t, every        the samples the reduction reads: those with t[0] <= time <= t[1] (None: all), every `every`-th of them
    p               None: rfparams' ray parameter; a number; or one per set (a station's own)
    max_rows        the rows are taken in split_runs' runs, cut further wherever p changes between sets; per run the
                    layers, the pass (ForwardEngine.rf_sensitivity at the run's p), q = vp / vs and bh_rf_sens_sets_add.
                    Default: what half of the free device memory holds, K counted at 8 nout 4 Lmax bytes a row; no
                    result depends on it

    -> a selection.SetList of dicts(mean, std, min, max [nsel, bins]: change of the trace's sample per km/s (per g/cm^3
    for 'rho') of the layer kernel that falls into the bin; halfspace_mean, halfspace_std [nsel]; nmodels, nexcluded
    (integers: the weighted rows that count; left out: no model, no trace); t [nsel], samples (their indices), edges,
    kind), every field bit for bit what rf_summarize returns for the set's rows alone at the set's p.  A set without a row
    that counts raises a ValueError naming the first such set -- or, with strict=False, has the entry None and its message
    in the list's `failed`."""
    from .engine import ForwardEngine
    code, edges = _check_kind(kind), _check_edges(dep_edges)
    spec = _rf_spec(rfparams, ref)
    taxis = rf_time_axis(spec)
    nout = taxis.size
    if nout > _lib.RF_SENS_SETS_MAX_SAMPLES:
        raise ValueError("rf_sensitivity: the trace has more than %d samples" % _lib.RF_SENS_SETS_MAX_SAMPLES)
    samples = rf_samples(taxis, t, every)

    def check(Z):
        if Z * samples.size * edges.size * 32 > _lib.RF_SENS_SETS_MAX_ACC_BYTES:
            raise ValueError("rf_sensitivity: %d sets x %d samples x %d cells exceed the accumulator budget of %d bytes; "
                             "narrow t or raise every" % (Z, samples.size, edges.size, _lib.RF_SENS_SETS_MAX_ACC_BYTES))
        if p is not None and np.ndim(p) != 0 and len(p) != Z:
            raise ValueError("p: a number, or one per set")
        if p is not None and not np.all(np.isfinite(np.asarray(p, dtype=np.float64))):
            raise ValueError("p: finite")

    def runs(set_start, max_rows):
        pz = np.broadcast_to(np.asarray(spec.p if p is None else p, dtype=np.float64), (set_start.size - 1,))
        return _p_runs(split_runs(set_start, max_rows), set_start, pz)

    def add(handle, eng, run, dm, q, w):
        res = eng.rf_sensitivity(dm, p=None if p is None else float(run[2]))
        handle.add(run[0], dm, res['K'], res['rf'], q, w)
    return _summarize_sets(_Pass(check, lambda dev: ForwardEngine(rf=[spec], device=dev),
                                 lambda eng, Lmax: 8 * (nout * 4 * Lmax + nout), runs,               # (K and the trace)
                                 lambda set_start, stream: RfSensSets(set_start, nout, samples, edges, code, drho_dvp, stream),
                                 add, lambda sums, z: _set_result(sums, z, {'t': taxis[samples], 'samples': samples.copy()},
                                                                  edges, kind), _RF_EMPTY),
                           models, set_start, vpvs, weights, kind, mantle, device, max_rows, strict)


def rf_summarize(rfparams, models, vpvs, weights=None, dep_edges=None, kind='vs_total', ref='prf', t=None, every=1,
                 mantle=None, device=None, max_rows=None, drho_dvp=0.32):
    """The depth-binned receiver-function sensitivity kernel over one set of sampled models: rf_summarize_sets' dict for
    all rows (see there).  ValueError for an empty selection."""
    shape = getattr(models, 'shape', None) or np.asarray(models).shape
    res = rf_summarize_sets(rfparams, models, [0, shape[0] if len(shape) == 2 else 0], vpvs, weights, dep_edges, kind, ref,
                            t, every, mantle, device, max_rows, drho_dvp, strict=False)
    if res[0] is None:
        raise ValueError(res.failed[0])
    return res[0]


def pool_rf_target(targets, ref=None):
    """The receiver-function target of a JointTarget the kernels are formed for -> (layout.RfSpec, its index among the
    receiver-function targets).  ref None: its only one.  ValueError for a pool without a receiver-function target, an
    ambiguous choice and an unknown ref."""
    specs = targets.batch_layout(ell=True)['layout'].rf
    if not specs:
        raise ValueError("rf_sensitivity: the pool has no receiver-function target")
    if ref is None:
        if len(specs) > 1:
            raise ValueError("rf_sensitivity: ref is one of %s" % ', '.join(repr(sp.ref) for sp in specs))
        return specs[0], 0
    if not any(sp.ref == ref for sp in specs):
        raise ValueError("rf_sensitivity: no receiver-function target %r (there are %s)" % (ref, ', '.join(sp.ref for sp in specs)))
    i = next(i for i, sp in enumerate(specs) if sp.ref == ref)
    return specs[i], i


def pool_rf_sensitivity(pool, ref=None, dep_edges=None, kind='vs_total', t=None, every=1, selection='weighted', dev=0.05,
                        exclude_outliers=True, device=None, max_rows=None):
    """ChainPool.rf_sensitivity: rf_summarize() over the rows ChainPool.posterior uses, at the target's gauss, p, nsv,
    wave type and time axis, plus 'ref' and 'chains' (global indices used)."""
    spec, _ = pool_rf_target(pool.targets, ref)
    ci, ri, w = sel.pool_rows(pool, selection, dev, exclude_outliers)
    res = rf_summarize(spec, pool.models[ci, ri], pool.vpvs[ci, ri].astype(np.float64), w.astype(np.int32), dep_edges, kind,
                       spec.ref, t, every, pool.priors.get('mantle'), device, max_rows)
    res['ref'] = spec.ref
    res['chains'] = np.unique(ci) + pool.first
    return res


class StationRfSensitivity(_StationArrays):
    """StationPool.rf_sensitivity's result, every array in the pool's station order.

    names, failed    the stations; {station name: message} (such a station is NaN throughout)
    stations         {station name: the dict pool.station(name).rf_sensitivity(...) returns}, failed stations left out
    ref, t, samples, edges, kind   the target, the selected samples' times and indices, the depth edges all stations share
    p                [nstations] the ray parameter every station's kernels were formed at
    mean, std, min, max [nstations, nsel, bins], halfspace_mean, halfspace_std [nstations, nsel] (float64, NaN for a
    failed station), nmodels, nexcluded [nstations] (0 for a failed station)"""

    def __init__(self, names, results, failed, ref, t, samples, edges, kind, p):
        self.t, self.samples, self.p = t, samples, p
        _StationArrays.__init__(self, names, results, failed, ref, edges, kind, t.size, ())


def stations_rf_sensitivity(spool, ref=None, dep_edges=None, kind='vs_total', t=None, every=1, selection='weighted',
                            dev=0.05, exclude_outliers=True, device=None, max_rows=None, strict=False):
    """StationPool.rf_sensitivity: rf_summarize_sets() over every station's main-phase rows, every station at its own ray
    parameter when the pool was built with per_station=('p',)."""
    pool, c = spool.pool, spool.chains_per_station
    spec, i = pool_rf_target(spool.stations[0], ref)
    edges = _check_edges(dep_edges)
    p = np.array([pool_rf_target(joint, spec.ref)[0].p for joint in spool.stations], dtype=np.float64)
    ci, ri, w, set_start, failed = sel.station_rows(pool, c, selection, dev, exclude_outliers)
    res = rf_summarize_sets(spec, pool.models[ci, ri], set_start, pool.vpvs[ci, ri].astype(np.float64), w.astype(np.int32),
                            edges, kind, spec.ref, t, every, pool.priors.get('mantle'), device, max_rows,
                            p=p if 'p' in spool.per_station else None, strict=False)
    _finish_stations(spool, res, failed, strict, spec.ref, ci, set_start)
    taxis = rf_time_axis(spec)
    samples = rf_samples(taxis, t, every)
    return StationRfSensitivity(spool.names, res, failed, spec.ref, taxis[samples], samples, edges, kind, p)
