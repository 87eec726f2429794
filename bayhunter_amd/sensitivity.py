"""Depth sensitivity kernels of the fundamental-mode phase velocity: dc/dh, dc/dvp, dc/dvs, dc/drho per layer and
period, for Rayleigh and Love waves (csrc/sens_core.h).

    batch(periods, H, VP, VS, RHO, nlay, wave)   the device search and the pass for a batch of models
    vs_total(K, dvp_dvs)                         the derivative with vp tied to vs and rho to vp, BayHunter's parameters
    group_velocity(c, dc_dT, T)                  the analytic group velocity
    to_depth(K, h, edges)                        a layer kernel spread over depth bins

Per model: plugins.SurfDisp.sensitivity; on an engine's own phase velocities: ForwardEngine.sensitivity.
"""
import numpy as np

KINDS = ('h', 'vp', 'vs', 'rho')          # K's kind axis
REFS = {'rayleigh': 'rdispph', 'love': 'ldispph'}


def batch(periods, H, VP, VS, RHO, nlay, wave='rayleigh'):
    """Search and pass on the device for B models ([B, Lmax] arrays, nlay [B]) at up to 60 periods: dict of numpy
    arrays c [B, nper] (the polished phase velocity), dc_dT [B, nper], K [B, nper, 4, Lmax] (KINDS), err [B] (the
    search's flag).  A (model, period) without a value is NaN."""
    import torch
    from .engine import ForwardEngine, SwdSpec
    if wave not in REFS:
        raise ValueError("wave %r: 'rayleigh' or 'love'" % (wave,))
    eng = ForwardEngine(swd=[SwdSpec(REFS[wave], periods)])
    models = eng.upload(H, VP, VS, RHO, np.asarray(nlay, dtype=np.int32))
    out, err = eng.run(models)
    res = eng.sensitivity(models, out=out, err=err)
    torch.cuda.synchronize(eng.device)
    res = {k: v.cpu().numpy() for k, v in res.items()}
    res['err'] = err.cpu().numpy()[:, 0]
    return res


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
