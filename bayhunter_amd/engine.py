"""Batched forward engine: many layered models per launch, inputs and outputs resident in HBM.

This is the entry point the reference does not have (it evaluates one model per call,
src/Targets.py:314-347); the single-model plugin classes in plugins.py are
thin views on it.  torch is used only for device memory and streams.
"""
import ctypes as C
import os

import numpy as np
import torch

from . import _lib
from .layout import ELL_REFS, ORDER_MIN, RF_REFS, SWD_REFS, EllSpec, RfSpec, RowLayout, SwdSpec, rf_obsparams  # noqa: F401 (re-exported)


class DeviceModels(object):
    """A batch of layered models resident in HBM: `packed` is [B, 4, Lmax] fp64 (h, vp, vs, rho
    rows of each model contiguous, zero padded), `nlay` int32 [B].  H/VP/VS/RHO are views."""

    def __init__(self, packed, nlay, order=None, depth=None, mean_depth=None):
        assert packed.dim() == 3 and packed.shape[1] == 4 and packed.is_contiguous()
        self.packed, self.nlay = packed, nlay
        self.B, self.Lmax = packed.shape[0], packed.shape[2]
        # mean layer count when the host knows it: a ragged batch is priced by it, not by its deepest model
        # (bh_swd_hint)
        self.mean_depth = None if mean_depth is None else float(mean_depth)
        # deepest model of the batch when the host knows it (<= Lmax): the kernels size their LDS
        # images and pick the team width by it instead of by the allocated row length
        self.depth = None if depth is None else max(1, min(int(depth), self.Lmax))
        self.H, self.VP, self.VS, self.RHO = (packed[:, i, :] for i in range(4))
        # Processing order of the dispersion searches (int32 permutation, ForwardEngine.reorder):
        # the data stay where they are and results land in the caller's rows.
        self.order = order


class ForwardEngine(object):
    """All targets of a joint inversion for a batch of models in (at most) two launches.

    Output row of model b: [swd target 0 | swd target 1 | ... | rf target 0 | ... | ellipticity target 0 | ...], fp64,
    `ncols` values; `slices[t]` is target t's column range.  Rows are `row` doubles apart: with a dispersion
    target of more than 60 periods `row` > `ncols` (the 60 solved values live behind the visible
    columns and are interpolated into them after the kernel).

    An ellipticity target (EllSpec) is one more launch, bh_ell_batch, behind the dispersion launch on the same stream:
    it reads the phase velocities of an equal 'rdispph' target of `swd`, or of a hidden one the layout adds behind the
    visible columns (layout.RowLayout).  `err` then has a column per solved dispersion target, the hidden ones last.
    ell_flags=True launches bh_ell_batch_rows instead, in the run's processing order if it has one: the same values,
    and a model without an ellipticity (water on top, a half-space alone, a period without a phase velocity) gets
    BH_ELL_NO_VALUE in its source target's column of `err`, as in an evaluation plan -- the likelihood then refuses
    the row.  The default leaves `err` as the dispersion launch wrote it.
    """

    def __init__(self, swd=(), rf=(), device=None, ell=(), ell_flags=False):
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise _lib.BayHunterAmdError("no HIP device visible to torch; there is no CPU fallback")
        self.device = torch.device('cuda', torch.cuda.current_device()) if device is None \
            else torch.device(device)
        self.layout = lay = RowLayout(swd, rf, ell)
        self.swd, self.rf, self.ell = lay.swd, lay.rf, lay.ell
        self.ell_flags = bool(ell_flags)
        self._nswd = len(lay.swd_all)        # dispersion targets the library solves: the visible and the hidden ones
        self.slices, self.ncols, self.row = lay.slices, lay.ncols, lay.row
        self._tg, self._rfp = lay.tg, lay.rfp
        with torch.cuda.device(self.device):
            self.periods = torch.from_numpy(lay.periods).to(self.device)
            # observed periods of every target with more than 60: the library interpolates to them on the device
            self._obsx = [torch.from_numpy(sp.obsx).to(self.device) for _, _, _, sp in lay.resampled]
        self._interp = lay.interp([x.data_ptr() for x in self._obsx])
        # per launch stream (batches may be in flight on several streams at once, chains.GpuEvaluator):
        self._ws = {}            # workspace of bh_swd_batch
        self._side = {}          # side stream: RF back-fills the SIMDs the SWD tail leaves idle
        self.overlap = True
        self.sort_ragged = True  # re-order ragged batches by layer count at upload
        self.order_by_length = os.environ.get('BH_ORDER_BY_LENGTH', '1') != '0'   # (A/B switch)

    # -- helpers
    def _as_dev(self, x, dtype):
        if isinstance(x, torch.Tensor):
            if x.device != self.device or x.dtype != dtype or not x.is_contiguous():
                x = x.to(device=self.device, dtype=dtype).contiguous()
            return x
        return torch.from_numpy(np.ascontiguousarray(x)).to(device=self.device, dtype=dtype)

    def upload(self, H, VP, VS, RHO, nlay):
        """[B, Lmax] arrays (+ int nlay[B]) -> DeviceModels: one packed [B, 4, Lmax] device tensor,
        i.e. one contiguous 32*Lmax-byte block per model, which is what a lane fetches from the
        work queue."""
        f64 = torch.float64
        parts = [self._as_dev(x, f64) for x in (H, VP, VS, RHO)]
        packed = torch.stack(parts, dim=1).contiguous()
        known = isinstance(nlay, np.ndarray) and nlay.size
        depth = int(np.max(nlay)) if known else None
        mean = float(np.mean(np.clip(nlay, 0, None))) if known else None
        nlay = self._as_dev(nlay, torch.int32)
        return self.reorder(packed, nlay, depth=depth, mean_depth=mean)

    def reorder(self, packed, nlay, ragged=None, depth=None, mean_depth=None):
        """DeviceModels for a packed [B, 4, Lmax] device tensor, with a processing order for large
        batches.  Three keys, one sort (no data move; bh_swd_batch_ordered takes the permutation):
          1. deepest models first: the layer loop of a wave runs to its deepest model;
          2. longest searches first: persistent lanes run a handful of searches each, so a launch ends
             with a tail in which lanes wait for the last searches -- shorter if those are short ones.
             A search costs ~11 evaluations per period plus one per 0.005 km/s between the start value
             (0.855 c_R of the slowest layer) and the phase velocity at the longest period; the
             predictor is a depth-kernel average of vs at that period minus 0.79 min(vs), in classes of
             0.15 km/s (5 % at 524 288 ten-layer models, tools/divergence_probe.py);
          3. within a class by the S-wave travel time through the stack: the lanes of a wave run in
             lock step, so neighbours should be alike (10 % over a random order,
             profiles/r01_divergence_probe.txt).
        (`ragged` is accepted for compatibility.)"""
        order = None
        if self.sort_ragged and self._nswd and packed.shape[0] > ORDER_MIN:
            B, L = packed.shape[0], packed.shape[2]
            keys = torch.empty(B, dtype=torch.int32, device=self.device)
            tmax = max(float(sp.periods.max()) for sp in self.layout.swd_all)
            st = torch.cuda.current_stream(self.device)
            with torch.cuda.device(self.device):
                _lib.check(self.lib.bh_swd_order_keys(
                    B, L, 4 * L, nlay.data_ptr(), packed[:, 0, :].data_ptr(), packed[:, 2, :].data_ptr(),
                    tmax, 1 if self.order_by_length else 0, keys.data_ptr(), C.c_void_p(st.cuda_stream)))
            order = torch.argsort(keys).to(torch.int32)
        return DeviceModels(packed, nlay, order, depth, mean_depth)

    def alloc_out(self, B):
        out = torch.empty((B, self.row), dtype=torch.float64, device=self.device)
        err = torch.empty((B, max(1, self._nswd)), dtype=torch.int32, device=self.device)
        return out, err

    def run(self, H, VP=None, VS=None, RHO=None, nlay=None, out=None, err=None, stream=None, rf_sets=None):
        """Launch all targets for the batch (asynchronous).  Either `run(models)` with resident
        DeviceModels (from `upload` / models.layers_from_voronoi) or `run(H, VP, VS, RHO, nlay)`
        with host or device arrays, which are packed first.  Returns (out[B,row], err[B,nswd]).

        rf_sets = (set_p, set_id): every row's receiver functions at the ray parameter of the row's set (station)
        instead of the engine's -- set_p [nrf][nsets] fp64 and set_id [B] int32, device tensors
        (bh_forward_batch_sets; a row is bit for bit what an engine with that p computes)."""
        models = H if isinstance(H, DeviceModels) else self.upload(H, VP, VS, RHO, nlay)
        if models.packed.device != self.device:
            raise ValueError("models live on %s, engine on %s" % (models.packed.device, self.device))
        if models.order is None and self.sort_ragged and self._nswd and models.B > ORDER_MIN:
            # resident models that came without a processing order (e.g. models.layers_from_voronoi):
            # computed once and kept with them
            models.order = self.reorder(models.packed, models.nlay).order
        H, VP, VS, RHO, nlay = models.H, models.VP, models.VS, models.RHO, models.nlay
        B, mstride, Lmax = models.B, 4 * models.Lmax, models.Lmax
        if models.depth is not None:                 # even, so that rows can be fetched two layers at a time
            Lmax = min(models.Lmax, models.depth + (models.depth % 2))
        st = torch.cuda.current_stream(self.device) if stream is None else stream
        sp = C.c_void_p(st.cuda_stream)
        if out is None or err is None:
            # allocated on the launch stream (the caching allocator recycles a block for the stream
            # it was allocated on); a buffer the caller passed is kept, only the missing one is made
            with torch.cuda.stream(st):
                new_out, new_err = self.alloc_out(B)
            out = new_out if out is None else out
            err = new_err if err is None else err
        with torch.cuda.device(self.device):
            # The two kernels are independent.  swd_kernel ends with a tail in which its persistent
            # waves retire one by one; launched on a second stream, rf_kernel's workgroups take over
            # the freed SIMDs instead of waiting for the last search to finish.
            side = None
            if self._nswd and self.rf and self.overlap:
                side = self._side.get(st.cuda_stream)
                if side is None:
                    side = self._side[st.cuda_stream] = torch.cuda.Stream(device=self.device)
                side.wait_stream(st)
            need, ws_ptr = self.lib.bh_swd_workspace_bytes(B, self._nswd, self._tg), None
            if need:
                ws = self._ws.get(st.cuda_stream)
                if ws is None or ws.numel() * 8 < need:
                    with torch.cuda.stream(st):          # the old block returns to this stream's pool
                        ws = self._ws[st.cuda_stream] = torch.empty((need + 7) // 8, dtype=torch.float64,
                                                                    device=self.device)
                ws_ptr = ws.data_ptr()
            # row, descriptors and overlap are read at every call: a caller may move a target's columns (bench.py)
            args = (B, Lmax, mstride, nlay.data_ptr(), H.data_ptr(), VP.data_ptr(), VS.data_ptr(), RHO.data_ptr(),
                    self._nswd, self._tg, self.periods.data_ptr(), len(self._obsx), self._interp, len(self.rf),
                    self._rfp, models.order.data_ptr() if models.order is not None else None, models.mean_depth or 0.0, 1,
                    out.data_ptr(), self.row, err.data_ptr(), ws_ptr, need, sp,
                    sp if side is None else C.c_void_p(side.cuda_stream))
            if rf_sets is None:
                _lib.check(self.lib.bh_forward_batch(*args))
            else:
                set_p, set_id = rf_sets
                if not self.rf or set_p.dim() != 2 or set_p.shape[0] != len(self.rf) or set_p.dtype != torch.float64 \
                        or not set_p.is_contiguous() or set_p.device != self.device:
                    raise ValueError("rf_sets: set_p [nrf][nsets] float64, contiguous, on the engine's device")
                if set_id.shape != (B,) or set_id.dtype != torch.int32 or not set_id.is_contiguous() \
                        or set_id.device != self.device:
                    raise ValueError("rf_sets: set_id [B] int32, contiguous, on the engine's device")
                _lib.check(self.lib.bh_forward_batch_sets(*(args + (set_p.shape[1], set_p.data_ptr(), set_id.data_ptr()))))
            # the ellipticities, behind the dispersion launch on its stream (beside the receiver functions on theirs)
            for e, (t, per_off, c_off), off in zip(self.ell, self.layout.ell_src, self.layout.ell_off):
                args = (B, Lmax, mstride, nlay.data_ptr(), H.data_ptr(), VP.data_ptr(), VS.data_ptr(), RHO.data_ptr(),
                        e.periods.size, self.periods.data_ptr() + 8 * per_off, e.flsph, out.data_ptr() + 8 * c_off, self.row,
                        err.data_ptr() + 4 * t, max(1, self._nswd), 1 if e.absolute else 0, out.data_ptr() + 8 * off, self.row)
                if self.ell_flags:
                    _lib.check(self.lib.bh_ell_batch_rows(
                        *(args + (models.order.data_ptr() if models.order is not None else None, 1, sp))))
                else:
                    _lib.check(self.lib.bh_ell_batch(*(args + (sp,))))
            if side is not None:
                st.wait_stream(side)
                for t in (H, VP, VS, RHO, nlay, out) + (() if rf_sets is None else tuple(rf_sets)):
                    t.record_stream(side)
        return out, err

    # -- the sensitivity passes (csrc/sens_pass.h)
    def _sens_swd_target(self, target, igr=False):
        """Dispersion target `target`, checked for what the phase and group passes serve (igr: a group-velocity target
        is served too)."""
        if not 0 <= target < len(self.layout.swd_all):
            raise ValueError("target %r: the engine solves %d dispersion targets" % (target, len(self.layout.swd_all)))
        spec = self.layout.swd_all[target]
        if spec.igr != 0 and not igr:
            raise ValueError("sensitivity: target '%s' has igr = %d; group-velocity targets are not served" % (spec.ref, spec.igr))
        if spec.mode != 1:
            raise ValueError("sensitivity: target '%s' has mode = %d; only the fundamental mode is served" % (spec.ref, spec.mode))
        if spec.flsph != 0:
            raise ValueError("sensitivity: target '%s' has flsph = %d; only a flat earth is served" % (spec.ref, spec.flsph))
        if spec.resample:
            raise ValueError("sensitivity: target '%s' has more than %d periods" % (spec.ref, _lib.MAX_PERIODS))
        return spec

    def _sens_buffers(self, src, models, out, err, nper, workspace_bytes, stream, nK, nrow):
        """What a pass reads and writes: (out, err) as given, or of `src`.run(models); the launch stream; nK tensors
        [B, nper, 4, Lmax], nrow tensors [B, nper] and the workspace (workspace_bytes: the pass's bh_*_workspace_bytes),
        allocated on that stream."""
        if out is None or err is None:
            out, err = src.run(models, stream=stream)
        st = torch.cuda.current_stream(self.device) if stream is None else stream
        B, Lmax = models.B, models.Lmax
        need = workspace_bytes(B, nper)
        with torch.cuda.stream(st):
            Ks = [torch.empty((B, nper, 4, Lmax), dtype=torch.float64, device=self.device) for _ in range(nK)]
            rows = [torch.empty((B, nper), dtype=torch.float64, device=self.device) for _ in range(nrow)]
            ws = torch.empty(max(1, (need + 7) // 8), dtype=torch.float64, device=self.device)
        return out, err, st, Ks, rows, ws

    @staticmethod
    def _sens_models(models):
        """The leading arguments of a pass's batch entry point: B, Lmax, model_stride, nlay, h, vp, vs, rho."""
        return (models.B, models.Lmax, 4 * models.Lmax, models.nlay.data_ptr(), models.H.data_ptr(), models.VP.data_ptr(),
                models.VS.data_ptr(), models.RHO.data_ptr())

    def sensitivity(self, H, VP=None, VS=None, RHO=None, nlay=None, out=None, err=None, target=0, stream=None):
        """Depth sensitivity kernels of dispersion target `target` for the batch (bh_sens_batch, asynchronous): the
        polished phase velocity c [B, nper], dc/dT [B, nper] and K [B, nper, 4, Lmax] = dc/dh, dc/dvp, dc/dvs, dc/drho
        per layer, device tensors in a dict.  `out`, `err`: what run() returned for these models -- the pass reads the
        engine's own phase velocities -- or None: run() is called first.  Fundamental-mode phase targets on a flat earth
        with at most 60 periods only; a (model, period) without a value is NaN (include/bayhunter_amd.h)."""
        models = H if isinstance(H, DeviceModels) else self.upload(H, VP, VS, RHO, nlay)
        spec = self._sens_swd_target(target)
        nper, tg = spec.periods.size, self._tg[target]
        out, err, st, (K,), (c, dc_dT), ws = self._sens_buffers(self, models, out, err, nper,
                                                                 self.lib.bh_sens_workspace_bytes, stream, 1, 2)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.bh_sens_batch(
                *self._sens_models(models), spec.iwave, nper, self.periods.data_ptr() + 8 * tg.per_off, 0,
                out.data_ptr() + 8 * tg.out_off, self.row, err.data_ptr() + 4 * target, max(1, self._nswd), K.data_ptr(),
                c.data_ptr(), dc_dT.data_ptr(), ws.data_ptr(), ws.numel() * 8, C.c_void_p(st.cuda_stream)))
        return {'c': c, 'dc_dT': dc_dT, 'K': K}

    def group_sensitivity(self, H, VP=None, VS=None, RHO=None, nlay=None, out=None, err=None, target=0, stream=None):
        """Depth sensitivity kernels of the GROUP velocity at the periods of dispersion target `target` for the batch
        (bh_sens_group_batch, asynchronous): U [B, nper] (the analytic group velocity of the polished root, not what a
        group target's columns hold), dU_dT, c [B, nper], K [B, nper, 4, Lmax] = dU/dh, dU/dvp, dU/dvs, dU/drho per layer
        and K_phase, what sensitivity() returns as K -- device tensors in a dict.  The pass reads phase velocities: a
        phase target's own columns; for a group target the columns of an equal phase target of this engine (the same
        wave type and periods) if there is one, else of a companion engine with that one target, kept with this engine
        and run on the same DeviceModels.  `out`, `err`: what run() returned for these models, or None: run() is called
        first.  Fundamental mode, flat earth, at most 60 periods; a (model, period) without a value is NaN."""
        models = H if isinstance(H, DeviceModels) else self.upload(H, VP, VS, RHO, nlay)
        spec = self._sens_swd_target(target, igr=True)
        src, source = self, target
        if spec.igr != 0:
            equal = [t for t, sp in enumerate(self.layout.swd_all)
                     if sp.igr == 0 and sp.iwave == spec.iwave and sp.mode == 1 and sp.flsph == 0 and not sp.resample
                     and np.array_equal(sp.periods, spec.periods)]
            if equal:
                source = equal[0]
            else:
                if not hasattr(self, '_phase_companions'):
                    self._phase_companions = {}
                src = self._phase_companions.get(target)
                if src is None:
                    src = self._phase_companions[target] = ForwardEngine(
                        swd=[SwdSpec('rdispph' if spec.iwave == 2 else 'ldispph', spec.periods)], device=self.device)
                source, out, err = 0, None, None
        nper, tg = spec.periods.size, src._tg[source]
        out, err, st, (K, Kp), (U, dU_dT, c), ws = self._sens_buffers(src, models, out, err, nper,
                                                                      self.lib.bh_sens_group_workspace_bytes, stream, 2, 3)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.bh_sens_group_batch(
                *self._sens_models(models), spec.iwave, nper, src.periods.data_ptr() + 8 * tg.per_off, 0,
                out.data_ptr() + 8 * tg.out_off, src.row, err.data_ptr() + 4 * source, max(1, src._nswd), K.data_ptr(),
                U.data_ptr(), dU_dT.data_ptr(), c.data_ptr(), Kp.data_ptr(), ws.data_ptr(), ws.numel() * 8,
                C.c_void_p(st.cuda_stream)))
        return {'K': K, 'U': U, 'dU_dT': dU_dT, 'c': c, 'K_phase': Kp}

    def ell_sensitivity(self, H, VP=None, VS=None, RHO=None, nlay=None, out=None, err=None, target=0, absolute=None,
                        stream=None):
        """Depth sensitivity kernels of ELLIPTICITY target `target` (an index into the engine's ellipticity targets) for the
        batch (bh_ell_sens_batch, asynchronous): E [B, nper] (H/V at the polished double-precision root -- not the
        target's columns, which hold H/V at the stored real*4 phase velocity), dE_dT, c [B, nper], K [B, nper, 4, Lmax] =
        dE/dh, dE/dvp, dE/dvs, dE/drho per layer (change of H/V per km, per km/s, per g/cm^3) and K_phase, what
        sensitivity() returns as K for the Rayleigh phase velocity -- device tensors in a dict.  The pass reads the phase
        velocities bh_ell_batch is given for that target: the columns of an equal 'rdispph' target, or of the hidden one.
        absolute: None for the target's; True: E, dE_dT and K are those of |H/V|.  `out`, `err`: what run() returned for
        these models, or None: run() is called first.  Flat earth only; a (model, period) without a value is NaN."""
        models = H if isinstance(H, DeviceModels) else self.upload(H, VP, VS, RHO, nlay)
        if not 0 <= target < len(self.ell):
            raise ValueError("target %r: the engine has %d ellipticity targets" % (target, len(self.ell)))
        e = self.ell[target]
        if e.flsph != 0:
            raise ValueError("sensitivity: target '%s' has flsph = %d; only a flat earth is served" % (e.ref, e.flsph))
        t, per_off, c_off = self.layout.ell_src[target]
        nper = e.periods.size
        absolute = e.absolute if absolute is None else bool(absolute)
        out, err, st, (K, Kp), (E, dE_dT, c), ws = self._sens_buffers(self, models, out, err, nper,
                                                                      self.lib.bh_ell_sens_workspace_bytes, stream, 2, 3)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.bh_ell_sens_batch(
                *self._sens_models(models), nper, self.periods.data_ptr() + 8 * per_off, 0, 1 if absolute else 0,
                out.data_ptr() + 8 * c_off, self.row, err.data_ptr() + 4 * t, max(1, self._nswd), K.data_ptr(), E.data_ptr(),
                dE_dT.data_ptr(), c.data_ptr(), Kp.data_ptr(), ws.data_ptr(), ws.numel() * 8, C.c_void_p(st.cuda_stream)))
        return {'K': K, 'E': E, 'dE_dT': dE_dT, 'c': c, 'K_phase': Kp}

    def rf_sensitivity(self, H, VP=None, VS=None, RHO=None, nlay=None, target=0, stream=None, p=None):
        """Sensitivity kernels of RECEIVER-FUNCTION target `target` (an index into the engine's receiver-function targets)
        for the batch (bh_rf_sens_batch, asynchronous): K [B, nt, 4, Lmax] = dRF(t)/dh, dRF/dvp, dRF/dvs, dRF/drho per
        layer and sample of the target's time axis, and rf [B, nt], the trace itself, bit for bit what run() writes into
        the target's columns -- device tensors in a dict, with 't' [nt], the time axis (numpy).  The time samples sit
        where the dispersion kernels have periods.  The engine's slowness for every row (run()'s rf_sets are not served);
        K is 0 for the half-space's thickness and NaN in the layers a model does not have (include/bayhunter_amd.h).
        p: a ray parameter [s/deg] for this call in place of the target's (a copy of its bh_rf_params goes to the
        library; the engine keeps its own)."""
        models = H if isinstance(H, DeviceModels) else self.upload(H, VP, VS, RHO, nlay)
        if not 0 <= target < len(self.rf):
            raise ValueError("target %r: the engine has %d receiver-function targets" % (target, len(self.rf)))
        if models.packed.device != self.device:
            raise ValueError("models live on %s, engine on %s" % (models.packed.device, self.device))
        spec, par = self.rf[target], self._rfp[target]
        if p is not None:
            par = _lib.RfParams.from_buffer_copy(par)
            par.p = float(p)
        st = torch.cuda.current_stream(self.device) if stream is None else stream
        B, Lmax, nt = models.B, models.Lmax, spec.obsx.size
        with torch.cuda.stream(st):
            K = torch.empty((B, nt, 4, Lmax), dtype=torch.float64, device=self.device)
            rf = torch.empty((B, nt), dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.bh_rf_sens_batch(*self._sens_models(models), None, None, C.byref(par), K.data_ptr(),
                                                 nt * 4 * Lmax, rf.data_ptr(), nt, None, 0, C.c_void_p(st.cuda_stream)))
        return {'K': K, 'rf': rf, 't': (np.arange(int(spec.nsamp)) / spec.fsamp - spec.tshft)[:nt]}
