"""Targets of a joint inversion and the layout of one model's output row -- no torch, no device.

Shared by the batched engine (engine.ForwardEngine: torch tensors and streams) and by the evaluation plan
of the chain pool (evalplan.EvalPlan: everything inside libbayhunter_amd).
"""
import numpy as np

from . import _lib

# Batches above this many models get a processing order (deepest first, ...: engine.reorder).  It is not only
# the lane kernel that needs it: the team kernels take one search per workgroup in launch order, a thousand or
# two are resident at a time, and a deep model started late is a tail of its own -- 8 192 ragged 2-31-layer
# models 14.3 -> 9.8 ms, 2 048 models of 2-21 layers 2.9 -> 1.9 ms with the order (profiles/r03_order_small.txt).
# Up to 1 024 searches every team is resident at once and the order is irrelevant.
ORDER_MIN = 1024

SWD_REFS = {'rdispgr': (2, 1), 'ldispgr': (1, 1), 'rdispph': (2, 0), 'ldispph': (1, 0)}
RF_REFS = {'prf': 0, 'seis': 0, 'srf': 1}
ELL_REFS = ('rellip',)


def rf_obsparams(obsx, ref='prf'):
    """fsamp, tshft, nsamp from the observed time axis (src/rfmini_modrf.py:41-62)."""
    obsx = np.asarray(obsx, dtype=np.float64)
    steps = np.unique(np.round(np.diff(obsx), 4))
    if steps.size != 1:
        raise ValueError("receiver-function target '%s': the time axis must be uniformly sampled" % ref)
    fsamp = 1. / float(steps[0])
    nsamp = 2.**int(np.ceil(np.log2(obsx.size * 2)))       # a float, like the reference's
    return fsamp, float(-obsx[0]), nsamp


class SwdSpec(object):
    def __init__(self, ref, periods, mode=1, flsph=0):
        if ref not in SWD_REFS:
            raise ReferenceError("no dispersion forward model for ref '%s'" % ref)
        self.ref = ref
        self.iwave, self.igr = SWD_REFS[ref]
        self.obsx = np.ascontiguousarray(periods, dtype=np.float64)
        # more than NP = 60 periods (surfdisp96.f:62): solve on 60 evenly spaced periods over the same
        # span and interpolate linearly to the observed ones, like SurfDisp (surf96_modsw.py:35-43,
        # 106-122); the library interpolates on the device (bh_forward_batch)
        self.resample = self.obsx.size > _lib.MAX_PERIODS
        self.periods = np.linspace(self.obsx.min(), self.obsx.max(), _lib.MAX_PERIODS) if self.resample \
            else self.obsx
        self.mode, self.flsph = int(mode), int(flsph)


class RfSpec(object):
    def __init__(self, ref, obsx, gauss=1.0, p=6.4, nsv=None, wtype=None):
        if wtype is None:
            if ref not in RF_REFS:
                raise ReferenceError("no receiver-function forward model for ref '%s'" % ref)
            self.waveno = RF_REFS[ref]
        else:
            self.waveno = {'P': 0, 'SV': 1}[wtype]
        self.ref = ref
        self.obsx = np.ascontiguousarray(obsx, dtype=np.float64)
        self.fsamp, self.tshft, self.nsamp = rf_obsparams(self.obsx, ref)
        self.gauss, self.p, self.nsv = float(gauss), float(p), nsv


class EllSpec(object):
    """Ellipticity (H/V) of the fundamental Rayleigh mode at `periods` (at most 60: a ratio that changes sign is not
    interpolated).  absolute: |H/V|, what most data are; else the signed ratio, positive for retrograde motion."""

    def __init__(self, ref, periods, flsph=0, absolute=True):
        if ref not in ELL_REFS:
            raise ReferenceError("no ellipticity forward model for ref '%s'" % ref)
        self.ref = ref
        self.obsx = np.ascontiguousarray(periods, dtype=np.float64)
        if self.obsx.size < 1 or self.obsx.size > _lib.MAX_PERIODS:
            raise ValueError("ellipticity target '%s': 1 to %d periods, not %d" % (ref, _lib.MAX_PERIODS, self.obsx.size))
        self.periods = self.obsx
        self.flsph, self.absolute = int(flsph), bool(absolute)

    def reads(self, sp):
        """Does the dispersion target `sp` solve what this target needs: fundamental-mode Rayleigh phase velocities
        on the same earth at bit-equal periods?"""
        return (sp.ref == 'rdispph' and sp.mode == 1 and sp.flsph == self.flsph and not sp.resample
                and sp.periods.tobytes() == self.periods.tobytes())


class RowLayout(object):
    """Output row of model b: [swd target 0 | swd target 1 | ... | rf target 0 | ... | ellipticity target 0 | ...],
    fp64, `ncols` values; `slices[t]` is target t's column range.  Rows are `row` doubles apart: with a dispersion
    target of more than 60 periods `row` > `ncols` (the 60 solved values live behind the visible
    columns and are interpolated into them after the kernel).  `tg` / `rfp` are the descriptor arrays
    bh_forward_batch takes (at least one element each), `periods` the concatenated solved periods, `resampled` the
    (target index, visible slice, scratch offset, SwdSpec) of every target with more than 60 periods.

    An ellipticity target reads the phase velocities of a dispersion target (EllSpec.reads).  Where `swd` has none, the
    layout adds a hidden 'rdispph' target whose columns lie behind the visible ones, like the solved values of a
    resampled target: `swd_all` is `swd` followed by the hidden targets, `tg` describes all of them, and `ell_src[i]`
    is (index into swd_all, period offset, column offset) of ellipticity target i's source.  Without ellipticity
    targets nothing differs from a layout that does not know them."""

    def __init__(self, swd=(), rf=(), ell=()):
        self.swd, self.rf, self.ell = list(swd), list(rf), list(ell)
        self.swd_all = list(self.swd)
        src = []
        for e in self.ell:
            t = next((i for i, sp in enumerate(self.swd_all) if e.reads(sp)), None)
            if t is None:
                t = len(self.swd_all)
                self.swd_all.append(SwdSpec('rdispph', e.periods, 1, e.flsph))
            src.append(t)
        if len(self.swd_all) > _lib.MAX_TARGETS:
            raise ValueError("too many SWD targets")
        off = 0
        self.slices = []
        for sp in self.swd:
            self.slices.append(slice(off, off + sp.obsx.size))
            off += sp.obsx.size
        rf_off = []
        for r in self.rf:
            rf_off.append(off)
            self.slices.append(slice(off, off + r.obsx.size))
            off += r.obsx.size
        self.ell_off = []
        for e in self.ell:
            self.ell_off.append(off)
            self.slices.append(slice(off, off + e.obsx.size))
            off += e.obsx.size
        self.ncols = off
        per_off = 0
        self.tg = (_lib.SwdTarget * max(1, len(self.swd_all)))()
        pers = []
        self.resampled = []
        for t, sp in enumerate(self.swd_all):
            if t >= len(self.swd):                         # hidden: solved behind the visible columns, shown nowhere
                koff = off
                off += sp.periods.size
            else:
                koff = self.slices[t].start
            if sp.resample:                                # the kernel writes behind the visible columns
                koff = off
                off += sp.periods.size
                self.resampled.append((t, self.slices[t], koff, sp))
            self.tg[t] = _lib.SwdTarget(sp.iwave, sp.igr, sp.mode, sp.flsph, sp.periods.size, per_off, koff, 0)
            pers.append(sp.periods)
            per_off += sp.periods.size
        self.rfp = (_lib.RfParams * max(1, len(self.rf)))(*[
            _lib.RfParams(r.p, r.gauss, r.fsamp, r.tshft, -1.0 if r.nsv is None else float(r.nsv), int(r.nsamp),
                          r.waveno, r.obsx.size, o) for r, o in zip(self.rf, rf_off)])
        self.row = off
        self.periods = np.ascontiguousarray(np.concatenate(pers) if pers else np.zeros(1), dtype=np.float64)
        self.ell_src = [(t, self.tg[t].per_off, self.tg[t].out_off) for t in src]

    def interp(self, obsx):
        """The bh_eval_interp array of the targets in `resampled`, with their observed periods at addresses obsx[i]."""
        return (_lib.EvalInterp * max(1, len(self.resampled)))(
            *[_lib.EvalInterp(t, sl.start, sl.stop - sl.start, 0, a) for (t, sl, _, _), a in zip(self.resampled, obsx)])
