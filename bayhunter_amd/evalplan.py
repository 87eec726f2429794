"""Evaluation plan: a batch of proposals -> (logL, misfits) in ONE call into libbayhunter_amd.

The hand-over between the sampler and the device (reference: one `JointTarget.evaluate` per chain and
iteration, src/SingleChain.py:545-552 -> src/Targets.py:314-347).  `bh_eval_submit` copies the pinned
staging block the proposals were written into, orders the batch, launches the dispersion, receiver-function
and likelihood kernels on the plan's own streams and copies 8*(ntargets+2) bytes per model back; the
plan owns every buffer (include/bayhunter_amd.h, "evaluation plan").  Nothing here imports torch.
"""
import ctypes as C

import numpy as np

from . import _lib


def _view(ptr, ctype, count):
    return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ctype)), shape=(count,))


class EvalPlan(object):
    """`layout` = JointTarget.batch_layout(ell=True).  A layout with ellipticity targets gives the plan its hidden
    dispersion sources and the targets themselves (bh_eval_set_ellipticity): a model without an ellipticity is then
    refused by the likelihood like a model whose search failed.  Host views of the plan's pinned staging block:
    packed[rows, 4, Lmax], nlay[rows], noise[rows, 2*ntargets], chain[rows]; `submit(count)` evaluates
    the first `count` rows, `wait()` returns (logL[count], misfits[count, ntargets+1]) -- views that stay
    valid until the next submit.

    A plan owns device memory, pinned host memory, two streams and events: `close()` it (or use it as a
    context manager) when the sampler is done with it.  `__del__` only backs that up -- when the interpreter
    collects an object is not something to hang device resources on."""

    def __init__(self, layout, max_models, Lmax, use_mfma=True):
        self.lib = _lib.load()
        lay, desc = layout['layout'], layout['desc']
        self.rows, self.Lmax, self.T, self.row = int(max_models), int(Lmax), len(desc), int(lay.row)
        self.nrf = len(lay.rf)
        # a layout whose targets have data gaps must not run before the plan has them (set_gaps)
        self._gaps_due = 'present' in layout and not np.asarray(layout['present']).all()
        interp = lay.interp([sp.obsx.ctypes.data for _, _, _, sp in lay.resampled])   # (copied by bh_eval_create)
        self.handle = C.c_void_p()
        _lib.check(self.lib.bh_eval_create(
            self.rows, self.Lmax, lay.row, len(lay.swd_all), lay.tg, lay.periods.ctypes.data, lay.periods.size,
            len(lay.rf), lay.rfp, self.T, desc, layout['nflags'], layout['yobs'].ctypes.data, layout['aux'].ctypes.data,
            layout['aux'].size, len(lay.resampled), interp, 1 if use_mfma else 0, C.byref(self.handle)))
        if lay.ell:                                  # the hidden sources are among swd_all: lay.tg describes them
            ell = (_lib.EllTarget * len(lay.ell))(*[
                _lib.EllTarget(t, e.periods.size, off, 1 if e.absolute else 0)
                for e, (t, _, _), off in zip(lay.ell, lay.ell_src, lay.ell_off)])
            try:
                _lib.check(self.lib.bh_eval_set_ellipticity(self.handle, len(lay.ell), ell))
            except Exception:
                self.lib.bh_eval_destroy(self.handle)
                self.handle = None
                raise
        p = [C.c_void_p() for _ in range(5)]
        _lib.check(self.lib.bh_eval_buffers(self.handle, *[C.byref(x) for x in p]))
        R, L, T = self.rows, self.Lmax, self.T
        self.packed = _view(p[0], C.c_double, R * 4 * L).reshape(R, 4, L)
        self.nlay = _view(p[1], C.c_int32, R)
        self.noise = _view(p[2], C.c_double, R * 2 * T).reshape(R, 2 * T)
        self.chain = _view(p[3], C.c_int32, R)
        self._results = _view(p[4], C.c_double, R * (T + 2))

    def _live(self):
        if not self.handle:
            raise _lib.BayHunterAmdError("this evaluation plan has been closed")
        return self.handle

    def submit(self, count):
        if self._gaps_due:
            raise _lib.BayHunterAmdError("the plan's targets have data gaps: give it every set's observations and the table "
                                         "of present samples first (set_observations, set_gaps)")
        _lib.check(self.lib.bh_eval_submit(self._live(), int(count)))

    def set_observations(self, yobs, set_of_chain, set_scale=None, set_logdet=None):
        """The chains behind this plan belong to yobs.shape[0] observation sets (bh_eval_set_observations):
        yobs[nsets, row], set_scale[nsets, row], set_logdet[nsets, ntargets] (both or neither), set_of_chain[nchains]
        for the chain numbers the sampler writes to `chain`.  Once, before the first submit."""
        yobs = np.ascontiguousarray(yobs, dtype=np.float64)
        soc = np.ascontiguousarray(set_of_chain, dtype=np.int32)
        if yobs.ndim != 2 or yobs.shape[1] != self.row:
            raise ValueError("yobs: one row of %d values per observation set" % self.row)
        tabs = []
        for tab, width in ((set_scale, self.row), (set_logdet, self.T)):
            if tab is not None:
                tab = np.ascontiguousarray(tab, dtype=np.float64)
                if tab.shape != (yobs.shape[0], width):
                    raise ValueError("per-set table of shape %s, expected %s" % (tab.shape, (yobs.shape[0], width)))
            tabs.append(tab)
        _lib.check(self.lib.bh_eval_set_observations(
            self._live(), yobs.shape[0], yobs.ctypes.data, *[None if t is None else t.ctypes.data for t in tabs],
            soc.ctypes.data, soc.size))

    def set_rf_slowness(self, p):
        """Per-set ray parameters of the receiver-function targets (bh_eval_set_rf_slowness): p[nsets, nrf] in s/deg,
        nsets that of `set_observations`, which comes first; the targets in the order of the layout's `rf`.  Once,
        before the first submit.  Every row is then computed at the slowness of its chain's set."""
        p = np.ascontiguousarray(p, dtype=np.float64)
        if p.ndim != 2 or p.shape[1] != self.nrf:
            raise ValueError("p: one row of %d ray parameters (one per receiver-function target) per observation set" % self.nrf)
        _lib.check(self.lib.bh_eval_set_rf_slowness(self._live(), p.shape[0], p.ctypes.data))

    def set_gaps(self, present):
        """Data gaps of the observation sets (bh_eval_set_gaps): present[nsets, row], nonzero where a set has the
        sample, nsets that of `set_observations`, which comes first (with set_scale / set_logdet computed over the kept
        samples and a finite placeholder in yobs at a gap).  Once, before the first submit.  The likelihood of a row
        then leaves out the samples its set lacks, as if those lines had been deleted from the station's data file;
        a dense-Gaussian target with a gap and a target without a kept sample are refused."""
        present = np.ascontiguousarray(np.asarray(present) != 0, dtype=np.uint8)
        if present.ndim != 2 or present.shape[1] != self.row:
            raise ValueError("present: one row of %d bytes per observation set" % self.row)
        _lib.check(self.lib.bh_eval_set_gaps(self._live(), present.shape[0], present.ctypes.data))
        self._gaps_due = False

    def set_concurrency(self, plans_in_flight):
        """How many plans take turns on the device (the chain groups of a pool): the library chooses its kernel
        forms for that load."""
        _lib.check(self.lib.bh_eval_set_concurrency(self._live(), int(plans_in_flight)))

    def wait(self):
        self._live()
        n = C.c_int(0)
        _lib.check(self.lib.bh_eval_wait(self.handle, C.byref(n)))
        n, T = n.value, self.T
        return self._results[:n], self._results[n:n * (T + 2)].reshape(n, T + 1)

    def close(self):
        """Wait for the plan's streams, then free everything it owns (idempotent).  The host views
        (packed, nlay, noise, chain, results) point into freed pinned memory afterwards and are dropped."""
        h, self.handle = getattr(self, 'handle', None), None
        if h:
            self.packed = self.nlay = self.noise = self.chain = self._results = None
            self.lib.bh_eval_destroy(h)

    @property
    def closed(self):
        return not self.handle

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
