"""Observation sets in the C ABI (bh_likelihood_sets, bh_eval_set_observations): every argument is checked before
the first device call, so these run on a machine without a GPU (fake device pointers: nothing is launched)."""
import ctypes as C

import numpy as np


def test_likelihood_sets_validates_arguments_without_gpu(lib):
    from bayhunter_amd import _lib
    desc = (_lib.LikeTarget * 2)(_lib.LikeTarget(21, 0, _lib.COV_NOCORR_SCALED, 0, 0.0),
                                 _lib.LikeTarget(201, 21, _lib.COV_EXP, 0, 0.0))

    def call(stages=3, B=4, nsets=3, obs_id=1, yobs=1, stride=222, scale=1, logdet=1, aux=1, targets=desc):
        return lib.bh_likelihood_sets(stages, B, 2, targets, 1, 222, None, 0, nsets, obs_id, yobs, stride, scale, logdet,
                                      1, aux, 1, 1, None, 0, None)
    assert call(B=0) == _lib.BH_OK                                                   # nothing to do
    assert call(nsets=0) == _lib.BH_ERR_ARG and b'nsets' in lib.bh_last_error()
    assert call(nsets=-2, B=0) == _lib.BH_ERR_ARG and b'nsets' in lib.bh_last_error()
    assert call(obs_id=None) == _lib.BH_ERR_ARG and b'obs_id' in lib.bh_last_error()
    assert call(yobs=None) == _lib.BH_ERR_ARG and b'NULL' in lib.bh_last_error()
    assert call(scale=None) == _lib.BH_ERR_ARG and b'come together' in lib.bh_last_error()
    assert call(logdet=None) == _lib.BH_ERR_ARG and b'come together' in lib.bh_last_error()
    assert call(scale=None, logdet=None) == _lib.BH_ERR_ARG and b'BH_COV_NOCORR_SCALED' in lib.bh_last_error()
    assert call(stride=221) == _lib.BH_ERR_ARG and b'set_stride' in lib.bh_last_error()
    assert call(stages=4) == _lib.BH_ERR_ARG and b'stages' in lib.bh_last_error()
    # one set without tables: the scaled errors come from aux, as in bh_likelihood_stage -- which needs aux
    assert call(nsets=1, obs_id=None, scale=None, logdet=None, aux=None) == _lib.BH_ERR_ARG and b'aux' in lib.bh_last_error()
    bad = (_lib.LikeTarget * 2)(_lib.LikeTarget(21, 0, 7, 0, 0.0), _lib.LikeTarget(201, 21, _lib.COV_EXP, 0, 0.0))
    assert call(targets=bad) == _lib.BH_ERR_ARG and b'covariance' in lib.bh_last_error()


def test_eval_set_observations_validates_arguments_without_gpu(lib):
    from bayhunter_amd import _lib
    y = np.zeros((3, 222))
    soc = np.array([0, 0, 1, 1, 2, 2], dtype=np.int32)

    def call(plan=None, nsets=3, yobs=y.ctypes.data, scale=None, logdet=None, chains=soc, nchains=None):
        return lib.bh_eval_set_observations(plan, nsets, yobs, scale, logdet, None if chains is None else chains.ctypes.data,
                                            (0 if chains is None else chains.size) if nchains is None else nchains)
    assert call(nsets=0) == _lib.BH_ERR_ARG and b'nsets' in lib.bh_last_error()
    assert call(yobs=None) == _lib.BH_ERR_ARG and b'NULL' in lib.bh_last_error()
    assert call(chains=None, nchains=6) == _lib.BH_ERR_ARG and b'NULL' in lib.bh_last_error()
    assert call(nchains=0) == _lib.BH_ERR_ARG and b'nchains' in lib.bh_last_error()
    assert call(scale=y.ctypes.data) == _lib.BH_ERR_ARG and b'come together' in lib.bh_last_error()
    for bad in (3, -1):
        wrong = soc.copy()
        wrong[4] = bad
        assert call(chains=wrong) == _lib.BH_ERR_ARG
        assert b'set_of_chain[4] = %d' % bad in lib.bh_last_error()
    assert call() == _lib.BH_ERR_ARG and b'plan is NULL' in lib.bh_last_error()      # everything else was in order
    assert call(plan=C.c_void_p(0)) == _lib.BH_ERR_ARG
