"""The ellipticity in the evaluation plan: bh_eval_set_ellipticity, the plan's ell_rows_kernel stage and the flag the
likelihood reads.

* (logL, misfits) of a plan equal JointTarget.evaluate_batch on the same rows, bit for bit -- both run the same kernels --
  for the three row layouts (shared source, hidden source, three targets in another order than the row's; once more
  with the dense Gaussian covariance, whose product runs on the side stream beside the ellipticity stage) at 1, 65 and
  1 030 ragged models of 2-10 layers, the last one in the plan's processing order; free noise columns.
* Eight rows of each layout equal the host's JointTarget.evaluate within the tolerance of
  test_gpu_ellipticity.py::test_joint_target_values_the_ellipticity_with_the_host_likelihood (1e-9 of |logL|, 1e-12 for
  a misfit).
* A water-topped model and a half-space alone are refused (logL -1e15, misfits 1e15) by both paths, their neighbours'
  values do not move.
* bh_eval_set_ellipticity refuses each bad field, sources that are not the fundamental Rayleigh mode's phase
  velocities, a second call and a call after the first submit.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PER = np.linspace(1., 41., 21)
TIME = np.linspace(-5., 35., 201)
LMAX = 10


def _joint(kind):
    from bayhunter_amd import targets as T
    rng = np.random.RandomState(3)
    disp = T.RayleighDispersionPhase(PER, 2.9 + 0.025 * PER + rng.normal(0, 0.02, 21))
    ell = T.RayleighEllipticity(PER, 0.75 + 0.1 * np.sin(PER / 7.) + rng.normal(0, 0.02, 21), yerr=np.full(21, 0.02))
    rf = T.PReceiverFunction(TIME, 0.3 * np.exp(-TIME ** 2) + rng.normal(0, 0.01, 201))
    if kind == 'shared':
        joint = T.JointTarget([disp, ell])
        joint.set_target_covariance([True, False], [0.0, 0.3], None)          # diagonal, exponential
    elif kind == 'hidden':
        joint = T.JointTarget([ell])
        joint.set_target_covariance([True], [0.0], None)                      # diagonal scaled by yerr
    else:
        joint = T.JointTarget([ell, rf, disp])                                # row: dispersion, receiver function, H/V
        gauss = kind == 'three_gauss'
        joint.set_target_covariance([False, gauss, True], [0.3, 0.9 if gauss else 0.5, 0.0], 1e-5 if gauss else None)
    return joint


def _random_batch(B, T, seed):
    from bayhunter_amd.synthetic import draw_models
    H, VP, VS, RHO, nl = draw_models(B, (2, LMAX), seed=seed, sorted_vs=False, Lmax=LMAX)
    rs = np.random.RandomState(seed + 1)
    noise = np.column_stack([f(B) for _ in range(T) for f in (lambda n: rs.uniform(0.0, 0.9, n), lambda n: rs.uniform(0.005, 0.05, n))])
    return np.stack([H, VP, VS, RHO], axis=1), nl, np.ascontiguousarray(noise)


def _both(joint, packed, nl, noise):
    """(logL, misfits) from a plan and from the engine path."""
    import torch
    B = nl.size
    with joint.eval_plan(B + 3, LMAX) as plan:
        plan.packed[:B], plan.nlay[:B], plan.noise[:B] = packed, nl, noise
        plan.submit(B)
        logL, mis = (a.copy() for a in plan.wait())
    wl, wm = joint.evaluate_batch(packed[:, 0], packed[:, 1], packed[:, 2], nl, noise, RHO=packed[:, 3])
    torch.cuda.synchronize()
    return logL, mis, wl.cpu().numpy(), wm.cpu().numpy()


@pytest.mark.parametrize('count', [1, 65, 1030])
@pytest.mark.parametrize('kind', ['shared', 'hidden', 'three', 'three_gauss'])
def test_plan_equals_the_engine_path(kind, count):
    joint = _joint(kind)
    T = joint.ntargets
    packed, nl, noise = _random_batch(count, T, seed=count)
    logL, mis, wl, wm = _both(joint, packed, nl, noise)
    assert logL.shape == (count,) and mis.shape == (count, T + 1)
    assert np.array_equal(logL, wl, equal_nan=True) and np.array_equal(mis, wm, equal_nan=True)
    ok = logL > -1e15
    assert np.isfinite(logL).all() and np.all(logL[~ok] == -1e15) and np.all(mis[~ok] == 1e15)
    assert count == 1 or ok.mean() > 0.8


@pytest.mark.parametrize('kind', ['shared', 'hidden', 'three'])
def test_eight_rows_equal_the_host_evaluation(kind):
    joint = _joint(kind)
    T = joint.ntargets
    packed, nl, noise = _random_batch(8, T, seed=21)
    logL, mis, _, _ = _both(joint, packed, nl, noise)
    valued = 0
    for b in range(8):
        n = int(nl[b])
        h, vp, vs, rho = (packed[b, i, :n] for i in range(4))
        joint.evaluate(h, vp, vs, noise[b], rho=rho)
        want, wmis = joint.proposallikelihood, np.asarray(joint.proposalmisfits, dtype=np.float64)
        print(kind, b, logL[b], want, np.abs(mis[b] - wmis).max())
        if want == -1e15:
            assert logL[b] == -1e15 and np.all(mis[b] == 1e15)
            continue
        valued += 1
        assert abs(logL[b] - want) <= 1e-9 * abs(want), (b, logL[b], want)
        assert np.all(np.abs(mis[b] - wmis) < 1e-12), (b, mis[b], wmis)
    assert valued >= 6


@pytest.mark.parametrize('kind', ['shared', 'hidden', 'three'])
def test_models_without_an_ellipticity_are_refused_and_their_neighbours_do_not_move(kind):
    import torch
    joint = _joint(kind)
    T = joint.ntargets
    packed, nl, noise = _random_batch(16, T, seed=5)
    clean = _both(joint, packed, nl, noise)
    packed, nl = packed.copy(), nl.copy()
    packed[3, :, 0] = (0.5, 1.5, 0.0, 1.03)                 # half a kilometre of water on top
    nl[9] = 1                                               # a half-space alone
    logL, mis, wl, wm = _both(joint, packed, nl, noise)
    bad = np.zeros(16, dtype=bool)
    bad[[3, 9]] = True
    for got_l, got_m in ((logL, mis), (wl, wm)):
        assert np.all(got_l[bad] == -1e15) and np.all(got_m[bad] == 1e15)
        assert np.array_equal(got_l[~bad], clean[0][~bad]) and np.array_equal(got_m[~bad], clean[1][~bad])
    assert (clean[0][~bad] > -1e15).sum() >= 10
    # it is the ellipticity that refuses the half-space: its search succeeds, the flag is BH_ELL_NO_VALUE (the search of
    # a model that has water where the sampler put rock may fail by itself: flag 1)
    eng = joint._batch['eng']
    src = eng.layout.ell_src[0][0]
    _, err = eng.run(packed[:, 0], packed[:, 1], packed[:, 2], packed[:, 3], nl)
    torch.cuda.synchronize()
    err = err.cpu().numpy()
    print(kind, 'flags of the refused rows:', err[[3, 9]].tolist())
    assert err[9, src] == 4 and err[3, src] in (1, 4)
    assert np.array_equal(err[~bad].any(axis=1), clean[0][~bad] == -1e15)      # a refused row is a flagged row


def test_set_ellipticity_refusals():
    from bayhunter_amd import _lib
    from bayhunter_amd import targets as T
    per15 = np.linspace(2., 30., 15)
    overtone = T.RayleighDispersionPhase(per15, np.full(15, 4.0))
    overtone.moddata.plugin.set_modelparams(mode=2)
    joint = T.JointTarget([T.RayleighDispersionPhase(PER, np.full(21, 3.5)), T.LoveDispersionPhase(PER, np.full(21, 3.6)),
                           T.RayleighDispersionGroup(PER, np.full(21, 3.2)), overtone])
    joint.set_target_covariance([True] * 4, [0.0] * 4, None)
    lib = _lib.load()

    def call(plan, *targets, nell=None):
        arr = (_lib.EllTarget * max(1, len(targets)))(*[_lib.EllTarget(*t) for t in targets])
        rc = lib.bh_eval_set_ellipticity(plan.handle, len(targets) if nell is None else nell, arr)
        return rc, lib.bh_last_error().decode()

    with joint.eval_plan(8, LMAX) as plan:
        assert plan.row == 78
        for target, word in (((-1, 21, 0, 1), 'src'), ((4, 21, 0, 1), 'src'),
                             ((1, 21, 0, 1), 'Rayleigh'), ((2, 21, 0, 1), 'Rayleigh'), ((3, 15, 0, 1), 'Rayleigh'),
                             ((0, 20, 0, 1), 'nper'), ((0, 0, 0, 1), 'nper'), ((0, 61, 0, 1), 'nper'),
                             ((0, 21, -1, 1), 'out_off'), ((0, 21, 58, 1), 'out_off')):
            rc, msg = call(plan, target)
            assert rc == _lib.BH_ERR_ARG and 'bh_eval_set_ellipticity' in msg and word in msg, (target, msg)
        rc, msg = call(plan, (0, 21, 21, 1), (4, 21, 21, 1))      # the second target is the bad one
        assert rc == _lib.BH_ERR_ARG and 'ell[1].src' in msg, msg
        for nell in (0, _lib.MAX_TARGETS + 1):
            rc, msg = call(plan, (0, 21, 21, 1), nell=nell)
            assert rc == _lib.BH_ERR_ARG and 'nell' in msg, msg
        assert lib.bh_eval_set_ellipticity(plan.handle, 1, None) == _lib.BH_ERR_ARG
        assert lib.bh_eval_set_ellipticity(None, 1, (_lib.EllTarget * 1)()) == _lib.BH_ERR_ARG
        assert call(plan, (0, 21, 57, 1))[0] == _lib.BH_OK        # nothing above has given the plan a target
        rc, msg = call(plan, (0, 21, 57, 1))
        assert rc == _lib.BH_ERR_ARG and 'already' in msg, msg
    with joint.eval_plan(8, LMAX) as plan:
        plan.submit(0)
        rc, msg = call(plan, (0, 21, 57, 1))
        assert rc == _lib.BH_ERR_ARG and 'after bh_eval_submit' in msg, msg
    # a plan made from a layout with the target has it already
    with _joint('shared').eval_plan(8, LMAX) as plan:
        rc, msg = call(plan, (0, 21, 21, 1))
        assert rc == _lib.BH_ERR_ARG and 'already' in msg, msg
