"""JointTarget.batch_layout(ell=True): the row layout, likelihood descriptors and observed data of joint targets with
an ellipticity (no device).  Three shapes: the ellipticity beside the dispersion target it reads (shared source), alone
(a hidden source behind the visible columns) and with a receiver function, the targets in another order in the
JointTarget than in the row.  Without the argument the method refuses the target as before."""
import numpy as np
import pytest

PER = np.linspace(1., 41., 21)
TIME = np.linspace(-5., 35., 201)


def _targets():
    from bayhunter_amd import targets
    rng = np.random.RandomState(5)
    disp = targets.RayleighDispersionPhase(PER, 3.0 + rng.rand(21))
    ell = targets.RayleighEllipticity(PER, 0.5 + rng.rand(21), yerr=0.01 + 0.02 * rng.rand(21))
    rf = targets.PReceiverFunction(TIME, rng.normal(0, 0.1, 201))
    return disp, rf, ell


def _check(joint, bl, want_slices, row, ncols, nswd_all, ell_src):
    lay, desc = bl['layout'], bl['desc']
    assert lay.row == row and lay.ncols == ncols and bl['nflags'] == max(1, nswd_all) == len(lay.swd_all)
    assert lay.ell_src == ell_src
    assert bl['yobs'].shape == (row,) and bl['present'].shape == (row,) and bl['present'].dtype == np.uint8
    assert bl['present'].all()
    covered = np.zeros(row, dtype=bool)
    for n, (t, sl) in enumerate(zip(joint.targets, want_slices)):
        assert (desc[n].off, desc[n].n) == (sl.start, sl.stop - sl.start), (n, desc[n].off, desc[n].n)
        assert desc[n].cov == t.covmodel
        assert np.array_equal(bl['yobs'][sl], t.obsdata.y)
        covered[sl] = True
    assert covered[:ncols].all() and not covered[ncols:].any()      # the likelihood sees the visible columns, all of them
    assert np.all(bl['yobs'][ncols:] == 0.0)


def test_shared_source():
    from bayhunter_amd import _lib, targets
    disp, _, ell = _targets()
    joint = targets.JointTarget([disp, ell])
    joint.set_target_covariance([True, True], [0.0, 0.0])         # ell has a usable yerr: the scaled diagonal model
    bl = joint.batch_layout(ell=True)
    _check(joint, bl, [slice(0, 21), slice(21, 42)], 42, 42, 1, [(0, 0, 0)])
    lay = bl['layout']
    assert len(lay.swd) == 1 and len(lay.ell) == 1 and lay.ell_off == [21]
    assert lay.ell[0].flsph == 0 and lay.ell[0].absolute is True
    d = bl['desc'][1]
    assert d.cov == _lib.COV_NOCORR_SCALED and d.aux_off == 0
    se = ell.obsdata.yerr / ell.obsdata.yerr.min()
    assert np.array_equal(bl['aux'][:21], se) and d.logdet_extra == float(np.log(np.prod(se)))


def test_hidden_source_and_plugin_parameters():
    from bayhunter_amd import targets
    _, _, ell = _targets()
    ell.moddata.plugin.set_modelparams(flsph=1, absolute=False)
    joint = targets.JointTarget([ell])
    bl = joint.batch_layout(ell=True)
    _check(joint, bl, [slice(0, 21)], 42, 21, 1, [(0, 0, 21)])
    lay = bl['layout']
    assert lay.swd == [] and len(lay.swd_all) == 1 and lay.ell_off == [0]
    assert (lay.tg[0].iwave, lay.tg[0].igr, lay.tg[0].mode, lay.tg[0].iflsph, lay.tg[0].nper, lay.tg[0].out_off) == \
        (2, 0, 1, 1, 21, 21)
    assert lay.ell[0].flsph == 1 and lay.ell[0].absolute is False
    assert len(bl['desc']) == 1


def test_three_targets_in_another_order_than_the_row():
    from bayhunter_amd import targets
    disp, rf, ell = _targets()
    joint = targets.JointTarget([ell, rf, disp])                  # row: dispersion, receiver function, ellipticity
    bl = joint.batch_layout(ell=True)
    _check(joint, bl, [slice(222, 243), slice(21, 222), slice(0, 21)], 243, 243, 1, [(0, 0, 0)])
    assert bl['layout'].ell_off == [222] and bl['layout'].rfp[0].out_off == 21
    # a Love target is no source: the ellipticity gets a hidden one, with a flag column of its own
    love = targets.LoveDispersionPhase(PER, np.full(21, 3.5))
    joint = targets.JointTarget([ell, love])
    bl = joint.batch_layout(ell=True)
    _check(joint, bl, [slice(21, 42), slice(0, 21)], 63, 42, 2, [(1, 21, 42)])


def test_without_the_argument_the_target_is_refused_and_other_layouts_do_not_change():
    from bayhunter_amd import targets
    disp, rf, ell = _targets()
    with pytest.raises(TypeError):
        targets.JointTarget([disp, ell]).batch_layout()
    with pytest.raises(TypeError):
        targets.JointTarget([disp, ell]).batch_layout(ell=False)
    joint = targets.JointTarget([rf, disp])
    a, b = joint.batch_layout(), joint.batch_layout(ell=True)
    assert a['nflags'] == b['nflags'] == 1 and a['layout'].row == b['layout'].row == 222
    assert a['yobs'].tobytes() == b['yobs'].tobytes() and a['aux'].tobytes() == b['aux'].tobytes()
    assert bytes(a['desc']) == bytes(b['desc']) and bytes(a['layout'].tg) == bytes(b['layout'].tg)
