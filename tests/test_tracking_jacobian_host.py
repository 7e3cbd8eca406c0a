"""The Jacobians of the coordinated turn, the radar and the bearing measurements on the host (no GPU): the 50-digit oracle of
tests/_tracking_jac_oracle.py against numerical differentiation, the NumPy twins of ssmod.py against the oracle, the placement
of meas_eval(dx=True), and which models the Jacobian transforms admit and refuse before the library is touched."""
import numpy as np
import pytest

from tests import _tracking_jac_oracle as tj

MODELS = ('ct', 'radar', 'bearing')


def _package_dx(name):
    from ssmtoybox_amd import ssmod as sm
    if name == 'ct':
        return sm.CoordinatedTurnTransition(dt=tj.DT).dyn_fcn_dx, 5
    if name == 'radar':
        return sm.Radar2DMeasurement(sm.GaussRV(2), 2, radar_loc=tj.RADAR_LOC).meas_fcn_dx, 2
    return sm.BearingMeasurement(sm.GaussRV(4), 2, sensor_pos=tj.SENSORS).meas_fcn_dx, 2


@pytest.mark.parametrize('name', MODELS)
def test_oracle_against_differentiation(name):
    """The analytic mpmath Jacobians against mpmath.diff of the mpmath functions: 1e-30 relative at every test point (entries
    that are structurally zero: 1e-30 absolute against the largest entry of the row's scale)."""
    import mpmath
    f, terms = {'ct': (tj.ct_f_mp, tj.ct_terms_mp), 'radar': (tj.radar_f_mp, tj.radar_terms_mp), 'bearing': (tj.bearing_f_mp, tj.bearing_terms_mp)}[name]
    pts = tj.reference(name)[0]
    assert len(pts) >= 64
    worst = 0.0
    for x in pts:
        J, _ = tj.collapse(terms(list(x)))
        Jd = tj.diff_jac_mp(f, list(x))
        for e in range(len(J)):
            for k in range(len(J[0])):
                a, d = J[e][k], Jd[e][k]
                err = abs(a - d) / abs(a) if a != 0 else abs(d)
                worst = max(worst, float(err))
                assert err <= mpmath.mpf('1e-30'), (name, x, e, k, a, d)
    print('{}: analytic against mpmath.diff, worst relative difference {:.3g}'.format(name, worst))


@pytest.mark.parametrize('name', MODELS)
def test_python_twins_against_the_oracle(name):
    """ssmod.py's dyn_fcn_dx / meas_fcn_dx at the bar of the device test: |err| <= K eps S, K = max(8, 4 x the worst ratio of the
    oracle module's own NumPy statement)."""
    f_dx, _ = _package_dx(name)
    K = tj.bound_K(name)
    J = np.array([f_dx(x, None, 0) for x in tj.reference(name)[0]])
    r = tj.ratio(J, name)
    print('{}: NumPy statement {:.3g}, ssmod twin {:.3g}, K = {:.3g}'.format(name, tj.twin_ratio(name), r, K))
    assert r <= K


def test_test_points():
    ct = tj.ct_points()
    th = np.abs(ct[:, 4]) * tj.DT
    for v in (5.2e-3, 1e-2, 0.1, 1.0, 3.0):
        assert np.any(np.abs(th - v) < 0.01 * v) and np.any(ct[np.abs(th - v) < 0.01 * v, 4] < 0) and np.any(ct[np.abs(th - v) < 0.01 * v, 4] > 0)
    assert np.max(np.abs(ct[:, [0, 2]])) > 1e3 and np.max(np.abs(ct[:, [1, 3]])) > 1e2
    for pts, centres in ((tj.radar_points(), [tj.RADAR_LOC]), (tj.bearing_points(), tj.SENSORS)):
        assert len(pts) >= 64
        near = np.min([np.hypot(pts[:, 0] - c[0], pts[:, 1] - c[1]) for c in centres], axis=0)
        assert near.min() < 1.01 and near.max() > 0.99e4
    p = tj.radar_points() - np.array(tj.RADAR_LOC)
    assert all(np.any((np.sign(p[:, 0]) == sx) & (np.sign(p[:, 1]) == sy)) for sx in (-1, 1) for sy in (-1, 1))
    ang = np.arctan2(p[:, 1], p[:, 0])
    assert np.any(ang > np.pi - 2e-3) and np.any(ang < -np.pi + 2e-3)


def test_placement():
    from ssmtoybox_amd import ssmod as sm
    p = np.array([730.0, -420.0])
    # radar without a state index on 4 and 5 states: the leading columns
    for D in (4, 5):
        x = np.concatenate((p, np.arange(1.0, D - 1)))
        J = sm.Radar2DMeasurement(sm.GaussRV(2), D, radar_loc=tj.RADAR_LOC).meas_eval(x, 0, dx=True)
        assert J.shape == (2, D) and not J[:, 2:].any()
        np.testing.assert_allclose(J[:, :2], tj.radar_dx(p), rtol=1e-15)
    # radar and bearings through state_index = [0, 2]
    x = np.array([p[0], 3.0, p[1], -4.0, 0.05])
    J = sm.Radar2DMeasurement(sm.GaussRV(2), 5, state_index=[0, 2], radar_loc=tj.RADAR_LOC).meas_eval(x, 0, dx=True)
    assert J.shape == (2, 5) and not J[:, [1, 3, 4]].any()
    np.testing.assert_allclose(J[:, [0, 2]], tj.radar_dx(p), rtol=1e-15)
    J = sm.BearingMeasurement(sm.GaussRV(4), 5, state_index=[0, 2], sensor_pos=tj.SENSORS).meas_eval(x, 0, dx=True)
    assert J.shape == (4, 5) and not J[:, [1, 3, 4]].any()
    np.testing.assert_allclose(J[:, [0, 2]], tj.bearing_dx(p), rtol=1e-15)
    # the pendulum's one-column broadcast is unchanged
    J = sm.Pendulum2DMeasurement(sm.GaussRV(1), 2).meas_eval(np.array([0.3, 1.0]), 0, dx=True)
    assert J.shape == (1, 2) and np.array_equal(J, np.full((1, 2), np.cos(0.3)))


def test_refusals():
    from ssmtoybox_amd import ssmod as sm
    from ssmtoybox_amd.bq.bqmtran import GaussianProcessDerTransform
    from ssmtoybox_amd.bq.bqmod import GaussianProcessDerModel
    tf = GaussianProcessDerTransform.__new__(GaussianProcessDerTransform)       # (the refusals need no weights: no __init__)
    tf.model = GaussianProcessDerModel(5, np.ones((1, 6)), 'ut', which_der=[])
    assert tf._device_integrand(sm.CoordinatedTurnTransition(dt=tj.DT).dyn_eval)[1] == 5
    assert tf._device_integrand(sm.Radar2DMeasurement(sm.GaussRV(2), 5, state_index=[0, 2]).meas_eval)[1] == 2
    assert tf._device_integrand(sm.BearingMeasurement(sm.GaussRV(4), 5, state_index=[0, 2]).meas_eval)[1] == 4
    with pytest.raises(NotImplementedError, match='no Jacobian'):
        tf._device_integrand(sm.ReentryVehicle2DTransition().dyn_eval)
    assert sm.ReentryVehicle1DTransition().dyn_fcn_dx(np.ones(3), np.zeros(3), 0) is None
    assert sm.RangeMeasurement(sm.GaussRV(1), 3).meas_fcn_dx(np.ones(1), np.zeros(1), 0) is None


def test_posterior_crlb_still_refuses_reentry():
    """The C range check of the posterior Cramer-Rao bound (no device needed): Reentry1D + Range has no Jacobian."""
    import ctypes
    from ssmtoybox_amd import _lib, ssmod as sm
    from ssmtoybox_amd import mcshard
    dyn = sm.ReentryVehicle1DTransition(sm.GaussRV(3), sm.GaussRV(3))
    obs = sm.RangeMeasurement(sm.GaussRV(1), 3)
    with pytest.raises(NotImplementedError, match='no Jacobian'):
        mcshard.crlb_kernel_name(dyn, obs)
    ct = sm.CoordinatedTurnTransition(sm.GaussRV(5), sm.GaussRV(5), dt=tj.DT)
    brg = sm.BearingMeasurement(sm.GaussRV(4, cov=1e-2 * np.eye(4)), 5, state_index=[0, 2], sensor_pos=tj.SENSORS)
    assert mcshard.crlb_kernel_name(ct, brg) == 'k_pcrlb_dyn<5, 5> | k_pcrlb_obs<5, 4> | k_pcrlb_rows'
