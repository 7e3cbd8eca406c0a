"""Taylor-GPQD transform and ExtendedKalmanGPQD, the parts that need no device: the NumPy restatement (tests/_taylor_oracle.py)
against the reference's outputs (tests/golden/g21_taylor_gpqd.npz), its linearisation limit, and the constructors' checks."""
import ctypes

import numpy as np
import pytest

from oracle import ssmq_oracle as orc
from tests._cases import rel_err
from tests import _taylor_oracle as to


@pytest.fixture(scope='module')
def g21(golden):
    return golden('g21_taylor_gpqd')


@pytest.mark.parametrize('tag', list(to.CASES))
def test_oracle_agrees_with_the_reference(g21, tag):
    """Every array of the block to 1e-12 relative (max |a - b| / max |b| per parameter row) - the formula in the (E, D) convention
    and the transposition of the reference's cross-covariance."""
    fid, p, D, E, _ = to.CASES[tag]
    par = g21[tag + '_par']
    assert par.shape == (to.N_PAR, 1 + D) and g21[tag + '_cfx'].shape == (to.N_PAR, to.N_ITEMS, E, D)
    for r in range(to.N_PAR):
        got = [to.apply(fid, g21[tag + '_mean'][i], g21[tag + '_cov'][i], g21[tag + '_time'][i], par[r], p) for i in range(to.N_ITEMS)]
        for k, key in enumerate(('mf', 'cf', 'cfx', 'mvar', 'ivar')):
            a, b = np.array([g[k] for g in got]), g21[tag + '_' + key][r]
            assert a.shape == b.shape
            e = rel_err(a, b)
            assert e <= 1e-12, (tag, r, key, e)


@pytest.mark.parametrize('tag', list(to.CASES))
def test_long_length_scales_give_the_linearisation(g21, tag):
    """ell = 1e3: f(m), J P J', J P of the linearisation transform within the deviation the formula itself implies
    (_taylor_oracle.limit_bound, O(||P|| / ell^2)), computed per item."""
    fid, p, D, E, _ = to.CASES[tag]
    par = g21[tag + '_par'][to.LIMIT_ROW]
    assert np.all(par[1:] == to.ELL_LIMIT)
    for i in range(to.N_ITEMS):
        mean, cov, t = g21[tag + '_mean'][i], g21[tag + '_cov'][i], g21[tag + '_time'][i]
        mf, cf, cfx, _, _ = to.apply(fid, mean, cov, t, par, p)
        lm, lc, lx = orc.apply_linear(fid, mean, cov, t, p)
        fm, J = to.value_and_jacobian(fid, mean, t, p)
        b_mean, b_cov, b_ccov = to.limit_bound(fm, J, cov, par[0], par[1:])
        assert np.max(np.abs(mf - lm)) <= b_mean and np.max(np.abs(cf - lc)) <= b_cov and np.max(np.abs(cfx - lx)) <= b_ccov, (tag, i)
    # ... and the bound discriminates: with the ordinary length-scales of row 0 the last item's covariance lies outside it
    mf, cf, cfx, _, _ = to.apply(fid, mean, cov, t, g21[tag + '_par'][0], p)
    assert np.max(np.abs(cf - lc)) > b_cov


def test_constructor_checks_come_before_the_library(monkeypatch):
    import ssmtoybox_amd as amd
    from ssmtoybox_amd import ssinf, ssmod as sm, _lib

    class UserPendulum(sm.TransitionModel):
        dim_state, dim_noise, noise_additive = 2, 2, True
        device_code = 'o[0] = x[0] + p[0] * x[1]; o[1] = x[1] - 9.81 * p[0] * sin(x[0]);'

        def _par(self):
            return (0.01,)

    class UserPendulumMeas(sm.MeasurementModel):
        dim_out, dim_substate, dim_noise, noise_additive = 1, 1, 1, True
        device_code = 'o[0] = sin(x[0]);'

    def no_library():
        raise AssertionError('the library was reached')
    monkeypatch.setattr(_lib, 'load', no_library)
    for dim, par in ((2, np.ones((1, 2))), (2, np.ones(3)), (1, np.ones((2, 2)))):
        with pytest.raises(ValueError, match='shape'):
            amd.TaylorGPQDTransform(dim, par)
    for par in (np.array([[1.0, 0.0, 2.0]]), np.array([[1.0, -1.0, 2.0]]), np.array([[1.0, np.nan, 2.0]]), np.array([[np.inf, 1.0, 2.0]])):
        with pytest.raises(ValueError, match='positive'):
            amd.TaylorGPQDTransform(2, par)
    tf = amd.TaylorGPQDTransform(2, np.array([[1.5, 2.0, 3.0]]))
    assert tf.alpha == 1.5 and np.array_equal(tf.ell, [2.0, 3.0]) and np.array_equal(tf.Lam, np.diag([4.0, 9.0]))
    assert tf.mvar_list == [] and tf.ivar_list == []
    m, P, t = np.ones(2), np.eye(2), np.atleast_1d(0.0)
    for call in (tf.apply, tf.apply_batch):
        args = (m, P, t) if call == tf.apply else (m[None], P[None], 0.0)
        with pytest.raises(NotImplementedError, match='built-in model'):
            call(lambda x, p: x, *args)
        with pytest.raises(NotImplementedError, match='user model'):
            call(UserPendulum(sm.GaussRV(2), sm.GaussRV(2)).dyn_eval, *args)
    with pytest.raises(NotImplementedError, match='user model'):
        tf.kernel_name(UserPendulum(sm.GaussRV(2), sm.GaussRV(2)).dyn_eval)
    assert tf.mvar_list == []
    # the filter
    dyn = sm.Pendulum2DTransition(sm.GaussRV(2, mean=np.array([1.5, 0.0]), cov=0.01 * np.eye(2)), sm.GaussRV(2, cov=1e-3 * np.eye(2)), dt=0.01)
    obs = sm.Pendulum2DMeasurement(sm.GaussRV(1, cov=np.array([[0.1]])), 2)
    flt = ssinf.ExtendedKalmanGPQD(dyn, obs, np.array([[1.0, 3.0, 3.0]]), np.array([[1.0, 2.0, 2.0]]))
    assert isinstance(flt.tf_dyn, amd.TaylorGPQDTransform) and isinstance(flt.tf_obs, amd.TaylorGPQDTransform)
    assert flt.tf_dyn.dim == 2 and flt.tf_obs.dim == 2 and isinstance(flt, ssinf.GaussianInference)
    for name in ('forward_pass', 'forward_pass_batch', 'forward_pass_dev', 'backward_pass', 'backward_pass_batch', 'kernel_name', 'reset'):
        assert callable(getattr(flt, name))
    with pytest.raises(ValueError, match='shape'):
        ssinf.ExtendedKalmanGPQD(dyn, obs, np.array([[1.0, 3.0]]), np.array([[1.0, 2.0, 2.0]]))
    with pytest.raises(NotImplementedError, match='user model'):
        ssinf.ExtendedKalmanGPQD(UserPendulum(sm.GaussRV(2), sm.GaussRV(2)), UserPendulumMeas(sm.GaussRV(1), 2), np.ones((1, 3)), np.ones((1, 3)))
    with pytest.raises(NotImplementedError, match='additive'):
        ssinf.ExtendedKalmanGPQD(sm.UNGMNATransition(sm.GaussRV(1), sm.GaussRV(1)), sm.UNGMNAMeasurement(sm.GaussRV(1), 1),
                                 np.ones((1, 3)), np.ones((1, 3)))
    monkeypatch.undo()          # (run_filters loads the library before it looks at its filters)
    with pytest.raises(NotImplementedError, match='ExtendedKalmanGPQD'):
        ssinf.run_filters([flt], np.zeros((1, 3, 2)))


def test_library_exports_the_new_entry_points():
    from ssmtoybox_amd import _lib
    assert 'ssmq_transform_create_taylor_gpqd' in _lib.EXPORTED_SYMBOLS and 'ssmq_taylor_gpqd_variance_planes' in _lib.EXPORTED_SYMBOLS
    lib = ctypes.CDLL(_lib.library_path())
    for name in ('ssmq_transform_create_taylor_gpqd', 'ssmq_taylor_gpqd_variance_planes'):
        assert hasattr(lib, name), name
    assert _lib.FORM_TAYLOR_GPQD == 4
    import ssmtoybox_amd as amd
    assert amd.TaylorGPQDTransform is amd.mtran.TaylorGPQDTransform
