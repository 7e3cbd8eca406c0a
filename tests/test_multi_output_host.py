"""Multi-output GP / t-process quadrature without a GPU: the NumPy composition from the oracle's single-output parts
(tests/_mo_oracle.py) against the reference's results (tests/golden/g19_multi_output.npz, tests/golden/make_golden_mo.py), and
the shape, range and refusal behaviour of the Python classes - every refusal is raised before the library is loaded."""
import numpy as np
import pytest

from oracle import ssmq_oracle as orc
from tests._cases import assert_moments_close, rel_err
from tests._mo_oracle import CASES, NU, mo_weights, mo_moments, mo_emv, weight_bars, check_weights


@pytest.fixture(scope='module')
def g19(golden):
    return golden('g19_multi_output')


@pytest.fixture(scope='module')
def composed(g19):
    """The oracle composition of every case, computed once."""
    return {name: mo_weights(g19[name + '_par'], g19[name + '_xi']) for name in CASES}


def test_golden_covers_the_cases(g19):
    assert list(g19['names']) == list(CASES)
    for name, (D, E, pts, ppar, _) in CASES.items():
        assert g19[name + '_par'].shape == (E, D + 1)
        assert np.array_equal(g19[name + '_xi'], orc.unit_points(D, pts, ppar))
        assert g19[name + '_cond'].max() <= 1e7


@pytest.mark.parametrize('name', list(CASES))
def test_oracle_composition_reproduces_the_reference_weights(g19, composed, name):
    check_weights(composed[name], g19, name)
    Wc = composed[name]['Wc']
    assert np.array_equal(Wc, Wc.swapaxes(2, 3)) and np.array_equal(Wc, Wc.swapaxes(0, 1))


@pytest.mark.parametrize('kind', ['gp', 'tp'])
@pytest.mark.parametrize('name', list(CASES))
def test_oracle_composition_reproduces_the_reference_moments(g19, composed, name, kind):
    w = composed[name]
    for b in range(g19[name + '_mean'].shape[0]):
        fx, cov = g19[name + '_fx'][b], g19[name + '_cov'][b]
        emv = mo_emv(fx, w, NU if kind == 'tp' else None)
        assert rel_err(emv, g19[name + '_emv_' + kind][b]) <= weight_bars(float(g19[name + '_cond'].max()))[1]
        got = mo_moments(fx, np.linalg.cholesky(cov), w['wm'], w['Wc'], w['Wcc'], emv)
        ref = tuple(g19['{}_{}_{}'.format(name, k, kind)][b] for k in ('mf', 'cf', 'cfx'))
        assert_moments_close(got, ref, cov, what=(name, kind, b))


def test_cross_block_of_Q_is_not_symmetric_but_of_Wc_is(g19):
    Q, Wc = g19['pend_Q'], g19['pend_Wc']
    assert np.abs(Q[..., 1, 0] - Q[..., 1, 0].T).max() > 1e-3
    assert np.array_equal(Wc[..., 1, 0], Wc[..., 1, 0].T) and np.array_equal(Wc[..., 1, 0], Wc[..., 0, 1])


# ---- the Python classes: nothing below may load the library ----------------------------------------------------------------------
@pytest.fixture
def no_library(monkeypatch):
    from ssmtoybox_amd import _lib

    def refuse():
        raise AssertionError('the library was loaded')
    monkeypatch.setattr(_lib, 'load', refuse)


def test_supported_models():
    from ssmtoybox_amd.bq.bqmtran import BQTransform
    assert BQTransform._supported_models_ == ['gp', 'tp', 'bs', 'gp-mo', 'tp-mo']


def test_public_names():
    import ssmtoybox_amd as amd
    from ssmtoybox_amd import ssinf
    from ssmtoybox_amd.bq import bqmod
    for n in ('MultiOutputGaussianProcessTransform', 'MultiOutputStudentTProcessTransform'):
        assert hasattr(amd, n)
    for n in ('MultiOutputModel', 'GaussianProcessMO', 'StudentTProcessMO'):
        assert hasattr(bqmod, n)
    assert hasattr(ssinf, 'MultiOutputGaussianProcessKalman')


@pytest.mark.parametrize('cls', ['MultiOutputGaussianProcessTransform', 'MultiOutputStudentTProcessTransform'])
def test_kern_par_shape_is_checked(no_library, cls):
    import ssmtoybox_amd as amd
    for bad in (np.ones(3), np.ones((1, 3)), np.ones((2, 4)), np.ones((3, 3))):
        with pytest.raises(ValueError):
            getattr(amd, cls)(2, 2, bad)


@pytest.mark.parametrize('cls', ['MultiOutputGaussianProcessTransform', 'MultiOutputStudentTProcessTransform'])
def test_range_refusals_name_the_range(no_library, cls):
    import ssmtoybox_amd as amd
    T = getattr(amd, cls)
    with pytest.raises(NotImplementedError, match='E <= 8'):
        T(2, 9, np.ones((9, 3)))
    with pytest.raises(NotImplementedError, match='D <= 16'):
        T(17, 2, np.ones((2, 18)))
    with pytest.raises(NotImplementedError, match='N <= 64'):
        T(2, 2, np.ones((2, 3)), point_str='gh', point_par={'degree': 9})        # 81 points
    with pytest.raises(NotImplementedError, match="'rbf'"):
        T(2, 2, np.ones((2, 3)), kern_str='rbf-student')


def test_models_refuse_before_the_library(no_library):
    from ssmtoybox_amd.bq.bqmod import GaussianProcessMO, StudentTProcessMO
    with pytest.raises(ValueError):
        GaussianProcessMO(2, 2, np.ones((2, 4)), 'rbf', 'ut')
    with pytest.raises(NotImplementedError, match='E <= 8'):
        StudentTProcessMO(1, 9, np.ones((9, 2)), 'rbf', 'ut')
    m = GaussianProcessMO(2, 3, np.ones((3, 3)), 'rbf', 'ut')
    assert (m.dim_in, m.dim_out, m.num_pts) == (2, 3, 5)
    with pytest.raises(NotImplementedError):
        m.predict(np.zeros((2, 1)), np.zeros((3, 5)))
    with pytest.raises(NotImplementedError):
        StudentTProcessMO(2, 3, np.ones((3, 3)), 'rbf', 'ut').integral_variance(np.zeros((3, 5)))
    assert StudentTProcessMO(2, 3, np.ones((3, 3)), 'rbf', 'ut', nu=5.0).nu == 5.0
    with pytest.raises(ValueError):
        m.bq_weights(np.ones((2, 3)))


def test_optimize_returns_par_and_results_from_one_batch(no_library, monkeypatch):
    """(par (E, P), [OptimizeResult] * E) as the reference returns them, from ONE optimize_batch call on (E, N, 1) data."""
    from ssmtoybox_amd.bq.bqmod import GaussianProcessMO
    E, D, N = 3, 2, 5
    m = GaussianProcessMO(D, E, np.ones((E, D + 1)), 'rbf', 'ut')
    calls = []

    def stub(log_par_0, fcn_obs, x_obs, **options):
        calls.append((np.array(log_par_0), np.array(fcn_obs), options))
        B = log_par_0.shape[0]
        return dict(x=log_par_0 + 1.0, fun=np.arange(B, dtype=float), jac=np.zeros((B, D + 1)), hess_inv=np.zeros((B, D + 1, D + 1)),
                    nit=np.full(B, 7, dtype=np.int32), nfev=np.full(B, 9, dtype=np.int32), njev=np.full(B, 9, dtype=np.int32),
                    status=np.array([0, 2, 0], dtype=np.int32), success=np.array([True, False, True]))
    monkeypatch.setattr(m, 'optimize_batch', stub)
    lp0, y = np.log(np.arange(1.0, 1.0 + E * (D + 1)).reshape(E, D + 1)), np.arange(float(E * N)).reshape(E, N)
    par, results = m.optimize(lp0, y, m.points, options={'gtol': 1e-6})
    assert len(calls) == 1 and calls[0][1].shape == (E, N, 1) and calls[0][2] == {'gtol': 1e-6}
    assert np.array_equal(calls[0][1][:, :, 0], y)
    assert par.shape == (E, D + 1) and np.array_equal(par, lp0 + 1.0)
    assert len(results) == E and [r.success for r in results] == [True, False, True]
    assert all(np.array_equal(r.x, par[e]) and r.nit == 7 for e, r in enumerate(results))
    with pytest.raises(NotImplementedError):
        m.optimize(lp0, y, m.points, method='CG')
    with pytest.raises(ValueError):
        m.optimize(lp0[:2], y, m.points)


def test_filter_refusals(no_library):
    from ssmtoybox_amd import ssinf, ssmod as sm
    dyn = sm.UNGMTransition(sm.GaussRV(1), sm.GaussRV(1, cov=np.array([[10.0]])))
    obs = sm.UNGMMeasurement(sm.GaussRV(1), 1)
    with pytest.raises(ValueError):
        ssinf.MultiOutputGaussianProcessKalman(dyn, obs, np.ones((2, 2)), np.ones((1, 2)))
    with pytest.raises(NotImplementedError):
        ssinf.MultiOutputGaussianProcessKalman(dyn, obs, np.ones((1, 2)), np.ones((1, 2)), kernel='rbf-student')


def _user_models():
    from ssmtoybox_amd import ssmod as sm

    class UserPendulum(sm.TransitionModel):
        dim_state, dim_noise, noise_additive = 2, 2, True
        device_code = 'o[0] = x[0] + x[1] * p[0];  o[1] = x[1] - 9.81 * p[0] * sin_nr(x[0]);'

        def _par(self):
            return (0.01,)

    class UserPendulumMeas(sm.MeasurementModel):
        dim_out, dim_substate, dim_noise, noise_additive = 1, 1, 1, True
        device_code = 'o[0] = sin_nr(x[0]);'

    return UserPendulum(sm.GaussRV(2), sm.GaussRV(2)), UserPendulumMeas(sm.GaussRV(1), 2)


def test_user_models_are_refused_before_the_library(no_library, monkeypatch):
    """A device_code model: the filter refuses at construction; the transform (whose weights are device work, stubbed here) when
    it is handed the model's function - before the code is registered with the library."""
    from ssmtoybox_amd import ssinf
    from ssmtoybox_amd.bq import bqmtran
    dyn, obs = _user_models()
    with pytest.raises(NotImplementedError, match='built-in models'):
        ssinf.MultiOutputGaussianProcessKalman(dyn, obs, np.ones((2, 3)), np.ones((1, 3)))
    monkeypatch.setattr(bqmtran._MultiOutputTransform, 'weights', lambda self, par, *a: (np.zeros((5, 2)), np.zeros((5, 5, 2, 2)),
                                                                                         np.zeros((2, 5, 2))))
    for cls, kw in ((bqmtran.MultiOutputGaussianProcessTransform, {}), (bqmtran.MultiOutputStudentTProcessTransform, {'nu': 4.0})):
        tf = cls(2, 2, np.ones((2, 3)), **kw)
        with pytest.raises(NotImplementedError, match='built-in models'):
            tf.apply(dyn.dyn_eval, np.zeros(2), np.eye(2), np.zeros(1))
        with pytest.raises(NotImplementedError, match='built-in models'):
            tf.apply_batch(dyn.dyn_eval, np.zeros((3, 2)), np.tile(np.eye(2), (3, 1, 1)))
        with pytest.raises(NotImplementedError, match='built-in models'):
            tf.kernel_name(dyn.dyn_eval)
