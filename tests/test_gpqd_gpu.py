"""GP quadrature with derivative observations (GPQ+D) on the device: the weights of k_weights_gpqd against the NumPy oracle
(tests/_gpqd_oracle.py) under the bound of tests/test_gpqd_host.py, the moments of k_apply_gpqd / k_apply_gpqd_lds against the
oracle fed with the device's own weights (rounding level: assert_moments_close with its defaults), bitwise properties, the status
of a covariance that is not positive definite, and GaussianProcessDerKalman against a Python loop of its own transforms.
Batches are B = 130: two full waves and a partial one."""
import numpy as np
import pytest

from oracle import ssmq_oracle as orc
from tests import _gpqd_oracle as go
from tests._cases import assert_moments_close, mean_err, cov_err
from tests._gpqd_cases import WEIGHT_CASES
from tests._taylor_oracle import value_and_jacobian
from tests.test_gpqd_host import BOUND, weight_distance, _user_model

pytestmark = pytest.mark.gpu

B = 130
PAR1, PAR2 = np.array([[3.0, 1.2]]), np.array([[1.5, 2.0, 3.5]])
# D = 6: the bound of the host test was measured on joint kernel matrices with cond(K + jitter I) <= 2.6e4, and the distance between two
# routes through the solve grows with that number; these length-scales keep the 91 x 91 matrix inside it (the test asserts so)
PAR6 = np.array([[1.0, 2.0, 1.8, 2.4, 2.2, 1.9, 2.6]])
COND_OF_THE_BOUND = 2.64e4


def rv(d, mean=None, cov=None):
    from ssmtoybox_amd import ssmod
    return ssmod.GaussRV(d, mean=mean, cov=cov)


def inputs(D, seed, n=B):
    rng = np.random.default_rng(seed)
    mean = rng.uniform(-2.0, 2.0, (n, D))
    a = rng.standard_normal((n, D, D)) / np.sqrt(D)
    cov = np.einsum('bij,bkj->bik', a, a) + 0.05 * np.eye(D)
    return mean, 0.5 * (cov + cov.transpose(0, 2, 1)), rng.integers(0, 20, n).astype(float)


def builtin(tag):
    """(f of the package, oracle f(x, t), oracle f_dx(x, t) in the columns of the full input)."""
    from tests._jacobian_cases import package_models
    from tests._taylor_oracle import CASES
    fid, p = CASES[tag][0], CASES[tag][1]
    return (package_models()[tag], lambda x, t: value_and_jacobian(fid, x, t, p)[0], lambda x, t: value_and_jacobian(fid, x, t, p)[1])


def device_weights(tf):
    return dict(wm=tf.wm, Wc=tf.Wc, Wcc=tf.Wcc, model_var=tf.model.model_var, integral_var=tf.model.integral_var)


@pytest.mark.parametrize('tag', list(WEIGHT_CASES) + ['d6_ut'])
def test_weights_against_the_oracle(tag):
    from ssmtoybox_amd.bq.bqmod import GaussianProcessDerModel
    D, pts, ppar, par = WEIGHT_CASES.get(tag, (6, 'ut', None, list(PAR6[0])))
    model = GaussianProcessDerModel(D, np.array([par]), pts, ppar)
    wm, Wc, Wcc, mv, iv = model.bq_weights(np.array([par]))
    M = model.num_pts * (1 + D)
    cond = np.linalg.cond(np.asarray(go.joint_kernel(model.points, par), dtype=float) + 1e-8 * np.eye(M))
    assert cond <= COND_OF_THE_BOUND, cond
    assert wm.shape == (M,) and Wc.shape == (M, M) and Wcc.shape == (D, M) and np.array_equal(Wc, Wc.T)
    e, parts = weight_distance(dict(wm=wm, Wc=Wc, Wcc=Wcc, model_var=mv, integral_var=iv), go.weights(model.points, par), par[0])
    print('{} (M = {}): device weights against the oracle {}'.format(tag, M, {k: '%.3g' % v for k, v in parts.items()}))
    assert e <= BOUND, parts


def test_kernel_methods_shapes_and_subset():
    from ssmtoybox_amd.bq.bqkern import RBFGaussDer
    k = RBFGaussDer(2, PAR2)
    x, wd = orc.points_ut(2), [0, 2]
    assert k.eval(PAR2, x, which_der=wd).shape == (9, 9) and k.eval_chol(PAR2, x, which_der=wd).shape == (9, 9)
    assert k.exp_x_dkx(PAR2, x, which_der=wd).shape == (4,) and k.exp_x_xdkx(PAR2, x, which_der=wd).shape == (2, 4)
    assert k.exp_x_kxdkx(PAR2, x, which_der=wd).shape == (5, 4) and k.exp_x_dkxdkx(PAR2, x, which_der=wd).shape == (4, 4)
    K = np.asarray(go.joint_kernel(x, PAR2[0], wd, scaling=True), dtype=float)
    assert np.max(np.abs(k.eval(PAR2, x, which_der=wd) - K)) <= 1e-13 * np.max(np.abs(K))
    L = k.eval_chol(PAR2, x, which_der=wd)
    assert np.max(np.abs(L.dot(L.T) - K - 1e-8 * np.eye(9))) <= 1e-13 * np.max(np.abs(K))
    q, Q, R = go.expectations(x, PAR2[0], wd)
    assert np.max(np.abs(k.exp_x_dkx(PAR2, x, which_der=wd) - q[5:])) <= 1e-14
    assert np.max(np.abs(k.exp_x_dkxdkx(PAR2, x, which_der=wd) - Q[5:, 5:])) <= 1e-14
    assert np.max(np.abs(k.exp_x_kxdkx(PAR2, x, which_der=wd) - Q[:5, 5:])) <= 1e-14
    assert np.max(np.abs(k.exp_x_xdkx(PAR2, x, which_der=wd) - R[:, 5:])) <= 1e-14


APPLY_CASES = {
    'ungm_dyn': ('ungm_dyn', 1, PAR1, 'ut', {'kappa': 0.0}, None, 'k_apply_gpqd'),
    'pend_dyn': ('pend_dyn', 2, PAR2, 'ut', None, None, 'k_apply_gpqd'),
    'pend_meas': ('pend_meas', 2, PAR2, 'ut', None, None, 'k_apply_gpqd'),
    'pend_dyn_sr': ('pend_dyn', 2, PAR2, 'sr', None, None, 'k_apply_gpqd'),
    'pend_dyn_der0': ('pend_dyn', 2, PAR2, 'ut', None, [0], 'k_apply_gpqd'),
    'pend_dyn_der02': ('pend_dyn', 2, PAR2, 'ut', None, [0, 2], 'k_apply_gpqd'),
    'pend_dyn_none': ('pend_dyn', 2, PAR2, 'ut', None, [], 'k_apply_gpqd'),
    'cv_dyn': ('cv_dyn', 4, np.array([[1.0, 3.0, 3.0, 3.0, 3.0]]), 'ut', None, None, 'k_apply_gpqd_lds'),
}


@pytest.mark.parametrize('case', list(APPLY_CASES))
def test_apply_builtin_against_the_oracle(case):
    import ssmtoybox_amd as amd
    tag, D, par, pts, ppar, wd, kernel = APPLY_CASES[case]
    f, of, odx = builtin(tag)
    mean, cov, time = inputs(D, 11)
    E = np.atleast_1d(of(mean[0], 0.0)).shape[0]
    tf = amd.GaussianProcessDerTransform(D, E, par, pts, ppar, which_der=wd)
    assert tf.kernel_name(f) == kernel
    got = tf.apply_batch(f, mean, cov, time)
    assert got[0].shape == (B, E) and got[1].shape == (B, E, E) and got[2].shape == (B, E, D)
    ref = go.apply_batch(of, odx, mean, cov, time, tf.model.points, wd, device_weights(tf))
    e = assert_moments_close(got, ref, cov, what=case)
    print('{}: device against the oracle with the device\'s weights {:.3g}'.format(case, e))


def wide_model():
    """D = 6, E = 4 user model (the LDS route) with its NumPy statement."""
    from ssmtoybox_amd import ssmod  # noqa: F401
    D, E = 6, 4
    mod = _user_model(D, E)(rv(E), D)
    idx = [(e % D, (e + 1) % D, (e + 2) % D) for e in range(E)]

    def f(x, t):
        return np.array([np.sin(x[a]) + 0.3 * x[b] * x[c] for a, b, c in idx])

    def f_dx(x, t):
        J = np.zeros((E, D))
        for e, (a, b, c) in enumerate(idx):
            J[e, a] += np.cos(x[a])
            J[e, b] += 0.3 * x[c]
            J[e, c] += 0.3 * x[b]
        return J
    return mod, f, f_dx


@pytest.mark.parametrize('wd', [None, [0, 5, 12]])
def test_apply_user_model_lds_route_against_the_oracle(wd):
    import ssmtoybox_amd as amd
    mod, f, f_dx = wide_model()
    tf = amd.GaussianProcessDerTransform(6, 4, PAR6, which_der=wd)
    assert tf.model.num_pts == 13 and tf.kernel_name(mod.meas_eval).startswith('k_apply_gpqd_lds<')
    mean, cov, time = inputs(6, 12)
    got = tf.apply_batch(mod.meas_eval, mean, cov, time)
    ref = go.apply_batch(f, f_dx, mean, cov, time, tf.model.points, wd, device_weights(tf))
    e = assert_moments_close(got, ref, cov, what='user 6x4')
    print('user model D = 6, E = 4, N = 13, which_der = {}: {:.3g}'.format(wd, e))
    # an item's bits depend neither on the batch nor on its position in it
    for b in (0, 77, 129):
        one = tf.apply_batch(mod.meas_eval, mean[b:b + 1], cov[b:b + 1], time[b:b + 1])
        assert all(np.array_equal(o[0], g[b]) for o, g in zip(one, got))


def test_no_derivatives_is_gp_quadrature():
    import ssmtoybox_amd as amd
    f, _, _ = builtin('pend_dyn')
    mean, cov, time = inputs(2, 13)
    tf = amd.GaussianProcessDerTransform(2, 2, PAR2, which_der=[])
    gp = amd.GaussianProcessTransform(2, 2, PAR2)
    e = assert_moments_close(tf.apply_batch(f, mean, cov, time), gp.apply_batch(f, mean, cov, time), cov, what='which_der=[]')
    print('which_der=[] against GaussianProcessTransform: {:.3g}'.format(e))


def test_bitwise_properties():
    import ssmtoybox_amd as amd
    from tests import _user_jac_oracle as uo
    f, _, _ = builtin('pend_dyn')
    mean, cov, time = inputs(2, 14)
    tf = amd.GaussianProcessDerTransform(2, 2, PAR2)
    got = tf.apply_batch(f, mean, cov, time)
    one = tf.apply(f, mean[0], cov[0], time[0])
    assert all(np.array_equal(o, g[0]) for o, g in zip(one, got))
    for b in (0, 64, 129):
        alone = tf.apply_batch(f, mean[b:b + 1], cov[b:b + 1], time[b:b + 1])
        assert all(np.array_equal(o[0], g[b]) for o, g in zip(alone, got))
    Pend = uo.transition('Pend', 2, uo.PEND_CODE, uo.PEND_JAC, (0.01,))
    user = Pend(rv(2), rv(2)).dyn_eval
    assert tf.kernel_name(user).startswith('k_apply_gpqd<')
    again = tf.apply_batch(user, mean, cov, time)
    assert all(np.array_equal(a, g) for a, g in zip(again, got))


def test_covariance_that_is_not_positive_definite():
    import ssmtoybox_amd as amd
    for tag, D, par in (('pend_dyn', 2, PAR2), ('cv_dyn', 4, np.array([[1.0, 3.0, 3.0, 3.0, 3.0]]))):
        f, _, _ = builtin(tag)
        mean, cov, time = inputs(D, 15)
        tf = amd.GaussianProcessDerTransform(D, D, par)
        good = tf.apply_batch(f, mean, cov, time)
        bad = cov.copy()
        bad[70] = -np.eye(D)
        mf, cf, cfx, st = tf.apply_batch(f, mean, bad, time, return_status=True)
        assert st[70] == 1 and st.sum() == 1 and np.all(np.isnan(mf[70])) and np.all(np.isnan(cf[70])) and np.all(np.isnan(cfx[70]))
        keep = np.arange(B) != 70
        assert np.array_equal(mf[keep], good[0][keep]) and np.array_equal(cf[keep], good[1][keep]) and np.array_equal(cfx[keep], good[2][keep])
        with pytest.raises(np.linalg.LinAlgError):
            tf.apply_batch(f, mean, bad, time)


def test_kalman_filter_on_the_pendulum():
    """T = 20, B = 70: step for step the filter equals a Python loop of its own transforms' apply_batch and the host Kalman update.
    Both run the same kernels on the same handles; what differs is the rounding of the update, carried through 20 steps: the
    project's bar for moments, 1e-10, on the row-scaled means and the entry-scaled covariances."""
    from ssmtoybox_amd import ssinf, ssmod
    T, Bf, dt = 20, 70, 0.01
    q2 = rv(2, cov=0.01 * np.array([[(dt ** 3) / 3, (dt ** 2) / 2], [(dt ** 2) / 2, dt]]))
    dyn = ssmod.Pendulum2DTransition(rv(2, mean=np.array([1.5, 0.0]), cov=0.01 * np.eye(2)), q2, dt=dt)
    obs = ssmod.Pendulum2DMeasurement(rv(1, cov=np.array([[0.1]])), 2)
    rng = np.random.default_rng(16)
    x = np.array([1.5, 0.0])[:, None] + 0.1 * rng.standard_normal((2, Bf))
    y = np.zeros((1, T, Bf))
    for k in range(T):
        x = np.stack((x[0] + x[1] * dt, x[1] - 9.81 * dt * np.sin(x[0])))
        y[0, k] = np.sin(x[0]) + np.sqrt(0.1) * rng.standard_normal(Bf)
    flt = ssinf.GaussianProcessDerKalman(dyn, obs, PAR2, PAR2, which_der_obs=[0, 1, 3])
    assert 'hipGraph of 3 T launches' in flt.kernel_name()
    fm, fP = flt.forward_pass_batch(y)
    assert not flt.status.any()
    m, P = np.tile(flt.x0_mean, (Bf, 1)), np.tile(flt.x0_cov, (Bf, 1, 1))
    gqg = flt.G.dot(flt.q_cov).dot(flt.G.T)
    rm, rP = np.zeros_like(fm), np.zeros_like(fP)
    for k in range(T):
        mp, Pp, _ = flt.tf_dyn.apply_batch(dyn.dyn_eval, m, P, float(k))
        Pp = Pp + gqg
        ym, Py, Pyx = flt.tf_obs.apply_batch(obs.meas_eval, mp, Pp, float(k))
        Py = Py + flt.r_cov
        for b in range(Bf):
            m[b], P[b] = orc.kalman_update(mp[b], Pp[b], ym[b], Py[b], Pyx[b], y[:, k, b])
        rm[:, k], rP[:, :, k] = m.T, P.transpose(1, 2, 0)
    e_m, e_P = mean_err(fm, rm), cov_err(fP, rP)
    print('GaussianProcessDerKalman on the pendulum against the loop of its transforms: mean_err {:.3g}, cov_err {:.3g}'.format(e_m, e_P))
    assert e_m <= 1e-10 and e_P <= 1e-10, (e_m, e_P)
    sm, sP = flt.backward_pass_batch()
    assert np.all(np.isfinite(sm)) and np.all(np.isfinite(sP))
    assert np.array_equal(sm[:, -1], flt.fi_mean[:, -1]) and np.array_equal(sP[:, :, -1], flt.fi_cov[:, :, -1])
    with pytest.raises(NotImplementedError, match='GaussianProcessDerKalman'):
        ssinf.run_filters([flt], y)
