"""Multi-output GP / t-process quadrature on the device: weights (ssmq_weights_gp_mo), the transform (k_apply_mo) through
apply / apply_batch / the Python-integrand route, the launch-loop filter and ML-II, against tests/golden/g19_multi_output.npz
and the NumPy composition of tests/_mo_oracle.py."""
import ctypes

import numpy as np
import pytest

from oracle import ssmq_oracle as orc
from tests._cases import assert_moments_close, mean_err, cov_err
from tests._mo_oracle import CASES, NU, mo_moments, smooth_map, check_weights

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def g19(golden):
    return golden('g19_multi_output')


def package_model(fname):
    from ssmtoybox_amd import ssmod as sm
    r = lambda n: sm.GaussRV(n)      # noqa: E731
    return {'ungm_dyn': lambda: sm.UNGMTransition().dyn_eval, 'pend_dyn': lambda: sm.Pendulum2DTransition(dt=0.01).dyn_eval,
            'radar_meas': lambda: sm.Radar2DMeasurement(r(2), 5).meas_eval,
            'reentry_dyn': lambda: sm.ReentryVehicle2DTransition().dyn_eval,
            'reentry_bias_dyn': lambda: sm.ReentryVehicle2DBiasTransition().dyn_eval}[fname]()


_TF = {}


def transform(g, name, kind):
    """One transform per (case, model), shared by the tests."""
    import ssmtoybox_amd as amd
    if (name, kind) not in _TF:
        D, E, pts, ppar, fname = CASES[name]
        if kind == 'gp':
            tf = amd.MultiOutputGaussianProcessTransform(D, E, g[name + '_par'], 'rbf', pts, ppar)
        else:
            tf = amd.MultiOutputStudentTProcessTransform(D, E, g[name + '_par'], 'rbf', pts, ppar, nu=NU)
        f = (lambda x, t, E=E: smooth_map(x, E)) if fname == 'smooth' else package_model(fname)
        _TF[(name, kind)] = (tf, f)
    return _TF[(name, kind)]


@pytest.mark.parametrize('name', list(CASES))
def test_weights_from_the_device(g19, name):
    tf, _ = transform(g19, name, 'gp')
    m = tf.model
    w = dict(wm=tf.wm, Wc=tf.Wc, Wcc=tf.Wcc, q=m.q, Q=m.Q, R=m.R, iK=m.iK, model_var=m.exp_model_variance(None),
             integral_var=m.integral_variance(None))
    check_weights(w, g19, name)
    assert np.array_equal(tf.Wc, tf.Wc.swapaxes(2, 3)), 'Wc[..., i, j] == Wc[..., j, i]'
    assert np.array_equal(tf.Wc, tf.Wc.swapaxes(0, 1)), 'every block equals its transpose'
    wm2, Wc2, Wcc2 = tf.weights(g19[name + '_par'])
    assert np.array_equal(wm2, tf.wm) and np.array_equal(Wc2, tf.Wc) and np.array_equal(Wcc2, tf.Wcc)


@pytest.mark.parametrize('kind', ['gp', 'tp'])
@pytest.mark.parametrize('name', list(CASES))
def test_apply_and_apply_batch(g19, name, kind):
    tf, f = transform(g19, name, kind)
    mean, cov, t = g19[name + '_mean'], g19[name + '_cov'], float(g19[name + '_time'])
    mf, cf, cfx = tf.apply_batch(f, mean, cov, t)
    for b in range(mean.shape[0]):
        ref = tuple(g19['{}_{}_{}'.format(name, k, kind)][b] for k in ('mf', 'cf', 'cfx'))
        assert_moments_close((mf[b], cf[b], cfx[b]), ref, cov[b], what=(name, kind, b))
        assert np.array_equal(cf[b], cf[b].T)
    for b in range(mean.shape[0]):        # B = 1 agrees with its row of the batch bit for bit, row by row
        one = tf.apply(f, mean[b], cov[b], np.atleast_1d(t))
        assert np.array_equal(one[0], mf[b]) and np.array_equal(one[1], cf[b]) and np.array_equal(one[2], cfx[b]), (name, kind, b)
        assert one[0].flags.writeable and one[1].base is not cf


@pytest.mark.parametrize('kind', ['gp', 'tp'])
@pytest.mark.parametrize('name', ['pend', 'reentry'])
def test_equal_rows_give_the_single_output_transform(g19, name, kind):
    import ssmtoybox_amd as amd
    D, E, pts, ppar, fname = CASES[name]
    row = g19[name + '_par'][:1]
    f = package_model(fname)
    if kind == 'gp':
        mo = amd.MultiOutputGaussianProcessTransform(D, E, np.repeat(row, E, axis=0), 'rbf', pts, ppar)
        so = amd.GaussianProcessTransform(D, E, row, 'rbf', pts, ppar)
    else:
        mo = amd.MultiOutputStudentTProcessTransform(D, E, np.repeat(row, E, axis=0), 'rbf', pts, ppar, nu=NU)
        so = amd.StudentTProcessTransform(D, E, row, 'rbf', pts, ppar, nu=NU)
        so.model.nu = NU
    mean, cov, t = g19[name + '_mean'], g19[name + '_cov'], float(g19[name + '_time'])
    got, ref = mo.apply_batch(f, mean, cov, t), so.apply_batch(f, mean, cov, t)
    for b in range(mean.shape[0]):
        assert_moments_close(tuple(a[b] for a in got), tuple(a[b] for a in ref), cov[b], what=(name, kind, b))


@pytest.mark.parametrize('name', ['pend', 'reentry_bias'])
def test_batch_independence(g19, name):
    """B = 193 (three waves and one lane): every row is its B = 1 result bit for bit; a covariance that is not positive definite
    marks its own row and leaves every other row's bits."""
    tf, f = transform(g19, name, 'tp')
    B = 193
    mean = np.tile(g19[name + '_mean'], (13, 1))[:B] * (1.0 + 1e-3 * np.arange(B)[:, None] / B)
    cov = np.tile(g19[name + '_cov'], (13, 1, 1))[:B]
    t = float(g19[name + '_time'])
    mf, cf, cfx, st = tf.apply_batch(f, mean, cov, t, return_status=True)
    assert not st.any() and np.all(np.isfinite(cf))
    for b in range(B):
        one = tf.apply_batch(f, mean[b:b + 1], cov[b:b + 1], t)
        assert np.array_equal(one[0][0], mf[b]) and np.array_equal(one[1][0], cf[b]) and np.array_equal(one[2][0], cfx[b]), (name, b)
    bad = cov.copy()
    bad[97] = -np.eye(cov.shape[1])
    mf2, cf2, cfx2, st2 = tf.apply_batch(f, mean, bad, t, return_status=True)
    assert st2[97] == 1 and st2.sum() == 1
    keep = np.arange(B) != 97
    assert np.array_equal(mf2[keep], mf[keep]) and np.array_equal(cf2[keep], cf[keep]) and np.array_equal(cfx2[keep], cfx[keep])
    with pytest.raises(np.linalg.LinAlgError):
        tf.apply_batch(f, mean, bad, t)


@pytest.mark.parametrize('kind', ['gp', 'tp'])
def test_constants_through_l2_give_the_bits_of_the_lds_route(g19, monkeypatch, kind):
    """SSMQ_MO_NO_LDS=1 reads the constant block through L2 instead of staging it in LDS: the same arithmetic, the same bits."""
    tf, f = transform(g19, 'reentry', kind)
    mean, cov, t = g19['reentry_mean'], g19['reentry_cov'], float(g19['reentry_time'])
    monkeypatch.delenv('SSMQ_MO_NO_LDS', raising=False)
    staged = tf.apply_batch(f, mean, cov, t)
    monkeypatch.setenv('SSMQ_MO_NO_LDS', '1')
    through_l2 = tf.apply_batch(f, mean, cov, t)
    monkeypatch.delenv('SSMQ_MO_NO_LDS')
    for a, b in zip(staged, through_l2):
        assert np.array_equal(a, b)


def test_all_covariances_failing_with_a_python_integrand(g19):
    """No integrand value can be formed: NaN moments of the transform's own shapes and a status per row, nothing out of bounds."""
    tf, f = transform(g19, 'smooth23', 'gp')
    mean, cov = g19['smooth23_mean'][:3], -np.tile(np.eye(2), (3, 1, 1))
    mf, cf, cfx, st = tf.apply_batch(f, mean, cov, return_status=True)
    assert mf.shape == (3, 3) and cf.shape == (3, 3, 3) and cfx.shape == (3, 3, 2) and np.all(st == 1)
    assert np.all(np.isnan(mf)) and np.all(np.isnan(cf))


def test_shapes_whose_work_space_exceeds_the_lds_are_refused():
    """Through the C ABI a point set may have fewer than 2 D points; 64 / N trajectories per wave then may not fit the LDS."""
    from ssmtoybox_amd import _lib
    lib = _lib.load()
    for D, E, N, ok in ((16, 8, 8, False), (12, 8, 4, False), (16, 8, 32, True), (16, 8, 64, True)):
        z = lambda *sh: _lib.as_c(np.zeros(sh))      # noqa: E731
        xi, wm, Wc, Wcc = z(D, N), z(E, N), z(E, E, N, N), z(E, D, N)
        h = lib.ssmq_transform_create_mo(D, E, N, xi[1], wm[1], Wc[1], Wcc[1], None, 0.0, None)
        assert bool(h) == ok, (D, E, N)
        if h:
            lib.ssmq_transform_destroy(ctypes.c_void_p(h))
        else:
            assert 'LDS' in _lib.last_error()


def test_range_boundary_with_assigned_weights():
    """D = 2, E = 8, N = 64 (Gauss-Hermite degree 8) on the apply path alone: random symmetric-block weights assigned through
    tf.wm / Wc / Wcc (the update entry point), against the NumPy composition; no kernel matrix, so conditioning plays no part."""
    import ssmtoybox_amd as amd
    D, E = 2, 8
    rng = np.random.default_rng(19)
    for cls, nu in ((amd.MultiOutputGaussianProcessTransform, None), (amd.MultiOutputStudentTProcessTransform, NU)):
        tf = cls(D, E, np.column_stack((np.ones(E), np.full((E, D), 3.0))), 'rbf', 'gh', {'degree': 8},
                 **({} if nu is None else {'nu': nu}))
        N = tf.model.points.shape[1]
        assert N == 64
        f = lambda x, t: np.concatenate((smooth_map(x, 4), smooth_map(x[::-1], 4)))      # noqa: E731
        mean, cov = rng.standard_normal((3, D)), np.array([np.eye(D) * 0.5 + 0.1 for _ in range(3)])
        first = tf.apply_batch(f, mean, cov)                    # creates the handle with the computed weights
        Wc = rng.standard_normal((N, N, E, E)) / N
        Wc = 0.5 * (Wc + Wc.swapaxes(0, 1))
        Wc = np.where((np.arange(E)[:, None] >= np.arange(E)[None, :]), Wc, Wc.swapaxes(2, 3))
        tf.wm, tf.Wc, tf.Wcc = rng.standard_normal((N, E)) / N, Wc, rng.standard_normal((D, N, E)) / N
        tf.model.model_var = rng.uniform(0.1, 1.0, E)
        got = tf.apply_batch(f, mean, cov)
        assert not np.array_equal(got[1], first[1])
        for b in range(3):
            chol = np.linalg.cholesky(cov[b])
            fx = np.apply_along_axis(f, 0, mean[b][:, None] + chol.dot(tf.model.points), None)
            emv = tf.model.model_var if nu is None else tf.model.exp_model_variance(fx)
            ref = mo_moments(fx, chol, tf.wm, tf.Wc, tf.Wcc, emv)
            assert_moments_close(tuple(a[b] for a in got), ref, cov[b], what=(cls.__name__, b))


def host_recursion(flt, y):
    """The filter's recursion stepped on the host: the transforms' own apply_batch per step and the oracle's Kalman update."""
    Y, T, B = y.shape
    D = flt.mod_dyn.dim_state
    m, P = np.tile(flt.x0_mean, (B, 1)), np.tile(flt.x0_cov, (B, 1, 1))
    gqg = flt.G.dot(flt.q_cov).dot(flt.G.T)
    fm, fP = np.zeros((D, T, B)), np.zeros((D, D, T, B))
    for k in range(T):
        mp, Pp, _ = flt.tf_dyn.apply_batch(flt.mod_dyn.dyn_eval, m, P, float(k))
        Pp = Pp + gqg
        ym, Py, Pyx = flt.tf_obs.apply_batch(flt.mod_obs.meas_eval, mp, Pp, float(k))
        Py = Py + flt.r_cov
        for b in range(B):
            m[b], P[b] = orc.kalman_update(mp[b], Pp[b], ym[b], Py[b], Pyx[b], y[:, k, b])
        fm[:, k], fP[:, :, k] = m.T, P.transpose(1, 2, 0)
    return fm, fP


@pytest.mark.parametrize('system', ['ungm', 'pendulum'])
def test_multi_output_kalman_filter(system):
    from ssmtoybox_amd import ssinf, ssmod as sm, _lib
    rng = np.random.default_rng(5)
    T, B = 20, 8
    if system == 'ungm':
        dyn = sm.UNGMTransition(sm.GaussRV(1), sm.GaussRV(1, cov=np.array([[10.0]])))
        obs = sm.UNGMMeasurement(sm.GaussRV(1), 1)
        kd, ko = np.array([[1.0, 3.0]]), np.array([[1.0, 2.0]])
        y = 0.05 * (3.0 * rng.standard_normal((1, T, B))) ** 2 + rng.standard_normal((1, T, B))
    else:
        dyn = sm.Pendulum2DTransition(sm.GaussRV(2, mean=np.array([1.5, 0.0]), cov=0.01 * np.eye(2)), sm.GaussRV(2, cov=1e-3 * np.eye(2)),
                                      dt=0.01)
        obs = sm.Pendulum2DMeasurement(sm.GaussRV(1, cov=np.array([[0.1]])), 2)
        kd, ko = np.array([[1.0, 3.0, 3.0], [1.5, 2.0, 1.0]]), np.array([[1.0, 3.0, 2.0]])
        y = np.sin(1.5) + 0.3 * rng.standard_normal((1, T, B))
    flt = ssinf.MultiOutputGaussianProcessKalman(dyn, obs, kd, ko)
    assert 'hipGraph of 3 T launches' in flt.kernel_name()
    assert flt.tf_dyn.kernel_name(dyn.dyn_eval) == 'k_apply_mo' and flt.tf_obs.kernel_name(obs.meas_eval) == 'k_apply_mo'
    fm, fP = flt.forward_pass_batch(y)
    rm, rP = host_recursion(flt, y)
    # the bars and metrics of the launch-loop parity tests (tests/test_gpu_parity.py: fused against loop): row-scaled mean error
    # 1e-12, entry-scaled covariance error 1e-11
    e_m, e_P = mean_err(fm, rm), cov_err(fP, rP)
    print('multi-output filter against the host recursion ({}): mean_err {:.3g}, cov_err {:.3g}'.format(system, e_m, e_P))
    assert e_m < 1e-12 and e_P < 1e-11, (system, e_m, e_P)
    fm1, fP1 = flt.forward_pass(y[..., 0])
    assert np.array_equal(fm1, fm[..., 0]) and np.array_equal(fP1, fP[..., 0])
    ld = 64
    d_y = _lib.DeviceBuffer(8 * T * ld)
    _lib.upload_study(y, 1, ld, d_y)
    d_fm, d_fP, d_st = flt.forward_pass_dev(d_y, B, ld, T)
    assert np.array_equal(_lib.download_study(d_fm, (dyn.dim_state,), T, B, ld), fm)
    for buf in (d_y, d_fm, d_fP, d_st):
        buf.free()
    for call in (flt.backward_pass, flt.backward_pass_batch, lambda: ssinf.run_filters([flt], y)):
        with pytest.raises(NotImplementedError):
            call()


def test_other_entry_points_refuse_the_form(g19):
    """SSMQ_E_UNSUPPORTED (-3) with the outputs untouched."""
    from ssmtoybox_amd import _lib, ssmod as sm
    lib = _lib.load()
    tf, _ = transform(g19, 'ungm', 'gp')
    h = ctypes.c_void_p(tf._handle_for(1))
    fd, _ = sm.UNGMTransition().device_integrand()
    fo, _ = sm.UNGMMeasurement(sm.GaussRV(1), 1).device_integrand()
    one, p1 = _lib.as_c(np.ones(4))
    assert lib.ssmq_transform_update(h, None, p1, None, None, None, 0, 0.0, None) == -3
    assert lib.ssmq_fxwc_batch_dev(h, 0, None, 0, None, 0, None) == -3
    buf = _lib.DeviceBuffer(8 * 64 * 64)
    p = ctypes.c_void_p(buf.ptr)
    sent = np.full(4, 7.0)
    s, ps = _lib.as_c(sent.copy())
    st = np.full(4, 9, dtype=np.int32)
    pst = st.ctypes.data_as(_lib.c_int32_p)
    assert lib.ssmq_filter_smooth_dev(h, ctypes.byref(fd), h, ctypes.byref(fo), 1, 64, 2, p, p, p, None, None, p, p, p, p, p) == -3
    assert lib.ssmq_student_filter_forward_dev(h, ctypes.byref(fd), h, ctypes.byref(fo), 1, 64, 2, p, p, p, None, None, p1, 4.0, p, p, p) == -3
    assert lib.ssmq_filter_forward_aug_dev(h, ctypes.byref(fd), h, ctypes.byref(fo), 1, 1, 64, 2, p, p, p, None, p1, 0, None, p1, 0, p, p, p) == -3
    assert lib.ssmq_filter_forward_piped(h, ctypes.byref(fd), h, ctypes.byref(fo), 1, 2, p1, p1, p1, None, None, ctypes.c_void_p(s.ctypes.data),
                                         ctypes.c_void_p(s.ctypes.data), ctypes.c_void_p(st.ctypes.data), 0, 0) == -3
    assert lib.ssmq_gp_theta_step(h, ctypes.byref(fd), h, ctypes.byref(fo), 1, p1, p1, 1e-8, p1, p1, 1, p1, 1, 0.0, None, None, ps, ps, ps, pst) == -3
    assert lib.ssmq_gp_theta_step_times(h, ctypes.byref(fd), h, ctypes.byref(fo), 1, p1, p1, 1e-8, p1, p1, 1, p1, 1, p1, None, None, ps, ps, ps,
                                        pst) == -3
    assert lib.ssmq_filter_smooth_aug_dev(h, ctypes.byref(fd), h, ctypes.byref(fo), 1, 1, 64, 2, p, p, p, None, p1, 0, None, p1, 0, p, p, p, p,
                                          p) == -3
    assert lib.ssmq_gp_marginal_laplace_batch(h, ctypes.byref(fd), h, ctypes.byref(fo), 1, 1e-8, p1, p1, p1, 0.0, None, None, p1, p1, 1.5e-8,
                                              ps, ps, pst, pst, None) == -3
    assert lib.ssmq_gp_marginal_filter_batch(h, ctypes.byref(fd), h, ctypes.byref(fo), 1, 2, 1e-8, p1, p1, p1, None, None, None, None, p1, p1,
                                             p1, p1, 4, 1.5e-8, 1e-8, ps, ps, pst, None, None, None) == -3
    job = (_lib.FilterJob * 1)()
    job[0].h_dyn, job[0].f_dyn, job[0].h_obs, job[0].f_obs = h.value, ctypes.pointer(fd), h.value, ctypes.pointer(fo)
    job[0].B, job[0].ld, job[0].T = 1, 64, 2
    job[0].d_y = job[0].d_m0 = job[0].d_P0 = buf.ptr
    job[0].d_fm, job[0].d_fP, job[0].d_status = buf.ptr, buf.ptr + 8 * 64, buf.ptr + 8 * 128
    assert lib.ssmq_filter_forward_multi_dev(1, job) == -3
    assert 'multi-output' in _lib.last_error()
    assert np.array_equal(s, sent) and np.all(st == 9)
    buf.free()


def test_optimize_rows_are_the_single_output_fits():
    """E = 3 on Gauss-Hermite degree 15 data (tests/test_ml2_gpu.py): row e of `par` is the single-output model's optimize_batch
    on column e, bit for bit."""
    import ssmtoybox_amd as amd
    from ssmtoybox_amd.bq.bqmod import GaussianProcessMO
    tf0 = amd.GaussianProcessTransform(1, 1, np.array([[1.0, 0.5]]), point_str='gh', point_par={'degree': 15})
    x = tf0.model.points
    Y = np.vstack((np.sin((x + 1) ** -1), np.cos(x), x * np.exp(-0.1 * x ** 2)))          # (3, N)
    lp0 = np.log(np.array([[1.0, 0.5], [1.0, 1.0], [2.0, 0.7]]))
    mo = GaussianProcessMO(1, 3, np.exp(lp0), 'rbf', 'gh', {'degree': 15})
    par, results = mo.optimize(lp0, Y, x)
    ref = tf0.model.optimize_batch(lp0, Y[:, :, None], x)
    assert par.shape == (3, 2) and len(results) == 3
    assert np.array_equal(par, ref['x'])
    assert [r.nit for r in results] == list(ref['nit'])
