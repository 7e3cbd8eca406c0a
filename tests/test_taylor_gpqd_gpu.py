"""Taylor-GPQD transform (k_taylor_gpqd) and ExtendedKalmanGPQD on the device against tests/golden/g21_taylor_gpqd.npz (the
reference's TaylorGPQDTransform and its filter on UNGM), the NumPy restatement of tests/_taylor_oracle.py and the linearisation
transform."""
import ctypes

import numpy as np
import pytest

from tests._cases import assert_moments_close, rel_err, mean_err, cov_err, within
from tests import _taylor_oracle as to
from tests._jacobian_cases import package_models, index_cases

pytestmark = pytest.mark.gpu

LINEAR_BAR = 1e-12        # tests/test_gpu_parity.py::test_linearization_transform_golden: k_linearize against the reference
VAR_BAR = 1e-12


@pytest.fixture(scope='module')
def g21(golden):
    return golden('g21_taylor_gpqd')


_TF = {}


def transform(g, tag, row):
    """One transform per (block, parameter row), shared by the tests."""
    import ssmtoybox_amd as amd
    if (tag, row) not in _TF:
        _TF[(tag, row)] = (amd.TaylorGPQDTransform(to.CASES[tag][2], g[tag + '_par'][row:row + 1]), package_models()[tag])
    return _TF[(tag, row)]


def var_close(got, ref, alpha, what):
    """model_var = alpha^2 - alpha^2 wc (1 + tr) and integ_var = alpha^2 wc - wm^2 are differences of terms of the size alpha^2 and
    wm^2 <= 1: 1e-12 relative to those terms (with ell = 1e3 the differences themselves are 1e-6 of them and carry, in the
    reference as here, the rounding of the terms)."""
    scale = max(alpha ** 2, 1.0)
    e = float(np.max(np.abs(got - ref))) / scale
    print('{}: {:.3g}'.format(what, e))
    assert np.all(np.isfinite(got)) and e <= VAR_BAR, (what, e)


@pytest.mark.parametrize('tag', list(to.CASES))
def test_apply_batch_against_the_reference(g21, monkeypatch, tag):
    """Every block and parameter row through the compile-time kernel and through the run-time-size one (SSMQ_TAYLOR_GPQD_GENERIC)."""
    mean, cov, time = g21[tag + '_mean'], g21[tag + '_cov'], g21[tag + '_time']
    for r in range(to.N_PAR):
        tf, f = transform(g21, tag, r)
        assert tf.kernel_name(f) == 'k_taylor_gpqd'
        ref = tuple(g21[tag + '_' + k][r] for k in ('mf', 'cf', 'cfx'))
        out = {}
        for route in ('shape', 'generic'):
            if route == 'generic':
                monkeypatch.setenv('SSMQ_TAYLOR_GPQD_GENERIC', '1')
            else:
                monkeypatch.delenv('SSMQ_TAYLOR_GPQD_GENERIC', raising=False)
            mf, cf, cfx, st, mv, iv = tf.apply_batch(f, mean, cov, time, return_status=True, return_variances=True)
            assert not st.any()
            e = assert_moments_close((mf, cf, cfx), ref, cov, rtol=LINEAR_BAR, what=(tag, r, route))
            print('{} row {} {}: {:.3g}'.format(tag, r, route, e))
            alpha = g21[tag + '_par'][r, 0]
            var_close(mv, g21[tag + '_mvar'][r], alpha, '{} row {} {} model_var'.format(tag, r, route))
            var_close(iv, g21[tag + '_ivar'][r], alpha, '{} row {} {} integ_var'.format(tag, r, route))
            out[route] = (mf, cf, cfx, mv, iv)
        monkeypatch.delenv('SSMQ_TAYLOR_GPQD_GENERIC', raising=False)
        assert_moments_close(out['generic'][:3], out['shape'][:3], cov, rtol=LINEAR_BAR, what=(tag, r, 'generic against shape'))
        var_close(out['generic'][3], out['shape'][3], alpha, '{} row {} generic against shape model_var'.format(tag, r))
        var_close(out['generic'][4], out['shape'][4], alpha, '{} row {} generic against shape integ_var'.format(tag, r))


@pytest.mark.parametrize('tag', ['ungm_dyn', 'pend_meas', 'pend_dyn', 'cv_dyn'])
def test_plane_addressing_and_padding(g21, tag):
    """B = 70 at ld = 128: two waves and a ragged tail.  Item b is item b mod 8 bit for bit; the padding lanes of every output
    plane keep the sentinel written beforehand."""
    from ssmtoybox_amd import _lib
    tf, f = transform(g21, tag, 1)
    _, _, D, E, _ = to.CASES[tag]
    B, ld, n = 70, 128, to.N_ITEMS
    idx = np.arange(B) % n
    mean, cov, time = g21[tag + '_mean'][idx], g21[tag + '_cov'][idx], g21[tag + '_time'][idx]
    d_m, d_c = _lib.SoA.from_host(mean, ld=ld), _lib.SoA.from_host(cov, ld=ld)
    d_t = _lib.DeviceBuffer(8 * B)
    d_t.upload(time)
    sent = 7.25
    outs = [_lib.SoA(k, B, ld=ld) for k in (E, E * E, E * D)]
    d_mv, d_iv, d_st = _lib.DeviceBuffer(8 * ld), _lib.DeviceBuffer(8 * ld), _lib.DeviceBuffer(4 * ld)
    for o in outs:
        o.buf.upload(np.full(o.n * ld, sent))
    d_mv.upload(np.full(ld, sent))
    d_iv.upload(np.full(ld, sent))
    d_st.upload(np.full(ld, 77, dtype=np.int32))
    tf.apply_batch_dev(f, d_m, d_c, d_t, outs[0], outs[1], outs[2], d_st, time_stride=1, model_var=d_mv, integ_var=d_iv)
    _lib.sync()
    planes = [o.buf.download((o.n, ld)) for o in outs] + [d_mv.download((1, ld)), d_iv.download((1, ld))]
    st = d_st.download((ld,), dtype=np.int32)
    for buf in [d_m.buf, d_c.buf, d_t, d_mv, d_iv, d_st] + [o.buf for o in outs]:
        buf.free()
    assert np.all(st[:B] == 0) and np.all(st[B:] == 77)
    mf8, cf8, cfx8, mv8, iv8 = tf.apply_batch(f, g21[tag + '_mean'], g21[tag + '_cov'], g21[tag + '_time'], return_variances=True)
    first = [mf8.reshape(n, -1).T, cf8.reshape(n, -1).T, cfx8.reshape(n, -1).T, mv8[None, :], iv8[None, :]]
    for p, f8 in zip(planes, first):
        assert np.all(np.isfinite(p[:, :B]))
        assert np.all(p[:, B:] == sent), 'padding lanes untouched'
        assert np.array_equal(p[:, :B], p[:, idx]), 'item b is item b mod 8'
        assert np.array_equal(p[:, :n], f8), 'the batch of 8 through apply_batch'


@pytest.mark.parametrize('tag', ['pend_meas_idx1', 'ungmna_meas_idx20'])
def test_state_index_against_the_oracle(monkeypatch, tag):
    """The model reached through a state index: inputs gathered by it, the Jacobian placed by it.  B = 193 at ld = 256 (four
    blocks' worth of lanes in one, a ragged tail), inputs as g21's (cov = A A' + 0.2 I, ell in [0.5, 5], alpha 1 and 2.5), as
    routed and through the run-time-size body, against tests/_taylor_oracle.taylor_gpqd with J placed by the index; the bars of
    test_apply_batch_against_the_reference.  The padding lanes of every output plane keep their sentinel."""
    import ssmtoybox_amd as amd
    from ssmtoybox_amd import _lib
    from oracle import ssmq_oracle as orc
    mod, fid, D, idx = index_cases()[tag]
    f, E = mod.meas_eval, 1
    B, ld, sent = 193, 256, 7.25
    rng = np.random.default_rng(22)
    mean = rng.standard_normal((B, D))
    a = rng.standard_normal((B, D, D))
    cov = np.einsum('bij,bkj->bik', a, a) + 0.2 * np.eye(D)
    d_m, d_c = _lib.SoA.from_host(mean, ld=ld), _lib.SoA.from_host(cov, ld=ld)
    d_t = _lib.DeviceBuffer(8)
    d_t.upload(np.zeros(1))
    outs = [_lib.SoA(k, B, ld=ld) for k in (E, E * E, E * D)]
    d_mv, d_iv, d_st = _lib.DeviceBuffer(8 * ld), _lib.DeviceBuffer(8 * ld), _lib.DeviceBuffer(4 * ld)
    try:
        for alpha in (1.0, 2.5):
            ell = rng.uniform(0.5, 5.0, D)
            tf = amd.TaylorGPQDTransform(D, np.hstack(([alpha], ell))[None, :])
            assert tf.kernel_name(f) == 'k_taylor_gpqd'
            ref = [np.zeros((B, E)), np.zeros((B, E, E)), np.zeros((B, E, D)), np.zeros(B), np.zeros(B)]
            for i in range(B):
                xs = mean[i][idx]
                J = np.zeros((E, D))
                J[:, idx] = orc.jacobian(fid, xs, 0.0)
                for r, v in zip(ref, to.taylor_gpqd(np.atleast_1d(orc.integrand(fid, xs, 0.0)), J, cov[i], alpha, ell)):
                    r[i] = v
            for route in ('shape', 'generic'):
                if route == 'generic':
                    monkeypatch.setenv('SSMQ_TAYLOR_GPQD_GENERIC', '1')
                else:
                    monkeypatch.delenv('SSMQ_TAYLOR_GPQD_GENERIC', raising=False)
                for o in outs:
                    o.buf.upload(np.full(o.n * ld, sent))
                d_mv.upload(np.full(ld, sent))
                d_iv.upload(np.full(ld, sent))
                d_st.upload(np.full(ld, 77, dtype=np.int32))
                tf.apply_batch_dev(f, d_m, d_c, d_t, outs[0], outs[1], outs[2], d_st, time_stride=0, model_var=d_mv, integ_var=d_iv)
                _lib.sync()
                planes = [o.buf.download((o.n, ld)) for o in outs] + [d_mv.download((1, ld)), d_iv.download((1, ld))]
                st = d_st.download((ld,), dtype=np.int32)
                assert np.all(st[:B] == 0) and np.all(st[B:] == 77)
                for p in planes:
                    assert np.all(p[:, B:] == sent), 'padding lanes untouched'
                mf, cf, cfx = planes[0][:, :B].T, planes[1][:, :B].T.reshape(B, E, E), planes[2][:, :B].T.reshape(B, E, D)
                what = (tag, alpha, route)
                e = assert_moments_close((mf, cf, cfx), ref[:3], cov, rtol=LINEAR_BAR, what=what)
                print('{} alpha {} {}: {:.3g}'.format(tag, alpha, route, e))
                var_close(planes[3][0, :B], ref[3], alpha, '{} model_var'.format(what))
                var_close(planes[4][0, :B], ref[4], alpha, '{} integ_var'.format(what))
    finally:
        for buf in [d_m.buf, d_c.buf, d_t, d_mv, d_iv, d_st] + [o.buf for o in outs]:
            buf.free()


@pytest.mark.parametrize('tag', ['pend_dyn', 'cv_dyn'])
def test_apply_is_row_zero_and_an_indefinite_covariance_marks_its_item(g21, tag):
    import ssmtoybox_amd as amd
    f = package_models()[tag]
    tf = amd.TaylorGPQDTransform(to.CASES[tag][2], g21[tag + '_par'][:1])
    mean, cov, time = g21[tag + '_mean'], g21[tag + '_cov'], g21[tag + '_time']
    mf, cf, cfx, st, mv, iv = tf.apply_batch(f, mean, cov, time, return_status=True, return_variances=True)
    assert tf.mvar_list == [] and tf.ivar_list == []
    one = tf.apply(f, mean[0], cov[0], np.atleast_1d(time[0]))
    assert np.array_equal(one[0], mf[0]) and np.array_equal(one[1], cf[0]) and np.array_equal(one[2], cfx[0])
    assert tf.mvar_list == [mv[0]] and tf.ivar_list == [iv[0]]
    tf.apply(f, mean[1], cov[1], np.atleast_1d(time[1]))
    assert tf.mvar_list == [mv[0], mv[1]] and tf.ivar_list == [iv[0], iv[1]]
    bad = cov.copy()
    bad[3] = -100.0 * np.eye(cov.shape[1])          # Lam / 2 + P has negative pivots for every ell <= 5
    mf2, cf2, cfx2, st2, mv2, iv2 = tf.apply_batch(f, mean, bad, time, return_status=True, return_variances=True)
    assert st2[3] == 1 and st2.sum() == 1
    assert np.all(np.isnan(mf2[3])) and np.all(np.isnan(cf2[3])) and np.all(np.isnan(cfx2[3])) and np.isnan(mv2[3]) and np.isnan(iv2[3])
    keep = np.arange(mean.shape[0]) != 3
    for a, b in ((mf2, mf), (cf2, cf), (cfx2, cfx), (mv2, mv), (iv2, iv)):
        assert np.array_equal(a[keep], b[keep])
    with pytest.raises(np.linalg.LinAlgError):
        tf.apply(f, mean[3], bad[3], np.atleast_1d(time[3]))
    with pytest.raises(np.linalg.LinAlgError):
        tf.apply_batch(f, mean, bad, time)


@pytest.mark.parametrize('tag', list(to.CASES))
def test_long_length_scales_give_the_linearisation_transform(g21, tag):
    """ell = 1e3 against LinearizationTransform.apply_batch on the same inputs, within the bound of the host test."""
    import ssmtoybox_amd as amd
    fid, p, D, E, _ = to.CASES[tag]
    tf, f = transform(g21, tag, to.LIMIT_ROW)
    par = g21[tag + '_par'][to.LIMIT_ROW]
    mean, cov, time = g21[tag + '_mean'], g21[tag + '_cov'], g21[tag + '_time']
    got = tf.apply_batch(f, mean, cov, time)
    lin = amd.LinearizationTransform(D).apply_batch(f, mean, cov, time)
    for i in range(to.N_ITEMS):
        fm, J = to.value_and_jacobian(fid, mean[i], time[i], p)
        bounds = to.limit_bound(fm, J, cov[i], par[0], par[1:])
        for a, b, bound, what in zip(got, lin, bounds, ('mean', 'cov', 'ccov')):
            assert np.max(np.abs(a[i] - b[i])) <= bound, (tag, i, what)


def test_filter_on_ungm_against_the_reference(g21):
    """ExtendedKalmanGPQD.forward_pass_batch (T = 20, B = 4) against the reference's filter; the bars of the ExtendedKalman golden
    test (tests/test_gpu_parity.py::test_extended_kalman_golden: 1e-9 on the norm-wise relative error of means and covariances)."""
    from ssmtoybox_amd import ssinf, ssmod as sm
    dyn = sm.UNGMTransition(sm.GaussRV(1), sm.GaussRV(1, cov=np.array([[10.0]])))
    obs = sm.UNGMMeasurement(sm.GaussRV(1), 1)
    flt = ssinf.ExtendedKalmanGPQD(dyn, obs, g21['ekf_ungm_par_dyn'], g21['ekf_ungm_par_obs'])
    assert 'hipGraph of 3 T launches' in flt.kernel_name()
    y = g21['ekf_ungm_y']
    assert y.shape == (1, 20, 4)
    fm, fP = flt.forward_pass_batch(y)
    e_m, e_P = rel_err(fm, g21['ekf_ungm_fm']), rel_err(fP, g21['ekf_ungm_fc'])
    print('EKF-GPQD on UNGM against the reference: means {:.3g}, covariances {:.3g}'.format(e_m, e_P))
    assert within(e_m, 1e-9, 'EKF-GPQD ungm filtered means vs the reference')
    assert within(e_P, 1e-9, 'EKF-GPQD ungm filtered covariances vs the reference')


def host_recursion(flt, y):
    """The filter's recursion stepped on the host: the transforms' own apply_batch per step and the oracle's Kalman update (the
    pattern of tests/test_multi_output_gpu.py)."""
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
            m[b], P[b] = to.kalman_update(mp[b], Pp[b], ym[b], Py[b], Pyx[b], y[:, k, b])
        fm[:, k], fP[:, :, k] = m.T, P.transpose(1, 2, 0)
    return fm, fP


def test_filter_on_the_pendulum_against_the_host_recursion():
    """dim_y = 1, dim_state = 2 - where the reference's filter cannot run.  T = 20, B = 8; bars of the launch-loop parity tests
    (row-scaled mean error 1e-12, entry-scaled covariance error 1e-11)."""
    from ssmtoybox_amd import ssinf, ssmod as sm, _lib
    rng = np.random.default_rng(21)
    T, B = 20, 8
    dyn = sm.Pendulum2DTransition(sm.GaussRV(2, mean=np.array([1.5, 0.0]), cov=0.01 * np.eye(2)), sm.GaussRV(2, cov=1e-3 * np.eye(2)), dt=0.01)
    obs = sm.Pendulum2DMeasurement(sm.GaussRV(1, cov=np.array([[0.1]])), 2)
    y = np.sin(1.5) + 0.3 * rng.standard_normal((1, T, B))
    flt = ssinf.ExtendedKalmanGPQD(dyn, obs, np.array([[1.0, 3.0, 2.0]]), np.array([[2.5, 1.5, 4.0]]))
    assert 'hipGraph of 3 T launches' in flt.kernel_name()
    assert flt.tf_dyn.kernel_name(dyn.dyn_eval) == 'k_taylor_gpqd' and flt.tf_obs.kernel_name(obs.meas_eval) == 'k_taylor_gpqd'
    fm, fP = flt.forward_pass_batch(y)
    rm, rP = host_recursion(flt, y)
    e_m, e_P = mean_err(fm, rm), cov_err(fP, rP)
    print('EKF-GPQD on the pendulum against the host recursion: mean_err {:.3g}, cov_err {:.3g}'.format(e_m, e_P))
    assert e_m < 1e-12 and e_P < 1e-11, (e_m, e_P)
    # the RTS smoother, where ExtendedKalman has it: the same forward pass, and the reference's indexing (the last two steps stay)
    sm_, sP = flt.backward_pass_batch()
    assert np.array_equal(flt.fi_mean, fm) and np.all(np.isfinite(sm_)) and np.all(np.isfinite(sP))
    assert np.array_equal(sm_[:, -2:], fm[:, -2:]) and not np.array_equal(sm_[:, :-2], fm[:, :-2])
    fm1, fP1 = flt.forward_pass(y[..., 0])
    assert np.array_equal(fm1, fm[..., 0]) and np.array_equal(fP1, fP[..., 0])
    ld = 64
    d_y = _lib.DeviceBuffer(8 * T * ld)
    _lib.upload_study(y, 1, ld, d_y)
    d_fm, d_fP, d_st = flt.forward_pass_dev(d_y, B, ld, T)
    assert np.array_equal(_lib.download_study(d_fm, (2,), T, B, ld), fm)
    assert np.array_equal(_lib.download_study(d_fP, (2, 2), T, B, ld), fP)
    for buf in (d_y, d_fm, d_fP, d_st):
        buf.free()
    with pytest.raises(NotImplementedError):
        ssinf.run_filters([flt], y)


def test_refusals_through_the_c_abi(g21):
    """SSMQ_E_UNSUPPORTED (-3) with the output sentinels intact: a user integrand, a model without a Jacobian, the new handle in
    ssmq_filter_forward_multi_dev - and the other entry points that cannot run the form."""
    from ssmtoybox_amd import _lib, ssmod as sm
    lib = _lib.load()
    ell, pe = _lib.as_c(np.array([2.0, 3.0, 1.0, 1.0, 1.0]))
    fd, _ = sm.UNGMTransition().device_integrand()
    fo, _ = sm.UNGMMeasurement(sm.GaussRV(1), 1).device_integrand()
    # creation: SSMQ_E_ARG semantics (a null handle and a message)
    for D, E, alpha, arr in ((17, 1, 1.0, np.ones(17)), (2, 2, np.nan, np.ones(2)), (2, 2, 1.0, np.array([1.0, 0.0])), (2, 2, 1.0, np.array([1.0, np.inf]))):
        a, pa = _lib.as_c(arr)
        assert not lib.ssmq_transform_create_taylor_gpqd(D, E, alpha, pa)
        assert 'taylor_gpqd' in _lib.last_error()
    sent = 7.0
    outs = [np.full(64, sent) for _ in range(3)]
    po = [o.ctypes.data_as(_lib.c_double_p) for o in outs]
    st = np.full(4, 9, dtype=np.int32)
    pst = st.ctypes.data_as(_lib.c_int32_p)
    one, p1 = _lib.as_c(np.ones(32))

    class UserMap(sm.TransitionModel):
        dim_state, dim_noise, noise_additive = 2, 2, True
        device_code = 'o[0] = x[0] + 0.01 * x[1]; o[1] = x[1] - 0.0981 * sin(x[0]);'
    fu, _ = UserMap(sm.GaussRV(2), sm.GaussRV(2)).device_integrand()
    h2 = ctypes.c_void_p(lib.ssmq_transform_create_taylor_gpqd(2, 2, 1.0, pe))
    assert lib.ssmq_apply_batch(h2, ctypes.byref(fu), 1, p1, p1, p1, 0, po[0], po[1], po[2], pst) == -3
    assert 'user' in _lib.last_error()
    fr, _ = sm.ReentryVehicle2DTransition(sm.GaussRV(5, cov=np.eye(5)), sm.GaussRV(3, cov=np.eye(3))).device_integrand()
    h5 = ctypes.c_void_p(lib.ssmq_transform_create_taylor_gpqd(5, 5, 1.0, pe))
    eye5, p5 = _lib.as_c(np.eye(5))
    assert lib.ssmq_apply_batch(h5, ctypes.byref(fr), 1, p1, p5, p1, 0, po[0], po[1], po[2], pst) == -3
    assert 'no Jacobian' in _lib.last_error()
    h = ctypes.c_void_p(lib.ssmq_transform_create_taylor_gpqd(1, 1, 1.0, pe))
    buf = _lib.DeviceBuffer(8 * 64 * 64)
    buf.upload(np.full(64 * 64, sent))
    job = (_lib.FilterJob * 1)()
    job[0].h_dyn, job[0].f_dyn, job[0].h_obs, job[0].f_obs = h.value, ctypes.pointer(fd), h.value, ctypes.pointer(fo)
    job[0].B, job[0].ld, job[0].T = 1, 64, 2
    job[0].d_y = job[0].d_m0 = job[0].d_P0 = buf.ptr
    job[0].d_fm, job[0].d_fP, job[0].d_status = buf.ptr + 8 * 256, buf.ptr + 8 * 512, buf.ptr + 8 * 1024
    assert lib.ssmq_filter_forward_multi_dev(1, job) == -3
    assert 'Taylor-GPQD' in _lib.last_error()
    # the others: sigma points, constants, time blocks, the theta-step, the marginalised filter
    assert lib.ssmq_transform_update(h, None, p1, None, None, None, 0, 0.0, None) == -3
    assert lib.ssmq_transform_update_mo(h, None, p1, None, None, None, 0.0, None) == -3
    assert lib.ssmq_fxwc_batch_dev(h, 0, None, 0, None, 0, None) == -3
    assert lib.ssmq_sigma_points_batch(h, 1, p1, p1, po[0], po[1], pst) == -3
    assert lib.ssmq_apply_fx_batch(h, 1, p1, p1, p1, p1, po[0], po[1], po[2]) == -3
    assert lib.ssmq_filter_forward_piped(h, ctypes.byref(fd), h, ctypes.byref(fo), 1, 2, p1, p1, p1, None, None, ctypes.c_void_p(outs[0].ctypes.data),
                                         ctypes.c_void_p(outs[1].ctypes.data), ctypes.c_void_p(st.ctypes.data), 0, 0) == -3
    assert lib.ssmq_gp_theta_step(h, ctypes.byref(fd), h, ctypes.byref(fo), 1, p1, p1, 1e-8, p1, p1, 1, p1, 1, 0.0, None, None, po[0], po[1], po[2],
                                  pst) == -3
    assert lib.ssmq_gp_theta_step_times(h, ctypes.byref(fd), h, ctypes.byref(fo), 1, p1, p1, 1e-8, p1, p1, 1, p1, 1, p1, None, None, po[0], po[1],
                                        po[2], pst) == -3
    assert lib.ssmq_gp_marginal_laplace_batch(h, ctypes.byref(fd), h, ctypes.byref(fo), 1, 1e-8, p1, p1, p1, 0.0, None, None, p1, p1, 1.5e-8,
                                              po[0], po[1], pst, pst, None) == -3
    assert lib.ssmq_gp_marginal_filter_batch(h, ctypes.byref(fd), h, ctypes.byref(fo), 1, 2, 1e-8, p1, p1, p1, None, None, None, None, p1, p1,
                                             p1, p1, 4, 1.5e-8, 1e-8, po[0], po[1], pst, None, None, None) == -3
    assert lib.ssmq_taylor_gpqd_variance_planes(None, None, None) == -1
    assert all(np.all(o == sent) for o in outs) and np.all(st == 9)
    assert np.all(buf.download((64 * 64,)) == sent)
    buf.free()
    for hh in (h, h2, h5):
        lib.ssmq_transform_destroy(hh)
