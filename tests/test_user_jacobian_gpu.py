"""User models with a device Jacobian on the device: k_linearize_fn / k_taylor_gpqd_fn (compiled at run time) through
LinearizationTransform, TaylorGPQDTransform, ExtendedKalman and ExtendedKalmanGPQD, against the built-in route where a built-in
model is restated and against the NumPy statements of tests/_user_jac_oracle.py.  Batches are B = 193 at ld = 256: neither a
multiple of the wave nor of the block."""
import ctypes

import numpy as np
import pytest

from tests._cases import assert_moments_close, mean_err, cov_err, rel_err
from tests import _user_jac_oracle as uo

pytestmark = pytest.mark.gpu

B, LD, T = 193, 256, 20
BAR = 1e-12                      # the project's bar for these two transforms, of the moment scales
PAR2 = np.array([[1.5, 2.0, 3.5]])
DT, MU = 0.1, 1.0


def inputs(D, seed, spread=1.0):
    rng = np.random.default_rng(seed)
    mean = spread * rng.uniform(-2.0, 2.0, (B, D))
    a = rng.standard_normal((B, D, D)) / np.sqrt(D)
    cov = np.einsum('bij,bkj->bik', a, a) + 0.05 * np.eye(D)
    return mean, cov, rng.integers(0, 20, B).astype(float)


def rv(d, mean=None, cov=None):
    from ssmtoybox_amd import ssmod
    return ssmod.GaussRV(d, mean=mean, cov=cov)


def var_close(got, ref, alpha, what):
    e = float(np.max(np.abs(got - ref))) / max(alpha ** 2, 1.0)
    print('{}: {:.3g}'.format(what, e))
    assert np.all(np.isfinite(got)) and e <= BAR, (what, e)


def both_transforms(D, par):
    import ssmtoybox_amd as amd
    return amd.LinearizationTransform(D), amd.TaylorGPQDTransform(D, par)


_VDP = {}


def vdp_system():
    """The Van der Pol pair, one instance for the tests that share it."""
    if not _VDP:
        VdP = uo.transition('VdP', 2, uo.VDP_CODE, uo.VDP_JAC, (DT, MU))
        VdPMeas = uo.measurement('VdPMeas', 1, uo.VDP_MEAS_CODE, uo.VDP_MEAS_JAC)
        _VDP['dyn'] = VdP(rv(2, mean=np.array([1.0, 0.5]), cov=0.1 * np.eye(2)), rv(2, cov=0.01 * np.eye(2)))
        _VDP['obs'] = VdPMeas(rv(1, cov=np.array([[0.05]])), 2)
    return _VDP['dyn'], _VDP['obs']


def test_a_restated_pendulum_against_the_builtin_route():
    from ssmtoybox_amd import ssmod
    Pend = uo.transition('Pend', 2, uo.PEND_CODE, uo.PEND_JAC, (0.01,))
    PendMeas = uo.measurement('PendMeas', 1, uo.PEND_MEAS_CODE, uo.PEND_MEAS_JAC)
    pairs = ((Pend(rv(2), rv(2)).dyn_eval, ssmod.Pendulum2DTransition(rv(2), rv(2), dt=0.01).dyn_eval),
             (PendMeas(rv(1), 2).meas_eval, ssmod.Pendulum2DMeasurement(rv(1), 2).meas_eval))
    mean, cov, time = inputs(2, 1)
    lin, tg = both_transforms(2, PAR2)
    worst = 0.0
    for user, builtin in pairs:
        assert lin.kernel_name(user).startswith('k_linearize_fn<') and lin.kernel_name(builtin) == 'k_linearize'
        assert tg.kernel_name(user).startswith('k_taylor_gpqd_fn<') and tg.kernel_name(builtin) == 'k_taylor_gpqd'
        got, ref = lin.apply_batch(user, mean, cov, time), lin.apply_batch(builtin, mean, cov, time)
        worst = max(worst, assert_moments_close(got, ref, cov, rtol=BAR, what='linearisation'))
        got = tg.apply_batch(user, mean, cov, time, return_variances=True)
        ref = tg.apply_batch(builtin, mean, cov, time, return_variances=True)
        worst = max(worst, assert_moments_close(got[:3], ref[:3], cov, rtol=BAR, what='Taylor-GPQD'))
        var_close(got[3], ref[3], PAR2[0, 0], 'model_var')
        var_close(got[4], ref[4], PAR2[0, 0], 'integ_var')
    print('restated pendulum against the built-in route, largest difference / moment scale: {:.3g}'.format(worst))


def test_b_van_der_pol_transforms_against_the_oracle():
    dyn, obs = vdp_system()
    mean, cov, time = inputs(2, 2)
    lin, tg = both_transforms(2, PAR2)
    for model_f, f, f_dx in ((dyn.dyn_eval, uo.vdp_f(DT, MU), uo.vdp_dx(DT, MU)), (obs.meas_eval, uo.vdp_meas_f, uo.vdp_meas_dx)):
        e = assert_moments_close(lin.apply_batch(model_f, mean, cov, time),
                                 uo.batch(lambda m, c, t: uo.linearize(f, f_dx, m, c, t), mean, cov, time), cov, rtol=BAR, what='lin')
        got = tg.apply_batch(model_f, mean, cov, time, return_variances=True)
        ref = uo.batch(lambda m, c, t: uo.taylor(f, f_dx, m, c, t, PAR2[0]), mean, cov, time)
        e = max(e, assert_moments_close(got[:3], ref[:3], cov, rtol=BAR, what='tg'))
        var_close(got[3], ref[3], PAR2[0, 0], 'model_var')
        var_close(got[4], ref[4], PAR2[0, 0], 'integ_var')
        print('Van der Pol transforms against the oracle: {:.3g}'.format(e))


def vdp_data(seed=3):
    rng = np.random.default_rng(seed)
    x = np.tile(np.array([1.0, 0.5])[:, None], (1, B)) + 0.3 * rng.standard_normal((2, B))
    y = np.zeros((1, T, B))
    f = uo.vdp_f(DT, MU)
    for k in range(T):
        x = np.stack([f(x[:, b], k) for b in range(B)], axis=1) + 0.1 * rng.standard_normal((2, B))
        y[0, k] = x[0] * x[0] + 0.5 * x[1] + 0.2 * rng.standard_normal(B)
    return y


@pytest.mark.parametrize('gpqd', [False, True])
def test_b_van_der_pol_filters_against_the_oracle(gpqd):
    """ExtendedKalman / ExtendedKalmanGPQD over T = 20, B = 193: 1e-12 on the means (row-scaled), 1e-11 on the covariances
    (entry-scaled).  (h) a second filter on the same pair compiles nothing; (g) the smoother is refused."""
    from ssmtoybox_amd import ssinf, _lib
    dyn, obs = vdp_system()
    y = vdp_data()
    make = (lambda: ssinf.ExtendedKalmanGPQD(dyn, obs, PAR2, PAR2)) if gpqd else (lambda: ssinf.ExtendedKalman(dyn, obs))
    flt = make()
    assert 'hipGraph of 3 T launches' in flt.kernel_name()
    fm, fP = flt.forward_pass_batch(y)
    f, f_dx = uo.vdp_f(DT, MU), uo.vdp_dx(DT, MU)
    if gpqd:
        sd = lambda m, c, t: uo.taylor(f, f_dx, m, c, t, PAR2[0])                            # noqa: E731
        so = lambda m, c, t: uo.taylor(uo.vdp_meas_f, uo.vdp_meas_dx, m, c, t, PAR2[0])      # noqa: E731
    else:
        sd = lambda m, c, t: uo.linearize(f, f_dx, m, c, t)                                  # noqa: E731
        so = lambda m, c, t: uo.linearize(uo.vdp_meas_f, uo.vdp_meas_dx, m, c, t)            # noqa: E731
    rm, rP = uo.ekf(sd, so, y, flt.x0_mean, flt.x0_cov, flt.G.dot(flt.q_cov).dot(flt.G.T), flt.r_cov)
    e_m, e_P = mean_err(fm, rm), cov_err(fP, rP)
    print('{} on Van der Pol against the oracle: mean_err {:.3g}, cov_err {:.3g}'.format(type(flt).__name__, e_m, e_P))
    assert not flt.status.any() and e_m < 1e-12 and e_P < 1e-11, (e_m, e_P)
    # the captured loop replays: the same bits from a second pass, from a second filter (nothing compiled) and from forward_pass
    compiles = _lib.rtc_stats()[0]
    fm2, fP2 = flt.forward_pass_batch(y)
    other = make()
    fm3, fP3 = other.forward_pass_batch(y)
    assert _lib.rtc_stats()[0] == compiles
    assert np.array_equal(fm2, fm) and np.array_equal(fP2, fP) and np.array_equal(fm3, fm) and np.array_equal(fP3, fP)
    fm1, fP1 = flt.forward_pass(y[..., 7])
    assert np.array_equal(fm1, fm[..., 7]) and np.array_equal(fP1, fP[..., 7])
    d_y = _lib.DeviceBuffer(8 * T * LD)
    _lib.upload_study(y, 1, LD, d_y)
    d_fm, d_fP, d_st = flt.forward_pass_dev(d_y, B, LD, T)
    assert np.array_equal(_lib.download_study(d_fm, (2,), T, B, LD), fm) and np.array_equal(_lib.download_study(d_fP, (2, 2), T, B, LD), fP)
    for buf in (d_y, d_fm, d_fP, d_st):
        buf.free()
    flt.forward_pass_batch(y)
    with pytest.raises(NotImplementedError):
        flt.backward_pass_batch()
    with pytest.raises((NotImplementedError, _lib.SsmqError)):       # (refused in Python for the GPQD filter, by the library otherwise)
        ssinf.run_filters([flt], y)


@pytest.mark.parametrize('D,E,DIN', [(3, 2, 3), (6, 4, 5), (6, 6, 6)])
def test_c_shapes_without_a_builtin_body(D, E, DIN):
    code, jac, f, f_dx = uo.poly_model(E, DIN)
    if E == D:
        model_f = uo.transition('Poly{}'.format(D), D, code, jac)(rv(D), rv(D)).dyn_eval
    else:
        model_f = uo.measurement('Poly{}{}'.format(D, E), E, code, jac, dim_substate=DIN if DIN < D else None)(rv(E), D).meas_eval
    fx = lambda x, t: f(x[:DIN], t)              # noqa: E731
    fdx = lambda x, t: f_dx(x[:DIN], t)          # noqa: E731
    mean, cov, time = inputs(D, 10 + D + E, spread=0.6)
    par = np.array([[1.3] + list(np.linspace(1.5, 4.0, D))])
    lin, tg = both_transforms(D, par)
    assert lin.kernel_name(model_f).startswith('k_linearize_fn<') and '{}, {}, {}>'.format(D, E, DIN) in lin.kernel_name(model_f)
    e = assert_moments_close(lin.apply_batch(model_f, mean, cov, time),
                             uo.batch(lambda m, c, t: uo.linearize(fx, fdx, m, c, t), mean, cov, time), cov, rtol=BAR, what='lin')
    got = tg.apply_batch(model_f, mean, cov, time, return_variances=True)
    ref = uo.batch(lambda m, c, t: uo.taylor(fx, fdx, m, c, t, par[0]), mean, cov, time)
    e = max(e, assert_moments_close(got[:3], ref[:3], cov, rtol=BAR, what='tg'))
    var_close(got[3], ref[3], par[0, 0], 'model_var')
    var_close(got[4], ref[4], par[0, 0], 'integ_var')
    print('({}, {}, {}) against the oracle: {:.3g}'.format(D, E, DIN, e))
    # placement: with cov = I the cross-covariance of the linearisation IS the Jacobian - zero behind the DIN leading columns
    jac_dev = lin.apply_batch(model_f, mean, np.tile(np.eye(D), (B, 1, 1)), time)[2]
    assert np.all(jac_dev[:, :, DIN:] == 0.0) and np.all(np.any(jac_dev[:, :, :DIN] != 0.0, axis=(0, 1)))
    # (its entries are cos(x_a) + 0.3 x_b + 0.3 x_c, at most 2 in magnitude on these inputs: 1e-12 of that scale)
    assert np.max(np.abs(jac_dev - np.stack([uo.place(fdx(m, t), D) for m, t in zip(mean, time)]))) <= BAR * 2.0


def test_d_time_reaches_the_jacobian():
    from ssmtoybox_amd import ssinf
    Timed = uo.transition('Timed', 2, uo.TIME_CODE, uo.TIME_JAC, (DT,))
    dyn = Timed(rv(2, mean=np.array([1.0, 0.5]), cov=0.1 * np.eye(2)), rv(2, cov=0.01 * np.eye(2)))
    _, obs = vdp_system()
    f, f_dx = uo.time_f(DT), uo.time_dx(DT)
    mean, cov, time = inputs(2, 4)
    assert len(set(time)) > 5                                              # per-item times: time_stride = 1
    lin, tg = both_transforms(2, PAR2)
    assert_moments_close(lin.apply_batch(dyn.dyn_eval, mean, cov, time),
                         uo.batch(lambda m, c, t: uo.linearize(f, f_dx, m, c, t), mean, cov, time), cov, rtol=BAR, what='lin')
    assert_moments_close(tg.apply_batch(dyn.dyn_eval, mean, cov, time),
                         uo.batch(lambda m, c, t: uo.taylor(f, f_dx, m, c, t, PAR2[0]), mean, cov, time)[:3], cov, rtol=BAR, what='tg')
    # ... and it matters: another time, other moments
    assert not np.allclose(lin.apply_batch(dyn.dyn_eval, mean, cov, time + 1.0)[1], lin.apply_batch(dyn.dyn_eval, mean, cov, time)[1])
    # the filter's step index
    y = vdp_data(5)
    flt = ssinf.ExtendedKalman(dyn, obs)
    fm, fP = flt.forward_pass_batch(y)
    rm, rP = uo.ekf(lambda m, c, t: uo.linearize(f, f_dx, m, c, t), lambda m, c, t: uo.linearize(uo.vdp_meas_f, uo.vdp_meas_dx, m, c, t),
                    y, flt.x0_mean, flt.x0_cov, flt.G.dot(flt.q_cov).dot(flt.G.T), flt.r_cov)
    e_m, e_P = mean_err(fm, rm), cov_err(fP, rP)
    print('timed model, ExtendedKalman against the oracle: mean_err {:.3g}, cov_err {:.3g}'.format(e_m, e_P))
    assert e_m < 1e-12 and e_P < 1e-11, (e_m, e_P)


@pytest.mark.parametrize('user_side', ['dyn', 'obs'])
def test_e_mixed_pairs_with_the_builtin_ungm_models(user_side):
    """A user model next to a built-in one that has a Jacobian (UNGM's transition reads the built-in time table).  The bar is the one
    the project holds ExtendedKalman on UNGM to (tests/test_gpu_parity.py::test_extended_kalman_golden: 1e-9 norm-wise - UNGM's
    recursion amplifies rounding differences, which is why that test does not use the launch-loop bars)."""
    from ssmtoybox_amd import ssinf, ssmod
    x0, q, r = rv(1, cov=np.array([[1.0]])), rv(1, cov=np.array([[10.0]])), rv(1, cov=np.array([[1.0]]))
    if user_side == 'dyn':
        dyn, obs = uo.transition('SDyn', 1, uo.S_DYN_CODE, uo.S_DYN_JAC)(x0, q), ssmod.UNGMMeasurement(r, 1)
        fd, hd = (uo.s_dyn_f, uo.s_dyn_dx), (uo.ungm_meas_f, uo.ungm_meas_dx)
    else:
        dyn, obs = ssmod.UNGMTransition(x0, q), uo.measurement('SMeas', 1, uo.S_MEAS_CODE, uo.S_MEAS_JAC)(r, 1)
        fd, hd = (uo.ungm_f, uo.ungm_dx), (uo.s_meas_f, uo.s_meas_dx)
    rng = np.random.default_rng(6)
    y = 2.0 + 3.0 * rng.standard_normal((1, T, B))
    flt = ssinf.ExtendedKalman(dyn, obs)
    fm, fP = flt.forward_pass_batch(y)
    rm, rP = uo.ekf(lambda m, c, t: uo.linearize(fd[0], fd[1], m, c, t), lambda m, c, t: uo.linearize(hd[0], hd[1], m, c, t),
                    y, flt.x0_mean, flt.x0_cov, flt.G.dot(flt.q_cov).dot(flt.G.T), flt.r_cov)
    e_m, e_P = rel_err(fm, rm), rel_err(fP, rP)
    print('mixed pair (user {}): means {:.3g}, covariances {:.3g}'.format(user_side, e_m, e_P))
    assert not flt.status.any() and e_m < 1e-9 and e_P < 1e-9, (e_m, e_P)


def test_f_indefinite_covariance_marks_its_item_alone():
    dyn, _ = vdp_system()
    mean, cov, time = inputs(2, 7)
    _, tg = both_transforms(2, PAR2)
    good = tg.apply_batch(dyn.dyn_eval, mean, cov, time, return_status=True, return_variances=True)
    bad = cov.copy()
    bad[100] = -100.0 * np.eye(2)
    out = tg.apply_batch(dyn.dyn_eval, mean, bad, time, return_status=True, return_variances=True)
    st = out[3]
    assert st[100] == 1 and st.sum() == 1
    keep = np.arange(B) != 100
    for a, g in zip(out[:3] + out[4:], good[:3] + good[4:]):
        assert np.all(np.isnan(a[100])) and np.array_equal(a[keep], g[keep])


def test_g_padding_lanes_and_refused_calls_leave_their_buffers():
    from ssmtoybox_amd import _lib, ssinf
    dyn, obs = vdp_system()
    mean, cov, time = inputs(2, 8)
    lin, tg = both_transforms(2, PAR2)
    sent = 7.25
    for tf in (lin, tg):
        d_m, d_c = _lib.SoA.from_host(mean, ld=LD), _lib.SoA.from_host(cov, ld=LD)
        d_t = _lib.DeviceBuffer(8 * B)
        d_t.upload(time)
        outs = [_lib.SoA(k, B, ld=LD) for k in (2, 4, 4)]
        extra = [_lib.DeviceBuffer(8 * LD), _lib.DeviceBuffer(8 * LD)] if tf is tg else []
        d_st = _lib.DeviceBuffer(4 * LD)
        for o in outs:
            o.buf.upload(np.full(o.n * LD, sent))
        for e in extra:
            e.upload(np.full(LD, sent))
        d_st.upload(np.full(LD, 77, dtype=np.int32))
        kw = dict(model_var=extra[0], integ_var=extra[1]) if extra else {}
        tf.apply_batch_dev(dyn.dyn_eval, d_m, d_c, d_t, outs[0], outs[1], outs[2], d_st, time_stride=1, **kw)
        _lib.sync()
        planes = [o.buf.download((o.n, LD)) for o in outs] + [e.download((1, LD)) for e in extra]
        st = d_st.download((LD,), dtype=np.int32)
        for buf in [d_m.buf, d_c.buf, d_t, d_st] + [o.buf for o in outs] + extra:
            buf.free()
        assert np.all(st[:B] == 0) and np.all(st[B:] == 77)
        host = tf.apply_batch(dyn.dyn_eval, mean, cov, time, **(dict(return_variances=True) if extra else {}))
        for p, h in zip(planes, host):
            assert np.all(p[:, B:] == sent), 'padding lanes untouched'
            assert np.array_equal(p[:, :B], h.reshape(B, -1).T)
    # the smoother with this pair: SSMQ_E_UNSUPPORTED before any output is touched
    lib = _lib.load()
    flt = ssinf.ExtendedKalman(dyn, obs)
    f_dyn, e_dyn = dyn.device_integrand()
    f_obs, e_obs = obs.device_integrand()
    h_dyn, h_obs = flt.tf_dyn._handle_for(e_dyn), flt.tf_obs._handle_for(e_obs)
    Bs, Ts, ld = 8, 5, 64
    sentinel = np.full((Ts * 4, ld), sent)
    bufs = [_lib.DeviceBuffer(sentinel.nbytes) for _ in range(7)]
    for b in bufs:
        b.upload(sentinel)
    d_y, d_m0, d_P0, d_fm, d_fP, d_sm, d_sP = bufs
    d_st = _lib.DeviceBuffer(4 * ld)
    d_st.upload(np.full(ld, 5, dtype=np.int32))
    gqg, pg = _lib.as_c(np.eye(2))
    rr, pr = _lib.as_c(np.eye(1))
    rc = lib.ssmq_filter_smooth_dev(ctypes.c_void_p(h_dyn), ctypes.byref(f_dyn), ctypes.c_void_p(h_obs), ctypes.byref(f_obs), Bs, ld, Ts,
                                    ctypes.c_void_p(d_y.ptr), ctypes.c_void_p(d_m0.ptr), ctypes.c_void_p(d_P0.ptr), pg, pr,
                                    ctypes.c_void_p(d_fm.ptr), ctypes.c_void_p(d_fP.ptr), ctypes.c_void_p(d_sm.ptr),
                                    ctypes.c_void_p(d_sP.ptr), ctypes.c_void_p(d_st.ptr))
    assert rc == -3 and 'user-defined integrands' in _lib.last_error()
    _lib.sync()
    for b in (d_fm, d_fP, d_sm, d_sP):
        assert np.array_equal(b.download(sentinel.shape), sentinel)
    assert np.array_equal(d_st.download((ld,), dtype=np.int32), np.full(ld, 5, dtype=np.int32))
    for b in bufs + [d_st]:
        b.free()


def test_i_check_jacobian():
    """Rounding of the central difference is ~1e-11 at the step 1e-5 and its truncation ~1e-11: five orders of margin either way."""
    dyn, obs = vdp_system()
    rng = np.random.default_rng(9)
    pts = rng.uniform(-2.0, 2.0, (B, 2))
    dev = dyn.check_jacobian(pts)
    assert dev.shape == (B,) and np.all(dev < 1e-6), dev.max()
    assert np.all(obs.check_jacobian(pts) < 1e-6)
    Flipped = uo.transition('Flipped', 2, uo.VDP_CODE, uo.VDP_JAC_FLIPPED, (DT, MU))
    wrong = Flipped(rv(2), rv(2)).check_jacobian(pts)
    entry = np.abs(DT * (-2.0 * MU * pts[:, 0] * pts[:, 1] - 1.0))            # |d o_1 / d x_0|; the deviation is twice that
    assert np.any(entry >= 0.1) and np.all(wrong[entry >= 0.1] > 1e-2)
    # a built-in model that has a Jacobian
    from ssmtoybox_amd import ssmod
    assert np.all(ssmod.Pendulum2DTransition(rv(2), rv(2), dt=0.01).check_jacobian(pts) < 1e-6)
