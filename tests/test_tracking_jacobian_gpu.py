"""The device Jacobians of the coordinated turn, the radar and the bearing measurements (csrc/ssmq_device.h: jac_integrand) and
what runs on them: k_linearize at the new register-resident shapes and at the run-time sizes, check_jacobian, k_ekf_loop at
(4, 2), (4, 4), (5, 2), (5, 4) against the launch loop and the NumPy recursion, the smoother, a failing trajectory, run_filters, the
Taylor-GPQD transform and the posterior Cramer-Rao bound.  B = 193 trajectories on planes of pitch 256, as tests/test_ekf_loop_gpu.py.

Jacobian entries: |err| <= K eps S against the 50-digit oracle (tests/_tracking_jac_oracle.py), S the sum of the absolute values of
the terms of the entry's formula, K = max(8, 4 x the worst ratio of the NumPy fp64 statement on the same points).  Measured on the
CPU: NumPy 5.31 (coordinated turn), 0.98 (radar), 1.63 (bearings), so K = 21.3, 8, 8.  The factor 4 is margin for the device's
division, reciprocal-square-root and sincos sequences, a few ulp from the correctly rounded host functions: a judgment, not a
measurement.  The device, measured on an MI355X by test_1 (which prints them), register-resident and run-time-size bodies alike:
5.31 (coordinated turn), 2.34 (radar), 1.63 (bearings).

Filter bars: MEAN_BAR = 1e-12, COV_BAR = 1e-11 (tests/_cases.py scalings) where the NumPy fp64 recursion, compared on the CPU with
the same recursion in np.longdouble on the same data, stays inside a quarter of them; else 4 x that error (host(): computed
from the two host runs, never from the device's output).  The referee needs the x87 format (64-bit mantissa, 2048 times finer than
fp64; asserted below): both runs amplify rounding alike, so their difference is the fp64 run's error to one part in 2048.  These
bars hold the device against the NumPy recursion.  k_ekf_loop against the launch loop - the same arithmetic on the same device -
is held to the project's fixed MEAN_BAR / COV_BAR whatever the set-up."""
import numpy as np
import pytest

from tests._cases import mean_err, cov_err, assert_moments_close, RTOL
from tests import _tracking_jac_oracle as tj

pytestmark = pytest.mark.gpu
assert np.finfo(np.longdouble).nmant >= 63, 'the extended-precision referee of host() needs a long double wider than fp64'

B, LD = 193, 256
MEAN_BAR, COV_BAR = 1e-12, 1e-11
LINEAR_BAR = 1e-12        # tests/test_taylor_gpqd_gpu.py
M0 = np.array([1000.0, 300.0, 1000.0, 0.0, np.deg2rad(-3.0)])
P0 = np.diag([100.0, 10.0, 100.0, 10.0, 0.1])


def ct_q():
    dt, rho_1, rho_2 = tj.DT, 0.1, 1.75e-4
    A = np.array([[dt ** 3 / 3, dt ** 2 / 2], [dt ** 2 / 2, dt]])
    Q = np.zeros((5, 5))
    Q[:2, :2], Q[2:4, 2:4], Q[4, 4] = rho_1 * A, rho_1 * A, rho_2 * dt
    return Q


def setup(name):
    """(ExtendedKalman, (fd, fd_dx, fo, fo_dx) host callables, kernel shape) of 'cv_radar' | 'ct_bearing' | 'ct_radar' | 'cv_bearing'."""
    from ssmtoybox_amd import ssinf, ssmod as sm
    dyn_name, obs_name = name.split('_')
    if dyn_name == 'ct':
        D, fd, fd_dx = 5, tj.ct_f, tj.ct_dx
        dyn = sm.CoordinatedTurnTransition(sm.GaussRV(5, M0, P0), sm.GaussRV(5, cov=ct_q()), dt=tj.DT)
    else:
        D, fd, fd_dx = 4, tj.cv_f, tj.cv_dx
        dyn = sm.ConstantVelocity(sm.GaussRV(4, M0[:4], P0[:4, :4]), sm.GaussRV(2, cov=0.2 * np.eye(2)), dt=tj.DT)
    if name == 'cv_radar':            # no state index: the state's two leading entries (x, vx) are the radar's inputs
        obs = sm.Radar2DMeasurement(sm.GaussRV(2, cov=np.diag([0.5, 1e-4])), 4, radar_loc=tj.RADAR_LOC)
        fo, fo_dx = tj.indexed(tj.radar_f, tj.radar_dx, [0, 1], 4)
    elif obs_name == 'radar':
        obs = sm.Radar2DMeasurement(sm.GaussRV(2, cov=np.diag([0.5, 1e-4])), D, state_index=[0, 2], radar_loc=tj.RADAR_LOC)
        fo, fo_dx = tj.indexed(tj.radar_f, tj.radar_dx, [0, 2], D)
    else:
        obs = sm.BearingMeasurement(sm.GaussRV(4, cov=1e-2 * np.eye(4)), D, state_index=[0, 2], sensor_pos=tj.SENSORS)
        fo, fo_dx = tj.indexed(tj.bearing_f, tj.bearing_dx, [0, 2], D)
    return ssinf.ExtendedKalman(dyn, obs), (fd, fd_dx, fo, fo_dx), 'D={},Y={}'.format(D, obs.dim_out)


_DATA, _HOST = {}, {}


def data(name, alg, T):
    if (name, T) not in _DATA:
        x = alg.mod_dyn.simulate_discrete(T, B, seed=11)
        _DATA[(name, T)] = np.ascontiguousarray(alg.mod_obs.simulate_measurements(x, seed=12))
    return _DATA[(name, T)]


def host(name, alg, fns, y):
    """The NumPy recursion in fp64 and its bars: (fm, fP, mean bar, covariance bar), once per set-up and length."""
    key = (name, y.shape[1])
    if key not in _HOST:
        args = (y, np.asarray(alg.x0_mean, dtype=float), np.asarray(alg.x0_cov, dtype=float), alg.G.dot(alg.q_cov).dot(alg.G.T),
                np.asarray(alg.r_cov, dtype=float))
        fm, fP = tj.ekf_in(np.float64, *fns, *args)
        xm, xP = tj.ekf_in(np.longdouble, *fns, *args)
        assert np.all(np.isfinite(fm)) and np.all(np.isfinite(fP))
        e_m, e_P = mean_err(fm, xm.astype(float)), cov_err(fP, xP.astype(float))
        bm = MEAN_BAR if e_m <= MEAN_BAR / 4 else 4 * e_m
        bP = COV_BAR if e_P <= COV_BAR / 4 else 4 * e_P
        print('{} T = {}: fp64 recursion against longdouble: means {:.3g}, covariances {:.3g} -> bars {:.3g}, {:.3g}'.format(
            name, y.shape[1], e_m, e_P, bm, bP))
        _HOST[key] = (fm, fP, bm, bP)
    return _HOST[key]


def both_routes(monkeypatch, run):
    monkeypatch.delenv('SSMQ_NO_EKF_LOOP', raising=False)
    fused = run()
    monkeypatch.setenv('SSMQ_NO_EKF_LOOP', '1')
    loop = run()
    monkeypatch.delenv('SSMQ_NO_EKF_LOOP')
    return fused, loop


def compare(what, got, ref, bm, bP):
    e_m, e_P = mean_err(got[0], ref[0]), cov_err(got[1], ref[1])
    print('{}: means {:.3g} (bar {:.3g}), covariances {:.3g} (bar {:.3g})'.format(what, e_m, bm, e_P, bP))
    assert np.all(np.isfinite(got[0])) and np.all(np.isfinite(got[1])) and e_m < bm and e_P < bP, (what, e_m, e_P)


def _jacobian_cases():
    from ssmtoybox_amd import ssmod as sm
    ct = sm.CoordinatedTurnTransition(dt=tj.DT)
    return {
        'ct55': ('ct', ct.dyn_eval, 5, None),
        'radar42': ('radar', sm.Radar2DMeasurement(sm.GaussRV(2), 4, radar_loc=tj.RADAR_LOC).meas_eval, 4, [0, 1]),
        'radar52': ('radar', sm.Radar2DMeasurement(sm.GaussRV(2), 5, state_index=[0, 2], radar_loc=tj.RADAR_LOC).meas_eval, 5, [0, 2]),
        'bearing54': ('bearing', sm.BearingMeasurement(sm.GaussRV(4), 5, state_index=[0, 2], sensor_pos=tj.SENSORS).meas_eval, 5, [0, 2]),
        'bearing44': ('bearing', sm.BearingMeasurement(sm.GaussRV(4), 4, state_index=[0, 2], sensor_pos=tj.SENSORS).meas_eval, 4, [0, 2]),
    }


@pytest.mark.parametrize('generic', [False, True])
@pytest.mark.parametrize('case', ['ct55', 'radar42', 'radar52', 'bearing54', 'bearing44'])
def test_1_jacobian_entries_against_the_oracle(monkeypatch, case, generic):
    """cov = I: cov_fx = J.  The register-resident body and k_linearize<0, 0> (SSMQ_LINEAR_GENERIC=1) at the same bar."""
    from ssmtoybox_amd.mtran import LinearizationTransform
    name, f, D, idx = _jacobian_cases()[case]
    pts = tj.reference(name)[0]
    x = pts if idx is None else tj.embed(pts, D, idx)
    if generic:
        monkeypatch.setenv('SSMQ_LINEAR_GENERIC', '1')
    else:
        monkeypatch.delenv('SSMQ_LINEAR_GENERIC', raising=False)
    tf = LinearizationTransform(D)
    J = tf.apply_batch(f, x, np.broadcast_to(np.eye(D), (len(x), D, D)), 0.0)[2]
    if idx is not None:
        rest = [d for d in range(D) if d not in idx]
        assert not J[:, :, rest].any()
        J = J[:, :, idx]
    K, r = tj.bound_K(name), tj.ratio(J, name)
    print('{} ({}): device |err| / (eps S) = {:.3g}, NumPy {:.3g}, K = {:.3g}'.format(case, 'run-time sizes' if generic else 'registers', r,
                                                                                      tj.twin_ratio(name), K))
    assert r <= K


def test_2_check_jacobian():
    """Below 1e-6 at the points of test 1.  The measurement models get rel_step = 1e-7: at r = 1 next to coordinates of order 1e3 the
    default step (1e-5 |x| = 1e-2) is no longer small against r, and the central difference itself is off by (h / r)^2."""
    from ssmtoybox_amd import ssmod as sm
    assert np.max(sm.CoordinatedTurnTransition(dt=tj.DT).check_jacobian(tj.ct_points())) < 1e-6
    x = tj.embed(tj.radar_points(), 5, [0, 2])
    assert np.max(sm.Radar2DMeasurement(sm.GaussRV(2), 5, state_index=[0, 2], radar_loc=tj.RADAR_LOC).check_jacobian(x, rel_step=1e-7)) < 1e-6
    x = tj.embed(tj.bearing_points(), 5, [0, 2])
    assert np.max(sm.BearingMeasurement(sm.GaussRV(4), 5, state_index=[0, 2], sensor_pos=tj.SENSORS).check_jacobian(x, rel_step=1e-7)) < 1e-6


@pytest.mark.parametrize('T', [1, 2, 20])
@pytest.mark.parametrize('name', ['cv_radar', 'ct_bearing', 'ct_radar', 'cv_bearing'])
def test_3_ekf_loop_against_the_launch_loop_and_numpy(monkeypatch, name, T):
    alg, fns, shape = setup(name)
    monkeypatch.delenv('SSMQ_NO_EKF_LOOP', raising=False)
    assert alg.kernel_name() == 'k_ekf_loop<{}>'.format(shape)
    y = data(name, alg, T)
    rm, rP, bm, bP = host(name, alg, fns, y)
    fused, loop = both_routes(monkeypatch, lambda: alg.forward_pass_batch(y))
    assert not alg.status.any()
    compare('{} T = {}: k_ekf_loop against the launch loop'.format(name, T), fused, loop, MEAN_BAR, COV_BAR)
    compare('{} T = {}: k_ekf_loop against the NumPy recursion'.format(name, T), fused, (rm, rP), bm, bP)


def test_4_smoother(monkeypatch):
    """backward_pass_batch of the (5, 4) set-up, fused against the launch loop; the forward bits of the kernel that keeps the predictive
    moments (k_ekf_loop_keep<D=5,Y=4>, run by backward_pass_batch) are those of the plain one (k_ekf_loop<D=5,Y=4>).  No entry point names the keeping kernel (ssmq_filter_kernel_name is the forward
    pass's): that it ran shows in the smoothed moments, which k_rts_backward forms from the predictive moments it kept and which
    agree with the launch loop's smoother."""
    alg, fns, _ = setup('ct_bearing')
    y = data('ct_bearing', alg, 20)
    _, _, bm, bP = host('ct_bearing', alg, fns, y)

    def run():
        fm, fP = alg.forward_pass_batch(y)                # the plain kernel
        fm, fP = fm.copy(), fP.copy()
        sm_, sP = alg.backward_pass_batch()               # forward_pass_batch(smooth=True): the keeping kernel, then k_rts_backward
        assert np.array_equal(alg.fi_mean, fm) and np.array_equal(alg.fi_cov, fP)
        assert np.array_equal(sm_[:, -2:], fm[:, -2:]) and not np.array_equal(sm_[:, :-2], fm[:, :-2])      # (the smoother ran)
        return sm_, sP
    monkeypatch.delenv('SSMQ_NO_EKF_LOOP', raising=False)
    assert alg.kernel_name() == 'k_ekf_loop<D=5,Y=4>'      # (backward_pass_batch runs the pass again, with the moments kept)
    fused, loop = both_routes(monkeypatch, run)
    compare('ct_bearing smoother: k_ekf_loop against the launch loop', fused, loop, MEAN_BAR, COV_BAR)


@pytest.mark.parametrize('name,scale', [('ct_radar', 1.0), ('ct_bearing', 1e6)])
def test_5_failure(monkeypatch, name, scale):
    """P0 = -I on one trajectory of coordinated turn + radar, k_ekf_loop<D=5,Y=2>: the range row of H has unit norm, so the innovation
    matrix of step 0 is R - 1 + .. < 0.  With four bearings |H| = 1 / r = 1e-3 and R = 1e-2 keeps S positive under P0 = -I, nothing
    fails there; P0 = -1e6 I (H P H' = -1) takes the status and NaN path of the (5, 4) body."""
    alg, _, _ = setup(name)
    T, bad = 5, 100
    y = data(name, alg, T)
    P0b = np.tile(P0, (B, 1, 1))
    P0b[bad] = -scale * np.eye(5)
    good = alg.forward_pass_batch(y)

    def run():
        fm, fP = alg.forward_pass_batch(y, x0_cov=P0b, raise_on_failure=False)
        return fm, fP, alg.status.copy()
    (fm, fP, st), (lm, lP, lst) = both_routes(monkeypatch, run)
    step = int(st[bad]) - 1
    assert st[bad] == 1 and np.count_nonzero(st) == 1 and np.array_equal(st, lst)
    assert np.all(np.isnan(fm[:, step:, bad])) and np.all(np.isnan(fP[:, :, step:, bad])) and np.all(np.isfinite(fm[:, :step, bad]))
    assert np.array_equal(np.isnan(fm), np.isnan(lm)) and np.array_equal(np.isnan(fP), np.isnan(lP))
    keep = np.arange(B) != bad
    assert np.array_equal(fm[..., keep], good[0][..., keep]) and np.array_equal(fP[..., keep], good[1][..., keep])


def test_6_padding_lanes_keep_their_sentinel():
    """ssmq_filter_forward_dev at (5, 4) on sentinel-filled planes of pitch 256: lanes 193 .. 255 of d_fm, d_fP and the status stay
    untouched, lanes 0 .. 192 hold the bits of forward_pass_batch."""
    import ctypes
    from ssmtoybox_amd import _lib
    from ssmtoybox_amd.mtran import resolve_integrand
    lib = _lib.load()
    alg, _, _ = setup('ct_bearing')
    T, D, Y, sent = 2, 5, 4, 7.25
    y = data('ct_bearing', alg, T)
    d_y = _lib.DeviceBuffer(8 * T * Y * LD)
    _lib.upload_study(y, Y, LD, d_y)
    m0, P0p = np.zeros((D, LD)), np.zeros((D * D, LD))
    m0[:, :B] = M0.reshape(D, 1)
    P0p[:, :B] = P0.reshape(D * D, 1)
    P0p[:, B:] = np.nan                                   # (never read)
    d_m0, d_P0 = _lib.DeviceBuffer(m0.nbytes), _lib.DeviceBuffer(P0p.nbytes)
    d_m0.upload(m0)
    d_P0.upload(P0p)
    outs = [_lib.DeviceBuffer(8 * T * n * LD) for n in (D, D * D)]
    for o, n in zip(outs, (D, D * D)):
        o.upload(np.full(T * n * LD, sent))
    d_st = _lib.DeviceBuffer(4 * LD)
    d_st.upload(np.full(LD, 77, dtype=np.int32))
    f_dyn, e_dyn = resolve_integrand(alg.mod_dyn.dyn_eval)
    f_obs, e_obs = resolve_integrand(alg.mod_obs.meas_eval)
    h_dyn, h_obs = ctypes.c_void_p(alg.tf_dyn._handle_for(e_dyn)), ctypes.c_void_p(alg.tf_obs._handle_for(e_obs))
    gqg, pg = _lib.as_c(alg.G.dot(alg.q_cov).dot(alg.G.T))
    rr, pr = _lib.as_c(alg.r_cov)
    p = [ctypes.c_void_p(b.ptr) for b in (d_y, d_m0, d_P0)]
    _lib.check(lib.ssmq_filter_forward_dev(h_dyn, ctypes.byref(f_dyn), h_obs, ctypes.byref(f_obs), B, LD, T, p[0], p[1], p[2], pg, pr,
                                           ctypes.c_void_p(outs[0].ptr), ctypes.c_void_p(outs[1].ptr), ctypes.c_void_p(d_st.ptr)),
               'ssmq_filter_forward_dev')
    _lib.sync()
    assert alg.kernel_name() == 'k_ekf_loop<D=5,Y=4>'
    fm, fP = alg.forward_pass_batch(y)
    for o, n, ref in zip(outs, (D, D * D), (fm, fP.reshape(D * D, T, B))):
        planes = o.download((T, n, LD))
        assert np.all(planes[:, :, B:] == sent) and np.array_equal(planes[:, :, :B], ref.transpose(1, 0, 2))
    st = d_st.download((LD,), dtype=np.int32)
    assert not st[:B].any() and np.all(st[B:] == 77)
    for b in [d_y, d_m0, d_P0, d_st] + outs:
        b.free()


def test_7_run_filters():
    from ssmtoybox_amd import ssinf
    alg, _, _ = setup('ct_bearing')
    y = data('ct_bearing', alg, 20)
    fm, fP = alg.forward_pass_batch(y)
    ukf = ssinf.UnscentedKalman(alg.mod_dyn, alg.mod_obs)
    um, uP = ukf.forward_pass_batch(y)
    for _ in range(2):                                   # the second: the captured launch, replayed
        (em, eP), (vm, vP) = ssinf.run_filters([alg, ukf], y)
        assert np.array_equal(em, fm) and np.array_equal(eP, fP) and np.array_equal(vm, um) and np.array_equal(vP, uP)
    assert not alg.status.any() and not ukf.status.any()


@pytest.mark.parametrize('case', ['ct55', 'bearing54'])
def test_8_taylor_gpqd(case):
    """TaylorGPQDTransform at (5, 5) and (5, 4) against tests/_taylor_oracle.py fed with the NumPy Jacobians, at the bar of
    tests/test_taylor_gpqd_gpu.py (assert_moments_close at LINEAR_BAR = 1e-12)."""
    from ssmtoybox_amd.mtran import TaylorGPQDTransform
    from tests import _taylor_oracle as to
    name, f, D, idx = _jacobian_cases()[case]
    rng = np.random.default_rng(3)
    n = 64
    mean = M0 + rng.standard_normal((n, 5)) * np.sqrt(np.diag(P0))
    a = rng.standard_normal((n, 5, 5)) * np.sqrt(np.diag(P0))[None, :, None]
    cov = np.einsum('bij,bkj->bik', a, a) / 5 + P0
    par = np.array([[1.0, 300.0, 100.0, 300.0, 100.0, 1.0]])
    tf = TaylorGPQDTransform(5, par)
    mf, cf, cfx = tf.apply_batch(f, mean, cov, 0.0)[:3]
    fx, f_dx = (tj.ct_f, tj.ct_dx) if name == 'ct' else tj.indexed(tj.bearing_f, tj.bearing_dx, [0, 2], 5)
    ref = [to.taylor_gpqd(np.atleast_1d(fx(mean[b], 0.0)), f_dx(mean[b], 0.0), cov[b], par[0, 0], par[0, 1:])[:3] for b in range(n)]
    ref = tuple(np.stack([r[k] for r in ref]) for k in range(3))
    assert_moments_close((mf, cf, cfx), ref, cov, rtol=LINEAR_BAR, what=case)


def test_8_posterior_crlb():
    """Coordinated turn + four bearings at the bars of the bound's own tests: the device sums against tests/_pcrlb_oracle.py::sums
    over the NumPy Jacobians at RTOL x the sum of |terms| (tests/test_pcrlb_gpu.py), the bound against the 50-digit recursion at
    RTOL x the condition number it meets (tests/test_pcrlb_host.py)."""
    from ssmtoybox_amd import ssinf, mcshard, _lib
    from tests import _pcrlb_oracle as po
    alg, (fd, fd_dx, fo, fo_dx), _ = setup('ct_bearing')
    T, Bc, ld = 10, 300, 320
    x = alg.mod_dyn.simulate_discrete(T + 1, Bc, seed=21)
    p = po.Pair('ct_bearing', 5, 4, fd_dx, fo_dx, ct_q(), 1e-2 * np.eye(4), P0, None, m0=M0)
    s, s_abs = po.sums(p, x)
    xb = np.zeros((T + 1, 5, ld))
    xb[:, :, :Bc] = x.transpose(1, 0, 2)
    d_x = _lib.DeviceBuffer(xb.nbytes)
    d_x.upload(xb)
    got = mcshard.device_crlb_sums(alg.mod_dyn, alg.mod_obs, d_x, Bc, ld, T)
    d_x.free()
    assert mcshard.crlb_kernel_name(alg.mod_dyn, alg.mod_obs) == 'k_pcrlb_dyn<5, 5> | k_pcrlb_obs<5, 4> | k_pcrlb_rows'
    print('sums: largest error relative to the sum of |terms| %.3g' % np.max(np.abs(got - s) / np.maximum(s_abs, 1e-300)))
    assert np.all(np.abs(got - s) <= RTOL * s_abs)
    out = ssinf.posterior_crlb(alg.mod_dyn, alg.mod_obs, x)
    _, xb_, xr, cond = po.recursion_mp(s, Bc, P0, ct_q())
    assert out['status'] == 0
    for what, g, r in (('bound', out['bound'], xb_), ('rmse_bound', out['rmse_bound'], xr)):
        err = np.max(np.abs(g - r)) / np.max(np.abs(r))
        print('%s: error %.3g, bar %.3g (cond %.3g)' % (what, err, RTOL * cond, cond))
        assert err <= RTOL * cond


def test_9_user_transition_with_builtin_radar(monkeypatch):
    """Constant velocity written as a user model (device_code + device_jacobian) + the built-in radar: the launch loop (a user
    member keeps it) against the built-in pair's launch loop, at the bars of test 3."""
    from ssmtoybox_amd import ssinf, ssmod as sm
    alg, fns, _ = setup('cv_radar')
    y = data('cv_radar', alg, 20)
    _, _, bm, bP = host('cv_radar', alg, fns, y)
    code = 'o[0] = x[0] + p[0]*x[1]; o[1] = x[1]; o[2] = x[2] + p[0]*x[3]; o[3] = x[3];'
    jac = 'J[0] = 1.0; J[ldj] = p[0]; J[ldj + 1] = 1.0; J[2*ldj + 2] = 1.0; J[3*ldj + 2] = p[0]; J[3*ldj + 3] = 1.0;'
    cls = type('UserCV', (sm.TransitionModel,), dict(dim_state=4, dim_noise=2, noise_additive=True, device_code=code, device_jacobian=jac,
                                                     _par=lambda self: (tj.DT,)))
    user = cls(alg.mod_dyn.init_rv, alg.mod_dyn.noise_rv, alg.mod_dyn.noise_gain)
    mixed = ssinf.ExtendedKalman(user, alg.mod_obs)
    monkeypatch.setenv('SSMQ_NO_EKF_LOOP', '1')
    ref = alg.forward_pass_batch(y)
    monkeypatch.delenv('SSMQ_NO_EKF_LOOP')
    got = mixed.forward_pass_batch(y)
    assert not mixed.status.any()
    compare('user constant velocity + radar against the built-in launch loop', got, ref, bm, bP)


@pytest.mark.parametrize('case', ['ct55', 'radar42', 'radar52', 'bearing54'])
def test_8_gpqd(case):
    """GaussianProcessDerTransform (k_apply_gpqd_lds at the new shapes) against tests/_gpqd_oracle.py with the device's weights, at the
    bar of tests/test_gpqd_gpu.py (assert_moments_close, RTOL)."""
    import ssmtoybox_amd as amd
    from tests import _gpqd_oracle as go
    from tests.test_gpqd_gpu import device_weights
    name, f, D, idx = _jacobian_cases()[case]
    fx, f_dx = (tj.ct_f, tj.ct_dx) if name == 'ct' else tj.indexed(*{'radar': (tj.radar_f, tj.radar_dx), 'bearing': (tj.bearing_f, tj.bearing_dx)}[name], idx, D)
    E = np.atleast_1d(fx(M0[:D], 0.0)).shape[0]
    rng = np.random.default_rng(4)
    n = 67
    sd = np.sqrt(np.diag(P0))[:D]
    mean = M0[:D] + 0.3 * rng.standard_normal((n, D)) * sd
    a = rng.standard_normal((n, D, D)) * sd[None, :, None]
    cov = 0.1 * np.einsum('bij,bkj->bik', a, a) / D + 0.1 * P0[:D, :D]
    time = np.zeros(n)
    tf = amd.GaussianProcessDerTransform(D, E, np.array([[1.0] + [3.0] * D]))
    assert tf.kernel_name(f) == 'k_apply_gpqd_lds'
    got = tf.apply_batch(f, mean, cov, time)
    ref = go.apply_batch(fx, f_dx, mean, cov, time, tf.model.points, None, device_weights(tf))
    e = assert_moments_close(got, ref, cov, what=case)
    print('{}: GPQ+D against the oracle with the device\'s weights {:.3g}'.format(case, e))


def _lin_tf(f, f_dx):
    """A linearisation as the transform callable of tests/_innovation_oracle.py / _iterated_oracle.py: (m, P, t) -> moments."""
    from tests import _user_jac_oracle as uo
    return lambda m, P, t: uo.linearize(f, f_dx, np.asarray(m, dtype=float), P, float(t))


def test_8_iterated_pass():
    """ExtendedKalman.iterated_pass_batch(iterations = 3) on constant velocity + radar: every step against the restatement of
    tests/_iterated_oracle.py started from the device's moments of the step before, under the bound of tests/test_iterated_gpu.py
    (max(RTOL, 64 eps x the condition numbers of the iterates), moment_scales)."""
    from tests import _iterated_oracle as ito
    from tests._cases import moment_scales
    alg, (fd, fd_dx, fo, fo_dx), _ = setup('cv_radar')
    T, J = 6, 3
    y = data('cv_radar', alg, T)
    fm, fP = alg.iterated_pass_batch(y, J)[:2]
    assert not alg.status.any()
    tfd, tfo = _lin_tf(fd, fd_dx), _lin_tf(fo, fo_dx)
    GQG = alg.G.dot(alg.q_cov).dot(alg.G.T)
    eps, worst = float(np.finfo(float).eps), 0.0
    for b in range(B):
        for k in range(T):
            m, P = (alg.x0_mean, alg.x0_cov) if k == 0 else (fm[:, k - 1, b], fP[..., k - 1, b])
            mj, Pj, dj, conds = ito.step(m, P, y[:, k, b], k, J, GQG, alg.r_cov, tfd, tfo)
            assert conds is not None, (b, k)
            rtol = max(RTOL, 64.0 * eps * sum(conds))
            ms, cs, _ = moment_scales(mj, Pj, np.zeros((1, 1)), np.asarray(P, dtype=float))
            worst = max(worst, float(np.max(np.abs(fm[:, k, b] - mj))) / ms / rtol, float(np.max(np.abs(fP[..., k, b] - Pj))) / cs / rtol)
    print('iterated EKF, constant velocity + radar, 3 iterations: largest error / bound {:.3g}'.format(worst))
    assert worst <= 1.0


def test_8_innovations():
    """innovations_batch of ExtendedKalman on coordinated turn + bearings against tests/_innovation_oracle.py over the NumPy
    linearisations, at the bars of tests/test_innovation_gpu.py (assert_moments_close, check_scores)."""
    from tests import _innovation_oracle as ino
    from tests.test_innovation_gpu import check_scores
    alg, (fd, fd_dx, fo, fo_dx), _ = setup('ct_bearing')
    T = 5
    y = data('ct_bearing', alg, T)
    fm, fP = alg.forward_pass_batch(y)
    out = alg.innovations_batch(y, fi_mean=fm, fi_cov=fP, return_moments=True)
    assert not out['status'].any()
    tfd, tfo = _lin_tf(fd, fd_dx), _lin_tf(fo, fo_dx)
    GQG = alg.G.dot(alg.q_cov).dot(alg.G.T)
    ref = [ino.innovations(y[..., b], alg.x0_mean, alg.x0_cov, fm[..., b], fP[..., b], GQG, alg.r_cov, tfd, tfo) for b in range(B)]
    zero = np.zeros((1, 1))
    for b in range(B):
        ym, S, _, _ = ref[b]
        for k in range(T):
            P_in = alg.x0_cov if k == 0 else fP[..., k - 1, b]
            assert_moments_close((out['y_mean'][:, k, b], out['y_cov'][:, :, k, b], zero), (ym[:, k], S[..., k], zero), P_in, what=(b, k))
    check_scores(out, [x[2] for x in ref], [x[3] for x in ref], [x[1] for x in ref], 'EKF on ct_bearing')


@pytest.mark.parametrize('kind', ['ekf_gpqd', 'gpqd'])
def test_8_jacobian_filters_on_the_coordinated_turn(kind):
    """ExtendedKalmanGPQD and GaussianProcessDerKalman on coordinated turn + bearings against a Python loop of their own transforms
    (each held to its oracle by test_8_taylor_gpqd / test_8_gpqd) and the host's Kalman update, as tests/test_gpqd_gpu.py tests
    GaussianProcessDerKalman, at its bars (1e-10 on row-scaled means and entry-scaled covariances); then the RTS smoother."""
    from oracle import ssmq_oracle as orc
    from ssmtoybox_amd import ssinf
    ekf, _, _ = setup('ct_bearing')
    dyn, obs = ekf.mod_dyn, ekf.mod_obs
    T, Bf = 5, 64
    y = data('ct_bearing', ekf, T)[..., :Bf]
    pd, po_ = np.array([[1.0, 300.0, 100.0, 300.0, 100.0, 1.0]]), np.array([[1.0, 300.0, 100.0, 300.0, 100.0, 1.0]])
    flt = ssinf.ExtendedKalmanGPQD(dyn, obs, pd, po_) if kind == 'ekf_gpqd' else ssinf.GaussianProcessDerKalman(dyn, obs, pd, po_)
    fm, fP = flt.forward_pass_batch(y)
    assert not flt.status.any()
    m, P = np.tile(flt.x0_mean, (Bf, 1)), np.tile(flt.x0_cov, (Bf, 1, 1))
    gqg = flt.G.dot(flt.q_cov).dot(flt.G.T)
    rm, rP = np.zeros_like(fm), np.zeros_like(fP)
    for k in range(T):
        mp, Pp = flt.tf_dyn.apply_batch(dyn.dyn_eval, m, P, float(k))[:2]
        Pp = Pp + gqg
        ym, Py, Pyx = flt.tf_obs.apply_batch(obs.meas_eval, mp, Pp, float(k))[:3]
        Py = Py + flt.r_cov
        for b in range(Bf):
            m[b], P[b] = orc.kalman_update(mp[b], Pp[b], ym[b], Py[b], Pyx[b], y[:, k, b])
        rm[:, k], rP[:, :, k] = m.T, P.transpose(1, 2, 0)
    e_m, e_P = mean_err(fm, rm), cov_err(fP, rP)
    print('{} on ct_bearing against the loop of its transforms: mean_err {:.3g}, cov_err {:.3g}'.format(kind, e_m, e_P))
    assert e_m <= 1e-10 and e_P <= 1e-10, (e_m, e_P)
    sm_, sP = flt.backward_pass_batch()
    assert np.all(np.isfinite(sm_)) and np.all(np.isfinite(sP))


@pytest.mark.parametrize('case', ['radar22', 'bearing22', 'bearing21'])
def test_8_gpqd_small_shapes(case):
    """GPQ+D of the radar on a 2-state, of two bearings and of one bearing on a 2-state (k_apply_gpqd<2, 2>, <2, 1>): values and
    Jacobian are both compiled wherever the Jacobian fits (csrc/ssmq_device.h: jacobian_fits)."""
    import ssmtoybox_amd as amd
    from ssmtoybox_amd import ssmod as sm
    from tests import _gpqd_oracle as go
    from tests.test_gpqd_gpu import device_weights
    sens = tj.SENSORS[:2] if case == 'bearing22' else tj.SENSORS[:1]
    if case == 'radar22':
        f, fx, f_dx, E = sm.Radar2DMeasurement(sm.GaussRV(2), 2, radar_loc=tj.RADAR_LOC).meas_eval, tj.radar_f, tj.radar_dx, 2
    else:
        E = len(sens)
        f = sm.BearingMeasurement(sm.GaussRV(E), 2, sensor_pos=np.array(sens)).meas_eval
        fx, f_dx = (lambda x, t: tj.bearing_f(x, t, sens)), (lambda x, t: tj.bearing_dx(x, t, sens))
    rng = np.random.default_rng(8)
    n = 67
    mean = np.array([700.0, 400.0]) + 10.0 * rng.standard_normal((n, 2))
    a = rng.standard_normal((n, 2, 2))
    cov = np.einsum('bij,bkj->bik', a, a) + 4.0 * np.eye(2)
    time = np.zeros(n)
    tf = amd.GaussianProcessDerTransform(2, E, np.array([[1.0, 3.0, 3.0]]))
    assert tf.kernel_name(f) == 'k_apply_gpqd'
    got = tf.apply_batch(f, mean, cov, time)
    ref = go.apply_batch(fx, f_dx, mean, cov, time, tf.model.points, None, device_weights(tf))
    assert np.max(np.abs(got[0])) > 0.1
    e = assert_moments_close(got, ref, cov, what=case)
    print('{}: GPQ+D against the oracle with the device\'s weights {:.3g}'.format(case, e))
