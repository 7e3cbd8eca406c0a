"""k_ekf_loop: the extended Kalman filter's whole forward pass in one kernel (csrc/ssmq_ekf_loop_kernel.h) against the reference's
runs (golden g13), the launch loop it replaces (SSMQ_NO_EKF_LOOP=1: k_linearize | k_linearize | k_kalman_update per step) and the
NumPy recursion of tests/_user_jac_oracle.py.  B = 193 trajectories on planes of pitch 256: three full waves and one lane."""
import ctypes

import numpy as np
import pytest

from tests._cases import rel_err, mean_err, cov_err, within
from tests import _user_jac_oracle as uo

pytestmark = pytest.mark.gpu

B, LD = 193, 256
LOOP = 'hipGraph of 3 T launches'
# launch-loop parity bars of tests/test_taylor_gpqd_gpu.py (row-scaled means, entry-scaled covariances); UNGM: the bar
# tests/test_gpu_parity.py::test_extended_kalman_golden holds ExtendedKalman on UNGM to (its recursion amplifies rounding)
MEAN_BAR, COV_BAR, UNGM_BAR = 1e-12, 1e-11, 1e-9


def ungm():
    from ssmtoybox_amd import ssinf, ssmod as sm
    dyn = sm.UNGMTransition(sm.GaussRV(1), sm.GaussRV(1, cov=np.array([[10.0]])))
    obs = sm.UNGMMeasurement(sm.GaussRV(1), 1)
    return ssinf.ExtendedKalman(dyn, obs)


def pendulum():
    from ssmtoybox_amd import ssinf, ssmod as sm
    dt = 0.01
    q2 = sm.GaussRV(2, cov=0.01 * np.array([[(dt ** 3) / 3, (dt ** 2) / 2], [(dt ** 2) / 2, dt]]))
    dyn = sm.Pendulum2DTransition(sm.GaussRV(2, mean=np.array([1.5, 0]), cov=0.01 * np.eye(2)), q2, dt=dt)
    obs = sm.Pendulum2DMeasurement(sm.GaussRV(1, cov=np.array([[0.1]])), 2)
    return ssinf.ExtendedKalman(dyn, obs)


def cv_indexed(meas):
    """Constant velocity (4 states) with a scalar measurement of state 2 through a state index."""
    from ssmtoybox_amd import ssinf, ssmod as sm
    dyn = sm.ConstantVelocity(sm.GaussRV(4, mean=np.array([0.3, 0.5, 1.0, -0.4]), cov=0.05 * np.eye(4)), sm.GaussRV(2, cov=0.2 * np.eye(2)), dt=0.1)
    obs = (sm.Pendulum2DMeasurement if meas == 'pend' else sm.UNGMMeasurement)(sm.GaussRV(1, cov=np.array([[0.1]])), 4, state_index=[2])
    return ssinf.ExtendedKalman(dyn, obs)


_DATA = {}


def data(name, alg, T):
    """Measurements (1, T, B) of the filter's own models, simulated once per set-up."""
    if (name, T) not in _DATA:
        x = alg.mod_dyn.simulate_discrete(T, B, seed=11)
        _DATA[(name, T)] = np.ascontiguousarray(alg.mod_obs.simulate_measurements(x, seed=12))
    return _DATA[(name, T)]


def oracle(alg, y):
    """tests/_user_jac_oracle.py::ekf with `linearize` over the models' host functions and Jacobians."""
    fd = lambda x, t: np.atleast_1d(alg.mod_dyn.dyn_eval(x, t))              # noqa: E731
    fd_dx = lambda x, t: alg.mod_dyn.dyn_eval(x, t, dx=True)                 # noqa: E731
    fo = lambda x, t: np.atleast_1d(alg.mod_obs.meas_eval(x, t))             # noqa: E731
    fo_dx = lambda x, t: alg.mod_obs.meas_eval(x, t, dx=True)                # noqa: E731
    return uo.ekf(lambda m, c, t: uo.linearize(fd, fd_dx, m, c, t), lambda m, c, t: uo.linearize(fo, fo_dx, m, c, t), y,
                  np.asarray(alg.x0_mean, dtype=float), np.asarray(alg.x0_cov, dtype=float), alg.G.dot(alg.q_cov).dot(alg.G.T), alg.r_cov)


def both_routes(monkeypatch, run):
    """run() on k_ekf_loop, then on the launch loop."""
    monkeypatch.delenv('SSMQ_NO_EKF_LOOP', raising=False)
    fused = run()
    monkeypatch.setenv('SSMQ_NO_EKF_LOOP', '1')
    loop = run()
    monkeypatch.delenv('SSMQ_NO_EKF_LOOP')
    return fused, loop


def compare(what, got, ref, ungm_bars):
    (fm, fP), (rm, rP) = got, ref
    if ungm_bars:
        e_m, e_P = rel_err(fm, rm), rel_err(fP, rP)
        ok = e_m < UNGM_BAR and e_P < UNGM_BAR
    else:
        e_m, e_P = mean_err(fm, rm), cov_err(fP, rP)
        ok = e_m < MEAN_BAR and e_P < COV_BAR
    print('{}: means {:.3g}, covariances {:.3g}'.format(what, e_m, e_P))
    assert np.all(np.isfinite(fm)) and np.all(np.isfinite(fP)) and ok, (what, e_m, e_P)


def test_1_route(monkeypatch):
    for alg, shape in ((ungm(), 'D=1,Y=1'), (pendulum(), 'D=2,Y=1'), (cv_indexed('pend'), 'D=4,Y=1')):
        monkeypatch.delenv('SSMQ_NO_EKF_LOOP', raising=False)
        monkeypatch.delenv('SSMQ_NO_FUSED', raising=False)
        assert alg.kernel_name() == 'k_ekf_loop<{}>'.format(shape) and alg.kernel_name(B) == alg.kernel_name()
        for switch in ('SSMQ_NO_FUSED', 'SSMQ_NO_EKF_LOOP'):
            monkeypatch.setenv(switch, '1')
            assert LOOP in alg.kernel_name()
            monkeypatch.delenv(switch)


@pytest.mark.parametrize('tag', ['ungm', 'pend'])
def test_2_reference(golden, tag):
    """The two set-ups of golden g13 at the bars of test_extended_kalman_golden: 1e-9 forward, 1e-8 smoothed."""
    g = golden('g13_linear')
    alg = ungm() if tag == 'ungm' else pendulum()
    assert 'k_ekf_loop' in alg.kernel_name()
    y = g['ekf_' + tag + '_y']
    fm, fP = alg.forward_pass_batch(y)
    assert within(rel_err(fm, g['ekf_' + tag + '_fm']), 1e-9, 'k_ekf_loop {} filtered means vs the reference'.format(tag))
    assert within(rel_err(fP, g['ekf_' + tag + '_fc']), 1e-9, 'k_ekf_loop {} filtered covariances vs the reference'.format(tag))
    sm_, sP = alg.backward_pass_batch()
    assert within(rel_err(sm_, g['ekf_' + tag + '_sm']), 1e-8, 'k_ekf_loop {} smoothed means vs the reference'.format(tag))
    assert within(rel_err(sP, g['ekf_' + tag + '_sc']), 1e-8, 'k_ekf_loop {} smoothed covariances vs the reference'.format(tag))


@pytest.mark.parametrize('T', [1, 2, 20])
@pytest.mark.parametrize('tag', ['ungm', 'pend'])
def test_3_launch_loop_and_oracle(monkeypatch, tag, T):
    alg = ungm() if tag == 'ungm' else pendulum()
    y = data(tag, alg, T)
    fused, loop = both_routes(monkeypatch, lambda: alg.forward_pass_batch(y))
    assert not alg.status.any()
    compare('{} T = {}: k_ekf_loop against the launch loop'.format(tag, T), fused, loop, tag == 'ungm')
    compare('{} T = {}: k_ekf_loop against the NumPy recursion'.format(tag, T), fused, oracle(alg, y), tag == 'ungm')


@pytest.mark.parametrize('meas', ['pend', 'ungm'])
def test_4_constant_velocity_with_a_state_index(monkeypatch, meas):
    """Shape (4, 1), T = 5: the measurement's Jacobian lands in column 2 of a 1 x 4 matrix, P is 4 x 4.  Pendulum bars."""
    alg = cv_indexed(meas)
    y = data('cv_' + meas, alg, 5)
    assert alg.kernel_name() == 'k_ekf_loop<D=4,Y=1>'
    fused, loop = both_routes(monkeypatch, lambda: alg.forward_pass_batch(y))
    compare('cv + {}[2]: k_ekf_loop against the launch loop'.format(meas), fused, loop, False)
    compare('cv + {}[2]: k_ekf_loop against the NumPy recursion'.format(meas), fused, oracle(alg, y), False)


@pytest.mark.parametrize('tag', ['ungm', 'pend'])
def test_5_smoother(monkeypatch, tag):
    """backward_pass_batch: k_ekf_loop with the predictive moments kept, then k_rts_backward, against the launch loop's smoother."""
    alg = ungm() if tag == 'ungm' else pendulum()
    y = data(tag, alg, 20)

    def run():
        fm, fP = alg.forward_pass_batch(y)
        sm_, sP = alg.backward_pass_batch()
        assert np.array_equal(alg.fi_mean, fm) and np.array_equal(alg.fi_cov, fP)        # (the keeping kernel: the forward pass's bits)
        assert np.array_equal(sm_[:, -2:], fm[:, -2:]) and np.array_equal(sP[:, :, -2:], fP[:, :, -2:])
        assert not np.array_equal(sm_[:, :-2], fm[:, :-2])
        return sm_, sP
    fused, loop = both_routes(monkeypatch, run)
    compare('{} smoother: k_ekf_loop against the launch loop'.format(tag), fused, loop, tag == 'ungm')


def test_6_failure(monkeypatch):
    """One trajectory starts from a covariance that makes the innovation variance of step 0 negative: status 1 and NaN from that step
    on, as the launch loop reports it, and every other trajectory keeps its bits."""
    alg = ungm()
    T, bad = 5, 100
    y = data('ungm', alg, T)
    P0 = np.tile(np.asarray(alg.x0_cov, dtype=float), (B, 1, 1))
    P0[bad] = -1.0
    # on the host: m- = f(0, t = 0) = 8, P- = J^2 P0 + 10 with J = 25.5, S = (0.1 m-)^2 P- + 1
    mp, Pp, _ = uo.linearize(uo.ungm_f, uo.ungm_dx, np.zeros(1), P0[bad], 0.0)
    _, S, _ = uo.linearize(uo.ungm_meas_f, uo.ungm_meas_dx, mp, Pp + 10.0, 0.0)
    assert S[0, 0] + 1.0 < -100.0
    good = alg.forward_pass_batch(y)

    def run():
        fm, fP = alg.forward_pass_batch(y, x0_cov=P0, raise_on_failure=False)
        return fm, fP, alg.status.copy()
    (fm, fP, st), (lm, lP, lst) = both_routes(monkeypatch, run)
    assert st[bad] == 1 and st.sum() == 1 and np.array_equal(st, lst)
    assert np.all(np.isnan(fm[..., bad])) and np.all(np.isnan(fP[..., bad]))
    assert np.array_equal(np.isnan(fm), np.isnan(lm)) and np.array_equal(np.isnan(fP), np.isnan(lP))
    keep = np.arange(B) != bad
    assert np.array_equal(fm[..., keep], good[0][..., keep]) and np.array_equal(fP[..., keep], good[1][..., keep])
    with pytest.raises(np.linalg.LinAlgError, match='trajectory 100, step 0'):
        alg.forward_pass_batch(y, x0_cov=P0)


@pytest.mark.parametrize('smooth', [False, True])
def test_7_padding_lanes_keep_their_sentinel(smooth):
    """The C ABI on sentinel-filled planes: lanes 193 .. 255 of d_fm and d_fP stay untouched by the forward kernel and by the kernel
    that keeps the predictive moments (ssmq_filter_smooth_dev; it allocates those planes itself, so what is visible of them here are
    the smoothed planes k_rts_backward makes of them)."""
    from ssmtoybox_amd import _lib
    from ssmtoybox_amd.mtran import resolve_integrand
    lib = _lib.load()
    alg = pendulum()
    T, D, sent = 2, 2, 7.25
    y = data('pend', alg, T)
    d_y = _lib.DeviceBuffer(8 * T * LD)
    _lib.upload_study(y, 1, LD, d_y)
    m0, P0 = np.zeros((D, LD)), np.zeros((D * D, LD))
    m0[:, :B] = np.asarray(alg.x0_mean).reshape(D, 1)
    P0[:, :B] = np.asarray(alg.x0_cov).reshape(D * D, 1)
    P0[:, B:] = np.nan                                    # (never read)
    d_m0, d_P0 = _lib.DeviceBuffer(m0.nbytes), _lib.DeviceBuffer(P0.nbytes)
    d_m0.upload(m0)
    d_P0.upload(P0)
    outs = [_lib.DeviceBuffer(8 * T * n * LD) for n in (D, D * D, D, D * D)]
    for o, n in zip(outs, (D, D * D, D, D * D)):
        o.upload(np.full(T * n * LD, sent))
    d_st = _lib.DeviceBuffer(4 * LD)
    d_st.upload(np.full(LD, 77, dtype=np.int32))
    f_dyn, e_dyn = resolve_integrand(alg.mod_dyn.dyn_eval)
    f_obs, e_obs = resolve_integrand(alg.mod_obs.meas_eval)
    h_dyn, h_obs = ctypes.c_void_p(alg.tf_dyn._handle_for(e_dyn)), ctypes.c_void_p(alg.tf_obs._handle_for(e_obs))
    gqg, pg = _lib.as_c(alg.G.dot(alg.q_cov).dot(alg.G.T))
    rr, pr = _lib.as_c(alg.r_cov)
    p = [ctypes.c_void_p(b.ptr) for b in (d_y, d_m0, d_P0)]
    po = [ctypes.c_void_p(o.ptr) for o in outs]
    if smooth:
        _lib.check(lib.ssmq_filter_smooth_dev(h_dyn, ctypes.byref(f_dyn), h_obs, ctypes.byref(f_obs), B, LD, T, p[0], p[1], p[2], pg, pr,
                                              po[0], po[1], po[2], po[3], ctypes.c_void_p(d_st.ptr)), 'ssmq_filter_smooth_dev')
    else:
        _lib.check(lib.ssmq_filter_forward_dev(h_dyn, ctypes.byref(f_dyn), h_obs, ctypes.byref(f_obs), B, LD, T, p[0], p[1], p[2], pg, pr,
                                               po[0], po[1], ctypes.c_void_p(d_st.ptr)), 'ssmq_filter_forward_dev')
    _lib.sync()
    fm, fP = alg.forward_pass_batch(y)
    for o, n, ref in zip(outs[:4 if smooth else 2], (D, D * D, D, D * D), (fm, fP.reshape(D * D, T, B), None, None)):
        planes = o.download((T, n, LD))
        assert np.all(planes[:, :, B:] == sent) and np.all(np.isfinite(planes[:, :, :B]))
        if ref is not None:
            assert np.array_equal(planes[:, :, :B], ref.transpose(1, 0, 2))
    assert not d_st.download((LD,), dtype=np.int32)[:B].any()
    for b in [d_y, d_m0, d_P0, d_st] + outs:
        b.free()


def test_8_same_kernel_same_bits():
    from ssmtoybox_amd import ssinf, ssmod as sm, _lib
    alg = ungm()
    T = 20
    y = data('ungm', alg, T)
    fm, fP = alg.forward_pass_batch(y)
    fm2, fP2 = alg.forward_pass_batch(y)
    assert np.array_equal(fm2, fm) and np.array_equal(fP2, fP)
    fm1, fP1 = alg.forward_pass(y[..., 7])
    assert np.array_equal(fm1, fm[..., 7]) and np.array_equal(fP1, fP[..., 7])
    d_y = _lib.DeviceBuffer(8 * T * LD)
    _lib.upload_study(y, 1, LD, d_y)
    d_fm, d_fP, d_st = alg.forward_pass_dev(d_y, B, LD, T)
    assert np.array_equal(_lib.download_study(d_fm, (1,), T, B, LD), fm) and np.array_equal(_lib.download_study(d_fP, (1, 1), T, B, LD), fP)
    for buf in (d_y, d_fm, d_fP, d_st):
        buf.free()
    # a study's list: the extended Kalman filter runs in the forked set next to the unscented one, each with its own kernel's bits
    ukf = ssinf.UnscentedKalman(alg.mod_dyn, alg.mod_obs)
    um, uP = ukf.forward_pass_batch(y)
    (em, eP), (vm, vP) = ssinf.run_filters([alg, ukf], y)
    assert np.array_equal(em, fm) and np.array_equal(eP, fP) and np.array_equal(vm, um) and np.array_equal(vP, uP)
    assert not alg.status.any() and not ukf.status.any()
    (em, eP), (vm, vP) = ssinf.run_filters([alg, ukf], y)        # the captured launch, replayed
    assert np.array_equal(em, fm) and np.array_equal(eP, fP) and np.array_equal(vm, um) and np.array_equal(vP, uP)
