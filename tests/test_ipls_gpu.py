"""The iterated posterior linearisation smoother (IPLS) on the device against its NumPy restatement (tests/_ipls_oracle.py):
k_ipls_pass<> for the table shapes and for user pairs.  B = 70 (one full block of 64 lanes and a partial one), T = 6.

Bound.  Every forward step k is compared with the one-step restatement started from the DEVICE's filtered moments of step k - 1, every
backward step with the restatement started from the device's smoothed moments of step k and the restatement's m-, P-, C_k, by
assert_moments_close with rtol = max(RTOL, 64 eps sum cond): the project's bound for one application of an inverse
(tests/test_gpu_parity.py), summed over the inverses the step applies - Pl_{k-1}, Pl_k and S in the forward step, P-_k in addition in the
backward step - with the condition numbers of the restatement.  For J = 3 the linearisation moments handed to the restatement are the
device's own J = 2 smoothed moments.  No case needed more than this bound (MEASURED is empty; the procedure for one that does - 4 x the
float64 restatement's own error against its long-double form - is helper_error_of)."""
import ctypes

import numpy as np
import pytest

from tests import _innovation_oracle as ino
from tests import _ipls_oracle as ipo
from tests._cases import RTOL, assert_moments_close, moment_scales
from tests.test_iterated_gpu import ONE_LAUNCH, case_tf, make_case
from tests.test_innovation_gpu import simulate

pytestmark = pytest.mark.gpu
EPS = float(np.finfo(float).eps)
B, T = 70, 6
Z = np.zeros((1, 1))
MEASURED = ()            # cases whose bound is 4 x the float64 restatement's own error (none)
_DATA, _RUNS, _ORACLE = {}, {}, {}


@pytest.fixture(scope='module')
def amd():
    import ssmtoybox_amd
    if ssmtoybox_amd.device_count() < 1:
        pytest.fail('no device: the GPU tests need an MI355X')
    ssmtoybox_amd.set_device(0)
    return ssmtoybox_amd


def case_data(name):
    """(filter, the built-in twin the restatement evaluates, measurements (Y, T, B)): made once, never modified."""
    if name not in _DATA:
        alg = make_case(name)
        twin = make_case('pend_ukf') if name == 'user_pend' else alg
        _DATA[name] = (alg, twin, simulate(twin, B, T, 3))
    return _DATA[name]


def run_case(name, J):
    """The case on the device.  Shared by the tests, never modified."""
    if (name, J) not in _RUNS:
        alg, _, y = case_data(name)
        sm, sP, delta = alg.iterated_smoother_batch(y, J, raise_on_failure=False, return_delta=True)
        _RUNS[(name, J)] = dict(sm=sm, sP=sP, delta=delta, fm=alg.fi_mean, fP=alg.fi_cov, sm0=alg.sm_x0_mean, sP0=alg.sm_x0_cov,
                                status=alg.status.copy())
    return _RUNS[(name, J)]


def case_tfs(name):
    alg, twin, _ = case_data(name)
    return case_tf(alg.tf_dyn, twin.mod_dyn.dyn_eval), case_tf(alg.tf_obs, twin.mod_obs.meas_eval)


def oracle_status(name, J):
    """The restatement alone, every trajectory: its status per trajectory."""
    if (name, J) not in _ORACLE:
        alg, _, y = case_data(name)
        tfd, tfo = case_tfs(name)
        GQG = alg.G.dot(alg.q_cov).dot(alg.G.T)
        _ORACLE[(name, J)] = np.array([ipo.ipls(y[..., b], alg.x0_mean, alg.x0_cov, J, GQG, alg.r_cov, tfd, tfo)['status'] for b in range(B)])
    return _ORACLE[(name, J)]


def lin_of(run, b):
    """The smoothed moments of trajectory b of a run as linearisation moments (D, T + 1), (D, D, T + 1)."""
    return (np.concatenate((run['sm0'][:, None, b], run['sm'][..., b]), axis=1),
            np.concatenate((run['sP0'][:, :, None, b], run['sP'][..., b]), axis=2))


def helper_error_of(name, run, lin_run):
    """max |float64 restatement - long-double restatement| of (mean / ms, covariance / cs) over the steps of a MEASURED case."""
    if name not in MEASURED:
        return np.zeros(2)
    from ssmtoybox_amd import mtran
    alg, twin, y = case_data(name)
    tfd, tfo = case_tfs(name)
    tfs = []
    for tf, ev in ((alg.tf_dyn, twin.mod_dyn.dyn_eval), (alg.tf_obs, twin.mod_obs.meas_eval)):
        f, _ = mtran.resolve_integrand(ev)
        tfs.append(ino.sigma_tf_ld(f.id, tuple(f.par[i] for i in range(f.n_par)), tf.unit_sp, tf.wm, np.diag(tf.Wc),
                                   tuple(f.idx[i] for i in range(f.n_idx)) if f.n_idx else None))
    GQG = alg.G.dot(alg.q_cov).dot(alg.G.T)
    worst = np.zeros(2)
    for b in np.flatnonzero(run['status'] == 0):
        lm, lP = lin_of(lin_run, b) if lin_run is not None else (None, None)
        for k in range(T):
            m, P = (alg.x0_mean, alg.x0_cov) if k == 0 else (run['fm'][:, k - 1, b], run['fP'][..., k - 1, b])
            lp, lc = (None, None) if lm is None else ((lm[:, k], lP[..., k]), (lm[:, k + 1], lP[..., k + 1]))
            f64 = ipo.forward_step(m, P, lp, lc, y[:, k, b], k, GQG, alg.r_cov, tfd, tfo)
            fld = ipo.forward_step_ld(m, P, lp, lc, y[:, k, b], k, GQG, alg.r_cov, tfs[0], tfs[1])
            b64 = ipo.backward_step(m, P, f64[0], f64[1], f64[2], run['sm'][:, k, b], run['sP'][..., k, b])
            bld = ipo.backward_step_ld(m, P, f64[0], f64[1], f64[2], run['sm'][:, k, b], run['sP'][..., k, b])
            for (m64, P64), (mld, Pld) in (((f64[3], f64[4]), (fld[3], fld[4])), (b64[:2], bld)):
                ms, cs, _ = moment_scales(m64, P64, Z, P)
                worst = np.maximum(worst, [float(np.max(np.abs(m64 - mld))) / ms, float(np.max(np.abs(P64 - Pld))) / cs])
    print('float64 restatement against long double {}: mean {:.3g}, cov {:.3g}'.format(name, *worst))
    return worst


@pytest.mark.parametrize('J', [1, 3])
@pytest.mark.parametrize('name', ONE_LAUNCH)
def test_1_every_step_against_the_restatement(amd, name, J):
    alg, _, y = case_data(name)
    kn = alg.iterated_smoother_kernel_name(J)
    assert 'k_ipls_pass' in kn and ('run-time compiled' in kn) == (name == 'user_pend'), kn
    # the condition: at most 10 % of the trajectories fail in the restatement, and the device fails exactly those
    ost = oracle_status(name, J)
    print('restatement {} J = {}: {} of {} trajectories fail'.format(name, J, np.count_nonzero(ost), B))
    assert np.count_nonzero(ost) <= B // 10, ost
    run = run_case(name, J)
    assert run['status'].dtype == np.int32 and np.array_equal(run['status'], ost), (run['status'], ost)
    lin_run = run_case(name, J - 1) if J > 1 else None
    tfd, tfo = case_tfs(name)
    GQG = alg.G.dot(alg.q_cov).dot(alg.G.T)
    herr = 4.0 * float(np.max(helper_error_of(name, run, lin_run)))
    worst = np.zeros(2)
    for b in range(B):
        if ost[b]:      # (a failure in iteration J - 1 is one of the J-iteration run too)
            assert all(np.isnan(run[key][..., b]).all() for key in ('fm', 'fP', 'sm', 'sP', 'sm0', 'sP0', 'delta')), b
            continue
        for key in ('fP', 'sP', 'sP0'):     # both triangles are written from one value
            assert np.array_equal(run[key][..., b], np.swapaxes(run[key][..., b], 0, 1))
        assert np.array_equal(run['sm'][:, T - 1, b], run['fm'][:, T - 1, b]) and np.array_equal(run['sP'][..., T - 1, b], run['fP'][..., T - 1, b])
        assert np.isfinite(run['delta'][b])
        lm, lP = lin_of(lin_run, b) if lin_run is not None else (None, None)
        for k in range(T):
            m, P = (alg.x0_mean, alg.x0_cov) if k == 0 else (run['fm'][:, k - 1, b], run['fP'][..., k - 1, b])
            lp, lc = (None, None) if lm is None else ((lm[:, k], lP[..., k]), (lm[:, k + 1], lP[..., k + 1]))
            m_pr, P_pr, C, mk, Pk, conds = ipo.forward_step(m, P, lp, lc, y[:, k, b], k, GQG, alg.r_cov, tfd, tfo)
            assert conds is not None, (name, J, b, k)
            rtol = max(RTOL, 64.0 * EPS * sum(conds), herr)
            what = '{} J = {} forward b = {} k = {}'.format(name, J, b, k)
            worst[0] = max(worst[0], assert_moments_close((run['fm'][:, k, b], run['fP'][..., k, b], Z), (mk, Pk, Z), P, rtol, what) / rtol)
            ms_k, Ps_k = run['sm'][:, k, b], run['sP'][..., k, b]
            mo, Po, cond = ipo.backward_step(m, P, m_pr, P_pr, C, ms_k, Ps_k)
            assert cond is not None, (name, J, b, k)
            rtol = max(RTOL, 64.0 * EPS * (sum(conds) + cond), herr)
            got = (run['sm0'][:, b], run['sP0'][..., b]) if k == 0 else (run['sm'][:, k - 1, b], run['sP'][..., k - 1, b])
            what = '{} J = {} backward b = {} k = {}'.format(name, J, b, k)
            worst[1] = max(worst[1], assert_moments_close(got + (Z,), (mo, Po, Z), Ps_k, rtol, what) / rtol)
    print('iterated smoother {} J = {}: largest error / bound: forward {:.3g}, backward {:.3g}'.format(name, J, *worst))
    assert np.all(worst <= 1.0), (name, J, worst)


@pytest.mark.parametrize('name', ['ungm_ukf', 'pend_gpqkf', 'cv_radar', 'ct_bearing'])
def test_2_one_iteration_is_the_filter(amd, name):
    """fi_* of iterations = 1 against forward_pass_batch, every step from the run's own moments of step k - 1 (a pass of one step uses
    time index 0: every step of a model without time dependence, step 0 alone of UNGM), under the bound of test 1; the last smoothed
    step is the filtered one, the same bits."""
    alg, _, y = case_data(name)
    run = run_case(name, 1)
    assert not run['status'].any()
    assert np.array_equal(run['sm'][:, T - 1, :], run['fm'][:, T - 1, :]) and np.array_equal(run['sP'][..., T - 1, :], run['fP'][..., T - 1, :])
    tfd, tfo = case_tfs(name)
    GQG = alg.G.dot(alg.q_cov).dot(alg.G.T)
    D = run['fm'].shape[0]
    worst = 0.0
    for k in range(1 if name.startswith('ungm') else T):
        m0 = np.broadcast_to(alg.x0_mean, (B, D)) if k == 0 else run['fm'][:, k - 1, :].T
        P0 = np.broadcast_to(alg.x0_cov, (B, D, D)) if k == 0 else run['fP'][..., k - 1, :].transpose(2, 0, 1)
        fm, fP = alg.forward_pass_batch(y[:, k:k + 1, :], x0_mean=np.ascontiguousarray(m0), x0_cov=np.ascontiguousarray(P0), raise_on_failure=False)
        assert not alg.status.any()
        for b in range(B):
            ref = ipo.forward_step(m0[b], P0[b], None, None, y[:, k, b], k, GQG, alg.r_cov, tfd, tfo)
            rtol = max(RTOL, 64.0 * EPS * sum(ref[5]))
            e = assert_moments_close((run['fm'][:, k, b], run['fP'][..., k, b], Z), (fm[:, 0, b], ino.lower_sym(fP[..., 0, b]), Z), P0[b], rtol,
                                     '{} b = {} k = {}'.format(name, b, k))
            worst = max(worst, e / rtol)
    print('iterated smoother J = 1 against forward_pass_batch {}: largest error / bound = {:.3g}'.format(name, worst))


def _linear_case():
    """ConstantVelocity dynamics with a user measurement of the two positions: linear and Gaussian, the run-time route."""
    from ssmtoybox_amd import ssinf, ssmod as sm
    from ssmtoybox_amd.mtran import resolve_integrand

    class PositionMeasurement(sm.MeasurementModel):
        dim_out, dim_substate, dim_noise, noise_additive = 2, 4, 2, True
        device_code = 'o[0] = x[0]; o[1] = x[2];'

    dyn = sm.ConstantVelocity(sm.GaussRV(4, np.array([100.0, 5.0, 200.0, -3.0]), np.diag([1.0, 0.1, 1.0, 0.1])), sm.GaussRV(2, cov=0.1 * np.eye(2)))
    alg = ssinf.UnscentedKalman(dyn, PositionMeasurement(sm.GaussRV(2, cov=np.diag([0.5, 0.3])), 4))
    f, _ = resolve_integrand(dyn.dyn_eval)
    dt = float(f.par[0])
    A = np.array([[1, dt, 0, 0], [0, 1, 0, 0], [0, 0, 1, dt], [0, 0, 0, 1]], dtype=float)
    H = np.array([[1.0, 0, 0, 0], [0, 0, 1.0, 0]])
    rng = np.random.default_rng(7)
    Lq, Lr = alg.G.dot(np.linalg.cholesky(alg.q_cov)), np.linalg.cholesky(alg.r_cov)
    y = np.zeros((2, T, B))
    for b in range(B):
        x = alg.x0_mean + np.linalg.cholesky(alg.x0_cov).dot(rng.standard_normal(4))
        for k in range(T):
            x = A.dot(x) + Lq.dot(rng.standard_normal(2))
            y[:, k, b] = H.dot(x) + Lr.dot(rng.standard_normal(2))
    return alg, A, H, y


def test_3_linear_gaussian_against_the_closed_form(amd):
    """J = 2 on a linear-Gaussian system against a Kalman filter and RTS smoother written out in NumPy, step by step from the device's
    own moments under the bound of test 1 (condition numbers: the J = 1 smoothed moments the device linearised at, S and P-); delta
    within the IPLF delta bound rtol (2 ms / s + delta cs / (2 s^2)) of its true value 0."""
    alg, A, H, y = _linear_case()
    assert 'run-time compiled' in alg.iterated_smoother_kernel_name(2)
    GQG, R = alg.G.dot(alg.q_cov).dot(alg.G.T), alg.r_cov
    alg.iterated_smoother_batch(y, 1)
    l_m = np.concatenate((alg.sm_x0_mean[:, None, :], alg.sm_mean), axis=1)
    l_P = np.concatenate((alg.sm_x0_cov[:, :, None, :], alg.sm_cov), axis=2)
    sm, sP, delta = alg.iterated_smoother_batch(y, 2, return_delta=True)
    fm, fP, sm0, sP0 = alg.fi_mean, alg.fi_cov, alg.sm_x0_mean, alg.sm_x0_cov
    assert not alg.status.any()
    worst = np.zeros(3)
    for b in range(B):
        dbound = 0.0
        for k in range(T):
            m, P = (alg.x0_mean, alg.x0_cov) if k == 0 else (fm[:, k - 1, b], ino.lower_sym(fP[..., k - 1, b]))
            m_pr, P_pr, C = A.dot(m), A.dot(P).dot(A.T) + GQG, P.dot(A.T)
            S = H.dot(P_pr).dot(H.T) + R
            K = np.linalg.solve(S, H.dot(P_pr)).T
            mk, Pk = m_pr + K.dot(y[:, k, b] - H.dot(m_pr)), P_pr - K.dot(S).dot(K.T)
            conds = [np.linalg.cond(l_P[..., k, b]), np.linalg.cond(l_P[..., k + 1, b]), np.linalg.cond(S)]
            rtol = max(RTOL, 64.0 * EPS * sum(conds))
            worst[0] = max(worst[0], assert_moments_close((fm[:, k, b], fP[..., k, b], Z), (mk, Pk, Z), P, rtol, 'forward {} {}'.format(b, k)) / rtol)
            G = np.linalg.solve(P_pr, C.T).T
            ms_k, Ps_k = sm[:, k, b], sP[..., k, b]
            mo, Po = m + G.dot(ms_k - m_pr), P + G.dot(Ps_k - P_pr).dot(G.T)
            rtol = max(RTOL, 64.0 * EPS * (sum(conds) + np.linalg.cond(P_pr)))
            got = (sm0[:, b], sP0[..., b]) if k == 0 else (sm[:, k - 1, b], sP[..., k - 1, b])
            worst[1] = max(worst[1], assert_moments_close(got + (Z,), (mo, Po, Z), Ps_k, rtol, 'backward {} {}'.format(b, k)) / rtol)
            ms, cs, _ = moment_scales(mo, Po, Z, Ps_k)
            dbound = max(dbound, rtol * 2.0 * ms / np.sqrt(float(np.min(np.diag(Po)))))
        worst[2] = max(worst[2], delta[b] / dbound)
    print('iterated smoother, linear-Gaussian J = 2: largest error / bound: forward {:.3g}, backward {:.3g}, delta {:.3g}'.format(*worst))
    assert np.all(delta >= 0.0) and np.all(worst <= 1.0), worst


@pytest.mark.parametrize('name', ['pend_gpqkf', 'cv_radar'])
def test_4_batch_independence_and_the_device_route(amd, name):
    """The first 5 trajectories run alone against their rows of the B = 70 run, and iterated_smoother_dev against the host-array
    route: equal bits."""
    from ssmtoybox_amd import _lib
    alg, _, y = case_data(name)
    full = run_case(name, 3)
    sm, sP, delta = alg.iterated_smoother_batch(y[..., :5], 3, raise_on_failure=False, return_delta=True)
    for got, key in ((sm, 'sm'), (sP, 'sP'), (delta, 'delta'), (alg.fi_mean, 'fm'), (alg.fi_cov, 'fP'), (alg.sm_x0_mean, 'sm0'),
                     (alg.sm_x0_cov, 'sP0'), (alg.status, 'status')):
        assert np.array_equal(got, full[key][..., :5], equal_nan=True), key
    Y, D, ld = y.shape[0], full['fm'].shape[0], 128
    d_y = _lib.DeviceBuffer(8 * T * Y * ld)
    _lib.upload_study(y, Y, ld, d_y)
    bufs = alg.iterated_smoother_dev(d_y, B, ld, T, 3)
    d_fm, d_fP, d_sm, d_sP, d_sm0, d_sP0, d_delta, d_st = bufs
    for buf, key in ((d_fm, 'fm'), (d_sm, 'sm')):
        assert np.array_equal(buf.download((T, D, ld))[:, :, :B].transpose(1, 0, 2), full[key], equal_nan=True), key
    for buf, key in ((d_fP, 'fP'), (d_sP, 'sP')):
        assert np.array_equal(buf.download((T, D, D, ld))[..., :B].transpose(1, 2, 0, 3), full[key], equal_nan=True), key
    assert np.array_equal(d_sm0.download((D, ld))[:, :B], full['sm0'], equal_nan=True)
    assert np.array_equal(d_sP0.download((D, D, ld))[..., :B], full['sP0'], equal_nan=True)
    assert np.array_equal(d_delta.download((ld,))[:B], full['delta'], equal_nan=True)
    assert np.array_equal(d_st.download((ld,), dtype=np.int32)[:B], full['status'])
    for buf in (d_y,) + tuple(bufs):
        buf.free()
    one = alg.iterated_smoother(y[..., 2], 3)
    assert np.array_equal(one[0], full['sm'][..., 2]) and np.array_equal(one[1], full['sP'][..., 2])


@pytest.mark.parametrize('name', ['pend_gpqkf', 'cv_radar'])
def test_5_failure_is_a_status_not_a_fault(amd, name):
    """One trajectory starts from an indefinite covariance, another has NaN measurements at step 3: status 1 and 4, all eight outputs
    of those two NaN, every other trajectory with the bits of the clean run."""
    alg, _, y = case_data(name)
    full = run_case(name, 3)
    D, bad0, bad3 = full['fm'].shape[0], 37, 66
    assert not full['status'][[bad0, bad3]].any()
    P0 = np.broadcast_to(alg.x0_cov, (B, D, D)).copy()
    P0[bad0] = -np.eye(D)
    yn = y.copy()
    yn[:, 3, bad3] = np.nan
    with pytest.raises(np.linalg.LinAlgError):
        alg.iterated_smoother_batch(yn, 3, x0_cov=P0)
    sm, sP, delta = alg.iterated_smoother_batch(yn, 3, x0_cov=P0, raise_on_failure=False, return_delta=True)
    assert alg.status[bad0] == 1 and alg.status[bad3] == 4
    keep = np.ones(B, dtype=bool)
    keep[[bad0, bad3]] = False
    assert np.array_equal(alg.status[keep], full['status'][keep])
    for got, key in ((sm, 'sm'), (sP, 'sP'), (delta, 'delta'), (alg.fi_mean, 'fm'), (alg.fi_cov, 'fP'), (alg.sm_x0_mean, 'sm0'),
                     (alg.sm_x0_cov, 'sP0')):
        assert np.isnan(got[..., ~keep]).all(), key
        assert np.array_equal(got[..., keep], full[key][..., keep], equal_nan=True), key


def test_6_user_pendulum_against_the_builtin_pair(amd):
    """The run-time compiled pair against the table kernel of the same models, J = 3: the same bits in every output."""
    alg, _, y = case_data('pend_ukf')
    assert alg.iterated_smoother_kernel_name(3).startswith('k_ipls_pass<D=2,Y=1')
    user_alg = case_data('user_pend')[0]
    assert 'run-time compiled' in user_alg.iterated_smoother_kernel_name(3)
    ref, user = run_case('pend_ukf', 3), run_case('user_pend', 3)
    for key in ('fm', 'fP', 'sm', 'sP', 'sm0', 'sP0', 'delta', 'status'):
        assert np.array_equal(user[key], ref[key]), (key, float(np.nanmax(np.abs(user[key] - ref[key]))))
    # iterating does something here: the smoothed mean moves between J = 1 and J = 3
    assert np.max(np.abs(run_case('user_pend', 1)['sm'] - user['sm'])) > 1e-6


def test_7_refusals_through_the_c_abi_leave_the_outputs_alone(amd):
    """A non-additive pair, a Gauss-Hermite pair (SSMQ_E_UNSUPPORTED), iterations 0 and 65 and flags = 1 (SSMQ_E_ARG) return before an
    output buffer or d_status is touched."""
    from ssmtoybox_amd import _lib, ssinf, ssmod as sm
    from ssmtoybox_amd.mtran import resolve_integrand
    lib = _lib.load()
    alg, _, y = case_data('ungm_ukf')
    na = ssinf.UnscentedKalman(sm.UNGMNATransition(sm.GaussRV(1), sm.GaussRV(1)), sm.UNGMNAMeasurement(sm.GaussRV(1), 1))
    gh = ssinf.GaussHermiteKalman(sm.UNGMTransition(sm.GaussRV(1), sm.GaussRV(1, cov=np.array([[10.0]]))), sm.UNGMMeasurement(sm.GaussRV(1), 1), deg=4)
    ld, sent = 128, -7.0259e+211
    planes = np.full((T, ld), sent)
    bufs = [_lib.DeviceBuffer(planes.nbytes) for _ in range(8)]          # fm, fP, sm, sP, sm0, sP0, delta, status (D = 1)
    for b in bufs:
        b.upload(planes)
    d_y, d_m0, d_P0 = _lib.DeviceBuffer(8 * T * ld), _lib.DeviceBuffer(8 * ld), _lib.DeviceBuffer(8 * ld)
    _lib.upload_study(y, 1, ld, d_y)
    d_m0.upload(np.zeros(ld))
    d_P0.upload(np.ones(ld))
    gqg, pg = _lib.as_c(alg.G.dot(alg.q_cov).dot(alg.G.T))      # (the UNGM's: every call gets the same pair)
    rr, pr = _lib.as_c(alg.r_cov)

    def call(a, iterations, flags=0):
        f_dyn, e_dyn = resolve_integrand(a.mod_dyn.dyn_eval)
        f_obs, e_obs = resolve_integrand(a.mod_obs.meas_eval)
        vp = lambda b: ctypes.c_void_p(b.ptr)       # noqa: E731
        return lib.ssmq_smoother_iterated_dev(ctypes.c_void_p(a.tf_dyn._handle_for(e_dyn)), ctypes.byref(f_dyn),
                                              ctypes.c_void_p(a.tf_obs._handle_for(e_obs)), ctypes.byref(f_obs), B, ld, T, vp(d_y), vp(d_m0),
                                              vp(d_P0), pg, pr, iterations, flags, None, None, *[vp(b) for b in bufs])
    assert call(alg, 0) == -1 and 'iterations' in _lib.last_error()
    assert call(alg, 65) == -1 and call(alg, 2, flags=1) == -1
    assert call(na, 2) == -3 and 'additive' in _lib.last_error()
    assert call(gh, 2) == -3 and 'Gauss-Hermite' in _lib.last_error()
    _lib.sync()
    for b in bufs:
        assert np.array_equal(b.download(planes.shape), planes)
    # ... and the accepted call writes lanes 0 .. B - 1 of every plane and leaves the padding lanes alone
    assert call(alg, 2) == 0
    ref = run_case('ungm_ukf', 2)
    for buf, key in ((bufs[0], 'fm'), (bufs[2], 'sm')):
        got = buf.download(planes.shape)
        assert np.array_equal(got[:, :B], ref[key][0]) and np.all(got[:, B:] == sent), key
    assert np.array_equal(bufs[6].download(planes.shape)[0, :B], ref['delta'])
    for b in bufs + [d_y, d_m0, d_P0]:
        b.free()
