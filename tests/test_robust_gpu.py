"""The outlier-robust pass on the device against its NumPy restatement (tests/_robust_oracle.py): k_robust_loop<> for the table shapes
(Y = 1, 2 and 4) and a user pair, the launch loop (apply dyn | apply obs | k_robust_update) for the other forms.  B = 70 (one full block
of 64 lanes and a partial one), T = 6, dof = 4; every fifth trajectory has a gross outlier (y + 1e3 sqrt(R_aa)) at step 3.

Bound.  Every step is compared with the one-step restatement started from the DEVICE's filtered moments of the step before, by
assert_moments_close (mean, covariance, and the weight in its third slot) with rtol = max(RTOL, 64 eps (cond P- + sum_i cond S_i)): the
project's bound for one application of an inverse (tests/test_gpu_parity.py), summed over the inverses of a step, the condition
numbers from the restatement.  The third scale of assert_moments_close is loose for a weight, so the weight is also held to
rtol x its own error scale (tests/_robust_oracle.py: weight_step - gamma is a sum that cancels), and mean and covariance are allowed
what that error of the weight moves them by on top of rtol x their scales (step: scales).  delta = |lambda_{J-1} - lambda_{J-2}| /
lambda_{J-1}: both weights within rtol ws, so within 2 rtol ws (1 + delta) / lambda.  No case needed more than this bound (MEASURED
is empty; the procedure for one that does - 4 x the float64 restatement's own error against its long-double form - is
helper_error_of)."""
import ctypes

import numpy as np
import pytest

from tests import _innovation_oracle as ino
from tests import _robust_oracle as rbo
from tests._cases import RTOL, assert_moments_close, moment_scales
from tests.test_innovation_gpu import simulate
from tests.test_iterated_gpu import case_tf, make_case

pytestmark = pytest.mark.gpu
EPS = float(np.finfo(float).eps)
B, T, DOF, KO = 70, 6, 4.0, 3

ONE_LAUNCH = ('ungm_ukf', 'pend_gpqkf', 'pend_tpqkf', 'cv_radar', 'ct_bearing', 'user_pend')
LOOP = ('pend_ghkf',)
MEASURED = ()            # cases whose bound is 4 x the float64 restatement's own error (none)
_DATA, _RUNS, _REFS = {}, {}, {}


@pytest.fixture(scope='module')
def amd():
    import ssmtoybox_amd
    if ssmtoybox_amd.device_count() < 1:
        pytest.fail('no device: the GPU tests need an MI355X')
    ssmtoybox_amd.set_device(0)
    return ssmtoybox_amd


def case_data(name):
    """(filter, the built-in twin the restatement evaluates, measurements (Y, T, B) with the outliers, the clean measurements): made
    once, never modified."""
    if name not in _DATA:
        alg = make_case(name)
        twin = make_case('pend_ukf') if name == 'user_pend' else alg
        clean = simulate(twin, B, T, 3)
        y = clean.copy()
        y[:, KO, ::5] += 1e3 * np.sqrt(np.diag(alg.r_cov))[:, None]
        _DATA[name] = (alg, twin, y, clean)
    return _DATA[name]


def run_case(name, J, dof=DOF, clean=False, **kw):
    """The case on the device: fm (D, T, B), fP (D, D, T, B), lam (T, B), delta (T, B), status.  Shared by the tests, never modified."""
    key = (name, J, dof, clean) + tuple(sorted(kw.items()))
    if key not in _RUNS:
        alg, _, y, yc = case_data(name)
        fm, fP, lam, delta = alg.robust_pass_batch(yc if clean else y, dof=dof, iterations=J, raise_on_failure=False, return_weights=True, **kw)
        _RUNS[key] = dict(fm=fm, fP=fP, lam=lam, delta=delta, status=alg.status.copy())
    return _RUNS[key]


def oracle_pair(name):
    alg, twin, _, _ = case_data(name)
    return case_tf(alg.tf_dyn, twin.mod_dyn.dyn_eval), case_tf(alg.tf_obs, twin.mod_obs.meas_eval), alg.G.dot(alg.q_cov).dot(alg.G.T)


def restated(name, J, run):
    """The one-step restatement of every (k, b) from the device's moments of step k - 1: list over b of lists over k."""
    key = (name, J, id(run))
    if key not in _REFS:
        alg, _, y, _ = case_data(name)
        tfd, tfo, GQG = oracle_pair(name)
        out = []
        for b in range(B):
            rows = []
            for k in range(T):
                m, P = (alg.x0_mean, alg.x0_cov) if k == 0 else (run['fm'][:, k - 1, b], run['fP'][..., k - 1, b])
                rows.append((m, P) + rbo.step(m, P, y[:, k, b], k, J, DOF, GQG, alg.r_cov, tfd, tfo))
            out.append(rows)
        _REFS[key] = out
    return _REFS[key]


def helper_error_of(name, J, run):
    """max |float64 restatement - long-double restatement| of (mean / ms, covariance / cs, weight / ws) over a MEASURED case."""
    if name not in MEASURED:
        return np.zeros(3)
    from ssmtoybox_amd import mtran
    alg, twin, y, _ = case_data(name)
    tfs = []
    for tf, ev in ((alg.tf_dyn, twin.mod_dyn.dyn_eval), (alg.tf_obs, twin.mod_obs.meas_eval)):
        f, _ = mtran.resolve_integrand(ev)
        tfs.append(ino.sigma_tf_ld(f.id, tuple(f.par[i] for i in range(f.n_par)), tf.unit_sp, tf.wm, np.diag(tf.Wc),
                                   tuple(f.idx[i] for i in range(f.n_idx)) if f.n_idx else None))
    GQG = alg.G.dot(alg.q_cov).dot(alg.G.T)
    worst = np.zeros(3)
    for b, rows in enumerate(restated(name, J, run)):
        for k, (m, P, mj, Pj, lj, dj, conds, (ws, dm, dP)) in enumerate(rows):
            ml, Pl, ll, _ = rbo.step_ld(m, P, y[:, k, b], k, J, DOF, GQG, alg.r_cov, tfs[0], tfs[1])
            ms, cs, _ = moment_scales(mj, Pj, np.zeros((1, 1)), P)
            worst = np.maximum(worst, [float(np.max(np.abs(mj - ml))) / (ms + ws * dm), float(np.max(np.abs(Pj - Pl))) / (cs + ws * dP),
                                       float(abs(lj - ll)) / max(ws, 1e-300) if J > 1 else 0.0])
    print('float64 restatement against long double {} J = {}: mean {:.3g}, cov {:.3g}, weight {:.3g}'.format(name, J, *worst))
    return worst


def check_against(run, ref_rows, what, J, helper_err=np.zeros(3)):
    """Every (k, b) of `run` against the restatement rows (m_in, P_in, m, P, lam, delta, conds, scales); prints the largest error / bound."""
    worst = np.zeros(4)
    for b, rows in enumerate(ref_rows):
        for k, (m, P, mj, Pj, lj, dj, conds, (ws, dm, dP)) in enumerate(rows):
            assert conds is not None and len(conds) == J + 1, (what, b, k)
            rtol = max(RTOL, 64.0 * EPS * sum(conds))
            gm, gP, gl, gd = run['fm'][:, k, b], run['fP'][..., k, b], run['lam'][k, b], run['delta'][k, b]
            assert np.isfinite(gl) and np.isfinite(gd), (what, b, k)
            ms, cs, _ = moment_scales(mj, Pj, np.zeros((1, 1)), P)
            rm, rP, rl = max(rtol, 4.0 * helper_err[0]), max(rtol, 4.0 * helper_err[1]), max(rtol, 4.0 * helper_err[2])
            if J == 1:
                assert gl == 1.0 and gd == 0.0, (what, b, k)
            assert_moments_close((gm, gP, np.array([[gl]])), (mj, Pj, np.array([[lj]])), P, max(rm, rP, rl), (what, b, k))
            e = [float(np.max(np.abs(gm - mj))) / (ms + ws * dm) / rm, float(np.max(np.abs(gP - Pj))) / (cs + ws * dP) / rP,
                 abs(gl - lj) / max(ws, 1e-300) / rl if J > 1 else 0.0, abs(gd - dj) / max(2.0 * rl * ws * (1.0 + dj) / lj, 1e-300) if J > 1 else 0.0]
            worst = np.maximum(worst, e)
    print('robust pass {}: largest error / bound: mean {:.3g}, cov {:.3g}, weight {:.3g}, delta {:.3g}'.format(what, *worst))
    assert np.all(worst <= 1.0), (what, worst)


@pytest.mark.parametrize('J', [1, 4])
@pytest.mark.parametrize('name', ONE_LAUNCH + LOOP)
def test_1_every_step_against_the_restatement(amd, name, J):
    alg = case_data(name)[0]
    kn = alg.robust_kernel_name(J)
    assert kn.startswith('k_robust_loop<') if name in ONE_LAUNCH else kn.startswith('launch loop'), kn
    assert ('run-time compiled' in kn) == (name == 'user_pend')
    run = run_case(name, J)
    assert run['status'].dtype == np.int32 and not run['status'].any()
    for b in range(B):     # both triangles are written from one value
        assert np.array_equal(run['fP'][..., b], run['fP'][..., b].transpose(1, 0, 2))
    check_against(run, restated(name, J, run), '{} J = {}'.format(name, J), J, helper_error_of(name, J, run))


def check_step_twin(name, J, run, one_step, what):
    """Step k of `run` against one_step(y_k (Y, 1, B), m (B, D), P (B, D, D)) -> (fm (D, 1, B), fP (D, D, 1, B), ...) started from the
    run's own moments of step k - 1, under the bound of the restatement for that step.  A pass of one step uses time index 0: every
    step of a model without time dependence, step 0 alone of UNGM."""
    alg, _, y, _ = case_data(name)
    rows = restated(name, J, run)
    D = run['fm'].shape[0]
    worst = 0.0
    for k in range(1 if name.startswith('ungm') else T):
        m0 = np.broadcast_to(alg.x0_mean, (B, D)) if k == 0 else run['fm'][:, k - 1, :].T
        P0 = np.broadcast_to(alg.x0_cov, (B, D, D)) if k == 0 else run['fP'][..., k - 1, :].transpose(2, 0, 1)
        out = one_step(y[:, k:k + 1, :], np.ascontiguousarray(m0), np.ascontiguousarray(P0))
        assert not alg.status.any()
        for b in range(B):
            m, P, mj, Pj, lj, dj, conds, (ws, dm, dP) = rows[b][k]
            rtol = max(RTOL, 64.0 * EPS * sum(conds))
            ms, cs, _ = moment_scales(mj, Pj, np.zeros((1, 1)), P)
            worst = max(worst, float(np.max(np.abs(run['fm'][:, k, b] - out[0][:, 0, b]))) / (ms + ws * dm) / rtol,
                        float(np.max(np.abs(run['fP'][..., k, b] - ino.lower_sym(out[1][..., 0, b])))) / (cs + ws * dP) / rtol)
            if len(out) > 2 and J > 1:
                worst = max(worst, abs(run['lam'][k, b] - out[2][0, b]) / max(ws, 1e-300) / rtol)
    print('{} {}: largest error / bound = {:.3g}'.format(what, name, worst))
    assert worst <= 1.0, (what, name, worst)


@pytest.mark.parametrize('name', ['ungm_ukf', 'pend_gpqkf', 'cv_radar', 'ct_bearing', 'pend_ghkf'])
def test_2_one_iteration_is_the_forward_pass(amd, name):
    alg = case_data(name)[0]
    check_step_twin(name, 1, run_case(name, 1), lambda yk, m, P: alg.forward_pass_batch(yk, x0_mean=m, x0_cov=P, raise_on_failure=False),
                    'robust pass J = 1 against forward_pass_batch')


@pytest.mark.parametrize('name', ONE_LAUNCH + LOOP)
def test_3_huge_dof_gives_the_bits_of_one_iteration(amd, name):
    one, five = run_case(name, 1), run_case(name, 5, dof=1e300)
    assert not five['status'].any()
    assert np.array_equal(five['fm'], one['fm']) and np.array_equal(five['fP'], one['fP'])
    assert np.all(five['lam'] == 1.0) and np.all(five['delta'] == 0.0) and np.all(one['lam'] == 1.0)


@pytest.mark.parametrize('name', ['ungm_ukf', 'pend_gpqkf', 'cv_radar', 'ct_bearing'])
def test_4_launch_loop_flag_agrees_with_the_one_launch_kernel(amd, name):
    alg = case_data(name)[0]
    assert alg.robust_kernel_name(4).startswith('k_robust_loop<') and alg.robust_kernel_name(4, launch_loop=True).startswith('launch loop')
    # the whole pass through the loop, every step against the restatement started from the loop's own moments ...
    loop = run_case(name, 4, launch_loop=True)
    assert not loop['status'].any()
    check_against(loop, restated(name, 4, loop), name + ' J = 4 (launch loop)', 4)
    # ... and the two routes against each other, step by step from the one-launch kernel's moments
    check_step_twin(name, 4, run_case(name, 4),
                    lambda yk, m, P: alg.robust_pass_batch(yk, dof=DOF, iterations=4, x0_mean=m, x0_cov=P, raise_on_failure=False,
                                                           return_weights=True, launch_loop=True),
                    'one launch against the launch loop, J = 4')


@pytest.mark.parametrize('name', ['pend_gpqkf', 'cv_radar', 'ct_bearing', 'pend_ghkf'])
def test_5_batch_independence_and_the_device_route(amd, name):
    """B = 70 against the slices 0:64, 64:70 and 5:6, and robust_pass_dev against robust_pass_batch: equal bits."""
    from ssmtoybox_amd import _lib
    alg, _, y, _ = case_data(name)
    full = run_case(name, 4)
    for sl in (slice(0, 64), slice(64, 70), slice(5, 6)):
        out = alg.robust_pass_batch(y[..., sl], dof=DOF, iterations=4, raise_on_failure=False, return_weights=True)
        for got, key in zip(out, ('fm', 'fP', 'lam', 'delta')):
            assert np.array_equal(got, full[key][..., sl]), (key, sl)
        assert not alg.status.any()
    Y, D, ld = y.shape[0], full['fm'].shape[0], 128
    d_y = _lib.DeviceBuffer(8 * T * Y * ld)
    _lib.upload_study(y, Y, ld, d_y)
    d_fm, d_fP, d_lam, d_delta, d_st = alg.robust_pass_dev(d_y, B, ld, T, dof=DOF, iterations=4)
    assert np.array_equal(d_fm.download((T, D, ld))[:, :, :B].transpose(1, 0, 2), full['fm'])
    assert np.array_equal(d_fP.download((T, D, D, ld))[..., :B].transpose(1, 2, 0, 3), full['fP'])
    assert np.array_equal(d_lam.download((T, ld))[:, :B], full['lam']) and np.array_equal(d_delta.download((T, ld))[:, :B], full['delta'])
    assert not d_st.download((ld,), dtype=np.int32)[:B].any()
    for buf in (d_y, d_fm, d_fP, d_lam, d_delta, d_st):
        buf.free()
    one = alg.robust_pass(y[..., 5], dof=DOF, iterations=4, return_weights=True)
    assert np.array_equal(one[0], full['fm'][..., 5]) and np.array_equal(one[1], full['fP'][..., 5]) and np.array_equal(one[2], full['lam'][:, 5])


@pytest.mark.parametrize('name', ONE_LAUNCH + LOOP)
def test_6_an_outlier_is_down_weighted(amd, name):
    """The weight of an outlier trajectory at step 3 is below its clean twin's, and its posterior there lies closer to the prior than
    the plain filter's from the same moments (prior and plain update: the restatement, from the run's own moments of step 2)."""
    alg, _, y, _ = case_data(name)
    rob, cln = run_case(name, 4), run_case(name, 4, clean=True)
    tfd, tfo, GQG = oracle_pair(name)
    for b in range(0, B, 5):
        assert rob['lam'][KO, b] < cln['lam'][KO, b], (name, b)
        assert np.array_equal(rob['fm'][:, :KO, b], cln['fm'][:, :KO, b])       # (the twin: the same trajectory up to the outlier)
        m, P = rob['fm'][:, KO - 1, b], ino.lower_sym(rob['fP'][..., KO - 1, b])
        m_pr = tfd(m, P, KO)[0]
        plain = rbo.step(m, P, y[:, KO, b], KO, 1, DOF, GQG, alg.r_cov, tfd, tfo)[0]
        assert np.linalg.norm(rob['fm'][:, KO, b] - m_pr) < np.linalg.norm(plain - m_pr), (name, b)
    assert np.all(rob['lam'] > 0.0)


@pytest.mark.parametrize('name', ['pend_gpqkf', 'cv_radar', 'ct_bearing', 'pend_ghkf'])
@pytest.mark.parametrize('J', [1, 4])
def test_7_failed_trajectory_is_a_status_not_a_fault(amd, name, J):
    """One trajectory of 70 starts from P0 = -I (status 1), another has a NaN measurement at step 2 (status 3): NaN outputs from that
    step on; every other trajectory has the bits of a run without them."""
    alg, _, y, _ = case_data(name)
    full = run_case(name, J)
    D, bad, nan_b = full['fm'].shape[0], 37, 11
    P0 = np.broadcast_to(alg.x0_cov, (B, D, D)).copy()
    P0[bad] = -np.eye(D)
    yn = y.copy()
    yn[0, 2, nan_b] = np.nan
    with pytest.raises(np.linalg.LinAlgError):
        alg.robust_pass_batch(yn, dof=DOF, iterations=J, x0_cov=P0)
    out = alg.robust_pass_batch(yn, dof=DOF, iterations=J, x0_cov=P0, raise_on_failure=False, return_weights=True)
    assert alg.status[bad] == 1 and alg.status[nan_b] == 3 and np.count_nonzero(alg.status) == 2
    keep = (np.arange(B) != bad) & (np.arange(B) != nan_b)
    for got, key in zip(out, ('fm', 'fP', 'lam', 'delta')):
        assert np.isnan(got[..., bad]).all() and np.isnan(got[..., 2:, nan_b]).all()
        assert np.array_equal(got[..., :2, nan_b], full[key][..., :2, nan_b])
        assert np.array_equal(got[..., keep], full[key][..., keep])


def test_8_user_pendulum_has_the_bits_of_the_builtin_pair(amd):
    alg, _, y, _ = case_data('user_pend')
    ukf = make_case('pend_ukf')
    assert ukf.robust_kernel_name(4).startswith('k_robust_loop<D=2,Y=1')
    out = ukf.robust_pass_batch(y, dof=DOF, iterations=4, return_weights=True)
    user = run_case('user_pend', 4)
    for got, key in zip(out, ('fm', 'fP', 'lam', 'delta')):
        assert np.array_equal(user[key], got), key
    # the fixed point does something here: the mean of an outlier trajectory moves between J = 1 and J = 4
    assert np.max(np.abs(run_case('user_pend', 1)['fm'][:, KO, ::5] - user['fm'][:, KO, ::5])) > 1e-6


def test_9_refusals_through_the_c_abi_leave_the_outputs_alone(amd):
    """iterations outside 1 .. 64, a dof that is not a positive finite number, an R that is not positive definite (SSMQ_E_ARG) and a
    pair the recursion does not cover (SSMQ_E_UNSUPPORTED) return before an output is touched."""
    from ssmtoybox_amd import _lib, ssinf, ssmod as sm
    from ssmtoybox_amd.mtran import resolve_integrand
    lib = _lib.load()
    alg, _, y, _ = case_data('ungm_ukf')
    cv = case_data('cv_radar')[0]
    na = ssinf.UnscentedKalman(sm.UNGMNATransition(sm.GaussRV(1), sm.GaussRV(1)), sm.UNGMNAMeasurement(sm.GaussRV(1), 1))
    ld, sent = 128, -7.0259e+211
    planes = np.full((16 * T, ld), sent)                                  # (room for fP of D = 4)
    bufs = [_lib.DeviceBuffer(planes.nbytes) for _ in range(5)]          # fm, fP, lam, delta, status
    for b in bufs:
        b.upload(planes)
    d_y, d_m0, d_P0 = _lib.DeviceBuffer(8 * 2 * T * ld), _lib.DeviceBuffer(8 * 4 * ld), _lib.DeviceBuffer(8 * 16 * ld)
    _lib.upload_study(y, 1, ld, d_y)
    d_m0.upload(np.zeros((4, ld)))
    d_P0.upload(np.ones((16, ld)))

    def call(a, iterations, dof, R, flags=0):
        f_dyn, e_dyn = resolve_integrand(a.mod_dyn.dyn_eval)
        f_obs, e_obs = resolve_integrand(a.mod_obs.meas_eval)
        gqg, pg = _lib.as_c(a.G.dot(a.q_cov).dot(a.G.T))
        rr, pr = _lib.as_c(np.asarray(R, dtype=float))
        vp = lambda b: ctypes.c_void_p(b.ptr)       # noqa: E731
        return lib.ssmq_filter_robust_dev(ctypes.c_void_p(a.tf_dyn._handle_for(e_dyn)), ctypes.byref(f_dyn),
                                          ctypes.c_void_p(a.tf_obs._handle_for(e_obs)), ctypes.byref(f_obs), B, ld, T, iterations, flags,
                                          vp(d_y), vp(d_m0), vp(d_P0), pg, pr, dof, vp(bufs[0]), vp(bufs[1]), vp(bufs[2]), vp(bufs[3]),
                                          vp(bufs[4]))
    one = np.eye(1)
    assert call(alg, 0, DOF, one) == -1 and 'iterations' in _lib.last_error()
    assert call(alg, 65, DOF, one) == -1 and call(alg, 2, DOF, one, flags=2) == -1
    for dof in (0.0, -1.0, np.nan, np.inf):
        assert call(alg, 2, dof, one) == -1 and 'dof' in _lib.last_error()
    for R in ([[0.0]], [[-1.0]], [[np.nan]]):
        assert call(alg, 2, DOF, R) == -1 and 'positive definite' in _lib.last_error()
    for R in ([[1.0, 2.0], [2.0, 1.0]], [[1.0, 0.5], [0.4, 1.0]]):        # indefinite; not symmetric
        assert call(cv, 2, DOF, R) == -1 and 'positive definite' in _lib.last_error()
    assert call(na, 2, DOF, one) == -3 and 'additive' in _lib.last_error()
    _lib.sync()
    for b in bufs:
        assert np.array_equal(b.download(planes.shape), planes)
    # ... and the accepted call writes lanes 0 .. B - 1 of every plane and leaves the padding lanes alone
    assert call(alg, 4, DOF, one) == 0
    _lib.sync()
    ref = run_case('ungm_ukf', 4)
    for buf, key in ((bufs[0], 'fm'), (bufs[2], 'lam'), (bufs[3], 'delta')):
        got = buf.download(planes.shape)[:T]
        assert np.array_equal(got[:, :B], ref[key].reshape(T, B)) and np.all(got[:, B:] == sent), key
    for b in bufs + [d_y, d_m0, d_P0]:
        b.free()
