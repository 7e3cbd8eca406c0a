"""The iterated posterior linearisation pass (IPLF) on the device against its NumPy restatement (tests/_iterated_oracle.py):
k_iplf_loop<> for the table shapes and a user pair, the launch loop (apply dyn | J x (apply obs | k_iplf_update)) for the other forms.
B = 70 (one full block of 64 lanes and a partial one), T = 6.

Bound.  Every step is compared with the one-step restatement started from the DEVICE's filtered moments of the step before, by
assert_moments_close with rtol = max(RTOL, 64 eps sum_i (cond P_i + cond S_i)): the project's bound for one application of an inverse
(tests/test_gpu_parity.py), summed over the 2 J applications of a step (P_i^-1 and S^-1 per iteration), the condition numbers from the
restatement's own iterates.  delta = max_d |m_J - m_{J-1}| / sqrt(P_J[d, d]) under the same bound: both means are within rtol ms (ms:
the mean scale of assert_moments_close) and P_J[d, d] within rtol cs, so |delta error| <= rtol (2 ms / s + delta cs / (2 s^2)) with
s^2 the smallest diagonal entry of P_J.  No case needed more than this bound (MEASURED is empty; the procedure for one that does -
4 x the float64 restatement's own error against its long-double form - is helper_error_of)."""
import ctypes

import numpy as np
import pytest

from tests import _innovation_oracle as ino
from tests import _iterated_oracle as ito
from tests._cases import RTOL, moment_scales
from tests.test_innovation_gpu import oracle_tf, simulate
from tests.test_innovation_host import pendulum_user

pytestmark = pytest.mark.gpu
EPS = float(np.finfo(float).eps)
B, T = 70, 6


@pytest.fixture(scope='module')
def amd():
    import ssmtoybox_amd
    if ssmtoybox_amd.device_count() < 1:
        pytest.fail('no device: the GPU tests need an MI355X')
    ssmtoybox_amd.set_device(0)
    return ssmtoybox_amd


def make_case(name):
    from ssmtoybox_amd import ssinf, ssmod as sm
    if name == 'ungm_ukf':
        dyn = sm.UNGMTransition(sm.GaussRV(1), sm.GaussRV(1, cov=np.array([[10.0]])))
        return ssinf.UnscentedKalman(dyn, sm.UNGMMeasurement(sm.GaussRV(1), 1))
    if name.startswith('pend') or name == 'user_pend':
        m0, P0 = np.array([1.5, 0.0]), 0.01 * np.eye(2)
        Q = 0.01 * np.array([[0.01 ** 3 / 3, 0.01 ** 2 / 2], [0.01 ** 2 / 2, 0.01]])
        Dyn, Obs = pendulum_user() if name == 'user_pend' else (sm.Pendulum2DTransition, sm.Pendulum2DMeasurement)
        dyn, obs = Dyn(sm.GaussRV(2, m0, P0), sm.GaussRV(2, cov=Q)), Obs(sm.GaussRV(1, cov=np.array([[0.1]])), 2)
        par = np.array([[1.0, 2.0, 2.0]])
        return {'pend_ukf': lambda: ssinf.UnscentedKalman(dyn, obs), 'user_pend': lambda: ssinf.UnscentedKalman(dyn, obs),
                'pend_gpqkf': lambda: ssinf.GaussianProcessKalman(dyn, obs, par, par, 'rbf', 'ut'),
                'pend_tpqkf': lambda: ssinf.StudentProcessKalman(dyn, obs, par, par, 'rbf', 'ut', nu=4.0),
                'pend_ghkf': lambda: ssinf.GaussHermiteKalman(dyn, obs, deg=3), 'pend_ekf': lambda: ssinf.ExtendedKalman(dyn, obs)}[name]()
    if name == 'reentry1d_ckf':
        m0, P0 = np.array([90.0, 6.0, 1.7]), np.diag([0.3048 ** 2, 1.2192 ** 2, 0.01])
        dyn = sm.ReentryVehicle1DTransition(sm.GaussRV(3, m0, P0), sm.GaussRV(3, cov=1e-6 * np.eye(3)))
        return ssinf.CubatureKalman(dyn, sm.RangeMeasurement(sm.GaussRV(1, cov=np.array([[0.03048 ** 2]])), 3))
    if name == 'cv_radar':
        dyn = sm.ConstantVelocity(sm.GaussRV(4, np.array([100.0, 5.0, 200.0, -3.0]), np.diag([1.0, 0.1, 1.0, 0.1])), sm.GaussRV(2, cov=0.1 * np.eye(2)))
        return ssinf.UnscentedKalman(dyn, sm.Radar2DMeasurement(sm.GaussRV(2, cov=np.diag([0.5, 1e-4])), 4))
    if name == 'ct_bearing':
        m0 = np.array([130.0, 35.0, -20.0, 20.0, -4 * np.pi / 180])
        dyn = sm.CoordinatedTurnTransition(sm.GaussRV(5, m0, np.diag([5.0, 5.0, 5.0, 5.0, 1e-4])), sm.GaussRV(5, cov=np.diag([0.1, 0.1, 0.1, 0.1, 1e-6])))
        sensors = np.vstack((1000 * np.eye(2), -1000 * np.eye(2))).astype(float)
        return ssinf.UnscentedKalman(dyn, sm.BearingMeasurement(sm.GaussRV(4, cov=1e-4 * np.eye(4)), 5, state_index=[0, 2], sensor_pos=sensors))
    if name == 'reentry2d_ukf':
        m0 = np.array([6500.4, 349.14, -1.8093, -6.7967, 0.6932])
        dyn = sm.ReentryVehicle2DTransition(sm.GaussRV(5, m0, np.diag([1e-6, 1e-6, 1e-6, 1e-6, 1.0])),
                                            sm.GaussRV(3, cov=np.diag([2.4064e-5, 2.4064e-5, 1e-6])))
        return ssinf.UnscentedKalman(dyn, sm.Radar2DMeasurement(sm.GaussRV(2, cov=np.diag([1e-6, 0.17e-3 ** 2])), 5, radar_loc=np.array([6374.0, 0.0])))
    raise KeyError(name)


ONE_LAUNCH = ('ungm_ukf', 'pend_gpqkf', 'pend_tpqkf', 'reentry1d_ckf', 'cv_radar', 'ct_bearing', 'reentry2d_ukf', 'user_pend')
LOOP = ('pend_ghkf', 'pend_ekf')
MEASURED = ()            # cases whose bound is 4 x the float64 restatement's own error (none)
_DATA, _RUNS, _REFS = {}, {}, {}


def case_tf(tf, model_eval):
    """oracle_tf of the innovation tests; the t-process transforms of StudentProcessKalman with their broadcast model variance."""
    from ssmtoybox_amd import mtran
    from ssmtoybox_amd.bq import bqmtran
    if not isinstance(tf, bqmtran.StudentTProcessTransform):
        return oracle_tf(tf, model_eval)
    f, _ = mtran.resolve_integrand(model_eval)
    w = dict(wm=tf.wm, Wc=tf.Wc, Wcc=tf.Wcc, model_var=tf.model.model_var, iK=tf.model.iK)
    return ito.tp_broadcast_tf(f.id, tuple(f.par[i] for i in range(f.n_par)), tf.model.points, w, tf.model.nu,
                               tuple(f.idx[i] for i in range(f.n_idx)) if f.n_idx else None)


def case_data(name):
    """(filter, the built-in twin the restatement evaluates, measurements (Y, T, B)): made once, never modified."""
    if name not in _DATA:
        alg = make_case(name)
        twin = make_case('pend_ukf') if name == 'user_pend' else alg
        _DATA[name] = (alg, twin, simulate(twin, B, T, 3))
    return _DATA[name]


def run_case(name, J, **kw):
    """The case on the device: fm (D, T, B), fP (D, D, T, B), delta (T, B), status.  Shared by the tests, never modified."""
    key = (name, J) + tuple(sorted(kw.items()))
    if key not in _RUNS:
        alg, _, y = case_data(name)
        fm, fP, delta = alg.iterated_pass_batch(y, J, raise_on_failure=False, return_delta=True, **kw)
        _RUNS[key] = dict(fm=fm, fP=fP, delta=delta, status=alg.status.copy())
    return _RUNS[key]


def restated(name, J, run):
    """The one-step restatement of every (k, b) from the device's moments of step k - 1: list over b of lists over k."""
    key = (name, J, id(run))
    if key not in _REFS:
        alg, twin, y = case_data(name)
        tfd, tfo = case_tf(alg.tf_dyn, twin.mod_dyn.dyn_eval), case_tf(alg.tf_obs, twin.mod_obs.meas_eval)
        GQG = alg.G.dot(alg.q_cov).dot(alg.G.T)
        out = []
        for b in range(B):
            rows = []
            for k in range(T):
                m, P = (alg.x0_mean, alg.x0_cov) if k == 0 else (run['fm'][:, k - 1, b], run['fP'][..., k - 1, b])
                rows.append((m, P) + ito.step(m, P, y[:, k, b], k, J, GQG, alg.r_cov, tfd, tfo))
            out.append(rows)
        _REFS[key] = out
    return _REFS[key]


def helper_error_of(name, J, run):
    """max |float64 restatement - long-double restatement| of (mean / ms, covariance / cs, delta) over a MEASURED case."""
    if name not in MEASURED:
        return np.zeros(3)
    from ssmtoybox_amd import mtran
    alg, twin, y = case_data(name)
    tfs = []
    for tf, ev in ((alg.tf_dyn, twin.mod_dyn.dyn_eval), (alg.tf_obs, twin.mod_obs.meas_eval)):
        f, _ = mtran.resolve_integrand(ev)
        tfs.append(ino.sigma_tf_ld(f.id, tuple(f.par[i] for i in range(f.n_par)), tf.unit_sp, tf.wm, np.diag(tf.Wc),
                                   tuple(f.idx[i] for i in range(f.n_idx)) if f.n_idx else None))
    GQG = alg.G.dot(alg.q_cov).dot(alg.G.T)
    worst = np.zeros(3)
    for b, rows in enumerate(restated(name, J, run)):
        for k, (m, P, mj, Pj, dj, conds) in enumerate(rows):
            ml, Pl, dl = ito.step_ld(m, P, y[:, k, b], k, J, GQG, alg.r_cov, tfs[0], tfs[1])
            ms, cs, _ = moment_scales(mj, Pj, np.zeros((1, 1)), P)
            worst = np.maximum(worst, [float(np.max(np.abs(mj - ml))) / ms, float(np.max(np.abs(Pj - Pl))) / cs, float(abs(dj - dl))])
    print('float64 restatement against long double {} J = {}: mean {:.3g}, cov {:.3g}, delta {:.3g}'.format(name, J, *worst))
    return worst


def check_against(run, ref_rows, what, helper_err=np.zeros(3)):
    """Every (k, b) of `run` against the restatement rows (m_in, P_in, m_J, P_J, delta, conds); prints the largest error / bound."""
    worst = np.zeros(3)
    for b, rows in enumerate(ref_rows):
        for k, (m, P, mj, Pj, dj, conds) in enumerate(rows):
            assert conds is not None, (what, b, k)
            rtol = max(RTOL, 64.0 * EPS * sum(conds))
            ms, cs, _ = moment_scales(mj, Pj, np.zeros((1, 1)), P)
            gm, gP, gd = run['fm'][:, k, b], run['fP'][..., k, b], run['delta'][k, b]
            assert np.all(np.isfinite(gm)) and np.all(np.isfinite(gP)) and np.isfinite(gd), (what, b, k)
            s2 = float(np.min(np.diag(Pj)))
            dtol = max(rtol, 4.0 * helper_err[0], 4.0 * helper_err[1]) * (2.0 * ms / np.sqrt(s2) + dj * cs / (2.0 * s2))
            e = [float(np.max(np.abs(gm - mj))) / ms / max(rtol, 4.0 * helper_err[0]), float(np.max(np.abs(gP - Pj))) / cs / max(rtol, 4.0 * helper_err[1]),
                 abs(gd - dj) / max(dtol, 4.0 * helper_err[2])]
            worst = np.maximum(worst, e)
    print('iterated pass {}: largest error / bound: mean {:.3g}, cov {:.3g}, delta {:.3g}'.format(what, *worst))
    assert np.all(worst <= 1.0), (what, worst)


@pytest.mark.parametrize('J', [1, 3])
@pytest.mark.parametrize('name', ONE_LAUNCH + LOOP)
def test_1_every_step_against_the_restatement(amd, name, J):
    alg = case_data(name)[0]
    kn = alg.iterated_kernel_name(J)
    assert kn.startswith('k_iplf_loop<') if name in ONE_LAUNCH else kn.startswith('launch loop'), kn
    assert ('run-time compiled' in kn) == (name == 'user_pend')
    run = run_case(name, J)
    assert run['status'].dtype == np.int32 and not run['status'].any()
    for b in range(B):     # both triangles are written from one value
        assert np.array_equal(run['fP'][..., b], run['fP'][..., b].transpose(1, 0, 2))
    check_against(run, restated(name, J, run), '{} J = {}'.format(name, J), helper_error_of(name, J, run))


def check_step_twin(name, J, run, one_step, what):
    """Step k of `run` against one_step(y_k (Y, 1, B), m (B, D), P (B, D, D)) -> (fm (D, 1, B), fP (D, D, 1, B)) started from the
    run's own moments of step k - 1, under the bound of the restatement's iterates for that step.  A pass of one step uses time
    index 0: every step of a model without time dependence, step 0 alone of UNGM."""
    alg, _, y = case_data(name)
    rows = restated(name, J, run)
    D = run['fm'].shape[0]
    worst = 0.0
    for k in range(1 if name.startswith('ungm') else T):
        m0 = np.broadcast_to(alg.x0_mean, (B, D)) if k == 0 else run['fm'][:, k - 1, :].T
        P0 = np.broadcast_to(alg.x0_cov, (B, D, D)) if k == 0 else run['fP'][..., k - 1, :].transpose(2, 0, 1)
        fm, fP = one_step(y[:, k:k + 1, :], np.ascontiguousarray(m0), np.ascontiguousarray(P0))
        assert not alg.status.any()
        for b in range(B):
            m, P, mj, Pj, dj, conds = rows[b][k]
            rtol = max(RTOL, 64.0 * EPS * sum(conds))
            ms, cs, _ = moment_scales(mj, Pj, np.zeros((1, 1)), P)
            worst = max(worst, float(np.max(np.abs(run['fm'][:, k, b] - fm[:, 0, b]))) / ms / rtol,
                        float(np.max(np.abs(run['fP'][..., k, b] - ino.lower_sym(fP[..., 0, b])))) / cs / rtol)
    print('{} {}: largest error / bound = {:.3g}'.format(what, name, worst))
    assert worst <= 1.0, (what, name, worst)


@pytest.mark.parametrize('name', ['ungm_ukf', 'pend_gpqkf', 'cv_radar', 'ct_bearing', 'pend_ghkf', 'pend_ekf'])
def test_2_one_iteration_is_the_forward_pass(amd, name):
    alg = case_data(name)[0]
    check_step_twin(name, 1, run_case(name, 1), lambda yk, m, P: alg.forward_pass_batch(yk, x0_mean=m, x0_cov=P, raise_on_failure=False),
                    'iterated pass J = 1 against forward_pass_batch')


@pytest.mark.parametrize('name', ['ungm_ukf', 'pend_gpqkf', 'cv_radar', 'ct_bearing'])
def test_3_launch_loop_flag_agrees_with_the_one_launch_kernel(amd, name):
    alg = case_data(name)[0]
    assert alg.iterated_kernel_name(3).startswith('k_iplf_loop<') and alg.iterated_kernel_name(3, launch_loop=True).startswith('launch loop')
    # the whole pass through the loop, every step against the restatement started from the loop's own moments ...
    loop = run_case(name, 3, launch_loop=True)
    assert not loop['status'].any()
    check_against(loop, restated(name, 3, loop), name + ' J = 3 (launch loop)')
    # ... and the two routes against each other, step by step from the one-launch kernel's moments
    check_step_twin(name, 3, run_case(name, 3), lambda yk, m, P: alg.iterated_pass_batch(yk, 3, x0_mean=m, x0_cov=P, raise_on_failure=False,
                                                                                          launch_loop=True),
                    'one launch against the launch loop, J = 3')


@pytest.mark.parametrize('name', ['pend_gpqkf', 'cv_radar', 'pend_ghkf'])
def test_4_batch_independence_and_the_device_route(amd, name):
    """B = 70 against the slices 0:64 and 64:70, and iterated_pass_dev against iterated_pass_batch: equal bits."""
    from ssmtoybox_amd import _lib
    alg, _, y = case_data(name)
    full = run_case(name, 3)
    for sl in (slice(0, 64), slice(64, 70)):
        fm, fP, delta = alg.iterated_pass_batch(y[..., sl], 3, raise_on_failure=False, return_delta=True)
        assert np.array_equal(fm, full['fm'][..., sl]) and np.array_equal(fP, full['fP'][..., sl]) and np.array_equal(delta, full['delta'][..., sl])
        assert not alg.status.any()
    Y, D, ld = y.shape[0], full['fm'].shape[0], 128
    d_y = _lib.DeviceBuffer(8 * T * Y * ld)
    _lib.upload_study(y, Y, ld, d_y)
    d_fm, d_fP, d_delta, d_st = alg.iterated_pass_dev(d_y, B, ld, T, 3)
    assert np.array_equal(d_fm.download((T, D, ld))[:, :, :B].transpose(1, 0, 2), full['fm'])
    assert np.array_equal(d_fP.download((T, D, D, ld))[..., :B].transpose(1, 2, 0, 3), full['fP'])
    assert np.array_equal(d_delta.download((T, ld))[:, :B], full['delta'])
    assert not d_st.download((ld,), dtype=np.int32)[:B].any()
    for buf in (d_y, d_fm, d_fP, d_delta, d_st):
        buf.free()
    one = alg.iterated_pass(y[..., 5], 3)
    assert np.array_equal(one[0], full['fm'][..., 5]) and np.array_equal(one[1], full['fP'][..., 5])


@pytest.mark.parametrize('name', ['pend_gpqkf', 'cv_radar', 'pend_ghkf'])
def test_5_failed_trajectory_is_a_status_not_a_fault(amd, name):
    """One trajectory of 70 starts from P0 = -I: status 1, NaN outputs; every other trajectory has the bits of a run without it."""
    alg, _, y = case_data(name)
    full = run_case(name, 3)
    D, bad = full['fm'].shape[0], 37
    P0 = np.broadcast_to(alg.x0_cov, (B, D, D)).copy()
    P0[bad] = -np.eye(D)
    with pytest.raises(np.linalg.LinAlgError):
        alg.iterated_pass_batch(y, 3, x0_cov=P0)
    fm, fP, delta = alg.iterated_pass_batch(y, 3, x0_cov=P0, raise_on_failure=False, return_delta=True)
    assert alg.status[bad] == 1 and np.count_nonzero(alg.status) == 1
    keep = np.arange(B) != bad
    for got, ref in ((fm, full['fm']), (fP, full['fP']), (delta, full['delta'])):
        assert np.isnan(got[..., bad]).all()
        assert np.array_equal(got[..., keep], ref[..., keep])


def test_6_user_pendulum_against_the_builtin_pair(amd):
    """As tests/test_user_models_gpu.py: rel_err < 1e-12 between the run-time compiled pair and the table kernel of the same models."""
    alg, _, y = case_data('pend_ukf')
    assert alg.iterated_kernel_name(3).startswith('k_iplf_loop<D=2,Y=1')
    fm, fP, delta = alg.iterated_pass_batch(y, 3, return_delta=True)
    user = run_case('user_pend', 3)

    def rel_err(a, b):
        return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))
    assert rel_err(user['fm'], fm) < 1e-12 and rel_err(user['fP'], fP) < 1e-12 and rel_err(user['delta'], delta) < 1e-12
    # iterating does something here: the mean moves between J = 1 and J = 3
    assert np.max(np.abs(run_case('user_pend', 1)['fm'] - user['fm'])) > 1e-6


def test_7_refusals_through_the_c_abi_leave_the_outputs_alone(amd):
    """iterations outside 1 .. 64 (SSMQ_E_ARG) and a pair the recursion does not cover (SSMQ_E_UNSUPPORTED: transforms of models that
    take their noise as an argument, the refusal of ssmq_filter_innovations_dev) return before an output is touched.  The handles of
    a Studentian filter are ordinary sigma-point handles - the C ABI cannot tell them apart, so that refusal is made and tested at
    the Python layer (tests/test_iterated_host.py), and here only that it writes nothing either."""
    from ssmtoybox_amd import _lib, ssinf, ssmod as sm
    from ssmtoybox_amd.mtran import resolve_integrand
    lib = _lib.load()
    alg, _, y = case_data('ungm_ukf')
    na = ssinf.UnscentedKalman(sm.UNGMNATransition(sm.GaussRV(1), sm.GaussRV(1)), sm.UNGMNAMeasurement(sm.GaussRV(1), 1))
    dyn_s = sm.UNGMTransition(sm.StudentRV(1, dof=4.0), sm.StudentRV(1, dof=4.0))
    stu = ssinf.FullySymmetricStudent(dyn_s, sm.UNGMMeasurement(sm.StudentRV(1, dof=4.0), 1))
    ld, sent = 128, -7.0259e+211
    planes = np.full((T, ld), sent)
    bufs = [_lib.DeviceBuffer(planes.nbytes) for _ in range(4)]          # fm, fP, delta, status (D = 1)
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
        return lib.ssmq_filter_iterated_dev(ctypes.c_void_p(a.tf_dyn._handle_for(e_dyn)), ctypes.byref(f_dyn),
                                            ctypes.c_void_p(a.tf_obs._handle_for(e_obs)), ctypes.byref(f_obs), B, ld, T, iterations, flags,
                                            vp(d_y), vp(d_m0), vp(d_P0), pg, pr, vp(bufs[0]), vp(bufs[1]), vp(bufs[2]), vp(bufs[3]))
    assert call(alg, 0) == -1 and 'iterations' in _lib.last_error()
    assert call(alg, 65) == -1 and call(alg, 2, flags=2) == -1
    assert call(na, 2) == -3 and 'additive' in _lib.last_error()
    with pytest.raises(NotImplementedError, match='Studentian'):
        stu.iterated_pass_dev(d_y, B, ld, T, 2)
    _lib.sync()
    for b in bufs:
        assert np.array_equal(b.download(planes.shape), planes)
    # ... and the accepted call writes lanes 0 .. B - 1 of every plane and leaves the padding lanes alone
    assert call(alg, 2) == 0
    _lib.sync()
    ref = run_case('ungm_ukf', 2)
    got = bufs[0].download(planes.shape)
    assert np.array_equal(got[:, :B], ref['fm'][0]) and np.all(got[:, B:] == sent)
    assert np.array_equal(bufs[2].download(planes.shape)[:, :B], ref['delta'])
    for b in bufs + [d_y, d_m0, d_P0]:
        b.free()
