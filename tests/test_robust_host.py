"""Outlier-robust pass, the parts that need no device: the NumPy restatement (tests/_robust_oracle.py) in its measurement-space and
state-space forms, at one iteration against the oracle's own Gaussian filter, at dof = 1e300 against one iteration, on a linear model
against the Kalman filter; the behaviour of the weight; the study gap on the restatement; the exported entry points, the run-time
compile of k_robust_loop<> for a user pendulum pair, and the refusals that come before the library is touched."""
import ctypes
import os

import numpy as np
import pytest

from oracle import ssmq_oracle as orc
from tests import _innovation_oracle as ino
from tests import _robust_oracle as rbo
from tests._cases import moment_scales
from tests.test_innovation_host import pendulum_user
from tests.test_iterated_host import _measurements, _pendulum, _ungm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = float(np.finfo(float).eps)


def _pendulum_gpq():
    """The pendulum with GP quadrature transforms on unscented points (2, 1, 5)."""
    c = _pendulum()
    pts, par = orc.points_ut(2), np.array([[1.0, 2.0, 2.0]])
    w = orc.gp_weights(par, pts)
    c['tfd'], c['tfo'] = ino.bq_tf(orc.F_PENDULUM_DYN, (0.01,), pts, w), ino.bq_tf(orc.F_PENDULUM_MEAS, (), pts, w, (0,))
    return c


def _with_outliers(c, T, rng):
    """Measurements of the model with a gross outlier (+ 1e3 sqrt(R_aa)) in every fifth step."""
    y = _measurements(c, T, rng)
    y[:, 3::5] += 1e3 * np.sqrt(np.diag(c['R']))[:, None]
    return y


@pytest.mark.parametrize('J', [1, 3, 8])
@pytest.mark.parametrize('case', [_ungm, _pendulum_gpq])
def test_measurement_space_and_state_space_forms_agree(case, J):
    """Every step from the same moments, dof = 4: mean, covariance and weight within 64 eps (cond P- + sum_i cond S_i) relative to the
    scales of the step - the project's bound for one application of an inverse (tests/test_iterated_gpu.py), summed over the
    inverses of the two forms (P-^-1 in the state-space form alone, S_i^-1 in both).  Scales: moment_scales for mean and covariance,
    as there, plus what the weight's own error moves them by (tests/_robust_oracle.py: step, scales); for the weight the error scale
    of weight_step (gamma is a sum that cancels).  The state-space form conditions the residual
    of the statistical linearisation, w ~ N(0, Omega), on y together with x (tests/_robust_oracle.py: step_state_space): with the
    residual left at its prior - Psi = (y - y^ - A (m_i - m-)) (..)' + A P_i A' + Omega read literally - the two forms are the same
    numbers on a linear model alone (test_linear_model_...), and on these two cases the weights of J = 3 differ in the first digits
    (printed below)."""
    c, rng, T = case(), np.random.default_rng(21), 12
    worst, literal = 0.0, 0.0
    for _ in range(4):
        y = _with_outliers(c, T, rng)
        fm, fP = rbo.robust_filter(y, c['m0'], c['P0'], J, 4.0, c['Q'], c['R'], c['tfd'], c['tfo'])[:2]
        assert np.all(np.isfinite(fm))
        for k in range(T):
            m, P = (c['m0'], c['P0']) if k == 0 else (fm[:, k - 1], fP[..., k - 1])
            a = rbo.step(m, P, y[:, k], k, J, 4.0, c['Q'], c['R'], c['tfd'], c['tfo'])
            b = rbo.step_state_space(m, P, y[:, k], k, J, 4.0, c['Q'], c['R'], c['tfd'], c['tfo'])
            assert a[4] is not None and len(a[4]) == J + 1
            tol = 64.0 * EPS * sum(a[4])
            ms, cs, _ = moment_scales(a[0], a[1], np.zeros((1, 1)), P)
            ws, dm, dP = a[5]
            worst = max(worst, float(np.max(np.abs(a[0] - b[0]))) / (ms + ws * dm) / tol, float(np.max(np.abs(a[1] - b[1]))) / (cs + ws * dP) / tol,
                        abs(a[2] - b[2]) / max(ws, 1e-300) / tol if J > 1 else float(a[2] != b[2]))
            lit = rbo.step_state_space(m, P, y[:, k], k, J, 4.0, c['Q'], c['R'], c['tfd'], c['tfo'], literal=True)
            literal = max(literal, abs(a[2] - lit[2]) / a[2])
    print('measurement-space against state-space form, J = {}: largest error / bound = {:.3g}; residual at its prior: weights differ by '
          '{:.3g} relative'.format(J, worst, literal))
    assert worst <= 1.0, worst


@pytest.mark.parametrize('case', [_ungm, _pendulum])
def test_one_iteration_is_the_gaussian_filter(case):
    """J = 1 against orc.gaussian_filter, every step from the filter's own moments of the step before: 1e-12 relative to
    max(1, |value|), the bar of tests/test_iterated_host.py; lam = 1 and delta = 0 exactly."""
    c, rng, T = case(), np.random.default_rng(11), 20
    D = c['m0'].shape[0]
    worst = 0.0
    for _ in range(8):
        y = _measurements(c, T, rng)
        fm, fP = orc.gaussian_filter(y, c['m0'], c['P0'], c['Q'], c['R'], np.eye(D), c['tfd'], c['tfo'])[:2]
        for k in range(T):
            m, P = (c['m0'], c['P0']) if k == 0 else (fm[:, k - 1], fP[..., k - 1])
            mj, Pj, lam, delta, conds, _ = rbo.step(m, P, y[:, k], k, 1, 4.0, c['Q'], c['R'], c['tfd'], c['tfo'])
            assert conds is not None and len(conds) == 2 and lam == 1.0 and delta == 0.0
            worst = max(worst, float(np.max(np.abs(mj - fm[:, k]) / np.maximum(1.0, np.abs(fm[:, k])))),
                        float(np.max(np.abs(Pj - ino.lower_sym(fP[..., k])) / np.maximum(1.0, np.abs(fP[..., k])))))
    print('restatement at J = 1 against orc.gaussian_filter: {:.3g}'.format(worst))
    assert worst <= 1e-12, worst


@pytest.mark.parametrize('case', [_ungm, _pendulum_gpq])
def test_huge_dof_gives_the_bits_of_one_iteration(case):
    """dof = 1e300: dof + Y == dof + gamma == dof, so every weight is exactly 1.0 and J = 5 has the bits of J = 1."""
    c, rng = case(), np.random.default_rng(13)
    y = _with_outliers(c, 12, rng)
    a = rbo.robust_filter(y, c['m0'], c['P0'], 1, 1e300, c['Q'], c['R'], c['tfd'], c['tfo'])
    b = rbo.robust_filter(y, c['m0'], c['P0'], 5, 1e300, c['Q'], c['R'], c['tfd'], c['tfo'])
    assert np.all(np.isfinite(a[0]))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.all(b[2] == 1.0) and np.all(b[3] == 0.0)
    # ... and the long-double restatement of a step agrees with the float64 one to rounding at dof = 4
    pts, (wm, wc) = orc.points_ut(1), orc.weights_ut(1)[:2]
    u = _ungm()
    tfd, tfo = ino.sigma_tf_ld(orc.F_UNGM_DYN, (), pts, wm, wc), ino.sigma_tf_ld(orc.F_UNGM_MEAS, (), pts, wm, wc)
    yu = _with_outliers(u, 4, rng)
    m64, P64, l64, d64, _, _ = rbo.step(u['m0'], u['P0'], yu[:, 3], 3, 4, 4.0, u['Q'], u['R'], u['tfd'], u['tfo'])
    mld, Pld, lld, dld = rbo.step_ld(u['m0'], u['P0'], yu[:, 3], 3, 4, 4.0, u['Q'], u['R'], tfd, tfo)
    assert abs(float(mld[0]) - m64[0]) <= 1e-12 * max(1.0, abs(m64[0])) and abs(float(Pld[0, 0]) - P64[0, 0]) <= 1e-12 * max(1.0, P64[0, 0])
    assert abs(float(lld) - l64) <= 1e-10 * l64 and abs(float(dld) - d64) <= 1e-8 * max(1.0, d64)
    # a covariance that is not positive definite, or a NaN measurement, gives NaN rows from that step on
    fm, fP, lam, delta = rbo.robust_filter(y, c['m0'], -np.eye(c['m0'].shape[0]), 2, 4.0, c['Q'], c['R'], c['tfd'], c['tfo'])
    assert np.isnan(fm).all() and np.isnan(fP).all() and np.isnan(lam).all() and np.isnan(delta).all()
    yn = y.copy()
    yn[0, 5] = np.nan
    fm = rbo.robust_filter(yn, c['m0'], c['P0'], 2, 4.0, c['Q'], c['R'], c['tfd'], c['tfo'])[0]
    assert np.all(np.isfinite(fm[:, :5])) and np.isnan(fm[:, 5:]).all()


# ---- a linear model: constant velocity, positions measured ----------------------------------------------------------------------
def _linear_cv(dt=1.0, q=0.05):
    F = np.array([[1, dt, 0, 0], [0, 1, 0, 0], [0, 0, 1, dt], [0, 0, 0, 1]], dtype=float)
    H = np.array([[1, 0, 0, 0], [0, 0, 1, 0]], dtype=float)
    G = np.array([[dt ** 2 / 2, 0], [dt, 0], [0, dt ** 2 / 2], [0, dt]])
    return dict(F=F, H=H, GQG=q * G.dot(G.T), R=np.eye(2), m0=np.array([0.0, 1.0, 0.0, -1.0]), P0=np.diag([1.0, 0.1, 1.0, 0.1]),
                tfd=lambda m, P, t: (F.dot(m), F.dot(P).dot(F.T), F.dot(P)), tfo=lambda m, P, t: (H.dot(m), H.dot(P).dot(H.T), H.dot(P)))


def _simulate_cv(c, B, T, dof, rng):
    """x (4, T, B), y (2, T, B): Gaussian initial state and process noise (G q of rank 2), t_dof measurement noise of scale R."""
    Lq = np.linalg.cholesky(c['GQG'] + 1e-12 * np.eye(4))
    x = c['m0'][:, None] + np.linalg.cholesky(c['P0']).dot(rng.standard_normal((4, B)))
    xs, ys = np.zeros((4, T, B)), np.zeros((2, T, B))
    for k in range(T):
        x = c['F'].dot(x) + Lq.dot(rng.standard_normal((4, B)))
        u = rng.chisquare(dof, B) / dof
        xs[:, k], ys[:, k] = x, c['H'].dot(x) + np.linalg.cholesky(c['R']).dot(rng.standard_normal((2, B))) / np.sqrt(u)
    return xs, ys


def test_linear_model_with_huge_dof_is_the_kalman_filter():
    c, rng, T = _linear_cv(), np.random.default_rng(5), 15
    _, y = _simulate_cv(c, 3, T, 3.0, rng)
    for b in range(3):
        fm, fP, lam, _ = rbo.robust_filter(y[..., b], c['m0'], c['P0'], 5, 1e300, c['GQG'], c['R'], c['tfd'], c['tfo'])
        m, P = c['m0'], c['P0']
        for k in range(T):
            m, P = c['F'].dot(m), c['F'].dot(P).dot(c['F'].T) + c['GQG']
            S = c['H'].dot(P).dot(c['H'].T) + c['R']
            K = P.dot(c['H'].T).dot(np.linalg.inv(S))
            m, P = m + K.dot(y[:, k, b] - c['H'].dot(m)), P - K.dot(S).dot(K.T)
            assert np.allclose(fm[:, k], m, rtol=1e-11, atol=1e-11) and np.allclose(fP[..., k], P, rtol=1e-11, atol=1e-11)
        assert np.all(lam == 1.0)
    # Omega = 0 here: both readings of the state-space form give the weights of the measurement-space form, at every iteration
    for literal in (False, True):
        a = rbo.step(c['m0'], c['P0'], y[:, 0, 0] + 30.0, 0, 8, 3.0, c['GQG'], c['R'], c['tfd'], c['tfo'])
        b = rbo.step_state_space(c['m0'], c['P0'], y[:, 0, 0] + 30.0, 0, 8, 3.0, c['GQG'], c['R'], c['tfd'], c['tfo'], literal=literal)
        assert abs(a[2] - b[2]) <= 1e-9 * a[2] and np.allclose(a[0], b[0], rtol=1e-9, atol=1e-9) and a[2] < 0.1


def test_the_weight_is_at_most_one_for_a_surprising_measurement_and_falls_with_the_innovation():
    """lambda_{i+1} = (dof + Y) / (dof + gamma) <= 1 exactly when gamma >= Y; along a ray e = s e0 the weight after 8 rounds falls as
    s grows."""
    c = _linear_cv()
    m_pr, P_pr, _ = c['tfd'](c['m0'], c['P0'], 0)
    P_pr = P_pr + c['GQG']
    yh, Ph, _ = c['tfo'](m_pr, P_pr, 0)
    R, iR, e0 = c['R'], np.linalg.inv(c['R']), np.array([0.6, -0.8])
    seen = [False, False]
    last = np.inf
    for s in (0.01, 0.1, 0.5, 1.0, 2.0, 4.0, 8.0, 30.0, 1e3):
        lam = 1.0
        for _ in range(8):
            lam, gamma, _, _ = rbo.weight_step(lam, s * e0, Ph, R, iR, 4.0)
            assert (lam <= 1.0) == (gamma >= 2.0)
            seen[int(gamma >= 2.0)] = True
        assert 0.0 < lam < last
        last = lam
    assert all(seen) and last < 1e-4
    # the same through `step`: the outlier's weight is far below its clean twin's, and its posterior stays nearer the prior
    y = yh + np.array([0.3, -0.2])
    clean = rbo.step(c['m0'], c['P0'], y, 0, 5, 4.0, c['GQG'], c['R'], c['tfd'], c['tfo'])
    out = rbo.step(c['m0'], c['P0'], y + 1e3, 0, 5, 4.0, c['GQG'], c['R'], c['tfd'], c['tfo'])
    plain = rbo.step(c['m0'], c['P0'], y + 1e3, 0, 1, 4.0, c['GQG'], c['R'], c['tfd'], c['tfo'])
    assert out[2] < 1e-3 * clean[2] and np.linalg.norm(out[0] - m_pr) < 1e-2 * np.linalg.norm(plain[0] - m_pr)


def test_study_gap_on_the_cpu():
    """Linear constant velocity, t_3 measurement noise, B = 256, T = 20, seed fixed: the time-averaged RMSE of the robust update
    (J = 5, dof = 3) against the plain filter (J = 1) with the same R, paired over the trajectories.  Measured with this seed: RMSE
    1.595 -> 1.358, the gap 9.7 standard errors; asserted at 3."""
    c, rng, B, T = _linear_cv(), np.random.default_rng(2012), 256, 20
    x, y = _simulate_cv(c, B, T, 3.0, rng)
    rmse = np.zeros((2, B))
    for b in range(B):
        for i, J in enumerate((1, 5)):
            fm = rbo.robust_filter(y[..., b], c['m0'], c['P0'], J, 3.0, c['GQG'], c['R'], c['tfd'], c['tfo'])[0]
            rmse[i, b] = np.sqrt(np.mean(np.sum((fm - x[..., b]) ** 2, axis=0)))
    d = rmse[0] - rmse[1]
    gap = float(np.mean(d) / (np.std(d, ddof=1) / np.sqrt(B)))
    print('study gap on the CPU: RMSE plain {:.3f}, robust {:.3f}, paired gap {:.2f} standard errors'.format(rmse[0].mean(), rmse[1].mean(), gap))
    assert rmse[1].mean() < rmse[0].mean() and gap >= 3.0, (rmse.mean(axis=1), gap)


def test_library_exports_and_declares_the_entry_points():
    from ssmtoybox_amd import _lib, ssinf
    header = open(os.path.join(ROOT, 'include', 'ssmq.h')).read()
    lib = ctypes.CDLL(_lib.library_path())
    for name in ('ssmq_filter_robust_dev', 'ssmq_robust_kernel_name'):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
        assert 'int ' + name + '(' in header
    assert _lib.RTC_ROBUST == 12 and 'SSMQ_RTC_ROBUST = 12' in header
    assert _lib.ROBUST_LAUNCH_LOOP == 1 and '#define SSMQ_ROBUST_LAUNCH_LOOP 1' in header
    for name in ('robust_pass', 'robust_pass_batch', 'robust_pass_dev', 'robust_kernel_name'):
        assert callable(getattr(ssinf.GaussianInference, name))


def test_user_pendulum_pair_compiles_for_gfx950_without_a_device():
    from ssmtoybox_amd import _lib, ssmod
    from ssmtoybox_amd.mtran import resolve_integrand
    UP, UM = pendulum_user()
    f_dyn, _ = resolve_integrand(UP(ssmod.GaussRV(2), ssmod.GaussRV(2)).dyn_eval)
    f_obs, _ = resolve_integrand(UM(ssmod.GaussRV(1), 2).meas_eval)
    for form, n in ((_lib.FORM_SIGMA, 5), (_lib.FORM_BQ, 5)):
        rc, log = _lib.rtc_compile_check(f_dyn.id, _lib.RTC_ROBUST, 2, 1, n, form, fid_obs=f_obs.id, N_obs=n, arch='gfx950')
        assert rc == 0, log
        assert 'k_robust_loop' in log and 'ScratchSize [bytes/lane]: 0' in log, log
    # the dense kernel is the only one: a fast-path request is a bad argument; a wrong shape is refused with a message
    rc, _ = _lib.rtc_compile_check(f_dyn.id, _lib.RTC_ROBUST, 2, 1, 5, _lib.FORM_SIGMA, opt=2, fid_obs=f_obs.id, N_obs=5)
    assert rc == -1
    rc, _ = _lib.rtc_compile_check(f_dyn.id, _lib.RTC_ROBUST, 7, 1, 15, _lib.FORM_SIGMA, fid_obs=f_obs.id, N_obs=15)
    assert rc == -3 and 'D <= 6' in _lib.last_error()


def test_refusals_come_before_the_library(monkeypatch):
    from ssmtoybox_amd import ssinf, ssmod as sm, _lib
    na = ssinf.UnscentedKalman(sm.UNGMNATransition(sm.GaussRV(1), sm.GaussRV(1)), sm.UNGMNAMeasurement(sm.GaussRV(1), 1))
    dyn_s = sm.UNGMTransition(sm.StudentRV(1, dof=4.0), sm.StudentRV(1, dof=4.0))
    stu = ssinf.FullySymmetricStudent(dyn_s, sm.UNGMMeasurement(sm.StudentRV(1, dof=4.0), 1))
    dyn = sm.UNGMTransition(sm.GaussRV(1), sm.GaussRV(1, cov=np.array([[10.0]])))
    mar = object.__new__(ssinf.MarginalizedGaussianProcessKalman)   # (the refusal needs none of its state)
    ok = ssinf.UnscentedKalman(dyn, sm.UNGMMeasurement(sm.GaussRV(1), 1))
    # a Gaussian filter takes a model whose measurement noise is a StudentRV: its scale and dof are the defaults of the robust pass
    heavy = ssinf.UnscentedKalman(dyn, sm.UNGMMeasurement(sm.StudentRV(1, scale=np.array([[2.0]]), dof=4.0), 1))
    assert np.array_equal(heavy.r_cov, [[2.0]])
    dof, J, R = heavy._robust_refusal(None, 5, None)
    assert (dof, J) == (4.0, 5) and np.array_equal(R, [[2.0]])
    dof, J, R = ok._robust_refusal(3, 2, None)
    assert (dof, J) == (3.0, 2) and np.array_equal(R, [[1.0]]) and ok._robust_refusal(1e300, 1, [[0.5]])[2][0, 0] == 0.5
    pair = ssinf.UnscentedKalman(sm.ConstantVelocity(sm.GaussRV(4), sm.GaussRV(2)), sm.Radar2DMeasurement(sm.GaussRV(2), 4))

    def no_library():
        raise AssertionError('the library was reached')
    monkeypatch.setattr(_lib, 'load', no_library)
    y = np.zeros((1, 4, 3))
    calls = (lambda a, **kw: a.robust_pass_batch(y, **kw), lambda a, **kw: a.robust_pass(y[..., 0], **kw),
             lambda a, **kw: a.robust_pass_dev(None, 3, 64, 4, **kw))
    for alg, what in ((na, 'non-additive'), (stu, 'Studentian'), (mar, 'marginalised')):
        for call in calls:
            with pytest.raises(NotImplementedError, match=what):
                call(alg, dof=4.0)
        with pytest.raises(NotImplementedError, match=what):
            alg.robust_kernel_name(2)
    for bad in (0, 65, -1, 2.5, True):
        for call in calls:
            with pytest.raises(ValueError, match='iterations'):
                call(ok, dof=4.0, iterations=bad)
        with pytest.raises(ValueError, match='iterations'):
            ok.robust_kernel_name(bad)
    for call in calls:
        with pytest.raises(ValueError, match='`dof` must be given'):
            call(ok)
        for bad in (0.0, -1.0, np.nan, np.inf):
            with pytest.raises(ValueError, match='dof must be a positive finite'):
                call(ok, dof=bad)
        for bad in ([[0.0]], [[-1.0]], [[np.nan]], np.eye(2)):
            with pytest.raises(ValueError, match='r_scale'):
                call(ok, dof=4.0, r_scale=bad)
    y2 = np.zeros((2, 4, 3))
    for bad in (np.array([[1.0, 2.0], [2.0, 1.0]]), np.array([[1.0, 0.5], [0.4, 1.0]])):     # indefinite; not symmetric
        with pytest.raises(ValueError, match='r_scale'):
            pair.robust_pass_batch(y2, dof=4.0, r_scale=bad)
