"""Iterated posterior linearisation smoother (IPLS), the parts that need no device: the exported entry points, the run-time compile of
k_ipls_pass<> for a user pendulum pair, the NumPy restatement (tests/_ipls_oracle.py) against the oracle's Gaussian filter, a textbook
RTS pass, a linear-Gaussian system and its own long-double form, and the refusals that come before the library is touched."""
import ctypes
import os

import numpy as np
import pytest

from oracle import ssmq_oracle as orc
from tests import _innovation_oracle as ino
from tests import _ipls_oracle as ipo
from tests.test_innovation_host import pendulum_user
from tests.test_iterated_host import _measurements, _pendulum, _ungm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_and_declares_the_entry_points():
    from ssmtoybox_amd import _lib, ssinf
    header = open(os.path.join(ROOT, 'include', 'ssmq.h')).read()
    lib = ctypes.CDLL(_lib.library_path())
    for name in ('ssmq_smoother_iterated_dev', 'ssmq_smoother_iterated_kernel_name'):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
        assert 'int ' + name + '(' in header
    assert _lib.RTC_SMOOTHER_ITERATED == 8 and 'SSMQ_RTC_SMOOTHER_ITERATED = 8' in header
    assert 'SSMQ_RTC_INNOVATION = 6, SSMQ_RTC_ITERATED = 7' in header       # appended: the earlier kinds keep their numbers
    assert _lib.ABI_VERSION == 102 and '#define SSMQ_VERSION 102' in header
    for name in ('iterated_smoother', 'iterated_smoother_batch', 'iterated_smoother_dev', 'iterated_smoother_kernel_name'):
        assert callable(getattr(ssinf.GaussianInference, name))


def test_user_pendulum_pair_compiles_for_gfx950_without_a_device():
    from ssmtoybox_amd import _lib, ssmod
    from ssmtoybox_amd.mtran import resolve_integrand
    UP, UM = pendulum_user()
    f_dyn, _ = resolve_integrand(UP(ssmod.GaussRV(2), ssmod.GaussRV(2)).dyn_eval)
    f_obs, _ = resolve_integrand(UM(ssmod.GaussRV(1), 2).meas_eval)
    for form, n in ((_lib.FORM_SIGMA, 5), (_lib.FORM_BQ, 5)):
        rc, log = _lib.rtc_compile_check(f_dyn.id, _lib.RTC_SMOOTHER_ITERATED, 2, 1, n, form, fid_obs=f_obs.id, N_obs=n, arch='gfx950')
        assert rc == 0, log
        assert 'k_ipls_pass' in log and 'ScratchSize [bytes/lane]: 0' in log, log
    # the dense transforms are the only ones: a fast-path request is a bad argument; a wrong shape is refused with a message
    rc, _ = _lib.rtc_compile_check(f_dyn.id, _lib.RTC_SMOOTHER_ITERATED, 2, 1, 5, _lib.FORM_SIGMA, opt=2, fid_obs=f_obs.id, N_obs=5)
    assert rc == -1
    rc, _ = _lib.rtc_compile_check(f_dyn.id, _lib.RTC_SMOOTHER_ITERATED, 7, 1, 15, _lib.FORM_SIGMA, fid_obs=f_obs.id, N_obs=15)
    assert rc == -3 and 'D <= 6' in _lib.last_error()


@pytest.mark.parametrize('case', [_ungm, _pendulum])
def test_one_iteration_is_the_gaussian_filter_and_a_textbook_rts_pass(case):
    """iterations = 1: the filtered moments against orc.gaussian_filter and the smoothed ones against an RTS pass written out here
    (np.linalg.solve on the oracle's predictive moments, down to the initial state): 1e-11 relative to max(1, |value|)."""
    c, rng, T = case(), np.random.default_rng(21), 20
    D = c['m0'].shape[0]
    worst = 0.0

    def rel(a, b):
        return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b))))
    for _ in range(6):
        y = _measurements(c, T, rng)
        fm, fP, pm, pP, pC = orc.gaussian_filter(y, c['m0'], c['P0'], c['Q'], c['R'], np.eye(D), c['tfd'], c['tfo'])
        r = ipo.ipls(y, c['m0'], c['P0'], 1, c['Q'], c['R'], c['tfd'], c['tfo'])
        assert r['status'] == 0 and np.isfinite(r['delta'])
        worst = max(worst, rel(r['fm'], fm), rel(r['fP'], fP), rel(r['pm'], pm), rel(r['pP'], pP))
        ms, Ps = fm[:, T - 1], fP[..., T - 1]
        assert np.array_equal(r['sm'][:, T], r['fm'][:, T - 1]) and np.array_equal(r['sP'][..., T], r['fP'][..., T - 1])
        for k in range(T - 1, -1, -1):
            mf, Pf = (c['m0'], c['P0']) if k == 0 else (fm[:, k - 1], fP[..., k - 1])
            G = np.linalg.solve(pP[..., k], pC[..., k]).T          # cov(x_{k-1}, x_k) (P-_k)^-1
            ms, Ps = mf + G.dot(ms - pm[:, k]), Pf + G.dot(Ps - pP[..., k]).dot(G.T)
            worst = max(worst, rel(r['sm'][:, k], ms), rel(r['sP'][..., k], Ps))
    print('restatement at one iteration against orc.gaussian_filter + RTS: {:.3g}'.format(worst))
    assert worst <= 1e-11, worst


def _linear_gaussian():
    dt = 0.1
    A = np.array([[1, dt, 0, 0], [0, 1, 0, 0], [0, 0, 1, dt], [0, 0, 0, 1]], dtype=float)
    H = np.array([[1.0, 0, 0, 0], [0, 0, 1.0, 0]])
    Gm = np.array([[dt ** 2 / 2, 0], [dt, 0], [0, dt ** 2 / 2], [0, dt]])
    return A, H, Gm.dot(0.1 * np.eye(2)).dot(Gm.T) + 1e-6 * np.eye(4), np.diag([0.5, 0.3])


def test_linear_gaussian_second_iteration_changes_nothing():
    """Exact linear transforms (mean A m, covariance A P A', cross-covariance A P): statistical linear regression returns A and H
    whatever the linearisation point, so iteration 2 is iteration 1 up to rounding and delta is rounding."""
    A, H, Q, R = _linear_gaussian()
    tfd = lambda m, P, t: (A.dot(m), A.dot(P).dot(A.T), A.dot(P))       # noqa: E731
    tfo = lambda m, P, t: (H.dot(m), H.dot(P).dot(H.T), H.dot(P))       # noqa: E731
    rng = np.random.default_rng(5)
    m0, P0, T = np.array([100.0, 5.0, 200.0, -3.0]), np.diag([1.0, 0.1, 1.0, 0.1]), 12
    x, y = m0 + np.linalg.cholesky(P0).dot(rng.standard_normal(4)), np.zeros((2, T))
    for k in range(T):
        x = A.dot(x) + np.linalg.cholesky(Q).dot(rng.standard_normal(4))
        y[:, k] = H.dot(x) + np.linalg.cholesky(R).dot(rng.standard_normal(2))
    one = ipo.ipls(y, m0, P0, 1, Q, R, tfd, tfo)
    two = ipo.ipls(y, m0, P0, 2, Q, R, tfd, tfo)
    assert one['status'] == 0 and two['status'] == 0
    for key in ('fm', 'fP', 'sm', 'sP'):
        assert np.max(np.abs(one[key] - two[key]) / np.maximum(1.0, np.abs(one[key]))) <= 1e-10, key
    assert two['delta'] <= 1e-9
    # smoothing helps: no smoothed variance above the filtered one, and the initial state is smoothed too
    assert np.all(np.diagonal(two['sP'][..., 1:]) <= np.diagonal(two['fP']) * (1 + 1e-9))
    assert np.all(np.diag(two['sP'][..., 0]) < np.diag(P0))


def test_the_long_double_form_agrees_and_failures_are_statuses():
    c, rng = _pendulum(), np.random.default_rng(22)
    y = _measurements(c, 8, rng)
    pts, (wm, wc) = orc.points_ut(2), orc.weights_ut(2)[:2]
    tfd_ld = ino.sigma_tf_ld(orc.F_PENDULUM_DYN, (0.01,), pts, wm, wc)
    tfo_ld = ino.sigma_tf_ld(orc.F_PENDULUM_MEAS, (), pts, wm, wc, (0,))
    first = ipo.ipls(y, c['m0'], c['P0'], 1, c['Q'], c['R'], c['tfd'], c['tfo'])
    second = ipo.ipls(y, c['m0'], c['P0'], 2, c['Q'], c['R'], c['tfd'], c['tfo'])
    assert second['status'] == 0 and np.max(np.abs(second['sm'] - first['sm'])) > 1e-6       # iterating does something here
    k = 3
    for lp, lc in ((None, None), ((first['sm'][:, k], first['sP'][..., k]), (first['sm'][:, k + 1], first['sP'][..., k + 1]))):
        m, P = first['fm'][:, k - 1], first['fP'][..., k - 1]
        f64 = ipo.forward_step(m, P, lp, lc, y[:, k], k, c['Q'], c['R'], c['tfd'], c['tfo'])
        fld = ipo.forward_step_ld(m, P, lp, lc, y[:, k], k, c['Q'], c['R'], tfd_ld, tfo_ld)
        assert f64[5] is not None and len(f64[5]) == 3
        for a, b in zip(f64[:5], fld):
            assert np.max(np.abs(a - np.asarray(b, dtype=float)) / np.maximum(1.0, np.abs(a))) <= 1e-11
        b64 = ipo.backward_step(m, P, f64[0], f64[1], f64[2], first['sm'][:, k + 1], first['sP'][..., k + 1])
        bld = ipo.backward_step_ld(m, P, f64[0], f64[1], f64[2], first['sm'][:, k + 1], first['sP'][..., k + 1])
        for a, b in zip(b64[:2], bld):
            assert np.max(np.abs(a - np.asarray(b, dtype=float)) / np.maximum(1.0, np.abs(a))) <= 1e-9 * max(1.0, b64[2] * 1e-6)
    # an indefinite initial covariance fails step 0, a NaN measurement the step it belongs to; every moment is NaN then
    bad = ipo.ipls(y, c['m0'], -np.eye(2), 2, c['Q'], c['R'], c['tfd'], c['tfo'])
    assert bad['status'] == 1 and np.isnan(bad['sm']).all() and np.isnan(bad['fP']).all() and np.isnan(bad['delta'])
    yn = y.copy()
    yn[:, 3] = np.nan
    assert ipo.ipls(yn, c['m0'], c['P0'], 3, c['Q'], c['R'], c['tfd'], c['tfo'])['status'] == 4


def test_refusals_come_before_the_library(monkeypatch):
    from ssmtoybox_amd import ssinf, ssmod as sm, _lib
    na = ssinf.UnscentedKalman(sm.UNGMNATransition(sm.GaussRV(1), sm.GaussRV(1)), sm.UNGMNAMeasurement(sm.GaussRV(1), 1))
    dyn_s = sm.UNGMTransition(sm.StudentRV(1, dof=4.0), sm.StudentRV(1, dof=4.0))
    stu = ssinf.FullySymmetricStudent(dyn_s, sm.UNGMMeasurement(sm.StudentRV(1, dof=4.0), 1))
    dyn = sm.UNGMTransition(sm.GaussRV(1), sm.GaussRV(1, cov=np.array([[10.0]])))
    obs = sm.UNGMMeasurement(sm.GaussRV(1), 1)
    mar = object.__new__(ssinf.MarginalizedGaussianProcessKalman)   # (the refusal needs none of its state)
    ok, ekf, gh = ssinf.UnscentedKalman(dyn, obs), ssinf.ExtendedKalman(dyn, obs), ssinf.GaussHermiteKalman(dyn, obs, deg=3)
    tru = ssinf.TruncatedUnscentedKalman(dyn, obs)

    def no_library():
        raise AssertionError('the library was reached')
    monkeypatch.setattr(_lib, 'load', no_library)
    y = np.zeros((1, 4, 3))
    calls = (lambda a, j: a.iterated_smoother_batch(y, j), lambda a, j: a.iterated_smoother(y[..., 0], j),
             lambda a, j: a.iterated_smoother_kernel_name(j), lambda a, j: a.iterated_smoother_dev(None, 3, 64, 4, j))
    for alg, what in ((na, 'non-additive'), (stu, 'Studentian'), (mar, 'marginalised'), (ekf, 'linearisation'), (gh, 'Gauss-Hermite'),
                      (tru, 'truncated')):
        for call in calls:
            with pytest.raises(NotImplementedError, match=what):
                call(alg, 2)
    for bad in (0, 65, -1, 2.5, True):
        for call in calls:
            with pytest.raises(ValueError, match='iterations'):
                call(ok, bad)
    with pytest.raises(ValueError, match='lin_mean'):
        ok.iterated_smoother_batch(y, 2, lin_mean=np.zeros((1, 5, 3)))
