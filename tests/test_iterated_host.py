"""Iterated posterior linearisation pass (IPLF), the parts that need no device: the NumPy restatement (tests/_iterated_oracle.py) at one
iteration against the oracle's own Gaussian filter, the exported entry points, the run-time compile of k_iplf_loop<> for a user
pendulum pair, and the refusals that come before the library is touched."""
import ctypes
import os

import numpy as np
import pytest

from oracle import ssmq_oracle as orc
from tests import _innovation_oracle as ino
from tests import _iterated_oracle as ito
from tests.test_innovation_host import pendulum_user

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ungm():
    pts, (wm, wc) = orc.points_ut(1), orc.weights_ut(1)[:2]
    tfd, tfo = ino.sigma_tf(orc.F_UNGM_DYN, (), pts, wm, wc), ino.sigma_tf(orc.F_UNGM_MEAS, (), pts, wm, wc)
    return dict(m0=np.zeros(1), P0=np.eye(1), Q=10.0 * np.eye(1), R=np.eye(1), tfd=tfd, tfo=tfo, fd=orc.F_UNGM_DYN, fo=orc.F_UNGM_MEAS,
                pd=(), so=None)


def _pendulum():
    pts, (wm, wc) = orc.points_ut(2), orc.weights_ut(2)[:2]
    tfd, tfo = ino.sigma_tf(orc.F_PENDULUM_DYN, (0.01,), pts, wm, wc), ino.sigma_tf(orc.F_PENDULUM_MEAS, (), pts, wm, wc, (0,))
    Q = 0.01 * np.array([[0.01 ** 3 / 3, 0.01 ** 2 / 2], [0.01 ** 2 / 2, 0.01]])
    return dict(m0=np.array([1.5, 0.0]), P0=0.01 * np.eye(2), Q=Q, R=0.1 * np.eye(1), tfd=tfd, tfo=tfo, fd=orc.F_PENDULUM_DYN,
                fo=orc.F_PENDULUM_MEAS, pd=(0.01,), so=[0])


def _measurements(c, T, rng):
    x = c['m0'] + np.linalg.cholesky(c['P0']).dot(rng.standard_normal(c['m0'].shape[0]))
    Lq, Lr = np.linalg.cholesky(c['Q']), np.linalg.cholesky(c['R'])
    y = np.zeros((c['R'].shape[0], T))
    for k in range(T):
        x = orc.integrand(c['fd'], x, float(k), c['pd']) + Lq.dot(rng.standard_normal(Lq.shape[0]))
        y[:, k] = orc.integrand(c['fo'], x if c['so'] is None else x[c['so']], float(k), ()) + Lr.dot(rng.standard_normal(Lr.shape[0]))
    return y


@pytest.mark.parametrize('case', [_ungm, _pendulum])
def test_one_iteration_is_the_gaussian_filter(case):
    """J = 1 against orc.gaussian_filter, every step from the filter's own moments of the step before: 1e-12 relative to
    max(1, |value|) (measured: 1.2e-14 at most)."""
    c, rng, T = case(), np.random.default_rng(11), 20
    D = c['m0'].shape[0]
    worst = 0.0
    for _ in range(8):
        y = _measurements(c, T, rng)
        fm, fP = orc.gaussian_filter(y, c['m0'], c['P0'], c['Q'], c['R'], np.eye(D), c['tfd'], c['tfo'])[:2]
        for k in range(T):
            m, P = (c['m0'], c['P0']) if k == 0 else (fm[:, k - 1], fP[..., k - 1])
            mj, Pj, delta, conds = ito.step(m, P, y[:, k], k, 1, c['Q'], c['R'], c['tfd'], c['tfo'])
            assert conds is not None and len(conds) == 2 and np.isfinite(delta)
            worst = max(worst, float(np.max(np.abs(mj - fm[:, k]) / np.maximum(1.0, np.abs(fm[:, k])))),
                        float(np.max(np.abs(Pj - ino.lower_sym(fP[..., k])) / np.maximum(1.0, np.abs(fP[..., k])))))
        # the recursion form is the chain of one-step forms
        rm, rP, rd = ito.iterated_filter(y, c['m0'], c['P0'], 1, c['Q'], c['R'], c['tfd'], c['tfo'])
        assert np.max(np.abs(rm - fm) / np.maximum(1.0, np.abs(fm))) <= 1e-9 and np.all(np.isfinite(rd))
    print('oracle at J = 1 against orc.gaussian_filter: {:.3g}'.format(worst))
    assert worst <= 1e-12, worst


def test_iterating_moves_the_mean_and_long_double_agrees():
    """J = 5 differs from J = 1 where the measurement is informative (UNGM), and the long-double restatement of a step agrees with
    the float64 one to rounding; a covariance that is not positive definite gives NaN rows from that step on."""
    c, rng = _ungm(), np.random.default_rng(12)
    y = _measurements(c, 20, rng)
    a = ito.iterated_filter(y, c['m0'], c['P0'], 1, c['Q'], c['R'], c['tfd'], c['tfo'])
    b = ito.iterated_filter(y, c['m0'], c['P0'], 5, c['Q'], c['R'], c['tfd'], c['tfo'])
    assert np.all(np.isfinite(b[0])) and np.max(np.abs(a[0] - b[0])) > 1e-3
    pts, (wm, wc) = orc.points_ut(1), orc.weights_ut(1)[:2]
    tfd, tfo = ino.sigma_tf_ld(orc.F_UNGM_DYN, (), pts, wm, wc), ino.sigma_tf_ld(orc.F_UNGM_MEAS, (), pts, wm, wc)
    m64, P64, d64, _ = ito.step(c['m0'], c['P0'], y[:, 0], 0, 3, c['Q'], c['R'], c['tfd'], c['tfo'])
    mld, Pld, dld = ito.step_ld(c['m0'], c['P0'], y[:, 0], 0, 3, c['Q'], c['R'], tfd, tfo)
    assert abs(float(mld[0]) - m64[0]) <= 1e-12 * max(1.0, abs(m64[0])) and abs(float(Pld[0, 0]) - P64[0, 0]) <= 1e-12 * max(1.0, P64[0, 0])
    assert abs(float(dld) - d64) <= 1e-10 * max(1.0, d64)
    fm, fP, delta = ito.iterated_filter(y, c['m0'], -np.eye(1), 2, c['Q'], c['R'], c['tfd'], c['tfo'])
    assert np.isnan(fm).all() and np.isnan(fP).all() and np.isnan(delta).all()


def test_library_exports_and_declares_the_entry_points():
    from ssmtoybox_amd import _lib, ssinf
    header = open(os.path.join(ROOT, 'include', 'ssmq.h')).read()
    lib = ctypes.CDLL(_lib.library_path())
    for name in ('ssmq_filter_iterated_dev', 'ssmq_iterated_kernel_name'):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
        assert 'int ' + name + '(' in header
    assert _lib.RTC_ITERATED == 7 and 'SSMQ_RTC_ITERATED = 7' in header
    assert _lib.ITERATED_MAX == 64 and '#define SSMQ_ITERATED_MAX 64' in header
    assert _lib.ABI_VERSION == 102 and '#define SSMQ_VERSION 102' in header
    lib.ssmq_version.restype = ctypes.c_int
    assert lib.ssmq_version() == 102
    for name in ('iterated_pass', 'iterated_pass_batch', 'iterated_pass_dev', 'iterated_kernel_name'):
        assert callable(getattr(ssinf.GaussianInference, name))


def test_user_pendulum_pair_compiles_for_gfx950_without_a_device():
    from ssmtoybox_amd import _lib, ssmod
    from ssmtoybox_amd.mtran import resolve_integrand
    UP, UM = pendulum_user()
    f_dyn, _ = resolve_integrand(UP(ssmod.GaussRV(2), ssmod.GaussRV(2)).dyn_eval)
    f_obs, _ = resolve_integrand(UM(ssmod.GaussRV(1), 2).meas_eval)
    for form, n in ((_lib.FORM_SIGMA, 5), (_lib.FORM_BQ, 5)):
        rc, log = _lib.rtc_compile_check(f_dyn.id, _lib.RTC_ITERATED, 2, 1, n, form, fid_obs=f_obs.id, N_obs=n, arch='gfx950')
        assert rc == 0, log
        assert 'k_iplf_loop' in log and 'ScratchSize [bytes/lane]: 0' in log, log
    # the dense kernel is the only one: a fast-path request is a bad argument; a wrong shape is refused with a message
    rc, _ = _lib.rtc_compile_check(f_dyn.id, _lib.RTC_ITERATED, 2, 1, 5, _lib.FORM_SIGMA, opt=2, fid_obs=f_obs.id, N_obs=5)
    assert rc == -1
    rc, _ = _lib.rtc_compile_check(f_dyn.id, _lib.RTC_ITERATED, 7, 1, 15, _lib.FORM_SIGMA, fid_obs=f_obs.id, N_obs=15)
    assert rc == -3 and 'D <= 6' in _lib.last_error()


def test_refusals_come_before_the_library(monkeypatch):
    from ssmtoybox_amd import ssinf, ssmod as sm, _lib
    na = ssinf.UnscentedKalman(sm.UNGMNATransition(sm.GaussRV(1), sm.GaussRV(1)), sm.UNGMNAMeasurement(sm.GaussRV(1), 1))
    dyn_s = sm.UNGMTransition(sm.StudentRV(1, dof=4.0), sm.StudentRV(1, dof=4.0))
    stu = ssinf.FullySymmetricStudent(dyn_s, sm.UNGMMeasurement(sm.StudentRV(1, dof=4.0), 1))
    dyn = sm.UNGMTransition(sm.GaussRV(1), sm.GaussRV(1, cov=np.array([[10.0]])))
    obs = sm.UNGMMeasurement(sm.GaussRV(1), 1)
    mar = object.__new__(ssinf.MarginalizedGaussianProcessKalman)   # (the refusal needs none of its state)
    ok = ssinf.UnscentedKalman(dyn, obs)

    def no_library():
        raise AssertionError('the library was reached')
    monkeypatch.setattr(_lib, 'load', no_library)
    y = np.zeros((1, 4, 3))
    calls = (lambda a, j: a.iterated_pass_batch(y, j), lambda a, j: a.iterated_pass(y[..., 0], j), lambda a, j: a.iterated_kernel_name(j),
             lambda a, j: a.iterated_pass_dev(None, 3, 64, 4, j))
    for alg, what in ((na, 'non-additive'), (stu, 'Studentian'), (mar, 'marginalised')):
        for call in calls:
            with pytest.raises(NotImplementedError, match=what):
                call(alg, 2)
    for bad in (0, 65, -1, 2.5, True):
        for call in calls:
            with pytest.raises(ValueError, match='iterations'):
                call(ok, bad)
