"""Innovation scores (NIS, measurement log-likelihood), the parts that need no device: the exported entry points, the run-time
compile of k_innovation<> for a user pendulum pair, the refusals that come before the library is touched, and the NumPy helper
(tests/_innovation_oracle.py) against the oracle's own Gaussian log-density."""
import ctypes
import os

import numpy as np
import pytest

from oracle import ssmq_oracle as orc
from tests import _innovation_oracle as ino

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def pendulum_user():
    from ssmtoybox_amd import ssmod

    class UserPendulum(ssmod.TransitionModel):
        dim_state, dim_noise, noise_additive = 2, 2, True
        # Fn<SSMQ_F_PENDULUM_DYN> restated (csrc/ssmq_device.h): the same expressions and helpers
        device_code = 'o[0] = x[0] + x[1] * p[0];  o[1] = x[1] - 9.81 * p[0] * sin_nr(x[0]);'

        def __init__(self, init_rv, noise_rv, dt=0.01):
            super().__init__(init_rv, noise_rv)
            self.dt = dt

        def _par(self):
            return (self.dt,)

    class UserPendulumMeas(ssmod.MeasurementModel):
        dim_out, dim_substate, dim_noise, noise_additive = 1, 1, 1, True
        device_code = 'o[0] = sin_nr(x[0]);'

    return UserPendulum, UserPendulumMeas


def test_library_exports_and_declares_the_entry_points():
    from ssmtoybox_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'ssmq.h')).read()
    lib = ctypes.CDLL(_lib.library_path())
    for name in ('ssmq_filter_innovations_dev', 'ssmq_innovations_kernel_name'):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
        assert 'int ' + name + '(' in header
    assert _lib.RTC_INNOVATION == 6 and 'SSMQ_RTC_INNOVATION = 6' in header
    from ssmtoybox_amd import ssinf
    for name in ('innovations', 'innovations_batch', 'innovations_dev', 'innovations_kernel_name'):
        assert callable(getattr(ssinf.GaussianInference, name))


def test_user_pendulum_pair_compiles_for_gfx950_without_a_device():
    from ssmtoybox_amd import _lib, ssmod
    from ssmtoybox_amd.mtran import resolve_integrand
    UP, UM = pendulum_user()
    f_dyn, _ = resolve_integrand(UP(ssmod.GaussRV(2), ssmod.GaussRV(2)).dyn_eval)
    f_obs, _ = resolve_integrand(UM(ssmod.GaussRV(1), 2).meas_eval)
    for form, n in ((_lib.FORM_SIGMA, 5), (_lib.FORM_BQ, 5), (_lib.FORM_SIGMA, 4)):
        rc, log = _lib.rtc_compile_check(f_dyn.id, _lib.RTC_INNOVATION, 2, 1, n, form, fid_obs=f_obs.id, N_obs=n, arch='gfx950')
        assert rc == 0, log
        assert 'k_innovation' in log and 'ScratchSize [bytes/lane]: 0' in log, log
    # a built-in member next to a user member, as the filter's kernel
    rc, log = _lib.rtc_compile_check(orc.F_PENDULUM_DYN, _lib.RTC_INNOVATION, 2, 1, 5, _lib.FORM_SIGMA, fid_obs=f_obs.id, N_obs=5)
    assert rc == 0, log
    # a wrong shape is refused with a message, nothing compiled
    rc, log = _lib.rtc_compile_check(f_dyn.id, _lib.RTC_INNOVATION, 7, 1, 15, _lib.FORM_SIGMA, fid_obs=f_obs.id, N_obs=15)
    assert rc == -3 and 'D <= 6' in _lib.last_error()


def test_refusals_come_before_the_library(monkeypatch):
    from ssmtoybox_amd import ssinf, ssmod as sm, _lib
    na = ssinf.UnscentedKalman(sm.UNGMNATransition(sm.GaussRV(1), sm.GaussRV(1)), sm.UNGMNAMeasurement(sm.GaussRV(1), 1))
    dyn_s = sm.UNGMTransition(sm.StudentRV(1, dof=4.0), sm.StudentRV(1, dof=4.0))
    stu = ssinf.FullySymmetricStudent(dyn_s, sm.UNGMMeasurement(sm.StudentRV(1, dof=4.0), 1))
    dyn = sm.UNGMTransition(sm.GaussRV(1), sm.GaussRV(1, cov=np.array([[10.0]])))
    obs = sm.UNGMMeasurement(sm.GaussRV(1), 1)
    # (its constructor computes GP weights on the device; the refusal needs none of its state)
    mar = object.__new__(ssinf.MarginalizedGaussianProcessKalman)
    ok = ssinf.UnscentedKalman(dyn, obs)

    def no_library():
        raise AssertionError('the library was reached')
    monkeypatch.setattr(_lib, 'load', no_library)
    y = np.zeros((1, 4, 3))
    for alg, what in ((na, 'non-additive'), (stu, 'Studentian'), (mar, 'marginalised')):
        for call in (lambda a: a.innovations_batch(y), lambda a: a.innovations(y[..., 0]), lambda a: a.innovations_kernel_name(),
                     lambda a: a.innovations_dev(None, None, None, 3, 64, 4)):
            with pytest.raises(NotImplementedError, match=what):
                call(alg)
    with pytest.raises(ValueError, match='fi_mean and fi_cov'):
        ok.innovations_batch(y, fi_mean=np.zeros((1, 4, 3)))


def test_helper_loglik_is_the_gaussian_log_density():
    rng = np.random.default_rng(5)
    for Y in (1, 2, 4):
        a = rng.standard_normal((Y, Y))
        S = a.dot(a.T) + 0.5 * np.eye(Y)
        y, ym = rng.standard_normal(Y), rng.standard_normal(Y)
        nis, ll = ino.score(y, ym, S)
        ref = float(orc.gauss_logpdf(y, ym, S))
        assert abs(ll - ref) <= 64 * np.linalg.cond(S) * np.finfo(float).eps * max(1.0, abs(ref))
        e = y - ym
        assert abs(nis - e.dot(np.linalg.solve(S, e))) <= 64 * np.linalg.cond(S) * np.finfo(float).eps * max(1.0, nis)
    # the recursion on a linear-Gaussian pair: the helper's moments are those of the Kalman prediction
    m0, P0, Q, R = np.zeros(4), np.eye(4), 0.01 * np.eye(4), 0.1 * np.eye(2)
    pts, (wm, wc) = orc.points_ut(4), orc.weights_ut(4)[:2]
    tfd = ino.sigma_tf(orc.F_CV_DYN, (0.1,), pts, wm, wc)
    lin = lambda m, P, t: (m[[0, 2]], P[np.ix_([0, 2], [0, 2])], None)       # noqa: E731
    y = rng.standard_normal((2, 3))
    fm, fP = rng.standard_normal((4, 3)), np.repeat(np.eye(4)[..., None], 3, axis=2)
    ym, S, nis, ll = ino.innovations(y, m0, P0, fm, fP, Q, R, tfd, lin)
    mp = orc.integrand(orc.F_CV_DYN, fm[:, 0], 1.0, (0.1,))
    assert np.allclose(ym[:, 1], mp[[0, 2]], rtol=0, atol=1e-12)
    for k in range(3):
        assert abs(ll[k] - float(orc.gauss_logpdf(y[:, k], ym[:, k], S[..., k]))) <= 1e-12 * max(1.0, abs(ll[k]))
    # failure rule: NaN inputs and a covariance that is not positive definite give NaN rows
    fm[:, 0] = np.nan
    out = ino.innovations(y, m0, -np.eye(4), fm, fP, Q, R, tfd, lin)
    assert np.isnan(out[2][0]) and np.isnan(out[2][1]) and np.isfinite(out[2][2]) and np.isnan(out[0][:, 0]).all()
