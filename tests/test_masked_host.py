"""Masked pass, the parts that need no device: the NumPy restatement (tests/_masked_oracle.py) on a linear model against a textbook
Kalman filter over the rows H[o] and against sequential scalar updates; the decoupling identity the device kernels rest on, for all 16
masks at Y = 4; the gate cases the GPU tests use; the refusals that come before the library is touched; the exported entry points and
their prototypes; the restated detection-mask generator."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import _masked_oracle as mko
from tests.test_innovation_gpu import oracle_tf
from tests.test_robust_host import _linear_cv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _linear_y4():
    """Constant velocity with four linear measurements (both positions, their sum and difference), R diagonal."""
    c = _linear_cv()
    H = np.array([[1, 0, 0, 0], [0, 0, 1, 0], [1, 0, 1, 0], [1, 0, -1, 0]], dtype=float)
    c['H'], c['R'] = H, np.diag([1.0, 0.5, 2.0, 0.25])
    c['tfo'] = lambda m, P, t: (H.dot(m), H.dot(P).dot(H.T), H.dot(P))
    return c


def _measure(c, T, rng):
    x = c['m0'] + np.linalg.cholesky(c['P0']).dot(rng.standard_normal(4))
    y = np.zeros((c['H'].shape[0], T))
    for k in range(T):
        x = c['F'].dot(x) + np.linalg.cholesky(c['GQG'] + 1e-12 * np.eye(4)).dot(rng.standard_normal(4))
        y[:, k] = c['H'].dot(x) + np.sqrt(np.diag(c['R'])) * rng.standard_normal(y.shape[0])
    return y


def test_linear_model_is_the_textbook_kalman_filter_over_the_observed_rows():
    c, rng, T = _linear_y4(), np.random.default_rng(11), 16
    y = _measure(c, T, rng)
    mask = np.arange(T, dtype=np.uint32) % 16                     # every pattern once, o = 0 at k = 0
    fm, fP, used, nis, ll = mko.masked_filter(y, mask, c['m0'], c['P0'], c['GQG'], c['R'], c['tfd'], c['tfo'])
    m, P = c['m0'], c['P0']
    for k in range(T):
        o = mko.bits(mask[k], 4)
        m, P = c['F'].dot(m), c['F'].dot(P).dot(c['F'].T) + c['GQG']
        if o.any():
            H, R = c['H'][o], c['R'][np.ix_(o, o)]
            S = H.dot(P).dot(H.T) + R
            K = P.dot(H.T).dot(np.linalg.inv(S))
            e = y[o, k] - H.dot(m)
            d2 = float(e.dot(np.linalg.solve(S, e)))
            assert np.isclose(nis[k], d2, rtol=1e-10) and np.isclose(ll[k], -0.5 * (o.sum() * np.log(2 * np.pi) + np.linalg.slogdet(S)[1] + d2), rtol=1e-10)
            m, P = m + K.dot(e), P - K.dot(S).dot(K.T)
        else:
            assert nis[k] == 0.0 and ll[k] == 0.0
        assert used[k] == mask[k]
        assert np.allclose(fm[:, k], m, rtol=1e-10, atol=1e-11) and np.allclose(fP[..., k], P, rtol=1e-10, atol=1e-11)


def test_diagonal_noise_is_sequential_scalar_updates():
    c, rng, T = _linear_y4(), np.random.default_rng(12), 16
    y = _measure(c, T, rng)
    mask = (5 * np.arange(T, dtype=np.uint32) + 3) % 16
    fm, fP, _, nis, _ = mko.masked_filter(y, mask, c['m0'], c['P0'], c['GQG'], c['R'], c['tfd'], c['tfo'])
    m, P = c['m0'], c['P0']
    for k in range(T):
        m, P = c['F'].dot(m), c['F'].dot(P).dot(c['F'].T) + c['GQG']
        d2 = 0.0
        for i in np.flatnonzero(mko.bits(mask[k], 4)):
            h = c['H'][i]
            s = float(h.dot(P).dot(h)) + c['R'][i, i]
            e = y[i, k] - h.dot(m)
            d2 += e * e / s                                     # (the innovations of sequential updates are independent)
            K = P.dot(h) / s
            m, P = m + K * e, P - np.outer(K, K) * s
        assert np.isclose(nis[k], d2, rtol=1e-9, atol=1e-12)
        assert np.allclose(fm[:, k], m, rtol=1e-10, atol=1e-11) and np.allclose(fP[..., k], P, rtol=1e-10, atol=1e-11)


def test_decoupling_in_place_is_the_compressed_update_for_all_16_masks():
    """The decoupled Y x Y system gives the moments, d2 and log det of the compressed one; the values under cleared bits (NaN, Inf,
    1e300) are not operands."""
    c, rng = _linear_y4(), np.random.default_rng(13)
    A = rng.standard_normal((4, 4))
    R = A.dot(A.T) + 0.5 * np.eye(4)                             # (a full R: the observed block is coupled)
    m_pr, P_pr, _ = c['tfd'](c['m0'], c['P0'], 0)
    P_pr = P_pr + c['GQG']
    yh, Ph, C = c['tfo'](m_pr, P_pr, 0)
    y = yh + rng.standard_normal(4)
    for w in range(16):
        obs = mko.bits(w, 4)
        mc, Pc, _, d2, ll, _, _ = mko.update(m_pr, P_pr, yh, Ph, C, R, y, obs)
        for fill in (0.0, np.nan, np.inf, 1e300):
            md, Pd, d2d, ldet = mko.decoupled(m_pr, P_pr, yh, Ph, C, R, np.where(obs, y, fill), obs)
            assert np.allclose(md, mc, rtol=1e-12, atol=1e-13) and np.allclose(Pd, Pc, rtol=1e-12, atol=1e-13), w
            assert np.isclose(d2d, d2, rtol=1e-12, atol=1e-300), w
            o = int(obs.sum())
            assert np.isclose(-0.5 * (o * np.log(2 * np.pi) + ldet + d2d), ll, rtol=1e-12, atol=1e-300), w
        if w == 0:
            assert np.array_equal(mc, m_pr) and np.array_equal(Pc, P_pr) and d2 == 0.0 and ll == 0.0


@pytest.mark.parametrize('name', mko.GATE_CASES)
def test_gate_cases_accept_and_reject_and_sit_off_the_threshold(name):
    alg, y, mask, gate = mko.gate_case(name)
    tfd, tfo = oracle_tf(alg.tf_dyn, alg.mod_dyn.dyn_eval), oracle_tf(alg.tf_obs, alg.mod_obs.meas_eval)
    GQG = alg.G.dot(alg.q_cov).dot(alg.G.T)
    Y = y.shape[0]
    offered = accepted = rejected = near = 0
    for b in range(mko.GATE_B):
        _, _, used, nis, _ = mko.masked_filter(y[..., b], mask[:, b], alg.x0_mean, alg.x0_cov, GQG, alg.r_cov, tfd, tfo, gate)
        assert np.all(np.isfinite(nis))
        for k in range(mko.GATE_T):
            o = int(mko.bits(mask[k, b], Y).sum())
            if o == 0:
                assert used[k] == 0
                continue
            offered += 1
            near += abs(nis[k] - gate[o]) < 1e-9 * gate[o]
            accepted += used[k] != 0
            rejected += used[k] == 0
            assert (used[k] == 0) == (nis[k] > gate[o])
    print('gate case {}: {} offered, {} accepted, {} rejected, {} near the threshold'.format(name, offered, accepted, rejected, near))
    assert accepted > 0 and rejected >= mko.GATE_B // 5 and near == 0
    assert near / offered == 0.0                                  # the share of steps skipped for being near the threshold


def test_refusals_come_before_the_library(monkeypatch):
    from ssmtoybox_amd import ssinf, ssmod as sm, _lib
    na = ssinf.UnscentedKalman(sm.UNGMNATransition(sm.GaussRV(1), sm.GaussRV(1)), sm.UNGMNAMeasurement(sm.GaussRV(1), 1))
    dyn_s = sm.UNGMTransition(sm.StudentRV(1, dof=4.0), sm.StudentRV(1, dof=4.0))
    stu = ssinf.FullySymmetricStudent(dyn_s, sm.UNGMMeasurement(sm.StudentRV(1, dof=4.0), 1))
    mar = object.__new__(ssinf.MarginalizedGaussianProcessKalman)   # (the refusal needs none of its state)
    dyn = sm.UNGMTransition(sm.GaussRV(1), sm.GaussRV(1, cov=np.array([[10.0]])))
    ok = ssinf.UnscentedKalman(dyn, sm.UNGMMeasurement(sm.GaussRV(1), 1))
    pair = ssinf.UnscentedKalman(sm.ConstantVelocity(sm.GaussRV(4), sm.GaussRV(2)), sm.Radar2DMeasurement(sm.GaussRV(2), 4))
    assert ok._masked_refusal(None) is None
    assert np.array_equal(ok._masked_refusal(3.0), [np.inf, 3.0]) and np.array_equal(pair._masked_refusal(np.inf), [np.inf] * 3)
    assert np.array_equal(pair._masked_refusal([4.0, 9.0]), [np.inf, 4.0, 9.0])
    assert np.array_equal(pair._mask_words(np.ones((2, 4, 3), dtype=bool), 2, 4, 3), np.full((4, 3), 3))
    assert np.array_equal(pair._mask_words(np.full((4, 3), 7, dtype=np.uint8), 2, 4, 3), np.full((4, 3), 3))   # (bits at or above Y dropped)

    def no_library():
        raise AssertionError('the library was reached')
    monkeypatch.setattr(_lib, 'load', no_library)
    y = np.zeros((1, 4, 3))
    calls = (lambda a, **kw: a.masked_pass_batch(y, **kw), lambda a, **kw: a.masked_pass(y[..., 0], **kw),
             lambda a, **kw: a.masked_pass_dev(None, 3, 64, 4, **kw))
    for alg, what in ((na, 'non-additive'), (stu, 'Studentian'), (mar, 'marginalised')):
        for call in calls:
            with pytest.raises(NotImplementedError, match=what):
                call(alg)
        with pytest.raises(NotImplementedError, match=what):
            alg.masked_kernel_name()
    for bad in (0.0, -1.0, np.nan, [1.0, 2.0], [[1.0]]):
        for call in calls:
            with pytest.raises(ValueError, match='gate'):
                call(ok, gate=bad)
    y2 = np.zeros((2, 4, 3))
    for bad in ([1.0], [1.0, 0.0], [1.0, np.nan], [1.0, 2.0, 3.0]):
        with pytest.raises(ValueError, match='gate'):
            pair.masked_pass_batch(y2, gate=bad)
    for bad in (np.ones((4, 3), dtype=bool), np.ones((2, 4, 4), dtype=bool), np.ones((2, 4, 3)), np.ones((4, 3), dtype=np.int32),
                np.ones((3, 4), dtype=np.uint32)):
        with pytest.raises(ValueError, match='mask'):
            pair.masked_pass_batch(y2, mask=bad)
    with pytest.raises(ValueError, match='mask'):
        ok.masked_pass(y[..., 0], mask=np.ones((2, 4), dtype=bool))
    with pytest.raises(ValueError, match='p_detect'):
        sm.detection_mask_dev(3, 64, 4, 2, [0.5, 1.5])
    if hasattr(ssinf, 'gate_thresholds'):
        from scipy.stats import chi2
        g = ssinf.gate_thresholds(4, 0.99)
        assert g.shape == (4,) and np.allclose(g, [chi2.ppf(0.99, o) for o in (1, 2, 3, 4)]) and np.all(np.diff(g) > 0)
        with pytest.raises(ValueError, match='prob'):
            ssinf.gate_thresholds(4, 0.0)


_C2CT = {'ssmq_transform *': 'c_void_p', 'const ssmq_transform *': 'c_void_p', 'const ssmq_integrand *': 'LP_Integrand', 'int64_t': 'c_long',
         'int': 'c_int', 'uint64_t': 'c_ulong', 'const double *': 'LP_c_double', 'double *': 'c_void_p', 'const uint32_t *': 'c_void_p',
         'uint32_t *': 'c_void_p', 'int32_t *': 'c_void_p', 'char *': 'c_char_p'}


def _declared(header, name):
    """The parameter types of `int name(...)` in the header, comments stripped, as the names of their ctypes twins.  Device pointers
    (d_*) travel as void pointers, host arrays of doubles as double pointers."""
    text = re.sub(r'/\*.*?\*/', '', header[header.index('int ' + name + '('):], flags=re.S)
    args = text[text.index('(') + 1:text.index(');')]
    out = []
    for a in args.split(','):
        a = ' '.join(a.split())
        m = re.match(r'(.*?)(\w+)$', a)
        typ, var = m.group(1).strip(), m.group(2)
        if typ == 'const double *' and var.startswith('d_'):
            typ = 'double *'
        out.append(_C2CT[typ])
    return out


def test_library_exports_and_declares_the_entry_points():
    from ssmtoybox_amd import _lib, ssinf, ssmod
    header = open(os.path.join(ROOT, 'include', 'ssmq.h')).read()
    lib = ctypes.CDLL(_lib.library_path())
    for name in ('ssmq_filter_masked_dev', 'ssmq_masked_kernel_name', 'ssmq_detection_mask_dev'):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
        assert 'int ' + name + '(' in header
        restype, argtypes = _lib._PROTOTYPES[name]
        assert restype is ctypes.c_int
        assert [t.__name__ for t in argtypes] == _declared(header, name), name
    assert _lib.MASKED_LAUNCH_LOOP == 1 and '#define SSMQ_MASKED_LAUNCH_LOOP 1' in header
    assert _lib.RTC_MASKED == 13 and 'SSMQ_RTC_MASKED = 13' in header
    for name in ('masked_pass', 'masked_pass_batch', 'masked_pass_dev', 'masked_kernel_name'):
        assert callable(getattr(ssinf.GaussianInference, name))
    assert callable(ssmod.detection_mask_dev)


def test_user_pendulum_pair_compiles_for_gfx950_without_a_device():
    from ssmtoybox_amd import _lib, ssmod
    from ssmtoybox_amd.mtran import resolve_integrand
    from tests.test_innovation_host import pendulum_user
    UP, UM = pendulum_user()
    f_dyn, _ = resolve_integrand(UP(ssmod.GaussRV(2), ssmod.GaussRV(2)).dyn_eval)
    f_obs, _ = resolve_integrand(UM(ssmod.GaussRV(1), 2).meas_eval)
    for form, n in ((_lib.FORM_SIGMA, 5), (_lib.FORM_BQ, 5)):
        rc, log = _lib.rtc_compile_check(f_dyn.id, _lib.RTC_MASKED, 2, 1, n, form, fid_obs=f_obs.id, N_obs=n, arch='gfx950')
        assert rc == 0, log
        assert 'k_masked_loop' in log and 'ScratchSize [bytes/lane]: 0' in log, log
    rc, _ = _lib.rtc_compile_check(f_dyn.id, _lib.RTC_MASKED, 2, 1, 5, _lib.FORM_SIGMA, opt=2, fid_obs=f_obs.id, N_obs=5)
    assert rc == -1


def test_restated_mask_generator_has_the_detection_frequencies():
    """Within 6 binomial standard deviations of p_detect, per component; per_component=False: the bits go together; the bits of a
    trajectory depend on its global index alone."""
    B, T, p = 400, 10, np.array([0.9, 0.6, 0.3, 0.05])
    m = mko.detection_mask(B, T, 4, p, seed=7)
    n = B * T
    for i in range(4):
        f = float(np.mean((m >> i) & 1))
        assert abs(f - p[i]) <= 6.0 * np.sqrt(p[i] * (1 - p[i]) / n), (i, f)
    assert np.all(m < 16)
    s = mko.detection_mask(B, T, 4, [0.8], seed=7, per_component=False)
    assert set(np.unique(s)) == {0, 15} and abs(float(np.mean(s == 15)) - 0.8) <= 6.0 * np.sqrt(0.16 / n)
    assert np.array_equal(mko.detection_mask(20, T, 4, p, seed=7, traj_offset=30), m[:, 30:50])
    assert not np.array_equal(mko.detection_mask(20, T, 4, p, seed=8), m[:, :20])
    assert mko.detection_mask(3, 2, 4, [0.0] * 4).max() == 0 and mko.detection_mask(3, 2, 4, [1.0] * 4).min() == 15
