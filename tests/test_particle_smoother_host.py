"""The particle smoothers without a device: the two symbols, every refusal through the C ABI and Python, and the NumPy restatement
(tests/_particle_smoother_oracle.py) against an unvectorised long-double form, its own invariants, the closed-form RTS smoother and
the filter it starts from."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import _particle_oracle as po
from tests import _particle_smoother_oracle as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_UNSUPPORTED = -1, -3
MARGINAL, GENEALOGY = 0, 1


def test_symbols_and_version():
    from ssmtoybox_amd import _lib
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'ssmq.h')).read(), flags=re.S)
    lib = _lib.load()
    for name in ('ssmq_particle_smoother_dev', 'ssmq_particle_smoother_kernel_name'):
        assert re.search(r'\b' + name + r'\s*\(', hdr), name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert re.search(r'SSMQ_PS_MARGINAL\s*=\s*0\s*,\s*SSMQ_PS_GENEALOGY\s*=\s*1', hdr)
    assert lib.ssmq_version() == _lib.ABI_VERSION == 102


def _c_call(fid, D, dq, N, method, q_chol=None, G=None, par=(), T=4, run=True):
    """Both entry points; the pass itself with an empty batch (B = 0: nothing is launched, no pointer is read) and only where `run`."""
    from ssmtoybox_amd import _lib
    lib = _lib.load()
    f_dyn = _lib.Integrand.make(fid, par)
    qL = np.ascontiguousarray(np.eye(dq) if q_chol is None else q_chol, dtype=np.float64)
    Gc = None if G is None else np.ascontiguousarray(G, dtype=np.float64)
    buf = ctypes.create_string_buffer(256)
    rc_name = lib.ssmq_particle_smoother_kernel_name(ctypes.byref(f_dyn), D, dq, N, None, _lib.dp(qL), _lib.dp(Gc), method, buf, 256)
    msg = _lib.last_error() if rc_name else buf.value.decode()
    if not run:
        return rc_name, None, msg
    dummy = ctypes.c_void_p(4096)
    rc = lib.ssmq_particle_smoother_dev(ctypes.byref(f_dyn), D, dq, N, 0, 64, T, None, _lib.dp(qL), _lib.dp(Gc), method, *([dummy] * 10),
                                        None, None, None)
    return rc_name, rc, msg


def test_refusals_c_abi():
    """Every refusal returns its code from both entry points, before a device is looked for."""
    from ssmtoybox_amd import _lib
    ungm = (_lib.F_UNGM_DYN, 1, 1)
    for method in (MARGINAL, GENEALOGY):
        assert _c_call(*ungm, 100, method)[:2] == (E_ARG, E_ARG)                               # N no multiple of 64
        assert _c_call(*ungm, 32, method)[:2] == (E_ARG, E_ARG)                                # N below 64
        assert _c_call(*ungm, 8192, method)[:2] == (E_UNSUPPORTED, E_UNSUPPORTED)              # N beyond 4096
        assert _c_call(15, 6, 6, 2048, method, par=(0.1,))[:2] == (E_UNSUPPORTED, E_UNSUPPORTED)   # (2 D + 1) N > 13312
        assert _c_call(1024, 1, 1, 64, method)[:2] == (E_UNSUPPORTED, E_UNSUPPORTED)           # a user model
        assert _c_call(13, 5, 2, 64, method)[:2] == (E_UNSUPPORTED, E_UNSUPPORTED)             # CTRS: noise as an argument
        assert _c_call(_lib.F_UNGM_DYN, 2, 2, 64, method)[:2] == (E_ARG, E_ARG)                # dimension mismatch
    assert _c_call(*ungm, 64, 2)[:2] == (E_ARG, E_ARG)                                         # unknown method
    name_rc, rc, name = _c_call(*ungm, 64, MARGINAL, T=0)
    assert name_rc == 0 and rc == E_ARG and 'k_particle_smooth<D=1>' in name                   # T = 0 (no part of the name query)
    # the LDS request: (2 D + 2) N + 96 doubles / 2 N + 96 doubles
    assert '11008 B' in _c_call(*ungm, 320, MARGINAL, run=False)[2]
    ok = _c_call(15, 6, 6, 1024, MARGINAL, par=(0.1,), run=False)
    assert ok[0] == 0 and 'k_particle_smooth<D=6>' in ok[2] and '115456 B' in ok[2]
    ok = _c_call(_lib.F_UNGM_DYN, 1, 1, 4096, MARGINAL, run=False)
    assert ok[0] == 0 and '131840 B' in ok[2]                                                  # the largest: 16384 + 96 doubles
    ok = _c_call(14, 4, 2, 128, GENEALOGY, par=(0.5,), run=False)
    assert ok[0] == 0 and 'k_particle_lineage<D=4>' in ok[2] and '2816 B' in ok[2]
    # the marginal method needs a transition density: dq == D and G Q G' positive definite, condition number at most 1e12
    for res in (_c_call(14, 4, 2, 128, MARGINAL, par=(0.5,)),                                  # constant velocity: dq = 2, D = 4
                _c_call(11, 5, 5, 128, MARGINAL, par=(0.2,), G=np.diag([1.0, 1.0, 1.0, 1.0, 0.0])),   # a noise-free state
                _c_call(11, 5, 5, 128, MARGINAL, par=(0.2,), G=np.ones((5, 5)))):                     # rank one
        assert res[:2] == (E_UNSUPPORTED, E_UNSUPPORTED), res
        assert "G Q G'" in res[2] and "method='genealogy'" in res[2], res[2]
    bad = _c_call(11, 5, 5, 128, MARGINAL, par=(0.2,), q_chol=np.diag([1.0, 1.0, 1.0, 1.0, 1e-7]))    # condition number 1e14
    assert bad[:2] == (E_ARG, E_ARG) and '1e12' in bad[2], bad
    assert _c_call(11, 5, 5, 128, MARGINAL, par=(0.2,), q_chol=np.diag([1.0, 1.0, 1.0, 1.0, 1e-5]), run=False)[0] == 0   # 1e10
    assert _c_call(11, 5, 5, 128, GENEALOGY, par=(0.2,), G=np.ones((5, 5)), run=False)[0] == 0   # genealogy reads no noise


def test_refusals_python():
    from ssmtoybox_amd import ssinf
    cv = ssinf.BootstrapParticleFilter(*so.package_models('cv_radar'), num_particles=128)
    with pytest.raises(NotImplementedError, match="G Q G'.*method='genealogy'"):
        cv.smoother_kernel_name('marginal')
    with pytest.raises(NotImplementedError, match="G Q G'.*method='genealogy'"):       # before the device is touched
        cv.smoother_batch(np.zeros((2, 3, 2)))
    with pytest.raises(NotImplementedError, match="G Q G'"):
        cv.smoother_dev(None, 2, 64, 3)
    assert 'k_particle_lineage<D=4>' in cv.smoother_kernel_name('genealogy')
    for name, N in (('ungm', 320), ('pend_t', 64), ('ct', 128)):
        pf = ssinf.BootstrapParticleFilter(*so.package_models(name), num_particles=N)
        D = pf.mod_dyn.dim_state
        assert 'k_particle_smooth<D=%d>' % D in pf.smoother_kernel_name() and 'k_particle_lineage<D=%d>' % D in pf.smoother_kernel_name('genealogy')
    for call in (lambda: pf.smoother_kernel_name('ffbsi'), lambda: pf.smoother_batch(np.zeros((2, 3, 2)), method='backward'),
                 lambda: pf.smoother(np.zeros((2, 3)), 'x'), lambda: pf.smoother_dev(None, 2, 64, 3, method=None)):
        with pytest.raises(ValueError, match='unknown smoother method'):
            call()
    with pytest.raises(ValueError, match='at least one time step'):
        pf.smoother_batch(np.zeros((2, 0, 3)))
    assert pf.cloud_block(6, 5, (8 * 6 + 4) * 6 * 128 * 2) == 2 and pf.cloud_block(6, 5, 1) == 1 and pf.cloud_block(6, 5) == 5
    for call in (pf.backward_pass, pf.backward_pass_batch, lambda: pf.iterated_smoother(None), lambda: pf.iterated_smoother_batch(None)):
        with pytest.raises(NotImplementedError, match='13312'):                       # the Gaussian smoothers stay refused
            call()
    assert 'smoother_batch' in ssinf.BootstrapParticleFilter.RANGE and 'x_{-1}' in ssinf.BootstrapParticleFilter.smoother_batch.__doc__


def _synthetic_cloud(N=8, T=3, D=2, seed=3):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((D, N, T))
    lw = rng.standard_normal((N, T))
    lw[2, 1] = -np.inf                                          # a particle of zero weight contributes nothing
    lw -= so.lse(lw, axis=0)[None, :]
    anc = rng.integers(0, N, (N, T))
    q = np.array([[0.5, 0.2], [0.2, 0.3]])
    model = po.Model(lambda x, t: np.stack((0.9 * x[0] + 0.1 * np.sin(x[1] + t), 0.8 * x[1])), lambda x, t: x[:1], D, 1, [0.1, -0.2],
                     np.linalg.cholesky(q), np.array([[1.0, 0.2], [0.0, 1.0]]), [0.0], [[1.0]])
    return model, x, lw, anc


def test_oracle_against_the_triple_loop():
    """The vectorised restatement against an unvectorised triple loop in long double on a synthetic cloud (N = 8, T = 3, D = 2, a
    correlated Q, a noise gain that is not the identity, a noise mean, one particle of zero weight): 1e-12."""
    model, x, lw, anc = _synthetic_cloud()
    ref = so.marginal_loops(model, x, lw, 3)
    for dtype in (np.float64, so.LD):
        got = so.marginal(model, x, lw, 3, dtype=dtype)['ls']
        fin = np.isfinite(ref)
        assert np.array_equal(np.isfinite(got), fin) and not fin.all()
        assert float(np.max(np.abs(got[fin] - ref[fin]) / (1 + np.abs(ref[fin])))) <= 1e-12
    s = so.marginal(model, x, lw, 3)
    for k in range(3):
        w = np.exp(s['ls'][:, k])
        np.testing.assert_allclose(s['sm'][:, k], x[:, :, k].dot(w), rtol=1e-13)
        np.testing.assert_allclose(s['ess'][k], 1.0 / np.sum(w * w), rtol=1e-13)
    g = so.genealogy(x, lw, anc, 3)
    assert np.array_equal(g['idx'][:, 2], np.arange(8)) and np.array_equal(g['idx'][:, 1], anc[:, 1])
    assert np.array_equal(g['idx'][:, 0], anc[anc[:, 1], 0])
    np.testing.assert_allclose(g['sm'][:, 0], x[:, anc[anc[:, 1], 0], 0].dot(np.exp(lw[:, 2])), rtol=1e-13)


@pytest.mark.parametrize('name,N', [(n, N) for n, Ns in so.CASES.items() for N in Ns])
def test_oracle_invariants(name, N):
    """On the oracle's own clouds of the GPU test's cases: the un-normalised ls_k has log-sum-exp 0 to 64 N eps (the recursion
    conserves the mass), the float64 form agrees with the long-double one within the bound the GPU test uses, and `unique` does not
    increase backwards in time."""
    model, m0, P0, _ = so.case(name)
    y = so.case_data(name)
    for b in range(so.B):
        o = po.full_pass(model, y[:, :, b], m0, P0, so.SEED, b, N, so.ESS_THRESHOLD)
        assert o['status'] == 0
        g = so.genealogy(o['x'], o['lwn'], o['anc'], so.T)
        assert g['unique'][-1] == N and np.all(np.diff(g['unique']) >= 0) and g['unique'][0] >= 1
        assert np.all(g['idx'] >= 0) and np.all(g['idx'] < N)
        if 'marginal' not in so.METHODS[name]:
            continue
        s, sl = so.marginal(model, o['x'], o['lwn'], so.T), so.marginal(model, o['x'], o['lwn'], so.T, dtype=so.LD)
        assert float(np.max(np.abs(so.lse(s['ls_raw'], axis=0)))) <= 64 * N * so.EPS
        tol = max(1e-10, 64 * so.EPS * np.linalg.cond(so.sigma(model)))
        big = sl['ls'] > -700
        assert float(np.max(np.abs(s['ls'][big] - sl['ls'][big]) / (1 + np.abs(sl['ls'][big])))) <= tol
        assert np.all(np.isfinite(s['sm'])) and np.all(s['ess'] >= 1 - 1e-9) and np.all(s['ess'] <= N * (1 + 1e-9))


def _rts(a, Q, R, m0, P0, y):
    """Closed-form Kalman filter and RTS smoother of x_j = a x_{j-1} + q, y_j = x_j + r, x_{-1} ~ N(m0, P0): (ms, Ps) of steps 0 .. T-1."""
    T = y.size
    mp, Pp, mf, Pf = np.empty(T), np.empty(T), np.empty(T), np.empty(T)
    m, P = m0, P0
    for j in range(T):
        mp[j], Pp[j] = a * m, a * a * P + Q
        K = Pp[j] / (Pp[j] + R)
        m, P = mp[j] + K * (y[j] - mp[j]), (1 - K) * Pp[j]
        mf[j], Pf[j] = m, P
    ms, Ps = mf.copy(), Pf.copy()
    for j in range(T - 2, -1, -1):
        Gj = Pf[j] * a / Pp[j + 1]
        ms[j] = mf[j] + Gj * (ms[j + 1] - mp[j + 1])
        Ps[j] = Pf[j] + Gj * Gj * (Ps[j + 1] - Pp[j + 1])
    return ms, Ps


def test_oracle_against_the_rts_smoother():
    """A scalar linear-Gaussian model, f = 0.9 x, h = x (Q = 0.5, R = 0.4, x_{-1} ~ N(0.3, 2)), where the RTS smoother is the exact
    smoothing posterior: the oracle's full pass plus FFBSm at N = 2048, T = 8 (data seed 5, filter seed 0) has
    |m - m_RTS| <= 6 sqrt(P_RTS / ess_s) at every step.  Largest observed ratio |m - m_RTS| / sqrt(P_RTS / ess_s): 0.873 (step 7; the
    others 0.05 .. 0.68); the smoothed variances are within 5.3 % of P_RTS."""
    a, Q, R, m0, P0, T, N = 0.9, 0.5, 0.4, np.array([0.3]), np.array([[2.0]]), 8, 2048
    model = po.Model(lambda x, t: a * x, lambda x, t: x, 1, 1, [0.0], [[np.sqrt(Q)]], np.eye(1), [0.0], [[np.sqrt(R)]])
    rng = np.random.default_rng(5)
    x, y = m0[0] + np.sqrt(P0[0, 0]) * rng.standard_normal(), np.empty((1, T))
    for j in range(T):
        x = a * x + np.sqrt(Q) * rng.standard_normal()
        y[0, j] = x + np.sqrt(R) * rng.standard_normal()
    ms, Ps = _rts(a, Q, R, m0[0], P0[0, 0], y[0])
    o = po.full_pass(model, y, m0, P0, 0, 0, N, 0.5)
    s = so.marginal(model, o['x'], o['lwn'], T)
    ratio = np.abs(s['sm'][0] - ms) / np.sqrt(Ps / s['ess'])
    print('ratios', np.round(ratio, 3), 'variance ratios', np.round(s['sP'][0, 0] / Ps, 3))
    assert np.all(s['ess'] > 100)
    assert np.all(ratio <= 6), ratio
    assert np.all(np.abs(s['sP'][0, 0] / Ps - 1) <= 0.25)
    # the genealogy estimate answers the same question: at the last steps, where the lineages have not collapsed, it agrees as well
    g = so.genealogy(o['x'], o['lwn'], o['anc'], T)
    assert np.all(np.abs(g['sm'][0, -3:] - ms[-3:]) <= 6 * np.sqrt(Ps[-3:] / np.minimum(g['unique'][-3:], g['ess'][-3:])))


STUDY_CPU = dict(B=64, T=po.STUDY['T'], N=256)          # the study's sizes reduced: B = 256, N = 512 takes 40 s in NumPy


def test_smoothing_beats_filtering_on_the_cpu():
    """What tests/test_particle_smoother_gpu.py::test_smoothing_beats_filtering relies on, established here first: UNGM on planes
    aligned with the filters' time convention (`po.study_cpu`), seed 11, T = 20, the oracle's full pass and FFBSm over its cloud,
    time-averaged RMSE over the batch of the filtered against the smoothed means, the standard error of the difference by a bootstrap
    over the trajectories (`po.bootstrap_se`).
      B = 64, N = 256 (this test):       filtered 4.9067, smoothed 2.0473, gap 2.8595 = 18.1 standard errors (0.1581)
      B = 256, N = 512 (`po.STUDY`):     filtered 4.5523, smoothed 1.7529, gap 2.7994 = 30.0 standard errors (0.0934)"""
    r_f, r_s = so.study_cpu(po.STUDY['seed'], **STUDY_CPU)
    gap, se = float(np.mean(r_f - r_s)), po.bootstrap_se(r_f - r_s)
    print('filtered %.4f, smoothed %.4f, gap %.4f, standard error %.4f' % (r_f.mean(), r_s.mean(), gap, se))
    assert gap >= 3 * se, (gap, se)
