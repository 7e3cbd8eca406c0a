"""The 'rbf-student' kernel on the device: Monte-Carlo expectations against the exact mixture oracle (tests/_student_oracle.py)
within bounds derived from the oracle's exact per-sample variances, the reference's exp_xy_kxy estimator, determinism, the weight
algebra, the transform and the TPQSF built from it, and the refusals."""
import numpy as np
import pytest

from tests import _student_oracle as so
from tests._cases import RTOL, rel_err, within

pytestmark = pytest.mark.gpu

Z = 6.0
SAMPLES = (100000, 2000000)
SEED = 11


@pytest.fixture(scope='module')
def amd():
    import ssmtoybox_amd
    if ssmtoybox_amd.device_count() < 1:
        pytest.fail('no device: the GPU tests need an MI355X')
    ssmtoybox_amd.set_device(0)
    return ssmtoybox_amd


@pytest.fixture(scope='module')
def golden18():
    import os
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g18_rbf_student.npz'))


_ORACLE = {}


def _oracle(name, x, par, dof):
    key = (name, dof)
    if key not in _ORACLE:
        _ORACLE[key] = so.expectations(x, par, dof)
    return _ORACLE[key]


def _setup(case, S, seed=SEED):
    from ssmtoybox_amd.bq.bqkern import RBFStudent
    name, D, ell, ppar, N, alpha, dof = case
    x = so.fs_points(D, ppar)
    assert x.shape == (D, N)
    par = np.array([[alpha] + [ell] * D])
    return RBFStudent(D, par, dof=dof, num_samples=S, seed=seed), x, par


@pytest.mark.parametrize('S', SAMPLES)
@pytest.mark.parametrize('case', so.CASES, ids=[c[0] for c in so.CASES])
def test_expectations_within_six_standard_errors(amd, case, S):
    """Every entry of q, R, Q within 6 sqrt(Var / S) of the oracle, Var the oracle's exact per-sample variance - and the bound
    can fail: the Gaussian closed form (every entry of q) and the nu = 5 oracle (worst entry) lie outside it at S = 2e6."""
    from ssmtoybox_amd.bq.bqkern import RBFGauss
    name, D, dof = case[0], case[1], case[6]
    k, x, par = _setup(case, S)
    if name == 'd1_fs3':
        assert np.array_equal(x, [[0.0, 3.0, -3.0]])
    o = _oracle(name, x, par[0], dof)
    got = dict(zip(('q', 'R', 'Q'), k.expectations(par, x)))
    for key in ('q', 'R', 'Q'):
        assert got[key].shape == o[key].shape and np.all(np.isfinite(got[key]))
        bound = Z * np.sqrt(o['var_' + key] / S)
        assert np.all(bound > 0)
        ratio = np.abs(got[key] - o[key]) / bound
        print('{} S={:.0e} {}: worst entry at {:.3f} of the bound'.format(name, S, key, ratio.max()))
        assert np.all(ratio <= 1.0), (key, float(ratio.max()))
    if S == SAMPLES[-1]:
        bq = Z * np.sqrt(o['var_q'] / S)
        gauss = np.abs(RBFGauss(D, par).exp_x_kx(par, x) - o['q']) / bq
        other = np.abs(_oracle(name, x, par[0], 5.0)['q'] - o['q']) / bq
        print('{}: Gaussian q {:.1f} .. {:.1f} bounds away, nu = 5 worst entry {:.1f} bounds away'.format(
            name, gauss.min(), gauss.max(), other.max()))
        assert np.all(gauss > 1.0) and other.max() > 1.0
        assert np.all(np.abs(RBFGauss(D, par).exp_x_kx(par, x) - got['q']) > 0)


@pytest.mark.parametrize('S', SAMPLES)
@pytest.mark.parametrize('case', so.CASES, ids=[c[0] for c in so.CASES])
def test_exp_xy_kxy_is_the_reference_estimator(amd, golden18, case, S):
    """Within 6 sqrt(10 000 Var T) / num_samples of alpha^2 (200 * 199 kappa + 200) * 10 000 / num_samples; kappa from the
    oracle, Var T the recorded variance of the reference's per-batch sums."""
    name, dof = case[0], case[6]
    k, x, par = _setup(case, S)
    value, sums = k.exp_xy_kxy(par, batch_sums=True)
    expected = so.kxy_expected(par[0], dof, S)
    bound = Z * np.sqrt(so.KXY_BATCHES * float(golden18[name + '_kxy_var'])) / S
    print('{} S={:.0e} kxy {:.6f} expected {:.6f} bound {:.6f}; batch-sum variance {:.1f} recorded {:.1f}'.format(
        name, S, value, expected, bound, sums.var(ddof=1), float(golden18[name + '_kxy_var'])))
    assert abs(value - expected) <= bound
    assert sums.shape == (10000,) and abs(sums.sum() / S - value) <= 1e-12 * abs(value)
    assert value == k.exp_xy_kxy(par)


def test_determinism_and_symmetry(amd, monkeypatch):
    case = so.CASES[2]                       # D = 5, N = 51
    k, x, par = _setup(case, 100000)
    q, R, Q = k.expectations(par, x)
    kxy = k.exp_xy_kxy(par)
    q2, R2, Q2 = k.expectations(par, x)
    assert np.array_equal(q, q2) and np.array_equal(R, R2) and np.array_equal(Q, Q2) and kxy == k.exp_xy_kxy(par)
    assert np.array_equal(Q, Q.T)
    assert np.array_equal(k.exp_x_kxkx(par, par, x), Q)
    assert np.array_equal(k.exp_x_kx(par, x), q) and np.array_equal(k.exp_x_xkx(par, x), R)
    # the launch grid does not enter the result
    for grid in ('1', '7', '64'):
        monkeypatch.setenv('SSMQ_STUDENT_MC_GRID', grid)
        q3, R3, Q3 = k.expectations(par, x)
        assert np.array_equal(q, q3) and np.array_equal(R, R3) and np.array_equal(Q, Q3), grid
        assert kxy == k.exp_xy_kxy(par), grid
    monkeypatch.delenv('SSMQ_STUDENT_MC_GRID')
    # a sample count that is not a multiple of the chunk, the slot or the MFMA's 4 samples
    k.num_samples = 100003
    qa = k.expectations(par, x)[0]
    monkeypatch.setenv('SSMQ_STUDENT_MC_GRID', '5')
    assert np.array_equal(qa, k.expectations(par, x)[0])
    monkeypatch.delenv('SSMQ_STUDENT_MC_GRID')
    k.num_samples = 100000
    # another seed differs
    k.seed = SEED + 1
    q4, R4, Q4 = k.expectations(par, x)
    assert not np.array_equal(q, q4) and not np.array_equal(Q, Q4) and not np.array_equal(R, R4)
    assert kxy != k.exp_xy_kxy(par)
    # scaling multiplies by alpha^2 (q, R) and alpha_0^2 alpha_1^2 (Q)
    k.seed = SEED
    p2 = par.copy()
    p2[0, 0] = 1.5
    assert np.allclose(k.exp_x_kx(p2, x, scaling=True), 2.25 * q, rtol=1e-15, atol=0)
    assert np.allclose(k.exp_x_kxkx(p2, p2, x, scaling=True), 2.25 ** 2 * Q, rtol=1e-15, atol=0)


def test_two_parameter_rows(amd):
    """exp_x_kxkx with two different parameter rows: Q[i, j] = E[k1_i k0_j] on the same samples (bq/bqkern.py:521-523).  Rows that
    differ in alpha only go through the two-kernel path and give the one-kernel Q to rounding; rows with different length-scales
    against the closed form of the product of two RBF factors, with Var(k1_i k0_j) <= Q (1 - Q) because 0 <= k <= 1."""
    case = so.CASES[1]                       # D = 2, N = 5
    S = 100000
    k, x, par = _setup(case, S)
    Q = k.exp_x_kxkx(par, par, x)
    pa = par.copy()
    pa[0, 0] = 2.0
    Qa = k.exp_x_kxkx(par, pa, x)
    assert np.max(np.abs(Qa - Q)) < 1e-13
    p1 = np.array([[1.0, 2.0, 4.0]])
    Q01, Q10 = k.exp_x_kxkx(par, p1, x), k.exp_x_kxkx(p1, par, x)
    assert np.max(np.abs(Q01 - Q10.T)) < 1e-13 and not np.allclose(Q01, Q01.T, atol=1e-6)
    h0, h1 = par[0, 1:] ** 2, p1[0, 1:] ** 2
    w = 1.0 / (1.0 / h0 + 1.0 / h1)
    xi, xj = x[:, :, None], x[:, None, :]                                   # i: k1 (p1), j: k0 (par)
    c = (xi / h1[:, None, None] + xj / h0[:, None, None]) * w[:, None, None]
    const = np.exp(-0.5 * np.sum((xi - xj) ** 2 / (h0 + h1)[:, None, None], axis=0))
    exact = so._mix(lambda s: (so._factor(s, w, c) * const).ravel(), case[6]).reshape(5, 5)
    bound = Z * np.sqrt(exact * (1.0 - exact) / S)
    ratio = np.abs(Q01 - exact) / bound
    print('two parameter rows: worst entry at {:.3f} of the bound'.format(ratio.max()))
    assert np.all(ratio <= 1.0)


@pytest.mark.parametrize('case', so.CASES, ids=[c[0] for c in so.CASES])
def test_weights_algebra(amd, case):
    """wm, Wc, Wcc, model_var, integral_var from the device against the NumPy restatement of bq/bqmod.py:495-523 applied to the
    device's own q, R, Q, iK, at the cond-scaled bars of the GP-weights tests (tests/test_gpu_parity.py: 64 cond eps for the
    single products, 8 cond^2 eps for the double ones, never below RTOL)."""
    from ssmtoybox_amd.bq.bqkern import device_student_weights
    name = case[0]
    k, x, par = _setup(case, 100000)
    w = device_student_weights(x, par, k)
    q, R, Q, iK = w['q'][0], w['R'][0], w['Q'][0], w['iK'][0]
    assert w['status'][0] == 0
    eps = 2.2e-16
    cond = np.linalg.cond(k.eval(par, x, scaling=False) + k.jitter * np.eye(x.shape[1]))
    tol1, tol2 = max(RTOL, 64 * cond * eps), max(RTOL, 8 * cond ** 2 * eps)
    wc = iK.dot(Q).dot(iK)
    wc = 0.5 * (wc + wc.T)
    t = 'rbf-student {} weights from given expectations: '.format(name)
    # the same inverse as eval_inv_dot's (bit for bit up to N = 64; above, the two entry points factorise by different routes)
    assert within(rel_err(iK, k.eval_inv_dot(par, x, scaling=False)), tol1, t + 'iK vs eval_inv_dot')
    assert within(rel_err(w['wm'][0], q.dot(iK)), tol1, t + 'wm')
    assert within(rel_err(w['Wcc'][0], R.dot(iK)), tol1, t + 'Wcc')
    assert within(rel_err(w['Wc'][0], wc), tol2, t + 'Wc')
    assert np.array_equal(w['Wc'][0], w['Wc'][0].T)
    mv = par[0, 0] ** 2 * (1.0 - np.trace(Q.dot(iK)))
    iv = w['kbar'] - q.dot(iK).dot(q)
    assert within(abs(w['model_var'][0] - mv) / max(1.0, abs(mv)), tol2, t + 'model_var')
    assert within(abs(w['integral_var'][0] - iv) / max(1.0, abs(iv)), tol2, t + 'integral_var')
    assert w['kbar'] == k.exp_xy_kxy(par)


def test_model_and_transform(amd):
    """The model caches what bq_weights computed; changing the kernel's attributes changes the next weights; the transform's
    apply equals that of an 'rbf' transform with the same weights injected, bit for bit; predict works, optimize is refused."""
    from ssmtoybox_amd import ssmod
    kp = np.array([[1.0, 1.0]])
    tf = amd.StudentTProcessTransform(1, 1, kp, 'rbf-student', 'fs', {'dof': 4})
    m = tf.model
    assert type(m.kernel).__name__ == 'RBFStudent' and m.kernel.dof == 4.0 and m.kernel.num_samples == 2000000
    o = so.expectations(m.points, kp[0], 4.0)
    assert np.all(np.abs(m.q - o['q']) <= Z * np.sqrt(o['var_q'] / 2e6))
    assert m.Q.shape == (3, 3) and m.R.shape == (1, 3) and m.iK.shape == (3, 3) and np.isfinite(m.model_var)
    assert np.isfinite(m.integral_var)
    ref = amd.StudentTProcessTransform(1, 1, kp, 'rbf', 'fs', {'dof': 4})
    assert not np.array_equal(ref.wm, tf.wm)
    ref.wm, ref.Wc, ref.Wcc = tf.wm, tf.Wc, tf.Wcc
    ref.model.model_var, ref.model.iK = m.model_var, m.iK
    f = ssmod.UNGMTransition(ssmod.StudentRV(1), ssmod.StudentRV(1)).dyn_eval
    mean, cov = np.array([0.3]), np.array([[1.7]])
    a, b = tf.apply(f, mean, cov, 2.0), ref.apply(f, mean, cov, 2.0)
    for u, v in zip(a, b):
        assert np.all(np.isfinite(u)) and np.array_equal(u, v)
    # new attributes, new weights; the same attributes again, the same weights
    wm0 = tf.wm.copy()
    m.kernel.seed, m.kernel.num_samples = 5, 100000
    wm1 = tf.weights(kp)[0]
    assert not np.array_equal(wm0, wm1)
    m.kernel.seed, m.kernel.num_samples = 0, 2000000
    assert np.array_equal(tf.weights(kp)[0], wm0)
    tg = amd.GaussianProcessTransform(2, 1, np.array([[1.5, 3.0, 3.0]]), 'rbf-student', 'fs', {'degree': 3},
                                      kern_attr={'num_samples': 100000, 'seed': 3, 'dof': 6.0})
    assert tg.model.kernel.dof == 6.0 and tg.wm.shape == (5,) and np.array_equal(tg.Wc, tg.Wc.T)
    mean_p, var_p = tg.model.predict(np.array([[0.1, 0.5], [0.2, -0.4]]), np.sin(tg.model.points).sum(axis=0))
    assert mean_p.shape == (2,) and var_p.shape == (2,) and np.all(np.isfinite(mean_p))
    with pytest.raises(NotImplementedError):
        tg.model.optimize(np.zeros(3), np.zeros(5), tg.model.points)


def test_tpqsf_native(amd):
    """StudentProcessStudent(kernel='rbf-student') on the UNGM Student system of g5_student: status 0 and finite output, the same
    bits from a second construction with the same seed, and the same bits as an 'rbf' filter with these weights injected."""
    import os
    from ssmtoybox_amd import ssinf, ssmod as sm
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g5_student.npz'))
    y = g['ungm_y']
    dyn = sm.UNGMTransition(sm.StudentRV(1), sm.StudentRV(1, scale=np.array([[10.0]])))
    obs = sm.UNGMMeasurement(sm.StudentRV(1), 1)
    kp = np.atleast_2d(np.ones(2))
    mc = {'num_samples': 2000000, 'seed': 21}
    alg = ssinf.StudentProcessStudent(dyn, obs, kp, kp, kernel='rbf-student', mc=mc)
    for tf, tag in ((alg.tf_dyn, 'dyn'), (alg.tf_obs, 'obs')):
        assert np.array_equal(tf.model.points, g['ungm_tpqs_' + tag + '_pts']) and tf.model.kernel.seed == 21
    fm, fP = alg.forward_pass_batch(y)
    assert np.all(np.isfinite(fm)) and np.all(np.isfinite(fP))
    assert alg.status is not None and alg.status.shape == (y.shape[-1],) and not alg.status.any()
    alg2 = ssinf.StudentProcessStudent(dyn, obs, kp, kp, kernel='rbf-student', mc=mc)
    fm2, fP2 = alg2.forward_pass_batch(y)
    assert np.array_equal(fm, fm2) and np.array_equal(fP, fP2)
    inj = ssinf.StudentProcessStudent(dyn, obs, kp, kp)
    for tf, src in ((inj.tf_dyn, alg.tf_dyn), (inj.tf_obs, alg.tf_obs)):
        tf.wm, tf.Wc, tf.Wcc = src.wm, src.Wc, src.Wcc
        tf.model.model_var, tf.model.iK = src.model.model_var, src.model.iK
    fm3, fP3 = inj.forward_pass_batch(y)
    assert np.array_equal(fm, fm3) and np.array_equal(fP, fP3)
    # recorded, not asserted: both sides carry independent Monte-Carlo noise amplified by iK
    print('TPQSF vs the reference trajectory (its own Monte-Carlo weights): mean deviation rel {:.3e}'.format(
        rel_err(fm, g['ungm_tpqs_fm'])))


def test_refusals_leave_outputs_untouched(amd):
    from ssmtoybox_amd import _lib
    lib = _lib.load()
    sentinel = -7.25
    q, R, Q = (np.full(s, sentinel) for s in ((200,), (17, 200), (200, 200)))
    dp = lambda a: a.ctypes.data_as(_lib.c_double_p)        # noqa: E731
    x = np.zeros((17, 200))
    par = np.ones(18)
    for D, N, S, dof in ((17, 5, 1000, 4.0), (0, 5, 1000, 4.0), (2, 129, 1000, 4.0), (2, 0, 1000, 4.0), (2, 5, 0, 4.0),
                         (2, 5, 2 ** 31, 4.0), (2, 5, 1000, 0.0), (2, 5, 1000, -2.0)):
        rc = lib.ssmq_rbf_student_expect(D, N, dp(x), dp(par), None, dof, S, 1, dp(q), dp(R), dp(Q))
        assert rc == -3, (D, N, S, dof, rc)                  # SSMQ_E_UNSUPPORTED
        assert 'D <= 16' in _lib.last_error()
        assert np.all(q == sentinel) and np.all(R == sentinel) and np.all(Q == sentinel)
    out, sums = np.full(1, sentinel), np.full(10000, sentinel)
    for D, S, dof in ((17, 1000, 4.0), (2, 0, 4.0), (2, 2 ** 31, 4.0), (2, 1000, 0.0)):
        assert lib.ssmq_rbf_student_kxy(D, dp(par), dof, S, 1, dp(out), dp(sums)) == -3
        assert out[0] == sentinel and np.all(sums == sentinel)
    w = [np.full(s, sentinel) for s in ((200,), (200, 200), (17, 200), (200, 200), (1,), (1,))]
    st = np.full(1, 77, dtype=np.int32)
    for D, N in ((17, 5), (2, 129)):
        rc = lib.ssmq_weights_gp_given(D, N, dp(x), dp(par), 1e-8, dp(q), dp(R), dp(Q), 1.0, *[dp(a) for a in w],
                                       st.ctypes.data_as(_lib.c_int32_p))
        assert rc == -3 and all(np.all(a == sentinel) for a in w) and st[0] == 77
    # in range, the same call works
    q5, R5, Q5 = np.empty(5), np.empty((2, 5)), np.empty((5, 5))
    x5 = np.ascontiguousarray(so.fs_points(2, {'degree': 3}))
    assert lib.ssmq_rbf_student_expect(2, 5, dp(x5), dp(par), None, 4.0, 1000, 1, dp(q5), dp(R5), dp(Q5)) == 0
    assert np.all(q5 > 0) and np.all(q5 <= 1)
