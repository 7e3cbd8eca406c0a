"""
ML-II on the device (csrc/ssmq_ml2.hip k_ml2: ssmq_gp_nlml_batch / ssmq_gp_ml2_batch) against the reference's
neg_log_marginal_likelihood and Model.optimize recorded in tests/golden/g16_ml2.npz (make_golden_ml2.py).
"""
import os

import numpy as np
import pytest

from ssmtoybox_amd.bq.bqmod import GaussianProcessModel, StudentTProcessModel

pytestmark = pytest.mark.gpu

G16 = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g16_ml2.npz')
NU = 3.0
EPS = np.finfo(float).eps


@pytest.fixture(scope='module')
def g16():
    return dict(np.load(G16))


@pytest.fixture(scope='module', autouse=True)
def device():
    import ssmtoybox_amd as amd
    if amd.device_count() < 1:
        pytest.fail('no device: these tests need a GPU')
    amd.set_device(0)


def model(kind, D):
    par = np.ones((1, D + 1))
    if kind == 'gp':
        return GaussianProcessModel(D, par, 'rbf', 'ut')
    return StudentTProcessModel(D, par, 'rbf', 'ut', nu=NU)


def nlml_cases(g):
    return sorted({k[len('nlml_'):-len('_lp')] for k in g if k.startswith('nlml_') and k.endswith('_lp')})


CASES = ['gh15_e1', 'gh15_e3', 'gh10_e1', 'gh10_e3', 'ut5_e1', 'ut5_e3', 'sc100_e1', 'sc100_e3', 'sc64_e1', 'sc64_e3',
         'sc65_e1', 'sc65_e3']


def test_fixture_cases_are_covered(g16):
    assert sorted(CASES) == nlml_cases(g16)


@pytest.mark.parametrize('kind', ['gp', 'tp'])
@pytest.mark.parametrize('case', CASES)
def test_nlml_against_reference(g16, case, kind):
    """Value to 1e-10 relative, gradient to 1e-8 of its norm (times cond(K) eps / 1e-8 where K is ill-conditioned); N = 64
    (dense LDS route) and N = 65 (packed route) among them."""
    x, y, lp = g16['nlml_{}_x'.format(case)], g16['nlml_{}_y'.format(case)], g16['nlml_{}_lp'.format(case)]
    f_ref, g_ref = g16['nlml_{}_{}_f'.format(case, kind)], g16['nlml_{}_{}_g'.format(case, kind)]
    cond = g16['nlml_{}_cond'.format(case)]
    m = model(kind, x.shape[0])
    N = x.shape[1]
    jit = 1e-8 * np.eye(N)
    B = lp.shape[0]
    f, g = m.neg_log_marginal_likelihood_batch(lp, np.broadcast_to(y, (B,) + y.shape), x, jit)
    for k in range(B):
        fbar = max(1e-10, 20 * cond[k] * EPS)
        assert abs(f[k] - f_ref[k]) <= fbar * max(1.0, abs(f_ref[k])), (case, kind, k, f[k], f_ref[k], cond[k])
        gbar = max(1e-8, 20 * cond[k] * EPS)
        assert np.linalg.norm(g[k] - g_ref[k]) <= gbar * np.linalg.norm(g_ref[k]), (case, kind, k, g[k], g_ref[k], cond[k])
        # the single-row method is the same computation
        f1, g1 = m.neg_log_marginal_likelihood(lp[k], y, x, jit)
        assert f1 == f[k] and np.array_equal(g1, g[k])


@pytest.mark.parametrize('kind', ['gp', 'tp'])
def test_alpha_gradient_quirk(g16, kind):
    """der_par differentiates with respect to alpha, not log alpha: the first gradient entry times alpha is the derivative
    of the value along log alpha (central difference), and the rows with alpha != 1 tell the two apart."""
    x, y, lp = g16['nlml_ut5_e3_x'], g16['nlml_ut5_e3_y'], g16['nlml_ut5_e3_lp']
    m = model(kind, 5)
    jit = 1e-8 * np.eye(x.shape[1])
    h = 1e-5
    for k in (1, 2):                        # alpha = 0.3, 2.5
        alpha = np.exp(lp[k, 0])
        assert abs(alpha - 1.0) > 0.5
        f, g = m.neg_log_marginal_likelihood(lp[k], y, x, jit)
        up, dn = lp[k].copy(), lp[k].copy()
        up[0] += h
        dn[0] -= h
        fd = (m.neg_log_marginal_likelihood(up, y, x, jit)[0] - m.neg_log_marginal_likelihood(dn, y, x, jit)[0]) / (2 * h)
        assert abs(g[0] * alpha - fd) <= 1e-6 * max(1.0, abs(fd)), (g[0], alpha, fd)
        assert abs(g[0] - fd) > 1e-3 * abs(fd)
        # length-scale entries are true log-derivatives
        for d in range(1, 6):
            up, dn = lp[k].copy(), lp[k].copy()
            up[d] += h
            dn[d] -= h
            fd = (m.neg_log_marginal_likelihood(up, y, x, jit)[0] - m.neg_log_marginal_likelihood(dn, y, x, jit)[0]) / (2 * h)
            assert abs(g[d] - fd) <= 1e-6 * max(1.0, abs(fd))


def test_check_grad_at_unit_alpha():
    """The reference's gradient test (tests/test_bqmod.py:88-96): 5-D UT points, alpha = 1, check_grad <= 1e-5."""
    from scipy.optimize import check_grad
    m = GaussianProcessModel(5, np.ones((1, 6)), 'rbf', 'ut', {'alpha': 1.0})
    y = np.sin((m.points + 1) ** -1).T                   # (N, 5): one output per input dimension, as fcn(points).T
    jit = 1e-8 * np.eye(m.num_pts)
    lhyp = np.log([1.0] + 5 * [3.0])
    err = check_grad(lambda lp: m.neg_log_marginal_likelihood(lp, y[:, :1], m.points, jit)[0],
                     lambda lp: m.neg_log_marginal_likelihood(lp, y[:, :1], m.points, jit)[1], lhyp)
    assert err <= 1e-5, err


def opt_cases(g):
    return sorted({k[len('opt_'):-len('_x0')] for k in g if k.startswith('opt_') and k.endswith('_x0')})


def test_optimize_against_reference(g16):
    names = opt_cases(g16)
    assert len(names) >= 7
    for name in names:
        kind = name.split('_')[0]
        x_obs, y, x0 = g16['opt_{}_x_obs'.format(name)], g16['opt_{}_y'.format(name)], g16['opt_{}_x0'.format(name)]
        m = model(kind, x_obs.shape[0])
        res = m.optimize(x0, y, x_obs, method='BFGS')
        assert res.status == int(g16['opt_{}_status'.format(name)]), (name, res.message)
        assert abs(res.nit - int(g16['opt_{}_nit'.format(name)])) <= 1, (name, res.nit)
        xr = g16['opt_{}_x'.format(name)]
        assert np.abs(res.x - xr).max() <= 1e-6 * max(1.0, np.abs(xr).max()), (name, res.x, xr)
        fr = float(g16['opt_{}_fun'.format(name)])
        assert abs(res.fun - fr) <= 1e-10 * max(1.0, abs(fr)), (name, res.fun, fr)
        assert res.success == (res.status == 0) and set(res.keys()) >= {'x', 'fun', 'jac', 'hess_inv', 'nit', 'nfev',
                                                                         'njev', 'status', 'success', 'message'}


def test_optimize_batch_equals_single_calls():
    """1 000 fits with different data in one launch equal 1 000 single calls bit for bit; fun and jac of each fit are the
    objective's value and gradient at its x, bit for bit."""
    rng = np.random.default_rng(5)
    B, D = 1000, 2
    m = GaussianProcessModel(D, np.ones((1, D + 1)), 'rbf', 'ut')
    x = m.points
    N = x.shape[1]
    y = np.sin((x + 1) ** -1).sum(axis=0)[None, :, None] + 0.05 * rng.standard_normal((B, N, 2))
    x0 = np.log(np.array([1.0, 3.0, 3.0])) + 0.2 * rng.standard_normal((B, D + 1))
    r = m.optimize_batch(x0, y, x)
    assert r['x'].shape == (B, D + 1) and r['hess_inv'].shape == (B, D + 1, D + 1)
    assert np.mean(r['status'] == 0) > 0.9
    for b in range(B):
        s = m.optimize(x0[b], y[b], x)
        assert np.array_equal(s.x, r['x'][b]) and s.fun == r['fun'][b] and np.array_equal(s.jac, r['jac'][b]), b
        assert np.array_equal(s.hess_inv, r['hess_inv'][b]) and (s.nit, s.status, s.nfev) == (
            r['nit'][b], r['status'][b], r['nfev'][b]), b
    f, g = m.neg_log_marginal_likelihood_batch(r['x'], y, x, 1e-8 * np.eye(N))
    assert np.array_equal(f, r['fun']) and np.array_equal(g, r['jac'])


def test_failed_cholesky_row_is_isolated():
    """A row whose K + jitter is not positive definite gets NaNs (and the single-row method raises as the reference does);
    the other rows are what they are without it."""
    rng = np.random.default_rng(9)
    D, N, B = 1, 12, 6
    m = GaussianProcessModel(D, np.ones((1, D + 1)), 'rbf', 'ut')
    x = np.linspace(-20, 20, N)[None, :]                 # far apart: K ~ alpha^2 I
    jit = -0.5 * np.eye(N)                               # alpha = 1: K + jitter ~ 0.5 I; alpha = 0.5: ~ -0.25 I
    lp = np.log(np.column_stack([np.ones(B), 0.5 + rng.random(B)]))
    lp[3, 0] = np.log(0.5)
    y = rng.standard_normal((B, N, 1))
    f, g = m.neg_log_marginal_likelihood_batch(lp, y, x, jit)
    assert np.isnan(f[3]) and np.isnan(g[3]).all()
    keep = [b for b in range(B) if b != 3]
    f2, g2 = m.neg_log_marginal_likelihood_batch(lp[keep], y[keep], x, jit)
    assert np.array_equal(f[keep], f2) and np.array_equal(g[keep], g2) and np.isfinite(f2).all()
    with pytest.raises(np.linalg.LinAlgError):
        m.neg_log_marginal_likelihood(lp[3], y[3], x, jit)
    # a fit that starts there stops with scipy's NaN status; the others are unaffected
    r = m.optimize_batch(lp, y, x)
    r2 = m.optimize_batch(lp[keep], y[keep], x)
    for k in ('x', 'fun', 'jac', 'nit', 'status'):
        assert np.array_equal(r[k][keep], r2[k], equal_nan=True), k


def test_fit_then_transform():
    """The README's example: fit the kernel of a GP quadrature transform to data, then use the fitted parameters."""
    import ssmtoybox_amd as amd
    tf0 = amd.GaussianProcessTransform(1, 1, np.array([[1.0, 0.5]]), point_str='gh', point_par={'degree': 15})
    x = tf0.model.points
    y = np.sin((x + 1) ** -1).T
    res = tf0.model.optimize(np.log([1.0, 0.5]), y, x)
    assert res.success
    tf = amd.GaussianProcessTransform(1, 1, np.exp(res.x)[None, :], point_str='gh', point_par={'degree': 15})
    assert np.all(np.isfinite(tf.wm))
