"""
Model.predict / predict_batch on the device (csrc/ssmq_predict.hip k_predict_fit + k_predict_test: ssmq_gp_predict_batch)
against the reference's predict recorded in tests/golden/g16_predict.npz (make_golden_predict.py), against the package's own
kernel methods, and against the interpolation identities.

Parity bar (test_golden_cases): the reference and the device both sit within cond(K) eps of the exact value, on different
summation orders, so the yardstick is how far the reference ITSELF is from an exact evaluation (stored per case by the
generator, 40-digit arithmetic): scaled error <= 8 x ref_err + 64 eps, errors of the mean scaled by max |fcn_obs|, of the
variance by alpha^2.  The factor allows for N-term sums in another order and the device's elementary functions; it is not
tuned against the device.  With SSMQ_PREDICT_PARITY_OUT set, the measured errors are appended to that file.
"""
import os

import numpy as np
import pytest

from ssmtoybox_amd import _lib
from ssmtoybox_amd.bq.bqmod import GaussianProcessModel, StudentTProcessModel, BayesSardModel

pytestmark = pytest.mark.gpu

G16P = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g16_predict.npz')
NU = 3.0
EPS = np.finfo(float).eps
CASES = ['gp_d1', 'gp_d2', 'tp_d1', 'tp_d2', 'bs_d1', 'bs_d2', 'gp_d2_e3', 'gp_d3_e2', 'bs_d2_e3', 'bs_d3_e2', 'gp_d6_e6',
         'gp_xo', 'tp_xo', 'bs_xo', 'gp_n128']
# the point set each case's model was built with (the TP denominator counts the model's points)
POINTS = {'d1': ('gh', {'degree': 15}), 'd2': ('gh', {'degree': 5}), 'd3': ('fs', {'degree': 5}), 'd6': ('ut', None),
          'xo': ('gh', {'degree': 5}), 'n128': ('ut', None)}


@pytest.fixture(scope='module')
def g16p():
    return dict(np.load(G16P))


@pytest.fixture(scope='module', autouse=True)
def device():
    import ssmtoybox_amd as amd
    if amd.device_count() < 1:
        pytest.fail('no device: these tests need a GPU')
    amd.set_device(0)


def model(kind, D, pts=('ut', None), par=None):
    par = np.ones((1, D + 1)) if par is None else np.atleast_2d(par)
    if kind == 'gp':
        return GaussianProcessModel(D, par, 'rbf', pts[0], pts[1])
    if kind == 'tp':
        return StudentTProcessModel(D, par, 'rbf', pts[0], pts[1], nu=NU)
    return BayesSardModel(D, par, 2, pts[0], pts[1])


def fcn(x):
    return np.sin((x + 1) ** -1)


def test_fixture_cases_are_covered(g16p):
    assert sorted(CASES) == sorted(str(c) for c in g16p['cases'])


@pytest.mark.parametrize('case', CASES)
def test_golden_cases(g16p, case):
    g = {k[len(case) + 1:]: v for k, v in g16p.items() if k.startswith(case + '_')}
    kind = str(g['kind'])
    x, y, xt, par = g['x'], g['y'], g['xt'], g['par']
    m = model(kind, x.shape[0], POINTS[case.split('_')[1]])
    assert m.num_pts == int(g['num_pts'])
    kw = {'mulind': g['mulind']} if kind == 'bs' else {}
    mean, var = m.predict(xt, y[0] if y.shape[0] == 1 else y, x, par, **kw)
    assert mean.shape == g['mean'].shape and var.shape == g['var'].shape == (xt.shape[1],)
    err_m = np.abs(mean - g['mean']).max() / np.abs(y).max()
    err_v = np.abs(var - g['var']).max() / par[0] ** 2
    bar_m, bar_v = 8 * float(g['ref_err_mean']) + 64 * EPS, 8 * float(g['ref_err_var']) + 64 * EPS
    line = '{:10s} N {:3d} M {:3d} E {:2d} cond {:.2e}  mean {:.3e} (bar {:.3e})  var {:.3e} (bar {:.3e})'.format(
        case, x.shape[1], xt.shape[1], y.shape[0], float(g['cond']), err_m, bar_m, err_v, bar_v)
    print(line)
    if os.environ.get('SSMQ_PREDICT_PARITY_OUT'):
        with open(os.environ['SSMQ_PREDICT_PARITY_OUT'], 'a') as f:
            f.write(line + '\n')
    assert err_m <= bar_m and err_v <= bar_v, line


def batch_data(rng, kind, D, N, E, B, M, per_fit):
    x = rng.standard_normal((B, D, N) if per_fit else (D, N))
    xt = 1.5 * rng.standard_normal((B, D, M) if per_fit else (D, M))
    y = rng.standard_normal((B, N, E))
    par = np.hstack((0.5 + rng.random((B, 1)), 0.4 + 0.3 * rng.random((B, D))))
    return x, xt, y, par


@pytest.mark.parametrize('per_fit', [False, True])
@pytest.mark.parametrize('B,M', [(1, 1), (3, 63), (3, 64), (3, 65), (3, 1000), (1000, 1), (1000, 65)])
@pytest.mark.parametrize('kind,D,N,E', [('gp', 6, 13, 6), ('gp', 2, 64, 1), ('gp', 3, 65, 2), ('tp', 2, 30, 1), ('tp', 2, 70, 1),
                                        ('bs', 2, 20, 3), ('bs', 2, 70, 1)])
def test_batch_rows_equal_single_calls(kind, D, N, E, B, M, per_fit):
    """Row b of predict_batch is bit-equal to predict on row b's data (every row for small B, a spread of rows at B = 1000);
    M on both sides of the 64-wide tile, N on both sides of 64 (dense and packed factorisation)."""
    rng = np.random.default_rng(1000 * N + 10 * M + B + per_fit)
    m = model(kind, D)
    x, xt, y, par = batch_data(rng, kind, D, N, E, B, M, per_fit)
    r = m.predict_batch(xt, y, x, par=par)
    assert r['mean'].shape == (B, M, E) and r['var'].shape == (B, M) and r['status'].dtype == np.int32
    assert not r['status'].any() and np.isfinite(r['mean']).all() and np.isfinite(r['var']).all()
    rows = range(B) if B <= 3 else sorted({0, 1, B // 2, B - 2, B - 1} | set(range(0, B, 97)))
    for b in rows:
        mean, var = m.predict(xt[b] if per_fit else xt, y[b].T, x[b] if per_fit else x, par[b])
        assert np.array_equal(np.squeeze(r['mean'][b]), mean) and np.array_equal(np.squeeze(r['var'][b]), var), (b, B, M)
    # one parameter row for all fits is the same as that row repeated
    r1 = m.predict_batch(xt, y, x, par=par[0])
    rB = m.predict_batch(xt, y, x, par=np.broadcast_to(par[0], par.shape))
    assert np.array_equal(r1['mean'], rB['mean']) and np.array_equal(r1['var'], rB['var'])


@pytest.mark.parametrize('N,D', [(25, 2), (64, 3), (100, 2)])
def test_kx_ties_to_the_kernel_methods(N, D):
    """fcn_obs = columns of the identity: the mean is then (kx iK)[:, :E], with kx and iK available from RBFGauss.eval and
    eval_inv_dot.  Bar: two N-term sums in different orders differ by at most 2 N eps sum |kx_n| |iK_nj|; the two kx agree to
    a few ulp of exp (2.5 ulp device, plus the exponent's rounding): 16 eps sum |kx_n| |iK_nj| more."""
    rng = np.random.default_rng(N)
    m = model('gp', D)
    x, xt = rng.standard_normal((D, N)), 1.5 * rng.standard_normal((D, 77))
    par = np.array([0.8] + [1.2] * D)
    E = 16
    y = np.eye(N)[:E]                                           # (E, N)
    mean, _ = m.predict(xt, y, x, par)
    kx, iK = m.kernel.eval(par, xt, x), m.kernel.eval_inv_dot(par, x)
    bar = (2 * N + 16) * EPS * np.abs(kx).dot(np.abs(iK))[:, :E]
    assert (np.abs(mean - kx.dot(iK)[:, :E]) <= bar).all()


@pytest.mark.parametrize('kind', ['gp', 'tp'])
def test_fit_then_predict(g16p, kind):
    """optimize_batch -> predict_batch on sin((x + 1)^-1) at the GH(15) points.  At training input i, exactly, mean_i - y_i =
    -jitter (iK y)_i and var_i = jitter - jitter^2 iK_ii (k_i = (K + jitter I) e_i - jitter e_i), times the TP scale - a
    jitter-sized variance that rounding may push below zero, so closeness to the identity is asserted, never var >= 0.  iK
    from eval_inv_dot; bar as test_golden_cases with the reference's own deviation from the identities at ITS fitted
    parameters (chain_* in the fixture) in place of ref_err."""
    m = model(kind, 1, ('gh', {'degree': 15}))
    x = m.points
    assert np.array_equal(x, g16p['chain_{}_x'.format(kind)])
    y = fcn(x)[0]                                               # (N,)
    Y = y[None, :, None]
    fits = m.optimize_batch(np.log(np.array([1.0, 0.5])), Y, x)
    assert fits['success'].all()
    par = np.exp(fits['x'])
    assert np.allclose(par[0], g16p['chain_{}_par'.format(kind)], rtol=1e-4)
    pred = m.predict_batch(x, Y, x, par=par)
    assert pred['status'][0] == 0
    jit = m.kernel.jitter
    iK = m.kernel.eval_inv_dot(par[0], x)
    scale = (NU - 2 + y.dot(iK).dot(y)) / (NU - 2 + m.num_pts) if kind == 'tp' else 1.0
    dev_m = np.abs((pred['mean'][0, :, 0] - y) + jit * iK.dot(y)).max() / np.abs(y).max()
    dev_v = np.abs(pred['var'][0] - scale * (jit - jit ** 2 * np.diag(iK))).max() / par[0, 0] ** 2
    bar_m = 8 * float(g16p['chain_{}_ref_ident_mean'.format(kind)]) + 64 * EPS
    bar_v = 8 * float(g16p['chain_{}_ref_ident_var'.format(kind)]) + 64 * EPS
    line = 'chain {} par {} identity deviation mean {:.3e} (bar {:.3e}) var {:.3e} (bar {:.3e})'.format(
        kind, par[0], dev_m, bar_m, dev_v, bar_v)
    print(line)
    if os.environ.get('SSMQ_PREDICT_PARITY_OUT'):
        with open(os.environ['SSMQ_PREDICT_PARITY_OUT'], 'a') as f:
            f.write(line + '\n')
    assert dev_m <= bar_m and dev_v <= bar_v, line
    # the single call is the batch's row
    mean, var = m.predict(x, y, x, par[0])
    assert np.array_equal(mean, pred['mean'][0, :, 0]) and np.array_equal(var, pred['var'][0])


@pytest.mark.parametrize('kind,N', [('gp', 12), ('tp', 12), ('gp', 80)])
def test_singular_kernel_matrix_is_flagged(kind, N):
    """Two equal training inputs and no jitter: the second pivot of the factorisation is exactly zero.  The row reports
    status 1 and NaN, its neighbours are finite and equal to their solo results, the single call raises LinAlgError."""
    rng = np.random.default_rng(5)
    D, B, M = 2, 3, 70
    m = model(kind, D)
    m.kernel.jitter = 0.0
    x = rng.uniform(-3, 3, (B, D, N))
    x[1, :, 1] = x[1, :, 0]
    xt = rng.standard_normal((D, M))
    y = rng.standard_normal((B, N, 1))
    par = np.array([1.0, 0.4, 0.4])
    r = m.predict_batch(xt, y, x, par=par)
    assert list(r['status']) == [0, 1, 0]
    assert np.isnan(r['mean'][1]).all() and np.isnan(r['var'][1]).all()
    for b in (0, 2):
        mean, var = m.predict(xt, y[b].T, x[b], par)
        assert np.isfinite(mean).all() and np.isfinite(var).all()
        assert np.array_equal(mean, r['mean'][b, :, 0]) and np.array_equal(var, r['var'][b])
    with pytest.raises(np.linalg.LinAlgError):
        m.predict(xt, y[1].T, x[1], par)


def test_bayes_sard_failures():
    """num_basis > N is refused before the device; a basis function that vanishes at every training input makes the first
    pivot of V' iK V exactly zero: status 2, NaN row, LinAlgError from the single call (the reference's cho_factor raises)."""
    bs6 = BayesSardModel(6, np.ones((1, 7)), 2, 'ut')
    with pytest.raises(NotImplementedError, match='num_basis <= N'):
        bs6.predict(np.zeros((6, 3)), np.zeros(13))
    rng = np.random.default_rng(6)
    D, N, B, M = 2, 10, 3, 5
    m = model('bs', D)
    x = rng.uniform(-2, 2, (B, D, N))
    x[2, 1, :] = 0.0
    mulind = np.array([[0, 0, 1], [1, 0, 0]])                  # x_2, 1, x_1
    xt, y = rng.standard_normal((D, M)), rng.standard_normal((B, N, 2))
    r = m.predict_batch(xt, y, x, par=np.array([1.0, 0.8, 0.8]), mulind=mulind)
    assert list(r['status']) == [0, 0, 2]
    assert np.isnan(r['mean'][2]).all() and np.isnan(r['var'][2]).all() and np.isfinite(r['mean'][:2]).all()
    with pytest.raises(np.linalg.LinAlgError):
        m.predict(xt, y[2].T, x[2], np.array([1.0, 0.8, 0.8]), mulind=mulind)


def test_range_edges():
    rng = np.random.default_rng(7)
    D, N, E, M = 16, 128, 16, 130
    m = model('gp', D)
    x, xt, y = rng.standard_normal((D, N)), rng.standard_normal((D, M)), rng.standard_normal((E, N))
    par = np.array([1.0] + [3.0] * D)
    mean, var = m.predict(xt, y, x, par)
    assert mean.shape == (M, E) and var.shape == (M,) and np.isfinite(mean).all() and np.isfinite(var).all()
    # Bayes-Sard with as many basis functions as points (one dimension, degrees 0 .. 7 on 8 points)
    bs = BayesSardModel(1, np.ones((1, 2)), 7, 'gh', {'degree': 8})
    assert bs.mulind.shape[1] == bs.num_pts == 8
    mean, var = bs.predict(rng.standard_normal((1, 9)), fcn(bs.points)[0])
    assert np.isfinite(mean).all() and np.isfinite(var).all()
    for bad in ((np.zeros((17, 5)), np.zeros((1, 5)), np.ones(18)), (np.zeros((1, 129)), np.zeros((1, 129)), np.ones(2)),
                (np.zeros((1, 5)), np.zeros((17, 5)), np.ones(2))):
        with pytest.raises(NotImplementedError, match='D <= 16'):
            model('gp', 1).predict(np.zeros((bad[0].shape[0], 3)), bad[1], bad[0], bad[2])


def test_c_entry_point_refuses_outside_the_range():
    lib = _lib.load()
    dp, ip = _lib.c_double_p, _lib.c_int32_p
    for D, N, E, NB in ((17, 5, 1, 0), (2, 129, 1, 0), (2, 5, 17, 0), (2, 5, 1, 6)):
        M = 3
        x, y, par, xt = np.zeros((D, N)), np.zeros((1, N, E)), np.ones((1, 1 + D)), np.zeros((D, M))
        mi = np.zeros((D, max(NB, 1)), dtype=np.int32)
        mean, var, st = np.full((1, M, E), -7.0), np.full((1, M), -7.0), np.full(1, -7, dtype=np.int32)
        rc = lib.ssmq_gp_predict_batch(D, N, E, 1, x.ctypes.data_as(dp), 0, y.ctypes.data_as(dp), 1e-8, 0.0, N,
                                       par.ctypes.data_as(dp), mi.ctypes.data_as(ip) if NB else None, NB, M,
                                       xt.ctypes.data_as(dp), 0, mean.ctypes.data_as(dp), var.ctypes.data_as(dp),
                                       st.ctypes.data_as(ip))
        assert rc == -3, (D, N, E, NB, rc)                      # SSMQ_E_UNSUPPORTED
        assert (mean == -7.0).all() and (var == -7.0).all() and st[0] == -7
