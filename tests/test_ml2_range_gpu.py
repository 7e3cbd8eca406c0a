"""
ML-II on the device (csrc/ssmq_ml2.hip k_ml2: ssmq_gp_nlml_batch / ssmq_gp_ml2_batch) over the whole range it
supports - D <= 16, N <= 128, E <= 16, GP and TP, x shared or per fit, any jitter - against the long-double form of the
oracle (oracle/ssmq_oracle.py: ml2_nlml), SciPy's BFGS on the float64 oracle, and the reference's values recorded in
tests/golden/g17_ml2_range.npz (make_golden_ml2_range.py).

Bars are k cond(K) eps relative: to max(1, |f|) for the value, and for the gradient to the norm of
1/2 sum_ij |W_ij| |dK_p,ij| (p = 0 .. P-1), the size of the terms its sum cancels (W, dK: oracle.ml2_terms).  k is about 4x
the worst ratio measured on the MI355X over every comparison of this file (KF, KG below); on well-conditioned rows
(cond <= 1e3) the g16 bars (1e-10 on the value, 1e-8 of the gradient's norm) hold as well.  Every comparison is recorded through tests/_cases.py::within.
"""
import ctypes
import os

import numpy as np
import pytest
from scipy.optimize import minimize

from oracle import ssmq_oracle as orc
from ssmtoybox_amd import _lib
from ssmtoybox_amd.bq.bqmod import GaussianProcessModel, StudentTProcessModel
from tests._cases import within

pytestmark = pytest.mark.gpu

G17 = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g17_ml2_range.npz')
G16 = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g16_ml2.npz')
EPS = np.finfo(float).eps
# the high-precision arithmetic: x87 long double where the host has it, else mpmath on the edge shapes only
HP = np.longdouble if np.finfo(np.longdouble).eps < 1e-17 else object
KF, KG = 40.0, 20.0             # measured worst ratios 9.5 (value, TP nu = 40) and 5.1 (gradient): about 4x
WELL = 1e3


@pytest.fixture(scope='module', autouse=True)
def device():
    import ssmtoybox_amd as amd
    if amd.device_count() < 1:
        pytest.fail('no device: these tests need a GPU')
    amd.set_device(0)


@pytest.fixture(scope='module')
def g17():
    return dict(np.load(G17))


@pytest.fixture(scope='module')
def g16():
    return dict(np.load(G16))


def model(D, nu):
    par = np.ones((1, D + 1))
    if nu == 0:
        return GaussianProcessModel(D, par, 'rbf', 'ut')
    return StudentTProcessModel(D, par, 'rbf', 'ut', nu=nu)


def upper_cond(lp, x, jit):
    """cond of what the reference factors: the upper triangle of K + jitter, mirrored."""
    N = x.shape[-1]
    out = []
    for b in range(lp.shape[0]):
        xb = x[b] if x.ndim == 3 else x
        A = orc.rbf_eval(np.exp(lp[b]), xb) + np.broadcast_to(jit, (N, N))
        out.append(np.linalg.cond(np.triu(A) + np.triu(A, 1).T))
    return np.array(out)


def check_hp(f, g, lp, y, x, jit, nu, what):
    """Device values f (B,), gradients g (B, P) against the wide oracle; returns the worst (value, gradient) ratios."""
    fh, Wh, dKh = orc.ml2_terms(lp, y, x, jit, nu, HP)
    gh = 0.5 * np.sum(Wh[:, None] * dKh, axis=(2, 3))
    sg = np.linalg.norm(np.array(0.5 * np.sum(np.abs(Wh[:, None] * dKh), axis=(2, 3)), dtype=float), axis=1)
    fh, gh = np.array(fh, dtype=float), np.array(gh, dtype=float)
    cond = upper_cond(lp, x, jit)
    worst = [0.0, 0.0]
    for b in range(lp.shape[0]):
        assert np.isfinite(f[b]) and np.isfinite(g[b]).all(), (what, b)
        ef = abs(f[b] - fh[b]) / max(1.0, abs(fh[b]))
        eg = np.linalg.norm(g[b] - gh[b]) / sg[b]
        rf, rg = ef / (cond[b] * EPS), eg / (cond[b] * EPS)
        worst = [max(worst[0], rf), max(worst[1], rg)]
        assert within(rf, KF, '{} row {} value / (cond eps)'.format(what, b)), (what, b, f[b], fh[b], cond[b])
        assert within(rg, KG, '{} row {} gradient / (cond eps)'.format(what, b)), (what, b, g[b], gh[b], cond[b])
        if cond[b] <= WELL:
            assert ef <= 1e-10 and np.linalg.norm(g[b] - gh[b]) <= 1e-8 * np.linalg.norm(gh[b]), (what, b, cond[b])
    return worst


# ---------------------------------------------------------------------------------------------------------------
# shape sweep
# ---------------------------------------------------------------------------------------------------------------
D_EDGES, N_EDGES, E_EDGES = (1, 2, 7, 15, 16), (1, 2, 3, 63, 64, 65, 66, 127, 128), (1, 2, 15, 16)


def sweep_shapes():
    shapes = {(16, 128, 16), (16, 64, 16), (16, 65, 16)}
    for i, N in enumerate(N_EDGES):                    # every N edge, with the D and E edges in turn
        shapes.add((D_EDGES[i % 5], N, E_EDGES[i % 4]))
        shapes.add((D_EDGES[(i + 2) % 5], N, E_EDGES[(i + 1) % 4]))
    for D in D_EDGES:
        for E in E_EDGES:
            shapes.add((D, (65, 64)[(D + E) % 2], E))
    rng = np.random.default_rng(170)
    for _ in range(40 if HP is not object else 0):
        shapes.add((int(rng.integers(1, 17)), int(rng.integers(1, 129)), int(rng.integers(1, 17))))
    return sorted(shapes)


SHAPES = sweep_shapes()


def sweep_case(D, N, E):
    """x, y and 4 rows: alpha = 1, 0.4 and 2.2 with mixed length-scales, and one ill-conditioned row (the longest
    length-scale of a ladder whose cond(K + 1e-8 I) stays below 1e9)."""
    rng = np.random.default_rng(1000 * D + 10 * N + E)
    x = rng.uniform(-2, 2, (D, N))
    w = rng.standard_normal((E, D)) / np.sqrt(D)
    y = np.sin(w.dot(x) + 0.3).T + 0.1 * rng.standard_normal((N, E))
    ell = 0.6 * np.sqrt(D) * (0.6 + 0.8 * rng.random(D))
    rows = [[1.0] + list(ell), [0.4] + list(ell[::-1]), [2.2] + list(0.5 * ell)]
    jit = 1e-8 * np.eye(N)
    ill = [1.0] + list(ell)
    for s in (1.5, 2, 3, 5, 8, 12, 20, 30, 50):
        r = [1.0] + list(s * ell)
        if upper_cond(np.log([r]), x, jit)[0] > 1e9:
            break
        ill = r
    rows.append(ill)
    return x, y, np.log(np.array(rows)), jit


@pytest.mark.parametrize('nu', [0.0, 2.5, 3.0, 40.0])
def test_shape_sweep_against_wide_oracle(nu):
    """Edges D in {1, 2, 7, 15, 16}, N in {1, 2, 3, 63, 64, 65, 66, 127, 128}, E in {1, 2, 15, 16}, the corner (16, 128,
    16) and its dense / packed neighbours (16, 64, 16), (16, 65, 16), and 40 seeded random shapes."""
    worst = [0.0, 0.0]
    for D, N, E in SHAPES:
        x, y, lp, jit = sweep_case(D, N, E)
        B = lp.shape[0]
        yb = np.broadcast_to(y, (B,) + y.shape)
        f, g = model(D, nu).neg_log_marginal_likelihood_batch(lp, yb, x, jit)
        w = check_hp(f, g, lp, yb, x, jit, nu, 'sweep nu={} D={} N={} E={}'.format(nu, D, N, E))
        worst = [max(worst[0], w[0]), max(worst[1], w[1])]
    print('sweep nu={}: worst value ratio {:.3g}, gradient ratio {:.3g} over {} shapes'.format(nu, worst[0], worst[1],
                                                                                              len(SHAPES)))


# ---------------------------------------------------------------------------------------------------------------
# x per fit, batch independence
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('D,N,E', [(4, 40, 3), (5, 100, 2)])
@pytest.mark.parametrize('nu', [0.0, 3.0])
def test_x_per_fit(D, N, E, nu):
    """x (B, D, N): row b is bit for bit a shared-x call on x[b], and matches the wide oracle (dense and packed route)."""
    rng = np.random.default_rng(D * N + E)
    B = 6
    x = rng.uniform(-2, 2, (B, D, N)) * (0.5 + np.arange(B))[:, None, None] / 3
    y = np.sin(x.sum(axis=1))[:, :, None] + 0.1 * rng.standard_normal((B, N, E))
    lp = np.log(np.column_stack([0.5 + rng.random(B), 0.8 + rng.random((B, D))]))
    jit = 1e-8 * np.eye(N)
    m = model(D, nu)
    f, g = m.neg_log_marginal_likelihood_batch(lp, y, x, jit)
    for b in range(B):
        f1, g1 = m.neg_log_marginal_likelihood_batch(lp[b:b + 1], y[b:b + 1], x[b], jit)
        assert f1[0] == f[b] and np.array_equal(g1[0], g[b]), b
    assert len({float(v) for v in f}) == B
    check_hp(f, g, lp, y, x, jit, nu, 'per-fit x nu={} D={} N={} E={}'.format(nu, D, N, E))
    # optimiser mode: a fit with its own x is the fit on that x alone
    r = m.optimize_batch(lp[:3], y[:3], x[:3])
    for b in range(3):
        s = m.optimize_batch(lp[b:b + 1], y[b:b + 1], x[b])
        for k in ('x', 'fun', 'jac', 'hess_inv', 'nit', 'status', 'nfev'):
            assert np.array_equal(s[k][0], r[k][b]), (b, k)


def test_batch_independence():
    """Row b is the same bits at B = 1, at B = 3000 and after a permutation of the rows (packed route, TP)."""
    rng = np.random.default_rng(33)
    D, N, E, B = 3, 66, 2, 3000
    x = rng.uniform(-2, 2, (D, N))
    y = np.sin(x.sum(axis=0))[None, :, None] + 0.1 * rng.standard_normal((B, N, E))
    lp = np.log(np.column_stack([0.5 + rng.random(B), 0.3 + rng.random((B, D))]))
    jit = 1e-8 * np.eye(N)
    m = model(D, 3.0)
    f, g = m.neg_log_marginal_likelihood_batch(lp, y, x, jit)
    assert np.isfinite(f).all()
    for b in (0, 1, 1499, 2999):
        f1, g1 = m.neg_log_marginal_likelihood_batch(lp[b:b + 1], y[b:b + 1], x, jit)
        assert f1[0] == f[b] and np.array_equal(g1[0], g[b]), b
    perm = rng.permutation(B)
    fp, gp = m.neg_log_marginal_likelihood_batch(lp[perm], y[perm], x, jit)
    assert np.array_equal(fp, f[perm]) and np.array_equal(gp, g[perm])


# ---------------------------------------------------------------------------------------------------------------
# failed rows
# ---------------------------------------------------------------------------------------------------------------
def raw_nlml(lp, y, x, jit, nu):
    """ssmq_gp_nlml_batch through ctypes: (return value, f, g, status)."""
    B, P = lp.shape
    D, N = x.shape[-2:]
    E = y.shape[2]
    lp, y, x, jit = (np.ascontiguousarray(a, dtype=np.float64) for a in (lp, y, x, np.broadcast_to(jit, (N, N))))
    f, g = np.empty(B), np.empty((B, P))
    st = np.zeros(B, dtype=np.int32)
    p = _lib.c_double_p
    rc = _lib.load().ssmq_gp_nlml_batch(D, N, E, B, x.ctypes.data_as(p), int(x.ndim == 3), y.ctypes.data_as(p),
                                        jit.ctypes.data_as(p), float(nu), lp.ctypes.data_as(p), f.ctypes.data_as(p),
                                        g.ctypes.data_as(p), st.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)))
    return rc, f, g, st


@pytest.mark.parametrize('D,N,E', [(1, 100, 1), (16, 128, 16)])
def test_failed_rows_are_isolated(D, N, E):
    """Rows whose K + jitter is not positive definite get NaNs and status 1 on the packed route and at the corner; the
    C entry point returns the first such row + 1; the other rows are what they are without them."""
    rng = np.random.default_rng(N)
    B = 7
    x = (np.linspace(-400, 400, N) * np.ones((D, 1))) / np.sqrt(D)     # far apart: K ~ alpha^2 I
    jit = -0.5 * np.eye(N)                                          # alpha = 1: ~ 0.5 I; alpha = 0.5: ~ -0.25 I
    lp = np.log(np.column_stack([np.ones(B), 0.5 + rng.random((B, D))]))
    bad = [2, 5]
    lp[bad, 0] = np.log(0.5)
    y = rng.standard_normal((B, N, E))
    for nu in (0.0, 3.0):
        rc, f, g, st = raw_nlml(lp, y, x, jit, nu)
        assert rc == bad[0] + 1, rc
        assert list(np.nonzero(st)[0]) == bad and np.isnan(f[bad]).all() and np.isnan(g[bad]).all()
        keep = [b for b in range(B) if b not in bad]
        rc2, f2, g2, st2 = raw_nlml(lp[keep], y[keep], x, jit, nu)
        assert rc2 == 0 and not st2.any() and np.isfinite(f2).all()
        assert np.array_equal(f[keep], f2) and np.array_equal(g[keep], g2)


# ---------------------------------------------------------------------------------------------------------------
# the reference's values at the range edges (g17), jitter forms
# ---------------------------------------------------------------------------------------------------------------
def g17_cases(g):
    return sorted({k[len('nlml_'):-len('_lp')] for k in g if k.startswith('nlml_') and k.endswith('_lp')})


G17_CASES = ['corner', 'd16n64', 'd16n65', 'jsym_n20', 'jsym_n70', 'jtri_n20', 'jtri_n70', 'jvec_n20', 'jvec_n70']


def test_g17_cases_are_covered(g17):
    assert g17_cases(g17) == G17_CASES


@pytest.mark.parametrize('case', G17_CASES)
def test_nlml_against_g17(g17, case):
    """The reference's values to the bars of test_ml2_gpu.py::test_nlml_against_reference: the corner D = 16, N = 128,
    E = 16 (GP; TP at nu = 2.5, 3, 40; at nu = 300 the reference's log(gamma) overflows to -inf, which the device
    reproduces with a finite gradient), N = 64 / 65 at D = 16, and the per-point 1-D, upper-triangular and dense symmetric
    jitters on both routes - the first two fail where the device reads the jitter's lower triangle."""
    x, y, lp, jit, cond = (g17['nlml_{}_{}'.format(case, k)] for k in ('x', 'y', 'lp', 'jit', 'cond'))
    names = sorted({k.split('_')[-2] for k in g17 if k.startswith('nlml_{}_'.format(case)) and k.endswith('_f')})
    B = lp.shape[0]
    for name in names:
        nu = float(g17['nlml_{}_{}_nu'.format(case, name)])
        f_ref, g_ref = g17['nlml_{}_{}_f'.format(case, name)], g17['nlml_{}_{}_g'.format(case, name)]
        f, g = model(x.shape[0], nu).neg_log_marginal_likelihood_batch(lp, np.broadcast_to(y, (B,) + y.shape), x, jit)
        for k in range(B):
            if np.isinf(f_ref[k]):
                assert f[k] == f_ref[k], (case, name, k, f[k])
            else:
                fbar = max(1e-10, 20 * cond[k] * EPS)
                assert within(abs(f[k] - f_ref[k]) / max(1.0, abs(f_ref[k])), fbar, 'g17 {} {} row {} value'.format(
                    case, name, k)), (case, name, k, f[k], f_ref[k], cond[k])
            assert np.isfinite(g[k]).all(), (case, name, k)
            gbar = max(1e-8, 20 * cond[k] * EPS)
            assert within(np.linalg.norm(g[k] - g_ref[k]) / np.linalg.norm(g_ref[k]), gbar, 'g17 {} {} row {} gradient'.format(
                case, name, k)), (case, name, k, g[k], g_ref[k], cond[k])


@pytest.mark.parametrize('form', ['scalar', 'identity', 'dense_symmetric', 'vector', 'triangle'])
def test_jitter_forms_against_wide_oracle(form):
    """Scalar (added to every entry, as K + jitter broadcasts it), identity, dense symmetric, per-point 1-D and
    upper-triangular jitters against the wide oracle, which reads K + jitter through its upper triangle."""
    for D, N, E in ((3, 30, 2), (3, 90, 2)):
        rng = np.random.default_rng(N)
        x = rng.uniform(-2, 2, (D, N))
        y = np.sin(x.sum(axis=0))[:, None] + 0.1 * rng.standard_normal((N, E))
        i = np.arange(N)
        jit = {'scalar': 1e-6, 'identity': 1e-6 * np.eye(N), 'dense_symmetric': 1e-5 * 0.5 ** np.abs(i[:, None] - i),
               'vector': 1e-6 * (2.0 - i / N), 'triangle': 1e-5 * np.triu(0.5 ** np.abs(i[:, None] - i))}[form]
        lp = np.log(np.array([[1.0, 0.8, 0.8, 0.8], [0.4, 0.5, 0.9, 1.3], [2.2, 1.1, 0.7, 0.6]]))
        yb = np.broadcast_to(y, (3,) + y.shape)
        for nu in (0.0, 3.0):
            f, g = model(D, nu).neg_log_marginal_likelihood_batch(lp, yb, x, jit)
            check_hp(f, g, lp, yb, x, jit, nu, 'jitter {} nu={} N={}'.format(form, nu, N))


# ---------------------------------------------------------------------------------------------------------------
# the optimiser
# ---------------------------------------------------------------------------------------------------------------
# hess_inv against SciPy-on-oracle, of its largest entry: measured up to 8.2e-6 on the g16 / g17 runs (tp_ut5; the others
# <= 1e-8), where NumPy's BLAS and the device round the updates differently (test_ml2_host.py); at the corner (P = 17)
# measured up to 5.0e-7
HBAR, HBAR_CORNER = 5e-5, 2e-6


def scipy_on_oracle(x0, y, x, nu):
    jit = 1e-8 * np.eye(x.shape[1])
    return minimize(lambda lp: orc.ml2_nlml(lp, y, x, jit, nu), x0, method='BFGS', jac=True)


def check_fit(r, b, ref, x, y, nu, what, fbar=1e-10, hbar=None):
    assert r['status'][b] == ref.status, (what, r['status'][b], ref.message)
    assert abs(r['nit'][b] - ref.nit) <= 1, (what, r['nit'][b], ref.nit)
    assert np.abs(r['x'][b] - ref.x).max() <= 1e-6 * max(1.0, np.abs(ref.x).max()), (what, r['x'][b], ref.x)
    assert abs(r['fun'][b] - ref.fun) <= fbar * max(1.0, abs(ref.fun)), (what, r['fun'][b], ref.fun)
    eh = np.abs(r['hess_inv'][b] - ref.hess_inv).max() / np.abs(ref.hess_inv).max()
    assert within(eh, HBAR if hbar is None else hbar, '{} hess_inv'.format(what)), (what, eh)
    if r['status'][b] == 0:
        gh = orc.ml2_nlml(r['x'][b], y, x, 1e-8 * np.eye(x.shape[1]), nu, dtype=HP)[1]
        assert np.abs(np.array(gh, dtype=float)).max() <= 1e-5 * (1 + 1e-6), (what, gh)


def test_optimize_corner_against_scipy_on_oracle():
    """P = 17 (the full size of the kernel's gradient accumulator and BFGS state) at D = 16, N = 128, E = 16, on rough
    data where K stays well-conditioned: status, nit +- 1, x, fun and hess_inv as SciPy's BFGS on the float64 oracle."""
    rng = np.random.default_rng(128)
    D, N, E = 16, 128, 16
    x = rng.uniform(-2, 2, (D, N))
    ph = rng.uniform(0, 2 * np.pi, (E, D))
    # additive in every input, so that no length-scale runs off to a flat direction (all fitted log ell in 1.1 .. 1.8)
    y = np.stack([np.sin(1.2 * x + ph[e][:, None]).sum(axis=0) for e in range(E)], axis=1) + 0.3 * rng.standard_normal((N, E))
    x0 = np.log(np.array([[2.0] + [1.5] * D, [3.0] + [2.5] * D]))
    m = model(D, 0.0)
    r = m.optimize_batch(x0, np.broadcast_to(y, (2, N, E)), x)
    for b in range(2):
        check_fit(r, b, scipy_on_oracle(x0[b], y, x, 0.0), x, y, 0.0, 'corner fit {}'.format(b), hbar=HBAR_CORNER)


def test_optimize_against_scipy_on_oracle(g16, g17):
    """The reference's optimiser runs (g16, and g17's D = 8) with hess_inv compared against SciPy-on-oracle, and the
    g17 run against the reference's own result."""
    runs = [(g16, n) for n in sorted({k[4:-3] for k in g16 if k.startswith('opt_') and k.endswith('_x0')})]
    runs.append((g17, 'd8'))
    assert len(runs) == 8
    for g, name in runs:
        nu = 3.0 if name.startswith('tp') else 0.0
        x, y, x0 = g['opt_{}_x_obs'.format(name)], g['opt_{}_y'.format(name)], g['opt_{}_x0'.format(name)]
        m = model(x.shape[0], nu)
        r = m.optimize_batch(x0[None], y[None], x)
        check_fit(r, 0, scipy_on_oracle(x0, y, x, nu), x, y, nu, 'opt {}'.format(name))
    # g17's run against the reference itself
    r = model(8, 0.0).optimize(g17['opt_d8_x0'], g17['opt_d8_y'], g17['opt_d8_x_obs'])
    assert r.status == int(g17['opt_d8_status']) and abs(r.nit - int(g17['opt_d8_nit'])) <= 1
    xr = g17['opt_d8_x']
    assert np.abs(r.x - xr).max() <= 1e-6 * max(1.0, np.abs(xr).max())
    assert abs(r.fun - float(g17['opt_d8_fun'])) <= 1e-10 * max(1.0, abs(float(g17['opt_d8_fun'])))
    eh = np.abs(r.hess_inv - g17['opt_d8_hess_inv']).max() / np.abs(g17['opt_d8_hess_inv']).max()
    assert within(eh, HBAR, 'opt d8 hess_inv against the reference'), eh
