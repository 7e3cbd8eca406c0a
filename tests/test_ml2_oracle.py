"""
The ML-II oracle (oracle/ssmq_oracle.py: ml2_nlml) against the reference: its float64 form against every NLML case of
g16_ml2.npz and g17_ml2_range.npz, SciPy's BFGS on it against the reference's Model.optimize runs, its long-double form
against the float64 one and against central differences of itself, and checks that its bars catch wrong arithmetic.  The
device tests (test_ml2_range_gpu.py) measure the kernel against the long-double form.
"""
import os

import numpy as np
import pytest
from scipy.optimize import minimize

from oracle import ssmq_oracle as orc

GDIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
EPS = np.finfo(float).eps
# the high-precision arithmetic: x87 long double where the host has it (eps 1.1e-19), else mpmath on fewer cases
HP = np.longdouble if np.finfo(np.longdouble).eps < 1e-17 else object


@pytest.fixture(scope='module')
def g16():
    return dict(np.load(os.path.join(GDIR, 'g16_ml2.npz')))


@pytest.fixture(scope='module')
def g17():
    return dict(np.load(os.path.join(GDIR, 'g17_ml2_range.npz')))


def nlml_cases(g):
    return sorted({k[len('nlml_'):-len('_lp')] for k in g if k.startswith('nlml_') and k.endswith('_lp')})


def models(g, case):
    """(name, nu) of the models recorded for a case: g16 has gp / tp (nu = 3), g17 names its nu."""
    names = sorted({k[len('nlml_{}_'.format(case)):-len('_f')] for k in g
                    if k.startswith('nlml_{}_'.format(case)) and k.endswith('_f')})
    return [(n, 0.0 if n == 'gp' else float(g.get('nlml_{}_{}_nu'.format(case, n), 3.0))) for n in names]


def jitter(g, case):
    key = 'nlml_{}_jit'.format(case)
    return g[key] if key in g else 1e-8 * np.eye(g['nlml_{}_x'.format(case)].shape[1])


def check_reference(g, case):
    x, y, lp, cond = (g['nlml_{}_{}'.format(case, k)] for k in ('x', 'y', 'lp', 'cond'))
    B = lp.shape[0]
    n = 0
    for name, nu in models(g, case):
        f_ref, g_ref = g['nlml_{}_{}_f'.format(case, name)], g['nlml_{}_{}_g'.format(case, name)]
        with np.errstate(over='ignore', divide='ignore'):
            f, gr = orc.ml2_nlml(lp, np.broadcast_to(y, (B,) + y.shape), x, jitter(g, case), nu)
        for k in range(B):
            # the bars of test_ml2_gpu.py::test_nlml_against_reference
            if np.isinf(f_ref[k]):
                assert f[k] == f_ref[k], (case, name, k, f[k])
            else:
                fbar = max(1e-10, 20 * cond[k] * EPS)
                assert abs(f[k] - f_ref[k]) <= fbar * max(1.0, abs(f_ref[k])), (case, name, k, f[k], f_ref[k], cond[k])
            gbar = max(1e-8, 20 * cond[k] * EPS)
            assert np.linalg.norm(gr[k] - g_ref[k]) <= gbar * np.linalg.norm(g_ref[k]), (case, name, k, cond[k])
            n += 1
    return n


def test_float64_oracle_against_g16(g16):
    assert sum(check_reference(g16, c) for c in nlml_cases(g16)) == 12 * 2 * 6


def test_float64_oracle_against_g17(g17):
    """The range fixture: D = 16 / N = 128 / E = 16, N = 64 / 65 at D = 16, TP at nu = 2.5, 3, 40 and 300 (the reference's
    -inf), and the jitters that are not symmetric - a per-point nugget and a triangle, read through the upper triangle as
    cho_factor reads them."""
    cases = nlml_cases(g17)
    assert len(cases) == 9
    assert sum(check_reference(g17, c) for c in cases) == 4 * (5 + 2 * 8)


def test_jitter_is_read_through_the_upper_triangle(g17):
    """Reading the jitter's lower triangle instead (jitter.T) misses the reference by far more than the bar."""
    for case in ('jvec_n20', 'jtri_n70'):
        x, y, lp = (g17['nlml_{}_{}'.format(case, k)] for k in ('x', 'y', 'lp'))
        jit = np.broadcast_to(jitter(g17, case), (x.shape[1],) * 2)
        f_ref = g17['nlml_{}_gp_f'.format(case)]
        f, g = orc.ml2_nlml(lp[:3], np.broadcast_to(y, (3,) + y.shape), x, jit.T)
        assert moved(f_ref[:3], g17['nlml_{}_gp_g'.format(case)][:3], f, g).all()


def moved(f, g, fm, gm, factor=100):
    """Per row: the value moved by more than factor x 1e-10 relative, or the gradient by more than factor x 1e-8 of its
    norm (the g16 bars, which the range test's bars never exceed on well-conditioned rows)."""
    return ((np.abs(fm - f) > factor * 1e-10 * np.abs(f))
            | (np.linalg.norm(gm - g, axis=1) > factor * 1e-8 * np.linalg.norm(g, axis=1)))


def rows_for(g, case, nrows=None):
    x, y, lp = (g['nlml_{}_{}'.format(case, k)] for k in ('x', 'y', 'lp'))
    lp = lp if nrows is None else lp[:nrows]
    return x, np.broadcast_to(y, (lp.shape[0],) + y.shape), lp


HP_CASES = [('g16', 'gh15_e3'), ('g16', 'ut5_e3'), ('g16', 'sc65_e1'), ('g17', 'd16n64'), ('g17', 'jtri_n20')]
if HP is object:        # mpmath is slow: the small cases only
    HP_CASES = HP_CASES[:2]


@pytest.mark.parametrize('src,case', HP_CASES)
def test_high_precision_against_float64(g16, g17, src, case):
    """The wide form agrees with the float64 form within 64 cond(K) eps, relative (measured: at most 3.8 cond eps on the
    value, 13 on the gradient, at cond 1.3 where its terms cancel); it is the same formula, not a different one."""
    g = g16 if src == 'g16' else g17
    x, y, lp = rows_for(g, case)
    cond = g['nlml_{}_cond'.format(case)]
    for _, nu in models(g, case):
        f64, g64 = orc.ml2_nlml(lp, y, x, jitter(g, case), nu)
        fhp, ghp = orc.ml2_nlml(lp, y, x, jitter(g, case), nu, dtype=HP)
        for k in range(lp.shape[0]):
            assert abs(f64[k] - float(fhp[k])) <= 64 * cond[k] * EPS * max(1.0, abs(f64[k])), (case, nu, k)
            gk = np.array(ghp[k], dtype=float)
            assert np.linalg.norm(g64[k] - gk) <= 64 * cond[k] * EPS * np.linalg.norm(gk), (case, nu, k)


@pytest.mark.parametrize('src,case', HP_CASES[:3] + [('g17', 'jvec_n20')])
def test_gradient_against_central_differences(g16, g17, src, case):
    """Central differences of the wide value (h = 1e-5 on the log-parameters): entry 0 times alpha is the derivative
    along log alpha (der_par's quirk), the others are log-derivatives.  Measured: <= 2e-10 of the gradient's norm."""
    g = g16 if src == 'g16' else g17
    x, y, lp = rows_for(g, case, 3)
    h = 1e-5
    for _, nu in models(g, case):
        f, gr = orc.ml2_nlml(lp, y, x, jitter(g, case), nu, dtype=HP)
        for k in range(lp.shape[0]):
            P = lp.shape[1]
            up = np.repeat(lp[k:k + 1], P, axis=0) + h * np.eye(P)
            dn = np.repeat(lp[k:k + 1], P, axis=0) - h * np.eye(P)
            yy = np.broadcast_to(y[0], (P,) + y.shape[1:])
            fd = (orc.ml2_nlml(up, yy, x, jitter(g, case), nu, dtype=HP)[0]
                  - orc.ml2_nlml(dn, yy, x, jitter(g, case), nu, dtype=HP)[0]) / (2 * h)
            fd = np.array(fd, dtype=float)
            an = np.array(gr[k], dtype=float)
            an[0] *= np.exp(lp[k, 0])
            assert np.linalg.norm(an - fd) <= 1e-8 * np.linalg.norm(fd), (case, nu, k, an, fd)


def opt_cases(g):
    return sorted({k[len('opt_'):-len('_x0')] for k in g if k.startswith('opt_') and k.endswith('_x0')})


def test_scipy_on_oracle_reproduces_reference_optimize(g16, g17):
    """minimize(BFGS, jac=True) on the float64 oracle follows the reference's Model.optimize: status, nit (+-1), x and
    fun to the bars of test_ml2_gpu.py::test_optimize_against_reference."""
    runs = [(g16, n) for n in opt_cases(g16)] + [(g17, n) for n in opt_cases(g17)]
    assert len(runs) == 8
    for g, name in runs:
        x_obs, y, x0 = g['opt_{}_x_obs'.format(name)], g['opt_{}_y'.format(name)], g['opt_{}_x0'.format(name)]
        nu = 3.0 if name.startswith('tp') else 0.0
        jit = 1e-8 * np.eye(x_obs.shape[1])
        res = minimize(lambda lp: orc.ml2_nlml(lp, y, x_obs, jit, nu), x0, method='BFGS', jac=True)
        assert res.status == int(g['opt_{}_status'.format(name)]), (name, res.message)
        assert abs(res.nit - int(g['opt_{}_nit'.format(name)])) <= 1, (name, res.nit)
        xr = g['opt_{}_x'.format(name)]
        assert np.abs(res.x - xr).max() <= 1e-6 * max(1.0, np.abs(xr).max()), (name, res.x, xr)
        fr = float(g['opt_{}_fun'.format(name)])
        assert abs(res.fun - fr) <= 1e-10 * max(1.0, abs(fr)), (name, res.fun, fr)


def test_tp_constant_overflows_as_the_reference():
    with np.errstate(over='ignore', divide='ignore'):
        assert orc.ml2_tp_const(300.0, 128) == -np.inf
        assert np.isfinite(orc.ml2_tp_const(40.0, 128)) and np.isfinite(orc.ml2_tp_const(300.0, 20))
    assert abs(float(orc.ml2_tp_const(40.0, 128, HP)) - orc.ml2_tp_const(40.0, 128)) <= 1e-13 * 300


def test_non_positive_definite_row_is_nan():
    x = np.linspace(-20, 20, 12)[None, :]
    lp = np.log([[1.0, 1.0], [0.5, 1.0]])
    y = np.ones((2, 12, 1))
    for dt in (np.float64, np.longdouble):
        f, g = orc.ml2_nlml(lp, y, x, -0.5 * np.eye(12), dtype=dt)
        assert np.isfinite(f[0]) and np.isfinite(g[0]).all() and np.isnan(f[1]) and np.isnan(g[1]).all()


def test_mpmath_form_agrees_with_long_double():
    """The fallback for hosts without a wide long double (object dtype, mpmath) is the same computation."""
    rng = np.random.default_rng(3)
    x = rng.uniform(-1, 1, (2, 6))
    y = rng.standard_normal((2, 6, 2))
    lp = np.log([[1.3, 0.7, 1.1], [0.6, 1.5, 0.9]])
    for nu in (0.0, 4.0):
        f1, g1 = orc.ml2_nlml(lp, y, x, 1e-8 * np.eye(6), nu, dtype=np.longdouble)
        f2, g2 = orc.ml2_nlml(lp, y, x, 1e-8 * np.eye(6), nu, dtype=object)
        assert np.abs(np.array(f2, dtype=float) - f1.astype(float)).max() <= 1e-15 * np.abs(f1).max().astype(float)
        assert np.abs(np.array(g2, dtype=float) - g1.astype(float)).max() <= 1e-14 * np.abs(g1).max().astype(float)


def test_bars_catch_wrong_arithmetic(g16, g17):
    """Three mistakes a kernel could make each move the value or the gradient by far more (100 x) than the bars the
    device is held to on these well-conditioned rows (`moved`): a jitter read
    from the wrong triangle, row 0's x used for every row of a per-fit batch, and the factor 2 of the off-diagonal terms
    of the gradient's sum over the lower triangle dropped."""
    # wrong triangle (the per-point nugget: K + v[None, :] read through its lower triangle is K + v[min(i, j)])
    x, y, lp = rows_for(g17, 'jvec_n70', 3)
    jit = np.broadcast_to(jitter(g17, 'jvec_n70'), (70, 70))
    f, g = orc.ml2_nlml(lp, y, x, jit)
    fm, gm = orc.ml2_nlml(lp, y, x, np.ascontiguousarray(jit.T))
    assert moved(f, g, fm, gm).all()
    # x of row 0 for every row
    rng = np.random.default_rng(11)
    xs = rng.uniform(-2, 2, (4, 5, 30))
    ys = rng.standard_normal((4, 30, 2))
    lp4 = np.log(np.column_stack([np.full(4, 1.2), np.full((4, 5), 1.5)]))
    f, g = orc.ml2_nlml(lp4, ys, xs, 1e-8 * np.eye(30))
    fm, gm = orc.ml2_nlml(lp4, ys, xs[0], 1e-8 * np.eye(30))
    assert moved(f[1:], g[1:], fm[1:], gm[1:]).all()
    # the off-diagonal factor 2 dropped: 1/2 sum over i >= j of W dK instead of the full sum
    for src, case in (('g16', 'ut5_e3'), ('g17', 'd16n65')):
        g_ = g16 if src == 'g16' else g17
        x, y, lp = rows_for(g_, case, 3)
        fv, W, dK = orc.ml2_terms(lp, y, x, jitter(g_, case))
        gfull = 0.5 * np.sum(W[:, None] * dK, axis=(2, 3))
        gm = 0.5 * np.sum(np.tril(W)[:, None] * dK, axis=(2, 3))
        assert moved(fv, gfull, fv, gm).all()
