"""
Golden vectors for ML-II over the whole range the device supports (D <= 16, N <= 128, E <= 16): the reference's
GaussianProcessModel / StudentTProcessModel.neg_log_marginal_likelihood (bq/bqmod.py:537-596, 1191-1245) and
Model.optimize (bq/bqmod.py:250-285) run here.  A sibling of make_golden_ml2.py (g16_ml2.npz), which it leaves alone.
Reuses the import shims of make_golden.py (importing that module installs them and loads the reference).

Run:  PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python tests/golden/make_golden_ml2_range.py   -> tests/golden/g17_ml2_range.npz

NLML cases `nlml_<case>_*`: x (D, N), y (N, E), lp (K, P) log-parameters, jit (the jitter exactly as passed to the
reference: a scalar, an (N,) per-point nugget that K + jit broadcasts to jit[i][j] = v[j], or (N, N)), cond (K,) the
2-norm condition number of the matrix the reference factors (the upper triangle of K + jitter, symmetrised), and per model
`<model>_nu`, `<model>_f` (K,), `<model>_g` (K, P).  Models: gp (nu = 0) and tp<nu> (nu = 3, 2.5, 40, 300; '.' as 'p').
  corner    D = 16, N = 128, E = 16 (the packed route at its largest LDS footprint, P = 17): gp, tp3, tp2p5, tp40 and
            tp300, where the reference's log(gamma((nu + N) / 2)) overflows and the value is -inf
  d16n64 / d16n65   D = 16, E = 4 on either side of the dense / packed switch
  jvec_n20 / jvec_n70, jtri_n20 / jtri_n70, jsym_n20 / jsym_n70   D = 3, E = 2: a per-point 1-D nugget, an upper-triangular
            jitter and a dense symmetric one, on the dense (N = 20) and the packed (N = 70) route
Rows: alpha in {1, 0.4, 2.2}, mixed length-scales, and one ill-conditioned row (long length-scales) per case.
Optimiser case `opt_d8_*` (x_obs, y, x0, x, fun, nit, status, jac, hess_inv): Model.optimize with its defaults (BFGS,
jac=True, jitter 1e-8 I) at D = 8, N = 40, E = 2 on rough data, where K stays well-conditioned along the path.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.golden import make_golden as mg  # noqa: E402,F401  (installs the shims, imports the reference)
from ssmtoybox.bq.bqmod import GaussianProcessModel, StudentTProcessModel  # noqa: E402


def model(D, nu):
    par = np.ones((1, D + 1))
    if nu == 0:
        return GaussianProcessModel(D, par, 'rbf', 'ut')
    return StudentTProcessModel(D, par, 'rbf', 'ut', nu=nu)


def model_name(nu):
    return 'gp' if nu == 0 else 'tp' + ('%g' % nu).replace('.', 'p')


def rows(D, ell, ill):
    """alpha != 1, mixed length-scales across the dimensions, one ill-conditioned row."""
    mix = ell * (0.6 + 0.8 * np.arange(D) / max(D - 1, 1))
    r = [[1.0] + [ell] * D, [0.4] + list(mix), [2.2] + list(mix[::-1]), [1.0] + [ill] * D]
    return np.log(np.array(r))


def data(x, E, rng):
    D, N = x.shape
    w = rng.standard_normal((E, D)) / np.sqrt(D)
    return np.sin(w.dot(x) + 0.3).T + 0.1 * rng.standard_normal((N, E))


def upper_matrix(K, jit):
    """What cho_factor(K + jit) factors: the upper triangle of K + jit, mirrored."""
    A = K + jit
    return np.triu(A) + np.triu(A, 1).T


def add_case(out, case, x, y, lp, jit, nus):
    D, N = x.shape
    out['nlml_{}_x'.format(case)] = x
    out['nlml_{}_y'.format(case)] = y
    out['nlml_{}_lp'.format(case)] = lp
    out['nlml_{}_jit'.format(case)] = np.asarray(jit, dtype=np.float64)
    kern = model(D, 0).kernel
    out['nlml_{}_cond'.format(case)] = np.array([np.linalg.cond(upper_matrix(kern.eval(np.exp(r), x), jit)) for r in lp])
    for nu in nus:
        m = model(D, nu)
        fs, gs = [], []
        for r in lp:
            f, g = m.neg_log_marginal_likelihood(r, y, x, jit)
            fs.append(f)
            gs.append(g)
        name = model_name(nu)
        out['nlml_{}_{}_nu'.format(case, name)] = np.float64(nu)
        out['nlml_{}_{}_f'.format(case, name)] = np.array(fs)
        out['nlml_{}_{}_g'.format(case, name)] = np.array(gs)


def main():
    rng = np.random.default_rng(17)
    out = {}
    with np.errstate(over='ignore', divide='ignore'):      # tp300: gamma(214) overflows in the reference, as recorded
        x = rng.uniform(-2, 2, (16, 128))
        add_case(out, 'corner', x, data(x, 16, rng), rows(16, 2.5, 30.0), 1e-8 * np.eye(128), (0, 3.0, 2.5, 40.0, 300.0))
    for N in (64, 65):
        x = rng.uniform(-2, 2, (16, N))
        add_case(out, 'd16n{}'.format(N), x, data(x, 4, rng), rows(16, 2.5, 30.0), 1e-8 * np.eye(N), (0, 3.0))
    for N in (20, 70):
        x = rng.uniform(-2, 2, (3, N))
        y = data(x, 2, rng)
        lp = rows(3, 0.8, 4.0)
        i = np.arange(N)
        jits = {
            'jvec': 1e-6 * (2.0 - np.arange(N) / N),     # per-point nugget K + v[None, :]; read upper: v[max(i, j)], PD
            'jtri': 1e-5 * np.triu(0.5 ** np.abs(i[:, None] - i[None, :])) + 1e-8 * np.eye(N),   # upper triangle only
            'jsym': 1e-5 * 0.5 ** np.abs(i[:, None] - i[None, :]) + 1e-8 * np.eye(N),           # dense symmetric
        }
        for name, jit in jits.items():
            add_case(out, '{}_n{}'.format(name, N), x, y, lp, jit, (0, 3.0))

    # one optimiser run at D = 8 (P = 9) on rough data: the fitted length-scales stay short and K well-conditioned
    D, N = 8, 40
    xo = rng.uniform(-2, 2, (D, N))
    yo = np.column_stack([np.sin(1.5 * xo.sum(axis=0)), np.cos(2.0 * xo[0] - xo[1])]) + 0.3 * rng.standard_normal((N, 2))
    x0 = np.log(np.array([1.0] + [1.5] * D))
    res = model(D, 0).optimize(x0, yo, xo, method='BFGS')
    for k, v in (('x_obs', xo), ('y', yo), ('x0', x0), ('x', res.x), ('fun', res.fun), ('nit', res.nit),
                 ('status', res.status), ('jac', res.jac), ('hess_inv', res.hess_inv)):
        out['opt_d8_{}'.format(k)] = np.asarray(v)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'g17_ml2_range.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes,', len(out), 'arrays;', 'opt_d8:', res.status, res.nit, res.x)


if __name__ == '__main__':
    main()
