"""
Golden vectors for type-II maximum likelihood (ML-II) of the RBF kernel's parameters: the reference's
GaussianProcessModel / StudentTProcessModel.neg_log_marginal_likelihood (bq/bqmod.py:537-596, 1191-1245, with
RBFGauss.der_par bq/bqkern.py:426-436) and Model.optimize (bq/bqmod.py:250-285, scipy.optimize.minimize BFGS) run here.
Reuses the import shims of make_golden.py (importing that module installs them and loads the reference).

Run:  PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python tests/golden/make_golden_ml2.py      -> tests/golden/g16_ml2.npz

NLML cases `nlml_<case>_<model>_<k>` (model gp / tp, k = parameter row): x (D, N), y (N, E), lp (K, P) log-parameters,
f (K,), g (K, P), and `cond` (K,) the 2-norm condition number of K + jitter.  Cases: GH(15) and GH(10) at D = 1, UT at
D = 5, 100 scattered points at D = 1, 64 and 65 scattered points at D = 2; E = 1 and E = 3; alpha in {1, 0.3, 2.5} and one
ill-conditioned length-scale per case.
Optimiser cases `opt_<name>_*`: x0 (P,), x (P,), fun, nit, status - the reference tests' starts taken as 1-D arrays
(tests/test_bqmod.py:167, 581) and others, among them alpha != 1 at the start.  (No 100-point run: on these data the
reference's own BFGS path ends in precision loss or a failed factorisation depending on the start - cond(K) ~ 1e8 - 1e9
along the way - so its status and iteration count are not reproducible.)  The TP models use nu = 3 (StudentTProcessModel's
default nu = 3.0 if nu < 2 else nu, with the nu the reference's tests give).
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.golden import make_golden as mg  # noqa: E402,F401  (installs the shims, imports the reference)
from ssmtoybox.bq.bqmod import GaussianProcessModel, StudentTProcessModel  # noqa: E402

NU = 3.0
# per case: the length-scale of the regular rows and the long one of the ill-conditioned row
ELL = {'gh15': (0.5, 3.0), 'gh10': (0.5, 3.0), 'ut5': (3.0, 30.0), 'sc100': (0.2, 0.6), 'sc64': (0.7, 2.5),
       'sc65': (0.7, 2.5)}


def fcn(x):            # the reference tests' integrand (tests/test_bqmod.py:15)
    return np.sin((x + 1) ** -1)


def models(D, pts, par):
    gp = GaussianProcessModel(D, par, 'rbf', pts[0], pts[1])
    tp = StudentTProcessModel(D, par, 'rbf', pts[0], pts[1], nu=NU)
    return gp, tp


def data(x, E, rng):
    base = fcn(x).sum(axis=0)                       # (N,)
    cols = [base] + [np.cos(0.7 * (e + 1) * x).sum(axis=0) + 0.1 * rng.standard_normal(x.shape[1]) for e in range(E - 1)]
    return np.stack(cols, axis=1)


def main():
    rng = np.random.default_rng(16)
    out = {}
    xs = {
        'gh15': (1, ('gh', {'degree': 15}), None),
        'gh10': (1, ('gh', {'degree': 10}), None),
        'ut5': (5, ('ut', {'alpha': 1.0}), None),
        'sc100': (1, ('gh', {'degree': 5}), np.sort(rng.uniform(-4, 4, (1, 100)), axis=1)),
        'sc64': (2, ('gh', {'degree': 5}), rng.uniform(-3, 3, (2, 64))),
        'sc65': (2, ('gh', {'degree': 5}), rng.uniform(-3, 3, (2, 65))),
    }
    for case, (D, pts, xdat) in xs.items():
        gp, tp = models(D, pts, np.ones((1, D + 1)))
        x = gp.points if xdat is None else xdat
        N = x.shape[1]
        jit = 1e-8 * np.eye(N)
        ell, ill = ELL[case]
        rows = [[a] + [ell] * D for a in (1.0, 0.3, 2.5)]
        rows.append([1.0] + [ell * 0.7] * D)
        rows.append([1.3] + [ell * (0.8 + 0.1 * d) for d in range(D)])
        rows.append([1.0] + [ill] * D)          # ill-conditioned: a long length-scale
        lp = np.log(np.array(rows))
        for E in (1, 3):
            y = data(x, E, rng)
            out['nlml_{}_e{}_x'.format(case, E)] = x
            out['nlml_{}_e{}_y'.format(case, E)] = y
            out['nlml_{}_e{}_lp'.format(case, E)] = lp
            conds = []
            for name, m in (('gp', gp), ('tp', tp)):
                fs, gs = [], []
                for r in lp:
                    f, g = m.neg_log_marginal_likelihood(r, y, x, jit)
                    fs.append(f)
                    gs.append(g)
                out['nlml_{}_e{}_{}_f'.format(case, E, name)] = np.array(fs)
                out['nlml_{}_e{}_{}_g'.format(case, E, name)] = np.array(gs)
            for r in lp:
                conds.append(np.linalg.cond(gp.kernel.eval(np.exp(r), x) + jit))
            out['nlml_{}_e{}_cond'.format(case, E)] = np.array(conds)

    # optimiser runs (Model.optimize with its defaults: BFGS, jac=True, jitter 1e-8 I)
    opt = [
        ('gp_gh15', 'gp', 1, ('gh', {'degree': 15}), [1.0, 0.5], 1),      # tests/test_bqmod.py:160-190 (start as 1-D)
        ('tp_gh10', 'tp', 1, ('gh', {'degree': 10}), [1.0, 0.5], 1),      # tests/test_bqmod.py:562-590
        ('gp_gh15_a', 'gp', 1, ('gh', {'degree': 15}), [0.4, 0.8], 1),
        ('tp_gh10_a', 'tp', 1, ('gh', {'degree': 10}), [2.0, 0.4], 1),
        ('gp_ut5', 'gp', 5, ('ut', {'alpha': 1.0}), [1.0] + [3.0] * 5, 1),
        ('gp_ut5_e3', 'gp', 5, ('ut', {'alpha': 1.0}), [0.5] + [2.0] * 5, 3),
        ('tp_ut5', 'tp', 5, ('ut', {'alpha': 1.0}), [1.5] + [3.0] * 5, 1),
    ]
    for name, kind, D, pts, start, E in opt:
        gp, tp = models(D, pts, np.ones((1, D + 1)))
        m = gp if kind == 'gp' else tp
        x = m.points
        y = data(x, E, np.random.default_rng(len(name)))
        x0 = np.log(np.array(start))
        res = m.optimize(x0, y, x, method='BFGS')
        for k, v in (('x_obs', x), ('y', y), ('x0', x0), ('x', res.x), ('fun', res.fun), ('nit', res.nit),
                     ('status', res.status), ('jac', res.jac)):
            out['opt_{}_{}'.format(name, k)] = np.asarray(v)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'g16_ml2.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes,', len(out), 'arrays')


if __name__ == '__main__':
    main()
