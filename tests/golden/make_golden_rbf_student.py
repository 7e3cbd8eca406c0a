"""
Golden vectors for the 'rbf-student' kernel: the reference's RBFStudent (bq/bqkern.py:457-536) Monte-Carlo expectations at
recorded NumPy seeds, the data tests/test_rbf_student_host.py holds the exact mixture oracle (tests/_student_oracle.py)
against.  Reuses the import shims of make_golden.py (importing that module installs them and loads the reference).

Run:  PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python tests/golden/make_golden_rbf_student.py  -> tests/golden/g18_rbf_student.npz

Per case `<case>_*`: x (D, N) unit points of the model, par (1 + D,), dof, seed, num_samples (2e5: ten times fewer than the
kernel's default, so that the script runs in a minute), q (N,), R (D, N), Q (N, N) as exp_x_kx / exp_x_xkx / exp_x_kxkx
return them (three independent sample sets, drawn in this order after np.random.seed(seed)), and for exp_xy_kxy the mean and
the variance (ddof = 1) of the 10 000 per-batch sums of eval(par, xs, xs) over 200 samples each - the estimator's own loop
(bq/bqkern.py:529-536) with its batches kept apart - as kxy_mean / kxy_var, drawn after np.random.seed(seed + 1).
`cases` lists the names.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.golden import make_golden as mg  # noqa: E402,F401  (installs the shims, imports the reference)
from ssmtoybox.bq.bqmod import GaussianProcessModel  # noqa: E402
from ssmtoybox.utils import multivariate_t  # noqa: E402

NUM_SAMPLES = int(2e5)
KXY_BATCHES, KXY_BATCH = 10000, 200
# name, D, ell, parameters of the fully-symmetric rule, alpha, dof of the kernel's density.  The rule's own `dof` only places the
# points: 3 in the first case, which gives the unit points [0, 3, -3]; the rule's default (4) elsewhere.
CASES = (('d1_fs3', 1, 1.0, {'degree': 3, 'dof': 3.0}, 1.0, 4.0), ('d2_fs3', 2, 3.0, {'degree': 3}, 1.5, 4.0),
         ('d5_fs5', 5, 3.0, {'degree': 5}, 1.0, 4.0), ('d6_fs5', 6, 3.0, {'degree': 5}, 1.0, 4.0),
         ('d2_fs3_nu6', 2, 3.0, {'degree': 3}, 1.5, 6.0))


def main():
    out = {}
    for i, (name, D, ell, ppar, alpha, dof) in enumerate(CASES):
        par = np.array([[alpha] + [ell] * D])
        m = GaussianProcessModel(D, par, 'rbf-student', 'fs', dict(ppar))
        k = m.kernel
        k.dof = dof
        k.num_samples = NUM_SAMPLES
        k.batch_size = NUM_SAMPLES // k.num_batches
        seed = 3 + 10 * i
        np.random.seed(seed)
        q = k.exp_x_kx(par, m.points)
        R = k.exp_x_xkx(par, m.points)
        Q = k.exp_x_kxkx(par, par, m.points)
        np.random.seed(seed + 1)
        sums = np.empty(KXY_BATCHES)
        for b in range(KXY_BATCHES):
            xs = multivariate_t(k.mean, k.scale_mat, k.dof, KXY_BATCH).T
            sums[b] = k.eval(par, xs, xs).sum()
        rec = dict(x=m.points, par=par[0], dof=dof, seed=seed, num_samples=NUM_SAMPLES, q=q, R=R, Q=Q, kxy_mean=sums.mean(),
                   kxy_var=sums.var(ddof=1))
        for key, v in rec.items():
            out['{}_{}'.format(name, key)] = np.asarray(v)
        print('  {:11s} D {} N {:3d} dof {} q[0] {:.6f} kxy batch mean {:.4f} var {:.4f}'.format(
            name, D, m.points.shape[1], dof, q[0], rec['kxy_mean'], rec['kxy_var']))
    out['cases'] = np.array([c[0] for c in CASES])
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'g18_rbf_student.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes,', len(out), 'arrays')


if __name__ == '__main__':
    main()
