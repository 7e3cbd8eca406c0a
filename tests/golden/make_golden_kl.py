"""
Generate tests/golden/g20_kl.npz by running the REFERENCE's `kl_divergence` / `symmetrized_kl_divergence` (ssmtoybox/utils.py:151-220;
see make_golden.py for how the reference is reached and for the shims - np.asscalar among them), and an extended-precision
(50-digit, mpmath) evaluation of the same formulas as the referee between the reference's float64 result and the device's.

Cases: E in {1, 2, 5, 6}, each with a well-conditioned pair, a pair of covariances with cond ~ 1e6 and an identical pair
(KL = 0), plus one case with scalar inputs.  Stored per case i: c{i}_m0, c{i}_P0, c{i}_m1, c{i}_P1; and over the cases
kl_ref, skl_ref (the reference, float64), kl_ext, skl_ext (extended, rounded to float64), kl_terms, skl_terms (the sum of the
absolute values of the terms the result is added up from: the scale of its rounding error), scalar (1: the inputs are scalars).

Run:  PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python tests/golden/make_golden_kl.py
"""
import os
import sys

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests.golden import make_golden as mg  # noqa: E402,F401  (installs the shims, puts the reference on the path)

from ssmtoybox.utils import kl_divergence, symmetrized_kl_divergence  # noqa: E402

mp.mp.dps = 50


def spd(rng, E, cond):
    q, _ = np.linalg.qr(rng.standard_normal((E, E)))
    ev = np.logspace(0, -np.log10(cond), E) if E > 1 else np.array([1.0])
    P = (q * ev).dot(q.T) * (0.5 + rng.random())
    return 0.5 * (P + P.T)


def kl_ext(m0, P0, m1, P1):
    """(value, sum of |terms|) of the reference's formula in extended precision."""
    k = len(m0)
    M0, M1 = mp.matrix(P0.tolist()), mp.matrix(P1.tolist())
    dm = mp.matrix([mp.mpf(a) - mp.mpf(b) for a, b in zip(m0, m1)])
    inv1 = M1 ** -1
    tr = sum((inv1 * M0)[i, i] for i in range(k))
    quad = (dm.T * inv1 * dm)[0]
    l0, l1 = mp.log(mp.det(M0)), mp.log(mp.det(M1))
    return (tr + quad + l0 - l1 - k) / 2, (abs(tr) + abs(quad) + abs(l0) + abs(l1) + k) / 2


def main():
    rng = np.random.default_rng(20)
    cases = []
    for E in (1, 2, 5, 6):
        for kind in ('well', 'ill', 'same'):
            cond = 1e6 if kind == 'ill' else 10.0
            m0, P0 = rng.standard_normal(E), spd(rng, E, cond)
            if kind == 'same':
                m1, P1 = m0.copy(), P0.copy()
            else:
                m1, P1 = m0 + 0.3 * rng.standard_normal(E), spd(rng, E, cond)
            cases.append((m0, P0, m1, P1, 0))
    cases.append((np.array([0.4]), np.array([[1.7]]), np.array([-0.2]), np.array([[0.6]]), 1))      # scalar inputs
    out = {k: [] for k in ('kl_ref', 'skl_ref', 'kl_ext', 'skl_ext', 'kl_terms', 'skl_terms', 'scalar')}
    for i, (m0, P0, m1, P1, scalar) in enumerate(cases):
        out['c{}_m0'.format(i)], out['c{}_P0'.format(i)], out['c{}_m1'.format(i)], out['c{}_P1'.format(i)] = m0, P0, m1, P1
        if scalar:
            args = (float(m0[0]), float(P0[0, 0]), float(m1[0]), float(P1[0, 0]))
        else:
            args = (m0, P0, m1, P1)
        out['kl_ref'].append(kl_divergence(*args))
        out['skl_ref'].append(symmetrized_kl_divergence(*args))
        a, ta = kl_ext(m0, P0, m1, P1)
        b, tb = kl_ext(m1, P1, m0, P0)
        out['kl_ext'].append(float(a))
        out['skl_ext'].append(float((a + b) / 2))
        out['kl_terms'].append(float(ta))
        out['skl_terms'].append(float((ta + tb) / 2))
        out['scalar'].append(scalar)
    np.savez(os.path.join(HERE, 'g20_kl.npz'), **{k: np.asarray(v) for k, v in out.items()})
    print('g20_kl.npz: {} cases; largest |reference - extended| / terms: KL {:.2e}, SKL {:.2e}'.format(
        len(cases), np.max(np.abs(np.array(out['kl_ref']) - out['kl_ext']) / out['kl_terms']),
        np.max(np.abs(np.array(out['skl_ref']) - out['skl_ext']) / out['skl_terms'])))


if __name__ == '__main__':
    main()
