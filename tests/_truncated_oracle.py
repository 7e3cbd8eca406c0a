"""NumPy restatement of the truncated sigma-point transform (mtran.py:598-622) on given points and weights, and the case
tables of tests/golden/g22_truncated.npz shared by its generator and its tests.

    x_eff_i = m_e + L_e xi_eff_i,  x_j = mean + L xi_j           L = chol(cov), L_e = chol(cov[:de, :de]) = L[:de, :de]
    mean_f = sum_i wm_i f(x_eff_i),  cov_f = sum_i wc_i (f(x_eff_i) - mean_f)(..)',  cov_fx = sum_j wcc_j (f(x_j) - mean_f)(x_j - mean)'
"""
import numpy as np

from oracle import ssmq_oracle as orc

RULES = ('ut', 'sr', 'gh')
DIMS = ((1, 1), (2, 1), (3, 1), (5, 2), (6, 2))          # (dim, dim_eff) of the stored constructor attributes
N_ITEMS = 8
# apply cases: tag -> (integrand id, constants, dim, dim_eff, outputs); every model reads the dim_eff leading state entries
CASES = {
    'pend_meas': (orc.F_PENDULUM_MEAS, (), 2, 1, 1),
    'range_meas': (orc.F_RANGE_MEAS, (), 3, 1, 1),
    'radar_meas': (orc.F_RADAR2D_MEAS, (0.0, 0.0), 5, 2, 2),
    'radar6_meas': (orc.F_RADAR2D_MEAS, (0.0, 0.0), 6, 2, 2),
}
# filter systems: tag -> (T, trajectories, smoothed moments stored)
FILTERS = {'pend': (30, 4, True), 'rer': (20, 4, False)}


def apply(f, mean, cov, dim_eff, xi_eff, wm, wc, xi, wcc):
    """f: callable on one point (the leading dim_eff entries are all it may read); wc, wcc: weight vectors.
    Returns mean_f (E,), cov_f (E, E), cov_fx (E, D)."""
    mean, cov = np.asarray(mean, dtype=float), np.asarray(cov, dtype=float)
    L = np.linalg.cholesky(cov)
    Le = np.linalg.cholesky(cov[:dim_eff, :dim_eff])
    x_eff = mean[:dim_eff, None] + Le.dot(xi_eff)
    x = mean[:, None] + L.dot(xi)
    fx_eff = np.stack([np.atleast_1d(f(x_eff[:, i])) for i in range(x_eff.shape[1])], axis=1)
    fx = np.stack([np.atleast_1d(f(x[:, j])) for j in range(x.shape[1])], axis=1)
    mean_f = fx_eff.dot(wm)
    d_eff, d = fx_eff - mean_f[:, None], fx - mean_f[:, None]
    return mean_f, (d_eff * wc).dot(d_eff.T), (d * wcc).dot((x - mean[:, None]).T)


def integrand(fid, par, time=0.0):
    """The oracle's own evaluation of a built-in integrand as a callable on one point."""
    return lambda x: orc.integrand(fid, np.asarray(x, dtype=float), time, par)
