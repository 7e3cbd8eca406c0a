"""NumPy restatement of the reference's TaylorGPQDTransform.apply (mtran.py:685-701) in this build's (E, D) orientation of the
cross-covariance, the case table of tests/golden/g21_taylor_gpqd.npz, and the bound of the linearisation limit.

The determinants, the inverse and the products are the reference's own NumPy calls in the reference's own order, so the
restatement agrees with the fixture to the last bits; the integrand value and the Jacobian come from the oracle's model
functions (oracle/ssmq_oracle.py: integrand, jacobian) with the Jacobian placed as apply_linear places it."""
import numpy as np

from oracle import ssmq_oracle as orc

# block -> (fid, integrand constants, D, E, uses the time index)
CASES = {
    'ungm_dyn': (orc.F_UNGM_DYN, (), 1, 1, True),
    'ungm_meas': (orc.F_UNGM_MEAS, (), 1, 1, False),
    'pend_dyn': (orc.F_PENDULUM_DYN, (0.01,), 2, 2, False),
    'pend_meas': (orc.F_PENDULUM_MEAS, (), 2, 1, False),
    'cv_dyn': (orc.F_CV_DYN, (0.5,), 4, 4, False),
    'ungmna_dyn': (orc.F_UNGMNA_DYN, (), 2, 1, True),
}
N_ITEMS = 8          # inputs per block
N_PAR = 3            # kernel-parameter rows per block: alpha = 1 and 2.5 with ell in [0.5, 5], and alpha = 2.5 with ell = 1e3
ELL_LIMIT = 1e3
LIMIT_ROW = 2


def value_and_jacobian(fid, mean, t, p=()):
    """f(mean) (E,) and the Jacobian in the columns of the full input (E, D): a one-column Jacobian on a wider input is
    broadcast into every column, as the reference's meas_eval does (oracle: apply_linear)."""
    D = mean.shape[0]
    fm = np.atleast_1d(orc.integrand(fid, mean, t, p))
    js = orc.jacobian(fid, mean, t, p)
    J = np.zeros((fm.shape[0], D))
    J[:] = js
    return fm, J


def taylor_gpqd(fm, J, cov, alpha, ell):
    """(mean_f (E,), cov_f (E, E), cov_fx (E, D), model_var, integ_var) of mtran.py:685-701 for the integrand value fm and the
    Jacobian J (E, D).  cov_fx is the transpose of the reference's (D, E) array."""
    D = cov.shape[0]
    ell = np.asarray(ell, dtype=float)
    Lam, iLam, eye = np.diag(ell ** 2 * np.ones(D)), np.diag(ell ** -2 * np.ones(D)), np.eye(D)
    wm = np.linalg.det(iLam.dot(cov) + eye) ** -0.5
    mean_f = wm * fm
    wc = np.linalg.det(2 * iLam.dot(cov) + eye) ** -0.5
    Wc = 0.5 * Lam.dot(np.linalg.inv(0.5 * Lam + cov)).dot(cov)
    model_var = alpha ** 2 - alpha ** 2 * wc * (1 + np.trace(Wc.dot(iLam)))
    integ_var = alpha ** 2 * wc - wm ** 2
    cov_f = wc * (np.outer(fm, fm) + J.dot(Wc).dot(J.T)) - np.outer(mean_f, mean_f) + model_var
    cov_fx = Lam.dot(np.linalg.inv(Lam + cov)).dot(cov).dot(J.T)
    return mean_f, cov_f, cov_fx.T, model_var, integ_var


def apply(fid, mean, cov, t, par, p=()):
    """The transform of one item with kernel parameters par = [alpha, ell_1 .. ell_D]."""
    fm, J = value_and_jacobian(fid, np.asarray(mean, dtype=float), t, p)
    return taylor_gpqd(fm, J, np.asarray(cov, dtype=float), par[0], par[1:])


def limit_bound(fm, J, cov, alpha, ell):
    """How far the GPQD moments may lie from the linearisation's f(m), J P J', J P at length-scales ell, per moment, as ABSOLUTE
    deviations (first order in r = ||P|| / min ell^2, doubled for the higher orders; r must be small):
      wm = det(I + Lam^-1 P)^-1/2 and wc = det(I + 2 Lam^-1 P)^-1/2 lie within D r / 2 and D r of 1 (log det <= trace);
      Wc = P - P (Lam / 2 + P)^-1 P and Lam (Lam + P)^-1 P = P - P (Lam + P)^-1 P lie within 2 ||P|| r and ||P|| r of P;
      model_var = alpha^2 (1 - wc (1 + tr(Wc Lam^-1))) lies within alpha^2 (D r + D r) of 0.
    With a = |f|^2 and j = ||J||^2 ||P|| (2-norms):
      mean:  |f| D r / 2
      cov:   D r (a + j) + 2 j r + D r a + 2 alpha^2 D r        (wc - 1 on both terms, Wc - P, wm^2 - 1, model_var)
      ccov:  ||J|| ||P|| r"""
    D = cov.shape[0]
    nP = np.linalg.norm(cov, 2)
    r = nP / float(np.min(np.asarray(ell, dtype=float)) ** 2)
    assert D * r < 1e-3
    nf, nJ = np.linalg.norm(fm), np.linalg.norm(J, 2)
    a, j = nf ** 2, nJ ** 2 * nP
    b_mean = nf * D * r / 2
    b_cov = D * r * (a + j) + 2 * j * r + D * r * a + 2 * alpha ** 2 * D * r
    b_ccov = nJ * nP * r
    return 2 * b_mean, 2 * b_cov, 2 * b_ccov


def kalman_update(m_pr, P_pr, y_mean, P_y, P_yx, y):
    """The oracle's measurement update (ssinf.py:297-323), under the name the filter tests use."""
    return orc.kalman_update(m_pr, P_pr, y_mean, P_y, P_yx, y)
