"""NumPy restatement of GP quadrature with derivative observations at the sigma points (GaussianProcessDerTransform), written from
the formulas of DESIGN.md 3.34 - not from the reference's code - for any `which_der`, output count and covariance.

Observation order per output: [f(x_1) .. f(x_N) | (J L)[e, :] at which_der[0] | (J L)[e, :] at which_der[1] | ..], M = N + Nd D.
All length-scale matrices are diagonal, lam_k = ell_k^2.  The one ill-conditioned step, the inverse of the jittered joint kernel
matrix, is done by a Cholesky factorisation in numpy.longdouble (80-bit on x86; where longdouble is float64 the oracle is a second
float64 route).  Everything is returned as float64."""
import numpy as np

LD = np.longdouble


def _slots(N, D, wd):
    """(point, direction) of every observation; direction -1: the value."""
    return [(n, -1) for n in range(N)] + [(int(n), k) for n in wd for k in range(D)]


def which(N, which_der):
    return np.arange(N) if which_der is None else np.asarray(which_der, dtype=int).reshape(-1)


def joint_kernel(x, par, which_der=None, scaling=False):
    """(M, M) joint kernel matrix of values and derivatives, no jitter; longdouble."""
    x = np.asarray(x, dtype=LD)
    D, N = x.shape
    par = np.asarray(par, dtype=LD).reshape(-1)
    lam = par[1:] ** 2
    a2 = par[0] ** 2 if scaling else LD(1)
    sl = _slots(N, D, which(N, which_der))
    M = len(sl)
    K = np.zeros((M, M), dtype=LD)
    for r, (i, k) in enumerate(sl):
        for c, (j, l) in enumerate(sl):
            d = (x[:, i] - x[:, j]) / lam
            kff = a2 * np.exp(-0.5 * np.sum((x[:, i] - x[:, j]) ** 2 / lam))
            if k < 0 and l < 0:
                K[r, c] = kff
            elif k < 0:
                K[r, c] = kff * d[l]                 # d/dx_j of k(x_i, x_j)
            elif l < 0:
                K[r, c] = -kff * d[k]                # d/dx_i
            else:
                K[r, c] = kff * ((1 / lam[k] if k == l else 0) - d[k] * d[l])
    return K


def _chol_inv(A):
    """Inverse of a symmetric positive definite longdouble matrix through its Cholesky factor; (inverse, factor)."""
    n = A.shape[0]
    L = np.zeros_like(A)
    for j in range(n):
        s = A[j, j] - np.dot(L[j, :j], L[j, :j])
        if not s > 0:
            raise np.linalg.LinAlgError('Matrix is not positive definite')
        L[j, j] = np.sqrt(s)
        L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j].dot(L[j, :j])) / L[j, j]
    Li = np.zeros_like(A)
    for c in range(n):
        for i in range(c, n):
            s = (1 if i == c else 0) - np.dot(L[i, c:i], Li[c:i, c])
            Li[i, c] = s / L[i, i]
    X = Li.T.dot(Li)
    return 0.5 * (X + X.T), L


def expectations(x, par, which_der=None):
    """Joint kernel expectations under N(0, I), alpha = 1: q (M,), Q (M, M), R (D, M); longdouble."""
    x = np.asarray(x, dtype=LD)
    D, N = x.shape
    par = np.asarray(par, dtype=LD).reshape(-1)
    lam = par[1:] ** 2
    sl = _slots(N, D, which(N, which_der))
    M = len(sl)
    qf = np.prod(1 / lam + 1) ** LD(-0.5) * np.exp(-0.5 * np.sum(x ** 2 / (lam + 1)[:, None], axis=0))
    cQ = np.prod(2 / lam + 1) ** LD(-0.5)
    eta = x / (lam * (2 + lam))[:, None]
    inn = x / lam[:, None]
    mu = x / (1 + lam)[:, None]

    def Qff(i, j):
        # E[k(x, x_i) k(x, x_j)]: product of two Gaussians in x times N(0, I)
        s = x[:, i] + x[:, j]
        return cQ * np.exp(-0.5 * np.sum((x[:, i] ** 2 + x[:, j] ** 2) / lam) + 0.5 * np.sum(s ** 2 / (lam * (2 + lam))))

    q = np.zeros(M, dtype=LD)
    R = np.zeros((D, M), dtype=LD)
    Q = np.zeros((M, M), dtype=LD)
    for r, (i, k) in enumerate(sl):
        if k < 0:
            q[r] = qf[i]
            R[:, r] = qf[i] * mu[:, i]
        else:
            q[r] = -qf[i] * x[k, i] / (1 + lam[k])
            R[:, r] = mu[:, i] * q[r]
            R[k, r] += qf[i] / (1 + lam[k])
        for c, (j, l) in enumerate(sl):
            m = eta[:, i] + eta[:, j]
            qq = Qff(i, j)
            if k < 0 and l < 0:
                Q[r, c] = qq
            elif k < 0:
                Q[r, c] = qq * (m[l] - inn[l, j])
            elif l < 0:
                Q[r, c] = qq * (m[k] - inn[k, i])
            else:
                Q[r, c] = qq * ((inn[k, i] - m[k]) * (inn[l, j] - m[l]) + (1 / (lam[k] * (2 + lam[k])) if k == l else 0))
    return q, Q, R


def weights(x, par, which_der=None, jitter=1e-8):
    """dict wm (M,), Wc (M, M), Wcc (D, M), model_var, integral_var (float64) and iK, q, Q, R."""
    par = np.asarray(par, dtype=float).reshape(-1)
    K = joint_kernel(x, par, which_der)
    iK, _ = _chol_inv(K + LD(jitter) * np.eye(K.shape[0], dtype=LD))
    q, Q, R = expectations(x, par, which_der)
    wm = q.dot(iK)
    Wc = iK.dot(Q).dot(iK)
    Wc = 0.5 * (Wc + Wc.T)
    Wcc = R.dot(iK)
    a2 = LD(par[0]) ** 2
    mv = a2 * (1 - np.trace(Q.dot(iK)))
    iv = a2 * np.prod(2 / np.asarray(par[1:], dtype=LD) ** 2 + 1) ** LD(-0.5) - wm.dot(q)
    f = lambda a: np.asarray(a, dtype=np.float64)      # noqa: E731
    return dict(wm=f(wm), Wc=f(Wc), Wcc=f(Wcc), model_var=float(mv), integral_var=float(iv), iK=f(iK), q=f(q), Q=f(Q), R=f(R))


def observations(f, f_dx, mean, cov, t, points, which_der=None):
    """(fx (E, M), L): f(x, t) -> (E,), f_dx(x, t) -> (E, D), the Jacobian with respect to the full input."""
    mean, cov = np.asarray(mean, dtype=float), np.asarray(cov, dtype=float)
    D, N = points.shape
    L = np.linalg.cholesky(cov)
    x = mean[:, None] + L.dot(points)
    vals = np.stack([np.atleast_1d(f(x[:, n], t)) for n in range(N)], axis=1)                       # (E, N)
    ders = [np.atleast_2d(f_dx(x[:, n], t)).dot(L) for n in which(N, which_der)]                     # (E, D) each
    return np.hstack([vals] + ders), L


def apply(f, f_dx, mean, cov, t, points, which_der, w):
    """(mean_f (E,), cov_f (E, E), cov_fx (E, D)) with the weights w = dict(wm, Wc, Wcc, model_var)."""
    fx, L = observations(f, f_dx, mean, cov, t, points, which_der)
    mf = fx.dot(w['wm'])
    cf = fx.dot(w['Wc']).dot(fx.T) - np.outer(mf, mf) + w['model_var'] * np.eye(fx.shape[0])
    cfx = fx.dot(np.asarray(w['Wcc']).T).dot(L.T)
    return mf, cf, cfx


def apply_batch(f, f_dx, means, covs, times, points, which_der, w):
    out = [apply(f, f_dx, means[b], covs[b], times[b], points, which_der, w) for b in range(len(means))]
    return tuple(np.stack([o[k] for o in out]) for k in range(3))
