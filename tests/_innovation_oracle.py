"""The innovation scores of a filter pass restated in NumPy on oracle.ssmq_oracle: for step k with (m, P) the initial moments
(k = 0) or the filtered moments of step k - 1 (lower triangle of P, as the device kernels read it),
    m_pr, P_pr = tf_dyn(m, P, k) + G Q G';   y_mean, S = tf_obs(m_pr, P_pr, k) + R;   e = y_k - y_mean;
    nis = e' S^-1 e (Cholesky of S);   ll = -(Y log 2 pi + log det S + nis) / 2
(additive-noise Gaussian recursion, ssinf.py:254-323 of the reference).  The transforms are callables (mean, cov, t) -> (mean_f,
cov_f, cov_fx) built on the oracle's apply_bq / apply_sigma / apply_linear (or another test oracle's apply)."""
import numpy as np

from oracle import ssmq_oracle as orc

LOG_2PI = float(np.log(2.0 * np.pi))


def lower_sym(P):
    """The symmetric matrix whose lower triangle is that of P."""
    L = np.tril(P)
    return L + np.tril(P, -1).T


def score(y, y_mean, S):
    """(nis, ll) of one innovation."""
    L = np.linalg.cholesky(S)
    v = np.linalg.solve(L, y - y_mean)
    nis = float(v.dot(v))
    return nis, -0.5 * (y.shape[0] * LOG_2PI + 2.0 * float(np.sum(np.log(np.diag(L)))) + nis)


def bq_tf(fid, p, pts, w, state_index=None, tp_nu=None):
    return lambda m, P, t: orc.apply_bq(fid, m, P, float(t), pts, w, p, state_index, tp_nu)


def sigma_tf(fid, p, pts, wm, wc_diag, state_index=None):
    return lambda m, P, t: orc.apply_sigma(fid, m, P, float(t), pts, wm, wc_diag, p, state_index)


def linear_tf(fid, p, state_index=None):
    return lambda m, P, t: orc.apply_linear(fid, m, P, float(t), p, state_index)


def innovations(y, m0, P0, fm, fP, GQG, R, tf_dyn, tf_obs):
    """One trajectory: y (Y, T), m0 (D,), P0 (D, D), fm (D, T), fP (D, D, T).  Returns y_mean (Y, T), S (Y, Y, T), nis (T,), ll (T,);
    a step whose inputs are NaN or one of whose Cholesky factorisations fails is NaN in all four."""
    Y, T = y.shape
    ym, S = np.full((Y, T), np.nan), np.full((Y, Y, T), np.nan)
    nis, ll = np.full(T, np.nan), np.full(T, np.nan)
    for k in range(T):
        m, P = (m0, P0) if k == 0 else (fm[:, k - 1], fP[..., k - 1])
        if not (np.all(np.isfinite(m)) and np.all(np.isfinite(np.tril(P)))):
            continue
        try:
            m_pr, P_pr, _ = tf_dyn(np.array(m, dtype=float), lower_sym(P), k)
            y_mean, P_y, _ = tf_obs(m_pr, lower_sym(P_pr + GQG), k)
            P_y = lower_sym(P_y + R)
            n, l = score(y[:, k], y_mean, P_y)
        except np.linalg.LinAlgError:
            continue
        ym[:, k], S[..., k], nis[k], ll[k] = y_mean, P_y, n, l
    return ym, S, nis, ll


# ---- the same recursion in long double (sigma-point transforms): what the float64 helper itself is worth on a case ------------
LD = np.longdouble


def chol_ld(A):
    n = A.shape[0]
    L = np.zeros((n, n), dtype=LD)
    for j in range(n):
        d = A[j, j] - L[j, :j].dot(L[j, :j])
        if not d > 0:
            raise np.linalg.LinAlgError('not positive definite')
        L[j, j] = np.sqrt(d)
        for i in range(j + 1, n):
            L[i, j] = (A[i, j] - L[i, :j].dot(L[j, :j])) / L[j, j]
    return L


def sigma_tf_ld(fid, p, pts, wm, wc_diag, state_index=None):
    pts, wm, wc = np.asarray(pts, dtype=LD), np.asarray(wm, dtype=LD), np.asarray(wc_diag, dtype=LD)
    p = tuple(LD(v) for v in p)

    def tf(m, P, t):
        x = m[:, None] + chol_ld(P).dot(pts)
        cols = [orc.integrand(fid, x[:, i] if state_index is None else x[np.asarray(state_index), i], LD(t), p) for i in range(x.shape[1])]
        fx = np.stack([np.asarray(c, dtype=LD) for c in cols], axis=1)
        mf = fx.dot(wm)
        dfx = fx - mf[:, None]
        return mf, (dfx * wc).dot(dfx.T), (dfx * wc).dot((x - m[:, None]).T)
    return tf


def score_ld(y, y_mean, S):
    L = chol_ld(S)
    e, v = np.asarray(y, dtype=LD) - y_mean, np.zeros(S.shape[0], dtype=LD)
    for i in range(S.shape[0]):
        v[i] = (e[i] - L[i, :i].dot(v[:i])) / L[i, i]
    nis = v.dot(v)
    return nis, -(S.shape[0] * np.log(2 * np.arccos(LD(-1))) + 2 * np.sum(np.log(np.diag(L))) + nis) / 2


def helper_error(y, m0, P0, fm, fP, GQG, R, tf_dyn_ld, tf_obs_ld, nis64, ll64):
    """max |float64 helper - long-double restatement| / max(1, |value|) over the steps of one trajectory, (nis, ll)."""
    worst = [0.0, 0.0]
    for k in range(y.shape[1]):
        m, P = (m0, P0) if k == 0 else (fm[:, k - 1], fP[..., k - 1])
        m_pr, P_pr, _ = tf_dyn_ld(np.asarray(m, dtype=LD), np.asarray(lower_sym(P), dtype=LD), k)
        y_mean, P_y, _ = tf_obs_ld(m_pr, lower_sym(P_pr + np.asarray(GQG, dtype=LD)), k)
        n, l = score_ld(y[:, k], y_mean, lower_sym(P_y + np.asarray(R, dtype=LD)))
        worst[0] = max(worst[0], float(abs(nis64[k] - n) / max(1, abs(n))))
        worst[1] = max(worst[1], float(abs(ll64[k] - l) / max(1, abs(l))))
    return worst
