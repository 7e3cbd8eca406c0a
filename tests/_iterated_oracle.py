"""The iterated posterior linearisation pass (IPLF) restated in NumPy on oracle.ssmq_oracle.  Step k (0-based) starts from (m, P)
(lower triangle of P, as the device kernels read it); both transforms use time index k at every iteration:
    m-, P- = tf_dyn(m, P, k) + G Q G';   (m_0, P_0) = (m-, P-);   for i = 0 .. J - 1:
        y^, S_y, C = tf_obs(m_i, P_i, k)          A = C P_i^-1      b = y^ - A m_i      Omega = S_y - A P_i A'
        S = A P- A' + Omega + R                   K = P- A' S^-1
        m_{i+1} = m- + K (y_k - A m- - b)         P_{i+1} = P- - K S K'
    delta = max_d |m_J[d] - m_{J-1}[d]| / sqrt(P_J[d, d])
Only P_i and S are factored.  The transforms are the callables of tests/_innovation_oracle.py (mean, cov, t) -> (mean_f, cov_f, cov_fx).
`step` is the one-step form (the tests feed it the device's own filtered moments of step k - 1), `iterated_filter` the recursion, and
`step_ld` the one-step form in long double for the sigma-point transforms (tests/_innovation_oracle.py: sigma_tf_ld)."""
import numpy as np
from scipy.linalg import cho_factor, cho_solve

from oracle import ssmq_oracle as orc
from tests._innovation_oracle import LD, chol_ld, lower_sym


def tp_broadcast_tf(fid, p, pts, w, nu, state_index=None):
    """The t-process BQ transform as StudentProcessKalman builds it (dim_out = 1, I_out = eye(1)): the whole scaled (E, E)
    model-variance matrix is added to the covariance, not its diagonal alone (orc.apply_bq adds the diagonal; the correction is that of
    tests/test_oracle_golden.py).  For E = 1 it is orc.apply_bq."""
    def tf(m, P, t):
        mf, cf, cfx = orc.apply_bq(fid, m, P, float(t), pts, w, p, state_index, nu)
        if mf.shape[0] > 1:
            fx = orc.eval_columns(fid, m[:, None] + np.linalg.cholesky(P).dot(pts), float(t), p, state_index)
            full = (nu - 2 + fx.dot(w['iK']).dot(fx.T)) / (nu - 2 + fx.shape[1]) * w['model_var']
            cf = cf - np.diag(np.diag(full)) + full
        return mf, cf, cfx
    return tf


def step(m, P, y, k, J, GQG, R, tf_dyn, tf_obs):
    """One step of one trajectory.  Returns m_J (D,), P_J (D, D), delta, conds: [cond P_0, cond S_0, cond P_1, cond S_1, ...] of the
    iterates - or NaN results (conds None) when an input is NaN or a factorisation fails."""
    D = np.asarray(m).shape[0]
    bad = np.full(D, np.nan), np.full((D, D), np.nan), np.nan, None
    if not (np.all(np.isfinite(m)) and np.all(np.isfinite(np.tril(P)))):
        return bad
    try:
        m_pr, P_pr, _ = tf_dyn(np.array(m, dtype=float), lower_sym(np.asarray(P, dtype=float)), k)
        P_pr = lower_sym(P_pr + GQG)
        mi, Pi, prev, conds = m_pr, P_pr, m_pr, []
        for _ in range(J):
            yh, Sy, C = tf_obs(mi, Pi, k)
            np.linalg.cholesky(Pi)                                   # (the transform factors P_i; raises as it does)
            A = cho_solve(cho_factor(Pi, lower=True), np.atleast_2d(C).T).T
            Om = Sy - A.dot(Pi).dot(A.T)
            S = lower_sym(A.dot(P_pr).dot(A.T) + Om + R)
            np.linalg.cholesky(S)
            K = cho_solve(cho_factor(S, lower=True), A.dot(P_pr)).T
            mn = m_pr + K.dot(y - A.dot(m_pr) - (yh - A.dot(mi)))
            Pn = lower_sym(P_pr - K.dot(S).dot(K.T))
            conds += [float(np.linalg.cond(Pi)), float(np.linalg.cond(S))]
            prev, mi, Pi = mi, mn, Pn
        if not np.all(np.diag(Pi) > 0):
            return bad
        return mi, Pi, float(np.max(np.abs(mi - prev) / np.sqrt(np.diag(Pi)))), conds
    except np.linalg.LinAlgError:
        return bad


def iterated_filter(y, m0, P0, J, GQG, R, tf_dyn, tf_obs):
    """The recursion for one trajectory, y (Y, T): fm (D, T), fP (D, D, T), delta (T,); NaN from the first failing step on."""
    D, T = m0.shape[0], y.shape[1]
    fm, fP, delta = np.full((D, T), np.nan), np.full((D, D, T), np.nan), np.full(T, np.nan)
    m, P = m0, P0
    for k in range(T):
        m, P, d, conds = step(m, P, y[:, k], k, J, GQG, R, tf_dyn, tf_obs)
        if conds is None:
            break
        fm[:, k], fP[..., k], delta[k] = m, P, d
    return fm, fP, delta


# ---- the one-step form in long double: what the float64 restatement itself is worth on a case -----------------------------------
def _solve_spd_ld(A, B):
    """A^-1 B through the Cholesky factor of A, long double."""
    L = chol_ld(A)
    n = A.shape[0]
    B = np.asarray(B, dtype=LD).reshape(n, -1)
    X = np.zeros(B.shape, dtype=LD)
    for c in range(B.shape[1]):
        v = np.zeros(n, dtype=LD)
        for i in range(n):
            v[i] = (B[i, c] - L[i, :i].dot(v[:i])) / L[i, i]
        for i in range(n - 1, -1, -1):
            v[i] = (v[i] - L[i + 1:, i].dot(v[i + 1:])) / L[i, i]
        X[:, c] = v
    return X


def step_ld(m, P, y, k, J, GQG, R, tf_dyn_ld, tf_obs_ld):
    """`step` in long double (transforms: sigma_tf_ld): m_J, P_J, delta."""
    m_pr, P_pr, _ = tf_dyn_ld(np.asarray(m, dtype=LD), np.asarray(lower_sym(np.asarray(P, dtype=float)), dtype=LD), k)
    P_pr = lower_sym(P_pr + np.asarray(GQG, dtype=LD))
    y, R = np.asarray(y, dtype=LD), np.asarray(R, dtype=LD)
    mi, Pi, prev = m_pr, P_pr, m_pr
    for _ in range(J):
        yh, Sy, C = tf_obs_ld(mi, Pi, k)
        A = _solve_spd_ld(Pi, np.atleast_2d(C).T).T
        S = lower_sym(A.dot(P_pr).dot(A.T) + (Sy - A.dot(Pi).dot(A.T)) + R)
        K = _solve_spd_ld(S, A.dot(P_pr)).T
        mn = m_pr + K.dot(y - A.dot(m_pr) - (yh - A.dot(mi)))
        Pn = lower_sym(P_pr - K.dot(S).dot(K.T))
        prev, mi, Pi = mi, mn, Pn
    return mi, Pi, np.max(np.abs(mi - prev) / np.sqrt(np.diag(Pi)))
