"""The iterated posterior linearisation smoother (IPLS) restated in NumPy on oracle.ssmq_oracle.  x_{-1} ~ N(m0, P0); step k = 0 .. T-1
uses time index k in both transforms.  One iteration takes linearisation moments (ml_j, Pl_j), j = -1 .. T-1 (column j + 1):
    forward, (m, P) the filtered moments of step k - 1:
        z, S_z, C_f = tf_dyn(ml_{k-1}, Pl_{k-1}, k)     F = C_f Pl_{k-1}^-1     a = z - F ml_{k-1}     Lambda = S_z - F Pl_{k-1} F'
        m- = F m + a      P- = F P F' + Lambda + G Q G'      C_k = P F'
        y^, S_y, C_h = tf_obs(ml_k, Pl_k, k)            H = C_h Pl_k^-1         c = y^ - H ml_k        Omega = S_y - H Pl_k H'
        S = H P- H' + Omega + R     K = P- H' S^-1     m_k = m- + K (y_k - H m- - c)     P_k = P- - K S K'
    backward, from (ms_{T-1}, Ps_{T-1}) = (m_{T-1}, P_{T-1}):
        G_k = C_k (P-_k)^-1     ms_{k-1} = m_{k-1} + G_k (ms_k - m-_k)     Ps_{k-1} = P_{k-1} + G_k (Ps_k - P-_k) G_k'
Without linearisation moments a step linearises at its own running moments, where it is the plain filter step (m- = z,
P- = S_z + G Q G', C_k = C_f', S = S_y + R, K = C_h' S^-1) - that route is taken.  A step fails when an input is not finite, a
factorisation fails (Pl, S; P-_k in the backward step) or the filtered mean is not finite (a NaN measurement).  The transforms are the
callables of tests/_innovation_oracle.py; the `_ld` forms are the same steps in long double for sigma_tf_ld transforms."""
import numpy as np
from scipy.linalg import cho_factor, cho_solve

from tests._innovation_oracle import LD, chol_ld, lower_sym
from tests._iterated_oracle import _solve_spd_ld


def _finite(*arrays):
    return all(np.all(np.isfinite(a)) for a in arrays)


def forward_step(m, P, lin_prev, lin_cur, y, k, GQG, R, tf_dyn, tf_obs):
    """One forward step of one trajectory; lin_prev = (ml_{k-1}, Pl_{k-1}), lin_cur = (ml_k, Pl_k), or both None (the running moments).
    Returns m-, P-, C_k, m_k, P_k, conds = [cond Pl_{k-1}, cond Pl_k, cond S] - or NaN results and conds None on a failure."""
    D = np.asarray(m).shape[0]
    nanv, nanm = np.full(D, np.nan), np.full((D, D), np.nan)
    bad = nanv, nanm, nanm, nanv, nanm, None
    m, P = np.array(m, dtype=float), lower_sym(np.asarray(P, dtype=float))
    if not _finite(m, P):
        return bad
    try:
        if lin_prev is None:
            z, Sz, Cf = tf_dyn(m, P, k)
            np.linalg.cholesky(P)
            m_pr, P_pr, C = z, lower_sym(Sz + GQG), np.atleast_2d(Cf).T
            if not _finite(m_pr, P_pr):
                return bad
            yh, Sy, Ch = tf_obs(m_pr, P_pr, k)
            np.linalg.cholesky(P_pr)
            S = lower_sym(Sy + R)
            np.linalg.cholesky(S)
            K = cho_solve(cho_factor(S, lower=True), np.atleast_2d(Ch)).T
            mk = m_pr + K.dot(y - yh)
            conds = [float(np.linalg.cond(P)), float(np.linalg.cond(P_pr)), float(np.linalg.cond(S))]
        else:
            ml0, Pl0 = np.array(lin_prev[0], dtype=float), lower_sym(np.asarray(lin_prev[1], dtype=float))
            ml1, Pl1 = np.array(lin_cur[0], dtype=float), lower_sym(np.asarray(lin_cur[1], dtype=float))
            if not _finite(ml0, Pl0, ml1, Pl1):
                return bad
            z, Sz, Cf = tf_dyn(ml0, Pl0, k)
            np.linalg.cholesky(Pl0)
            F = cho_solve(cho_factor(Pl0, lower=True), np.atleast_2d(Cf).T).T
            m_pr = z + F.dot(m - ml0)
            P_pr = lower_sym(F.dot(P).dot(F.T) + (Sz - F.dot(Pl0).dot(F.T)) + GQG)
            C = P.dot(F.T)
            yh, Sy, Ch = tf_obs(ml1, Pl1, k)
            np.linalg.cholesky(Pl1)
            H = cho_solve(cho_factor(Pl1, lower=True), np.atleast_2d(Ch).T).T
            S = lower_sym(H.dot(P_pr).dot(H.T) + (Sy - H.dot(Pl1).dot(H.T)) + R)
            if not _finite(S):
                return bad
            np.linalg.cholesky(S)
            K = cho_solve(cho_factor(S, lower=True), H.dot(P_pr)).T
            mk = m_pr + K.dot(y - H.dot(m_pr) - (yh - H.dot(ml1)))
            conds = [float(np.linalg.cond(Pl0)), float(np.linalg.cond(Pl1)), float(np.linalg.cond(S))]
        Pk = lower_sym(P_pr - K.dot(S).dot(K.T))
        if not _finite(mk):
            return bad
        return m_pr, P_pr, C, mk, Pk, conds
    except (np.linalg.LinAlgError, ValueError):
        return bad


def backward_step(m_prev, P_prev, m_pr, P_pr, C, ms, Ps):
    """(m_{k-1}, P_{k-1}), (m-_k, P-_k), C_k, (ms_k, Ps_k) -> ms_{k-1}, Ps_{k-1}, cond P-_k (NaN results and None on a failure)."""
    D = np.asarray(ms).shape[0]
    P_pr, P_prev, Ps = lower_sym(np.asarray(P_pr, dtype=float)), lower_sym(np.asarray(P_prev, dtype=float)), lower_sym(np.asarray(Ps, dtype=float))
    try:
        if not _finite(P_pr):
            raise np.linalg.LinAlgError('not finite')
        np.linalg.cholesky(P_pr)
        G = cho_solve(cho_factor(P_pr, lower=True), np.asarray(C, dtype=float).T).T
    except (np.linalg.LinAlgError, ValueError):
        return np.full(D, np.nan), np.full((D, D), np.nan), None
    return m_prev + G.dot(ms - m_pr), lower_sym(P_prev + G.dot(Ps - P_pr).dot(G.T)), float(np.linalg.cond(P_pr))


def iteration(y, m0, P0, lin_m, lin_P, GQG, R, tf_dyn, tf_obs):
    """One iteration for one trajectory, y (Y, T); lin_m (D, T + 1) / lin_P (D, D, T + 1) or None.  Returns a dict: fm (D, T), fP,
    pm, pP, C (D, D, T), sm (D, T + 1), sP (D, D, T + 1) (column 0: the initial state), status (0 or 1 + the failing step: forward sweep
    first, then the backward sweep in its own order), conds_f [T][3], conds_b [T]."""
    D, T = m0.shape[0], y.shape[1]
    out = dict(fm=np.full((D, T), np.nan), fP=np.full((D, D, T), np.nan), pm=np.full((D, T), np.nan), pP=np.full((D, D, T), np.nan),
               C=np.full((D, D, T), np.nan), sm=np.full((D, T + 1), np.nan), sP=np.full((D, D, T + 1), np.nan), status=0, conds_f=[], conds_b=[None] * T)
    m, P = np.asarray(m0, dtype=float), lower_sym(np.asarray(P0, dtype=float))
    for k in range(T):
        lp = None if lin_m is None else (lin_m[:, k], lin_P[..., k])
        lc = None if lin_m is None else (lin_m[:, k + 1], lin_P[..., k + 1])
        m_pr, P_pr, C, m, P, conds = forward_step(m, P, lp, lc, y[:, k], k, GQG, R, tf_dyn, tf_obs)
        if conds is None:
            out['status'] = k + 1
            return out
        out['pm'][:, k], out['pP'][..., k], out['C'][..., k], out['fm'][:, k], out['fP'][..., k] = m_pr, P_pr, C, m, P
        out['conds_f'].append(conds)
    ms, Ps = m, P
    out['sm'][:, T], out['sP'][..., T] = ms, Ps
    for k in range(T - 1, -1, -1):
        mf, Pf = (m0, lower_sym(np.asarray(P0, dtype=float))) if k == 0 else (out['fm'][:, k - 1], out['fP'][..., k - 1])
        ms, Ps, cond = backward_step(mf, Pf, out['pm'][:, k], out['pP'][..., k], out['C'][..., k], ms, Ps)
        if cond is None:
            out['status'] = k + 1
            return out
        out['sm'][:, k], out['sP'][..., k], out['conds_b'][k] = ms, Ps, cond
    return out


def ipls(y, m0, P0, J, GQG, R, tf_dyn, tf_obs, lin_m=None, lin_P=None):
    """J iterations for one trajectory.  Returns the dict of the last iteration plus delta; after a failure every moment is NaN, delta
    is NaN and status that of the first failing iteration."""
    D, T = m0.shape[0], y.shape[1]
    it = None
    for _ in range(J):
        ref = lin_m
        it = iteration(y, m0, P0, lin_m, lin_P, GQG, R, tf_dyn, tf_obs)
        if it['status']:
            for key in ('fm', 'fP', 'pm', 'pP', 'C', 'sm', 'sP'):
                it[key] = np.full(it[key].shape, np.nan)
            it['delta'] = np.nan
            return it
        if ref is None:
            ref = np.concatenate((np.asarray(m0, dtype=float)[:, None], it['fm']), axis=1)
        lin_m, lin_P = it['sm'], it['sP']
    sd = np.sqrt(np.stack([np.diag(it['sP'][..., j]) for j in range(T + 1)], axis=1))
    it['delta'] = float(np.max(np.abs(it['sm'] - ref) / sd))
    return it


# ---- both steps in long double (sigma-point transforms: sigma_tf_ld): what the float64 restatement itself is worth on a case -----------
def forward_step_ld(m, P, lin_prev, lin_cur, y, k, GQG, R, tf_dyn_ld, tf_obs_ld):
    """`forward_step` in long double: m-, P-, C_k, m_k, P_k."""
    m, P = np.asarray(m, dtype=LD), np.asarray(lower_sym(np.asarray(P, dtype=float)), dtype=LD)
    y, R, GQG = np.asarray(y, dtype=LD), np.asarray(R, dtype=LD), np.asarray(GQG, dtype=LD)
    if lin_prev is None:
        z, Sz, Cf = tf_dyn_ld(m, P, k)
        m_pr, P_pr, C = z, lower_sym(Sz + GQG), np.atleast_2d(Cf).T
        yh, Sy, Ch = tf_obs_ld(m_pr, P_pr, k)
        S = lower_sym(Sy + R)
        K = _solve_spd_ld(S, np.atleast_2d(Ch)).T
        mk = m_pr + K.dot(y - yh)
    else:
        ml0, Pl0 = np.asarray(lin_prev[0], dtype=LD), np.asarray(lower_sym(np.asarray(lin_prev[1], dtype=float)), dtype=LD)
        ml1, Pl1 = np.asarray(lin_cur[0], dtype=LD), np.asarray(lower_sym(np.asarray(lin_cur[1], dtype=float)), dtype=LD)
        z, Sz, Cf = tf_dyn_ld(ml0, Pl0, k)
        F = _solve_spd_ld(Pl0, np.atleast_2d(Cf).T).T
        m_pr = z + F.dot(m - ml0)
        P_pr = lower_sym(F.dot(P).dot(F.T) + (Sz - F.dot(Pl0).dot(F.T)) + GQG)
        C = P.dot(F.T)
        yh, Sy, Ch = tf_obs_ld(ml1, Pl1, k)
        H = _solve_spd_ld(Pl1, np.atleast_2d(Ch).T).T
        S = lower_sym(H.dot(P_pr).dot(H.T) + (Sy - H.dot(Pl1).dot(H.T)) + R)
        K = _solve_spd_ld(S, H.dot(P_pr)).T
        mk = m_pr + K.dot(y - H.dot(m_pr) - (yh - H.dot(ml1)))
    return m_pr, P_pr, C, mk, lower_sym(P_pr - K.dot(S).dot(K.T))


def backward_step_ld(m_prev, P_prev, m_pr, P_pr, C, ms, Ps):
    """`backward_step` in long double: ms_{k-1}, Ps_{k-1}."""
    ld = lambda a: np.asarray(a, dtype=LD)      # noqa: E731
    P_pr, P_prev, Ps = ld(lower_sym(np.asarray(P_pr, dtype=float))), ld(lower_sym(np.asarray(P_prev, dtype=float))), ld(lower_sym(np.asarray(Ps, dtype=float)))
    G = _solve_spd_ld(P_pr, ld(C).T).T
    return ld(m_prev) + G.dot(ld(ms) - ld(m_pr)), lower_sym(ld(P_prev) + G.dot(Ps - P_pr).dot(G.T))
