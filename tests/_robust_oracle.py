"""The outlier-robust pass restated in NumPy on oracle.ssmq_oracle.  Measurement noise r_k | lambda_k ~ N(0, R / lambda_k), lambda_k ~
Gamma(dof / 2, rate dof / 2), R the scale matrix.  Step k (0-based) starts from (m, P) (lower triangle of P, as the device kernels
read it); both transforms use time index k:
    m-, P- = tf_dyn(m, P, k) + G Q G';   y^, P_h, C = tf_obs(m-, P-, k)  (P_h without noise);   e = y_k - y^;   lambda_0 = 1
    for i = 0 .. J - 2:   S_i = P_h + R / lambda_i      r^ = (R / lambda_i) S_i^-1 e      Psi = r^ r^' + P_h - P_h S_i^-1 P_h
                          gamma = sum_ab iR[a, b] Psi[a, b]      lambda_{i+1} = (dof + Y) / (dof + gamma)
    S = P_h + R / lambda_{J-1}      K = C' S^-1      m = m- + K e      P = P- - K S K'
    lam = lambda_{J-1},  delta = |lambda_{J-1} - lambda_{J-2}| / lambda_{J-1}  (0 for J = 1)
Only Y x Y matrices are factored after the transforms.  The transforms are the callables of tests/_innovation_oracle.py (mean, cov, t)
-> (mean_f, cov_f, cov_fx), the helpers tests/_iterated_oracle.py uses.  `step` is the one-step form (the tests feed it the device's
own filtered moments of step k - 1), `robust_filter` the recursion, `step_state_space` the form of the papers (Psi through the
posterior moments of every iterate, A = C P-^-1), and `step_ld` the one-step form in long double for the sigma-point
transforms (tests/_innovation_oracle.py: sigma_tf_ld)."""
import numpy as np
from scipy.linalg import cho_factor, cho_solve

from tests._innovation_oracle import LD, lower_sym
from tests._iterated_oracle import _solve_spd_ld, tp_broadcast_tf  # noqa: F401  (tp_broadcast_tf: re-exported for the tests)


def _bad(D):
    return np.full(D, np.nan), np.full((D, D), np.nan), np.nan, np.nan, None, (np.nan, np.nan, np.nan)


def _prior(m, P, k, GQG, tf_dyn, tf_obs):
    m_pr, P_pr, _ = tf_dyn(np.array(m, dtype=float), lower_sym(np.asarray(P, dtype=float)), k)
    P_pr = lower_sym(P_pr + GQG)
    np.linalg.cholesky(P_pr)                                       # (the measurement transform factors P-; raises as it does)
    yh, Ph, C = tf_obs(m_pr, P_pr, k)
    return m_pr, P_pr, np.atleast_1d(yh), lower_sym(np.atleast_2d(Ph)), np.atleast_2d(C)


def weight_step(lam, e, Ph, R, iR, dof):
    """One round of the fixed point: (lambda_{i+1}, gamma, cond S_i, the error scale of lambda_{i+1}).  gamma is a sum of terms of
    size gs = sum_ab |iR[a, b]| (|r^_a r^_b| + |P_h[a, b]| + |(P_h S^-1 P_h)[a, b]|) - P_h - P_h S^-1 P_h cancels where R / lambda is
    small against P_h - so a relative error rtol of the terms is an absolute error rtol gs of gamma, and of lambda_{i+1} =
    (dof + Y) / (dof + gamma) one of rtol gs lambda_{i+1} / (dof + gamma): that factor is the scale."""
    Rl = R / lam
    S = lower_sym(Ph + Rl)
    np.linalg.cholesky(S)
    cf = cho_factor(S, lower=True)
    rh = Rl.dot(cho_solve(cf, e))
    PSP = Ph.dot(cho_solve(cf, Ph))
    Psi = np.outer(rh, rh) + Ph - PSP
    gamma = float(np.sum(iR * Psi))
    gs = float(np.sum(np.abs(iR) * (np.abs(np.outer(rh, rh)) + np.abs(Ph) + np.abs(PSP))))
    ln = (dof + e.shape[0]) / (dof + gamma)
    return ln, gamma, float(np.linalg.cond(S)), gs * ln / (dof + gamma)


def step(m, P, y, k, J, dof, GQG, R, tf_dyn, tf_obs):
    """One step of one trajectory.  Returns m (D,), P (D, D), lam, delta, conds: [cond P-, cond S_0, .., cond S_{J-2}, cond S], and
    scales = (ws, dm, dP): ws the largest error scale of a weight over the iterations (weight_step; 0 for J = 1: the weight is the
    constant 1), dm = max |dm / dlambda| = max |K (R / lambda) S^-1 e| / lambda and dP = max |dP / dlambda| = max |K (R / lambda) K'| /
    lambda at the last weight: an error rtol ws of the weight moves the mean by rtol ws dm and the covariance by rtol ws dP, on top
    of their own rounding - or NaN results (conds None) when an input is NaN, a factorisation fails or a weight is not a positive finite number."""
    D = np.asarray(m).shape[0]
    if not (np.all(np.isfinite(m)) and np.all(np.isfinite(np.tril(P))) and np.all(np.isfinite(y))):
        return _bad(D)
    try:
        m_pr, P_pr, yh, Ph, C = _prior(m, P, k, GQG, tf_dyn, tf_obs)
        R = np.atleast_2d(np.asarray(R, dtype=float))
        iR = np.linalg.inv(R)
        e = np.atleast_1d(y) - yh
        lam, prev, conds, wscale = 1.0, 1.0, [float(np.linalg.cond(P_pr))], 0.0
        for _ in range(J - 1):
            prev = lam
            lam, _, c, ws = weight_step(lam, e, Ph, R, iR, dof)
            conds.append(c)
            wscale = max(wscale, ws)
            if not (np.isfinite(lam) and lam > 0.0):
                return _bad(D)
        S = lower_sym(Ph + R / lam)
        np.linalg.cholesky(S)
        K = cho_solve(cho_factor(S, lower=True), C).T
        conds.append(float(np.linalg.cond(S)))
        mn = m_pr + K.dot(e)
        Pn = lower_sym(P_pr - K.dot(S).dot(K.T))
        KR = K.dot(R / lam)
        dm = float(np.max(np.abs(KR.dot(cho_solve(cho_factor(S, lower=True), e))))) / lam
        return mn, Pn, lam, (abs(lam - prev) / lam if J > 1 else 0.0), conds, (wscale, dm, float(np.max(np.abs(KR.dot(K.T)))) / lam)
    except np.linalg.LinAlgError:
        return _bad(D)


def robust_filter(y, m0, P0, J, dof, GQG, R, tf_dyn, tf_obs):
    """The recursion for one trajectory, y (Y, T): fm (D, T), fP (D, D, T), lam (T,), delta (T,); NaN from the first failing step on."""
    D, T = m0.shape[0], y.shape[1]
    fm, fP, lam, delta = np.full((D, T), np.nan), np.full((D, D, T), np.nan), np.full(T, np.nan), np.full(T, np.nan)
    m, P = m0, P0
    for k in range(T):
        m, P, lk, d, conds, _ = step(m, P, y[:, k], k, J, dof, GQG, R, tf_dyn, tf_obs)
        if conds is None:
            break
        fm[:, k], fP[..., k], lam[k], delta[k] = m, P, lk, d
    return fm, fP, lam, delta


def step_state_space(m, P, y, k, J, dof, GQG, R, tf_dyn, tf_obs, literal=False):
    """`step` in the state-space form of the papers, with A = C P-^-1, b = y^ - A m- and Omega = P_h - A P- A': the measurement model
    is y = A x + b + w + r, w ~ N(0, Omega) the residual of the statistical linearisation.  Under the moment-matched joint w is
    conditioned on y together with x, which is the Gaussian conditioning of `step` written on the pair (x, w):
        Psi = (y - y^ - [A I] (mu_i - mu-)) (..)' + [A I] Sigma_i [A I]',   (mu_i, Sigma_i) the posterior of (x, w) under lambda_i.
    literal=True is the formula with the residual left at its prior, Psi = (y - y^ - A (m_i - m-)) (..)' + A P_i A' + Omega with
    (m_i, P_i) the posterior of x alone: the same numbers where Omega = 0 (a linear model), another fixed point where it is not.
    Returns m, P, lam, delta, the weights of every iteration."""
    m_pr, P_pr, yh, Ph, C = _prior(m, P, k, GQG, tf_dyn, tf_obs)
    R = np.atleast_2d(np.asarray(R, dtype=float))
    iR = np.linalg.inv(R)
    y = np.atleast_1d(y)
    D, Y = m_pr.shape[0], y.shape[0]
    A = cho_solve(cho_factor(P_pr, lower=True), C.T).T
    Om = Ph - A.dot(P_pr).dot(A.T)
    Pa = np.zeros((D + Y, D + Y))
    Pa[:D, :D], Pa[D:, D:] = P_pr, Om
    Ha = np.hstack((A, np.eye(Y)))
    lam, prev, lams = 1.0, 1.0, [1.0]

    def posterior(lam):
        S = lower_sym(Ha.dot(Pa).dot(Ha.T) + R / lam)
        K = cho_solve(cho_factor(S, lower=True), Ha.dot(Pa)).T
        return K.dot(y - yh), Pa - K.dot(S).dot(K.T)
    for _ in range(J - 1):
        du, Sg = posterior(lam)
        if literal:
            r = y - yh - A.dot(du[:D])
            Psi = np.outer(r, r) + A.dot(Sg[:D, :D]).dot(A.T) + Om
        else:
            r = y - yh - Ha.dot(du)
            Psi = np.outer(r, r) + Ha.dot(Sg).dot(Ha.T)
        prev, lam = lam, (dof + Y) / (dof + float(np.sum(iR * Psi)))
        lams.append(lam)
    du, Sg = posterior(lam)
    return m_pr + du[:D], lower_sym(Sg[:D, :D]), lam, (abs(lam - prev) / lam if J > 1 else 0.0), lams


# ---- the one-step form in long double: what the float64 restatement itself is worth on a case -----------------------------------
def step_ld(m, P, y, k, J, dof, GQG, R, tf_dyn_ld, tf_obs_ld):
    """`step` in long double (transforms: sigma_tf_ld): m, P, lam, delta."""
    m_pr, P_pr, _ = tf_dyn_ld(np.asarray(m, dtype=LD), np.asarray(lower_sym(np.asarray(P, dtype=float)), dtype=LD), k)
    P_pr = lower_sym(P_pr + np.asarray(GQG, dtype=LD))
    yh, Ph, C = tf_obs_ld(m_pr, P_pr, k)
    Ph, C = lower_sym(np.atleast_2d(Ph)), np.atleast_2d(C)
    R = np.atleast_2d(np.asarray(R, dtype=LD))
    Y = R.shape[0]
    iR = _solve_spd_ld(R, np.eye(Y, dtype=LD))
    e = np.atleast_1d(np.asarray(y, dtype=LD)) - np.atleast_1d(yh)
    lam = prev = LD(1.0)
    dof = LD(dof)
    for _ in range(J - 1):
        Rl = R / lam
        S = lower_sym(Ph + Rl)
        rh = Rl.dot(_solve_spd_ld(S, e)[:, 0])
        Psi = np.outer(rh, rh) + Ph - Ph.dot(_solve_spd_ld(S, Ph))
        prev, lam = lam, (dof + Y) / (dof + np.sum(iR * Psi))
    S = lower_sym(Ph + R / lam)
    K = _solve_spd_ld(S, C).T
    return m_pr + K.dot(e), lower_sym(P_pr - K.dot(S).dot(K.T)), lam, (abs(lam - prev) / lam if J > 1 else LD(0.0))
