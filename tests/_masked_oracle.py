"""The masked pass restated in NumPy on oracle.ssmq_oracle.  Step k (0-based) starts from (m, P) (lower triangle of P, as the device
kernels read it); both transforms use time index k; w is the set of observed components, o their number:
    m-, P- = tf_dyn(m, P, k) + G Q G';   y^, P_h, C = tf_obs(m-, P-, k)  (P_h without noise);   S = P_h + R;   e = y_k - y^
    d2 = e_o' S_oo^-1 e_o;   ll = -(o log 2 pi + log det S_oo + d2) / 2                                   (both 0 for o = 0)
    take = (o > 0) and not (d2 > gate[o])
    take:  K = C_o' S_oo^-1,  m = m- + K e_o,  P = P- - K S_oo K';      else:  m = m-,  P = P-
This restatement COMPRESSES to the observed rows and uses numpy.linalg - it does not decouple the unobserved components in place as the
device does (`decoupled` is that form, for the identity test).  The measurement transform runs whatever the mask.  The transforms are
the callables of tests/_innovation_oracle.py, (mean, cov, t) -> (mean_f, cov_f, cov_fx).  `detection_mask` restates the device's mask
generator on tests/_bootstrap_oracle.py::philox4x32_10."""
import numpy as np

from tests._bootstrap_oracle import M32, philox4x32_10
from tests._innovation_oracle import LOG_2PI, lower_sym

DETECT_TAG = 15 << 28


def bits(w, Y):
    """The observed components of mask word w as a bool vector (bits at or above Y are ignored)."""
    return np.array([(int(w) >> i) & 1 for i in range(Y)], dtype=bool)


def _bad(D):
    return dict(m=np.full(D, np.nan), P=np.full((D, D), np.nan), used=0, nis=np.nan, ll=np.nan, conds=None, scales=None, m_pr=None, P_pr=None)


def update(m_pr, P_pr, yh, Ph, C, R, y, obs, gate=None):
    """The update alone, compressed to the rows `obs` (bool (Y,)): m, P, take, d2, ll, cond S_oo, (nis scale, ll scale).  The error
    scales: d2 = |L^-1 e|^2 with e = y - y^ a difference that cancels, so a relative error rtol of y^ is an absolute error rtol (|y| +
    |y^|) of e and the scale of d2 is | |L^-1| (|y| + |y^|) |^2 (at least d2 itself); ll adds o log 2 pi and |log L_ii| term by term."""
    o = int(np.count_nonzero(obs))
    if o == 0:
        return m_pr.copy(), P_pr.copy(), False, 0.0, 0.0, 1.0, (0.0, 0.0)
    S = lower_sym(Ph + R)[np.ix_(obs, obs)]
    e = (np.atleast_1d(y)[obs] - yh[obs]).astype(float)
    L = np.linalg.cholesky(S)
    v = np.linalg.solve(L, e)
    d2 = float(v.dot(v))
    logs = np.log(np.diag(L))
    ll = -0.5 * (o * LOG_2PI + 2.0 * float(np.sum(logs)) + d2)
    iL = np.linalg.inv(L)
    es = np.abs(np.atleast_1d(y)[obs]) + np.abs(yh[obs])
    ns = max(d2, float(np.sum((np.abs(iL).dot(es)) ** 2)))
    ls = 0.5 * (o * LOG_2PI + 2.0 * float(np.sum(np.abs(logs))) + ns)
    thr = np.inf if gate is None else float(np.asarray(gate, dtype=float)[o])
    take = not (d2 > thr)
    if not take:
        return m_pr.copy(), P_pr.copy(), False, d2, ll, float(np.linalg.cond(S)), (ns, ls)
    K = np.linalg.solve(S, C[obs]).T
    return m_pr + K.dot(e), lower_sym(P_pr - K.dot(S).dot(K.T)), True, d2, ll, float(np.linalg.cond(S)), (ns, ls)


def step(m, P, y, w, k, GQG, R, tf_dyn, tf_obs, gate=None):
    """One step of one trajectory; w: the mask word (None: NaN = missing), gate: [Y + 1] or None.  Returns a dict: m (D,), P (D, D),
    used (the mask word applied, 0 when nothing was offered or the gate rejected), nis, ll, conds = (cond P-, cond S_oo), scales = (nis
    scale, ll scale), m_pr, P_pr - or NaN results (conds None) when an input is NaN, a factorisation fails or an observed component is
    not finite."""
    D = np.asarray(m).shape[0]
    y = np.atleast_1d(np.asarray(y, dtype=float))
    Y = y.shape[0]
    obs = ~np.isnan(y) if w is None else bits(w, Y)
    if not (np.all(np.isfinite(m)) and np.all(np.isfinite(np.tril(P))) and np.all(np.isfinite(y[obs]))):
        return _bad(D)
    try:
        m_pr, P_pr, _ = tf_dyn(np.array(m, dtype=float), lower_sym(np.asarray(P, dtype=float)), k)
        P_pr = lower_sym(P_pr + GQG)
        np.linalg.cholesky(P_pr)                                   # (the measurement transform factors P-; raises as it does)
        yh, Ph, C = tf_obs(m_pr, P_pr, k)
        yh, Ph, C = np.atleast_1d(yh), lower_sym(np.atleast_2d(Ph)), np.atleast_2d(C)
        R = np.atleast_2d(np.asarray(R, dtype=float))
        mn, Pn, take, d2, ll, cS, scales = update(m_pr, P_pr, yh, Ph, C, R, y, obs, gate)
    except np.linalg.LinAlgError:
        return _bad(D)
    word = sum(1 << i for i in range(Y) if obs[i])
    return dict(m=mn, P=Pn, used=word if take else 0, nis=d2, ll=ll, conds=(float(np.linalg.cond(P_pr)), cS), scales=scales, m_pr=m_pr,
                P_pr=P_pr)


def masked_filter(y, mask, m0, P0, GQG, R, tf_dyn, tf_obs, gate=None):
    """The recursion for one trajectory, y (Y, T), mask (T,) words or None: fm (D, T), fP (D, D, T), used (T,), nis (T,), ll (T,); NaN
    (used 0) from the first failing step on."""
    D, T = m0.shape[0], y.shape[1]
    fm, fP = np.full((D, T), np.nan), np.full((D, D, T), np.nan)
    used, nis, ll = np.zeros(T, dtype=np.uint32), np.full(T, np.nan), np.full(T, np.nan)
    m, P = m0, P0
    for k in range(T):
        r = step(m, P, y[:, k], None if mask is None else mask[k], k, GQG, R, tf_dyn, tf_obs, gate)
        if r['conds'] is None:
            break
        m, P = r['m'], r['P']
        fm[:, k], fP[..., k], used[k], nis[k], ll[k] = m, P, r['used'], r['nis'], r['ll']
    return fm, fP, used, nis, ll


def decoupled(m_pr, P_pr, yh, Ph, C, R, y, obs):
    """The update as the device forms it: the full Y x Y system with the unobserved components decoupled in place (e_i = 0, S_ii = 1,
    S_ij = S_ji = 0, C_i. = 0).  Returns m, P, d2, log det S."""
    Y = yh.shape[0]
    S = lower_sym(Ph + R)
    keep = np.outer(obs, obs)
    S = np.where(keep, S, np.eye(Y))
    e = np.where(obs, np.where(obs, y, yh) - yh, 0.0)
    Cm = np.where(obs[:, None], C, 0.0)
    L = np.linalg.cholesky(S)
    v = np.linalg.solve(L, e)
    K = np.linalg.solve(S, Cm).T
    return m_pr + K.dot(e), lower_sym(P_pr - K.dot(S).dot(K.T)), float(v.dot(v)), 2.0 * float(np.sum(np.log(np.diag(L))))


# ---- the detection-mask generator (csrc/ssmq_filter_masked.hip: k_detection_mask) -----------------------------------------------------
def uniform(seed, traj, k, tag):
    """uniform_one of csrc/ssmq_rng.h: counter (traj lo, traj hi, k, tag), key (seed lo, seed hi), 53 bits from the first two words."""
    o = philox4x32_10((traj & M32, (traj >> 32) & M32, k & M32, tag & M32), (seed & M32, (seed >> 32) & M32))
    return (float(((o[0] >> 5) << 26) | (o[1] >> 6)) + 0.5) * (1.0 / 9007199254740992.0)


def detection_mask(B, T, Y, p_detect, seed=0, traj_offset=0, per_component=True):
    """mask (T, B) uint32: bit i set iff u(seed, traj_offset + b, k, DETECT_TAG | i) < p_detect[i]; per_component False: one draw
    (i = 0) against p_detect[0], all Y bits together."""
    p = np.broadcast_to(np.asarray(p_detect, dtype=float), (Y,))
    out = np.zeros((T, B), dtype=np.uint32)
    for k in range(T):
        for b in range(B):
            if per_component:
                out[k, b] = sum(1 << i for i in range(Y) if uniform(seed, traj_offset + b, k, DETECT_TAG | i) < p[i])
            else:
                out[k, b] = ((1 << Y) - 1) if uniform(seed, traj_offset + b, k, DETECT_TAG) < p[0] else 0
    return out


# ---- the gate cases the host and the GPU tests share ----------------------------------------------------------------------------------
GATE_CASES = ('ungm_ukf', 'cv_radar', 'ct_bearing')      # sigma-point filters: built without a device
GATE_B, GATE_T, GATE_PROB = 70, 6, 0.99
_GATE = {}


def gate_case(name):
    """(filter, y (Y, T, B), mask (T, B) uint32, gate [Y + 1]): measurements of the filter's own models, every fifth trajectory with a
    gross error (+ 30 sqrt(R_aa) in every component) at step 3; mask[k][b] = (b + k) mod 2^Y; the gate at the chi-square quantiles of
    GATE_PROB.  Made once, never modified."""
    if name not in _GATE:
        from scipy.stats import chi2
        from tests.test_innovation_gpu import simulate
        from tests.test_iterated_gpu import make_case
        alg = make_case(name)
        Y = alg.mod_obs.dim_out
        y = simulate(alg, GATE_B, GATE_T, 3)
        y[:, 3, ::5] += 30.0 * np.sqrt(np.diag(alg.r_cov))[:, None]
        mask = ((np.arange(GATE_B)[None, :] + np.arange(GATE_T)[:, None]) % (1 << Y)).astype(np.uint32)
        mask[3, ::5] = (1 << Y) - 1                    # (the gross errors are offered in full)
        gate = np.concatenate(([np.inf], chi2.ppf(GATE_PROB, np.arange(1, Y + 1))))
        for a in (y, mask, gate):
            a.setflags(write=False)
        _GATE[name] = (alg, y, mask, gate)
    return _GATE[name]
