"""High-precision restatements of the two step kernels under every filter and smoother, and the builders of their test cases.

kalman_update_hp restates `ssmq_kalman_update_dev` (k_kalman_update<D, Y> / k_kalman_update_generic), rts_backward_hp restates
`ssmq_rts_backward_dev` (k_rts_backward<D>), both in DPS-digit mpmath arithmetic from the float64 inputs taken exactly (mpf(float) is
exact, so y - y_mean and every other difference is formed from the exact inputs).  Sums are exact dot products (mp.fdot) rounded
once.  The results go back as float64 (rounded once: half an ulp of the result, against bars of at least 64 eps of the scale).

Every restatement also returns componentwise error scales: the sum of the absolute values of the terms of each update, with the
high-precision gains.  The scales are evaluated in float64 from the rounded gains - a scale needs no more than its leading digits.

The bound (bound_update / bound_rts) is the project's bound for one application of an inverse, max(RTOL, 64 cond eps), taken
componentwise and per item against those scales; `floor=False` drops RTOL for the low-condition sets, where it would hide a
digit-level regression."""
import functools

import mpmath as mp
import numpy as np

from tests._cases import RTOL

DPS = 50
EPS = float(np.finfo(float).eps)
FACTOR = 64.0

TABLE_PAIRS = ((1, 1), (2, 1), (2, 2), (3, 1), (4, 2), (5, 2), (5, 4), (6, 2))      # k_kalman_update<D, Y>
GENERIC_PAIRS = ((1, 2), (3, 3), (7, 3), (16, 1), (1, 16), (16, 16))                # k_kalman_update_generic
RTS_DIMS = (1, 2, 3, 4, 5, 6, 7)                                                    # k_rts_backward<D>
UPDATE_CONDS = {'lo': 1e2, 'hi': 1e8}
RTS_CONDS = {'lo': 1e2, 'hi': 1e6}


# ---- linear algebra on lists of mpf ------------------------------------------------------------------------------------------
def _mat(a):
    return [[mp.mpf(v) for v in row] for row in np.asarray(a, dtype=float).tolist()]


def _vec(a):
    return [mp.mpf(v) for v in np.asarray(a, dtype=float).tolist()]


def _chol(A):
    """Lower Cholesky factor (rows) of the symmetric matrix whose lower triangle is A's."""
    n = len(A)
    L = [[mp.mpf(0)] * n for _ in range(n)]
    for j in range(n):
        d = A[j][j] - mp.fdot(L[j][:j], L[j][:j])
        if not d > 0:
            raise np.linalg.LinAlgError('not positive definite')
        L[j][j] = mp.sqrt(d)
        for i in range(j + 1, n):
            L[i][j] = (A[i][j] - mp.fdot(L[i][:j], L[j][:j])) / L[j][j]
    return L


def _chol_solve(L, b):
    n = len(L)
    v = [mp.mpf(0)] * n
    for i in range(n):
        v[i] = (b[i] - mp.fdot(L[i][:i], v[:i])) / L[i][i]
    for i in range(n - 1, -1, -1):
        v[i] = (v[i] - mp.fdot([L[k][i] for k in range(i + 1, n)], v[i + 1:])) / L[i][i]
    return v


def _gain(A, C):
    """(A^-1 C)' as rows: G[d][i] = X[i][d], X = A^-1 C."""
    L = _chol(A)
    return [_chol_solve(L, [C[i][d] for i in range(len(A))]) for d in range(len(C[0]))]


def _f(a):
    return np.array([[float(v) for v in row] for row in a]) if isinstance(a[0], list) else np.array([float(v) for v in a])


def cond_hp(P):
    """2-norm condition number of a symmetric positive definite float64 matrix: the ratio of the Rayleigh quotients, in DPS digits and
    of the exact matrix, at float64 eigenvectors of its extreme eigenvalues.  A Rayleigh quotient is second order in the vector's error
    (~ cond eps here), so the ratio is good to ~ cond eps relative - where float64 eigenvalues alone leave cond^2 eps in the bar."""
    P = np.asarray(P, dtype=float)
    if P.shape[0] == 1:
        return 1.0
    with mp.workdps(DPS):
        _, V = np.linalg.eigh(P)
        A = _mat(P)

        def rq(v):
            v = _vec(v)
            return mp.fdot(v, [mp.fdot(row, v) for row in A]) / mp.fdot(v, v)
        return float(rq(V[:, -1]) / rq(V[:, 0]))


# ---- the restatements --------------------------------------------------------------------------------------------------------
def kalman_update_hp(m_pr, P_pr, y_mean, P_y, P_yx, y):
    """G = (P_y^-1 P_yx)', m = m_pr + G (y - y_mean), P = P_pr - G P_y G' (left unsymmetrised, as include/ssmq.h promises) of one item:
    m_pr (D,), P_pr (D, D), y_mean (Y,), P_y (Y, Y) symmetric, P_yx (Y, D), y (Y,).
    Returns m_fi, P_fi, and the scales |m_pr| + |G| |y - y_mean| and |P_pr| + |G| |P_y| |G|'."""
    with mp.workdps(DPS):
        Py, D = _mat(P_y), len(m_pr)
        Y = len(Py)
        G = _gain(Py, _mat(P_yx))
        dy = [a - b for a, b in zip(_vec(y), _vec(y_mean))]
        mpr, Ppr = _vec(m_pr), _mat(P_pr)
        m = [mpr[d] + mp.fdot(G[d], dy) for d in range(D)]
        cols = [[Py[i][j] for i in range(Y)] for j in range(Y)]
        W = [[mp.fdot(G[d], cols[j]) for j in range(Y)] for d in range(D)]
        P = [[Ppr[d][e] - mp.fdot(W[d], G[e]) for e in range(D)] for d in range(D)]
        m, P, Gf, dyf = _f(m), _f(P), np.abs(_f(G)), np.abs(_f(dy))
    m_sc = np.abs(np.asarray(m_pr, dtype=float)) + Gf.dot(dyf)
    P_sc = np.abs(np.asarray(P_pr, dtype=float)) + Gf.dot(np.abs(np.asarray(P_y, dtype=float))).dot(Gf.T)
    return m, P, m_sc, P_sc


def rts_backward_hp(fm, fP, pm, pP, pC):
    """The backward pass with the reference's indexing exactly as oracle.ssmq_oracle.rts_smoother states it: arrays (D, T) / (D, D, T)
    hold steps 1..T, the loop is `for k in range(T - 2, 0, -1)`, the gain is (pP[k]^-1 pC[k])', the last two smoothed steps equal the
    filtered ones.  Returns sm, sP and per-step scales |fm[k-1]| + |G| (|ms| + |pm[k]|), |fP[k-1]| + |G| (|Ps| + |pP[k]|) |G|' (the
    filtered moments' own magnitude at the steps the recursion does not reach)."""
    fm, fP = np.asarray(fm, dtype=float), np.asarray(fP, dtype=float)
    D, T = fm.shape
    sm, sP, m_sc, P_sc = fm.copy(), fP.copy(), np.abs(fm), np.abs(fP)
    if T < 3:
        return sm, sP, m_sc, P_sc
    with mp.workdps(DPS):
        ms, Ps = _vec(fm[:, T - 1]), _mat(fP[..., T - 1])
        for k in range(T - 2, 0, -1):
            Pp, mpk = _mat(pP[..., k]), _vec(pm[:, k])
            G = _gain(Pp, _mat(pC[..., k]))
            Gf = np.abs(_f(G))
            m_sc[:, k - 1] = np.abs(fm[:, k - 1]) + Gf.dot(np.abs(_f(ms)) + np.abs(pm[:, k]))
            P_sc[..., k - 1] = np.abs(fP[..., k - 1]) + Gf.dot(np.abs(_f(Ps)) + np.abs(pP[..., k])).dot(Gf.T)
            dm = [a - b for a, b in zip(ms, mpk)]
            dcols = [[Ps[i][j] - Pp[i][j] for i in range(D)] for j in range(D)]
            W = [[mp.fdot(G[d], dcols[j]) for j in range(D)] for d in range(D)]
            f_m, f_P = _vec(fm[:, k - 1]), _mat(fP[..., k - 1])
            ms = [f_m[d] + mp.fdot(G[d], dm) for d in range(D)]
            Ps = [[f_P[d][e] + mp.fdot(W[d], G[e]) for e in range(D)] for d in range(D)]
            sm[:, k - 1], sP[..., k - 1] = _f(ms), _f(Ps)
    return sm, sP, m_sc, P_sc


# ---- bounds ------------------------------------------------------------------------------------------------------------------
def ratio(got, ref, scale, cond, floor=True, steps=1):
    """max over items and components of |got - ref| / scale, in units of that item's steps cond eps (floor: of
    steps max(RTOL / 64, cond eps)), item axis first.  The bound max(RTOL, 64 cond eps) steps holds where this is below FACTOR = 64."""
    got, ref, scale = (np.asarray(a, dtype=float) for a in (got, ref, scale))
    unit = np.asarray(cond, dtype=float) * EPS
    if floor:
        unit = np.maximum(unit, RTOL / FACTOR)
    unit = (unit * max(steps, 1)).reshape((-1,) + (1,) * (got.ndim - 1))
    with np.errstate(invalid='ignore', divide='ignore'):
        r = np.abs(got - ref) / (scale * unit)
    r = np.where((got == ref) & np.isfinite(ref), 0.0, r)            # an exact match is no error, whatever its scale
    return float(np.max(np.where(np.isnan(r), np.inf, r))) if r.size else 0.0


# ---- case builders -----------------------------------------------------------------------------------------------------------
def spd(rng, n, cond, scale=1.0):
    """Symmetric positive definite with a prescribed spectrum: random orthogonal factor, geometric eigenvalues scale .. scale / cond."""
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    lam = scale * cond ** (-np.arange(n) / max(n - 1, 1))
    P = (Q * lam).dot(Q.T)
    return 0.5 * (P + P.T)


def general_cov(rng, n):
    """SPD (cond 10) plus a small antisymmetric part: what an unsymmetrised covariance looks like, so a pass-through of [i][j] is
    distinguishable from one of [j][i]."""
    N = rng.standard_normal((n, n))
    return spd(rng, n, 10.0, rng.uniform(0.5, 2.0)) + 0.05 * (N - N.T)


def update_case(rng, D, Y, B, cond):
    """B independent items, item axis first: m_pr (B, D), P_pr (B, D, D) general, y_mean, y (B, Y), P_y (B, Y, Y) symmetric positive
    definite with the prescribed condition number (Y = 1: log-uniform in [1e-3, 1e3]), P_yx (B, Y, D) general, and cond (B,)."""
    c = dict(m_pr=rng.standard_normal((B, D)), P_pr=np.stack([general_cov(rng, D) for _ in range(B)]),
             y_mean=rng.standard_normal((B, Y)), y=rng.standard_normal((B, Y)), P_yx=rng.standard_normal((B, Y, D)))
    if Y == 1:
        c['P_y'] = 10.0 ** rng.uniform(-3.0, 3.0, (B, 1, 1))
    else:
        c['P_y'] = np.stack([spd(rng, Y, cond, rng.uniform(0.5, 2.0)) for _ in range(B)])
    c['cond'] = np.array([cond_hp(S) for S in c['P_y']])
    return c


def update_ref(c):
    """kalman_update_hp over the items of a case: m (B, D), P (B, D, D) and their scales."""
    out = [kalman_update_hp(c['m_pr'][b], c['P_pr'][b], c['y_mean'][b], c['P_y'][b], c['P_yx'][b], c['y'][b])
           for b in range(c['m_pr'].shape[0])]
    return tuple(np.stack([o[i] for o in out]) for i in range(4))


def scaled_update_case(c, p, space):
    """The case with its measurement space ('y': P_y s^2, P_yx s, y s, y_mean s) or its state space ('x': m_pr s, P_pr s^2, P_yx s)
    scaled by s = 2^p - exact in float64, so the oracle's answer scales exactly with it."""
    s = 2.0 ** p
    c = dict(c)
    c['P_yx'] = c['P_yx'] * s
    if space == 'y':
        c.update(P_y=c['P_y'] * s * s, y=c['y'] * s, y_mean=c['y_mean'] * s)
    else:
        c.update(m_pr=c['m_pr'] * s, P_pr=c['P_pr'] * s * s)
    return c


def rts_case(rng, D, T, B, cond, nan_unread=True):
    """B independent sequences, lane axis first: fm, pm (B, D, T), fP general, pP symmetric positive definite with the prescribed
    condition number, pC[k] = pP[k] A_k' with ||A_k||_2 <= 0.9 (non-symmetric; the gain is then A_k and the recursion does not amplify
    earlier error), all (B, D, D, T); cond (B,) = max_k cond(pP[k]) over the elements the recursion reads.  nan_unread: elements 0 and
    T - 1 of pm, pP, pC, which the reference's indexing never reads, are NaN."""
    fm, pm = rng.standard_normal((B, D, T)), rng.standard_normal((B, D, T))
    fP, pP, pC = (np.zeros((B, D, D, T)) for _ in range(3))
    cond_max = np.ones(B)
    for b in range(B):
        for k in range(T):
            fP[b, :, :, k] = general_cov(rng, D)
            pP[b, :, :, k] = spd(rng, D, cond, rng.uniform(0.5, 2.0))
            A = rng.standard_normal((D, D))
            A *= rng.uniform(0.45, 0.9) / np.linalg.norm(A, 2)
            pC[b, :, :, k] = pP[b, :, :, k].dot(A.T)
            if 1 <= k <= T - 2:
                cond_max[b] = max(cond_max[b], cond_hp(pP[b, :, :, k]))
    if nan_unread:
        for a in (pm, pP, pC):
            a[..., 0] = np.nan
            a[..., T - 1] = np.nan
    return dict(fm=fm, fP=fP, pm=pm, pP=pP, pC=pC, cond=cond_max)


def rts_ref(c):
    out = [rts_backward_hp(c['fm'][b], c['fP'][b], c['pm'][b], c['pP'][b], c['pC'][b]) for b in range(c['fm'].shape[0])]
    return tuple(np.stack([o[i] for o in out]) for i in range(4))


# ---- the shared tables: built once per session, never modified -------------------------------------------------------------
UPD_B, RTS_T, RTS_B = 130, 6, 70


def _freeze(c, ref):
    for a in list(c.values()) + list(ref):
        a.setflags(write=False)
    return c, ref


@functools.lru_cache(maxsize=None)
def update_table(D, Y, cset):
    """(case, (m, P, m_scale, P_scale)) of one (D, Y) pair and conditioning set at the batch the device test runs, read-only."""
    rng = np.random.default_rng([20241, D, Y, int(np.log10(UPDATE_CONDS[cset]))])
    c = update_case(rng, D, Y, UPD_B, UPDATE_CONDS[cset])
    return _freeze(c, update_ref(c))


@functools.lru_cache(maxsize=None)
def rts_table(D, cset):
    rng = np.random.default_rng([20242, D, int(np.log10(RTS_CONDS[cset]))])
    c = rts_case(rng, D, RTS_T, RTS_B, RTS_CONDS[cset])
    return _freeze(c, rts_ref(c))
