"""High-precision restatement of the Monte-Carlo error statistics of csrc/ssmq_metrics.hip (k_error_sums<D>, k_lcr_sums<D>, their
run-time-sized forms, k_indef_sums, k_traj_scores<DT>, k_reduce_partials), and the builders of their test cases.

item_hp gives the terms of one (trajectory, step) entry in DPS-digit mpmath arithmetic from the float64 inputs taken exactly
(mpf(float) is exact, so x - m is formed from the exact inputs): dx^2 per component, ||dx||, the lower triangle of dx dx', the
negative log-likelihood 0.5 (sign(det P) log|det P| + dx' P^-1 dx + D log 2 pi) of any nonsingular P (Cholesky where P is positive
definite, LU with partial pivoting otherwise; an exactly zero pivot = exactly singular, no term), and the log credibility ratio
10 (log10 dx'|P|^-1 dx - log10 dx' M^-1 dx) with |P| from the symmetric eigendecomposition (mp.eigsy) in absolute value - P itself
where P is positive definite, so there the Cholesky factor serves (a singular P: a zero eigenvalue, the ratio is +inf).

Aggregations (sums_ref, scores_ref) are mp.fsum over the entries, rounded once, in the layouts of ssmq_error_sums_dev,
ssmq_lcr_sums_dev and ssmq_traj_scores_dev.  A case holds N distinct entries per step and a lane map idx (B,): lane b carries entry
idx[b] at every step.  Small batches have N = B; large ones draw from a pool of POOL = 61 entries (prime to the wave, block and chunk
sizes 64 / 256 / 2048) through the fixed map (37 b + 11) mod 61, so the oracle evaluates 61 entries per step and adds them with
their multiplicities.

Every value comes with its error scale: the sum of the absolute values of its terms (|0.5 log|det||, 0.5 |q|, the constant;
|10 log10 qa|, |10 log10 qb|; the value itself for the sums of non-negative terms), and with the condition number that enters its
bound: the largest cond(P) among the entries of the value, for the credibility ratio together with cond(M); 1 for the values that
apply no inverse (se, rmse, mse, the RMSE rows).  check() applies the project's bound for one application of an inverse,
max(RTOL, 64 cond eps) (tests/_step_oracle.ratio), after the non-finite values have been compared exactly.

The sums over the batch add nothing to that bound for the device: its summation order is fixed and shallow (8 entries serially per
thread, 6 shuffle levels, 4 waves, then the chunks: at most 8 + 6 + 4 + 3 additions deep at the largest batch tested), i.e. at most
21 eps of the scale against the bar's 64 eps at cond = 1.  The NumPy restatement adds its entries serially, (n - 1) eps in the worst
case and about sqrt(n) eps in practice (31 eps at n = 2049, 68 eps at n = 4097, measured at D = 1), so the host test holds it to
the same bound at batches of up to 257 and leaves the larger ones to the device."""
import functools

import mpmath as mp
import numpy as np

from tests import _step_oracle as so
from tests._step_oracle import DPS, EPS, FACTOR, cond_hp, ratio, spd  # noqa: F401  (re-exported for the tests)

POOL, PERM_A, PERM_C = 61, 37, 11
CONDS = {'lo': 1e2, 'hi': 1e8}
EDGE_LANES = (0, 63, 64, 255, 256, 2047, 2048)


# ---- one entry ---------------------------------------------------------------------------------------------------------------
def _chol_or_none(A):
    try:
        return so._chol(A)
    except np.linalg.LinAlgError:
        return None


def _forward(L, b):
    v = []
    for i in range(len(L)):
        v.append((b[i] - mp.fdot(L[i][:i], v)) / L[i][i])
    return v


def _lu_solve(A, b):
    """(sign of det, log|det|, A^-1 b) by LU with partial pivoting; None at an exactly zero pivot column (A exactly singular)."""
    n = len(A)
    A, z = [row[:] for row in A], list(b)
    sign, la = 1, mp.mpf(0)
    for k in range(n):
        p = max(range(k, n), key=lambda i: abs(A[i][k]))
        if A[p][k] == 0:
            return None
        if p != k:
            A[k], A[p], z[k], z[p], sign = A[p], A[k], z[p], z[k], -sign
        if A[k][k] < 0:
            sign = -sign
        la += mp.log(abs(A[k][k]))
        for i in range(k + 1, n):
            f = A[i][k] / A[k][k]
            A[i] = A[i][:k + 1] + [A[i][j] - f * A[k][j] for j in range(k + 1, n)]
            z[i] -= f * z[k]
    for i in range(n - 1, -1, -1):
        z[i] = (z[i] - mp.fdot(A[i][i + 1:], z[i + 1:])) / A[i][i]
    return sign, la, z


def item_hp(x, m, P, Lm=None):
    """The terms of one entry, mpf valued (call inside mp.workdps(DPS)): dx2 [D], norm, outer (lower triangle, row by row), pd,
    singular, nll / nll_scale (None if singular), cond, and with the Cholesky factor Lm of the step's MSE matrix lcr / lcr_scale."""
    D = len(x)
    dx = [a - b for a, b in zip(so._vec(x), so._vec(m))]
    A = so._mat(P)
    e = dict(dx2=[d * d for d in dx], outer=[dx[i] * dx[j] for i in range(D) for j in range(i + 1)])
    e['norm'] = mp.sqrt(mp.fsum(e['dx2']))
    const = D * mp.log(2 * mp.pi) / 2
    L = _chol_or_none(A)
    e['pd'], e['singular'] = L is not None, False
    if L is not None:
        v = _forward(L, dx)
        qa, hl = mp.fdot(v, v), mp.fsum(mp.log(L[i][i]) for i in range(D))
        e['nll'], e['nll_scale'] = hl + qa / 2 + const, abs(hl) + qa / 2 + const
        e['cond'] = cond_hp(P)
    else:
        lu = _lu_solve(A, dx)
        if lu is None:
            e['singular'], e['nll'], e['nll_scale'], e['cond'], qa = True, None, None, np.inf, mp.inf
        else:
            sign, la, z = lu
            q = mp.fdot(dx, z)
            e['nll'], e['nll_scale'] = (sign * la + q) / 2 + const, (abs(la) + abs(q)) / 2 + const
            E, Q = mp.eigsy(mp.matrix(A))
            lam = [abs(E[i]) for i in range(D)]
            e['cond'] = float(max(lam) / min(lam))
            qa = mp.fsum(mp.fdot([Q[k, i] for k in range(D)], dx) ** 2 / lam[i] for i in range(D))
    if Lm is not None:
        w = _forward(Lm, dx)
        qb = mp.fdot(w, w)
        la10, lb10 = 10 * mp.log10(qa), 10 * mp.log10(qb)
        e['lcr'], e['lcr_scale'] = la10 - lb10, abs(la10) + abs(lb10)
    return e


# ---- cases -------------------------------------------------------------------------------------------------------------------
def pool_index(B):
    """Lane -> pool entry of a large batch."""
    return (PERM_A * np.arange(B) + PERM_C) % POOL


def make_case(x, fm, fP, mse=None, idx=None, ok=None, reg=1e-6):
    """x, fm (D, T, N), fP (D, D, T, N): N distinct entries per step; mse (T, D, D) as handed to the wrappers (None: no credibility
    ratio); idx (B,) lane -> entry (default: one lane per entry); ok (B,) False = the trajectory is excluded."""
    D, T, N = fm.shape
    assert np.array_equal(fP, np.swapaxes(fP, 0, 1), equal_nan=True), 'every P is exactly symmetric'
    idx = np.arange(N) if idx is None else np.asarray(idx)
    ok = np.ones(idx.size, dtype=bool) if ok is None else np.asarray(ok, dtype=bool)
    c = dict(D=D, T=T, N=N, B=idx.size, x=x, fm=fm, fP=fP, mse=mse, idx=idx, ok=ok, reg=reg, _cache={},
             M=None if mse is None else np.asarray(mse, dtype=float) + reg * np.eye(D))       # as the wrapper forms it
    for a in c.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return c


def with_lanes(c, idx=None, ok=None):
    """The same entries (and their evaluated terms: _cache is shared) under another lane map / status mask."""
    d = dict(c)
    if idx is not None:
        d['idx'], d['B'] = np.asarray(idx), len(idx)
        d['ok'] = np.ones(d['B'], dtype=bool)
    if ok is not None:
        d['ok'] = np.asarray(ok, dtype=bool)
    return d


def lanes(c):
    """The batch as the NumPy oracle takes it: x, fm (D, T, B), fP (D, D, T, B), ok (B,)."""
    return c['x'][..., c['idx']], c['fm'][..., c['idx']], c['fP'][..., c['idx']], c['ok']


def planes(c, ld):
    """The batch as the device takes it: x, fm [T][D][ld], fP [T][D*D][ld], status [ld] int32.  The padding lanes B .. ld-1 and the
    excluded trajectories hold NaN in every plane, as a failed filter leaves them."""
    x, fm, fP, ok = lanes(c)
    D, T, B = c['D'], c['T'], c['B']
    out = [np.full((T, n, ld), np.nan) for n in (D, D, D * D)]
    out[0][:, :, :B], out[1][:, :, :B] = x.transpose(1, 0, 2), fm.transpose(1, 0, 2)
    out[2][:, :, :B] = fP.transpose(2, 0, 1, 3).reshape(T, D * D, B)
    for a in out:
        a[:, :, :B][:, :, ~ok] = np.nan
    status = np.zeros(ld, dtype=np.int32)
    status[:B][~ok] = 3
    return out[0], out[1], out[2], status


def evaluate(c):
    """terms[t][i] = item_hp of entry i at step t, and the MSE factors; evaluated once per set of entries and kept with it."""
    if 'terms' not in c['_cache']:
        with mp.workdps(DPS):
            Lm = [None] * c['T'] if c['M'] is None else [_chol_or_none(so._mat(c['M'][t])) for t in range(c['T'])]
            terms = [[item_hp(c['x'][:, t, i], c['fm'][:, t, i], c['fP'][:, :, t, i], Lm[t]) for i in range(c['N'])]
                     for t in range(c['T'])]
        cm = [np.nan if L is None else cond_hp(c['M'][t]) for t, L in enumerate(Lm)]
        c['_cache']['terms'] = (terms, [L is not None for L in Lm], cm)
    return c['_cache']['terms']


def _fmax(v, default=1.0):
    v = [a for a in v if np.isfinite(a)]
    return max(v) if v else default


def sums_ref(c):
    """(ref, scale, cond): dicts of se (T, D), rmse, nll (T,), mse (T, D, D), n_ok, n_pd, lcr, n (T,) - the layouts of
    ssmq_error_sums_dev and ssmq_lcr_sums_dev (lcr, n: only with an MSE matrix; a step whose MSE matrix is not positive definite has
    lcr = n = 0).  scale: of every value the sum of the absolute values of its terms; cond: (T,) per value."""
    terms, m_ok, cm = evaluate(c)
    D, T = c['D'], c['T']
    mult = np.bincount(c['idx'][c['ok']], minlength=c['N'])
    used = np.flatnonzero(mult)
    ref = dict(se=np.zeros((T, D)), rmse=np.zeros(T), nll=np.zeros(T), mse=np.zeros((T, D, D)), n_ok=np.zeros(T), n_pd=np.zeros(T))
    scale = dict(nll=np.zeros(T))
    cond = dict(se=np.ones(T), rmse=np.ones(T), mse=np.ones(T), nll=np.ones(T))
    if c['M'] is not None:
        ref.update(lcr=np.zeros(T), n=np.zeros(T))
        scale['lcr'], cond['lcr'] = np.zeros(T), np.ones(T)
    tri = [(i, j) for i in range(D) for j in range(i + 1)]
    with mp.workdps(DPS):
        for t in range(T):
            es = [(int(mult[i]), terms[t][i]) for i in used]
            ref['se'][t] = [float(mp.fsum(k * e['dx2'][d] for k, e in es)) for d in range(D)]
            ref['rmse'][t] = float(mp.fsum(k * e['norm'] for k, e in es))
            for p, (i, j) in enumerate(tri):
                ref['mse'][t, i, j] = ref['mse'][t, j, i] = float(mp.fsum(k * e['outer'][p] for k, e in es))
            ref['n_ok'][t] = sum(k for k, e in es)
            reg = [(k, e) for k, e in es if not e['singular']]
            ref['n_pd'][t] = sum(k for k, e in reg)
            ref['nll'][t] = float(mp.fsum(k * e['nll'] for k, e in reg))
            scale['nll'][t] = float(mp.fsum(k * e['nll_scale'] for k, e in reg))
            cond['nll'][t] = _fmax([e['cond'] for k, e in reg])
            if c['M'] is not None and m_ok[t]:
                ref['n'][t] = ref['n_ok'][t]
                ref['lcr'][t] = float(mp.fsum(k * e['lcr'] for k, e in es))
                scale['lcr'][t] = float(mp.fsum(k * e['lcr_scale'] for k, e in reg))
                cond['lcr'][t] = max(_fmax([e['cond'] for k, e in reg]), cm[t])
    scale['se'], scale['rmse'] = ref['se'], ref['rmse']                       # sums of non-negative terms
    d = np.sqrt(np.einsum('tii->ti', ref['mse']))
    scale['mse'] = d[:, :, None] * d[:, None, :]                               # sum |dx_i dx_j| <= sqrt(sum dx_i^2 sum dx_j^2)
    return ref, scale, cond


def scores_ref(c, k0):
    """(ref, scale, cond), each (D + 3, B): the rows of ssmq_traj_scores_dev over the steps k0 .. T-1.  NaN columns for excluded
    trajectories; NaN in the NLL row where a step's P is singular (the LCR row is +inf there), NaN in the LCR row without an MSE
    matrix or where a step's MSE matrix is not positive definite."""
    terms, m_ok, cm = evaluate(c)
    D, T, N = c['D'], c['T'], c['N']
    n = T - k0
    ref, scale, cond = np.full((D + 3, N), np.nan), np.full((D + 3, N), np.nan), np.ones((D + 3, N))
    with mp.workdps(DPS):
        for i in np.unique(c['idx'][c['ok']]):
            es = [terms[t][i] for t in range(k0, T)]
            ref[:D, i] = [float(mp.sqrt(mp.fsum(e['dx2'][d] for e in es) / n)) for d in range(D)]
            ref[D, i] = float(mp.fsum(e['norm'] for e in es) / n)
            scale[:D + 1, i] = ref[:D + 1, i]
            cp = _fmax([e['cond'] for e in es])
            if not any(e['singular'] for e in es):
                ref[D + 1, i] = float(mp.fsum(e['nll'] for e in es) / n)
                scale[D + 1, i] = float(mp.fsum(e['nll_scale'] for e in es) / n)
                cond[D + 1, i] = cp
            if c['M'] is not None and all(m_ok[k0:]):
                ref[D + 2, i] = float(mp.fsum(e['lcr'] for e in es) / n)
                scale[D + 2, i] = float(mp.fsum(e['lcr_scale'] for e in es if not e['singular']) / n)
                cond[D + 2, i] = max(cp, _fmax(cm[k0:]))
    out = tuple(a[:, c['idx']] for a in (ref, scale, cond))
    for a in out[:2]:
        a[:, ~c['ok']] = np.nan
    out[2][:, ~c['ok']] = 1.0
    return out


# ---- the bound ---------------------------------------------------------------------------------------------------------------
def check(got, ref, scale, cond, floor=True):
    """The non-finite values (NaN, +-inf) of got and ref must coincide exactly; returns so.ratio over the finite ones, every value
    an item of its own with its own cond (cond broadcasts against got from the left: (T,) against (T, D, D), or elementwise).  The
    bound max(RTOL, 64 cond eps) holds where the result is below FACTOR."""
    got, ref, scale = (np.asarray(a, dtype=float) for a in (got, ref, scale))
    assert got.shape == ref.shape, (got.shape, ref.shape)
    cond = np.asarray(cond, dtype=float)
    if cond.shape != got.shape:
        cond = cond.reshape(cond.shape + (1,) * (got.ndim - cond.ndim))
    cond = np.broadcast_to(cond, got.shape)
    fin = np.isfinite(ref)
    odd = ~fin
    assert np.array_equal(got[odd], ref[odd], equal_nan=True), 'non-finite values differ: {} against {}'.format(got[odd], ref[odd])
    return ratio(got[fin], ref[fin], scale[fin], cond[fin], floor=floor)


# ---- builders of covariances ---------------------------------------------------------------------------------------------------
def _sym(P):
    return 0.5 * (P + P.T)


def indefinite(rng, n, spread, negative=False, scale=1.0):
    """Symmetric nonsingular with dense eigenvectors: |lambda| geometric scale .. scale / spread; signs alternate (n >= 2: at least
    one of each), or are all negative."""
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    lam = scale * spread ** (-np.arange(n) / max(n - 1, 1))
    lam = -lam if negative else lam * np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
    return _sym((Q * lam).dot(Q.T))


def singular_rowcol(rng, n, i):
    """Positive definite (cond 1e2) with row and column i zeroed: exactly singular."""
    P = spd(rng, n, 1e2).copy()
    P[i, :] = 0.0
    P[:, i] = 0.0
    return P


def rank_deficient(rng, n):
    """A A' with A (n, n - 1), symmetrised: rank n - 1 up to rounding - the last Cholesky pivot is at rounding level, of either sign."""
    A = rng.standard_normal((n, n - 1))
    return _sym(A.dot(A.T))


def _fma(a, b, c):
    """a b + c rounded once."""
    with mp.workprec(2200):
        return float(mp.mpf(a) * mp.mpf(b) + mp.mpf(c))


def lu_pivots(P, fused=False):
    """The pivots of float64 LU with partial pivoting in the operation order of lu_solve_logdet (csrc/ssmq_metrics.hip); fused: with
    the elimination's multiply-subtract contracted into one fused operation, as the device compiler is free to do."""
    A = np.array(P, dtype=float)
    n = A.shape[0]
    piv = np.zeros(n)
    for k in range(n):
        p = k + int(np.argmax(np.abs(A[k:, k])))
        A[[k, p]] = A[[p, k]]
        piv[k] = A[k, k]
        if piv[k] == 0.0:
            break
        for i in range(k + 1, n):
            f = A[i, k] / piv[k]
            for j in range(k + 1, n):
                A[i, j] = _fma(-f, A[k, j], A[i, j]) if fused else A[i, j] - f * A[k, j]
    return piv


def nonsingular_f64(P):
    """No float64 LU pivot is exactly zero, with or without fused multiply-subtracts."""
    return bool(np.all(lu_pivots(P) != 0.0) and np.all(lu_pivots(P, fused=True) != 0.0))


def deviations(rng, P, lo=0.5, hi=2.0):
    """A deviation x - m of the size P claims: V sqrt|lambda| z, z standard normal, times a factor in [lo, hi] (dx' |P|^-1 dx ~ D)."""
    lam, V = np.linalg.eigh(P)
    return rng.uniform(lo, hi) * V.dot(np.sqrt(np.abs(lam)) * rng.standard_normal(P.shape[0]))


def entries(rng, covs):
    """x, fm (D, T, N), fP (D, D, T, N) from covs[t][i]: means standard normal, deviations as `deviations` (standard normal where
    P is exactly singular, so that the deviation has a component in its null space)."""
    T, N, D = len(covs), len(covs[0]), covs[0][0].shape[0]
    fm, x, fP = rng.standard_normal((D, T, N)), np.zeros((D, T, N)), np.zeros((D, D, T, N))
    for t in range(T):
        for i in range(N):
            P = covs[t][i]
            fP[:, :, t, i] = P
            x[:, t, i] = fm[:, t, i] + (deviations(rng, P) if np.all(lu_pivots(P) != 0.0) else rng.standard_normal(D))
    return x, fm, fP


def mse_matrices(rng, D, T, cond):
    return np.stack([spd(rng, D, cond, rng.uniform(0.5, 2.0)) for _ in range(T)])


def pd_case(seed, D, T, N, cond):
    """N positive-definite entries per step with the prescribed condition number (P and the MSE matrices), scales in [0.5, 2]."""
    rng = np.random.default_rng([20251, seed, D, T, N, int(np.log10(cond))])
    covs = [[spd(rng, D, cond, rng.uniform(0.5, 2.0)) for _ in range(N)] for _ in range(T)]
    x, fm, fP = entries(rng, covs)
    return make_case(x, fm, fP, mse_matrices(rng, D, T, cond))


# ---- the shared tables: built once per session, never modified -------------------------------------------------------------
DIM_B, DIM_LD, DIM_T = 130, 192, 3


@functools.lru_cache(maxsize=None)
def dim_case(D, cset):
    """Every dimension: a distinct entry per lane and step, B = 130, T = 3."""
    return pd_case(1, D, DIM_T, DIM_B, CONDS[cset])


@functools.lru_cache(maxsize=None)
def pool_case(D, T):
    """The pool of the batch-edge and status cases: 61 entries per step, cond 1e2."""
    return pd_case(2, D, T, POOL, CONDS['lo'])


NOTPD_B, NOTPD_LD, NOTPD_T = 2053, 2112, 2
NOTPD_LANES = EDGE_LANES + (NOTPD_B - 1,)
NOTPD_KINDS = (('indef', 1e2), ('negdef', 1e2), ('indef', 1e6), ('negdef', 1e6), ('indef', 1e6), ('negdef', 1e2), ('indef', 1e2),
               ('negdef', 1e6))
SING_STEP, SING_ZERO, SING_ROWCOL = 1, 2, 5          # at step 1 the entries of NOTPD_LANES[2] / [5] are exactly singular


@functools.lru_cache(maxsize=None)
def notpd_case(D):
    """A positive-definite pool batch (B = 2053, T = 2) with eight entries of their own at NOTPD_LANES: indefinite and negative
    definite with dense eigenvectors and |lambda| spreads of 1e2 and 1e6; at step SING_STEP two of them are exactly singular (the
    zero matrix; a positive-definite matrix with one row and column zeroed)."""
    rng = np.random.default_rng([20252, D])
    covs = [[spd(rng, D, CONDS['lo'], rng.uniform(0.5, 2.0)) for _ in range(POOL)] for _ in range(NOTPD_T)]
    for t in range(NOTPD_T):
        for kind, spread in NOTPD_KINDS:
            covs[t].append(indefinite(rng, D, spread, kind == 'negdef', rng.uniform(0.5, 2.0)))
    covs[SING_STEP][POOL + SING_ZERO] = np.zeros((D, D))
    covs[SING_STEP][POOL + SING_ROWCOL] = singular_rowcol(rng, D, D // 2)
    x, fm, fP = entries(rng, covs)
    idx = pool_index(NOTPD_B)
    idx[list(NOTPD_LANES)] = POOL + np.arange(len(NOTPD_LANES))
    return make_case(x, fm, fP, mse_matrices(rng, D, NOTPD_T, CONDS['lo']), idx=idx)


CLS_B, CLS_T = 512, 2


@functools.lru_cache(maxsize=None)
def classification_case(D):
    """Every P numerically rank deficient, except one genuinely indefinite entry per step (lane 100 + t) that sends the sums to
    their second pass.  No entry is exactly singular: no float64 LU pivot is zero (nonsingular_f64; asserted again by the host
    test)."""
    rng = np.random.default_rng([20253, D])
    def draw():
        while True:             # about one A A' in ten has a last float64 pivot of exactly zero: those are drawn again
            P = rank_deficient(rng, D)
            if nonsingular_f64(P):
                return P
    covs = [[draw() for _ in range(CLS_B)] for _ in range(CLS_T)]
    for t in range(CLS_T):
        covs[t][100 + t] = indefinite(rng, D, 1e2)
    x, fm, fP = entries(rng, covs)
    return make_case(x, fm, fP, mse_matrices(rng, D, CLS_T, CONDS['lo']))


def scaled_case(c, p):
    """x, m scaled by 2^p and P, mse by 2^2p - exact in float64, so se and the MSE sums scale exactly; the NLL and the credibility
    ratio (the regularisation keeps its size) are the oracle's on the scaled inputs."""
    s = 2.0 ** p
    return make_case(c['x'] * s, c['fm'] * s, c['fP'] * s * s, c['mse'] * s * s, idx=c['idx'], ok=c['ok'], reg=c['reg'])
