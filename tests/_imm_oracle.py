"""The interacting multiple-model filter over noise modes restated in NumPy (Blom & Bar-Shalom 1988; the six steps of
ssmq_filter_imm_dev in include/ssmq.h).  Mode j's filter step is the step of the CPU pieces that exist - the oracle's gaussian_filter on
ONE measurement through tests/_sweep_oracle.py: filtered, and the innovation scores of tests/_innovation_oracle.py on its result, both
with the transforms pinned to time index k - with the transforms of tests/_noise_sweep_oracle.py: transforms.  New here: the mixing,
the log-sum-exp weighting and the combination, every sum over modes ascending in the mode index, written once for a dtype: float64 is
the oracle, np.longdouble its twin (`imm(..., dtype=np.longdouble)` runs mixing, weighting and combination in long double on the same
float64 filter steps - what the float64 arithmetic of those three is worth on a case, carried through the recursion)."""
import numpy as np

from tests import _innovation_oracle as ino
from tests import _noise_sweep_oracle as nso
from tests import _sweep_oracle as swo

LD = np.longdouble


def mix(pi, mu, ms, Ps, dtype=np.float64):
    """Steps 1 - 3: (c (M,), m0 (M, D), P0 (M, D, D)) from mu (M,), ms (M, D), Ps (M, D, D)."""
    pi, mu, ms, Ps = (np.asarray(a, dtype=dtype) for a in (pi, mu, ms, Ps))
    M, D = ms.shape
    c, m0, P0 = np.zeros(M, dtype=dtype), np.zeros((M, D), dtype=dtype), np.zeros((M, D, D), dtype=dtype)
    for j in range(M):
        for i in range(M):
            c[j] = c[j] + pi[i, j] * mu[i]
        w = [(pi[i, j] * mu[i] / c[j]) if c[j] != 0 else dtype(i == j) for i in range(M)]
        for i in range(M):
            m0[j] = m0[j] + w[i] * ms[i]
        for i in range(M):
            e = ms[i] - m0[j]
            P0[j] = P0[j] + w[i] * (Ps[i] + np.outer(e, e))
    return c, m0, P0


def combine(c, ll, ms, Ps, dtype=np.float64):
    """Steps 5 - 6: (loglik, mu (M,), fm (D,), fP (D, D)) from c (M,), ll (M,), the updated ms (M, D), Ps (M, D, D)."""
    c, ll, ms, Ps = (np.asarray(a, dtype=dtype) for a in (c, ll, ms, Ps))
    M, D = ms.shape
    with np.errstate(divide='ignore', invalid='ignore'):
        a = np.array([np.log(c[j]) + ll[j] if c[j] != 0 else -dtype(np.inf) for j in range(M)], dtype=dtype)
        amax = a[0]
        for j in range(1, M):
            amax = a[j] if a[j] > amax else amax
        se = dtype(0)
        for j in range(M):
            se = se + np.exp(a[j] - amax)
        lk = amax + np.log(se)
        mu = np.array([np.exp(a[j] - lk) for j in range(M)], dtype=dtype)
    fm, fP = np.zeros(D, dtype=dtype), np.zeros((D, D), dtype=dtype)
    for j in range(M):
        fm = fm + mu[j] * ms[j]
    for j in range(M):
        e = ms[j] - fm
        fP = fP + mu[j] * (Ps[j] + np.outer(e, e))
    return lk, mu, fm, fP


def mode_step(yk, k, m0, P0, Q, R, G, tfd, tfo):
    """Mode j's filter step of time index k from (m0, P0): (m, P lower-symmetric, ll, S), or None where a factorisation fails or a
    score is not a finite number.  gaussian_filter and ino.innovations run on the one measurement with the transforms pinned to k."""
    tdk, tok = (lambda m, P, t: tfd(m, P, k)), (lambda m, P, t: tfo(m, P, k))
    if not (np.all(np.isfinite(m0)) and np.all(np.isfinite(P0))):
        return None
    y1 = yk[:, None]
    fm, fP = swo.filtered(y1, m0, P0, Q, R, G, tdk, tok)
    with np.errstate(all='ignore'):
        _, S, nis, ll = ino.innovations(y1, m0, P0, fm, fP, G.dot(Q).dot(G.T), R, tdk, tok)
    if not (np.isfinite(nis[0]) and np.isfinite(ll[0])):
        return None
    return fm[:, 0], ino.lower_sym(fP[..., 0]), float(ll[0]), S[..., 0]


def imm(case, y, q_rows, r_rows, x0_rows, pi, mu0, weights=None, x0_means=None, dtype=np.float64):
    """y (Y, T, B); q_rows (M, dq, dq), r_rows (M, Y, Y), x0_rows (M, D, D): mode j's covariances; pi (M, M), mu0 (M,); x0_means (M, D) or
    None (the case's m0 for every mode).  Returns dict: mean (D, T, B), cov (D, D, T, B), mode_prob (M, T, B), loglik (T, B),
    loglik_total (B,), status (B,), cond (T, B): the largest cond(S) over the modes; mode_ll (M, T, B).  A trajectory fails as a whole: the
    first step at which a mode's step fails or a mixed quantity is not finite sets status = 1 + k, everything NaN from there on."""
    Y, T, B = y.shape
    M, D = len(q_rows), case['m0'].shape[0]
    tfd, tfo = nso.transforms(case, weights)
    G = case['G']
    out = dict(mean=np.full((D, T, B), np.nan), cov=np.full((D, D, T, B), np.nan), mode_prob=np.full((M, T, B), np.nan),
               loglik=np.full((T, B), np.nan), loglik_total=np.full(B, np.nan), status=np.zeros(B, dtype=np.int32),
               cond=np.full((T, B), np.nan), mode_ll=np.full((M, T, B), np.nan))
    f64 = lambda a: np.asarray(a, dtype=np.float64)      # noqa: E731
    for b in range(B):
        ms = np.array([case['m0'] if x0_means is None else x0_means[j] for j in range(M)], dtype=float)
        Ps = np.array([ino.lower_sym(x0_rows[j]) for j in range(M)], dtype=float)
        mu, total = np.asarray(mu0, dtype=float), 0.0
        for k in range(T):
            c, m0, P0 = (f64(a) for a in mix(pi, mu, ms, Ps, dtype))
            steps = [mode_step(y[:, k, b], k, m0[j], P0[j], q_rows[j], r_rows[j], G, tfd, tfo) for j in range(M)] \
                if np.all(np.isfinite(c)) else [None]
            if any(s is None for s in steps):
                out['status'][b] = 1 + k
                break
            ms, Ps = np.array([s[0] for s in steps]), np.array([s[1] for s in steps])
            ll = np.array([s[2] for s in steps])
            lk, mu, fm, fP = (f64(a) for a in combine(c, ll, ms, Ps, dtype))
            if not (np.isfinite(lk) and np.all(np.isfinite(fm)) and np.all(np.isfinite(fP))):
                out['status'][b] = 1 + k
                break
            total = total + float(lk)
            out['mean'][:, k, b], out['cov'][..., k, b], out['mode_prob'][:, k, b], out['loglik'][k, b] = fm, fP, mu, lk
            out['cond'][k, b], out['mode_ll'][:, k, b] = max(np.linalg.cond(s[3]) for s in steps), ll
        if out['status'][b] == 0:
            out['loglik_total'][b] = total
    return out


def twin_difference(ref, twin):
    """{mean, cov, mode_prob}: max |float64 oracle - long-double twin| / max(1, |value|) over a case."""
    return {k: float(np.max(np.abs(ref[k] - twin[k]) / np.maximum(1.0, np.abs(twin[k])))) for k in ('mean', 'cov', 'mode_prob')}
