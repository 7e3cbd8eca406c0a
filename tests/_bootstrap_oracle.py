"""
Exact restatement, in Python integers and NumPy, of what csrc/ssmq_bootstrap.hip and k_traj_scores (csrc/ssmq_metrics.hip)
compute - the oracle of tests/test_bootstrap_host.py and tests/test_bootstrap_gpu.py.

The draw (the header comment of csrc/ssmq_bootstrap.hip): resample s at position i reads entry j(s, i) of the included list,
    (o0, o1, o2, o3) = Philox4x32-10(counter = (i >> 1, 0, s, BOOT_TAG), key = (seed & 0xffffffff, seed >> 32))
    word = o0 | o1 << 32 for even i,  o2 | o3 << 32 for odd i;     j = (word * n) >> 64.
The per-trajectory scores are the oracle's per-item functions (oracle/ssmq_oracle.py), averaged over the steps k0 .. T-1.
"""
import functools
import math

import numpy as np

from oracle import ssmq_oracle as orc

BOOT_TAG = 0xB0075747
M32 = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon, Moraes, Dror, Shaw: Parallel random numbers: as easy as 1, 2, 3, SC'11)."""
    c0, c1, c2, c3 = counter
    k0, k1 = key
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def draw(seed, s, i, n):
    """j(s, i): the entry of the included list that resample s reads at position i."""
    o = philox4x32_10((i >> 1, 0, s, BOOT_TAG), (seed & M32, (seed >> 32) & M32))
    word = (o[0] | o[1] << 32) if i % 2 == 0 else (o[2] | o[3] << 32)
    return (word * n) >> 64


@functools.lru_cache(maxsize=None)
def draws(seed, s, n):
    """All n entries of resample s (read-only; cached: the tests share them)."""
    out = np.empty(n, dtype=np.int64)
    key = (seed & M32, (seed >> 32) & M32)
    for p in range((n + 1) // 2):
        o = philox4x32_10((p, 0, s, BOOT_TAG), key)
        out[2 * p] = ((o[0] | o[1] << 32) * n) >> 64
        if 2 * p + 1 < n:
            out[2 * p + 1] = ((o[2] | o[3] << 32) * n) >> 64
    out.setflags(write=False)
    return out


def resample_means(data, idx, S, seed, which=None):
    """Means of the resamples `which` (default: all of 0 .. S-1) of data[..., idx] (idx None: all entries), each the
    exactly rounded sum (math.fsum) over n.  data (n_all,) -> (len(which),); data (R, n_all) -> (R, len(which)): the rows
    share the draws."""
    data = np.asarray(data, dtype=np.float64)
    vals = data if idx is None else data[..., np.asarray(idx)]
    n = vals.shape[-1]
    which = range(S) if which is None else which
    rows = np.atleast_2d(vals)
    out = np.array([[math.fsum(row[draws(seed, s, n)]) / n for s in which] for row in rows])
    return out if data.ndim == 2 else out[0]


def traj_scores(x, fm, fP, mse=None, ok=None, k0=0):
    """(scores, scale), each (D + 3, B).  scores: per-dimension RMSE, mean ||x - m||, mean NLL, mean LCR against mse
    (T, D, D) (NaN without) over the steps k0 .. T-1 of every trajectory; NaN columns where not ok[b].  scale: the mean of
    the ABSOLUTE per-step terms of the NLL and LCR rows (what a rounding error of their mean is relative to), the scores
    themselves in the RMSE rows.  x, fm (D, T, B); fP (D, D, T, B)."""
    D, T, B = fm.shape
    ok = np.ones(B, dtype=bool) if ok is None else np.asarray(ok, dtype=bool)
    out, scale = np.full((D + 3, B), np.nan), np.full((D + 3, B), np.nan)
    steps = range(k0, T)
    for b in np.flatnonzero(ok):
        dx = x[:, k0:, b] - fm[:, k0:, b]
        out[:D, b] = np.sqrt(np.mean(orc.squared_error(x[:, k0:, b], fm[:, k0:, b]), axis=1))
        out[D, b] = np.mean(np.sqrt((dx ** 2).sum(axis=0)))
        nll = np.array([orc.neg_log_likelihood(x[:, k, b], fm[:, k, b], fP[..., k, b]) for k in steps])
        out[D + 1, b], scale[D + 1, b] = nll.mean(), np.abs(nll).mean()
        if mse is not None:
            lcr = np.array([orc.log_cred_ratio(x[:, k, b], fm[:, k, b], fP[..., k, b], mse[k]) for k in steps])
            out[D + 2, b], scale[D + 2, b] = lcr.mean(), np.abs(lcr).mean()
        scale[:D + 1, b] = out[:D + 1, b]
    return out, scale
