"""
The helper functions of the reference's `ssmtoybox/utils.py` that lie on the accelerated path, under their own names:
the multi-index / Vandermonde helpers of the Bayes-Sard weights (utils.py:459-502), the performance metrics
(utils.py:41-148), the KL divergences of the transform accuracy studies (utils.py:151-220) and the bootstrap variance of a score
(utils.py:223-244).  Everything numerical runs on the device through
the C ABI; there is no NumPy fallback.

The metric functions keep the reference's PER-ITEM signatures (one state, one mean, one covariance) and are a thin
convenience: a Monte-Carlo study should reduce its filter outputs where they lie with `mcshard.device_error_sums` /
`device_lcr_sums` (one launch for all trajectories and steps) instead of calling these in a loop, which is what
research/tpq/tpq_base.py:154-172 does on the CPU.  `squared_error` is not restated: its aggregate over the Monte-Carlo
axis is the `se` entry of `mcshard.device_error_sums`.
"""

import ctypes

import numpy as np

from . import _lib, mcshard
from .bq.bqmod import n_sum_k  # noqa: F401  (utils.py:459-475; integer code, defined next to its only user)


def vandermonde(mul_ind, x):
    """utils.py:478-502: (num_points, num_basis) matrix of the monomials x_n ** mul_ind[:, b] (`ssmq_bs_moments`)."""
    mi = np.ascontiguousarray(mul_ind, dtype=np.int32)
    xs, px = _lib.as_c(np.atleast_2d(np.asarray(x, dtype=np.float64)))
    D, N = xs.shape
    if mi.ndim != 2 or mi.shape[0] != D:
        raise ValueError('multi-indices must have one row per dimension of the points')
    out, pout = _lib.out_c((N, mi.shape[1]))
    _lib.check(_lib.load().ssmq_bs_moments(D, N, px, None, mi.ctypes.data_as(_lib.c_int32_p), mi.shape[1], None, None,
                                           None, None, pout), 'ssmq_bs_moments')
    return out


def _planes(a, ld):
    """(D, B) or (D, D, B) host array -> planes [D..][ld] in HBM (one time step)."""
    src = np.asarray(a, dtype=np.float64).reshape(-1, a.shape[-1])
    buf = np.zeros((src.shape[0], ld))
    buf[:, :src.shape[1]] = src
    d = _lib.DeviceBuffer(buf.nbytes)
    d.upload(buf)
    return d


def _one_step(x, m, P):
    """Upload B states / means / covariances of ONE time step; returns (D, B, ld, d_x, d_m, d_P)."""
    x, m = np.asarray(x, dtype=np.float64), np.asarray(m, dtype=np.float64)
    D = m.shape[0]
    m2 = m.reshape(D, -1)
    B = m2.shape[1]
    x2 = np.broadcast_to(x.reshape(D, -1), (D, B))
    ld = max(64, (B + 63) // 64 * 64)
    if P is None:
        P = np.broadcast_to(np.eye(D)[:, :, None], (D, D, B))
    P3 = np.asarray(P, dtype=np.float64).reshape(D, D, -1)
    return D, B, ld, _planes(x2, ld), _planes(m2, ld), _planes(np.broadcast_to(P3, (D, D, B)), ld)


def mse_matrix(x, m):
    """utils.py:41-64: sample mean-square-error matrix of the estimates m (dim, mc) of the state(s) x (dim, 1 | mc)."""
    D, B, ld, d_x, d_m, d_P = _one_step(x, m, None)
    try:
        s = mcshard.device_error_sums(D, B, ld, 1, d_x, d_m, d_P)
    finally:
        for b in (d_x, d_m, d_P):
            b.free()
    return s['mse'][0] / B


def neg_log_likelihood(x, m, P):
    """utils.py:123-148: 0.5 (sign log|det P| + dx' inv(P) dx + d log 2 pi) of one estimate; raises LinAlgError for a
    singular P, where numpy.linalg.inv raises in the reference."""
    D, B, ld, d_x, d_m, d_P = _one_step(x, m, P)
    try:
        s = mcshard.device_error_sums(D, B, ld, 1, d_x, d_m, d_P)
    finally:
        for b in (d_x, d_m, d_P):
            b.free()
    if s['n_pd'][0] != B:
        raise np.linalg.LinAlgError('Singular matrix')
    return float(s['nll'][0])


def log_cred_ratio(x, m, P, MSE):
    """utils.py:66-120: 10 (log10 dx' P^-1 dx - log10 dx' MSE^-1 dx) of one estimate, with `mat_sqrt`'s SVD route for a
    P that is not positive definite (utils.py:412-433).  MSE must be symmetric positive definite here (a sample MSE
    matrix plus its regulariser, research/tpq/tpq_base.py:161-167)."""
    D, B, ld, d_x, d_m, d_P = _one_step(x, m, P)
    try:
        s = mcshard.device_lcr_sums(D, B, ld, 1, d_x, d_m, d_P, np.asarray(MSE, dtype=np.float64).reshape(1, D, D),
                                    reg=0.0)
    finally:
        for b in (d_x, d_m, d_P):
            b.free()
    if s['n'][0] != B:
        raise np.linalg.LinAlgError('log_cred_ratio: covariance or MSE matrix is singular')
    return float(s['lcr'][0])


def bootstrap_var(data, samples=1000, seed=None):
    """utils.py:223-244: bootstrap estimate of the variance of the mean of `data` ((1, mc_sims) or (mc_sims,), squeezed as
    the reference does), `samples` resamples drawn on the device (`ssmq_bootstrap_var`; the draws are the library's
    counter-based ones, not numpy's, so the value agrees with the reference's statistically, not digit by digit).
    seed=None takes the seed from numpy's global generator, so `np.random.seed` governs it as it governs the reference."""
    data = np.ascontiguousarray(np.asarray(data, dtype=np.float64).squeeze())
    if data.ndim != 1:
        raise ValueError('bootstrap_var: data must squeeze to one dimension, got shape {}'.format(data.shape))
    mcshard._check_bootstrap_range(data.shape[0], int(samples), 1)
    if seed is None:
        seed = int(np.random.randint(0, 2 ** 31 - 1)) << 31 | int(np.random.randint(0, 2 ** 31 - 1))
    d, pd = _lib.as_c(data)
    var, pv = _lib.out_c((1,))
    _lib.check(_lib.load().ssmq_bootstrap_var(pd, data.shape[0], int(samples), ctypes.c_uint64(int(seed) & (2 ** 64 - 1)), pv),
               'ssmq_bootstrap_var')
    return float(var[0])


KL_MAX_DIM = 6      # include/ssmq.h ssmq_kl_divergence_dev


def kl_divergence_batch(mean_0, cov_0, mean_1, cov_1, symmetrized=False):
    """B KL divergences in one launch (`k_kl_divergence`, csrc/ssmq_kl.hip): mean_1 (B, E), cov_1 (B, E, E); mean_0 / cov_0
    likewise, or one pair (E,), (E, E) that is used for every item (the Monte-Carlo ground truth against a grid of
    approximations).  Returns (kl (B,), status (B,)).  Each item is the reference's `kl_divergence` (utils.py:151-182, as
    written there, with log(det cov_0 / det cov_1)) or, with `symmetrized`, `symmetrized_kl_divergence` (utils.py:185-220),
    computed through the two Cholesky factors.  A pair with a covariance that is not positive definite gets status 1 and NaN;
    the reference returns NaN or a number without meaning from log(det / det) there.  E <= 6 (NotImplementedError beyond)."""
    m1 = np.ascontiguousarray(mean_1, dtype=np.float64)
    P1 = np.ascontiguousarray(cov_1, dtype=np.float64)
    m0 = np.ascontiguousarray(mean_0, dtype=np.float64)
    P0 = np.ascontiguousarray(cov_0, dtype=np.float64)
    if m1.ndim != 2 or P1.shape != m1.shape + m1.shape[1:]:
        raise ValueError('mean_1 must have shape (B, E) and cov_1 (B, E, E)')
    B, E = m1.shape
    bcast = m0.ndim == 1
    if (bcast and (m0.shape != (E,) or P0.shape != (E, E))) or (not bcast and (m0.shape != (B, E) or P0.shape != (B, E, E))):
        raise ValueError('mean_0 / cov_0 must be (B, E), (B, E, E) like mean_1 / cov_1, or one pair (E,), (E, E)')
    if not 1 <= E <= KL_MAX_DIM:
        raise NotImplementedError('kl_divergence on the device covers 1 <= E <= {} (got E = {})'.format(KL_MAX_DIM, E))
    if B == 0:
        return np.empty(0), np.empty(0, dtype=np.int32)
    d1m, d1P = _lib.SoA.from_host(m1), _lib.SoA.from_host(P1)
    ld = d1m.ld
    if bcast:
        d0m, d0P = _lib.DeviceBuffer(m0.nbytes), _lib.DeviceBuffer(P0.nbytes)
        d0m.upload(m0)
        d0P.upload(P0)
        bufs = [d0m, d0P]
    else:
        s0m, s0P = _lib.SoA.from_host(m0), _lib.SoA.from_host(P0)
        d0m, d0P = s0m.buf, s0P.buf
        bufs = [d0m, d0P]
    d_kl, d_st = _lib.DeviceBuffer(8 * ld), _lib.DeviceBuffer(4 * ld)
    bufs += [d1m.buf, d1P.buf, d_kl, d_st]
    try:
        _lib.check(_lib.load().ssmq_kl_divergence_dev(E, B, ld, ctypes.c_void_p(d0m.ptr), ctypes.c_void_p(d0P.ptr), 1 if bcast else 0,
                                                      d1m.ptr, d1P.ptr, 1 if symmetrized else 0, ctypes.c_void_p(d_kl.ptr),
                                                      ctypes.c_void_p(d_st.ptr)), 'ssmq_kl_divergence_dev')
        kl = d_kl.download((ld,))[:B].copy()
        st = d_st.download((ld,), dtype=np.int32)[:B].copy()
    finally:
        for b in bufs:
            b.free()
    return kl, st


def _kl_single(mean_0, cov_0, mean_1, cov_1, symmetrized):
    m0, m1 = np.atleast_1d(np.asarray(mean_0, dtype=np.float64)), np.atleast_1d(np.asarray(mean_1, dtype=np.float64))
    P0, P1 = np.atleast_2d(np.asarray(cov_0, dtype=np.float64)), np.atleast_2d(np.asarray(cov_1, dtype=np.float64))
    kl, _ = kl_divergence_batch(m0[None], P0[None], m1[None], P1[None], symmetrized=symmetrized)
    return float(kl[0])


def kl_divergence(mean_0, cov_0, mean_1, cov_1):
    """utils.py:151-182: KL divergence between the true Gaussian N(mean_0, cov_0) and the approximation N(mean_1, cov_1), with
    the reference's signature (scalars and 1-D inputs as there) and its formula as written; a Python float - item 0 of
    `kl_divergence_batch`, bit for bit.  NaN if a covariance is not positive definite."""
    return _kl_single(mean_0, cov_0, mean_1, cov_1, False)


def symmetrized_kl_divergence(mean_0, cov_0, mean_1, cov_1):
    """utils.py:185-220: 0.5 (KL(0, 1) + KL(1, 0)); see `kl_divergence`."""
    return _kl_single(mean_0, cov_0, mean_1, cov_1, True)
