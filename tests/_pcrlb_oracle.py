"""
NumPy restatement of the posterior Cramer-Rao sums and recursion (csrc/ssmq_pcrlb_kernel.h, csrc/ssmq_api_pcrlb.hip; include/ssmq.h
ssmq_pcrlb_sums_dev states both) - the oracle of tests/test_pcrlb_host.py and tests/test_pcrlb_gpu.py - and a twin of the recursion in
50-digit mpmath arithmetic from the float64 sums taken exactly.

A pair of models is a `Pair`: the Jacobians as NumPy callables that return the matrices ALREADY PLACED into the state's columns
(Jf (D, D), Jh (Y, D)), the noise, the initial covariance, and a function that builds the package's model objects.  The sums run in the
device's stated order: trajectories in groups of 256, inside a group the 64 lanes of a wave by the butterfly l ^ 32, 16, .. 1, the four
waves as (w0 + w1) + (w2 + w3), the groups in ascending order; lanes past B hold zeros.
"""
import numpy as np

from tests import _user_jac_oracle as uj

DPS = 50


def tri_index(D):
    return [(i, k) for i in range(D) for k in range(i + 1)]


def width(D):
    return D * (D + 1) + D * D


def ordered_sum(terms):
    """terms (B, N) -> (N,) in the device's order."""
    B, N = terms.shape
    G = (B + 255) // 256
    v = np.zeros((G * 256, N))
    v[:B] = terms
    v = v.reshape(G, 4, 64, N)
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, :, lane ^ o]
    w = v[:, :, 0]                                   # (G, 4, N): every lane holds the same bits
    rows = (w[:, 0] + w[:, 1]) + (w[:, 2] + w[:, 3])
    s = rows[0].copy()
    for g in range(1, G):
        s = s + rows[g]
    return s


def quad_terms(J, W):
    """Per trajectory the lower triangle of J' W J, packed: J (B, E, D), W (E, E) -> (B, D (D + 1) / 2), and the same with every factor
    replaced by its absolute value (the sum of the absolute values of the terms)."""
    D = J.shape[2]
    M = np.einsum('bei,bek->bik', J, np.einsum('ef,bfk->bek', W, J))
    Ma = np.einsum('bei,bek->bik', np.abs(J), np.einsum('ef,bfk->bek', np.abs(W), np.abs(J)))
    ii, kk = zip(*tri_index(D))
    return M[:, ii, kk], Ma[:, ii, kk]


class Pair:
    def __init__(self, name, D, Y, Jf, Jh, Q, R, P0, models, m0=None, G=None):
        self.name, self.D, self.Y, self.Jf, self.Jh = name, D, Y, Jf, Jh
        self.Q, self.R, self.P0 = (np.atleast_2d(np.asarray(a, dtype=float)) for a in (Q, R, P0))
        self.m0 = np.zeros(D) if m0 is None else np.asarray(m0, dtype=float)
        self.G = np.eye(D) if G is None else np.asarray(G, dtype=float)
        self.models = models                          # () -> (dyn, obs) of the package

    @property
    def Qi(self):
        return np.linalg.inv(self.G.dot(self.Q).dot(self.G.T))

    @property
    def Ri(self):
        return np.linalg.inv(self.R)


def jacobians(pair, x):
    """x (D, T + 1, B) -> F (T, B, D, D) at (p_j, t = j), H (T, B, Y, D) at (p_{j+1}, t = j)."""
    D, T1, B = x.shape
    T = T1 - 1
    F, H = np.empty((T, B, D, D)), np.empty((T, B, pair.Y, D))
    for j in range(T):
        for b in range(B):
            F[j, b] = pair.Jf(x[:, j, b], float(j))
            H[j, b] = pair.Jh(x[:, j + 1, b], float(j))
    return F, H


def sums(pair, x):
    """(sums (T, S), the sums of the absolute values of the terms (T, S)) in the layout of ssmq_pcrlb_sums_dev."""
    F, H = jacobians(pair, x)
    T, B, D = F.shape[0], F.shape[1], pair.D
    out, out_abs = np.empty((T, width(D))), np.empty((T, width(D)))
    Qi, Ri = pair.Qi, pair.Ri
    for j in range(T):
        a, a_abs = quad_terms(F[j], Qi)
        c, c_abs = quad_terms(H[j], Ri)
        terms = np.concatenate([a, F[j].reshape(B, D * D), c], axis=1)
        out[j] = ordered_sum(terms)
        out_abs[j] = np.abs(np.concatenate([a_abs, np.abs(F[j]).reshape(B, D * D), c_abs], axis=1)).sum(axis=0)
    return out, out_abs


def unpack(row, D):
    """One row of sums -> (A (D, D) symmetric, Fsum (D, D), C (D, D) symmetric)."""
    tri = D * (D + 1) // 2
    A, C = np.zeros((D, D)), np.zeros((D, D))
    for n, (i, k) in enumerate(tri_index(D)):
        A[i, k] = A[k, i] = row[n]
        C[i, k] = C[k, i] = row[tri + D * D + n]
    return A, row[tri:tri + D * D].reshape(D, D).copy(), C


def recursion(s, B_total, P0, Qi):
    """float64: info (D, D, T), bound (D, D, T), rmse_bound (T,), status - the finaliser's statement in NumPy."""
    D, T = P0.shape[0], s.shape[0]
    info, bound, rmse = (np.full(sh, np.nan) for sh in ((D, D, T), (D, D, T), (T,)))
    try:
        J = np.linalg.inv(P0)
        np.linalg.cholesky(P0)
    except np.linalg.LinAlgError:
        return info, bound, rmse, 1
    for j in range(T):
        if not np.all(np.isfinite(s[j])):
            return info, bound, rmse, 1 + j
        A, Fs, C = unpack(s[j], D)
        D11, Fm, D22 = A / B_total, Fs / B_total, Qi + C / B_total
        D12 = -Fm.T.dot(Qi)
        M = J + D11
        try:
            np.linalg.cholesky(M)
            Jn = D22 - D12.T.dot(np.linalg.solve(M, D12))
            Jn = 0.5 * (Jn + Jn.T)
            np.linalg.cholesky(Jn)
        except np.linalg.LinAlgError:
            return info, bound, rmse, 1 + j
        J = Jn
        info[:, :, j], bound[:, :, j] = J, np.linalg.inv(J)
        rmse[j] = np.sqrt(np.trace(bound[:, :, j]))
    return info, bound, rmse, 0


def recursion_mp(s, B_total, P0, Q, G=None):
    """The same in DPS-digit arithmetic from the float64 inputs taken exactly (Qi is inverted there too): float64 roundings of info,
    bound, rmse_bound, and the largest 2-norm condition number of the matrices J_{j-1} + D11_j it factors."""
    import mpmath as mp
    with mp.workdps(DPS):
        D, T = P0.shape[0], s.shape[0]
        Gm = mp.eye(D) if G is None else mp.matrix(G.tolist())
        Qi = mp.inverse(Gm * mp.matrix(Q.tolist()) * Gm.T)
        J = mp.inverse(mp.matrix(P0.tolist()))
        info, bound, rmse, cond = np.empty((D, D, T)), np.empty((D, D, T)), np.empty(T), 0.0
        n = mp.mpf(int(B_total))
        for j in range(T):
            A, Fs, C = unpack(s[j], D)
            D11, Fm = mp.matrix(A.tolist()) / n, mp.matrix(Fs.tolist()) / n
            D22 = Qi + mp.matrix(C.tolist()) / n
            D12 = -(Fm.T * Qi)
            M = J + D11
            cond = max(cond, float(np.linalg.cond(np.array(M.tolist(), dtype=float))))
            J = D22 - D12.T * mp.inverse(M) * D12
            Bm = mp.inverse(J)
            info[:, :, j] = np.array(J.tolist(), dtype=float)
            bound[:, :, j] = np.array(Bm.tolist(), dtype=float)
            rmse[j] = float(mp.sqrt(sum(Bm[i, i] for i in range(D))))
        return info, bound, rmse, cond


def riccati(F, H, Q, R, P0, T):
    """The Kalman filter's covariance recursion for constant F, H: P_j (D, D, T), P_{-1} = P0."""
    P, out = P0.copy(), np.empty(P0.shape + (T,))
    for j in range(T):
        Pp = F.dot(P).dot(F.T) + Q
        S = H.dot(Pp).dot(H.T) + R
        K = Pp.dot(H.T).dot(np.linalg.inv(S))
        P = Pp - K.dot(S).dot(K.T)
        P = 0.5 * (P + P.T)
        out[:, :, j] = P
    return out


def linear_sums(F, H, Qi, Ri, T, B):
    """The exact sums of a linear pair over B trajectories (every term the same): (T, S)."""
    D = F.shape[0]
    a = quad_terms(F[None], Qi)[0][0]
    c = quad_terms(H[None], Ri)[0][0]
    return np.tile(B * np.concatenate([a, F.reshape(-1), c]), (T, 1))


# ---- the pairs of the two test files ---------------------------------------------------------------------------------------------------
PEND_DT = 0.01
VDP_DT, VDP_MU = 0.1, 1.5
POLAR_CODE = 'const double r2 = x[0]*x[0] + x[1]*x[1]; o[0] = sqrt(r2); o[1] = atan2(x[1], x[0]);'
POLAR_JAC = ('const double r2 = x[0]*x[0] + x[1]*x[1]; const double r = sqrt(r2); J[0] = x[0]/r; J[1] = x[1]/r; '
             'J[ldj] = -x[1]/r2; J[ldj+1] = x[0]/r2;')
# time in both Jacobians: the transition of tests/_user_jac_oracle.py, and a measurement whose H' Ri H is (1 + 0.5 t)^2 / R whatever the state
TMEAS_CODE = 'o[0] = (1.0 + 0.5*t)*x[0];'
TMEAS_JAC = 'J[0] = 1.0 + 0.5*t;'
LIN_F = np.array([[0.9, 0.2], [-0.1, 0.8]])
LIN_H = np.array([[1.0, 0.5]])
LIN_CODE = 'o[0] = 0.9*x[0] + 0.2*x[1]; o[1] = -0.1*x[0] + 0.8*x[1];'
LIN_JAC = 'J[0] = 0.9; J[1] = 0.2; J[ldj] = -0.1; J[ldj+1] = 0.8;'
LIN_MEAS_CODE = 'o[0] = x[0] + 0.5*x[1];'
LIN_MEAS_JAC = 'J[0] = 1.0; J[1] = 0.5;'


def _polar_dx(x, t):
    r2 = x[0] * x[0] + x[1] * x[1]
    r = np.sqrt(r2)
    return np.array([[x[0] / r, x[1] / r], [-x[1] / r2, x[0] / r2]])


def _rv(sm, dim, cov, mean=None):
    return sm.GaussRV(dim, mean=mean, cov=np.atleast_2d(cov))


def pair(name):
    from ssmtoybox_amd import ssmod as sm
    if name == 'ungm':
        Q, R, P0 = [[10.0]], [[1.0]], [[1.0]]
        return Pair(name, 1, 1, uj.ungm_dx, uj.ungm_meas_dx, Q, R, P0,
                    lambda: (sm.UNGMTransition(_rv(sm, 1, P0), _rv(sm, 1, Q)), sm.UNGMMeasurement(_rv(sm, 1, R), 1)))
    if name == 'pendulum':
        dt = PEND_DT
        Q = 0.01 * np.array([[(dt ** 3) / 3, (dt ** 2) / 2], [(dt ** 2) / 2, dt]])
        R, P0, m0 = [[0.002]], 0.05 * np.eye(2), np.array([1.5, 0.0])
        Jf = lambda x, t: np.array([[1.0, dt], [-9.81 * dt * np.cos(x[0]), 1.0]])               # noqa: E731
        Jh = lambda x, t: np.array([[np.cos(x[0]), np.cos(x[0])]])                              # noqa: E731  (the one column, broadcast)
        return Pair(name, 2, 1, Jf, Jh, Q, R, P0,
                    lambda: (sm.Pendulum2DTransition(_rv(sm, 2, P0, m0), _rv(sm, 2, Q), dt=dt), sm.Pendulum2DMeasurement(_rv(sm, 1, R), 2)), m0)
    if name in ('vdp_polar', 'vdp_pendulum'):
        Q, P0, m0 = np.array([[0.02, 0.005], [0.005, 0.05]]), np.array([[0.3, 0.1], [0.1, 0.4]]), np.array([1.0, 0.5])
        Dyn = uj.transition('PcrlbVdp', 2, uj.VDP_CODE, uj.VDP_JAC, (VDP_DT, VDP_MU))
        if name == 'vdp_polar':
            R = np.array([[0.04, 0.01], [0.01, 0.02]])
            Obs = uj.measurement('PcrlbPolar', 2, POLAR_CODE, POLAR_JAC)
            return Pair(name, 2, 2, uj.vdp_dx(VDP_DT, VDP_MU), _polar_dx, Q, R, P0,
                        lambda: (Dyn(_rv(sm, 2, P0, m0), _rv(sm, 2, Q)), Obs(_rv(sm, 2, R), 2)), m0)
        R = [[0.01]]
        Jh = lambda x, t: np.array([[np.cos(x[0]), np.cos(x[0])]])                              # noqa: E731
        return Pair(name, 2, 1, uj.vdp_dx(VDP_DT, VDP_MU), Jh, Q, R, P0,
                    lambda: (Dyn(_rv(sm, 2, P0, m0), _rv(sm, 2, Q)), sm.Pendulum2DMeasurement(_rv(sm, 1, R), 2)), m0)
    if name == 'six':
        rng = np.random.default_rng(5)
        a, c = rng.standard_normal((6, 6)), rng.standard_normal((4, 4))
        Q, R, P0 = 0.1 * a.dot(a.T) + 0.2 * np.eye(6), 0.1 * c.dot(c.T) + 0.1 * np.eye(4), 0.5 * np.eye(6) + 0.1
        cd, jd, _, fd_dx = uj.poly_model(6, 6)
        co, jo, _, fo_dx = uj.poly_model(4, 3)
        Dyn, Obs = uj.transition('PcrlbSix', 6, cd, jd), uj.measurement('PcrlbSixMeas', 4, co, jo, dim_substate=3)
        return Pair(name, 6, 4, fd_dx, lambda x, t: uj.place(fo_dx(x[:3], t), 6), Q, R, P0,
                    lambda: (Dyn(_rv(sm, 6, P0), _rv(sm, 6, Q)), Obs(_rv(sm, 4, R), 6)))
    if name == 'time':
        dt, Q, R, P0 = 0.1, np.array([[0.05, 0.0], [0.0, 0.1]]), [[0.25]], np.eye(2)
        Dyn = uj.transition('PcrlbTime', 2, uj.TIME_CODE, uj.TIME_JAC, (dt,))
        Obs = uj.measurement('PcrlbTimeMeas', 1, TMEAS_CODE, TMEAS_JAC, dim_substate=1)
        return Pair(name, 2, 1, uj.time_dx(dt), lambda x, t: np.array([[1.0 + 0.5 * t, 0.0]]), Q, R, P0,
                    lambda: (Dyn(_rv(sm, 2, P0), _rv(sm, 2, Q)), Obs(_rv(sm, 1, R), 2)))
    if name == 'linear':
        Q, R, P0 = np.array([[0.3, 0.1], [0.1, 0.2]]), [[0.5]], np.array([[2.0, 0.3], [0.3, 1.0]])
        Dyn = uj.transition('PcrlbLin', 2, LIN_CODE, LIN_JAC)
        Obs = uj.measurement('PcrlbLinMeas', 1, LIN_MEAS_CODE, LIN_MEAS_JAC)
        return Pair(name, 2, 1, lambda x, t: LIN_F, lambda x, t: LIN_H, Q, R, P0,
                    lambda: (Dyn(_rv(sm, 2, P0), _rv(sm, 2, Q)), Obs(_rv(sm, 1, R), 2)))
    raise KeyError(name)


def states(p, T, B, seed=0):
    """Plausible true states (D, T + 1, B) for a pair: the initial moments, then a bounded random walk (the sums are checked on ANY
    states; the polar measurement is kept away from the origin by the walk's mean)."""
    rng = np.random.default_rng(100 + seed)
    L = np.linalg.cholesky(p.P0)
    x = np.empty((p.D, T + 1, B))
    x[:, 0] = (p.m0 + 1.0)[:, None] + L.dot(rng.standard_normal((p.D, B)))
    for j in range(T):
        x[:, j + 1] = 0.8 * x[:, j] + 0.4 + 0.3 * rng.standard_normal((p.D, B))
    return x
