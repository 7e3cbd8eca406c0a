"""
NumPy restatement of the bootstrap particle filter (csrc/ssmq_particle.hip; include/ssmq.h ssmq_particle_filter_dev states the
recursion) - the oracle of tests/test_particle_host.py and tests/test_particle_gpu.py.

The draws: Philox4x32-10 keyed by the seed, counter = (trajectory lo, hi, step, tag), tag = purpose << 28 | particle << 4 | pair,
Box-Muller as in tests/_mc_oracle.unit_points (pair p gives z[2 p], z[2 p + 1]); purpose 8 the initial particles (step 0), 9 the
process noise of step j, 10 the resampling uniform of step j (particle 0, pair 0).

`resample` and `step` are the one-step forms the GPU test starts from the DEVICE's particles and log-weights; `full_pass` chains
them.  The sums here are NumPy's (pairwise), not the device's butterfly: ancestors and resampling decisions are compared exactly only
where the margins returned here say that no rounding can flip them, everything else under a tolerance.  `dtype=LD` runs the weight and
moment arithmetic in long double (the yardstick of the float64 restatement's own error).
"""
import numpy as np

from tests._bootstrap_oracle import philox4x32_10, M32
from tests._mc_oracle import _cospi_sinpi, cholesky, f_ungm, f_pendulum, f_radar, f_cv, LD

EPS = float(np.finfo(float).eps)
P_INIT, P_NOISE, P_RESAMPLE = 8, 9, 10


def _philox(seed, traj, step, tags):
    """The four output words of every tag in `tags` (uint64 array), as uint64 arrays."""
    tags = np.asarray(tags, dtype=np.uint64)
    full = lambda v: np.full(tags.shape, v, dtype=np.uint64)       # noqa: E731
    o = philox4x32_10((full(traj & M32), full((traj >> 32) & M32), full(step), tags), (seed & M32, (seed >> 32) & M32))
    return [np.asarray(v, dtype=np.uint64) for v in o]


def _u53(hi, lo):
    return (((hi >> np.uint64(5)) << np.uint64(26) | (lo >> np.uint64(6))).astype(np.float64) + 0.5) * 2.0 ** -53


def normals(seed, traj, step, purpose, N, n):
    """(n, N) standard normals of particles 0 .. N-1."""
    z = np.empty((n, N))
    part = np.arange(N, dtype=np.uint64)
    for p in range((n + 1) // 2):
        o = _philox(seed, traj, step, np.uint64(purpose << 28) | (part << np.uint64(4)) | np.uint64(p))
        r = np.sqrt(-2.0 * np.log(_u53(o[0], o[1])))
        cs, sn = _cospi_sinpi(2.0 * _u53(o[2], o[3]))
        z[2 * p] = r * cs
        if 2 * p + 1 < n:
            z[2 * p + 1] = r * sn
    return z


def resampling_uniform(seed, traj, step):
    o = _philox(seed, traj, step, np.array([P_RESAMPLE << 28], dtype=np.uint64))
    return float(_u53(o[0], o[1])[0])


class Model:
    """A pair of models with additive noise as the filter sees it: f (D, N) -> (D, N), h (D, N) -> (Y, N), the process noise
    q_mean + Lq z through the gain G, the measurement noise with mean r_mean and factor Lr of R (the scale matrix with `dof`)."""

    def __init__(self, f, h, D, Y, q_mean, Lq, G, r_mean, Lr, dof=None):
        self.f, self.h, self.D, self.Y = f, h, D, Y
        self.q_mean, self.Lq, self.G = np.asarray(q_mean, float), np.asarray(Lq, float), np.asarray(G, float)
        self.r_mean, self.Lr, self.dof = np.asarray(r_mean, float), np.asarray(Lr, float), dof
        self.dq = self.q_mean.size

    def log_norm(self, dtype=np.float64):
        from math import lgamma, log, pi
        logdet = float(np.sum(np.log(np.diag(self.Lr))))
        if self.dof is None:
            return dtype(-0.5 * self.Y * log(2.0 * pi) - logdet)
        return dtype(lgamma(0.5 * (self.dof + self.Y)) - lgamma(0.5 * self.dof) - 0.5 * self.Y * log(self.dof * pi) - logdet)

    def log_density(self, y, hx, dtype=np.float64):
        """log p(y | h) for every column of hx (Y, N)."""
        res = (np.asarray(y, dtype=dtype)[:, None] - np.asarray(hx, dtype=dtype)) - self.r_mean.astype(dtype)[:, None]
        L = self.Lr.astype(dtype)
        v = np.zeros_like(res)
        for e in range(self.Y):                     # forward substitution
            v[e] = (res[e] - (L[e, :e, None] * v[:e]).sum(axis=0)) / L[e, e]
        d2 = (v * v).sum(axis=0)
        if self.dof is None:
            return self.log_norm(dtype) - d2 / dtype(2)
        return self.log_norm(dtype) - dtype(0.5 * (self.dof + self.Y)) * np.log1p(d2 / dtype(self.dof))


def initial_particles(model, m0, P0, seed, traj, N):
    L = cholesky(np.asarray(P0, dtype=np.float64))
    return np.asarray(m0, float)[:, None] + L.dot(normals(seed, traj, 0, P_INIT, N, model.D))


def moments(x, lwn, dtype=np.float64):
    """fm, fP (second pass around the mean) and ess of the cloud x (D, N) with normalised log-weights lwn."""
    w = np.exp(np.asarray(lwn, dtype=dtype))
    xx = np.asarray(x, dtype=dtype)
    fm = (w * xx).sum(axis=1)
    dx = xx - fm[:, None]
    fP = (w * dx).dot(dx.T)
    return fm, fP, dtype(1) / (w * w).sum()


def resample(lwn, seed, traj, step, ess_threshold):
    """Systematic resampling after step `step` from the normalised log-weights of that step: (ancestors, resampled?, per-particle
    ancestor margin min_m |cdf[m] - p_i|, ESS margin |ess - ess_threshold N| / N) - the margins +inf where nothing is decided."""
    N = lwn.size
    w = np.exp(lwn)
    ess = 1.0 / np.sum(w * w)
    if ess_threshold >= 1.0:
        do, ess_margin = True, np.inf
    elif ess_threshold <= 0.0:
        do, ess_margin = False, np.inf
    else:
        do, ess_margin = bool(ess < ess_threshold * N), abs(ess - ess_threshold * N) / N
    if not do:
        return np.arange(N, dtype=np.int64), False, np.full(N, np.inf), ess_margin
    cdf = np.cumsum(w)
    cdf[-1] = 1.0
    p = (np.arange(N, dtype=np.float64) + resampling_uniform(seed, traj, step)) / float(N)
    anc = np.minimum(np.searchsorted(cdf, p, side='right'), N - 1)
    margin = np.min(np.abs(cdf[None, :] - p[:, None]), axis=1)
    return anc.astype(np.int64), True, margin, ess_margin


def propagate(model, x_prev, anc, seed, traj, j):
    """x_j = f(x_{j-1}[:, anc], j) + G (q_mean + Lq z)."""
    N = x_prev.shape[1]
    q = model.q_mean[:, None] + model.Lq.dot(normals(seed, traj, j, P_NOISE, N, model.dq))
    return model.f(np.ascontiguousarray(x_prev[:, anc]), float(j)) + model.G.dot(q)


def weigh(model, x, lw_prev, y, j, dtype=np.float64):
    """Normalised log-weights and the log-likelihood increment of step j from the (normalised) log-weights the particles carry."""
    lw = np.asarray(lw_prev, dtype=dtype) + model.log_density(y, model.h(x, float(j)), dtype)
    m = np.max(lw)
    if not np.isfinite(m):
        return None, dtype(np.nan)
    ll = m + np.log(np.sum(np.exp(lw - m)))
    return lw - ll, ll


def step(model, x_prev, lwn_prev, y, j, seed, traj, ess_threshold, first=False):
    """Step j from the particles and normalised log-weights of step j - 1 (first: the initial cloud - nothing to resample): dict with
    anc, resampled, anc_margin (N,), ess_margin, x, lwn, fm, fP, ll, ess."""
    N = x_prev.shape[1]
    if first:
        anc, did, am, em = np.arange(N, dtype=np.int64), False, np.full(N, np.inf), np.inf
    else:
        anc, did, am, em = resample(lwn_prev, seed, traj, j - 1, ess_threshold)
    x = propagate(model, x_prev, anc, seed, traj, j)
    carried = np.full(N, -np.log(float(N))) if (did or first) else lwn_prev
    lwn, ll = weigh(model, x, carried, y, j)
    out = dict(anc=anc, resampled=did, anc_margin=am, ess_margin=em, x=x, lwn=lwn, ll=ll)
    if lwn is None:
        out.update(fm=np.full(model.D, np.nan), fP=np.full((model.D, model.D), np.nan), ess=np.nan)
    else:
        out['fm'], out['fP'], out['ess'] = moments(x, lwn)
    return out


def full_pass(model, y, m0, P0, seed, traj, N, ess_threshold):
    """The whole pass of one trajectory, y (Y, T): dict of fm (D, T), fP (D, D, T), ll (T,), ess (T,), x (D, N, T), lwn (N, T), anc (N, T)
    (chosen after each step), resampled (T,), anc_margin (N, T), ess_margin (T,), status."""
    T, D = y.shape[1], model.D
    o = dict(fm=np.full((D, T), np.nan), fP=np.full((D, D, T), np.nan), ll=np.full(T, np.nan), ess=np.full(T, np.nan),
             x=np.full((D, N, T), np.nan), lwn=np.full((N, T), np.nan), anc=np.full((N, T), -1, dtype=np.int64),
             resampled=np.zeros(T, dtype=bool), anc_margin=np.full((N, T), np.inf), ess_margin=np.full(T, np.inf), status=0)
    x, lwn = initial_particles(model, m0, P0, seed, traj, N), np.full(N, -np.log(float(N)))
    for j in range(T):
        s = step(model, x, lwn, y[:, j], j, seed, traj, ess_threshold, first=(j == 0))
        if j > 0:
            o['anc'][:, j - 1], o['resampled'][j - 1] = s['anc'], s['resampled']
            o['anc_margin'][:, j - 1], o['ess_margin'][j - 1] = s['anc_margin'], s['ess_margin']
        if s['lwn'] is None:
            o['status'] = 1 + j
            return o
        x, lwn = s['x'], s['lwn']
        o['fm'][:, j], o['fP'][:, :, j], o['ll'][j], o['ess'][j], o['x'][:, :, j], o['lwn'][:, j] = s['fm'], s['fP'], s['ll'], s['ess'], x, lwn
    o['anc'][:, T - 1], o['resampled'][T - 1], o['anc_margin'][:, T - 1], o['ess_margin'][T - 1] = resample(lwn, seed, traj, T - 1, ess_threshold)
    return o


# ---- the cases of the two test files: B = 5 trajectories, T = 6 steps, ess_threshold = 0.5 -------------------------------------------
B, T, ESS_THRESHOLD, SEED = 5, 6, 0.5, 11
CV_DT = 0.5
CASES = {'ungm': (64, 320), 'cv_radar': (128,), 'pend_t': (64,)}            # name -> particle counts


def _chol(a):
    return np.linalg.cholesky(np.atleast_2d(np.asarray(a, dtype=float)))


def case(name):
    """(Model, m0, P0, keyword arguments that build the package's models)."""
    if name == 'ungm':
        q, r = np.array([[10.0]]), np.array([[1.0]])
        return Model(f_ungm, lambda x, t: 0.05 * x[:1] ** 2, 1, 1, [0.0], _chol(q), np.eye(1), [0.0], _chol(r)), np.zeros(1), np.eye(1), dict(q=q, r=r)
    if name == 'cv_radar':
        q, r = np.diag([0.5, 0.8]), np.array([[4.0, 0.01], [0.01, 1e-3]])
        G = np.array([[CV_DT ** 2 / 2, 0], [CV_DT, 0], [0, CV_DT ** 2 / 2], [0, CV_DT]])
        m0, P0 = np.array([40.0, 2.0, 30.0, -1.0]), np.diag([4.0, 0.5, 4.0, 0.5]) + 0.1
        return (Model(lambda x, t: f_cv(x, t, CV_DT), lambda x, t: f_radar(x, t, (0, 2)), 4, 2, [0.0, 0.0], _chol(q), G, [0.0, 0.0], _chol(r)),
                m0, P0, dict(q=q, r=r))
    if name == 'pend_t':
        dt = 0.01
        q = 0.01 * np.array([[(dt ** 3) / 3, (dt ** 2) / 2], [(dt ** 2) / 2, dt]])
        r, dof = np.array([[0.002]]), 4.0
        m0, P0 = np.array([1.5, 0.0]), 0.05 * np.eye(2)
        return (Model(lambda x, t: f_pendulum(x, t, dt), lambda x, t: np.sin(x[:1]), 2, 1, [0.0, 0.0], _chol(q), np.eye(2), [0.0], _chol(r), dof),
                m0, P0, dict(q=q, r=r, dof=dof, dt=dt))
    raise KeyError(name)


def package_models(name):
    """The package's model objects of a case."""
    from ssmtoybox_amd import ssmod as sm
    model, m0, P0, kw = case(name)
    if name == 'ungm':
        return sm.UNGMTransition(sm.GaussRV(1, m0, P0), sm.GaussRV(1, cov=kw['q'])), sm.UNGMMeasurement(sm.GaussRV(1, cov=kw['r']), 1)
    if name == 'cv_radar':
        return (sm.ConstantVelocity(sm.GaussRV(4, m0, P0), sm.GaussRV(2, cov=kw['q']), dt=CV_DT),
                sm.Radar2DMeasurement(sm.GaussRV(2, cov=kw['r']), 4, state_index=[0, 2]))
    return (sm.Pendulum2DTransition(sm.GaussRV(2, m0, P0), sm.GaussRV(2, cov=kw['q']), dt=kw['dt']),
            sm.Pendulum2DMeasurement(sm.StudentRV(1, scale=kw['r'], dof=kw['dof']), 2))


def case_data(name, seed=SEED):
    """Measurements (Y, T, B) of a case, simulated on the host in the filter's time convention (NumPy's generator: the data only have
    to be plausible)."""
    model, m0, P0, kw = case(name)
    rng = np.random.default_rng(1000 + seed)
    y = np.empty((model.Y, T, B))
    for b in range(B):
        x = m0 + cholesky(np.asarray(P0, float)).dot(rng.standard_normal(model.D))
        for j in range(T):
            x = model.f(x[:, None], float(j))[:, 0] + model.G.dot(model.q_mean + model.Lq.dot(rng.standard_normal(model.dq)))
            noise = model.Lr.dot(rng.standard_normal(model.Y))
            if model.dof is not None:
                noise = noise / np.sqrt(rng.chisquare(model.dof) / model.dof)
            y[:, j, b] = model.h(x[:, None], float(j))[:, 0] + model.r_mean + noise
    return y


# ---- the accuracy study of tests/test_particle_gpu.py::test_better_filter_than_the_ukf, on the CPU -----------------------------------
STUDY = dict(B=256, T=20, N=512, seed=11)


def study_cpu(seed, aligned=True, B=STUDY['B'], T=STUDY['T'], N=STUDY['N']):
    """Per-trajectory time-averaged RMSE (B,) of this oracle's full pass and of the UnscentedKalman of oracle/ssmq_oracle.py on UNGM
    data of the device simulator's restatement (the same counters as `ssmod.simulate_dev`).  The simulator's convention is
    x[0] ~ init, x[k] = f(x[k-1], k-1); the filters' is x_{-1} ~ init, x_j = f(x_{j-1}, j).  aligned: T + 1 steps are simulated and
    the filters get y[1:], scored against x[1:] - then x_j = x[j + 1] follows the filters' model exactly; else the raw T steps."""
    from oracle import ssmq_oracle as orc
    model, m0, P0, kw = case('ungm')
    pts, (wm, wc) = orc.points_ut(1), orc.weights_ut(1)
    tf_d = lambda m, P, t: orc.apply_sigma(orc.F_UNGM_DYN, m, P, t, pts, wm, wc)       # noqa: E731
    tf_o = lambda m, P, t: orc.apply_sigma(orc.F_UNGM_MEAS, m, P, t, pts, wm, wc)      # noqa: E731
    x, y = orc.simulate(orc.F_UNGM_DYN, orc.F_UNGM_MEAS, T + (1 if aligned else 0), B, m0, P0, np.zeros(1), kw['q'], np.zeros(1), kw['r'],
                        seed=seed)
    if aligned:
        x, y = x[:, 1:], y[:, 1:]
    r_pf, r_ukf = np.empty(B), np.empty(B)
    for b in range(B):
        o = full_pass(model, y[:, :, b], m0, P0, seed, b, N, ESS_THRESHOLD)
        fm = orc.gaussian_filter(y[:, :, b], m0, P0, kw['q'], kw['r'], np.eye(1), tf_d, tf_o)[0]
        r_pf[b] = np.sqrt(np.mean((x[0, :, b] - o['fm'][0]) ** 2))
        r_ukf[b] = np.sqrt(np.mean((x[0, :, b] - fm[0]) ** 2))
    return r_pf, r_ukf


def bootstrap_se(d, samples=2000, seed=0):
    """Bootstrap standard error of the mean of d (resampling trajectories with replacement)."""
    rng = np.random.default_rng(seed)
    return float(np.std([d[rng.integers(0, d.size, d.size)].mean() for _ in range(samples)]))
