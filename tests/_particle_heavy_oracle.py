"""
NumPy restatement of the bootstrap particle filter and its marginal smoother with a Student-t initial state and process noise
(csrc/ssmq_particle.hip k_particle_filter<D, QK=1>, csrc/ssmq_particle_smooth.hip k_particle_smooth<D, QK=1>; include/ssmq.h
ssmq_particle_filter_rv_dev states both) - the oracle of tests/test_particle_heavy_host.py and tests/test_particle_heavy_gpu.py.  It
extends tests/_particle_oracle.py, which it imports unchanged: the normals, the resampling, the weights and the moments are that
module's.

A Student-t draw is mean + L z / sqrt(u), u ~ Gamma(nu / 2, scale 2 / nu).  z comes from the counters of the Gaussian filter (purposes
8 and 9); u by Marsaglia-Tsang (gamma_mt_tags of csrc/ssmq_rng.h), one per particle and draw: attempt t = 0 .. 15 sits in the low four
bits of the tag, purpose 11 its normal and 12 its uniform for the initial particle (step 0), 13 and 14 for the process noise of step j.
`gamma_tags` returns, with the variates, the margin by which every acceptance it made or refused was decided.
"""
import numpy as np

from tests import _particle_oracle as po
from tests import _particle_smoother_oracle as so
from tests._mc_oracle import _cospi_sinpi, cholesky, f_ungm, f_pendulum, f_radar, f_cv, LD

EPS = po.EPS
P_INIT_GN, P_INIT_GU, P_NOISE_GN, P_NOISE_GU = 11, 12, 13, 14


def gamma_tags(seed, traj, step, purpose_normal, purpose_uniform, N, shape):
    """Gamma(shape, 1), shape >= 1, of particles 0 .. N-1: (g (N,), margin (N,)) - margin the smallest |log u - bound| and |v| over the
    attempts the particle went through."""
    d = shape - 1.0 / 3.0
    c = 1.0 / np.sqrt(9.0 * d)
    part = np.arange(N, dtype=np.uint64)
    v = np.ones(N)
    done = np.zeros(N, dtype=bool)
    margin = np.full(N, np.inf)
    for t in range(16):
        o = po._philox(seed, traj, step, np.uint64(purpose_normal << 28) | (part << np.uint64(4)) | np.uint64(t))
        r = np.sqrt(-2.0 * np.log(po._u53(o[0], o[1])))
        x = r * _cospi_sinpi(2.0 * po._u53(o[2], o[3]))[0]
        o = po._philox(seed, traj, step, np.uint64(purpose_uniform << 28) | (part << np.uint64(4)) | np.uint64(t))
        u = po._u53(o[0], o[1])
        w = 1.0 + c * x
        vt = w * w * w
        with np.errstate(invalid='ignore', divide='ignore'):
            bound = 0.5 * x * x + d - d * vt + d * np.log(vt)
            ok = (vt > 0.0) & (np.log(u) < bound)
            m = np.where(vt > 0.0, np.minimum(np.abs(np.log(u) - bound), np.abs(vt)), np.abs(vt))
        live = ~done
        margin[live] = np.minimum(margin[live], m[live])
        fallback = np.where(np.abs(vt) > 0.0, np.abs(vt), 1.0)
        v[live] = np.where(ok[live], vt[live], fallback[live])
        done |= ok
        if done.all():
            break
    return d * v, margin


def t_factor(seed, traj, step, purposes, N, nu):
    """1 / sqrt(u), u ~ Gamma(nu / 2, scale 2 / nu), per particle; (factor, margin)."""
    g, margin = gamma_tags(seed, traj, step, purposes[0], purposes[1], N, 0.5 * nu)
    return 1.0 / np.sqrt(g * (2.0 / nu)), margin


class Model(po.Model):
    """`po.Model` with the degrees of freedom of the initial state (nu0) and of the process noise (nuq); None: Gaussian.  For a
    Student-t side P0 / Lq are the scale matrix and its factor."""

    def __init__(self, *args, nu0=None, nuq=None, **kw):
        super().__init__(*args, **kw)
        self.nu0, self.nuq = nu0, nuq


def initial_particles(model, m0, P0, seed, traj, N, with_margin=False):
    L = cholesky(np.asarray(P0, dtype=np.float64))
    s = L.dot(po.normals(seed, traj, 0, po.P_INIT, N, model.D))
    margin = np.full(N, np.inf)
    if model.nu0 is not None:
        sc, margin = t_factor(seed, traj, 0, (P_INIT_GN, P_INIT_GU), N, model.nu0)
        s = s * sc
    x = np.asarray(m0, float)[:, None] + s
    return (x, margin) if with_margin else x


def propagate(model, x_prev, anc, seed, traj, j, with_margin=False):
    """x_j = f(x_{j-1}[:, anc], j) + G (q_mean + Lq z / sqrt(u))."""
    N = x_prev.shape[1]
    s = model.Lq.dot(po.normals(seed, traj, j, po.P_NOISE, N, model.dq))
    margin = np.full(N, np.inf)
    if model.nuq is not None:
        sc, margin = t_factor(seed, traj, j, (P_NOISE_GN, P_NOISE_GU), N, model.nuq)
        s = s * sc
    x = model.f(np.ascontiguousarray(x_prev[:, anc]), float(j)) + model.G.dot(model.q_mean[:, None] + s)
    return (x, margin) if with_margin else x


def step(model, x_prev, lwn_prev, y, j, seed, traj, ess_threshold, first=False):
    """`po.step` with this module's `propagate`; adds gamma_margin (N,)."""
    N = x_prev.shape[1]
    if first:
        anc, did, am, em = np.arange(N, dtype=np.int64), False, np.full(N, np.inf), np.inf
    else:
        anc, did, am, em = po.resample(lwn_prev, seed, traj, j - 1, ess_threshold)
    x, gm = propagate(model, x_prev, anc, seed, traj, j, with_margin=True)
    carried = np.full(N, -np.log(float(N))) if (did or first) else lwn_prev
    lwn, ll = po.weigh(model, x, carried, y, j)
    out = dict(anc=anc, resampled=did, anc_margin=am, ess_margin=em, gamma_margin=gm, x=x, lwn=lwn, ll=ll)
    if lwn is None:
        out.update(fm=np.full(model.D, np.nan), fP=np.full((model.D, model.D), np.nan), ess=np.nan)
    else:
        out['fm'], out['fP'], out['ess'] = po.moments(x, lwn)
    return out


def full_pass(model, y, m0, P0, seed, traj, N, ess_threshold):
    """`po.full_pass` with this module's draws; adds gamma_margin, the smallest margin of any Gamma acceptance of the pass."""
    T, D = y.shape[1], model.D
    o = dict(fm=np.full((D, T), np.nan), fP=np.full((D, D, T), np.nan), ll=np.full(T, np.nan), ess=np.full(T, np.nan),
             x=np.full((D, N, T), np.nan), lwn=np.full((N, T), np.nan), anc=np.full((N, T), -1, dtype=np.int64),
             resampled=np.zeros(T, dtype=bool), anc_margin=np.full((N, T), np.inf), ess_margin=np.full(T, np.inf), status=0)
    (x, gm), lwn = initial_particles(model, m0, P0, seed, traj, N, with_margin=True), np.full(N, -np.log(float(N)))
    o['gamma_margin'] = float(gm.min())
    for j in range(T):
        s = step(model, x, lwn, y[:, j], j, seed, traj, ess_threshold, first=(j == 0))
        o['gamma_margin'] = min(o['gamma_margin'], float(s['gamma_margin'].min()))
        if j > 0:
            o['anc'][:, j - 1], o['resampled'][j - 1] = s['anc'], s['resampled']
            o['anc_margin'][:, j - 1], o['ess_margin'][j - 1] = s['anc_margin'], s['ess_margin']
        if s['lwn'] is None:
            o['status'] = 1 + j
            return o
        x, lwn = s['x'], s['lwn']
        o['fm'][:, j], o['fP'][:, :, j], o['ll'][j], o['ess'][j], o['x'][:, :, j], o['lwn'][:, j] = s['fm'], s['fP'], s['ll'], s['ess'], x, lwn
    o['anc'][:, T - 1], o['resampled'][T - 1], o['anc_margin'][:, T - 1], o['ess_margin'][T - 1] = po.resample(lwn, seed, traj, T - 1, ess_threshold)
    return o


# ---- the marginal smoother with the Student-t transition density ---------------------------------------------------------------------
def marginal(model, x, lwn, T, dtype=np.float64):
    """`so.marginal` with log p(x' | x) = const - (nuq + D) / 2 log1p(d2 / nuq) in place of -d2 / 2 (Gaussian process noise: so.marginal
    itself); dtype=LD is the long-double twin."""
    if model.nuq is None:
        return so.marginal(model, x, lwn, T, dtype)
    D, N = x.shape[0], x.shape[1]
    o = dict(ls=np.empty((N, T), dtype=dtype), ls_raw=np.empty((N, T), dtype=dtype), sm=np.empty((D, T), dtype=dtype),
             sP=np.empty((D, D, T), dtype=dtype), ess=np.empty(T, dtype=dtype))
    ls = np.asarray(lwn[:, T - 1], dtype=dtype)
    o['ls'][:, T - 1] = o['ls_raw'][:, T - 1] = ls
    nu, hk = dtype(model.nuq), dtype(model.nuq + D) / dtype(2)
    for k in range(T - 2, -1, -1):
        lw = np.asarray(lwn[:, k], dtype=dtype)
        cost = hk * np.log1p(so.pair_distances(model, x[:, :, k], x[:, :, k + 1], k, dtype) / nu)
        lv = so.lse(lw[:, None] - cost, axis=0)
        with np.errstate(invalid='ignore'):
            term = np.where(np.isfinite(lv) & np.isfinite(ls), ls - lv, -np.inf)
        raw = lw + so.lse(term[None, :] - cost, axis=1)
        ls = raw - so.lse(raw, axis=0)
        o['ls_raw'][:, k], o['ls'][:, k] = raw, ls
    for k in range(T):
        o['sm'][:, k], o['sP'][:, :, k], o['ess'][k] = po.moments(x[:, :, k], o['ls'][:, k], dtype)
    return o


# ---- the cases: B = 5 trajectories, T = 6 steps, ess_threshold = 0.5 -----------------------------------------------------------------
B, T, ESS_THRESHOLD = po.B, po.T, po.ESS_THRESHOLD
CASES = {'ungm_t': (64, 320), 'pend_tq': (64,), 'cv_radar_t': (128,)}       # name -> particle counts
METHODS = {'ungm_t': ('marginal', 'genealogy'), 'pend_tq': ('marginal', 'genealogy'), 'cv_radar_t': ('genealogy',)}
# the seed of each case: the first of 11, 1, 2, .. at which tests/test_particle_heavy_host.py::test_oracle_cases_are_decidable holds
SEEDS = {'ungm_t': 11, 'pend_tq': 11, 'cv_radar_t': 11}


def case(name):
    """(Model, m0, P0 - the scale matrix for a Student-t initial state -, keyword arguments that build the package's models)."""
    if name == 'ungm_t':
        q, r = np.array([[10.0]]), np.array([[1.0]])
        return (Model(f_ungm, lambda x, t: 0.05 * x[:1] ** 2, 1, 1, [0.0], po._chol(q), np.eye(1), [0.0], po._chol(r), 4.0, nu0=4.0, nuq=4.0),
                np.zeros(1), np.eye(1), dict(q=q, r=r, dof=4.0))
    if name == 'pend_tq':
        dt = 0.01
        q = 0.01 * np.array([[(dt ** 3) / 3, (dt ** 2) / 2], [(dt ** 2) / 2, dt]])
        r = np.array([[0.002]])
        m0, P0 = np.array([1.0, 0.0]), 0.05 * np.eye(2)        # (away from sin's maximum: the measurement tells the angle, steps resample)
        return (Model(lambda x, t: f_pendulum(x, t, dt), lambda x, t: np.sin(x[:1]), 2, 1, [0.0, 0.0], po._chol(q), np.eye(2), [0.0], po._chol(r),
                      nuq=3.0), m0, P0, dict(q=q, r=r, dt=dt, dof=3.0))
    if name == 'cv_radar_t':
        q, r = np.diag([0.5, 0.8]), np.array([[4.0, 0.01], [0.01, 1e-3]])
        G = np.array([[po.CV_DT ** 2 / 2, 0], [po.CV_DT, 0], [0, po.CV_DT ** 2 / 2], [0, po.CV_DT]])
        m0, P0 = np.array([40.0, 2.0, 30.0, -1.0]), np.diag([4.0, 0.5, 4.0, 0.5]) + 0.1
        return (Model(lambda x, t: f_cv(x, t, po.CV_DT), lambda x, t: f_radar(x, t, (0, 2)), 4, 2, [0.0, 0.0], po._chol(q), G, [0.0, 0.0],
                      po._chol(r), nu0=5.0, nuq=5.0), m0, P0, dict(q=q, r=r, dof=5.0))
    raise KeyError(name)


def package_models(name):
    """The package's model objects of a case."""
    from ssmtoybox_amd import ssmod as sm
    model, m0, P0, kw = case(name)
    if name == 'ungm_t':
        return (sm.UNGMTransition(sm.StudentRV(1, m0, P0, dof=4.0), sm.StudentRV(1, scale=kw['q'], dof=4.0)),
                sm.UNGMMeasurement(sm.StudentRV(1, scale=kw['r'], dof=4.0), 1))
    if name == 'pend_tq':
        return (sm.Pendulum2DTransition(sm.GaussRV(2, m0, P0), sm.StudentRV(2, scale=kw['q'], dof=3.0), dt=kw['dt']),
                sm.Pendulum2DMeasurement(sm.GaussRV(1, cov=kw['r']), 2))
    return (sm.ConstantVelocity(sm.StudentRV(4, m0, P0, dof=5.0), sm.StudentRV(2, scale=kw['q'], dof=5.0), dt=po.CV_DT),
            sm.Radar2DMeasurement(sm.GaussRV(2, cov=kw['r']), 4, state_index=[0, 2]))


def case_data(name):
    """Measurements (Y, T, B) of a case, simulated on the host in the filter's time convention with the case's own heavy tails (NumPy's
    generator: the data only have to be plausible)."""
    model, m0, P0, kw = case(name)
    rng = np.random.default_rng(1000 + SEEDS[name])

    def draw(L, nu):
        v = L.dot(rng.standard_normal(L.shape[1]))
        return v if nu is None else v / np.sqrt(rng.chisquare(nu) / nu)

    y = np.empty((model.Y, T, B))
    for b in range(B):
        x = m0 + draw(cholesky(np.asarray(P0, float)), model.nu0)
        for j in range(T):
            x = model.f(x[:, None], float(j))[:, 0] + model.G.dot(model.q_mean + draw(model.Lq, model.nuq))
            y[:, j, b] = model.h(x[:, None], float(j))[:, 0] + model.r_mean + draw(model.Lr, model.dof)
    return y


# ---- the accuracy study of tests/test_particle_heavy_gpu.py::test_study, on the CPU --------------------------------------------------
STUDY = dict(B=256, T=20, N=512)
# seed 11, the first of 11, 1, 2 tried (tests/test_particle_heavy_host.py::test_study_gap_on_the_cpu): competitor -> (its RMSE, the
# particle filter's, the gap, the bootstrap standard error of the gap).  The GPU test asserts the inequality against the competitors
# that lose by at least 5 standard errors: FullySymmetricStudent (17.5); the Gaussian-noise particle filter with matched covariances
# (2.0) is reported, not asserted.
STUDY_SEED = 11
STUDY_FIGURES = {'fss': (11.0942, 5.7030, 5.3913, 0.3077), 'pf_gauss': (5.9054, 5.7030, 0.2024, 0.1021)}
STUDY_LOSERS = ('fss',)


def study_cpu(seed, B=STUDY['B'], T=STUDY['T'], N=STUDY['N']):
    """Per-trajectory time-averaged RMSE (B,) on Student-t UNGM data (the `ungm_t` noises) of the device simulator's restatement,
    aligned with the filters' time convention (T + 1 steps, the first dropped - `po.study_cpu`), of three filters: 'pf' this oracle's
    particle filter; 'fss' the Studentian filter of oracle/ssmq_oracle.py (fully-symmetric rule, dof 4); 'pf_gauss' the Gaussian-noise
    particle filter of tests/_particle_oracle.py given the matched covariances nu / (nu - 2) times the scale matrices."""
    from oracle import ssmq_oracle as orc
    model, m0, P0, kw = case('ungm_t')
    nu = 4.0
    x, y = orc.simulate_rv(orc.F_UNGM_DYN, orc.F_UNGM_MEAS, T + 1, B, orc.student_rv(m0, P0, nu), orc.student_rv(np.zeros(1), kw['q'], nu),
                           orc.student_rv(np.zeros(1), kw['r'], nu), seed=seed)
    x, y = x[:, 1:], y[:, 1:]
    f = nu / (nu - 2.0)
    gauss = po.Model(model.f, model.h, 1, 1, [0.0], po._chol(f * kw['q']), np.eye(1), [0.0], po._chol(f * kw['r']))
    # the Studentian filter as tests/test_oracle_golden.py::test_student_filters builds it for g5_student, at dof 4
    sc = orc.student_scale_sequence(T, 1, nu, nu, nu)
    pts, w = orc.points_fs(1, 3, None, nu), orc.weights_fs(1, 3, None, nu)
    tfd = lambda m, P, t: orc.apply_sigma(orc.F_UNGM_DYN, m, P, t, pts, w, w)          # noqa: E731
    tfo = lambda m, P, t: orc.apply_sigma(orc.F_UNGM_MEAS, m, P, t, pts, w, w)         # noqa: E731
    out = {k: np.empty(B) for k in ('pf', 'fss', 'pf_gauss')}
    for b in range(B):
        o = full_pass(model, y[:, :, b], m0, P0, seed, b, N, ESS_THRESHOLD)
        g = po.full_pass(gauss, y[:, :, b], m0, f * P0, seed, b, N, ESS_THRESHOLD)
        fm = orc.student_filter(y[:, :, b], m0, np.atleast_2d(P0), kw['q'], kw['r'], np.eye(1), tfd, tfo, sc, dof=nu)[0]
        for k, est in (('pf', o['fm'][0]), ('pf_gauss', g['fm'][0]), ('fss', fm[0])):
            out[k][b] = np.sqrt(np.mean((x[0, :, b] - est) ** 2))
    return out
