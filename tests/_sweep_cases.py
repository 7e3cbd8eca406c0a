"""The cases of the likelihood-sweep tests, built without a device: the models (ssmod is plain Python), what the oracle needs of
them, the parameter grids and the measurements (simulated with the oracle's integrands).  The filter object of a case needs the
device (its constructor computes weights there): `make_filter`."""
import numpy as np

from oracle import ssmq_oracle as orc
from tests import _sweep_oracle as swo

# case 1's grid, alpha = 1, the same row for both transforms.  On ell in {0.1, 0.3, 1, 3, 10, 30} the oracle's likelihood table
# of the case rises to the last point (-8779.8, -4264.2, -2064.0, -1965.7, -1756.4, -1745.5: no interior maximum), and ell = 100
# gives -1992.0: the grid is that one moved up by one point.  Maximum at ell = 30, runner-up ell = 10, margin 10.9
# (tests/test_sweep_host.py asserts both).
UNGM_ELLS = (0.3, 1.0, 3.0, 10.0, 30.0, 100.0)
# a row whose kernel matrix is not positive definite (ell = 0: 0 / 0 on the diagonal of K); tests/test_sweep_host.py checks that the
# weights oracle fails on it
BAD_ROW = np.array([1.0, 0.0])


def models(name):
    from ssmtoybox_amd import ssmod as sm
    if name == 'ungm_gp':
        return (sm.UNGMTransition(sm.GaussRV(1), sm.GaussRV(1, cov=np.array([[10.0]]))), sm.UNGMMeasurement(sm.GaussRV(1), 1))
    if name == 'pend_bs':
        Q = 0.01 * np.array([[0.01 ** 3 / 3, 0.01 ** 2 / 2], [0.01 ** 2 / 2, 0.01]])
        return (sm.Pendulum2DTransition(sm.GaussRV(2, np.array([1.5, 0.0]), 0.01 * np.eye(2)), sm.GaussRV(2, cov=Q)),
                sm.Pendulum2DMeasurement(sm.GaussRV(1, cov=np.array([[0.1]])), 2))
    if name == 'reentry_gp':
        m0 = np.array([6500.4, 349.14, -1.8093, -6.7967, 0.6932])
        return (sm.ReentryVehicle2DTransition(sm.GaussRV(5, m0, np.diag([1e-6, 1e-6, 1e-6, 1e-6, 1.0])),
                                              sm.GaussRV(3, cov=np.diag([2.4064e-5, 2.4064e-5, 1e-6]))),
                sm.Radar2DMeasurement(sm.GaussRV(2, cov=np.diag([1e-6, 0.17e-3 ** 2])), 5, radar_loc=np.array([6374.0, 0.0])))
    raise KeyError(name)


# name -> (kind, B, T, grid of [alpha, ell ...] rows)
SHAPES = {
    'ungm_gp': ('gp', 70, 6, np.array([[1.0, e] for e in UNGM_ELLS])),
    'pend_bs': ('bs', 5, 4, np.array([[1.0, 1.0, 1.0], [1.0, 2.0, 2.0], [1.0, 3.0, 2.5]])),
    'reentry_gp': ('gp', 5, 4, np.array([[1.0] + [5.0] * 5, [1.0] + [10.0] * 5, [1.0, 5.0, 5.0, 10.0, 10.0, 30.0]])),
}
_CASES = {}


def case(name):
    """dict for swo.sweep plus y (Y, T, B), par (P, 1 + D), B, T - built once, never modified."""
    if name in _CASES:
        return _CASES[name]
    from ssmtoybox_amd import mtran
    dyn, obs = models(name)
    kind, B, T, par = SHAPES[name]
    fd, _ = mtran.resolve_integrand(dyn.dyn_eval)
    fo, _ = mtran.resolve_integrand(obs.meas_eval)
    D = dyn.dim_state
    m0, P0 = dyn.init_rv.get_stats()
    c = dict(kind=kind, fid_dyn=fd.id, p_dyn=tuple(fd.par[i] for i in range(fd.n_par)), fid_obs=fo.id,
             p_obs=tuple(fo.par[i] for i in range(fo.n_par)), sidx=tuple(fo.idx[i] for i in range(fo.n_idx)) if fo.n_idx else None,
             pts=orc.points_ut(D), mulind=np.hstack((np.zeros((D, 1), dtype=int), np.eye(D, dtype=int), 2 * np.eye(D, dtype=int))),
             m0=np.asarray(m0, dtype=float), P0=np.asarray(P0, dtype=float), Q=np.atleast_2d(dyn.noise_rv.get_stats()[1]),
             G=np.asarray(dyn.noise_gain, dtype=float), R=np.atleast_2d(obs.noise_rv.get_stats()[1]), B=B, T=T, par=par, name=name)
    rng = np.random.default_rng(3)
    Y = c['R'].shape[0]
    Gq, L0, Lr = c['G'].dot(np.linalg.cholesky(c['Q'])), np.linalg.cholesky(c['P0']), np.linalg.cholesky(c['R'])
    y = np.zeros((Y, T, B))
    for b in range(B):
        x = c['m0'] + L0.dot(rng.standard_normal(D))
        for k in range(T):
            x = orc.integrand(c['fid_dyn'], x, float(k), c['p_dyn']) + Gq.dot(rng.standard_normal(Gq.shape[1]))
            y[:, k, b] = orc.integrand(c['fid_obs'], x if c['sidx'] is None else x[list(c['sidx'])], float(k), c['p_obs']) + \
                Lr.dot(rng.standard_normal(Y))
    c['y'] = y
    _CASES[name] = c
    return c


_REFS = {}


def reference(name):
    """The oracle's sweep of the case, computed once."""
    if name not in _REFS:
        c = case(name)
        _REFS[name] = swo.sweep(c, c['y'], c['par'], c['par'])
    return _REFS[name]


def make_filter(name, par_dyn, par_obs):
    """The case's filter with ONE parameter row per transform (needs the device)."""
    from ssmtoybox_amd import ssinf
    dyn, obs = models(name)
    c = case(name)
    if c['kind'] == 'bs':
        return ssinf.BayesSardKalman(dyn, obs, np.atleast_2d(par_dyn), np.atleast_2d(par_obs), mulind_dyn=c['mulind'], mulind_obs=c['mulind'])
    return ssinf.GaussianProcessKalman(dyn, obs, np.atleast_2d(par_dyn), np.atleast_2d(par_obs), 'rbf', 'ut')
