"""
Golden vectors for user-defined models (device_code, include/ssmq.h ssmq_integrand_define): the reference's filters and
transforms run on its own NumPy subclasses of TransitionModel / MeasurementModel with the same formulas that
tests/test_user_models_gpu.py gives this build as device code.  Reuses the import shims of make_golden.py (importing that
module installs them and loads the reference).

Run:  PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python tests/golden/make_golden_user.py      -> tests/golden/g15_user_models.npz

Models (state x, additive noise):
  vdp   2-D Van der Pol, Euler step:  x0' = x0 + dt x1,  x1' = x1 + dt (mu (1 - x0^2) x1 - x0);  par (dt, mu)
  vdpm  scalar measurement y = x0 + 0.5 sin(x1)
  cpl   4-D pair of coupled damped pendulums [a1, w1, a2, w2], Euler step, par (dt, c, k):
        a1' = a1 + dt w1,  w1' = w1 + dt (-sin a1 - c w1 + k (a2 - a1)),  a2' = a2 + dt w2,  w2' = w2 + dt (-sin a2 - c w2 + k (a1 - a2))
  cplm  two measurements y = [sin a1 + 0.5 a2, 0.5 a1 + sin a2]
Filters (T = 50 steps, 8 trajectories): UKF, CKF, GPQKF ('ut'), BSQKF, TPQKF and FullySymmetricStudent; one
UnscentedTransform.apply and one GaussianProcessTransform.apply per model function on 8 random inputs.  Filtered covariances
are stored as their lower triangles (`<system>_<filter>_fcl`, np.tril_indices order); filtered means and covariances are rounded
to 32 mantissa bits (round32), so that the file stays under 300 kB.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.golden import make_golden as mg  # noqa: E402  (installs the shims, imports the reference)
from ssmtoybox import ssmod, ssinf  # noqa: E402
from ssmtoybox.mtran import UnscentedTransform  # noqa: E402
from ssmtoybox.bq.bqmtran import GaussianProcessTransform  # noqa: E402
from ssmtoybox.utils import GaussRV, StudentRV  # noqa: E402

STEPS, SEEDS, N_IN = 50, 8, 8
VDP_PAR = (0.1, 1.0)          # dt, mu
CPL_PAR = (0.05, 0.2, 0.5)    # dt, c, k


class VanDerPol(ssmod.TransitionModel):
    dim_state, dim_noise, noise_additive = 2, 2, True

    def __init__(self, init_rv, noise_rv):
        super().__init__(init_rv, noise_rv)
        self.dt, self.mu = VDP_PAR

    def dyn_fcn(self, x, q, time):
        return np.array([x[0] + self.dt * x[1], x[1] + self.dt * (self.mu * (1.0 - x[0] * x[0]) * x[1] - x[0])]) + q

    def dyn_fcn_cont(self, x, q, time):
        return None

    def dyn_fcn_dx(self, x, q, time):
        return None


class VdPMeasurement(ssmod.MeasurementModel):
    dim_substate, dim_out, dim_noise, noise_additive = 2, 1, 1, True

    def __init__(self, noise_rv, dim_state, state_index=None):
        super().__init__(noise_rv, dim_state, state_index)

    def meas_fcn(self, x, r, time):
        return np.array([x[0] + 0.5 * np.sin(x[1])]) + r

    def meas_fcn_dx(self, x, r, time):
        return None


class CoupledPendulums(ssmod.TransitionModel):
    dim_state, dim_noise, noise_additive = 4, 4, True

    def __init__(self, init_rv, noise_rv):
        super().__init__(init_rv, noise_rv)
        self.dt, self.c, self.k = CPL_PAR

    def dyn_fcn(self, x, q, time):
        dt, c, k = self.dt, self.c, self.k
        return np.array([x[0] + dt * x[1], x[1] + dt * (-np.sin(x[0]) - c * x[1] + k * (x[2] - x[0])),
                         x[2] + dt * x[3], x[3] + dt * (-np.sin(x[2]) - c * x[3] + k * (x[0] - x[2]))]) + q

    def dyn_fcn_cont(self, x, q, time):
        return None

    def dyn_fcn_dx(self, x, q, time):
        return None


class CoupledMeasurement(ssmod.MeasurementModel):
    dim_substate, dim_out, dim_noise, noise_additive = 4, 2, 2, True

    def __init__(self, noise_rv, dim_state, state_index=None):
        super().__init__(noise_rv, dim_state, state_index)

    def meas_fcn(self, x, r, time):
        return np.array([np.sin(x[0]) + 0.5 * x[2], 0.5 * x[0] + np.sin(x[2])]) + r

    def meas_fcn_dx(self, x, r, time):
        return None


# (m0, P0, Q, R) of each system; the Student filter uses the same matrices as scale matrices
SYSTEMS = {
    'vdp': (VanDerPol, VdPMeasurement, np.array([1.0, 0.0]), 0.1 * np.eye(2), 1e-3 * np.eye(2), np.array([[0.01]])),
    'cpl': (CoupledPendulums, CoupledMeasurement, np.array([0.5, 0.0, -0.3, 0.0]), 0.05 * np.eye(4), 1e-4 * np.eye(4),
            0.01 * np.eye(2)),
}
ELL = {'vdp': 2.0, 'cpl': 2.0}


def round32(a):
    """fp64 values rounded to 32 mantissa bits (relative error <= 2^-33 = 1.2e-10, far inside the 1e-8 / 5e-9 bars the filter
    results are held to): the zeroed low bytes compress, which keeps the fixture under 300 kB."""
    u = np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)
    drop = np.uint64(52 - 32)
    u = (u + (np.uint64(1) << (drop - np.uint64(1)))) & ~((np.uint64(1) << drop) - np.uint64(1))
    return u.view(np.float64)


def filters(dyn, obs, D, ell):
    par = np.array([[1.0] + [ell] * D])
    mi = np.hstack((np.zeros((D, 1)), np.eye(D), 2 * np.eye(D))).astype(int)
    return {
        'ukf': ssinf.UnscentedKalman(dyn, obs),
        'ckf': ssinf.CubatureKalman(dyn, obs),
        'gpqkf': ssinf.GaussianProcessKalman(dyn, obs, par, par, 'rbf', 'ut'),
        'bsqkf': ssinf.BayesSardKalman(dyn, obs, par, par, mi, mi, 'ut'),
        'tpqkf': ssinf.StudentProcessKalman(dyn, obs, par, par, 'rbf', 'ut'),
    }


def main():
    out = {}
    rng = np.random.default_rng(20261016)
    for tag, (Dyn, Obs, m0, P0, Q, R) in SYSTEMS.items():
        D, Y = m0.shape[0], R.shape[0]
        dyn, obs = Dyn(GaussRV(D, m0, P0), GaussRV(D, cov=Q)), Obs(GaussRV(Y, cov=R), D)
        np.random.seed(1000 + D)
        x = dyn.simulate_discrete(STEPS, SEEDS)
        y = obs.simulate_measurements(x)
        out[tag + '_y'], out[tag + '_m0'], out[tag + '_P0'], out[tag + '_Q'], out[tag + '_R'] = y, m0, P0, Q, R
        algs = filters(dyn, obs, D, ELL[tag])
        sdyn = Dyn(StudentRV(D, m0, P0, 1000.0), StudentRV(D, scale=Q, dof=1000.0))
        sobs = Obs(StudentRV(Y, scale=R, dof=4.0), D)
        algs['fss'] = ssinf.FullySymmetricStudent(sdyn, sobs)
        for name, alg in algs.items():
            fm, fc = np.zeros((D, STEPS, SEEDS)), np.zeros((D, D, STEPS, SEEDS))
            for s in range(SEEDS):
                fm[..., s], fc[..., s] = alg.forward_pass(y[..., s])
                alg.reset()
            # covariances as their lower triangles (np.tril_indices order; the file stays small): (D (D + 1) / 2, T, seeds)
            out['{}_{}_fm'.format(tag, name)], out['{}_{}_fcl'.format(tag, name)] = round32(fm), round32(fc[np.tril_indices(D)])
            print(tag, name, 'ok', float(np.abs(fm).max()))
        # one sigma-point and one GP-quadrature transform per model function
        for fname, model, f, din, dout in ((tag + '_dyn', dyn, dyn.dyn_eval, D, D), (tag + '_meas', obs, obs.meas_eval, D, Y)):
            means, covs = mg.random_inputs(rng, m0, np.sqrt(np.diag(P0)), N_IN)
            out[fname + '_mean'], out[fname + '_cov'] = means, covs
            par = np.array([[1.0] + [ELL[tag]] * din])
            for tname, tf in (('ut', UnscentedTransform(din)), ('gpq', GaussianProcessTransform(din, dout, par, 'rbf', 'ut'))):
                mf, cf, cfx = np.zeros((N_IN, dout)), np.zeros((N_IN, dout, dout)), np.zeros((N_IN, dout, din))
                for i in range(N_IN):
                    mf[i], cf[i], cfx[i] = tf.apply(f, means[i], covs[i], np.atleast_1d(0))
                key = '{}_{}'.format(fname, tname)
                out[key + '_mf'], out[key + '_cf'], out[key + '_cfx'] = mf, cf, cfx
                if tname == 'gpq':
                    out[key + '_wm'], out[key + '_Wc'], out[key + '_Wcc'] = tf.wm, tf.Wc, tf.Wcc
                    out[key + '_pts'], out[key + '_mv'] = tf.model.points, np.float64(tf.model.model_var)
    mg.save('g15_user_models', **out)


if __name__ == '__main__':
    main()
