"""
Generate tests/golden/g21_taylor_gpqd.npz by running the REFERENCE's TaylorGPQDTransform (mtran.py:668-701) and its filter
ExtendedKalmanGPQD (ssinf.py:1302-1319); see make_golden.py for how the reference is reached and for the shims.

Per block of tests/_taylor_oracle.py CASES: N_ITEMS seeded inputs (means of order one, P = A A' + 0.05 I with A ~ N(0, 1) / sqrt(D),
time indices 0 .. 7) and N_PAR kernel-parameter rows (alpha = 1 and 2.5 with ell ~ U[0.5, 5] per dimension, alpha = 2.5 with
ell = 1e3: the linearisation limit); stored are mean_f, cov_f, the TRANSPOSE of the reference's (D, E) cov_fx, model_var and
integ_var of every (row, item).  For UNGM - the one system on which the reference's own filter runs (its measurement update
needs dim_y == dim_state) - fi_mean / fi_cov of ExtendedKalmanGPQD over T = 20 steps for 4 sequences.

Run:  PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python tests/golden/make_golden_taylor.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests.golden import make_golden as mg  # noqa: E402  (installs the shims, puts the reference on the path)
from tests._taylor_oracle import CASES, N_ITEMS, N_PAR, ELL_LIMIT  # noqa: E402

from ssmtoybox.mtran import TaylorGPQDTransform  # noqa: E402
from ssmtoybox.utils import GaussRV  # noqa: E402
from ssmtoybox import ssmod, ssinf  # noqa: E402

FILTER_STEPS, FILTER_SEQS = 20, 4
FILTER_PAR_DYN, FILTER_PAR_OBS = np.array([[1.0, 3.0]]), np.array([[2.5, 2.0]])


def models():
    dt = 0.01
    q2 = GaussRV(2, cov=0.01 * np.array([[(dt ** 3) / 3, (dt ** 2) / 2], [(dt ** 2) / 2, dt]]))
    return {
        'ungm_dyn': (ssmod.UNGMTransition(GaussRV(1), GaussRV(1, cov=np.array([[10.0]]))), 'dyn'),
        'ungm_meas': (ssmod.UNGMMeasurement(GaussRV(1), 1), 'meas'),
        'pend_dyn': (ssmod.Pendulum2DTransition(GaussRV(2, mean=np.array([1.5, 0]), cov=0.01 * np.eye(2)), q2, dt=dt), 'dyn'),
        'pend_meas': (ssmod.Pendulum2DMeasurement(GaussRV(1, cov=np.array([[0.1]])), 2), 'meas'),
        'cv_dyn': (ssmod.ConstantVelocity(GaussRV(4), GaussRV(2), dt=0.5), 'dyn'),
        'ungmna_dyn': (ssmod.UNGMNATransition(GaussRV(1), GaussRV(1, cov=np.array([[10.0]]))), 'dyn'),
    }


def main():
    rng = np.random.default_rng(21)
    out = {'names': np.array(list(CASES))}
    worst_cond = 0.0
    for tag, (mod, kind) in models().items():
        fid, p, D, E, _ = CASES[tag]
        assert mod.dim_in == D
        f = mod.dyn_eval if kind == 'dyn' else mod.meas_eval
        # the model sees a scalar time, as make_golden.py g13 passes it (with the 1-element array of the filters
        # UNGMNATransition.dyn_fcn_dx builds a ragged list and NumPy >= 1.24 raises), and apply() a value it can take len() of
        g = lambda x, t, dx=False, f=f: np.atleast_1d(f(x, float(np.asarray(t).reshape(-1)[0]), dx=dx))      # noqa: E731
        means = rng.standard_normal((N_ITEMS, D))
        a = rng.standard_normal((N_ITEMS, D, D)) / np.sqrt(D)
        covs = np.einsum('bij,bkj->bik', a, a) + 0.05 * np.eye(D)
        covs = 0.5 * (covs + covs.transpose(0, 2, 1))
        times = np.arange(N_ITEMS, dtype=float)
        par = np.column_stack((np.array([1.0, 2.5, 2.5]), rng.uniform(0.5, 5.0, (N_PAR, D))))
        par[N_PAR - 1, 1:] = ELL_LIMIT
        mf, cf, cfx = np.zeros((N_PAR, N_ITEMS, E)), np.zeros((N_PAR, N_ITEMS, E, E)), np.zeros((N_PAR, N_ITEMS, E, D))
        for r in range(N_PAR):
            tf = TaylorGPQDTransform(D, par[r:r + 1])
            for i in range(N_ITEMS):
                m, c, cx = tf.apply(g, means[i], covs[i], np.atleast_1d(times[i]))
                mf[r, i], cf[r, i], cfx[r, i] = np.atleast_1d(m), np.atleast_2d(c), np.atleast_2d(cx).reshape(D, E).T
                Lam = np.diag(par[r, 1:] ** 2)
                worst_cond = max(worst_cond, np.linalg.cond(Lam + covs[i]), np.linalg.cond(0.5 * Lam + covs[i]))
            out[tag + '_mvar_%d' % r], out[tag + '_ivar_%d' % r] = np.array(tf.mvar_list), np.array(tf.ivar_list)
        out[tag + '_mean'], out[tag + '_cov'], out[tag + '_time'], out[tag + '_par'] = means, covs, times, par
        out[tag + '_mf'], out[tag + '_cf'], out[tag + '_cfx'] = mf, cf, cfx
        out[tag + '_mvar'] = np.array([out.pop(tag + '_mvar_%d' % r) for r in range(N_PAR)])
        out[tag + '_ivar'] = np.array([out.pop(tag + '_ivar_%d' % r) for r in range(N_PAR)])
    # every quantity is a well-conditioned function of its inputs: cond(Lam + P), cond(Lam / 2 + P) times the unit roundoff
    print('largest condition number of Lam + P and Lam / 2 + P: %.3g  ->  relative accuracy about %.1e' % (worst_cond, worst_cond * 2.2e-16))
    assert worst_cond < 1e4
    # the reference's own filter on UNGM
    dyn = ssmod.UNGMTransition(GaussRV(1), GaussRV(1, cov=np.array([[10.0]])))
    obs = ssmod.UNGMMeasurement(GaussRV(1), 1)
    np.random.seed(2100)
    x = dyn.simulate_discrete(FILTER_STEPS, FILTER_SEQS)
    y = obs.simulate_measurements(x)
    alg = ssinf.ExtendedKalmanGPQD(dyn, obs, FILTER_PAR_DYN, FILTER_PAR_OBS)
    fm, fc = np.zeros((1, FILTER_STEPS, FILTER_SEQS)), np.zeros((1, 1, FILTER_STEPS, FILTER_SEQS))
    for s in range(FILTER_SEQS):
        fm[..., s], fc[..., s] = alg.forward_pass(y[..., s])
        alg.reset()
    out.update(ekf_ungm_y=y, ekf_ungm_fm=fm, ekf_ungm_fc=fc, ekf_ungm_par_dyn=FILTER_PAR_DYN, ekf_ungm_par_obs=FILTER_PAR_OBS)
    mg.save('g21_taylor_gpqd', **out)


if __name__ == '__main__':
    main()
