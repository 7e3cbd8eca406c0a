"""
Generate tests/golden/g22_truncated.npz by running the REFERENCE's truncated sigma-point transforms (mtran.py:588-658) and its
GaussianInference with a truncated measurement transform passed in directly; see make_golden.py for how the reference is reached
and for the shims.

  * constructor attributes wm, Wc, Wcc, unit_sp_eff, unit_sp of the three classes for the (dim, dim_eff) pairs of
    tests/_truncated_oracle.py DIMS;
  * per apply case of CASES: N_ITEMS seeded inputs - means around the model's working point, covariances S (A A' / D + 0.05 I) S
    with A ~ N(0, 1) dense, so the trailing block is correlated with the leading one - and mean_f, cov_f, cov_fx of every rule;
  * filter trajectories of GaussianInference(dyn, obs, plain rule, Truncated*Transform(obs.dim_state, obs.dim_substate, ..)): the
    pendulum (T = 30, 4 sequences, all three rules, smoothed moments too) and reentry-2D + radar (T = 20, 4 sequences, unscented and
    spherical-radial).  The reference's own classes pass obs.dim_in, which equals dim_state, and so never truncate (ssinf.py:859).

Every item and every trajectory finishes in the reference without a LinAlgError (asserted here), so the device tests leave none out.

Run:  PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python tests/golden/make_golden_truncated.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests.golden import make_golden as mg  # noqa: E402  (installs the shims, puts the reference on the path)
from tests._truncated_oracle import CASES, DIMS, FILTERS, N_ITEMS, RULES  # noqa: E402

from ssmtoybox.mtran import (UnscentedTransform, SphericalRadialTransform, GaussHermiteTransform, TruncatedUnscentedTransform,  # noqa: E402
                             TruncatedSphericalRadialTransform, TruncatedGaussHermiteTransform)
from ssmtoybox.utils import GaussRV  # noqa: E402
from ssmtoybox import ssmod, ssinf  # noqa: E402

TRUNC = {'ut': TruncatedUnscentedTransform, 'sr': TruncatedSphericalRadialTransform, 'gh': TruncatedGaussHermiteTransform}
PLAIN = {'ut': UnscentedTransform, 'sr': SphericalRadialTransform, 'gh': GaussHermiteTransform}
M0_REENTRY = np.array([6500.4, 349.14, -1.8093, -6.7967, 0.6932])


def apply_models():
    """tag -> (measurement model, working point, per-state scale of the input covariance)"""
    return {
        'pend_meas': (ssmod.Pendulum2DMeasurement(GaussRV(1, cov=np.array([[0.1]])), 2), np.array([1.5, 0.0]), np.array([0.3, 0.5])),
        'range_meas': (ssmod.RangeMeasurement(GaussRV(1), 3), np.array([90.0, 6.0, 1.5]), np.array([2.0, 0.5, 0.2])),
        'radar_meas': (ssmod.Radar2DMeasurement(GaussRV(2), 5), M0_REENTRY, np.array([1e-2, 1e-2, 1e-3, 1e-3, 0.5])),
        'radar6_meas': (ssmod.Radar2DMeasurement(GaussRV(2), 6), np.append(M0_REENTRY, 0.2), np.array([1e-2, 1e-2, 1e-3, 1e-3, 0.5, 0.1])),
    }


def filter_systems():
    dt = 0.01
    q2 = GaussRV(2, cov=0.01 * np.array([[(dt ** 3) / 3, (dt ** 2) / 2], [(dt ** 2) / 2, dt]]))
    pend = (ssmod.Pendulum2DTransition(GaussRV(2, mean=np.array([1.5, 0]), cov=0.01 * np.eye(2)), q2, dt=dt),
            ssmod.Pendulum2DMeasurement(GaussRV(1, cov=np.array([[0.1]])), 2))
    P0 = np.diag([1e-6, 1e-6, 1e-6, 1e-6, 1])
    Qn = np.diag([2.4064e-5, 2.4064e-5, 1e-6])
    Rn = np.diag([1e-6, 0.17e-6])
    rer = (ssmod.ReentryVehicle2DTransition(GaussRV(5, M0_REENTRY, P0), GaussRV(3, cov=Qn)), ssmod.Radar2DMeasurement(GaussRV(2, cov=Rn), 5))
    return {'pend': (pend, RULES, 2200), 'rer': (rer, ('ut', 'sr'), 2201)}


def main():
    rng = np.random.default_rng(22)
    out = {'names': np.array(list(CASES)), 'dims': np.array(DIMS)}
    for rule in RULES:
        for dim, de in DIMS:
            tf = TRUNC[rule](dim, de)
            assert (tf.dim, tf.dim_eff) == (dim, de)
            for attr in ('wm', 'Wc', 'Wcc', 'unit_sp_eff', 'unit_sp'):
                out['ctor_%s_%d_%d_%s' % (rule, dim, de, attr)] = np.asarray(getattr(tf, attr), dtype=float)
    for tag, (mod, m0, scale) in apply_models().items():
        fid, p, D, de, E = CASES[tag]
        assert mod.dim_state == D and mod.dim_substate == de and mod.dim_out == E
        means = m0 + scale * rng.standard_normal((N_ITEMS, D))
        a = rng.standard_normal((N_ITEMS, D, D)) / np.sqrt(D)
        covs = (np.einsum('bij,bkj->bik', a, a) + 0.05 * np.eye(D)) * scale[:, None] * scale[None, :]
        covs = 0.5 * (covs + covs.transpose(0, 2, 1))
        assert np.all(np.abs(covs[:, de:, :de]) > 0)
        out[tag + '_mean'], out[tag + '_cov'] = means, covs
        for rule in RULES:
            tf = TRUNC[rule](D, de)
            mf, cf, cfx = np.zeros((N_ITEMS, E)), np.zeros((N_ITEMS, E, E)), np.zeros((N_ITEMS, E, D))
            for i in range(N_ITEMS):
                mf[i], cf[i], cfx[i] = tf.apply(mod.meas_eval, means[i], covs[i], np.atleast_1d(0.0))      # (a LinAlgError would end the run)
            out['%s_%s_mf' % (tag, rule)], out['%s_%s_cf' % (tag, rule)], out['%s_%s_cfx' % (tag, rule)] = mf, cf, cfx
    for tag, ((dyn, obs), rules, seed) in filter_systems().items():
        T, S, smooth = FILTERS[tag]
        D = dyn.dim_state
        np.random.seed(seed)
        x = dyn.simulate_discrete(T, S)
        y = obs.simulate_measurements(x)
        out[tag + '_y'] = y
        for rule in rules:
            alg = ssinf.GaussianInference(dyn, obs, PLAIN[rule](dyn.dim_in), TRUNC[rule](obs.dim_state, obs.dim_substate))
            fm, fc = np.zeros((D, T, S)), np.zeros((D, D, T, S))
            sm, sc = np.zeros((D, T, S)), np.zeros((D, D, T, S))
            for s in range(S):
                fm[..., s], fc[..., s] = alg.forward_pass(y[..., s])
                if smooth:
                    sm[..., s], sc[..., s] = alg.backward_pass()
                alg.reset()
            assert np.all(np.isfinite(fm)) and np.all(np.isfinite(fc))
            out['%s_%s_fm' % (tag, rule)], out['%s_%s_fc' % (tag, rule)] = fm, fc
            if smooth:
                out['%s_%s_sm' % (tag, rule)], out['%s_%s_sc' % (tag, rule)] = sm, sc
    mg.save('g22_truncated', **out)


if __name__ == '__main__':
    main()
