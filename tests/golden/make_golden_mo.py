"""
Generate tests/golden/g19_multi_output.npz by running the REFERENCE's multi-output parts (see make_golden.py for how the
reference is reached and for the shims).  The reference's multi-output transforms are unfinished: the
moments are composed from the parts that work - `model.bq_weights(par)`, `exp_model_variance`, `_mean` and `_cross_covariance`
as they are, the per-pair loop of `_covariance`, the model variance as `np.diag(emv)`.

Run:  PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python tests/golden/make_golden_mo.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests.golden import make_golden as mg  # noqa: E402  (installs the shims, puts the reference on the path)
from tests._mo_oracle import CASES, JITTER, NU, smooth_map  # noqa: E402

from ssmtoybox.bq.bqmtran import (GaussianProcessTransform, StudentTProcessTransform,  # noqa: E402
                                  MultiOutputGaussianProcessTransform, MultiOutputStudentTProcessTransform)

COND_CAP = 1e7
N_INPUTS = 16


def integrand(name, E, mods):
    """f(x_column, time) -> (E,) of the reference's model functions (additive models are evaluated without noise)."""
    if name == 'smooth':
        return lambda x, t: smooth_map(x, E)
    if name == 'reentry_bias_dyn':        # this build's synthetic 6-D case: reentry-2D + a pass-through state
        core = mods['reentry_dyn'][0]
        return lambda x, t: np.concatenate((core.dyn_eval(x[:5], t), x[5:]))
    mod, kind = mods[name][0], mods[name][1]
    return mod.dyn_eval if kind == 'dyn' else mod.meas_eval


def compose(tf, w, fx, chol, emv):
    wm, Wc, Wcc = w
    E = fx.shape[0]
    mean = tf._mean(wm, fx).copy()
    cov = np.zeros((E, E))
    for i in range(E):
        for j in range(i + 1):
            cov[i, j] = cov[j, i] = fx[i, :].dot(Wc[..., i, j]).dot(fx[j, :])
    cov = cov - np.outer(mean, mean.T) + np.diag(emv)
    ccov = tf._cross_covariance(Wcc, fx, chol).copy()
    return mean, cov, ccov


def main():
    rng = np.random.default_rng(0)
    mods = mg.make_models()
    out = {'names': np.array(list(CASES))}
    for name, (D, E, pts, ppar, fname) in CASES.items():
        par = np.column_stack((rng.uniform(0.5, 2.0, E), rng.uniform(1.0, 3.5, (E, D))))
        f = integrand(fname, E, mods)
        if fname == 'smooth':
            mean0, std0 = np.zeros(D), np.ones(D)
        elif fname == 'reentry_bias_dyn':
            mean0, std0 = np.append(mods['reentry_dyn'][4], 0.3), np.append(mods['reentry_dyn'][5], 0.3)
        else:
            mean0, std0 = mods[fname][4], mods[fname][5]
        tfs = {'gp': MultiOutputGaussianProcessTransform(D, E, par, 'rbf', pts, ppar),
               'tp': MultiOutputStudentTProcessTransform(D, E, par, 'rbf', pts, ppar, nu=NU)}
        ws = {k: tf.model.bq_weights(par) for k, tf in tfs.items()}
        model = tfs['gp'].model
        xi = model.points
        N = xi.shape[1]
        cond = np.array([np.linalg.cond(model.kernel.eval(par[e], xi, scaling=False) + JITTER * np.eye(N)) for e in range(E)])
        assert cond.max() <= COND_CAP, (name, cond)
        means = mean0[None, :] + std0[None, :] * rng.standard_normal((N_INPUTS, D))
        covs = np.zeros((N_INPUTS, D, D))
        for b in range(N_INPUTS):
            a = 0.3 * std0[:, None] * rng.standard_normal((D, D))
            covs[b] = a.dot(a.T) + 1e-3 * np.diag(std0 ** 2)
        time = 3.0
        res = {k: [] for k in ('fx', 'emv_gp', 'emv_tp', 'mf_gp', 'cf_gp', 'cfx_gp', 'mf_tp', 'cf_tp', 'cfx_tp')}
        for b in range(N_INPUTS):
            chol = np.linalg.cholesky(covs[b])
            x = means[b][:, None] + chol.dot(xi)
            fx = np.apply_along_axis(f, 0, x, np.atleast_1d(time)).reshape(E, N)
            res['fx'].append(fx)
            for k, tf in tfs.items():
                emv = tf.model.exp_model_variance(fx)
                m, c, cx = compose(tf, ws[k], fx, chol, emv)
                res['emv_' + k].append(np.array(emv))
                res['mf_' + k].append(m)
                res['cf_' + k].append(c)
                res['cfx_' + k].append(cx)
        # equal rows: the composition is the reference's single-output transform
        par_eq = np.repeat(par[:1], E, axis=0)
        for k, cls, kw in (('gp', GaussianProcessTransform, {}), ('tp', StudentTProcessTransform, {'nu': NU})):
            mo = (MultiOutputGaussianProcessTransform if k == 'gp' else MultiOutputStudentTProcessTransform)(
                D, E, par_eq, 'rbf', pts, ppar, **kw)
            w_eq = mo.model.bq_weights(par_eq)
            so = cls(D, E, par_eq[:1], 'rbf', pts, ppar, **kw)
            if k == 'tp':
                so.model.nu = NU          # the reference does not forward nu to the 'tp' model
            chol = np.linalg.cholesky(covs[0])
            m, c, cx = compose(mo, w_eq, res['fx'][0], chol, mo.model.exp_model_variance(res['fx'][0]))
            m1, c1, cx1 = so.apply(f, means[0], covs[0], np.atleast_1d(time))
            scale = max(1.0, np.abs(m1).max()) ** 2
            assert np.abs(m - m1).max() <= 1e-12 * scale and np.abs(c - c1).max() <= 1e-12 * scale and \
                np.abs(cx - cx1).max() <= 1e-12 * scale, (name, k)
        wm, Wc, Wcc = ws['gp']
        out.update({name + '_xi': xi, name + '_par': par, name + '_wm': wm, name + '_Wc': Wc, name + '_Wcc': Wcc,
                    name + '_q': model.q, name + '_Q': model.Q, name + '_R': model.R, name + '_iK': model.iK,
                    name + '_model_var': tfs['gp'].model.exp_model_variance(res['fx'][0]),
                    name + '_integral_var': tfs['gp'].model.integral_variance(res['fx'][0], par),
                    name + '_cond': cond, name + '_mean': means, name + '_cov': covs, name + '_time': np.array(time)})
        out.update({name + '_' + k: np.array(v) for k, v in res.items()})
        print(name, 'N', N, 'cond max %.3g' % cond.max())
    mg.save('g19_multi_output', **out)


if __name__ == '__main__':
    main()
