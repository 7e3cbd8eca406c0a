"""
Golden vectors for Model.predict: the reference's GaussianProcessModel / StudentTProcessModel / BayesSardModel.predict
(bq/bqmod.py:454-493, 1090-1130, 840-891) run here, together with the reference's OWN deviation from an exact evaluation of
the same formulas (mpmath, 40 digits, from the same float64 inputs), which is the yardstick of tests/test_predict_gpu.py.
Reuses the import shims of make_golden.py (importing that module installs them and loads the reference).

Run:  PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python tests/golden/make_golden_predict.py   -> tests/golden/g16_predict.npz

Per case `<case>_*`: x (D, N) training inputs, y (E, N) observations (outputs first, as predict takes them), xt (D, M) test
inputs = random points followed by the N training inputs, par (1 + D,), mean / var the reference's result, cond = cond_2(K +
jitter I), ref_err_mean = max |mean - exact| / max |y| and ref_err_var = max |var - exact| / alpha^2, and ref_ident_mean /
ref_ident_var: the reference's deviation, at the training inputs, from the interpolation identities
    mean_i - y_i = -jitter (iK y)_i,    var_i = jitter - jitter^2 iK_ii         (k_i = (K + jitter I) e_i - jitter e_i)
evaluated with its own eval_inv_dot, scaled the same way (GP and TP cases; the TP variance carries its scale).
`cases` lists the names; `<case>_kind` is gp / tp / bs; `<case>_num_pts` the model's own point count (the TP denominator);
`<case>_mulind` the Bayes-Sard multi-indices.  A case is only written if cond <= 1e7 and both ref_err < 1e-6.
`chain_*`: the reference's optimize on the GH(15) data of its own tests, then predict at the fitted parameters - the
identities' deviations at a fitted (longer, worse conditioned) length-scale, for the fit -> predict test.
"""
import os
import sys

import mpmath as mp
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.golden import make_golden as mg  # noqa: E402,F401  (installs the shims, imports the reference)
from ssmtoybox.bq.bqmod import GaussianProcessModel, StudentTProcessModel, BayesSardModel  # noqa: E402

NU = 3.0
COND_CAP, ERR_CAP = 1e7, 1e-6
mp.mp.dps = 40


def fcn(x):            # the reference tests' integrand (tests/test_bqmod.py:15)
    return np.sin((x + 1) ** -1)


def data(x, E, rng):
    """(E, N): the integrand summed over the inputs, then smooth columns with a little noise."""
    rows = [fcn(x).sum(axis=0)]
    rows += [np.cos(0.7 * (e + 1) * x).sum(axis=0) + 0.1 * rng.standard_normal(x.shape[1]) for e in range(E - 1)]
    return np.stack(rows, axis=0)


def make_model(kind, D, par, pts):
    if kind == 'gp':
        return GaussianProcessModel(D, par, 'rbf', pts[0], pts[1])
    if kind == 'tp':
        return StudentTProcessModel(D, par, 'rbf', pts[0], pts[1], nu=NU)
    return BayesSardModel(D, par, 2, pts[0], pts[1])


def mp_kernel(par, a, b):
    """alpha^2 exp(-sum_d ((a_di - b_dj) / ell_d)^2 / 2), exact in the float64 inputs."""
    al2 = mp.mpf(float(par[0])) ** 2
    K = mp.matrix(a.shape[1], b.shape[1])
    for i in range(a.shape[1]):
        for j in range(b.shape[1]):
            s = mp.mpf(0)
            for d in range(a.shape[0]):
                s += ((mp.mpf(float(a[d, i])) - mp.mpf(float(b[d, j]))) / mp.mpf(float(par[1 + d]))) ** 2
            K[i, j] = al2 * mp.exp(-s / 2)
    return K


def mp_vandermonde(mulind, x):
    V = mp.matrix(x.shape[1], mulind.shape[1])
    for n in range(x.shape[1]):
        for q in range(mulind.shape[1]):
            v = mp.mpf(1)
            for d in range(x.shape[0]):
                v *= mp.mpf(float(x[d, n])) ** int(mulind[d, q])
            V[n, q] = v
    return V


def exact_predict(kind, x, y, xt, par, jitter, num_pts, mulind):
    """The formulas of the three predict methods in 40-digit arithmetic: (mean (M, E), var (M,)) as float64."""
    N, M, E = x.shape[1], xt.shape[1], y.shape[0]
    K = mp_kernel(par, x, x)
    for i in range(N):
        K[i, i] += mp.mpf(jitter)
    iK = mp.inverse(K)
    kx = mp_kernel(par, xt, x)
    Y = mp.matrix(y.T.tolist())                 # (N, E)
    kxiK = kx * iK
    quad = [sum(kxiK[m, n] * kx[m, n] for n in range(N)) for m in range(M)]
    kxx = mp.mpf(float(par[0])) ** 2
    if kind == 'bs':
        V = mp_vandermonde(mulind, x)
        Z = V.T * iK
        iG = mp.inverse(Z * V)
        A = iG * V.T
        b = Z * kx.T - mp_vandermonde(mulind, xt).T          # (NB, M)
        mean = (kx - b.T * A) * (iK * Y)
        biG = b.T * iG
        var = [kxx - quad[m] + sum(biG[m, q] * b[q, m] for q in range(b.rows)) for m in range(M)]
    else:
        mean = kxiK * Y
        var = [kxx - quad[m] for m in range(M)]
        if kind == 'tp':
            yiKy = (Y.T * iK * Y)[0, 0]
            scale = (mp.mpf(NU) - 2 + yiKy) / (mp.mpf(NU) - 2 + num_pts)
            var = [scale * v for v in var]
    return (np.array([[float(mean[m, e]) for e in range(E)] for m in range(M)]), np.array([float(v) for v in var]),
            np.array([[mean[m, e] for e in range(E)] for m in range(M)], dtype=object), np.array(var, dtype=object))


def run_case(out, name, kind, D, pts, par, E, M, rng, x_obs=None, y=None):
    par = np.asarray(par, dtype=float)
    m = make_model(kind, D, par[None, :], pts)
    x = m.points if x_obs is None else x_obs
    N = x.shape[1]
    if y is None:
        y = data(x, E, rng)
    xt = np.hstack((1.5 * rng.standard_normal((D, M)), x))
    jitter = m.kernel.jitter
    cond = np.linalg.cond(m.kernel.eval(par, x) + jitter * np.eye(N))
    if cond > COND_CAP:
        print('  {}: cond {:.2e} over the cap'.format(name, cond))
        return False
    yy = y[0] if kind == 'tp' else (y[0] if E == 1 else y)      # the TP takes (N,) only
    mean, var = m.predict(xt, yy, x, par[None, :])
    mean2 = np.asarray(mean).reshape(xt.shape[1], E)
    mulind = m.mulind if kind == 'bs' else None
    _, _, emean, evar = exact_predict(kind, x, y, xt, par, jitter, m.num_pts, mulind)
    ys, vs = np.abs(y).max(), par[0] ** 2
    err_m = float(max(abs(mp.mpf(float(mean2[i, e])) - emean[i, e]) for i in range(mean2.shape[0]) for e in range(E))) / ys
    err_v = float(max(abs(mp.mpf(float(var[i])) - evar[i]) for i in range(var.shape[0]))) / vs
    if not (err_m < ERR_CAP and err_v < ERR_CAP):
        raise SystemExit('{}: the reference is {:.2e} / {:.2e} from exact - not a fair yardstick'.format(name, err_m, err_v))
    rec = dict(x=x, y=y, xt=xt, par=par, mean=np.asarray(mean), var=np.asarray(var), cond=cond, ref_err_mean=err_m,
               ref_err_var=err_v, kind=kind, num_pts=m.num_pts)
    if kind == 'bs':
        rec['mulind'] = mulind
    else:
        rec.update(identity_deviation(m, kind, x, y, par, mean2[M:], np.asarray(var)[M:]))
    for k, v in rec.items():
        out['{}_{}'.format(name, k)] = np.asarray(v)
    print('  {:10s} N {:3d} M {:3d} E {} cond {:.2e} ref_err mean {:.2e} var {:.2e}'.format(name, N, xt.shape[1], E, cond,
                                                                                           err_m, err_v))
    return True


def identity_deviation(m, kind, x, y, par, mean_tr, var_tr):
    """The reference against the interpolation identities at the training inputs, with its own eval_inv_dot."""
    jit = m.kernel.jitter
    iK = m.kernel.eval_inv_dot(par[None, :], x)
    scale = 1.0
    if kind == 'tp':
        scale = (NU - 2 + y[0].dot(iK).dot(y[0])) / (NU - 2 + m.num_pts)
    dm = np.abs((mean_tr - y.T) - (-jit * iK.dot(y.T))).max() / np.abs(y).max()
    dv = np.abs(var_tr - scale * (jit - jit ** 2 * np.diag(iK))).max() / par[0] ** 2
    return dict(ref_ident_mean=dm, ref_ident_var=dv)


def main():
    rng = np.random.default_rng(1609)
    out, names = {}, []

    def case(name, *args, **kw):
        if run_case(out, name, *args, **kw):
            names.append(name)
            return True
        return False

    gh15, gh5 = ('gh', {'degree': 15}), ('gh', {'degree': 5})
    for kind in ('gp', 'tp', 'bs'):
        case(kind + '_d1', kind, 1, gh15, [1.0, 0.5], 1, 40, rng)
        case(kind + '_d2', kind, 2, gh5, [1.0, 0.7, 1.3], 1, 63, rng)
    for kind in ('gp', 'bs'):
        case(kind + '_d2_e3', kind, 2, gh5, [1.0, 0.7, 1.3], 3, 9, rng)
        case(kind + '_d3_e2', kind, 3, ('fs', {'degree': 5}), [1.0, 1.5, 1.5, 1.5], 2, 30, rng)
    case('gp_d6_e6', 'gp', 6, ('ut', None), [1.0] + [2.0] * 6, 6, 200, rng)
    # training inputs that are not the model's points (40 random ones, the model has 25): the TP's num_pts quirk shows.  The
    # length-scales are shortened until cond(K + jitter I) passes the cap.
    xo = rng.uniform(-3, 3, (2, 40))
    for s in (1.0, 0.7, 0.5, 0.35, 0.25):
        par = [1.0, 0.7 * s, 1.3 * s]
        if case('gp_xo', 'gp', 2, gh5, par, 1, 50, rng, x_obs=xo):
            case('tp_xo', 'tp', 2, gh5, par, 1, 50, rng, x_obs=xo)
            case('bs_xo', 'bs', 2, gh5, par, 1, 50, rng, x_obs=xo)
            break
    # the packed route
    case('gp_n128', 'gp', 16, ('ut', None), [1.0] + [3.0] * 16, 2, 9, rng, x_obs=rng.standard_normal((16, 128)))
    out['cases'] = np.array(names)

    # fit -> predict with the reference: optimize from [1, 0.5] on the GH(15) data, predict at the fitted parameters
    for kind in ('gp', 'tp'):
        m = make_model(kind, 1, np.array([[1.0, 0.5]]), gh15)
        x = m.points
        y = fcn(x)                                          # (1, N)
        res = m.optimize(np.log(np.array([1.0, 0.5])), y.T, x, method='BFGS')
        par = np.exp(res.x)
        mean, var = m.predict(x, y[0], x, par[None, :])
        dev = identity_deviation(m, kind, x, y, par, np.asarray(mean)[:, None], np.asarray(var))
        cond = np.linalg.cond(m.kernel.eval(par, x) + m.kernel.jitter * np.eye(x.shape[1]))
        for k, v in dict(x=x, y=y, par=par, cond=cond, **dev).items():
            out['chain_{}_{}'.format(kind, k)] = np.asarray(v)
        print('  chain {} par {} cond {:.2e} identity deviation mean {:.2e} var {:.2e}'.format(
            kind, par, cond, dev['ref_ident_mean'], dev['ref_ident_var']))
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'g16_predict.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes,', len(out), 'arrays,', len(names), 'cases')


if __name__ == '__main__':
    main()
