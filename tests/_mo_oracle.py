"""NumPy composition of the multi-output BQ weights and moments from the oracle's single-output parts (oracle/ssmq_oracle.py:
rbf_inv, rbf_q, rbf_R, rbf_Q with two parameter rows), in the reference's layouts (bq/bqmod.py:1254-1315,
bq/bqmtran.py:486-520), plus the host-evaluated integrands and the case table of tests/golden/g19_multi_output.npz."""
import numpy as np

from oracle import ssmq_oracle as orc
from tests._cases import RTOL, rel_err

EPS = np.finfo(float).eps

JITTER = 1e-8
NU = 3.0

# name -> (D, E, points, point_par, integrand): integrand = a key of tests/_cases.MODELS, or 'smooth' (host-evaluated)
CASES = {
    'ungm': (1, 1, 'ut', None, 'ungm_dyn'),
    'pend': (2, 2, 'ut', None, 'pend_dyn'),
    'smooth23': (2, 3, 'gh', {'degree': 3}, 'smooth'),
    'radar': (5, 2, 'ut', None, 'radar_meas'),
    'reentry': (5, 5, 'ut', None, 'reentry_dyn'),
    'reentry_bias': (6, 6, 'ut', None, 'reentry_bias_dyn'),
    'smooth34': (3, 4, 'fs', {'degree': 5}, 'smooth'),
}


def smooth_map(x, E):
    """A smooth map R^D -> R^E of one column x (D >= 2)."""
    a, b = x[0], x[1]
    c = x[2] if x.shape[0] > 2 else 0.0
    out = [np.sin(a) + b * b, a * np.cos(b) + 0.5 * c, np.exp(-0.5 * a * a) + b - c * c, np.tanh(a + b) * (1.0 + c)]
    return np.array(out[:E])


def mo_weights(par, x, jitter=JITTER):
    """dict: wm (N, E), Wc (N, N, E, E), Wcc (D, N, E), q, Q, R, iK, model_var (E,), integral_var (E,)."""
    par = np.atleast_2d(par)
    E, (D, N) = par.shape[0], x.shape
    q, R, iK = np.zeros((N, E)), np.zeros((D, N, E)), np.zeros((N, N, E))
    Q, Wc = np.zeros((N, N, E, E)), np.zeros((N, N, E, E))
    for i in range(E):
        q[:, i] = orc.rbf_q(par[i], x)
        R[..., i] = orc.rbf_R(par[i], x)
        ik = orc.rbf_inv(par[i], x, jitter, scaling=False)
        iK[..., i] = 0.5 * (ik + ik.T)
        for j in range(i + 1):
            Q[..., i, j] = Q[..., j, i] = orc.rbf_Q(par[i], par[j], x)
            Wc[..., i, j] = Wc[..., j, i] = iK[..., i].dot(Q[..., i, j]).dot(iK[..., j])
    Wc = 0.5 * (Wc + Wc.swapaxes(0, 1).swapaxes(2, 3))
    wm = np.einsum('ne, nme -> me', q, iK)
    Wcc = np.einsum('die, ine -> dne', R, iK)
    mv = np.array([par[i, 0] ** 2 * (1 - np.trace(Q[..., i, i].dot(iK[..., i]))) for i in range(E)])
    iv = np.array([orc.rbf_kbar(par[i]) - q[:, i].dot(iK[..., i]).dot(q[:, i]) for i in range(E)])
    return dict(wm=wm, Wc=Wc, Wcc=Wcc, q=q, Q=Q, R=R, iK=iK, model_var=mv, integral_var=iv)


def mo_moments(fx, chol, wm, Wc, Wcc, emv):
    """(mean_f (E,), cov_f (E, E), cov_fx (E, D)) of bq/bqmtran.py:486-520 with the model variance on the diagonal."""
    E = fx.shape[0]
    mean = np.array([fx[i].dot(wm[:, i]) for i in range(E)])
    cov = np.zeros((E, E))
    for i in range(E):
        for j in range(i + 1):
            cov[i, j] = cov[j, i] = fx[i].dot(Wc[..., i, j]).dot(fx[j])
    cov = cov - np.outer(mean, mean) + np.diag(emv)
    ccov = np.array([fx[i].dot(Wcc[..., i].T).dot(chol.T) for i in range(E)])
    return mean, cov, ccov


def mo_emv(fx, w, nu=None):
    """Expected model variance per output: model_var ('gp-mo'), or scaled with the integrand values ('tp-mo', nu given)."""
    if nu is None:
        return np.array(w['model_var'])
    E, N = fx.shape
    quad = np.array([fx[i].dot(w['iK'][..., i]).dot(fx[i]) for i in range(E)])
    return (nu - 2 + quad) / (nu - 2 + N) * w['model_var']


def weight_bars(cond):
    """The bars of tests/test_gpu_parity.py for weights: (wm / Wcc and the other first-order quantities, Wc and the variances)."""
    return max(RTOL, 64 * cond * EPS), max(RTOL, 8 * cond ** 2 * EPS)


def check_weights(w, g, name):
    """w: dict in the reference's layouts, against the golden case `name` of g."""
    cond = float(g[name + '_cond'].max())
    b1, b2 = weight_bars(cond)
    for k in ('wm', 'Wcc', 'q', 'R', 'iK'):
        assert rel_err(w[k], g[name + '_' + k]) <= b1, (name, k, rel_err(w[k], g[name + '_' + k]), b1)
    for k in ('Wc', 'Q', 'model_var', 'integral_var'):
        assert rel_err(w[k], g[name + '_' + k]) <= b2, (name, k, rel_err(w[k], g[name + '_' + k]), b2)
