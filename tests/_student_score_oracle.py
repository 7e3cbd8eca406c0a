"""The scored recursions of k_filter_score<> restated in NumPy: the steps of oracle.ssmq_oracle.student_filter (and of gaussian_filter
for the Gaussian recursion on t-process transforms) with the score of every step,

    Studentian:  nis = Delta^2 = e' S_y^-1 e,   ll = log t_dof(y | y_mean, S_y)
                     = lgamma((dof + Y) / 2) - lgamma(dof / 2) - Y / 2 log(dof pi) - log det S_y / 2 - (dof + Y) / 2 log1p(Delta^2 / dof)
    Gaussian:    nis = e' S^-1 e,               ll = -(Y log 2 pi + log det S + nis) / 2

The transforms take their WEIGHTS as arguments, so a test can hand them the device's own (at large length-scales the oracle's weights
drift far more than the recursion's rounding).  Everything runs in float64 or, with ld=True, in long double on the same float64
weights: `helper_error` is what the float64 restatement itself is worth on a case (the convention of tests/_sweep_oracle.py)."""
import math

import numpy as np

from oracle import ssmq_oracle as orc
from tests import _innovation_oracle as ino

LD = ino.LD


def _chol(A, ld):
    return ino.chol_ld(A) if ld else np.linalg.cholesky(A)


def _fwd(L, b):
    """L^-1 b, columns of b."""
    v = np.zeros_like(b)
    for i in range(L.shape[0]):
        v[i] = (b[i] - L[i, :i].dot(v[:i])) / L[i, i]
    return v


def _bwd(L, v):
    """L^-T v."""
    x = np.zeros_like(v)
    for i in range(L.shape[0] - 1, -1, -1):
        x[i] = (v[i] - L[i + 1:, i].dot(x[i + 1:])) / L[i, i]
    return x


def tp_tf(fid, p, pts, w, nu, state_index=None, ld=False):
    """t-process BQ transform (mean, cov, t) -> (mean_f, cov_f, cov_fx) of the weights w (wm, Wc, Wcc, iK, model_var), as the
    t-process FILTERS build it - with one output, so for E > 1 the whole matrix (nu - 2 + fx iK fx') / (nu - 2 + N) model_var is added
    (bq/bqmtran.py:394-415, `* I_out` with I_out = eye(1))."""
    T = LD if ld else float
    pts, wm, Wc, Wcc, iK = (np.asarray(a, dtype=T) for a in (pts, w['wm'], w['Wc'], w['Wcc'], w['iK']))
    p, mv, nu = tuple(T(v) for v in p), T(w['model_var']), T(nu)
    N = pts.shape[1]

    def tf(m, P, t):
        chol = _chol(np.asarray(P, dtype=T), ld)
        x = np.asarray(m, dtype=T)[:, None] + chol.dot(pts)
        fx = np.stack([np.asarray(orc.integrand(fid, x[:, i] if state_index is None else x[np.asarray(state_index), i], T(t), p), dtype=T)
                       for i in range(N)], axis=1)
        mf = fx.dot(wm)
        emv = (nu - 2 + fx.dot(iK).dot(fx.T)) / (nu - 2 + N) * mv
        return mf, fx.dot(Wc).dot(fx.T) - np.outer(mf, mf) + emv, fx.dot(Wcc.T).dot(chol.T)
    return tf


def fs_tf(fid, p, pts, wm, wc_diag, state_index=None, ld=False):
    """The centred sigma-point transform of the fully-symmetric rule (oracle apply_sigma; long double: ino.sigma_tf_ld)."""
    if ld:
        return ino.sigma_tf_ld(fid, p, pts, wm, wc_diag, state_index)
    return ino.sigma_tf(fid, p, pts, wm, wc_diag, state_index)


def student_lnorm(dof, Y):
    return math.lgamma(0.5 * (dof + Y)) - math.lgamma(0.5 * dof) - 0.5 * Y * math.log(dof * math.pi)


def score(e, S, dof=None, ld=False):
    """(nis, ll) of the innovation e with scale matrix / covariance S: Student-t with `dof`, or Gaussian (dof None)."""
    T = LD if ld else float
    Y = S.shape[0]
    L = _chol(np.asarray(S, dtype=T), ld)
    v = _fwd(L, np.asarray(e, dtype=T))
    nis = v.dot(v)
    lg = np.sum(np.log(np.diag(L)))
    if dof is None:
        pi = np.arccos(T(-1)) if ld else np.pi
        return nis, -(Y * np.log(2 * pi) + 2 * lg + nis) / 2
    return nis, T(student_lnorm(dof, Y)) - lg - (T(dof) + Y) / 2 * np.log1p(nis / T(dof))


def step(y_k, m, smat, k, GqG, r_smat, tf_dyn, tf_obs, sc=1.0, dof=None, ld=False):
    """One step from (m, smat) - the lower triangle of smat is read, as on the device: (nis, ll, S_y, m_new, smat_new)."""
    T = LD if ld else float
    m_pr, P_pr, _ = tf_dyn(np.asarray(m, dtype=T), ino.lower_sym(np.asarray(smat, dtype=T)), k)
    S_pr = ino.lower_sym(sc * P_pr + np.asarray(GqG, dtype=T))
    y_mean, P_y, P_yx = tf_obs(m_pr, S_pr, k)
    S_y = ino.lower_sym(sc * P_y + np.asarray(r_smat, dtype=T))
    S_yx = sc * P_yx
    e = np.asarray(y_k, dtype=T) - y_mean
    nis, ll = score(e, S_y, dof, ld)
    L = _chol(S_y, ld)
    gain = _bwd(L, _fwd(L, S_yx)).T
    P = S_pr - gain.dot(S_y).dot(gain.T)
    fac = 1 if dof is None else (T(dof) + nis) / (T(dof) + y_k.shape[0])
    return nis, ll, S_y, m_pr + gain.dot(e), fac * P


def scored(y, m0, S0, GqG, r_smat, tf_dyn, tf_obs, scale_seq=None, dof=None):
    """One trajectory y (Y, T) in float64.  dof None: the Gaussian recursion (scale_seq ignored); else the Studentian one with the
    scale table scale_seq (T,).  Returns dict nis, loglik (T,), loglik_total, nis_mean, status (1 + the first step whose scores are
    not numbers, NaN from there on - the device's rule), S (Y, Y, T) and `inputs`, the (m, smat) every step started from."""
    Y, T = y.shape
    out = dict(nis=np.full(T, np.nan), loglik=np.full(T, np.nan), S=np.full((Y, Y, T), np.nan), inputs=[], status=0)
    m, smat = np.array(m0, dtype=float), np.array(S0, dtype=float)
    sl = sn = 0.0
    for k in range(T):
        try:
            with np.errstate(all='ignore'):
                nis, ll, S_y, m_new, s_new = step(y[:, k], m, smat, k, GqG, r_smat, tf_dyn, tf_obs, 1.0 if dof is None else scale_seq[k], dof)
        except (np.linalg.LinAlgError, ValueError):
            nis = ll = np.nan
        if not (np.isfinite(nis) and np.isfinite(ll)):
            out['status'] = k + 1
            sl = sn = np.nan
            break
        out['inputs'].append((m, smat))
        out['nis'][k], out['loglik'][k], out['S'][..., k] = nis, ll, S_y
        sl, sn = sl + ll, sn + nis
        m, smat = m_new, s_new
    out['loglik_total'], out['nis_mean'] = sl, sn / T
    return out


def helper_error(y, ref, GqG, r_smat, tf_dyn_ld, tf_obs_ld, scale_seq=None, dof=None):
    """max |float64 restatement - its long-double form| / max(1, |value|) over the steps of one trajectory, (nis, ll): every step from
    the float64 inputs `ref['inputs']` of a `scored` result."""
    worst = [0.0, 0.0]
    for k, (m, smat) in enumerate(ref['inputs']):
        n, l = step(y[:, k], m, smat, k, GqG, r_smat, tf_dyn_ld, tf_obs_ld, LD(1.0 if dof is None else scale_seq[k]), dof, ld=True)[:2]
        worst[0] = max(worst[0], float(abs(ref['nis'][k] - n) / max(1, abs(n))))
        worst[1] = max(worst[1], float(abs(ref['loglik'][k] - l) / max(1, abs(l))))
    return worst


def predictive_draws(rng, n, y_mean, S_y, dof):
    """n draws of t_dof(y_mean, S_y): y_mean + chol(S_y) z sqrt(dof / chi2_dof)."""
    Y = S_y.shape[0]
    z = rng.standard_normal((n, Y)).dot(np.linalg.cholesky(S_y).T)
    return y_mean + z * np.sqrt(dof / rng.chisquare(dof, n))[:, None]
