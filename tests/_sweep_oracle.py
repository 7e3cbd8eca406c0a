"""The kernel-parameter sweep restated on the CPU pieces that exist: for every row p the oracle's weights, the oracle's filter
recursion (oracle.ssmq_oracle.gaussian_filter) and the innovation scores of tests/_innovation_oracle.py on its filtered moments.
New here: the loop over p, the totals (ascending k) and the status words - no arithmetic of a step."""
import numpy as np

from oracle import ssmq_oracle as orc
from tests import _innovation_oracle as ino


def row_weights(kind, par_row, pts, mulind=None):
    """The oracle's weights of one parameter row, or None where its kernel matrix is not positive definite (LinAlgError) or not
    even finite (the ValueError of scipy's cho_factor)."""
    try:
        with np.errstate(all='ignore'):
            w = orc.gp_weights(par_row, pts) if kind == 'gp' else orc.bs_weights(par_row, pts, mulind)
    except (np.linalg.LinAlgError, ValueError):
        return None
    return w if np.all(np.isfinite(w['wm'])) else None


def bq_tf_ld(fid, p, pts, w, state_index=None):
    """orc.apply_bq of the float64 weights `w` in long double (as ino.sigma_tf_ld is of apply_sigma): what the float64 restatement
    itself is worth on a case (ino.helper_error)."""
    LD = ino.LD
    pts, wm, Wc, Wcc = (np.asarray(a, dtype=LD) for a in (pts, w['wm'], w['Wc'], w['Wcc']))
    p, mv = tuple(LD(v) for v in p), LD(w['model_var'])

    def tf(m, P, t):
        chol = ino.chol_ld(P)
        x = m[:, None] + chol.dot(pts)
        fx = np.stack([np.asarray(orc.integrand(fid, x[:, i] if state_index is None else x[np.asarray(state_index), i], LD(t), p), dtype=LD)
                       for i in range(x.shape[1])], axis=1)
        mf = fx.dot(wm)
        return mf, fx.dot(Wc).dot(fx.T) - np.outer(mf, mf) + mv * np.eye(fx.shape[0], dtype=LD), fx.dot(Wcc.T).dot(chol.T)
    return tf


def helper_error(case, y, par_dyn, par_obs, ref):
    """max over the items of ino.helper_error: (nis, ll) errors of the float64 restatement against its long-double form, relative to
    max(1, |value|), each step from the float64 filtered moments of `ref` (a `sweep` result)."""
    GQG = case['G'].dot(case['Q']).dot(case['G'].T)
    worst = np.zeros(2)
    for p in range(par_dyn.shape[0]):
        wd, wo = ref['weights'][p]
        tfd = bq_tf_ld(case['fid_dyn'], case['p_dyn'], case['pts'], wd)
        tfo = bq_tf_ld(case['fid_obs'], case['p_obs'], case['pts'], wo, case['sidx'])
        for b in range(y.shape[2]):
            fm, fP = ref['fm'][p][b]
            worst = np.maximum(worst, ino.helper_error(y[..., b], case['m0'], case['P0'], fm, fP, GQG, case['R'], tfd, tfo,
                                                       ref['nis'][p, :, b], ref['loglik'][p, :, b]))
    return tuple(worst)


def filtered(y, m0, P0, Q, R, G, tfd, tfo):
    """gaussian_filter on the longest prefix of y it completes; the steps after it NaN (the device's failure rule)."""
    D, T = m0.shape[0], y.shape[1]
    fm, fP = np.full((D, T), np.nan), np.full((D, D, T), np.nan)
    for n in range(T, 0, -1):
        try:
            with np.errstate(all='ignore'):
                a, b = orc.gaussian_filter(y[:, :n], m0, P0, Q, R, G, tfd, tfo)[:2]
        except (np.linalg.LinAlgError, ValueError):      # (ValueError: scipy's cho_factor on a matrix that holds a NaN)
            continue
        fm[:, :n], fP[..., :n] = a, b
        break
    return fm, fP


def sweep(case, y, par_dyn, par_obs, weights=None):
    """case: dict(kind, fid_dyn, p_dyn, fid_obs, p_obs, sidx, pts, mulind, m0, P0, Q, G, R); y (Y, T, B); par_* (P, 1 + D).
    weights: None - the oracle's own weights of every row - or (dyn, obs) lists of P weight dicts (wm, Wc, Wcc, model_var; None = that
    row failed): the device's, so that the comparison is about the recursion and not about the conditioning of the kernel matrix.
    Returns dict: loglik, nis (P, T, B), loglik_total, nis_mean, status (P, B), theta_status (P,), S (P, B) lists of (Y, Y, T), fm (P, B) lists of the
    filtered (fm, fP) the scores were taken from."""
    Y, T, B = y.shape
    P = par_dyn.shape[0]
    GQG = case['G'].dot(case['Q']).dot(case['G'].T)
    out = dict(loglik=np.full((P, T, B), np.nan), nis=np.full((P, T, B), np.nan), loglik_total=np.full((P, B), np.nan), nis_mean=np.full((P, B), np.nan),
               status=np.zeros((P, B), dtype=np.int32), theta_status=np.zeros(P, dtype=np.int32), S=[[None] * B for _ in range(P)], fm=[[None] * B for _ in range(P)], weights=[None] * P)
    for p in range(P):
        wd = row_weights(case['kind'], par_dyn[p], case['pts'], case['mulind']) if weights is None else weights[0][p]
        wo = row_weights(case['kind'], par_obs[p], case['pts'], case['mulind']) if weights is None else weights[1][p]
        out['weights'][p] = (wd, wo)
        if wd is None or wo is None:
            out['theta_status'][p] = (wd is None) + 4 * (wo is None)
            out['status'][p] = -1
            continue
        tfd = ino.bq_tf(case['fid_dyn'], case['p_dyn'], case['pts'], wd)
        tfo = ino.bq_tf(case['fid_obs'], case['p_obs'], case['pts'], wo, case['sidx'])
        for b in range(B):
            fm, fP = filtered(y[..., b], case['m0'], case['P0'], case['Q'], case['R'], case['G'], tfd, tfo)
            out['fm'][p][b] = (fm, fP)
            _, S, nis, ll = ino.innovations(y[..., b], case['m0'], case['P0'], fm, fP, GQG, case['R'], tfd, tfo)
            bad = np.flatnonzero(~(np.isfinite(nis) & np.isfinite(ll)))
            if bad.size:
                nis[bad[0]:], ll[bad[0]:] = np.nan, np.nan
                out['status'][p, b] = 1 + bad[0]
            sl = sn = 0.0
            for k in range(T):
                sl, sn = sl + ll[k], sn + nis[k]
            out['nis'][p, :, b] = nis
            out['loglik'][p, :, b], out['loglik_total'][p, b], out['nis_mean'][p, b], out['S'][p][b] = ll, sl, sn / T, S
    return out
