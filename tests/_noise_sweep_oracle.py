"""The noise sweep restated on the CPU pieces that exist: for every row p the oracle's filter recursion (oracle.ssmq_oracle.gaussian_filter
through tests/_sweep_oracle.py: filtered) with that row's Q, R and P0, and the innovation scores of tests/_innovation_oracle.py on its
filtered moments; the transforms are ino.sigma_tf / ino.bq_tf (and, for the t-process filter with more than one output, tp_tf of
tests/_student_score_oracle.py, which adds the whole model-variance matrix as StudentProcessKalman does) and are shared by all rows.
New here: the loop over p, the totals (ascending k) and the status words of tests/_sweep_oracle.py - no arithmetic of a step."""
import numpy as np

from oracle import ssmq_oracle as orc
from tests import _innovation_oracle as ino
from tests import _student_score_oracle as sso
from tests import _sweep_oracle as swo


def sigma_rule(form, D):
    """(unit points, wm, wc_diag) of the filter's sigma-point rule: 'ut' (UnscentedKalman's defaults) or 'sr' (CubatureKalman)."""
    if form == 'ut':
        return (orc.points_ut(D),) + orc.weights_ut(D)
    return orc.points_sr(D), orc.weights_sr(D), orc.weights_sr(D)


def transforms(case, weights=None):
    """(tf_dyn, tf_obs) of the case, shared by all rows.  weights: None - the oracle's own - or (dyn, obs) dicts (wm, Wc, Wcc,
    model_var, iK) of the device's weights, for the BQ forms."""
    form, D = case['form'], case['m0'].shape[0]
    fd, pd, fo, po, sidx = case['fid_dyn'], case['p_dyn'], case['fid_obs'], case['p_obs'], case['sidx']
    if form in ('ut', 'sr'):
        pts, wm, wc = sigma_rule(form, D)
        return ino.sigma_tf(fd, pd, pts, wm, wc), ino.sigma_tf(fo, po, pts, wm, wc, sidx)
    pts = orc.points_ut(D)
    wd, wo = weights if weights is not None else (orc.gp_weights(case['par'], pts), orc.gp_weights(case['par'], pts))
    if form == 'tp':
        return sso.tp_tf(fd, pd, pts, wd, case['nu']), sso.tp_tf(fo, po, pts, wo, case['nu'], sidx)
    return ino.bq_tf(fd, pd, pts, wd), ino.bq_tf(fo, po, pts, wo, sidx)


def sweep(case, y, q_rows, r_rows, x0_rows, weights=None):
    """y (Y, T, B); q_rows (P, dq, dq), r_rows (P, Y, Y), x0_rows (P, D, D): row p's covariances (a shared matrix repeated).
    Returns dict: loglik, nis (P, T, B), loglik_total, nis_mean, status (P, B), S (P, B) lists of (Y, Y, T), fm (P, B) lists of the
    filtered (fm, fP) the scores were taken from."""
    Y, T, B = y.shape
    P = len(q_rows)
    tfd, tfo = transforms(case, weights)
    G, m0 = case['G'], case['m0']
    out = dict(loglik=np.full((P, T, B), np.nan), nis=np.full((P, T, B), np.nan), loglik_total=np.full((P, B), np.nan),
               nis_mean=np.full((P, B), np.nan), status=np.zeros((P, B), dtype=np.int32), S=[[None] * B for _ in range(P)],
               fm=[[None] * B for _ in range(P)])
    for p in range(P):
        Q, R, P0 = q_rows[p], r_rows[p], x0_rows[p]
        GQG = G.dot(Q).dot(G.T)
        for b in range(B):
            fm, fP = swo.filtered(y[..., b], m0, P0, Q, R, G, tfd, tfo)
            out['fm'][p][b] = (fm, fP)
            with np.errstate(all='ignore'):
                _, S, nis, ll = ino.innovations(y[..., b], m0, P0, fm, fP, GQG, R, tfd, tfo)
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
