"""High-precision restatement of one register-resident moment transform (k_apply_small, csrc/ssmq_apply_small.h), the reader of its
four dispatch tables, and the builders of the rules and inputs every instantiation is pinned with.

The restatement works in DPS-digit mpmath arithmetic from the float64 inputs taken exactly (mpf(float) is exact; the literal constants
of the models are the float64 numbers the reference's program holds, e.g. mpf(1.2), not 6/5): Cholesky factor of the lower triangle
of cov, x_n = m + L xi_n, f(x_n) with sub-state selection as oracle.ssmq_oracle.eval_columns does it, then moments_bq (model variance
as the (E, E) matrix ssmq_transform_create takes, both emv modes, optionally the t-process variance of tp_emv_diag) or moments_sigma.
Sums are exact dot products (mp.fdot) rounded once; results go back as float64.

Besides the moments every transform returns a float64 error scale per output entry, in two parts:

  A  the sum of the absolute values of the terms of the entry (for the uncentred covariance including |mean_i mean_j| and the model
     variance), i.e. what one rounding error per term is relative to;
  S  the first-order effect on the entry of rounding at the inputs and inside f: every sigma point carries
        dx_n = |m| + (1 + cond) |L| |xi_n|        (units of eps; cond: the condition number of the input covariance after scaling it to
                                                   unit diagonal - the error of a Cholesky factor is invariant under that scaling)
        df_n = T(x_n) + |J(x_n)| dx_n + |df/dt| |t|
     with J the Jacobian of f by central differences in mpmath and T the sum of the absolute values of the terms inside f (with the
     amplification of a rounded argument where f subtracts nearly equal numbers: 1 - cos(om dt) of the coordinated turn, the
     difference of two sines of CTRS, the exponent of the reentry drag).  df_n then goes through the exact first derivative of the
     entry with respect to f(x_n) (and dx_n / the factor's error through the explicit L' and x_n - m of the cross-covariances).

The bar of an entry is K eps (A + S).  K is not chosen: tests/test_apply_small_host.py measures the worst ratio K_REF of the plain
float64 NumPy restatement (oracle.ssmq_oracle.apply_bq / apply_sigma) over every case below and the kernels get K = max(16, 8 K_REF) -
the factor 8 for their different but fixed summation orders, the LDL' / symmetric-parameter factorisations of Wc (accepted by the host
only when they reproduce Wc to 1e-14), and the 2.5-ulp branch-free sincos / atan2 / exp sequences where libm has 0.5 ulp.

f(x_n), T and J are cached per (model, point set, input): the three forms of one shape share them."""
import collections
import functools
import os
import re

import mpmath as mp
import numpy as np

from oracle import ssmq_oracle as orc

DPS = 50
EPS = float(np.finfo(float).eps)

# Measured by tests/test_apply_small_host.py::test_float64_restatement_within_k_ref (2026-10-19): the worst ratio
# |float64 NumPy - oracle| / (eps (A + S)) over all 168 rows x 9 good probes is 0.963 (BQ: mean 0.35, cov 0.68, cross 0.36; BQ + t-process:
# 0.42, 0.96, 0.27; centred: 0.43, 0.20, 0.28; worst row: t-process form of the 2 -> 1 UNGM measurement with noise input, N = 9, the
# ill-scaled probe; worst model after it: radar 0.83); K_REF is that rounded up.  K = max(16, 8 K_REF).
K_REF = 0.97
K = max(16.0, 8.0 * K_REF)
# Worst |device - oracle| / (eps (A + S)) per form, (mean, cov, cross-covariance), on an MI355X (2026-10-19, the table test of
# tests/test_apply_small_gpu.py; the one-rule test of the fast-path shapes reaches 1.03 on a covariance): docs/KERNELS.md 3.1.
MEASURED_DEVICE = {'BQ': (0.59, 0.68, 0.41), 'BQ+TP': (0.61, 0.96, 0.38), 'SIGMA': (0.58, 0.18, 0.35)}

FORM_BQ, FORM_SIGMA = 0, 1
EMV_DIAG, EMV_BROADCAST = 0, 1
TP_NU = 4.5
N_PROBES, BAD_PROBE, ILL_PROBE = 10, 9, 8
B_LANES, LD = 131, 192
EXPECTED_ROWS = 168        # 46 shapes x 3 forms + 6 fast-path shapes x 5 kernels: a change of the tables is an edit here as well

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'ssmtoybox_amd', 'csrc')
TABLE_FILES = ('ssmq_small_a.hip', 'ssmq_small_b.hip', 'ssmq_small_c.hip', 'ssmq_small_d.hip')

_SENS = tuple(np.vstack((1000 * np.eye(2), -1000 * np.eye(2))).astype(float).reshape(-1))
_RE5 = [6500.4, 349.14, -1.8093, -6.7967, 0.6932]
_CT5 = [1000.0, 300.0, 1000.0, 0.0, -0.05]
# integrand -> (oracle id, constants, {(D, SEL): operating point}, jitter of the probes' means, descending ill-scaled diagonal)
# Operating points: those of test_generic_routes_random_point_sets; the coordinated-turn models keep their turn rate away from 0 (the
# ill-scaled probe gives THEM the small variances at the end of the state, where the turn rate sits).
MODELS = {
    'SSMQ_F_UNGM_DYN': (orc.F_UNGM_DYN, (), {(1, 0): [0.3]}, 1.0, False),
    'SSMQ_F_UNGM_MEAS': (orc.F_UNGM_MEAS, (), {(1, 0): [0.3]}, 1.0, False),
    'SSMQ_F_UNGMNA_DYN': (orc.F_UNGMNA_DYN, (), {(2, 0): [0.3, 0.1]}, 0.5, False),
    'SSMQ_F_UNGMNA_MEAS': (orc.F_UNGMNA_MEAS, (), {(2, 0): [0.3, 0.1]}, 0.5, False),
    'SSMQ_F_PENDULUM_DYN': (orc.F_PENDULUM_DYN, (0.01,), {(2, 0): [1.5, 0.0]}, 0.01, False),
    'SSMQ_F_PENDULUM_MEAS': (orc.F_PENDULUM_MEAS, (), {(2, 0): [1.5, 0.0]}, 0.01, False),
    'SSMQ_F_REENTRY1D_DYN': (orc.F_REENTRY1D_DYN, (0.1,), {(3, 0): [90.0, 6.0, 1.5]}, 0.01, False),
    'SSMQ_F_RANGE_MEAS': (orc.F_RANGE_MEAS, (), {(3, 0): [90.0, 6.0, 1.5]}, 0.01, False),
    'SSMQ_F_REENTRY2D_DYN': (orc.F_REENTRY2D_DYN, (0.1,), {(5, 0): _RE5}, 0.01, False),
    'SSMQ_F_REENTRY2D_BIAS_DYN': (orc.F_REENTRY2D_BIAS_DYN, (0.1,), {(6, 0): _RE5 + [0.5]}, 0.01, False),
    'SSMQ_F_RADAR2D_MEAS': (orc.F_RADAR2D_MEAS, (0.0, 0.0), {(5, 0): [6500.4, 349.14, -1.8, -6.8, 0.7], (5, 1): _CT5,
                                                              (4, 1): [10.0, 1.0, -5.0, 0.5], (6, 0): _RE5 + [0.5]}, 0.01, False),
    'SSMQ_F_CT_DYN': (orc.F_CT_DYN, (0.1,), {(5, 0): _CT5}, 0.01, True),
    'SSMQ_F_BEARING_MEAS': (orc.F_BEARING_MEAS, _SENS, {(5, 1): [100.0, 3.0, 200.0, 0.0, -0.05],
                                                        (5, 0): [100.0, 200.0, 3.0, 0.0, -0.05]}, 0.01, False),
    'SSMQ_F_CV_DYN': (orc.F_CV_DYN, (0.1,), {(4, 0): [10.0, 1.0, -5.0, 0.5]}, 0.01, False),
    'SSMQ_F_CTRS_DYN': (orc.F_CTRS_DYN, (0.05,), {(7, 0): [0.0, 0.0, 10.0, 0.3, 0.05, 0.0, 0.0]}, 0.01, True),
}
DIN = {orc.F_UNGM_DYN: 1, orc.F_UNGM_MEAS: 1, orc.F_UNGMNA_DYN: 2, orc.F_UNGMNA_MEAS: 2, orc.F_PENDULUM_DYN: 2, orc.F_PENDULUM_MEAS: 1,
       orc.F_REENTRY1D_DYN: 3, orc.F_RANGE_MEAS: 1, orc.F_REENTRY2D_DYN: 5, orc.F_REENTRY2D_BIAS_DYN: 6, orc.F_RADAR2D_MEAS: 2,
       orc.F_CT_DYN: 5, orc.F_BEARING_MEAS: 2, orc.F_CV_DYN: 4, orc.F_CTRS_DYN: 7, orc.F_SMOOTH10D_DYN: 10}


# ---- the dispatch tables -------------------------------------------------------------------------------------------------------
Row = collections.namedtuple('Row', 'file F D E N form tp sel opt name fast')
_ROW_RE = re.compile(r'SSMQ_SMALL(_FAST)?\(\s*(SSMQ_F_\w+)\s*,\s*(\d+)\s*,\s*(\d+)\s*,\s*(\d+)\s*,\s*(\d+)\s*\)')
_SMALL = ((FORM_BQ, 0, 0), (FORM_BQ, 1, 0), (FORM_SIGMA, 0, 0))                       # SSMQ_SMALL: (FORM, TP, OPT)
_FAST = ((FORM_BQ, 0, 7), (FORM_BQ, 0, 3), (FORM_BQ, 0, 1), (FORM_BQ, 1, 2), (FORM_SIGMA, 0, 2))   # SSMQ_SMALL_FAST adds these


def kernel_name(F, D, E, N, form, tp, sel, opt):
    """The string SSMQ_SMALL_ONE builds (the integrand and form ids are enumerators: they stringify as written)."""
    return 'k_apply_small<D=%d,E=%d,N=%d,%s,%s,TP=%d,SEL=%d,OPT=%d>' % (D, E, N, F, ('SSMQ_FORM_BQ', 'SSMQ_FORM_SIGMA')[form], tp, sel, opt)


@functools.lru_cache(maxsize=None)
def table_rows():
    """Every SmallEntry of the four tables, in table order, expanded exactly as ssmq_small_inst.h expands the two macros."""
    rows = []
    for fname in TABLE_FILES:
        with open(os.path.join(CSRC, fname)) as fh:
            text = fh.read()
        for m in _ROW_RE.finditer(text):
            fast, F = bool(m.group(1)), m.group(2)
            D, E, N, sel = (int(m.group(i)) for i in (3, 4, 5, 6))
            for form, tp, opt in _SMALL + (_FAST if fast else ()):
                rows.append(Row(fname, F, D, E, N, form, tp, sel, opt, kernel_name(F, D, E, N, form, tp, sel, opt), fast))
    return tuple(rows)


def form_tag(row):
    return 'SIGMA' if row.form == FORM_SIGMA else ('BQ+TP' if row.tp else 'BQ')


def state_index(row):
    """SEL 0: the leading entries (None); SEL 1: entries (0, 2, ...) of the state."""
    fid = MODELS[row.F][0]
    return None if row.sel == 0 else tuple(2 * k for k in range(DIN[fid]))


# ---- rules: random constants with no quadrature structure, shaped only so that the host offers the kernel wanted -------------------
def _ldl_accepts(Wc, upper=False, wmax=None):
    """upload_consts' own test, restated: LDL' without pivoting (of the index-reversed matrix for the unit UPPER factor of the symmetric
    block) reproduces the matrix to 1e-14 of its largest entry and meets no pivot below 1e-13 of it.  Taken at a third of the host's
    thresholds: its compiler may contract multiply-adds differently."""
    A = np.asarray(Wc, dtype=float)
    if upper:
        A = A[::-1, ::-1]
    n = A.shape[0]
    wmax = float(np.abs(A).max()) if wmax is None else wmax
    U, d = np.zeros((n, n)), np.zeros(n)
    for j in range(n):
        dj = A[j, j] - float(np.sum(U[j, :j] ** 2 * d[:j]))
        if not abs(dj) > 3e-13 * wmax:
            return False
        d[j], U[j, j] = dj, 1.0
        for i in range(j + 1, n):
            U[i, j] = (0.5 * (A[i, j] + A[j, i]) - float(np.sum(U[i, :j] * U[j, :j] * d[:j]))) / dj
    return bool(np.abs((U * d).dot(U.T) - A).max() <= 0.3e-14 * wmax)


def _mirror(A):
    """Symmetric to the last bit: the lower triangle mirrored."""
    return np.tril(A) + np.tril(A, -1).T


def _factorable(rng, n):
    """U diag(d) U' with a unit lower U of moderate entries and d of either sign: a symmetric Wc whose LDL' exists and is benign."""
    U = np.tril(0.4 * rng.standard_normal((n, n)), -1) + np.eye(n)
    d = rng.choice([-1.0, 1.0], n) * rng.uniform(0.3, 1.0, n) / n
    return _mirror((U * d).dot(U.T))


def _dyadic(a, bits=22):
    """Rounded to multiples of 2^-bits (|a| < 4): sums and differences of a few such numbers are exact in float64."""
    return np.round(np.asarray(a, dtype=float) * 2.0 ** bits) / 2.0 ** bits


def unscented_points(D, c):
    xi = np.zeros((D, 2 * D + 1))
    for d in range(D):
        xi[d, 1 + d], xi[d, 1 + D + d] = c, -c
    return xi


def _wants_ut(row):
    return row.opt in (7, 3, 2)


@functools.lru_cache(maxsize=None)
def points_for(F, D, N, sel, ut):
    """The point set of a shape: shared by all its rows that want the same kind ([0 | cI | -cI] for the unscented-type kernels, random
    points for the others), so that f(x_n) and the Jacobians are computed once."""
    rng = np.random.default_rng([20271, MODELS[F][0], D, N, sel, int(ut)])
    xi = unscented_points(D, float(rng.uniform(1.0, 2.5))) if ut else rng.standard_normal((D, N))
    xi.setflags(write=False)
    return xi


def symmetric_rule(rng, D):
    """(wm, Wc, Wcc) of a 2D+1-point rule that is invariant under every reflection of the unscented point set TO THE LAST BIT, from
    random symmetric parameters (wm_s, gamma, beta, Mt) on a dyadic grid: the host's symmetrisation then returns exactly these
    parameters, so kernel and oracle work with the same rule."""
    N, M = 2 * D + 1, D + 1
    u = rng.uniform(-0.5, 1.5, M)
    wms = _dyadic(u / (u[0] + 2 * u[1:].sum()))
    gam, beta = _dyadic(rng.standard_normal(D) / N), _dyadic(rng.choice([-1.0, 1.0], D) * rng.uniform(0.2, 1.0, D) / N)
    Mt = _dyadic(_factorable(rng, M))
    cls = [0] + [1 + k for k in range(D)] * 2
    wm = wms[cls]
    Wc = Mt[np.ix_(cls, cls)].copy()
    Wcc = np.zeros((D, N))
    for k in range(D):
        p, q = 1 + k, 1 + D + k
        Wc[p, p] += beta[k]
        Wc[q, q] += beta[k]
        Wc[p, q] -= beta[k]
        Wc[q, p] -= beta[k]
        Wcc[k, p], Wcc[k, q] = gam[k], -gam[k]
    return wm, Wc, Wcc, Mt


def permuted_rule(rule, perm):
    """The same rule with its points listed in another order (what makes the host's unscented-type test fail without changing the rule)."""
    r = dict(rule)
    perm = np.asarray(perm)
    r['xi'], r['wm'], r['Wcc'] = rule['xi'][:, perm].copy(), rule['wm'][perm].copy(), rule['Wcc'][:, perm].copy()
    r['Wc'] = rule['Wc'][np.ix_(perm, perm)].copy()
    if rule['iK'] is not None:
        r['iK'] = rule['iK'][np.ix_(perm, perm)].copy()
    return r


@functools.lru_cache(maxsize=None)
def rule_for(row):
    """dict(xi (D, N), wm (N,), Wc (N, N) or (N,), Wcc (D, N) or None, emv (E, E), emv_mode, nu, iK (N, N) or None) of one table row."""
    fid = MODELS[row.F][0]
    D, E, N = row.D, row.E, row.N
    xi = points_for(row.F, D, N, row.sel, _wants_ut(row))
    rule = None
    for attempt in range(200):
        rng = np.random.default_rng([20272, fid, D, N, row.sel, row.form, row.tp, row.opt, attempt])
        u = rng.uniform(-0.5, 1.5, N)
        if abs(u.sum()) < N / 4:
            continue
        wm = u / u.sum()
        if row.form == FORM_SIGMA:
            rule = dict(xi=xi, wm=wm, Wc=rng.choice([-1.0, 1.0], N) * rng.uniform(0.2, 1.0, N) / N, Wcc=None)
            break
        Wcc = rng.standard_normal((D, N)) / N
        if row.opt == 7:
            wm, Wc, Wcc, Mt = symmetric_rule(rng, D)
            if not (_ldl_accepts(Wc) and _ldl_accepts(Mt, upper=True, wmax=float(np.abs(Wc).max()))):
                continue
        elif row.opt in (3, 1):
            Wc = _factorable(rng, N)              # (not reflection-symmetric: OPT = 3 stays 3)
            if not _ldl_accepts(Wc):
                continue
        else:
            G = rng.standard_normal((N, N)) / N
            Wc = _mirror(G + G.T)
            if row.fast and not row.tp:
                Wc[0, 0] = 0.0                    # a zero leading pivot: the host refuses the LDL' and the dense kernel runs
        rule = dict(xi=xi, wm=wm, Wc=Wc, Wcc=Wcc)
        break
    assert rule is not None, row.name
    rng = np.random.default_rng([20273, fid, D, N, row.sel, row.form, row.tp, row.opt])
    G = rng.standard_normal((E, E))
    emv = _mirror(0.3 * (G + G.T))
    emv[np.arange(E), np.arange(E)] = rng.uniform(0.5, 1.5, E)
    G = rng.standard_normal((N, N))
    rule.update(emv=emv, emv_mode=EMV_BROADCAST if (E > 1 and (D + N + row.tp + row.opt) % 2) else EMV_DIAG,
                nu=TP_NU if row.tp else 0.0, iK=_mirror(G.dot(G.T) / N + 0.1 * np.eye(N)) if row.tp else None)
    for v in rule.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return rule


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def _spd(rng, n, cond, scale):
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    lam = scale * cond ** (-np.arange(n) / max(n - 1, 1))
    return _mirror((Q * lam).dot(Q.T))


@functools.lru_cache(maxsize=None)
def probes_for(F, D, sel):
    """Ten distinct probe items of a shape: mean (10, D), cov (10, D, D) symmetric, time (10,).  Probes 0..7: condition numbers 1 .. 1e3
    at the scale 1e-3 of the generic-route tests; probe 8: an ill-scaled diagonal 1e-6 .. 1 as in the reentry study (correlated, condition
    10 after scaling); probe 9: not positive definite (the last pivot is negative).  Every item has its own time."""
    fid, _, g0, jitter, descending = MODELS[F]
    rng = np.random.default_rng([20274, fid, D, sel])
    mean = np.array(g0[(D, sel)], dtype=float) + jitter * rng.standard_normal((N_PROBES, D))
    cov = np.empty((N_PROBES, D, D))
    for k in range(8):
        cov[k] = _spd(rng, D, 10.0 ** (3.0 * k / 7.0) if D > 1 else 1.0, 1e-3 * rng.uniform(0.5, 2.0))
    C = _spd(rng, D, 10.0 if D > 1 else 1.0, 1.0)
    var = np.logspace(-6.0, 0.0, D) if D > 1 else np.array([1e-6])
    s = np.sqrt((var[::-1] if descending else var) / np.diag(C))
    cov[ILL_PROBE] = _mirror(C * s[:, None] * s[None, :])
    cov[BAD_PROBE] = cov[3]
    cov[BAD_PROBE, D - 1, D - 1] = -cov[3, D - 1, D - 1]
    time = 0.5 + 1.75 * np.arange(N_PROBES) + rng.uniform(0.0, 1.0, N_PROBES)
    for a in (mean, cov, time):
        a.setflags(write=False)
    return mean, cov, time


def lane_probe(b, B=B_LANES):
    """Probe of lane b: the ten probes tiled over the lanes, the non-PD one also on the last lane."""
    return BAD_PROBE if b == B - 1 else b % N_PROBES


# ---- high-precision integrands ---------------------------------------------------------------------------------------------------
def _c(v):
    return mp.mpf(float(v))


def integrand_hp(fid, x, t, p=()):
    """oracle.ssmq_oracle.integrand in DPS digits: x, t lists / numbers of mpf, p float64 constants.  Returns (f, T): the values and, per
    output, the sum of the absolute values of the terms of the float64 evaluation (see the module's text)."""
    a = abs
    p = [_c(v) for v in p]
    if fid in (orc.F_UNGM_DYN, orc.F_UNGMNA_DYN):
        q = x[1] if fid == orc.F_UNGMNA_DYN else mp.mpf(1)
        th = _c(1.2) * t
        u, v, w = _c(0.5) * x[0], 25 * (x[0] / (1 + x[0] ** 2)), 8 * q * mp.cos(th)
        return [u + v + w], [a(u) + a(v) + a(w) + 8 * a(q) * a(mp.sin(th)) * a(th)]
    if fid == orc.F_UNGM_MEAS:
        v = _c(0.05) * x[0] ** 2
        return [v], [a(v)]
    if fid == orc.F_UNGMNA_MEAS:
        v = _c(0.05) * x[1] * x[0] ** 2
        return [v], [a(v)]
    if fid == orc.F_PENDULUM_DYN:
        dt, g = p[0], _c(9.81)
        u, v = x[1] * dt, g * dt * mp.sin(x[0])
        return [x[0] + u, x[1] - v], [a(x[0]) + a(u), a(x[1]) + a(v)]
    if fid == orc.F_PENDULUM_MEAS:
        v = mp.sin(x[0])
        return [v], [a(v)]
    if fid == orc.F_REENTRY1D_DYN:
        dt, gam = p[0], _c(1 / 6.096)
        arg = -gam * x[0]
        u, v = dt * x[1], dt * mp.exp(arg) * x[1] ** 2 * x[2]
        return [x[0] - u, x[1] - v, x[2]], [a(x[0]) + a(u), a(x[1]) + a(v) * (1 + a(arg)), a(x[2])]
    if fid == orc.F_RANGE_MEAS:
        v = mp.sqrt(_c(30.0) ** 2 + (x[0] - _c(30.0)) ** 2)
        return [v], [a(v)]
    if fid in (orc.F_REENTRY2D_DYN, orc.F_REENTRY2D_BIAS_DYN):
        dt = p[0]
        r0, h0, gm0, b0 = _c(6374.0), _c(13.406), _c(3.9860e5), _c(-0.59783)
        rr, vv = mp.sqrt(x[0] ** 2 + x[1] ** 2), mp.sqrt(x[2] ** 2 + x[3] ** 2)
        arg = (r0 - rr) / h0
        dr = b0 * mp.exp(x[4]) * mp.exp(arg) * vv
        gr = -gm0 / rr ** 3
        amp = 1 + a(arg) + a(x[4])
        out = [x[0] + dt * x[2], x[1] + dt * x[3], x[2] + dt * (dr * x[2] + gr * x[0]), x[3] + dt * (dr * x[3] + gr * x[1]), x[4]]
        T = [a(x[0]) + a(dt * x[2]), a(x[1]) + a(dt * x[3]), a(x[2]) + dt * (a(dr * x[2]) * amp + a(gr * x[0])),
             a(x[3]) + dt * (a(dr * x[3]) * amp + a(gr * x[1])), a(x[4])]
        if fid == orc.F_REENTRY2D_BIAS_DYN:
            out.append(x[5])
            T.append(a(x[5]))
        return out, T
    if fid == orc.F_RADAR2D_MEAS:
        lx, ly = (p[0], p[1]) if len(p) >= 2 else (mp.mpf(0), mp.mpf(0))
        r, th = mp.sqrt((x[0] - lx) ** 2 + (x[1] - ly) ** 2), mp.atan2(x[1] - ly, x[0] - lx)
        return [r, th], [a(r), a(th)]
    if fid == orc.F_CT_DYN:
        dt, om = p[0], x[4]
        sa, cb = mp.sin(om * dt), mp.cos(om * dt)
        c, d = sa / om, (1 - cb) / om
        dd = (1 + a(cb)) / a(om)                  # the rounding of 1 - cos(om dt), divided by om
        return ([x[0] + c * x[1] - d * x[3], cb * x[1] - sa * x[3], d * x[1] + x[2] + c * x[3], sa * x[1] + cb * x[3], x[4]],
                [a(x[0]) + a(c * x[1]) + dd * a(x[3]), a(cb * x[1]) + a(sa * x[3]), dd * a(x[1]) + a(x[2]) + a(c * x[3]),
                 a(sa * x[1]) + a(cb * x[3]), a(x[4])])
    if fid == orc.F_BEARING_MEAS:
        out = [mp.atan2(x[1] - p[2 * s + 1], x[0] - p[2 * s]) for s in range(len(p) // 2)]
        return out, [a(v) for v in out]
    if fid == orc.F_CTRS_DYN:
        dt = p[0]
        s, q = x[:5], x[5:7]
        h = _c(0.5) * dt ** 2
        if s[4] == 0:
            f0, f1 = dt * s[2] * mp.cos(s[3]), dt * s[2] * mp.sin(s[3])
            T0, T1 = a(f0), a(f1)
        else:
            c, th = s[2] / s[4], s[3] + s[4] * dt
            tha = a(s[3]) + a(s[4] * dt)          # the rounding of the argument s3 + s4 dt, which the difference does not damp
            f0 = c * (mp.sin(th) - mp.sin(s[3])) + h * mp.cos(s[3]) * q[0]
            f1 = c * (-mp.cos(th) + mp.cos(s[3])) + h * mp.sin(s[3]) * q[0]
            T0 = a(c) * (a(mp.sin(th)) + a(mp.sin(s[3])) + a(mp.cos(th)) * tha) + a(h * mp.cos(s[3]) * q[0])
            T1 = a(c) * (a(mp.cos(th)) + a(mp.cos(s[3])) + a(mp.sin(th)) * tha) + a(h * mp.sin(s[3]) * q[0])
        return ([s[0] + f0, s[1] + f1, s[2] + dt * q[0], s[3] + (dt * s[3] + h * q[1]), s[4] + dt * q[1]],
                [a(s[0]) + T0, a(s[1]) + T1, a(s[2]) + a(dt * q[0]), a(s[3]) + a(dt * s[3]) + a(h * q[1]), a(s[4]) + a(dt * q[1])])
    if fid == orc.F_CV_DYN:
        dt = p[0]
        return ([x[0] + dt * x[1], x[1], x[2] + dt * x[3], x[3]],
                [a(x[0]) + a(dt * x[1]), a(x[1]), a(x[2]) + a(dt * x[3]), a(x[3])])
    if fid == orc.F_SMOOTH10D_DYN:                # (no row of the small tables: the generic kernels' cases, tests/_apply_generic_oracle.py)
        sn, cs = [mp.sin(x[i]) for i in range(5)], [mp.cos(x[i]) for i in range(5)]
        lo, hi = [sn[i] + x[5 + i] ** 2 for i in range(5)], [x[5 + i] * cs[i] for i in range(5)]
        return lo + hi, [a(sn[i]) + x[5 + i] ** 2 for i in range(5)] + [a(v) for v in hi]
    raise ValueError(fid)


def _jacobian_hp(fid, xs, t, p):
    """|J| (E, DIN) and |df/dt| (E,) at one point by central differences in DPS digits (step 1e-15 of the coordinate's size: the
    truncation error is ~1e-30 relative, the rounding ~1e-35), as float64."""
    cols = []
    for d in range(len(xs) + 1):
        v = xs[d] if d < len(xs) else t
        h = mp.mpf(10) ** -15 * (abs(v) + mp.mpf(10) ** -3)
        lo, hi = list(xs), list(xs)
        tl = th = t
        if d < len(xs):
            lo[d], hi[d] = v - h, v + h
        else:
            tl, th = t - h, t + h
        fl, fh = integrand_hp(fid, lo, tl, p)[0], integrand_hp(fid, hi, th, p)[0]
        cols.append([float(abs((b - a_) / (2 * h))) for a_, b in zip(fl, fh)])
    J = np.array(cols).T
    return J[:, :-1], J[:, -1]


def _chol_hp(A):
    """Lower factor (rows of mpf) of the matrix whose lower triangle is A's, or None where a pivot is not positive."""
    n = len(A)
    L = [[mp.mpf(0)] * n for _ in range(n)]
    for j in range(n):
        d = A[j][j] - mp.fdot(L[j][:j], L[j][:j])
        if not d > 0:
            return None
        L[j][j] = mp.sqrt(d)
        for i in range(j + 1, n):
            L[i][j] = (A[i][j] - mp.fdot(L[i][:j], L[j][:j])) / L[j][j]
    return L


def _scaled_cond(cov):
    """2-norm condition number of the covariance scaled to unit diagonal (float64 eigenvalues: a scale needs its leading digits)."""
    cov = np.tril(cov) + np.tril(cov, -1).T
    s = 1.0 / np.sqrt(np.diag(cov))
    w = np.linalg.eigvalsh(cov * s[:, None] * s[None, :])
    return float(w[-1] / w[0])


_POINT_CACHE = {}


def points_hp(fid, p, sidx, xi, mean, cov, t):
    """What the three forms of a shape share for one input: None where cov is not positive definite, else dict(L, x, fx (lists of mpf),
    Lf, dxf (D, N) = x_n - m, fxf (E, N), dF (E, N), dX (D, N), cond) - the last four float64, dF / dX in units of eps."""
    key = (fid, tuple(p), sidx, xi.tobytes(), xi.shape, np.asarray(mean).tobytes(), np.tril(cov).tobytes(), float(t))
    if key in _POINT_CACHE:
        return _POINT_CACHE[key]
    with mp.workdps(DPS):
        D, N = xi.shape
        L = _chol_hp([[mp.mpf(float(v)) for v in r] for r in np.asarray(cov, dtype=float)])
        out = None
        if L is not None:
            m, tt = [mp.mpf(float(v)) for v in mean], mp.mpf(float(t))
            X = [[mp.mpf(float(v)) for v in xi[:, n]] for n in range(N)]
            dx = [[mp.fdot(L[d][:d + 1], X[n][:d + 1]) for d in range(D)] for n in range(N)]
            x = [[m[d] + dx[n][d] for d in range(D)] for n in range(N)]
            Lf = np.array([[float(v) for v in r] for r in L])
            cond = _scaled_cond(cov)
            dX = np.abs(np.asarray(mean, dtype=float))[:, None] + (1.0 + cond) * np.abs(Lf).dot(np.abs(xi))
            idx = list(range(DIN[fid])) if sidx is None else list(sidx)
            fx, dF = [], []
            for n in range(N):
                xs = [x[n][i] for i in idx]
                f, T = integrand_hp(fid, xs, tt, p)
                J, Jt = _jacobian_hp(fid, xs, tt, p)
                fx.append(f)
                dF.append(np.array([float(v) for v in T]) + J.dot(dX[idx, n]) + Jt * abs(float(t)))
            out = dict(L=L, x=x, fx=[[fx[n][e] for n in range(N)] for e in range(len(fx[0]))], Lf=Lf,
                       dxf=np.array([[float(v) for v in r] for r in dx]).T, dF=np.array(dF).T, dX=dX, cond=cond)
            out['fxf'] = np.array([[float(v) for v in r] for r in out['fx']])
    _POINT_CACHE[key] = out
    return out


# ---- one transform -------------------------------------------------------------------------------------------------------------------
def _fl(M):
    return np.array([[float(v) for v in r] for r in M]) if isinstance(M[0], list) else np.array([float(v) for v in M])


def transform_hp(fid, p, sidx, form, rule, mean, cov, t):
    """One moment transform from exact inputs.  Returns None where cov is not positive definite (reported, not raised), else
    (mean_f (E,), cov_f (E, E), cov_fx (E, D)) and the scales (A + S) of the same shapes, all float64."""
    pt = points_hp(fid, p, sidx, rule['xi'], mean, cov, t)
    if pt is None:
        return None
    xi, wm = rule['xi'], rule['wm']
    D, N = xi.shape
    F, dF, dX, Lf, aF = pt['fxf'], pt['dF'], pt['dX'], pt['Lf'], np.abs(pt['fxf'])
    E = F.shape[0]
    with mp.workdps(DPS):
        fx, L = pt['fx'], pt['L']
        w = [mp.mpf(float(v)) for v in wm]
        mf = [mp.fdot(fx[e], w) for e in range(E)]
        mff = _fl(mf)
        A_m, S_m = aF.dot(np.abs(wm)), dF.dot(np.abs(wm))
        if form == FORM_SIGMA:
            wc = rule['Wc']
            wch = [mp.mpf(float(v)) for v in wc]
            df = [[fx[e][n] - mf[e] for n in range(N)] for e in range(E)]
            wdf = [[wch[n] * df[e][n] for n in range(N)] for e in range(E)]
            dxh = [[pt['x'][n][d] - mp.mpf(float(mean[d])) for n in range(N)] for d in range(D)]
            cf = [[mp.fdot(wdf[e], df[e2]) for e2 in range(E)] for e in range(E)]
            cfx = [[mp.fdot(wdf[e], dxh[d]) for d in range(D)] for e in range(E)]
            adf, adx, awc = np.abs(_fl(df)), np.abs(pt['dxf']), np.abs(wc)
            ddf = dF + (A_m + S_m)[:, None] + adf        # rounding of f, of the mean subtracted from it, and of the difference itself
            A_c = (adf * awc).dot(adf.T)
            S_c = (ddf * awc).dot(adf.T) + (adf * awc).dot(ddf.T)
            A_x = (adf * awc).dot(adx.T)
            S_x = (ddf * awc).dot(adx.T) + (adf * awc).dot((dX + adx).T)
        else:
            Wc, Wcc, emv = rule['Wc'], rule['Wcc'], rule['emv']
            Wch = [[mp.mpf(float(v)) for v in r] for r in Wc]
            WcT = [[Wch[i][j] for i in range(N)] for j in range(N)]
            Tm = [[mp.fdot(fx[e], WcT[j]) for j in range(N)] for e in range(E)]          # fx Wc
            mask = np.ones((E, E)) if rule['emv_mode'] == EMV_BROADCAST else np.eye(E)
            em = [[mp.mpf(float(emv[e, e2] * mask[e, e2])) for e2 in range(E)] for e in range(E)]
            A_e, S_e = np.abs(emv * mask), np.zeros((E, E))
            if rule['nu'] > 0.0:
                iK, nu = rule['iK'], mp.mpf(float(rule['nu']))
                iKh = [[mp.mpf(float(v)) for v in r] for r in iK]
                Um = [[mp.fdot(fx[e], [iKh[i][j] for i in range(N)]) for j in range(N)] for e in range(E)]     # fx iK
                sq = [[mp.fdot(Um[e], fx[e2]) for e2 in range(E)] for e in range(E)]
                em = [[(nu - 2 + sq[e][e2]) / (nu - 2 + N) * em[e][e2] for e2 in range(E)] for e in range(E)]
                den = float(rule['nu']) - 2.0 + N
                Uf = np.abs(F.dot(iK))
                A_e = np.abs(emv * mask) * (abs(float(rule['nu']) - 2.0) + aF.dot(np.abs(iK)).dot(aF.T)) / den
                S_e = np.abs(emv * mask) * (dF.dot(np.abs(F.dot(iK.T)).T) + Uf.dot(dF.T)) / den
            cf = [[mp.fdot(Tm[e], fx[e2]) - mf[e] * mf[e2] + em[e][e2] for e2 in range(E)] for e in range(E)]
            Wcch = [[mp.mpf(float(v)) for v in r] for r in Wcc]
            Gm = [[mp.fdot(fx[e], Wcch[d]) for d in range(D)] for e in range(E)]          # fx Wcc'
            cfx = [[mp.fdot(Gm[e], L[d]) for d in range(D)] for e in range(E)]            # (fx Wcc') L'
            A_c = aF.dot(np.abs(Wc)).dot(aF.T) + np.abs(np.outer(mff, mff)) + A_e
            # d cov[e][e2] / d f[e][n] = (Wc f_e2')[n] - wm[n] mean[e2]   and   d / d f[e2][n] = (f_e Wc)[n] - wm[n] mean[e]
            g1 = np.abs(F.dot(Wc.T) - np.outer(mff, wm))
            g2 = np.abs(F.dot(Wc) - np.outer(mff, wm))
            S_c = dF.dot(g1.T) + g2.dot(dF.T) + S_e
            aL = np.abs(Lf)
            A_x = aF.dot(np.abs(Wcc).T).dot(aL.T)
            S_x = dF.dot(np.abs(Lf.dot(Wcc)).T) + np.abs(F.dot(Wcc.T)).dot((pt['cond'] * aL).T)
        out = (mff, _fl(cf), _fl(cfx))
    return out + (A_m + S_m, A_c + S_c, A_x + S_x)


def transform_f64(fid, p, sidx, form, rule, mean, cov, t):
    """The plain float64 restatement of the reference (NumPy): apply_sigma, or apply_bq with the (E, E) model variance - its diagonal
    through apply_bq's own model_var, the whole matrix (SSMQ_EMV_BROADCAST: I_out = eye(1)) added to the result; with the t-process
    variance the factor (nu - 2 + fx_e iK fx_e2') / (nu - 2 + N) on every entry kept, which on the diagonal is tp_emv_diag."""
    mean, cov = np.asarray(mean, dtype=float), np.asarray(cov, dtype=float)
    if form == FORM_SIGMA:
        return orc.apply_sigma(fid, mean, cov, t, rule['xi'], rule['wm'], rule['Wc'], p, sidx)
    w = dict(wm=rule['wm'], Wc=rule['Wc'], Wcc=rule['Wcc'], iK=rule['iK'], model_var=rule['emv'])
    tp = rule['nu'] if rule['nu'] > 0.0 else None
    if rule['emv_mode'] == EMV_DIAG:
        return orc.apply_bq(fid, mean, cov, t, rule['xi'], w, p, sidx, tp)
    w['model_var'] = 0.0
    mf, cf, cfx = orc.apply_bq(fid, mean, cov, t, rule['xi'], w, p, sidx)
    em = rule['emv']
    if tp is not None:
        L = np.linalg.cholesky(cov)
        fx = orc.eval_columns(fid, mean[:, None] + L.dot(rule['xi']), t, p, sidx)
        em = (tp - 2 + fx.dot(rule['iK']).dot(fx.T)) / (tp - 2 + fx.shape[1]) * em
    return mf, cf + em, cfx


# ---- the reference of one row: built once per session, never modified ---------------------------------------------------------
def model_of(row):
    fid, p = MODELS[row.F][:2]
    return fid, p, state_index(row)


def reference(row, rule=None):
    """Per probe: the oracle's (mean_f, cov_f, cov_fx, scale_mean, scale_cov, scale_cross) or None (not positive definite)."""
    return _reference(row) if rule is None else _build_reference(row, rule)


@functools.lru_cache(maxsize=None)
def _reference(row):
    return _build_reference(row, rule_for(row))


def _build_reference(row, rule):
    fid, p, sidx = model_of(row)
    mean, cov, time = probes_for(row.F, row.D, row.sel)
    out = []
    for k in range(N_PROBES):
        r = transform_hp(fid, p, sidx, row.form, rule, mean[k], cov[k], time[k])
        if r is not None:
            for a_ in r:
                a_.setflags(write=False)
        out.append(r)
    return tuple(out)


def ratios(got, ref):
    """Worst |got - ref| / (eps scale) of the three moments of one probe (an exact match is no error; a NaN is an infinite one)."""
    out = []
    for g, r, s in zip(got, ref[:3], ref[3:]):
        g = np.asarray(g, dtype=float)
        with np.errstate(invalid='ignore', divide='ignore'):
            q = np.abs(g - r) / (EPS * s)
        q = np.where(g == r, 0.0, q)
        out.append(float(np.max(np.where(np.isnan(q), np.inf, q))))
    return tuple(out)
