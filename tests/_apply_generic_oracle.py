"""The cases the three generic-shape transform kernels are pinned with - k_apply_tile (csrc/ssmq_apply_tile.hip), k_apply_wave and
k_apply_wide (csrc/ssmq_apply_wide.hip) - against the 50-digit restatement transform_hp of tests/_apply_small_oracle.py, which is
written for any D, E, N and state index.  Here: a LITERAL case table aimed at the places where these kernels change behaviour, the
restatement of the dispatch those places are read off (checked against the source text on the CPU), and the builders of rules and
probes.

Rules are random constants with no quadrature structure (unit points standard normal, wm of either sign, a symmetric Wc of either
sign for the BQ form and a positive diagonal for the centred one, random Wcc, an SPD iK with nu = 4.5 for the t-process form, both
emv modes across the table), seeded by the SHAPE: a shape that appears under several kernels or switches has one rule and one
reference.  Where D exceeds the model's own input count the integrand reads a state index that is not increasing and does not start
at 0; the selected entries sit at the model's operating point (MODELS of the small oracle), the others have standard-normal means.

Four probes per case, tiled over the lanes: 0 well conditioned (condition 10 at scale 1e-3), 1 condition 1e3, 2 an ill-scaled
diagonal 1e-6 .. 1 (descending for the coordinated-turn models: their turn rate keeps away from 0), 3 not positive definite.

The bar is K eps (A + S) with the scales of transform_hp and K = max(16, 8 K_REF_GENERIC), K_REF_GENERIC measured on the float64
NumPy restatement by tests/test_apply_generic_host.py (docs/KERNELS.md 3.2).

E > 10 does not occur: no built-in integrand has more than ten outputs."""
import collections
import functools
import os
import re

import numpy as np

from oracle import ssmq_oracle as orc
from tests import _apply_small_oracle as ao
from tests._apply_small_oracle import EPS, TP_NU, _spd, ratios, transform_f64, transform_hp      # noqa: F401

# Measured by tests/test_apply_generic_host.py::test_float64_restatement_within_k_ref_generic (2026-10-21): the worst ratio
# |float64 NumPy - oracle| / (eps (A + S)) over the 72 distinct shapes x 3 good probes is 0.593 (BQ: mean 0.57, cov 0.59, cross 0.22;
# BQ + t-process: 0.56, 0.35, 0.15; centred: 0.48, 0.21, 0.24; worst case: covariance of the radar measurement through the state index
# (12, 6) of a 13-dimensional state, N = 16, BQ form, the well-conditioned probe; by model: radar 0.59, bearings 0.57, SMOOTH10D 0.35,
# every other one below 0.3).  No case comes near 2: the scales need no further term at D = 16 or through a state index.
# K_REF_GENERIC is that rounded up; K follows by the rule of docs/KERNELS.md 3.1.
K_REF_GENERIC = 0.60
K_REF_WORST = 'k_apply_tile<16,4>G4-radar2d_meas-D13E2N16-BQ'
K = max(16.0, 8.0 * K_REF_GENERIC)
# Worst |device - oracle| / (eps (A + S)) per kernel and form, (mean, cov, cross-covariance), on an MI355X (2026-10-21, the table test
# of tests/test_apply_generic_gpu.py, which prints them after its last case): docs/KERNELS.md 3.2 and 3.7.
MEASURED_DEVICE = {('k_apply_tile', 'BQ'): (0.871, 0.593, 0.222), ('k_apply_tile', 'BQ+TP'): (0.664, 0.347, 0.185),
                   ('k_apply_tile', 'SIGMA'): (0.391, 0.116, 0.137), ('k_apply_wave', 'BQ'): (0.355, 0.222, 0.222),
                   ('k_apply_wave', 'BQ+TP'): (0.534, 0.217, 0.169), ('k_apply_wave', 'SIGMA'): (0.479, 0.152, 0.252),
                   ('k_apply_wide', 'BQ'): (0.379, 0.212, 0.144), ('k_apply_wide', 'BQ+TP'): (0.222, 0.0864, 0.169),
                   ('k_apply_wide', 'SIGMA'): (0.298, 0.0777, 0.252)}

N_PROBES, BAD_PROBE = 4, 3
TILE, WAVE, WIDE = 'k_apply_tile', 'k_apply_wave', 'k_apply_wide'
EXPECTED_CASES = 91

# ---- the dispatch, restated (test_apply_generic_host.py holds these against the source text) --------------------------------------
KSM_STEPS = ((16, 4), (24, 6), (32, 8), (52, 13))      # tile_ksm: N <= bound -> k-steps; above the last bound:
KSM_LAST = 16
DM_CLASSES = (4, 8, 12)                                # launch_tile_ks / launch_apply_wave: max(D, E) <= bound -> DM; above: 16
DM_LAST = 16                                           # (SSMQ_MAX_DIM)
SMOOTH_DM = 10                                         # SMOOTH10D without a state index and max(D, E) <= 10: <10, FC>
EXACT_SHAPE = (10, 10, 21)                             # ... in the BQ form without t-process at this shape: <10, 6, FC, 21>
TILE_WAVES, WAVE_WAVES, TILE_WGS_PER_CU, CUS = 4, 4, 2, 256
WIDE_SWITCH = 1024                                     # k_apply_wide<256> from E N >= 1024 on


def tile_ksm(N):
    for bound, ks in KSM_STEPS:
        if N <= bound:
            return ks
    return KSM_LAST


def tile_g(N):
    return min(4, 64 // N)


def dm_class(D, E):
    for bound in DM_CLASSES:
        if max(D, E) <= bound:
            return bound
    return DM_LAST


def tile_lds_bytes(D, E, N, tp, mrow):
    """tile_geom's LDS size of a workgroup (SSMQ_TILE_ALIAS = 0, no padding builds)."""
    ks = tile_ksm(N)
    ksp, nb, g = ks | 1, (ks + 3) // 4, tile_g(N)
    frag = (64 * ((2 if tp else 1) * nb * ks + (1 if mrow else 2) * ks) + N * (D | 1) + 1) & ~1
    per_traj = D * D + D + E * 4 * ksp + E + E * E + E * D
    wave = (g * per_traj + 2 + 64 + 16 + 1) & ~1
    return 8 * (frag + TILE_WAVES * wave)


def wave_slice_bytes(D, E, N, tp):
    """wave_lds_doubles, rounded up to even: the LDS slice of one trajectory of k_apply_wave."""
    m = max(D, E)
    return 8 * ((D * D + D + E + E * m + (E * E if tp else 0) + (E + m) * N + 2 + 1) & ~1)


def wave_k(D, E, N, tp, env=()):
    """wave_groups: trajectories side by side in one wave of k_apply_wave."""
    env = dict(env)
    if 'SSMQ_WAVE_K' in env:
        return max(1, min(64 // N, int(env['SSMQ_WAVE_K'])))
    return max(1, min(64 // N, ((160 * 1024) // 12) // wave_slice_bytes(D, E, N, tp)))


def parsed_dispatch():
    """What the source text says of the same: dict(ksm, ksm_last, g, dm_tile, dm_wave, wgs_per_cu, tile_waves, wave_waves, wide_switch)."""
    def read(name):
        with open(os.path.join(ao.CSRC, name)) as fh:
            return fh.read()
    tile, wide = read('ssmq_apply_tile.hip'), read('ssmq_apply_wide.hip')
    line = re.search(r'int tile_ksm\(int N\) \{\s*return ([^;]+);', tile).group(1)
    steps = tuple((int(a), int(b)) for a, b in re.findall(r'N <= (\d+) \? (\d+) :', line))
    last = int(re.search(r': (\d+)$', line.strip()).group(1))

    def body(text, head):
        i = text.index(head)
        return text[i:text.index('\n}', i)]
    pat = re.compile(r'dm <= (\d+)\)\s*(?:return|e =) launch_(?:tile|wave)_one<(\d+|SSMQ_MAX_DIM)')
    tail = re.compile(r'(?:return|else e =) launch_(?:tile|wave)_one<(\d+|SSMQ_MAX_DIM), (?:KS, )?-1>\(a, B, s\);\s*(?:return e;\s*)?$')

    def classes(b):
        return tuple((int(x), int(y)) for x, y in pat.findall(b)), tail.search(b.rstrip()).group(1)
    return dict(ksm=steps, ksm_last=last, g='g.G = 64 / N < 4 ? 64 / N : 4;' in tile,
                dm_tile=classes(body(tile, 'hipError_t launch_tile_ks(')), dm_wave=classes(body(wide, 'static hipError_t launch_apply_wave(')),
                exact='a.D == 10 && a.E == 10 && a.N == 21 && a.form == SSMQ_FORM_BQ && !(a.tp_nu > 0.0)' in tile,
                wgs_per_cu=int(re.search(r'#define SSMQ_TILE_WGS_PER_CU (\d+)', tile).group(1)),
                cap='const int64_t cap = 256 * SSMQ_TILE_WGS_PER_CU;' in tile,
                tile_waves=int(re.search(r'constexpr int kTileWaves = (\d+);', tile).group(1)),
                wave_waves=int(re.search(r'constexpr int kWaveWaves = (\d+);', wide).group(1)),
                wide_switch=int(re.search(r'\(int64_t\)a\.E \* a\.N >= (\d+)', wide).group(1)))


# ---- the cases -------------------------------------------------------------------------------------------------------------------
Case = collections.namedtuple('Case', 'kernel env F D sidx E N form tp')
_NT, _NW, _NM, _MROW, _EXACT = (('SSMQ_NO_TILE', '1'),), (('SSMQ_NO_WAVE', '1'),), (('SSMQ_NO_MFMA', '1'),), (('SSMQ_TILE_NO_MROW', '1'),), \
    (('SSMQ_TILE_NO_EXACT', '1'),)
_I12, _I15, _I16 = (11, 0, 3, 4, 7, 1, 9, 10, 2, 6), (14, 0, 3, 4, 7, 1, 9, 12, 2, 6), (15, 0, 3, 13, 7, 1, 9, 10, 2, 6)
_U, _CV, _PD, _RE, _CT, _CTRS, _BE, _RA, _SM = ('SSMQ_F_UNGM_DYN', 'SSMQ_F_CV_DYN', 'SSMQ_F_PENDULUM_DYN', 'SSMQ_F_REENTRY2D_DYN', 'SSMQ_F_CT_DYN',
                                               'SSMQ_F_CTRS_DYN', 'SSMQ_F_BEARING_MEAS', 'SSMQ_F_RADAR2D_MEAS', 'SSMQ_F_SMOOTH10D_DYN')
# (kernel wanted, switches, model, D, state index, E, N, forms: B = BQ, T = BQ with the t-process variance, S = centred)
TABLE = (
    # k_apply_tile, one shape per (DM class, KS class), all three forms.  DM 4:
    (TILE, (), _U, 1, None, 1, 9, 'BTS'), (TILE, (), _CV, 4, None, 4, 17, 'BTS'), (TILE, (), _PD, 4, (3, 1), 2, 25, 'BTS'),
    (TILE, (), _CV, 4, None, 4, 52, 'BTS'), (TILE, (), _U, 1, None, 1, 53, 'BTS'),
    # DM 8 (bearings with 4 and with 8 sensors):
    (TILE, (), _RE, 5, None, 5, 16, 'BTS'), (TILE, (), _CT, 5, None, 5, 21, 'BTS'), (TILE, (), _CTRS, 7, None, 5, 32, 'BTS'),
    (TILE, (), _BE, 8, (5, 2), 4, 33, 'BTS'), (TILE, (), _BE, 5, (3, 1), 8, 53, 'BTS'),
    # DM 12:
    (TILE, (), _RA, 9, (7, 2), 2, 9, 'BTS'), (TILE, (), _BE, 11, (9, 4), 4, 24, 'BTS'), (TILE, (), _SM, 12, _I12, 10, 25, 'BTS'),
    (TILE, (), _RA, 12, (10, 3), 2, 52, 'BTS'), (TILE, (), _BE, 12, (8, 5), 8, 64, 'BTS'),
    # DM 16: D = 15 is the last shape whose mean rides in the Wcc operand, D = 16 takes the separate sum; the last one is the largest
    # LDS slice there is (132 KB with the t-process fragments)
    (TILE, (), _RA, 13, (12, 6), 2, 16, 'BTS'), (TILE, (), _SM, 15, _I15, 10, 22, 'BTS'), (TILE, (), _BE, 16, (15, 7), 4, 32, 'BTS'),
    (TILE, (), _RA, 15, (13, 4), 2, 33, 'BTS'), (TILE, (), _SM, 16, _I16, 10, 64, 'BTS'),
    # a D <= 15 shape without the mean row; second appearances of N = 22 and 24
    (TILE, _MROW, _CV, 4, None, 4, 17, 'B'), (TILE, (), 'SSMQ_F_REENTRY2D_BIAS_DYN', 6, None, 6, 22, 'B'),
    (TILE, (), 'SSMQ_F_UNGMNA_DYN', 2, None, 1, 24, 'S'),
    # the compile-time integrand: exact shape, the same on the run-time-shape body, and <10, 6, FC> at the shapes that are not exact
    (TILE, (), _SM, 10, None, 10, 21, 'BTS'), (TILE, _EXACT, _SM, 10, None, 10, 21, 'B'), (TILE, (), _SM, 10, None, 10, 20, 'B'),
    # k_apply_wave behind SSMQ_NO_TILE: N = 9, 16, 21, 22, 32, 33, 64, the four DM classes and <10, FC>
    (WAVE, _NT, _U, 1, None, 1, 9, 'B'), (WAVE, _NT, _RE, 5, None, 5, 16, 'T'), (WAVE, _NT, _CT, 5, None, 5, 21, 'S'),
    (WAVE, _NT, _SM, 15, _I15, 10, 22, 'B'), (WAVE, _NT, _CTRS, 7, None, 5, 32, 'B'), (WAVE, _NT, _BE, 8, (5, 2), 4, 33, 'S'),
    (WAVE, _NT, _SM, 16, _I16, 10, 64, 'T'), (WAVE, _NT, _SM, 12, _I12, 10, 25, 'B'), (WAVE, _NT, _RA, 9, (7, 2), 2, 9, 'T'),
    (WAVE, _NT, _SM, 10, None, 10, 21, 'B'),
    # one and the most trajectories per wave
    (WAVE, _NT + (('SSMQ_WAVE_K', '1'),), _U, 1, None, 1, 9, 'B'), (WAVE, _NT + (('SSMQ_WAVE_K', '7'),), _U, 1, None, 1, 9, 'B'),
    # N <= 8 without a register specialisation: this kernel by default
    (WAVE, (), _CV, 4, None, 4, 7, 'B'), (WAVE, (), 'SSMQ_F_REENTRY1D_DYN', 3, None, 3, 8, 'T'), (WAVE, (), 'SSMQ_F_UNGM_MEAS', 1, None, 1, 4, 'S'),
    # k_apply_wide behind SSMQ_NO_WAVE; N <= 64 keeps E N below 1024 (E <= 10), so the <64> | <256> switch is crossed at N > 64, where
    # SSMQ_NO_MFMA keeps the matrix-core routes away: E N = 1016 | 1024 and 1030, run at B = 5
    (WIDE, _NW, _SM, 16, _I16, 10, 64, 'T'), (WIDE, _NW, _BE, 12, (8, 5), 8, 64, 'B'), (WIDE, _NW, _U, 1, None, 1, 9, 'S'),
    (WIDE, _NW, _CT, 5, None, 5, 21, 'BS'),
    (WIDE, _NM, _BE, 5, (3, 1), 8, 127, 'B'), (WIDE, _NM, _BE, 5, (3, 1), 8, 128, 'B'), (WIDE, _NM, _SM, 10, None, 10, 103, 'T'),
)
_FORMS = {'B': (ao.FORM_BQ, 0), 'T': (ao.FORM_BQ, 1), 'S': (ao.FORM_SIGMA, 0)}
CASES = tuple(Case(*(r[:7] + _FORMS[f])) for r in TABLE for f in r[7])

_SENS8 = ao._SENS + (1000.0, 1000.0, -1000.0, 1000.0, -1000.0, -1000.0, 1000.0, -1000.0)
_SMOOTH_OP = (0.4, -0.7, 1.1, 0.2, -1.3, 0.8, -0.5, 1.2, 0.3, -0.9)


def form_tag(case):
    return 'SIGMA' if case.form == ao.FORM_SIGMA else ('BQ+TP' if case.tp else 'BQ')


def shape_of(case):
    """What rule and reference depend on."""
    return (case.F, case.D, case.sidx, case.E, case.N, case.form, case.tp)


def instance(case):
    """The instantiation the case is aimed at, as the test id states it."""
    env = dict(case.env)
    if case.kernel == WIDE:
        return '<%d>' % (256 if case.E * case.N >= WIDE_SWITCH else 64)
    smooth = case.F == _SM and case.sidx is None and max(case.D, case.E) <= SMOOTH_DM
    if case.kernel == WAVE:
        return '<%s>K%d' % ('10,FC' if smooth else '%d' % dm_class(case.D, case.E), wave_k(case.D, case.E, case.N, case.tp, case.env))
    ks = tile_ksm(case.N)
    smooth = smooth and ks == 6
    exact = smooth and (case.D, case.E, case.N) == EXACT_SHAPE and case.form == ao.FORM_BQ and not case.tp and \
        'SSMQ_TILE_NO_EXACT' not in env and 'SSMQ_TILE_NO_MROW' not in env
    return '<%s,%d%s>G%d' % (('10' if smooth else '%d' % dm_class(case.D, case.E)), ks, ',FC,21' if exact else (',FC' if smooth else ''), tile_g(case.N))


def case_id(case):
    f = case.F.replace('SSMQ_F_', '').lower()
    sw = ''.join('-' + k.replace('SSMQ_', '') + ('' if v == '1' else v) for k, v in case.env)
    return '%s%s-%s-D%dE%dN%d-%s%s' % (case.kernel, instance(case), f, case.D, case.E, case.N, form_tag(case), sw)


def uses_mrow(case):
    return case.form == ao.FORM_BQ and case.D <= 15 and 'SSMQ_TILE_NO_MROW' not in dict(case.env)


def lanes_per_round(case):
    """Trajectories one workgroup (tile: 4 G) / one block (wave: 4 K) takes at a time; k_apply_wide takes one."""
    if case.kernel == TILE:
        return TILE_WAVES * tile_g(case.N)
    if case.kernel == WAVE:
        return WAVE_WAVES * wave_k(case.D, case.E, case.N, case.tp, case.env)
    return 1


def batch_of(case):
    """Three full rounds and a ragged one with an odd count just above half a round (r is a multiple of 4); B = 5 beyond 64 points (below
    the matrix-core routes' minimum), 13 otherwise for the kernel of one workgroup per trajectory."""
    r = lanes_per_round(case)
    if case.kernel == WIDE:
        return 5 if case.N > 64 else 13
    return 3 * r + r // 2 + 1


def lane_probe(b, B):
    return BAD_PROBE if b == B - 1 else b % N_PROBES


def model_of(case):
    """(oracle id, constants, state index)."""
    if case.F == _SM:
        return orc.F_SMOOTH10D_DYN, (), case.sidx
    fid, p = ao.MODELS[case.F][:2]
    if fid == orc.F_BEARING_MEAS and case.E == 8:
        p = _SENS8
    return fid, tuple(p), case.sidx


def _operating_point(F, D, sidx):
    """(values, jitter, descending, positions): the model's own operating point and where in the state its entries sit."""
    if F == _SM:
        op, jitter, desc = list(_SMOOTH_OP), 0.5, False
    else:
        fid, _, g0, jitter, desc = ao.MODELS[F]
        if sidx is None and (D, 0) in g0:
            return list(g0[(D, 0)]), jitter, desc, list(range(D))
        full = sorted((k, v) for k, v in g0.items() if k[1] == 0)[0][1]
        op = list(full[:ao.DIN[fid]])
    pos = list(range(len(op))) if sidx is None else list(sidx)
    assert len(pos) == len(op) and max(pos) < D, (F, D, sidx)
    return op, jitter, desc, pos


@functools.lru_cache(maxsize=None)
def probes_for(F, D, sidx):
    """mean (4, D), cov (4, D, D) symmetric, time (4,) - see the module's text."""
    op, jitter, desc, pos = _operating_point(F, D, sidx)
    fid = orc.F_SMOOTH10D_DYN if F == _SM else ao.MODELS[F][0]
    rng = np.random.default_rng([20281, fid, D] + list(sidx or ()))
    mean = rng.standard_normal((N_PROBES, D))
    mean[:, pos] = np.array(op) + jitter * rng.standard_normal((N_PROBES, len(pos)))
    cov = np.empty((N_PROBES, D, D))
    cov[0] = _spd(rng, D, 10.0 if D > 1 else 1.0, 1e-3 * rng.uniform(0.5, 2.0))
    cov[1] = _spd(rng, D, 1e3 if D > 1 else 1.0, 1e-3 * rng.uniform(0.5, 2.0))
    C = _spd(rng, D, 10.0 if D > 1 else 1.0, 1.0)
    v = np.logspace(-6.0, 0.0, D) if D > 1 else np.array([1e-6])
    v = v[::-1] if desc else v
    rest = [d for d in range(D) if d not in pos]
    var = np.empty(D)
    var[pos + rest] = v                              # the model's entries take the leading variances in the model's own order
    s = np.sqrt(var / np.diag(C))
    cov[2] = ao._mirror(C * s[:, None] * s[None, :])
    cov[BAD_PROBE] = cov[0]
    cov[BAD_PROBE, D - 1, D - 1] = -cov[0, D - 1, D - 1]
    time = 0.5 + 1.75 * np.arange(N_PROBES) + rng.uniform(0.0, 1.0, N_PROBES)
    for a in (mean, cov, time):
        a.setflags(write=False)
    return mean, cov, time


@functools.lru_cache(maxsize=None)
def _points(fid, D, sidx, E, N):
    xi = np.random.default_rng([20282, fid, D, E, N] + list(sidx or ())).standard_normal((D, N))
    xi.setflags(write=False)
    return xi


@functools.lru_cache(maxsize=None)
def _rule(shape):
    F, D, sidx, E, N, form, tp = shape
    fid = orc.F_SMOOTH10D_DYN if F == _SM else ao.MODELS[F][0]
    xi = _points(fid, D, sidx, E, N)
    rng = np.random.default_rng([20283, fid, D, E, N, form, tp] + list(sidx or ()))
    while True:
        u = rng.uniform(-0.5, 1.5, N)
        if abs(u.sum()) >= N / 4 and u.min() < 0.0:
            break
    wm = u / u.sum()
    if form == ao.FORM_SIGMA:
        rule = dict(xi=xi, wm=wm, Wc=rng.uniform(0.2, 1.0, N) / N, Wcc=None)
    else:
        G = rng.standard_normal((N, N)) / N
        rule = dict(xi=xi, wm=wm, Wc=ao._mirror(G + G.T), Wcc=rng.standard_normal((D, N)) / N)
    G = rng.standard_normal((E, E))
    emv = ao._mirror(0.3 * (G + G.T))
    emv[np.arange(E), np.arange(E)] = rng.uniform(0.5, 1.5, E)
    G = rng.standard_normal((N, N))
    rule.update(emv=emv, emv_mode=ao.EMV_BROADCAST if (E > 1 and (D + N + tp) % 2) else ao.EMV_DIAG, nu=TP_NU if tp else 0.0,
                iK=ao._mirror(G.dot(G.T) / N + 0.1 * np.eye(N)) if tp else None)
    for a in rule.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return rule


def rule_for(case):
    return _rule(shape_of(case))


@functools.lru_cache(maxsize=None)
def _reference(shape):
    F, D, sidx, E, N, form, tp = shape
    case = Case(None, (), F, D, sidx, E, N, form, tp)
    fid, p, _ = model_of(case)
    mean, cov, time = probes_for(F, D, sidx)
    out = []
    for k in range(N_PROBES):
        r = transform_hp(fid, p, sidx, form, _rule(shape), mean[k], cov[k], time[k])
        if r is not None:
            for a in r:
                a.setflags(write=False)
        out.append(r)
    return tuple(out)


def reference(case):
    """Per probe: the oracle's (mean_f, cov_f, cov_fx, scale_mean, scale_cov, scale_cross), or None (not positive definite).  Built once
    per shape and session, never modified."""
    return _reference(shape_of(case))
