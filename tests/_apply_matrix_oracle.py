"""The cases the matrix-core transform routes for more than 64 points are pinned with - k_bq_fused (csrc/ssmq_bq_fused.hip), the two-
and three-pass routes over k_eval_wave / k_fxwc_cov_mfma / k_fxwc_mfma (csrc/ssmq_gemm_mfma.hip), k_bq_stream (csrc/ssmq_bq_stream.hip)
and the blocked route k_apply_big (csrc/ssmq_apply_big.hip) - against the 50-digit restatement transform_hp of
tests/_apply_small_oracle.py.  Here: a LITERAL case table aimed at the edges of those routes, the restatement of the dispatch the edges
are read off (held against the source text on the CPU by tests/test_apply_matrix_host.py), and the builders of rules and probes.

Rules are random constants with no quadrature structure, seeded by the SHAPE (a shape listed under several routes or switches has one
rule and one reference): unit points standard normal, wm of either sign, and - unlike the generic table - magnitudes spread over three
decades: |Wc_ij| and |Wcc_dn| are |randn| 10^U(-3, 0) / N, wm_n carries 10^U(-2, 0), so that a term dropped, doubled or misplaced is
not drowned by terms of one common size.  Wc is symmetric to the last bit in the forms B and T; the form N perturbs the strict upper
triangle (the host then refuses the routes built on S = tril(Wc)); the reference uses the rule as given and, as the kernels do,
mirrors the lower triangle of (fx Wc) fx'.  Centred form S: a positive spread diagonal.  D above the model's input count goes
through a state index that is not increasing and does not start at 0.  The four probes are those of the generic table.

The bar is K eps (A + S) with the scales of transform_hp and K = max(16, 8 K_REF_MATRIX), K_REF_MATRIX measured on the float64 NumPy
restatement by tests/test_apply_matrix_host.py (docs/KERNELS.md 3.1).  The host-supplied cases (ssmq_apply_fx_batch, E up to 16) have
the linear algebra alone as their reference: exact inputs, so S = 0 and the scale is A.

E = 9 does not occur: no built-in integrand has nine outputs (bearings: 1 .. 8 sensors; SMOOTH10D: 10), and a user-defined
integrand runs on k_apply_small only.

Reference cost: all distinct shapes (REFERENCE_SECONDS below) are built once per process (lru_cache) and shared by the device and
the host tests; E N^2 stays below 1e6 per shape."""
import collections
import functools
import os
import re

import mpmath as mp
import numpy as np

from oracle import ssmq_oracle as orc
from tests import _apply_generic_oracle as go
from tests import _apply_small_oracle as ao
from tests._apply_small_oracle import EPS, TP_NU, ratios, transform_f64, transform_hp      # noqa: F401

# Measured by tests/test_apply_matrix_host.py::test_float64_restatement_within_k_ref_matrix (2026-10-21): the worst ratio
# |float64 NumPy - oracle| / (eps (A + S)) over the 44 distinct shapes x 3 good probes and the 5 host-supplied cases x 3 probes is 1.183,
# the cross-covariance (fx Wcc') L' - a chain of two products - of the host-supplied case D = 4, E = 11, N = 120.  The transforms of the
# table stay below 0.90 (mean of a k_bq_fused case; covariances 0.68 at most, t-process form on k_apply_big): no shape stands out, the
# scales need no further term for the spread weights or for N = 551.  K_REF_MATRIX is that rounded up; K by docs/KERNELS.md 3.1.
K_REF_MATRIX = 1.19
K_REF_WORST = 'fx-three-pass-D4E11N120'
K = max(16.0, 8.0 * K_REF_MATRIX)
# Building every reference of the table on one CPU core (pure-Python mpmath), seconds:
REFERENCE_SECONDS = 115
# Worst |device - oracle| / (eps (A + S)) per route and form, (mean, cov, cross-covariance), on an MI355X (the table test of
# tests/test_apply_matrix_gpu.py prints them after its last case): docs/KERNELS.md 3.6, 3.8, 3.10, 3.12.
MEASURED_DEVICE = {('k_bq_fused', 'BQ'): (1.51, 0.479, 0.284), ('k_bq_stream', 'BQ'): (1.34, 0.167, 0.285),
                   ('two-pass', 'BQ'): (0.331, 0.305, 0.36), ('two-pass', 'BQ-nonsym'): (0.181, 0.055, 0.285),
                   ('three-pass', 'BQ'): (0.188, 0.0746, 0.0907), ('three-pass', 'BQ+TP'): (0.217, 0.0877, 0.331),
                   ('k_apply_big', 'BQ'): (0.323, 0.232, 0.218), ('k_apply_big', 'BQ+TP'): (0.194, 0.106, 0.203),
                   ('k_apply_big', 'BQ-nonsym'): (0.35, 0.076, 0.285), ('k_apply_big', 'SIGMA'): (0.181, 0.0531, 0.0307),
                   ('fx two-pass', 'BQ'): (0.627, 0.722, 2.11), ('fx three-pass', 'BQ'): (0.613, 0.605, 2.5),
                   ('fx k_apply_big', 'BQ'): (0.363, 0.655, 2.6)}

N_PROBES, BAD_PROBE = go.N_PROBES, go.BAD_PROBE
FUSED, TWO, THREE, STREAM, BIG, WIDE = 'k_bq_fused', 'two-pass', 'three-pass', 'k_bq_stream', 'k_apply_big', 'k_apply_wide'
KERNEL_NAME = {FUSED: 'k_bq_fused', TWO: 'k_apply_wide', THREE: 'k_apply_wide', STREAM: 'k_bq_stream', BIG: 'k_apply_big', WIDE: 'k_apply_wide'}
EXPECTED_CASES = 49
EXPECTED_FX_CASES = 5

# ---- the dispatch, restated (test_apply_matrix_host.py holds these against the source text) ---------------------------------------
GEMM_TILES = (8, 13, 16)                  # gemm_mfma_padded: ceil(N / 16) in these -> 16 times that, else 0
GEMM_MIN_ROWS = 256                       # kGemmMinRows: B E from which a batch takes the matrix-core routes
BIG_COLS = 256                            # kBigCols: columns of one block of the blocked GEMM
LDS_BOUND = 160 * 1024 - 64               # the LDS-resident generic kernel fits up to here
FUSED_PADDED, FUSED_D_MAX, FUSED_E = (128, 208), 15, (6, 10)
FUSED_DM_SMALL, FUSED_DM_SMOOTH, MAX_DIM = 8, 10, 16
STREAM_MIN_N, STREAM_MAX_N, STREAM_D_MAX, STREAM_E_MAX, PANEL_COLS = 208, 4096, 15, 10, 256
SPLIT_NUM, SPLIT_DEN = 3, 5               # bq_stream_split: a last round of at most 3/5 of the compute units is cut by panel


def gemm_mfma_padded(N):
    nt = (N + 15) // 16
    return 16 * nt if nt in GEMM_TILES else 0


def fxwc_cov_supported(E):
    """Every trajectory that meets a 16-row tile lies inside the 32 rows from the first such trajectory on."""
    if E < 1 or E > 16:
        return False
    for a in range(E):
        s0 = (16 * a // E) * E
        last = ((16 * a + 15) // E) * E + E
        if last - s0 > 32:
            return False
    return True


def fused_dm(D, E, smooth=False):
    """The compile-time bound on D and E of a k_bq_fused launch: register Cholesky up to 8, 10 for the compile-time integrand."""
    dm = max(D, E)
    if smooth and dm <= FUSED_DM_SMOOTH:
        return FUSED_DM_SMOOTH
    return FUSED_DM_SMALL if dm <= FUSED_DM_SMALL else MAX_DIM


def fused_geom(NT, D, E, DM, waves=8):
    """(trajectories per workgroup, LDS bytes) of fused_geom_for."""
    NP, RT, KS = 16 * NT, waves // 2, 2 * waves
    LB, FP, cap = NP + 16 + 4, NP + 2, 160 * 1024
    tpw, lds = 16 * RT // E, 0
    while tpw >= 1:
        lds = 8 * (tpw * E * FP + 2 * KS * LB + 16 * RT + tpw * (DM * (DM + 1) // 2 + DM)) + 4 * (16 + 16 * RT)
        if lds <= cap:
            break
        tpw -= 1
    return tpw, lds


def fused_geom_ok(tpw, NT, D, E, waves=8):
    RT, KS = waves // 2, 2 * waves
    slab = 2 * KS * (16 * NT + 20)
    return tpw >= 1 and 4 * tpw * E >= 3 * 16 * RT and tpw * D * D <= slab and 2 * RT * 64 * 8 + 512 + 32 <= slab


def bq_fused_supported(D, E, N, env=()):
    if 'SSMQ_NO_BQ_FUSED' in dict(env):
        return False
    np_ = gemm_mfma_padded(N)
    if np_ not in FUSED_PADDED:
        return False
    if D < 1 or D > FUSED_D_MAX or E < FUSED_E[0] or E > FUSED_E[1] or not fxwc_cov_supported(E):
        return False
    return fused_geom_ok(fused_geom(np_ // 16, D, E, fused_dm(D, E))[0], np_ // 16, D, E)


def fused_tpw(D, E, N, smooth=False):
    """Trajectories per workgroup of launch_bq_fused (the instantiation's own bound first, the generic one where that does not fit)."""
    nt = gemm_mfma_padded(N) // 16
    tpw = fused_geom(nt, D, E, fused_dm(D, E, smooth))[0]
    return tpw if fused_geom_ok(tpw, nt, D, E) else fused_geom(nt, D, E, fused_dm(D, E))[0]


def bq_stream_supported(D, E, N, env=()):
    env = dict(env)
    if 'SSMQ_NO_BQ_STREAM' in env or 'SSMQ_NO_MFMA' in env:
        return False
    if N <= STREAM_MIN_N or N > STREAM_MAX_N:
        return False
    return 1 <= D <= STREAM_D_MAX and 1 <= E <= STREAM_E_MAX


def bq_stream_tpw(E):
    return 64 // E


def bq_stream_panels(N):
    return (N + PANEL_COLS - 1) // PANEL_COLS


def bq_stream_split(nblocks, npan, cus):
    """(blocks run whole, blocks of the last round cut by panel)."""
    rem = nblocks % cus if cus >= 1 else 0
    if npan < 2 or cus < 1 or rem == 0 or SPLIT_DEN * rem > SPLIT_NUM * cus:
        return nblocks, 0
    return nblocks - rem, rem


def wide_lds_bytes(D, E, N):
    return 8 * (D * D + D + D * N + 2 * E * N + E + 2 * E * E + E * D)


def centred_first_big_n(D, E):
    """The smallest N whose centred form no longer fits the LDS-resident kernel: 8 (D D + D + E + 2 E E + E D + (D + 2 E) N) > bound."""
    fixed = D * D + D + E + 2 * E * E + E * D
    return (LDS_BOUND // 8 - fixed) // (D + 2 * E) + 1


def route(D, E, N, form, tp, symmetric, env=(), rows=1 << 20):
    """apply_dev_impl's choice for a shape without a register specialisation: streamed before big before one_launch, then the passes
    over the padded GEMM, then the workgroup kernel.  `rows` = B E (the name query reports the route of a large batch)."""
    envd = dict(env)
    bq, mfma = form == ao.FORM_BQ, 'SSMQ_NO_MFMA' not in envd
    np_ = gemm_mfma_padded(N) if bq else 0
    wc_pad = bool(np_) and mfma
    sx_pad = wc_pad and symmetric
    sx_pan = bq and bq_stream_supported(D, E, N, env) and not tp and symmetric
    wc_blk = bq and N > 64 and not np_ and mfma
    fits = wide_lds_bytes(D, E, N) <= LDS_BOUND
    enough = rows >= GEMM_MIN_ROWS
    big = N > 64 and ((bq and wc_blk and (enough or not fits)) or (not bq and not fits))
    streamed = bq and not tp and sx_pan and enough
    one_launch = not big and bq and wc_pad and sx_pad and not tp and enough and bq_fused_supported(D, E, N, env)
    if streamed:
        return STREAM
    if big:
        return BIG
    if one_launch:
        return FUSED
    if wc_pad and enough:
        if not tp and fxwc_cov_supported(E) and D <= 16 and 'SSMQ_NO_FUSED_COV' not in envd:
            return TWO
        return THREE
    return WIDE


def _squash(text):
    return re.sub(r'\s+', ' ', text)


def parsed_dispatch():
    """What the source text says of the same: numbers read out of it, and whether the statements restated above stand in it."""
    def read(name):
        root = os.path.join(os.path.dirname(os.path.dirname(ao.CSRC)), 'include') if name == 'ssmq.h' else ao.CSRC
        with open(os.path.join(root, name)) as fh:
            return _squash(fh.read())
    gemm, fused, strm, api, wide, host = (read(n) for n in ('ssmq_gemm_mfma.hip', 'ssmq_bq_fused.hip', 'ssmq_bq_stream.hip',
                                                            'ssmq_api_transform.hip', 'ssmq_apply_wide.hip', 'ssmq_host.h'))
    has = lambda text, s: _squash(s) in text
    return dict(
        tiles=tuple(int(v) for v in re.search(r'return \(nt == (\d+) \|\| nt == (\d+) \|\| nt == (\d+)\) \? nt \* 16 : 0;', gemm).groups()),
        cov_window=all(has(gemm, s) for s in ('if (E < 1 || E > 16) return false;', 'for (int a = 0; a < E; ++a) {',
                                              'const int s0 = (16 * a / E) * E;', 'const int last = ((16 * a + 15) / E) * E + E;',
                                              'if (last - s0 > 32) return false;')),
        fused=all(has(fused, s) for s in (
            'if (ssmq::sw("SSMQ_NO_BQ_FUSED")) return false;', 'if (np != 128 && np != 208) return false;',
            'if (D < 1 || D > 15 || E < 6 || E > 10 || !fxwc_cov_supported(E)) return false;',
            'return fused_geom_ok(fused_geom(np / 16, D, E, fused_dm(nullptr, D, E)), np / 16, D, E);')),
        fused_geom=all(has(fused, s) for s in (
            'const int NP = NT * 16, LB = NP + 16 + 4, FP = NP + 2, RT = waves / 2, KS = 2 * waves;',
            'const size_t cap = waves == 4 ? 80 * 1024 : 160 * 1024;', 'for (q.tpw = 16 * RT / E; q.tpw >= 1; --q.tpw) {',
            'q.fx_doubles = q.tpw * E * FP;',
            'q.lds = sizeof(double) * ((size_t)q.fx_doubles + 2 * KS * LB + 16 * RT + (size_t)q.tpw * (DM * (DM + 1) / 2 + DM)) + sizeof(int) * (16 + 16 * RT);',
            'const size_t slab = (size_t)2 * KS * (NT * 16 + 20);',
            'return q.tpw >= 1 && 4 * q.tpw * E >= 3 * 16 * RT && (size_t)q.tpw * D * D <= slab && (size_t)2 * RT * 64 * 8 + 512 + 32 <= slab;',
            'FusedGeom fused_geom(int NT, int D, int E, int DM) { return fused_geom_for(8, NT, D, E, DM); }')),
        fused_dm=all(has(fused, s) for s in ('if (a && a->fid == SSMQ_F_SMOOTH10D_DYN && a->fp.n_idx == 0 && dm <= 10) return 10;',
                                             'return dm <= 8 ? 8 : SSMQ_MAX_DIM;')),
        stream=all(has(strm, s) for s in (
            'if (ssmq::sw("SSMQ_NO_BQ_STREAM") || ssmq::sw("SSMQ_NO_MFMA")) return false;',
            'if (N <= (mn ? atoi(mn) : 208) || N > SSMQ_MAX_PTS) return false;', 'return D >= 1 && D <= 15 && E >= 1 && E <= 10;')),
        tpw=has(strm, 'int bq_stream_tpw(int E) { return 64 / E; }'),
        panel=(int(re.search(r'constexpr int kPanT = (\d+);', strm).group(1)), has(strm, 'constexpr int kPanW = 16 * kPanT;')),
        split=all(has(strm, s) for s in ('if (npan < 2 || cus < 1 || ssmq::sw("SSMQ_BQ_STREAM_NO_SPLIT")) return;',
                                         'const int64_t rem = nblocks % cus;', 'if (rem == 0 || 5 * rem > 3 * cus) return;')),
        min_rows=int(re.search(r'constexpr int64_t kGemmMinRows = (\d+);', host).group(1)),
        big_cols=int(re.search(r'constexpr int kBigCols = (\d+);', host).group(1)),
        max_pts=int(re.search(r'#define SSMQ_MAX_PTS (\d+)', read('ssmq.h')).group(1)),
        wide_lds=has(wide, 'return sizeof(double) * (size_t)(D * D + D + D * N + 2 * E * N + E + 2 * E * E + E * D);'),
        precedence=all(has(api, s) for s in (
            'const bool wide_fits = wide_lds_bytes(h->D, h->E, h->N) <= 160 * 1024 - 64;',
            'const bool big = !se && h->N > 64 && ((h->form == SSMQ_FORM_BQ && h->d_wc_blk && (b_route * h->E >= kGemmMinRows || !wide_fits) && '
            '(h->tp_nu <= 0.0 || h->d_ik_blk)) || (h->form == SSMQ_FORM_SIGMA && !wide_fits));',
            'const bool streamed = !se && h->form == SSMQ_FORM_BQ && h->tp_nu <= 0.0 && h->d_sx_pan && b_route * h->E >= kGemmMinRows && '
            'bq_stream_supported(h->D, h->E, h->N);',
            'const bool one_launch = !se && !big && h->form == SSMQ_FORM_BQ && h->d_wc_pad && h->d_sx_pad && h->tp_nu <= 0.0 && '
            'b_route * h->E >= kGemmMinRows && bq_fused_supported(h->D, h->E, h->N);',
            'se ? se->name : streamed ? "k_bq_stream" : big ? "k_apply_big" : one_launch ? "k_bq_fused" :',
            'if (streamed) {', 'if (big) {', 'if (h->d_wc_pad && h->form == SSMQ_FORM_BQ && B * h->E >= kGemmMinRows) {',
            'if (h->tp_nu <= 0.0 && h->d_wcx_pad && fxwc_cov_supported(h->E) && h->D <= 16 && !ssmq::sw("SSMQ_NO_FUSED_COV")) {',
            'if (np && !ssmq::sw("SSMQ_NO_MFMA")) {', 'if (!sigma && N > 64 && !np && !ssmq::sw("SSMQ_NO_MFMA")) {',
            'bool symmetric = bq_stream_supported(D, E, N) && h->tp_nu <= 0.0;')))


# ---- the cases -------------------------------------------------------------------------------------------------------------------
Case = collections.namedtuple('Case', 'route env F D sidx E N form tp sym batch')
_NF, _NS, _NC = (('SSMQ_NO_BQ_FUSED', '1'),), (('SSMQ_NO_BQ_STREAM', '1'),), (('SSMQ_NO_FUSED_COV', '1'),)
_I12, _I15, _I16 = go._I12, go._I15, go._I16
_U, _PD, _R1, _CV, _RE, _RB, _BE, _RA, _SM = ('SSMQ_F_UNGM_DYN', 'SSMQ_F_PENDULUM_DYN', 'SSMQ_F_REENTRY1D_DYN', 'SSMQ_F_CV_DYN', 'SSMQ_F_REENTRY2D_DYN',
                                               'SSMQ_F_REENTRY2D_BIAS_DYN', 'SSMQ_F_BEARING_MEAS', 'SSMQ_F_RADAR2D_MEAS', 'SSMQ_F_SMOOTH10D_DYN')
_J8, _J15 = (7, 0, 3, 4, 6, 1), (14, 0, 3, 4, 7, 1)
# (route wanted, switches, model, D, state index, E, N, forms: B = BQ with a symmetric Wc, N = BQ with a Wc that is not symmetric,
#  T = BQ with the t-process variance, S = centred; a lower-case letter: the same with the batch that cuts k_bq_stream's last round)
TABLE = (
    # k_bq_fused: N = 113, 127, 128 (128 columns), 193, 201, 207, 208 (208 columns); E = 6, 7, 8, 10; max(D, E) <= 8 (register Cholesky)
    # and above (LDS Cholesky); D = 15 (wm in the Wcc' tile); the compile-time integrand at the benchmark's shape and at 128 columns
    (FUSED, (), _RB, 6, None, 6, 113, 'B'), (FUSED, (), _BE, 5, (3, 1), 7, 127, 'B'), (FUSED, (), _BE, 8, (5, 2), 8, 128, 'B'),
    (FUSED, (), _SM, 10, None, 10, 128, 'B'), (FUSED, (), _SM, 12, _I12, 10, 120, 'B'), (FUSED, (), _RB, 15, _J15, 6, 193, 'B'),
    (FUSED, (), _SM, 10, None, 10, 201, 'B'), (FUSED, (), _RB, 8, _J8, 6, 201, 'B'), (FUSED, (), _BE, 9, (7, 2), 7, 207, 'B'),
    (FUSED, (), _BE, 15, (13, 4), 8, 208, 'B'), (FUSED, (), _SM, 15, _I15, 10, 208, 'B'),
    # two passes: E = 1 .. 5 (the one-launch route refuses them), E = 7 and 10 behind SSMQ_NO_BQ_FUSED, D = 16, a Wc that is not
    # symmetric, 256 columns behind SSMQ_NO_BQ_STREAM / with a Wc that is not symmetric; E = 3, 5, 7 straddle the 16-row tiles
    (TWO, (), _U, 1, None, 1, 113, 'B'), (TWO, (), _PD, 2, None, 2, 128, 'B'), (TWO, (), _R1, 3, None, 3, 127, 'B'),
    (TWO, (), _CV, 4, None, 4, 193, 'B'), (TWO, (), _RE, 5, None, 5, 208, 'B'),
    (TWO, _NF, _BE, 5, (3, 1), 7, 127, 'B'), (TWO, _NF, _SM, 10, None, 10, 201, 'B'), (TWO, (), _BE, 16, (15, 7), 8, 201, 'B'),
    (TWO, (), _RB, 6, None, 6, 113, 'N'), (TWO, _NS, _R1, 3, None, 3, 241, 'B'), (TWO, (), _CV, 4, None, 4, 256, 'N'),
    (TWO, _NS, _BE, 5, (3, 1), 7, 256, 'B'),
    # three passes: the t-process form at N = 120, 201, 250 (and 241), both emv modes; one BQ shape behind SSMQ_NO_FUSED_COV
    (THREE, (), _R1, 3, None, 3, 120, 'T'), (THREE, (), _RE, 5, None, 5, 201, 'T'), (THREE, (), _CV, 4, None, 4, 250, 'T'),
    (THREE, (), _PD, 2, None, 2, 241, 'T'), (THREE, _NC, _R1, 3, None, 3, 127, 'B'),
    # k_bq_stream: N = 209, 240, 241, 256 (16 k-blocks, one panel), 257 (one k-block into the second panel), 272, 273, 513 (three
    # panels); E = 1, 2, 3, 5, 7, 8, 10; D = 1 and 15; the last one with more blocks than compute units
    (STREAM, (), _U, 1, None, 1, 209, 'B'), (STREAM, (), _PD, 2, None, 2, 240, 'B'), (STREAM, (), _R1, 3, None, 3, 241, 'B'),
    (STREAM, (), _RE, 5, None, 5, 256, 'B'), (STREAM, (), _BE, 5, (3, 1), 7, 257, 'B'), (STREAM, (), _SM, 15, _I15, 10, 272, 'B'),
    (STREAM, (), _BE, 8, (5, 2), 8, 273, 'B'), (STREAM, (), _RA, 9, (7, 2), 2, 513, 'B'), (STREAM, (), _SM, 10, None, 10, 257, 'b'),
    # k_apply_big: N = 65, 80, 81, 112, 129, 192; 209 and 257 with a Wc that is not symmetric; N = 240 with D = 16 (16 kb + D = 256:
    # exactly one column block); 257 (two column blocks); the t-process form (second GEMM with iK) at N = 112 and 257; the centred
    # form at the first N that no longer fits the LDS-resident kernel
    (BIG, (), _U, 1, None, 1, 65, 'B'), (BIG, (), _PD, 2, None, 2, 80, 'B'), (BIG, (), _CV, 4, None, 4, 81, 'B'),
    (BIG, (), _RE, 5, None, 5, 112, 'T'), (BIG, (), _RB, 6, None, 6, 129, 'B'), (BIG, (), _SM, 10, None, 10, 192, 'B'),
    (BIG, (), _R1, 3, None, 3, 209, 'N'), (BIG, (), _BE, 16, (15, 7), 8, 240, 'B'), (BIG, (), _PD, 2, None, 2, 257, 'T'),
    (BIG, (), _BE, 5, (3, 1), 7, 257, 'N'), (BIG, _NS, _R1, 3, None, 3, 257, 'B'), (BIG, (), _SM, 16, _I16, 10, 551, 'S'),
)
_FORMS = {'B': (ao.FORM_BQ, 0, True, 'ragged'), 'N': (ao.FORM_BQ, 0, False, 'ragged'), 'T': (ao.FORM_BQ, 1, True, 'ragged'),
          'S': (ao.FORM_SIGMA, 0, True, 'ragged'), 'b': (ao.FORM_BQ, 0, True, 'split')}
CASES = tuple(Case(*(r[:7] + _FORMS[f])) for r in TABLE for f in r[7])

# the row threshold: one shape per route family (each a row of the table) at B E just below 256 and at the first B at or above it
THRESHOLD = tuple(c for c in CASES if (c.route, c.N, c.E) in ((FUSED, 127, 7), (TWO, 127, 3), (THREE, 120, 3), (STREAM, 241, 3), (BIG, 81, 4))
                  and not c.env)

# host-supplied values (ssmq_apply_fx_batch): (route, D, E, N)
FX_TABLE = ((THREE, 4, 11, 120), (THREE, 5, 13, 120), (TWO, 3, 12, 120), (TWO, 16, 16, 120), (BIG, 7, 16, 130))
FxCase = collections.namedtuple('FxCase', 'route D E N')
FX_CASES = tuple(FxCase(*r) for r in FX_TABLE)

_SENS8 = go._SENS8


def form_tag(case):
    return 'SIGMA' if case.form == ao.FORM_SIGMA else ('BQ+TP' if case.tp else ('BQ' if case.sym else 'BQ-nonsym'))


def shape_of(case):
    """What rule and reference depend on."""
    return (case.F, case.D, case.sidx, case.E, case.N, case.form, case.tp, case.sym)


def case_id(case):
    f = case.F.replace('SSMQ_F_', '').lower()
    sw = ''.join('-' + k.replace('SSMQ_', '') for k, _ in case.env)
    return '%s-%s-D%dE%dN%d-%s%s%s' % (case.route, f, case.D, case.E, case.N, form_tag(case), sw, '-split' if case.batch == 'split' else '')


def fx_case_id(c):
    return 'fx-%s-D%dE%dN%d' % (c.route, c.D, c.E, c.N)


def is_smooth(case):
    return case.F == _SM and case.sidx is None


def restated_route(case, rows=1 << 20):
    return route(case.D, case.E, case.N, case.form, case.tp, case.sym, case.env, rows)


def fx_route(c, rows=1 << 20):
    """ssmq_apply_fx_batch: no streamed and no one-launch route."""
    wc_blk = c.N > 64 and not gemm_mfma_padded(c.N)
    if wc_blk and rows >= GEMM_MIN_ROWS:
        return BIG
    if gemm_mfma_padded(c.N) and rows >= GEMM_MIN_ROWS:
        return TWO if fxwc_cov_supported(c.E) and c.D <= 16 else THREE
    return WIDE


def lanes_per_tile(case):
    """Trajectories of one workgroup tile: k_bq_fused's geometry, k_bq_stream's 64-row blocks; the GEMM passes work on 64 rows."""
    if case.route == FUSED:
        return fused_tpw(case.D, case.E, case.N, is_smooth(case))
    return max(1, 64 // case.E)


def batch_of(case, cus=256):
    """Whole tiles and a ragged one of about half a tile with B E >= 256 (at least three whole ones); 'split': more blocks than the
    device has compute units, the last round 5/32 full, and a ragged block."""
    r = lanes_per_tile(case)
    if case.batch == 'split':
        return r * (cus + (5 * cus) // 32 - 1) + r // 2 + 1
    k = 3
    while (k * r + r // 2 + 1) * case.E < GEMM_MIN_ROWS:
        k += 1
    return k * r + r // 2 + 1


def threshold_batches(case):
    b = -(-GEMM_MIN_ROWS // case.E)
    return b - 1, b


def lane_probe(b, B):
    return go.lane_probe(b, B)


def model_of(case):
    """(oracle id, constants, state index); bearings with E sensors."""
    if case.F == _SM:
        return orc.F_SMOOTH10D_DYN, (), case.sidx
    fid, p = ao.MODELS[case.F][:2]
    if fid == orc.F_BEARING_MEAS:
        p = _SENS8[:2 * case.E]
    return fid, tuple(p), case.sidx


def probes_for(case):
    return go.probes_for(case.F, case.D, case.sidx)


def _spread(rng, shape, decades):
    return rng.standard_normal(shape) * 10.0 ** rng.uniform(-decades, 0.0, shape)


@functools.lru_cache(maxsize=None)
def _rule(shape):
    F, D, sidx, E, N, form, tp, sym = shape
    fid = orc.F_SMOOTH10D_DYN if F == _SM else ao.MODELS[F][0]
    xi = go._points(fid, D, sidx, E, N)
    rng = np.random.default_rng([20291, fid, D, E, N, form, tp, int(sym)] + list(sidx or ()))
    while True:
        u = rng.uniform(-0.5, 1.5, N) * 10.0 ** rng.uniform(-2.0, 0.0, N)
        if abs(u.sum()) >= np.abs(u).sum() / 4 and u.min() < 0.0:
            break
    wm = u / u.sum()
    if form == ao.FORM_SIGMA:
        rule = dict(xi=xi, wm=wm, Wc=rng.uniform(0.2, 1.0, N) * 10.0 ** rng.uniform(-3.0, 0.0, N) / N, Wcc=None)
    else:
        Wc = ao._mirror(_spread(rng, (N, N), 3.0) / N)
        if not sym:
            Wc = Wc + np.triu(1e-2 * _spread(rng, (N, N), 3.0) / N, 1)
        rule = dict(xi=xi, wm=wm, Wc=Wc, Wcc=_spread(rng, (D, N), 3.0) / N)
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


def mirrored(r, sym):
    """The kernels mirror the lower triangle of (fx Wc) fx': the same of the covariance (and its scale) where Wc is not symmetric."""
    if r is None or sym:
        return r
    r = list(r)
    for i in (1, 4):
        if i < len(r):
            r[i] = ao._mirror(r[i])
    return tuple(r)


@functools.lru_cache(maxsize=None)
def _reference(shape):
    F, D, sidx, E, N, form, tp, sym = shape
    case = Case(None, (), F, D, sidx, E, N, form, tp, sym, 'ragged')
    fid, p, _ = model_of(case)
    mean, cov, time = probes_for(case)
    out = []
    for k in range(N_PROBES):
        r = mirrored(transform_hp(fid, p, sidx, form, _rule(shape), mean[k], cov[k], time[k]), sym)
        if r is not None:
            for a in r:
                a.setflags(write=False)
        out.append(r)
    return tuple(out)


def reference(case):
    """Per probe: the oracle's (mean_f, cov_f, cov_fx, scale_mean, scale_cov, scale_cross), or None (not positive definite).  Built once
    per shape and process, never modified."""
    return _reference(shape_of(case))


def float64(case, k, rule=None):
    """The float64 NumPy restatement of probe k (with the lower triangle mirrored as the reference has it)."""
    fid, p, sidx = model_of(case)
    mean, cov, time = probes_for(case)
    return mirrored(transform_f64(fid, p, sidx, case.form, rule or rule_for(case), mean[k], cov[k], time[k]), case.sym)


# ---- host-supplied values ----------------------------------------------------------------------------------------------------------
FX_PROBES = 3


@functools.lru_cache(maxsize=None)
def fx_inputs(c):
    """rule (BQ, symmetric spread Wc, model variance of either mode), fx (3, E, N) with magnitudes over two decades, chol (3, D, D)."""
    D, E, N = c.D, c.E, c.N
    rng = np.random.default_rng([20292, D, E, N])
    u = rng.uniform(-0.5, 1.5, N) * 10.0 ** rng.uniform(-2.0, 0.0, N)
    G = rng.standard_normal((E, E))
    emv = ao._mirror(0.3 * (G + G.T))
    emv[np.arange(E), np.arange(E)] = rng.uniform(0.5, 1.5, E)
    rule = dict(xi=rng.standard_normal((D, N)), wm=u / np.abs(u).sum(), Wc=ao._mirror(_spread(rng, (N, N), 3.0) / N),
                Wcc=_spread(rng, (D, N), 3.0) / N, emv=emv, emv_mode=ao.EMV_BROADCAST if (D + E) % 2 else ao.EMV_DIAG, nu=0.0, iK=None)
    fx = _spread(rng, (FX_PROBES, E, N), 2.0)
    chol = np.tril(_spread(rng, (FX_PROBES, D, D), 1.0)) + np.eye(D)
    for a in list(rule.values()) + [fx, chol]:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return rule, fx, chol


def moments_f64(rule, fx, chol):
    mask = np.ones_like(rule['emv']) if rule['emv_mode'] == ao.EMV_BROADCAST else np.eye(rule['emv'].shape[0])
    mf = fx.dot(rule['wm'])
    return mf, fx.dot(rule['Wc']).dot(fx.T) - np.outer(mf, mf) + rule['emv'] * mask, fx.dot(rule['Wcc'].T).dot(chol.T)


def moments_hp(rule, fx, chol):
    """mean = fx wm, cov = fx Wc fx' - mean mean' + emv, cross = (fx Wcc') L' at 50 digits from the float64 inputs taken exactly, and the
    scales A (sums of the absolute values of the terms; the inputs are exact: no S)."""
    E, N = fx.shape
    D = chol.shape[0]
    with mp.workdps(ao.DPS):
        h = lambda M: [[mp.mpf(float(v)) for v in r] for r in M]
        F, L, Wcc = h(fx), h(chol), h(rule['Wcc'])
        WcT = h(rule['Wc'].T)
        w = [mp.mpf(float(v)) for v in rule['wm']]
        mask = np.ones((E, E)) if rule['emv_mode'] == ao.EMV_BROADCAST else np.eye(E)
        em = rule['emv'] * mask
        mf = [mp.fdot(F[e], w) for e in range(E)]
        T = [[mp.fdot(F[e], WcT[j]) for j in range(N)] for e in range(E)]
        cf = [[mp.fdot(T[e], F[e2]) - mf[e] * mf[e2] + mp.mpf(float(em[e, e2])) for e2 in range(E)] for e in range(E)]
        G = [[mp.fdot(F[e], Wcc[d]) for d in range(D)] for e in range(E)]
        cfx = [[mp.fdot(G[e], L[d]) for d in range(D)] for e in range(E)]
        out = (ao._fl(mf), ao._fl(cf), ao._fl(cfx))
    aF = np.abs(fx)
    return out + (aF.dot(np.abs(rule['wm'])), aF.dot(np.abs(rule['Wc'])).dot(aF.T) + np.abs(np.outer(out[0], out[0])) + np.abs(em),
                  aF.dot(np.abs(rule['Wcc']).T).dot(np.abs(chol).T))


@functools.lru_cache(maxsize=None)
def fx_reference(c):
    rule, fx, chol = fx_inputs(c)
    out = []
    for k in range(FX_PROBES):
        r = moments_hp(rule, fx[k], chol[k])
        for a in r:
            a.setflags(write=False)
        out.append(r)
    return tuple(out)
