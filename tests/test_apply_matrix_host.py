"""Host half of the pinning of the matrix-core transform routes for more than 64 points (tests/_apply_matrix_oracle.py): the restated
dispatch against the source text, the case table against what it claims to cover, the measurement of K_REF_MATRIX - the worst ratio
of the plain float64 NumPy restatement against the 50-digit oracle in units of eps (A + S) - and the teeth of the bar: three wrong
restatements (the whole diagonal in S = tril(Wc), the last point of the rule dropped, wm added into the last cross-covariance column at
D = 15) must exceed K eps (A + S) on every case they concern.  The device half (tests/test_apply_matrix_gpu.py) holds the kernels to
K = max(16, 8 K_REF_MATRIX) on the same cases."""
import numpy as np
import pytest

from tests import _apply_matrix_oracle as mo
from tests import _apply_small_oracle as ao

CASES = mo.CASES
GOOD = tuple(k for k in range(mo.N_PROBES) if k != mo.BAD_PROBE)


def test_dispatch_restatement_matches_the_source():
    src = mo.parsed_dispatch()
    assert src['tiles'] == mo.GEMM_TILES == (8, 13, 16)
    for key in ('cov_window', 'fused', 'fused_geom', 'fused_dm', 'stream', 'tpw', 'split', 'wide_lds', 'precedence'):
        assert src[key] is True, key
    assert src['panel'] == (mo.PANEL_COLS // 16, True)
    assert (src['min_rows'], src['big_cols'], src['max_pts']) == (mo.GEMM_MIN_ROWS, mo.BIG_COLS, mo.STREAM_MAX_N) == (256, 256, 4096)
    assert [mo.gemm_mfma_padded(n) for n in (112, 113, 128, 129, 192, 193, 208, 209, 240, 241, 256, 257)] == \
        [0, 128, 128, 0, 0, 208, 208, 0, 0, 256, 256, 0]
    assert [e for e in range(0, 18) if mo.fxwc_cov_supported(e)] == [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 14, 15, 16]
    assert [mo.bq_stream_tpw(e) for e in (1, 2, 3, 5, 7, 8, 10)] == [64, 32, 21, 12, 9, 8, 6]
    assert [64 - e * mo.bq_stream_tpw(e) for e in (1, 2, 3, 5, 7, 8, 10)] == [0, 0, 1, 4, 1, 0, 4]
    assert mo.bq_fused_supported(10, 10, 201) and mo.bq_fused_supported(15, 6, 113) and not mo.bq_fused_supported(16, 8, 201)
    assert not mo.bq_fused_supported(5, 5, 208) and not mo.bq_fused_supported(5, 7, 256) and not mo.bq_fused_supported(5, 7, 127, mo._NF)
    assert mo.bq_stream_supported(15, 10, 209) and not mo.bq_stream_supported(15, 10, 208) and not mo.bq_stream_supported(16, 10, 240)
    assert mo.bq_stream_split(296, 2, 256) == (256, 40) and mo.bq_stream_split(296, 1, 256) == (296, 0) and \
        mo.bq_stream_split(256 + 154, 2, 256) == (410, 0) and mo.bq_stream_split(256 + 153, 2, 256) == (256, 153)
    # the centred form leaves the LDS-resident kernel a little above 550 points at D = 16, E = 10
    n = mo.centred_first_big_n(16, 10)
    assert n == 551 and mo.wide_lds_bytes(16, 10, n - 1) <= mo.LDS_BOUND < mo.wide_lds_bytes(16, 10, n)


def test_case_table_covers_what_it_is_aimed_at():
    assert len(CASES) == mo.EXPECTED_CASES == 49
    assert len(mo.FX_CASES) == mo.EXPECTED_FX_CASES == 5 and len(mo.THRESHOLD) == 5
    ids = [mo.case_id(c) for c in CASES]
    assert len(set(ids)) == len(ids)
    small = {(r.F, r.D, r.E, r.N) for r in ao.table_rows()}
    for c in CASES:
        assert (c.F, c.D, c.E, c.N) not in small and c.N > 64 and c.E <= 10 and c.D <= 16
        assert mo.restated_route(c) == c.route, c
        assert c.E * c.N ** 2 * (2 if c.tp else 1) <= 1e6 or c.form == ao.FORM_SIGMA, c        # the reference budget
        fid, p, sidx = mo.model_of(c)
        if sidx is None:
            assert ao.DIN[fid] <= c.D
        else:                                                     # not increasing, not from 0, within the state
            assert len(sidx) == ao.DIN[fid] and sidx[0] != 0 and list(sidx) != sorted(sidx) and max(sidx) < c.D and len(set(sidx)) == len(sidx)
        B = mo.batch_of(c)
        r = mo.lanes_per_tile(c)
        assert B * c.E >= mo.GEMM_MIN_ROWS and B // r >= 3 and 0 < B % r < r, (c, B, r)
        assert {mo.lane_probe(b, B) for b in range(B)} == set(range(mo.N_PROBES)) and mo.lane_probe(B - 1, B) == mo.BAD_PROBE
    by = lambda route: [c for c in CASES if c.route == route]
    fused = by(mo.FUSED)
    assert {c.N for c in fused} >= {113, 127, 128, 193, 201, 207, 208} and {c.E for c in fused} == {6, 7, 8, 10}
    assert {mo.fused_dm(c.D, c.E, mo.is_smooth(c)) for c in fused} == {8, 10, 16}
    assert {mo.lanes_per_tile(c) for c in fused} == {mo.fused_tpw(d, e, n, sm) for d in range(1, 16) for e in (6, 7, 8, 10) for n in (128, 208)
                                                     for sm in (False, True) if mo.bq_fused_supported(d, e, n)} == {5, 6, 7, 8, 9, 10}
    assert any(c.D == 15 for c in fused) and any((c.F, c.D, c.E, c.N, c.sidx) == (mo._SM, 10, 10, 201, None) for c in fused)
    assert {mo.rule_for(c)['emv_mode'] for c in fused} == {ao.EMV_DIAG, ao.EMV_BROADCAST}
    two = by(mo.TWO)
    assert {c.E for c in two if not c.env and c.sym} >= {1, 2, 3, 4, 5} and {c.E for c in two if c.env == mo._NF} == {7, 10}
    assert any(c.D == 16 for c in two) and any(not c.sym for c in two)
    assert {c.N for c in two if mo.gemm_mfma_padded(c.N) == 256} == {241, 256} and {c.E for c in two} >= {3, 5, 7}
    three = by(mo.THREE)
    assert {c.N for c in three if c.tp} >= {120, 201, 250} and any(c.env == mo._NC for c in three)
    assert {mo.rule_for(c)['emv_mode'] for c in three if c.tp} == {ao.EMV_DIAG, ao.EMV_BROADCAST}
    strm = by(mo.STREAM)
    assert {c.N for c in strm} >= {209, 240, 241, 256, 257, 272, 273, 513} and {c.E for c in strm} == {1, 2, 3, 5, 7, 8, 10}
    assert {c.D for c in strm} >= {1, 15} and sum(1 for c in strm if c.batch == 'split') == 1
    assert all(c.E <= 2 for c in strm if c.N > 273) and {mo.bq_stream_panels(c.N) for c in strm} == {1, 2, 3}
    big = by(mo.BIG)
    assert {c.N for c in big} >= {65, 80, 81, 112, 129, 192, 209, 240, 257}
    assert any(c.N == 209 and not c.sym for c in big) and any(c.N == 240 and c.D == 16 for c in big)
    assert {-(-(16 * ((c.N + 15) // 16) + c.D) // mo.BIG_COLS) for c in big if c.form == ao.FORM_BQ} == {1, 2}
    assert sum(1 for c in big if c.tp) == 2 and [c.N for c in big if c.form == ao.FORM_SIGMA] == [mo.centred_first_big_n(16, 10)]
    assert {c.route for c in mo.THRESHOLD} == {mo.FUSED, mo.TWO, mo.THREE, mo.STREAM, mo.BIG}
    for c in mo.THRESHOLD:
        lo, hi = mo.threshold_batches(c)
        assert mo.restated_route(c, lo * c.E) == mo.WIDE and mo.restated_route(c, hi * c.E) == c.route
    assert [(c.E, c.N, mo.fx_route(c)) for c in mo.FX_CASES] == [(11, 120, mo.THREE), (13, 120, mo.THREE), (12, 120, mo.TWO), (16, 120, mo.TWO),
                                                                (16, 130, mo.BIG)]


def test_rules_and_probes():
    for c in CASES:
        rule = mo.rule_for(c)
        D, N = c.D, c.N
        assert rule['xi'].shape == (D, N) and rule['wm'].shape == (N,) and rule['wm'].min() < 0.0 < rule['wm'].max()
        if c.form == ao.FORM_SIGMA:
            assert rule['Wc'].shape == (N,) and np.all(rule['Wc'] > 0.0) and rule['Wcc'] is None
        else:
            W = rule['Wc']
            assert np.array_equal(W, W.T) == c.sym and np.any(W < 0.0) and rule['Wcc'].shape == (D, N)
            assert np.array_equal(np.tril(W), np.tril(W.T)) or not c.sym
            a = np.abs(W[np.tril_indices(N)])
            assert np.percentile(a, 95) / np.percentile(a, 5) > 300.0, c          # magnitudes over about three decades
        if c.tp:
            assert np.array_equal(rule['iK'], rule['iK'].T) and np.linalg.eigvalsh(rule['iK'])[0] > 0.0 and rule['nu'] == ao.TP_NU
        mean, cov, time = mo.probes_for(c)
        for k in GOOD:
            assert np.array_equal(cov[k], cov[k].T) and np.linalg.eigvalsh(cov[k])[0] > 0.0, (c, k)
        fid, p, sidx = mo.model_of(c)
        if fid in (mo.orc.F_RADAR2D_MEAS, mo.orc.F_BEARING_MEAS):  # the angles keep away from the branch cut
            idx = list(sidx) if sidx is not None else [0, 1]
            sens = np.asarray(p, dtype=float).reshape(-1, 2)
            assert fid == mo.orc.F_RADAR2D_MEAS or len(sens) == c.E
            for k in GOOD:
                x = mean[k][:, None] + np.linalg.cholesky(cov[k]).dot(rule['xi'])
                for sx, sy in sens:
                    dy, dx = x[idx[1]] - sy, x[idx[0]] - sx
                    assert np.all((np.abs(dy) > 50.0) | (dx > 50.0)), (c, k)


@pytest.fixture(scope='module')
def f64_ratios():
    """(id, probe) -> ratios of the float64 restatement against the oracle, in units of eps (A + S); shapes listed under several
    routes or switches count once."""
    out, seen = {}, set()
    for c in CASES:
        s = mo.shape_of(c)
        if s in seen:
            continue
        seen.add(s)
        ref = mo.reference(c)
        assert [k for k in range(mo.N_PROBES) if ref[k] is None] == [mo.BAD_PROBE], c
        for k in GOOD:
            for v, sc in zip(ref[k][:3], ref[k][3:]):
                assert v.shape == sc.shape and np.all(np.isfinite(v)) and np.all(np.isfinite(sc)) and np.all(sc > 0.0), (c, k)
            out[(mo.case_id(c), k)] = mo.ratios(mo.float64(c, k), ref[k])
    for c in mo.FX_CASES:
        rule, fx, chol = mo.fx_inputs(c)
        ref = mo.fx_reference(c)
        for k in range(mo.FX_PROBES):
            out[(mo.fx_case_id(c), k)] = mo.ratios(mo.moments_f64(rule, fx[k], chol[k]), ref[k])
    return out


def test_float64_restatement_within_k_ref_matrix(f64_ratios):
    """K_REF_MATRIX: the worst ratio over all shapes and good probes.  Above about 2 the scale A + S would be missing a term for that
    case - a finding for the derivation, not a reason for a larger K."""
    worst, by_route = (0.0, None), {}
    for (cid, k), q in f64_ratios.items():
        tag = cid.split('-D')[0].rsplit('-', 1)[0] + ' ' + cid.split('-')[-1 if 'NO_' not in cid else -2]
        by_route[tag] = tuple(max(a, b) for a, b in zip(by_route.get(tag, (0.0,) * 3), q))
        if max(q) > worst[0]:
            worst = (max(q), (cid, k, q))
    for t in sorted(by_route):
        print('K_ref_matrix %-28s mean %.3g cov %.3g cross %.3g' % ((t,) + by_route[t]))
    print('K_ref_matrix worst', worst)
    assert worst[0] < 2.0, worst
    assert worst[0] <= mo.K_REF_MATRIX, worst
    assert worst[0] > 0.9 * mo.K_REF_MATRIX - 0.05, worst            # the literal is the measurement rounded up
    assert worst[1][0] == mo.K_REF_WORST
    assert mo.K == max(16.0, 8.0 * mo.K_REF_MATRIX)


def _points(c, k):
    """Float64 integrand values (E, N) and factor (D, D) of probe k, as the oracle's point cache holds them."""
    fid, p, sidx = mo.model_of(c)
    mean, cov, time = mo.probes_for(c)
    mo.reference(c)
    pt = ao.points_hp(fid, p, sidx, mo.rule_for(c)['xi'], mean[k], cov[k], time[k])
    return pt['fxf'], pt['Lf']


def test_whole_diagonal_in_s_exceeds_the_bar():
    """S = tril(Wc) with its WHOLE diagonal gives fx (Wc + diag Wc) fx': the routes built on S (k_bq_fused, k_bq_stream)."""
    n = 0
    for c in CASES:
        if c.route not in (mo.FUSED, mo.STREAM):
            continue
        ref = mo.reference(c)
        d = np.diag(mo.rule_for(c)['Wc'])
        for k in GOOD:
            mf, cf, cfx = mo.float64(c, k)
            F, _ = _points(c, k)
            q = mo.ratios((mf, cf + (F * d).dot(F.T), cfx), ref[k])
            assert q[1] > mo.K, (mo.case_id(c), k, q)
            n += 1
    assert n == 3 * 20


def test_dropped_last_point_exceeds_the_bar():
    """The last point of the rule left out (a partial k-block cut short): every moment of every case."""
    for c in CASES:
        ref = mo.reference(c)
        rule = dict(mo.rule_for(c))
        for key in ('wm', 'Wc', 'Wcc'):
            if rule[key] is not None:
                a = rule[key].copy()
                a[..., -1] = 0.0
                if a.ndim == 2 and a.shape[0] == a.shape[1] == c.N:
                    a[-1, :] = 0.0
                rule[key] = a
        for k in GOOD:
            q = mo.ratios(mo.float64(c, k, rule), ref[k])
            assert min(q) > mo.K, (mo.case_id(c), k, q)


def test_wm_in_the_last_cross_covariance_column_exceeds_the_bar():
    """D = 15: column 15 of the Wcc' tile carries wm; a column bound one too far adds mean_f L[14][14] to the last column."""
    n = 0
    for c in CASES:
        if c.D != 15 or c.route not in (mo.FUSED, mo.STREAM):
            continue
        ref = mo.reference(c)
        for k in GOOD:
            mf, cf, cfx = mo.float64(c, k)
            _, L = _points(c, k)
            bad = cfx.copy()
            bad[:, 14] += mf * L[14, 14]
            q = mo.ratios((mf, cf, bad), ref[k])
            assert q[2] > mo.K, (mo.case_id(c), k, q)
            n += 1
    assert n == 3 * 4
