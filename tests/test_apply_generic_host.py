"""Host half of the pinning of k_apply_tile / k_apply_wave / k_apply_wide (tests/_apply_generic_oracle.py): the case table against
what it claims to cover, the restated dispatch against the source text, the measurement of K_REF_GENERIC - the worst ratio of the
plain float64 NumPy restatement against the 50-digit oracle in units of eps (A + S) - and the sanity of scales and probes.  The
device half (tests/test_apply_generic_gpu.py) holds the kernels to K = max(16, 8 K_REF_GENERIC) on the same cases."""
import numpy as np
import pytest

from tests import _apply_generic_oracle as go
from tests import _apply_small_oracle as ao

CASES = go.CASES


def test_dispatch_restatement_matches_the_source():
    """A change of tile_ksm, of the trajectories per wave, of the DM classes, of the grid cap or of the <64> | <256> switch is an edit
    of the literals the table was laid out by."""
    src = go.parsed_dispatch()
    assert src['ksm'] == go.KSM_STEPS and src['ksm_last'] == go.KSM_LAST
    assert src['g'] and src['cap'] and src['exact']
    want = (((go.SMOOTH_DM, go.SMOOTH_DM),) + tuple((b, b) for b in go.DM_CLASSES), 'SSMQ_MAX_DIM')
    assert src['dm_tile'] == want and src['dm_wave'] == want
    assert (src['wgs_per_cu'], src['tile_waves'], src['wave_waves'], src['wide_switch']) == \
        (go.TILE_WGS_PER_CU, go.TILE_WAVES, go.WAVE_WAVES, go.WIDE_SWITCH)
    assert [go.tile_ksm(n) for n in (9, 16, 17, 24, 25, 32, 33, 52, 53, 64)] == [4, 4, 6, 6, 8, 8, 13, 13, 16, 16]
    assert [go.tile_g(n) for n in (9, 16, 17, 21, 22, 32, 33, 64)] == [4, 4, 3, 3, 2, 2, 1, 1]
    assert [go.dm_class(d, 1) for d in (4, 5, 8, 9, 12, 13, 16)] == [4, 8, 8, 12, 12, 16, 16]


def test_case_table_covers_what_it_is_aimed_at():
    assert len(CASES) == go.EXPECTED_CASES == 91
    ids = [go.case_id(c) for c in CASES]
    assert len(set(ids)) == len(ids)
    small = {(r.F, r.D, r.E, r.N) for r in ao.table_rows()}
    for c in CASES:
        assert (c.F, c.D, c.E, c.N) not in small, c              # no register specialisation takes the case away
        assert c.E <= 10 and c.D <= 16
        fid, p, sidx = go.model_of(c)
        if sidx is None:
            assert ao.DIN[fid] <= c.D
        else:                                                     # not increasing, not from 0, within the state
            assert len(sidx) == ao.DIN[fid] and sidx[0] != 0 and list(sidx) != sorted(sidx) and max(sidx) < c.D and len(set(sidx)) == len(sidx)
        if c.kernel == go.TILE:
            assert 8 < c.N <= 64 and not {'SSMQ_NO_TILE', 'SSMQ_NO_WAVE'} & set(dict(c.env))
        elif c.kernel == go.WAVE:
            assert c.N <= 8 or 'SSMQ_NO_TILE' in dict(c.env)
        else:
            assert 'SSMQ_NO_WAVE' in dict(c.env) or (c.N > 64 and 'SSMQ_NO_MFMA' in dict(c.env))
    tile = [c for c in CASES if c.kernel == go.TILE]
    plain = [c for c in tile if not c.env and not (c.F == go._SM and c.sidx is None)]
    # every (DM class, KS class) in all three forms
    for dm in (4, 8, 12, 16):
        for ks in (4, 6, 8, 13, 16):
            got = {go.form_tag(c) for c in plain if go.dm_class(c.D, c.E) == dm and go.tile_ksm(c.N) == ks}
            assert got == {'BQ', 'BQ+TP', 'SIGMA'}, (dm, ks, got)
    shapes = {(c.F, c.D, c.sidx, c.E, c.N, c.env) for c in tile}
    for n in (9, 16, 17, 21, 22, 24, 25, 32, 33, 52, 53, 64):
        assert sum(1 for s in shapes if s[4] == n) >= 2, n
    assert {max(c.D, c.E) for c in tile} >= {1, 4, 5, 8, 9, 12, 13, 15, 16}
    # the DM = 12 and 16 bodies in every form through a state index; the mean row's last shape, the first without, one shape both ways
    assert any(c.D == 15 and go.uses_mrow(c) for c in tile) and any(c.D == 16 and c.form == ao.FORM_BQ and not go.uses_mrow(c) for c in tile)
    both = [c for c in tile if 'SSMQ_TILE_NO_MROW' in dict(c.env)]
    assert both and all(c._replace(env=()) in tile for c in both)
    big = max(tile, key=lambda c: go.tile_lds_bytes(c.D, c.E, c.N, bool(c.tp), go.uses_mrow(c)))
    assert (big.D, big.E, big.N, big.tp) == (16, 10, 64, 1)
    assert 128 * 1024 < go.tile_lds_bytes(16, 10, 64, True, False) <= 160 * 1024 - 64
    assert sum(1 for c in tile if go.tile_lds_bytes(c.D, c.E, c.N, bool(c.tp), go.uses_mrow(c)) > 48 * 1024) >= 3
    inst = {go.instance(c) for c in tile}
    assert {'<10,6,FC,21>G3', '<10,6,FC>G3'} <= inst
    assert sum(1 for c in tile if go.instance(c) == '<10,6,FC>G3') == 4          # N = 21 t-process, centred, no-exact; N = 20
    # k_apply_wave: the point counts, the DM classes, <10, FC>, K = 1 ... 7, three shapes that reach it with no switch
    wave = [c for c in CASES if c.kernel == go.WAVE]
    assert {c.N for c in wave if c.env} >= {9, 16, 21, 22, 32, 33, 64}
    assert {go.instance(c).split('>')[0] for c in wave} == {'<4', '<8', '<12', '<16', '<10,FC'}
    assert {go.wave_k(c.D, c.E, c.N, c.tp, c.env) for c in wave} >= {1, 2, 3, 4, 7}
    assert sum(1 for c in wave if not c.env and c.N <= 8) == 3
    assert any(go.WAVE_WAVES * go.wave_k(c.D, c.E, c.N, c.tp, c.env) * go.wave_slice_bytes(c.D, c.E, c.N, c.tp) > 48 * 1024 for c in wave)
    # k_apply_wide: both block sizes, E N just below, at and above the switch, N > 64
    wide = [c for c in CASES if c.kernel == go.WIDE]
    assert {go.instance(c) for c in wide} == {'<64>', '<256>'}
    assert {c.E * c.N for c in wide} >= {1016, 1024, 1030} and any(c.N <= 64 for c in wide)
    # both emv modes, and every batch ragged with an odd tail
    assert {go.rule_for(c)['emv_mode'] for c in CASES if c.form == ao.FORM_BQ} == {ao.EMV_DIAG, ao.EMV_BROADCAST}
    for c in CASES:
        r, B = go.lanes_per_round(c), go.batch_of(c)
        if c.kernel != go.WIDE:
            assert r % 4 == 0 and B // r == 3 and (B % r) % 2 == 1, (c, B)
        assert B <= 400 and {go.lane_probe(b, B) for b in range(B)} == set(range(go.N_PROBES))


def test_rules_and_probes():
    for c in CASES:
        rule = go.rule_for(c)
        D, E, N = c.D, c.E, c.N
        assert rule['xi'].shape == (D, N) and rule['wm'].shape == (N,) and rule['wm'].min() < 0.0 < rule['wm'].max()
        if c.form == ao.FORM_SIGMA:
            assert rule['Wc'].shape == (N,) and np.all(rule['Wc'] > 0.0) and rule['Wcc'] is None
        else:
            assert np.array_equal(rule['Wc'], rule['Wc'].T) and np.any(rule['Wc'] < 0.0) and rule['Wcc'].shape == (D, N)
        if c.tp:
            assert np.array_equal(rule['iK'], rule['iK'].T) and np.linalg.eigvalsh(rule['iK'])[0] > 0.0 and rule['nu'] == ao.TP_NU
        mean, cov, time = go.probes_for(c.F, D, c.sidx)
        assert mean.shape == (4, D) and len(set(time.tolist())) == 4
        for k in range(3):
            assert np.array_equal(cov[k], cov[k].T) and np.linalg.eigvalsh(cov[k])[0] > 0.0, (c, k)
        if D > 1:
            assert 5e2 < np.linalg.cond(cov[1]) < 2e3 and np.diag(cov[2]).max() / np.diag(cov[2]).min() > 0.99e6
        if c.F in ('SSMQ_F_CT_DYN', 'SSMQ_F_CTRS_DYN'):           # the turn rate stays away from 0 at every sigma point
            for k in range(3):
                x = mean[k][:, None] + np.linalg.cholesky(cov[k]).dot(rule['xi'])
                assert np.all(np.abs(x[4]) > 0.01) and np.all(np.sign(x[4]) == np.sign(mean[k][4])), (c, k)
        fid, p, sidx = go.model_of(c)
        if fid in (go.orc.F_RADAR2D_MEAS, go.orc.F_BEARING_MEAS):  # ... and the angles away from the branch cut
            idx = list(sidx) if sidx is not None else [0, 1]
            sens = np.asarray(p, dtype=float).reshape(-1, 2)
            for k in range(3):
                x = mean[k][:, None] + np.linalg.cholesky(cov[k]).dot(rule['xi'])
                for sx, sy in sens:
                    dy, dx = x[idx[1]] - sy, x[idx[0]] - sx
                    assert np.all((np.abs(dy) > 50.0) | (dx > 50.0)), (c, k)


@pytest.fixture(scope='module')
def f64_ratios():
    """(shape, probe) -> ratios of the float64 restatement against the oracle, in units of eps (A + S); shapes listed under several
    kernels or switches count once."""
    out = {}
    for c in CASES:
        s = go.shape_of(c)
        if (s, 0) in out:
            continue
        fid, p, sidx = go.model_of(c)
        rule, ref = go.rule_for(c), go.reference(c)
        mean, cov, time = go.probes_for(c.F, c.D, c.sidx)
        for k in range(go.N_PROBES):
            if ref[k] is not None:
                out[(s, k)] = go.ratios(go.transform_f64(fid, p, sidx, c.form, rule, mean[k], cov[k], time[k]), ref[k])
    return out


def test_float64_restatement_within_k_ref_generic(f64_ratios):
    """K_REF_GENERIC: the worst ratio over all cases and good probes; per model and form for the record.  Above about 2 the scale
    A + S would be missing a term for that case - a finding for the derivation, not a reason for a larger K."""
    worst, by_model, by_form = (0.0, None), {}, {}
    for (s, k), q in f64_ratios.items():
        m = max(q)
        tag = 'SIGMA' if s[5] == ao.FORM_SIGMA else ('BQ+TP' if s[6] else 'BQ')
        by_model[s[0]] = max(by_model.get(s[0], 0.0), m)
        by_form[tag] = tuple(max(a, b) for a, b in zip(by_form.get(tag, (0.0,) * 3), q))
        if m > worst[0]:
            worst = (m, (s, k, q))
    for F in sorted(by_model):
        print('K_ref_generic %-28s %.3g' % (F, by_model[F]))
    for t in sorted(by_form):
        print('K_ref_generic %-6s mean %.3g cov %.3g cross %.3g' % ((t,) + by_form[t]))
    print('K_ref_generic worst', worst)
    assert worst[0] < 2.0, worst
    assert worst[0] <= go.K_REF_GENERIC, worst
    assert go.K == max(16.0, 8.0 * go.K_REF_GENERIC)


def test_scales_and_failures():
    """A + S is positive and finite for every entry of every case; the non-PD probe is the only one the oracle reports as failed."""
    for c in CASES:
        ref = go.reference(c)
        assert [k for k in range(go.N_PROBES) if ref[k] is None] == [go.BAD_PROBE], c
        for k in range(go.N_PROBES - 1):
            for v, s in zip(ref[k][:3], ref[k][3:]):
                assert v.shape == s.shape and np.all(np.isfinite(v)) and np.all(np.isfinite(s)) and np.all(s > 0.0), (c, k)
            assert ref[k][0].shape == (c.E,) and ref[k][1].shape == (c.E, c.E) and ref[k][2].shape == (c.E, c.D)
