"""k_apply_tile, k_apply_wave and k_apply_wide (csrc/ssmq_apply_tile.hip, csrc/ssmq_apply_wide.hip) through the C entry points
ssmq_transform_create / ssmq_apply_kernel_name / ssmq_apply_batch_dev, entry by entry against the 50-digit restatement at
K eps (A + S), K = max(16, 8 K_REF_GENERIC) with K_REF_GENERIC measured on float64 NumPy by tests/test_apply_generic_host.py.

The case list is the literal table of tests/_apply_generic_oracle.py; the test id names the kernel the case must reach and the
instantiation it is aimed at (the name query knows the kernel only).  Per case one call at three full rounds of the kernel's
trajectories-per-workgroup plus a ragged round with an odd count, at a pitch above the batch, four probes tiled over the lanes.
Every trajectory runs the same instruction sequence whatever its group, wave or chunk, so lanes that share a probe must agree bit
for bit; one oracle evaluation per probe then pins all lanes.  Also: exact symmetry of cov_f, NaN in the strict upper triangle of
the input covariances, untouched padding lanes, status and NaN outputs of exactly the non-PD lanes.

The edge tests walk two small k_apply_tile shapes (G = 4 and G = 1 trajectories per wave) through the batch sizes around a group
and a chunk, across the grid cap, over an odd pitch and over output planes that are not 16-byte aligned.

Out of reach here: per-item constants of k_apply_wave (the theta-batched step), cov_add / cov_scale / ccov_scale (set by the filters
only), E > 10 (no built-in integrand has more than ten outputs)."""
import ctypes

import numpy as np
import pytest

from tests import _apply_generic_oracle as go
from tests import _apply_small_oracle as ao
from tests._cases import within

pytestmark = pytest.mark.gpu

SENT = -7.0259e+211                  # sentinel of the output planes, padding lanes included
ST_SENT = 0x5A5A5A5A                 # sentinel of the status plane
CANARY = 3.0621e-188                 # around output planes that start 8 bytes off a 16-byte boundary
SWITCHES = ('SSMQ_NO_TILE', 'SSMQ_NO_WAVE', 'SSMQ_NO_MFMA', 'SSMQ_TILE_NO_MROW', 'SSMQ_TILE_NO_EXACT', 'SSMQ_WAVE_K', 'SSMQ_WIDE_ONE_WAVE',
            'SSMQ_NO_FASTPATH', 'SSMQ_NO_SYM')
WORST = {}                           # (kernel, form) -> worst ratios of the table test, for the record printed at its end


@pytest.fixture(scope='module')
def amd():
    import ssmtoybox_amd
    if ssmtoybox_amd.device_count() < 1:
        pytest.fail('no device: the GPU tests need an MI355X')
    ssmtoybox_amd.set_device(0)
    return ssmtoybox_amd


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    for v in SWITCHES:
        monkeypatch.delenv(v, raising=False)


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def ptr(b, off=0):
    return ctypes.c_void_p(b.ptr + off)


def run(case, lanes, ld, times, time_stride, monkeypatch, shift=0):
    """One call under the case's switches: `lanes` lists the probe of every lane (B = len(lanes)), `times` is the time plane as
    uploaded.  shift = 1: every output plane block starts one double into its buffer, canaries before and behind.  Returns the kernel
    name of the handle and the raw planes mean_f (E, ld), cov_f (E E, ld), cov_fx (E D, ld), status (ld,)."""
    from ssmtoybox_amd import _lib
    lib = _lib.load()
    for k, v in case.env:
        monkeypatch.setenv(k, v)
    D, E, N, B = case.D, case.E, case.N, len(lanes)
    rule = go.rule_for(case)
    fid, p, sidx = go.model_of(case)
    mean, cov, _ = go.probes_for(case.F, D, case.sidx)
    c = lambda a: None if a is None else _lib.as_c(a)[1]
    keep = [np.ascontiguousarray(rule[k], dtype=float) if rule[k] is not None else None for k in ('xi', 'wm', 'Wc', 'Wcc', 'emv', 'iK')]
    h = lib.ssmq_transform_create(D, E, N, case.form, c(keep[0]), c(keep[1]), c(keep[2]), c(keep[3]), c(keep[4]), int(rule['emv_mode']),
                                  float(rule['nu']), c(keep[5]))
    assert h, (case, _lib.last_error())
    bufs = []
    try:
        integ = _lib.Integrand.make(fid, p, sidx)
        buf = ctypes.create_string_buffer(256)
        _lib.check(lib.ssmq_apply_kernel_name(ctypes.c_void_p(h), ctypes.byref(integ), buf, 256), 'ssmq_apply_kernel_name')
        lanes = np.asarray(lanes)
        m_pl = np.full((D, ld), SENT)
        m_pl[:, :B] = mean[lanes].T
        c_pl = np.full((D * D, ld), SENT)
        cl = cov[lanes].copy()                                   # (B, D, D)
        cl[:, np.triu_indices(D, 1)[0], np.triu_indices(D, 1)[1]] = np.nan       # the header: only the lower triangle is read
        c_pl[:, :B] = cl.reshape(B, D * D).T
        outs = [np.full(n * ld + 2 * shift, SENT) for n in (E, E * E, E * D)]
        for o in outs:
            if shift:
                o[0] = o[-1] = CANARY
        st = np.full(ld, ST_SENT, dtype=np.int32)
        for host in [m_pl, c_pl, np.ascontiguousarray(times, dtype=float)] + outs + [st]:
            b = _lib.DeviceBuffer(host.nbytes)
            b.upload(host)
            bufs.append(b)
        rc = lib.ssmq_apply_batch_dev(ctypes.c_void_p(h), ctypes.byref(integ), B, ld, ptr(bufs[0]), ptr(bufs[1]), ptr(bufs[2]),
                                      time_stride, ptr(bufs[3], 8 * shift), ptr(bufs[4], 8 * shift), ptr(bufs[5], 8 * shift), ptr(bufs[6]))
        assert rc == 0, (case, rc, _lib.last_error())
        _lib.check(lib.ssmq_sync(), 'ssmq_sync')
        raw = [bufs[3 + i].download(outs[i].shape) for i in range(3)]
        if shift:
            assert all(bits(r[[0, -1]]).tolist() == bits(np.array([CANARY, CANARY])).tolist() for r in raw), (case, 'canary overwritten')
        got = [r[shift:r.size - shift].reshape(-1, ld) for r in raw] + [bufs[6].download((ld,), dtype=np.int32)]
    finally:
        for b in bufs:
            b.free()
        lib.ssmq_transform_destroy(ctypes.c_void_p(h))
        for k, _ in case.env:
            monkeypatch.delenv(k)
    return buf.value.decode(), got


def check(case, what, lanes, got, ref, oracle=True):
    """Everything the module's text promises of one call's planes, against the per-probe references `ref`.  Returns the worst ratios."""
    D, E, B = case.D, case.E, len(lanes)
    mf, cf, cfx, st = got
    lanes = np.asarray(lanes)
    # padding lanes untouched
    for a in (mf, cf, cfx):
        assert np.all(bits(a[:, B:]) == bits(np.array(SENT))), (what, 'padding lanes written')
    assert np.all(st[B:] == ST_SENT), (what, 'status of padding lanes written')
    # status and the non-PD lanes
    bad = np.array([ref[k] is None for k in lanes])
    assert np.all(st[:B][~bad] == 0) and np.all(st[:B][bad] != 0), (what, st[:B].tolist())
    for a in (mf, cf, cfx):
        assert np.all(np.isnan(a[:, :B][:, bad])) and np.all(np.isfinite(a[:, :B][:, ~bad])), (what, 'NaN / finite lanes')
    # exact symmetry
    c3 = cf[:, :B].reshape(E, E, B)
    assert np.all(bits(c3[:, :, ~bad]) == bits(c3.transpose(1, 0, 2)[:, :, ~bad])), (what, 'cov_f not symmetric')
    # bit identity of the lanes that share a probe, then the probe against the oracle
    worst = [0.0, 0.0, 0.0]
    for k in sorted(set(lanes.tolist())):
        idx = np.flatnonzero(lanes == k)
        if ref[k] is None:
            continue
        for a in (mf, cf, cfx):
            diff = np.any(bits(a[:, idx]) != bits(a[:, idx[:1]]), axis=0)
            assert not diff.any(), (what, 'lanes of probe %d differ from lane %d' % (k, idx[0]), idx[diff].tolist()[:20])
        if not oracle:
            continue
        b0 = idx[0]
        g = (mf[:, b0], cf[:, b0].reshape(E, E), cfx[:, b0].reshape(E, D))
        q = go.ratios(g, ref[k])
        worst = [max(a, b) for a, b in zip(worst, q)]
        if max(q) >= go.K:
            i = int(np.argmax(q))
            with np.errstate(invalid='ignore', divide='ignore'):
                r = np.abs(g[i] - ref[k][i]) / (go.EPS * ref[k][3 + i])
            e = np.unravel_index(int(np.nanargmax(r)), r.shape)
            print('%s probe %d %s entry %s: got %.17g want %.17g ratio %.3g' % (what, k, ('mean', 'cov', 'cross')[i], e, g[i][e], ref[k][i][e], r[e]))
    if oracle:
        print('%s: device / (eps (A + S)): mean %.3g cov %.3g cross %.3g (K = %g)' % ((what,) + tuple(worst) + (go.K,)))
        for tag, v in zip(('mean', 'cov', 'cross'), worst):
            assert within(v, go.K, 'apply_generic %s %s' % (tag, what)), (what, tag, v, go.K)
    return worst


def call_planes(case, B, ld):
    """The probe of every lane (tiled, the non-PD one also last) and the time plane: every item its own time."""
    lanes = [go.lane_probe(b, B) for b in range(B)]
    _, _, time = go.probes_for(case.F, case.D, case.sidx)
    tpl = np.full(ld, SENT)
    tpl[:B] = time[lanes]
    return lanes, tpl


@pytest.mark.parametrize('case', go.CASES, ids=[go.case_id(c) for c in go.CASES])
def test_apply_generic_table(amd, monkeypatch, case):
    assert len(go.CASES) == go.EXPECTED_CASES
    B = go.batch_of(case)
    ld = B + 7 + (B & 1)                                          # even and above the batch
    lanes, times = call_planes(case, B, ld)
    name, got = run(case, lanes, ld, times, 1, monkeypatch)
    assert name == case.kernel, (name, go.case_id(case))
    w = check(case, go.case_id(case), lanes, got, go.reference(case))
    key = (case.kernel, go.form_tag(case))
    WORST[key] = tuple(max(a, b) for a, b in zip(WORST.get(key, (0.0,) * 3), w))
    if case is go.CASES[-1]:
        for k in sorted(WORST):
            print('worst of the table: %-13s %-6s mean %.3g cov %.3g cross %.3g' % (k + WORST[k]))


# ---- k_apply_tile at the edges of its groups, chunks, grid and stores -------------------------------------------------------------
EDGE = (go.Case(go.TILE, (), 'SSMQ_F_PENDULUM_DYN', 2, None, 2, 12, ao.FORM_BQ, 0),        # G = 4, KS = 4
        go.Case(go.TILE, (), 'SSMQ_F_PENDULUM_DYN', 2, None, 2, 40, ao.FORM_BQ, 1))        # G = 1, KS = 13
EDGE_IDS = ['G4-N12', 'G1-N40']


def _first_lanes(case, got, lanes):
    """Bits of the first lane of every good probe: what every other call of the shape must reproduce."""
    lanes = np.asarray(lanes)
    return {k: [bits(a[:, np.flatnonzero(lanes == k)[0]]).copy() for a in got[:3]] for k in range(go.N_PROBES) if k != go.BAD_PROBE and k in lanes}


def _same_bits(case, what, got, lanes, want):
    lanes = np.asarray(lanes)
    for k, planes in want.items():
        idx = np.flatnonzero(lanes == k)
        for a, w in zip(got[:3], planes):
            diff = np.any(bits(a[:, idx]) != w[:, None], axis=0)
            assert not diff.any(), (what, 'probe %d' % k, idx[diff].tolist()[:20])


@pytest.fixture(scope='module')
def edge_base(amd):
    """Per edge shape: the aligned even-pitch call at three rounds and a ragged one, held to the oracle once; its bits serve every
    other call."""
    mp = pytest.MonkeyPatch()
    out = {}
    try:
        for case in EDGE:
            assert go.tile_g(case.N) == (4 if case.N == 12 else 1) and case.D == case.E == 2
            B = go.batch_of(case)
            ld = B + 7 + (B & 1)
            lanes, times = call_planes(case, B, ld)
            name, got = run(case, lanes, ld, times, 1, mp)
            assert name == go.TILE
            check(case, 'edge base ' + go.case_id(case), lanes, got, go.reference(case))
            out[case] = (_first_lanes(case, got, lanes), got, lanes, ld)
    finally:
        mp.undo()
    return out


@pytest.mark.parametrize('case', EDGE, ids=EDGE_IDS)
def test_tile_batch_sizes_around_a_group_and_a_chunk(amd, monkeypatch, edge_base, case):
    """B = 1, G - 1, G, G + 1, 4 G - 1, 4 G, 4 G + 1: partly filled waves, a full chunk (compile-time store map), one trajectory beyond
    it (the ragged map with a single double as its only piece)."""
    want, G = edge_base[case][0], go.tile_g(case.N)
    for B in sorted({1, G - 1, G, G + 1, 4 * G - 1, 4 * G, 4 * G + 1} - {0}):
        ld = B + 2 + (B & 1)
        lanes = [b % go.N_PROBES for b in range(B)]               # (B = 1: the good probe 0; the non-PD one from B = 4 on)
        _, _, time = go.probes_for(case.F, case.D, case.sidx)
        times = np.full(ld, SENT)
        times[:B] = time[lanes]
        name, got = run(case, lanes, ld, times, 1, monkeypatch)
        assert name == go.TILE
        check(case, 'B = %d' % B, lanes, got, go.reference(case), oracle=False)
        _same_bits(case, 'B = %d' % B, got, lanes, want)


@pytest.mark.parametrize('case', EDGE, ids=EDGE_IDS)
def test_tile_batch_above_the_grid_cap(amd, monkeypatch, edge_base, case):
    """512 workgroups of 4 G trajectories, one more chunk and one more trajectory: the first workgroup walks a second chunk with the
    next group fetched ahead, the second one a ragged chunk of one, every other one clamps its fetch address."""
    want, G = edge_base[case][0], go.tile_g(case.N)
    B = go.CUS * go.TILE_WGS_PER_CU * go.TILE_WAVES * G + go.TILE_WAVES * G + 1
    assert B == 512 * 4 * G + 4 * G + 1
    ld = B + 1 + (B & 1) + 6
    lanes, times = call_planes(case, B, ld)
    name, got = run(case, lanes, ld, times, 1, monkeypatch)
    assert name == go.TILE
    check(case, 'B = %d' % B, lanes, got, go.reference(case), oracle=False)
    _same_bits(case, 'B = %d' % B, got, lanes, want)


@pytest.mark.parametrize('case', EDGE, ids=EDGE_IDS)
def test_tile_odd_pitch_and_unaligned_planes(amd, monkeypatch, edge_base, case):
    """The 16-byte stores need three 16-byte-aligned output bases and an even pitch; an odd pitch, and an even one with every base 8 bytes
    off (between canaries), take the scalar stores: the bits of the aligned call, nothing written outside."""
    want, base, lanes, ld = edge_base[case]
    B = len(lanes)
    for what, ldx, shift in (('odd pitch', ld + 1, 0), ('bases 8 mod 16', ld, 1)):
        _, times = call_planes(case, B, ldx)
        name, got = run(case, lanes, ldx, times, 1, monkeypatch, shift=shift)
        assert name == go.TILE
        check(case, what, lanes, got, go.reference(case), oracle=False)
        _same_bits(case, what, got, lanes, want)
        for a, b in zip(got[:3], base[:3]):
            assert np.array_equal(bits(a[:, :B][:, np.asarray(lanes) != go.BAD_PROBE]), bits(b[:, :B][:, np.asarray(lanes) != go.BAD_PROBE])), what


def test_tile_time_per_item_and_broadcast(amd, monkeypatch):
    """UNGM dynamics at N = 15 (G = 4): every item its own time, then one time for the whole batch read from a one-element plane."""
    case = go.Case(go.TILE, (), 'SSMQ_F_UNGM_DYN', 1, None, 1, 15, ao.FORM_BQ, 0)
    B = go.batch_of(case)
    ld = B + 7 + (B & 1)
    lanes, times = call_planes(case, B, ld)
    name, got = run(case, lanes, ld, times, 1, monkeypatch)
    assert name == go.TILE
    check(case, 'time per item', lanes, got, go.reference(case))
    fid, p, sidx = go.model_of(case)
    mean, cov, time = go.probes_for(case.F, case.D, case.sidx)
    t0 = float(time[2])
    ref = [None if k == go.BAD_PROBE else go.transform_hp(fid, p, sidx, case.form, go.rule_for(case), mean[k], cov[k], t0) for k in range(go.N_PROBES)]
    name, got0 = run(case, lanes, ld, np.array([t0]), 0, monkeypatch)
    assert name == go.TILE
    check(case, 'broadcast time', lanes, got0, ref)
    k2 = np.flatnonzero(np.asarray(lanes) == 2)                   # probe 2 keeps its own time in both calls, the others do not
    assert np.array_equal(bits(got0[0][:, k2]), bits(got[0][:, k2])) and not np.array_equal(bits(got0[0][:, :B]), bits(got[0][:, :B]))
