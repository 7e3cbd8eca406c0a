"""The matrix-core transform routes for more than 64 points - k_bq_fused, the two- and three-pass routes over k_eval_wave /
k_fxwc_cov_mfma / k_fxwc_mfma, k_bq_stream and the blocked route k_apply_big - through the C entry points ssmq_transform_create /
ssmq_apply_kernel_name / ssmq_apply_batch_dev and ssmq_apply_fx_batch, entry by entry against the 50-digit restatement at
K eps (A + S), K = max(16, 8 K_REF_MATRIX) with K_REF_MATRIX measured on float64 NumPy by tests/test_apply_matrix_host.py.

The case list is the literal table of tests/_apply_matrix_oracle.py; the test id names the route the restated dispatch gives, and the
kernel the handle reports must be that route's.  Per case one call at whole workgroup tiles plus a ragged one with B E >= 256, at a
pitch above the batch, four probes tiled over the lanes, the non-PD one also in the last, partial tile.  Every trajectory runs the same
instruction sequence whatever its rows in a tile, its block, or the side of k_bq_stream's split it falls on, so lanes that share a
probe must agree bit for bit; one oracle evaluation per probe then pins all lanes.  Also: exact symmetry of cov_f, NaN in the
strict upper triangle of the input covariances, untouched padding lanes, status and NaN outputs of exactly the non-PD lanes.

The name query has no batch (it reports the route of a large one), so the row threshold is pinned by bits: below B E = 256 a batch
must reproduce the SSMQ_NO_MFMA run - k_apply_wide by name - bit for bit, at the threshold it must not, and both meet the oracle.

Out of reach here: cov_add / cov_scale / ccov_scale (set by the filters only), per-item constants, E = 9 (no built-in integrand has nine
outputs), N beyond what E N^2 <= 1e6 multiply-adds of the 50-digit reference allow."""
import ctypes

import numpy as np
import pytest

from tests import _apply_matrix_oracle as mo
from tests import _apply_small_oracle as ao
from tests._cases import within

pytestmark = pytest.mark.gpu

SENT = -7.0259e+211                  # sentinel of the output planes, padding lanes included
ST_SENT = 0x5A5A5A5A                 # sentinel of the status plane
SWITCHES = ('SSMQ_NO_MFMA', 'SSMQ_NO_BQ_FUSED', 'SSMQ_NO_BQ_STREAM', 'SSMQ_NO_FUSED_COV', 'SSMQ_BQ_STREAM_MIN_N', 'SSMQ_BQ_STREAM_NO_SPLIT',
                'SSMQ_NO_TILE', 'SSMQ_NO_WAVE', 'SSMQ_NO_FASTPATH')
WORST = {}                           # (route, form) -> worst ratios of the table tests, for the record printed at their end


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


def ptr(b):
    return ctypes.c_void_p(b.ptr)


def compute_units():
    """The device's compute-unit count from the HIP runtime the library is linked against (the attribute launch_bq_stream's caller
    reads as multiProcessorCount).  torch.cuda sees no device in a process whose GPU this library has opened, so it is not asked."""
    from ssmtoybox_amd import _lib
    v = ctypes.c_int(0)
    rc = _lib.load().hipDeviceGetAttribute(ctypes.byref(v), 63, 0)        # hipDeviceAttributeMultiprocessorCount
    assert rc == 0 and 16 <= v.value <= 1024, (rc, v.value)
    return v.value


def run(case, lanes, ld, monkeypatch, env=None):
    """One call under the case's switches (or `env`): `lanes` lists the probe of every lane (B = len(lanes)).  Returns the kernel name
    of the handle and the raw planes mean_f (E, ld), cov_f (E E, ld), cov_fx (E D, ld), status (ld,)."""
    from ssmtoybox_amd import _lib
    lib = _lib.load()
    env = case.env if env is None else env
    for k, v in env:
        monkeypatch.setenv(k, v)
    D, E, B = case.D, case.E, len(lanes)
    rule = mo.rule_for(case)
    fid, p, sidx = mo.model_of(case)
    mean, cov, time = mo.probes_for(case)
    c = lambda a: None if a is None else _lib.as_c(a)[1]
    keep = [np.ascontiguousarray(rule[k], dtype=float) if rule[k] is not None else None for k in ('xi', 'wm', 'Wc', 'Wcc', 'emv', 'iK')]
    h = lib.ssmq_transform_create(D, E, case.N, case.form, c(keep[0]), c(keep[1]), c(keep[2]), c(keep[3]), c(keep[4]), int(rule['emv_mode']),
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
        t_pl = np.full(ld, SENT)
        t_pl[:B] = time[lanes]
        outs = [np.full(n * ld, SENT) for n in (E, E * E, E * D)]
        st = np.full(ld, ST_SENT, dtype=np.int32)
        for host in [m_pl, c_pl, t_pl] + outs + [st]:
            b = _lib.DeviceBuffer(host.nbytes)
            b.upload(host)
            bufs.append(b)
        rc = lib.ssmq_apply_batch_dev(ctypes.c_void_p(h), ctypes.byref(integ), B, ld, ptr(bufs[0]), ptr(bufs[1]), ptr(bufs[2]),
                                      1, ptr(bufs[3]), ptr(bufs[4]), ptr(bufs[5]), ptr(bufs[6]))
        assert rc == 0, (case, rc, _lib.last_error())
        _lib.check(lib.ssmq_sync(), 'ssmq_sync')
        got = [bufs[3 + i].download(outs[i].shape).reshape(-1, ld) for i in range(3)] + [bufs[6].download((ld,), dtype=np.int32)]
    finally:
        for b in bufs:
            b.free()
        lib.ssmq_transform_destroy(ctypes.c_void_p(h))
        for k, _ in env:
            monkeypatch.delenv(k)
    return buf.value.decode(), got


def _oracle_bar(what, k, g, ref, worst):
    q = mo.ratios(g, ref)
    if max(q) >= mo.K:
        i = int(np.argmax(q))
        with np.errstate(invalid='ignore', divide='ignore'):
            r = np.abs(g[i] - ref[i]) / (mo.EPS * ref[3 + i])
        e = np.unravel_index(int(np.nanargmax(r)), r.shape)
        print('%s probe %d %s entry %s: got %.17g want %.17g ratio %.3g' % (what, k, ('mean', 'cov', 'cross')[i], e, g[i][e], ref[i][e], r[e]))
    return [max(a, b) for a, b in zip(worst, q)]


def check(case, what, lanes, got, ref):
    """Everything the module's text promises of one call's planes, against the per-probe references `ref`.  Returns the worst ratios."""
    D, E, B = case.D, case.E, len(lanes)
    mf, cf, cfx, st = got
    lanes = np.asarray(lanes)
    for a in (mf, cf, cfx):
        assert np.all(bits(a[:, B:]) == bits(np.array(SENT))), (what, 'padding lanes written')
    assert np.all(st[B:] == ST_SENT), (what, 'status of padding lanes written')
    bad = np.array([ref[k] is None for k in lanes])
    assert np.all(st[:B][~bad] == 0) and np.all(st[:B][bad] != 0), (what, st[:B].tolist()[:64])
    for a in (mf, cf, cfx):
        assert np.all(np.isnan(a[:, :B][:, bad])) and np.all(np.isfinite(a[:, :B][:, ~bad])), (what, 'NaN / finite lanes')
    c3 = cf[:, :B].reshape(E, E, B)
    assert np.all(bits(c3[:, :, ~bad]) == bits(c3.transpose(1, 0, 2)[:, :, ~bad])), (what, 'cov_f not symmetric')
    worst = [0.0, 0.0, 0.0]
    for k in sorted(set(lanes.tolist())):
        idx = np.flatnonzero(lanes == k)
        if ref[k] is None:
            continue
        for a in (mf, cf, cfx):
            diff = np.any(bits(a[:, idx]) != bits(a[:, idx[:1]]), axis=0)
            assert not diff.any(), (what, 'lanes of probe %d differ from lane %d' % (k, idx[0]), idx[diff].tolist()[:20])
        b0 = idx[0]
        worst = _oracle_bar(what, k, (mf[:, b0], cf[:, b0].reshape(E, E), cfx[:, b0].reshape(E, D)), ref[k], worst)
    print('%s: device / (eps (A + S)): mean %.3g cov %.3g cross %.3g (K = %g)' % ((what,) + tuple(worst) + (mo.K,)))
    for tag, v in zip(('mean', 'cov', 'cross'), worst):
        assert within(v, mo.K, 'apply_matrix %s %s' % (tag, what)), (what, tag, v, mo.K)
    return worst


def _record(key, w, last):
    WORST[key] = tuple(max(a, b) for a, b in zip(WORST.get(key, (0.0,) * 3), w))
    if last:
        for k in sorted(WORST):
            print('worst of the table: %-12s %-10s mean %.3g cov %.3g cross %.3g' % (k + WORST[k]))


@pytest.mark.parametrize('case', mo.CASES, ids=[mo.case_id(c) for c in mo.CASES])
def test_apply_matrix_table(amd, monkeypatch, case):
    assert len(mo.CASES) == mo.EXPECTED_CASES
    assert mo.restated_route(case) == case.route
    cus = compute_units() if case.batch == 'split' else 256
    B = mo.batch_of(case, cus)
    assert B * case.E >= mo.GEMM_MIN_ROWS
    if case.batch == 'split':                                     # more blocks than compute units, the last round cut by panel
        nblocks = -(-B // mo.bq_stream_tpw(case.E))
        assert nblocks > cus and mo.bq_stream_split(nblocks, mo.bq_stream_panels(case.N), cus)[1] > 0
    ld = B + 7 + (B & 1)                                          # even and above the batch
    lanes = [mo.lane_probe(b, B) for b in range(B)]
    name, got = run(case, lanes, ld, monkeypatch)
    assert name == mo.KERNEL_NAME[case.route], (name, mo.case_id(case))
    w = check(case, mo.case_id(case), lanes, got, mo.reference(case))
    _record((case.route, mo.form_tag(case)), w, case is mo.CASES[-1])


@pytest.mark.parametrize('case', mo.THRESHOLD, ids=[mo.case_id(c) for c in mo.THRESHOLD])
def test_row_threshold(amd, monkeypatch, case):
    """B E just below kGemmMinRows runs on k_apply_wide, the first B at or above it on the matrix-core route."""
    assert len(mo.THRESHOLD) == 5
    below, at = mo.threshold_batches(case)
    assert below * case.E < mo.GEMM_MIN_ROWS <= at * case.E
    assert mo.restated_route(case, below * case.E) == mo.WIDE and mo.restated_route(case, at * case.E) == case.route
    ref = mo.reference(case)
    for B, same in ((below, True), (at, False)):
        ld = B + 3 + (B & 1)
        lanes = [mo.lane_probe(b, B) for b in range(B)]
        name, got = run(case, lanes, ld, monkeypatch)
        assert name == mo.KERNEL_NAME[case.route]
        check(case, '%s B = %d' % (mo.case_id(case), B), lanes, got, ref)
        wname, wide = run(case, lanes, ld, monkeypatch, env=(('SSMQ_NO_MFMA', '1'),))
        assert wname == 'k_apply_wide'
        good = np.asarray(lanes) != mo.BAD_PROBE
        equal = all(np.array_equal(bits(a[:, :B][:, good]), bits(b[:, :B][:, good])) for a, b in zip(got[:3], wide[:3]))
        assert equal == same, (mo.case_id(case), B, 'bits equal to the k_apply_wide run: %s' % equal)


@pytest.mark.parametrize('case', mo.FX_CASES, ids=[mo.fx_case_id(c) for c in mo.FX_CASES])
def test_apply_fx_batch_table(amd, case):
    """Host-supplied integrand values and factors through ssmq_apply_fx_batch: E = 11 and 13 (three passes), 12 and 16 (covariance
    epilogue), 16 on the blocked route; the reference is the linear algebra alone."""
    from ssmtoybox_amd import _lib
    lib = _lib.load()
    assert len(mo.FX_CASES) == mo.EXPECTED_FX_CASES
    D, E, N = case.D, case.E, case.N
    r = max(1, 64 // E)
    B = 4 * r + r // 2 + 1
    while B * E < mo.GEMM_MIN_ROWS:
        B += r
    assert mo.fx_route(case, B * E) == case.route
    rule, fxp, cholp = mo.fx_inputs(case)
    ref = mo.fx_reference(case)
    lanes = np.arange(B) % mo.FX_PROBES
    fx, chol = np.ascontiguousarray(fxp[lanes]), np.ascontiguousarray(cholp[lanes])
    c = lambda a: _lib.as_c(a)[1]
    keep = [np.ascontiguousarray(rule[k], dtype=float) for k in ('xi', 'wm', 'Wc', 'Wcc', 'emv')]
    h = lib.ssmq_transform_create(D, E, N, ao.FORM_BQ, c(keep[0]), c(keep[1]), c(keep[2]), c(keep[3]), c(keep[4]), int(rule['emv_mode']), 0.0, None)
    assert h, _lib.last_error()
    try:
        mf, cf, cfx = np.full((B, E), SENT), np.full((B, E, E), SENT), np.full((B, E, D), SENT)
        _lib.check(lib.ssmq_apply_fx_batch(ctypes.c_void_p(h), B, c(chol), None, None, c(fx), c(mf), c(cf), c(cfx)), 'ssmq_apply_fx_batch')
    finally:
        lib.ssmq_transform_destroy(ctypes.c_void_p(h))
    what = mo.fx_case_id(case)
    assert np.all(np.isfinite(mf)) and np.all(np.isfinite(cf)) and np.all(np.isfinite(cfx)), what
    assert np.array_equal(bits(cf), bits(cf.transpose(0, 2, 1))), (what, 'cov_f not symmetric')
    worst = [0.0, 0.0, 0.0]
    for k in range(mo.FX_PROBES):
        idx = np.flatnonzero(lanes == k)
        for a in (mf, cf, cfx):
            diff = np.any((bits(a[idx]) != bits(a[idx[:1]])).reshape(len(idx), -1), axis=1)
            assert not diff.any(), (what, 'items of probe %d differ from item %d' % (k, idx[0]), idx[diff].tolist()[:20])
        worst = _oracle_bar(what, k, (mf[idx[0]], cf[idx[0]], cfx[idx[0]]), ref[k], worst)
    print('%s: device / (eps A): mean %.3g cov %.3g cross %.3g (K = %g)' % ((what,) + tuple(worst) + (mo.K,)))
    for tag, v in zip(('mean', 'cov', 'cross'), worst):
        assert within(v, mo.K, 'apply_matrix %s %s' % (tag, what)), (what, tag, v, mo.K)
    _record(('fx ' + case.route, 'BQ'), worst, case is mo.FX_CASES[-1])
