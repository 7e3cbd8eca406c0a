"""Every instantiation of k_apply_small (csrc/ssmq_apply_small.h; the four dispatch tables ssmq_small_{a,b,c,d}.hip) through the C
entry points ssmq_transform_create / ssmq_apply_kernel_name / ssmq_apply_batch_dev, entry by entry against the 50-digit restatement
of tests/_apply_small_oracle.py at K eps (A + S), K = max(16, 8 K_REF) with K_REF measured on float64 NumPy by
tests/test_apply_small_host.py.

The case list is the table itself (read from the .hip files), the test id the kernel's name: a rule builder that does not reach its
kernel fails.  Per case: B = 131 lanes at pitch 192 (two waves and a ragged third), ten probe items tiled over the lanes - condition
numbers up to 1e3, one ill-scaled covariance, one that is not positive definite (also on the last lane) - each with its own time.
The kernel is one trajectory per lane with no cross-lane work, so bit identity of the lanes that share a probe pins all 131 lanes
for the price of ten oracle evaluations.  Also: exact symmetry of cov_f, NaN in the strict upper triangle of the input covariances
(only the lower one is read), untouched padding lanes, status and NaN outputs of the non-PD lanes.

Out of reach: the plain-store variant of the OPT != 0 kernels (stream_out = 0) is selected only inside the filters' launch loop - no
apply entry point selects it; it stays covered by the filter tests alone."""
import ctypes

import numpy as np
import pytest

from tests import _apply_small_oracle as ao
from tests._cases import within

pytestmark = pytest.mark.gpu

SENT = -7.0259e+211                  # sentinel of the output planes, padding lanes included
ST_SENT = 0x5A5A5A5A                 # sentinel of the status plane
ROWS = ao.table_rows()
FAST_SHAPES = [r for r in ROWS if r.opt == 7]


@pytest.fixture(scope='module')
def amd():
    import ssmtoybox_amd
    if ssmtoybox_amd.device_count() < 1:
        pytest.fail('no device: the GPU tests need an MI355X')
    ssmtoybox_amd.set_device(0)
    return ssmtoybox_amd


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    for v in ('SSMQ_NO_SYM', 'SSMQ_NO_FASTPATH'):
        monkeypatch.delenv(v, raising=False)


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def ptr(b):
    return None if b is None else ctypes.c_void_p(b.ptr)


def run(row, rule, lanes, ld, times, time_stride):
    """One call: `lanes` lists the probe of every lane (B = len(lanes)), `times` is the time plane as uploaded.  Returns the kernel
    name of the handle and the raw planes mean_f (E, ld), cov_f (E E, ld), cov_fx (E D, ld), status (ld,)."""
    from ssmtoybox_amd import _lib
    lib = _lib.load()
    D, E, N, B = row.D, row.E, row.N, len(lanes)
    fid, p, sidx = ao.model_of(row)
    mean, cov, _ = ao.probes_for(row.F, row.D, row.sel)
    c = lambda a: None if a is None else _lib.as_c(a)[1]
    keep = [np.ascontiguousarray(rule[k], dtype=float) if rule[k] is not None else None for k in ('xi', 'wm', 'Wc', 'Wcc', 'emv', 'iK')]
    h = lib.ssmq_transform_create(D, E, N, row.form, c(keep[0]), c(keep[1]), c(keep[2]), c(keep[3]), c(keep[4]), int(rule['emv_mode']),
                                  float(rule['nu']), c(keep[5]))
    assert h, (row.name, _lib.last_error())
    bufs = []
    try:
        integ = _lib.Integrand.make(fid, p, sidx)
        buf = ctypes.create_string_buffer(256)
        _lib.check(lib.ssmq_apply_kernel_name(ctypes.c_void_p(h), ctypes.byref(integ), buf, 256), 'ssmq_apply_kernel_name')
        m_pl = np.full((D, ld), SENT)
        m_pl[:, :B] = mean[lanes].T
        c_pl = np.full((D * D, ld), SENT)
        cl = cov[lanes].copy()                                   # (B, D, D)
        cl[:, np.triu_indices(D, 1)[0], np.triu_indices(D, 1)[1]] = np.nan       # the header: only the lower triangle is read
        c_pl[:, :B] = cl.reshape(B, D * D).T
        outs = [np.full((E, ld), SENT), np.full((E * E, ld), SENT), np.full((E * D, ld), SENT)]
        st = np.full(ld, ST_SENT, dtype=np.int32)
        for host in [m_pl, c_pl, np.ascontiguousarray(times, dtype=float)] + outs + [st]:
            b = _lib.DeviceBuffer(host.nbytes)
            b.upload(host)
            bufs.append(b)
        rc = lib.ssmq_apply_batch_dev(ctypes.c_void_p(h), ctypes.byref(integ), B, ld, ptr(bufs[0]), ptr(bufs[1]), ptr(bufs[2]),
                                      time_stride, ptr(bufs[3]), ptr(bufs[4]), ptr(bufs[5]), ptr(bufs[6]))
        assert rc == 0, (row.name, rc, _lib.last_error())
        _lib.check(lib.ssmq_sync(), 'ssmq_sync')
        got = [bufs[3 + i].download(outs[i].shape) for i in range(3)] + [bufs[6].download((ld,), dtype=np.int32)]
    finally:
        for b in bufs:
            b.free()
        lib.ssmq_transform_destroy(ctypes.c_void_p(h))
    return buf.value.decode(), got


def check(row, what, lanes, got, ref):
    """Everything the module's text promises of one call's planes, against the per-probe references `ref`."""
    D, E, B = row.D, row.E, len(lanes)
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
            assert np.all(bits(a[:, idx]) == bits(a[:, idx[:1]])), (what, 'lanes of probe %d differ' % k, idx[np.any(bits(a[:, idx]) != bits(a[:, idx[:1]]), axis=0)].tolist())
        b0 = idx[0]
        q = ao.ratios((mf[:, b0], cf[:, b0].reshape(E, E), cfx[:, b0].reshape(E, D)), ref[k])
        worst = [max(a, b) for a, b in zip(worst, q)]
        if max(q) >= ao.K:
            g = (mf[:, b0], cf[:, b0].reshape(E, E), cfx[:, b0].reshape(E, D))
            i = int(np.argmax(q))
            r = np.abs(g[i] - ref[k][i]) / (ao.EPS * ref[k][3 + i])
            e = np.unravel_index(int(np.nanargmax(r)), r.shape)
            print('%s probe %d %s entry %s: got %.17g want %.17g ratio %.3g' % (what, k, ('mean', 'cov', 'cross')[i], e, g[i][e], ref[k][i][e], r[e]))
    print('%s: device / (eps (A + S)): mean %.3g cov %.3g cross %.3g (K = %g)' % ((what,) + tuple(worst) + (ao.K,)))
    for tag, v in zip(('mean', 'cov', 'cross'), worst):
        assert within(v, ao.K, 'apply_small %s %s' % (tag, what)), (what, tag, v, ao.K)
    return worst


def table_case(row):
    lanes = [ao.lane_probe(b) for b in range(ao.B_LANES)]
    _, _, time = ao.probes_for(row.F, row.D, row.sel)
    times = np.full(ao.LD, SENT)
    times[:ao.B_LANES] = time[lanes]
    return lanes, times


@pytest.mark.parametrize('row', ROWS, ids=[r.name for r in ROWS])
def test_apply_small_table(amd, row):
    assert len(ROWS) == ao.EXPECTED_ROWS
    rule = ao.rule_for(row)
    lanes, times = table_case(row)
    name, got = run(row, rule, lanes, ao.LD, times, 1)
    assert name == row.name, (name, row.name)
    check(row, row.name, lanes, got, ao.reference(row))


@pytest.mark.parametrize('row', FAST_SHAPES, ids=[r.name for r in FAST_SHAPES])
def test_one_rule_on_every_fast_path(amd, monkeypatch, row):
    """The reflection-symmetric rule of a fast-path shape on its OPT = 7, 3, 1 and 0 kernels, each against the oracle at the same bar
    (not against each other): SSMQ_NO_SYM / SSMQ_NO_FASTPATH at handle creation switch the symmetric and all fast paths off; listing
    the points in another order - the same rule - fails the host's unscented-type test and leaves the LDL' kernel alone."""
    assert len(FAST_SHAPES) == 6
    rule = ao.rule_for(row)
    lanes, times = table_case(row)
    ref = ao.reference(row)
    rng = np.random.default_rng([20275, row.D, row.E])
    perm = None
    for _ in range(50):
        q = rng.permutation(row.N)
        if ao._ldl_accepts(rule['Wc'][np.ix_(q, q)]) and not np.array_equal(rule['xi'][:, q], rule['xi']):
            perm = q
            break
    assert perm is not None
    prule = ao.permuted_rule(rule, perm)
    for opt, env, rl, rf in ((7, None, rule, ref), (3, 'SSMQ_NO_SYM', rule, ref), (1, None, prule, None), (0, 'SSMQ_NO_FASTPATH', rule, ref)):
        if env:
            monkeypatch.setenv(env, '1')
        name, got = run(row, rl, lanes, ao.LD, times, 1)
        if env:
            monkeypatch.delenv(env)
        want = ao.kernel_name(row.F, row.D, row.E, row.N, row.form, row.tp, row.sel, opt)
        assert name == want, (name, want)
        check(row, 'one rule: ' + want, lanes, got, rf if rf is not None else ao.reference(row, prule))


def _one_per_file():
    out = []
    for fname in ao.TABLE_FILES:
        rows = [r for r in ROWS if r.file == fname]
        pick = [r for r in rows if r.opt == 7] or [r for r in rows if r.F == 'SSMQ_F_UNGM_DYN' and r.N == 3 and r.form == ao.FORM_BQ and not r.tp]
        out.append(pick[0])
    return out


@pytest.mark.parametrize('row', _one_per_file(), ids=[r.name for r in _one_per_file()])
def test_broadcast_time_and_single_item(amd, row):
    """time_stride = 0: one time for the whole batch, read from a one-element plane; and B = 1 at pitch 1."""
    rule = ao.rule_for(row)
    fid, p, sidx = ao.model_of(row)
    mean, cov, time = ao.probes_for(row.F, row.D, row.sel)
    lanes = [ao.lane_probe(b) for b in range(ao.B_LANES)]
    t0 = float(time[5])
    ref = [None if k == ao.BAD_PROBE else ao.transform_hp(fid, p, sidx, row.form, rule, mean[k], cov[k], t0) for k in range(ao.N_PROBES)]
    name, got = run(row, rule, lanes, ao.LD, np.array([t0]), 0)
    assert name == row.name
    check(row, 'broadcast time: ' + row.name, lanes, got, ref)
    for k in (0, ao.BAD_PROBE):
        name, got = run(row, rule, [k], 1, np.array([time[k]]), 1)
        assert name == row.name
        check(row, 'B = 1, probe %d: %s' % (k, row.name), [k], got, ao.reference(row))
