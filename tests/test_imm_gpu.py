"""The IMM filter over noise modes on the device (k_imm_loop<>): against the CPU restatement (tests/_imm_oracle.py) on the device's
weights, one mode against the two-call path, identity transitions against the noise sweep, bit-for-bit independence of the batch,
failures that stay local (and do not disturb the barriers of their workgroup), the refusals of the C entry points, the object unchanged.

Cases: tests/_imm_cases.py.  Bounds: loglik by the rule of tests/test_innovation_gpu.py - max(RTOL, 64 cond(S) eps) max(1, |value|), cond(S)
the largest over the modes; mean, cov and mode_prob by the float64 oracle's distance to its long-double twin, measured on the CPU
(tests/_imm_cases.py: TWIN - per case max |difference| / max(1, |value|): mean 4.5e-16 .. 1.5e-13, cov 2.0e-17 .. 6.7e-12, mode_prob
2.8e-16 .. 1.1e-12) times MARGIN = 64 for the device's other summation order, FMA contraction and div_nr.  On an MI355X the largest
|error| / bound is 0.034 against the oracle (ungm_ukf, mode_prob; mean 0.022, cov 0.018, loglik 0.0013) and 0.035 against the two-call
path (ct_tp at M = 1, which runs k_filter_wsplit and the OPT = 2 innovation kernel there); ungm_ukf, pend_ckf and cv_gp at M = 1 have the
bits of the two-call path."""
import ctypes

import numpy as np
import pytest

from tests import _imm_cases as ic
from tests import _imm_oracle as imo
from tests import _noise_sweep_cases as nc
from tests._cases import RTOL
from tests.test_noise_sweep_gpu import device_weights

pytestmark = pytest.mark.gpu
EPS = float(np.finfo(float).eps)
KEYS = ('mean', 'cov', 'mode_prob', 'loglik', 'loglik_total', 'status')


@pytest.fixture(scope='module')
def amd():
    import ssmtoybox_amd
    if ssmtoybox_amd.device_count() < 1:
        pytest.fail('no device: the GPU tests need an MI355X')
    ssmtoybox_amd.set_device(0)
    return ssmtoybox_amd


_RUNS, _DEV_REFS = {}, {}


def run_case(amd, name):
    """The case's IMM pass on the device, once, shared by the tests (never modified)."""
    if name not in _RUNS:
        c = ic.get(name)
        alg = nc.make_filter(name)
        _RUNS[name] = dict(alg=alg, out=alg.imm_pass_batch(c['y'], **ic.args(c)))
    return _RUNS[name]


def device_weights_reference(amd, name):
    """The oracle's pass of the case on the DEVICE's weights (the sigma-point rules have none to hand over), computed once."""
    if name not in _DEV_REFS:
        w = device_weights(run_case(amd, name)['alg'])
        _DEV_REFS[name] = ic.reference(name) if w is None else ic.oracle(ic.get(name), weights=w)
    return _DEV_REFS[name]


def equal(a, b, keys=KEYS):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in keys)


def ratios(name, out, ref):
    """Largest |error| / bound per output."""
    tw = ic.TWIN[name]
    bl = np.maximum(RTOL, 64.0 * ref['cond'] * EPS) * np.maximum(1.0, np.abs(ref['loglik']))
    r = {k: float(np.max(np.abs(out[k] - ref[k]) / (ic.MARGIN * tw[k] * np.maximum(1.0, np.abs(ref[k]))))) for k in ('mean', 'cov', 'mode_prob')}
    r['loglik'] = float(np.max(np.abs(out['loglik'] - ref['loglik']) / bl))
    r['loglik_total'] = float(np.max(np.abs(out['loglik_total'] - ref['loglik_total']) / bl.sum(axis=0)))
    return r


@pytest.mark.parametrize('name', ic.NAMES)
def test_against_the_oracle(amd, name):
    c, r, ref = ic.get(name), run_case(amd, name), device_weights_reference(amd, name)
    assert r['alg'].imm_kernel_name(c['M']).startswith('k_imm_loop<D={},Y={},'.format(c['m0'].shape[0], c['R'].shape[0]))
    assert not ref['status'].any()
    worst = ratios(name, r['out'], ref)
    print('imm {} against the oracle: largest |error| / bound = {}'.format(name, {k: float('{:.3g}'.format(v)) for k, v in worst.items()}))
    assert np.array_equal(r['out']['status'], ref['status'])
    assert np.array_equal(r['out']['cov'], r['out']['cov'].transpose(1, 0, 2, 3))
    assert max(worst.values()) <= 1.0, worst
    assert np.array_equal(r['alg'].fi_mean, r['out']['mean']) and np.array_equal(r['alg'].status, r['out']['status'])


@pytest.mark.parametrize('name', ic.NAMES)
def test_one_mode_is_the_two_call_path(amd, name):
    """M = 1: forward_pass_batch + innovations_batch - bit for bit where that path runs the dense kernels (the condition of
    tests/test_noise_sweep_gpu.py::test_row_is_the_two_call_path), else within the bounds.  The IMM writes both triangles of a
    covariance from the lower one; the forward pass computes each entry on its own, so the lower triangles are compared."""
    c = ic.get(name)
    B, D = c['B'], c['m0'].shape[0]
    alg = nc.make_filter(name)
    got = alg.imm_pass_batch(c['y'], np.ones((1, 1)))
    two = nc.make_filter(name)
    names = (two.kernel_name(B), two.innovations_kernel_name(B))
    dense = names[0].startswith('k_filter_fused<') and names[1].startswith('k_innovation<') and all(n.endswith('OPT=0>') for n in names)
    fm, fP = two.forward_pass_batch(c['y'], raise_on_failure=False)
    inn = two.innovations_batch(c['y'], fi_mean=fm, fi_cov=fP)
    low = np.tril_indices(D)
    bits = dict(mean=bool(np.array_equal(got['mean'], fm)), cov=bool(np.array_equal(got['cov'][low], fP[low])),
                loglik=bool(np.array_equal(got['loglik'], inn['loglik'])), loglik_total=bool(np.array_equal(got['loglik_total'], inn['loglik_total'])))
    print('imm {} M = 1: the two-call path ran {} ({}); bit-equal: {}'.format(name, names, 'dense' if dense else 'not the dense kernels', bits))
    assert not got['status'].any() and (got['mode_prob'] == 1.0).all()
    if name in ('ungm_ukf', 'pend_ckf') and dense:
        assert all(bits.values()), bits
    else:
        one = imo.imm(c, c['y'], c['q_rows'][:1], c['r_rows'][:1], c['x0_rows'][:1], np.ones((1, 1)), np.ones(1), weights=device_weights(alg))      # (cond)
        sym = np.array(fP)
        sym[low[1], low[0]] = fP[low]
        ref = dict(one, mean=fm, cov=sym, loglik=inn['loglik'], loglik_total=inn['loglik_total'], mode_prob=got['mode_prob'])
        worst = ratios(name, got, ref)
        print('imm {} M = 1 against the two-call path: largest |error| / bound = {}'.format(name, worst))
        assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize('name', ('pend_ckf', 'cv_gp'))
def test_identity_transitions_are_the_noise_sweep(amd, name):
    c, alg = ic.get(name), run_case(amd, name)['alg']
    M, LD = c['M'], np.longdouble
    mu0 = np.arange(1.0, M + 1) / np.arange(1.0, M + 1).sum()
    got = alg.imm_pass_batch(c['y'], **dict(ic.args(c), pi=np.eye(M), mu0=mu0))
    sweep = alg.noise_sweep_batch(c['y'], c['q_cov'], c['r_cov'], c['x0_cov'], steps=True)
    ref = ic.oracle(c, pi=np.eye(M), mu0=mu0, weights=device_weights(alg))
    assert not got['status'].any() and not sweep['status'].any()
    a = np.log(mu0.astype(LD))[:, None] + sweep['loglik_total'].astype(LD)
    lse = a.max(axis=0) + np.log(np.exp(a - a.max(axis=0)).sum(axis=0))
    soft = np.exp(a - lse)
    bound = (np.maximum(RTOL, 64.0 * ref['cond'] * EPS) * np.maximum(1.0, np.abs(ref['loglik']))).sum(axis=0)      # the summed step bounds
    worst = (float(np.max(np.abs(got['loglik_total'] - lse) / bound)), float(np.max(np.abs(got['mode_prob'][:, -1] - soft) / bound)))
    print('imm {} identity transitions: largest |error| / summed step bounds: loglik_total {:.3g}, final mode_prob {:.3g}'.format(name, *worst))
    assert max(worst) <= 1.0


def test_batch_independence_bit_for_bit(amd):
    c, r = ic.get('ungm_ukf'), run_case(amd, 'ungm_ukf')
    alg, out, y, kw = r['alg'], r['out'], c['y'], ic.args(c)
    assert c['B'] == 70
    pick = lambda o, idx: {k: o[k][..., idx] for k in KEYS}      # noqa: E731
    for B in (1, 64, 65, 70):
        assert equal(alg.imm_pass_batch(y[..., :B], **kw), pick(out, slice(0, B))), B
    assert equal(alg.imm_pass_batch(y[..., 69:70], **kw), pick(out, slice(69, 70)))
    perm = np.random.default_rng(1).permutation(70)
    assert equal(alg.imm_pass_batch(y[..., perm], **kw), pick(out, perm))
    one = alg.imm_pass(y[..., 3], **kw)
    assert all(np.array_equal(one[k], out[k][..., 3]) for k in KEYS)
    # the device route: the same bits
    from ssmtoybox_amd import _lib
    (Y, T, B), ld, M = y.shape, 128, c['M']
    d_y = _lib.DeviceBuffer(8 * T * Y * ld)
    _lib.upload_study(y, Y, ld, d_y)
    bufs = alg.imm_pass_dev(d_y, B, ld, T, **kw)
    assert np.array_equal(_lib.download_study(bufs[0], (1,), T, B, ld), out['mean']) and np.array_equal(_lib.download_study(bufs[2], (M,), T, B, ld), out['mode_prob'])
    assert np.array_equal(bufs[4].download((ld,))[:B], out['loglik_total']) and np.array_equal(bufs[5].download((ld,), dtype=np.int32)[:B], out['status'])
    for buf in (d_y,) + tuple(bufs):
        buf.free()


def test_failures_stay_local(amd):
    """One trajectory of a workgroup fails at a known step; the others of the workgroup have the bits of the run without the failure,
    so a poisoned trajectory disturbs neither its neighbours nor the barriers.  Nothing here is out of range for the kernel."""
    c, r = ic.get('ungm_ukf'), run_case(amd, 'ungm_ukf')
    alg, out, kw = r['alg'], r['out'], ic.args(c)
    B, T, step, lane = c['B'], c['T'], ic.FAIL_STEP, ic.FAIL_LANE
    y = c['y'].copy()
    y[0, step, lane] = np.nan
    got = alg.imm_pass_batch(y, raise_on_failure=False, **kw)
    keep = np.arange(B) != lane
    assert got['status'][lane] == 1 + step and not got['status'][keep].any()
    for k in ('mean', 'cov', 'mode_prob', 'loglik'):
        assert np.isnan(got[k][..., step:, lane]).all() and np.array_equal(got[k][..., :step, lane], out[k][..., :step, lane]), k
    assert np.isnan(got['loglik_total'][lane])
    assert equal({k: got[k][..., keep] for k in KEYS}, {k: out[k][..., keep] for k in KEYS})
    with pytest.raises(np.linalg.LinAlgError, match=r'trajectory {}, step {}'.format(lane, step)):
        alg.imm_pass_batch(y, **kw)
    # an indefinite R row in one mode: the oracle's pattern of failures (tests/test_imm_host.py), NaN from the failing step on, and the
    # trajectories that survive have the bits they have in a batch of their own
    rr = ic.failing_r(c)
    want = ic.oracle(c, r_rows=rr)
    got = alg.imm_pass_batch(c['y'], raise_on_failure=False, **dict(kw, r_cov=rr))
    st = got['status']
    assert np.array_equal(st, want['status']) and 0 < np.count_nonzero(st) < B
    for b in np.flatnonzero(st):
        for k in ('mean', 'cov', 'mode_prob', 'loglik'):
            assert np.isnan(got[k][..., st[b] - 1:, b]).all() and np.isfinite(got[k][..., :st[b] - 1, b]).all(), (k, b)
    good = st == 0
    assert np.isnan(got['loglik_total'][~good]).all() and np.isfinite(got['loglik_total'][good]).all()
    alone = alg.imm_pass_batch(c['y'][..., good], **dict(kw, r_cov=rr))
    assert equal(alone, {k: got[k][..., good] for k in KEYS})
    tw = ic.TWIN['ungm_ukf']
    assert np.all(np.abs(alone['mean'] - want['mean'][..., good]) <= ic.MARGIN * tw['mean'] * np.maximum(1.0, np.abs(alone['mean'])))


@pytest.mark.parametrize('name', ('pend_ckf', 'cv_gp'))
def test_the_object_is_unchanged(amd, name):
    c = ic.get(name)
    alg = nc.make_filter(name)
    state = lambda: (alg.tf_dyn.wm, alg.tf_dyn.Wc, alg.tf_obs.wm, alg.tf_obs.Wc, alg.q_cov, alg.r_cov, alg.x0_cov, alg.x0_mean)      # noqa: E731
    before = [np.array(a, copy=True) for a in state()]
    fm = alg.forward_pass_batch(c['y'])[0].copy()
    alg.imm_pass_batch(c['y'], **ic.args(c))
    for a, b in zip(before, state()):
        assert np.array_equal(a, b)
    assert np.array_equal(alg.forward_pass_batch(c['y'])[0], fm)


def test_c_abi_refusals_leave_the_outputs_untouched(amd):
    from ssmtoybox_amd import _lib, ssinf, ssmod as sm
    from tests.test_innovation_host import pendulum_user
    lib = _lib.load()
    M, B, ld, T = 2, 3, 64, 2
    one = np.array([[1.0, 3.0]])
    ukf, gp = run_case(amd, 'ungm_ukf')['alg'], ssinf.GaussianProcessKalman(*nc.models('ungm_ukf'), one, one)
    ekf, trunc = ssinf.ExtendedKalman(*nc.models('ungm_ukf')), ssinf.TruncatedUnscentedKalman(*nc.models('pend_ckf'))
    gh = ssinf.GaussHermiteKalman(*nc.models('pend_ckf'), deg=3)
    UP, UM = pendulum_user()
    user = ssinf.UnscentedKalman(UP(sm.GaussRV(2), sm.GaussRV(2)), UM(sm.GaussRV(1), 2))
    sizes = (T * 4 * ld, T * 16 * ld, T * 8 * ld, T * ld, ld)
    outs = [_lib.DeviceBuffer(8 * n) for n in sizes] + [_lib.DeviceBuffer(4 * ld)]
    d_y = _lib.DeviceBuffer(8 * T * ld)
    d_y.upload(np.zeros(T * ld))
    for o in outs[:5]:
        o.upload(np.full(o.nbytes // 8, 7.0))
    outs[5].upload(np.full(ld, 7, dtype=np.int32))
    untouched = lambda: all((o.download((o.nbytes // 8,)) == 7.0).all() for o in outs[:5]) and (outs[5].download((ld,), dtype=np.int32) == 7).all()      # noqa: E731
    vp, dp = _lib.vp, _lib.dp

    def call(pair, D=1, Y=1, recursion=0, M=M, B=B, ld=ld, T=T, gqg=None, x0=None, strides=None, pi=None, mu0=None, name=True, null=()):
        gqg = np.ones((8, D * D)) if gqg is None else gqg
        rr = np.ones((8, Y * Y))
        x0 = np.ones((8, D + D * D)) if x0 is None else x0
        s = (D * D, Y * Y, D + D * D) if strides is None else strides
        pi = np.full((max(M, 1), max(M, 1)), 1.0 / max(M, 1)) if pi is None else pi
        mu0 = np.full(max(M, 1), 1.0 / max(M, 1)) if mu0 is None else mu0
        arg = lambda key, buf: vp(None if key in null else buf)      # noqa: E731
        rc = lib.ssmq_filter_imm_dev(*pair, recursion, B, ld, T, arg('y', d_y), M, dp(gqg), s[0], dp(rr), s[1], dp(x0), s[2],
                                     None if 'pi' in null else dp(pi), dp(mu0), arg('fm', outs[0]), vp(outs[1]), vp(outs[2]), vp(outs[3]),
                                     arg('total', outs[4]), arg('status', outs[5]))
        msg = _lib.last_error()
        if name:
            buf = ctypes.create_string_buffer(256)
            assert lib.ssmq_filter_imm_kernel_name(*pair, recursion, buf, 256) == rc, msg
        return rc, msg
    pu, pg = ukf._pair(), gp._pair()
    for kwargs, code, what in ((dict(pair=user._pair(), D=2), -3, 'user-defined models'),
                               (dict(pair=(pu[0], pu[1], pg[2], pg[3])), -3, 'different forms'),
                               (dict(pair=ekf._pair()), -3, 'linearisation and Taylor-GPQD'),
                               (dict(pair=trunc._pair(), D=2), -3, 'truncated'),
                               (dict(pair=pu, recursion=1), -3, 'Studentian recursion'),
                               (dict(pair=pu, recursion=2), -1, 'bad recursion'),
                               (dict(pair=gh._pair(), D=2), -3, 'no kernel for this pair'),
                               (dict(pair=pu, M=0, name=False), -1, '1 <= M <= 8'), (dict(pair=pu, M=9, name=False), -1, '1 <= M <= 8'),
                               (dict(pair=pu, ld=70, name=False), -1, 'multiple of 64'), (dict(pair=pu, B=65, name=False), -1, 'multiple of 64 and >= B'),
                               (dict(pair=pu, T=-1, name=False), -1, 'bad argument'),
                               (dict(pair=pu, strides=(2, 1, 2), name=False), -1, 'row stride of gqg'),
                               (dict(pair=pu, gqg=np.array([[1.0], [np.nan]]), name=False), -1, 'row 1 of gqg is not finite'),
                               (dict(pair=pu, x0=np.array([[0.0, 1.0], [0.0, np.inf]]), name=False), -1, 'row 1 of x0 is not finite'),
                               (dict(pair=pu, pi=np.array([[0.9, 0.1], [0.3, 0.6]]), name=False), -1, 'row 1 of pi does not sum to 1'),
                               (dict(pair=pu, pi=np.array([[1.5, -0.5], [0.3, 0.7]]), name=False), -1, 'row 0 of pi has an entry'),
                               (dict(pair=pu, mu0=np.array([0.5, np.nan]), name=False), -1, 'mu0 has an entry'),
                               (dict(pair=pu, mu0=np.array([0.5, 0.5 + 1e-11]), name=False), -1, 'mu0 does not sum to 1'),
                               (dict(pair=pu, null=('pi',), name=False), -1, 'bad argument'), (dict(pair=pu, null=('y',), name=False), -1, 'bad argument'),
                               (dict(pair=pu, null=('fm',), name=False), -1, 'bad argument'), (dict(pair=pu, null=('total',), name=False), -1, 'bad argument'),
                               (dict(pair=pu, null=('status',), name=False), -1, 'bad argument')):
        rc, msg = call(**kwargs)
        assert rc == code and what in msg and 'filter_imm' in msg and 'filter_noise_sweep:' not in msg and 'D <= 6, Y <= 4' in msg and untouched(), (kwargs, rc, msg)
    rc, msg = call(pair=pu, name=False)
    assert rc == 0, msg
    assert not untouched()
    for buf in outs + [d_y]:
        buf.free()
