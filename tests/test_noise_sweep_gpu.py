"""Noise sweeps by measurement likelihood on the device (k_noise_sweep<>): against the two-call path (one filter per row:
forward_pass_batch, then innovations_batch), against the CPU restatement (tests/_noise_sweep_oracle.py), bit-for-bit independence of
rows and trajectories, shared against stacked row arrays, failures that stay local, the refusals of the C entry points that read a
transform handle, and `fit_noise_covariances`.

Cases (tests/_noise_sweep_cases.py): ungm_ukf (sigma-point, D = Y = 1, N = 3, P = 5, B = 70, T = 6), pend_ckf (sigma-point, D = 2, Y = 1,
N = 4, R stack alone, P = 3, B = 5, T = 4), cv_gp (BQ, D = 4, Y = 2, N = 9, full Q rows and a P0 stack), ct_tp (t-process, D = 5, Y = 4,
N = 11, SELO = 1, Q scale rows); and UNGM on the five Gauss-Hermite points of degree 5 (N = 5 at D = 1, a table entry beyond 2 D + 1).

Bounds: the rule of tests/test_innovation_gpu.py, no new tolerance - a step's nis / loglik within max(RTOL, 64 cond(S) eps) max(1,
|value|) of the reference's, cond(S) from the oracle's S of that step; a total within the sum of its steps' bounds (the mean NIS: their
mean).  No case needs that file's MEASURED convention: on an MI355X the largest |error| / bound is 0.0101 (ct_tp, nis_mean against
the oracle; against the two-call path, which runs k_filter_wsplit and the OPT = 2 innovation kernel there, 0.0099), and every row of
ungm_ukf, pend_ckf and cv_gp has the bits of the two-call path, which runs the dense kernels for them."""
import ctypes

import numpy as np
import pytest

from tests import _noise_sweep_cases as nc
from tests import _noise_sweep_oracle as nso
from tests._cases import RTOL

pytestmark = pytest.mark.gpu
EPS = float(np.finfo(float).eps)
KEYS = ('loglik', 'loglik_total', 'nis_mean', 'status')


@pytest.fixture(scope='module')
def amd():
    import ssmtoybox_amd
    if ssmtoybox_amd.device_count() < 1:
        pytest.fail('no device: the GPU tests need an MI355X')
    ssmtoybox_amd.set_device(0)
    return ssmtoybox_amd


_RUNS = {}


def run_case(amd, name):
    """The case's sweep on the device, once, shared by the tests (never modified)."""
    if name not in _RUNS:
        c = nc.case(name)
        alg = nc.make_filter(name)
        _RUNS[name] = dict(alg=alg, out=alg.noise_sweep_batch(c['y'], c['q_cov'], c['r_cov'], c['x0_cov'], steps=True))
    return _RUNS[name]


def device_weights(alg):
    """The weights of the filter's two BQ transforms as the oracle takes them, or None for a sigma-point filter."""
    if not hasattr(alg.tf_dyn, 'model'):
        return None
    return tuple(dict(wm=tf.wm, Wc=tf.Wc, Wcc=tf.Wcc, model_var=tf.model.model_var, iK=tf.model.iK) for tf in (alg.tf_dyn, alg.tf_obs))


_DEV_REFS = {}


def device_weights_reference(amd, name):
    """The oracle's sweep of the case on the DEVICE's weights (the sigma-point rules have none to hand over), so that the comparison
    is about the recursion and not about the conditioning of the kernel matrix (tests/test_sweep_gpu.py).  Computed once."""
    if name not in _DEV_REFS:
        c, alg = nc.case(name), run_case(amd, name)['alg']
        w = device_weights(alg)
        if w is None:
            _DEV_REFS[name] = (nc.reference(name), None)
        else:
            if c['form'] == 'tp':
                assert alg.tf_dyn.model.nu == c['nu'] == alg.tf_obs.model.nu
            _DEV_REFS[name] = (nso.sweep(c, c['y'], c['q_rows'], c['r_rows'], c['x0_rows'], weights=w), w)
    return _DEV_REFS[name]


def step_bounds(amd, name, ref_nis, ref_ll):
    """(P, T, B) bounds of nis and loglik under the rule of tests/test_innovation_gpu.py."""
    S = nc.reference(name)['S']
    P, T, B = ref_ll.shape
    f = np.array([[[max(RTOL, 64.0 * np.linalg.cond(S[p][b][..., k]) * EPS) for b in range(B)] for k in range(T)] for p in range(P)])
    return f * np.maximum(1.0, np.abs(ref_nis)), f * np.maximum(1.0, np.abs(ref_ll))


def check_against(amd, name, out, ref, what):
    bn, bl = step_bounds(amd, name, ref['nis'], ref['loglik'])
    worst = {'loglik': np.max(np.abs(out['loglik'] - ref['loglik']) / bl),
             'loglik_total': np.max(np.abs(out['loglik_total'] - ref['loglik_total']) / bl.sum(axis=1)),
             'nis_mean': np.max(np.abs(out['nis_mean'] - ref['nis_mean']) / bn.mean(axis=1))}
    print('noise sweep {} {}: largest |error| / bound = {}'.format(name, what, {k: float('{:.3g}'.format(v)) for k, v in worst.items()}))
    assert np.array_equal(out['status'], ref['status']), what
    assert max(worst.values()) <= 1.0, (what, worst)


@pytest.mark.parametrize('name', nc.NAMES)
def test_row_is_the_two_call_path(amd, name):
    c, r = nc.case(name), run_case(amd, name)
    D, B, P = c['m0'].shape[0], c['B'], c['P']
    assert r['alg'].noise_sweep_kernel_name(P).startswith('k_noise_sweep<D={},Y={},'.format(D, c['R'].shape[0]))
    ref = dict(loglik=[], nis=[], loglik_total=[], nis_mean=[], status=[])
    dense, names = True, set()
    for p in range(P):
        alg = nc.make_filter(name, c['q_rows'][p], c['r_rows'][p], c['x0_rows'][p])
        row = (alg.kernel_name(B), alg.innovations_kernel_name(B))
        names.add(row)
        dense = dense and row[0].startswith('k_filter_fused<') and row[1].startswith('k_innovation<') and all(n.endswith('OPT=0>') for n in row)
        fm, fP = alg.forward_pass_batch(c['y'], raise_on_failure=False)
        inn = alg.innovations_batch(c['y'], fi_mean=fm, fi_cov=fP)
        for key in ref:
            ref[key].append(inn[key])
    ref = {k: np.stack(v) for k, v in ref.items()}
    equal = [bool(np.array_equal(r['out']['loglik'][p], ref['loglik'][p])) for p in range(P)]
    print('noise sweep {}: the two-call path ran {} ({}); rows bit-equal to it: {}'.format(name, sorted(names), 'dense' if dense else 'not the dense kernels', equal))
    check_against(amd, name, r['out'], ref, 'against the two-call path')
    if name in ('ungm_ukf', 'pend_ckf') and dense:
        for key in KEYS:
            assert np.array_equal(r['out'][key], ref[key]), key


@pytest.mark.parametrize('kind', ('ghkf', 'gpqkf'))
def test_five_points_at_one_state_are_in_the_table(amd, kind):
    """UNGM with the five Gauss-Hermite points of degree 5 (N = 5 > 2 D + 1: a table entry of its own): every row has the bits of the
    two-call path where that runs the dense kernels, and is within the bound of it otherwise."""
    from ssmtoybox_amd import ssinf, ssmod as sm
    c = nc.case('ungm_ukf')
    par = np.array([[1.0, 3.0]])

    def make(q=None, r=None):
        dyn, obs = nc.models('ungm_ukf')
        if q is not None:
            dyn.noise_rv, obs.noise_rv = sm.GaussRV(1, cov=q), sm.GaussRV(1, cov=r)
        return ssinf.GaussHermiteKalman(dyn, obs, deg=5) if kind == 'ghkf' else ssinf.GaussianProcessKalman(dyn, obs, par, par, 'rbf', 'gh', {'degree': 5})
    alg = make()
    assert alg.tf_dyn._num_points() == 5 and alg.noise_sweep_kernel_name(c['P']).startswith('k_noise_sweep<D=1,Y=1,ND=5,NO=5,')
    out = alg.noise_sweep_batch(c['y'], c['q_cov'], c['r_cov'], steps=True)
    ref = dict(loglik=[], nis=[], loglik_total=[], nis_mean=[], status=[])
    dense = True
    for p in range(c['P']):
        row = make(c['q_rows'][p], c['r_rows'][p])
        names = (row.kernel_name(c['B']), row.innovations_kernel_name(c['B']))
        dense = dense and names[0].startswith('k_filter_fused<') and names[1].startswith('k_innovation<') and all(n.endswith('OPT=0>') for n in names)
        fm, fP = row.forward_pass_batch(c['y'], raise_on_failure=False)
        inn = row.innovations_batch(c['y'], fi_mean=fm, fi_cov=fP)
        for key in ref:
            ref[key].append(inn[key])
    ref = {k: np.stack(v) for k, v in ref.items()}
    print('noise sweep five points {}: two-call path {} ({}); rows bit-equal: {}'.format(
        kind, names, 'dense' if dense else 'not the dense kernels', [bool(np.array_equal(out['loglik'][p], ref['loglik'][p])) for p in range(c['P'])]))
    assert not out['status'].any() and np.isfinite(out['loglik']).all()
    check_against(amd, 'ungm_ukf', out, ref, 'five points, against the two-call path')
    if dense:
        for key in KEYS:
            assert np.array_equal(out[key], ref[key]), key


def test_a_point_count_without_a_table_entry_is_refused_by_the_library(amd):
    from ssmtoybox_amd import ssinf
    alg = ssinf.GaussHermiteKalman(*nc.models('pend_ckf'), deg=3)      # nine points at D = 2
    c = nc.case('pend_ckf')
    for call in (lambda: alg.noise_sweep_kernel_name(3), lambda: alg.noise_sweep_batch(c['y'], r_cov=c['r_cov']),
                 lambda: alg.fit_noise_covariances(c['y'], r_cov=c['r_cov'])):
        with pytest.raises(NotImplementedError, match='no kernel for this pair of models and point sets') as info:
            call()
        assert 'D <= 6, Y <= 4' in str(info.value)


@pytest.mark.parametrize('name', nc.NAMES)
def test_against_the_oracle(amd, name):
    ref, _ = device_weights_reference(amd, name)
    assert not ref['status'].any()
    check_against(amd, name, run_case(amd, name)['out'], ref, 'against the oracle')


def test_rows_and_trajectories_are_independent_bit_for_bit(amd):
    c, r = nc.case('ungm_ukf'), run_case(amd, 'ungm_ukf')
    alg, out, q, rc, y = r['alg'], r['out'], c['q_cov'], c['r_cov'], c['y']
    for p in range(c['P']):
        one = alg.noise_sweep_batch(y, q[p:p + 1], rc[p:p + 1], steps=True)
        for key in KEYS:
            assert np.array_equal(one[key][0], out[key][p]), (key, p)
    perm = np.array([3, 0, 4, 2, 1])
    shuffled = alg.noise_sweep_batch(y, q[perm], rc[perm], steps=True)
    for key in KEYS:
        assert np.array_equal(shuffled[key], out[key][perm]), key
    alone = alg.noise_sweep_batch(y[..., 67:68], q, rc, steps=True)
    for key in KEYS:
        assert np.array_equal(alone[key][..., 0], out[key][..., 67]), key
    again = alg.noise_sweep_batch(y, q, rc, steps=True)
    for key in KEYS:
        assert np.array_equal(again[key], out[key]), key
    bare = alg.noise_sweep_batch(y, q, rc)
    assert set(bare) == {'loglik_total', 'nis_mean', 'status'}
    for key in bare:
        assert np.array_equal(bare[key], out[key]), key
    # the device route: the same bits
    from ssmtoybox_amd import _lib
    (Y, T, B), ld, P = y.shape, 128, c['P']
    d_y = _lib.DeviceBuffer(8 * T * Y * ld)
    _lib.upload_study(y, Y, ld, d_y)
    d_tot, d_nis, d_ll, d_st = alg.noise_sweep_dev(d_y, B, ld, T, q, rc, steps=True)
    assert np.array_equal(d_tot.download((P, ld))[:, :B], out['loglik_total']) and np.array_equal(d_nis.download((P, ld))[:, :B], out['nis_mean'])
    assert np.array_equal(d_ll.download((P, T, ld))[:, :, :B], out['loglik'])
    assert np.array_equal(d_st.download((P, ld), dtype=np.int32)[:, :B], out['status'])
    lean = alg.noise_sweep_dev(d_y, B, ld, T, q, rc)
    assert lean[2] is None and np.array_equal(lean[0].download((P, ld))[:, :B], out['loglik_total'])
    for buf in (d_y, d_tot, d_nis, d_ll, d_st, lean[0], lean[1], lean[3]):
        buf.free()


@pytest.mark.parametrize('name', ('ungm_ukf', 'pend_ckf', 'cv_gp'))
def test_shared_is_stacked(amd, name):
    """An argument left to the model (row stride 0) against the same matrix as a stack of identical rows (row stride = row size)."""
    c, r = nc.case(name), run_case(amd, name)
    args = dict(q_cov=c['q_cov'], r_cov=c['r_cov'], x0_cov=c['x0_cov'])
    for key, rows in (('q_cov', c['q_rows']), ('r_cov', c['r_rows']), ('x0_cov', c['x0_rows'])):
        if args[key] is None:
            stacked = r['alg'].noise_sweep_batch(c['y'], steps=True, **dict(args, **{key: np.ascontiguousarray(rows)}))
            one = r['alg'].noise_sweep_batch(c['y'], steps=True, **dict(args, **{key: rows[0]}))
            for k in KEYS:
                assert np.array_equal(stacked[k], r['out'][k]) and np.array_equal(one[k], r['out'][k]), (key, k)


def test_failures_stay_local(amd):
    c, r = nc.case('ungm_ukf'), run_case(amd, 'ungm_ukf')
    alg, out = r['alg'], r['out']
    P, B, T = c['P'], c['B'], c['T']
    # a Q row with a negative variance: the oracle's status pattern (tests/test_noise_sweep_host.py), every other row untouched
    q = nc.failing_q(c)
    want = nso.sweep(c, c['y'], q[nc.FAIL_ROW:nc.FAIL_ROW + 1], c['r_rows'][nc.FAIL_ROW:nc.FAIL_ROW + 1], c['x0_rows'][:1])
    got = alg.noise_sweep_batch(c['y'], q, c['r_cov'], steps=True)
    st = got['status'][nc.FAIL_ROW]
    assert np.array_equal(st, want['status'][0]) and np.count_nonzero(st) == B - 1
    bad = st != 0
    assert np.isnan(got['loglik_total'][nc.FAIL_ROW, bad]).all() and np.isnan(got['nis_mean'][nc.FAIL_ROW, bad]).all()
    assert np.isfinite(got['loglik_total'][nc.FAIL_ROW, ~bad]).all()
    for b in np.flatnonzero(bad):
        assert np.isnan(got['loglik'][nc.FAIL_ROW, st[b] - 1:, b]).all() and np.isfinite(got['loglik'][nc.FAIL_ROW, :st[b] - 1, b]).all()
    keep = np.arange(P) != nc.FAIL_ROW
    for key in KEYS:
        assert np.array_equal(got[key][keep], out[key][keep]), key
    # a NaN in one measurement of one trajectory
    step, lane = 2, 5
    y = c['y'].copy()
    y[0, step, lane] = np.nan
    got = alg.noise_sweep_batch(y, c['q_cov'], c['r_cov'], steps=True)
    keep = np.arange(B) != lane
    assert (got['status'][:, lane] == 1 + step).all() and not got['status'][:, keep].any()
    assert np.isnan(got['loglik_total'][:, lane]).all() and np.isnan(got['nis_mean'][:, lane]).all()
    assert np.isnan(got['loglik'][:, step:, lane]).all() and np.array_equal(got['loglik'][:, :step, lane], out['loglik'][:, :step, lane])
    for key in ('loglik', 'loglik_total', 'nis_mean'):
        assert np.array_equal(got[key][..., keep], out[key][..., keep]), key


def test_fit_noise_covariances_is_the_oracle_argmax(amd):
    c, r = nc.case('ungm_ukf'), run_case(amd, 'ungm_ukf')
    index, q, rr, table = r['alg'].fit_noise_covariances(c['y'], c['q_cov'], c['r_cov'])
    ref = nc.reference('ungm_ukf')
    want = ref['loglik_total'].sum(axis=1)
    _, bl = step_bounds(amd, 'ungm_ukf', ref['nis'], ref['loglik'])
    print('noise likelihood table: device {}, oracle {}, largest |error| / bound {:.3g}'.format(table, want, np.max(np.abs(table - want) / bl.sum(axis=(1, 2)))))
    assert index == int(np.argmax(want)) == 2            # scale 1: an interior point of the grid
    assert np.array_equal(q, c['q_cov'][index]) and np.array_equal(rr, c['r_cov'][index])
    assert np.all(np.abs(table - want) <= bl.sum(axis=(1, 2)))


@pytest.mark.parametrize('name', ('pend_ckf', 'cv_gp'))
def test_the_object_is_unchanged(amd, name):
    c = nc.case(name)
    alg = nc.make_filter(name)
    alg.forward_pass_batch(c['y'])
    state = lambda: (alg.tf_dyn.wm, alg.tf_dyn.Wc, alg.tf_obs.wm, alg.tf_obs.Wc, alg.fi_mean, alg.fi_cov, alg.status, alg.q_cov, alg.r_cov, alg.x0_cov)      # noqa: E731
    before = [np.array(a, copy=True) for a in state()]
    alg.noise_sweep_batch(c['y'], c['q_cov'], c['r_cov'], c['x0_cov'])
    alg.fit_noise_covariances(c['y'], c['q_cov'], c['r_cov'], c['x0_cov'])
    for a, b in zip(before, state()):
        assert np.array_equal(a, b)
    fm, _ = alg.forward_pass_batch(c['y'])
    assert np.array_equal(fm, before[4])


def test_c_abi_refusals_leave_the_outputs_untouched(amd):
    """The refusals that read a transform handle, from both entry points: code, the range in the message, outputs untouched."""
    from ssmtoybox_amd import _lib, ssinf, ssmod as sm
    from tests.test_innovation_host import pendulum_user
    lib = _lib.load()
    P, B, ld, T = 2, 3, 64, 2
    ukf, gp = run_case(amd, 'ungm_ukf')['alg'], ssinf.GaussianProcessKalman(*nc.models('ungm_ukf'), np.array([[1.0, 3.0]]), np.array([[1.0, 3.0]]))
    ekf = ssinf.ExtendedKalman(*nc.models('ungm_ukf'))
    one = np.array([[1.0, 3.0]])
    tgpqd = ssinf.ExtendedKalmanGPQD(*nc.models('ungm_ukf'), one, one)
    gpqd = ssinf.GaussianProcessDerKalman(*nc.models('ungm_ukf'), one, one)
    mo = ssinf.MultiOutputGaussianProcessKalman(*nc.models('ungm_ukf'), one, one)
    trunc = ssinf.TruncatedUnscentedKalman(*nc.models('pend_ckf'))
    gh = ssinf.GaussHermiteKalman(*nc.models('pend_ckf'), deg=3)
    UP, UM = pendulum_user()
    user = ssinf.UnscentedKalman(UP(sm.GaussRV(2), sm.GaussRV(2)), UM(sm.GaussRV(1), 2))
    outs = [_lib.DeviceBuffer(8 * P * ld), _lib.DeviceBuffer(8 * P * ld), _lib.DeviceBuffer(8 * P * T * ld), _lib.DeviceBuffer(4 * P * ld)]
    d_y = _lib.DeviceBuffer(8 * T * ld)
    d_y.upload(np.zeros(T * ld))
    for o in outs[:3]:
        o.upload(np.full(o.nbytes // 8, 7.0))
    outs[3].upload(np.full(P * ld, 7, dtype=np.int32))
    untouched = lambda: all((o.download((o.nbytes // 8,)) == 7.0).all() for o in outs[:3]) and (outs[3].download((P * ld,), dtype=np.int32) == 7).all()      # noqa: E731
    vp, dp = _lib.vp, _lib.dp

    def call(pair, D=1, Y=1, recursion=0, P=P, B=B, ld=ld, T=T, gqg=None, rr=None, x0=None, strides=None, name=True, null=()):
        """null: names of pointer arguments passed as NULL ('y', 'x0', 'total', 'nis', 'status')."""
        gqg = np.ones((2, D * D)) if gqg is None else gqg
        rr = np.ones((2, Y * Y)) if rr is None else rr
        x0 = np.ones((2, D + D * D)) if x0 is None else x0
        s = (D * D, Y * Y, D + D * D) if strides is None else strides
        arg = lambda key, buf: vp(None if key in null else buf)      # noqa: E731
        rc = lib.ssmq_filter_noise_sweep_dev(*pair, recursion, B, ld, T, arg('y', d_y), P, dp(gqg), s[0], dp(rr), s[1],
                                             None if 'x0' in null else dp(x0), s[2], arg('total', outs[0]), arg('nis', outs[1]), vp(outs[2]),
                                             arg('status', outs[3]))
        msg = _lib.last_error()
        if name:
            buf = ctypes.create_string_buffer(256)
            assert lib.ssmq_filter_noise_sweep_kernel_name(*pair, recursion, buf, 256) == rc, msg
        return rc, msg
    pu, pg = ukf._pair(), gp._pair()
    for kwargs, code, what in ((dict(pair=user._pair(), D=2), -3, 'user-defined models'),
                               (dict(pair=(pu[0], pu[1], pg[2], pg[3])), -3, 'different forms'),
                               (dict(pair=ekf._pair()), -3, 'linearisation and Taylor-GPQD'),
                               (dict(pair=tgpqd._pair()), -3, 'linearisation and Taylor-GPQD'),
                               (dict(pair=gpqd._pair()), -3, 'GPQ+D transforms'),
                               (dict(pair=mo._pair()), -3, 'multi-output'),
                               (dict(pair=trunc._pair(), D=2), -3, 'truncated'),
                               (dict(pair=pu, recursion=1), -3, 'Studentian recursion'),
                               (dict(pair=pu, recursion=2), -1, 'bad recursion'),
                               (dict(pair=gh._pair(), D=2), -3, 'no kernel for this pair'),
                               (dict(pair=pu, P=0, name=False), -1, 'P >= 1'), (dict(pair=pu, ld=70, name=False), -1, 'multiple of 64'),
                               (dict(pair=pu, B=65, name=False), -1, 'ld a multiple of 64 and >= B'), (dict(pair=pu, T=-1, name=False), -1, 'bad argument'),
                               (dict(pair=pu, strides=(2, 1, 2), name=False), -1, 'row stride of gqg'),
                               (dict(pair=pu, strides=(1, 1, 3), name=False), -1, 'row stride of x0'),
                               (dict(pair=pu, strides=(1, 2, 2), name=False), -1, 'row stride of rr'),
                               (dict(pair=pu, gqg=np.array([[1.0], [np.nan]]), name=False), -1, 'row 1 of gqg is not finite'),
                               (dict(pair=pu, rr=np.array([[np.inf], [1.0]]), name=False), -1, 'row 0 of rr is not finite'),
                               (dict(pair=pu, x0=np.array([[0.0, 1.0], [0.0, np.nan]]), name=False), -1, 'row 1 of x0 is not finite'),
                               (dict(pair=pu, null=('x0',), name=False), -1, 'x0 is null'), (dict(pair=pu, null=('y',), name=False), -1, 'bad argument'),
                               (dict(pair=pu, null=('total',), name=False), -1, 'bad argument'), (dict(pair=pu, null=('nis',), name=False), -1, 'bad argument'),
                               (dict(pair=pu, null=('status',), name=False), -1, 'bad argument')):
        rc, msg = call(**kwargs)
        assert rc == code and what in msg and 'D <= 6, Y <= 4' in msg and untouched(), (kwargs, rc, msg)
    # a shared non-finite second row is never read (stride 0: one row)
    rc, msg = call(pair=pu, gqg=np.array([[1.0], [np.nan]]), strides=(0, 1, 2), name=False)
    assert rc == 0, msg
    assert not untouched()
    for buf in outs + [d_y]:
        buf.free()
