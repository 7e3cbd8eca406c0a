"""The masked pass on the device against its NumPy restatement (tests/_masked_oracle.py, which compresses to the observed rows):
k_masked_loop<> for the table shapes (Y = 1, 2 and 4) and a user pair, the launch loop (apply dyn | apply obs | k_masked_update) for the
other forms, k_masked_update<0, 0> for a (4, 4) pair.  B = 70 (one full block of 64 lanes and a partial one); T = 6 with the pattern mask
mask[k][b] = (b + k) mod 2^Y (every pattern at every step, o = 0 at k = 0 and at k = T - 1 for some trajectories), T = 8 with a random
mask at p = 0.6.

Bound.  Every step is compared with the one-step restatement started from the DEVICE's filtered moments of the step before, by
assert_moments_close with rtol = max(RTOL, 64 eps (cond P- + cond S_oo)): the project's bound for one application of an inverse
(tests/test_gpu_parity.py, tests/test_robust_gpu.py), the condition numbers from the restatement.  nis and loglik are held to rtol x
their own error scales (tests/_masked_oracle.py: update).  `used` must match exactly.  No case needed more than this bound (MEASURED is
empty)."""
import ctypes

import numpy as np
import pytest

from tests import _innovation_oracle as ino
from tests import _masked_oracle as mko
from tests._cases import RTOL, assert_moments_close, moment_scales
from tests.test_innovation_gpu import simulate
from tests.test_iterated_gpu import case_tf, make_case as iterated_case

pytestmark = pytest.mark.gpu
EPS = float(np.finfo(float).eps)
B = 70
T_OF = {'pattern': 6, 'random': 8, 'full': 6}

ONE_LAUNCH = ('ungm_ukf', 'pend_gpqkf', 'pend_tpqkf', 'cv_radar', 'ct_bearing', 'user_pend')
LOOP = ('pend_ghkf', 'cv_bearing4')      # cv_bearing4: D = 4, Y = 4 - no register instantiation, k_masked_update<0, 0>
MEASURED = ()                            # cases whose bound is 4 x the float64 restatement's own error (none)
_DATA, _RUNS, _REFS = {}, {}, {}
ONE = np.zeros((1, 1))


@pytest.fixture(scope='module')
def amd():
    import ssmtoybox_amd
    if ssmtoybox_amd.device_count() < 1:
        pytest.fail('no device: the GPU tests need an MI355X')
    ssmtoybox_amd.set_device(0)
    return ssmtoybox_amd


def make_case(name):
    if name != 'cv_bearing4':
        return iterated_case(name)
    from ssmtoybox_amd import ssinf, ssmod as sm
    dyn = sm.ConstantVelocity(sm.GaussRV(4, np.array([100.0, 5.0, 200.0, -3.0]), np.diag([1.0, 0.1, 1.0, 0.1])), sm.GaussRV(2, cov=0.1 * np.eye(2)))
    sensors = np.vstack((1000 * np.eye(2), -1000 * np.eye(2))).astype(float)
    return ssinf.UnscentedKalman(dyn, sm.BearingMeasurement(sm.GaussRV(4, cov=1e-4 * np.eye(4)), 4, state_index=[0, 2], sensor_pos=sensors))


def case_data(name, kind):
    """(filter, the built-in twin the restatement evaluates, measurements (Y, T, B), mask (T, B) uint32): made once, never modified."""
    if (name, kind) not in _DATA:
        alg = make_case(name)
        twin = make_case('pend_ukf') if name == 'user_pend' else alg
        T, Y = T_OF[kind], alg.mod_obs.dim_out
        y = simulate(twin, B, T, 3)
        if kind == 'pattern':
            mask = (np.arange(B)[None, :] + np.arange(T)[:, None]) % (1 << Y)
        elif kind == 'random':
            mask = (np.random.default_rng(60).random((Y, T, B)) < 0.6).astype(np.int64)
            mask = (mask << np.arange(Y)[:, None, None]).sum(axis=0)
        else:
            mask = np.full((T, B), (1 << Y) - 1)
        mask = mask.astype(np.uint32)
        y.setflags(write=False)
        mask.setflags(write=False)
        _DATA[(name, kind)] = (alg, twin, y, mask)
    return _DATA[(name, kind)]


def as_run(alg, out):
    return dict(fm=out['fm'], fP=out['fP'], used=out['used'], nis=out['nis'], ll=out['loglik'], status=alg.status.copy(),
                n_used=out['n_used'], ll_total=out['loglik_total'])


def run_case(name, kind, **kw):
    """The case on the device.  Shared by the tests, never modified."""
    key = (name, kind) + tuple(sorted((k, repr(v)) for k, v in kw.items()))
    if key not in _RUNS:
        alg, _, y, mask = case_data(name, kind)
        _RUNS[key] = as_run(alg, alg.masked_pass_batch(y, mask=mask, raise_on_failure=False, return_scores=True, **kw))
    return _RUNS[key]


def oracle_pair(alg, twin):
    return case_tf(alg.tf_dyn, twin.mod_dyn.dyn_eval), case_tf(alg.tf_obs, twin.mod_obs.meas_eval), alg.G.dot(alg.q_cov).dot(alg.G.T)


def restated(alg, twin, y, mask, run, gate=None):
    """The one-step restatement of every (k, b) from the device's moments of step k - 1: list over b of lists over k."""
    key = (id(run), id(y), id(mask))
    if key not in _REFS:
        tfd, tfo, GQG = oracle_pair(alg, twin)
        out = []
        for b in range(y.shape[2]):
            rows = []
            for k in range(y.shape[1]):
                m, P = (alg.x0_mean, alg.x0_cov) if k == 0 else (run['fm'][:, k - 1, b], run['fP'][..., k - 1, b])
                r = mko.step(m, P, y[:, k, b], mask[k, b], k, GQG, alg.r_cov, tfd, tfo, gate)
                r['P_in'] = P
                rows.append(r)
            out.append(rows)
        _REFS[key] = (out, run, y, mask)       # (the arrays are kept: their ids stay theirs)
    return _REFS[key][0]


def word_of(used, k, b):
    return int(sum(int(used[i, k, b]) << i for i in range(used.shape[0])))


def check_against(run, rows, what):
    """Every (k, b) of `run` against the restatement rows; prints the largest error / bound.  No case is left out."""
    worst = np.zeros(4)
    for b, rs in enumerate(rows):
        for k, r in enumerate(rs):
            assert r['conds'] is not None, (what, b, k)
            rtol = max(RTOL, 64.0 * EPS * sum(r['conds']))
            gm, gP = run['fm'][:, k, b], run['fP'][..., k, b]
            assert word_of(run['used'], k, b) == r['used'], (what, b, k)
            assert_moments_close((gm, gP, ONE), (r['m'], r['P'], ONE), r['P_in'], rtol, (what, b, k))
            ms, cs, _ = moment_scales(r['m'], r['P'], ONE, r['P_in'])
            ns, ls = r['scales']
            if ns == 0.0:      # nothing offered
                assert run['nis'][k, b] == 0.0 and run['ll'][k, b] == 0.0 and np.signbit(run['ll'][k, b]) == 0, (what, b, k)
                en = el = 0.0
            else:
                en, el = abs(run['nis'][k, b] - r['nis']) / (rtol * ns), abs(run['ll'][k, b] - r['ll']) / (rtol * ls)
            worst = np.maximum(worst, [float(np.max(np.abs(gm - r['m']))) / ms / rtol, float(np.max(np.abs(gP - r['P']))) / cs / rtol, en, el])
    print('masked pass {}: largest error / bound: mean {:.3g}, cov {:.3g}, nis {:.3g}, loglik {:.3g}'.format(what, *worst))
    assert np.all(worst <= 1.0), (what, worst)


def same_bits(a, b, keys=('fm', 'fP', 'used', 'nis', 'll', 'status')):
    for key in keys:
        assert np.array_equal(a[key], b[key], equal_nan=True), key
        if a[key].dtype == np.float64:
            assert np.array_equal(np.signbit(a[key]), np.signbit(b[key])), key


@pytest.mark.parametrize('kind', ['pattern', 'random'])
@pytest.mark.parametrize('name', ONE_LAUNCH + LOOP)
def test_1_every_step_against_the_restatement(amd, name, kind):
    alg, twin, y, mask = case_data(name, kind)
    kn = alg.masked_kernel_name()
    assert kn.startswith('k_masked_loop<') if name in ONE_LAUNCH else kn.startswith('launch loop'), kn
    assert ('run-time compiled' in kn) == (name == 'user_pend')
    run = run_case(name, kind)
    assert run['status'].dtype == np.int32 and not run['status'].any()
    assert run['used'].dtype == np.bool_ and run['used'].shape == y.shape
    for b in range(B):     # both triangles are written from one value
        assert np.array_equal(run['fP'][..., b], run['fP'][..., b].transpose(1, 0, 2))
    Y = y.shape[0]
    if kind == 'pattern':
        assert all(np.any(mask[k] == w) for k in range(mask.shape[0]) for w in range(1 << Y))
    check_against(run, restated(alg, twin, y, mask, run), '{} ({} mask)'.format(name, kind))
    assert np.array_equal(run['n_used'], run['used'].sum(axis=(0, 1))) and np.array_equal(run['ll_total'], run['ll'].sum(axis=0))


@pytest.mark.parametrize('name', ONE_LAUNCH + LOOP)
def test_2_a_fully_masked_step_returns_the_prior_bit_for_bit(amd, name):
    """Two runs that differ only in y where nothing is observed have the same bits; such a step has nis = loglik = 0, used = 0, its
    covariance is the time update's (no update term: P = P- exactly), checked against the restatement's prior in test 1."""
    alg, twin, y, mask = case_data(name, 'pattern')
    run = run_case(name, 'pattern')
    none = mask == 0
    assert none[0].any() and none[-1].any()
    y2 = y.copy()
    y2[:, none] += 5.0
    other = as_run(alg, alg.masked_pass_batch(y2, mask=mask, raise_on_failure=False, return_scores=True))
    same_bits(run, other)
    assert np.all(run['nis'][none] == 0.0) and np.all(run['ll'][none] == 0.0) and not run['used'][:, none].any()
    rows = restated(alg, twin, y, mask, run)
    for k, b in zip(*np.nonzero(none)):     # the restatement's update is the identity there: the device's bits against its prior
        r = rows[b][k]
        rtol = max(RTOL, 64.0 * EPS * r['conds'][0])
        assert_moments_close((run['fm'][:, k, b], run['fP'][..., k, b], ONE), (r['m_pr'], r['P_pr'], ONE), r['P_in'], rtol, (name, b, k))


@pytest.mark.parametrize('name', ['ungm_ukf', 'cv_radar', 'ct_bearing', 'pend_ghkf', 'cv_bearing4'])
def test_3_values_under_cleared_bits_are_never_read(amd, name):
    alg, _, y, mask = case_data(name, 'pattern')
    Y = y.shape[0]
    clear = np.array([[(mask >> i) & 1 == 0] for i in range(Y)]).reshape(Y, *mask.shape)
    runs = []
    for fill in (0.0, np.nan, np.inf, 1e300):
        yf = np.where(clear, fill, y)
        runs.append(as_run(alg, alg.masked_pass_batch(yf, mask=mask, raise_on_failure=False, return_scores=True)))
        assert not runs[-1]['status'].any()
        same_bits(runs[0], runs[-1])
    same_bits(run_case(name, 'pattern'), runs[0])
    inferred = as_run(alg, alg.masked_pass_batch(np.where(clear, np.nan, y), mask=None, raise_on_failure=False, return_scores=True))
    same_bits(runs[0], inferred)
    # bits at or above Y are ignored (the C ABI; the Python wrapper drops them)
    wide = as_run(alg, alg.masked_pass_batch(y, mask=(mask | np.uint32(1 << 16)), raise_on_failure=False, return_scores=True))
    same_bits(runs[0], wide)


@pytest.mark.parametrize('name', ['ungm_ukf', 'pend_gpqkf', 'cv_radar', 'ct_bearing', 'pend_ghkf'])
def test_4_full_mask_without_gate_is_the_forward_pass_and_its_innovation_scores(amd, name):
    """Step by step from the masked run's own moments (a pass of one step uses time index 0: every step of a model without time
    dependence, step 0 alone of UNGM), under the bound of test 1."""
    alg, twin, y, mask = case_data(name, 'full')
    run = run_case(name, 'full')
    assert not run['status'].any() and run['used'].all()
    rows = restated(alg, twin, y, mask, run)
    check_against(run, rows, name + ' (full mask)')
    D, worst = run['fm'].shape[0], 0.0
    for k in range(1 if name.startswith('ungm') else y.shape[1]):
        m0 = np.broadcast_to(alg.x0_mean, (B, D)) if k == 0 else run['fm'][:, k - 1, :].T
        P0 = np.broadcast_to(alg.x0_cov, (B, D, D)) if k == 0 else run['fP'][..., k - 1, :].transpose(2, 0, 1)
        m0, P0 = np.ascontiguousarray(m0), np.ascontiguousarray(P0)
        fm, fP = alg.forward_pass_batch(y[:, k:k + 1, :], x0_mean=m0, x0_cov=P0, raise_on_failure=False)
        assert not alg.status.any()
        sc = alg.innovations_batch(y[:, k:k + 1, :], x0_mean=m0, x0_cov=P0, fi_mean=fm, fi_cov=fP)
        for b in range(B):
            r = rows[b][k]
            rtol = max(RTOL, 64.0 * EPS * sum(r['conds']))
            ms, cs, _ = moment_scales(r['m'], r['P'], ONE, r['P_in'])
            ns, ls = r['scales']
            worst = max(worst, float(np.max(np.abs(run['fm'][:, k, b] - fm[:, 0, b]))) / ms / rtol,
                        float(np.max(np.abs(run['fP'][..., k, b] - ino.lower_sym(fP[..., 0, b])))) / cs / rtol,
                        abs(run['nis'][k, b] - sc['nis'][0, b]) / (rtol * ns), abs(run['ll'][k, b] - sc['loglik'][0, b]) / (rtol * ls))
    print('full mask against forward_pass_batch / innovations_batch {}: largest error / bound = {:.3g}'.format(name, worst))
    assert worst <= 1.0, (name, worst)


@pytest.mark.parametrize('name', mko.GATE_CASES)
def test_5_gate(amd, name):
    same_bits(run_case(name, 'pattern', gate=np.inf), run_case(name, 'pattern'))
    alg, y, mask, gate = mko.gate_case(name)
    Y = y.shape[0]
    run = as_run(alg, alg.masked_pass_batch(y, mask=mask, gate=gate[1:], raise_on_failure=False, return_scores=True))
    assert not run['status'].any()
    rows = restated(alg, alg, y, mask, run, gate)
    check_against(run, rows, name + ' (gate)')          # `used` against the restatement's decisions, exactly
    words = np.array([[word_of(run['used'], k, b) for b in range(B)] for k in range(y.shape[1])], dtype=np.uint32)
    rejected = (mask != 0) & (words == 0)
    accepted = (mask != 0) & (words != 0)
    assert rejected.sum() >= B // 5 and accepted.any() and np.array_equal(words[accepted], mask[accepted])
    o = np.array([[bin(int(w)).count('1') for w in row] for row in mask])
    assert np.all(run['nis'][rejected] > gate[o[rejected]]) and np.all(np.isfinite(run['nis'][rejected])) and np.all(np.isfinite(run['ll'][rejected]))
    assert np.all(run['nis'][accepted] <= gate[o[accepted]])
    # a rejected step returns the prior bit for bit: the run whose mask is cleared at the rejected steps has the same moments
    cleared = as_run(alg, alg.masked_pass_batch(y, mask=np.where(rejected, 0, mask).astype(np.uint32), gate=gate[1:], raise_on_failure=False,
                                                return_scores=True))
    same_bits(run, cleared, keys=('fm', 'fP', 'used', 'status'))
    assert np.all(cleared['nis'][rejected] == 0.0) and np.array_equal(cleared['nis'][~rejected], run['nis'][~rejected])
    # a scalar gate is the same threshold for every o
    s = as_run(alg, alg.masked_pass_batch(y, mask=mask, gate=float(gate[1]), raise_on_failure=False, return_scores=True))
    t = as_run(alg, alg.masked_pass_batch(y, mask=mask, gate=[gate[1]] * Y, raise_on_failure=False, return_scores=True))
    same_bits(s, t)


@pytest.mark.parametrize('name', ['ungm_ukf', 'pend_gpqkf', 'cv_radar', 'ct_bearing'])
def test_6_launch_loop_flag_agrees_with_the_one_launch_kernel(amd, name):
    alg, twin, y, mask = case_data(name, 'pattern')
    assert alg.masked_kernel_name().startswith('k_masked_loop<') and alg.masked_kernel_name(launch_loop=True).startswith('launch loop')
    loop = run_case(name, 'pattern', launch_loop=True)
    assert not loop['status'].any()
    check_against(loop, restated(alg, twin, y, mask, loop), name + ' (launch loop)')
    # ... and the two routes against each other, step by step from the one-launch kernel's moments
    run = run_case(name, 'pattern')
    rows = restated(alg, twin, y, mask, run)
    D, worst = run['fm'].shape[0], 0.0
    for k in range(1 if name.startswith('ungm') else y.shape[1]):
        m0 = np.broadcast_to(alg.x0_mean, (B, D)) if k == 0 else run['fm'][:, k - 1, :].T
        P0 = np.broadcast_to(alg.x0_cov, (B, D, D)) if k == 0 else run['fP'][..., k - 1, :].transpose(2, 0, 1)
        out = alg.masked_pass_batch(y[:, k:k + 1, :], mask=mask[k:k + 1], x0_mean=np.ascontiguousarray(m0), x0_cov=np.ascontiguousarray(P0),
                                    raise_on_failure=False, return_scores=True, launch_loop=True)
        assert not alg.status.any() and np.array_equal(out['used'][:, 0], run['used'][:, k])
        for b in range(B):
            r = rows[b][k]
            rtol = max(RTOL, 64.0 * EPS * sum(r['conds']))
            ms, cs, _ = moment_scales(r['m'], r['P'], ONE, r['P_in'])
            ns, ls = r['scales']
            worst = max(worst, float(np.max(np.abs(run['fm'][:, k, b] - out['fm'][:, 0, b]))) / ms / rtol,
                        float(np.max(np.abs(run['fP'][..., k, b] - out['fP'][..., 0, b]))) / cs / rtol,
                        abs(run['nis'][k, b] - out['nis'][0, b]) / (rtol * ns) if ns else 0.0,
                        abs(run['ll'][k, b] - out['loglik'][0, b]) / (rtol * ls) if ls else 0.0)
    print('one launch against the launch loop {}: largest error / bound = {:.3g}'.format(name, worst))
    assert worst <= 1.0, (name, worst)


@pytest.mark.parametrize('name', ['pend_gpqkf', 'cv_radar', 'ct_bearing', 'pend_ghkf'])
def test_7_batch_independence_and_the_device_route(amd, name):
    """B = 70 against the slices 0:64, 64:70 and 5:6, and masked_pass_dev against masked_pass_batch: equal bits."""
    from ssmtoybox_amd import _lib
    alg, _, y, mask = case_data(name, 'random')
    full = run_case(name, 'random')
    T = y.shape[1]
    for sl in (slice(0, 64), slice(64, 70), slice(5, 6)):
        out = as_run(alg, alg.masked_pass_batch(y[..., sl], mask=mask[:, sl], raise_on_failure=False, return_scores=True))
        for key in ('fm', 'fP', 'used', 'nis', 'll', 'status'):
            assert np.array_equal(out[key], full[key][..., sl]), (key, sl)
    Y, D, ld = y.shape[0], full['fm'].shape[0], 128
    d_y, d_mask = _lib.DeviceBuffer(8 * T * Y * ld), _lib.DeviceBuffer(4 * T * ld)
    _lib.upload_study(y, Y, ld, d_y)
    planes = np.zeros((T, ld), dtype=np.uint32)
    planes[:, :B] = mask
    d_mask.upload(planes)
    d_fm, d_fP, d_used, d_nis, d_ll, d_st = alg.masked_pass_dev(d_y, B, ld, T, d_mask=d_mask)
    assert np.array_equal(d_fm.download((T, D, ld))[:, :, :B].transpose(1, 0, 2), full['fm'])
    assert np.array_equal(d_fP.download((T, D, D, ld))[..., :B].transpose(1, 2, 0, 3), full['fP'])
    uw = d_used.download((T, ld), dtype=np.uint32)[:, :B]
    assert np.array_equal(((uw[None] >> np.arange(Y, dtype=np.uint32)[:, None, None]) & 1).astype(bool), full['used'])
    assert np.array_equal(d_nis.download((T, ld))[:, :B], full['nis']) and np.array_equal(d_ll.download((T, ld))[:, :B], full['ll'])
    assert not d_st.download((ld,), dtype=np.int32)[:B].any()
    for buf in (d_y, d_mask, d_fm, d_fP, d_used, d_nis, d_ll, d_st):
        buf.free()
    one = alg.masked_pass(y[..., 5], mask=mask[:, 5])
    assert np.array_equal(one[0], full['fm'][..., 5]) and np.array_equal(one[1], full['fP'][..., 5])


@pytest.mark.parametrize('name', ['pend_gpqkf', 'cv_radar', 'ct_bearing', 'pend_ghkf'])
def test_8_failed_trajectory_is_a_status_not_a_fault(amd, name):
    """One trajectory of 70 starts from P0 = -I (status 1), another has a NaN in an OBSERVED component at step 2 (status 3): NaN outputs
    and used = 0 from that step on; every other trajectory has the bits of a run without them."""
    alg, _, y, mask = case_data(name, 'pattern')
    full = run_case(name, 'pattern')
    D, bad = full['fm'].shape[0], 37
    nan_b = int(np.flatnonzero(mask[2] & 1)[3])            # component 0 is observed there
    P0 = np.broadcast_to(alg.x0_cov, (B, D, D)).copy()
    P0[bad] = -np.eye(D)
    yn = y.copy()
    yn[0, 2, nan_b] = np.nan
    with pytest.raises(np.linalg.LinAlgError):
        alg.masked_pass_batch(yn, mask=mask, x0_cov=P0)
    out = as_run(alg, alg.masked_pass_batch(yn, mask=mask, x0_cov=P0, raise_on_failure=False, return_scores=True))
    assert out['status'][bad] == 1 and out['status'][nan_b] == 3 and np.count_nonzero(out['status']) == 2
    keep = (np.arange(B) != bad) & (np.arange(B) != nan_b)
    for key in ('fm', 'fP', 'nis', 'll'):
        assert np.isnan(out[key][..., bad]).all() and np.isnan(out[key][..., 2:, nan_b]).all()
        assert np.array_equal(out[key][..., :2, nan_b], full[key][..., :2, nan_b])
        assert np.array_equal(out[key][..., keep], full[key][..., keep])
    assert not out['used'][..., bad].any() and not out['used'][:, 2:, nan_b].any()
    assert np.array_equal(out['used'][..., keep], full['used'][..., keep])


def test_9_user_pendulum_has_the_bits_of_the_builtin_pair(amd):
    alg, _, y, mask = case_data('user_pend', 'pattern')
    ukf = make_case('pend_ukf')
    assert ukf.masked_kernel_name().startswith('k_masked_loop<D=2,Y=1')
    out = as_run(ukf, ukf.masked_pass_batch(y, mask=mask, return_scores=True))
    same_bits(run_case('user_pend', 'pattern'), out)


def test_10_refusals_through_the_c_abi_leave_the_outputs_alone(amd):
    """Flags other than bit 0, a gate entry that is NaN or <= 0, an R that is not symmetric (SSMQ_E_ARG) and a pair the recursion does
    not cover (SSMQ_E_UNSUPPORTED) return before an output is touched."""
    from ssmtoybox_amd import _lib, ssinf, ssmod as sm
    from ssmtoybox_amd.mtran import resolve_integrand
    lib = _lib.load()
    alg, _, y, mask = case_data('ungm_ukf', 'pattern')
    cv = case_data('cv_radar', 'pattern')[0]
    na = ssinf.UnscentedKalman(sm.UNGMNATransition(sm.GaussRV(1), sm.GaussRV(1)), sm.UNGMNAMeasurement(sm.GaussRV(1), 1))
    T, ld, sent = y.shape[1], 128, -7.0259e+211
    planes = np.full((16 * T, ld), sent)                                  # (room for fP of D = 4)
    bufs = [_lib.DeviceBuffer(planes.nbytes) for _ in range(6)]          # fm, fP, used, nis, loglik, status
    for b in bufs:
        b.upload(planes)
    d_y, d_m0, d_P0, d_mask = _lib.DeviceBuffer(8 * 2 * T * ld), _lib.DeviceBuffer(8 * 4 * ld), _lib.DeviceBuffer(8 * 16 * ld), _lib.DeviceBuffer(4 * T * ld)
    _lib.upload_study(y, 1, ld, d_y)
    d_m0.upload(np.zeros((4, ld)))
    d_P0.upload(np.ones((16, ld)))
    mp = np.zeros((T, ld), dtype=np.uint32)
    mp[:, :B] = mask | np.uint32(1 << 20)                                 # (bits at or above Y are ignored)
    d_mask.upload(mp)

    def call(a, R, gate=None, flags=0):
        f_dyn, e_dyn = resolve_integrand(a.mod_dyn.dyn_eval)
        f_obs, e_obs = resolve_integrand(a.mod_obs.meas_eval)
        gqg, pg = _lib.as_c(a.G.dot(a.q_cov).dot(a.G.T))
        rr, pr = _lib.as_c(np.asarray(R, dtype=float))
        gt, pgt = (None, None) if gate is None else _lib.as_c(np.asarray(gate, dtype=float))
        vp = lambda b: ctypes.c_void_p(b.ptr)       # noqa: E731
        return lib.ssmq_filter_masked_dev(ctypes.c_void_p(a.tf_dyn._handle_for(e_dyn)), ctypes.byref(f_dyn),
                                          ctypes.c_void_p(a.tf_obs._handle_for(e_obs)), ctypes.byref(f_obs), B, ld, T, flags, vp(d_y),
                                          vp(d_mask), vp(d_m0), vp(d_P0), pg, pr, pgt, *[vp(b) for b in bufs])
    one = np.eye(1)
    for flags in (2, 3, 4, -2):
        assert call(alg, one, flags=flags) == -1 and 'flags' in _lib.last_error()
    for g in (0.0, -1.0, np.nan, -np.inf):
        assert call(alg, one, gate=[np.nan, g]) == -1 and 'gate' in _lib.last_error()
    assert call(cv, np.eye(2), gate=[1.0, 5.0, 0.0]) == -1 and 'gate' in _lib.last_error()
    for R in ([[1.0, 0.5], [0.4, 1.0]], [[1.0, np.nan], [np.nan, 1.0]]):
        assert call(cv, R) == -1 and 'symmetric' in _lib.last_error()
    assert call(na, one) == -3 and 'additive' in _lib.last_error()
    _lib.sync()
    for b in bufs:
        assert np.array_equal(b.download(planes.shape), planes)
    # ... and the accepted call (entry 0 of the gate is ignored) writes lanes 0 .. B - 1 of every plane and leaves the padding alone
    assert call(alg, alg.r_cov, gate=[np.nan, np.inf]) == 0
    _lib.sync()
    ref = run_case('ungm_ukf', 'pattern')
    for buf, key in ((bufs[0], 'fm'), (bufs[3], 'nis'), (bufs[4], 'll')):
        got = buf.download(planes.shape)[:T]
        assert np.array_equal(got[:, :B], ref[key].reshape(T, B)) and np.all(got[:, B:] == sent), key
    uw = bufs[2].download((T, ld), dtype=np.uint32)
    assert np.array_equal(uw[:, :B] != 0, ref['used'][0])
    for b in bufs + [d_y, d_m0, d_P0, d_mask]:
        b.free()


def test_11_mask_generator(amd):
    from ssmtoybox_amd import ssmod as sm
    T, Y, ld, p = 8, 4, 128, [0.9, 0.6, 0.3, 0.5]
    ref = mko.detection_mask(B, T, Y, p, seed=2024, traj_offset=5)

    def draw(nb, pitch, **kw):
        buf = sm.detection_mask_dev(nb, pitch, T, Y, kw.pop('p', p), **kw)
        out = buf.download((T, pitch), dtype=np.uint32)[:, :nb]
        buf.free()
        return out
    got = draw(B, ld, seed=2024, traj_offset=5)
    assert np.array_equal(got, ref)                                                  # the Philox restatement, exactly
    assert np.array_equal(draw(6, 64, seed=2024, traj_offset=5), ref[:, :6])         # independent of B and the pitch
    assert np.array_equal(draw(300, 320, seed=2024, traj_offset=5)[:, :B], ref)
    assert np.array_equal(draw(20, 64, seed=2024, traj_offset=35), ref[:, 30:50])    # consistent under traj_offset
    assert np.array_equal(draw(4, 64, seed=2024, traj_offset=(1 << 32) + 1), mko.detection_mask(4, T, Y, p, seed=2024, traj_offset=(1 << 32) + 1))
    assert not np.array_equal(draw(B, ld, seed=2025, traj_offset=5), ref)
    scan = draw(B, ld, seed=2024, traj_offset=5, per_component=False, p=[0.7])
    assert np.array_equal(scan, mko.detection_mask(B, T, Y, [0.7], seed=2024, traj_offset=5, per_component=False))
    assert set(np.unique(scan)) == {0, 15}                                           # the bits go together
    same_p = draw(B, ld, seed=2024, traj_offset=5, p=[0.7] * 4)
    assert np.array_equal(scan == 15, same_p & 1 == 1)                               # ... on the draw of component 0
    # the masks feed the pass
    alg, _, y, _ = case_data('ct_bearing', 'random')
    out = alg.masked_pass_batch(y, mask=got, return_scores=True)
    assert np.array_equal(out['n_used'], [sum(bin(int(v)).count('1') for v in got[:, b]) for b in range(B)])
