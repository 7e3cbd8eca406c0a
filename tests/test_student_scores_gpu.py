"""Student-t measurement likelihood (`student_scores*`) and the likelihood sweeps of the t-process filters on the device
(k_filter_score<>): against the CPU restatement (tests/_student_score_oracle.py) run on the device's weights, against
`forward_pass_batch`'s status, sweep rows against the filter built from the row, bit-for-bit independence of rows and trajectories,
failures that stay local, `fit_kernel_parameters`, and the kernel names.  Cases: tests/_student_score_cases.py.

Bounds: the rule of tests/test_innovation_gpu.py, no new tolerance - a step's nis within max(RTOL, 64 cond(S_y) eps) max(1, |value|),
cond(S_y) from the oracle's S_y of that step; a step's Student-t loglik within (dof + Y) / dof times that rule (|d loglik / d Delta^2| =
(dof + Y) / (2 (dof + Delta^2)) <= (dof + Y) / dof times the Gaussian's 1/2); a total within the sum of its steps' bounds (the mean NIS:
their mean).  The float64 oracle's own error against its long-double form is printed with every comparison; no case needed the MEASURED
convention of that file (the set below is empty): measured on an MI355X, the largest |error| / bound of any comparison is 6.4e-3 (nis,
UNGM t-process filter) and the oracle's own error at most 1.4e-14.  The likelihood tables of test_fit_kernel_parameters_is_the_oracle_argmax
have a margin best - second of 229.9 (Studentian) and 248.6 (Gaussian recursion) against summed bounds of 2e-7 per row.

Status.  `status` is 1 + the first step whose SCORES are not numbers - the convention of `likelihood_sweep_batch` and
`innovations_batch`.  On data every filter completes it equals `forward_pass_batch(raise_on_failure=False)`'s status, which is what
test_status_is_the_forward_pass_status asserts.  A NaN measurement at step 2 gives the scores' status 3 (asserted); the forward pass
stores the filtered moments and notices the NaN only when the NEXT step factors the poisoned scale matrix, so its own status for that
trajectory is 4 (asserted too): the two cannot be equal there, and the scores' number is the one that names the step."""
import numpy as np
import pytest

from tests import _student_score_cases as ssc
from tests._cases import RTOL

pytestmark = pytest.mark.gpu
EPS = float(np.finfo(float).eps)
MEASURED = ()
KEYS = ('nis', 'loglik', 'loglik_total', 'nis_mean', 'status')


@pytest.fixture(scope='module')
def amd():
    import ssmtoybox_amd
    if ssmtoybox_amd.device_count() < 1:
        pytest.fail('no device: the GPU tests need an MI355X')
    ssmtoybox_amd.set_device(0)
    return ssmtoybox_amd


_DATA, _RUNS = {}, {}


def data(amd, name):
    """The case's measurements (Y, T, B) from `simulate_dev` on the Student-t models, once."""
    if name not in _DATA:
        from ssmtoybox_amd import _lib, ssmod as sm
        dyn, obs = ssc.models(name)
        B, T = ssc.SHAPES[name]
        d_x, d_y, ld = sm.simulate_dev(dyn, obs, T, B, seed=21)
        _DATA[name] = np.ascontiguousarray(_lib.download_study(d_y, (obs.dim_out,), T, B, ld))
        d_x.free()
        d_y.free()
        assert np.all(np.isfinite(_DATA[name]))
    return _DATA[name]


def run(amd, name, kind, fixed):
    """student_scores_batch of a case's filter, once, shared by the tests (never modified)."""
    key = (name, kind, fixed)
    if key not in _RUNS:
        alg = ssc.make_filter(name, kind, fixed)
        _RUNS[key] = dict(alg=alg, out=alg.student_scores_batch(data(amd, name)))
    return _RUNS[key]


def bounds(ref, dof, Y, helper=(0.0, 0.0)):
    """(T, B) bounds of nis and loglik under the rule (dof None: the Gaussian score)."""
    T, B = ref['loglik'].shape
    f = np.array([[max(RTOL, 64.0 * np.linalg.cond(ref['S'][b][..., k]) * EPS) if np.isfinite(ref['loglik'][k, b]) else np.nan for b in range(B)]
                  for k in range(T)])
    g = 1.0 if dof is None else (dof + Y) / dof
    return np.maximum(f, 4.0 * helper[0]) * np.maximum(1.0, np.abs(ref['nis'])), np.maximum(g * f, 4.0 * helper[1]) * np.maximum(1.0, np.abs(ref['loglik']))


def check_against(what, out, ref, dof, Y, measured=False):
    helper = ref.get('helper_error', (0.0, 0.0))
    bn, bl = bounds(ref, dof, Y, helper if measured else (0.0, 0.0))
    for key in out:         # a trajectory that fails is NaN from the same step on in both (its status is compared below)
        assert np.array_equal(np.isnan(out[key]), np.isnan(ref[key])), (what, key)
    with np.errstate(invalid='ignore'):
        worst = {'loglik_total': np.nanmax(np.abs(out['loglik_total'] - ref['loglik_total']) / np.nansum(bl, axis=0)),
                 'nis_mean': np.nanmax(np.abs(out['nis_mean'] - ref['nis_mean']) / np.nanmean(bn, axis=0))}
        if 'nis' in out:
            worst['nis'] = np.nanmax(np.abs(out['nis'] - ref['nis']) / bn)
        if 'loglik' in out:
            worst['loglik'] = np.nanmax(np.abs(out['loglik'] - ref['loglik']) / bl)
    print('{}: largest |error| / bound = {}; float64 oracle against long double: nis {:.3g}, ll {:.3g}'.format(
        what, {k: float('{:.3g}'.format(v)) for k, v in worst.items()}, *helper))
    assert np.array_equal(out['status'], ref['status']), what
    assert max(worst.values()) <= 1.0, (what, worst)


@pytest.mark.parametrize('fixed', (True, False))
@pytest.mark.parametrize('kind', ('fs', 'tps'))
@pytest.mark.parametrize('name', ('ungm', 'pend'))
def test_scores_against_the_oracle(amd, name, kind, fixed):
    r, y = run(amd, name, kind, fixed), data(amd, name)
    alg, out = r['alg'], r['out']
    D, Y = alg.mod_dyn.dim_state, alg.mod_obs.dim_out
    assert alg.student_scores_kernel_name().startswith('k_filter_score<D={},'.format(D))
    assert ('SSMQ_FORM_SIGMA' if kind == 'fs' else 'TP=1') in alg.student_scores_kernel_name() and 'STU=1' in alg.student_scores_kernel_name()
    assert out['nis'].shape == out['loglik'].shape == y.shape[1:] and out['status'].dtype == np.int32
    ref = ssc.oracle_scores(alg, y, helper=True)
    assert (ref['status'] == 0).sum() >= y.shape[2] - 2
    check_against('student_scores {} {} fixed_dof={}'.format(name, kind, fixed), out, ref, float(alg.dof), Y, (name, kind, fixed) in MEASURED)
    # one trajectory through the single-trajectory method: the same bits
    one = alg.student_scores(y[..., 3])
    assert np.array_equal(one['loglik'], out['loglik'][:, 3]) and one['loglik_total'] == out['loglik_total'][3] and one['status'] == out['status'][3] == 0


@pytest.mark.parametrize('kind', ('fs', 'tps'))
@pytest.mark.parametrize('name', ('ungm', 'pend'))
def test_status_is_the_forward_pass_status(amd, name, kind):
    r, y = run(amd, name, kind, False), data(amd, name)
    alg, out = ssc.make_filter(name, kind, False), r['out']
    alg.forward_pass_batch(y, raise_on_failure=False)
    assert np.array_equal(out['status'], alg.status)
    # a NaN measurement at step 2 of one trajectory
    step, bad = 2, 3
    yn = y.copy()
    yn[0, step, bad] = np.nan
    got = alg.student_scores_batch(yn)
    keep = np.arange(y.shape[2]) != bad
    assert got['status'][bad] == 3 == 1 + step
    assert np.isnan(got['loglik_total'][bad]) and np.isnan(got['nis_mean'][bad]) and np.isnan(got['loglik'][step:, bad]).all()
    assert np.array_equal(got['loglik'][:step, bad], out['loglik'][:step, bad]) and np.array_equal(got['nis'][:step, bad], out['nis'][:step, bad])
    for key in KEYS:
        assert np.array_equal(got[key][..., keep], out[key][..., keep]), key
    alg.forward_pass_batch(yn, raise_on_failure=False)
    print('NaN measurement at step {}: status of the scores {}, of the forward pass {}'.format(step, got['status'][bad], alg.status[bad]))
    assert np.array_equal(alg.status[keep], got['status'][keep]) and alg.status[bad] == 2 + step     # (see the module's docstring)


_SWEEPS = {}


def sweep(amd, name, kind):
    key = (name, kind)
    if key not in _SWEEPS:
        par, nu, dof = ssc.ROWS[name]
        alg = ssc.make_filter(name, kind, False)
        kw = dict(nu=nu, dof=dof) if kind == 'tps' else dict(nu=nu)
        _SWEEPS[key] = dict(alg=alg, kw=kw, out=alg.likelihood_sweep_batch(data(amd, name), par, par, steps=True, **kw))
    return _SWEEPS[key]


@pytest.mark.parametrize('name', ('ungm', 'pend'))
def test_student_sweep_row_is_the_filter_of_the_row_bit_for_bit(amd, name):
    par, nu, dof = ssc.ROWS[name]
    s, y = sweep(amd, name, 'tps'), data(amd, name)
    D = s['alg'].mod_dyn.dim_state
    name_k = s['alg'].likelihood_sweep_kernel_name(len(par))
    assert name_k.startswith('k_filter_score<D={},'.format(D)) and 'TP=1' in name_k and 'STU=1' in name_k
    assert not s['out']['theta_status'].any()
    for p in range(len(par)):
        alg = ssc.make_filter(name, 'tps', False, par[p], dof[p], nu[p])
        one = alg.student_scores_batch(y)
        assert alg.student_scores_kernel_name() == name_k
        for key in ('loglik', 'loglik_total', 'nis_mean', 'status'):
            assert np.array_equal(one[key], s['out'][key][p]), (key, p)
        # ... and the oracle, on that filter's (the device's) weights
        ref = ssc.oracle_scores(alg, y, helper=True)
        check_against('student sweep {} row {}'.format(name, p), {k: s['out'][k][p] for k in ('loglik', 'loglik_total', 'nis_mean', 'status')}, ref,
                      float(dof[p]), y.shape[0])
    # fixed_dof = True: the scale table comes from the laws' dof and is the same for every row
    alg = ssc.make_filter(name, 'tps', True)
    got = alg.likelihood_sweep_batch(y, par[1:3], par[1:3], nu=nu[1:3], dof=dof[1:3])
    for p in (1, 2):
        one = ssc.make_filter(name, 'tps', True, par[p], dof[p], nu[p]).student_scores_batch(y)
        assert np.array_equal(one['loglik_total'], got['loglik_total'][p - 1]) and np.array_equal(one['nis_mean'], got['nis_mean'][p - 1])


@pytest.mark.parametrize('name', ('ungm', 'pend'))
def test_gaussian_sweep_row_is_the_two_call_path(amd, name):
    par, nu, _ = ssc.ROWS[name]
    s, y = sweep(amd, name, 'tpk'), data(amd, name)
    name_k = s['alg'].likelihood_sweep_kernel_name()
    assert name_k.startswith('k_filter_score<D={},'.format(s['alg'].mod_dyn.dim_state)) and 'TP=1' in name_k and 'STU=0' in name_k
    assert not s['out']['theta_status'].any()
    equal = []
    for p in range(len(par)):
        alg = ssc.make_filter(name, 'tpk', par=par[p], nu=nu[p])
        fm, fP = alg.forward_pass_batch(y, raise_on_failure=False)
        inn = alg.innovations_batch(y, fi_mean=fm, fi_cov=fP)
        row = {k: s['out'][k][p] for k in ('loglik', 'loglik_total', 'nis_mean', 'status')}
        equal.append(bool(np.array_equal(row['loglik'], inn['loglik'])))
        ref = ssc.oracle_scores(alg, y, helper=True)
        check_against('gaussian t-process sweep {} row {} against the oracle'.format(name, p), row, ref, None, y.shape[0])
        ref2 = dict(inn, S=ref['S'])
        check_against('gaussian t-process sweep {} row {} against the two-call path'.format(name, p), row, ref2, None, y.shape[0])
    print('gaussian t-process sweep {}: rows bit-equal to the two-call path: {}'.format(name, equal))


def test_rows_and_trajectories_are_independent_bit_for_bit(amd):
    par, nu, dof = ssc.ROWS['ungm']
    y = data(amd, 'ungm')
    keys = ('loglik', 'loglik_total', 'nis_mean', 'status')
    for kind in ('tps', 'tpk'):
        s = sweep(amd, 'ungm', kind)
        alg, out, kw = s['alg'], s['out'], s['kw']
        for B in (1, 64, 65, 70):
            got = alg.likelihood_sweep_batch(y[..., :B], par, par, steps=True, **kw)
            for key in keys:
                assert np.array_equal(got[key], out[key][..., :B]), (kind, key, B)
        perm = np.array([2, 0, 3, 1])
        got = alg.likelihood_sweep_batch(y, par[perm], par[perm], steps=True, **{k: v[perm] for k, v in kw.items()})
        for key in keys:
            assert np.array_equal(got[key], out[key][perm]), (kind, key)
        for p in range(len(par)):
            one = alg.likelihood_sweep_batch(y, par[p:p + 1], par[p:p + 1], steps=True, **{k: v[p:p + 1] for k, v in kw.items()})
            for key in keys:
                assert np.array_equal(one[key][0], out[key][p]), (kind, key, p)
    # trajectories of student_scores_batch, and the device route
    r = run(amd, 'ungm', 'fs', False)
    for B in (1, 64, 65):
        got = r['alg'].student_scores_batch(y[..., :B])
        for key in KEYS:
            assert np.array_equal(got[key], r['out'][key][..., :B]), (key, B)
    from ssmtoybox_amd import _lib
    (Y, T, B), ld = y.shape, 128
    d_y = _lib.DeviceBuffer(8 * T * Y * ld)
    _lib.upload_study(y, Y, ld, d_y)
    bufs = r['alg'].student_scores_dev(d_y, B, ld, T)
    assert np.array_equal(_lib.download_study(bufs[1], (), T, B, ld), r['out']['loglik']) and np.array_equal(bufs[2].download((ld,))[:B], r['out']['loglik_total'])
    assert np.array_equal(bufs[4].download((ld,), dtype=np.int32)[:B], r['out']['status'])
    s = sweep(amd, 'ungm', 'tps')
    dev = s['alg'].likelihood_sweep_dev(d_y, B, ld, T, par, par, steps=True, **s['kw'])
    assert np.array_equal(dev[0].download((4, ld))[:, :B], s['out']['loglik_total']) and not dev[4].any()
    for buf in (d_y,) + tuple(bufs) + tuple(dev[:4]):
        buf.free()


def test_a_failed_row_stays_local(amd):
    par, nu, dof = ssc.ROWS['ungm']
    y = data(amd, 'ungm')
    at = 2
    grid = np.insert(par, at, ssc.BAD_ROW['ungm'], axis=0)
    good = np.arange(len(par) + 1) != at
    for kind in ('tps', 'tpk'):
        s = sweep(amd, 'ungm', kind)
        kw = {k: np.insert(v, at, v[0]) for k, v in s['kw'].items()}
        got = s['alg'].likelihood_sweep_batch(y, grid, grid, steps=True, **kw)
        assert got['theta_status'][at] != 0 and not got['theta_status'][good].any()
        assert (got['status'][at] == -1).all() and np.isnan(got['loglik_total'][at]).all() and np.isnan(got['nis_mean'][at]).all()
        assert np.isnan(got['loglik'][at]).all()
        for key in ('loglik', 'loglik_total', 'nis_mean', 'status'):
            assert np.array_equal(got[key][good], s['out'][key]), (kind, key)
        with pytest.raises(ValueError, match='weights of every parameter row failed'):
            s['alg'].fit_kernel_parameters(y, grid[at:at + 1], grid[at:at + 1])


def test_fit_kernel_parameters_is_the_oracle_argmax(amd):
    """UNGM, the four rows of the case: the oracle's likelihood table (on the device's weights of every row) has its best and second-best
    entries further apart than the summed bounds of the two - the margin is printed and asserted before the comparison."""
    par, nu, dof = ssc.ROWS['ungm']
    y = data(amd, 'ungm')
    for kind in ('tps', 'tpk'):
        s = sweep(amd, 'ungm', kind)
        want, bound = np.zeros(len(par)), np.zeros(len(par))
        for p in range(len(par)):
            alg = ssc.make_filter('ungm', kind, False, par[p], dof[p], nu[p])
            ref = ssc.oracle_scores(alg, y)
            want[p] = ref['loglik_total'].sum()
            bound[p] = bounds(ref, float(dof[p]) if kind == 'tps' else None, 1)[1].sum()
        order = np.argsort(want)
        margin = want[order[-1]] - want[order[-2]]
        print('{} likelihood table: oracle {}, summed bounds {}, margin best - second {:.4g}'.format(kind, want, bound, margin))
        assert margin > bound[order[-1]] + bound[order[-2]]
        index, pd, po, table = s['alg'].fit_kernel_parameters(y, par, par, **s['kw'])
        assert index == int(order[-1]) and np.array_equal(pd, par[index]) and np.array_equal(po, par[index])
        assert np.all(np.abs(table - want) <= bound)


def test_the_object_is_unchanged(amd):
    y = data(amd, 'pend')
    par, nu, dof = ssc.ROWS['pend']
    alg = ssc.make_filter('pend', 'tps', False)
    alg.forward_pass_batch(y)
    before = [np.array(a, copy=True) for a in (alg.tf_dyn.wm, alg.tf_dyn.Wc, alg.tf_dyn.Wcc, alg.tf_obs.wm, alg.fi_mean, alg.fi_cov, alg.status)]
    alg.student_scores_batch(y)
    alg.likelihood_sweep_batch(y, par, par, nu=nu, dof=dof)
    alg.fit_kernel_parameters(y, par, par, nu=nu, dof=dof)
    after = (alg.tf_dyn.wm, alg.tf_dyn.Wc, alg.tf_dyn.Wcc, alg.tf_obs.wm, alg.fi_mean, alg.fi_cov, alg.status)
    for a, b in zip(before, after):
        assert np.array_equal(a, b)
    assert alg.tf_dyn.model.nu == 4.0 and alg.dof == 4.0
