"""Innovation scores on the device against the NumPy helper (tests/_innovation_oracle.py): k_innovation<> for the table shapes and
a user pair, the launch-loop route for the other forms.  Shapes: the smallest that cross a wave (B = 65 / 70) and reach every branch.

Bounds: y_mean, S by assert_moments_close / RTOL as the transform parity tests; nis, ll by max(RTOL, 64 cond(S) eps) max(1, |value|),
the project's bound for one application of an inverse (tests/test_gpu_parity.py), cond(S) from the helper's S.  One case needs more
(reentry + radar, UKF: device against helper 4.4e-10 where that bound is 1e-10): there the float64 helper's own error against its
long-double restatement is measured (3.4e-10 for nis, 5.6e-11 for ll, relative to max(1, |value|)) and 4 x that is allowed."""
import numpy as np
import pytest

from oracle import ssmq_oracle as orc
from tests import _innovation_oracle as ino
from tests import _truncated_oracle as tro
from tests._cases import RTOL, assert_moments_close
from tests._mo_oracle import mo_moments
from tests.test_innovation_host import pendulum_user

pytestmark = pytest.mark.gpu
EPS = float(np.finfo(float).eps)


@pytest.fixture(scope='module')
def amd():
    import ssmtoybox_amd
    if ssmtoybox_amd.device_count() < 1:
        pytest.fail('no device: the GPU tests need an MI355X')
    ssmtoybox_amd.set_device(0)
    return ssmtoybox_amd


def oracle_tf(tf, model_eval):
    """The transform object `tf` applied to the model behind `model_eval`, restated on the oracle."""
    from ssmtoybox_amd import mtran
    from ssmtoybox_amd.bq import bqmtran
    f, _ = mtran.resolve_integrand(model_eval)
    fid, p = f.id, tuple(f.par[i] for i in range(f.n_par))
    sidx = tuple(f.idx[i] for i in range(f.n_idx)) if f.n_idx else None
    if isinstance(tf, mtran.LinearizationTransform):
        return ino.linear_tf(fid, p, sidx)
    if isinstance(tf, mtran.TruncatedSigmaPointTransform):
        return lambda m, P, t: tro.apply(tro.integrand(fid, p, float(t)), m, P, tf.dim_eff, tf.unit_sp_eff, tf.wm, np.diag(tf.Wc), tf.unit_sp,
                                         np.diag(tf.Wcc))
    if isinstance(tf, bqmtran.MultiOutputGaussianProcessTransform):
        def mo(m, P, t):
            chol = np.linalg.cholesky(P)
            fx = orc.eval_columns(fid, m[:, None] + chol.dot(tf.model.points), float(t), p, sidx)
            return mo_moments(fx, chol, tf.wm, tf.Wc, tf.Wcc, tf.model.model_var)
        return mo
    if hasattr(tf, 'model'):
        w = dict(wm=tf.wm, Wc=tf.Wc, Wcc=tf.Wcc, model_var=tf.model.model_var, iK=tf.model.iK)
        nu = tf.model.nu if isinstance(tf, bqmtran.StudentTProcessTransform) else None
        return ino.bq_tf(fid, p, tf.model.points, w, sidx, nu)
    return ino.sigma_tf(fid, p, tf.unit_sp, tf.wm, np.diag(tf.Wc), sidx)


def simulate(alg, B, T, seed):
    """Measurements (Y, T, B) of noisy trajectories of the filter's own models, from the oracle's integrands."""
    from ssmtoybox_amd import mtran
    rng = np.random.default_rng(seed)
    fd, _ = mtran.resolve_integrand(alg.mod_dyn.dyn_eval)
    fo, _ = mtran.resolve_integrand(alg.mod_obs.meas_eval)
    pd, po = tuple(fd.par[i] for i in range(fd.n_par)), tuple(fo.par[i] for i in range(fo.n_par))
    so = [fo.idx[i] for i in range(fo.n_idx)] if fo.n_idx else None
    D, Y = alg.mod_dyn.dim_state, alg.mod_obs.dim_out
    Gq = alg.G.dot(np.linalg.cholesky(np.atleast_2d(alg.q_cov)))
    L0, Lr = np.linalg.cholesky(alg.x0_cov), np.linalg.cholesky(alg.r_cov)
    y = np.zeros((Y, T, B))
    for b in range(B):
        x = alg.x0_mean + L0.dot(rng.standard_normal(D))
        for k in range(T):
            x = orc.integrand(fd.id, x, float(k), pd)
            x = x + Gq.dot(rng.standard_normal(Gq.shape[1]))
            y[:, k, b] = orc.integrand(fo.id, x if so is None else x[so], float(k), po) + Lr.dot(rng.standard_normal(Y))
    return y


def make_case(amd, name):
    """(filter, B, T) of a case of the table."""
    from ssmtoybox_amd import ssinf, ssmod as sm
    one = np.array([[1.0, 3.0]])
    if name.startswith('ungm'):
        dyn = sm.UNGMTransition(sm.GaussRV(1), sm.GaussRV(1, cov=np.array([[10.0]])))
        obs = sm.UNGMMeasurement(sm.GaussRV(1), 1)
        alg = {'ungm_ukf': lambda: ssinf.UnscentedKalman(dyn, obs), 'ungm_gpqkf': lambda: ssinf.GaussianProcessKalman(dyn, obs, one, one, 'rbf', 'ut'),
               'ungm_tpqkf': lambda: ssinf.StudentProcessKalman(dyn, obs, one, one, 'rbf', 'ut', nu=4.0)}[name]()
        return alg, 70, 5
    if name.startswith('pend') or name == 'user_pend':
        m0, P0 = np.array([1.5, 0.0]), 0.01 * np.eye(2)
        Q = 0.01 * np.array([[0.01 ** 3 / 3, 0.01 ** 2 / 2], [0.01 ** 2 / 2, 0.01]])
        Dyn, Obs = pendulum_user() if name == 'user_pend' else (sm.Pendulum2DTransition, sm.Pendulum2DMeasurement)
        dyn, obs = Dyn(sm.GaussRV(2, m0, P0), sm.GaussRV(2, cov=Q)), Obs(sm.GaussRV(1, cov=np.array([[0.1]])), 2)
        par = np.array([[1.0, 2.0, 2.0]])
        alg = {'pend_ukf': lambda: ssinf.UnscentedKalman(dyn, obs), 'pend_ckf': lambda: ssinf.CubatureKalman(dyn, obs),
               'user_pend': lambda: ssinf.UnscentedKalman(dyn, obs), 'pend_ghkf': lambda: ssinf.GaussHermiteKalman(dyn, obs, deg=3),
               'pend_mo': lambda: ssinf.MultiOutputGaussianProcessKalman(dyn, obs, np.array([[1.0, 2.0, 2.0], [1.1, 2.5, 1.5]]), par),
               'pend_trunc': lambda: ssinf.TruncatedUnscentedKalman(dyn, obs), 'pend_ekf': lambda: ssinf.ExtendedKalman(dyn, obs)}[name]()
        return alg, 65, 3
    if name == 'cv_radar':
        dyn = sm.ConstantVelocity(sm.GaussRV(4, np.array([100.0, 5.0, 200.0, -3.0]), np.diag([1.0, 0.1, 1.0, 0.1])), sm.GaussRV(2, cov=0.1 * np.eye(2)))
        obs = sm.Radar2DMeasurement(sm.GaussRV(2, cov=np.diag([0.5, 1e-4])), 4)
        return ssinf.UnscentedKalman(dyn, obs), 65, 3
    if name.startswith('reentry'):
        m0 = np.array([6500.4, 349.14, -1.8093, -6.7967, 0.6932])
        dyn = sm.ReentryVehicle2DTransition(sm.GaussRV(5, m0, np.diag([1e-6, 1e-6, 1e-6, 1e-6, 1.0])),
                                            sm.GaussRV(3, cov=np.diag([2.4064e-5, 2.4064e-5, 1e-6])))
        obs = sm.Radar2DMeasurement(sm.GaussRV(2, cov=np.diag([1e-6, 0.17e-3 ** 2])), 5, radar_loc=np.array([6374.0, 0.0]))
        par = np.array([[1.0] + [3.0] * 5])
        alg = ssinf.UnscentedKalman(dyn, obs) if name == 'reentry_ukf' else ssinf.GaussianProcessKalman(dyn, obs, par, par, 'rbf', 'ut')
        return alg, 65, 2
    if name == 'ct_bearing':
        m0 = np.array([130.0, 35.0, -20.0, 20.0, -4 * np.pi / 180])
        dyn = sm.CoordinatedTurnTransition(sm.GaussRV(5, m0, np.diag([5.0, 5.0, 5.0, 5.0, 1e-4])), sm.GaussRV(5, cov=np.diag([0.1, 0.1, 0.1, 0.1, 1e-6])))
        sensors = np.vstack((1000 * np.eye(2), -1000 * np.eye(2))).astype(float)
        obs = sm.BearingMeasurement(sm.GaussRV(4, cov=1e-4 * np.eye(4)), 5, state_index=[0, 2], sensor_pos=sensors)
        return ssinf.UnscentedKalman(dyn, obs), 65, 2
    raise KeyError(name)


ONE_LAUNCH = ('ungm_ukf', 'ungm_gpqkf', 'ungm_tpqkf', 'pend_ukf', 'pend_ckf', 'cv_radar', 'reentry_gpqkf', 'reentry_ukf', 'ct_bearing', 'user_pend')
LOOP = ('pend_ghkf', 'pend_mo', 'pend_trunc', 'pend_ekf')
_RUNS = {}


def run_case(amd, name):
    """The case run once on the device and once on the helper, shared by the tests (never modified)."""
    if name not in _RUNS:
        alg, B, T = make_case(amd, name)
        y = simulate(make_case(amd, 'pend_ukf')[0] if name == 'user_pend' else alg, B, T, 3)
        fm, fP = alg.forward_pass_batch(y, raise_on_failure=False)
        assert not alg.status.any(), name
        out = alg.innovations_batch(y, fi_mean=fm, fi_cov=fP, return_moments=True)
        twin = make_case(amd, 'pend_ukf')[0] if name == 'user_pend' else alg      # (the helper evaluates the built-in models)
        tfd, tfo = oracle_tf(alg.tf_dyn, twin.mod_dyn.dyn_eval), oracle_tf(alg.tf_obs, twin.mod_obs.meas_eval)
        GQG = alg.G.dot(alg.q_cov).dot(alg.G.T)
        ref = [ino.innovations(y[..., b], alg.x0_mean, alg.x0_cov, fm[..., b], fP[..., b], GQG, alg.r_cov, tfd, tfo) for b in range(B)]
        _RUNS[name] = dict(alg=alg, B=B, T=T, y=y, fm=fm, fP=fP, out=out, ref=ref, GQG=GQG)
    return _RUNS[name]


# cases whose scores need more than the bound of one inverse: the helper's own float64 error decides (measured here against the
# long-double restatement; DESIGN.md 3.35 records the values)
MEASURED = ('reentry_ukf',)


def helper_error_of(r, name):
    if name not in MEASURED:
        return (0.0, 0.0)
    from ssmtoybox_amd import mtran
    alg, args = r['alg'], []
    for tf, ev in ((alg.tf_dyn, alg.mod_dyn.dyn_eval), (alg.tf_obs, alg.mod_obs.meas_eval)):
        f, _ = mtran.resolve_integrand(ev)
        args.append(ino.sigma_tf_ld(f.id, tuple(f.par[i] for i in range(f.n_par)), tf.unit_sp, tf.wm, np.diag(tf.Wc),
                                    tuple(f.idx[i] for i in range(f.n_idx)) if f.n_idx else None))
    worst = np.zeros(2)
    for b in range(r['B']):
        worst = np.maximum(worst, ino.helper_error(r['y'][..., b], alg.x0_mean, alg.x0_cov, r['fm'][..., b], r['fP'][..., b], r['GQG'], alg.r_cov,
                                                   args[0], args[1], r['ref'][b][2], r['ref'][b][3]))
    print('helper float64 error {}: nis {:.3g}, ll {:.3g} (relative to max(1, |value|))'.format(name, *worst))
    return tuple(worst)


def score_bound(S, value):
    return max(RTOL, 64.0 * np.linalg.cond(S) * EPS) * max(1.0, abs(value))


def check_scores(got, ref_nis, ref_ll, ref_S, what, helper_err=(0.0, 0.0)):
    """nis (T, B), loglik (T, B) of `got` against the helper's, each within the bound of its own S - or, where the float64 helper
    itself is worth less than that on the case, within 4 x its measured error (helper_err: max |float64 helper - long-double
    restatement| / max(1, |value|) of nis and ll over the case; the device sums in another order).  Prints the largest ratio."""
    worst = 0.0
    T, B = got['nis'].shape
    for b in range(B):
        for k in range(T):
            for (key, r), he in zip((('nis', ref_nis[b][k]), ('loglik', ref_ll[b][k])), helper_err):
                bound = max(score_bound(ref_S[b][..., k], r), 4.0 * he * max(1.0, abs(r)))
                worst = max(worst, abs(got[key][k, b] - r) / bound)
    print('innovation scores {}: largest |error| / bound = {:.3g}'.format(what, worst))
    assert worst <= 1.0, (what, worst)


@pytest.mark.parametrize('name', ONE_LAUNCH + LOOP)
def test_moments_and_scores_against_the_helper(amd, name):
    r = run_case(amd, name)
    alg, out, B, T = r['alg'], r['out'], r['B'], r['T']
    kn = alg.innovations_kernel_name()
    assert kn.startswith('k_innovation<') if name in ONE_LAUNCH else kn.startswith('launch loop'), kn
    assert ('run-time compiled' in kn) == (name == 'user_pend')
    zero = np.zeros((1, 1))
    for b in range(B):
        ym, S, nis, ll = r['ref'][b]
        for k in range(T):
            P_in = alg.x0_cov if k == 0 else r['fP'][..., k - 1, b]
            assert_moments_close((out['y_mean'][:, k, b], out['y_cov'][:, :, k, b], zero), (ym[:, k], S[..., k], zero), P_in, what=(name, b, k))
        assert np.array_equal(out['y_cov'][..., b], out['y_cov'][..., b].transpose(1, 0, 2))
    check_scores(out, [x[2] for x in r['ref']], [x[3] for x in r['ref']], [x[1] for x in r['ref']], name, helper_error_of(r, name))
    # totals: the ascending-order sums of the per-step arrays, bit for bit
    sl, sn = np.zeros(B), np.zeros(B)
    for k in range(T):
        sl, sn = sl + out['loglik'][k], sn + out['nis'][k]
    assert np.array_equal(out['loglik_total'], sl) and np.array_equal(out['nis_mean'], sn / T)
    assert out['status'].dtype == np.int32 and not out['status'].any()
    # null moment outputs: the same scores
    bare = alg.innovations_batch(r['y'], fi_mean=r['fm'], fi_cov=r['fP'])
    assert set(bare) == {'nis', 'loglik', 'loglik_total', 'nis_mean', 'status'}
    for key in bare:
        assert np.array_equal(bare[key], out[key]), key


def test_user_pendulum_has_the_bits_of_the_builtin_pair(amd):
    a, b = run_case(amd, 'pend_ukf'), run_case(amd, 'user_pend')
    assert np.array_equal(a['fm'], b['fm']) and np.array_equal(a['fP'], b['fP'])
    for key in ('nis', 'loglik', 'loglik_total', 'nis_mean', 'status', 'y_mean', 'y_cov'):
        assert np.array_equal(a['out'][key], b['out'][key]), key


@pytest.mark.parametrize('name', ['ungm_gpqkf', 'cv_radar', 'pend_ghkf'])
def test_batch_independence(amd, name):
    """B = 193 against the same trajectories in batches of 1 and 64: equal bits."""
    alg, _, T = make_case(amd, name)
    y = simulate(alg, 193, T, 9)
    fm, fP = alg.forward_pass_batch(y, raise_on_failure=False)
    full = alg.innovations_batch(y, fi_mean=fm, fi_cov=fP, return_moments=True)
    for sl in (slice(0, 64), slice(64, 128), slice(70, 71), slice(192, 193)):
        part = alg.innovations_batch(y[..., sl], fi_mean=fm[..., sl], fi_cov=fP[..., sl], return_moments=True)
        for key in full:
            assert np.array_equal(part[key], full[key][..., sl], equal_nan=True), (key, sl)


@pytest.mark.parametrize('name', ['ungm_ukf', 'pend_ukf', 'cv_radar', 'reentry_gpqkf', 'ct_bearing'])
def test_launch_loop_route_agrees(amd, name, monkeypatch):
    r = run_case(amd, name)
    monkeypatch.setenv('SSMQ_NO_FUSED', '1')
    assert r['alg'].innovations_kernel_name().startswith('launch loop')
    loop = r['alg'].innovations_batch(r['y'], fi_mean=r['fm'], fi_cov=r['fP'])
    monkeypatch.delenv('SSMQ_NO_FUSED')
    assert not loop['status'].any()
    check_scores(loop, r['out']['nis'].T, r['out']['loglik'].T, [x[1] for x in r['ref']], name + ' (launch loop against one launch)')


@pytest.mark.parametrize('name', ['pend_ukf', 'cv_radar', 'pend_ghkf'])
def test_failed_trajectory_is_a_status_not_a_fault(amd, name):
    """One trajectory of 65 starts from P0 = -I: status 1 and NaN rows; every other trajectory has the bits of a run without it."""
    r = run_case(amd, name)
    alg, B, T = r['alg'], r['B'], r['T']
    D = alg.mod_dyn.dim_state
    bad = 37
    P0 = np.broadcast_to(alg.x0_cov, (B, D, D)).copy()
    P0[bad] = -np.eye(D)
    fm, fP = alg.forward_pass_batch(r['y'], x0_cov=P0, raise_on_failure=False)
    assert alg.status[bad] == 1
    out = alg.innovations_batch(r['y'], x0_cov=P0, fi_mean=fm, fi_cov=fP, return_moments=True)
    assert out['status'][bad] == 1 and np.count_nonzero(out['status']) == 1
    for key in ('nis', 'loglik', 'y_mean', 'y_cov', 'loglik_total', 'nis_mean'):
        assert np.isnan(out[key][..., bad]).all(), key
        keep = np.arange(B) != bad
        assert np.array_equal(out[key][..., keep], r['out'][key][..., keep]), key


def test_dev_route_and_anis(amd):
    """simulate -> filter -> innovations_dev with everything on the device: the planes are those of innovations_batch."""
    r = run_case(amd, 'ungm_gpqkf')
    alg, B, T, y = r['alg'], r['B'], r['T'], r['y']
    from ssmtoybox_amd import _lib
    ld = 128
    d_y = _lib.DeviceBuffer(8 * T * ld)
    _lib.upload_study(y, 1, ld, d_y)
    d_fm, d_fP, d_st = alg.forward_pass_dev(d_y, B, ld, T)
    d_nis, d_ll, d_tot, d_ist = alg.innovations_dev(d_y, d_fm, d_fP, B, ld, T)
    nis = d_nis.download((T, ld))[:, :B]
    assert np.array_equal(nis, r['out']['nis']) and np.array_equal(d_ll.download((T, ld))[:, :B], r['out']['loglik'])
    tot = d_tot.download((2, ld))
    assert np.array_equal(tot[0, :B], r['out']['loglik_total']) and np.array_equal(tot[1, :B], r['out']['nis_mean'])
    assert not d_ist.download((ld,), dtype=np.int32)[:B].any()
    one = alg.innovations(y[..., 0])
    assert np.array_equal(one['nis'], r['out']['nis'][:, 0]) and one['loglik_total'] == r['out']['loglik_total'][0]
    for buf in (d_y, d_fm, d_fP, d_st, d_nis, d_ll, d_tot, d_ist):
        buf.free()
