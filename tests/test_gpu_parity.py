"""
Parity of the HIP path (through the C ABI / ctypes, never through the oracle) with the reference:
  - golden vectors produced by the reference itself (tests/golden/*.npz),
  - the CPU oracle on seeded random batches,
  - size-independent properties at BASELINE.json's full batch sizes.
Bar: 1e-10 relative in fp64 (scales defined in tests/_cases.py: moment_scales); weights that go through K^-1 are
reproducible only to cond(K) eps / cond(K)^2 eps and are checked against that.
All tests need a real MI355X.
"""
import ctypes
import os

import numpy as np
import pytest

from oracle import ssmq_oracle as orc
from tests._cases import MODELS, SIGMA_TF, BQ_TF, SENSORS, assert_moments_close, rel_err, RTOL, cov_err, mean_err, mean_err_sigma, within, capped
from tests.golden.make_golden_cases import GP_CASES, BS_CASES, gp_par
from tests._jacobian_cases import linear_models

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def amd():
    import ssmtoybox_amd
    assert ssmtoybox_amd.device_count() >= 1, 'no GPU visible - the HIP path cannot run (there is no CPU fallback)'
    return ssmtoybox_amd


def make_model(name):
    from ssmtoybox_amd import ssmod as sm
    r = sm.GaussRV
    table = {
        'ungm_dyn': lambda: (sm.UNGMTransition(), 'dyn'),
        'ungm_meas': lambda: (sm.UNGMMeasurement(r(1), 1), 'meas'),
        'ungmna_dyn': lambda: (sm.UNGMNATransition(), 'dyn'),
        'ungmna_meas': lambda: (sm.UNGMNAMeasurement(r(1), 1), 'meas'),
        'pend_dyn': lambda: (sm.Pendulum2DTransition(dt=0.01), 'dyn'),
        'pend_meas': lambda: (sm.Pendulum2DMeasurement(r(1), 2), 'meas'),
        'reentry_dyn': lambda: (sm.ReentryVehicle2DTransition(), 'dyn'),
        'radar_meas': lambda: (sm.Radar2DMeasurement(r(2), 5), 'meas'),
        'ct_dyn': lambda: (sm.CoordinatedTurnTransition(), 'dyn'),
        'bearing_meas': lambda: (sm.BearingMeasurement(r(4), 5, state_index=[0, 2], sensor_pos=SENSORS), 'meas'),
        'cv_dyn': lambda: (sm.ConstantVelocity(), 'dyn'),
        'reentry1d_dyn': lambda: (sm.ReentryVehicle1DTransition(), 'dyn'),
        'range_meas': lambda: (sm.RangeMeasurement(r(1), 3), 'meas'),
        'ctrs_dyn': lambda: (sm.ConstantTurnRateSpeed(), 'dyn'),
    }
    mod, kind = table[name]()
    return mod, (mod.dyn_eval if kind == 'dyn' else mod.meas_eval)


def make_transform(amd, tname, din, dout, g=None, key=None):
    """Transform object of this build; BQ weights are then overwritten with the reference's own (golden) weights, as
    the reference's research code does (research/tpq/tpq_ungm.py:114-124), so that apply() is compared in isolation."""
    if tname == 'ut':
        return amd.UnscentedTransform(din)
    if tname == 'sr':
        return amd.SphericalRadialTransform(din)
    if tname == 'gh':
        return amd.GaussHermiteTransform(din, 3)
    if tname == 'fs':
        return amd.FullySymmetricStudentTransform(din, 3)
    ell = 3.0
    par = gp_par(din, ell)
    if tname == 'gpq':
        tf = amd.GaussianProcessTransform(din, dout, par, 'rbf', 'ut')
    elif tname == 'gpqsr':
        tf = amd.GaussianProcessTransform(din, dout, gp_par(din, 3.0, 1.3, True), 'rbf', 'sr')
    elif tname == 'tpq':
        tf = amd.StudentTProcessTransform(din, dout, par, 'rbf', 'ut')
    elif tname == 'tpq1':
        tf = amd.StudentTProcessTransform(din, 1, par, 'rbf', 'ut')
    else:
        mi = np.hstack((np.zeros((din, 1)), np.eye(din), 2 * np.eye(din))).astype(int)
        tf = amd.BayesSardTransform(din, dout, par, mi, 'ut')
    if g is not None:
        assert np.array_equal(tf.model.points, g[key + '_pts'])
        tf.wm, tf.Wc, tf.Wcc = g[key + '_wm'], g[key + '_Wc'], g[key + '_Wcc']
        tf.model.model_var = float(g[key + '_mv'])
        if tname.startswith('tpq'):
            tf.model.iK = g[key + '_iK']
            assert tf.model.nu == float(g[key + '_nu']) == 4.0
    return tf


# ---------------------------------------------------------------------------------------------------------------
def test_study_layout_transfers(amd):
    """ssmq_upload_planes / ssmq_download_planes: (n_elem..., T, B) host arrays <-> time-major planes [T][n_elem][ld],
    ragged B (zero-filled padding lanes), and a transfer that spans several staging chunks."""
    from ssmtoybox_amd import _lib
    rng = np.random.default_rng(5)
    for shape_elem, T, B in (((3,), 7, 100), ((2, 2), 5, 64), ((), 4, 1), ((6, 6), 6, 100000)):
        n = int(np.prod(shape_elem)) if shape_elem else 1
        ld = (B + 63) // 64 * 64
        arr = rng.standard_normal(tuple(shape_elem) + (T, B))
        d = _lib.DeviceBuffer(8 * T * n * ld)
        _lib.upload_study(arr, n, ld, d)
        planes = d.download((T, n, ld)) if T * n * ld < 5_000_000 else None
        if planes is not None:
            want = np.moveaxis(arr.reshape(n, T, B), 0, 1)                      # (T, n, B)
            assert np.array_equal(planes[:, :, :B], want) and not planes[:, :, B:].any()
        back = _lib.download_study(d, shape_elem, T, B, ld)
        assert back.shape == arr.shape and np.array_equal(back, arr)
        d.free()


def test_layout_roundtrip(amd):
    from ssmtoybox_amd import _lib
    rng = np.random.default_rng(0)
    for B, n in ((1, 1), (7, 3), (64, 36), (1000, 42), (4097, 78)):
        a = rng.standard_normal((B, n))
        s = _lib.SoA.from_host(a)
        assert np.array_equal(s.to_host(), a)
        planes = s.buf.download((n, s.ld))
        assert np.array_equal(planes[:, :B], a.T)


@pytest.mark.parametrize('name', sorted(MODELS))
def test_apply_golden(amd, golden, name):
    """apply() and apply_batch() against outputs of the reference's apply() on the same inputs and weights."""
    g = golden('g3_apply')
    fid, p, sidx, din, dout = MODELS[name]
    mod, f = make_model(name)
    means, covs, times = g[name + '_mean'], g[name + '_cov'], g[name + '_time']
    worst = 0.0
    for tname in SIGMA_TF + BQ_TF:
        key = '{}_{}'.format(name, tname)
        if key + '_mf' not in g:
            continue
        tf = make_transform(amd, tname, din, dout, g if tname in BQ_TF else None, key)
        ref = (g[key + '_mf'], g[key + '_cf'], g[key + '_cfx'])
        got = tf.apply_batch(f, means, covs, times.astype(float))
        for i in range(means.shape[0]):
            worst = max(worst, assert_moments_close([a[i] for a in got], [a[i] for a in ref], covs[i],
                                                    what=(key, i, tf.kernel_name(f))))
        # the drop-in single call (B = 1) returns fresh, writable arrays of the reference's shapes
        mf, cf, cfx = tf.apply(f, means[3], covs[3], np.atleast_1d(times[3]))
        assert mf.shape == (dout,) and cf.shape == (dout, dout) and cfx.shape == (dout, din)
        cf += 1.0
        assert_moments_close((mf, cf - 1.0, cfx), [a[3] for a in ref], covs[3], what=key)
    print('{}: worst scaled error {:.2e}'.format(name, worst))


@pytest.mark.parametrize('name', sorted(MODELS))
def test_apply_generic_kernel_matches(amd, golden, name):
    """The run-time-shape kernel (forced through an unusual state index / odd N) agrees with the oracle."""
    g = golden('g3_apply')
    fid, p, sidx, din, dout = MODELS[name]
    mod, f = make_model(name)
    means, covs, times = g[name + '_mean'], g[name + '_cov'], g[name + '_time']
    deg = 5 if din <= 3 else 3                   # N = 5^D (<= 125) or 3^D (81 ... 2187): no register-resident
    tf = amd.GaussHermiteTransform(din, deg)     # specialisation for D >= 2; 3^7 = 2187 points (the 7-input CTRS model) are
    pts, wm = orc.points_gh(din, deg), orc.weights_gh(din, deg)      # beyond the LDS-resident kernel: k_apply_big
    assert din <= 3 or tf.kernel_name(f) == ('k_apply_big' if din == 7 else 'k_apply_wide')
    got = tf.apply_batch(f, means, covs, times.astype(float))
    for i in range(means.shape[0]):
        ref = orc.apply_sigma(fid, means[i], covs[i], times[i], pts, wm, wm, p, sidx)
        assert_moments_close([a[i] for a in got], ref, covs[i], what=(name, i, tf.kernel_name(f)))


@pytest.mark.parametrize('kind,pstr,deg,name', [('gp', 'gh', 3, 'cv_dyn'), ('tp', 'fs', 5, 'ctrs_dyn'), ('bs', 'gh', 3, 'cv_dyn'),
                                                ('gp', 'gh', 3, 'ctrs_dyn')])
def test_blocked_matrix_core_route(amd, golden, monkeypatch, kind, pstr, deg, name):
    """BQ transforms on point sets beyond the wave kernels that have no instantiation of the fused matrix-core route
    (Gauss-Hermite degree 3 at D = 4: N = 81, at D = 7: N = 2187; fully-symmetric degree 5 at D = 7: N = 99): evaluation pass,
    T = FX [Wc | Wcc'] by column blocks of 256 on the matrix cores (and fx iK for the t-process), per-trajectory rest
    (k_apply_big) - against the oracle with the device's own weights, and against the LDS-resident workgroup kernel where the
    shape fits it."""
    monkeypatch.setenv('SSMQ_NO_BQ_STREAM', '1')       # (BQ shapes with a symmetric Wc would take k_bq_stream: its own test)
    if os.environ.get('SSMQ_NO_MFMA'):
        pytest.skip('the matrix-core routes are switched off in this run (tools/alt_paths.sh)')
    g = golden('g3_apply')
    fid, p, sidx, din, dout = MODELS[name]
    mod, f = make_model(name)
    means, covs, times = g[name + '_mean'], g[name + '_cov'], g[name + '_time']
    reps = 32                                             # 16 x 32 = 512 trajectories: beyond the route's minimum row count
    means, covs, times = np.tile(means, (reps, 1)), np.tile(covs, (reps, 1, 1)), np.tile(times, reps)
    par = np.array([[1.0] + [3.0] * din])
    mi = np.hstack((np.zeros((din, 1)), np.eye(din), 2 * np.eye(din))).astype(int)
    make = {'gp': lambda: amd.GaussianProcessTransform(din, dout, par, 'rbf', pstr, {'degree': deg}),
            'tp': lambda: amd.StudentTProcessTransform(din, dout, par, 'rbf', pstr, {'degree': deg}),
            'bs': lambda: amd.BayesSardTransform(din, dout, par, mi, pstr, {'degree': deg})}[kind]
    tf = make()
    N = tf.model.points.shape[1]
    assert N == (deg ** din if pstr == 'gh' else 2 * din * din + 1) and tf.kernel_name(f) == 'k_apply_big'
    got = tf.apply_batch(f, means, covs, times.astype(float), return_status=True)
    assert not got[3].any()
    w = dict(wm=tf.wm, Wc=tf.Wc, Wcc=tf.Wcc, model_var=tf.model.model_var, iK=getattr(tf.model, 'iK', None))
    worst = 0.0
    for i in range(0, 16, 3):
        ref = orc.apply_bq(fid, means[i], covs[i], times[i], tf.model.points, w, p, sidx, tp_nu=4.0 if kind == 'tp' else None)
        worst = max(worst, assert_moments_close([a[i] for a in got[:3]], ref, covs[i], what=(kind, name, i)))
    assert within(worst, 1e-10, 'blocked matrix-core route {} {} N={} vs oracle (scaled)'.format(kind, name, N))
    assert np.array_equal(got[1], got[1].transpose(0, 2, 1))
    assert np.array_equal(got[0][:16], got[0][16:32]) and np.array_equal(got[1][:16], got[1][-16:])     # tiled inputs, same outputs
    # the same transform with the integrand as an arbitrary Python callable (device sigma points -> host f -> device
    # reductions through the same blocked route)
    nb = 16 if N <= 1024 else 4
    host = tf.apply_batch(lambda x, par: orc.integrand(fid, x if sidx is None else x[list(sidx)], par[0], p), means[:nb], covs[:nb],
                          times[:nb].astype(float), fcn_pars=None)
    for a_, b_, what in zip(host, got[:3], ('mean', 'cov', 'ccov')):
        assert within(np.abs(a_ - b_[:nb]).max() / np.abs(b_[:nb]).max(), 1e-11, 'blocked route, host callable vs device integrand {} {} {}'.format(kind, name, what))
    if N <= 1024:
        monkeypatch.setenv('SSMQ_NO_MFMA', '1')
        tf2 = make()
        tf2.wm, tf2.Wc, tf2.Wcc = tf.wm, tf.Wc, tf.Wcc
        assert tf2.kernel_name(f) == 'k_apply_wide'        # SSMQ_NO_MFMA: no column blocks are built
        ref = tf2.apply_batch(f, means[:16], covs[:16], times[:16].astype(float))
        monkeypatch.delenv('SSMQ_NO_MFMA')
        for a_, b_, what in zip(got[:3], ref, ('mean', 'cov', 'ccov')):
            assert within(np.abs(a_[:16] - b_).max() / np.abs(b_).max(), 1e-11, 'blocked route vs workgroup kernel {} {} {}'.format(kind, name, what))


@pytest.mark.parametrize('n', [40, 1000])
def test_monte_carlo_transform(amd, golden, n):
    """MonteCarloTransform (mtran.py:62-94, the reference's baseline): unit points from np.random at construction, weights
    1 / n and 1 / (n - 1); on the device a centred rule (k_apply_tile for n <= 64, the streaming route beyond).  Against the
    oracle's centred moments on the transform's own points, and against a plain NumPy evaluation of the reference's lines."""
    g = golden('g3_apply')
    name = 'reentry_dyn'
    fid, p, sidx, din, dout = MODELS[name]
    mod, f = make_model(name)
    means, covs, times = g[name + '_mean'], g[name + '_cov'], g[name + '_time']
    np.random.seed(5)
    tf = amd.MonteCarloTransform(din, n)
    assert tf.unit_sp.shape == (din, n) and tf.kernel_name(f) in ('k_apply_tile', 'k_apply_wave', 'k_apply_wide', 'k_apply_big')
    got = tf.apply_batch(f, means, covs, times.astype(float))
    for i in range(0, means.shape[0], 5):
        ref = orc.apply_sigma(fid, means[i], covs[i], times[i], tf.unit_sp, tf.wm, np.diag(tf.Wc), p, sidx)
        assert_moments_close([a[i] for a in got], ref, covs[i], what=('mc', n, i))
        x = means[i][:, None] + np.linalg.cholesky(covs[i]).dot(tf.unit_sp)                      # mtran.py:79-91 as written
        fx = np.apply_along_axis(lambda c: orc.integrand(fid, c, times[i], p), 0, x)
        mf = (1.0 / n * fx).sum(axis=1)
        dfx = fx - mf[:, None]
        assert np.allclose(got[0][i], mf, rtol=1e-12) and np.allclose(got[1][i], 1.0 / (n - 1) * dfx.dot(dfx.T), rtol=1e-9, atol=1e-12)


def test_wave_kernel_matches_workgroup_kernel(amd, golden, monkeypatch):
    """Point sets of 9 ... 64 points without a register-resident specialisation run on k_apply_tile (every product on the
    matrix cores); SSMQ_NO_TILE=1 sends them to k_apply_wave (one wave per trajectory, lanes over output entries),
    SSMQ_NO_WAVE=1 to k_apply_wide (one workgroup per trajectory).  Same arithmetic up to the summation order inside the
    products: BQ, t-process and centred forms, sub-state measurement models, not-positive-definite inputs."""
    g = golden('g3_apply')
    cases = [('reentry_dyn', lambda d, e: amd.GaussianProcessTransform(d, e, np.array([[1.0] + [3.0] * d]), 'rbf', 'gh',
                                                                      {'degree': 2})),                     # N = 32
             ('reentry_dyn', lambda d, e: amd.StudentTProcessTransform(d, e, np.array([[1.0] + [3.0] * d]), 'rbf', 'fs',
                                                                       {'degree': 5})),                    # N = 51
             ('radar_meas', lambda d, e: amd.GaussHermiteTransform(d, 2)),                                  # N = 32, sub-state
             ('bearing_meas', lambda d, e: amd.BayesSardTransform(d, e, np.array([[1.0] + [3.0] * d]), 2, 'fs',
                                                                  {'degree': 5})),                          # N = 51, E = 4
             ('ct_dyn', lambda d, e: amd.FullySymmetricStudentTransform(d, 5)),                             # N = 51
             ('pend_dyn', lambda d, e: amd.GaussHermiteTransform(d, 7)),                                    # N = 49
             ('pend_dyn', lambda d, e: amd.GaussHermiteTransform(d, 4)),                                    # N = 16
             ('ungm_dyn', lambda d, e: amd.GaussianProcessTransform(d, e, np.array([[1.0, 3.0]]), 'rbf', 'gh',
                                                                    {'degree': 15}))]                       # D = 1, N = 15
    for name, make in cases:
        fid, p, sidx, din, dout = MODELS[name]
        mod, f = make_model(name)
        means, covs, times = g[name + '_mean'].copy(), g[name + '_cov'].copy(), g[name + '_time']
        covs[3] = -covs[3]                                  # one input that is not positive definite
        tf = make(din, dout)
        monkeypatch.delenv('SSMQ_NO_WAVE', raising=False)
        monkeypatch.delenv('SSMQ_NO_TILE', raising=False)
        assert tf.kernel_name(f) == 'k_apply_tile', tf.kernel_name(f)
        tile = tf.apply_batch(f, means, covs, times.astype(float), return_status=True)
        monkeypatch.setenv('SSMQ_NO_TILE', '1')
        assert tf.kernel_name(f) == 'k_apply_wave', tf.kernel_name(f)
        got = tf.apply_batch(f, means, covs, times.astype(float), return_status=True)
        monkeypatch.setenv('SSMQ_NO_WAVE', '1')
        assert tf.kernel_name(f) == 'k_apply_wide'
        ref = tf.apply_batch(f, means, covs, times.astype(float), return_status=True)
        monkeypatch.delenv('SSMQ_NO_WAVE')
        monkeypatch.delenv('SSMQ_NO_TILE')
        for res, kern, bar in ((got, 'wave', 1e-13), (tile, 'tile', 1e-12)):
            assert np.array_equal(res[3], ref[3]) and res[3][3] != 0 and not res[3][:3].any()
            ok = ref[3] == 0
            assert np.isnan(res[0][3]).all() and np.isnan(res[1][3]).all() and np.isnan(res[2][3]).all()
            for a_, b_, what in zip(res[:3], ref[:3], ('mean', 'cov', 'ccov')):
                sc = np.abs(b_[ok]).max()
                if kern == 'tile' and what == 'ccov' and isinstance(tf, amd.SigmaPointTransform):
                    # the centred rules form x_n - m from x_n = m + L xi_n (mtran.py:145-148), rounded at eps |m| (the radar
                    # model: m = 6500, L xi = 1e-3); the tile kernel multiplies by L xi_n itself - closer to the exact value
                    bar = 1e-10
                assert within(np.abs(a_[ok] - b_[ok]).max() / sc, bar, '{} {} {} vs workgroup {}'.format(
                    name, type(tf).__name__, kern, what))
            if kern == 'tile':          # formed for e2 <= e1 and mirrored: exactly symmetric
                assert np.array_equal(res[1][ok], res[1][ok].transpose(0, 2, 1))


def test_apply_python_callable(amd, golden):
    """Arbitrary Python integrand: device sigma points, host f, device reductions (bq/bqmtran.py:97-107 split)."""
    g = golden('g3_apply')
    name = 'reentry_dyn'
    fid, p, sidx, din, dout = MODELS[name]
    means, covs, times = g[name + '_mean'], g[name + '_cov'], g[name + '_time']

    def f(x, par):
        return orc.integrand(fid, x, par[0], p)      # a host callable the library knows nothing about
    for tname in ('ut', 'gpq', 'tpq'):
        key = '{}_{}'.format(name, tname)
        tf = make_transform(amd, tname, din, dout, g if tname in BQ_TF else None, key)
        for i in (0, 5):
            got = tf.apply(f, means[i], covs[i], np.atleast_1d(times[i]))
            ref = (g[key + '_mf'][i], g[key + '_cf'][i], g[key + '_cfx'][i])
            assert_moments_close(got, ref, covs[i], what=(key, i))


def test_reference_variance_sign_tests(amd):
    """tests/test_bqmtran.py:48-64 of the reference: model and integral variance stay non-negative for "numerically
    unpleasant settings" - and equal the oracle's values there."""
    ker_par = np.array([[1.0, 3.0, 3.0]])
    tf = amd.GaussianProcessTransform(2, 1, ker_par, point_str='sr')
    pts = orc.points_sr(2)
    emv = tf.model.exp_model_variance(ker_par)
    assert emv >= 0 and abs(emv - orc.gp_weights(ker_par, pts)['model_var']) < 1e-12
    for par in ([1, 600, 6], [1.1, 600, 6]):
        ivar = tf.model.integral_variance(par)
        ref = orc.gp_weights(np.array([par], dtype=float), pts)['integral_var']
        assert ivar >= 0 and abs(ivar - ref) < 1e-9 * max(1.0, abs(ref)), par


def test_reference_quadratic_form_routes(amd):
    """tests/test_mult_dot_einsum.py:56-105 of the reference: Y iK Q iK Y' of the 5-D reentry integrand by plain products
    and by the Cholesky-whitened route agree; here additionally with what the device kernel forms (cov + m m' - emv I)."""
    from ssmtoybox_amd import ssmod as sm
    mean_in = np.array([6500.4, 349.14, 1.8093, 6.7967, 0.6932])
    cov_in = np.diag([1e-6, 1e-6, 1e-6, 1e-6, 1])
    model = sm.ReentryVehicle2DTransition(sm.GaussRV(5, mean_in, cov_in), sm.GaussRV(3))
    ker_par = np.hstack((np.ones((1, 1)), 25 * np.ones((1, 5))))
    tf = amd.GaussianProcessTransform(5, 5, ker_par, point_str='sr')
    x = mean_in[:, None] + np.linalg.cholesky(cov_in).dot(tf.model.points)
    Y = np.stack([orc.integrand(orc.F_REENTRY2D_DYN, x[:, n], 1.0, (0.1,)) for n in range(x.shape[1])], axis=1)
    iK, Q = tf.model.iK, tf.model.Q
    C1 = Y.dot(iK.dot(Q).dot(iK)).dot(Y.T)
    C2 = np.einsum('ab,bc,cd', Y, np.einsum('ab,bc,cd', iK, Q, iK), Y.T)
    assert np.allclose(C1, C2)
    K = orc.rbf_eval(ker_par, tf.model.points) + 1e-8 * np.eye(Q.shape[0])
    bet = np.linalg.solve(np.linalg.cholesky(K), Y.T).T.dot(np.linalg.solve(np.linalg.cholesky(K), np.linalg.cholesky(Q)))
    C3 = bet.dot(bet.T)
    assert np.allclose(C1, C3, rtol=1e-5)
    mf, cf, _ = tf.apply(model.dyn_eval, mean_in, cov_in, np.atleast_1d(1.0))
    C_dev = cf + np.outer(mf, mf) - tf.model.model_var * np.eye(5)
    assert np.abs(C_dev - C1).max() < 1e-9 * np.abs(C1).max()


def test_reference_property_tests(amd):
    """The reference's own assertions on apply() (tests/test_bqmtran.py:66-104): GPQ on UNGM and pendulum at the
    standard normal with time 1.0 gives a symmetric positive-definite covariance and I_out of shape (dim, dim); the
    Bayes-Sard transform of polar -> cartesian (a Python callable) gives a positive-definite covariance."""
    from ssmtoybox_amd import ssmod as sm
    models = [sm.UNGMTransition(sm.GaussRV(1), sm.GaussRV(1, cov=np.array([[10.0]]))),
              sm.Pendulum2DTransition(sm.GaussRV(2), sm.GaussRV(2), 0.01)]
    for mod in models:
        dim = mod.dim_in
        ker_par = np.hstack((np.ones((1, 1)), 3 * np.ones((1, dim))))
        tf = amd.GaussianProcessTransform(dim, dim, ker_par)
        tmean, tcov, tccov = tf.apply(mod.dyn_eval, np.zeros(dim), np.eye(dim), np.atleast_1d(1.0))
        assert tf.I_out.shape == (dim, dim) and tmean.shape == (dim,) and tccov.shape == (dim, dim)
        np.linalg.cholesky(tcov)
        assert np.allclose(tcov, tcov.T)
        tcov += 1.0                                        # outputs are fresh, writable arrays (ssinf.py:279 does +=)

    def polar2cartesian(x, pars):
        return x[0] * np.array([np.cos(x[1]), np.sin(x[1])])
    alpha_ut = np.array([[0, 1, 0, 2, 0], [0, 0, 1, 0, 2]])
    mt = amd.BayesSardTransform(2, 2, np.array([[1.0, 1, 1]]), multi_ind=alpha_ut, point_str='ut')
    mean_out, cov_out, cc = mt.apply(polar2cartesian, np.array([1, np.pi / 2]), np.diag([0.05 ** 2, (np.pi / 10) ** 2]),
                                     np.atleast_1d(0))
    assert mt.I_out.shape == (2, 2)
    np.linalg.cholesky(cov_out)
    assert abs(mean_out[0]) < 1e-12 and 0.9 < mean_out[1] < 1.0      # E[r sin(th)] a little below 1


def test_integration_md_binding_runs(amd):
    """The reference-side binding printed in INTEGRATION.md (sections 1-2) is executed as written - only the import of
    the reference's ABC and the library path are redirected, since the reference does not travel to the GPU box - and its
    apply() is compared with the package's own transform on UNGM."""
    import re
    from ssmtoybox_amd import ssmod as sm, _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, 'INTEGRATION.md')).read()
    blocks = re.findall(r'```python\n(.*?)```', text, flags=re.S)
    stub = blocks[0]
    assert 'class HipGaussianProcessTransform' in stub and "ctypes.CDLL('libssmq.so')" in stub
    stub = stub.replace('from ssmtoybox.mtran import MomentTransform', 'from ssmtoybox_amd.mtran import MomentTransform')
    stub = stub.replace("ctypes.CDLL('libssmq.so')", 'ctypes.CDLL({!r})'.format(_lib.library_path()))
    ns = {}
    exec(compile(stub, 'INTEGRATION.md#1', 'exec'), ns)
    helper = re.search(r'def _integrand\(fid, par=\(\), idx=\(\)\):.*?return s\n', blocks[1], flags=re.S).group(0)
    exec(compile(helper, 'INTEGRATION.md#2', 'exec'), ns)

    class Model:                                   # what section 2 attaches to the reference's model classes
        ssmq_integrand = ns['_integrand'](1)       # SSMQ_F_UNGM_DYN

        def dyn_eval(self, x, t, dx=False):
            raise AssertionError('the device evaluates the integrand')
    par = np.array([[1.0, 3.0]])
    pts = amd.UnscentedTransform.unit_sigma_points(1)
    tf = ns['HipGaussianProcessTransform'](1, 1, par, pts)
    ours = amd.GaussianProcessTransform(1, 1, par)
    assert np.allclose(tf.wm, ours.wm, rtol=1e-13) and np.allclose(tf.Wc, ours.Wc, rtol=1e-12, atol=1e-15)
    dyn = sm.UNGMTransition(sm.GaussRV(1), sm.GaussRV(1, cov=np.array([[10.0]])))
    for mean, cov, t in ((0.3, 1.7, 4.0), (-2.0, 0.4, 11.0)):
        got = tf.apply(Model().dyn_eval, np.array([mean]), np.array([[cov]]), np.atleast_1d(t))
        ref = ours.apply(dyn.dyn_eval, np.array([mean]), np.array([[cov]]), np.atleast_1d(t))
        for a, b in zip(got, ref):
            assert a.shape == b.shape and np.allclose(a, b, rtol=1e-13, atol=1e-15)
    with pytest.raises(np.linalg.LinAlgError):
        tf.apply(Model().dyn_eval, np.zeros(1), -np.eye(1), np.atleast_1d(0.0))


def test_not_positive_definite(amd):
    from ssmtoybox_amd import ssmod as sm
    tf = amd.UnscentedTransform(2)
    f = sm.Pendulum2DTransition().dyn_eval
    bad = np.array([[1.0, 2.0], [2.0, 1.0]])
    with pytest.raises(np.linalg.LinAlgError):
        tf.apply(f, np.zeros(2), bad, np.atleast_1d(0))
    covs = np.stack([np.eye(2), bad, np.eye(2), -np.eye(2)])
    mf, cf, cfx, st = tf.apply_batch(f, np.zeros((4, 2)), covs, 0.0, return_status=True)
    assert list(st) == [0, 1, 0, 1]
    assert np.all(np.isfinite(mf[[0, 2]])) and np.all(np.isnan(mf[[1, 3]])) and np.all(np.isnan(cf[1]))
    with pytest.raises(np.linalg.LinAlgError):
        tf.apply_batch(f, np.zeros((4, 2)), covs, 0.0)
    # empty batch
    mf, cf, cfx = tf.apply_batch(f, np.zeros((0, 2)), np.zeros((0, 2, 2)), 0.0)
    assert mf.shape == (0, 2) and cf.shape == (0, 2, 2)


# ---------------------------------------------------------------------------------------------------------------
# weights
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', GP_CASES, ids=[c[0] for c in GP_CASES])
def test_gp_weights_golden(amd, golden, case):
    from ssmtoybox_amd.bq.bqkern import device_gp_weights
    g = golden('g2_gp_weights')
    tag, dim, ell, pstr, ppar = case
    for aniso, alpha in ((False, 1.0), (True, 1.7)):
        t = 'gp_' + tag + ('_aniso' if aniso else '')
        if t + '_par' not in g:
            continue
        par = gp_par(dim, ell, alpha, aniso)
        tf = amd.GaussianProcessTransform(dim, dim, par, 'rbf', pstr, ppar)
        assert np.array_equal(tf.model.points, g[t + '_pts'])
        cond = float(g[t + '_cond'])
        tol1 = max(RTOL, 64 * cond * 2.2e-16)          # one application of K^-1
        tol2 = max(RTOL, 8 * cond ** 2 * 2.2e-16)      # two (Wc = iK Q iK, variances)
        assert rel_err(tf.model.q, g[t + '_q']) < 1e-13
        assert rel_err(tf.model.Q, g[t + '_Q']) < 1e-13
        assert rel_err(tf.model.R, g[t + '_R']) < 1e-13
        def chk(value, bar, what):          # worst-case conditioning bar, capped by what earlier rounds measured
            what = t + ' ' + what
            return within(value, capped(bar, what), what)
        assert chk(rel_err(tf.model.iK, g[t + '_iK']), tol1, 'iK')
        assert chk(rel_err(tf.wm, g[t + '_wm']), tol1, 'wm')
        assert chk(rel_err(tf.Wcc, g[t + '_Wcc']), tol1, 'Wcc')
        assert chk(rel_err(tf.Wc, g[t + '_Wc']), tol2, 'Wc')
        assert np.array_equal(tf.Wc, tf.Wc.T)
        assert chk(abs(tf.model.model_var - g[t + '_mv']) / max(1.0, abs(float(g[t + '_mv']))), tol2, 'model_var')
        assert chk(abs(tf.model.integral_var - g[t + '_iv']), tol2, 'integral_var')
        # theta-batched: every row of a (P, 1 + D) parameter matrix gets its own workgroup
        pars = np.vstack([par, gp_par(dim, ell * 1.5, 1.0, aniso), par])
        w = device_gp_weights(tf.model.points, pars)
        assert np.array_equal(w['wm'][0], tf.wm) and np.array_equal(w['wm'][2], tf.wm)
        assert np.array_equal(w['Wc'][0], tf.Wc) and not np.array_equal(w['wm'][1], tf.wm)


@pytest.mark.parametrize('case', [c for c in GP_CASES if c[1] <= 6], ids=[c[0] for c in GP_CASES if c[1] <= 6])
def test_rbf_kernel_methods_golden(amd, golden, case):
    """Row a9 / a10 of the path as callables: RBFGauss.eval (two point sets, diag), eval_chol, eval_inv_dot (scaling, right-
    hand side), exp_x_kxkx with two different parameter rows, exp_x_kx with scaling, GP exp_model_variance with
    alpha != 1 - device results against the reference's (the reference pins eval against a naive double loop with
    array_equal, ssmtoybox/tests/test_bqkern.py:23-56; two libms are not bit-compatible, so the bar here is a few ulp
    and the measured maximum is recorded)."""
    g = golden('g2_gp_weights')
    tag, dim, ell, pstr, ppar = case
    for aniso, alpha in ((False, 1.0), (True, 1.7)):
        t = 'gp_' + tag + ('_aniso' if aniso else '')
        par, x = g[t + '_par'], g[t + '_pts']
        tf = amd.GaussianProcessTransform(dim, dim, par, 'rbf', pstr, ppar)
        k = tf.model.kernel
        cond, conds = float(g[t + '_cond']), float(g[t + '_conds'])
        K, Ks = k.eval(par, x, scaling=False), k.eval(par, x)
        ulp = max(np.max(np.abs(K - g[t + '_K']) / np.spacing(g[t + '_K'])), np.max(np.abs(Ks - g[t + '_Ks']) / np.spacing(g[t + '_Ks'])))
        assert within(ulp, 16.5, t + ' RBFGauss.eval vs reference (ulp)')      # measured: at most 8
        assert np.array_equal(K, K.T) and np.all(np.diag(K) == 1.0)
        assert rel_err(k.eval(par, x, g[t + '_x2']), g[t + '_K12']) < 1e-14
        assert rel_err(k.eval(par, x, 0.5 * x + 0.2, diag=True), g[t + '_Kdiag']) < 1e-14
        assert within(rel_err(k.eval_chol(par, x, scaling=False), g[t + '_L']), capped(max(1e-13, 64 * cond * 2.2e-16), t + ' eval_chol'), t + ' eval_chol')
        assert within(rel_err(k.eval_chol(par, x), g[t + '_Ls']), capped(max(1e-13, 64 * conds * 2.2e-16), t + ' eval_chol scaled'), t + ' eval_chol scaled')
        L = k.eval_chol(par, x)
        assert np.array_equal(L, np.tril(L))
        assert within(rel_err(k.eval_inv_dot(par, x), g[t + '_iKs']), capped(max(1e-13, 64 * conds * 2.2e-16), t + ' eval_inv_dot scaled'), t + ' eval_inv_dot scaled')
        assert within(rel_err(k.eval_inv_dot(par, x, scaling=False), g[t + '_iK']), capped(max(1e-13, 64 * cond * 2.2e-16), t + ' eval_inv_dot'), t + ' eval_inv_dot')
        assert np.array_equal(k.eval_inv_dot(par, x, scaling=False), tf.model.iK)      # the inverse the weights were made with
        assert within(rel_err(k.eval_inv_dot(par, x, g[t + '_b'], scaling=False), g[t + '_iKb']),
                      capped(max(1e-13, 64 * cond * 2.2e-16), t + ' eval_inv_dot rhs'), t + ' eval_inv_dot rhs')
        with pytest.raises(ValueError):
            k.eval_inv_dot(par, x, np.ones((x.shape[1], 2)))
        par2 = g[t + '_par2']
        assert rel_err(k.exp_x_kxkx(par, par2, x), g[t + '_Q01']) < 1e-13
        assert rel_err(k.exp_x_kxkx(par, par2, x, scaling=True), g[t + '_Q01s']) < 1e-13
        assert rel_err(k.exp_x_kxkx(par, par, x, scaling=True), g[t + '_Qs']) < 1e-13
        assert rel_err(k.exp_x_kxkx(par, par, x), g[t + '_Q']) < 1e-13
        assert rel_err(k.exp_x_kx(par, x, scaling=True), g[t + '_qs']) < 1e-13
        tol2 = max(1e-10, 8 * conds ** 2 * 2.2e-16)
        emv = float(g[t + '_emv_call'])
        assert within(abs(tf.model.exp_model_variance(par) - emv) / max(1.0, abs(emv)),
                      capped(tol2, t + ' exp_model_variance(par)'), t + ' exp_model_variance(par)')
        assert within(abs(tf.model.integral_variance(par) - float(g[t + '_ivar_call'])),
                      capped(max(1e-10, 8 * cond ** 2 * 2.2e-16), t + ' integral_variance(par)'), t + ' integral_variance(par)')


# ---------------------------------------------------------------------------------------------------------------
# weights and transforms on LARGE point sets (202 <= N): the reference's values on injected sets (golden g12)
# ---------------------------------------------------------------------------------------------------------------
G12_CASES = [('d6_gh3_l15', 'gh', {'degree': 3}), ('d10_fs7_l1', 'fs', {'degree': 7}), ('d10_fs7_l3', 'fs', {'degree': 7})]


def _digest_err(g, key, a):
    from tests.test_oracle_golden import digest_err
    return digest_err(g, key, a)


def _full_from_tril(v, n):
    full = np.zeros((n, n))
    full[np.tril_indices(n)] = v
    return full + np.tril(full, -1).T


@pytest.mark.parametrize('case', G12_CASES, ids=[c[0] for c in G12_CASES])
def test_large_set_weights_golden(amd, golden, case):
    """Quadrature weights above N = 201 (the tiled stage-2 route of k_weights<1024>): GP and Bayes-Sard (total degree <=
    2) on the Gauss-Hermite degree-3 grid at D = 6 (N = 729) and on this build's degree-7 rule at D = 10 (N = 1181, BASELINE
    configs[4] as worded), against the REFERENCE's weights on the same (injected) point sets - full vectors, and for the
    (N, N) matrices the committed digest (diagonal, 24 rows, 6 probe products, Frobenius norm).  Bars: cond-scaled with the
    stored condition numbers, as for the small sets."""
    g = golden('g12_large_weights')
    tag, pstr, ppar = case
    pts, par, mi = g[tag + '_pts'], g[tag + '_par'], g[tag + '_mi']
    dim, N = pts.shape
    eps = 2.2e-16
    tf = amd.GaussianProcessTransform(dim, dim, par, 'rbf', pstr, ppar)
    assert np.array_equal(tf.model.points, pts)          # the rule the fixture was made on IS the one the build generates
    cond = float(g['gp_' + tag + '_cond'])
    tol1, tol2 = max(RTOL, 64 * cond * eps), max(RTOL, 8 * cond ** 2 * eps)
    t = 'g12 gp ' + tag + ' '
    assert rel_err(tf.model.q, g['gp_' + tag + '_q']) < 1e-13
    assert within(_digest_err(g, 'gp_' + tag + '_Q', tf.model.Q), 1e-13, t + 'Q')
    assert within(_digest_err(g, 'gp_' + tag + '_K', tf.model.kernel.eval(par, pts, scaling=False)), 1e-13, t + 'K')
    assert within(_digest_err(g, 'gp_' + tag + '_iK', tf.model.iK), tol1, t + 'iK')
    assert within(rel_err(tf.wm, g['gp_' + tag + '_wm']), tol1, t + 'wm')
    assert within(rel_err(tf.Wcc, g['gp_' + tag + '_Wcc']), tol1, t + 'Wcc')
    assert within(_digest_err(g, 'gp_' + tag + '_Wc', tf.Wc), tol2, t + 'Wc')
    assert np.array_equal(tf.Wc, tf.Wc.T)
    assert within(abs(tf.model.model_var - float(g['gp_' + tag + '_mv'])), tol2, t + 'model_var')
    assert within(abs(tf.model.integral_var - float(g['gp_' + tag + '_iv'])), tol2, t + 'integral_var')
    # Bayes-Sard, general case (66 / 28 basis functions < N)
    tb = amd.BayesSardTransform(dim, dim, par, mi, pstr, ppar)
    cK, cVKV = float(g['bs_' + tag + '_condK']), float(g['bs_' + tag + '_condVKV'])
    tolb = max(1e-12, 64 * max(cK, cVKV) * eps)
    tolb2 = max(1e-12, 8 * max(cK, cVKV) ** 2 * eps)      # Wc = iK (Q - A B A') iK: K^-1 twice (bq/bqmod.py:976)
    t = 'g12 bs ' + tag + ' '
    assert within(rel_err(tb.model._exp_x_kxpx(par, mi, pts), g['bs_' + tag + '_kxpx']), 1e-13, t + 'kxpx')
    assert within(rel_err(tb.wm, g['bs_' + tag + '_wm']), tolb, t + 'wm')
    assert within(rel_err(tb.Wcc, g['bs_' + tag + '_Wcc']), tolb, t + 'Wcc')
    assert within(_digest_err(g, 'bs_' + tag + '_Wc', tb.Wc), capped(tolb2, t + 'Wc'), t + 'Wc')
    assert np.array_equal(tb.Wc, tb.Wc.T)
    if 'bs_' + tag + '_Wc_tril' in g:
        assert within(rel_err(tb.Wc, _full_from_tril(g['bs_' + tag + '_Wc_tril'], N)), capped(tolb2, t + 'Wc (every entry)'), t + 'Wc (every entry)')
    assert within(abs(tb.model.model_var - float(g['bs_' + tag + '_mv'])), tolb, t + 'model_var')
    assert within(abs(tb.model.integral_var - float(g['bs_' + tag + '_iv'])), tolb, t + 'integral_var')
    # apply() with the build's OWN large-set weights against the reference's apply() with ITS weights (6 inputs each)
    if os.environ.get('SSMQ_NO_MFMA') and N > 1000:
        return      # tools/alt_paths.sh: 1181 points at D = 10 have no route without the matrix cores (the LDS image of the generic kernel)
    h = dim // 2

    def f(x, par_):
        return np.concatenate((np.sin(x[:h]) + x[h:2 * h] ** 2, x[h:2 * h] * np.cos(x[:h])))
    for kind, tr, bar in (('gp', tf, max(RTOL, tol2)), ('bs', tb, max(RTOL, tolb2))):
        worst = 0.0
        for i in range(g[tag + '_apply_mean'].shape[0]):
            mean, cov = g[tag + '_apply_mean'][i], g[tag + '_apply_cov'][i]
            got = tr.apply(f, mean, cov, np.atleast_1d(0))
            ref = (g[kind + '_' + tag + '_apply_mf'][i], g[kind + '_' + tag + '_apply_cf'][i], g[kind + '_' + tag + '_apply_cfx'][i])
            worst = max(worst, assert_moments_close(got, ref, cov, rtol=bar, what=(kind, tag, i)))
        assert within(worst, bar, 'g12 {} {} apply() with own weights vs the reference (scaled)'.format(kind, tag))


def test_config4_as_worded_degree7_full_batch(amd, golden):
    """BASELINE configs[4] AS WORDED: Bayes-Sard transform, D = E = 10, fully-symmetric degree-7 rule (N = 1181), B = 1e4
    on the device integrand, with the REFERENCE's weights injected (golden g12: the reference's bq_weights on this point
    set, every entry of Wc).  128 sampled trajectories against the oracle with the same weights, the reference's own
    apply() outputs for the 6 committed inputs, exact symmetry, batch-permutation invariance bit for bit."""
    from ssmtoybox_amd import ssmod as sm
    g = golden('g12_large_weights')
    tag = 'd10_fs7_l3'
    pts, par, mi = g[tag + '_pts'], g[tag + '_par'], g[tag + '_mi']
    N = pts.shape[1]
    B = 10000
    rng = np.random.default_rng(177)
    means = rng.standard_normal((B, 10))
    a = rng.standard_normal((B, 10, 10)) / np.sqrt(10)
    covs = np.einsum('bij,bkj->bik', a, a) + 0.1 * np.eye(10)
    n_ref = g[tag + '_apply_mean'].shape[0]
    means[:n_ref], covs[:n_ref] = g[tag + '_apply_mean'], g[tag + '_apply_cov']
    tf = amd.BayesSardTransform(10, 10, par, mi, 'fs', {'degree': 7})
    assert np.array_equal(tf.model.points, pts)
    w = dict(wm=g['bs_' + tag + '_wm'], Wc=_full_from_tril(g['bs_' + tag + '_Wc_tril'], N), Wcc=g['bs_' + tag + '_Wcc'],
             model_var=float(g['bs_' + tag + '_mv']))
    tf.wm, tf.Wc, tf.Wcc, tf.model.model_var = w['wm'], w['Wc'], w['Wcc'], w['model_var']
    f = sm.Smooth10DTransition().dyn_eval
    if not (os.environ.get('SSMQ_NO_MFMA') or os.environ.get('SSMQ_NO_BQ_STREAM')):
        assert tf.kernel_name(f) == 'k_bq_stream'           # one launch, the point axis tiled (ssmq_bq_stream.hip)
    mf, cf, cfx, st = tf.apply_batch(f, means, covs, 0.0, return_status=True)
    assert not st.any() and np.all(np.isfinite(mf)) and np.all(np.isfinite(cf)) and np.all(np.isfinite(cfx))
    assert np.array_equal(cf, cf.transpose(0, 2, 1))
    worst = 0.0
    for i in range(n_ref):
        ref = (g['bs_' + tag + '_apply_mf'][i], g['bs_' + tag + '_apply_cf'][i], g['bs_' + tag + '_apply_cfx'][i])
        worst = max(worst, assert_moments_close((mf[i], cf[i], cfx[i]), ref, covs[i], what=('reference apply', i)))
    assert within(worst, 1e-10, 'configs[4] as worded: device transform vs the REFERENCE apply() (6 inputs, scaled)')
    worst = 0.0
    for i in np.random.default_rng(178).choice(B, 128, replace=False):
        ref = orc.apply_bq(orc.F_SMOOTH10D_DYN, means[i], covs[i], 0.0, pts, w)
        worst = max(worst, assert_moments_close((mf[i], cf[i], cfx[i]), ref, covs[i], what=(tag, i)))
    assert within(worst, 1e-10, 'configs[4] as worded (degree 7, N=1181, B=1e4) device transform vs oracle (128 samples, scaled)')
    perm = np.random.default_rng(179).permutation(B)[:1024]
    mf2, cf2, cfx2 = tf.apply_batch(f, means[perm], covs[perm], 0.0)
    assert np.array_equal(mf2, mf[perm]) and np.array_equal(cf2, cf[perm]) and np.array_equal(cfx2, cfx[perm])
    # the same batch with the build's OWN weights: differs by what the weights' conditioning allows
    tf2 = amd.BayesSardTransform(10, 10, par, mi, 'fs', {'degree': 7})
    mf3, cf3, cfx3 = tf2.apply_batch(f, means[:256], covs[:256], 0.0)
    eps = 2.2e-16
    bar = max(1e-10, 64 * max(float(g['bs_' + tag + '_condK']), float(g['bs_' + tag + '_condVKV'])) * eps)
    worst = 0.0
    for i in range(256):
        worst = max(worst, assert_moments_close((mf3[i], cf3[i], cfx3[i]), (mf[i], cf[i], cfx[i]), covs[i], rtol=bar, what=('own weights', i)))
    assert within(worst, bar, 'configs[4] as worded: own weights vs reference weights, 256 transforms (scaled)')


def test_gp_weights_scaling_invariance(amd):
    # tests/test_bqmtran.py:40-46 of the reference: exact equality
    tf = amd.GaussianProcessTransform(3, 3, np.array([[1.0, 3.0, 3.0, 3.0]]))
    wm, wc, wcc = tf.weights(np.array([[50.0, 3.0, 3.0, 3.0]]))
    assert np.array_equal(wm, tf.wm) and np.array_equal(wc, tf.Wc) and np.array_equal(wcc, tf.Wcc)


@pytest.mark.parametrize('case', BS_CASES, ids=[c[0] for c in BS_CASES])
def test_bs_weights_golden(amd, golden, case):
    """Bayes-Sard weights against the reference, to what their conditioning allows (the condition numbers are stored with
    the fixture).  Unisolvent sets (as many basis functions as points): the kernel drops out, wm = V^-T px, Wc =
    V^-T pxpx V^-1 (bq/bqmod.py:952-961) - an LU solve with V: cond(V) eps, twice for Wc.  General case: K^-1 and
    (V' K^-1 V + 1e-8 I)^-1 both enter (:963-982)."""
    g = golden('g2_bs_weights')
    tag, dim, pstr, ppar, mi, ell = case
    t = 'bs_' + tag
    par = gp_par(dim, ell)
    mi = g[t + '_mi']
    tf = amd.BayesSardTransform(dim, dim, par, mi, pstr, ppar)
    assert np.array_equal(tf.model.points, g[t + '_pts'])
    eps = 2.2e-16
    cK, cV, cVKV = float(g[t + '_condK']), float(g[t + '_condV']), float(g[t + '_condVKV'])
    uni = mi.shape[1] == tf.model.points.shape[1]
    k1 = cV if uni else max(cK, cVKV)        # one pass through the worse-conditioned solve
    tol1 = max(1e-12, 64 * k1 * eps)         # unisolvent cases: 1e-12 (measured <= 4e-16); general: <= 8.3e-11 (measured <= 2.3e-12)
    tol2 = max(1e-12, 64 * (cV ** 2 if uni else max(cK, cVKV)) * eps)
    assert within(rel_err(tf.wm, g[t + '_wm']), tol1, t + ' wm')
    assert within(rel_err(tf.Wcc, g[t + '_Wcc']), tol1, t + ' Wcc')
    assert within(rel_err(tf.Wc, g[t + '_Wc']), tol2, t + ' Wc')
    # the variances always involve the kernel (:958-961, 984-988): differences of O(1) terms
    tolv = max(1e-12, 64 * (cK if uni else max(cK, cVKV)) * eps)
    assert within(abs(tf.model.model_var - g[t + '_mv']), tolv, t + ' model_var')
    assert within(abs(tf.model.integral_var - g[t + '_iv']), tolv, t + ' integral_var')


def test_variance_sweeps_golden(amd, golden):
    """Length-scale sweeps (research/bsq/bsq_ungm.py:244-282): the whole grid in ONE theta-batched launch, against the
    reference's exp_model_variance / integral_variance values."""
    g = golden('g9_sweeps')
    ls, ls2 = g['ls'], g['ls2']
    tf = amd.BayesSardTransform(1, 1, np.array([[1.0, 1.0]]), np.array([[0, 1, 2]]), 'ut')
    pars = np.column_stack((np.ones(ls.size), ls))
    emv, ivar = tf.model.exp_model_variance_batch(pars), tf.model.integral_variance_batch(pars)
    # the long end of the sweep has cond(K) ~ 1 / jitter = 1e8: absolute agreement at the kernel's unit scale
    assert np.abs(emv - g['bs1_emv']).max() < 2e-8 and np.abs(ivar - g['bs1_ivar']).max() < 2e-8
    short = ls < 3.0
    assert np.abs(emv - g['bs1_emv'])[short].max() < 1e-12
    assert abs(tf.model.exp_model_variance(np.array([[1.0, ls[3]]])) - g['bs1_emv'][3]) < 1e-12
    assert abs(tf.model.integral_variance(np.array([[1.0, ls[3]]])) - g['bs1_ivar'][3]) < 1e-12
    grid = np.array([[1.0, a, b] for a in ls2 for b in ls2])
    for tag in ('bs2', 'bs3'):
        tf = amd.BayesSardTransform(2, 1, np.array([[1.0, 1.0, 1.0]]), g[tag + '_mi'], 'ut')
        emv = tf.model.exp_model_variance_batch(grid).reshape(ls2.size, ls2.size)
        assert np.abs(emv - g[tag + '_emv']).max() < 2e-8, tag
        assert np.abs(emv - g[tag + '_emv'])[:4, :4].max() < 1e-11, tag
    iv = tf.model.integral_variance_batch(grid).reshape(ls2.size, ls2.size)
    assert np.abs(iv - g['bs3_ivar']).max() < 2e-8
    tg = amd.GaussianProcessTransform(2, 1, np.array([[1.0, 1.0, 1.0]]), 'rbf', 'ut')
    w = tg.model.bq_weights_batch(grid)
    assert np.abs(w['model_var'].reshape(ls2.size, -1) - g['gp2_emv']).max() < 2e-8
    assert np.abs(w['integral_var'].reshape(ls2.size, -1) - g['gp2_ivar']).max() < 2e-8
    # a 100 x 100 grid as in the reference's 2-D demo: 1e4 parameter rows, one launch, all finite and in range
    big = np.logspace(-1, 1, 100)
    grid = np.array([[1.0, a, b] for a in big for b in big])
    tf = amd.BayesSardTransform(2, 1, np.array([[1.0, 1.0, 1.0]]), g['bs2_mi'], 'ut')
    emv = tf.model.exp_model_variance_batch(grid)
    assert emv.shape == (10000,) and np.all(np.isfinite(emv)) and emv.max() < 4.0 and emv.min() > -1e-6


def test_bs_reproduces_classical_rules(amd):
    # the reference's known-answer tests (tests/test_bqmod.py:368-459) on the device path
    one = np.array([[1.0, 1.0]])
    tf = amd.BayesSardTransform(1, 1, one, np.array([[0, 1, 2]]), 'ut')
    assert np.allclose(tf.wm, amd.UnscentedTransform.weights(1)[0])
    tf = amd.BayesSardTransform(1, 1, one, np.array([[0, 1, 2, 3, 4]]), 'gh', {'degree': 5})
    assert np.allclose(tf.wm, amd.GaussHermiteTransform.weights(1, 5))
    two = np.array([[1.0, 1.0, 1.0]])
    tf = amd.BayesSardTransform(2, 2, two, np.array([[0, 1, 0, 2, 0], [0, 0, 1, 0, 2]]), 'ut')
    assert np.allclose(tf.wm, amd.UnscentedTransform.weights(2)[0])
    mi = np.array([[0, 1, 0, 1, 2, 0, 1, 2, 2], [0, 0, 1, 1, 0, 2, 2, 1, 2]])
    tf = amd.BayesSardTransform(2, 2, two, mi, 'gh', {'degree': 3})
    assert np.allclose(tf.wm, amd.GaussHermiteTransform.weights(2, 3))
    assert tf.model.model_var >= 0 and tf.model.integral_var >= 0
    np.linalg.cholesky(tf.Wc)


def test_bs_polynomial_expectations_on_the_device(amd, golden):
    """BayesSardModel._exp_x_kxpx and utils.vandermonde as callables of their own (`ssmq_bs_moments`): the reference's
    known answer (ssmtoybox/tests/test_bqmod.py:316-326), its outputs for every Bayes-Sard golden case, and its
    Monte-Carlo verification of all four expectations (test_bqmod.py:328-366, tolerance 5e-3 as there)."""
    from ssmtoybox_amd import utils
    from ssmtoybox_amd.bq.bqmod import BayesSardModel
    model = BayesSardModel(1, np.array([[1.0, 1.0]]), multi_ind=2, point_str='ut', point_par={'kappa': 0.0})
    mi_1d = np.array([[0, 1, 2]])
    par_1d = np.array([[1.0, 1.0]])
    data = np.array([[0.0, 1.0, -1.0]])
    ke = model._exp_x_kxpx(par_1d, mi_1d, data)
    s2, e = 2 ** 0.5, np.exp(-0.25)
    ke_true = np.array([[1 / s2, 0, 1 / (2 * s2)], [e / s2, e / (2 * s2), 3 * e / (4 * s2)],
                        [e / s2, -e / (2 * s2), 3 * e / (4 * s2)]])
    assert ke.shape == (3, 3) and np.allclose(ke, ke_true, rtol=1e-14, atol=1e-16)
    g = golden('g2_bs_weights')
    tags = sorted({k[:-3] for k in g if k.endswith('_mi')})
    for t in tags:
        mi, pts, par = g[t + '_mi'], g[t + '_pts'], g[t + '_par']
        m = BayesSardModel(pts.shape[0], par, multi_ind=mi, point_str='ut')
        kx = m._exp_x_kxpx(par, mi, pts)
        assert within(rel_err(kx, g[t + '_kxpx']), 1e-13, 'bs kxpx vs reference ' + t)
        V = utils.vandermonde(mi, pts)
        assert V.shape == g[t + '_V'].shape
        assert within(rel_err(V, g[t + '_V']), 1e-15, 'vandermonde vs reference ' + t)
    # Monte-Carlo verification, 2e6 standard normal samples (the reference draws 1e7; same 5e-3 bar)
    rng = np.random.default_rng(12)
    xs = rng.standard_normal((1, 2000000))
    p = xs.T ** mi_1d[0][None, :]
    k = np.exp(-0.5 * (xs.T - data) ** 2)                   # alpha = 1, ell = 1, unscaled kernel
    px, xpx, pxpx = model._exp_x_px(mi_1d), model._exp_x_xpx(mi_1d), model._exp_x_pxpx(mi_1d)
    assert np.abs(px - p.mean(axis=0)).max() < 5e-3
    assert np.abs(xpx - (xs.T * p).mean(axis=0)[None, :]).max() < 5e-3
    assert np.abs(pxpx - p.T.dot(p) / p.shape[0]).max() < 5e-3
    assert np.abs(ke - k.T.dot(p) / p.shape[0]).max() < 5e-3


@pytest.mark.parametrize('tag', ['d1', 'd3', 'd6'])
def test_reference_metric_functions_per_item(amd, golden, tag):
    """utils.neg_log_likelihood / log_cred_ratio / mse_matrix with the reference's per-item signatures
    (ssmtoybox/tests/test_utils.py:16-33 calls them this way), through the device reductions, against the reference's
    values - including covariances that are not positive definite."""
    from ssmtoybox_amd import utils
    g = golden('g7_metrics')
    x, m, P = g[tag + '_x'], g[tag + '_m'], g[tag + '_P']
    D, T, M = m.shape
    for k in (0, T // 2, T - 1):
        mse = utils.mse_matrix(x[:, k, :], m[:, k, :])
        assert mse.shape == (D, D) and np.allclose(mse, g[tag + '_mse'][..., k], rtol=1e-12, atol=1e-14)
        for i in (0, M - 1):
            nll = utils.neg_log_likelihood(x[:, k, i], m[:, k, i], P[..., k, i])
            assert abs(nll - g[tag + '_nll'][k, i]) < 1e-11 * max(1.0, abs(nll))
            lcr = utils.log_cred_ratio(x[:, k, i], m[:, k, i], P[..., k, i], mse + 1e-6 * np.eye(D))
            assert abs(lcr - g[tag + '_lcr'][k, i]) < 1e-9 * max(1.0, abs(lcr))
    if tag + '_Pi' in g:
        Pi, flip = g[tag + '_Pi'], g[tag + '_flip']
        ks, is_ = np.nonzero(flip)
        for k, i in list(zip(ks, is_))[:4]:
            mse = g[tag + '_mse'][..., k] + 1e-6 * np.eye(D)
            nll = utils.neg_log_likelihood(x[:, k, i], m[:, k, i], Pi[..., k, i])
            assert abs(nll - g[tag + '_nlli'][k, i]) < 1e-9 * max(1.0, abs(nll))
            lcr = utils.log_cred_ratio(x[:, k, i], m[:, k, i], Pi[..., k, i], mse)
            assert abs(lcr - g[tag + '_lcri'][k, i]) < 1e-8 * max(1.0, abs(lcr))
    with pytest.raises(np.linalg.LinAlgError):
        utils.neg_log_likelihood(np.zeros(D), np.ones(D), np.zeros((D, D)))
    # the reference's own smoke test: a random state, mean and covariance of dimension 5
    rng = np.random.default_rng(3)
    xx, mm, A = rng.standard_normal(5), rng.standard_normal(5), rng.standard_normal((5, 5))
    cov = A.dot(A.T)
    dx = xx - mm
    want = 0.5 * (np.linalg.slogdet(cov)[1] + dx.dot(np.linalg.inv(cov)).dot(dx) + 5 * np.log(2 * np.pi))
    assert abs(utils.neg_log_likelihood(xx, mm, cov) - want) < 1e-10 * abs(want)
    assert utils.mse_matrix(rng.standard_normal((5, 100)), rng.standard_normal((5, 100))).shape == (5, 5)


# ---------------------------------------------------------------------------------------------------------------
# the filter recursion around the path
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['ukf', 'ckf', 'ghkf', 'gpqkf', 'tpqkf', 'bsqkf'])
def test_ungm_filter_golden(amd, golden, name):
    from ssmtoybox_amd import ssinf, ssmod as sm
    g = golden('g4_filters')
    y = g['ungm_y']                                    # (1, T, seeds)
    dyn = sm.UNGMTransition(sm.GaussRV(1), sm.GaussRV(1, cov=np.array([[10.0]])))
    obs = sm.UNGMMeasurement(sm.GaussRV(1), 1)
    par = np.array([[1.0, 3.0]])
    mi = np.array([[0, 1, 2]])
    alg = {'ukf': lambda: ssinf.UnscentedKalman(dyn, obs), 'ckf': lambda: ssinf.CubatureKalman(dyn, obs),
           'ghkf': lambda: ssinf.GaussHermiteKalman(dyn, obs, deg=5),
           'gpqkf': lambda: ssinf.GaussianProcessKalman(dyn, obs, par, par, 'rbf', 'ut'),
           'tpqkf': lambda: ssinf.StudentProcessKalman(dyn, obs, par, par, 'rbf', 'ut'),
           'bsqkf': lambda: ssinf.BayesSardKalman(dyn, obs, par, par, mi, mi, 'ut')}[name]()
    fm, fP = alg.forward_pass_batch(y)                 # all seeds in one batch
    k = 'ungm_' + name
    assert rel_err(fm, g[k + '_fm']) < 1e-8, name      # 100 steps amplify weight round-off ~900x
    assert within(cov_err(fP, g[k + '_fc']), 5e-9, 'ungm %s fP vs reference' % name), name
    # the reference's one-trajectory interface
    fm1, fP1 = alg.forward_pass(y[..., 0])
    assert np.array_equal(fm1, fm[..., 0]) and np.array_equal(fP1, fP[..., 0])
    # RTS smoother (backward_pass), including the reference's indexing quirk at the last two steps
    fm, fP = alg.forward_pass_batch(y)
    sm, sP = alg.backward_pass_batch()
    assert rel_err(sm, g[k + '_sm']) < 1e-8 and within(cov_err(sP, g[k + '_sc']), 5e-9, 'ungm %s sP vs reference' % name), name
    assert np.array_equal(sm[:, -2:], fm[:, -2:]) and np.array_equal(alg.fi_mean, fm)


def test_fused_filter_matches_unfused_loop(amd, golden, monkeypatch):
    """The one-kernel time loop and the 3 T-launch loop (hipGraph replay) are the same arithmetic."""
    from ssmtoybox_amd import ssinf, ssmod as sm
    g = golden('g4_filters')
    y = np.repeat(g['ungm_y'], 40, axis=2)[..., :300]
    dyn = sm.UNGMTransition(sm.GaussRV(1), sm.GaussRV(1, cov=np.array([[10.0]])))
    obs = sm.UNGMMeasurement(sm.GaussRV(1), 1)
    par = np.array([[1.0, 3.0]])
    for alg in (ssinf.GaussianProcessKalman(dyn, obs, par, par), ssinf.UnscentedKalman(dyn, obs),
                ssinf.StudentProcessKalman(dyn, obs, par, par)):
        monkeypatch.delenv('SSMQ_NO_FUSED', raising=False)
        assert 'k_filter_fused' in alg.kernel_name()
        fm, fP = alg.forward_pass_batch(y)
        monkeypatch.setenv('SSMQ_NO_FUSED', '1')
        assert 'hipGraph' in alg.kernel_name()
        fm2, fP2 = alg.forward_pass_batch(y)
        fm3, fP3 = alg.forward_pass_batch(y)          # second call replays the captured graph
        monkeypatch.delenv('SSMQ_NO_FUSED')
        assert np.array_equal(fm2, fm3) and np.array_equal(fP2, fP3)
        assert rel_err(fm, fm2) < 1e-12 and within(cov_err(fP, fP2), 1e-11, 'ungm fused vs loop fP ' + type(alg).__name__)
    # reentry: fused (5, 2, 11) kernel against the loop of stand-alone kernels
    y = g['rer_y']
    dyn = sm.ReentryVehicle2DTransition(sm.GaussRV(5, g['rer_m0'], g['rer_P0']), sm.GaussRV(3, cov=g['rer_Q']))
    obs = sm.Radar2DMeasurement(sm.GaussRV(2, cov=g['rer_R']), 5)
    alg = ssinf.UnscentedKalman(dyn, obs)
    assert 'k_filter_fused<D=5,Y=2' in alg.kernel_name()
    had_quad = os.environ.get('SSMQ_FUSED_QUAD')
    monkeypatch.setenv('SSMQ_FUSED_QUAD', '0')          # the register kernel (a batch this small would take k_filter_quad: other summation order)
    fm, fP = alg.forward_pass_batch(y)
    if had_quad is None:
        monkeypatch.delenv('SSMQ_FUSED_QUAD')
    else:
        monkeypatch.setenv('SSMQ_FUSED_QUAD', had_quad)
    monkeypatch.setenv('SSMQ_NO_FUSED', '1')
    fm2, fP2 = alg.forward_pass_batch(y)
    monkeypatch.delenv('SSMQ_NO_FUSED')
    assert within(mean_err(fm, fm2), 1e-12, 'reentry ukf fused vs loop fm (row-scaled)')
    assert within(cov_err(fP, fP2), 1e-11, 'reentry ukf fused vs loop fP (entry-scaled)')
    # smoother: forward pass that keeps the predictive moments, as one kernel and as the launch loop
    y = np.repeat(g['ungm_y'], 40, axis=2)[..., :300]
    dyn = sm.UNGMTransition(sm.GaussRV(1), sm.GaussRV(1, cov=np.array([[10.0]])))
    obs = sm.UNGMMeasurement(sm.GaussRV(1), 1)
    for alg in (ssinf.GaussianProcessKalman(dyn, obs, par, par), ssinf.UnscentedKalman(dyn, obs),
                ssinf.StudentProcessKalman(dyn, obs, par, par)):
        alg.forward_pass_batch(y)
        s1, S1 = alg.backward_pass_batch()
        monkeypatch.setenv('SSMQ_NO_FUSED', '1')
        s2, S2 = alg.backward_pass_batch()
        monkeypatch.delenv('SSMQ_NO_FUSED')
        assert rel_err(s1, s2) < 1e-12 and within(cov_err(S1, S2), 1e-11, 'ungm smoother fused vs loop ' + type(alg).__name__)
    y = g['rer_y']
    dyn = sm.ReentryVehicle2DTransition(sm.GaussRV(5, g['rer_m0'], g['rer_P0']), sm.GaussRV(3, cov=g['rer_Q']))
    obs = sm.Radar2DMeasurement(sm.GaussRV(2, cov=g['rer_R']), 5)
    alg = ssinf.UnscentedKalman(dyn, obs)
    alg.forward_pass_batch(y)
    s1, S1 = alg.backward_pass_batch()
    monkeypatch.setenv('SSMQ_NO_FUSED', '1')
    s2, S2 = alg.backward_pass_batch()
    monkeypatch.delenv('SSMQ_NO_FUSED')
    assert within(mean_err(s1, s2), 1e-8, 'reentry ukf smoother fused vs loop sm (row-scaled)')
    assert within(cov_err(S1, S2), 2e-8, 'reentry ukf smoother fused vs loop sP (entry-scaled)')


def test_spherical_radial_fused_filters_match_launch_loop(amd, golden, monkeypatch):
    """Fused instantiations for spherical-radial point sets (2 D points: the cubature Kalman filter, BQ transforms built
    with 'sr'): one-kernel time loop against the launch loop of stand-alone kernels, on the reentry, pendulum and
    coordinated-turn models; the cubature filter on UNGM additionally has a reference golden (test_ungm_filter_golden)."""
    from ssmtoybox_amd import ssinf, ssmod as sm
    g = golden('g4_filters')
    dyn = sm.ReentryVehicle2DTransition(sm.GaussRV(5, g['rer_m0'], g['rer_P0']), sm.GaussRV(3, cov=g['rer_Q']))
    obs = sm.Radar2DMeasurement(sm.GaussRV(2, cov=g['rer_R']), 5)
    rng = np.random.default_rng(21)
    pend = sm.Pendulum2DTransition(sm.GaussRV(2, mean=np.array([1.5, 0.0]), cov=0.01 * np.eye(2)),
                                   sm.GaussRV(2, cov=0.01 * np.eye(2)), 0.01)
    pobs = sm.Pendulum2DMeasurement(sm.GaussRV(1, cov=np.array([[0.1]])), 2)
    yp = np.sin(1.5 + 0.05 * rng.standard_normal((1, 40, 64))) + 0.3 * rng.standard_normal((1, 40, 64))
    m0c = np.array([1000, 300, 1000, 0, np.deg2rad(-3.0)])
    ct = sm.CoordinatedTurnTransition(sm.GaussRV(5, m0c, np.diag([100, 10, 100, 10, 0.1])),
                                      sm.GaussRV(5, cov=np.diag([1e-3, 1e-2, 1e-3, 1e-2, 1e-5])), dt=0.1)
    bear = sm.BearingMeasurement(sm.GaussRV(4, cov=10e-3 * np.eye(4)), 5, state_index=[0, 2], sensor_pos=SENSORS)
    pos = m0c[[0, 2]][:, None, None] + np.array([30.0, 0.0])[:, None, None] * np.arange(1, 9)[None, :, None]
    yc = np.arctan2(pos[1][None] - SENSORS[:, 1][:, None, None], pos[0][None] - SENSORS[:, 0][:, None, None]) + \
        0.05 * rng.standard_normal((4, 8, 64))
    cases = [('reentry ckf', ssinf.CubatureKalman(dyn, obs), np.tile(g['rer_y'], (1, 1, 8))[:, :40], 'D=5,Y=2,ND=10', 1e-11),
             ('pendulum ckf', ssinf.CubatureKalman(pend, pobs), yp, 'D=2,Y=1,ND=4', 1e-11),
             ('pendulum gpqkf sr', ssinf.GaussianProcessKalman(pend, pobs, np.array([[1.0, 3, 3]]), np.array([[1.0, 3, 3]]),
                                                               'rbf', 'sr'), yp, 'D=2,Y=1,ND=4', 1e-10),
             ('pendulum tpqkf sr', ssinf.StudentProcessKalman(pend, pobs, np.array([[1.0, 3, 3]]), np.array([[1.0, 3, 3]]),
                                                              'rbf', 'sr'), yp, 'D=2,Y=1,ND=4', 1e-10),
             ('ct ckf', ssinf.CubatureKalman(ct, bear), yc, 'D=5,Y=4,ND=10', 1e-10)]
    for name, alg, y, tag, bar in cases:
        monkeypatch.delenv('SSMQ_NO_FUSED', raising=False)
        assert 'k_filter_fused<' + tag in alg.kernel_name(), alg.kernel_name()
        fm, fP = alg.forward_pass_batch(y, raise_on_failure=False)
        st = alg.status.copy()
        monkeypatch.setenv('SSMQ_NO_FUSED', '1')
        assert 'hipGraph' in alg.kernel_name()
        fm2, fP2 = alg.forward_pass_batch(y, raise_on_failure=False)
        monkeypatch.delenv('SSMQ_NO_FUSED')
        assert np.array_equal(st, alg.status), name
        ok = st == 0
        assert ok.any(), name
        assert within(mean_err(fm[..., ok], fm2[..., ok]), bar, name + ' fused vs loop fm (row-scaled)')
        assert within(cov_err(fP[..., ok], fP2[..., ok]), 10 * bar, name + ' fused vs loop fP (entry-scaled)')
        if name in ('reentry ckf', 'pendulum ckf') and ok.all():
            # cubature smoother: forward pass that keeps the predictive moments as one kernel, then the RTS pass
            alg.forward_pass_batch(y)
            s1, S1 = alg.backward_pass_batch()
            monkeypatch.setenv('SSMQ_NO_FUSED', '1')
            s2, S2 = alg.backward_pass_batch()
            monkeypatch.delenv('SSMQ_NO_FUSED')
            assert within(mean_err(s1, s2), 1e-8, name + ' smoother fused vs loop sm (row-scaled)')
            assert within(cov_err(S1, S2), 2e-8, name + ' smoother fused vs loop sP (entry-scaled)')


def test_student_filters_golden(amd, golden, monkeypatch):
    """Studentian recursion (ssinf.py:555-857) against the reference's trajectories: fully-symmetric Student filter on
    UNGM (fused kernel) and on CV + radar (launch loop, generic kernels), and the t-process quadrature Student filter
    with the reference's Monte-Carlo weights injected."""
    from ssmtoybox_amd import ssinf, ssmod as sm
    g = golden('g5_student')
    y = g['ungm_y']
    dyn = sm.UNGMTransition(sm.StudentRV(1), sm.StudentRV(1, scale=np.array([[10.0]])))
    obs = sm.UNGMMeasurement(sm.StudentRV(1), 1)
    alg = ssinf.FullySymmetricStudent(dyn, obs)
    assert np.array_equal(alg.tf_dyn.unit_sp, [[0.0, 3.0, -3.0]])
    for no_fused in (False, True):
        if no_fused:
            monkeypatch.setenv('SSMQ_NO_FUSED', '1')
        else:
            monkeypatch.delenv('SSMQ_NO_FUSED', raising=False)
        assert ('hipGraph' if no_fused else 'k_filter_fused') in alg.kernel_name()
        fm, fP = alg.forward_pass_batch(y)
        assert rel_err(fm, g['ungm_fss_fm']) < 1e-9 and within(cov_err(fP, g['ungm_fss_fc']), 1e-10, 'ungm fss fP vs reference'), no_fused
    monkeypatch.delenv('SSMQ_NO_FUSED', raising=False)
    kp = np.atleast_2d(np.ones(2))
    alg = ssinf.StudentProcessStudent(dyn, obs, kp, kp)
    for tf, tag in ((alg.tf_dyn, 'dyn'), (alg.tf_obs, 'obs')):
        k = 'ungm_tpqs_' + tag
        assert np.array_equal(tf.model.points, g[k + '_pts']) and tf.model.nu == float(g[k + '_nu'])
        tf.wm, tf.Wc, tf.Wcc = g[k + '_wm'], g[k + '_Wc'], g[k + '_Wcc']
        tf.model.model_var, tf.model.iK = float(g[k + '_mv']), g[k + '_iK']
    fm, fP = alg.forward_pass_batch(y)
    assert rel_err(fm, g['ungm_tpqs_fm']) < 1e-8 and within(cov_err(fP, g['ungm_tpqs_fc']), 1e-10, 'ungm tpqs fP vs reference')
    # constant velocity + radar
    y = g['cv_y']
    dyn = sm.ConstantVelocity(sm.StudentRV(4, g['cv_m0'], g['cv_P0'], 1000.0),
                              sm.StudentRV(2, scale=np.diag([50.0, 5.0]), dof=1000.0), dt=0.5)
    obs = sm.Radar2DMeasurement(sm.StudentRV(2, scale=np.diag([50.0, 0.4e-6]), dof=4.0), 4)
    alg = ssinf.FullySymmetricStudent(dyn, obs)
    assert 'k_filter_fused<D=4,Y=2' in alg.kernel_name()
    fm, fP = alg.forward_pass_batch(y)
    assert within(mean_err(fm, g['cv_fss_fm']), 1e-12, 'cv fss fm vs reference (row-scaled)')
    assert within(cov_err(fP, g['cv_fss_fc']), 1e-10, 'cv fss fP vs reference (entry-scaled)')
    monkeypatch.setenv('SSMQ_NO_FUSED', '1')
    fm2, fP2 = alg.forward_pass_batch(y)
    monkeypatch.delenv('SSMQ_NO_FUSED')
    assert within(mean_err(fm, fm2), 1e-12, 'cv fss fused vs loop fm') and within(cov_err(fP, fP2), 1e-10, 'cv fss fused vs loop fP')
    # reentry-1D + range (tests/test_ssinf.py:40-50 of the reference): fused (3, 1, 7) kernel against the launch loop
    m0, P0 = np.array([90.0, 6.0, 1.7]), np.diag([0.3048 ** 2, 1.2192 ** 2, 10.0])
    dyn = sm.ReentryVehicle1DTransition(sm.GaussRV(3, m0, P0), sm.GaussRV(3, cov=np.zeros((3, 3))))
    obs = sm.RangeMeasurement(sm.GaussRV(1, cov=np.array([[0.03048 ** 2]])), 3)
    xs, ys, _ = sm.simulate_dev(dyn, obs, 30, 500, seed=4)
    yy = ys.download((30, 1, 512))[:, :, :500].transpose(1, 0, 2)
    xs.free()
    ys.free()
    alg = ssinf.UnscentedKalman(dyn, obs)
    assert 'k_filter_fused<D=3,Y=1' in alg.kernel_name()
    fm, fP = alg.forward_pass_batch(yy, raise_on_failure=False)
    st = alg.status.copy()
    monkeypatch.setenv('SSMQ_NO_FUSED', '1')
    fm2, fP2 = alg.forward_pass_batch(yy, raise_on_failure=False)
    monkeypatch.delenv('SSMQ_NO_FUSED')
    ok = (st == 0) & (alg.status == 0)
    assert ok.mean() > 0.9 and within(mean_err(fm[..., ok], fm2[..., ok]), 1e-12, 'reentry1d fused vs loop fm')
    assert within(cov_err(fP[..., ok], fP2[..., ok]), 1e-12, 'reentry1d fused vs loop fP')


def test_reentry_ukf_golden(amd, golden):
    from ssmtoybox_amd import ssinf, ssmod as sm
    g = golden('g4_filters')
    y = g['rer_y']
    dyn = sm.ReentryVehicle2DTransition(sm.GaussRV(5, g['rer_m0'], g['rer_P0']), sm.GaussRV(3, cov=g['rer_Q']))
    obs = sm.Radar2DMeasurement(sm.GaussRV(2, cov=g['rer_R']), 5)
    alg = ssinf.UnscentedKalman(dyn, obs)
    fm, fP = alg.forward_pass_batch(y)
    assert within(mean_err(fm, g['rer_ukf_fm']), 1e-8, 'reentry ukf fm vs reference (row-scaled)')
    assert within(cov_err(fP, g['rer_ukf_fc']), 2e-8, 'reentry ukf fP vs reference (entry-scaled)')


@pytest.mark.parametrize('name', ['ukf', 'ckf', 'gpqkf'])
def test_ungmna_filter_golden(amd, golden, name):
    """Noise as a model argument (ssinf.py:271-295): augmented moments, trimmed cross-covariance."""
    from ssmtoybox_amd import ssinf, ssmod as sm
    g = golden('g6_nonadditive')
    y = g['ungmna_y']
    q = sm.GaussRV(1, cov=np.array([[10.0]]))
    dyn = sm.UNGMNATransition(sm.GaussRV(1, mean=np.array([1.0])), q)
    obs = sm.UNGMNAMeasurement(sm.GaussRV(1), 1)
    par = np.array([[1.0, 3.0, 3.0]])
    mk = {'ukf': lambda d: ssinf.UnscentedKalman(d, obs), 'ckf': lambda d: ssinf.CubatureKalman(d, obs),
          'gpqkf': lambda d: ssinf.GaussianProcessKalman(d, obs, par, par, 'rbf', 'ut')}[name]
    alg = mk(dyn)
    fm, fP = alg.forward_pass_batch(y)
    assert g['ungmna_' + name + '_ok'].all() and not alg.status.any()
    assert rel_err(fm, g['ungmna_' + name + '_fm']) < 1e-8, name
    assert within(cov_err(fP, g['ungmna_' + name + '_fc']), 1e-11, 'ungmna %s fP vs reference' % name), name
    # RTS smoother: backward_pass of the reference does not look at the model; the cross-covariance is the one cut back
    # to the state columns (ssinf.py:120-147, 294-295).  One kernel with the predictive moments kept, and the launch loop.
    xs, Ps = alg.backward_pass_batch()
    assert rel_err(xs, g['ungmna_' + name + '_sm']) < 1e-8, name
    assert within(cov_err(Ps, g['ungmna_' + name + '_sc']), 1e-9, 'ungmna %s sP vs reference' % name), name
    assert np.array_equal(xs[:, -2:], fm[:, -2:]) and np.array_equal(alg.fi_mean, fm)
    os.environ['SSMQ_NO_FUSED'] = '1'
    try:
        xs2, Ps2 = alg.backward_pass_batch()
    finally:
        del os.environ['SSMQ_NO_FUSED']
    assert rel_err(xs2, xs) < 1e-11 and within(cov_err(Ps2, Ps), 1e-10, 'ungmna %s smoother fused vs loop' % name)
    if name == 'ckf':
        # zero-mean prior: the cubature rule has no centre point, so m_pr = 0 and the measurement 0.05 r x^2 gets
        # P_y = 0 exactly at the first step - the reference raises LinAlgError for every trajectory (golden mask)
        assert not g['ungmna0_ckf_ok'].any()
        alg0 = mk(sm.UNGMNATransition(sm.GaussRV(1), q))
        alg0.forward_pass_batch(y, raise_on_failure=False)
        assert np.array_equal(alg0.status, np.ones(y.shape[2], dtype=np.int32))      # 1 + first failing step (0)
        with pytest.raises(np.linalg.LinAlgError):
            alg0.forward_pass_batch(y)


def test_nonadditive_fused_matches_launch_loop(amd, golden, monkeypatch):
    """k_filter_fused_aug against the loop of stand-alone kernels (SSMQ_NO_FUSED=1) on the same data."""
    from ssmtoybox_amd import ssinf, ssmod as sm
    g = golden('g6_nonadditive')
    q = sm.GaussRV(1, cov=np.array([[10.0]]))
    dyn = sm.UNGMNATransition(sm.GaussRV(1, mean=np.array([1.0])), q)
    obs = sm.UNGMNAMeasurement(sm.GaussRV(1), 1)
    par = np.array([[1.0, 3.0, 3.0]])
    y = np.tile(g['ungmna_y'], (1, 1, 40))[..., :200]
    for alg in (ssinf.UnscentedKalman(dyn, obs), ssinf.CubatureKalman(dyn, obs),
                ssinf.GaussianProcessKalman(dyn, obs, par, par, 'rbf', 'ut'),
                ssinf.StudentProcessKalman(dyn, obs, par, par, 'rbf', 'ut')):
        fm, fP = alg.forward_pass_batch(y, raise_on_failure=False)
        st = alg.status.copy()
        monkeypatch.setenv('SSMQ_NO_FUSED', '1')
        fm2, fP2 = alg.forward_pass_batch(y, raise_on_failure=False)
        monkeypatch.delenv('SSMQ_NO_FUSED')
        assert np.array_equal(st, alg.status)
        ok = st == 0
        assert rel_err(fm[..., ok], fm2[..., ok]) < 1e-11, type(alg).__name__
        assert within(cov_err(fP[..., ok], fP2[..., ok]), 1e-13, 'ungmna fused vs loop fP ' + type(alg).__name__)
    dyn = sm.ConstantTurnRateSpeed(sm.GaussRV(5, mean=g['ctrs_m0'], cov=0.1 * np.eye(5)),
                                   sm.GaussRV(2, cov=np.diag([0.1, 0.1 * np.pi])))
    obs = sm.Radar2DMeasurement(sm.GaussRV(2, cov=np.diag([0.3, 0.03])), 5)
    alg = ssinf.UnscentedKalman(dyn, obs)
    yy = np.tile(g['ctrs_y'], (1, 1, 25))
    fm, fP = alg.forward_pass_batch(yy)
    monkeypatch.setenv('SSMQ_NO_FUSED', '1')
    fm2, fP2 = alg.forward_pass_batch(yy)
    monkeypatch.delenv('SSMQ_NO_FUSED')
    assert within(mean_err(fm, fm2), 1e-11, 'ctrs fused vs loop fm') and within(cov_err(fP, fP2), 1e-10, 'ctrs fused vs loop fP')


def test_ctrs_radar_ukf_golden(amd, golden):
    """Non-additive dynamics (5 states + 2 noise inputs, D = 7 transform) with an additive radar."""
    from ssmtoybox_amd import ssinf, ssmod as sm
    g = golden('g6_nonadditive')
    y = g['ctrs_y']
    dyn = sm.ConstantTurnRateSpeed(sm.GaussRV(5, mean=g['ctrs_m0'], cov=0.1 * np.eye(5)),
                                   sm.GaussRV(2, cov=np.diag([0.1, 0.1 * np.pi])))
    obs = sm.Radar2DMeasurement(sm.GaussRV(2, cov=np.diag([0.3, 0.03])), 5)
    alg = ssinf.UnscentedKalman(dyn, obs)
    fm, fP = alg.forward_pass_batch(y)
    assert within(mean_err(fm, g['ctrs_ukf_fm']), 1e-11, 'ctrs ukf fm vs reference (row-scaled)')
    assert within(cov_err(fP, g['ctrs_ukf_fc']), 1e-10, 'ctrs ukf fP vs reference (entry-scaled)')
    # smoother of a model with non-additive dynamics (7-input transform, cross-covariance with 7 columns of which the RTS
    # pass uses the 5 state columns): launch loop + k_rts_backward
    sm, sP = alg.backward_pass_batch()
    assert within(mean_err(sm, g['ctrs_ukf_sm']), 1e-10, 'ctrs ukf sm vs reference (row-scaled)')
    assert within(cov_err(sP, g['ctrs_ukf_sc']), 1e-9, 'ctrs ukf sP vs reference (entry-scaled)')
    # ragged batch through the same loop: 130 copies of the four trajectories
    yy = np.tile(y, (1, 1, 33))[..., :130]
    fm2, _ = alg.forward_pass_batch(yy)
    assert np.array_equal(fm2[..., :4], fm) and np.array_equal(fm2[..., 128:130], fm[..., :2])


# ---------------------------------------------------------------------------------------------------------------
# marginalised GP-quadrature filter: theta-batched step on the device (ssinf.py:1034-1292)
# ---------------------------------------------------------------------------------------------------------------
def _marginal_models(tag, g):
    from ssmtoybox_amd import ssmod as sm
    if tag.startswith('ungm'):
        dyn = sm.UNGMTransition(sm.GaussRV(1), sm.GaussRV(1, cov=np.array([[10.0]])))
        obs = sm.UNGMMeasurement(sm.GaussRV(1), 1)
        return dyn, obs, tag.split('_')[1]
    dyn = sm.Pendulum2DTransition(sm.GaussRV(2, np.array([1.5, 0]), 0.01 * np.eye(2)), sm.GaussRV(2, cov=g['pend_Q']), 0.01)
    obs = sm.Pendulum2DMeasurement(sm.GaussRV(1, cov=g['pend_R']), 2)
    return dyn, obs, 'sr'


@pytest.mark.parametrize('tag', ['ungm_sr', 'ungm_ut', 'pend'])
def test_marginal_theta_step_golden(amd, golden, tag):
    from ssmtoybox_amd import ssinf
    g = golden('g8_marginal')
    dyn, obs, pts = _marginal_models(tag, g)
    alg = ssinf.MarginalizedGaussianProcessKalman(dyn, obs, 'rbf', pts)
    th, m, P, y = g[tag + '_theta'], g[tag + '_m'], g[tag + '_P'], g[tag + '_y']
    n = th.shape[0]
    ks = g[tag + '_k'] if tag.startswith('ungm') else np.full(n, 3)
    pm, pc, ll = np.zeros_like(g[tag + '_pm']), np.zeros_like(g[tag + '_pc']), np.zeros(n)
    for k in np.unique(ks):          # one device call per time index, items with their own state and measurement
        sel = np.flatnonzero(ks == k)
        pm[sel], pc[sel], ll[sel], st = alg.theta_step(th[sel], m[sel], P[sel], y[sel], int(k))
        assert not st.any()
    assert rel_err(pm, g[tag + '_pm']) < 1e-9
    assert rel_err(pc, g[tag + '_pc']) < 1e-8
    assert np.max(np.abs(ll - g[tag + '_ll']) / np.maximum(1.0, np.abs(g[tag + '_ll']))) < 1e-9
    # shared state / measurement (the marginalisation call pattern) = the same items one by one
    pm2, pc2, ll2, _ = alg.theta_step(th, m[0], P[0], y[0], int(ks[0]))
    one = alg.theta_step(th[3], m[0], P[0], y[0], int(ks[0]))
    assert np.array_equal(pm2[3], one[0][0]) and np.array_equal(pc2[3], one[1][0]) and ll2[3] == one[2][0]
    alg.x_mean_fi, alg.x_cov_fi = m[0], P[0]
    assert alg._param_log_likelihood(th[3], y[0], int(ks[0])) == ll2[3]


def test_marginal_theta_step_batch_vs_oracle(amd):
    """1000 parameter items in one call (k_weights with one workgroup per item feeding k_apply_wide in place)."""
    from ssmtoybox_amd import ssinf, ssmod as sm
    dt = 0.01
    Q = np.array([[dt ** 3 / 3, dt ** 2 / 2], [dt ** 2 / 2, dt]])
    dyn = sm.Pendulum2DTransition(sm.GaussRV(2, np.array([1.5, 0]), 0.01 * np.eye(2)), sm.GaussRV(2, cov=Q), dt)
    obs = sm.Pendulum2DMeasurement(sm.GaussRV(1, cov=np.array([[0.1]])), 2)
    alg = ssinf.MarginalizedGaussianProcessKalman(dyn, obs, 'rbf', 'ut')
    rng = np.random.default_rng(5)
    n = 1000
    th = 0.5 * rng.standard_normal((n, alg.param_dim))
    m = np.array([1.5, 0.0]) + 0.3 * rng.standard_normal((n, 2))
    a = rng.standard_normal((n, 2, 2)) * 0.1
    P = np.einsum('nij,nkj->nik', a, a) + 0.01 * np.eye(2)
    y = np.sin(m[:, :1]) + 0.3 * rng.standard_normal((n, 1))
    pm, pc, ll, st = alg.theta_step(th, m, P, y, 7)
    assert not st.any()
    pts = orc.points_ut(2)
    for i in rng.choice(n, 25, replace=False):
        om, oc, ol = orc.marginal_theta_step(np.exp(th[i, :3]), np.exp(th[i, 3:]), m[i], P[i], y[i], 7, orc.F_PENDULUM_DYN,
                                             orc.F_PENDULUM_MEAS, pts, pts, Q, 0.1 * np.eye(1), (dt,), (),
                                             emv_broadcast=True)
        assert rel_err(pm[i], om) < 1e-9 and rel_err(pc[i], oc) < 1e-8 and abs(ll[i] - ol) < 1e-9 * max(1, abs(ol)), i
    # a covariance that is not positive definite is flagged (bit 2) on its item only
    P2 = P.copy()
    P2[17] = -np.eye(2)
    st2 = alg.theta_step(th, m, P2, y, 7)[3]
    assert st2[17] & 4 and not np.delete(st2, 17).any()


@pytest.mark.gpu
@pytest.mark.parametrize('model', ['ungm', 'pendulum_ut', 'pendulum_gh', 'nonadditive'])
def test_theta_step_two_launch_route_is_bitwise_the_stage_route(amd, model, monkeypatch):
    """`ssmq_gp_theta_step` as two launches (k_theta_weights: both transforms' weights in LDS; k_theta_chain: transform ->
    transform -> update -> log-likelihood in the wave that owns the item) against the launch-per-stage route
    (SSMQ_NO_THETA_FUSED) on the same items: same bodies, same summation orders, so EQUAL BITS - including items whose
    covariance or kernel matrix is not positive definite (NaN results, same flags) and item counts that leave waves and
    lane groups ragged.  The stage route runs eagerly the first time a shape is seen, is captured the second time and
    replayed from then on."""
    from ssmtoybox_amd import ssinf, ssmod as sm
    if os.environ.get('SSMQ_NO_WAVE'):
        pytest.skip('the chained kernel is built on the wave kernel')
    rng = np.random.default_rng(11)
    if model == 'ungm':
        dyn = sm.UNGMTransition(sm.GaussRV(1), sm.GaussRV(1, cov=np.array([[10.0]])))
        obs = sm.UNGMMeasurement(sm.GaussRV(1), 1)
        alg = ssinf.MarginalizedGaussianProcessKalman(dyn, obs, 'rbf', 'sr')
    elif model.startswith('pendulum'):
        dt = 0.01
        Q = np.array([[dt ** 3 / 3, dt ** 2 / 2], [dt ** 2 / 2, dt]])
        dyn = sm.Pendulum2DTransition(sm.GaussRV(2, np.array([1.5, 0]), 0.01 * np.eye(2)), sm.GaussRV(2, cov=Q), dt)
        obs = sm.Pendulum2DMeasurement(sm.GaussRV(1, cov=np.array([[0.1]])), 2)
        alg = ssinf.MarginalizedGaussianProcessKalman(dyn, obs, 'rbf', 'ut' if model.endswith('ut') else 'gh',
                                                      point_hyp=None if model.endswith('ut') else {'degree': 3})
    else:
        dyn = sm.UNGMNATransition(sm.GaussRV(1), sm.GaussRV(1, cov=np.array([[1.0]])))
        obs = sm.UNGMMeasurement(sm.GaussRV(1), 1)
        alg = ssinf.MarginalizedGaussianProcessKalman(dyn, obs, 'rbf', 'ut')
    D = dyn.dim_state
    # (20 001 items on one model: many workgroups per CU in flight, the hand-over through global planes under load)
    for n in (1, alg.param_dim + 1, 2 * alg.param_dim, 333) + ((20001,) if model == 'pendulum_ut' else ()):
        th = 0.4 * rng.standard_normal((n, alg.param_dim))
        m = 0.5 * rng.standard_normal((n, D))
        a = rng.standard_normal((n, D, D)) * 0.3
        P = np.einsum('nij,nkj->nik', a, a) + 0.05 * np.eye(D)
        if n > 20:
            P[5] = -np.eye(D)                       # input covariance not positive definite
            th[9, 1:] = np.nan                      # no kernel matrix: both weight sets fail
        y = rng.standard_normal((n, obs.dim_out))
        res = {}
        for route in ('two', 'two_again', 'stage', 'stage_captured', 'stage_replayed'):
            if route == 'stage':
                monkeypatch.setenv('SSMQ_NO_THETA_FUSED', '1')
            res[route] = alg.theta_step(th, m, P, y, 4)
        monkeypatch.delenv('SSMQ_NO_THETA_FUSED')
        for route in ('two_again', 'stage', 'stage_captured', 'stage_replayed'):
            for got, want in zip(res[route], res['two']):
                assert np.array_equal(got, want, equal_nan=got.dtype.kind == 'f'), (model, n, route)
        if n > 20:
            st = res['two'][3]
            assert st[5] & 4 and st[9] and not np.delete(st, [5, 9]).any()
            assert np.isnan(res['two'][0][5]).all() and np.isfinite(np.delete(res['two'][2], [5, 9])).all()
        # the same arguments shared by all items (the marginalisation call pattern)
        r1 = alg.theta_step(th, m[0], P[0], y[0], 4)
        monkeypatch.setenv('SSMQ_NO_THETA_FUSED', '1')
        r2 = alg.theta_step(th, m[0], P[0], y[0], 4)
        monkeypatch.delenv('SSMQ_NO_THETA_FUSED')
        for got, want in zip(r1, r2):
            assert np.array_equal(got, want, equal_nan=got.dtype.kind == 'f'), (model, n, 'shared')
    # the per-filter cache of the wrapper (descriptors, handles, noise terms) follows a noise covariance assigned afterwards
    before = alg.theta_step(th, m[0], P[0], y[0], 4)
    alg.r_cov = 2.0 * alg.r_cov
    after = alg.theta_step(th, m[0], P[0], y[0], 4)
    ok = ~np.isnan(before[2])
    assert ok.any() and not np.any(before[2][ok] == after[2][ok])
    alg.r_cov = 0.5 * alg.r_cov
    again = alg.theta_step(th, m[0], P[0], y[0], 4)
    assert np.array_equal(again[2], before[2], equal_nan=True)


def test_marginal_filter_forward_pass(amd, golden):
    """Whole marginalised filter on a short UNGM sequence.  BFGS on finite differences of a 1e-13-accurate objective:
    the optimiser path, not the device arithmetic, limits how closely two implementations agree."""
    from ssmtoybox_amd import ssinf, ssmod as sm
    g = golden('g8_marginal')
    dyn = sm.UNGMTransition(sm.GaussRV(1), sm.GaussRV(1, cov=np.array([[10.0]])))
    obs = sm.UNGMMeasurement(sm.GaussRV(1), 1)
    alg = ssinf.MarginalizedGaussianProcessKalman(dyn, obs, 'rbf', 'sr')
    fm, fP = alg.forward_pass(g['fwd_y'])
    assert fm.shape == g['fwd_fm'].shape and np.all(np.isfinite(fm)) and np.all(fP > 0)
    err_m = np.abs(fm - g['fwd_fm']) / np.maximum(1.0, np.abs(g['fwd_fm']))
    err_P = np.abs(fP - g['fwd_fc']) / np.maximum(1.0, np.abs(g['fwd_fc']))
    print('marginal forward pass: max rel diff mean %.3e cov %.3e' % (err_m.max(), err_P.max()))
    assert err_m[:, 0].max() < 1e-4 and err_P[..., 0].max() < 1e-4       # first step: same start, same optimum
    assert np.median(err_m) < 1e-2 and np.median(err_P) < 1e-2
    # the Laplace posterior of the last step is a valid covariance
    assert np.all(np.linalg.eigvalsh(alg.param_cov) > 0)
    fm2, _ = alg.forward_pass_serial(g['fwd_y'][..., None])
    assert np.array_equal(fm2[..., 0], fm)
    # The same pass with the optimiser taken out of the comparison: at every step the Laplace moments the REFERENCE's BFGS
    # run arrived at (stored with the fixture) are injected, so that what is compared over the 12 steps is the device
    # arithmetic - weights at the 2 P parameter points, two transforms each, update, mixture - and nothing else.
    alg.reset()
    T = g['fwd_y'].shape[1]
    fm3, fP3 = np.zeros((1, T)), np.zeros((1, 1, T))
    for k in range(1, T + 1):
        alg._measurement_update(g['fwd_y'][:, k - 1], k, laplace=(g['fwd_tm'][:, k - 1], g['fwd_tc'][..., k - 1]))
        fm3[:, k - 1], fP3[..., k - 1] = alg.x_mean_fi, alg.x_cov_fi
    e_m = np.abs(fm3 - g['fwd_fm']) / np.maximum(1.0, np.abs(g['fwd_fm']))
    e_P = np.abs(fP3 - g['fwd_fc']) / np.maximum(1.0, np.abs(g['fwd_fc']))
    assert within(e_m.max(), 1e-11, 'marginal filter, reference Laplace moments injected: means over 12 steps')
    assert within(e_P.max(), 1e-11, 'marginal filter, reference Laplace moments injected: covariances over 12 steps')


def test_marginal_filter_batched_monte_carlo(amd, golden):
    """forward_pass_batch of the marginalised filter: all trajectories advanced together, their BFGS runs in lock step
    (csrc/ssmq_marginal.hip; per round ONE theta step of (unfinished trajectories) x (param_dim + 1) items), against the loop
    the reference's research code runs (one scipy BFGS per trajectory and step: forward_pass_serial; research/tpq/
    tpq_base.py:175-192).  The two optimisers take the same path up to the noise of the forward-difference gradient
    (tests/test_bfgs_lockstep.py pins the restatement against scipy on the CPU); what the filter amplifies of that is what
    the comparison of this build's serial path with the reference shows as well (test_marginal_filter_forward_pass).  With
    the REFERENCE's Laplace moments the batch arithmetic is compared on its own: the marginalisation of 3 trajectories in one
    call against the golden pass."""
    from ssmtoybox_amd import ssinf, ssmod as sm
    from bench import simulate_ungm
    g = golden('g8_marginal')
    dyn = sm.UNGMTransition(sm.GaussRV(1), sm.GaussRV(1, cov=np.array([[10.0]])))
    obs = sm.UNGMMeasurement(sm.GaussRV(1), 1)
    alg = ssinf.MarginalizedGaussianProcessKalman(dyn, obs, 'rbf', 'sr')
    B, T = 24, 8
    _, y = simulate_ungm(B, T, 11)
    data = np.ascontiguousarray(y[None])                   # (1, T, B)
    data[:, :, 0] = g['fwd_y'][:, :T]                      # trajectory 0: the golden sequence
    fmb, fPb = alg.forward_pass_batch(data)
    stats = dict(alg.batch_stats)
    fms, fPs = alg.forward_pass_serial(data)
    assert fmb.shape == (1, T, B) and np.all(np.isfinite(fmb)) and np.all(fPb > 0)
    em = np.abs(fmb - fms) / np.maximum(1.0, np.abs(fms))
    eP = np.abs(fPb - fPs) / np.maximum(1.0, np.abs(fPs))
    print('batched vs serial marginal filter: mean max %.2e median %.2e; cov max %.2e median %.2e; %s' % (
        em.max(), np.median(em), eP.max(), np.median(eP), stats))
    ok = np.isfinite(fmb).all(axis=(0, 1)) & np.isfinite(fms).all(axis=(0, 1))
    assert ok.sum() >= B - 2 and np.array_equal(alg.batch_failed > 0, ~np.isfinite(fmb).all(axis=(0, 1)))
    em, eP = em[..., ok], eP[..., ok]
    # Two BFGS runs on forward differences of the same objective agree in the minimiser to ~1e-7 but in the inverse Hessian -
    # the Laplace covariance - only to ~1e-3 (tests/test_bfgs_lockstep.py), and the marginalised moments inherit that: the
    # bar of the serial path against the reference (1e-4 at the first step, test_marginal_filter_forward_pass) holds for the
    # typical trajectory, not for the worst of 24
    assert within(np.median(em[:, 0]), 2e-4, 'batched marginal filter vs serial, first step, means (median over trajectories)')
    assert within(np.median(eP[:, :, 0]), 2e-4, 'batched marginal filter vs serial, first step, covariances (median)')
    assert within(np.median(em), 2e-3, 'batched marginal filter vs serial, %d steps x %d trajectories, means (median)' % (T, B))
    assert within(np.median(eP), 2e-3, 'batched marginal filter vs serial, covariances (median)')
    # (the UNGM recursion amplifies: a tenth of the (trajectory, step) pairs differ by more than 1e-2 after a few steps)
    assert np.quantile(em, 0.75) < 5e-2 and np.quantile(eP, 0.75) < 5e-2
    # trajectory 0 is the golden sequence: as close to the reference as the serial path is
    e0 = np.abs(fmb[:, :, 0] - g['fwd_fm'][:, :T]) / np.maximum(1.0, np.abs(g['fwd_fm'][:, :T]))
    assert e0[:, 0].max() < 1e-4 and np.median(e0) < 1e-2
    # device calls: the lock step needs as many rounds as the SLOWEST trajectory of a step, not their sum
    assert stats['rounds'] < 0.4 * (stats['iterations'] * 2 + B * T) and stats['fallbacks'] == 0      # (set by the ONE longest trajectory: varies with the optimiser's noise)
    # a batch of one is the same computation
    fm1, fP1 = alg.forward_pass_batch(data[:, :, 3:4])
    assert np.array_equal(fm1[..., 0], fmb[..., 3]) and np.array_equal(fP1[..., 0], fPb[..., 3])
    # ... and so is the route that keeps the trajectories in lock step per time step (laplace_batch + one marginalisation call):
    # same optimiser, same device items; only the host-side mixture sums differ in their order of summation
    fmw, fPw = alg.forward_pass_batch_stepwise(data)
    stw = dict(alg.batch_stats)
    both = np.isfinite(fmw).all(axis=(0, 1)) & ok
    ew = np.abs(fmb - fmw)[..., both] / np.maximum(1.0, np.abs(fmw[..., both]))
    # (round 5: the own-pace route runs its state machines on the device - exp / log of another math library in the packing of the
    # kernel parameters and in the log prior, which BFGS's forward differences amplify like any other last-bit difference; with
    # the state machines on the host, as the per-step route has them, the two are the same arithmetic)
    assert within(np.median(ew), 2e-3, 'batched marginal filter: own-pace route (device rounds) vs per-step lock step, means (median)')
    import os
    os.environ['SSMQ_MARGINAL_HOST_ROUNDS'] = '1'
    try:
        fmh, fPh = alg.forward_pass_batch(data)
        sth = dict(alg.batch_stats)
    finally:
        del os.environ['SSMQ_MARGINAL_HOST_ROUNDS']
    bothh = np.isfinite(fmw).all(axis=(0, 1)) & np.isfinite(fmh).all(axis=(0, 1))
    ewh = np.abs(fmh - fmw)[..., bothh] / np.maximum(1.0, np.abs(fmw[..., bothh]))
    assert within(np.median(ewh), 2e-4, 'batched marginal filter: own-pace route (host rounds) vs per-step lock step, means (median)')
    # the longest trajectory's total against the sum of the slowest per step: strictly fewer where the two run the same arithmetic
    # (host rounds), about as many or fewer where the optimiser's noise differs (device rounds)
    assert sth['rounds'] < stw['rounds'] and stats['rounds'] < 1.3 * stw['rounds']
    print('rounds: own pace', stats['rounds'], '(host rounds', sth['rounds'], ') per-step lock step', stw['rounds'])


def test_marginal_filter_smoother_and_nonadditive_dynamics(amd, golden):
    """(1) The smoother the reference's MarginalInference inherits (ssinf.py:120-147): with the reference's per-step Laplace
    moments injected, the predictive moments forward_pass keeps (generic time update at index k - 1 with the weights of the
    LAST parameter point of the previous step - bq/bqmtran.py:93-95 - the dummy unit parameters at step 1), the filtered
    and the smoothed moments against the reference's.  (2) theta-conditioned steps for dynamics that take their noise as an
    argument (UNGMNA; augmented moments, ssinf.py:1174-1176) against the reference's _param_log_likelihood /
    _state_posterior_moments."""
    from ssmtoybox_amd import ssinf, ssmod as sm
    g = golden('g11_marginal_smoother')
    dyn = sm.UNGMTransition(sm.GaussRV(1), sm.GaussRV(1, cov=np.array([[10.0]])))
    obs = sm.UNGMMeasurement(sm.GaussRV(1), 1)
    alg = ssinf.MarginalizedGaussianProcessKalman(dyn, obs, 'rbf', 'sr')
    y = g['ungm_y']
    T = y.shape[1]
    pm, pP, pC = np.zeros((1, T)), np.zeros((1, 1, T)), np.zeros((1, 1, T))
    fm, fP = np.zeros((1, T)), np.zeros((1, 1, T))
    for k in range(1, T + 1):
        pm[:, k - 1], pP[..., k - 1], pC[..., k - 1] = alg._predictive_moments(k - 1)
        alg._measurement_update(y[:, k - 1], k, laplace=(g['ungm_tm'][:, k - 1], g['ungm_tc'][..., k - 1]))
        fm[:, k - 1], fP[..., k - 1] = alg.x_mean_fi, alg.x_cov_fi
    alg.fi_mean, alg.fi_cov, alg.pr_mean, alg.pr_cov, alg.pr_xx_cov = fm, fP, pm, pP, pC
    smm, smP = alg.backward_pass()
    rel = lambda a, b: float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b))))
    assert within(max(rel(fm, g['ungm_fm']), rel(fP, g['ungm_fc'])), 1e-10, 'marginal smoother: filtered moments, Laplace moments injected')
    assert within(max(rel(pm, g['ungm_pm']), rel(pP, g['ungm_pc']), rel(pC, g['ungm_pxx'])), 1e-10,
                  'marginal smoother: predictive moments kept by forward_pass')
    assert within(max(rel(smm, g['ungm_sm']), rel(smP, g['ungm_sc'])), 1e-10, 'marginal smoother: smoothed moments vs reference')
    assert np.array_equal(smm[:, -2:], fm[:, -2:])                      # the reference's indexing quirk
    # the whole thing through the public calls (own BFGS runs: optimiser paths differ, loose)
    alg2 = ssinf.MarginalizedGaussianProcessKalman(dyn, obs, 'rbf', 'sr')
    f2, _ = alg2.forward_pass(y)
    s2, sP2 = alg2.backward_pass()
    assert s2.shape == (1, T) and np.all(np.isfinite(s2)) and np.all(sP2 > 0) and np.median(np.abs(s2 - g['ungm_sm'])) < 0.05
    # (2) noise as an argument of the dynamics
    dyn = sm.UNGMNATransition(sm.GaussRV(1, mean=np.array([1.0])), sm.GaussRV(1, cov=np.array([[10.0]])))
    alg = ssinf.MarginalizedGaussianProcessKalman(dyn, obs, 'rbf', 'ut')
    assert alg.param_dim == 3 + 2
    worst = 0.0
    for i in range(g['na_theta'].shape[0]):
        alg.x_mean_fi, alg.x_cov_fi = g['na_m'][i], g['na_P'][i]
        ll = alg._param_log_likelihood(g['na_theta'][i], g['na_y'][i], int(g['na_k'][i]))
        m, c = alg._state_posterior_moments(g['na_theta'][i], g['na_y'][i], int(g['na_k'][i]))
        worst = max(worst, abs(ll - g['na_ll'][i]) / max(1.0, abs(g['na_ll'][i])), rel(m, g['na_pm'][i]), rel(c, g['na_pc'][i]))
    assert within(worst, 1e-9, 'marginal filter, noise as an argument of the dynamics: theta-conditioned steps vs reference')
    # all items in one call = one at a time
    alg.x_mean_fi, alg.x_cov_fi = g['na_m'][0], g['na_P'][0]
    mb, cb, llb, st = alg.theta_step(g['na_theta'], g['na_m'][0], g['na_P'][0], g['na_y'][0], int(g['na_k'][0]))
    m0, c0 = alg._state_posterior_moments(g['na_theta'][3], g['na_y'][0], int(g['na_k'][0]))
    assert not st.any() and np.array_equal(mb[3], m0) and np.array_equal(cb[3], c0)
    # the filter runs on such a model (the reference's own forward_pass fails to store its dim_in-sized state mean)
    np.random.seed(0)
    ys = 0.05 * np.cumsum(np.ones((1, 6)), axis=1)
    fm3, fP3 = alg.forward_pass(ys)
    assert fm3.shape == (1, 6) and np.all(np.isfinite(fm3)) and np.all(fP3 > 0)
    with pytest.raises(NotImplementedError):
        ssinf.MarginalizedGaussianProcessKalman(dyn, sm.UNGMNAMeasurement(sm.GaussRV(1), 1), 'rbf', 'ut')


# ---------------------------------------------------------------------------------------------------------------
# simulators on the device (ssmod.py:168-199, 1011-1039), counter-based generator
# ---------------------------------------------------------------------------------------------------------------
def _sim_models(name):
    from ssmtoybox_amd import ssmod as sm
    if name == 'ungm':
        dyn = sm.UNGMTransition(sm.GaussRV(1), sm.GaussRV(1, cov=np.array([[10.0]])))
        obs = sm.UNGMMeasurement(sm.GaussRV(1), 1)
        return dyn, obs, dict(fid_dyn=orc.F_UNGM_DYN, fid_obs=orc.F_UNGM_MEAS)
    if name == 'ungmna':
        dyn = sm.UNGMNATransition(sm.GaussRV(1, mean=np.array([1.0])), sm.GaussRV(1, cov=np.array([[10.0]])))
        obs = sm.UNGMNAMeasurement(sm.GaussRV(1), 1)
        return dyn, obs, dict(fid_dyn=orc.F_UNGMNA_DYN, fid_obs=orc.F_UNGMNA_MEAS, dyn_additive=False, obs_additive=False)
    if name == 'reentry':
        m0 = np.array([6500.4, 349.14, -1.8093, -6.7967, 0.6932])
        P0 = np.diag([1e-6, 1e-6, 1e-6, 1e-6, 1.0])
        dyn = sm.ReentryVehicle2DTransition(sm.GaussRV(5, m0, P0), sm.GaussRV(3, cov=np.diag([2.4064e-5, 2.4064e-5, 1e-6])))
        obs = sm.Radar2DMeasurement(sm.GaussRV(2, cov=np.diag([1e-6, 0.17e-6])), 5, radar_loc=[6374.0, 0.0])
        return dyn, obs, dict(fid_dyn=orc.F_REENTRY2D_DYN, fid_obs=orc.F_RADAR2D_MEAS, p_dyn=(0.1,), p_obs=(6374.0, 0.0),
                              G=dyn.noise_gain)
    a = np.array([[0.5, 0.1], [0.1, 0.3]])
    dyn = sm.ConstantTurnRateSpeed(sm.GaussRV(5, mean=np.array([10.0, 10.0, 5.0, 0.3, 0.1]), cov=0.1 * np.eye(5)),
                                   sm.GaussRV(2, cov=a))
    obs = sm.Radar2DMeasurement(sm.GaussRV(2, cov=np.diag([0.3, 0.03])), 5)
    return dyn, obs, dict(fid_dyn=orc.F_CTRS_DYN, fid_obs=orc.F_RADAR2D_MEAS, p_dyn=(0.05,), p_obs=(0.0, 0.0),
                          dyn_additive=False)


def _download_sim(d_x, d_y, ld, D, Y, T, B):
    x = d_x.download((T, D, ld))[:, :, :B].transpose(1, 0, 2)
    y = d_y.download((T, Y, ld))[:, :, :B].transpose(1, 0, 2)
    d_x.free()
    d_y.free()
    return x, y


@pytest.mark.parametrize('name', ['ungm', 'ungmna', 'reentry', 'ctrs'])
def test_simulate_matches_generator_restatement(amd, name):
    from ssmtoybox_amd import ssmod as sm
    dyn, obs, kw = _sim_models(name)
    T, B, seed, off = 6, 130, 20261003, 5000000000       # the offset exercises the high counter word
    d_x, d_y, ld = sm.simulate_dev(dyn, obs, T, B, seed=seed, traj_offset=off)
    x, y = _download_sim(d_x, d_y, ld, dyn.dim_state, obs.dim_out, T, B)
    ox, oy = orc.simulate(steps=T, B=B, x0_mean=dyn.init_rv.mean, x0_cov=dyn.init_rv.cov, q_mean=dyn.noise_rv.mean,
                          q_cov=dyn.noise_rv.cov, r_mean=obs.noise_rv.mean, r_cov=obs.noise_rv.cov, seed=seed,
                          traj_offset=off, **kw)
    assert np.array_equal(x[:, 0] != 0, ox[:, 0] != 0)
    assert rel_err(x[:, 0], ox[:, 0]) < 1e-13            # initial draw: generator + Box-Muller only
    # six steps of UNGM amplify a last-bit difference of log / sincos by up to 25^5
    assert rel_err(x, ox) < 1e-8 and rel_err(y, oy) < 1e-8, name
    # sharding invariance: two shards with their global offsets reproduce the whole batch bit for bit
    h = 70
    xa, ya = _download_sim(*sm.simulate_dev(dyn, obs, T, h, seed=seed, traj_offset=off), dyn.dim_state, obs.dim_out, T, h)
    xb, yb = _download_sim(*sm.simulate_dev(dyn, obs, T, B - h, seed=seed, traj_offset=off + h), dyn.dim_state,
                           obs.dim_out, T, B - h)
    assert np.array_equal(np.concatenate((xa, xb), axis=2), x) and np.array_equal(np.concatenate((ya, yb), axis=2), y)
    # the reference's two-call interface gives the same numbers
    x2 = dyn.simulate_discrete(T, B, seed=seed, traj_offset=off)
    y2 = obs.simulate_measurements(x2, seed=seed, traj_offset=off)
    assert np.array_equal(x2, x) and np.array_equal(y2, y)
    assert not np.array_equal(dyn.simulate_discrete(T, B, seed=seed + 1, traj_offset=off), x)


def test_simulate_long_run_one_step_residuals(amd):
    """T = 100: every step obeys x[k] = f(x[k-1], k-1) + G q[k-1], y[k] = h(x[k], k+1) + r[k] with the generator's
    q, r (a check that does not suffer from the chaotic amplification of whole-trajectory comparisons)."""
    from ssmtoybox_amd import ssmod as sm
    dyn, obs, _ = _sim_models('ungm')
    T, B, seed = 100, 256, 99
    x, y = _download_sim(*sm.simulate_dev(dyn, obs, T, B, seed=seed), 1, 1, T, B)
    traj = np.arange(B)
    for k in (0, 1, 37, 98):
        q = orc.gauss_vectors(seed, traj, k, 1, np.zeros(1), np.sqrt(10.0) * np.eye(1))
        f = 0.5 * x[0, k] + 25 * x[0, k] / (1 + x[0, k] ** 2) + 8 * np.cos(1.2 * k)
        assert np.allclose(x[0, k + 1], f + q[0], rtol=1e-12, atol=1e-12)
    for k in (0, 50, 99):
        r = orc.gauss_vectors(seed, traj, k, 2, np.zeros(1), np.eye(1))
        assert np.allclose(y[0, k], 0.05 * x[0, k] ** 2 + r[0], rtol=1e-12, atol=1e-12)


def test_simulate_statistics_match_numpy_streams(amd):
    """Statistical parity with an np.random simulation of the same model (what the reference's simulators draw from):
    per-step mean and variance of states and measurements over 2e5 trajectories agree within sampling error."""
    from ssmtoybox_amd import ssmod as sm
    dyn, obs, _ = _sim_models('ungm')
    T, B = 12, 200000
    x, y = _download_sim(*sm.simulate_dev(dyn, obs, T, B, seed=7), 1, 1, T, B)
    rng = np.random.default_rng(123)
    xr = np.zeros((T, B))
    xr[0] = rng.standard_normal(B)
    for k in range(1, T):
        xr[k] = 0.5 * xr[k - 1] + 25 * xr[k - 1] / (1 + xr[k - 1] ** 2) + 8 * np.cos(1.2 * (k - 1)) + \
            np.sqrt(10.0) * rng.standard_normal(B)
    yr = 0.05 * xr ** 2 + rng.standard_normal((T, B))
    for dev, ref in ((x[0], xr), (y[0], yr)):
        se_mean = np.sqrt((dev.var(axis=1) + ref.var(axis=1)) / B)
        assert np.all(np.abs(dev.mean(axis=1) - ref.mean(axis=1)) < 5 * se_mean)
        m4 = ((ref - ref.mean(axis=1, keepdims=True)) ** 4).mean(axis=1)
        se_var = np.sqrt(2 * (m4 - ref.var(axis=1) ** 2) / B)
        assert np.all(np.abs(dev.var(axis=1) - ref.var(axis=1)) < 5 * se_var)
    # a filter run on device-generated data behaves like on host-generated data
    from ssmtoybox_amd import ssinf
    alg = ssinf.UnscentedKalman(dyn, obs)
    fm, _ = alg.forward_pass_batch(y[:, :, :5000], raise_on_failure=False)
    fr, _ = alg.forward_pass_batch(yr[None, :, :5000], raise_on_failure=False)
    # NB the reference's convention: y[k] belongs to x[k] although the filter's first prediction runs from the prior
    e_dev = np.sqrt(np.nanmean((fm[0] - x[0, :, :5000]) ** 2))
    e_ref = np.sqrt(np.nanmean((fr[0] - xr[:, :5000]) ** 2))
    assert abs(e_dev - e_ref) < 0.1 * e_ref


def _oracle_rv(rv):
    from ssmtoybox_amd import ssmod as sm
    if isinstance(rv, sm.StudentRV):
        return orc.student_rv(rv.mean, rv.scale, rv.dof)
    if isinstance(rv, sm.GaussianMixtureRV):
        return orc.mixture_rv(rv.means, rv.covs, rv.alphas)
    return orc.gauss_rv(rv.mean, rv.cov)


def test_simulate_student_and_mixture_noise_match_restatement(amd):
    """Student-t and Gaussian-mixture random variables in the simulators (utils.py:254-299, 349-382; StudentRV :628-674,
    GaussianMixtureRV research/tpq/tpq_base.py:13-32) - the reference's heavy-tailed studies (research/tpq/tpq_ungm.py:40-66):
    device draws against the oracle's restatement of the generator, shard invariance, and the two-call interface."""
    from ssmtoybox_amd import ssmod as sm
    nu = 4.0
    cases = {
        'student': (sm.UNGMTransition(sm.StudentRV(1, scale=(nu - 2) / nu * np.eye(1), dof=nu),
                                      sm.StudentRV(1, scale=(nu - 2) / nu * 10 * np.eye(1), dof=nu)),
                    sm.UNGMMeasurement(sm.StudentRV(1, scale=(nu - 2) / nu * np.eye(1), dof=nu), 1)),
        'mixture': (sm.UNGMTransition(sm.GaussRV(1), sm.GaussianMixtureRV(1, covs=(10 * np.eye(1), 100 * np.eye(1)), alphas=(0.8, 0.2))),
                    sm.UNGMMeasurement(sm.GaussianMixtureRV(1, means=(np.zeros(1), 0.5 * np.ones(1)),
                                                            covs=(0.01 * np.eye(1), np.eye(1)), alphas=(0.9, 0.1)), 1)),
    }
    T, B, seed, off = 6, 200, 77, 4000000000
    for name, (dyn, obs) in cases.items():
        x, y = _download_sim(*sm.simulate_dev(dyn, obs, T, B, seed=seed, traj_offset=off), 1, 1, T, B)
        ox, oy = orc.simulate_rv(orc.F_UNGM_DYN, orc.F_UNGM_MEAS, T, B, _oracle_rv(dyn.init_rv), _oracle_rv(dyn.noise_rv),
                                 _oracle_rv(obs.noise_rv), seed=seed, traj_offset=off)
        assert within(rel_err(x[:, 0], ox[:, 0]), 1e-12, 'simulate ' + name + ': initial draw vs generator restatement')
        assert within(max(rel_err(x, ox), rel_err(y, oy)), 1e-8, 'simulate ' + name + ': 6 steps vs generator restatement')
        h = 70
        xa, ya = _download_sim(*sm.simulate_dev(dyn, obs, T, h, seed=seed, traj_offset=off), 1, 1, T, h)
        xb, yb = _download_sim(*sm.simulate_dev(dyn, obs, T, B - h, seed=seed, traj_offset=off + h), 1, 1, T, B - h)
        assert np.array_equal(np.concatenate((xa, xb), axis=2), x) and np.array_equal(np.concatenate((ya, yb), axis=2), y)
        x2 = dyn.simulate_discrete(T, B, seed=seed, traj_offset=off)
        assert np.array_equal(x2, x) and np.array_equal(obs.simulate_measurements(x2, seed=seed, traj_offset=off), y)


def test_simulate_student_and_mixture_statistics(amd):
    """Statistical parity with the reference's samplers (np.random.gamma / multivariate_normal / choice streams):
    Student-t draws against the t distribution (Kolmogorov-Smirnov) and NumPy's multivariate_t recipe, mixture draws
    against the component proportions and the mixture's moments, 2e5 draws each."""
    from scipy import stats
    from ssmtoybox_amd import ssmod as sm
    B = 200000
    nu, scale = 5.0, np.array([[2.0, 0.6], [0.6, 1.0]])
    obs = sm.Radar2DMeasurement(sm.StudentRV(2, mean=np.array([1.0, -2.0]), scale=scale, dof=nu), 5)     # additive: y = h(x) + r
    x = np.tile(np.array([6500.0, 350.0, -1.8, -6.8, 0.7])[:, None, None], (1, 1, B))
    r = obs.simulate_measurements(x, seed=11)[:, 0] - np.array([np.hypot(6500.0, 350.0), np.arctan2(350.0, 6500.0)])[:, None]
    L = np.linalg.cholesky(scale)
    w = np.linalg.solve(L, r - np.array([[1.0], [-2.0]]))           # whitened: independent-looking t marginals
    for i in range(2):
        assert stats.kstest(w[i], 't', args=(nu,)).pvalue > 1e-3
    rng = np.random.default_rng(5)
    ref = (rng.multivariate_normal(np.zeros(2), scale, B) / np.sqrt(rng.gamma(nu / 2, 2 / nu, B))[:, None]).T   # utils.py:379-382
    assert np.allclose(np.cov(r), np.cov(ref), rtol=0.1) and np.allclose(np.cov(r), scale * nu / (nu - 2), rtol=0.1)
    assert abs(stats.kurtosis(w[0]) - stats.kurtosis(np.linalg.solve(L, ref)[0])) < 3.0          # heavy tails, both
    assert stats.kurtosis(w[0]) > 2.0
    # mixture: glint noise as in research/tpq/tpq_constant_velocity.py:33
    alphas, covs = np.array([0.85, 0.15]), (0.01 * np.eye(1), 4.0 * np.eye(1))
    obs = sm.UNGMMeasurement(sm.GaussianMixtureRV(1, covs=covs, alphas=alphas), 1)
    r = obs.simulate_measurements(np.zeros((1, 1, B)), seed=12)[0, 0]
    var = alphas[0] * 0.01 + alphas[1] * 4.0
    assert abs(r.mean()) < 5 * np.sqrt(var / B) and abs(r.var() - var) < 0.03 * var
    inner = np.mean(np.abs(r) < 0.3)            # within 3 sigma of the narrow component: ~ alpha_0 + alpha_1 P(|N(0,4)| < 0.3)
    assert abs(inner - (alphas[0] * stats.norm.cdf(3) * 1 + alphas[0] * (stats.norm.cdf(3) - 1) +
                        alphas[1] * (2 * stats.norm.cdf(0.15) - 1))) < 5e-3


@pytest.mark.parametrize('name', ['reentry2d', 'reentry1d', 'ctrs'])
def test_simulate_continuous(amd, name):
    """TransitionModel.simulate_continuous (ssmod.py:201-244): Euler-Maruyama over dyn_fcn_cont for the three models that
    define it, against the oracle's restatement with the same generator, against the model's own host dyn_fcn_cont driven by
    the generator's noise (one-step residuals), and refused for the models whose dyn_fcn_cont is `pass` in the reference."""
    from ssmtoybox_amd import ssmod as sm
    if name == 'reentry2d':
        m0 = np.array([6500.4, 349.14, -1.8093, -6.7967, 0.6932])
        dyn = sm.ReentryVehicle2DTransition(sm.GaussRV(5, m0, np.diag([1e-6, 1e-6, 1e-6, 1e-6, 1e-3])),
                                            sm.GaussRV(3, cov=np.diag([2.4064e-5, 2.4064e-5, 1e-6])))
        fid = orc.F_REENTRY2D_DYN
    elif name == 'reentry1d':
        dyn = sm.ReentryVehicle1DTransition(sm.GaussRV(3, np.array([90.0, 6.0, 1.5]), np.diag([0.0929, 1.4865, 1e-4])),
                                            sm.GaussRV(3, cov=np.diag([1e-4, 1e-4, 1e-6])))
        fid = orc.F_REENTRY1D_DYN
    else:
        dyn = sm.ConstantTurnRateSpeed(sm.GaussRV(5, np.array([0.0, 0.0, 10.0, 0.3, 0.05]), 0.01 * np.eye(5)),
                                       sm.StudentRV(2, scale=0.1 * np.eye(2), dof=4.0))
        fid = orc.F_CTRS_DYN
    dt, duration, B, seed, off = 0.05, 2.0, 150, 5, 12345678901
    x = dyn.simulate_continuous(duration, dt, B, seed=seed, traj_offset=off)
    T = int(np.floor(duration / dt))
    assert x.shape == (dyn.dim_state, T, B)
    ox, _ = orc.simulate_rv(fid, None, T, B, _oracle_rv(dyn.init_rv), _oracle_rv(dyn.noise_rv), None, seed=seed, traj_offset=off,
                            continuous_dt=dt)
    assert within(rel_err(x, ox), 1e-9, 'simulate_continuous ' + name + ' vs generator restatement')
    # one-step residuals with the model's own dyn_fcn_cont (host NumPy) and the generator's noise
    traj = np.arange(B, dtype=np.uint64) + np.uint64(off)
    for k in (1, 7, T - 1):
        q = (np.sqrt(dt) / dt) * orc.sample_rv(_oracle_rv(dyn.noise_rv), seed, traj, k, 1)
        step = np.stack([x[:, k - 1, b] + dt * dyn.dyn_fcn_cont(x[:, k - 1, b], q[:, b], k - 1) for b in range(B)], axis=1)
        assert np.allclose(x[:, k], step, rtol=1e-12, atol=1e-12)
    # measurements of a continuous trajectory, as research/gpq/gpq_tracking.py:144-146 takes them
    if name == 'reentry2d':
        obs = sm.Radar2DMeasurement(sm.GaussRV(2, cov=np.diag([1e-6, 0.17e-6])), 5)
        y = obs.simulate_measurements(x, seed=seed, traj_offset=off)
        assert y.shape == (2, T, B) and np.allclose(y[0], np.hypot(x[0], x[1]), atol=1e-2)
    with pytest.raises(amd.SsmqError):
        sm.UNGMTransition(sm.GaussRV(1), sm.GaussRV(1)).simulate_continuous(1.0, 0.1, 4)


# ---------------------------------------------------------------------------------------------------------------
# error statistics reduced on the device (utils.py:18-148 aggregated as research/tpq/tpq_base.py:154-172)
# ---------------------------------------------------------------------------------------------------------------
def _lib_buffer(host):
    from ssmtoybox_amd import _lib
    d = _lib.DeviceBuffer(host.nbytes)
    d.upload(host)
    return d


def _planes(a, ld):
    """(D, T, B) or (D, D, T, B) -> DeviceBuffer of planes [T][D..][ld]."""
    from ssmtoybox_amd import _lib
    B = a.shape[-1]
    t_ax = a.ndim - 2
    src = np.moveaxis(a, t_ax, 0).reshape(a.shape[t_ax], -1, B)
    buf = np.zeros((src.shape[0], src.shape[1], ld))
    buf[:, :, :B] = src
    d = _lib.DeviceBuffer(buf.nbytes)
    d.upload(buf)
    return d


@pytest.mark.parametrize('tag', ['d1', 'd3', 'd6'])
def test_error_sums_golden(amd, golden, tag):
    from ssmtoybox_amd import mcshard, _lib
    g = golden('g7_metrics')
    x, m, P = g[tag + '_x'], g[tag + '_m'], g[tag + '_P']
    D, T, M = m.shape
    ld = 64
    d_x, d_m, d_P = _planes(x, ld), _planes(m, ld), _planes(P, ld)
    s1 = mcshard.device_error_sums(D, M, ld, T, d_x, d_m, d_P)
    assert np.allclose(s1['se'], g[tag + '_se'].sum(axis=2).T, rtol=1e-12)
    assert np.allclose(s1['rmse'], g[tag + '_rmse'].sum(axis=1), rtol=1e-12)
    assert np.allclose(s1['nll'], g[tag + '_nll'].sum(axis=1), rtol=1e-11)
    assert np.allclose(s1['mse'] / M, g[tag + '_mse'].transpose(2, 0, 1), rtol=1e-11, atol=1e-13)
    assert np.all(s1['n_ok'] == M) and np.all(s1['n_pd'] == M)
    s2 = mcshard.device_lcr_sums(D, M, ld, T, d_x, d_m, d_P, s1['mse'] / M)
    assert np.allclose(s2['lcr'], g[tag + '_lcr'].sum(axis=1), rtol=1e-9, atol=1e-9) and np.all(s2['n'] == M)
    # status mask: trajectory 1 failed in the filter -> left out of every sum, as the oracle does
    st = np.zeros(ld, dtype=np.int32)
    st[1] = 3
    d_st = _lib.DeviceBuffer(st.nbytes)
    d_st.upload(st)
    ok = st[:M] == 0
    s3, o3 = mcshard.device_error_sums(D, M, ld, T, d_x, d_m, d_P, d_st), orc.error_sums(x, m, P, ok)
    for k in ('se', 'rmse', 'nll', 'mse', 'n_ok', 'n_pd'):
        assert np.allclose(s3[k], o3[k], rtol=1e-11, atol=1e-12), k
    for buf in (d_x, d_m, d_P, d_st):
        buf.free()
    if tag + '_Pi' in g:
        # covariances that are not positive definite: the reference's formulas still apply (inv / slogdet; SVD square
        # root) - second pass of the device reduction (k_indef_sums), against the reference's own numbers
        Pi, flip = g[tag + '_Pi'], g[tag + '_flip']
        assert flip.any()
        d_x, d_m, d_Pi = _planes(x, ld), _planes(m, ld), _planes(Pi, ld)
        s4 = mcshard.device_error_sums(D, M, ld, T, d_x, d_m, d_Pi)
        assert np.all(s4['n_ok'] == M) and np.all(s4['n_pd'] == M)
        assert np.allclose(s4['nll'], g[tag + '_nlli'].sum(axis=1), rtol=1e-9, atol=1e-9)
        assert np.allclose(s4['se'], s1['se']) and np.allclose(s4['mse'], s1['mse'])
        s5 = mcshard.device_lcr_sums(D, M, ld, T, d_x, d_m, d_Pi, s4['mse'] / M)
        assert np.all(s5['n'] == M)
        assert np.allclose(s5['lcr'], g[tag + '_lcri'].sum(axis=1), rtol=1e-8, atol=1e-8)
        for buf in (d_x, d_m, d_Pi):
            buf.free()


def test_error_sums_large_batch_properties(amd):
    """Size-independent checks at a ragged B that spans several reduction chunks: additivity over a split of the batch,
    covariances that are not positive definite, determinism."""
    from ssmtoybox_amd import mcshard
    rng = np.random.default_rng(11)
    D, T, B = 5, 3, 5003
    ld = (B + 63) // 64 * 64
    x = rng.standard_normal((D, T, B))
    m = x + 0.5 * rng.standard_normal((D, T, B))
    a = rng.standard_normal((D, D, T, B)) / np.sqrt(D)
    P = np.einsum('ijtb,kjtb->iktb', a, a) + 0.2 * np.eye(D)[:, :, None, None]
    bad = rng.choice(B, 17, replace=False)
    P[..., 1, bad] = -np.eye(D)[:, :, None]
    d_x, d_m, d_P = _planes(x, ld), _planes(m, ld), _planes(P, ld)
    s = mcshard.device_error_sums(D, B, ld, T, d_x, d_m, d_P)
    s_again = mcshard.device_error_sums(D, B, ld, T, d_x, d_m, d_P)
    assert all(np.array_equal(s[k], s_again[k]) for k in s)
    assert np.all(s['n_pd'] == B) and np.all(s['n_ok'] == B)      # -I is not positive definite, but it is not singular
    dx = x - m
    assert np.allclose(s['se'], (dx ** 2).sum(axis=2).T, rtol=1e-12)
    assert np.allclose(s['mse'], np.einsum('itb,jtb->tij', dx, dx), rtol=1e-11, atol=1e-9)
    sample = rng.choice(B, 40, replace=False)
    o = orc.error_sums(x[..., sample], m[..., sample], P[..., sample])
    dd = [_planes(v[..., sample], 64) for v in (x, m, P)]
    ssub = mcshard.device_error_sums(D, 40, 64, T, *dd)
    for k in o:
        assert np.allclose(ssub[k], o[k], rtol=1e-11, atol=1e-12), k
    # additivity: sums of two halves (separate launches over sub-batches) = sums of the whole
    h = 2500
    d1 = [_planes(v[..., :h], (h + 63) // 64 * 64) for v in (x, m, P)]
    d2 = [_planes(v[..., h:], (B - h + 63) // 64 * 64) for v in (x, m, P)]
    sa = mcshard.device_error_sums(D, h, (h + 63) // 64 * 64, T, *d1)
    sb = mcshard.device_error_sums(D, B - h, (B - h + 63) // 64 * 64, T, *d2)
    for k in s:
        assert np.allclose(sa[k] + sb[k], s[k], rtol=1e-12, atol=1e-12), k
    mse = s['mse'] / B
    l_all = mcshard.device_lcr_sums(D, B, ld, T, d_x, d_m, d_P, mse)
    la = mcshard.device_lcr_sums(D, h, (h + 63) // 64 * 64, T, *d1, mse)
    lb = mcshard.device_lcr_sums(D, B - h, (B - h + 63) // 64 * 64, T, *d2, mse)
    assert np.allclose(la['lcr'] + lb['lcr'], l_all['lcr'], rtol=1e-11) and np.all(l_all['n'] == B)
    osub = orc.lcr_sums(x[..., sample], m[..., sample], P[..., sample], mse + 1e-6 * np.eye(D))
    lsub = mcshard.device_lcr_sums(D, 40, 64, T, *dd, mse)
    assert np.allclose(lsub['lcr'], osub['lcr'], rtol=1e-10) and np.array_equal(lsub['n'], osub['n'])


def test_error_sums_generic_dimension(amd):
    """D = 10 takes the run-time-sized kernel."""
    from ssmtoybox_amd import mcshard
    rng = np.random.default_rng(12)
    D, T, B = 10, 2, 70
    x = rng.standard_normal((D, T, B))
    m = x + 0.5 * rng.standard_normal((D, T, B))
    a = rng.standard_normal((D, D, T, B)) / np.sqrt(D)
    P = np.einsum('ijtb,kjtb->iktb', a, a) + 0.2 * np.eye(D)[:, :, None, None]
    dd = [_planes(v, 128) for v in (x, m, P)]
    s, o = mcshard.device_error_sums(D, B, 128, T, *dd), orc.error_sums(x, m, P)
    for k in o:
        assert np.allclose(s[k], o[k], rtol=1e-11, atol=1e-12), k
    l, ol = mcshard.device_lcr_sums(D, B, 128, T, *dd, s['mse'] / B), orc.lcr_sums(x, m, P, s['mse'] / B + 1e-6 * np.eye(D))
    assert np.allclose(l['lcr'], ol['lcr'], rtol=1e-10) and np.array_equal(l['n'], ol['n'])


def test_empty_inputs_of_the_caller_side_entry_points(amd):
    """B = 0 / T = 0 / P = 0 through the entry points around the path: no launch, no error, well-formed outputs."""
    from ssmtoybox_amd import ssinf, ssmod as sm, mcshard, _lib
    dyn = sm.UNGMNATransition(sm.GaussRV(1, mean=np.array([1.0])), sm.GaussRV(1, cov=np.array([[10.0]])))
    obs = sm.UNGMNAMeasurement(sm.GaussRV(1), 1)
    alg = ssinf.UnscentedKalman(dyn, obs)
    fm, fP = alg.forward_pass_batch(np.zeros((1, 5, 0)))
    assert fm.shape == (1, 5, 0) and fP.shape == (1, 1, 5, 0)
    fm, fP = alg.forward_pass_batch(np.zeros((1, 0, 3)))
    assert fm.shape == (1, 0, 3)
    d = _lib.DeviceBuffer(8)
    s = mcshard.device_error_sums(2, 0, 0, 4, d, d, d)
    assert s['se'].shape == (4, 2) and not s['se'].any() and not s['n_ok'].any()
    assert mcshard.device_error_sums(2, 0, 0, 0, d, d, d)['mse'].shape == (0, 2, 2)
    assert mcshard.device_lcr_sums(2, 0, 0, 4, d, d, d, np.tile(np.eye(2), (4, 1, 1)))['lcr'].shape == (4,)
    d.free()
    dyn2 = sm.UNGMTransition(sm.GaussRV(1), sm.GaussRV(1, cov=np.array([[10.0]])))
    obs2 = sm.UNGMMeasurement(sm.GaussRV(1), 1)
    assert dyn2.simulate_discrete(5, 0).shape == (1, 5, 0) and dyn2.simulate_discrete(0, 3).shape == (1, 0, 3)
    assert obs2.simulate_measurements(np.zeros((1, 4, 0))).shape == (1, 4, 0)
    mg = ssinf.MarginalizedGaussianProcessKalman(dyn2, obs2, 'rbf', 'sr')
    pm, pc, ll, st = mg.theta_step(np.zeros((0, mg.param_dim)), np.zeros(1), np.eye(1), np.zeros(1), 0)
    assert pm.shape == (0, 1) and pc.shape == (0, 1, 1) and ll.shape == (0,) and st.shape == (0,)
    # argument errors come back as SsmqError, not as a crash
    d = _lib.DeviceBuffer(8 * 64 * 8)
    with pytest.raises(_lib.SsmqError):
        mcshard.device_error_sums(2, 10, 5, 1, d, d, d)          # pitch smaller than the batch
    with pytest.raises(_lib.SsmqError):
        mcshard.device_error_sums(40, 10, 64, 1, d, d, d)        # dimension above SSMQ_MAX_DIM
    d.free()


# ---------------------------------------------------------------------------------------------------------------
# full-size batches (BASELINE.json configs): oracle on a sample + size-independent properties
# ---------------------------------------------------------------------------------------------------------------
def synthetic_reentry6(B, seed=2):
    """reentry-shaped 6-D batch."""
    rng = np.random.default_rng(seed)
    m0 = np.array([6500.4, 349.14, -1.8093, -6.7967, 0.6932, 0.0])
    p0 = np.array([1e-6, 1e-6, 1e-6, 1e-6, 1.0, 1e-2])
    means = m0 + rng.standard_normal((B, 6)) * np.sqrt(p0)
    a = rng.standard_normal((B, 6, 6)) / np.sqrt(6)
    s = np.sqrt(p0)
    covs = np.einsum('i,bij,bkj,k->bik', s, a, a, s) + 1e-6 * np.diag(p0)
    return means, 0.5 * (covs + covs.transpose(0, 2, 1))


@pytest.mark.parametrize('ell', [3.0, 25.0])
def test_gpq_d6_full_batch(amd, ell):
    from ssmtoybox_amd import ssmod as sm
    B = 100000
    means, covs = synthetic_reentry6(B)
    par = gp_par(6, ell)
    tf = amd.GaussianProcessTransform(6, 6, par, 'rbf', 'ut')
    w = orc.gp_weights(par, orc.points_ut(6))
    tf.wm, tf.Wc, tf.Wcc, tf.model.model_var = w['wm'], w['Wc'], w['Wcc'], w['model_var']   # identical weights
    f = sm.ReentryVehicle2DBiasTransition(dt=0.1).dyn_eval
    assert 'k_apply_small<D=6,E=6,N=13' in tf.kernel_name(f)
    mf, cf, cfx, st = tf.apply_batch(f, means, covs, 0.0, return_status=True)
    assert not st.any() and np.all(np.isfinite(cf))
    assert np.array_equal(cf, cf.transpose(0, 2, 1))
    # oracle on a sample of the batch
    idx = np.random.default_rng(5).choice(B, 200, replace=False)
    for i in idx:
        ref = orc.apply_bq(orc.F_REENTRY2D_BIAS_DYN, means[i], covs[i], 0, orc.points_ut(6), w, (0.1,))
        assert_moments_close((mf[i], cf[i], cfx[i]), ref, covs[i], what=('d6', ell, i))
    # properties: trajectories are independent (a permuted batch gives the permuted result, bit for bit) ...
    perm = np.random.default_rng(6).permutation(B)[:4096]
    mf2, cf2, cfx2 = tf.apply_batch(f, means[perm], covs[perm], 0.0)
    assert np.array_equal(mf2, mf[perm]) and np.array_equal(cf2, cf[perm]) and np.array_equal(cfx2, cfx[perm])
    # ... and the pass-through sixth state is integrated exactly when sum(wm) = 1:  E[x6] = m6 sum(wm) + L6. xi wm
    pts = orc.points_ut(6)
    chol = np.linalg.cholesky(covs[:1000])
    x6 = means[:1000, 5, None] + np.einsum('bk,kn->bn', chol[:, 5, :], pts)
    assert np.allclose(mf[:1000, 5], x6.dot(w['wm']), rtol=1e-12, atol=1e-14)


def test_fast_paths_match_dense(amd, monkeypatch):
    """SSMQ_OPT_LDL / SSMQ_OPT_UT kernels (chosen per handle on the host) against the dense kernels and the oracle."""
    from ssmtoybox_amd import ssmod as sm
    B = 4096
    means, covs = synthetic_reentry6(B)
    f6 = sm.ReentryVehicle2DBiasTransition(dt=0.1).dyn_eval
    f5 = sm.ReentryVehicle2DTransition(dt=0.1).dyn_eval
    h5 = sm.Radar2DMeasurement(sm.GaussRV(2), 5).meas_eval
    # (OPT=7: the weights are also reflection-symmetric to 2e-13 - length scale 3; at length scale 25 the ill-conditioned kernel
    # matrix leaves an asymmetry of ~5e-7 in Wc and the host keeps OPT=3)
    cases = [(lambda: amd.GaussianProcessTransform(6, 6, gp_par(6, 3.0)), f6, 6, 'OPT=7'),
             (lambda: amd.GaussianProcessTransform(5, 5, gp_par(5, 25.0)), f5, 5, 'OPT=3'),
             (lambda: amd.StudentTProcessTransform(5, 5, gp_par(5, 3.0)), f5, 5, 'OPT=2'),
             (lambda: amd.UnscentedTransform(5), f5, 5, 'OPT=2'),
             (lambda: amd.GaussianProcessTransform(5, 2, gp_par(5, 3.0)), h5, 5, 'OPT=7'),
             (lambda: amd.GaussianProcessTransform(5, 5, gp_par(5, 3.0), 'rbf', 'sr'), f5, 5, 'OPT=0')]
    for make, f, d, tag in cases:
        if tag == 'OPT=7' and 'SSMQ_NO_SYM' in os.environ:         # (tools/alt_paths.sh)
            tag = 'OPT=3'
        monkeypatch.delenv('SSMQ_NO_FASTPATH', raising=False)
        tf = make()
        assert tag in tf.kernel_name(f), tf.kernel_name(f)
        fast = tf.apply_batch(f, means[:, :d], covs[:, :d, :d], 0.0)
        monkeypatch.setenv('SSMQ_NO_FASTPATH', '1')
        tf2 = make()
        assert 'OPT=0' in tf2.kernel_name(f)
        dense = tf2.apply_batch(f, means[:, :d], covs[:, :d, :d], 0.0)
        monkeypatch.delenv('SSMQ_NO_FASTPATH')
        for i in range(0, B, 97):
            assert_moments_close([a[i] for a in fast], [a[i] for a in dense], covs[i, :d, :d], what=(tag, i))
        if tag == 'OPT=7':       # ... and against the LDL' kernel the symmetric one replaces (SSMQ_NO_SYM: tools/alt_paths.sh)
            monkeypatch.setenv('SSMQ_NO_SYM', '1')
            tf3 = make()
            assert 'OPT=3' in tf3.kernel_name(f)
            ldl = tf3.apply_batch(f, means[:, :d], covs[:, :d, :d], 0.0)
            monkeypatch.delenv('SSMQ_NO_SYM')
            for i in range(0, B, 97):
                assert_moments_close([a[i] for a in fast], [a[i] for a in ldl], covs[i, :d, :d], what=(tag, 'vs OPT=3', i))


def test_ungm_gpq_full_batch(amd):
    """Config C2 shape: D = 1, N = 3, B = 1e4, per-trajectory time index."""
    from ssmtoybox_amd import ssmod as sm
    B = 10000
    rng = np.random.default_rng(1)
    means = rng.standard_normal((B, 1)) * 3
    covs = (0.1 + rng.random((B, 1, 1)) * 5)
    times = rng.integers(0, 100, B).astype(float)
    par = np.array([[1.0, 3.0]])
    tf = amd.GaussianProcessTransform(1, 1, par)
    w = orc.gp_weights(par, orc.points_ut(1))
    tf.wm, tf.Wc, tf.Wcc, tf.model.model_var = w['wm'], w['Wc'], w['Wcc'], w['model_var']
    for mod, fid in ((sm.UNGMTransition(), orc.F_UNGM_DYN), (sm.UNGMMeasurement(sm.GaussRV(1), 1), orc.F_UNGM_MEAS)):
        f = mod.dyn_eval if fid == orc.F_UNGM_DYN else mod.meas_eval
        mf, cf, cfx = tf.apply_batch(f, means, covs, times)
        for i in range(0, B, 37):
            ref = orc.apply_bq(fid, means[i], covs[i], times[i], orc.points_ut(1), w)
            assert_moments_close((mf[i], cf[i], cfx[i]), ref, covs[i], what=('ungm', fid, i))


def test_bsq_d10(amd, golden):
    """Config C5 shapes: D = E = 10 with N = 21 (unisolvent UT) and N = 201 (fully-symmetric degree 5)."""
    g = golden('g2_bs_weights')
    rng = np.random.default_rng(9)
    B = 64
    means = rng.standard_normal((B, 10))
    a = rng.standard_normal((B, 10, 10)) / np.sqrt(10)
    covs = np.einsum('bij,bkj->bik', a, a) + 0.1 * np.eye(10)

    def f(x, par):                                        # smooth 10-D test integrand, evaluated on the host
        return np.concatenate((np.sin(x[:5]) + x[5:] ** 2, x[5:] * np.cos(x[:5])))
    for tag, pstr, ppar in (('d10_ut', 'ut', None), ('d10_fs5_td2', 'fs', {'degree': 5})):
        t = 'bs_' + tag
        tf = amd.BayesSardTransform(10, 10, gp_par(10, 3.0), g[t + '_mi'], pstr, ppar)
        w = dict(wm=g[t + '_wm'], Wc=g[t + '_Wc'], Wcc=g[t + '_Wcc'], model_var=float(g[t + '_mv']))
        tf.wm, tf.Wc, tf.Wcc, tf.model.model_var = w['wm'], w['Wc'], w['Wcc'], w['model_var']
        mf, cf, cfx = tf.apply_batch(f, means, covs, 0.0)
        pts = g[t + '_pts']
        for i in range(0, B, 7):
            chol = np.linalg.cholesky(covs[i])
            fx = np.apply_along_axis(f, 0, means[i][:, None] + chol.dot(pts), None)
            ref = orc.moments_bq(fx, chol, w['wm'], w['Wc'], w['Wcc'], w['model_var'])
            assert_moments_close((mf[i], cf[i], cfx[i]), ref, covs[i], what=(tag, i))


@pytest.mark.parametrize('tag,pstr,ppar,B', [('d10_fs5_td2', 'fs', {'degree': 5}, 10000), ('d10_ut', 'ut', None, 100000)])
def test_bsq_d10_full_batch(amd, golden, tag, pstr, ppar, B):
    """BASELINE configs[4] at the sizes bench.py times (SURVEY 8d's restatement: Bayes-Sard, D = E = 10, fully-symmetric
    degree-5 rule N = 201 at B = 1e4 - evaluation pass + matrix-core GEMM with the covariance epilogue - and the unisolvent
    unscented set N = 21 at B = 1e5 on k_apply_tile), device integrand, the reference's weights injected: 200 sampled
    trajectories against the oracle, exact symmetry, batch-permutation invariance bit for bit, status all zero."""
    from ssmtoybox_amd import ssmod as sm
    g = golden('g2_bs_weights')
    t = 'bs_' + tag
    rng = np.random.default_rng(77)
    means = rng.standard_normal((B, 10))
    a = rng.standard_normal((B, 10, 10)) / np.sqrt(10)
    covs = np.einsum('bij,bkj->bik', a, a) + 0.1 * np.eye(10)
    tf = amd.BayesSardTransform(10, 10, gp_par(10, 3.0), g[t + '_mi'], pstr, ppar)
    w = dict(wm=g[t + '_wm'], Wc=g[t + '_Wc'], Wcc=g[t + '_Wcc'], model_var=float(g[t + '_mv']))
    tf.wm, tf.Wc, tf.Wcc, tf.model.model_var = w['wm'], w['Wc'], w['Wcc'], w['model_var']
    f = sm.Smooth10DTransition().dyn_eval
    assert tf.kernel_name(f) in (('k_apply_tile',) if pstr == 'ut' else ('k_bq_fused', 'k_apply_wide'))   # (wide = the two-pass matrix-core route's name)
    mf, cf, cfx, st = tf.apply_batch(f, means, covs, 0.0, return_status=True)
    assert not st.any() and np.all(np.isfinite(mf)) and np.all(np.isfinite(cf)) and np.all(np.isfinite(cfx))
    assert np.array_equal(cf, cf.transpose(0, 2, 1))
    pts = g[t + '_pts']
    worst = 0.0
    for i in np.random.default_rng(78).choice(B, 200, replace=False):
        ref = orc.apply_bq(orc.F_SMOOTH10D_DYN, means[i], covs[i], 0.0, pts, w)
        worst = max(worst, assert_moments_close((mf[i], cf[i], cfx[i]), ref, covs[i], what=(tag, i)))
    assert within(worst, 1e-10, 'configs[4] {} B={} device transform vs oracle (200 samples, scaled)'.format(tag, B))
    perm = np.random.default_rng(79).permutation(B)[:2048]
    mf2, cf2, cfx2 = tf.apply_batch(f, means[perm], covs[perm], 0.0)
    assert np.array_equal(mf2, mf[perm]) and np.array_equal(cf2, cf[perm]) and np.array_equal(cfx2, cfx[perm])
    if pstr == 'ut' and 'SSMQ_TILE_NO_EXACT' not in os.environ and 'SSMQ_TILE_NO_MROW' not in os.environ:
        # this shape runs k_apply_tile's EXACT-shape instantiation (D = E = 10, N = 21 at compile time, round 6): the same arithmetic
        # as the run-time-shape body, so the same bits
        os.environ['SSMQ_TILE_NO_EXACT'] = '1'
        try:
            mf3, cf3, cfx3 = tf.apply_batch(f, means[:20000], covs[:20000], 0.0)
        finally:
            os.environ.pop('SSMQ_TILE_NO_EXACT')
        assert np.array_equal(mf3, mf[:20000]) and np.array_equal(cf3, cf[:20000]) and np.array_equal(cfx3, cfx[:20000])


@pytest.mark.parametrize('N,E,B', [(201, 10, 64), (201, 7, 37), (120, 5, 60), (250, 3, 100), (201, 10, 2500)])
def test_matrix_core_route_exact_on_integers(amd, monkeypatch, N, E, B):
    """fx Wc through v_mfma_f64_16x16x4_f64 (ssmq_gemm_mfma.hip): with small-integer operands every product and sum
    is exact in fp64, so the moments must equal integer arithmetic exactly - any slip in the operand / accumulator lane
    maps, the k permutation, the zero padding or the ragged last row block shows up as a wrong integer.  Also equal to
    the generic kernel's result (SSMQ_NO_MFMA=1) bit for bit."""
    from ssmtoybox_amd import _lib
    lib = _lib.load()
    D = 3
    rng = np.random.default_rng(N + E + B)
    xi = rng.integers(-3, 4, (D, N)).astype(float)
    wm = rng.integers(-2, 3, N).astype(float)
    Wc = rng.integers(-3, 4, (N, N)).astype(float)
    Wc = Wc + Wc.T
    Wcc = rng.integers(-2, 3, (D, N)).astype(float)
    fx = rng.integers(-4, 5, (B, E, N)).astype(float)
    chol = np.tile(np.tril(rng.integers(1, 4, (D, D))).astype(float), (B, 1, 1))
    mean_i = np.einsum('ben,n->be', fx, wm)
    cov_i = np.einsum('ben,nm,bfm->bef', fx, Wc, fx) - mean_i[:, :, None] * mean_i[:, None, :] + 5.0 * np.eye(E)
    ccov_i = np.einsum('ben,dn,bjd->bej', fx, Wcc, chol)
    assert np.abs(cov_i).max() < 2 ** 50

    def run():
        h = lib.ssmq_transform_create(D, E, N, 0, _lib.as_c(xi)[1], _lib.as_c(wm)[1], _lib.as_c(Wc)[1], _lib.as_c(Wcc)[1],
                                      _lib.as_c(5.0 * np.eye(E))[1], 0, 0.0, None)
        assert h
        mf, cf, cfx = np.empty((B, E)), np.empty((B, E, E)), np.empty((B, E, D))
        f, pf = _lib.as_c(fx)
        c, pc = _lib.as_c(chol)
        _lib.check(lib.ssmq_apply_fx_batch(ctypes.c_void_p(h), B, pc, None, None, pf, _lib.as_c(mf)[1], _lib.as_c(cf)[1],
                                           _lib.as_c(cfx)[1]), 'ssmq_apply_fx_batch')
        lib.ssmq_transform_destroy(ctypes.c_void_p(h))
        return mf, cf, cfx
    got = run()
    assert np.array_equal(got[0], mean_i) and np.array_equal(got[1], cov_i) and np.array_equal(got[2], ccov_i)
    if B == 64:
        # replacing the weights of a live handle refreshes the padded copy the GEMM reads
        h = lib.ssmq_transform_create(D, E, N, 0, _lib.as_c(xi)[1], _lib.as_c(wm)[1], _lib.as_c(Wc)[1], _lib.as_c(Wcc)[1],
                                      _lib.as_c(5.0 * np.eye(E))[1], 0, 0.0, None)
        Wc2 = Wc + np.diag(np.arange(N, dtype=float) % 3)
        _lib.check(lib.ssmq_transform_update(ctypes.c_void_p(h), None, None, _lib.as_c(Wc2)[1], None, None, 0, 0.0, None),
                   'ssmq_transform_update')
        mf, cf, cfx = np.empty((B, E)), np.empty((B, E, E)), np.empty((B, E, D))
        _lib.check(lib.ssmq_apply_fx_batch(ctypes.c_void_p(h), B, _lib.as_c(chol)[1], None, None, _lib.as_c(fx)[1],
                                           _lib.as_c(mf)[1], _lib.as_c(cf)[1], _lib.as_c(cfx)[1]), 'ssmq_apply_fx_batch')
        lib.ssmq_transform_destroy(ctypes.c_void_p(h))
        cov2 = np.einsum('ben,nm,bfm->bef', fx, Wc2, fx) - mean_i[:, :, None] * mean_i[:, None, :] + 5.0 * np.eye(E)
        assert np.array_equal(cf, cov2)
    monkeypatch.setenv('SSMQ_NO_MFMA', '1')
    ref = run()
    assert all(np.array_equal(a, b) for a, b in zip(got, ref))


@pytest.mark.parametrize('case', ['reentry1d_gh5', 'range_gh5', 'cv_gh4', 'radar_gh4', 'ctrs_gh2', 'smooth10_fs5'])
def test_two_pass_matrix_core_route(amd, monkeypatch, case):
    """Large point sets with a device integrand take two passes: k_eval_wave (one wave per trajectory: factor, points,
    integrand values, mean) and k_fxwc_cov_mfma, whose epilogue forms covariance and cross-covariance from the
    accumulators (ssmq_gemm_mfma.hip).  Checked against the three-pass route (values and T through memory,
    SSMQ_NO_FUSED_COV=1), the generic kernel (SSMQ_NO_MFMA=1) and the oracle, for every output dimension pattern the
    tile / trajectory bookkeeping has (E = 1, 2, 3, 4, 5, 10), ragged batches, a weight matrix that is not symmetric,
    additive and scaled covariances, and a batch item that is not positive definite."""
    from ssmtoybox_amd import ssmod as sm
    D, E, model, f, fid, p, sidx, pstr, ppar, N = {
        'reentry1d_gh5': (3, 3, sm.ReentryVehicle1DTransition, 'dyn_eval', orc.F_REENTRY1D_DYN, (0.1,), None, 'gh', {'degree': 5}, 125),
        'range_gh5': (3, 1, lambda: sm.RangeMeasurement(sm.GaussRV(1), 3), 'meas_eval', orc.F_RANGE_MEAS, (), None, 'gh', {'degree': 5}, 125),
        'cv_gh4': (4, 4, lambda: sm.ConstantVelocity(sm.GaussRV(4), sm.GaussRV(2), dt=0.5), 'dyn_eval', orc.F_CV_DYN, (0.5,), None, 'gh', {'degree': 4}, 256),
        'radar_gh4': (4, 2, lambda: sm.Radar2DMeasurement(sm.GaussRV(2), 4), 'meas_eval', orc.F_RADAR2D_MEAS, (0.0, 0.0), None, 'gh', {'degree': 4}, 256),
        'ctrs_gh2': (7, 5, lambda: sm.ConstantTurnRateSpeed(sm.GaussRV(5), sm.GaussRV(2)), 'dyn_eval', orc.F_CTRS_DYN, (0.05,), None, 'gh', {'degree': 2}, 128),
        'smooth10_fs5': (10, 10, sm.Smooth10DTransition, 'dyn_eval', orc.F_SMOOTH10D_DYN, (), None, 'fs', {'degree': 5}, 201),
    }[case]
    mdl = model()
    fn = getattr(mdl, f)
    rng = np.random.default_rng(sum(map(ord, case)) % 1000)      # (str hashes differ from process to process)
    tf = amd.GaussianProcessTransform(D, E, gp_par(D, 2.0), 'rbf', pstr, ppar)
    pts = tf.model.points
    assert pts.shape == (D, N)
    # injected weights of moderate size (a Gaussian-process Wc at N = 256 is ill-conditioned; this test is about the
    # arithmetic of the route, and a route must not rely on the symmetry of Wc)
    wm = rng.standard_normal(N) / N
    Wc = rng.standard_normal((N, N)) / N
    Wc = 0.5 * (Wc + Wc.T) + 1e-3 * rng.standard_normal((N, N)) / N
    Wcc = rng.standard_normal((D, N)) / N
    tf.wm, tf.Wc, tf.Wcc, tf.model.model_var = wm, Wc, Wcc, 0.37
    w = dict(wm=wm, Wc=Wc, Wcc=Wcc, model_var=0.37)
    for B in (300, 1001):
        base = np.array([90.0, 6.0, 1.7]) if D == 3 else (np.array([20.0, 1.0, 30.0, -1.0]) if D == 4 else np.zeros(D))
        if D == 7:
            base = np.array([1.0, 2.0, 5.0, 0.3, 0.2, 0.0, 0.0])
        means = base + 0.3 * rng.standard_normal((B, D))
        a = rng.standard_normal((B, D, D)) / np.sqrt(D)
        covs = 0.05 * (np.einsum('bij,bkj->bik', a, a) + 0.1 * np.eye(D))
        covs[B // 2] = -np.eye(D)
        monkeypatch.delenv('SSMQ_NO_FUSED_COV', raising=False)
        monkeypatch.delenv('SSMQ_NO_MFMA', raising=False)
        assert tf.kernel_name(fn) in ('k_apply_wide', 'k_bq_fused')
        mf, cf, cfx, st = tf.apply_batch(fn, means, covs, 2.0, return_status=True)
        monkeypatch.setenv('SSMQ_NO_FUSED_COV', '1')
        mf3, cf3, cfx3, st3 = tf.apply_batch(fn, means, covs, 2.0, return_status=True)
        monkeypatch.delenv('SSMQ_NO_FUSED_COV')
        bad = B // 2
        assert st[bad] != 0 and not np.delete(st, bad).any() and np.array_equal(st, st3)
        assert np.all(np.isnan(mf[bad])) and np.all(np.isnan(cf[bad])) and np.all(np.isnan(cfx[bad]))
        ok = np.arange(B) != bad
        assert np.all(np.isfinite(cf[ok])) and np.all(np.isfinite(cfx[ok]))
        assert np.array_equal(cf[ok], cf[ok].transpose(0, 2, 1))                      # mirrored lower triangle
        sc = np.abs(cf3[ok]).max()
        assert within(np.abs(mf[ok] - mf3[ok]).max() / np.abs(mf3[ok]).max(), 1e-13, case + ' two-pass vs three-pass mean')
        assert within(np.abs(cf[ok] - cf3[ok]).max() / sc, 1e-13, case + ' two-pass vs three-pass cov')
        assert within(np.abs(cfx[ok] - cfx3[ok]).max() / np.abs(cfx3[ok]).max(), 1e-13, case + ' two-pass vs three-pass ccov')
        for i in (0, 1, B // 2 + 1, B - 1):
            ref = orc.apply_bq(fid, means[i], covs[i], 2.0, pts, w, p, sidx)
            # the oracle forms the full product; the kernels mirror the lower triangle of (fx Wc) fx'
            rc = np.tril(ref[1]) + np.tril(ref[1], -1).T
            assert_moments_close((mf[i], cf[i], cfx[i]), (ref[0], rc, ref[2]), covs[i], what=(case, B, i))
    monkeypatch.setenv('SSMQ_NO_MFMA', '1')
    tfg = amd.GaussianProcessTransform(D, E, gp_par(D, 2.0), 'rbf', pstr, ppar)
    tfg.wm, tfg.Wc, tfg.Wcc, tfg.model.model_var = wm, Wc, Wcc, 0.37
    mg, cg, xg = tfg.apply_batch(fn, means[:64], covs[:64], 2.0)
    monkeypatch.delenv('SSMQ_NO_MFMA')
    assert within(max(np.abs(cg - cf[:64]).max() / sc, np.abs(xg - cfx[:64]).max() / np.abs(cfx3[ok]).max()), 5e-13,
                  'matrix-core route vs workgroup kernel, ' + case)     # (1.5e-13 seen at N = 125 with a non-symmetric Wc)


@pytest.mark.parametrize('D, pstr, ppar, N, E', [(10, 'fs', {'degree': 5}, 201, 6), (10, 'fs', {'degree': 5}, 201, 7),
                                                 (10, 'fs', {'degree': 5}, 201, 8), (7, 'gh', {'degree': 2}, 128, 6),
                                                 (7, 'gh', {'degree': 2}, 128, 7), (7, 'gh', {'degree': 2}, 128, 8),
                                                 (3, 'gh', {'degree': 5}, 125, 8)])
def test_one_launch_bq_route_shapes(amd, monkeypatch, D, pstr, ppar, N, E):
    """k_bq_fused (ssmq_bq_fused.hip: factor, integrand values into an LDS tile, both matrix-core products and the covariance
    epilogue in one launch) over its shape space beside the D = E = 10 model of the other tests: output dimensions 6, 7, 8
    (a workgroup owns 10, 9 or 8 whole trajectories or fewer - what fits the LDS - with the compile-time bounds 8 and 16,
    i.e. the register and the LDS factorisation, and the 128- and 208-column instantiations), an integrand behind a state
    index (bearings to E sensors from two entries of the state: ssmod.py:1155-1198; 8 sensors = SSMQ_MAX_FPAR), batches
    that end in a partial tile, a covariance that is not positive definite.  Against the two-pass route (SSMQ_NO_BQ_FUSED)
    at the rounding level and against the oracle."""
    from ssmtoybox_amd import ssmod as sm
    if os.environ.get('SSMQ_NO_MFMA') or os.environ.get('SSMQ_NO_BQ_FUSED'):
        pytest.skip('the matrix-core routes are switched off')
    rng = np.random.default_rng(100 * D + E)
    sens = 30.0 * rng.standard_normal((E, 2))
    sidx = [0, 2] if D > 3 else [0, 1]
    obs = sm.BearingMeasurement(sm.GaussRV(E), D, state_index=sidx, sensor_pos=sens)
    fn = obs.meas_eval
    tf = amd.GaussianProcessTransform(D, E, gp_par(D, 2.0), 'rbf', pstr, ppar)
    pts = tf.model.points
    assert pts.shape == (D, N)
    wm = rng.standard_normal(N) / N
    Wc = rng.standard_normal((N, N)) / N
    Wc = 0.5 * (Wc + Wc.T)
    Wcc = rng.standard_normal((D, N)) / N
    # the one-launch route forms fx Wc fx' as C + C' with C = (fx S) fx', Wc = S + S' (half the matrix instructions): it is
    # offered for a Wc that is symmetric to the last bit only; any other keeps the two passes, which form (fx Wc) fx' as written
    tf.wm, tf.Wc, tf.Wcc, tf.model.model_var = wm, Wc + 1e-3 * np.triu(rng.standard_normal((N, N)), 1) / N, Wcc, 0.21
    assert tf.kernel_name(fn) == 'k_apply_wide'
    tf.Wc = Wc
    w = dict(wm=wm, Wc=Wc, Wcc=Wcc, model_var=0.21)
    assert tf.kernel_name(fn) == 'k_bq_fused'
    for B in (257, 1000):
        means = 3.0 * rng.standard_normal((B, D))
        a = rng.standard_normal((B, D, D)) / np.sqrt(D)
        covs = 0.5 * (np.einsum('bij,bkj->bik', a, a) + 0.1 * np.eye(D))
        bad = B - 2                                            # in the last, partial tile
        covs[bad] = -np.eye(D)
        mf, cf, cfx, st = tf.apply_batch(fn, means, covs, 0.0, return_status=True)
        monkeypatch.setenv('SSMQ_NO_BQ_FUSED', '1')
        assert tf.kernel_name(fn) == 'k_apply_wide'
        mf2, cf2, cfx2, st2 = tf.apply_batch(fn, means, covs, 0.0, return_status=True)
        monkeypatch.delenv('SSMQ_NO_BQ_FUSED')
        assert st[bad] != 0 and not np.delete(st, bad).any() and np.array_equal(st, st2)
        assert np.all(np.isnan(mf[bad])) and np.all(np.isnan(cf[bad])) and np.all(np.isnan(cfx[bad]))
        ok = np.arange(B) != bad
        assert np.all(np.isfinite(mf[ok])) and np.all(np.isfinite(cf[ok])) and np.all(np.isfinite(cfx[ok]))
        assert np.array_equal(cf[ok], cf[ok].transpose(0, 2, 1))
        sc = np.abs(cf2[ok]).max()
        what = 'one launch vs two passes, D=%d E=%d N=%d B=%d ' % (D, E, N, B)
        assert within(np.abs(mf[ok] - mf2[ok]).max() / np.abs(mf2[ok]).max(), 1e-13, what + 'mean')
        assert within(np.abs(cf[ok] - cf2[ok]).max() / sc, 1e-13, what + 'cov')
        assert within(np.abs(cfx[ok] - cfx2[ok]).max() / np.abs(cfx2[ok]).max(), 1e-13, what + 'ccov')
        for i in (0, 1, B // 2, B - 1):
            ref = orc.apply_bq(orc.F_BEARING_MEAS, means[i], covs[i], 0.0, pts, w, tuple(sens.reshape(-1)), sidx)
            rc = np.tril(ref[1]) + np.tril(ref[1], -1).T
            assert_moments_close((mf[i], cf[i], cfx[i]), (ref[0], rc, ref[2]), covs[i], what=(D, E, N, B, i))


@pytest.mark.parametrize('D, pstr, ppar, N, E', [(6, 'gh', {'degree': 3}, 729, 6), (6, 'gh', {'degree': 3}, 729, 7),
                                                 (3, 'gh', {'degree': 7}, 343, 8), (10, 'fs', {'degree': 7}, 1181, 8),
                                                 (4, 'gh', {'degree': 4}, 256, 6), (2, 'gh', {'degree': 15}, 225, 7),
                                                 (3, 'gh', {'degree': 7}, 343, 2), (4, 'gh', {'degree': 4}, 256, 4), (5, 'gh', {'degree': 4}, 1024, 1)])
def test_streamed_bq_route_shapes(amd, monkeypatch, D, pstr, ppar, N, E):
    """k_bq_stream (ssmq_bq_stream.hip: the route for 209 ... 4096 points - k_eval_wave, then the streamed product with S =
    tril(Wc) by panels of 16 column tiles and the C + C' epilogue) over its shape space beside configs[4]: output dimensions
    1 ... 8 (64 ... 8 trajectories per 64-row tile), point counts with a partial last panel / a single k-block past a panel
    boundary / exactly 16 k-blocks / 64 k-blocks, batches that end in a partial tile, a covariance that is not positive
    definite.  Against the blocked route (SSMQ_NO_BQ_STREAM) at rounding level and against the oracle."""
    from ssmtoybox_amd import ssmod as sm
    if os.environ.get('SSMQ_NO_MFMA') or os.environ.get('SSMQ_NO_BQ_STREAM'):
        pytest.skip('the matrix-core routes are switched off')
    rng = np.random.default_rng(1000 * D + E)
    sens = 30.0 * rng.standard_normal((E, 2))
    sidx = [0, 2] if D > 3 else [0, 1]
    obs = sm.BearingMeasurement(sm.GaussRV(E), D, state_index=sidx, sensor_pos=sens)
    fn = obs.meas_eval
    tf = amd.GaussianProcessTransform(D, E, gp_par(D, 2.0), 'rbf', pstr, ppar)
    pts = tf.model.points
    assert pts.shape == (D, N)
    wm = rng.standard_normal(N) / N
    Wc = rng.standard_normal((N, N)) / N
    Wc = 0.5 * (Wc + Wc.T)
    Wcc = rng.standard_normal((D, N)) / N
    # offered for a Wc that is symmetric to the last bit only (Wc = S + S'); any other keeps the blocked route
    tf.wm, tf.Wc, tf.Wcc, tf.model.model_var = wm, Wc + 1e-3 * np.triu(rng.standard_normal((N, N)), 1) / N, Wcc, 0.21
    other = 'k_apply_wide' if N > 240 and N <= 256 else 'k_apply_big'     # (256 points: the two-pass route's third instantiation)
    assert tf.kernel_name(fn) == other
    tf.Wc = Wc
    w = dict(wm=wm, Wc=Wc, Wcc=Wcc, model_var=0.21)
    assert tf.kernel_name(fn) == 'k_bq_stream'
    for B in (257, 3001):
        means = 3.0 * rng.standard_normal((B, D))
        a = rng.standard_normal((B, D, D)) / np.sqrt(D)
        covs = 0.5 * (np.einsum('bij,bkj->bik', a, a) + 0.1 * np.eye(D))
        bad = B - 2                                            # in the last, partial tile
        covs[bad] = -np.eye(D)
        mf, cf, cfx, st = tf.apply_batch(fn, means, covs, 0.0, return_status=True)
        # the last, partly empty round of workgroups is cut by panel (bq_stream_split) and summed in the whole-block order: same bits
        monkeypatch.setenv('SSMQ_BQ_STREAM_NO_SPLIT', '1')
        mf0, cf0, cfx0, st0 = tf.apply_batch(fn, means, covs, 0.0, return_status=True)
        monkeypatch.delenv('SSMQ_BQ_STREAM_NO_SPLIT')
        assert np.array_equal(mf, mf0, equal_nan=True) and np.array_equal(cf, cf0, equal_nan=True) and \
            np.array_equal(cfx, cfx0, equal_nan=True) and np.array_equal(st, st0)
        monkeypatch.setenv('SSMQ_NO_BQ_STREAM', '1')
        assert tf.kernel_name(fn) == other
        mf2, cf2, cfx2, st2 = tf.apply_batch(fn, means, covs, 0.0, return_status=True)
        monkeypatch.delenv('SSMQ_NO_BQ_STREAM')
        assert st[bad] != 0 and not np.delete(st, bad).any() and np.array_equal(st, st2)
        assert np.all(np.isnan(mf[bad])) and np.all(np.isnan(cf[bad])) and np.all(np.isnan(cfx[bad]))
        ok = np.arange(B) != bad
        assert np.all(np.isfinite(mf[ok])) and np.all(np.isfinite(cf[ok])) and np.all(np.isfinite(cfx[ok]))
        assert np.array_equal(cf[ok], cf[ok].transpose(0, 2, 1))
        sc = np.abs(cf2[ok]).max()
        what = 'streamed vs blocked route, D=%d E=%d N=%d B=%d ' % (D, E, N, B)
        assert within(np.abs(mf[ok] - mf2[ok]).max() / np.abs(mf2[ok]).max(), 1e-13, what + 'mean')
        assert within(np.abs(cf[ok] - cf2[ok]).max() / sc, 1e-13, what + 'cov')
        assert within(np.abs(cfx[ok] - cfx2[ok]).max() / np.abs(cfx2[ok]).max(), 1e-13, what + 'ccov')
        for i in (0, 1, B // 2, B - 1):
            ref = orc.apply_bq(orc.F_BEARING_MEAS, means[i], covs[i], 0.0, pts, w, tuple(sens.reshape(-1)), sidx)
            assert_moments_close((mf[i], cf[i], cfx[i]), ref, covs[i], what=(D, E, N, B, i))
        perm = rng.permutation(B)
        perm = perm[perm != bad][:300]
        mf3, cf3, cfx3 = tf.apply_batch(fn, means[perm], covs[perm], 0.0)
        assert np.array_equal(mf3, mf[perm]) and np.array_equal(cf3, cf[perm]) and np.array_equal(cfx3, cfx[perm])


def test_calls_from_several_threads_on_different_handles(amd):
    """"functions are re-entrant across handles".  Every calling thread has a context of its own - a stream and the
    caches that belong to it (include/ssmq.h, conventions) - and a handle is locked only for the entry point that uses it:
    threads that hammer different transforms (ctypes releases the GIL inside each call) run concurrently and must get exactly
    the results of the same calls made one after the other."""
    import threading
    from ssmtoybox_amd import ssmod as sm
    rng = np.random.default_rng(5)
    jobs = []
    for D, model in ((1, sm.UNGMTransition()), (5, sm.ReentryVehicle2DTransition()), (2, sm.Pendulum2DTransition(dt=0.01)),
                     (5, sm.CoordinatedTurnTransition())):
        tf = amd.GaussianProcessTransform(D, D, gp_par(D, 3.0)) if D != 2 else amd.UnscentedTransform(D)
        B = 777 + 64 * D
        base = {1: [0.5], 2: [1.5, 0.0], 5: [6500.4, 349.14, -1.8093, -6.7967, 0.6932]}[D] if not isinstance(model, sm.CoordinatedTurnTransition) \
            else [1000.0, 300.0, 1000.0, 0.0, -0.05]
        means = np.asarray(base) + 1e-2 * rng.standard_normal((B, D))
        a = rng.standard_normal((B, D, D)) * 1e-2
        covs = np.einsum('bij,bkj->bik', a, a) + 1e-6 * np.eye(D)
        jobs.append((tf, model.dyn_eval, means, covs))
    serial = [tf.apply_batch(f, m, c, 1.0) for tf, f, m, c in jobs]
    results, errors = [None] * len(jobs), []

    def work(i):
        try:
            tf, f, m, c = jobs[i]
            for _ in range(25):
                out = tf.apply_batch(f, m, c, 1.0)
            results[i] = out
        except Exception as e:        # noqa: BLE001
            errors.append((i, repr(e)))
    threads = [threading.Thread(target=work, args=(i,)) for i in range(len(jobs))]
    for t in threads:
        t.start()
    for t in threads:
        t.join(120)
    assert not errors, errors
    for got, ref in zip(results, serial):
        assert got is not None and all(np.array_equal(g, r) for g, r in zip(got, ref))


def test_threads_share_a_handle_and_filters_run_on_their_own_streams(amd):
    """The other two cases of the threading contract (include/ssmq.h): (a) several threads on the SAME handle - the handle's lock
    serialises them and a context that takes the handle over waits for the stream that used it last (here: the main thread's,
    which uploaded new constants just before); (b) whole filters (fused time loop, cached workspace and launch graph per
    context) from four threads at once, each on its own objects, then on objects created by the main thread.  Results EQUAL
    to the serial ones; contexts of threads that ended are reused (a fifth round of threads finds them)."""
    import threading
    from ssmtoybox_amd import ssinf, ssmod as sm
    from bench import simulate_ungm
    rng = np.random.default_rng(11)
    D = 5
    tf = amd.GaussianProcessTransform(D, D, gp_par(D, 3.0))
    f = sm.ReentryVehicle2DTransition().dyn_eval
    means = np.asarray([6500.4, 349.14, -1.8093, -6.7967, 0.6932]) + 1e-2 * rng.standard_normal((1500, D))
    a = rng.standard_normal((1500, D, D)) * 1e-2
    covs = np.einsum('bij,bkj->bik', a, a) + 1e-6 * np.eye(D)
    results, errors = {}, []

    def run(threads):
        for t in threads:
            t.start()
        for t in threads:
            t.join(300)
        assert not errors, errors

    # (a) same handle; the constants change between the rounds (uploaded from the main thread's stream)
    for par in (3.0, 1.7):
        tf.wm, tf.Wc, tf.Wcc = tf.weights(gp_par(D, par))       # new weights: the next apply uploads new constant blocks
        ref = tf.apply_batch(f, means, covs, 1.0)

        def same(i):
            try:
                for _ in range(10):
                    results[('a', i)] = tf.apply_batch(f, means, covs, 1.0)
            except Exception as e:        # noqa: BLE001
                errors.append((i, repr(e)))
        run([threading.Thread(target=same, args=(i,)) for i in range(4)])
        for i in range(4):
            assert all(np.array_equal(g, r) for g, r in zip(results[('a', i)], ref)), (par, i)

    # (b) whole filters
    def make(kind):
        dyn = sm.UNGMTransition(sm.GaussRV(1), sm.GaussRV(1, cov=np.array([[10.0]])))
        obs = sm.UNGMMeasurement(sm.GaussRV(1), 1)
        if kind == 0:
            return ssinf.GaussianProcessKalman(dyn, obs, np.array([[1.0, 3.0]]), np.array([[1.0, 3.0]]), points='sr')
        if kind == 1:
            return ssinf.UnscentedKalman(dyn, obs)
        if kind == 2:
            return ssinf.CubatureKalman(dyn, obs)
        return ssinf.GaussHermiteKalman(dyn, obs, deg=5)
    data = []
    for kind in range(4):
        _, y = simulate_ungm(2000 + 64 * kind, 40, 30 + kind)
        data.append(np.ascontiguousarray(y[None]))
    main_algs = [make(k) for k in range(4)]
    serial = [tuple(x.copy() for x in main_algs[k].forward_pass_batch(data[k])) for k in range(4)]

    def filt(k, alg):
        try:
            alg = alg or make(k)
            for _ in range(8):
                out = alg.forward_pass_batch(data[k])
            results[('b', k)] = tuple(x.copy() for x in out)
        except Exception as e:        # noqa: BLE001
            errors.append((k, repr(e)))
    for own in (True, False, True, False, True):
        run([threading.Thread(target=filt, args=(k, None if own else main_algs[k])) for k in range(4)])
        for k in range(4):
            assert all(np.array_equal(g, r) for g, r in zip(results[('b', k)], serial[k])), (own, k)


def test_state_index_with_more_than_eight_entries(amd):
    """A measurement-type integrand that reads 10 selected entries of a 13-dimensional state (state_index of 10 entries):
    the device integrand evaluates on the selected sub-state (generic kernel), as the oracle's restatement of
    MeasurementModel.meas_eval's state_index selection does (ssmod.py:990-991).  The reference has no model above seven
    inputs; the 10-D synthetic model stands in."""
    from ssmtoybox_amd import _lib
    from oracle import c_oracle as co
    lib = _lib.load()
    D, E, B = 13, 10, 200
    sidx = [12, 0, 3, 4, 7, 1, 9, 10, 2, 6]
    rng = np.random.default_rng(23)
    pts = orc.points_ut(D)
    wm, wc = orc.weights_ut(D)
    N = pts.shape[1]
    h = lib.ssmq_transform_create(D, E, N, 1, _lib.as_c(pts)[1], _lib.as_c(wm)[1], _lib.as_c(wc)[1], None, None, 0, 0.0, None)
    assert h
    means = rng.standard_normal((B, D))
    a = rng.standard_normal((B, D, D)) / np.sqrt(D)
    covs = np.einsum('bij,bkj->bik', a, a) + 0.1 * np.eye(D)
    integ = _lib.Integrand.make(_lib.F_SMOOTH10D_DYN, (), sidx)
    mf, cf, cfx = np.empty((B, E)), np.empty((B, E, E)), np.empty((B, E, D))
    st = np.zeros(B, dtype=np.int32)
    t0 = np.zeros(1)
    _lib.check(lib.ssmq_apply_batch(ctypes.c_void_p(h), ctypes.byref(integ), B, _lib.as_c(means)[1], _lib.as_c(covs)[1],
                                    _lib.as_c(t0)[1], 0, _lib.as_c(mf)[1], _lib.as_c(cf)[1], _lib.as_c(cfx)[1],
                                    st.ctypes.data_as(_lib.c_int32_p)), 'ssmq_apply_batch')
    lib.ssmq_transform_destroy(ctypes.c_void_p(h))
    assert not st.any()
    t, keep = co.make_transform(1, D, E, pts, wm, wc, integrand=co.Integrand.make(orc.F_SMOOTH10D_DYN, (), sidx))
    omf, ocf, ocfx, ost = co.apply_batch(t, means, covs, 0.0)
    for i in range(0, B, 7):
        assert_moments_close((mf[i], cf[i], cfx[i]), (omf[i], ocf[i], ocfx[i]), covs[i], what=('idx10', i))
    ref = orc.apply_sigma(orc.F_SMOOTH10D_DYN, means[0], covs[0], 0.0, pts, wm, wc, (), sidx)
    assert_moments_close((mf[0], cf[0], cfx[0]), ref, covs[0], what='idx10 vs numpy oracle')


def test_extreme_covariance_scales(amd):
    """The register kernels take square roots and reciprocals of the Cholesky pivots with a one-round refinement of
    v_rsq_f64 / v_rcp_f64 (csrc/ssmq_device.h) instead of the compiler's range-rescaled sequences: covariances scaled by
    2^+-900 (1e+-271, far beyond any model of the reference) must still go through a linear model exactly as the
    unscaled ones do, up to the power of two."""
    from ssmtoybox_amd import ssmod as sm
    rng = np.random.default_rng(77)
    B = 200
    means = np.zeros((B, 4))      # zero mean: the points are +-c L columns, whatever the scale (no absorption into m)
    a = rng.standard_normal((B, 4, 4)) / 2
    covs = np.einsum('bij,bkj->bik', a, a) + 0.1 * np.eye(4)
    model = sm.ConstantVelocity(dt=0.5)
    f = model.dyn_eval
    A = np.array([[1, 0.5, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0.5], [0, 0, 0, 1]])
    tf = amd.UnscentedTransform(4)
    assert 'k_apply_small' in tf.kernel_name(f)
    base = tf.apply_batch(f, means, covs, 0.0)
    assert np.allclose(base[1], np.einsum('ij,bjk,lk->bil', A, covs, A), rtol=1e-12, atol=1e-13)   # linear: UT is exact
    for k in (-900, 900):
        sc = 2.0 ** k
        got = tf.apply_batch(f, means, covs * sc, 0.0)
        # centred form on a linear map: covariance and cross-covariance scale with the input covariance exactly
        assert np.allclose(got[1] / sc, base[1], rtol=1e-12, atol=1e-13)
        assert np.allclose(got[2] / sc, base[2], rtol=1e-12, atol=1e-13)
        assert np.abs(got[0]).max() <= 1e-12 * np.sqrt(sc)          # sums of +-c L columns: zero up to rounding
    tg = amd.GaussianProcessTransform(4, 4, np.array([[1.0, 3.0, 3.0, 3.0, 3.0]]), 'rbf', 'ut')
    assert 'k_apply_small' in tg.kernel_name(f)
    for k in (-900, 0, 600):
        got = tg.apply_batch(f, means, covs * 2.0 ** k, 0.0)
        assert all(np.all(np.isfinite(g)) for g in got), k


def test_random_shapes_against_oracle(amd):
    """Sweep of run-time shapes through the generic kernel's split entry points (sigma points out, reductions in): random
    D, E, N, random weights (not from any quadrature rule), BQ / BQ + t-process variance / centred form."""
    from ssmtoybox_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(2026)
    for trial in range(40):
        D, E, N = int(rng.integers(1, 9)), int(rng.integers(1, 9)), int(rng.integers(1, 45))
        form = int(rng.integers(0, 2))
        tp = (form == 0) and bool(rng.integers(0, 2))
        B = int(rng.integers(1, 70))
        xi = rng.standard_normal((D, N))
        wm = rng.standard_normal(N) / N
        Wc = rng.standard_normal((N, N)) / N
        Wc = Wc + Wc.T
        wcd = rng.random(N) / N
        Wcc = rng.standard_normal((D, N)) / N
        emv = np.diag(rng.random(E))
        iK = rng.standard_normal((N, N))
        iK = iK.dot(iK.T) / N
        h = lib.ssmq_transform_create(D, E, N, form, _lib.as_c(xi)[1], _lib.as_c(wm)[1],
                                      _lib.as_c(wcd if form else Wc)[1], None if form else _lib.as_c(Wcc)[1],
                                      _lib.as_c(emv)[1], 0, 4.0 if tp else 0.0, _lib.as_c(iK)[1] if tp else None)
        assert h, (D, E, N, form)
        means = rng.standard_normal((B, D))
        a = rng.standard_normal((B, D, D)) / np.sqrt(D)
        covs = np.einsum('bij,bkj->bik', a, a) + 0.2 * np.eye(D)
        x, chol = np.empty((B, D, N)), np.empty((B, D, D))
        st = np.zeros(B, dtype=np.int32)
        assert lib.ssmq_sigma_points_batch(ctypes.c_void_p(h), B, _lib.as_c(means)[1], _lib.as_c(covs)[1], _lib.as_c(x)[1],
                                           _lib.as_c(chol)[1], st.ctypes.data_as(_lib.c_int32_p)) == 0
        fx = rng.standard_normal((B, E, N)) + np.sin(x[:, :1, :])          # any values: the reductions are linear algebra
        mf, cf, cfx = np.empty((B, E)), np.empty((B, E, E)), np.empty((B, E, D))
        _lib.check(lib.ssmq_apply_fx_batch(ctypes.c_void_p(h), B, _lib.as_c(chol)[1], _lib.as_c(means)[1], _lib.as_c(x)[1],
                                           _lib.as_c(fx)[1], _lib.as_c(mf)[1], _lib.as_c(cf)[1], _lib.as_c(cfx)[1]),
                   'ssmq_apply_fx_batch')
        lib.ssmq_transform_destroy(ctypes.c_void_p(h))
        for b in range(0, B, max(1, B // 5)):
            L = np.linalg.cholesky(covs[b])
            assert np.allclose(chol[b], L, rtol=1e-13, atol=1e-14) and np.allclose(x[b], means[b][:, None] + L.dot(xi),
                                                                                 rtol=1e-13, atol=1e-13)
            if form:
                ref = orc.moments_sigma(fx[b], x[b], means[b], wm, wcd)
            else:
                ed = orc.tp_emv_diag(fx[b], iK, np.diag(emv), 4.0) if tp else np.diag(emv)
                ref = orc.moments_bq(fx[b], chol[b], wm, Wc, Wcc, ed)
            for got, want in zip((mf[b], cf[b], cfx[b]), ref):
                assert np.allclose(got, want, rtol=1e-11, atol=1e-11 * max(1.0, np.abs(want).max())), (trial, D, E, N, form, tp)


@pytest.mark.parametrize('no_mrow', [False, True])
def test_generic_routes_random_point_sets(amd, monkeypatch, no_mrow):
    """(no_mrow: k_apply_tile's path for D = 16, where the transformed mean cannot ride along as row 15 of the cross-covariance
    product, forced on these smaller models.)  The run-time-shape routes on RANDOM rules (points, weights, model variances drawn at random - no structure a
    kernel could lean on) with the reference's models as device integrands: k_apply_tile (9 ... 64 points), the blocked
    matrix-core route (65 ... 700 points, batches above its minimum row count) and the workgroup kernel (small batches),
    BQ / t-process / centred forms, sub-state measurement models - against the oracle's moments of the same rule."""
    from ssmtoybox_amd import _lib
    lib = _lib.load()
    if no_mrow:
        monkeypatch.setenv('SSMQ_TILE_NO_MROW', '1')
    rng = np.random.default_rng(303)
    names = ('reentry_dyn', 'radar_meas', 'ct_dyn', 'bearing_meas', 'pend_dyn', 'cv_dyn', 'reentry1d_dyn', 'ctrs_dyn', 'ungm_dyn')
    seen = set()
    for trial in range(36):
        name = names[trial % len(names)]
        fid, p, sidx, D, E = MODELS[name]
        N = int(rng.integers(9, 65)) if trial % 2 == 0 else int(rng.integers(65, 700))
        form = int(rng.integers(0, 2))
        tp = (form == 0) and bool(rng.integers(0, 2))
        B = int(rng.integers(1, 40)) if trial % 3 == 0 else int(rng.integers(260, 400))
        xi = rng.standard_normal((D, N))
        wm = rng.random(N)
        wm /= wm.sum()
        Wc = rng.standard_normal((N, N)) / N
        Wc = Wc + Wc.T
        wcd = rng.random(N) / N
        Wcc = rng.standard_normal((D, N)) / N
        emv = np.diag(rng.random(E))
        iK = rng.standard_normal((N, N))
        iK = iK.dot(iK.T) / N
        h = lib.ssmq_transform_create(D, E, N, form, _lib.as_c(xi)[1], _lib.as_c(wm)[1], _lib.as_c(wcd if form else Wc)[1],
                                      None if form else _lib.as_c(Wcc)[1], _lib.as_c(emv)[1], 0, 4.0 if tp else 0.0,
                                      _lib.as_c(iK)[1] if tp else None)
        assert h, (name, N, form)
        integ = _lib.Integrand.make(fid, p, sidx)
        buf = ctypes.create_string_buffer(256)
        lib.ssmq_apply_kernel_name(ctypes.c_void_p(h), ctypes.byref(integ), buf, 256)
        if name == 'ungm_dyn':
            means = rng.standard_normal((B, D))
        else:
            g0 = {'reentry_dyn': [6500.4, 349.14, -1.8093, -6.7967, 0.6932], 'radar_meas': [6500.4, 349.14, -1.8, -6.8, 0.7],
                  'ct_dyn': [1000, 300, 1000, 0, -0.05], 'bearing_meas': [100, 3, 200, 0, -0.05], 'pend_dyn': [1.5, 0.0],
                  'cv_dyn': [10.0, 1.0, -5.0, 0.5], 'reentry1d_dyn': [90.0, 6.0, 1.5], 'ctrs_dyn': [0, 0, 10, 0.3, 0.05, 0, 0]}[name]
            means = np.array(g0, dtype=float) + 0.01 * rng.standard_normal((B, D))
        a_ = rng.standard_normal((B, D, D)) / np.sqrt(D)
        covs = 1e-3 * (np.einsum('bij,bkj->bik', a_, a_) + 0.2 * np.eye(D))
        times = np.full(B, 3.0)
        mf, cf, cfx = np.empty((B, E)), np.empty((B, E, E)), np.empty((B, E, D))
        st = np.zeros(B, dtype=np.int32)
        rc = lib.ssmq_apply_batch(ctypes.c_void_p(h), ctypes.byref(integ), B, _lib.as_c(means)[1], _lib.as_c(covs)[1],
                                  _lib.as_c(times)[1], 1, _lib.as_c(mf)[1], _lib.as_c(cf)[1], _lib.as_c(cfx)[1],
                                  st.ctypes.data_as(_lib.c_int32_p))
        assert rc == 0 and not st.any(), (name, N, form, tp, B, buf.value)
        lib.ssmq_transform_destroy(ctypes.c_void_p(h))
        seen.add(buf.value.decode())
        for b in range(0, B, max(1, B // 4)):
            L = np.linalg.cholesky(covs[b])
            x = means[b][:, None] + L.dot(xi)
            fx = orc.eval_columns(fid, x, 3.0, p, sidx)
            if form:
                ref = orc.moments_sigma(fx, x, means[b], wm, wcd)
            else:
                ed = orc.tp_emv_diag(fx, iK, np.diag(emv), 4.0) if tp else np.diag(emv)
                ref = orc.moments_bq(fx, L, wm, Wc, Wcc, ed)
            # random weights of either sign: terms of size max|fx|^2 sum(|W|) cancel, that is the scale of the rounding
            sc = max(1.0, float(np.abs(fx).max())) ** 2 * max(1.0, float(np.abs(wcd if form else Wc).sum()))
            for got, want, s_ in zip((mf[b], cf[b], cfx[b]), ref, (np.sqrt(sc), sc, np.sqrt(sc))):
                assert np.max(np.abs(got - want)) <= 1e-11 * s_, (trial, name, N, form, tp, B, buf.value, np.max(np.abs(got - want)) / s_)
    if not any(os.environ.get(v) for v in ('SSMQ_NO_MFMA', 'SSMQ_NO_TILE', 'SSMQ_NO_WAVE')):
        assert {'k_apply_tile', 'k_apply_big'} <= seen, seen      # (small batches of the large rules run on k_apply_wide)


def test_bsq_d10_device_integrand(amd, golden):
    """Config C5 without the host in the loop: the synthetic 10-D model evaluated on the device, N = 21 (generic kernel)
    and N = 201 (EVAL pass -> matrix-core GEMM -> FX pass), against the oracle with the reference's weights injected,
    and against the host-callable route of the same function."""
    from ssmtoybox_amd import ssmod as sm
    g = golden('g2_bs_weights')
    rng = np.random.default_rng(19)
    B = 96
    means = rng.standard_normal((B, 10))
    a = rng.standard_normal((B, 10, 10)) / np.sqrt(10)
    covs = np.einsum('bij,bkj->bik', a, a) + 0.1 * np.eye(10)
    model = sm.Smooth10DTransition()
    for tag, pstr, ppar in (('d10_ut', 'ut', None), ('d10_fs5_td2', 'fs', {'degree': 5})):
        t = 'bs_' + tag
        tf = amd.BayesSardTransform(10, 10, gp_par(10, 3.0), g[t + '_mi'], pstr, ppar)
        w = dict(wm=g[t + '_wm'], Wc=g[t + '_Wc'], Wcc=g[t + '_Wcc'], model_var=float(g[t + '_mv']))
        tf.wm, tf.Wc, tf.Wcc, tf.model.model_var = w['wm'], w['Wc'], w['Wcc'], w['model_var']
        assert tf.kernel_name(model.dyn_eval) in (('k_apply_tile', 'k_apply_wave', 'k_apply_wide') if pstr == 'ut' else ('k_apply_wide', 'k_bq_fused'))
        mf, cf, cfx = tf.apply_batch(model.dyn_eval, means, covs, 0.0)
        for i in range(0, B, 9):
            ref = orc.apply_bq(orc.F_SMOOTH10D_DYN, means[i], covs[i], 0.0, g[t + '_pts'], w)
            assert_moments_close((mf[i], cf[i], cfx[i]), ref, covs[i], what=(tag, i))
        host = tf.apply_batch(lambda x, par: model.dyn_fcn(x, np.zeros(10), 0), means, covs, 0.0)
        for dev_arr, host_arr in zip((mf, cf, cfx), host):
            assert np.allclose(dev_arr, host_arr, rtol=1e-11, atol=1e-11 * np.abs(host_arr).max()), tag
        # a covariance that is not positive definite is flagged and poisoned, the others are untouched
        bad = covs.copy()
        bad[5] = -np.eye(10)
        m2, c2, x2, st = tf.apply_batch(model.dyn_eval, means, bad, 0.0, return_status=True)
        assert st[5] != 0 and not np.delete(st, 5).any() and np.all(np.isnan(c2[5])) and np.array_equal(c2[6], cf[6])


# ---------------------------------------------------------------------------------------------------------------
# edge cases of the batch interface
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B', [1, 2, 63, 64, 65, 127, 1000])
def test_ragged_batch_sizes(amd, B):
    """Batch sizes around the wave width; every trajectory's result equals its single-call result bit for bit."""
    from ssmtoybox_amd import ssmod as sm
    rng = np.random.default_rng(B)
    tf = amd.GaussianProcessTransform(2, 2, gp_par(2, 3.0))
    f = sm.Pendulum2DTransition(dt=0.01).dyn_eval
    means = rng.standard_normal((B, 2))
    a = rng.standard_normal((B, 2, 2))
    covs = np.einsum('bij,bkj->bik', a, a) + 0.1 * np.eye(2)
    mf, cf, cfx = tf.apply_batch(f, means, covs, 0.0)
    w = dict(wm=tf.wm, Wc=tf.Wc, Wcc=tf.Wcc, model_var=tf.model.model_var)
    for i in sorted({0, B // 2, B - 1}):
        one = tf.apply(f, means[i], covs[i], np.atleast_1d(0))
        assert np.array_equal(one[0], mf[i]) and np.array_equal(one[1], cf[i]) and np.array_equal(one[2], cfx[i])
        ref = orc.apply_bq(orc.F_PENDULUM_DYN, means[i], covs[i], 0, orc.points_ut(2), w, (0.01,))
        assert_moments_close((mf[i], cf[i], cfx[i]), ref, covs[i], what=(B, i))


def test_device_resident_api_with_padded_pitch(amd):
    """ssmq_apply_batch_dev on SoA planes whose pitch ld is larger than B; padding lanes are never touched."""
    from ssmtoybox_amd import _lib, ssmod as sm
    B, ld, D = 1000, 1280, 5
    means, covs = synthetic_reentry6(B)
    means, covs = means[:, :D], covs[:, :D, :D]
    tf = amd.UnscentedTransform(D)
    f = sm.ReentryVehicle2DTransition(dt=0.1).dyn_eval
    mean, cov = _lib.SoA.from_host(means, ld), _lib.SoA.from_host(covs, ld)
    mf, cf, cfx = _lib.SoA(D, B, ld), _lib.SoA(D * D, B, ld), _lib.SoA(D * D, B, ld)
    sentinel = np.full((D * D, ld), 7.25)
    for buf in (cf, cfx):
        buf.buf.upload(sentinel)
    st = _lib.DeviceBuffer(4 * ld)
    tbuf = _lib.DeviceBuffer(8)
    tbuf.upload(np.zeros(1))
    tf.apply_batch_dev(f, mean, cov, tbuf, mf, cf, cfx, st, 0)
    _lib.sync()
    ref = tf.apply_batch(f, means, covs, 0.0)
    assert np.array_equal(mf.to_host(), ref[0]) and np.array_equal(cf.to_host((D, D)), ref[1])
    assert np.array_equal(cfx.to_host((D, D)), ref[2])
    planes = cf.buf.download((D * D, ld))
    assert np.all(planes[:, B:] == 7.25)                       # nothing written beyond the batch
    assert not st.download((ld,), dtype=np.int32)[:B].any()


def test_sixteen_million_trajectories_64bit_offsets(amd):
    """Maximum-size case: B = 1.6e7 at D = E = 6 (5.4 GB in, 10 GB out; element offsets inside one buffer pass 2^32
    bytes).  The batch is a 65 536-trajectory block tiled on the device; every sampled tile must reproduce the block's
    own result bit for bit, first to last lane."""
    from ssmtoybox_amd import _lib, ssmod as sm
    lib = _lib.load()
    D, b0, B = 6, 65536, 16000000
    means, covs = synthetic_reentry6(b0, seed=4)
    tf = amd.GaussianProcessTransform(6, 6, np.array([[1.0] + [3.0] * 6]), 'rbf', 'ut')
    f = sm.ReentryVehicle2DBiasTransition(dt=0.1).dyn_eval
    small = [_lib.SoA.from_host(means), _lib.SoA.from_host(covs)]
    big = [_lib.SoA(D, B), _lib.SoA(D * D, B)]
    assert big[1].ld == B and 8 * 35 * B > 2 ** 32
    tiles = [(lo, min(b0, B - lo)) for lo in range(0, B, b0)]
    for src, dst in zip(small, big):
        for e in range(src.n):
            for lo, n in tiles:
                _lib.check(lib.ssmq_memcpy_d2d(dst.buf.at(8 * (e * dst.ld + lo)), src.buf.at(8 * e * src.ld),
                                               ctypes.c_size_t(8 * n)), 'ssmq_memcpy_d2d')
    tbuf = _lib.DeviceBuffer(8)
    tbuf.upload(np.zeros(1))

    def run(inp, nb):
        out = [_lib.SoA(D, nb), _lib.SoA(D * D, nb), _lib.SoA(D * D, nb)]
        st = _lib.DeviceBuffer(4 * out[0].ld)
        tf.apply_batch_dev(f, inp[0], inp[1], tbuf, out[0], out[1], out[2], st, 0)
        _lib.sync()
        first = ctypes.c_int64(-1)
        _lib.check(lib.ssmq_status_first(ctypes.c_void_p(st.ptr), nb, ctypes.byref(first)), 'ssmq_status_first')
        assert first.value < 0
        st.free()
        return out
    ref = [o.buf.download((o.n, o.ld)) for o in run(small, b0)]
    out = run(big, B)
    for lo, n in (tiles[0], tiles[len(tiles) // 2], tiles[-2], tiles[-1]):
        for o, r in zip(out, ref):
            for e in (0, o.n // 2, o.n - 1):
                got = o.buf.download((n,), byte_offset=8 * (e * o.ld + lo))
                assert np.array_equal(got, r[e, :n]), (lo, e)
    for buf in small + big + out:
        buf.buf.free()


def test_filter_calls_with_changing_batch_size(amd, golden):
    """The filter loop keeps its workspace and constants between calls: a call with another batch size (another pitch,
    hence another carve-up of the workspace) must not leave the next one with stale constants."""
    from ssmtoybox_amd import ssinf, ssmod as sm
    y = golden('g4_filters')['ungm_y']                     # (1, T, 8)
    dyn = sm.UNGMTransition(sm.GaussRV(1), sm.GaussRV(1, cov=np.array([[10.0]])))
    obs = sm.UNGMMeasurement(sm.GaussRV(1), 1)
    par = np.array([[1.0, 3.0]])
    for alg in (ssinf.GaussianProcessKalman(dyn, obs, par, par, 'rbf', 'ut'), ssinf.GaussHermiteKalman(dyn, obs, deg=5)):
        first = alg.forward_pass_batch(y)
        alg.forward_pass_batch(np.tile(y, (1, 1, 700)))    # 5600 trajectories: larger pitch, workspace regrown
        again = alg.forward_pass_batch(y)
        assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])
        one = alg.forward_pass_batch(y[..., :1])
        assert np.array_equal(one[0][..., 0], first[0][..., 0])


def test_device_resident_study_at_scale(amd):
    """Simulate -> filter -> error statistics without touching the host, B = 6.4e6 UNGM trajectories x T = 100
    (5 GB per buffer: plane offsets pass 2^32 bytes).  Trajectories are named by their global index, so the first and
    the last 65 536 of the big run must equal two small runs bit for bit, and the sums of the two halves of a mid-size
    run must add up."""
    from ssmtoybox_amd import ssinf, ssmod as sm, mcshard
    dyn = sm.UNGMTransition(sm.GaussRV(1), sm.GaussRV(1, cov=np.array([[10.0]])))
    obs = sm.UNGMMeasurement(sm.GaussRV(1), 1)
    par = np.array([[1.0, 3.0]])
    alg = ssinf.GaussianProcessKalman(dyn, obs, par, par, 'rbf', 'ut')
    T, B, b0, seed = 100, 6400000, 65536, 31
    assert 8 * T * B > 2 ** 32

    def study(nb, offset):
        d_x, d_y, ld = sm.simulate_dev(dyn, obs, T, nb, seed=seed, traj_offset=offset)
        d_fm, d_fP, d_st = alg.forward_pass_dev(d_y, nb, ld, T)
        return dict(x=d_x, y=d_y, fm=d_fm, fP=d_fP, st=d_st, ld=ld, nb=nb)

    def free(r):
        for k in ('x', 'y', 'fm', 'fP', 'st'):
            r[k].free()
    big = study(B, 0)
    s_big = mcshard.device_error_sums(1, B, big['ld'], T, big['x'], big['fm'], big['fP'], big['st'])
    assert np.all(s_big['n_ok'] + (B - s_big['n_ok'][0]) == B) and s_big['n_ok'][0] > 0.99 * B
    for offset in (0, B - b0):
        small = study(b0, offset)
        for key in ('y', 'fm', 'fP'):
            for t in (0, T // 2, T - 1):
                a = big[key].download((b0,), byte_offset=8 * (t * big['ld'] + offset))
                assert np.array_equal(a, small[key].download((b0,), byte_offset=8 * t * small['ld']),
                                      equal_nan=True), (key, t, offset)
        sa = big['st'].download((b0,), dtype=np.int32, byte_offset=4 * offset)
        assert np.array_equal(sa, small['st'].download((b0,), dtype=np.int32))
        free(small)
    free(big)
    # additivity of the device sums over a split by global index
    whole, lo, hi = study(200000, 0), study(120000, 0), study(80000, 120000)
    sums = [mcshard.device_error_sums(1, r['nb'], r['ld'], T, r['x'], r['fm'], r['fP'], r['st']) for r in (whole, lo, hi)]
    for k in sums[0]:
        assert np.allclose(sums[1][k] + sums[2][k], sums[0][k], rtol=1e-11, atol=1e-9), k
    rm = mcshard.finalize(sums[0])['rmse_total']
    assert 5.0 < rm < 20.0          # the known behaviour of this filter on UNGM (bench.py reports ~12.4)
    for r in (whole, lo, hi):
        free(r)


def test_weights_can_be_replaced_after_construction(amd):
    """The reference's research scripts assign tf.wm / tf.Wc / tf.Wcc / model.model_var after construction; the device
    constants must follow (research/tpq/tpq_ungm.py:114-124, research/bsq/bsq_tracking.py:276-281)."""
    from ssmtoybox_amd import ssmod as sm
    f = sm.UNGMTransition().dyn_eval
    tf = amd.GaussianProcessTransform(1, 1, np.array([[1.0, 3.0]]))
    m, P = np.array([0.3]), np.array([[2.0]])
    a = tf.apply(f, m, P, np.atleast_1d(2))
    w = orc.gp_weights([1.0, 0.7], orc.points_ut(1))
    tf.wm, tf.Wc, tf.Wcc, tf.model.model_var = w['wm'], w['Wc'], w['Wcc'], w['model_var']
    b = tf.apply(f, m, P, np.atleast_1d(2))
    ref = orc.apply_bq(orc.F_UNGM_DYN, m, P, 2, orc.points_ut(1), w)
    assert not np.allclose(a[1], b[1])
    assert_moments_close(b, ref, P)
    tf.model.model_var = np.array([[0.5]])                      # matrix-valued model variance
    c = tf.apply(f, m, P, np.atleast_1d(2))
    assert np.isclose(c[1][0, 0] - b[1][0, 0], 0.5 - w['model_var'])
    # apply(..., kern_par) re-computes the weights on the device (bq/bqmtran.py:93-95)
    d = tf.apply(f, m, P, np.atleast_1d(2), np.array([[1.0, 0.7]]))
    assert rel_err(tf.wm, w['wm']) < 1e-10 and rel_err(d[0], b[0]) < 1e-10


def test_theta_batched_weights_large(amd):
    """One launch, 512 parameter rows (the length-scale sweeps of research/bsq/bsq_ungm.py:190-282)."""
    from ssmtoybox_amd.bq.bqkern import device_gp_weights
    pts = orc.points_ut(3)
    ells = np.linspace(0.5, 6.0, 512)
    pars = np.column_stack((np.ones(512), ells, ells, ells))
    w = device_gp_weights(pts, pars)
    assert w['wm'].shape == (512, 7) and not w['status'].any()
    for i in (0, 100, 511):
        ref = orc.gp_weights(pars[i], pts)
        cond = np.linalg.cond(orc.rbf_eval(pars[i], pts, scaling=False) + 1e-8 * np.eye(7))
        for key, bar in (('wm', max(1e-10, 64 * cond * 2.2e-16)), ('Wc', max(1e-10, 8 * cond ** 2 * 2.2e-16))):
            what = 'theta-batched weights row {} {} vs oracle'.format(i, key)
            assert within(rel_err(w[key][i], ref[key]), capped(bar, what), what)


def test_many_workgroup_weights_route(amd, monkeypatch):
    """Point sets beyond the CU-resident route (N > 201): factor, inverse and the two N^3 products on many workgroups
    (k_wb_*, csrc/ssmq_weights.hip) against the single-workgroup route of earlier rounds (SSMQ_WEIGHTS_ONE_WG=1), three
    parameter rows in one call, the middle one not positive definite (NaN length scale): status and NaN outputs for that row
    only.  GP on N = 300 random points at D = 3, then Bayes-Sard (10 basis functions) through the transform on the same set
    shape (N = 343: Gauss-Hermite degree 7 at D = 3)."""
    from ssmtoybox_amd.bq.bqkern import device_gp_weights
    from ssmtoybox_amd import _lib as _amdlib
    rng = np.random.default_rng(12)
    pts = rng.standard_normal((3, 300))
    pars = np.array([[1.0, 0.6, 0.7, 0.5], [1.0, np.nan, 1.0, 1.0], [1.3, 0.4, 0.5, 0.6]])
    monkeypatch.delenv('SSMQ_WEIGHTS_ONE_WG', raising=False)
    with pytest.raises(np.linalg.LinAlgError):
        device_gp_weights(pts, pars)
    rows = pars[[0, 2]]
    new = device_gp_weights(pts, rows)
    monkeypatch.setenv('SSMQ_WEIGHTS_ONE_WG', '1')
    old = device_gp_weights(pts, rows)
    monkeypatch.delenv('SSMQ_WEIGHTS_ONE_WG')
    assert not new['status'].any() and not old['status'].any()
    for i in range(2):
        cond = np.linalg.cond(orc.rbf_eval(rows[i], pts, scaling=False) + 1e-8 * np.eye(300))
        assert np.array_equal(new['Q'][i], old['Q'][i]) and np.array_equal(new['q'][i], old['q'][i])
        for key, bar in (('iK', 64 * cond * 2.2e-16), ('wm', 64 * cond * 2.2e-16), ('Wcc', 64 * cond * 2.2e-16),
                         ('Wc', 8 * cond ** 2 * 2.2e-16)):
            what = 'many-workgroup weights row {} {} vs one workgroup'.format(i, key)
            assert within(rel_err(new[key][i], old[key][i]), capped(max(1e-12, bar), what), what)
        assert np.array_equal(new['Wc'][i], new['Wc'][i].T)
    # the status of the row that fails, next to two that do not (low-level call: the wrapper raises on the first failure)
    lib = _amdlib.load()
    x, px = _amdlib.as_c(pts)
    par, pp = _amdlib.as_c(pars)
    wm, Wc = _amdlib.out_c((3, 300)), _amdlib.out_c((3, 300, 300))
    st = np.zeros(3, dtype=np.int32)
    rc = lib.ssmq_weights_gp(3, 300, px, pp, 3, 1e-8, wm[1], Wc[1], None, None, None, None, None, None, None,
                             st.ctypes.data_as(_amdlib.c_int32_p))
    assert rc == 2 and list(st) == [0, 1, 0]
    assert np.isnan(wm[0][1]).all() and np.isnan(Wc[0][1]).all()
    assert np.array_equal(wm[0][0], new['wm'][0]) and np.array_equal(Wc[0][2], new['Wc'][1])
    # Bayes-Sard, general branch
    mi = np.array([[0, 1, 0, 0, 2, 1, 1, 0, 0, 0], [0, 0, 1, 0, 0, 1, 0, 2, 1, 0], [0, 0, 0, 1, 0, 0, 1, 0, 1, 2]])
    par = np.array([[1.0, 1.2, 1.1, 1.3]])
    tn = amd.BayesSardTransform(3, 3, par, mi, 'gh', {'degree': 7})
    monkeypatch.setenv('SSMQ_WEIGHTS_ONE_WG', '1')
    to = amd.BayesSardTransform(3, 3, par, mi, 'gh', {'degree': 7})
    monkeypatch.delenv('SSMQ_WEIGHTS_ONE_WG')
    assert tn.model.points.shape[1] == 343
    cond = np.linalg.cond(orc.rbf_eval(par[0], tn.model.points, scaling=False) + 1e-8 * np.eye(343))
    for key, bar in (('wm', 64 * cond * 2.2e-16), ('Wcc', 64 * cond * 2.2e-16), ('Wc', 8 * cond ** 2 * 2.2e-16)):
        what = 'many-workgroup Bayes-Sard weights {} vs one workgroup'.format(key)
        assert within(rel_err(getattr(tn, key), getattr(to, key)), capped(max(1e-12, bar), what), what)


def test_launch_loop_graph_follows_weight_updates(amd, golden, monkeypatch):
    """The launch-loop path caches its 3 T launches as a hipGraph.  Replacing a transform's weights keeps the handle and
    its constant-block addresses, but may change WHICH kernel variant qualifies (the LDL' fast path is withdrawn and its
    factors zeroed when the new Wc fails the acceptance test): the next pass must re-capture, not replay the stale
    variant.  Checked against a freshly built filter holding the same weights."""
    from ssmtoybox_amd import ssinf, ssmod as sm
    monkeypatch.delenv('SSMQ_NO_FASTPATH', raising=False)      # the premise of this test is that a fast path is selected
    g = golden('g4_filters')
    y = np.tile(g['rer_y'], (1, 1, 16))[:, :30]
    dyn = sm.ReentryVehicle2DTransition(sm.GaussRV(5, g['rer_m0'], g['rer_P0']), sm.GaussRV(3, cov=g['rer_Q']))
    obs = sm.Radar2DMeasurement(sm.GaussRV(2, cov=g['rer_R']), 5)
    mi = g['rer_bsqkf_mi']

    def make():
        a = ssinf.BayesSardKalman(dyn, obs, g['rer_bsqkf_par_dyn'], g['rer_bsqkf_par_obs'], mi, mi, 'ut')
        a.tf_dyn.model.model_var = 2e-6 * np.eye(5)
        a.tf_obs.model.model_var = 0 * np.eye(2)
        return a
    monkeypatch.setenv('SSMQ_NO_FUSED', '1')
    alg = make()
    f_dyn = dyn.dyn_eval
    kn = alg.tf_dyn.kernel_name(f_dyn)
    assert ('OPT=3' in kn or 'OPT=7' in kn) and 'hipGraph' in alg.kernel_name()
    fm1, fP1 = alg.forward_pass_batch(y, raise_on_failure=False)
    fm1b, _ = alg.forward_pass_batch(y, raise_on_failure=False)          # replay of the captured loop
    assert np.array_equal(fm1, fm1b, equal_nan=True)
    # an asymmetric 1e-10-sized perturbation: same filter for all practical purposes, but Wc no longer equals its
    # (symmetric) U diag(d) U' factorisation to 1e-14, so the LDL' variant is withdrawn
    Wc2 = alg.tf_dyn.Wc.copy()
    Wc2[1, 0] += 1e-10 * np.max(np.abs(Wc2))
    alg.tf_dyn.Wc = Wc2
    assert 'OPT=3' not in alg.tf_dyn.kernel_name(f_dyn) and 'OPT=7' not in alg.tf_dyn.kernel_name(f_dyn)       # the dense kernel (no BQ instantiation with only the point-set fast path)
    fm2, fP2 = alg.forward_pass_batch(y, raise_on_failure=False)
    fresh = make()
    fresh.tf_dyn.Wc = Wc2
    fm3, fP3 = fresh.forward_pass_batch(y, raise_on_failure=False)
    assert np.array_equal(fm2, fm3, equal_nan=True) and np.array_equal(fP2, fP3, equal_nan=True)
    ok = (alg.status == 0)
    assert ok.mean() > 0.9 and np.all(np.isfinite(fm2[..., ok]))
    # and back: the original weights give the original pass again
    alg.tf_dyn.Wc = fresh.tf_dyn.Wc * 0 + make().tf_dyn.Wc
    fm4, _ = alg.forward_pass_batch(y, raise_on_failure=False)
    assert np.array_equal(fm4, fm1, equal_nan=True)


def test_rccl_communicator_single_rank(amd, tmp_path):
    """The collective of the path through the C ABI (ssmq_comm_* / ssmq_allreduce_*: RCCL opened by libssmq at run
    time, no PyTorch), with a real RCCL communicator of one rank: rendezvous file, sum / max, barrier, teardown."""
    from ssmtoybox_amd import mcshard
    idf = str(tmp_path / 'rccl.id')
    comm = mcshard.RcclComm(0, 1, id_file=idf, force=True)
    assert os.path.getsize(idf) == 128
    v = np.arange(1000, dtype=float) * 0.5 - 3.0
    assert np.array_equal(comm.allreduce_sum(v), v) and np.array_equal(comm.allreduce_max(v), v)
    sums = dict(a=np.ones((3, 2)), b=np.arange(4.0))
    tot = mcshard.allreduce_sums(sums, comm)
    assert np.array_equal(tot['a'], sums['a']) and np.array_equal(tot['b'], sums['b'])
    comm.barrier()
    comm.close()
    assert not os.path.exists(idf)
    with pytest.raises(Exception):
        mcshard.RcclComm(1, 1)            # rank out of range: refused by ssmq_comm_init


# ---------------------------------------------------------------------------------------------------------------
# BASELINE.json configs as full-size parity cases: device filter loop vs the C oracle on the same trajectories
# ---------------------------------------------------------------------------------------------------------------
def _c_bq_transform(tf, E, integ, nu=0.0, broadcast=0):
    from oracle import c_oracle as co
    mv = tf.model.model_var
    emv = (np.asarray(mv, dtype=float) * np.ones((E, E))) if np.ndim(mv) == 0 else np.asarray(mv, dtype=float)
    return co.make_transform(0, tf.model.points.shape[0], E, tf.model.points, tf.wm, tf.Wc, tf.Wcc, emv, broadcast, nu,
                             tf.model.iK if nu > 0 else None, integ)


def _compare_filter(fm, fP, st, cfm, cfP, cst, first=10, tol_first=1e-9, tol_median=1e-12, tol_q99=1e-8):
    """Trajectory-wise comparison of two filter runs on identical inputs/weights.  The recursion amplifies rounding
    differences (uncentred BQ covariance), so: tight over the first steps for every trajectory, and median / 99th
    percentile over the full length."""
    both = (st == 0) & (cst == 0)
    assert both.mean() > 0.5
    assert np.array_equal(st == 0, cst == 0) or (np.sum((st == 0) != (cst == 0)) <= 0.002 * st.size)
    scale = np.max(np.abs(cfm[:, :, both]), axis=(1, 2), keepdims=True)
    rel = np.max(np.abs(fm - cfm)[:, :, both] / scale, axis=0)          # (T, b)
    stats = (float(np.max(rel[:first])), float(np.median(rel)), float(np.quantile(rel, 0.99)))
    assert stats[0] < tol_first and stats[1] < tol_median and stats[2] < tol_q99, stats
    return rel


def test_config2_ungm_gpqkf_1e4(amd):
    """BASELINE configs[1]: GPQ-Kalman on UNGM, 1e4 MC runs, T = 100 - every trajectory against the C oracle."""
    from oracle import c_oracle as co
    from bench import simulate_ungm
    from ssmtoybox_amd import ssinf, ssmod as sm
    B, T = 10000, 100
    x, y = simulate_ungm(B, T, 11)
    dyn = sm.UNGMTransition(sm.GaussRV(1), sm.GaussRV(1, cov=np.array([[10.0]])))
    obs = sm.UNGMMeasurement(sm.GaussRV(1), 1)
    par = np.array([[1.0, 3.0]])
    alg = ssinf.GaussianProcessKalman(dyn, obs, par, par)
    fm, fP = alg.forward_pass_batch(y[None], raise_on_failure=False)
    td, k1 = _c_bq_transform(alg.tf_dyn, 1, co.Integrand.make(orc.F_UNGM_DYN))
    to, k2 = _c_bq_transform(alg.tf_obs, 1, co.Integrand.make(orc.F_UNGM_MEAS))
    one = np.eye(1)
    cfm, cfP, cst = co.filter_forward(td, to, np.ascontiguousarray(y.T[:, :, None]), np.zeros(1), one, 10 * one, one,
                                      threads=8)
    _compare_filter(fm, fP, alg.status, cfm.transpose(2, 1, 0), cfP.transpose(2, 3, 1, 0), cst)


def test_lengthscale_filter_sweep(amd):
    """research/bsq/bsq_ungm.py:190-240 (`lengthscale_filter_demo`): GPQ-Kalman on UNGM re-built for every length-scale of
    a grid and run over the same 20 measurement sequences of 500 steps, then RMSE / NLL / credibility ratio per grid
    point.  Every filter run is compared with the C oracle on the device's own weights; the error statistics come from
    the device reductions and are compared with the oracle's restatement of utils.py on the downloaded moments."""
    from oracle import c_oracle as co
    from bench import simulate_ungm
    from ssmtoybox_amd import ssinf, ssmod as sm, mcshard
    steps, mc = 500, 20
    x, y = simulate_ungm(mc, steps, 23)
    dyn = sm.UNGMTransition(sm.GaussRV(1, cov=np.array([[5.0]])), sm.GaussRV(1, cov=np.array([[10.0]])))
    obs = sm.UNGMMeasurement(sm.GaussRV(1), 1)
    one = np.eye(1)
    rmse = []
    for el in (1e-1, 3e-1, 1.0, 3.0, 1e1, 3e1):
        par = np.array([[1.0, el]])
        alg = ssinf.GaussianProcessKalman(dyn, obs, par, par, kernel='rbf', points='ut')
        fm, fP = alg.forward_pass_batch(y[None], raise_on_failure=False)
        td, keep1 = _c_bq_transform(alg.tf_dyn, 1, co.Integrand.make(orc.F_UNGM_DYN))     # keep*: the structs point into them
        to, keep2 = _c_bq_transform(alg.tf_obs, 1, co.Integrand.make(orc.F_UNGM_MEAS))
        cfm, cfP, cst = co.filter_forward(td, to, np.ascontiguousarray(y.T[:, :, None]), np.zeros(1), 5.0 * one,
                                          10 * one, one, threads=4)
        cfm, cfP = cfm.transpose(2, 1, 0), cfP.transpose(2, 3, 1, 0)
        st = alg.status
        assert np.array_equal(st == 0, cst == 0), el
        ok = st == 0
        assert ok.sum() >= mc // 2, (el, int(ok.sum()))
        # 500 steps of a recursion that amplifies rounding differences: tight at the start, percentiles over the run
        rel = np.abs(fm - cfm)[0][:, ok] / np.abs(cfm[0][:, ok]).max()
        assert within(float(rel[:10].max()), 1e-10, 'lengthscale sweep l={} first steps'.format(el))
        assert within(float(np.median(rel)), 1e-11, 'lengthscale sweep l={} median'.format(el))
        # error statistics of this grid point, device reductions vs the oracle on the same moments
        ld = 64
        d_x, d_m, d_P = _planes(x[None, :, :], ld), _planes(fm, ld), _planes(fP, ld)
        stl = np.zeros(ld, dtype=np.int32)
        stl[:mc] = st
        d_st = _lib_buffer(stl)
        s1 = mcshard.device_error_sums(1, mc, ld, steps, d_x, d_m, d_P, d_st)
        o1 = orc.error_sums(x[None, :, :], fm, fP, ok)
        for k in ('se', 'rmse', 'nll', 'mse', 'n_ok', 'n_pd'):
            assert np.allclose(s1[k], o1[k], rtol=1e-10, atol=1e-12), (el, k)
        tot = mcshard.finalize(s1)
        s2 = mcshard.device_lcr_sums(1, mc, ld, steps, d_x, d_m, d_P, tot['mse'], d_st)
        o2 = orc.lcr_sums(x[None, :, :], fm, fP, tot['mse'] + 1e-6 * np.eye(1), ok)
        assert np.allclose(s2['lcr'], o2['lcr'], rtol=1e-8, atol=1e-8) and np.array_equal(s2['n'], o2['n'])
        rmse.append(tot['rmse_total'])
        for buf in (d_x, d_m, d_P, d_st):
            buf.free()
    assert np.all(np.isfinite(rmse)) and max(rmse) / min(rmse) > 1.01      # the length-scale matters


def _compare_filter_prefix(fm, fP, st, cfm, cfP, cst, T, what, tol_m=1e-9, tol_P=1e-9):
    """Two runs of a filter that may lose positive definiteness (status = 1 + first failing step): every step BEFORE the
    first failure of either run is compared entry-wise - means in standard deviations (|dm_i| / sqrt(P_ii)), covariance
    entries against sqrt(P_ii P_jj).  Layouts (D, T, b) / (D, D, T, b).  Returns (mean error, covariance error)."""
    st, cst = np.asarray(st), np.asarray(cst)
    nd, nc = np.where(st > 0, st - 1, T), np.where(cst > 0, cst - 1, T)     # completed steps
    mask = np.arange(T)[:, None] < np.minimum(nd, nc)[None, :]                # (T, b)
    # nothing is reported for a step at or after the failure (NaN poison), everything before it is finite
    assert np.all(np.isfinite(fm[:, np.arange(T)[:, None] < nd[None, :]]))
    assert np.all(np.isnan(fm[:, np.arange(T)[:, None] >= nd[None, :]]))
    em = mean_err_sigma(fm, cfm, cfP, mask)
    eP = cov_err(fP, cfP, mask)
    assert within(em, tol_m, what + ': pre-failure means (in standard deviations)')
    assert within(eP, tol_P, what + ': pre-failure covariances (entry-scaled)')
    return em, eP


def _failing_matrix_singularity(st, fm, fP, idx, y, m0, P0, GQG, R, pts, wd, wo, f_dyn, p_dyn, f_obs, p_obs):
    """For the sampled trajectories: restart the NumPy oracle from the device's own state one step before the device
    reported its failure and return, per trajectory, |lambda_min| / lambda_max of the matrix whose factorisation the step
    needs next and that is closest to singular (input covariance, predictive covariance, innovation covariance).
    ~0 means that matrix is numerically singular: whether a Cholesky factorisation 'succeeds' is then decided by the
    last bits of the rounding, i.e. by the order of the floating-point operations, in any implementation."""
    out = []
    for b in idx:
        k = int(st[b]) - 1
        m, P = (m0, P0) if k == 0 else (fm[:, k - 1, b], fP[:, :, k - 1, b])
        ratios = []

        def ratio(a):
            ev = np.linalg.eigvalsh(0.5 * (a + a.T))
            ratios.append(float(np.min(np.abs(ev)) / np.max(np.abs(ev))) if ev[0] > 0 else 0.0)
            return ev[0] > 0
        if ratio(P):
            try:
                pm, pP, _ = orc.apply_bq(f_dyn, m, P, float(k), pts, wd, p_dyn)
                pP = pP + GQG
                if ratio(pP):
                    ym, S, _ = orc.apply_bq(f_obs, pm, pP, float(k), pts, wo, p_obs)
                    ratio(S + R)
            except np.linalg.LinAlgError:
                ratios.append(0.0)
        out.append(min(ratios))
    return np.array(out)


@pytest.mark.parametrize('ell', [3.0, 25.0])
def test_config3_gpqkf_reentry6_1e5_vs_oracle(amd, ell, monkeypatch):
    """BASELINE configs[2]: GPQ-Kalman on the 6-D reentry-shaped model, 1e5 MC runs (one GPU's share), the fused time
    loop against the C oracle with IDENTICAL weights - both kernel variants (LDL' / unscented-point fast path, dense).

    What this recursion is on this model (measured, tools/c3_gpq_stats.py; the reference's author calls GPQKF fragile
    here, research/gpq/gpq_tracking.py:590-592, and the reference itself raises LinAlgError at step 1 on the 5-D model at
    its own l = 25): the GP weights do not sum to one, so the uncentred covariance fx Wc fx' - m m' (bq/bqmtran.py:199)
    of a 6.5e3-sized state is (1'Wc 1 - 1) m m' + O(1e-6): a numerically RANK-ONE matrix.
      * l = 25: every trajectory fails at step 1, in the device loop, in the C oracle and in the reference - asserted.
      * l = 3: all runs are finite for 1-3 steps and then hit a Cholesky factorisation of a numerically singular matrix;
        which step that is depends on the last bits (device fast path / device dense / C oracle agree on the step for
        only 31-42 % of the trajectories among EACH OTHER, within +-1 step for 78-87 %).  So the failing step itself
        cannot be pinned.  Pinned instead, on all 1e5 trajectories: every moment of every step before the first failure
        (entry-wise, 1e-9), the poisoning / flagging of the rest, the distribution of the failing step, and - on a sample -
        that the matrix the device gave up on is numerically singular in the oracle's arithmetic too."""
    from oracle import c_oracle as co
    from bench import simulate_reentry
    from ssmtoybox_amd import ssinf, ssmod as sm
    B, T = 100000, 50
    x, y, m0, P0, Q, G, R = simulate_reentry(B, T, 12, True)
    dyn = sm.ReentryVehicle2DBiasTransition(sm.GaussRV(6, m0, P0), sm.GaussRV(4, cov=Q))
    obs = sm.Radar2DMeasurement(sm.GaussRV(2, cov=R), 6)
    par = np.array([[1.0] + [ell] * 6])
    GQG = G.dot(Q).dot(G.T)
    cfm = cfP = cst = None
    for fast in (True, False):
        tag = 'configs[2] GPQKF l=%g %s' % (ell, 'fast' if fast else 'dense')
        if fast:
            monkeypatch.delenv('SSMQ_NO_FASTPATH', raising=False)
        else:
            monkeypatch.setenv('SSMQ_NO_FASTPATH', '1')
        gpq = ssinf.GaussianProcessKalman(dyn, obs, par, par)
        # (fast: OPT=7 where both transforms' weights are reflection-symmetric to 2e-13 - length scale 3 -, else OPT=3)
        kn = gpq.kernel_name()
        assert (('OPT=7' in kn or 'OPT=3' in kn) if fast else 'OPT=0' in kn) and 'k_filter_fused<D=6,Y=2' in kn, kn
        if fast and ell == 3.0 and 'SSMQ_NO_SYM' not in os.environ:
            assert 'OPT=7' in kn, kn
        if fast:
            with pytest.raises(np.linalg.LinAlgError):
                gpq.forward_pass_batch(y[:, :, :4096])
        fm, fP = gpq.forward_pass_batch(y, raise_on_failure=False)
        st = gpq.status.copy()
        if cst is None:
            td, k1 = _c_bq_transform(gpq.tf_dyn, 6, co.Integrand.make(orc.F_REENTRY2D_BIAS_DYN, (0.1,)))
            to, k2 = _c_bq_transform(gpq.tf_obs, 2, co.Integrand.make(orc.F_RADAR2D_MEAS, (0.0, 0.0)))
            cfm, cfP, cst = co.filter_forward(td, to, np.ascontiguousarray(y.transpose(2, 1, 0)), m0, P0, GQG, R,
                                              threads=16)
            cfm, cfP = cfm.transpose(2, 1, 0), cfP.transpose(2, 3, 1, 0)
        _compare_filter_prefix(fm, fP, st, cfm, cfP, cst, T, tag)
        if ell == 25.0:
            assert np.all(st == 1) and np.all(cst == 1)           # as the reference: LinAlgError in the first step
            continue
        nd, nc = np.where(st > 0, st, T + 1), np.where(cst > 0, cst, T + 1)
        assert within(abs(np.median(nd) - np.median(nc)), 0.5, tag + ': |median failing step - oracle median|')
        assert within(1.0 - np.mean(np.abs(nd - nc) <= 1), 0.3, tag + ': failing step differs by more than one')
        assert within(abs(np.mean(st == 0) - np.mean(cst == 0)), 2e-3, tag + ': surviving fraction vs oracle')
        # the matrix the device could not factor is numerically singular when the oracle recomputes it from the device's
        # own previous state
        wd = dict(wm=gpq.tf_dyn.wm, Wc=gpq.tf_dyn.Wc, Wcc=gpq.tf_dyn.Wcc, model_var=gpq.tf_dyn.model.model_var)
        wo = dict(wm=gpq.tf_obs.wm, Wc=gpq.tf_obs.Wc, Wcc=gpq.tf_obs.Wcc, model_var=gpq.tf_obs.model.model_var)
        idx = np.random.default_rng(5).choice(np.flatnonzero(st > 0), 300, replace=False)
        r = _failing_matrix_singularity(st, fm, fP, idx, y, m0, P0, GQG, R, gpq.tf_dyn.model.points, wd, wo,
                                        orc.F_REENTRY2D_BIAS_DYN, (0.1,), orc.F_RADAR2D_MEAS, (0.0, 0.0))
        assert within(float(np.max(r)), 1e-9, tag + ': |lambda_min| / lambda_max of the matrix that failed to factor')
    monkeypatch.delenv('SSMQ_NO_FASTPATH', raising=False)


def test_config3_reentry_filters_1e5(amd):
    """BASELINE configs[2], the filters that ARE stable on the reentry model: the unscented filter on the 6-D variant
    (1e5 MC runs on the device, a 4000-trajectory sample against the C oracle) and the Bayes-Sard filter on the
    reference's 5-D model in the configuration of the reference's own reentry study
    (research/bsq/bsq_tracking.py:263-281).  The GPQ-Kalman loop is test_config3_gpqkf_reentry6_1e5_vs_oracle."""
    from oracle import c_oracle as co
    from bench import simulate_reentry
    from ssmtoybox_amd import ssinf, ssmod as sm
    B, T = 100000, 50
    x, y, m0, P0, Q, G, R = simulate_reentry(B, T, 12, True)
    dyn = sm.ReentryVehicle2DBiasTransition(sm.GaussRV(6, m0, P0), sm.GaussRV(4, cov=Q))
    obs = sm.Radar2DMeasurement(sm.GaussRV(2, cov=R), 6)
    # unscented filter, all 1e5 trajectories on the device, a 4000-trajectory sample against the oracle
    alg = ssinf.UnscentedKalman(dyn, obs)
    assert 'k_filter_fused<D=6,Y=2' in alg.kernel_name()
    # the ROUTE this batch takes (ssmq_filter_kernel_name_batch), not only the shape: 1 563 blocks on 1 024 SIMDs -> the strips
    # (tools/alt_paths.sh forces the choice either way through the environment; then the forced route is the one named)
    forced = os.environ.get('SSMQ_FUSED_CHUNKED')
    if forced is None and 'SSMQ_NO_FUSED' not in os.environ:
        assert 'k_filter_chunked<D=6,Y=2' in alg.kernel_name(B), alg.kernel_name(B)
    elif forced == '0':
        assert 'k_filter_fused<D=6,Y=2' in alg.kernel_name(B)
    fm, fP = alg.forward_pass_batch(y)
    idx = np.random.default_rng(0).choice(B, 4000, replace=False)
    pts = orc.points_ut(6)
    wm, wc = orc.weights_ut(6)
    td, k3 = co.make_transform(1, 6, 6, pts, wm, wc, integrand=co.Integrand.make(orc.F_REENTRY2D_BIAS_DYN, (0.1,)))
    to, k4 = co.make_transform(1, 6, 2, pts, wm, wc, integrand=co.Integrand.make(orc.F_RADAR2D_MEAS, (0.0, 0.0)))
    cfm, cfP, cst = co.filter_forward(td, to, np.ascontiguousarray(y[:, :, idx].transpose(2, 1, 0)), m0, P0,
                                      G.dot(Q).dot(G.T), R, threads=8)
    assert not cst.any() and not alg.status.any()
    assert within(mean_err(fm[:, :, idx], cfm.transpose(2, 1, 0)), 1e-8, 'configs[2] UKF 6-D fm vs oracle (row-scaled)')
    assert within(cov_err(fP[:, :, :, idx], cfP.transpose(2, 3, 1, 0)), 2e-8, 'configs[2] UKF 6-D fP vs oracle (entry-scaled)')
    rmse = np.sqrt(np.mean((fm[:2] - x[:2]) ** 2))
    assert rmse < 0.2       # sanity only: the filter tracks (position error, km)
    # Bayes-Sard filter on the reference's 5-D model as its reentry study configures it
    Bs = 20000
    x5, y5, m5, P5, Q5, G5, R5 = simulate_reentry(Bs, T, 13, False)
    dyn5 = sm.ReentryVehicle2DTransition(sm.GaussRV(5, m5, P5), sm.GaussRV(3, cov=Q5))
    obs5 = sm.Radar2DMeasurement(sm.GaussRV(2, cov=R5), 5)
    mi = np.hstack((np.zeros((5, 1)), np.eye(5), 2 * np.eye(5))).astype(int)
    bsq = ssinf.BayesSardKalman(dyn5, obs5, np.array([[1.0, 1, 1, 1, 1, 1]]), np.array([[1.0, 0.9, 0.9, 1e4, 1e4, 1e4]]),
                                mi, mi, 'ut')
    bsq.tf_dyn.model.model_var = 2e-6 * np.eye(5)
    bsq.tf_obs.model.model_var = 0 * np.eye(2)
    assert 'k_filter_fused<D=5,Y=2' in bsq.kernel_name()
    if 'SSMQ_FUSED_CHUNKED' not in os.environ and 'SSMQ_NO_FUSED' not in os.environ:
        assert 'k_filter_fused<D=5,Y=2' in bsq.kernel_name(Bs), bsq.kernel_name(Bs)      # 313 blocks: every wave has a SIMD, whole passes
    fm, fP = bsq.forward_pass_batch(y5, raise_on_failure=False)
    td, k5 = _c_bq_transform(bsq.tf_dyn, 5, co.Integrand.make(orc.F_REENTRY2D_DYN, (0.1,)))
    to, k6 = _c_bq_transform(bsq.tf_obs, 2, co.Integrand.make(orc.F_RADAR2D_MEAS, (0.0, 0.0)))
    cfm, cfP, cst = co.filter_forward(td, to, np.ascontiguousarray(y5[:, :, :2000].transpose(2, 1, 0)), m5, P5,
                                      G5.dot(Q5).dot(G5.T), R5, threads=8)
    good = (bsq.status[:2000] == 0) & (cst == 0)
    assert good.mean() > 0.95
    # unisolvent Bayes-Sard weights reproduce the UT rule: stable, but the covariance is still the uncentred form
    assert within(mean_err(fm[:, :, :2000][:, :, good], cfm.transpose(2, 1, 0)[:, :, good]), 1e-2,
                  'configs[2] BSQKF 5-D fm vs oracle (row-scaled)')
    _compare_filter_prefix(fm[:, :, :2000], fP[:, :, :, :2000], bsq.status[:2000], cfm.transpose(2, 1, 0),
                           cfP.transpose(2, 3, 1, 0), cst, T, 'configs[2] BSQKF 5-D', tol_m=0.1, tol_P=0.1)   # measured 4e-2 / 5e-2: the
    # uncentred form's own noise level on this model - two fp64 evaluations cannot be closer.  What pins the device here is
    # test_referee_reentry_bsqkf_device: against the EXACT recursion it is as close as the reference's own NumPy run.


def _referee_no_worse(got, ref, what, factor=2.0, floor=1e-12):
    """Per time step, pooled over the trajectories: the device's distance from the EXACT result against the reference's.
    The root mean square over trajectories and entries is held to `factor`; the maximum over a few dozen trajectories
    is itself a noisy statistic of two independent rounding-error samples and gets 1.5 x that."""
    for key, f in (('m_rms', factor), ('P_rms', factor), ('m_max', 1.5 * factor), ('P_max', 1.5 * factor)):
        ratio = float(np.max(got[key] / (ref[key] + floor)))
        assert within(ratio, f, '{}: max over steps of |device - exact| / |reference - exact| ({})'.format(what, key))
    # and over the whole run the two are equally good: mean ratio of the per-step rms errors
    for key in ('m_rms', 'P_rms'):
        assert within(float(np.mean(got[key] / (ref[key] + floor))), 1.25, '{}: mean over steps of the {} ratio'.format(what, key))


def test_referee_reentry_bsqkf_device(amd, monkeypatch):
    """BASELINE configs[2] with the filter that is stable on the reentry model, refereed in extended precision: the
    reference's NumPy evaluation of this recursion is itself 1e-2 (covariance, entry-scaled) / 0.9 standard deviations
    (mean) away from the exact result of its algorithm at step 1 (uncentred covariance, bq/bqmtran.py:199;
    tests/test_referee.py) - so device-vs-reference differences of a few per cent say nothing.  What is asserted here:
    at every step the device is no further from the EXACT moments (oracle/ssmq_referee.py, 40 digits, same fp64 weights
    and measurements) than twice the reference's own distance - for the dense kernels and for the LDL' fast path."""
    from ssmtoybox_amd import ssinf, ssmod as sm
    from tests import _referee as rf
    g = rf.load()
    xm, xP = rf.reentry_exact()
    ref = rf.step_errors(g['rer_fm'], g['rer_fc'], xm, xP)
    dyn = sm.ReentryVehicle2DTransition(sm.GaussRV(5, g['rer_m0'], g['rer_P0']), sm.GaussRV(3, cov=g['rer_Q']))
    obs = sm.Radar2DMeasurement(sm.GaussRV(2, cov=g['rer_R']), 5)
    mi = np.hstack((np.zeros((5, 1)), np.eye(5), 2 * np.eye(5))).astype(int)
    for fast in (True, False):
        if fast:
            monkeypatch.delenv('SSMQ_NO_FASTPATH', raising=False)
        else:
            monkeypatch.setenv('SSMQ_NO_FASTPATH', '1')
        alg = ssinf.BayesSardKalman(dyn, obs, np.array([[1.0, 1, 1, 1, 1, 1]]), np.array([[1.0, 0.9, 0.9, 1e4, 1e4, 1e4]]),
                                    mi, mi, 'ut')
        for tf, tag in ((alg.tf_dyn, 'rer_dyn'), (alg.tf_obs, 'rer_obs')):
            tf.wm, tf.Wc, tf.Wcc = g[tag + '_wm'], g[tag + '_Wc'], g[tag + '_Wcc']       # the reference's weights
            tf.model.model_var = g[tag + '_mv']
        kn = alg.kernel_name()
        assert 'k_filter_fused<D=5,Y=2' in kn and ('OPT=3' in kn or 'OPT=7' in kn) == fast, kn
        fm, fP = alg.forward_pass_batch(g['rer_y'])
        assert not alg.status.any()
        got = rf.step_errors(fm, fP, xm, xP)
        _referee_no_worse(got, ref, 'reentry BSQKF ' + ('LDL fast path' if fast else 'dense kernels'))
    monkeypatch.delenv('SSMQ_NO_FASTPATH', raising=False)


def test_referee_ct_tpqkf_device(amd):
    """BASELINE configs[3] refereed the same way: t-process Kalman filter, coordinated turn + four bearing sensors, heavy-tailed
    measurement noise; all six steps (the verdict asked for steps 4-6, where the per-step bars against the C oracle are
    widest)."""
    from ssmtoybox_amd import ssinf, ssmod as sm
    from tests import _referee as rf
    g = rf.load()
    xm, xP = rf.ct_exact()
    ref = rf.step_errors(g['ct_fm'], g['ct_fc'], xm, xP)
    dyn = sm.CoordinatedTurnTransition(sm.GaussRV(5, g['ct_m0'], g['ct_P0']), sm.GaussRV(5, cov=g['ct_Q']), dt=float(g['ct_dt'][0]))
    obs = sm.BearingMeasurement(sm.GaussRV(4, cov=g['ct_R']), 5, state_index=[0, 2], sensor_pos=g['ct_sensors'])
    par = np.array([[1.0, 100, 100, 100, 100, 1]])
    alg = ssinf.StudentProcessKalman(dyn, obs, par, par)
    for tf, tag in ((alg.tf_dyn, 'ct_dyn'), (alg.tf_obs, 'ct_obs')):
        tf.wm, tf.Wc, tf.Wcc = g[tag + '_wm'], g[tag + '_Wc'], g[tag + '_Wcc']
        tf.model.iK = g[tag + '_iK']
        tf.model.model_var = float(g[tag + '_mv'][0, 0])
    assert 'k_filter_fused<D=5,Y=4' in alg.kernel_name()
    fm, fP = alg.forward_pass_batch(g['ct_y'], raise_on_failure=False)
    assert (alg.status == 0).mean() > 0.9
    got = rf.step_errors(np.where(alg.status[None, None] == 0, fm, np.nan), fP, xm, xP)
    _referee_no_worse(got, ref, 'coordinated-turn TPQKF', factor=3.0)


def stats_kurtosis(v):
    v = np.asarray(v, dtype=float) - np.mean(v)
    return float(np.mean(v ** 4) / np.mean(v ** 2) ** 2 - 3.0)


def test_config4_tpq_ct_bearing_1e4(amd):
    """BASELINE configs[3]: Student-t process quadrature Kalman filter, 5-D coordinated-turn state, bearing sensors,
    1e4 MC runs (StudentProcessKalman builds its transforms with dim_out = 1: broadcast model variance)."""
    from oracle import c_oracle as co
    from ssmtoybox_amd import ssinf, ssmod as sm
    B, T = 10000, 6
    rng = np.random.default_rng(14)
    m0 = np.array([1000, 300, 1000, 0, np.deg2rad(-3.0)])
    P0 = np.diag([100, 10, 100, 10, 0.1])
    dt, r1, r2 = 0.1, 0.1, 1.75e-4
    A = np.array([[dt ** 3 / 3, dt ** 2 / 2], [dt ** 2 / 2, dt]])
    Q = np.zeros((5, 5))
    Q[:2, :2], Q[2:4, 2:4], Q[4, 4] = r1 * A, r1 * A, r2 * dt
    Rn = 10e-3 * np.eye(4)
    dyn = sm.CoordinatedTurnTransition(sm.GaussRV(5, m0, P0), sm.GaussRV(5, cov=Q), dt=dt)
    obs = sm.BearingMeasurement(sm.GaussRV(4, cov=Rn), 5, state_index=[0, 2], sensor_pos=SENSORS)
    # heavy-tailed synthetic measurements from the PRODUCT's simulator: true bearings of a noisy turn + Student-t (nu = 3)
    # noise of scale 0.1 (the filter itself is told the Gaussian R above, as a mismatched-noise study would)
    sim_obs = sm.BearingMeasurement(sm.StudentRV(4, scale=0.01 * np.eye(4), dof=3.0), 5, state_index=[0, 2], sensor_pos=SENSORS)
    d_x, d_y, ld = sm.simulate_dev(dyn, sim_obs, T, B, seed=14)
    y = d_y.download((T, 4, ld))[:, :, :B].transpose(1, 0, 2)
    d_x.free()
    d_y.free()
    assert stats_kurtosis(y[0, 0] - np.median(y[0, 0])) > 3.0        # heavy tails are there
    par = np.array([[1.0, 100, 100, 100, 100, 1]])
    alg = ssinf.StudentProcessKalman(dyn, obs, par, par)
    assert 'k_filter_fused<D=5,Y=4' in alg.kernel_name()
    # the route at B = 1e4 (157 blocks on 1 024 SIMDs): the t-process form runs with its points split over two waves
    if 'SSMQ_FUSED_WSPLIT' not in os.environ and 'SSMQ_NO_FUSED' not in os.environ:
        assert 'k_filter_wsplit' in alg.kernel_name(B) and 'W=2>' in alg.kernel_name(B), alg.kernel_name(B)
    fm, fP = alg.forward_pass_batch(y, raise_on_failure=False)
    nu = float(alg.tf_dyn.model.nu)
    td, k1 = _c_bq_transform(alg.tf_dyn, 5, co.Integrand.make(orc.F_CT_DYN, (dt,)), nu, 1)
    to, k2 = _c_bq_transform(alg.tf_obs, 4, co.Integrand.make(orc.F_BEARING_MEAS, tuple(SENSORS.reshape(-1)), (0, 2)),
                             nu, 1)
    cfm, cfP, cst = co.filter_forward(td, to, np.ascontiguousarray(y.transpose(2, 1, 0)), m0, P0, Q, Rn, threads=8)
    # 1000-sized positions with 100-sized variances through the uncentred covariance: every step multiplies the
    # rounding difference between two evaluation orders by ~1e2 (step 1: 1e-14, step 5: 1e-9 ... 1e-6); nobody, the
    # reference's research code included (research/tpq/synthetic.py:2009-2014 has its TPQ filters commented out on this
    # model), runs this recursion for long.  First steps tight, the whole run in distribution.
    rel = _compare_filter(fm, fP, alg.status, cfm.transpose(2, 1, 0), cfP.transpose(2, 3, 1, 0), cst, first=3,
                          tol_first=1e-9, tol_median=1e-8, tol_q99=1.0)
    # step by step (all 1e4 trajectories): the growth described above, pinned per step.  This test covers the CONFIGURATION
    # (shapes, kernel selection, state-index pattern, t-process scaling with the broadcast model variance at B = 1e4); the
    # t-process arithmetic itself is pinned to 1e-10 by the reference's vectors (test_apply_golden: tpq / tpq1,
    # test_ungm_filter_golden[tpqkf], test_student_filters_golden).
    bars = (1e-10, 1e-9, 1e-8, 1e-6, 1e-4, 5e-2)     # measured maxima: 1.8e-12, 1.1e-11, 1.9e-10, 5.2e-8, 7.0e-6, 1.8e-3
    for k in range(T):
        assert within(float(np.max(rel[k])), bars[k], 'configs[3] TPQKF step %d max rel diff vs C oracle' % (k + 1))


# ---------------------------------------------------------------------------------------------------------------
# linearisation transform and the extended Kalman filter (mtran.py:49-59, ssinf.py:347-357; golden g13)
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('tag', ['ungm_dyn', 'ungmna_dyn', 'pend_dyn', 'cv_dyn', 'ungm_meas', 'ungmna_meas', 'pend_meas', 'pend_meas_idx'])
def test_linearization_transform_golden(amd, golden, tag):
    """LinearizationTransform.apply (k_linearize through ssmq_apply_batch) against the reference's outputs (golden g13) one
    input at a time, then one batch of 3000 inputs against the oracle; the host mirror of the model's Jacobian
    (dyn_eval / meas_eval with dx=True) against the oracle's."""
    g = golden('g13_linear')
    mod, kind, fid, p, idx = linear_models()[tag]
    f = mod.dyn_eval if kind == 'dyn' else mod.meas_eval
    D = mod.dim_in
    tf = amd.LinearizationTransform(D)
    assert tf.kernel_name(f) == 'k_linearize'
    for i in range(g[tag + '_mean'].shape[0]):
        mean, cov, t = g[tag + '_mean'][i], g[tag + '_cov'][i], g[tag + '_time'][i]
        got = tf.apply(f, mean, cov, np.atleast_1d(t))
        ref = (g[tag + '_mf'][i], g[tag + '_cf'][i], g[tag + '_cfx'][i])
        for a, b, what in zip(got, ref, ('mean', 'cov', 'ccov')):
            assert within(rel_err(a, b), 1e-12, 'g13 {} input {} {} vs the reference'.format(tag, i, what))
        # host mirror of meas_eval / dyn_eval with dx=True: the Jacobian in the columns of the full input
        J = f(mean, t, dx=True)
        xs = mean if idx is None else mean[np.asarray(idx)]
        js = orc.jacobian(fid, xs, t, p)
        assert np.allclose(J.dot(cov), ref[2], rtol=1e-12, atol=1e-300), (tag, i, J, js)
    rng = np.random.default_rng(5)
    B = 3000
    means = rng.standard_normal((B, D))
    a = rng.standard_normal((B, D, D))
    covs = np.einsum('bij,bkj->bik', a, a) + 0.2 * np.eye(D)
    times = np.arange(B, dtype=float) % 50
    mf, cf, cfx, st = tf.apply_batch(f, means, covs, times, return_status=True)
    assert not st.any()
    worst = 0.0
    for i in range(0, B, 37):
        r = orc.apply_linear(fid, means[i], covs[i], times[i], p, idx)
        for a_, b_ in zip((mf[i], cf[i], cfx[i]), r):
            worst = max(worst, rel_err(a_, b_))
    assert within(worst, 1e-12, 'k_linearize {} batch of 3000 vs oracle'.format(tag))


@pytest.mark.gpu
@pytest.mark.parametrize('tag', ['ungm', 'pend'])
def test_extended_kalman_golden(amd, golden, tag):
    """ExtendedKalman forward pass and RTS smoother (launch loop of k_linearize / k_kalman_update, smoother kernel) against the
    reference's runs (golden g13: the set-ups of its tests/test_ssinf.py)."""
    from ssmtoybox_amd import ssinf, ssmod as sm
    g = golden('g13_linear')
    y = g['ekf_' + tag + '_y']
    if tag == 'ungm':
        dyn = sm.UNGMTransition(sm.GaussRV(1), sm.GaussRV(1, cov=np.array([[10.0]])))
        obs = sm.UNGMMeasurement(sm.GaussRV(1), 1)
    else:
        dt = 0.01
        q2 = sm.GaussRV(2, cov=0.01 * np.array([[(dt ** 3) / 3, (dt ** 2) / 2], [(dt ** 2) / 2, dt]]))
        dyn = sm.Pendulum2DTransition(sm.GaussRV(2, mean=np.array([1.5, 0]), cov=0.01 * np.eye(2)), q2, dt=dt)
        obs = sm.Pendulum2DMeasurement(sm.GaussRV(1, cov=np.array([[0.1]])), 2)
    alg = ssinf.ExtendedKalman(dyn, obs)
    assert isinstance(alg.tf_dyn, amd.LinearizationTransform)
    fm, fP = alg.forward_pass_batch(y)
    assert within(rel_err(fm, g['ekf_' + tag + '_fm']), 1e-9, 'EKF {} filtered means vs the reference'.format(tag))
    assert within(rel_err(fP, g['ekf_' + tag + '_fc']), 1e-9, 'EKF {} filtered covariances vs the reference'.format(tag))
    sm_, sP = alg.backward_pass_batch()
    assert within(rel_err(sm_, g['ekf_' + tag + '_sm']), 1e-8, 'EKF {} smoothed means vs the reference'.format(tag))
    assert within(rel_err(sP, g['ekf_' + tag + '_sc']), 1e-8, 'EKF {} smoothed covariances vs the reference'.format(tag))
    # one trajectory through the drop-in call
    f1, P1 = alg.forward_pass(y[..., 0])
    assert np.array_equal(f1, fm[..., 0]) and np.array_equal(P1, fP[..., 0])


@pytest.mark.gpu
def test_extended_kalman_nonadditive_and_unsupported(amd):
    """UNGM with the noise as an input (the reference's own EKF run of this model stops in NumPy >= 1.24 on a ragged list in
    dyn_fcn_dx, so the oracle's recursion is the comparison); a model without a Jacobian fails loudly, as the reference's does."""
    from ssmtoybox_amd import ssinf, ssmod as sm, _lib as L
    dyn = sm.UNGMNATransition(sm.GaussRV(1, mean=np.array([1.0])), sm.GaussRV(1, cov=np.array([[10.0]])))
    obs = sm.UNGMNAMeasurement(sm.GaussRV(1), 1)
    x = dyn.simulate_discrete(40, 6, seed=3)
    y = obs.simulate_measurements(x, seed=4)
    alg = ssinf.ExtendedKalman(dyn, obs)
    fm, fP = alg.forward_pass_batch(y)
    one, z1 = np.eye(1), np.zeros(1)
    tf_dyn = lambda m, P, t: orc.apply_linear(orc.F_UNGMNA_DYN, m, P, t)
    tf_obs = lambda m, P, t: orc.apply_linear(orc.F_UNGMNA_MEAS, m, P, t)
    for s in range(y.shape[2]):
        rm, rP = orc.gaussian_filter_aug(y[..., s], np.ones(1), one, z1, 10.0 * one, z1, one, one, tf_dyn, tf_obs, False, False)
        assert within(rel_err(fm[..., s], rm), 1e-9, 'EKF ungmna means vs oracle')
        assert within(rel_err(fP[..., s], rP), 1e-9, 'EKF ungmna covariances vs oracle')
    rer = sm.ReentryVehicle2DTransition(sm.GaussRV(5, cov=np.eye(5)), sm.GaussRV(3, cov=np.eye(3)))
    with pytest.raises(L.SsmqError, match='no Jacobian'):
        amd.LinearizationTransform(5).apply(rer.dyn_eval, np.ones(5), np.eye(5), np.atleast_1d(0))
    with pytest.raises(NotImplementedError):
        amd.LinearizationTransform(2).apply(lambda x, p: x, np.ones(2), np.eye(2), np.atleast_1d(0))


# ---------------------------------------------------------------------------------------------------------------
# k_filter_wsplit: the time loop with the sigma points of every transform shared out over the W waves of a workgroup
# (csrc/ssmq_filter_wsplit.hip).  Default choice: the t-process form at batches that leave most of the device idle (configs[3]);
# SSMQ_FUSED_WSPLIT = 0 / 2 / 4 forces the register kernel / a wave count where one is instantiated.
# ---------------------------------------------------------------------------------------------------------------
def _wsplit_filters(seed):
    """(name, filter, measurements (Y, T, B), C-oracle transforms + arguments) for the three instantiated systems, B not a
    multiple of 64 (the idle lanes of the last workgroup take part in every barrier and store nothing)."""
    from oracle import c_oracle as co
    from bench import simulate_reentry
    from ssmtoybox_amd import ssinf, ssmod as sm
    out = []
    B, T = 200, 12
    x, y, m0, P0, Q, G, R = simulate_reentry(B, T, seed)
    dyn = sm.ReentryVehicle2DTransition(sm.GaussRV(5, m0, P0), sm.GaussRV(3, cov=Q))
    obs = sm.Radar2DMeasurement(sm.GaussRV(2, cov=R), 5)
    alg = ssinf.UnscentedKalman(dyn, obs)
    sp = lambda tf, E, ci: co.make_transform(1, tf.unit_sp.shape[0], E, tf.unit_sp, tf.wm, np.diag(tf.Wc).copy(), integrand=ci)   # noqa: E731
    out.append(('ukf reentry 5-D', alg, y, sp(alg.tf_dyn, 5, co.Integrand.make(orc.F_REENTRY2D_DYN, (0.1,))),
                sp(alg.tf_obs, 2, co.Integrand.make(orc.F_RADAR2D_MEAS, (0.0, 0.0))), m0, P0, G.dot(Q).dot(G.T), R, 2e-8, 2e-8))
    mi = np.hstack((np.zeros((5, 1)), np.eye(5), 2 * np.eye(5))).astype(int)
    alg = ssinf.BayesSardKalman(dyn, obs, np.array([[1.0] + [1.0] * 5]), np.array([[1.0, 0.9, 0.9] + [1e4] * 3]), mi, mi, 'ut')
    alg.tf_dyn.model.model_var = 2e-6 * np.eye(5)
    alg.tf_obs.model.model_var = 0 * np.eye(2)
    out.append(('bsqkf reentry 5-D', alg, y, _c_bq_transform(alg.tf_dyn, 5, co.Integrand.make(orc.F_REENTRY2D_DYN, (0.1,))),
                _c_bq_transform(alg.tf_obs, 2, co.Integrand.make(orc.F_RADAR2D_MEAS, (0.0, 0.0))), m0, P0, G.dot(Q).dot(G.T), R, 0.1, 0.1))   # (the bars of test_config3_reentry_filters_1e5: this recursion amplifies rounding by 1e13)
    x, y, m0, P0, Q, G, R = simulate_reentry(B, T, seed + 1, True)
    dyn6 = sm.ReentryVehicle2DBiasTransition(sm.GaussRV(6, m0, P0), sm.GaussRV(4, cov=Q))
    obs6 = sm.Radar2DMeasurement(sm.GaussRV(2, cov=R), 6)
    alg = ssinf.UnscentedKalman(dyn6, obs6)
    out.append(('ukf reentry 6-D', alg, y, sp(alg.tf_dyn, 6, co.Integrand.make(orc.F_REENTRY2D_BIAS_DYN, (0.1,))),
                sp(alg.tf_obs, 2, co.Integrand.make(orc.F_RADAR2D_MEAS, (0.0, 0.0))), m0, P0, G.dot(Q).dot(G.T), R, 2e-8, 2e-8))
    # configs[3]: t-process quadrature Kalman filter, coordinated turn + four bearings
    m0 = np.array([1000, 300, 1000, 0, np.deg2rad(-3.0)])
    P0 = np.diag([100, 10, 100, 10, 0.1])
    dt, r1, r2 = 0.1, 0.1, 1.75e-4
    A = np.array([[dt ** 3 / 3, dt ** 2 / 2], [dt ** 2 / 2, dt]])
    Q = np.zeros((5, 5))
    Q[:2, :2], Q[2:4, 2:4], Q[4, 4] = r1 * A, r1 * A, r2 * dt
    Rn = 10e-3 * np.eye(4)
    dync = sm.CoordinatedTurnTransition(sm.GaussRV(5, m0, P0), sm.GaussRV(5, cov=Q), dt=dt)
    obsc = sm.BearingMeasurement(sm.GaussRV(4, cov=Rn), 5, state_index=[0, 2], sensor_pos=SENSORS)
    Tc = 4
    d_x, d_y, ld = sm.simulate_dev(dync, obsc, Tc, B, seed=seed)
    yc = d_y.download((Tc, 4, ld))[:, :, :B].transpose(1, 0, 2)
    d_x.free()
    d_y.free()
    par = np.array([[1.0, 100, 100, 100, 100, 1]])
    alg = ssinf.StudentProcessKalman(dync, obsc, par, par)
    nu = float(alg.tf_dyn.model.nu)
    out.append(('tpqkf ct + bearings', alg, yc, _c_bq_transform(alg.tf_dyn, 5, co.Integrand.make(orc.F_CT_DYN, (dt,)), nu, 1),
                _c_bq_transform(alg.tf_obs, 4, co.Integrand.make(orc.F_BEARING_MEAS, tuple(SENSORS.reshape(-1)), (0, 2)), nu, 1),
                m0, P0, Q, Rn, 1e-8, 1e-7))
    return out


def test_wsplit_filters_match_oracle_and_register_kernel(amd, monkeypatch):
    """Every wave count of the wave-split time loop, and the register kernel it replaces, against the C oracle on the same
    trajectories (pre-failure steps, means in standard deviations, covariances entry-scaled) and against each other: partial sums
    re-associate, nothing else changes."""
    from oracle import c_oracle as co
    for name, alg, y, (td, k1), (to, k2), m0, P0, GQG, R, tol_m, tol_P in _wsplit_filters(51):
        T, B = y.shape[1], y.shape[2]
        cfm, cfP, cst = co.filter_forward(td, to, np.ascontiguousarray(y.transpose(2, 1, 0)), m0, P0, GQG, R, threads=8)
        cfm, cfP = cfm.transpose(2, 1, 0), cfP.transpose(2, 3, 1, 0)
        runs = {}
        for mode in ('0', '2', '4'):
            monkeypatch.setenv('SSMQ_FUSED_WSPLIT', mode)
            kn = alg.kernel_name(B)
            assert ('k_filter_wsplit' in kn and kn.endswith('W=%s>' % mode)) if mode != '0' else 'k_filter_fused<' in kn, kn
            fm, fP = alg.forward_pass_batch(y, raise_on_failure=False)
            runs[mode] = (fm.copy(), fP.copy(), alg.status.copy())
            _compare_filter_prefix(fm, fP, alg.status, cfm, cfP, cst, T, '%s, wave-split mode %s vs C oracle' % (name, mode), tol_m, tol_P)
        monkeypatch.delenv('SSMQ_FUSED_WSPLIT')
        for mode in ('2', '4'):
            assert np.array_equal(runs[mode][2], runs['0'][2]), name
            _compare_filter_prefix(runs[mode][0], runs[mode][1], runs[mode][2], runs['0'][0], runs['0'][1], runs['0'][2], T,
                                   '%s, W=%s vs the register kernel' % (name, mode), tol_m, tol_P)
        # a second call with the same mode replays nothing stale: bitwise the same
        monkeypatch.setenv('SSMQ_FUSED_WSPLIT', '2')
        fm2, fP2 = alg.forward_pass_batch(y, raise_on_failure=False)
        monkeypatch.delenv('SSMQ_FUSED_WSPLIT')
        assert np.array_equal(fm2, runs['2'][0], equal_nan=True) and np.array_equal(fP2, runs['2'][1], equal_nan=True)


def test_quad_filters_match_oracle_and_register_kernel(amd, monkeypatch):
    """k_filter_quad (csrc/ssmq_filter_quad.hip: one trajectory on the four lanes of a quad, the sigma points dealt to the lanes,
    partial sums all-reduced with DPP) against the C oracle on the same trajectories with the bars of the register kernel, against
    the register kernel itself (summation order differs: rounding, not bits), batch sizes that are not multiples of 16, failing
    trajectories at the same step, the default choice, and device-resident repeats bitwise equal."""
    from oracle import c_oracle as co
    from ssmtoybox_amd import ssinf, ssmod as sm
    if 'SSMQ_NO_FASTPATH' in os.environ or 'SSMQ_NO_FUSED' in os.environ:
        pytest.skip('k_filter_quad is offered for point sets the host verified as unscented-type (SSMQ_OPT_UT) only')
    flt = _wsplit_filters(61)
    cases = [flt[0], flt[2]]                      # UKF on the 5-D reentry model and on the 6-D variant
    # + the unscented filter on the coordinated-turn model with four bearing sensors (measurements of the t-process case)
    name, tpq, yc, _, _, m0c, P0c, Qc, Rc, _, _ = flt[3]
    ukfc = ssinf.UnscentedKalman(tpq.mod_dyn, tpq.mod_obs)
    spc = lambda tf, E, ci: co.make_transform(1, tf.unit_sp.shape[0], E, tf.unit_sp, tf.wm, np.diag(tf.Wc).copy(), integrand=ci)   # noqa: E731
    cases.append(('ukf ct + bearings', ukfc, yc, spc(ukfc.tf_dyn, 5, co.Integrand.make(orc.F_CT_DYN, (0.1,))),
                  spc(ukfc.tf_obs, 4, co.Integrand.make(orc.F_BEARING_MEAS, tuple(SENSORS.reshape(-1)), (0, 2))), m0c, P0c, Qc, Rc, 1e-8, 1e-7))
    for name, alg, y, (td, k1), (to, k2), m0, P0, GQG, R, tol_m, tol_P in cases:
        T, B = y.shape[1], y.shape[2]
        y = y[:, :, :B - 5]                       # 195 trajectories: 12 full quads-of-16 and a wave with 3 trajectories
        B = y.shape[2]
        cfm, cfP, cst = co.filter_forward(td, to, np.ascontiguousarray(y.transpose(2, 1, 0)), m0, P0, GQG, R, threads=8)
        cfm, cfP = cfm.transpose(2, 1, 0), cfP.transpose(2, 3, 1, 0)
        x0c = np.tile(P0, (B, 1, 1))
        x0c[7] = -np.eye(P0.shape[0])             # not positive definite from the start
        runs = {}
        for mode in ('0', '1'):
            monkeypatch.setenv('SSMQ_FUSED_QUAD', mode)
            kn = alg.kernel_name(B)
            assert ('k_filter_quad<' if mode == '1' else 'k_filter_fused<') in kn, kn
            fm, fP = alg.forward_pass_batch(y, raise_on_failure=False)
            runs[mode] = (fm.copy(), fP.copy(), alg.status.copy())
            _compare_filter_prefix(fm, fP, alg.status, cfm, cfP, cst, T, '%s, quad mode %s vs C oracle' % (name, mode), tol_m, tol_P)
            fmx, fPx = alg.forward_pass_batch(y, x0_cov=x0c, raise_on_failure=False)
            runs[mode + 'x'] = (fmx.copy(), fPx.copy(), alg.status.copy())
        monkeypatch.delenv('SSMQ_FUSED_QUAD')
        assert np.array_equal(runs['1'][2], runs['0'][2]), name
        _compare_filter_prefix(runs['1'][0], runs['1'][1], runs['1'][2], runs['0'][0], runs['0'][1], runs['0'][2], T,
                               '%s, quad vs the register kernel' % name, tol_m, tol_P)
        assert np.array_equal(runs['1x'][2], runs['0x'][2]) and runs['1x'][2][7] == 1 and np.isnan(runs['1x'][0][:, :, 7]).all()
        # the default for a batch this small is the quad kernel; a second pass replays nothing stale
        if 'SSMQ_FUSED_WSPLIT' not in os.environ:       # (a forced wave-split mode keeps its meaning: tools/alt_paths.sh)
            assert 'k_filter_quad<' in alg.kernel_name(B) and 'k_filter_quad<' in alg.kernel_name(12500) and 'k_filter_quad<' not in alg.kernel_name(20000)
        monkeypatch.setenv('SSMQ_FUSED_QUAD', '1')
        fm2, fP2 = alg.forward_pass_batch(y, raise_on_failure=False)
        monkeypatch.delenv('SSMQ_FUSED_QUAD')
        assert np.array_equal(fm2, runs['1'][0], equal_nan=True) and np.array_equal(fP2, runs['1'][1], equal_nan=True)


def test_quad_share_of_config3_at_full_size(amd):
    """One GPU's share of BASELINE configs[2] on an eight-GPU node: 12 500 trajectories x 50 steps of the unscented filter on the
    reentry model, device-resident - the batch k_filter_quad is the default for.  A 600-trajectory sample against the C oracle with
    the bars of the 1e5 test, every trajectory against the register kernel (rounding-level: other summation order), the route
    by name."""
    from oracle import c_oracle as co
    from benchlib.workloads import FilterBench
    if any(k in os.environ for k in ('SSMQ_NO_FASTPATH', 'SSMQ_NO_FUSED', 'SSMQ_FUSED_QUAD', 'SSMQ_FUSED_WSPLIT')):
        pytest.skip('the default route of this batch is what is tested')
    B, T = 12500, 50
    wl = FilterBench(amd, B, T, 35, 'reentry5', 'ukf')
    assert 'k_filter_quad<D=5,Y=2' in wl.kernel, wl.kernel
    wl.step()
    fm, fP, st = wl.results()
    assert not st.any()
    idx = np.random.default_rng(1).choice(B, 600, replace=False)
    pts = orc.points_ut(5)
    wm, wc = orc.weights_ut(5)
    td, k1 = co.make_transform(1, 5, 5, pts, wm, wc, integrand=co.Integrand.make(orc.F_REENTRY2D_DYN, (0.1,)))
    to, k2 = co.make_transform(1, 5, 2, pts, wm, wc, integrand=co.Integrand.make(orc.F_RADAR2D_MEAS, (0.0, 0.0)))
    GQG = wl.alg.G.dot(wl.alg.q_cov).dot(wl.alg.G.T)
    cfm, cfP, cst = co.filter_forward(td, to, np.ascontiguousarray(wl.y_host[:, :, idx].transpose(2, 1, 0)), wl.m0, wl.P0, GQG, wl.alg.r_cov, threads=8)
    assert not cst.any()
    assert within(mean_err(fm[:, :, idx], cfm.transpose(2, 1, 0)), 1e-8, 'configs[2] share, k_filter_quad fm vs oracle (row-scaled)')
    assert within(cov_err(fP[:, :, :, idx], cfP.transpose(2, 3, 1, 0)), 2e-8, 'configs[2] share, k_filter_quad fP vs oracle (entry-scaled)')
    os.environ['SSMQ_FUSED_QUAD'] = '0'
    try:
        wl.d_fm.upload(np.zeros((T, wl.D, wl.ld)))
        assert 'k_filter_fused<D=5,Y=2' in wl.alg.kernel_name(B)
        wl.step()
        rm, rP, rst = wl.results()
    finally:
        os.environ.pop('SSMQ_FUSED_QUAD')
    assert not rst.any()
    # (the bars of the oracle comparison: 50 steps of this recursion amplify a last-bit difference to ~2e-9 of a covariance entry,
    # measured 2.0e-9 over all 12 500 trajectories, whichever two implementations are compared)
    assert within(mean_err(fm, rm), 1e-8, 'configs[2] share, k_filter_quad vs k_filter_fused fm (row-scaled)')
    assert within(cov_err(fP, rP), 2e-8, 'configs[2] share, k_filter_quad vs k_filter_fused fP (entry-scaled)')
    wl.free()


def test_chunked_time_loop_is_bitwise_the_whole_pass(amd, monkeypatch):
    """k_filter_chunked (csrc/ssmq_filter_chunked.hip): the block-steps of a batch cut into equal strips, one wave per strip; a block
    that straddles two strips is begun by one wave and finished by another from the state - mean, covariance triangle, status word
    as the registers held them - handed over through memory.  The results must be the BITS of the whole-pass kernel, failures
    included, for any number of strips (SSMQ_FUSED_CHUNKED = n) and for the default choice."""
    from benchlib.workloads import FilterBench
    for wl_name, filt, B, T, modes in (('reentry5', 'ukf', 70000, 23, ('1', '100', '333', '1000')), ('reentry6', 'ukf', 9000, 12, ('7', '100', '140')),
                                       ('reentry5', 'bsqkf', 30000, 10, ('64', '400')), ('ct', 'ukf', 20000, 20, ('5', '300')),
                                       ('ct', 'tpqkf', 70000, 6, ('1', '700')), ('reentry5', 'gpqkf', 70000, 9, ('1',))):
        monkeypatch.setenv('SSMQ_FUSED_CHUNKED', '0')
        wl = FilterBench(amd, B, T, 5, wl_name, filt)
        if wl_name == 'reentry5' and filt == 'ukf':       # some trajectories that fail on the way: not-PD initial covariances
            P = np.zeros((wl.D * wl.D, wl.ld))
            P[:] = wl.P0.reshape(-1, 1)
            P[0, 100:B:977] = -1.0
            wl.d_P0.upload(P)
        wl.step()
        ref = wl.results()
        assert np.isfinite(ref[0]).any()
        for mode in modes:
            monkeypatch.setenv('SSMQ_FUSED_CHUNKED', mode)
            wl.d_fm.upload(np.zeros((T, wl.D, wl.ld)))      # (what is compared was written by this pass)
            wl.step()
            got = wl.results()
            assert all(np.array_equal(g, r, equal_nan=True) for g, r in zip(got, ref)), (wl_name, filt, mode)
        if wl_name == 'reentry5' and filt == 'ukf':
            assert (ref[2] != 0).sum() >= B // 977 - 1
            monkeypatch.delenv('SSMQ_FUSED_CHUNKED')
            assert 'k_filter_chunked<' in wl.alg.kernel_name(B)       # 1 094 blocks on 1 024 SIMDs: the default takes the strips
        wl.free()
    monkeypatch.delenv('SSMQ_FUSED_CHUNKED', raising=False)


def _ungm_study_filters(ssinf, sm, with_loop=False):
    dyn = sm.UNGMTransition(sm.GaussRV(1), sm.GaussRV(1, cov=np.array([[10.0]])))
    obs = sm.UNGMMeasurement(sm.GaussRV(1), 1)
    par = np.array([[1.0, 3.0]])
    mi = np.array([[0, 1, 2]])
    algs = [ssinf.UnscentedKalman(dyn, obs), ssinf.CubatureKalman(dyn, obs), ssinf.GaussHermiteKalman(dyn, obs, deg=5),
            ssinf.GaussianProcessKalman(dyn, obs, par, par, 'rbf', 'ut'), ssinf.StudentProcessKalman(dyn, obs, par, par, 'rbf', 'ut'),
            ssinf.BayesSardKalman(dyn, obs, par, par, mi, mi, 'ut')]
    if with_loop:
        algs.append(ssinf.GaussHermiteKalman(dyn, obs, deg=7))         # 7 points: no fused kernel, the launch loop after the graph
    return algs


def test_run_filters_is_the_serial_calls_bit_for_bit(amd, monkeypatch):
    """ssinf.run_filters / ssmq_filter_forward_multi_dev: the six filters of the reference's UNGM studies (research/bsq/bsq_ungm.py:
    132-137, research/tpq/tpq_base.py:175-192) over the same measurements as ONE launch graph - one branch per filter, each the
    filter's own fused kernel - must give exactly what the filters give one after the other; also with a filter that has no
    fused kernel in the list, with a Studentian filter, with filters of another model in the same call, on a replayed graph,
    and without the graph (SSMQ_MULTI_NO_GRAPH)."""
    from ssmtoybox_amd import ssinf, ssmod as sm
    from bench import simulate_ungm
    B, T = 3000, 40
    _, y = simulate_ungm(B, T, 77)
    y = np.ascontiguousarray(y[None])
    serial = [a.forward_pass_batch(y, raise_on_failure=False) + (a.status.copy(),) for a in _ungm_study_filters(ssinf, sm, True)]
    # the six filters of one model family: ONE kernel (k_filter_multi_ungm), first call and repeated call; then the same six as
    # a forked graph (SSMQ_MULTI_NO_FAMILY)
    for mode in ('family', 'family again', 'graph of six'):
        if mode == 'graph of six':
            monkeypatch.setenv('SSMQ_MULTI_NO_FAMILY', '1')
        algs = _ungm_study_filters(ssinf, sm) if mode != 'family again' else algs
        got = ssinf.run_filters(algs, y, raise_on_failure=False)
        for i, (a, g, s) in enumerate(zip(algs, got, serial)):
            assert np.array_equal(g[0], s[0], equal_nan=True) and np.array_equal(g[1], s[1], equal_nan=True), (mode, i, type(a).__name__)
            assert np.array_equal(a.status, s[2])
    monkeypatch.delenv('SSMQ_MULTI_NO_FAMILY')
    for mode in ('graph', 'replay', 'nograph'):
        if mode == 'nograph':
            monkeypatch.setenv('SSMQ_MULTI_NO_GRAPH', '1')
        algs = _ungm_study_filters(ssinf, sm, True) if mode != 'replay' else algs
        assert 'k_filter_fused' in algs[0].kernel_name() and 'hipGraph' in algs[-1].kernel_name()
        got = ssinf.run_filters(algs, y, raise_on_failure=False)
        for i, (a, g, s) in enumerate(zip(algs, got, serial)):
            assert np.array_equal(g[0], s[0], equal_nan=True) and np.array_equal(g[1], s[1], equal_nan=True), (mode, i, type(a).__name__)
            assert np.array_equal(a.status, s[2]) and a.fi_mean is g[0]
    monkeypatch.delenv('SSMQ_MULTI_NO_GRAPH')
    # a Studentian filter and filters of a 5-D model in the same launch as scalar ones is not possible (other measurements), but
    # filters of different kinds over the reentry measurements are: UKF, CKF, Bayes-Sard on the 5-D model
    from bench import simulate_reentry
    Br, Tr = 2500, 12
    x5, y5, m5, P5, Q5, G5, R5 = simulate_reentry(Br, Tr, 5, False)
    dyn5 = sm.ReentryVehicle2DTransition(sm.GaussRV(5, m5, P5), sm.GaussRV(3, cov=Q5))
    obs5 = sm.Radar2DMeasurement(sm.GaussRV(2, cov=R5), 5)
    mi = np.hstack((np.zeros((5, 1)), np.eye(5), 2 * np.eye(5))).astype(int)

    def make5():
        b = ssinf.BayesSardKalman(dyn5, obs5, np.array([[1.0, 1, 1, 1, 1, 1]]), np.array([[1.0, 0.9, 0.9, 1e4, 1e4, 1e4]]), mi, mi, 'ut')
        b.tf_dyn.model.model_var = 2e-6 * np.eye(5)
        b.tf_obs.model.model_var = 0 * np.eye(2)
        return [ssinf.UnscentedKalman(dyn5, obs5), ssinf.CubatureKalman(dyn5, obs5), b]
    had_quad = os.environ.get('SSMQ_FUSED_QUAD')
    monkeypatch.setenv('SSMQ_FUSED_QUAD', '0')          # (the jobs of a multi-launch are whole-pass kernels; so is the serial reference)
    serial = [a.forward_pass_batch(y5, raise_on_failure=False) for a in make5()]
    if had_quad is None:
        monkeypatch.delenv('SSMQ_FUSED_QUAD')
    else:
        monkeypatch.setenv('SSMQ_FUSED_QUAD', had_quad)
    got = ssinf.run_filters(make5(), y5, raise_on_failure=False)
    for g, s in zip(got, serial):
        assert np.array_equal(g[0], s[0], equal_nan=True) and np.array_equal(g[1], s[1], equal_nan=True)
    # Studentian recursion as a job beside a Gaussian one (UNGM; ssmq_student_filter_forward_dev's arguments through `scale` / `dof`)
    dynS = sm.UNGMTransition(sm.StudentRV(1), sm.StudentRV(1, scale=np.array([[10.0]])))
    obsS = sm.UNGMMeasurement(sm.StudentRV(1), 1)
    dynG = sm.UNGMTransition(sm.GaussRV(1), sm.GaussRV(1, cov=np.array([[10.0]])))
    obsG = sm.UNGMMeasurement(sm.GaussRV(1), 1)
    ys = y
    mk = lambda: [ssinf.FullySymmetricStudent(dynS, obsS), ssinf.UnscentedKalman(dynG, obsG)]
    serial = [a.forward_pass_batch(ys, raise_on_failure=False) for a in mk()]
    got = ssinf.run_filters(mk(), ys, raise_on_failure=False)
    for g, s in zip(got, serial):
        assert np.array_equal(g[0], s[0], equal_nan=True) and np.array_equal(g[1], s[1], equal_nan=True)
    # argument errors: two jobs with one output buffer
    from ssmtoybox_amd import _lib
    lib = _lib.load()
    jobs = (_lib.FilterJob * 2)()
    assert lib.ssmq_filter_forward_multi_dev(2, jobs) == -1 and lib.ssmq_filter_forward_multi_dev(0, None) == 0


def test_piped_forward_pass_is_the_plain_one_bit_for_bit(amd, monkeypatch):
    """forward_pass_batch with its transfers overlapped (ssmq_filter_forward_piped: K launches of k_filter_range over consecutive
    time blocks, copies on their own streams) against the upload / whole pass / download path (SSMQ_NO_PIPED=1): same bits - for the
    headline filter, for a failing trajectory, for per-trajectory initial moments, for every block count, for pageable and for
    page-locked result arrays, and for a 5-D filter; the returned arrays are ordinary writable ndarrays."""
    from ssmtoybox_amd import ssinf, ssmod as sm, _lib
    from bench import simulate_ungm, simulate_reentry
    lib = _lib.load()
    # tools/alt_paths.sh runs the suite with routes forced through the environment: a forced route is not pipelined
    piped = 0 if any(k in os.environ for k in ('SSMQ_NO_FUSED', 'SSMQ_FUSED_WSPLIT', 'SSMQ_FUSED_QUAD', 'SSMQ_FUSED_CHUNKED', 'SSMQ_FUSED_LPW')) else 1
    B, T = 5000, 37
    _, y = simulate_ungm(B, T, 3)
    y = np.ascontiguousarray(y[None])
    dyn = sm.UNGMTransition(sm.GaussRV(1), sm.GaussRV(1, cov=np.array([[10.0]])))
    obs = sm.UNGMMeasurement(sm.GaussRV(1), 1)
    par = np.array([[1.0, 3.0]])
    rng = np.random.default_rng(0)
    x0m = rng.standard_normal((B, 1))
    x0c = 0.5 + rng.random((B, 1, 1))
    x0c[17, 0, 0] = -1.0                                           # one trajectory that fails at the first factorisation
    for make in (lambda: ssinf.GaussianProcessKalman(dyn, obs, par, par, 'rbf', 'ut'), lambda: ssinf.UnscentedKalman(dyn, obs),
                 lambda: ssinf.CubatureKalman(dyn, obs)):
        monkeypatch.setenv('SSMQ_NO_PIPED', '1')
        a0 = make()
        ref = a0.forward_pass_batch(y)
        ref_x = a0.forward_pass_batch(y, x0m, x0c, raise_on_failure=False) + (a0.status.copy(),)
        monkeypatch.delenv('SSMQ_NO_PIPED')
        a1 = make()
        got = a1.forward_pass_batch(y)
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]) and not a1.status.any()
        assert lib.ssmq_pinned_is_block(ctypes.c_void_p(got[0].ctypes.data)) == piped      # (the pipelined route was taken)
        got[0][0, 0, 0] += 1.0                                      # writable, the caller's own (ssinf.py:279 mutates its results)
        got_x = a1.forward_pass_batch(y, x0m, x0c, raise_on_failure=False)
        assert np.array_equal(got_x[0], ref_x[0], equal_nan=True) and np.array_equal(got_x[1], ref_x[1], equal_nan=True)
        assert np.array_equal(a1.status, ref_x[2]) and a1.status[17] == 1
        with pytest.raises(np.linalg.LinAlgError):
            a1.forward_pass_batch(y, x0m, x0c)
    # the C entry point: every block count, pageable outputs
    alg = ssinf.GaussianProcessKalman(dyn, obs, par, par, 'rbf', 'ut')
    monkeypatch.setenv('SSMQ_NO_PIPED', '1')
    ref = alg.forward_pass_batch(y)
    monkeypatch.delenv('SSMQ_NO_PIPED')
    from ssmtoybox_amd.mtran import resolve_integrand
    f_dyn, e_dyn = resolve_integrand(dyn.dyn_eval)
    f_obs, e_obs = resolve_integrand(obs.meas_eval)
    dp = lambda a: a.ctypes.data_as(_lib.c_double_p)            # noqa: E731
    for K in (1, 2, 5, 36, 37, 64):
        fm, fP, st = np.full((1, T, B), np.nan), np.full((1, 1, T, B), np.nan), np.full(B, -7, dtype=np.int32)
        rc = lib.ssmq_filter_forward_piped(ctypes.c_void_p(alg.tf_dyn._handle_for(e_dyn)), ctypes.byref(f_dyn),
                                           ctypes.c_void_p(alg.tf_obs._handle_for(e_obs)), ctypes.byref(f_obs), B, T, dp(y), dp(np.zeros(1)),
                                           dp(np.ones((1, 1))), dp(np.array([[10.0]])), dp(np.ones((1, 1))), ctypes.c_void_p(fm.ctypes.data),
                                           ctypes.c_void_p(fP.ctypes.data), ctypes.c_void_p(st.ctypes.data), 0, K)
        if not piped:
            assert rc == -3
            continue
        assert rc == 0 and np.array_equal(fm, ref[0]) and np.array_equal(fP, ref[1]) and not st.any(), K
    # a 5-D filter (42 strided copies per block) and a shape without a time-block kernel (falls back, same call)
    Br, Tr = 3000, 20
    x5, y5, m5, P5, Q5, G5, R5 = simulate_reentry(Br, Tr, 8, False)
    dyn5 = sm.ReentryVehicle2DTransition(sm.GaussRV(5, m5, P5), sm.GaussRV(3, cov=Q5))
    obs5 = sm.Radar2DMeasurement(sm.GaussRV(2, cov=R5), 5)
    had_quad = os.environ.get('SSMQ_FUSED_QUAD')
    monkeypatch.setenv('SSMQ_NO_PIPED', '1')
    monkeypatch.setenv('SSMQ_FUSED_QUAD', '0')          # (device-resident batches this small take k_filter_quad: rounding-level differences)
    ref = ssinf.UnscentedKalman(dyn5, obs5).forward_pass_batch(y5)
    refg = ssinf.GaussHermiteKalman(dyn, obs, deg=7).forward_pass_batch(y)
    monkeypatch.delenv('SSMQ_NO_PIPED')
    if had_quad is None:
        monkeypatch.delenv('SSMQ_FUSED_QUAD')
    else:
        monkeypatch.setenv('SSMQ_FUSED_QUAD', had_quad)
    got = ssinf.UnscentedKalman(dyn5, obs5).forward_pass_batch(y5)
    if piped:
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])
    assert lib.ssmq_pinned_is_block(ctypes.c_void_p(got[0].ctypes.data)) == piped
    gotg = ssinf.GaussHermiteKalman(dyn, obs, deg=7).forward_pass_batch(y)
    assert np.array_equal(gotg[0], refg[0]) and lib.ssmq_pinned_is_block(ctypes.c_void_p(gotg[0].ctypes.data)) == 0


def test_chunked_many_small_strips_across_xcds(amd, monkeypatch):
    """Stress of the strip hand-over's ordering (csrc/ssmq_filter_chunked.hip, "Ordering"): strip counts just below the block count
    make nearly every wave both publish a state and consume one, on compute units of different XCDs, hundreds of hand-overs per
    launch and thousands over the repetitions; a stale or torn state would change bits of the filtered moments.  Every pass must
    be the whole-pass kernel's bits."""
    from benchlib.workloads import FilterBench
    B, T = 70000, 16           # 1 094 blocks
    monkeypatch.setenv('SSMQ_FUSED_CHUNKED', '0')
    wl = FilterBench(amd, B, T, 21, 'reentry5', 'ukf')
    wl.step()
    ref = wl.results()
    for strips in ('1093', '1000', '777', '547'):
        monkeypatch.setenv('SSMQ_FUSED_CHUNKED', strips)
        assert 'k_filter_chunked<' in wl.alg.kernel_name(B)
        for rep in range(12):
            wl.d_fm.upload(np.zeros((T, wl.D, wl.ld)))
            wl.step()
            got = wl.results()
            assert all(np.array_equal(g, r, equal_nan=True) for g, r in zip(got, ref)), (strips, rep)
    wl.free()
    monkeypatch.delenv('SSMQ_FUSED_CHUNKED', raising=False)


def test_strip_kernels_from_several_threads_at_once(amd, monkeypatch):
    """Three threads launch k_filter_chunked (1 024 strips each) at the same time on their own streams: the strips of the launches
    compete for the chip's wave slots, so part of every grid starts late - a strip may only ever wait for a strip whose index was
    taken before its own.  Results: the whole-pass kernel's bits, for every thread and repetition."""
    import threading
    from benchlib.workloads import FilterBench
    B, T = 70000, 12
    monkeypatch.setenv('SSMQ_FUSED_CHUNKED', '0')
    ref_wl = FilterBench(amd, B, T, 9, 'reentry5', 'ukf')
    ref_wl.step()
    ref = ref_wl.results()
    ref_wl.free()
    monkeypatch.delenv('SSMQ_FUSED_CHUNKED')
    results, errors = {}, []

    def work(i):
        try:
            wl = FilterBench(amd, B, T, 9, 'reentry5', 'ukf')          # (same seed: same data as the reference run)
            assert 'k_filter_chunked<' in wl.alg.kernel_name(B)
            for _ in range(30):
                wl.step()
            results[i] = wl.results()
            wl.free()
        except Exception as e:        # noqa: BLE001
            errors.append((i, repr(e)))
    threads = [threading.Thread(target=work, args=(i,)) for i in range(3)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(300)
    assert not errors, errors
    for i in range(3):
        assert all(np.array_equal(g, r, equal_nan=True) for g, r in zip(results[i], ref)), i


def test_wsplit_default_choice_and_failures(amd, monkeypatch):
    """What is picked without the switch: the wave-split loop for the t-process form while the batch leaves SIMDs idle, the
    register kernel for saturated batches and for every other form (measured slower there: profiles/r05_wsplit.txt).  A
    trajectory whose covariance is not positive definite fails at the same step in both kernels and is NaN from there on."""
    monkeypatch.delenv('SSMQ_FUSED_WSPLIT', raising=False)
    flt = _wsplit_filters(52)
    ukf, tpq = flt[0][1], flt[3][1]
    # (the wave split is not for the unscented reentry filter; at 1e5 trajectories - 1 563 blocks on 1 024 SIMDs - the five- and
    # six-state time loops run as equal strips of block-steps, csrc/ssmq_filter_chunked.hip, below the SIMD count as whole passes)
    # (... and below 16 384 trajectories - every whole-pass wave alone on a SIMD - with a trajectory on four lanes, ssmq_filter_quad.hip)
    if 'SSMQ_FUSED_QUAD' not in os.environ and 'SSMQ_NO_FASTPATH' not in os.environ:      # (the quad kernel needs the verified unscented point set)
        assert 'k_filter_quad<' in ukf.kernel_name(200) and 'k_filter_quad<' in ukf.kernel_name(12500)
        assert 'SSMQ_FUSED_CHUNKED' in os.environ or 'k_filter_fused<' in ukf.kernel_name(20000)
    assert 'SSMQ_FUSED_CHUNKED' in os.environ or 'k_filter_fused<' in ukf.kernel_name(60000)
    if 'SSMQ_FUSED_CHUNKED' not in os.environ:           # (tools/alt_paths.sh runs the suite with the choice forced either way)
        assert 'k_filter_chunked<' in ukf.kernel_name(100000)
    assert 'k_filter_wsplit' in tpq.kernel_name(10000) and 'W=2>' in tpq.kernel_name(10000)
    assert 'k_filter_fused<' in tpq.kernel_name() and ('SSMQ_FUSED_CHUNKED' in os.environ or 'k_filter_chunked<' in tpq.kernel_name(100000))
    name, alg, y, _, _, m0, P0, GQG, R, _, _ = flt[3]
    B = y.shape[2]
    x0c = np.tile(P0, (B, 1, 1))
    x0c[3] = -np.eye(5)                  # not positive definite from the start
    x0c[70, 0, 0] = np.nan
    res = {}
    for mode in ('0', '2', '4'):
        monkeypatch.setenv('SSMQ_FUSED_WSPLIT', mode)
        fm, fP = alg.forward_pass_batch(y, x0_mean=np.tile(m0, (B, 1)), x0_cov=x0c, raise_on_failure=False)
        res[mode] = (fm.copy(), alg.status.copy())
        assert alg.status[3] == 1 and alg.status[70] == 1 and np.all(np.isnan(fm[:, :, 3])) and np.all(np.isnan(fP[:, :, :, 70]))
        assert np.all(np.isfinite(fm[:, :, alg.status == 0]))
    monkeypatch.delenv('SSMQ_FUSED_WSPLIT')
    assert np.array_equal(res['0'][1], res['2'][1]) and np.array_equal(res['0'][1], res['4'][1])


def test_marginal_filter_device_rounds_match_host_rounds(amd, monkeypatch):
    """The batched marginalised filter with its state machines on the device (round 5: pack | theta step | advance, five launches
    per round and no host turn) against round 4's host rounds of the SAME optimiser code (csrc/ssmq_bfgs.h) and the SAME theta
    kernels: what differs is exp / log of the device's math library against glibc's in the packing of the kernel parameters and
    the log prior - last-bit differences that the forward-difference gradients of BFGS amplify exactly as they amplify the
    difference between two summation orders (tests/test_bfgs_lockstep.py)."""
    from ssmtoybox_amd import ssinf, ssmod as sm
    from bench import simulate_ungm
    dyn = sm.UNGMTransition(sm.GaussRV(1), sm.GaussRV(1, cov=np.array([[10.0]])))
    obs = sm.UNGMMeasurement(sm.GaussRV(1), 1)
    alg = ssinf.MarginalizedGaussianProcessKalman(dyn, obs, 'rbf', 'sr')
    B, T = 200, 6
    _, y = simulate_ungm(B, T, 21)
    data = np.ascontiguousarray(y[None])
    monkeypatch.delenv('SSMQ_MARGINAL_HOST_ROUNDS', raising=False)
    fd, Pd = alg.forward_pass_batch(data)
    sd, bd = dict(alg.batch_stats), alg.batch_failed.copy()
    fd2, Pd2 = alg.forward_pass_batch(data)
    assert np.array_equal(fd, fd2, equal_nan=True) and np.array_equal(Pd, Pd2, equal_nan=True)       # deterministic
    monkeypatch.setenv('SSMQ_MARGINAL_HOST_ROUNDS', '1')
    fh, Ph = alg.forward_pass_batch(data)
    sh, bh = dict(alg.batch_stats), alg.batch_failed.copy()
    monkeypatch.delenv('SSMQ_MARGINAL_HOST_ROUNDS')
    both = (bd == 0) & (bh == 0)
    assert both.sum() >= B - 4
    em = np.abs(fd - fh)[..., both] / np.maximum(1.0, np.abs(fh[..., both]))
    eP = np.abs(Pd - Ph)[..., both] / np.maximum(1.0, np.abs(Ph[..., both]))
    print('marginal filter, device rounds vs host rounds: means median %.2e p90 %.2e; cov median %.2e; rounds %d / %d' % (
        np.median(em), np.quantile(em, 0.9), np.median(eP), sd['rounds'], sh['rounds']))
    assert within(np.median(em[:, 0]), 2e-4, 'marginal filter device rounds vs host rounds, first step, means (median)')
    assert within(np.median(em), 2e-3, 'marginal filter device rounds vs host rounds, means (median)')
    assert within(np.median(eP), 2e-3, 'marginal filter device rounds vs host rounds, covariances (median)')
    # same optimiser: the same amount of work to within the noise of its paths
    assert 0.7 < sd['iterations'] / sh['iterations'] < 1.4 and 0.7 < sd['items'] / sh['items'] < 1.4
    # non-additive dynamics (P = 5: UNGM with its noise as an argument) run the device rounds as well
    dyn_na = sm.UNGMNATransition(sm.GaussRV(1), sm.GaussRV(1, cov=np.array([[10.0]])))
    alg_na = ssinf.MarginalizedGaussianProcessKalman(dyn_na, obs, 'rbf', 'sr')
    fna, Pna = alg_na.forward_pass_batch(data[:, :3, :32])
    sna = dict(alg_na.batch_stats)
    monkeypatch.setenv('SSMQ_MARGINAL_HOST_ROUNDS', '1')
    fnh, Pnh = alg_na.forward_pass_batch(data[:, :3, :32])
    monkeypatch.delenv('SSMQ_MARGINAL_HOST_ROUNDS')
    okn = np.isfinite(fna).all(axis=(0, 1)) & np.isfinite(fnh).all(axis=(0, 1))
    assert okn.sum() >= 28 and sna['rounds'] > 0
    assert np.median(np.abs(fna - fnh)[..., okn] / np.maximum(1.0, np.abs(fnh[..., okn]))) < 5e-3


def test_marginal_filter_host_rounds_threads_do_not_change_results(amd, monkeypatch):
    """The host rounds cut a round with many active trajectories into chunks for a pool of worker threads (Workers in
    csrc/ssmq_marginal.hip; SSMQ_MARGINAL_THREADS), every thread running the shared state machine of csrc/ssmq_marginal_traj.h
    on its own trajectories: one thread and the pool give the same bits.  B = 512 is the smallest batch at which the pool gets a
    second thread (B / 256) and a round passes its threshold of 256 active trajectories."""
    from ssmtoybox_amd import ssinf, ssmod as sm
    from bench import simulate_ungm
    dyn = sm.UNGMTransition(sm.GaussRV(1), sm.GaussRV(1, cov=np.array([[10.0]])))
    obs = sm.UNGMMeasurement(sm.GaussRV(1), 1)
    alg = ssinf.MarginalizedGaussianProcessKalman(dyn, obs, 'rbf', 'sr')
    B, T = 512, 2
    _, y = simulate_ungm(B, T, 21)
    data = np.ascontiguousarray(y[None])
    monkeypatch.setenv('SSMQ_MARGINAL_HOST_ROUNDS', '1')
    res = []
    for threads in ('1', None):
        if threads is None:
            monkeypatch.delenv('SSMQ_MARGINAL_THREADS', raising=False)
        else:
            monkeypatch.setenv('SSMQ_MARGINAL_THREADS', threads)
        fm, fP = alg.forward_pass_batch(data)
        res.append((fm.copy(), fP.copy(), alg.batch_failed.copy(), alg.batch_param_mean.copy(), dict(alg.batch_stats)))
    monkeypatch.delenv('SSMQ_MARGINAL_HOST_ROUNDS')
    one, pool = res
    print('marginal filter host rounds, one thread %s | pool %s | failed %d / %d' % (
        one[4], pool[4], int((one[2] != 0).sum()), int((pool[2] != 0).sum())))
    assert np.array_equal(one[0], pool[0], equal_nan=True) and np.array_equal(one[1], pool[1], equal_nan=True)
    assert np.array_equal(one[2], pool[2]) and np.array_equal(one[3], pool[3], equal_nan=True)
    assert one[4] == pool[4]
    assert (one[2] == 0).sum() >= B - 8 and (pool[2] == 0).sum() >= B - 8


def test_marginal_filter_one_launch_matches_device_rounds(amd, monkeypatch):
    """The one-launch route of the batched marginalised filter (k_mg_persistent: a group of lanes per trajectory loops over
    evaluate | advance inside one kernel) against the device rounds (fill | k_theta_item | advance, three launches per round): the
    same device functions on the same values in the same order - the results are EQUAL, failures and BFGS iteration counts
    included.  UNGM (P = 4), UNGM with its noise as an argument (P = 5) and the pendulum (P = 6)."""
    from ssmtoybox_amd import ssinf, ssmod as sm
    from bench import simulate_ungm
    obs = sm.UNGMMeasurement(sm.GaussRV(1), 1)
    _, y = simulate_ungm(203, 6, 21)
    cases = [
        ('ungm', ssinf.MarginalizedGaussianProcessKalman(
            sm.UNGMTransition(sm.GaussRV(1), sm.GaussRV(1, cov=np.array([[10.0]]))), obs, 'rbf', 'sr'), np.ascontiguousarray(y[None])),
        ('ungm-na', ssinf.MarginalizedGaussianProcessKalman(
            sm.UNGMNATransition(sm.GaussRV(1), sm.GaussRV(1, cov=np.array([[10.0]]))), obs, 'rbf', 'ut'),
         np.ascontiguousarray(y[None, :3, :37])),
    ]
    x0 = sm.GaussRV(2, mean=np.array([1.5, 0.0]), cov=0.01 * np.eye(2))
    pdyn = sm.Pendulum2DTransition(x0, sm.GaussRV(2, cov=np.diag([1e-4, 1e-3])), 0.05)
    pobs = sm.Pendulum2DMeasurement(sm.GaussRV(1, cov=np.array([[0.1]])), 2)
    rng = np.random.default_rng(3)
    xs = np.empty((2, 4, 24))
    x = x0.mean[:, None] + 0.1 * rng.standard_normal((2, 24))
    for k in range(4):
        x = np.stack([x[0] + 0.05 * x[1], x[1] - 9.81 * 0.05 * np.sin(x[0])]) + np.sqrt([[1e-4], [1e-3]]) * rng.standard_normal((2, 24))
        xs[:, k] = x
    yp = np.sin(xs[:1]) + np.sqrt(0.1) * rng.standard_normal((1, 4, 24))
    cases.append(('pendulum', ssinf.MarginalizedGaussianProcessKalman(pdyn, pobs, 'rbf', 'sr'), np.ascontiguousarray(yp)))
    for name, alg, data in cases:
        monkeypatch.delenv('SSMQ_MARGINAL_ROUNDS', raising=False)
        f1, P1 = alg.forward_pass_batch(data)
        s1, b1, th1 = dict(alg.batch_stats), alg.batch_failed.copy(), alg.batch_param_mean.copy()
        monkeypatch.setenv('SSMQ_MARGINAL_ROUNDS', '1')
        f2, P2 = alg.forward_pass_batch(data)
        s2, b2, th2 = dict(alg.batch_stats), alg.batch_failed.copy(), alg.batch_param_mean.copy()
        monkeypatch.delenv('SSMQ_MARGINAL_ROUNDS')
        print('marginal filter %s: one launch %s | rounds %s | failed %d' % (name, s1, s2, int((b1 != 0).sum())))
        assert np.isfinite(f1).any()
        assert np.array_equal(b1, b2), name
        assert np.array_equal(f1, f2, equal_nan=True) and np.array_equal(P1, P2, equal_nan=True), name
        assert np.array_equal(th1, th2, equal_nan=True), name
        assert s1['iterations'] == s2['iterations'] and s1['items'] == s2['items'], name
        assert 0 < s1['rounds'] <= s2['rounds'], name          # the longest wave's loop count against the batch's rounds


def test_marginal_filter_failures_are_the_reference_s_linalg_errors(amd, golden):
    """The few trajectories of a batch that the marginalised filter reports as failed (bench.py: 2-3 of 1 024 on the UNGM batch).

    What happens in them, shown here on the bench's own batch: BFGS ends the Laplace step on a nearly flat objective with an
    inverse Hessian that has an eigenvalue of 20 ... 1e8 (rho = 1 / (y's) of its last updates, y the difference of two
    forward-difference gradients); the parameter sigma points mean +- chol(cov) u (ssinf.py:1103-1106) then lie ten to
    thousands of units away in LOG-parameter space, exp() gives kernel scales of 1e6 or overflows, and the kernel matrix of those points is not a matrix any
    factorisation accepts - where the reference's _state_posterior_moments raises out of forward_pass (numpy.linalg.LinAlgError
    / scipy's finite check), the batch parks the trajectory (`batch_failed`, reason 4: include/ssmq.h) and goes on.
    WHICH trajectories end so depends on the path the optimiser takes through the noise of its gradients: the reference itself
    completes every one of these sequences (tests/golden/g14_marginal_failures.npz, made by running the reference on them), the
    build's device rounds and host rounds fail on different ones (one in common in round 5's run), at the same rate."""
    from ssmtoybox_amd import ssinf, ssmod as sm
    from bench import simulate_ungm
    g = golden('g14_marginal_failures')
    assert not g['raised'].any()                            # the reference completes all ten sequences (CPU test: test_oracle_golden)
    dyn = sm.UNGMTransition(sm.GaussRV(1), sm.GaussRV(1, cov=np.array([[10.0]])))
    obs = sm.UNGMMeasurement(sm.GaussRV(1), 1)
    alg = ssinf.MarginalizedGaussianProcessKalman(dyn, obs, 'rbf', 'sr')
    B, T = 1024, 10
    _, y = simulate_ungm(B, T, 5)
    assert np.array_equal(y[:, g['idx']], g['y'])           # the fixture's sequences are this batch's
    fm, fP = alg.forward_pass_batch(np.ascontiguousarray(y[None]))
    failed, reason = alg.batch_failed, alg.batch_failed_reason
    idx = np.flatnonzero(failed)
    print('failed trajectories', idx.tolist(), 'at steps', failed[idx].tolist(), 'reasons', reason[idx].tolist())
    assert 1 <= idx.size <= 8                               # what is measured: 6 of 1 024 on this batch in every run since round 5 (bench.py: legs.marginal_failed)
    for b in idx:
        k = int(failed[b])
        assert np.all(np.isfinite(fm[:, :k - 1, b])) and np.all(np.isnan(fm[:, k - 1:, b]))
        assert reason[b] in (3, 4, 5)                       # the Laplace covariance, or what its sigma points lead to
        cov = alg.batch_param_cov[b]
        eig = np.linalg.eigvalsh(0.5 * (cov + cov.T))
        if reason[b] == 3:
            assert eig.min() <= 0 or not np.all(np.isfinite(cov))
            continue
        # reasons 4 / 5: the Laplace covariance is positive definite, and wide in one direction (eigenvalues of 20 ... 1e8) - or the
        # parameters themselves have run away over the previous steps (a filter that has diverged: state variances of 1e30) ...
        assert eig.min() > 0, (b, eig)
        pts = alg.batch_param_mean[b][:, None] + np.linalg.cholesky(cov).dot(alg.param_upts)
        # ... so that at least one sigma point's kernel parameters exp(theta) are out of the range of a usable kernel: a scale or
        # length-scale beyond e^8 (the model variance alpha^2 (1 - tr(Q K^-1)) is then a difference of numbers of 1e7 and more) up to
        # values whose exponential is not a double at all
        assert np.abs(pts).max() > 8.0, (b, np.abs(pts).max())
    # the sequences the reference was run on: where the build completes them too, it agrees with the reference as the serial path
    # does with the golden pass (test_marginal_filter_forward_pass: 1e-4 at the first step, BFGS noise later)
    # (first step: the Laplace step from the common prior; later steps inherit what BFGS's noise did to the parameter posterior)
    first, rest = [], []
    for i, b in enumerate(g['idx']):
        if failed[b]:
            continue
        e = np.abs(fm[0, :, b] - g['fm'][i]) / np.maximum(1.0, np.abs(g['fm'][i]))
        first.append(e[0])
        rest.append(np.median(e))
    assert len(first) >= 7 and np.median(first) < 2e-4 and max(first) < 5e-2 and np.median(rest) < 5e-2, (first, rest)


def test_theta_item_route_matches_two_launch_route(amd, monkeypatch):
    """k_theta_item (round 5: one lane per parameter item, weights + both transforms + update + log-likelihood in registers, for the
    marginalised filter's small systems) against the two-launch route it replaces (k_theta_weights + k_theta_chain), item by item:
    same operations in the same order - posterior moments and flags bit for bit, the log-likelihood to the last bit or two (one
    a + b c of its final expression contracts differently)."""
    if os.environ.get('SSMQ_NO_WAVE') or os.environ.get('SSMQ_NO_THETA_FUSED'):
        pytest.skip('the two-launch route is switched off: the stage route sums in another order (tools/alt_paths.sh)')
    from ssmtoybox_amd import ssinf, ssmod as sm
    rng = np.random.default_rng(3)
    q10 = sm.GaussRV(1, cov=np.array([[10.0]]))
    pend = lambda: sm.Pendulum2DTransition(sm.GaussRV(2, mean=np.array([1.5, 0.0]), cov=0.01 * np.eye(2)), sm.GaussRV(2, cov=0.01 * np.eye(2)), 0.01)   # noqa: E731
    systems = [(sm.UNGMTransition(sm.GaussRV(1), q10), sm.UNGMMeasurement(sm.GaussRV(1), 1), 'sr'),
               (sm.UNGMTransition(sm.GaussRV(1), q10), sm.UNGMMeasurement(sm.GaussRV(1), 1), 'ut'),
               (sm.UNGMNATransition(sm.GaussRV(1), q10), sm.UNGMMeasurement(sm.GaussRV(1), 1), 'sr'),
               (sm.UNGMNATransition(sm.GaussRV(1), q10), sm.UNGMMeasurement(sm.GaussRV(1), 1), 'ut'),
               (pend(), sm.Pendulum2DMeasurement(sm.GaussRV(1, cov=np.array([[0.1]])), 2), 'sr'),
               (pend(), sm.Pendulum2DMeasurement(sm.GaussRV(1, cov=np.array([[0.1]])), 2), 'ut')]
    for dyn, obs, pts in systems:
        alg = ssinf.MarginalizedGaussianProcessKalman(dyn, obs, 'rbf', pts)
        D, n = dyn.dim_state, 777
        theta = 0.8 * rng.standard_normal((n, alg.param_dim))
        theta[::7] *= 6.0                                       # far out: flagged items, NaN outputs
        m = rng.standard_normal((n, D)) * 2.0
        a = rng.standard_normal((n, D, D))
        P = np.einsum('nij,nkj->nik', a, a) + 0.3 * np.eye(D)
        P[5] = -np.eye(D)                                       # a state covariance that is not positive definite
        y = rng.standard_normal((n, obs.dim_out))
        monkeypatch.delenv('SSMQ_NO_THETA_ITEM', raising=False)
        m1, c1, l1, s1 = alg.theta_step(theta, m, P, y, 3)
        shared = alg.theta_step(theta[:9], m[0], P[0], y[0], 3)          # state and measurement shared by the items
        monkeypatch.setenv('SSMQ_NO_THETA_ITEM', '1')
        m2, c2, l2, s2 = alg.theta_step(theta, m, P, y, 3)
        shared2 = alg.theta_step(theta[:9], m[0], P[0], y[0], 3)
        monkeypatch.delenv('SSMQ_NO_THETA_ITEM')
        what = type(dyn).__name__ + ' ' + pts
        assert np.array_equal(s1, s2) and s1[5] != 0 and (s1 == 0).sum() > n // 2, what
        ok = s1 == 0
        assert np.array_equal(m1[ok], m2[ok]) and np.array_equal(c1[ok], c2[ok]), what
        assert np.array_equal(np.isnan(l1), np.isnan(l2)) and np.max(np.abs(l1[ok] - l2[ok]) / np.abs(l2[ok])) < 1e-14, what
        assert np.array_equal(shared[0], shared2[0]) and np.array_equal(shared[1], shared2[1]) and np.array_equal(shared[3], shared2[3]), what
