"""Streaming Monte-Carlo transform on the device (csrc/ssmq_mc_transform.hip, k_mc_moments / k_mc_finish) against the NumPy
restatement of tests/_mc_oracle.py.

MEASURED (MI355X):
  draws      unit_points against the NumPy restatement: largest gap 3.00 ulp of the value over 1e5 values (the device's log and
             sincospi against glibc's log and a long-double cos / sin after an exact argument reduction); the test asserts 4 x that.
  moments    test_moments_against_long_double, per integrand the case (n) with the largest ratio device / float64 of the scaled
             errors to the long-double oracle (the bar is 8), and the case n = 2:
               ungm          n = 4097  device 3.704e-15   float64 1.846e-15   ratio 2.01      n = 2: 3.748e-15 / 1.585e-14
               pendulum      n = 2048  device 3.963e-16   float64 2.967e-16   ratio 1.34      n = 2: 1.250e-15 / 1.676e-15
               radar         n = 2     device 6.877e-15   float64 8.295e-15   ratio 0.83
               reentry       n = 4097  device 1.421e-13   float64 1.419e-13   ratio 1.00      n = 2: 2.877e-11 / 1.252e-10
               reentry_bias  n = 4097  device 4.498e-15   float64 5.032e-15   ratio 0.89      n = 2: 4.005e-13 / 2.519e-12
             With ONE pass around f(m) at every n, ungm at n = 2 came out at 1.910e-13 (ratio 12.05): two samples close to each
             other on one side of the pivot.  Sample counts of one chunk now take a second pass around the first pass's mean
             (csrc/ssmq_mc_moments.h, SMALL n).
"""
import numpy as np
import pytest

import ssmtoybox_amd as amd
from ssmtoybox_amd import _lib, ssmod
from tests import _mc_oracle as mo
from tests.test_mc_transform_host import STAT_N, STAT_SEED, STAT_DT, STAT_MEAN, STAT_COV, check_linear_statistics

pytestmark = pytest.mark.gpu

MEASURED_DRAW_ULP = 3.0
C = mo.CHUNK
SEED = 12345


def _models():
    g = ssmod.GaussRV
    return {
        # name: (bound integrand, oracle function, D, centre of the means, spread of the states, time)
        'ungm': (ssmod.UNGMTransition(g(1), g(1)).dyn_eval, mo.f_ungm, 1, [0.7], [1.5], 3.0),
        'pendulum': (ssmod.Pendulum2DTransition(g(2), g(2)).dyn_eval, mo.f_pendulum, 2, [1.5, 0.0], [0.4, 0.8], 0.0),
        'radar': (ssmod.Radar2DMeasurement(g(2), 5, state_index=[0, 2]).meas_eval, lambda x, t: mo.f_radar(x, t, (0, 2)), 5,
                  [30.0, 1.0, 40.0, -1.0, 0.1], [2.0, 1.0, 2.0, 1.0, 0.05], 0.0),
        'reentry': (ssmod.ReentryVehicle2DTransition(g(5), g(3)).dyn_eval, mo.f_reentry, 5,
                    [6500.4, 349.14, -1.8093, -6.7967, 0.6932], [1e-1, 1e-1, 1e-2, 1e-2, 1e-2], 0.0),
        'reentry_bias': (ssmod.ReentryVehicle2DBiasTransition(g(6), g(4)).dyn_eval, mo.f_reentry_bias, 6,
                         [6500.4, 349.14, -1.8093, -6.7967, 0.6932, 0.3], [1e-1, 1e-1, 1e-2, 1e-2, 1e-2, 1.0], 0.0),
    }


@pytest.fixture(scope='module')
def device_points():
    """The device's own unit points for SEED, the first 3 C + 5 samples of the widest shape (coordinate d does not depend on D);
    computed once, read-only."""
    z = amd.MonteCarloTransform(6, 3 * C + 5, seed=SEED).unit_points()
    z.setflags(write=False)
    return z


# ---- draws ------------------------------------------------------------------------------------------------------------------------
def test_unit_points_against_numpy():
    tf = amd.MonteCarloTransform(5, 20000, seed=SEED)
    z, ref = tf.unit_points(0, 20000), mo.unit_points(SEED, 5, 0, 20000)
    gap = np.max(np.abs(z - ref) / np.spacing(np.abs(ref)))
    print('unit_points: largest gap to the NumPy restatement {:.2f} ulp'.format(gap))
    assert gap <= 4 * MEASURED_DRAW_ULP
    hi = amd.MonteCarloTransform(2, 2 ** 31 - 1, seed=(1 << 40) | 3)     # the last sample indices, a seed with a high half
    zh, rh = hi.unit_points(2 ** 31 - 6, 5), mo.unit_points((1 << 40) | 3, 2, 2 ** 31 - 6, 5)
    assert np.max(np.abs(zh - rh) / np.spacing(np.abs(rh))) <= 4 * MEASURED_DRAW_ULP


def test_unit_point_slices_and_seeds():
    tf = amd.MonteCarloTransform(5, 5000, seed=SEED)
    z = tf.unit_points(0, 200)
    assert np.array_equal(z[:, 37:90], tf.unit_points(37, 53))
    assert np.array_equal(z[:3], amd.MonteCarloTransform(3, 5000, seed=SEED).unit_points(0, 200))
    assert not np.array_equal(z, amd.MonteCarloTransform(5, 5000, seed=SEED + 1).unit_points(0, 200))
    assert np.array_equal(amd.MonteCarloTransform(5, 5000).unit_points(0, 50), amd.MonteCarloTransform(5, 5000, seed=0).unit_points(0, 50))


# ---- reductions and integrands ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['ungm', 'pendulum', 'radar', 'reentry', 'reentry_bias'])
def test_moments_against_long_double(name, device_points):
    """The device against the long-double oracle fed the device's own unit points; its scaled error may be at most 8 x that of
    the same (two-pass) formulas in NumPy float64 on the same draws - the one-pass pivot form and a different summation order
    may lose a little.  The scaled error of a case (integrand, n) is the largest over its three items and the three outputs, each
    output's largest deviation over its largest magnitude: the error of ONE float64 result to the exact value is anything between
    zero (the mean of two samples is often exact) and a few ulp, so a ratio per element would have no scale; the largest of a
    case's nine arrays is the noise level of float64 on that case."""
    f, f_np, D, centre, spread, t = _models()[name]
    mean, cov = mo.random_moments(np.random.default_rng(D), 3, D, centre, spread)
    worst, failed = (0.0, 0.0, 0.0), []
    for n in (2, 63, 64, 65, C - 1, C, C + 1, 3 * C + 5, 4097):
        tf = amd.MonteCarloTransform(D, n, seed=SEED)
        got = tf.apply_batch(f, mean, cov, time=t)
        z = device_points[:D, :n]
        e_dev = e_f64 = 0.0
        for b in range(3):
            exact = mo.moments(f_np, mean[b], cov[b], z, t)
            f64 = mo.moments(f_np, mean[b], cov[b], z, t, dtype=np.float64)
            e_dev = max(e_dev, max(mo.scaled_errors([g[b] for g in got], exact)))
            e_f64 = max(e_f64, max(mo.scaled_errors(f64, exact)))
            assert np.array_equal(got[1][b], got[1][b].T)          # both triangles from one value
        print('{} n = {}: device {:.3e}, float64 {:.3e}, ratio {:.2f}'.format(name, n, e_dev, e_f64, e_dev / e_f64))
        if e_dev / e_f64 > worst[2]:
            worst = (e_dev, e_f64, e_dev / e_f64)
        if not e_dev <= 8 * e_f64:
            failed.append((n, e_dev, e_f64))
    print('{}: worst ratio {:.2f} (device {:.3e}, float64 {:.3e})'.format(name, worst[2], worst[0], worst[1]))
    assert not failed, failed


# ---- reproducibility ----------------------------------------------------------------------------------------------------------------
def test_bits_do_not_depend_on_the_batch():
    f, _, D, centre, spread, t = _models()['pendulum']
    mean, cov = mo.random_moments(np.random.default_rng(3), 193, D, centre, spread)
    n = 64 * C + 7                                                 # one item alone: 65 workgroups share it
    tf = amd.MonteCarloTransform(D, n, seed=SEED)
    full = tf.apply_batch(f, mean, cov, time=t)
    again = tf.apply_batch(f, mean, cov, time=t)
    for a, b in zip(full, again):
        assert np.array_equal(a, b)
    for b in (0, 100, 192):
        one = tf.apply_batch(f, mean[b:b + 1], cov[b:b + 1], time=t)
        for a, o in zip(full, one):
            assert np.array_equal(a[b], o[0])
    single = tf.apply(f, mean[7], cov[7], np.atleast_1d(t))
    for a, o in zip(full, single):
        assert np.array_equal(a[7], o)
    assert single[0].shape == (2,) and single[1].shape == (2, 2) and single[2].shape == (2, 2)


def test_device_resident_variant_and_per_item_time():
    f, f_np, D, centre, spread, _ = _models()['ungm']
    B, n = 70, 1000
    mean, cov = mo.random_moments(np.random.default_rng(4), B, D, centre, spread)
    times = np.arange(B, dtype=float)
    tf = amd.MonteCarloTransform(D, n, seed=SEED)
    host = tf.apply_batch(f, mean, cov, time=times)
    d_m, d_c = _lib.SoA.from_host(mean), _lib.SoA.from_host(cov)
    d_t = _lib.DeviceBuffer(8 * B)
    d_t.upload(times)
    d_mf, d_cf, d_cfx, d_st = _lib.SoA(1, B), _lib.SoA(1, B), _lib.SoA(1, B), _lib.DeviceBuffer(4 * d_m.ld)
    tf.apply_batch_dev(f, d_m, d_c, d_t, d_mf, d_cf, d_cfx, d_st, time_stride=1)
    assert np.array_equal(d_mf.to_host(), host[0]) and np.array_equal(d_cf.to_host((1, 1)), host[1])
    assert np.array_equal(d_cfx.to_host((1, 1)), host[2])
    z = tf.unit_points()
    for b in (0, 69):
        exact = mo.moments(f_np, mean[b], cov[b], z, times[b])
        assert max(mo.scaled_errors([h[b] for h in host], exact)) < 1e-13


# ---- statistics ---------------------------------------------------------------------------------------------------------------------
def test_linear_statistics():
    cv = ssmod.ConstantVelocity(ssmod.GaussRV(4), ssmod.GaussRV(2), dt=STAT_DT)
    mf, cf, cfx = amd.MonteCarloTransform(4, STAT_N, seed=STAT_SEED).apply(cv.dyn_eval, STAT_MEAN, STAT_COV, None)
    check_linear_statistics(mf, cf)


# ---- status -------------------------------------------------------------------------------------------------------------------------
def test_indefinite_covariance_marks_its_item_only():
    f, _, D, centre, spread, t = _models()['reentry']
    mean, cov = mo.random_moments(np.random.default_rng(5), 5, D, centre, spread)
    tf = amd.MonteCarloTransform(D, 3 * C + 5, seed=SEED)
    clean = tf.apply_batch(f, mean, cov, time=t, return_status=True)
    assert not clean[3].any()
    bad = cov.copy()
    bad[2, 3, 3] = -bad[2, 3, 3]
    got = tf.apply_batch(f, mean, bad, time=t, return_status=True)
    assert got[3][2] != 0 and not got[3][[0, 1, 3, 4]].any()
    for a, c in zip(got[:3], clean[:3]):
        assert np.isnan(a[2]).all()
        assert np.array_equal(a[[0, 1, 3, 4]], c[[0, 1, 3, 4]])
    with pytest.raises(np.linalg.LinAlgError):
        tf.apply(f, mean[2], bad[2], None)
    with pytest.raises(np.linalg.LinAlgError):
        tf.apply_batch(f, mean, bad, time=t)


def test_unsupported_combination_is_an_error():
    ct = ssmod.CoordinatedTurnTransition(ssmod.GaussRV(5), ssmod.GaussRV(5))
    odd = ssmod.Radar2DMeasurement(ssmod.GaussRV(2), 5, state_index=[1, 3])          # a state index the kernels have no pattern for
    tf = amd.MonteCarloTransform(5, 5000)
    with pytest.raises(_lib.SsmqError, match='no streaming kernel'):
        tf.apply_batch(odd.meas_eval, np.ones((1, 5)), np.eye(5)[None])
    mf, _, _ = tf.apply_batch(ct.dyn_eval, np.ones((1, 5)), np.eye(5)[None])
    assert np.isfinite(mf).all()


# ---- user model ---------------------------------------------------------------------------------------------------------------------
class UserPendulum(ssmod.TransitionModel):
    dim_state, dim_noise, noise_additive = 2, 2, True
    device_code = 'o[0] = x[0] + x[1] * p[0];  o[1] = x[1] - 9.81 * p[0] * sin_nr(x[0]);  /* streaming Monte-Carlo test */'

    def _par(self):
        return (0.01,)


def test_user_model_gives_the_builtin_bits():
    f, _, D, centre, spread, t = _models()['pendulum']
    mean, cov = mo.random_moments(np.random.default_rng(6), 3, D, centre, spread)
    tf = amd.MonteCarloTransform(2, 4097, seed=SEED)
    builtin = tf.apply_batch(f, mean, cov)
    user = UserPendulum(ssmod.GaussRV(2), ssmod.GaussRV(2))
    c0, h0, _ = _lib.rtc_stats()
    first = tf.apply_batch(user.dyn_eval, mean, cov)
    c1, h1, _ = _lib.rtc_stats()
    second = tf.apply_batch(user.dyn_eval, mean, cov)
    c2, h2, _ = _lib.rtc_stats()
    assert c1 == c0 + 1 and c2 == c1 and h2 == h1 + 1            # one compile, then the cache
    for a, b, c in zip(builtin, first, second):
        assert np.array_equal(a, b) and np.array_equal(a, c)
    assert tf.kernel_name(user.dyn_eval) == 'k_mc_moments'
