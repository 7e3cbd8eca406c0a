"""Streaming Monte-Carlo transform and KL scores, the parts that need no GPU: the routing of MonteCarloTransform(dim, n, seed),
the range errors (raised before the library is touched), the new C ABI names, the NumPy restatement of the draws, and the
statistical bounds of tests/test_mc_transform_gpu.py checked here on the oracle's draws, so that the seeds the GPU test uses are
known to pass before a GPU sees them."""
import os
import re

import numpy as np
import pytest

import ssmtoybox_amd as amd
from ssmtoybox_amd import _lib, ssmod, utils
from tests import _mc_oracle as mo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ('ssmq_mc_transform_dev', 'ssmq_mc_unit_points', 'ssmq_kl_divergence_dev')

# the linear case of the statistics tests (here on the oracle's draws, in test_mc_transform_gpu.py on the device)
STAT_N, STAT_SEED, STAT_DT = 65536, 2024, 0.5
STAT_MEAN = np.array([1.0, -2.0, 0.5, 3.0])
_a = np.random.default_rng(11).standard_normal((4, 4))
STAT_COV = _a.dot(_a.T) / 4 + 0.5 * np.eye(4)
STAT_A = np.array([[1, STAT_DT, 0, 0], [0, 1, 0, 0], [0, 0, 1, STAT_DT], [0, 0, 0, 1.0]])


def check_linear_statistics(mean_f, cov_f, n=STAT_N):
    """mean_f - A m within 6 standard errors sqrt((A P A')_ii / n) per component, cov_f within the 6 standard-error Wishart
    bound sqrt(((APA')_ii (APA')_jj + (APA')_ij^2) / (n - 1)): every component, no exemptions."""
    S = STAT_A.dot(STAT_COV).dot(STAT_A.T)
    em = np.abs(mean_f - STAT_A.dot(STAT_MEAN)) / np.sqrt(np.diag(S) / n)
    ec = np.abs(cov_f - S) / np.sqrt((np.outer(np.diag(S), np.diag(S)) + S ** 2) / (n - 1))
    print('linear statistics: mean within {:.2f} se, covariance within {:.2f} se'.format(em.max(), ec.max()))
    assert (em <= 6.0).all(), em
    assert (ec <= 6.0).all(), ec


def test_routing_of_n_and_seed():
    tf = amd.MonteCarloTransform(3, 4096)
    assert not tf.streaming and tf.unit_sp.shape == (3, 4096) and tf.wm.shape == (4096,) and tf.Wc.shape == (4096, 4096)
    tf = amd.MonteCarloTransform(3, 4097)             # the parent commit raised ValueError above 4 096 points
    assert tf.streaming and tf.seed == 0 and not hasattr(tf, 'unit_sp')
    assert tf.wm == 1.0 / 4097 and tf.Wc == 1.0 / 4096
    tf = amd.MonteCarloTransform(2, int(1e4), seed=5)
    assert tf.streaming and tf.n == 10000 and tf.seed == 5
    tf = amd.MonteCarloTransform(2, 100, seed=0)      # any seed takes the streaming route
    assert tf.streaming and tf.wm == 0.01
    assert not amd.MonteCarloTransform(2).streaming   # the reference's default n = 100, np.random points


def test_range_errors_before_the_library_is_touched(monkeypatch):
    def no_library():
        raise AssertionError('the library was touched')
    monkeypatch.setattr(_lib, 'load', no_library)
    with pytest.raises(NotImplementedError, match='1 <= dim <= 6'):
        amd.MonteCarloTransform(7, 5000)
    with pytest.raises(ValueError, match='2 <= n'):
        amd.MonteCarloTransform(2, 1, seed=3)
    with pytest.raises(ValueError, match='2 <= n'):
        amd.MonteCarloTransform(2, 2 ** 31, seed=3)
    tf = amd.MonteCarloTransform(5, 5000)
    m, P = np.zeros((2, 5)), np.tile(np.eye(5), (2, 1, 1))
    seven = ssmod.BearingMeasurement(ssmod.GaussRV(7), 5, state_index=[0, 2], sensor_pos=np.arange(14.0).reshape(7, 2))
    with pytest.raises(NotImplementedError, match='outputs <= 6'):
        tf.apply_batch(seven.meas_eval, m, P)
    with pytest.raises(NotImplementedError, match='Python callable'):
        tf.apply_batch(lambda x, t: x, m, P)
    with pytest.raises(NotImplementedError, match='Python callable'):
        tf.apply(lambda x, t: x, m[0], P[0], None)
    with pytest.raises(NotImplementedError, match='filter'):
        tf._handle_for(5)
    with pytest.raises(NotImplementedError, match='1 <= E <= 6'):
        utils.kl_divergence_batch(np.zeros(7), np.eye(7), np.zeros((3, 7)), np.tile(np.eye(7), (3, 1, 1)))


def test_streaming_transform_is_refused_as_a_filter_transform():
    from ssmtoybox_amd import ssinf
    dyn = ssmod.UNGMTransition(ssmod.GaussRV(1), ssmod.GaussRV(1))
    obs = ssmod.UNGMMeasurement(ssmod.GaussRV(1), 1)
    alg = ssinf.UnscentedKalman(dyn, obs)
    alg.tf_dyn = amd.MonteCarloTransform(1, 5000)
    with pytest.raises(NotImplementedError, match='filter'):
        alg.forward_pass(np.zeros((1, 3)))


def test_new_symbols_in_header_and_binding():
    header = open(os.path.join(ROOT, 'include', 'ssmq.h')).read()
    for name in NEW_SYMBOLS:
        assert re.search(r'\bint {}\('.format(name), header), name
        assert name in _lib.EXPORTED_SYMBOLS
        assert hasattr(_lib.load(), name)
    assert _lib.load().ssmq_version() == _lib.ABI_VERSION == 102


def test_user_integrand_compiles_for_the_streaming_kernel():
    """k_mc_moments<id, D, E, 0> through the run-time compiler, for gfx950, without a device: the embedded headers (the generator
    and the kernel body among them) compile there and the kernel keeps its accumulators in registers."""
    fid = _lib.define_integrand('o[0] = x[0] + x[1] * p[0];  o[1] = x[1] - 9.81 * p[0] * sin_nr(x[0]);', 2, 2, False)
    rc, log = _lib.rtc_compile_check(fid, _lib.RTC_MC, 2, 2, 0, 0)
    assert rc == 0, log
    assert 'k_mc_moments' in log.splitlines()[0]
    six = _lib.define_integrand('for (int i = 0; i < 6; ++i) o[i] = x[i] * x[(i + 1) % 6];', 6, 6, False)
    rc, log = _lib.rtc_compile_check(six, _lib.RTC_MC, 6, 6, 0, 0)
    assert rc == 0, log
    assert re.search(r'ScratchSize \[bytes/lane\]: 0\b', log), log
    rc, _ = _lib.rtc_compile_check(six, _lib.RTC_MC, 7, 6, 0, 0)
    assert rc == -3                                   # SSMQ_E_UNSUPPORTED: D = 7


def test_oracle_draws_are_counter_based():
    z = mo.unit_points(7, 5, 0, 200)
    assert z.shape == (5, 200) and np.isfinite(z).all()
    assert np.array_equal(z[:, 37:90], mo.unit_points(7, 5, 37, 53))
    assert np.array_equal(z[:4], mo.unit_points(7, 4, 0, 200))           # coordinate d does not depend on D
    assert not np.array_equal(z, mo.unit_points(8, 5, 0, 200))
    big = mo.unit_points(1 << 40 | 3, 2, 2 ** 31 - 5, 5)                 # the last sample indices, a seed with a high half
    assert np.isfinite(big).all()


def test_oracle_draws_are_standard_normal():
    z = mo.unit_points(STAT_SEED, 4, 0, STAT_N)
    assert np.abs(z.mean(axis=1)).max() < 6 / np.sqrt(STAT_N)
    assert np.abs(np.cov(z) - np.eye(4)).max() < 6 * np.sqrt(2.0 / STAT_N)
    assert abs(np.mean(z ** 4) - 3.0) < 6 * np.sqrt(96.0 / z.size)


def test_linear_statistics_on_the_oracle_draws():
    z = mo.unit_points(STAT_SEED, 4, 0, STAT_N)
    mf, cf, cfx = mo.moments(lambda x, t: mo.f_cv(x, t, STAT_DT), STAT_MEAN, STAT_COV, z, dtype=np.float64)
    check_linear_statistics(mf, cf)
    # the one-pass pivot form of the kernel agrees with the centred form in exact arithmetic: here in long double
    L = mo.cholesky(STAT_COV.astype(mo.LD))
    zz = z.astype(mo.LD)
    c = mo.f_cv(STAT_MEAN.astype(mo.LD)[:, None], 0.0, STAT_DT)[:, 0]
    df = mo.f_cv(STAT_MEAN.astype(mo.LD)[:, None] + L.dot(zz), 0.0, STAT_DT) - c[:, None]
    n = mo.LD(STAT_N)
    S1, S2, S3, Sz = df.sum(axis=1), df.dot(df.T), df.dot(zz.T), zz.sum(axis=1)
    exact = mo.moments(lambda x, t: mo.f_cv(x, t, STAT_DT), STAT_MEAN, STAT_COV, z)
    pivot = (c + S1 / n, (S2 - np.outer(S1, S1) / n) / (n - 1), ((S3 - np.outer(S1, Sz) / n) / (n - 1)).dot(L.T))
    assert max(mo.scaled_errors(pivot, exact)) < 1e-16
