"""k_filter_ungm_quad (csrc/ssmq_filter_ungm_quad.hip: a scalar UNGM trajectory on the four lanes of a quad, only the dynamics
integrand dealt to the lanes and its values broadcast) against the one-lane kernel k_filter_fused<1, 1, N, N, ..., OPT = 0> it
stands in for: the same operations in the same order, so `ssmq_filter_forward_dev` with the route forced on (SSMQ_FUSED_QUAD=1)
and forced off (=0) must leave the same BITS - filtered means, covariances (NaNs by position: compared as uint64) and status.

GP-quadrature Kalman filters on UNGM with 2 (spherical-radial), 3 (unscented) and 5 (Gauss-Hermite) points.  Batches of 1, 3, 15,
16, 17 and 195 trajectories: partial quads' worth of a wave, a full wave of 16, one trajectory in a second wave, a last wave with
three.  T = 1, 2, 3, 40 (the measurement of step k + 1 is requested in step k; the last step re-requests its own).  The planes'
pitch is always larger than the batch.

The batches that fail: a NEGATIVE measurement-noise variance makes the innovation variance P_y <= 0 on some trajectories at some
step.  (N, R, T) below and the seed were chosen against the C oracle (oracle/c_oracle.py filter_forward on oracle weights, B = 195,
y = 3 * standard_normal(seed 1)): N = 2, R = -0.01, T = 40: 65 trajectories fail, first at steps 4 .. 40; N = 3, R = -0.4, T = 12:
154 fail; N = 5, R = -0.6, T = 12: 145 fail."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

POINTS = {2: ('sr', None), 3: ('ut', None), 5: ('gh', {'degree': 5})}
BATCHES = (1, 3, 15, 16, 17, 195)
STEPS = (1, 2, 3, 40)
FAILING = {2: (-0.01, 40), 3: (-0.4, 12), 5: (-0.6, 12)}      # N: (measurement-noise variance, T); B = 195, seed 1
_ALGS = {}


@pytest.fixture(scope='module')
def amd():
    import ssmtoybox_amd
    if ssmtoybox_amd.device_count() < 1:
        pytest.fail('no device: the GPU tests need an MI355X')
    ssmtoybox_amd.set_device(0)
    return ssmtoybox_amd


def gpqkf(n, r_var=1.0):
    """The GPQ-Kalman filter on UNGM with n points and measurement-noise variance r_var: made once."""
    from ssmtoybox_amd import ssinf, ssmod as sm
    if (n, r_var) not in _ALGS:
        dyn = sm.UNGMTransition(sm.GaussRV(1), sm.GaussRV(1, cov=np.array([[10.0]])))
        obs = sm.UNGMMeasurement(sm.GaussRV(1, cov=np.array([[r_var]])), 1)
        par = np.array([[1.0, 3.0]])
        pts, hyp = POINTS[n]
        _ALGS[(n, r_var)] = ssinf.GaussianProcessKalman(dyn, obs, par, par, 'rbf', pts, hyp)
        assert _ALGS[(n, r_var)].tf_dyn.model.points.shape[1] == n
    return _ALGS[(n, r_var)]


def measurements(T, B, seed=1):
    return 3.0 * np.random.default_rng(seed).standard_normal((1, T, B))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def run(monkeypatch, alg, n, y, ld, mode):
    """One `ssmq_filter_forward_dev` call (forward_pass_dev) on planes of pitch ld with SSMQ_FUSED_QUAD=mode:
    (fm (1, T, B), fP (1, 1, T, B), status (B,))."""
    from ssmtoybox_amd import _lib
    _, T, B = y.shape
    monkeypatch.setenv('SSMQ_FUSED_QUAD', mode)
    kn = alg.kernel_name(B)
    assert kn.startswith('k_filter_ungm_quad<N=%d,' % n if mode == '1' else 'k_filter_fused<D=1,Y=1,ND=%d,' % n), kn
    d_y = _lib.DeviceBuffer(8 * T * ld)
    bufs = ()
    try:
        _lib.upload_study(y, 1, ld, d_y)
        bufs = alg.forward_pass_dev(d_y, B, ld, T)
        d_fm, d_fP, d_st = bufs
        return (_lib.download_study(d_fm, (1,), T, B, ld), _lib.download_study(d_fP, (1, 1), T, B, ld),
                d_st.download((ld,), dtype=np.int32)[:B])
    finally:
        d_y.free()
        for b in bufs:
            b.free()


def assert_same_bits(a, b, what):
    for name, u, v in zip(('filtered means', 'covariances', 'status'), a, b):
        assert u.shape == v.shape, (what, name)
        same = np.array_equal(bits(u), bits(v)) if u.dtype == np.float64 else np.array_equal(u, v)
        assert same, '%s: %s differ in %d of %d entries' % (what, name, int(np.sum(bits(u) != bits(v)) if u.dtype == np.float64 else np.sum(u != v)), u.size)


@pytest.mark.parametrize('B', BATCHES)
@pytest.mark.parametrize('n', sorted(POINTS))
def test_quad_route_leaves_the_bits_of_the_one_lane_kernel(amd, monkeypatch, n, B):
    from ssmtoybox_amd import _lib
    alg = gpqkf(n)
    for T in STEPS:
        ld = _lib.padded(B) + (64 if T == 2 else 0)          # the pitch: always > B, once not the batch rounded up
        assert ld > B
        y = measurements(T, B, seed=100 * n + T)
        quad = run(monkeypatch, alg, n, y, ld, '1')
        lane = run(monkeypatch, alg, n, y, ld, '0')
        assert np.isfinite(lane[0]).any()
        assert_same_bits(quad, lane, 'N = %d, B = %d, T = %d, ld = %d' % (n, B, T, ld))
        if T == STEPS[-1]:       # the same call once more: nothing stale, bit for bit
            assert_same_bits(run(monkeypatch, alg, n, y, ld, '1'), quad, 'N = %d, B = %d, T = %d, repeated' % (n, B, T))


@pytest.mark.parametrize('n', sorted(FAILING))
def test_failing_trajectories_fail_at_the_same_step_on_both_routes(amd, monkeypatch, n):
    from ssmtoybox_amd import _lib
    r_var, T = FAILING[n]
    B = 195
    alg = gpqkf(n, r_var)
    y = measurements(T, B, seed=1)
    ld = _lib.padded(B)
    quad = run(monkeypatch, alg, n, y, ld, '1')
    lane = run(monkeypatch, alg, n, y, ld, '0')
    st = lane[2]
    print('N = %d, R = %g, T = %d: %d of %d trajectories fail, first failing steps %s' % (n, r_var, T, int((st != 0).sum()), B, np.unique(st[st != 0])))
    assert (st != 0).any() and (st == 0).any(), (n, int((st != 0).sum()))
    assert st.min() >= 0 and st.max() <= T
    assert_same_bits(quad, lane, 'N = %d with failing trajectories' % n)
    for fm, fP, s in (quad, lane):
        for b in range(B):
            k = s[b] - 1 if s[b] else T          # first failing step (0-based); everything before it finite, NaN from it on
            assert np.all(np.isfinite(fm[0, :k, b])) and np.all(np.isfinite(fP[0, 0, :k, b])), (n, b, s[b])
            assert np.all(np.isnan(fm[0, k:, b])) and np.all(np.isnan(fP[0, 0, k:, b])), (n, b, s[b])
    assert_same_bits(run(monkeypatch, alg, n, y, ld, '1'), quad, 'N = %d with failing trajectories, repeated' % n)


def test_default_route(amd, monkeypatch):
    """Without the switch the quad kernel runs the batches whose quad waves fill at most three quarters of the SIMDs:
    ceil(B / 16) <= 3 x compute units (where it was measured clearly faster)."""
    if any(k in os.environ for k in ('SSMQ_FUSED_QUAD', 'SSMQ_FUSED_WSPLIT', 'SSMQ_NO_FUSED', 'SSMQ_NO_FASTPATH')):
        return           # (a run of the suite under a forced route: the other tests of this file still force both)
    simds = 3 * 256          # MI355X: 256 compute units
    for n in sorted(POINTS):
        alg = gpqkf(n)
        for B in (1, 10000, 16 * simds):
            assert alg.kernel_name(B).startswith('k_filter_ungm_quad<N=%d,' % n), (n, B, alg.kernel_name(B))
        assert alg.kernel_name(16 * simds + 1).startswith('k_filter_fused<D=1,Y=1,ND=%d,' % n), alg.kernel_name(16 * simds + 1)
        assert alg.kernel_name().startswith('k_filter_fused<D=1,Y=1,ND=%d,' % n)          # (no batch given: one that fills the device)
    monkeypatch.setenv('SSMQ_FUSED_WSPLIT', '0')      # a forced wave-split mode (0: the one-lane kernel) is what runs
    assert gpqkf(3).kernel_name(10000).startswith('k_filter_fused<')
