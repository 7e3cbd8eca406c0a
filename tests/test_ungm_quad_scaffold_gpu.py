"""The time loop of k_filter_ungm_quad (csrc/ssmq_filter_ungm_quad.hip): one 32-bit lane byte offset for the planes of y, fm and fP
against uniform bases, a scalar offset into the time table, the last step peeled (it requests nothing ahead), the steps before it
two per trip with an odd one behind them.  None of that touches the arithmetic, so the kernel must still leave the BITS of the
one-lane kernel k_filter_fused<1, 1, N, N, ...> (route forced with SSMQ_FUSED_QUAD = 1 / 0, as in tests/test_ungm_quad_gpu.py) -
here at the shapes where this scaffold can go wrong:

  T = 1 .. 5        only the peeled step; the odd step and the peeled one; one trip; a trip and the odd step; two trips
  B = 1 .. 65       a partial quad wave, a full one, one trajectory in a second wave, five waves
  ld                the batch rounded up to 64, and 64 more: the step offset is the PITCH, not the batch
  N = 2, 3, 5

The outputs are given to `ssmq_filter_forward_dev` as blocks of T + 1 planes filled with a canary: the kernels own the first B
entries of the first T planes, and everything else - the padding of every plane and the whole plane behind the last step, where an
offset that runs one plane too far would land - must still hold the canary afterwards.  The blocks of both routes are compared whole.

The failing batches: a NEGATIVE measurement-noise variance makes the innovation variance P_y <= 0 on some trajectories.  (N, R, T,
seed) were chosen on the CPU against the C oracle (oracle/c_oracle.py filter_forward on oracle weights, B = 65, y = 3 *
standard_normal(seed)) so that at least one and at most half of the trajectories fail: N = 2, R = -0.01, T = 12, seed 2: 5 fail
(steps 5, 7); N = 3, R = -0.4, T = 5, seed 2: 4 fail (step 4); N = 5, R = -0.6, T = 5, seed 3: 6 fail (steps 4, 5)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

POINTS = {2: ('sr', None), 3: ('ut', None), 5: ('gh', {'degree': 5})}
BATCHES = (1, 15, 16, 17, 65)
STEPS = (1, 2, 3, 4, 5)
FAILING = {2: (-0.01, 12, 2), 3: (-0.4, 5, 2), 5: (-0.6, 5, 3)}      # N: (measurement-noise variance, T, seed); B = 65
CANARY = np.float64(-1.2345678901234567e+123)
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


def measurements(T, B, seed):
    return 3.0 * np.random.default_rng(seed).standard_normal((1, T, B))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def run(monkeypatch, alg, n, y, ld, mode):
    """One `ssmq_filter_forward_dev` call with SSMQ_FUSED_QUAD=mode on measurement planes of exactly T * ld doubles and output
    blocks of T + 1 planes of canaries: (fm block (T + 1, ld), fP block (T + 1, ld), status (B,))."""
    from ssmtoybox_amd import _lib
    _, T, B = y.shape
    monkeypatch.setenv('SSMQ_FUSED_QUAD', mode)
    kn = alg.kernel_name(B, ld, T)
    assert kn.startswith('k_filter_ungm_quad<N=%d,' % n if mode == '1' else 'k_filter_fused<D=1,Y=1,ND=%d,' % n), kn
    d_y, d_fm, d_fP, d_st = (_lib.DeviceBuffer(8 * T * ld), _lib.DeviceBuffer(8 * (T + 1) * ld), _lib.DeviceBuffer(8 * (T + 1) * ld),
                             _lib.DeviceBuffer(4 * ld))
    try:
        _lib.upload_study(y, 1, ld, d_y)
        canaries = np.full((T + 1, ld), CANARY)
        d_fm.upload(canaries)
        d_fP.upload(canaries)
        d_st.upload(np.full(ld, -77, dtype=np.int32))
        with _lib.Staging() as stage:
            d_m0, d_P0 = alg._initial_planes(stage, B, ld, broadcast_on_device=True)
            alg._launch(_lib.load(), B, ld, T, d_y, d_m0, d_P0, d_fm, d_fP, d_st)
            _lib.sync()
        st = d_st.download((ld,), dtype=np.int32)
        assert np.all(st[B:] == -77), 'status written behind the batch'
        return d_fm.download((T + 1, ld)), d_fP.download((T + 1, ld)), st[:B]
    finally:
        for b in (d_y, d_fm, d_fP, d_st):
            b.free()


def assert_canaries(res, B, what):
    """Only the first B entries of the first T planes were written."""
    for name, blk in zip(('fm', 'fP'), res[:2]):
        T = blk.shape[0] - 1
        assert np.all(bits(blk[T]) == bits(CANARY)), '%s: %s: the plane behind the last step was written' % (what, name)
        assert np.all(bits(blk[:T, B:]) == bits(CANARY)), '%s: %s: the padding of a plane was written' % (what, name)
        assert not np.any(bits(blk[:T, :B]) == bits(CANARY)), '%s: %s: a result was not written' % (what, name)


def assert_same_bits(a, b, what):
    for name, u, v in zip(('filtered means', 'covariances', 'status'), a, b):
        assert u.shape == v.shape, (what, name)
        same = np.array_equal(bits(u), bits(v)) if u.dtype == np.float64 else np.array_equal(u, v)
        assert same, '%s: %s differ in %d of %d entries' % (what, name, int(np.sum(bits(u) != bits(v)) if u.dtype == np.float64 else np.sum(u != v)), u.size)


@pytest.mark.parametrize('B', BATCHES)
@pytest.mark.parametrize('n', sorted(POINTS))
def test_scaffold_leaves_the_bits_of_the_one_lane_kernel_and_nothing_else(amd, monkeypatch, n, B):
    from ssmtoybox_amd import _lib
    alg = gpqkf(n)
    for T in STEPS:
        for ld in (_lib.padded(B), _lib.padded(B) + 64):
            what = 'N = %d, B = %d, T = %d, ld = %d' % (n, B, T, ld)
            y = measurements(T, B, seed=1000 * n + 10 * T + B)
            quad = run(monkeypatch, alg, n, y, ld, '1')
            lane = run(monkeypatch, alg, n, y, ld, '0')
            assert np.isfinite(lane[0][:T, :B]).any(), what
            assert_canaries(lane, B, what + ', one lane')
            assert_canaries(quad, B, what + ', quad')
            assert_same_bits(quad, lane, what)
    # the same call once more: the same bits
    assert_same_bits(run(monkeypatch, alg, n, y, ld, '1'), quad, what + ', repeated')


@pytest.mark.parametrize('n', sorted(FAILING))
def test_failing_trajectories_leave_the_same_status_and_nans(amd, monkeypatch, n):
    from ssmtoybox_amd import _lib
    r_var, T, seed = FAILING[n]
    B = 65
    alg = gpqkf(n, r_var)
    y = measurements(T, B, seed)
    ld = _lib.padded(B)
    quad = run(monkeypatch, alg, n, y, ld, '1')
    lane = run(monkeypatch, alg, n, y, ld, '0')
    st = lane[2]
    failed = int((st != 0).sum())
    print('N = %d, R = %g, T = %d, seed %d: %d of %d trajectories fail, first failing steps %s' % (n, r_var, T, seed, failed, B, np.unique(st[st != 0])))
    assert 1 <= failed <= B // 2, (n, failed)
    assert st.min() >= 0 and st.max() <= T
    assert_canaries(quad, B, 'N = %d with failing trajectories' % n)
    assert_same_bits(quad, lane, 'N = %d with failing trajectories' % n)
    for fm, fP, s in (quad, lane):
        for b in range(B):
            k = s[b] - 1 if s[b] else T          # first failing step (0-based); everything before it finite, NaN from it on
            assert np.all(np.isfinite(fm[:k, b])) and np.all(np.isfinite(fP[:k, b])), (n, b, s[b])
            assert np.all(np.isnan(fm[k:T, b])) and np.all(np.isnan(fP[k:T, b])), (n, b, s[b])
    assert_same_bits(run(monkeypatch, alg, n, y, ld, '1'), quad, 'N = %d with failing trajectories, repeated' % n)


def test_route_is_bounded_by_the_32_bit_offsets(amd, monkeypatch):
    """The kernel's byte offsets into a pass's planes are 32-bit: it takes passes of 8 ld T < 2^31 bytes, larger ones keep the
    one-lane kernel.  Name queries only - nothing of these sizes is allocated or launched."""
    monkeypatch.setenv('SSMQ_FUSED_QUAD', '1')
    for n in sorted(POINTS):
        alg = gpqkf(n)
        quad, lane = 'k_filter_ungm_quad<N=%d,' % n, 'k_filter_fused<D=1,Y=1,ND=%d,' % n
        assert alg.kernel_name(10000).startswith(quad)                              # no pitch, no step count: the batch alone
        assert alg.kernel_name(10000, 10048, 100).startswith(quad)                  # the benchmark's pass
        assert alg.kernel_name(10000, 2 ** 21, 127).startswith(quad)                # 8 ld T = 2^31 - 2^24
        assert alg.kernel_name(10000, 2 ** 21 - 64, 128).startswith(quad)           # 8 ld T = 2^31 - 2^16
        assert alg.kernel_name(10000, 2 ** 21, 128).startswith(lane), alg.kernel_name(10000, 2 ** 21, 128)       # 8 ld T = 2^31
        assert alg.kernel_name(10000, 2 ** 29, 1).startswith(lane)                  # 8 ld alone is 2^32
    monkeypatch.setenv('SSMQ_FUSED_QUAD', '0')
    assert gpqkf(3).kernel_name(10000, 10048, 100).startswith('k_filter_fused<D=1,Y=1,ND=3,')
