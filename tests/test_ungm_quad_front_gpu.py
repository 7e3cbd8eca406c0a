"""The front and the tail of k_filter_ungm_quad (csrc/ssmq_filter_ungm_quad.hip): the kernel requests its arguments in one batch in
front of its early-out, requests the initial state and every transform constant of a step together behind that, and runs the
peeled odd step and the peeled last step on the constants the loop holds.  None of that is arithmetic, so the quad route must
still give the bits of the one-lane route k_filter_fused<1, 1, N, N, ...> (SSMQ_FUSED_QUAD=0, forced as in
tests/test_ungm_quad_gpu.py) - at the shapes where index arithmetic, the early-out or a peeled step can go wrong:

  N = 2, 3, 5;  T = 1 (last step only), 2 (odd step and last), 3 (one trip), 4, 5;
  B = 1, 15, 16, 17 (partial wave, full wave, one more), 63, 64, 65, 257 (the same for a group of four waves);
  ld = the batch rounded up to 64, and to 128.

`fm`, `fP` and `status` lie between canary planes, and the padding of every plane (columns B .. ld - 1, status words beyond B) is
canary too: a wave or a lane that leaves through the early-out - now behind loads - must still write nothing."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

POINTS = {2: ('sr', None), 3: ('ut', None), 5: ('gh', {'degree': 5})}
BATCHES = (1, 15, 16, 17, 63, 64, 65, 257)
STEPS = (1, 2, 3, 4, 5)
CANARY = np.float64(-1.2345678901234567e+123)
ST_CANARY = -77
_ALGS = {}


@pytest.fixture(scope='module')
def amd():
    import ssmtoybox_amd
    if ssmtoybox_amd.device_count() < 1:
        pytest.fail('no device: the GPU tests need an MI355X')
    ssmtoybox_amd.set_device(0)
    return ssmtoybox_amd


def gpqkf(n):
    """The GPQ-Kalman filter on UNGM with n points: made once."""
    from ssmtoybox_amd import ssinf, ssmod as sm
    if n not in _ALGS:
        dyn = sm.UNGMTransition(sm.GaussRV(1), sm.GaussRV(1, cov=np.array([[10.0]])))
        obs = sm.UNGMMeasurement(sm.GaussRV(1), 1)
        par = np.array([[1.0, 3.0]])
        pts, hyp = POINTS[n]
        _ALGS[n] = ssinf.GaussianProcessKalman(dyn, obs, par, par, 'rbf', pts, hyp)
        assert _ALGS[n].tf_dyn.model.points.shape[1] == n
    return _ALGS[n]


def pitches(B):
    return ((B + 63) // 64 * 64, (B + 127) // 128 * 128)


def measurements(n, B, T):
    return 3.0 * np.random.default_rng(100000 * n + 10 * B + T).standard_normal((T, B))


class Pass:
    """The buffers of one route for one shape: y [T][ld], m0 / P0 [ld], and fm, fP ([T + 2][ld]) and status ([3][ld]) with a
    canary plane before and behind what the kernel owns.  Every run() goes into the same buffers."""

    def __init__(self, alg, n, B, ld, T, mode):
        from ssmtoybox_amd import _lib
        self.alg, self.n, self.B, self.ld, self.T, self.mode = alg, n, B, ld, T, mode
        self.d_y, self.d_m0, self.d_P0 = _lib.DeviceBuffer(8 * T * ld), _lib.DeviceBuffer(8 * ld), _lib.DeviceBuffer(8 * ld)
        self.d_fm, self.d_fP, self.d_st = _lib.DeviceBuffer(8 * (T + 2) * ld), _lib.DeviceBuffer(8 * (T + 2) * ld), _lib.DeviceBuffer(4 * 3 * ld)
        canaries = np.full((T + 2, ld), CANARY)
        self.d_fm.upload(canaries)
        self.d_fP.upload(canaries)
        self.d_st.upload(np.full(3 * ld, ST_CANARY, dtype=np.int32))
        self.d_m0.upload(np.full(ld, float(np.atleast_1d(alg.x0_mean).ravel()[0])))
        self.d_P0.upload(np.ones(ld))

    def run(self, monkeypatch, y, first):
        """One pass: (fm (T, B), fP (T, B), status (B,)) as stored, the canaries checked."""
        from ssmtoybox_amd import _lib
        B, ld, T, n = self.B, self.ld, self.T, self.n
        if self.mode is None and not any(k in os.environ for k in ('SSMQ_FUSED_WSPLIT', 'SSMQ_NO_FUSED', 'SSMQ_NO_FASTPATH')):
            monkeypatch.delenv('SSMQ_FUSED_QUAD', raising=False)         # the default route
        else:
            monkeypatch.setenv('SSMQ_FUSED_QUAD', self.mode or '1')
        kn = self.alg.kernel_name(B, ld, T)
        assert kn.startswith('k_filter_fused<D=1,Y=1,ND=%d,' % n if self.mode == '0' else 'k_filter_ungm_quad<N=%d,' % n), kn
        planes = np.zeros((T, ld))
        planes[:, :B] = y
        self.d_y.upload(planes)
        self.alg._launch(_lib.load(), B, ld, T, self.d_y, self.d_m0, self.d_P0, self.d_fm.view(8 * ld), self.d_fP.view(8 * ld),
                         self.d_st.view(4 * ld))
        _lib.sync()
        what = 'N = %d, B = %d, T = %d, ld = %d, SSMQ_FUSED_QUAD = %s' % (n, B, T, ld, self.mode)
        out = []
        for name, buf in (('fm', self.d_fm), ('fP', self.d_fP)):
            blk = buf.download((T + 2, ld))
            assert blk[0].tobytes() == np.full(ld, CANARY).tobytes(), '%s: %s: the plane before step 0 was written' % (what, name)
            assert blk[T + 1].tobytes() == np.full(ld, CANARY).tobytes(), '%s: %s: the plane behind the last step was written' % (what, name)
            pad = np.ascontiguousarray(blk[1:T + 1, B:])
            assert pad.tobytes() == np.full(pad.shape, CANARY).tobytes(), '%s: %s: columns B .. ld - 1 were written' % (what, name)
            if first:
                assert not np.any(blk[1:T + 1, :B].view(np.uint64) == CANARY.view(np.uint64)), '%s: %s: a result was not written' % (what, name)
            out.append(np.ascontiguousarray(blk[1:T + 1, :B]))
        st = self.d_st.download((3, ld), dtype=np.int32)
        assert np.all(st[0] == ST_CANARY) and np.all(st[2] == ST_CANARY), what + ': the status rows around the pass were written'
        assert np.all(st[1, B:] == ST_CANARY), what + ': status words beyond B were written'
        out.append(np.ascontiguousarray(st[1, :B]))
        return out

    def free(self):
        for b in (self.d_y, self.d_m0, self.d_P0, self.d_fm, self.d_fP, self.d_st):
            b.free()


def assert_same_bytes(a, b, what):
    for name, u, v in zip(('filtered means', 'covariances', 'status'), a, b):
        assert u.shape == v.shape and u.dtype == v.dtype, (what, name)
        assert u.tobytes() == v.tobytes(), '%s: %s differ in %d of %d entries' % (
            what, name, int(np.sum(u.view(np.uint64 if u.dtype == np.float64 else np.int32) != v.view(np.uint64 if v.dtype == np.float64 else np.int32))), u.size)


@pytest.mark.parametrize('B', BATCHES)
@pytest.mark.parametrize('n', sorted(POINTS))
def test_quad_route_gives_the_bits_of_the_one_lane_route(amd, monkeypatch, n, B):
    alg = gpqkf(n)
    for T in STEPS:
        y = measurements(n, B, T)
        for ld in pitches(B):
            quad, lane = Pass(alg, n, B, ld, T, None), Pass(alg, n, B, ld, T, '0')
            try:
                q, l = quad.run(monkeypatch, y, True), lane.run(monkeypatch, y, True)
                assert_same_bytes(q, l, 'N = %d, B = %d, T = %d, ld = %d' % (n, B, T, ld))
                assert not np.any(q[2]), (n, B, T, ld, q[2])
            finally:
                quad.free()
                lane.free()


@pytest.mark.parametrize('B', (1, 17, 65, 257))
@pytest.mark.parametrize('n', sorted(POINTS))
def test_second_pass_into_the_same_buffers_equals_the_first(amd, monkeypatch, n, B):
    """Two passes into planes pre-filled with a canary: the same bits, and (Pass.run, after each) nothing written outside
    columns 0 .. B - 1 of steps 0 .. T - 1 and status words 0 .. B - 1."""
    alg = gpqkf(n)
    for T in (1, 2, 5):
        y = measurements(n, B, T)
        for ld in pitches(B):
            quad = Pass(alg, n, B, ld, T, None)
            try:
                first = quad.run(monkeypatch, y, True)
                second = quad.run(monkeypatch, y, False)
                assert_same_bytes(second, first, 'N = %d, B = %d, T = %d, ld = %d, second pass' % (n, B, T, ld))
            finally:
                quad.free()


@pytest.mark.parametrize('step', ('first', 'last'))
@pytest.mark.parametrize('n', sorted(POINTS))
def test_status_after_a_planted_failure(amd, monkeypatch, n, step):
    """One trajectory with a NaN measurement at step 0 (the covariance of step 1 is lost: the read-back behind the loop) or at
    step T - 1 (the covariance does not depend on the step's own measurement: status 0), T = 4, B = 17 - planted in the first
    wave's last quad and in the second wave's only one."""
    B, T = 17, 4
    alg = gpqkf(n)
    k = 0 if step == 'first' else T - 1
    for bad in (15, 16):
        y = measurements(n, B, T)
        y[k, bad] = np.nan
        for ld in pitches(B):
            quad, lane = Pass(alg, n, B, ld, T, None), Pass(alg, n, B, ld, T, '0')
            try:
                q, l = quad.run(monkeypatch, y, True), lane.run(monkeypatch, y, True)
                what = 'N = %d, NaN at step %d of trajectory %d, ld = %d' % (n, k, bad, ld)
                assert_same_bytes(q, l, what)
                assert l[2][bad] == (2 if k == 0 else 0), (what, l[2])
                assert not np.any(np.delete(q[2], bad)), (what, q[2])
            finally:
                quad.free()
                lane.free()


@pytest.mark.parametrize('n', sorted(POINTS))
def test_kernel_name(amd, monkeypatch, n):
    if not any(k in os.environ for k in ('SSMQ_FUSED_WSPLIT', 'SSMQ_NO_FUSED', 'SSMQ_NO_FASTPATH')):
        monkeypatch.delenv('SSMQ_FUSED_QUAD', raising=False)
    else:
        monkeypatch.setenv('SSMQ_FUSED_QUAD', '1')
    for B in BATCHES:
        assert gpqkf(n).kernel_name(B) == 'k_filter_ungm_quad<N=%d,SSMQ_FORM_BQ,TP=0>' % n
