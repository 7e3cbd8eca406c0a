"""The status word of k_filter_ungm_quad (csrc/ssmq_filter_ungm_quad.hip).  Its time loop keeps no failure count: behind the loop
a trajectory whose last covariance is a number gets status 0, and a wave that holds a failed one reads the covariances it stored
back - step 0 .. T - 1 - and the first NaN at step k gives status k + 1.  That must be the status of the one-lane kernel
k_filter_fused<1, 1, N, N, ...> (SSMQ_FUSED_QUAD=0), which counts in its loop, for every input - and the read-back must leave
every stored bit alone.  The default route (the quad kernel for these batches) against SSMQ_FUSED_QUAD=0, forced as in
tests/test_ungm_quad_gpu.py; `fm` and `fP` compared as bits, `status` for equality.

  N = 2, 3, 5;  T = 1 .. 5 (both parities of the two-step loop and the peeled last step);  B = 1, 15, 16, 17, 65;
  ld = the batch rounded up to 64, and 64 more.

Failures are PLANTED, each at every step in turn: a measurement of NaN at step k, a measurement of +Inf at step k (the mean of step
k is lost, the covariance of step k + 1 with it: status k + 2, or 0 when k is the last step - the covariance does not depend on
the step's own measurement), and an initial variance of 0 or -1 (status 1).  They sit on the trajectories of quad 0, the middle
of a wave (6, 7), the last quad of a wave (15, 31), the first of the next (16), further waves (40) and the end of the last,
partly filled wave (B - 2, B - 1); every other trajectory of those waves is healthy.  One shape runs 2 T + 2 passes; in pass r the
i-th of those trajectories gets plant (r + i) mod (2 T + 2), so every one of them meets every plant, the failing trajectories of
one wave fail at different steps, and - all passes of a shape go into the SAME buffers - each pass finds the previous pass's NaNs
at other steps of the planes it reads back.  `fm`, `fP` and `status` lie between canary planes (one before, one behind, and the
padding of every plane), which must hold after every pass."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

POINTS = {2: ('sr', None), 3: ('ut', None), 5: ('gh', {'degree': 5})}
BATCHES = (1, 15, 16, 17, 65)
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


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def failing_positions(B):
    return sorted({b for b in (0, 6, 7, 15, 16, 31, 40, B - 2, B - 1) if 0 <= b < B})


def plants(T):
    """What a trajectory can be given: (kind, step or initial variance)."""
    return [('nan', k) for k in range(T)] + [('inf', k) for k in range(T)] + [('P0', 0.0), ('P0', -1.0)]


def expected_status(plant, T):
    kind, v = plant
    if kind == 'P0':
        return 1
    return v + 2 if v + 1 < T else 0


class Pass:
    """The buffers of one route for one shape: y [T][ld], m0 / P0 [ld], and fm, fP ([T + 2][ld]) and status ([3][ld]) with a
    canary plane before and behind what the kernels own.  Allocated once, every pass of the shape goes into them."""

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

    def run(self, monkeypatch, y, P0, first):
        """One `ssmq_filter_forward_dev` call: (fm (T, B), fP (T, B), status (B,)), the canaries checked."""
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
        p0 = np.ones(ld)
        p0[:B] = P0
        self.d_P0.upload(p0)
        self.alg._launch(_lib.load(), B, ld, T, self.d_y, self.d_m0, self.d_P0, self.d_fm.view(8 * ld), self.d_fP.view(8 * ld),
                         self.d_st.view(4 * ld))
        _lib.sync()
        what = 'N = %d, B = %d, T = %d, ld = %d, SSMQ_FUSED_QUAD = %s' % (n, B, T, ld, self.mode)
        out = []
        for name, buf in (('fm', self.d_fm), ('fP', self.d_fP)):
            blk = buf.download((T + 2, ld))
            assert np.all(bits(blk[0]) == bits(CANARY)), '%s: %s: the plane before step 0 was written' % (what, name)
            assert np.all(bits(blk[T + 1]) == bits(CANARY)), '%s: %s: the plane behind the last step was written' % (what, name)
            assert np.all(bits(blk[1:T + 1, B:]) == bits(CANARY)), '%s: %s: the padding of a plane was written' % (what, name)
            if first:
                assert not np.any(bits(blk[1:T + 1, :B]) == bits(CANARY)), '%s: %s: a result was not written' % (what, name)
            out.append(blk[1:T + 1, :B].copy())
        st = self.d_st.download((3, ld), dtype=np.int32)
        assert np.all(st[0] == ST_CANARY) and np.all(st[2] == ST_CANARY) and np.all(st[1, B:] == ST_CANARY), what + ': status canaries'
        out.append(st[1, :B].copy())
        return out

    def free(self):
        for b in (self.d_y, self.d_m0, self.d_P0, self.d_fm, self.d_fP, self.d_st):
            b.free()


def assert_same_bits(a, b, what):
    for name, u, v in zip(('filtered means', 'covariances', 'status'), a, b):
        assert u.shape == v.shape, (what, name)
        same = np.array_equal(bits(u), bits(v)) if u.dtype == np.float64 else np.array_equal(u, v)
        assert same, '%s: %s differ: quad %s, one lane %s' % (what, name, u[..., :8], v[..., :8]) if u.dtype != np.float64 else \
            '%s: %s differ in %d of %d entries' % (what, name, int(np.sum(bits(u) != bits(v))), u.size)


@pytest.mark.parametrize('B', BATCHES)
@pytest.mark.parametrize('n', sorted(POINTS))
def test_planted_failures_leave_the_status_of_the_one_lane_kernel(amd, monkeypatch, n, B):
    from ssmtoybox_amd import _lib
    alg = gpqkf(n)
    fail = failing_positions(B)
    for T in STEPS:
        menu = plants(T)
        for ld in (_lib.padded(B), _lib.padded(B) + 64):
            y0 = 3.0 * np.random.default_rng(1000 * n + 10 * T + B).standard_normal((T, B))
            quad, lane = Pass(alg, n, B, ld, T, None), Pass(alg, n, B, ld, T, '0')
            try:
                for r in range(len(menu)):
                    what = 'N = %d, B = %d, T = %d, ld = %d, pass %d' % (n, B, T, ld, r)
                    y, P0, given = y0.copy(), np.ones(B), {}
                    for i, b in enumerate(fail):
                        kind, v = given[b] = menu[(r + i) % len(menu)]
                        if kind == 'P0':
                            P0[b] = v
                        else:
                            y[v, b] = np.nan if kind == 'nan' else np.inf
                    q = quad.run(monkeypatch, y, P0, r == 0)
                    l = lane.run(monkeypatch, y, P0, r == 0)
                    assert_same_bits(q, l, what)
                    # the plants do what this file says they do (on the one-lane kernel), and nobody else fails
                    st = l[2]
                    for b in range(B):
                        want = expected_status(given[b], T) if b in given else 0
                        if b in given and given[b][0] == 'inf':          # (an infinite mean: lost at the next step in all but name)
                            assert st[b] in (want, 0), (what, b, given[b], st[b])
                        else:
                            assert st[b] == want, (what, b, given.get(b), st[b])
                    # the same pass once more into the buffers it has just filled: the same bits
                    if r == len(menu) - 1:
                        assert_same_bits(quad.run(monkeypatch, y, P0, False), q, what + ', repeated')
            finally:
                quad.free()
                lane.free()


def test_failing_steps_of_one_wave_differ(amd):
    """What the passes above give the trajectories of the first wave: at least two different failing steps in one pass."""
    for T in STEPS[1:]:
        menu = plants(T)
        fail = [b for b in failing_positions(65) if b < 16]
        for r in range(len(menu)):
            steps = {expected_status(menu[(r + i) % len(menu)], T) for i in range(len(fail))}
            assert len(steps) >= 2, (T, r, steps)
