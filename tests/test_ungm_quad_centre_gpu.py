"""The centre point of k_filter_ungm_quad's measurement transform (csrc/ssmq_filter_ungm_quad.hip), which may not change a stored
bit: a measurement transform whose first unit point is +0.0 (the host reads the handle's own points, by bits) evaluates that point
at the predictive mean itself instead of at fma(+0.0, L, m) - N = 3 with the unscented points.  N = 2 ('sr': no centre), N = 5 and
every handle whose first point is anything else - the same three points in another order, or -0.0 first - keep the body that
multiplies.  The shapes also cover every path of the time loop (both peeled steps, no trip, one, two and four trips), for any
change to how the loop requests its time-table entries.

The reference in every case is the one-lane kernel k_filter_fused<1, 1, N, N, ...> on the same inputs (SSMQ_FUSED_QUAD=0, forced as
in tests/test_ungm_quad_gpu.py), which shares none of this: `fm` and `fP` bit for bit wherever the reference holds a number, NaN in
the same places, `status` equal.

  clean runs       N = 2, 3, 5;  B = 1, 15, 16, 17, 65;  pitch = the batch rounded up to 64, and 64 more;
                   T = 1 (last step only), 2 (odd step and last), 3 (one trip), 4, 5 (two trips), 6, 9 (four trips)
  other points     N = 3: the measurement transform's points, after construction, in the orders (1, 0, 2) and (2, 1, 0) with the
                   weights moved along, and the unscented order with -0.0 first
  planted failures a NaN and a +Inf measurement at each of steps 0, 1, T - 2, T - 1, an initial variance of 0, -1 and +Inf, each on
                   the trajectories at places 0 and 15 of the first and of the last full wave (B = 65), T = 5 and 6; pass r gives
                   the i-th of those trajectories plant (r + i) mod 11, so every one meets every plant.  The reference shows every
                   plant: a non-zero status - all but a measurement planted at the LAST step, whose covariance does not depend on
                   it (status 0, tests/test_ungm_quad_status_gpu.py), and a +Inf measurement, which that file allows a 0 too -,
                   or where the status is 0 a stored mean that is not a number.  The comparison leaves nothing out.
  guards           `y`, `fm`, `fP` and `status` lie between canary planes (and the padding of every plane is canary) which hold
                   after every pass, `y` itself included; the last pass of a shape runs twice into the same buffers.
                   The time table's device copy is a segment of the library's own per-context constants block (scale | table |
                   the measurement's table | step numbers), which no entry point hands out: the test cannot put canaries around
                   it.  The kernel only reads it; an entry read from the wrong place shows as a wrong bit in the step that uses it.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

POINTS = {2: ('sr', None), 3: ('ut', None), 5: ('gh', {'degree': 5})}
BATCHES = (1, 15, 16, 17, 65)
STEPS = (1, 2, 3, 4, 5, 6, 9)
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


def make_gpqkf(n):
    from ssmtoybox_amd import ssinf, ssmod as sm
    dyn = sm.UNGMTransition(sm.GaussRV(1), sm.GaussRV(1, cov=np.array([[10.0]])))
    obs = sm.UNGMMeasurement(sm.GaussRV(1), 1)
    par = np.array([[1.0, 3.0]])
    pts, hyp = POINTS[n]
    alg = ssinf.GaussianProcessKalman(dyn, obs, par, par, 'rbf', pts, hyp)
    assert alg.tf_dyn.model.points.shape[1] == n and alg.tf_obs.model.points.shape[1] == n
    return alg


def gpqkf(n):
    """The GPQ-Kalman filter on UNGM with n points: made once."""
    if n not in _ALGS:
        _ALGS[n] = make_gpqkf(n)
    return _ALGS[n]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def measurements(n, B, T):
    return 3.0 * np.random.default_rng(7000 * n + 10 * B + T).standard_normal((T, B))


class Buffers:
    """Device blocks for the passes of one test, big enough for its largest shape: y, fm, fP as [T + 2][ld] and status as [3][ld],
    each with a canary plane before and behind what a pass owns; m0, P0 [ld]."""

    def __init__(self, T_max, ld_max):
        from ssmtoybox_amd import _lib
        n = 8 * (T_max + 2) * ld_max
        self.d_y, self.d_fm, self.d_fP = _lib.DeviceBuffer(n), _lib.DeviceBuffer(n), _lib.DeviceBuffer(n)
        self.d_st, self.d_m0, self.d_P0 = _lib.DeviceBuffer(4 * 3 * ld_max), _lib.DeviceBuffer(8 * ld_max), _lib.DeviceBuffer(8 * ld_max)
        self.shape = None

    def run(self, monkeypatch, alg, n, mode, B, ld, T, y, P0=None):
        """One `ssmq_filter_forward_dev` pass on route `mode` (None: the default route, the quad kernel; '0': one lane):
        (fm (T, B), fP (T, B), status (B,)) as stored, every canary checked.  A new shape starts from canaries; the same shape
        again goes into what the pass before left."""
        from ssmtoybox_amd import _lib
        if mode is None and not any(k in os.environ for k in ('SSMQ_FUSED_WSPLIT', 'SSMQ_NO_FUSED', 'SSMQ_NO_FASTPATH')):
            monkeypatch.delenv('SSMQ_FUSED_QUAD', raising=False)         # the default route
        else:
            monkeypatch.setenv('SSMQ_FUSED_QUAD', mode or '1')
        kn = alg.kernel_name(B, ld, T)
        assert kn.startswith('k_filter_fused<D=1,Y=1,ND=%d,' % n if mode == '0' else 'k_filter_ungm_quad<N=%d,' % n), kn
        what = 'N = %d, B = %d, T = %d, ld = %d, SSMQ_FUSED_QUAD = %s' % (n, B, T, ld, mode)
        first = self.shape != (B, ld, T)
        if first:
            self.shape = (B, ld, T)
            canaries = np.full((T + 2, ld), CANARY)
            self.d_fm.upload(canaries)
            self.d_fP.upload(canaries)
            self.d_st.upload(np.full(3 * ld, ST_CANARY, dtype=np.int32))
            self.d_m0.upload(np.full(ld, float(np.atleast_1d(alg.x0_mean).ravel()[0])))
        planes = np.full((T + 2, ld), CANARY)
        planes[1:T + 1] = 0.0
        planes[1:T + 1, :B] = y
        self.d_y.upload(planes)
        p0 = np.ones(ld)
        if P0 is not None:
            p0[:B] = P0
        self.d_P0.upload(p0)
        alg._launch(_lib.load(), B, ld, T, self.d_y.view(8 * ld), self.d_m0, self.d_P0, self.d_fm.view(8 * ld), self.d_fP.view(8 * ld),
                    self.d_st.view(4 * ld))
        _lib.sync()
        assert self.d_y.download((T + 2, ld)).tobytes() == planes.tobytes(), what + ': y or the planes around it were written'
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
        for b in (self.d_y, self.d_fm, self.d_fP, self.d_st, self.d_m0, self.d_P0):
            b.free()


def assert_same(q, l, what):
    """fm, fP: NaN where the reference is NaN and nowhere else, the reference's bits everywhere else; status equal."""
    for name, u, v in zip(('filtered means', 'covariances'), q, l):
        assert u.shape == v.shape, (what, name)
        assert np.array_equal(np.isnan(u), np.isnan(v)), '%s: %s: NaN at other places' % (what, name)
        num = ~np.isnan(v)
        assert np.array_equal(bits(u)[num], bits(v)[num]), '%s: %s differ in %d of %d entries' % (
            what, name, int(np.sum(bits(u)[num] != bits(v)[num])), u.size)
    assert np.array_equal(q[2], l[2]), '%s: status: quad %s, one lane %s' % (what, q[2], l[2])


def both_routes(monkeypatch, alg, n, B, T, y, P0=None, clean=True):
    """The quad route against the one-lane route at both pitches; the quad pass once more into the buffers it has just filled."""
    from ssmtoybox_amd import _lib
    for ld in (_lib.padded(B), _lib.padded(B) + 64):
        quad, lane = Buffers(T, ld), Buffers(T, ld)
        try:
            what = 'N = %d, B = %d, T = %d, ld = %d' % (n, B, T, ld)
            q = quad.run(monkeypatch, alg, n, None, B, ld, T, y, P0)
            l = lane.run(monkeypatch, alg, n, '0', B, ld, T, y, P0)
            assert_same(q, l, what)
            if clean:
                assert not np.any(l[2]), (what, l[2])
                assert np.all(np.isfinite(l[0])) and np.all(np.isfinite(l[1])), what
            assert_same(quad.run(monkeypatch, alg, n, None, B, ld, T, y, P0), q, what + ', second pass')
        finally:
            quad.free()
            lane.free()


@pytest.mark.parametrize('B', BATCHES)
@pytest.mark.parametrize('n', sorted(POINTS))
def test_clean_runs_give_the_bits_of_the_one_lane_kernel(amd, monkeypatch, n, B):
    alg = gpqkf(n)
    for T in STEPS:
        both_routes(monkeypatch, alg, n, B, T, measurements(n, B, T))


def test_unscented_points_start_with_plus_zero(amd):
    """What sends the N = 3 filter to the centre-point body: the first unit point of its measurement transform is +0.0 by bits."""
    xi = np.ascontiguousarray(gpqkf(3).tf_obs.model.points, dtype=np.float64)
    assert xi.shape == (1, 3) and bits(xi)[0, 0] == 0, xi


@pytest.mark.parametrize('first', ('order 1 0 2', 'order 2 1 0', 'minus zero'))
def test_a_first_point_that_is_not_plus_zero_keeps_the_body_that_multiplies(amd, monkeypatch, first):
    """The measurement transform's points replaced after construction (the handle is updated at the next pass).  The kernel keeps
    its name; what it computes must still be the one-lane kernel's bits on the same handle."""
    n = 3
    alg = make_gpqkf(n)
    tf = alg.tf_obs
    xi = np.array(tf.model.points, dtype=np.float64)
    if first == 'minus zero':
        assert bits(xi)[0, 0] == 0
        xi[0, 0] = -0.0
        assert bits(xi)[0, 0] == 1 << 63
    else:
        p = [int(c) for c in first.split()[1:]]
        xi = np.ascontiguousarray(xi[:, p])
        tf.wm = np.ascontiguousarray(np.asarray(tf.wm)[p])
        tf.Wc = np.ascontiguousarray(np.asarray(tf.Wc)[np.ix_(p, p)])
        tf.Wcc = np.ascontiguousarray(np.asarray(tf.Wcc)[:, p])
        assert bits(xi)[0, 0] != 0
    tf.model.points = xi
    for B in (17, 65):
        for T in (1, 2, 5, 6):
            both_routes(monkeypatch, alg, n, B, T, measurements(n, B, T))


def plants(T):
    """What a trajectory can be given: (kind, step or initial variance)."""
    steps = (0, 1, T - 2, T - 1)
    return [('nan', k) for k in steps] + [('inf', k) for k in steps] + [('P0', 0.0), ('P0', -1.0), ('P0', np.inf)]


@pytest.mark.parametrize('T', (5, 6))
@pytest.mark.parametrize('n', sorted(POINTS))
def test_planted_failures_give_the_bits_and_the_status_of_the_one_lane_kernel(amd, monkeypatch, n, T):
    from ssmtoybox_amd import _lib
    B = 65
    places = (0, 15, 48, 63)            # places 0 and 15 of the first and of the last full wave of 16 trajectories
    alg = gpqkf(n)
    menu = plants(T)
    assert len(menu) == 11 and len({k for kind, k in menu if kind != 'P0'}) == 4
    y0 = measurements(n, B, T)
    for ld in (_lib.padded(B), _lib.padded(B) + 64):
        quad, lane = Buffers(T, ld), Buffers(T, ld)
        try:
            for r in range(len(menu)):
                what = 'N = %d, T = %d, ld = %d, pass %d' % (n, T, ld, r)
                y, P0, given = y0.copy(), np.ones(B), {}
                for i, b in enumerate(places):
                    kind, v = given[b] = menu[(r + i) % len(menu)]
                    if kind == 'P0':
                        P0[b] = v
                    else:
                        y[v, b] = np.nan if kind == 'nan' else np.inf
                q = quad.run(monkeypatch, alg, n, None, B, ld, T, y, P0)
                l = lane.run(monkeypatch, alg, n, '0', B, ld, T, y, P0)
                assert_same(q, l, what)
                # the reference shows every plant, and nobody else fails
                for b in range(B):
                    if b not in given:
                        assert l[2][b] == 0 and np.all(np.isfinite(l[0][:, b])) and np.all(np.isfinite(l[1][:, b])), (what, b, l[2][b])
                        continue
                    kind, v = given[b]
                    if kind == 'P0':
                        assert l[2][b] == 1, (what, b, given[b], l[2][b])
                    elif kind == 'nan' and v + 1 < T:
                        assert l[2][b] == v + 2, (what, b, given[b], l[2][b])
                    else:
                        assert l[2][b] != 0 or not np.all(np.isfinite(l[0][:, b])), (what, b, given[b], l[2][b])
                if r == len(menu) - 1:
                    assert_same(quad.run(monkeypatch, alg, n, None, B, ld, T, y, P0), q, what + ', repeated')
        finally:
            quad.free()
            lane.free()
