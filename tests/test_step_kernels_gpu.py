"""The two step kernels under every filter and smoother, called directly through their public C entry points and pinned per
instantiation against the 50-digit restatements of tests/_step_oracle.py:

  ssmq_kalman_update_dev  k_kalman_update<D, Y> for the eight table pairs, k_kalman_update_generic for every other shape
  ssmq_rts_backward_dev   k_rts_backward<D>, D = 1..7

Bound: max(RTOL, 64 cond eps), the project's bound for one application of an inverse, componentwise and per item against the
oracle's scales (sum of the absolute values of the terms of each update); cond = cond(P_y) of the item, or max_k cond(pP[k]) of the
lane times the T - 2 recursion steps (gains of norm <= 0.9: per-step errors add and do not grow).  The low-condition sets drop the
RTOL floor.  tests/test_step_kernels_host.py shows that float64 NumPy meets the same bound on the same cases.

Shapes: B = 130 at pitch 192 (two full 64-lane blocks and a partial one, ld > B), B = 1 / 63 / 64 / 65 at ld = B and B + 7 around
the block size, T = 1, 2, 3 at the edges of the smoother's indexing; a distinct random item per lane, so a lane-indexing error gives
a wrong answer and not the same one.

Covered only through filter passes, because they are not arguments of the public calls: the merging of the transforms' status words
(st_a / st_b), a nonzero `step`, the Studentian rescaling (smat_out), and Dx > D / c_cols > D (cross-covariances of noise-augmented
states) - Student goldens, UNGMNA and CTRS non-additive goldens, the launch-loop tests."""
import ctypes

import numpy as np
import pytest

from tests import _step_oracle as so
from tests._cases import within

pytestmark = pytest.mark.gpu

OK, E_ARG, E_UNSUPPORTED = 0, -1, -3
SENT = -7.0259e+211                  # sentinel of the output planes and of the padding lanes
ST_SENT = 0x5A5A5A5A                 # sentinel of the status plane
UPD_LD, RTS_LD = 192, 96


@pytest.fixture(scope='module')
def amd():
    import ssmtoybox_amd
    if ssmtoybox_amd.device_count() < 1:
        pytest.fail('no device: the GPU tests need an MI355X')
    ssmtoybox_amd.set_device(0)
    return ssmtoybox_amd


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


class Planes:
    """Device buffers of one call, freed together."""

    def __init__(self):
        from ssmtoybox_amd import _lib
        self._lib, self.bufs = _lib, []

    def up(self, host):
        buf = self._lib.DeviceBuffer(host.nbytes)
        buf.upload(host)
        self.bufs.append(buf)
        return buf

    def free(self):
        for b in self.bufs:
            b.free()


def soa(a, ld, lead=0):
    """Item-first (B, n...) -> planes (n, ld) (lead = 0) or, for sequences (B, n..., T), (T, n, ld); padding lanes hold SENT."""
    a = np.asarray(a, dtype=float)
    B = a.shape[0]
    if lead:
        T = a.shape[-1]
        out = np.full((T, int(np.prod(a.shape[1:-1])), ld), SENT)
        out[:, :, :B] = np.moveaxis(a, -1, 0).reshape(T, B, -1).transpose(0, 2, 1)
        return out
    out = np.full((int(np.prod(a.shape[1:])), ld), SENT)
    out[:, :B] = a.reshape(B, -1).T
    return out


def ptr(b):
    return None if b is None else ctypes.c_void_p(b.ptr)


# ---- measurement update --------------------------------------------------------------------------------------------------------
def run_update(amd, D, Y, c, B, ld, inplace=False, status=None):
    """The entry point on the first B items of a case at pitch ld.  Returns m (B, D), P (B, D, D) and the raw planes m (D, ld),
    P (D D, ld), status (ld,) - outputs and status pre-filled with sentinels."""
    from ssmtoybox_amd import _lib
    lib, pl = _lib.load(), Planes()
    try:
        ins = [pl.up(soa(c[k][:B], ld)) for k in ('m_pr', 'P_pr', 'y_mean', 'P_y', 'P_yx', 'y')]
        d_m = ins[0] if inplace else pl.up(np.full((D, ld), SENT))
        d_P = ins[1] if inplace else pl.up(np.full((D * D, ld), SENT))
        d_st = pl.up(np.full(ld, ST_SENT, dtype=np.int32) if status is None else status)
        _lib.check(lib.ssmq_kalman_update_dev(D, Y, B, ld, *(ptr(b) for b in ins), ptr(d_m), ptr(d_P), ptr(d_st)), 'ssmq_kalman_update_dev')
        _lib.check(lib.ssmq_sync(), 'ssmq_sync')
        m_raw, P_raw, st = d_m.download((D, ld)), d_P.download((D * D, ld)), d_st.download((ld,), dtype=np.int32)
    finally:
        pl.free()
    return m_raw[:, :B].T.copy(), P_raw[:, :B].T.reshape(B, D, D).copy(), m_raw, P_raw, st


def check_update(what, m, P, ref, cond, floor, lanes=None):
    rm, rP, m_sc, P_sc = ref
    sel = slice(0, m.shape[0]) if lanes is None else lanes
    a = so.ratio(m[sel], rm[sel], m_sc[sel], cond[sel], floor)
    b = so.ratio(P[sel], rP[sel], P_sc[sel], cond[sel], floor)
    print('%s: device / (cond eps): mean %.3g cov %.3g' % (what, a, b))
    assert within(a, so.FACTOR, 'step dev update mean ' + what), (what, a)
    assert within(b, so.FACTOR, 'step dev update cov ' + what), (what, b)


@pytest.mark.parametrize('cset', sorted(so.UPDATE_CONDS))
@pytest.mark.parametrize('D,Y', so.TABLE_PAIRS + so.GENERIC_PAIRS)
def test_update_every_instantiation(amd, D, Y, cset):
    c, ref = so.update_table(D, Y, cset)
    m, P, m_raw, P_raw, st = run_update(amd, D, Y, c, so.UPD_B, UPD_LD)
    assert np.all(st[:so.UPD_B] == 0) and np.all(st[so.UPD_B:] == ST_SENT)
    assert np.all(bits(m_raw[:, so.UPD_B:]) == bits(np.float64(SENT))) and np.all(bits(P_raw[:, so.UPD_B:]) == bits(np.float64(SENT)))
    check_update('(%d,%d) %s' % (D, Y, cset), m, P, ref, c['cond'], cset != 'lo')


@pytest.mark.parametrize('pad', (0, 7))
@pytest.mark.parametrize('B', (1, 63, 64, 65))
@pytest.mark.parametrize('D,Y', ((5, 2), (3, 3)))
def test_update_batch_edges(amd, D, Y, B, pad):
    c, ref = so.update_table(D, Y, 'lo')
    ld = B + pad
    m, P, m_raw, P_raw, st = run_update(amd, D, Y, c, B, ld)
    assert np.all(st[:B] == 0)
    assert np.all(st[B:] == ST_SENT)                                   # the entry point clears B status words, not ld
    assert np.all(bits(m_raw[:, B:]) == bits(np.float64(SENT))) and np.all(bits(P_raw[:, B:]) == bits(np.float64(SENT)))
    check_update('(%d,%d) B=%d ld=%d' % (D, Y, B, ld), m, P, ref, c['cond'], False, slice(0, B))


@pytest.mark.parametrize('D,Y', ((5, 4), (2, 1), (7, 3)))
def test_update_in_place(amd, D, Y):
    c, _ = so.update_table(D, Y, 'lo')
    m, P, _, _, st = run_update(amd, D, Y, c, so.UPD_B, UPD_LD)
    m2, P2, m_raw, P_raw, st2 = run_update(amd, D, Y, c, so.UPD_B, UPD_LD, inplace=True)
    assert np.array_equal(bits(m), bits(m2)) and np.array_equal(bits(P), bits(P2)) and np.array_equal(st, st2)
    assert np.all(bits(m_raw[:, so.UPD_B:]) == bits(np.float64(SENT))) and np.all(bits(P_raw[:, so.UPD_B:]) == bits(np.float64(SENT)))


@pytest.mark.parametrize('space', ('y', 'x'))
@pytest.mark.parametrize('p', (-200, -60, 60, 200))
@pytest.mark.parametrize('D,Y', ((2, 1), (5, 2), (5, 4), (3, 3)))
def test_update_scale_range(amd, D, Y, p, space):
    """The private division / square root far from O(1): the measurement space or the state space scaled by 2^p.  Scaling by a power
    of two is exact for the oracle (tests/test_step_kernels_host.py), so the reference and its scales are the table's, scaled."""
    c, (rm, rP, m_sc, P_sc) = so.update_table(D, Y, 'lo')
    s = 2.0 ** p if space == 'x' else 1.0
    m, P, _, _, st = run_update(amd, D, Y, so.scaled_update_case(c, p, space), so.UPD_B, UPD_LD)
    assert np.all(st[:so.UPD_B] == 0)
    check_update('(%d,%d) %s 2^%d' % (D, Y, space, p), m, P, (rm * s, rP * s * s, m_sc * s, P_sc * s * s), c['cond'], False)


@pytest.mark.parametrize('D,Y', ((1, 1), (2, 1), (3, 1)))
def test_update_quotient_is_faithful(amd, D, Y):
    """The Y = 1 shortcut shows the private quotient bit for bit: with m_pr = 0, y_mean = 0, y = 1 the filtered mean is
    0 + (P_yx / P_y) 1, the gain itself.  div_nr (ssmq_device.h) is one Newton round on the hardware reciprocal (relative error
    ~2^-48 from a 2^-24 seed), q = a r, and a residual correction q + (a - b q) r: the residual is exact in the fma, so the result
    is the exact quotient, off by ~2^-96 relative, rounded once - within one ulp for every operand, and correctly rounded unless
    the quotient sits that close to a rounding boundary.  Without the correction the error is up to ~2^-48 = 16 ulp, which the
    64 cond eps bound of the other tests cannot see (measured with the correction taken out: 6.7 to 9.1 ulp).  Table pairs only:
    the generic kernel has no Y = 1 shortcut, its gain goes through sqrt(P_y) twice and carries three roundings (measured 2.4 ulp).
    Operands over the declared range: P_y in 2^[-400, 400], P_yx in 2^[-50, 50], both signs of P_yx."""
    import mpmath as mp
    rng = np.random.default_rng([20244, D])
    B = so.UPD_B
    c = dict(m_pr=np.zeros((B, D)), P_pr=np.ones((B, D, D)), y_mean=np.zeros((B, 1)), y=np.ones((B, 1)),
             P_y=np.ldexp(rng.uniform(1.0, 2.0, (B, 1, 1)), rng.integers(-400, 401, (B, 1, 1))),
             P_yx=np.ldexp(rng.uniform(1.0, 2.0, (B, 1, D)), rng.integers(-50, 51, (B, 1, D))) * rng.choice([-1.0, 1.0], (B, 1, D)))
    m, _, _, _, st = run_update(amd, D, Y, c, B, UPD_LD)
    assert np.all(st[:B] == 0)
    with mp.workdps(so.DPS):
        ulps = max(float(abs(mp.mpf(float(m[b, d])) - mp.mpf(float(c['P_yx'][b, 0, d])) / mp.mpf(float(c['P_y'][b, 0, 0]))) /
                         mp.mpf(float(np.spacing(abs(m[b, d]))))) for b in range(B) for d in range(D))
    exact = int(np.sum(m == c['P_yx'][:, 0, :] / c['P_y'][:, 0, :]))
    print('(%d,1): quotient within %.3f ulp, %d of %d correctly rounded' % (D, ulps, exact, B * D))
    assert within(ulps, 1.0, 'step dev update quotient ulp (%d,1)' % D)


BAD_LANES = (3, 64, 69)


def bad_py(Y, kind):
    if Y == 1:
        return np.array([[{0: 0.0, 1: -2.5, 2: np.nan}[kind]]])
    S = np.eye(Y) * 3.0
    if kind == 0:
        S[0, 0] = 0.0                                                  # leading entry 0
    elif kind == 1:
        S[:2, :2] = [[1.0, 2.0], [2.0, 1.0]]                           # second pivot 1 - 4 < 0
    else:
        S[0, 0], S[1, 1] = 2.0, 2.5
        S[Y - 1, 0] = np.nan                                           # lower triangle only: the triangle the factorisation reads
    return S


@pytest.mark.parametrize('D,Y', ((2, 1), (16, 1), (5, 2), (5, 4), (7, 3)))
def test_update_not_positive_definite(amd, D, Y):
    B, ld = 70, 77
    c0, ref = so.update_table(D, Y, 'lo')
    c = {k: v[:B].copy() for k, v in c0.items()}
    for kind, lane in enumerate(BAD_LANES):
        c['P_y'][lane] = bad_py(Y, kind)
    m, P, _, _, st = run_update(amd, D, Y, c, B, ld)
    good = np.setdiff1d(np.arange(B), BAD_LANES)
    assert np.all(st[list(BAD_LANES)] == 1), st[list(BAD_LANES)]       # 1 + step, and the entry point runs as step 0
    assert np.all(np.isnan(m[list(BAD_LANES)])) and np.all(np.isnan(P[list(BAD_LANES)]))
    assert np.all(st[good] == 0) and np.all(st[B:] == ST_SENT)
    check_update('(%d,%d) beside bad lanes' % (D, Y), m, P, ref, c0['cond'], False, good)      # a bad neighbour does not leak


def test_update_refusals(amd):
    from ssmtoybox_amd import _lib
    lib, pl = _lib.load(), Planes()
    M, B, ld = 17, 5, 8
    try:
        ins = [pl.up(np.full((M * M, ld), 1.0)) for _ in range(6)]
        outs = [pl.up(np.full((M * M, ld), SENT)), pl.up(np.full((M * M, ld), SENT)), pl.up(np.full(ld, ST_SENT, dtype=np.int32))]
        p = [ptr(b) for b in ins + outs]

        def call(D, Y, B_, ld_, args=p):
            return lib.ssmq_kalman_update_dev(D, Y, B_, ld_, *args)
        assert call(0, 1, B, ld) == E_ARG and call(-1, 1, B, ld) == E_ARG
        assert call(2, 0, B, ld) == E_ARG and call(2, -3, B, ld) == E_ARG
        assert call(2, 1, -1, ld) == E_ARG
        assert call(2, 1, B, B - 1) == E_ARG
        for i in range(len(p)):
            assert call(2, 1, B, ld, p[:i] + [None] + p[i + 1:]) == E_ARG, i
        assert call(17, 1, B, ld) == E_UNSUPPORTED and call(1, 17, B, ld) == E_UNSUPPORTED and call(17, 17, B, ld) == E_UNSUPPORTED
        assert call(2, 1, 0, ld) == OK
        _lib.check(lib.ssmq_sync(), 'ssmq_sync')
        for b in outs[:2]:
            assert np.all(bits(b.download((M * M, ld))) == bits(np.float64(SENT)))       # nothing above reached the outputs
        assert np.all(outs[2].download((ld,), dtype=np.int32) == ST_SENT)                # ... nor the status words
    finally:
        pl.free()


def test_update_empty_batch_leaves_status(amd):
    from ssmtoybox_amd import _lib
    lib, pl = _lib.load(), Planes()
    try:
        ins = [pl.up(np.full((4, 8), 1.0)) for _ in range(6)]
        outs = [pl.up(np.full((4, 8), SENT)), pl.up(np.full((4, 8), SENT)), pl.up(np.full(8, ST_SENT, dtype=np.int32))]
        assert lib.ssmq_kalman_update_dev(2, 1, 0, 8, *(ptr(b) for b in ins + outs)) == OK
        assert lib.ssmq_kalman_update_dev(2, 1, 0, 0, *(ptr(b) for b in ins + outs)) == OK
        _lib.check(lib.ssmq_sync(), 'ssmq_sync')
        assert np.all(bits(outs[0].download((4, 8))) == bits(np.float64(SENT))) and np.all(bits(outs[1].download((4, 8))) == bits(np.float64(SENT)))
        assert np.all(outs[2].download((8,), dtype=np.int32) == ST_SENT)
    finally:
        pl.free()


# ---- RTS backward pass ---------------------------------------------------------------------------------------------------------
def run_rts(amd, D, c, B, ld, T, status=None, expect=OK):
    """The entry point on the first B lanes of a case.  Returns sm (B, D, T), sP (B, D, D, T), the raw planes and status (ld,)."""
    from ssmtoybox_amd import _lib
    lib, pl = _lib.load(), Planes()
    Ta = max(T, 1)
    try:
        ins = [pl.up(soa(c[k][:B], ld, lead=1) if T else np.full((1, c[k][0, ..., 0].size, ld), SENT)) for k in ('fm', 'fP', 'pm', 'pP', 'pC')]
        d_sm, d_sP = pl.up(np.full((Ta, D, ld), SENT)), pl.up(np.full((Ta, D * D, ld), SENT))
        d_st = pl.up(np.full(ld, ST_SENT, dtype=np.int32) if status is None else status)
        rc = lib.ssmq_rts_backward_dev(D, B, ld, T, *(ptr(b) for b in ins), ptr(d_sm), ptr(d_sP), ptr(d_st))
        assert rc == expect, (rc, _lib.last_error() if hasattr(_lib, 'last_error') else '')
        sm_raw, sP_raw, st = d_sm.download((Ta, D, ld)), d_sP.download((Ta, D * D, ld)), d_st.download((ld,), dtype=np.int32)
    finally:
        pl.free()
    sm = np.moveaxis(sm_raw[:, :, :B], 0, -1).transpose(1, 0, 2).copy()                                # (B, D, Ta)
    sP = np.moveaxis(sP_raw[:, :, :B], 0, -1).transpose(1, 0, 2).reshape(B, D, D, Ta).copy()
    return sm, sP, sm_raw, sP_raw, st


def check_rts(what, sm, sP, ref, cond, floor, T, lanes=None):
    rm, rP, m_sc, P_sc = ref
    sel = slice(0, sm.shape[0]) if lanes is None else lanes
    a = so.ratio(sm[sel], rm[sel], m_sc[sel], cond[sel], floor, T - 2)
    b = so.ratio(sP[sel], rP[sel], P_sc[sel], cond[sel], floor, T - 2)
    print('%s: device / (steps cond eps): mean %.3g cov %.3g' % (what, a, b))
    assert within(a, so.FACTOR, 'step dev rts mean ' + what), (what, a)
    assert within(b, so.FACTOR, 'step dev rts cov ' + what), (what, b)


def padding_untouched(B, raws, st):
    return all(np.all(bits(r[..., B:]) == bits(np.float64(SENT))) for r in raws) and bool(np.all(st[B:] == ST_SENT))


@pytest.mark.parametrize('cset', sorted(so.RTS_CONDS))
@pytest.mark.parametrize('D', so.RTS_DIMS)
def test_rts_every_dimension(amd, D, cset):
    """fP general, pP symmetric, pC = pP A' non-symmetric (the orientation of the gain, which D = 1 cannot see); elements 0 and T - 1 of
    pm, pP, pC are NaN - the reference's indexing never reads them."""
    c, ref = so.rts_table(D, cset)
    assert np.all(np.isnan(c['pP'][..., 0])) and np.all(np.isnan(c['pC'][..., so.RTS_T - 1]))
    st0 = np.zeros(RTS_LD, dtype=np.int32)
    st0[so.RTS_B:] = ST_SENT
    sm, sP, sm_raw, sP_raw, st = run_rts(amd, D, c, so.RTS_B, RTS_LD, so.RTS_T, status=st0)
    assert np.all(np.isfinite(sm)) and np.all(np.isfinite(sP))
    assert np.all(st[:so.RTS_B] == 0) and padding_untouched(so.RTS_B, (sm_raw, sP_raw), st)
    check_rts('D=%d %s' % (D, cset), sm, sP, ref, c['cond'], cset != 'lo', so.RTS_T)


@pytest.fixture(scope='module')
def edge_cases():
    out = {}
    for D in (2, 5):
        for T in (1, 2, 3):
            c = so.rts_case(np.random.default_rng([20243, D, T]), D, T, 65, 1e2)
            out[D, T] = (c, so.rts_ref(c))
    return out


@pytest.mark.parametrize('T', (1, 2, 3))
@pytest.mark.parametrize('D', (2, 5))
def test_rts_time_edges(amd, edge_cases, D, T):
    B, ld = 65, 72
    c, ref = edge_cases[D, T]
    st0 = np.zeros(ld, dtype=np.int32)
    st0[B:] = ST_SENT
    sm, sP, sm_raw, sP_raw, st = run_rts(amd, D, c, B, ld, T, status=st0)
    assert np.all(st[:B] == 0) and padding_untouched(B, (sm_raw, sP_raw), st)
    keep = slice(0, T) if T < 3 else slice(1, T)
    assert np.array_equal(bits(sm[..., keep]), bits(c['fm'][..., keep])) and np.array_equal(bits(sP[..., keep]), bits(c['fP'][..., keep]))
    if T == 3:
        assert not np.any(sm[..., 0] == c['fm'][..., 0])
        check_rts('D=%d T=3' % D, sm, sP, ref, c['cond'], False, T)


@pytest.mark.parametrize('D', (2, 5))
def test_rts_no_steps(amd, edge_cases, D):
    c, _ = edge_cases[D, 1]
    sm, sP, sm_raw, sP_raw, st = run_rts(amd, D, c, 65, 72, 0)
    assert padding_untouched(0, (sm_raw, sP_raw), st)                   # T = 0: SSMQ_OK and nothing written at all


@pytest.mark.parametrize('D', (2, 6))
def test_rts_status_word(amd, D):
    """The entry point ORs bit 30 into the status word where a predictive covariance the recursion reads is not positive definite, and
    clears nothing."""
    B, ld, T, k = so.RTS_B, RTS_LD, so.RTS_T, 2
    c0, ref = so.rts_table(D, 'lo')
    c = {n: v.copy() for n, v in c0.items()}
    bad = (5, 64, 66)
    c['pP'][5, 0, 0, k] = 0.0                                           # zero leading entry
    for lane in (64, 66):                                               # negative second pivot
        c['pP'][lane, :, :, k] = np.eye(D)
        c['pP'][lane, :2, :2, k] = [[1.0, 2.0], [2.0, 1.0]]
    st0 = np.full(ld, ST_SENT, dtype=np.int32)
    st0[:B] = 0
    st0[[5, 7, 66]] = 5
    sm, sP, sm_raw, sP_raw, st = run_rts(amd, D, c, B, ld, T, status=st0)
    good = np.setdiff1d(np.arange(B), bad)
    assert np.array_equal(st[list(bad)], st0[list(bad)] | (1 << 30)), st[list(bad)]
    assert np.array_equal(st[good], st0[good]) and padding_untouched(B, (sm_raw, sP_raw), st)
    last = slice(T - 2, T)
    assert np.array_equal(bits(sm[..., last]), bits(c['fm'][..., last])) and np.array_equal(bits(sP[..., last]), bits(c['fP'][..., last]))
    check_rts('D=%d beside bad lanes' % D, sm, sP, ref, c0['cond'], False, T, good)


def test_rts_refusals(amd):
    from ssmtoybox_amd import _lib
    lib, pl = _lib.load(), Planes()
    D, B, ld, T = 8, 5, 8, 4
    try:
        ins = [pl.up(np.full((T, D * D, ld), 1.0)) for _ in range(5)]
        outs = [pl.up(np.full((T, D * D, ld), SENT)), pl.up(np.full((T, D * D, ld), SENT)), pl.up(np.full(ld, ST_SENT, dtype=np.int32))]
        p = [ptr(b) for b in ins + outs]
        assert lib.ssmq_rts_backward_dev(8, B, ld, T, *p) == E_UNSUPPORTED
        assert lib.ssmq_rts_backward_dev(0, B, ld, T, *p) == E_ARG and lib.ssmq_rts_backward_dev(-2, B, ld, T, *p) == E_ARG
        assert lib.ssmq_rts_backward_dev(2, B, ld, -1, *p) == E_ARG
        assert lib.ssmq_rts_backward_dev(2, B, B - 1, T, *p) == E_ARG
        assert lib.ssmq_rts_backward_dev(2, -1, ld, T, *p) == E_ARG
        for i in range(len(p)):
            assert lib.ssmq_rts_backward_dev(2, B, ld, T, *(p[:i] + [None] + p[i + 1:])) == E_ARG, i
        assert lib.ssmq_rts_backward_dev(2, 0, ld, T, *p) == OK
        for b in outs[:2]:
            assert np.all(bits(b.download((T, D * D, ld))) == bits(np.float64(SENT)))
        assert np.all(outs[2].download((ld,), dtype=np.int32) == ST_SENT)
    finally:
        pl.free()
