"""The posterior Cramer-Rao bound without a device: the finaliser (ssmq_pcrlb_finalize, host code) against the 50-digit twin of
tests/_pcrlb_oracle.py and against the Kalman filter's Riccati recursion, its status, every refusal through the C ABI and Python, and
the compile check of the run-time kernels for gfx950."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import _pcrlb_oracle as po
from tests import _user_jac_oracle as uj
from tests._cases import RTOL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_UNSUPPORTED = -1, -3
GAUSS, STUDENT, MIXTURE = 0, 1, 2
# (case, output, bound): bounds beyond the rule of test_finalize_against_the_50_digit_twin, each 4 x the float64 restatement's own
# error against the twin - none was needed
MEASURED = ()


def _rv(kind, L, dof=0.0):
    from ssmtoybox_amd import _lib
    L = np.ascontiguousarray(L, dtype=np.float64)
    d = _lib.Rv()
    d.kind, d.dim, d.n_comp, d.dof = kind, L.shape[-1], 1, dof
    d.mean, d.chol = None, L.ctypes.data_as(_lib.c_double_p)
    alpha = np.ones(1)
    d.alpha = alpha.ctypes.data_as(_lib.c_double_p) if kind == MIXTURE else None
    return d, (L, alpha)


def _finalize(D, T, B_total, sums, P0, Q, G=None):
    """ssmq_pcrlb_finalize itself: (rc, info (D, D, T), bound (D, D, T), rmse (T,), status)."""
    from ssmtoybox_amd import _lib
    q, keep = _rv(GAUSS, np.linalg.cholesky(np.atleast_2d(Q)))
    sums, P0 = np.ascontiguousarray(sums, dtype=np.float64), np.ascontiguousarray(P0, dtype=np.float64)
    Gc = None if G is None else np.ascontiguousarray(G, dtype=np.float64)
    info, bound, rmse = np.full((T, D, D), -7.0), np.full((T, D, D), -7.0), np.full(T, -7.0)
    status = ctypes.c_int32(-7)
    rc = _lib.load().ssmq_pcrlb_finalize(D, T, B_total, _lib.dp(sums), _lib.dp(P0), ctypes.byref(q), _lib.dp(Gc), _lib.dp(info), _lib.dp(bound),
                                         _lib.dp(rmse), ctypes.byref(status))
    return rc, info.transpose(1, 2, 0), bound.transpose(1, 2, 0), rmse, status.value


def test_symbols():
    from ssmtoybox_amd import _lib
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'ssmq.h')).read(), flags=re.S)
    lib = _lib.load()
    for name in ('ssmq_pcrlb_sums_dev', 'ssmq_pcrlb_sums_width', 'ssmq_pcrlb_kernel_name', 'ssmq_pcrlb_finalize'):
        assert re.search(r'\b' + name + r'\s*\(', hdr), name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert re.search(r'SSMQ_RTC_PCRLB_DYN\s*=\s*9\s*,\s*SSMQ_RTC_PCRLB_OBS\s*=\s*10', hdr)
    assert [lib.ssmq_pcrlb_sums_width(D) for D in (1, 2, 6)] == [3, 10, 78] == [po.width(D) for D in (1, 2, 6)]
    assert lib.ssmq_pcrlb_sums_width(0) == E_ARG and lib.ssmq_pcrlb_sums_width(7) == E_ARG


@pytest.mark.parametrize('name', ['ungm', 'pendulum', 'six'])
def test_finalize_against_the_50_digit_twin(name):
    """The bar: RTOL, relative to the largest entry of each output, times the condition number of the worst J_{j-1} + D11_j the twin
    meets."""
    p = po.pair(name)
    T, B = 5, 24
    s, _ = po.sums(p, po.states(p, T, B))
    rc, info, bound, rmse, status = _finalize(p.D, T, B, s, p.P0, p.Q)
    assert rc == 0 and status == 0
    xi, xb, xr, cond = po.recursion_mp(s, B, p.P0, p.Q)
    ni, nb, nr, nst = po.recursion(s, B, p.P0, p.Qi)
    assert nst == 0
    extra = {(c, o): v for c, o, v in MEASURED}
    for what, got, own, ref in (('info', info, ni, xi), ('bound', bound, nb, xb), ('rmse_bound', rmse, nr, xr)):
        scale = np.max(np.abs(ref))
        err, own_err = np.max(np.abs(got - ref)) / scale, np.max(np.abs(own - ref)) / scale
        print('%s %s: error %.3g (the NumPy restatement %.3g), bar %.3g, cond %.3g' % (name, what, err, own_err, RTOL * cond, cond))
        assert err <= max(RTOL * cond, extra.get((name, what), 0.0)), (name, what, err)
        assert np.array_equal(got, np.swapaxes(got, 0, 1)) if got.ndim == 3 else True      # both triangles from one value


def _linear_case(D, Y, seed):
    rng = np.random.default_rng(seed)
    F = 0.9 * np.linalg.qr(rng.standard_normal((D, D)))[0] + 0.05 * rng.standard_normal((D, D))
    H = rng.standard_normal((Y, D))
    a, c, e = rng.standard_normal((D, D)), rng.standard_normal((Y, Y)), rng.standard_normal((D, D))
    return F, H, 0.2 * a.dot(a.T) + 0.1 * np.eye(D), 0.3 * c.dot(c.T) + 0.2 * np.eye(Y), 0.5 * e.dot(e.T) + 0.5 * np.eye(D)


@pytest.mark.parametrize('D,Y', [(2, 1), (4, 2)])
def test_riccati_property(D, Y):
    """For a linear pair (F, H constant, any states) J_j^-1 is the Kalman filter's covariance - through ssmq_pcrlb_finalize alone, at the
    bar of the twin test."""
    F, H, Q, R, P0 = _linear_case(D, Y, 10 * D + Y)
    T, B = 8, 37
    s = po.linear_sums(F, H, np.linalg.inv(Q), np.linalg.inv(R), T, B)
    rc, info, bound, rmse, status = _finalize(D, T, B, s, P0, Q)
    assert rc == 0 and status == 0
    cond = po.recursion_mp(s, B, P0, Q)[3]
    P = po.riccati(F, H, Q, R, P0, T)
    err = np.max(np.abs(bound - P)) / np.max(np.abs(P))
    print('D = %d, Y = %d: error %.3g, bar %.3g (cond %.3g)' % (D, Y, err, RTOL * cond, cond))
    assert err <= RTOL * cond
    tr = np.sqrt(np.einsum('iit->t', P))
    assert np.max(np.abs(rmse - tr)) <= RTOL * cond * np.max(tr)
    # the noise gain enters through G Q G'
    G = np.linalg.qr(np.random.default_rng(3).standard_normal((D, D)))[0] + 0.1
    rc, _, bound_g, _, status = _finalize(D, T, B, po.linear_sums(F, H, np.linalg.inv(G.dot(Q).dot(G.T)), np.linalg.inv(R), T, B), P0, Q, G)
    Pg = po.riccati(F, H, G.dot(Q).dot(G.T), R, P0, T)
    assert rc == 0 and status == 0 and np.max(np.abs(bound_g - Pg)) <= RTOL * po.recursion_mp(s, B, P0, G.dot(Q).dot(G.T))[3] * np.max(np.abs(Pg))


def test_status():
    p = po.pair('pendulum')
    T, B = 5, 24
    s, _ = po.sums(p, po.states(p, T, B))
    good = _finalize(p.D, T, B, s, p.P0, p.Q)
    assert good[0] == 0 and good[4] == 0 and all(np.all(np.isfinite(a)) for a in good[1:4])
    bad = s.copy()
    bad[2, 4] = np.nan
    rc, info, bound, rmse, status = _finalize(p.D, T, B, bad, p.P0, p.Q)
    assert rc == 0 and status == 3
    for got, ref in ((info, good[1]), (bound, good[2]), (rmse, good[3])):
        assert np.array_equal(got[..., :2], ref[..., :2]) and np.all(np.isnan(got[..., 2:]))
    bad[2, 4] = np.inf
    assert _finalize(p.D, T, B, bad, p.P0, p.Q)[4] == 3
    # an information matrix that loses positive definiteness: sums of F' Qi F that are hugely negative at step 1
    bad = s.copy()
    bad[1, 0] = -1e30
    assert _finalize(p.D, T, B, bad, p.P0, p.Q)[4] == 2
    rc, info, bound, rmse, status = _finalize(p.D, T, B, s, np.array([[1.0, 2.0], [2.0, 1.0]]), p.Q)      # an indefinite P0
    assert rc == 0 and status == 1 and all(np.all(np.isnan(a)) for a in (info, bound, rmse))
    # Python: the same through finalize_crlb
    from ssmtoybox_amd import mcshard, ssmod as sm
    dyn, _ = p.models()
    out = mcshard.finalize_crlb(s, dyn, B)
    assert out['status'] == 0 and out['info'].shape == (2, 2, T) and out['rmse_bound'].shape == (T,)
    assert np.array_equal(out['bound'], good[2]) and np.array_equal(out['info'], good[1]) and np.array_equal(out['rmse_bound'], good[3])
    dyn.init_rv = sm.GaussRV(2, cov=np.array([[1.0, 2.0], [2.0, 1.0]]))
    assert mcshard.finalize_crlb(s, dyn, B)['status'] == 1
    with pytest.raises(ValueError, match='shape'):
        mcshard.finalize_crlb(s[:, :-1], dyn, B)
    assert _finalize(p.D, T, 0, s, p.P0, p.Q)[0] == E_ARG                                                  # B_total < 1


def _define(code, jac, din, dout):
    from ssmtoybox_amd import _lib
    return _lib.define_integrand(code, din, dout, False) if jac is None else _lib.define_integrand_dx(code, jac, din, dout, False)


def _c_call(f_dyn, f_obs, D, Y, dq=None, Lq=None, G=None, Lr=None, q_kind=GAUSS, r_kind=GAUSS, B=0, ld=64, T=3):
    """(rc of ssmq_pcrlb_kernel_name, rc of ssmq_pcrlb_sums_dev, message, the sums buffer untouched?) - the sums call with an empty batch
    unless told otherwise: nothing is launched, d_x is never read."""
    from ssmtoybox_amd import _lib
    lib = _lib.load()
    dq = D if dq is None else dq
    q, kq = _rv(q_kind, np.eye(dq) if Lq is None else Lq, 4.0)
    r, kr = _rv(r_kind, np.eye(Y) if Lr is None else Lr, 4.0)
    Gc = None if G is None else np.ascontiguousarray(G, dtype=np.float64)
    buf = ctypes.create_string_buffer(512)
    rc_name = lib.ssmq_pcrlb_kernel_name(ctypes.byref(f_dyn), ctypes.byref(f_obs), D, Y, dq, ctypes.byref(q), _lib.dp(Gc), ctypes.byref(r), buf, 512)
    msg = _lib.last_error() if rc_name else buf.value.decode()
    sums = np.full((max(T, 1), 200), -7.0)
    rc = lib.ssmq_pcrlb_sums_dev(ctypes.byref(f_dyn), ctypes.byref(f_obs), D, Y, dq, B, ld, T, ctypes.c_void_p(4096), ctypes.byref(q),
                                 _lib.dp(Gc), ctypes.byref(r), _lib.dp(sums))
    if rc:
        msg = _lib.last_error()
    return rc_name, rc, msg, bool(np.all(sums == -7.0))


def refusal_cases():
    """name -> (arguments of _c_call, expected code, what the message must name); shared with the GPU test of the sentinels."""
    from ssmtoybox_amd import _lib
    I = _lib.Integrand.make
    ungm_d, ungm_m, pend_d, pend_m = I(_lib.F_UNGM_DYN), I(_lib.F_UNGM_MEAS), I(_lib.F_PENDULUM_DYN, (0.01,)), I(_lib.F_PENDULUM_MEAS)
    no_jac = I(_define(uj.S_DYN_CODE, None, 1, 1))
    big_d = I(_define(*uj.poly_model(7, 7)[:2], 7, 7))
    big_m = I(_define(*uj.poly_model(5, 3)[:2], 3, 5))
    six_d = I(_define(*uj.poly_model(6, 6)[:2], 6, 6))
    return {
        'noise as an argument (transition)': ((I(_lib.F_UNGMNA_DYN), ungm_m, 1, 1), E_UNSUPPORTED, 'noise as an argument'),
        'noise as an argument (measurement)': ((ungm_d, I(_lib.F_UNGMNA_MEAS), 1, 1), E_UNSUPPORTED, 'noise as an argument'),
        'noise as an argument (CTRS)': ((I(_lib.F_CTRS_DYN, (0.05,)), pend_m, 5, 1), E_UNSUPPORTED, 'noise as an argument'),
        'built-in transition without a Jacobian': ((I(_lib.F_REENTRY1D_DYN, (0.1,)), I(_lib.F_RANGE_MEAS), 3, 1), E_UNSUPPORTED, 'no Jacobian'),
        'built-in measurement without a Jacobian': ((ungm_d, I(_lib.F_RANGE_MEAS), 1, 1), E_UNSUPPORTED, 'measurement model has no Jacobian'),
        'user model without a Jacobian': ((no_jac, ungm_m, 1, 1), E_UNSUPPORTED, 'transition model has no Jacobian'),
        'Student-t measurement noise': ((ungm_d, ungm_m, 1, 1, None, None, None, None, GAUSS, STUDENT), E_UNSUPPORTED, 'Student-t'),
        'mixture measurement noise': ((ungm_d, ungm_m, 1, 1, None, None, None, None, GAUSS, MIXTURE), E_UNSUPPORTED, 'mixture'),
        'Student-t process noise': ((ungm_d, ungm_m, 1, 1, None, None, None, None, STUDENT, GAUSS), E_UNSUPPORTED, 'Student-t'),
        'mixture process noise': ((ungm_d, ungm_m, 1, 1, None, None, None, None, MIXTURE, GAUSS), E_UNSUPPORTED, 'mixture'),
        'dq != D': ((I(_lib.F_CV_DYN, (0.5,)), I(_lib.F_PENDULUM_MEAS, (), [0]), 4, 1, 2), E_UNSUPPORTED, "G Q G'"),
        "G Q G' not positive definite": ((pend_d, pend_m, 2, 1, None, None, np.ones((2, 2))), E_UNSUPPORTED, 'not positive definite'),
        'condition number above 1e12': ((pend_d, pend_m, 2, 1, None, np.diag([1.0, 1e-7])), E_ARG, '1e12'),
        'D > 6': ((big_d, pend_m, 7, 1), E_UNSUPPORTED, 'D = 7'),
        'Y > 4': ((six_d, big_m, 6, 5), E_UNSUPPORTED, 'Y = 5'),
    }


def test_refusals_c_abi():
    """Every refusal of the table returns its code from both entry points before a device is looked for, names the range where it is
    SSMQ_E_UNSUPPORTED, and leaves the output alone."""
    for name, (args, code, word) in refusal_cases().items():
        rc_name, rc, msg, untouched = _c_call(*args)
        assert (rc_name, rc) == (code, code), (name, rc_name, rc, msg)
        assert word in msg and untouched, (name, msg)
        if code == E_UNSUPPORTED:
            assert 'range' in msg and 'D <= 6' in msg, (name, msg)
    from ssmtoybox_amd import _lib
    I = _lib.Integrand.make
    pend = (I(_lib.F_PENDULUM_DYN, (0.01,)), I(_lib.F_PENDULUM_MEAS), 2, 1)
    ok = _c_call(*pend, Lq=np.diag([1.0, 1e-5]), T=0)                                  # condition number 1e10; T = 0 is no part of the name
    assert ok[0] == 0 and ok[1] == E_ARG and ok[3] and 'T >= 1' in ok[2]
    res = _c_call(*pend, B=10, ld=5)
    assert res[0] == 0 and res[1] == E_ARG and res[3]                                  # ld < B
    assert _c_call(*pend, B=-1)[1] == E_ARG
    assert _c_call(I(_lib.F_UNGM_DYN), I(_lib.F_UNGM_MEAS), 2, 1)[:2] == (E_ARG, E_ARG)   # dimension mismatch
    assert _c_call(*pend, Lr=np.zeros((1, 1)))[:2] == (E_ARG, E_ARG)                   # a factor of R without a positive diagonal
    # the names: built-in, user, mixed
    buf =ctypes.create_string_buffer(512)
    q, kq = _rv(GAUSS, np.eye(2))
    r, kr = _rv(GAUSS, np.eye(1))
    lib = _lib.load()
    assert lib.ssmq_pcrlb_kernel_name(ctypes.byref(pend[0]), ctypes.byref(pend[1]), 2, 1, 2, ctypes.byref(q), None, ctypes.byref(r), buf, 512) == 0
    assert buf.value.decode() == 'k_pcrlb_dyn<2, 2> | k_pcrlb_obs<2, 1> | k_pcrlb_rows'
    vdp = I(_define(uj.VDP_CODE, uj.VDP_JAC, 2, 2), (0.1, 1.5))
    assert lib.ssmq_pcrlb_kernel_name(ctypes.byref(vdp), ctypes.byref(pend[1]), 2, 1, 2, ctypes.byref(q), None, ctypes.byref(r), buf, 512) == 0
    assert re.fullmatch(r'k_pcrlb_dyn_fn<\d+, 2, 2> \(run-time compiled\) \| k_pcrlb_obs<2, 1> \| k_pcrlb_rows', buf.value.decode()), buf.value


def test_refusals_python():
    from ssmtoybox_amd import mcshard, ssinf, ssmod as sm
    g1 = sm.GaussRV(1)
    ungm = sm.UNGMTransition(g1, sm.GaussRV(1, cov=np.array([[10.0]])))
    meas = sm.UNGMMeasurement(g1, 1)
    cv = sm.ConstantVelocity(sm.GaussRV(4), sm.GaussRV(2), dt=0.5)
    cases = [
        (sm.UNGMNATransition(g1, g1), sm.UNGMNAMeasurement(g1, 1), 'noise as an argument'),
        (sm.ReentryVehicle1DTransition(sm.GaussRV(3), sm.GaussRV(3)), sm.RangeMeasurement(g1, 3), 'no Jacobian'),
        (ungm, sm.UNGMMeasurement(sm.StudentRV(1), 1), 'Student-t'),
        (sm.UNGMTransition(g1, sm.StudentRV(1)), meas, 'Student-t'),
        (ungm, sm.UNGMMeasurement(sm.GaussianMixtureRV(1, covs=(np.eye(1), 2 * np.eye(1)), alphas=(0.5, 0.5)), 1), 'mixture'),
        (cv, sm.Pendulum2DMeasurement(g1, 4, state_index=[0]), "G Q G'"),
    ]
    for dyn, obs, word in cases:
        for call in (lambda: mcshard.crlb_kernel_name(dyn, obs), lambda: mcshard.device_crlb_sums(dyn, obs, None, 0, 64, 3),
                     lambda: ssinf.posterior_crlb_dev(dyn, obs, None, 0, 64, 3)):
            with pytest.raises(NotImplementedError, match='(?s)' + re.escape(word) + '.*range.*D <= 6'):       # before the device is touched
                call()
    Plain = uj.transition('PcrlbPlain', 1, uj.S_DYN_CODE, None)
    with pytest.raises(NotImplementedError, match='no Jacobian.*range'):
        mcshard.crlb_kernel_name(Plain(g1, g1), meas)
    pend = sm.Pendulum2DTransition(sm.GaussRV(2), sm.GaussRV(2, cov=np.diag([1.0, 1e-14])), dt=0.01)
    with pytest.raises(ValueError, match='1e12'):
        mcshard.crlb_kernel_name(pend, sm.Pendulum2DMeasurement(g1, 2))
    with pytest.raises(ValueError, match='T >= 1'):
        mcshard.device_crlb_sums(ungm, meas, None, 0, 64, 0)
    with pytest.raises(ValueError, match='shape'):
        ssinf.posterior_crlb(ungm, meas, np.zeros((1, 1, 4)))
    with pytest.raises(NotImplementedError, match='initial state'):
        mcshard.finalize_crlb(np.zeros((2, 3)), sm.UNGMTransition(sm.StudentRV(1), g1), 4)
    assert mcshard.crlb_kernel_name(ungm, meas) == 'k_pcrlb_dyn<1, 1> | k_pcrlb_obs<1, 1> | k_pcrlb_rows'
    # allreduce_sums takes the array of device_crlb_sums unchanged
    s = np.arange(12.0).reshape(4, 3)
    assert np.array_equal(mcshard.allreduce_sums(s), s)


COMPILE_SHAPES = [(1, 1, 1), (2, 1, 2), (6, 4, 3)]


def _compile(kind, D, E, DIN):
    """The compile check of one _fn kernel for gfx950: the resource remarks as a dict."""
    from ssmtoybox_amd import _lib
    dyn = kind == _lib.RTC_PCRLB_DYN
    code, jac = uj.poly_model(D if dyn else E, DIN)[:2]
    fid = _define(code, jac, DIN, D if dyn else E)
    rc, log = _lib.rtc_compile_check(fid, kind, D, E, 0, 0)
    assert rc == 0, log
    assert ('k_pcrlb_dyn_fn' if dyn else 'k_pcrlb_obs_fn') in log.splitlines()[0]
    res = {k: int(v) for k, v in re.findall(r'(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)', log)}
    print(log.splitlines()[0], res)
    return res


@pytest.mark.parametrize('D,E,DIN', COMPILE_SHAPES)
def test_compile_check_gfx950(D, E, DIN):
    """Both _fn kernels compile for gfx950 without scratch memory."""
    from ssmtoybox_amd import _lib
    for kind in (_lib.RTC_PCRLB_DYN, _lib.RTC_PCRLB_OBS):
        res = _compile(kind, D, E, DIN)
        assert res['ScratchSize [bytes/lane]'] == 0 and res['VGPRs'] <= 256, res


def test_compile_check_gfx950_full_transition():
    """k_pcrlb_dyn_fn at (6, 6, 6): all 57 sums of the largest shape in registers."""
    from ssmtoybox_amd import _lib
    res = _compile(_lib.RTC_PCRLB_DYN, 6, 6, 6)
    assert res['ScratchSize [bytes/lane]'] == 0 and res['VGPRs'] <= 256, res
    # what the compile check refuses
    plain = _define(uj.S_DYN_CODE, None, 1, 1)
    assert _lib.rtc_compile_check(plain, _lib.RTC_PCRLB_DYN, 1, 1, 0, 0)[0] == E_UNSUPPORTED
    wide = _define(*uj.poly_model(5, 3)[:2], 3, 5)
    assert _lib.rtc_compile_check(wide, _lib.RTC_PCRLB_OBS, 6, 5, 0, 0)[0] == E_UNSUPPORTED
