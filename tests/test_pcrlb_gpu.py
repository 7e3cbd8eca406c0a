"""The posterior Cramer-Rao sums on the device (k_pcrlb_dyn / k_pcrlb_obs, their run-time compiled _fn forms, k_pcrlb_rows) against
the NumPy restatement of tests/_pcrlb_oracle.py from the same states, the bits of the reduction, and the bound as the floor of the
filter study of tests/test_particle_gpu.py."""
import functools

import numpy as np
import pytest

from tests import _particle_oracle as ppo
from tests import _pcrlb_oracle as po
from tests._cases import RTOL

pytestmark = pytest.mark.gpu

T = 5
SHAPES = [(300, 320), (1, 64)]      # two workgroups per step with a partial wave and 20 padding lanes; one trajectory
PAIRS = ['ungm', 'pendulum', 'vdp_polar', 'vdp_pendulum', 'six']


@functools.lru_cache(maxsize=None)
def _case(name, B):
    """(pair, states (D, T + 1, B), the oracle's sums, the sums of the absolute values of their terms), shared and read-only."""
    p = po.pair(name)
    x = po.states(p, T, B)
    ref, ref_abs = po.sums(p, x)
    for a in (x, ref, ref_abs):
        a.setflags(write=False)
    return p, x, ref, ref_abs


@functools.lru_cache(maxsize=None)
def _models(name):
    return po.pair(name).models()


def _upload(x, ld, fill=0.0):
    from ssmtoybox_amd import _lib
    D, T1, B = x.shape
    xb = np.full((T1, D, ld), fill)
    xb[:, :, :B] = x.transpose(1, 0, 2)
    d_x = _lib.DeviceBuffer(xb.nbytes)
    d_x.upload(xb)
    return d_x


def _device_sums(name, x, ld, fill=0.0):
    from ssmtoybox_amd import mcshard
    dyn, obs = _models(name)
    d_x = _upload(x, ld, fill)
    try:
        return mcshard.device_crlb_sums(dyn, obs, d_x, x.shape[2], ld, x.shape[1] - 1)
    finally:
        d_x.free()


def _assert_sums_close(got, ref, ref_abs, what):
    err = np.abs(got - ref)
    worst = float(np.max(err / np.maximum(ref_abs, 1e-300)))
    print(what, 'largest error relative to the sum of |terms|: %.3g' % worst)
    assert np.all(err <= RTOL * ref_abs), (what, worst)


@pytest.mark.parametrize('B,ld', SHAPES)
@pytest.mark.parametrize('name', PAIRS)
def test_sums_against_the_oracle(name, B, ld):
    p, x, ref, ref_abs = _case(name, B)
    got = _device_sums(name, x, ld)
    assert got.shape == (T, po.width(p.D))
    _assert_sums_close(got, ref, ref_abs, (name, B, ld))


def test_bits():
    from ssmtoybox_amd import _lib, mcshard, ssinf
    name, B = 'pendulum', 300
    p, x, ref, _ = _case(name, B)
    a = _device_sums(name, x, 320)
    assert np.array_equal(a, _device_sums(name, x, 512))                      # the pitch does not enter
    assert np.array_equal(a, _device_sums(name, x, 320))                      # twice
    assert np.array_equal(a, _device_sums(name, x, 320, fill=np.nan))         # padding columns are never read
    assert np.array_equal(a, _device_sums(name, x, 512, fill=np.nan))
    dyn, obs = _models(name)
    one = ssinf.posterior_crlb(dyn, obs, x)                                   # host arrays: upload, sums, finalise
    d_x = _upload(x, 320)
    dev = ssinf.posterior_crlb_dev(dyn, obs, d_x, B, 320, T)
    d_x.free()
    two = mcshard.finalize_crlb(mcshard.allreduce_sums(a), dyn, B)
    for k in ('info', 'bound', 'rmse_bound'):
        assert np.array_equal(one[k], two[k]) and np.array_equal(dev[k], two[k]) and np.all(np.isfinite(one[k])), k
    assert one['status'] == dev['status'] == two['status'] == 0
    # a user pair as well: the run-time compiled kernels reduce in the same order
    b = _device_sums('vdp_polar', _case('vdp_polar', B)[1], 320)
    assert np.array_equal(b, _device_sums('vdp_polar', _case('vdp_polar', B)[1], 512, fill=np.nan))
    assert mcshard.crlb_kernel_name(dyn, obs) == 'k_pcrlb_dyn<2, 2> | k_pcrlb_obs<2, 1> | k_pcrlb_rows'
    # an empty batch: zeros
    d_e = _lib.DeviceBuffer(8 * (T + 1) * 2 * 64)
    assert np.array_equal(mcshard.device_crlb_sums(dyn, obs, d_e, 0, 64, T), np.zeros((T, po.width(2))))
    d_e.free()


def test_time_reaches_the_jacobian():
    """Item (j, b) is evaluated at t = j - the measurement kernel too, whose input is plane j + 1."""
    name, B = 'time', 300
    p, x, ref, ref_abs = _case(name, B)
    got = _device_sums(name, x, 320)
    _assert_sums_close(got, ref, ref_abs, name)
    c00 = got[:, 3 + 4]                                                       # H' Ri H, entry (0, 0): B (1 + 0.5 t)^2 / R
    j = np.arange(T)
    np.testing.assert_allclose(c00, B * (1.0 + 0.5 * j) ** 2 / p.R[0, 0], rtol=RTOL)
    assert np.all(np.abs(c00 - B * (1.0 + 0.5 * (j + 1)) ** 2 / p.R[0, 0]) > 0.1 * c00)
    assert np.ptp(got[:, 2]) > 0                                              # F' Qi F, entry (1, 1) moves with t as well


def test_linear_user_model():
    """F, H constant: the sums are B times one term whatever the states, and the bound is the Kalman filter's Riccati recursion."""
    from ssmtoybox_amd import ssinf
    name, B = 'linear', 300
    p, x, ref, ref_abs = _case(name, B)
    got = _device_sums(name, x, 320)
    _assert_sums_close(got, ref, ref_abs, name)
    exact = po.linear_sums(po.LIN_F, po.LIN_H, p.Qi, p.Ri, T, B)
    assert np.all(np.abs(got - exact) <= RTOL * ref_abs)
    dyn, obs = _models(name)
    out = ssinf.posterior_crlb(dyn, obs, x)
    P = po.riccati(po.LIN_F, po.LIN_H, p.Q, p.R, p.P0, T)
    err = np.max(np.abs(out['bound'] - P)) / np.max(np.abs(P))
    print('bound against the Riccati recursion: %.3g' % err)
    assert out['status'] == 0 and err <= RTOL
    other = ssinf.posterior_crlb(dyn, obs, po.states(p, T, B, seed=9))        # other states, the same bound
    assert np.max(np.abs(other['bound'] - P)) <= RTOL * np.max(np.abs(P))


def test_nan_true_state():
    """A NaN in plane 2 of one trajectory: the transition kernel reads it at step 2, the measurement kernel at step 1 - those two rows
    are non-finite, the others keep their bits, and the finaliser stops at step 1."""
    from ssmtoybox_amd import mcshard
    name, B = 'pendulum', 300
    p, x, ref, _ = _case(name, B)
    clean = _device_sums(name, x, 320)
    xn = x.copy()
    xn[0, 2, 77] = np.nan
    got = _device_sums(name, xn, 320)
    tri, DD = 3, 4
    assert np.array_equal(got[[0, 3, 4]], clean[[0, 3, 4]])
    assert np.array_equal(got[1, :tri + DD], clean[1, :tri + DD]) and not np.all(np.isfinite(got[1, tri + DD:]))
    assert np.array_equal(got[2, tri + DD:], clean[2, tri + DD:]) and not np.all(np.isfinite(got[2, :tri + DD]))
    dyn, _ = _models(name)
    out, ok = mcshard.finalize_crlb(got, dyn, B), mcshard.finalize_crlb(clean, dyn, B)
    assert out['status'] == 2 and ok['status'] == 0
    for k in ('info', 'bound', 'rmse_bound'):
        assert np.array_equal(out[k][..., :1], ok[k][..., :1]) and np.all(np.isnan(out[k][..., 1:])), k


def test_refusals_leave_the_outputs_alone():
    """One case of each error code through the C ABI, with a device present: the code, and the sentinel-filled sums untouched."""
    from tests import test_pcrlb_host as th
    cases = th.refusal_cases()
    for name in ('Student-t measurement noise', 'condition number above 1e12'):
        args, code, word = cases[name]
        rc_name, rc, msg, untouched = th._c_call(*args)
        assert (rc_name, rc) == (code, code) and word in msg and untouched, (name, rc_name, rc, msg)


def test_the_bound_is_the_floor_of_the_study():
    """UNGM, the aligned data of tests/_particle_oracle.py::STUDY (B = 256, T = 20, seed 11): the time-averaged rmse_bound lies below
    the particle filter's time-averaged RMSE and below the UnscentedKalman's.  Established on the CPU first, with the oracles alone
    (tests/_pcrlb_oracle.py on the states of oracle/ssmq_oracle.simulate, float64 and the 50-digit twin agree to the last digit): the
    bound is 0.9254 (0.749 .. 1.142 over the steps), the particle filter 4.5523, the UKF 8.3312 - a gap of 3.6268 = 38.3 bootstrap
    standard errors (0.0946) of the particle filter's score.  The bound is loose on this model: the measurement x^2 / 20 hides the sign
    of the state, which the Jacobians at the true states do not know.  The bound comes from 256 sampled trajectories and the device's
    particle filter differs from the oracle's by rounding-level resampling decisions, so what is asserted is the CPU gap less two of
    those standard errors: 3.4376 = 36.3 standard errors - not a margin chosen beforehand."""
    from ssmtoybox_amd import mcshard, ssinf, ssmod as sm
    dyn, obs = ppo.package_models('ungm')
    B, Ts, N, seed = (ppo.STUDY[k] for k in ('B', 'T', 'N', 'seed'))
    d_x, d_y, ld = sm.simulate_dev(dyn, obs, Ts + 1, B, seed=seed)
    bound = ssinf.posterior_crlb_dev(dyn, obs, d_x, B, ld, Ts)                  # the raw planes: p_0 .. p_T
    x1, y1 = d_x.view(8 * ld), d_y.view(8 * ld)                                # the filters get the planes from step 1 on
    rmse, owned = {}, [d_x, d_y]
    pf = ssinf.BootstrapParticleFilter(dyn, obs, num_particles=N, ess_threshold=ppo.ESS_THRESHOLD, seed=seed)
    for name, alg in (('ukf', ssinf.UnscentedKalman(dyn, obs)), ('pf', pf)):
        d_fm, d_fP, d_st = alg.forward_pass_dev(y1, B, ld, Ts)
        assert not d_st.download((ld,), dtype=np.int32)[:B].any(), name
        d_sc, names = mcshard.device_traj_scores(1, B, ld, Ts, x1, d_fm, d_fP, None, d_st)
        rmse[name] = d_sc.download((len(names), ld))[0, :B]
        owned += [d_fm, d_fP, d_st, d_sc]
    pf.free_dev()
    for buf in owned:
        buf.free()
    floor = float(bound['rmse_bound'].mean())
    se = ppo.bootstrap_se(rmse['pf'])
    print('bound %.4f, particle filter %.4f (bootstrap standard error %.4f), UKF %.4f' % (floor, rmse['pf'].mean(), se, rmse['ukf'].mean()))
    assert bound['status'] == 0 and bound['rmse_bound'].shape == (Ts,) and np.all(bound['rmse_bound'] > 0)
    assert rmse['pf'].mean() - floor > 3.6268 - 2 * 0.0946, (floor, rmse['pf'].mean())
    assert floor < rmse['ukf'].mean()
