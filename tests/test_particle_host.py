"""The bootstrap particle filter without a device: the two symbols, every refusal through Python and the C ABI, the conditions under
which the GPU test may demand exact ancestors, and the NumPy restatement against the exact Kalman filter."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import _particle_oracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_UNSUPPORTED = -1, -3


def test_symbols_and_version():
    from ssmtoybox_amd import _lib
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'ssmq.h')).read(), flags=re.S)
    lib = _lib.load()
    for name in ('ssmq_particle_filter_dev', 'ssmq_particle_kernel_name'):
        assert re.search(r'\b' + name + r'\s*\(', hdr), name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert lib.ssmq_version() == _lib.ABI_VERSION == 102


def _rv(kind, dim, dof=0.0, n_comp=1):
    from ssmtoybox_amd import _lib
    chol = np.ascontiguousarray(np.tile(np.eye(dim), (n_comp, 1, 1)))
    alpha = np.full(n_comp, 1.0 / n_comp)
    r = _lib.Rv()
    r.kind, r.dim, r.n_comp, r.dof = kind, dim, n_comp, dof
    r.mean, r.chol, r.alpha = None, chol.ctypes.data_as(_lib.c_double_p), alpha.ctypes.data_as(_lib.c_double_p)
    return r, (chol, alpha)


def _c_call(fid_dyn, fid_obs, D, Y, dq, N, T=4, rv=None, par_dyn=(), idx_obs=None, run=True):
    """Both entry points; the pass itself with an empty batch (B = 0: nothing is launched, no pointer is read) and only where `run`:
    the refusals come before the device is touched."""
    from ssmtoybox_amd import _lib
    lib = _lib.load()
    f_dyn, f_obs = _lib.Integrand.make(fid_dyn, par_dyn), _lib.Integrand.make(fid_obs, (), idx_obs)
    r, keep = rv if rv is not None else _rv(_lib.RV_GAUSS, Y)
    qL = np.ascontiguousarray(np.eye(dq))
    buf = ctypes.create_string_buffer(256)
    rc_name = lib.ssmq_particle_kernel_name(ctypes.byref(f_dyn), ctypes.byref(f_obs), D, Y, dq, N, ctypes.byref(r), buf, 256)
    if not run:
        return rc_name, None, buf.value.decode()
    dummy = ctypes.c_void_p(4096)
    rc = lib.ssmq_particle_filter_dev(ctypes.byref(f_dyn), ctypes.byref(f_obs), D, Y, dq, N, 0, 64, T, dummy, dummy, dummy, None,
                                      qL.ctypes.data_as(_lib.c_double_p), None, ctypes.byref(r), 0.5, 1, 0, dummy, dummy, dummy, dummy, dummy,
                                      None, None, None)
    return rc_name, rc, buf.value.decode()


def test_refusals_c_abi():
    """Every refusal returns its code from both entry points, before a device is looked for (this host has none: an accepted call
    ends in SSMQ_E_HIP, never in a result)."""
    from ssmtoybox_amd import _lib
    ungm = (_lib.F_UNGM_DYN, _lib.F_UNGM_MEAS, 1, 1, 1)
    assert _c_call(*ungm, 100)[:2] == (E_ARG, E_ARG)                                         # N no multiple of 64
    assert _c_call(*ungm, 32)[:2] == (E_ARG, E_ARG)                                          # N below 64
    assert _c_call(*ungm, 8192)[:2] == (E_UNSUPPORTED, E_UNSUPPORTED)                        # N beyond 4096
    radar_idx = dict(idx_obs=(0, 1), par_dyn=(0.1,))
    assert _c_call(15, 10, 6, 2, 6, 2048, **radar_idx)[:2] == (E_UNSUPPORTED, E_UNSUPPORTED)  # D = 6 with N = 2048: (2 D + 1) N > 13312
    ok = _c_call(15, 10, 6, 2, 6, 1024, run=False, **radar_idx)
    assert ok[0] == 0 and 'k_particle_filter<D=6>' in ok[2] and '107264 B' in ok[2]         # (13 * 1024 + 96) doubles
    assert _c_call(1024, _lib.F_UNGM_MEAS, 1, 1, 1, 64)[:2] == (E_UNSUPPORTED, E_UNSUPPORTED)   # a user model
    assert _c_call(_lib.F_UNGM_DYN, 1025, 1, 1, 1, 64)[:2] == (E_UNSUPPORTED, E_UNSUPPORTED)
    assert _c_call(3, 4, 1, 1, 1, 64)[:2] == (E_UNSUPPORTED, E_UNSUPPORTED)                  # UNGMNA: noise as an argument
    assert _c_call(13, 10, 5, 2, 2, 64, idx_obs=(0, 1))[:2] == (E_UNSUPPORTED, E_UNSUPPORTED)   # CTRS
    assert _c_call(*ungm, 64, rv=_rv(_lib.RV_MIXTURE, 1, n_comp=2))[:2] == (E_UNSUPPORTED, E_UNSUPPORTED)
    name_rc, rc, name = _c_call(*ungm, 64, T=0)
    assert name_rc == 0 and rc == E_ARG and 'k_particle_filter<D=1>' in name               # T = 0 (no part of the name query)
    assert _c_call(*ungm, 64, rv=_rv(_lib.RV_STUDENT, 1, dof=0.0))[:2] == (E_ARG, E_ARG)     # Student-t without dof
    assert _c_call(14, 10, 4, 2, 2, 64, idx_obs=(0,), par_dyn=(0.5,))[:2] == (E_ARG, E_ARG)    # a state index shorter than the radar's two inputs
    assert _c_call(*ungm, 320, run=False)[0] == 0                                          # an accepted shape: the name query only


def test_refusals_python():
    from ssmtoybox_amd import ssinf, ssmod as sm
    dyn, obs = po.package_models('ungm')
    for n in (100, 32):
        with pytest.raises(ValueError, match='multiple of 64'):
            ssinf.BootstrapParticleFilter(dyn, obs, num_particles=n)
    with pytest.raises(NotImplementedError, match='outside the range'):
        ssinf.BootstrapParticleFilter(dyn, obs, num_particles=8192)
    dyn6, obs6 = sm.ReentryVehicle2DBiasTransition(sm.GaussRV(6), sm.GaussRV(4)), sm.Radar2DMeasurement(sm.GaussRV(2), 6, state_index=[0, 1])
    with pytest.raises(NotImplementedError, match='13312'):
        ssinf.BootstrapParticleFilter(dyn6, obs6, num_particles=2048)
    assert 'D=6' in ssinf.BootstrapParticleFilter(dyn6, obs6, num_particles=1024).kernel_name()

    class UserDyn(sm.TransitionModel):
        dim_state, dim_noise, noise_additive = 1, 1, True
        device_code = 'o[0] = 0.9 * x[0];'

    with pytest.raises(NotImplementedError, match='user models'):
        ssinf.BootstrapParticleFilter(UserDyn(sm.GaussRV(1), sm.GaussRV(1)), obs)
    with pytest.raises(NotImplementedError, match='non-additive'):
        ssinf.BootstrapParticleFilter(sm.UNGMNATransition(sm.GaussRV(1), sm.GaussRV(1)), sm.UNGMNAMeasurement(sm.GaussRV(1), 1))
    mix = sm.GaussianMixtureRV(1, covs=(np.eye(1), 4 * np.eye(1)), alphas=(0.5, 0.5))
    with pytest.raises(NotImplementedError, match='GaussianMixtureRV'):
        ssinf.BootstrapParticleFilter(dyn, sm.UNGMMeasurement(mix, 1))
    pf = ssinf.BootstrapParticleFilter(dyn, obs, num_particles=320)
    assert 'k_particle_filter<D=1>' in pf.kernel_name()
    with pytest.raises(ValueError, match='at least one time step'):
        pf.forward_pass_batch(np.zeros((1, 0, 3)))
    for call in (pf.backward_pass, pf.backward_pass_batch, lambda: pf.innovations(np.zeros((1, 3))), lambda: pf.innovations_batch(None),
                 lambda: pf.innovations_dev(None, None, None, 1, 64, 1), lambda: pf.iterated_pass(None, 2),
                 lambda: pf.iterated_pass_batch(None, 2), lambda: pf.iterated_smoother(None), lambda: pf.iterated_smoother_batch(None),
                 lambda: ssinf.run_filters([pf], np.zeros((1, 3, 2)))):
        with pytest.raises(NotImplementedError, match='13312'):           # the message names the range
            call()
    assert not isinstance(pf, ssinf.GaussianInference)


@pytest.mark.parametrize('name,N', [(n, N) for n, Ns in po.CASES.items() for N in Ns])
def test_oracle_cases_are_decidable(name, N):
    """The cases of tests/test_particle_gpu.py, oracle alone: at least one step resamples and one does not, every ancestor is
    decided by a margin of at least 64 N eps and every resampling decision by an ESS margin of at least 1e-9 - so the GPU test may
    demand exact ancestors and decisions.  Seed 11, the issue's, meets this in every case; no other seed was needed."""
    model, m0, P0, _ = po.case(name)
    y = po.case_data(name)
    did = []
    for b in range(po.B):
        o = po.full_pass(model, y[:, :, b], m0, P0, po.SEED, b, N, po.ESS_THRESHOLD)
        assert o['status'] == 0 and np.all(np.isfinite(o['fm'])) and np.all(np.isfinite(o['fP']))
        assert o['anc_margin'].min() >= 64 * N * po.EPS, (b, o['anc_margin'].min())
        assert o['ess_margin'].min() >= 1e-9, (b, o['ess_margin'].min())
        assert np.all(o['anc'][:, ~o['resampled']] == np.arange(N)[:, None])
        assert np.all(np.diff(o['anc'][:, o['resampled']], axis=0) >= 0)          # systematic resampling keeps the order
        np.testing.assert_allclose(np.exp(o['lwn']).sum(axis=0), 1.0, rtol=1e-12)
        did.extend(o['resampled'])
    assert any(did) and not all(did)


def test_oracle_long_double_twin():
    """The long-double form of the weight and moment arithmetic agrees with the float64 one to rounding."""
    model, m0, P0, _ = po.case('cv_radar')
    y = po.case_data('cv_radar')[:, :, 0]
    x = po.propagate(model, po.initial_particles(model, m0, P0, po.SEED, 0, 128), np.arange(128), po.SEED, 0, 0)
    lw0 = np.full(128, -np.log(128.0))
    l64, ll64 = po.weigh(model, x, lw0, y[:, 0], 0)
    lld, llld = po.weigh(model, x, lw0, y[:, 0], 0, dtype=po.LD)
    assert abs(float(ll64 - llld)) <= 64 * po.EPS * (1 + abs(float(llld)))
    assert np.max(np.abs(l64 - lld) / (1 + np.abs(lld))) <= 64 * po.EPS * np.linalg.cond(model.Lr.dot(model.Lr.T))
    m64, mld = po.moments(x, l64), po.moments(x, l64, dtype=po.LD)
    for a64, ald in zip(m64, mld):
        assert np.max(np.abs(np.asarray(a64) - np.asarray(ald))) <= 1e-12 * max(1.0, float(np.max(np.abs(np.asarray(ald)))))


def test_oracle_against_the_kalman_filter():
    """A scalar linear-Gaussian model x_j = a x_{j-1} + q, y_j = c x_j + r, where the Kalman filter is the exact posterior mean: the
    oracle's means at N = 4096 are within 5 Monte-Carlo standard errors of it, the standard error taken from the spread of the
    bootstrap filter over 32 seeds."""
    a, c, Q, R, m0, P0, T = 0.9, 0.7, 0.5, 0.4, np.array([0.3]), np.array([[2.0]]), 8
    model = po.Model(lambda x, t: a * x, lambda x, t: c * x, 1, 1, [0.0], [[np.sqrt(Q)]], np.eye(1), [0.0], [[np.sqrt(R)]])
    rng = np.random.default_rng(5)
    x, y = m0[0] + np.sqrt(P0[0, 0]) * rng.standard_normal(), np.empty((1, T))
    for j in range(T):
        x = a * x + np.sqrt(Q) * rng.standard_normal()
        y[0, j] = c * x + np.sqrt(R) * rng.standard_normal()
    km, m, P = np.empty(T), m0[0], P0[0, 0]
    for j in range(T):
        mp, Pp = a * m, a * a * P + Q
        K = Pp * c / (c * c * Pp + R)
        m, P = mp + K * (y[0, j] - c * mp), (1 - K * c) * Pp
        km[j] = m
    runs = np.array([po.full_pass(model, y, m0, P0, seed, 0, 4096, 0.5)['fm'][0] for seed in range(32)])
    se = runs.std(axis=0, ddof=1)
    assert np.all(se > 0) and np.all(se < 0.05)
    assert np.all(np.abs(runs[0] - km) <= 5 * se), (runs[0] - km) / se
    assert np.all(np.abs(runs.mean(axis=0) - km) <= 5 * se / np.sqrt(32) + 1e-12), (runs.mean(axis=0) - km) / se


def test_gap_to_the_ukf_on_the_cpu():
    """What tests/test_particle_gpu.py::test_better_filter_than_the_ukf relies on, established here first: UNGM, B = 256, T = 20,
    N = 512, seed 11, the oracle's full pass against the UnscentedKalman of oracle/ssmq_oracle.py on the simulator's data, time-averaged
    RMSE over the batch, the standard error of the difference by a bootstrap over the trajectories.
      data aligned with the filters' time convention (T + 1 steps simulated, the first dropped: `study_cpu`):
          particle filter 4.5523, UKF 8.3312, gap 3.7790 = 19.8 standard errors (0.1913);  seeds 1 / 2: 21.5 / 21.9
      the raw T steps of the simulator, as the issue words the test:
          particle filter 9.2691, UKF 8.5704, gap -0.6987 = -3.4 standard errors (0.2085);  seeds 1 / 2: -2.3 / -3.5
    On the raw data the simulator's x[k] = f(x[k-1], k - 1) is one step behind the time argument both filters use, a model error of
    up to 8 |cos 1.2 k - cos 1.2 (k - 1)| in the UNGM drift: the particle filter, which trusts its model more, loses.  The gap the
    issue asks for does not exist there for any seed tried (11, 1, 2), so the GPU test runs on the aligned data, nothing else changed."""
    r_pf, r_ukf = po.study_cpu(po.STUDY['seed'])
    gap, se = float(np.mean(r_ukf - r_pf)), po.bootstrap_se(r_ukf - r_pf)
    print('particle filter %.4f, UKF %.4f, gap %.4f, standard error %.4f' % (r_pf.mean(), r_ukf.mean(), gap, se))
    assert gap >= 4 * se, (gap, se)
