"""The particle filter and smoothers with a Student-t initial state and process noise, without a device: the four *_rv symbols, every
refusal through the C ABI and Python, the conditions under which the GPU test may demand exact decisions, the sampler's distribution
and the gap of the heavy-tailed study, oracle alone."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import _particle_oracle as po
from tests import _particle_heavy_oracle as ho

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_UNSUPPORTED = -1, -3
NEW = ('ssmq_particle_filter_rv_dev', 'ssmq_particle_kernel_name_rv', 'ssmq_particle_smoother_rv_dev', 'ssmq_particle_smoother_kernel_name_rv')


def test_symbols_and_version():
    from ssmtoybox_amd import _lib
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'ssmq.h')).read(), flags=re.S)
    lib = _lib.load()
    for name in NEW:
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


def _filter_call(fid_dyn, fid_obs, D, Y, dq, N, x0, q, T=4, par_dyn=(), idx_obs=None):
    """Both filter entry points: the name query, and the pass with an empty batch (B = 0: nothing is launched, no pointer is read) -
    run only where the name query refuses: the refusals come before the device is touched, and this host has none."""
    from ssmtoybox_amd import _lib
    lib = _lib.load()
    f_dyn, f_obs = _lib.Integrand.make(fid_dyn, par_dyn), _lib.Integrand.make(fid_obs, (), idx_obs)
    r, keep = _rv(_lib.RV_GAUSS, Y)
    buf = ctypes.create_string_buffer(256)
    rc_name = lib.ssmq_particle_kernel_name_rv(ctypes.byref(f_dyn), ctypes.byref(f_obs), D, Y, dq, N, ctypes.byref(x0[0]), ctypes.byref(q[0]),
                                               ctypes.byref(r), buf, 256)
    if rc_name == 0:
        return rc_name, None, buf.value.decode()
    dummy = ctypes.c_void_p(4096)
    rc = lib.ssmq_particle_filter_rv_dev(ctypes.byref(f_dyn), ctypes.byref(f_obs), D, Y, dq, N, 0, 64, T, dummy, dummy, dummy,
                                         ctypes.byref(x0[0]), ctypes.byref(q[0]), None, ctypes.byref(r), 0.5, 1, 0, dummy, dummy, dummy, dummy,
                                         dummy, None, None, None)
    return rc_name, rc, _lib.last_error()


def _smoother_call(fid_dyn, D, dq, N, q, method, T=4, par_dyn=(), G=None):
    from ssmtoybox_amd import _lib
    lib = _lib.load()
    f_dyn = _lib.Integrand.make(fid_dyn, par_dyn)
    Gc = None if G is None else np.ascontiguousarray(G, dtype=np.float64)
    buf = ctypes.create_string_buffer(256)
    rc_name = lib.ssmq_particle_smoother_kernel_name_rv(ctypes.byref(f_dyn), D, dq, N, ctypes.byref(q[0]), _lib.dp(Gc), method, buf, 256)
    if rc_name == 0:
        return rc_name, None, buf.value.decode()
    dummy = ctypes.c_void_p(4096)
    rc = lib.ssmq_particle_smoother_rv_dev(ctypes.byref(f_dyn), D, dq, N, 0, 64, T, ctypes.byref(q[0]), _lib.dp(Gc), method, *([dummy] * 10),
                                           None, None, None)
    return rc_name, rc, _lib.last_error()


def test_refusals_c_abi():
    from ssmtoybox_amd import _lib
    ungm = (_lib.F_UNGM_DYN, _lib.F_UNGM_MEAS, 1, 1, 1, 64)
    gauss, t4 = _rv(_lib.RV_GAUSS, 1), _rv(_lib.RV_STUDENT, 1, dof=4.0)
    mix = _rv(_lib.RV_MIXTURE, 1, n_comp=2)
    # mixture kinds, either side: unsupported, the range named
    for x0, q in ((mix, gauss), (gauss, mix), (mix, t4)):
        a, b, text = _filter_call(*ungm, x0, q)
        assert (a, b) == (E_UNSUPPORTED, E_UNSUPPORTED) and 'range' in text and 'dof >= 2' in text, text
    # dof below 2: unsupported, the range named; a dof that is no dof: an argument error
    for x0, q in ((_rv(_lib.RV_STUDENT, 1, dof=1.5), gauss), (gauss, _rv(_lib.RV_STUDENT, 1, dof=1.999))):
        a, b, text = _filter_call(*ungm, x0, q)
        assert (a, b) == (E_UNSUPPORTED, E_UNSUPPORTED) and 'below 2' in text and 'dof >= 2' in text, text
    for bad in (0.0, -1.0, np.nan, np.inf):
        assert _filter_call(*ungm, gauss, _rv(_lib.RV_STUDENT, 1, dof=bad))[:2] == (E_ARG, E_ARG), bad
        assert _filter_call(*ungm, _rv(_lib.RV_STUDENT, 1, dof=bad), gauss)[:2] == (E_ARG, E_ARG), bad
    # kind / dimension mismatch
    assert _filter_call(*ungm, gauss, _rv(_lib.RV_STUDENT, 2, dof=4.0))[:2] == (E_ARG, E_ARG)            # q of dimension 2, dq = 1
    assert _filter_call(*ungm, gauss, _rv(7, 1))[:2] == (E_ARG, E_ARG)                                   # no such kind
    assert _filter_call(*ungm, gauss, _rv(_lib.RV_STUDENT, 1, dof=4.0, n_comp=2))[:2] == (E_ARG, E_ARG)   # two components
    # what the Gaussian entries refuse is refused here as well
    assert _filter_call(_lib.F_UNGM_DYN, _lib.F_UNGM_MEAS, 1, 1, 1, 100, t4, t4)[:2] == (E_ARG, E_ARG)
    assert _filter_call(_lib.F_UNGM_DYN, _lib.F_UNGM_MEAS, 1, 1, 1, 8192, t4, t4)[:2] == (E_UNSUPPORTED, E_UNSUPPORTED)
    assert _filter_call(1024, _lib.F_UNGM_MEAS, 1, 1, 1, 64, t4, t4)[:2] == (E_UNSUPPORTED, E_UNSUPPORTED)           # a user model
    assert _filter_call(3, 4, 1, 1, 1, 64, t4, t4)[:2] == (E_UNSUPPORTED, E_UNSUPPORTED)                             # noise as an argument
    # accepted: the names and the LDS
    for x0, q in ((t4, t4), (gauss, t4), (t4, gauss), (_rv(_lib.RV_STUDENT, 1, dof=2.0), t4)):
        rc, _, name = _filter_call(_lib.F_UNGM_DYN, _lib.F_UNGM_MEAS, 1, 1, 1, 320, x0, q)
        assert rc == 0 and 'k_particle_filter<D=1, QK=1>' in name and '%d B' % (8 * (3 * 320 + 96)) in name, name
    rc, _, name = _filter_call(_lib.F_UNGM_DYN, _lib.F_UNGM_MEAS, 1, 1, 1, 320, gauss, gauss)
    assert rc == 0 and 'k_particle_filter<D=1>' in name and 'QK' not in name                            # all-Gaussian: the old kernel
    radar_idx = dict(idx_obs=(0, 1), par_dyn=(0.1,))
    rc, _, name = _filter_call(15, 10, 6, 2, 6, 1024, _rv(_lib.RV_STUDENT, 6, dof=3.0), _rv(_lib.RV_STUDENT, 6, dof=3.0), **radar_idx)
    assert rc == 0 and 'k_particle_filter<D=6, QK=1>' in name and '107264 B' in name, name

    # ---- smoothers ----
    MARG, GEN = 0, 1
    for method in (MARG, GEN):
        a, b, text = _smoother_call(_lib.F_UNGM_DYN, 1, 1, 64, mix, method)
        assert (a, b) == (E_UNSUPPORTED, E_UNSUPPORTED) and 'dof >= 2' in text, text
        a, b, text = _smoother_call(_lib.F_UNGM_DYN, 1, 1, 64, _rv(_lib.RV_STUDENT, 1, dof=1.0), method)
        assert (a, b) == (E_UNSUPPORTED, E_UNSUPPORTED) and 'below 2' in text, text
        assert _smoother_call(_lib.F_UNGM_DYN, 1, 1, 64, _rv(_lib.RV_STUDENT, 2, dof=4.0), method)[:2] == (E_ARG, E_ARG)
    # the marginal smoother with dq != D (constant velocity, D = 4, dq = 2): no transition density
    cv = dict(par_dyn=(0.5,), G=np.array([[0.125, 0], [0.5, 0], [0, 0.125], [0, 0.5]]))
    t5 = _rv(_lib.RV_STUDENT, 2, dof=5.0)
    a, b, text = _smoother_call(14, 4, 2, 128, t5, MARG, **cv)
    assert (a, b) == (E_UNSUPPORTED, E_UNSUPPORTED) and 'singular' in text and 'genealogy' in text, text
    rc, _, name = _smoother_call(14, 4, 2, 128, t5, GEN, **cv)
    assert rc == 0 and 'k_particle_lineage<D=4>' in name and '%d B' % (8 * (2 * 128 + 96)) in name, name
    rc, _, name = _smoother_call(_lib.F_UNGM_DYN, 1, 1, 320, t4, MARG)
    assert rc == 0 and 'k_particle_smooth<D=1, QK=1>' in name and '%d B' % (8 * (4 * 320 + 96)) in name, name
    rc, _, name = _smoother_call(_lib.F_UNGM_DYN, 1, 1, 320, gauss, MARG)
    assert rc == 0 and 'k_particle_smooth<D=1>' in name and 'QK' not in name, name


def test_python_refusals_and_acceptances():
    from ssmtoybox_amd import ssinf, ssmod as sm
    dyn_g, obs_g = po.package_models('ungm')
    assert ssinf.BootstrapParticleFilter(dyn_g, obs_g, num_particles=320).kernel_name().startswith('k_particle_filter<D=1> ')
    for name, Ns in ho.CASES.items():
        dyn, obs = ho.package_models(name)
        pf = ssinf.BootstrapParticleFilter(dyn, obs, num_particles=Ns[-1])
        D = dyn.dim_state
        assert 'k_particle_filter<D=%d, QK=1>' % D in pf.kernel_name()
        assert 'k_particle_lineage<D=%d>' % D in pf.smoother_kernel_name('genealogy')
        if 'marginal' in ho.METHODS[name]:
            assert 'k_particle_smooth<D=%d, QK=1>' % D in pf.smoother_kernel_name('marginal')
        else:
            with pytest.raises(NotImplementedError, match='singular'):
                pf.smoother_kernel_name('marginal')
    # a StudentRV initial state: the plane holds the scale matrix, not the covariance
    dyn, obs = ho.package_models('cv_radar_t')
    pf = ssinf.BootstrapParticleFilter(dyn, obs, num_particles=128)
    assert np.array_equal(pf.x0_cov, ho.case('cv_radar_t')[2]) and np.array_equal(pf.x0_mean, ho.case('cv_radar_t')[1])
    # one side each
    one = sm.UNGMTransition(sm.GaussRV(1), sm.StudentRV(1, scale=[[10.0]]))
    assert 'QK=1' in ssinf.BootstrapParticleFilter(one, obs_g, num_particles=64).kernel_name()
    one = sm.UNGMTransition(sm.StudentRV(1), sm.GaussRV(1, cov=[[10.0]]))
    assert 'QK=1' in ssinf.BootstrapParticleFilter(one, obs_g, num_particles=64).kernel_name()
    # refusals: mixtures anywhere, and what the Gaussian filter refuses
    mix = sm.GaussianMixtureRV(1, covs=(np.eye(1), 4 * np.eye(1)), alphas=(0.5, 0.5))
    with pytest.raises(NotImplementedError, match='GaussianMixtureRV process noise'):
        ssinf.BootstrapParticleFilter(sm.UNGMTransition(sm.StudentRV(1), mix), obs_g)
    with pytest.raises(NotImplementedError, match='GaussianMixtureRV initial state'):
        ssinf.BootstrapParticleFilter(sm.UNGMTransition(mix, sm.StudentRV(1)), obs_g)
    with pytest.raises(NotImplementedError, match='GaussianMixtureRV'):
        ssinf.BootstrapParticleFilter(ho.package_models('ungm_t')[0], sm.UNGMMeasurement(mix, 1))
    dyn, obs = ho.package_models('ungm_t')
    with pytest.raises(ValueError, match='multiple of 64'):
        ssinf.BootstrapParticleFilter(dyn, obs, num_particles=100)
    with pytest.raises(NotImplementedError, match='outside the range'):
        ssinf.BootstrapParticleFilter(dyn, obs, num_particles=8192)
    for text in ('13312', 'StudentRV (dof >= 2) initial state and process noise'):
        assert text in ssinf.BootstrapParticleFilter.RANGE


@pytest.mark.parametrize('name,N', [(n, N) for n, Ns in ho.CASES.items() for N in Ns])
def test_oracle_cases_are_decidable(name, N):
    """The cases of tests/test_particle_heavy_gpu.py, oracle alone: every Gamma acceptance is decided by at least 1e-9 in its
    inequality, every ancestor by 64 N eps and every resampling decision by an ESS margin of 1e-9; at least one step resamples and one
    does not - so the GPU test may demand exact ancestors and decisions.  Seed 11 meets this in every case; no other was needed."""
    model, m0, P0, _ = ho.case(name)
    y, seed = ho.case_data(name), ho.SEEDS[name]
    did = []
    for b in range(ho.B):
        o = ho.full_pass(model, y[:, :, b], m0, P0, seed, b, N, ho.ESS_THRESHOLD)
        assert o['status'] == 0 and np.all(np.isfinite(o['fm'])) and np.all(np.isfinite(o['fP']))
        assert o['gamma_margin'] >= 1e-9, (b, o['gamma_margin'])
        assert o['anc_margin'].min() >= 64 * N * po.EPS, (b, o['anc_margin'].min())
        assert o['ess_margin'].min() >= 1e-9, (b, o['ess_margin'].min())
        assert np.all(o['anc'][:, ~o['resampled']] == np.arange(N)[:, None])
        np.testing.assert_allclose(np.exp(o['lwn']).sum(axis=0), 1.0, rtol=1e-12)
        did.extend(o['resampled'])
    assert any(did) and not all(did)


def test_gaussian_sides_are_the_gaussian_oracle():
    """With both degrees of freedom None the heavy oracle is tests/_particle_oracle.py, bit for bit."""
    model, m0, P0, _ = po.case('cv_radar')
    heavy = ho.Model(model.f, model.h, model.D, model.Y, model.q_mean, model.Lq, model.G, model.r_mean, model.Lr)
    y = po.case_data('cv_radar')[:, :, 0]
    a, b = po.full_pass(model, y, m0, P0, 11, 0, 128, 0.5), ho.full_pass(heavy, y, m0, P0, 11, 0, 128, 0.5)
    for k in ('fm', 'fP', 'x', 'lwn', 'anc'):
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize('nu', [2.0, 3.0, 4.0])
def test_sampler_distribution(nu):
    """The oracle's Student-t factor on the particle kernels' counters: z / sqrt(u) passes a Kolmogorov-Smirnov test against
    scipy.stats.t at the bar tests/test_oracle_golden.py uses for gamma_mt (p > 1e-3), for the initial draw and for the step draw."""
    stats = pytest.importorskip('scipy.stats')
    N = 4096
    for step, pz, pg in ((0, po.P_INIT, (ho.P_INIT_GN, ho.P_INIT_GU)), (3, po.P_NOISE, (ho.P_NOISE_GN, ho.P_NOISE_GU))):
        draws = []
        for traj in range(4):
            sc, margin = ho.t_factor(5, traj, step, pg, N, nu)
            draws.append(po.normals(5, traj, step, pz, N, 1)[0] * sc)
        p = stats.kstest(np.concatenate(draws), stats.t(nu).cdf).pvalue
        assert p > 1e-3, (nu, step, p)
    # the two draws of one particle do not share a stream
    a, b = ho.t_factor(5, 0, 0, (ho.P_INIT_GN, ho.P_INIT_GU), N, nu)[0], ho.t_factor(5, 0, 0, (ho.P_NOISE_GN, ho.P_NOISE_GU), N, nu)[0]
    assert not np.any(a == b)


def test_smoothing_density_long_double_twin():
    """The Student-t FFBSm of the oracle in float64 against its long-double form on a small cloud: to rounding."""
    model, m0, P0, _ = ho.case('pend_tq')
    y = ho.case_data('pend_tq')[:, :, 0]
    o = ho.full_pass(model, y, m0, P0, ho.SEEDS['pend_tq'], 0, 64, ho.ESS_THRESHOLD)
    s64, sld = ho.marginal(model, o['x'], o['lwn'], ho.T), ho.marginal(model, o['x'], o['lwn'], ho.T, dtype=ho.LD)
    big = sld['ls'] > -700
    tol = 64 * po.EPS * np.linalg.cond(ho.so.sigma(model))
    assert np.max(np.abs(s64['ls'][big] - sld['ls'][big]) / (1 + np.abs(sld['ls'][big]))) <= tol
    assert not np.array_equal(s64['sm'][:, 0], o['fm'][:, 0])
    # and it is another density than the Gaussian one
    g = ho.so.marginal(model, o['x'], o['lwn'], ho.T)
    assert np.max(np.abs(g['ls'][big] - s64['ls'][big])) > 1e-3


def test_study_gap_on_the_cpu():
    """What tests/test_particle_heavy_gpu.py::test_study relies on, established here first: UNGM with Student-t initial state,
    process noise (scale 10) and measurement noise, all of dof 4, data of the simulator's restatement aligned with the filters' time
    convention, B = 256, T = 20, N = 512; time-averaged RMSE over the batch, the standard error of each difference by a bootstrap over
    the trajectories (`po.bootstrap_se`).  Seed 11, the first tried:
        particle filter 5.7030;  Studentian filter (fully-symmetric rule, dof 4) 11.0942, gap 5.3913 = 17.5 standard errors (0.3077)
        Gaussian-noise particle filter with the matched covariances 5.9054, gap 0.2024 = 2.0 standard errors (0.1021)
    The GPU test asserts an inequality only against a competitor that loses here by at least 5 standard errors: the Studentian filter.
    The Gaussian-noise particle filter is within 5 standard errors and is not asserted against."""
    r = ho.study_cpu(ho.STUDY_SEED)
    found = {}
    for k in ('fss', 'pf_gauss'):
        d = r[k] - r['pf']
        gap, se = float(d.mean()), po.bootstrap_se(d)
        found[k] = gap / se
        print('seed %d: particle filter %.4f, %s %.4f, gap %.4f = %.1f standard errors (%.4f)' % (ho.STUDY_SEED, r['pf'].mean(), k,
                                                                                                 r[k].mean(), gap, gap / se, se))
        np.testing.assert_allclose((r[k].mean(), r['pf'].mean(), gap), ho.STUDY_FIGURES[k][:3], atol=5e-4)
    assert ho.STUDY_LOSERS == tuple(k for k in ('fss', 'pf_gauss') if found[k] >= 5.0), found
