"""The particle filter and smoothers with a Student-t initial state and process noise on the device (k_particle_filter<D, QK=1>,
k_particle_smooth<D, QK=1>) against their NumPy restatement (tests/_particle_heavy_oracle.py), step by step from the DEVICE's own
cloud; the *_rv entry points against the Gaussian ones, bit for bit; the properties of a pass; the heavy-tailed study.
tests/test_particle_heavy_host.py shows, oracle alone, that the cases decide every Gamma acceptance by 1e-9, every ancestor by 64 N eps
and every resampling decision by 1e-9, so decisions are compared exactly here."""
import ctypes
import functools

import numpy as np
import pytest

from tests import _particle_oracle as po
from tests import _particle_heavy_oracle as ho
from tests._cases import RTOL, assert_moments_close

pytestmark = pytest.mark.gpu

CASE_IDS = [(n, N) for n, Ns in ho.CASES.items() for N in Ns]
SMOOTH_IDS = [(n, N, m) for n, Ns in ho.CASES.items() for N in Ns for m in ho.METHODS[n]]
# (case, N, quantity, bound): bounds beyond the rule of the tests, each 4 x the float64 restatement's own error against its
# long-double form - none was needed
MEASURED = ()


def _filter(name, N, ess_threshold=ho.ESS_THRESHOLD, seed=None):
    from ssmtoybox_amd import ssinf
    dyn, obs = ho.package_models(name)
    return ssinf.BootstrapParticleFilter(dyn, obs, num_particles=N, ess_threshold=ess_threshold,
                                         seed=ho.SEEDS[name] if seed is None else seed)


@functools.lru_cache(maxsize=None)
def _run(name, N, seed=None):
    """One pass with the cloud kept, shared by the tests (read-only)."""
    pf = _filter(name, N, seed=seed)
    y = ho.case_data(name)
    fm, fP = pf.forward_pass_batch(y, return_particles=True)
    out = dict(y=y, fm=fm, fP=fP, ll=pf.loglik, ll_total=pf.loglik_total, ess=pf.ess, status=pf.status, x=pf.particles,
               lwn=pf.log_weights, anc=pf.ancestors)
    for v in out.values():
        v.setflags(write=False)
    return out


@pytest.mark.parametrize('name,N', CASE_IDS)
def test_step_by_step(name, N):
    model, m0, P0, _ = ho.case(name)
    seed = ho.SEEDS[name]
    g = _run(name, N)
    assert not g['status'].any()
    cond_r = np.linalg.cond(model.Lr.dot(model.Lr.T))
    lw_tol = max(RTOL, 64 * po.EPS * cond_r)
    left_out = 0
    for b in range(ho.B):
        x_prev, lwn_prev = ho.initial_particles(model, m0, P0, seed, b, N), np.full(N, -np.log(float(N)))
        for j in range(ho.T + 1):
            if j == ho.T:        # the ancestors chosen after the last step
                anc, did, am, em = po.resample(lwn_prev, seed, b, ho.T - 1, ho.ESS_THRESHOLD)
                s = None
            else:
                s = ho.step(model, x_prev, lwn_prev, g['y'][:, j, b], j, seed, b, ho.ESS_THRESHOLD, first=(j == 0))
                anc, did, am, em = s['anc'], s['resampled'], s['anc_margin'], s['ess_margin']
            if j > 0:
                dev_anc = g['anc'][:, j - 1, b]
                assert em >= 1e-9, (b, j, em)
                if not did:
                    assert np.array_equal(dev_anc, np.arange(N)), (b, j)
                sure = am >= 64 * N * po.EPS
                left_out += int(np.sum(~sure))
                assert np.array_equal(dev_anc[sure], anc[sure]), (b, j)
            if s is None:
                break
            dx, dl = g['x'][:, :, j, b], g['lwn'][:, j, b]
            scale = max(float(np.max(np.abs(s['x']))), 1e-300)
            print(name, N, b, j, 'x', np.max(np.abs(dx - s['x'])) / scale, 'lw', np.max(np.abs(dl - s['lwn']) / (1 + np.abs(s['lwn']))))
            assert np.max(np.abs(dx - s['x'])) <= RTOL * scale, (b, j, np.max(np.abs(dx - s['x'])) / scale)
            assert np.max(np.abs(dl - s['lwn']) / (1 + np.abs(s['lwn']))) <= lw_tol, (b, j)
            fm, fP, ess = po.moments(dx, dl)
            lw_carried = np.full(N, -np.log(float(N))) if (did or j == 0) else lwn_prev
            _, ll = po.weigh(model, dx, lw_carried, g['y'][:, j, b], j)
            cov_in = np.cov(dx) if model.D > 1 else np.array([[np.var(dx)]])
            assert_moments_close((g['fm'][:, j, b], g['fP'][:, :, j, b], np.array([g['ess'][j, b]])), (fm, fP, np.array([ess])),
                                 np.atleast_2d(cov_in), what=(name, N, b, j))
            assert abs(g['ll'][j, b] - ll) <= lw_tol * (1 + abs(ll)), (b, j, g['ll'][j, b], ll)
            x_prev, lwn_prev = dx, dl
        np.testing.assert_allclose(g['ll_total'][b], g['ll'][:, b].sum(), rtol=1e-13)
    assert left_out <= 1, left_out
    res = np.any(g['anc'] != np.arange(N)[:, None, None], axis=0)
    assert res.any() and not res.all()


def _gauss_rv(mean, cov):
    from ssmtoybox_amd import ssmod as sm
    return sm._rv_desc(sm.GaussRV(len(mean), mean, cov), 'test')


@pytest.mark.parametrize('name,N,method', [('ungm', 320, 'marginal'), ('cv_radar', 128, 'genealogy')])
def test_rv_entries_with_gaussian_descriptors(name, N, method):
    """All-Gaussian descriptors through ssmq_particle_filter_rv_dev / ssmq_particle_smoother_rv_dev: the bits of the Gaussian entry
    points (which BootstrapParticleFilter calls for an all-Gaussian model)."""
    from ssmtoybox_amd import _lib, ssinf
    dyn, obs = po.package_models(name)
    y = po.case_data(name)
    pf = ssinf.BootstrapParticleFilter(dyn, obs, num_particles=N, ess_threshold=po.ESS_THRESHOLD, seed=po.SEED)
    assert not pf._heavy
    pf.smoother_batch(y, method=method, return_particles=True)
    ref = dict(fm=pf.fi_mean, fP=pf.fi_cov, ll=pf.loglik, ess=pf.ess, x=pf.particles, lwn=pf.log_weights, anc=pf.ancestors,
               sm=pf.sm_mean, sP=pf.sm_cov, ess_s=pf.ess_smooth, ls=pf.smoothed_log_weights)
    lib = _lib.load()
    Y, T, B = y.shape
    D, ld = dyn.dim_state, _lib.padded(B)
    f_dyn, f_obs, r, qm, qL, keep = pf._c_args()
    x0, keep0 = _gauss_rv(dyn.init_rv.mean, dyn.init_rv.cov)
    q, keepq = _gauss_rv(dyn.noise_rv.mean, dyn.noise_rv.cov)
    vp, dp = _lib.vp, _lib.dp
    code = pf.SMOOTHER_METHODS[method]
    with _lib.Staging() as stage:
        d_y = stage.scratch(8 * T * Y * ld)
        _lib.upload_study(y, Y, ld, d_y)
        d_m0, d_P0 = pf._initial_planes(stage, B, ld)
        d = {k: stage.scratch(n) for k, n in dict(fm=8 * T * D * ld, fP=8 * T * D * D * ld, ll=8 * (T + 1) * ld, ess=8 * T * ld, st=4 * ld,
                                                   sm=8 * T * D * ld, sP=8 * T * D * D * ld, ess_s=8 * T * ld, unique=4 * T * ld,
                                                   part=8 * T * D * B * N, logw=8 * T * B * N, anc=4 * T * B * N, lws=8 * T * B * N,
                                                   lin=4 * T * B * N).items()}
        d['st'].zero()
        _lib.check(lib.ssmq_particle_filter_rv_dev(ctypes.byref(f_dyn), ctypes.byref(f_obs), D, Y, qm.size, N, B, ld, T, vp(d_y), vp(d_m0),
                                                   vp(d_P0), ctypes.byref(x0), ctypes.byref(q), dp(pf.G), ctypes.byref(r), pf.ess_threshold,
                                                   ctypes.c_uint64(pf.seed), ctypes.c_uint64(0), vp(d['fm']), vp(d['fP']), vp(d['ll']),
                                                   vp(d['ess']), vp(d['st']), vp(d['part']), vp(d['logw']), vp(d['anc'])),
                   'ssmq_particle_filter_rv_dev')
        _lib.check(lib.ssmq_particle_smoother_rv_dev(ctypes.byref(f_dyn), D, qm.size, N, B, ld, T, ctypes.byref(q), dp(pf.G), code,
                                                     vp(d['part']), vp(d['logw']), vp(d['anc']), vp(d['fm']), vp(d['fP']), vp(d['ess']),
                                                     vp(d['st']), vp(d['sm']), vp(d['sP']), vp(d['ess_s']), vp(d['lws']),
                                                     vp(d['lin']) if code == 1 else None, vp(d['unique']) if code == 1 else None),
                   'ssmq_particle_smoother_rv_dev')
        got = dict(fm=_lib.download_study(d['fm'], (D,), T, B, ld), fP=_lib.download_study(d['fP'], (D, D), T, B, ld),
                   ll=d['ll'].download((T + 1, ld))[:T, :B], ess=d['ess'].download((T, ld))[:, :B],
                   x=d['part'].download((T, D, B, N)).transpose(1, 3, 0, 2), lwn=d['logw'].download((T, B, N)).transpose(2, 0, 1),
                   anc=d['anc'].download((T, B, N), dtype=np.int32).transpose(2, 0, 1),
                   sm=_lib.download_study(d['sm'], (D,), T, B, ld), sP=_lib.download_study(d['sP'], (D, D), T, B, ld),
                   ess_s=d['ess_s'].download((T, ld))[:, :B], ls=d['lws'].download((T, B, N)).transpose(2, 0, 1))
        assert not d['st'].download((ld,), dtype=np.int32)[:B].any()
    for k in ref:
        assert np.array_equal(got[k], ref[k]), k


def test_full_pass_bits():
    name, N = 'ungm_t', 320
    g = _run(name, N)
    y = g['y']
    pf = _filter(name, N)
    fm, fP = pf.forward_pass_batch(y)                                      # without the cloud: the same bits
    assert np.array_equal(fm, g['fm']) and np.array_equal(fP, g['fP']) and pf.particles is None
    assert np.array_equal(pf.loglik, g['ll']) and np.array_equal(pf.ess, g['ess'])
    pf2 = _filter(name, N)
    fm2, fP2 = pf2.forward_pass_batch(y, return_particles=True)            # twice: the same bits
    assert np.array_equal(fm2, fm) and np.array_equal(fP2, fP) and np.array_equal(pf2.particles, g['x'])
    assert np.array_equal(pf2.ancestors, g['anc']) and np.array_equal(pf2.log_weights, g['lwn'])
    # trajectory 3 alone, at its global index: independent of the batch around it
    from ssmtoybox_amd import _lib
    Y, T, B = y.shape
    D, ld = 1, 64
    d_y3 = _lib.DeviceBuffer(8 * T * Y * ld)
    _lib.upload_study(np.ascontiguousarray(y[:, :, 3:4]), Y, ld, d_y3)
    d_fm, d_fP, d_st = pf.forward_pass_dev(d_y3, 1, ld, T, traj_offset=3)
    assert np.array_equal(_lib.download_study(d_fm, (D,), T, 1, ld)[..., 0], fm[..., 3])
    assert np.array_equal(_lib.download_study(d_fP, (D, D), T, 1, ld)[..., 0], fP[..., 3])
    pf.free_dev()
    for buf in (d_fm, d_fP, d_st, d_y3):
        buf.free()
    other = _run(name, N, ho.SEEDS[name] + 1)                              # another seed: another cloud
    assert not np.array_equal(other['x'], g['x']) and np.all(np.isfinite(other['fm']))


def test_failure_is_local():
    name, N = 'ungm_t', 320
    g = _run(name, N)
    y = g['y'].copy()
    y[:, 2, 1] = np.nan
    pf = _filter(name, N)
    with pytest.raises(np.linalg.LinAlgError):
        pf.forward_pass_batch(y)
    fm, fP = pf.forward_pass_batch(y, raise_on_failure=False)
    assert list(pf.status) == [0, 3, 0, 0, 0]
    for arr, ref in ((fm, g['fm']), (fP, g['fP']), (pf.loglik, g['ll']), (pf.ess, g['ess'])):
        assert np.all(np.isnan(arr[..., 2:, 1])) and np.array_equal(arr[..., :2, 1], ref[..., :2, 1])
        keep = [0, 2, 3, 4]
        assert np.array_equal(arr[..., keep], ref[..., keep])
    assert np.isnan(pf.loglik_total[1]) and np.array_equal(pf.loglik_total[[0, 2, 3, 4]], g['ll_total'][[0, 2, 3, 4]])


@pytest.mark.parametrize('name,N,method', SMOOTH_IDS)
def test_smoother_parity(name, N, method):
    """The structure and the bounds of tests/test_particle_smoother_gpu.py::test_parity, against the heavy oracle's FFBSm (the
    Student-t transition density) and the lineage oracle, from the device's own cloud."""
    from tests import _particle_smoother_oracle as so
    model, m0, P0, _ = ho.case(name)
    pf = _filter(name, N)
    y = ho.case_data(name)
    pf.smoother_batch(y, method=method, return_particles=True)
    g = _run(name, N)
    assert not pf.status.any()
    # the forward pass of the smoother is forward_pass_batch's; step T-1 is the filter's
    assert np.array_equal(pf.fi_mean, g['fm']) and np.array_equal(pf.particles, g['x']) and np.array_equal(pf.ancestors, g['anc'])
    last = ho.T - 1
    assert np.array_equal(pf.sm_mean[:, last], g['fm'][:, last]) and np.array_equal(pf.sm_cov[:, :, last], g['fP'][:, :, last])
    tol = max(RTOL, 64 * po.EPS * np.linalg.cond(so.sigma(model))) if method == 'marginal' else RTOL
    for b in range(ho.B):
        x, lwn, anc = pf.particles[..., b], pf.log_weights[..., b], pf.ancestors[..., b]
        if method == 'marginal':
            ref = ho.marginal(model, x, lwn, ho.T)
        else:
            ref = so.genealogy(x, lwn, anc, ho.T)
            assert np.array_equal(pf.lineage[..., b], ref['idx']), b
            assert np.array_equal(pf.unique[:, b], ref['unique']), b
        ls = pf.smoothed_log_weights[..., b]
        big = ref['ls'] > -700
        assert np.all(np.isfinite(ls[big]))
        err = float(np.max(np.abs(ls[big] - ref['ls'][big]) / (1 + np.abs(ref['ls'][big]))))
        print(name, N, method, b, 'ls', err, 'bound', tol)
        assert err <= tol, (b, err)
        for k in range(ho.T):
            xk = x[:, :, k] if method == 'marginal' else x[:, ref['idx'][:, k], k]
            cov_in = np.atleast_2d(np.cov(xk) if model.D > 1 else np.array([[np.var(xk)]]))
            assert_moments_close((pf.sm_mean[:, k, b], pf.sm_cov[:, :, k, b], np.array([pf.ess_smooth[k, b]])),
                                 (ref['sm'][:, k], ref['sP'][:, :, k], np.array([ref['ess'][k]])), cov_in, rtol=tol,
                                 what=(name, N, method, b, k))
    if method == 'marginal':
        assert not np.array_equal(pf.sm_mean[:, 0], g['fm'][:, 0])


def test_marginal_smoother_refused_for_singular_noise():
    pf = _filter('cv_radar_t', 128)
    with pytest.raises(NotImplementedError, match='singular'):
        pf.smoother_batch(ho.case_data('cv_radar_t'), method='marginal')


def test_study():
    """The heavy-tailed study: UNGM with Student-t initial state, process noise (scale 10) and measurement noise, dof 4;
    `simulate_dev` -> the particle filter and FullySymmetricStudent -> `device_traj_scores`, on planes aligned with the filters' time
    convention (T + 1 steps simulated, both filters get the planes from step 1 on), B = 256, T = 20, N = 512.  The inequality is the
    one tests/test_particle_heavy_host.py::test_study_gap_on_the_cpu established on the CPU (seed 11; `ho.STUDY_FIGURES`): the
    particle filter's time-averaged RMSE is below FullySymmetricStudent's."""
    from ssmtoybox_amd import mcshard, ssinf, ssmod as sm
    dyn, obs = ho.package_models('ungm_t')
    B, T, N = (ho.STUDY[k] for k in ('B', 'T', 'N'))
    seed = ho.STUDY_SEED
    d_x, d_y, ld = sm.simulate_dev(dyn, obs, T + 1, B, seed=seed)
    x1, y1 = d_x.view(8 * ld), d_y.view(8 * ld)                          # D = Y = 1: one plane per step
    rmse, owned = {}, [d_x, d_y]
    pf = ssinf.BootstrapParticleFilter(dyn, obs, num_particles=N, ess_threshold=ho.ESS_THRESHOLD, seed=seed)
    assert 'QK=1' in pf.kernel_name()
    for name, alg in (('fss', ssinf.FullySymmetricStudent(dyn, obs, dof=4.0)), ('pf', pf)):
        d_fm, d_fP, d_st = alg.forward_pass_dev(y1, B, ld, T)
        assert not d_st.download((ld,), dtype=np.int32)[:B].any(), name
        d_sc, names = mcshard.device_traj_scores(1, B, ld, T, x1, d_fm, d_fP, None, d_st)
        rmse[name] = d_sc.download((len(names), ld))[0, :B]
        owned += [d_fm, d_fP, d_st, d_sc]
    pf.free_dev()
    for buf in owned:
        buf.free()
    print('particle filter %.4f, FullySymmetricStudent %.4f' % (rmse['pf'].mean(), rmse['fss'].mean()))
    assert np.all(np.isfinite(rmse['pf'])) and np.all(np.isfinite(rmse['fss']))
    for loser in ho.STUDY_LOSERS:
        assert loser == 'fss'            # the Gaussian-noise particle filter is a competitor of the CPU study only
        assert rmse['pf'].mean() < rmse[loser].mean(), (rmse['pf'].mean(), rmse[loser].mean())
