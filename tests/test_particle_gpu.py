"""The bootstrap particle filter on the device (k_particle_filter<D>) against its NumPy restatement (tests/_particle_oracle.py), step by
step from the DEVICE's own cloud, and the properties of a full pass.  tests/test_particle_host.py shows, oracle alone, that the cases
decide every ancestor by 64 N eps and every resampling decision by 1e-9, so both are compared exactly here."""
import functools

import numpy as np
import pytest

from tests import _particle_oracle as po
from tests._cases import RTOL, assert_moments_close

pytestmark = pytest.mark.gpu

CASE_IDS = [(n, N) for n, Ns in po.CASES.items() for N in Ns]
# (case, N, quantity, bound): bounds beyond the rule of the test, each 4 x the float64 restatement's own error against its
# long-double form - none was needed
MEASURED = ()


def _filter(name, N, ess_threshold=po.ESS_THRESHOLD, seed=po.SEED):
    from ssmtoybox_amd import ssinf
    dyn, obs = po.package_models(name)
    return ssinf.BootstrapParticleFilter(dyn, obs, num_particles=N, ess_threshold=ess_threshold, seed=seed)


@functools.lru_cache(maxsize=None)
def _run(name, N, ess_threshold=po.ESS_THRESHOLD, seed=po.SEED):
    """One pass with the cloud kept, shared by the tests (read-only)."""
    pf = _filter(name, N, ess_threshold, seed)
    y = po.case_data(name)
    fm, fP = pf.forward_pass_batch(y, return_particles=True)
    out = dict(y=y, fm=fm, fP=fP, ll=pf.loglik, ll_total=pf.loglik_total, ess=pf.ess, status=pf.status, x=pf.particles,
               lwn=pf.log_weights, anc=pf.ancestors)
    for v in out.values():
        v.setflags(write=False)
    return out


@pytest.mark.parametrize('name,N', CASE_IDS)
def test_step_by_step(name, N):
    model, m0, P0, _ = po.case(name)
    g = _run(name, N)
    assert not g['status'].any()
    cond_r = np.linalg.cond(model.Lr.dot(model.Lr.T))
    lw_tol = max(RTOL, 64 * po.EPS * cond_r)
    left_out = 0
    for b in range(po.B):
        x_prev, lwn_prev = po.initial_particles(model, m0, P0, po.SEED, b, N), np.full(N, -np.log(float(N)))
        for j in range(po.T + 1):
            if j == po.T:        # the ancestors chosen after the last step
                anc, did, am, em = po.resample(lwn_prev, po.SEED, b, po.T - 1, po.ESS_THRESHOLD)
                s = None
            else:
                s = po.step(model, x_prev, lwn_prev, g['y'][:, j, b], j, po.SEED, b, po.ESS_THRESHOLD, first=(j == 0))
                anc, did, am, em = s['anc'], s['resampled'], s['anc_margin'], s['ess_margin']
            if j > 0:
                dev_anc = g['anc'][:, j - 1, b]
                assert em >= 1e-9, (b, j, em)                                        # no decision is left out
                if not did:                                                          # the decision: no resampling leaves the identity
                    assert np.array_equal(dev_anc, np.arange(N)), (b, j)
                sure = am >= 64 * N * po.EPS
                left_out += int(np.sum(~sure))
                assert np.array_equal(dev_anc[sure], anc[sure]), (b, j)
            if s is None:
                break
            dx, dl = g['x'][:, :, j, b], g['lwn'][:, j, b]
            # particles: one integrand evaluation, scales as assert_moments_close takes them (largest |value| of the step)
            scale = max(float(np.max(np.abs(s['x']))), 1e-300)
            assert np.max(np.abs(dx - s['x'])) <= RTOL * scale, (b, j, np.max(np.abs(dx - s['x'])) / scale)
            assert np.max(np.abs(dl - s['lwn']) / (1 + np.abs(s['lwn']))) <= lw_tol, (b, j)
            # the moments from the device's own cloud
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


def test_full_pass_bits():
    name, N = 'ungm', 320
    g = _run(name, N)
    y = g['y']
    pf = _filter(name, N)
    fm, fP = pf.forward_pass_batch(y)                                      # without the cloud: the same bits
    assert np.array_equal(fm, g['fm']) and np.array_equal(fP, g['fP']) and pf.particles is None
    assert np.array_equal(pf.loglik, g['ll']) and np.array_equal(pf.ess, g['ess'])
    fm2, fP2 = _filter(name, N).forward_pass_batch(y)                      # twice: the same bits
    assert np.array_equal(fm2, fm) and np.array_equal(fP2, fP)
    # forward_pass_dev
    from ssmtoybox_amd import _lib
    Y, T, B = y.shape
    D, ld = 1, 64
    d_y = _lib.DeviceBuffer(8 * T * Y * ld)
    _lib.upload_study(y, Y, ld, d_y)
    d_fm, d_fP, d_st = pf.forward_pass_dev(d_y, B, ld, T)
    assert np.array_equal(_lib.download_study(d_fm, (D,), T, B, ld), fm) and np.array_equal(_lib.download_study(d_fP, (D, D), T, B, ld), fP)
    assert not d_st.download((ld,), dtype=np.int32)[:B].any()
    assert np.array_equal(pf.d_loglik.download((T + 1, ld))[:T, :B], g['ll'])
    for buf in (d_fm, d_fP, d_st):
        buf.free()
    # trajectory 3 alone, at its global index: independent of the batch around it
    d_y3 = _lib.DeviceBuffer(8 * T * Y * ld)
    _lib.upload_study(np.ascontiguousarray(y[:, :, 3:4]), Y, ld, d_y3)
    d_fm, d_fP, d_st = pf.forward_pass_dev(d_y3, 1, ld, T, traj_offset=3)
    assert np.array_equal(_lib.download_study(d_fm, (D,), T, 1, ld)[..., 0], fm[..., 3])
    assert np.array_equal(_lib.download_study(d_fP, (D, D), T, 1, ld)[..., 0], fP[..., 3])
    pf.free_dev()
    for buf in (d_fm, d_fP, d_st, d_y, d_y3):
        buf.free()
    # forward_pass is trajectory 0 of a batch of one
    f1, P1 = pf.forward_pass(y[:, :, 0])
    assert np.array_equal(f1, fm[..., 0]) and np.array_equal(P1, fP[..., 0])
    other = _run(name, N, po.ESS_THRESHOLD, po.SEED + 1)                   # another seed: another cloud
    assert not np.array_equal(other['x'], g['x']) and np.all(np.isfinite(other['fm']))


def test_thresholds():
    name, N = 'ungm', 64
    never, always = _run(name, N, 0.0), _run(name, N, 1.0)
    assert np.all(never['anc'] == np.arange(N)[:, None, None])
    assert np.mean(never['ess'][-1]) < np.mean(never['ess'][0]) and np.all(never['ess'][-1] < 0.5 * N)
    model, m0, P0, _ = po.case(name)
    for b in range(po.B):
        for j in range(1, po.T):
            # every step resampled: the log-weights after step j are -log N + log p, normalised
            lwn, _ = po.weigh(model, always['x'][:, :, j, b], np.full(N, -np.log(float(N))), always['y'][:, j, b], j)
            assert np.max(np.abs(always['lwn'][:, j, b] - lwn) / (1 + np.abs(lwn))) <= RTOL
            anc = po.resample(always['lwn'][:, j, b], po.SEED, b, j, 1.0)
            sure = anc[2] >= 64 * N * po.EPS
            assert anc[1] and np.array_equal(always['anc'][sure, j, b], anc[0][sure]) and np.sum(~sure) <= 1


def test_failure_is_local():
    name, N = 'cv_radar', 128
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


def test_scores_plumbing():
    """mcshard.device_error_sums / device_traj_scores take the triple of forward_pass_dev unchanged."""
    from ssmtoybox_amd import _lib, mcshard, ssmod as sm
    dyn, obs = po.package_models('cv_radar')
    B, T, D = 70, 5, 4
    d_x, d_y, ld = sm.simulate_dev(dyn, obs, T, B, seed=3)
    pf = _filter('cv_radar', 128)
    d_fm, d_fP, d_st = pf.forward_pass_dev(d_y, B, ld, T)
    x = _lib.download_study(d_x, (D,), T, B, ld)
    fm, fP = _lib.download_study(d_fm, (D,), T, B, ld), _lib.download_study(d_fP, (D, D), T, B, ld)
    assert not d_st.download((ld,), dtype=np.int32)[:B].any() and np.all(np.isfinite(fm))
    sums = mcshard.device_error_sums(D, B, ld, T, d_x, d_fm, d_fP, d_st)
    err = x - fm                                                            # (D, T, B)
    np.testing.assert_allclose(sums['se'], (err ** 2).sum(axis=2).T, rtol=1e-10)
    np.testing.assert_allclose(sums['rmse'], np.sqrt((err ** 2).sum(axis=0)).sum(axis=1), rtol=1e-10)
    assert np.all(sums['n_ok'] == B)
    d_sc, names = mcshard.device_traj_scores(D, B, ld, T, d_x, d_fm, d_fP, None, d_st)
    sc = d_sc.download((len(names), ld))[:, :B]
    np.testing.assert_allclose(sc[:D], np.sqrt((err ** 2).mean(axis=1)), rtol=1e-10)
    np.testing.assert_allclose(sc[D], np.sqrt((err ** 2).sum(axis=0)).mean(axis=0), rtol=1e-10)
    pf.free_dev()
    for buf in (d_x, d_y, d_fm, d_fP, d_st, d_sc):
        buf.free()


def test_better_filter_than_the_ukf():
    """It is a better filter where it should be: UNGM, `simulate_dev`, B = 256, T = 20, N = 512, the particle filter's time-averaged
    RMSE over the batch is below the UnscentedKalman's on the same measurements.  The gap was established on the CPU first
    (tests/test_particle_host.py::test_gap_to_the_ukf_on_the_cpu, seed 11): particle filter 4.5523 against 8.3312, 19.8 bootstrap
    standard errors - on data aligned with the filters' time convention: T + 1 steps are simulated and both filters get the planes
    from step 1 on, so that x_j = f(x_{j-1}, j) holds for what they filter.  On the raw T steps (x[k] = f(x[k-1], k - 1), one step
    behind the filters' time argument) the CPU gap is -0.70 = -3.4 standard errors for seed 11 and negative for seeds 1 and 2 as well:
    in that form the test was dropped, as the issue provides."""
    from ssmtoybox_amd import mcshard, ssinf, ssmod as sm
    dyn, obs = po.package_models('ungm')
    B, T, N, seed = (po.STUDY[k] for k in ('B', 'T', 'N', 'seed'))
    d_x, d_y, ld = sm.simulate_dev(dyn, obs, T + 1, B, seed=seed)
    x1, y1 = d_x.view(8 * ld), d_y.view(8 * ld)                          # D = Y = 1: one plane per step
    rmse, owned = {}, [d_x, d_y]
    pf = ssinf.BootstrapParticleFilter(dyn, obs, num_particles=N, ess_threshold=po.ESS_THRESHOLD, seed=seed)
    for name, alg in (('ukf', ssinf.UnscentedKalman(dyn, obs)), ('pf', pf)):
        d_fm, d_fP, d_st = alg.forward_pass_dev(y1, B, ld, T)
        assert not d_st.download((ld,), dtype=np.int32)[:B].any(), name
        d_sc, names = mcshard.device_traj_scores(1, B, ld, T, x1, d_fm, d_fP, None, d_st)
        rmse[name] = d_sc.download((len(names), ld))[0, :B]
        owned += [d_fm, d_fP, d_st, d_sc]
    pf.free_dev()
    for buf in owned:
        buf.free()
    print('particle filter %.4f, UKF %.4f' % (rmse['pf'].mean(), rmse['ukf'].mean()))
    assert np.all(np.isfinite(rmse['pf'])) and np.all(np.isfinite(rmse['ukf']))
    assert rmse['pf'].mean() < rmse['ukf'].mean(), (rmse['pf'].mean(), rmse['ukf'].mean())
