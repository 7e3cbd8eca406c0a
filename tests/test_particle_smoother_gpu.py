"""The particle smoothers on the device (k_particle_smooth<D>, k_particle_lineage<D>) against their NumPy restatement
(tests/_particle_smoother_oracle.py), started from the DEVICE's own cloud, and the properties of a smoother pass: step T-1 is the
filter's, the bits do not depend on the batch, the route or the block size, failures stay local, the results go through the scores."""
import functools

import numpy as np
import pytest

from tests import _particle_oracle as po
from tests import _particle_smoother_oracle as so
from tests._cases import RTOL, assert_moments_close

pytestmark = pytest.mark.gpu

CASE_IDS = [(n, N, m) for n, Ns in so.CASES.items() for N in Ns for m in so.METHODS[n]]
# (case, N, quantity, bound): bounds beyond the rule of test_parity, each 4 x the float64 restatement's own error against its
# long-double form on the same inputs - none was needed
MEASURED = ()


def _filter(name, N, seed=so.SEED):
    from ssmtoybox_amd import ssinf
    dyn, obs = so.package_models(name)
    return ssinf.BootstrapParticleFilter(dyn, obs, num_particles=N, ess_threshold=so.ESS_THRESHOLD, seed=seed)


def _outputs(pf, method):
    out = dict(sm=pf.sm_mean, sP=pf.sm_cov, ess_s=pf.ess_smooth, fm=pf.fi_mean, fP=pf.fi_cov, ll=pf.loglik, ess=pf.ess, status=pf.status,
               x=pf.particles, lwn=pf.log_weights, anc=pf.ancestors, ls=pf.smoothed_log_weights)
    if method == 'genealogy':
        out.update(lineage=pf.lineage, unique=pf.unique)
    return out


@functools.lru_cache(maxsize=None)
def _run(name, N, method):
    """One smoother pass with the cloud kept, shared by the tests (read-only)."""
    pf = _filter(name, N)
    y = so.case_data(name)
    pf.smoother_batch(y, method=method, return_particles=True)
    out = dict(y=y, **_outputs(pf, method))
    for v in out.values():
        v.setflags(write=False)
    return out


def _bound(case_key, quantity, rule):
    for name, N, q, bound in MEASURED:
        if (name, N) == case_key and q == quantity:
            return max(rule, bound)
    return rule


@pytest.mark.parametrize('name,N,method', CASE_IDS)
def test_parity(name, N, method):
    """Every case and method: the device's smoothed log-weights, moments and lineages against the oracle's, from the device's cloud."""
    model, m0, P0, _ = so.case(name)
    g = _run(name, N, method)
    assert not g['status'].any()
    assert g['sm'].shape == (model.D, so.T, so.B) and g['sP'].shape == (model.D, model.D, so.T, so.B) and g['ess_s'].shape == (so.T, so.B)
    assert g['ls'].shape == (N, so.T, so.B)
    tol = max(RTOL, 64 * so.EPS * np.linalg.cond(so.sigma(model))) if method == 'marginal' else RTOL
    worst = dict(ls=0.0, moments=0.0)
    for b in range(so.B):
        x, lwn, anc = g['x'][..., b], g['lwn'][..., b], g['anc'][..., b]
        if method == 'marginal':
            ref = so.marginal(model, x, lwn, so.T)
        else:
            ref = so.genealogy(x, lwn, anc, so.T)
            assert np.array_equal(g['lineage'][..., b], ref['idx']), b
            assert np.array_equal(g['unique'][:, b], ref['unique']), b
        big = ref['ls'] > -700
        assert np.all(np.isfinite(g['ls'][..., b][big]))
        err = float(np.max(np.abs(g['ls'][..., b][big] - ref['ls'][big]) / (1 + np.abs(ref['ls'][big]))))
        worst['ls'] = max(worst['ls'], err)
        print(name, N, method, b, 'ls', err)
        assert err <= _bound((name, N), 'ls', tol), (b, err)
        for k in range(so.T):
            xk = x[:, :, k] if method == 'marginal' else x[:, ref['idx'][:, k], k]
            cov_in = np.atleast_2d(np.cov(xk) if model.D > 1 else np.array([[np.var(xk)]]))
            e = assert_moments_close((g['sm'][:, k, b], g['sP'][:, :, k, b], np.array([g['ess_s'][k, b]])),
                                     (ref['sm'][:, k], ref['sP'][:, :, k], np.array([ref['ess'][k]])), cov_in,
                                     rtol=_bound((name, N), 'moments', tol), what=(name, N, method, b, k))
            worst['moments'] = max(worst['moments'], e)
    print(name, N, method, 'largest errors', worst, 'bound', tol)


@pytest.mark.parametrize('name,N,method', CASE_IDS)
def test_last_step_is_the_filters(name, N, method):
    g = _run(name, N, method)
    last = so.T - 1
    assert np.array_equal(g['sm'][:, last], g['fm'][:, last]) and np.array_equal(g['sP'][:, :, last], g['fP'][:, :, last])
    assert np.array_equal(g['ess_s'][last], g['ess'][last]) and np.array_equal(g['ls'][:, last], g['lwn'][:, last])
    # and the forward pass is forward_pass_batch's
    pf = _filter(name, N)
    fm, fP = pf.forward_pass_batch(g['y'], return_particles=True)
    assert np.array_equal(fm, g['fm']) and np.array_equal(fP, g['fP']) and np.array_equal(pf.loglik, g['ll'])
    assert np.array_equal(pf.particles, g['x']) and np.array_equal(pf.log_weights, g['lwn']) and np.array_equal(pf.ancestors, g['anc'])
    if method == 'marginal':       # smoothing changes something before the last step
        assert not np.array_equal(g['sm'][:, 0], g['fm'][:, 0])


@pytest.mark.parametrize('name,N,method', [('ungm', 320, 'marginal'), ('ct', 128, 'marginal'), ('cv_radar', 128, 'genealogy')])
def test_bits(name, N, method):
    from ssmtoybox_amd import _lib
    g = _run(name, N, method)
    y = g['y']
    Y, T, B = y.shape
    pf = _filter(name, N)
    D = pf.mod_dyn.dim_state
    keys = ('sm', 'sP', 'ess_s', 'fm', 'fP', 'ess', 'x', 'lwn', 'anc', 'ls') + (('lineage', 'unique') if method == 'genealogy' else ())
    # twice, and without the cloud
    pf.smoother_batch(y, method=method, return_particles=True)
    o = _outputs(pf, method)
    for k in keys:
        assert np.array_equal(o[k], g[k], equal_nan=True), k
    sm, sP = pf.smoother_batch(y, method=method)
    assert np.array_equal(sm, g['sm']) and np.array_equal(sP, g['sP']) and pf.particles is None and pf.smoothed_log_weights is None
    # blocks of 2 trajectories (2, 2, 1): the same bits as one block
    two = (8 * (D + 1) + 4) * T * N * 2
    assert pf.cloud_block(T, B, two) == 2
    pf.smoother_batch(y, method=method, return_particles=True, cloud_bytes=two)
    o = _outputs(pf, method)
    for k in keys:
        assert np.array_equal(o[k], g[k], equal_nan=True), ('blocks of 2', k)
    # smoother_dev, in one block and in blocks of 2
    ld = 64
    d_y = _lib.DeviceBuffer(8 * T * Y * ld)
    _lib.upload_study(y, Y, ld, d_y)
    for cloud_bytes in (2 ** 30, two):
        d_sm, d_sP, d_st = pf.smoother_dev(d_y, B, ld, T, method=method, cloud_bytes=cloud_bytes)
        assert np.array_equal(_lib.download_study(d_sm, (D,), T, B, ld), g['sm'])
        assert np.array_equal(_lib.download_study(d_sP, (D, D), T, B, ld), g['sP'])
        assert not d_st.download((ld,), dtype=np.int32)[:B].any()
        assert np.array_equal(pf.d_ess_smooth.download((T, ld))[:, :B], g['ess_s'])
        assert np.array_equal(pf.d_loglik.download((T + 1, ld))[:T, :B], g['ll']) and np.array_equal(pf.d_ess.download((T, ld))[:, :B], g['ess'])
        for buf in (d_sm, d_sP, d_st):
            buf.free()
    # trajectory 3 alone, at its global index
    d_y3 = _lib.DeviceBuffer(8 * T * Y * ld)
    _lib.upload_study(np.ascontiguousarray(y[:, :, 3:4]), Y, ld, d_y3)
    d_sm, d_sP, d_st = pf.smoother_dev(d_y3, 1, ld, T, method=method, traj_offset=3)
    assert np.array_equal(_lib.download_study(d_sm, (D,), T, 1, ld)[..., 0], g['sm'][..., 3])
    assert np.array_equal(_lib.download_study(d_sP, (D, D), T, 1, ld)[..., 0], g['sP'][..., 3])
    pf.free_dev()
    assert pf.d_ess_smooth is None and pf.d_loglik is None
    for buf in (d_sm, d_sP, d_st, d_y, d_y3):
        buf.free()
    # smoother is trajectory 0 of a batch of one
    s1, P1 = pf.smoother(y[:, :, 0], method)
    assert np.array_equal(s1, g['sm'][..., 0]) and np.array_equal(P1, g['sP'][..., 0])


@pytest.mark.parametrize('name,N,method', [('ct', 128, 'marginal'), ('cv_radar', 128, 'genealogy')])
def test_failure_is_local(name, N, method):
    g = _run(name, N, method)
    y = g['y'].copy()
    y[:, 2, 1] = np.nan
    pf = _filter(name, N)
    with pytest.raises(np.linalg.LinAlgError):
        pf.smoother_batch(y, method=method)
    pf.smoother_batch(y, method=method, raise_on_failure=False, return_particles=True)
    assert list(pf.status) == [0, 3, 0, 0, 0]
    o = _outputs(pf, method)
    keep = [0, 2, 3, 4]
    for k in ('sm', 'sP', 'ess_s', 'ls'):
        assert np.all(np.isnan(o[k][..., 1])), k                               # every step, the ones before the failure included
        assert np.array_equal(o[k][..., keep], g[k][..., keep]), k
    assert np.all(np.isnan(o['fm'][:, 2:, 1])) and np.array_equal(o['fm'][:, :2, 1], g['fm'][:, :2, 1])
    if method == 'genealogy':
        assert np.all(o['lineage'][..., 1] == -1) and np.all(o['unique'][:, 1] == -1)
        assert np.array_equal(o['lineage'][..., keep], g['lineage'][..., keep]) and np.array_equal(o['unique'][:, keep], g['unique'][:, keep])


def test_scores_plumbing():
    """mcshard.device_error_sums / device_traj_scores take the triple of smoother_dev unchanged (B = 70 in blocks of 32, 32, 6)."""
    from ssmtoybox_amd import _lib, mcshard, ssmod as sm
    dyn, obs = so.package_models('cv_radar')
    B, T, D, N = 70, 5, 4, 128
    d_x, d_y, ld = sm.simulate_dev(dyn, obs, T, B, seed=3)
    pf = _filter('cv_radar', N)
    cloud_bytes = (8 * (D + 1) + 4) * T * N * 32
    assert pf.cloud_block(T, B, cloud_bytes) == 32
    d_sm, d_sP, d_st = pf.smoother_dev(d_y, B, ld, T, method='genealogy', cloud_bytes=cloud_bytes)
    x = _lib.download_study(d_x, (D,), T, B, ld)
    sm_, sP_ = _lib.download_study(d_sm, (D,), T, B, ld), _lib.download_study(d_sP, (D, D), T, B, ld)
    assert not d_st.download((ld,), dtype=np.int32)[:B].any() and np.all(np.isfinite(sm_)) and np.all(np.isfinite(sP_))
    sums = mcshard.device_error_sums(D, B, ld, T, d_x, d_sm, d_sP, d_st)
    err = x - sm_
    np.testing.assert_allclose(sums['se'], (err ** 2).sum(axis=2).T, rtol=1e-10)
    assert np.all(sums['n_ok'] == B)
    d_sc, names = mcshard.device_traj_scores(D, B, ld, T, d_x, d_sm, d_sP, None, d_st)
    sc = d_sc.download((len(names), ld))[:, :B]
    np.testing.assert_allclose(sc[:D], np.sqrt((err ** 2).mean(axis=1)), rtol=1e-10)
    np.testing.assert_allclose(sc[D], np.sqrt((err ** 2).sum(axis=0)).mean(axis=0), rtol=1e-10)
    # one block gives the same planes
    d_sm1, d_sP1, d_st1 = pf.smoother_dev(d_y, B, ld, T, method='genealogy')
    assert np.array_equal(_lib.download_study(d_sm1, (D,), T, B, ld), sm_) and np.array_equal(_lib.download_study(d_sP1, (D, D), T, B, ld), sP_)
    pf.free_dev()
    for buf in (d_x, d_y, d_sm, d_sP, d_st, d_sc, d_sm1, d_sP1, d_st1):
        buf.free()


def test_smoothing_beats_filtering():
    """UNGM, `simulate_dev`, the sizes of tests/test_particle_gpu.py::test_better_filter_than_the_ukf (B = 256, T = 20, N = 512) on
    planes aligned with the filters' time convention: the particle smoother's time-averaged RMSE over the batch is below the particle
    filter's on the same planes.  Established on the CPU first (tests/test_particle_smoother_host.py::
    test_smoothing_beats_filtering_on_the_cpu: filtered 4.5523, smoothed 1.7529, 30.0 bootstrap standard errors at these sizes).  The
    UnscentedKalman's iterated smoother (IPLS, 3 iterations) on the same planes is printed beside it, not asserted."""
    from ssmtoybox_amd import mcshard, ssinf, ssmod as sm
    dyn, obs = po.package_models('ungm')
    B, T, N, seed = (po.STUDY[k] for k in ('B', 'T', 'N', 'seed'))
    d_x, d_y, ld = sm.simulate_dev(dyn, obs, T + 1, B, seed=seed)
    x1, y1 = d_x.view(8 * ld), d_y.view(8 * ld)                          # D = Y = 1: one plane per step
    pf = ssinf.BootstrapParticleFilter(dyn, obs, num_particles=N, ess_threshold=po.ESS_THRESHOLD, seed=seed)
    rmse, owned = {}, [d_x, d_y]

    def score(name, d_m, d_P, d_st, asserted=True):
        assert not (asserted and d_st.download((ld,), dtype=np.int32)[:B].any()), name
        d_sc, names = mcshard.device_traj_scores(1, B, ld, T, x1, d_m, d_P, None, d_st)
        rmse[name] = d_sc.download((len(names), ld))[0, :B]
        owned.append(d_sc)

    trip = pf.forward_pass_dev(y1, B, ld, T)
    score('pf', *trip)
    owned.extend(trip)
    for method in ('marginal', 'genealogy'):
        trip = pf.smoother_dev(y1, B, ld, T, method=method)
        score('ps_' + method, *trip)
        owned.extend(trip)
    outs = ssinf.UnscentedKalman(dyn, obs).iterated_smoother_dev(y1, B, ld, T, 3)
    score('ipls', outs[2], outs[3], outs[7], asserted=False)
    owned.extend(outs)
    pf.free_dev()
    for buf in owned:
        buf.free()
    print('particle filter %.4f, particle smoother (marginal) %.4f, (genealogy) %.4f, UKF IPLS %.4f'
          % tuple(np.nanmean(rmse[k]) for k in ('pf', 'ps_marginal', 'ps_genealogy', 'ipls')))
    assert all(np.all(np.isfinite(v)) for k, v in rmse.items() if k != 'ipls')
    assert rmse['ps_marginal'].mean() < rmse['pf'].mean(), (rmse['ps_marginal'].mean(), rmse['pf'].mean())
