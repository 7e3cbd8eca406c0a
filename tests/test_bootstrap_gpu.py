"""
Bootstrap error bars on the device: the streaming resampler (csrc/ssmq_bootstrap.hip) against the exact oracle of its draw
(tests/_bootstrap_oracle.py), against theory and the reference's own value (tests/golden/g20_bootstrap.npz), and the
per-trajectory scores (k_traj_scores, csrc/ssmq_metrics.hip) against the oracle's per-item functions and the existing sums.
"""
import numpy as np
import pytest

from oracle import ssmq_oracle as orc
from tests import _bootstrap_oracle as bo

pytestmark = pytest.mark.gpu

SEED = 20261018


@pytest.fixture(scope='module')
def amd():
    import ssmtoybox_amd
    assert ssmtoybox_amd.device_count() >= 1, 'no GPU visible - the HIP path cannot run (there is no CPU fallback)'
    return ssmtoybox_amd


def _rows(data, ld):
    """(R, n_all) host rows -> DeviceBuffer [R][ld]; the lanes past n_all hold NaN, so a read outside the list shows."""
    from ssmtoybox_amd import _lib
    data = np.atleast_2d(np.asarray(data, dtype=np.float64))
    buf = np.full((data.shape[0], ld), np.nan)
    buf[:, :data.shape[1]] = data
    d = _lib.DeviceBuffer(buf.nbytes)
    d.upload(buf)
    return d


def _planes(a, ld):
    """(D, T, B) or (D, D, T, B) -> DeviceBuffer of planes [T][D..][ld]."""
    from ssmtoybox_amd import _lib
    B = a.shape[-1]
    t_ax = a.ndim - 2
    src = np.moveaxis(a, t_ax, 0).reshape(a.shape[t_ax], -1, B)
    buf = np.zeros((src.shape[0], src.shape[1], ld))
    buf[:, :, :B] = src
    d = _lib.DeviceBuffer(buf.nbytes)
    d.upload(buf)
    return d


def _status(st, ld):
    from ssmtoybox_amd import _lib
    full = np.zeros(ld, dtype=np.int32)
    full[:st.shape[0]] = st
    d = _lib.DeviceBuffer(full.nbytes)
    d.upload(full)
    return d


def _run(data, ld, B, status, S, seed=SEED):
    """var (R,), means (R, S) of bootstrap_var_dev on host rows."""
    from ssmtoybox_amd import mcshard
    data = np.atleast_2d(data)
    d = _rows(data, ld)
    try:
        return mcshard.bootstrap_var_dev(d, ld, data.shape[0], B, status, samples=S, seed=seed, return_means=True)
    finally:
        d.free()


def _check_means(means, data, idx, S, seed, which=None):
    """|mean_dev - mean_oracle| <= n 2^-53 mean|data|: the worst case of any summation order against the exact sum."""
    data = np.atleast_2d(data)
    vals = data if idx is None else data[:, idx]
    n = vals.shape[1]
    ref = np.atleast_2d(bo.resample_means(data, idx, S, seed, which))
    got = means if which is None else means[:, which]
    bound = n * 2.0 ** -53 * np.abs(vals).mean(axis=1)
    err = np.abs(got - ref).max(axis=1)
    print('n {} S {} rows {}: max |mean_dev - mean_oracle| / bound = {:.3g}'.format(n, S, data.shape[0], (err / bound).max()))
    assert np.all(err <= bound), (err, bound)


def _check_var(var, means):
    """var = numpy.var of the means to rtol 1e-12; where the means (nearly) coincide, both sides are rounding noise of the
    mean of S numbers, at most (S 2^-53 max|mean|)^2 in any summation order - the floor."""
    S = means.shape[1]
    floor = (S * 2.0 ** -53 * np.abs(means).max(axis=1)) ** 2
    assert np.all(np.abs(var - np.var(means, axis=1)) <= 1e-12 * np.var(means, axis=1) + floor), (var, np.var(means, axis=1))


@pytest.mark.parametrize('n', [1, 2, 63, 64, 65, 193, 1000])
def test_draw_exact(amd, n):
    data = np.random.default_rng(n).standard_normal(n) + 0.25
    for S in (1, 2, 257):
        var, means = _run(data, (n + 63) // 64 * 64, n, None, S)
        assert means.shape == (1, S) and var.shape == (1,)
        _check_means(means, data, None, S, SEED)
        _check_var(var, means)


@pytest.mark.parametrize('n', [193, 1000])
def test_draw_exact_index_list_with_gaps_and_rows(amd, n):
    """The included list is every third trajectory of a longer batch (ld > B > n), four rows."""
    B = 3 * n - 1
    ld = (B + 63) // 64 * 64 + 64
    data = np.random.default_rng(100 + n).standard_normal((4, B)) * np.array([[1.0], [10.0], [0.1], [1.0]]) + 0.5
    status = np.ones(B, dtype=np.int32)
    status[::3] = 0
    idx = np.flatnonzero(status == 0)
    assert idx.shape[0] == n
    for S in (2, 257):
        var, means = _run(data, ld, B, status, S)
        _check_means(means, data, idx, S, SEED)
        _check_var(var, means)


def test_rows_are_independent_and_calls_repeat(amd):
    n, S = 1000, 129
    data = np.random.default_rng(5).standard_normal((4, n))
    var4, means4 = _run(data, 1024, n, None, S)
    again = _run(data, 1024, n, None, S)
    assert np.array_equal(var4, again[0]) and np.array_equal(means4, again[1])
    for r in range(4):
        var1, means1 = _run(data[r], 1024, n, None, S)
        assert np.array_equal(means1[0], means4[r]) and np.array_equal(var1[0], var4[r])
    assert not np.array_equal(_run(data, 1024, n, None, S, seed=SEED + 1)[1], means4)


def test_two_routes_one_result(amd, monkeypatch):
    """SSMQ_BOOT_NO_LDS=1 gathers through L2 instead of staging the values in LDS: the same arithmetic, the same bits."""
    n, S = 5000, 64
    data = np.random.default_rng(6).standard_normal((3, 2 * n))
    status = np.ones(2 * n, dtype=np.int32)
    status[1::2] = 0
    monkeypatch.delenv('SSMQ_BOOT_NO_LDS', raising=False)
    var, means = _run(data, 2 * n + 112, 2 * n, status, S)
    monkeypatch.setenv('SSMQ_BOOT_NO_LDS', '1')
    var2, means2 = _run(data, 2 * n + 112, 2 * n, status, S)
    monkeypatch.delenv('SSMQ_BOOT_NO_LDS')
    assert np.array_equal(means, means2) and np.array_equal(var, var2)
    which = [0, 1, 31, 63]
    _check_means(means, data, np.flatnonzero(status == 0), S, SEED, which)


def test_beyond_the_lds_bound(amd):
    """R n 8 > 160 KiB: the gather route is the only one; several chunks of positions per resample."""
    n, S = 30000, 64
    data = np.random.default_rng(7).standard_normal(n) + 1.0
    var, means = _run(data, 30016, n, None, S)
    _check_means(means, data, None, S, SEED, [0, 1, 2, 17, 31, 32, 62, 63])
    _check_var(var, means)


def test_uniformity(amd):
    n, S = 1000, 4096
    data = np.zeros((3, n))
    data[0] = np.arange(n)
    data[1, 0] = data[2, n - 1] = 1.0
    var, means = _run(data, 1024, n, None, S)
    dev = means[0].mean() - (n - 1) / 2.0
    bound = 5.0 * np.sqrt((n * n - 1.0) / (12.0 * n * S))
    print('mean of the resample means - (n - 1) / 2 = {:+.4f} (bound {:.4f})'.format(dev, bound))
    assert abs(dev) <= bound
    assert means[0].min() >= 0.0 and means[0].max() <= n - 1.0
    assert means[1].max() > 0.0 and means[2].max() > 0.0          # entries 0 and n - 1 are drawn
    # each is drawn n S / n = S times in all, +- 5 sqrt(S): an off-by-one at either end would halve or double it
    for r in (1, 2):
        hits = means[r].sum() * n
        assert abs(hits - S) <= 5.0 * np.sqrt(S), hits


def test_against_theory_and_the_reference(amd, golden):
    from ssmtoybox_amd import utils
    g = golden('g20_bootstrap')
    S = int(g['samples'])
    assert S == 4096
    band = 5.0 * np.sqrt(2.0 / (S - 1))
    for name, data in (('normal', g['normal_data']), ('skewed', g['normal_data'] ** 2)):
        n = data.shape[0]
        var, _ = _run(data, n, n, None, S)
        r_theory, r_ref = var[0] / (np.var(data) / n) - 1.0, var[0] / float(g[name + '_var']) - 1.0
        print('{}: var_dev / (var(data) / n) - 1 = {:+.4f} (band {:.4f}); var_dev / var_ref - 1 = {:+.4f} (band {:.4f})'.format(
            name, r_theory, band, r_ref, np.sqrt(2.0) * band))
        assert abs(r_theory) <= band
        assert abs(r_ref) <= np.sqrt(2.0) * band
        assert utils.bootstrap_var(data[None, :], S, seed=SEED) == var[0]


# ---------------------------------------------------------------------------------------------------------------
# per-trajectory scores
# ---------------------------------------------------------------------------------------------------------------
T_SC, B_SC, LD_SC = 3, 193, 256


def _random_case(D, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((D, T_SC, B_SC))
    m = x + 0.5 * rng.standard_normal((D, T_SC, B_SC))
    a = rng.standard_normal((D, D, T_SC, B_SC)) / np.sqrt(D)
    P = np.einsum('ijtb,kjtb->iktb', a, a) + 0.2 * np.eye(D)[:, :, None, None]
    return x, m, P


@pytest.fixture(scope='module')
def score_cases(golden):
    """name -> (x, m, P, indefinite (T, B) mask, status (B,), mse (T, D, D) regularised).  d1: the inputs of g7_metrics
    (100 steps x 8 trajectories) laid out as 3 steps x 193 trajectories; d5: the generator of
    test_error_sums_large_batch_properties (g7_metrics has no 5-D set); d10: the run-time-sized kernel.  Each has planted
    covariances that are not positive definite (but not singular) and excluded trajectories."""
    g = golden('g7_metrics')
    n = T_SC * B_SC
    cases = {'d1': tuple(g['d1_' + k].reshape(g['d1_' + k].shape[:-2] + (-1,))[..., :n].reshape(
        g['d1_' + k].shape[:-2] + (T_SC, B_SC)).copy() for k in ('x', 'm', 'P')),
        'd5': _random_case(5, 11), 'd10': _random_case(10, 12)}
    out = {}
    for name, (x, m, P) in cases.items():
        D = m.shape[0]
        rng = np.random.default_rng(D)
        indef = np.zeros((T_SC, B_SC), dtype=bool)
        for k in range(T_SC):
            bad = rng.choice(B_SC, 5, replace=False)
            indef[k, bad] = True
            P[..., k, bad] = -P[..., k, bad] if D == 1 else (P[..., k, bad] - 2.0 * np.diag(np.arange(D) % 2)[:, :, None])
        status = np.zeros(B_SC, dtype=np.int32)
        status[[1, 64, B_SC - 1]] = (3, 1, 7)
        dx = (x - m)[..., status == 0]
        mse = np.einsum('itb,jtb->tij', dx, dx) / dx.shape[-1] + 1e-6 * np.eye(D)
        out[name] = (x, m, P, indef, status, mse)
    return out


@pytest.fixture(scope='module')
def score_refs(score_cases):
    """The oracle's scores of every case, for k0 = 0 and 1 - computed once."""
    return {(name, k0): bo.traj_scores(x, m, P, mse, status == 0, k0)
            for name, (x, m, P, indef, status, mse) in score_cases.items() for k0 in (0, 1)}


@pytest.mark.parametrize('k0', [0, 1])
@pytest.mark.parametrize('name', ['d1', 'd5', 'd10'])
def test_traj_scores(amd, score_cases, score_refs, name, k0):
    from ssmtoybox_amd import mcshard
    x, m, P, indef, status, mse = score_cases[name]
    D = m.shape[0]
    ref, scale = score_refs[name, k0]
    dd = [_planes(v, LD_SC) for v in (x, m, P)]
    d_st = _status(status, LD_SC)
    d_sc, names = mcshard.device_traj_scores(D, B_SC, LD_SC, T_SC, *dd, mse_global=mse, d_status=d_st, k0=k0, reg=0.0)
    assert names == ['rmse_{}'.format(d) for d in range(D)] + ['rmse', 'nll', 'lcr']
    sc = d_sc.download((D + 3, LD_SC))
    ok = status == 0
    assert np.all(np.isnan(sc[:, B_SC:])) and np.all(np.isnan(sc[:, :B_SC][:, ~ok])) and not np.isnan(sc[:, :B_SC][:, ok]).any()
    got, ref, scale = sc[:, :B_SC][:, ok], ref[:, ok], scale[:, ok]
    touched = indef[k0:].any(axis=0)[ok]          # trajectories with a step whose P is not positive definite
    assert touched.any() and not touched.all()
    err = np.abs(got - ref)
    for rows, what, rt_pd, rt_indef, floor in ((slice(0, D + 1), 'rmse', 1e-12, 1e-12, 0.0),
                                               (slice(D + 1, D + 2), 'nll', 1e-11, 1e-9, 0.0),
                                               (slice(D + 2, D + 3), 'lcr', 1e-9, 1e-8, 1.0)):
        # the bars of the existing sums' tests (rtol 1e-12 / 1e-11 / 1e-9, 1e-9 / 1e-8 where P is not positive definite;
        # the lcr with an equal atol), relative to the mean of the absolute per-step terms: a mean over three steps can
        # cancel where a sum over a batch does not
        for mask, rt in ((~touched, rt_pd), (touched, rt_indef)):
            rel = (err[rows][:, mask] / (scale[rows][:, mask] + floor)).max()
            print('{} k0 {} {} ({}): max error / scale = {:.3g} (bar {:g})'.format(
                name, k0, what, 'P positive definite' if mask is not touched else 'some P not', rel, rt))
            assert rel <= rt
    # a call without MSE matrices: the same rows, NaN in the lcr row
    d_sc2, _ = mcshard.device_traj_scores(D, B_SC, LD_SC, T_SC, *dd, d_status=d_st, k0=k0)
    sc2 = d_sc2.download((D + 3, LD_SC))
    assert np.array_equal(sc2[:D + 2], sc[:D + 2], equal_nan=True) and np.all(np.isnan(sc2[D + 2]))
    if k0 == 0:
        # consistency with the existing sums over the Monte-Carlo axis
        s1 = mcshard.device_error_sums(D, B_SC, LD_SC, T_SC, *dd, d_st)
        s2 = mcshard.device_lcr_sums(D, B_SC, LD_SC, T_SC, *dd, mse, d_st, reg=0.0)
        assert np.all(s1['n_pd'] == ok.sum()) and np.all(s2['n'] == ok.sum())
        for row, total in ((D, s1['rmse'].sum()), (D + 1, s1['nll'].sum()), (D + 2, s2['lcr'].sum())):
            mine = (T_SC * got[row]).sum()
            print('{} row {}: T sum(scores) / sum(sums) - 1 = {:+.3g}'.format(name, row, mine / total - 1.0))
            assert np.isclose(mine, total, rtol=1e-11, atol=0.0)
        assert np.allclose((T_SC * got[:D] ** 2).sum(axis=1), s1['se'].sum(axis=0), rtol=1e-12)
    for buf in dd + [d_st, d_sc, d_sc2]:
        buf.free()


def test_study_end_to_end(amd):
    """simulate -> filter -> score bars, all on the device (the chain of the README's Monte-Carlo study)."""
    from ssmtoybox_amd import ssmod, ssinf, mcshard, utils
    B, T, S, k0 = 256, 20, 512, 1
    dyn = ssmod.UNGMTransition(ssmod.GaussRV(1), ssmod.GaussRV(1, cov=np.array([[10.0]])))
    obs = ssmod.UNGMMeasurement(ssmod.GaussRV(1), 1)
    d_x, d_y, ld = ssmod.simulate_dev(dyn, obs, T, B, seed=1)
    alg = ssinf.UnscentedKalman(dyn, obs)
    d_fm, d_fP, d_st = alg.forward_pass_dev(d_y, B, ld, T)
    bars = mcshard.device_score_bars(1, B, ld, T, d_x, d_fm, d_fP, d_st, samples=S, seed=SEED, k0=k0)
    assert list(bars) == ['rmse_0', 'rmse', 'nll', 'lcr']
    status = d_st.download((B,), dtype=np.int32)
    ok = status == 0
    assert ok.sum() > B // 2
    mse = mcshard.finalize(mcshard.device_error_sums(1, B, ld, T, d_x, d_fm, d_fP, d_st))['mse']
    d_sc, names = mcshard.device_traj_scores(1, B, ld, T, d_x, d_fm, d_fP, mse, d_st, k0)
    sc = d_sc.download((4, ld))[:, :B][:, ok]
    var = mcshard.bootstrap_var_dev(d_sc, ld, 4, B, status, samples=S, seed=SEED)
    for r, nm in enumerate(names):
        assert bars[nm]['mean'] == np.mean(sc[r]) and bars[nm]['var'] == var[r] and bars[nm]['bar'] == 2.0 * np.sqrt(var[r])
        assert np.isfinite(bars[nm]['mean']) and bars[nm]['var'] > 0.0
        # the host-array entry point on the downloaded row of included scores: the same draws, the same variance
        assert utils.bootstrap_var(sc[r][None, :], S, seed=SEED) == var[r]
        # and it is a bootstrap variance of that row: within the five-sigma band of var(row) / n
        assert abs(var[r] / (np.var(sc[r]) / sc.shape[1]) - 1.0) <= 5.0 * np.sqrt(2.0 / (S - 1))
    for buf in (d_x, d_y, d_fm, d_fP, d_st, d_sc):
        buf.free()
