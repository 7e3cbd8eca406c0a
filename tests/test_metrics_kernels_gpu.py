"""The Monte-Carlo error statistics of csrc/ssmq_metrics.hip, pinned per instantiation against the 50-digit restatement of
tests/_metrics_oracle.py through mcshard.device_error_sums, device_lcr_sums and device_traj_scores (default reg):

  k_error_sums<D>, k_lcr_sums<D>, k_traj_scores<D>   D = 1..6          k_reduce_partials behind every sum
  their run-time-sized forms                          D = 7..16         k_indef_sums, traj_items_indef: the second pass

Bound: max(RTOL, 64 cond eps), the project's bound for one application of an inverse, of every value against the oracle's scale of
it (the sum of the absolute values of its terms; for a sum over the batch the sum of the entries' scales); cond = the largest
cond(P) among the entries of the value, with cond(M) for the credibility ratio, 1 for the values that apply no inverse.  The
low-condition sets drop the RTOL floor.  tests/test_metrics_kernels_host.py shows that float64 NumPy meets the same bound on the
same cases.  Counts and non-finite values are compared exactly.

Shapes: every dimension at B = 130, pitch 192, T = 3 with a distinct entry per lane and step; the batch edges around the wave (64),
the block (256) and the chunk (2048) at D = 1, 2, 6, 7 with entries drawn from a pool of 61 (the oracle adds 61 terms per step with
their multiplicities).  The padding lanes and the excluded trajectories hold NaN in every plane, as a failed filter leaves them."""
import numpy as np
import pytest

from tests import _metrics_oracle as mo
from tests._cases import within

pytestmark = pytest.mark.gpu

ALL_DIMS = tuple(range(1, 17))
EDGE_DIMS = (1, 2, 6, 7)
EDGE_B = (1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4097)
SUM_KEYS = ('se', 'rmse', 'mse', 'nll')


@pytest.fixture(scope='module')
def amd():
    import ssmtoybox_amd
    if ssmtoybox_amd.device_count() < 1:
        pytest.fail('no device: the GPU tests need an MI355X')
    ssmtoybox_amd.set_device(0)
    return ssmtoybox_amd


def run(c, ld, k0s=(0,)):
    """The three wrappers on a case at pitch ld: (error sums, lcr sums, {k0: scores (D + 3, ld)}).  The status plane is passed only
    where a trajectory is excluded, so both forms of the argument run."""
    from ssmtoybox_amd import _lib, mcshard
    bufs = []
    try:
        for a in mo.planes(c, ld):
            bufs.append(_lib.DeviceBuffer(a.nbytes))
            bufs[-1].upload(np.ascontiguousarray(a))
        d_x, d_m, d_P, d_st = bufs
        st = None if c['ok'].all() else d_st
        D, B, T = c['D'], c['B'], c['T']
        es = mcshard.device_error_sums(D, B, ld, T, d_x, d_m, d_P, d_status=st)
        ls = mcshard.device_lcr_sums(D, B, ld, T, d_x, d_m, d_P, c['mse'], d_status=st)
        scores = {}
        for k0 in k0s:
            d_sc, names = mcshard.device_traj_scores(D, B, ld, T, d_x, d_m, d_P, mse_global=c['mse'], d_status=st, k0=k0)
            bufs.append(d_sc)
            assert len(names) == D + 3
            scores[k0] = d_sc.download((D + 3, ld))
        return es, ls, scores
    finally:
        for b in bufs:
            b.free()


def sums_ratios(c, es, ls, floor=True, steps=None):
    """Counts exactly; returns (worst ratio of se / rmse / mse / nll, ratio of lcr) over `steps` (default: all)."""
    ref, scale, cond = mo.sums_ref(c)
    s = slice(None) if steps is None else list(steps)
    for k in ('n_ok', 'n_pd'):
        assert np.array_equal(es[k][s], ref[k][s]), (k, es[k], ref[k])
    assert np.array_equal(ls['n'][s], ref['n'][s]), (ls['n'], ref['n'])
    assert np.array_equal(es['n_all'], np.full(c['T'], float(c['B'])))
    assert np.array_equal(es['mse'], np.swapaxes(es['mse'], 1, 2), equal_nan=True), 'mse is exactly symmetric'
    r = {k: mo.check(es[k][s], ref[k][s], scale[k][s], cond[k][s], floor) for k in SUM_KEYS}
    print('ratios', {k: round(v, 3) for k, v in r.items()})
    return max(r.values()), mo.check(ls['lcr'][s], ref['lcr'][s], scale['lcr'][s], cond['lcr'][s], floor)


def scores_ratio(c, sc, ld, k0, floor=True):
    """Padding lanes NaN in every row; the B columns against the oracle (its NaN and inf exactly)."""
    B = c['B']
    assert np.isnan(sc[:, B:]).all(), 'padding lanes of the scores'
    ref, scale, cond = mo.scores_ref(c, k0)
    return mo.check(sc[:, :B], ref, scale, cond, floor)


# ---- every dimension ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cset', ('lo', 'hi'))
@pytest.mark.parametrize('D', ALL_DIMS)
def test_every_dimension(amd, D, cset):
    c = mo.dim_case(D, cset)
    T, floor = c['T'], cset != 'lo'
    es, ls, sc = run(c, mo.DIM_LD, k0s=(0, 1, T - 1))
    a, b = sums_ratios(c, es, ls, floor)
    s = max(scores_ratio(c, sc[k0], mo.DIM_LD, k0, floor) for k0 in sc)
    print('D', D, cset, 'sums', a, 'lcr', b, 'scores', s)
    what = ' D=%d %s' % (D, cset)
    assert within(a, mo.FACTOR, 'metrics dev sums' + what), (what, a)
    assert within(b, mo.FACTOR, 'metrics dev lcr' + what), (what, b)
    assert within(s, mo.FACTOR, 'metrics dev scores' + what), (what, s)


# ---- batch edges, padding, status ------------------------------------------------------------------------------------------------
def edge_check(c, ld, what):
    es, ls, sc = run(c, ld, k0s=(0,))
    a, b = sums_ratios(c, es, ls, floor=False)
    s = scores_ratio(c, sc[0], ld, 0, floor=False)
    assert np.isnan(sc[0][:, :c['B']][:, ~c['ok']]).all(), 'excluded trajectories of the scores'
    print(what, 'sums', a, 'lcr', b, 'scores', s)
    assert within(a, mo.FACTOR, 'metrics dev sums ' + what), (what, a)
    assert within(b, mo.FACTOR, 'metrics dev lcr ' + what), (what, b)
    assert within(s, mo.FACTOR, 'metrics dev scores ' + what), (what, s)


@pytest.mark.parametrize('T', (1, 2))
@pytest.mark.parametrize('D', EDGE_DIMS)
def test_batch_edges(amd, D, T):
    pool = mo.pool_case(D, T)
    for B in EDGE_B:
        c = mo.with_lanes(pool, idx=mo.pool_index(B))
        tight = -(-B // 64) * 64
        for ld in (tight, tight + 192):
            edge_check(c, ld, 'edges D=%d T=%d B=%d ld=%d' % (D, T, B, ld))


@pytest.mark.parametrize('D', EDGE_DIMS)
def test_status_mask(amd, D):
    pool = mo.pool_case(D, 2)
    for B in (65, 257, 2049, 4097):
        ok = np.ones(B, dtype=bool)
        ok[[b for b in mo.EDGE_LANES if b < B] + [B - 1]] = False
        c = mo.with_lanes(pool, idx=mo.pool_index(B), ok=ok)
        edge_check(c, -(-B // 64) * 64 + 64, 'status D=%d B=%d' % (D, B))
    c = mo.with_lanes(pool, idx=mo.pool_index(65), ok=np.zeros(65, dtype=bool))           # nothing left: zeros, not NaN
    es, ls, sc = run(c, 128)
    assert all(not np.any(es[k]) for k in ('se', 'rmse', 'nll', 'mse', 'n_ok', 'n_pd')) and not np.any(ls['lcr']) and not np.any(ls['n'])
    assert np.isnan(sc[0]).all()


# ---- covariances that are not positive definite ------------------------------------------------------------------------------------
@pytest.mark.parametrize('D', (2, 3, 4, 5, 6, 7, 12, 16))
def test_not_positive_definite(amd, D):
    c = mo.notpd_case(D)
    terms, _, _ = mo.evaluate(c)
    special = [terms[t][mo.POOL + i] for t in range(c['T']) for i in range(len(mo.NOTPD_LANES))]
    assert not any(e['pd'] for e in special) and sum(e['singular'] for e in special) == 2
    es, ls, sc = run(c, mo.NOTPD_LD, k0s=(0, 1))
    ref, _, _ = mo.sums_ref(c)
    # the exactly singular entries: no NLL term, counted in n_ok and in the credibility ratio's n; their ratio is +inf (the quadratic
    # form with |P| has a zero eigenvalue), and so are that step's sum and their score; their NLL score is NaN (include/ssmq.h)
    assert ref['n_pd'][mo.SING_STEP] == ref['n_ok'][mo.SING_STEP] - 2 and ref['lcr'][mo.SING_STEP] == np.inf
    a, b = sums_ratios(c, es, ls)
    for k0 in sc:
        lanes = [mo.NOTPD_LANES[mo.SING_ZERO], mo.NOTPD_LANES[mo.SING_ROWCOL]]
        assert np.isnan(sc[k0][D + 1, lanes]).all() and np.all(sc[k0][D + 2, lanes] == np.inf)
        assert np.isfinite(np.delete(sc[k0][:, :c['B']], lanes, axis=1)).all()
    s = max(scores_ratio(c, sc[k0], mo.NOTPD_LD, k0) for k0 in sc)
    print('not pd D', D, 'sums', a, 'lcr', b, 'scores', s)
    assert within(a, mo.FACTOR, 'metrics dev second pass sums D=%d' % D), a
    assert within(b, mo.FACTOR, 'metrics dev second pass lcr D=%d' % D), b
    assert within(s, mo.FACTOR, 'metrics dev second pass scores D=%d' % D), s


@pytest.mark.parametrize('D', (2, 3, 4, 5, 6))
def test_one_classification_per_entry(amd, D):
    """Every covariance numerically rank deficient, none exactly singular: whichever side of "positive definite" the streaming
    kernel puts an entry on, the second pass must put it on the same one - every entry is counted exactly once.  Values are not
    compared (ill conditioned by construction); the counts are exact.  When k_indef_sums decided for itself with chol_dense (sqrt
    and a quotient against chol_packed's sqrt_rsqrt) n_pd came out as 589 .. 644 for n_ok = 512 at every D = 2 .. 6; with
    chol_packed<D> itself in the second pass still as 515 (the same routine, inlined into other code, is contracted into other
    fused operations).  The streaming kernels now record what they leave out and the second pass reads that."""
    c = mo.classification_case(D)
    B, T = c['B'], c['T']
    es, ls, sc = run(c, B, k0s=tuple(range(T)))
    print('classification D', D, 'n_ok', es['n_ok'], 'n_pd', es['n_pd'], 'n', ls['n'])
    assert np.array_equal(es['n_ok'], np.full(T, float(B)))
    assert np.array_equal(es['n_pd'], es['n_ok']), (es['n_pd'], es['n_ok'])
    assert np.array_equal(ls['n'], es['n_ok']), (ls['n'], es['n_ok'])
    assert np.isfinite(es['nll']).all() and np.isfinite(ls['lcr']).all()
    for k0 in sc:
        assert np.isfinite(sc[k0][D + 1, :B]).sum() == B, 'k_traj_scores decides once per entry: every NLL is finite'


# ---- scale -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('p', (100, -100))
@pytest.mark.parametrize('D', (3, 6))
def test_scale(amd, D, p):
    c0 = mo.dim_case(D, 'lo')
    c = mo.scaled_case(c0, p)
    es0, _, _ = run(c0, mo.DIM_LD)
    es, ls, sc = run(c, mo.DIM_LD, k0s=(0, 1))
    s2 = 2.0 ** (2 * p)
    assert np.array_equal(es['se'], es0['se'] * s2) and np.array_equal(es['mse'], es0['mse'] * s2), 'se and mse scale exactly'
    assert np.array_equal(es['rmse'], es0['rmse'] * 2.0 ** p)
    a, b = sums_ratios(c, es, ls, floor=False)
    s = max(scores_ratio(c, sc[k0], mo.DIM_LD, k0, floor=False) for k0 in sc)
    what = ' scale D=%d p=%d' % (D, p)
    assert within(a, mo.FACTOR, 'metrics dev sums' + what), (what, a)
    assert within(b, mo.FACTOR, 'metrics dev lcr' + what), (what, b)
    assert within(s, mo.FACTOR, 'metrics dev scores' + what), (what, s)


# ---- an MSE matrix that is not positive definite ------------------------------------------------------------------------------------
@pytest.mark.parametrize('D', (3, 9))
def test_mse_not_positive_definite(amd, D):
    c0 = mo.dim_case(D, 'lo')
    mse = np.array(c0['mse'])
    mse[1] = mo.indefinite(np.random.default_rng([20254, D]), D, 1e2)
    c = mo.make_case(c0['x'], c0['fm'], c0['fP'], mse)
    T = c['T']
    es, ls, sc = run(c, mo.DIM_LD, k0s=(0, 1, 2))
    assert ls['lcr'][1] == 0.0 and ls['n'][1] == 0.0
    a, b = sums_ratios(c, es, ls, floor=False)
    for k0 in (0, 1):
        assert np.isnan(sc[k0][D + 2, :c['B']]).all() and np.isfinite(sc[k0][:D + 2, :c['B']]).all()
    assert np.isfinite(sc[2][:, :c['B']]).all()
    s = max(scores_ratio(c, sc[k0], mo.DIM_LD, k0, floor=False) for k0 in sc)
    what = ' mse not pd D=%d' % D
    assert within(a, mo.FACTOR, 'metrics dev sums' + what), (what, a)
    assert within(b, mo.FACTOR, 'metrics dev lcr' + what), (what, b)
    assert within(s, mo.FACTOR, 'metrics dev scores' + what), (what, s)
