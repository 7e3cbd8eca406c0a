"""Host side of tests/test_metrics_kernels_gpu.py: on the same cases float64 NumPy (oracle.ssmq_oracle.error_sums / lcr_sums,
tests/_bootstrap_oracle.traj_scores) meets the bound max(RTOL, 64 cond eps) against the 50-digit oracle of tests/_metrics_oracle.py -
so the bound is attainable and the case builders give what they claim - and the oracle's own bookkeeping (pool and multiplicities,
the classification case's condition on its inputs) is checked against plain loops."""
import mpmath as mp
import numpy as np
import pytest

from oracle import ssmq_oracle as orc
from tests import _bootstrap_oracle as bo
from tests import _metrics_oracle as mo


def numpy_ratios(c, floor, k0s=(0,), lcr=True, steps=None):
    """Worst ratios (sums, lcr, scores) of the NumPy restatement on a case; counts exactly."""
    x, fm, fP, ok = mo.lanes(c)
    ref, scale, cond = mo.sums_ref(c)
    s = slice(None) if steps is None else list(steps)
    es = orc.error_sums(x, fm, fP, ok)
    assert np.array_equal(es['n_ok'], ref['n_ok']) and np.array_equal(es['n_pd'], ref['n_pd'])
    a = max(mo.check(es[k][s], ref[k][s], scale[k][s], cond[k][s], floor) for k in ('se', 'rmse', 'mse', 'nll'))
    b = sc = 0.0
    if lcr:
        ls = orc.lcr_sums(x, fm, fP, c['M'], ok)
        assert np.array_equal(ls['n'][s], ref['n'][s])
        b = mo.check(ls['lcr'][s], ref['lcr'][s], scale['lcr'][s], cond['lcr'][s], floor)
        for k0 in k0s:
            got, _ = bo.traj_scores(x, fm, fP, c['M'], ok, k0)
            sc = max(sc, mo.check(got, *mo.scores_ref(c, k0), floor))
    return a, b, sc


def steps_of(c, steps):
    """The case cut down to some of its steps."""
    steps = list(steps)
    return mo.make_case(c['x'][:, steps], c['fm'][:, steps], c['fP'][:, :, steps], c['mse'][steps], idx=c['idx'], ok=c['ok'])


@pytest.mark.parametrize('cset', ('lo', 'hi'))
@pytest.mark.parametrize('D', range(1, 17))
def test_numpy_meets_bound_every_dimension(D, cset):
    c = mo.dim_case(D, cset)
    terms, m_ok, cm = mo.evaluate(c)
    conds = np.array([[e['cond'] for e in row] for row in terms])
    assert all(e['pd'] for row in terms for e in row) and all(m_ok)
    if D > 1:
        assert np.all(np.abs(conds / mo.CONDS[cset] - 1.0) < 1e-3), 'the builder gives the condition number it claims'
    r = numpy_ratios(c, cset != 'lo', k0s=(0, 1, c['T'] - 1))
    print('numpy D', D, cset, r)
    assert max(r) < mo.FACTOR, r


@pytest.mark.parametrize('D', (1, 2, 6, 7))
def test_numpy_meets_bound_pool_batches(D):
    pool = mo.pool_case(D, 2)
    for B in (1, 65, 257):           # serial summation: see the docstring of tests/_metrics_oracle.py
        ok = np.ones(B, dtype=bool)
        if B > 1:
            ok[[b for b in mo.EDGE_LANES if b < B] + [B - 1]] = False
        r = numpy_ratios(mo.with_lanes(pool, idx=mo.pool_index(B), ok=ok), False)
        print('numpy pool D', D, 'B', B, r)
        assert max(r) < mo.FACTOR, (B, r)


@pytest.mark.parametrize('D', (2, 3, 4, 5, 6, 7, 12, 16))
def test_numpy_meets_bound_not_positive_definite(D):
    c = mo.notpd_case(D)
    terms, _, _ = mo.evaluate(c)
    for t in range(c['T']):
        for i, (kind, spread) in enumerate(mo.NOTPD_KINDS):
            e, P = terms[t][mo.POOL + i], c['fP'][:, :, t, mo.POOL + i]
            assert not e['pd']
            if e['singular']:
                assert t == mo.SING_STEP and i in (mo.SING_ZERO, mo.SING_ROWCOL) and not np.all(mo.lu_pivots(P))
                continue
            lam = np.linalg.eigvalsh(P)
            assert abs(e['cond'] / spread - 1.0) < 1e-3 and np.all(mo.lu_pivots(P))
            assert np.all(lam < 0) if kind == 'negdef' else (lam.min() < 0 < lam.max())
            assert np.count_nonzero(np.abs(np.linalg.eigh(P)[1]) > 1e-3) > D * D // 2, 'dense eigenvectors'
    # NumPy's log_cred_ratio raises at a singular P: sums of the NLL over both steps, the rest on the step without such entries
    a, _, _ = numpy_ratios(c, True, lcr=False)
    _, b, sc = numpy_ratios(steps_of(c, [1 - mo.SING_STEP]), True)
    print('numpy not pd D', D, a, b, sc)
    assert max(a, b, sc) < mo.FACTOR, (a, b, sc)
    ref, _, _ = mo.sums_ref(c)
    assert ref['n_pd'][mo.SING_STEP] == c['B'] - 2 and ref['lcr'][mo.SING_STEP] == np.inf and ref['n'][mo.SING_STEP] == c['B']
    sref = mo.scores_ref(c, 0)[0]
    lanes = [mo.NOTPD_LANES[mo.SING_ZERO], mo.NOTPD_LANES[mo.SING_ROWCOL]]
    assert np.isnan(sref[D + 1, lanes]).all() and np.all(sref[D + 2, lanes] == np.inf)


@pytest.mark.parametrize('p', (100, -100))
@pytest.mark.parametrize('D', (3, 6))
def test_numpy_meets_bound_scaled(D, p):
    c0 = mo.dim_case(D, 'lo')
    c = mo.scaled_case(c0, p)
    r0, r1 = mo.sums_ref(c0)[0], mo.sums_ref(c)[0]
    assert np.array_equal(r1['se'], r0['se'] * 4.0 ** p) and np.array_equal(r1['mse'], r0['mse'] * 4.0 ** p)
    r = numpy_ratios(c, False, k0s=(0, 1))
    print('numpy scaled D', D, p, r)
    assert max(r) < mo.FACTOR, r


@pytest.mark.parametrize('D', (3, 9))
def test_oracle_mse_not_positive_definite(D):
    c0 = mo.dim_case(D, 'lo')
    mse = np.array(c0['mse'])
    mse[1] = mo.indefinite(np.random.default_rng([20254, D]), D, 1e2)
    c = mo.make_case(c0['x'], c0['fm'], c0['fP'], mse)
    with pytest.raises(np.linalg.LinAlgError):
        np.linalg.cholesky(c['M'][1])
    ref, _, _ = mo.sums_ref(c)
    assert ref['lcr'][1] == 0.0 and ref['n'][1] == 0.0 and ref['n'][0] == ref['n'][2] == c['B']
    assert np.isnan(mo.scores_ref(c, 1)[0][D + 2]).all() and np.isfinite(mo.scores_ref(c, 2)[0]).all()
    _, b, _ = numpy_ratios(steps_of(c, [0, 2]), False)
    assert b < mo.FACTOR


def test_pool_aggregation_against_plain_loop():
    """Sums with multiplicities and the gathered scores against one evaluation per lane."""
    D, B = 3, 150
    pool = mo.pool_case(D, 2)
    ok = np.ones(B, dtype=bool)
    ok[[0, 63, 64, 149]] = False
    c = mo.with_lanes(pool, idx=mo.pool_index(B), ok=ok)
    assert np.array_equal(np.sort(np.unique(c['idx'])), np.arange(mo.POOL)) and np.bincount(c['idx']).max() == 3
    x, fm, fP, _ = mo.lanes(c)
    plain = mo.make_case(x, fm, fP, c['mse'], ok=ok)                     # B entries of their own
    assert '_cache' in plain and plain['_cache'] is not pool['_cache']
    for a, b in zip(mo.sums_ref(c), mo.sums_ref(plain)):
        for k in a:
            assert np.array_equal(a[k], b[k]), k
    for a, b in zip(mo.scores_ref(c, 1), mo.scores_ref(plain, 1)):
        assert np.array_equal(a, b, equal_nan=True)
    # and the plain loop itself, term by term
    ref = mo.sums_ref(plain)[0]
    with mp.workdps(mo.DPS):
        tot = mp.mpf(0)
        for b in np.flatnonzero(ok):
            tot += mo.item_hp(x[:, 1, b], fm[:, 1, b], fP[:, :, 1, b])['nll']
        assert float(tot) == ref['nll'][1] and ref['n_ok'][1] == B - 4


@pytest.mark.parametrize('D', (2, 3, 4, 5, 6))
def test_classification_case_has_no_singular_entry(D):
    """The condition of the device test on its inputs: no float64 LU pivot is exactly zero, the covariances are rank deficient up to
    rounding, and float64 Cholesky puts entries on both sides of "positive definite"."""
    c = mo.classification_case(D)
    n_pd = 0
    for t in range(c['T']):
        for i in range(c['N']):
            P = c['fP'][:, :, t, i]
            assert mo.nonsingular_f64(P), (t, i)
            lam = np.linalg.eigvalsh(P)
            if i == 100 + t:
                assert lam.min() < -1e-3
                continue
            assert abs(lam[0]) < 1e-13 * lam[-1] and lam[1] > 1e-9 * lam[-1], 'rank D - 1 up to rounding'
            try:
                np.linalg.cholesky(P)
                n_pd += 1
            except np.linalg.LinAlgError:
                pass
    print('classification D', D, 'float64 Cholesky succeeds on', n_pd, 'of', c['T'] * (c['N'] - 1))
    assert 0.1 * c['T'] * c['N'] < n_pd < 0.9 * c['T'] * c['N']
