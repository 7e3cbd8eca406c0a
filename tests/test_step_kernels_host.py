"""The step oracle (tests/_step_oracle.py) against the float64 NumPy/SciPy restatements of the oracle package, on exactly the case
tables the device tests use (tests/test_step_kernels_gpu.py): a correct float64 implementation meets the bound max(RTOL, 64 cond eps)
- componentwise, per item, without the RTOL floor on the low-condition sets - on these very inputs.  A case NumPy could not meet the
bound on would be an ill-chosen case, to be changed; the factor stays.

Measured here (largest |error| / scale in units of cond eps, NumPy against the 50-digit restatement): see the figures recorded by
tests/_cases.py::within under 'step host ...'."""
import numpy as np
import pytest

from oracle import ssmq_oracle as orc
from tests import _step_oracle as so
from tests._cases import within


def numpy_update(c):
    out = [orc.kalman_update(c['m_pr'][b], c['P_pr'][b], c['y_mean'][b], c['P_y'][b], c['P_yx'][b], c['y'][b])
           for b in range(c['m_pr'].shape[0])]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def numpy_rts(c):
    out = [orc.rts_smoother(c['fm'][b], c['fP'][b], c['pm'][b], c['pP'][b], c['pC'][b]) for b in range(c['fm'].shape[0])]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


@pytest.mark.parametrize('cset', sorted(so.UPDATE_CONDS))
@pytest.mark.parametrize('D,Y', so.TABLE_PAIRS + so.GENERIC_PAIRS)
def test_numpy_update_meets_the_bound(D, Y, cset):
    c, (m, P, m_sc, P_sc) = so.update_table(D, Y, cset)
    assert np.all(c['cond'] <= so.UPDATE_CONDS[cset] * 1.001) and (Y == 1 or np.all(c['cond'] >= so.UPDATE_CONDS[cset] * 0.999))
    m_np, P_np = numpy_update(c)
    floor = cset != 'lo'
    rm, rP = so.ratio(m_np, m, m_sc, c['cond'], floor), so.ratio(P_np, P, P_sc, c['cond'], floor)
    print('update (%d,%d) %s: numpy / (cond eps): mean %.3g cov %.3g' % (D, Y, cset, rm, rP))
    assert within(rm, so.FACTOR, 'step host update mean (%d,%d) %s' % (D, Y, cset))
    assert within(rP, so.FACTOR, 'step host update cov (%d,%d) %s' % (D, Y, cset))


@pytest.mark.parametrize('cset', sorted(so.RTS_CONDS))
@pytest.mark.parametrize('D', so.RTS_DIMS)
def test_numpy_rts_meets_the_bound(D, cset):
    c, (sm, sP, m_sc, P_sc) = so.rts_table(D, cset)
    assert np.all(c['cond'] <= so.RTS_CONDS[cset] * 1.001)
    assert np.all(np.isfinite(sm)) and np.all(np.isfinite(sP))          # the NaN elements 0 and T - 1 of pm, pP, pC are never read
    sm_np, sP_np = numpy_rts(c)
    floor, steps = cset != 'lo', so.RTS_T - 2
    rm, rP = so.ratio(sm_np, sm, m_sc, c['cond'], floor, steps), so.ratio(sP_np, sP, P_sc, c['cond'], floor, steps)
    print('rts D=%d %s: numpy / (steps cond eps): mean %.3g cov %.3g' % (D, cset, rm, rP))
    assert within(rm, so.FACTOR, 'step host rts mean D=%d %s' % (D, cset))
    assert within(rP, so.FACTOR, 'step host rts cov D=%d %s' % (D, cset))


def test_update_oracle_is_the_stated_formula():
    """The restatement against mpmath's own matrix algebra (LU inverse), and the scales against their definition."""
    import mpmath as mp
    rng = np.random.default_rng(5)
    c = so.update_case(rng, 4, 3, 2, 1e4)
    for b in range(2):
        m, P, m_sc, P_sc = so.kalman_update_hp(*(c[k][b] for k in ('m_pr', 'P_pr', 'y_mean', 'P_y', 'P_yx', 'y')))
        with mp.workdps(so.DPS):
            Py, Pyx = mp.matrix(c['P_y'][b].tolist()), mp.matrix(c['P_yx'][b].tolist())
            G = (mp.inverse(Py) * Pyx).T
            mm = mp.matrix(c['m_pr'][b].tolist()) + G * (mp.matrix(c['y'][b].tolist()) - mp.matrix(c['y_mean'][b].tolist()))
            PP = mp.matrix(c['P_pr'][b].tolist()) - G * Py * G.T
            Gf = np.abs(np.array(G.tolist(), dtype=float))
            assert np.array_equal(m, np.array([float(v) for v in mm]))
            assert np.array_equal(P, np.array(PP.tolist(), dtype=float))
        assert not np.array_equal(P, P.T)                                # left unsymmetrised
        np.testing.assert_allclose(m_sc, np.abs(c['m_pr'][b]) + Gf.dot(np.abs(c['y'][b] - c['y_mean'][b])), rtol=1e-12)
        np.testing.assert_allclose(P_sc, np.abs(c['P_pr'][b]) + Gf.dot(np.abs(c['P_y'][b])).dot(Gf.T), rtol=1e-12)
    assert abs(so.cond_hp(c['P_y'][0]) / np.linalg.cond(c['P_y'][0]) - 1.0) < 1e-9


def test_rts_oracle_time_edges():
    """T = 1, 2: smoothed = filtered; T = 3: only element 0 moves; the gain of the built cases is the prescribed A_k."""
    rng = np.random.default_rng(6)
    for T in (1, 2):
        c = so.rts_case(rng, 3, T, 1, 10.0)
        sm, sP, _, _ = so.rts_backward_hp(*(c[k][0] for k in ('fm', 'fP', 'pm', 'pP', 'pC')))
        assert np.array_equal(sm, c['fm'][0]) and np.array_equal(sP, c['fP'][0])
    c = so.rts_case(rng, 3, 3, 1, 10.0)
    sm, sP, _, _ = so.rts_backward_hp(*(c[k][0] for k in ('fm', 'fP', 'pm', 'pP', 'pC')))
    assert np.array_equal(sm[:, 1:], c['fm'][0][:, 1:]) and np.array_equal(sP[..., 1:], c['fP'][0][..., 1:])
    assert not np.any(sm[:, 0] == c['fm'][0][:, 0])
    A = np.linalg.solve(c['pP'][0][..., 1], c['pC'][0][..., 1]).T
    assert np.linalg.norm(A, 2) <= 0.9 * (1 + 1e-12) and not np.allclose(A, A.T)
    np.testing.assert_allclose(sm[:, 0], c['fm'][0][:, 0] + A.dot(c['fm'][0][:, 2] - c['pm'][0][:, 1]), rtol=1e-10)


def test_scaling_is_exact_for_the_oracle():
    rng = np.random.default_rng(7)
    c = so.update_case(rng, 3, 2, 1, 1e2)
    m, P, m_sc, P_sc = (a[0] for a in so.update_ref(c))
    for p in (-200, 200):
        s = 2.0 ** p
        my, Py, _, _ = (a[0] for a in so.update_ref(so.scaled_update_case(c, p, 'y')))
        assert np.array_equal(my, m) and np.array_equal(Py, P)
        mx, Px, mx_sc, Px_sc = (a[0] for a in so.update_ref(so.scaled_update_case(c, p, 'x')))
        assert np.array_equal(mx, m * s) and np.array_equal(Px, P * s * s)
        assert np.allclose(mx_sc, m_sc * s, rtol=1e-14, atol=0) and np.allclose(Px_sc, P_sc * s * s, rtol=1e-14, atol=0)
