"""KL and symmetrised KL divergence on the device (csrc/ssmq_kl.hip, k_kl_divergence) against the reference's own values and an
extended-precision evaluation of them (tests/golden/g20_kl.npz, made by tests/golden/make_golden_kl.py).

Tolerance: the device's error to the extended value may be at most 4 x the reference's float64 error to it (the method differs:
Cholesky factors here, LU - det and inv - there), with a floor of E^2 eps sum|terms|: the result is added up from ~E^2 products
per term, each rounded to eps of the term's magnitude, and without the floor the identical pairs (KL = 0, reference error 0)
would have no scale.

The kernel factors and substitutes in double-double arithmetic (with contraction off: the back end otherwise fuses the rounded
products of the error-free transformations into the sums that follow and the gain is lost).  In plain fp64 the pairs of condition 1e6 came out at 5 to 13 x
the reference's error (cases 4 and 10: 8.7e-06 against 1.7e-06, 1.9e-06 against 1.4e-07), inside cond * eps of the value but over
the bar.  MEASURED (MI355X) with the kernel as it is: 25 of the 26 values are the extended value
rounded to float64 (device error 0), case 0 is off by 1.4e-17 (bar 3.5e-16).
"""
import numpy as np
import pytest

from ssmtoybox_amd import utils

pytestmark = pytest.mark.gpu
EPS = np.finfo(float).eps


def _cases(golden):
    g = golden('g20_kl')
    for i in range(len(g['kl_ref'])):
        yield i, g['c{}_m0'.format(i)], g['c{}_P0'.format(i)], g['c{}_m1'.format(i)], g['c{}_P1'.format(i)], g


def test_single_calls_against_reference_and_extended(golden):
    seen, missed = set(), []
    for i, m0, P0, m1, P1, g in _cases(golden):
        E = len(m0)
        seen.add(E)
        args = (float(m0[0]), float(P0[0, 0]), float(m1[0]), float(P1[0, 0])) if g['scalar'][i] else (m0, P0, m1, P1)
        for fn, ref, ext, terms in ((utils.kl_divergence, g['kl_ref'][i], g['kl_ext'][i], g['kl_terms'][i]),
                                    (utils.symmetrized_kl_divergence, g['skl_ref'][i], g['skl_ext'][i], g['skl_terms'][i])):
            got = fn(*args)
            assert isinstance(got, float)
            bar = max(4 * abs(ref - ext), E * E * EPS * terms)
            print('case {} E = {} {}: device error {:.3e}, reference error {:.3e}, bar {:.3e}'.format(
                i, E, fn.__name__, abs(got - ext), abs(ref - ext), bar))
            if not abs(got - ext) <= bar:
                missed.append((i, fn.__name__, got, ext, ref))
    assert seen == {1, 2, 5, 6}
    assert not missed, missed


def test_batch_is_the_single_call_bit_for_bit(golden):
    for E in (2, 6):
        rows = [(m0, P0, m1, P1) for _, m0, P0, m1, P1, g in _cases(golden) if len(m0) == E]
        m0, P0, m1, P1 = (np.array([r[k] for r in rows] * 30) for k in range(4))         # 90 items: more than one wave
        for sym, fn in ((False, utils.kl_divergence), (True, utils.symmetrized_kl_divergence)):
            kl, st = utils.kl_divergence_batch(m0, P0, m1, P1, symmetrized=sym)
            assert kl.shape == (90,) and st.shape == (90,) and not st.any()
            for b in (0, 1, 2, 64, 89):
                assert kl[b] == fn(m0[b], P0[b], m1[b], P1[b])
            # one true pair against a grid of approximations
            klb, stb = utils.kl_divergence_batch(m0[1], P0[1], m1, P1, symmetrized=sym)
            full, _ = utils.kl_divergence_batch(np.tile(m0[1], (90, 1)), np.tile(P0[1], (90, 1, 1)), m1, P1, symmetrized=sym)
            assert np.array_equal(klb, full) and not stb.any()


def test_indefinite_covariance_marks_its_item_only(golden):
    rows = [(m0, P0, m1, P1) for _, m0, P0, m1, P1, g in _cases(golden) if len(m0) == 5]
    m0, P0, m1, P1 = (np.array([r[k] for r in rows] * 2) for k in range(4))
    clean, _ = utils.kl_divergence_batch(m0, P0, m1, P1)
    bad = P1.copy()
    bad[3, 2, 2] = -bad[3, 2, 2]
    kl, st = utils.kl_divergence_batch(m0, P0, m1, bad)
    assert st[3] != 0 and np.isnan(kl[3])
    keep = [0, 1, 2, 4, 5]
    assert not st[keep].any() and np.array_equal(kl[keep], clean[keep])
    assert np.isnan(utils.kl_divergence(m0[3], P0[3], m1[3], bad[3]))
    assert np.isnan(utils.symmetrized_kl_divergence(m0[3], bad[3], m1[3], P1[3]))


def test_seven_dimensions_are_refused():
    with pytest.raises(NotImplementedError, match='1 <= E <= 6'):
        utils.kl_divergence(np.zeros(7), np.eye(7), np.ones(7), 2 * np.eye(7))
