"""
Bootstrap error bars, the part that needs no GPU: the test oracle itself (tests/_bootstrap_oracle.py: Philox4x32-10 against
its published known-answer vectors, the index draw, the resample means) and the Python-side range refusals, which come
before the library is loaded.
"""
import numpy as np
import pytest

from tests import _bootstrap_oracle as bo


def test_oracle_philox_known_answers():
    """Random123's kat_vectors for philox4x32 with 10 rounds (Salmon et al., SC'11)."""
    assert bo.philox4x32_10((0, 0, 0, 0), (0, 0)) == (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)
    assert bo.philox4x32_10((0xffffffff,) * 4, (0xffffffff,) * 2) == (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)
    assert bo.philox4x32_10((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0)) == \
        (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)


@pytest.mark.parametrize('n', [1, 2, 63, 1000, 2 ** 31 - 1])
def test_oracle_indices_in_range(n):
    for seed in (0, 7, 2 ** 64 - 1):
        for s in (0, 1, 2 ** 20 - 1):
            js = [bo.draw(seed, s, i, n) for i in list(range(min(n, 40))) + [n - 1]]
            assert all(0 <= j < n for j in js)
    if n <= 1000:
        full = bo.draws(3, 5, n)
        assert full.shape == (n,) and full.min() >= 0 and full.max() < n
        assert all(full[i] == bo.draw(3, 5, i, n) for i in range(n))
        if n == 1000:          # a pair of positions shares one Philox call but not its words
            assert len(set(full.tolist())) > 500 and not np.array_equal(full[0::2], full[1::2])


def test_oracle_resample_means():
    assert np.array_equal(bo.resample_means(np.full(37, 0.1), None, 5, 11), np.full(5, 0.1))
    data = np.arange(10.0)
    idx = np.array([2, 5, 7])
    m = bo.resample_means(data, idx, 64, 1)
    assert set(np.unique(np.round(3 * m)).astype(int)) <= set(range(6, 22)) and m.min() >= 2.0 and m.max() <= 7.0
    assert np.array_equal(m[[3, 9]], bo.resample_means(data, idx, 64, 1, which=[3, 9]))
    assert not np.array_equal(m, bo.resample_means(data, idx, 64, 2))


def test_range_refusals_before_the_library_is_loaded(monkeypatch):
    from ssmtoybox_amd import _lib, mcshard, utils

    def no_load():
        raise AssertionError('the library was loaded before the range check')

    monkeypatch.setattr(_lib, 'load', no_load)
    for B in (0, 2 ** 31):
        with pytest.raises(ValueError, match='n < 2\\^31'):
            mcshard.bootstrap_var_dev(None, 2 ** 31, 1, B)
    with pytest.raises(ValueError, match='n < 2\\^31'):          # every trajectory excluded
        mcshard.bootstrap_var_dev(None, 64, 1, 5, status=np.ones(5, dtype=np.int32))
    for S in (0, 2 ** 20 + 1):
        with pytest.raises(ValueError, match='S <= 2\\^20'):
            mcshard.bootstrap_var_dev(None, 64, 1, 5, samples=S)
        with pytest.raises(ValueError, match='S <= 2\\^20'):
            utils.bootstrap_var(np.zeros(5), S)
        with pytest.raises(ValueError, match='S <= 2\\^20'):
            mcshard.device_score_bars(1, 5, 64, 3, None, None, None, samples=S)
    for R in (0, 20):
        with pytest.raises(ValueError, match='R <= 19'):
            mcshard.bootstrap_var_dev(None, 64, R, 5)
    with pytest.raises(ValueError, match='n < 2\\^31'):
        utils.bootstrap_var(np.zeros((1, 0)))
    with pytest.raises(ValueError, match='one dimension'):
        utils.bootstrap_var(np.zeros((2, 5)))
    with pytest.raises(ValueError, match='k0'):
        mcshard.device_traj_scores(1, 5, 64, 3, None, None, None, k0=3)


def test_utils_bootstrap_var_squeezes_and_seeds_like_the_reference(monkeypatch):
    """(1, n) input is squeezed as the reference does (utils.py:239); seed=None is drawn from numpy's global generator."""
    from ssmtoybox_amd import _lib, utils
    calls = []

    class FakeLib:
        @staticmethod
        def ssmq_bootstrap_var(pd, n, samples, seed, pv):
            calls.append((n, samples, seed.value, [pd[i] for i in range(n)]))
            pv[0] = 0.25
            return 0

    monkeypatch.setattr(_lib, 'load', lambda: FakeLib)
    data = np.array([[1.0, 2.0, 4.0]])
    assert utils.bootstrap_var(data, 17, seed=9) == 0.25
    assert utils.bootstrap_var(data[0], 17, seed=9) == 0.25
    assert calls[0] == calls[1] == (3, 17, 9, [1.0, 2.0, 4.0])
    np.random.seed(5)
    utils.bootstrap_var(data)
    np.random.seed(5)
    utils.bootstrap_var(data)
    np.random.seed(6)
    utils.bootstrap_var(data)
    assert calls[2][1] == 1000 and calls[2][2] == calls[3][2] != calls[4][2]
