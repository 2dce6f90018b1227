"""tests/_topk_ref.py against hand-written cases, and the device's rank formula (restated here)
against the exact fractions it must order like."""
from fractions import Fraction

import numpy as np

from tests import _topk_ref as ref

S_MAX = 16384


def rank(c, d):
    """include/hymet_gpu.h at hymet_mash_dist_topk: 2^31 - floor(common * 2^31 / denom), 0 for 0 / 0."""
    return 0 if d == 0 else 2 ** 31 - (c << 31) // d


def test_half_ties_by_index():
    # 1/2 = 2/4 = 500/1000: index order; 3/4 before them, 1/3 after
    c, d = [1, 1, 3, 2, 500], [2, 3, 4, 4, 1000]
    assert ref.order(c, d, 1000) == [2, 0, 3, 4, 1]
    assert ref.topk_dense([c], [d], 2, 1000) == [[2, 0]]


def test_zero_over_zero_first_and_common_zero_last():
    c, d = [0, 5, 0, 7, 0], [9, 10, 0, 7, 0]
    # 0/0 and 7/7 are 1: positions 2, 3, 4 in index order; 0/9 last
    assert ref.order(c, d, 10) == [2, 3, 4, 1, 0]


def test_contract_and_table():
    c, d = [3, 11, 5, 2], [4, 10, 12, 4]
    assert ref.order(c, d, 10) == [0, 3]                       # common > denom, denom > s: out
    table = [0, 1, 2, 3, 3] + [9] * 6                          # denom 4 needs common >= 3
    assert ref.order(c, d, 10, table) == [0]


def test_csr_rows_and_reference_index():
    row_off = [0, 0, 3, 4]
    idx = [4, 9, 12, 1]
    c, d = [1, 3, 2, 0], [2, 4, 4, 5]
    assert ref.topk_csr(row_off, idx, c, d, 2, 10) == [[], [(9, 1), (4, 0)], [(1, 3)]]
    assert ref.topk_csr(row_off, idx, c, d, 5, 10)[1] == [(9, 1), (4, 0), (12, 2)]


def _same_order(pairs):
    """The rank compares two entries exactly as their fractions do, for all the given pairs of entries."""
    for (c1, d1), (c2, d2) in pairs:
        f1, f2 = ref.fraction(c1, d1), ref.fraction(c2, d2)
        r1, r2 = rank(c1, d1), rank(c2, d2)
        assert (f1 > f2) == (r1 < r2) and (f1 == f2) == (r1 == r2), ((c1, d1), (c2, d2))
        assert 0 <= r1 < 2 ** 32


def test_rank_orders_like_fractions_small_denominators():
    entries = [(c, d) for d in range(65) for c in range(d + 1)]
    by_fraction = sorted(entries, key=lambda e: ref.fraction(*e))
    # neighbours in fraction order decide every comparison of a monotone map
    _same_order(zip(by_fraction, by_fraction[1:]))
    ranks = [rank(*e) for e in by_fraction]
    assert ranks == sorted(ranks, reverse=True)
    assert rank(0, 0) == rank(1, 1) == rank(64, 64) == 0 and rank(0, 5) == 2 ** 31


def test_rank_orders_like_fractions_random_pairs():
    rng = np.random.default_rng(31)
    d = rng.integers(1, S_MAX + 1, size=(4000, 2))
    c = (rng.random((4000, 2)) * (d + 1)).astype(np.int64)
    _same_order((((int(c[i, 0]), int(d[i, 0])), (int(c[i, 1]), int(d[i, 1])))) for i in range(4000))
    # near misses: the second fraction is the first moved by one in the numerator or the denominator
    near = []
    for i in range(2000):
        c1, d1 = int(c[i, 0]), int(d[i, 0])
        for c2, d2 in ((c1 + 1, d1), (c1, d1 + 1), (c1 - 1, d1), (c1, d1 - 1)):
            if 0 <= c2 <= d2 <= S_MAX and d2 >= 1:
                near.append(((c1, d1), (c2, d2)))
    _same_order(near)


def test_rank_separates_the_closest_neighbours():
    top = [(S_MAX - 1, S_MAX), (S_MAX - 2, S_MAX - 1), (S_MAX, S_MAX), (S_MAX - 1, S_MAX - 1), (S_MAX - 3, S_MAX - 2),
           (1, S_MAX), (1, S_MAX - 1), (0, S_MAX), (0, 1), (1, 2), (S_MAX // 2, S_MAX), (S_MAX // 2 - 1, S_MAX - 1),
           (8191, 16383), (8192, 16383), (0, 0)]
    _same_order((a, b) for a in top for b in top)
    # the smallest gap two different fractions can have is 1 / (d1 * d2) >= 2^-28: 8 in rank units
    assert Fraction(S_MAX - 1, S_MAX) - Fraction(S_MAX - 2, S_MAX - 1) == Fraction(1, S_MAX * (S_MAX - 1))
    assert rank(S_MAX - 2, S_MAX - 1) - rank(S_MAX - 1, S_MAX) >= 8
