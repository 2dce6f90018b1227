"""The grouped anchor sort alone (csrc/mm_asort.hip through hymet_mm_anchor_sort) against
numpy: the anchor set is np.lexsort((val, key)) of the input, exactly, with the head bitmap of
its (query, strand, target) groups -- on inputs shaped like the emitter's (groups that rise
or fall in target position, interleaved minimizer by minimizer, plus stray hits), at every
class boundary of the block sorts, at the outlier path's limits (flagged words, passes), on
ties, on inputs the path must decline, with coarse bins, and on rows that only an
order-preserving scatter leaves sorted.  The library's counters say which path a segment took.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

K_OUT_MAX = 128         # csrc/mm_asort.hip kOutMax: most outliers the outlier path takes
PB = 28                 # key bits of the target position
MAX_QLEN = 1 << 20      # bound of y
YHI = 5
FAST_SEGS, FAST_ANCHORS, FULL_SEGS, FULL_ANCHORS = range(4)


@pytest.fixture(scope="module")
def gpu():
    from hymet_amd._lib import Gpu
    return Gpu(0)


def make_key(q, rev, rid, rpos, rb):
    q, rev, rid, rpos = (np.asarray(a, np.uint64) for a in (q, rev, rid, rpos))
    return q << np.uint64(1 + rb + PB) | rev << np.uint64(rb + PB) | rid << np.uint64(PB) | rpos


def anchor_sort(g, key, val, qoff, rb, want_stats=True):
    """(ax, ay, ax32, head bits as a bool array, stats) of one hymet_mm_anchor_sort call."""
    key = np.ascontiguousarray(key, np.uint64)
    val = np.ascontiguousarray(val, np.uint32)
    qoff = np.ascontiguousarray(qoff, np.int64)
    n = len(key)
    ax, ay = np.empty(n, np.uint64), np.empty(n, np.uint64)
    ax32 = np.empty(n, np.uint32)
    hb = np.zeros((n + 31) // 32, np.uint32)
    stats = np.full(4, -1, np.int64)
    vp = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    g.call("hymet_mm_anchor_sort", vp(key), vp(val), n, vp(qoff), len(qoff) - 1, rb, PB, YHI, MAX_QLEN, vp(ax), vp(ay),
           vp(ax32), vp(hb), vp(stats) if want_stats else None)
    bits = (hb[np.arange(n) >> 5] >> (np.arange(n, dtype=np.uint32) & np.uint32(31)) & np.uint32(1)).astype(bool)
    return ax, ay, ax32, bits, stats


def expected(key, val, rb):
    key, val = np.asarray(key, np.uint64), np.asarray(val, np.uint32)
    order = np.lexsort((val, key))
    k, v = key[order], val[order]
    rev = k >> np.uint64(rb + PB) & np.uint64(1)
    rid = k >> np.uint64(PB) & np.uint64((1 << rb) - 1)
    rpos = k & np.uint64((1 << PB) - 1)
    ax = rev << np.uint64(63) | rid << np.uint64(32) | rpos
    ay = np.uint64(YHI << 32) | v.astype(np.uint64)
    head = np.ones(len(k), bool)
    head[1:] = (k[1:] >> np.uint64(PB)) != (k[:-1] >> np.uint64(PB))
    return ax, ay, rpos.astype(np.uint32), head


def check(g, key, val, qoff, rb=9):
    """The call's arrays equal numpy's; returns the stats."""
    ax, ay, ax32, bits, stats = anchor_sort(g, key, val, qoff, rb)
    wx, wy, wx32, whead = expected(key, val, rb)
    np.testing.assert_array_equal(ax, wx)
    np.testing.assert_array_equal(ay, wy)
    np.testing.assert_array_equal(ax32, wx32)
    np.testing.assert_array_equal(bits, whead)
    return stats


def outlier_passes(words):
    """The outlier path as the issue defines it, on a segment's words in input order: read back
    to front where the first word is above the last; flag both ends of every descent among the
    unflagged words, pass by pass, until a pass flags nothing.  -> (flagged words, flagging
    passes)."""
    w = np.asarray(words, np.uint64)
    if w[0] > w[-1]:
        w = w[::-1]
    flagged = np.zeros(len(w), bool)
    passes = 0
    while True:
        idx = np.nonzero(~flagged)[0]
        d = np.nonzero(w[idx[1:]] < w[idx[:-1]])[0]
        if len(d) == 0:
            return int(flagged.sum()), passes
        flagged[idx[d]] = True
        flagged[idx[d + 1]] = True
        passes += 1


def takes_outlier_path(words):
    f, p = outlier_passes(words)
    return f <= K_OUT_MAX and p <= 3


def pack(rpos, y):
    return np.asarray(rpos, np.uint64) << np.uint64(21) | np.asarray(y, np.uint64)


# ------------------------------------------------------------------ 1 class boundaries

BOUNDARY_SIZES = [65, 256, 257, 1024, 1025, 4096, 4097, 8192, 8193, 16384, 16385]


def boundary_case(falling_half):
    """One query; group g has BOUNDARY_SIZES[g] anchors rising (or, every other group with
    falling_half, falling) in target position, emitted interleaved: anchor i of a group of m at
    time (i + 0.5) / m, as minimizers along the query hit every group in turn."""
    gid = np.concatenate([np.full(m, g) for g, m in enumerate(BOUNDARY_SIZES)])
    idx = np.concatenate([np.arange(m) for m in BOUNDARY_SIZES])
    size = np.asarray(BOUNDARY_SIZES)[gid]
    order = np.lexsort((gid, (idx + 0.5) / size))
    gid, idx, size = gid[order], idx[order], size[order]
    fall = (gid % 2 == 1) if falling_half else np.zeros(len(gid), bool)
    rpos = 100 + 3 * np.where(fall, size - 1 - idx, idx)
    key = make_key(0, fall.astype(np.uint64), 7 + 2 * gid, rpos, 9)
    val = np.arange(len(gid), dtype=np.uint32)          # the query position rises along the emission
    return key, val, np.array([0, len(gid)], np.int64)


def block_sorted(sizes):
    """(segments, anchors) of the groups the block sorts take: 65..16384 anchors."""
    s = [m for m in sizes if 64 < m <= 16384]
    return len(s), sum(s)


@pytest.mark.parametrize("falling_half", [False, True])
def test_class_boundaries(gpu, falling_half):
    key, val, qoff = boundary_case(falling_half)
    stats = check(gpu, key, val, qoff)
    segs, anchors = block_sorted(BOUNDARY_SIZES)
    assert list(stats) == [segs, anchors, 0, 0], "a rising or falling group did not finish by the outlier path"


def test_without_stats(gpu):
    key, val, qoff = boundary_case(True)
    ax, ay, ax32, bits, stats = anchor_sort(gpu, key, val, qoff, 9, want_stats=False)
    np.testing.assert_array_equal(ax, expected(key, val, 9)[0])
    assert list(stats) == [-1] * 4


# ------------------------------------------------------------------ 2 outlier counts

def displaced(n, pairs, triples, rng):
    """A rising group of n positions in which `pairs` single words were moved far below their
    place (the descent in front of each flags 2 words) and `triples` falling couples (two
    descents: 3 words), far enough apart not to meet."""
    rpos = 1000 + 10 * np.arange(n)
    slots = rng.choice(np.arange(2, n // 8 - 1), pairs + triples, replace=False) * 8
    for i, s in enumerate(slots):
        if i < pairs:
            rpos[s] = 5 + i
        else:
            rpos[s], rpos[s + 1] = 700 + i, 300 + i
    return rpos


def two_queries(rpos_a, rpos_b):
    """Query 0 holds group a (<= 4096 anchors: sorted whole), query 1 group b (> 4096 anchors:
    tiled and scattered first)."""
    na, nb = len(rpos_a), len(rpos_b)
    key = np.concatenate([make_key(0, 0, 3, rpos_a, 9), make_key(1, 1, 40, rpos_b, 9)])
    val = np.concatenate([np.arange(na), np.arange(nb)]).astype(np.uint32)
    return key, val, np.array([0, na, na + nb], np.int64)


@pytest.mark.parametrize("flagged", [2, K_OUT_MAX - 1, K_OUT_MAX, K_OUT_MAX + 1])
def test_outlier_count(gpu, flagged):
    triples = flagged % 2
    pairs = (flagged - 3 * triples) // 2
    rng = np.random.default_rng(flagged)
    a, b = displaced(1000, pairs, triples, rng), displaced(5000, pairs, triples, rng)
    for r in (a, b):
        assert outlier_passes(pack(r, np.arange(len(r)))) == (flagged, 1)
    stats = check(gpu, *two_queries(a, b))
    if flagged <= K_OUT_MAX:
        assert list(stats) == [2, 6000, 0, 0]
    else:
        assert list(stats) == [0, 0, 2, 6000]


def rising(n):
    return 1000 + 10 * np.arange(n)


def outliers_at_the_ends(n):
    r = rising(n)
    r[0], r[n - 1] = r[n // 3] + 1, r[2 * n // 3] + 1    # first above its place, last below; first < last
    return r, 4, 1


def adjacent_rising_outliers(n):
    r = rising(n)
    r[500], r[501] = 20, 30          # the second is a descent only once the first is gone
    return r, 4, 2


def outlier_next_to_descent(n):
    r = rising(n)
    r[300:303] = [20, 30, 40]        # one more pass for each
    r[700], r[701] = 90, 80
    return r, 9, 3


def needs_a_fourth_pass(n):
    r = rising(n)
    r[300:304] = [20, 30, 40, 50]
    return r, 8, 4


@pytest.mark.parametrize("build", [outliers_at_the_ends, adjacent_rising_outliers, outlier_next_to_descent,
                                   needs_a_fourth_pass])
def test_outlier_passes(gpu, build):
    (a, flagged, passes), (b, _, _) = build(1000), build(5000)
    for r in (a, b):
        assert outlier_passes(pack(r, np.arange(len(r)))) == (flagged, passes)
    stats = check(gpu, *two_queries(a, b))
    assert list(stats) == ([2, 6000, 0, 0] if passes <= 3 else [0, 0, 2, 6000])


# ------------------------------------------------------------------ 3 wrong reversal guess

@pytest.mark.parametrize("mirror", [False, True])
def test_wrong_reversal_guess(gpu, mirror):
    """A rising group whose last word is its minimum is read back to front (first > last), a
    falling group whose last word is its maximum is not: exact either way."""
    a, b = rising(1000), rising(5000)
    a[-1], b[-1] = 1, 1
    if mirror:
        a, b = (1 << 20) - a, (1 << 20) - b
    stats = check(gpu, *two_queries(a, b))
    assert stats[FAST_SEGS] + stats[FULL_SEGS] == 2


# ------------------------------------------------------------------ 4 ties

def test_equal_positions_order_by_y(gpu):
    a, b = np.full(1000, 777), np.full(5000, 777)
    key, val, qoff = two_queries(a, b)
    val = val.copy()
    val[[10, 400, 1000 + 17, 1000 + 4000]] = [900, 3, 4500, 2]       # stray y values
    check(gpu, key, val, qoff)


def test_identical_words(gpu):
    """Pairs of identical (position, y) words, some of them displaced: kept words and outliers
    that compare equal still take distinct slots."""
    def build(n):
        r = 1000 + 10 * (np.arange(n) // 2)
        y = np.arange(n) // 2
        for s, t in ((101, 40), (301, 200), (600, 901), (601, 900)):   # a pair member moved to another place
            r[t], y[t] = r[s], y[s]
        return r, y
    (ra, ya), (rb_, yb) = build(1000), build(5000)
    key, _, qoff = two_queries(ra, rb_)
    val = np.concatenate([ya, yb]).astype(np.uint32)
    assert takes_outlier_path(pack(ra, ya)) and takes_outlier_path(pack(rb_, yb))
    stats = check(gpu, key, val, qoff)
    assert list(stats) == [2, 6000, 0, 0]


# ------------------------------------------------------------------ 5 shuffled input

def test_shuffled_group_and_whole_query(gpu):
    rng = np.random.default_rng(5)
    shuffled = rng.permutation(3000) * 7 + 50             # a group of query 0, beside a rising one of 2000
    k0 = np.concatenate([make_key(0, 0, 11, shuffled, 9), make_key(0, 0, 12, rising(2000), 9)])
    k1 = make_key(1, rng.integers(0, 2, 3000), rng.integers(100, 140, 3000), rng.integers(0, 1 << 20, 3000), 9)
    key = np.concatenate([k0, k1])
    val = rng.integers(0, MAX_QLEN, len(key)).astype(np.uint32)
    val[3000:5000] = np.arange(2000)
    stats = check(gpu, key, val, np.array([0, 5000, 8000], np.int64))
    assert list(stats) == [1, 2000, 2, 6000]


# ------------------------------------------------------------------ 6 coarse bins

def test_coarse_bins_head_bits(gpu):
    """rb = 12: targets 2t and 2t + 1 share a bin, so a segment holds two chaining groups and a
    head bit falls inside it.  Query 0 (tiled): two rising groups of one bin, interleaved;
    query 1 (sorted whole): two rising groups one after the other with a few stray hits, which
    the outlier path finishes."""
    rb = 12
    n0 = 3000
    t0 = np.tile([600, 601], n0)
    r0 = rising(2 * n0)
    r0[[50, 51, 4000]] = [3, 2, 9]
    r1 = np.concatenate([rising(1500), rising(1500)])
    r1[[20, 700, 1600, 2900]] = [5, 9_000_000, 4, 6]
    t1 = np.repeat([2050, 2051], 1500)
    key = np.concatenate([make_key(0, 1, t0, r0, rb), make_key(1, 0, t1, r1, rb)])
    val = np.concatenate([np.arange(2 * n0), np.arange(3000)]).astype(np.uint32)
    w1 = pack(t1.astype(np.uint64) << np.uint64(PB) | r1.astype(np.uint64), 0)  # order of query 1's words (y rises)
    assert takes_outlier_path(w1)
    stats = check(gpu, key, val, np.array([0, 2 * n0, 2 * n0 + 3000], np.int64), rb=rb)
    assert stats[FAST_SEGS] >= 1 and stats[FAST_ANCHORS] >= 3000
    head = expected(key, val, rb)[3]
    assert head.sum() == 4                                # two groups per query


# ------------------------------------------------------------------ 7 scatter order

def scatter_case():
    """One query of 24,576 anchors (a tile and a half, twelve scatter rounds) in rows of 64:
    a hot bin on half the lanes; two hot bins; thirty bins on exactly two lanes each; thin bins
    on the remaining lanes.  Every bin's anchors rise in emission order, so after an
    order-preserving scatter no group has a descent."""
    rng = np.random.default_rng(7)
    rows = 384
    hot1, hot2 = 900, 901
    pair_bins = 300 + np.arange(30)
    thin = 20 + np.arange(200)
    t = 0
    bins = np.empty((rows, 64), np.int64)
    for r in range(rows):
        if r % 3 == 0:
            row = [hot1] * 32
        elif r % 3 == 1:
            row = [hot1] * 24 + [hot2] * 24
        else:
            row = list(np.repeat(pair_bins, 2))
        while len(row) < 64:
            row.append(thin[t % len(thin)])
            t += 1
        bins[r] = rng.permutation(row)
    bins = bins.ravel()
    count = np.zeros(1024, np.int64)
    rpos = np.empty(len(bins), np.int64)
    for i, b in enumerate(bins):
        rpos[i] = 100 + 5 * count[b]
        count[b] += 1
    key = make_key(0, bins >> 9, bins & 511, rpos, 9)
    val = np.arange(len(bins), dtype=np.uint32)
    return key, val, np.array([0, len(bins)], np.int64), count[count > 0]


def test_scatter_keeps_input_order(gpu):
    key, val, qoff, sizes = scatter_case()
    segs, anchors = block_sorted(sizes)
    assert segs == 32                                     # the hot and the two-lane bins
    stats = check(gpu, key, val, qoff)
    assert list(stats) == [segs, anchors, 0, 0], "a bin's anchors did not leave the scatter in input order"


# ------------------------------------------------------------------ 8 fallback switch

def _child(out_path):
    """Run by test_fallback_switch in a fresh process with HYMET_ASORT_ADAPT=0."""
    from hymet_amd._lib import Gpu
    g = Gpu(0)
    key, val, qoff = boundary_case(True)
    ax, ay, ax32, bits, stats = anchor_sort(g, key, val, qoff, 9)
    np.savez(out_path, ax=ax, ay=ay, ax32=ax32, bits=bits, stats=stats)


def test_fallback_switch(gpu, tmp_path):
    out = tmp_path / "full.npz"
    env = dict(os.environ, HYMET_ASORT_ADAPT="0")
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-m", "tests.test_anchor_sort_gpu", str(out)]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    z = np.load(out)
    key, val, qoff = boundary_case(True)
    ax, ay, ax32, bits, _ = anchor_sort(gpu, key, val, qoff, 9)
    wx, wy, wx32, whead = expected(key, val, 9)
    for got, here, want in ((z["ax"], ax, wx), (z["ay"], ay, wy), (z["ax32"], ax32, wx32), (z["bits"], bits, whead)):
        np.testing.assert_array_equal(got, want)
        np.testing.assert_array_equal(here, want)
    segs, anchors = block_sorted(BOUNDARY_SIZES)
    assert list(z["stats"]) == [0, 0, segs, anchors]


if __name__ == "__main__":
    _child(sys.argv[1])
