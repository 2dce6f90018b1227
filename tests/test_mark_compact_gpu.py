"""The long join's compaction (mark_count_kernel, the scan of the tile counts,
mark_compact_kernel) through hymet_mm_mark_compact, bit for bit against numpy: an anchor is
kept iff its mark equals 2 and its query is flagged; a kept anchor is a group head iff it is
the first kept one or its x >> 32 differs from the previous kept anchor's.  Anchor counts on
both sides of the 16-anchor runs a thread decides, of a wave's 64 and of the 4,096-anchor
tile, each with: everything kept, nothing kept, random marks (1 and a stale stamp 7 are not
marks) over random queries some of them empty and some unflagged, a query boundary inside a
16-anchor run, and -- where the count reaches them -- a query boundary on a tile boundary, a
group that continues across a tile boundary and one that ends on it, and a whole tile with
nothing kept between two tiles that keep (the look-back over last_kept).  y comes back
widened: the device holds its low word and one span per set.  Also: hymet_mm_chain_dp rejects
y values of two spans and works on the same context afterwards, and a small mapping whose
long join runs gives the same region records with anchor words and with the two-key fallback.
"""
import ctypes

import numpy as np
import pytest

from tests._anchors import PEN_GAP, assemble, colinear
from tests._data import mutate, rand_seq

pytestmark = pytest.mark.gpu

HYMET_E_ARG = -2
SPAN = 15
TILE = 4096
COUNTS = [1, 15, 16, 17, 63, 64, 65, 4095, 4096, 4097, 3 * 4096 + 5]
U = np.uint64


@pytest.fixture(scope="module")
def gpu():
    from hymet_amd._lib import Gpu
    return Gpu(0)


def vp(a):
    return ctypes.c_void_p(a.ctypes.data)


def mark_compact(g, x, y, mark, qoff, qflag):
    """(return code, kept x, kept y, head bits of the kept anchors) of one hymet_mm_mark_compact call."""
    x, y = np.ascontiguousarray(x, np.uint64), np.ascontiguousarray(y, np.uint64)
    mark = np.ascontiguousarray(mark, np.int32)
    qoff = np.ascontiguousarray(qoff, np.int64)
    qflag = np.ascontiguousarray(qflag, np.uint32)
    n = len(x)
    ox, oy = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    hb = np.zeros((n + 31) // 32, np.uint32)
    kept = ctypes.c_int64(-1)
    rc = g.lib.hymet_mm_mark_compact(g.ctx, vp(x), vp(y), vp(mark), n, vp(qoff), vp(qflag), len(qoff) - 1, vp(ox), vp(oy),
                                     vp(hb), ctypes.byref(kept))
    k = kept.value
    bits = (hb[np.arange(k) >> 5] >> (np.arange(k, dtype=np.uint32) & np.uint32(31)) & np.uint32(1)).astype(bool)
    return rc, ox[:k], oy[:k], bits


def expected(x, y, mark, qoff, qflag):
    qid = np.repeat(np.arange(len(qoff) - 1), np.diff(qoff))
    keep = (mark == 2) & (qflag[qid] != 0)
    kx, ky = x[keep], y[keep]
    head = np.ones(len(kx), bool)
    head[1:] = (kx[1:] >> U(32)) != (kx[:-1] >> U(32))
    return kx, ky, head


def anchors(rng, n, cuts):
    """n anchors in (strand, target) groups that change exactly at `cuts` (sorted, within
    (0, n)): x = group << 32 | a rising position, y = SPAN << 32 | any 32-bit word."""
    gid = np.zeros(n, np.int64)
    gid[np.asarray(cuts, np.int64)] = 1
    gid = np.cumsum(gid)
    hi = (gid * 7 + 3) & 0x7fffffff | ((gid & 1) << 31)          # distinct neighbours, both strands
    x = hi.astype(U) << U(32) | np.arange(n, dtype=U) * U(3)
    y = U(SPAN) << U(32) | rng.integers(0, 1 << 32, n, dtype=np.uint64)
    return x, y


def random_cuts(rng, n):
    return np.flatnonzero(rng.random(n) < 0.02)[1:] if n > 1 else np.empty(0, np.int64)


def offsets(n, starts):
    """Query offsets over n anchors from the queries' first anchors (a repeated start: an empty query)."""
    return np.r_[0, np.asarray(starts, np.int64), n].astype(np.int64)


def build(n, scenario):
    rng = np.random.default_rng(n * 31 + len(scenario))
    if scenario == "all":
        x, y = anchors(rng, n, random_cuts(rng, n))
        return x, y, np.full(n, 2), offsets(n, []), np.ones(1)
    if scenario == "none":
        x, y = anchors(rng, n, random_cuts(rng, n))
        return x, y, rng.choice([0, 1, 7], n), offsets(n, []), np.ones(1)
    if scenario == "random":
        # random queries, empty ones among them and at both ends, a third of them unflagged;
        # an unflagged query with every anchor marked 2
        x, y = anchors(rng, n, random_cuts(rng, n))
        starts = np.sort(rng.integers(0, n + 1, min(n, 12)))
        qoff = offsets(n, np.r_[0, starts, starts[len(starts) // 2], n])
        qoff.sort()
        qflag = (rng.random(len(qoff) - 1) < 0.67).astype(np.uint32)
        mark = rng.choice([0, 1, 2, 7], n, p=[0.1, 0.1, 0.7, 0.1])
        big = int(np.argmax(np.diff(qoff)))
        qflag[big] = 0
        mark[qoff[big]:qoff[big + 1]] = 2
        if len(qflag) > 1:
            qflag[(big + 1) % len(qflag)] = 1
        return x, y, mark, qoff, qflag
    if scenario == "query_in_run":
        # query boundaries inside 16-anchor runs, flags alternating: the keep bits change
        # in the middle of a thread's 16 anchors
        x, y = anchors(rng, n, random_cuts(rng, n))
        starts = [s for s in (5, 16 + 7, 64 + 15, TILE - 3, TILE + 1, 2 * TILE + 9) if s < n]
        qoff = offsets(n, starts)
        qflag = (np.arange(len(qoff) - 1) & 1).astype(np.uint32)
        return x, y, np.full(n, 2), qoff, qflag
    if scenario == "query_on_tile":
        x, y = anchors(rng, n, random_cuts(rng, n))
        qoff = offsets(n, [TILE] + ([2 * TILE, 2 * TILE] if n > 2 * TILE else []))
        qflag = np.ones(len(qoff) - 1, np.uint32)
        qflag[0] = 0
        return x, y, rng.choice([0, 2], n, p=[0.2, 0.8]), qoff, qflag
    if scenario == "group_across_tile":   # no head at the tile's first anchor
        x, y = anchors(rng, n, [c for c in (TILE - 9, TILE + 3) if c < n])
        return x, y, np.full(n, 2), offsets(n, []), np.ones(1)
    if scenario == "group_ends_on_tile":  # a head there
        x, y = anchors(rng, n, [TILE - 9, TILE])
        return x, y, np.full(n, 2), offsets(n, []), np.ones(1)
    if scenario in ("empty_tile_same_group", "empty_tile_new_group"):
        # tile 1 keeps nothing; the group of tile 2's first kept anchor is or is not that of
        # tile 0's last kept one, which sits before unkept anchors at the tile's end
        cuts = [100, TILE - 40] + ([] if scenario == "empty_tile_same_group" else [TILE + 11]) + [2 * TILE + 50]
        x, y = anchors(rng, n, cuts)
        mark = np.full(n, 2)
        mark[TILE - 20:2 * TILE + 7] = 7
        mark[TILE + 5] = 1
        return x, y, mark, offsets(n, [TILE + 100]), np.ones(2)
    raise AssertionError(scenario)


def cases():
    out = []
    for n in COUNTS:
        sc = ["all", "none", "random"]
        if n >= 15:
            sc.append("query_in_run")
        if n > TILE:
            sc += ["query_on_tile", "group_across_tile", "group_ends_on_tile"]
        if n > 2 * TILE + 50:
            sc += ["empty_tile_same_group", "empty_tile_new_group"]
        out += [(n, s) for s in sc]
    return out


@pytest.mark.parametrize("n,scenario", cases())
def test_mark_compact(gpu, n, scenario):
    x, y, mark, qoff, qflag = build(n, scenario)
    mark, qflag = np.asarray(mark, np.int32), np.asarray(qflag, np.uint32)
    assert len(x) == n and qoff[0] == 0 and qoff[-1] == n and (np.diff(qoff) >= 0).all()
    kx, ky, head = expected(x, y, mark, qoff, qflag)
    if scenario == "none":
        assert len(kx) == 0
    if scenario == "all":
        assert len(kx) == n
    if scenario == "group_across_tile":
        assert not head[TILE]
    if scenario == "group_ends_on_tile":
        assert head[TILE]
    if scenario.startswith("empty_tile"):
        # the kept anchors skip from TILE - 21 to 2 TILE + 7: the head there is the look-back's
        assert head[TILE - 20] == (scenario == "empty_tile_new_group")
    rc, ox, oy, bits = mark_compact(gpu, x, y, mark, qoff, qflag)
    assert rc == 0, gpu.lib.hymet_last_error()
    assert len(ox) == len(kx)
    np.testing.assert_array_equal(ox, kx)
    np.testing.assert_array_equal(oy, ky)
    np.testing.assert_array_equal(bits, head)


def test_mark_compact_rejects_two_spans(gpu):
    x, y, mark, qoff, qflag = build(65, "all")
    y = y.copy()
    y[40] = U(19) << U(32) | (y[40] & U(0xffffffff))
    rc, ox, _, _ = mark_compact(gpu, x, y, mark, qoff, qflag)
    assert rc == HYMET_E_ARG
    assert b"span" in gpu.lib.hymet_last_error()


def test_chain_dp_rejects_two_spans_then_runs(gpu):
    """y values of two spans have no 32-bit form with one span beside it: HYMET_E_ARG; the next
    call on the same context, with one span, gives the oracle's f and p."""
    from oracle import oracle_lib
    rng = np.random.default_rng(5)
    x, y = assemble([colinear(rng, 700, rid=0), colinear(rng, 90, rid=1, rev=1), colinear(rng, 5, rid=2)])
    n = len(x)
    f, p = np.zeros(n, np.int32), np.zeros(n, np.int64)
    args = (10000, 1000, 1000, 25, 100000, ctypes.c_float(PEN_GAP), ctypes.c_float(0.0), vp(f), vp(p))
    y2 = y.copy()
    y2[n // 2] = U(19) << U(32) | (y2[n // 2] & U(0xffffffff))
    rc = gpu.lib.hymet_mm_chain_dp(gpu.ctx, vp(x), vp(y2), n, *args)
    assert rc == HYMET_E_ARG
    assert b"span" in gpu.lib.hymet_last_error()
    assert not f.any() and not p.any()   # nothing written
    rc = gpu.lib.hymet_mm_chain_dp(gpu.ctx, vp(x), vp(y), n, *args)
    assert rc == 0, gpu.lib.hymet_last_error()
    fo, po = oracle_lib.mm_debug_chain(np.stack([x, y], axis=1), 10000, 1000, 1000, 25, 100000, float(PEN_GAP), 0.0)
    np.testing.assert_array_equal(f, fo)
    np.testing.assert_array_equal(p, po)


def test_map_long_join_with_words_and_with_pairs(gpu, monkeypatch):
    """One small mapping whose long join runs (a query of two target stretches 35 kbp apart:
    two first-pass chains, each leaving half of it uncovered), with HYMET_ANCHOR_LEGACY unset
    (the grouped sort writes the first-pass set) and = 1 (the two-key fallback writes it): the
    compaction hands the long join the same set either way, and the region records agree."""
    from hymet_amd import mapper
    from hymet_amd.seqio import DevicePool, from_records
    rng = np.random.default_rng(78)
    base = rand_seq(rng, 120_000)
    refs = [base, mutate(rng, base, 0.02), rand_seq(rng, 60_000)]
    ss = from_records([(f"NC_{i:06d}.1", "", s) for i, s in enumerate(refs)])
    part = mapper.IndexPart(gpu, ss)
    opt = mapper.MapOpt.asm10()
    opt.resolve_mid_occ(part)
    assert opt.bw_long > opt.bw   # the long join is on
    qs = [mutate(rng, base[5_000:25_000] + base[60_000:85_000], 0.01),   # re-chained; > 4,096 anchors
          mutate(rng, base[30_000:50_000], 0.01),                          # one chain: kept as it is
          mutate(rng, refs[2][1_000:9_000] + refs[2][40_000:46_000], 0.02),
          b""]
    qpool = DevicePool(gpu, from_records([(f"q{i}", "", s) for i, s in enumerate(qs)]), DevicePool.ALPHA_MINIMAP2)
    out = {}
    gpu.prof(True)
    try:
        for form, env in (("words", None), ("twokey", "1")):
            if env is None:
                monkeypatch.delenv("HYMET_ANCHOR_LEGACY", raising=False)
            else:
                monkeypatch.setenv("HYMET_ANCHOR_LEGACY", env)
            gpu.prof_reset()
            res = mapper.map_part(gpu, part, qpool, opt)
            out[form] = (res, {k for k, v in gpu.prof_table().items() if v[1] > 0})
    finally:
        gpu.prof(False)
    (rw, sw), (rt, st) = out["words"], out["twokey"]
    assert "mm_anchor_gsort" in sw and "radix_sort_anchor_group" not in sw
    assert "radix_sort_anchor_group" in st and "mm_anchor_gsort" not in st
    for s in (sw, st):   # the long join chained a set of its own
        assert "mm_chain_long" in s or "mm_chain_long_small" in s
    assert (np.diff(rw.off)[:3] > 0).all()
    np.testing.assert_array_equal(rw.off, rt.off)
    np.testing.assert_array_equal(rw.rep_len, rt.rep_len)
    for f in rw.regs.dtype.names:
        np.testing.assert_array_equal(rw.regs[f], rt.regs[f], err_msg=f)
