"""The anchor word W = (rev | rid | rpos) << ybits | y at the edge of its 63 bits: the grouped
anchor sort through hymet_mm_anchor_sort (which packs the caller's key / value pairs into
words on the device), exact against np.lexsort on (query, rev, rid, rpos, y), with target
positions of all ones and y = max_qlen in every shape -- a query sorted whole in one block, a
tiled query with a group for the device radix sort and two small groups, queries at the
thread / wave / block class boundaries and an empty one -- with 2,048 (strand, target) bins
(the order-preserving scatter), with 4,096 (the atomic ranking) and with coarse bins; a layout
one bit too wide, which the entry declines; a y beyond its field, which it rejects; and a
small mapping with anchors emitted as words for the grouped sort and through the two-key
fallback (the path of layouts without a word), whose region records must not differ.
"""
import ctypes

import numpy as np
import pytest

from tests._data import mutate, rand_seq, revcomp

pytestmark = pytest.mark.gpu

MAX_QLEN = (1 << 20) - 1   # ybits = 20
YHI = 15
HYMET_E_ARG = -2


@pytest.fixture(scope="module")
def gpu():
    from hymet_amd._lib import Gpu
    return Gpu(0)


def vp(a):
    return ctypes.c_void_p(a.ctypes.data)


def anchor_sort_rc(g, key, val, qoff, rb, pb, max_qlen):
    """(return code, ax, ay, ax32, head bits as a bool array) of one hymet_mm_anchor_sort call."""
    key = np.ascontiguousarray(key, np.uint64)
    val = np.ascontiguousarray(val, np.uint32)
    qoff = np.ascontiguousarray(qoff, np.int64)
    n = len(key)
    ax, ay = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    ax32 = np.zeros(n, np.uint32)
    hb = np.zeros((n + 31) // 32, np.uint32)
    rc = g.lib.hymet_mm_anchor_sort(g.ctx, vp(key), vp(val), n, vp(qoff), len(qoff) - 1, rb, pb, YHI, max_qlen, vp(ax), vp(ay),
                                    vp(ax32), vp(hb), None)
    bits = (hb[np.arange(n) >> 5] >> (np.arange(n, dtype=np.uint32) & np.uint32(31)) & np.uint32(1)).astype(bool)
    return rc, ax, ay, ax32, bits


def group(rng, m, rev, rid, pb, shape, max_qlen=MAX_QLEN):
    """m anchors of one (strand, target) group in emission order: (rev, rid, rpos, y) columns.
    shape "rise": target positions rise along the query but for a few stray hits (the block
    sorts' outlier path); "shuffle": any order (their full sort).  Some positions repeat with
    other y (ties on the key), and the group holds rpos = 2^pb - 1 and y = max_qlen."""
    top = (1 << pb) - 1
    rpos = np.sort(rng.integers(0, 1 << pb, m, dtype=np.int64))
    if m >= 4:
        rpos[1] = rpos[0]                   # a tie on (rev, rid, rpos): y decides
        rpos[-2:] = top                     # twice the largest position
    else:
        rpos[-1] = top
    if shape == "shuffle":
        rng.shuffle(rpos)
    elif m >= 64:
        stray = rng.choice(m, max(1, m // 200), replace=False)
        rpos[stray] = rng.integers(0, 1 << pb, len(stray), dtype=np.int64)
    y = rng.integers(0, max_qlen + 1, m, dtype=np.int64)
    y[rng.integers(0, m)] = max_qlen
    if m >= 4:
        y[-2], y[-1] = max_qlen, 0          # emitted before its equal-key neighbour, sorted after it
    return np.full(m, rev), np.full(m, rid), rpos, y


def interleave(rng, groups):
    """The groups' anchors merged as the emitter does: each group's in their own order, the
    groups taking turns at random."""
    owner = rng.permutation(np.concatenate([np.full(len(g[0]), i) for i, g in enumerate(groups)]))
    cols = [np.empty(len(owner), np.int64) for _ in range(4)]
    for i, g in enumerate(groups):
        at = np.nonzero(owner == i)[0]
        for c, col in zip(cols, g):
            c[at] = col
    return cols


def make_case(rb, pb, max_qlen=MAX_QLEN):
    """Queries: 3,000 anchors (whole-query block sort); ~40,000 anchors in tiles, with a group of
    17,000 (above 16,384: the device radix sort), two small groups (5 and 40) and block-sorted
    ones; 1, 8, 9, 64 and 65 anchors; none.  With rb = 12 neighbouring targets (2k, 2k + 1)
    share a coarse bin."""
    rng = np.random.default_rng(1000 + rb)
    top_rid = (1 << rb) - 1
    q = []
    q.append(interleave(rng, [group(rng, 1400, 0, 6, pb, "rise", max_qlen), group(rng, 1000, 1, 6, pb, "shuffle", max_qlen),
                              group(rng, 593, 0, top_rid, pb, "rise", max_qlen), group(rng, 7, 1, 7, pb, "shuffle", max_qlen)]))
    q.append(interleave(rng, [group(rng, 17000, 0, 20, pb, "rise", max_qlen), group(rng, 5, 1, 20, pb, "shuffle", max_qlen),
                              group(rng, 40, 0, 21, pb, "shuffle", max_qlen), group(rng, 9000, 1, 21, pb, "rise", max_qlen),
                              group(rng, 6000, 0, top_rid - 1, pb, "shuffle", max_qlen), group(rng, 4200, 0, top_rid, pb, "rise", max_qlen),
                              group(rng, 3754, 1, 0, pb, "rise", max_qlen), group(rng, 1, 1, 1, pb, "shuffle", max_qlen)]))
    for m in (1, 8, 9, 64, 65):
        q.append(interleave(rng, [group(rng, m - m // 2, 0, 2, pb, "shuffle", max_qlen)] +
                            ([group(rng, m // 2, 1, 3, pb, "rise", max_qlen)] if m // 2 else [])))
    q.append([np.empty(0, np.int64)] * 4)
    qoff = np.zeros(len(q) + 1, np.int64)
    qoff[1:] = np.cumsum([len(c[0]) for c in q])
    qid = np.concatenate([np.full(len(c[0]), i) for i, c in enumerate(q)])
    rev, rid, rpos, y = (np.concatenate([c[j] for c in q]) for j in range(4))
    return qid, rev, rid, rpos, y, qoff


@pytest.mark.parametrize("rb,pb,max_qlen", [(11, 31, MAX_QLEN), (12, 30, MAX_QLEN), (10, 31, (1 << 21) - 1)])
def test_word_at_63_bits(gpu, rb, pb, max_qlen):
    """rb = 11, pb = 31: 4,096 (strand, target) bins, ranked by atomics; rb = 12: coarse bins of
    two targets, with pb = 30 so that the word is again 63 bits; rb = 10 with 21 bits of y:
    2,048 bins, the order-preserving scatter (the kernel of parts up to 1,023 targets)."""
    assert 1 + rb + pb + int(max_qlen).bit_length() == 63
    qid, rev, rid, rpos, y, qoff = make_case(rb, pb, max_qlen)
    u = lambda a: a.astype(np.uint64)  # noqa: E731
    key = u(qid) << np.uint64(1 + rb + pb) | u(rev) << np.uint64(rb + pb) | u(rid) << np.uint64(pb) | u(rpos)
    assert (rpos == (1 << pb) - 1).any() and (y == max_qlen).any()
    rc, ax, ay, ax32, bits = anchor_sort_rc(gpu, key, y.astype(np.uint32), qoff, rb, pb, max_qlen)
    assert rc == 0
    o = np.lexsort((y, rpos, rid, rev, qid))
    np.testing.assert_array_equal(ax, u(rev[o]) << np.uint64(63) | u(rid[o]) << np.uint64(32) | u(rpos[o]))
    np.testing.assert_array_equal(ay, np.uint64(YHI << 32) | u(y[o]))
    np.testing.assert_array_equal(ax32, rpos[o].astype(np.uint32))
    g = np.stack([qid[o], rev[o], rid[o]])
    head = np.ones(len(o), bool)
    head[1:] = (g[:, 1:] != g[:, :-1]).any(axis=0)
    np.testing.assert_array_equal(bits, head)


def test_word_of_64_bits_is_declined(gpu):
    """max_qlen = 2^20 takes 21 bits of y: 1 + 11 + 31 + 21 = 64, no word -- the fallback code."""
    qid, rev, rid, rpos, y, qoff = make_case(11, 31)
    u = lambda a: a.astype(np.uint64)  # noqa: E731
    key = u(qid) << np.uint64(43) | u(rev) << np.uint64(42) | u(rid) << np.uint64(31) | u(rpos)
    rc, ax, ay, _, bits = anchor_sort_rc(gpu, key, y.astype(np.uint32), qoff, 11, 31, 1 << 20)
    assert rc == 1
    assert not ax.any() and not ay.any() and not bits.any()   # nothing written


def test_y_beyond_its_field_is_rejected(gpu):
    """One y of 21 bits where max_qlen has 20: it would run into the position bits of the word."""
    qid, rev, rid, rpos, y, qoff = make_case(11, 31)
    u = lambda a: a.astype(np.uint64)  # noqa: E731
    key = u(qid) << np.uint64(43) | u(rev) << np.uint64(42) | u(rid) << np.uint64(31) | u(rpos)
    y[len(y) // 2] = MAX_QLEN + 1
    rc, ax, ay, _, bits = anchor_sort_rc(gpu, key, y.astype(np.uint32), qoff, 11, 31, MAX_QLEN)
    assert rc == HYMET_E_ARG
    assert b"y value" in gpu.lib.hymet_last_error()
    assert not ax.any() and not ay.any() and not bits.any()   # nothing written


def test_map_with_words_and_with_pairs(gpu, monkeypatch):
    """One small mapping twice: HYMET_ANCHOR_LEGACY unset (anchors emitted as words, grouped
    sort) and = 1 (the two-key fallback: raw anchors, two device sorts, gathers).  The
    profiler's scopes say which form ran; the region records are the same."""
    from hymet_amd import mapper
    from hymet_amd.seqio import DevicePool, from_records
    rng = np.random.default_rng(77)
    base = rand_seq(rng, 120_000)
    refs = [base, mutate(rng, base, 0.02), rand_seq(rng, 60_000)]
    ss = from_records([(f"NC_{i:06d}.1", "", s) for i, s in enumerate(refs)])
    part = mapper.IndexPart(gpu, ss)
    opt = mapper.MapOpt.asm10()
    opt.resolve_mid_occ(part)
    qs = [mutate(rng, base[5_000:95_000], 0.01),            # > 4,096 anchors: tiled
          revcomp(mutate(rng, base[20_000:26_000], 0.03)),
          mutate(rng, refs[2][1_000:4_000], 0.0),
          refs[2][30_000:30_040], b""]
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
    assert (np.diff(rw.off)[:3] > 0).all()   # the three queries cut from the targets map
    np.testing.assert_array_equal(rw.off, rt.off)
    np.testing.assert_array_equal(rw.rep_len, rt.rep_len)
    for f in rw.regs.dtype.names:
        np.testing.assert_array_equal(rw.regs[f], rt.regs[f], err_msg=f)
