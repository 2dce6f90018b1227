"""The backtrack's marks are one byte per anchor (0 free, 1 used by a dropped walk, 2 in a kept
chain), so neighbouring (strand, target) groups -- each marked by one thread or one wave --
share 32-bit words and the long join's 16-byte loads.

Narrowing: hymet_mm_mark_compact still takes int32 marks and narrows them on upload as
m == 2 ? 2 : (m != 0).  Marks drawn from {0, 1, 2, 7, 258, 2 + (1 << 16), -2}: only == 2 keeps
(258 and 2 + 65536 would be 2 after a plain truncation to a byte).

Shared words: a small mapping whose first-pass set has many neighbouring groups of sizes not
divisible by 4 (checked on the oracle's anchors), PAF lines identical to the oracle's, with
HYMET_BT_LONG unset (groups above 64 anchors go to the wave-per-group backtrack) and = 8 (so
the small odd groups meet it too); one query takes the long join.
"""
import ctypes

import numpy as np
import pytest

from tests._data import mutate, rand_seq, revcomp
from tests.test_mark_compact_gpu import anchors, expected, mark_compact, offsets, random_cuts

pytestmark = pytest.mark.gpu

MARKS = np.array([0, 1, 2, 7, 258, 2 + (1 << 16), -2], np.int32)


@pytest.fixture(scope="module")
def gpu():
    from hymet_amd._lib import Gpu
    return Gpu(0)


@pytest.mark.parametrize("n", [65, 4097])
def test_marks_narrowed_on_upload(gpu, n):
    rng = np.random.default_rng(n)
    x, y = anchors(rng, n, random_cuts(rng, n))
    mark = MARKS[rng.integers(0, len(MARKS), n)]
    mark[:len(MARKS)] = MARKS                      # every value at least once
    qoff = offsets(n, [n // 3, n // 3, n - 9])     # an empty query among them
    qflag = np.array([1, 0, 1, 1], np.uint32)
    kx, ky, head = expected(x, y, mark, qoff, qflag)
    keep_all_flagged = (mark == 2).sum()
    assert 0 < len(kx) <= keep_all_flagged < n
    assert ((mark & 0xff) == 2).sum() > keep_all_flagged   # truncation would keep more
    rc, ox, oy, bits = mark_compact(gpu, x, y, mark, qoff, qflag)
    assert rc == 0, gpu.lib.hymet_last_error()
    print(f"n {n}: kept {len(ox)}, expected {len(kx)}")
    np.testing.assert_array_equal(ox, kx)
    np.testing.assert_array_equal(oy, ky)
    np.testing.assert_array_equal(bits, head)


SMALL = [25, 30, 35, 40, 45, 50, 60, 70, 85, 100, 130, 160, 200, 260, 330, 420, 560, 700, 900, 1300]
PIECES = [(0, 20_000), (15_000, 27_000), (25_000, 28_000), (26_000, 41_000), (40_000, 42_500), (38_000, 60_000),
          (5_000, 11_000), (44_000, 52_000)]


def odd_groups_input():
    """Eight 2.5-22 kbp targets, mutated copies of overlapping pieces of one base (so a stretch
    of the base hits two or three of them: neighbouring groups), 60 short queries of one or two
    25-1,300 bp stretches of them on either strand, a query of two stretches of one target
    5.5 kbp apart (the long join) and a 13.5 kbp one."""
    rng = np.random.default_rng(1105)
    base = rand_seq(rng, 60_000)
    refs = [mutate(rng, base[a:b], 0.01 + 0.005 * (i % 4)) for i, (a, b) in enumerate(PIECES)]
    names = [f"NC_{i:06d}.1" for i in range(len(refs))]

    def stitch(lens, seed):
        r = np.random.default_rng(seed)
        out = []
        for L in lens:
            t = int(r.integers(len(refs)))
            s0 = int(r.integers(0, len(refs[t]) - L))
            seg = refs[t][s0:s0 + L]
            out.append(revcomp(seg) if r.random() < 0.4 else seg)
        return b"".join(out)

    qs = [(f"s{i}", stitch([SMALL[i % 20]] + ([SMALL[(7 * i) % 20]] if i % 3 == 0 else []), 100 + i)) for i in range(60)]
    qs += [("join", mutate(rng, refs[0][1_000:7_000] + refs[0][12_500:19_000], 0.01)),
           ("long", mutate(rng, base[26_500:40_000], 0.01))]
    return refs, names, qs


def test_map_odd_groups_share_mark_words(gpu, monkeypatch):
    from hymet_amd import mapper
    from hymet_amd.seqio import DevicePool, from_records
    from oracle import oracle_lib as ol
    refs, names, qs = odd_groups_input()
    ss = from_records([(n, "", s) for n, s in zip(names, refs)])
    part = mapper.IndexPart(gpu, ss)
    opt = mapper.MapOpt.asm10()
    opt.resolve_mid_occ(part)
    assert opt.bw_long > opt.bw   # the long join is on
    oi = ol.MmIndex(refs, names=names)
    oopt = ol.asm10_opt()
    ol._mm_lib().mmo_opt_update_mid_occ(ctypes.byref(oopt), oi.h)
    assert oopt.mid_occ == opt.mid_occ
    # the oracle's side: group sizes of the first-pass set, and the expected PAF
    sizes, o_lines = [], []
    for name, s in qs:
        a, _ = ol.mm_debug_anchors(oi, oopt, s)
        g = a[:, 0] >> np.uint64(32)
        heads = np.flatnonzero(np.r_[True, g[1:] != g[:-1]]) if len(g) else np.empty(0, np.int64)
        sizes += np.diff(np.r_[heads, len(g)]).tolist()
        oregs, orl = ol.mm_map(oi, oopt, s, name)
        o_lines.append(ol.format_paf(name, len(s), oregs, orl, names, ss.lengths))
    sizes = np.array(sizes)
    odd = sizes % 4 != 0
    print("groups", len(sizes), "not divisible by 4:", int(odd.sum()), "neighbouring pairs of them:",
          int((odd[1:] & odd[:-1]).sum()), "sizes", sorted(set(sizes.tolist())))
    assert odd.sum() >= 100 and (odd[1:] & odd[:-1]).sum() >= 60
    assert {1, 2, 3, 5, 7, 13, 63, 65} <= set(sizes.tolist())
    assert (odd & (sizes > 8) & (sizes <= 64)).sum() >= 20 and (odd & (sizes > 64)).sum() >= 10
    assert sum(len(l) for l in o_lines) > len(qs) // 2

    qpool = DevicePool(gpu, from_records([(n, "", s) for n, s in qs]), DevicePool.ALPHA_MINIMAP2)
    gpu.prof(True)
    try:
        for bt_long in (None, "8"):
            if bt_long is None:
                monkeypatch.delenv("HYMET_BT_LONG", raising=False)
            else:
                monkeypatch.setenv("HYMET_BT_LONG", bt_long)
            gpu.prof_reset()
            res = mapper.map_part(gpu, part, qpool, opt)
            scopes = {k for k, v in gpu.prof_table().items() if v[1] > 0}
            assert "mm_backtrack.long" in scopes
            assert "mm_chain_long" in scopes or "mm_chain_long_small" in scopes   # a long join chained a set
            bad = 0
            for qi, (name, s) in enumerate(qs):
                g_lines = mapper.paf_lines(name, len(s), res.query(qi), int(res.rep_len[qi]), names, ss.lengths)
                bad += g_lines != o_lines[qi]
            print(f"HYMET_BT_LONG {bt_long}: queries whose PAF differs from the oracle's: {bad} of {len(qs)}")
            for qi, (name, s) in enumerate(qs):
                g_lines = mapper.paf_lines(name, len(s), res.query(qi), int(res.rep_len[qi]), names, ss.lengths)
                assert g_lines == o_lines[qi], (bt_long, name)
    finally:
        gpu.prof(False)
