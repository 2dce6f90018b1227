"""Chain statistics (chain_rec_kernel + chain_stats_flat_kernel: mlen, blen and mm_est_err's
walk per chain) through hymet_mm_map, whole region records and PAF lines against the minimap2
restatement in oracle/mm_oracle.c.  The inputs put chain boundaries where the kernel changes
path: at a wave's edge lanes (the halo positions), inside waves, across blocks, in blocks
inside one chain, and beyond the chain records a block stages in LDS."""
import ctypes

import numpy as np
import pytest

from tests._data import mutate, rand_seq, revcomp
from tests.test_mm_map_gpu import gpu  # noqa: F401  (the module-scoped context fixture)

pytestmark = pytest.mark.gpu

# Query lengths whose one chain against an exact copy has 63, 64, 65, 127, 128, 129, 575, 576,
# 577, 639, 640, 1087, 1088, 1089 and 1151 anchors (found with the oracle; the test asserts the
# classes from the oracle's cm, so a drifted sweep fails)
SWEEP = [340, 350, 354, 698, 705, 715, 3061, 3062, 3072, 3425, 3426, 5871, 5879, 5883, 6214]
FIELDS = ("qs", "qe", "rs", "re", "rid", "rev", "mlen", "blen", "mapq", "cnt", "score", "subsc", "parent", "id", "n_sub")


def _sweep_seq():
    return rand_seq(np.random.default_rng(12), 7000)


def _copies(rng, base, n, rate):
    """n diverged copies of base, every third reverse-complemented, each between random flanks."""
    return [rand_seq(rng, 200) + (mutate(rng, base, rate) if i % 3 else revcomp(mutate(rng, base, rate))) + rand_seq(rng, 200)
            for i in range(n)]


def _map_both(gpu, refs, qs):  # noqa: F811
    """Map qs against refs on the GPU and with the oracle; assert identical records and PAF
    lines; return (oracle records, GPU records) per query."""
    from hymet_amd import mapper
    from hymet_amd.seqio import DevicePool, from_records
    from oracle import oracle_lib as ol
    names = [f"NC_{i:06d}.1" for i in range(len(refs))]
    ss = from_records([(n, "", s) for n, s in zip(names, refs)])
    part = mapper.IndexPart(gpu, ss)
    opt = mapper.MapOpt.asm10()
    opt.resolve_mid_occ(part)
    oi = ol.MmIndex(refs, names=names)
    oopt = ol.asm10_opt()
    ol._mm_lib().mmo_opt_update_mid_occ(ctypes.byref(oopt), oi.h)
    assert oopt.mid_occ == opt.mid_occ
    qpool = DevicePool(gpu, from_records([(n, "", s) for n, s in qs]), DevicePool.ALPHA_MINIMAP2)
    res = mapper.map_part(gpu, part, qpool, opt)
    out_o, out_g = [], []
    for qi, (name, s) in enumerate(qs):
        oregs, orl = ol.mm_map(oi, oopt, s, name)
        gregs = res.query(qi).copy()
        assert res.rep_len[qi] == orl, name
        assert len(gregs) == len(oregs), (name, len(gregs), len(oregs))
        for f in FIELDS:
            np.testing.assert_array_equal(gregs[f], oregs[f], err_msg=f"{name}:{f}")
        np.testing.assert_array_equal(gregs["div"], oregs["div"], err_msg=name)
        assert mapper.paf_lines(name, len(s), gregs, int(res.rep_len[qi]), names, ss.lengths) == \
            ol.format_paf(name, len(s), oregs, orl, names, ss.lengths), name
        out_o.append(oregs)
        out_g.append(gregs)
    return out_o, out_g


@pytest.mark.parametrize("strand", ["fwd", "rev"])
def test_length_sweep(gpu, strand):  # noqa: F811
    """One chain per query against an exact copy (fwd) or its reverse complement (rev: est_err
    walks the chain backwards, so the successor halo orders it): anchor counts at 64 k - 1,
    64 k and 64 k + 1, below 512, between 512 and 1,024 (chains that cross blocks) and above
    1,024 (at least one block inside one chain)."""
    seq = _sweep_seq()
    qs = [(f"len{L}", seq[:L]) for L in SWEEP]
    oregs, _ = _map_both(gpu, [seq if strand == "fwd" else revcomp(seq)], qs)
    assert all(len(r) == 1 and r[0]["rev"] == (strand == "rev") for r in oregs)
    cm = [int(r[0]["cnt"]) for r in oregs]
    for rem in (0, 1, 63):
        for lo, hi in ((0, 512), (512, 1024), (1024, 1 << 30)):
            assert any(c % 64 == rem and lo < c <= hi for c in cm), (rem, lo, hi, cm)


def test_many_short_chains(gpu):  # noqa: F811
    """One query against 36 diverged copies, a third of them reverse-complemented: chains of
    ~100 anchors, so chain boundaries fall inside waves and several chains share a block."""
    rng = np.random.default_rng(13)
    base = rand_seq(rng, 1000)
    oregs, _ = _map_both(gpu, _copies(rng, base, 36, 0.03), [("multi", base)])
    cm = oregs[0]["cnt"]
    assert len(cm) == 36 and cm.min() >= 64 and cm.max() <= 160, cm
    assert 0 < int(oregs[0]["rev"].sum()) < 36


def test_mixed_batch_beyond_staged_chains(gpu, monkeypatch):  # noqa: F811
    """Queries the long join re-chains (36 chains each: their first-pass chains take no slots in
    the chain order, a run of empty chains) between queries of one chain, which keep their
    first-pass chain.  With four chain records staged per block the positions after such a
    run lie beyond the staged chains and take the search over the chain offsets; the default
    stages every chain of these blocks.  Both runs: the oracle's records, and each other's."""
    rng = np.random.default_rng(14)
    seq = _sweep_seq()
    base = rand_seq(rng, 1000)
    refs = [seq] + _copies(rng, base, 36, 0.03)
    qs = []
    for i, L in enumerate((350, 705, 3062, 354)):
        qs.append((f"one{i}", seq[:L]))
        if i < 3:
            qs.append((f"multi{i}", mutate(rng, base, 0.005 * i)))
    runs = []
    for stage in ("4", None):
        if stage is None:
            monkeypatch.delenv("HYMET_STAT_STAGE", raising=False)
        else:
            monkeypatch.setenv("HYMET_STAT_STAGE", stage)
        oregs, gregs = _map_both(gpu, refs, qs)
        for (name, _), r in zip(qs, oregs):
            assert len(r) == 1 if name.startswith("one") else len(r) > 4, (name, len(r))
        runs.append(gregs)
    for (name, _), a, b in zip(qs, *runs):
        assert a.tobytes() == b.tobytes(), name
