"""The streamed read-set sketch (csrc/sketch_stream.hip through sketch.sketch_stream, sketch_files
and the CLI) against the plain-Python restatement tests/_reads_ref.py and against the one-batch
path (sketch_pool_counted): hashes and multiplicities, exact equality, whatever the batches, the
slices and max_live."""
import ctypes
from functools import lru_cache

import numpy as np
import pytest

from tests import _reads_ref as rr
from tests._data import add_noise, rand_seq, revcomp

pytestmark = pytest.mark.gpu

E_ARG = -2
SLICES = (1_000, 4_099, 1 << 40)
PARAMS = [(21, 42, 1000, 2), (21, 42, 1000, 3), (16, 42, 1000, 2), (32, 7, 200, 2), (9, 42, 200, 2), (21, 42, 1, 2),
          (21, 42, 1000, 1)]


@pytest.fixture(scope="module")
def gpu():
    from hymet_amd._lib import Gpu
    return Gpu(0)


def _batches(seqs, per):
    """The reads as SeqSets of `per` reads each (the last may be shorter); per=None: one batch."""
    from hymet_amd.seqio import from_records
    seqs = list(seqs)
    per = per or max(len(seqs), 1)
    return [from_records([(f"r{i + j}", "", s) for j, s in enumerate(seqs[i:i + per])])
            for i in range(0, max(len(seqs), 1), per)]


@lru_cache(maxsize=None)
def _counter(k, seed):
    return rr.hash_counter(rr.read_set(), k, seed)


def _want(k, seed, s, m):
    cnt = _counter(k, seed)
    keep = sorted(h for h, c in cnt.items() if c >= m)[:s]
    return np.array(keep, np.uint64), np.array([cnt[h] for h in keep], np.uint32)


def _equal(got, want, what=""):
    assert got[0].dtype == np.uint64 and got[1].dtype == np.uint32
    assert len(got[0]) == len(want[0]) == len(got[1]), (what, len(got[0]), len(want[0]))
    np.testing.assert_array_equal(got[0], want[0], err_msg=f"hashes {what}")
    np.testing.assert_array_equal(got[1], want[1], err_msg=f"counts {what}")


@pytest.mark.parametrize("k,seed,s,m", PARAMS)
def test_parity_whatever_the_batches_and_slices(gpu, k, seed, s, m):
    from hymet_amd import sketch as sk
    from hymet_amd.seqio import DevicePool
    reads = rr.read_set()
    want = _want(k, seed, s, m)
    whole = _batches(reads, None)
    pool = DevicePool(gpu, whole[0], DevicePool.ALPHA_MASH)
    (one_batch,) = sk.sketch_pool_counted(gpu, pool, np.zeros(len(reads), np.int64), k, seed, s, m)
    _equal(one_batch, want, "sketch_pool_counted")
    for per, n_batches in ((7, 46), (50, 7), (None, 1)):
        batches = _batches(reads, per)
        assert len(batches) == n_batches
        for sl in SLICES:
            got = sk.sketch_stream(gpu, batches, k, seed, s, m, slice_bases=sl)
            _equal(got, want, f"{per} reads per batch, slices of {sl}")
            _equal(got, one_batch)
            st = sk.sketch_stream.stats
            assert st["passes"] == 1
            starts = sum(max(len(b.buf) - k + 1, 0) for b in batches)
            assert st["slices"] == sum(-(-max(len(b.buf) - k + 1, 0) // sl) for b in batches)
            assert 0 < st["emitted"] <= starts and 0 < st["max_live"] <= st["emitted"]
    if (k, s, m) == (21, 1000, 2):
        assert len(want[0]) == 1000
        # the default slice and max_live
        _equal(sk.sketch_stream(gpu, _batches(reads, 50), k, seed, s, m), want, "defaults")


def test_the_other_shapes_of_the_parity_pool(gpu):
    from hymet_amd import sketch as sk
    reads = list(rr.read_set())
    rng = np.random.default_rng(99)
    k, seed, s, m = 21, 42, 1000, 2

    def run(seqs, per, sl=4_099, **kw):
        return sk.sketch_stream(gpu, _batches(seqs, per), k, seed, s, m, slice_bases=sl, **kw)

    # fewer than s qualifiers: a short row, one pass, nothing more asked for
    few = run(reads[:20], 7)
    _equal(few, rr.counted_ref(reads[:20], k, seed, s, m), "reads[:20]")
    assert 0 < len(few[0]) < s and sk.sketch_stream.stats["passes"] == 1
    # one read three times, ten once
    tripled = [reads[0]] * 3 + reads[40:50]
    h3, c3 = run(tripled, 2)
    _equal((h3, c3), rr.counted_ref(tripled, k, seed, s, m), "tripled")
    assert len(h3) >= 130 and c3.min() >= 2 and c3.max() >= 3
    # nothing to hash: records shorter than k, an empty record, no record
    for seqs in ([b"ACGTACGT", b"TTGACA", b"GGGGGGGG"], [b""], []):
        for per in (1, None):
            h, c = run(seqs, per)
            assert len(h) == 0 and len(c) == 0 and h.dtype == np.uint64 and c.dtype == np.uint32
            assert sk.sketch_stream.stats["passes"] == 1
    # N runs, IUPAC codes, lower case
    noisy = [add_noise(rng, r) for r in reads[100:160]]
    for per in (7, None):
        _equal(run(noisy, per, sl=1_000), rr.counted_ref(noisy, k, seed, s, m), "noisy")
    # the other strand: the same canonical k-mers
    fwd = run(reads, 50)
    _equal(run([revcomp(r) for r in reads], 50), fwd, "reverse complement")
    _equal(fwd, _want(k, seed, s, m))
    # a read ends the batch: no k-mer spans two batches (the restatement counts per read)
    for cut in (1, 160, 319):
        from hymet_amd.seqio import from_records
        two = [from_records([(f"r{i}", "", r) for i, r in enumerate(part)]) for part in (reads[:cut], reads[cut:])]
        _equal(sk.sketch_stream(gpu, two, k, seed, s, m, slice_bases=1 << 40), fwd, f"cut at read {cut}")
    # preserve case is the pool's alphabet
    from hymet_amd.seqio import DevicePool
    low = [r[:70] + r[70:].lower() for r in reads[:60]]
    got = sk.sketch_stream(gpu, _batches(low, 7), k, seed, s, m, alphabet=DevicePool.ALPHA_MASH_PRESERVE_CASE)
    _equal(got, rr.counted_ref(low, k, seed, s, m, preserve_case=True), "preserve case")


@pytest.mark.parametrize("max_live,sl", [(256, 4_099), (16, 1 << 40)])
def test_forced_cut(gpu, max_live, sl):
    """A window of max_live pairs: more passes, the same row.  The pass bound: a cut pass that
    does not finish retires at least max_live / 2 distinct hashes at or below the row's last."""
    from hymet_amd import sketch as sk
    reads = rr.read_set()
    k, seed, s, m = 21, 42, 1000, 2
    batches = _batches(reads, None)
    uncapped = sk.sketch_stream(gpu, batches, k, seed, s, m, slice_bases=sl)
    assert sk.sketch_stream.stats["passes"] == 1
    got = sk.sketch_stream(gpu, batches, k, seed, s, m, max_live=max_live, slice_bases=sl)
    st = dict(sk.sketch_stream.stats)
    _equal(got, uncapped, "capped against uncapped")
    _equal(got, _want(k, seed, s, m))
    last = int(got[0][-1])
    D = sum(1 for h in _counter(k, seed) if h <= last)
    print(f"max_live {max_live}: {st}, D = {D}")
    assert 1 < st["passes"] <= D // (max_live // 2) + 1
    starts = len(batches[0].buf) - k + 1
    assert st["max_live"] <= max_live + min(sl, starts)
    # next to nothing qualifies: the whole set is walked through max_live / 2 hashes at a time
    rng = np.random.default_rng(4)
    strangers = [rand_seq(rng, 150) for _ in range(40)]
    cnt = rr.hash_counter(strangers, k, seed)
    got = sk.sketch_stream(gpu, _batches(strangers, None), k, seed, s, m, max_live=max_live, slice_bases=sl)
    st = dict(sk.sketch_stream.stats)
    _equal(got, rr.counted_ref(strangers, k, seed, s, m), "strangers")
    assert len(got[0]) <= 2
    print(f"max_live {max_live}, strangers: {st}, distinct = {len(cnt)}")
    assert 1 < st["passes"] <= len(cnt) // (max_live // 2) + 1


class _Handle:
    """One hymet_sketch_stream, fed packed pools directly."""

    def __init__(self, gpu, k, seed, s, m, max_live=1 << 28):
        from hymet_amd._lib import check
        self.gpu, self.s, self.h = gpu, s, ctypes.c_void_p()
        check(gpu.lib.hymet_sketch_stream_create(gpu.ctx, k, seed, s, m, max_live, ctypes.byref(self.h)), "create")

    def add(self, pool, slice_bases=1 << 24):
        from hymet_amd._lib import ptr
        return self.gpu.lib.hymet_sketch_stream_add(self.h, ptr(pool.w2b), ptr(pool.wmask), pool.n_bases, slice_bases)

    def end_pass(self):
        more = ctypes.c_int32(-1)
        assert self.gpu.lib.hymet_sketch_stream_end_pass(self.h, ctypes.byref(more)) == 0
        return more.value

    def result(self):
        from hymet_amd._lib import ptr
        torch = self.gpu.torch
        out = self.gpu.zeros(self.s, torch.int64)
        out_c = self.gpu.zeros(self.s, torch.int32)
        n = ctypes.c_int32(-1)
        stats = (ctypes.c_int64 * 4)()
        rc = self.gpu.lib.hymet_sketch_stream_result(self.h, ptr(out), ptr(out_c), ctypes.byref(n),
                                                     ctypes.cast(stats, ctypes.c_void_p))
        if rc:
            return rc, None, None, None
        return (0, out.cpu().numpy().view(np.uint64)[:n.value], out_c.cpu().numpy().view(np.uint32)[:n.value],
                [int(x) for x in stats])

    def close(self):
        self.gpu.lib.hymet_sketch_stream_destroy(self.h)
        self.h = None


def test_beyond_two_to_the_32_positions_and_saturation(gpu):
    """One k-mer 257 x (2^24 - 20) = 2^32 + 16,772,076 times through one handle: no refusal, and
    the count stops at 2^32 - 1.  Seen on an MI355X: 1.3 s for the 257 feedings."""
    import time
    from hymet_amd.seqio import DevicePool, from_records
    k, seed = 21, 42
    pool = DevicePool(gpu, from_records([("polyA", "", b"A" * (1 << 24))]), DevicePool.ALPHA_MASH)
    assert 257 * ((1 << 24) - k + 1) > 1 << 32
    h = _Handle(gpu, k, seed, 1, 2)
    try:
        t0 = time.perf_counter()
        for _ in range(257):
            assert h.add(pool) == 0
        assert h.end_pass() == 0
        rc, hashes, counts, stats = h.result()
        print(f"poly-A: 257 feedings of 2^24 bases in {time.perf_counter() - t0:.2f} s, stats {stats}")
    finally:
        h.close()
    assert rc == 0
    (a21,) = rr.hash_counter([b"A" * k], k, seed)
    assert hashes.tolist() == [a21] and counts.tolist() == [(1 << 32) - 1]
    assert stats[0] == 1 and stats[1] >= 257 and stats[2] == 257 * ((1 << 24) - k + 1)
    del pool

    # a random pool three times: the same hashes, three times the counts
    rng = np.random.default_rng(12)
    rand = DevicePool(gpu, from_records([("rand", "", rand_seq(rng, 1 << 22))]), DevicePool.ALPHA_MASH)
    rows = {}
    for times, m in ((1, 1), (3, 1), (3, 3)):
        h = _Handle(gpu, k, seed, 1000, m)
        try:
            for _ in range(times):
                assert h.add(rand, 1 << 20) == 0
            assert h.end_pass() == 0
            rc, hashes, counts, stats = h.result()
        finally:
            h.close()
        assert rc == 0 and len(hashes) == 1000 and stats[0] == 1 and stats[1] == 4 * times
        rows[times, m] = (hashes, counts)
    np.testing.assert_array_equal(rows[3, 1][0], rows[1, 1][0])
    np.testing.assert_array_equal(rows[3, 1][1], 3 * rows[1, 1][1])
    np.testing.assert_array_equal(rows[3, 3][0], rows[1, 1][0])
    np.testing.assert_array_equal(rows[3, 3][1], 3 * rows[1, 1][1])
    assert (np.diff(rows[1, 1][0].astype(object)) > 0).all() and rows[1, 1][1].min() >= 1


def test_refusals(gpu):
    """Bad arguments fail in the host checks with a message naming the function."""
    from hymet_amd import sketch as sk
    from hymet_amd._lib import ptr
    from hymet_amd.seqio import DevicePool
    lib = gpu.lib
    smax = sk.max_counted_sketch_size()

    def create(k=21, s=1000, m=2, max_live=1 << 20):
        h = ctypes.c_void_p()
        rc = lib.hymet_sketch_stream_create(gpu.ctx, k, 42, s, m, max_live, ctypes.byref(h))
        return rc, h

    def rejected(fn, rc):
        assert rc == E_ARG
        msg = lib.hymet_last_error()
        assert msg and fn.encode() in msg, msg

    for kw in (dict(k=0), dict(k=33), dict(s=0), dict(s=smax + 1), dict(m=0), dict(m=-3), dict(max_live=1), dict(max_live=0)):
        rc, h = create(**kw)
        rejected("hymet_sketch_stream_create", rc)
        assert not h.value
    for kw in (dict(k=1), dict(k=32), dict(s=smax), dict(max_live=2)):
        rc, h = create(**kw)
        assert rc == 0 and h.value
        assert lib.hymet_sketch_stream_destroy(h) == 0
    assert lib.hymet_sketch_stream_destroy(None) == 0

    pool = DevicePool(gpu, _batches(rr.read_set()[:20], None)[0], DevicePool.ALPHA_MASH)
    rc, h = create()
    assert rc == 0
    try:
        n = ctypes.c_int32()
        more = ctypes.c_int32()
        out = gpu.zeros(1000, gpu.torch.int64)
        out_c = gpu.zeros(1000, gpu.torch.int32)
        rejected("hymet_sketch_stream_add", lib.hymet_sketch_stream_add(h, ptr(pool.w2b), ptr(pool.wmask), pool.n_bases, 0))
        rejected("hymet_sketch_stream_add", lib.hymet_sketch_stream_add(h, ptr(pool.w2b), ptr(pool.wmask), pool.n_bases, -5))
        rejected("hymet_sketch_stream_add", lib.hymet_sketch_stream_add(h, ptr(pool.w2b), ptr(pool.wmask), -1, 1000))
        rejected("hymet_sketch_stream_add", lib.hymet_sketch_stream_add(h, None, None, pool.n_bases, 1000))
        rejected("hymet_sketch_stream_add", lib.hymet_sketch_stream_add(None, ptr(pool.w2b), ptr(pool.wmask), pool.n_bases, 1000))
        rejected("hymet_sketch_stream_result", lib.hymet_sketch_stream_result(h, ptr(out), ptr(out_c), ctypes.byref(n), None))
        rejected("hymet_sketch_stream_end_pass", lib.hymet_sketch_stream_end_pass(h, None))
        assert lib.hymet_sketch_stream_add(h, ptr(pool.w2b), ptr(pool.wmask), pool.n_bases, 1000) == 0
        assert lib.hymet_sketch_stream_add(h, ptr(pool.w2b), ptr(pool.wmask), 20, 1000) == 0     # shorter than k: nothing
        assert lib.hymet_sketch_stream_end_pass(h, ctypes.byref(more)) == 0 and more.value == 0
        # finished: no more input
        rejected("hymet_sketch_stream_add", lib.hymet_sketch_stream_add(h, ptr(pool.w2b), ptr(pool.wmask), pool.n_bases, 1000))
        assert lib.hymet_sketch_stream_end_pass(h, ctypes.byref(more)) == 0 and more.value == 0
        rejected("hymet_sketch_stream_result", lib.hymet_sketch_stream_result(h, None, None, ctypes.byref(n), None))
        assert lib.hymet_sketch_stream_result(h, ptr(out), ptr(out_c), ctypes.byref(n), None) == 0
        want = rr.counted_ref(rr.read_set()[:20], 21, 42, 1000, 2)
        assert n.value == len(want[0]) > 0
        np.testing.assert_array_equal(out.cpu().numpy().view(np.uint64)[:n.value], want[0])
    finally:
        assert lib.hymet_sketch_stream_destroy(h) == 0
    with pytest.raises(Exception, match="hymet_sketch_stream_create"):
        sk.sketch_stream(gpu, [], 21, 42, smax + 1, 2)
    gpu.sync()


def _fasta(recs, width=70):
    out = []
    for name, comment, seq in recs:
        out.append(b">" + (name + (" " + comment if comment else "")).encode() + b"\n")
        out.extend(seq[i:i + width] + b"\n" for i in range(0, len(seq), width))
    return b"".join(out)


def test_sketch_files_streams_large_read_files(gpu, tmp_path):
    from hymet_amd import sketch as sk
    reads = list(rr.read_set())
    k, seed, s = 21, 42, 1000
    small = rr.write_fastq(tmp_path / "small.fastq", reads[:20], prefix="s")
    none = rr.write_fastq(tmp_path / "none.fastq", [b"ACGT"] * 2_000)        # 8,000 bases, no k-mer
    for name in ("reads.fastq", "reads.fastq.gz"):
        big = rr.write_fastq(tmp_path / name, reads)
        paths = [small, big, none, small]
        info_a, info_b = [], []
        sk.sketch_stream.stats = {}
        a = sk.sketch_files(gpu, paths, k=k, seed=seed, s=s, reads=True, min_copies=2, read_info=info_a)
        assert sk.sketch_stream.stats == {}                                  # nothing streamed at the default
        b = sk.sketch_files(gpu, paths, k=k, seed=seed, s=s, reads=True, min_copies=2, read_info=info_b,
                            batch_bases=5_000)
        st = sk.sketch_stream.stats                                          # the last streamed file: `none`
        assert st["passes"] == 1 and st["slices"] == 2 and st["emitted"] == 0
        assert list(a.names) == list(b.names) == [small, big, small]
        assert list(a.comments) == list(b.comments) and a.comments[1] == "[320 seqs] read0 [...]"
        np.testing.assert_array_equal(a.lengths, b.lengths)
        np.testing.assert_array_equal(a.offsets, b.offsets)
        np.testing.assert_array_equal(a.hashes, b.hashes)
        assert info_a == info_b and len(info_a) == 3
        np.testing.assert_array_equal(b.ref_hashes(1), rr.counted_ref(reads, k, seed, s, 2)[0])
    # file mode reads the file whole, whatever batch_bases says about grouping
    fa = tmp_path / "g.fna"
    fa.write_bytes(_fasta([("chr", "", rr.genome())]))
    x = sk.sketch_files(gpu, [str(fa)], batch_bases=1_000)
    y = sk.sketch_files(gpu, [str(fa)])
    np.testing.assert_array_equal(x.hashes, y.hashes)


def test_cli_batch_bases(gpu, tmp_path, capsys):
    from hymet_amd import cli
    from hymet_amd import sketch as sk
    reads = list(rr.read_set())
    fq_gz = rr.write_fastq(tmp_path / "reads.fastq.gz", reads)
    small = rr.write_fastq(tmp_path / "small.fastq", reads[:20], prefix="s")
    assert cli.main(["sketch", "-r", "-m", "2", "-o", str(tmp_path / "whole"), fq_gz, small]) == 0
    err_whole = capsys.readouterr().err
    sk.sketch_stream.stats = {}
    assert cli.main(["sketch", "-r", "-m", "2", "--batch-bases", "5k", "-o", str(tmp_path / "batched"), fq_gz, small]) == 0
    err_batched = capsys.readouterr().err
    assert sk.sketch_stream.stats["slices"] == 10 and sk.sketch_stream.stats["passes"] == 1
    assert (tmp_path / "whole.msh").read_bytes() == (tmp_path / "batched.msh").read_bytes()
    assert err_whole.replace("whole.msh", "batched.msh") == err_batched and "estimated coverage" in err_batched

    rng = np.random.default_rng(8)
    paths = []
    for name, seq in (("ref_a.fna", rr.genome()), ("ref_b.fna", rand_seq(rng, 6_000))):
        (tmp_path / name).write_bytes(_fasta([(name, "", seq)]))
        paths.append(str(tmp_path / name))
    assert cli.main(["sketch", "-o", str(tmp_path / "REF")] + paths) == 0
    capsys.readouterr()
    ref_msh = str(tmp_path / "REF.msh")
    assert cli.main(["dist", "-r", "-m", "2", ref_msh, fq_gz, small]) == 0
    whole = capsys.readouterr().out
    sk.sketch_stream.stats = {}
    assert cli.main(["dist", "-r", "-m", "2", "--batch-bases", "5k", ref_msh, fq_gz, small]) == 0
    assert capsys.readouterr().out == whole
    assert sk.sketch_stream.stats["slices"] == 10
    assert len(whole.splitlines()) == 4
    assert int(whole.splitlines()[0].split("\t")[4].split("/")[0]) > 0
