"""GPU read-set sketch (csrc/sketch_counted.hip through hymet_amd.sketch and the CLI) against the
plain-Python restatement tests/_reads_ref.py: hashes and multiplicities, exact equality."""
import ctypes
import gzip
from functools import lru_cache

import numpy as np
import pytest

from tests import _reads_ref as rr
from tests._data import add_noise, rand_seq, revcomp

pytestmark = pytest.mark.gpu

E_ARG = -2
CHUNK = 4099      # the large groups get many chunks and a merge, the small ones a single chunk


@pytest.fixture(scope="module")
def gpu():
    from hymet_amd._lib import Gpu
    return Gpu(0)


@lru_cache(maxsize=None)
def _groups():
    reads = list(rr.read_set())
    rng = np.random.default_rng(99)
    return (
        reads,                                                   # 12 chunks at CHUNK
        [revcomp(r) for r in reads],                             # the same k-mers: an equal row
        reads[:20],                                              # fewer than s qualifiers
        [reads[0]] * 3 + reads[40:50],                           # one read three times, ten once
        [b"ACGTACGT", b"TTGACA", b"GGGGGGGG"],                   # all shorter than k: an empty row
        [b""],                                                   # an empty record
        [add_noise(rng, r) for r in reads[100:160]],             # N runs, IUPAC codes, lower case
    )


_POOL = {}


def _pool(gpu, which=None):
    """The parity pool (which=None) or a pool of one of its groups, packed once."""
    from hymet_amd.seqio import DevicePool, from_records
    if which not in _POOL:
        groups = _groups() if which is None else (_groups()[which],)
        recs = [(f"g{g}_r{j}", "", s) for g, seqs in enumerate(groups) for j, s in enumerate(seqs)]
        group_of = np.array([g for g, seqs in enumerate(groups) for _ in seqs], np.int64)
        _POOL[which] = (DevicePool(gpu, from_records(recs), DevicePool.ALPHA_MASH), group_of)
    return _POOL[which]


@lru_cache(maxsize=None)
def _counter(g, k, seed):
    # group 1 holds group 0's k-mers on the other strand: the same canonical k-mers, the same Counter
    return rr.hash_counter(_groups()[0 if g == 1 else g], k, seed)


def _want(g, k, seed, s, m):
    cnt = _counter(g, k, seed)
    keep = sorted(h for h, c in cnt.items() if c >= m)[:s]
    return np.array(keep, np.uint64), np.array([cnt[h] for h in keep], np.uint32)


def _check(got, k, seed, s, m, groups=None):
    groups = range(len(_groups())) if groups is None else groups
    assert len(got) == len(groups)
    for (h, c), g in zip(got, groups):
        wh, wc = _want(g, k, seed, s, m)
        assert h.dtype == np.uint64 and c.dtype == np.uint32
        assert len(h) == len(wh) == len(c), (g, len(h), len(wh))
        np.testing.assert_array_equal(h, wh, err_msg=f"hashes of group {g}")
        np.testing.assert_array_equal(c, wc, err_msg=f"counts of group {g}")


@pytest.mark.parametrize("k,seed,s,m", [(21, 42, 1000, 2), (21, 42, 1000, 3), (16, 42, 1000, 2), (32, 7, 200, 2),
                                        (9, 42, 200, 2), (21, 42, 1, 2), (21, 42, 1000, 1)])
def test_parity_with_the_restatement(gpu, k, seed, s, m):
    from hymet_amd import sketch as sk
    pool, group_of = _pool(gpu)
    got = sk.sketch_pool_counted(gpu, pool, group_of, k, seed, s, m, chunk_bases=CHUNK)
    _check(got, k, seed, s, m)
    np.testing.assert_array_equal(got[0][0], got[1][0])
    np.testing.assert_array_equal(got[0][1], got[1][1])
    assert len(got[4][0]) == 0 and len(got[5][0]) == 0
    assert sk.sketch_pool_counted.stats["passes"] >= 1
    if (k, s, m) == (21, 1000, 2):
        assert len(got[0][0]) == 1000 and 0 < len(got[2][0]) < 1000
        h3, c3 = got[3]                                   # the tripled read's k-mers and the singles' overlaps
        assert len(h3) >= 130 and c3.min() >= 2 and c3.max() >= 3
        assert sk.sketch_pool_counted.stats["merged"] > 0


def test_one_copy_equals_sketch_pool(gpu):
    from hymet_amd import sketch as sk
    pool, group_of = _pool(gpu)
    for k, s in ((21, 1000), (16, 300)):
        plain = sk.sketch_pool(gpu, pool, group_of, k=k, seed=42, s=s, chunk_bases=CHUNK)
        got = sk.sketch_pool_counted(gpu, pool, group_of, k, 42, s, 1, chunk_bases=CHUNK)
        assert len(plain) == len(got)
        for a, (h, c) in zip(plain, got):
            np.testing.assert_array_equal(a, h)
            assert len(c) == len(h) and (len(c) == 0 or c.min() >= 1)


def test_chunking_independence(gpu):
    from hymet_amd import sketch as sk
    pool, group_of = _pool(gpu)
    runs = [sk.sketch_pool_counted(gpu, pool, group_of, 21, 42, 1000, 2, chunk_bases=cb) for cb in (1000, CHUNK, 1 << 40)]
    assert sk.sketch_pool_counted.stats["merged"] == 0          # one chunk per sketch: no merge
    for other in runs[1:]:
        for (h0, c0), (h1, c1) in zip(runs[0], other):
            np.testing.assert_array_equal(h0, h1)
            np.testing.assert_array_equal(c0, c1)
    assert len(runs[0][0][0]) == 1000


def test_several_passes(gpu):
    """64 slots per chunk: the rows take many passes and stay the same.  At 8x nearly every kept
    hash has copies before and after the set fills, so a cut test that drops the cut hash's own
    later copies shows as a wrong count."""
    from hymet_amd import sketch as sk
    lib = gpu.lib
    pool, group_of = _pool(gpu)
    assert lib.hymet_sketch_counted_tune(64) == 0
    try:
        for cb in (CHUNK, 1 << 40):                       # merged chunks; the single-chunk path
            got = sk.sketch_pool_counted(gpu, pool, group_of, 21, 42, 1000, 2, chunk_bases=cb)
            assert sk.sketch_pool_counted.stats["passes"] > 1
            _check(got, 21, 42, 1000, 2)
        got = sk.sketch_pool_counted(gpu, pool, group_of, 16, 42, 300, 3, chunk_bases=CHUNK)
        assert sk.sketch_pool_counted.stats["passes"] > 1
        _check(got, 16, 42, 300, 3)
        # nothing qualifies: the whole group is walked through, 64 distinct hashes per pass
        small, small_of = _pool(gpu, 2)
        got = sk.sketch_pool_counted(gpu, small, small_of, 21, 42, 1000, 50, chunk_bases=CHUNK)
        assert len(got) == 1 and len(got[0][0]) == 0 and len(got[0][1]) == 0
        distinct = len(_counter(2, 21, 42))
        assert 1 < sk.sketch_pool_counted.stats["passes"] <= -(-distinct // 64) + 1
    finally:
        assert lib.hymet_sketch_counted_tune(0) == 0


def test_refusals(gpu):
    """Bad parameters and plans fail in the host checks with a message; nothing is launched."""
    from hymet_amd import sketch as sk
    from hymet_amd._lib import ptr
    torch = gpu.torch
    pool, _ = _pool(gpu)
    lib, n_bases, k = gpu.lib, pool.n_bases, 21
    smax = sk.max_counted_sketch_size()
    assert 1000 <= smax < sk.max_sketch_size()
    assert smax == (160 * 1024 - 64) // 12 - 2048
    out = gpu.zeros(2 * smax, torch.int64)
    out_c = gpu.zeros(2 * smax, torch.int32)
    out_n = gpu.zeros(2, torch.int32)
    stats = (ctypes.c_int64 * 2)()

    def call(k=k, s=1000, m=2, sketch=(0, 1), begin=(0, 5000), end=(5000, 9000), n_sketches=2):
        cs = np.array(sketch, np.int32)
        cb = np.array(begin, np.int64)
        ce = np.array(end, np.int64)
        return lib.hymet_sketch_counted(gpu.ctx, ptr(pool.w2b), ptr(pool.wmask), n_bases, k, 42, s, m, len(cs),
                                        cs.ctypes.data_as(ctypes.c_void_p), cb.ctypes.data_as(ctypes.c_void_p),
                                        ce.ctypes.data_as(ctypes.c_void_p), n_sketches, ptr(out), ptr(out_c), ptr(out_n),
                                        ctypes.cast(stats, ctypes.c_void_p))

    def rejected(**kw):
        assert call(**kw) == E_ARG
        msg = lib.hymet_last_error()
        assert msg and b"hymet_sketch_counted" in msg

    assert call() == 0 and stats[0] >= 1
    assert call(n_sketches=0, sketch=(), begin=(), end=()) == 0
    rejected(s=smax + 1)
    rejected(s=0)
    rejected(m=0)
    rejected(m=-3)
    rejected(begin=(0, 4000))                             # overlap
    rejected(sketch=(1, 0))                               # unsorted sketch ids
    rejected(end=(5000, n_bases - k + 2))                 # past the pool's last k-mer start
    rejected(k=33)
    assert lib.hymet_sketch_counted_tune(smax + 1) == E_ARG
    assert lib.hymet_sketch_counted_tune(-1) == E_ARG
    assert lib.hymet_sketch_counted_tune(0) == 0
    gpu.sync()


def _fasta(recs, width=70):
    out = []
    for name, comment, seq in recs:
        out.append(b">" + (name + (" " + comment if comment else "")).encode() + b"\n")
        out.extend(seq[i:i + width] + b"\n" for i in range(0, len(seq), width))
    return b"".join(out)


def test_cli_end_to_end(gpu, tmp_path, capsys):
    from hymet_amd import cli
    from hymet_amd.msh import load_db
    from hymet_amd.sketch import read_set_length
    reads = list(rr.read_set())
    k, seed, s = 21, 42, 1000
    fq_gz = rr.write_fastq(tmp_path / "reads.fastq.gz", reads)
    fq = rr.write_fastq(tmp_path / "reads.fastq", reads)
    want, _ = rr.counted_ref(reads, k, seed, s, 2)

    # sketch -r -m 2: the hashes, the length by the rule, -g
    assert cli.main(["sketch", "-r", "-m", "2", "-o", str(tmp_path / "X"), fq_gz]) == 0
    err = capsys.readouterr().err
    assert "estimated genome size" in err and "estimated coverage" in err
    db = load_db(str(tmp_path / "X.msh"))
    assert (db.n_refs, db.k, db.seed, db.sketch_size) == (1, k, seed, s)
    np.testing.assert_array_equal(db.ref_hashes(0), want)
    assert list(db.names) == [fq_gz] and db.comments[0] == "[320 seqs] read0 [...]"
    assert int(db.lengths[0]) == read_set_length(want, s, k)
    assert 3_000 < int(db.lengths[0]) < 12_000           # the genome has 6,000 bases
    assert cli.main(["sketch", "-m", "2", "-g", "6000", "-o", str(tmp_path / "G.msh"), fq_gz]) == 0
    dbg = load_db(str(tmp_path / "G.msh"))
    np.testing.assert_array_equal(dbg.ref_hashes(0), want)
    assert int(dbg.lengths[0]) == 6000
    capsys.readouterr()

    # dist -r -m 2 over the reads == dist over the sketch made of them
    rng = np.random.default_rng(8)
    refs = [("ref_a.fna", [("chrA", "", rr.genome())]), ("ref_b.fna", [("chrB", "", rand_seq(rng, 6_000))]),
            ("ref_c.fna", [("chrC", "", rr.genome()[:3_000] + rand_seq(rng, 3_000))])]
    paths = []
    for name, recs in refs:
        (tmp_path / name).write_bytes(_fasta(recs))
        paths.append(str(tmp_path / name))
    assert cli.main(["sketch", "-o", str(tmp_path / "REF")] + paths) == 0
    capsys.readouterr()
    ref_msh = str(tmp_path / "REF.msh")
    assert cli.main(["dist", ref_msh, str(tmp_path / "X.msh")]) == 0
    from_sketch = capsys.readouterr().out
    assert len(from_sketch.splitlines()) == 3
    assert cli.main(["dist", "-r", "-m", "2", ref_msh, fq_gz]) == 0
    assert capsys.readouterr().out == from_sketch
    assert cli.main(["dist", "-r", "-m", "2", ref_msh, fq]) == 0
    assert capsys.readouterr().out == from_sketch.replace(fq_gz, fq)
    shared = [int(l.split("\t")[4].split("/")[0]) for l in from_sketch.splitlines()]
    assert shared[0] > shared[2] > shared[1] == 0        # the genome, its half, a stranger
    assert cli.main(["dist", "-m", "2", ref_msh, str(tmp_path / "X.msh")]) == 2
    capsys.readouterr()

    # mash-screen reads FASTQ: the same rows as the same sequences given as FASTA
    fa = tmp_path / "reads.fna"
    fa.write_bytes(_fasta([(f"read{i}", "", r) for i, r in enumerate(reads)], width=60))
    assert cli.main(["mash-screen", ref_msh, str(fa)]) == 0
    from_fasta = capsys.readouterr().out
    assert cli.main(["mash-screen", ref_msh, fq]) == 0
    assert capsys.readouterr().out == from_fasta
    assert len(from_fasta.splitlines()) >= 2
    with gzip.open(fq_gz, "rb") as f:                     # and the gzip is what the plain file is
        assert f.read() == open(fq, "rb").read()
