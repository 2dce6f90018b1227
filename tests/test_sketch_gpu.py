"""GPU sketch (csrc/sketch.hip through hymet_amd.sketch and `cli sketch`) vs the CPU oracle
(oracle/mash_oracle.c oracle_sketch): exact equality of every reference's bottom-s set."""
import ctypes
import gzip

import numpy as np
import pytest

from tests._data import add_noise, rand_seq, revcomp

pytestmark = pytest.mark.gpu

E_ARG = -2


@pytest.fixture(scope="module")
def gpu():
    from hymet_amd._lib import Gpu
    return Gpu(0)


def _groups(with_300k: bool):
    """The parity pool: (records, group_of, sequences per group).  Seeded, built once per shape."""
    rng = np.random.default_rng(2024)
    genome = rand_seq(rng, 60_000)
    unit = rand_seq(rng, 200)
    mid = bytearray(rand_seq(rng, 2_500))
    mid[1200:1205] = b"NNNNN"
    groups = [
        [genome],                                                  # many chunks and a merge
        [revcomp(genome)],                                         # same sketch as group 0
        [rand_seq(rng, 3_000), b"ACGTACGT", rand_seq(rng, 2_000).lower(), bytes(mid), rand_seq(rng, 1_500)],
        [rand_seq(rng, 300)],                                      # fewer than s distinct hashes
        [unit * 500],                                              # duplicate-heavy, never fills
        [b"ACGTACGT"],                                             # only record shorter than k: empty row
        [b""],                                                     # an empty record
        [add_noise(rng, rand_seq(rng, 20_000, gc=0.35))],          # N runs, IUPAC codes, a lower-case stretch
    ]
    if with_300k:
        groups.append([rand_seq(rng, 300_000)])                    # k = 9: nearly every hash a duplicate
    recs, group_of = [], []
    for g, seqs in enumerate(groups):
        for j, s in enumerate(seqs):
            recs.append((f"g{g}_r{j}", "", s))
            group_of.append(g)
    return recs, np.array(group_of, np.int64), groups


_POOLS = {}


def _pool(gpu, with_300k=False):
    from hymet_amd.seqio import DevicePool, from_records
    if with_300k not in _POOLS:
        recs, group_of, groups = _groups(with_300k)
        _POOLS[with_300k] = (DevicePool(gpu, from_records(recs), DevicePool.ALPHA_MASH), group_of, groups)
    return _POOLS[with_300k]


@pytest.mark.parametrize("k,seed,s", [(21, 42, 1000), (17, 7, 500), (32, 42, 200), (16, 42, 1000), (13, 7, 400),
                                      (9, 42, 200), (21, 42, 1), (21, 42, 10000)])
def test_sketch_matches_oracle(gpu, k, seed, s):
    from hymet_amd import sketch as sk
    from oracle import oracle_lib
    pool, group_of, groups = _pool(gpu, with_300k=(k == 9))
    got = sk.sketch_pool(gpu, pool, group_of, k=k, seed=seed, s=s, chunk_bases=4099)
    assert len(got) == len(groups)
    for g, seqs in enumerate(groups):
        want = oracle_lib.sketch(seqs, k, seed, s)
        assert got[g].dtype == np.uint64
        assert len(got[g]) == len(want), (g, len(got[g]), len(want))
        np.testing.assert_array_equal(got[g], want, err_msg=f"group {g}")
    np.testing.assert_array_equal(got[0], got[1])     # a genome and its reverse complement
    assert len(got[5]) == 0 and len(got[6]) == 0
    if (k, s) == (21, 1000):                            # the shapes the oracle was checked on
        assert [len(got[g]) for g in (0, 3, 4)] == [1000, 280, 200]
    if (k, s) == (9, 200):
        assert len(got[8]) == 200


def test_sketch_does_not_depend_on_chunking(gpu):
    from hymet_amd import sketch as sk
    pool, group_of, groups = _pool(gpu)
    runs = [sk.sketch_pool(gpu, pool, group_of, k=21, seed=42, s=1000, chunk_bases=cb) for cb in (1000, 4099, 1 << 40)]
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            np.testing.assert_array_equal(a, b)
    assert len(runs[0][0]) == 1000


def test_one_sketch_per_record_equals_sketch_sequences(gpu):
    from hymet_amd import screen as scr
    from hymet_amd import sketch as sk
    pool, _, _ = _pool(gpu)
    got = sk.sketch_pool(gpu, pool, None, k=21, seed=42, s=1000)
    want = scr.sketch_sequences(gpu, pool, k=21, seed=42, s=1000)
    assert len(got) == len(want) == pool.ss.n
    for a, b in zip(got, want):
        np.testing.assert_array_equal(a, b)


def test_preserve_case(gpu):
    from hymet_amd import sketch as sk
    from hymet_amd.seqio import DevicePool, from_records
    from oracle import oracle_lib
    rng = np.random.default_rng(77)
    a = bytearray(rand_seq(rng, 12_000))
    for st in (100, 4_000, 4_030, 11_950):
        a[st:st + 25] = bytes(a[st:st + 25]).lower()
    seq = bytes(a)
    masked = bytes(ord("N") if 97 <= c <= 122 else c for c in seq)
    pool = DevicePool(gpu, from_records([("s", "", seq)]), DevicePool.ALPHA_MASH_PRESERVE_CASE)
    got = sk.sketch_pool(gpu, pool, None, k=21, seed=42, s=1000, chunk_bases=4099)[0]
    np.testing.assert_array_equal(got, oracle_lib.sketch([masked], 21, 42, 1000))
    # and without -Z the lower-case bases count
    pool = DevicePool(gpu, from_records([("s", "", seq)]), DevicePool.ALPHA_MASH)
    got = sk.sketch_pool(gpu, pool, None, k=21, seed=42, s=1000, chunk_bases=4099)[0]
    np.testing.assert_array_equal(got, oracle_lib.sketch([seq], 21, 42, 1000))


def _fasta(recs, width=70):
    out = []
    for name, comment, seq in recs:
        out.append(b">" + (name + (" " + comment if comment else "")).encode() + b"\n")
        out.extend(seq[i:i + width] + b"\n" for i in range(0, len(seq), width))
    return b"".join(out)


def test_cli_sketch_end_to_end(gpu, tmp_path):
    from hymet_amd import cli
    from hymet_amd import screen as scr
    from hymet_amd.msh import read_msh
    from hymet_amd.seqio import DevicePool, from_records
    from oracle import oracle_lib
    rng = np.random.default_rng(31)
    k, seed, s = 21, 42, 400
    files = [
        ("a.fna.gz", [("chrA", "Genus one strain A", rand_seq(rng, 30_000))]),
        ("b.fna", [("ctg1", "draft assembly", rand_seq(rng, 12_000)), ("tiny", "", b"ACGTACGTACGT"),
                   ("ctg2", "plasmid", rand_seq(rng, 5_000))]),
        ("c.fna", [("chrC", "", rand_seq(rng, 20_000))]),
    ]
    paths = []
    for name, recs in files:
        p = tmp_path / name
        data = _fasta(recs)
        if name.endswith(".gz"):
            with gzip.open(p, "wb") as f:
                f.write(data)
        else:
            p.write_bytes(data)
        paths.append(str(p))
    assert cli.main(["sketch", "-k", str(k), "-s", str(s), "-o", str(tmp_path / "db")] + paths) == 0
    db = read_msh(tmp_path / "db.msh")
    assert (db.k, db.seed, db.sketch_size, db.preserve_case, db.noncanonical, db.alphabet) == (k, seed, s, False, False, "ACGT")
    assert list(db.names) == paths
    assert list(db.comments) == ["chrA Genus one strain A", "[2 seqs] ctg1 draft assembly [...]", "chrC"]
    assert db.lengths.tolist() == [30_000, 17_000, 20_000]
    want = [oracle_lib.sketch([r[2] for r in recs], k, seed, s) for _, recs in files]
    for i, w in enumerate(want):
        np.testing.assert_array_equal(db.ref_hashes(i), w)
    # the DB screens: a pool of b.fna's own records holds every hash of reference 2
    recs = files[1][1]
    pool = DevicePool(gpu, from_records(recs), DevicePool.ALPHA_MASH)
    res = scr.screen(gpu, pool, [db])[0]
    assert res.shared[1] == len(want[1]) == s
    sh, md, set_size, nk = oracle_lib.screen([r[2] for r in recs], k, seed, s, want)
    np.testing.assert_array_equal(res.shared, sh)
    np.testing.assert_array_equal(res.median, md)
    assert res.set_size == set_size and res.n_kmers == nk
    line2 = [l for l in res.lines() if l.split("\t")[4] == paths[1]]
    assert len(line2) == 1 and line2[0].split("\t")[0] == "1"       # identity 1


def test_batch_argument_errors(gpu):
    """Bad plans and parameters fail in the host checks with a message; nothing is launched."""
    from hymet_amd import sketch as sk
    from hymet_amd._lib import ptr
    torch = gpu.torch
    pool, _, _ = _pool(gpu)
    lib, n_bases, k = gpu.lib, pool.n_bases, 21
    smax = sk.max_sketch_size()
    assert smax >= 10_000
    out = gpu.zeros(2 * smax + 2, torch.int64)
    out_n = gpu.zeros(2, torch.int32)

    def call(k=k, s=1000, sketch=(0, 1), begin=(0, 5000), end=(5000, 9000), n_sketches=2, n_chunks=None):
        cs = np.array(sketch, np.int32)
        cb = np.array(begin, np.int64)
        ce = np.array(end, np.int64)
        return lib.hymet_sketch_batch(gpu.ctx, ptr(pool.w2b), ptr(pool.wmask), n_bases, k, 42, s,
                                      len(cs) if n_chunks is None else n_chunks, cs.ctypes.data_as(ctypes.c_void_p),
                                      cb.ctypes.data_as(ctypes.c_void_p), ce.ctypes.data_as(ctypes.c_void_p), n_sketches,
                                      ptr(out), ptr(out_n))

    def rejected(**kw):
        assert call(**kw) == E_ARG
        msg = lib.hymet_last_error()
        assert msg and b"hymet_sketch_batch" in msg

    assert call() == 0
    assert call(n_chunks=0) == 0
    assert call(n_sketches=0, sketch=(), begin=(), end=()) == 0
    rejected(end=(5000, n_bases - k + 2))                 # past the pool's last k-mer start
    rejected(begin=(-1, 5000))
    rejected(begin=(6000, 5000), end=(5000, 9000))        # begin > end
    rejected(sketch=(1, 0))                               # unsorted sketch ids
    rejected(sketch=(0, 2))                               # id >= n_sketches
    rejected(begin=(0, 4000))                             # overlap
    rejected(s=0)
    rejected(s=smax + 1)
    rejected(k=33)
    rejected(k=0)
    gpu.sync()
