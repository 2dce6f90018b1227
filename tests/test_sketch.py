"""Host side of the sketch stage (hymet_amd/sketch.py, `cli sketch`): the chunk plan, the
references' metadata and the command line.  No device: the CLI tests stub the device call."""
import gzip

import numpy as np
import pytest

from hymet_amd import cli
from hymet_amd import sketch as sk
from hymet_amd.seqio import from_records


def _plan(lens, groups, k, chunk):
    ss = from_records([(f"r{i}", "", b"A" * L) for i, L in enumerate(lens)])
    cs, cb, ce = sk.plan_chunks(ss.starts, ss.lengths, groups, k, chunk)
    assert cs.dtype == np.int32 and cb.dtype == np.int64 and ce.dtype == np.int64
    return ss, cs.tolist(), cb.tolist(), ce.tolist()


def test_plan_two_groups_known_answer():
    # pool: r0 at 0 (12 bases), r1 at 13 (3 < k), r2 at 17 (9), r3 at 27 (20); k = 5
    # group 0 spans starts [0, 17 + 9 - 4) = [0, 22): ceil(22 / 7) = 4 chunks of ceil(22 / 4) = 6
    # group 1 spans [27, 27 + 20 - 4) = [27, 43): ceil(16 / 7) = 3 chunks of ceil(16 / 3) = 6
    ss, cs, cb, ce = _plan([12, 3, 9, 20], [0, 0, 0, 1], 5, 7)
    assert ss.starts.tolist() == [0, 13, 17, 27]
    assert cs == [0, 0, 0, 0, 1, 1, 1]
    assert cb == [0, 6, 12, 18, 27, 33, 39]
    assert ce == [6, 12, 18, 22, 33, 39, 43]


def test_plan_record_of_exactly_k_bases():
    _, cs, cb, ce = _plan([5], [0], 5, 7)
    assert (cs, cb, ce) == ([0], [0], [1])


def test_plan_short_record_between_long_ones():
    # r0 at 0 (10), r1 at 11 (4 < k), r2 at 16 (10): one group, one chunk over [0, 16 + 10 - 4)
    _, cs, cb, ce = _plan([10, 4, 10], [0, 0, 0], 5, 100)
    assert (cs, cb, ce) == ([0], [0], [22])
    # the short record alone in the middle group: that group gets no chunk
    _, cs, cb, ce = _plan([10, 4, 10], [0, 1, 2], 5, 100)
    assert (cs, cb, ce) == ([0, 2], [0, 16], [6, 22])


def test_plan_empty_group_and_empty_input():
    # group 1 has no record at all, group 2 only an empty record
    _, cs, cb, ce = _plan([8, 0, 8], [0, 2, 3], 5, 100)
    assert (cs, cb, ce) == ([0, 3], [0, 10], [4, 14])
    cs, cb, ce = sk.plan_chunks([], [], [], 5, 7)
    assert len(cs) == len(cb) == len(ce) == 0


def test_plan_sorted_by_sketch_id_when_groups_are_not_in_pool_order():
    _, cs, cb, ce = _plan([10, 10, 10], [2, 0, 1], 5, 100)
    assert (cs, cb, ce) == ([0, 1, 2], [11, 22, 0], [17, 28, 6])


def test_plan_rejects_scattered_group():
    with pytest.raises(ValueError):
        _plan([10, 10, 10], [0, 1, 0], 5, 100)


@pytest.mark.parametrize("seed", range(6))
def test_plan_covers_every_kmer_start_once(seed):
    rng = np.random.default_rng(seed)
    k = int(rng.integers(1, 33))
    n = int(rng.integers(1, 60))
    lens = np.where(rng.random(n) < 0.3, rng.integers(0, k + 2, n), rng.integers(k, 400, n))
    groups = np.cumsum(rng.random(n) < 0.4)               # contiguous, non-decreasing
    groups = rng.permutation(groups.max() + 1)[groups]    # ... under arbitrary ids
    chunk = int(rng.integers(1, 300))
    ss, cs, cb, ce = _plan(lens.tolist(), groups, k, chunk)
    n_pos = len(ss.buf)
    hit = np.zeros(n_pos + 1, np.int64)
    owner = np.full(n_pos + 1, -1, np.int64)
    assert cs == sorted(cs)
    for g, b, e in zip(cs, cb, ce):
        assert 0 <= b < e <= n_pos - k + 1
        assert e - b <= chunk
        hit[b:e] += 1
        owner[b:e] = g
    assert hit.max() <= 1                                  # no overlap anywhere
    for i in range(n):
        L, st = int(ss.lengths[i]), int(ss.starts[i])
        if L >= k:                                         # every valid start once, in its own group
            assert (hit[st:st + L - k + 1] == 1).all()
            assert (owner[st:st + L - k + 1] == groups[i]).all()
    # a chunk never reaches a valid start of another group: checked above through owner


def test_file_meta_strings():
    names, comments = ["chr1", "p1", "tiny"], ["Escherichia coli K-12", "", "x"]
    assert sk.file_meta("g/a.fna", names[:1], comments[:1], [5000], 21) == ("g/a.fna", "chr1 Escherichia coli K-12", 5000)
    assert sk.file_meta("g/a.fna", names[1:2], comments[1:2], [30], 21) == ("g/a.fna", "p1", 30)
    # two usable records and a short one: N counts the usable ones, so does the length
    assert sk.file_meta("a.fna", names, comments, [5000, 300, 20], 21) == \
        ("a.fna", "[2 seqs] chr1 Escherichia coli K-12 [...]", 5300)
    # the first USABLE record heads the comment
    assert sk.file_meta("a.fna", ["tiny", "chr1", "p1"], ["x", "c", ""], [3, 50, 60], 21) == \
        ("a.fna", "[2 seqs] chr1 c [...]", 110)
    assert sk.file_meta("a.fna", ["tiny"], ["x"], [20], 21) is None
    assert sk.file_meta("a.fna", [], [], [], 21) is None


# ------------------------------------------------------------------ command line
def test_sketch_args_defaults_and_flags():
    a = cli.sketch_args(["-o", "db", "a.fna", "b.fna"])
    assert (a.k, a.s, a.seed, a.individual, a.preserve_case, a.lists) == (21, 1000, 42, False, False, False)
    assert a.out == "db" and a.files == ["a.fna", "b.fna"]
    a = cli.sketch_args(["-k", "16", "-s", "400", "-S", "7", "-i", "-Z", "-l", "-o", "x", "list.txt"])
    assert (a.k, a.s, a.seed, a.individual, a.preserve_case, a.lists) == (16, 400, 7, True, True, True)


@pytest.mark.parametrize("argv", [["-n", "-o", "x", "a.fna"], ["-q", "-o", "x", "a.fna"], ["-o", "x"], ["a.fna"],
                                  ["-k", "abc", "-o", "x", "a.fna"]])
def test_sketch_bad_arguments_exit_2_with_usage(argv, capsys):
    assert cli.main(["sketch"] + argv) == 2
    assert "usage: sketch" in capsys.readouterr().err


class _StubGpu:
    def __init__(self, device=0):
        self.device = device


@pytest.fixture
def stub(monkeypatch):
    """The device side of `cli sketch` replaced: records the call, returns a two-reference DB."""
    from hymet_amd import _lib
    from hymet_amd.msh import SketchDB
    calls = []

    def fake_sketch_files(gpu, paths, k=21, seed=42, s=1000, individual=False, preserve_case=False, **kw):
        calls.append(dict(gpu=gpu, paths=list(paths), k=k, seed=seed, s=s, individual=individual,
                          preserve_case=preserve_case))
        return SketchDB(k=k, seed=seed, sketch_size=s, preserve_case=preserve_case, names=[str(p) for p in paths],
                        comments=["c"] * len(paths), lengths=np.full(len(paths), 100, np.int64),
                        offsets=np.arange(len(paths) + 1, dtype=np.int64) * 2,
                        hashes=np.arange(2 * len(paths), dtype=np.uint64) + 5)

    monkeypatch.setattr(_lib, "Gpu", _StubGpu)
    monkeypatch.setattr(sk, "sketch_files", fake_sketch_files)
    return calls


@pytest.mark.parametrize("prefix", ["x", "x.msh"])
def test_sketch_writes_prefix_msh(stub, tmp_path, monkeypatch, prefix):
    from hymet_amd.msh import read_msh_py
    monkeypatch.setenv("HYMET_DEVICE", "3")
    out = tmp_path / prefix
    assert cli.main(["sketch", "-k", "17", "-s", "2", "-S", "9", "-Z", "-o", str(out), "a.fna", "b.fna"]) == 0
    assert sorted(p.name for p in tmp_path.iterdir()) == ["x.msh"]
    assert stub[0]["gpu"].device == 3
    assert stub[0]["paths"] == ["a.fna", "b.fna"]
    assert (stub[0]["k"], stub[0]["s"], stub[0]["seed"], stub[0]["individual"], stub[0]["preserve_case"]) == \
        (17, 2, 9, False, True)
    db = read_msh_py(tmp_path / "x.msh")
    assert (db.k, db.seed, db.sketch_size, db.preserve_case, db.noncanonical) == (17, 9, 2, True, False)
    assert list(db.names) == ["a.fna", "b.fna"]
    assert db.hashes.tolist() == [5, 6, 7, 8]


def test_sketch_list_expansion(stub, tmp_path):
    l1, l2 = tmp_path / "l1.txt", tmp_path / "l2.txt"
    l1.write_text("g/a.fna\n\n  g/b.fna.gz  \n")
    l2.write_text("h/c.fna")
    assert cli.main(["sketch", "-l", "-i", "-o", str(tmp_path / "db"), str(l1), str(l2)]) == 0
    assert stub[0]["paths"] == ["g/a.fna", "g/b.fna.gz", "h/c.fna"]
    assert stub[0]["individual"] is True
    assert (tmp_path / "db.msh").exists()


def test_sketch_files_rejects_bad_parameters_before_the_device():
    with pytest.raises(ValueError):
        sk.sketch_files(None, [], k=33)
    with pytest.raises(ValueError):
        sk.sketch_files(None, [], s=0)
    with pytest.raises(ValueError):
        sk.sketch_files(None, [], s=sk.max_sketch_size() + 1)
    assert sk.max_sketch_size() >= 10_000


def test_sketch_files_skips_with_warning_without_device_work(tmp_path, capsys):
    """Files with no usable record never reach the device: the empty DB comes back from the
    host alone (gpu=None would fail on first use)."""
    a = tmp_path / "a.fna"
    a.write_text(">tiny x\nACGT\n")
    b = tmp_path / "b.fna.gz"
    with gzip.open(b, "wb") as f:
        f.write(b">t2\nACGTACGT\n")
    db = sk.sketch_files(None, [str(a), str(b)], k=21)
    assert db.n_refs == 0 and len(db.hashes) == 0 and db.offsets.tolist() == [0]
    err = capsys.readouterr().err
    assert "a.fna" in err and "b.fna.gz" in err
    db = sk.sketch_files(None, [str(a)], k=21, individual=True)
    assert db.n_refs == 0
    assert "tiny" in capsys.readouterr().err
