"""Read-set sketching, the parts that need no GPU: the plain-Python restatement against the CPU
oracle, the FASTQ reader, the argument rules of `cli sketch` / `cli dist` and the length rule."""
import gzip

import numpy as np
import pytest

from tests import _reads_ref as rr
from tests._data import rand_seq


@pytest.mark.parametrize("k", [21, 16])
def test_restatement_equals_oracle_at_one_copy(k):
    from oracle import oracle_lib
    reads = rr.read_set()
    h, c = rr.counted_ref(reads, k, 42, 1000, 1)
    np.testing.assert_array_equal(h, oracle_lib.sketch(list(reads), k, 42, 1000))
    assert len(c) == 1000 and c.min() >= 1


def test_read_set_shape():
    cnt = rr.hash_counter(rr.read_set(), 21, 42)
    assert (sum(cnt.values()), len(cnt), sum(1 for v in cnt.values() if v == 1)) == (41_600, 16_610, 10_779)
    for m in (2, 3):
        h, c = rr.counted_ref(rr.read_set(), 21, 42, 1000, m)
        assert len(h) == 1000 and c.min() >= m


def test_hand_made_counts():
    rng = np.random.default_rng(5)
    a, b = rand_seq(rng, 60), rand_seq(rng, 60)
    k = 21
    h, c = rr.counted_ref([a, b, a, a], k, 42, 1000, 2)
    only_a, ca = rr.counted_ref([a], k, 42, 1000, 1)
    np.testing.assert_array_equal(h, only_a)          # b's k-mers are seen once: gone
    assert len(h) == 60 - k + 1 and ca.tolist() == [1] * len(h) and c.tolist() == [3] * len(h)
    h1, c1 = rr.counted_ref([a, b, a, a], k, 42, 1000, 1)
    assert len(h1) == 2 * (60 - k + 1) and sorted(set(c1.tolist())) == [1, 3]
    assert len(rr.counted_ref([a, b, a, a], k, 42, 1000, 4)[0]) == 0
    # strands fold: a read and its reverse complement are two copies
    from tests._data import revcomp
    h2, c2 = rr.counted_ref([a, revcomp(a)], k, 42, 1000, 2)
    np.testing.assert_array_equal(h2, only_a)
    assert c2.tolist() == [2] * len(h2)
    # case: folded by default, a lower-case k-mer is no k-mer with preserve_case
    low = a[:30] + a[30:].lower()
    np.testing.assert_array_equal(rr.counted_ref([low], k, 42, 1000, 1)[0], only_a)
    assert len(rr.counted_ref([low], k, 42, 1000, 1, preserve_case=True)[0]) == 30 - k + 1


# ------------------------------------------------------------------ FASTQ
RECS = [("r1", "first read", b"ACGTACGTAC"), ("r2", "", b"GGGTTTAAACCCGG"), ("r3", "x y  z", b"T")]


def test_fastq_four_line_records():
    from hymet_amd.seqio import _fastq_four_lines, parse_fastq_bytes
    data = rr.fastq_bytes(RECS)
    assert _fastq_four_lines(data) == RECS
    assert parse_fastq_bytes(data) == RECS
    assert parse_fastq_bytes(rr.fastq_bytes(RECS, final_newline=False)) == RECS
    assert parse_fastq_bytes(rr.fastq_bytes(RECS, crlf=True)) == RECS
    assert parse_fastq_bytes(rr.fastq_bytes(RECS, crlf=True, final_newline=False)) == RECS


def test_fastq_wrapped_records_take_the_general_path():
    from hymet_amd.seqio import _fastq_four_lines, parse_fastq_bytes
    data = rr.fastq_bytes(RECS, wrap=4)
    assert _fastq_four_lines(data) is None
    assert parse_fastq_bytes(data) == RECS
    assert parse_fastq_bytes(rr.fastq_bytes(RECS, wrap=4, crlf=True, final_newline=False)) == RECS


def test_fastq_quality_lines_that_look_like_headers():
    from hymet_amd.seqio import parse_fastq_bytes
    # four-line records whose quality starts with '@' / '>'
    data = b"@a c1\nACGT\n+\n@III\n@b\nGGCC\n+a\n>III\n"
    want = [("a", "c1", b"ACGT"), ("b", "", b"GGCC")]
    assert parse_fastq_bytes(data) == want
    # wrapped: the second quality line of a starts with '@', the first of b with '>'
    data = b"@a c1\nAC\nGT\n+\nII\n@I\n@b\nGG\nCC\n+\n>I\nII\n"
    assert parse_fastq_bytes(data) == want
    # leading blank lines, an empty record between two others
    data = b"\n\n@a c1\nACGT\n+\nIIII\n@e\n\n+\n\n@b\nGGCC\n+\nIIII\n"
    assert parse_fastq_bytes(data) == [want[0], ("e", "", b""), want[1]]


def test_fastq_empty_and_truncated():
    from hymet_amd.seqio import parse_fastq_bytes
    assert parse_fastq_bytes(b"") == []
    assert parse_fastq_bytes(b"\n \n") == []
    for bad in (b"@a\nACGT\n+\nIIII\n@last one\nACGTACGT\n+\nIIII\n",      # quality cut short
                b"@a\nACGT\n+\nIIII\n@last one\nACGTACGT\n+\n",            # no quality
                b"@a\nACGT\n+\nIIII\n@last one\nACGTACGT\n"):              # no '+' line
        with pytest.raises(ValueError, match="last"):
            parse_fastq_bytes(bad)


def test_read_seqs_mixes_fasta_and_fastq(tmp_path):
    from hymet_amd.seqio import read_fasta, read_seqs
    fa = tmp_path / "a.fna"
    fa.write_bytes(b">c1 contig one\nACGTAC\nGTAC\n>c2\nTTTT\n")
    fq = tmp_path / "b.fastq.gz"
    with gzip.open(fq, "wb") as f:
        f.write(b"\n" + rr.fastq_bytes(RECS))
    empty = tmp_path / "e.fastq"
    empty.write_bytes(b"")
    ss = read_seqs([fa, fq, empty, fa])
    assert ss.names == ["c1", "c2", "r1", "r2", "r3", "c1", "c2"]
    assert ss.comments == ["contig one", "", "first read", "", "x y  z", "contig one", ""]
    assert [ss.seq(i) for i in range(ss.n)] == [b"ACGTACGTAC", b"TTTT"] + [r[2] for r in RECS] + [b"ACGTACGTAC", b"TTTT"]
    assert ss.file_of.tolist() == [0, 0, 1, 1, 1, 3, 3]
    assert ss.files == [str(fa), str(fq), str(empty), str(fa)]
    one = read_fasta([fa])
    two = read_seqs(fa)
    assert (one.names, one.buf, one.files) == (two.names, two.buf, two.files)
    assert read_seqs([empty]).n == 0


# ------------------------------------------------------------------ arguments
def test_sketch_args_read_options(capsys):
    from hymet_amd import cli
    assert cli.sketch_args(["-m", "0", "-o", "x", "f.fq"]) is None
    assert cli.sketch_args(["-r", "-i", "-o", "x", "f.fq"]) is None
    assert cli.sketch_args(["-m", "2", "-i", "-o", "x", "f.fq"]) is None
    assert cli.sketch_args(["-g", "zero", "-r", "-o", "x", "f.fq"]) is None
    assert cli.main(["sketch", "-m", "0", "-o", "x", "f.fq"]) == 2
    assert cli.main(["sketch", "-r", "-i", "-o", "x", "f.fq"]) == 2
    a = cli.sketch_args(["-m", "2", "-o", "x", "f.fq"])
    assert (a.reads, a.min_copies, a.genome_size) == (True, 2, None)
    a = cli.sketch_args(["-r", "-g", "4.6m", "-o", "x", "f.fq"])
    assert (a.reads, a.min_copies, a.genome_size) == (True, 1, 4_600_000)
    a = cli.sketch_args(["-o", "x", "f.fna"])
    assert (a.reads, a.min_copies, a.genome_size) == (False, 1, None)
    assert "-m M" in cli.SKETCH_USAGE and "-r" in cli.SKETCH_USAGE and "-g SIZE" in cli.SKETCH_USAGE
    capsys.readouterr()


def test_dist_args_read_options(capsys):
    from hymet_amd import cli
    assert cli.dist_args(["-r", "ref.msh", "q.msh"]) is None
    assert cli.dist_args(["-m", "2", "ref.msh", "q1.msh", "q2.msh"]) is None
    assert cli.dist_args(["-m", "0", "ref.msh", "q.fq"]) is None
    assert cli.dist_args(["-r", "-i", "ref.msh", "q.fq"]) is None
    assert cli.main(["dist", "-r", "ref.msh", "q.msh"]) == 2
    a = cli.dist_args(["-m", "2", "ref.msh", "q.msh", "reads.fastq.gz"])
    assert (a.reads, a.min_copies, a.queries) == (True, 2, ["q.msh", "reads.fastq.gz"])
    a = cli.dist_args(["-r", "--top", "10", "ref.msh", "reads.fastq"])
    assert (a.reads, a.min_copies, a.top) == (True, 1, 10)
    a = cli.dist_args(["ref.msh", "q.fna"])
    assert (a.reads, a.min_copies) == (False, 1)
    capsys.readouterr()


def test_sketch_files_refuses_reads_with_individual():
    from hymet_amd import sketch as sk
    with pytest.raises(ValueError, match="individual"):
        sk.sketch_files(None, [], reads=True, individual=True)
    with pytest.raises(ValueError, match="individual"):
        sk.sketch_files(None, [], min_copies=2, individual=True)
    with pytest.raises(ValueError, match="min_copies"):
        sk.sketch_files(None, [], min_copies=0)


# ------------------------------------------------------------------ the length rule
def test_read_set_length_rule():
    from hymet_amd.sketch import read_set_length
    full64 = np.array([5, 1 << 40, 1 << 62], np.uint64)
    assert read_set_length(full64, 3, 21) == 12                      # 3 * 2^64 / 2^62
    assert read_set_length(full64, 3, 17) == 12
    full32 = np.array([7, 1 << 20, 1 << 30], np.uint64)
    assert read_set_length(full32, 3, 16) == 12                      # 3 * 2^32 / 2^30
    assert read_set_length(full32, 3, 9) == 12
    assert read_set_length(np.array([3, 3 << 61], np.uint64), 2, 21) == 5    # 16 / 3 = 5.33
    assert read_set_length(np.array([3, 3 << 60], np.uint64), 2, 21) == 11   # 32 / 3 = 10.67
    assert read_set_length(np.array([1, 1 << 63], np.uint64), 2, 21) == 4
    assert read_set_length(np.array([(1 << 64) - 1], np.uint64), 1, 21) == 1
    # not full: every qualifying k-mer is in the row
    assert read_set_length(full64, 4, 21) == 3
    assert read_set_length(np.zeros(0, np.uint64), 1000, 21) == 0
    # h_max = 0 divides by 1
    assert read_set_length(np.array([0], np.uint64), 1, 21) == 1 << 64
    assert read_set_length(np.array([0], np.uint64), 1, 16) == 1 << 32
    # -g wins, full or not
    assert read_set_length(full64, 3, 21, genome_size=6000) == 6000
    assert read_set_length(full64, 4, 21, genome_size=6000) == 6000
