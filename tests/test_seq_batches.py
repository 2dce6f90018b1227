"""The batched sequence reader (seqio.iter_seq_batches) against the whole-text parsers, the
`--batch-bases` flag of `cli sketch` / `cli dist`, and file_meta collected over batches.  No GPU."""
import gzip

import numpy as np
import pytest

from tests import _reads_ref as rr
from tests._data import rand_seq

BATCH_BASES = (1, 300, 5_000, 1 << 40)
BLOCK_BYTES = (64, 1_000, 1 << 20)


def _recs(n=60, seed=3):
    """Reads of varying length, an empty one and a one-base one among them; comments on some."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        L = 0 if i == 7 else 1 if i == 11 else int(rng.integers(20, 160))
        out.append((f"read{i}", "a  comment" if i % 5 == 0 else "", rand_seq(rng, L) if L else b""))
    return out


def _fasta(recs, width=37, eol=b"\n"):
    out = []
    for name, comment, seq in recs:
        out.append(b">" + (name + (" " + comment if comment else "")).encode() + eol)
        out.extend(seq[i:i + width] + eol for i in range(0, len(seq), width))
    return b"".join(out)


def _records(ss):
    return [(ss.names[i], ss.comments[i], ss.seq(i)) for i in range(ss.n)]


def _check_batches(batches, want, batch_bases):
    """The batches hold `want` in order, whole; every batch but the last reaches batch_bases --
    with the record that closes it, so without that record it does not -- or is one record."""
    got = [r for ss in batches for r in _records(ss)]
    assert got == want
    assert len(batches) >= 1
    for ss in batches:
        assert ss.buf == b"N".join(r[2] for r in _records(ss))          # a SeqSet as from_records makes it
    for ss in batches[:-1]:
        assert ss.n >= 1
        assert ss.total_bases >= batch_bases or ss.n == 1
        assert ss.total_bases - int(ss.lengths[-1]) < batch_bases       # closed by the record that reached it


def _write(path, data):
    if str(path).endswith(".gz"):
        with gzip.open(path, "wb") as f:
            f.write(data)
    else:
        path.write_bytes(data)
    return path


FASTQ_TEXTS = {
    "plain": lambda r: rr.fastq_bytes(r),
    "crlf": lambda r: rr.fastq_bytes(r, crlf=True),
    "no_final_newline": lambda r: rr.fastq_bytes(r, final_newline=False),
    "crlf_no_final_newline": lambda r: rr.fastq_bytes(r, crlf=True, final_newline=False),
    "leading_blank_lines": lambda r: b"\n\n" + rr.fastq_bytes(r),
    "quality_like_headers": lambda r: b"@a c1\nACGT\n+\n@III\n@b\nGGCC\n+a\n>III\n" + rr.fastq_bytes(r),
}


@pytest.mark.parametrize("shape", sorted(FASTQ_TEXTS))
@pytest.mark.parametrize("suffix", [".fastq", ".fastq.gz"])
def test_fastq_batches_equal_the_whole_parse(tmp_path, shape, suffix):
    from hymet_amd.seqio import iter_seq_batches, parse_fastq_bytes
    data = FASTQ_TEXTS[shape](_recs())
    want = parse_fastq_bytes(data)
    assert len(want) >= 60
    path = _write(tmp_path / ("reads" + suffix), data)
    for bb in BATCH_BASES:
        for blk in BLOCK_BYTES:
            batches = list(iter_seq_batches(path, bb, block_bytes=blk))
            _check_batches(batches, want, bb)
            if shape != "leading_blank_lines" and bb == 300:
                assert len(batches) > 5                    # streamed, not one whole-file batch
            if shape == "leading_blank_lines":
                assert len(batches) == 1                   # the first piece is not of the four-line shape


def test_fasta_batches_equal_the_whole_parse(tmp_path):
    from hymet_amd.seqio import iter_seq_batches, parse_fasta_bytes
    texts = {"plain": _fasta(_recs()), "crlf": _fasta(_recs(), eol=b"\r\n"), "junk": b"junk line\n\n" + _fasta(_recs()),
             "no_final_newline": _fasta(_recs())[:-1], "header_only_tail": _fasta(_recs()) + b">last"}
    for name, data in texts.items():
        want = parse_fasta_bytes(data)
        assert len(want) >= 60
        for suffix in (".fna", ".fna.gz"):
            path = _write(tmp_path / (name + suffix), data)
            for bb in BATCH_BASES:
                for blk in BLOCK_BYTES:
                    batches = list(iter_seq_batches(path, bb, block_bytes=blk))
                    _check_batches(batches, want, bb)
                    if bb == 300:
                        assert len(batches) > 5


def test_default_block_and_read_seqs_agree(tmp_path):
    from hymet_amd.seqio import iter_seq_batches, read_seqs
    reads = list(rr.read_set())
    path = rr.write_fastq(tmp_path / "reads.fastq.gz", reads)
    whole = read_seqs([path])
    batches = list(iter_seq_batches(path, 5_000))
    assert len(batches) == 10                              # 34 reads of 150 bases reach 5,000
    _check_batches(batches, _records(whole), 5_000)
    one = list(iter_seq_batches(path, 1 << 29))
    assert len(one) == 1 and one[0].buf == whole.buf and one[0].names == whole.names


def test_empty_files_give_one_empty_batch(tmp_path):
    from hymet_amd.seqio import iter_seq_batches
    for name, data in (("e.fastq", b""), ("w.fastq", b"\n \n"), ("j.fna", b"no record here\n")):
        path = _write(tmp_path / name, data)
        for blk in (1, 1 << 20):
            batches = list(iter_seq_batches(path, 100, block_bytes=blk))
            assert len(batches) == 1 and batches[0].n == 0


@pytest.mark.parametrize("blk", BLOCK_BYTES)
def test_wrapped_fastq_falls_back_to_one_batch(tmp_path, blk):
    from hymet_amd.seqio import iter_seq_batches, parse_fastq_bytes
    recs = _recs()
    for i, data in enumerate((rr.fastq_bytes(recs, wrap=4), rr.fastq_bytes(recs, wrap=4, crlf=True, final_newline=False),
                              b"@a c1\nAC\nGT\n+\nII\n@I\n@b\nGG\nCC\n+\n>I\nII\n")):
        want = parse_fastq_bytes(data)
        path = _write(tmp_path / f"w{i}.fastq", data)
        batches = list(iter_seq_batches(path, 50, block_bytes=blk))
        assert len(batches) == 1
        assert _records(batches[0]) == want
    assert _records(batches[0]) == [("a", "c1", b"ACGT"), ("b", "", b"GGCC")]


def test_wrapped_tail_after_four_line_records(tmp_path):
    """Four-line records, then wrapped ones: the accepted pieces end at a record boundary, the
    rest goes through the general rules; together the whole text's records."""
    from hymet_amd.seqio import iter_seq_batches, parse_fastq_bytes
    recs = _recs()
    data = rr.fastq_bytes(recs[:40]) + rr.fastq_bytes(recs[40:], wrap=9)
    want = parse_fastq_bytes(data)
    assert want == recs
    path = _write(tmp_path / "mixed.fastq", data)
    for blk in BLOCK_BYTES:
        batches = list(iter_seq_batches(path, 300, block_bytes=blk))
        assert [r for ss in batches for r in _records(ss)] == want


@pytest.mark.parametrize("blk", BLOCK_BYTES)
def test_truncated_fastq_raises_the_same_error(tmp_path, blk):
    from hymet_amd.seqio import iter_seq_batches, parse_fastq_bytes
    good = rr.fastq_bytes(_recs(20))
    for i, tail in enumerate((b"@last one\nACGTACGT\n+\nIIII\n", b"@last one\nACGTACGT\n+\n", b"@last one\nACGTACGT\n")):
        data = good + tail
        with pytest.raises(ValueError) as whole:
            parse_fastq_bytes(data)
        path = _write(tmp_path / f"t{i}.fastq", data)
        with pytest.raises(ValueError) as got:
            list(iter_seq_batches(path, 300, block_bytes=blk))
        assert str(got.value) == str(whole.value) and "last" in str(got.value)


# ------------------------------------------------------------------ arguments
def test_batch_bases_flag(capsys):
    from hymet_amd import cli
    from hymet_amd.sketch import DEFAULT_BATCH_BASES
    a = cli.sketch_args(["-r", "--batch-bases", "5k", "-o", "x", "f.fq"])
    assert (a.reads, a.batch_bases) == (True, 5_000)
    assert cli.sketch_args(["--batch-bases", "1.5G", "-o", "x", "f.fna"]).batch_bases == 1_500_000_000
    assert cli.sketch_args(["-r", "-o", "x", "f.fq"]).batch_bases == DEFAULT_BATCH_BASES == 1 << 29
    a = cli.dist_args(["-m", "2", "--batch-bases", "5k", "ref.msh", "reads.fastq"])
    assert (a.reads, a.min_copies, a.batch_bases) == (True, 2, 5_000)
    assert cli.dist_args(["ref.msh", "q.fna"]).batch_bases == DEFAULT_BATCH_BASES
    capsys.readouterr()
    for bad in ("zero", "0", "-3", "k", ""):
        assert cli.sketch_args(["-r", f"--batch-bases={bad}", "-o", "x", "f.fq"]) is None
        assert cli.SKETCH_USAGE in capsys.readouterr().err
        assert cli.dist_args([f"--batch-bases={bad}", "ref.msh", "q.fq"]) is None
        assert cli.DIST_USAGE in capsys.readouterr().err
    assert cli.sketch_args(["-r", "--batch-bases", "-o", "x", "f.fq"]) is None      # the value is missing
    assert cli.main(["sketch", "-r", "--batch-bases", "none", "-o", "x", "f.fq"]) == 2
    assert cli.main(["dist", "--batch-bases", "none", "ref.msh", "q.fq"]) == 2
    assert cli.sketch_args(["--batch", "5k", "-o", "x", "f.fq"]) is None            # no abbreviations
    capsys.readouterr()
    assert "--batch-bases SIZE" in cli.SKETCH_USAGE and "--batch-bases SIZE" in cli.DIST_USAGE
    assert "--batch-bases" in cli.cmd_sketch.__doc__ and "--batch-bases" in cli.cmd_dist.__doc__
    assert "--batch-bases" in cli.__doc__


# ------------------------------------------------------------------ file_meta over batches
def test_file_meta_collected_over_batches(tmp_path):
    from hymet_amd.seqio import iter_seq_batches, read_seqs
    from hymet_amd.sketch import FileMetaAcc, file_meta
    recs = [("short", "too short", b"ACGT")] + _recs()
    path = str(_write(tmp_path / "reads.fastq", rr.fastq_bytes(recs)))
    whole = read_seqs([path])
    for k in (21, 3, 100, 1000):
        want = file_meta(path, whole.names, whole.comments, whole.lengths, k)
        for bb in (1, 300, 1 << 40):
            acc = FileMetaAcc(k)
            for ss in iter_seq_batches(path, bb, block_bytes=1_000):
                acc.add(ss.names, ss.comments, ss.lengths)
            assert acc.meta(path) == want
    assert file_meta(path, whole.names, whole.comments, whole.lengths, 1000) is None
    name, comment, length = file_meta(path, whole.names, whole.comments, whole.lengths, 21)
    n_ok = sum(1 for r in recs if len(r[2]) >= 21)
    assert (name, comment) == (path, f"[{n_ok} seqs] read0 a  comment [...]")
    assert length == sum(len(r[2]) for r in recs if len(r[2]) >= 21)
    one = FileMetaAcc(21)
    one.add(["a", "b"], ["c", ""], [5, 30])
    assert one.meta("p") == ("p", "b", 30)


def test_file_batches_reiterate(tmp_path):
    """sketch_files' re-iterable: the first iteration goes on from the batches already read and
    collects file_meta's inputs, later ones read the file again."""
    from hymet_amd.seqio import iter_seq_batches, read_seqs
    from hymet_amd.sketch import _FileBatches, file_meta
    path = rr.write_fastq(tmp_path / "reads.fastq", list(rr.read_set()))
    whole = read_seqs([path])
    it = iter_seq_batches(path, 5_000)
    head = [next(it), next(it)]
    fb = _FileBatches(path, 5_000, head, it, 21)
    first = [r for ss in fb for r in _records(ss)]
    again = [r for ss in fb for r in _records(ss)]
    assert first == again == _records(whole)
    assert fb.acc.meta(path) == file_meta(path, whole.names, whole.comments, whole.lengths, 21)
