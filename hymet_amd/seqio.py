"""FASTA / FASTQ input and the packed on-device sequence pool.

A *pool* is every sequence of a set of FASTA files concatenated with one 'N' separator
between records, so that no k-mer or minimizer window can span two records (the invalid
separator resets every rolling state).  On the device it is held packed: 2-bit codes
(16 bases / uint32) + an invalid-base bitmask (32 bases / uint32) -- 0.375 B per base.
The reference reads FASTA through Mash's and minimap2's kseq readers: a record name is the
first whitespace-delimited token after '>', the rest of the header line is the comment.
Sequencing reads come as FASTQ: read_seqs takes either format per file (parse_fastq_bytes, kseq's
FASTQ rules); read_fasta stays FASTA-only for the stage drop-ins and the mapper.
"""
from __future__ import annotations

import gzip
from dataclasses import dataclass, field
from typing import List, Optional, Sequence

import numpy as np

SEP = b"N"


@dataclass
class SeqSet:
    names: List[str]
    comments: List[str]
    lengths: np.ndarray          # int64 per record
    starts: np.ndarray           # int64 offset of each record inside `buf`
    buf: bytes                   # records joined by SEP
    files: List[str] = field(default_factory=list)
    file_of: Optional[np.ndarray] = None   # record -> file index

    @property
    def n(self) -> int:
        return len(self.names)

    @property
    def total_bases(self) -> int:
        return int(self.lengths.sum())

    def seq(self, i: int) -> bytes:
        s = int(self.starts[i])
        return self.buf[s:s + int(self.lengths[i])]

    def subset(self, idx: Sequence[int]) -> "SeqSet":
        return from_records([(self.names[i], self.comments[i], self.seq(i)) for i in idx])


def _open(path):
    with open(path, "rb") as f:
        magic = f.read(2)
    return gzip.open(path, "rb") if magic == b"\x1f\x8b" else open(path, "rb")


def parse_fasta_bytes(data: bytes):
    out = []
    if not data:
        return out
    if data.startswith(b">"):
        chunks = data[1:].split(b"\n>")
    else:  # tolerate leading junk before the first record (kseq skips to '>')
        i = data.find(b"\n>")
        if i < 0:
            return out
        chunks = data[i + 2:].split(b"\n>")
    for ch in chunks:
        nl = ch.find(b"\n")
        head = ch if nl < 0 else ch[:nl]
        body = b"" if nl < 0 else ch[nl + 1:]
        head = head.rstrip(b"\r")
        parts = head.split(None, 1)
        name = parts[0].decode() if parts else ""
        comment = parts[1].decode() if len(parts) > 1 else ""
        seq = body.replace(b"\n", b"").replace(b"\r", b"")
        out.append((name, comment, seq))
    return out


def from_records(records, files=None, file_of=None) -> SeqSet:
    names = [r[0] for r in records]
    comments = [r[1] for r in records]
    seqs = [r[2] for r in records]
    lengths = np.array([len(s) for s in seqs], dtype=np.int64)
    starts = np.zeros(len(seqs), dtype=np.int64)
    if len(seqs):
        starts[1:] = np.cumsum(lengths[:-1] + len(SEP))
    return SeqSet(names, comments, lengths, starts, SEP.join(seqs), list(files or []),
                  None if file_of is None else np.asarray(file_of, dtype=np.int64))


def read_fasta(paths) -> SeqSet:
    if isinstance(paths, (str, bytes)) or hasattr(paths, "__fspath__"):
        paths = [paths]
    recs, file_of = [], []
    for fi, p in enumerate(paths):
        with _open(p) as f:
            r = parse_fasta_bytes(f.read())
        recs.extend(r)
        file_of.extend([fi] * len(r))
    return from_records(recs, [str(p) for p in paths], file_of)


def _fastq_head(head: bytes):
    parts = head[1:].split(None, 1)
    return (parts[0].decode() if parts else "", parts[1].decode() if len(parts) > 1 else "")


def _fastq_four_lines(data: bytes):
    """The records of a FASTQ text in which every record is exactly four lines (header, sequence,
    '+' line, quality of the sequence's length), or None when the text is not of that shape.
    data: no '\\r', ends with a line break.  The shape is checked on the line-start bytes and
    line lengths as arrays, and the fields are cut with whole-text operations: nothing here
    loops over the records."""
    import re
    a = np.frombuffer(data, dtype=np.uint8)
    nl = np.flatnonzero(a == 10)
    n_lines = len(nl)
    if n_lines == 0 or n_lines % 4:
        return None
    starts = np.empty(n_lines, np.int64)
    starts[0] = 0
    starts[1:] = nl[:-1] + 1
    lens = nl - starts
    # a sequence line that itself starts with '+' would end the sequence under the general rules
    if not ((a[starts[0::4]] == 64).all() and (a[starts[2::4]] == 43).all() and (a[starts[1::4]] != 43).all()
            and (lens[1::4] == lens[3::4]).all()):
        return None
    lines = data.split(b"\n")                      # n_lines entries and a last empty one
    heads = b"\n".join(lines[0:n_lines:4])
    names = b"\n".join(re.findall(rb"^@[^\S\n]*(\S*)", heads, re.M)).decode().split("\n")
    comments = b"\n".join(re.findall(rb"^@[^\S\n]*\S*[^\S\n]*(.*)$", heads, re.M)).decode().split("\n")
    return list(zip(names, comments, lines[1:n_lines:4]))


def parse_fastq_bytes(data: bytes):
    """[(name, comment, sequence)] of a FASTQ text, by kseq's rules: a record starts at a line
    beginning with '@' (name = the first whitespace-delimited token of that line, comment = the
    rest); its sequence is the following lines up to a line beginning with '+'; its quality is
    the lines after that until their summed length reaches the sequence's length -- so a quality
    line that starts with '@' or '>' is not a record start.  '\\r' is stripped, a missing final
    line break is fine, lines before the first record are skipped.  ValueError, naming the
    record, when the quality is shorter than the sequence at the end of the text (a truncated
    file) or longer than it.  Texts whose records are all four lines take a path without a
    loop over the records (_fastq_four_lines)."""
    data = bytes(data).replace(b"\r", b"")
    if not data.strip():
        return []
    if not data.endswith(b"\n"):
        data += b"\n"
    out = _fastq_four_lines(data)
    if out is not None:
        return out
    out = []
    lines = data.split(b"\n")
    lines.pop()                                    # the empty piece behind the last line break
    i, n = 0, len(lines)
    while i < n:
        if not lines[i].startswith(b"@"):
            i += 1
            continue
        name, comment = _fastq_head(lines[i])
        i += 1
        seq = []
        while i < n and not lines[i].startswith(b"+"):
            seq.append(lines[i])
            i += 1
        seq = b"".join(seq)
        i += 1                                     # the '+' line
        q = 0
        while i < n and q < len(seq):
            q += len(lines[i])
            i += 1
        if q != len(seq):
            raise ValueError(f"FASTQ record {name!r}: quality of {q} characters for a sequence of {len(seq)}"
                             + (" (truncated file?)" if q < len(seq) else ""))
        out.append((name, comment, seq))
    return out


def read_seqs(paths) -> SeqSet:
    """read_fasta for FASTA and FASTQ files alike (gzip too): per file, the first byte after
    leading white space decides -- '@' is FASTQ (parse_fastq_bytes), anything else goes to
    parse_fasta_bytes.  files / file_of as read_fasta."""
    import re
    if isinstance(paths, (str, bytes)) or hasattr(paths, "__fspath__"):
        paths = [paths]
    recs, file_of = [], []
    for fi, p in enumerate(paths):
        with _open(p) as f:
            data = f.read()
        m = re.search(rb"\S", data)
        fastq = m is not None and data[m.start():m.start() + 1] == b"@"
        r = parse_fastq_bytes(data) if fastq else parse_fasta_bytes(data)
        recs.extend(r)
        file_of.extend([fi] * len(r))
    return from_records(recs, [str(p) for p in paths], file_of)


DEFAULT_BLOCK_BYTES = 1 << 24


def _record_batches(recs, pending, batch_bases):
    """Move recs behind pending (a list of records and its number of bases) and yield a SeqSet
    whenever the collected records hold batch_bases bases; the cuts are found on the cumulated
    lengths, not by a loop over the records."""
    if not recs:
        return
    ends = np.cumsum(np.fromiter((len(r[2]) for r in recs), np.int64, len(recs)))
    done, at = 0, 0                       # records and bases of recs already handed on
    while True:
        # the first record with which pending reaches batch_bases
        j = int(np.searchsorted(ends, at + batch_bases - pending[1], side="left"))
        if j >= len(recs):
            break
        pending[0].extend(recs[done:j + 1])
        yield from_records(pending[0])
        pending[0], pending[1] = [], 0
        done, at = j + 1, int(ends[j])
    pending[0].extend(recs[done:])
    pending[1] += int(ends[-1]) - at


def iter_seq_batches(path, batch_bases: int, block_bytes: int = DEFAULT_BLOCK_BYTES):
    """The records of one FASTA or FASTQ file (gzip too) as SeqSets of whole records, in file
    order: every batch but the last holds at least batch_bases bases -- it is closed by the record
    that reaches them -- and at least one batch is yielded (an empty one for a file without
    records).  The file is read in blocks of block_bytes and never held whole: at any time there
    is one batch being collected plus one block (and the tail of the last block that did not end a
    record).  The concatenated records are those of read_seqs([path]); the format is decided as
    there, by the first byte after leading white space.

    FASTA: the text read so far is cut at its last b"\\n>", the piece before it goes through
    parse_fasta_bytes and the rest waits for the next block.  Every piece but the first starts
    with '>', a record's lines are never split, and leading junk stays in the first piece, so the
    pieces' records are the whole text's.

    FASTQ: '\\r' is dropped as parse_fastq_bytes drops it, and the text is cut at the last line
    break whose line index from the start of the file is a multiple of four.  A piece is accepted
    only if it has the strict four-line shape (_fastq_four_lines: '@' line, a sequence line not
    starting with '+', '+' line, a quality line of the sequence's length).  Why the pieces
    together are kseq's parse of the whole text: kseq is at a record boundary at the start of the
    file; on a text of the strict shape it reads, per four lines, the header, one sequence line
    (the next line starts with '+'), the '+' line and one quality line (its length reaches the
    sequence's at once), so after a piece that passes the check it stands at a record boundary
    again, exactly at the piece's end -- a multiple of four lines from the file's start, where
    the next piece begins.  By induction every accepted piece is parsed as kseq parses that
    stretch of the whole text, '@' or '>' at the start of a quality line included.
    A piece that is not of that shape (wrapped sequences, leading blank lines, a truncated tail)
    ends the streaming: it and the rest of the file go through parse_fastq_bytes -- kseq's rules
    from a record boundary on -- and are yielded, with the records still waiting, as one last
    batch.  When the first piece already fails, that is the whole file as one batch, read_seqs'
    behaviour; a wrapped FASTQ is therefore not streamed (out of scope).  A truncated file raises
    parse_fastq_bytes' ValueError."""
    import re
    batch_bases = max(1, int(batch_bases))
    block_bytes = max(1, int(block_bytes))
    pending = [[], 0]
    n_out = 0
    with _open(path) as f:
        buf = b""
        fastq = None
        while fastq is None:              # the first byte after leading white space decides
            block = f.read(block_bytes)
            buf += block
            m = re.search(rb"\S", buf)
            if m is not None:
                fastq = buf[m.start():m.start() + 1] == b"@"
            elif not block:
                fastq = False
        if fastq:
            buf = buf.replace(b"\r", b"")
        eof = False
        while not eof:
            block = f.read(block_bytes)
            eof = not block
            if fastq:
                buf += block.replace(b"\r", b"")
                if eof:
                    if buf and not buf.endswith(b"\n"):
                        buf += b"\n"
                    cut = len(buf)
                else:
                    nl = np.flatnonzero(np.frombuffer(buf, dtype=np.uint8) == 10)
                    cut = int(nl[len(nl) // 4 * 4 - 1]) + 1 if len(nl) >= 4 else 0
                piece = buf[:cut]
                recs = _fastq_four_lines(piece) if piece else []
                if recs is None:          # not the strict shape: the general rules for all that is left
                    pending[0].extend(parse_fastq_bytes(piece + buf[cut:] + f.read()))
                    break
                buf = b"" if eof else buf[cut:]
            else:
                buf += block
                cut = len(buf) if eof else buf.rfind(b"\n>") + 1
                recs = parse_fasta_bytes(buf[:cut]) if cut else []
                buf = buf[cut:]
            for ss in _record_batches(recs, pending, batch_bases):
                n_out += 1
                yield ss
    if pending[0] or n_out == 0:
        yield from_records(pending[0])


class DevicePool:
    """A SeqSet resident in HBM, packed for one alphabet (hymet_pack)."""

    ALPHA_MASH, ALPHA_MASH_PRESERVE_CASE, ALPHA_MINIMAP2 = 0, 1, 2

    def __init__(self, gpu, ss: SeqSet, alphabet: int):
        from ._lib import ptr

        torch = gpu.torch
        self.gpu = gpu
        self.ss = ss
        self.alphabet = alphabet
        self.n_bases = len(ss.buf)
        n = self.n_bases
        raw = torch.frombuffer(bytearray(ss.buf) if n else bytearray(b"N"), dtype=torch.uint8)
        d_ascii = raw.to(gpu.dev)
        self.w2b = gpu.zeros((n + 15) // 16 + 4, torch.int32)
        self.wmask = gpu.zeros((n + 31) // 32 + 4, torch.int32)
        if n:
            gpu.call("hymet_pack", ptr(d_ascii), n, alphabet, ptr(self.w2b), ptr(self.wmask))
        del d_ascii
        self.starts = torch.from_numpy(ss.starts).to(gpu.dev)
        self.lengths = torch.from_numpy(ss.lengths).to(gpu.dev)
