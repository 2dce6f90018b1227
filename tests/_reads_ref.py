"""Plain-Python restatement of the read-set sketch (`mash sketch -r -m M`) and the seeded read
set the CPU and GPU tests share.  Nothing here is fast or clever: the multiplicity of every
canonical k-mer hash is counted in a Counter, and the sketch is read off it."""
import gzip
from collections import Counter
from functools import lru_cache

import numpy as np

from tests._data import mutate, rand_seq, revcomp

_RC = bytes.maketrans(b"ACGT", b"TGCA")
_ACGT = frozenset(b"ACGT")


def hash_counter(seqs, k, seed, preserve_case=False) -> Counter:
    """hash -> copies over every k-mer start of every sequence: the k-mer upper-cased (unless
    preserve_case), skipped if it holds a non-ACGT letter, the lexicographically smaller of it
    and its reverse complement hashed with murmur3_h0 (k > 16) or murmur3_x86_32 (k <= 16)."""
    from oracle import oracle_lib
    fn = oracle_lib.murmur3_h0 if k > 16 else oracle_lib.murmur3_x86_32
    cnt = Counter()
    for seq in seqs:
        for i in range(len(seq) - k + 1):
            km = seq[i:i + k]
            if not preserve_case:
                km = km.upper()
            if not _ACGT.issuperset(km):
                continue
            rc = km.translate(_RC)[::-1]
            cnt[fn(min(km, rc), seed)] += 1
    return cnt


def counted_ref(seqs, k, seed, s, m, preserve_case=False):
    """(hashes uint64, counts uint32): the s smallest hashes seen at least m times, ascending."""
    cnt = hash_counter(seqs, k, seed, preserve_case)
    keep = sorted(h for h, c in cnt.items() if c >= m)[:s]
    return np.array(keep, np.uint64), np.array([cnt[h] for h in keep], np.uint32)


@lru_cache(maxsize=None)
def _make():
    rng = np.random.default_rng(20261)
    genome = rand_seq(rng, 6_000)
    reads = []
    for i in range(320):
        p = int(rng.integers(0, len(genome) - 150 + 1))
        r = mutate(rng, genome[p:p + 150], 0.01)
        reads.append(revcomp(r) if i & 1 else r)
    return genome, tuple(reads)


def genome() -> bytes:
    return _make()[0]


def read_set():
    """The seeded read set: a 6,000-base genome, 320 reads of 150 bases at uniform positions
    (8x), 1 % substitutions, every second read reverse-complemented.  41,600 21-mers, 16,610
    distinct, 10,779 of them seen once; M = 2 and M = 3 both fill s = 1,000, with about 3,000
    distinct hashes at or below the last kept one."""
    return _make()[1]


def fastq_bytes(recs, wrap=None, crlf=False, final_newline=True) -> bytes:
    """FASTQ text of [(name, comment, seq)]; wrap: sequence and quality line width."""
    eol = b"\r\n" if crlf else b"\n"
    out = []
    for name, comment, seq in recs:
        qual = b"I" * len(seq)
        out.append(b"@" + (name + (" " + comment if comment else "")).encode())
        w = wrap or max(len(seq), 1)
        out.extend(seq[i:i + w] for i in range(0, max(len(seq), 1), w))
        out.append(b"+")
        out.extend(qual[i:i + w] for i in range(0, max(len(seq), 1), w))
    data = eol.join(out) + eol
    return data if final_newline else data[:-len(eol)]


def write_fastq(path, seqs, prefix="read", **kw):
    data = fastq_bytes([(f"{prefix}{i}", "", s) for i, s in enumerate(seqs)], **kw)
    if str(path).endswith(".gz"):
        with gzip.open(path, "wb") as f:
            f.write(data)
    else:
        with open(path, "wb") as f:
            f.write(data)
    return str(path)
