"""Sketch stage: the MI355X replacement for `mash sketch`, the step that builds the sketch
databases (`data/sketch{1,2,3}.msh`) the screen reads.  The reference workflow downloads
them; here they are built from genome FASTA files already on disk.

Device work (libhymet_gpu.so, csrc/sketch.hip): one call of `hymet_sketch_batch` sketches a
whole batch of references exactly -- every canonical k-mer of the packed pool is hashed once
(the screen's hashing) and the bottom-s distinct hashes of each reference are selected in
LDS.  Host work here: the chunk plan (which k-mer start positions belong to which
reference), FASTA reading in batches bounded by bases, and the references' metadata.

The metadata rules (name / comment / length of a reference, below) restate what Mash's
`sketch` writes from memory of its behaviour.  No Mash binary and no Mash-written .msh is
available to check them against: they are PARITY-UNPINNED, like the .msh schema (msh.py).
The hashes are pinned to the CPU oracle (oracle/mash_oracle.c oracle_sketch), as the
screen is pinned to oracle_screen.
"""
from __future__ import annotations

import ctypes
import sys
from typing import List, Optional, Sequence, Tuple

import numpy as np

from ._lib import load, ptr
from .msh import SketchDB

# k-mer start positions per chunk (= per workgroup).  Chosen among 256 k, 1 M and 4 M by
# tools/sketch_bench.py
DEFAULT_CHUNK_BASES = 1 << 20
# bases per batch of sketch_files: the ASCII pool on the host and in HBM, then 0.375 B per base
DEFAULT_BATCH_BASES = 1 << 29
# the streamed read-set sketch (sketch_stream).  max_live: 2^28 (hash, count) pairs are 3 GiB, and
# the merge writes a second list beside the first; chosen from memory, not measured.  slice_bases:
# k-mer starts per slice, chosen among 2^20, 2^22, 2^24 and 2^26 by tools/sketch_stream_bench.py
# (DESIGN.md §3 "Sketch: read sets, streamed")
DEFAULT_STREAM_MAX_LIVE = 1 << 28
DEFAULT_STREAM_SLICE_BASES = 1 << 26
# output rows per batch of sketch_files are capped so that rows x s x 8 B stays under this
_MAX_OUT_BYTES = 1 << 30


def plan_chunks(starts, lengths, group_of, k: int, chunk_bases: int):
    """The work plan of hymet_sketch_batch: (chunk_sketch int32, chunk_begin int64, chunk_end
    int64), sorted by sketch id.  starts / lengths: the records' offsets and lengths in the
    pool (SeqSet.starts / .lengths); group_of[i]: the sketch record i belongs to.  The records
    of a group must be contiguous in the pool (ValueError otherwise).

    Records shorter than k are skipped.  A group's span runs from the first k-mer start of its
    first usable record to one past the last k-mer start of its last usable one, and is cut
    into ceil(span / chunk_bases) chunks of equal size (the last may be shorter).  A chunk
    never crosses a group.  Every k-mer start of every record of length >= k is covered exactly
    once; positions in separators, in short records between usable ones and in the k - 1 tail
    of a record are covered too: their k-mers hold a separator, so the kernel drops them."""
    starts = np.asarray(starts, np.int64)
    lengths = np.asarray(lengths, np.int64)
    group_of = np.asarray(group_of, np.int64)
    if not (len(starts) == len(lengths) == len(group_of)):
        raise ValueError("plan_chunks: starts, lengths and group_of differ in length")
    if k < 1 or chunk_bases < 1:
        raise ValueError("plan_chunks: k and chunk_bases must be positive")
    empty = (np.zeros(0, np.int32), np.zeros(0, np.int64), np.zeros(0, np.int64))
    if len(group_of) == 0:
        return empty
    if group_of.min() < 0:
        raise ValueError("plan_chunks: negative group id")
    # runs of equal group id; a group seen in two runs is not contiguous
    run_first = np.flatnonzero(np.r_[True, group_of[1:] != group_of[:-1]])
    run_gid = group_of[run_first]
    if len(np.unique(run_gid)) != len(run_gid):
        raise ValueError("plan_chunks: the records of a group are not contiguous in the pool")
    if len(starts) > 1 and (np.diff(starts) < 0).any():
        raise ValueError("plan_chunks: record starts are not ascending")
    usable = np.flatnonzero(lengths >= k)
    if len(usable) == 0:
        return empty
    g = group_of[usable]
    first = np.flatnonzero(np.r_[True, g[1:] != g[:-1]])          # first usable record of each group
    last = np.r_[first[1:] - 1, len(g) - 1]
    gid = g[first]
    b = starts[usable[first]]
    e = starts[usable[last]] + lengths[usable[last]] - k + 1
    span = e - b
    n = -(-span // int(chunk_bases))
    size = -(-span // n)
    which = np.repeat(np.arange(len(gid)), n)                     # chunk -> group slot
    j = np.arange(int(n.sum())) - np.repeat(np.cumsum(n) - n, n)  # chunk index within its group
    cb = b[which] + j * size[which]
    ce = np.minimum(cb + size[which], e[which])
    keep = cb < ce     # ceil(span / size) can be below n: drop the empty tail chunks
    cs, cb, ce = gid[which][keep], cb[keep], ce[keep]
    order = np.argsort(cs, kind="stable")
    return cs[order].astype(np.int32), cb[order].astype(np.int64), ce[order].astype(np.int64)


def max_sketch_size() -> int:
    return int(load().hymet_sketch_max_size())


def sketch_pool(gpu, pool, group_of=None, k: int = 21, seed: int = 42, s: int = 1000,
                chunk_bases: Optional[int] = None) -> List[np.ndarray]:
    """Mash `sketch` of a packed pool (seqio.DevicePool): the bottom-s distinct canonical k-mer
    hashes of every group of records, sorted, as np.uint64 arrays -- one per group id in
    0..max(group_of).  group_of=None: one sketch per record (`mash sketch -i`).  One call of
    hymet_sketch_batch and one copy to the host, whatever the number of groups."""
    torch = gpu.torch
    ss = pool.ss
    if group_of is None:
        group_of = np.arange(ss.n, dtype=np.int64)
    group_of = np.asarray(group_of, np.int64)
    if len(group_of) != ss.n:
        raise ValueError("sketch_pool: group_of needs one entry per record")
    n_sk = int(group_of.max()) + 1 if len(group_of) else 0
    if n_sk == 0:
        return []
    s = int(s)
    cs, cb, ce = plan_chunks(ss.starts, ss.lengths, group_of, k, int(chunk_bases or DEFAULT_CHUNK_BASES))
    # rows and, behind them in the same buffer, the rows' counts: one copy brings both
    out = gpu.empty(n_sk * s + (n_sk + 1) // 2, torch.int64)
    d_n = ctypes.c_void_p(out.data_ptr() + 8 * n_sk * s)
    gpu.call("hymet_sketch_batch", ptr(pool.w2b), ptr(pool.wmask), pool.n_bases, int(k), int(seed), s, len(cs),
             cs.ctypes.data_as(ctypes.c_void_p), cb.ctypes.data_as(ctypes.c_void_p), ce.ctypes.data_as(ctypes.c_void_p),
             n_sk, ptr(out), d_n)
    host = out.cpu().numpy()
    rows = host[:n_sk * s].view(np.uint64).reshape(n_sk, s)
    cnt = host[n_sk * s:].view(np.int32)[:n_sk]
    return [rows[r, :c] for r, c in enumerate(cnt.tolist())]    # views of the one host copy


def max_counted_sketch_size() -> int:
    return int(load().hymet_sketch_counted_max_size())


def sketch_pool_counted(gpu, pool, group_of, k: int, seed: int, s: int, min_copies: int,
                        chunk_bases: Optional[int] = None) -> List[Tuple[np.ndarray, np.ndarray]]:
    """Mash `sketch -r -m M` of a packed pool: per group of records the s smallest canonical
    k-mer hashes seen at least min_copies times over the whole group, sorted (np.uint64), and
    each one's multiplicity (np.uint32) -- one (hashes, counts) pair per group id in
    0..max(group_of); group_of=None: one sketch per record.  Exact, whatever the chunking
    (csrc/sketch_counted.hip).  One call of hymet_sketch_counted and one copy to the host.
    sketch_pool_counted.stats holds what the last call did: {"passes", "merged"} (passes over the
    pool; (hash, count) pairs that went through a per-sketch merge)."""
    torch = gpu.torch
    ss = pool.ss
    if group_of is None:
        group_of = np.arange(ss.n, dtype=np.int64)
    group_of = np.asarray(group_of, np.int64)
    if len(group_of) != ss.n:
        raise ValueError("sketch_pool_counted: group_of needs one entry per record")
    n_sk = int(group_of.max()) + 1 if len(group_of) else 0
    sketch_pool_counted.stats = {"passes": 0, "merged": 0}
    if n_sk == 0:
        return []
    s = int(s)
    cs, cb, ce = plan_chunks(ss.starts, ss.lengths, group_of, k, int(chunk_bases or DEFAULT_CHUNK_BASES))
    # one buffer, one copy: the rows (8 B), their multiplicities (4 B), the rows' lengths (4 B)
    w_cnt = (n_sk * s + 1) // 2
    out = gpu.empty(n_sk * s + w_cnt + (n_sk + 1) // 2, torch.int64)
    d_cnt = ctypes.c_void_p(out.data_ptr() + 8 * n_sk * s)
    d_n = ctypes.c_void_p(out.data_ptr() + 8 * (n_sk * s + w_cnt))
    stats = (ctypes.c_int64 * 2)()
    gpu.call("hymet_sketch_counted", ptr(pool.w2b), ptr(pool.wmask), pool.n_bases, int(k), int(seed), s, int(min_copies),
             len(cs), cs.ctypes.data_as(ctypes.c_void_p), cb.ctypes.data_as(ctypes.c_void_p),
             ce.ctypes.data_as(ctypes.c_void_p), n_sk, ptr(out), d_cnt, d_n, ctypes.cast(stats, ctypes.c_void_p))
    sketch_pool_counted.stats = {"passes": int(stats[0]), "merged": int(stats[1])}
    host = out.cpu().numpy()
    rows = host[:n_sk * s].view(np.uint64).reshape(n_sk, s)
    cnts = host[n_sk * s:n_sk * s + w_cnt].view(np.uint32)[:n_sk * s].reshape(n_sk, s)
    n = host[n_sk * s + w_cnt:].view(np.int32)[:n_sk]
    return [(rows[r, :c], cnts[r, :c]) for r, c in enumerate(n.tolist())]    # views of the one host copy


sketch_pool_counted.stats = {"passes": 0, "merged": 0}


def sketch_stream(gpu, batches, k: int, seed: int, s: int, min_copies: int, max_live: Optional[int] = None,
                  slice_bases: Optional[int] = None, alphabet: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray]:
    """Mash `sketch -r -m M` of ONE read set given as batches: (hashes np.uint64, counts np.uint32),
    what sketch_pool_counted returns for the batches' records as one group, whatever the batches,
    slice_bases and max_live (csrc/sketch_stream.hip).  batches: a re-iterable of seqio.SeqSets
    of whole records (a list, or an object whose __iter__ reads the file again): each is packed
    (DevicePool, alphabet: DevicePool.ALPHA_MASH by default) and fed, one at a time in HBM, and the
    whole sequence is fed again for every further pass the device asks for.  max_live: (hash,
    count) pairs the window may hold between slices (DEFAULT_STREAM_MAX_LIVE); slice_bases: k-mer
    starts per slice (DEFAULT_STREAM_SLICE_BASES).  The counts saturate at 2^32 - 1; there is no
    limit on the read set's size.  sketch_stream.stats holds what the call did: {"passes",
    "slices", "emitted" (candidate hashes written), "max_live" (the most pairs the window held)}."""
    from ._lib import check
    from .seqio import DevicePool
    torch = gpu.torch
    lib = gpu.lib
    s = int(s)
    alphabet = DevicePool.ALPHA_MASH if alphabet is None else alphabet
    sketch_stream.stats = {"passes": 0, "slices": 0, "emitted": 0, "max_live": 0}
    h = ctypes.c_void_p()
    check(lib.hymet_sketch_stream_create(gpu.ctx, int(k), int(seed), s, int(min_copies),
                                         int(max_live or DEFAULT_STREAM_MAX_LIVE), ctypes.byref(h)),
          "hymet_sketch_stream_create")
    try:
        more = ctypes.c_int32(1)
        while more.value:
            for ss in batches:
                pool = DevicePool(gpu, ss, alphabet)
                check(lib.hymet_sketch_stream_add(h, ptr(pool.w2b), ptr(pool.wmask), pool.n_bases,
                                                  int(slice_bases or DEFAULT_STREAM_SLICE_BASES)), "hymet_sketch_stream_add")
                del pool
            check(lib.hymet_sketch_stream_end_pass(h, ctypes.byref(more)), "hymet_sketch_stream_end_pass")
        # one buffer, one copy: the row (8 B per entry), then its multiplicities (4 B)
        out = gpu.empty(s + (s + 1) // 2, torch.int64)
        n = ctypes.c_int32()
        stats = (ctypes.c_int64 * 4)()
        check(lib.hymet_sketch_stream_result(h, ptr(out), ctypes.c_void_p(out.data_ptr() + 8 * s), ctypes.byref(n),
                                             ctypes.cast(stats, ctypes.c_void_p)), "hymet_sketch_stream_result")
    finally:
        lib.hymet_sketch_stream_destroy(h)
    sketch_stream.stats = {"passes": int(stats[0]), "slices": int(stats[1]), "emitted": int(stats[2]),
                           "max_live": int(stats[3])}
    host = out.cpu().numpy()
    return host[:s].view(np.uint64)[:n.value], host[s:].view(np.uint32)[:n.value]


sketch_stream.stats = {"passes": 0, "slices": 0, "emitted": 0, "max_live": 0}


# ------------------------------------------------------------------ metadata (unpinned)
def read_set_length(hashes, s: int, k: int, genome_size: Optional[int] = None) -> int:
    """The `length` a read-set sketch carries in the .msh -- this project's rule, restating
    Mash's genome-size estimate from memory and unpinned like the other metadata: genome_size
    when given (`-g`); else for a full row (n = s hashes) the estimate n * 2^b / max(h_max, 1)
    rounded to the nearest integer (halves up), with b = 64, or 32 for k <= 16, and h_max the
    row's largest hash -- the hash space divided by the mean gap of the kept hashes; else (the
    row is not full: every qualifying k-mer is in it) n."""
    if genome_size is not None:
        return int(genome_size)
    n = len(hashes)
    if n < int(s) or n == 0:
        return n
    d = max(int(hashes[-1]), 1)
    return (2 * n * (1 << (32 if int(k) <= 16 else 64)) + d) // (2 * d)



def _join(name: str, comment: str) -> str:
    return f"{name} {comment}" if comment else name


def file_meta(path: str, names: Sequence[str], comments: Sequence[str], lengths: Sequence[int],
              k: int) -> Optional[Tuple[str, str, int]]:
    """(name, comment, length) of the reference `mash sketch` makes of one FASTA file, or None
    when no record has k bases (the file is skipped).  name = the path as given; length = the
    summed lengths of the records of >= k bases; comment = "<first name> <first comment>" for
    one such record, "[N seqs] <first name> <first comment> [...]" for N > 1.  Unpinned (module
    docstring)."""
    acc = FileMetaAcc(k)
    acc.add(names, comments, lengths)
    return acc.meta(path)


class FileMetaAcc:
    """file_meta's inputs collected over the batches of one file: the first record of >= k bases,
    the number of such records and their summed length."""

    def __init__(self, k: int):
        self.k = int(k)
        self.first: Optional[Tuple[str, str]] = None
        self.n = 0
        self.total = 0

    def add(self, names: Sequence[str], comments: Sequence[str], lengths: Sequence[int]):
        ok = [i for i, L in enumerate(lengths) if int(L) >= self.k]
        if ok and self.first is None:
            self.first = (names[ok[0]], comments[ok[0]])
        self.n += len(ok)
        self.total += int(sum(int(lengths[i]) for i in ok))

    def meta(self, path: str) -> Optional[Tuple[str, str, int]]:
        if self.first is None:
            return None
        head = _join(*self.first)
        comment = head if self.n == 1 else f"[{self.n} seqs] {head} [...]"
        return str(path), comment, self.total


class _FileBatches:
    """The batches of one read file as sketch_stream's re-iterable: the first iteration hands on
    the batches already read and goes on with the open reader, collecting file_meta's inputs on
    the way; every later one reads the file again."""

    def __init__(self, path, batch_bases: int, head, rest, k: int):
        self.path, self.batch_bases = path, batch_bases
        self.head, self.rest = head, rest
        self.acc = FileMetaAcc(k)

    def __iter__(self):
        if self.rest is None:
            from .seqio import iter_seq_batches
            yield from iter_seq_batches(self.path, self.batch_bases)
            return
        head, rest, self.head, self.rest = self.head, self.rest, None, None
        while head:
            ss = head.pop(0)
            self.acc.add(ss.names, ss.comments, ss.lengths)
            yield ss
        for ss in rest:
            self.acc.add(ss.names, ss.comments, ss.lengths)
            yield ss


def _warn(msg: str):
    print(f"WARNING: {msg}", file=sys.stderr)


def sketch_files(gpu, paths: Sequence[str], k: int = 21, seed: int = 42, s: int = 1000, individual: bool = False,
                 preserve_case: bool = False, batch_bases: int = DEFAULT_BATCH_BASES,
                 chunk_bases: Optional[int] = None, reads: bool = False, min_copies: int = 1,
                 genome_size: Optional[int] = None, read_info: Optional[list] = None) -> SketchDB:
    """`mash sketch [-i] [-Z] [-r] [-m M] [-g SIZE] -k K -s S -S SEED FILE...` -> SketchDB,
    references in argument order.  The files are FASTA or FASTQ (gzip too, seqio.read_seqs) and
    are sketched in batches of about batch_bases bases -- read, pack (DevicePool), sketch_pool --
    so neither the host nor HBM ever holds the whole collection; one file is the smallest unit of
    a batch, except a read file larger than a batch (below).

    File mode: one reference per file (file_meta); a file with no record of k bases is skipped
    with a warning.  individual (`-i`): one reference per record, named and commented as the
    record; shorter records are skipped with a warning.  preserve_case (`-Z`): lower-case bases
    are not k-mer letters.  Metadata rules unpinned (module docstring).

    reads (`-r`; min_copies > 1 implies it): every file is a read set and one sketch, named and
    commented by file_meta as in file mode, holding the s smallest hashes seen at least
    min_copies (`-m`) times in the file (sketch_pool_counted).  Its length is this project's
    rule (read_set_length): genome_size (`-g`) if given, else the genome-size estimate of a full
    row, else the number of hashes.  The multiplicities are not written to the .msh; read_info,
    when a list, receives per sketch (name, length, mean multiplicity of the kept hashes -- the
    estimated coverage).  Not with individual (ValueError).  A read file is read in batches of
    batch_bases bases (seqio.iter_seq_batches): one that ends within its first batch goes the way
    described above, grouped with its neighbours; a larger one is never held whole -- it is
    streamed through sketch_stream, batch by batch, to the same row, name, comment and length."""
    from .seqio import DevicePool, from_records, iter_seq_batches, read_seqs
    if not 1 <= int(k) <= 32:
        raise ValueError(f"k={k}: Mash k-mer sizes are 1..32")
    if int(min_copies) < 1:
        raise ValueError(f"min_copies={min_copies}: at least 1")
    reads = bool(reads) or int(min_copies) > 1
    if reads and individual:
        raise ValueError("a read set is one sketch per file: reads does not go with individual")
    s_max = max_counted_sketch_size() if reads else max_sketch_size()
    if not 1 <= int(s) <= s_max:
        raise ValueError(f"sketch size {s}: supported sizes are 1..{s_max}" + (" for read sets" if reads else ""))
    alpha = DevicePool.ALPHA_MASH_PRESERVE_CASE if preserve_case else DevicePool.ALPHA_MASH
    max_refs = max(1, _MAX_OUT_BYTES // (8 * int(s)))
    names: List[str] = []
    comments: List[str] = []
    lengths: List[int] = []
    hashes: List[np.ndarray] = []
    recs, group_of, meta = [], [], []     # the batch being collected
    bases = 0

    def flush():
        nonlocal recs, group_of, meta, bases
        if meta:
            pool = DevicePool(gpu, from_records(recs), alpha)
            if reads:
                pairs = sketch_pool_counted(gpu, pool, np.asarray(group_of, np.int64), k, seed, s, int(min_copies),
                                            chunk_bases)
                rows = [h for h, _ in pairs]
                meta = [(nm, cm, min(read_set_length(h, s, k, genome_size), (1 << 63) - 1))   # SketchDB lengths: int64
                        for (nm, cm, _), h in zip(meta, rows)]
                if read_info is not None:
                    read_info.extend((nm, ln, float(c.mean()) if len(c) else 0.0)
                                     for (nm, _, ln), (_, c) in zip(meta, pairs))
            else:
                rows = sketch_pool(gpu, pool, np.asarray(group_of, np.int64), k, seed, s, chunk_bases)
            del pool
            for (nm, cm, ln), h in zip(meta, rows):
                names.append(nm)
                comments.append(cm)
                lengths.append(ln)
                hashes.append(h)
        recs, group_of, meta, bases = [], [], [], 0

    def stream(p, head, rest):
        """A read file of more than one batch: sketched on its own, batch by batch."""
        fb = _FileBatches(p, batch_bases, head, rest, k)
        h, c = sketch_stream(gpu, fb, k, seed, s, int(min_copies), alphabet=alpha)
        m = fb.acc.meta(str(p))
        if m is None:
            _warn(f"Skipping {p}: no sequence of at least {k} bases.")
            return
        ln = min(read_set_length(h, s, k, genome_size), (1 << 63) - 1)
        if read_info is not None:
            read_info.append((m[0], ln, float(c.mean()) if len(c) else 0.0))
        names.append(m[0])
        comments.append(m[1])
        lengths.append(ln)
        hashes.append(h)

    for p in paths:
        if reads:
            it = iter_seq_batches(p, batch_bases)
            ss = next(it)
            second = next(it, None)
            if second is not None:       # larger than one batch: the pending files first, to keep the order
                flush()
                head = [ss, second]
                ss = second = None
                stream(p, head, it)
                continue
        else:
            ss = read_seqs([p])
        if individual:
            for i in range(ss.n):
                L = int(ss.lengths[i])
                if L < k:
                    _warn(f"Skipping sequence {ss.names[i]!r} of {p}: shorter than the k-mer size ({L} < {k}).")
                    continue
                if bases and (bases + L > batch_bases or len(meta) >= max_refs):
                    flush()
                group_of.append(len(meta))
                meta.append((ss.names[i], ss.comments[i], L))
                recs.append((ss.names[i], ss.comments[i], ss.seq(i)))
                bases += L
            continue
        m = file_meta(str(p), ss.names, ss.comments, ss.lengths, k)
        if m is None:
            _warn(f"Skipping {p}: no sequence of at least {k} bases.")
            continue
        if bases and (bases + ss.total_bases > batch_bases or len(meta) >= max_refs):
            flush()
        for i in range(ss.n):
            group_of.append(len(meta))
            recs.append((ss.names[i], ss.comments[i], ss.seq(i)))
        meta.append(m)
        bases += ss.total_bases
    flush()
    off = np.zeros(len(hashes) + 1, np.int64)
    if hashes:
        off[1:] = np.cumsum([len(h) for h in hashes])
    return SketchDB(k=int(k), seed=int(seed), sketch_size=int(s), alphabet="ACGT", preserve_case=bool(preserve_case),
                    noncanonical=False, names=names, comments=comments, lengths=np.asarray(lengths, np.int64),
                    offsets=off, hashes=np.concatenate(hashes) if hashes else np.zeros(0, np.uint64))
