"""Dist stage: the MI355X replacement for `mash dist`, all-pairs distances between two sketch
databases (finding redundant strains before a DB is written, placing new genomes against a
DB, checking two DB builds against each other).

Device work (libhymet_gpu.so, csrc/mash_dist.hip): `hymet_mash_dist` computes the two exact
integers of every (reference, query) pair -- common and denom of Mash's merge loop over the
s smallest values of the two lists' union -- and `hymet_mash_dist_select` keeps the pairs that
pass a distance threshold.  Host work here: the distance and p-value arithmetic in double
(the one `distance()` below both formats the output and builds the device filter's table, so
the filter agrees exactly with the printed numbers), blocking, and the text.
`hymet_mash_dist_sparse` gives the filtered result of a threshold below 1 from the pairs that
share a hash only (opt-in: sparse_blocks; DESIGN.md §3 Sparse dist).  `hymet_mash_dist_topk` and
`hymet_mash_topk_edges` (csrc/mash_topk.hip) keep the nearest references of every query on the
device (opt-in: dist_blocks(top=K); DESIGN.md §3 Nearest (top-K)).

The semantics restate Mash's `dist` command from memory of its behaviour.  No Mash binary is
available to check them against: they are PARITY-UNPINNED, like the .msh schema (msh.py) and
the sketch metadata (sketch.py).  DESIGN.md §Dist holds the restated merge loop.
"""
from __future__ import annotations

import ctypes
import sys
from typing import Iterator, List, Sequence, Tuple

import numpy as np

from .msh import SketchDB
from .screen import binomial_upper_tail

E_CAPACITY = -3


def distance(common, denom, k: int):
    """Mash distance of pairs with `common` shared hashes out of `denom`: 0 when common == denom
    (0/0 included), 1 when common == 0, else -log(2j / (1 + j)) / k with j = common / denom.
    Arrays in, float64 array out; scalars in, float out -- through the same arithmetic."""
    c = np.asarray(common, np.float64)
    d = np.asarray(denom, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        j = c / d
        dist = -np.log(2.0 * j / (1.0 + j)) / float(k)
    dist = np.where(c == 0, 1.0, dist)
    dist = np.where(c == d, 0.0, dist)
    return float(dist) if dist.ndim == 0 else dist


def p_value(common: int, denom: int, len_ref: int, len_qry: int, k: int, alphabet_size: int = 4) -> float:
    """Mash's p-value of seeing at least `common` of `denom` hashes shared by chance between
    genomes of len_ref and len_qry bases.  A recorded length of 0 gives 1 (this project's
    choice: Mash has no rule for it)."""
    common, denom = int(common), int(denom)
    if common == 0 or len_ref <= 0 or len_qry <= 0:
        return 1.0
    kmer_space = float(alphabet_size) ** int(k)
    px = 1.0 / (1.0 + kmer_space / float(len_ref))
    py = 1.0 / (1.0 + kmer_space / float(len_qry))
    r = px * py / (px + py - px * py)
    return binomial_upper_tail(common - 1, r, denom)


def min_common_table(s: int, k: int, max_dist: float) -> np.ndarray:
    """t[denom], denom in 0..s: the smallest common with distance(common, denom, k) <= max_dist,
    or denom + 1 when there is none (uint16: the device filter keeps common >= t[denom]).
    For max_dist < 1 the pairs that pass are exactly those with common >= t[denom]: common = 0
    has distance 1 and from 1 up the distance falls as common grows.  (For max_dist >= 1 every
    pair of a k >= 2 DB passes and dist_blocks does not filter on the device at all.)"""
    s = int(s)
    if not 1 <= s <= 0xFFFE:
        raise ValueError(f"min_common_table: sketch size {s} outside 1..65534")
    d = np.arange(s + 1, dtype=np.int64)
    if max_dist >= 1.0:
        first = np.where(distance(np.zeros(s + 1), d, k) <= max_dist, 0, d + 1)
        # common = 0 aside, the walk below still finds the smallest passing common
    else:
        first = d + 1
    # bisection over common in 1..denom, all denoms at once: distance(denom, denom) = 0
    lo = np.ones(s + 1, np.int64)
    hi = d.copy()
    ok = (d >= 1) & (distance(d, d, k) <= max_dist)          # false everywhere for max_dist < 0
    while True:
        act = ok & (lo < hi)
        if not act.any():
            break
        mid = (lo + hi) // 2
        passes = distance(mid, d, k) <= max_dist
        hi = np.where(act & passes, mid, hi)
        lo = np.where(act & ~passes, mid + 1, lo)
    t = np.where(ok, np.minimum(first, hi), first)
    if max_dist >= 0.0:
        t[0] = 0                                              # 0/0: distance 0
    return t.astype(np.uint16)


def _warn(msg: str):
    print(f"WARNING: {msg}", file=sys.stderr)


def check_compatible(ref_db: SketchDB, qry_db: SketchDB, warn: bool = True) -> int:
    """The sketch size to compare two DBs at (the smaller of the two; one warning on stderr when
    they differ).  ValueError when k, seed, alphabet or strand rule differ, and for
    noncanonical DBs, which this project does not build (`cli sketch` refuses -n)."""
    if qry_db.k != ref_db.k:
        raise ValueError(f"The query sketch has a kmer size ({qry_db.k}) that does not match the reference ({ref_db.k}).")
    if qry_db.seed != ref_db.seed:
        raise ValueError(f"The query sketch has a hash seed ({qry_db.seed}) that does not match the reference "
                         f"({ref_db.seed}).")
    if qry_db.alphabet != ref_db.alphabet:
        raise ValueError(f"The query sketch has an alphabet ({qry_db.alphabet}) that does not match the reference "
                         f"({ref_db.alphabet}).")
    if bool(qry_db.noncanonical) != bool(ref_db.noncanonical):
        raise ValueError("The query sketch and the reference differ in strand handling (noncanonical).")
    if ref_db.noncanonical:
        raise ValueError("Noncanonical sketches are not supported.")
    s = min(int(ref_db.sketch_size), int(qry_db.sketch_size))
    if s < 1:
        raise ValueError("A sketch database records a sketch size of 0.")
    if warn and ref_db.sketch_size != qry_db.sketch_size:
        _warn(f"The query sketch size ({qry_db.sketch_size}) does not match the reference ({ref_db.sketch_size}); "
              f"comparing at the smaller ({s}).")
    return s


def concat_dbs(dbs: Sequence[SketchDB]) -> SketchDB:
    """Several sketch DBs (already checked against one reference) as one, entries in argument
    order; its sketch size is the smallest of theirs."""
    first = dbs[0]
    if len(dbs) == 1:
        return first
    off = np.zeros(sum(d.n_refs for d in dbs) + 1, np.int64)
    pos = at = 0
    for d in dbs:
        off[at + 1:at + d.n_refs + 1] = np.asarray(d.offsets[1:d.n_refs + 1], np.int64) - int(d.offsets[0]) + pos
        at += d.n_refs
        pos += int(d.offsets[d.n_refs]) - int(d.offsets[0])
    return SketchDB(k=first.k, seed=first.seed, sketch_size=min(int(d.sketch_size) for d in dbs), alphabet=first.alphabet,
                    preserve_case=first.preserve_case, noncanonical=first.noncanonical,
                    names=[n for d in dbs for n in d.names], comments=[c for d in dbs for c in d.comments],
                    lengths=np.concatenate([np.asarray(d.lengths, np.int64)[:d.n_refs] for d in dbs]), offsets=off,
                    hashes=np.concatenate([np.asarray(d.hashes, np.uint64)[int(d.offsets[0]):int(d.offsets[d.n_refs])]
                                           for d in dbs]))


class DeviceSketches:
    """A sketch DB's CSR in HBM."""

    def __init__(self, gpu, db: SketchDB):
        torch = gpu.torch
        self.n = int(db.n_refs)
        off = np.ascontiguousarray(np.asarray(db.offsets, np.int64)[:self.n + 1])
        h = np.ascontiguousarray(np.asarray(db.hashes, np.uint64))
        self.n_hashes = len(h)
        self.hashes = torch.from_numpy(h.view(np.int64).copy()).to(gpu.dev) if len(h) else gpu.zeros(1, torch.int64)
        self.offsets = torch.from_numpy(off.copy()).to(gpu.dev)


def dist_block(gpu, ref: DeviceSketches, qry: DeviceSketches, q_begin: int, q_end: int, s: int):
    """The dense (q_end - q_begin) x ref.n device tensor (int32 bits of common << 16 | denom)."""
    from ._lib import ptr
    torch = gpu.torch
    out = gpu.empty(max(1, (q_end - q_begin) * ref.n), torch.int32)
    gpu.call("hymet_mash_dist", ptr(ref.hashes), ref.n_hashes, ptr(ref.offsets), ref.n, ptr(qry.hashes), qry.n_hashes,
             ptr(qry.offsets), qry.n, int(q_begin), int(q_end), int(s), ptr(out))
    return out


def select_block(gpu, block, n_rows: int, n_ref: int, table, s: int, cap: int = 0):
    """hymet_mash_dist_select over a dense device block: (row_off int64 [n_rows + 1], ref index
    int32, packed value uint32) on the host.  Retries once with the reported total when the
    first capacity was too small."""
    from ._lib import check, ptr
    torch = gpu.torch
    row_off = gpu.empty(n_rows + 1, torch.int64)
    cap = int(cap) if cap > 0 else max(1024, (n_rows * n_ref) // 16)
    total = ctypes.c_int64()
    while True:
        idx = gpu.empty(cap, torch.int32)
        val = gpu.empty(cap, torch.int32)
        rc = gpu.lib.hymet_mash_dist_select(gpu.ctx, ptr(block), n_rows, n_ref, ptr(table), int(s), ptr(row_off), ptr(idx),
                                            ptr(val), cap, ctypes.byref(total))
        if rc == E_CAPACITY and total.value > cap:
            cap = total.value
            continue
        check(rc, "hymet_mash_dist_select")
        break
    gpu.sync()
    n = total.value
    return row_off.cpu().numpy(), idx[:n].cpu().numpy(), val[:n].cpu().numpy().view(np.uint32)


def topk_max() -> int:
    """The largest `top` (hymet_mash_topk_max)."""
    from ._lib import load
    return int(load().hymet_mash_topk_max())


def _topk_host(gpu, n_rows: int, top: int, idx, val, cnt):
    """The device result of a top-K call as host CSR arrays: (row_off int64 [n_rows + 1],
    reference index int32, packed value uint32), each row nearest first."""
    gpu.sync()
    c = cnt.cpu().numpy()
    written = np.arange(top, dtype=np.int32)[None, :] < c[:, None]
    row_off = np.r_[0, np.cumsum(c, dtype=np.int64)].astype(np.int64)
    return (row_off, idx.cpu().numpy().reshape(n_rows, top)[written],
            val.cpu().numpy().view(np.uint32).reshape(n_rows, top)[written])


def topk_block(gpu, block, n_rows: int, n_ref: int, table, s: int, top: int):
    """hymet_mash_dist_topk over a dense device block: per row the `top` nearest references
    among those that pass `table` (a device min_common_table; None: among all), nearest first
    (the order stands at hymet_mash_dist_topk in include/hymet_gpu.h), as host CSR arrays."""
    from ._lib import ptr
    torch = gpu.torch
    idx = gpu.empty(max(1, n_rows * top), torch.int32)
    val = gpu.empty(max(1, n_rows * top), torch.int32)
    cnt = gpu.empty(max(1, n_rows), torch.int32)
    gpu.call("hymet_mash_dist_topk", ptr(block), int(n_rows), int(n_ref), ptr(table) if table is not None else None, int(s),
             int(top), ptr(idx), ptr(val), ptr(cnt))
    return _topk_host(gpu, n_rows, top, idx[:n_rows * top], val[:n_rows * top], cnt[:n_rows])


def topk_edges(gpu, row_off, n_rows: int, ref_idx, val_in, s: int, top: int):
    """hymet_mash_topk_edges over a device CSR (as select_block's call or sparse_block leaves it
    on the device): per row its `top` nearest entries, nearest first, as host CSR arrays."""
    from ._lib import ptr
    torch = gpu.torch
    idx = gpu.empty(max(1, n_rows * top), torch.int32)
    val = gpu.empty(max(1, n_rows * top), torch.int32)
    cnt = gpu.empty(max(1, n_rows), torch.int32)
    gpu.call("hymet_mash_topk_edges", ptr(row_off), int(n_rows), ptr(ref_idx), ptr(val_in), int(s), int(top), ptr(idx),
             ptr(val), ptr(cnt))
    return _topk_host(gpu, n_rows, top, idx[:n_rows * top], val[:n_rows * top], cnt[:n_rows])


def candidate_min_common(table) -> int:
    """cmin of the sparse path: the fewest shared hashes a pair that passes `table`
    (min_common_table) can have, the smallest t[denom] over denom >= 1.  At least 1 for
    max_dist < 1, where common = 0 never passes; a pair of two empty sketches (denom 0) shares
    nothing and is handled on its own (hymet_mash_dist_sparse)."""
    t = np.asarray(table).astype(np.int64)
    if len(t) < 2:
        raise ValueError("candidate_min_common: the table has no denom >= 1")
    return int(t[1:].min())


def sparse_ranges(q_end: int, rows: int, attempt, q_begin: int = 0):
    """The blocking policy of the sparse path, shared by sparse_blocks and derep.cluster: the row
    ranges in ascending order, starting with the whole of [q_begin, q_end).  attempt(q0, q1)
    returns None on an emission overflow; the range is then halved, and a range of at most
    `rows` rows (the dense path's block) is handed out as ("dense", q0, q1, None) instead.
    Yields ("sparse", q0, q1, what attempt returned) otherwise."""
    todo = [(q_begin, q_end)]
    while todo:
        q0, q1 = todo.pop()
        if q1 <= q0:
            continue
        got = attempt(q0, q1)
        if got is not None:
            yield "sparse", q0, q1, got
        elif q1 - q0 <= rows:
            yield "dense", q0, q1, None
        else:
            mid = (q0 + q1) // 2
            todo += [(mid, q1), (q0, mid)]


def sparse_block(gpu, ref: DeviceSketches, qry: DeviceSketches, q_begin: int, q_end: int, s: int, table, cmin: int,
                 max_pairs: int, tri: bool = False, cap: int = 0):
    """One hymet_mash_dist_sparse call over the rows [q_begin, q_end): (row_off int64
    [rows + 1], ref index int32, packed value int32, total, counters) with the arrays on the
    device, or None when the range emits more than max_pairs pair keys.  Retries once with the
    reported total when the first capacity was too small."""
    from ._lib import SparseCounters, check, ptr
    torch = gpu.torch
    rows = q_end - q_begin
    row_off = gpu.empty(rows + 1, torch.int64)
    cap = int(cap) if cap > 0 else max(1024, min(int(max_pairs), rows * max(ref.n, 1)) // 16)
    total, ctr = ctypes.c_int64(), SparseCounters()
    while True:
        idx = gpu.empty(cap, torch.int32)
        val = gpu.empty(cap, torch.int32)
        rc = gpu.lib.hymet_mash_dist_sparse(gpu.ctx, ptr(ref.hashes), ref.n_hashes, ptr(ref.offsets), ref.n, ptr(qry.hashes),
                                            qry.n_hashes, ptr(qry.offsets), qry.n, int(q_begin), int(q_end), int(s),
                                            int(bool(tri)), ptr(table), int(cmin), int(max_pairs), ptr(row_off), ptr(idx),
                                            ptr(val), cap, ctypes.byref(total), ctypes.byref(ctr))
        if rc == E_CAPACITY and total.value == -1:
            return None
        if rc == E_CAPACITY and total.value > cap:
            cap = total.value
            continue
        check(rc, "hymet_mash_dist_sparse")
        break
    return row_off, idx, val, total.value, (ctr.postings, ctr.emitted, ctr.candidates)


def sparse_blocks(gpu, ref_db: SketchDB, qry_db: SketchDB, max_dist: float, block_bytes: int = 1 << 30,
                  plan: list = None) -> Iterator[Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]]:
    """What dist_blocks yields for max_dist < 1 (ValueError otherwise), from the pairs that share
    a hash only (hymet_mash_dist_sparse): exact, since a pair that shares none has distance 1.
    A call may emit block_bytes // 16 pair keys; the whole query range is tried first, a range
    that emits more is halved, and one no larger than dist_blocks' block that still does takes
    the dense kernels.  The concatenated result depends neither on block_bytes nor on which
    ranges fell back.  plan, when given, receives (path, q0, q1, counters) per range, path
    "sparse" or "dense", counters (postings, emitted, candidates) or None."""
    if not max_dist < 1.0:
        raise ValueError(f"sparse_blocks: max_dist {max_dist} is not below 1")
    s = check_compatible(ref_db, qry_db, warn=False)
    torch = gpu.torch
    ref, qry = DeviceSketches(gpu, ref_db), DeviceSketches(gpu, qry_db)
    n_ref = ref.n
    rows = max(1, int(block_bytes) // (4 * max(n_ref, 1)))
    max_pairs = max(0, int(block_bytes) // 16)
    host_table = min_common_table(s, ref_db.k, max_dist)
    cmin = candidate_min_common(host_table)
    table = torch.from_numpy(host_table.view(np.int16).copy()).to(gpu.dev)
    for path, q0, q1, got in sparse_ranges(qry.n, rows, lambda a, b: sparse_block(gpu, ref, qry, a, b, s, table, cmin,
                                                                                  max_pairs)):
        if plan is not None:
            plan.append((path, q0, q1, got[4] if got else None))
        if n_ref == 0:
            z = np.zeros(0, np.int32)
            yield z, z, z, z
            continue
        if path == "dense":
            row_off, ri, v = select_block(gpu, dist_block(gpu, ref, qry, q0, q1, s), q1 - q0, n_ref, table, s)
        else:
            d_off, d_idx, d_val, n, _ = got
            row_off, ri, v = d_off.cpu().numpy(), d_idx[:n].cpu().numpy(), d_val[:n].cpu().numpy().view(np.uint32)
        qi = np.repeat(np.arange(q0, q1, dtype=np.int32), np.diff(row_off))
        yield qi, ri, (v >> 16).astype(np.int32), (v & 0xFFFF).astype(np.int32)


def top_blocks(gpu, ref_db: SketchDB, qry_db: SketchDB, top: int, max_dist: float = 1.0, block_bytes: int = 1 << 30,
               sparse: bool = False) -> Iterator[Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]]:
    """dist_blocks(top=...): per query at most `top` references, nearest first (the order stands
    at hymet_mash_dist_topk in include/hymet_gpu.h), among those with distance() <= max_dist.
    The selection runs on the device over the dense block (the threshold's table fused into it)
    or, sparse, over the CSR of each range of the sparse path; neither the dense block nor the
    unselected pairs reach the host.  ValueError for a `top` outside 1..topk_max()."""
    top = int(top)
    if not 1 <= top <= topk_max():
        raise ValueError(f"top {top} outside 1..{topk_max()}")
    if sparse and not max_dist < 1.0:
        raise ValueError(f"sparse_blocks: max_dist {max_dist} is not below 1")
    s = check_compatible(ref_db, qry_db, warn=False)
    torch = gpu.torch
    ref, qry = DeviceSketches(gpu, ref_db), DeviceSketches(gpu, qry_db)
    n_ref = ref.n
    rows = max(1, int(block_bytes) // (4 * max(n_ref, 1)))
    table = None
    if max_dist < 1.0:
        host_table = min_common_table(s, ref_db.k, max_dist)
        table = torch.from_numpy(host_table.view(np.int16).copy()).to(gpu.dev)
    if sparse:
        cmin, max_pairs = candidate_min_common(host_table), max(0, int(block_bytes) // 16)
        ranges = sparse_ranges(qry.n, rows, lambda a, b: sparse_block(gpu, ref, qry, a, b, s, table, cmin, max_pairs))
    else:
        ranges = (("dense", q0, min(qry.n, q0 + rows), None) for q0 in range(0, qry.n, rows))
    for path, q0, q1, got in ranges:
        if n_ref == 0:
            z = np.zeros(0, np.int32)
            yield z, z, z, z
            continue
        if path == "dense":
            row_off, ri, v = topk_block(gpu, dist_block(gpu, ref, qry, q0, q1, s), q1 - q0, n_ref, table, s, top)
        else:
            row_off, ri, v = topk_edges(gpu, got[0], q1 - q0, got[1], got[2], s, top)
        qi = np.repeat(np.arange(q0, q1, dtype=np.int32), np.diff(row_off))
        yield qi, ri, (v >> 16).astype(np.int32), (v & 0xFFFF).astype(np.int32)


def dist_blocks(gpu, ref_db: SketchDB, qry_db: SketchDB, max_dist: float = 1.0, block_bytes: int = 1 << 30,
                sparse: bool = False, top: int = 0) -> Iterator[Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]]:
    """`mash dist` of two DBs on the device: yields (q_index, r_index, common, denom) int32
    arrays, query-major (for each query in DB order, the references in DB order), one tuple per
    block of queries.  Both DBs are uploaded once; a block holds as many queries as keep the
    dense result within block_bytes, and the concatenated result does not depend on it.
    max_dist >= 1: every pair; below, the pairs with distance() <= max_dist, filtered on the
    device (min_common_table).  sparse: the same result through sparse_blocks (max_dist < 1).
    top > 0: per query only the `top` nearest of those references, nearest first (top_blocks)."""
    if top:
        yield from top_blocks(gpu, ref_db, qry_db, top, max_dist, block_bytes, sparse)
        return
    if sparse:
        yield from sparse_blocks(gpu, ref_db, qry_db, max_dist, block_bytes)
        return
    s = check_compatible(ref_db, qry_db, warn=False)
    torch = gpu.torch
    ref, qry = DeviceSketches(gpu, ref_db), DeviceSketches(gpu, qry_db)
    n_ref = ref.n
    rows = max(1, int(block_bytes) // (4 * max(n_ref, 1)))
    table = None
    if max_dist < 1.0:
        table = torch.from_numpy(min_common_table(s, ref_db.k, max_dist).view(np.int16).copy()).to(gpu.dev)
    for q0 in range(0, qry.n, rows):
        q1 = min(qry.n, q0 + rows)
        nq = q1 - q0
        block = dist_block(gpu, ref, qry, q0, q1, s)
        if n_ref == 0:
            z = np.zeros(0, np.int32)
            yield z, z, z, z
            continue
        if table is None:
            gpu.sync()
            v = block[:nq * n_ref].cpu().numpy().view(np.uint32)
            qi = np.repeat(np.arange(q0, q1, dtype=np.int32), n_ref)
            ri = np.tile(np.arange(n_ref, dtype=np.int32), nq)
        else:
            row_off, ri, v = select_block(gpu, block, nq, n_ref, table, s)
            qi = np.repeat(np.arange(q0, q1, dtype=np.int32), np.diff(row_off))
        yield qi, ri, (v >> 16).astype(np.int32), (v & 0xFFFF).astype(np.int32)


def format_lines(ref_db: SketchDB, qry_db: SketchDB, q_index, r_index, common, denom, max_dist: float = 1.0,
                 max_p: float = 1.0) -> List[str]:
    """`mash dist` rows: reference name, query name, distance, p-value, common/denom, tab
    separated, floats as %g (C++ ostream default, as format_screen); pairs with a distance above
    max_dist or a p-value above max_p are dropped."""
    k, asz = ref_db.k, len(ref_db.alphabet) or 4
    dist = np.atleast_1d(distance(common, denom, k))
    out = []
    memo = {}
    for n in range(len(dist)):
        if not dist[n] <= max_dist:
            continue
        q, r, c, d = int(q_index[n]), int(r_index[n]), int(common[n]), int(denom[n])
        key = (c, d, int(ref_db.lengths[r]), int(qry_db.lengths[q]))
        p = memo.get(key)
        if p is None:
            p = memo[key] = p_value(c, d, key[2], key[3], k, asz)
        if p > max_p:
            continue
        out.append("%s\t%s\t%g\t%g\t%d/%d" % (ref_db.names[r], qry_db.names[q], dist[n], p, c, d))
    return out


def format_table(ref_db: SketchDB, qry_db: SketchDB, common, denom) -> List[str]:
    """`mash dist -t`: a header `#query`, the reference names; then one row per query: its name
    and the distance to every reference (%g).  common / denom: n_qry x n_ref, query-major."""
    n_q, n_r = qry_db.n_refs, ref_db.n_refs
    dist = np.atleast_1d(distance(common, denom, ref_db.k)).reshape(n_q, n_r)
    out = ["\t".join(["#query"] + [str(n) for n in ref_db.names])]
    for q in range(n_q):
        out.append("\t".join([str(qry_db.names[q])] + ["%g" % x for x in dist[q]]))
    return out
