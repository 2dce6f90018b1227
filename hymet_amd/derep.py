"""Dereplication of a sketch DB on the MI355X: single-linkage clusters of its sketches under a
Mash distance threshold, one representative per cluster, and the reduced DB (the answer `dist`
only prepares: finding redundant strains before a DB is written).

Device work (libhymet_gpu.so, csrc/mash_dist.hip): `hymet_mash_dist_tri` computes the lower
triangle of the DB against itself (every pair once), `hymet_mash_link` applies `dist -d`'s filter
to it and unites each passing pair in a union-find that stays in HBM -- no edge list is built --
and `hymet_mash_labels` names every sketch's cluster by its smallest member.  Host work here:
blocking, the choice of representatives, the reduced DB and the text.  With sparse=True the
links come from `hymet_mash_dist_sparse` (the pairs that share a hash only) and are united by
`hymet_mash_link_edges`; the clusters are the same.

`cluster_greedy` is the other answer (`derep --greedy`): greedy representatives in priority
order, every member within the threshold of its own representative and no two representatives
within it of each other.  The DB is uploaded in priority order (`permute_db`), so that row q of
the triangle holds q's higher-priority neighbours; `hymet_mash_greedy` (a dense block) and
`hymet_mash_greedy_edges` (the sparse path's CSR) choose the representatives in rounds on the
device (DESIGN.md §3 "Greedy derep").

`triangle_lines` prints the triangle itself in the format of Mash's `triangle` command as
remembered; like the rest of dist it is PARITY-UNPINNED (mashdist.py): no Mash binary is
available to check it against.
"""
from __future__ import annotations

from typing import Iterator, List, NamedTuple, Sequence

import numpy as np

from . import mashdist as md
from .msh import SketchDB


class ClusterResult(NamedTuple):
    labels: np.ndarray     # int32 [n]: the smallest index of each sketch's cluster
    n_links: int           # pairs r < q within the threshold


class GreedyResult(NamedTuple):
    rep: np.ndarray        # int32 [n], DB indices: rep[i] == i for a representative, else i's representative
    n_links: int           # pairs within the threshold
    rounds: tuple          # rounds the device ran per row range, in range order


def _block_rows(n: int, block_bytes: int) -> int:
    """Rows per block, as dist_blocks sizes them."""
    return max(1, int(block_bytes) // (4 * max(n, 1)))


def cluster(gpu, db: SketchDB, max_dist: float, block_bytes: int = 1 << 30, sparse: bool = False,
            plan: list = None) -> ClusterResult:
    """Single-linkage clusters of db's sketches: two sketches share a cluster when a chain of
    pairs with distance() <= max_dist joins them.  0 <= max_dist < 1.  The DB is uploaded once;
    per block of rows the triangle kernel and the link kernel are queued on one stream with
    nothing copied back in between; the labels and the link count come back once, at the end.
    The result does not depend on block_bytes.
    sparse: the same result from the pairs that share a hash only -- hymet_mash_dist_sparse in
    tri mode per row range (mashdist.sparse_ranges: halved on an emission overflow, the dense
    kernels for a range no larger than a dense block that still overflows), its CSR united on the
    device by hymet_mash_link_edges.  plan, when given, receives (path, q0, q1, counters) per
    range."""
    if not 0.0 <= max_dist < 1.0:          # also refuses NaN
        raise ValueError(f"cluster: max_dist {max_dist} outside [0, 1)")
    s = md.check_compatible(db, db, warn=False)
    from ._lib import ptr
    torch = gpu.torch
    dev = md.DeviceSketches(gpu, db)
    n = dev.n
    table = torch.from_numpy(md.min_common_table(s, db.k, max_dist).view(np.int16).copy()).to(gpu.dev)
    parent = torch.arange(max(n, 1), dtype=torch.int32, device=gpu.dev)
    label = gpu.empty(max(n, 1), torch.int32)
    n_links = gpu.zeros(1, torch.int64)
    rows = _block_rows(n, block_bytes)
    if sparse:
        cmin = md.candidate_min_common(md.min_common_table(s, db.k, max_dist))
        max_pairs = max(0, int(block_bytes) // 16)
        for path, q0, q1, got in md.sparse_ranges(n, rows, lambda a, b: md.sparse_block(gpu, dev, dev, a, b, s, table, cmin,
                                                                                        max_pairs, tri=True)):
            if plan is not None:
                plan.append((path, q0, q1, got[4] if got else None))
            if path == "dense":
                block = gpu.empty(max(1, (q1 - q0) * n), torch.int32)
                gpu.call("hymet_mash_dist_tri", ptr(dev.hashes), dev.n_hashes, ptr(dev.offsets), n, q0, q1, s, ptr(block))
                gpu.call("hymet_mash_link", ptr(block), q1 - q0, n, q0, ptr(table), s, ptr(parent), ptr(n_links))
            else:
                gpu.call("hymet_mash_link_edges", ptr(got[0]), q1 - q0, q0, ptr(got[1]), ptr(parent), ptr(n_links))
        gpu.call("hymet_mash_labels", ptr(parent), n, ptr(label))
        return ClusterResult(label[:n].cpu().numpy().astype(np.int32), int(n_links.cpu().item()))
    block = gpu.empty(max(1, min(rows, n) * n), torch.int32)
    for q0 in range(0, n, rows):
        q1 = min(n, q0 + rows)
        gpu.call("hymet_mash_dist_tri", ptr(dev.hashes), dev.n_hashes, ptr(dev.offsets), n, q0, q1, s, ptr(block))
        gpu.call("hymet_mash_link", ptr(block), q1 - q0, n, q0, ptr(table), s, ptr(parent), ptr(n_links))
    gpu.call("hymet_mash_labels", ptr(parent), n, ptr(label))
    return ClusterResult(label[:n].cpu().numpy().astype(np.int32), int(n_links.cpu().item()))


def priority_order(lengths, n: int, rule: str = "longest") -> np.ndarray:
    """The DB indices of n sketches in the order the greedy walk takes them.  longest: recorded
    genome length descending, ties by DB index ascending; first: DB index."""
    if rule not in ("longest", "first"):
        raise ValueError(f"priority_order: unknown rule {rule!r}")
    if rule == "first":
        return np.arange(n, dtype=np.int64)
    lengths = np.asarray(lengths, np.int64)[:n]
    if len(lengths) != n:
        raise ValueError("priority_order: fewer lengths than sketches")
    return np.lexsort((np.arange(n), -lengths)).astype(np.int64)


def permute_db(db: SketchDB, order: Sequence[int]) -> SketchDB:
    """db with its references in the order `order` (a permutation of its indices): entry i of the
    result is reference order[i] (names, comments, lengths, hashes gathered, offsets rebuilt)."""
    order = np.asarray(order, np.int64)
    n = db.n_refs
    if len(order) != n or not np.array_equal(np.sort(order), np.arange(n)):
        raise ValueError("permute_db: order is not a permutation of the DB's indices")
    offs = np.asarray(db.offsets, np.int64)
    off = np.zeros(n + 1, np.int64)
    off[1:] = np.cumsum(offs[order + 1] - offs[order])
    hashes = np.asarray(db.hashes, np.uint64)
    parts = [hashes[int(offs[i]):int(offs[i + 1])] for i in order]
    comments = list(db.comments) + [""] * (n - len(db.comments))
    return SketchDB(k=db.k, seed=db.seed, sketch_size=db.sketch_size, alphabet=db.alphabet, preserve_case=db.preserve_case,
                    noncanonical=db.noncanonical, window_size=db.window_size, names=[db.names[int(i)] for i in order],
                    comments=[comments[int(i)] for i in order], lengths=np.asarray(db.lengths, np.int64)[:n][order],
                    offsets=off, hashes=np.concatenate(parts) if parts else np.zeros(0, np.uint64))


def cluster_greedy(gpu, db: SketchDB, max_dist: float, rule: str = "longest", block_bytes: int = 1 << 30,
                   sparse: bool = False, plan: list = None) -> GreedyResult:
    """Greedy dereplication: walking the sketches in priority order (priority_order), a sketch is
    a representative iff no earlier representative lies within max_dist of it (the pairs that pass
    are cluster()'s links), else a member of the nearest of the earlier representatives within
    max_dist -- nearest by the exact rational common / denom, equal ones to the earlier in
    priority order.  So every member lies within max_dist of its representative and no two
    representatives within it of each other.  0 <= max_dist < 1.  Blocking, sparse and plan are
    cluster()'s; the triangle (or its CSR) of a row range stays on the device while
    hymet_mash_greedy (hymet_mash_greedy_edges) runs its rounds over it, and the result comes
    back once, at the end.  It depends neither on block_bytes nor on sparse."""
    if not 0.0 <= max_dist < 1.0:          # also refuses NaN
        raise ValueError(f"cluster_greedy: max_dist {max_dist} outside [0, 1)")
    s = md.check_compatible(db, db, warn=False)
    order = priority_order(db.lengths, db.n_refs, rule)
    import ctypes
    from ._lib import ptr
    torch = gpu.torch
    # the gather is a copy of every hash on the host: skipped when the priority order is the DB's
    dev = md.DeviceSketches(gpu, db if np.array_equal(order, np.arange(db.n_refs)) else permute_db(db, order))
    n = dev.n
    host_table = md.min_common_table(s, db.k, max_dist)
    table = torch.from_numpy(host_table.view(np.int16).copy()).to(gpu.dev)
    rep = torch.full((max(n, 1),), -1, dtype=torch.int32, device=gpu.dev)
    n_links = gpu.zeros(1, torch.int64)
    rows = _block_rows(n, block_bytes)
    rounds, r = [], ctypes.c_int32()
    block = None

    def dense_range(q0, q1):
        nonlocal block
        if block is None:
            block = gpu.empty(max(1, min(rows, n) * n), torch.int32)
        gpu.call("hymet_mash_dist_tri", ptr(dev.hashes), dev.n_hashes, ptr(dev.offsets), n, q0, q1, s, ptr(block))
        gpu.call("hymet_mash_greedy", ptr(block), q1 - q0, n, q0, ptr(table), s, ptr(rep), ptr(n_links), ctypes.byref(r))
        rounds.append(int(r.value))

    if sparse:
        cmin = md.candidate_min_common(host_table)
        max_pairs = max(0, int(block_bytes) // 16)
        for path, q0, q1, got in md.sparse_ranges(n, rows, lambda a, b: md.sparse_block(gpu, dev, dev, a, b, s, table, cmin,
                                                                                        max_pairs, tri=True)):
            if plan is not None:
                plan.append((path, q0, q1, got[4] if got else None))
            if path == "dense":
                dense_range(q0, q1)
            else:
                gpu.call("hymet_mash_greedy_edges", ptr(got[0]), q1 - q0, q0, ptr(got[1]), ptr(got[2]), s, ptr(rep),
                         ptr(n_links), ctypes.byref(r))
                rounds.append(int(r.value))
    else:
        for q0 in range(0, n, rows):
            dense_range(q0, min(n, q0 + rows))
    dev_rep = rep[:n].cpu().numpy().astype(np.int64)     # in priority order
    out = np.empty(n, np.int32)
    out[order] = order[dev_rep]
    return GreedyResult(out, int(n_links.cpu().item()), tuple(rounds))


def greedy_labels(rep) -> np.ndarray:
    """format_rows' labels of a greedy result: the smallest DB index of each sketch's cluster (a
    cluster is a representative and its members)."""
    rep = np.asarray(rep, np.int64)
    if len(rep) and not np.array_equal(rep[rep], rep):
        raise ValueError("greedy_labels: a representative's entry is not its own index")
    low = np.full(len(rep), len(rep), np.int64)
    np.minimum.at(low, rep, np.arange(len(rep)))
    return low[rep].astype(np.int32)


def greedy_representatives(rep) -> np.ndarray:
    """The representatives of a greedy result, one per cluster in format_rows' cluster order."""
    rep = np.asarray(rep, np.int64)
    labels = greedy_labels(rep)
    roots = np.unique(labels)              # the cluster order: by smallest member
    return rep[roots]


def representatives(labels, lengths, rule: str = "longest") -> np.ndarray:
    """One index per cluster, clusters numbered by their smallest member in DB order.
    longest: the member with the greatest recorded genome length, ties to the smallest index;
    first: the smallest index."""
    if rule not in ("longest", "first"):
        raise ValueError(f"representatives: unknown rule {rule!r}")
    labels = np.asarray(labels, np.int64)
    roots = np.unique(labels)              # a label is its cluster's smallest member
    if rule == "first" or len(labels) == 0:
        return roots
    lengths = np.asarray(lengths, np.int64)[:len(labels)]
    # per cluster the first index of the greatest length: sort by (label, -length, index)
    order = np.lexsort((np.arange(len(labels)), -lengths, labels))
    first = np.r_[True, labels[order][1:] != labels[order][:-1]]
    return order[first].astype(np.int64)


def subset_db(db: SketchDB, keep: Sequence[int]) -> SketchDB:
    """The references `keep` of db, in DB order, as a SketchDB of their own (names, comments,
    lengths, hashes and rebuilt offsets: what msh.write_msh needs)."""
    keep = np.unique(np.asarray(keep, np.int64))
    if len(keep) and (keep[0] < 0 or keep[-1] >= db.n_refs):
        raise ValueError("subset_db: index outside the DB")
    offs = np.asarray(db.offsets, np.int64)
    lens = offs[keep + 1] - offs[keep]
    off = np.zeros(len(keep) + 1, np.int64)
    off[1:] = np.cumsum(lens)
    hashes = np.asarray(db.hashes, np.uint64)
    parts = [hashes[int(offs[i]):int(offs[i + 1])] for i in keep]
    comments = list(db.comments) + [""] * (db.n_refs - len(db.comments))
    return SketchDB(k=db.k, seed=db.seed, sketch_size=db.sketch_size, alphabet=db.alphabet, preserve_case=db.preserve_case,
                    noncanonical=db.noncanonical, window_size=db.window_size, names=[db.names[int(i)] for i in keep],
                    comments=[comments[int(i)] for i in keep], lengths=np.asarray(db.lengths, np.int64)[keep], offsets=off,
                    hashes=np.concatenate(parts) if parts else np.zeros(0, np.uint64))


def format_rows(db: SketchDB, labels, reps) -> List[str]:
    """One row per sketch in DB order: member, representative, cluster index (clusters numbered
    by their smallest member in DB order), cluster size; tab separated."""
    labels = np.asarray(labels, np.int64)
    roots, index, size = np.unique(labels, return_inverse=True, return_counts=True)
    reps = np.asarray(reps, np.int64)
    if len(reps) != len(roots) or not np.array_equal(labels[reps], roots):
        raise ValueError("format_rows: reps is not one member per cluster in cluster order")
    return ["%s\t%s\t%d\t%d" % (db.names[i], db.names[int(reps[c])], c, size[c]) for i, c in enumerate(index)]


def triangle_blocks(gpu, db: SketchDB, block_bytes: int = 1 << 26) -> Iterator[tuple]:
    """(q0, q1, common, denom) per block of rows; common and denom are (q1 - q0) x n int32 whose
    entries r < q are the pair's; the others are 0."""
    s = md.check_compatible(db, db, warn=False)
    from ._lib import ptr
    torch = gpu.torch
    dev = md.DeviceSketches(gpu, db)
    n = dev.n
    rows = _block_rows(n, block_bytes)
    for q0 in range(0, n, rows):
        q1 = min(n, q0 + rows)
        block = gpu.zeros(max(1, (q1 - q0) * n), torch.int32)
        gpu.call("hymet_mash_dist_tri", ptr(dev.hashes), dev.n_hashes, ptr(dev.offsets), n, q0, q1, s, ptr(block))
        gpu.sync()
        v = block[:(q1 - q0) * n].cpu().numpy().view(np.uint32).reshape(q1 - q0, n)
        yield q0, q1, (v >> 16).astype(np.int32), (v & 0xFFFF).astype(np.int32)


def triangle_lines(gpu, db: SketchDB, block_bytes: int = 1 << 26) -> Iterator[str]:
    """`mash triangle` (PARITY-UNPINNED): a first line `\\t<n>`, then per sketch its name and the
    distance (%g, mashdist.distance) to every earlier sketch."""
    yield "\t%d" % db.n_refs
    for q0, q1, common, denom in triangle_blocks(gpu, db, block_bytes):
        for q in range(q0, q1):
            d = np.atleast_1d(md.distance(common[q - q0, :q], denom[q - q0, :q], db.k))
            yield "\t".join([str(db.names[q])] + ["%g" % x for x in d])
