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
