#!/usr/bin/env python3
"""Timing of the GPU dereplication (hymet_amd/derep.py, csrc/mash_dist.hip) on one seeded
synthetic DB, nothing read from outside the tree: 20,000 sketches of size 1,000, clustered at
D = 0.05.  A tenth of the sketches come in families that share most of their hashes (the DB of
tools/dist_bench.py); the rest are unrelated.

Legs, alternating in one process with their order rotated every repeat, each timed with device
events around work that ends in a synchronisation, after a warm-up round in which the legs are
checked to agree:

    a   derep.cluster(): hymet_mash_dist_tri + hymet_mash_link per block, one labels call
    b   the same clustering through the full square: hymet_mash_dist of the DB with itself +
        hymet_mash_link per block (what a user had before the triangle).  Labels must be equal.
    c   hymet_mash_link alone over a resident block (the first block of leg a)

It reports every repeat, the median and the spread (min..max) per leg, the ratio a / b against
the pair-count ratio (n - 1) / 2n, the kernels' own times (the library's event pairs) and
leg c's bytes per second at 4 B per triangle pair, and whether a is slower than b beyond the two
legs' spreads.

    python tools/derep_bench.py [--reps 5] [--scale 1.0] [--json OUT]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from dist_bench import K, make_db, timed  # noqa: E402

N, S, D = 20_000, 1_000, 0.05
BLOCK_BYTES = 1 << 30


def cluster_square(gpu, db, max_dist, block_bytes=BLOCK_BYTES):
    """derep.cluster() with hymet_mash_dist (every pair twice and the diagonal) in the place of
    hymet_mash_dist_tri; everything else is the same."""
    from hymet_amd import mashdist as md
    from hymet_amd._lib import ptr
    torch = gpu.torch
    s = md.check_compatible(db, db, warn=False)
    dev = md.DeviceSketches(gpu, db)
    n = dev.n
    table = torch.from_numpy(md.min_common_table(s, db.k, max_dist).view(np.int16).copy()).to(gpu.dev)
    parent = torch.arange(n, dtype=torch.int32, device=gpu.dev)
    label = gpu.empty(n, torch.int32)
    n_links = gpu.zeros(1, torch.int64)
    rows = max(1, int(block_bytes) // (4 * n))
    block = gpu.empty(min(rows, n) * n, torch.int32)
    for q0 in range(0, n, rows):
        q1 = min(n, q0 + rows)
        gpu.call("hymet_mash_dist", ptr(dev.hashes), dev.n_hashes, ptr(dev.offsets), n, ptr(dev.hashes), dev.n_hashes,
                 ptr(dev.offsets), n, q0, q1, s, ptr(block))
        gpu.call("hymet_mash_link", ptr(block), q1 - q0, n, q0, ptr(table), s, ptr(parent), ptr(n_links))
    gpu.call("hymet_mash_labels", ptr(parent), n, ptr(label))
    return label.cpu().numpy(), int(n_links.cpu().item())


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the sketches (quick runs)")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    from hymet_amd import derep as dr
    from hymet_amd import mashdist as md
    from hymet_amd._lib import Gpu, ptr
    gpu = Gpu(int(os.environ.get("HYMET_DEVICE", "0")))
    torch = gpu.torch
    n = max(20, int(N * a.scale))
    rng = np.random.default_rng(4321)
    fams = rng.integers(0, 2 ** 64, size=(max(1, n // 100), S), dtype=np.uint64)
    db = make_db(rng, n, S, fams)
    pairs = n * (n - 1) // 2
    print(f"{n} sketches, s={S}, D={D}: {pairs} pairs in the triangle, {n * n} in the square "
          f"(pair-count ratio {(n - 1) / (2 * n):.4f})", flush=True)

    # leg c's resident block: the first block of leg a
    dev = md.DeviceSketches(gpu, db)
    table = torch.from_numpy(md.min_common_table(S, K, D).view(np.int16).copy()).to(gpu.dev)
    rows = min(n, max(1, BLOCK_BYTES // (4 * n)))
    block = gpu.zeros(rows * n, torch.int32)
    gpu.call("hymet_mash_dist_tri", ptr(dev.hashes), dev.n_hashes, ptr(dev.offsets), n, 0, rows, S, ptr(block))
    gpu.sync()
    c_pairs = rows * (rows - 1) // 2

    def link_alone():
        parent = torch.arange(n, dtype=torch.int32, device=gpu.dev)
        links = gpu.zeros(1, torch.int64)
        gpu.call("hymet_mash_link", ptr(block), rows, n, 0, ptr(table), S, ptr(parent), ptr(links))
        return int(links.cpu().item())

    legs = {"a": lambda: dr.cluster(gpu, db, D, BLOCK_BYTES), "b": lambda: cluster_square(gpu, db, D), "c": link_alone}
    order = sorted(legs)
    ms = {l: [] for l in order}
    seen = {}
    for rep in range(a.reps + 1):        # round 0 warms up (allocator, code objects) and checks the legs agree
        for l in order[rep % len(order):] + order[:rep % len(order)]:   # rotate: no leg always follows the same one
            t, out = timed(gpu, legs[l])
            if rep == 0:
                seen[l] = out
                continue
            ms[l].append(t)
            print(f"  rep {rep} leg {l} {t:10.2f} ms", flush=True)
        if rep == 0:
            la, lb = seen["a"], seen["b"]
            assert np.array_equal(la.labels, lb[0]), "legs a and b give different labels"
            assert la.n_links == lb[1], f"leg a counts {la.n_links} links, leg b {lb[1]}"
            # leg c sees the first block's rows only: some of the links, never more than all
            assert 0 < seen["c"] <= la.n_links, f"leg c counts {seen['c']} links of {la.n_links}"
            print(f"  {la.n_links} links, {len(np.unique(la.labels))} clusters; {seen['c']} links in the first "
                  f"{rows} rows", flush=True)
    kern = {}
    for l in order:                      # one profiled call per leg: the kernels' own times and algorithmic bytes
        gpu.prof(True)
        gpu.prof_reset()
        legs[l]()
        gpu.sync()
        kern[l] = {k: {"kernel_ms": v[0], "launches": v[1], "alg_bytes": v[2],
                       "gb_per_s": v[2] / (v[0] * 1e-3) / 1e9 if v[0] > 0 else 0.0}
                   for k, v in gpu.prof_table().items() if k.startswith("mash_")}
        gpu.prof(False)
    res = {"_shape": {"n": n, "s": S, "max_dist": D, "block_rows": rows, "pairs": pairs, "c_pairs": c_pairs}}
    print(f"{'leg':4s} {'median ms':>10s} {'min':>10s} {'max':>10s}")
    for l in order:
        v = ms[l]
        res[l] = {"ms": v, "median": statistics.median(v), "min": min(v), "max": max(v), "kernels": kern[l]}
        print(f"{l:4s} {res[l]['median']:10.2f} {min(v):10.2f} {max(v):10.2f}")
        for k, kv in kern[l].items():
            print(f"       {k:16s} {kv['kernel_ms']:10.2f} ms in {kv['launches']} launches, {kv['gb_per_s']:8.1f} GB/s algorithmic")
    av, bv, cv = res["a"], res["b"], res["c"]
    spread = (av["max"] - av["min"]) + (bv["max"] - bv["min"])
    res["a_over_b"] = av["median"] / bv["median"]
    res["c_gb_per_s"] = 4.0 * c_pairs / (cv["median"] * 1e-3) / 1e9
    print(f"a / b = {res['a_over_b']:.3f} (pair-count ratio {(n - 1) / (2 * n):.3f})")
    print(f"c: {4.0 * c_pairs / 1e9:.3f} GB at 4 B per triangle pair in {cv['median']:.2f} ms = {res['c_gb_per_s']:.1f} GB/s")
    slower = av["median"] - bv["median"] > spread
    res["a_slower_than_b_beyond_spread"] = bool(slower)
    print(f"a slower than b beyond the two spreads: {'YES' if slower else 'no'} (spreads {spread:.2f} ms)")
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
    return 1 if slower else 0


if __name__ == "__main__":
    sys.exit(main())
