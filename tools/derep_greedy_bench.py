#!/usr/bin/env python3
"""Timing of the greedy dereplication (hymet_amd/derep.py cluster_greedy; csrc/mash_dist.hip
hymet_mash_greedy, hymet_mash_greedy_edges) beside the single-linkage one on the seeded synthetic
DB of tools/derep_bench.py, nothing read from outside the tree: 20,000 sketches of size 1,000,
D = 0.05; a tenth of the sketches come in families that share most of their hashes, the rest are
unrelated.  All recorded lengths are equal, so the priority order is the DB order.

Legs, alternating in one process with their order rotated every repeat, each timed with device
events around work that ends in a synchronisation, after a warm-up round in which they are checked
(the two greedy legs give one result, it counts cluster()'s links, every member passes with its
representative's cluster -- shares cluster()'s label with it -- and the representatives are no
fewer than the clusters):

    a   derep.cluster(): single linkage, dense
    b   derep.cluster(sparse=True)
    c   derep.cluster_greedy(): dense
    d   derep.cluster_greedy(sparse=True)
    c1, c16   leg c with HYMET_GREEDY_BATCH = 1 and 16 (rounds queued per read of the undecided
        count; the library's default is leg c's)
    e   leg c under a seeded permutation as the priority order (distinct recorded lengths): the
        host gathers the hash lists into that order before the upload (derep.permute_db)

It reports every repeat, the median and the spread (min..max) per leg, the stage times of one
profiled call per leg (the library's event pairs), the rounds per row range and the number of
representatives against the number of single-linkage clusters.

    python tools/derep_greedy_bench.py [--reps 5] [--scale 1.0] [--json OUT]
"""
import argparse
import dataclasses
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


def with_batch(value, fn):
    """fn() with HYMET_GREEDY_BATCH set to value (None: unset, the library's default); the
    library reads the variable at every call."""
    def run(*args):
        old = os.environ.pop("HYMET_GREEDY_BATCH", None)
        if value is not None:
            os.environ["HYMET_GREEDY_BATCH"] = str(value)
        try:
            return fn(*args)
        finally:
            os.environ.pop("HYMET_GREEDY_BATCH", None)
            if old is not None:
                os.environ["HYMET_GREEDY_BATCH"] = old
    return run


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the sketches (quick runs)")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    from hymet_amd import derep as dr
    from hymet_amd._lib import Gpu
    gpu = Gpu(int(os.environ.get("HYMET_DEVICE", "0")))
    n = max(20, int(N * a.scale))
    rng = np.random.default_rng(4321)
    fams = rng.integers(0, 2 ** 64, size=(max(1, n // 100), S), dtype=np.uint64)
    db = make_db(rng, n, S, fams)
    assert K == db.k
    print(f"{n} sketches, s={S}, D={D}", flush=True)
    shuffled = dataclasses.replace(db, lengths=np.random.default_rng(99).permutation(n).astype(np.int64) + 1_000_000)
    plans = {"b": [], "d": []}

    def sparse_leg(name, fn):
        def run():
            plans[name].clear()
            return fn(plans[name])
        return run

    def greedy():
        return dr.cluster_greedy(gpu, db, D, block_bytes=BLOCK_BYTES)

    legs = {"a": lambda: dr.cluster(gpu, db, D, BLOCK_BYTES),
            "b": sparse_leg("b", lambda plan: dr.cluster(gpu, db, D, BLOCK_BYTES, sparse=True, plan=plan)),
            "c": with_batch(None, greedy),
            "d": sparse_leg("d", with_batch(None, lambda plan: dr.cluster_greedy(gpu, db, D, block_bytes=BLOCK_BYTES, sparse=True,
                                                                                 plan=plan))),
            "c1": with_batch(1, greedy), "c16": with_batch(16, greedy),
            "e": with_batch(None, lambda: dr.cluster_greedy(gpu, shuffled, D, block_bytes=BLOCK_BYTES))}
    order = sorted(legs)
    ms = {l: [] for l in order}
    seen, info = {}, {}
    for rep in range(a.reps + 1):        # round 0 warms up (allocator, code objects) and checks the legs
        for l in order[rep % len(order):] + order[:rep % len(order)]:   # rotate: no leg always follows the same one
            t, out = timed(gpu, legs[l])
            if rep == 0:
                seen[l] = out
                continue
            ms[l].append(t)
            print(f"  rep {rep} leg {l} {t:10.2f} ms", flush=True)
        if rep == 0:
            single, g = seen["a"], seen["c"]
            assert np.array_equal(single.labels, seen["b"].labels) and single.n_links == seen["b"].n_links, "legs a and b differ"
            for l in ("d", "c1", "c16"):
                assert np.array_equal(g.rep, seen[l].rep) and g.n_links == seen[l].n_links, f"legs c and {l} differ"
            assert g.n_links == single.n_links, f"greedy counts {g.n_links} links, single linkage {single.n_links}"
            is_rep = g.rep == np.arange(n)
            for l in ("c", "e"):
                r = seen[l].rep
                assert (r[r] == r).all(), f"leg {l}: a representative's entry is not its own index"
                assert np.array_equal(single.labels[r], single.labels), f"leg {l}: a member outside its representative's cluster"
                assert int((r == np.arange(n)).sum()) >= len(np.unique(single.labels)), f"leg {l}: too few representatives"
            assert seen["e"].n_links == single.n_links
            info = {"links": int(g.n_links), "clusters": int(len(np.unique(single.labels))), "representatives": int(is_rep.sum()),
                    "rounds": {l: list(seen[l].rounds) for l in ("c", "d", "c1", "c16", "e")},
                    "ranges_d": [(p[0], p[1], p[2]) for p in plans["d"]]}
            assert info["representatives"] >= info["clusters"]
            print(f"  {info['links']} links, {info['clusters']} single-linkage clusters, {info['representatives']} greedy "
                  f"representatives; rounds per range: {info['rounds']}", flush=True)
            seen.clear()
    res = {"shape": {"n": n, "s": S, "max_dist": D, "block_bytes": BLOCK_BYTES}, "info": info, "legs": {}}
    for l in order:                      # one profiled call per leg: the stages' own times
        gpu.prof(True)
        gpu.prof_reset()
        legs[l]()
        gpu.sync()
        kern = {k: {"ms": v[0], "launches": v[1]} for k, v in sorted(gpu.prof_table().items())
                if k.startswith(("mash_", "sparse_"))}
        gpu.prof(False)
        v = ms[l]
        res["legs"][l] = {"ms": v, "median": statistics.median(v), "min": min(v), "max": max(v), "stages": kern}
    print(f"{'leg':4s} {'median ms':>10s} {'min':>10s} {'max':>10s}")
    for l in order:
        r = res["legs"][l]
        print(f"{l:4s} {r['median']:10.2f} {r['min']:10.2f} {r['max']:10.2f}")
        for k, kv in r["stages"].items():
            print(f"       {k:22s} {kv['ms']:10.3f} ms in {kv['launches']} scopes")
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
