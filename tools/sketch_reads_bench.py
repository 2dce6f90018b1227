#!/usr/bin/env python3
"""Timing of the read-set sketch (hymet_amd/sketch.py sketch_pool_counted, csrc/sketch_counted.hip)
against the plain sketch over the same pool, on two seeded synthetic shapes, nothing read from
outside the tree:

    reads     : N read sets, each 150-base reads of a random genome at ~30x with 1 % substitutions
    singleton : the same number of reads cut from random bases: nearly every k-mer is seen once

Every read set is one sketch.  Four legs alternate in one process, order rotated, each timed with
device events around work that ends in a synchronisation, after a warm-up round that also checks
that (b) returns (a)'s rows:

    a  sketch.sketch_pool               (hymet_sketch_batch: the code as it stood)
    b  sketch.sketch_pool_counted, M = 1
    c  sketch.sketch_pool_counted, M = 2
    d  the hash-only floor: hymet_screen_count with ndb = 0 over the pool

It reports every repeat, the median and the range per leg and the passes (b) and (c) took.
--keep runs (b) and (c) once more per value of hymet_sketch_counted_tune.

    python tools/sketch_reads_bench.py [--shapes reads,singleton] [--sets 4] [--genome 1000000]
                                       [--reps 5] [--keep 1000,11600] [--json OUT]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.sketch_bench import hash_floor, timed  # noqa: E402

READ_LEN, COVERAGE, ERR = 150, 30, 0.01


def make_pool(gpu, shape, n_sets, genome_len, seed):
    """n_sets read sets as one packed pool ('N' between reads) and the reads' set ids."""
    from hymet_amd.seqio import DevicePool, SeqSet
    rng = np.random.default_rng(seed)
    per_set = genome_len * COVERAGE // READ_LEN
    n = n_sets * per_set
    step = READ_LEN + 1
    codes = np.empty((n, step), np.uint8)
    for g in range(n_sets):
        rows = codes[g * per_set:(g + 1) * per_set, :READ_LEN]
        if shape == "reads":
            genome = rng.integers(0, 4, size=genome_len, dtype=np.uint8)
            pos = rng.integers(0, genome_len - READ_LEN + 1, size=per_set)
            rows[:] = genome[pos[:, None] + np.arange(READ_LEN)]
            sub = rng.random(rows.shape) < ERR
            rows[sub] = (rows[sub] + rng.integers(1, 4, size=int(sub.sum()), dtype=np.uint8)) & 3
        else:
            rows[:] = rng.integers(0, 4, size=rows.shape, dtype=np.uint8)
    buf = np.frombuffer(b"ACGTN", np.uint8)[np.where(np.arange(step) == READ_LEN, 4, codes).astype(np.uint8)]
    ss = SeqSet([f"r{i}" for i in range(n)], [""] * n, np.full(n, READ_LEN, np.int64),
                np.arange(n, dtype=np.int64) * step, buf.tobytes()[:-1])
    return DevicePool(gpu, ss, DevicePool.ALPHA_MASH), np.repeat(np.arange(n_sets, dtype=np.int64), per_set)


def run_shape(gpu, name, pool, group_of, reps, k, seed, s, keeps):
    from hymet_amd import sketch as sk
    passes = {}

    def counted(m, keep, tag):
        def fn():
            assert gpu.lib.hymet_sketch_counted_tune(keep) == 0
            try:
                out = sk.sketch_pool_counted(gpu, pool, group_of, k, seed, s, m)
            finally:
                gpu.lib.hymet_sketch_counted_tune(0)
            passes[tag] = sk.sketch_pool_counted.stats["passes"]
            return out
        return fn

    legs = {"a": lambda: sk.sketch_pool(gpu, pool, group_of, k=k, seed=seed, s=s),
            "b": counted(1, 0, "b"), "c": counted(2, 0, "c"), "d": lambda: hash_floor(gpu, pool, k, seed)}
    for kp in keeps:
        legs[f"b_keep{kp}"] = counted(1, kp, f"b_keep{kp}")
        legs[f"c_keep{kp}"] = counted(2, kp, f"c_keep{kp}")
    order = sorted(legs)
    ms = {l: [] for l in order}
    first = {}
    for rep in range(reps + 1):          # round 0 warms up (allocator, code objects) and checks equality
        for l in order[rep % len(order):] + order[:rep % len(order)]:   # rotate: no leg always follows the same one
            t, out = timed(gpu, legs[l])
            if rep == 0:
                first[l] = out
                continue
            ms[l].append(t)
            print(f"  {name} rep {rep} leg {l:12s} {t:10.2f} ms  passes {passes.get(l, '-')}", flush=True)
    for l, out in first.items():
        if l[0] == "b":
            assert all(np.array_equal(x, h) for x, (h, _) in zip(first["a"], out)), f"leg {l} differs from leg a"
        if l[0] == "c":
            assert all(np.array_equal(h, h0) and np.array_equal(c, c0)
                       for (h, c), (h0, c0) in zip(out, first["c"])), f"leg {l} differs from leg c"
    kept = [len(h) for h, _ in first["c"]]
    print(f"  {name}: M = 2 rows hold {min(kept)}..{max(kept)} hashes")
    return {l: {"ms": v, "median": statistics.median(v), "min": min(v), "max": max(v), "passes": passes.get(l)}
            for l, v in ms.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default="reads,singleton")
    ap.add_argument("--sets", type=int, default=4)
    ap.add_argument("--genome", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--keep", default="", help="comma-separated slots per chunk to time beside the default")
    ap.add_argument("-k", type=int, default=21)
    ap.add_argument("-s", type=int, default=1000)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    from hymet_amd._lib import Gpu
    gpu = Gpu(int(os.environ.get("HYMET_DEVICE", "0")))
    keeps = [int(x) for x in a.keep.split(",") if x]
    res = {}
    for name in a.shapes.split(","):
        pool, group_of = make_pool(gpu, name, a.sets, a.genome, 4321)
        print(f"{name}: {a.sets} sets x {len(group_of) // a.sets} reads of {READ_LEN} bases "
              f"({pool.n_bases / 1e6:.1f} Mbases), k={a.k} s={a.s}", flush=True)
        r = res[name] = run_shape(gpu, name, pool, group_of, a.reps, a.k, a.seed, a.s, keeps)
        del pool
        gpu.trim()
        gpu.torch.cuda.empty_cache()
        print(f"{'leg':12s} {'median ms':>10s} {'min':>10s} {'max':>10s} {'passes':>7s} {'/ a':>6s}")
        for l, v in r.items():
            print(f"{l:12s} {v['median']:10.2f} {v['min']:10.2f} {v['max']:10.2f} {str(v['passes'] or '-'):>7s} "
                  f"{v['median'] / r['a']['median']:6.2f}")
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
