#!/usr/bin/env python3
"""Timing of the streamed read-set sketch (csrc/sketch_stream.hip) against the one-batch path
(sketch_pool_counted, csrc/sketch_counted.hip) over the same reads, on the two seeded shapes of
tools/sketch_reads_bench.py (`reads`, `singleton`), nothing read from outside the tree.

Every read set is one sketch, M = 2.  The legs alternate in one process, order rotated, each
timed with device events around work that ends in a synchronisation, after a warm-up round that
checks every (b) leg against (a), hashes and counts:

    a     sketch.sketch_pool_counted over the whole pool (all read sets in one call)
    bN    the stream: one handle per read set, the set's reads fed as N batches (1, 8, 64)

The batches are packed once, before the timing: a (b) leg is the device path -- create, add per
batch, end_pass until the device asks for no more, result -- without the host's reading and
packing, which leg (a) does not pay either.  --slices adds, at 1 batch per read set (where the
slice and not the batch cuts the work), one leg per slice_bases value beside the default.  It
reports every repeat, the median and the range per leg, and per (b) leg the passes, the slices
(both summed over the sets) and the most (hash, count) pairs the window of any set held.

    python tools/sketch_stream_bench.py [--shapes reads,singleton] [--sets 4] [--genome 1000000]
                                        [--reps 5] [--batches 1,8,64] [--slices 1048576,16777216]
                                        [--json OUT]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.sketch_bench import timed  # noqa: E402
from tools.sketch_reads_bench import READ_LEN, make_pool  # noqa: E402


def pack_batches(gpu, ss, n_sets, n_batches):
    """Per read set, its reads as n_batches packed pools (the reads lie READ_LEN + 1 apart)."""
    from hymet_amd.seqio import DevicePool, SeqSet
    per_set = ss.n // n_sets
    step = READ_LEN + 1
    out = []
    for g in range(n_sets):
        cuts = np.linspace(g * per_set, (g + 1) * per_set, n_batches + 1).astype(np.int64)
        pools = []
        for i0, i1 in zip(cuts[:-1].tolist(), cuts[1:].tolist()):
            n = i1 - i0
            part = SeqSet(ss.names[i0:i1], ss.comments[i0:i1], np.full(n, READ_LEN, np.int64),
                          np.arange(n, dtype=np.int64) * step, ss.buf[i0 * step:i1 * step - 1])
            pools.append(DevicePool(gpu, part, DevicePool.ALPHA_MASH))
        out.append(pools)
    return out


def stream_sets(gpu, sets, k, seed, s, m, slice_bases, stats):
    """One handle per read set over its packed batches -> [(hashes, counts)]; stats gets the sums
    of passes and slices and the largest window."""
    from hymet_amd._lib import check, ptr
    from hymet_amd.sketch import DEFAULT_STREAM_MAX_LIVE
    lib, torch = gpu.lib, gpu.torch
    rows = []
    stats.update(passes=0, slices=0, max_live=0)
    for pools in sets:
        h = ctypes.c_void_p()
        check(lib.hymet_sketch_stream_create(gpu.ctx, k, seed, s, m, DEFAULT_STREAM_MAX_LIVE, ctypes.byref(h)), "create")
        try:
            more = ctypes.c_int32(1)
            while more.value:
                for p in pools:
                    check(lib.hymet_sketch_stream_add(h, ptr(p.w2b), ptr(p.wmask), p.n_bases, slice_bases), "add")
                check(lib.hymet_sketch_stream_end_pass(h, ctypes.byref(more)), "end_pass")
            out = gpu.empty(s + (s + 1) // 2, torch.int64)
            n = ctypes.c_int32()
            st = (ctypes.c_int64 * 4)()
            check(lib.hymet_sketch_stream_result(h, ptr(out), ctypes.c_void_p(out.data_ptr() + 8 * s), ctypes.byref(n),
                                                 ctypes.cast(st, ctypes.c_void_p)), "result")
        finally:
            lib.hymet_sketch_stream_destroy(h)
        host = out.cpu().numpy()
        rows.append((host[:s].view(np.uint64)[:n.value], host[s:].view(np.uint32)[:n.value]))
        stats["passes"] += int(st[0])
        stats["slices"] += int(st[1])
        stats["max_live"] = max(stats["max_live"], int(st[3]))
    return rows


def run_shape(gpu, name, pool, group_of, n_sets, reps, k, seed, s, batches, slices):
    from hymet_amd import sketch as sk
    m = 2
    info = {}

    def stream(tag, sets, slice_bases):
        info[tag] = {}
        return lambda: stream_sets(gpu, sets, k, seed, s, m, slice_bases, info[tag])

    def whole():
        out = sk.sketch_pool_counted(gpu, pool, group_of, k, seed, s, m)
        info["a"] = {"passes": sk.sketch_pool_counted.stats["passes"]}
        return out

    legs = {"a": whole}
    packed = {nb: pack_batches(gpu, pool.ss, n_sets, nb) for nb in sorted(set(batches) | ({1} if slices else set()))}
    for nb in batches:
        legs[f"b{nb}"] = stream(f"b{nb}", packed[nb], sk.DEFAULT_STREAM_SLICE_BASES)
    for sl in slices:
        legs[f"b1_slice{sl}"] = stream(f"b1_slice{sl}", packed[1], sl)
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
            print(f"  {name} rep {rep} leg {l:18s} {t:10.2f} ms  {info.get(l)}", flush=True)
    for l, out in first.items():
        assert len(out) == len(first["a"]) and all(
            np.array_equal(h, h0) and np.array_equal(c, c0) for (h, c), (h0, c0) in zip(out, first["a"])), \
            f"leg {l} differs from leg a"
    kept = [len(h) for h, _ in first["a"]]
    print(f"  {name}: M = 2 rows hold {min(kept)}..{max(kept)} hashes; every (b) leg equals (a)")
    return {l: dict(info.get(l, {}), ms=v, median=statistics.median(v), min=min(v), max=max(v)) for l, v in ms.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default="reads,singleton")
    ap.add_argument("--sets", type=int, default=4)
    ap.add_argument("--genome", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batches", default="1,8,64")
    ap.add_argument("--slices", default="", help="comma-separated slice_bases values to time at 1 batch beside the default")
    ap.add_argument("-k", type=int, default=21)
    ap.add_argument("-s", type=int, default=1000)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    from hymet_amd._lib import Gpu
    gpu = Gpu(int(os.environ.get("HYMET_DEVICE", "0")))
    batches = [int(x) for x in a.batches.split(",") if x]
    slices = [int(x) for x in a.slices.split(",") if x]
    res = {}
    for name in a.shapes.split(","):
        pool, group_of = make_pool(gpu, name, a.sets, a.genome, 4321)
        print(f"{name}: {a.sets} sets x {len(group_of) // a.sets} reads of {READ_LEN} bases "
              f"({pool.n_bases / 1e6:.1f} Mbases), k={a.k} s={a.s} M=2", flush=True)
        r = res[name] = run_shape(gpu, name, pool, group_of, a.sets, a.reps, a.k, a.seed, a.s, batches, slices)
        del pool
        gpu.trim()
        gpu.torch.cuda.empty_cache()
        print(f"{'leg':18s} {'median ms':>10s} {'min':>10s} {'max':>10s} {'passes':>7s} {'slices':>7s} {'max live':>10s} {'/ a':>6s}")
        for l, v in r.items():
            print(f"{l:18s} {v['median']:10.2f} {v['min']:10.2f} {v['max']:10.2f} {str(v.get('passes', '-')):>7s} "
                  f"{str(v.get('slices', '-')):>7s} {str(v.get('max_live', '-')):>10s} {v['median'] / r['a']['median']:6.2f}")
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
