#!/usr/bin/env python3
"""Timing of the GPU sketch builder (hymet_amd/sketch.py, csrc/sketch.hip) on two seeded
synthetic shapes, nothing read from outside the tree:

    small : 20,000 references x 30 kb   (viral / plasmid-like: the reason for batching)
    bact  :    300 references x 4 Mbp   (bacterial-like: many chunks and a merge per reference)

Three legs alternate in one process, each timed with device events around work that ends in a
synchronisation, after a warm-up round:

    a  screen.sketch_sequences: one screen-kernel launch, two host syncs, a D2H copy and an
       np.unique per record (what the project had before the batch path)
    b  sketch.sketch_pool: one hymet_sketch_batch call and one D2H copy, for each chunk size
    c  the hash-only floor: hymet_screen_count with ndb = 0 and cand_thr = 0 over the pool

It reports every repeat, the median and the spread (min..max) per leg, b / c (the cost of the
selection over bare hashing), and whether b beats a on `small` by more than the spread and is
not slower than a on `bact` beyond the spread.

    python tools/sketch_bench.py [--shapes small,bact] [--reps 5] [--scale 1.0] [--json OUT]
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

SHAPES = {"small": (20_000, 30_000), "bact": (300, 4_000_000)}
CHUNKS = {"256k": 1 << 18, "1M": 1 << 20, "4M": 1 << 22}


def make_pool(gpu, n_refs, ref_len, seed):
    """n_refs random references of ref_len bases as one packed pool ('N' between records)."""
    from hymet_amd.seqio import DevicePool, SeqSet
    rng = np.random.default_rng(seed)
    step = ref_len + 1
    buf = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=n_refs * step - 1, dtype=np.uint8)]
    buf[ref_len::step] = ord("N")
    ss = SeqSet([f"ref{i}" for i in range(n_refs)], [""] * n_refs, np.full(n_refs, ref_len, np.int64),
                np.arange(n_refs, dtype=np.int64) * step, buf.tobytes())
    del buf
    return DevicePool(gpu, ss, DevicePool.ALPHA_MASH)


def timed(gpu, fn):
    torch = gpu.torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    gpu.sync()
    a.record(gpu.bound_stream)
    out = fn()
    gpu.sync()
    b.record(gpu.bound_stream)
    b.synchronize()
    return a.elapsed_time(b), out


def hash_floor(gpu, pool, k, seed):
    from hymet_amd._lib import ptr
    torch = gpu.torch
    cand_n, nk = gpu.zeros(1, torch.int64), gpu.zeros(1, torch.int64)
    null4 = (ctypes.c_void_p * 4)()
    zero4 = (ctypes.c_int64 * 4)()
    gpu.call("hymet_screen_count", ptr(pool.w2b), ptr(pool.wmask), pool.n_bases, 0, pool.n_bases - k + 1, k, seed, 0,
             null4, zero4, null4, zero4, null4, 0, None, 0, ptr(cand_n), ptr(nk))
    gpu.sync()
    return int(nk.item())


def run_shape(gpu, name, n_refs, ref_len, reps, k, seed, s, skip_a):
    from hymet_amd import screen as scr
    from hymet_amd import sketch as sk
    pool = make_pool(gpu, n_refs, ref_len, 1234)
    legs = {"c": lambda: hash_floor(gpu, pool, k, seed)}
    for cn, cb in CHUNKS.items():
        legs["b_" + cn] = (lambda cb=cb: sk.sketch_pool(gpu, pool, None, k=k, seed=seed, s=s, chunk_bases=cb))
    if not skip_a:
        legs["a"] = lambda: scr.sketch_sequences(gpu, pool, k=k, seed=seed, s=s)
    order = sorted(legs)
    ms = {l: [] for l in order}
    ref = None
    for rep in range(reps + 1):          # round 0 warms up (allocator, code objects) and checks equality
        for l in order[rep % len(order):] + order[:rep % len(order)]:   # rotate: no leg always follows the same one
            t, out = timed(gpu, legs[l])
            if rep == 0:
                if l[0] in "ab":
                    if ref is None:
                        ref = out
                    else:
                        assert len(out) == len(ref) and all(np.array_equal(x, y) for x, y in zip(out, ref)), \
                            f"leg {l} differs from leg {order[0]}"
                continue
            ms[l].append(t)
            print(f"  {name} rep {rep} leg {l:7s} {t:10.2f} ms", flush=True)
    # one profiled batch call at the default chunk size: the two kernels' own times
    gpu.prof(True)
    gpu.prof_reset()
    sk.sketch_pool(gpu, pool, None, k=k, seed=seed, s=s)
    gpu.sync()
    for kn, (t, n, nbytes) in sorted(gpu.prof_table().items()):
        if kn.startswith("sketch_"):
            print(f"  {name} kernel {kn:13s} {t:10.2f} ms  {n} launch(es)  {nbytes / 1e6 / max(t, 1e-9):8.1f} GB/s algorithmic")
    gpu.prof(False)
    return {l: {"ms": v, "median": statistics.median(v), "min": min(v), "max": max(v)} for l, v in ms.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default="small,bact")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of each shape's references (quick runs)")
    ap.add_argument("-k", type=int, default=21)
    ap.add_argument("-s", type=int, default=1000)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--skip-a", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    from hymet_amd import sketch as sk
    from hymet_amd._lib import Gpu
    gpu = Gpu(int(os.environ.get("HYMET_DEVICE", "0")))
    default = next(n for n, v in CHUNKS.items() if v == sk.DEFAULT_CHUNK_BASES)
    res = {}
    for name in a.shapes.split(","):
        n_refs, ref_len = SHAPES[name]
        n_refs = max(1, int(n_refs * a.scale))
        print(f"{name}: {n_refs} x {ref_len} bases, k={a.k} s={a.s}", flush=True)
        r = res[name] = run_shape(gpu, name, n_refs, ref_len, a.reps, a.k, a.seed, a.s, a.skip_a)
        gpu.trim()
        gpu.torch.cuda.empty_cache()
        print(f"{'leg':8s} {'median ms':>10s} {'min':>10s} {'max':>10s}")
        for l, v in r.items():
            print(f"{l:8s} {v['median']:10.2f} {v['min']:10.2f} {v['max']:10.2f}")
        b = r["b_" + default]
        print(f"b/c (chunk {default}): {b['median'] / r['c']['median']:.2f}")
        if "a" in r:
            av = r["a"]
            if name == "small":
                ok = b["max"] < av["min"]
                print(f"b beats a beyond the spread: {'yes' if ok else 'NO'} (a/b = {av['median'] / b['median']:.1f})")
            else:
                ok = b["min"] <= av["max"]
                print(f"b not slower than a beyond the spread: {'yes' if ok else 'NO'} "
                      f"(a/b = {av['median'] / b['median']:.2f})")
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
