#!/usr/bin/env python3
"""Timing of the GPU dist kernels (hymet_amd/mashdist.py, csrc/mash_dist.hip) on two seeded
synthetic shapes, nothing read from outside the tree:

    s1000  : 20,000 references x 2,000 queries, sketch size 1,000   (4 x 10^7 pairs)
    s10000 :  2,000 references x 2,000 queries, sketch size 10,000

A tenth of the sketches come in families that share most of their hashes; the rest are
unrelated (no shared hash: the common case of an all-pairs run).

Legs, alternating in one process with their order rotated every repeat, each timed with device
events around work that ends in a synchronisation, after a warm-up round in which the legs'
blocks are checked equal:

    a      hymet_mash_dist, the default path (the tiled kernel where the tile fits the LDS)
    a_tqN  the same with N query sketches per tile (--tq)
    b      hymet_mash_dist with the plain kernel forced (what HYMET_DIST_PATH=global selects)
    c      hymet_mash_dist_select alone at D = 0.05 over leg a's block

It reports every repeat, the median and the spread (min..max) per leg, pairs/s, the kernel's
own time (the library's event pair around the launch), its algorithmic bytes over that time
against the 8.0 TB/s HBM roof, the LDS bytes read per pair (the kernel's loads replayed on the
host for a sample of pairs), and whether a beats b at the medians by more than the two legs'
spreads.

    python tools/dist_bench.py [--shapes s1000,s10000] [--reps 5] [--scale 1.0] [--tq 4,16] [--json OUT]
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

SHAPES = {"s1000": (20_000, 2_000, 1_000), "s10000": (2_000, 2_000, 10_000)}
ROOF = 8.0e12
K = 21


def make_db(rng, n, s, family_rows):
    """n sorted lists of s random uint64; every tenth list takes 90 % of a family row."""
    from hymet_amd.msh import SketchDB
    h = rng.integers(0, 2 ** 64, size=(n, s), dtype=np.uint64)
    keep = int(0.9 * s)
    for i in range(0, n, 10):
        fam = family_rows[(i // 10) % len(family_rows)]
        h[i, :keep] = fam[rng.permutation(s)[:keep]]
    h.sort(axis=1)
    return SketchDB(k=K, sketch_size=s, names=[f"g{i}" for i in range(n)], comments=[""] * n,
                    lengths=np.full(n, 4_000_000, np.int64), offsets=np.arange(n + 1, dtype=np.int64) * s,
                    hashes=h.reshape(-1))


def lds_loads(A, B, s):
    """8-byte LDS loads of one pair in the tiled kernel (csrc/mash_dist.hip wave_pair), replayed."""
    A, B = A[:s], B[:s]
    la, lb = len(A), len(B)
    if la == 0 or lb == 0:
        return 0
    tot = la + lb
    d0, d1, matches, loads = 0, min(s, tot), 0, 0
    while True:
        step = (d1 - d0 + 63) >> 6
        for lane in range(64):
            d = min(d0 + lane * step, d1)
            n = min(step, d1 - d)
            lo, hi = max(0, d - lb), min(d, la)
            while lo < hi:
                mid = (lo + hi) >> 1
                loads += 2
                if A[mid] <= B[d - mid - 1]:
                    lo = mid + 1
                else:
                    hi = mid
            i, j = lo, d - lo
            for _ in range(n):
                a, b = A[min(i, la - 1)], B[min(j, lb - 1)]
                loads += 2
                take_a = i < la and (j >= lb or a <= b)
                matches += take_a and j < lb and a == b
                i += take_a
                j += not take_a
        nxt = min(s + matches, tot)
        if nxt == d1:
            return loads
        d0, d1 = d1, nxt


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


def run_shape(gpu, name, n_ref, n_qry, s, reps, tqs):
    from hymet_amd import mashdist as md
    lib, torch = gpu.lib, gpu.torch
    rng = np.random.default_rng(4321)
    fams = rng.integers(0, 2 ** 64, size=(max(1, n_ref // 100), s), dtype=np.uint64)
    ref_db, qry_db = make_db(rng, n_ref, s, fams), make_db(rng, n_qry, s, fams)
    ref, qry = md.DeviceSketches(gpu, ref_db), md.DeviceSketches(gpu, qry_db)
    table = torch.from_numpy(md.min_common_table(s, K, 0.05).view(np.int16).copy()).to(gpu.dev)
    pairs = n_ref * n_qry
    lib.hymet_mash_dist_tune(0, 0)
    tq0 = lib.hymet_mash_dist_tile(s)
    print(f"  {name}: default path {'tiled, TQ = %d' % tq0 if tq0 else 'plain (the tile does not fit the LDS)'}", flush=True)

    def dist(path, tq):
        def leg():
            lib.hymet_mash_dist_tune(path, tq)
            return md.dist_block(gpu, ref, qry, 0, n_qry, s)
        return leg

    block = dist(0, 0)()
    gpu.sync()
    legs = {"a": dist(0, 0), "b": dist(1, 0),
            "c": lambda: md.select_block(gpu, block, n_qry, n_ref, table, s, cap=pairs // 8 + 1024)[0][-1]}
    if tq0:
        for tq in tqs:
            lib.hymet_mash_dist_tune(0, tq)
            if lib.hymet_mash_dist_tile(s) == tq and tq != tq0:
                legs[f"a_tq{tq}"] = dist(0, tq)
    order = sorted(legs)
    ms = {l: [] for l in order}
    for rep in range(reps + 1):          # round 0 warms up (allocator, code objects) and checks equality
        for l in order[rep % len(order):] + order[:rep % len(order)]:   # rotate: no leg always follows the same one
            t, out = timed(gpu, legs[l])
            if rep == 0:
                if l != "c":
                    assert torch.equal(out, block), f"leg {l} differs from leg a"
                else:
                    v = block.cpu().numpy().view(np.uint32)
                    want = int((md.distance(v >> 16, v & 0xFFFF, K) <= 0.05).sum())
                    assert int(out) == want, f"leg c kept {int(out)} pairs, the host filter {want}"
                    print(f"  {name}: {want} of {pairs} pairs within D = 0.05", flush=True)
                del out
                continue
            del out
            ms[l].append(t)
            print(f"  {name} rep {rep} leg {l:7s} {t:10.2f} ms", flush=True)
    # one profiled call per leg: the kernels' own times and algorithmic bytes
    kern = {}
    for l in order:
        gpu.prof(True)
        gpu.prof_reset()
        legs[l]()
        gpu.sync()
        tab = gpu.prof_table()
        gpu.prof(False)
        kn = "mash_dist_select" if l == "c" else "mash_dist"
        if kn in tab:
            t, n, nbytes = tab[kn]
            kern[l] = {"kernel_ms": t, "alg_bytes": nbytes, "roof_fraction": nbytes / (t * 1e-3) / ROOF if t > 0 else 0.0}
    lib.hymet_mash_dist_tune(0, 0)
    # LDS traffic of the tiled kernel: a sample of pairs replayed on the host
    H = ref_db.hashes.reshape(n_ref, s)
    Q = qry_db.hashes.reshape(n_qry, s)
    srng = np.random.default_rng(7)
    sample = [(int(srng.integers(n_ref)), int(srng.integers(n_qry))) for _ in range(48)] + \
             [(10 * int(srng.integers(n_ref // 10)), 10 * int(srng.integers(n_qry // 10))) for _ in range(16)]
    lds = statistics.mean(8 * lds_loads(H[r].tolist(), Q[q].tolist(), s) for r, q in sample)
    res = {}
    for l, v in ms.items():
        med = statistics.median(v)
        res[l] = {"ms": v, "median": med, "min": min(v), "max": max(v), "pairs_per_s": pairs / (med * 1e-3)}
        res[l].update(kern.get(l, {}))
        if l.startswith("a") and tq0:
            res[l]["lds_bytes_per_pair"] = lds
    res["_shape"] = {"n_ref": n_ref, "n_qry": n_qry, "s": s, "default_tq": tq0}
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default="s1000,s10000")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of each shape's sketches (quick runs)")
    ap.add_argument("--tq", default="4,16", help="tile sizes to time beside the default")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    from hymet_amd._lib import Gpu
    gpu = Gpu(int(os.environ.get("HYMET_DEVICE", "0")))
    tqs = [int(x) for x in a.tq.split(",") if x]
    out = {}
    for name in a.shapes.split(","):
        n_ref, n_qry, s = SHAPES[name]
        n_ref, n_qry = max(10, int(n_ref * a.scale)), max(10, int(n_qry * a.scale))
        print(f"{name}: {n_ref} x {n_qry} sketches, s={s}", flush=True)
        r = out[name] = run_shape(gpu, name, n_ref, n_qry, s, a.reps, tqs)
        gpu.trim()
        gpu.torch.cuda.empty_cache()
        print(f"{'leg':8s} {'median ms':>10s} {'min':>10s} {'max':>10s} {'Gpairs/s':>9s} {'kernel ms':>10s} {'of roof':>8s} "
              f"{'LDS B/pair':>11s}")
        for l, v in r.items():
            if l.startswith("_"):
                continue
            print(f"{l:8s} {v['median']:10.2f} {v['min']:10.2f} {v['max']:10.2f} {v['pairs_per_s'] / 1e9:9.3f} "
                  f"{v.get('kernel_ms', float('nan')):10.2f} {100 * v.get('roof_fraction', float('nan')):7.2f}% "
                  f"{v.get('lds_bytes_per_pair', 0.0):11.0f}")
        av, bv = r["a"], r["b"]
        if r["_shape"]["default_tq"]:
            gain = bv["median"] - av["median"]
            spread = (av["max"] - av["min"]) + (bv["max"] - bv["min"])
            print(f"a beats b beyond the two spreads: {'yes' if gain > spread else 'NO'} "
                  f"(b/a = {bv['median'] / av['median']:.2f}, gain {gain:.2f} ms, spreads {spread:.2f} ms)")
        else:
            print("a and b are the same kernel at this sketch size")
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
