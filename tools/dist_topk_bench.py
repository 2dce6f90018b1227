#!/usr/bin/env python3
"""Timing of the nearest-references path (`dist --top K`: hymet_amd/mashdist.py top_blocks,
csrc/mash_topk.hip) on the seeded synthetic shape of tools/dist_bench.py, nothing read from
outside the tree:

    s1000 : 20,000 references x 2,000 queries, sketch size 1,000 (4 x 10^7 pairs), a tenth of
            the sketches in families that share most of their hashes

Legs, alternating in one process with their order rotated every repeat, each timed with device
events around work that ends in a synchronisation, after a warm-up round in which every leg's rows
are checked equal:

    a        what the code without --top offers: dist_blocks dense, every pair to the host, then
             the K best per query with numpy (argpartition on the exact order's key, then a sort
             of the K); K = 10 (the host work does not depend on K)
    b_K      dist_blocks(top=K), K = 1, 10, 100 and hymet_mash_topk_max()
    c_K      hymet_mash_dist_topk alone over a resident dense block, same K
    c_sel    hymet_mash_dist_select alone at D = 0.05 over the same block

It reports every repeat, the median and the spread (min..max) per leg, the kernels' own time (the
library's event pair around the launches) with their algorithmic bytes against the 8.0 TB/s HBM
roof, the ratio of c_K to c_sel, and whether b_K beats a at the medians by more than the two
legs' spreads together.

    python tools/dist_topk_bench.py [--reps 5] [--scale 1.0] [--json OUT] [--md OUT]
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

from tools.dist_bench import K, ROOF, SHAPES, make_db, timed  # noqa: E402


def host_topk(parts, n_ref, top):
    """The K best references of every query from dist_blocks' dense arrays, in the order of
    `dist --top` (include/hymet_gpu.h at hymet_mash_dist_topk): (q, r, common, denom)."""
    out = []
    for qi, ri, c, d in parts:
        nq = len(qi) // n_ref
        c64, d64 = c.astype(np.int64), d.astype(np.int64)
        rank = np.where(d64 == 0, 0, (1 << 31) - (c64 << 31) // np.maximum(d64, 1)).astype(np.uint64)
        key = (rank << np.uint64(32) | ri.astype(np.uint64)).reshape(nq, n_ref)
        k = min(top, n_ref)
        best = np.argpartition(key, k - 1, axis=1)[:, :k] if k < n_ref else np.tile(np.arange(n_ref), (nq, 1))
        best = np.take_along_axis(best, np.argsort(np.take_along_axis(key, best, axis=1), axis=1), axis=1)
        flat = (np.arange(nq)[:, None] * n_ref + best).reshape(-1)
        out.append((qi[flat], ri[flat], c[flat], d[flat]))
    return tuple(np.concatenate([p[i] for p in out]) for i in range(4))


def run(gpu, n_ref, n_qry, s, reps):
    from hymet_amd import mashdist as md
    from hymet_amd._lib import ptr
    lib, torch = gpu.lib, gpu.torch
    rng = np.random.default_rng(4321)
    fams = rng.integers(0, 2 ** 64, size=(max(1, n_ref // 100), s), dtype=np.uint64)
    ref_db, qry_db = make_db(rng, n_ref, s, fams), make_db(rng, n_qry, s, fams)
    ref, qry = md.DeviceSketches(gpu, ref_db), md.DeviceSketches(gpu, qry_db)
    table = torch.from_numpy(md.min_common_table(s, K, 0.05).view(np.int16).copy()).to(gpu.dev)
    pairs = n_ref * n_qry
    tops = [1, 10, 100, md.topk_max()]
    block = md.dist_block(gpu, ref, qry, 0, n_qry, s)
    gpu.sync()

    def collect(blocks):
        parts = list(blocks)
        return tuple(np.concatenate([p[i] for p in parts]) for i in range(4))

    def kernels(top):
        idx = gpu.empty(n_qry * top, torch.int32)
        val = gpu.empty(n_qry * top, torch.int32)
        cnt = gpu.empty(n_qry, torch.int32)

        def leg():
            gpu.call("hymet_mash_dist_topk", ptr(block), n_qry, n_ref, None, s, top, ptr(idx), ptr(val), ptr(cnt))
            return idx, val, cnt
        return leg

    legs = {"a": lambda: host_topk(list(md.dist_blocks(gpu, ref_db, qry_db)), n_ref, 10),
            "c_sel": lambda: md.select_block(gpu, block, n_qry, n_ref, table, s, cap=pairs // 8 + 1024)[0][-1]}
    for top in tops:
        legs[f"b_{top}"] = (lambda t: lambda: collect(md.dist_blocks(gpu, ref_db, qry_db, top=t)))(top)
        legs[f"c_{top}"] = kernels(top)
    order = sorted(legs)
    ms = {l: [] for l in order}
    want = {}
    for rep in range(reps + 1):          # round 0 warms up (allocator, code objects) and checks equality
        for l in order[rep % len(order):] + order[:rep % len(order)]:   # rotate: no leg always follows the same one
            t, out = timed(gpu, legs[l])
            if rep > 0:
                del out
                ms[l].append(t)
                print(f"  rep {rep} leg {l:7s} {t:10.2f} ms", flush=True)
                continue
            if not want:                 # the reference rows: leg a's method at every K
                dense = list(md.dist_blocks(gpu, ref_db, qry_db))
                want.update({top: host_topk(dense, n_ref, top) for top in tops})
                del dense
            if l == "a":
                rows, top = out, 10
            elif l.startswith("b_"):
                rows, top = out, int(l[2:])
            elif l == "c_sel":
                print(f"  {int(out)} of {pairs} pairs within D = 0.05", flush=True)
                continue
            else:
                top = int(l[2:])
                gpu.sync()
                idx, val, cnt = (x.cpu().numpy() for x in out)
                k = min(top, n_ref)
                assert (cnt == k).all(), f"leg {l}: counts differ from {k}"
                v = val.view(np.uint32).reshape(n_qry, top)[:, :k].reshape(-1)
                rows = (np.repeat(np.arange(n_qry, dtype=np.int32), k), idx.reshape(n_qry, top)[:, :k].reshape(-1),
                        (v >> 16).astype(np.int32), (v & 0xFFFF).astype(np.int32))
            for x, y in zip(rows, want[top]):
                assert np.array_equal(x, y), f"leg {l} differs from the host's rows at K = {top}"
            del out, rows
    print("  warm-up: every leg's rows equal the host's", flush=True)
    kern = {}
    for l in order:                      # one profiled call per leg: the kernels' own times and algorithmic bytes
        if not l.startswith("c_"):
            continue
        gpu.prof(True)
        gpu.prof_reset()
        legs[l]()
        gpu.sync()
        tab = gpu.prof_table()
        gpu.prof(False)
        kn = "mash_dist_select" if l == "c_sel" else "mash_dist_topk"
        if kn in tab:
            t, _, nbytes = tab[kn]
            kern[l] = {"kernel_ms": t, "alg_bytes": nbytes, "roof_fraction": nbytes / (t * 1e-3) / ROOF if t > 0 else 0.0}
    res = {}
    for l, v in ms.items():
        res[l] = {"ms": v, "median": statistics.median(v), "min": min(v), "max": max(v)}
        res[l].update(kern.get(l, {}))
    res["_shape"] = {"n_ref": n_ref, "n_qry": n_qry, "s": s, "tops": tops}
    return res


def report(r):
    """The table and the two claims, as Markdown lines."""
    sh = r["_shape"]
    out = [f"{sh['n_ref']:,} references x {sh['n_qry']:,} queries, s = {sh['s']:,}; ms, median of {len(r['a']['ms'])} (min..max)", "",
           "| leg | what | median ms | min..max | kernels' own ms | of the 8.0 TB/s roof |", "|---|---|---|---|---|---|"]
    what = {"a": "dense `dist_blocks`, K best with numpy (K = 10)", "c_sel": "`hymet_mash_dist_select` alone, D = 0.05"}
    for l, v in r.items():
        if l.startswith("_"):
            continue
        w = what.get(l) or (f"`dist_blocks(top={l[2:]})`" if l.startswith("b_") else f"`hymet_mash_dist_topk` alone, K = {l[2:]}")
        km = f"{v['kernel_ms']:.3f}" if "kernel_ms" in v else ""
        rf = f"{100 * v['roof_fraction']:.1f} %" if "roof_fraction" in v else ""
        out.append(f"| {l} | {w} | {v['median']:.2f} | {v['min']:.2f}..{v['max']:.2f} | {km} | {rf} |")
    out.append("")
    a = r["a"]
    for top in sh["tops"]:
        b, c = r[f"b_{top}"], r[f"c_{top}"]
        gain, spread = a["median"] - b["median"], (a["max"] - a["min"]) + (b["max"] - b["min"])
        line = (f"K = {top}: b beats a beyond the two spreads: {'yes' if gain > spread else 'NO'} "
                f"(a/b = {a['median'] / b['median']:.1f}, gain {gain:.1f} ms, spreads {spread:.1f} ms)")
        if "kernel_ms" in c and "kernel_ms" in r["c_sel"]:
            line += f"; top-K kernels / select kernels = {c['kernel_ms'] / r['c_sel']['kernel_ms']:.2f}"
        out.append("- " + line)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the shape's sketches (quick runs)")
    ap.add_argument("--json", default=None)
    ap.add_argument("--md", default=None, help="write the table and the claims as Markdown")
    a = ap.parse_args()
    from hymet_amd._lib import Gpu
    gpu = Gpu(int(os.environ.get("HYMET_DEVICE", "0")))
    n_ref, n_qry, s = SHAPES["s1000"]
    n_ref, n_qry = max(10, int(n_ref * a.scale)), max(10, int(n_qry * a.scale))
    print(f"s1000: {n_ref} x {n_qry} sketches, s={s}", flush=True)
    r = run(gpu, n_ref, n_qry, s, a.reps)
    lines = report(r)
    print("\n".join(lines))
    for path, text in ((a.json, json.dumps(r, indent=1)), (a.md, "\n".join(lines) + "\n")):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as f:
                f.write(text)


if __name__ == "__main__":
    main()
