#!/usr/bin/env python3
"""Timing of the sparse dist path (hymet_mash_dist_sparse, hymet_mash_link_edges) against the
dense kernels on the seeded synthetic DB of tools/derep_bench.py, nothing read from outside the
tree: 20,000 sketches of size 1,000, D = 0.05; a tenth of the sketches come in families that
share most of their hashes, the rest are unrelated.

Legs, alternating in one process with their order rotated every repeat, each timed with device
events around work that ends in a synchronisation, after a warm-up round in which the sparse
legs are checked equal to the dense ones (labels and link counts; every row of dist):

    a   derep.cluster(): hymet_mash_dist_tri + hymet_mash_link per block
    b   derep.cluster(sparse=True): hymet_mash_dist_sparse (tri) + hymet_mash_link_edges
    c   mashdist.dist_blocks at D: 20,000 references x 2,000 queries, dense + select
    d   the same with sparse=True

It reports every repeat, the median and the spread (min..max) per leg, the kernels' own times
(the library's event pairs), the counters postings / emitted / candidates of the sparse legs,
whether each sparse leg beats its dense leg by more than the two spreads, and the emitted-key
count at which the two would meet: this shape's count plus the gap between the two medians over
the per-key time of the stages that grow with the keys (emit, key sort, runs) -- a straight-line
extrapolation from this one shape, not a measurement.

--tree runs the dense legs only with hymet_amd imported from another checkout (the parent
commit); --baseline-json brings that run's result into the text.  --write-design replaces the
text between the dist_sparse_bench markers of DESIGN.md.

    python tools/dist_sparse_bench.py --json new.json
    python tools/dist_sparse_bench.py --tree ../parent --json base.json
    python tools/dist_sparse_bench.py --from-json new.json --baseline-json base.json --write-design
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "tools")

N, NQ, S, D = 20_000, 2_000, 1_000, 0.05
BLOCK_BYTES = 1 << 30
BEGIN, END = "<!-- dist_sparse_bench:begin -->", "<!-- dist_sparse_bench:end -->"
KEY_STAGES = ("sparse_emit", "sparse_sort_keys", "sparse_runs")


def collect(blocks):
    parts = list(blocks)
    return tuple(np.concatenate([p[i] for p in parts]) for i in range(4))


def run(gpu, n, nq, reps, dense_only):
    from dist_bench import K, make_db, timed
    from hymet_amd import derep as dr
    from hymet_amd import mashdist as md
    rng = np.random.default_rng(4321)
    fams = rng.integers(0, 2 ** 64, size=(max(1, n // 100), S), dtype=np.uint64)
    db = make_db(rng, n, S, fams)
    qdb = make_db(rng, nq, S, fams)
    assert K == db.k
    print(f"{n} sketches, s={S}, D={D}; dist: {n} x {nq}", flush=True)
    plans = {"b": [], "d": []}

    def leg_b():
        plans["b"].clear()
        return dr.cluster(gpu, db, D, BLOCK_BYTES, sparse=True, plan=plans["b"])

    def leg_d():
        plans["d"].clear()
        return collect(md.sparse_blocks(gpu, db, qdb, D, BLOCK_BYTES, plan=plans["d"]))

    legs = {"a": lambda: dr.cluster(gpu, db, D, BLOCK_BYTES), "c": lambda: collect(md.dist_blocks(gpu, db, qdb, D, BLOCK_BYTES))}
    if not dense_only:
        legs.update(b=leg_b, d=leg_d)
    order = sorted(legs)
    ms = {l: [] for l in order}
    seen = {}
    for rep in range(reps + 1):          # round 0 warms up (allocator, code objects) and checks the legs agree
        for l in order[rep % len(order):] + order[:rep % len(order)]:   # rotate: no leg always follows the same one
            t, out = timed(gpu, legs[l])
            if rep == 0:
                seen[l] = out
                continue
            del out
            ms[l].append(t)
            print(f"  rep {rep} leg {l} {t:10.2f} ms", flush=True)
        if rep == 0:
            info = {"links": int(seen["a"].n_links), "clusters": int(len(np.unique(seen["a"].labels))), "rows": int(len(seen["c"][0]))}
            if not dense_only:
                assert np.array_equal(seen["a"].labels, seen["b"].labels), "legs a and b give different labels"
                assert seen["a"].n_links == seen["b"].n_links, "legs a and b count different links"
                for x, y in zip(seen["c"], seen["d"]):
                    assert x.dtype == y.dtype and np.array_equal(x, y), "legs c and d give different rows"
                assert {p[0] for p in plans["b"]} == {"sparse"} and {p[0] for p in plans["d"]} == {"sparse"}, "a range fell back"
            print(f"  {info['links']} links, {info['clusters']} clusters; {info['rows']} dist rows within D", flush=True)
            seen.clear()
    res = {"shape": {"n": n, "n_qry": nq, "s": S, "max_dist": D, "block_bytes": BLOCK_BYTES}, "info": info, "legs": {}}
    for l in order:                      # one profiled call per leg: the kernels' own times
        gpu.prof(True)
        gpu.prof_reset()
        legs[l]()
        gpu.sync()
        kern = {k: v[0] for k, v in sorted(gpu.prof_table().items()) if k.startswith(("mash_", "sparse_"))}
        gpu.prof(False)
        v = ms[l]
        res["legs"][l] = {"ms": v, "median": statistics.median(v), "min": min(v), "max": max(v), "kernels_ms": kern}
        if l in plans:
            c = [p[3] for p in plans[l]]
            res["legs"][l]["counters"] = {"calls": len(c), "postings": sum(x[0] for x in c), "emitted": sum(x[1] for x in c),
                                          "candidates": sum(x[2] for x in c)}
    print(f"{'leg':4s} {'median ms':>10s} {'min':>10s} {'max':>10s}")
    for l in order:
        r = res["legs"][l]
        print(f"{l:4s} {r['median']:10.2f} {r['min']:10.2f} {r['max']:10.2f}   {r.get('counters', '')}")
        for k, t in r["kernels_ms"].items():
            print(f"       {k:22s} {t:10.3f} ms")
    return res


def verdict(dense, sparse):
    """(beats beyond the two spreads, gain ms, spreads ms, emitted keys at which the legs meet)"""
    gain = dense["median"] - sparse["median"]
    spread = (dense["max"] - dense["min"]) + (sparse["max"] - sparse["min"])
    k = sparse["kernels_ms"]
    keyed = sum(k.get(x, 0.0) for x in KEY_STAGES)
    emitted = sparse["counters"]["emitted"]
    meet = None
    if keyed > 0 and emitted > 0:
        meet = emitted + (dense["median"] - sparse["median"]) / (keyed / emitted)
    return gain > spread, gain, spread, meet


def design_text(new, base, where):
    sh, L = new["shape"], new["legs"]
    lines = [f"Measured by `tools/dist_sparse_bench.py` on {where}: {sh['n']:,} sketches of s = {sh['s']:,}, D = {sh['max_dist']}; "
             f"dist is {sh['n']:,} x {sh['n_qry']:,}; {len(L['a']['ms'])} alternating repeats after a checked warm-up "
             f"({new['info']['links']:,} links, {new['info']['clusters']:,} clusters, {new['info']['rows']:,} dist rows; the sparse "
             "legs equal the dense ones).", "",
             "| leg | median ms (min..max) | postings | emitted | candidates |", "|---|---|---|---|---|"]
    names = {"a": "a cluster() dense", "b": "b cluster(sparse=True)", "c": "c dist_blocks dense", "d": "d dist_blocks(sparse=True)"}
    for l in sorted(L):
        c = L[l].get("counters")
        cnt = f"{c['postings']:,} | {c['emitted']:,} | {c['candidates']:,}" if c else "- | - | -"
        lines.append(f"| {names[l]} | {L[l]['median']:.2f} ({L[l]['min']:.2f}..{L[l]['max']:.2f}) | {cnt} |")
    lines += ["", "Kernel times of one profiled call per leg (the library's event pairs, ms):", ""]
    for l in sorted(L):
        lines.append(f"- {l}: " + ", ".join(f"{k} {t:.3f}" for k, t in L[l]["kernels_ms"].items())
                     + f"; sum {sum(L[l]['kernels_ms'].values()):.2f}")
    lines += ["", "What a leg takes beyond its kernels is the same in all four: the upload of the DBs, the offsets copied back by "
              "each entry's argument check, the table, the copies of the result.", ""]
    for dn, sp in (("a", "b"), ("c", "d")):
        if dn in L and sp in L:
            beats, gain, spread, meet = verdict(L[dn], L[sp])
            lines.append(f"Leg {sp} {'beats' if beats else 'does NOT beat'} leg {dn} beyond the sum of the two spreads on this shape: "
                         f"{L[dn]['median'] / L[sp]['median']:.1f}x, gain {gain:.2f} ms, spreads {spread:.2f} ms.  "
                         + (f"Extrapolated along the per-key time of the emit, key sort and run stages, the two would meet near "
                            f"{meet:,.0f} emitted keys (this shape emits {L[sp]['counters']['emitted']:,}); one shape, a straight "
                            "line, not a measurement of that density." if meet else ""))
    if base is not None:
        B = base["legs"]
        lines += ["", "The dense legs with the parent commit's library in the same tool (`--tree`), same visit: "
                  + "; ".join(f"{l} {B[l]['median']:.2f} ({B[l]['min']:.2f}..{B[l]['max']:.2f}) ms" for l in sorted(B)) + "."]
    return "\n".join(lines)


def write_design(text):
    path = os.path.join(ROOT, "DESIGN.md")
    with open(path, "r", encoding="utf-8") as f:
        s = f.read()
    i, j = s.index(BEGIN), s.index(END)
    with open(path, "w", encoding="utf-8") as f:
        f.write(s[:i + len(BEGIN)] + "\n" + text + "\n" + s[j:])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the sketches (quick runs)")
    ap.add_argument("--tree", default=None, help="import hymet_amd from this checkout (the parent commit): dense legs only")
    ap.add_argument("--json", default=None)
    ap.add_argument("--from-json", default=None, help="skip the run: read its result from this file")
    ap.add_argument("--baseline-json", default=None, help="the --tree run's result")
    ap.add_argument("--write-design", action="store_true")
    ap.add_argument("--where", default="1 x MI355X")
    a = ap.parse_args()
    if a.from_json:
        with open(a.from_json) as f:
            res = json.load(f)
    else:
        sys.path.insert(0, TOOLS)
        sys.path.insert(0, os.path.abspath(a.tree) if a.tree else ROOT)
        from hymet_amd._lib import Gpu
        gpu = Gpu(int(os.environ.get("HYMET_DEVICE", "0")))
        res = run(gpu, max(20, int(N * a.scale)), max(10, int(NQ * a.scale)), a.reps, dense_only=bool(a.tree))
        if a.json:
            os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
            with open(a.json, "w") as f:
                json.dump(res, f, indent=1)
    base = None
    if a.baseline_json:
        with open(a.baseline_json) as f:
            base = json.load(f)
    if "b" in res["legs"]:
        text = design_text(res, base, a.where)
        print(text)
        if a.write_design:
            write_design(text)


if __name__ == "__main__":
    main()
