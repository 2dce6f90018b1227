#!/usr/bin/env python3
"""Timing of the screen with and without winner-take-all (`mash screen -w`; hymet_amd/screen.py,
csrc/screen.hip) in one session, on a seeded synthetic shape, nothing read from outside the tree:

    DB   : 100,000 references x 1,000 hashes (the shape of tools/table_bench.py): 50 organisms
           x 6 strains sketched on the GPU (the references the pool can hit), the rest decoys
    pool : ~20 Mbp of contigs cut from the 50 organisms (synth.make_cami)

Two legs alternate in one process, each timed with device events around a screen() call that
ends in a synchronisation (host work included: ranking, formatting is not), after a warm-up
round that also checks that the first-pass arrays of the two legs are equal:

    plain   screen(..., winner=False)
    winner  screen(..., winner=True)

A profiled pass then reports the kernels' own times per call: screen_count, screen_stats and,
for the winner leg, screen_winner (the fill of `win`, the claim kernel and the winner
statistics together).

The baseline the extra work is held against is the PARENT commit's screen_count + screen_stats,
not this code's own: run the tool once more with --tree pointing at a checkout of the parent
(built), which imports hymet_amd from there and runs the plain leg only, then merge:

    python tools/screen_winner_bench.py --json new.json
    python tools/screen_winner_bench.py --tree ../parent --json base.json
    python tools/screen_winner_bench.py --from-json new.json --baseline-json base.json --write-design

--write-design replaces the text between the screen_winner_bench markers of DESIGN.md.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BEGIN, END = "<!-- screen_winner_bench:begin -->", "<!-- screen_winner_bench:end -->"


def make_case(gpu, n_refs, n_taxa, per_taxon, pool_gbp, seed):
    from hymet_amd import sketch as sk
    from hymet_amd import synth
    from hymet_amd.msh import SketchDB
    from hymet_amd.seqio import DevicePool, from_records
    rng = np.random.default_rng(seed)
    w = synth.make_cami(rng, n_taxa=n_taxa, per_taxon=per_taxon, genome_mbp=(0.3, 0.5), contig_gbp=pool_gbp, name="winner")
    refs = from_records([(n, "", s) for n, s in zip(w.ref_names, w.refs)])
    hl = sk.sketch_pool(gpu, DevicePool(gpu, refs, DevicePool.ALPHA_MASH), None, k=21, seed=42, s=1000)
    lengths = [len(s) for s in w.refs]
    n_dec = max(0, n_refs - len(hl))
    hl = list(hl) + list(synth.decoy_sketches(rng, n_dec, 1000))
    lengths += [4_000_000] * n_dec
    off = np.zeros(len(hl) + 1, np.int64)
    off[1:] = np.cumsum([len(h) for h in hl])
    names = [f"r{i}" for i in range(len(hl))]
    db = SketchDB(names=names, comments=[""] * len(hl), lengths=np.array(lengths, np.int64), offsets=off,
                  hashes=np.concatenate(hl))
    pool = DevicePool(gpu, from_records([(n, "", s) for n, s in zip(w.contig_names, w.contigs)]), DevicePool.ALPHA_MASH)
    return db, pool


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


def run(gpu, db, pool, legs, reps):
    from hymet_amd import screen as scr
    table = scr.ScreenTable(gpu, db)
    gpu.sync()
    fns = {"plain": lambda: scr.screen(gpu, pool, [db], [table])[0]}
    if "winner" in legs:
        fns["winner"] = lambda: scr.screen(gpu, pool, [db], [table], winner=True)[0]
    order = [l for l in ("plain", "winner") if l in legs]
    ms = {l: [] for l in order}
    info = {}
    for rep in range(reps + 1):          # round 0 warms up (allocator, code objects) and checks equality
        for l in order[rep % len(order):] + order[:rep % len(order)]:
            t, res = timed(gpu, fns[l])
            if rep == 0:
                first = res.shared_first if l == "winner" else res.shared
                info.setdefault("first", first)
                assert np.array_equal(first, info["first"]), "the legs' first-pass arrays differ"
                info[l + "_refs_hit"] = int(np.count_nonzero(res.shared))
                info[l + "_shared_sum"] = int(res.shared.sum())
                continue
            ms[l].append(t)
            print(f"  rep {rep} leg {l:7s} {t:9.3f} ms", flush=True)
    out = {"legs": {l: {"ms": v, "median": statistics.median(v), "min": min(v), "max": max(v)} for l, v in ms.items()},
           "competing_refs": int(np.count_nonzero(info["first"])), "n_refs": db.n_refs, "n_hashes": int(len(db.hashes)),
           "pool_bases": int(pool.n_bases)}
    out.update({k: v for k, v in info.items() if k != "first"})
    # the kernels' own times, per call, from a profiled pass of each leg
    gpu.prof(True)
    for l in order:
        gpu.prof_reset()
        for _ in range(reps):
            fns[l]()
        gpu.sync()
        out["legs"][l]["kernels_ms"] = {kn: t / reps for kn, (t, n, _) in sorted(gpu.prof_table().items())
                                        if kn.startswith("screen_")}
        for kn, t in out["legs"][l]["kernels_ms"].items():
            print(f"  leg {l:7s} kernel {kn:14s} {t:9.3f} ms per call", flush=True)
    gpu.prof(False)
    return out


def design_text(new, base, where):
    p, w = new["legs"]["plain"], new["legs"]["winner"]
    pk, wk = p["kernels_ms"], w["kernels_ms"]
    lines = [f"Measured by `tools/screen_winner_bench.py` on {where}: {new['n_refs']:,} references / "
             f"{new['n_hashes'] / 1e6:.0f} M hashes, pool {new['pool_bases'] / 1e6:.1f} Mbp, {new['competing_refs']} competing "
             f"references (first-pass shared > 0), {len(p['ms'])} alternating repeats after a warm-up.", "",
             "| leg | screen() median ms (min..max) | screen_count | screen_stats | screen_winner |", "|---|---|---|---|---|"]
    for name, leg, k in (("plain", p, pk), ("winner", w, wk)):
        win = f"{k['screen_winner']:.3f}" if "screen_winner" in k else "-"
        lines.append(f"| {name} | {leg['median']:.3f} ({leg['min']:.3f}..{leg['max']:.3f}) | {k.get('screen_count', 0):.3f} | "
                     f"{k.get('screen_stats', 0):.3f} | {win} |")
    extra = wk["screen_winner"]
    lines += ["", f"With winner-take-all the rows keep {new['winner_refs_hit']} of the {new['plain_refs_hit']} references "
              f"the plain screen reports."]
    if base is not None:
        bk = base["legs"]["plain"]["kernels_ms"]
        b = bk.get("screen_count", 0) + bk.get("screen_stats", 0)
        lines += ["", f"Baseline, the parent commit's library in the same tool (`--tree`): screen_count "
                  f"{bk.get('screen_count', 0):.3f} ms + screen_stats {bk.get('screen_stats', 0):.3f} ms = {b:.3f} ms per call "
                  f"(screen() median {base['legs']['plain']['median']:.3f} ms).  The winner kernels add {extra:.3f} ms = "
                  f"{100 * extra / b:.1f} % of that, {100 * extra / max(bk.get('screen_count', 0), 1e-9):.1f} % of screen_count; "
                  f"the whole call, host ranking and the two extra copies included, goes from {p['median']:.3f} to "
                  f"{w['median']:.3f} ms."]
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
    ap.add_argument("--refs", type=int, default=100_000)
    ap.add_argument("--taxa", type=int, default=50)
    ap.add_argument("--per-taxon", type=int, default=6)
    ap.add_argument("--pool-gbp", type=float, default=0.02)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--tree", default=None, help="import hymet_amd from this checkout (the parent commit): plain leg only")
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
        sys.path.insert(0, os.path.abspath(a.tree) if a.tree else ROOT)
        from hymet_amd._lib import Gpu
        gpu = Gpu(int(os.environ.get("HYMET_DEVICE", "0")))
        db, pool = make_case(gpu, a.refs, a.taxa, a.per_taxon, a.pool_gbp, a.seed)
        print(f"DB {db.n_refs} refs / {len(db.hashes) / 1e6:.0f}M hashes, pool {pool.n_bases / 1e6:.1f} Mbp", flush=True)
        res = run(gpu, db, pool, ["plain"] if a.tree else ["plain", "winner"], a.reps)
        if a.json:
            os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
            with open(a.json, "w") as f:
                json.dump(res, f, indent=1)
    base = None
    if a.baseline_json:
        with open(a.baseline_json) as f:
            base = json.load(f)
    if "winner" in res["legs"]:
        text = design_text(res, base, a.where)
        print(text)
        if a.write_design:
            write_design(text)


if __name__ == "__main__":
    main()
