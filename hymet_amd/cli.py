"""Stage drop-ins with the reference scripts' argv / file / exit-code contracts.

    python -m hymet_amd.cli screen  INPUT_DIR DB.msh SCREEN_TAB FILTERED SORTED TOP_HITS SELECTED THRESH
        == scripts/mash.sh:4-55 (mash screen -p 8 -v 0.9, sort -u -k5,5, sort -gr, threshold walk)
           HYMET_SCREEN_WINNER=1 in the environment: mash screen -w (winner-take-all) instead
    python -m hymet_amd.cli limit --selected F --output F [--score-file F]... [--max N] [--dedupe] ...
        == scripts/limit_candidates.py:47-89,249-289
    python -m hymet_amd.cli map     INPUT_DIR REFERENCE_FASTA INDEX_PATH PAF_OUT
        == scripts/minimap2.sh:4-33 (minimap2 -I2g -d, minimap2 -x asm10)
    python -m hymet_amd.cli classify        --paf P --taxonomy T --hierarchy H --output O [--processes N]
        == scripts/classification_cami.py:345-354
    python -m hymet_amd.cli classify-legacy (same flags)
        == scripts/classification.py:184-200
    python -m hymet_amd.cli build-id-map detailed_taxonomy.tsv out_map.tsv
        == tools/build_id_map.py (classification fallback, run_hymet_cami.sh:191)
    python -m hymet_amd.cli mini-classify input.paf id_to_taxid.tsv out.tsv
        == tools/mini_classify.py (classification fallback, run_hymet_cami.sh:192)
    python -m hymet_amd.cli hymet2cami classified_sequences.tsv
        == tools/hymet2cami.py (CAMI profile export, run_hymet_cami.sh:214-218)
    python -m hymet_amd.cli taxonomy-hierarchy [NAMES_DMP NODES_DMP OUT]
        == scripts/taxonomy_hierarchy.py (taxdump -> taxonomy_hierarchy.tsv)
    python -m hymet_amd.cli download-db GENOMES_FILE OUTPUT_DIR TAXONOMY_FILE CACHE_DIR
        == scripts/downloadDB.py:178-249 offline (detailed_taxonomy.tsv, combined_genomes.fasta)
    python -m hymet_amd.cli eval-cami [--pred-profile ... --outdir D]
        == tools/eval_cami.py (CAMI profile and contig metrics)
    python -m hymet_amd.cli sketch [-k K] [-s S] [-S SEED] [-i] [-Z] [-l] [-r] [-m M] [-g SIZE] [--batch-bases SIZE] -o PREFIX FILE...
        == mash sketch (builds the sketch DB the screen reads; the reference downloads its DBs,
           so there is no stage script and no scripts/ wrapper for it).  FILE is FASTA or FASTQ;
           -r: each FILE is a read set, -m M: keep only k-mers seen at least M times;
           --batch-bases SIZE: bases read and held per batch, a read file above it is streamed
    python -m hymet_amd.cli dist [-d D] [-v P] [-t] [--sparse] [--top K] [-i] [-l] [-r] [-m M] [--batch-bases SIZE] REF.msh QUERY...
        == mash dist (all-pairs distances between sketch DBs; QUERY is .msh, FASTA or FASTQ,
           with -r / -m M a read set, --batch-bases SIZE as for sketch; like sketch, not a stage
           of the reference workflow)
    python -m hymet_amd.cli mash-screen [-w] [-i MIN_IDENTITY] [-v MAX_P] DB.msh FILE...
        == mash screen (the rows on stdout, in sketch order; -w: winner-take-all; FILE is FASTA
           or FASTQ)
    python -m hymet_amd.cli derep [-d D] [-r longest|first] [-o PREFIX] [-k K] [-s S] [-S SEED] [--greedy] [--sparse] [-i]
                                  [-l] INPUT...
        single-linkage clusters of the INPUT sketches under a distance threshold, one
        representative per cluster, optionally the reduced .msh (no Mash command does this);
        --greedy: greedy representatives instead, every member within the threshold of its own
    python -m hymet_amd.cli triangle [-i] [-l] INPUT...
        == mash triangle (the lower-triangular distance matrix of the INPUT sketches)

The thin wrappers under scripts/ call these, so run_hymet_cami.sh / main.pl can use them
in place of the reference stage scripts unchanged.  All device work goes through
libhymet_gpu.so; without it (or without a GPU) every GPU subcommand fails loudly.
"""
from __future__ import annotations

import argparse
import glob
import logging
import os
import sys
from typing import List, Optional, Sequence

import numpy as np


def _fna_files(input_dir: str) -> List[str]:
    # bash expands "$INPUT_DIR"/*.fna in collation order; LC_ALL=C byte order here
    return sorted(glob.glob(os.path.join(input_dir, "*.fna")), key=lambda p: p.encode())


def _write_lines(path: str, lines: Sequence[str]):
    with open(path, "w", encoding="utf-8", newline="") as f:
        for l in lines:
            f.write(l + "\n")


# ------------------------------------------------------------------ screen (mash.sh)
def screen_winner_env(environ=None) -> bool:
    """HYMET_SCREEN_WINNER: 1 / true / yes / on switch the screen stage to `mash screen -w`;
    unset, empty, 0 / false / no / off leave it as the reference runs it.  Anything else is an
    error (a typo must not silently change the candidate list)."""
    v = (os.environ if environ is None else environ).get("HYMET_SCREEN_WINNER", "").strip().lower()
    if v in ("", "0", "false", "no", "off"):
        return False
    if v in ("1", "true", "yes", "on"):
        return True
    raise ValueError(f"HYMET_SCREEN_WINNER={v!r}: expected 1 or 0")


def cmd_screen(argv: Sequence[str]) -> int:
    if len(argv) != 8:
        print("usage: screen INPUT_DIR DB.msh SCREEN_TAB FILTERED SORTED TOP_HITS SELECTED THRESH", file=sys.stderr)
        return 2
    input_dir, msh_path, screen_tab, filtered, sorted_p, top_hits, selected, thresh = argv
    try:
        winner = screen_winner_env()
    except ValueError as e:
        print(f"screen: {e}", file=sys.stderr)
        return 2
    from . import screen as scr
    from . import select as sel
    from ._lib import Gpu
    from .msh import load_db
    from .seqio import DevicePool, read_fasta
    files = _fna_files(input_dir)
    db = load_db(msh_path)
    gpu = Gpu(int(os.environ.get("HYMET_DEVICE", "0")))
    rows: List[str] = []
    if files:
        ss = read_fasta(files)
        res = scr.screen(gpu, DevicePool(gpu, ss, DevicePool.ALPHA_MASH), [db], winner=winner)[0]
        rows = res.lines(v_max=0.9)
    _write_lines(screen_tab, rows)
    f_rows = sel.sort_unique_k5(rows)
    _write_lines(filtered, f_rows)
    s_rows = sel.sort_gr(f_rows)
    _write_lines(sorted_p, s_rows)
    n_files = len(files)
    need = sel.min_candidates(n_files)
    print("====================================")
    print(f"Number of input sequences: {n_files}")
    print(f"Minimum expected candidates: {need}")
    print("====================================")
    best, top, names, log = sel.threshold_walk(s_rows, thresh, n_files)
    _write_lines(top_hits, top)
    _write_lines(selected, names)
    print("\n".join(log))     # mash.sh:35-36,50,57-60: per-threshold lines, fallback note, summary
    return 0


# ------------------------------------------------------------ limit (limit_candidates.py)
def cmd_limit(argv: Sequence[str]) -> int:
    from . import select as sel
    p = argparse.ArgumentParser(prog="limit", description="Limit Mash candidate genomes (limit_candidates.py).")
    p.add_argument("--selected", required=True)
    p.add_argument("--output", required=True)
    p.add_argument("--score-file", action="append", default=[], dest="score_files")
    p.add_argument("--assembly-dir", default=None)
    p.add_argument("--max", type=int, default=5000)
    p.add_argument("--dedupe", action="store_true")
    p.add_argument("--log", default=None)
    p.add_argument("--no-download", action="store_true")
    a = p.parse_args(argv)
    if a.max <= 0:
        raise SystemExit("The --max value must be greater than zero.")
    with open(a.selected, "r", encoding="utf-8") as f:
        cands = [l.strip() for l in f if l.strip()]
    if not cands:
        raise SystemExit(f"No candidates found in {a.selected}")
    scores = sel.read_scores([s for s in a.score_files if os.path.exists(s)])
    # never downloads: without local assembly summaries the species key is the accession.
    # Default directory as limit_candidates.py:259-263 resolves it (repo/data/...).
    adir = a.assembly_dir or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "data",
                                          "downloaded_genomes", "assembly_summaries")
    smap = sel.species_map(adir) if a.dedupe else {}
    chosen = sel.limit(cands, scores, a.max, a.dedupe, smap)
    tmp = a.output + ".tmp"
    _write_lines(tmp, chosen)
    os.replace(tmp, a.output)
    kept = len(chosen)
    summary = (f"[limit_candidates] kept {kept} / {len(cands)} candidates ({kept} unique keys) "
               f"{'(species dedupe)' if a.dedupe else ''}")
    print(summary)
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "a", encoding="utf-8") as f:
            f.write(summary.rstrip("\n") + "\n")
    return 0


# ------------------------------------------------------------------ map (minimap2.sh)
def build_parts(gpu, refs, split_idx: str = "2g", mini_batch: float = 50e6, w: int = 10, k: int = 15):
    """minimap2 -I<split_idx> -d: the device index, one part per <= split_idx bases."""
    from . import mapper as mp
    parts_idx = mp.split_parts(refs.lengths, float(mp.parse_num(split_idx)), mini_batch)
    parts, first = [], []
    for p in parts_idx:
        sub = refs.subset(p) if len(parts_idx) > 1 else refs
        parts.append(mp.IndexPart(gpu, sub, w, k))
        first.append(int(p[0]))
    return parts, list(refs.names), refs.lengths, first


def read_query_files(paths: Sequence[str]) -> bytes:
    """The pooled input/*.fna as one FASTA text, file order kept; bytes before a file's
    first record are skipped (kseq does) and files are joined on a line break."""
    out = []
    for p in paths:
        with open(p, "rb") as f:
            d = f.read()
        if p.endswith(".gz") or d[:2] == b"\x1f\x8b":
            import gzip
            d = gzip.decompress(d)
        if not d.startswith(b">"):
            i = d.find(b"\n>")
            d = d[i + 1:] if i >= 0 else b""
        if d and not d.endswith(b"\n"):
            d += b"\n"
        out.append(d)
    return b"".join(out)


def map_paf(gpu, parts, names, lens, first, query_fasta: bytes, batch_bases: int = 40_000_000) -> bytes:
    """`-x asm10` mapping of the pooled queries against the index parts -> resultados.paf
    bytes in minimap2's order (part by part; queries in input order within a part), through
    the fused path's device kernels (records accumulated in HBM, text written on the GPU)."""
    from . import pipeline
    from .ingest import FastaIndex, QueryShard
    ix = pipeline.make_index_set(gpu, names, lens, parts, first)
    fx = FastaIndex(query_fasta)
    sh = QueryShard.from_fasta(gpu, fx, 0, fx.n, batch_bases)
    acc = pipeline.PafAcc(gpu)
    pipeline.map_shard(gpu, ix, sh, acc)
    return pipeline.emit_paf_bytes(gpu, ix, sh, acc, {})


def cmd_map(argv: Sequence[str]) -> int:
    """scripts/minimap2.sh: build the index unless INDEX_PATH is non-empty (:10-19), then map
    input/*.fna with asm10 (:23).  The device index is persisted as INDEX_PATH.hymet beside a
    manifest in INDEX_PATH, so a warm call only loads it (no sketching, no sorting)."""
    if len(argv) != 4:
        print("usage: map INPUT_DIR REFERENCE_FASTA INDEX_PATH PAF_OUT", file=sys.stderr)
        return 2
    input_dir, ref_fasta, index_path, paf_out = argv
    from . import mapper as mp
    from ._lib import Gpu
    from .seqio import read_fasta
    split = os.environ.get("SPLIT_IDX", "2g")
    cached = os.path.exists(index_path) and os.path.getsize(index_path) > 0
    try:
        gpu = Gpu(int(os.environ.get("HYMET_DEVICE", "0")))
        loaded = None
        if not cached:
            print("Creating index with minimap2...")
        else:
            print(f"Using cached minimap2 index: {index_path}")
            loaded = mp.load_index(gpu, index_path, ref_fasta, split)
        if loaded is None:   # fresh, or a CPU minimap2 .mmi we keep untouched: build in HBM
            # HYMET_INDEX_MINI_BATCH: the index reader's mini-batch (minimap2's 50 Mbp chunking)
            mini = float(os.environ.get("HYMET_INDEX_MINI_BATCH", "50e6"))
            parts, names, lens, first = build_parts(gpu, read_fasta([ref_fasta]), split, mini)
            if not cached:
                mp.save_index(index_path, parts, names, lens, first, ref_fasta, split)
        else:
            parts, names, lens, first = loaded
    except Exception as e:  # minimap2.sh:13-16
        print(f"Error creating index with minimap2. ({e})")
        return 1
    print("Running alignment with minimap2...")
    try:
        data = map_paf(gpu, parts, names, lens, first, read_query_files(_fna_files(input_dir)))
        with open(paf_out, "wb") as f:
            f.write(data)
    except Exception as e:  # minimap2.sh:25-29
        print(f"Error running alignment with minimap2. ({e})")
        return 1
    print(f"Alignment completed successfully! Results saved to {paf_out}.")
    return 0


# --------------------------------------------------- classify (classification*.py)
def cmd_classify(argv: Sequence[str], legacy: bool = False) -> int:
    from . import classify as cls
    from ._lib import Gpu
    p = argparse.ArgumentParser(prog="classify")
    p.add_argument("--paf", required=True)
    p.add_argument("--taxonomy", required=True)
    p.add_argument("--hierarchy", required=True)
    p.add_argument("--output", required=True)
    p.add_argument("--processes", type=int, default=4)   # accepted; the GPU does the fan-out
    a = p.parse_args(argv)
    logging.basicConfig(level=logging.INFO, format="%(asctime)s - %(levelname)s - %(message)s")
    gpu = Gpu(int(os.environ.get("HYMET_DEVICE", "0")))
    variant = cls.LEGACY if legacy else cls.CAMI
    c = cls.Classifier(gpu, a.taxonomy, a.hierarchy, variant)
    paf = cls.read_paf(a.paf, variant)
    if legacy and len(paf.queries) == 0:
        raise ZeroDivisionError("division by zero")  # classification.py:182 on an empty PAF
    res = c.run(paf)
    rows = c.rows(res)
    with open(a.output, "wb") as f:
        f.write(c.tsv_bytes(res, rows))
    n = len(rows)
    k = sum(1 for r in rows if r[1] != "Unknown")
    logging.info(f"Classification complete. Results saved to {a.output}")
    logging.info(f"Classified: {k}/{n} ({(k / n if n else 0):.1%})")
    return 0


# ------------------------------------------- CAMI export / taxdump
def cmd_hymet2cami(argv: Sequence[str]) -> int:
    """tools/hymet2cami.py <classified_sequences.tsv>: CAMI profile on stdout, progress on
    stderr; names.dmp / nodes.dmp from TAXONKIT_DB (default <repo>/taxonomy_files)."""
    from pathlib import Path
    from .taxonomy import hymet2cami
    if len(argv) != 1:
        print("Usage: hymet2cami.py <classified_sequences.tsv>", file=sys.stderr)
        return 1
    path = Path(argv[0]).resolve()
    if not path.is_file():
        print(f"Missing classified_sequences TSV: {path}", file=sys.stderr)
        return 1
    taxdb = os.environ.get("TAXONKIT_DB", str(Path(__file__).resolve().parents[1] / "taxonomy_files"))
    sys.stdout.write(hymet2cami(str(path), taxdb))
    return 0


def cmd_taxonomy_hierarchy(argv: Sequence[str]) -> int:
    """scripts/taxonomy_hierarchy.py: taxonomy_files/{names,nodes}.dmp -> data/taxonomy_hierarchy.tsv
    (paths relative to the working directory, as the reference; or NAMES NODES OUT)."""
    from .taxonomy import hierarchy_tsv
    if argv and len(argv) != 3:
        print("usage: taxonomy-hierarchy [NAMES_DMP NODES_DMP OUT_TSV]", file=sys.stderr)
        return 2
    names, nodes, out = argv if argv else (os.path.join(".", "taxonomy_files", "names.dmp"),
                                           os.path.join(".", "taxonomy_files", "nodes.dmp"),
                                           os.path.join(".", "data", "taxonomy_hierarchy.tsv"))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    for p in (names, nodes):
        if not os.path.exists(p):
            raise FileNotFoundError(f"File {p} not found.")
    print("Loading data from files...")
    data = hierarchy_tsv(names, nodes)
    print("Generating taxonomy_hierarchy.tsv...")
    with open(out, "wb") as f:
        f.write(data)
    print(f"File generated successfully: {out}")
    return 0


def cmd_download_db(argv: Sequence[str]) -> int:
    """scripts/downloadDB.py <genomes_file> <output_dir> <taxonomy_file> <cache_dir>, offline
    (SURVEY.md §8f-2): genomes already in output_dir, summaries cached in cache_dir."""
    from .cache import build_cache
    if len(argv) != 4:
        print("Usage: python3 download_genomes.py <genomes_file> <output_dir> <taxonomy_file> <cache_dir>")
        return 1
    build_cache(argv[0], argv[1], argv[2], argv[3], log=lambda m: print(m, file=sys.stderr))
    return 0


# ------------------------------------------------------------------ sketch (mash sketch)
SKETCH_USAGE = "usage: sketch [-k K] [-s S] [-S SEED] [-i] [-Z] [-l] [-r] [-m M] [-g SIZE] [--batch-bases SIZE] -o PREFIX FILE..."


def parse_size(text: str) -> int:
    """A genome size as `mash sketch -g` takes it: a positive number with an optional k / m / g /
    t suffix in either case (4.6m = 4,600,000)."""
    mult = {"k": 10 ** 3, "m": 10 ** 6, "g": 10 ** 9, "t": 10 ** 12}.get(text[-1:].lower())
    v = float(text[:-1] if mult else text) * (mult or 1)
    if not v >= 1:
        raise ValueError(f"{text}: not a size")
    return int(round(v))


def sketch_args(argv: Sequence[str]):
    """`mash sketch`'s flag letters.  Returns the parsed namespace, or None after printing the
    usage line (unknown flag, -n, no -o, no FILE, -m below 1, -r or -m above 1 with -i, a -g or
    --batch-bases that is no size).  a.reads is set by -r and by -m above 1, a.batch_bases is
    sketch.DEFAULT_BATCH_BASES unless --batch-bases gives it."""
    class _Parser(argparse.ArgumentParser):
        def error(self, message):
            raise ValueError(message)

    p = _Parser(prog="sketch", add_help=False, allow_abbrev=False)
    p.add_argument("-k", type=int, default=21, dest="k")
    p.add_argument("-s", type=int, default=1000, dest="s")
    p.add_argument("-S", type=int, default=42, dest="seed")
    p.add_argument("-i", action="store_true", dest="individual")
    p.add_argument("-Z", action="store_true", dest="preserve_case")
    p.add_argument("-l", action="store_true", dest="lists")
    p.add_argument("-n", action="store_true", dest="noncanonical")
    p.add_argument("-r", action="store_true", dest="reads")
    p.add_argument("-m", type=int, default=1, dest="min_copies")
    p.add_argument("-g", type=parse_size, default=None, dest="genome_size")
    p.add_argument("--batch-bases", type=parse_size, default=None, dest="batch_bases")
    p.add_argument("-o", dest="out")
    p.add_argument("-h", action="store_true", dest="help")
    p.add_argument("files", nargs="*")
    try:
        a = p.parse_args(list(argv))
        if a.help:
            print(cmd_sketch.__doc__, file=sys.stderr)
            raise ValueError("")
        if a.noncanonical:
            raise ValueError("-n: noncanonical sketches are not supported")
        if a.min_copies < 1:
            raise ValueError(f"-m {a.min_copies}: the minimum number of copies is at least 1")
        a.reads = a.reads or a.min_copies > 1
        if a.reads and a.individual:
            raise ValueError("-r / -m does not go with -i: a read set is one sketch per FILE")
        if a.batch_bases is None:
            from .sketch import DEFAULT_BATCH_BASES
            a.batch_bases = DEFAULT_BATCH_BASES
        if not a.out:
            raise ValueError("-o PREFIX is required")
        if not a.files:
            raise ValueError("no input FILE")
    except ValueError as e:
        if str(e):
            print(f"sketch: {e}", file=sys.stderr)
        print(SKETCH_USAGE, file=sys.stderr)
        return None
    return a


def expand_lists(files: Sequence[str]) -> List[str]:
    """-l: each FILE is a list of paths, one per line (blank lines skipped)."""
    out: List[str] = []
    for lf in files:
        with open(lf, "r", encoding="utf-8") as f:
            out.extend(l.strip() for l in f if l.strip())
    return out


def cmd_sketch(argv: Sequence[str]) -> int:
    """mash sketch [-k K] [-s S] [-S SEED] [-i] [-Z] [-l] [-r] [-m M] [-g SIZE] [--batch-bases SIZE] -o PREFIX FILE...:
    sketch each FILE (each record with -i) on the GPU and write PREFIX.msh (the suffix is not
    doubled).  A FILE is FASTA or FASTQ (gzip too).
      -k  k-mer size, 1..32 (21)        -s  sketch size (1000)       -S  hash seed (42)
      -i  one reference per sequence    -Z  preserve case            -l  FILEs list paths
      -r  each FILE is a read set: one sketch per FILE, its length the estimated genome size;
          one stderr line per FILE with that estimate and the estimated coverage
      -m  with -r: keep only k-mers seen at least M times in the FILE (1); M > 1 implies -r
      -g  with -r: the genome size to record instead of the estimate (k / m / g suffix allowed)
      --batch-bases  bases read and sketched per batch (512 Mi; k / m / g suffix allowed): the
          host-memory knob.  A read set (-r) larger than this is never held whole: it is read
          batch by batch and streamed through the GPU, to the same sketch
    Known limits: -n (noncanonical), protein alphabets and the Bloom filter (-b) are not
    supported, -r does not go with -i, and hash lists are always written 64 bits wide, also for
    k <= 16 where Mash writes 32-bit lists (this project's reader widens either form)."""
    a = sketch_args(argv)
    if a is None:
        return 2
    from . import sketch as sk
    from ._lib import Gpu
    from .msh import write_msh
    files = expand_lists(a.files) if a.lists else list(a.files)
    out = a.out if a.out.endswith(".msh") else a.out + ".msh"
    gpu = Gpu(int(os.environ.get("HYMET_DEVICE", "0")))
    print("Sketching...", file=sys.stderr)
    info = []
    try:
        db = sk.sketch_files(gpu, files, k=a.k, seed=a.seed, s=a.s, individual=a.individual, preserve_case=a.preserve_case,
                             reads=a.reads, min_copies=a.min_copies, genome_size=a.genome_size, read_info=info,
                             batch_bases=a.batch_bases)
    except ValueError as e:
        print(f"ERROR: {e}", file=sys.stderr)
        return 1
    for name, size, cov in info:
        print(f"{name}: estimated genome size {size:g}, estimated coverage {cov:.3g}", file=sys.stderr)
    if db.n_refs == 0:
        print("ERROR: no sequences to sketch.", file=sys.stderr)
        return 1
    print(f"Writing to {out}...", file=sys.stderr)
    write_msh(db, out)
    return 0


# ------------------------------------------------------------------ dist (mash dist)
DIST_USAGE = "usage: dist [-d D] [-v P] [-t] [--sparse] [--top K] [-i] [-l] [-r] [-m M] [--batch-bases SIZE] REF.msh QUERY..."


def dist_args(argv: Sequence[str]):
    """`mash dist`'s flag letters.  Returns the parsed namespace, or None after printing the
    usage line (unknown flag, no REF.msh, no QUERY, -m below 1, -r or -m above 1 with -i or with
    nothing but .msh QUERYs, a --batch-bases that is no size).  a.reads is set by -r and by -m
    above 1, a.batch_bases is sketch.DEFAULT_BATCH_BASES unless --batch-bases gives it."""
    class _Parser(argparse.ArgumentParser):
        def error(self, message):
            raise ValueError(message)

    p = _Parser(prog="dist", add_help=False, allow_abbrev=False)
    p.add_argument("-r", action="store_true", dest="reads")
    p.add_argument("-m", type=int, default=1, dest="min_copies")
    p.add_argument("--batch-bases", type=parse_size, default=None, dest="batch_bases")
    p.add_argument("-d", type=float, default=None, dest="max_dist")
    p.add_argument("-v", type=float, default=1.0, dest="max_p")
    p.add_argument("-t", action="store_true", dest="table")
    p.add_argument("--sparse", action="store_true", dest="sparse")
    p.add_argument("--top", type=int, default=None, dest="top")
    p.add_argument("-i", action="store_true", dest="individual")
    p.add_argument("-l", action="store_true", dest="lists")
    p.add_argument("-h", action="store_true", dest="help")
    p.add_argument("files", nargs="*")
    try:
        a = p.parse_args(list(argv))
        if a.help:
            print(cmd_dist.__doc__, file=sys.stderr)
            raise ValueError("")
        if not a.files:
            raise ValueError("no REF.msh")
        if len(a.files) < 2:
            raise ValueError("no QUERY")
        if a.min_copies < 1:
            raise ValueError(f"-m {a.min_copies}: the minimum number of copies is at least 1")
        a.reads = a.reads or a.min_copies > 1
        if a.batch_bases is None:
            from .sketch import DEFAULT_BATCH_BASES
            a.batch_bases = DEFAULT_BATCH_BASES
        if a.reads and a.individual:
            raise ValueError("-r / -m does not go with -i: a read set is one sketch per QUERY")
        if a.reads and not a.lists and all(q.endswith(".msh") for q in a.files[1:]):
            raise ValueError("-r / -m apply to sequence QUERYs: every QUERY is a .msh")
        if a.sparse and a.table:
            raise ValueError("--sparse does not go with -t: the table holds every pair")
        if a.sparse and a.max_dist is None:
            raise ValueError("--sparse needs a distance threshold: give -d D with D < 1")
        if a.sparse and not a.max_dist < 1.0:
            raise ValueError(f"--sparse with -d {a.max_dist:g}: the distance threshold must be below 1")
        if a.top is not None:
            from .mashdist import topk_max
            if a.table:
                raise ValueError("--top does not go with -t: the table holds every pair")
            if a.max_p < 1.0:
                raise ValueError("--top does not go with -v P below 1: a p-value filter after the selection "
                                 "would return fewer than K")
            if not 1 <= a.top <= topk_max():
                raise ValueError(f"--top {a.top}: K must be in 1..{topk_max()}")
        a.top = a.top or 0
        if a.max_dist is None:
            a.max_dist = 1.0
    except ValueError as e:
        if str(e):
            print(f"dist: {e}", file=sys.stderr)
        print(DIST_USAGE, file=sys.stderr)
        return None
    a.ref, a.queries = a.files[0], a.files[1:]
    return a


def cmd_dist(argv: Sequence[str]) -> int:
    """mash dist [-d D] [-v P] [-t] [--sparse] [--top K] [-i] [-l] [-r] [-m M] [--batch-bases SIZE] REF.msh QUERY...: the distance of every QUERY
    sketch to every sketch of REF.msh, computed on the GPU; one row per pair on stdout
    (reference, query, distance, p-value, shared/compared hashes), query-major.
      -d  keep pairs with distance <= D (1)     -v  keep pairs with p-value <= P (1)
      -t  table output (ignores -d and -v)      -l  QUERYs list paths
      -i  one query per sequence of a FASTA QUERY
      --sparse  with -d D, D < 1: visit only the pairs that share a hash (the same rows)
      --top K   per query only its K nearest references (of those within -d D), nearest first;
                equal common/denom ratios in reference order.  Not with -t or -v P < 1.
      -r  each sequence QUERY is a read set (one sketch per QUERY)
      -m  with -r: keep only k-mers seen at least M times in the QUERY (1); M > 1 implies -r
      --batch-bases  bases of sequence QUERYs read and sketched per batch (512 Mi; k / m / g suffix
                allowed); a read-set QUERY larger than this is streamed, to the same sketch
    A QUERY ending in .msh is loaded; any other is FASTA or FASTQ (gzip too), sketched on the GPU
    with REF.msh's k-mer size, seed, sketch size and case rule.  -r / -m need such a QUERY."""
    a = dist_args(argv)
    if a is None:
        return 2
    from . import mashdist as md
    from . import sketch as sk
    from ._lib import Gpu
    from .msh import load_db
    ref = load_db(a.ref)
    queries = expand_lists(a.queries) if a.lists else list(a.queries)
    if not queries:
        print("dist: no QUERY", file=sys.stderr)
        print(DIST_USAGE, file=sys.stderr)
        return 2
    if a.reads and all(q.endswith(".msh") for q in queries):
        print("dist: -r / -m apply to sequence QUERYs: every QUERY is a .msh", file=sys.stderr)
        print(DIST_USAGE, file=sys.stderr)
        return 2
    gpu = Gpu(int(os.environ.get("HYMET_DEVICE", "0")))
    dbs, fasta = [], []

    def flush():      # consecutive FASTA queries are sketched in one call
        if fasta:
            dbs.append(sk.sketch_files(gpu, fasta, k=ref.k, seed=ref.seed, s=ref.sketch_size, individual=a.individual,
                                       preserve_case=ref.preserve_case, reads=a.reads, min_copies=a.min_copies,
                                       batch_bases=a.batch_bases))
            fasta.clear()

    try:
        md.check_compatible(ref, ref)      # a noncanonical REF.msh is refused before anything is sketched
        for q in queries:
            if q.endswith(".msh"):
                flush()
                dbs.append(load_db(q))
                md.check_compatible(ref, dbs[-1])
            else:
                fasta.append(q)
        flush()
    except ValueError as e:
        print(f"ERROR: {e}", file=sys.stderr)
        return 1
    qry = md.concat_dbs(dbs)
    if a.table:
        parts = list(md.dist_blocks(gpu, ref, qry, 1.0))
        common = np.concatenate([p[2] for p in parts]) if parts else np.zeros(0, np.int32)
        denom = np.concatenate([p[3] for p in parts]) if parts else np.zeros(0, np.int32)
        sys.stdout.write("".join(l + "\n" for l in md.format_table(ref, qry, common, denom)))
        return 0
    for qi, ri, common, denom in md.dist_blocks(gpu, ref, qry, a.max_dist, block_bytes=1 << 26, sparse=a.sparse,
                                                top=a.top):
        sys.stdout.write("".join(l + "\n" for l in md.format_lines(ref, qry, qi, ri, common, denom, a.max_dist, a.max_p)))
    return 0


# ------------------------------------------------------------------ derep / triangle
DEREP_USAGE = ("usage: derep [-d D] [-r longest|first] [-o PREFIX] [-k K] [-s S] [-S SEED] [--greedy] [--sparse] [-i] [-l] "
               "INPUT...")
TRIANGLE_USAGE = "usage: triangle [-i] [-l] INPUT..."


def derep_args(argv: Sequence[str]):
    """Returns the parsed namespace, or None after printing the usage line (unknown flag, no
    INPUT, -d outside [0, 1), an unknown -r rule)."""
    class _Parser(argparse.ArgumentParser):
        def error(self, message):
            raise ValueError(message)

    p = _Parser(prog="derep", add_help=False, allow_abbrev=False)
    p.add_argument("-d", type=float, default=0.05, dest="max_dist")
    p.add_argument("-r", default="longest", dest="rule")
    p.add_argument("-o", dest="out")
    p.add_argument("-k", type=int, default=21, dest="k")
    p.add_argument("-s", type=int, default=1000, dest="s")
    p.add_argument("-S", type=int, default=42, dest="seed")
    p.add_argument("--sparse", action="store_true", dest="sparse")
    p.add_argument("--greedy", action="store_true", dest="greedy")
    p.add_argument("-i", action="store_true", dest="individual")
    p.add_argument("-l", action="store_true", dest="lists")
    p.add_argument("-h", action="store_true", dest="help")
    p.add_argument("files", nargs="*")
    try:
        a = p.parse_args(list(argv))
        if a.help:
            print(cmd_derep.__doc__, file=sys.stderr)
            raise ValueError("")
        if not 0.0 <= a.max_dist < 1.0:
            raise ValueError(f"-d {a.max_dist:g}: the distance threshold must be in [0, 1)")
        if a.rule not in ("longest", "first"):
            raise ValueError(f"-r {a.rule}: expected longest or first")
        if not a.files:
            raise ValueError("no INPUT")
    except ValueError as e:
        if str(e):
            print(f"derep: {e}", file=sys.stderr)
        print(DEREP_USAGE, file=sys.stderr)
        return None
    return a


def triangle_args(argv: Sequence[str]):
    """Returns the parsed namespace, or None after printing the usage line (unknown flag, no INPUT)."""
    class _Parser(argparse.ArgumentParser):
        def error(self, message):
            raise ValueError(message)

    p = _Parser(prog="triangle", add_help=False, allow_abbrev=False)
    p.set_defaults(k=21, s=1000, seed=42)      # cmd_sketch's defaults, for FASTA INPUTs
    p.add_argument("-i", action="store_true", dest="individual")
    p.add_argument("-l", action="store_true", dest="lists")
    p.add_argument("-h", action="store_true", dest="help")
    p.add_argument("files", nargs="*")
    try:
        a = p.parse_args(list(argv))
        if a.help:
            print(cmd_triangle.__doc__, file=sys.stderr)
            raise ValueError("")
        if not a.files:
            raise ValueError("no INPUT")
    except ValueError as e:
        if str(e):
            print(f"triangle: {e}", file=sys.stderr)
        print(TRIANGLE_USAGE, file=sys.stderr)
        return None
    return a


def _load_inputs(gpu, inputs: Sequence[str], a):
    """The INPUTs of derep / triangle as one sketch DB: a path ending in .msh is loaded, any other
    is FASTA and sketched on the GPU with the parameters of the first .msh INPUT if there is one,
    else with -k / -s / -S.  ValueError when two inputs do not go together."""
    from . import mashdist as md
    from . import sketch as sk
    from .msh import load_db
    loaded = {p: load_db(p) for p in inputs if p.endswith(".msh")}
    first = next(iter(loaded.values()), None)
    if first is not None:
        md.check_compatible(first, first)
        par = dict(k=first.k, seed=first.seed, s=first.sketch_size, preserve_case=first.preserve_case)
    else:
        par = dict(k=a.k, seed=a.seed, s=a.s, preserve_case=False)
    dbs, fasta = [], []

    def flush():      # consecutive FASTA inputs are sketched in one call
        if fasta:
            dbs.append(sk.sketch_files(gpu, list(fasta), individual=a.individual, **par))
            fasta.clear()

    for p in inputs:
        if p in loaded:
            flush()
            dbs.append(loaded[p])
        else:
            fasta.append(p)
    flush()
    for d in dbs:
        md.check_compatible(dbs[0], d)
    return md.concat_dbs(dbs)


def cmd_derep(argv: Sequence[str]) -> int:
    """derep [-d D] [-r longest|first] [-o PREFIX] [-k K] [-s S] [-S SEED] [--greedy] [--sparse] [-i] [-l] INPUT...:
    single-linkage clusters of all INPUT sketches under the Mash distance D, computed on the GPU
    (each pair once, the clusters formed in device memory); one row per sketch on stdout in input
    order (member, representative, cluster index, cluster size) and a summary line on stderr.
      -d  sketches within distance D share a cluster, 0 <= D < 1 (0.05)
      -r  a cluster's representative: its longest genome (longest) or its first member (first)
      -o  write PREFIX.msh holding the representatives only (the suffix is not doubled)
      -i  one sketch per sequence of a FASTA INPUT      -l  INPUTs list paths
      --sparse  visit only the pairs that share a hash (the same clusters)
      --greedy  greedy representatives instead of single linkage: the sketches are taken in the
                order of -r (longest genome first, or input order), one is kept as a representative
                unless an earlier representative lies within D of it, and then joins the nearest
                such; every member lies within D of its representative, no two representatives do
      -k -s -S  k-mer size, sketch size and seed for FASTA INPUTs when no INPUT is a .msh
                (21, 1000, 42); otherwise the first .msh INPUT's parameters are used
    An INPUT ending in .msh is loaded; any other is FASTA or FASTQ (gzip too), sketched on the GPU."""
    a = derep_args(argv)
    if a is None:
        return 2
    from . import derep as dr
    from ._lib import Gpu
    from .msh import write_msh
    inputs = expand_lists(a.files) if a.lists else list(a.files)
    if not inputs:
        print("derep: no INPUT", file=sys.stderr)
        print(DEREP_USAGE, file=sys.stderr)
        return 2
    gpu = Gpu(int(os.environ.get("HYMET_DEVICE", "0")))
    try:
        db = _load_inputs(gpu, inputs, a)
    except ValueError as e:
        print(f"ERROR: {e}", file=sys.stderr)
        return 1
    if db.n_refs == 0:
        print("ERROR: no sequences to sketch.", file=sys.stderr)
        return 1
    if a.greedy:
        res = dr.cluster_greedy(gpu, db, a.max_dist, rule=a.rule, sparse=a.sparse)
        labels, reps = dr.greedy_labels(res.rep), dr.greedy_representatives(res.rep)
    else:
        res = dr.cluster(gpu, db, a.max_dist, sparse=a.sparse)
        labels, reps = res.labels, dr.representatives(res.labels, db.lengths, a.rule)
    sys.stdout.write("".join(l + "\n" for l in dr.format_rows(db, labels, reps)))
    print(f"derep: {db.n_refs} sketches, {res.n_links} links, {len(reps)} clusters" + (" (greedy)" if a.greedy else ""),
          file=sys.stderr)
    if a.out:
        out = a.out if a.out.endswith(".msh") else a.out + ".msh"
        print(f"Writing to {out}...", file=sys.stderr)
        write_msh(dr.subset_db(db, reps), out)
    return 0


def cmd_triangle(argv: Sequence[str]) -> int:
    """triangle [-i] [-l] INPUT...: the lower-triangular distance matrix of all INPUT sketches,
    computed on the GPU: a first line with the number of sketches, then per sketch its name and
    the distance to every earlier one.
      -i  one sketch per sequence of a FASTA INPUT      -l  INPUTs list paths
    An INPUT ending in .msh is loaded; any other is FASTA or FASTQ (gzip too), sketched on the GPU with
    the first .msh INPUT's parameters, or k = 21, s = 1000, seed 42 when there is none."""
    a = triangle_args(argv)
    if a is None:
        return 2
    from . import derep as dr
    from ._lib import Gpu
    inputs = expand_lists(a.files) if a.lists else list(a.files)
    if not inputs:
        print("triangle: no INPUT", file=sys.stderr)
        print(TRIANGLE_USAGE, file=sys.stderr)
        return 2
    gpu = Gpu(int(os.environ.get("HYMET_DEVICE", "0")))
    try:
        db = _load_inputs(gpu, inputs, a)
    except ValueError as e:
        print(f"ERROR: {e}", file=sys.stderr)
        return 1
    for line in dr.triangle_lines(gpu, db):
        sys.stdout.write(line + "\n")
    return 0


# ------------------------------------------------------------------ mash-screen (mash screen)
MASH_SCREEN_USAGE = "usage: mash-screen [-w] [-i MIN_IDENTITY] [-v MAX_P] DB.msh FILE..."


def mash_screen_args(argv: Sequence[str]):
    """`mash screen`'s flag letters.  Returns the parsed namespace, or None after printing the
    usage line (unknown flag, no DB.msh, no FILE)."""
    class _Parser(argparse.ArgumentParser):
        def error(self, message):
            raise ValueError(message)

    p = _Parser(prog="mash-screen", add_help=False, allow_abbrev=False)
    p.add_argument("-w", action="store_true", dest="winner")
    p.add_argument("-i", type=float, default=0.0, dest="min_identity")
    p.add_argument("-v", type=float, default=1.0, dest="max_p")
    p.add_argument("-h", action="store_true", dest="help")
    p.add_argument("files", nargs="*")
    try:
        a = p.parse_args(list(argv))
        if a.help:
            print(cmd_mash_screen.__doc__, file=sys.stderr)
            raise ValueError("")
        if not a.files:
            raise ValueError("no DB.msh")
        if len(a.files) < 2:
            raise ValueError("no input FILE")
    except ValueError as e:
        if str(e):
            print(f"mash-screen: {e}", file=sys.stderr)
        print(MASH_SCREEN_USAGE, file=sys.stderr)
        return None
    a.db, a.inputs = a.files[0], a.files[1:]
    return a


def cmd_mash_screen(argv: Sequence[str]) -> int:
    """mash screen [-w] [-i MIN_IDENTITY] [-v MAX_P] DB.msh FILE...: how well each sketch of
    DB.msh is contained in the pooled FILEs (FASTA or FASTQ, gzip too), computed on the GPU; one row per
    reference on stdout in sketch order (identity, shared-hashes, median-multiplicity, p-value,
    name, comment).
      -w  winner-take-all: each hash found in the pool is credited to the best-scoring
          reference holding it, and the rows are recomputed from the credited hashes
      -i  keep rows with identity >= MIN_IDENTITY (0; negative: also references sharing nothing)
      -v  keep rows with p-value <= MAX_P (1)"""
    a = mash_screen_args(argv)
    if a is None:
        return 2
    from . import screen as scr
    from ._lib import Gpu
    from .msh import load_db
    from .seqio import DevicePool, read_seqs
    db = load_db(a.db)
    gpu = Gpu(int(os.environ.get("HYMET_DEVICE", "0")))
    ss = read_seqs(list(a.inputs))
    res = scr.screen(gpu, DevicePool(gpu, ss, DevicePool.ALPHA_MASH), [db], winner=a.winner)[0]
    sys.stdout.write("".join(l + "\n" for l in res.lines(v_max=a.max_p, identity_min=a.min_identity)))
    return 0


def main(argv: Optional[Sequence[str]] = None) -> int:
    argv = list(sys.argv[1:] if argv is None else argv)
    if not argv:
        print(__doc__, file=sys.stderr)
        return 2
    cmd, rest = argv[0], argv[1:]
    if cmd == "screen":
        return cmd_screen(rest)
    if cmd == "limit":
        return cmd_limit(rest)
    if cmd == "map":
        return cmd_map(rest)
    if cmd == "classify":
        return cmd_classify(rest)
    if cmd == "classify-legacy":
        return cmd_classify(rest, legacy=True)
    if cmd == "build-id-map":
        from .fallback import main_build_id_map
        return main_build_id_map(rest)
    if cmd == "mini-classify":
        from .fallback import main_mini_classify
        return main_mini_classify(rest)
    if cmd == "hymet2cami":
        return cmd_hymet2cami(rest)
    if cmd == "taxonomy-hierarchy":
        return cmd_taxonomy_hierarchy(rest)
    if cmd == "download-db":
        return cmd_download_db(rest)
    if cmd == "eval-cami":
        from .evaluate import main as eval_main
        return eval_main(rest)
    if cmd == "sketch":
        return cmd_sketch(rest)
    if cmd == "dist":
        return cmd_dist(rest)
    if cmd == "mash-screen":
        return cmd_mash_screen(rest)
    if cmd == "derep":
        return cmd_derep(rest)
    if cmd == "triangle":
        return cmd_triangle(rest)
    print(f"unknown subcommand {cmd!r}", file=sys.stderr)
    return 2


if __name__ == "__main__":
    sys.exit(main())
