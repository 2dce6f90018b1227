"""Winner-take-all screen (`mash screen -w`) on the GPU vs the plain-Python reference
(tests/_winner_ref.py): the kernels on synthetic counts, then the whole screen, the command
line, the stage drop-in and the pipeline on a pool of three organisms with one strain each."""
import numpy as np
import pytest

from tests._data import mutate, rand_seq
from tests._winner_ref import winner_ref

pytestmark = pytest.mark.gpu

ALL_ONES = 2**64 - 1


@pytest.fixture(scope="module")
def gpu():
    from hymet_amd._lib import Gpu
    return Gpu(0)


def _db(hash_lists, lengths, names=None, k=21, s=1000):
    from hymet_amd.msh import SketchDB
    n = len(hash_lists)
    off = np.zeros(n + 1, np.int64)
    off[1:] = np.cumsum([len(h) for h in hash_lists])
    names = names or [f"ref{i}.fna.gz" for i in range(n)]
    return SketchDB(k=k, seed=42, sketch_size=s, names=names, comments=[f"[1 seqs] {x}" for x in names],
                    lengths=np.asarray(lengths, np.int64), offsets=off,
                    hashes=np.concatenate([np.asarray(h, np.uint64) for h in hash_lists]))


def _upload_counts(gpu, db, key_counts):
    """The counts array the count kernel would leave: one counter per key at the smallest DB
    hash index holding it, the all-ones key's at index n_hashes."""
    h = np.asarray(db.hashes, np.uint64)
    n = len(h)
    _, first, inv = np.unique(h, return_index=True, return_inverse=True)
    canon = first[inv]
    canon[h == np.uint64(ALL_ONES)] = n
    counts = np.zeros(n + 1, np.int32)
    for j in range(n):
        counts[canon[j]] = key_counts.get(int(h[j]), 0)
    return gpu.torch.from_numpy(counts).to(gpu.dev)


def _winner_on_counts(gpu, db, key_counts):
    from hymet_amd import screen as scr
    t = scr.ScreenTable(gpu, db)
    counts = _upload_counts(gpu, db, key_counts)
    sh, md = scr.table_stats(gpu, t, counts)
    sh_w, md_w = scr.table_winner(gpu, t, counts, sh)
    return sh, md, sh_w, md_w


# ------------------------------------------------------------------ kernels, synthetic counts
@pytest.fixture(scope="module")
def handmade():
    """40 references over a pool of distinct random keys.  key_counts: key -> pool count."""
    rng = np.random.default_rng(2024)
    keys = [int(x) for x in np.unique(rng.integers(1, 2**63, size=30_000, dtype=np.int64))]
    rng.shuffle(keys)
    it = iter(keys)

    def take(n):
        return [next(it) for _ in range(n)]

    key_counts = {}

    def count(ks, p_hit):
        for x in ks:
            key_counts[x] = int(rng.integers(1, 60)) if rng.random() < p_hit else 0
        return ks

    refs = [[] for _ in range(40)]
    lengths = [int(x) for x in rng.integers(10_000, 5_000_000, size=40)]
    # 0: 5000 hashes, above the 4096 entries the stats kernels keep in LDS; mostly found
    refs[0] = count(take(5000), 0.9)
    # 1, 2: share keys with 0; 1 is found less than 0 (loses them), 2 is found whole (wins them)
    refs[1] = refs[0][100:160] + count(take(140), 0.3)
    refs[2] = [x for x in refs[0][200:400] if key_counts[x] > 0][:60] + count(take(100), 1.0)
    # 3, 4: 30 keys held by two references; 3 (the canonical holder, smaller index) is found
    # poorly, 4 well: the winner is not the canonical holder
    k2 = count(take(30), 0.8)
    refs[3] = k2 + count(take(170), 0.1)
    refs[4] = k2 + count(take(170), 0.95)
    # 5, 6, 7: 30 keys held by three references, the middle one found best
    k3 = count(take(30), 0.8)
    refs[5] = k3 + count(take(170), 0.5)
    refs[6] = k3 + count(take(170), 0.9)
    refs[7] = k3 + count(take(170), 0.2)
    # 10..19: 20 keys held by ten references
    k10 = count(take(20), 0.8)
    for r in range(10, 20):
        refs[r] = k10 + count(take(180), 0.05 + 0.09 * ((r * 7) % 10))
    # 20, 21: identical first-pass shared (150 common keys, 50 private ones all found),
    # different lengths: the longer genome takes the common keys
    com = count(take(150), 0.7)
    refs[20] = com + count(take(50), 1.0)
    refs[21] = com + count(take(50), 1.0)
    lengths[20], lengths[21] = 1_000_000, 2_000_000
    # 22, 23: identical shared and length: the smaller index takes the common keys
    com = count(take(150), 0.7)
    refs[22] = com + count(take(50), 1.0)
    refs[23] = com + count(take(50), 1.0)
    lengths[22] = lengths[23] = 1_500_000
    # 24, 25: the all-ones key (its counter is the extra one at n_hashes) held by both
    key_counts[ALL_ONES] = 9
    refs[24] = count(take(199), 0.4) + [ALL_ONES]
    refs[25] = count(take(199), 0.6) + [ALL_ONES]
    # 26: shorter than the sketch size; 27: empty; 28: nothing found (does not compete)
    refs[26] = count(take(37), 0.6)
    refs[27] = []
    refs[28] = count(take(200), 0.0)
    for r in (8, 9, 29, 30, 31, 32, 33, 34, 35, 36, 37, 38, 39):
        refs[r] = count(take(150), rng.random()) + refs[0][1000 + 20 * r:1010 + 20 * r]
    refs = [sorted(set(r)) for r in refs]         # each sketch ascending, as Mash writes them
    db = _db(refs, lengths, s=200)
    ref = winner_ref(db.offsets, db.hashes, lengths, key_counts, db.k)
    return db, key_counts, ref


def test_kernels_match_reference_on_synthetic_counts(gpu, handmade):
    db, key_counts, (shared, shared_w, median_w) = handmade
    sh, md, sh_w, md_w = _winner_on_counts(gpu, db, key_counts)
    np.testing.assert_array_equal(sh, np.array(shared, np.uint32))
    np.testing.assert_array_equal(sh_w, np.array(shared_w, np.uint32))
    np.testing.assert_array_equal(md_w, np.array(median_w, np.uint32))
    # the case holds what it is meant to hold
    assert db.offsets[1] - db.offsets[0] > 4096 and shared_w[0] > 4096
    assert 0 < shared_w[3] < shared[3] and shared_w[4] == shared[4]          # canonical holder 3 loses to 4
    assert shared[20] == shared[21] and shared_w[21] == shared[21] and shared_w[20] == 50
    assert shared[22] == shared[23] and shared_w[22] == shared[22] and shared_w[23] == 50
    assert shared_w[24] + shared_w[25] == shared[24] + shared[25] - 1       # the all-ones key credited once
    assert shared[27] == 0 == shared_w[27] and shared[28] == 0 == shared_w[28]
    assert any(c == 0 for c in key_counts.values())


def test_invariants_on_synthetic_counts(gpu, handmade):
    from hymet_amd.screen import rank_competitors
    db, key_counts, _ = handmade
    sh, md, sh_w, md_w = _winner_on_counts(gpu, db, key_counts)
    held = {int(h) for h in db.hashes}
    assert int(sh_w.sum()) == sum(1 for x in held if key_counts.get(x, 0) > 0)
    assert (sh_w <= sh).all()
    top = int(rank_competitors(db, sh)[0])
    assert sh_w[top] == sh[top] > 0 and md_w[top] == md[top]
    assert ((sh_w == 0) == (md_w == 0)).all()


def test_one_reference_and_no_hit(gpu):
    """One reference keeps everything it found.  A DB the pool does not hit gives all zeros
    without a launch: no screen_winner entry in the profile, which the hit case does leave."""
    rng = np.random.default_rng(8)
    hs = sorted(int(x) for x in np.unique(rng.integers(1, 2**63, size=300, dtype=np.int64)))
    one = _db([hs], [1000], s=300)
    kc = {x: int(rng.integers(0, 5)) for x in hs}
    gpu.prof(True)
    try:
        gpu.prof_reset()
        sh, md, sh_w, md_w = _winner_on_counts(gpu, one, kc)
        gpu.sync()
        assert "screen_winner" in gpu.prof_table()
        shared, shared_w, median_w = winner_ref(one.offsets, one.hashes, [1000], kc, one.k)
        assert shared_w == shared and sh_w.tolist() == shared_w and md_w.tolist() == median_w
        assert sh.tolist() == shared and md.tolist() == median_w and 0 < shared[0] < len(hs)
        cold = _db([hs[:100], hs[100:200], hs[200:]], [1, 2, 3], s=100)
        gpu.prof_reset()
        sh, md, sh_w, md_w = _winner_on_counts(gpu, cold, {})
        gpu.sync()
        assert "screen_winner" not in gpu.prof_table()
        assert sh.tolist() == [0, 0, 0] and sh_w.tolist() == [0, 0, 0] and md_w.tolist() == [0, 0, 0]
        assert sh_w.dtype == np.uint32 and md_w.dtype == np.uint32
    finally:
        gpu.prof(False)


# ------------------------------------------------------------------ end to end
K, SEED, S = 21, 42, 1000


@pytest.fixture(scope="module")
def strains():
    """Three genomes of ~150 kbp, each with a strain 0.5 % away (~90 % of the 21-mers kept),
    a few decoys, and a pool of 40 contigs cut from the three base genomes at 1 %.  The pool's
    count of every DB key comes from the CPU oracle: a DB of one key per reference, whose
    median is that key's count."""
    from oracle import oracle_lib
    rng = np.random.default_rng(77)
    base = [rand_seq(rng, int(n)) for n in (150_000, 140_000, 160_000)]
    genomes, names = [], []
    for i, g in enumerate(base):
        genomes += [g, mutate(rng, g, 0.005)]
        names += [f"GCF_{i:09d}.1_org{i}.fna.gz", f"GCF_{i:09d}.2_org{i}_strain.fna.gz"]
    hl = [np.sort(oracle_lib.sketch([g], K, SEED, S)) for g in genomes]
    lengths = [len(g) for g in genomes]
    for j in range(4):
        hl.append(np.sort(rng.integers(0, 2**63, size=S, dtype=np.int64).astype(np.uint64) * 2 + 1))
        names.append(f"decoy_{j}.fna.gz")
        lengths.append(10**6)
    db = _db(hl, lengths, names)
    recs = []
    for c in range(40):
        g = base[c % 3]
        L = int(rng.integers(5_000, 30_000))
        st = int(rng.integers(0, len(g) - L))
        recs.append((f"ctg{c}", "", mutate(rng, g[st:st + L], 0.01)))
    seqs = [r[2] for r in recs]
    keys = np.unique(db.hashes)
    k_sh, k_md, _, _ = oracle_lib.screen(seqs, K, SEED, S, [keys[i:i + 1] for i in range(len(keys))])
    key_counts = {int(x): int(m) for x, s_, m in zip(keys, k_sh, k_md) if s_}
    first = oracle_lib.screen(seqs, K, SEED, S, [db.ref_hashes(i) for i in range(db.n_refs)])
    return {"db": db, "recs": recs, "key_counts": key_counts, "first": first}


def _expect(case, db):
    """Reference arrays and rows of `db` (references drawn from the case's) for the case's pool."""
    from oracle import select_oracle
    shared, shared_w, median_w = winner_ref(db.offsets, db.hashes, db.lengths, case["key_counts"], db.k)
    refs = [(db.names[i], db.comments[i], int(db.offsets[i + 1] - db.offsets[i])) for i in range(db.n_refs)]

    def rows(v_max=0.9, identity_min=0.0):
        return select_oracle.screen_lines(refs, shared_w, median_w, case["first"][2], db.k, v_max, identity_min)

    return shared, shared_w, median_w, rows


def _pool(gpu, case):
    from hymet_amd.seqio import DevicePool, from_records
    return DevicePool(gpu, from_records(case["recs"]), DevicePool.ALPHA_MASH)


def test_screen_winner_matches_reference(gpu, strains):
    from hymet_amd import screen as scr
    from oracle import select_oracle
    db = strains["db"]
    o_sh, o_md, o_set, o_nk = strains["first"]
    shared, shared_w, median_w, rows = _expect(strains, db)
    np.testing.assert_array_equal(np.array(shared, np.uint32), o_sh)        # the two references agree
    pool = _pool(gpu, strains)
    res = scr.screen(gpu, pool, [db], winner=True)[0]
    assert res.winner is True
    np.testing.assert_array_equal(res.shared, np.array(shared_w, np.uint32))
    np.testing.assert_array_equal(res.median, np.array(median_w, np.uint32))
    np.testing.assert_array_equal(res.shared_first, o_sh)
    np.testing.assert_array_equal(res.median_first, o_md)
    assert res.set_size == o_set and res.n_kmers == o_nk
    assert res.lines() == rows() and res.lines(1.0, -1.0) == rows(1.0, -1.0)
    # every strain loses to its base genome; the base genomes keep what they found
    for i in range(3):
        assert res.shared[2 * i + 1] < res.shared_first[2 * i + 1]
        assert res.shared[2 * i] == res.shared_first[2 * i] > 0
    assert len(res.lines(identity_min=0.9)) == 3 < len(scr.format_screen(db, o_sh, o_md, o_set, identity_min=0.9)) == 6
    # off: as before
    plain = scr.screen(gpu, pool, [db])[0]
    off = scr.screen(gpu, pool, [db], winner=False)[0]
    for r in (plain, off):
        assert r.winner is False
        np.testing.assert_array_equal(r.shared, o_sh)
        np.testing.assert_array_equal(r.median, o_md)
        assert r.shared_first is r.shared and r.median_first is r.median
        refs = [(db.names[i], db.comments[i], int(db.offsets[i + 1] - db.offsets[i])) for i in range(db.n_refs)]
        assert r.lines() == select_oracle.screen_lines(refs, o_sh, o_md, o_set, K)


def _sub_db(db, idx):
    return _db([db.ref_hashes(i) for i in idx], [int(db.lengths[i]) for i in idx], [db.names[i] for i in idx])


def test_screen_winner_two_dbs_are_independent(gpu, strains):
    """Two DBs probed in one pass: a strain whose base genome is in the other DB keeps its keys."""
    from hymet_amd import screen as scr
    db = strains["db"]
    db_a = _sub_db(db, [0, 1, 2, 6, 7])            # org0 and its strain, org1 alone
    db_b = _sub_db(db, [3, 1, 4, 5, 8])            # org1's strain alone, org0's strain alone, org2 and its strain
    out = scr.screen(gpu, _pool(gpu, strains), [db_a, db_b], winner=True)
    for d, r in zip((db_a, db_b), out):
        shared, shared_w, median_w, rows = _expect(strains, d)
        np.testing.assert_array_equal(r.shared_first, np.array(shared, np.uint32))
        np.testing.assert_array_equal(r.shared, np.array(shared_w, np.uint32))
        np.testing.assert_array_equal(r.median, np.array(median_w, np.uint32))
        assert r.lines() == rows()
    a, b = out
    assert a.shared[1] < a.shared_first[1]                     # org0's strain beside org0
    assert b.shared[1] == b.shared_first[1] > 0                # the same strain without it
    assert b.shared[0] == b.shared_first[0] > 0
    assert b.shared[3] < b.shared_first[3]                     # org2's strain beside org2


def _fasta(path, recs):
    with open(path, "w") as f:
        for n, _, s in recs:
            f.write(f">{n}\n")
            for i in range(0, len(s), 80):
                f.write(s[i:i + 80].decode() + "\n")


def test_mash_screen_cli_and_stage_dropin(gpu, strains, tmp_path, capsys, monkeypatch):
    from hymet_amd.cli import main as cli
    from hymet_amd.msh import write_msh
    from oracle import select_oracle
    db, recs = strains["db"], strains["recs"]
    o_sh, o_md, o_set, _ = strains["first"]
    _, _, _, rows = _expect(strains, db)
    refs = [(db.names[i], db.comments[i], int(db.offsets[i + 1] - db.offsets[i])) for i in range(db.n_refs)]
    msh = tmp_path / "strains.msh"
    write_msh(db, msh)
    inp = tmp_path / "input"
    inp.mkdir()
    _fasta(inp / "a.fna", recs[:15])
    _fasta(inp / "b.fna", recs[15:])
    files = [str(inp / "a.fna"), str(inp / "b.fna")]
    monkeypatch.delenv("HYMET_SCREEN_WINNER", raising=False)
    # ---- mash-screen: with -w, without, and with the filters
    capsys.readouterr()
    assert cli(["mash-screen", "-w", str(msh)] + files) == 0
    assert capsys.readouterr().out.splitlines() == rows(1.0, 0.0)
    assert cli(["mash-screen", str(msh)] + files) == 0
    assert capsys.readouterr().out.splitlines() == select_oracle.screen_lines(refs, o_sh, o_md, o_set, K, 1.0, 0.0)
    assert cli(["mash-screen", "-w", "-i", "0.9", "-v", "0.5", str(msh)] + files) == 0
    got = capsys.readouterr().out.splitlines()
    assert got == rows(0.5, 0.9) and len(got) == 3

    # ---- the stage drop-in: unset = as before, set = winner-take-all
    def stage(tag):
        outs = [tmp_path / f"{tag}_{f}" for f in ("screen.tab", "filtered.tab", "sorted.tab", "top_hits.tab", "selected.txt")]
        assert cli(["screen", str(inp), str(msh)] + [str(o) for o in outs] + ["0.90"]) == 0
        capsys.readouterr()
        return [o.read_bytes() for o in outs]

    def want(screen_rows):
        srt = select_oracle.sort_gr(select_oracle.sort_unique_k5(screen_rows))
        _, top, names, _ = select_oracle.select_threshold(srt, "0.90", 2)
        return [("".join(l + "\n" for l in x)).encode() for x in (screen_rows, select_oracle.sort_unique_k5(screen_rows), srt, top, names)]

    plain_rows = select_oracle.screen_lines(refs, o_sh, o_md, o_set, K)
    assert stage("off") == want(plain_rows)
    monkeypatch.setenv("HYMET_SCREEN_WINNER", "0")
    assert stage("zero") == want(plain_rows)
    monkeypatch.setenv("HYMET_SCREEN_WINNER", "1")
    on = stage("on")
    assert on == want(rows()) and on[0] != want(plain_rows)[0]


def test_pipeline_screen_winner(gpu, tmp_path):
    """Config(screen_winner=True) on the smoke run's workload: the screen rows are those of
    screen(..., winner=True) and the selection is a subset of the default's."""
    from hymet_amd import pipeline, screen as scr, select as sel, synth
    from hymet_amd.msh import SketchDB
    from hymet_amd.seqio import DevicePool, from_records
    rng = np.random.default_rng(3)
    w = synth.make_cami(rng, n_taxa=2, per_taxon=3, genome_mbp=(0.2, 0.3), contig_gbp=0.0002, max_contigs=24, name="smoke")
    refs = from_records([(n, "", s) for n, s in zip(w.ref_names, w.refs)])
    hl = scr.sketch_sequences(gpu, DevicePool(gpu, refs, DevicePool.ALPHA_MASH), 21, 42, 1000)
    hl += list(synth.decoy_sketches(rng, 20, 1000))
    off = np.zeros(len(hl) + 1, np.int64)
    off[1:] = np.cumsum([len(h) for h in hl])
    names = [n + ".fna.gz" for n in w.ref_names] + [f"decoy_{i}.fna.gz" for i in range(len(hl) - len(w.ref_names))]
    db = SketchDB(names=names, comments=[f"[1 seqs] {n}" for n in names], lengths=np.ones(len(hl), np.int64),
                  offsets=off, hashes=np.concatenate(hl))
    by_name = {n + ".fna.gz": (n, s) for n, s in zip(w.ref_names, w.refs)}
    tax, hier = tmp_path / "detailed_taxonomy.tsv", tmp_path / "taxonomy_hierarchy.tsv"
    tax.write_text(w.taxonomy_tsv())
    hier.write_text(w.hierarchy_tsv())
    queries = from_records([(n, "", s) for n, s in zip(w.contig_names, w.contigs)])
    out = {}
    for on in (False, True):
        cfg = pipeline.Config(split_idx="1m", index_mini_batch=5e5, map_batch_bases=200_000, screen_winner=on)
        p = pipeline.Pipeline(gpu, [db], lambda ns: from_records([(by_name[n][0], "", by_name[n][1]) for n in ns]),
                              str(tax), str(hier), cfg)
        out[on] = p.run(queries)
    assert pipeline.Config().screen_winner is False
    direct = scr.screen(gpu, DevicePool(gpu, queries, DevicePool.ALPHA_MASH), [db], winner=True)[0]
    got = out[True].screen[0]
    assert got.winner is True and out[False].screen[0].winner is False
    np.testing.assert_array_equal(got.shared, direct.shared)
    np.testing.assert_array_equal(got.median, direct.median)
    np.testing.assert_array_equal(got.shared_first, out[False].screen[0].shared)
    assert out[True].screen_rows[0] == sel.sort_gr(sel.sort_unique_k5(direct.lines(v_max=0.9)))
    assert out[True].selected and set(out[True].selected) <= set(out[False].selected)
    assert (got.shared <= got.shared_first).all() and got.shared.sum() < got.shared_first.sum()
