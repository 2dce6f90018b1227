"""GPU dereplication (csrc/mash_dist.hip through hymet_amd.derep, `cli derep`, `cli triangle`):
the triangle against the square hymet_mash_dist (itself pinned by test_mashdist_gpu.py), the
fused filter + union-find against a plain Python union-find, and the whole path on planted
families."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests._cc_ref import labels as cc_labels
from tests._data import mutate, rand_seq
from tests.test_mashdist_gpu import _fasta, dense, make_db, merge_loop, parity_lists

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG = -2
K = 21
FILL = 0xDEADBEEF
TRI_N = (1, 2, 3, 4, 5, 17, 70, 300)


@pytest.fixture(scope="module")
def gpu():
    from hymet_amd._lib import Gpu
    return Gpu(0)


# ------------------------------------------------------------------ triangle parity
def tri(gpu, D, s, q0, q1):
    """One raw hymet_mash_dist_tri call over a pre-filled output: the (q1 - q0) x n block."""
    from hymet_amd._lib import ptr
    torch = gpu.torch
    n = D.n
    out = torch.full((max(1, (q1 - q0) * n),), FILL - (1 << 32), dtype=torch.int32, device=gpu.dev)
    gpu.call("hymet_mash_dist_tri", ptr(D.hashes), D.n_hashes, ptr(D.offsets), n, q0, q1, s, ptr(out))
    gpu.sync()
    return out.cpu().numpy().view(np.uint32)[:(q1 - q0) * n].reshape(q1 - q0, n)


def check_tri(gpu, s, tq):
    from hymet_amd import mashdist as md
    lists = parity_lists(s, max(TRI_N), 1)[0]
    for n in TRI_N:
        db = make_db(lists[:n], s)
        square = dense(gpu, db, db, s)
        D = md.DeviceSketches(gpu, db)
        ranges = {(0, n), (0, 0), (1, n), (n - 1, n), (1, min(n, tq + 2)), (min(n, tq + 1), min(n, 2 * tq + 3)),
                  (n // 2 + 1, max(n // 2 + 1, n - 1)), (min(n, 3), min(n, 3))}
        for q0, q1 in sorted(ranges):
            got = tri(gpu, D, s, q0, q1)
            below = np.arange(n)[None, :] < np.arange(q0, q1)[:, None]
            np.testing.assert_array_equal(got[below], square[q0:q1][below], err_msg=f"s={s} n={n} rows [{q0}, {q1})")
            assert (got[~below] == FILL).all(), f"s={s} n={n} rows [{q0}, {q1}): an entry r >= q was written"


@pytest.mark.parametrize("s", [1, 64, 65, 1000])
def test_triangle_equals_square_tiled(gpu, s):
    tq = gpu.lib.hymet_mash_dist_tile(s)
    assert tq >= 2, "the tiled kernel must be the default here"
    assert any(n in (tq - 1, tq, tq + 1) for n in TRI_N)
    check_tri(gpu, s, tq)


def test_triangle_equals_square_plain(gpu):
    lib = gpu.lib
    before = 0 if lib.hymet_mash_dist_tile(64) >= 2 else 1
    assert lib.hymet_mash_dist_tune(1, -1) == 0
    try:
        assert lib.hymet_mash_dist_tile(64) == 0
        check_tri(gpu, 64, 4)
    finally:
        assert lib.hymet_mash_dist_tune(before, -1) == 0


def test_triangle_argument_checks(gpu):
    from hymet_amd import mashdist as md
    from hymet_amd._lib import ptr
    lists = parity_lists(64, 17, 1)[0]
    D = md.DeviceSketches(gpu, make_db(lists, 64))
    out = gpu.zeros(D.n * D.n, gpu.torch.int32)

    def call(s=64, off=None, n_hashes=None, q0=0, q1=D.n):
        return gpu.lib.hymet_mash_dist_tri(gpu.ctx, ptr(D.hashes), D.n_hashes if n_hashes is None else n_hashes,
                                           ptr(D.offsets if off is None else off), D.n, q0, q1, s, ptr(out))

    assert call() == 0
    for kw in (dict(s=0), dict(s=16385), dict(q1=D.n + 1), dict(q0=-1), dict(q0=3, q1=2), dict(n_hashes=D.n_hashes - 1)):
        assert call(**kw) == E_ARG, kw
    dec = D.offsets.clone()
    dec[3] = dec[4] + 1
    assert call(off=dec) == E_ARG
    gpu.sync()


# ------------------------------------------------------------------ link kernel on crafted blocks
LINK_S = 100
BLOCKINGS = (None, 1, 63, 64, 65, 1000)


def link_table(gpu, s, max_dist=0.05):
    from hymet_amd import mashdist as md
    t = md.min_common_table(s, K, max_dist)
    return t, gpu.torch.from_numpy(t.view(np.int16).copy()).to(gpu.dev)


def run_link(gpu, d_block, n, d_table, s, rows=None, parent=None):
    """hymet_mash_link over the n x n device block in calls of `rows` rows (None: one call), then
    hymet_mash_labels: (rc of the labels call, labels, n_links)."""
    from hymet_amd._lib import ptr
    torch = gpu.torch
    if parent is None:
        parent = torch.arange(max(n, 1), dtype=torch.int32, device=gpu.dev)
    label = torch.full((max(n, 1),), -7, dtype=torch.int32, device=gpu.dev)
    links = gpu.zeros(1, torch.int64)
    step = n if rows is None else rows
    for q0 in range(0, n, max(step, 1)):
        q1 = min(n, q0 + step)
        gpu.call("hymet_mash_link", ptr(d_block[q0 * n:]) if n else None, q1 - q0, n, q0, ptr(d_table), s, ptr(parent),
                 ptr(links))
    if n == 0:
        gpu.call("hymet_mash_link", None, 0, 0, 0, ptr(d_table), s, None, ptr(links))
    rc = gpu.lib.hymet_mash_labels(gpu.ctx, ptr(parent) if n else None, n, ptr(label) if n else None)
    gpu.sync()
    return rc, label[:n].cpu().numpy(), int(links.cpu().item())


def crafted(gpu, n, edges, s):
    """The n x n block of a graph: a passing entry at (max, min) of every edge, failing entries
    elsewhere below the diagonal, and passing entries on and above it, which must have no effect."""
    ok, bad = np.uint32(s << 16 | s), np.uint32(s)
    m = np.full((n, n), bad, np.uint32)
    m[np.triu_indices(n)] = ok
    e = np.asarray(edges, np.int64).reshape(-1, 2)
    m[e.max(axis=1), e.min(axis=1)] = ok
    return gpu.torch.from_numpy(m.view(np.int32).reshape(-1).copy()).to(gpu.dev) if n else gpu.zeros(1, gpu.torch.int32)


def sparse_edges():
    rng = np.random.default_rng(2000)
    e = rng.integers(0, 2000, size=(1500, 2))
    return e[e[:, 0] != e[:, 1]]


CASES = {    # name -> (n, the edges, built when the case runs)
    "n0": (0, lambda: []),
    "n1": (1, lambda: []),
    "path": (4097, lambda: [(i, i + 1) for i in range(4096)]),
    "star": (600, lambda: [(599, i) for i in range(599)]),               # the centre is the last index
    "complete": (1024, lambda: np.argwhere(np.tri(1024, k=-1, dtype=bool))),   # every union contends for root 0
    "even_odd": (501, lambda: [(i, i + 2) for i in range(499)]),
    "sparse": (2000, sparse_edges),
}


@pytest.mark.parametrize("case", list(CASES))
def test_link_matches_union_find(gpu, case):
    n, edges = CASES[case]
    e = np.asarray(edges(), np.int64).reshape(-1, 2)
    want = cc_labels(n, e)
    n_edges = len({(max(a, b), min(a, b)) for a, b in e.tolist()})
    if case == "path":
        assert (want == 0).all()
    if case == "even_odd":
        np.testing.assert_array_equal(want, np.arange(n) % 2)
    if case == "sparse":
        assert len(np.unique(want)) > 1
        linked = {(max(a, b), min(a, b)) for a, b in e.tolist()}
        assert any(want[i] != i and (i, int(want[i])) not in linked for i in range(n)), \
            "no member reaches its root only through others"
    _, d_table = link_table(gpu, LINK_S)
    d_block = crafted(gpu, n, e, LINK_S)
    for rows in BLOCKINGS:
        rc, got, links = run_link(gpu, d_block, n, d_table, LINK_S, rows)
        assert rc == 0
        np.testing.assert_array_equal(got, want, err_msg=f"{case}, blocks of {rows} rows")
        assert links == n_edges, f"{case}, blocks of {rows} rows"


def test_link_filter_boundary(gpu):
    s = 20
    t, d_table = link_table(gpu, s, 0.1)
    assert t[0] == 0 and (t[1:] >= 1).all() and (t[s] <= s)
    n = 2 * (s + 1) + 2
    m = np.full((n, n), s, np.uint32)                      # common 0 of denom s: fails
    m[np.triu_indices(n)] = s << 16 | s
    for d in range(s + 1):
        m[1 + 2 * d, 0] = int(t[d]) << 16 | d              # the smallest common that passes at this denom
        if t[d] >= 1:
            m[2 + 2 * d, 0] = (int(t[d]) - 1) << 16 | d    # one below it
    m[n - 1, 0] = (s + 1) << 16 | (s + 1)                  # a denom past the table
    d_block = gpu.torch.from_numpy(m.view(np.int32).reshape(-1).copy()).to(gpu.dev)
    rc, got, links = run_link(gpu, d_block, n, d_table, s)
    assert rc == 0
    want = np.arange(n)
    want[1:2 * s + 2:2] = 0
    np.testing.assert_array_equal(got, want)
    assert links == s + 1


def test_labels_report_a_parent_above_its_index(gpu):
    torch = gpu.torch
    _, d_table = link_table(gpu, LINK_S)
    d_block = crafted(gpu, 8, [(1, 0)], LINK_S)
    parent = torch.arange(8, dtype=torch.int32, device=gpu.dev)
    parent[3] = 7                                          # inside the array, above its own index
    rc, _, _ = run_link(gpu, d_block, 8, d_table, LINK_S, parent=parent)
    assert rc == E_ARG and b"hymet_mash_labels" in gpu.lib.hymet_last_error()
    parent = torch.arange(8, dtype=torch.int32, device=gpu.dev)
    parent[5] = -1
    rc, _, _ = run_link(gpu, d_block, 8, d_table, LINK_S, parent=parent)
    assert rc == E_ARG
    rc, got, links = run_link(gpu, d_block, 8, d_table, LINK_S)      # the error does not stick
    assert rc == 0 and links == 1
    np.testing.assert_array_equal(got, [0, 0, 2, 3, 4, 5, 6, 7])


@pytest.mark.parametrize("max_dist", [0.05, 0.3])
def test_link_counts_what_dist_select_keeps(gpu, max_dist):
    from hymet_amd import mashdist as md
    s = 64
    lists = parity_lists(s, 70, 1)[0]
    n = len(lists)
    db = make_db(lists, s)
    square = dense(gpu, db, db, s)
    d_block = gpu.torch.from_numpy(square.view(np.int32).reshape(-1).copy()).to(gpu.dev)
    t, d_table = link_table(gpu, s, max_dist)
    row_off, ri, _ = md.select_block(gpu, d_block, n, n, d_table, s)
    qi = np.repeat(np.arange(n), np.diff(row_off))
    below = ri < qi
    assert below.sum() > 0
    rc, got, links = run_link(gpu, d_block, n, d_table, s)
    assert rc == 0 and links == int(below.sum())
    np.testing.assert_array_equal(got, cc_labels(n, zip(qi[below], ri[below])))


# ------------------------------------------------------------------ end to end
S_E2E = 200
FAMILIES = [0, 1, 2, 0, 4, 1, 0, 7, 4, 9, 1, 0]            # the planted clusters, by smallest member


@pytest.fixture(scope="module")
def planted(gpu, tmp_path_factory):
    """12 sequences of about 20 kb: families {0, 3, 6, 11}, {1, 5, 10}, {4, 8} of 1 % mutants and
    three singletons; sequence 11 is the longest of its family.  Sketched on the GPU at s = 200."""
    from hymet_amd import sketch as sk
    from hymet_amd.msh import write_msh
    rng = np.random.default_rng(77)
    base = {f: rand_seq(rng, 20_000) for f in (0, 1, 4)}
    recs = []
    for i, f in enumerate(FAMILIES):
        if f == i and f not in base:
            seq = rand_seq(rng, 20_000)
        elif f == i:
            seq = base[f]
        else:
            seq = mutate(rng, base[f], 0.01)
        if i == 11:
            seq += rand_seq(rng, 1_500)
        recs.append((f"seq{i}", seq))
    d = tmp_path_factory.mktemp("derep")
    (d / "all.fna").write_bytes(_fasta(recs))
    db = sk.sketch_files(gpu, [str(d / "all.fna")], k=K, seed=42, s=S_E2E, individual=True)
    write_msh(db, str(d / "all.msh"))
    return d, recs, db


def test_cluster_finds_the_planted_families(gpu, planted):
    from hymet_amd import derep as dr
    from hymet_amd import mashdist as md
    _, recs, db = planted
    n = db.n_refs
    assert n == 12
    lists = [np.asarray(db.ref_hashes(i), np.uint64).tolist() for i in range(n)]
    edges = []
    for q in range(n):
        for r in range(q):
            c, d = merge_loop(lists[r], lists[q], S_E2E)
            if md.distance(c, d, K) <= 0.05:
                edges.append((q, r))
    want = cc_labels(n, edges)
    np.testing.assert_array_equal(want, FAMILIES)          # the expectation is what was planted
    for bb in (4 * n, 4 * n * 5, 1 << 30):
        res = dr.cluster(gpu, db, 0.05, block_bytes=bb)
        np.testing.assert_array_equal(res.labels, want, err_msg=f"block_bytes={bb}")
        assert res.n_links == len(edges)
    np.testing.assert_array_equal(dr.representatives(res.labels, db.lengths), [11, 1, 2, 4, 7, 9])
    # nothing within the threshold: every sketch alone
    alone = dr.cluster(gpu, db, 0.0)
    np.testing.assert_array_equal(alone.labels, np.arange(n))
    assert alone.n_links == 0


def test_cli_derep_writes_the_representatives(planted):
    from hymet_amd.msh import load_db
    d, recs, db = planted
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + \
        ["-m", "hymet_amd.cli", "derep", "-o", str(d / "reduced"), str(d / "all.msh")]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    reps = {0: "seq11", 1: "seq1", 2: "seq2", 4: "seq4", 7: "seq7", 9: "seq9"}
    index = {0: 0, 1: 1, 2: 2, 4: 3, 7: 4, 9: 5}
    want = [f"seq{i}\t{reps[f]}\t{index[f]}\t{FAMILIES.count(f)}" for i, f in enumerate(FAMILIES)]
    assert r.stdout.splitlines() == want
    assert "derep: 12 sketches, 10 links, 6 clusters" in r.stderr.splitlines()
    out = load_db(str(d / "reduced.msh"))
    keep = [1, 2, 4, 7, 9, 11]                             # the representatives in DB order
    assert out.names == [db.names[i] for i in keep]
    np.testing.assert_array_equal(np.asarray(out.lengths, np.int64)[:6], np.asarray(db.lengths, np.int64)[keep])
    for n, i in enumerate(keep):
        np.testing.assert_array_equal(out.ref_hashes(n), db.ref_hashes(i))
    assert (out.k, out.seed, out.sketch_size) == (db.k, db.seed, db.sketch_size)
    assert not (d / "reduced.msh.msh").exists()


def test_cli_derep_fasta_beside_msh(gpu, planted, capsys):
    from hymet_amd import cli
    d, recs, db = planted
    rng = np.random.default_rng(5)
    extra = [("near4", mutate(rng, recs[4][1], 0.01)), ("new", rand_seq(rng, 20_000))]
    (d / "extra.fna").write_bytes(_fasta(extra))
    assert cli.main(["derep", "-r", "first", "-i", str(d / "all.msh"), str(d / "extra.fna")]) == 0
    cap = capsys.readouterr()
    rows = [l.split("\t") for l in cap.out.splitlines()]
    assert len(rows) == 14
    assert rows[12] == ["near4", "seq4", "3", "3"] and rows[13] == ["new", "new", "6", "1"]
    assert rows[0] == ["seq0", "seq0", "0", "4"]           # -r first
    assert "derep: 14 sketches, 12 links, 7 clusters" in cap.err.splitlines()
    # FASTA alone: -k / -s / -S apply
    assert cli.main(["derep", str(d / "extra.fna"), "-s", "200", "-i"]) == 0
    assert capsys.readouterr().out.splitlines() == ["near4\tnear4\t0\t1", "new\tnew\t1\t1"]


def test_cli_triangle_equals_dist_table(gpu, planted, capsys):
    from hymet_amd import cli
    d, _, db = planted
    path = str(d / "all.msh")
    assert cli.main(["triangle", path]) == 0
    tri_lines = capsys.readouterr().out.splitlines()
    assert cli.main(["dist", "-t", path, path]) == 0
    table = [l.split("\t") for l in capsys.readouterr().out.splitlines()][1:]
    assert tri_lines[0] == "\t12" and len(tri_lines) == 13 and len(table) == 12
    some = set()
    for q, line in enumerate(tri_lines[1:]):
        f = line.split("\t")
        assert f[0] == table[q][0] == db.names[q] and len(f) == 1 + q
        assert [float(x) for x in f[1:]] == [float(x) for x in table[q][1:1 + q]]
        some.update(f[1:])
    assert "1" in some and any(0 < float(x) < 0.05 for x in some)
