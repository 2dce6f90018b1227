"""Greedy dereplication on the GPU (csrc/mash_dist.hip hymet_mash_greedy / hymet_mash_greedy_edges
through hymet_amd.derep.cluster_greedy and `cli derep --greedy`) against the sequential walk of
tests/_greedy_ref.py: crafted blocks and CSRs, real pair values, and the whole path."""
import ctypes
import dataclasses
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import _greedy_ref as gr
from tests._cc_ref import labels as cc_labels
from tests._data import mutate, rand_seq
from tests.test_derep_gpu import sparse_edges
from tests.test_mashdist_gpu import _fasta, dense, make_db, merge_loop, parity_lists

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG = -2
K = 21
S = 1000                                                   # crafted blocks: 500 / 1000 must fit
BLOCKINGS = (None, 1, 63, 64, 65, 1000)
FAIL = np.uint32(S)                                        # common 0 of denom S
ABOVE = np.uint32(S << 16 | S)                             # on and above the diagonal: would pass


@pytest.fixture(scope="module")
def gpu():
    from hymet_amd._lib import Gpu
    return Gpu(0)


@pytest.fixture(scope="module")
def any_common(gpu):
    """The filter of the crafted cases: any common >= 1 passes, and 0 / 0."""
    t = np.ones(S + 1, np.uint16)
    t[0] = 0
    return gpu.torch.from_numpy(t.view(np.int16).copy()).to(gpu.dev)


def upload(gpu, a, dtype):
    a = np.ascontiguousarray(a, dtype)
    return gpu.torch.from_numpy(a.copy()).to(gpu.dev) if a.size else gpu.zeros(1, getattr(gpu.torch, np.dtype(dtype).name))


def crafted(gpu, n, pairs):
    """The n x n block of a graph: the pair's packed value at (q, r), failing entries elsewhere
    below the diagonal, and passing entries on and above it, which must have no effect."""
    m = np.full((n, n), FAIL, np.uint32)
    m[np.triu_indices(n)] = ABOVE
    for (q, r), (c, d) in pairs.items():
        m[q, r] = c << 16 | d
    return upload(gpu, m.view(np.int32).reshape(-1), np.int32)


def csr(gpu, n, pairs):
    """The same graph as a host-built CSR: (row_off int64 [n + 1], index int32, value int32) on
    the device, the entries of a row in ascending index order."""
    rows = gr.below(pairs)
    off = np.zeros(n + 1, np.int64)
    idx, val = [], []
    for q in range(n):
        for r, c, d in rows.get(q, ()):
            idx.append(r)
            val.append(c << 16 | d)
        off[q + 1] = len(idx)
    return (upload(gpu, off, np.int64), upload(gpu, idx, np.int32),
            upload(gpu, np.asarray(val, np.uint32).view(np.int32), np.int32))


def fresh(gpu, n):
    return gpu.torch.full((max(n, 1),), -1, dtype=gpu.torch.int32, device=gpu.dev)


def run_greedy(gpu, d_block, n, d_table, s, rows=None, rep=None, q_from=0):
    """hymet_mash_greedy over the n x n device block in calls of `rows` rows (None: one call):
    (rc of the last call made, rep, n_links, [(rows of the call, its rounds)])."""
    from hymet_amd._lib import ptr
    rep = fresh(gpu, n) if rep is None else rep
    links = gpu.zeros(1, gpu.torch.int64)
    step = max(n if rows is None else rows, 1)
    rounds, r, rc = [], ctypes.c_int32(-7), 0
    for q0 in range(q_from, max(n, 1), step):
        q1 = min(n, q0 + step)
        rc = gpu.lib.hymet_mash_greedy(gpu.ctx, ptr(d_block[q0 * n:]) if n else None, q1 - q0, n, q0, ptr(d_table), s,
                                       ptr(rep) if n else None, ptr(links), ctypes.byref(r))
        rounds.append((q1 - q0, r.value))
        if rc:
            break
    gpu.sync()
    return rc, rep[:n].cpu().numpy(), int(links.cpu().item()), rounds


def run_edges(gpu, d_csr, n, s, rows=None, rep=None, q_from=0):
    """hymet_mash_greedy_edges over the n-row device CSR in calls of `rows` rows."""
    from hymet_amd._lib import ptr
    d_off, d_idx, d_val = d_csr
    rep = fresh(gpu, n) if rep is None else rep
    links = gpu.zeros(1, gpu.torch.int64)
    step = max(n if rows is None else rows, 1)
    rounds, r, rc = [], ctypes.c_int32(-7), 0
    for q0 in range(q_from, max(n, 1), step):
        q1 = min(n, q0 + step)
        rc = gpu.lib.hymet_mash_greedy_edges(gpu.ctx, ptr(d_off[q0:]), q1 - q0, q0, ptr(d_idx), ptr(d_val), s, ptr(rep),
                                             ptr(links), ctypes.byref(r))
        rounds.append((q1 - q0, r.value))
        if rc:
            break
    gpu.sync()
    return rc, rep[:n].cpu().numpy(), int(links.cpu().item()), rounds


def in_bound(rounds):
    """Every call ran at least one round over its rows and at most rows + 1."""
    return all((rows == 0 and r == 0) or 1 <= r <= rows + 1 for rows, r in rounds)


# ------------------------------------------------------------------ the crafted graphs
def _values(rng, edges, few=False):
    """A (common, denom) per edge (q, r), q > r: random ones, or drawn from a few rationals that
    several (common, denom) spell, so that ties occur."""
    e = {(int(max(a, b)), int(min(a, b))) for a, b in np.asarray(edges, np.int64).reshape(-1, 2).tolist()}
    spell = [(1, 2), (500, 1000), (2, 4), (1, 3), (2, 6), (2, 3), (3, 4), (750, 1000), (0, 0), (7, 7)]
    out = {}
    for k in sorted(e):
        if few:
            out[k] = spell[int(rng.integers(len(spell)))]
        else:
            d = int(rng.integers(1, S + 1))
            out[k] = (int(rng.integers(1, d + 1)), d)
    return out


def _path():
    return {(i + 1, i): (1 + i % 7, 10 + i % 3) for i in range(1024)}


def _star_first():
    return {(i, 0): (1 + i % 9, 10) for i in range(1, 600)}


def _star_last():                # distinct values: 37 i mod 599 is a bijection of 0..598
    return {(599, i): (1 + 37 * i % 599, S) for i in range(599)}


def _star_last_tie(swap):        # the two nearest are one rational written twice; the rest lie below it
    p = {(599, i): (1 + i % 499, S) for i in range(599)}
    p[(599, 17)], p[(599, 400)] = ((1, 2), (500, 1000)) if swap else ((500, 1000), (1, 2))
    return p


def _complete():
    rng = np.random.default_rng(512)
    return _values(rng, np.argwhere(np.tri(512, k=-1, dtype=bool)))


def _zero_over_zero():           # 0, 1, 2 are apart; 3, 4, 5 choose among them
    return {(3, 0): (999, 1000), (3, 1): (0, 0), (3, 2): (1000, 1000), (4, 0): (0, 0), (4, 1): (1, 1),
            (5, 1): (3, 4), (5, 2): (0, 0)}


def _sparse():
    return _values(np.random.default_rng(2001), sparse_edges())


def _dense_ties():
    rng = np.random.default_rng(300)
    m = np.tril(rng.random((300, 300)) < 0.1, k=-1)
    return _values(rng, np.argwhere(m), few=True)


CASES = {    # name -> (n, the pairs, built when the case runs)
    "n0": (0, dict),
    "n1": (1, dict),
    "path": (1025, _path),
    "star_first": (600, _star_first),
    "star_last": (600, _star_last),
    "star_last_tie": (600, lambda: _star_last_tie(False)),
    "star_last_tie_swapped": (600, lambda: _star_last_tie(True)),
    "complete": (512, _complete),
    "zero_over_zero": (6, _zero_over_zero),
    "sparse": (2000, _sparse),
    "dense_ties": (300, _dense_ties),
}
_WANT = {}


def case(name):
    """(n, pairs, the reference's rep): computed once per case and shared."""
    if name not in _WANT:
        n, make = CASES[name]
        pairs = make()
        _WANT[name] = (n, pairs, gr.greedy(n, pairs))
    return _WANT[name]


def check_case_expectation(name, n, pairs, want):
    """What the case is there for, asserted on the reference before the device is asked."""
    gr.check_members_pass(want, pairs)
    gr.check_representatives_apart(want, pairs)
    i = np.arange(n)
    if name == "path":
        np.testing.assert_array_equal(want, i - i % 2)
    if name in ("star_first", "complete"):
        assert (want == 0).all()
    if name == "star_last":
        np.testing.assert_array_equal(want[:599], i[:599])
        assert want[599] == max(range(599), key=lambda r: pairs[(599, r)][0]) != 598
    if name.startswith("star_last_tie"):
        np.testing.assert_array_equal(want[:599], i[:599])
        assert want[599] == 17
    if name == "zero_over_zero":
        np.testing.assert_array_equal(want, [0, 1, 2, 1, 0, 2])
    if name == "sparse":
        assert 1 < int((want == i).sum()) < n and (want != gr.first_passing(n, pairs)).any()
    if name == "dense_ties":
        assert gr.has_tie(n, pairs, want), "no member has two nearest representatives of one rational"
        assert (want != gr.first_passing(n, pairs)).any()


@pytest.mark.parametrize("name", list(CASES))
def test_greedy_dense_matches_the_walk(gpu, any_common, name):
    n, pairs, want = case(name)
    check_case_expectation(name, n, pairs, want)
    d_block = crafted(gpu, n, pairs)
    for rows in BLOCKINGS:
        rc, got, links, rounds = run_greedy(gpu, d_block, n, any_common, S, rows)
        assert rc == 0, f"{name}, blocks of {rows} rows"
        np.testing.assert_array_equal(got, want, err_msg=f"{name}, blocks of {rows} rows")
        assert links == len(pairs), f"{name}, blocks of {rows} rows"
        assert in_bound(rounds), (name, rows, rounds)       # the path is the deepest chain
        gr.check_members_pass(got, pairs)
        gr.check_representatives_apart(got, pairs)
        if name == "star_first":
            # row 0 is final after the first round whatever the others read of it, so the second
            # settles every row; a call that starts past row 0 needs one
            assert all(r <= (2 if i == 0 else 1) for i, (_, r) in enumerate(rounds)), (rows, rounds)


@pytest.mark.parametrize("name", list(CASES))
def test_greedy_edges_equal_the_dense_result(gpu, any_common, name):
    n, pairs, want = case(name)
    d_csr = csr(gpu, n, pairs)
    _, dense_rep, dense_links, _ = run_greedy(gpu, crafted(gpu, n, pairs), n, any_common, S)
    for rows in (None, 1, 63, 257, 1000):
        rc, got, links, rounds = run_edges(gpu, d_csr, n, S, rows)
        assert rc == 0, f"{name}, calls of {rows} rows"
        np.testing.assert_array_equal(got, dense_rep, err_msg=f"{name}, calls of {rows} rows")
        np.testing.assert_array_equal(got, want, err_msg=f"{name}, calls of {rows} rows")
        assert links == dense_links == len(pairs)
        assert in_bound(rounds), (name, rows, rounds)


def test_greedy_dense_and_edges_alternate(gpu, any_common):
    """Row ranges of one DB may take either entry point, as a sparse run with a dense fallback does."""
    from hymet_amd._lib import ptr
    n, pairs, want = case("sparse")
    d_block, (d_off, d_idx, d_val) = crafted(gpu, n, pairs), csr(gpu, n, pairs)
    rep, links, r = fresh(gpu, n), gpu.zeros(1, gpu.torch.int64), ctypes.c_int32()
    for i, q0 in enumerate(range(0, n, 333)):
        q1 = min(n, q0 + 333)
        if i % 2:
            gpu.call("hymet_mash_greedy", ptr(d_block[q0 * n:]), q1 - q0, n, q0, ptr(any_common), S, ptr(rep), ptr(links),
                     ctypes.byref(r))
        else:
            gpu.call("hymet_mash_greedy_edges", ptr(d_off[q0:]), q1 - q0, q0, ptr(d_idx), ptr(d_val), S, ptr(rep), ptr(links),
                     ctypes.byref(r))
    np.testing.assert_array_equal(rep.cpu().numpy(), want)
    assert int(links.cpu().item()) == len(pairs)


def test_greedy_filter_boundary(gpu):
    """As test_link_filter_boundary builds it: per denom the smallest passing common makes a
    member of row 0's, one below leaves a representative; a denom past the table is ignored."""
    from hymet_amd import mashdist as md
    s = 20
    t = md.min_common_table(s, K, 0.1)
    d_table = gpu.torch.from_numpy(t.view(np.int16).copy()).to(gpu.dev)
    assert t[0] == 0 and (t[1:] >= 1).all() and (t[s] <= s)
    n = 2 * (s + 1) + 2
    m = np.full((n, n), s, np.uint32)                      # common 0 of denom s: fails
    m[np.triu_indices(n)] = s << 16 | s
    for d in range(s + 1):
        m[1 + 2 * d, 0] = int(t[d]) << 16 | d              # the smallest common that passes at this denom
        if t[d] >= 1:
            m[2 + 2 * d, 0] = (int(t[d]) - 1) << 16 | d    # one below it
    m[n - 1, 0] = (s + 1) << 16 | (s + 1)                  # a denom past the table
    d_block = upload(gpu, m.view(np.int32).reshape(-1), np.int32)
    want = np.arange(n)
    want[1:2 * s + 2:2] = 0
    for rows in (None, 5):
        rc, got, links, _ = run_greedy(gpu, d_block, n, d_table, s, rows)
        assert rc == 0
        np.testing.assert_array_equal(got, want)
        assert links == s + 1


# ------------------------------------------------------------------ the contract
def test_greedy_reports_an_undecided_earlier_row(gpu, any_common):
    n, pairs, want = case("zero_over_zero")
    d_block, d_csr = crafted(gpu, n, pairs), csr(gpu, n, pairs)
    # rows [3, 6) over a rep that still holds -1 for the rows they pass with
    rc, _, _, rounds = run_greedy(gpu, d_block, n, any_common, S, rows=3, q_from=3)
    assert rc == E_ARG and b"hymet_mash_greedy" in gpu.lib.hymet_last_error()
    assert len(rounds) == 1 and rounds[0][1] <= 3 + 1      # it gave up inside the bound
    rc, _, _, rounds = run_edges(gpu, d_csr, n, S, rows=3, q_from=3)
    assert rc == E_ARG and b"hymet_mash_greedy_edges" in gpu.lib.hymet_last_error()
    assert len(rounds) == 1 and rounds[0][1] <= 3 + 1
    # the error does not stick to the next correct call
    for run, arg in ((run_greedy, (d_block, n, any_common, S)), (run_edges, (d_csr, n, S))):
        rc, got, links, _ = run(gpu, *arg, rows=3)
        assert rc == 0 and links == len(pairs)
        np.testing.assert_array_equal(got, want)


def test_greedy_edges_report_an_index_outside_the_row(gpu):
    n = 4
    for bad in (-1, 2, 3, 1 << 30):                        # row 2 may name 0 and 1 only
        d_csr = (upload(gpu, [0, 0, 1, 2, 3], np.int64), upload(gpu, [0, bad, 0], np.int32),
                 upload(gpu, [5 << 16 | 10] * 3, np.int32))
        rc, _, _, rounds = run_edges(gpu, d_csr, n, S)
        assert rc == E_ARG and in_bound(rounds), bad
    d_csr = (upload(gpu, [0, 0, 1, 2, 3], np.int64), upload(gpu, [0, 1, 0], np.int32), upload(gpu, [5 << 16 | 10] * 3, np.int32))
    rc, got, links, _ = run_edges(gpu, d_csr, n, S)
    assert rc == 0 and links == 3
    np.testing.assert_array_equal(got, [0, 0, 2, 0])       # 1 is a member: 2 stands alone; 3 joins 0


def test_greedy_argument_checks(gpu, any_common):
    from hymet_amd._lib import ptr
    n, pairs, want = case("zero_over_zero")
    d_block, (d_off, d_idx, d_val) = crafted(gpu, n, pairs), csr(gpu, n, pairs)
    rep, links, r = fresh(gpu, n), gpu.zeros(1, gpu.torch.int64), ctypes.c_int32()

    def call(s=S, n_rows=n, q0=0, nn=n):
        return gpu.lib.hymet_mash_greedy(gpu.ctx, ptr(d_block), n_rows, nn, q0, ptr(any_common), s, ptr(rep), ptr(links),
                                         ctypes.byref(r))

    def call_edges(s=S, n_rows=n, q0=0):
        return gpu.lib.hymet_mash_greedy_edges(gpu.ctx, ptr(d_off), n_rows, q0, ptr(d_idx), ptr(d_val), s, ptr(rep), ptr(links),
                                               ctypes.byref(r))

    for kw in (dict(s=0), dict(s=16385), dict(n_rows=n + 1), dict(q0=1), dict(q0=-1), dict(n_rows=-1), dict(nn=-1),
               dict(nn=1 << 31)):
        assert call(**kw) == E_ARG, kw
    for kw in (dict(s=0), dict(s=16385), dict(q0=-1), dict(n_rows=-1), dict(q0=1 << 31)):
        assert call_edges(**kw) == E_ARG, kw
    gpu.sync()
    assert (rep.cpu().numpy() == -1).all() and int(links.cpu().item()) == 0      # nothing ran
    assert call() == 0 and r.value >= 1
    np.testing.assert_array_equal(rep.cpu().numpy(), want)


# ------------------------------------------------------------------ real pair values
PARITY_S, PARITY_N = 64, 300


@pytest.fixture(scope="module")
def parity(gpu):
    """The lists of the dist tests and their square of pair values, computed once."""
    lists = parity_lists(PARITY_S, PARITY_N, 1)[0]
    db = make_db(lists, PARITY_S)
    return lists, dense(gpu, db, db, PARITY_S)


def passing_pairs(square, order, table, s):
    """{(q, r): (common, denom)}, r < q, of the passing pairs with the sketches renumbered so
    that new index i is sketch order[i]."""
    v = square[np.ix_(order, order)]
    c, d = (v >> 16).astype(np.int64), (v & 0xFFFF).astype(np.int64)
    ok = np.tril(np.ones(v.shape, bool), k=-1) & (d <= s) & (c >= table[np.minimum(d, s)])
    return {(int(q), int(r)): (int(c[q, r]), int(d[q, r])) for q, r in np.argwhere(ok)}


@pytest.mark.parametrize("max_dist", [0.05, 0.3])
def test_cluster_greedy_on_real_pairs(gpu, parity, max_dist):
    from hymet_amd import derep as dr
    from hymet_amd import mashdist as md
    lists, square = parity
    n, s = PARITY_N, PARITY_S
    table = md.min_common_table(s, K, max_dist)
    seeded = np.random.default_rng(7).permutation(n) + 1_000     # distinct lengths: the order is theirs alone
    for rule, lengths in (("first", None), ("longest", seeded)):
        db = make_db(lists, s, lengths=lengths)
        order = dr.priority_order(db.lengths, n, rule)
        assert (rule == "first") == np.array_equal(order, np.arange(n))
        pairs = passing_pairs(square, order, table, s)
        walk = gr.greedy(n, pairs)
        want = np.empty(n, np.int64)
        want[order] = order[walk]                          # back to DB indices
        if rule == "first":                                # the numbers test_derep_greedy.py pins on the host
            assert int((walk == np.arange(n)).sum()) == {0.05: 57, 0.3: 24}[max_dist]
            assert len(np.unique(cc_labels(n, pairs))) == {0.05: 55, 0.3: 3}[max_dist]
        for bb in (4 * n, 20 * n, 1 << 30):
            res = dr.cluster_greedy(gpu, db, max_dist, rule=rule, block_bytes=bb)
            np.testing.assert_array_equal(res.rep, want, err_msg=f"{rule}, block_bytes={bb}")
            assert res.n_links == len(pairs)
            assert len(res.rounds) == -(-n // max(1, bb // (4 * n))) and all(r >= 1 for r in res.rounds)
        plan = []
        res = dr.cluster_greedy(gpu, db, max_dist, rule=rule, block_bytes=4 * n, sparse=True, plan=plan)
        assert {p[0] for p in plan} == {"sparse", "dense"}, plan
        np.testing.assert_array_equal(res.rep, want, err_msg=f"{rule}, sparse with a dense fallback")
        assert res.n_links == len(pairs) and len(res.rounds) == len(plan)
        res = dr.cluster_greedy(gpu, db, max_dist, rule=rule, sparse=True)
        np.testing.assert_array_equal(res.rep, want, err_msg=f"{rule}, sparse")
        assert res.n_links == len(pairs)


# ------------------------------------------------------------------ end to end
S_E2E = 1000
NAMES = ["A", "B", "C", "A2", "C2", "S"]


@pytest.fixture(scope="module")
def chain(gpu, tmp_path_factory):
    """A - B - C drift apart by 3.5 % steps, so that A and C are no longer within D = 0.05 of
    each other; A2 and C2 are 1 % mutants of A and C; S is unrelated.  Sketched on the GPU."""
    from hymet_amd import sketch as sk
    from hymet_amd.msh import write_msh
    rng = np.random.default_rng(78)
    A = rand_seq(rng, 20_000)
    B = mutate(rng, A, 0.035)
    C = mutate(rng, B, 0.035)
    A2 = mutate(rng, A, 0.01)
    C2 = mutate(rng, C, 0.01)
    S_ = rand_seq(rng, 20_000)
    d = tmp_path_factory.mktemp("greedy")
    (d / "all.fna").write_bytes(_fasta(list(zip(NAMES, [A, B, C, A2, C2, S_]))))
    db = sk.sketch_files(gpu, [str(d / "all.fna")], k=K, seed=42, s=S_E2E, individual=True)
    write_msh(db, str(d / "all.msh"))
    return d, db


def test_cluster_greedy_end_to_end(gpu, chain):
    from hymet_amd import derep as dr
    from hymet_amd import mashdist as md
    _, db = chain
    n = db.n_refs
    assert db.names == NAMES
    lists = [np.asarray(db.ref_hashes(i), np.uint64).tolist() for i in range(n)]
    t = md.min_common_table(S_E2E, K, 0.05)
    assert t[S_E2E] == 213
    shared = {(q, r): merge_loop(lists[r], lists[q], S_E2E) for q in range(n) for r in range(q)}
    assert all(d == S_E2E for _, d in shared.values())
    links = {k: v for k, v in shared.items() if v[0] >= t[v[1]]}
    A, B, C, A2, C2 = range(5)
    assert {k: v[0] for k, v in links.items()} == {(B, A): 309, (C, B): 317, (A2, A): 692, (A2, B): 250, (C2, B): 243,
                                                   (C2, C): 674}
    assert [shared[k][0] for k in ((C, A), (A2, C), (C2, A), (C2, A2))] == [123, 105, 97, 84]
    single = dr.cluster(gpu, db, 0.05)
    np.testing.assert_array_equal(single.labels, [0, 0, 0, 0, 0, 5])
    assert single.n_links == 6
    for sparse in (False, True):
        res = dr.cluster_greedy(gpu, db, 0.05, rule="first", sparse=sparse)
        np.testing.assert_array_equal(res.rep, [0, 0, 2, 0, 2, 5])
        assert res.n_links == 6
        gr.check_members_pass(res.rep, links)
        gr.check_representatives_apart(res.rep, links)
        # C2 first, then DB order: B's first preceding representative is C2 (243 shared), its
        # nearest is A (309)
        longest = dataclasses.replace(db, lengths=np.array([20_000, 20_000, 20_000, 20_000, 20_001, 20_000], np.int64))
        res = dr.cluster_greedy(gpu, longest, 0.05, rule="longest", sparse=sparse)
        np.testing.assert_array_equal(res.rep, [0, 0, 4, 0, 4, 5])
        assert res.n_links == 6


def _cli(args):
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-m", "hymet_amd.cli"] + args
    return subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)


def test_cli_derep_greedy_writes_the_representatives(chain):
    from hymet_amd.msh import load_db
    d, db = chain
    r = _cli(["derep", "--greedy", "-r", "first", "-o", str(d / "kept"), str(d / "all.msh")])
    assert r.returncode == 0, r.stdout + r.stderr
    want = ["A\tA\t0\t3", "B\tA\t0\t3", "C\tC\t1\t2", "A2\tA\t0\t3", "C2\tC\t1\t2", "S\tS\t2\t1"]
    assert r.stdout.splitlines() == want
    assert "derep: 6 sketches, 6 links, 3 clusters (greedy)" in r.stderr.splitlines()
    out = load_db(str(d / "kept.msh"))
    assert out.names == ["A", "C", "S"]
    for i, j in enumerate((0, 2, 5)):
        np.testing.assert_array_equal(out.ref_hashes(i), db.ref_hashes(j))
    assert (out.k, out.seed, out.sketch_size) == (db.k, db.seed, db.sketch_size)


def test_cli_derep_greedy_sparse_and_plain(gpu, chain, capsys):
    from hymet_amd import cli
    d, _ = chain
    path = str(d / "all.msh")

    def run(*args):
        assert cli.main(["derep", *args, path]) == 0
        cap = capsys.readouterr()
        return cap.out, cap.err

    greedy = run("--greedy", "-r", "first")
    assert run("--greedy", "--sparse", "-r", "first") == greedy
    assert greedy[1].splitlines()[-1] == "derep: 6 sketches, 6 links, 3 clusters (greedy)"
    # without the flag: single linkage, the summary line without a suffix
    out, err = run("-r", "first")
    assert out.splitlines() == [f"{name}\tA\t0\t5" for name in NAMES[:5]] + ["S\tS\t1\t1"]
    assert err.splitlines()[-1] == "derep: 6 sketches, 6 links, 2 clusters"
