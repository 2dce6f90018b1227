"""Sparse dist (hymet_mash_dist_sparse, hymet_mash_link_edges; mashdist.sparse_blocks,
derep.cluster(sparse=True), `--sparse`) against the dense path it must equal byte for byte:
hymet_mash_dist_select over hymet_mash_dist's block (pinned by test_mashdist_gpu.py), and its
counters against tests/_sparse_ref.py."""
import ctypes

import numpy as np
import pytest

from tests import _sparse_ref as ref
from tests._cc_ref import labels as cc_labels
from tests.test_derep_gpu import FAMILIES, planted  # noqa: F401  (planted: a fixture)
from tests.test_mashdist_gpu import cut_lists, dense, make_db, merge_loop, parity_lists

pytestmark = pytest.mark.gpu

E_ARG, E_CAPACITY = -2, -3
K = 21
FILL = 0x5A5A5A5A
DISTS = (0.0, 0.05, 0.3, 0.999)
AMPLE = 1 << 24


@pytest.fixture(scope="module")
def gpu():
    from hymet_amd._lib import Gpu
    return Gpu(0)


def tables(gpu, s, max_dist):
    """(host table, device table, cmin)"""
    from hymet_amd import mashdist as md
    t = md.min_common_table(s, K, max_dist)
    return t, gpu.torch.from_numpy(t.view(np.int16).copy()).to(gpu.dev), md.candidate_min_common(t)


def sparse_raw(gpu, R, Q, q0, q1, s, d_table, cmin, max_pairs=AMPLE, tri=False, cap=1 << 16, **over):
    """One raw hymet_mash_dist_sparse call over pre-filled outputs: rc, total, row offsets, the
    whole index and value buffers (cap + 8 entries), counters.  over: arguments to replace."""
    from hymet_amd._lib import SparseCounters, ptr
    torch = gpu.torch
    rows = max(q1 - q0, 0)
    row_off = torch.full((rows + 1,), -9, dtype=torch.int64, device=gpu.dev)
    idx = torch.full((cap + 8,), FILL, dtype=torch.int32, device=gpu.dev)
    val = torch.full((cap + 8,), FILL, dtype=torch.int32, device=gpu.dev)
    total, ctr = ctypes.c_int64(-5), SparseCounters(-1, -1, -1)
    a = dict(rh=ptr(R.hashes), rn=R.n_hashes, ro=ptr(R.offsets), n_ref=R.n, qh=ptr(Q.hashes), qn=Q.n_hashes,
             qo=ptr(Q.offsets), n_qry=Q.n, s=s)
    a.update(over)
    rc = gpu.lib.hymet_mash_dist_sparse(gpu.ctx, a["rh"], a["rn"], a["ro"], a["n_ref"], a["qh"], a["qn"], a["qo"], a["n_qry"],
                                        q0, q1, a["s"], int(tri), ptr(d_table), cmin, max_pairs, ptr(row_off), ptr(idx),
                                        ptr(val), cap, ctypes.byref(total), ctypes.byref(ctr))
    gpu.sync()
    return (rc, total.value, row_off.cpu().numpy(), idx.cpu().numpy(), val.cpu().numpy().view(np.uint32),
            (ctr.postings, ctr.emitted, ctr.candidates))


def dense_select(gpu, block, table, d_table, s, q0=0, tri=False):
    """hymet_mash_dist_select over the rows of a dense host block (row 0 is query q0): row_off,
    reference index, value; tri: its entries r < q only."""
    from hymet_amd import mashdist as md
    n_rows, n_ref = block.shape
    if n_rows == 0 or n_ref == 0:
        return np.zeros(n_rows + 1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.uint32)
    d_block = gpu.torch.from_numpy(np.ascontiguousarray(block).view(np.int32).reshape(-1).copy()).to(gpu.dev)
    row_off, ri, v = md.select_block(gpu, d_block, n_rows, n_ref, d_table, s)
    if tri:
        qi = np.repeat(np.arange(q0, q0 + n_rows), np.diff(row_off))
        below = ri < qi
        row_off = np.r_[0, np.cumsum(np.bincount(qi[below] - q0, minlength=n_rows))].astype(np.int64)
        ri, v = ri[below], v[below]
    return row_off, ri, v


def assert_same(got, want, msg):
    rc, total, row_off, idx, val, _ = got
    w_off, w_ri, w_v = want
    assert rc == 0, msg
    assert total == len(w_ri), msg
    np.testing.assert_array_equal(row_off, w_off, err_msg=msg)
    np.testing.assert_array_equal(idx[:total], w_ri, err_msg=msg)
    np.testing.assert_array_equal(val[:total], w_v, err_msg=msg)
    assert (idx[total:] == FILL).all() and (val[total:] == FILL).all(), msg


def check_counters(got, refs, qrys, s, q0, q1, cmin, sh, msg):
    want = (ref.postings(refs, qrys, s, q0, q1), ref.emitted(refs, qrys, s, q0, q1, sh),
            ref.candidates(refs, qrys, s, q0, q1, cmin, sh))
    assert got[5] == want, msg


# ------------------------------------------------------------------ parity with the dense path
@pytest.mark.parametrize("shape", [(1, 17, 5), (64, 17, 5), (65, 17, 5), (1000, 17, 5), (64, 65, 65)])
def test_parity_with_dense_select(gpu, shape):
    from hymet_amd import mashdist as md
    s, n_ref, n_qry = shape
    refs, qrys = parity_lists(s, n_ref, n_qry)
    assert {len(a) for a in refs} == {0, 1, s - 1, s, s + 5}
    assert ref.empty_pairs(refs, qrys, s, 0, n_qry), "the empty-pair rule is not exercised"
    ref_db, qry_db = make_db(refs, s), make_db(qrys, s)
    block = dense(gpu, ref_db, qry_db, s)
    R, Q = md.DeviceSketches(gpu, ref_db), md.DeviceSketches(gpu, qry_db)
    sh = ref.shared(refs, qrys, s, 0, n_qry)
    kept = set()
    for max_dist in DISTS:
        t, d_t, cmin = tables(gpu, s, max_dist)
        for q0, q1 in sorted({(0, n_qry), (1, n_qry), (n_qry - 1, n_qry), (3, 3)}):
            msg = f"s={s} {n_ref}x{n_qry} D={max_dist} rows [{q0}, {q1})"
            got = sparse_raw(gpu, R, Q, q0, q1, s, d_t, cmin)
            assert_same(got, dense_select(gpu, block[q0:q1], t, d_t, s), msg)
            if q1 > q0:
                check_counters(got, refs, qrys, s, q0, q1, cmin, sh, msg)
            kept.add(got[1])
    assert max(kept) > 0


@pytest.mark.parametrize("s", [1, 64, 65, 1000])
def test_tri_parity_with_dense_lower_triangle(gpu, s):
    from hymet_amd import mashdist as md
    lists = parity_lists(s, 300, 1)[0]
    sh_all = ref.shared(lists, None, s, 0, 300)
    for n in (1, 2, 3, 17, 70, 300):
        sub = lists[:n]
        db = make_db(sub, s)
        square = dense(gpu, db, db, s)
        D = md.DeviceSketches(gpu, db)
        sh = {k: v for k, v in sh_all.items() if k[0] < n}
        for max_dist in DISTS:
            t, d_t, cmin = tables(gpu, s, max_dist)
            for q0, q1 in sorted({(0, n), (min(1, n), n), (n - 1, n), (min(3, n), min(3, n))}):
                msg = f"s={s} n={n} D={max_dist} rows [{q0}, {q1})"
                got = sparse_raw(gpu, D, D, q0, q1, s, d_t, cmin, tri=True)
                assert_same(got, dense_select(gpu, square[q0:q1], t, d_t, s, q0, tri=True), msg)
                if q1 > q0:
                    check_counters(got, sub, None, s, q0, q1, cmin, sh, msg)
    assert len(ref.empty_pairs(lists, None, s, 0, 300)) > 0


@pytest.mark.parametrize("s", [64, 1000])
def test_union_rank_cut(gpu, s):
    """shared counts the whole truncated intersection, common only what lies in the s smallest
    of the union: the run length is never the answer."""
    from hymet_amd import mashdist as md
    refs, qrys = cut_lists(s)
    more = 0
    for n in range(len(refs)):
        A, B = refs[n].tolist()[:s], qrys[n].tolist()[:s]
        more += len(set(A) & set(B)) > merge_loop(refs[n].tolist(), qrys[n].tolist(), s)[0]
    assert more > 0, "no pair with shared > common"
    ref_db, qry_db = make_db(refs, s), make_db(qrys, s)
    block = dense(gpu, ref_db, qry_db, s)
    R, Q = md.DeviceSketches(gpu, ref_db), md.DeviceSketches(gpu, qry_db)
    t, d_t, cmin = tables(gpu, s, 0.999)
    got = sparse_raw(gpu, R, Q, 0, len(qrys), s, d_t, cmin)
    want = dense_select(gpu, block, t, d_t, s)
    assert_same(got, want, f"s={s}")
    # the values are the dense block's, not the run lengths
    qi = np.repeat(np.arange(len(qrys)), np.diff(want[0]))
    np.testing.assert_array_equal(got[4][:got[1]], block[qi, want[1]])
    check_counters(got, refs, qrys, s, 0, len(qrys), cmin, None, f"s={s}")


def test_unsigned_order_and_no_sentinel(gpu):
    from hymet_amd import mashdist as md
    top = 2 ** 64 - 1
    refs = [[5, 2 ** 63 - 1, 2 ** 63, 2 ** 63 + 7, top - 1, top], [1, 2 ** 63, top - 1], [top], [],
            [3, 2 ** 62, 2 ** 63 - 1, 2 ** 63 + 7, top]]
    qrys = [[5, 2 ** 63, top], [2 ** 63 - 1, 2 ** 63 + 7, top - 1], [top], [top - 1], [],
            [0, 5, 2 ** 63 - 1, 2 ** 63, 2 ** 63 + 1, top - 1]]
    s = 64
    ref_db, qry_db = make_db(refs, s), make_db(qrys, s)
    block = dense(gpu, ref_db, qry_db, s)
    assert block[0, 0] == 3 << 16 | 6 and block[2, 2] == 1 << 16 | 1 and block[4, 3] == 0
    R, Q = md.DeviceSketches(gpu, ref_db), md.DeviceSketches(gpu, qry_db)
    for max_dist in DISTS:
        t, d_t, cmin = tables(gpu, s, max_dist)
        got = sparse_raw(gpu, R, Q, 0, len(qrys), s, d_t, cmin)
        want = dense_select(gpu, block, t, d_t, s)
        assert_same(got, want, f"D={max_dist}")
        check_counters(got, refs, qrys, s, 0, len(qrys), cmin, None, f"D={max_dist}")
        entries = set(zip(np.repeat(np.arange(len(qrys)), np.diff(want[0])).tolist(), want[1].tolist()))
        assert (2, 2) in entries and (4, 3) in entries           # 2^64 - 1 shared; two empty lists


# ------------------------------------------------------------------ budget and capacity
def skew_lists():
    """300 sketches of 64 hashes: one hash (the smallest, so it lies in every union's first 64)
    held by all, the others private."""
    rng = np.random.default_rng(300)
    pool = np.unique(rng.integers(1000, 2 ** 64, size=300 * 63 + 64, dtype=np.uint64))[:300 * 63]
    return [np.sort(np.r_[pool[i * 63:(i + 1) * 63], np.uint64(0)]) for i in range(300)]


def test_skew_and_emission_budget(gpu):
    from hymet_amd import mashdist as md
    lists, s, n = skew_lists(), 64, 300
    assert all(len(a) == 64 and len(np.unique(a)) == 64 for a in lists)
    db = make_db(lists, s)
    D = md.DeviceSketches(gpu, db)
    t, d_t, cmin = tables(gpu, s, 0.999)
    want_emitted = ref.emitted(lists, None, s, 0, n)
    assert want_emitted >= 44_850
    rc, total, row_off, idx, val, ctr = sparse_raw(gpu, D, D, 0, n, s, d_t, cmin, max_pairs=1000, tri=True)
    assert rc == E_CAPACITY and total == -1
    assert ctr[1] == want_emitted and ctr[0] == 300 * 64
    assert (row_off == -9).all() and (idx == FILL).all() and (val == FILL).all()
    assert b"hymet_mash_dist_sparse" in gpu.lib.hymet_last_error()
    # one key short of the need is refused as well; the need itself is enough
    assert sparse_raw(gpu, D, D, 0, n, s, d_t, cmin, max_pairs=want_emitted - 1, tri=True)[0] == E_CAPACITY
    square = dense(gpu, db, db, s)
    want = dense_select(gpu, square, t, d_t, s, 0, tri=True)
    assert len(want[1]) == n * (n - 1) // 2                      # common 1 of denom 64 passes at 0.999
    got = sparse_raw(gpu, D, D, 0, n, s, d_t, cmin, max_pairs=want_emitted, tri=True)
    assert_same(got, want, "skew, exact budget")
    check_counters(got, lists, None, s, 0, n, cmin, None, "skew")


def test_output_capacity(gpu):
    from hymet_amd import mashdist as md
    s = 64
    refs, qrys = parity_lists(64, 65, 65)
    ref_db, qry_db = make_db(refs, s), make_db(qrys, s)
    R, Q = md.DeviceSketches(gpu, ref_db), md.DeviceSketches(gpu, qry_db)
    t, d_t, cmin = tables(gpu, s, 0.3)
    want = dense_select(gpu, dense(gpu, ref_db, qry_db, s), t, d_t, s)
    total = len(want[1])
    assert total > 1
    assert_same(sparse_raw(gpu, R, Q, 0, 65, s, d_t, cmin, cap=total), want, "cap == total")
    rc, got_total, row_off, idx, val, _ = sparse_raw(gpu, R, Q, 0, 65, s, d_t, cmin, cap=total - 1)
    assert rc == E_CAPACITY and got_total == total
    np.testing.assert_array_equal(row_off, want[0])
    assert (idx == FILL).all() and (val == FILL).all()
    # the host wrapper retries with the reported total
    d_off, d_idx, d_val, n, _ = md.sparse_block(gpu, R, Q, 0, 65, s, d_t, cmin, AMPLE, cap=1)
    assert n == total
    np.testing.assert_array_equal(d_off.cpu().numpy(), want[0])
    np.testing.assert_array_equal(d_idx[:n].cpu().numpy(), want[1])
    np.testing.assert_array_equal(d_val[:n].cpu().numpy().view(np.uint32), want[2])


def test_argument_checks(gpu):
    """hymet_mash_dist_tri's rejections, before any launch."""
    from hymet_amd import mashdist as md
    from hymet_amd._lib import ptr
    lists = parity_lists(64, 17, 1)[0]
    D = md.DeviceSketches(gpu, make_db(lists, 64))
    _, d_t, cmin = tables(gpu, 64, 0.05)

    def call(s=64, q0=0, q1=D.n, tri=True, cmin=cmin, max_pairs=AMPLE, **over):
        return sparse_raw(gpu, D, D, q0, q1, s, d_t, cmin, max_pairs=max_pairs, tri=tri, **over)[0]

    assert call() == 0
    assert call(tri=False) == 0
    for kw in (dict(s=0), dict(s=16385), dict(q1=D.n + 1), dict(q0=-1), dict(q0=3, q1=2),
               dict(rn=D.n_hashes - 1, qn=D.n_hashes - 1), dict(cmin=0), dict(max_pairs=-1)):
        assert call(**kw) == E_ARG, kw
        assert b"hymet_mash_dist" in gpu.lib.hymet_last_error()
    dec = D.offsets.clone()
    dec[3] = dec[4] + 1
    assert call(ro=ptr(dec), qo=ptr(dec)) == E_ARG
    other = D.offsets.clone()
    assert call(qo=ptr(other)) == E_ARG                           # tri mode: one DB as both arguments
    assert call(qo=ptr(other), tri=False) == 0


# ------------------------------------------------------------------ host
def _collect(blocks):
    parts = list(blocks)
    return tuple(np.concatenate([p[i] for p in parts]) for i in range(4))


def test_sparse_blocks_equal_dist_blocks(gpu):
    from hymet_amd import mashdist as md
    refs, qrys = parity_lists(64, 65, 65)
    ref_db, qry_db = make_db(refs, 64), make_db(qrys, 64)
    sh = ref.shared(refs, qrys, 64, 0, 65)
    for max_dist in (0.05, 0.3):
        want = _collect(md.dist_blocks(gpu, ref_db, qry_db, max_dist))
        assert len(want[0]) > 0
        got = _collect(md.dist_blocks(gpu, ref_db, qry_db, max_dist, sparse=True))
        for a, b in zip(got, want):
            np.testing.assert_array_equal(a, b)
            assert a.dtype == b.dtype
        # ample: one sparse call.  One dense row and 16 keys: the range splits down to single rows,
        # the short queries stay sparse and the long ones fall back.  No key at all: dense wherever
        # there is anything to visit.
        for bb, paths in ((1 << 30, {"sparse"}), (4 * 65, {"sparse", "dense"}), (15, None)):
            plan = []
            got = _collect(md.sparse_blocks(gpu, ref_db, qry_db, max_dist, block_bytes=bb, plan=plan))
            for a, b in zip(got, want):
                np.testing.assert_array_equal(a, b, err_msg=f"block_bytes={bb}")
            assert [p[1] for p in plan] == sorted(p[1] for p in plan) and plan[0][1] == 0 and plan[-1][2] == 65
            assert all(a[2] == b[1] for a, b in zip(plan, plan[1:]))
            if paths is None:
                assert any(p[0] == "dense" for p in plan) and all(p[0] == "dense" or p[3][1] == 0 for p in plan)
            else:
                assert {p[0] for p in plan} == paths, (bb, plan)
            for path, q0, q1, ctr in plan:
                if path == "sparse":
                    assert ctr[1] == ref.emitted(refs, qrys, 64, q0, q1, sh) and ctr[1] <= bb // 16
                else:
                    assert q1 - q0 <= max(1, bb // (4 * 65))
    with pytest.raises(ValueError):
        next(md.sparse_blocks(gpu, ref_db, qry_db, 1.0))


# ------------------------------------------------------------------ clustering
def edge_labels(gpu, n, d_off, d_idx, step):
    """hymet_mash_link_edges over the n-row CSR in calls of `step` rows, then the labels."""
    from hymet_amd._lib import ptr
    torch = gpu.torch
    parent = torch.arange(n, dtype=torch.int32, device=gpu.dev)
    label = torch.full((n,), -7, dtype=torch.int32, device=gpu.dev)
    links = gpu.zeros(1, torch.int64)
    for q0 in range(0, n, step):
        q1 = min(n, q0 + step)
        gpu.call("hymet_mash_link_edges", ptr(d_off[q0:]), q1 - q0, q0, ptr(d_idx), ptr(parent), ptr(links))
    gpu.call("hymet_mash_labels", ptr(parent), n, ptr(label))
    return label.cpu().numpy(), int(links.cpu().item())


def test_cluster_sparse_on_planted_families(gpu, planted):  # noqa: F811
    from hymet_amd import derep as dr
    _, _, db = planted
    n = db.n_refs
    lists = [np.asarray(db.ref_hashes(i), np.uint64) for i in range(n)]
    want = dr.cluster(gpu, db, 0.05)
    np.testing.assert_array_equal(want.labels, FAMILIES)
    # as test_sparse_blocks_equal_dist_blocks: ample; one dense row and 3 keys; no key at all
    for bb, paths in ((1 << 30, {"sparse"}), (4 * n, {"sparse", "dense"}), (15, None)):
        plan = []
        res = dr.cluster(gpu, db, 0.05, block_bytes=bb, sparse=True, plan=plan)
        np.testing.assert_array_equal(res.labels, want.labels, err_msg=f"block_bytes={bb}")
        assert res.n_links == want.n_links == 10
        if paths is None:
            assert any(p[0] == "dense" for p in plan) and all(p[0] == "dense" or p[3][1] == 0 for p in plan)
        else:
            assert {p[0] for p in plan} == paths, (bb, plan)
    t, d_t, cmin = tables(gpu, 200, 0.05)
    edges = []
    for q in range(n):
        for r in range(q):
            c, d = merge_loop(lists[r].tolist(), lists[q].tolist(), 200)
            if c >= t[d]:
                edges.append((q, r))
    np.testing.assert_array_equal(res.labels, cc_labels(n, edges))
    alone = dr.cluster(gpu, db, 0.0, sparse=True)
    np.testing.assert_array_equal(alone.labels, np.arange(n))
    assert alone.n_links == 0


def test_cluster_sparse_clique_and_edge_blocking(gpu):
    from hymet_amd import derep as dr
    from hymet_amd import mashdist as md
    n, s = 1024, 64
    rng = np.random.default_rng(1024)
    base = np.unique(rng.integers(0, 2 ** 64, size=80, dtype=np.uint64))[:64]
    private = np.unique(rng.integers(0, 2 ** 64, size=n + 8, dtype=np.uint64))
    private = private[~np.isin(private, base)][:n]
    # every sketch: 63 of the 64 base hashes and one of its own -> any two share 62 or 63
    lists = [np.sort(np.r_[np.delete(base, i % 64), private[i]]) for i in range(n)]
    db = make_db(lists, s)
    want = dr.cluster(gpu, db, 0.05)
    assert (want.labels == 0).all() and want.n_links == n * (n - 1) // 2
    np.testing.assert_array_equal(want.labels, cc_labels(n, [(q, q - 1) for q in range(1, n)]))
    plan = []
    res = dr.cluster(gpu, db, 0.05, sparse=True, plan=plan)
    np.testing.assert_array_equal(res.labels, want.labels)
    assert res.n_links == want.n_links and {p[0] for p in plan} == {"sparse"}
    # the CSR of one call, united in one call and in calls of 1, 63 and 65 rows
    D = md.DeviceSketches(gpu, db)
    _, d_t, cmin = tables(gpu, s, 0.05)
    d_off, d_idx, _, total, _ = md.sparse_block(gpu, D, D, 0, n, s, d_t, cmin, 1 << 27, tri=True, cap=n * n // 2)
    assert total == want.n_links
    for step in (n, 1, 63, 65):
        got, links = edge_labels(gpu, n, d_off, d_idx, step)
        np.testing.assert_array_equal(got, want.labels, err_msg=f"calls of {step} rows")
        assert links == total


def test_link_edges_on_a_sparse_graph(gpu):
    """Components that are not cliques, from a hand-made CSR."""
    torch = gpu.torch
    n = 2000
    rng = np.random.default_rng(2000)
    e = rng.integers(0, n, size=(1500, 2))
    e = e[e[:, 0] != e[:, 1]]
    e = np.unique(np.c_[e.max(axis=1), e.min(axis=1)], axis=0)   # (q, r), r < q, sorted by q then r
    row_off = np.r_[0, np.cumsum(np.bincount(e[:, 0], minlength=n))].astype(np.int64)
    d_off = torch.from_numpy(row_off).to(gpu.dev)
    d_idx = torch.from_numpy(e[:, 1].astype(np.int32)).to(gpu.dev)
    want = cc_labels(n, e)
    assert len(np.unique(want)) > 1
    for step in (n, 1, 63, 65):
        got, links = edge_labels(gpu, n, d_off, d_idx, step)
        np.testing.assert_array_equal(got, want, err_msg=f"calls of {step} rows")
        assert links == len(e)


def test_cli_sparse_prints_the_same_bytes(gpu, planted, capsys):  # noqa: F811
    from hymet_amd import cli
    d, _, _ = planted
    path = str(d / "all.msh")

    def run(*args):
        assert cli.main(list(args)) == 0
        cap = capsys.readouterr()
        return cap.out, cap.err

    out, err = run("derep", path)
    out2, err2 = run("derep", "--sparse", path)
    assert out2 == out and err2 == err and len(out.splitlines()) == 12
    assert "derep: 12 sketches, 10 links, 6 clusters" in err2.splitlines()
    out, _ = run("dist", "-d", "0.05", path, path)
    out2, _ = run("dist", "--sparse", "-d", "0.05", path, path)
    assert out2 == out and len(out.splitlines()) == 12 + 2 * 10
