"""Nearest references (hymet_mash_dist_topk, hymet_mash_topk_edges; mashdist.dist_blocks(top=K),
`dist --top K`) against tests/_topk_ref.py, the order restated on exact fractions.  Blocks are
uploaded as uint32 arrays, outputs are pre-filled so that "not written" is checked."""
import numpy as np
import pytest

from tests import _topk_ref as ref
from tests.test_mashdist_gpu import dense, make_db, parity_lists

pytestmark = pytest.mark.gpu

E_ARG = -2
K21 = 21
FILL = 0x5A5A5A5A
CNT_FILL = -9
PAD = 8


@pytest.fixture(scope="module")
def gpu():
    from hymet_amd._lib import Gpu
    return Gpu(0)


@pytest.fixture(scope="module")
def kmax(gpu):
    return int(gpu.lib.hymet_mash_topk_max())


def pack(c, d):
    return (np.asarray(c, np.uint32) << np.uint32(16) | np.asarray(d, np.uint32)).astype(np.uint32)


def upload(gpu, a, dtype=np.int32):
    return gpu.torch.from_numpy(np.ascontiguousarray(a).view(dtype).reshape(-1).copy()).to(gpu.dev)


def outputs(gpu, n_rows, K):
    torch = gpu.torch
    n = max(n_rows, 0) * max(K, 1) + PAD
    return (torch.full((n,), FILL, dtype=torch.int32, device=gpu.dev), torch.full((n,), FILL, dtype=torch.int32, device=gpu.dev),
            torch.full((max(n_rows, 0) + PAD,), CNT_FILL, dtype=torch.int32, device=gpu.dev))


def host(gpu, rc, out):
    gpu.sync()
    idx, val, cnt = out
    return rc, idx.cpu().numpy(), val.cpu().numpy().view(np.uint32), cnt.cpu().numpy()


def topk_raw(gpu, block, K, s, d_table=None, **over):
    """One raw hymet_mash_dist_topk call over the host block (rows x n_ref uint32) and pre-filled
    outputs: rc, idx, val (rows * K + PAD entries), cnt (rows + PAD).  over: arguments to replace."""
    from hymet_amd._lib import ptr
    n_rows, n_ref = block.shape
    d_block = upload(gpu, block) if block.size else gpu.zeros(1, gpu.torch.int32)
    a = dict(n_rows=n_rows, n_ref=n_ref, s=s, K=K)
    a.update(over)
    out = outputs(gpu, n_rows, K)
    rc = gpu.lib.hymet_mash_dist_topk(gpu.ctx, ptr(d_block), a["n_rows"], a["n_ref"], ptr(d_table) if d_table is not None else None,
                                      a["s"], a["K"], ptr(out[0]), ptr(out[1]), ptr(out[2]))
    return host(gpu, rc, out)


def edges_raw(gpu, row_off, ri, v, K, s, **over):
    from hymet_amd._lib import ptr
    n_rows = len(row_off) - 1
    d_off = upload(gpu, np.asarray(row_off, np.int64), np.int64)
    d_ri = upload(gpu, np.asarray(ri, np.int32)) if len(ri) else gpu.zeros(1, gpu.torch.int32)
    d_v = upload(gpu, np.asarray(v, np.uint32)) if len(v) else gpu.zeros(1, gpu.torch.int32)
    a = dict(n_rows=n_rows, s=s, K=K)
    a.update(over)
    out = outputs(gpu, n_rows, K)
    rc = gpu.lib.hymet_mash_topk_edges(gpu.ctx, ptr(d_off), a["n_rows"], ptr(d_ri), ptr(d_v), a["s"], a["K"], ptr(out[0]),
                                       ptr(out[1]), ptr(out[2]))
    return host(gpu, rc, out)


def assert_rows(got, want_idx, want_val, K, msg):
    """want_idx / want_val: per row the reference indices and packed values, nearest first."""
    rc, idx, val, cnt = got
    n_rows = len(want_idx)
    assert rc == 0, msg
    exp_idx = np.full(n_rows * K + PAD, FILL, np.int32)
    exp_val = np.full(n_rows * K + PAD, FILL, np.uint32)
    for r in range(n_rows):
        n = len(want_idx[r])
        assert n <= K
        exp_idx[r * K:r * K + n] = want_idx[r]
        exp_val[r * K:r * K + n] = want_val[r]
    np.testing.assert_array_equal(cnt[:n_rows], [len(w) for w in want_idx], err_msg=msg)
    assert (cnt[n_rows:] == CNT_FILL).all(), msg
    np.testing.assert_array_equal(idx, exp_idx, err_msg=msg)
    np.testing.assert_array_equal(val, exp_val, err_msg=msg)


def check_dense(gpu, block, K, s, msg, table=None, d_table=None, orders=None):
    """orders: the restatement's whole order per row, when the caller shares it among several K"""
    if orders is None:
        orders = ref.topk_dense(block >> 16, block & 0xFFFF, block.shape[1], s, table)
    want = [o[:K] for o in orders]
    got = topk_raw(gpu, block, K, s, d_table)
    assert_rows(got, want, [block[r, w] for r, w in enumerate(want)], K, msg)
    return got


def random_block(rng, n_rows, n_ref, s):
    """Random (common, denom <= s); a third of the denominators from a handful of values and a few
    0 / 0, common == denom and common == 0 entries, so that equal fractions and the ends occur."""
    d = rng.integers(0, s + 1, size=(n_rows, n_ref))
    few = rng.choice([0, 1, 2, 4, s // 2, s], size=(n_rows, n_ref))
    d = np.where(rng.random((n_rows, n_ref)) < 0.33, few, d)
    c = (rng.random((n_rows, n_ref)) * (d + 1)).astype(np.int64)
    u = rng.random((n_rows, n_ref))
    c = np.where(u < 0.05, d, np.where(u < 0.1, 0, c))
    return pack(c, d)


# ------------------------------------------------------------------ shapes
@pytest.mark.parametrize("n_ref", [1, 63, 64, 65, 255, 256, 257, 4097])
def test_shapes_against_the_restatement(gpu, kmax, n_ref):
    rng = np.random.default_rng(7000 + n_ref)
    for s in (1000, 16384):
        for n_rows in (1, 5):
            block = random_block(rng, n_rows, n_ref, s)
            orders = ref.topk_dense(block >> 16, block & 0xFFFF, n_ref, s)
            for K in sorted({1, 2, 64, 65, n_ref, n_ref + 1, kmax}):
                if K <= kmax:
                    check_dense(gpu, block, K, s, f"s={s} {n_rows}x{n_ref} K={K}", orders=orders)


# ------------------------------------------------------------------ adversarial rows
N_ADV, K_ADV = 5000, 100


def adversarial_block():
    i = np.arange(N_ADV)
    rows = [
        pack(np.full(N_ADV, 500), np.full(N_ADV, 1000)),                 # all equal
        pack(i + 1, np.full(N_ADV, 16384)),                              # strictly improving with the index
        pack(N_ADV - i, np.full(N_ADV, 16384)),                          # strictly worsening
        pack(np.where(i >= N_ADV - K_ADV, 1 + i % 7, 0), np.full(N_ADV, 1000)),   # only the last K non-zero
        pack(i % 8192 + 1, 2 * (i % 8192 + 1)),                          # one fraction, many (c, d)
        pack(np.where(i % 3 == 1, 1 + i % 100, 0), np.where(i % 3 == 0, 0, 1 + i % 100)),   # 0/0, c == d, c == 0
    ]
    return np.stack(rows)


def test_adversarial_rows(gpu):
    block = adversarial_block()
    got = check_dense(gpu, block, K_ADV, 16384, "adversarial")
    idx = got[1].reshape(-1)[:6 * K_ADV].reshape(6, K_ADV)
    np.testing.assert_array_equal(idx[0], np.arange(K_ADV))                            # ties: the first K indices
    np.testing.assert_array_equal(idx[1], np.arange(N_ADV - 1, N_ADV - 1 - K_ADV, -1))
    np.testing.assert_array_equal(idx[2], np.arange(K_ADV))
    assert set(idx[3].tolist()) == set(range(N_ADV - K_ADV, N_ADV))
    np.testing.assert_array_equal(idx[4], np.arange(K_ADV))
    # one row at a time too: the chunks per row depend on the row count
    for r in (0, 1):
        check_dense(gpu, block[r:r + 1], K_ADV, 16384, f"adversarial row {r} alone")


def test_entries_outside_the_contract_are_skipped(gpu):
    rng = np.random.default_rng(99)
    s = 1000
    block = random_block(rng, 3, N_ADV, s)
    c, d = (block >> 16).astype(np.int64), (block & 0xFFFF).astype(np.int64)
    u = rng.random(block.shape)
    d = np.where(u < 0.2, rng.integers(s + 1, 65536, size=block.shape), d)             # denom > s
    c = np.where((u >= 0.2) & (u < 0.4), d + 1 + rng.integers(0, 50, size=block.shape), c)   # common > denom
    bad = pack(c, d)
    bad[2] = pack(np.full(N_ADV, 7), np.full(N_ADV, 5))                                # nothing competes
    assert (~np.array([[ref.competes(x >> 16, x & 0xFFFF, s) for x in row] for row in bad])).sum() > N_ADV
    got = check_dense(gpu, bad, K_ADV, s, "outside the contract")
    assert got[3][2] == 0


# ------------------------------------------------------------------ chunkings
@pytest.mark.parametrize("case", ["4097", "adversarial"])
def test_chunkings_agree(gpu, kmax, case):
    if case == "4097":
        block, s = random_block(np.random.default_rng(4097), 5, 4097, 1000), 1000
    else:
        block, s = adversarial_block(), 16384
    orders = ref.topk_dense(block >> 16, block & 0xFFFF, block.shape[1], s)
    try:
        for K in (1, K_ADV, kmax):
            runs = []
            for chunk in (64, 256, 0):
                assert gpu.lib.hymet_mash_topk_tune(chunk) == 0
                runs.append(check_dense(gpu, block, K, s, f"{case} K={K} chunk={chunk}", orders=orders))
            for other in runs[1:]:
                for a, b in zip(runs[0][1:], other[1:]):
                    assert a.tobytes() == b.tobytes()
    finally:
        gpu.lib.hymet_mash_topk_tune(0)


# ------------------------------------------------------------------ filter
def filter_block():
    """6 rows x 700 at s = 1,000: row 0 all common = 0 (nothing passes below D = 1), row 1 one
    identical pair, row 2 300 close entries, row 3 all close, rows 4-5 random."""
    rng = np.random.default_rng(700)
    s, n = 1000, 700
    block = random_block(rng, 6, n, s)
    close_d = rng.integers(900, s + 1, size=(2, n))
    close_c = (close_d * (0.4 + 0.6 * rng.random((2, n)))).astype(np.int64)
    block[0] = pack(np.zeros(n), rng.integers(1, s + 1, size=n))
    block[1] = block[0]
    block[1, 333] = pack(1000, 1000)
    block[2] = np.where(np.arange(n) % 7 < 3, pack(close_c[0], close_d[0]), block[0])
    block[3] = pack(close_c[1], close_d[1])
    return block, s


def tables(gpu, s, max_dist):
    from hymet_amd import mashdist as md
    t = md.min_common_table(s, K21, max_dist)
    return t, upload(gpu, t, np.int16)


@pytest.mark.parametrize("max_dist", [0.0, 0.05, 0.999])
def test_filter_equals_select_then_restatement(gpu, max_dist):
    from hymet_amd import mashdist as md
    block, s = filter_block()
    n_rows, n_ref = block.shape
    t, d_t = tables(gpu, s, max_dist)
    row_off, ri, v = md.select_block(gpu, upload(gpu, block), n_rows, n_ref, d_t, s)
    assert row_off[1] == 0, "row 0 must keep nothing"
    assert row_off[2] - row_off[1] >= 1
    for K in (1, 10, 400):
        want = ref.topk_csr(row_off, ri, v >> 16, v & 0xFFFF, K, s)
        got = check_dense(gpu, block, K, s, f"D={max_dist} K={K}", table=t, d_table=d_t)
        rc, idx, val, cnt = got
        for r in range(n_rows):
            np.testing.assert_array_equal(idx[r * K:r * K + cnt[r]], [w[0] for w in want[r]])
            np.testing.assert_array_equal(val[r * K:r * K + cnt[r]], [v[w[1]] for w in want[r]])
        assert cnt[0] == 0 and (idx[:K] == FILL).all() and (val[:K] == FILL).all()


# ------------------------------------------------------------------ CSR
def test_csr_equals_restatement_and_dense(gpu):
    from hymet_amd import mashdist as md
    block, s = filter_block()
    n_rows, n_ref = block.shape
    t, d_t = tables(gpu, s, 0.05)
    row_off, ri, v = md.select_block(gpu, upload(gpu, block), n_rows, n_ref, d_t, s)
    lens = np.diff(row_off)
    assert lens[0] == 0 and lens[1] == 1 and lens[2] > 256 and lens[3] == n_ref
    try:
        for chunk in (64, 0):
            assert gpu.lib.hymet_mash_topk_tune(chunk) == 0
            for K in (1, 10, 300, 700):
                msg = f"chunk={chunk} K={K}"
                want = ref.topk_csr(row_off, ri, v >> 16, v & 0xFFFF, K, s)
                got = edges_raw(gpu, row_off, ri, v, K, s)
                assert_rows(got, [[w[0] for w in row] for row in want], [[v[w[1]] for w in row] for row in want], K, msg)
                same = topk_raw(gpu, block, K, s, d_t)
                for a, b in zip(got[1:], same[1:]):
                    np.testing.assert_array_equal(a, b, err_msg=msg)
    finally:
        gpu.lib.hymet_mash_topk_tune(0)
    # a CSR of empty rows only
    got = edges_raw(gpu, np.zeros(4, np.int64), np.zeros(0, np.int32), np.zeros(0, np.uint32), 5, s)
    assert_rows(got, [[], [], []], [[], [], []], 5, "empty CSR")


# ------------------------------------------------------------------ arguments
def untouched(got):
    _, idx, val, cnt = got
    return (idx == FILL).all() and (val == FILL).all() and (cnt == CNT_FILL).all()


def test_argument_checks(gpu, kmax):
    block = random_block(np.random.default_rng(5), 3, 70, 1000)
    assert topk_raw(gpu, block, 4, 1000)[0] == 0
    for kw in (dict(K=0), dict(K=-1), dict(K=kmax + 1), dict(s=0), dict(s=16385), dict(n_ref=2 ** 31), dict(n_ref=-1),
               dict(n_rows=-1)):
        a = {**dict(K=4, s=1000), **kw}
        got = topk_raw(gpu, block, a.pop("K"), a.pop("s"), **a)
        assert got[0] == E_ARG, kw
        assert untouched(got), kw
        assert b"hymet_mash_dist_topk" in gpu.lib.hymet_last_error()
    row_off, ri, v = np.array([0, 2, 3], np.int64), np.array([1, 5, 2], np.int32), pack([1, 2, 3], [4, 4, 4])
    assert edges_raw(gpu, row_off, ri, v, 4, 1000)[0] == 0
    for kw in (dict(K=0), dict(K=kmax + 1), dict(s=0), dict(s=16385), dict(n_rows=-1)):
        a = {**dict(K=4, s=1000), **kw}
        got = edges_raw(gpu, row_off, ri, v, a.pop("K"), a.pop("s"), **a)
        assert got[0] == E_ARG, kw
        assert untouched(got), kw
        assert b"hymet_mash_topk_edges" in gpu.lib.hymet_last_error()
    assert gpu.lib.hymet_mash_topk_tune(-2) == E_ARG
    # zero rows: nothing written; zero references: the counts are 0
    got = topk_raw(gpu, block, 4, 1000, n_rows=0)
    assert got[0] == 0 and untouched(got)
    got = edges_raw(gpu, row_off, ri, v, 4, 1000, n_rows=0)
    assert got[0] == 0 and untouched(got)
    got = topk_raw(gpu, block, 4, 1000, n_ref=0)
    assert got[0] == 0 and (got[3][:3] == 0).all() and (got[3][3:] == CNT_FILL).all()
    assert (got[1] == FILL).all() and (got[2] == FILL).all()


# ------------------------------------------------------------------ end to end
def _collect(blocks):
    parts = list(blocks)
    return tuple(np.concatenate([p[i] for p in parts]) for i in range(4))


@pytest.fixture(scope="module")
def e2e(gpu):
    refs, qrys = parity_lists(64, 65, 65)
    ref_db, qry_db = make_db(refs, 64), make_db(qrys, 64)
    return ref_db, qry_db, dense(gpu, ref_db, qry_db, 64)


def expected_rows(block, s, top, max_dist):
    from hymet_amd import mashdist as md
    table = md.min_common_table(s, K21, max_dist) if max_dist < 1.0 else None
    want = ref.topk_dense(block >> 16, block & 0xFFFF, top, s, table)
    qi = np.repeat(np.arange(len(want), dtype=np.int32), [len(w) for w in want])
    ri = np.array([r for w in want for r in w], np.int32)
    v = block[qi, ri]
    return qi, ri, (v >> 16).astype(np.int32), (v & 0xFFFF).astype(np.int32)


def test_dist_blocks_top(gpu, e2e):
    from hymet_amd import mashdist as md
    ref_db, qry_db, block = e2e
    for top in (3, 70):
        for max_dist, sparse in ((1.0, False), (0.05, False), (0.05, True)):
            want = expected_rows(block, 64, top, max_dist)
            assert len(want[0]) > 0
            # one block; several row blocks (and, sparse, ranges that fall back to dense: one dense
            # row and 16 pair keys, as test_mashdist_sparse_gpu.py)
            for bb in (1 << 30, 4 * 65):
                got = _collect(md.dist_blocks(gpu, ref_db, qry_db, max_dist, block_bytes=bb, sparse=sparse, top=top))
                for a, b in zip(got, want):
                    np.testing.assert_array_equal(a, b, err_msg=f"top={top} D={max_dist} sparse={sparse} block_bytes={bb}")
                    assert a.dtype == b.dtype
            d = md.distance(got[2], got[3], K21)
            same_q = got[0][1:] == got[0][:-1]
            assert (d[1:][same_q] >= d[:-1][same_q]).all()              # a query's distances never decrease
    plan = []
    list(md.sparse_blocks(gpu, ref_db, qry_db, 0.05, block_bytes=4 * 65, plan=plan))
    assert {p[0] for p in plan} == {"sparse", "dense"}                  # the fall-back was exercised above
    for bad in (-1, md.topk_max() + 1):
        with pytest.raises(ValueError):
            next(md.dist_blocks(gpu, ref_db, qry_db, top=bad))


def test_cli_top(gpu, e2e, tmp_path, capsys):
    from hymet_amd import cli
    from hymet_amd import mashdist as md
    from hymet_amd.msh import write_msh
    ref_db, qry_db, block = e2e
    rp, qp = str(tmp_path / "ref.msh"), str(tmp_path / "qry.msh")
    write_msh(ref_db, rp)
    write_msh(qry_db, qp)
    for extra, max_dist in (((), 1.0), (("-d", "0.05"), 0.05), (("--sparse", "-d", "0.05"), 0.05)):
        assert cli.main(["dist", "--top", "3", *extra, rp, qp]) == 0
        out = capsys.readouterr().out
        want = md.format_lines(ref_db, qry_db, *expected_rows(block, 64, 3, max_dist), max_dist, 1.0)
        assert out == "".join(l + "\n" for l in want) and len(want) > 0
    for bad in (["--top", "3", "-t"], ["--top", "3", "-v", "0.5"], ["--top", "0"], ["--top", str(md.topk_max() + 1)]):
        assert cli.main(["dist", *bad, rp, qp]) != 0
        cap = capsys.readouterr()
        assert cap.out == "" and "usage: dist" in cap.err
