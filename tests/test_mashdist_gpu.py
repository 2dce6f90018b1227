"""GPU dist (csrc/mash_dist.hip through hymet_amd.mashdist and `cli dist`) vs a literal Python
transcription of Mash's merge loop: exact equality of every pair's (common, denom)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from tests._data import add_noise, mutate, rand_seq, revcomp

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_CAPACITY = -2, -3
K = 21
PARITY_SIZES = (1, 2, 63, 64, 65, 1000, 1025)


def merge_loop(A, B, s):
    """Mash's pair loop, as DESIGN.md §Dist states it.  A, B: lists of Python ints."""
    i = j = common = denom = 0
    while denom < s and i < len(A) and j < len(B):
        if A[i] < B[j]:
            i += 1
        elif B[j] < A[i]:
            j += 1
        else:
            i += 1
            j += 1
            common += 1
        denom += 1
    if denom < s:
        denom += (len(A) - i) + (len(B) - j)
        denom = min(denom, s)
    return common, denom


def expected(ref_lists, qry_lists, s):
    """The dense block the device must write: rows = queries, packed common << 16 | denom."""
    R = [np.asarray(a, np.uint64).tolist() for a in ref_lists]
    Q = [np.asarray(b, np.uint64).tolist() for b in qry_lists]
    out = np.zeros((len(Q), len(R)), np.uint32)
    for q, B in enumerate(Q):
        for r, A in enumerate(R):
            c, d = merge_loop(A, B, s)
            out[q, r] = c << 16 | d
    return out


def make_db(lists, s, prefix="x", lengths=None):
    from hymet_amd.msh import SketchDB
    lists = [np.asarray(a, np.uint64) for a in lists]
    off = np.zeros(len(lists) + 1, np.int64)
    if lists:
        off[1:] = np.cumsum([len(a) for a in lists])
    return SketchDB(k=K, seed=42, sketch_size=int(s), names=[f"{prefix}{i}" for i in range(len(lists))],
                    comments=[""] * len(lists),
                    lengths=np.asarray(lengths if lengths is not None else [100_000] * len(lists), np.int64), offsets=off,
                    hashes=np.concatenate(lists) if lists else np.zeros(0, np.uint64))


def dense(gpu, ref_db, qry_db, s, q0=0, q1=None):
    from hymet_amd import mashdist as md
    R, Q = md.DeviceSketches(gpu, ref_db), md.DeviceSketches(gpu, qry_db)
    q1 = Q.n if q1 is None else q1
    blk = md.dist_block(gpu, R, Q, q0, q1, s)
    gpu.sync()
    return blk[:(q1 - q0) * R.n].cpu().numpy().view(np.uint32).reshape(q1 - q0, R.n)


def _draw(rng, pool, n):
    return np.sort(rng.choice(pool, size=n, replace=False))


def parity_lists(s, n_ref=17, n_qry=5):
    """Seeded lists of lengths from {0, 1, s - 1, s, s + 5} over shared pools: a narrow pool
    (lists overlap almost wholly), a wide one and a separate one (disjoint pairs); one query
    equals a reference.  The same for every caller, the child process of the path test included."""
    rng = np.random.default_rng(1000 + s)
    wide = np.unique(rng.integers(0, 2 ** 64, size=3 * s + 16, dtype=np.uint64))
    apart = np.unique(rng.integers(0, 2 ** 64, size=s + 16, dtype=np.uint64))
    pools = [wide[:s + 6], wide, apart]
    lens = [0, 1, s - 1, s, s + 5]

    def some(n, shift):
        out = []
        for i in range(n):
            L = lens[(i + shift) % 5] if i < 10 else int(rng.choice(lens))
            out.append(_draw(rng, pools[i % 3], L))
        return out

    refs, qrys = some(n_ref, 0), some(n_qry, 2)
    full = [i for i, a in enumerate(refs) if len(a) >= s]
    qrys[0] = refs[full[0]].copy()
    return refs, qrys


@pytest.fixture(scope="module")
def gpu():
    from hymet_amd._lib import Gpu
    return Gpu(0)


_PARITY = {}


def _parity_block(gpu, s):
    if s not in _PARITY:
        refs, qrys = parity_lists(s)
        _PARITY[s] = (refs, qrys, dense(gpu, make_db(refs, s), make_db(qrys, s), s))
    return _PARITY[s]


@pytest.mark.parametrize("s", PARITY_SIZES)
def test_parity_awkward_shapes(gpu, s):
    refs, qrys, got = _parity_block(gpu, s)
    assert {len(a) for a in refs} == {0, 1, s - 1, s, s + 5}
    want = expected(refs, qrys, s)
    np.testing.assert_array_equal(got, want)
    c, d = want >> 16, want & 0xFFFF
    if s >= 63:   # the shapes range from disjoint to identical
        assert (c == 0).any() and ((c == d) & (d == s)).any() and ((c > 0) & (c < d)).any()


def cut_lists(s):
    """Pairs over 2s distinct values with a prescribed class per union rank (0-based; the s-th
    element has rank s - 1).  Classes: 'a' A only, 'b' B only, 'c' both."""
    rng = np.random.default_rng(77 + s)
    vals = np.sort(np.unique(rng.integers(0, 2 ** 64, size=2 * s + 8, dtype=np.uint64))[:2 * s])
    tails = ["c", "ac", "bc"]            # ends at the cut: common; A-only then common; B-only then common
    refs, qrys = [], []
    for union_len in (2 * s, s - 1):
        for tail in tails:
            cls = ["abc"[(r * 7 + r // 5) % 3] for r in range(union_len)]
            if union_len > s:            # the tail's first class sits at rank s - 1
                at = s - 1
                if s >= 3:
                    cls[s - 2] = "b" if tail[0] == "a" else "a"
            else:                        # the tail ends the (shorter) union
                at = union_len - len(tail)
            if at >= 0:
                for n, ch in enumerate(tail):
                    cls[at + n] = ch
            v = vals[:union_len]
            pick = np.array(cls)
            refs.append(v[(pick == "a") | (pick == "c")])
            qrys.append(v[(pick == "b") | (pick == "c")])
    return refs, qrys


@pytest.mark.parametrize("s", [64, 1000])
def test_cut_at_union_rank_s(gpu, s):
    refs, qrys = cut_lists(s)
    want = expected(refs, qrys, s)
    # the cases are what they claim: with the union longer than s, a common element at rank
    # s - 1 counts and one at rank s does not
    for n, tail in enumerate(["c", "ac", "bc"]):
        A, B = refs[n].tolist(), qrys[n].tolist()
        union = sorted(set(A) | set(B))
        both = set(A) & set(B)
        assert len(union) == 2 * s
        assert (union[s - 1] in both) == (tail == "c")
        assert union[s] in both or tail == "c"
        assert want[n, n] >> 16 == len(both & set(union[:s])) and want[n, n] & 0xFFFF == s
    for n in (3, 4, 5):
        assert want[n, n] & 0xFFFF == s - 1
    got = dense(gpu, make_db(refs, s), make_db(qrys, s), s)
    np.testing.assert_array_equal(got, want)


def test_unsigned_order_and_no_sentinel(gpu):
    top = 2 ** 64 - 1
    refs = [[5, 2 ** 63 - 1, 2 ** 63, 2 ** 63 + 7, top - 1, top], [1, 2 ** 63, top - 1], [top], [],
            [3, 2 ** 62, 2 ** 63 - 1, 2 ** 63 + 7, top]]
    qrys = [[5, 2 ** 63, top], [2 ** 63 - 1, 2 ** 63 + 7, top - 1], [top], [top - 1], [],
            [0, 5, 2 ** 63 - 1, 2 ** 63, 2 ** 63 + 1, top - 1]]
    for s in (1, 3, 4, 6, 64):
        want = expected(refs, qrys, s)
        got = dense(gpu, make_db(refs, s), make_db(qrys, s), s)
        np.testing.assert_array_equal(got, want, err_msg=f"s={s}")
    want = expected(refs, qrys, 64)
    assert want[0, 0] == 3 << 16 | 6          # 2^64 - 1 in both lists is a shared hash
    assert want[2, 2] == 1 << 16 | 1
    assert want[2, 3] == 0 << 16 | 1          # in one list only: it counts in the union
    assert want[4, 3] == 0                    # two empty lists


_EDGE = {}


def _edge(gpu):
    """65 x 65 lists at s = 64 and their expected block, shared by the tests below."""
    if not _EDGE:
        refs, qrys = parity_lists(64, 65, 65)
        _EDGE.update(refs=refs, qrys=qrys, want=expected(refs, qrys, 64))
    return _EDGE["refs"], _EDGE["qrys"], _EDGE["want"]


def test_tile_edges_and_row_ranges(gpu):
    s = 64
    tq = gpu.lib.hymet_mash_dist_tile(s)
    assert tq >= 2, "s = 64 must take the tiled kernel"
    assert gpu.lib.hymet_mash_dist_tile(16384) == 0 and gpu.lib.hymet_mash_dist_tile(0) == 0
    refs, qrys, want = _edge(gpu)
    counts = sorted({1, tq - 1, tq, tq + 1, 65})
    for n_ref in counts:
        ref_db = make_db(refs[:n_ref], s)
        for n_qry in counts:
            got = dense(gpu, ref_db, make_db(qrys[:n_qry], s), s)
            np.testing.assert_array_equal(got, want[:n_qry, :n_ref], err_msg=f"{n_ref} x {n_qry}")
    ref_db, qry_db = make_db(refs, s), make_db(qrys, s)
    for q0, q1 in [(1, 2), (3, 3 + tq), (tq - 1, 2 * tq + 1), (tq, 65), (64, 65), (7, 7)]:
        got = dense(gpu, ref_db, qry_db, s, q0, q1)
        np.testing.assert_array_equal(got, want[q0:q1], err_msg=f"rows [{q0}, {q1})")
    assert dense(gpu, make_db([], s), qry_db, s).shape == (65, 0)       # zero references: not an error


def test_largest_sketch_size(gpu):
    from hymet_amd import sketch as sk
    s = sk.max_sketch_size()
    assert s == 16384
    rng = np.random.default_rng(5)
    pool = np.unique(rng.integers(0, 2 ** 64, size=2 * s + 64, dtype=np.uint64))
    refs = [_draw(rng, pool[:s + 40], s), _draw(rng, pool, s), pool[:s].copy()]
    qrys = [refs[0].copy(), _draw(rng, pool[:s + 40], s), _draw(rng, pool[s // 2:], s)]
    got = dense(gpu, make_db(refs, s), make_db(qrys, s), s)
    np.testing.assert_array_equal(got, expected(refs, qrys, s))
    assert got[0, 0] == s << 16 | s


def _child(out_path):
    """Run by test_both_paths_agree in a fresh process with HYMET_DIST_PATH=global."""
    from hymet_amd._lib import Gpu
    g = Gpu(0)
    assert all(g.lib.hymet_mash_dist_tile(s) == 0 for s in PARITY_SIZES), "the plain path was not forced"
    blocks = {}
    for s in PARITY_SIZES:
        refs, qrys = parity_lists(s)
        blocks[f"s{s}"] = dense(g, make_db(refs, s), make_db(qrys, s), s)
    np.savez(out_path, **blocks)


def test_both_paths_agree(gpu, tmp_path):
    assert gpu.lib.hymet_mash_dist_tile(1000) >= 2          # this process runs the tiled kernel
    out = tmp_path / "global.npz"
    env = dict(os.environ, HYMET_DIST_PATH="global")
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-m", "tests.test_mashdist_gpu", str(out)]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    z = np.load(out)
    for s in PARITY_SIZES:
        np.testing.assert_array_equal(z[f"s{s}"], _parity_block(gpu, s)[2], err_msg=f"s={s}")


def _collect(blocks):
    parts = list(blocks)
    return tuple(np.concatenate([p[i] for p in parts]) for i in range(4))


def test_blocking_does_not_matter(gpu):
    from hymet_amd import mashdist as md
    refs, qrys, want = _edge(gpu)
    ref_db, qry_db = make_db(refs, 64), make_db(qrys[:40], 64)
    for max_dist in (1.0, 0.3):
        runs = [_collect(md.dist_blocks(gpu, ref_db, qry_db, max_dist, block_bytes=bb)) for bb in (1 << 10, 1 << 16)]
        runs.append(_collect(md.dist_blocks(gpu, ref_db, qry_db, max_dist)))
        for other in runs[1:]:
            for a, b in zip(runs[0], other):
                np.testing.assert_array_equal(a, b)
        qi, ri, common, denom = runs[0]
        w = want[:40]
        keep = md.distance(w >> 16, w & 0xFFFF, K) <= max_dist
        wq, wr = np.nonzero(keep)                       # row-major: query-major, references in order
        np.testing.assert_array_equal(qi, wq)
        np.testing.assert_array_equal(ri, wr)
        np.testing.assert_array_equal(common, (w >> 16)[keep])
        np.testing.assert_array_equal(denom, (w & 0xFFFF)[keep])
        assert 0 < keep.sum() and (max_dist >= 1.0) == bool(keep.all())


def _select(gpu, block, n_rows, n_ref, table, s, cap, fill=0x5A5A5A5A):
    """One raw hymet_mash_dist_select call: rc, total, row offsets, and the whole output buffers
    (cap + 8 entries, pre-filled)."""
    from hymet_amd._lib import ptr
    torch = gpu.torch
    d_block = torch.from_numpy(np.ascontiguousarray(block).view(np.int32).reshape(-1).copy()).to(gpu.dev)
    d_table = torch.from_numpy(table.view(np.int16).copy()).to(gpu.dev)
    row_off = gpu.zeros(n_rows + 1, torch.int64)
    idx = torch.full((cap + 8,), fill, dtype=torch.int32, device=gpu.dev)
    val = torch.full((cap + 8,), fill, dtype=torch.int32, device=gpu.dev)
    total = ctypes.c_int64(-1)
    rc = gpu.lib.hymet_mash_dist_select(gpu.ctx, ptr(d_block), n_rows, n_ref, ptr(d_table), s, ptr(row_off), ptr(idx),
                                        ptr(val), cap, ctypes.byref(total))
    gpu.sync()
    return rc, total.value, row_off.cpu().numpy(), idx.cpu().numpy(), val.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("max_dist", [0.0, 0.05, 0.3])
def test_select_equals_host_filter(gpu, max_dist):
    from hymet_amd import mashdist as md
    _, _, edge = _edge(gpu)
    # a computed block, and a made-up one whose rows span several 256-reference rounds
    rng = np.random.default_rng(9)
    s2 = 1000
    d2 = rng.integers(0, s2 + 1, size=(5, 700))
    c2 = (d2 * rng.choice([0.0, 0.2, 0.5, 0.9, 1.0], size=d2.shape) + rng.integers(0, 2, size=d2.shape)).astype(np.int64)
    c2 = np.minimum(c2, d2)
    for s, block in ((64, edge), (s2, (c2 << 16 | d2).astype(np.uint32))):
        n_rows, n_ref = block.shape
        table = md.min_common_table(s, K, max_dist)
        keep = md.distance(block >> 16, block & 0xFFFF, K) <= max_dist
        wq, wr = np.nonzero(keep)
        total = int(keep.sum())
        assert total > 0
        rc, got_total, row_off, idx, val = _select(gpu, block, n_rows, n_ref, table, s, total)
        assert rc == 0 and got_total == total
        np.testing.assert_array_equal(row_off, np.r_[0, np.cumsum(keep.sum(axis=1))])
        np.testing.assert_array_equal(idx[:total], wr)
        np.testing.assert_array_equal(val[:total], block[keep])
        assert (idx[total:] == 0x5A5A5A5A).all() and (val[total:] == 0x5A5A5A5A).all()
        # a capacity one short: the true total, the offsets, and nothing written
        rc, got_total, row_off2, idx, val = _select(gpu, block, n_rows, n_ref, table, s, total - 1)
        assert rc == E_CAPACITY and got_total == total
        np.testing.assert_array_equal(row_off2, row_off)
        assert (idx == 0x5A5A5A5A).all() and (val == 0x5A5A5A5A).all()
        # and the host wrapper retries with the reported total
        d_block = gpu.torch.from_numpy(block.view(np.int32).reshape(-1).copy()).to(gpu.dev)
        d_table = gpu.torch.from_numpy(table.view(np.int16).copy()).to(gpu.dev)
        ro, ri, rv = md.select_block(gpu, d_block, n_rows, n_ref, d_table, s, cap=1)
        np.testing.assert_array_equal(ro, row_off)
        np.testing.assert_array_equal(ri, wr)
        np.testing.assert_array_equal(rv, block[keep])


def test_self_comparison(gpu):
    for s in (64, 1000):
        refs, qrys = parity_lists(s)
        lists = refs + qrys
        db = make_db(lists, s)
        got = dense(gpu, db, db, s)
        np.testing.assert_array_equal(got, got.T)
        diag = np.diagonal(got)
        np.testing.assert_array_equal(diag >> 16, diag & 0xFFFF)
        np.testing.assert_array_equal(diag & 0xFFFF, [min(s, len(a)) for a in lists])


def test_argument_checks(gpu):
    """Host-side rejections before any launch: nothing here makes the device read out of bounds."""
    from hymet_amd import mashdist as md
    from hymet_amd import sketch as sk
    from hymet_amd._lib import ptr
    torch = gpu.torch
    s = 64
    refs, qrys = parity_lists(s)
    R, Q = md.DeviceSketches(gpu, make_db(refs, s)), md.DeviceSketches(gpu, make_db(qrys, s))
    out = gpu.zeros(R.n * Q.n, torch.int32)

    def call(s=s, r_off=None, q_off=None, n_ref_hashes=None, n_qry_hashes=None, q0=0, q1=Q.n):
        return gpu.lib.hymet_mash_dist(gpu.ctx, ptr(R.hashes), R.n_hashes if n_ref_hashes is None else n_ref_hashes,
                                       ptr(R.offsets if r_off is None else r_off), R.n, ptr(Q.hashes),
                                       Q.n_hashes if n_qry_hashes is None else n_qry_hashes,
                                       ptr(Q.offsets if q_off is None else q_off), Q.n, q0, q1, s, ptr(out))

    def rejected(**kw):
        assert call(**kw) == E_ARG
        msg = gpu.lib.hymet_last_error()
        assert msg and b"hymet_mash_dist" in msg

    assert call() == 0
    assert call(q0=2, q1=2) == 0                       # zero rows
    rejected(s=0)
    rejected(s=sk.max_sketch_size() + 1)
    dec = R.offsets.clone()
    dec[3] = dec[4] + 1                                # offsets[3] > offsets[4]
    rejected(r_off=dec)
    dec = Q.offsets.clone()
    dec[2] = dec[1] - 1
    rejected(q_off=dec)
    rejected(n_ref_hashes=R.n_hashes - 1)              # the last offset lies past the array
    rejected(n_qry_hashes=Q.n_hashes - 1)
    neg = R.offsets.clone()
    neg[0] = -1
    rejected(r_off=neg)
    rejected(q0=0, q1=Q.n + 1)
    rejected(q0=-1, q1=2)
    rejected(q0=3, q1=2)
    gpu.sync()
    assert (out.cpu().numpy() != 0).any()              # the accepted calls did run


def _fasta(recs, width=70):
    out = []
    for name, seq in recs:
        out.append(b">" + name.encode() + b"\n")
        out.extend(seq[i:i + width] + b"\n" for i in range(0, len(seq), width))
    return b"".join(out)


def test_cli_dist_end_to_end(gpu, tmp_path, capsys):
    from hymet_amd import cli
    from hymet_amd import mashdist as md
    from oracle import oracle_lib
    rng = np.random.default_rng(41)
    k, seed, s = 21, 42, 400
    base = add_noise(rng, rand_seq(rng, 20_000))
    plasmid = rand_seq(rng, 8_000)
    ref_recs = [("chrA", base), ("plasmidB", plasmid), ("ctgC", rand_seq(rng, 3_000))]
    qry_recs = [("chrA_mut", mutate(rng, base, 0.02)), ("plasmidB_rc", revcomp(plasmid)), ("other", rand_seq(rng, 5_000))]
    (tmp_path / "refs.fna").write_bytes(_fasta(ref_recs))
    (tmp_path / "other.fna").write_bytes(_fasta(qry_recs))
    db_path = str(tmp_path / "db.msh")
    assert cli.main(["sketch", "-i", "-s", str(s), "-o", db_path, str(tmp_path / "refs.fna")]) == 0
    capsys.readouterr()

    def run(*flags):
        assert cli.main(["dist", *flags, db_path, str(tmp_path / "other.fna"), "-i"]) == 0
        return capsys.readouterr().out.splitlines()

    ref_lists = [oracle_lib.sketch([seq], k, seed, s) for _, seq in ref_recs]
    qry_lists = [oracle_lib.sketch([seq], k, seed, s) for _, seq in qry_recs]
    ref_db = make_db(ref_lists, s, lengths=[len(q) for _, q in ref_recs])
    qry_db = make_db(qry_lists, s, lengths=[len(q) for _, q in qry_recs])
    ref_db.names, qry_db.names = [n for n, _ in ref_recs], [n for n, _ in qry_recs]
    w = expected(ref_lists, qry_lists, s)
    qi, ri = np.repeat(np.arange(3), 3), np.tile(np.arange(3), 3)
    common, denom = (w >> 16).reshape(-1), (w & 0xFFFF).reshape(-1)
    want = md.format_lines(ref_db, qry_db, qi, ri, common, denom)
    lines = run()
    assert lines == want and len(lines) == 9
    rc_line = lines[4].split("\t")                     # plasmidB vs its reverse complement
    assert rc_line[:3] == ["plasmidB", "plasmidB_rc", "0"] and rc_line[4] == f"{s}/{s}"
    mut = lines[0].split("\t")
    assert mut[:2] == ["chrA", "chrA_mut"] and 0.005 < float(mut[2]) < 0.05
    near = run("-d", "0.1")
    assert near == md.format_lines(ref_db, qry_db, qi, ri, common, denom, max_dist=0.1)
    assert near == [lines[0], lines[4]]                # the unrelated pairs are gone
    assert run("-t") == md.format_table(ref_db, qry_db, common, denom)
    # from two .msh files
    assert cli.main(["dist", db_path, db_path]) == 0
    self_lines = capsys.readouterr().out.splitlines()
    assert len(self_lines) == 9 and [l.split("\t")[2] for l in self_lines[::4]] == ["0", "0", "0"]


if __name__ == "__main__":
    _child(sys.argv[1])
