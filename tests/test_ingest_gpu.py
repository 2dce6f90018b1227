"""Device half of the ingest, kernel by kernel: hymet_pack (csrc/pack.hip), hymet_fasta_compact
and hymet_name_hash (csrc/ingest.hip), each against a plain reference written here from the
documented layout (include/hymet_gpu.h) or against seqio.parse_fasta_bytes.  Every comparison is
exact (bytes and integers).  Sizes sit on the edges of the 32-base thread tile, the 16-base
word, the 256-thread block and the 8 KiB compaction chunk."""
import ctypes

import numpy as np
import pytest

from hymet_amd.seqio import from_records, parse_fasta_bytes

needs_gpu = pytest.mark.gpu

SENT8 = 0xA5          # sentinel byte of pre-filled outputs
SENT32 = 0x5A5A5A5A   # sentinel word
PAD = 8               # sentinel words / 8-byte groups kept past every output
CHUNK = 8192          # raw bytes per compaction chunk (ingest.hip)


@pytest.fixture(scope="module")
def gpu():
    from hymet_amd._lib import Gpu
    return Gpu(0)


def _vp(t, off=0):
    return ctypes.c_void_p(t.data_ptr() + off)


def _np_vp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _dev(gpu, a):
    return gpu.torch.from_numpy(np.ascontiguousarray(a)).to(gpu.dev)


def _dev_bytes(gpu, b: bytes):
    return _dev(gpu, np.frombuffer(b or b"\0", np.uint8).copy())


# ------------------------------------------------------------------------------- hymet_pack
ACCEPT = {0: b"ACGTacgt", 1: b"ACGT", 2: b"ACGTUacgtu"}
CODE = {ord("A"): 0, ord("C"): 1, ord("G"): 2, ord("T"): 3, ord("U"): 3}
PACK_NS = sorted({1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 8191, 8192, 8193, 256 * 32 - 1, 256 * 32 + 1})


def _pack_ref(a: np.ndarray, alphabet: int):
    """The header's layout, base by base: (2-bit words, mask words)."""
    n = len(a)
    code = np.zeros(256, np.uint32)
    bad = np.ones(256, np.uint32)
    for c in ACCEPT[alphabet]:
        code[c] = CODE[ord(chr(c).upper())]
        bad[c] = 0
    w2b = np.zeros((n + 15) // 16, np.uint32)
    wm = np.zeros((n + 31) // 32, np.uint32)
    i = np.arange(n)
    np.bitwise_or.at(w2b, i // 16, code[a] << (2 * (i % 16)).astype(np.uint32))   # an invalid base packs as 0
    np.bitwise_or.at(wm, i // 32, bad[a] << (i % 32).astype(np.uint32))
    t = np.arange(n, 32 * len(wm))   # positions at or past n in the last mask word: invalid, code 0
    np.bitwise_or.at(wm, t // 32, np.uint32(1) << (t % 32).astype(np.uint32))
    return w2b, wm


def _pack_input(n: int, seed: int) -> np.ndarray:
    """Shuffled blocks of all 256 byte values, every other byte replaced by a letter that
    some alphabet accepts (so short inputs hold valid bases too)."""
    rng = np.random.default_rng(seed)
    a = np.concatenate([rng.permutation(256) for _ in range(n // 256 + 1)])[:n].astype(np.uint8)
    letters = np.frombuffer(b"ACGTUacgtuNn", np.uint8)
    pick = rng.random(n) < 0.5
    a[pick] = rng.choice(letters, int(pick.sum()))
    return a


def _run_pack(gpu, a: np.ndarray, n: int, alphabet: int, misalign: int = 0):
    torch = gpu.torch
    d_a = gpu.zeros(len(a) + 64, torch.uint8)
    d_a[misalign:misalign + len(a)].copy_(torch.from_numpy(a))
    d_2b = torch.full(((n + 15) // 16 + PAD,), SENT32, dtype=torch.int32, device=gpu.dev)
    d_m = torch.full(((n + 31) // 32 + PAD,), SENT32, dtype=torch.int32, device=gpu.dev)
    try:
        gpu.call("hymet_pack", _vp(d_a, misalign), n, alphabet, _vp(d_2b), _vp(d_m))
    finally:
        gpu.sync()
    return d_2b.cpu().numpy().view(np.uint32), d_m.cpu().numpy().view(np.uint32)


@needs_gpu
@pytest.mark.parametrize("alphabet", [0, 1, 2])
def test_pack_every_byte_value(gpu, alphabet):
    """All 256 byte values, shuffled: the three code tables (alphabet 1 rejects lower case,
    alphabet 2 alone takes U/u), and a short tail after eight full thread tiles."""
    a = np.random.default_rng(11 + alphabet).permutation(256).astype(np.uint8)
    a = np.concatenate([a, a[::-1][:9]])
    w2b, wm = _run_pack(gpu, a, len(a), alphabet)
    r2b, rm = _pack_ref(a, alphabet)
    np.testing.assert_array_equal(w2b[:len(r2b)], r2b)
    np.testing.assert_array_equal(wm[:len(rm)], rm)
    ok = np.frombuffer(ACCEPT[alphabet], np.uint8)
    valid = ~((rm[np.arange(len(a)) // 32] >> (np.arange(len(a)) % 32).astype(np.uint32)) & 1).astype(bool)
    np.testing.assert_array_equal(valid, np.isin(a, ok))   # the reference itself: accepted set == unflagged set


@needs_gpu
@pytest.mark.parametrize("alphabet", [0, 1, 2])
@pytest.mark.parametrize("n", PACK_NS)
def test_pack_tile_word_and_block_edges(gpu, n, alphabet):
    """Edges of the 32-base thread tile, the 16-base word and the 256-thread block: exact words,
    tail positions of the last mask word flagged invalid with code 0, and nothing written past
    ceil(n/16) and ceil(n/32) words."""
    a = _pack_input(n, 1000 * alphabet + n)
    w2b, wm = _run_pack(gpu, a, n, alphabet)
    r2b, rm = _pack_ref(a, alphabet)
    np.testing.assert_array_equal(w2b[:len(r2b)], r2b)
    np.testing.assert_array_equal(wm[:len(rm)], rm)
    if n % 32:
        assert int(rm[-1]) >> (n % 32) == (1 << (32 - n % 32)) - 1   # the reference's own tail: all flagged
        assert int(wm[len(rm) - 1]) >> (n % 32) == (1 << (32 - n % 32)) - 1
    if n % 16:
        assert int(w2b[len(r2b) - 1]) >> (2 * (n % 16)) == 0
    assert (w2b[len(r2b):] == SENT32).all() and len(w2b) == len(r2b) + PAD
    assert (wm[len(rm):] == SENT32).all() and len(wm) == len(rm) + PAD


@needs_gpu
def test_pack_zero_bases_writes_nothing(gpu):
    w2b, wm = _run_pack(gpu, np.frombuffer(b"ACGT" * 8, np.uint8).copy(), 0, 2)
    assert (w2b == SENT32).all() and (wm == SENT32).all()


@needs_gpu
def test_pack_rejects_unaligned_input(gpu):
    """The kernel reads 16 bytes at a time: a pointer one byte past an aligned address is an
    argument error, reported before anything is written."""
    from hymet_amd._lib import HymetError
    torch = gpu.torch
    a = _pack_input(100, 5)
    d_a = gpu.zeros(256, torch.uint8)
    d_a[1:101].copy_(torch.from_numpy(a))
    assert d_a.data_ptr() % 16 == 0
    d_2b = torch.full((7 + PAD,), SENT32, dtype=torch.int32, device=gpu.dev)
    d_m = torch.full((4 + PAD,), SENT32, dtype=torch.int32, device=gpu.dev)
    with pytest.raises(HymetError):
        gpu.call("hymet_pack", _vp(d_a, 1), 100, 0, _vp(d_2b), _vp(d_m))
    gpu.sync()
    assert (d_2b.cpu().numpy().view(np.uint32) == SENT32).all()
    assert (d_m.cpu().numpy().view(np.uint32) == SENT32).all()


# ---------------------------------------------------------------------- hymet_fasta_compact
def _bases(n: int, seed: int) -> bytes:
    return np.random.default_rng(seed).choice(np.frombuffer(b"ACGTNacgtn", np.uint8), n).tobytes()


def _wrap(seq: bytes, width: int, eol: bytes = b"\n") -> bytes:
    return b"".join(seq[i:i + width] + eol for i in range(0, len(seq), width))


def _body_of_raw_len(L: int, seed: int, width: int = 61) -> bytes:
    """A wrapped sequence body of exactly L raw bytes (line breaks included), not ending in a
    line break: the record's raw sequence range when another record follows."""
    if L == 0:
        return b""
    out = bytearray(_wrap(_bases(L, seed), width)[:L])
    if out[-1:] == b"\n":
        out[-1:] = b"A"
    return bytes(out)


def _compact_file():
    """(FASTA text whose records hit every chunk-edge case, the record names in file order).
    A record's chunks start at its own sequence offset, so every edge below is an offset into
    the record's body."""
    recs = []   # (header, body); the body is followed by "\n" unless it is the file's last record

    def add(name, body):
        recs.append((name, body))

    add("empty_first", b"")
    for L in (0, 1, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 5):
        add(f"raw{L} length={L}", _body_of_raw_len(L, L))
    # CRLF split by a chunk edge: '\r' is byte 8191 of the body, '\n' byte 8192
    add("crlf_split", _bases(CHUNK - 1, 21) + b"\r\n" + _wrap(_bases(500, 22), 70, b"\r\n") + _bases(33, 23))
    # '\n' as the last byte of a chunk, and as the first byte of the next one
    add("lf_chunk_last", _bases(CHUNK - 1, 24) + b"\n" + _bases(100, 25))
    add("lf_chunk_first", _bases(CHUNK, 26) + b"\n" + _bases(100, 27) + b"\n" + _bases(CHUNK - 103, 28) + b"\n" + _bases(7, 29))
    add("only_breaks", b"\n" * 70 + b"\r\n" * 20 + b"\r" * 3)
    add("empty_middle", b"")
    add("\tws_before_name  and a comment", _wrap(_bases(200, 30), 60).rstrip(b"\n"))
    # width 7: a line break every 8 bytes, 1,024 of them per chunk and four per thread span;
    # width 1: every other byte; a 40-byte run of breaks: a whole thread span kept nothing
    add("width7", _wrap(_bases(2 * CHUNK + 100, 31), 7).rstrip(b"\n"))
    add("width1", _wrap(_bases(CHUNK // 2 + 9, 32), 1).rstrip(b"\n"))
    add("break_run", _bases(50, 33) + b"\n" * 40 + _bases(3 * 32 + 5, 34) + b"\r\n" * 16 + _bases(9, 35))
    add("crlf_lines with a CRLF header\r", _wrap(_bases(CHUNK + 300, 36), 80, b"\r\n").rstrip(b"\r\n"))
    add("empty_before_last", b"")
    add("no_terminator", _bases(CHUNK + 77, 37))   # a single line, no '\n' at end of file
    data = b"".join(b">" + h.encode() + b"\n" + b + b"\n" for h, b in recs)[:-1]
    return data, [h.split()[0] if h.split() else "" for h, _ in recs]


def _compact(gpu, fx, r0, r1, d_all=None, d_base=0):
    """hymet_fasta_compact on records [r0, r1) with QueryShard.from_fasta's arguments (its own
    upload of the records' byte range, or bytes already resident from file offset d_base on),
    into a sentinel-filled pool.  Returns (pool bytes with padding, pool_len, pool starts)."""
    torch = gpu.torch
    n = r1 - r0
    nb = np.ascontiguousarray(fx.nbases[r0:r1])
    pool_len = int(nb.sum()) + max(n - 1, 0)
    lo = int(min(fx.name_off[r0], fx.seq_off[r0]))
    hi = int(fx.seq_end[r1 - 1])
    if d_all is not None:
        assert lo >= d_base and hi - d_base <= d_all.numel()
        d_raw, lo = d_all, d_base
    else:
        d_raw = _dev_bytes(gpu, fx.data[lo:hi])
    d_pool = torch.full((max(pool_len, 1) + 16 + 8 * PAD,), SENT8, dtype=torch.uint8, device=gpu.dev)
    d_start = torch.full((n + PAD,), -SENT32, dtype=torch.int64, device=gpu.dev)
    so = np.ascontiguousarray(fx.seq_off[r0:r1])
    se = np.ascontiguousarray(fx.seq_end[r0:r1])
    gpu.call("hymet_fasta_compact", _vp(d_raw), hi - lo, lo, _np_vp(so), _np_vp(se), _np_vp(nb), n, _vp(d_pool), pool_len,
             _vp(d_start))
    gpu.sync()
    start = d_start.cpu().numpy()
    assert (start[n:] == -SENT32).all()
    return d_pool.cpu().numpy().tobytes(), pool_len, start[:n]


@pytest.fixture(scope="module")
def compact_file():
    """(FASTA bytes, its record table, the whole-file parse): host work only."""
    from hymet_amd.ingest import FastaIndex
    data, names = _compact_file()
    fx = FastaIndex(data, threads=1)
    ref = parse_fasta_bytes(data)
    assert [r[0] for r in ref] == names and fx.n == len(ref)
    return data, fx, ref


@pytest.fixture(scope="module")
def compact_case(gpu, compact_file):
    """The file above plus its bytes resident in HBM (a whole-file upload)."""
    data, fx, ref = compact_file
    return data, fx, ref, _dev_bytes(gpu, data)


def _check_pool(got, ref_records):
    pool, pool_len, start = got
    want = from_records(ref_records)   # sequences joined by one 'N', each record's pool start
    assert pool_len == len(want.buf)
    assert pool[:pool_len] == want.buf
    np.testing.assert_array_equal(start, want.starts)
    assert pool[pool_len:] == bytes([SENT8]) * (len(pool) - pool_len)   # nothing at or past pool_len


def test_compact_file_has_the_edge_cases(compact_file):
    """No GPU work: the constructed file really holds the raw range lengths and the byte
    patterns at chunk edges that the tests below rely on."""
    data, fx, ref = compact_file
    raw_len = (fx.seq_end - fx.seq_off).tolist()
    for L in (0, 1, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 5):
        assert L in raw_len
    by = {r[0]: i for i, r in enumerate(ref)}

    def body(name):
        return data[fx.seq_off[by[name]]:fx.seq_end[by[name]]]
    assert body("crlf_split")[CHUNK - 1:CHUNK + 1] == b"\r\n"
    assert body("lf_chunk_last")[CHUNK - 1:CHUNK] == b"\n"
    b = body("lf_chunk_first")
    assert b[CHUNK:CHUNK + 1] == b"\n" and b[2 * CHUNK - 1:2 * CHUNK] == b"\n"
    assert fx.nbases[by["only_breaks"]] == 0 and len(body("only_breaks")) > 64
    assert body("width7")[:CHUNK].count(b"\n") == CHUNK // 8
    assert [fx.nbases[by[k]] for k in ("empty_first", "empty_middle", "empty_before_last")] == [0, 0, 0]
    assert by["empty_first"] == 0 and by["no_terminator"] == fx.n - 1 and not data.endswith(b"\n")
    assert len(ref[by["no_terminator"]][2]) == CHUNK + 77


@needs_gpu
def test_compact_whole_file(gpu, compact_case):
    """Every record of the file in one call, from the call's own upload (raw_base = 0 only
    because the first record starts the file)."""
    data, fx, ref, _ = compact_case
    _check_pool(_compact(gpu, fx, 0, fx.n), ref)


def _ranges(n):
    """Record ranges: every single record (each edge case alone, first and last of its shard),
    shards that start mid-file, and shards that begin or end with an empty record."""
    out = [(i, i + 1) for i in range(n)]
    out += [(1, n), (3, 9), (7, 12), (11, n), (n - 2, n), (0, 2), (11, 13)]
    return out


@needs_gpu
def test_compact_shard_with_its_own_upload(gpu, compact_case):
    """Records [r0, r1) with r0 > 0 and only their byte range uploaded: raw_base != 0."""
    data, fx, ref, _ = compact_case
    for r0, r1 in _ranges(fx.n):
        _check_pool(_compact(gpu, fx, r0, r1), ref[r0:r1])


@needs_gpu
def test_compact_shard_from_resident_bytes(gpu, compact_case):
    """The same records taken from bytes already in HBM: the whole file (d_base = 0), and the
    file from an odd offset on (d_base > 0, so no record or chunk is aligned in the upload)."""
    data, fx, ref, d_all = compact_case
    for r0, r1 in _ranges(fx.n):
        _check_pool(_compact(gpu, fx, r0, r1, d_all=d_all, d_base=0), ref[r0:r1])
    r0 = 3
    d_base = int(fx.name_off[r0]) - 1   # the record's '>'
    d_tail = _dev_bytes(gpu, data[d_base:])
    for r1 in (4, 9, fx.n):
        _check_pool(_compact(gpu, fx, r0, r1, d_all=d_tail, d_base=d_base), ref[r0:r1])


def _unpack(w2b, wm, n):
    i = np.arange(n)
    return ((w2b[i // 16] >> (2 * (i % 16)).astype(np.uint32)) & 3), ((wm[i // 32] >> (i % 32).astype(np.uint32)) & 1)


@needs_gpu
@pytest.mark.parametrize("route", ["upload", "resident"])
@pytest.mark.parametrize("r0,r1", [(0, None), (7, 16)])
def test_query_shard_from_fasta(gpu, compact_case, r0, r1, route):
    """QueryShard.from_fasta end to end on the same file (compaction, then both packed pools
    and the name hashes): the packed pools are the reference packing of the expected pool."""
    from hymet_amd.ingest import QueryShard
    data, fx, ref, d_all = compact_case
    r1 = fx.n if r1 is None else r1
    sh = QueryShard.from_fasta(gpu, fx, r0, r1, d_all=d_all if route == "resident" else None)
    gpu.sync()
    want = from_records(ref[r0:r1])
    np.testing.assert_array_equal(sh.lengths, want.lengths)
    np.testing.assert_array_equal(sh.starts, want.starts)
    a = np.frombuffer(want.buf, np.uint8)
    for pp, alphabet in ((sh.mash, 0), (sh.mm, 2)):
        r2b, rm = _pack_ref(a, alphabet)
        np.testing.assert_array_equal(pp.w2b.cpu().numpy().view(np.uint32)[:len(r2b)], r2b)
        np.testing.assert_array_equal(pp.wmask.cpu().numpy().view(np.uint32)[:len(rm)], rm)
    names = [data[o:o + l] for o, l in zip(fx.name_off[r0:r1].tolist(), fx.name_len[r0:r1].tolist())]
    np.testing.assert_array_equal(sh.name_hash.cpu().numpy().view(np.uint32), np.array([_x31(s) for s in names], np.uint32))


# -------------------------------------------------------------------------- hymet_name_hash
def _x31(s: bytes) -> int:
    """khash's __ac_X31_hash_string over signed chars, modulo 2^32."""
    if not s:
        return 0
    sc = [c - 256 if c >= 128 else c for c in s]
    h = sc[0]
    for c in sc[1:]:
        h = h * 31 + c
    return h % (1 << 32)


def _hash_names():
    rng = np.random.default_rng(41)
    # bytes a FASTA name can hold: no white space, no NUL, no '>'
    ok = np.array([c for c in range(1, 256) if c not in b"\t\n\v\f\r >"], np.uint8)
    names = [b"", b"A", b"\x80", b"\xff", b"\xc3\xa9\x80\xfe\x7f\x81", b"k141_3", bytes(rng.choice(ok, 300)),
             bytes(rng.choice(ok[ok >= 128], 40))]
    names += [bytes(rng.choice(ok, int(rng.integers(1, 40)))) for _ in range(1000)]
    names.append(b"")
    return names


def test_x31_reference_values():
    """The reference hash itself, against values worked out by hand from the definition."""
    assert _x31(b"") == 0
    assert _x31(b"A") == 65
    assert _x31(b"AB") == 65 * 31 + 66
    assert _x31(b"\x80") == 2 ** 32 - 128                         # a high byte is negative
    assert _x31(b"\xff\x01") == (2 ** 32 - 31 + 1)                # -1 * 31 + 1
    assert _x31(b"\x01\xff") == 30                                # 31 - 1
    assert _x31(b"\x80") != 0x80 and _x31(b"a\xff") != ord("a") * 31 + 255



def _run_hash(gpu, d_bytes, off, length):
    n = len(off)
    d_hash = gpu.torch.full((n + PAD,), SENT32, dtype=gpu.torch.int32, device=gpu.dev)
    d_off = _dev(gpu, np.asarray(off, np.int64))      # named: both stay allocated until the kernel is done
    d_len = _dev(gpu, np.asarray(length, np.int32))
    assert int((np.asarray(off, np.int64) + length).max()) <= d_bytes.numel() and int(np.min(off)) >= 0 and len(length) == n
    gpu.call("hymet_name_hash", _vp(d_bytes), _vp(d_off), _vp(d_len), n, _vp(d_hash))
    gpu.sync()
    got = d_hash.cpu().numpy().view(np.uint32)
    assert (got[n:] == SENT32).all()
    return got[:n]


@needs_gpu
def test_name_hash_offsets_into_fasta_bytes(gpu):
    """from_fasta's layout: names hashed where they stand in the uploaded FASTA bytes, offsets
    relative to the uploaded range (here a range that starts mid-file)."""
    from hymet_amd.ingest import FastaIndex
    names = _hash_names()
    data = b"".join(b">" + s + (b" some comment" if s and i % 3 == 0 else b"") + b"\nACGT\nAC\n" for i, s in enumerate(names))
    fx = FastaIndex(data, threads=1)
    assert fx.n == len(names)
    assert [data[o:o + l] for o, l in zip(fx.name_off.tolist(), fx.name_len.tolist())] == names
    want = np.array([_x31(s) for s in names], np.uint32)
    for r0 in (0, 5):
        lo = int(min(fx.name_off[r0], fx.seq_off[r0]))
        got = _run_hash(gpu, _dev_bytes(gpu, data[lo:]), fx.name_off[r0:] - lo, fx.name_len[r0:])
        np.testing.assert_array_equal(got, want[r0:])


@needs_gpu
def test_name_hash_offsets_into_a_name_pool(gpu):
    """from_seqset's layout: the names back to back in a compact pool."""
    names = _hash_names()
    off = np.zeros(len(names) + 1, np.int64)
    np.cumsum([len(s) for s in names], out=off[1:])
    got = _run_hash(gpu, _dev_bytes(gpu, b"".join(names)), off[:-1], np.diff(off))
    np.testing.assert_array_equal(got, np.array([_x31(s) for s in names], np.uint32))


@needs_gpu
def test_name_hash_high_bytes_sign_extend(gpu):
    """Names made of bytes >= 0x80 only, where a hash over unsigned chars differs in every
    value (checked here against such a hash, so the inputs can tell the two apart)."""
    rng = np.random.default_rng(43)
    names = [bytes(rng.integers(128, 256, int(rng.integers(1, 24)), dtype=np.uint8)) for _ in range(300)]
    off = np.zeros(len(names) + 1, np.int64)
    np.cumsum([len(s) for s in names], out=off[1:])
    want = np.array([_x31(s) for s in names], np.uint32)
    unsigned = []
    for s in names:
        h = 0
        for c in s:
            h = (h * 31 + c) % (1 << 32)
        unsigned.append(h)
    assert (want != np.array(unsigned, np.uint32)).all()
    got = _run_hash(gpu, _dev_bytes(gpu, b"".join(names)), off[:-1], np.diff(off))
    np.testing.assert_array_equal(got, want)


@needs_gpu
def test_query_shard_from_seqset_hashes_names(gpu):
    """QueryShard.from_seqset: names encoded to UTF-8 (multi-byte characters are high bytes),
    hashed from the compact name pool."""
    from hymet_amd.ingest import QueryShard
    names = ["k141_3", "contig_é_ü", "x", "ß" * 50, "plain_name_2"]
    ss = from_records([(n, "", b"ACGTACGTAC" * (i + 1)) for i, n in enumerate(names)])
    sh = QueryShard.from_seqset(gpu, ss)
    gpu.sync()
    np.testing.assert_array_equal(sh.name_hash.cpu().numpy().view(np.uint32),
                                  np.array([_x31(n.encode()) for n in names], np.uint32))
    a = np.frombuffer(ss.buf, np.uint8)
    r2b, rm = _pack_ref(a, 2)
    np.testing.assert_array_equal(sh.mm.w2b.cpu().numpy().view(np.uint32)[:len(r2b)], r2b)
    np.testing.assert_array_equal(sh.mm.wmask.cpu().numpy().view(np.uint32)[:len(rm)], rm)
