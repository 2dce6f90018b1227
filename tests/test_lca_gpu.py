"""lca_wave_kernel / lca_row_seq (csrc/lca.hip, hymet_lca) and hymet_lca_ref_counts on rows built
to reach every multi-round path: rows on both sides of the 512-line switch, more than 64
distinct taxids and names, probe chains that wrap the 1,024-slot LDS dictionary, exact weight
ties within and across 64-lane rounds, and sums whose bit pattern depends on the order of the
additions.

The expectation is never a copy of the kernel: the integer tables handed to hymet_lca are
rendered as strings (taxid i -> "t{i}", name j -> "n{j}", target t -> "T{t}") and given to
oracle.classify_oracle.weighted_lca_cami / lca_legacy, which tests/test_classify_oracle.py pins
to the reference scripts' own outputs.  Every comparison is exact: depth, name ids, the shortcut
taxid, and the uint64 bit pattern of the confidence."""
import ctypes
from collections import defaultdict

import numpy as np
import pytest

from oracle import classify_oracle as co

needs_gpu = pytest.mark.gpu

RANKS = co.RANKS
NTAX = 1 << 18        # taxid indices and name ids stay below 2^18
ROUND = 64            # lanes per round of the wave kernel
LDS_LINES = 512       # the last row length handled in LDS


@pytest.fixture(scope="module")
def gpu():
    from hymet_amd._lib import Gpu
    return Gpu(0)


def _slots(keys):
    """Home slot of a key in the kernel's 1,024-slot dictionary.  Used to CHOOSE inputs only."""
    return ((np.asarray(keys, np.uint64) * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)) >> np.uint64(22)


_ALL = np.arange(1, NTAX)
STRESS = _ALL[_slots(_ALL) >= 1020].tolist()   # chains from here run past slot 1023 and wrap to slot 0
LOW = _ALL[_slots(_ALL) <= 60].tolist()        # keys at home where a wrapped chain lands
_RESERVED = set(STRESS) | set(LOW)


class _Lin(str):
    """A hierarchy lineage that knows its taxid.  lca_legacy's exact-match shortcut returns the
    hierarchy's own object; a weighted walk joins a new plain str."""
    tid = -1


class Tables:
    """The integer tables of one hymet_lca call, grown case by case, and their string form."""

    def __init__(self):
        self.tax_names = np.full((NTAX, 8), -1, np.int32)
        self.in_hier = np.zeros(NTAX, np.uint8)
        self.t_tax, self.counts = [], []
        self.used_tax, self._used = [], set()
        self._free_tax = (i for i in range(1, NTAX) if i not in _RESERVED)
        self._free_name = (i for i in range(1, NTAX) if i not in _RESERVED)
        self.rows = []      # (case name, lines); a line is (target, blen, qlen, exact)
        self.index = {}

    def name(self, at=None) -> int:
        return next(self._free_name) if at is None else at

    def names(self, k):
        return [self.name() for _ in range(k)]

    def taxid(self, names=(), in_hier=1, at=None) -> int:
        i = next(self._free_tax) if at is None else at
        assert i not in self._used
        self._used.add(i)
        n8 = list(names) + [-1] * (8 - len(names))
        self.tax_names[i] = n8
        self.in_hier[i] = in_hier
        self.used_tax.append(i)
        return i

    def target(self, tid, count=1) -> int:
        self.t_tax.append(tid)
        self.counts.append(count)
        return len(self.t_tax) - 1

    def add(self, case, lines):
        assert case not in self.index
        self.index[case] = len(self.rows)
        self.rows.append((case, [tuple(int(x) for x in ln) for ln in lines]))

    # ---- the arrays hymet_lca takes
    def arrays(self):
        q_off = np.zeros(len(self.rows) + 1, np.int64)
        np.cumsum([len(r[1]) for r in self.rows], out=q_off[1:])
        flat = np.array([ln for _, r in self.rows for ln in r], np.int64).reshape(-1, 4)
        return dict(q_off=q_off, line_t=flat[:, 0].astype(np.int32), line_blen=flat[:, 1].copy(),
                    line_qlen=flat[:, 2].copy(), line_exact=flat[:, 3].astype(np.uint8),
                    ref_counts=np.array(self.counts, np.int32), t_tax=np.array(self.t_tax, np.int32),
                    tax_names=self.tax_names.reshape(-1), tax_in_hier=self.in_hier)

    # ---- the same tables as the reference scripts' dictionaries
    def strings(self):
        hier_cami, hier_legacy = {}, {}
        for i in self.used_tax:
            nm = self.tax_names[i].tolist()
            if any(j >= 0 for j in nm):   # no name at any rank = no hierarchy row for the CAMI walk
                hier_cami[f"t{i}"] = [f"n{j}" if j >= 0 else "" for j in nm]
            if self.in_hier[i]:
                lin = _Lin(";".join(f"{RANKS[r]}:n{j}" for r, j in enumerate(nm) if j >= 0))
                lin.tid = i
                hier_legacy[f"t{i}"] = lin
        tax = {f"T{t}": f"t{i}" for t, i in enumerate(self.t_tax) if i >= 0}
        counts = {f"T{t}": c for t, c in enumerate(self.counts)}
        return hier_cami, hier_legacy, tax, counts


def _bits(x: float) -> int:
    return int(np.array([x], np.float64).view(np.uint64)[0])


def _parse(lin: str, sep: str):
    names = []
    if lin != "Unknown":
        for r, part in enumerate(lin.split(sep)):
            rank, nm = part.split(":")
            assert rank == RANKS[r] and nm.startswith("n")
            names.append(int(nm[1:]))
    return len(names), tuple(names)


def expect(T: Tables, S, lines, mode: int):
    """(depth, names[:depth], shortcut taxid, confidence bits) from the oracle functions."""
    hier_cami, hier_legacy, tax, counts = S
    if mode == 0:
        tw, hit = defaultdict(float), False     # classify_cami's loop, line by line
        for t, blen, qlen, _ in lines:
            tid = tax.get(f"T{t}")
            if not tid:
                continue
            hit = True
            cov = (blen / qlen) if qlen > 0 else 0.0
            tw[tid] += cov * counts.get(f"T{t}", 1)
        lin, _, conf = co.weighted_lca_cami(tw, hier_cami) if hit else ("Unknown", "root", 0.0)
        return _parse(lin, "; ") + (-1, _bits(conf))
    refs = [(f"T{t}", (blen / qlen if qlen > 0 else 0), bool(ex)) for t, blen, qlen, ex in lines]
    lin, _, conf = co.lca_legacy(refs, counts, tax, hier_legacy)
    if isinstance(lin, _Lin):
        return -1, (), lin.tid, _bits(conf)
    return _parse(lin, ";") + (-1, _bits(conf))


# ------------------------------------------------------------------------------ the cases
def _weights(rng, m):
    """Ordinary line weights: blen / qlen in (0, 1.5], any double."""
    return rng.integers(1, 6000, m), rng.integers(1000, 4000, m)


def _taxa(T, rng, nt, nn, holes=0.0, in_hier=1):
    """nt fresh taxids; at every rank they are dealt over nn fresh names, another deal at each
    rank, so each rank has exactly min(nt, nn) distinct names."""
    pools = [T.names(nn) for _ in range(8)]
    deal = [rng.permutation(nt) for _ in range(8)]
    out = []
    for i in range(nt):
        nm = [pools[r][deal[r][i] % nn] if rng.random() >= holes else -1 for r in range(8)]
        out.append(T.taxid(nm, in_hier))
    return out


def _targets(T, rng, tids, per=2, max_count=50):
    """`per` targets for every taxid, each with its own line count."""
    return {i: [T.target(i, int(rng.integers(1, max_count + 1))) for _ in range(per)] for i in tids}


def _row(T, rng, m, nt, nn, **kw):
    """m lines over exactly nt distinct taxids (all of them among the first lines when m allows,
    in shuffled order), random weights, no exact flag."""
    tids = _taxa(T, rng, nt, nn, **kw)
    tg = _targets(T, rng, tids)
    seq = [tids[i] for i in rng.permutation(nt)][:m] + [tids[int(i)] for i in rng.integers(0, nt, max(m - nt, 0))]
    bl, ql = _weights(rng, m)
    return [(tg[i][int(rng.integers(0, 2))], bl[k], ql[k], 0) for k, i in enumerate(seq)]


def _tie_row(T, rng, nn, tied, addends=None):
    """nn names at rank 0 in insertion order, one taxid and one line each (weights are small
    integers, exact in FP64); the entries in `tied` share the maximum.  Rank 1 holds one name."""
    n1 = T.name()
    lines = []
    for e, nm in enumerate(T.names(nn)):
        w = 1000 if e in tied else int(rng.integers(1, 1000))
        parts = addends.get(e, [w]) if addends else [w]
        for p in parts:   # several taxids of the same name: its weight is a sum
            lines.append((T.target(T.taxid([nm, n1]), 1), p, 1, 0))
    return lines


def _order_row(T, seed):
    """Weights from 2^0 to 2^71 over 150 taxids, three names per rank with holes: every sum of
    the walk has contributions in rounds 1, 2 and 3, and rounds at each addition."""
    rng = np.random.default_rng(seed)
    m, nt = 400, 150
    pools = [T.names(3) for _ in range(8)]
    tids = [T.taxid([pools[r][int(rng.integers(0, 3))] if (j + r) % 11 else -1 for r in range(8)]) for j in range(nt)]
    # most targets were hit by 2^24 .. 2^31 - 1 lines, one in five by a handful
    tg = {i: [T.target(i, int(rng.choice([1, 2, 1000])) if rng.random() < 0.2 else int(rng.integers(2 ** 24, 2 ** 31)))
              for _ in range(3)] for i in tids}
    seq = list(range(nt)) + rng.integers(0, nt, m - nt).tolist()
    for k in (0, 5, 70, 90, 140, *range(150, m, 8)):   # one key fed in every line round
        seq[k] = 0
    lines = []
    for j in seq:
        bits = int(rng.integers(36, 41)) if rng.random() < 0.8 else int(rng.integers(1, 12))
        blen = int(rng.integers(2 ** (bits - 1), 2 ** bits + 1))   # up to 2^40: full mantissas after the product
        qlen = int(rng.choice([1, 1, 3, 7]))
        lines.append((tg[tids[j]][int(rng.integers(0, 3))], blen, qlen, 0))
    return lines


ROW_LENGTHS = [0, 1, 63, 64, 65, 128, 129, 511, 512, 513, 1500]
# seeds at which every sum named in test_order_rows_depend_on_the_order_of_additions changes its
# bits when taken backwards (about one seed in ten does; found by running that test)
ORDER_SEEDS = [116, 141, 152, 154, 160, 176, 182, 185]
LEGACY_EXACT_AT = [0, 63, 64, 511]


def _build() -> Tables:
    T = Tables()
    rng = np.random.default_rng(2024)

    def filler():   # short ordinary rows between the cases: a batch of a few hundred rows
        for _ in range(3):
            m = int(rng.integers(0, 30))
            T.add(f"filler{len(T.rows)}", _row(T, rng, m, min(m, int(rng.integers(1, 6))), 3) if m else [])

    def add(case, lines):
        T.add(case, lines)
        filler()

    # row length and path selection
    for m in ROW_LENGTHS:
        add(f"len{m}", _row(T, rng, m, min(m, 37), 5) if m else [])
    base = _row(T, rng, LDS_LINES, 100, 7)
    add("switch512", base)
    add("switch513", base + [(-1, 10, 10, 0)])

    # distinct taxids and names
    for nt, m in ((1, 130), (2, 130), (64, 200), (65, 200), (200, 400), (512, 512)):
        add(f"nt{nt}", _row(T, rng, m, nt, 3))
    for nn, nt, m in ((1, 130, 200), (64, 130, 200), (65, 130, 200), (300, 400, 512)):
        add(f"nn{nn}", _row(T, rng, m, nt, nn))
    tids = _taxa(T, rng, 70, 4)
    tg = _targets(T, rng, tids)
    seq = tids[:64] + [tids[3], tids[3], tids[64], tids[65]] + tids[5:60] + [tids[64], tids[3]] + tids[66:70] + [tids[64]] * 3
    seq[4] = seq[40] = tids[3]   # one taxid three times inside round 1; tids[64] first seen in round 2, back in rounds 2 and 3
    bl, ql = _weights(rng, len(seq))
    add("late_and_repeated_taxids", [(tg[i][k % 2], bl[k], ql[k], 0) for k, i in enumerate(seq)])

    # partial lineages
    add("holes", _row(T, rng, 150, 40, 4, holes=0.3))
    lines = _row(T, rng, 150, 40, 4)
    for ln in lines:
        T.tax_names[T.t_tax[ln[0]], 3] = -1
    add("rank3_empty_everywhere", lines)
    lines = _row(T, rng, 100, 20, 3)
    bare = [T.target(T.taxid([], in_hier=1), 7), T.target(T.taxid([], in_hier=0), 7)]
    add("taxids_without_names", [(bare[0], 5000, 1000, 0)] + lines[:70] + [(bare[1], 900, 1000, 0), (bare[0], 10, 1000, 0)] + lines[70:])
    add("only_taxids_without_names", [(bare[0], 5000, 1000, 0), (bare[1], 900, 1000, 0)] * 40)

    # dictionary stress: keys whose home slots are 1020..1023 (chains wrap to slot 0), alone and
    # mixed with keys at home in the slots where the wrapped chain lands
    sn = iter(STRESS)
    ln_ = iter(LOW)
    st_names = [next(sn) for _ in range(300)]
    low_names = [next(ln_) for _ in range(60)]
    other = T.names(3)
    st_tax = [T.taxid([T.name(at=st_names[i % 300]), other[i % 3]], at=STRESS[i]) for i in range(330)]
    low_tax = [T.taxid([T.name(at=low_names[i % 60]), other[i % 3]], at=LOW[i]) for i in range(120)]
    tg = _targets(T, rng, st_tax + low_tax)
    for case, seq in (("dict_wrap", st_tax + [st_tax[int(i)] for i in rng.integers(0, 330, 100)]),
                      ("dict_wrap_into_occupied", [x for p in zip(low_tax, st_tax) for x in p] + st_tax[120:] + low_tax[:30]),
                      ("dict_wrap_seq_path", st_tax + low_tax + st_tax[::-1])):
        bl, ql = _weights(rng, len(seq))
        add(case, [(tg[i][k % 2], bl[k], ql[k], 0) for k, i in enumerate(seq)])

    # first-maximum ties between exactly equal weights
    add("tie_in_one_round", _tie_row(T, rng, 20, {5, 9}))
    add("tie_across_rounds", _tie_row(T, rng, 80, {3, 70}))
    add("tie_first_has_highest_lane", _tie_row(T, rng, 70, {63, 64, 65}))
    add("tie_of_sums", _tie_row(T, rng, 70, {2, 66}, addends={2: [300, 700], 66: [1, 999]}))
    add("tie_everywhere", _tie_row(T, rng, 130, set(range(130))))

    # order-sensitive sums
    for s in ORDER_SEEDS:
        add(f"order{s}", _order_row(T, s))

    # degenerate weights
    tids = _taxa(T, rng, 6, 2)
    t1 = {i: T.target(i, 3) for i in tids}
    t0 = {i: T.target(i, 0) for i in tids}      # targets that no PAF line counted
    none = T.target(-1, 9)                      # a target without a taxid
    n = len(tids)
    add("qlen0_some", [(t1[tids[k % n]], 100 + k, 0 if k % 3 == 0 else 500, 0) for k in range(40)])
    add("qlen0_all", [(t1[tids[k % n]], 100 + k, 0, 0) for k in range(40)])
    add("blen0_some", [(t1[tids[k % n]], 0 if k % 2 else 77 + k, 500, 0) for k in range(70)])
    add("blen0_all", [(t1[tids[k % n]], 0, 500, 0) for k in range(70)])
    add("refcount0_some", [((t0 if k % 4 else t1)[tids[k % n]], 100 + k, 500, 0) for k in range(70)])
    add("refcount0_all", [(t0[tids[k % n]], 100 + k, 500, 0) for k in range(70)])
    add("no_target_some", [(-1 if k % 3 == 1 else t1[tids[k % n]], 100 + k, 500, 0) for k in range(70)])
    add("no_target_all", [(-1, 100 + k, 500, 0) for k in range(70)])
    add("no_taxid_some", [(none if k % 3 == 1 else t1[tids[k % n]], 100 + k, 500, 0) for k in range(70)])
    add("no_taxid_all", [(none, 100 + k, 500, 1) for k in range(70)])
    add("no_taxid_all_long", [(none if k % 2 else -1, 100 + k, 500, k % 2) for k in range(600)])

    # legacy exact-match shortcut
    for p in LEGACY_EXACT_AT:
        lines = _row(T, rng, 512 if p == 511 else 200, 30, 3)
        lines[p] = lines[p][:3] + (1,)
        add(f"exact_at{p}", lines)
    lines = _row(T, rng, 700, 30, 3)
    lines[650] = lines[650][:3] + (1,)
    add("exact_at650_seq_path", lines)
    lines = _row(T, rng, 150, 20, 3)
    lines[10] = (none, 500, 500, 1)             # exact, but the target has no taxid: not a candidate
    lines[20] = (-1, 500, 500, 1)
    lines[90] = lines[90][:3] + (1,)            # the first exact line with a taxid: round 2
    lines[120] = lines[120][:3] + (1,)
    add("exact_first_has_no_taxid", lines)
    for case, m, at in (("exact_not_in_hierarchy", 150, (30, 100)), ("exact_not_in_hierarchy_seq_path", 600, (30, 560))):
        lines = _row(T, rng, m, 20, 3)
        outside = T.target(T.taxid(T.names(8), in_hier=0), 4)
        lines[at[0]] = (outside, 500, 500, 1)   # only this one is tried; the row falls through
        lines[at[1]] = lines[at[1]][:3] + (1,)  # in the hierarchy and exact, yet ignored
        add(case, lines)
    tids = _taxa(T, rng, 30, 3)
    for i in tids[::3]:
        T.in_hier[i] = 0                        # left out of the lineages, still counted in `total`
    tg = _targets(T, rng, tids)
    bl, ql = _weights(rng, 150)
    add("some_taxids_outside_hierarchy", [(tg[tids[int(rng.integers(0, 30))]][k % 2], bl[k], ql[k], 0) for k in range(150)])
    tids = _taxa(T, rng, 10, 3, in_hier=0)
    tg = _targets(T, rng, tids)
    add("all_taxids_outside_hierarchy", [(tg[tids[k % 10]][0], 100 + k, 500, 0) for k in range(80)])
    return T


T = _build()
S = T.strings()
CASES = [c for c, _ in T.rows if not c.startswith("filler")]
_expected = {}


def expected(mode):
    """Oracle results of every row, computed once per mode and left unchanged."""
    if mode not in _expected:
        _expected[mode] = [expect(T, S, lines, mode) for _, lines in T.rows]
    return _expected[mode]


# ------------------------------------------------------------ CPU checks of the cases themselves
def _chunk_reversed(v):
    return [x for k in range(0, len(v), ROUND) for x in reversed(v[k:k + ROUND])]


def _sum(v):
    acc = 0.0
    for x in v:
        acc += x
    return acc


@pytest.mark.parametrize("seed", ORDER_SEEDS)
def test_order_rows_depend_on_the_order_of_additions(seed):
    """Precondition of the order-sensitive cases (no GPU): for the key fed in several rounds, the
    line total, the taxid total and the rank-0 denominator and name weights, adding the same
    contributions backwards -- over the whole list, or inside each group of 64 -- gives another
    bit pattern, and the confidences of the row change with it."""
    lines = T.rows[T.index[f"order{seed}"]][1]
    w = [(blen / qlen) * T.counts[t] for t, blen, qlen, _ in lines]
    tid = [T.t_tax[t] for t, *_ in lines]
    assert len(set(tid)) > 2 * ROUND and len(lines) > 2 * ROUND
    assert min(w) < 2.0 ** 3 and max(w) > 2.0 ** 60
    key = tid[0]
    at = [k for k, i in enumerate(tid) if i == key]
    assert {0, 1, 2} <= {k // ROUND for k in at}   # contributions in rounds 1, 2 and 3
    tw = defaultdict(float)
    for i, x in zip(tid, w):
        tw[i] += x
    order = list(tw)
    r0 = [T.tax_names[i, 0] for i in order]
    sums = {"key": [x for i, x in zip(tid, w) if i == key], "total": w, "tot": [tw[i] for i in order],
            "denom": [tw[i] for i, nm in zip(order, r0) if nm >= 0]}
    for nm in sorted(set(r0) - {-1}):
        js = [j for j, x in enumerate(r0) if x == nm]
        assert js[0] < ROUND and any(ROUND <= j < 2 * ROUND for j in js) and js[-1] >= 2 * ROUND
        sums[f"name{nm}"] = [tw[order[j]] for j in js]
    for what, v in sums.items():
        assert _bits(_sum(v)) != _bits(_sum(v[::-1])), what
    for what in ("total", "tot", "denom"):
        assert _bits(_sum(sums[what])) != _bits(_sum(_chunk_reversed(sums[what]))), what
    # the per-key sums inside each group of 64 candidates, as one number: the row's confidence
    for mode in (0, 1):
        fwd = expect(T, S, lines, mode)
        back = expect(T, S, lines[::-1], mode)
        assert fwd[0] == 8 and fwd[3] != back[3]


def test_cases_are_what_they_claim():
    """No GPU: the oracle's verdicts on the constructed rows show that each case reaches the
    path it is named after (a tie really is a tie and the first name wins, the shortcut is or
    is not taken, a zero total is Unknown, ...)."""
    e0, e1 = expected(0), expected(1)
    ix = T.index
    assert 200 <= len(T.rows) <= 400
    assert [len(T.rows[ix[f"len{m}"]][1]) for m in ROW_LENGTHS] == ROW_LENGTHS
    for e in (e0, e1):
        assert e[ix["switch512"]] == e[ix["switch513"]] and e[ix["switch512"]][0] == 8
        assert e[ix["rank3_empty_everywhere"]][0] == 3
        assert e[ix["only_taxids_without_names"]] == (0, (), -1, 0)
        for c in ("qlen0_all", "blen0_all", "refcount0_all", "no_target_all", "no_taxid_all", "no_taxid_all_long", "len0"):
            assert e[ix[c]] == (0, (), -1, 0), c
        for c in ("qlen0_some", "blen0_some", "refcount0_some", "no_target_some", "no_taxid_some", "holes", "dict_wrap"):
            assert e[ix[c]][0] > 0, c
    for nt in (1, 2, 64, 65, 200, 512):
        lines = T.rows[ix[f"nt{nt}"]][1]
        assert len({T.t_tax[t] for t, *_ in lines}) == nt
    for nn in (1, 64, 65, 300):
        lines = T.rows[ix[f"nn{nn}"]][1]
        assert all(len({T.tax_names[T.t_tax[t], r] for t, *_ in lines}) == nn for r in range(8))
    for c in ("dict_wrap", "dict_wrap_into_occupied", "dict_wrap_seq_path"):
        tids = {T.t_tax[t] for t, *_ in T.rows[ix[c]][1]}
        nms = {int(T.tax_names[i, 0]) for i in tids}
        assert len(tids & set(STRESS)) >= 300 and len(nms & set(STRESS)) >= 300
        assert len(T.rows[ix[c]][1]) > LDS_LINES if c.endswith("seq_path") else len(T.rows[ix[c]][1]) <= LDS_LINES
    # ties: the winner is the first-inserted name of the tied ones, which a maximum that
    # prefers later entries would not return
    for c, tied in (("tie_in_one_round", (5, 9)), ("tie_across_rounds", (3, 70)), ("tie_first_has_highest_lane", (63, 64, 65)),
                    ("tie_of_sums", (2, 66)), ("tie_everywhere", tuple(range(130)))):
        lines = T.rows[ix[c]][1]
        order = list(dict.fromkeys(int(T.tax_names[T.t_tax[t], 0]) for t, *_ in lines))
        wsum = defaultdict(int)
        for t, blen, _, _ in lines:
            wsum[int(T.tax_names[T.t_tax[t], 0])] += blen
        best = max(wsum.values())
        assert tuple(k for k, nm in enumerate(order) if wsum[nm] == best) == tied
        for e in (e0, e1):
            assert e[ix[c]][0] == 2 and e[ix[c]][1][0] == order[tied[0]], c
    # legacy shortcut
    for p in LEGACY_EXACT_AT:
        lines = T.rows[ix[f"exact_at{p}"]][1]
        assert [k for k, ln in enumerate(lines) if ln[3]] == [p]
        assert e1[ix[f"exact_at{p}"]][:3] == (-1, (), T.t_tax[lines[p][0]]) and e0[ix[f"exact_at{p}"]][0] == 8
    lines = T.rows[ix["exact_at650_seq_path"]][1]
    assert e1[ix["exact_at650_seq_path"]][:3] == (-1, (), T.t_tax[lines[650][0]])
    lines = T.rows[ix["exact_first_has_no_taxid"]][1]
    assert e1[ix["exact_first_has_no_taxid"]][:3] == (-1, (), T.t_tax[lines[90][0]])
    for c in ("exact_not_in_hierarchy", "exact_not_in_hierarchy_seq_path"):
        assert e1[ix[c]][0] == 8 and e1[ix[c]][2] == -1
    assert e1[ix["some_taxids_outside_hierarchy"]][0] == 8 and e1[ix["some_taxids_outside_hierarchy"]][3] < _bits(0.5)
    assert e1[ix["all_taxids_outside_hierarchy"]] == (0, (), -1, 0) and e0[ix["all_taxids_outside_hierarchy"]][0] == 8


# ------------------------------------------------------------------------------ the GPU side
def _vp(t):
    return ctypes.c_void_p(t.data_ptr())


@pytest.fixture(scope="module")
def device_tables(gpu):
    torch = gpu.torch
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(gpu.dev) for k, v in T.arrays().items()}


@pytest.fixture(scope="module")
def gpu_results(gpu, device_tables):
    """Both modes, each as one launch over the whole batch, as Classifier.run calls hymet_lca;
    the outputs start from values the kernel never writes."""
    torch = gpu.torch
    d = device_tables
    nq, nl = len(T.rows), int(d["line_t"].numel())
    out = {}
    for mode in (0, 1):
        s_tid = gpu.empty(nl, torch.int32)
        s_w = gpu.empty(nl, torch.float64)
        s_nm = gpu.empty(nl, torch.int32)
        s_nw = gpu.empty(nl, torch.float64)
        o_depth = torch.full((nq,), 99, dtype=torch.int32, device=gpu.dev)
        o_names = torch.full((nq * 8,), -99, dtype=torch.int32, device=gpu.dev)
        o_conf = torch.full((nq,), -99.0, dtype=torch.float64, device=gpu.dev)
        o_tax = torch.full((nq,), 99, dtype=torch.int32, device=gpu.dev)
        gpu.call("hymet_lca", mode, nq, _vp(d["q_off"]), _vp(d["line_t"]), _vp(d["line_blen"]), _vp(d["line_qlen"]),
                 _vp(d["line_exact"]), _vp(d["ref_counts"]), _vp(d["t_tax"]), _vp(d["tax_names"]), _vp(d["tax_in_hier"]),
                 _vp(s_tid), _vp(s_w), _vp(s_nm), _vp(s_nw), _vp(o_depth), _vp(o_names), _vp(o_conf), _vp(o_tax))
        gpu.sync()
        out[mode] = (o_depth.cpu().numpy(), o_names.cpu().numpy().reshape(nq, 8), o_tax.cpu().numpy(),
                     o_conf.cpu().numpy().view(np.uint64))
    return out


def _got(res, q):
    depth, names, tax, conf = res
    d = int(depth[q])
    return d, tuple(names[q, :max(d, 0)].tolist()), int(tax[q]), int(conf[q])


@needs_gpu
@pytest.mark.parametrize("mode", [0, 1], ids=["cami", "legacy"])
@pytest.mark.parametrize("case", CASES)
def test_lca_row(gpu_results, case, mode):
    q = T.index[case]
    got, want = _got(gpu_results[mode], q), expected(mode)[q]
    assert got == want, (f"{case}: depth, names, shortcut taxid, confidence bits = {got[:3]} {got[3]:#018x}, "
                         f"oracle {want[:3]} {want[3]:#018x}")


@needs_gpu
@pytest.mark.parametrize("mode", [0, 1], ids=["cami", "legacy"])
def test_lca_filler_rows(gpu_results, mode):
    """The short ordinary rows launched between the cases."""
    want = expected(mode)
    bad = [c for q, (c, _) in enumerate(T.rows) if c.startswith("filler") and _got(gpu_results[mode], q) != want[q]]
    assert not bad


@needs_gpu
@pytest.mark.parametrize("mode", [0, 1], ids=["cami", "legacy"])
def test_lca_same_result_on_both_sides_of_the_switch(gpu_results, mode):
    """512 lines run in LDS, the same lines plus one without a target run in lca_row_seq."""
    a, b = (_got(gpu_results[mode], T.index[c]) for c in ("switch512", "switch513"))
    assert a == b and a[0] == 8


@needs_gpu
@pytest.mark.parametrize("n", [1, 255, 256, 257, 100_003])
def test_ref_counts_match_bincount(gpu, n):
    """Per-target line counts: -1 entries are skipped, and half of all lines hit one target."""
    torch = gpu.torch
    rng = np.random.default_rng(n)
    n_t = 300
    line_t = rng.integers(-1, n_t, n).astype(np.int32)
    line_t[line_t == 17] = 18
    line_t[::7] = -1
    line_t[1::2] = 17     # every second line: the atomics contend on one counter
    if n == 1:
        line_t[0] = 17
    d_t = torch.from_numpy(line_t).to(gpu.dev)
    counts = gpu.zeros(n_t + 8, torch.int32)
    gpu.call("hymet_lca_ref_counts", _vp(d_t), n, _vp(counts))
    gpu.sync()
    want = np.bincount(line_t[line_t >= 0], minlength=n_t + 8)
    assert want[17] == max(n // 2, 1) and (n == 1 or (line_t == -1).any())
    np.testing.assert_array_equal(counts.cpu().numpy(), want)
