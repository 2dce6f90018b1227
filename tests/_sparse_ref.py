"""The counters of the sparse dist path (hymet_mash_dist_sparse) restated from the hash lists in
plain Python and numpy: no GPU, no library.  A list counts with its first min(len, s) entries.

dist mode: references and the queries of the row range [q0, q1).  tri mode (qrys is None): one
DB against itself, the pairs r < q with q in [q0, q1); only the sketches below q1 have postings.

shared() is the costly part; the other functions take a table it made for a wider row range
through `sh` and restrict it themselves.
"""
import numpy as np


def _cut(lists, s):
    return [[int(x) for x in np.asarray(a, np.uint64).tolist()[:s]] for a in lists]


def _lens(lists, s):
    return [min(len(a), s) for a in lists]


def postings(refs, qrys, s, q0, q1):
    """(hash, sketch) entries the call sorts."""
    if qrys is None:
        return sum(_lens(refs, s)[:q1])
    return sum(_lens(refs, s)) + sum(_lens(qrys, s)[q0:q1])


def shared(refs, qrys, s, q0, q1):
    """{(q, r): hashes the two truncated lists share} over the pairs that share any."""
    R = _cut(refs, s)
    Q = R if qrys is None else _cut(qrys, s)
    holders = {}
    for r, a in enumerate(R):
        for h in a:
            holders.setdefault(h, []).append(r)
    out = {}
    for q in range(q0, q1):
        hit = [holders[h] for h in Q[q] if h in holders]
        if not hit:
            continue
        n = np.bincount(np.concatenate([np.asarray(x, np.int64) for x in hit]), minlength=len(R))
        for r in np.nonzero(n)[0].tolist():
            if qrys is not None or r < q:
                out[(q, r)] = int(n[r])
    return out


def _rows(sh, q0, q1):
    return {k: v for k, v in sh.items() if q0 <= k[0] < q1}


def emitted(refs, qrys, s, q0, q1, sh=None):
    """Pair keys: one per shared hash of a pair."""
    return sum(_rows(shared(refs, qrys, s, q0, q1) if sh is None else sh, q0, q1).values())


def empty_pairs(refs, qrys, s, q0, q1):
    """The (q, r) pairs of two empty sketches, which share nothing and still pass (denom 0)."""
    R = _lens(refs, s)
    Q = R if qrys is None else _lens(qrys, s)
    none = [r for r, n in enumerate(R) if n == 0]
    return {(q, r) for q in range(q0, q1) if Q[q] == 0 for r in none if qrys is not None or r < q}


def candidates(refs, qrys, s, q0, q1, cmin, sh=None):
    """Pairs that go to the exact routine: cmin or more shared hashes, or two empty sketches."""
    sh = _rows(shared(refs, qrys, s, q0, q1) if sh is None else sh, q0, q1)
    return sum(1 for v in sh.values() if v >= cmin) + len(empty_pairs(refs, qrys, s, q0, q1))
