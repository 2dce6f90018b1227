"""The order of `dist --top K` restated in plain Python (include/hymet_gpu.h at
hymet_mash_dist_topk; DESIGN.md §3 "Nearest (top-K)"), on exact rationals.

An entry is (common, denom).  Nearest first: by common / denom as an exact fraction, descending,
0 / 0 counting as 1; equal fractions by reference index, ascending.  An entry competes when
denom <= s, common <= denom and, with a min-common table, common >= table[denom].

Nothing here uses the device's rank formula: the formula is what the tests pin against this.
"""
from fractions import Fraction


def fraction(common, denom):
    common, denom = int(common), int(denom)
    return Fraction(1) if denom == 0 else Fraction(common, denom)


def competes(common, denom, s, table=None):
    common, denom = int(common), int(denom)
    return denom <= s and common <= denom and (table is None or common >= int(table[denom]))


def order(common, denom, s, table=None, index=None):
    """The positions of one row's competing entries, nearest first.  index: the reference index
    of each position (a CSR row; ascending), the position itself when None."""
    pos = [p for p in range(len(common)) if competes(common[p], denom[p], s, table)]
    ref = (lambda p: p) if index is None else (lambda p: int(index[p]))
    return sorted(pos, key=lambda p: (-fraction(common[p], denom[p]), ref(p)))


def topk_dense(common, denom, K, s, table=None):
    """Per row of the dense (rows x n_ref) arrays: the reference indices of its K nearest."""
    return [order(c, d, s, table)[:K] for c, d in zip(common, denom)]


def topk_csr(row_off, ref_idx, common, denom, K, s):
    """Per row of a CSR: the (reference index, entry position in the arrays) of its K nearest."""
    out = []
    for r in range(len(row_off) - 1):
        a, b = int(row_off[r]), int(row_off[r + 1])
        o = order(common[a:b], denom[a:b], s, None, ref_idx[a:b])[:K]
        out.append([(int(ref_idx[a + p]), a + p) for p in o])
    return out
