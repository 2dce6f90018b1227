"""Greedy dereplication by the sequential walk its definition gives (DESIGN.md §3 "Greedy
derep"): the reference of the device selection (hymet_mash_greedy / hymet_mash_greedy_edges).
The sketches are numbered in priority order; `pairs` maps (q, r), r < q, of every passing pair
to its (common, denom).  The order of "nearest" is the exact rational, by fractions.Fraction."""
from fractions import Fraction

import numpy as np


def nearness(common, denom):
    """common / denom as an exact rational; 0 / 0 counts as 1."""
    return Fraction(1) if denom == 0 else Fraction(int(common), int(denom))


def below(pairs):
    """{q: [(r, common, denom), ...]} with r ascending, from the pair dict."""
    rows = {}
    for (q, r), (c, d) in pairs.items():
        assert r < q, "a pair is keyed (q, r) with r < q"
        rows.setdefault(q, []).append((r, c, d))
    for v in rows.values():
        v.sort()
    return rows


def greedy(n, pairs):
    """int32 [n]: rep[i] == i for a representative, else the nearest of the representatives that
    precede i and pass with it; equal rationals go to the earlier one."""
    rows = below(pairs)
    rep = np.full(n, -1, np.int32)
    for q in range(n):
        best = None
        for r, c, d in rows.get(q, ()):
            if rep[r] != r:
                continue
            key = (-nearness(c, d), r)
            if best is None or key < best[0]:
                best = (key, r)
        rep[q] = q if best is None else best[1]
    return rep


def first_passing(n, pairs):
    """What a walk without the nearest rule gives: a member goes to the first preceding
    representative that passes with it."""
    rows = below(pairs)
    rep = np.full(n, -1, np.int32)
    for q in range(n):
        rep[q] = next((r for r, _, _ in rows.get(q, ()) if rep[r] == r), q)
    return rep


def has_tie(n, pairs, rep):
    """True when some member's nearest preceding representatives include two of one rational."""
    rows = below(pairs)
    for q in range(n):
        if rep[q] == q:
            continue
        cand = [nearness(c, d) for r, c, d in rows.get(q, ()) if rep[r] == r]
        if cand.count(max(cand)) > 1:
            return True
    return False


def check_members_pass(rep, pairs):
    """Every member passes with its representative, which precedes it and is one."""
    rep = np.asarray(rep)
    for i, r in enumerate(rep.tolist()):
        assert 0 <= r <= i, f"rep[{i}] = {r}"
        assert rep[r] == r, f"rep[{i}] = {r}, which is a member itself"
        assert r == i or (i, r) in pairs, f"member {i} does not pass with its representative {r}"


def check_representatives_apart(rep, pairs):
    """No two representatives pass with each other."""
    rep = np.asarray(rep)
    for (q, r) in pairs:
        assert not (rep[q] == q and rep[r] == r), f"representatives {r} and {q} pass with each other"
