"""Plain-Python restatement of winner-take-all screening (`mash screen -w`, Mash 2.x
CommandScreen.cpp), the reference of tests/test_screen_winner*.py.  Nothing here imports the
product.

Every key (sketch hash) found in the pool is credited to one of the references holding it: the
one with the highest first-pass identity, then the longest genome, then the smallest index
(Mash leaves the last tie to its hash set's iteration order; the project fixes it).  shared and
median are then recounted from the credited keys only."""
import math


def winner_ref(offsets, hashes, lengths, counts, k):
    """offsets: CSR of the references into hashes (each reference's hashes distinct);
    lengths: genome length per reference (taken as all 0 unless there is one per reference);
    counts: mapping key -> occurrences in the pool (a missing key counts 0); k: k-mer size.
    Returns (shared, shared_w, median_w), three lists of ints."""
    n = len(offsets) - 1
    lengths = [int(x) for x in lengths] if lengths is not None and len(lengths) == n else [0] * n
    refs = [[int(h) for h in hashes[int(offsets[r]):int(offsets[r + 1])]] for r in range(n)]
    shared = [sum(1 for h in hs if counts.get(h, 0) > 0) for hs in refs]
    score = []
    for r in range(n):
        ln = len(refs[r])
        score.append(1.0 if shared[r] == ln else math.pow(shared[r] / ln, 1.0 / k))
    holders = {}
    for r in range(n):                      # ascending reference index
        for h in refs[r]:
            holders.setdefault(h, []).append(r)
    credited = [[] for _ in range(n)]
    for h, rs in holders.items():
        c = counts.get(h, 0)
        if c <= 0:
            continue
        best = rs[0]
        for r in rs[1:]:
            if score[r] > score[best] or (score[r] == score[best] and lengths[r] > lengths[best]):
                best = r
        credited[best].append(c)
    shared_w = [len(c) for c in credited]
    median_w = [sorted(c)[len(c) // 2] if c else 0 for c in credited]
    return shared, shared_w, median_w
