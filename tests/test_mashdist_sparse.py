"""Host side of the sparse dist path: cmin, the reference counters on a hand-written case, and
the --sparse flag of `cli dist` / `cli derep` (no GPU)."""
import numpy as np
import pytest

from tests import _sparse_ref as ref


@pytest.mark.parametrize("s", [1, 64, 1000])
@pytest.mark.parametrize("max_dist", [0.0, 0.05, 0.3, 0.999])
def test_candidate_min_common_is_at_least_one(s, max_dist):
    from hymet_amd import mashdist as md
    t = md.min_common_table(s, 21, max_dist)
    cmin = md.candidate_min_common(t)
    assert cmin >= 1
    assert cmin == min(int(x) for x in t[1:])
    # no pair with fewer shared hashes passes at any denom >= 1
    assert all(int(t[d]) >= cmin for d in range(1, s + 1))
    if max_dist == 0.0:
        assert cmin == 1 and int(t[s]) == s            # only identical lists: common == denom


def test_candidate_min_common_needs_a_denominator():
    from hymet_amd import mashdist as md
    with pytest.raises(ValueError):
        md.candidate_min_common(np.zeros(1, np.uint16))


A, B, C = [1, 2, 3, 4], [2, 3, 9], [3, 4, 10]


def test_reference_counters_three_sketches_tri():
    lists, s = [A, B, C], 3                            # A counts as [1, 2, 3]
    assert ref.postings(lists, None, s, 0, 3) == 9
    assert ref.shared(lists, None, s, 0, 3) == {(1, 0): 2, (2, 0): 1, (2, 1): 1}
    assert ref.emitted(lists, None, s, 0, 3) == 4
    assert ref.candidates(lists, None, s, 0, 3, 1) == 3
    assert ref.candidates(lists, None, s, 0, 3, 2) == 1
    assert ref.empty_pairs(lists, None, s, 0, 3) == set()
    # rows [2, 3): every sketch below 3 still has postings; only q = 2 emits
    assert ref.postings(lists, None, s, 2, 3) == 9 and ref.emitted(lists, None, s, 2, 3) == 2
    # rows [0, 2): sketch 2 has none
    assert ref.postings(lists, None, s, 0, 2) == 6 and ref.emitted(lists, None, s, 0, 2) == 2
    # untruncated, 4 is shared by A and C as well
    assert ref.shared(lists, None, 4, 0, 3)[(2, 0)] == 2
    # two empty sketches and a third: the pairs r < q among them
    assert ref.empty_pairs([[], A, [], []], None, s, 0, 4) == {(2, 0), (3, 0), (3, 2)}
    assert ref.empty_pairs([[], A, [], []], None, s, 3, 4) == {(3, 0), (3, 2)}
    assert ref.candidates([[], A, [], []], None, s, 0, 4, 1) == 3


def test_reference_counters_three_sketches_dist():
    refs, qrys, s = [A, B, []], [C, []], 3
    assert ref.postings(refs, qrys, s, 0, 2) == 9
    assert ref.shared(refs, qrys, s, 0, 2) == {(0, 0): 1, (0, 1): 1}
    assert ref.emitted(refs, qrys, s, 0, 2) == 2
    assert ref.empty_pairs(refs, qrys, s, 0, 2) == {(1, 2)}
    assert ref.candidates(refs, qrys, s, 0, 2, 1) == 3
    assert ref.candidates(refs, qrys, s, 0, 2, 2) == 1
    assert ref.postings(refs, qrys, s, 1, 2) == 6 and ref.emitted(refs, qrys, s, 1, 2) == 0
    assert ref.candidates(refs, qrys, s, 1, 2, 1) == 1


def test_cli_dist_sparse_arguments(capsys):
    from hymet_amd import cli
    a = cli.dist_args(["--sparse", "-d", "0.05", "ref.msh", "q.msh"])
    assert a.sparse and a.max_dist == 0.05 and not a.table
    a = cli.dist_args(["-d", "0.05", "ref.msh", "q.msh"])
    assert not a.sparse and a.max_dist == 0.05
    a = cli.dist_args(["ref.msh", "q.msh"])
    assert not a.sparse and a.max_dist == 1.0          # the default is unchanged
    assert "--sparse" in cli.DIST_USAGE
    for bad, word in ((["--sparse", "-t", "-d", "0.05", "ref.msh", "q.msh"], "-t"),
                      (["--sparse", "-d", "1", "ref.msh", "q.msh"], "below 1"),
                      (["--sparse", "-d", "1.5", "ref.msh", "q.msh"], "below 1"),
                      (["--sparse", "ref.msh", "q.msh"], "-d")):
        assert cli.dist_args(bad) is None, bad
        err = capsys.readouterr().err.splitlines()
        assert err[-1] == cli.DIST_USAGE and "--sparse" in err[0] and word in err[0], bad
        assert cli.main(["dist", *bad]) == 2           # refused before anything is loaded
        capsys.readouterr()


def test_cli_derep_sparse_arguments(capsys):
    from hymet_amd import cli
    a = cli.derep_args(["--sparse", "a.msh"])
    assert a.sparse and a.max_dist == 0.05
    assert not cli.derep_args(["a.msh"]).sparse
    assert "--sparse" in cli.DEREP_USAGE
    assert cli.derep_args(["--sparse", "-d", "1", "a.msh"]) is None
    err = capsys.readouterr().err.splitlines()
    assert err[-1] == cli.DEREP_USAGE and "-d" in err[0]


def test_sparse_blocks_refuses_a_threshold_of_one():
    from hymet_amd import mashdist as md
    with pytest.raises(ValueError):
        next(md.sparse_blocks(None, None, None, 1.0))
    with pytest.raises(ValueError):
        next(md.dist_blocks(None, None, None, 1.0, sparse=True))


def test_sparse_ranges_policy():
    """The whole range first; an overflow halves it; a range within the dense block falls back."""
    from hymet_amd import mashdist as md
    tried = []

    def attempt(q0, q1):
        tried.append((q0, q1))
        return None if (q1 - q0 > 4 or q0 == 4) else ("ok", q0, q1)

    got = list(md.sparse_ranges(16, 2, attempt))
    assert tried[0] == (0, 16)
    assert [g[1:3] for g in got] == sorted(g[1:3] for g in got)           # ascending
    assert got[0][1] == 0 and got[-1][2] == 16
    assert all(a[2] == b[1] for a, b in zip(got, got[1:]))                # no gap, no overlap
    assert [g[:3] for g in got] == [("sparse", 0, 4), ("dense", 4, 6), ("sparse", 6, 8), ("sparse", 8, 12),
                                    ("sparse", 12, 16)]
    assert list(md.sparse_ranges(0, 2, attempt)) == []
