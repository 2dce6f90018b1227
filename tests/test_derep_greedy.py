"""Host side of the greedy dereplication (hymet_amd/derep.py cluster_greedy's helpers,
`cli derep --greedy`) and its reference walk (tests/_greedy_ref.py): no GPU."""
import numpy as np
import pytest

from tests import _greedy_ref as gr
from tests._cc_ref import labels as cc_labels
from tests.test_derep import make_db

K = 21


# ------------------------------------------------------------------ the reference, by hand
def test_reference_path():
    pairs = {(1, 0): (5, 10), (2, 1): (5, 10)}
    rep = gr.greedy(3, pairs)
    np.testing.assert_array_equal(rep, [0, 0, 2])          # 2's only neighbour is a member
    gr.check_members_pass(rep, pairs)
    gr.check_representatives_apart(rep, pairs)
    np.testing.assert_array_equal(cc_labels(3, pairs), [0, 0, 0])      # single linkage chains them


def test_reference_equal_rationals_go_to_the_earlier():
    pairs = {(2, 0): (500, 1000), (2, 1): (1, 2)}
    np.testing.assert_array_equal(gr.greedy(3, pairs), [0, 1, 0])
    pairs = {(2, 0): (1, 2), (2, 1): (500, 1000)}
    np.testing.assert_array_equal(gr.greedy(3, pairs), [0, 1, 0])
    assert gr.has_tie(3, pairs, gr.greedy(3, pairs))
    pairs = {(2, 0): (499, 1000), (2, 1): (1, 2)}          # the nearer one, not the first
    np.testing.assert_array_equal(gr.greedy(3, pairs), [0, 1, 1])
    np.testing.assert_array_equal(gr.first_passing(3, pairs), [0, 1, 0])
    assert not gr.has_tie(3, pairs, gr.greedy(3, pairs))


def test_reference_zero_over_zero_is_nearest():
    pairs = {(2, 0): (999, 1000), (2, 1): (0, 0)}
    np.testing.assert_array_equal(gr.greedy(3, pairs), [0, 1, 1])
    pairs = {(2, 0): (0, 0), (2, 1): (7, 7)}               # 0 / 0 counts as 1: a tie, to the earlier
    np.testing.assert_array_equal(gr.greedy(3, pairs), [0, 1, 0])


def test_reference_checkers_refuse_what_they_should():
    pairs = {(1, 0): (5, 10), (2, 1): (5, 10)}
    with pytest.raises(AssertionError):
        gr.check_members_pass([0, 0, 0], pairs)            # 2 does not pass with 0
    with pytest.raises(AssertionError):
        gr.check_members_pass([0, 0, 1], pairs)            # 1 is a member itself
    with pytest.raises(AssertionError):
        gr.check_representatives_apart([0, 1, 2], pairs)
    gr.check_representatives_apart([0, 0, 2], pairs)


# ------------------------------------------------------------------ host helpers of cluster_greedy
def test_permute_db_round_trip():
    from hymet_amd import derep as dr
    rng = np.random.default_rng(3)
    lists = [np.sort(rng.choice(2 ** 40, size=L, replace=False)).astype(np.uint64) for L in (8, 0, 5, 8, 1, 8)]
    db = make_db(lists, 8, lengths=[10, 0, 30, 2 ** 33, 50, 60])
    order = np.array([3, 5, 4, 2, 0, 1])
    p = dr.permute_db(db, order)
    assert p.names == [f"g{i}" for i in order] and p.comments == [f"c{i}" for i in order]
    np.testing.assert_array_equal(p.lengths, [2 ** 33, 60, 50, 30, 10, 0])
    np.testing.assert_array_equal(p.offsets, [0, 8, 16, 17, 22, 30, 30])
    for n, i in enumerate(order):
        np.testing.assert_array_equal(np.asarray(p.ref_hashes(n), np.uint64), lists[i])
    assert (p.k, p.seed, p.sketch_size) == (db.k, db.seed, db.sketch_size)
    back = dr.permute_db(p, np.argsort(order))
    assert back.names == db.names and back.comments == db.comments
    np.testing.assert_array_equal(back.offsets, db.offsets)
    np.testing.assert_array_equal(back.hashes, db.hashes)
    np.testing.assert_array_equal(back.lengths, db.lengths)
    assert dr.permute_db(make_db([], 8), []).n_refs == 0
    for bad in ([0, 1, 2], [0, 0, 1, 2, 3, 4], [1, 2, 3, 4, 5, 6]):
        with pytest.raises(ValueError):
            dr.permute_db(db, bad)


def test_priority_order_rules_and_equal_lengths():
    from hymet_amd import derep as dr
    lengths = [5, 9, 7, 9, 1, 7, 2]
    np.testing.assert_array_equal(dr.priority_order(lengths, 7), [1, 3, 2, 5, 0, 6, 4])
    np.testing.assert_array_equal(dr.priority_order(lengths, 7, "longest"), [1, 3, 2, 5, 0, 6, 4])
    np.testing.assert_array_equal(dr.priority_order(lengths, 7, "first"), np.arange(7))
    np.testing.assert_array_equal(dr.priority_order([4] * 5, 5), np.arange(5))     # all equal: DB order
    np.testing.assert_array_equal(dr.priority_order([], 0), [])
    with pytest.raises(ValueError):
        dr.priority_order(lengths, 7, "median")


def test_derep_args_accept_greedy(capsys):
    from hymet_amd import cli
    a = cli.derep_args(["--greedy", "a.msh"])
    assert a.greedy and not a.sparse and a.rule == "longest" and a.files == ["a.msh"]
    a = cli.derep_args(["--greedy", "--sparse", "-r", "first", "-d", "0.1", "-o", "out", "a.msh"])
    assert a.greedy and a.sparse and (a.rule, a.max_dist, a.out) == ("first", 0.1, "out")
    assert not cli.derep_args(["a.msh"]).greedy
    assert "--greedy" in cli.DEREP_USAGE and "--greedy" in cli.cmd_derep.__doc__ and "--greedy" in cli.__doc__
    assert cli.main(["derep", "--greed", "a.msh"]) == 2    # no abbreviations
    assert capsys.readouterr().err.splitlines()[-1] == cli.DEREP_USAGE


def test_rows_and_subset_follow_from_rep():
    from hymet_amd import derep as dr
    db = make_db([[i + 1] for i in range(7)], 1)
    #      0  1  2  3  4  5  6
    rep = [3, 1, 3, 3, 4, 1, 6]
    np.testing.assert_array_equal(dr.greedy_labels(rep), [0, 1, 0, 0, 4, 1, 6])
    reps = dr.greedy_representatives(rep)
    np.testing.assert_array_equal(reps, [3, 1, 4, 6])      # in the order of the clusters' smallest members
    assert dr.format_rows(db, dr.greedy_labels(rep), reps) == [
        "g0\tg3\t0\t3", "g1\tg1\t1\t2", "g2\tg3\t0\t3", "g3\tg3\t0\t3", "g4\tg4\t2\t1", "g5\tg1\t1\t2", "g6\tg6\t3\t1"]
    assert dr.subset_db(db, reps).names == ["g1", "g3", "g4", "g6"]    # DB order
    np.testing.assert_array_equal(dr.greedy_labels([]), [])
    np.testing.assert_array_equal(dr.greedy_representatives([]), [])
    with pytest.raises(ValueError):
        dr.greedy_labels([1, 2, 2])                        # 0's representative is a member


def test_cluster_greedy_refuses_bad_arguments_before_any_device_work():
    from hymet_amd import derep as dr
    db = make_db([[1, 2], [2, 3]], 2)
    for bad in (1.0, 1.5, -0.01, float("nan")):
        with pytest.raises(ValueError):
            dr.cluster_greedy(None, db, bad)               # no GPU object is ever touched
    with pytest.raises(ValueError):
        dr.cluster_greedy(None, db, 0.05, rule="median")


# ------------------------------------------------------------------ the graph of the GPU test
def test_parity_graph_exercises_the_nearest_rule():
    """The real-pair graph test_derep_greedy_gpu.py runs on the device, here on the reference
    with the host merge loop: greedy and single linkage differ, and so do nearest and first."""
    from hymet_amd import mashdist as md
    from tests.test_mashdist_gpu import merge_loop, parity_lists
    s = 64
    lists = [np.asarray(a, np.uint64).tolist() for a in parity_lists(s, 300, 1)[0]]
    n = len(lists)
    vals = {(q, r): merge_loop(lists[r], lists[q], s) for q in range(n) for r in range(q)}
    for max_dist, n_reps, n_single, n_not_first in ((0.3, 24, 3, 21), (0.05, 57, 55, None)):
        t = md.min_common_table(s, K, max_dist)
        pairs = {k: v for k, v in vals.items() if v[1] <= s and v[0] >= t[v[1]]}
        rep = gr.greedy(n, pairs)
        gr.check_members_pass(rep, pairs)
        gr.check_representatives_apart(rep, pairs)
        assert int((rep == np.arange(n)).sum()) == n_reps
        assert len(np.unique(cc_labels(n, pairs))) == n_single
        if n_not_first is not None:
            assert int((rep != gr.first_passing(n, pairs)).sum()) == n_not_first
