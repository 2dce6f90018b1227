"""Host side of the dereplication (hymet_amd/derep.py, `cli derep`, `cli triangle`): no GPU."""
import numpy as np
import pytest

from tests._cc_ref import labels as cc_labels

K = 21


def make_db(lists, s, lengths=None, comments=None):
    from hymet_amd.msh import SketchDB
    lists = [np.asarray(a, np.uint64) for a in lists]
    off = np.zeros(len(lists) + 1, np.int64)
    if lists:
        off[1:] = np.cumsum([len(a) for a in lists])
    n = len(lists)
    return SketchDB(k=K, seed=42, sketch_size=int(s), names=[f"g{i}" for i in range(n)],
                    comments=comments if comments is not None else [f"c{i}" for i in range(n)],
                    lengths=np.asarray(lengths if lengths is not None else [1000 + i for i in range(n)], np.int64),
                    offsets=off, hashes=np.concatenate(lists) if lists else np.zeros(0, np.uint64))


def test_cc_ref():
    np.testing.assert_array_equal(cc_labels(6, [(5, 3), (3, 4), (1, 2)]), [0, 1, 1, 3, 3, 3])
    np.testing.assert_array_equal(cc_labels(0, []), [])
    np.testing.assert_array_equal(cc_labels(4, [(3, 2), (2, 1), (1, 0)]), [0, 0, 0, 0])


def test_representatives_rules_and_ties():
    from hymet_amd import derep as dr
    #         0  1  2  3  4  5  6
    labels = [0, 1, 0, 1, 4, 0, 1]
    lengths = [5, 9, 7, 9, 1, 7, 2]
    # cluster 0 = {0, 2, 5}: lengths 5, 7, 7 -> 2 (tie to the smaller index); cluster 1 = {1, 3, 6}:
    # 9, 9, 2 -> 1; cluster 4 = {4}
    np.testing.assert_array_equal(dr.representatives(labels, lengths), [2, 1, 4])
    np.testing.assert_array_equal(dr.representatives(labels, lengths, "longest"), [2, 1, 4])
    np.testing.assert_array_equal(dr.representatives(labels, lengths, "first"), [0, 1, 4])
    # no recorded length anywhere: every tie goes to the smallest index
    np.testing.assert_array_equal(dr.representatives(labels, [0] * 7), [0, 1, 4])
    np.testing.assert_array_equal(dr.representatives([], []), [])
    np.testing.assert_array_equal(dr.representatives([0], [0]), [0])
    with pytest.raises(ValueError):
        dr.representatives(labels, lengths, "median")


def test_subset_db_round_trip(tmp_path):
    from hymet_amd import derep as dr
    from hymet_amd.msh import load_db, write_msh
    rng = np.random.default_rng(3)
    lists = [np.sort(rng.choice(2 ** 40, size=L, replace=False)).astype(np.uint64) for L in (8, 0, 5, 8, 1, 8)]
    db = make_db(lists, 8, lengths=[10, 0, 30, 2 ** 33, 50, 60])
    sub = dr.subset_db(db, [4, 0, 3])                      # any order in, DB order out
    assert sub.names == ["g0", "g3", "g4"] and sub.comments == ["c0", "c3", "c4"]
    np.testing.assert_array_equal(sub.offsets, [0, 8, 16, 17])
    assert (sub.k, sub.seed, sub.sketch_size) == (db.k, db.seed, db.sketch_size)
    path = tmp_path / "sub.msh"
    write_msh(sub, str(path))
    back = load_db(str(path))
    assert back.names == sub.names and back.comments == sub.comments
    np.testing.assert_array_equal(np.asarray(back.lengths, np.int64)[:3], [10, 2 ** 33, 50])
    assert (back.k, back.seed, back.sketch_size) == (db.k, db.seed, db.sketch_size)
    for n, i in enumerate((0, 3, 4)):
        np.testing.assert_array_equal(np.asarray(back.ref_hashes(n), np.uint64), lists[i])
    empty = dr.subset_db(db, [])
    assert empty.n_refs == 0 and len(empty.hashes) == 0
    with pytest.raises(ValueError):
        dr.subset_db(db, [6])


def test_format_rows():
    from hymet_amd import derep as dr
    db = make_db([[1]] * 5, 1)
    labels = [0, 1, 0, 3, 1]
    reps = dr.representatives(labels, [1, 1, 9, 1, 9])
    np.testing.assert_array_equal(reps, [2, 4, 3])
    assert dr.format_rows(db, labels, reps) == ["g0\tg2\t0\t2", "g1\tg4\t1\t2", "g2\tg2\t0\t2", "g3\tg3\t2\t1",
                                                "g4\tg4\t1\t2"]
    with pytest.raises(ValueError):
        dr.format_rows(db, labels, [2, 3, 4])              # not in cluster order


def test_cluster_refuses_a_threshold_of_one_before_any_device_work():
    from hymet_amd import derep as dr
    db = make_db([[1, 2], [2, 3]], 2)
    for bad in (1.0, 1.5, -0.01, float("nan")):
        with pytest.raises(ValueError):
            dr.cluster(None, db, bad)                      # no GPU object is ever touched


def test_derep_argument_parsing(capsys):
    from hymet_amd import cli
    assert cli.main(["derep"]) == 2
    assert capsys.readouterr().err.splitlines()[-1] == cli.DEREP_USAGE
    assert cli.main(["derep", "-x", "a.msh"]) == 2
    assert capsys.readouterr().err.splitlines()[-1] == cli.DEREP_USAGE
    assert cli.main(["derep", "-d", "1.0", "a.msh"]) == 2
    err = capsys.readouterr().err.splitlines()
    assert err[-1] == cli.DEREP_USAGE and "-d" in err[0]
    assert cli.main(["derep", "-r", "shortest", "a.msh"]) == 2
    capsys.readouterr()
    a = cli.derep_args(["-o", "out", "-i", "a.msh", "b.fna"])
    assert (a.max_dist, a.rule, a.out, a.individual, a.files) == (0.05, "longest", "out", True, ["a.msh", "b.fna"])
    assert (a.k, a.s, a.seed) == (21, 1000, 42)
    a = cli.derep_args(["-d", "0", "-r", "first", "-k", "16", "-s", "200", "-S", "7", "x.fna"])
    assert (a.max_dist, a.rule, a.k, a.s, a.seed) == (0.0, "first", 16, 200, 7)


def test_triangle_argument_parsing(capsys):
    from hymet_amd import cli
    assert cli.main(["triangle"]) == 2
    assert capsys.readouterr().err.splitlines()[-1] == cli.TRIANGLE_USAGE
    assert cli.main(["triangle", "-d", "0.1", "a.msh"]) == 2
    assert capsys.readouterr().err.splitlines()[-1] == cli.TRIANGLE_USAGE
    a = cli.triangle_args(["-l", "list.txt"])
    assert a.lists and not a.individual and a.files == ["list.txt"]
