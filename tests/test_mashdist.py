"""Host side of `cli dist` (hymet_amd/mashdist.py): the distance and p-value arithmetic, the
device filter's table, the DB compatibility rules, the text forms and the argument parser.
No GPU."""
import math

import numpy as np
import pytest

from hymet_amd.msh import SketchDB


def _db(names, lengths, **kw):
    n = len(names)
    return SketchDB(names=list(names), comments=[""] * n, lengths=np.asarray(lengths, np.int64),
                    offsets=np.zeros(n + 1, np.int64), hashes=np.zeros(0, np.uint64), **kw)


def test_distance_exact_cases():
    from hymet_amd.mashdist import distance
    d = distance(1000, 1000, 21)
    assert d == 0.0 and math.copysign(1.0, d) == 1.0          # 0.0, not -0.0
    d = distance(0, 0, 21)
    assert d == 0.0 and math.copysign(1.0, d) == 1.0          # 0/0
    assert distance(0, 1000, 21) == 1.0
    assert distance(500, 1000, 21) == pytest.approx(-math.log(2.0 / 3.0) / 21, rel=1e-15)
    assert isinstance(distance(500, 1000, 21), float)


def test_distance_vectorised_equals_scalar():
    from hymet_amd.mashdist import distance
    c = np.array([1000, 0, 0, 500, 1, 999, 37])
    d = np.array([1000, 0, 1000, 1000, 1000, 1000, 64])
    v = distance(c, d, 21)
    assert v.dtype == np.float64 and v.shape == c.shape
    assert not np.signbit(v).any()
    for i in range(len(c)):
        assert v[i] == distance(int(c[i]), int(d[i]), 21)      # bit-identical
    assert (np.diff(distance(np.arange(1, 1001), np.full(1000, 1000), 21)) < 0).all()


def test_p_value():
    from hymet_amd.mashdist import p_value
    from hymet_amd.screen import binomial_upper_tail
    assert p_value(0, 1000, 5_000_000, 4_000_000, 21, 4) == 1.0
    assert p_value(10, 1000, 0, 4_000_000, 21, 4) == 1.0
    assert p_value(10, 1000, 5_000_000, 0, 21, 4) == 1.0
    for common, denom, lr, lq, k in [(1, 1000, 5_000_000, 4_000_000, 21), (3, 1000, 3_000, 20_000, 11),
                                     (700, 1000, 12_000, 12_000, 21), (5, 64, 100_000, 50_000, 9)]:
        space = 4.0 ** k
        px, py = 1.0 / (1.0 + space / lr), 1.0 / (1.0 + space / lq)
        r = px * py / (px + py - px * py)
        want = binomial_upper_tail(common - 1, r, denom)
        assert p_value(common, denom, lr, lq, k, 4) == want
        assert 0.0 <= want <= 1.0
    assert p_value(3, 1000, 3_000, 20_000, 11, 4) > p_value(30, 1000, 3_000, 20_000, 11, 4)


@pytest.mark.parametrize("max_dist", [0.0, 0.01, 0.05, 0.3, 0.999, 1.0, -0.5])
@pytest.mark.parametrize("k", [21, 11])
def test_min_common_table_agrees_with_distance(max_dist, k):
    from hymet_amd.mashdist import distance, min_common_table
    s = 64
    t = min_common_table(s, k, max_dist)
    assert t.dtype == np.uint16 and len(t) == s + 1
    for denom in range(s + 1):
        c = int(t[denom])
        assert 0 <= c <= denom + 1
        if c <= denom:
            assert distance(c, denom, k) <= max_dist
        if c >= 1:
            assert distance(c - 1, denom, k) > max_dist
        # the filter `common >= t[denom]` is the filter `distance <= max_dist`
        for common in range(denom + 1):
            assert (common >= c) == (distance(common, denom, k) <= max_dist), (common, denom)


def test_min_common_table_large_s():
    from hymet_amd.mashdist import distance, min_common_table
    s = 16384
    t = min_common_table(s, 21, 0.05).astype(np.int64)
    d = np.arange(s + 1)
    assert (t[1:] >= 1).all() and (t <= d).all()
    assert (distance(t[1:], d[1:], 21) <= 0.05).all()
    assert (distance(t[1:] - 1, d[1:], 21) > 0.05).all()


def test_check_compatible(capsys):
    from hymet_amd.mashdist import check_compatible
    ref = _db(["r"], [10], k=21, seed=42, sketch_size=1000)
    assert check_compatible(ref, _db(["q"], [10], k=21, seed=42, sketch_size=1000)) == 1000
    assert capsys.readouterr().err == ""
    for kw in (dict(k=19), dict(seed=7), dict(alphabet="ACGTN"), dict(noncanonical=True)):
        args = dict(k=21, seed=42, sketch_size=1000)
        args.update(kw)
        with pytest.raises(ValueError):
            check_compatible(ref, _db(["q"], [10], **args))
    nonc = _db(["r"], [10], k=21, seed=42, sketch_size=1000, noncanonical=True)
    with pytest.raises(ValueError, match="[Nn]oncanonical"):
        check_compatible(nonc, nonc)
    assert capsys.readouterr().err == ""
    assert check_compatible(ref, _db(["q"], [10], k=21, seed=42, sketch_size=400)) == 400
    err = capsys.readouterr().err
    assert err.count("WARNING") == 1 and "400" in err and "1000" in err
    assert check_compatible(_db(["r"], [10], sketch_size=200), ref) == 200
    assert capsys.readouterr().err.count("WARNING") == 1
    assert check_compatible(ref, _db(["q"], [10], sketch_size=400), warn=False) == 400
    assert capsys.readouterr().err == ""


def _case_2x3():
    ref = _db(["refA", "refB", "refC"], [5_000_000, 4_000_000, 0], k=21, sketch_size=1000)
    qry = _db(["q1", "q2"], [4_500_000, 3_000], k=21, sketch_size=1000)
    common = np.array([1000, 500, 0, 1, 0, 7])
    denom = np.array([1000, 1000, 1000, 1000, 1000, 1000])
    qi = np.repeat(np.arange(2), 3)
    ri = np.tile(np.arange(3), 2)
    return ref, qry, qi, ri, common, denom


def test_format_lines():
    from hymet_amd.mashdist import format_lines, p_value
    ref, qry, qi, ri, common, denom = _case_2x3()
    lines = format_lines(ref, qry, qi, ri, common, denom)
    assert len(lines) == 6
    p_half = "%g" % p_value(500, 1000, 4_000_000, 4_500_000, 21)
    p_one = "%g" % p_value(1, 1000, 5_000_000, 3_000, 21)
    assert lines[0] == "refA\tq1\t0\t0\t1000/1000"
    assert lines[1] == "refB\tq1\t0.0193079\t%s\t500/1000" % p_half
    assert lines[2] == "refC\tq1\t1\t1\t0/1000"
    assert lines[3] == "refA\tq2\t0.295981\t%s\t1/1000" % p_one
    assert lines[4] == "refB\tq2\t1\t1\t0/1000"
    assert lines[5] == "refC\tq2\t0.203604\t1\t7/1000"          # a reference of recorded length 0: p = 1
    assert float(p_half) == 0.0 and 0.0 < float(p_one) < 1.0
    # -d
    assert format_lines(ref, qry, qi, ri, common, denom, max_dist=0.25) == [lines[0], lines[1], lines[5]]
    # -v keeps p <= P: the chance-level pair and the p = 1 pairs go
    assert format_lines(ref, qry, qi, ri, common, denom, max_p=float(p_one) / 2) == [lines[0], lines[1]]
    assert format_lines(ref, qry, qi, ri, common, denom, max_p=float(p_one) * 2) == [lines[0], lines[1], lines[3]]


def test_format_table():
    from hymet_amd.mashdist import format_table
    ref, qry, _, _, common, denom = _case_2x3()
    assert format_table(ref, qry, common, denom) == [
        "#query\trefA\trefB\trefC",
        "q1\t0\t0.0193079\t1",
        "q2\t0.295981\t1\t0.203604",
    ]
    assert format_table(ref, qry, common.reshape(2, 3), denom.reshape(2, 3))[2] == "q2\t0.295981\t1\t0.203604"


def test_concat_dbs():
    from hymet_amd.mashdist import concat_dbs
    a = SketchDB(names=["a0", "a1"], comments=["", "x"], lengths=np.array([5, 6]), offsets=np.array([0, 2, 3]),
                 hashes=np.array([1, 5, 9], np.uint64), sketch_size=3)
    b = SketchDB(names=["b0"], comments=["y"], lengths=np.array([7]), offsets=np.array([0, 2]),
                 hashes=np.array([2, 2 ** 64 - 1], np.uint64), sketch_size=2)
    c = concat_dbs([a, b])
    assert list(c.names) == ["a0", "a1", "b0"] and list(c.comments) == ["", "x", "y"]
    assert c.offsets.tolist() == [0, 2, 3, 5] and c.lengths.tolist() == [5, 6, 7] and c.sketch_size == 2
    assert c.hashes.tolist() == [1, 5, 9, 2, 2 ** 64 - 1] and c.hashes.dtype == np.uint64
    assert concat_dbs([a]) is a


def test_dist_argument_parser(capsys):
    from hymet_amd import cli
    a = cli.dist_args(["ref.msh", "q.fna"])
    assert (a.max_dist, a.max_p, a.table, a.individual, a.lists) == (1.0, 1.0, False, False, False)
    assert a.ref == "ref.msh" and a.queries == ["q.fna"]
    a = cli.dist_args(["-t", "-d", "0.1", "-v", "1e-5", "-i", "-l", "ref.msh", "a.msh", "b.fna"])
    assert a.table and a.individual and a.lists and a.max_dist == 0.1 and a.max_p == 1e-5
    assert a.queries == ["a.msh", "b.fna"]
    capsys.readouterr()
    for bad in (["-x", "ref.msh", "q.fna"], ["ref.msh"], [], ["-d", "abc", "ref.msh", "q.fna"]):
        assert cli.dist_args(bad) is None
        assert cli.DIST_USAGE in capsys.readouterr().err
        assert cli.main(["dist"] + bad) == 2
        capsys.readouterr()
