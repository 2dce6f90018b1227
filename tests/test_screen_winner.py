"""Winner-take-all screen (`mash screen -w`), host side: the reference restatement on the
worked example, the host ranking, the command-line parsing and the output rows.  No GPU."""
import math

import numpy as np

from tests._winner_ref import winner_ref


def _db(hash_lists, lengths=None, k=21, names=None):
    from hymet_amd.msh import SketchDB
    n = len(hash_lists)
    off = np.zeros(n + 1, np.int64)
    off[1:] = np.cumsum([len(h) for h in hash_lists])
    names = names or [f"ref{i}.fna.gz" for i in range(n)]
    hs = np.concatenate([np.asarray(h, np.uint64) for h in hash_lists]) if n else np.zeros(0, np.uint64)
    return SketchDB(k=k, sketch_size=max([len(h) for h in hash_lists] + [1]), names=names,
                    comments=[f"[1 seqs] {x}" for x in names],
                    lengths=np.zeros(0, np.int64) if lengths is None else np.asarray(lengths, np.int64), offsets=off, hashes=hs)


EX_HASHES = [[1, 2, 3, 4], [3, 4, 5, 6], [5, 6, 7, 8]]
EX_LENGTHS = [100, 200, 50]
EX_COUNTS = {1: 2, 2: 1, 3: 5, 4: 1, 5: 3, 6: 0, 7: 0, 8: 4}


def test_worked_example_reference():
    off = [0, 4, 8, 12]
    hashes = [h for hs in EX_HASHES for h in hs]
    for k in (21, 16, 32):
        shared, shared_w, median_w = winner_ref(off, hashes, EX_LENGTHS, EX_COUNTS, k)
        assert shared == [4, 3, 2]
        assert shared_w == [4, 1, 1]
        assert median_w == [2, 3, 4]


def test_worked_example_ranking():
    from hymet_amd.screen import rank_competitors
    db = _db(EX_HASHES, EX_LENGTHS)
    assert rank_competitors(db, np.array([4, 3, 2], np.uint32)).tolist() == [0, 1, 2]


def test_rank_score_tie_broken_by_length():
    from hymet_amd.screen import rank_competitors
    db = _db([[1, 2, 3, 4]] * 3, [100, 300, 200])
    assert rank_competitors(db, np.array([2, 2, 2], np.uint32)).tolist() == [1, 2, 0]
    # the score comes first: a longer genome does not beat a better identity
    assert rank_competitors(db, np.array([3, 2, 2], np.uint32)).tolist() == [0, 1, 2]


def test_rank_full_tie_broken_by_index():
    from hymet_amd.screen import rank_competitors
    db = _db([[1, 2, 3, 4]] * 4, [100, 100, 100, 100])
    assert rank_competitors(db, np.array([2, 2, 0, 2], np.uint32)).tolist() == [0, 1, 3]   # shared 0 does not compete


def test_rank_full_sketch_scores_exactly_one():
    from hymet_amd.screen import mash_identity, rank_competitors
    assert mash_identity(4, 4, 21) == 1.0
    assert mash_identity(1000, 1000, 21) == 1.0
    assert mash_identity(999, 1000, 21) == math.pow(999 / 1000, 1.0 / 21) < 1.0
    assert mash_identity(0, 1000, 21) == 0.0
    # a short sketch found whole outranks a long one found almost whole, whatever the lengths
    db = _db([list(range(1, 1001)), [2001, 2002, 2003]], [10**7, 10])
    assert rank_competitors(db, np.array([999, 3], np.uint32)).tolist() == [1, 0]


def test_rank_different_sketch_lengths():
    from hymet_amd.screen import rank_competitors
    # 3/4 = 0.75 > 7/10 = 0.7 > 1/2: the fraction found decides, not the number of hashes found
    db = _db([list(range(10, 20)), [1, 2, 3, 4], [5, 6]], [1, 1, 1], k=16)
    assert rank_competitors(db, np.array([7, 3, 1], np.uint32)).tolist() == [1, 0, 2]
    # 2/4 and 5/10 are the same double: a score tie across sketch lengths goes to the length
    db = _db([list(range(10, 20)), [1, 2, 3, 4]], [5, 9], k=16)
    assert rank_competitors(db, np.array([5, 2], np.uint32)).tolist() == [1, 0]


def test_rank_missing_lengths_count_as_zero():
    from hymet_amd.screen import rank_competitors
    for lengths in (None, [500], [1, 2, 3, 4, 5]):      # not one per reference: all lengths 0
        db = _db([[1, 2, 3, 4]] * 3, lengths)
        assert rank_competitors(db, np.array([2, 2, 2], np.uint32)).tolist() == [0, 1, 2]
        assert rank_competitors(db, np.array([1, 2, 3], np.uint32)).tolist() == [2, 1, 0]
    assert rank_competitors(_db([[1, 2]] * 2, [5, 6]), np.zeros(2, np.uint32)).tolist() == []


def test_rank_agrees_with_reference_on_random_cases():
    """The host order, applied key by key, credits what the reference credits."""
    from hymet_amd.screen import rank_competitors
    rng = np.random.default_rng(12)
    for trial in range(20):
        n = int(rng.integers(2, 9))
        keys = np.arange(1, 41)
        hl = [np.sort(rng.choice(keys, size=int(rng.integers(1, 12)), replace=False)).tolist() for _ in range(n)]
        lengths = rng.integers(1, 4, size=n).tolist()       # few values: ties happen
        counts = {int(x): int(c) for x, c in zip(keys, rng.integers(0, 4, size=len(keys)))}
        db = _db(hl, lengths)
        shared, shared_w, _ = winner_ref(db.offsets, db.hashes, lengths, counts, db.k)
        order = rank_competitors(db, np.array(shared, np.uint32)).tolist()
        prio = {r: p for p, r in enumerate(order)}
        got = [0] * n
        for key, c in counts.items():
            holders = [r for r in range(n) if key in hl[r]]
            if c > 0 and holders:
                got[min(holders, key=lambda r: prio[r])] += 1
        assert got == shared_w, trial


def test_mash_screen_args(capsys):
    from hymet_amd import cli
    a = cli.mash_screen_args(["db.msh", "a.fna"])
    assert (a.winner, a.min_identity, a.max_p, a.db, a.inputs) == (False, 0.0, 1.0, "db.msh", ["a.fna"])
    a = cli.mash_screen_args(["-w", "-i", "0.8", "-v", "0.05", "db.msh", "a.fna", "b.fna"])
    assert (a.winner, a.min_identity, a.max_p, a.db, a.inputs) == (True, 0.8, 0.05, "db.msh", ["a.fna", "b.fna"])
    capsys.readouterr()
    for bad in (["-x", "db.msh", "a.fna"], ["-w"], ["-w", "db.msh"], [], ["-i", "high", "db.msh", "a.fna"]):
        assert cli.mash_screen_args(bad) is None
        assert cli.MASH_SCREEN_USAGE in capsys.readouterr().err
        assert cli.main(["mash-screen"] + bad) == 2
        err = capsys.readouterr()
        assert err.err.rstrip("\n").endswith(cli.MASH_SCREEN_USAGE) and err.out == ""
    assert cli.MASH_SCREEN_USAGE == "usage: mash-screen [-w] [-i MIN_IDENTITY] [-v MAX_P] DB.msh FILE..."
    assert "mash-screen [-w]" in cli.__doc__ and "HYMET_SCREEN_WINNER" in cli.__doc__


def test_screen_winner_env(monkeypatch, capsys):
    from hymet_amd import cli
    assert cli.screen_winner_env({}) is False
    for v in ("", "0", "false", "no", "off", " 0 "):
        assert cli.screen_winner_env({"HYMET_SCREEN_WINNER": v}) is False
    for v in ("1", "true", "YES", "on"):
        assert cli.screen_winner_env({"HYMET_SCREEN_WINNER": v}) is True
    monkeypatch.setenv("HYMET_SCREEN_WINNER", "1")
    assert cli.screen_winner_env() is True
    monkeypatch.delenv("HYMET_SCREEN_WINNER")
    assert cli.screen_winner_env() is False
    # a value that is neither is refused before anything is read or written
    monkeypatch.setenv("HYMET_SCREEN_WINNER", "maybe")
    assert cli.main(["screen"] + ["x"] * 8) == 2
    assert "HYMET_SCREEN_WINNER" in capsys.readouterr().err


def test_format_screen_on_winner_arrays_matches_oracle_rows():
    from hymet_amd.screen import ScreenResult, format_screen
    from oracle import select_oracle
    rng = np.random.default_rng(3)
    hl = [np.sort(rng.choice(2**40, size=n, replace=False)).tolist() for n in (1000, 1000, 400, 1000, 37)]
    db = _db(hl, [10**6] * 5)
    first = np.array([1000, 930, 400, 0, 20], np.uint32)
    shared_w = np.array([1000, 11, 0, 0, 20], np.uint32)
    median_w = np.array([7, 2, 0, 0, 3], np.uint32)
    refs = [(db.names[i], db.comments[i], len(hl[i])) for i in range(5)]
    for v_max, ident in ((0.9, 0.0), (1.0, 0.0), (1.0, -1.0), (0.9, 0.85)):
        want = select_oracle.screen_lines(refs, shared_w, median_w, 123_456, db.k, v_max=v_max, identity_min=ident)
        assert format_screen(db, shared_w, median_w, 123_456, v_max, ident) == want
        res = ScreenResult(db, shared_w, median_w, 123_456, 10**6, True, first, median_w)
        assert res.lines(v_max, ident) == want
    assert len(format_screen(db, shared_w, median_w, 123_456, 1.0, 0.0)) == 3
    # without winner the first-pass names are the arrays themselves
    plain = ScreenResult(db, first, median_w, 123_456, 10**6)
    assert plain.winner is False and plain.shared_first is plain.shared and plain.median_first is plain.median
