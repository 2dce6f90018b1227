"""bench.py's multi-rank contract (the driver runs `bench.py --gpus N` under
torch.distributed.run, or bare): `--gpus N` without a launcher starts N rank processes, the
world size must equal N, and rank 0 prints one JSON line for the whole job.

CPU: the launch and the record sharding in gloo dry mode.  GPU: two ranks sharing one GPU
(gloo staging the collectives through the host) must write the same classified_sequences.tsv
as one rank on the same synthetic workload."""
import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(REPO, "bench.py")


def _env():
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    return env


def _json_line(out: str) -> dict:
    lines = [l for l in out.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out
    return json.loads(lines[0])


@pytest.mark.timeout(300)
def test_gpus2_launches_two_ranks_dry():
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--dry-run"], capture_output=True, text=True,
                       env=_env(), timeout=280)
    assert r.returncode == 0, r.stderr[-3000:]
    line = _json_line(r.stdout)
    assert line["n_gpus"] == 2 and line["backend"] == "gloo" and line["covers_input_once"]
    assert line["shards"][0][0] == 0 and line["shards"][0][1] == line["shards"][1][0]


@pytest.mark.timeout(120)
def test_world_size_must_match_gpus():
    env = _env()
    env.update(RANK="0", WORLD_SIZE="3", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--dry-run"], capture_output=True, text=True, env=env,
                       timeout=110)
    assert r.returncode != 0 and "started 3 rank(s)" in r.stderr


def test_plain_run_is_the_default_and_full_is_an_option():
    """--full (the CPU baseline and the shard-balance prediction) is off unless asked for."""
    sys.path.insert(0, REPO)
    import bench
    assert bench.parse_args([]).full is False and bench.parse_args([]).dump_outputs is None
    a = bench.parse_args(["--full", "--dump-outputs", "d", "--steps", "7"])
    assert a.full is True and a.dump_outputs == "d" and a.steps == 7
    with pytest.raises(SystemExit):
        bench.parse_args(["--steps", "0"])


def test_dump_outputs_writes_the_result_as_float64_arrays(tmp_path):
    """--dump-outputs: every array a caller of the timed path receives, text as CRC-32."""
    import zlib
    from types import SimpleNamespace as NS

    import numpy as np
    sys.path.insert(0, REPO)
    import bench
    from hymet_amd.pipeline import TSV_HEADER, RunResult
    scr = [NS(shared=np.array([3, 0, 7], np.int32), median=np.array([1, 0, 2], np.int32), set_size=11, n_kmers=99)]
    tsv = TSV_HEADER + b"c1\tk__A;p__B\tphylum\t0.7500\r\nc2\tUnknown\troot\t0.0000\r\n"
    paf = (b"c1\t100\t2\t90\t+\tt1\t500\t10\t98\t80\t88\t60\ttp:A:P\tcm:i:9\n"
           b"c2\t50\t0\t50\t-\tt2\t300\t5\t55\t45\t50\t0\ttp:A:P\tcm:i:4\n")
    res = RunResult(["t1.fna.gz", "t2.fna.gz"], [[]], ["0.9"], tsv, 2, 1, 2, paf, scr)
    bench.dump_outputs(str(tmp_path), scr, res)
    got = {p.stem: np.load(p) for p in tmp_path.glob("*.npy")}
    assert set(got) == {"screen0_shared", "screen0_median", "screen_sizes", "selected", "tsv", "paf_sample", "summary"}
    assert all(a.dtype == np.float64 for a in got.values())
    assert got["screen0_shared"].tolist() == [3, 0, 7] and got["screen_sizes"].tolist() == [[11, 99]]
    assert got["selected"].tolist() == [zlib.crc32(b"t1.fna.gz"), zlib.crc32(b"t2.fna.gz")]
    assert got["tsv"].tolist() == [[zlib.crc32(b"c1"), zlib.crc32(b"k__A;p__B"), zlib.crc32(b"phylum"), 0.75],
                                   [zlib.crc32(b"c2"), zlib.crc32(b"Unknown"), zlib.crc32(b"root"), 0.0]]
    assert got["paf_sample"].tolist() == [
        [0, zlib.crc32(b"c1"), 100, 2, 90, 1, zlib.crc32(b"t1"), 500, 10, 98, 80, 88, 60, zlib.crc32(b"tp:A:P\tcm:i:9")],
        [1, zlib.crc32(b"c2"), 50, 0, 50, -1, zlib.crc32(b"t2"), 300, 5, 55, 45, 50, 0, zlib.crc32(b"tp:A:P\tcm:i:4")]]
    assert got["summary"].tolist() == [2, 1, 2, len(tsv), zlib.crc32(tsv), len(paf), zlib.crc32(paf)]
    # more lines than the cap: a fixed sample, the same from call to call, in file order
    many = RunResult([], [[]], [], TSV_HEADER, 0, 0, 0, paf * (bench.DUMP_PAF_LINES // 2 + 5), [])
    bench.dump_outputs(str(tmp_path / "a"), [], many)
    bench.dump_outputs(str(tmp_path / "b"), [], many)
    a, b = np.load(tmp_path / "a" / "paf_sample.npy"), np.load(tmp_path / "b" / "paf_sample.npy")
    assert a.shape == (bench.DUMP_PAF_LINES, 14) and np.array_equal(a, b) and np.all(np.diff(a[:, 0]) > 0)
    assert sum(p.stat().st_size for p in (tmp_path / "a").glob("*.npy")) < 64e6


SMALL = ["--taxa", "2", "--per-taxon", "3", "--contig-gbp", "0.004", "--db-hashes", "2e4", "--batch-mbp", "1",
         "--map-streams", "1", "--no-cpu", "--steps", "1", "--warmup", "1"]


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_bench_two_ranks_tsv_equals_one_rank(tmp_path):
    one, two = tmp_path / "one.tsv", tmp_path / "two.tsv"
    r1 = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--tsv-out", str(one), "--dump-outputs",
                         str(tmp_path / "dump")] + SMALL, capture_output=True, text=True, env=_env(), timeout=280)
    assert r1.returncode == 0, r1.stderr[-3000:]
    r2 = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--backend", "gloo", "--share-gpu", "--tsv-out", str(two)]
                        + SMALL, capture_output=True, text=True, env=_env(), timeout=280)
    assert r2.returncode == 0, r2.stderr[-3000:]
    l1, l2 = _json_line(r1.stdout), _json_line(r2.stdout)
    assert l1["n_gpus"] == 1 and l2["n_gpus"] == 2 and l2["config"]["backend"] == "gloo"
    assert l1["paf_lines"] == l2["paf_lines"] > 0
    a, b = one.read_bytes(), two.read_bytes()
    assert a.count(b"\r\n") > 10 and a == b
    # the plain line carries no leg of --full, and --dump-outputs wrote the last step's result
    import zlib

    import numpy as np
    assert "cpu_baseline" not in l1 and "predicted_imbalance" not in l1["config"] and l1["ms_per_step"] > 0
    s = np.load(tmp_path / "dump" / "summary.npy")
    assert s.dtype == np.float64 and s[2] == l1["paf_lines"] and s[3] == len(a) and s[4] == zlib.crc32(a)
    assert len(np.load(tmp_path / "dump" / "tsv.npy")) == a.count(b"\r\n") - 1 == s[0]
    assert len(np.load(tmp_path / "dump" / "paf_sample.npy")) == min(l1["paf_lines"], 200_000)
