"""bench.py's plain run, --full and --dump-outputs.  A plain run times the steps and prints the line, nothing
else (recall_at_10 null, no side measurements); --full adds the checks and side figures; --dump-outputs writes
the last timed step's answer, and two runs with the same arguments write the same arrays."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--gpus", "1", "--nodes", "40000", "--nq", "64", "--steps", "6", "--warmup", "2", "--pipeline", "3"]


def _run(extra, timeout=600):
    env = dict(os.environ)
    for v in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(v, None)
    pr = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + extra, env=env, cwd=ROOT,
                        stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout)
    lines = [l for l in pr.stdout.decode().splitlines() if l.startswith("{")]
    assert pr.returncode == 0, pr.stderr.decode()[-2000:]
    assert len(lines) == 1, (lines, pr.stderr.decode()[-1000:])
    return json.loads(lines[0])


def _load(d):
    return {n[:-4]: np.load(os.path.join(d, n)) for n in sorted(os.listdir(d)) if n.endswith(".npy")}


def test_dump_masks_unwritten_slots_and_samples_large_outputs(tmp_path, monkeypatch):
    sys.path.insert(0, ROOT)
    monkeypatch.setattr(sys, "argv", ["bench.py"])
    import bench

    ids = np.arange(12, dtype=np.int64).reshape(3, 4)
    dist = np.linspace(0.0, 1.0, 12, dtype=np.float32).reshape(3, 4)
    cnt = np.array([4, 2, 0], dtype=np.int32)
    bench.dump_outputs(str(tmp_path / "all"), ids, dist, cnt)
    got = _load(tmp_path / "all")
    assert sorted(got) == ["counts", "distances", "ids"]
    assert got["ids"].dtype == np.float64 and got["distances"].dtype == np.float32
    assert got["counts"].dtype == np.float32 and got["counts"].tolist() == [4, 2, 0]
    assert got["ids"].tolist() == [[0, 1, 2, 3], [4, 5, -1, -1], [-1, -1, -1, -1]]
    assert got["distances"][0].tolist() == dist[0].tolist() and got["distances"][1, :2].tolist() == dist[1, :2].tolist()
    assert np.isinf(got["distances"][1, 2:]).all() and np.isinf(got["distances"][2]).all()

    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 150)  # room for two of the three rows
    bench.dump_outputs(str(tmp_path / "a"), ids, dist, cnt)
    bench.dump_outputs(str(tmp_path / "b"), ids, dist, cnt)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sorted(a) == ["counts", "distances", "ids", "query_rows"]
    rows = a["query_rows"].astype(np.int64)
    assert len(rows) == 2 and (np.diff(rows) > 0).all()
    assert a["ids"].tolist() == got["ids"][rows].tolist()
    assert sum(v.nbytes for v in a.values()) <= 150
    for n in a:  # the sample is fixed
        assert np.array_equal(a[n], b[n])


@pytest.mark.gpu
@pytest.mark.timeout(1200)
def test_plain_run_is_lean_and_its_outputs_repeat(tmp_path):
    r1 = _run(SMALL + ["--dump-outputs", str(tmp_path / "one")])
    assert r1["steps"] == 6 and r1["warmup"] == 2 and r1["ms_per_step"] > 0 and r1["value"] > 0
    assert r1["full"] is False and r1["recall_at_10"] is None
    for side in ("host_buffer_path", "cpu_baseline", "neutral_workload", "ef_sweep"):
        assert side not in r1
    assert r1["roofline"]["traffic"] is None
    one = _load(tmp_path / "one")
    assert sorted(one) == ["counts", "distances", "ids"]
    assert one["ids"].shape == (64, 10) and one["distances"].shape == (64, 10) and one["counts"].shape == (64,)
    assert (one["counts"] == 10).all() and (one["ids"] >= 0).all() and (one["ids"] < 40000).all()
    assert (np.diff(one["distances"], axis=1) >= 0).all()

    r2 = _run(SMALL + ["--dump-outputs", str(tmp_path / "two")])
    two = _load(tmp_path / "two")
    for n in one:
        assert np.array_equal(one[n], two[n]), n
    assert r2["config"]["per_query"] == r1["config"]["per_query"]

    # the dump is the LAST timed step: 6 steps after 2 warm-ups, 3 in flight, and 1 step after 7 warm-ups, 1 in flight,
    # both end on step 7 = batch 7 (8 distinct batches either way), from another output slot and after other steps
    shifted = ["--steps", "1", "--warmup", "7", "--pipeline", "1"]
    r3 = _run(SMALL[:SMALL.index("--steps")] + shifted + ["--dump-outputs", str(tmp_path / "shifted")])
    assert r3["steps"] == 1 and r3["config"]["distinct_batches"] == r1["config"]["distinct_batches"] == 8
    three = _load(tmp_path / "shifted")
    for n in one:
        assert np.array_equal(one[n], three[n]), n


@pytest.mark.gpu
@pytest.mark.timeout(1200)
def test_full_run_adds_the_checks(tmp_path):
    res = _run(SMALL + ["--full", "--no-traffic", "--no-cpu-baseline", "--no-neutral-side",
                        "--dump-outputs", str(tmp_path / "full")])
    assert res["full"] is True and res["recall_at_10"] > 0.9
    assert res["host_buffer_path"]["ids_equal_device_resident_path"] is True
    assert sorted(_load(tmp_path / "full")) == ["counts", "distances", "ids"]
