"""CPU dry run of `bench.py --gpus N` exactly as the driver may launch it -- a plain `python bench.py --gpus 2`, no torchrun
environment: the script must spawn its own ranks (it raised SystemExit), run the shared step driver
(`ssdn.hip.dp.exchange_step`, bucketed exchange) with barrier + max-over-ranks timing, and print ONE JSON line.  With
SSDN_BENCH_STUB=1 a stub stands where the HIP engine stands and the ranks talk gloo; without a GPU and without the stub the same
launch must END in one JSON {"error": ...} line, not in a traceback without a result."""
import json
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(extra_env, *argv):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(extra_env)
    env["OMP_NUM_THREADS"] = "2"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + list(argv), env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=600)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    return p, lines


def test_bench_gpus2_self_spawns_and_prints_one_line():
    p, lines = _run({"SSDN_BENCH_STUB": "1"}, "--gpus", "2", "--steps", "3", "--warmup", "1", "--full")
    assert p.returncode == 0, p.stderr[-3000:]
    assert len(lines) == 1, p.stdout
    r = json.loads(lines[0])
    assert r["n_gpus"] == 2 and r["steps"] == 3 and r["warmup"] == 1 and r["stub"] is True
    assert r["value"] > 0 and r["unit"] == "patches/s" and r["scaling"] == "weak" and r["higher_is_better"] is True
    assert r["config"]["global_batch"] == 64 and r["config"]["parallelism"] == "dp2" and r["config"]["dp_plan"] == "split"
    assert abs(r["value"] - 3 * 64 / (r["ms_per_step"] * 3 / 1e3)) < 1e-2 * r["value"]
    assert "resident" not in r["data"]
    # N > 1: the line says how long the optimiser waited for the gradient exchange behind the backward pass
    assert r["allreduce_exposed_us"] is not None and r["allreduce_exposed_us"] >= 0 and r["allreduce"]["steps"] == 20
    assert sum(r["allreduce"]["collectives_per_step_bytes"]) == 4 * 1269129


def test_bench_plain_run_leaves_the_extra_legs_to_full():
    """A plain run prints the headline line without the measurements that take steps of their own; --full adds them (N > 1: the
    exposed all-reduce over 20 extra steps) and leaves the headline fields as they are."""
    p, lines = _run({"SSDN_BENCH_STUB": "1"}, "--gpus", "2", "--steps", "3", "--warmup", "1")
    assert p.returncode == 0, p.stderr[-3000:]
    assert len(lines) == 1, p.stdout
    r = json.loads(lines[0])
    assert r["n_gpus"] == 2 and r["steps"] == 3 and r["warmup"] == 1 and r["stub"] is True
    assert r["value"] > 0 and r["unit"] == "patches/s" and r["higher_is_better"] is True and r["dtype"] == "f16"
    assert abs(r["value"] - 3 * 64 / (r["ms_per_step"] * 3 / 1e3)) < 1e-2 * r["value"]
    for k in ("allreduce_exposed_us", "allreduce", "families", "value_resident", "value_trainer_hdf5", "cpu_baseline"):
        assert k not in r, k
    p, lines = _run({"SSDN_BENCH_STUB": "1"}, "--gpus", "2", "--steps", "3", "--warmup", "1", "--full")
    assert p.returncode == 0, p.stderr[-3000:]
    f = json.loads(lines[-1])
    assert f["allreduce"]["steps"] == 20
    assert {k: f[k] for k in ("metric", "unit", "higher_is_better", "dtype", "steps", "warmup")} == \
        {k: r[k] for k in ("metric", "unit", "higher_is_better", "dtype", "steps", "warmup")}


def test_bench_dp_plan_is_echoed():
    """SSDN_DP_PLAN picks the weight-gradient plan of the benchmarked engines (a scaling run can A/B "split" against "buckets")."""
    p, lines = _run({"SSDN_BENCH_STUB": "1", "SSDN_DP_PLAN": "buckets"}, "--steps", "2", "--warmup", "1")
    assert p.returncode == 0, p.stderr[-3000:]
    assert json.loads(lines[-1])["config"]["dp_plan"] == "buckets"
    p, lines = _run({"SSDN_BENCH_STUB": "1", "SSDN_DP_PLAN": "nonsense"}, "--steps", "2", "--warmup", "1")
    assert p.returncode != 0 and "error" in json.loads(lines[-1])


def test_bench_single_rank_stub_line():
    p, lines = _run({"SSDN_BENCH_STUB": "1"}, "--steps", "2", "--warmup", "1")
    assert p.returncode == 0, p.stderr[-3000:]
    r = json.loads(lines[-1])
    assert r["n_gpus"] == 1 and r["config"]["global_batch"] == 32 and r["stub"] is True


@pytest.mark.skipif(torch.cuda.is_available(), reason="describes the behaviour on a box WITHOUT a GPU")
def test_bench_failure_is_one_json_error_line():
    p, lines = _run({}, "--gpus", "2", "--steps", "2", "--warmup", "1")
    assert p.returncode != 0
    assert len(lines) == 1, p.stdout
    r = json.loads(lines[0])
    assert "error" in r and r["n_gpus"] == 2


def test_bench_dump_outputs_is_reproducible(tmp_path):
    """--dump-outputs DIR: the last timed step's arrays land in DIR as .npy (float32 / float64) and are listed in the line; the same
    arguments give the same arrays; --steps is the number of timed steps the line reports."""
    import numpy as np
    dumps = []
    for run in ("a", "b"):
        p, lines = _run({"SSDN_BENCH_STUB": "1"}, "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / run))
        assert p.returncode == 0, p.stderr[-3000:]
        r = json.loads(lines[-1])
        assert r["steps"] == 3 and r["ms_per_step"] > 0
        files = r["dump_outputs"]["files"]
        assert "params" in files and files["params"]["shape"] == [1269129]
        arrays = {n: np.load(str(tmp_path / run / (n + ".npy"))) for n in files}
        assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
        assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
        dumps.append(arrays)
    assert dumps[0].keys() == dumps[1].keys()
    for n in dumps[0]:
        assert np.array_equal(dumps[0][n], dumps[1][n]), n
