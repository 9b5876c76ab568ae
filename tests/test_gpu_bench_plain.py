"""bench.py's two kinds of run.  A plain run does only what `value` needs (set up, warm up, time the steps, write
--dump-outputs, print the line); `--full` adds the readings and checks beside it.  Both run as child processes, as the
benchmark is run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("stages_ms", "roofline", "encode_stage", "route_stage", "variants", "end_to_end", "operator_surface", "timed_check",
             "cpu_baseline", "extra", "recall_sweep", "groundtruth")


def _bench(*args, timeout=600):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", *args], env=env, capture_output=True, text=True,
                       timeout=timeout)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [x for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_writes_the_outputs_only(tmp_path):
    out = tmp_path / "dump"
    d = _bench("--steps", "8", "--warmup", "2", "--dump-outputs", str(out))
    assert d["unit"] == "queries/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
    assert d["metric"].startswith("queries/sec @ recall@10")
    assert d["steps"] == 8 and d["warmup"] == 2 and d["n_gpus"] == 1
    assert d["value"] > 0 and d["ms_per_step"] > 0
    assert abs(d["value"] - 1024 * 1000.0 / d["ms_per_step"]) <= 0.01 * d["value"]
    for key in FULL_ONLY:
        assert d[key] is None, key
    assert d["recall_at_10"] is None and d["cpu_baseline"] is None
    names = sorted(os.listdir(out))
    assert names == ["scored.npy", "topk_count.npy", "topk_dist.npy", "topk_ids.npy"]
    ids, cnt = np.load(out / "topk_ids.npy"), np.load(out / "topk_count.npy")
    assert ids.shape == (1024, 10) and cnt.shape == (1024,) and cnt.max() == 10


@pytest.mark.gpu
def test_full_run_adds_the_readings_and_checks():
    # small workload, no extra passes, no CPU baseline, no child runs: what --full adds to the headline's own pipeline
    # (k = 5: B >= 10 k, one pass per step, so the front pipeline runs and its timed steps are checked)
    d = _bench("--workload", "synth10k_T8_b16_B64_Q100", "--k", "5", "--steps", "8", "--warmup", "2", "--full", "--no-extras",
               "--no-cpu-baseline", "--no-shipped")
    assert d["value"] > 0
    assert d["stages_ms"] is not None and d["roofline"]["launches"] > 0 and d["route_stage"] is not None
    assert d["encode_stage"]["query_side_mfma_vs_exact"]["codes_equal"] is True
    assert d["timed_check"]["same_as_plain_path"] is True
    assert 0.0 <= d["recall_at_k"]["recall"] <= 1.0
    assert d["groundtruth"]["ms"] is not None
