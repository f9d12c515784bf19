"""bench.py without --full times the headline and nothing else; --full adds the runs of their own after it (N = 1:
single_block, configs, cpu_baseline, other_modes; N > 1: solo and the two scalings that are not the headline)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
sys.path.insert(0, ROOT)
import bench  # noqa: E402

HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "roofline",
            "kernel_ms_per_step", "decrypt_check")
EXTRAS_N1 = ("single_block", "configs", "cpu_baseline", "other_modes")


def test_full_is_off_by_default():
    assert bench.parse_args([]).full is False
    a = bench.parse_args(["--gpus", "1", "--steps", "2", "--warmup", "1", "--full", "--no-cpu-baseline"])
    assert a.full and a.no_cpu_baseline and a.steps == 2 and a.warmup == 1


def _run(args, env_extra=None):
    env = dict(os.environ)
    env.pop("RANK", None)
    env.pop("WORLD_SIZE", None)
    env.update(env_extra or {})
    p = subprocess.run([sys.executable, BENCH] + args, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    line = json.loads(lines[0])
    assert "error" not in line, line.get("error")
    return line


@pytest.mark.gpu
def test_plain_run_is_the_headline_only_and_full_adds_the_rest():
    small = ["--gpus", "1", "--steps", "1", "--warmup", "0", "--blocks", "2"]
    plain = _run(small)
    for key in HEADLINE:
        assert key in plain, key
    assert plain["value"] > 0 and plain["unit"] == "gate-bootstraps/s" and plain["higher_is_better"] is True
    assert plain["config"]["blocks_total"] == 2 and plain["roofline"]["frac"] > 0
    for key in EXTRAS_N1:
        assert key not in plain, key
    # --full with the two longest parts left out: the one-block latency run and the BASELINE.json configurations
    full = _run(small + ["--full", "--no-cpu-baseline", "--no-other-modes"])
    assert full["single_block"]["wall_s"] > 0 and full["single_block"]["bootstraps"] == full["config"]["bootstraps_per_step"] // 2
    assert all(full["configs"][k]["decrypt_ok"] for k in ("1_2bit_adder_gates", "2_c880_class_gates"))
    assert "cpu_baseline" not in full and "other_modes" not in full


@pytest.mark.gpu
def test_plain_run_with_several_ranks_times_the_headline_only():
    """N > 1 (rank threads on one GPU): without --full neither the solo run nor the other two scalings run."""
    line = _run(["--gpus", "2", "--steps", "1", "--warmup", "0", "--blocks", "1"], {"HELM_BENCH_REHEARSE": "threads"})
    assert line["headline_kind"] == "sharded_weak" and line["sharded_weak"]["value"] == line["value"] > 0
    for key in ("solo", "strong", "weak", "n1_same_job_value"):
        assert key not in line, key
    assert set(line["planned_wall_s"]) == {"sharded_weak"}
