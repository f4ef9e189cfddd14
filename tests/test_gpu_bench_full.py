"""bench.py with and without --full on a small frame: a plain run times the headline and reports nothing that needs a run of its own;
--full adds the side legs, the clock probe, the CPU baseline and the parity against the checker, and their checks hold."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIDE_KEYS = ("loop_mode", "reference_schedule", "deployed_max_steps_16", "folded_geo", "fp16_head", "cfg5_1024_ellipsoid_f16", "dense192",
             "cfg2_hashgrid_render", "roofline_gridencoder", "train_step", "occupancy_grid_update", "torso_branch", "talking_head_frame",
             "cpu_baseline", "psnr_vs_checker_db")


def run_bench(tmp_path, tag, extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--size", "64",
           "--detail", str(tmp_path / f"{tag}.json")] + extra
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0]), json.load(open(tmp_path / f"{tag}.json"))


def test_plain_run_and_full_run(tmp_path):
    line, detail = run_bench(tmp_path, "plain", [])
    assert line["steps"] == 2 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["value"] > 0 and line["dtype"] == "f32"
    assert line["roofline"]["avg_launch_ms"] > 0 and detail["roofline"]["shader_clock_mhz_under_load"] is None
    assert not any(k in detail for k in SIDE_KEYS) and "leg_errors" not in detail
    assert not any(k in line for k in ("cpu_baseline", "legs_ms", "checks", "roofline_f16", "roofline_gridencoder"))
    full, fdetail = run_bench(tmp_path, "full", ["--full"])
    assert "leg_errors" not in fdetail, fdetail.get("leg_errors")
    assert all(k in fdetail for k in SIDE_KEYS), [k for k in SIDE_KEYS if k not in fdetail]
    assert fdetail["roofline"]["shader_clock_mhz_under_load"] is not None
    assert full["checks"] == {"reference_schedule_image_equal": True, "deployed_16_image_equal": True, "deployed_16_counts_equal": True}
    assert full["psnr_vs_checker_db"] == "inf" and full["sample_counts_equal"] is True and full["cpu_baseline"]["s_per_frame"] > 0
    # the headline itself is the same computation in both runs
    assert full["config"]["samples_per_step"] == line["config"]["samples_per_step"] and full["metric"] == line["metric"]
