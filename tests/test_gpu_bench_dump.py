"""bench.py --dump-outputs: the arrays the headline path returned in its last timed step, written as float32 .npy files -- equal to what
the renderer returns for the same seeded inputs, and identical between two runs with the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = W = 64
MAX_STEPS = 64


def run_bench(tmp_path, tag, steps):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1", "--size", str(H),
           "--max-steps", str(MAX_STEPS), "--no-side-legs", "--no-clock-probe", "--detail", str(tmp_path / f"{tag}.json"),
           "--dump-outputs", str(tmp_path / tag)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


def test_bench_dumps_the_last_timed_step(tmp_path, params, golden):
    from lzzx_nerf_amd.head import FusedTriplaneHead
    from lzzx_nerf_amd.renderer import TriplaneRenderer
    from lzzx_nerf_amd.synthetic import ones_bitfield, orbit_pose, synthetic_camera
    from lzzx_nerf_amd.utils import frame_rays
    r1, r2 = run_bench(tmp_path, "a", 3), run_bench(tmp_path, "b", 2)
    assert r1["steps"] == 3 and r2["steps"] == 2 and r1["ms_per_step"] > 0 and r2["ms_per_step"] > 0
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == sorted(os.listdir(tmp_path / "b")) and "image.npy" in files and "depth.npy" in files
    assert not any(f.endswith("_rows.npy") for f in files)        # 64 x 64 rays: far below the byte budget, nothing sampled
    got = {f[:-4]: np.load(tmp_path / "a" / f) for f in files}
    for f in files:
        assert got[f[:-4]].dtype == np.float32 and np.array_equal(got[f[:-4]], np.load(tmp_path / "b" / f)), f
    assert got["image"].shape == (H * W, 3) and got["depth"].shape == (H * W,)
    # the same frame through the renderer directly, configured as bench.py's headline
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    head = FusedTriplaneHead({k: torch.from_numpy(v) for k, v in params.items()}, bound=1.0)
    r = TriplaneRenderer(head, dev(ones_bitfield()), bound=1.0, budget_factor=4, n_step_cap=4, mode="fused", cap="reference")
    _, intr = synthetic_camera(H, W)
    ro, rd = frame_rays(dev(orbit_pose(0)), intr, H, W)
    out = r.render(ro, rd, dev(golden["net_enc_a"]), dev(golden["net_ind"]), dev(golden["net_eye"]), dt_gamma=1 / 256,
                   max_steps=MAX_STEPS, T_thresh=1e-4)
    for k, v in got.items():
        np.testing.assert_allclose(v, out[k].float().cpu().numpy(), rtol=0, atol=1e-6, err_msg=k)
