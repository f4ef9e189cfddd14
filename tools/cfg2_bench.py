#!/usr/bin/env python3
"""BASELINE cfg2 alone (256 x 256 rays, max_steps 128, all-ones occupancy, hash-grid NeRF): the fused path (lzzx_nerf_amd/ngp.py) under a
few schedules, next to the operator-API device loop.  tools/cfg2_bench.py [f32|f16|autocast] [--ref] [B,C ...]
    f32       f32 tables, f32 head
    f16       half tables, f32 head (half_tables=True: the bench leg cfg2_fused_f16_ms)
    autocast  half tables, half head (precision="f16": the reference's torch-autocast arithmetic)
  --mode loop|fused|both   HashgridRenderer's mode (default loop; fused: csrc/lz_ngp_frame.hip needs n_step_cap 8).  both: loop and
                           fused ALTERNATED, --rounds times each (default 2), every timing listed: the same-box comparison of DESIGN 4.5
  --max-steps K            (default 128)      --size S   an S x S frame (default 256; 64 = a tile)      --cap reference|per_ray"""
import json, os, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lzzx_nerf_amd.ngp import FusedHashgridNeRF, HashgridRenderer
from lzzx_nerf_amd.synthetic import GenericHashgridNeRF, synthetic_camera
from lzzx_nerf_amd.utils import frame_rays

def _opt(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


rmode, cap = _opt("--mode", "loop"), _opt("--cap", "reference")
max_steps, size, rounds = int(_opt("--max-steps", 128)), int(_opt("--size", 256)), int(_opt("--rounds", 2))
mode = sys.argv[1] if len(sys.argv) > 1 and sys.argv[1] in ("f32", "f16", "autocast") else "f32"
half = mode in ("f16", "autocast")
dev = torch.device("cuda", 0)
pose, intr = synthetic_camera(size, size)
ro, rd = frame_rays(torch.from_numpy(np.ascontiguousarray(pose)).to(dev), intr, size, size)
aabb = torch.tensor([-1, -1, -1, 1, 1, 1], dtype=torch.float32, device=dev)
bits = torch.full((128 ** 3 // 8,), 255, dtype=torch.uint8, device=dev)
g = GenericHashgridNeRF(dev, half_tables=half)
net = FusedHashgridNeRF(g.enc, g.sigma_net, g.color_net, half_tables=half, precision="f16" if mode == "autocast" else "f32")


def timed(f, n=10):
    for _ in range(3):
        o = f()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        o = f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3, o


scheds = [tuple(int(x) for x in a.split(",")) for a in sys.argv[2:] if "," in a] or [(8, 8), (4, 4), (8, 16), (16, 16), (1, 8)]
out = {"mode": mode, "renderer_mode": rmode, "max_steps": max_steps, "size": size}


def entry(r):
    ms, o = timed(lambda: r.render(ro, rd, max_steps=max_steps))
    st = o["state"].cpu().numpy()
    return dict(ms=round(ms, 3), samples=int(st[5]), rows=int(st[72]), iterations=int(st[6]))


for s in scheds:
    if rmode == "both":
        rs = {m: HashgridRenderer(net, bits, bound=1.0, aabb=aabb, budget_factor=s[0], n_step_cap=s[1], mode=m, cap=cap) for m in ("loop", "fused")}
        runs = [(m, entry(rs[m])) for _ in range(rounds) for m in ("loop", "fused")]
        out["%dx%d" % s] = {m: dict(ms=[e["ms"] for k, e in runs if k == m], **{k: v for k, v in [e for kk, e in runs if kk == m][0].items() if k != "ms"})
                            for m in ("loop", "fused")}
        del rs
        continue
    r = HashgridRenderer(net, bits, bound=1.0, aabb=aabb, budget_factor=s[0], n_step_cap=s[1], mode=rmode, cap=cap)
    out["%dx%d" % s] = entry(r)
    del r
if "--ref" in sys.argv:
    from lzzx_nerf_amd.renderer import NetworkRenderer
    nr = NetworkRenderer(lambda x, d: g.net(x, d, 1.0), bits, bound=1.0, aabb=aabb, graph=True)
    ms, o = timed(lambda: nr.render(ro, rd, max_steps=128), 5)
    out["operator_api_device_loop_hipgraph"] = dict(ms=round(ms, 3))
print(json.dumps(out))
