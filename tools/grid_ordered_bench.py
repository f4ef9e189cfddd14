"""The ordered table gradient (lz_grid_encode_backward_ordered: sort + segmented sequential sum, no float atomics) and the order-free one
(lz_grid_encode_backward_fixed: 64-bit integer sums with one scale per level) against the atomic scatter (lz_grid_encode_backward) they
are alternatives to, on two shapes:

    cfg2    the BASELINE cfg2 training batch: 256 x 256 rays, march_rays_train with max_steps 128, D 3, C 2, L 16, T 19, gradient [L, B, C]
    plane   one plane of the triplane head on the same samples' (x, y): D 2, C 1, L 12, T 14, gradient [L, B, C] (the LDS scatter)

The variants alternate; each round times `--iters` calls per variant, every timed step under its own time limit (`--limit` seconds: the
process exits with status 3 when a step has not finished by then); the median over `--rounds` rounds is printed as one JSON line (and
written to `--out`).  Per-kernel time: run under `rocprofv3 --kernel-trace --stats -- python tools/grid_ordered_bench.py --iters 1
--rounds 1` (`--only fixed` leaves the other two variants out of the trace)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from lzzx_nerf_amd import _lib, gridencoder  # noqa: E402
from lzzx_nerf_amd import raymarching as R  # noqa: E402
from lzzx_nerf_amd._util import call, ptr, stream  # noqa: E402
from lzzx_nerf_amd.encoding import get_encoder  # noqa: E402
from lzzx_nerf_amd.synthetic import ellipsoid_bitfield_device, synthetic_camera  # noqa: E402
from lzzx_nerf_amd.utils import frame_rays  # noqa: E402


def timed(fn, iters, limit):
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    for _ in range(iters):
        fn()
    ev1.record()
    deadline = time.monotonic() + limit
    while not ev1.query():
        if time.monotonic() > deadline:
            print("grid_ordered_bench: a timed step did not finish in %.0f s" % limit, file=sys.stderr, flush=True)
            os._exit(3)
        time.sleep(0.0005)
    return ev0.elapsed_time(ev1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--limit", type=float, default=60.0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, help="comma-separated variants to run (atomic, ordered, fixed); default all, with the ratios")
    a = ap.parse_args()
    H = W = a.size
    pose, intr = synthetic_camera(H, W)
    ro, rd = frame_rays(torch.from_numpy(pose).cuda(), intr, H, W)
    bits, _ = ellipsoid_bitfield_device("cuda")
    aabb = torch.tensor([-1, -1, -1, 1, 1, 1], dtype=torch.float32, device="cuda")
    nears, fars = R.near_far_from_aabb(ro, rd, aabb, 0.05)
    ctr = torch.zeros(2, dtype=torch.int32, device="cuda")
    xyzs, _, _, _ = R.march_rays_train(ro, rd, 1.0, bits, 1, 128, nears, fars, ctr, -1, False, 128, True, 1 / 256, 128)
    unit = ((xyzs.detach() + 1.0) / 2.0).contiguous()
    M = unit.shape[0]
    shapes = {}
    for name, kw, x in (("cfg2", dict(), unit),
                        ("plane", dict(input_dim=2, num_levels=12, level_dim=1, base_resolution=64, log2_hashmap_size=14, desired_resolution=512),
                         unit[:, :2].contiguous())):
        enc = get_encoder("hashgrid", **kw)[0].cuda()
        D, C, L = enc.input_dim, enc.level_dim, enc.num_levels
        S, Hres = float(np.float32(np.log2(enc.per_level_scale))), int(enc.base_resolution)
        g = torch.randn(L, M, C, device="cuda")
        ge = torch.zeros_like(enc.embeddings)
        small = name == "plane"

        def atomic(enc=enc, x=x, g=g, ge=ge, D=D, C=C, L=L, S=S, Hres=Hres, small=small):
            ge.zero_()
            call("lz_grid_encode_backward", ptr(g), ptr(x), ptr(enc.embeddings), ptr(enc.offsets), ptr(ge), M, D, C, L, S, Hres, None, None, 0, 0, 0,
                 3 if (small and M >= 16384) else 0, stream())

        def ordered(enc=enc, x=x, g=g, ge=ge, D=D, C=C, L=L, S=S, Hres=Hres):
            ge.zero_()
            gridencoder.grid_backward_ordered(g, x, enc.embeddings, enc.offsets, ge, M, D, C, L, S, Hres, None, None, 0, False, 0)

        def fixed(enc=enc, x=x, g=g, ge=ge, D=D, C=C, L=L, S=S, Hres=Hres):
            ge.zero_()
            gridencoder.grid_backward_fixed(g, x, enc.embeddings, enc.offsets, ge, M, D, C, L, S, Hres, None, None, 0, False, 0)

        need = int(_lib.load().lz_grid_ordered_workspace(M, D))
        shapes[name] = dict(D=D, C=C, L=L, atomic=atomic, ordered=ordered, fixed=fixed, need=need,
                            need_fixed=int(_lib.load().lz_grid_fixed_workspace(enc.embeddings.shape[0], C)))
    variants = [v for v in ("atomic", "ordered", "fixed") if a.only is None or v in a.only.split(",")]
    for s in shapes.values():                 # warm-up: allocations, the workspaces
        for v in variants:
            s[v]()
    torch.cuda.synchronize()
    res = {"rays": H * W, "samples": M, "rounds": a.rounds, "iters": a.iters}
    for name, s in shapes.items():
        times = {v: [] for v in variants}
        for _ in range(a.rounds):
            for k in times:
                times[k].append(timed(s[k], a.iters, a.limit))
        for k, v in times.items():
            res["%s_%s_ms" % (name, k)] = round(float(np.median(v)), 4)
        for num, den in (("ordered", "atomic"), ("fixed", "atomic"), ("fixed", "ordered")):
            if num in times and den in times:
                res["%s_%s_over_%s" % (name, num, den)] = round(res["%s_%s_ms" % (name, num)] / res["%s_%s_ms" % (name, den)], 3 if den == "ordered" else 2)
        res["%s_workspace_unchunked_bytes" % name] = s["need"]
        res["%s_workspace_used_bytes" % name] = min(s["need"], gridencoder.ORDERED_WORKSPACE_CAP)
        res["%s_fixed_workspace_bytes" % name] = s["need_fixed"]
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
