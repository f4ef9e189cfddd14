"""Fused hash-grid NeRF training (ngp_train.FusedHashgridTrainNeRF) against the operator path (synthetic.GenericHashgridNeRF.net under
autograd) on the same weights, BASELINE cfg2 batch: 256 x 256 rays, march_rays_train with max_steps 128.

    net    forward + backward of the network over the marched samples (fixed inputs)
    step   march -> net -> composite_rays_train -> MSE -> backward -> Adam

The variants alternate; each round times `--iters` repetitions of each leg per variant; the median over `--rounds` rounds is printed as
one JSON line.  Launch counts and per-kernel time: run under `rocprofv3 --kernel-trace --stats -- python tools/ngp_train_bench.py --iters 1
--rounds 1`."""
import argparse
import copy
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from lzzx_nerf_amd import raymarching as R  # noqa: E402
from lzzx_nerf_amd.ngp_train import FusedHashgridTrainNeRF  # noqa: E402
from lzzx_nerf_amd.synthetic import GenericHashgridNeRF, ellipsoid_bitfield_device, synthetic_camera  # noqa: E402
from lzzx_nerf_amd.utils import frame_rays  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    H = W = a.size
    pose, intr = synthetic_camera(H, W)
    ro, rd = frame_rays(torch.from_numpy(pose).cuda(), intr, H, W)
    bits, _ = ellipsoid_bitfield_device("cuda")
    aabb = torch.tensor([-1, -1, -1, 1, 1, 1], dtype=torch.float32, device="cuda")
    nears, fars = R.near_far_from_aabb(ro, rd, aabb, 0.05)
    target = torch.rand(H * W, 3, generator=torch.Generator().manual_seed(5)).cuda()
    g = GenericHashgridNeRF("cuda", seed=3)
    f = FusedHashgridTrainNeRF(copy.deepcopy(g.enc), copy.deepcopy(g.sigma_net), copy.deepcopy(g.color_net)).cuda()
    variants = {"operator": (lambda x, d: g.net(x, d, 1.0), [g.enc.embeddings] + [m.net[i].weight for m in (g.sigma_net, g.color_net) for i in (0, 1)]),
                "fused": (lambda x, d: f(x, d, 1.0), list(f.parameters()))}
    opts = {k: torch.optim.Adam(p, lr=1e-2, betas=(0.9, 0.99), eps=1e-15) for k, (_, p) in variants.items()}

    def march():
        ctr = torch.zeros(2, dtype=torch.int32, device="cuda")
        return R.march_rays_train(ro, rd, 1.0, bits, 1, 128, nears, fars, ctr, -1, False, 128, True, 1 / 256, 128)

    xyzs, dirs, deltas, rays = march()
    xyzs, dirs = xyzs.detach().contiguous(), dirs.detach().contiguous()
    M = xyzs.shape[0]
    gs, gr = torch.randn(M, device="cuda"), torch.randn(M, 3, device="cuda")

    def leg_net(k):
        fn, params = variants[k]
        for p in params:
            p.grad = None
        s, c = fn(xyzs, dirs)
        torch.autograd.backward([s, c], [gs, gr])

    def leg_step(k):
        fn, params = variants[k]
        x, d, dl, r = march()
        s, c = fn(x.detach().contiguous(), d.detach().contiguous())
        ws, _, _, img = R.composite_rays_train(s, c, torch.zeros_like(s), dl, r)
        loss = ((img + (1 - ws)[:, None] - target) ** 2).mean()
        opts[k].zero_grad(set_to_none=True)
        loss.backward()
        opts[k].step()

    legs = {"net": leg_net, "step": leg_step}
    for k in variants:                       # warm-up: allocations, workspaces, the constant tables
        for fn in legs.values():
            fn(k)
    torch.cuda.synchronize()
    times = {(k, l): [] for k in variants for l in legs}
    for _ in range(a.rounds):
        for l, fn in legs.items():
            for k in variants:
                ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                ev0.record()
                for _ in range(a.iters):
                    fn(k)
                ev1.record()
                ev1.synchronize()
                times[(k, l)].append(ev0.elapsed_time(ev1) / a.iters)
    res = {"rays": H * W, "samples": M, "rounds": a.rounds, "iters": a.iters}
    for (k, l), v in times.items():
        res["%s_%s_ms" % (l, k)] = round(float(np.median(v)), 4)
    for l in legs:
        res["%s_speedup" % l] = round(res["%s_operator_ms" % l] / res["%s_fused_ms" % l], 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
