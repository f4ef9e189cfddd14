"""Perceptual loss: FusedLPIPS (lzzx_nerf_amd/perceptual.py) against the same definition restated in torch (tests/lpips_checker.py, f32 on
the GPU: library convolutions and autograd -- what the `lpips` package runs), forward plus backward, in the same run.

    python tools/lpips_bench.py [--steps K] [--rounds R] [--out profiles/lpips_bench.json]

1. LPIPS alone at 32^2, 64^2, 96^2, 128^2 with P = 1 and 32^2 with P = 16, on the seeded stand-in weights;
2. the `-O` training step of tools/objective_bench.py (cfg3: FusedTriplaneTrainHead f16 / recompute, GradScaler, fused Adam) on the 4096
   rays of a 64 x 64 rectangle, without and with the lips term (HeadObjective(finetune_lips=True, lpips=...)(..., rect=...)).
Variants alternate within each round; every number is the median over rounds of per-round medians of device-event times per call.
Launch counts: ours is the kernels' own (nine forward, eight backward); torch's is the number of aten operator calls of one forward plus
backward, counted on the host with a dispatch mode -- each is at least one launch."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
from torch.utils._python_dispatch import TorchDispatchMode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import lpips_checker as K  # noqa: E402
from objective_bench import alternate  # noqa: E402
from lzzx_nerf_amd.objective import HeadObjective  # noqa: E402
from lzzx_nerf_amd.perceptual import FusedLPIPS  # noqa: E402
from lzzx_nerf_amd.synthetic import lpips_alex_state  # noqa: E402


class _CountOps(TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.n = 0

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        name = func.overloadpacket.__name__
        if name not in ("view", "detach", "alias", "expand", "permute", "reshape", "_unsafe_view", "t", "transpose", "unsqueeze", "squeeze", "as_strided"):
            self.n += 1
        return func(*args, **(kwargs or {}))


def bench_lpips(net, w, P, H, W, k, rounds):
    g = torch.Generator(device="cuda").manual_seed(H * 1000 + P)
    target = torch.rand(P, 3, H, W, device="cuda", generator=g) * 2 - 1
    pred = (target + 0.25 * torch.randn(P, 3, H, W, device="cuda", generator=g)).clamp(-1, 1).requires_grad_(True)
    out = {}

    def fused():
        v = net(pred, target)
        out["fused"] = (v, torch.autograd.grad(v.sum(), pred)[0])

    def torch_():
        v = K.lpips(w, pred, target)
        out["torch"] = (v, torch.autograd.grad(v.sum(), pred)[0])

    ms = alternate({"torch": torch_, "fused": fused}, k, rounds)
    with _CountOps() as c:
        torch_()
    (vf, gf), (vt, gt) = [(v.detach(), g) for v, g in (out["fused"], out["torch"])]
    return dict(P=P, H=H, W=W, ms_torch=ms["torch"], ms_fused=ms["fused"], speedup=round(ms["torch"] / ms["fused"], 2),
                launches_fused=net.FORWARD_LAUNCHES + net.BACKWARD_LAUNCHES, aten_ops_torch=c.n,
                value_rel_diff=float(((vf - vt).abs() / vt.abs()).max()), grad_rel_diff=float((gf - gt).abs().max() / gt.abs().max()))


def bench_step(net_lp, k, rounds, size=512, side=64, max_steps=192, step_no=96001):
    from lzzx_nerf_amd import raymarching as R
    from lzzx_nerf_amd.head_train import FusedTriplaneTrainHead
    from lzzx_nerf_amd.synthetic import load_golden, make_params, ones_bitfield, synthetic_camera
    from lzzx_nerf_amd.utils import frame_rays
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    golden = load_golden()
    P = make_params(golden)
    bits = dev(ones_bitfield())
    pose, intr = synthetic_camera(size, size)
    ro, rd = frame_rays(dev(pose), intr, size, size)
    lo = (size - side) // 2
    rect = (lo, lo + side, lo, lo + side)
    idx = (torch.arange(lo, lo + side, device="cuda").view(-1, 1) * size + torch.arange(lo, lo + side, device="cuda").view(1, -1)).reshape(-1)
    ro, rd = ro[idx].contiguous(), rd[idx].contiguous()
    n_rays = side * side
    g = torch.Generator(device="cuda").manual_seed(0)
    target = torch.rand(n_rays, 3, device="cuda", generator=g)
    bg = torch.rand(n_rays, 3, device="cuda", generator=g)
    face = torch.rand(n_rays, device="cuda", generator=g) < 0.4
    enc_a, ind, eye = dev(golden["net_enc_a"]), dev(golden["net_ind"]), dev(golden["net_eye"])
    aabb = dev(np.array([-1, -0.5, -1, 1, 0.5, 1], np.float32))
    net = FusedTriplaneTrainHead({k_: torch.from_numpy(v) for k_, v in P.items()}, bound=1.0, record_dtype="f16", forward_dtype="f16",
                                 backward_dtype="f16", recompute_mlp=True).cuda()
    opt = torch.optim.Adam(net.parameters(), lr=1e-3, eps=1e-15, fused=True)
    scaler = torch.amp.GradScaler("cuda", init_scale=65536.0)
    ctr = torch.zeros(2, dtype=torch.int32, device="cuda")
    mean_count = [-1]
    obj = HeadObjective(200000, unc_loss=False, finetune_lips=True, lpips=net_lp)      # the reference's arrangement while it flips finetune_lips
    losses = {}

    def make(kind):
        def step():
            nears, fars = R.near_far_from_aabb(ro, rd, aabb, 0.05)
            ctr.zero_()
            xyzs, dirs, deltas, rays = R.march_rays_train(ro, rd, 1.0, bits, 1, 128, nears, fars, ctr, mean_count[0], True, 128,
                                                          mean_count[0] <= 0, 1 / 256, max_steps, layout="step")
            if mean_count[0] <= 0:
                mean_count[0] = int(xyzs.shape[0]) + n_rays // 64
            sigma, rgb, a0, a1, unc = net(xyzs, dirs, enc_a, ind, eye)
            a0, a1, unc = a0.squeeze(-1), a1.squeeze(-1), unc.squeeze(-1)
            ws, a0s, a1s, us, dep, img = R.composite_rays_train_triplane(sigma, rgb, a0, a1, unc, deltas, rays)
            loss, _, terms = obj(img, ws, a0s, a1s, us, bg, target, face, step_no, rect=rect if kind == "lips" else None)
            opt.zero_grad(set_to_none=True)
            scaler.scale(loss).backward()
            scaler.step(opt)
            scaler.update()
            losses[kind] = terms
        return step

    variants = {kind: make(kind) for kind in ("plain", "lips")}
    variants["plain"]()            # the start-up step that sizes the sample buffers (mean_count)
    torch.cuda.synchronize()
    ms = alternate(variants, k, rounds)
    return dict(rays=n_rays, rect=f"{side}x{side}", frame=f"{size}x{size}", max_steps=max_steps, samples_per_step=int(ctr[0].item()),
                ms_step_without_lips=ms["plain"], ms_step_with_lips=ms["lips"], lips_ms_per_step=round(ms["lips"] - ms["plain"], 4),
                lips_term=float(losses["lips"][6]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-step", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "lpips_bench needs a GPU"
    t0 = time.time()
    sd = lpips_alex_state(0)
    net = FusedLPIPS(sd)
    w = {k: ([t.cuda() for t in v] if isinstance(v, list) else v.cuda()) for k, v in K.weights(sd, torch.float32).items()}
    res = dict(device=torch.cuda.get_device_name(0), steps=a.steps, rounds=a.rounds, lpips=[])
    for P, H, W in ((1, 32, 32), (1, 64, 64), (1, 96, 96), (1, 128, 128), (16, 32, 32)):
        res["lpips"].append(bench_lpips(net, w, P, H, W, a.steps, a.rounds))
        print(res["lpips"][-1], file=sys.stderr, flush=True)
    if not a.skip_step:
        res["train_step_O_lips"] = bench_step(net, a.steps, a.rounds)
    res["wall_s"] = round(time.time() - t0, 1)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
