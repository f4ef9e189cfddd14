"""Training objective: the fused kernels (lzzx_nerf_amd/objective.py) against the same objective restated in torch (tests/objective_spec.py,
f32 on the GPU -- what a user of this library writes without the fused op).

    python tools/objective_bench.py [--steps K] [--rounds R] [--out profiles/objective_bench.json]

1. objective alone, forward + backward, at N = 65 536 and 262 144 rays; the jitter regulariser at M = 1 M and 6 M samples;
2. the `-O` training step set up like bench.py's cfg3 leg (tools/bench_legs.py train_bench: 65 536 random rays of the 512x512 frame,
   max_steps 192 and occupancy "ones" (bench.py's defaults), step-major march, FusedTriplaneTrainHead with f16 forward / backward and the recomputing arrangement, GradScaler(65536),
   fused Adam) once per objective: the leg's stand-in loss, the torch restatement, the fused objective.
Variants alternate within each round; every number is the median over rounds of per-round medians of device-event times per call / step.
Outputs are compared at the timed sizes (the fused and the torch losses agree to a few ulp of f32 sums)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import objective_spec as S  # noqa: E402
from lzzx_nerf_amd.objective import HeadObjective, jitter_regularizer  # noqa: E402


def timed(fn, k):
    """median device time of fn() over k calls (events around each call)"""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(k + 1)]
    ev[0].record()
    for i in range(k):
        fn()
        ev[i + 1].record()
    torch.cuda.synchronize()
    return float(np.median([ev[i].elapsed_time(ev[i + 1]) for i in range(k)]))


def alternate(variants, k, rounds):
    """{name: median over rounds of the per-round median ms}; variants run alternately, each warmed up first"""
    for fn in variants.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    res = {n: [] for n in variants}
    for _ in range(rounds):
        for n, fn in variants.items():
            res[n].append(timed(fn, k))
    return {n: round(float(np.median(v)), 4) for n, v in res.items()}


def objective_inputs(N, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    u = lambda *s: torch.rand(*s, device="cuda", generator=g)
    leaves = dict(image_raw=u(N, 3) * 1.2 - 0.1, ws=u(N), aud=u(N) * 4, eye=u(N) * 16, unc=u(N) * 3)
    leaves = {k: v.requires_grad_(True) for k, v in leaves.items()}
    return leaves, u(N, 3), u(N, 3), u(N) < 0.4


def bench_objective(N, k, rounds, step=96001):
    leaves, bg, target, face = objective_inputs(N)
    obj = HeadObjective(200000)
    sf = obj.step_factor(step)
    L = [leaves[n] for n in ("image_raw", "ws", "aud", "eye", "unc")]
    out = {}

    def fused():
        loss, _, _ = obj(*L, bg, target, face, step)
        torch.autograd.grad(loss, L)
        out["fused"] = loss

    def torch_():
        loss, _, _ = S.head_objective(*L, bg, target, face, sf, (True, True, True))
        torch.autograd.grad(loss, L)
        out["torch"] = loss

    ms = alternate({"torch": torch_, "fused": fused}, k, rounds)
    rel = abs(float(out["fused"].detach()) - float(out["torch"].detach())) / abs(float(out["torch"].detach()))
    return dict(N=N, ms_torch=ms["torch"], ms_fused=ms["fused"], speedup=round(ms["torch"] / ms["fused"], 2), loss_rel_diff=rel)


def bench_jitter(M, k, rounds, sf=0.5):
    g = torch.Generator(device="cuda").manual_seed(1)
    raw = [torch.rand(M, 1, device="cuda", generator=g) for _ in range(3)]
    reg = [(r + (torch.rand(M, 1, device="cuda", generator=g) - 0.5) * 1e-2).requires_grad_(True) for r in raw]
    out = {}

    def fused():
        loss = jitter_regularizer(raw, reg, sf, (True, True, True))
        torch.autograd.grad(loss, reg)
        out["fused"] = loss

    def torch_():
        loss = S.jitter(raw, reg, sf, (True, True, True))
        torch.autograd.grad(loss, reg)
        out["torch"] = loss

    ms = alternate({"torch": torch_, "fused": fused}, k, rounds)
    rel = abs(float(out["fused"].detach()) - float(out["torch"].detach())) / abs(float(out["torch"].detach()))
    return dict(M=M, ms_torch=ms["torch"], ms_fused=ms["fused"], speedup=round(ms["torch"] / ms["fused"], 2), loss_rel_diff=rel)


def bench_step(k, rounds, n_rays=65536, size=512, max_steps=192, step_no=96001):
    from lzzx_nerf_amd import raymarching as R
    from lzzx_nerf_amd.head_train import FusedTriplaneTrainHead
    from lzzx_nerf_amd.synthetic import load_golden, make_params, ones_bitfield, synthetic_camera
    from lzzx_nerf_amd.utils import frame_rays
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    golden = load_golden()
    P = make_params(golden)
    bits = dev(ones_bitfield())                     # bench.py --scene ones (its default)
    pose, intr = synthetic_camera(size, size)
    ro, rd = frame_rays(dev(pose), intr, size, size)
    g = torch.Generator(device="cuda").manual_seed(0)
    sel = torch.randperm(size * size, device="cuda", generator=g)[:n_rays]
    ro, rd = ro[sel].contiguous(), rd[sel].contiguous()
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
    obj = HeadObjective(200000)
    sf = obj.step_factor(step_no)
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
            if kind == "stand_in":     # tools/bench_legs.py train_bench
                loss = ((img + (1 - ws).unsqueeze(-1) - target) ** 2).mean() + 1e-4 * a0s.mean() + 1e-4 * a1s.mean() + 1e-3 * us.mean()
            elif kind == "torch":
                loss, _, _ = S.head_objective(img, ws, a0s, a1s, us, bg, target, face, sf, (True, True, True))
            else:
                loss, _, _ = obj(img, ws, a0s, a1s, us, bg, target, face, step_no)
            opt.zero_grad(set_to_none=True)
            scaler.scale(loss).backward()
            scaler.step(opt)
            scaler.update()
            losses[kind] = loss
        return step

    variants = {kind: make(kind) for kind in ("stand_in", "torch", "fused")}
    variants["stand_in"]()            # the start-up step that sizes the sample buffers (mean_count)
    torch.cuda.synchronize()
    ms = alternate(variants, k, rounds)
    return dict(rays=n_rays, frame=f"{size}x{size}", max_steps=max_steps, samples_per_step=int(ctr[0].item()),
                ms_step_stand_in=ms["stand_in"], ms_step_torch_objective=ms["torch"], ms_step_fused_objective=ms["fused"],
                saving_ms_per_step=round(ms["torch"] - ms["fused"], 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-step", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "objective_bench needs a GPU"
    t0 = time.time()
    res = dict(device=torch.cuda.get_device_name(0), steps=a.steps, rounds=a.rounds,
               objective=[bench_objective(N, a.steps, a.rounds) for N in (65536, 262144)],
               jitter=[bench_jitter(M, a.steps, a.rounds) for M in (1 << 20, 6_000_000)])
    if not a.skip_step:
        res["train_step_O"] = bench_step(a.steps, a.rounds)
    res["wall_s"] = round(time.time() - t0, 1)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
