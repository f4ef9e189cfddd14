"""Torso stage (train.py --torso): the fused training kernels (lzzx_nerf_amd.torso_train.FusedTorsoTrainNet) against the operator path
(TorsoTrainNet, an autograd graph over this repo's operators), reference torso configuration, ind_dim_torso 8.

    python tools/torso_train_bench.py [--steps K] [--rounds R] [--sizes 65536,262144] [--only step] [--table-grad fixed]
                                      [--out profiles/torso_train_bench.json]

At each N (65 536 = train.py's rays per step; 262 144 = the whole 512 x 512 frame):
  (a) TorsoTrainNet forward + backward        (b) FusedTorsoTrainNet forward + backward
  (c) a whole torso-stage step both ways: run_torso (2-D occupancy mask, masked forward_torso, background mix; for the operator path the
      reference's boolean-mask gather / scatter composed around TorsoTrainNet, renderer.py:572-631) -> TorsoObjective -> backward ->
      torch.optim.AdamW(betas=(0.0, 0.99), eps=1e-8).
Variants alternate within each round; each number is the median over rounds of per-round medians of device-event times per call.
`--only step` runs (c) alone, `--only step_fused` / `--only step_ops` one way of it (the rocprofv3 --kernel-trace --stats runs).
`--table-grad ordered|fixed` adds, to the same alternation (so the float-atomic fused path of the same run is the yardstick), the fused
net with that table_grad (`..._fused_..._<mode>`) and the operator path under gridencoder.set_table_grad(<mode>) (`..._ops_..._<mode>`);
with `--out` the numbers are merged into the file's results under `table_grad_<mode>`, the file's other entries staying as they are."""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as Fn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lzzx_nerf_amd import gridencoder  # noqa: E402
from lzzx_nerf_amd.objective import TorsoObjective  # noqa: E402
from lzzx_nerf_amd.torso_train import FusedTorsoTrainNet, TorsoTrainNet  # noqa: E402


def timed(fn, k):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(k + 1)]
    ev[0].record()
    for i in range(k):
        fn()
        ev[i + 1].record()
    torch.cuda.synchronize()
    return float(np.median([ev[i].elapsed_time(ev[i + 1]) for i in range(k)]))


def alternate(variants, k, rounds):
    res = {n: [] for n in variants}
    for fn in variants.values():   # warm-up
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for n, fn in variants.items():
            res[n].append(timed(fn, k))
    return {n: float(np.median(v)) for n, v in res.items()}


def setup(N, G=128):
    g = torch.Generator().manual_seed(0)
    torch.manual_seed(0)
    fused = FusedTorsoTrainNet(ind_dim_torso=8).cuda()
    ops = TorsoTrainNet(ind_dim_torso=8).cuda()
    ops.load_state_dict(fused.state_dict())
    ys, xs = torch.meshgrid(torch.linspace(-1, 1, 512), torch.linspace(-1, 1, 512), indexing="ij")
    frame = torch.stack([xs.reshape(-1), ys.reshape(-1)], 1)
    xy = (frame if N >= frame.shape[0] else frame[torch.randperm(frame.shape[0], generator=g)[:N]]).cuda().contiguous()
    c = (torch.randn(1, 8, generator=g) * 0.1).cuda()
    pose = torch.eye(4)
    pose[:3, 3] = torch.tensor([0.05, -0.02, 3.3])
    poses = pose[None].cuda()
    yy, xx = torch.meshgrid(torch.arange(G), torch.arange(G), indexing="ij")
    grid = torch.exp(-(((xx - 64) / 30.0) ** 2 + ((yy - 80) / 40.0) ** 2)).float().reshape(-1).cuda()   # a torso-like occupancy blob
    thresh = torch.tensor([0.01], device="cuda")
    target = torch.rand(xy.shape[0], 3, generator=g).cuda()
    gout = [torch.randn(xy.shape[0], k, generator=g).cuda() for k in (1, 3, 2)]
    return dict(fused=fused, ops=ops, xy=xy, c=c, poses=poses, grid=grid, G=G, thresh=thresh, target=target, gout=gout)


def run_torso_ops(net, s):
    """renderer.py:572-631 around TorsoTrainNet: grid_sample mask, mask.any() (a host synchronisation), gather, forward, scatter, mix"""
    xy, G, N = s["xy"], s["G"], s["xy"].shape[0]
    occ = Fn.grid_sample(s["grid"].view(1, 1, G, G), xy.view(1, -1, 1, 2), align_corners=True).view(-1)
    mask = occ > s["thresh"]
    alpha, color = torch.zeros(N, 1, device=xy.device), torch.zeros(N, 3, device=xy.device)
    if mask.any():
        a, col, _ = net(xy[mask], s["poses"], s["c"])
        alpha[mask], color[mask] = a, col
    return color * alpha + 1 * (1 - alpha)


def make(s, table_grad="atomic"):
    fused, ops = s["fused"], s["ops"]
    ga, gc, gd = s["gout"]
    obj = TorsoObjective()
    opt_f = torch.optim.AdamW(fused.parameters(), lr=1e-4, betas=(0.0, 0.99), eps=1e-8)
    opt_o = torch.optim.AdamW(ops.parameters(), lr=1e-4, betas=(0.0, 0.99), eps=1e-8)

    def fwd_bwd(net):
        def f():
            net.zero_grad(set_to_none=True)
            a, col, d = net(s["xy"], s["poses"], s["c"])
            ((a * ga).sum() + (col * gc).sum() + (d * gd).sum()).backward()
        return f

    def step_fused():
        out = fused.run_torso(s["xy"], s["poses"], s["c"], 1, s["grid"], s["thresh"])
        loss, _ = obj(out["torso_color"], s["target"], fused.anchor_points)
        opt_f.zero_grad(set_to_none=True)
        loss.backward()
        opt_f.step()

    def step_ops():
        loss, _ = obj(run_torso_ops(ops, s), s["target"], ops.anchor_points)
        opt_o.zero_grad(set_to_none=True)
        loss.backward()
        opt_o.step()

    pairs, steps = {"a_ops_fwd_bwd": fwd_bwd(ops), "b_fused_fwd_bwd": fwd_bwd(fused)}, {"c_step_ops": step_ops, "c_step_fused": step_fused}
    if table_grad != "atomic":
        # the same fused net with the attribute switched for the call (it is read at every backward); the operator path under the module
        # default of the same name.  Both restore "atomic", so the variants they alternate with are the parent's.
        def in_mode(fn, on_fused):
            def f():
                if on_fused:
                    fused.table_grad = table_grad
                else:
                    gridencoder.set_table_grad(table_grad)
                try:
                    fn()
                finally:
                    fused.table_grad = "atomic"
                    gridencoder.set_table_grad("atomic")
            return f

        pairs.update({"a_ops_fwd_bwd_" + table_grad: in_mode(pairs["a_ops_fwd_bwd"], False),
                      "b_fused_fwd_bwd_" + table_grad: in_mode(pairs["b_fused_fwd_bwd"], True)})
        steps.update({"c_step_ops_" + table_grad: in_mode(step_ops, False), "c_step_fused_" + table_grad: in_mode(step_fused, True)})
    return pairs, steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sizes", default="65536,262144")
    ap.add_argument("--only", default="")
    ap.add_argument("--table-grad", default="atomic", choices=["atomic", "ordered", "fixed"])
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0), "steps": a.steps, "rounds": a.rounds, "ind_dim_torso": 8, "results": {}}
    for N in [int(v) for v in a.sizes.split(",")]:
        s = setup(N)
        with torch.no_grad():
            frac = float((Fn.grid_sample(s["grid"].view(1, 1, 128, 128), s["xy"].view(1, -1, 1, 2), align_corners=True).view(-1) > 0.01).float().mean())
        pairs, steps = make(s, a.table_grad)
        r = {"masked_fraction": frac}
        if not a.only.startswith("step"):
            r.update(alternate(pairs, a.steps, a.rounds))
        if a.only in ("step_fused", "step_ops"):
            name = "c_" + a.only + ("_" + a.table_grad if a.table_grad != "atomic" else "")
            steps = {name: steps[name]}
        r.update(alternate(steps, a.steps, a.rounds))
        out["results"][str(N)] = {k: (round(v, 4) if isinstance(v, float) else v) for k, v in r.items()}
        print(N, out["results"][str(N)], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        doc = out
        if a.table_grad != "atomic" and os.path.exists(a.out):   # merged into the float-atomic run's file
            with open(a.out) as f:
                doc = json.load(f)
            doc["table_grad_" + a.table_grad] = {k: out[k] for k in ("device", "steps", "rounds", "results")}
        elif a.table_grad != "atomic":
            doc = {"table_grad_" + a.table_grad: out}
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
