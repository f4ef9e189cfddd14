"""The three-plane encoder (gridencoder.TriplaneEncoder) against the path it replaces -- three GridEncoders and a torch.cat, the reference's
NeRFNetwork.encode_x (network.py:208-223) on this package's operators -- in ONE process, alternating rounds:

    python tools/triplane_encoder_bench.py [--rounds 7] [--iters 10] [--pmc-summary FILE] [--out profiles/triplane_encoder_bench.json]
    rocprofv3 --pmc TCP_TCC_WRITE_REQ_sum ... -- python tools/triplane_encoder_bench.py --pmc-run      (a counter run of its own: no timing)

Forward, and forward + backward (table gradients; xyz carries none, as in training), at B = 2^20 and B = 5 954 764 (the cfg3 step's
sample count), sample positions in march order (ray-major: consecutive rows are consecutive steps of one ray).  The yardstick is the
operator path of the same run.  --pmc-summary: tools/summarize_pmc.py's file over the --pmc-run, whose store requests are reported
beside the times."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lzzx_nerf_amd import gridencoder  # noqa: E402
from lzzx_nerf_amd.gridencoder import GridEncoder, TriplaneEncoder  # noqa: E402

SIZES = (1 << 20, 5954764)
PMC_B = 1 << 24       # the batch the stand-alone plane encoder's 151 M write requests were counted at (tools/profile_plane.sh)
PLANE_WRITE_REQ_2P24 = 151e6


def march_rows(B, device):
    """B sample positions in [-1, 1]^3 in march_rays_train order: the 256 x 256 synthetic camera's rays, ray-major, as many consecutive
    steps per ray as B needs (128 for the cfg3 count)"""
    from lzzx_nerf_amd.synthetic import synthetic_camera
    from lzzx_nerf_amd.utils import frame_rays
    pose, intr = synthetic_camera(256, 256)
    ro, rd = frame_rays(torch.from_numpy(pose).to(device), intr, 256, 256)
    steps = -(-B // ro.shape[0])
    t = torch.linspace(2.35, 4.35, max(steps, 2), device=device)[:steps]
    x = (ro[:, None, :] + rd[:, None, :] * t[None, :, None]).clamp(-1, 1).reshape(-1, 3)
    return x[:B].contiguous()


def make(device):
    g = torch.Generator(device=device).manual_seed(0)
    encs = []
    for _ in range(3):
        e = GridEncoder(input_dim=2, num_levels=12, level_dim=1, base_resolution=64, log2_hashmap_size=14, desired_resolution=512).to(device)
        e.embeddings.data.uniform_(-1, 1, generator=g)
        encs.append(e)
    return encs, TriplaneEncoder(*encs)


def three(encs, x):
    return torch.cat([encs[0](x[:, :2], bound=1), encs[1](x[:, 1:], bound=1), encs[2](x[:, [0, 2]], bound=1)], -1)


def timed(f, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--pmc-run", action="store_true")
    ap.add_argument("--pmc-summary", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "triplane_encoder_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    dev = torch.device("cuda")
    encs, tri = make(dev)

    if a.pmc_run:   # two launches each of the fused forward and of ONE plane's stand-alone forward, nothing else
        x = torch.rand(PMC_B, 3, device=dev, generator=torch.Generator(device=dev).manual_seed(1)) * 2 - 1
        with torch.no_grad():
            for _ in range(2):
                tri(x, bound=1)
                encs[0](x[:, :2].contiguous(), bound=1)
        torch.cuda.synchronize()
        return

    assert gridencoder.table_grad() == "atomic"
    res = dict(rounds=a.rounds, iters=a.iters, order="march (ray-major rows of the 256 x 256 synthetic camera)", sizes={})
    for B in SIZES:
        x = march_rows(B, dev)
        up = torch.randn(B, 36, device=dev, generator=torch.Generator(device=dev).manual_seed(2))
        with torch.no_grad():
            same = torch.equal(tri(x, bound=1), three(encs, x))

        def fwd(f):
            def run():
                with torch.no_grad():
                    f()
            return run

        def fwd_bwd(f):
            def run():
                for e in encs:
                    e.embeddings.grad = None
                f().backward(up)
            return run

        variants = {"fused_forward": fwd(lambda: tri(x, bound=1)), "three_forward": fwd(lambda: three(encs, x)),
                    "fused_forward_backward": fwd_bwd(lambda: tri(x, bound=1)), "three_forward_backward": fwd_bwd(lambda: three(encs, x))}
        for f in variants.values():          # warm every shape of the timed window
            for _ in range(3):
                f()
        torch.cuda.synchronize()
        ms = {k: [] for k in variants}
        for _ in range(a.rounds):            # alternating: every round times every variant once
            for k, f in variants.items():
                ms[k].append(timed(f, a.iters))
        case = dict(forward_bits_equal=same)
        for k, v in ms.items():
            case[k] = dict(median_ms=round(statistics.median(v), 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4),
                           rounds_ms=[round(t, 4) for t in v])
        for what in ("forward", "forward_backward"):
            f_, t_ = case["fused_" + what], case["three_" + what]
            case["three_over_fused_" + what] = round(t_["median_ms"] / f_["median_ms"], 3)
            case["spread_between_rounds_ms_" + what] = round(max(f_["max_ms"] - f_["min_ms"], t_["max_ms"] - t_["min_ms"]), 4)
        res["sizes"][str(B)] = case
        print(B, json.dumps({k: (v["median_ms"] if isinstance(v, dict) else v) for k, v in case.items()}), flush=True)
        del x, up
    if a.pmc_summary:
        pmc = json.load(open(a.pmc_summary))
        stores = {}
        for counter in ("TCP_TCC_WRITE_REQ_sum", "TCP_TCC_READ_REQ_sum", "TCP_TOTAL_ACCESSES_sum"):
            for k, v in pmc.get(counter, {}).items():
                if "lz_k_triplane_encode" in k or "lz_k_grid_forward" in k:
                    stores.setdefault(counter, {})[k] = dict(per_launch=v["avg_per_launch"], launches=v["launches"])
        res["counters"] = dict(batch=PMC_B, source="rocprofv3 --pmc, a run of its own (--pmc-run): uniform random samples", per_kernel=stores,
                               plane_encoder_write_requests_recorded=PLANE_WRITE_REQ_2P24)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
