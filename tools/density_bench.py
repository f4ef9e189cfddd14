"""What NeRFNetwork.density on the fused head (csrc/lz_density.hip) buys against running the whole head and dropping everything but
sigma, in ONE process, alternating rounds:

    python tools/density_bench.py [--rounds 7] [--iters 5] [--out profiles/density_bench.json]

  * occupancy.update_density_grid at G = 128, bound = 1 with density_only off (lz_density_grid_points + a dummy direction buffer +
    lz_triplane_head_forward: the comparison base, kernels this tool's subject does not touch) and on (one lz_triplane_density_lattice
    launch that makes the cells' points itself and writes sigma alone), on the f32 head and on the f16 head;
  * head.density() against head.forward() at 2^21 rows, both precisions, and density(geo_feat=True).

Times are device events around `iters` calls (a synchronise behind them), medians over the rounds; each case records its rounds and the
spread between them, which is what a difference has to clear.  Before timing, the two arrangements of each case are compared on the same
inputs: grid, bitfield and sigma bit for bit."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lzzx_nerf_amd.head import FusedTriplaneHead  # noqa: E402
from lzzx_nerf_amd.occupancy import update_density_grid  # noqa: E402
from lzzx_nerf_amd.synthetic import load_golden, make_params  # noqa: E402

G, ROWS = 128, 1 << 21


def timed(f, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def alternate(variants, rounds, iters):
    for f in variants.values():              # warm every shape of the timed window
        for _ in range(2):
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(rounds):                  # every round times every variant once
        for k, f in variants.items():
            ms[k].append(timed(f, iters))
    return {k: dict(median_ms=round(statistics.median(v), 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4), rounds_ms=[round(t, 4) for t in v])
            for k, v in ms.items()}


def compare(case, base, new):
    b, n = case[base], case[new]
    case["%s_over_%s" % (base, new)] = round(b["median_ms"] / n["median_ms"], 3)
    case["spread_between_rounds_ms"] = round(max(v["max_ms"] - v["min_ms"] for v in case.values() if isinstance(v, dict)), 4)
    case["difference_ms"] = round(b["median_ms"] - n["median_ms"], 4)
    case["difference_clears_the_spread"] = bool(abs(case["difference_ms"]) > case["spread_between_rounds_ms"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "density_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    dev = torch.device("cuda")
    golden = load_golden()
    params = {k: torch.from_numpy(v) for k, v in make_params(golden).items()}
    to = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)
    enc_a, eye = to(golden["net_enc_a"]), to(golden["net_eye"])
    gen = torch.Generator(device=dev).manual_seed(0)
    noise = torch.rand(1, G ** 3, 3, device=dev, generator=gen)
    xyz = torch.rand(ROWS, 3, device=dev, generator=gen) * 2 - 1
    dirs = torch.zeros(ROWS, 3, device=dev)
    dirs[:, 2] = 1.0
    res = dict(rounds=a.rounds, iters=a.iters, device=torch.cuda.get_device_name(0), grid_size=G, bound=1.0, rows=ROWS, update_density_grid={},
               density_vs_forward={})
    for prec in ("f32", "f16"):
        head = FusedTriplaneHead(params, bound=1.0, precision=prec)
        grid0 = torch.rand(1, G ** 3, device=dev, generator=gen)

        def update(only, grid=None, bits=None):
            grid = grid0.clone() if grid is None else grid
            bits = torch.zeros(G ** 3 // 8, dtype=torch.uint8, device=dev) if bits is None else bits
            return (grid, bits) + update_density_grid(head, grid, bits, enc_a, eye, bound=1.0, noise=noise, density_only=only)
        off, on = update(False), update(True)
        same = all(torch.equal(x, y) for x, y in zip(off, on))
        g_off, b_off, g_on, b_on = off[0], off[1], on[0], on[1]      # timed in place: the EMA's values do not change the work
        case = alternate({"density_only_off": lambda: update(False, g_off, b_off), "density_only_on": lambda: update(True, g_on, b_on)}, a.rounds, a.iters)
        case["grid_bitfield_stats_bits_equal"] = same
        compare(case, "density_only_off", "density_only_on")
        res["update_density_grid"][prec] = case
        print("update_density_grid", prec, json.dumps({k: (v["median_ms"] if isinstance(v, dict) else v) for k, v in case.items()}), flush=True)

        sig = head.forward(xyz, dirs, enc_a, None, eye)[0]
        same = torch.equal(head.density(xyz, enc_a, eye)["sigma"], sig) and torch.equal(head.density(xyz, enc_a, eye, geo_feat=True)["sigma"], sig)
        case = alternate({"forward": lambda: head.forward(xyz, dirs, enc_a, None, eye), "density": lambda: head.density(xyz, enc_a, eye),
                          "density_geo_feat": lambda: head.density(xyz, enc_a, eye, geo_feat=True)}, a.rounds, a.iters)
        case["sigma_bits_equal"] = same
        compare(case, "forward", "density")
        case["forward_over_density_geo_feat"] = round(case["forward"]["median_ms"] / case["density_geo_feat"]["median_ms"], 3)
        res["density_vs_forward"][prec] = case
        print("density_vs_forward", prec, json.dumps({k: (v["median_ms"] if isinstance(v, dict) else v) for k, v in case.items()}), flush=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
