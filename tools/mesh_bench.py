"""What mesh extraction on the device (csrc/lz_mesh.hip, lzzx_nerf_amd/mesh.py) costs, beside the only route there was before it: the
`density_field(...).cpu()` copy a CPU marching cubes needs before it can start.  ONE process, arrangements alternating within rounds:

    python tools/mesh_bench.py [--rounds 7] [--iters 5] [--res 256,512] [--kernel-stats CSV] [--out profiles/mesh_bench.json]

Per resolution R and field (an analytic sphere; the synthetic head's density_field cut at its 90th percentile):
  * count_scan: lz_mc_count (the count kernel and the scan kernel, one entry), emit: lz_mc_emit -- device events around `iters` calls;
  * whole_call: mesh.marching_cubes (allocations, both entries, the read-back of the two totals), wall clock behind a synchronise;
  * whole_call_to_host: the same plus vertices.cpu() and triangles.cpu();
  * copy_u_to_host: u.cpu() alone, the yardstick.
Medians over the rounds with min / max and every round; V, T, the workspace, the bytes each pass must move (u once, the 16-bit words,
the tile totals, the outputs) and what fraction of the 6.3 TB/s achievable HBM rate that is at the measured time.
--kernel-stats: the `rocprofv3 --kernel-trace --stats` CSV of a run of this tool (a run of its own), whose lz_k_mc_* rows split count
and scan; they are copied into the result as `kernel_trace`."""
import argparse
import csv
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lzzx_nerf_amd import _lib  # noqa: E402
from lzzx_nerf_amd._util import call, ptr, stream  # noqa: E402
from lzzx_nerf_amd.head import FusedTriplaneHead  # noqa: E402
from lzzx_nerf_amd.mesh import marching_cubes  # noqa: E402
from lzzx_nerf_amd.occupancy import density_field  # noqa: E402
from lzzx_nerf_amd.synthetic import load_golden, make_params  # noqa: E402

HBM_ACHIEVABLE = 6.3e12   # bytes / s, DESIGN 4
LZM_TILE = 256            # csrc/lz_mesh.hip


def events(f, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def wall(f, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def alternate(variants, rounds, iters):
    for f, _ in variants.values():
        for _ in range(2):
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(rounds):                  # every round times every variant once
        for k, (f, timer) in variants.items():
            ms[k].append(timer(f, iters))
    return {k: dict(median_ms=round(statistics.median(v), 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4), rounds_ms=[round(t, 4) for t in v])
            for k, v in ms.items()}


def case(u, thr, rounds, iters):
    R = u.shape[0]
    N = u.numel()
    lib = _lib.load()
    nbytes = lib.lz_mc_workspace(*u.shape)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=u.device)
    totals = torch.zeros(2, dtype=torch.int32, device=u.device)
    v, t = marching_cubes(u, thr)
    V, T = len(v), len(t)
    count = lambda: call("lz_mc_count", ptr(u), R, R, R, thr, ptr(ws), ptr(totals), stream())
    emit = lambda: call("lz_mc_emit", ptr(u), R, R, R, thr, ptr(ws), V, T, ptr(v), ptr(t), stream())
    count()

    def to_host():
        a, b = marching_cubes(u, thr)
        return a.cpu(), b.cpu()

    res = alternate({"count_scan": (count, events), "emit": (emit, events), "whole_call": (lambda: marching_cubes(u, thr), wall),
                     "whole_call_to_host": (to_host, wall), "copy_u_to_host": (lambda: u.cpu(), wall)}, rounds, iters)
    tiles = R * R * ((R + LZM_TILE - 1) // LZM_TILE)
    bytes_count = 4 * N + 2 * N + 8 * tiles + 2 * 8 * tiles            # u, the words, the tile totals and their scan
    bytes_emit = 4 * N + 16 * tiles + 12 * V + 12 * T + 3 * T * (2 + 16)  # u, the tile bases, the outputs, a word and two bases per corner
    res.update(resolution=R, nodes=N, threshold=thr, V=V, T=T, workspace_bytes=int(nbytes), tiles=tiles,
               bytes_count_scan=bytes_count, bytes_emit=bytes_emit,
               hbm_fraction_count_scan=round(bytes_count / (res["count_scan"]["median_ms"] * 1e-3) / HBM_ACHIEVABLE, 4),
               hbm_fraction_emit=round(bytes_emit / (res["emit"]["median_ms"] * 1e-3) / HBM_ACHIEVABLE, 4),
               peak_bytes_whole_call=int(4 * N + nbytes + 12 * V + 12 * T),
               device_to_host_faster_than_copy=bool(res["whole_call_to_host"]["median_ms"] < res["copy_u_to_host"]["median_ms"]))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--res", default="256,512")
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    dev = torch.device("cuda")
    golden = load_golden()
    params = {k: torch.from_numpy(v) for k, v in make_params(golden).items()}
    to = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)
    enc_a, eye = to(golden["net_enc_a"]), to(golden["net_eye"])
    head = FusedTriplaneHead(params, bound=1.0, precision="f32")
    res = dict(rounds=a.rounds, iters=a.iters, device=torch.cuda.get_device_name(0), hbm_achievable_bytes_per_s=HBM_ACHIEVABLE, cases={})
    for R in [int(r) for r in a.res.split(",")]:
        ax = torch.linspace(-1, 1, R, device=dev)
        x, y, z = torch.meshgrid(ax, ax, ax, indexing="ij")
        sphere = (0.7 - (x * x + y * y + z * z).sqrt()).contiguous()
        del x, y, z
        fields = {"sphere": (sphere, 0.0)}
        u = density_field(head, enc_a, eye, (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), R)
        fields["head"] = (u, float(torch.quantile(u.reshape(-1)[::max(1, u.numel() // (1 << 20))], 0.9)))   # a threshold that yields a surface
        for name, (f, thr) in fields.items():
            c = case(f, thr, a.rounds, a.iters)
            res["cases"]["%s_%d" % (name, R)] = c
            print(name, R, json.dumps({k: (v["median_ms"] if isinstance(v, dict) else v) for k, v in c.items()}), flush=True)
        del fields, sphere, u
        torch.cuda.empty_cache()
    if a.kernel_stats:
        with open(a.kernel_stats) as f:
            res["kernel_trace"] = [dict(name=r["Name"].split("(")[0], calls=int(r["Calls"]), average_ns=float(r["AverageNs"]), min_ns=int(r["MinNs"]),
                                        max_ns=int(r["MaxNs"])) for r in csv.DictReader(f) if "lz_k_mc_" in r["Name"]]
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
