#!/usr/bin/env python3
"""BASELINE cfg2 alone (256 x 256 rays, max_steps 128, all-ones occupancy, hash-grid NeRF): the fused path (lzzx_nerf_amd/ngp.py) under a
few schedules, next to the operator-API device loop.  tools/cfg2_bench.py [f32|f16|autocast] [--ref] [B,C ...]
    f32       f32 tables, f32 head
    f16       half tables, f32 head (half_tables=True: the bench leg cfg2_fused_f16_ms)
    autocast  half tables, half head (precision="f16": the reference's torch-autocast arithmetic)
  --mode loop|fused|both   HashgridRenderer's mode (default loop; fused: csrc/lz_ngp_frame.hip needs n_step_cap 8).  both: loop and
                           fused ALTERNATED, --rounds times each (default 2), every timing listed: the same-box comparison of DESIGN 4.5
  --max-steps K            (default 128)      --size S   an S x S frame (default 256; 64 = a tile)      --cap reference|per_ray
  --steps-per-pass LIST    the fused mode at each steps_per_pass of LIST (1,2,4,8,16; 0 = auto, reported with the S it chose; "entry" = the
                           S = 1 kernels through lz_ngp_frame_render, the entry without the argument), with --loops also the loop under
                           (1, 8) and (8, 8): all configurations ALTERNATED in one process, --rounds times each (default 3), every timing
                           listed.  --size and --max-steps may be comma lists here; --out FILE writes the JSON there as well.  The sweep
                           behind the auto rule (csrc/lz_ngp_frame_spp.hip): profiles/cfg2_spp_sweep.json
  --clip                   the fused mode with clip_to_occupancy off and on, ALTERNATED in one process, --rounds times each (default 3),
                           every timing listed, on --occupancy ones (default) or ellipsoid (synthetic.ellipsoid_bitfield_device); --size
                           and --max-steps may be comma lists, --steps-per-pass one value (default 1), --out FILE as above.  Per cell also
                           `within`: clip on's mean exceeds clip off's by no more than clip off's own max - min (the A/B rule of DESIGN 4.4)
                           and `same`: the two frames are equal bit for bit.  profiles/cfg2_clip_bench.json"""
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
spp_list = [x if x == "entry" else int(x) for x in _opt("--steps-per-pass", "").split(",") if x]
sizes, steps_list = [int(x) for x in str(_opt("--size", 256)).split(",")], [int(x) for x in str(_opt("--max-steps", 128)).split(",")]
max_steps, size, rounds = steps_list[0], sizes[0], int(_opt("--rounds", 3 if spp_list or "--clip" in sys.argv else 2))
mode = sys.argv[1] if len(sys.argv) > 1 and sys.argv[1] in ("f32", "f16", "autocast") else "f32"
half = mode in ("f16", "autocast")
dev = torch.device("cuda", 0)


def rays(n):
    pose, intr = synthetic_camera(n, n)
    o, d = frame_rays(torch.from_numpy(np.ascontiguousarray(pose)).to(dev), intr, n, n)
    return o.reshape(-1, 3).contiguous(), d.reshape(-1, 3).contiguous()


ro, rd = rays(size)
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


class EntryRenderer(HashgridRenderer):
    """the fused mode through lz_ngp_frame_render, the entry without steps_per_pass (the S = 1 kernels): what the renderer called before
    lz_ngp_frame_render_spp existed"""

    def _render_fused(self, *a):
        import lzzx_nerf_amd.ngp as M
        real = M.call
        # (f, no options, steps_per_pass, timing, stream) -> (f, timing, stream)
        M.call = lambda name, *args: real("lz_ngp_frame_render", args[0], *args[3:]) if name == "lz_ngp_frame_render_opts" else real(name, *args)
        try:
            return super()._render_fused(*a)
        finally:
            M.call = real


def spp_sweep():
    """{size: {max_steps: {configuration: {ms: [one per round], S, samples, rows}}}}; a timing is the mean frame time of a window of at
    least 0.1 s (at least 10 frames) behind a warm-up, host clock around a device synchronise"""
    res = {}
    for n in sizes:
        o, d = rays(n)
        for ms_cap in steps_list:
            cfgs = {}
            for s in spp_list:
                cls, kw = (EntryRenderer, {}) if s == "entry" else (HashgridRenderer, dict(steps_per_pass=s))
                cfgs["entry" if s == "entry" else ("auto" if s == 0 else "S%d" % s)] = cls(net, bits, bound=1.0, aabb=aabb, mode="fused", cap=cap, **kw)
            if "--loops" in sys.argv:
                for b, c in ((1, 8), (8, 8)):
                    cfgs["loop_%dx%d" % (b, c)] = HashgridRenderer(net, bits, bound=1.0, aabb=aabb, budget_factor=b, n_step_cap=c)
            cell = {k: dict(ms=[]) for k in cfgs}
            for _ in range(rounds):
                for k, r in cfgs.items():
                    f = lambda: r.render(o, d, max_steps=ms_cap)
                    est, _o = timed(f, 5)
                    t, got = timed(f, max(10, min(2000, int(100.0 / max(est, 1e-3)))))
                    st = got["state"].cpu().numpy()
                    cell[k]["ms"].append(round(t, 4))
                    cell[k].update(samples=int(st[5]), rows=int(st[72]))
                    if r.mode == "fused":
                        cell[k]["S"] = r.last_steps_per_pass
            res.setdefault(str(n), {})[str(ms_cap)] = cell
            del cfgs
    return res


def clip_sweep():
    """{size: {max_steps: {"off" | "on": {ms: [one per round], samples, rows}, within, same}}}; timings as spp_sweep's"""
    res = {}
    S = spp_list[0] if spp_list else 1
    for n in sizes:
        o, d = rays(n)
        for ms_cap in steps_list:
            cfgs = {k: HashgridRenderer(net, clip_bits, bound=1.0, aabb=aabb, mode="fused", cap=cap, steps_per_pass=S, clip_to_occupancy=k == "on")
                    for k in ("off", "on")}
            cell = {k: dict(ms=[]) for k in cfgs}
            frames = {}
            for _ in range(rounds):
                for k, r in cfgs.items():
                    f = lambda: r.render(o, d, max_steps=ms_cap)
                    est, _o = timed(f, 5)
                    t, got = timed(f, max(10, min(2000, int(100.0 / max(est, 1e-3)))))
                    st = got["state"].cpu().numpy()
                    cell[k]["ms"].append(round(t, 4))
                    cell[k].update(samples=int(st[5]), rows=int(st[72]), S=r.last_steps_per_pass)
                    frames[k] = {q: got[q].clone() for q in ("image", "image_raw", "weights_sum", "depth")}
            off, on = cell["off"]["ms"], cell["on"]["ms"]
            cell["within"] = bool(sum(on) / len(on) - sum(off) / len(off) <= max(off) - min(off))
            cell["same"] = all(torch.equal(frames["off"][q], frames["on"][q]) for q in frames["off"]) and cell["off"]["samples"] == cell["on"]["samples"]
            res.setdefault(str(n), {})[str(ms_cap)] = cell
            del cfgs
    return res


if "--clip" in sys.argv:
    occupancy = _opt("--occupancy", "ones")
    if occupancy not in ("ones", "ellipsoid"):
        sys.exit("--occupancy ones|ellipsoid")
    if occupancy == "ellipsoid":
        from lzzx_nerf_amd.synthetic import ellipsoid_bitfield_device
        clip_bits = ellipsoid_bitfield_device(dev)[0]
    else:
        clip_bits = bits
    out = {"mode": mode, "cap": cap, "rounds": rounds, "occupancy": "all ones" if occupancy == "ones" else "ellipsoid", "device": torch.cuda.get_device_name(0),
           "frames": clip_sweep()}
    line = json.dumps(out)
    if "--out" in sys.argv:
        with open(_opt("--out", None), "w") as fh:
            fh.write(line + "\n")
    print(line)
    sys.exit(0)

if spp_list:
    out = {"mode": mode, "cap": cap, "rounds": rounds, "occupancy": "all ones", "device": torch.cuda.get_device_name(0), "frames": spp_sweep()}
    line = json.dumps(out)
    if "--out" in sys.argv:
        with open(_opt("--out", None), "w") as fh:
            fh.write(line + "\n")
    print(line)
    sys.exit(0)

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
