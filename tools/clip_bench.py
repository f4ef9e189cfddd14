"""A clip of frames from one audio track: TalkingHeadFrame.render_clip against a loop of TalkingHeadFrame.render over the same frames
(DESIGN 4.11), at the reference's deployed inference settings (HubertInferenceMQ.do_inference: max_steps 16, fp16).

    python tools/clip_bench.py [--frames K] [--size 450] [--rounds 5] [--out profiles/clip_bench.json]

Workload: the synthetic scene and camera of lzzx_nerf_amd.synthetic (ellipsoid occupancy, orbiting head pose), size x size frames, fused
frame kernel in f16, HuBERT features (dim_in 1024), att_mode 2, smooth_lips on, torso branch on every pixel over a scalar background,
RGB24 output, a track of exactly K rows.  The two paths run in the same process, alternating clip / loop within each round, each timed
by the wall clock around the whole clip with a device synchronisation at both ends; the figure is the median over the rounds of ms per
frame.  The loop is what a caller of the per-frame interface writes: frame_rays, audio_window, render.  Next to it, the whole-track audio
encoder alone against K calls of the per-frame encoder (median of device-event times)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lzzx_nerf_amd.gridencoder import grid_offsets  # noqa: E402
from lzzx_nerf_amd.pipeline import TalkingHeadFrame, audio_window  # noqa: E402
from lzzx_nerf_amd.synthetic import ellipsoid_bitfield_device, load_golden, make_params, orbit_pose, synthetic_camera  # noqa: E402
from lzzx_nerf_amd.utils import frame_rays  # noqa: E402


def state_dict(dim_in=1024, dim_aud=32):
    """head: the synthetic workload's parameters; torso and audio nets: seeded random weights in the reference's shapes"""
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in make_params(load_golden()).items()}
    rng = np.random.default_rng(7)
    offs = np.asarray(grid_offsets(2, 16, np.exp2(np.log2(2048 / 16) / 15), 16, 16))
    lin = lambda n, k: torch.from_numpy((rng.uniform(-1, 1, (n, k)) / np.sqrt(k)).astype(np.float32))
    sd.update({"anchor_points": torch.tensor([[0.01, 0.01, 0.1, 1], [-0.1, -0.1, 0.1, 1], [0.1, -0.1, 0.1, 1]]),
               "torso_deform_net.net.0.weight": lin(32, 84), "torso_deform_net.net.1.weight": lin(32, 32),
               "torso_deform_net.net.2.weight": lin(2, 32), "torso_net.net.0.weight": lin(32, 116), "torso_net.net.1.weight": lin(32, 32),
               "torso_net.net.2.weight": lin(4, 32), "torso_encoder.offsets": torch.from_numpy(offs.astype(np.int32)),
               "torso_encoder.embeddings": torch.from_numpy(rng.uniform(-1, 1, (int(offs[-1]), 2)).astype(np.float32))})
    for idx, (ci, co) in zip((0, 2, 4, 6), ((dim_in, 32), (32, 32), (32, 64), (64, 64))):
        sd[f"audio_net.encoder_conv.{idx}.weight"], sd[f"audio_net.encoder_conv.{idx}.bias"] = lin(co, ci * 3).reshape(co, ci, 3), lin(1, co).reshape(co)
    for idx, (ci, co) in zip((0, 2), ((64, 64), (64, dim_aud))):
        sd[f"audio_net.encoder_fc1.{idx}.weight"], sd[f"audio_net.encoder_fc1.{idx}.bias"] = lin(co, ci), lin(1, co).reshape(co)
    for idx, (ci, co) in zip((0, 2, 4, 6, 8), ((dim_aud, 16), (16, 8), (8, 4), (4, 2), (2, 1))):
        sd[f"audio_att_net.attentionConvNet.{idx}.weight"] = lin(co, ci * 3).reshape(co, ci, 3)
        sd[f"audio_att_net.attentionConvNet.{idx}.bias"] = lin(1, co).reshape(co)
    sd["audio_att_net.attentionNet.0.weight"], sd["audio_att_net.attentionNet.0.bias"] = lin(8, 8), lin(1, 8).reshape(8)
    return sd


def event_median(fn, reps):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
    ev[0].record()
    for i in range(reps):
        fn()
        ev[i + 1].record()
    torch.cuda.synchronize()
    return float(np.median([ev[i].elapsed_time(ev[i + 1]) for i in range(reps)]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--size", type=int, default=450)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--max-steps", type=int, default=16)
    ap.add_argument("--precision", default="f16")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clip_bench.json"))
    a = ap.parse_args()
    device = torch.device("cuda")
    K, H, W = a.frames, a.size, a.size
    golden = load_golden()
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(device)
    bits, _ = ellipsoid_bitfield_device(device)
    thf = TalkingHeadFrame(state_dict(), bits, bound=1.0, precision=a.precision, device=device, smooth_lips=True, mode="fused")
    _, intr = synthetic_camera(H, W)
    poses = dev(np.stack([orbit_pose(k) for k in range(K)]))
    feats = torch.randn(K, 1024, 16, device=device, generator=torch.Generator(device=device).manual_seed(4))
    eyes = torch.full((K, 1), 0.25, device=device)
    ind, ind_t = dev(golden["net_ind"]), torch.zeros(8, device=device)
    lin1 = torch.linspace(-1, 1, H, device=device)
    bgc = torch.stack(torch.meshgrid(lin1, lin1, indexing="xy"), -1).reshape(-1, 2).contiguous()
    kw = dict(ind_code=ind, bg_coords=bgc, ind_code_torso=ind_t, bg_color=1.0, max_steps=a.max_steps, rgb24=True)
    last = {}

    def clip():
        thf.reset()
        for out in thf.render_clip(poses, intr, H, W, feats, 2, eyes=eyes, **kw):
            pass
        last["clip"] = out["image_rgb24"]

    def loop():
        thf.reset()
        for k in range(K):
            ro, rd = frame_rays(poses[k], intr, H, W)
            out = thf.render(ro, rd, audio_window(feats, 2, k), eye=eyes[k], poses=poses[k:k + 1], **kw)
        last["loop"] = out["image_rgb24"]

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / K * 1e3

    clip()                                             # warm-up: code objects, buffers
    last_clip = last["clip"].clone()
    loop()
    same = bool(torch.equal(last_clip, last["loop"]))  # the last frame of both paths, bit for bit
    rounds = {"render_clip": [], "render_loop": []}
    for _ in range(a.rounds):
        rounds["render_clip"].append(wall(clip))
        rounds["render_loop"].append(wall(loop))
    enc = thf.audio
    track_ms = event_median(lambda: enc.encode_track(feats, 2, 0, K, True, None), 20)
    wins = [audio_window(feats, 2, k) for k in range(K)]
    per_frame_ms = event_median(lambda: [enc(w) for w in wins], 5)
    res = {"device": torch.cuda.get_device_name(0),
           "workload": f"{H}x{W}, max_steps {a.max_steps}, {a.precision}, fused frame kernel, dim_in 1024, att_mode 2, smooth_lips, torso on, "
                       f"rgb24, K = T = {K}",
           "unit": "ms per frame, wall clock around the whole clip; median of rounds",
           "rounds": {k: [round(v, 4) for v in vs] for k, vs in rounds.items()},
           "render_clip_ms_per_frame": round(float(np.median(rounds["render_clip"])), 4),
           "render_loop_ms_per_frame": round(float(np.median(rounds["render_loop"])), 4),
           "last_frame_same_bits": same,
           "audio": {"encode_track_ms_per_clip": round(track_ms, 4), "per_frame_encoder_ms_per_clip": round(per_frame_ms, 4), "frames": K}}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
