"""Audio encoder training: forward + backward of FusedAudioTrainNet (csrc/lz_audio.hip + csrc/lz_audio_train.hip) against torch autograd over
the same layers (nn.Conv1d / nn.Linear / LeakyReLU / softmax, encode_audio's graph, network.py:9-70, 226-240), in f32 and under autocast
(fp16) as the reference's `-O` mode runs them.

    python tools/audio_train_bench.py [--steps K] [--rounds R] [--dims 29,1024] [--only fused|torch_f32|torch_autocast] [--out PATH]

Each variant is one call of: zero_grad, enc_a = encode_audio(a) on 8 windows with attention, sum(enc_a * g).backward().  Variants alternate
within each round; each number is the median over rounds of per-round medians of device-event times per call (ms).  `--only` runs one
variant alone (the rocprofv3 --kernel-trace --stats runs)."""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as Fn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lzzx_nerf_amd.audio_train import FusedAudioTrainNet  # noqa: E402


def torch_encode_audio(net, a):
    """encode_audio as torch modules compute it (the reference's graph), on FusedAudioTrainNet's parameters"""
    x = net.audio_net.encoder_conv(a).squeeze(-1)
    feat = net.audio_net.encoder_fc1(x)                                     # [8, dim_aud]
    att = net.audio_att_net
    y = att.attentionConvNet(feat.unsqueeze(0).permute(0, 2, 1))
    s = att.attentionNet(y.view(1, -1)).view(1, -1, 1)
    return torch.sum(s * feat.unsqueeze(0), dim=1)                          # [1, dim_aud]


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
    for fn in variants.values():   # warm-up: code objects, library algorithm choice
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for n, fn in variants.items():
            res[n].append(timed(fn, k))
    return {n: float(np.median(v)) for n, v in res.items()}


def make(dim_in):
    torch.manual_seed(0)
    fused = FusedAudioTrainNet(dim_in=dim_in, dim_aud=32, att=True).cuda()
    ref = FusedAudioTrainNet(dim_in=dim_in, dim_aud=32, att=True).cuda()
    ref.load_state_dict(fused.state_dict())
    g = torch.Generator().manual_seed(1)
    a = torch.randn(8, dim_in, 16, generator=g).cuda()
    up = torch.randn(1, 32, generator=g).cuda()

    def fused_step():
        fused.zero_grad(set_to_none=True)
        (fused(a) * up).sum().backward()

    def torch_step(autocast):
        def f():
            ref.zero_grad(set_to_none=True)
            with torch.autocast("cuda", dtype=torch.float16, enabled=autocast):
                enc = torch_encode_audio(ref, a)
            (enc.float() * up).sum().backward()
        return f

    return {"fused": fused_step, "torch_f32": torch_step(False), "torch_autocast": torch_step(True)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--dims", default="29,1024")
    ap.add_argument("--only", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0), "steps": a.steps, "rounds": a.rounds, "n_win": 8, "dim_aud": 32, "att": True,
           "unit": "ms per forward + backward", "results": {}}
    for dim_in in [int(v) for v in a.dims.split(",")]:
        variants = make(dim_in)
        if a.only:
            variants = {a.only: variants[a.only]}
        r = alternate(variants, a.steps, a.rounds)
        out["results"][str(dim_in)] = {k: round(v, 4) for k, v in r.items()}
        print(dim_in, out["results"][str(dim_in)], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
