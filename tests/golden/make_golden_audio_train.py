#!/usr/bin/env python3
"""Generate tests/golden/reference_audio_train.npz from the REFERENCE's own Python (build container only; see make_golden.py for the
back-end adapters): NeRFNetwork.encode_audio (network.py:226-240) for asr_model deepspeech (29) and esperanto (44), with
attention (8 windows) and without (opt.att = 0, one window), and the .grad of every audio_net.* / audio_att_net.* parameter after
backward of sum(enc_a * g) for a seeded upstream gradient g, after net.double() and (deepspeech with attention) in the reference's f32.

Weights, windows and g come from numpy generators (tests/audio_train_inputs.py), so the fixture holds outputs and key names only.
Key layout: "<case>/<prec>/enc_a", "<case>/<prec>/grad/<state-dict key>", "<case>/keys" (the parameter names in state-dict order).

Run:  python tests/golden/make_golden_audio_train.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402  (installs sys.path for the reference and the checker)
import make_golden_frontends as MGF  # noqa: E402

sys.path.insert(0, os.path.dirname(HERE))
from audio_train_inputs import case_weights, case_windows, cases, upstream  # noqa: E402


def main():
    MG.install_backends()
    MGF.install_raymarching_backend()
    from nerf_triplane.network import NeRFNetwork  # reference
    asr = {29: "deepspeech", 44: "esperanto"}
    out = {}
    for tag, (dim_in, att, precs) in cases().items():
        for prec in precs:
            opt = MG.Opt()
            opt.asr_model = asr[dim_in]
            torch.manual_seed(0)
            net = NeRFNetwork(opt)
            assert net.audio_in_dim == dim_in
            MGF.load_np(net, case_weights(tag))
            if not att:
                net.att = 0
            dt = torch.float64 if prec == "f64" else torch.float32
            if prec == "f64":
                net.double()
            a = torch.from_numpy(case_windows(tag)).to(dt)
            g = torch.from_numpy(upstream(tag)).to(dt)
            net.zero_grad(set_to_none=True)
            enc = net.encode_audio(a)
            assert tuple(enc.shape) == (1, 32)
            (enc * g).sum().backward()
            names = [k for k, _ in net.named_parameters() if k.startswith("audio_net.") or (att and k.startswith("audio_att_net."))]
            params = dict(net.named_parameters())
            store = np.float32   # see audio_train_inputs.cases
            out[f"{tag}/{prec}/enc_a"] = enc.detach().numpy().astype(store)
            for k in names:
                out[f"{tag}/{prec}/grad/{k}"] = params[k].grad.numpy().astype(store)
            out[f"{tag}/keys"] = np.array(names)
    path = os.path.join(HERE, "reference_audio_train.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path) // 1024, "KB;", len(out), "arrays")


if __name__ == "__main__":
    main()
