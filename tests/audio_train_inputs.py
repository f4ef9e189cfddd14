"""Seeded inputs of tests/golden/reference_audio_train.npz: the cases, their weights and windows (tests/frontends_inputs.py) and the upstream
gradient d enc_a.  Shared by the generator (tests/golden/make_golden_audio_train.py) and the tests, so the fixture holds outputs only.
numpy generators only."""
import numpy as np

from frontends_inputs import audio_weights, audio_windows

ATT_SCALE = 6.0   # the "att_scaled" case: attentionConvNet / attentionNet weights x 6, so the softmax is far from uniform and the
                  # gradient reaching AudioNet's output through the attention convs is a large share of the total


def cases():
    """tag -> (dim_in, att, precisions recorded).  To keep the fixture under 1 MB, the reference's f32 gradients are recorded for the
    deepspeech case with attention only, every gradient is stored as float32 (the float64 ones thereby rounded by at most 6e-8 of their
    value, far below the tests' bounds), and hubert (1024 channels: 98 304 encoder_conv.0 gradients per run) is left to the tests' own
    float64 model."""
    return {"29_att": (29, True, ("f32", "f64")), "29_noatt": (29, False, ("f64",)), "44_att": (44, True, ("f64",)),
            "44_noatt": (44, False, ("f64",)), "29_att_scaled": (29, True, ("f64",))}


def case_weights(tag):
    dim_in, att, _ = cases()[tag]
    P = audio_weights(dim_in)
    if tag.endswith("_scaled"):
        for k in P:
            if k.startswith("audio_att_net.") and k.endswith(".weight"):
                P[k] = (P[k] * np.float32(ATT_SCALE)).astype(np.float32)
    if not att:
        P = {k: v for k, v in P.items() if not k.startswith("audio_att_net.")}
    return P


def case_windows(tag):
    dim_in, att, _ = cases()[tag]
    a = audio_windows(dim_in)
    return a if att else a[:1].copy()


def upstream(tag, dim_aud=32, seed=31):
    """d enc_a: [1, dim_aud] with attention, [1, dim_aud] for the one-window case without"""
    dim_in, att, _ = cases()[tag]
    return np.random.default_rng(seed + dim_in + (100 if tag.endswith("_scaled") else 0)).normal(size=(1, dim_aud)).astype(np.float32)


def torch_encode_audio(P, a, att, drop_att_conv_path=False):
    """encode_audio (network.py:226-240) restated with torch.nn.functional on whatever dtype / device P's tensors have (the tests' float64
    model).  drop_att_conv_path: AudioAttNet's conv stack reads a detached copy of AudioNet's output, i.e. the gradient a backward would
    give if it forgot that path into feat"""
    import torch.nn.functional as Fn
    x = a
    for i in (0, 2, 4, 6):
        x = Fn.leaky_relu(Fn.conv1d(x, P[f"audio_net.encoder_conv.{i}.weight"], P[f"audio_net.encoder_conv.{i}.bias"], stride=2, padding=1), 0.02)
    x = Fn.leaky_relu(Fn.linear(x.squeeze(-1), P["audio_net.encoder_fc1.0.weight"], P["audio_net.encoder_fc1.0.bias"]), 0.02)
    feat = Fn.linear(x, P["audio_net.encoder_fc1.2.weight"], P["audio_net.encoder_fc1.2.bias"])           # [n, dim_aud]
    if not att:
        return feat
    y = (feat.detach() if drop_att_conv_path else feat).T[None]                                            # [1, dim_aud, n]
    for i in (0, 2, 4, 6, 8):
        y = Fn.leaky_relu(Fn.conv1d(y, P[f"audio_att_net.attentionConvNet.{i}.weight"], P[f"audio_att_net.attentionConvNet.{i}.bias"], padding=1), 0.02)
    s = Fn.softmax(Fn.linear(y.reshape(1, -1), P["audio_att_net.attentionNet.0.weight"], P["audio_att_net.attentionNet.0.bias"]), dim=1)
    return (s.reshape(-1, 1) * feat).sum(0, keepdim=True)                                                  # [1, dim_aud]


def softmax_backward_condition(P, a, g):
    """condition number of AudioAttNet's softmax backward, dL/dlogit[t] = s[t] (gs[t] - sum_u s[u] gs[u]) with gs[t] = feat[t] . g, in a
    float64 evaluation: the magnitude of the terms it cancels, max_t s[t] (|feat[t]| . |g| + sum_u s[u] |feat[u]| . |g|), over max_t
    |dL/dlogit[t]|.  Rounding of those terms (in any f32 evaluation, the reference's included) reaches every AudioAttNet gradient scaled by it."""
    import torch
    import torch.nn.functional as Fn
    P = {k: torch.as_tensor(v).double() for k, v in P.items()}
    x = torch.as_tensor(a).double()
    for i in (0, 2, 4, 6):
        x = Fn.leaky_relu(Fn.conv1d(x, P[f"audio_net.encoder_conv.{i}.weight"], P[f"audio_net.encoder_conv.{i}.bias"], stride=2, padding=1), 0.02)
    x = Fn.leaky_relu(Fn.linear(x.squeeze(-1), P["audio_net.encoder_fc1.0.weight"], P["audio_net.encoder_fc1.0.bias"]), 0.02)
    feat = Fn.linear(x, P["audio_net.encoder_fc1.2.weight"], P["audio_net.encoder_fc1.2.bias"])
    y = feat.T[None]
    for i in (0, 2, 4, 6, 8):
        y = Fn.leaky_relu(Fn.conv1d(y, P[f"audio_att_net.attentionConvNet.{i}.weight"], P[f"audio_att_net.attentionConvNet.{i}.bias"], padding=1), 0.02)
    s = Fn.softmax(Fn.linear(y.reshape(1, -1), P["audio_att_net.attentionNet.0.weight"], P["audio_att_net.attentionNet.0.bias"]), dim=1)[0]
    g = torch.as_tensor(g).double().reshape(-1)
    gs, mag = feat @ g, feat.abs() @ g.abs()
    return float((s * (mag + (s * mag).sum())).max() / (s * (gs - (s * gs).sum())).abs().max())
