"""Fused audio encoder training (lzzx_nerf_amd.audio_train.FusedAudioTrainNet, csrc/lz_audio_train.hip): the forward is the inference
kernel's bits; every parameter gradient matches the reference's (tests/golden/reference_audio_train.npz) and a float64 model; the fixed-order
reductions repeat bit for bit and scale exactly with the upstream gradient; a step never synchronises with the host; enc_a's gradient from
FusedTriplaneTrainHead reaches the audio weights; fifty AdamW steps follow torch autograd's.

Gradient bound.  Every gradient element is an f32 chain of at most 3 072 products (encoder_conv.0 at 1 024 channels: 8 windows x 8 positions
for its weights; 3 x 1 024 terms in the forward it differentiates) evaluated once in f32 against a float64 evaluation of the same function.
The recomputed activations and each layer's backward carry relative rounding of order sqrt(terms) x 2^-24 ~ 3e-6 at worst, and the layers
compound a few of these; measured against each tensor's largest magnitude that is ~1e-6 typically and under 1e-5 always, so the tests
demand TOL = 2e-5 x max|reference| per tensor of AudioNet.  Every AudioAttNet gradient passes through the softmax backward,
s[t] (gs[t] - sum_u s[u] gs[u]), which cancels terms up to kappa times larger than its result (kappa =
audio_train_inputs.softmax_backward_condition: 120 to 1 500 on these inputs); their rounding reaches those gradients scaled by kappa, so
they are held to kappa x TOL.  The reference's own f32 gradients sit up to 2e-5 from its float64 ones for the same reason.  Against the
reference's f32 run the same bounds hold (two f32 evaluations that differ in summation order)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from audio_train_inputs import (case_weights, case_windows, cases, softmax_backward_condition, torch_encode_audio,  # noqa: E402
                                upstream)
from test_audio_oracle import audio_state  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "reference_audio_train.npz")
TOL = 2e-5


def _net(sd, dim_in, att):
    from lzzx_nerf_amd.audio_train import FusedAudioTrainNet
    net = FusedAudioTrainNet(dim_in=dim_in, dim_aud=32, att=att)
    net.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
    return net.cuda()


def _fused_grads(net, a, g):
    net.zero_grad(set_to_none=True)
    out = net(a)
    (out * g).sum().backward()
    return out, {k: p.grad.detach().double().cpu().numpy() for k, p in net.named_parameters()}


def _f64_grads(sd, a, g, att, drop_att_conv_path=False):
    P = {k: torch.as_tensor(v).double().clone().requires_grad_(True) for k, v in sd.items()}
    out = torch_encode_audio(P, torch.as_tensor(a).double(), att, drop_att_conv_path)
    (out * torch.as_tensor(g).double()).sum().backward()
    return {k: v.grad.numpy() for k, v in P.items()}


def _rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def _assert_close(got, want, kappa=1.0, what=""):
    """TOL per AudioNet tensor, kappa x TOL per AudioAttNet tensor (module docstring)"""
    assert set(got) == set(want), (what, sorted(set(got) ^ set(want)))
    for k in want:
        tol = TOL * (max(kappa, 1.0) if k.startswith("audio_att_net.") else 1.0)
        assert got[k].shape == want[k].shape, (what, k)
        assert _rel(got[k], want[k]) <= tol, (what, k, _rel(got[k], want[k]), tol)


@pytest.mark.parametrize("dim_in", [29, 44, 1024])
@pytest.mark.parametrize("att", [True, False])
def test_forward_is_the_inference_kernel_bit_for_bit(dim_in, att):
    from lzzx_nerf_amd.audio import FusedAudioEncoder
    from oracle.audio import encode_audio
    sd = audio_state(dim_in, 32, att)
    net = _net(sd, dim_in, att)
    n = 8 if att else 3
    a = np.random.default_rng(dim_in + 7).normal(size=(n, dim_in, 16)).astype(np.float32)
    ad = torch.from_numpy(a).cuda()
    out = net(ad)
    assert out.requires_grad and out.shape == ((1, 32) if att else (n, 32))
    inf = FusedAudioEncoder(net.state_dict())(ad)
    assert torch.equal(out.detach(), inf)
    assert np.array_equal(out.detach().cpu().numpy(), encode_audio(sd, a, att))


@pytest.mark.parametrize("tag", sorted(cases()))
def test_gradients_match_the_reference(tag):
    """every parameter gradient against the reference's float64 gradients (and, where recorded, its f32 ones) within TOL"""
    dim_in, att, precs = cases()[tag]
    z = np.load(GOLDEN)
    sd = case_weights(tag)
    net = _net(sd, dim_in, att)
    out, got = _fused_grads(net, torch.from_numpy(case_windows(tag)).cuda(), torch.from_numpy(upstream(tag)).cuda())
    keys = list(z[tag + "/keys"])
    assert list(got) == keys
    kappa = softmax_backward_condition(sd, case_windows(tag), upstream(tag)) if att else 1.0
    for prec in precs:
        want = {k: z[f"{tag}/{prec}/grad/{k}"].astype(np.float64) for k in keys}
        _assert_close(got, want, kappa, what=(tag, prec))
        assert _rel(out.detach().double().cpu().numpy(), z[f"{tag}/{prec}/enc_a"].astype(np.float64)) <= 1e-5


def test_the_attention_conv_path_into_feat_is_there():
    """With the attention weights scaled (case 29_att_scaled), the gradient AudioNet receives through AudioAttNet's conv stack is a large
    share of the total: a backward that dropped it would miss the float64 model by far more than TOL -- and the fused one does not."""
    tag = "29_att_scaled"
    sd, a, g = case_weights(tag), case_windows(tag), upstream(tag)
    full, dropped = _f64_grads(sd, a, g, True), _f64_grads(sd, a, g, True, drop_att_conv_path=True)
    assert max(_rel(dropped[k], full[k]) for k in full if k.startswith("audio_net.")) > 100 * TOL
    _, got = _fused_grads(_net(sd, 29, True), torch.from_numpy(a).cuda(), torch.from_numpy(g).cuda())
    _assert_close(got, full, softmax_backward_condition(sd, a, g), what=tag)


@pytest.mark.parametrize("att", [True, False])
def test_hubert_gradients_match_float64_model(att):
    """1 024 input channels: the wide first layer's output comes from the forward's workspace and encoder_conv.0's 98 304 weight gradients
    from the chip-wide kernel"""
    sd = audio_state(1024, 32, att)
    n = 8 if att else 2
    a = np.random.default_rng(5).normal(size=(n, 1024, 16)).astype(np.float32)
    g = np.random.default_rng(6).normal(size=(1, 32) if att else (n, 32)).astype(np.float32)
    _, got = _fused_grads(_net(sd, 1024, att), torch.from_numpy(a).cuda(), torch.from_numpy(g).cuda())
    _assert_close(got, _f64_grads(sd, a, g, att), softmax_backward_condition(sd, a, g) if att else 1.0, what=("hubert", att))


@pytest.mark.parametrize("dim_in", [29, 1024])
def test_repeatable_and_exactly_linear_in_the_upstream_gradient(dim_in):
    sd = audio_state(dim_in, 32, True)
    net = _net(sd, dim_in, True)
    a = torch.from_numpy(np.random.default_rng(1).normal(size=(8, dim_in, 16)).astype(np.float32)).cuda()
    g = torch.from_numpy(np.random.default_rng(2).normal(size=(1, 32)).astype(np.float32)).cuda()
    ps = list(net.parameters())
    out = net(a)
    g1 = torch.autograd.grad(out, ps, g, retain_graph=True)
    g2 = torch.autograd.grad(out, ps, g, retain_graph=True)
    g3 = torch.autograd.grad(out, ps, g * 65536.0)
    for x, y, s in zip(g1, g2, g3):
        assert torch.equal(x, y)
        assert torch.equal(x * 65536.0, s)


def test_no_host_synchronisation_under_autocast():
    sd = audio_state(1024, 32, True)
    net = _net(sd, 1024, True)
    a = torch.randn(8, 1024, 16, device="cuda")
    target = torch.randn(1, 32, device="cuda")
    opt = torch.optim.AdamW(net.param_groups(1e-3, 1e-4), betas=(0.0, 0.99), eps=1e-8)
    for _ in range(2):   # allocator and optimizer state set up outside the check
        opt.zero_grad(set_to_none=True)
        ((net(a) - target) ** 2).mean().backward()
        opt.step()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with torch.autocast("cuda", dtype=torch.float16):
            enc = net(a)
            loss = ((enc - target) ** 2).mean()
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert enc.dtype == torch.float32
    assert all(p.grad is not None and p.grad.dtype == torch.float32 for p in net.parameters())


@pytest.mark.parametrize("record", [True, False])
def test_wired_to_the_training_head(params, golden, record):
    """enc_a from FusedAudioTrainNet -> FusedTriplaneTrainHead (recording and recomputing arrangements) -> composite -> HeadObjective ->
    backward: the audio gradients equal a float64 model's fed the enc_a gradient the head produced"""
    from conftest import ellipsoid_bitfield, synthetic_camera
    from lzzx_nerf_amd import raymarching as R
    from lzzx_nerf_amd.head_train import FusedTriplaneTrainHead
    from lzzx_nerf_amd.objective import HeadObjective
    from oracle.head import get_rays
    H = W = 32
    pose, intr = synthetic_camera(H, W)
    ro, rd = get_rays(pose, intr, H, W)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    head = FusedTriplaneTrainHead({k: v for k, v in params.items()}, bound=1.0, record=record).cuda()
    sd = case_weights("29_att")
    audio = _net(sd, 29, True)
    a = case_windows("29_att")
    nears, fars = R.near_far_from_aabb(dev(ro), dev(rd), dev(np.array([-1, -0.5, -1, 1, 0.5, 1], np.float32)), 0.05)
    ctr = torch.zeros(2, dtype=torch.int32, device="cuda")
    xyzs, dirs, deltas, rays = R.march_rays_train(dev(ro), dev(rd), 1.0, dev(ellipsoid_bitfield()[0]), 1, 128, nears, fars, ctr, -1, True, 128,
                                                  True, 1 / 256, 16)
    gen = torch.Generator(device="cuda").manual_seed(0)
    N = H * W
    target, bg = torch.rand(N, 3, device="cuda", generator=gen), torch.rand(N, 3, device="cuda", generator=gen)
    face = torch.rand(N, device="cuda", generator=gen) < 0.4
    obj = HeadObjective(200000)
    enc_a = audio(dev(a))
    captured = {}
    enc_a.register_hook(lambda g: captured.setdefault("g", g.detach().clone()))
    sigma, rgb, a0, a1, unc = head(xyzs.contiguous(), dirs.contiguous(), enc_a, dev(golden["net_ind"]), dev(golden["net_eye"]))
    ws, a0s, a1s, us, dep, img = R.composite_rays_train_triplane(sigma, rgb, a0.squeeze(-1), a1.squeeze(-1), unc.squeeze(-1), deltas, rays)
    loss, _, _ = obj(img, ws, a0s, a1s, us, bg, target, face, 96000)
    loss.backward()
    g = captured["g"]
    assert g.shape == (1, 32) and float(g.abs().max()) > 0
    got = {k: p.grad.detach().double().cpu().numpy() for k, p in audio.named_parameters()}
    gn = g.cpu().numpy()
    _assert_close(got, _f64_grads(sd, a, gn, True), softmax_backward_condition(sd, a, gn), what=("head", record))


def test_fifty_adamw_steps_follow_torch_autograd():
    """fifty AdamW(betas=(0, 0.99), eps=1e-8) steps on param_groups toward a fixed target, against the same steps on the f32 torch model:
    the loss curves agree to 1e-3 relative at every step.  The loss falls from 0.27 to about 4e-3 and oscillates near the optimum (beta1 = 0);
    a float64 run of the same steps stays within 3e-5 of an f32 one, and so does an f32 run whose gradients carry 1e-6 relative noise, so
    1e-3 leaves a 30x margin for summation order while a wrong gradient moves the curve by far more.  Afterwards the inference encoder on the trained state dict still gives net(a)'s
    bits, and a write through .data (the reference's EMA) changes the next forward."""
    from lzzx_nerf_amd.audio import FusedAudioEncoder
    sd = case_weights("29_att")
    net = _net(sd, 29, True)
    P = {k: torch.from_numpy(v).cuda().requires_grad_(True) for k, v in sd.items()}
    names = list(net.state_dict())
    a = torch.from_numpy(case_windows("29_att")).cuda()
    target = torch.from_numpy(np.random.default_rng(9).normal(size=(1, 32)).astype(np.float32) * 0.5).cuda()
    groups = net.param_groups(1e-3, wd=1e-4)
    opt_f = torch.optim.AdamW(groups, betas=(0.0, 0.99), eps=1e-8)
    ref_groups = [{"params": [P[k] for k in names if k.startswith(pre)], "lr": g["lr"], "weight_decay": g["weight_decay"]}
                  for pre, g in zip(("audio_net.", "audio_att_net."), groups)]
    opt_t = torch.optim.AdamW(ref_groups, betas=(0.0, 0.99), eps=1e-8)
    lf, lt = [], []
    for _ in range(50):
        opt_f.zero_grad(set_to_none=True)
        loss = ((net(a) - target) ** 2).mean()
        loss.backward()
        opt_f.step()
        opt_t.zero_grad(set_to_none=True)
        loss_t = ((torch_encode_audio(P, a, True) - target) ** 2).mean()
        loss_t.backward()
        opt_t.step()
        lf.append(loss.detach())
        lt.append(loss_t.detach())
    lf, lt = torch.stack(lf).cpu().numpy(), torch.stack(lt).cpu().numpy()
    assert lf[-1] < 0.5 * lf[0]
    assert np.max(np.abs(lf - lt) / lt) < 1e-3, np.max(np.abs(lf - lt) / lt)
    with torch.no_grad():
        out = net(a)
        assert torch.equal(FusedAudioEncoder(net.state_dict())(a), out)
        w = net.audio_net.encoder_fc1[2].weight
        w.data.copy_(w.data * 0.5)      # EMA-style write: does not bump _version
        assert not torch.equal(net(a), out)
        assert torch.equal(FusedAudioEncoder(net.state_dict())(a), net(a))
