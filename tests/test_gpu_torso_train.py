"""Fused torso training (lzzx_nerf_amd.torso_train.FusedTorsoTrainNet, csrc/lz_torso_train.hip): the forward is FusedTorso's bits,
every gradient agrees with a float64 torch model of forward_torso (network.py:170-205) and with TorsoTrainNet, masked-out pixels
contribute nothing, the fixed-order reductions repeat bit for bit, a whole torso-stage step never synchronises with the host, and fifty
steps follow the operator path's loss curve."""
import numpy as np
import pytest
import torch

from test_gpu_torso import _torso_state
from torso_train_cases import model

pytestmark = pytest.mark.gpu
F32 = np.float32
MLP_KEYS = ["torso_deform_net.net.%d.weight" % i for i in range(3)] + ["torso_net.net.%d.weight" % i for i in range(3)]


def _pose():
    pose = np.eye(4, dtype=F32)
    th = 0.1
    pose[:3, :3] = np.array([[np.cos(th), 0, np.sin(th)], [0, 1, 0], [-np.sin(th), 0, np.cos(th)]], F32)
    pose[:3, 3] = [0.05, -0.02, 3.3]
    return torch.from_numpy(pose[None]).cuda()


def _blob(G=128):
    yy, xx = np.meshgrid(np.arange(G), np.arange(G), indexing="ij")
    return torch.from_numpy(np.exp(-(((xx - 64) / 30.0) ** 2 + ((yy - 80) / 40.0) ** 2)).astype(F32).reshape(-1)).cuda()


def _nets(ind_dim, seed=0):
    from lzzx_nerf_amd.torso import FusedTorso
    from lzzx_nerf_amd.torso_train import FusedTorsoTrainNet, TorsoTrainNet
    sd = {k: torch.from_numpy(v) for k, v in _torso_state(ind_dim, seed).items()}
    fused = FusedTorsoTrainNet(ind_dim_torso=ind_dim).cuda()
    fused.load_state_dict(sd)
    ops = TorsoTrainNet(ind_dim_torso=ind_dim).cuda()
    ops.load_state_dict(sd)
    return sd, fused, ops, FusedTorso(sd)


def _inputs(N, ind_dim, seed=4):
    g = torch.Generator().manual_seed(seed)
    xy = (torch.rand(N, 2, generator=g) * 2 - 1).cuda()
    c = (torch.randn(1, ind_dim, generator=g) * 0.1).cuda() if ind_dim else None
    return xy, c


@pytest.mark.parametrize("ind_dim", [0, 8])
@pytest.mark.parametrize("N", [1, 63, 3000, 65536])
def test_forward_is_the_inference_kernel_bit_for_bit(ind_dim, N):
    sd, fused, _, inf = _nets(ind_dim)
    xy, c = _inputs(N, ind_dim)
    poses, grid = _pose(), _blob()
    with torch.no_grad():
        a, col, d = fused(xy, poses, c)
        a_i, c_i, d_i = inf(xy, poses, c)
        assert torch.equal(a, a_i) and torch.equal(col, c_i) and torch.equal(d, d_i)
        out = fused.run_torso(xy, poses, c, bg_color=0.25, density_grid=grid, density_thresh=torch.tensor([0.05], device="cuda"))
        a_i, c_i, d_i = inf(xy, poses, c, density_grid=grid, density_thresh=0.05)
        assert torch.equal(out["torso_alpha"], a_i) and torch.equal(out["deform"], d_i)
        assert torch.equal(out["torso_color"], FusedTorso_mix(a_i, c_i, 0.25)) and out["bg_color"] is out["torso_color"]


def FusedTorso_mix(a, c, bg):
    from lzzx_nerf_amd.torso import FusedTorso
    return FusedTorso.mix_background(a, c, bg)


def _f64_grads(sd, xy, pose, c, g_alpha, g_color, g_dx):
    """float64 torch model of forward_torso (tests/torso_train_cases.py) -> gradients of sum(alpha g_alpha + color g_color + dx g_dx)"""
    return model(sd, xy, pose, c, g_alpha, g_color, g_dx, torch.float64, 0.8)[0]


def _grads(net, xy, poses, c, ga, gc, gd):
    net.zero_grad(set_to_none=True)
    cc = c.clone().requires_grad_(True) if c is not None else None
    a, col, d = net(xy, poses, cc)
    ((a * ga).sum() + (col * gc).sum() + (d * gd).sum()).backward()
    g = {k: p.grad.detach().double().cpu() for k, p in net.named_parameters()}
    if cc is not None:
        g["ind_code"] = cc.grad.detach().double().cpu()
    return g


@pytest.mark.parametrize("ind_dim", [0, 8])
def test_gradients_match_float64_model_and_operator_path(ind_dim):
    """The seeded state dict with its table scaled to U(-1e-3, 1e-3) (the reference initialises it at U(-1e-4, 1e-4)).  On the unscaled
    U(-1, 1) table dy/dx at the finest levels is ~2048 x the table's jumps, and the f32 forward's rounding of the sample positions moves the
    deform-path gradients by up to ~2e-2 x max against float64 -- for TorsoTrainNet exactly as much as for the fused kernels."""
    sd, fused, ops, _ = _nets(ind_dim, seed=3)
    sd["torso_encoder.embeddings"] = sd["torso_encoder.embeddings"] * 1e-3
    fused.load_state_dict(sd)
    ops.load_state_dict(sd)
    N = 3000
    xy, c = _inputs(N, ind_dim, seed=9)
    poses = _pose()
    g = torch.Generator().manual_seed(11)
    ga, gc, gd = [torch.randn(N, k, generator=g).cuda() for k in (1, 3, 2)]
    gf = _grads(fused, xy, poses, c, ga, gc, gd)
    go = _grads(ops, xy, poses, c, ga, gc, gd)
    ref = _f64_grads(sd, xy, poses, c, ga, gc, gd)
    keys = MLP_KEYS + ["torso_encoder.embeddings", "anchor_points"] + (["ind_code"] if ind_dim else [])
    for k in keys:
        r = ref[k].reshape(gf[k].shape)
        scale = float(r.abs().max())
        assert scale > 0, k
        tol = 1e-4 if k in MLP_KEYS else 2e-3
        assert float((gf[k] - r).abs().max()) <= tol * scale, (k, float((gf[k] - r).abs().max()), scale)
        assert float((gf[k] - go[k]).abs().max()) <= 2e-3 * scale, (k, "vs TorsoTrainNet")


def test_masked_out_pixels_contribute_nothing():
    sd, fused, _, _ = _nets(8, seed=1)
    N = 4096
    xy, c = _inputs(N, 8, seed=2)
    poses, grid = _pose(), _blob()
    bg = torch.rand(N, 3, generator=torch.Generator().manual_seed(3)).cuda()
    out = fused.run_torso(xy, poses, c, bg_color=bg, density_grid=grid, density_thresh=0.05)
    from lzzx_nerf_amd.torso import FusedTorso
    with torch.no_grad():
        occ_alpha = FusedTorso(sd)(xy, poses, c, density_grid=grid, density_thresh=0.05)[0]
    # which pixels the kernel masked: the inference kernel's zeros where the unmasked forward is not zero
    with torch.no_grad():
        free_alpha = FusedTorso(sd)(xy, poses, c)[0]
    off = (occ_alpha[:, 0] == 0) & (free_alpha[:, 0] != 0)
    assert 0.05 < float(off.float().mean()) < 0.95
    assert torch.equal(out["torso_color"][off], bg[off]) and bool((out["torso_alpha"][off] == 0).all()) and bool((out["deform"][off] == 0).all())
    # gradients of masked-out pixels only: exactly zero
    fused.zero_grad(set_to_none=True)
    w = off.float()[:, None]
    ((out["torso_color"] * w).sum() + (out["torso_alpha"] * w).sum() + (out["deform"] * w).sum()).backward()
    for k, p in fused.named_parameters():
        assert p.grad is not None and not bool(p.grad.any()), k
    # every pixel masked out: zero gradients, no error
    fused.zero_grad(set_to_none=True)
    out = fused.run_torso(xy, poses, c, bg_color=1.0, density_grid=torch.zeros_like(grid), density_thresh=0.05)
    assert bool((out["torso_color"] == 1).all())
    (out["torso_color"].sum() + out["torso_alpha"].sum()).backward()
    for k, p in fused.named_parameters():
        assert p.grad is not None and not bool(p.grad.any()), k


def test_two_backward_passes_give_the_same_bits():
    _, fused, _, _ = _nets(8, seed=5)
    N = 65536
    xy, c = _inputs(N, 8, seed=6)
    poses = _pose()
    g = torch.Generator().manual_seed(7)
    ga, gc, gd = [torch.randn(N, k, generator=g).cuda() for k in (1, 3, 2)]
    g1 = _grads(fused, xy, poses, c, ga, gc, gd)
    g2 = _grads(fused, xy, poses, c, ga, gc, gd)
    for k in MLP_KEYS + ["anchor_points", "ind_code"]:
        assert torch.equal(g1[k], g2[k]), k
    # the table: float atomics, the order of the adds is free
    assert torch.allclose(g1["torso_encoder.embeddings"], g2["torso_encoder.embeddings"], rtol=1e-5, atol=1e-6 * float(g1["torso_encoder.embeddings"].abs().max()))


def test_torso_stage_step_never_synchronises_and_scales_exactly():
    from lzzx_nerf_amd.objective import TorsoObjective
    from lzzx_nerf_amd.occupancy import update_density_grid_torso
    from lzzx_nerf_amd.torso import FusedTorso
    _, fused, _, _ = _nets(8, seed=2)
    N = 65536
    xy, c = _inputs(N, 8, seed=3)
    poses = _pose()
    grid = _blob(64) * 0.5
    target = torch.rand(N, 3, generator=torch.Generator().manual_seed(5)).cuda()
    inf = FusedTorso(fused.state_dict())
    noise = torch.rand(64 * 64, 2, generator=torch.Generator().manual_seed(6)).cuda()
    opt = torch.optim.AdamW(fused.parameters(), lr=1e-3, betas=(0.0, 0.99), eps=1e-8)
    scaler = torch.amp.GradScaler("cuda", init_scale=65536.0)

    def grads(scale):
        fused.zero_grad(set_to_none=True)
        g = grid.clone()
        thresh = update_density_grid_torso(inf, g, poses, c, density_thresh=0.01, noise=noise)[1]
        out = fused.run_torso(xy, poses, c, bg_color=1.0, density_grid=g, density_thresh=thresh)
        loss, _ = TorsoObjective()(out["torso_color"], target, fused.anchor_points)
        (loss * scale if scale != 1 else loss).backward()
        return {k: p.grad.clone() for k, p in fused.named_parameters()}

    g1 = grads(1)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        g = grid.clone()
        thresh = update_density_grid_torso(inf, g, poses, c, density_thresh=0.01, noise=noise)[1]
        out = fused.run_torso(xy, poses, c, bg_color=1.0, density_grid=g, density_thresh=thresh)
        loss, _ = TorsoObjective()(out["torso_color"], target, fused.anchor_points)
        opt.zero_grad(set_to_none=True)
        scaler.scale(loss).backward()
        gs = {k: p.grad.clone() for k, p in fused.named_parameters()}
        scaler.unscale_(opt)
        opt.step()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    for k in MLP_KEYS + ["anchor_points"]:
        assert torch.equal(gs[k], g1[k] * 65536.0), k
    e1, es = g1["torso_encoder.embeddings"], gs["torso_encoder.embeddings"]
    assert torch.allclose(es, e1 * 65536.0, rtol=1e-5, atol=1e-6 * float(es.abs().max()))


def test_fifty_steps_follow_the_operator_path():
    from lzzx_nerf_amd.objective import TorsoObjective
    from lzzx_nerf_amd.torso import FusedTorso
    from lzzx_nerf_amd.torso_train import FusedTorsoTrainNet, TorsoTrainNet
    torch.manual_seed(0)
    fused = FusedTorsoTrainNet(ind_dim_torso=8).cuda()
    ops = TorsoTrainNet(ind_dim_torso=8).cuda()
    ops.load_state_dict(fused.state_dict())
    N = 8192
    xy, c = _inputs(N, 8, seed=8)
    poses = _pose()
    grid = _blob(64)
    target = torch.rand(N, 3, generator=torch.Generator().manual_seed(9)).cuda()
    G = 64
    import torch.nn.functional as Fn

    def run_ops(net):   # renderer.py:572-631 around the operator path
        occ = Fn.grid_sample(grid.view(1, 1, G, G), xy.view(1, -1, 1, 2), align_corners=True).view(-1)
        mask = occ > 0.05
        alpha, color = torch.zeros(N, 1, device="cuda"), torch.zeros(N, 3, device="cuda")
        a, col, _ = net(xy[mask], poses, c)
        alpha[mask], color[mask] = a, col
        return color * alpha + 1.0 * (1 - alpha)

    curves = []
    for net, fwd in ((fused, lambda n: n.run_torso(xy, poses, c, 1.0, grid, 0.05)["torso_color"]), (ops, run_ops)):
        opt = torch.optim.AdamW(net.parameters(), lr=1e-3, betas=(0.0, 0.99), eps=1e-8)
        losses = []
        for _ in range(50):
            loss, _ = TorsoObjective()(fwd(net), target, net.anchor_points)
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
            losses.append(loss.detach())
        curves.append(torch.stack(losses).cpu().numpy())
    lf, lo = curves
    assert lf[-1] < lf[0] * 0.98
    assert np.abs(lf - lo).max() <= 1e-3 * np.abs(lo).max(), (lf, lo)
    with torch.no_grad():
        a_t = fused(xy, poses, c)[0]
        a_i = FusedTorso(fused.state_dict())(xy, poses, c)[0]
    assert torch.equal(a_t, a_i)
