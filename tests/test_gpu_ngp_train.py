"""Hash-grid NeRF training on fused kernels (lzzx_nerf_amd/ngp_train.py, csrc/lz_ngp_train.hip) on the device: the forward is
FusedHashgridNeRF's bits; the MLP gradients and d feats agree with a float64 restatement of network.py:73-94 under autograd; the table
gradient is lz_grid_encode_backward's scatter (float atomics: it repeats only up to summation order); the fused gradients agree with the
operator path (GenericHashgridNeRF.net); weight gradients repeat bit for bit and scale exactly; no host synchronisation; a short training
run follows the operator path's loss curve; the occupancy update and the inference round trip."""
import copy

import numpy as np
import pytest
import torch

from lzzx_nerf_amd import raymarching as R
from lzzx_nerf_amd._util import call, ptr, stream
from lzzx_nerf_amd.ngp import FusedHashgridNeRF, HashgridRenderer
from lzzx_nerf_amd.ngp_train import FusedHashgridTrainNeRF, _pack
from lzzx_nerf_amd.synthetic import GenericHashgridNeRF, ellipsoid_bitfield_device, synthetic_camera
from lzzx_nerf_amd.utils import frame_rays

pytestmark = pytest.mark.gpu

SIZES = [1, 15, 16, 257, 65536 + 5]
KINK = 1e-4     # samples with a ReLU pre-activation closer than this to 0 get no upstream gradient (f32 and f64 may take different sides)


@pytest.fixture(scope="module")
def generic():
    return GenericHashgridNeRF("cuda", seed=3)


def _fused(g):
    return FusedHashgridTrainNeRF(copy.deepcopy(g.enc), copy.deepcopy(g.sigma_net), copy.deepcopy(g.color_net)).cuda()


def _points(M, seed):
    gen = torch.Generator().manual_seed(seed)
    xyzs = (torch.rand(M, 3, generator=gen) * 1.9 - 0.95).cuda()
    d = torch.randn(M, 3, generator=gen)
    dirs = (d / d.norm(dim=-1, keepdim=True)).cuda()
    gs, gr = torch.randn(M, generator=gen).cuda(), torch.randn(M, 3, generator=gen).cuda()
    return xyzs, dirs, gs, gr


def _weights(m):
    return [m.sigma_net.net[0].weight, m.sigma_net.net[1].weight, m.color_net.net[0].weight, m.color_net.net[1].weight]


def _f64(g, xyzs, dirs, gs, gr):
    """network.py:73-94 in float64 on the operator forward's features: weight gradients, d feats [M, 32], and the samples near a ReLU kink"""
    with torch.no_grad():
        F = g.enc(xyzs, bound=1.0).double().requires_grad_(True)
        sh = g.sh(dirs).double()
    ws = [w.detach().double().requires_grad_(True) for w in _weights(g)]
    p1 = F @ ws[0].t()
    h = torch.relu(p1) @ ws[1].t()
    sigma = torch.exp(h[:, 0])
    p2 = torch.cat([sh, h[:, 1:]], -1) @ ws[2].t()
    rgb = torch.sigmoid(torch.relu(p2) @ ws[3].t())
    near = (p1.abs() < KINK).any(1) | (p2.abs() < KINK).any(1)
    keep = (~near).double()
    torch.autograd.backward([sigma, rgb], [gs.double() * keep, gr.double() * keep[:, None]])
    return [w.grad for w in ws], F.grad, near


def _close(a, b, rel):
    a, b = a.double(), b.double()
    scale = float(b.abs().max())
    return float((a - b).abs().max()) <= rel * max(scale, 1e-30), (float((a - b).abs().max()), scale)


def _backward(net, xyzs, dirs, gs, gr):
    for p in net.parameters():
        p.grad = None
    sigma, rgb = net(xyzs, dirs, 1.0)
    torch.autograd.backward([sigma, rgb], [gs, gr])
    return [w.grad.clone() for w in _weights(net)], net.encoder.embeddings.grad.clone()


def _d_feats(net, xyzs, dirs, gs, gr):
    """lz_ngp_head_backward's d feats [16, M, 2] straight from the entry point"""
    M = xyzs.shape[0]
    ws = [w.detach().contiguous() for w in _weights(net)]
    packed = _pack(ws)
    e = net.encoder
    feats = torch.empty(M, 32, device="cuda")
    call("lz_grid_encode_forward_tiled", ptr(xyzs), ptr(e.embeddings), ptr(e.offsets), ptr(feats), M, None, 1.0, 3, 2, 16, net._S, net._H, 0, 0, 0,
         stream())
    d = torch.empty(16, M, 2, device="cuda")
    g = [torch.empty_like(w) for w in ws]
    from lzzx_nerf_amd.ngp_train import _workspace
    call("lz_ngp_head_backward", ptr(packed), *[ptr(w) for w in ws], ptr(feats), ptr(dirs), M, None, ptr(gs), ptr(gr), ptr(d), *[ptr(t) for t in g],
         ptr(_workspace(xyzs.device)), stream())
    return d


@pytest.mark.parametrize("M", SIZES)
def test_forward_is_the_inference_kernel_bit_for_bit(generic, M):
    xyzs, dirs, _, _ = _points(M, M)
    net = _fused(generic)
    s, c = net(xyzs, dirs, 1.0)
    s0, c0 = FusedHashgridNeRF(generic.enc, generic.sigma_net, generic.color_net).forward(xyzs, dirs, 1.0)
    assert torch.equal(s, s0) and torch.equal(c, c0)


@pytest.mark.parametrize("M", SIZES)
def test_gradients_against_float64(generic, M):
    """every MLP weight gradient and d feats within 1e-4 x each tensor's max magnitude; the table gradient within 1e-5 x max of
    lz_grid_encode_backward fed the f64 d feats rounded to f32 (both scatters use float atomics: equal up to summation order)"""
    xyzs, dirs, gs, gr = _points(M, 100 + M)
    ref_w, ref_F, near = _f64(generic, xyzs, dirs, gs, gr)
    keep = (~near).float()
    gs, gr = gs * keep, gr * keep[:, None]
    net = _fused(generic)
    gw, gemb = _backward(net, xyzs, dirs, gs, gr)
    for a, b in zip(gw, ref_w):
        ok, info = _close(a, b, 1e-4)
        assert ok, info
    d = _d_feats(net, xyzs, dirs, gs, gr)
    ok, info = _close(d.permute(1, 0, 2).reshape(M, 32), ref_F, 1e-4)
    assert ok, info
    e = net.encoder
    ref_emb = torch.zeros_like(e.embeddings)
    unit = ((xyzs + 1.0) / 2.0).contiguous()
    call("lz_grid_encode_backward", ptr(ref_F.float().contiguous()), ptr(unit), ptr(e.embeddings), ptr(e.offsets), ptr(ref_emb), M, 3, 2, 16,
         net._S, net._H, None, None, 0, 0, 0, 1, stream())
    ok, info = _close(gemb, ref_emb, 1e-5)
    assert ok, info


@pytest.mark.parametrize("M", [257, 65536 + 5])
def test_gradients_against_the_operator_path(generic, M):
    xyzs, dirs, gs, gr = _points(M, 200 + M)
    _, _, near = _f64(generic, xyzs, dirs, gs, gr)
    keep = (~near).float()
    gs, gr = gs * keep, gr * keep[:, None]
    g = copy.deepcopy(generic)
    params = [g.enc.embeddings] + _weights(g)
    sigma, rgb = g.net(xyzs, dirs, 1.0)
    torch.autograd.backward([sigma, rgb], [gs, gr])
    net = _fused(generic)
    gw, gemb = _backward(net, xyzs, dirs, gs, gr)
    for a, p in zip([gemb] + gw, params):
        ok, info = _close(a, p.grad, 1e-4)
        assert ok, info


def test_weight_gradients_repeat_and_scale_exactly(generic):
    M = 65536 + 5
    xyzs, dirs, gs, gr = _points(M, 7)
    net = _fused(generic)
    a, _ = _backward(net, xyzs, dirs, gs, gr)
    b, _ = _backward(net, xyzs, dirs, gs, gr)
    c, _ = _backward(net, xyzs, dirs, gs * 65536.0, gr * 65536.0)
    for x, y, z in zip(a, b, c):
        assert torch.equal(x, y)
        assert torch.equal(z, x * 65536.0)


def test_no_host_synchronisation(generic):
    xyzs, dirs, gs, gr = _points(4096, 9)
    net = _fused(generic)
    _backward(net, xyzs, dirs, gs, gr)         # first call: workspace and the constant gather table
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        sigma, rgb = net(xyzs, dirs, 1.0)
        torch.autograd.backward([sigma, rgb], [gs, gr])
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(net.encoder.embeddings.grad).all())


def test_live_parameters_are_read_on_every_call(generic):
    """a write through .data (an EMA swap-in) reaches the next forward: no packed copy keyed on the version counter"""
    xyzs, dirs, _, _ = _points(1000, 11)
    net = _fused(generic)
    s0, _ = net(xyzs, dirs, 1.0)
    with torch.no_grad():
        net.sigma_net.net[1].weight.data.copy_(net.sigma_net.net[1].weight.data * 0.5)
    s1, _ = net(xyzs, dirs, 1.0)
    ref, _ = net.to_inference().forward(xyzs, dirs, 1.0)
    assert not torch.equal(s0, s1) and torch.equal(s1, ref)


def _train(net_fn, params, steps, rays_o, rays_d, nears, fars, bits, target):
    opt = torch.optim.Adam(params, lr=1e-2, betas=(0.9, 0.99), eps=1e-15)
    losses = []
    for _ in range(steps):
        ctr = torch.zeros(2, dtype=torch.int32, device="cuda")
        xyzs, dirs, deltas, rays = R.march_rays_train(rays_o, rays_d, 1.0, bits, 1, 128, nears, fars, ctr, -1, False, 128, True, 1 / 256, 128)
        sigma, rgb = net_fn(xyzs.detach().contiguous(), dirs.detach().contiguous())
        ws, _, _, img = R.composite_rays_train(sigma, rgb, torch.zeros_like(sigma), deltas, rays)
        pred = img + (1 - ws)[:, None]
        loss = ((pred - target) ** 2).mean()
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        losses.append(loss.detach())
    return torch.stack(losses).cpu().numpy()


def test_training_curve_follows_the_operator_path(generic):
    H = W = 64
    pose, intr = synthetic_camera(H, W)
    ro, rd = frame_rays(torch.from_numpy(pose).cuda(), intr, H, W)
    bits, _ = ellipsoid_bitfield_device("cuda")
    aabb = torch.tensor([-1, -1, -1, 1, 1, 1], dtype=torch.float32, device="cuda")
    nears, fars = R.near_far_from_aabb(ro, rd, aabb, 0.05)
    target = torch.rand(H * W, 3, generator=torch.Generator().manual_seed(5)).cuda()
    g = copy.deepcopy(generic)
    ref = _train(lambda x, d: g.net(x, d, 1.0), [g.enc.embeddings] + _weights(g), 50, ro, rd, nears, fars, bits, target)
    net = _fused(generic)
    got = _train(lambda x, d: net(x, d, 1.0), list(net.parameters()), 50, ro, rd, nears, fars, bits, target)
    assert ref[-1] < ref[0]
    np.testing.assert_allclose(got, ref, rtol=1e-3, atol=0)


def test_occupancy_update_matches_a_torch_restatement(generic):
    """update_extra_state's head branch (renderer.py:699-766) restated with torch and the operator API on the same points"""
    from lzzx_nerf_amd.occupancy import update_density_grid_ngp
    G, decay, thresh = 32, 0.95, 0.01
    rng = np.random.default_rng(3)
    grid0 = rng.uniform(0, 2, (1, G ** 3)).astype(np.float32)
    grid0[rng.uniform(size=grid0.shape) < 0.2] = -1.0
    noise = torch.from_numpy(rng.uniform(0, 1, (1, G ** 3, 3)).astype(np.float32)).cuda()
    net = _fused(generic)
    dg = torch.from_numpy(grid0.copy()).cuda()
    bf = torch.zeros(G ** 3 // 8, dtype=torch.uint8, device="cuda")
    mean, th = update_density_grid_ngp(net, dg, bf, bound=1.0, decay=decay, density_thresh=thresh, noise=noise)
    # the restatement, on the same points (lz_density_grid_points: torch divides by a host scalar as a reciprocal multiply, the reference's
    # formula does not) and with the per-sample arithmetic of the inference kernel
    ax = torch.arange(G, dtype=torch.int32, device="cuda")
    xx, yy, zz = torch.meshgrid(ax, ax, ax, indexing="ij")
    coords = torch.stack([xx.reshape(-1), yy.reshape(-1), zz.reshape(-1)], 1)
    idx = R.morton3D(coords).long()
    xyzs = torch.empty(G ** 3, 3, device="cuda")
    call("lz_density_grid_points", ptr(noise), 1, G, 1.0, ptr(xyzs), stream())
    dirs = torch.zeros_like(xyzs)
    dirs[:, 2] = 1
    sig = FusedHashgridNeRF(generic.enc, generic.sigma_net, generic.color_net).forward(xyzs, dirs, 1.0)[0]
    tmp = torch.zeros(1, G ** 3, device="cuda")
    tmp[0, idx] = sig
    tmp = R.morton3D_dilation(tmp)
    ref = torch.from_numpy(grid0.copy()).cuda()
    valid = (ref >= 0) & (tmp >= 0)
    ref[valid] = torch.maximum(ref[valid] * decay, tmp[valid])
    ok, info = _close(dg, ref, 1e-6)
    assert ok, info
    ref_mean = float(ref.clamp(min=0).double().mean())
    assert float(mean) == pytest.approx(ref_mean, rel=1e-5) and float(th) == np.float32(min(ref_mean, thresh))
    ref_bits = R.packbits(ref, float(th))
    near = ((ref - float(th)).abs() <= 1e-6 * ref.abs().clamp(min=1)).reshape(-1).cpu().numpy()
    mism = np.unpackbits((bf ^ ref_bits).cpu().numpy(), bitorder="little").astype(bool)
    assert not (mism & ~near).any()


def test_to_inference_renders_like_a_fused_inference_net(generic):
    H = W = 64
    pose, intr = synthetic_camera(H, W)
    ro, rd = frame_rays(torch.from_numpy(pose).cuda(), intr, H, W)
    bits, _ = ellipsoid_bitfield_device("cuda")
    net = _fused(generic)
    a = HashgridRenderer(net.to_inference(), bits).render(ro, rd, max_steps=64)["image"].clone()
    b = HashgridRenderer(FusedHashgridNeRF(generic.enc, generic.sigma_net, generic.color_net), bits).render(ro, rd, max_steps=64)["image"].clone()
    assert torch.equal(a, b)
