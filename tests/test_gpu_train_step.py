"""Training step (BASELINE cfg3 shape, scaled down): forward + backward through the operator API exactly as the
reference's run_cuda training branch arranges it (renderer.py:279-304) -- march_rays_train -> 3 GridEncoders ->
bias-free MLPs (torch Linear, autograd) -> SH -> composite_rays_train_triplane -> loss -> backward -- against an
independent float64 PyTorch model of the same math on the CPU (dense bilinear/hash lookups written with index_select,
compositing with a python loop over rays).  This checks the whole gradient chain: compositing backward, SH backward,
grid scatter-add backward and the chain rule through the (x + bound) / (2 bound) mapping."""
import numpy as np
import pytest
import torch

from conftest import ellipsoid_bitfield, synthetic_camera
from oracle import oracle as O
from oracle.head import TriplaneSpec, get_rays

pytestmark = pytest.mark.gpu


def _grid64(x01, emb, offsets, scales, ress):
    """float64 differentiable restatement of one D=2, C=1 hash-grid plane (gridencoder.cu:75-177)"""
    outs = []
    for l in range(len(scales)):
        hs = int(offsets[l + 1] - offsets[l])
        pos = x01 * float(scales[l]) + 0.5
        pg = torch.floor(pos.detach())
        fr = pos - pg
        pg = pg.long()
        stride = int(ress[l]) + 1
        dense = stride * stride <= hs
        acc = 0
        for c in range(4):
            c0, c1 = pg[:, 0] + (c & 1), pg[:, 1] + (c >> 1)
            if dense:
                idx = c0 + c1 * stride
            else:
                idx = (c0 ^ ((c1 * 2654435761) & 0xFFFFFFFF)) & 0xFFFFFFFF
            idx = idx % hs + int(offsets[l])
            w = (fr[:, 0] if c & 1 else 1 - fr[:, 0]) * (fr[:, 1] if c >> 1 else 1 - fr[:, 1])
            acc = acc + w * emb[idx, 0]
        outs.append(acc)
    return torch.stack(outs, 1)


@pytest.mark.parametrize("K,N,relu", [(36, 64, True), (64, 32, False), (36, 16, True), (16, 1, False), (69, 64, True), (64, 64, True),
                                      (64, 65, False), (84, 64, True), (64, 3, False), (36, 32, True), (32, 1, False), (1, 5, True),
                                      (96, 64, False), (128, 7, True), (116, 32, True)])
def test_lz_linear_matches_float64(K, N, relu):
    """csrc/lz_linear.hip (forward with fused ReLU, data gradient with fused ReLU mask, in-kernel weight-gradient reduction)
    against float64 torch on every layer shape of the triplane head, ragged M; tolerance = f32 accumulation order"""
    from lzzx_nerf_amd.linear import lz_linear
    g = torch.Generator().manual_seed(K * 131 + N)
    M = 5003
    x = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g) / K ** 0.5
    gy = torch.randn(M, N, generator=g)
    xg, wg = x.cuda().requires_grad_(True), w.cuda().requires_grad_(True)
    y = lz_linear(xg, wg, relu)
    xc, wc = x.double().requires_grad_(True), w.double().requires_grad_(True)
    yc = xc @ wc.T
    if relu:
        yc = torch.relu(yc)
    assert torch.allclose(y.detach().cpu().double(), yc.detach(), atol=2e-5, rtol=1e-5)
    y.backward(gy.cuda())     # layers wider than one launch's 96 columns / 24 accumulator tiles go in column blocks (linear.py)
    yc.backward(gy.double())
    # ReLU mask decided in f32 vs f64: exclude the (measure-zero) samples where the pre-activation is within rounding of 0
    assert torch.allclose(xg.grad.cpu().double(), xc.grad, atol=5e-4, rtol=1e-4)
    assert torch.allclose(wg.grad.cpu().double(), wc.grad, atol=2e-3 * max(1.0, float(wc.grad.abs().max())), rtol=1e-4)
    nb, kb = (N + 15) // 16, (K + 15) // 16
    if not (nb * kb <= 24 and kb <= 6):       # the C entry point itself refuses such a shape in ONE launch
        from lzzx_nerf_amd._lib import LzError
        from lzzx_nerf_amd._util import call, ptr, stream
        dw = torch.zeros(N, K, device="cuda")
        with pytest.raises(LzError, match="<= 24"):
            call("lz_linear_grad_w", ptr(gy.cuda()), N, None, ptr(x.cuda()), K, ptr(dw), K, M, K, N, stream())


def test_lz_linear_leading_dimensions_and_errors():
    """C ABI: column slices of wider buffers in and out (what saves the torch.cat copies), argument checks"""
    from lzzx_nerf_amd._util import call, ptr, stream
    g = torch.Generator().manual_seed(5)
    M, K, N = 1000, 36, 64
    big_in = torch.randn(M, 80, generator=g).cuda()
    big_out = torch.full((M, 100), 7.0).cuda()
    w = (torch.randn(N, K, generator=g) / 6).cuda()
    xin, yout = big_in[:, 8:], big_out[:, 16:]
    call("lz_linear_forward", ptr(xin), 80, None, ptr(w), K, ptr(yout), 100, M, K, N, 1, stream())
    ref = torch.relu(xin[:, :K].double() @ w.double().T)
    assert torch.allclose(big_out[:, 16:16 + N].double(), ref, atol=2e-5) and bool((big_out[:, :16] == 7).all()) and bool((big_out[:, 80:] == 7).all())
    gy = torch.randn(M, N, generator=g).cuda()
    dw2 = torch.zeros(N, K).cuda()
    ym = big_out[:, 16:16 + N].contiguous()   # the mask shares dY's layout (same leading dimension)
    call("lz_linear_grad_w", ptr(gy), N, ptr(ym), ptr(xin), 80, ptr(dw2), K, M, K, N, stream())
    refw = (gy.double() * (ref > 0)).T @ xin[:, :K].double()
    assert torch.allclose(dw2.double(), refw, atol=2e-3)
    with pytest.raises(RuntimeError, match="leading dimension"):
        call("lz_linear_forward", ptr(big_in), 8, None, ptr(w), K, ptr(big_out), 100, M, K, N, 0, stream())


@pytest.mark.parametrize("mlp", ["torch", "lz"])
def test_train_step_gradients(params, golden, mlp):
    from lzzx_nerf_amd import raymarching as R
    from lzzx_nerf_amd.linear import lz_linear
    from lzzx_nerf_amd.encoding import get_encoder
    torch.manual_seed(0)
    H = W = 24
    pose, intr = synthetic_camera(H, W)
    ro, rd = get_rays(pose, intr, H, W)
    bits = ellipsoid_bitfield()[0]
    spec = TriplaneSpec(1.0)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    enc_a, eye, ind = golden["net_enc_a"], golden["net_eye"], golden["net_ind"]
    # ---------------- GPU: operator path ----------------
    encs = []
    for n in ("xy", "yz", "xz"):
        e, _ = get_encoder("hashgrid", input_dim=2, num_levels=12, level_dim=1, base_resolution=64, log2_hashmap_size=14, desired_resolution=512)
        e = e.cuda()
        e.embeddings.data.copy_(dev(params[f"encoder_{n}.embeddings"]))
        encs.append(e)
    enc_dir, _ = get_encoder("spherical_harmonics")
    Wg = {k: dev(v).requires_grad_(True) for k, v in params.items() if k.endswith(".weight")}
    lin = torch.nn.functional.linear
    aabb = dev(np.array([-1, -0.5, -1, 1, 0.5, 1], np.float32))
    nears, fars = R.near_far_from_aabb(dev(ro), dev(rd), aabb, 0.05)
    ctr = torch.zeros(2, dtype=torch.int32, device="cuda")
    xyzs, dirs, deltas, rays = R.march_rays_train(dev(ro), dev(rd), 1.0, dev(bits), 1, 128, nears, fars, ctr, -1, False, 128, True, 1 / 256, 32)
    M = int(ctr[0])
    assert M > 500
    x = xyzs.contiguous()

    def mlp_(h, name, n):
        for i in range(n):
            if mlp == "lz":   # hand-written MFMA Linear (csrc/lz_linear.hip), ReLU fused
                h = lz_linear(h, Wg[f"{name}.net.{i}.weight"], i < n - 1)
            else:
                h = lin(h, Wg[f"{name}.net.{i}.weight"])
                if i < n - 1:
                    h = torch.relu(h)
        return h

    enc_x = torch.cat([encs[0](x[:, :2], bound=1), encs[1](x[:, 1:], bound=1), encs[2](x[:, [0, 2]], bound=1)], -1)
    att = mlp_(enc_x, "aud_ch_att_net", 2)
    eye_att = torch.sigmoid(mlp_(enc_x, "eye_att_net", 2))
    h = mlp_(torch.cat([enc_x, dev(enc_a) * att, dev(eye) * eye_att], -1), "sigma_net", 3)
    sigma = torch.exp(h[:, 0])
    rgb = torch.sigmoid(mlp_(torch.cat([enc_dir(dirs), h[:, 1:], dev(ind).repeat(x.shape[0], 1)], -1), "color_net", 2)) * 1.002 - 0.001
    unc = torch.log(1 + torch.exp(mlp_(enc_x.detach(), "unc_net", 2)))
    ws, a0s, a1s, us, dep, img = R.composite_rays_train_triplane(sigma, rgb, att.norm(dim=-1), eye_att.abs().sum(-1), unc[:, 0], deltas, rays)
    target = torch.linspace(0, 1, H * W * 3, device="cuda").reshape(-1, 3)
    loss = ((img - target) ** 2).mean() + 0.1 * ws.mean() + 1e-3 * a0s.mean() + 1e-3 * a1s.mean() + 1e-2 * us.mean()
    loss.backward()
    # ---------------- CPU: float64 model of the same math ----------------
    dd = lambda a: torch.from_numpy(np.ascontiguousarray(a)).double()
    E = [dd(params[f"encoder_{n}.embeddings"]).requires_grad_(True) for n in ("xy", "yz", "xz")]
    Wc = {k: dd(v).requires_grad_(True) for k, v in params.items() if k.endswith(".weight")}
    sc, rs = O.grid_level_params(12, np.float32(np.log2(spec.per_level_scale)), 64)
    xc = dd(xyzs.cpu().numpy())
    x01 = (xc + 1) / 2

    def mlpc(h, name, n):
        for i in range(n):
            h = h @ Wc[f"{name}.net.{i}.weight"].T
            if i < n - 1:
                h = torch.relu(h)
        return h

    enc_xc = torch.cat([_grid64(x01[:, [0, 1]], E[0], spec.offsets, sc, rs), _grid64(x01[:, [1, 2]], E[1], spec.offsets, sc, rs),
                        _grid64(x01[:, [0, 2]], E[2], spec.offsets, sc, rs)], -1)
    # f32 rounding of pos = x * 511 + 0.5 at the finest level is ~3e-5 cells, times a table slope of up to 2 per cell
    assert np.allclose(enc_xc.detach().numpy(), enc_x.detach().cpu().numpy(), atol=1e-4)
    attc = mlpc(enc_xc, "aud_ch_att_net", 2)
    eyec = torch.sigmoid(mlpc(enc_xc, "eye_att_net", 2))
    hc = mlpc(torch.cat([enc_xc, dd(enc_a) * attc, dd(eye) * eyec], -1), "sigma_net", 3)
    sigc = torch.exp(hc[:, 0])
    shc = dd(O.sh_encode_forward(dirs.cpu().numpy(), 4)[0])
    rgbc = torch.sigmoid(mlpc(torch.cat([shc, hc[:, 1:], dd(ind).repeat(xc.shape[0], 1)], -1), "color_net", 2)) * 1.002 - 0.001
    uncc = torch.log(1 + torch.exp(mlpc(enc_xc.detach(), "unc_net", 2)))[:, 0]
    dl = dd(deltas.cpu().numpy())
    rays_np = rays.cpu().numpy()
    N = rays_np.shape[0]
    imgs, wss, a0c, a1c, usc = [None] * N, [None] * N, [None] * N, [None] * N, [None] * N
    zero = torch.zeros((), dtype=torch.float64)
    for n in range(N):
        i, o, c = [int(v) for v in rays_np[n]]
        T, r, w_, a0_, a1_, u_ = 1.0, torch.zeros(3, dtype=torch.float64), zero, zero, zero, zero
        for s in range(o, o + c):
            alpha = 1 - torch.exp(-sigc[s] * dl[s, 0])
            wgt = alpha * T
            r = r + wgt * rgbc[s]
            w_ = w_ + wgt
            a0_ = a0_ + attc[s].norm()
            a1_ = a1_ + eyec[s].abs().sum()
            u_ = u_ + wgt * uncc[s]
            T = T * (1 - alpha)
            if float(T.detach()) < 1e-4:
                break
        imgs[i], wss[i], a0c[i], a1c[i], usc[i] = r, w_, a0_, a1_, u_
    imgc = torch.stack(imgs)
    lossc = ((imgc - target.cpu().double()) ** 2).mean() + 0.1 * torch.stack(wss).mean() + 1e-3 * torch.stack(a0c).mean() + \
        1e-3 * torch.stack(a1c).mean() + 1e-2 * torch.stack(usc).mean()
    lossc.backward()
    assert float(loss) == pytest.approx(float(lossc), rel=1e-5)

    def close(g_gpu, g_cpu, name):
        a, b = g_gpu.detach().cpu().double().numpy(), g_cpu.numpy()
        scale = max(np.abs(b).max(), 1e-12)
        assert np.max(np.abs(a - b)) / scale < 2e-3, (name, np.max(np.abs(a - b)) / scale)

    for k in Wg:
        close(Wg[k].grad, Wc[k].grad, k)
    for e, g, n in zip(encs, E, ("xy", "yz", "xz")):
        close(e.embeddings.grad, g.grad, "encoder_" + n)
        assert float(e.embeddings.grad.abs().sum()) > 0


def test_fused_train_head_gradients(params, golden):
    """FusedTriplaneTrainHead: forward = the fused head kernel in training mode (bit-exact against the checker), backward = ONE
    kernel for the data-gradient chain + per-layer weight-gradient reductions + LDS grid scatter.  Every gradient against the float64
    model of the whole step (same model as test_train_step_gradients)."""
    from lzzx_nerf_amd import raymarching as R
    from lzzx_nerf_amd.head_train import FusedTriplaneTrainHead
    from oracle.head import head_forward
    H = W = 24
    pose, intr = synthetic_camera(H, W)
    ro, rd = get_rays(pose, intr, H, W)
    bits = ellipsoid_bitfield()[0]
    spec = TriplaneSpec(1.0)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    enc_a, eye, ind = golden["net_enc_a"], golden["net_eye"], golden["net_ind"]
    net = FusedTriplaneTrainHead({k: v for k, v in params.items()}, bound=1.0).cuda()
    aabb = dev(np.array([-1, -0.5, -1, 1, 0.5, 1], np.float32))
    nears, fars = R.near_far_from_aabb(dev(ro), dev(rd), aabb, 0.05)
    ctr = torch.zeros(2, dtype=torch.int32, device="cuda")
    xyzs, dirs, deltas, rays = R.march_rays_train(dev(ro), dev(rd), 1.0, dev(bits), 1, 128, nears, fars, ctr, -1, False, 128, True, 1 / 256, 32)
    enc_a_t, ind_t = dev(enc_a).requires_grad_(True), dev(ind).requires_grad_(True)
    sigma, rgb, aa, ae, unc = net(xyzs.contiguous(), dirs.contiguous(), enc_a_t, ind_t, dev(eye))
    # forward: the training-mode head, bit for bit
    so, ro_, ao, eo, uo = head_forward(spec, params, xyzs.cpu().numpy(), dirs.cpu().numpy(), enc_a, ind, eye, testing=False)
    assert np.array_equal(sigma.detach().cpu().numpy(), so) and np.array_equal(rgb.detach().cpu().numpy(), ro_)
    assert np.array_equal(unc.detach().cpu().numpy(), uo) and np.array_equal(aa.detach().cpu().numpy(), ao)
    ws, a0s, a1s, us, dep, img = R.composite_rays_train_triplane(sigma, rgb, aa[:, 0], ae[:, 0], unc[:, 0], deltas, rays)
    target = torch.linspace(0, 1, H * W * 3, device="cuda").reshape(-1, 3)
    loss = ((img - target) ** 2).mean() + 0.1 * ws.mean() + 1e-3 * a0s.mean() + 1e-3 * a1s.mean() + 1e-2 * us.mean()
    loss.backward()
    # ---------------- float64 model (as in test_train_step_gradients) ----------------
    dd = lambda a: torch.from_numpy(np.ascontiguousarray(a)).double()
    E = [dd(params[f"encoder_{n}.embeddings"]).requires_grad_(True) for n in ("xy", "yz", "xz")]
    Wc = {k: dd(v).requires_grad_(True) for k, v in params.items() if k.endswith(".weight")}
    ea_c, ind_c = dd(enc_a).requires_grad_(True), dd(ind).requires_grad_(True)
    sc, rs = O.grid_level_params(12, np.float32(np.log2(spec.per_level_scale)), 64)
    xc = dd(xyzs.cpu().numpy())
    x01 = (xc + 1) / 2

    def mlpc(h, name, n):
        for i in range(n):
            h = h @ Wc[f"{name}.net.{i}.weight"].T
            if i < n - 1:
                h = torch.relu(h)
        return h

    enc_xc = torch.cat([_grid64(x01[:, [0, 1]], E[0], spec.offsets, sc, rs), _grid64(x01[:, [1, 2]], E[1], spec.offsets, sc, rs),
                        _grid64(x01[:, [0, 2]], E[2], spec.offsets, sc, rs)], -1)
    attc = mlpc(enc_xc, "aud_ch_att_net", 2)
    eyec = torch.sigmoid(mlpc(enc_xc, "eye_att_net", 2))
    hc = mlpc(torch.cat([enc_xc, ea_c * attc, dd(eye) * eyec], -1), "sigma_net", 3)
    sigc = torch.exp(hc[:, 0])
    shc = dd(O.sh_encode_forward(dirs.cpu().numpy(), 4)[0])
    rgbc = torch.sigmoid(mlpc(torch.cat([shc, hc[:, 1:], ind_c.repeat(xc.shape[0], 1)], -1), "color_net", 2)) * 1.002 - 0.001
    uncc = torch.log(1 + torch.exp(mlpc(enc_xc.detach(), "unc_net", 2)))[:, 0]
    dl = dd(deltas.cpu().numpy())
    rays_np = rays.cpu().numpy()
    N = rays_np.shape[0]
    imgs, wss, a0c, a1c, usc = [None] * N, [None] * N, [None] * N, [None] * N, [None] * N
    zero = torch.zeros((), dtype=torch.float64)
    for n in range(N):
        i, o, c = [int(v) for v in rays_np[n]]
        T, r, w_, a0_, a1_, u_ = 1.0, torch.zeros(3, dtype=torch.float64), zero, zero, zero, zero
        for s in range(o, o + c):
            alpha = 1 - torch.exp(-sigc[s] * dl[s, 0])
            wgt = alpha * T
            r = r + wgt * rgbc[s]
            w_ = w_ + wgt
            a0_ = a0_ + attc[s].norm()
            a1_ = a1_ + eyec[s].abs().sum()
            u_ = u_ + wgt * uncc[s]
            T = T * (1 - alpha)
            if float(T.detach()) < 1e-4:
                break
        imgs[i], wss[i], a0c[i], a1c[i], usc[i] = r, w_, a0_, a1_, u_
    lossc = ((torch.stack(imgs) - target.cpu().double()) ** 2).mean() + 0.1 * torch.stack(wss).mean() + 1e-3 * torch.stack(a0c).mean() + \
        1e-3 * torch.stack(a1c).mean() + 1e-2 * torch.stack(usc).mean()
    lossc.backward()
    assert float(loss) == pytest.approx(float(lossc), rel=1e-5)

    def close(g_gpu, g_cpu, name, tol=2e-3):
        a, b = g_gpu.detach().cpu().double().numpy(), g_cpu.numpy()
        scale = max(np.abs(b).max(), 1e-12)
        assert np.max(np.abs(a - b)) / scale < tol, (name, np.max(np.abs(a - b)) / scale)

    sd = dict(net.named_parameters())
    for k in Wc:
        close(sd[k].grad, Wc[k].grad, k)
    for n, g in zip(("xy", "yz", "xz"), E):
        close(sd[f"encoder_{n}.embeddings"].grad, g.grad, "encoder_" + n)
    close(enc_a_t.grad, ea_c.grad, "enc_a")
    close(ind_t.grad, ind_c.grad, "ind_code")


@pytest.mark.parametrize("exp_eye,ind_dim", [(False, 0), (True, 0), (False, 4)])
def test_fused_train_head_variants_match_operator_graph(params, golden, exp_eye, ind_dim):
    """exp_eye off / no individual code: the fused forward + backward against the same network built from the operator API
    (GridEncoder + SHEncoder + torch Linear under autograd) on the GPU, f32 vs f32"""
    from lzzx_nerf_amd.encoding import get_encoder
    from lzzx_nerf_amd.head_train import FusedTriplaneTrainHead
    rng = np.random.default_rng(3)
    p = dict(params)
    p["sigma_net.net.0.weight"] = np.ascontiguousarray(params["sigma_net.net.0.weight"][:, :68 + int(exp_eye)])
    p["color_net.net.0.weight"] = np.ascontiguousarray(params["color_net.net.0.weight"][:, :80 + ind_dim])
    net = FusedTriplaneTrainHead(p, bound=1.0, exp_eye=exp_eye, ind_dim=ind_dim).cuda()
    M = 4096 + 48
    xyz = torch.from_numpy(rng.uniform(-1, 1, (M, 3)).astype(np.float32)).cuda()
    d = torch.nn.functional.normalize(torch.from_numpy(rng.normal(size=(M, 3)).astype(np.float32)), dim=-1).cuda()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    enc_a, eye, ind = dev(golden["net_enc_a"]), dev(golden["net_eye"]) if exp_eye else None, dev(golden["net_ind"]) if ind_dim else None
    gout = [torch.from_numpy(rng.normal(size=sh).astype(np.float32)).cuda() for sh in ((M,), (M, 3), (M, 1), (M, 1), (M, 1))]
    outs = net(xyz, d, enc_a, ind, eye)
    torch.autograd.backward([o for o, g in zip(outs, gout) if o.requires_grad], [g for o, g in zip(outs, gout) if o.requires_grad])
    # the same network from operators
    encs = []
    for n in ("xy", "yz", "xz"):
        e = get_encoder("hashgrid", input_dim=2, num_levels=12, level_dim=1, base_resolution=64, log2_hashmap_size=14, desired_resolution=512)[0].cuda()
        e.embeddings.data.copy_(dev(p[f"encoder_{n}.embeddings"]))
        encs.append(e)
    sh = get_encoder("spherical_harmonics")[0]
    Wg = {k: dev(v).requires_grad_(True) for k, v in p.items() if k.endswith(".weight")}
    lin = torch.nn.functional.linear

    def mlp(h, name, n):
        for i in range(n):
            h = lin(h, Wg[f"{name}.net.{i}.weight"])
            if i < n - 1:
                h = torch.relu(h)
        return h

    enc_x = torch.cat([encs[0](xyz[:, :2], bound=1), encs[1](xyz[:, 1:], bound=1), encs[2](xyz[:, [0, 2]], bound=1)], -1)
    att = mlp(enc_x, "aud_ch_att_net", 2)
    parts = [enc_x, enc_a * att]
    if exp_eye:
        eye_att = torch.sigmoid(mlp(enc_x, "eye_att_net", 2))
        parts.append(eye * eye_att)
    h = mlp(torch.cat(parts, -1), "sigma_net", 3)
    cin = [sh(d), h[:, 1:]] + ([ind.repeat(M, 1)] if ind_dim else [])
    ref = [torch.exp(h[:, 0]), torch.sigmoid(mlp(torch.cat(cin, -1), "color_net", 2)) * 1.002 - 0.001, att.norm(dim=-1, keepdim=True),
           eye_att if exp_eye else None, torch.nn.functional.softplus(mlp(enc_x.detach(), "unc_net", 2))]
    for o, r in zip(outs, ref):
        if r is not None:
            assert torch.allclose(o, r, rtol=2e-4, atol=2e-5)
    torch.autograd.backward([r for r in ref if r is not None], [g for r, g in zip(ref, gout) if r is not None])
    sd = dict(net.named_parameters())
    for k, wg in Wg.items():
        if not exp_eye and k.startswith("eye_att_net"):
            continue
        a, b = sd[k].grad, wg.grad
        assert float((a - b).abs().max()) <= 2e-3 * max(float(b.abs().max()), 1e-6), k
    for n, e in zip(("xy", "yz", "xz"), encs):
        a, b = sd[f"encoder_{n}.embeddings"].grad, e.embeddings.grad
        assert float((a - b).abs().max()) <= 2e-3 * max(float(b.abs().max()), 1e-6), n


def test_fused_train_head_gradient_bucket_sharded_step(params, golden):
    """Data-parallel arrangement (training variant) in one process: gradients of two ray shards accumulated into the flat
    GradientBucket (every .grad a view of one buffer, what the ONE all-reduce per step operates on) equal the full-batch gradients
    of the summed loss, and backward through the fused kernels keeps the views attached."""
    from lzzx_nerf_amd import raymarching as R
    from lzzx_nerf_amd.dist import GradientBucket, shard_bounds
    from lzzx_nerf_amd.head_train import FusedTriplaneTrainHead
    H = W = 24
    pose, intr = synthetic_camera(H, W)
    ro, rd = get_rays(pose, intr, H, W)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    ro, rd, bits = dev(ro), dev(rd), dev(ellipsoid_bitfield()[0])
    enc_a, eye, ind = dev(golden["net_enc_a"]), dev(golden["net_eye"]), dev(golden["net_ind"])
    aabb = dev(np.array([-1, -0.5, -1, 1, 0.5, 1], np.float32))
    target = torch.linspace(0, 1, H * W * 3, device="cuda").reshape(-1, 3)

    def shard_loss(net, lo, hi):
        o, d = ro[lo:hi].contiguous(), rd[lo:hi].contiguous()
        nears, fars = R.near_far_from_aabb(o, d, aabb, 0.05)
        ctr = torch.zeros(2, dtype=torch.int32, device="cuda")
        xyzs, dirs, deltas, rays = R.march_rays_train(o, d, 1.0, bits, 1, 128, nears, fars, ctr, -1, False, 128, True, 1 / 256, 32)
        sigma, rgb, aa, ae, unc = net(xyzs.contiguous(), dirs.contiguous(), enc_a, ind, eye)
        ws, a0s, a1s, us, dep, img = R.composite_rays_train_triplane(sigma, rgb, aa[:, 0], ae[:, 0], unc[:, 0], deltas, rays)
        return ((img - target[lo:hi]) ** 2).sum() + 0.1 * ws.sum() + 1e-2 * us.sum()

    n = H * W
    full = FusedTriplaneTrainHead({k: v for k, v in params.items()}, bound=1.0).cuda()
    shard_loss(full, 0, n).backward()
    net = FusedTriplaneTrainHead({k: v for k, v in params.items()}, bound=1.0).cuda()
    bucket = GradientBucket(net.parameters())
    lo_hi = [shard_bounds(n, r, 2) for r in range(2)]
    for lo, hi in lo_hi:
        shard_loss(net, lo, hi).backward()
    end = bucket.flat.data_ptr() + bucket.flat.numel() * 4
    for (name, p), q in zip(net.named_parameters(), full.parameters()):
        assert bucket.flat.data_ptr() <= p.grad.data_ptr() < end, name      # still a view of the flat buffer
        scale = float(q.grad.abs().max()) + 1e-20
        assert float((p.grad - q.grad).abs().max()) <= 2e-5 * scale, name   # same sums, different association of the reduction
    assert float(bucket.flat.abs().sum()) > 0
    assert torch.equal(bucket.all_reduce(), bucket.flat)                     # single process: no-op
    bucket.zero()
    assert all(float(p.grad.abs().sum()) == 0.0 for p in net.parameters())


@pytest.mark.parametrize("M,k_sig0", [(1, 69), (15, 68), (1000, 69), (70001, 69)])
def test_head_grad_w_products_match_float64(M, k_sig0):
    """lz_triplane_head_grad_w on random records: the five products (one pass, partial tiles per workgroup, second launch sums them)
    against float64 matmuls of the same column slots; ragged sample counts (tail groups read record 0 with a zero factor)."""
    from lzzx_nerf_amd import _lib
    from lzzx_nerf_amd._util import call, ptr, stream
    REC = 656
    col = dict(X_A1=0, X_SIG0=64, X_S1=144, X_S2C=208, G_X=304, G_ATT=416, G_S1=448, G_S2=512, G_C1H=576)
    g = torch.Generator(device="cuda").manual_seed(M)
    rec = torch.randn(M, REC, device="cuda", generator=g)
    rec[:, col["X_SIG0"] + 69: col["X_S1"]] = float("nan")      # slot padding is never read into a written output
    rec[:, col["G_C1H"] + 65:] = float("nan")
    # the kernels keep records blocked by 16-sample slice, [slice][tile of 16 columns][sample][16] (lz_head_bwd_common.h); rows past M
    # of the last slice are never read
    Mb = (M + 15) // 16 * 16
    padded = torch.full((Mb, REC), float("nan"), device="cuda")
    padded[:M] = rec
    rec_rows, rec = rec, padded.view(Mb // 16, 16, REC // 16, 16).permute(0, 2, 1, 3).contiguous()
    shapes = dict(x3=(112, 36), aud1=(32, 64), sig0=(64, k_sig0), sig1=(64, 64), c1h=(65, 84))
    out = {n: torch.full(sh, 7.0, device="cuda") for n, sh in shapes.items()}
    ws = torch.empty(_lib.load().lz_triplane_head_grad_w_workspace() // 4, device="cuda")
    call("lz_triplane_head_grad_w", ptr(rec), M, k_sig0, *[ptr(out[n]) for n in ("x3", "aud1", "sig0", "sig1", "c1h")], ptr(ws), stream())
    r = rec_rows.double()
    sl = lambda name, w: r[:, col[name]: col[name] + w]
    want = dict(x3=sl("G_X", 112).T @ sl("X_SIG0", 36), aud1=sl("G_ATT", 32).T @ sl("X_A1", 64), sig0=sl("G_S1", 64).T @ sl("X_SIG0", k_sig0),
                sig1=sl("G_S2", 64).T @ sl("X_S1", 64), c1h=sl("G_C1H", 65).T @ sl("X_S2C", 84))
    for n in shapes:
        got = out[n].double()
        assert torch.isfinite(got).all(), n
        assert float((got - want[n]).abs().max()) <= 2e-5 * float(want[n].abs().max()) + 1e-6, n
    # deterministic: no atomics anywhere in the reduction
    out2 = {n: torch.empty(sh, device="cuda") for n, sh in shapes.items()}
    call("lz_triplane_head_grad_w", ptr(rec), M, k_sig0, *[ptr(out2[n]) for n in ("x3", "aud1", "sig0", "sig1", "c1h")], ptr(ws), stream())
    assert all(torch.equal(out[n], out2[n]) for n in shapes)
    with pytest.raises(RuntimeError):
        call("lz_triplane_head_grad_w", ptr(rec), M, 70, *[ptr(out[n]) for n in ("x3", "aud1", "sig0", "sig1", "c1h")], ptr(ws), stream())


@pytest.mark.parametrize("M", [0, 1, 5, 17])
def test_fused_train_head_tiny_batches(params, golden, M):
    """sample counts below one 16-row slice (and none at all: a batch of rays that misses the box) through forward + backward:
    outputs and every gradient against the same head fed with the batch padded to 64 rows whose padding gets zero upstream gradient"""
    from lzzx_nerf_amd.head_train import FusedTriplaneTrainHead
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    g = torch.Generator(device="cuda").manual_seed(11)
    xyz = (torch.rand(64, 3, device="cuda", generator=g) * 2 - 1) * torch.tensor([1.0, 0.5, 1.0], device="cuda")
    dirs = torch.nn.functional.normalize(torch.randn(64, 3, device="cuda", generator=g), dim=-1)
    up = [torch.randn(64, device="cuda", generator=g), torch.randn(64, 3, device="cuda", generator=g)] + \
         [torch.randn(64, 1, device="cuda", generator=g) for _ in range(3)]
    enc_a, eye, ind = dev(golden["net_enc_a"]), dev(golden["net_eye"]), dev(golden["net_ind"])

    def run(n_rows, n_live):
        net = FusedTriplaneTrainHead({k: v for k, v in params.items()}, bound=1.0).cuda()
        ea, ic = enc_a.clone().requires_grad_(True), ind.clone().requires_grad_(True)
        outs = net(xyz[:n_rows].contiguous(), dirs[:n_rows].contiguous(), ea, ic, eye)
        loss = sum((o[:n_live] * u[:n_live]).sum() for o, u in zip(outs, up))
        loss.backward()
        grads = [p.grad if p.grad is not None else torch.zeros_like(p) for p in net.parameters()]
        return [o[:n_live].detach() for o in outs], grads + [ea.grad if ea.grad is not None else torch.zeros_like(ea),
                                                              ic.grad if ic.grad is not None else torch.zeros_like(ic)]

    out_s, g_s = run(M, M)
    out_p, g_p = run(64, M)
    for a, b in zip(out_s, out_p):
        assert torch.equal(a, b)
    for a, b in zip(g_s, g_p):
        assert a.shape == b.shape and float((a - b).abs().max()) <= 1e-5 * (float(b.abs().max()) + 1e-12) + 1e-12


@pytest.mark.parametrize("exp_eye,ind_dim", [(True, 4), (False, 0)])
def test_fused_train_head_record_equals_recompute(params, golden, exp_eye, ind_dim):
    """record=True (forward writes the layer inputs and a state row, backward starts from them) against record=False (backward
    recomputes the forward): same outputs bit for bit, d loss / d enc_x (last_denc: one plain store per sample) and the wide layers'
    weight gradients bit for bit (the per-sample records are the same and their reduction is deterministic), everything that ends in
    float atomics to 1e-5 of its largest entry"""
    from lzzx_nerf_amd.head_train import FusedTriplaneTrainHead
    rng = np.random.default_rng(11)
    p = dict(params)
    p["sigma_net.net.0.weight"] = np.ascontiguousarray(params["sigma_net.net.0.weight"][:, :68 + int(exp_eye)])
    p["color_net.net.0.weight"] = np.ascontiguousarray(params["color_net.net.0.weight"][:, :80 + ind_dim])
    M = 16 * 700 + 5
    xyz = torch.from_numpy(rng.uniform(-1, 1, (M, 3)).astype(np.float32)).cuda()
    d = torch.nn.functional.normalize(torch.from_numpy(rng.normal(size=(M, 3)).astype(np.float32)), dim=-1).cuda()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    gout = [torch.from_numpy(rng.normal(size=sh).astype(np.float32)).cuda() for sh in ((M,), (M, 3), (M, 1), (M, 1), (M, 1))]
    res = []
    for record in (True, False):
        net = FusedTriplaneTrainHead(p, bound=1.0, exp_eye=exp_eye, ind_dim=ind_dim, record=record).cuda()
        net.keep_denc = True
        enc_a = dev(golden["net_enc_a"]).requires_grad_(True)
        eye = dev(golden["net_eye"]) if exp_eye else None
        ind = dev(golden["net_ind"]).requires_grad_(True) if ind_dim else None
        outs = net(xyz, d, enc_a, ind, eye)
        torch.autograd.backward([o for o, g in zip(outs, gout) if o.requires_grad], [g for o, g in zip(outs, gout) if o.requires_grad])
        grads = {k: v.grad for k, v in net.named_parameters() if v.grad is not None}
        grads["enc_a"] = enc_a.grad
        if ind is not None:
            grads["ind"] = ind.grad
        res.append(([o.detach() for o in outs], grads, net.last_denc))
    (o1, g1, denc1), (o2, g2, denc2) = res
    for a, b in zip(o1, o2):
        assert torch.equal(a, b)
    assert denc1 is not None and denc1.shape == (3, 12, M)
    assert torch.equal(denc1, denc2)
    assert g1.keys() == g2.keys()
    exact = ("aud_ch_att_net.net.0.weight", "aud_ch_att_net.net.1.weight", "sigma_net.net.0.weight", "sigma_net.net.1.weight", "unc_net.net.0.weight")
    for k in g1:
        if k in exact:
            assert torch.equal(g1[k], g2[k]), k
        else:
            scale = float(g2[k].abs().max()) + 1e-30
            assert float((g1[k] - g2[k]).abs().max()) / scale < 1e-5, k


@pytest.mark.parametrize("exp_eye,ind_dim", [(True, 4), (False, 0)])
def test_fused_train_head_f16_records(params, golden, exp_eye, ind_dim):
    """record_dtype="f16": the operands of the weight-gradient products go through memory in half (the reference's autocast dW GEMMs
    see the same rounding), everything else is f32.  Outputs and the data gradients (tables, enc_a, ind_code) equal the f32-record run
    (bit for bit / to atomic order); the weight gradients to 1e-3 of their largest entry (per-term rounding 2^-11, summed over M)."""
    from lzzx_nerf_amd.head_train import FusedTriplaneTrainHead
    rng = np.random.default_rng(12)
    p = dict(params)
    p["sigma_net.net.0.weight"] = np.ascontiguousarray(params["sigma_net.net.0.weight"][:, :68 + int(exp_eye)])
    p["color_net.net.0.weight"] = np.ascontiguousarray(params["color_net.net.0.weight"][:, :80 + ind_dim])
    for n in ("xy", "yz", "xz"):   # the fixture's tables are at their initial scale (1e-4): half-precision records want trained-size features
        p[f"encoder_{n}.embeddings"] = params[f"encoder_{n}.embeddings"] * np.float32(100.0)
    M = 16 * 900 + 3
    xyz = torch.from_numpy(rng.uniform(-1, 1, (M, 3)).astype(np.float32)).cuda()
    d = torch.nn.functional.normalize(torch.from_numpy(rng.normal(size=(M, 3)).astype(np.float32)), dim=-1).cuda()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    gout = [torch.from_numpy(rng.normal(size=sh).astype(np.float32)).cuda() for sh in ((M,), (M, 3), (M, 1), (M, 1), (M, 1))]
    res = []
    for dt in ("f32", "f16"):
        net = FusedTriplaneTrainHead(p, bound=1.0, exp_eye=exp_eye, ind_dim=ind_dim, record_dtype=dt).cuda()
        enc_a = dev(golden["net_enc_a"]).requires_grad_(True)
        eye = dev(golden["net_eye"]) if exp_eye else None
        ind = dev(golden["net_ind"]).requires_grad_(True) if ind_dim else None
        outs = net(xyz, d, enc_a, ind, eye)
        torch.autograd.backward([o for o, g in zip(outs, gout) if o.requires_grad], [g for o, g in zip(outs, gout) if o.requires_grad])
        grads = {k: v.grad for k, v in net.named_parameters() if v.grad is not None}
        grads["enc_a"] = enc_a.grad
        if ind is not None:
            grads["ind"] = ind.grad
        res.append(([o.detach() for o in outs], grads))
    (o1, g1), (o2, g2) = res
    for a, b in zip(o1, o2):
        assert torch.equal(a, b)
    assert g1.keys() == g2.keys()
    for k in g1:
        data_path = k.startswith("encoder_") or k in ("enc_a", "ind")
        scale = float(g1[k].abs().max()) + 1e-30
        err = float((g1[k] - g2[k]).abs().max()) / scale
        assert err < (1e-5 if data_path else 1e-3), (k, err)
        if not data_path and (exp_eye or not k.startswith("eye_att_net")):
            assert float(g2[k].abs().max()) > 0, k


@pytest.mark.parametrize("backward_dtype,exp_eye,ind_dim", [("f32", True, 4), ("f16", True, 4), ("f16", False, 0), ("f16", True, 0)])
def test_fused_train_head_f16_forward(params, golden, backward_dtype, exp_eye, ind_dim):
    """forward_dtype="f16": the training forward in the reference's autocast arithmetic (lz_head_rec16.hip) + data-gradient chain (f32, or
    backward_dtype="f16": on the f16 matrix cores with half dY / W like autocast's own backward) + half records.  Checked against the same network built from the operator API under torch.autocast (what the reference's `-O`
    training runs: half Linear on rocBLAS, half ReLU / sigmoid / products, f32 exp / norm / softplus, half gradients): outputs to half
    rounding, every gradient to 2e-2 of its largest entry; and against the f16 inference kernel for the outputs they share."""
    from lzzx_nerf_amd.encoding import get_encoder
    from lzzx_nerf_amd.head import FusedTriplaneHead
    from lzzx_nerf_amd.head_train import FusedTriplaneTrainHead
    rng = np.random.default_rng(13)
    p = dict(params)
    p["sigma_net.net.0.weight"] = np.ascontiguousarray(params["sigma_net.net.0.weight"][:, :68 + int(exp_eye)])
    p["color_net.net.0.weight"] = np.ascontiguousarray(params["color_net.net.0.weight"][:, :80 + ind_dim])
    for n in ("xy", "yz", "xz"):
        p[f"encoder_{n}.embeddings"] = params[f"encoder_{n}.embeddings"] * np.float32(30.0)
    M = 16 * 800 + 7
    xyz = torch.from_numpy(rng.uniform(-1, 1, (M, 3)).astype(np.float32)).cuda()
    d = torch.nn.functional.normalize(torch.from_numpy(rng.normal(size=(M, 3)).astype(np.float32)), dim=-1).cuda()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    gout = [torch.from_numpy(rng.normal(size=sh).astype(np.float32)).cuda() for sh in ((M,), (M, 3), (M, 1), (M, 1), (M, 1))]
    gout[0] *= 1e-2   # d loss / d sigma times sigma has to fit a half: the job of the reference's GradScaler
    enc_a_np = golden["net_enc_a"].astype(np.float16).astype(np.float32)   # enc_a is a half tensor under autocast (AudioNet output)
    net = FusedTriplaneTrainHead(p, bound=1.0, exp_eye=exp_eye, ind_dim=ind_dim, forward_dtype="f16", backward_dtype=backward_dtype).cuda()
    enc_a = dev(enc_a_np).requires_grad_(True)
    ind = dev(golden["net_ind"]).requires_grad_(True) if ind_dim else None
    eye = dev(golden["net_eye"]) if exp_eye else None
    outs = net(xyz, d, enc_a, ind, eye)
    live = [k for k in range(5) if outs[k].requires_grad]
    torch.autograd.backward([outs[k] for k in live], [gout[k] for k in live])
    # ---- the f16 inference kernel: the same rounding sequence, but since round 5 on v_mfma_f32_32x32x16_f16 (lz_head_f16w_slice.h): the f32
    # accumulation inside a Linear is grouped by 16 k instead of the recording forward's 32 (v_mfma_f32_16x16x32_f16), which the reference
    # leaves to its GEMM library -- so the two agree to half rounding: the bulk bit-equal, the rest within a few half ulps (rounds 2-4 shared
    # one slice and agreed bit for bit)
    pi = dict(p) if ind_dim else {k: v for k, v in p.items() if k != "individual_codes"}
    inf = FusedTriplaneHead({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in pi.items()}, bound=1.0, exp_eye=exp_eye, precision="f16")
    oi = inf.forward(xyz, d, dev(enc_a_np), dev(golden["net_ind"]) if ind_dim else None, eye)
    for a, b, nm in zip(outs[:4], oi[:4], ("sigma", "rgb", "amb_aud", "amb_eye")):
        if nm == "amb_eye" and not exp_eye:
            continue
        a, b = a.detach().reshape(-1), b.reshape(-1)
        rel = (a - b).abs() / (b.abs() + 1e-3)
        # (||att|| is an f32 sum of 32 squares whose order differs too -- 16 + 16 over two lanes against 8 x 4 over four: equal to f32 rounding)
        same = float((a == b).float().mean()) if nm != "amb_aud" else float((rel < 1e-6).float().mean())
        assert same > 0.9 and float(rel.max()) < 2e-2, (nm, same, float(rel.max()))
    # ---- the operator graph under autocast
    encs = []
    for n in ("xy", "yz", "xz"):
        e = get_encoder("hashgrid", input_dim=2, num_levels=12, level_dim=1, base_resolution=64, log2_hashmap_size=14, desired_resolution=512)[0].cuda()
        e.embeddings.data.copy_(dev(p[f"encoder_{n}.embeddings"]))
        encs.append(e)
    sh = get_encoder("spherical_harmonics")[0]
    Wg = {k: dev(v).requires_grad_(True) for k, v in p.items() if k.endswith(".weight")}
    ea_r = dev(enc_a_np).requires_grad_(True)
    ind_r = dev(golden["net_ind"]).requires_grad_(True) if ind_dim else None

    def mlp(h, name, n):
        for i in range(n):
            h = torch.nn.functional.linear(h, Wg[f"{name}.net.{i}.weight"])
            if i < n - 1:
                h = torch.relu(h)
        return h

    with torch.autocast("cuda", dtype=torch.float16):
        enc_x = torch.cat([encs[0](xyz[:, :2], bound=1), encs[1](xyz[:, 1:], bound=1), encs[2](xyz[:, [0, 2]], bound=1)], -1)
        att = mlp(enc_x, "aud_ch_att_net", 2)
        eye_att = torch.sigmoid(mlp(enc_x, "eye_att_net", 2)) if exp_eye else None
        h = mlp(torch.cat([enc_x, ea_r.half() * att] + ([eye * eye_att] if exp_eye else []), -1), "sigma_net", 3)
        rgb = torch.sigmoid(mlp(torch.cat([sh(d), h[:, 1:]] + ([ind_r.repeat(M, 1)] if ind_dim else []), -1), "color_net", 2)) * 1.002 - 0.001
        ref = [torch.exp(h[:, 0]), rgb, att.norm(dim=-1, keepdim=True), eye_att, torch.nn.functional.softplus(mlp(enc_x.detach(), "unc_net", 2))]
    for o, r, nm in zip(outs, ref, ("sigma", "rgb", "amb_aud", "amb_eye", "unc")):
        if r is None:
            continue
        o, r = o.detach().reshape(-1), r.detach().float().reshape(-1)
        assert float(((o - r).abs() / (r.abs() + 1e-2)).max()) < 3e-2, nm   # a half ulp of a pre-activation through exp
        assert float(((o - r).abs() / (r.abs() + 1e-2)).mean()) < 1e-3, nm
    torch.autograd.backward([r for r in ref if r is not None], [g.to(r.dtype) for r, g in zip(ref, gout) if r is not None])
    sd = dict(net.named_parameters())

    def close(a, b, name):
        scale = float(b.float().abs().max()) + 1e-30
        err = float((a - b.float()).abs().max()) / scale
        assert err < 2e-2, (name, err)

    for k, wg in Wg.items():
        if not exp_eye and k.startswith("eye_att_net"):
            continue
        close(sd[k].grad, wg.grad, k)
    for n, e in zip(("xy", "yz", "xz"), encs):
        close(sd[f"encoder_{n}.embeddings"].grad, e.embeddings.grad, "encoder_" + n)
    close(enc_a.grad, ea_r.grad, "enc_a")
    if ind_dim:
        close(ind.grad, ind_r.grad, "ind_code")


@pytest.mark.parametrize("M", [1, 17, 33])
def test_fused_train_head_tiny_batches_all_arrangements(params, golden, M):
    """a handful of samples (one partial slice, one slice and a bit), every arrangement of the training head: the prefetch of the next
    slice and the clamped lanes of the last one must not leak into the sums.  Checked by isolation -- the same samples followed by 50
    more whose upstream gradients are zero give the same gradients -- and, for the f32 arrangements, against the recomputing pair."""
    from lzzx_nerf_amd.head_train import FusedTriplaneTrainHead
    rng = np.random.default_rng(20 + M)
    p = dict(params)
    for n in ("xy", "yz", "xz"):
        p[f"encoder_{n}.embeddings"] = params[f"encoder_{n}.embeddings"] * np.float32(30.0)
    Mx = M + 50
    xyz = torch.from_numpy(rng.uniform(-1, 1, (Mx, 3)).astype(np.float32)).cuda()
    d = torch.nn.functional.normalize(torch.from_numpy(rng.normal(size=(Mx, 3)).astype(np.float32)), dim=-1).cuda()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    gout = [torch.from_numpy(rng.normal(size=sh).astype(np.float32)).cuda() for sh in ((Mx,), (Mx, 3), (Mx, 1), (Mx, 1), (Mx, 1))]
    gout[0] *= 1e-2
    for g in gout:
        g[M:] = 0

    def run(n, **kw):
        net = FusedTriplaneTrainHead(p, bound=1.0, **kw).cuda()
        enc_a, ind = dev(golden["net_enc_a"]).requires_grad_(True), dev(golden["net_ind"]).requires_grad_(True)
        outs = net(xyz[:n].contiguous(), d[:n].contiguous(), enc_a, ind, dev(golden["net_eye"]))
        torch.autograd.backward(list(outs), [g[:n].contiguous() for g in gout])
        g = {k: v.grad for k, v in net.named_parameters()}
        g["enc_a"], g["ind"] = enc_a.grad, ind.grad
        return [o.detach() for o in outs], g

    o_ref, g_ref = run(M, record=False)
    for kw in (dict(), dict(record_dtype="f16"), dict(forward_dtype="f16"), dict(forward_dtype="f16", backward_dtype="f16")):
        o, g = run(M, **kw)
        ox, gx = run(Mx, **kw)
        for a, b in zip(o, ox):
            assert torch.equal(a, b[:M])
        for k in g:
            scale = float(g[k].abs().max()) + 1e-30
            assert float((g[k] - gx[k]).abs().max()) / scale < 1e-4, (kw, k)
        if "forward_dtype" not in kw:
            for a, b in zip(o, o_ref):
                assert torch.equal(a, b)
            for k in g_ref:
                scale = float(g_ref[k].abs().max()) + 1e-30
                assert float((g[k] - g_ref[k]).abs().max()) / scale < (2e-3 if kw else 1e-5), (kw, k)


@pytest.mark.parametrize("M", [1, 17, 16 * 8 + 5, 16 * 8 * 3, 16 * 8 * 256 + 16 * 3 + 9, 120001])
@pytest.mark.parametrize("exp_eye,ind_dim,arr", [(True, 4, dict(forward_dtype="f16", backward_dtype="f16")), (False, 0, dict(forward_dtype="f16", backward_dtype="f16")),
                                                 (True, 4, dict(record_dtype="f16")), (True, 4, dict(forward_dtype="f16"))])
def test_fused_weight_gradients_in_the_backward_kernel_equal_the_two_pass_arrangement(params, golden, M, exp_eye, ind_dim, arr):
    """fuse_dw (the default of the all-f16 arrangement): the weight gradients of the wide layers reduced inside the backward kernel
    (lz_triplane_head_backward_recorded_dw16: G / X tiles transposed through LDS, 95 accumulator tiles shared by the workgroup's waves)
    against backward + lz_triplane_head_grad_w_f16 over the records.  Same operand rounding (half), same f32 products, another summation
    order: outputs and the data-gradient side (tables) bit for bit, weight gradients to f32 reassociation.  Batch sizes: less than one
    slice, ragged last slice, a ragged last ROUND of a workgroup (8 slices per round), one round per workgroup, many rounds.
    Arrangements: the all-f16 step (two LDS buffers), and the two with the f32 data-gradient chain (f32 or f16 forward; one LDS buffer)."""
    from lzzx_nerf_amd.head_train import FusedTriplaneTrainHead
    rng = np.random.default_rng(41)
    p = dict(params)
    p["sigma_net.net.0.weight"] = np.ascontiguousarray(params["sigma_net.net.0.weight"][:, :68 + int(exp_eye)])
    p["color_net.net.0.weight"] = np.ascontiguousarray(params["color_net.net.0.weight"][:, :80 + ind_dim])
    for n in ("xy", "yz", "xz"):
        p[f"encoder_{n}.embeddings"] = params[f"encoder_{n}.embeddings"] * np.float32(30.0)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    xyz = dev(rng.uniform(-1, 1, (M, 3)).astype(np.float32))
    d = torch.nn.functional.normalize(dev(rng.normal(size=(M, 3)).astype(np.float32)), dim=-1)
    gout = [dev(rng.normal(size=sh).astype(np.float32)) for sh in ((M,), (M, 3), (M, 1), (M, 1), (M, 1))]
    gout[0] *= 1e-2

    def run(fuse):
        net = FusedTriplaneTrainHead(p, bound=1.0, exp_eye=exp_eye, ind_dim=ind_dim, fuse_dw=fuse, **arr).cuda()
        assert net.fuse_dw == fuse
        enc_a = dev(golden["net_enc_a"]).requires_grad_(True)
        ind = dev(golden["net_ind"]).requires_grad_(True) if ind_dim else None
        outs = net(xyz, d, enc_a, ind, dev(golden["net_eye"]) if exp_eye else None)
        live = [k for k in range(5) if outs[k].requires_grad]
        torch.autograd.backward([outs[k] for k in live], [gout[k] for k in live])
        g = {k: v.grad for k, v in net.named_parameters()}
        g["enc_a"] = enc_a.grad
        if ind is not None:
            g["ind"] = ind.grad
        return [o.detach() for o in outs], g

    o2, g2 = run(False)
    o1, g1 = run(True)
    for a, b in zip(o1, o2):
        assert torch.equal(a, b)
    for k in g2:
        if g2[k] is None:
            assert g1[k] is None, k
            continue
        assert torch.isfinite(g1[k]).all(), k
        if "embeddings" in k:                       # the chain is the same instruction sequence: d enc_x, hence the table scatter inputs, equal
            assert float((g1[k] - g2[k]).abs().max()) <= 2e-4 * float(g2[k].abs().max()) + 1e-30, k      # scatter-add order only
            continue
        scale = float(g2[k].abs().max()) + 1e-30
        # color_net.1: the two-pass arrangement sums f32 dY x half input per lane, the fused one rounds dY to half like every other
        # weight-gradient operand (autocast's dW GEMM has half operands): half rounding of one factor
        tol = 2e-3 if k == "color_net.net.1.weight" else 2e-5
        assert float((g1[k] - g2[k]).abs().max()) / scale < tol, (k, float((g1[k] - g2[k]).abs().max()) / scale)
        assert exp_eye is False and k.startswith("eye_att_net") or float(g1[k].abs().max()) > 0, k


@pytest.mark.parametrize("M,k_sig0", [(1, 69), (3, 68), (15, 69), (16, 69), (1000, 68), (70001, 69)])
def test_head_grad_w_f16_products_match_float64(M, k_sig0):
    """lz_triplane_head_grad_w_f16 on random half records built here from the documented layout (LZ_R16_*: 16-column tiles interleaved in
    pairs, a few natural-layout inputs regrouped; buffers blocked by 16-sample slice): the five products against float64 matmuls of the
    logical matrices.  Padding tiles / columns and the rows past M hold NaN: none of it may reach a written output."""
    from lzzx_nerf_amd import _lib
    from lzzx_nerf_amd._util import call, ptr, stream
    g = torch.Generator(device="cuda").manual_seed(100 + M)
    h = lambda *sh: torch.randn(*sh, device="cuda", generator=g).half()
    enc_x, enc_w, eye, a1, s1, s2, sh, ind = h(M, 36), h(M, 32), h(M), h(M, 64), h(M, 64), h(M, 64), h(M, 16), h(M, 4)
    g_x, g_att, g_s1, g_s2, g_c1, dh0 = h(M, 112), h(M, 32), h(M, 64), h(M, 64), h(M, 64), h(M)
    T = torch.full((M, 44, 16), float("nan"), device="cuda", dtype=torch.float16)   # logical tiles of 16 columns
    put = lambda t0, mat: T[:, t0:t0 + mat.shape[1] // 16].copy_(mat.reshape(M, -1, 16))
    put(0, a1)                                               # X_A1
    j = torch.arange(16, device="cuda")
    for p in (0, 1):                                         # X_SIG0 tiles 0, 1: enc_x feature 8 (j % 4) + 4 p + j / 4 at column j
        T[:, 4 + p] = enc_x[:, 8 * (j % 4) + 4 * p + j // 4]
    T[:, 6] = 0
    T[:, 6, 0::4] = enc_x[:, 32:36]                          # tile 2: feature 32 + q at column 4 q, the eye term at column 1
    T[:, 6, 1] = eye
    put(7, enc_w)                                            # tiles 3, 4: enc_a * att
    put(10, s1)                                              # X_S1
    put(14, s2)                                              # X_S2C: s2 | SH component 4 (j % 4) + j / 4 at column j | ind q at column 4 q
    T[:, 18] = sh[:, 4 * (j % 4) + j // 4]
    T[:, 19] = 0
    T[:, 19, 0::4] = ind
    put(20, g_x)                                             # G_X 7 tiles (+ 1 padding)
    put(28, g_att)
    put(30, g_s1)
    put(34, g_s2)
    put(38, g_c1)                                            # G_C1H: colour.0 gradient | d h0 at column 0 of the fifth tile
    T[:, 42, 0] = dh0
    Mb = (M + 15) // 16 * 16
    pairs = torch.full((Mb, 22, 16, 2), float("nan"), device="cuda", dtype=torch.float16)
    pairs[:M] = T.reshape(M, 22, 2, 16).permute(0, 1, 3, 2)  # dword j of pair g = {tile 2 g column j, tile 2 g + 1 column j}
    rec = pairs.reshape(Mb // 16, 16, 22, 32).permute(0, 2, 1, 3).contiguous()   # [slice][pair][sample][16 dwords]
    shapes = dict(x3=(112, 36), aud1=(32, 64), sig0=(64, k_sig0), sig1=(64, 64), c1h=(65, 84))
    out = {n: torch.full(shp, 7.0, device="cuda") for n, shp in shapes.items()}
    ws = torch.empty(_lib.load().lz_triplane_head_grad_w_workspace() // 4, device="cuda")
    call("lz_triplane_head_grad_w_f16", ptr(rec), M, k_sig0, *[ptr(out[n]) for n in ("x3", "aud1", "sig0", "sig1", "c1h")], ptr(ws), stream())
    d = lambda t: t.double()
    x_sig0 = torch.cat([d(enc_x), d(enc_w)] + ([d(eye)[:, None]] if k_sig0 == 69 else []), 1)
    want = dict(x3=d(g_x).T @ d(enc_x), aud1=d(g_att).T @ d(a1), sig0=d(g_s1).T @ x_sig0, sig1=d(g_s2).T @ d(s1),
                c1h=torch.cat([d(g_c1), d(dh0)[:, None]], 1).T @ torch.cat([d(s2), d(sh), d(ind)], 1))
    for n in shapes:
        got = out[n].double()
        assert torch.isfinite(got).all(), n
        assert float((got - want[n]).abs().max()) <= 2e-5 * float(want[n].abs().max()) + 1e-6, n


@pytest.mark.parametrize("arr", [dict(), dict(record=False), dict(record_dtype="f16"), dict(forward_dtype="f16", backward_dtype="f16"),
                                 dict(forward_dtype="f16")])
def test_fused_train_head_camera_gradients(params, golden, arr):
    """opt.train_camera (renderer.py:129-132, 225-230): rays carry gradients, march_rays_train hands them to xyzs / dirs, and the reference
    reaches them through the encoders' dy_dx (grid.py:44-84, gridencoder.cu:179-222, 316-342; sphere_harmonics.py:27-58).  The fused
    training head returns both input gradients in every arrangement (with fuse_dw the call falls back to the two-pass arrangement, whose
    record keeps color_net.0's output gradient): against the float64 model of the whole step, differentiated with respect to the sample
    positions (bilinear weights) and, through the checker's SH Jacobian, the directions -- and on to rays_o / rays_d through the
    march_rays_train backward (raymarching.cu:535-583)."""
    from lzzx_nerf_amd import raymarching as R
    from lzzx_nerf_amd.head_train import FusedTriplaneTrainHead
    H = W = 24
    pose, intr = synthetic_camera(H, W)
    ro, rd = get_rays(pose, intr, H, W)
    bits = ellipsoid_bitfield()[0]
    spec = TriplaneSpec(1.0)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    enc_a, eye, ind = golden["net_enc_a"], golden["net_eye"], golden["net_ind"]
    net = FusedTriplaneTrainHead({k: v for k, v in params.items()}, bound=1.0, **arr).cuda()
    half = "forward_dtype" in arr or "record_dtype" in arr
    aabb = dev(np.array([-1, -0.5, -1, 1, 0.5, 1], np.float32))
    ro_t, rd_t = dev(ro).requires_grad_(True), dev(rd).requires_grad_(True)
    nears, fars = R.near_far_from_aabb(ro_t.detach(), rd_t.detach(), aabb, 0.05)
    ctr = torch.zeros(2, dtype=torch.int32, device="cuda")
    xyzs, dirs, deltas, rays = R.march_rays_train(ro_t, rd_t, 1.0, dev(bits), 1, 128, nears, fars, ctr, -1, False, 128, True, 1 / 256, 32)
    assert xyzs.requires_grad and dirs.requires_grad
    xyzs.retain_grad()
    dirs.retain_grad()
    scale = 1024.0 if half else 1.0          # the half arrangements expect a GradScaler in front (bench.py does the same)
    sigma, rgb, aa, ae, unc = net(xyzs, dirs, dev(enc_a), dev(ind), dev(eye))
    ws, a0s, a1s, us, dep, img = R.composite_rays_train_triplane(sigma, rgb, aa[:, 0], ae[:, 0], unc[:, 0], deltas, rays)
    target = torch.linspace(0, 1, H * W * 3, device="cuda").reshape(-1, 3)
    loss = ((img - target) ** 2).mean() + 0.1 * ws.mean() + 1e-3 * a0s.mean() + 1e-3 * a1s.mean() + 1e-2 * us.mean()
    (loss * scale).backward()
    gx, gd = xyzs.grad / scale, dirs.grad / scale
    # ---------------- float64 model (as in test_fused_train_head_gradients), inputs as leaves ----------------
    dd = lambda a: torch.from_numpy(np.ascontiguousarray(a)).double()
    E = [dd(params[f"encoder_{n}.embeddings"]) for n in ("xy", "yz", "xz")]
    Wc = {k: dd(v) for k, v in params.items() if k.endswith(".weight")}
    sc, rs = O.grid_level_params(12, np.float32(np.log2(spec.per_level_scale)), 64)
    xc = dd(xyzs.detach().cpu().numpy()).requires_grad_(True)
    x01 = (xc + 1) / 2

    def mlpc(h, name, n):
        for i in range(n):
            h = h @ Wc[f"{name}.net.{i}.weight"].T
            if i < n - 1:
                h = torch.relu(h)
        return h

    enc_xc = torch.cat([_grid64(x01[:, [0, 1]], E[0], spec.offsets, sc, rs), _grid64(x01[:, [1, 2]], E[1], spec.offsets, sc, rs),
                        _grid64(x01[:, [0, 2]], E[2], spec.offsets, sc, rs)], -1)
    attc = mlpc(enc_xc, "aud_ch_att_net", 2)
    eyec = torch.sigmoid(mlpc(enc_xc, "eye_att_net", 2))
    hc = mlpc(torch.cat([enc_xc, dd(enc_a) * attc, dd(eye) * eyec], -1), "sigma_net", 3)
    sigc = torch.exp(hc[:, 0])
    sh_np, jac_np = O.sh_encode_forward(dirs.detach().cpu().numpy(), 4, True)
    shc = dd(sh_np).requires_grad_(True)
    rgbc = torch.sigmoid(mlpc(torch.cat([shc, hc[:, 1:], dd(ind).repeat(xc.shape[0], 1)], -1), "color_net", 2)) * 1.002 - 0.001
    uncc = torch.log(1 + torch.exp(mlpc(enc_xc.detach(), "unc_net", 2)))[:, 0]
    dl = dd(deltas.detach().cpu().numpy())
    rays_np = rays.cpu().numpy()
    N = rays_np.shape[0]
    imgs, wss, a0c, a1c, usc = [None] * N, [None] * N, [None] * N, [None] * N, [None] * N
    zero = torch.zeros((), dtype=torch.float64)
    for n in range(N):
        i, o, c = [int(v) for v in rays_np[n]]
        T, r, w_, a0_, a1_, u_ = 1.0, torch.zeros(3, dtype=torch.float64), zero, zero, zero, zero
        for s in range(o, o + c):
            alpha = 1 - torch.exp(-sigc[s] * dl[s, 0])
            wgt = alpha * T
            r = r + wgt * rgbc[s]
            w_ = w_ + wgt
            a0_ = a0_ + attc[s].norm()
            a1_ = a1_ + eyec[s].abs().sum()
            u_ = u_ + wgt * uncc[s]
            T = T * (1 - alpha)
            if float(T.detach()) < 1e-4:
                break
        imgs[i], wss[i], a0c[i], a1c[i], usc[i] = r, w_, a0_, a1_, u_
    lossc = ((torch.stack(imgs) - target.cpu().double()) ** 2).mean() + 0.1 * torch.stack(wss).mean() + 1e-3 * torch.stack(a0c).mean() + \
        1e-3 * torch.stack(a1c).mean() + 1e-2 * torch.stack(usc).mean()
    lossc.backward()
    want_x = xc.grad.numpy()
    want_d = np.einsum("bk,bdk->bd", shc.grad.numpy(), jac_np.astype(np.float64).reshape(-1, 3, 16))
    assert np.abs(want_x).max() > 0 and np.abs(want_d).max() > 0

    f16_forward = "forward_dtype" in arr

    def close(got, want, name, tol):
        a = got.detach().cpu().double().numpy()
        err, l2 = np.max(np.abs(a - want)) / np.abs(want).max(), np.linalg.norm(a - want) / np.linalg.norm(want)
        p95 = np.percentile(np.abs(a - want), 95) / np.abs(want).max()
        # a half forward flips the ReLU mask of a unit whose pre-activation is within half rounding of zero: one sample's gradient then
        # differs by that unit's whole contribution (sums over samples -- the weight gradients -- average it out, a per-sample gradient
        # does not; ~200 flips among 3 200 x 64 colour units give the measured l2 of 0.03), so those arrangements are held in the l2
        # norm and on 95 % of the entries
        if f16_forward:
            assert l2 < 6e-2 and p95 < 1e-2, (name, err, l2, p95)
        else:
            assert err < tol, (name, err, l2)

    # positions: the finest level turns a table difference into a slope of ~511 per unit, and f32 rounding of pos = x * scale + 0.5 moves
    # the corner weights of the gradient's other factor by ~3e-5 of a cell
    close(gx, want_x, "xyzs", 3e-2 if half else 2e-3)
    close(gd, want_d, "dirs", 3e-2 if half else 2e-3)
    # and on through the march: d rays_o = sum over the ray's samples of d xyz, d rays_d = sum of d xyz * deltas[:, 1] + d dirs -- the
    # reference multiplies by the stored step difference, not by t (raymarching.cu:570-572); mirrored
    assert ro_t.grad is not None and rd_t.grad is not None and float(ro_t.grad.abs().sum()) > 0 and float(rd_t.grad.abs().sum()) > 0
    go = np.zeros((N, 3)), np.zeros((N, 3))
    dl_np = dl.numpy()
    for n in range(N):
        i, o, c = [int(v) for v in rays_np[n]]
        for s in range(o, o + c):
            go[0][i] += want_x[s]
            go[1][i] += dl_np[s, 1] * want_x[s] + want_d[s]
    close(ro_t.grad / scale, go[0], "rays_o", 3e-2 if half else 2e-3)
    close(rd_t.grad / scale, go[1], "rays_d", 3e-2 if half else 2e-3)


@pytest.mark.parametrize("exp_eye,ind_dim", [(True, 4), (False, 4), (True, 0)])
def test_recomputing_f16_step_equals_the_recorded_one(params, golden, exp_eye, ind_dim):
    """recompute_mlp (round 5, the default of the all-f16 arrangement): the forward keeps only the enc_x halves (80 B per sample), the backward
    kernel runs the MLP again from them with the forward's own code (csrc/lz_head_fwd16_chain.h) and a sink that keeps in registers what the
    recording forward stored.  Same arithmetic in the same order, so the five outputs and EVERY gradient (11 weight matrices, 3 tables,
    enc_a, ind_code) equal the recorded pair's bit for bit -- ragged last slice, a workgroup's last round with idle waves included."""
    from lzzx_nerf_amd.head_train import FusedTriplaneTrainHead
    rng = np.random.default_rng(77)
    p = dict(params)
    p["sigma_net.net.0.weight"] = np.ascontiguousarray(params["sigma_net.net.0.weight"][:, :68 + int(exp_eye)])
    p["color_net.net.0.weight"] = np.ascontiguousarray(params["color_net.net.0.weight"][:, :80 + ind_dim])
    for n in ("xy", "yz", "xz"):
        p[f"encoder_{n}.embeddings"] = params[f"encoder_{n}.embeddings"] * np.float32(30.0)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    for M in (16 * 4321 + 5, 37):
        xyz = torch.from_numpy(rng.uniform(-1, 1, (M, 3)).astype(np.float32)).cuda()
        d = torch.nn.functional.normalize(torch.from_numpy(rng.normal(size=(M, 3)).astype(np.float32)), dim=-1).cuda()
        gout = [torch.from_numpy(rng.normal(size=sh).astype(np.float32)).cuda() for sh in ((M,), (M, 3), (M, 1), (M, 1), (M, 1))]
        gout[0] *= 1e-2
        res = []
        for rc in (False, True):
            net = FusedTriplaneTrainHead(p, bound=1.0, exp_eye=exp_eye, ind_dim=ind_dim, forward_dtype="f16", backward_dtype="f16", recompute_mlp=rc).cuda()
            assert net.recompute_mlp is rc
            enc_a = dev(golden["net_enc_a"]).requires_grad_(True)
            ind = dev(golden["net_ind"]).requires_grad_(True) if ind_dim else None
            eye = dev(golden["net_eye"]) if exp_eye else None
            outs = net(xyz, d, enc_a, ind, eye)
            live = [k for k in range(5) if outs[k].requires_grad]
            torch.autograd.backward([outs[k] for k in live], [gout[k] for k in live])
            g = {n: t.grad.clone() for n, t in net.named_parameters()}
            g["enc_a"] = enc_a.grad.clone()
            if ind is not None:
                g["ind"] = ind.grad.clone()
            res.append(([o.detach().clone() for o in outs], g))
        (o0, g0), (o1, g1) = res
        for a, b, nm in zip(o0, o1, ("sigma", "rgb", "amb_aud", "amb_eye", "unc")):
            assert torch.equal(a, b), (M, nm)
        assert set(g0) == set(g1)
        for n in g0:
            assert bool(torch.isfinite(g1[n]).all()) and float(g1[n].abs().max()) > 0 or n.startswith("eye_att") and not exp_eye, (M, n)
            # float atomics in a free order: the table scatter's flush, and the per-workgroup sums of the skinny layers / enc_a / ind_code
            if "embeddings" in n or n in ("enc_a", "ind") or n.endswith(("eye_att_net.net.1.weight", "unc_net.net.1.weight", "color_net.net.1.weight")):
                assert float((g0[n] - g1[n]).abs().max()) <= 1e-5 * float(g0[n].abs().max()), (M, n)
            else:
                assert torch.equal(g0[n], g1[n]), (M, n, float((g0[n] - g1[n]).abs().max()))
    # the default of the all-f16 arrangement, and what it refuses
    assert FusedTriplaneTrainHead(p, exp_eye=exp_eye, ind_dim=ind_dim, forward_dtype="f16", backward_dtype="f16").recompute_mlp is True
    assert FusedTriplaneTrainHead(p, exp_eye=exp_eye, ind_dim=ind_dim, forward_dtype="f16").recompute_mlp is False
    with pytest.raises(ValueError, match="recompute_mlp"):
        FusedTriplaneTrainHead(p, exp_eye=exp_eye, ind_dim=ind_dim, recompute_mlp=True)
