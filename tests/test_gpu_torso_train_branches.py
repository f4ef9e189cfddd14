"""The branches of the fused torso backward (lzzx_nerf_amd.torso_train.FusedTorsoTrainNet, csrc/lz_torso_train.hip) against the float64
model of tests/torso_train_cases.py: the clamp gate, the mask (float and device threshold), the background mix (c - bg on alpha, the
colour path scaled by alpha, scalar and per-pixel background), tail slices, the C entry point's null upstream pointers, and the anchor
backward on general poses.  The inputs, their two regimes (F: scaled table, nothing clamped; C: coarse table, clamp active, zero upstream
deform gradient) and the bounds are the cases module's; tests/test_torso_train_cases_host.py shows on the CPU that a model with any one
of these branches wrong misses the bounds by a factor of ten or more.

Bounds, max-norm per tensor relative to the tensor's largest reference magnitude: regime F 1e-4 for the MLP weights and 2e-3 for the
table, anchor points and individual code; regime C 2e-4 throughout.  Worst error / bound, the fused kernels on the MI355X next to the
CPU's float32 restatement of the model:

  error / bound: kernel (f32 restatement)    deform net     torso net      table          anchors        ind code     
  F run_torso, 12 cases, N = 1000            0.029 (0.018)  0.029 (0.025)  0.058 (0.058)  0.000 (0.000)  0.000 (0.000)
  F colour only (table zero from level 9)    0.113 (0.092)  0.014 (0.013)  0.038 (0.029)  0.000 (0.000)  0.000 (0.000)
  C clamp, 4 cases, N = 3000                 0.059 (0.038)  0.030 (0.031)  0.216 (0.215)  0.028 (0.029)  0.036 (0.019)
  C sizes 1-257 and tails                    0.068 (0.064)  0.042 (0.033)  0.663 (0.663)  0.018 (0.015)  0.012 (0.010)
  C size 4099                                0.055 (0.058)  0.044 (0.016)  0.177 (0.177)  0.010 (0.007)  0.024 (0.011)

(0.000: under 5e-4 of the bound.)  The table's 0.66 at 15-17 pixels is no kernel error: a single pixel's table gradient at level 15 is its
corner weight times a number of the tensor's own maximum, and the weight carries the rounding of pos = fma(u, 2047, 0.5) to f32, up to
6e-5 of a cell; kernel and restatement round alike.  From N = 3000 up the coarse levels' sums set the maximum (0.15-0.22).
Each branch also has a mutant of the kernel that only the tests named for it (and the size cases) reject: clamp gate dropped or read
from the other coordinate -> c; - bg or the alpha scaling of the colour path dropped -> a, b; `live` without `valid` -> d; device
threshold ignored -> a[tensor].
"""
import ctypes as C
import functools

import pytest
import torch

import torso_train_cases as T

pytestmark = pytest.mark.gpu


def _dev(t):
    return t.cuda() if torch.is_tensor(t) else t


@functools.lru_cache(maxsize=None)
def _ref(key):
    """the float64 model of a case, once; key = (builder name, args...)"""
    return T.run_model(_case(key))


def _case(key):
    return getattr(T, key[0])(*key[1:])


def _net(c, cls_name="FusedTorsoTrainNet"):
    from lzzx_nerf_amd import torso_train
    net = getattr(torso_train, cls_name)(ind_dim_torso=c.ind_dim, torso_shrink=c.shrink).cuda()
    net.load_state_dict(c.sd)
    return net


def _forward(net, c, thresh="float"):
    """the case through the fused net: forward() without a background, run_torso with one -> alpha, colour, deform, the code leaf"""
    cc = c.ind.cuda().requires_grad_(True) if c.ind is not None else None
    xy, pose = c.xy.cuda(), c.pose.cuda()
    if c.bg is None:
        a, col, d = net(xy, pose, cc)
        return a, col, d, cc
    th = None if c.grid is None else T.GRID_THRESH if thresh == "float" else torch.tensor([T.GRID_THRESH], device="cuda")
    out = net.run_torso(xy, pose, cc, bg_color=_dev(c.bg), density_grid=_dev(c.grid), density_thresh=th)
    return out["torso_alpha"], out["torso_color"], out["deform"], cc


def _forward_ops(net, c):
    """TorsoTrainNet (the f32 operator graph) with torch's mask and mix around it, as test_fifty_steps_follow_the_operator_path"""
    cc = c.ind.cuda().requires_grad_(True) if c.ind is not None else None
    xy, pose = c.xy.cuda(), c.pose.cuda()
    if c.mask is None:
        a, col, d = net(xy, pose, cc)
    else:
        m = c.mask.cuda()
        a, col, d = torch.zeros(c.N, 1, device="cuda"), torch.zeros(c.N, 3, device="cuda"), torch.zeros(c.N, 2, device="cuda")
        a_m, c_m, d_m = net(xy[m], pose, cc)
        a[m], col[m], d[m] = a_m, c_m, d_m
    if c.bg is not None:
        col = col * a + _dev(c.bg) * (1 - a)
    return a, col, d, cc


def _backward(net, c, outs):
    a, col, d, cc = outs
    net.zero_grad(set_to_none=True)
    ((a * c.ga.cuda()).sum() + (col * c.gc.cuda()).sum() + (d * c.gd.cuda()).sum()).backward()
    g = {k: p.grad.detach().double().cpu() for k, p in net.named_parameters()}
    if cc is not None:
        g["ind_code"] = cc.grad.detach().double().cpu()
    return g


def _check(name, c, ref, got):
    """every gradient within its bound; if one is not, the operator path on the same inputs goes into the message (a bound that
    TorsoTrainNet meets and the fused kernel misses is a finding in the kernel, one that both miss a defect of the inputs)"""
    r = T.ratios(got, ref, c)
    print("RATIO %-28s %s" % (name, " ".join("%s=%.3f" % (k, v) for k, v in r.items())))
    for k in c.keys:
        assert float(ref[k].abs().max()) > 0, (name, k)
    if max(r.values()) > 1:
        ops = _net(c, "TorsoTrainNet")
        r_ops = T.ratios(_backward(ops, c, _forward_ops(ops, c)), ref, c)
        assert max(r.values()) <= 1, (name, {k: (round(r[k], 3), round(r_ops[k], 3)) for k in c.keys if r[k] > 1}, "(fused, TorsoTrainNet) error / bound")


# ---- a. run_torso against the float64 model ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask", ["nogrid", "float", "tensor"])
@pytest.mark.parametrize("bg_kind", ["scalar", "tensor"])
@pytest.mark.parametrize("ind_dim", [0, 8])
def test_run_torso_gradients_match_the_float64_model(ind_dim, bg_kind, mask):
    key = ("case_f", ind_dim, bg_kind, mask != "nogrid")
    c, (ref, diag) = _case(key), _ref(key)
    net = _net(c)
    outs = _forward(net, c, mask)
    a, col = outs[0].detach(), outs[1].detach()
    if c.mask is not None:   # the kernel's mask is the model's: exact zeros and the background's bits outside, a live alpha inside
        off = ~c.mask.cuda()
        bg = _dev(c.bg) if torch.is_tensor(c.bg) else torch.full((c.N, 3), c.bg, device="cuda")
        assert bool((a[off] == 0).all()) and torch.equal(col[off], bg[off]) and bool((outs[2].detach()[off] == 0).all())
        assert bool((a[~off] != 0).all())
    assert float((a.double().cpu() - diag["alpha"]).abs().max()) < 2e-5 and float((col.double().cpu() - diag["color"]).abs().max()) < 2e-5
    _check("F ind%d bg=%s mask=%s" % (ind_dim, bg_kind, mask), c, ref, _backward(net, c, outs))


# ---- b. only the colour is used (TorsoObjective) -------------------------------------------------------------------------------------
@pytest.mark.parametrize("ind_dim", [0, 8])
def test_colour_only_loss_matches_the_float64_model(ind_dim):
    """The deform net's gradients then come through the grid's dy/dx alone.  On the full table that path carries the rounding of the
    f32 sample positions at the fine levels (half an ulp at 2^11 is 6e-5 of a cell): the CPU's f32 restatement misses the MLP bound of
    1e-4 by up to 1.9 x.  So this case zeroes the table from level 9 on, as regime C does (restatement: 0.09 x the bound)."""
    key = ("case_f", ind_dim, "tensor", True, True)
    c, (ref, _) = _case(key), _ref(key)
    assert not bool(c.ga.any()) and not bool(c.gd.any())
    net = _net(c)
    _check("F colour only ind%d" % ind_dim, c, ref, _backward(net, c, _forward(net, c)))


# ---- c. the clamp -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mix", [False, True])
@pytest.mark.parametrize("ind_dim", [0, 8])
def test_clamp_gate_against_the_float64_model(ind_dim, mix):
    key = ("case_c", ind_dim, mix)
    c, (ref, diag) = _case(key), _ref(key)
    net = _net(c)
    outs = _forward(net, c)
    # forward: deform is the unclamped dx (a clamped one would differ by |v| - 1 >= 1e-4 on every clamped pixel); the rest is FusedTorso
    d = outs[2].detach()
    assert float((d.double().cpu() - diag["deform"]).abs().max()) < 1e-5
    clamped = (diag["v"].abs() > 1)
    assert bool(((c.xy.double() + d.double().cpu()).abs() > 1)[clamped].all()) and int(clamped.sum()) > 100
    from lzzx_nerf_amd.torso import FusedTorso
    a_i, c_i, d_i = FusedTorso(c.sd, torso_shrink=1.0)(c.xy.cuda(), c.pose.cuda(), _dev(c.ind))
    if mix:
        c_i = FusedTorso.mix_background(a_i, c_i, c.bg.cuda())
    assert torch.equal(outs[0].detach(), a_i) and torch.equal(outs[1].detach(), c_i) and torch.equal(d, d_i)
    _check("C ind%d %s" % (ind_dim, "mix" if mix else "nomix"), c, ref, _backward(net, c, outs))


@pytest.mark.parametrize("mix", [False, True])
@pytest.mark.parametrize("ind_dim", [0, 8])
@pytest.mark.parametrize("only", ["both", "only0", "only1"])
def test_clamped_pixels_send_exactly_nothing_to_the_deform_net(only, ind_dim, mix):
    """upstream gradients on the pixels clamped in both coordinates alone (deform gradient zero): the deform net's weight gradients
    are zeros, not small numbers; on the pixels clamped in coordinate d alone: row d of the last deform layer"""
    c = T.case_c(ind_dim, mix, only=only)
    assert int((c.ga[:, 0] != 0).sum()) >= 16
    net = _net(c)
    g = _backward(net, c, _forward(net, c))
    assert all(bool(g[k].any()) for k in T.MLP_KEYS[3:])
    if only == "both":
        for k in T.DEFORM_KEYS:
            assert bool((g[k] == 0).all()), k
    else:
        d = 0 if only == "only0" else 1
        w2 = g["torso_deform_net.net.2.weight"]
        assert bool((w2[d] == 0).all()) and bool(w2[1 - d].any())


# ---- d. sizes -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", T.SIZES)
def test_gradients_at_sizes_around_the_slice(N):
    key = ("case_size", N)
    c, (ref, _) = _case(key), _ref(key)
    net = _net(c)
    _check("C size %d" % N, c, ref, _backward(net, c, _forward(net, c)))


@pytest.mark.parametrize("N", [1, 17])
def test_tail_lanes_do_not_count_the_last_pixel_twice(N):
    """a tail slice's invalid lanes read pixel N - 1; with all the upstream gradient on that pixel a lane that leaked would double it"""
    key = ("case_size", N, True)
    c, (ref, _) = _case(key), _ref(key)
    assert bool(c.ga[-1].any()) and not bool(c.ga[:-1].any()) and not bool(c.gc[:-1].any())
    net = _net(c)
    _check("C tail %d" % N, c, ref, _backward(net, c, _forward(net, c)))


# ---- e. null upstream pointers of the C entry point ---------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["g_alpha", "g_color", "g_deform"])
def test_null_upstream_pointer_is_a_zero_tensor(which):
    from lzzx_nerf_amd import _lib, torso_train
    from lzzx_nerf_amd._util import call, ptr, stream
    from lzzx_nerf_amd.torso import FusedTorso
    c = T.case_f(8, "tensor", True)
    net = _net(c)
    xy, ind, bg, grid = c.xy.cuda(), c.ind.cuda().reshape(-1).contiguous(), c.bg.cuda().contiguous(), c.grid.cuda()
    enc_anchor = FusedTorso(c.sd).encode_anchor(c.pose.cuda()).reshape(-1).contiguous()
    meta = dict(net=net, offsets=net.torso_encoder.offsets.to("cuda", torch.int32).contiguous(), density_grid=grid, G=T.GRID_G,
                thresh_f=T.GRID_THRESH, thresh_t=None, bg=bg, bg_scalar=0.0, mix=True)
    dw = [net.torso_deform_net.net[i].weight for i in range(3)]
    tw = [net.torso_net.net[i].weight for i in range(3)]
    emb = net.torso_encoder.embeddings
    p = net._params(meta, xy, enc_anchor, ind, dw, tw, emb)
    up = dict(g_alpha=c.ga.cuda().contiguous(), g_color=c.gc.cuda().contiguous(), g_deform=c.gd.cuda().contiguous())

    def run(**replace):
        u = dict(up, **replace)
        ws = [torch.empty_like(w) for w in dw + tw]
        g_emb, g_enc, g_ind = torch.zeros_like(emb), torch.empty_like(enc_anchor), torch.empty_like(ind)
        g = _lib.TorsoGrads()
        g.g_deform_w0, g.g_deform_w1, g.g_deform_w2, g.g_torso_w0, g.g_torso_w1, g.g_torso_w2 = [w.data_ptr() for w in ws]
        g.g_emb, g.g_enc_anchor, g.g_ind_code = g_emb.data_ptr(), g_enc.data_ptr(), g_ind.data_ptr()
        call("lz_torso_train_backward", C.byref(p), ptr(xy), c.N, ptr(u["g_alpha"]), ptr(u["g_color"]), ptr(u["g_deform"]), C.byref(g),
             ptr(torso_train._workspace(xy.device)), stream())
        torch.cuda.synchronize()
        return ws + [g_enc, g_ind], g_emb

    fixed_n, emb_n = run(**{which: None})
    fixed_z, emb_z = run(**{which: torch.zeros_like(up[which])})
    fixed_f, _ = run()
    for a, b in zip(fixed_n, fixed_z):
        assert torch.equal(a, b) and bool(a.any())
    assert any(not torch.equal(a, f) for a, f in zip(fixed_n, fixed_f))   # the pointer that was dropped did carry a gradient
    assert torch.allclose(emb_n, emb_z, rtol=1e-5, atol=1e-6 * float(emb_z.abs().max())) and bool(emb_n.any())


# ---- f. background shapes ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["float", "one", "three", "full"])
def test_background_shapes_give_mix_background_bits(kind):
    from lzzx_nerf_amd.torso import FusedTorso
    c = T.case_f(8, "tensor", True)
    net = _net(c)
    N = c.N
    rgb = torch.tensor([0.25, 0.5, 0.75], device="cuda")
    bg, full = {"float": (0.25, torch.full((N, 3), 0.25, device="cuda")), "one": (torch.tensor([0.25], device="cuda"), torch.full((N, 3), 0.25, device="cuda")),
                "three": (rgb, rgb.expand(N, 3).contiguous()), "full": (c.bg.cuda(), c.bg.cuda())}[kind]
    xy, pose, ind, grid = c.xy.cuda(), c.pose.cuda(), c.ind.cuda(), c.grid.cuda()
    with torch.no_grad():
        out = net.run_torso(xy, pose, ind, bg_color=bg, density_grid=grid, density_thresh=T.GRID_THRESH)
        a_i, c_i, d_i = FusedTorso(c.sd)(xy, pose, ind, density_grid=grid, density_thresh=T.GRID_THRESH)
    assert torch.equal(out["torso_alpha"], a_i) and torch.equal(out["deform"], d_i)
    assert torch.equal(out["torso_color"], FusedTorso.mix_background(a_i, c_i, full))
    assert torch.equal(a_i[:, 0] != 0, c.mask.cuda())


# ---- g. anchor backward on general poses ------------------------------------------------------------------------------------------
def _anchor_poses():
    p = T.pose3()[0]
    general = p.copy()
    general[3] = [0.01, -0.02, 0.03, 1.1]
    return {"three_axes": p, "rows_exchanged": p[[1, 0, 2, 3]].copy(), "general_bottom_row": general}


@pytest.mark.parametrize("which", ["three_axes", "rows_exchanged", "general_bottom_row"])
def test_anchor_backward_matches_float64_autograd(which):
    """lz_torso_anchor_encode_backward computes in double and rounds once: 1e-6 x max |reference| per element.  rows_exchanged is the
    pose of test_gpu_clip.py whose elimination exchanges rows (determinant -1); general_bottom_row has a bottom row other than
    (0, 0, 0, 1), which the cofactor inverse must handle as torch.inverse does."""
    from lzzx_nerf_amd._util import call, ptr, stream
    pose = torch.from_numpy(_anchor_poses()[which])
    assert int((pose[:3, :3] != 0).sum()) == 9
    anchors = torch.from_numpy(T.torso_state(8, seed=3)["anchor_points"])
    g_enc = torch.randn(42, generator=torch.Generator().manual_seed(31))
    a64 = anchors.double().requires_grad_(True)
    w = a64[None] @ pose.double()[None].permute(0, 2, 1).inverse()
    w = (w[:, :, :2] / w[:, :, 3, None] / w[:, :, 2, None]).view(1, -1)
    (T._freq(w, 3).view(-1) * g_enc.double()).sum().backward()
    ref = a64.grad
    pose_d, anchors_d, g_d = pose.cuda().contiguous(), anchors.cuda().contiguous(), g_enc.cuda().contiguous()
    got = torch.empty_like(anchors_d)
    call("lz_torso_anchor_encode_backward", ptr(pose_d), ptr(anchors_d), ptr(g_d), 3, ptr(got), stream())
    err = float((got.double().cpu() - ref).abs().max())
    print("RATIO anchor %s %.3f" % (which, err / (1e-6 * float(ref.abs().max()))))
    assert bool(ref.abs().min() > 0) and err <= 1e-6 * float(ref.abs().max()), (which, err, float(ref.abs().max()))
