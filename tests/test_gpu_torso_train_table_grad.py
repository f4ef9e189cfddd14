"""FusedTorsoTrainNet(table_grad="ordered" | "fixed") (lzzx_nerf_amd/torso_train.py, csrc/lz_torso_train.hip): the backward kernel writes
the gradient of the grid features (last_denc, level-major [16, N, 2]) and the coordinates it gathered at (last_u [N, 2]) instead of
scattering, and gridencoder.grid_backward_ordered / grid_backward_fixed sum them into the table.

Inputs: the seeded state dict of tests/torso_train_cases.py (regime F: table x 1e-3, torso_shrink 0.8), its head pose, upstream
gradients and occupancy blob.  Shapes: the first N of 4099 uniform pixels for N in 1, 15, 16, 17, 4099 (tail slices, more than one
workgroup's worth of slices), 3000 uniform pixels, and rows 290-353 x columns 418-481 of the 512 x 512 frame in row order (neighbours: at
level 0 the 4096 pixels fall into a few cells, so thousands of terms meet in one entry).  Each with ind_dim_torso 0 and 8, through
forward() and through run_torso() with the blob at threshold 0.4 (it passes about half: 0.47-0.53 of these sets; the one pixel of N = 1 is masked out, so that case is a skipped tail slice) and a per-pixel background.

A masked-out pixel's rows are zeros with u = (-1, -1): out of range, so the grid encoder's table-gradient kernels skip them.

What the checks rest on.  Bit equality throughout, except the float64 model: its bounds are those of
tests/test_gpu_torso_train_branches.py for the same cases (torso_train_cases.bound), and its references are that module's cache.
"Same terms" (d): with float atomics an entry that one term reaches holds fl(w g) added to zero; "ordered" adds the same f32 term to zero;
"fixed" quantises it with the level's scale 2^e, e = 51 - hb - ex (hb = 6 for 15 x 4 corners, max |g| < 2^ex), which is exact for every
term not below 2^-21 of the level's largest gradient -- so where no entry is reached twice the three must agree bit for bit."""
import functools
import types

import pytest
import torch

import torso_train_cases as T
from test_gpu_torso_train_branches import _backward as _model_backward, _case, _check, _forward as _model_forward, _ref

pytestmark = pytest.mark.gpu

THRESH = 0.4
SHAPES = ("n1", "n15", "n16", "n17", "n4099", "rand3000", "block64")
MODES = ("ordered", "fixed")
TABLE = "torso_encoder.embeddings"


# ---- inputs (CPU) -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _pixels(shape):
    if shape == "block64":
        lin = torch.linspace(-1, 1, 512)
        ys, xs = torch.meshgrid(lin[290:354], lin[418:482], indexing="ij")
        return torch.stack([xs.reshape(-1), ys.reshape(-1)], 1).contiguous()
    if shape == "rand3000":
        return torch.rand(3000, 2, generator=torch.Generator().manual_seed(41)) * 2 - 1
    return (torch.rand(4099, 2, generator=torch.Generator().manual_seed(42)) * 2 - 1)[:int(shape[1:])].contiguous()


@functools.lru_cache(maxsize=None)
def _inputs(shape, ind_dim, xy=None):
    xy = _pixels(shape) if xy is None else xy
    N = xy.shape[0]
    gen = torch.Generator().manual_seed(43)
    ind = torch.randn(1, ind_dim, generator=gen) * 0.1 if ind_dim else None
    ga, gc, gd = T._upstream(N, 44)
    return types.SimpleNamespace(N=N, ind_dim=ind_dim, xy=xy, ind=ind, ga=ga, gc=gc, gd=gd, bg=torch.rand(N, 3, generator=gen),
                                 grid=torch.from_numpy(T.blob()), pose=torch.from_numpy(T.pose3()))


def _permuted(c, perm):
    return types.SimpleNamespace(N=c.N, ind_dim=c.ind_dim, xy=c.xy[perm].contiguous(), ind=c.ind, ga=c.ga[perm], gc=c.gc[perm], gd=c.gd[perm],
                                 bg=c.bg[perm].contiguous(), grid=c.grid, pose=c.pose)


# ---- the net and one backward -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _net(ind_dim):
    from lzzx_nerf_amd.torso_train import FusedTorsoTrainNet
    net = FusedTorsoTrainNet(ind_dim_torso=ind_dim, torso_shrink=0.8).cuda()
    net.load_state_dict(T.state("F", ind_dim))
    return net


def _grads(c, path, mode, scale=1.0, net=None):
    """one forward + backward -> (gradients by state-dict key plus "ind_code", last_denc, last_u); table_grad is set on the shared net
    (a plain attribute, read by the backward)"""
    net = _net(c.ind_dim) if net is None else net
    net.table_grad, net.keep_denc, net.last_denc, net.last_u = mode, True, None, None
    cc = c.ind.cuda().requires_grad_(True) if c.ind is not None else None
    xy, pose = c.xy.cuda(), c.pose.cuda()
    if path == "forward":
        a, col, d = net(xy, pose, cc)
    else:
        out = net.run_torso(xy, pose, cc, bg_color=c.bg.cuda(), density_grid=c.grid.cuda(), density_thresh=THRESH)
        a, col, d = out["torso_alpha"], out["torso_color"], out["deform"]
    net.zero_grad(set_to_none=True)
    ((a * (c.ga.cuda() * scale)).sum() + (col * (c.gc.cuda() * scale)).sum() + (d * (c.gd.cuda() * scale)).sum()).backward()
    g = {k: p.grad.detach().clone() for k, p in net.named_parameters()}
    if cc is not None:
        g["ind_code"] = cc.grad.detach().clone()
    denc, u = net.last_denc, net.last_u
    net.table_grad, net.keep_denc, net.last_denc, net.last_u = "atomic", False, None, None
    return g, denc, u


def _standalone(mode, denc, u, net):
    """the table gradient of the grid encoder's own backward entry on the rows, into zeros"""
    from lzzx_nerf_amd import gridencoder
    emb = net.torso_encoder.embeddings.detach()
    g_emb = torch.zeros_like(emb)
    offsets = net.torso_encoder.offsets.to("cuda", torch.int32).contiguous()
    fn = gridencoder.grid_backward_ordered if mode == "ordered" else gridencoder.grid_backward_fixed
    fn(denc, u, emb, offsets, g_emb, u.shape[0], 2, 2, 16, net._S, net._H, None, None, 1, False, 0)
    return g_emb


ALL = pytest.mark.parametrize("shape,ind_dim,path", [(s, i, p) for s in SHAPES for i in (0, 8) for p in ("forward", "run_torso")])


def test_the_mask_passes_about_half():
    for shape in ("n4099", "rand3000", "block64"):
        frac = float((T.occupancy(T.blob(), T.GRID_G, _pixels(shape)) > THRESH).mean())
        assert 0.4 < frac < 0.65, (shape, frac)


# ---- a. repeat; c. plumbing; e. the other gradients ------------------------------------------------------------------------------------
@ALL
@pytest.mark.parametrize("mode", MODES)
def test_two_backwards_give_the_same_bits_and_the_standalone_table_gradient(mode, shape, ind_dim, path):
    c = _inputs(shape, ind_dim)
    g1, denc, u = _grads(c, path, mode)
    g2, denc2, u2 = _grads(c, path, mode)
    assert tuple(denc.shape) == (16, c.N, 2) and tuple(u.shape) == (c.N, 2)
    assert torch.equal(denc, denc2) and torch.equal(u, u2)
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k
    if path == "run_torso":   # a masked-out pixel's rows are written too (they were allocated with torch.empty): zeros, and u = -1
        occ = torch.from_numpy(T.occupancy(T.blob(), T.GRID_G, c.xy))   # float64; the kernel's f32 may differ within OCC_MARGIN of it
        off, on = (occ < THRESH - T.OCC_MARGIN).cuda(), (occ > THRESH + T.OCC_MARGIN).cuda()
        assert bool((denc[:, off] == 0).all()) and bool((u[off] == -1).all())   # out of range: the grid kernels skip the row
        assert bool(((u[on] >= 0) & (u[on] <= 1)).all())
    else:
        assert bool(((u >= 0) & (u <= 1)).all())
    assert bool(torch.isfinite(denc).all()) and bool((((u >= 0) & (u <= 1)) | (u == -1)).all())
    # the fused table gradient is the grid encoder's own backward on exactly these rows: layout, level and channel order, mask, tails
    assert torch.equal(g1[TABLE], _standalone(mode, denc, u, _net(ind_dim)))
    if path == "forward" or shape != "n1":
        assert bool(g1[TABLE].any())


@ALL
def test_every_other_gradient_has_the_atomic_bits(shape, ind_dim, path):
    c = _inputs(shape, ind_dim)
    ga, denc_a, _ = _grads(c, path, "atomic")
    assert denc_a is None   # the atomic call leaves no rows
    for mode in MODES:
        g, _, _ = _grads(c, path, mode)
        assert set(g) == set(ga)
        for k in g:
            if k != TABLE:
                assert torch.equal(g[k], ga[k]), (mode, k)


# ---- b. order-free --------------------------------------------------------------------------------------------------------------------
@ALL
def test_fixed_is_free_of_the_pixels_order(shape, ind_dim, path):
    c = _inputs(shape, ind_dim)
    perm = torch.randperm(c.N, generator=torch.Generator().manual_seed(45))
    g, denc, u = _grads(c, path, "fixed")
    gp, denc_p, u_p = _grads(_permuted(c, perm), path, "fixed")
    # a pixel's rows do not depend on its place in a slice
    assert torch.equal(denc_p, denc[:, perm.cuda()]) and torch.equal(u_p, u[perm.cuda()])
    assert torch.equal(gp[TABLE], g[TABLE])


# ---- d. the same terms as the atomic kernel --------------------------------------------------------------------------------------
def _fine_entries(u, net):
    """entries (level, index) that the live pixels' four corners reach at levels 14 and 15, per pixel: int64 [n_live, 2, 4]; the
    tiled grid's index (gridencoder.cu:54-72) from u in float32, as the kernels form it"""
    import numpy as np
    offs = net.torso_encoder.offsets.cpu().numpy().astype(np.int64)
    uu = u.cpu().numpy().astype(np.float32)
    out = []
    for l in (14, 15):
        sc = np.float32(np.exp2(np.float32(l) * np.float32(net._S)) * np.float32(16) - np.float32(1))
        res = int(np.ceil(sc)) + 1
        pos = (uu.astype(np.float64) * float(sc) + 0.5).astype(np.float32)   # the kernels' fma: one rounding
        g0 = np.floor(pos).astype(np.int64)
        hs = int(offs[l + 1] - offs[l])
        out.append(np.stack([((g0[:, 0] + cx) + (g0[:, 1] + cy) * (res + 1)) % hs for cy in (0, 1) for cx in (0, 1)], 1))
    return torch.from_numpy(np.stack(out, 1))


def _scattered(ind_dim, seed):
    xy = torch.rand(15, 2, generator=torch.Generator().manual_seed(seed)) * 2 - 1
    return _inputs("scattered%d" % seed, ind_dim, xy)


@pytest.mark.parametrize("path", ["forward", "run_torso"])
@pytest.mark.parametrize("ind_dim", [0, 8])
def test_single_terms_agree_bit_for_bit_across_the_three_modes(ind_dim, path):
    """15 scattered pixels; at the two finest levels (2^16 entries each, 60 corners) no entry may be reached by two pixels.  The first
    seed, 50, meets that at the first draw for both networks and both paths (computed on the CPU from the float64 model's coordinates:
    60 distinct entries per level, 32 from the 8 pixels the mask passes); the loop redraws with the next seed otherwise."""
    net = _net(ind_dim)
    offs = net.torso_encoder.offsets.cpu().long()
    for seed in range(50, 54):
        c = _scattered(ind_dim, seed)
        gf, denc, u = _grads(c, path, "fixed")
        live = (u >= 0).all(-1).cpu()   # a masked-out pixel carries u = -1 and zeros
        assert bool((denc[:, ~live.cuda()] == 0).all())
        e = _fine_entries(u[live.cuda()], net)
        if int(live.sum()) >= 5 and all(e[:, j].unique().numel() == e[:, j].numel() for j in (0, 1)):
            break
    else:
        pytest.fail("no draw with single-term entries at levels 14 and 15")
    ga, _, _ = _grads(c, path, "atomic")
    go, _, _ = _grads(c, path, "ordered")
    for j, l in enumerate((14, 15)):
        lo, hi = int(offs[l]), int(offs[l + 1])
        a, o, f = ga[TABLE][lo:hi], go[TABLE][lo:hi], gf[TABLE][lo:hi]
        rows = e[:, j].reshape(-1).cuda()
        assert bool((a[rows] != 0).any(-1).all())                    # every corner got its term ...
        mask = torch.zeros(hi - lo, dtype=torch.bool, device="cuda")
        mask[rows] = True
        assert not bool(a[~mask].any()) and not bool(o[~mask].any()) and not bool(f[~mask].any())   # ... and nothing else did
        assert torch.equal(a[rows], o[rows]) and torch.equal(a[rows], f[rows]), l


# ---- f. the float64 model -------------------------------------------------------------------------------------------------------------
MODEL_CASES = [("case_f", 0, "tensor", True), ("case_f", 8, "tensor", True), ("case_c", 0, False), ("case_c", 8, False)] + \
              [("case_size", N) for N in (1, 15, 16, 17, 4099)]


@pytest.mark.parametrize("key", MODEL_CASES, ids=lambda k: "-".join(str(v) for v in k))
@pytest.mark.parametrize("mode", MODES)
def test_gradients_meet_the_float64_model(mode, key):
    """the cases and bounds of tests/test_gpu_torso_train_branches.py: run_torso with the mask and a per-pixel background (regime F: 1e-4
    x max for the MLP weights, 2e-3 x max for the rest), forward() with the clamp active and the tail sizes (regime C: 2e-4 x max)"""
    from lzzx_nerf_amd.torso_train import FusedTorsoTrainNet
    c, (ref, _) = _case(key), _ref(key)
    net = FusedTorsoTrainNet(ind_dim_torso=c.ind_dim, torso_shrink=c.shrink, table_grad=mode).cuda()
    net.load_state_dict(c.sd)
    _check("%s %s" % (mode, key), c, ref, _model_backward(net, c, _model_forward(net, c)))


# ---- g. GradScaler ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["n17", "rand3000", "block64"])
@pytest.mark.parametrize("ind_dim", [0, 8])
def test_fixed_scales_exactly_with_a_power_of_two(ind_dim, shape):
    """every rows element is linear in the upstream gradients, so x 2^10 is exact; the level's exponent moves with its maximum, so the
    integers that are summed are the same"""
    c = _inputs(shape, ind_dim)
    g, denc, _ = _grads(c, "run_torso", "fixed")
    gs, denc_s, _ = _grads(c, "run_torso", "fixed", scale=1024.0)
    assert torch.equal(denc_s, denc * 1024.0)
    assert torch.equal(gs[TABLE], g[TABLE] * 1024.0) and bool(g[TABLE].any())


# ---- h. the default does not follow the global mode ------------------------------------------------------------------------------------
@pytest.mark.parametrize("ind_dim", [0, 8])
def test_default_net_takes_the_atomic_call_under_a_global_fixed_mode(ind_dim):
    from lzzx_nerf_amd import gridencoder
    from lzzx_nerf_amd.torso_train import FusedTorsoTrainNet
    c = _inputs("rand3000", ind_dim)
    base, _, _ = _grads(c, "run_torso", "atomic")
    prev = gridencoder.set_table_grad("fixed")
    try:
        net = FusedTorsoTrainNet(ind_dim_torso=ind_dim, torso_shrink=0.8).cuda()
        net.load_state_dict(T.state("F", ind_dim))
        assert net.table_grad == "atomic"
        net.keep_denc = True
        cc = c.ind.cuda().requires_grad_(True) if c.ind is not None else None
        out = net.run_torso(c.xy.cuda(), c.pose.cuda(), cc, bg_color=c.bg.cuda(), density_grid=c.grid.cuda(), density_thresh=THRESH)
        ((out["torso_alpha"] * c.ga.cuda()).sum() + (out["torso_color"] * c.gc.cuda()).sum() + (out["deform"] * c.gd.cuda()).sum()).backward()
        assert net.last_denc is None and net.last_u is None   # the rows call was not made
        g = {k: p.grad for k, p in net.named_parameters()}
        if cc is not None:
            g["ind_code"] = cc.grad
    finally:
        gridencoder.set_table_grad(prev)
    assert gridencoder.table_grad() == prev
    for k in base:
        if k != TABLE:
            assert torch.equal(g[k], base[k]), k
    assert bool(g[TABLE].any())


# ---- i. the empty batch ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["forward", "run_torso"])
@pytest.mark.parametrize("mode", ("atomic",) + MODES)
@pytest.mark.parametrize("ind_dim", [0, 8])
def test_empty_batch_returns_zero_gradients(ind_dim, mode, path):
    c = _inputs("empty", ind_dim, torch.zeros(0, 2))
    g, denc, u = _grads(c, path, mode)
    net = _net(ind_dim)
    assert denc is None and u is None
    for k, p in net.named_parameters():
        assert g[k].shape == p.shape and not bool(g[k].any()), k
    if ind_dim:
        assert g["ind_code"].shape == (1, ind_dim) and not bool(g["ind_code"].any())
