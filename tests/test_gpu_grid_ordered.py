"""The ordered table gradient (lz_grid_encode_backward_ordered, gridencoder.set_table_grad("ordered")): no float atomics, every table
entry summed in the CPU checker's (level, sample ascending, corner ascending) order -- so it EQUALS oracle.grid_encode_backward bit for
bit, repeats on every call, continues a sum across consecutive sample ranges and does not depend on the workspace size.  Small tables
make entries collide heavily, so that the order matters (see the guard test: the checker itself gives other bits for another order)."""
import copy
import functools

import numpy as np
import pytest
import torch

from lzzx_nerf_amd import _lib, gridencoder
from lzzx_nerf_amd import raymarching as R
from lzzx_nerf_amd._util import call, ptr, stream
from lzzx_nerf_amd.encoding import get_encoder
from lzzx_nerf_amd.ngp_train import FusedHashgridTrainNeRF, _pack, _workspace
from lzzx_nerf_amd.synthetic import GenericHashgridNeRF, ellipsoid_bitfield_device, synthetic_camera
from lzzx_nerf_amd.utils import frame_rays

pytestmark = pytest.mark.gpu

ENCODERS = {
    "d3_t17": ("hashgrid", dict(input_dim=3, level_dim=2, num_levels=16, base_resolution=16, log2_hashmap_size=17, desired_resolution=2048)),
    "d3_t8": ("hashgrid", dict(input_dim=3, level_dim=2, num_levels=16, base_resolution=16, log2_hashmap_size=8, desired_resolution=2048)),
    "plane": ("hashgrid", dict(input_dim=2, level_dim=1, num_levels=12, base_resolution=64, log2_hashmap_size=14, desired_resolution=512)),
    "tiled_ac": ("tiledgrid", dict(input_dim=2, level_dim=2, num_levels=4, base_resolution=16, log2_hashmap_size=10, desired_resolution=128,
                                   align_corners=True)),
    "c4": ("hashgrid", dict(input_dim=3, level_dim=4, num_levels=2, base_resolution=16, log2_hashmap_size=9, desired_resolution=32)),
    "c8": ("hashgrid", dict(input_dim=2, level_dim=8, num_levels=2, base_resolution=16, log2_hashmap_size=9, desired_resolution=64)),
}
SIZES = [1, 63, 64, 65, 257, 4099, 70001]


@functools.lru_cache(maxsize=None)
def _encoder(name):
    kind, kw = ENCODERS[name]
    enc, _ = get_encoder(kind, **kw)
    return enc


def _hyper(enc):
    return dict(D=enc.input_dim, C=enc.level_dim, L=enc.num_levels, S=float(np.float32(np.log2(enc.per_level_scale))), H=int(enc.base_resolution),
                gridtype=enc.gridtype_id, ac=bool(enc.align_corners), offsets=enc.offsets.numpy().astype(np.int32), shape=tuple(enc.embeddings.shape))


@functools.lru_cache(maxsize=None)
def _data(name, B):
    """inputs [B, D] in [0, 1] with a few rows outside, grad [B, L*C] ~ N(0, 1); shared and never modified"""
    enc = _encoder(name)
    rng = np.random.default_rng(1000 * sorted(ENCODERS).index(name) + B % 997)
    x = rng.random((B, enc.input_dim), dtype=np.float32)
    if B >= 63:
        x[5, 0], x[17, -1], x[B - 1, 0], x[B // 2, 0] = -0.25, 1.5, 1.0000001, -1e-7
    g = rng.standard_normal((B, enc.num_levels * enc.level_dim)).astype(np.float32)
    x.setflags(write=False)
    g.setflags(write=False)
    return x, g


def _oracle(name, x, g, dy_dx=None):
    from oracle import oracle as O
    enc = _encoder(name)
    return O.grid_encode_backward(g, x, tuple(enc.embeddings.shape), enc.offsets.numpy(), enc.per_level_scale, enc.base_resolution, dy_dx,
                                  enc.gridtype_id, enc.align_corners)


@functools.lru_cache(maxsize=None)
def _reference(name, B):
    x, g = _data(name, B)
    ge, _ = _oracle(name, x, g)
    ge.setflags(write=False)
    return ge


def _bits(a):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _run(name, x, g, layout=1, out=None, dy_dx=None, ws_bytes=None, check=True):
    """lz_grid_encode_backward_ordered straight from the C ABI; x, g: numpy or cuda tensors ([B, D], [B, L*C]).  Returns (grad_embeddings,
    grad_inputs | None, return code)"""
    h = _hyper(_encoder(name))
    x = (x if torch.is_tensor(x) else torch.from_numpy(np.array(x))).cuda().contiguous()
    g = (g if torch.is_tensor(g) else torch.from_numpy(np.array(g))).cuda().contiguous()
    B = x.shape[0]
    if layout == 0:
        g = g.view(B, h["L"], h["C"]).permute(1, 0, 2).contiguous()
    ge = torch.zeros(h["shape"], device="cuda") if out is None else out
    off = torch.from_numpy(h["offsets"]).cuda()
    need = int(_lib.load().lz_grid_ordered_workspace(B, h["D"]))
    nbytes = need if ws_bytes is None else ws_bytes
    ws = torch.empty(max(nbytes, 256), dtype=torch.uint8, device="cuda")
    jac = gi = None
    if dy_dx is not None:
        jac, gi = torch.from_numpy(np.array(dy_dx, dtype=np.float32)).cuda().contiguous(), torch.zeros(B, h["D"], device="cuda")
    rc = _lib.load().lz_grid_encode_backward_ordered(ptr(g), ptr(x), None, ptr(off), ptr(ge), B, h["D"], h["C"], h["L"], h["S"], h["H"], ptr(jac),
                                                     ptr(gi), h["gridtype"], int(h["ac"]), 0, layout, ptr(ws), nbytes & 0xFFFFFFFF, nbytes >> 32,
                                                     stream())
    if check:
        _lib.check(rc, "lz_grid_encode_backward_ordered")
    torch.cuda.synchronize()
    return ge, gi, rc


@pytest.mark.parametrize("B", SIZES)
@pytest.mark.parametrize("name", sorted(ENCODERS))
def test_equals_the_checker_bit_for_bit(name, B):
    from oracle import oracle as O
    enc = _encoder(name)
    x, g = _data(name, B)
    ref = _bits(_reference(name, B))
    for layout in (0, 1):
        ge, _, _ = _run(name, x, g, layout)
        got = _bits(ge)
        print(name, B, "layout", layout, "entries that differ:", int((got != ref).sum()), "of", ref.size)
        assert np.array_equal(got, ref), (name, B, layout)
    _, jac = O.grid_encode_forward(x, enc.embeddings.detach().numpy(), enc.offsets.numpy(), enc.per_level_scale, enc.base_resolution, True,
                                   enc.gridtype_id, enc.align_corners)
    _, gi_ref = _oracle(name, x, g, jac)
    for layout in (0, 1):
        ge, gi, _ = _run(name, x, g, layout, dy_dx=jac)
        assert np.array_equal(_bits(ge), ref), (name, B, layout, "with dy_dx")
        assert np.array_equal(_bits(gi), _bits(gi_ref)), (name, B, layout, "grad_inputs")


@pytest.mark.parametrize("name", ["d3_t17", "d3_t8"])
def test_the_checker_itself_depends_on_the_order(name):
    """the guard on the inputs (CPU only): the checker fed the samples in reverse gives other bits in most entries with >= 8 terms, so the
    parity test above cannot pass with a wrong order"""
    from oracle import oracle as O
    enc = _encoder(name)
    B = 4099
    x, g = _data(name, B)
    fwd = _bits(_reference(name, B))
    rev = _bits(_oracle(name, x[::-1].copy(), g[::-1].copy())[0])
    idx = O.grid_corner_indices(x, enc.offsets.numpy(), enc.level_dim, enc.per_level_scale, enc.base_resolution, enc.gridtype_id, enc.align_corners)
    idx = idx[idx >= 0].astype(np.int64)                                   # element offset of channel 0 of every term's entry
    terms = np.bincount(idx // enc.level_dim, minlength=enc.embeddings.shape[0])
    busy = terms >= 8
    differ = (fwd != rev).any(axis=1)
    print(name, "entries with >= 8 terms:", int(busy.sum()), "of which differ:", int((differ & busy).sum()))
    assert busy.sum() > 100
    assert (differ & busy).sum() > 0.5 * busy.sum()


@pytest.mark.parametrize("name", ["d3_t17", "d3_t8", "plane"])
def test_same_bits_twice(name):
    x, g = _data(name, 4099)
    a, _, _ = _run(name, x, g)
    b, _, _ = _run(name, x, g)
    assert np.array_equal(_bits(a), _bits(b))


@pytest.mark.parametrize("name", ["d3_t17", "d3_t8", "plane", "c8"])
def test_split_and_continue(name):
    x, g = _data(name, 4099)
    ge, _, _ = _run(name, x[:1500], g[:1500])
    ge, _, _ = _run(name, x[1500:], g[1500:], out=ge)
    assert np.array_equal(_bits(ge), _bits(_reference(name, 4099)))


@pytest.mark.parametrize("B", [257, 4099, 70001])
@pytest.mark.parametrize("name", ["d3_t17", "d3_t8", "plane", "c4"])
def test_workspace_size_does_not_change_the_bits(name, B):
    x, g = _data(name, B)
    full = int(_lib.load().lz_grid_ordered_workspace(B, _encoder(name).input_dim))
    small = (full // 7) // 256 * 256
    for layout in (0, 1):
        ge, _, _ = _run(name, x, g, layout, ws_bytes=small)
        assert np.array_equal(_bits(ge), _bits(_reference(name, B))), (name, B, layout, small, full)


def test_workspace_too_small_for_one_sample_is_an_argument_error():
    x, g = _data("d3_t8", 257)
    ge, _, rc = _run("d3_t8", x, g, ws_bytes=256, check=False)
    assert rc == -2, (rc, _lib.load().lz_last_error())
    assert not ge.any()


@pytest.mark.parametrize("name", ["d3_t8", "plane"])
def test_exact_scaling(name):
    x, g = _data(name, 4099)
    ge, _, _ = _run(name, x, g * np.float32(65536.0))
    ref = _reference(name, 4099) * np.float32(65536.0)
    assert np.array_equal(_bits(ge), _bits(ref))


@pytest.mark.parametrize("name", ["d3_t17", "d3_t8"])
def test_non_finite_gradients_poison_what_the_checker_poisons(name):
    x, g = _data(name, 4099)
    g = g.copy()
    g[100, 3], g[2000, 17] = np.inf, np.nan
    ref, _ = _oracle(name, x, g)
    ge, _, _ = _run(name, x, g)
    got = ge.cpu().numpy()
    assert np.isnan(ref).any() and np.isinf(ref).any()
    assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(np.isinf(got), np.isinf(ref))
    ok = np.isfinite(ref)
    assert np.array_equal(_bits(got)[ok], _bits(ref)[ok])
    assert np.array_equal(_bits(got)[np.isinf(ref)], _bits(ref)[np.isinf(ref)])


def test_all_rows_out_of_bounds_leave_the_buffer_untouched():
    x, g = _data("d3_t8", 257)
    x = x.copy()
    x[:, 1] = 1.25
    before = torch.randn(_hyper(_encoder("d3_t8"))["shape"], generator=torch.Generator().manual_seed(2)).cuda()
    ge, _, _ = _run("d3_t8", x, g, out=before.clone())
    assert np.array_equal(_bits(ge), _bits(before))


def test_autograd_switch(monkeypatch):
    name = "d3_t8"
    enc = copy.deepcopy(_encoder(name)).cuda()
    x01, g = _data(name, 4099)
    pts = (torch.from_numpy(x01.copy()) * 2 - 1).cuda()
    unit = ((pts + 1) / 2).cpu().numpy()                     # GridEncoder.forward's own mapping (grid.py:143)
    ref, _ = _oracle(name, unit, g)
    calls = []
    real = gridencoder.grid_backward_ordered
    monkeypatch.setattr(gridencoder, "grid_backward_ordered", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    assert gridencoder.table_grad() == "atomic"
    prev = gridencoder.set_table_grad("ordered")
    try:
        assert prev == "atomic" and gridencoder.table_grad() == "ordered"
        enc(pts).backward(torch.from_numpy(g.copy()).cuda())
        assert len(calls) == 1
        assert np.array_equal(_bits(enc.embeddings.grad), _bits(ref))
        with pytest.raises(ValueError):
            gridencoder.set_table_grad("sorted")
        assert gridencoder.table_grad() == "ordered"
        # half tables (autocast, even level_dim) are refused, not summed some other way
        enc.embeddings.grad = None
        with torch.autocast("cuda", dtype=torch.float16):
            out = enc(pts)
        assert out.dtype == torch.float16
        with pytest.raises(RuntimeError, match="f32 tables only"):
            out.backward(torch.from_numpy(g.copy()).cuda().half())
    finally:
        assert gridencoder.set_table_grad(prev) == "ordered"
    # back on the default: the atomic scatter, equal up to the summation order.  Any order's error is below eps * (sum of the magnitudes
    # of an entry's terms) <= 2^-23 * (8 B terms) * max |g| (weights <= 1)
    enc.embeddings.grad = None
    enc(pts).backward(torch.from_numpy(g.copy()).cuda())
    assert len(calls) == 1 and gridencoder.table_grad() == "atomic"
    bound = 2.0 ** -23 * 8 * 4099 * float(np.abs(g).max())
    assert float(np.abs(enc.embeddings.grad.cpu().numpy().astype(np.float64) - ref).max()) <= bound


# ---- the fused hash-grid network -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def generic():
    return GenericHashgridNeRF("cuda", seed=3)


def _fused(g, table_grad="ordered"):
    return FusedHashgridTrainNeRF(copy.deepcopy(g.enc), copy.deepcopy(g.sigma_net), copy.deepcopy(g.color_net), table_grad=table_grad).cuda()


def _weights(m):
    return [m.sigma_net.net[0].weight, m.sigma_net.net[1].weight, m.color_net.net[0].weight, m.color_net.net[1].weight]


def _points(M, seed):
    gen = torch.Generator().manual_seed(seed)
    xyzs = (torch.rand(M, 3, generator=gen) * 1.9 - 0.95).cuda()
    d = torch.randn(M, 3, generator=gen)
    dirs = (d / d.norm(dim=-1, keepdim=True)).cuda()
    return xyzs, dirs, torch.randn(M, generator=gen).cuda(), torch.randn(M, 3, generator=gen).cuda()


def _table_grad_of(net, xyzs, dirs, gs, gr, bound=1.0):
    for p in net.parameters():
        p.grad = None
    sigma, rgb = net(xyzs, dirs, bound)
    torch.autograd.backward([sigma, rgb], [gs, gr])
    return net.encoder.embeddings.grad.clone()


def _d_feats(net, xyzs, dirs, gs, gr, bound=1.0):
    """lz_ngp_head_backward's d feats [16, M, 2] straight from the entry point"""
    M = xyzs.shape[0]
    ws = [w.detach().contiguous() for w in _weights(net)]
    e = net.encoder
    feats = torch.empty(M, 32, device="cuda")
    call("lz_grid_encode_forward_tiled", ptr(xyzs), ptr(e.embeddings), ptr(e.offsets), ptr(feats), M, None, bound, 3, 2, 16, net._S, net._H, 0, 0, 0,
         stream())
    d = torch.empty(16, M, 2, device="cuda")
    gw = [torch.empty_like(w) for w in ws]
    call("lz_ngp_head_backward", ptr(_pack(ws)), *[ptr(w) for w in ws], ptr(feats), ptr(dirs), M, None, ptr(gs), ptr(gr), ptr(d), *[ptr(t) for t in gw],
         ptr(_workspace(xyzs.device)), stream())
    return d


@pytest.mark.parametrize("M", [1, 257, 4099])
def test_fused_net_table_gradient_repeats_and_equals_the_checker(generic, M):
    with pytest.raises(ValueError):
        FusedHashgridTrainNeRF(table_grad="sorted")
    net = _fused(generic)
    xyzs, dirs, gs, gr = _points(M, 40 + M)
    ref = _table_gradient_repeats_and_equals_the_checker(net, xyzs, dirs, gs, gr, 1.0)
    # the module switch is what table_grad=None follows
    follow = _fused(generic, None)
    prev = gridencoder.set_table_grad("ordered")
    try:
        c = _table_grad_of(follow, xyzs, dirs, gs, gr)
    finally:
        gridencoder.set_table_grad(prev)
    assert np.array_equal(_bits(c), _bits(ref))


def _table_gradient_repeats_and_equals_the_checker(net, xyzs, dirs, gs, gr, bound):
    from oracle import oracle as O
    M = xyzs.shape[0]
    a = _table_grad_of(net, xyzs, dirs, gs, gr, bound)
    b = _table_grad_of(net, xyzs, dirs, gs, gr, bound)
    assert np.array_equal(_bits(a), _bits(b))
    d = _d_feats(net, xyzs, dirs, gs, gr, bound).permute(1, 0, 2).reshape(M, 32).cpu().numpy()
    unit = O.map01(xyzs.cpu().numpy(), bound)
    e = net.encoder
    ref, _ = O.grid_encode_backward(d, unit, tuple(e.embeddings.shape), e.offsets.cpu().numpy(), e.per_level_scale, e.base_resolution)
    assert np.array_equal(_bits(a), _bits(ref))
    return ref


def test_fused_net_table_gradient_repeats_and_equals_the_checker_at_bound_1p5(generic):
    """2 bound = 3: the scatter's coordinates are the gather's (tests/bound_cases.py: rows whose cell differs under a true division)"""
    import bound_cases as BC
    M = 257
    _, dirs, gs, gr = _points(M, 40 + M)
    xyzs = torch.from_numpy(BC.points(1.5, M, "cfg2").copy()).cuda()
    _table_gradient_repeats_and_equals_the_checker(_fused(generic), xyzs, dirs, gs, gr, 1.5)


def _five_steps(generic, ro, rd, nears, fars, bits, target):
    net = _fused(generic)
    params = list(net.parameters())
    opt = torch.optim.Adam(params, lr=1e-2, betas=(0.9, 0.99), eps=1e-15)
    for _ in range(5):
        ctr = torch.zeros(2, dtype=torch.int32, device="cuda")
        xyzs, dirs, deltas, rays = R.march_rays_train(ro, rd, 1.0, bits, 1, 128, nears, fars, ctr, -1, False, 128, True, 1 / 256, 32)
        sigma, rgb = net(xyzs.detach().contiguous(), dirs.detach().contiguous(), 1.0)
        ws, _, _, img = R.composite_rays_train(sigma, rgb, torch.zeros_like(sigma), deltas, rays)
        loss = ((img + (1 - ws)[:, None] - target) ** 2).mean()
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
    return [p.detach().clone() for p in params]


def test_whole_training_step_repeats_bit_for_bit(generic):
    """march -> net -> composite -> MSE -> backward -> Adam, five steps, twice from one initialisation and one ray batch: every parameter
    ends with the same bits"""
    H = W = 64
    pose, intr = synthetic_camera(H, W)
    ro, rd = frame_rays(torch.from_numpy(pose).cuda(), intr, H, W)
    bits, _ = ellipsoid_bitfield_device("cuda")
    aabb = torch.tensor([-1, -1, -1, 1, 1, 1], dtype=torch.float32, device="cuda")
    nears, fars = R.near_far_from_aabb(ro, rd, aabb, 0.05)
    target = torch.rand(H * W, 3, generator=torch.Generator().manual_seed(5)).cuda()
    a = _five_steps(generic, ro, rd, nears, fars, bits, target)
    b = _five_steps(generic, ro, rd, nears, fars, bits, target)
    for i, (p, q) in enumerate(zip(a, b)):
        n = int((_bits(p) != _bits(q)).sum())
        print("parameter", i, tuple(p.shape), "elements that differ:", n)
    for p, q in zip(a, b):
        assert np.array_equal(_bits(p), _bits(q))
