"""The three-plane encoder (gridencoder.TriplaneEncoder, csrc/lz_triplane_enc.hip) against the path it replaces: three GridEncoders and a
torch.cat (network.py:208-223).  Forward, Jacobian-based input gradient and the ordered table gradient are compared bit for bit; the
atomic table gradient against the ordered one within the bound of a reordered float sum."""
import functools
import types

import numpy as np
import pytest
import torch

from lzzx_nerf_amd import _lib, gridencoder
from lzzx_nerf_amd._util import call, ptr, stream
from lzzx_nerf_amd.gridencoder import GridEncoder, TriplaneEncoder

pytestmark = pytest.mark.gpu

# "reference": what network.py:131-133 builds (desired_resolution = 512 * bound); "small": the second configuration, whose four levels
# are all hashed (17^2 > 2^8); "mixed": a dense level next to hashed ones in a table as small; "wide": a level of 2^15 entries, too big
# for the backward's LDS accumulator
CONFIGS = {
    "reference": lambda bound: dict(num_levels=12, base_resolution=64, log2_hashmap_size=14, desired_resolution=512 * bound),
    "small": lambda bound: dict(num_levels=4, base_resolution=16, log2_hashmap_size=8),
    "mixed": lambda bound: dict(num_levels=4, base_resolution=16, log2_hashmap_size=10),
    "wide": lambda bound: dict(num_levels=2, base_resolution=16, log2_hashmap_size=15, per_level_scale=16),
}


@functools.lru_cache(maxsize=None)
def encoders(config, bound):
    """three seeded GridEncoders on the GPU (tables uniform in [-1, 1]) and the operator over them; shared, never modified"""
    g = torch.Generator().manual_seed(1234 + 17 * sorted(CONFIGS).index(config))
    encs = []
    for _ in range(3):
        e = GridEncoder(input_dim=2, level_dim=1, **CONFIGS[config](bound))
        with torch.no_grad():
            e.embeddings.copy_(torch.rand(e.embeddings.shape, generator=g) * 2 - 1)
        encs.append(e.cuda())
    return tuple(encs), TriplaneEncoder(*encs)


@functools.lru_cache(maxsize=None)
def points(B, bound):
    """uniform in the box; from 8 rows on: the box's corners exactly at +-bound, one row per coordinate outside the box, and the last row
    of the batch (the end of a partial wave) on the box's surface"""
    g = torch.Generator().manual_seed(99 + B)
    x = (torch.rand(B, 3, generator=g) * 2 - 1) * bound
    if B >= 8:
        b = float(bound)
        x[0] = torch.tensor([b, b, b])
        x[1] = torch.tensor([-b, -b, -b])
        x[2] = torch.tensor([b, -b, 0.25 * b])
        x[3, 0] = 1.25 * b          # x outside: zeroes xy and xz, leaves yz
        x[4, 1] = -1.5 * b          # y outside: zeroes xy and yz
        x[5, 2] = b * (1 + 2.0 ** -20)   # z just outside: zeroes yz and xz
        x[B - 1] = torch.tensor([-b, 0.5 * b, b])
    return x.cuda()


def three(encs, xyz, bound):
    """NeRFNetwork.encode_x, network.py:208-223"""
    return torch.cat([encs[0](xyz[:, :2], bound=bound), encs[1](xyz[:, 1:], bound=bound), encs[2](xyz[:, [0, 2]], bound=bound)], -1)


def grads_of(encs):
    g = [e.embeddings.grad.clone() for e in encs]
    for e in encs:
        e.embeddings.grad = None
    return g


@pytest.fixture
def ordered():
    prev = gridencoder.set_table_grad("ordered")
    yield
    gridencoder.set_table_grad(prev)


@pytest.mark.parametrize("config", ["reference", "small", "mixed"])
@pytest.mark.parametrize("bound", [1, 1.5, 2])      # 1.5: 2 bound is no power of two (tests/bound_cases.py)
@pytest.mark.parametrize("B", [1, 63, 64, 65, 1000, 70001])
def test_forward_equals_the_three_encoders(config, bound, B):
    encs, tri = encoders(config, bound)
    xyz = points(B, bound)
    L = encs[0].num_levels
    with torch.no_grad():
        got, want = tri(xyz, bound=bound), three(encs, xyz, bound)
    assert got.shape == (B, 3 * L) and got.dtype == torch.float32
    assert torch.equal(got, want)
    if B >= 8:
        z = torch.zeros(L, device="cuda")
        for row, dead, alive in ((3, (0, 2), 1), (4, (0, 1), 2), (5, (1, 2), 0)):
            for p in dead:
                assert torch.equal(got[row, p * L:(p + 1) * L], z), (row, p)
            assert bool(got[row, alive * L:(alive + 1) * L].abs().max() > 0), (row, alive)
        assert bool((got[:3].abs().amax(1) > 0).all()) and bool(got[B - 1].abs().max() > 0)    # +-bound is inside the box
    if B <= 1000:
        from oracle import oracle as O
        from oracle.head import encode_x
        e = encs[0]
        spec = types.SimpleNamespace(bound=float(bound), per_level_scale=e.per_level_scale, base_resolution=e.base_resolution,
                                     offsets=O.grid_offsets(2, L, e.per_level_scale, e.base_resolution, e.log2_hashmap_size))
        assert np.array_equal(spec.offsets, e.offsets.cpu().numpy())
        P = {"encoder_%s.embeddings" % n: enc.embeddings.detach().cpu().numpy() for n, enc in zip(("xy", "yz", "xz"), encs)}
        assert np.array_equal(got.cpu().numpy(), encode_x(spec, xyz.cpu().numpy(), P))


@pytest.mark.parametrize("with_jacobian", [False, True])
@pytest.mark.parametrize("B", [1, 65])
def test_nothing_is_written_past_row_B(B, with_jacobian):
    encs, _ = encoders("reference", 1)
    L, e = 12, encs[0]
    xyz = points(B, 1)
    sentinel = 0x7FC12345                         # a NaN payload no kernel produces
    rows = B + 130                                # room for two more waves behind the batch
    buf = torch.full((rows * 3 * L,), sentinel, dtype=torch.int32, device="cuda")
    jac = torch.full((3 * rows * L * 2,), sentinel, dtype=torch.int32, device="cuda") if with_jacobian else None
    S = float(np.float32(np.log2(e.per_level_scale)))
    call("lz_triplane_encode_forward", ptr(xyz), ptr(encs[0].embeddings), ptr(encs[1].embeddings), ptr(encs[2].embeddings), ptr(e.offsets), ptr(buf),
         ptr(jac), B, L, S, int(e.base_resolution), 1.0, stream())
    torch.cuda.synchronize()
    with torch.no_grad():
        want = three(encs, xyz, 1)
    assert torch.equal(buf[:B * 3 * L].view(torch.float32).view(B, 3 * L), want)
    assert bool((buf[B * 3 * L:] == sentinel).all())
    if with_jacobian:
        assert bool((jac[:3 * B * L * 2] != sentinel).all()) and bool((jac[3 * B * L * 2:] == sentinel).all())


def test_empty_batch():
    encs, tri = encoders("reference", 1)
    xyz = torch.zeros(0, 3, device="cuda", requires_grad=True)
    out = tri(xyz, bound=1)
    assert out.shape == (0, 36) and out.dtype == torch.float32
    out.sum().backward()
    assert xyz.grad.shape == (0, 3)
    for g in grads_of(encs):
        assert not bool(g.any())


def _upstream(B, W, seed=5):
    return torch.randn(B, W, generator=torch.Generator().manual_seed(seed + B)).cuda()


@pytest.mark.parametrize("config", ["reference", "mixed"])
@pytest.mark.parametrize("B", [65, 1000])
def test_ordered_table_gradient_equals_the_three_encoders(ordered, config, B):
    _ordered_equals_the_three_encoders(config, B, 1)


@pytest.mark.parametrize("B", [65, 1000])
def test_ordered_table_gradient_equals_the_three_encoders_at_bound_1p5(ordered, B):
    _ordered_equals_the_three_encoders("reference", B, 1.5)


def _ordered_equals_the_three_encoders(config, B, bound):
    encs, tri = encoders(config, bound)
    xyz, up = points(B, bound), _upstream(B, 3 * encs[0].num_levels)
    three(encs, xyz, bound).backward(up)
    want = grads_of(encs)
    tri(xyz, bound=bound).backward(up)
    got = grads_of(encs)
    tri(xyz, bound=bound).backward(up)
    again = grads_of(encs)
    for w, g, a in zip(want, got, again):
        assert bool(w.any())
        assert torch.equal(g, w) and torch.equal(a, g)


def _ordered_reference(encs, tri, xyz, up, bound=1):
    """the ordered sum of the terms, and per entry A = sum |w g| (the ordered path on |grad|)"""
    prev = gridencoder.set_table_grad("ordered")
    try:
        tri(xyz, bound=bound).backward(up)
        ref = grads_of(encs)
        tri(xyz, bound=bound).backward(up.abs())
        mag = grads_of(encs)
    finally:
        gridencoder.set_table_grad(prev)
    return ref, mag


# B = 16384 is where the backward changes from global float atomics to the per-(plane, level, chunk) accumulator in LDS; "wide" has a
# level that does not fit that accumulator and takes the global path inside the same launch
@pytest.mark.parametrize("config,B", [("reference", 65), ("reference", 1000), ("mixed", 1000), ("reference", 16383), ("reference", 16384),
                                      ("reference", 70001), ("mixed", 70001), ("wide", 16384)])
def test_atomic_table_gradient_is_the_ordered_sum_reordered(config, B):
    """Per entry |atomic - ordered| <= n 2^-24 A: both add the same f32 terms w g, in different orders; n = 4 B bounds the number of terms
    into one entry and A is the entry's sum of |w g|.  Entries no sample touches are exactly zero in both."""
    _atomic_is_the_ordered_sum_reordered(config, B, 1)


@pytest.mark.parametrize("B", [1000, 16384])       # global atomics, and the accumulator in LDS
def test_atomic_table_gradient_is_the_ordered_sum_reordered_at_bound_1p5(B):
    """the same bound on |atomic - ordered|, where the scatter's coordinates come from a reciprocal that is not exact"""
    _atomic_is_the_ordered_sum_reordered("reference", B, 1.5)


def _atomic_is_the_ordered_sum_reordered(config, B, bound):
    assert gridencoder.table_grad() == "atomic"
    encs, tri = encoders(config, bound)
    xyz, up = points(B, bound), _upstream(B, 3 * encs[0].num_levels)
    ref, mag = _ordered_reference(encs, tri, xyz, up, bound)
    tri(xyz, bound=bound).backward(up)
    got = grads_of(encs)
    n = 4 * B
    for plane, (g, r, a) in enumerate(zip(got, ref, mag)):
        g, r, a = g.double(), r.double(), a.double()
        untouched = a == 0
        assert bool(untouched.any()) and bool((~untouched).any())
        assert not bool(g[untouched].any()) and not bool(r[untouched].any())
        excess = ((g - r).abs() / (n * 2.0 ** -24 * a).clamp_min(1e-300))[~untouched]
        print("config %s B %d plane %d: max |atomic - ordered| / bound = %.3g, max |diff| = %.3g" % (config, B, plane, float(excess.max()),
                                                                                                     float((g - r).abs().max())))
        assert float(excess.max()) <= 1.0


@pytest.mark.parametrize("mode", ["atomic", "ordered"])
@pytest.mark.parametrize("bound", [1, 1.5, 2])      # 1.5: 2 bound is no power of two (tests/bound_cases.py)
@pytest.mark.parametrize("B", [65, 1000])
def test_input_gradient_in_the_stated_order(mode, bound, B):
    encs, tri = encoders("reference", bound)
    x0, up = points(B, bound), _upstream(B, 36, seed=11)
    prev = gridencoder.set_table_grad(mode)
    try:
        # the three operator encoders on separate leaves, then d_x = g_xy[0] + g_xz[0], d_y = g_xy[1] + g_yz[0], d_z = g_yz[1] + g_xz[1]
        leaves = [x0[:, cols].clone().requires_grad_() for cols in ([0, 1], [1, 2], [0, 2])]
        torch.cat([enc(leaf, bound=bound) for enc, leaf in zip(encs, leaves)], -1).backward(up)
        gxy, gyz, gxz = (leaf.grad for leaf in leaves)
        want = torch.stack([gxy[:, 0] + gxz[:, 0], gxy[:, 1] + gyz[:, 0], gyz[:, 1] + gxz[:, 1]], 1)
        want_tables = grads_of(encs)
        xyz = x0.clone().requires_grad_()
        tri(xyz, bound=bound).backward(up)
    finally:
        gridencoder.set_table_grad(prev)
    assert bool(want.any()) and torch.equal(xyz.grad, want)
    assert float(xyz.grad[3, 0]) == 0.0 and float(xyz.grad[3, 1]) != 0.0      # x outside the box: only the yz plane reaches that row
    for g, w in zip(grads_of(encs), want_tables):                             # the tables get theirs in the same call
        assert bool(g.any())
        if mode == "ordered":
            assert torch.equal(g, w)


def test_autocast_keeps_f32_like_the_three_encoders():
    encs, tri = encoders("reference", 1)
    xyz = points(1000, 1)
    with torch.no_grad(), torch.autocast("cuda", torch.float16):
        got, want = tri(xyz, bound=1), three(encs, xyz, 1)
    assert got.dtype == want.dtype == torch.float32           # odd level_dim: grid.py:28,38-39
    assert torch.equal(got, want)


def test_strided_upstream_gradient(ordered):
    encs, tri = encoders("reference", 1)
    B = 1000
    xyz = points(B, 1).clone().requires_grad_()
    up_t = _upstream(36, B, seed=3)                # [36, B]; its transpose is a non-contiguous [B, 36] view
    assert not up_t.t().is_contiguous()
    tri(xyz, bound=1).backward(up_t.t())
    strided, gx = grads_of(encs), xyz.grad.clone()
    xyz.grad = None
    tri(xyz, bound=1).backward(up_t.t().contiguous())
    for s, c in zip(strided, grads_of(encs)):
        assert bool(s.any()) and torch.equal(s, c)
    assert torch.equal(gx, xyz.grad)
