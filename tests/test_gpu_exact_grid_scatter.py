"""The free-order table gradients of csrc/lz_grid.hip and csrc/lz_triplane_enc.hip held to bit equality with the CPU checker.  The float
atomics of lz_k_grid_backward and lz_k_grid_backward_xc, the fixed-point LDS accumulators of lz_k_grid_backward_lds_fx (and its in-kernel
fall-back to global atomics) and the triplane encoder's atomic scatter add their terms in an order nobody fixes.  On the inputs of
tests/exact_inputs.py (per_level_scale 2, coordinates k / 2^q, integer gradients) every term and every partial sum is exact in f32, so
all orders give the checker's bits: a dropped corner, a sample of a ragged chunk left out or one added twice is a mismatch, not
rounding.  tests/test_exact_inputs_host.py proves the premise on the checker alone.

Out of scope, because their terms cannot be made exact or belong elsewhere: half tables (11 bits leave no room);
lz_ngp_head_backward, lz_train_wgrad.h and the other fused head gradients (their terms pass through exp and sigmoid); align_corners;
bounds whose double is no power of two."""
import functools

import numpy as np
import pytest
import torch

import exact_inputs as E
from oracle import oracle as O

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()      # a copy: the shared inputs are read-only


def bits(t):
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t
    return np.ascontiguousarray(a).view(np.uint32)


def where_off(got, want):
    g, w = bits(got), bits(want)
    bad = np.argwhere(g != w)
    gf, wf = g.view(np.float32), w.view(np.float32)
    return "%d of %d entries off; first: %s" % (len(bad), g.size, [(tuple(i), float(gf[tuple(i)]), float(wf[tuple(i)])) for i in bad[:6]])


@functools.lru_cache(maxsize=None)
def encoder(name):
    from lzzx_nerf_amd.gridencoder import GridEncoder
    enc = GridEncoder(**E.grid_kwargs(name)).cuda()
    assert enc.per_level_scale == 2.0
    return enc


@functools.lru_cache(maxsize=None)
def reference(name, B):
    """the checker's table gradient and the entries any sample touches (the checker on |grad| is nonzero there); computed once, read-only"""
    D, L, C, H, T, gt, _ = E.GRID_CASES[name]
    enc = encoder(name)
    off = enc.offsets.cpu().numpy()
    assert np.array_equal(off, O.grid_offsets(D, L, 2.0, H, T))
    x, g = E.grid_inputs(name, B)
    gid = 0 if gt == "hash" else 1
    shape = tuple(enc.embeddings.shape)
    ge, _ = O.grid_encode_backward(g, x, shape, off, 2.0, H, None, gid)
    mass, _ = O.grid_encode_backward(np.abs(g), x, shape, off, 2.0, H, None, gid)
    ge.setflags(write=False)
    return ge, mass != 0


CASES = [(n, B) for n in E.GRID_CASES for B in E.GRID_BATCHES[n]]


@pytest.mark.parametrize("name,B", CASES)
def test_c_entry_equals_the_checker_in_every_layout(name, B):
    """lz_grid_encode_backward, grad_layout 0 .. 3.  Layouts 0 / 1: lz_k_grid_backward below 4096 samples and for C = 4,
    lz_k_grid_backward_xc from 4096 on; layouts 2 / 3: lz_k_grid_backward_lds_fx, with levels that fit its LDS accumulator and (D3C2T16)
    levels that take global atomics inside it.  A second launch into the same buffer doubles every entry, still exactly."""
    from lzzx_nerf_amd._util import call, ptr, stream
    D, L, C, H, T, gt, _ = E.GRID_CASES[name]
    enc = encoder(name)
    ge, touched = reference(name, B)
    assert touched.any() and (~touched).any()
    x, g = E.grid_inputs(name, B)
    xt, g_sm = dev(x), dev(g)
    g_lm = g_sm.view(B, L, C).permute(1, 0, 2).contiguous()      # [L, B, C], the reference FFI's layout
    gid = 0 if gt == "hash" else 1
    for layout in (0, 1, 2, 3):
        gemb = torch.zeros_like(enc.embeddings.data)
        gin = g_sm if layout in (1, 2) else g_lm
        for launch in (1, 2):
            call("lz_grid_encode_backward", ptr(gin), ptr(xt), ptr(enc.embeddings.data), ptr(enc.offsets), ptr(gemb), B, D, C, L, 1.0, H, None, None,
                 gid, 0, 0, layout, stream())
            got = gemb.cpu().numpy()
            want = ge * np.float32(launch)
            assert np.array_equal(bits(got), bits(want)), "layout %d launch %d: " % (layout, launch) + where_off(got, want)
        assert not bits(got)[~touched].any()          # entries no sample touches: +0, not even -0


@pytest.mark.parametrize("name,B", CASES)
def test_autograd_wrapper_equals_the_checker(name, B):
    """GridEncoder picks its own kernel (level-resident from 16384 samples on when the levels fit); the bits must not depend on the pick"""
    enc = encoder(name)
    ge, touched = reference(name, B)
    x, g = E.grid_inputs(name, B)
    enc.embeddings.grad = None
    enc(dev(x * 2 - 1), bound=1).backward(dev(g))
    got = enc.embeddings.grad.cpu().numpy()
    enc.embeddings.grad = None
    assert np.array_equal(bits(got), bits(ge)), where_off(got, ge)
    assert not bits(got)[~touched].any()


# ---- three planes -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def planes(config):
    from lzzx_nerf_amd.gridencoder import GridEncoder, TriplaneEncoder
    encs = tuple(GridEncoder(input_dim=2, level_dim=1, **E.PLANE_CONFIGS[config]).cuda() for _ in range(3))
    assert all(e.per_level_scale == 2.0 for e in encs)
    return encs, TriplaneEncoder(*encs)


def grads_of(encs):
    g = [e.embeddings.grad.cpu().numpy() for e in encs]
    for e in encs:
        e.embeddings.grad = None
    return g


@pytest.mark.parametrize("config", sorted(E.PLANE_CONFIGS))
@pytest.mark.parametrize("bound", E.PLANE_BOUNDS)
@pytest.mark.parametrize("B", E.PLANE_BATCHES)
def test_triplane_atomic_table_gradient_equals_ordered_three_encoders_and_checker(config, bound, B):
    """TriplaneEncoder with table_grad "atomic" (global float atomics below 16384 samples, the accumulator in LDS from there on) against
    its "ordered" mode, against the three GridEncoders and against the checker: the same bits four ways"""
    from lzzx_nerf_amd import gridencoder
    encs, tri = planes(config)
    kw = E.PLANE_CONFIGS[config]
    xyz, g = E.plane_inputs(B, bound)
    xt, gt = dev(xyz), dev(g)
    off = encs[0].offsets.cpu().numpy()
    shape = tuple(encs[0].embeddings.shape)
    unit01 = O.map01(xyz, bound)
    want = [O.grid_encode_backward(g[:, 4 * p:4 * p + 4], unit01[:, cols], shape, off, 2.0, kw["base_resolution"], None, 0)[0]
            for p, cols in enumerate(E.PLANE_COLUMNS)]
    assert gridencoder.table_grad() == "atomic"
    tri(xt, bound=bound).backward(gt)
    atomic = grads_of(encs)
    torch.cat([encs[p](xt[:, list(cols)], bound=bound) for p, cols in enumerate(E.PLANE_COLUMNS)], -1).backward(gt)
    three = grads_of(encs)
    prev = gridencoder.set_table_grad("ordered")
    try:
        tri(xt, bound=bound).backward(gt)
        ordered = grads_of(encs)
    finally:
        gridencoder.set_table_grad(prev)
    for p in range(3):
        assert want[p].any()
        for label, got in (("atomic", atomic), ("three encoders", three), ("ordered", ordered)):
            assert np.array_equal(bits(got[p]), bits(want[p])), "plane %d %s: " % (p, label) + where_off(got[p], want[p])
