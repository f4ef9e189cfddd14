"""csrc/lz_linear.hip held to bit equality.  On the integer-valued inputs of tests/exact_inputs.py every product and every partial sum of
the forward, the data gradient and the weight gradient (float atomics, per-workgroup partials through LDS: the order is free) is exact
in f32, so the kernels have to reproduce the integer model with `torch.equal`: a dropped or doubled sample, a wave's partial lost in the
reduction or a ReLU mask off by one column is a mismatch, not rounding.  tests/test_exact_inputs_host.py proves the premise on the CPU.
On ordinary random floats two more things hold without a measured tolerance: the bits of a forward row do not depend on the batch around
it, and every element stays inside the textbook bound of a K-term f32 dot product.

Out of scope, because their terms cannot be made exact or belong elsewhere: half tables (11 bits leave no room);
lz_ngp_head_backward, lz_train_wgrad.h and the other fused head gradients (their terms pass through exp and sigmoid); align_corners;
bounds whose double is no power of two."""
import functools

import numpy as np
import pytest
import torch

import exact_inputs as E

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC12345      # a NaN payload no kernel produces


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()      # a copy: the shared inputs are read-only


def same_bits(got, want_int64):
    """got (a device f32 tensor) is the int64 model, bit for bit: zeros are +0"""
    want = dev(E.as_f32(want_int64))
    return got.shape == want.shape and got.dtype == torch.float32 and torch.equal(got.contiguous().view(torch.int32), want.view(torch.int32))


def where_off(got, want_int64):
    """for the assertion message: how many elements differ, and the first few (index, got, want)"""
    g, w = got.detach().cpu().numpy(), E.as_f32(want_int64)
    bad = np.argwhere(g.view(np.uint32) != w.view(np.uint32))
    return "%d of %d off; first: %s" % (len(bad), g.size, [(tuple(i), float(g[tuple(i)]), float(w[tuple(i)])) for i in bad[:6]])


def run_layer(x, w, gy, relu):
    from lzzx_nerf_amd.linear import lz_linear
    xg, wg = dev(x).requires_grad_(True), dev(w).requires_grad_(True)
    y = lz_linear(xg, wg, relu)
    y.backward(dev(gy))
    return y.detach(), xg.grad, wg.grad


def check_layer(M, K, N, relu):
    x, w, gy = E.linear_case(M, K, N)
    ref = E.linear_reference(x, w, gy, relu)
    y, dx, dw = run_layer(x, w, gy, relu)
    tag = "M %d K %d N %d relu %s: " % (M, K, N, relu)
    assert same_bits(y, ref["y"]), tag + "y " + where_off(y, ref["y"])
    assert same_bits(dx, ref["dx"]), tag + "dx " + where_off(dx, ref["dx"])
    assert same_bits(dw, ref["dw"]), tag + "dW " + where_off(dw, ref["dw"])
    return ref


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("K,N", E.LINEAR_SHAPES)
def test_layer_equals_the_integer_model(K, N, relu):
    """forward, data gradient (gradient 0 where y == 0, no sample excused) and weight gradient at every batch size, ragged ones included"""
    for M in E.LINEAR_BATCHES:
        ref = check_layer(M, K, N, relu)
    if relu:
        assert (ref["pre"] == 0).any() and (ref["gm"] != 0).any()


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("M", [E.M_PAST_FORWARD_CAP, E.M_PAST_GRAD_W_CAP])
def test_layer_past_the_workgroup_caps(M, relu):
    """more sample groups than 2048 workgroups (forward, data gradient) resp. 1536 workgroups of 8 groups per wave (weight gradient) take
    in one round: the grid-stride loops, with a ragged last group"""
    check_layer(M, 36, 64, relu)


def test_c_entry_points_on_column_slices():
    """lz_linear_forward and lz_linear_grad_w with leading dimensions: operands and results are column slices of wider buffers whose
    surroundings hold a NaN sentinel (read: the result is poisoned; written: the sentinel changes), dW starts from integers"""
    from lzzx_nerf_amd._util import call, ptr, stream
    M, K, N = 5003, 36, 64
    x, w, gy = E.linear_case(M, K, N, seed=3)
    rng = np.random.default_rng(8)
    pre = E.linear_reference(x, w, gy, False)["pre"]

    def framed(a, ld, c0):
        buf = torch.full((a.shape[0], ld), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)
        buf[:, c0:c0 + a.shape[1]] = dev(a)
        return buf

    def frame_untouched(buf, c0, width):
        b = buf.view(torch.int32)
        return bool((b[:, :c0] == SENTINEL).all()) and bool((b[:, c0 + width:] == SENTINEL).all())

    # forward: y = relu((x . [mask > 0]) w^T); x and the mask share a leading dimension
    mask = rng.integers(-1, 2, (M, K)).astype(np.float32)
    X, Mk, W, Y = framed(x, 80, 8), framed(mask, 80, 8), framed(w, 50, 3), framed(np.zeros((M, N), np.float32), 100, 16)
    Y[:, 16:16 + N] = 7.0
    call("lz_linear_forward", ptr(X[:, 8:]), 80, ptr(Mk[:, 8:]), ptr(W[:, 3:]), 50, ptr(Y[:, 16:]), 100, M, K, N, 1, stream())
    want = np.maximum(E._exact_matmul(x * (mask > 0), w.T), 0)
    assert same_bits(Y[:, 16:16 + N], want), where_off(Y[:, 16:16 + N], want)
    assert frame_untouched(Y, 16, N) and frame_untouched(X, 8, K) and frame_untouched(W, 3, K)

    # weight gradient: dW += (gy . [y > 0])^T x; gy and the mask share a leading dimension, dW is accumulated into
    y = np.maximum(pre, 0).astype(np.float32)
    dw0 = rng.integers(-5, 6, (N, K)).astype(np.float32)
    G, Ym, DW = framed(gy, 70, 2), framed(y, 70, 2), framed(dw0, 64, 20)
    call("lz_linear_grad_w", ptr(G[:, 2:]), 70, ptr(Ym[:, 2:]), ptr(X[:, 8:]), 80, ptr(DW[:, 20:]), 64, M, K, N, stream())
    want = np.rint(dw0).astype(np.int64) + E.linear_reference(x, w, gy, True)["dw"]
    assert same_bits(DW[:, 20:20 + K], want), where_off(DW[:, 20:20 + K], want)
    assert frame_untouched(DW, 20, K) and frame_untouched(G, 2, N) and frame_untouched(Ym, 2, N)


# ---- ordinary random floats -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def random_case(M, K, N):
    g = torch.Generator().manual_seed(1000 * K + N)
    w = torch.randn(N, K, generator=g) / K ** 0.5
    x = torch.randn(M, K, generator=g)
    gy = torch.randn(M, N, generator=g)
    return x, w, gy


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("K,N", [(36, 64), (116, 32), (1, 5)])
def test_forward_rows_do_not_depend_on_the_batch(K, N, relu):
    """the k order of a row's dot products is fixed by the kernel, so the same five rows give the same bits alone in a 16-row batch,
    mid-batch at M = 5003 (other lanes of the wave, another wave of the workgroup) and as the ragged tail past the 2048-workgroup cap
    (a later trip of the grid-stride loop)"""
    from lzzx_nerf_amd.linear import lz_linear
    big, w, _ = random_case(E.M_PAST_FORWARD_CAP, K, N)
    rows = big[-5:]
    wg = w.cuda()
    with torch.no_grad():
        tail = lz_linear(big.cuda(), wg, relu)[-5:]
        small = torch.zeros(16, K)
        small[:5] = rows
        alone = lz_linear(small.cuda(), wg, relu)[:5]
        mid = big[:5003].clone()
        mid[2501:2506] = rows
        middle = lz_linear(mid.cuda(), wg, relu)[2501:2506]
    assert bool(tail.abs().sum() > 0)
    assert torch.equal(alone, tail) and torch.equal(middle, tail)


@pytest.mark.parametrize("K,N", [(36, 64), (69, 64), (64, 65), (128, 7), (116, 32)])
def test_forward_and_data_gradient_inside_the_dot_product_bound(K, N):
    """|err| <= 2 (K + 1) 2^-24 sum_k |x_k w_k| per element against float64: the bound of a K-term f32 dot product in any order
    (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1: gamma_K with u = 2^-24, plus one rounding of the result), doubled
    for a rounding other than to nearest inside the matrix unit.  Derived, not measured.  With ReLU the data gradient is compared on the rows
    whose float64 pre-activations all stay further than that bound from 0 (elsewhere the mask may legitimately differ)."""
    M = 5003
    x, w, gy = random_case(M, K, N)
    xd, wd, gd = x.double(), w.double(), gy.double()
    pre = xd @ wd.T
    bound_y = 2 * (K + 1) * 2.0 ** -24 * (xd.abs() @ wd.abs().T)
    for relu in (False, True):
        y, dx, _ = run_layer(x.numpy(), w.numpy(), gy.numpy(), relu)
        want = torch.relu(pre) if relu else pre
        err = (y.cpu().double() - want).abs()
        print("K %d N %d relu %s: forward max err / bound = %.3g" % (K, N, relu, float((err / bound_y).max())))
        assert bool((err <= bound_y).all())
        gm = gd * (pre > 0) if relu else gd
        clear = (pre.abs() > bound_y).all(1) if relu else torch.ones(M, dtype=torch.bool)
        assert int(clear.sum()) > 0.9 * M
        bound_dx = 2 * (N + 1) * 2.0 ** -24 * (gm.abs() @ wd.abs())
        err = (dx.cpu().double() - gm @ wd).abs()
        print("K %d N %d relu %s: data gradient max err / bound = %.3g, rows compared %d" % (K, N, relu, float((err / bound_dx.clamp_min(1e-300))[clear].max()),
                                                                                          int(clear.sum())))
        assert bool((err <= bound_dx)[clear].all())


# ---- MLP ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", E.MLP_BATCHES)
def test_mlp_equals_the_integer_model(M):
    """linear.MLP, the operator path other suites use as their yardstick: every activation, the input gradient and every weight gradient"""
    from lzzx_nerf_amd.linear import MLP
    x, ws, g = E.mlp_case(M)
    ref = E.mlp_reference(x, ws, g)
    mlp = MLP(**E.MLP_DIMS).cuda()
    with torch.no_grad():
        for lin, w in zip(mlp.net, ws):
            lin.weight.copy_(dev(w))
    xg = dev(x).requires_grad_(True)
    out = mlp(xg)
    out.backward(dev(g))
    # the intermediate activations, layer by layer through the same operator (MLP.forward keeps none)
    from lzzx_nerf_amd.linear import lz_linear
    acts = []
    with torch.no_grad():
        h = dev(x)
        for l, lin in enumerate(mlp.net):
            h = lz_linear(h, lin.weight, l != len(ws) - 1)
            acts.append(h)
    for l, a in enumerate(acts):
        assert same_bits(a, ref["acts"][l + 1]), "activation %d " % l + where_off(a, ref["acts"][l + 1])
    assert same_bits(out.detach(), ref["acts"][-1]), where_off(out.detach(), ref["acts"][-1])
    assert same_bits(xg.grad, ref["dx"]), "dx " + where_off(xg.grad, ref["dx"])
    for l, lin in enumerate(mlp.net):
        assert same_bits(lin.weight.grad, ref["dws"][l]), "dW %d " % l + where_off(lin.weight.grad, ref["dws"][l])
