"""Seeded inputs on which every product and every partial sum of the free-order training sums is exactly representable in f32, so that
any summation order gives the same bits and a test can ask for equality instead of a tolerance.  Shared by tests/test_exact_inputs_host.py
(which proves the premises below on the CPU, with integers and the checker alone) and the GPU modules test_gpu_exact_linear.py and
test_gpu_exact_grid_scatter.py (which then hold the kernels to `array_equal`).

Premises the generators promise:
  linear  x, w, gy are integer-valued f32; for y = x w^T, relu(y), dx = (gy . [y > 0]) w and dW = (gy . [y > 0])^T x the sum of the
          ABSOLUTE values of the terms of every element stays below 2^24, so every partial sum in any order is an integer below 2^24.
  mlp     the same at every layer of a bias-free ReLU MLP with weights in {-1, 0, 1}.
  grid    per_level_scale == 2 exactly, coordinates k / 2^q, integer gradients in [-8, 8]: every term w g is a multiple of 2^-(D q) and
          the per-entry sum of |w g| stays below 2^24 2^-(D q).
  planes  the same for the three planes of the triplane encoder at bound 1 and 2 (q = 5).
"""
import functools

import numpy as np

LIMIT = 1 << 24          # integers below this magnitude are exact in f32

# ---------------------------------------------------------------------------------------------------------------------------------
# linear
# ---------------------------------------------------------------------------------------------------------------------------------
LINEAR_SHAPES = [(36, 64), (69, 64), (64, 65), (1, 5), (128, 7), (116, 32), (96, 64)]     # (K, N); (116, 32) splits the column blocks of dW
LINEAR_BATCHES = [1, 15, 16, 17, 63, 5003]
M_PAST_FORWARD_CAP = 131072 + 16 * 4 + 5          # 2048 workgroups x 4 waves x 16 rows, one more round of waves and a ragged tail
M_PAST_GRAD_W_CAP = 786432 + 16 * 32 + 5          # 1536 workgroups x 4 waves x 8 groups x 16 rows, likewise


def _ints(rng, shape, amp, zero_share=0.0):
    a = rng.integers(-amp, amp + 1, shape)
    if zero_share:
        a[rng.random(shape) < zero_share] = 0
    return a


def linear_case(M, K, N, seed=0, amp=None):
    """integer-valued f32 x [M, K], w [N, K], gy [M, N].  A quarter of x is zero and every 16th row entirely, the last row of w is the
    negated first and (N > 2) the third row is zero: y == 0 is common, y > 0 and y < 0 are both frequent.  amp: largest magnitude
    (default 3; 2 at the batch sizes past the workgroup caps, where 4 M has to stay below 2^24)."""
    if amp is None:
        amp = 3 if M <= 5003 else 2
    rng = np.random.default_rng([seed, M, K, N])
    x = _ints(rng, (M, K), amp, 0.25)
    x[5::16] = 0
    w = _ints(rng, (N, K), amp)
    if N > 1:
        w[N - 1] = -w[0]
    if N > 2:
        w[2] = 0
    gy = _ints(rng, (M, N), amp)
    return x.astype(np.float32), w.astype(np.float32), gy.astype(np.float32)


def _exact_matmul(a, b):
    """a @ b for integer-valued arrays through float64 (exact below 2^53), back as int64"""
    r = np.asarray(a, np.float64) @ np.asarray(b, np.float64)
    assert float(np.abs(r).max(initial=0.0)) < 2.0 ** 53
    return np.rint(r).astype(np.int64)


def linear_reference(x, w, gy, relu):
    """the integer model of lz_linear forward / backward: dict(pre, y, dx, dw) as int64.  With relu the gradient passes where y > 0 only
    (0 at y == 0)."""
    pre = _exact_matmul(x, np.asarray(w).T)
    y = np.maximum(pre, 0) if relu else pre
    gm = np.rint(gy).astype(np.int64)
    if relu:
        gm = gm * (pre > 0)
    return dict(pre=pre, y=y, gm=gm, dx=_exact_matmul(gm, w), dw=_exact_matmul(gm.T, x))


def linear_budget(x, w, gy, relu):
    """largest sum of |term| over the elements of y, dx and dW: every partial sum of every element is below this"""
    r = linear_reference(x, w, gy, relu)
    ax, aw, agm = np.abs(x), np.abs(w), np.abs(r["gm"])
    return dict(y=int(_exact_matmul(ax, aw.T).max()), dx=int(_exact_matmul(agm, aw).max()), dw=int(_exact_matmul(agm.T, ax).max()))


def as_f32(a):
    """an int64 result as the f32 the kernel has to produce: exact, zeros are +0"""
    assert int(np.abs(a).max(initial=0)) < LIMIT
    return a.astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------------------
# MLP chain: weights in {-1, 0, 1}
# ---------------------------------------------------------------------------------------------------------------------------------
MLP_DIMS = dict(dim_in=36, dim_out=4, dim_hidden=64, num_layers=3)
MLP_BATCHES = [5003, M_PAST_FORWARD_CAP]
MLP_DENSITY = 0.125      # share of nonzero weights


def mlp_case(M, seed=0):
    """x [M, dim_in] in [-2, 2], weights [(out, in)] in {-1, 0, 1} with MLP_DENSITY nonzeros, upstream gradient [M, dim_out] in [-2, 2]"""
    d = MLP_DIMS
    rng = np.random.default_rng([seed, M, 77])
    x = _ints(rng, (M, d["dim_in"]), 2, 0.25).astype(np.float32)
    ws = []
    for l in range(d["num_layers"]):
        fan_in = d["dim_in"] if l == 0 else d["dim_hidden"]
        fan_out = d["dim_out"] if l == d["num_layers"] - 1 else d["dim_hidden"]
        w = rng.integers(0, 2, (fan_out, fan_in)) * 2 - 1
        w[rng.random((fan_out, fan_in)) >= MLP_DENSITY] = 0
        ws.append(w.astype(np.float32))
    g = _ints(rng, (M, d["dim_out"]), 2).astype(np.float32)
    return x, ws, g


def mlp_reference(x, ws, g):
    """integer model of MLP.forward / backward (ReLU after every layer but the last).  Returns dict(acts: input of every layer and the
    output, dx, dws, budget: the largest sum of |term| over everything computed)"""
    acts, pres = [np.rint(x).astype(np.int64)], []
    budget = 0
    for l, w in enumerate(ws):
        pre = _exact_matmul(acts[-1], w.T)
        budget = max(budget, int(_exact_matmul(np.abs(acts[-1]), np.abs(w).T).max()))
        pres.append(pre)
        acts.append(np.maximum(pre, 0) if l != len(ws) - 1 else pre)
    gcur = np.rint(g).astype(np.int64)
    dws = [None] * len(ws)
    for l in reversed(range(len(ws))):
        if l != len(ws) - 1:
            gcur = gcur * (pres[l] > 0)
        dws[l] = _exact_matmul(gcur.T, acts[l])
        budget = max(budget, int(_exact_matmul(np.abs(gcur).T, np.abs(acts[l])).max()), int(_exact_matmul(np.abs(gcur), np.abs(ws[l])).max()))
        gcur = _exact_matmul(gcur, ws[l])
    return dict(acts=acts, dx=gcur, dws=dws, budget=budget)


# ---------------------------------------------------------------------------------------------------------------------------------
# grid encoder
# ---------------------------------------------------------------------------------------------------------------------------------
# D, L, C, H, log2 T, gridtype, q.  desired_resolution = H 2^(L-1) makes per_level_scale 2 exactly; the finest scale H 2^(L-1) - 1 times
# k <= 2^q stays below 2^24, so pos = x scale + 0.5 is exact as well
GRID_CASES = {
    "D2C1T14": (2, 6, 1, 64, 14, "hash", 7),         # one triplane plane's shape: every level fits the LDS accumulator
    "D3C2T13": (3, 8, 2, 16, 13, "hash", 5),         # 8192 x 2 accumulators of 8 bytes = 128 KB exactly
    "D2C2T12tiled": (2, 6, 2, 64, 12, "tiled", 7),
    "D3C2T16": (3, 8, 2, 16, 16, "hash", 5),         # fine levels do not fit: global atomics inside the level-resident kernel
    "D3C4T12": (3, 4, 4, 8, 12, "hash", 5),          # C = 4: the plain kernel at every batch size
}
# 70001 samples on tables of 2^13 and 2^12 entries would pile more than 2^24 units on the busiest entries of the fine levels (dyadic
# points fall on few cells there): those two cases stop at 20001, still five ragged chunks of the level-resident kernel
GRID_BATCHES = {"D2C1T14": [257, 4099, 70001], "D3C2T13": [257, 4099, 20001], "D2C2T12tiled": [257, 4099, 20001], "D3C2T16": [4099, 70001],
                "D3C4T12": [4099]}


def grid_kwargs(name):
    D, L, C, H, T, gt, _ = GRID_CASES[name]
    return dict(input_dim=D, num_levels=L, level_dim=C, base_resolution=H, log2_hashmap_size=T, desired_resolution=H * 2 ** (L - 1), gridtype=gt)


def grid_unit(name):
    """the unit every table-gradient value is a multiple of: 2^-(D q)"""
    D, q = GRID_CASES[name][0], GRID_CASES[name][6]
    return 2.0 ** -(D * q)


@functools.lru_cache(maxsize=None)
def grid_inputs(name, B, q=None):
    """x [B, D] = k / 2^q in [0, 1] (row 0 all 0, row 1 all 1, rows 10 .. 49 equal when the batch has them), g [B, L C] integers in
    [-8, 8].  Read-only: shared between tests.  q overrides the case's own (the host test shows what that breaks)."""
    D, L, C = GRID_CASES[name][:3]
    q = GRID_CASES[name][6] if q is None else q
    rng = np.random.default_rng([B, D, L, C, 3])
    k = rng.integers(0, (1 << q) + 1, (B, D))
    k[0] = 0
    if B > 1:
        k[1] = 1 << q
    if B >= 64:
        k[10:50] = k[10]
    x = (k / float(1 << q)).astype(np.float32)
    g = rng.integers(-8, 9, (B, L * C)).astype(np.float32)
    x.setflags(write=False)
    g.setflags(write=False)
    return x, g


# ---------------------------------------------------------------------------------------------------------------------------------
# triplane encoder: three D = 2, C = 1 planes
# ---------------------------------------------------------------------------------------------------------------------------------
# both rely on GridEncoder's default per_level_scale (asserted to be 2.0 by the host test): resolutions 16 .. 128
PLANE_CONFIGS = {
    "small": dict(num_levels=4, base_resolution=16, log2_hashmap_size=8),      # all four levels hashed
    "mixed": dict(num_levels=4, base_resolution=16, log2_hashmap_size=10),     # a dense level next to hashed ones
}
PLANE_Q = 5
PLANE_UNIT = 2.0 ** -(2 * PLANE_Q)
PLANE_BATCHES = [65, 1000, 16383, 16384, 70001]      # 16384: the backward changes from global atomics to the accumulator in LDS
PLANE_BOUNDS = [1, 2]                                # 1.5 is left out: its reciprocal is inexact (tests/test_gpu_bound_mapping.py)
PLANE_COLUMNS = ((0, 1), (1, 2), (0, 2))


@functools.lru_cache(maxsize=None)
def plane_inputs(B, bound):
    """xyz [B, 3] dyadic in [-bound, bound] (unit coordinates k / 2^5), with the special rows of test_gpu_triplane_encoder.points(): the
    box's corners, one row per coordinate outside the box, the last row on the surface; g [B, 3 L] integers in [-8, 8] for L = 4"""
    rng = np.random.default_rng([B, int(bound), 5])
    b = float(bound)
    k = rng.integers(0, (1 << PLANE_Q) + 1, (B, 3))
    x = ((2.0 * k / (1 << PLANE_Q) - 1.0) * b).astype(np.float32)
    if B >= 64:
        x[10:50] = x[10]
    if B >= 8:
        x[0] = [b, b, b]
        x[1] = [-b, -b, -b]
        x[2] = [b, -b, 0.25 * b]
        x[3, 0] = 1.25 * b
        x[4, 1] = -1.5 * b
        x[5, 2] = b * (1 + 2.0 ** -20)
        x[B - 1] = [-b, 0.5 * b, b]
    g = rng.integers(-8, 9, (B, 3 * 4)).astype(np.float32)
    x.setflags(write=False)
    g.setflags(write=False)
    return x, g
