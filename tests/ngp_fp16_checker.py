"""CPU checker of the hash-grid NeRF in the reference's autocast arithmetic (lzzx_nerf_amd/ngp.py precision="f16", csrc/lz_ngp.hip:
lz_k_ngp_head16) -- test infrastructure, not a conftest.  It restates the CUDA autocast policy's rounding sequence for
synthetic.GenericHashgridNeRF.net's composition and is pinned to the reference's own modules by tests/test_golden_ngp_autocast.py
(tests/golden/reference_ngp_autocast.npz):

  1. features: half (grid.py:38-39 gathers from a half copy of the table)
  2. s0 = half(f32 dot) of sigma_net.0, ReLU in half
  3. h = half(f32 dot) of sigma_net.1, 16 values
  4. sigma = exp in f32 of float(h[:, 0])            (exp is on CUDA autocast's fp32 list)
  5. SH(4) in f32; cat([SH, h[:, 1:]]) promotes to f32, colour_net.0's cast rounds SH to half
  6. c0 = half(f32 dot), ReLU in half; c1 = half(f32 dot)
  7. rgb = half(sigmoid(c1))                         (sigmoid runs in the input type)

The f32 dot is numpy's f32 matmul (oracle.head._lin16): the summation order inside a half GEMM is the library's, so agreement with the
kernel is to half rounding, not to the bit; exp / sigmoid are the checker's deterministic lz_expf / lz_sigmoidf."""
import numpy as np

from oracle import oracle as O
from oracle.head import _lin16

F16, F32 = np.float16, np.float32
LAYERS = ("sigma_net.net.0", "sigma_net.net.1", "color_net.net.0", "color_net.net.1")


def features(emb, offsets, per_level_scale, xyz, bound, base_resolution=16):
    """GridEncoder.forward (grid.py:139-154) on a half copy of the table -> half features [M, 32]"""
    x01 = O.map01(xyz, bound)
    feats, _ = O.grid_encode_forward(x01, np.asarray(emb).astype(F16), offsets, per_level_scale, base_resolution)
    return feats


def head(W, feats16, dirs, trace=None):
    """W: dict of the four weights under the reference's module names (LAYERS; f32 [out, in]); feats16 [M, 32] half; dirs [M, 3]
    -> (sigma f32 [M], rgb half [M, 3]); `trace` (dict): the half output of every Linear, under its module name"""
    tr = trace if trace is not None else {}
    relu = lambda a: np.maximum(a, F16(0))
    s0 = _lin16(np.asarray(feats16, F16), W["sigma_net.net.0"])
    tr["sigma_net.net.0"] = s0
    h = _lin16(relu(s0), W["sigma_net.net.1"])
    tr["sigma_net.net.1"] = h
    sigma = O.unary("exp", np.ascontiguousarray(h[:, 0].astype(F32)))
    sh, _ = O.sh_encode_forward(np.ascontiguousarray(dirs, F32), 4)
    x = np.concatenate([sh, h[:, 1:].astype(F32)], 1)          # cat promotes to f32
    c0 = _lin16(x.astype(F16), W["color_net.net.0"])             # colour_net.0's cast: SH rounded to half, geometry exact
    tr["color_net.net.0"] = c0
    c1 = _lin16(relu(c0), W["color_net.net.1"])
    tr["color_net.net.1"] = c1
    rgb = O.unary("sigmoid", np.ascontiguousarray(c1.astype(F32))).astype(F16)
    return sigma, rgb


def network(W, emb, offsets, per_level_scale, base_resolution=16):
    """(xyzs, dirs, bound) -> (sigma f32, rgb half)"""
    def net(xyzs, dirs, bound, trace=None):
        return head(W, features(emb, offsets, per_level_scale, xyzs, bound, base_resolution), dirs, trace)
    return net


def half_ulps(a, b):
    """distance of two half arrays in units in the last place (ordered bit patterns)"""
    def key(v):
        i = np.asarray(v, F16).view(np.int16).astype(np.int32)
        return np.where(i < 0, -32768 - i, i)
    return np.abs(key(a) - key(b))
