"""LPIPS v0.1 on the AlexNet trunk (lpips.LPIPS(net='alex'), as called at nerf_triplane/TrainerUtil.py:283,309) on the
kernels of csrc/lz_lpips.hip, as an autograd Function:

    FusedLPIPS(state_dict, device="cuda")(pred, target) -> [P]      pred, target [P,3,H,W] f32 in [-1, 1], 31 <= H, W <= 256

The operation is defined in DESIGN 4.14.  The gradient flows to `pred` only; `target` and all weights are constants.  Nine launches
forward and eight backward, no host synchronisation (the upstream gradient is read on the device), no float atomics: the same inputs
give the same bits, and equal images give exactly 0.

Arithmetic: f32 throughout.  The reference evaluates this term under autocast (f16 convolutions); f16 or autocast arithmetic for the trunk
is out of scope here, and under autocast the inputs are cast to f32.

Weights: `state_dict` has the key layout of lpips.LPIPS(net='alex').state_dict() -- net.slice1.0.{weight,bias}, net.slice2.3.*,
net.slice3.6.*, net.slice4.8.*, net.slice5.10.*, lin{0..4}.model.1.weight [1,C,1,1] (or the duplicate keys lins.{i}.model.1.weight), and
optionally scaling_layer.shift / scaling_layer.scale [1,3,1,1].  The `lpips` package is not available where this project is built, so this
layout is stated from the published package and has not been checked against it.  synthetic.lpips_alex_state(seed) gives seeded stand-in
weights of the same layout for the tests and benchmarks."""
import ctypes as C

import numpy as np
import torch
from torch.autograd import Function

from . import _lib
from ._util import call, ptr, stream

CONV_KEYS = ("net.slice1.0", "net.slice2.3", "net.slice3.6", "net.slice4.8", "net.slice5.10")
CONV_SHAPES = ((64, 3, 11, 11), (192, 64, 5, 5), (384, 192, 3, 3), (256, 384, 3, 3), (256, 256, 3, 3))
SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)
MIN_SIZE, MAX_SIZE = 31, 256


def _array(state_dict, key, shape):
    """state_dict[key] as a contiguous f32 numpy array of `shape` (ValueError naming the key otherwise)"""
    if key not in state_dict:
        raise ValueError(f"LPIPS state dict: missing key '{key}'")
    v = state_dict[key]
    a = v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
    if tuple(a.shape) != tuple(shape):
        raise ValueError(f"LPIPS state dict: '{key}' has shape {tuple(a.shape)}, expected {tuple(shape)}")
    return np.ascontiguousarray(a, dtype=np.float32)


def read_state(state_dict):
    """-> (conv_w [5], conv_b [5], lin_w [5] flattened to [C], shift [3], scale [3]) as f32 numpy arrays"""
    conv_w, conv_b, lin_w = [], [], []
    for i, (key, shape) in enumerate(zip(CONV_KEYS, CONV_SHAPES)):
        conv_w.append(_array(state_dict, key + ".weight", shape))
        conv_b.append(_array(state_dict, key + ".bias", shape[:1]))
        lin_key = f"lin{i}.model.1.weight"
        if lin_key not in state_dict and f"lins.{i}.model.1.weight" in state_dict:
            lin_key = f"lins.{i}.model.1.weight"
        lin = _array(state_dict, lin_key, (1, shape[0], 1, 1)).reshape(-1)
        if not (lin >= 0).all():
            raise ValueError(f"LPIPS state dict: '{lin_key}' has negative weights (the lin layers are non-negative)")
        lin_w.append(np.ascontiguousarray(lin))
    shift = _array(state_dict, "scaling_layer.shift", (1, 3, 1, 1)).reshape(3) if "scaling_layer.shift" in state_dict else np.array(SHIFT, np.float32)
    scale = _array(state_dict, "scaling_layer.scale", (1, 3, 1, 1)).reshape(3) if "scaling_layer.scale" in state_dict else np.array(SCALE, np.float32)
    if not (scale != 0).all():
        raise ValueError("LPIPS state dict: 'scaling_layer.scale' holds a zero")
    return conv_w, conv_b, lin_w, shift, scale


def pack_weights(state_dict):
    """the packed weight image of lz_lpips_pack (include/lzzx_nerf_hip.h) as a CPU f32 tensor; host code, needs no GPU"""
    conv_w, conv_b, lin_w, shift, scale = read_state(state_dict)
    w = _lib.LpipsWeights()
    for i in range(5):
        w.conv_w[i], w.conv_b[i], w.lin_w[i] = conv_w[i].ctypes.data, conv_b[i].ctypes.data, lin_w[i].ctypes.data
    for c in range(3):
        w.shift[c], w.scale[c] = float(shift[c]), float(scale[c])
    n = _lib.load().lz_lpips_packed_floats()
    packed = torch.empty(n, dtype=torch.float32)
    call("lz_lpips_pack", C.byref(w), C.c_void_p(packed.data_ptr()), n)
    return packed


def check_shape(P, H, W):
    if P < 1:
        raise ValueError(f"LPIPS: {P} patches")
    if not (MIN_SIZE <= H <= MAX_SIZE and MIN_SIZE <= W <= MAX_SIZE):
        raise ValueError(f"LPIPS: {H} x {W} image; the trunk needs {MIN_SIZE} <= H, W <= {MAX_SIZE}")


class _LPIPS(Function):
    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, pred, target, packed):
        P, _, H, W = pred.shape
        pred, target = pred.contiguous(), target.contiguous()
        nbytes = _lib.load().lz_lpips_workspace_bytes(P, H, W)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=pred.device)     # features now, gradients in the backward: lives with the graph
        value = torch.empty(P, device=pred.device)
        call("lz_lpips_forward", ptr(packed), ptr(pred), ptr(target), P, H, W, ptr(ws), ptr(value), stream())
        ctx.save_for_backward(packed, ws)
        ctx.shape = (P, H, W)
        return value

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, g_value):
        packed, ws = ctx.saved_tensors
        P, H, W = ctx.shape
        g = g_value.float().contiguous()
        g_pred = torch.empty(P, 3, H, W, device=g.device)
        call("lz_lpips_backward", ptr(packed), ptr(g), P, H, W, ptr(ws), ptr(g_pred), stream())
        return g_pred, None, None


class FusedLPIPS:
    """LPIPS-AlexNet on fused kernels; see the module docstring.  Weights are read, checked and packed once, here."""
    FORWARD_LAUNCHES, BACKWARD_LAUNCHES = 9, 8

    def __init__(self, state_dict, device="cuda"):
        self.device = torch.device(device)
        self.packed = pack_weights(state_dict).to(self.device)

    def __call__(self, pred, target):
        for name, t in (("pred", pred), ("target", target)):
            if not isinstance(t, torch.Tensor) or t.dim() != 4 or t.shape[1] != 3:
                raise ValueError(f"LPIPS: {name} must be a [P,3,H,W] tensor")
            if not t.is_cuda:
                raise ValueError(f"LPIPS: {name} must be a CUDA tensor")
        if pred.shape != target.shape:
            raise ValueError(f"LPIPS: pred {tuple(pred.shape)} and target {tuple(target.shape)} differ")
        if target.requires_grad:
            raise ValueError("LPIPS: target must not require grad (the gradient flows to pred only)")
        check_shape(pred.shape[0], pred.shape[2], pred.shape[3])
        return _LPIPS.apply(pred, target, self.packed)
