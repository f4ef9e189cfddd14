"""Small helpers shared by the operator wrappers: raw pointers, current HIP stream, argument checks."""
import ctypes as C

import torch

from . import _lib


def ptr(t):
    """device pointer of a tensor (None -> NULL)"""
    if t is None:
        return None
    return C.c_void_p(t.data_ptr())


def stream():
    """hipStream_t of torch's current stream: kernels launch where the caller's torch ops do
    (the reference launches on the legacy default stream)."""
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def require_cuda(**tensors):
    """the reference's CHECK_CUDA / CHECK_CONTIGUOUS (gridencoder.cu:15-18) -> RuntimeError"""
    for name, t in tensors.items():
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError(f"{name} must be a CUDA tensor")
        if not t.is_contiguous():
            raise RuntimeError(f"{name} must be a contiguous tensor")


_WS = {}


def workspace(tag, device, nbytes, zero=False, grow=False):
    """a cached byte tensor per (tag, device): kernel scratch that lives across calls (zero: cleared once, when allocated).
    grow: a request larger than the cached tensor replaces it (the old one is freed in stream order by torch's allocator).
    Launches on it are ordered by the stream; two streams at once would share it (not supported)"""
    key = (tag, device.type, device.index)
    ws = _WS.get(key)
    if ws is None or (grow and ws.numel() < nbytes):
        ws = _WS[key] = (torch.zeros if zero else torch.empty)(nbytes, dtype=torch.uint8, device=device)
    return ws


def as_f32(t):
    """an upstream gradient as the kernels read it: contiguous f32 (None stays None)"""
    return None if t is None else t.float().contiguous()


def map01(x, bound):
    """[-bound, bound] -> [0, 1], GridEncoder.forward's first line (grid.py:143), for a tensor `x` and a Python number `bound`: THE mapping on
    the Python side.  The expression is the reference's own and stays differentiable; on the device torch evaluates a division by a
    host scalar as the add followed by a multiplication with the scalar's f32 reciprocal (measured:
    tests/test_gpu_bound_mapping.py::test_device_division_by_scalar_is_a_reciprocal_multiply), which csrc/lz_common.h: lz_map01 and
    oracle.oracle.map01 restate.  Never divide by a tensor here: that is a true division, other bits when 2 bound is no power of two."""
    return (x + bound) / (2 * bound)


def call(name, *args):
    _lib.call(name, *args)
