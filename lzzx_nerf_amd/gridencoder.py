"""Multi-resolution hash / tiled grid encoder -- operator API of the reference's `gridencoder` package
(/root/reference/gridencoder/grid.py:19-154) on top of the gfx950 kernels (csrc/lz_grid.hip).

Same names, arguments, defaults, state-dict keys (`embeddings`, `offsets`) and error behaviour.  Differences
that are invisible to callers: the kernel writes [B, L*C] directly (no permute/reshape copy, grid.py:52) and
reads the gradient in that layout (no permute copy, grid.py:70); kernels run on torch's current stream.
"""
import numpy as np
import torch
import torch.nn as nn
from torch.autograd import Function

from . import _lib
from ._util import call, map01, ptr, require_cuda, stream, workspace

_gridtype_to_id = {"hash": 0, "tiled": 1}

# How the table gradient is summed: "atomic" = float atomics (the reference's way: repeatable only up to summation order), "ordered" =
# lz_grid_encode_backward_ordered: no float atomics, every entry summed in the CPU checker's (sample, corner) order, the same bits on
# every call (f32 tables, D 2 / 3), "fixed" = lz_grid_encode_backward_fixed: every term quantised with one power-of-two scale per level and
# summed as 64-bit integers, one rounding at the end -- the same bits on every call AND under any order of the rows (f32 tables, D 2 / 3,
# C 1 / 2).
_TABLE_GRADS = ("atomic", "ordered", "fixed")
_TABLE_GRAD = "atomic"
ORDERED_WORKSPACE_CAP = 256 << 20   # bytes; a batch whose level needs more is processed in sample ranges (same bits)


def set_table_grad(mode):
    """module default for the table gradient of grid_encode / GridEncoder, FusedHashgridTrainNeRF(table_grad=None) and the f32 training
    head's per-plane scatter; returns the previous one"""
    global _TABLE_GRAD
    if mode not in _TABLE_GRADS:
        raise ValueError("table_grad must be one of %s, got %r" % (_TABLE_GRADS, mode))
    prev, _TABLE_GRAD = _TABLE_GRAD, mode
    return prev


def table_grad():
    return _TABLE_GRAD


def grid_backward_ordered(grad, inputs, embeddings, offsets, grad_embeddings, B, D, C, L, S, H, dy_dx, grad_inputs, gridtype, align_corners,
                          grad_layout, workspace_bytes=None):
    """lz_grid_encode_backward_ordered on a per-device cached workspace of min(what one level of B samples needs, ORDERED_WORKSPACE_CAP)
    bytes (the cache keeps the largest size asked for so far); workspace_bytes overrides the size"""
    need = int(_lib.load().lz_grid_ordered_workspace(B, D))
    if need == 0:
        raise RuntimeError("the ordered table gradient is built for input_dim 2 and 3 (got %d)" % D)
    nbytes = min(need, ORDERED_WORKSPACE_CAP) if workspace_bytes is None else int(workspace_bytes)
    ws = workspace("grid_ordered", grad_embeddings.device, nbytes, grow=True)
    call("lz_grid_encode_backward_ordered", ptr(grad), ptr(inputs), ptr(embeddings), ptr(offsets), ptr(grad_embeddings), B, D, C, L, S, H,
         ptr(dy_dx), ptr(grad_inputs), int(gridtype), int(bool(align_corners)), int(embeddings.dtype == torch.float16), grad_layout,
         ptr(ws), nbytes & 0xFFFFFFFF, nbytes >> 32, stream())


def _check_fixed(D, C, dtype):
    """what lz_grid_encode_backward_fixed does not serve, refused with the modes that do"""
    if dtype != torch.float32:
        raise RuntimeError("set_table_grad('fixed') sums f32 tables only; half tables (autocast with an even level_dim) take the atomic "
                           "path: set_table_grad('atomic') or leave autocast")
    if D not in (2, 3):
        raise RuntimeError("set_table_grad('fixed') is built for input_dim 2 and 3 (got %d): set_table_grad('atomic') serves every input_dim" % D)
    if C not in (1, 2):
        raise RuntimeError("set_table_grad('fixed') is built for level_dim 1 and 2 (got %d): set_table_grad('atomic') or 'ordered' serve "
                           "level_dim 4 and 8" % C)


def grid_backward_fixed(grad, inputs, embeddings, offsets, grad_embeddings, B, D, C, L, S, H, dy_dx, grad_inputs, gridtype, align_corners,
                        grad_layout, grad_row_stride=0, workspace_bytes=None):
    """lz_grid_encode_backward_fixed on a per-device cached workspace of lz_grid_fixed_workspace(entries of the table, C) bytes (the cache
    keeps the largest size asked for so far; the call clears what it uses); workspace_bytes overrides the size.  grad may be a tensor or,
    for a block of columns of a wider matrix, a device address (with grad_row_stride)"""
    _check_fixed(D, C, embeddings.dtype)
    need = int(_lib.load().lz_grid_fixed_workspace(grad_embeddings.shape[0], C))
    nbytes = need if workspace_bytes is None else int(workspace_bytes)
    ws = workspace("grid_fixed", grad_embeddings.device, nbytes, grow=True)
    call("lz_grid_encode_backward_fixed", grad if isinstance(grad, int) else ptr(grad), ptr(inputs), ptr(embeddings), ptr(offsets),
         ptr(grad_embeddings), B, D, C, L, S, H, ptr(dy_dx), ptr(grad_inputs), int(gridtype), int(bool(align_corners)), 0, grad_layout, ptr(ws),
         nbytes & 0xFFFFFFFF, nbytes >> 32, int(grad_row_stride), stream())


def _check_dc(D, C):
    # the reference throws std::runtime_error from the dispatch switch (gridencoder.cu:354,372)
    if C not in (1, 2, 4, 8):
        raise RuntimeError("GridEncoding: C must be 1, 2, 4, or 8.")
    if D not in (1, 2, 3, 4, 5):
        raise RuntimeError("GridEncoding: D must be 1, 2, 3, 4, or 5")


_LEVEL_SIZE_CACHE = {}


def _max_level_entries(offsets):
    """largest per-level table (entries) of an `offsets` tensor; one tiny device->host copy the first time a given
    offsets buffer is seen, cached afterwards (offsets are constants of a GridEncoder)"""
    key = (offsets.data_ptr(), offsets._version, offsets.numel())
    v = _LEVEL_SIZE_CACHE.get(key)
    if v is None:
        o = offsets.detach().cpu().numpy().astype(np.int64)
        v = int(np.max(o[1:] - o[:-1])) if o.size > 1 else 0
        if len(_LEVEL_SIZE_CACHE) > 256:
            _LEVEL_SIZE_CACHE.clear()
        _LEVEL_SIZE_CACHE[key] = v
    return v


class _grid_encode(Function):
    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda")
    def forward(ctx, inputs, embeddings, offsets, per_level_scale, base_resolution, calc_grad_inputs=False, gridtype=0,
                align_corners=False):
        # inputs: [B, D] float in [0, 1]; embeddings: [sO, C]; offsets: [L + 1] int32; returns [B, L * C]
        inputs = inputs.float().contiguous()
        B, D = inputs.shape
        L = offsets.shape[0] - 1
        C = embeddings.shape[1]
        S = float(np.float32(np.log2(per_level_scale)))  # narrowed to float at the FFI, gridencoder.h:12
        H = int(base_resolution)
        _check_dc(D, C)

        # half tables only under autocast and only when C is even (grid.py:38-39)
        if torch.is_autocast_enabled() and C % 2 == 0:
            embeddings = embeddings.to(torch.half)
        embeddings = embeddings.contiguous()
        if embeddings.dtype not in (torch.float32, torch.float16):
            raise RuntimeError("embeddings must be a float32 or float16 tensor")
        if offsets.dtype != torch.int32:
            raise RuntimeError("offsets must be an int tensor")
        require_cuda(inputs=inputs, embeddings=embeddings, offsets=offsets)

        outputs = torch.empty(B, L * C, device=inputs.device, dtype=embeddings.dtype)
        dy_dx = torch.empty(B, L * D * C, device=inputs.device, dtype=embeddings.dtype) if calc_grad_inputs else None
        # large batches over small tables (the triplane: <= 16384 entries per level): level-resident LDS kernel
        layout = 1
        small = D <= 3 and C <= 2 and _max_level_entries(offsets) * C * embeddings.element_size() <= 65536
        if B >= 32768 and not calc_grad_inputs and small:
            layout = 2
        call("lz_grid_encode_forward", ptr(inputs), ptr(embeddings), ptr(offsets), ptr(outputs), B, D, C, L, S, H, ptr(dy_dx),
             int(gridtype), int(bool(align_corners)), int(embeddings.dtype == torch.float16), layout, stream())

        ctx.save_for_backward(inputs, embeddings, offsets, dy_dx)
        ctx.dims = [B, D, C, L, S, H, gridtype]
        ctx.small_levels = small
        ctx.align_corners = align_corners
        return outputs

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, grad):
        inputs, embeddings, offsets, dy_dx = ctx.saved_tensors
        B, D, C, L, S, H, gridtype = ctx.dims
        grad = grad.contiguous()  # [B, L * C], consumed in place of the reference's [L, B, C] copy
        if grad.dtype != embeddings.dtype:
            grad = grad.to(embeddings.dtype)
        grad_embeddings = torch.zeros_like(embeddings)
        # small f32 tables + large batches: per-level accumulation in LDS instead of scattered global atomics
        glayout = 2 if (ctx.small_levels and B >= 16384 and embeddings.dtype == torch.float32) else 1
        grad_inputs = torch.zeros_like(inputs, dtype=embeddings.dtype) if dy_dx is not None else None
        if _TABLE_GRAD == "ordered":
            if embeddings.dtype != torch.float32:
                raise RuntimeError("set_table_grad('ordered') sums f32 tables only; half tables (autocast with an even level_dim) take the "
                                   "atomic path: set_table_grad('atomic') or leave autocast")
            grid_backward_ordered(grad, inputs, embeddings, offsets, grad_embeddings, B, D, C, L, S, H, dy_dx, grad_inputs, gridtype,
                                  ctx.align_corners, 1)
            return grad_inputs, grad_embeddings, None, None, None, None, None, None
        if _TABLE_GRAD == "fixed":
            _check_fixed(D, C, embeddings.dtype)
            grid_backward_fixed(grad, inputs, embeddings, offsets, grad_embeddings, B, D, C, L, S, H, dy_dx, grad_inputs, gridtype,
                                ctx.align_corners, 1)
            return grad_inputs, grad_embeddings, None, None, None, None, None, None
        call("lz_grid_encode_backward", ptr(grad), ptr(inputs), ptr(embeddings), ptr(offsets), ptr(grad_embeddings), B, D, C, L,
             S, H, ptr(dy_dx), ptr(grad_inputs), int(gridtype), int(bool(ctx.align_corners)),
             int(embeddings.dtype == torch.float16), glayout, stream())
        if dy_dx is not None:
            grad_inputs = grad_inputs.to(inputs.dtype)
        return grad_inputs, grad_embeddings, None, None, None, None, None, None


grid_encode = _grid_encode.apply


def grid_offsets(input_dim, num_levels, per_level_scale, base_resolution, log2_hashmap_size, align_corners=False):
    """Start of every level's table (plus the total) as GridEncoder lays them out (grid.py:108-121): side = ceil(H * s^l) in
    float64 (+1 cell corner unless align_corners), entries = min(2^T, side^D) rounded up to a multiple of 8."""
    cap = 1 << log2_hashmap_size
    starts = [0]
    for level in range(num_levels):
        side = int(np.ceil(base_resolution * per_level_scale ** level)) + (0 if align_corners else 1)
        entries = min(cap, side ** input_dim)
        starts.append(starts[-1] + 8 * ((entries + 7) // 8))
    return starts


class GridEncoder(nn.Module):
    """`[..., D]` points in `[-bound, bound]` -> `[..., L * C]` features.  Parameter `embeddings` [sum of level sizes, C]
    (U(-1e-4, 1e-4)), buffer `offsets` int32 [L + 1]: the reference's state-dict contract (grid.py:91-137)."""

    def __init__(self, input_dim=3, num_levels=16, level_dim=2, per_level_scale=2, base_resolution=16, log2_hashmap_size=19,
                 desired_resolution=None, gridtype="hash", align_corners=False):
        super().__init__()
        if desired_resolution is not None:   # geometric growth that reaches desired_resolution at the last level (grid.py:95-96)
            per_level_scale = np.exp2(np.log2(desired_resolution / base_resolution) / (num_levels - 1))
        hyper = dict(input_dim=input_dim, num_levels=num_levels, level_dim=level_dim, per_level_scale=per_level_scale,
                     log2_hashmap_size=log2_hashmap_size, base_resolution=base_resolution, gridtype=gridtype,
                     align_corners=align_corners)
        for name, value in hyper.items():
            setattr(self, name, value)
        self.gridtype_id = _gridtype_to_id[gridtype]
        self.output_dim = num_levels * level_dim
        self.max_params = 1 << log2_hashmap_size
        starts = grid_offsets(input_dim, num_levels, per_level_scale, base_resolution, log2_hashmap_size, align_corners)
        self.register_buffer("offsets", torch.tensor(starts, dtype=torch.int32))
        self.n_params = starts[-1] * level_dim
        self.embeddings = nn.Parameter(torch.empty(starts[-1], level_dim))
        self.reset_parameters()

    def reset_parameters(self):
        nn.init.uniform_(self.embeddings, -1e-4, 1e-4)

    def extra_repr(self):
        finest = int(round(self.base_resolution * self.per_level_scale ** (self.num_levels - 1)))
        return ("input_dim=%d num_levels=%d level_dim=%d resolution=%d -> %d per_level_scale=%.4f params=%s gridtype=%s align_corners=%s"
                % (self.input_dim, self.num_levels, self.level_dim, self.base_resolution, finest, self.per_level_scale,
                   tuple(self.embeddings.shape), self.gridtype, self.align_corners))

    def __repr__(self):
        return "GridEncoder: " + self.extra_repr()

    def forward(self, inputs, bound=1):
        unit = map01(inputs, bound)                         # [-bound, bound] -> [0, 1] (grid.py:143)
        rows = unit.view(-1, self.input_dim)
        feats = grid_encode(rows, self.embeddings, self.offsets, self.per_level_scale, self.base_resolution, rows.requires_grad,
                            self.gridtype_id, self.align_corners)
        return feats.view(*inputs.shape[:-1], self.output_dim)


class _triplane_encode(Function):
    """xyz [B, 3] -> [B, 3 L] through lz_triplane_encode_forward / _backward: one launch each way, gradients for the three tables and,
    when asked for, xyz.  With level_dim 1 the tables stay f32 under autocast (grid.py:28,38-39), so the output is f32 there as well."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda")
    def forward(ctx, xyz, emb_xy, emb_yz, emb_xz, offsets, L, S, H, bound):
        xyz = xyz.float().contiguous()
        B = xyz.shape[0]
        tables = [e.contiguous() for e in (emb_xy, emb_yz, emb_xz)]
        require_cuda(xyz=xyz, embeddings_xy=tables[0], embeddings_yz=tables[1], embeddings_xz=tables[2], offsets=offsets)
        out = torch.empty(B, 3 * L, device=xyz.device, dtype=torch.float32)
        dy_dx = torch.empty(3, B, L, 2, device=xyz.device, dtype=torch.float32) if ctx.needs_input_grad[0] else None
        call("lz_triplane_encode_forward", ptr(xyz), ptr(tables[0]), ptr(tables[1]), ptr(tables[2]), ptr(offsets), ptr(out), ptr(dy_dx), B, L, S,
             H, bound, stream())
        ctx.save_for_backward(xyz, offsets, dy_dx, *tables)
        ctx.dims = (B, L, S, H, bound)
        return out

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, grad):
        xyz, offsets, dy_dx, *tables = ctx.saved_tensors
        B, L, S, H, bound = ctx.dims
        grad = grad.contiguous()                       # [B, 3 L], read in place by every kernel below: no per-plane slices
        if grad.dtype != torch.float32:
            grad = grad.float()
        want_tables = any(ctx.needs_input_grad[1:4])
        g_tables = [torch.zeros_like(t) for t in tables] if want_tables else [None] * 3
        g_xyz = torch.empty_like(xyz) if dy_dx is not None else None
        per_plane = _TABLE_GRAD if (_TABLE_GRAD != "atomic" and want_tables and B > 0) else None
        if per_plane is not None:
            # the checker's summation order ("ordered", lz_grid_encode_backward_ordered_strided) or the order-free integer sum ("fixed",
            # lz_grid_encode_backward_fixed with a row stride) per plane, on the plane's [0, 1] coordinates as the three-encoder path
            # forms them and on the plane's columns of the [B, 3 L] gradient where they lie
            unit = map01(xyz, bound)
            if per_plane == "ordered":
                need = int(_lib.load().lz_grid_ordered_workspace(B, 2))
                nbytes = min(need, ORDERED_WORKSPACE_CAP)
                ws = workspace("grid_ordered", xyz.device, nbytes, grow=True)
            for plane, cols in enumerate(((0, 1), (1, 2), (0, 2))):
                uv = unit[:, cols].contiguous()
                if per_plane == "ordered":
                    call("lz_grid_encode_backward_ordered_strided", grad.data_ptr() + 4 * plane * L, 3 * L, ptr(uv), ptr(offsets),
                         ptr(g_tables[plane]), B, 2, 1, L, S, H, 0, 0, ptr(ws), nbytes & 0xFFFFFFFF, nbytes >> 32, stream())
                else:
                    grid_backward_fixed(grad.data_ptr() + 4 * plane * L, uv, tables[plane], offsets, g_tables[plane], B, 2, 1, L, S, H, None,
                                        None, 0, False, 1, grad_row_stride=3 * L)
        if (want_tables and per_plane is None) or g_xyz is not None:
            gt = [None] * 3 if per_plane is not None else g_tables
            call("lz_triplane_encode_backward", ptr(grad), ptr(xyz), ptr(offsets), ptr(gt[0]), ptr(gt[1]), ptr(gt[2]), ptr(dy_dx), ptr(g_xyz), B, L,
                 S, H, bound, stream())
        return (g_xyz, g_tables[0], g_tables[1], g_tables[2], None, None, None, None, None)


class TriplaneEncoder(nn.Module):
    """NeRFNetwork.encode_x (network.py:208-223) as one operator: `xyz [B, 3]` in `[-bound, bound]` -> `[B, 3 L]`, the bits of
    `cat([encoder_xy(xyz[:, :2]), encoder_yz(xyz[:, 1:]), encoder_xz(xyz[:, [0, 2]])], -1)` in one launch, and one launch back.

    The three `GridEncoder`s are held in a plain tuple: not registered as submodules, their parameters not copied.  A network that
    adds `self.encoder_xyz = TriplaneEncoder(self.encoder_xy, self.encoder_yz, self.encoder_xz)` keeps its state_dict keys,
    parameters() and optimizer groups; gradients arrive in the three encoders' own `embeddings`."""

    def __init__(self, encoder_xy, encoder_yz, encoder_xz):
        super().__init__()
        encoders = (encoder_xy, encoder_yz, encoder_xz)
        self._check(encoders)
        object.__setattr__(self, "encoders", encoders)      # past nn.Module.__setattr__ on purpose (a tuple is not registered anyway)
        self.num_levels = encoder_xy.num_levels
        self.output_dim = 3 * encoder_xy.num_levels

    @staticmethod
    def _check(encoders):
        names = ("encoder_xy", "encoder_yz", "encoder_xz")
        for name, enc in zip(names, encoders):
            for field, want in (("input_dim", 2), ("level_dim", 1), ("gridtype", "hash"), ("align_corners", False)):
                if getattr(enc, field) != want:
                    raise RuntimeError("TriplaneEncoder: %s.%s must be %r, got %r" % (name, field, want, getattr(enc, field)))
            if not 1 <= enc.num_levels <= 16:
                raise RuntimeError("TriplaneEncoder: %s.num_levels must be 1 .. 16, got %r" % (name, enc.num_levels))
        first = encoders[0]
        for name, enc in zip(names[1:], encoders[1:]):
            for field in ("num_levels", "base_resolution", "per_level_scale"):
                if getattr(enc, field) != getattr(first, field):
                    raise RuntimeError("TriplaneEncoder: %s.%s = %r differs from encoder_xy.%s = %r"
                                       % (name, field, getattr(enc, field), field, getattr(first, field)))
            if enc.offsets.shape != first.offsets.shape or not torch.equal(enc.offsets.cpu(), first.offsets.cpu()):
                raise RuntimeError("TriplaneEncoder: %s.offsets differs from encoder_xy.offsets" % name)

    def _check_tables(self):
        # dtype and device can change after construction (.half(), .to(device)): looked at per call, metadata only
        first = self.encoders[0].embeddings
        for name, enc in zip(("encoder_xy", "encoder_yz", "encoder_xz"), self.encoders):
            if enc.embeddings.dtype != torch.float32:
                raise RuntimeError("TriplaneEncoder: %s.embeddings dtype must be torch.float32, got %s" % (name, enc.embeddings.dtype))
            if enc.embeddings.device != first.device or enc.offsets.device != first.device:
                raise RuntimeError("TriplaneEncoder: %s.embeddings device %s / offsets device %s differ from encoder_xy's device %s"
                                   % (name, enc.embeddings.device, enc.offsets.device, first.device))

    def extra_repr(self):
        return "3 x (%s) -> %d" % (self.encoders[0].extra_repr(), self.output_dim)

    def forward(self, xyz, bound=1):
        self._check_tables()
        exy, eyz, exz = self.encoders
        rows = xyz.reshape(-1, 3)
        S = float(np.float32(np.log2(exy.per_level_scale)))
        feats = _triplane_encode.apply(rows, exy.embeddings, eyz.embeddings, exz.embeddings, exy.offsets, exy.num_levels, S,
                                       int(exy.base_resolution), float(bound))
        return feats.view(*xyz.shape[:-1], self.output_dim)
