"""BASELINE cfg2 for TRAINING: the generic hash-grid NeRF of `synthetic.GenericHashgridNeRF.net` (get_encoder('hashgrid') -> sigma MLP
32-64-16 -> [SH(4) | 15 geometry features] -> colour MLP 31-64-3, bias-free Linear + ReLU like network.py:73-94, sigma = exp(h[0]),
rgb = sigmoid) as an autograd Function over fused kernels instead of ~25 operator launches per forward and their mirror images:

    forward   lz_grid_encode_forward_tiled (level-major gather, tiled f32 features) -> lz_ngp_head_forward (csrc/lz_ngp.hip)
    backward  lz_ngp_head_backward (csrc/lz_ngp_train.hip: recomputes the head, every MLP gradient on the matrix cores, a fixed-order
              combine of the weight gradients) -> lz_grid_encode_backward (grad_layout 0: the table scatter, float atomics), or with
              table_grad "ordered" lz_grid_encode_backward_ordered (no float atomics, the CPU checker's summation order)
              table_grad "fixed"   lz_grid_encode_backward_fixed (64-bit integer sums, one scale per level: free of the samples' order)

Scope: f32 arithmetic and f32 tables at the fixed cfg2 shape; no position / direction gradient.  What is not built is refused with an
error, never answered with a silently wrong gradient."""
import numpy as np
import torch
import torch.nn as nn
from torch.autograd import Function

from . import _lib, gridencoder
from ._util import as_f32, call, map01, ptr, stream, workspace
from .encoding import get_encoder
from .linear import MLP
from .ngp import GEO, HIDDEN, FusedHashgridNeRF, _check_shapes, _fragment_tables

_SHAPES = [(HIDDEN, 32), (1 + GEO, HIDDEN), (HIDDEN, 16 + GEO), (3, HIDDEN)]
_GATHER = {}


def _workspace(device):
    """lz_ngp_train_workspace() bytes per device: per-workgroup partials, rewritten by every backward (no initialisation)"""
    return workspace("ngp_train", device, _lib.load().lz_ngp_train_workspace())


def _gather_index(device):
    """per packed float of lz_ngp_head_forward's image: its index into cat(the four flattened weights, [0]) (ngp.pack_weights' layout).
    A constant table, copied to the device once from pinned memory without blocking the host"""
    key = (device.type, device.index)
    g = _GATHER.get(key)
    if g is None:
        layer, row, col, keep = _fragment_tables()
        sizes = [a * b for a, b in _SHAPES]
        base = np.cumsum([0] + sizes)
        ncols = np.array([b for _, b in _SHAPES])
        idx = np.where(keep, base[layer] + row * ncols[layer] + col, base[-1]).astype(np.int64)
        host = torch.from_numpy(idx).pin_memory()
        g = _GATHER[key] = (host, host.to(device, non_blocking=True))
    return g[1]


def _pack(ws):
    """the four live weight tensors -> LZ_NGP_FRAGS * 64 floats in fragment order (the values ngp.pack_weights writes), on the device"""
    flat = torch.cat([w.detach().reshape(-1) for w in ws] + [ws[0].new_zeros(1)])
    return flat[_gather_index(flat.device)]


class _NgpTrain(Function):
    @staticmethod
    def forward(ctx, meta, xyzs, dirs, emb, ws0, ws1, wc0, wc1):
        M, dev = xyzs.shape[0], xyzs.device
        sigma, rgb = torch.empty(M, dtype=torch.float32, device=dev), torch.empty(M, 3, dtype=torch.float32, device=dev)
        packed = _pack((ws0, ws1, wc0, wc1))
        feats = torch.empty(M, 32, dtype=torch.float32, device=dev)      # tiled: [tile][level][sample in tile][2]
        if M:
            call("lz_grid_encode_forward_tiled", ptr(xyzs), ptr(emb), ptr(meta["offsets"]), ptr(feats), M, None, meta["bound"], 3, 2, 16,
                 meta["S"], meta["H"], 0, 0, 0, stream())
            call("lz_ngp_head_forward", ptr(packed), ptr(feats), 1, ptr(dirs), M, None, ptr(sigma), ptr(rgb), stream())
        ctx.meta = meta
        ctx.save_for_backward(xyzs, dirs, emb, ws0, ws1, wc0, wc1, packed, feats)
        return sigma, rgb

    @staticmethod
    def backward(ctx, g_sigma, g_rgb):
        xyzs, dirs, emb, ws0, ws1, wc0, wc1, packed, feats = ctx.saved_tensors
        meta = ctx.meta
        M, dev = xyzs.shape[0], xyzs.device
        gws = [torch.empty_like(w) for w in (ws0, ws1, wc0, wc1)]
        g_emb = torch.zeros_like(emb)
        if M == 0:
            for g in gws:
                g.zero_()
        else:
            g_sigma, g_rgb = as_f32(g_sigma), as_f32(g_rgb)
            d_feats = torch.empty(16, M, 2, dtype=torch.float32, device=dev)
            call("lz_ngp_head_backward", ptr(packed), ptr(ws0), ptr(ws1), ptr(wc0), ptr(wc1), ptr(feats), ptr(dirs), M, None, ptr(g_sigma),
                 ptr(g_rgb), ptr(d_feats), *[ptr(g) for g in gws], ptr(_workspace(dev)), stream())
            # the gather's own mapping (lz_grid_unit -> lz_map01): torch's division by a host scalar, measured to be a reciprocal multiply
            unit = map01(xyzs, meta["bound"])
            mode = meta["table_grad"] or gridencoder.table_grad()
            if mode == "ordered":
                gridencoder.grid_backward_ordered(d_feats, unit, emb, meta["offsets"], g_emb, M, 3, 2, 16, meta["S"], meta["H"], None, None, 0,
                                                  False, 0)
            elif mode == "fixed":
                gridencoder.grid_backward_fixed(d_feats, unit, emb, meta["offsets"], g_emb, M, 3, 2, 16, meta["S"], meta["H"], None, None, 0,
                                                False, 0)
            else:
                call("lz_grid_encode_backward", ptr(d_feats), ptr(unit), ptr(emb), ptr(meta["offsets"]), ptr(g_emb), M, 3, 2, 16, meta["S"],
                     meta["H"], None, None, 0, 0, 0, 0, stream())
        return (None, None, None, g_emb) + tuple(gws)


def _check_encoder(encoder):
    if (encoder.input_dim != 3 or encoder.level_dim != 2 or encoder.gridtype_id != 0 or encoder.align_corners or encoder.num_levels != 16):
        raise RuntimeError("FusedHashgridTrainNeRF: the encoder must be get_encoder('hashgrid') with input_dim 3, num_levels 16, level_dim 2 "
                           "(hash, no align_corners); other encoders train on the operator API")


class FusedHashgridTrainNeRF(nn.Module):
    """The cfg2 network for training as two fused passes (csrc/lz_ngp.hip forward, csrc/lz_ngp_train.hip backward).

    Modules `encoder` (gridencoder.GridEncoder from get_encoder('hashgrid')), `sigma_net` and `color_net` (linear.MLP): the parameters and
    state-dict keys are theirs (`encoder.embeddings`, `encoder.offsets`, `sigma_net.net.{0,1}.weight`, `color_net.net.{0,1}.weight`), so
    the modules of a `synthetic.GenericHashgridNeRF` load as they are, or are passed in and shared.  Every call reads the live parameter
    tensors (writes through `.data`, as an EMA swap-in does, are seen).  forward(xyzs, dirs, bound) gives `ngp.FusedHashgridNeRF`'s bits
    for sigma and rgb.  The backward returns the table gradient and the four weight gradients (a fixed-order reduction: the same bits on
    every call, exactly linear in the upstream gradient, so GradScaler's powers of two pass through).  No host synchronisation.

    table_grad: how the table gradient is summed.  "atomic" = float atomics, repeatable only up to summation order; "ordered" = every
    table entry summed without atomics in the CPU checker's (sample, corner) order.  With "ordered" the whole backward repeats bit for
    bit -- `encoder.embeddings.grad` and the four weight gradients are the same bits on every call from the same inputs, and the table
    gradient equals oracle.grid_encode_backward on the d_feats of the backward -- at the price of a sort per level.  "fixed" = every
    term quantised with one power-of-two scale per level and summed as 64-bit integers (lz_grid_encode_backward_fixed): the backward
    repeats bit for bit as well, and the table gradient does not depend on the order of the samples either.  None (the default)
    follows gridencoder.set_table_grad, read at every backward.

    Refused: inputs that require grad (no position / direction gradient), autocast, half tables, other encoder or MLP shapes."""

    def __init__(self, encoder=None, sigma_net=None, color_net=None, table_grad=None):
        super().__init__()
        if table_grad is not None and table_grad not in gridencoder._TABLE_GRADS:
            raise ValueError("table_grad must be None or one of %s, got %r" % (gridencoder._TABLE_GRADS, table_grad))
        self.table_grad = table_grad
        if encoder is None:
            encoder, _ = get_encoder("hashgrid")
        _check_encoder(encoder)
        self.encoder = encoder
        self.sigma_net = sigma_net if sigma_net is not None else MLP(32, 1 + GEO, HIDDEN, 2)
        self.color_net = color_net if color_net is not None else MLP(16 + GEO, 3, HIDDEN, 2)
        _check_shapes(self._weights())
        # GridEncoder hyper-parameters as the kernels take them (gridencoder.h:12: log2 of the per-level scale narrowed to float)
        self._S = float(np.float32(np.log2(encoder.per_level_scale)))
        self._H = int(encoder.base_resolution)

    def _weights(self):
        return (self.sigma_net.net[0].weight, self.sigma_net.net[1].weight, self.color_net.net[0].weight, self.color_net.net[1].weight)

    def forward(self, xyzs, dirs, bound=1.0):
        """xyzs [..., 3] in [-bound, bound], dirs [..., 3] (unit) -> (sigma [M], rgb [M, 3]), M = the number of points"""
        if (torch.is_tensor(xyzs) and xyzs.requires_grad) or (torch.is_tensor(dirs) and dirs.requires_grad):
            raise RuntimeError("FusedHashgridTrainNeRF: no gradient with respect to positions or directions (train_camera); detach them or "
                               "use the operator path")
        if torch.is_autocast_enabled("cuda"):
            raise RuntimeError("FusedHashgridTrainNeRF trains in f32 only: run it outside torch.autocast (f16 training of this network is "
                               "not built)")
        emb = self.encoder.embeddings
        if emb.dtype != torch.float32:
            raise RuntimeError("FusedHashgridTrainNeRF trains f32 tables only (embeddings are %s)" % emb.dtype)
        _check_encoder(self.encoder)
        ws = self._weights()
        _check_shapes(ws)
        if any(w.dtype != torch.float32 for w in ws):
            raise RuntimeError("FusedHashgridTrainNeRF: the MLP weights must be float32")
        if not emb.is_cuda:
            raise RuntimeError("FusedHashgridTrainNeRF runs on the GPU: move the module with .cuda()")
        dev = emb.device
        xyzs = xyzs.reshape(-1, 3).to(dev, torch.float32).contiguous()
        dirs = dirs.reshape(-1, 3).to(dev, torch.float32).contiguous()
        if dirs.shape[0] != xyzs.shape[0]:
            raise RuntimeError("FusedHashgridTrainNeRF: xyzs and dirs hold different numbers of points")
        meta = dict(offsets=self.encoder.offsets.to(dev, torch.int32).contiguous(), bound=float(bound), S=self._S, H=self._H,
                    table_grad=self.table_grad)
        return _NgpTrain.apply(meta, xyzs, dirs, emb.contiguous(), *[w.contiguous() for w in ws])

    def to_inference(self, precision="f32", mode=None, **renderer):
        """an `ngp.FusedHashgridNeRF` on the current weights (renders through `ngp.HashgridRenderer`); its table is the live parameter.
        With `mode` ("loop" / "fused") or renderer arguments (density_bitfield=..., bound=..., cap=..., steps_per_pass=..., clip_to_occupancy=...): the
        `ngp.HashgridRenderer` of that network in that mode instead."""
        net = FusedHashgridNeRF(self.encoder, self.sigma_net, self.color_net, precision=precision)
        if mode is None and not renderer:
            return net
        from .ngp import HashgridRenderer
        return HashgridRenderer(net, mode="loop" if mode is None else mode, **renderer)
