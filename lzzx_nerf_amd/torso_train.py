"""Torso branch for TRAINING: `NeRFNetwork.forward_torso` (/root/reference/nerf_triplane/network.py:170-205) as an autograd graph over
this repo's operators -- frequency encoder (csrc/lz_encoders.hip, forward + backward), tiled-grid encoder D = 2 / L = 16 / C = 2
(csrc/lz_grid.hip, forward + scatter-add backward + dy/dx for the deformation path) and the bias-free MLPs on the MFMA Linear kernels
(csrc/lz_linear.hip).  Same parameters and state-dict keys as the reference (`anchor_points`, `torso_deform_net.*`, `torso_encoder.*`,
`torso_net.*`), so a checkpoint moves between this module, the reference and the one-launch inference kernel (`torso.FusedTorso`)
unchanged.  The audio nets (`AudioNet`, `AudioAttNet`) are plain torch Conv1d / Linear modules in the reference; their fused training path
is `audio_train.FusedAudioTrainNet` (the inference kernel `audio.FusedAudioEncoder` is forward-only).

`FusedTorsoTrainNet` is the same network trained through two kernels (csrc/lz_torso_train.hip): a forward that is the inference
kernel's arithmetic and a backward that recomputes it, plus `run_torso`, the reference's masked torso query with the background mix."""
import ctypes as C

import numpy as np
import torch
import torch.nn as nn
from torch.autograd import Function

from . import _lib, gridencoder
from ._util import as_f32, call, ptr, stream, workspace
from .encoding import get_encoder
from .linear import MLP

_TABLE_GRADS = gridencoder._TABLE_GRADS


class TorsoTrainNet(nn.Module):
    def __init__(self, ind_dim_torso=8, torso_shrink=0.8):
        super().__init__()
        self.torso_shrink = float(torso_shrink)
        self.anchor_points = nn.Parameter(torch.tensor([[0.01, 0.01, 0.1, 1], [-0.1, -0.1, 0.1, 1], [0.1, -0.1, 0.1, 1]]))   # network.py:158-159
        self.torso_deform_encoder, d_in = get_encoder("frequency", input_dim=2, multires=8)
        self.anchor_encoder, a_in = get_encoder("frequency", input_dim=6, multires=3)
        self.torso_deform_net = MLP(d_in + a_in + ind_dim_torso, 2, 32, 3)
        self.torso_encoder, t_in = get_encoder("tiledgrid", input_dim=2, num_levels=16, level_dim=2, base_resolution=16, log2_hashmap_size=16,
                                               desired_resolution=2048)
        self.torso_net = MLP(t_in + d_in + a_in + ind_dim_torso, 4, 32, 3)

    def forward(self, x, poses, c=None):
        """x [N,2] in [-1,1]; poses [1,4,4]; c [1, ind_dim_torso] or None -> alpha [N,1], color [N,3], dx [N,2]"""
        x = x * self.torso_shrink
        wrapped = self.anchor_points[None, ...] @ poses.permute(0, 2, 1).inverse()
        wrapped = (wrapped[:, :, :2] / wrapped[:, :, 3, None] / wrapped[:, :, 2, None]).view(1, -1)
        enc_anchor = self.anchor_encoder(wrapped)
        enc_x = self.torso_deform_encoder(x)
        parts = [enc_x, enc_anchor.repeat(x.shape[0], 1)]
        if c is not None:
            parts.append(c.repeat(x.shape[0], 1))
        h = torch.cat(parts, dim=-1)
        dx = self.torso_deform_net(h)
        x = (x + dx).clamp(-1, 1)
        x = self.torso_encoder(x, bound=1)
        h = self.torso_net(torch.cat([x, h], dim=-1))
        alpha = torch.sigmoid(h[..., :1]) * (1 + 2 * 0.001) - 0.001
        color = torch.sigmoid(h[..., 1:]) * (1 + 2 * 0.001) - 0.001
        return alpha, color, dx


def _workspace(device):
    """lz_torso_train_workspace() bytes per device: per-workgroup partials, rewritten by every backward (no initialisation)"""
    return workspace("torso_train", device, _lib.load().lz_torso_train_workspace())


class _AnchorEncode(Function):
    """network.py:179-183: anchor_points [3,4] through the inverse head pose -> enc_anchor [42]; no torch.inverse (its singularity check
    synchronises with the host)"""

    @staticmethod
    def forward(ctx, pose, anchors):
        enc = torch.empty(42, dtype=torch.float32, device=anchors.device)
        call("lz_torso_anchor_encode", ptr(pose), ptr(anchors), ptr(enc), stream())
        ctx.save_for_backward(pose, anchors)
        return enc

    @staticmethod
    def backward(ctx, g_enc):
        pose, anchors = ctx.saved_tensors
        g = g_enc.float().contiguous()
        g_anchors = torch.empty_like(anchors)
        call("lz_torso_anchor_encode_backward", ptr(pose), ptr(anchors), ptr(g), anchors.shape[0], ptr(g_anchors), stream())
        return None, g_anchors


class _TorsoTrain(Function):
    @staticmethod
    def forward(ctx, meta, xy, enc_anchor, ind, dw0, dw1, dw2, tw0, tw1, tw2, emb):
        net, N = meta["net"], xy.shape[0]
        kw = dict(dtype=torch.float32, device=xy.device)
        alpha, color, deform = torch.empty(N, 1, **kw), torch.empty(N, 3, **kw), torch.empty(N, 2, **kw)
        p = net._params(meta, xy, enc_anchor, ind, (dw0, dw1, dw2), (tw0, tw1, tw2), emb)
        call("lz_torso_train_forward", C.byref(p), ptr(xy), N, ptr(alpha), ptr(color), ptr(deform), stream())
        ctx.meta = meta
        ctx.save_for_backward(xy, enc_anchor, ind, dw0, dw1, dw2, tw0, tw1, tw2, emb)
        return alpha, color, deform

    @staticmethod
    def backward(ctx, g_alpha, g_color, g_deform):
        xy, enc_anchor, ind, dw0, dw1, dw2, tw0, tw1, tw2, emb = ctx.saved_tensors
        meta = ctx.meta
        net, N = meta["net"], xy.shape[0]
        ws = [torch.empty_like(w) for w in (dw0, dw1, dw2, tw0, tw1, tw2)]
        g_emb, g_enc = torch.zeros_like(emb), torch.empty_like(enc_anchor)
        g_ind = torch.empty_like(ind) if ind is not None else None
        if N == 0:
            for t in ws + [g_enc] + ([g_ind] if g_ind is not None else []):
                t.zero_()
        else:
            p = net._params(meta, xy, enc_anchor, ind, (dw0, dw1, dw2), (tw0, tw1, tw2), emb)
            g = _lib.TorsoGrads()
            g.g_deform_w0, g.g_deform_w1, g.g_deform_w2, g.g_torso_w0, g.g_torso_w1, g.g_torso_w2 = [w.data_ptr() for w in ws]
            g.g_emb, g.g_enc_anchor, g.g_ind_code = g_emb.data_ptr(), g_enc.data_ptr(), g_ind.data_ptr() if g_ind is not None else None
            g_alpha, g_color, g_deform = as_f32(g_alpha), as_f32(g_color), as_f32(g_deform)
            mode = net.table_grad
            if mode == "atomic":
                call("lz_torso_train_backward", C.byref(p), ptr(xy), N, ptr(g_alpha), ptr(g_color), ptr(g_deform), C.byref(g),
                     ptr(_workspace(xy.device)), stream())
            else:
                # the kernel writes d loss / d (grid features), level-major [16, N, 2], and the [0, 1] coordinates it gathered at (every row;
                # zeros and u = -1, which the grid kernels skip, for masked-out pixels); the grid encoder's table-gradient kernels sum
                # them into the zeroed g_emb
                if mode not in _TABLE_GRADS:
                    raise ValueError("FusedTorsoTrainNet: table_grad must be one of %s, got %r" % (_TABLE_GRADS, mode))
                denc, u = torch.empty(16, N, 2, dtype=torch.float32, device=xy.device), torch.empty(N, 2, dtype=torch.float32, device=xy.device)
                call("lz_torso_train_backward_rows", C.byref(p), ptr(xy), N, ptr(g_alpha), ptr(g_color), ptr(g_deform), C.byref(g),
                     ptr(_workspace(xy.device)), ptr(denc), ptr(u), stream())
                table_backward = gridencoder.grid_backward_ordered if mode == "ordered" else gridencoder.grid_backward_fixed
                table_backward(denc, u, emb, meta["offsets"], g_emb, N, 2, 2, 16, net._S, net._H, None, None, 1, False, 0)
                if net.keep_denc:
                    net.last_denc, net.last_u = denc, u
        return (None, None, g_enc, g_ind) + tuple(ws) + (g_emb,)


class FusedTorsoTrainNet(TorsoTrainNet):
    """`NeRFNetwork.forward_torso` for training, as two kernels (csrc/lz_torso_train.hip) instead of an autograd graph over operators.

    Same parameters, buffers and state-dict keys as `TorsoTrainNet` and the reference (`anchor_points`, `torso_deform_net.net.i.weight`,
    `torso_encoder.embeddings` / `.offsets`, `torso_net.net.i.weight`), the same initialisation, so a state dict moves between them and
    `torso.FusedTorso`.  Every call reads the live parameter tensors (no packed copies: writes through `.data`, as the reference's EMA
    does, are seen).  The forward gives `FusedTorso`'s bits for alpha, colour and deform.  The backward recomputes the forward and returns
    every gradient: weights, table, `anchor_points` (through the pose inverse) and the individual code; MLP weight and frame-constant
    gradients are reduced in a fixed order (same bits on every call).

    table_grad: how the table gradient is summed -- a plain attribute, read at every backward.  "atomic" (the default): float atomics
    inside the backward kernel, repeatable only up to summation order.  "ordered" / "fixed": the backward kernel writes the gradient of
    the grid features instead ([16, N, 2], with the [0, 1] coordinates it gathered at) and `gridencoder.grid_backward_ordered` /
    `grid_backward_fixed` sum it into the table: the same bits on every call, and with "fixed" under any order of the pixels as well
    (every term quantised with one power-of-two scale per level and summed as 64-bit integers, so the gradient still scales exactly
    with a GradScaler's power of two).  Every other gradient has the same bits in all three.  The default does NOT follow
    `gridencoder.set_table_grad`: a global mode set for another module leaves this one as it was.  With `keep_denc` set, the last
    "ordered" / "fixed" backward leaves those two tensors in `last_denc` and `last_u` (diagnostics; a masked-out pixel's rows are zeros
    and its `last_u` is (-1, -1), out of range for the grid encoder).

    Precision: f32 always.  Under `autocast` the inputs are cast to f32 and the kernels run in f32, as `FusedTorso` does (the reference's
    `-O` half-precision Linears are not reproduced).  Works under `GradScaler`: every gradient is linear in the upstream one.
    No host synchronisation: the occupancy threshold may stay a device scalar."""

    def __init__(self, ind_dim_torso=8, torso_shrink=0.8, table_grad="atomic"):
        if ind_dim_torso not in (0, 8):
            raise ValueError("FusedTorsoTrainNet: ind_dim_torso must be 0 or 8 (the reference's default)")
        if table_grad not in _TABLE_GRADS:
            raise ValueError("FusedTorsoTrainNet: table_grad must be one of %s, got %r" % (_TABLE_GRADS, table_grad))
        super().__init__(ind_dim_torso=ind_dim_torso, torso_shrink=torso_shrink)
        self.ind_dim = ind_dim_torso
        self.table_grad = table_grad
        self.keep_denc, self.last_denc, self.last_u = False, None, None
        # GridEncoder hyper-parameters of the torso encoder (network.py:166, grid.py:95-96), as torso.FusedTorso states them
        self._S = float(np.float32(np.log2(np.exp2(np.log2(2048 / 16) / 15))))
        self._H = 16

    def _params(self, meta, xy, enc_anchor, ind, dw, tw, emb):
        p = _lib.TorsoTrainParams()
        n = p.net
        n.deform_w0, n.deform_w1, n.deform_w2 = [w.data_ptr() for w in dw]
        n.torso_w0, n.torso_w1, n.torso_w2 = [w.data_ptr() for w in tw]
        n.emb, n.offsets, n.enc_anchor = emb.data_ptr(), meta["offsets"].data_ptr(), enc_anchor.data_ptr()
        n.ind_code = ind.data_ptr() if ind is not None else None
        n.ind_dim, n.gridtype, n.torso_shrink, n.S, n.H = self.ind_dim, 1, self.torso_shrink, self._S, self._H
        grid = meta["density_grid"]
        n.density_grid, n.G, n.density_thresh = (grid.data_ptr(), meta["G"], meta["thresh_f"]) if grid is not None else (None, 0, 0.0)
        p.density_thresh = meta["thresh_t"].data_ptr() if meta["thresh_t"] is not None else None
        bg = meta["bg"]
        p.bg, p.bg_scalar, p.mix = (bg.data_ptr() if bg is not None else None), meta["bg_scalar"], int(meta["mix"])
        p.n_offsets = meta["offsets"].numel()
        return p

    def _run(self, bg_coords, poses, c, mix=False, bg_color=1.0, density_grid=None, density_thresh=None):
        dev = self.anchor_points.device
        with torch.autocast(device_type="cuda", enabled=False):
            xy = bg_coords.reshape(-1, 2).to(dev, torch.float32).contiguous()
            N = xy.shape[0]
            pose = poses.to(dev, torch.float32).reshape(-1, 4, 4)
            if pose.shape[0] != 1:
                raise RuntimeError("FusedTorsoTrainNet: one head pose per call (network.py:179)")
            ind = None
            if self.ind_dim:
                if c is None:
                    raise RuntimeError("this torso network has an individual code (ind_dim_torso = %d)" % self.ind_dim)
                ind = c.reshape(-1).to(dev, torch.float32).contiguous()
                if ind.numel() != self.ind_dim:
                    raise RuntimeError("individual code: %d values, want %d" % (ind.numel(), self.ind_dim))
            meta = dict(net=self, offsets=self.torso_encoder.offsets.to(dev, torch.int32).contiguous(), density_grid=None, G=0, thresh_f=0.0,
                        thresh_t=None, bg=None, bg_scalar=0.0, mix=mix)
            if density_grid is not None:
                grid = density_grid.reshape(-1).detach().to(dev, torch.float32).contiguous()
                G = round(grid.numel() ** 0.5)
                if G * G != grid.numel() or G < 2:
                    raise RuntimeError("density_grid must hold grid_size^2 values")
                meta.update(density_grid=grid, G=G)
                if isinstance(density_thresh, torch.Tensor):
                    meta["thresh_t"] = density_thresh.detach().reshape(-1)[:1].to(dev, torch.float32).contiguous()
                else:
                    meta["thresh_f"] = float(0.0 if density_thresh is None else density_thresh)
            if mix:
                if isinstance(bg_color, torch.Tensor):   # broadcast on the device: no .item()
                    bg = bg_color.detach().to(dev, torch.float32)
                    meta["bg"] = (bg.reshape(1, 1) if bg.numel() == 1 else bg.reshape(-1, 3)).expand(N, 3).contiguous()
                else:
                    meta["bg_scalar"] = float(bg_color)
            enc_anchor = _AnchorEncode.apply(pose.contiguous(), self.anchor_points)
            w = lambda m, i: m.net[i].weight
            return _TorsoTrain.apply(meta, xy, enc_anchor, ind, w(self.torso_deform_net, 0), w(self.torso_deform_net, 1), w(self.torso_deform_net, 2),
                                     w(self.torso_net, 0), w(self.torso_net, 1), w(self.torso_net, 2), self.torso_encoder.embeddings)

    def forward(self, x, poses, c=None):
        """x [N,2] in [-1,1]; poses [1,4,4]; c [1, ind_dim_torso] or None -> alpha [N,1], color [N,3], dx [N,2] (as TorsoTrainNet)"""
        return self._run(x, poses, c)

    def run_torso(self, bg_coords, poses, ind_code=None, bg_color=1, density_grid=None, density_thresh=None):
        """`NeRFRenderer.run_torso` (renderer.py:572-631) for training: 2-D occupancy mask (density_grid [G*G], density_thresh a float or a
        one-element device tensor, e.g. update_density_grid_torso's threshold), masked forward_torso, background mix -> dict(torso_alpha
        [N,1], torso_color [N,3] = c a + bg (1 - a), bg_color (the same tensor, as the reference returns it), deform [N,2]).  The result
        feeds objective.TorsoObjective directly.  Unlike the reference, whose `deform` holds only the masked rows, `deform` here covers all
        N pixels with zeros on the masked-out ones; masked-out pixels have alpha 0 and colour exactly bg, and contribute no gradient.
        bg_color: a number, a one-element tensor or [N,3] / [3] (not differentiated)."""
        alpha, color, deform = self._run(bg_coords, poses, ind_code, mix=True, bg_color=bg_color, density_grid=density_grid,
                                         density_thresh=density_thresh)
        return dict(torso_alpha=alpha, torso_color=color, bg_color=color, deform=deform)
