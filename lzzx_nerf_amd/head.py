"""Fused triplane head: the per-sample arithmetic of NeRFNetwork.forward / density
(/root/reference/nerf_triplane/network.py:252-311) as ONE gfx950 kernel (csrc/lz_head.hip):
3 hash-grid planes -> audio-channel / eye attention -> sigma net -> SH(4) -> colour net (-> uncertainty net).

It consumes the reference's state_dict unchanged (keys `encoder_{xy,yz,xz}.embeddings`, `*.offsets`,
`{aud_ch_att,eye_att,sigma,color,unc}_net.net.N.weight`, `individual_codes`), so a trained
checkpoint renders without conversion.  The drop-in operator path (encoding.get_encoder + torch Linear)
stays available for the reference's own NeRFNetwork; this module is the fast path used by
lzzx_nerf_amd.renderer and bench.py.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._util import call, ptr, stream

_W_KEYS = ["aud_ch_att_net.net.0.weight", "aud_ch_att_net.net.1.weight", "eye_att_net.net.0.weight", "eye_att_net.net.1.weight",
           "sigma_net.net.0.weight", "sigma_net.net.1.weight", "sigma_net.net.2.weight", "color_net.net.0.weight",
           "color_net.net.1.weight", "unc_net.net.0.weight", "unc_net.net.1.weight"]


class FusedTriplaneHead:
    """Inference/forward-only fused head (autograd for training goes through the operator path)."""

    def __init__(self, state_dict, bound=1.0, exp_eye=True, device="cuda", precision="f32", fold_geo=False):
        """precision "f32": f32 MFMA, bit-exact against the checker.  "f16": the reference's opt.fp16 / autocast arithmetic
        (half Linear inputs, weights and outputs, f32 accumulate) on the f16 matrix cores; inference only."""
        if precision not in ("f32", "f16"):
            raise ValueError("precision must be 'f32' or 'f16'")
        self.precision = precision
        # fold_geo (f32, inference): geo_feat = sigma_net.2[1:65] s2 reaches color_net.0 through nothing but that linear map
        # (network.py:304-306), so the 64 x 64 product of the two matrices is packed in color_net.0's geo columns and the geo rows of
        # sigma_net.2 are never evaluated: 64 of 361 MFMAs per 16 samples less.  sigma is unchanged bit for bit, rgb moves by the
        # reassociation (a few 1e-7).
        if fold_geo and precision != "f32":
            raise ValueError("fold_geo goes with precision='f32' (the f16 head keeps autocast's rounding points)")
        self.fold_geo = bool(fold_geo)
        self.device = torch.device(device)
        self.bound = float(bound)
        sd = {k: v.detach().to(self.device, torch.float32).contiguous() for k, v in state_dict.items()
              if k in _W_KEYS or k.startswith("encoder_") and k.endswith(".embeddings") or k == "individual_codes"}
        self.emb = [sd["encoder_%s.embeddings" % p] for p in ("xy", "yz", "xz")]
        self.offsets = state_dict["encoder_xy.offsets"].to(self.device, torch.int32).contiguous()
        if self.offsets.numel() != 13 or self.emb[0].shape[1] != 1:
            raise RuntimeError("FusedTriplaneHead expects the triplane configuration (D=2, L=12, C=1, network.py:129-133)")
        # the fused kernel masks instead of taking `% size` on hashed levels: sizes there are 2^14 by construction
        # (grid.py:116); verify once on the host, at construction
        off = self.offsets.cpu().numpy().astype(np.int64)
        for l in range(12):
            size, res1 = int(off[l + 1] - off[l]), int(np.ceil(np.float32(np.exp2(np.float32(l) * np.float32(np.log2(np.exp2(np.log2(512 * self.bound / 64) / 11)))) * 64 - 1))) + 2
            if res1 * res1 > size and size & (size - 1):
                raise RuntimeError("FusedTriplaneHead: hashed level %d has a non power-of-two table (%d entries)" % (l, size))
        self.w = [sd.get(k) for k in _W_KEYS]
        self.has_eye = bool(exp_eye)
        self.individual_codes = sd.get("individual_codes")
        self.has_ind = self.individual_codes is not None and self.w[7].shape[1] == 84
        exp_sig = 68 + (1 if self.has_eye else 0)
        if self.w[4].shape[1] != exp_sig:
            raise RuntimeError("sigma_net input width %d does not match exp_eye=%s" % (self.w[4].shape[1], self.has_eye))
        # GridEncoder hyper-parameters of the triplane (network.py:131-133, grid.py:95-96)
        self.H = 64
        self.per_level_scale = np.exp2(np.log2(512 * self.bound / 64) / 11)
        self.S = float(np.float32(np.log2(self.per_level_scale)))
        if precision == "f16":
            self.packed = torch.empty(_lib.load().lz_head_packed_size_f16w(), dtype=torch.uint8, device=self.device)
        else:
            self.packed = torch.empty(_lib.load().lz_head_packed_size(), dtype=torch.float32, device=self.device)
        self.repack()

    @classmethod
    def from_network(cls, net, **kw):
        """net: a nerf_triplane.network.NeRFNetwork (reference class, unmodified)"""
        return cls(net.state_dict(), bound=net.bound, exp_eye=bool(getattr(net, "exp_eye", True)), **kw)

    def repack(self):
        """(re)build the MFMA A-fragment buffer; call after the weights change"""
        w = self.w
        if self.precision == "f16":
            call("lz_head_pack_weights_f16w", *[ptr(t) for t in w[:9]], int(self.has_eye), int(self.has_ind), ptr(self.packed), stream())
        else:
            if self.fold_geo:
                w = list(w)
                folded = (w[7][:, 16:80].double() @ w[6][1:65].double()).float()
                w[7] = torch.cat([w[7][:, :16], folded, w[7][:, 80:]], 1).contiguous()
            call("lz_head_pack_weights", *[ptr(t) for t in w], int(self.has_eye), int(self.has_ind), ptr(self.packed), stream())

    def _params(self, enc_a, ind_code, eye, testing):
        p = _lib.HeadParams()
        p.emb_xy, p.emb_yz, p.emb_xz = self.emb[0].data_ptr(), self.emb[1].data_ptr(), self.emb[2].data_ptr()
        p.offsets, p.packed, p.enc_a = self.offsets.data_ptr(), self.packed.data_ptr(), enc_a.data_ptr()
        p.ind_code = ind_code.data_ptr() if (ind_code is not None and self.has_ind) else None
        p.eye = eye.data_ptr() if (eye is not None and self.has_eye) else None
        p.bound, p.S, p.H, p.testing = self.bound, self.S, self.H, int(bool(testing))
        p.precision = 1 if self.precision == "f16" else (2 if self.fold_geo and testing else 0)
        return p

    def forward(self, xyzs, dirs, enc_a, ind_code=None, eye=None, testing=True, count_ptr=None, out=None):
        """xyzs, dirs: [M, 3] f32 cuda.  Returns sigma [M], rgb [M,3], amb_aud [M,1], amb_eye [M,1], unc [M,1]
        (same tuple as NeRFNetwork.forward, network.py:280).  `count_ptr`: device address of an int32 that bounds
        the rows actually processed (the render loop's n_samples)."""
        M = xyzs.shape[0]
        enc_a = enc_a.reshape(-1).float().contiguous()
        if enc_a.numel() != 32:
            raise RuntimeError("enc_a must hold 32 audio features")
        ind_code = None if ind_code is None else ind_code.reshape(-1).float().contiguous()
        eye = None if eye is None else eye.reshape(-1).float().contiguous()
        if not testing and self.w[9] is None:
            raise RuntimeError("training-mode uncertainty needs unc_net weights")
        if not testing and self.precision == "f16":
            raise RuntimeError("the f16 head is inference-only")
        if not testing and self.fold_geo:
            raise RuntimeError("fold_geo packs an inference-only arrangement of color_net.0")
        if out is None:
            kw = dict(dtype=torch.float32, device=xyzs.device)
            out = (torch.empty(M, **kw), torch.empty(M, 3, **kw), torch.empty(M, 1, **kw), torch.empty(M, 1, **kw),
                   torch.empty(M, 1, **kw))
        sig, rgb, aa, ae, un = out
        p = self._params(enc_a, ind_code, eye, testing)
        # keep the small tensors alive until the launch is enqueued (same stream -> ordering is enough)
        call("lz_triplane_head_forward", C.byref(p), ptr(xyzs), ptr(dirs), M, C.c_void_p(count_ptr) if count_ptr else None,
             ptr(sig), ptr(rgb), ptr(aa), ptr(ae), ptr(un), stream())
        self._keep = (enc_a, ind_code, eye)
        return sig, rgb, aa, ae, un

    __call__ = forward

    def _density_inputs(self, enc_a, eye):
        enc_a = enc_a.reshape(-1).float().contiguous()
        if enc_a.numel() != 32:
            raise RuntimeError("enc_a must hold 32 audio features")
        eye = None if eye is None else eye.reshape(-1).float().contiguous()
        self._keep = (enc_a, None, eye)   # alive until the launch is enqueued (same stream -> ordering is enough)
        return self._params(enc_a, None, eye, True), eye is not None and self.has_eye

    def density(self, x, enc_a, eye=None, geo_feat=False, count_ptr=None, out=None):
        """NeRFNetwork.density(x, enc_a, e) (network.py:283-311) as one launch that stops behind sigma_net (csrc/lz_density.hip): no SH, no
        colour net.  x: [M, 3] f32 cuda.  Returns the reference's keys: sigma [M], ambient_aud [M,1], ambient_eye [M,1] (None without an
        eye input) -- the bits forward() gives for the same points -- and, when asked for, geo_feat [M,64] (f32; half on the f16 head, as
        under autocast).  `out`: a dict of preallocated tensors under the same keys (at least M rows each)."""
        M = x.shape[0]
        p, with_eye = self._density_inputs(enc_a, eye)
        kw = dict(dtype=torch.float32, device=x.device)
        o = dict(out) if out is not None else {}
        o.setdefault("sigma", torch.empty(M, **kw))
        o.setdefault("ambient_aud", torch.empty(M, 1, **kw))
        if with_eye:
            o.setdefault("ambient_eye", torch.empty(M, 1, **kw))
        else:
            o["ambient_eye"] = None
        if geo_feat:
            o.setdefault("geo_feat", torch.empty(M, 64, dtype=torch.float16 if self.precision == "f16" else torch.float32, device=x.device))
        call("lz_triplane_head_density", C.byref(p), ptr(x), M, C.c_void_p(count_ptr) if count_ptr else None, ptr(o["sigma"]),
             ptr(o["ambient_aud"]), ptr(o["ambient_eye"]), ptr(o["geo_feat"]) if geo_feat else None, stream())
        return o

    def density_lattice(self, enc_a, eye=None, noise=None, grid_size=0, axes=None, sigma=False, ambient=False):
        """density() on points made in the kernel (lz_triplane_density_lattice), storing only what is asked for.  Either `noise`
        [cascade, G^3, 3] with `grid_size` G -- the occupancy grid's cells, rows in the order lz_density_grid_update consumes -- or
        `axes` = (X, Y, Z), three 1-d f32 cuda tensors: row (i Ry + j) Rz + k is (X[i], Y[j], Z[k]).  Returns (sigma, ambient_aud,
        ambient_eye), flat [rows] f32; None where not asked for (ambient_eye also without an eye input)."""
        p, with_eye = self._density_inputs(enc_a, eye)
        if axes is None:
            rows = noise.shape[0] * grid_size ** 3
            src = (_lib.LZ_LATTICE_CELLS, ptr(noise), noise.shape[0], grid_size, None, 0, None, 0, None, 0)
            dev = noise.device
        else:
            X, Y, Z = axes
            rows = X.numel() * Y.numel() * Z.numel()
            src = (_lib.LZ_LATTICE_AXES, None, 0, 0, ptr(X), X.numel(), ptr(Y), Y.numel(), ptr(Z), Z.numel())
            dev = X.device
        new = lambda want: torch.empty(rows, dtype=torch.float32, device=dev) if want else None
        sig, aud, eyo = new(sigma), new(ambient), new(ambient and with_eye)
        call("lz_triplane_density_lattice", C.byref(p), *src, ptr(sig), ptr(aud), ptr(eyo), stream())
        return sig, aud, eyo
