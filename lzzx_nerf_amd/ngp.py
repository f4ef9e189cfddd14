"""BASELINE cfg2 on fused kernels: a generic hash-grid NeRF on the operators of `encoding.get_encoder` (encoding.py:6-37) --
hashgrid defaults (input_dim 3, num_levels 16, level_dim 2, log2_hashmap_size 19), SH(4) directions, a sigma MLP 32-64-16 and a colour
MLP 31-64-3 (bias-free Linear + ReLU like network.py:73-94; sigma = exp(row 0), rgb = sigmoid) -- as

    FusedHashgridNeRF   the per-sample network: level-major gather (tiled output, never untiled) + ONE MFMA kernel for both MLPs, SH and
                        the activations (csrc/lz_ngp.hip) -- what `GridEncoder -> MLP -> cat -> MLP` does in ~25 launches per iteration;
                        precision="f16": the same in the reference's torch-autocast arithmetic on f16 MFMAs
    HashgridRenderer    the reference's inference loop (renderer.py:495-548) around it: loop state on the device, 4 launches per
                        iteration (march, gather, head, composite) enqueued by one C call per chunk, no host round trip

Same operators, same arithmetic per sample as the operator-API network (`synthetic.GenericHashgridNeRF`), up to the summation order of
the Linear layers (here: MFMA k order, restated by the checker in oracle/ngp.py; there: the lz_linear kernels')."""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._util import call, ptr, stream
from .renderer import MAX_RAYS_PER_PASS, _STATE_INTS, _N_SAMPLES_OFF, RayRenderer, TriplaneRenderer, _empty_result   # noqa: F401

NGP_FRAGS = 96          # LZ_NGP_FRAGS
TILE_ROWS = 256         # LZ_GRID_TILE_ROWS
GEO = 15                # geometry features handed from the sigma net to the colour net
HIDDEN = 64


def _fragment_tables():
    """(layer, row, col, keep) per packed float: fragment (ks, ft), lane l = W[16 ft + (l & 15)][k(ks, l >> 4)] (csrc/lz_ngp.hip)"""
    lane = np.arange(64)
    m, q = lane & 15, lane >> 4
    layer, row, col, keep = [], [], [], []

    def add(which, r, c, k):
        layer.append(np.full(64, which)); row.append(r); col.append(c); keep.append(k)

    one = np.ones(64, bool)
    for ks in range(8):                     # sigma_net.0 [64, 32]: lane q reads levels q, q + 4, q + 8, q + 12, both channels
        for ft in range(4):
            add(0, 16 * ft + m, 2 * (q + 4 * (ks >> 1)) + (ks & 1), one)
    for ks in range(16):                    # sigma_net.1 [16, 64]: the previous accumulator tile in place
        add(1, m, 16 * (ks >> 2) + 4 * q + (ks & 3), one)
    for ks in range(8):                     # colour_net.0 [64, 31]: SH component 4 ks + q, then sigma_net output 4 q + r (row 0 = sigma: weight 0)
        for ft in range(4):
            if ks < 4:
                add(2, 16 * ft + m, 4 * ks + q, one)
            else:
                slot = 4 * q + (ks - 4)
                add(2, 16 * ft + m, np.maximum(16 + slot - 1, 0), slot >= 1)
    for ks in range(16):                    # colour_net.1 [3, 64] in one 16-row tile
        add(3, np.minimum(m, 2), 16 * (ks >> 2) + 4 * q + (ks & 3), m < 3)
    return [np.concatenate(a) for a in (layer, row, col, keep)]


_TABLES = None

NGP_FRAGS_F16 = 16      # LZ_NGP_PACKED_F16_BYTES / 1024: fragments of 64 lanes x 8 halves
SIGMA_ROW = 4           # tile row of sigma_net's output 0 (sigma) in the f16 head; output 4 takes row 0 (csrc/lz_ngp.hip: lz_k_ngp_head16)
COLOUR_ROWS = (0, 4, 1)  # tile rows of colour channels 0, 1, 2 in the f16 head


def _fragment_tables_f16():
    """(layer, row, col, keep) per packed half of lz_k_ngp_head16 (v_mfma_f32_32x32x16_f16, csrc/lz_head_f16w_slice.h's layout):
    fragment (ks, ft) of a layer, lane l = (r = l & 31, h = l >> 5), element j = W[tile row 32 ft + r][k slot 16 ks + 8 h + j]"""
    lane = np.arange(64)
    r, h = lane & 31, lane >> 5
    chain = lambda ks, j: 16 * ks + 8 * (j >> 2) + 4 * h + (j & 3)     # w_chain: k slot -> feature of the previous layer's D tiles
    sig_out = np.array([SIGMA_ROW if t == 0 else (0 if t == SIGMA_ROW else t) for t in range(32)])   # tile row -> sigma_net output
    col_out = np.full(32, -1)
    col_out[list(COLOUR_ROWS)] = [0, 1, 2]
    layer, row, col, keep = [], [], [], []

    def add(which, rr, cc, kk):
        layer.append(np.full(64, which)); row.append(rr); col.append(cc); keep.append(kk)

    one = np.ones(64, bool)
    for ks in range(2):                     # sigma_net.0 [64, 32]: k slot = feature (lane half h gathers levels 8 ks + 4 h .. + 3)
        for ft in range(2):
            for j in range(8):
                add(0, 32 * ft + r, 16 * ks + 8 * h + j, one)
    for ks in range(4):                     # sigma_net.1 [16, 64]: one tile, rows 16..31 zero, sigma at tile row SIGMA_ROW
        for j in range(8):
            add(1, np.where(r < 16, sig_out[r], 0), chain(ks, j), r < 16)
    for ks in range(2):                     # colour_net.0 [64, 31]: SH component 8 h + j, then sigma_net's tile (sigma's row weighted 0)
        for ft in range(2):
            for j in range(8):
                if ks == 0:
                    add(2, 32 * ft + r, 8 * h + j, one)
                else:
                    o = sig_out[chain(0, j)]
                    add(2, 32 * ft + r, np.maximum(16 + o - 1, 0), o >= 1)
    for ks in range(4):                     # colour_net.1 [3, 64]: channels at tile rows COLOUR_ROWS, every other row zero
        for j in range(8):
            add(3, np.maximum(col_out[r], 0), chain(ks, j), col_out[r] >= 0)
    # element order: fragment, lane, j
    n = NGP_FRAGS_F16 * 64 * 8
    out = [np.concatenate(a).reshape(NGP_FRAGS_F16, 8, 64).transpose(0, 2, 1).reshape(n) for a in (layer, row, col, keep)]
    return out


_TABLES16 = None


def pack_weights_f16(sigma_w0, sigma_w1, color_w0, color_w1):
    """the four weight matrices (torch Linear layout [out, in]) -> LZ_NGP_PACKED_F16_BYTES of halves (float16 tensor on their device) in
    lz_k_ngp_head16's fragment order; each weight rounded to half once, as autocast casts an f32 Linear weight"""
    global _TABLES16
    ws = [w.detach().float() for w in (sigma_w0, sigma_w1, color_w0, color_w1)]
    _check_shapes(ws)
    if _TABLES16 is None:
        _TABLES16 = _fragment_tables_f16()
    layer, row, col, keep = _TABLES16
    dev = ws[0].device
    out = torch.zeros(NGP_FRAGS_F16 * 64 * 8, dtype=torch.float16, device=dev)
    for i, w in enumerate(ws):
        sel = np.nonzero((layer == i) & keep)[0]
        out[torch.from_numpy(sel).to(dev)] = w[torch.from_numpy(row[sel]).to(dev), torch.from_numpy(col[sel]).to(dev)].half()
    return out.contiguous()


def _check_shapes(ws):
    shapes = [(HIDDEN, 32), (1 + GEO, HIDDEN), (HIDDEN, 16 + GEO), (3, HIDDEN)]
    for w, sh in zip(ws, shapes):
        if tuple(w.shape) != sh:
            raise RuntimeError("FusedHashgridNeRF supports sigma MLP 32-64-16 and colour MLP 31-64-3 (got a weight of shape %s where %s is expected); "
                               "other architectures run on the operator API (renderer.NetworkRenderer)" % (tuple(w.shape), sh))


def pack_weights(sigma_w0, sigma_w1, color_w0, color_w1):
    """the four weight matrices (torch Linear layout [out, in]) -> LZ_NGP_FRAGS * 64 floats in MFMA fragment order, on their device"""
    global _TABLES
    ws = [w.detach().float() for w in (sigma_w0, sigma_w1, color_w0, color_w1)]
    _check_shapes(ws)
    if _TABLES is None:
        _TABLES = _fragment_tables()
    layer, row, col, keep = _TABLES
    dev = ws[0].device
    out = torch.zeros(NGP_FRAGS * 64, dtype=torch.float32, device=dev)
    for i, w in enumerate(ws):
        sel = np.nonzero((layer == i) & keep)[0]
        out[torch.from_numpy(sel).to(dev)] = w[torch.from_numpy(row[sel]).to(dev), torch.from_numpy(col[sel]).to(dev)]
    return out.contiguous()


class FusedHashgridNeRF:
    """encoder: a gridencoder.GridEncoder built by get_encoder('hashgrid') (input_dim 3, level_dim 2, gridtype hash, no align_corners);
    sigma_net / color_net: linear.MLP or anything with `.net[i].weight` (two bias-free layers each).  half_tables: gather from an f16
    copy of the table and hand f16 features to the (f32) head (what grid.py:28,38-39 does under autocast with an even level_dim).
    precision "f16": the whole network in the reference's autocast arithmetic -- half tables and the half head (csrc/lz_ngp.hip:
    lz_k_ngp_head16); sigma / rgb come back as f32 tensors holding half-derived values (rgb: halves, sigma: exp in f32 of a half)."""

    def __init__(self, encoder, sigma_net, color_net, half_tables=None, precision="f32"):
        if encoder.input_dim != 3 or encoder.level_dim != 2 or encoder.gridtype_id != 0 or encoder.align_corners or encoder.num_levels != 16:
            raise RuntimeError("FusedHashgridNeRF: the encoder must be get_encoder('hashgrid') with input_dim 3, num_levels 16, level_dim 2")
        if precision not in ("f32", "f16"):
            raise ValueError("FusedHashgridNeRF: precision is 'f32' or 'f16', not %r" % (precision,))
        if precision == "f16" and half_tables is not None and not half_tables:
            raise ValueError("FusedHashgridNeRF: precision 'f16' gathers from half tables (half_tables=False contradicts it)")
        self.encoder = encoder
        self.precision = precision
        self.half_tables = precision == "f16" or bool(half_tables)
        ws = (sigma_net.net[0].weight, sigma_net.net[1].weight, color_net.net[0].weight, color_net.net[1].weight)
        self.packed = pack_weights(*ws)
        self.packed16 = pack_weights_f16(*ws) if precision == "f16" else None
        emb = encoder.embeddings.detach()
        self.table = emb.half().contiguous() if self.half_tables else emb.float().contiguous()
        self.offsets = encoder.offsets.contiguous()
        self.S = float(np.log2(encoder.per_level_scale))

    def forward(self, xyzs, dirs, bound=1.0, out=None):
        """xyzs [M, 3] in [-bound, bound], dirs [M, 3] -> (sigma [M], rgb [M, 3]); ready in stream order"""
        xyzs = xyzs.reshape(-1, 3).float().contiguous()
        dirs = dirs.reshape(-1, 3).float().contiguous()
        M, dev = xyzs.shape[0], xyzs.device
        feats = torch.empty(M, 32, dtype=self.table.dtype, device=dev)
        sigma, rgb = out if out is not None else (torch.empty(M, device=dev), torch.empty(M, 3, device=dev))
        self.encode_tiled(xyzs, feats, bound)
        if self.packed16 is not None:
            call("lz_ngp_head_forward_f16", ptr(self.packed16), ptr(feats), 2, ptr(dirs), M, None, ptr(sigma), ptr(rgb), stream())
        else:
            call("lz_ngp_head_forward", ptr(self.packed), ptr(feats), 2 if self.half_tables else 1, ptr(dirs), M, None, ptr(sigma), ptr(rgb), stream())
        return sigma, rgb

    def encode_tiled(self, xyzs, feats, bound, count_ptr=None):
        e = self.encoder
        call("lz_grid_encode_forward_tiled", ptr(xyzs), ptr(self.table), ptr(self.offsets), ptr(feats), xyzs.shape[0], count_ptr, float(bound), 3, 2,
             e.num_levels, self.S, e.base_resolution, 0, 0, int(self.half_tables), stream())


class HashgridRenderer(RayRenderer):
    """Inference renderer of one FusedHashgridNeRF + occupancy bitfield: the reference's loop (renderer.py:495-548: march n_step samples per
    alive ray, network, composite_rays, drop dead rays, n_step = max(min(budget_factor * N // n_alive, n_step_cap), 1), stop at max_steps)
    with the state on the device; (budget_factor, n_step_cap) = (1, 8) is the reference's schedule -- same pixels under any schedule for
    rays that end before max_steps, and exactly the reference's cap semantics under (1, 8), the default (like TriplaneRenderer /
    NetworkRenderer; fatter schedules such as (8, 8) are faster and differ on rays that reach max_steps).

    mode "loop" (default): four launches per iteration of that loop, the host looks a few chunks ahead for the end of the frame.
    mode "fused": the whole frame as one persistent kernel (csrc/lz_ngp_frame.hip: march, 16-level gather, network and compositing per ray
      slot, refill from a longest-first queue; 6 launches per frame, 3 under cap "per_ray"), no per-sample buffers, no host round trip: no
      ring, no events.  Same result dict, same bits as mode "loop" for f32 and f16 alike.
        cap "reference" (default): exactly the loop's cap semantics under this renderer's schedule -- every ray alive at the cap receives
          C_eff = the schedule's sum of n_step samples (budget_factor scales the ray budget of the replayed schedule; n_step_cap must be
          the reference's 8).
        cap "per_ray": a ray alive at max_steps stops there; equal to the loop on every ray that ends before max_steps, three launches less.
      Measured on MI355X (loop and fused alternated on one box): fused is faster than the loop in every case measured
      but one -- the 256^2 x 128-step frame 1.07 against 3.14 ms under (1, 8) and 1.98 under (8, 8) (f16 head 0.73 against 2.54 / 1.75;
      half tables + f32 head: see DESIGN), max_steps 16 0.30 against 0.62 ms, a 64^2 tile 0.50 against 2.03 / 0.54 -- and slower only on
      a 64^2 tile with the f16 head under the fat schedule (8, 8): 0.59 against 0.48 ms.  The default stays "loop".
        steps_per_pass (fused only; default 1): samples per ray and pass of the persistent kernel, S = 1, 2, 4, 8 or 16, or 0 = chosen
          per frame from the ray count, the head's slot width and the CU count (1 whenever the rays fill the slots).  With S > 1 a
          slice's columns hold 16 / S (f16 head: 32 / S) rays with S consecutive samples each (csrc/lz_ngp_frame_spp.hip), so a ray needs
          1 / S of the dependent passes: for tiles, crops and previews, whose rays do not fill the chip.  A launch shape only -- a ray stops
          exactly at the cap under either `cap`, every output and count is S = 1's bit for bit; state[72] (slices run) differs.  An
          attribute, changeable between frames; `last_steps_per_pass` is the S the last fused frame ran at.  Measured (DESIGN.md 4.5 has
          the sweep): a 64^2 tile at 0 (S = 4 / 8 chosen) 0.22 ms f32 and 0.18 ms with the f16 head, against 0.48 / 0.58 at 1 and
          0.52 / 0.44 for the loop under (8, 8); a 256^2 frame picks 1 and runs as before.
        Next to the frame, all opt-in (csrc/lz_ngp_frame.hip: lz_ngp_frame_render_opts / lz_ngp_frame_finish; with none in use the
        launches are those of before):
          tiles of ONE frame under cap "reference": `frame_rays_total` (the frame's ray count) and `cap_exchange` (a callable that sums
            the [max_steps + 1] int32 histogram over the tiles in place) -- dist.ShardedFrame.configure sets both -- or fused_begin /
            fused_finish around the caller's own sum.  A ray alive at the cap receives C_eff samples of the FRAME-wide schedule; a tile
            rendered on its own replays the schedule with its own ray counts and differs on exactly those rays.  With these the tiles
            are the frame's pixels, sums and counts on every ray, whatever steps_per_pass each tile runs at.
          `clip_to_occupancy` (default False; constructor argument and attribute), `occupancy_margin`, occupied_bounds(),
            invalidate_occupancy(): TriplaneRenderer's -- the march confined to the box of the occupied cells, the same samples bit
            for bit (256^2 ellipsoid frame 0.286 -> 0.258 ms; all-ones occupancy: no difference).
          render(..., perturb=True[, noises=u]) and render(..., rgb24=True): both modes, the same bits in both."""

    STEPS_PER_PASS = (0, 1, 2, 4, 8, 16)
    FusedDescriptor = _lib.FrameNgpFused

    def __init__(self, net, density_bitfield, bound=1.0, cascade=None, grid_size=128, aabb=None, min_near=0.05, budget_factor=1, n_step_cap=8,
                 mode="loop", cap="reference", steps_per_pass=1, clip_to_occupancy=False):
        super().__init__(density_bitfield, bound, cascade, grid_size, aabb, min_near, budget_factor, n_step_cap, mode, cap, chunk=4,
                         clip_to_occupancy=clip_to_occupancy)
        self.steps_per_pass = self._checked_steps_per_pass(steps_per_pass)
        if mode == "loop" and steps_per_pass != 1:
            raise ValueError("steps_per_pass is the fused mode's launch shape: mode 'loop' has its own schedule (budget_factor, n_step_cap)")
        if mode == "loop" and clip_to_occupancy:
            raise ValueError("clip_to_occupancy belongs to mode 'fused': the loop's march kernels test every cell")
        if mode == "fused" and cap == "reference" and int(n_step_cap) != 8:
            raise ValueError("mode 'fused' with cap 'reference' replays the schedule with the reference's step cap: n_step_cap must be 8")
        self.net = net

    def _checked_steps_per_pass(self, spp):
        if isinstance(spp, bool) or spp not in self.STEPS_PER_PASS:
            raise ValueError("steps_per_pass must be 0 (auto), 1, 2, 4, 8 or 16, not %r" % (spp,))
        return int(spp)

    @staticmethod
    def _check_ray_count(N):
        if N > MAX_RAYS_PER_PASS:
            raise RuntimeError("HashgridRenderer renders at most %d rays per call" % MAX_RAYS_PER_PASS)

    def _loop_extras(self, N, rows, dev):
        return dict(feats=torch.zeros(rows, 32, dtype=self.net.table.dtype, device=dev))

    @torch.no_grad()
    def render(self, rays_o, rays_d, dt_gamma=1.0 / 256, max_steps=128, T_thresh=1e-4, bg_color=1.0, count_samples=False, rgb24=False,
               perturb=False, noises=None):
        """-> dict(image [N,3] blended + clamped, image_raw, weights_sum, depth, state, ray_counts if requested, image_rgb24 [N,3] uint8
        with rgb24: the video pipe's hand-off format, quantised on the device); ready in stream order.
        perturb: the reference's inference loop passes `perturb` to march_rays on its FIRST iteration only (renderer.py:344,521), where
        every ray's start moves by clamp(near * dt_gamma, dt_min, dt_max) * U[0,1) (raymarching.cu:873).  `noises` [N] supplies the draws
        (tests; default torch.rand like raymarching.py:298).  Both modes, the same bits."""
        rays_o, rays_d, N, dev, noises = self._rays(rays_o, rays_d, perturb, noises)
        self._check_ray_count(N)
        tile = self.mode == "fused" and self.cap == "reference" and self.frame_rays_total is not None
        if N == 0 and not tile:       # (an empty tile of a larger frame still takes part in the exchange of the histogram)
            return _empty_result(dev, count_samples, rgb24, ambient=False)
        if self.mode == "fused":
            return self._render_fused(rays_o, rays_d, dt_gamma, max_steps, T_thresh, bg_color, count_samples, rgb24, noises)
        b = self._buffers(N, dev)
        self._begin(b, rays_o, rays_d, N, dt_gamma, max_steps, count_samples, noises)
        net, e = self.net, self.net.encoder
        f = self._fill_loop(_lib.FrameNgp(), b, rays_o, rays_d, N, dt_gamma, max_steps, T_thresh, count_samples)
        f.packed, f.embeddings, f.offsets, f.feats = net.packed.data_ptr(), net.table.data_ptr(), net.offsets.data_ptr(), b["feats"].data_ptr()
        f.enc_L, f.enc_H, f.enc_S, f.emb_f16 = e.num_levels, e.base_resolution, net.S, int(net.half_tables)
        if net.precision == "f16":
            enqueue = lambda k, n: call("lz_ngp_loop_run_f16", C.byref(f), ptr(net.packed16), k & 1, n, stream())
        else:
            enqueue = lambda k, n: call("lz_ngp_loop_run", C.byref(f), k & 1, n, stream())
        # n_step >= 1: max_steps iterations suffice; the state of iteration k is committed by iteration k + 1's launches
        self._poll(b, enqueue, int(max_steps) + 1, self.chunk, self.lookahead)
        return self._finish(b, N, dev, bg_color, count_samples, rgb24, (rays_o, rays_d, noises))

    # ---- the whole frame as one persistent kernel (csrc/lz_ngp_frame.hip, csrc/lz_ngp_frame_spp.hip) ----
    @property
    def last_steps_per_pass(self):
        """samples per ray and pass of the last fused frame (what steps_per_pass = 0 chose); None before the first.  Reads the frame's
        state buffer: waits for the frame."""
        if self._fbuf is None:
            return None
        return int(self._fbuf["state"][13]) or 1      # LZNF_SPP: written by the S > 1 kernels, 0 after the S = 1 kernels

    def _fused_extras(self, N, dev):
        return dict(scratch=torch.empty(N, dtype=torch.float32, device=dev))

    def fused_begin(self, rays_o, rays_d, dt_gamma=1.0 / 256, max_steps=128, T_thresh=1e-4, bg_color=1.0, count_samples=False, rgb24=False,
                    noises=None):
        """Fused mode in two calls, for callers that render tiles of ONE frame under cap = "reference" (TriplaneRenderer.fused_begin's
        contract): with `frame_rays_total` set to the frame's ray count, fused_begin enqueues phase 1 and the histogram of the rays' last
        surviving chunk boundary -- ctx["hist"], int32 [max_steps + 1] on the device; the caller sums it over all tiles of the frame, in
        place -- and fused_finish(ctx) enqueues the schedule replay (ray budget frame_rays_total * budget_factor), phase 2 and the count
        fix-up and returns the result dict.  The tiles then hold the whole frame's pixels on every ray, whatever steps_per_pass each ran
        at.  With frame_rays_total unset (a whole frame) and for cap = "per_ray" everything happens in fused_begin."""
        if self.mode != "fused":
            raise RuntimeError("fused_begin / fused_finish belong to mode 'fused'")
        self._checked_steps_per_pass(self.steps_per_pass)
        self._check_ray_count(rays_o.reshape(-1, 3).shape[0])
        return self._fused_begin(rays_o, rays_d, (), dt_gamma, max_steps, T_thresh, bg_color, count_samples, rgb24, noises)

    def _cap_total(self, N, total):
        # the ray budget of the schedule the loop runs (renderer.py:513 with budget_factor = 1), of the whole frame for a tile
        return (N if total is None else total) * self.budget_factor, total is not None

    def _fused_launch(self, ctx, opts, cond):
        f, net, e = ctx["f"], self.net, self.net.encoder
        p = lambda t: None if t is None else t.data_ptr()
        f.precision = 1 if net.precision == "f16" else 0
        f.packed, f.packed16 = p(net.packed), p(net.packed16)
        f.embeddings, f.offsets, f.emb_f16 = p(net.table), p(net.offsets), int(net.half_tables)
        f.enc_L, f.enc_H, f.enc_S = e.num_levels, e.base_resolution, net.S
        f.scratch = p(ctx["b"]["scratch"])
        # the options next to the frame: none in use -> no record, and the call is lz_ngp_frame_render_spp launch for launch
        o = None
        if opts:
            o = _lib.FrameNgpFusedOpts()
            for k, v in opts.items():
                setattr(o, k, v)
        ctx.update(o=o, spp=int(self.steps_per_pass))
        call("lz_ngp_frame_render_opts", C.byref(f), None if o is None else C.byref(o), ctx["spp"], None, stream())

    def _fused_finish_launch(self, ctx):
        call("lz_ngp_frame_finish", C.byref(ctx["f"]), C.byref(ctx["o"]), ctx["spp"], stream())
