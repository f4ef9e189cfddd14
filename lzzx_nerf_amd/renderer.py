"""Device-resident triplane renderer: the thin counterpart of NeRFRenderer.run_cuda_for_inference
(/root/reference/nerf_triplane/renderer.py:406-570) used by bench.py and the parity tests.

Same algorithm and iteration schedule as the reference loop -- per iteration: march n_step samples for every
alive ray, evaluate the head, composite, drop dead rays, n_step = max(min(N // n_alive, 8), 1), stop at
max_steps -- but (n_alive, n_step, step) live in device memory (lz_loop_state), compaction is an
order-preserving device scan, and the host never synchronises inside a frame: it enqueues iterations in chunks
and peeks at a pinned copy of the state between chunks to stop early.  The reference's own renderer keeps
working unmodified through the drop-in operators; this class is what removes its per-iteration host sync
(38 % of its loop time) and ~20 launches per iteration.

RayRenderer holds the host-side frame loop that TriplaneRenderer, NetworkRenderer and ngp.HashgridRenderer share; each of them adds its
network, its descriptors' own fields and its C calls.
"""
import ctypes as C
import math
import os

import torch

from . import _lib
from ._util import call, ptr, stream
from .head import FusedTriplaneHead
from .utils import frame_rays   # noqa: F401  (full-image rays of one pose; utils.get_rays has the reference's signature)

_STATE_INTS = 80         # LZ_LOOP_STATE_INTS: lz_loop_state (8 ints) + 64 sample-count slots + statistics
STAT_ROWS = 72           # LZ_LOOP_STAT_ROWS: sample rows handed to the head (exhausted rows included)
MAX_RAYS_PER_PASS = 4096 * 256   # lz_loop_march sums at most 4096 workgroup counts
_N_SAMPLES_OFF = (74 + 2) * 4   # LZ_LOOP_NEXT + 2: n_samples of the iteration in flight (the head's `count`)
_SPLIT_CAP = bool(os.environ.get("LZ_FRAME_SPLIT_CAP"))

get_rays = frame_rays   # round-1 name, kept for callers of (pose, intrinsics, H, W) -> (rays_o, rays_d)


def _empty_result(device, count_samples=False, rgb24=False, ambient=True):
    """what the loops return for a batch of no rays (a rank whose tile of a small frame is empty): empty outputs, a finished state"""
    z = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=device)
    state = torch.zeros(1024, dtype=torch.int32, device=device)
    state[3] = 1
    res = dict(image=z(0, 3), image_raw=z(0, 3), weights_sum=z(0), depth=z(0), state=state, nears=z(0), fars=z(0))
    if ambient:
        res.update(amb_aud_sum=z(0), amb_eye_sum=z(0), uncertainty_sum=z(0))
    if count_samples:
        res["ray_counts"] = torch.empty(0, dtype=torch.int32, device=device)
    if rgb24:
        res["image_rgb24"] = torch.empty(0, 3, dtype=torch.uint8, device=device)
    return res


def _ambient_buffers(N, rows, dev):
    """the per-ray sums and per-sample rows of the triplane head's ambient and uncertainty outputs (lz_loop_composite takes them)"""
    z = lambda *shape: torch.zeros(*shape, dtype=torch.float32, device=dev)
    return dict(amb_aud_sum=z(N), amb_eye_sum=z(N), unc_sum=z(N), amb_aud=z(rows, 1), amb_eye=z(rows, 1), unc=z(rows, 1))


class RayRenderer:
    """The host side of a frame, once, for every renderer of this package: construction (mode, cap, box, occupancy grid, schedule, tile and
    occupancy attributes), ray and noise preparation, the loop's buffers, prologue, descriptor and look-ahead poll, the background rule,
    the final blend and the result dict, and the fused frame's buffers, descriptor and two-call protocol.  A subclass supplies its
    network: the extra buffers (_loop_extras, _fused_extras), its descriptors' own fields and its C calls (_fused_launch,
    _fused_finish_launch), and its own `render` / `fused_begin` signatures."""

    AABB_Y = 1.0             # y extent of the default aabb, in units of `bound`
    RESULT = (("image", "out"), ("image_raw", "image"), ("weights_sum", "weights_sum"), ("depth", "depth"), ("state", "state"))   # result key, buffer
    RESULT_EXTRA = ()
    FusedDescriptor = None   # the ctypes mirror of the fused frame's descriptor

    def __init__(self, density_bitfield, bound, cascade, grid_size, aabb, min_near, budget_factor, n_step_cap, mode="loop", cap="reference",
                 chunk=8, clip_to_occupancy=False):
        if mode not in ("loop", "fused"):
            raise ValueError("mode must be 'loop' or 'fused', not %r" % (mode,))
        if cap not in ("reference", "per_ray"):
            raise ValueError("cap must be 'reference' or 'per_ray', not %r" % (cap,))
        self.mode, self.cap = mode, cap
        # fused mode, cap "reference", when this renderer draws a TILE of a frame: the frame's ray count (the N of renderer.py:513) and a
        # callable that sums the [max_steps + 1] int32 histogram over the ranks in place (dist.ShardedFrame.configure sets both)
        self.frame_rays_total = None
        self.cap_exchange = None
        self.bound = float(bound)
        self.cascade = cascade if cascade is not None else 1 + math.ceil(math.log2(bound))  # renderer.py:93
        self.grid_size = grid_size
        self.bitfield = density_bitfield.contiguous()
        dev = self.bitfield.device
        if aabb is None:
            y = bound * self.AABB_Y
            aabb = torch.tensor([-bound, -y, -bound, bound, y, bound], dtype=torch.float32, device=dev)
        self.aabb = aabb.to(dev, torch.float32).contiguous()
        self.min_near = float(min_near)
        # iteration schedule n_step = max(min(budget_factor * N // n_alive, n_step_cap), 1); (1, 8) is the reference's
        # (renderer.py:513).  A larger budget trades HBM (288 GB here) for fewer, fatter iterations; pixels are unchanged.
        self.budget_factor, self.n_step_cap = int(budget_factor), int(n_step_cap)
        self.chunk = chunk   # iterations enqueued per C call
        self.lookahead = 2   # chunks the host keeps queued ahead of the one whose result it inspects (the ring holds lookahead + 2)
        self._buf = self._fbuf = self._keep = None
        # fused mode: confine every ray's march to the bounds of the occupied cells (lz_occupied_bounds, recomputed when the bitfield
        # tensor changes): same samples, bit for bit, without a cell test per empty cell in front of / behind the object
        self.clip_to_occupancy = bool(clip_to_occupancy)
        self.occupancy_margin = 8      # cells; see occupied_bounds()
        self._occ = None

    def occupied_bounds(self):
        """device tensor [6]: world-space box of the occupied cells of `self.bitfield`, dilated by `occupancy_margin` cells of each level's own size and by
        at least four of the march's longest steps (dt_max = sqrt(3) cells of the outermost level), so that the march walks its last steps
        in front of the first occupied cell with its ordinary cell tests.  Cached per (tensor object, version): an in-place update of the bitfield through torch or through this package
        (occupancy.update_density_grid, raymarching.packbits into a supplied bitfield: both bump the version) recomputes it; code that writes
        the bitfield through its raw pointer by other means calls invalidate_occupancy()."""
        bf = self.bitfield
        # the entry holds the tensor itself: identity (not the address, which the caching allocator hands to the next bitfield of the same
        # size) plus the version counter.  Inference tensors (created under torch.inference_mode, e.g. a checkpoint loaded inside a serving
        # loop) track no version: they are rescanned every frame (two small launches)
        version = None if bf.is_inference() else bf._version
        hit = (self._occ is not None and version is not None and self._occ[0] is bf and self._occ[1] == (version, self.occupancy_margin, self.cascade,
                                                                                                      self.grid_size, self.bound))
        if not hit:
            box = torch.empty(6, dtype=torch.float32, device=bf.device)
            ws = torch.empty(48, dtype=torch.int32, device=bf.device)
            call("lz_occupied_bounds", ptr(bf), int(self.cascade), int(self.grid_size), self.bound, int(self.occupancy_margin), ptr(ws), ptr(box), stream())
            self._occ = (bf, (version, self.occupancy_margin, self.cascade, self.grid_size, self.bound), box, ws)
        return self._occ[2]

    def invalidate_occupancy(self):
        """forget the cached bounds of the occupied cells (the next fused frame rescans the bitfield)"""
        self._occ = None

    @staticmethod
    def _rays(rays_o, rays_d, perturb=False, noises=None):
        """-> (rays_o [N,3], rays_d [N,3], N, device, noises [N] or None): contiguous f32; perturb without noises draws them"""
        rays_o = rays_o.reshape(-1, 3).float().contiguous()
        rays_d = rays_d.reshape(-1, 3).float().contiguous()
        N, dev = rays_o.shape[0], rays_o.device
        if perturb and noises is None:
            noises = torch.rand(N, dtype=torch.float32, device=dev)
        if noises is not None:
            noises = noises.reshape(-1).to(dev, torch.float32).contiguous()
            if noises.numel() != N:
                raise RuntimeError("noises must hold one value per ray")
        return rays_o, rays_d, N, dev, noises

    @staticmethod
    def _background(bg_color, N, dev):
        """-> (bg [N,3] or None, bg_scalar): a tensor background is expanded to one colour per ray, a number stays a number"""
        if torch.is_tensor(bg_color):
            return bg_color.to(dev, torch.float32).expand(N, 3).contiguous(), 1.0
        return None, float(bg_color)

    def _result(self, b, count_samples, rgb24):
        res = {key: b[name] for key, name in self.RESULT + self.RESULT_EXTRA}
        if count_samples:
            res["ray_counts"] = b["ray_counts"]
        if rgb24:
            res["image_rgb24"] = b["out_rgb24"]
        return res

    # ---- mode "loop": the reference's iteration structure, the state on the device ----
    def _loop_extras(self, N, rows, dev):
        """the subclass's own loop buffers: name -> tensor"""
        return {}

    def _buffers(self, N, dev):
        rows = max(N * self.budget_factor, N)   # n_alive * n_step <= rows = max(sample budget, N) always (renderer.py:513 with budget = N)
        b = self._buf
        if b is None or (b["N"], b["rows"], b["dev"]) != (N, rows, dev):
            f = dict(dtype=torch.float32, device=dev)
            i = dict(dtype=torch.int32, device=dev)
            # rows no march has written yet may be evaluated too (NetworkRenderer, the hash-grid gather): they hold finite positions
            b = self._buf = dict(N=N, rows=rows, dev=dev, nears=torch.empty(N, **f), fars=torch.empty(N, **f), rays_alive=[torch.empty(N, **i), torch.empty(N, **i)],
                                 rays_t=torch.empty(N, **f), weights_sum=torch.empty(N, **f), depth=torch.empty(N, **f), image=torch.empty(N, 3, **f),
                                 out=torch.empty(N, 3, **f), out_rgb24=None, xyzs=torch.zeros(rows, 3, **f), dirs=torch.zeros(rows, 3, **f),
                                 deltas=torch.zeros(rows, 2, **f), sigmas=torch.empty(rows, **f), rgbs=torch.empty(rows, 3, **f),
                                 state=torch.zeros(_STATE_INTS, **i), workspace=torch.empty(4096, **i), ray_counts=torch.zeros(N, **i),
                                 ring=[torch.zeros(8, dtype=torch.int32).pin_memory() for _ in range(4)], **self._loop_extras(N, rows, dev))
        return b

    def _begin(self, b, rays_o, rays_d, N, dt_gamma, max_steps, count_samples, noises=None):
        """the loop's prologue: near / far, the (perturbed) starts, the initial state; the ambient sums are the subclass's own or NULL"""
        call("lz_near_far_from_aabb", ptr(rays_o), ptr(rays_d), ptr(self.aabb), N, self.min_near, ptr(b["nears"]), ptr(b["fars"]), stream())
        if count_samples:
            b["ray_counts"].zero_()
        starts = b["nears"]
        if noises is not None:   # the loop's first march starts every ray at its perturbed t (the kernel copies `starts` into rays_t)
            starts = torch.empty_like(b["nears"])
            call("lz_perturb_starts", ptr(b["nears"]), ptr(noises), float(dt_gamma), int(max_steps), int(self.cascade), int(self.grid_size), N, ptr(starts), stream())
        call("lz_loop_begin", N, int(max_steps), N * self.budget_factor, self.n_step_cap, ptr(starts), ptr(b["rays_alive"][0]), ptr(b["rays_t"]), ptr(b["weights_sum"]),
             ptr(b["depth"]), ptr(b["image"]), ptr(b.get("amb_aud_sum")), ptr(b.get("amb_eye_sum")), ptr(b.get("unc_sum")), ptr(b["state"]), ptr(b["workspace"]), stream())

    def _fill_loop(self, f, b, rays_o, rays_d, N, dt_gamma, max_steps, T_thresh, count_samples):
        """the fields lz_frame and lz_frame_ngp share (_lib.Frame, _lib.FrameNgp)"""
        p = lambda t: t.data_ptr()
        for k in ("state", "workspace", "rays_t", "nears", "fars", "xyzs", "dirs", "deltas", "sigmas", "rgbs", "weights_sum", "depth", "image"):
            setattr(f, k, p(b[k]))
        f.rays_alive[0], f.rays_alive[1] = p(b["rays_alive"][0]), p(b["rays_alive"][1])
        f.rays_o, f.rays_d, f.grid = p(rays_o), p(rays_d), p(self.bitfield)
        f.ray_counts = p(b["ray_counts"]) if count_samples else None
        f.N, f.max_steps, f.C, f.H = N, int(max_steps), int(self.cascade), int(self.grid_size)
        f.bound, f.dt_gamma, f.T_thresh = self.bound, float(dt_gamma), float(T_thresh)
        f.sample_budget, f.n_step_cap = N * self.budget_factor, self.n_step_cap
        return f

    def _march(self, b, cur, rays_o, rays_d, N, dt_gamma, max_steps, count_samples):
        """one iteration driven from Python, first half: compaction of list[cur] -> list[1 - cur], fused with the march of the survivors"""
        call("lz_loop_march", ptr(b["state"]), N, N * self.budget_factor, self.n_step_cap, ptr(b["rays_alive"][cur]), ptr(b["rays_alive"][1 - cur]),
             ptr(b["workspace"]), ptr(b["rays_t"]), ptr(rays_o), ptr(rays_d), self.bound, float(dt_gamma), int(max_steps), int(self.cascade),
             int(self.grid_size), ptr(self.bitfield), ptr(b["nears"]), ptr(b["fars"]), ptr(b["xyzs"]), ptr(b["dirs"]), ptr(b["deltas"]),
             ptr(b["ray_counts"]) if count_samples else None, stream())

    def _composite(self, b, cur, N, T_thresh):
        """... second half, behind the network: composite the samples of list[1 - cur]"""
        call("lz_loop_composite", ptr(b["state"]), N, float(T_thresh), ptr(b["rays_alive"][1 - cur]), ptr(b["rays_t"]), ptr(b["sigmas"]), ptr(b["rgbs"]),
             ptr(b["deltas"]), ptr(b["amb_aud"]), ptr(b["amb_eye"]), ptr(b["unc"]), ptr(b["weights_sum"]), ptr(b["depth"]), ptr(b["image"]),
             ptr(b["amb_aud_sum"]), ptr(b["amb_eye_sum"]), ptr(b["unc_sum"]), ptr(b["workspace"]), stream())

    def _poll(self, b, enqueue, limit, chunk, lookahead):
        """enqueue(k, n) enqueues units k .. k + n - 1 (iterations; NetworkRenderer: pairs of them), `chunk` at a time and `limit` at most.
        After every chunk the loop state is copied to a pinned slot (a ring) behind an event.  Before enqueuing more, the host looks at
        the chunk `lookahead` chunks back: the GPU always has that many chunks queued (no bubble), and at most that many no-op chunks
        are enqueued after the frame has finished."""
        ring, pending, it = b["ring"], [], 0
        while it < limit:
            n = min(chunk, limit - it)
            enqueue(it, n)
            it += n
            k = len(pending)
            slot = ring[k % len(ring)]
            slot.copy_(b["state"][:8], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            pending.append((ev, slot))
            if k >= lookahead:
                ev_old, slot_old = pending[k - lookahead]
                ev_old.synchronize()
                if int(slot_old[3]) == 1:
                    break

    def _finish(self, b, N, dev, bg_color, count_samples, rgb24, keep):
        """the final blend over the background (+ RGB24, the video pipe's hand-off format, quantised on device: TrainerUtil.py:550-555)
        and the result dict; `keep` and the background stay referenced until the next frame"""
        bg, bg_scalar = self._background(bg_color, N, dev)
        if rgb24:
            if b["out_rgb24"] is None:
                b["out_rgb24"] = torch.empty(N, 3, dtype=torch.uint8, device=dev)
            call("lz_final_blend_rgb24", ptr(b["image"]), ptr(b["weights_sum"]), ptr(bg), bg_scalar, N, ptr(b["out"]), ptr(b["out_rgb24"]), stream())
        else:
            call("lz_final_blend", ptr(b["image"]), ptr(b["weights_sum"]), ptr(bg), bg_scalar, N, ptr(b["out"]), stream())
        self._keep = (bg,) + tuple(keep)
        return self._result(b, count_samples, rgb24)

    # ---- mode "fused": the whole frame as one persistent kernel ----
    def _fused_extras(self, N, dev):
        """the subclass's own fused-frame buffers: name -> tensor"""
        return {}

    def _fused_buffers(self, N, dev):
        b = self._fbuf
        if b is None or b["N"] != N or b["dev"] != dev:
            f = dict(dtype=torch.float32, device=dev)
            i = dict(dtype=torch.int32, device=dev)
            b = self._fbuf = dict(N=N, dev=dev, nears=torch.empty(N, **f), fars=torch.empty(N, **f), rays_t=torch.empty(N, **f), order=torch.empty(N, **i),
                                  state=torch.zeros(1024, **i), keys=torch.empty(N, dtype=torch.uint8, device=dev), weights_sum=torch.empty(N, **f),
                                  depth=torch.empty(N, **f), image=torch.empty(N, 3, **f), out=torch.empty(N, 3, **f), ray_counts=None,
                                  ray_last=torch.empty(N, **i), cap_ws=None, t_end=None, out_rgb24=None)
            b.update(self._fused_extras(N, dev))
        return b

    def _render_fused(self, *args):
        """a fused frame in one go; `args` are fused_begin's"""
        ctx = self.fused_begin(*args)
        if ctx["deferred"] and self.cap_exchange is not None:
            self.cap_exchange(ctx["hist"])
        return self.fused_finish(ctx)

    def _cap_applies(self, count_samples, dt_gamma, max_steps):
        """cap "reference": does this frame need the schedule replay at all?"""
        return True

    def _cap_total(self, N, total):
        """cap "reference" -> (N_total of the descriptor, defer_finish) for N rays of a frame of `total` rays (None: a whole frame)"""
        raise NotImplementedError

    def _fused_launch(self, ctx, opts, cond):
        """fill the rest of ctx["f"] -- the network, `opts` (name -> value of every option in use: noises, occupied_aabb, t_end, out_rgb24,
        defer_finish) -- and make the C call that renders the frame"""
        raise NotImplementedError

    def _fused_finish_launch(self, ctx):
        """the C call that finishes a deferred frame"""
        raise NotImplementedError

    def _fused_begin(self, rays_o, rays_d, cond, dt_gamma, max_steps, T_thresh, bg_color, count_samples, rgb24, noises):
        """what the subclasses' fused_begin share; `cond`: the network's per-frame tensors, kept alive with the rays"""
        rays_o, rays_d, N, dev, noises = self._rays(rays_o, rays_d, noises=noises)
        b = self._fused_buffers(N, dev)
        bg, bg_scalar = self._background(bg_color, N, dev)
        p = lambda t: None if t is None else t.data_ptr()
        f = self.FusedDescriptor()
        # the fields lz_frame_fused and lz_frame_ngp_fused share (_lib.FrameFused, _lib.FrameNgpFused)
        f.rays_o, f.rays_d, f.grid, f.aabb = p(rays_o), p(rays_d), p(self.bitfield), p(self.aabb)
        for k in ("nears", "fars", "rays_t", "order", "state", "keys", "weights_sum", "depth", "image", "out"):
            setattr(f, k, p(b[k]))
        f.bg, f.bg_scalar = p(bg), bg_scalar
        if count_samples:
            if b["ray_counts"] is None:
                b["ray_counts"] = torch.zeros(N, dtype=torch.int32, device=dev)
            f.ray_counts = p(b["ray_counts"])
        f.bound, f.dt_gamma, f.T_thresh, f.min_near = self.bound, float(dt_gamma), float(T_thresh), self.min_near
        f.N, f.max_steps, f.C, f.H = N, int(max_steps), int(self.cascade), int(self.grid_size)
        opts, deferred = {}, False
        if noises is not None:
            opts["noises"] = p(noises)
        if self.clip_to_occupancy:
            if b["t_end"] is None:
                b["t_end"] = torch.empty(N, dtype=torch.float32, device=dev)
            opts["occupied_aabb"], opts["t_end"] = p(self.occupied_bounds()), p(b["t_end"])
        if rgb24:
            if b["out_rgb24"] is None:
                b["out_rgb24"] = torch.empty(N, 3, dtype=torch.uint8, device=dev)
            opts["out_rgb24"] = p(b["out_rgb24"])
        if self.cap == "reference" and self._cap_applies(count_samples, dt_gamma, max_steps):
            need = 2 * int(max_steps) + 24            # LZ_FRAME_CAP_WS_INTS
            if b["cap_ws"] is None or b["cap_ws"].numel() < need:
                b["cap_ws"] = torch.zeros(need, dtype=torch.int32, device=dev)
            f.cap_mode, f.ray_last, f.cap_ws = 1, p(b["ray_last"]), p(b["cap_ws"])
            total = self.frame_rays_total
            if total is not None and int(total) < N:
                raise ValueError("frame_rays_total is the ray count of the whole frame (>= the rays of this call)")
            f.N_total, deferred = self._cap_total(N, None if total is None else int(total))
            if deferred:
                opts["defer_finish"] = 1
        self._keep = keep = (bg, rays_o, rays_d, noises) + tuple(cond)
        ctx = dict(f=f, b=b, keep=keep, deferred=deferred, count_samples=count_samples, rgb24=rgb24,
                   hist=b["cap_ws"][: int(max_steps) + 1] if deferred else None)
        self._fused_launch(ctx, opts, cond)
        return ctx

    def fused_finish(self, ctx):
        if ctx["deferred"]:
            self._fused_finish_launch(ctx)
        return self._result(ctx["b"], ctx["count_samples"], ctx["rgb24"])


class TriplaneRenderer(RayRenderer):
    """Inference renderer for one head / one occupancy grid.

    head:             FusedTriplaneHead
    density_bitfield: uint8 [cascade * grid_size^3 / 8] (cuda), as produced by raymarching.packbits
    """

    AABB_Y = 0.5             # renderer.py:110 -- y extent halved
    RESULT_EXTRA = (("amb_aud_sum", "amb_aud_sum"), ("amb_eye_sum", "amb_eye_sum"), ("uncertainty_sum", "unc_sum"), ("nears", "nears"), ("fars", "fars"))
    FusedDescriptor = _lib.FrameFused

    def __init__(self, head: FusedTriplaneHead, density_bitfield, bound=1.0, cascade=None, grid_size=128, aabb=None,
                 min_near=0.05, density_scale=1, budget_factor=1, n_step_cap=8, mode="loop", cap="reference"):
        """mode "loop": the reference's iteration structure, 3 launches per iteration (march, head, composite), schedule
        (budget_factor, n_step_cap).  mode "fused": the whole frame as one persistent kernel (csrc/lz_frame.hip) with on-the-fly refill of
        finished ray slots; `steps_per_pass` (0 = chosen from the ray count: 1 for a whole frame, up to 16 for small tiles) is its launch shape.
        Cap semantics: the reference tests `step < max_steps` once per ITERATION (renderer.py:503-548) with n_step = max(min(N // n_alive, 8), 1),
        so every ray still alive at the cap has received the same frame-wide C_eff = sum of n_step samples, in [max_steps, max_steps + 7]
        (the deployed max_steps = 16 binds on most foreground rays).
          cap = "reference" (default): fused mode reproduces exactly that -- phase 1 to max_steps, a device-side replay of the schedule from
            a histogram over the rays, phase 2 to C_eff -- and equals the loop under the reference schedule (1, 8) bit for bit: pixels, depth,
            sums and, with count_samples, per-ray marched counts.  A tile of a larger frame passes the frame's ray count and a histogram
            exchange (dist.ShardedFrame.configure does both) and then equals the unsharded frame.
          cap = "per_ray": a ray alive at the cap stops at ceil(max_steps / S) * S samples, S = steps_per_pass -- the loop under the
            schedule (budget_factor, n_step_cap) = (S, S); one launch less, no exchange between ranks, NOT the reference's pixels on rays
            that reach the cap.
        Every ray that leaves the box or falls under T_thresh before max_steps -- all rays of the 512^2 / 192-step headline frame -- is
        the same under both."""
        super().__init__(density_bitfield, bound, cascade, grid_size, aabb, min_near, budget_factor, n_step_cap, mode, cap, chunk=8,
                         clip_to_occupancy=True)
        if density_scale != 1:
            raise NotImplementedError("density_scale != 1 (the reference hard-codes 1, renderer.py:95)")
        self.steps_per_pass = 0    # fused mode: samples per ray and pass (0 = auto by ray count; 1, 2, 4, 8, 16 = the schedule n_step it equals)
        self.head = head
        self._aabb_diag = None      # (tensor, version, diagonal): see _cap_can_bind
        self._head_events = None  # set to a list: Python-driven loop with torch events around every head launch (debug)
        self._timing = None       # lz_timing handle: native loop records a HIP event pair around every head launch

    def _cap_can_bind(self, dt_gamma, max_steps):
        """False when no ray can collect max_steps samples, so the cap -- and with it the iteration schedule -- cannot touch any pixel: a
        ray's samples lie inside the aabb, at most its diagonal D apart, and consecutive samples are at least dt_min = min(dt_max, 2 sqrt(3) /
        max_steps) apart (raymarching.cu:866-867, 907), so a ray holds at most D / dt_min + 1 of them.  The reference's own aabb (y extent
        halved, renderer.py:110: D = 3 bound < 2 sqrt(3) bound) never reaches the cap once dt_min = 2 sqrt(3) / max_steps, e.g. the 192-step
        headline frame; its deployed max_steps = 16 (dt_min = dt_max) does.  The diagonal is read back once per aabb tensor."""
        a = self.aabb
        ver = None if a.is_inference() else a._version
        if self._aabb_diag is None or self._aabb_diag[0] is not a or self._aabb_diag[1] != ver or ver is None:
            lo_hi = a.detach().cpu().double()
            self._aabb_diag = (a, ver, float(((lo_hi[3:] - lo_hi[:3]) ** 2).sum().sqrt()))
        dt_max = 2 * math.sqrt(3) * (1 << (int(self.cascade) - 1)) / int(self.grid_size)
        dt_min = min(dt_max, 2 * math.sqrt(3) / max(int(max_steps), 1))
        return self._aabb_diag[2] / dt_min + 2 >= int(max_steps)

    def timing_start(self, n_pairs):
        """bracket every head launch of the following render() calls with HIP events (bench.py's roofline leg)"""
        h = C.c_void_p()
        call("lz_timing_create", int(n_pairs), C.byref(h))
        self._timing = h

    def timing_stop(self):
        """-> list of head-launch durations in ms (synchronises the device)"""
        torch.cuda.synchronize()
        h, self._timing = self._timing, None
        cap = 1 << 20
        buf = (C.c_float * cap)()
        n = C.c_uint32()
        call("lz_timing_elapsed_ms", h, buf, cap, C.byref(n))
        out = list(buf[: n.value])
        call("lz_timing_destroy", h)
        return out

    def _loop_extras(self, N, rows, dev):
        return _ambient_buffers(N, rows, dev)

    def _conditioning(self, enc_a, ind_code, eye):
        """the small conditioning tensors as the head's descriptor reads them; kept alive on self until the next frame"""
        flat = lambda t: None if t is None else t.reshape(-1).float().contiguous()
        self._cond = (flat(enc_a), flat(ind_code), flat(eye))
        return self._cond

    def _iteration(self, b, cur, rays_o, rays_d, N, enc_a, ind_code, eye, dt_gamma, max_steps, T_thresh, count_samples):
        """one iteration of the Python-driven loop, torch events around the head"""
        self._march(b, cur, rays_o, rays_d, N, dt_gamma, max_steps, count_samples)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        self.head.forward(b["xyzs"], b["dirs"], enc_a, ind_code, eye, testing=True, count_ptr=b["state"].data_ptr() + _N_SAMPLES_OFF,
                          out=(b["sigmas"], b["rgbs"], b["amb_aud"], b["amb_eye"], b["unc"]))
        e1.record()
        self._head_events.append((e0, e1))
        self._composite(b, cur, N, T_thresh)

    def _frame(self, b, rays_o, rays_d, N, enc_a, ind_code, eye, dt_gamma, max_steps, T_thresh, count_samples):
        """lz_frame for lz_loop_run"""
        f = self._fill_loop(_lib.Frame(), b, rays_o, rays_d, N, dt_gamma, max_steps, T_thresh, count_samples)
        f.head = self.head._params(*self._conditioning(enc_a, ind_code, eye), True)
        for k in ("amb_aud", "amb_eye", "unc", "amb_aud_sum", "amb_eye_sum", "unc_sum"):
            setattr(f, k, b[k].data_ptr())
        return f

    @torch.no_grad()
    def render(self, rays_o, rays_d, enc_a, ind_code=None, eye=None, dt_gamma=1.0 / 256, max_steps=16, T_thresh=1e-4,
               bg_color=1.0, count_samples=False, sync_free=True, rgb24=False, perturb=False, noises=None):
        """rays_o, rays_d: [N,3] (or [1,N,3]) f32 cuda.  Returns dict(image [N,3] blended+clamped, weights_sum, depth,
        amb_aud_sum, amb_eye_sum, uncertainty_sum, state (device int32[8]), ray_counts if requested).
        perturb: the reference's inference loop passes `perturb` to march_rays on its FIRST iteration only (renderer.py:344,521), where
        every ray's start moves by clamp(near * dt_gamma, dt_min, dt_max) * U[0,1) (raymarching.cu:873).  `noises` [N] supplies the
        draws (tests; default torch.rand like raymarching.py:298).
        sync_free: the host never waits for the newest work, only for the chunk `lookahead` chunks back (the GPU
        queue never drains); the returned tensors are ready in stream order."""
        rays_o, rays_d, N, dev, noises = self._rays(rays_o, rays_d, perturb, noises)
        if N > MAX_RAYS_PER_PASS and self.mode != "fused":
            # rays are independent: larger batches are rendered in passes of <= 2^20 rays (the device loop scans at most 4096
            # workgroup counts per iteration) and concatenated; pixels do not depend on the split
            outs = []
            for lo in range(0, N, MAX_RAYS_PER_PASS):
                hi = min(lo + MAX_RAYS_PER_PASS, N)
                bg = bg_color[lo:hi] if torch.is_tensor(bg_color) and bg_color.dim() > 1 and bg_color.shape[0] == N else bg_color
                o = self.render(rays_o[lo:hi], rays_d[lo:hi], enc_a, ind_code, eye, dt_gamma, max_steps, T_thresh, bg, count_samples,
                                sync_free, rgb24, noises=None if noises is None else noises[lo:hi])
                outs.append({k: v.clone() for k, v in o.items()})
            res = {k: torch.cat([o[k] for o in outs], 0) for k in outs[0] if k not in ("state",)}
            st = torch.stack([o["state"] for o in outs])
            res["state"] = st[-1].clone()
            res["state"][5] = st[:, 5].sum()      # marched samples of the whole batch
            res["state"][72] = st[:, 72].sum()
            res["state"][6] = st[:, 6].max()
            return res
        if self.mode == "fused":
            return self._render_fused(rays_o, rays_d, enc_a, ind_code, eye, dt_gamma, max_steps, T_thresh, bg_color, count_samples, rgb24, noises)
        if N == 0:
            return _empty_result(dev, count_samples, rgb24)
        b = self._buffers(N, dev)
        self._begin(b, rays_o, rays_d, N, dt_gamma, max_steps, count_samples, noises)
        if self._head_events is None:   # one C call enqueues n x (march, head, composite, advance)
            frame = self._frame(b, rays_o, rays_d, N, enc_a, ind_code, eye, dt_gamma, max_steps, T_thresh, count_samples)
            enqueue = lambda k, n: call("lz_loop_run", C.byref(frame), k & 1, n, self._timing, stream())
        else:                           # the Python-driven loop is kept for debugging with torch events
            def enqueue(k, n):
                for it in range(k, k + n):
                    self._iteration(b, it & 1, rays_o, rays_d, N, enc_a, ind_code, eye, dt_gamma, max_steps, T_thresh, count_samples)
        # n_step >= 1: max_steps iterations always suffice (renderer.py:503,546); the state of iteration k is committed by iteration
        # k + 1's launches, hence one more
        self._poll(b, enqueue, int(max_steps) + 1, self.chunk, self.lookahead if sync_free else 0)
        return self._finish(b, N, dev, bg_color, count_samples, rgb24, (rays_o, rays_d, noises))

    # ---- the whole frame as one persistent kernel (csrc/lz_frame.hip) ----
    def _fused_extras(self, N, dev):
        e = lambda: torch.empty(N, dtype=torch.float32, device=dev)
        return dict(amb_aud_sum=e(), amb_eye_sum=e(), unc_sum=e(), t_end=e())

    def fused_begin(self, rays_o, rays_d, enc_a, ind_code=None, eye=None, dt_gamma=1.0 / 256, max_steps=16, T_thresh=1e-4, bg_color=1.0,
                    count_samples=False, rgb24=False, noises=None):
        """Fused mode in two calls, for callers that render tiles of ONE frame under cap = "reference": fused_begin enqueues phase 1 and the
        histogram of the rays' last surviving chunk boundary -- ctx["hist"], int32 [max_steps + 1] on the device; the caller sums it over all
        tiles of the frame, in place -- and fused_finish(ctx) enqueues the schedule replay, phase 2 and returns the result dict.  With
        frame_rays_total unset (a whole frame) and for cap = "per_ray" everything happens in fused_begin."""
        return self._fused_begin(rays_o, rays_d, self._conditioning(enc_a, ind_code, eye), dt_gamma, max_steps, T_thresh, bg_color, count_samples,
                                 rgb24, noises)

    def _cap_applies(self, count_samples, dt_gamma, max_steps):
        # the reference's cap needs the schedule replay only if some ray can reach max_steps at all (or marched counts are asked for: a
        # T_thresh-cut ray's count depends on the chunk it was cut in); otherwise the plain launch renders the same pixels
        # (ranks rendering tiles of one frame share aabb and max_steps, so they take the same branch: no histogram exchange either)
        return count_samples or self._cap_can_bind(dt_gamma, max_steps)

    def _cap_total(self, N, total):
        if total is None:      # a whole frame; LZ_FRAME_SPLIT_CAP: the two cap kernels as separate launches (a diagnostic, tools/frame_trace.sh)
            return (N, True) if _SPLIT_CAP else (0, False)
        return total, True

    def _fused_launch(self, ctx, opts, cond):
        f, b = ctx["f"], ctx["b"]
        f.head = self.head._params(*cond, True)
        f.amb_aud_sum, f.amb_eye_sum, f.unc_sum = b["amb_aud_sum"].data_ptr(), b["amb_eye_sum"].data_ptr(), b["unc_sum"].data_ptr()
        f.steps_per_pass = int(self.steps_per_pass)
        for k, v in opts.items():
            setattr(f, k, v)
        call("lz_frame_render", C.byref(f), self._timing, stream())   # timing: one event pair around the persistent kernel

    def _fused_finish_launch(self, ctx):
        call("lz_frame_finish", C.byref(ctx["f"]), stream())


class NetworkRenderer(RayRenderer):
    """The device-resident inference loop around ANY per-sample network (BASELINE cfg2: a generic hash-grid NeRF on the operator API):
    run_cuda_for_inference's iteration (renderer.py:503-548) as lz_loop_march -> net -> lz_loop_composite with the loop state in device
    memory, like TriplaneRenderer(mode="loop") -- but the network is a Python callable over torch tensors,

        net(xyzs [rows, 3], dirs [rows, 3]) -> (sigma [rows], rgb [rows, 3])

    evaluated every iteration on the WHOLE row budget (rows = budget_factor * N, static shapes): rows behind the iteration's n_alive *
    n_step samples hold older samples whose results nobody reads.  That costs a few useless rows (the budget is what the schedule
    fills while most rays are alive) and buys an iteration without a host round trip -- the reference syncs on `rays_alive[rays_alive >=
    0]` every iteration -- and with static shapes, so that a pair of iterations (the alive list ping-pongs) is captured ONCE as a hipGraph
    (torch.cuda.CUDAGraph over torch's kernels and this library's launches on the capturing stream) and replayed: the ~25 launches of an
    iteration cost one graph launch.  Pixels and per-ray sample counts equal the reference loop's on the same operators (rays are
    independent, compositing resumes exactly; tests/test_gpu_cfg2_render.py)."""

    AABB_Y = 0.5             # TriplaneRenderer's default box

    def __init__(self, net, density_bitfield, bound=1.0, cascade=None, grid_size=128, aabb=None, min_near=0.05, budget_factor=4, n_step_cap=4,
                 graph=True):
        super().__init__(density_bitfield, bound, cascade, grid_size, aabb, min_near, budget_factor, n_step_cap, chunk=8)
        self.net = net
        self.use_graph = bool(graph)
        self._graph = None        # (key, CUDAGraph) of two iterations

    def _loop_extras(self, N, rows, dev):
        # the graph holds the addresses of the ray tensors: keep them in buffers of our own
        return dict(_ambient_buffers(N, rows, dev), ro=torch.empty(N, 3, device=dev), rd=torch.empty(N, 3, device=dev))

    def _pair(self, b, N, dt_gamma, max_steps, T_thresh, count_samples):
        for cur in (0, 1):
            self._march(b, cur, b["ro"], b["rd"], N, dt_gamma, max_steps, count_samples)
            sigma, rgb = self.net(b["xyzs"], b["dirs"])
            b["sigmas"].copy_(sigma.reshape(-1))
            b["rgbs"].copy_(rgb.reshape(-1, 3))
            self._composite(b, cur, N, T_thresh)

    @torch.no_grad()
    def render(self, rays_o, rays_d, dt_gamma=1.0 / 256, max_steps=128, T_thresh=1e-4, bg_color=1.0, count_samples=False):
        """-> dict(image [N,3] blended + clamped, image_raw, weights_sum, depth, state, ray_counts if requested); ready in stream order"""
        rays_o, rays_d, N, dev, _ = self._rays(rays_o, rays_d)
        if N > MAX_RAYS_PER_PASS:
            raise RuntimeError("NetworkRenderer renders at most %d rays per call" % MAX_RAYS_PER_PASS)
        if N == 0:
            return _empty_result(dev, count_samples, ambient=False)
        prev = self._buf
        b = self._buffers(N, dev)
        if b is not prev:      # fresh buffers (also when the row budget changed: budget_factor); their rows are zero: rows no march has
            self._graph = None   # written yet are evaluated too, and the network finds finite positions there
        b["ro"].copy_(rays_o); b["rd"].copy_(rays_d)
        self._begin(b, b["ro"], b["rd"], N, dt_gamma, max_steps, count_samples)
        # everything the captured launches bake in: scalars, the addresses of the bitfield / aabb / buffers, the schedule
        key = (N, float(dt_gamma), int(max_steps), float(T_thresh), bool(count_samples), self.bitfield.data_ptr(), self.aabb.data_ptr(), self.bound,
               int(self.cascade), int(self.grid_size), self.n_step_cap, self.budget_factor, self.min_near, id(b))
        done_pairs = 0
        if self.use_graph and (self._graph is None or self._graph[0] != key):
            # capture two iterations.  The capture itself executes nothing, and torch wants the ops warmed up on a side stream first:
            # run one pair for real there (it is simply the frame's first pair), then capture
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                self._pair(b, N, dt_gamma, max_steps, T_thresh, count_samples)
            torch.cuda.current_stream().wait_stream(side)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                self._pair(b, N, dt_gamma, max_steps, T_thresh, count_samples)
            self._graph = (key, g)
            done_pairs = 1

        def enqueue(k, n):
            for _ in range(n):
                if self.use_graph:
                    self._graph[1].replay()
                else:
                    self._pair(b, N, dt_gamma, max_steps, T_thresh, count_samples)
        limit = (int(max_steps) + 2) // 2 + 1          # pairs: n_step >= 1, plus the iteration that commits the last state
        self._poll(b, enqueue, limit - done_pairs, max(self.chunk // 2, 1), self.lookahead)
        return self._finish(b, N, dev, bg_color, count_samples, False, (rays_o, rays_d))
