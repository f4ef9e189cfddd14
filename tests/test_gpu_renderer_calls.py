"""What the three renderers hand to the library, call for call: every frame goes through lzzx_nerf_amd._lib.call, which these tests replace
with a recorder that forwards to the real one.  A record is one line per call -- the entry's name and its arguments: Python scalars as
they are, a pointer as `null` or as pN (N numbers the distinct addresses of one record in order of first appearance, so a record also
says WHICH calls share a buffer: the `starts` that lz_perturb_starts writes is the one lz_loop_begin reads), a ctypes.Structure passed
by reference with every field (written out where its content first appears in the record, by its number afterwards).  Equal consecutive
lines are folded into one with a count.  The records are compared with the literals of EXPECTED below, which were taken from a run of
this file on the renderers as they were before they shared a base class (the chunk counts in them depend on the scene and are measured
numbers too); the host-side driver may be reorganised freely as long as the library sees the same calls."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import ellipsoid_bitfield, synthetic_camera

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Recorder:
    def __init__(self, monkeypatch):
        from lzzx_nerf_amd import _lib
        self.real = _lib.call
        self.lines, self.ptrs, self.structs = [], {}, {}
        monkeypatch.setattr(_lib, "call", self)

    def __call__(self, name, *args):
        self.lines.append("%s(%s)" % (name, ", ".join(self.arg(a) for a in args)))
        self.real(name, *args)

    def note(self, text):
        self.lines.append(text)

    def pointer(self, value):
        return "null" if not value else self.ptrs.setdefault(value, "p%d" % len(self.ptrs))

    def arg(self, a):
        if a is None:
            return "null"
        if hasattr(a, "_obj"):              # ctypes.byref(x)
            return self.arg(a._obj)
        if isinstance(a, C.Structure):
            text = self.fields(a)
            first = text not in self.structs
            tag = "%s#%d" % (type(a).__name__, self.structs.setdefault(text, len(self.structs)))
            return tag + text if first else tag
        if isinstance(a, C.c_void_p):
            return self.pointer(a.value)
        assert isinstance(a, (int, float)), a
        return repr(a)

    def fields(self, s):
        out = []
        for name, typ in s._fields_:
            v = getattr(s, name)
            if typ is C.c_void_p:
                v = self.pointer(v)
            elif issubclass(typ, C.Array):
                v = "(%s)" % ",".join(self.pointer(x) for x in v)
            elif issubclass(typ, C.Structure):
                v = self.fields(v)
            else:
                v = repr(v)
            out.append("%s=%s" % (name, v))
        return "{%s}" % " ".join(out)

    def take(self):
        """the record so far, folded; the next record numbers its addresses and structures afresh"""
        out = []
        for line in self.lines:
            if out and out[-1][0] == line:
                out[-1][1] += 1
            else:
                out.append([line, 1])
        self.lines, self.ptrs, self.structs = [], {}, {}
        return [line if n == 1 else "%s x%d" % (line, n) for line, n in out]


@pytest.fixture
def rec(monkeypatch):
    return Recorder(monkeypatch)


@pytest.fixture(scope="module")
def triplane(params, golden):
    """the 32 x 32 ellipsoid frame of tests/test_gpu_fused_frame.py"""
    from lzzx_nerf_amd.head import FusedTriplaneHead
    from lzzx_nerf_amd.utils import frame_rays
    head = FusedTriplaneHead({k: torch.from_numpy(v) for k, v in params.items()}, bound=1.0)
    pose, intr = synthetic_camera(32, 32)
    ro, rd = frame_rays(dev(pose), intr, 32, 32)
    cond = (dev(golden["net_enc_a"]), dev(golden["net_ind"]), dev(golden["net_eye"]))
    return dict(head=head, bits=dev(ellipsoid_bitfield()[0]), ro=ro.reshape(-1, 3).contiguous(), rd=rd.reshape(-1, 3).contiguous(), cond=cond)


@pytest.fixture(scope="module")
def hashgrid():
    """the 48 x 48 frame of tests/test_gpu_ngp_fused.py: the ellipsoid with seeded holes"""
    from lzzx_nerf_amd.ngp import FusedHashgridNeRF
    from lzzx_nerf_amd.synthetic import GenericHashgridNeRF
    from lzzx_nerf_amd.utils import frame_rays
    g = GenericHashgridNeRF(torch.device("cuda"), seed=3)
    nets = {p: FusedHashgridNeRF(g.enc, g.sigma_net, g.color_net, precision=p) for p in ("f32", "f16")}
    full = ellipsoid_bitfield()[0]
    holes = full & np.where(np.random.default_rng(5).random(full.shape) < 0.25, 0, 255).astype(full.dtype)
    pose, intr = synthetic_camera(48, 48)
    ro, rd = frame_rays(dev(pose), intr, 48, 48)
    ro, rd = ro.reshape(-1, 3).contiguous(), rd.reshape(-1, 3).contiguous()
    return dict(nets=nets, bits=dev(holes), ro=ro, rd=rd, noises=dev(np.random.default_rng(1).random(ro.shape[0], dtype=np.float32)))


def operator_net(xyzs, dirs):
    """a per-sample network of torch operators alone (NetworkRenderer's `net`): a dense ball, coloured by direction"""
    return 40.0 * (xyzs.square().sum(-1) < 0.16).float(), dirs.abs()


# ---- the cases: name -> the records of its frames -------------------------------------------------------------------------------------
def triplane_renderer(t, **kw):
    from lzzx_nerf_amd.renderer import TriplaneRenderer
    return TriplaneRenderer(t["head"], t["bits"], bound=1.0, **kw)


def triplane_loop(rec, t, prepare=None, **kw):
    r = triplane_renderer(t)
    if prepare:
        prepare(r)
    r.render(t["ro"], t["rd"], *t["cond"], max_steps=kw.pop("max_steps", 32), **kw)
    torch.cuda.synchronize()
    return rec.take()


def triplane_fused(rec, t, frames=1, tile=False, **kw):
    r = triplane_renderer(t, mode="fused", cap=kw.pop("cap", "reference"))
    n = t["ro"].shape[0]
    if tile:
        r.frame_rays_total = 2 * n
        r.cap_exchange = lambda hist: rec.note("exchange(%s %s)" % (hist.dtype, tuple(hist.shape)))
    out = []
    for _ in range(frames):
        r.render(t["ro"], t["rd"], *t["cond"], **kw)
        torch.cuda.synchronize()
        out.append(rec.take())
    return out if frames > 1 else out[0]


def hashgrid_frame(rec, h, mode, precision="f32", ctor=None, tile=None, n=None, **kw):
    from lzzx_nerf_amd.ngp import HashgridRenderer
    r = HashgridRenderer(h["nets"][precision], h["bits"], bound=1.0, mode=mode, **(ctor or {}))
    if tile is not None:
        r.frame_rays_total = tile
        r.cap_exchange = lambda hist: rec.note("exchange(%s %s)" % (hist.dtype, tuple(hist.shape)))
    ro, rd = (h["ro"], h["rd"]) if n is None else (h["ro"][:n].contiguous(), h["rd"][:n].contiguous())
    if kw.pop("with_noises", False):
        kw["noises"] = h["noises"]
    r.render(ro, rd, max_steps=kw.pop("max_steps", 16), **kw)
    torch.cuda.synchronize()
    return rec.take()


def network_frames(rec, h, graph, frames):
    from lzzx_nerf_amd.renderer import NetworkRenderer
    r = NetworkRenderer(operator_net, h["bits"], bound=1.0, graph=graph)
    out = []
    for _ in range(frames):
        r.render(h["ro"], h["rd"], max_steps=6)
        torch.cuda.synchronize()
        out.append(rec.take())
    return out if frames > 1 else out[0]


def python_driven(r):
    r._head_events = []


CASES = {
    # TriplaneRenderer, loop mode
    "triplane loop": lambda rec, t, h: triplane_loop(rec, t),
    "triplane loop noises": lambda rec, t, h: triplane_loop(rec, t, noises=h["noises"][:1024]),
    "triplane loop rgb24": lambda rec, t, h: triplane_loop(rec, t, rgb24=True),
    "triplane loop sync_free=False": lambda rec, t, h: triplane_loop(rec, t, sync_free=False),
    "triplane loop python-driven": lambda rec, t, h: triplane_loop(rec, t, prepare=python_driven, max_steps=3),
    # TriplaneRenderer, fused mode
    "triplane fused two frames": lambda rec, t, h: triplane_fused(rec, t, frames=2, max_steps=16),
    "triplane fused per_ray": lambda rec, t, h: triplane_fused(rec, t, cap="per_ray", max_steps=16),
    "triplane fused reference, cap cannot bind": lambda rec, t, h: triplane_fused(rec, t, max_steps=192),
    "triplane fused reference, cap can bind": lambda rec, t, h: triplane_fused(rec, t, max_steps=16, rgb24=True, noises=h["noises"][:1024]),
    "triplane fused tile": lambda rec, t, h: triplane_fused(rec, t, tile=True, max_steps=16, count_samples=True),
    # HashgridRenderer, loop mode
    "hashgrid loop f32": lambda rec, t, h: hashgrid_frame(rec, h, "loop", max_steps=128),
    "hashgrid loop f16": lambda rec, t, h: hashgrid_frame(rec, h, "loop", "f16", count_samples=True),
    "hashgrid loop noises": lambda rec, t, h: hashgrid_frame(rec, h, "loop", with_noises=True),
    "hashgrid loop rgb24": lambda rec, t, h: hashgrid_frame(rec, h, "loop", rgb24=True, bg_color=torch.full((3,), 0.5, device="cuda")),
    # HashgridRenderer, fused mode
    "hashgrid fused S=1": lambda rec, t, h: hashgrid_frame(rec, h, "fused"),
    "hashgrid fused S=4 f16 per_ray": lambda rec, t, h: hashgrid_frame(rec, h, "fused", "f16", ctor=dict(steps_per_pass=4, cap="per_ray"), count_samples=True),
    "hashgrid fused noises": lambda rec, t, h: hashgrid_frame(rec, h, "fused", with_noises=True),
    "hashgrid fused clip_to_occupancy": lambda rec, t, h: hashgrid_frame(rec, h, "fused", ctor=dict(clip_to_occupancy=True)),
    "hashgrid fused rgb24": lambda rec, t, h: hashgrid_frame(rec, h, "fused", rgb24=True),
    "hashgrid fused tile": lambda rec, t, h: hashgrid_frame(rec, h, "fused", ctor=dict(budget_factor=2, steps_per_pass=2), tile=4096, n=1000),
    "hashgrid fused empty tile": lambda rec, t, h: hashgrid_frame(rec, h, "fused", tile=4096, n=0),
    # NetworkRenderer
    "network graph=False": lambda rec, t, h: network_frames(rec, h, False, 1),
    "network graph=True two frames": lambda rec, t, h: network_frames(rec, h, True, 2),
}

# recorded on the renderers before the refactor (see the module docstring)
EXPECTED = {'triplane loop': ['lz_near_far_from_aabb(p0, p1, p2, 1024, 0.05, p3, p4, null)',
                   'lz_loop_begin(1024, 32, 1024, 8, p3, p5, p6, p7, p8, p9, p10, p11, p12, p13, p14, null)',
                   'lz_loop_run(Frame#0{head={emb_xy=p15 emb_yz=p16 emb_xz=p17 offsets=p18 packed=p19 enc_a=p20 ind_code=p21 eye=p22 bound=1.0 '
                   'S=0.27272728085517883 H=64 testing=1 precision=0} state=p13 workspace=p14 rays_alive=(p5,p23) rays_t=p6 rays_o=p0 rays_d=p1 '
                   'nears=p3 fars=p4 grid=p24 xyzs=p25 dirs=p26 deltas=p27 sigmas=p28 rgbs=p29 amb_aud=p30 amb_eye=p31 unc=p32 weights_sum=p7 '
                   'depth=p8 image=p9 amb_aud_sum=p10 amb_eye_sum=p11 unc_sum=p12 ray_counts=null N=1024 max_steps=32 C=1 H=128 bound=1.0 '
                   'dt_gamma=0.00390625 T_thresh=9.999999747378752e-05 sample_budget=1024 n_step_cap=8}, 0, 8, null, null)',
                   'lz_loop_run(Frame#0, 0, 8, null, null) x3',
                   'lz_final_blend(p9, p7, null, 1.0, 1024, p33, null)'],
 'triplane loop noises': ['lz_near_far_from_aabb(p0, p1, p2, 1024, 0.05, p3, p4, null)',
                          'lz_perturb_starts(p3, p5, 0.00390625, 32, 1, 128, 1024, p6, null)',
                          'lz_loop_begin(1024, 32, 1024, 8, p6, p7, p8, p9, p10, p11, p12, p13, p14, p15, p16, null)',
                          'lz_loop_run(Frame#0{head={emb_xy=p17 emb_yz=p18 emb_xz=p19 offsets=p20 packed=p21 enc_a=p22 ind_code=p23 eye=p24 '
                          'bound=1.0 S=0.27272728085517883 H=64 testing=1 precision=0} state=p15 workspace=p16 rays_alive=(p7,p25) rays_t=p8 '
                          'rays_o=p0 rays_d=p1 nears=p3 fars=p4 grid=p26 xyzs=p27 dirs=p28 deltas=p29 sigmas=p30 rgbs=p31 amb_aud=p32 amb_eye=p33 '
                          'unc=p34 weights_sum=p9 depth=p10 image=p11 amb_aud_sum=p12 amb_eye_sum=p13 unc_sum=p14 ray_counts=null N=1024 '
                          'max_steps=32 C=1 H=128 bound=1.0 dt_gamma=0.00390625 T_thresh=9.999999747378752e-05 sample_budget=1024 n_step_cap=8}, 0, '
                          '8, null, null)',
                          'lz_loop_run(Frame#0, 0, 8, null, null) x3',
                          'lz_final_blend(p11, p9, null, 1.0, 1024, p35, null)'],
 'triplane loop rgb24': ['lz_near_far_from_aabb(p0, p1, p2, 1024, 0.05, p3, p4, null)',
                         'lz_loop_begin(1024, 32, 1024, 8, p3, p5, p6, p7, p8, p9, p10, p11, p12, p13, p14, null)',
                         'lz_loop_run(Frame#0{head={emb_xy=p15 emb_yz=p16 emb_xz=p17 offsets=p18 packed=p19 enc_a=p20 ind_code=p21 eye=p22 bound=1.0 '
                         'S=0.27272728085517883 H=64 testing=1 precision=0} state=p13 workspace=p14 rays_alive=(p5,p23) rays_t=p6 rays_o=p0 '
                         'rays_d=p1 nears=p3 fars=p4 grid=p24 xyzs=p25 dirs=p26 deltas=p27 sigmas=p28 rgbs=p29 amb_aud=p30 amb_eye=p31 unc=p32 '
                         'weights_sum=p7 depth=p8 image=p9 amb_aud_sum=p10 amb_eye_sum=p11 unc_sum=p12 ray_counts=null N=1024 max_steps=32 C=1 H=128 '
                         'bound=1.0 dt_gamma=0.00390625 T_thresh=9.999999747378752e-05 sample_budget=1024 n_step_cap=8}, 0, 8, null, null)',
                         'lz_loop_run(Frame#0, 0, 8, null, null) x3',
                         'lz_final_blend_rgb24(p9, p7, null, 1.0, 1024, p33, p34, null)'],
 'triplane loop sync_free=False': ['lz_near_far_from_aabb(p0, p1, p2, 1024, 0.05, p3, p4, null)',
                                   'lz_loop_begin(1024, 32, 1024, 8, p3, p5, p6, p7, p8, p9, p10, p11, p12, p13, p14, null)',
                                   'lz_loop_run(Frame#0{head={emb_xy=p15 emb_yz=p16 emb_xz=p17 offsets=p18 packed=p19 enc_a=p20 ind_code=p21 eye=p22 '
                                   'bound=1.0 S=0.27272728085517883 H=64 testing=1 precision=0} state=p13 workspace=p14 rays_alive=(p5,p23) '
                                   'rays_t=p6 rays_o=p0 rays_d=p1 nears=p3 fars=p4 grid=p24 xyzs=p25 dirs=p26 deltas=p27 sigmas=p28 rgbs=p29 '
                                   'amb_aud=p30 amb_eye=p31 unc=p32 weights_sum=p7 depth=p8 image=p9 amb_aud_sum=p10 amb_eye_sum=p11 unc_sum=p12 '
                                   'ray_counts=null N=1024 max_steps=32 C=1 H=128 bound=1.0 dt_gamma=0.00390625 T_thresh=9.999999747378752e-05 '
                                   'sample_budget=1024 n_step_cap=8}, 0, 8, null, null)',
                                   'lz_loop_run(Frame#0, 0, 8, null, null)',
                                   'lz_final_blend(p9, p7, null, 1.0, 1024, p33, null)'],
 'triplane loop python-driven': ['lz_near_far_from_aabb(p0, p1, p2, 1024, 0.05, p3, p4, null)',
                                 'lz_loop_begin(1024, 3, 1024, 8, p3, p5, p6, p7, p8, p9, p10, p11, p12, p13, p14, null)',
                                 'lz_loop_march(p13, 1024, 1024, 8, p5, p15, p14, p6, p0, p1, 1.0, 0.00390625, 3, 1, 128, p16, p3, p4, p17, p18, '
                                 'p19, null, null)',
                                 'lz_triplane_head_forward(HeadParams#0{emb_xy=p20 emb_yz=p21 emb_xz=p22 offsets=p23 packed=p24 enc_a=p25 '
                                 'ind_code=p26 eye=p27 bound=1.0 S=0.27272728085517883 H=64 testing=1 precision=0}, p17, p18, 1024, p28, p29, p30, '
                                 'p31, p32, p33, null)',
                                 'lz_loop_composite(p13, 1024, 0.0001, p15, p6, p29, p30, p19, p31, p32, p33, p7, p8, p9, p10, p11, p12, p14, null)',
                                 'lz_loop_march(p13, 1024, 1024, 8, p15, p5, p14, p6, p0, p1, 1.0, 0.00390625, 3, 1, 128, p16, p3, p4, p17, p18, '
                                 'p19, null, null)',
                                 'lz_triplane_head_forward(HeadParams#0, p17, p18, 1024, p28, p29, p30, p31, p32, p33, null)',
                                 'lz_loop_composite(p13, 1024, 0.0001, p5, p6, p29, p30, p19, p31, p32, p33, p7, p8, p9, p10, p11, p12, p14, null)',
                                 'lz_loop_march(p13, 1024, 1024, 8, p5, p15, p14, p6, p0, p1, 1.0, 0.00390625, 3, 1, 128, p16, p3, p4, p17, p18, '
                                 'p19, null, null)',
                                 'lz_triplane_head_forward(HeadParams#0, p17, p18, 1024, p28, p29, p30, p31, p32, p33, null)',
                                 'lz_loop_composite(p13, 1024, 0.0001, p15, p6, p29, p30, p19, p31, p32, p33, p7, p8, p9, p10, p11, p12, p14, null)',
                                 'lz_loop_march(p13, 1024, 1024, 8, p15, p5, p14, p6, p0, p1, 1.0, 0.00390625, 3, 1, 128, p16, p3, p4, p17, p18, '
                                 'p19, null, null)',
                                 'lz_triplane_head_forward(HeadParams#0, p17, p18, 1024, p28, p29, p30, p31, p32, p33, null)',
                                 'lz_loop_composite(p13, 1024, 0.0001, p5, p6, p29, p30, p19, p31, p32, p33, p7, p8, p9, p10, p11, p12, p14, null)',
                                 'lz_final_blend(p9, p7, null, 1.0, 1024, p34, null)'],
 'triplane fused two frames': [['lz_occupied_bounds(p0, 1, 128, 1.0, 8, p1, p2, null)',
                                'lz_frame_render(FrameFused#0{head={emb_xy=p3 emb_yz=p4 emb_xz=p5 offsets=p6 packed=p7 enc_a=p8 ind_code=p9 eye=p10 '
                                'bound=1.0 S=0.27272728085517883 H=64 testing=1 precision=0} rays_o=p11 rays_d=p12 grid=p0 aabb=p13 nears=p14 '
                                'fars=p15 rays_t=p16 order=p17 state=p18 keys=p19 weights_sum=p20 depth=p21 image=p22 amb_aud_sum=p23 '
                                'amb_eye_sum=p24 unc_sum=p25 out=p26 bg=null out_rgb24=null ray_counts=null bg_scalar=1.0 bound=1.0 '
                                'dt_gamma=0.00390625 T_thresh=9.999999747378752e-05 min_near=0.05000000074505806 N=1024 max_steps=16 C=1 H=128 '
                                'steps_per_pass=0 noises=null occupied_aabb=p2 t_end=p27 cap_mode=1 N_total=0 defer_finish=0 ray_last=p28 '
                                'cap_ws=p29}, null, null)'],
                               ['lz_frame_render(FrameFused#0{head={emb_xy=p0 emb_yz=p1 emb_xz=p2 offsets=p3 packed=p4 enc_a=p5 ind_code=p6 eye=p7 '
                                'bound=1.0 S=0.27272728085517883 H=64 testing=1 precision=0} rays_o=p8 rays_d=p9 grid=p10 aabb=p11 nears=p12 '
                                'fars=p13 rays_t=p14 order=p15 state=p16 keys=p17 weights_sum=p18 depth=p19 image=p20 amb_aud_sum=p21 '
                                'amb_eye_sum=p22 unc_sum=p23 out=p24 bg=null out_rgb24=null ray_counts=null bg_scalar=1.0 bound=1.0 '
                                'dt_gamma=0.00390625 T_thresh=9.999999747378752e-05 min_near=0.05000000074505806 N=1024 max_steps=16 C=1 H=128 '
                                'steps_per_pass=0 noises=null occupied_aabb=p25 t_end=p26 cap_mode=1 N_total=0 defer_finish=0 ray_last=p27 '
                                'cap_ws=p28}, null, null)']],
 'triplane fused per_ray': ['lz_occupied_bounds(p0, 1, 128, 1.0, 8, p1, p2, null)',
                            'lz_frame_render(FrameFused#0{head={emb_xy=p3 emb_yz=p4 emb_xz=p5 offsets=p6 packed=p7 enc_a=p8 ind_code=p9 eye=p10 '
                            'bound=1.0 S=0.27272728085517883 H=64 testing=1 precision=0} rays_o=p11 rays_d=p12 grid=p0 aabb=p13 nears=p14 fars=p15 '
                            'rays_t=p16 order=p17 state=p18 keys=p19 weights_sum=p20 depth=p21 image=p22 amb_aud_sum=p23 amb_eye_sum=p24 unc_sum=p25 '
                            'out=p26 bg=null out_rgb24=null ray_counts=null bg_scalar=1.0 bound=1.0 dt_gamma=0.00390625 '
                            'T_thresh=9.999999747378752e-05 min_near=0.05000000074505806 N=1024 max_steps=16 C=1 H=128 steps_per_pass=0 noises=null '
                            'occupied_aabb=p2 t_end=p27 cap_mode=0 N_total=0 defer_finish=0 ray_last=null cap_ws=null}, null, null)'],
 'triplane fused reference, cap cannot bind': ['lz_occupied_bounds(p0, 1, 128, 1.0, 8, p1, p2, null)',
                                               'lz_frame_render(FrameFused#0{head={emb_xy=p3 emb_yz=p4 emb_xz=p5 offsets=p6 packed=p7 enc_a=p8 '
                                               'ind_code=p9 eye=p10 bound=1.0 S=0.27272728085517883 H=64 testing=1 precision=0} rays_o=p11 '
                                               'rays_d=p12 grid=p0 aabb=p13 nears=p14 fars=p15 rays_t=p16 order=p17 state=p18 keys=p19 '
                                               'weights_sum=p20 depth=p21 image=p22 amb_aud_sum=p23 amb_eye_sum=p24 unc_sum=p25 out=p26 bg=null '
                                               'out_rgb24=null ray_counts=null bg_scalar=1.0 bound=1.0 dt_gamma=0.00390625 '
                                               'T_thresh=9.999999747378752e-05 min_near=0.05000000074505806 N=1024 max_steps=192 C=1 H=128 '
                                               'steps_per_pass=0 noises=null occupied_aabb=p2 t_end=p27 cap_mode=0 N_total=0 defer_finish=0 '
                                               'ray_last=null cap_ws=null}, null, null)'],
 'triplane fused reference, cap can bind': ['lz_occupied_bounds(p0, 1, 128, 1.0, 8, p1, p2, null)',
                                            'lz_frame_render(FrameFused#0{head={emb_xy=p3 emb_yz=p4 emb_xz=p5 offsets=p6 packed=p7 enc_a=p8 '
                                            'ind_code=p9 eye=p10 bound=1.0 S=0.27272728085517883 H=64 testing=1 precision=0} rays_o=p11 rays_d=p12 '
                                            'grid=p0 aabb=p13 nears=p14 fars=p15 rays_t=p16 order=p17 state=p18 keys=p19 weights_sum=p20 depth=p21 '
                                            'image=p22 amb_aud_sum=p23 amb_eye_sum=p24 unc_sum=p25 out=p26 bg=null out_rgb24=p27 ray_counts=null '
                                            'bg_scalar=1.0 bound=1.0 dt_gamma=0.00390625 T_thresh=9.999999747378752e-05 min_near=0.05000000074505806 '
                                            'N=1024 max_steps=16 C=1 H=128 steps_per_pass=0 noises=p28 occupied_aabb=p2 t_end=p29 cap_mode=1 '
                                            'N_total=0 defer_finish=0 ray_last=p30 cap_ws=p31}, null, null)'],
 'triplane fused tile': ['lz_occupied_bounds(p0, 1, 128, 1.0, 8, p1, p2, null)',
                         'lz_frame_render(FrameFused#0{head={emb_xy=p3 emb_yz=p4 emb_xz=p5 offsets=p6 packed=p7 enc_a=p8 ind_code=p9 eye=p10 '
                         'bound=1.0 S=0.27272728085517883 H=64 testing=1 precision=0} rays_o=p11 rays_d=p12 grid=p0 aabb=p13 nears=p14 fars=p15 '
                         'rays_t=p16 order=p17 state=p18 keys=p19 weights_sum=p20 depth=p21 image=p22 amb_aud_sum=p23 amb_eye_sum=p24 unc_sum=p25 '
                         'out=p26 bg=null out_rgb24=null ray_counts=p27 bg_scalar=1.0 bound=1.0 dt_gamma=0.00390625 T_thresh=9.999999747378752e-05 '
                         'min_near=0.05000000074505806 N=1024 max_steps=16 C=1 H=128 steps_per_pass=0 noises=null occupied_aabb=p2 t_end=p28 '
                         'cap_mode=1 N_total=2048 defer_finish=1 ray_last=p29 cap_ws=p30}, null, null)',
                         'exchange(torch.int32 (17,))',
                         'lz_frame_finish(FrameFused#0, null)'],
 'hashgrid loop f32': ['lz_near_far_from_aabb(p0, p1, p2, 2304, 0.05, p3, p4, null)',
                       'lz_loop_begin(2304, 128, 2304, 8, p3, p5, p6, p7, p8, p9, null, null, null, p10, p11, null)',
                       'lz_ngp_loop_run(FrameNgp#0{packed=p12 embeddings=p13 offsets=p14 enc_L=16 enc_H=16 enc_S=0.46666666865348816 emb_f16=0 '
                       'feats=p15 state=p10 workspace=p11 rays_alive=(p5,p16) rays_t=p6 rays_o=p0 rays_d=p1 nears=p3 fars=p4 grid=p17 xyzs=p18 '
                       'dirs=p19 deltas=p20 sigmas=p21 rgbs=p22 weights_sum=p7 depth=p8 image=p9 ray_counts=null N=2304 max_steps=128 C=1 H=128 '
                       'bound=1.0 dt_gamma=0.00390625 T_thresh=9.999999747378752e-05 sample_budget=2304 n_step_cap=8}, 0, 4, null)',
                       'lz_ngp_loop_run(FrameNgp#0, 0, 4, null) x3',
                       'lz_final_blend(p9, p7, null, 1.0, 2304, p23, null)'],
 'hashgrid loop f16': ['lz_near_far_from_aabb(p0, p1, p2, 2304, 0.05, p3, p4, null)',
                       'lz_loop_begin(2304, 16, 2304, 8, p3, p5, p6, p7, p8, p9, null, null, null, p10, p11, null)',
                       'lz_ngp_loop_run_f16(FrameNgp#0{packed=p12 embeddings=p13 offsets=p14 enc_L=16 enc_H=16 enc_S=0.46666666865348816 emb_f16=1 '
                       'feats=p15 state=p10 workspace=p11 rays_alive=(p5,p16) rays_t=p6 rays_o=p0 rays_d=p1 nears=p3 fars=p4 grid=p17 xyzs=p18 '
                       'dirs=p19 deltas=p20 sigmas=p21 rgbs=p22 weights_sum=p7 depth=p8 image=p9 ray_counts=p23 N=2304 max_steps=16 C=1 H=128 '
                       'bound=1.0 dt_gamma=0.00390625 T_thresh=9.999999747378752e-05 sample_budget=2304 n_step_cap=8}, p24, 0, 4, null)',
                       'lz_ngp_loop_run_f16(FrameNgp#0, p24, 0, 4, null) x3',
                       'lz_final_blend(p9, p7, null, 1.0, 2304, p25, null)'],
 'hashgrid loop noises': ['lz_near_far_from_aabb(p0, p1, p2, 2304, 0.05, p3, p4, null)',
                          'lz_perturb_starts(p3, p5, 0.00390625, 16, 1, 128, 2304, p6, null)',
                          'lz_loop_begin(2304, 16, 2304, 8, p6, p7, p8, p9, p10, p11, null, null, null, p12, p13, null)',
                          'lz_ngp_loop_run(FrameNgp#0{packed=p14 embeddings=p15 offsets=p16 enc_L=16 enc_H=16 enc_S=0.46666666865348816 emb_f16=0 '
                          'feats=p17 state=p12 workspace=p13 rays_alive=(p7,p18) rays_t=p8 rays_o=p0 rays_d=p1 nears=p3 fars=p4 grid=p19 xyzs=p20 '
                          'dirs=p21 deltas=p22 sigmas=p23 rgbs=p24 weights_sum=p9 depth=p10 image=p11 ray_counts=null N=2304 max_steps=16 C=1 H=128 '
                          'bound=1.0 dt_gamma=0.00390625 T_thresh=9.999999747378752e-05 sample_budget=2304 n_step_cap=8}, 0, 4, null)',
                          'lz_ngp_loop_run(FrameNgp#0, 0, 4, null) x3',
                          'lz_final_blend(p11, p9, null, 1.0, 2304, p25, null)'],
 'hashgrid loop rgb24': ['lz_near_far_from_aabb(p0, p1, p2, 2304, 0.05, p3, p4, null)',
                         'lz_loop_begin(2304, 16, 2304, 8, p3, p5, p6, p7, p8, p9, null, null, null, p10, p11, null)',
                         'lz_ngp_loop_run(FrameNgp#0{packed=p12 embeddings=p13 offsets=p14 enc_L=16 enc_H=16 enc_S=0.46666666865348816 emb_f16=0 '
                         'feats=p15 state=p10 workspace=p11 rays_alive=(p5,p16) rays_t=p6 rays_o=p0 rays_d=p1 nears=p3 fars=p4 grid=p17 xyzs=p18 '
                         'dirs=p19 deltas=p20 sigmas=p21 rgbs=p22 weights_sum=p7 depth=p8 image=p9 ray_counts=null N=2304 max_steps=16 C=1 H=128 '
                         'bound=1.0 dt_gamma=0.00390625 T_thresh=9.999999747378752e-05 sample_budget=2304 n_step_cap=8}, 0, 4, null)',
                         'lz_ngp_loop_run(FrameNgp#0, 0, 4, null) x3',
                         'lz_final_blend_rgb24(p9, p7, p23, 1.0, 2304, p24, p25, null)'],
 'hashgrid fused S=1': ['lz_ngp_frame_render_opts(FrameNgpFused#0{packed=p0 packed16=null precision=0 emb_f16=0 embeddings=p1 offsets=p2 enc_L=16 '
                        'enc_H=16 enc_S=0.46666666865348816 cap_mode=1 rays_o=p3 rays_d=p4 grid=p5 aabb=p6 nears=p7 fars=p8 rays_t=p9 order=p10 '
                        'state=p11 keys=p12 scratch=p13 weights_sum=p14 depth=p15 image=p16 out=p17 bg=null ray_counts=null ray_last=p18 cap_ws=p19 '
                        'bg_scalar=1.0 bound=1.0 dt_gamma=0.00390625 T_thresh=9.999999747378752e-05 min_near=0.05000000074505806 N=2304 max_steps=16 '
                        'C=1 H=128 N_total=2304}, null, 1, null, null)'],
 'hashgrid fused S=4 f16 per_ray': ['lz_ngp_frame_render_opts(FrameNgpFused#0{packed=p0 packed16=p1 precision=1 emb_f16=1 embeddings=p2 offsets=p3 '
                                    'enc_L=16 enc_H=16 enc_S=0.46666666865348816 cap_mode=0 rays_o=p4 rays_d=p5 grid=p6 aabb=p7 nears=p8 fars=p9 '
                                    'rays_t=p10 order=p11 state=p12 keys=p13 scratch=p14 weights_sum=p15 depth=p16 image=p17 out=p18 bg=null '
                                    'ray_counts=p19 ray_last=null cap_ws=null bg_scalar=1.0 bound=1.0 dt_gamma=0.00390625 '
                                    'T_thresh=9.999999747378752e-05 min_near=0.05000000074505806 N=2304 max_steps=16 C=1 H=128 N_total=0}, null, 4, '
                                    'null, null)'],
 'hashgrid fused noises': ['lz_ngp_frame_render_opts(FrameNgpFused#0{packed=p0 packed16=null precision=0 emb_f16=0 embeddings=p1 offsets=p2 enc_L=16 '
                           'enc_H=16 enc_S=0.46666666865348816 cap_mode=1 rays_o=p3 rays_d=p4 grid=p5 aabb=p6 nears=p7 fars=p8 rays_t=p9 order=p10 '
                           'state=p11 keys=p12 scratch=p13 weights_sum=p14 depth=p15 image=p16 out=p17 bg=null ray_counts=null ray_last=p18 '
                           'cap_ws=p19 bg_scalar=1.0 bound=1.0 dt_gamma=0.00390625 T_thresh=9.999999747378752e-05 min_near=0.05000000074505806 '
                           'N=2304 max_steps=16 C=1 H=128 N_total=2304}, FrameNgpFusedOpts#1{noises=p20 occupied_aabb=null t_end=null out_rgb24=null '
                           'defer_finish=0}, 1, null, null)'],
 'hashgrid fused clip_to_occupancy': ['lz_occupied_bounds(p0, 1, 128, 1.0, 8, p1, p2, null)',
                                      'lz_ngp_frame_render_opts(FrameNgpFused#0{packed=p3 packed16=null precision=0 emb_f16=0 embeddings=p4 '
                                      'offsets=p5 enc_L=16 enc_H=16 enc_S=0.46666666865348816 cap_mode=1 rays_o=p6 rays_d=p7 grid=p0 aabb=p8 '
                                      'nears=p9 fars=p10 rays_t=p11 order=p12 state=p13 keys=p14 scratch=p15 weights_sum=p16 depth=p17 image=p18 '
                                      'out=p19 bg=null ray_counts=null ray_last=p20 cap_ws=p21 bg_scalar=1.0 bound=1.0 dt_gamma=0.00390625 '
                                      'T_thresh=9.999999747378752e-05 min_near=0.05000000074505806 N=2304 max_steps=16 C=1 H=128 N_total=2304}, '
                                      'FrameNgpFusedOpts#1{noises=null occupied_aabb=p2 t_end=p22 out_rgb24=null defer_finish=0}, 1, null, null)'],
 'hashgrid fused rgb24': ['lz_ngp_frame_render_opts(FrameNgpFused#0{packed=p0 packed16=null precision=0 emb_f16=0 embeddings=p1 offsets=p2 enc_L=16 '
                          'enc_H=16 enc_S=0.46666666865348816 cap_mode=1 rays_o=p3 rays_d=p4 grid=p5 aabb=p6 nears=p7 fars=p8 rays_t=p9 order=p10 '
                          'state=p11 keys=p12 scratch=p13 weights_sum=p14 depth=p15 image=p16 out=p17 bg=null ray_counts=null ray_last=p18 '
                          'cap_ws=p19 bg_scalar=1.0 bound=1.0 dt_gamma=0.00390625 T_thresh=9.999999747378752e-05 min_near=0.05000000074505806 N=2304 '
                          'max_steps=16 C=1 H=128 N_total=2304}, FrameNgpFusedOpts#1{noises=null occupied_aabb=null t_end=null out_rgb24=p20 '
                          'defer_finish=0}, 1, null, null)'],
 'hashgrid fused tile': ['lz_ngp_frame_render_opts(FrameNgpFused#0{packed=p0 packed16=null precision=0 emb_f16=0 embeddings=p1 offsets=p2 enc_L=16 '
                         'enc_H=16 enc_S=0.46666666865348816 cap_mode=1 rays_o=p3 rays_d=p4 grid=p5 aabb=p6 nears=p7 fars=p8 rays_t=p9 order=p10 '
                         'state=p11 keys=p12 scratch=p13 weights_sum=p14 depth=p15 image=p16 out=p17 bg=null ray_counts=null ray_last=p18 cap_ws=p19 '
                         'bg_scalar=1.0 bound=1.0 dt_gamma=0.00390625 T_thresh=9.999999747378752e-05 min_near=0.05000000074505806 N=1000 '
                         'max_steps=16 C=1 H=128 N_total=8192}, FrameNgpFusedOpts#1{noises=null occupied_aabb=null t_end=null out_rgb24=null '
                         'defer_finish=1}, 2, null, null)',
                         'exchange(torch.int32 (17,))',
                         'lz_ngp_frame_finish(FrameNgpFused#0, FrameNgpFusedOpts#1, 2, null)'],
 'hashgrid fused empty tile': ['lz_ngp_frame_render_opts(FrameNgpFused#0{packed=p0 packed16=null precision=0 emb_f16=0 embeddings=p1 offsets=p2 '
                               'enc_L=16 enc_H=16 enc_S=0.46666666865348816 cap_mode=1 rays_o=null rays_d=null grid=p3 aabb=p4 nears=null fars=null '
                               'rays_t=null order=null state=p5 keys=null scratch=null weights_sum=null depth=null image=null out=null bg=null '
                               'ray_counts=null ray_last=null cap_ws=p6 bg_scalar=1.0 bound=1.0 dt_gamma=0.00390625 T_thresh=9.999999747378752e-05 '
                               'min_near=0.05000000074505806 N=0 max_steps=16 C=1 H=128 N_total=4096}, FrameNgpFusedOpts#1{noises=null '
                               'occupied_aabb=null t_end=null out_rgb24=null defer_finish=1}, 1, null, null)',
                               'exchange(torch.int32 (17,))',
                               'lz_ngp_frame_finish(FrameNgpFused#0, FrameNgpFusedOpts#1, 1, null)'],
 'network graph=False': ['lz_near_far_from_aabb(p0, p1, p2, 2304, 0.05, p3, p4, null)',
                         'lz_loop_begin(2304, 6, 9216, 4, p3, p5, p6, p7, p8, p9, p10, p11, p12, p13, p14, null)',
                         'lz_loop_march(p13, 2304, 9216, 4, p5, p15, p14, p6, p0, p1, 1.0, 0.00390625, 6, 1, 128, p16, p3, p4, p17, p18, p19, null, '
                         'null)',
                         'lz_loop_composite(p13, 2304, 0.0001, p15, p6, p20, p21, p19, p22, p23, p24, p7, p8, p9, p10, p11, p12, p14, null)',
                         'lz_loop_march(p13, 2304, 9216, 4, p15, p5, p14, p6, p0, p1, 1.0, 0.00390625, 6, 1, 128, p16, p3, p4, p17, p18, p19, null, '
                         'null)',
                         'lz_loop_composite(p13, 2304, 0.0001, p5, p6, p20, p21, p19, p22, p23, p24, p7, p8, p9, p10, p11, p12, p14, null)',
                         'lz_loop_march(p13, 2304, 9216, 4, p5, p15, p14, p6, p0, p1, 1.0, 0.00390625, 6, 1, 128, p16, p3, p4, p17, p18, p19, null, '
                         'null)',
                         'lz_loop_composite(p13, 2304, 0.0001, p15, p6, p20, p21, p19, p22, p23, p24, p7, p8, p9, p10, p11, p12, p14, null)',
                         'lz_loop_march(p13, 2304, 9216, 4, p15, p5, p14, p6, p0, p1, 1.0, 0.00390625, 6, 1, 128, p16, p3, p4, p17, p18, p19, null, '
                         'null)',
                         'lz_loop_composite(p13, 2304, 0.0001, p5, p6, p20, p21, p19, p22, p23, p24, p7, p8, p9, p10, p11, p12, p14, null)',
                         'lz_loop_march(p13, 2304, 9216, 4, p5, p15, p14, p6, p0, p1, 1.0, 0.00390625, 6, 1, 128, p16, p3, p4, p17, p18, p19, null, '
                         'null)',
                         'lz_loop_composite(p13, 2304, 0.0001, p15, p6, p20, p21, p19, p22, p23, p24, p7, p8, p9, p10, p11, p12, p14, null)',
                         'lz_loop_march(p13, 2304, 9216, 4, p15, p5, p14, p6, p0, p1, 1.0, 0.00390625, 6, 1, 128, p16, p3, p4, p17, p18, p19, null, '
                         'null)',
                         'lz_loop_composite(p13, 2304, 0.0001, p5, p6, p20, p21, p19, p22, p23, p24, p7, p8, p9, p10, p11, p12, p14, null)',
                         'lz_loop_march(p13, 2304, 9216, 4, p5, p15, p14, p6, p0, p1, 1.0, 0.00390625, 6, 1, 128, p16, p3, p4, p17, p18, p19, null, '
                         'null)',
                         'lz_loop_composite(p13, 2304, 0.0001, p15, p6, p20, p21, p19, p22, p23, p24, p7, p8, p9, p10, p11, p12, p14, null)',
                         'lz_loop_march(p13, 2304, 9216, 4, p15, p5, p14, p6, p0, p1, 1.0, 0.00390625, 6, 1, 128, p16, p3, p4, p17, p18, p19, null, '
                         'null)',
                         'lz_loop_composite(p13, 2304, 0.0001, p5, p6, p20, p21, p19, p22, p23, p24, p7, p8, p9, p10, p11, p12, p14, null)',
                         'lz_loop_march(p13, 2304, 9216, 4, p5, p15, p14, p6, p0, p1, 1.0, 0.00390625, 6, 1, 128, p16, p3, p4, p17, p18, p19, null, '
                         'null)',
                         'lz_loop_composite(p13, 2304, 0.0001, p15, p6, p20, p21, p19, p22, p23, p24, p7, p8, p9, p10, p11, p12, p14, null)',
                         'lz_loop_march(p13, 2304, 9216, 4, p15, p5, p14, p6, p0, p1, 1.0, 0.00390625, 6, 1, 128, p16, p3, p4, p17, p18, p19, null, '
                         'null)',
                         'lz_loop_composite(p13, 2304, 0.0001, p5, p6, p20, p21, p19, p22, p23, p24, p7, p8, p9, p10, p11, p12, p14, null)',
                         'lz_final_blend(p9, p7, null, 1.0, 2304, p25, null)'],
 'network graph=True two frames': [['lz_near_far_from_aabb(p0, p1, p2, 2304, 0.05, p3, p4, null)',
                                    'lz_loop_begin(2304, 6, 9216, 4, p3, p5, p6, p7, p8, p9, p10, p11, p12, p13, p14, null)',
                                    'lz_loop_march(p13, 2304, 9216, 4, p5, p15, p14, p6, p0, p1, 1.0, 0.00390625, 6, 1, 128, p16, p3, p4, p17, p18, '
                                    'p19, null, p20)',
                                    'lz_loop_composite(p13, 2304, 0.0001, p15, p6, p21, p22, p19, p23, p24, p25, p7, p8, p9, p10, p11, p12, p14, '
                                    'p20)',
                                    'lz_loop_march(p13, 2304, 9216, 4, p15, p5, p14, p6, p0, p1, 1.0, 0.00390625, 6, 1, 128, p16, p3, p4, p17, p18, '
                                    'p19, null, p20)',
                                    'lz_loop_composite(p13, 2304, 0.0001, p5, p6, p21, p22, p19, p23, p24, p25, p7, p8, p9, p10, p11, p12, p14, p20)',
                                    'lz_loop_march(p13, 2304, 9216, 4, p5, p15, p14, p6, p0, p1, 1.0, 0.00390625, 6, 1, 128, p16, p3, p4, p17, p18, '
                                    'p19, null, p26)',
                                    'lz_loop_composite(p13, 2304, 0.0001, p15, p6, p21, p22, p19, p23, p24, p25, p7, p8, p9, p10, p11, p12, p14, '
                                    'p26)',
                                    'lz_loop_march(p13, 2304, 9216, 4, p15, p5, p14, p6, p0, p1, 1.0, 0.00390625, 6, 1, 128, p16, p3, p4, p17, p18, '
                                    'p19, null, p26)',
                                    'lz_loop_composite(p13, 2304, 0.0001, p5, p6, p21, p22, p19, p23, p24, p25, p7, p8, p9, p10, p11, p12, p14, p26)',
                                    'lz_final_blend(p9, p7, null, 1.0, 2304, p27, null)'],
                                   ['lz_near_far_from_aabb(p0, p1, p2, 2304, 0.05, p3, p4, null)',
                                    'lz_loop_begin(2304, 6, 9216, 4, p3, p5, p6, p7, p8, p9, p10, p11, p12, p13, p14, null)',
                                    'lz_final_blend(p9, p7, null, 1.0, 2304, p15, null)']]}


@pytest.mark.parametrize("case", list(CASES))
def test_calls_are_those_of_the_record(rec, triplane, hashgrid, case):
    got = CASES[case](rec, triplane, hashgrid)
    print("RECORD %r: %r" % (case, got))
    assert got == EXPECTED[case]


# ---- every renderer and mode: the result's keys, and a steady state that allocates nothing ---------------------------------------------
BASE_KEYS = {"image", "image_raw", "weights_sum", "depth", "state"}
TRIPLANE_KEYS = BASE_KEYS | {"amb_aud_sum", "amb_eye_sum", "uncertainty_sum", "nears", "fars"}


def steady_triplane(t, mode):
    r = triplane_renderer(t, mode=mode)
    return lambda **kw: r.render(t["ro"], t["rd"], *t["cond"], max_steps=16, **kw)


def steady_hashgrid(h, mode):
    from lzzx_nerf_amd.ngp import HashgridRenderer
    r = HashgridRenderer(h["nets"]["f32"], h["bits"], bound=1.0, mode=mode)
    return lambda **kw: r.render(h["ro"], h["rd"], max_steps=16, **kw)


def steady_network(h, graph):
    from lzzx_nerf_amd.renderer import NetworkRenderer
    r = NetworkRenderer(operator_net, h["bits"], bound=1.0, graph=graph)
    return lambda **kw: r.render(h["ro"], h["rd"], max_steps=6, **kw)


STEADY = {
    "triplane loop": (lambda t, h: steady_triplane(t, "loop"), TRIPLANE_KEYS, True),
    "triplane fused": (lambda t, h: steady_triplane(t, "fused"), TRIPLANE_KEYS, True),
    "hashgrid loop": (lambda t, h: steady_hashgrid(h, "loop"), BASE_KEYS, True),
    "hashgrid fused": (lambda t, h: steady_hashgrid(h, "fused"), BASE_KEYS, True),
    "network": (lambda t, h: steady_network(h, False), BASE_KEYS, False),
    "network graph": (lambda t, h: steady_network(h, True), BASE_KEYS, False),
}


@pytest.mark.parametrize("which", list(STEADY))
def test_keys_and_steady_state(triplane, hashgrid, which):
    make, keys, has_rgb24 = STEADY[which]
    frame = make(triplane, hashgrid)
    assert set(frame()) == keys
    assert set(frame(count_samples=True)) == keys | {"ray_counts"}
    if has_rgb24:
        assert set(frame(count_samples=True, rgb24=True)) == keys | {"ray_counts", "image_rgb24"}
    # a new renderer; the same N, a scalar background, no noises: frame 3 writes the tensors of frame 2 and allocates nothing
    frame = make(triplane, hashgrid)
    frame()
    second = {k: v.data_ptr() for k, v in frame().items()}
    torch.cuda.synchronize()
    held = torch.cuda.memory_allocated()
    third = {k: v.data_ptr() for k, v in frame().items()}
    torch.cuda.synchronize()
    assert third == second
    assert torch.cuda.memory_allocated() == held
