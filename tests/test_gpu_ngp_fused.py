"""HashgridRenderer(mode="fused") -- the cfg2 frame as one persistent kernel (csrc/lz_ngp_frame.hip) -- against the LOOP mode of the same
renderer, which the existing cfg2 tests pin bit for bit to the checker and to the reference's loop.  Every comparison is torch.equal, for
the f32 network, the f16 network and the f32 network on half tables alike: a sample's sigma / rgb do not depend on which other samples share its slice, and compositing is
sequential per ray."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import ellipsoid_bitfield, synthetic_camera

pytestmark = pytest.mark.gpu
F32 = np.float32
LZF_CEFF = 10
KEYS = ("image", "image_raw", "weights_sum", "depth", "ray_counts")
# the three kernel instances: f32 tables + f32 head, half tables + f16 head, half tables + f32 head
NETS = ["f32", "f16", "half_tables"]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def nets():
    from lzzx_nerf_amd.ngp import FusedHashgridNeRF
    from lzzx_nerf_amd.synthetic import GenericHashgridNeRF
    g = GenericHashgridNeRF(torch.device("cuda"), seed=3)
    nets = {p: FusedHashgridNeRF(g.enc, g.sigma_net, g.color_net, precision=p) for p in ("f32", "f16")}
    nets["half_tables"] = FusedHashgridNeRF(g.enc, g.sigma_net, g.color_net, half_tables=True)
    assert nets["half_tables"].precision == "f32" and nets["half_tables"].table.dtype == torch.float16
    return nets


@pytest.fixture(scope="module")
def scene():
    """the ellipsoid with seeded holes (a quarter of its bytes cleared: empty cells inside the object), 48 x 48 camera rays"""
    from lzzx_nerf_amd.utils import frame_rays
    full = ellipsoid_bitfield()[0]
    holes = full & np.where(np.random.default_rng(5).random(full.shape) < 0.25, 0, 255).astype(full.dtype)
    assert 0 < int(np.unpackbits(holes).sum()) < int(np.unpackbits(full).sum())
    pose, intr = synthetic_camera(48, 48)
    ro, rd = frame_rays(dev(pose), intr, 48, 48)
    return dict(full=dev(full), holes=dev(holes), ro=ro.reshape(-1, 3).contiguous(), rd=rd.reshape(-1, 3).contiguous())


def pair(net, bits, ro, rd, ctor=None, **kw):
    """the same frame in both modes -> (loop, fused) result dicts (cloned)"""
    from lzzx_nerf_amd.ngp import HashgridRenderer
    ctor = {"bound": 1.0, **(ctor or {})}
    out = []
    for mode in ("loop", "fused"):
        r = HashgridRenderer(net, bits, mode=mode, **ctor)
        out.append({k: v.clone() for k, v in r.render(ro, rd, count_samples=True, **kw).items()})
    torch.cuda.synchronize()
    return out


def assert_same(loop, fused, keys=KEYS):
    for k in keys:
        assert loop[k].shape == fused[k].shape and loop[k].dtype == fused[k].dtype, k
        assert torch.equal(loop[k], fused[k]), (k, int((loop[k] != fused[k]).sum()), loop[k].numel())


# ---- 1. fused == loop, full outputs -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", NETS)
def test_fused_equals_loop_cap_not_binding(nets, scene, precision):
    """case A: 48 x 48 rays, max_steps 128, the reference's schedule (1, 8)"""
    loop, fused = pair(nets[precision], scene["holes"], scene["ro"], scene["rd"], max_steps=128)
    assert_same(loop, fused)
    cnt = loop["ray_counts"]
    assert int(cnt.max()) > 8 and int(cnt.max()) < 128 and float(loop["weights_sum"].max()) > 0.5 and int((cnt == 0).sum()) > 0
    assert int(fused["state"][3]) == 1 and int(fused["state"][5]) == int(cnt.sum())


@pytest.mark.parametrize("precision", NETS)
def test_fused_equals_loop_cap_binding(nets, scene, precision):
    """case B: max_steps 16, T_thresh 1e-4, the full ellipsoid: rays stand at the cap and the schedule carries them past it (C_eff > 16)"""
    loop, fused = pair(nets[precision], scene["full"], scene["ro"], scene["rd"], max_steps=16, T_thresh=1e-4)
    c_eff = int(fused["state"][LZF_CEFF])
    print("C_eff %d, rays at the cap %d, max count %d" % (c_eff, int(fused["state"][9]), int(loop["ray_counts"].max())))
    assert c_eff > 16 and int(fused["state"][9]) > 0
    assert int(loop["ray_counts"].max()) == c_eff
    assert_same(loop, fused)


@pytest.mark.parametrize("precision", NETS)
def test_fused_equals_loop_fat_schedule(nets, scene, precision):
    """(budget_factor, n_step_cap) = (8, 8) at max_steps 16: n_step = 8 throughout, the fused mode replays that schedule's C_eff"""
    loop, fused = pair(nets[precision], scene["holes"], scene["ro"], scene["rd"], ctor=dict(budget_factor=8, n_step_cap=8), max_steps=16)
    assert int(fused["state"][LZF_CEFF]) == 16 and int(loop["ray_counts"].max()) == 16
    assert_same(loop, fused)


# ---- 2. shapes where slots and the queue can go wrong ------------------------------------------------------------------------------------
def _sub(scene, n, seed):
    idx = torch.from_numpy(np.random.default_rng(seed).permutation(scene["ro"].shape[0])[:n]).cuda()
    return scene["ro"][idx].contiguous(), scene["rd"][idx].contiguous()


@pytest.mark.parametrize("precision", NETS)
@pytest.mark.parametrize("n", [5, 37 * 29])
def test_fused_ray_counts_that_do_not_fill_the_slots(nets, scene, precision, n):
    ro, rd = _sub(scene, n, n)
    loop, fused = pair(nets[precision], scene["holes"], ro, rd, max_steps=48)
    assert_same(loop, fused)
    assert float(loop["weights_sum"].max()) > 0.0


@pytest.mark.parametrize("mode,cap", [("fused", "reference"), ("fused", "per_ray")])
def test_fused_on_no_rays(nets, scene, mode, cap):
    from lzzx_nerf_amd.ngp import HashgridRenderer
    e = torch.empty(0, 3, device="cuda")
    o = HashgridRenderer(nets["f32"], scene["holes"], bound=1.0, mode=mode, cap=cap).render(e, e, max_steps=16, count_samples=True)
    torch.cuda.synchronize()
    assert o["image"].shape == (0, 3) and o["depth"].shape == (0,) and o["ray_counts"].shape == (0,) and int(o["state"][5]) == 0


@pytest.mark.parametrize("precision", NETS)
def test_fused_all_rays_miss_the_box(nets, scene, precision):
    """every pixel is background and the queue is empty"""
    ro = scene["ro"][:300] + torch.tensor([0.0, 50.0, 0.0], device="cuda")
    rd = torch.tensor([1.0, 0.0, 0.0], device="cuda").expand(300, 3).contiguous()
    loop, fused = pair(nets[precision], scene["holes"], ro.contiguous(), rd, max_steps=32, bg_color=0.25)
    assert_same(loop, fused)
    assert bool((fused["image"] == 0.25).all()) and int(fused["state"][1]) == 0 and int(fused["ray_counts"].sum()) == 0


@pytest.mark.parametrize("precision", NETS)
@pytest.mark.parametrize("fill", [0, 255])
def test_fused_uniform_bitfields(nets, scene, precision, fill):
    """all-zero (no sample anywhere) and all-ones (every cell of the box occupied) bitfields"""
    bits = torch.full_like(scene["full"], fill)
    ro, rd = _sub(scene, 700, 7)
    loop, fused = pair(nets[precision], bits, ro, rd, max_steps=24)
    assert_same(loop, fused)
    assert (int(loop["ray_counts"].sum()) == 0) == (fill == 0)


@pytest.mark.parametrize("precision", NETS)
def test_fused_two_cascades(nets, scene, precision):
    """bound = 2: cascade level 1 (the ellipsoid at twice the size, with holes) around level 0"""
    bits = torch.cat([scene["full"], scene["holes"]])
    ro, rd = _sub(scene, 1200, 9)
    loop, fused = pair(nets[precision], bits, ro, rd, ctor=dict(bound=2.0), max_steps=64)
    assert_same(loop, fused)
    assert int(loop["ray_counts"].max()) > 16


@pytest.mark.parametrize("precision", NETS)
@pytest.mark.parametrize("bg", ["scalar", "tensor"])
def test_fused_background(nets, scene, precision, bg):
    ro, rd = _sub(scene, 900, 13)
    g = torch.Generator().manual_seed(17)
    bgc = 0.3 if bg == "scalar" else torch.rand(900, 3, generator=g).cuda()
    loop, fused = pair(nets[precision], scene["holes"], ro, rd, max_steps=32, bg_color=bgc)
    assert_same(loop, fused)
    assert not torch.equal(fused["image"], fused["image_raw"])


@pytest.mark.parametrize("precision", NETS)
@pytest.mark.parametrize("cap", ["reference", "per_ray"])
def test_fused_writes_every_output_element(nets, scene, precision, cap):
    """the output buffers are prefilled with NaN before the call; compared with loop mode (under cap "per_ray" with the loop whose
    cap is per ray as well: the schedule (1, 1))"""
    from lzzx_nerf_amd.ngp import HashgridRenderer
    ro, rd = _sub(scene, 37 * 29, 21)
    loop = HashgridRenderer(nets[precision], scene["holes"], bound=1.0, mode="loop", n_step_cap=8 if cap == "reference" else 1)
    want = {k: v.clone() for k, v in loop.render(ro, rd, max_steps=16, count_samples=True).items()}
    r = HashgridRenderer(nets[precision], scene["holes"], bound=1.0, mode="fused", cap=cap)
    r.render(ro, rd, max_steps=16, count_samples=True)          # allocates the buffers that are then poisoned
    for k in ("out", "image", "weights_sum", "depth"):
        r._fbuf[k].fill_(float("nan"))
    r._fbuf["ray_counts"].fill_(-12345)
    o = r.render(ro, rd, max_steps=16, count_samples=True)
    torch.cuda.synchronize()
    for k in KEYS:
        assert not bool(torch.isnan(o[k].float()).any()), k
    assert_same(want, o)


# ---- 3. same object, two frames -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", NETS)
def test_fused_no_state_leaks_between_frames(nets, scene, precision):
    from lzzx_nerf_amd.ngp import HashgridRenderer
    r = HashgridRenderer(nets[precision], scene["holes"], bound=1.0, mode="fused")
    a_rays, b_rays = _sub(scene, 1000, 31), _sub(scene, 1000, 32)
    a0 = {k: v.clone() for k, v in r.render(*a_rays, max_steps=16, count_samples=True).items()}
    b0 = {k: v.clone() for k, v in r.render(*b_rays, max_steps=16, count_samples=True).items()}
    a1 = r.render(*a_rays, max_steps=16, count_samples=True)
    torch.cuda.synchronize()
    assert_same(a0, a1)
    assert not torch.equal(a0["image"], b0["image"])


# ---- 4. cap = "per_ray" ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", NETS)
def test_fused_per_ray_cap(nets, scene, precision):
    """cap "per_ray" stops a ray alive at max_steps there.  Against the loop under the reference's schedule: equal on every ray the loop
    marches fewer than max_steps samples on -- in this frame (48 x 48 camera rays at the full ellipsoid, max_steps 16: case B's frame, where
    476 of the 2 304 rays stand at the cap) the rays that miss the object or saturate early, 0.79 of the frame (at least half is asserted; the
    share is printed).  Against the loop under the schedule (1, 1), whose cap is per ray as well: equal on every ray, counts included."""
    from lzzx_nerf_amd.ngp import HashgridRenderer
    ms = 16
    ro, rd = scene["ro"], scene["rd"]
    rend = lambda **kw: {k: v.clone() for k, v in HashgridRenderer(nets[precision], scene["full"], bound=1.0, **kw).render(
        ro, rd, max_steps=ms, count_samples=True).items()}
    loop, fused, loop11 = rend(mode="loop"), rend(mode="fused", cap="per_ray"), rend(mode="loop", n_step_cap=1)
    torch.cuda.synchronize()
    below = loop["ray_counts"] < ms
    share = float(below.float().mean())
    print("rays below the cap: %.3f of %d" % (share, below.numel()))
    assert 0.5 <= share <= 0.9
    for k in ("image", "image_raw", "weights_sum", "depth"):
        assert torch.equal(loop[k][below], fused[k][below]), k
    assert_same(loop11, fused)
    assert int(fused["ray_counts"].max()) == ms


# ---- 5. the C entry: documented codes (one GPU test, in the style of test_gpu_empty_batches.py) -----------------------------------------
def test_c_entry_null_and_empty_descriptors():
    from lzzx_nerf_amd import _lib
    lib = _lib.load()
    assert lib.lz_ngp_frame_render(None, None, None) == -2
    f = _lib.FrameNgpFused()
    assert lib.lz_ngp_frame_render(C.byref(f), None, None) == 0                      # N == 0: LZ_OK, nothing launched
    state = torch.full((1024,), 7, dtype=torch.int32, device="cuda")
    f.state = state.data_ptr()
    assert lib.lz_ngp_frame_render(C.byref(f), None, None) == 0
    torch.cuda.synchronize()
    assert int(state.abs().sum()) == 0                                                # "done, no samples"
    f.N = 4
    assert lib.lz_ngp_frame_render(C.byref(f), None, None) == -2   # incomplete
    f.N, f.precision = 0, 2
    assert lib.lz_ngp_frame_render(C.byref(f), None, None) == -2
    f.precision, f.cap_mode, f.max_steps = 0, 1, 4097
    assert lib.lz_ngp_frame_render(C.byref(f), None, None) == -1    # as lz_frame_render refuses it
    torch.cuda.synchronize()
