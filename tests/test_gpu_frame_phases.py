"""The f32 frame kernels' wave priorities and scheduling fences (lz_head_gather.h: LZF_PRIO_TAIL, LZF_PRIO_YOUNG; lz_head_slice.h:
LZ_SLICE_GAP_FENCE) decide WHEN a wave's instructions issue, never what they compute: with the library as built, the fused frame equals
the multi-launch loop bit for bit -- pixels, every per-ray sum and the per-ray sample counts -- on a dense grid at full depth, where the
cap binds and phase 2 runs, on a frame of 35 rays (partly filled waves, several samples per ray and pass), with and without the eye and
ind_code inputs, with the folded head, and on 3 000 rays, where the queue runs dry while other slots of a wave still march.  Each loop
render is made once and shared by the cases that compare against it."""
import numpy as np
import pytest
import torch

from conftest import ellipsoid_bitfield, synthetic_camera

pytestmark = pytest.mark.gpu
KEYS = ("image", "depth", "weights_sum", "amb_aud_sum", "amb_eye_sum", "uncertainty_sum", "ray_counts")
ONES = "ones"
ELLIPSOID = "ellipsoid"
_cache = {}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(scene):
    if ("bits", scene) not in _cache:
        _cache[("bits", scene)] = dev(np.full(128 ** 3 // 8, 255, np.uint8) if scene == ONES else ellipsoid_bitfield()[0])
    return _cache[("bits", scene)]


def _head(params, fold_geo):
    from lzzx_nerf_amd.head import FusedTriplaneHead
    if ("head", fold_geo) not in _cache:
        _cache[("head", fold_geo)] = FusedTriplaneHead({k: torch.from_numpy(v) for k, v in params.items()}, bound=1.0, fold_geo=fold_geo)
    return _cache[("head", fold_geo)]


def _rays(H, W, n_rays=None):
    from lzzx_nerf_amd.utils import frame_rays
    pose, intr = synthetic_camera(H, W)
    ro, rd = frame_rays(dev(pose), intr, H, W)
    ro, rd = ro.reshape(-1, 3), rd.reshape(-1, 3)
    return (ro, rd) if n_rays is None else (ro[:n_rays].contiguous(), rd[:n_rays].contiguous())


def _cond(golden, with_eye, with_ind):
    return (dev(golden["net_enc_a"]), dev(golden["net_ind"]) if with_ind else None, dev(golden["net_eye"]) if with_eye else None)


def _render(params, golden, mode, scene, H, W, max_steps, with_eye=True, with_ind=True, fold_geo=False, n_rays=None, S=0):
    from lzzx_nerf_amd.renderer import TriplaneRenderer
    head = _head(params, fold_geo)
    ro, rd = _rays(H, W, n_rays)
    if mode == "fused":
        r = TriplaneRenderer(head, _bits(scene), bound=1.0, mode="fused")
        r.steps_per_pass = S
    else:
        r = TriplaneRenderer(head, _bits(scene), bound=1.0, budget_factor=1, n_step_cap=8)
    out = r.render(ro, rd, *_cond(golden, with_eye, with_ind), max_steps=max_steps, count_samples=True)
    torch.cuda.synchronize()
    return {k: v.clone() for k, v in out.items()}


def _loop(params, golden, *key, **kw):
    k = ("loop", key, tuple(sorted(kw.items())))
    if k not in _cache:
        _cache[k] = _render(params, golden, "loop", *key, **kw)
    return _cache[k]


def _equal(fused, loop):
    for k in KEYS:
        assert torch.equal(fused[k], loop[k]), k
    assert int(fused["state"][5]) == int(loop["state"][5]) == int(fused["ray_counts"].sum())


@pytest.mark.parametrize("with_eye,with_ind", [(True, True), (True, False), (False, True), (False, False)])
@pytest.mark.parametrize("S", [1, 0])
def test_dense_grid_full_depth(params, golden, S, with_eye, with_ind):
    """48 x 48 rays through the all-ones grid at max_steps 192: every slot of every wave is busy pass after pass (S = 1: the headline
    kernel's shape; S = 0: the samples per pass the renderer picks for 2 304 rays)"""
    case = (ONES, 48, 48, 192)
    kw = dict(with_eye=with_eye, with_ind=with_ind)
    fused = _render(params, golden, "fused", *case, S=S, **kw)
    _equal(fused, _loop(params, golden, *case, **kw))
    assert int(fused["state"][5]) > 48 * 48 * 16
    assert (float(fused["amb_eye_sum"].abs().max()) > 0.0) == with_eye


@pytest.mark.parametrize("with_eye,with_ind", [(True, True), (False, False)])
@pytest.mark.parametrize("S", [1, 0])
def test_cap_binds_and_phase_2_runs(params, golden, S, with_eye, with_ind):
    """the ellipsoid at max_steps 16: rays stand at the cap, phase 2 continues them from phase 1's partials"""
    case = (ELLIPSOID, 48, 48, 16)
    kw = dict(with_eye=with_eye, with_ind=with_ind)
    fused = _render(params, golden, "fused", *case, S=S, **kw)
    _equal(fused, _loop(params, golden, *case, **kw))
    assert int(fused["state"][9]) > 0 and int(fused["ray_counts"].max()) > 16      # phase 2 ran


@pytest.mark.parametrize("scene,max_steps", [(ONES, 192), (ELLIPSOID, 16)])
def test_five_by_seven_frame(params, golden, scene, max_steps):
    """35 rays: one partly filled wave.  With steps_per_pass = 0 the launcher doubles the samples per ray and pass until the rows in flight
    fill the chip or S reaches 16 (lz_frame.hip: lz_frame_render) -- for 35 rays that is lz_k_frame<0, 16, 1>; S = 4 beside it"""
    case = (scene, 5, 7, max_steps)
    for S in (0, 4):
        _equal(_render(params, golden, "fused", *case, S=S), _loop(params, golden, *case))


@pytest.mark.parametrize("S", [1, 0])
@pytest.mark.parametrize("scene,max_steps", [(ONES, 48), (ELLIPSOID, 16)])
def test_folded_head_against_its_own_loop(params, golden, scene, max_steps, S):
    case = (scene, 40, 40, max_steps)
    fused = _render(params, golden, "fused", *case, fold_geo=True, S=S)
    _equal(fused, _loop(params, golden, *case, fold_geo=True))


@pytest.mark.parametrize("S", [1, 0])
def test_three_thousand_rays_slots_run_dry_in_mid_wave(params, golden, S):
    """3 000 rays of a 64 x 64 frame through the ellipsoid: fewer rays than the kernel has slots for, rays of very different lengths -- the
    queue is dry while other slots of the same wave still march; the sample total in `state` equals the loop's"""
    case = (ELLIPSOID, 64, 64, 64)
    fused = _render(params, golden, "fused", *case, n_rays=3000, S=S)
    loop = _loop(params, golden, *case, n_rays=3000)
    _equal(fused, loop)
    assert fused["ray_counts"].shape[0] == 3000
    assert int(fused["state"][5]) == int(loop["state"][5]) > 3000
