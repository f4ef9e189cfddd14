"""The f32 frame kernel's per-ray SH partial of colour_net.0 (lz_k_frame_c1sh: k-steps 0..3 once per ray, the slice resumes the chain at
k-step 4) and sigma_net.0's eye column on the VALU (lz_head_slice.h) change no bit: the fused frame against the multi-launch loop (whose
stand-alone head runs the full colour_net.0 per sample) and the CPU checker, with and without the eye input, at every samples-per-pass,
under the reference's cap with phase 2 and as deferred-finish tiles, with fold_geo, and on ray counts that leave partial 16-ray tiles."""
import numpy as np
import pytest
import torch

from conftest import ellipsoid_bitfield, synthetic_camera
from oracle.head import TriplaneSpec
from oracle.render import render_inference

pytestmark = pytest.mark.gpu
KEYS = ("image", "image_raw", "weights_sum", "depth", "amb_aud_sum", "amb_eye_sum", "uncertainty_sum", "nears", "fars", "ray_counts")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _setup(params, golden, H, W, fold_geo=False):
    from lzzx_nerf_amd.head import FusedTriplaneHead
    from lzzx_nerf_amd.utils import frame_rays
    head = FusedTriplaneHead({k: torch.from_numpy(v) for k, v in params.items()}, bound=1.0, fold_geo=fold_geo)
    pose, intr = synthetic_camera(H, W)
    ro, rd = frame_rays(dev(pose), intr, H, W)
    return head, ro, rd


def _render(head, bits, ro, rd, cond, mode, **kw):
    from lzzx_nerf_amd.renderer import TriplaneRenderer
    S = kw.pop("steps_per_pass", None)
    cap = kw.pop("cap", "reference")
    sched = kw.pop("schedule", (1, 8))
    if mode == "fused":
        r = TriplaneRenderer(head, dev(bits), bound=1.0, mode="fused", cap=cap)
        if S is not None:
            r.steps_per_pass = S
    else:
        r = TriplaneRenderer(head, dev(bits), bound=1.0, budget_factor=sched[0], n_step_cap=sched[1])
    return {k: v.clone() for k, v in r.render(ro, rd, *cond, count_samples=True, **kw).items()}


def _checker(params, golden, ro, rd, bits, eye, sched, **kw):
    st = {}
    ref = render_inference(TriplaneSpec(1.0), params, ro.cpu().numpy(), rd.cpu().numpy(), bits, golden["net_enc_a"], golden["net_ind"],
                           eye, stats=st, budget_factor=sched[0], n_step_cap=sched[1], **kw)
    return ref, st


def _equal(fused, loop):
    for k in KEYS:
        assert torch.equal(fused[k], loop[k]), k


def _equal_checker(fused, ref, st, eye_sum=True):
    for k in ("image", "depth", "weights_sum", "amb_aud_sum", "uncertainty_sum") + (("amb_eye_sum",) if eye_sum else ()):
        assert np.array_equal(fused[k].cpu().numpy(), ref[k]), k
    assert np.array_equal(fused["ray_counts"].cpu().numpy().astype(np.int64), st["samples_per_ray"])


@pytest.mark.parametrize("with_eye", [True, False])
@pytest.mark.parametrize("S", [1, 2, 4, 8, 16])
def test_frame_sh_partial_every_S_with_and_without_eye(params, golden, S, with_eye):
    """per-ray cap under n_step = S against the loop and the checker run with (S, S); without the eye input k-step 17 of sigma_net.0 is
    skipped, with it it runs as one fma per feature"""
    H, W = 40, 48
    head, ro, rd = _setup(params, golden, H, W)
    bits = ellipsoid_bitfield()[0]
    eye = golden["net_eye"] if with_eye else None
    cond = (dev(golden["net_enc_a"]), dev(golden["net_ind"]), None if eye is None else dev(eye))
    kw = dict(max_steps=64)
    fused = _render(head, bits, ro, rd, cond, "fused", steps_per_pass=S, cap="per_ray", **kw)
    loop = _render(head, bits, ro, rd, cond, "loop", schedule=(S, S), **kw)
    _equal(fused, loop)
    # the checker needs the eye input when the weights have the eye column: without it the frame equals the checker fed eye = 0 (sigma_net.0's
    # input 68 is then 0 * eye_att = 0 either way) in everything but the eye attention's own sum, which the head then leaves at 0
    ref, st = _checker(params, golden, ro, rd, bits, eye if with_eye else np.zeros_like(golden["net_eye"]), (S, S), **kw)
    _equal_checker(fused, ref, st, eye_sum=with_eye)
    if not with_eye:
        assert float(fused["amb_eye_sum"].abs().max()) == 0.0
    else:
        assert float(fused["amb_eye_sum"].abs().max()) > 0.0


@pytest.mark.parametrize("S", [1, 4])
def test_frame_sh_partial_reference_cap_phase_2(params, golden, S):
    """cap_mode 1 at max_steps 16 on the ellipsoid: rays stand at the cap and phase 2 continues them from phase 1's partials"""
    head, ro, rd = _setup(params, golden, 64, 64)
    bits = ellipsoid_bitfield()[0]
    cond = (dev(golden["net_enc_a"]), dev(golden["net_ind"]), dev(golden["net_eye"]))
    fused = _render(head, bits, ro, rd, cond, "fused", steps_per_pass=S, max_steps=16)
    loop = _render(head, bits, ro, rd, cond, "loop", max_steps=16)
    _equal(fused, loop)
    ref, st = _checker(params, golden, ro, rd, bits, golden["net_eye"], (1, 8), max_steps=16)
    _equal_checker(fused, ref, st)
    assert int(fused["state"][9]) > 0 and int(fused["ray_counts"].max()) > 16      # phase 2 ran


def test_frame_sh_partial_deferred_finish_tiles(params, golden):
    """defer_finish: each tile's lz_frame_finish computes its own partials for the rays parked at the cap"""
    from lzzx_nerf_amd import dist as D
    from lzzx_nerf_amd.renderer import TriplaneRenderer
    H = W = 48
    head, ro, rd = _setup(params, golden, H, W)
    bits = dev(ellipsoid_bitfield()[0])
    cond = (dev(golden["net_enc_a"]), dev(golden["net_ind"]), dev(golden["net_eye"]))
    ref = TriplaneRenderer(head, bits, bound=1.0).render(ro, rd, *cond, count_samples=True, max_steps=16)
    ref = {k: v.clone() for k, v in ref.items()}
    world, tiles = 3, "interleaved"
    rs, ctxs = [], []
    for g in range(world):
        sf = D.ShardedFrame(H, W, g, world, tiles, device="cuda")
        sf.gatherer = None
        r = sf.configure(TriplaneRenderer(head, bits, bound=1.0, mode="fused"))
        px = sf.pixels
        ctxs.append(r.fused_begin(ro[px].contiguous(), rd[px].contiguous(), *cond, max_steps=16, count_samples=True))
        rs.append(r)
    total = torch.stack([c["hist"] for c in ctxs]).sum(0)
    imgs, cnts = [], []
    for r, c in zip(rs, ctxs):
        c["hist"].copy_(total)
        o = r.fused_finish(c)
        imgs.append(o["image"].clone())
        cnts.append(o["ray_counts"].clone())
    assert torch.equal(D.assemble_frame(torch.cat(imgs), H, W, world, tiles), ref["image"])
    assert torch.equal(D.assemble_frame(torch.cat(cnts)[:, None], H, W, world, tiles)[:, 0], ref["ray_counts"])
    assert int(ref["ray_counts"].max()) > 16


@pytest.mark.parametrize("S", [1, 2])
def test_frame_sh_partial_fold_geo(params, golden, S):
    """precision 2 (fold_geo): its colour_net.0 keeps the SH columns, the partial is the same; the fused frame equals the folded loop"""
    head, ro, rd = _setup(params, golden, 40, 40, fold_geo=True)
    bits = ellipsoid_bitfield()[0]
    cond = (dev(golden["net_enc_a"]), dev(golden["net_ind"]), dev(golden["net_eye"]))
    fused = _render(head, bits, ro, rd, cond, "fused", steps_per_pass=S, max_steps=32)
    loop = _render(head, bits, ro, rd, cond, "loop", max_steps=32)
    _equal(fused, loop)


@pytest.mark.parametrize("H,W,S", [(37, 23, 1), (29, 31, 4), (3, 5, 1)])
def test_frame_sh_partial_ray_count_not_a_multiple_of_16(params, golden, H, W, S):
    """851 / 899 / 15 rays: the partial kernel's last 16-ray tile is partly empty"""
    head, ro, rd = _setup(params, golden, H, W)
    bits = np.full(128 ** 3 // 8, 255, np.uint8)
    cond = (dev(golden["net_enc_a"]), dev(golden["net_ind"]), dev(golden["net_eye"]))
    fused = _render(head, bits, ro, rd, cond, "fused", steps_per_pass=S, max_steps=24)
    loop = _render(head, bits, ro, rd, cond, "loop", max_steps=24)
    _equal(fused, loop)
    ref, st = _checker(params, golden, ro, rd, bits, golden["net_eye"], (1, 8), max_steps=24)
    _equal_checker(fused, ref, st)
