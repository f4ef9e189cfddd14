"""The clip front end: batched anchor encoding, the torso that writes the mixed background, and
TalkingHeadFrame.render_clip -- each bit for bit the per-frame code it stands in for."""
import functools

import numpy as np
import pytest
import torch

from frontends_inputs import camera_set, torso_pixels
from test_audio_oracle import audio_state
from test_gpu_torso import _torso_state

pytestmark = pytest.mark.gpu
F32 = np.float32
dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def _torso(ind_dim=8):
    from lzzx_nerf_amd.torso import FusedTorso
    return FusedTorso({k: torch.from_numpy(v) for k, v in _torso_state(ind_dim).items()}, torso_shrink=0.8)


def test_encode_anchors_equals_encode_anchor():
    torso = _torso()
    poses = camera_set(3)
    poses[1] = poses[1][[1, 0, 2, 3]]          # a pose whose elimination exchanges rows
    assert not np.array_equal(poses[0], poses[2])
    batch = torso.encode_anchors(dev(poses)).cpu().numpy()
    assert batch.shape == (3, 42)
    for k in range(3):
        assert np.array_equal(batch[k:k + 1], torso.encode_anchor(dev(poses[k:k + 1])).cpu().numpy()), k
    assert len({batch[k].tobytes() for k in range(3)}) == 3
    assert tuple(torso.encode_anchors(torch.zeros(0, 4, 4)).shape) == (0, 42)


@pytest.mark.parametrize("N", [600, 17])
@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("bg_kind", ["scalar", "tensor"])
def test_forward_mix_bg_equals_mix_background(bg_kind, masked, N):
    from lzzx_nerf_amd.torso import FusedTorso
    torso = _torso()
    rng = np.random.default_rng(21)
    xy = torso_pixels()[:N]
    G = 32
    yy, xx = np.meshgrid(np.arange(G), np.arange(G), indexing="ij")
    dens = np.exp(-(((xx - 16) / 8.0) ** 2 + ((yy - 20) / 10.0) ** 2)).astype(F32).reshape(-1)
    if masked and N == 600:
        xy = xy.copy()
        xy[64:96] = rng.uniform(0.9, 1.0, (32, 2)).astype(F32)     # two whole 16-pixel slices outside the blob: the wave-uniform early-out
    ind = dev((rng.normal(size=(1, 8)) * 0.1).astype(F32))
    anchor = torso.encode_anchor(dev(camera_set(1)))
    kw = dict(ind_code=ind, density_grid=dev(dens) if masked else None, density_thresh=0.05, enc_anchor=anchor)
    a0, c0, d0 = [t.clone() for t in torso(dev(xy), **kw)]
    bg = 0.25 if bg_kind == "scalar" else dev(rng.uniform(0, 1, (N, 3)).astype(F32))
    ref = FusedTorso.mix_background(a0, c0, torch.full_like(c0, bg) if bg_kind == "scalar" else bg)
    a1, m1, d1 = torso(dev(xy), mix_bg=bg, **kw)
    assert tuple(m1.shape) == (N, 3)
    assert torch.equal(m1, ref) and torch.equal(a1, a0) and torch.equal(d1, d0)
    dropped = (a0 == 0).reshape(-1)
    if masked:
        assert 0 < int(dropped.sum()) < N
        if N == 600:
            assert bool(dropped[64:96].all())
        assert torch.equal(m1[dropped], torch.full_like(c0, bg)[dropped] if bg_kind == "scalar" else bg[dropped])
    else:
        assert not bool(dropped.any())
    assert not torch.equal(m1, c0)


def _frame(params, precision, smooth_lips):
    from conftest import ellipsoid_bitfield
    from lzzx_nerf_amd.pipeline import TalkingHeadFrame
    sd = dict(params)
    sd.update(_torso_state(8))
    sd.update(audio_state(29, 32, True))
    return TalkingHeadFrame({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, dev(ellipsoid_bitfield()[0]), bound=1.0,
                            precision=precision, smooth_lips=smooth_lips, mode="fused")


KEYS = ("enc_a", "torso_alpha", "torso_color", "image", "image_rgb24")


@pytest.mark.parametrize("smooth_lips", [False, True])
@pytest.mark.parametrize("precision", ["f32", "f16"])
@pytest.mark.parametrize("max_steps", [16, 32])
def test_render_clip_equals_stepped_render(params, golden, max_steps, precision, smooth_lips):
    from conftest import synthetic_camera
    from lzzx_nerf_amd.pipeline import audio_window
    from lzzx_nerf_amd.synthetic import orbit_pose
    from lzzx_nerf_amd.utils import frame_rays
    H = W = 24
    K, T, first = 4, 6, 1
    _, intr = synthetic_camera(H, W)
    poses = dev(np.stack([orbit_pose(10 * k) for k in range(K + 1)]))
    rng = np.random.default_rng(31)
    feats = dev(rng.normal(size=(T, 29, 16)).astype(F32))
    eyes = dev(rng.uniform(0, 1, (K + 1, 1)).astype(F32))
    ys, xs = np.meshgrid(np.linspace(-1, 1, H, dtype=F32), np.linspace(-1, 1, W, dtype=F32), indexing="ij")
    bgc = dev(np.stack([xs.ravel(), ys.ravel()], 1).astype(F32))
    ind, ind_t = dev(golden["net_ind"]), dev((rng.normal(size=(1, 8)) * 0.1).astype(F32))

    def step(frame, k):
        ro, rd = frame_rays(poses[k], intr, H, W)
        return frame.render(ro, rd, audio_window(feats, 2, first + k), eye=eyes[k], ind_code=ind, bg_coords=bgc, poses=poses[k:k + 1],
                            ind_code_torso=ind_t, bg_color=1.0, max_steps=max_steps, rgb24=True)

    stepped, clip = _frame(params, precision, smooth_lips), _frame(params, precision, smooth_lips)
    ref = [{k: v.clone() for k, v in step(stepped, k).items()} for k in range(K)]
    n = 0
    for k, out in enumerate(clip.render_clip(poses[:K], intr, H, W, feats, 2, first_index=first, eyes=eyes, ind_code=ind, ind_code_torso=ind_t,
                                             bg_coords=bgc, bg_color=1.0, max_steps=max_steps, rgb24=True)):
        assert set(out) == set(ref[k])
        for key in KEYS:
            assert out[key].shape == ref[k][key].shape and out[key].dtype == ref[k][key].dtype, (k, key)
            assert torch.equal(out[key], ref[k][key]), (k, key)
        n += 1
    assert n == K
    assert not torch.equal(ref[0]["image"], ref[K - 1]["image"]) and not torch.equal(ref[0]["torso_color"], ref[K - 1]["torso_color"])
    if smooth_lips:
        assert torch.equal(clip._enc_a_prev, stepped._enc_a_prev)
    else:
        assert clip._enc_a_prev is None
    # the state is handed on: one more per-frame step after the clip equals the stepped object's next frame
    a, b = step(clip, K), step(stepped, K)
    for key in KEYS:
        assert torch.equal(a[key], b[key]), key
    clip.reset()
    assert clip._enc_a_prev is None
