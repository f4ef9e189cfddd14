"""Whole-track audio encoder (FusedAudioEncoder.encode_track, csrc/lz_audio.hip): the codes of all frames of a clip from one pass over
the feature track, bit for bit the per-frame kernel on pipeline.audio_window of each frame (and the CPU checker on a few of them)."""
import functools

import numpy as np
import pytest
import torch

from test_audio_oracle import audio_state

pytestmark = pytest.mark.gpu
F32 = np.float32
WIN = 8                       # windows per stage-A workgroup (LZ_AUDIO_TRACK_WIN)
LENGTHS = (1, WIN - 1, WIN, WIN + 1, 21)
CASES = [(29, True, 1), (29, True, 2), (1024, True, 1), (1024, True, 2), (29, False, 0)]


@functools.lru_cache(maxsize=None)
def _encoder(dim_in, att):
    from lzzx_nerf_amd.audio import FusedAudioEncoder
    sd = audio_state(dim_in, 32, att)
    return sd, FusedAudioEncoder({k: torch.from_numpy(v) for k, v in sd.items()})


@functools.lru_cache(maxsize=None)
def _track(dim_in, T):
    return torch.from_numpy(np.random.default_rng(100 * dim_in + T).normal(size=(T, dim_in, 16)).astype(F32)).cuda()


@functools.lru_cache(maxsize=None)
def _per_frame(dim_in, att, att_mode, T):
    """the yardstick: the per-frame kernel on every frame's windows, stacked [T, 32] (computed once, shared, read only)"""
    from lzzx_nerf_amd.pipeline import audio_window
    _, enc = _encoder(dim_in, att)
    f = _track(dim_in, T)
    out = torch.cat([enc(audio_window(f, att_mode, i)) for i in range(T)]).cpu().numpy()
    out.setflags(write=False)
    return out


@pytest.mark.parametrize("T", LENGTHS)
@pytest.mark.parametrize("dim_in,att,att_mode", CASES)
def test_track_equals_per_frame_kernel(dim_in, att, att_mode, T):
    from lzzx_nerf_amd.pipeline import audio_window
    from oracle.audio import encode_audio
    sd, enc = _encoder(dim_in, att)
    f = _track(dim_in, T)
    out = enc.encode_track(f, att_mode).cpu().numpy()
    assert out.shape == (T, 32) and out.dtype == F32
    assert np.array_equal(out, _per_frame(dim_in, att, att_mode, T))
    for i in sorted({0, T // 2, T - 1}):
        ref = encode_audio(sd, audio_window(f, att_mode, i).cpu().numpy(), att)
        assert np.array_equal(out[i:i + 1], ref), i


@pytest.mark.parametrize("dim_in,att,att_mode", CASES)
def test_slice_of_the_track(dim_in, att, att_mode):
    _, enc = _encoder(dim_in, att)
    full = _per_frame(dim_in, att, att_mode, 21)
    out = enc.encode_track(_track(dim_in, 21), att_mode, start=5, count=7).cpu().numpy()
    assert np.array_equal(out, full[5:12])
    assert tuple(enc.encode_track(_track(dim_in, 21), att_mode, start=5, count=0).shape) == (0, 32)


def _blend(own, prev):
    """TalkingHeadFrame.render's smooth_lips over the frames, in numpy f32: each product and the sum rounded once"""
    out = np.empty_like(own)
    for k in range(own.shape[0]):
        prev = own[k] if prev is None else F32(0.35) * prev + F32(1 - 0.35) * own[k]
        out[k] = prev
    return out


@pytest.mark.parametrize("dim_in,att,att_mode", [(29, True, 2), (1024, True, 1), (29, False, 0)])
def test_smooth_lips_recurrence(dim_in, att, att_mode):
    _, enc = _encoder(dim_in, att)
    own = _per_frame(dim_in, att, att_mode, 21)
    f = _track(dim_in, 21)
    out = enc.encode_track(f, att_mode, start=5, smooth_lips=True).cpu().numpy()          # no previous code: frame 5 keeps its own
    assert np.array_equal(out, _blend(own[5:], None)) and np.array_equal(out[0], own[5]) and not np.array_equal(out[1], own[6])
    prev = np.random.default_rng(3).normal(size=(1, 32)).astype(F32)
    out = enc.encode_track(f, att_mode, start=5, count=7, smooth_lips=True, enc_a_prev=torch.from_numpy(prev).cuda()).cpu().numpy()
    assert np.array_equal(out, _blend(own[5:12], prev[0]))
    # what the per-frame path computes with torch on the device
    e = torch.from_numpy(prev).cuda()
    for k in range(7):
        e = 0.35 * e + (1 - 0.35) * torch.from_numpy(own[5 + k:6 + k].copy()).cuda()
        assert np.array_equal(out[k:k + 1], e.cpu().numpy()), k
    assert np.array_equal(enc.encode_track(f, att_mode, start=5, count=7).cpu().numpy(), own[5:12])      # off: untouched


def test_shape_and_mode_errors():
    _, enc = _encoder(29, True)
    _, plain = _encoder(29, False)
    f = _track(29, 9)
    with pytest.raises(RuntimeError, match="must be"):
        enc.encode_track(torch.zeros(9, 30, 16), 2)
    with pytest.raises(RuntimeError, match="must be"):
        enc.encode_track(torch.zeros(9, 29, 8), 2)
    with pytest.raises(RuntimeError, match="must be"):
        enc.encode_track(torch.zeros(29, 16), 2)
    with pytest.raises(RuntimeError, match="windows"):
        enc.encode_track(f, 0)                      # an attention net needs its 8 windows
    for mode in (1, 2):
        with pytest.raises(RuntimeError, match="attention"):
            plain.encode_track(f, mode)
    with pytest.raises(RuntimeError):
        enc.encode_track(f, 3)
    with pytest.raises(RuntimeError, match="inside the track"):
        enc.encode_track(f, 2, start=5, count=5)
