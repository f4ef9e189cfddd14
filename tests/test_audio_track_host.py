"""CPU: the host index table of the whole-track audio encoder (pipeline.audio_track_windows) reproduces pipeline.audio_window for every
frame, and the clip front end's entry points are declared, bound and exported."""
import ctypes

import pytest
import torch

NEW = ("lz_audio_track_workspace", "lz_audio_encode_track", "lz_torso_anchor_encode_batch", "lz_torso_forward_mixed")


@pytest.mark.parametrize("att_mode", [0, 1, 2])
@pytest.mark.parametrize("T", [1, 3, 8, 13])
def test_track_windows_reproduce_audio_window(T, att_mode):
    from lzzx_nerf_amd.pipeline import audio_track_windows, audio_window
    features = (torch.arange(T, dtype=torch.float32) + 1)[:, None, None].expand(T, 5, 16).contiguous()   # row r holds r + 1 throughout
    table = audio_track_windows(T, att_mode)
    assert table.dtype == torch.int64 and tuple(table.shape) == (T, 1 if att_mode == 0 else 8)
    assert int(table.min()) >= 0 and int(table.max()) <= T
    padded = torch.cat([features, torch.zeros(1, 5, 16)])
    for i in range(T):
        assert torch.equal(padded[table[i]], audio_window(features, att_mode, i)), (T, att_mode, i)


def test_track_windows_reject_other_modes():
    from lzzx_nerf_amd.pipeline import audio_track_windows
    with pytest.raises(NotImplementedError):
        audio_track_windows(4, 3)


def test_new_symbols_are_bound_and_exported():
    from lzzx_nerf_amd import _lib
    from lzzx_nerf_amd import build as B
    for n in NEW:
        assert n in _lib.ALL_SYMBOLS, n
    lib = ctypes.CDLL(B.build())     # python -m lzzx_nerf_amd.build: a no-op when the library is up to date
    for n in NEW:
        assert hasattr(lib, n), n
    ws = _lib.load().lz_audio_track_workspace
    # a zeroed window, count + 8 rows of codes, and for wide inputs as many rows of the first layer's 256 outputs
    assert ws(100, 29, 32) == 4 * (29 * 16 + 108 * 32)
    assert ws(100, 1024, 32) == 4 * (1024 * 16 + 108 * 32 + 108 * 256)


def test_track_guards_need_no_device():
    """count 0 is a no-op before any pointer is looked at; a range outside the track and an unknown att_mode are argument errors"""
    import ctypes as C
    from lzzx_nerf_amd import _lib
    lib = _lib.load()
    p = _lib.AudioParams()
    fake = C.c_void_p(0x10000)
    assert lib.lz_audio_encode_track(C.byref(p), None, 0, 2, 0, 0, 0.0, 0.0, None, None, None, None) == 0
    assert lib.lz_audio_encode_track(C.byref(p), fake, 4, 2, 2, 3, 0.0, 0.0, None, fake, fake, None) == -2      # start + count > T
    assert lib.lz_audio_encode_track(C.byref(p), fake, 4, 3, 0, 4, 0.0, 0.0, None, fake, fake, None) == -1      # att_mode 3
