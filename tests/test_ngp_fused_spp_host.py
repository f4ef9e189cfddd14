"""HashgridRenderer(mode="fused", steps_per_pass=S) / lz_ngp_frame_render_spp (csrc/lz_ngp_frame_spp.hip): what can be checked without
a GPU -- the declared / exported / bound symbol, refusals that return before any launch, argument validation, the register and LDS
report of the twelve new kernels, and that the three S = 1 kernels are still three."""
import ctypes as C
import json
import os

import pytest
import torch

SYMBOL = "lz_ngp_frame_render_spp"


def _renderer(**kw):
    from lzzx_nerf_amd.ngp import HashgridRenderer
    return HashgridRenderer(None, torch.zeros(128 ** 3 // 8, dtype=torch.uint8), **kw)


def _resources():
    from lzzx_nerf_amd import build as B
    if not os.path.exists(B.RESOURCES) or not B.up_to_date():
        B.build(force=True)
    return json.load(open(B.RESOURCES))


def test_symbol_declared_exported_bound():
    from test_cabi import _declared
    from lzzx_nerf_amd import _lib, build as B
    assert SYMBOL in _declared() and SYMBOL in _lib.ALL_SYMBOLS
    assert hasattr(C.CDLL(_lib.SO_PATH), SYMBOL)
    assert "lz_ngp_frame_spp.hip" in B.SOURCES and "lz_ngp_frame.hip" in B.SOURCES
    lib = _lib.load()
    assert lib.lz_abi_version() == 11
    assert list(getattr(lib, SYMBOL).argtypes)[1] is C.c_uint32


@pytest.mark.parametrize("bad", [3, 32, 17])
def test_bad_steps_per_pass_is_refused_before_any_launch(bad):
    from lzzx_nerf_amd import _lib
    lib = _lib.load()
    f = _lib.FrameNgpFused()
    f.N = 16                                                          # (null buffers: a launch would have been refused for those instead)
    for desc in (C.byref(f), None):
        assert lib.lz_ngp_frame_render_spp(desc, bad, None, None) == -2
        assert "steps_per_pass" in lib.lz_last_error().decode()


@pytest.mark.parametrize("S", [0, 1, 2, 4, 8, 16])
def test_empty_and_null_descriptors(S):
    from lzzx_nerf_amd import _lib
    lib = _lib.load()
    f = _lib.FrameNgpFused()
    assert lib.lz_ngp_frame_render_spp(C.byref(f), S, None, None) == 0        # N == 0 (and no state buffer): nothing to do
    assert lib.lz_ngp_frame_render_spp(None, S, None, None) == -2
    assert "steps_per_pass" not in lib.lz_last_error().decode()
    f.N = 16
    assert lib.lz_ngp_frame_render_spp(C.byref(f), S, None, None) == -2       # null buffers, as lz_ngp_frame_render
    f.N, f.cap_mode, f.max_steps = 0, 1, 4097
    assert lib.lz_ngp_frame_render_spp(C.byref(f), S, None, None) == -1       # LZF_CAP_MAX_STEPS, as lz_ngp_frame_render


def test_steps_per_pass_is_validated_at_construction():
    for bad in (3, 32, 17, -1, 2.5, "4", None, True):
        with pytest.raises(ValueError, match="steps_per_pass"):
            _renderer(mode="fused", steps_per_pass=bad)
    for S in (0, 2, 4, 8, 16):
        assert _renderer(mode="fused", steps_per_pass=S).steps_per_pass == S
        with pytest.raises(ValueError, match="steps_per_pass"):
            _renderer(mode="loop", steps_per_pass=S)                  # the loop has its own schedule
        with pytest.raises(ValueError, match="steps_per_pass"):
            _renderer(steps_per_pass=S)
    assert _renderer().steps_per_pass == 1 and _renderer(mode="loop", steps_per_pass=1).mode == "loop"
    r = _renderer(mode="fused")
    assert r.steps_per_pass == 1 and r.last_steps_per_pass is None    # the default keeps the S = 1 kernels


def test_to_inference_passes_steps_per_pass_through():
    from lzzx_nerf_amd.ngp_train import FusedHashgridTrainNeRF
    net = FusedHashgridTrainNeRF()
    bits = torch.zeros(128 ** 3 // 8, dtype=torch.uint8)
    r = net.to_inference(mode="fused", density_bitfield=bits, steps_per_pass=8)
    assert (r.mode, r.steps_per_pass) == ("fused", 8)
    assert net.to_inference(precision="f16", mode="fused", density_bitfield=bits, steps_per_pass=0).steps_per_pass == 0
    assert net.to_inference(mode="fused", density_bitfield=bits).steps_per_pass == 1
    with pytest.raises(ValueError, match="steps_per_pass"):
        net.to_inference(mode="fused", density_bitfield=bits, steps_per_pass=3)
    with pytest.raises(ValueError, match="steps_per_pass"):
        net.to_inference(density_bitfield=bits, steps_per_pass=4)    # mode "loop"


def test_new_kernels_have_no_spills_no_scratch_and_fit_the_lds():
    res = _resources()["lz_ngp_frame_spp.hip"]
    want = {"_Z18lz_k_ngp_frame_sppILi%dE%sLi%dEEv14LzNgpFrameArgs8LzFrameK" % (prec, tt, S)
            for prec, tt in ((0, "f"), (1, "6__half"), (0, "6__half")) for S in (2, 4, 8, 16)}
    assert set(res) == want and len(res) == 12
    for name, r in res.items():
        assert r.get("vgpr_spill", 0) == 0 and r.get("scratch", 0) == 0 and r["lds"] <= 163840, (name, r)
        assert r["occupancy"] >= 2, (name, r)          # the bar of the S = 1 siblings (test_ngp_fused_host.py), for the same reason


def test_the_one_sample_kernels_are_still_three():
    res = _resources()["lz_ngp_frame.hip"]
    assert sorted(res) == ["_Z14lz_k_ngp_frameILi0E6__halfEv14LzNgpFrameArgs8LzFrameK", "_Z14lz_k_ngp_frameILi0EfEv14LzNgpFrameArgs8LzFrameK",
                           "_Z14lz_k_ngp_frameILi1E6__halfEv14LzNgpFrameArgs8LzFrameK"]
    for name, r in res.items():
        assert r.get("vgpr_spill", 0) == 0 and r.get("scratch", 0) == 0 and r["occupancy"] >= 2, (name, r)
