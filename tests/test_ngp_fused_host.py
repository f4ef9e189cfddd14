"""HashgridRenderer(mode="fused") / lz_ngp_frame_render (csrc/lz_ngp_frame.hip): what can be checked without a GPU -- argument
refusals, the declared / exported / bound symbol, the register and LDS report of the new kernels, descriptor refusals that
return before any launch."""
import ctypes as C
import json
import os

import pytest
import torch


def _renderer(**kw):
    from lzzx_nerf_amd.ngp import HashgridRenderer
    return HashgridRenderer(None, torch.zeros(128 ** 3 // 8, dtype=torch.uint8), **kw)


def test_mode_and_cap_are_validated_at_construction():
    with pytest.raises(ValueError, match="mode"):
        _renderer(mode="bogus")
    with pytest.raises(ValueError, match="cap"):
        _renderer(cap="bogus")
    with pytest.raises(ValueError, match="cap"):
        _renderer(mode="fused", cap="bogus")
    with pytest.raises(ValueError, match="n_step_cap"):
        _renderer(mode="fused", n_step_cap=4)          # the schedule replay has the reference's step cap
    assert _renderer().mode == "loop" and _renderer().cap == "reference"      # the default stays the loop
    r = _renderer(mode="fused", cap="per_ray", n_step_cap=4, budget_factor=4)
    assert (r.mode, r.cap) == ("fused", "per_ray")


def test_symbol_declared_exported_bound():
    from test_cabi import _declared
    from lzzx_nerf_amd import _lib, build as B
    assert "lz_ngp_frame_render" in _declared() and "lz_ngp_frame_render" in _lib.ALL_SYMBOLS
    assert hasattr(C.CDLL(_lib.SO_PATH), "lz_ngp_frame_render")
    assert "lz_ngp_frame.hip" in B.SOURCES
    assert _lib.load().lz_abi_version() == 11


def test_descriptor_mirror_matches_the_header():
    """field names and order of _lib.FrameNgpFused against the struct in the header"""
    import re
    from lzzx_nerf_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "include", "lzzx_nerf_hip.h")).read()
    body = src[: src.index("} lz_frame_ngp_fused;")]
    body = re.sub(r"/\*.*?\*/", "", body[body.rindex("typedef struct {"):], flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.replace("typedef struct {", "").strip()
        if decl:
            names += [re.sub(r"[^A-Za-z0-9_]", "", part.split()[-1]) for part in decl.split(",")]
    assert names == [n for n, _ in _lib.FrameNgpFused._fields_]


def test_kernels_have_no_spills_no_scratch_and_fit_the_lds():
    from lzzx_nerf_amd import build as B
    if not os.path.exists(B.RESOURCES) or not B.up_to_date():
        B.build(force=True)
    res = json.load(open(B.RESOURCES))["lz_ngp_frame.hip"]
    assert len(res) == 3 and all(k.startswith("_Z14lz_k_ngp_frame") for k in res), sorted(res)
    for name, r in res.items():
        assert r.get("vgpr_spill", 0) == 0 and r.get("scratch", 0) == 0 and r["lds"] <= 163840, (name, r)
        assert r["occupancy"] >= 2, (name, r)          # at least two 256-thread workgroups per SIMD row: a wave's gather latency is covered


def test_refusals_before_any_launch():
    from lzzx_nerf_amd import _lib
    lib = _lib.load()
    assert lib.lz_ngp_frame_render(None, None, None) == -2
    f = _lib.FrameNgpFused()
    assert lib.lz_ngp_frame_render(C.byref(f), None, None) == 0          # N == 0 (and no state buffer): nothing to do
    f.N = 16
    assert lib.lz_ngp_frame_render(C.byref(f), None, None) == -2         # null buffers
    f.precision = 3
    assert lib.lz_ngp_frame_render(C.byref(f), None, None) == -2
    f.precision, f.cap_mode = 0, 2
    assert lib.lz_ngp_frame_render(C.byref(f), None, None) == -2
    f.cap_mode, f.max_steps = 1, 4097
    assert lib.lz_ngp_frame_render(C.byref(f), None, None) == -1         # LZF_CAP_MAX_STEPS, as lz_frame_render


def test_to_inference_passes_the_mode_through():
    from lzzx_nerf_amd.ngp import FusedHashgridNeRF, HashgridRenderer
    from lzzx_nerf_amd.ngp_train import FusedHashgridTrainNeRF
    net = FusedHashgridTrainNeRF()
    bits = torch.zeros(128 ** 3 // 8, dtype=torch.uint8)
    assert isinstance(net.to_inference(), FusedHashgridNeRF)                       # as before: the network alone
    r = net.to_inference(mode="fused", density_bitfield=bits)
    assert isinstance(r, HashgridRenderer) and r.mode == "fused" and r.cap == "reference" and isinstance(r.net, FusedHashgridNeRF)
    r = net.to_inference(precision="f16", mode="fused", density_bitfield=bits, cap="per_ray")
    assert (r.mode, r.cap, r.net.precision) == ("fused", "per_ray", "f16")
    assert net.to_inference(density_bitfield=bits).mode == "loop"
    with pytest.raises(ValueError, match="mode"):
        net.to_inference(mode="bogus", density_bitfield=bits)
