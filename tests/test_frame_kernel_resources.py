"""Register and LDS budget of the f32 frame kernels at one sample per ray and pass (the headline launch and its fold_geo twin), from
build.py's per-kernel report (lib/kernel_resources.json): the per-ray SH partial of colour_net.0 is loaded early in the slice and must
not cost a spill or a wave -- at most 128 VGPRs keeps four waves per SIMD -- and the slot fields it replaces leave the LDS smaller."""
import json
import os

import pytest

FRAME_F32_S1 = ["_Z10lz_k_frameILi0ELi1ELi1EEvN7LzfHeadIXT_EE4ArgsE8LzFrameK",
                "_Z10lz_k_frameILi2ELi1ELi1EEvN7LzfHeadIXT_EE4ArgsE8LzFrameK"]
LDS_BEFORE_PARTIAL = 134160        # bytes, with 16 SH words per ray slot in LDS


@pytest.mark.parametrize("name", FRAME_F32_S1)
def test_f32_frame_kernel_registers_and_lds(name):
    from lzzx_nerf_amd import build as B
    if not os.path.exists(B.RESOURCES) or not B.up_to_date():
        B.build(force=True)
    r = json.load(open(B.RESOURCES))["lz_frame.hip"][name]
    assert r.get("vgpr_spill", 0) == 0 and r.get("sgpr_spill", 0) == 0 and r.get("scratch", 0) == 0, r
    assert r["vgprs"] <= 128 and r["occupancy"] >= 4, r
    assert r["lds"] <= LDS_BEFORE_PARTIAL, r
