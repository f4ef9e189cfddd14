"""Register and LDS budget of the f32 training head's kernels that run lz_fwd32_chain (csrc/lz_head_fwd32_chain.h): the two recording
forwards (f32 / f16 records) and the backward that recomputes the forward from the positions (record=False), from build.py's per-kernel
report (lib/kernel_resources.json).  The forwards run three waves per SIMD (at most 168 VGPRs), the backwards two (LZ_BWD_WG = 512 with
one workgroup per CU); none may spill a vector register.  The bounds are the numbers of the kernels as they stood when the chain became
one function: a change of the shared chain that costs the recording forward a wave or the recomputing backward a spill fails here."""
import json
import os

import pytest

FWD_REC = {   # name: (VGPRs, SGPRs spilled to VGPR lanes)
    "_Z30lz_k_triplane_head_forward_recILb0EEv10LzHeadArgsPKfS2_jPfS3_S3_S3_S3_S3_S3_": (136, 101),
    "_Z30lz_k_triplane_head_forward_recILb1EEv10LzHeadArgsPKfS2_jPfS3_S3_S3_S3_S3_S3_": (137, 105),
}
# the recomputing f32 backward (<0, 0, 0, 1>).  Its predecessor, a kernel of its own with a second copy of the chains, used 229 VGPRs
# and 110 SGPR spills at the same two waves per SIMD
BWD_XYZ = "_Z31lz_k_triplane_head_backward_recILb0ELb0ELb0ELb1EEv13LzHeadBwdArgsPKfjPf"
LDS = 98816   # bytes: the f32 fragments, the VALU rows and the level table (LzHeadLds<true>::FLOATS)


def _resources():
    from lzzx_nerf_amd import build as B
    if not os.path.exists(B.RESOURCES) or not B.up_to_date():
        B.build(force=True)
    return json.load(open(B.RESOURCES))["lz_head_rec.hip"]


@pytest.mark.parametrize("name", sorted(FWD_REC))
def test_recording_forward_registers_and_lds(name):
    r = _resources()[name]
    vgprs, sgpr_spill = FWD_REC[name]
    assert r.get("vgpr_spill", 0) == 0 and r.get("scratch", 0) == 0, r
    assert r["vgprs"] <= vgprs and r["occupancy"] >= 3, r
    assert r.get("sgpr_spill", 0) <= sgpr_spill, r
    assert r["lds"] <= LDS, r


def test_recomputing_f32_backward_registers_and_lds():
    r = _resources()[BWD_XYZ]
    assert r.get("vgpr_spill", 0) == 0 and r.get("scratch", 0) == 0, r
    assert r["vgprs"] <= 232 and r["occupancy"] >= 2, r
    assert r.get("sgpr_spill", 0) <= 110, r
    assert r["lds"] <= LDS, r
