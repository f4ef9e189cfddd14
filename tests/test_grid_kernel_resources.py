"""Register budget of the hot grid-encoder kernels, from build.py's per-kernel report (lib/kernel_resources.json): the triplane plane
forward and its training scatter, the cfg2 hash-grid gather (f32 and f16) with its untile pass, and the big-table scatter.  They share
the level, cell and corner helpers of csrc/lz_grid.hip with every other grid kernel, so a change there must not cost any of them a spill,
scratch or a wave."""
import json
import os

import pytest

# mangled prefix: (VGPRs at most, occupancy at least, SGPR spills at most)
BUDGET = {
    "_Z21lz_k_grid_forward_ldsIfLj2ELj1E": (42, 8, 0),            # triplane plane forward
    "_Z21lz_k_grid_forward_lmpIfLj3ELj2E": (36, 8, 0),            # cfg2, f32
    "_Z21lz_k_grid_forward_lmpI6__halfLj3ELj2E": (24, 8, 0),      # cfg2, f16
    "_Z16lz_k_grid_untile": (74, 6, 0),
    "_Z25lz_k_grid_backward_lds_fxILj2ELj1E": (101, 4, 28),       # triplane training scatter
    "_Z25lz_k_grid_backward_lds_fxILj3ELj2E": (37, 8, 0),
    "_Z21lz_k_grid_backward_xcILj3ELj2E": (17, 8, 0),
}


def _grid_resources():
    from lzzx_nerf_amd import build as B
    if not os.path.exists(B.RESOURCES) or not B.up_to_date():
        B.build(force=True)
    return json.load(open(B.RESOURCES))["lz_grid.hip"]


@pytest.mark.parametrize("prefix", sorted(BUDGET))
def test_grid_kernel_registers(prefix):
    res = _grid_resources()
    names = [k for k in res if k.startswith(prefix)]
    assert len(names) == 1, names
    r = res[names[0]]
    vgprs, occupancy, sgpr_spill = BUDGET[prefix]
    assert r.get("vgpr_spill", 0) == 0 and r.get("scratch", 0) == 0, r
    assert r["vgprs"] <= vgprs and r["occupancy"] >= occupancy, r
    assert r.get("sgpr_spill", 0) <= sgpr_spill, r
