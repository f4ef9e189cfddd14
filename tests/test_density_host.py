"""NeRFNetwork.density on the fused head (csrc/lz_density.hip): what can be checked without a GPU -- the two entries are declared, exported
and bound under the unchanged ABI version, they reject bad arguments before any launch, and a cross-compiled build gives the new kernels
no more spilled registers than the forward kernel of the same precision, inside the forward's launch bounds."""
import ctypes as C
import json
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("lz_triplane_head_density", "lz_triplane_density_lattice")
FWD = {"f32": "_Z18lz_k_triplane_headILb0ELb0EE", "f16": "_Z23lz_k_triplane_head_f16w"}       # lz_k_triplane_head<false, false> and its f16 twin
NEW = {"f32": "_Z21lz_k_triplane_densityIL", "f16": "_Z26lz_k_triplane_density_f16wIL"}


def test_entries_are_declared_exported_and_bound():
    from lzzx_nerf_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lzzx_nerf_hip.h")).read(), flags=re.S)
    raw = C.CDLL(_lib.SO_PATH)
    lib = _lib.load()
    for name in ENTRIES:
        assert re.search(r"^\s*int\s+%s\s*\(" % name, hdr, flags=re.M), name
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES and getattr(lib, name).argtypes == _lib.SIGNATURES[name], name
    # the binding has one ctypes argument per declared parameter
    for name in ENTRIES:
        decl = re.search(r"int\s+%s\s*\((.*?)\)\s*;" % name, hdr, flags=re.S).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name]), name
    assert re.search(r"#define\s+LZ_LATTICE_CELLS\s+0u", hdr) and re.search(r"#define\s+LZ_LATTICE_AXES\s+1u", hdr)
    assert (_lib.LZ_LATTICE_CELLS, _lib.LZ_LATTICE_AXES) == (0, 1)


def test_abi_version_is_unchanged():
    from lzzx_nerf_amd import _lib
    assert _lib.load().lz_abi_version() == _lib.ABI_VERSION == 11


def _head_params(complete=True):
    from lzzx_nerf_amd import _lib
    p = _lib.HeadParams()
    if complete:
        for f in ("emb_xy", "emb_yz", "emb_xz", "offsets", "packed", "enc_a"):
            setattr(p, f, 0x10000)
    p.bound, p.S, p.H, p.testing, p.precision = 1.0, 0.27, 64, 1, 0
    return p


def test_empty_work_returns_ok_and_bad_arguments_are_rejected_before_any_launch():
    """No device here: a call that got as far as a launch would come back with a HIP error, not LZ_OK / LZ_ERR_BAD_ARGUMENT."""
    from lzzx_nerf_amd import _lib
    lib = _lib.load()
    fake = C.c_void_p(0x10000)
    p = _head_params()
    dens, latt = lib.lz_triplane_head_density, lib.lz_triplane_density_lattice
    CELLS, AXES = _lib.LZ_LATTICE_CELLS, _lib.LZ_LATTICE_AXES
    # zero work: LZ_OK before any pointer is looked at
    assert dens(None, None, 0, None, None, None, None, None, None) == 0
    assert latt(None, CELLS, None, 0, 16, None, 0, None, 0, None, 0, None, None, None, None) == 0
    assert latt(None, CELLS, None, 1, 0, None, 0, None, 0, None, 0, None, None, None, None) == 0
    assert latt(None, AXES, None, 0, 0, None, 4, None, 0, None, 4, None, None, None, None) == 0
    bad = [
        dens(C.byref(p), fake, 4, None, None, fake, None, None, None),                                   # null sigma
        dens(C.byref(p), None, 4, None, fake, fake, None, None, None),                                   # null xyzs
        dens(None, fake, 4, None, fake, fake, None, None, None),                                         # null params
        dens(C.byref(_head_params(False)), fake, 4, None, fake, fake, None, None, None),                 # incomplete params
        latt(C.byref(p), CELLS, None, 1, 16, None, 0, None, 0, None, 0, fake, None, None, None),         # cells without noise
        latt(C.byref(p), CELLS, fake, 1, 16, None, 0, None, 0, None, 0, None, None, None, None),         # no output asked for
        latt(C.byref(p), CELLS, fake, 9, 16, None, 0, None, 0, None, 0, fake, None, None, None),         # cascade > 8
        latt(C.byref(p), CELLS, fake, 1, 1, None, 0, None, 0, None, 0, fake, None, None, None),          # grid_size < 2
        latt(C.byref(p), AXES, None, 0, 0, fake, 4, None, 4, fake, 4, fake, None, None, None),           # axes without Y
        latt(C.byref(p), AXES, None, 0, 0, fake, 2048, fake, 2048, fake, 2048, fake, None, None, None),  # 2^33 points
        latt(C.byref(p), 2, fake, 1, 16, fake, 4, fake, 4, fake, 4, fake, None, None, None),             # unknown source
        latt(C.byref(_head_params(False)), AXES, None, 0, 0, fake, 4, fake, 4, fake, 4, fake, None, None, None),
    ]
    assert bad == [-2] * len(bad), bad
    pbad = _head_params()
    pbad.precision = 3
    assert dens(C.byref(pbad), fake, 4, None, fake, fake, None, None, None) == -2


@pytest.fixture(scope="module")
def resources():
    from lzzx_nerf_amd import build as B
    if not os.path.exists(B.RESOURCES) or not B.up_to_date():
        B.build(force=True)
    return json.load(open(B.RESOURCES))


@pytest.mark.parametrize("prec", ["f32", "f16"])
def test_density_kernels_stay_inside_the_forward_kernels_budget(resources, prec):
    """lz_k_triplane_density* run a prefix of the forward's slice in the forward's workgroup: no more spilled registers than the forward
    kernel of the same build, and registers + LDS that fit its launch bounds (1024 threads = four waves per SIMD: 128 VGPRs; 160 KB)."""
    fwd = [r for src in ("lz_head.hip", "lz_head_f16.hip") for k, r in resources[src].items() if k.startswith(FWD[prec])]
    assert len(fwd) == 1
    fwd = fwd[0]
    new = {k: r for k, r in resources["lz_density.hip"].items() if k.startswith(NEW[prec])}
    assert len(new) == 3, sorted(new)      # rows, rows + geo_feat, lattice
    for k, r in new.items():
        assert r["vgpr_spill"] <= fwd["vgpr_spill"] and r["sgpr_spill"] <= fwd["sgpr_spill"] and r["scratch"] <= fwd["scratch"], (k, r, fwd)
        assert r["vgprs"] + r["agprs"] <= 128 and r["occupancy"] >= 4, (k, r)
        assert r["lds"] <= fwd["lds"] <= 160 * 1024, (k, r)
