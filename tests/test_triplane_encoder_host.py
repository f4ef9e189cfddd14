"""Host side of the three-plane encoder (csrc/lz_triplane_enc.hip, gridencoder.TriplaneEncoder): exported symbols and their binding, the
kernels' register report, the argument checks of the C entries and the module's configuration check.  No GPU: nothing here gets as far
as a launch."""
import ctypes as C
import json
import os

import pytest
import torch

from lzzx_nerf_amd import _lib, gridencoder
from lzzx_nerf_amd.gridencoder import GridEncoder, TriplaneEncoder

NEW = ("lz_triplane_encode_forward", "lz_triplane_encode_backward", "lz_grid_encode_backward_ordered_strided")
PLANE = dict(input_dim=2, num_levels=12, level_dim=1, base_resolution=64, log2_hashmap_size=14, desired_resolution=512)


def test_library_exports_and_binds_the_new_entries():
    raw = C.CDLL(_lib.SO_PATH)
    bound = _lib.load()
    for name in NEW:
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES and name in _lib.ALL_SYMBOLS, name
        assert getattr(bound, name).argtypes == _lib.SIGNATURES[name], name
    assert bound.lz_abi_version() == _lib.ABI_VERSION == 11


def test_header_cites_the_reference_lines_it_replaces():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "include", "lzzx_nerf_hip.h")).read()
    i = src.index("int lz_triplane_encode_forward(")
    comment = src[src.rindex("/*", 0, i):i]
    assert "network.py:208-223" in comment and "grid.py:18-84" in comment


def test_new_kernels_use_no_scratch_and_spill_nothing():
    from lzzx_nerf_amd import build as B
    if not os.path.exists(B.RESOURCES) or not B.up_to_date():
        B.build(force=True)
    assert "lz_triplane_enc.hip" in B.SOURCES
    res = json.load(open(B.RESOURCES))["lz_triplane_enc.hip"]
    for prefix, count in (("_Z20lz_k_triplane_encodeILb", 2), ("_Z29lz_k_triplane_encode_backward", 1), ("_Z28lz_k_triplane_input_backward", 1)):
        names = [k for k in res if k.startswith(prefix)]
        assert len(names) == count, (prefix, sorted(res))
        for k in names:
            r = res[k]
            assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, (k, r)


def _args(name, pointers, over):
    at = _lib.SIGNATURES[name]
    args = [pointers if a is _lib.vp else (a(4) if a in (_lib.u32, _lib.i32) else a(1.0)) for a in at]
    for i, v in over.items():
        args[i] = at[i](v)
    return args


def _run(name, over, pointers=C.c_void_p(0x10000)):
    lib = _lib.load()
    rc = getattr(lib, name)(*_args(name, pointers, over))
    return rc, lib.lz_last_error().decode()


FWD = {7: 4, 8: 12, 9: 0.2, 10: 64, 11: 1.0}     # B, L, S, H, bound
BWD = {8: 4, 9: 12, 10: 0.2, 11: 64, 12: 1.0}
STRIDED = {1: 36, 5: 4, 6: 2, 7: 1, 8: 12, 9: 0.2, 10: 64, 11: 0, 12: 0, 14: 1 << 20, 15: 0}


@pytest.mark.parametrize("name,base", [("lz_triplane_encode_forward", FWD), ("lz_triplane_encode_backward", BWD),
                                       ("lz_grid_encode_backward_ordered_strided", STRIDED)])
def test_zero_samples_and_null_arrays(name, base):
    at = _lib.SIGNATURES[name]
    lib = _lib.load()
    zero = dict(base)
    zero[[i for i, a in enumerate(at) if a is _lib.u32][0 if name != "lz_grid_encode_backward_ordered_strided" else 1]] = 0     # B
    assert getattr(lib, name)(*_args(name, None, zero)) == 0
    rc, msg = _run(name, base, pointers=None)
    assert rc == -2 and "null tensor" in msg, (rc, msg)


@pytest.mark.parametrize("name,over", [
    ("lz_triplane_encode_forward", {8: 0}), ("lz_triplane_encode_forward", {8: 17}), ("lz_triplane_encode_forward", {10: 0}),
    ("lz_triplane_encode_forward", {11: 0.0}), ("lz_triplane_encode_forward", {11: -1.0}), ("lz_triplane_encode_forward", {11: float("inf")}),
    ("lz_triplane_encode_forward", {11: float("nan")}), ("lz_triplane_encode_forward", {5: 0x10004}), ("lz_triplane_encode_forward", {7: 0xFFFFFFFF}),
    ("lz_triplane_encode_backward", {9: 0}), ("lz_triplane_encode_backward", {9: 17}), ("lz_triplane_encode_backward", {11: 0}),
    ("lz_triplane_encode_backward", {12: 0.0}), ("lz_triplane_encode_backward", {4: None}), ("lz_triplane_encode_backward", {6: None}),
    ("lz_triplane_encode_backward", {7: None}), ("lz_triplane_encode_backward", {3: None, 4: None, 5: None, 6: None, 7: None}),
    ("lz_grid_encode_backward_ordered_strided", {1: 11}), ("lz_grid_encode_backward_ordered_strided", {1: 37, 7: 2, 8: 6}),
    ("lz_grid_encode_backward_ordered_strided", {6: 4}), ("lz_grid_encode_backward_ordered_strided", {7: 3, 1: 36}),
    ("lz_grid_encode_backward_ordered_strided", {14: 64}),
])
def test_unsupported_arguments_come_back_as_argument_errors(name, over):
    """fake non-null pointers and no device: a call that reached a launch would report a HIP error instead"""
    base = dict({"lz_triplane_encode_forward": FWD, "lz_triplane_encode_backward": BWD, "lz_grid_encode_backward_ordered_strided": STRIDED}[name])
    base.update(over)
    rc, msg = _run(name, base)
    assert rc in (-1, -2), (name, over, rc, msg)
    assert msg and not any(w in msg.lower() for w in ("launch failed", "rocm-capable", "hip error")), msg


def _planes(**over):
    kw = dict(PLANE)
    kw.update(over)
    return GridEncoder(**kw)


@pytest.mark.parametrize("field,bad", [
    ("num_levels", dict(num_levels=8)), ("level_dim", dict(level_dim=2)), ("input_dim", dict(input_dim=3)),
    ("base_resolution", dict(base_resolution=32)), ("per_level_scale", dict(desired_resolution=1024)), ("offsets", dict(log2_hashmap_size=13)),
    ("gridtype", dict(gridtype="tiled")), ("align_corners", dict(align_corners=True)), ("num_levels", dict(num_levels=17)),
])
@pytest.mark.parametrize("slot", [0, 2])
def test_mismatched_encoders_are_rejected_by_field(field, bad, slot):
    encs = [_planes(), _planes(), _planes()]
    encs[slot] = _planes(**bad)
    with pytest.raises(RuntimeError, match=field):
        TriplaneEncoder(*encs)


def test_half_tables_are_rejected_at_the_call():
    encs = [_planes(), _planes().half(), _planes()]
    tri = TriplaneEncoder(*encs)
    with pytest.raises(RuntimeError, match="dtype"):
        tri(torch.zeros(4, 3))


def test_no_cpu_fallback():
    tri = TriplaneEncoder(_planes(), _planes(), _planes())
    with pytest.raises(RuntimeError, match="CUDA"):
        tri(torch.zeros(4, 3))


def test_holding_the_encoders_adds_nothing_to_the_enclosing_module():
    class Net(torch.nn.Module):
        def __init__(self, fused):
            super().__init__()
            self.encoder_xy, self.encoder_yz, self.encoder_xz = _planes(), _planes(), _planes()
            self.sigma = torch.nn.Linear(36, 4)
            if fused:
                self.encoder_xyz = TriplaneEncoder(self.encoder_xy, self.encoder_yz, self.encoder_xz)

    plain, fused = Net(False), Net(True)
    assert list(fused.state_dict().keys()) == list(plain.state_dict().keys())
    assert [n for n, _ in fused.named_parameters()] == [n for n, _ in plain.named_parameters()]
    assert [n for n, _ in fused.named_buffers()] == [n for n, _ in plain.named_buffers()]
    assert list(fused.encoder_xyz.parameters()) == [] and list(fused.encoder_xyz.state_dict()) == []
    assert fused.encoder_xyz.encoders[0] is fused.encoder_xy and fused.encoder_xyz.encoders[2] is fused.encoder_xz
    assert fused.encoder_xyz.output_dim == 36
    fused.load_state_dict(plain.state_dict())           # strict: the key sets agree both ways


def test_dropin_reexports_the_module():
    from lzzx_nerf_amd.dropin import gridencoder as D
    from lzzx_nerf_amd.dropin.gridencoder import grid as G
    assert D.TriplaneEncoder is gridencoder.TriplaneEncoder and G.TriplaneEncoder is gridencoder.TriplaneEncoder
