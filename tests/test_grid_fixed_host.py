"""The order-free table gradient (csrc/lz_grid_fixed.hip, gridencoder.set_table_grad("fixed")) without a device: the two entry points are
declared, exported and bound, the workspace function grows with its arguments, what the host can see is rejected before any launch, the
Python switch takes the mode, and the kernels neither spill nor use scratch."""
import ctypes as C
import json
import os

import pytest

NEW = ("lz_grid_encode_backward_fixed", "lz_grid_fixed_workspace")
FAKE = 0x10000   # 16-byte aligned, never dereferenced: every case below is rejected (or a no-op) on the host
BIG = 1 << 30


def test_new_symbols_declared_exported_bound():
    from test_cabi import _declared
    from lzzx_nerf_amd import _lib
    names = _declared()
    lib = C.CDLL(_lib.SO_PATH)
    for n in NEW:
        assert n in names and hasattr(lib, n) and n in _lib.ALL_SYMBOLS, n
    assert len(_lib.SIGNATURES["lz_grid_encode_backward_fixed"]) == len(_lib.SIGNATURES["lz_grid_encode_backward_ordered"]) + 1
    assert _lib.load().lz_abi_version() == _lib.ABI_VERSION == 11


def test_workspace_grows_with_its_arguments():
    from lzzx_nerf_amd import _lib
    ws = _lib.load().lz_grid_fixed_workspace
    assert ws(0, 1) == 256 and ws(8, 1) == 256 + 64
    assert ws(1000, 1) < ws(1001, 1) < ws(1001, 2)
    assert ws(6000000, 2) == 256 + 6000000 * 2 * 8            # one int64 per table element: about 100 MB for the cfg2 table
    assert ws((1 << 32) - 1, 2) > 1 << 35                     # no 32-bit wrap
    assert ws(1000, 4) == 0 and ws(1000, 8) == 0 and ws(1000, 0) == 0 and ws(1000, 3) == 0


def _call(null=None, B=64, D=3, C_=2, L=16, emb_f16=0, layout=0, workspace=FAKE, ws_bytes=BIG, stride=0, dy_dx=None, grad_inputs=None):
    from lzzx_nerf_amd import _lib
    names = ["grad", "inputs", "embeddings", "offsets", "grad_embeddings"]
    ptrs = {n: FAKE for n in names}
    if null:
        ptrs[null] = None
    return _lib.load().lz_grid_encode_backward_fixed(ptrs["grad"], ptrs["inputs"], ptrs["embeddings"], ptrs["offsets"], ptrs["grad_embeddings"], B, D, C_,
                                                     L, 1.0, 16, dy_dx, grad_inputs, 0, 0, emb_f16, layout, workspace, ws_bytes & 0xFFFFFFFF,
                                                     ws_bytes >> 32, stride, None)


def _message():
    from lzzx_nerf_amd import _lib
    return _lib.load().lz_last_error().decode()


@pytest.mark.parametrize("null", ["grad", "inputs", "offsets", "grad_embeddings"])
def test_null_tensors_are_rejected_before_any_launch(null):
    assert _call(null) == -2, _message()
    assert "null" in _message()


def test_null_short_and_misaligned_workspaces_are_rejected_before_any_launch():
    from lzzx_nerf_amd import _lib
    assert _call(workspace=None) == -2, _message()
    floor = int(_lib.load().lz_grid_fixed_workspace(8 * 16, 2))        # every level holds at least 8 entries
    assert _call(ws_bytes=floor - 1) == -2, _message()
    assert "lz_grid_fixed_workspace" in _message()
    assert _call(ws_bytes=0) == -2 and _call(ws_bytes=255) == -2
    assert _call(workspace=FAKE + 8) == -2, _message()
    assert "aligned" in _message()


def test_unsupported_shapes_are_rejected_before_any_launch():
    for kw, word in ((dict(D=4), "D must be 2 or 3"), (dict(D=1), "D must be 2 or 3"), (dict(C_=4), "C must be 1 or 2"), (dict(C_=8), "C must be 1 or 2"),
                     (dict(emb_f16=1), "f32 tables only"), (dict(B=1 << 28), "2^31"), (dict(B=1 << 29, D=2), "2^31"), (dict(L=33), "levels")):
        assert _call(**kw) == -1, (kw, _message())
        assert word in _message(), (kw, _message())
    for kw in (dict(layout=2), dict(layout=-1), dict(L=0), dict(grad_inputs=FAKE), dict(stride=31, layout=1), dict(stride=33, layout=1),
               dict(stride=64, layout=0), dict(stride=64, layout=1, dy_dx=FAKE, grad_inputs=FAKE)):
        assert _call(**kw) == -2, (kw, _message())


def test_zero_rows_is_a_no_op():
    assert _call("grad", B=0) == 0
    assert _call(B=0, workspace=None, D=7, C_=5) == 0


def test_switch_round_trips():
    from lzzx_nerf_amd import gridencoder
    from lzzx_nerf_amd.dropin import gridencoder as dropin
    assert "fixed" in gridencoder._TABLE_GRADS and gridencoder.table_grad() == "atomic"
    prev = gridencoder.set_table_grad("fixed")
    try:
        assert prev == "atomic" and gridencoder.table_grad() == "fixed"
        with pytest.raises(ValueError):
            gridencoder.set_table_grad("fixd")
        assert gridencoder.table_grad() == "fixed"
    finally:
        assert gridencoder.set_table_grad(prev) == "fixed"
    assert gridencoder.table_grad() == "atomic"
    assert dropin.grid_backward_fixed is gridencoder.grid_backward_fixed and dropin.set_table_grad is gridencoder.set_table_grad


def test_python_refusals_name_the_modes_that_serve():
    import torch
    from lzzx_nerf_amd import gridencoder
    for D, Cc, dtype, word in ((3, 2, torch.float16, "atomic"), (3, 4, torch.float32, "ordered"), (3, 8, torch.float32, "ordered"),
                               (4, 2, torch.float32, "atomic"), (1, 1, torch.float32, "atomic")):
        with pytest.raises(RuntimeError, match=word):
            gridencoder._check_fixed(D, Cc, dtype)
    gridencoder._check_fixed(2, 1, torch.float32)
    gridencoder._check_fixed(3, 2, torch.float32)


def test_fused_net_constructs_with_the_mode():
    from lzzx_nerf_amd.ngp_train import FusedHashgridTrainNeRF
    assert FusedHashgridTrainNeRF(table_grad="fixed").table_grad == "fixed"
    assert FusedHashgridTrainNeRF().table_grad is None
    with pytest.raises(ValueError):
        FusedHashgridTrainNeRF(table_grad="fixd")


def test_kernels_have_no_spills_or_scratch():
    from lzzx_nerf_amd import build as B
    if not os.path.exists(B.RESOURCES) or not B.up_to_date():
        B.build(force=True)
    res = json.load(open(B.RESOURCES))["lz_grid_fixed.hip"]
    for stem in ("lz_k_grid_fixed_max", "lz_k_grid_fixed_scale", "lz_k_grid_fixed_convert"):
        assert sum(stem in k for k in res) == 1, stem
    for stem in ("lz_k_grid_fixed_scatter", "lz_k_grid_fixed_lds"):
        assert sum(stem in k for k in res) == 4, stem              # D 2 / 3 x C 1 / 2
    for name, r in res.items():
        assert r.get("vgpr_spill", 0) == 0 and r.get("sgpr_spill", 0) == 0 and r.get("scratch", 0) == 0, (name, r)
