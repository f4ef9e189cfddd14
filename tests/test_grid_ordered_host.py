"""Host side of the ordered table gradient: the module switch, the workspace query and the argument checks of
lz_grid_encode_backward_ordered.  No GPU: nothing here gets as far as a launch."""
import ctypes as C

import pytest

from lzzx_nerf_amd import _lib, gridencoder


def test_set_table_grad_validates_and_returns_the_previous_value():
    assert gridencoder.table_grad() == "atomic"
    assert gridencoder.set_table_grad("ordered") == "atomic"
    try:
        assert gridencoder.table_grad() == "ordered"
        for bad in ("sorted", "", None, 1, "Ordered"):
            with pytest.raises(ValueError):
                gridencoder.set_table_grad(bad)
        assert gridencoder.table_grad() == "ordered"
    finally:
        assert gridencoder.set_table_grad("atomic") == "ordered"
    assert gridencoder.table_grad() == "atomic"


def test_dropin_reexports_the_switch():
    from lzzx_nerf_amd.dropin import gridencoder as D
    from lzzx_nerf_amd.dropin.gridencoder import grid as G
    assert D.set_table_grad is gridencoder.set_table_grad and D.table_grad is gridencoder.table_grad
    assert G.set_table_grad is gridencoder.set_table_grad


def test_fused_net_validates_table_grad():
    from lzzx_nerf_amd.ngp_train import FusedHashgridTrainNeRF
    with pytest.raises(ValueError):
        FusedHashgridTrainNeRF(table_grad="sorted")


def test_workspace_query_is_monotone_and_non_zero():
    ws = _lib.load().lz_grid_ordered_workspace
    for D in (2, 3):
        sizes = [ws(B, D) for B in (1, 2, 63, 64, 65, 257, 4099, 70001, 357000, 1 << 24)]
        assert all(s > 0 for s in sizes)
        assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] < sizes[-1]
        assert ws(70001, D) >= 70001 * (1 << D) * 16          # two (entry, rank) pair buffers
    assert ws(1000, 3) > ws(1000, 2)
    assert ws(1 << 28, 3) > 1 << 32                            # size_t, not 32 bits


def _call(over):
    lib = _lib.load()
    at = _lib.SIGNATURES["lz_grid_encode_backward_ordered"]
    args = [C.c_void_p(0x10000) if a is _lib.vp else (a(4) if a in (_lib.u32, _lib.i32) else a(1.0)) for a in at]
    base = {5: 4, 6: 3, 7: 2, 8: 16, 10: 16, 13: 0, 14: 0, 15: 0, 16: 1, 18: 1 << 20, 19: 0}
    base.update(over)
    for i, v in base.items():
        args[i] = at[i](v)
    return lib.lz_grid_encode_backward_ordered(*args), lib.lz_last_error().decode()


@pytest.mark.parametrize("over", [{6: 1}, {6: 4}, {6: 5}, {6: 0}, {15: 1}, {16: 2}, {16: 3}, {16: -1}, {7: 3}, {7: 16}, {8: 0}, {8: 33}, {10: 0},
                                  {13: 2}, {18: 64}, {18: 0}])
def test_unsupported_arguments_come_back_as_argument_errors(over):
    """fake non-null pointers and no device: a call that reached a launch would report a HIP error instead"""
    rc, msg = _call(over)
    assert rc in (-1, -2), (over, rc, msg)
    assert "grid_encode_backward_ordered" in msg
    assert not any(w in msg.lower() for w in ("launch failed", "rocm-capable", "hip error")), msg


def test_zero_samples_return_before_anything_is_looked_at():
    lib = _lib.load()
    at = _lib.SIGNATURES["lz_grid_encode_backward_ordered"]
    args = [None if a is _lib.vp else a(0) for a in at]
    assert lib.lz_grid_encode_backward_ordered(*args) == 0
