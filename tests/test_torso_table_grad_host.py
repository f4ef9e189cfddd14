"""FusedTorsoTrainNet(table_grad=...) and lz_torso_train_backward_rows (csrc/lz_torso_train.hip) without a device: the constructor's
argument, the new entry point declared, exported and bound, its argument errors (all rejected before any launch), and the register report
of the rows-emitting backward instantiations."""
import ctypes as C
import json
import os

import pytest

FAKE = 0x10000   # never dereferenced: every call below is rejected (or a no-op) on the host
BAD = -2         # LZ_ERR_BAD_ARGUMENT
SYMBOL = "lz_torso_train_backward_rows"


def test_wrong_mode_is_a_value_error_before_any_library_is_loaded(monkeypatch):
    from lzzx_nerf_amd import _lib, torso_train

    def no_load():
        raise AssertionError("the constructor loaded the library")

    monkeypatch.setattr(_lib, "load", no_load)
    for bad in ("Fixed", "sorted", None, 0):
        with pytest.raises(ValueError):
            torso_train.FusedTorsoTrainNet(ind_dim_torso=8, table_grad=bad)
    for ok in ("atomic", "ordered", "fixed"):
        assert torso_train.FusedTorsoTrainNet(ind_dim_torso=0, table_grad=ok).table_grad == ok


def test_default_is_atomic_whatever_the_global_mode():
    from lzzx_nerf_amd import gridencoder
    from lzzx_nerf_amd.torso_train import FusedTorsoTrainNet
    assert FusedTorsoTrainNet().table_grad == "atomic"
    prev = gridencoder.set_table_grad("fixed")
    try:
        net = FusedTorsoTrainNet()
        assert net.table_grad == "atomic"
    finally:
        gridencoder.set_table_grad(prev)
    assert net.keep_denc is False and net.last_denc is None and net.last_u is None
    net.table_grad = "ordered"   # a plain attribute
    assert net.table_grad == "ordered" and "table_grad" not in net.state_dict()


def test_new_symbol_declared_exported_bound():
    from test_cabi import _declared
    from lzzx_nerf_amd import _lib
    assert SYMBOL in _declared() and SYMBOL in _lib.SIGNATURES and SYMBOL in _lib.ALL_SYMBOLS
    assert len(_lib.SIGNATURES[SYMBOL]) == len(_lib.SIGNATURES["lz_torso_train_backward"]) + 2   # denc, u before the stream
    assert hasattr(C.CDLL(_lib.SO_PATH), SYMBOL)
    assert _lib.load().lz_abi_version() == _lib.ABI_VERSION == 11


def _params(ind_dim=8, n_offsets=17, null=None):
    from lzzx_nerf_amd import _lib
    p = _lib.TorsoTrainParams()
    n = p.net
    for f in ("deform_w0", "deform_w1", "deform_w2", "torso_w0", "torso_w1", "torso_w2", "emb", "offsets", "enc_anchor", "ind_code"):
        setattr(n, f, None if f == null else FAKE)
    n.ind_dim, n.gridtype, n.torso_shrink, n.S, n.H = ind_dim, 1, 0.8, 0.5, 16
    p.n_offsets = n_offsets
    return p


def _grads(null=None):
    from lzzx_nerf_amd import _lib
    g = _lib.TorsoGrads()
    for f, _ in _lib.TorsoGrads._fields_:
        setattr(g, f, None if f == null else FAKE)
    return g


@pytest.mark.parametrize("case", ["null_params", "null_grads", "null_ws", "null_xy", "null_denc", "null_u", "ind_dim", "offsets", "null_g_w",
                                  "null_g_ind", "null_table"])
def test_rows_entry_argument_errors(case):
    """lz_torso_train_backward's checks, plus denc and u; every case comes back before a launch"""
    from lzzx_nerf_amd import _lib
    p, g, a = _params(), _grads(), dict(xy=FAKE, ws=FAKE, denc=FAKE, u=FAKE)
    if case == "null_params":
        p = None
    elif case == "null_grads":
        g = None
    elif case == "ind_dim":
        p = _params(ind_dim=16)
    elif case == "offsets":
        p = _params(n_offsets=33)
    elif case == "null_g_w":
        g = _grads(null="g_torso_w1")
    elif case == "null_g_ind":
        g = _grads(null="g_ind_code")
    elif case == "null_table":
        p = _params(null="emb")
    else:
        a[case[5:]] = None
    lib = _lib.load()
    rc = lib.lz_torso_train_backward_rows(C.byref(p) if p is not None else None, a["xy"], 64, None, FAKE, None,
                                          C.byref(g) if g is not None else None, a["ws"], a["denc"], a["u"], None)
    msg = lib.lz_last_error().decode()
    assert rc == BAD, (case, rc, msg)
    assert "torso_train_backward_rows" in msg and "launch" not in msg.lower() and "hip error" not in msg.lower(), msg


def test_rows_entry_zero_pixels_is_a_no_op():
    from lzzx_nerf_amd import _lib
    assert _lib.load().lz_torso_train_backward_rows(None, None, 0, None, None, None, None, None, None, None, None) == 0


def test_rows_backward_instantiations_neither_spill_nor_use_scratch():
    """the way tests/test_grid_kernel_resources.py reads build.py's report.  lz_k_torso_train_backward<IND, ROWS>: the two ROWS = true
    instantiations are new; like the scattering ones they run one workgroup per compute unit on the whole register file"""
    from lzzx_nerf_amd import build as B
    if not os.path.exists(B.RESOURCES) or not B.up_to_date():
        B.build(force=True)
    res = json.load(open(B.RESOURCES))["lz_torso_train.hip"]
    for ind in (0, 8):
        rows = [k for k in res if k.startswith("_Z25lz_k_torso_train_backwardILi%dELb1EE" % ind)]
        scatter = [k for k in res if k.startswith("_Z25lz_k_torso_train_backwardILi%dELb0EE" % ind)]
        assert len(rows) == 1 and len(scatter) == 1, (rows, scatter)
        r, s = res[rows[0]], res[scatter[0]]
        assert r.get("vgpr_spill", 0) == 0 and r.get("sgpr_spill", 0) == 0 and r.get("scratch", 0) == 0, r
        assert r["vgprs"] <= 256 and r["occupancy"] >= 1 and r["lds"] == s["lds"], (r, s)
