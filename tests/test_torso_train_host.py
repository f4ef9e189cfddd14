"""Torso training entry points (csrc/lz_torso_train.hip) without a device: declared, exported and bound; argument errors come back before
any launch (a call that got as far as a launch would report a HIP error on this box); N = 0 is a no-op; no spills, no scratch."""
import ctypes as C
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("lz_torso_train_forward", "lz_torso_train_backward", "lz_torso_anchor_encode_backward", "lz_torso_train_workspace")
FAKE = 0x10000   # never dereferenced: every case below is rejected (or a no-op) on the host


def test_new_symbols_declared_exported_bound():
    from test_cabi import _declared
    from lzzx_nerf_amd import _lib
    names = _declared()
    lib = C.CDLL(_lib.SO_PATH)
    for n in NEW:
        assert n in names and hasattr(lib, n) and n in _lib.ALL_SYMBOLS, n
    bound = _lib.load()
    assert bound.lz_abi_version() == _lib.ABI_VERSION == 11
    assert bound.lz_torso_train_workspace() >= 256 * 28 * 256 * 4


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


def _fwd(p, N=64, xy=FAKE, alpha=FAKE, color=FAKE):
    from lzzx_nerf_amd import _lib
    lib = _lib.load()
    return lib.lz_torso_train_forward(C.byref(p) if p is not None else None, xy, N, alpha, color, None, None)


def _bwd(p, g, N=64, xy=FAKE, ws=FAKE):
    from lzzx_nerf_amd import _lib
    lib = _lib.load()
    return lib.lz_torso_train_backward(C.byref(p) if p is not None else None, xy, N, None, FAKE, None, C.byref(g) if g is not None else None, ws, None)


BAD = -2   # LZ_ERR_BAD_ARGUMENT


@pytest.mark.parametrize("case", ["null_params", "null_xy", "null_out", "ind_dim", "offsets", "null_weight", "null_ind"])
def test_forward_argument_errors(case):
    if case == "null_params":
        rc = _fwd(None)
    elif case == "null_xy":
        rc = _fwd(_params(), xy=None)
    elif case == "null_out":
        rc = _fwd(_params(), color=None)
    elif case == "ind_dim":
        rc = _fwd(_params(ind_dim=4))
    elif case == "offsets":
        rc = _fwd(_params(n_offsets=16))
    elif case == "null_weight":
        rc = _fwd(_params(null="torso_w1"))
    else:
        rc = _fwd(_params(null="ind_code"))
    from lzzx_nerf_amd import _lib
    msg = _lib.load().lz_last_error().decode()
    assert rc == BAD, (case, rc, msg)
    assert "launch" not in msg.lower() and "hip error" not in msg.lower(), msg


@pytest.mark.parametrize("case", ["null_params", "null_grads", "null_ws", "null_xy", "ind_dim", "offsets", "null_g_emb", "null_g_ind", "null_table"])
def test_backward_argument_errors(case):
    p, g, kw = _params(), _grads(), {}
    if case == "null_params":
        p = None
    elif case == "null_grads":
        g = None
    elif case == "null_ws":
        kw["ws"] = None
    elif case == "null_xy":
        kw["xy"] = None
    elif case == "ind_dim":
        p = _params(ind_dim=16)
    elif case == "offsets":
        p = _params(n_offsets=33)
    elif case == "null_g_emb":
        g = _grads(null="g_emb")
    elif case == "null_g_ind":
        g = _grads(null="g_ind_code")
    else:
        p = _params(null="emb")
    rc = _bwd(p, g, **kw)
    from lzzx_nerf_amd import _lib
    msg = _lib.load().lz_last_error().decode()
    assert rc == BAD, (case, rc, msg)
    assert "launch" not in msg.lower() and "hip error" not in msg.lower(), msg


def test_anchor_backward_argument_errors():
    from lzzx_nerf_amd import _lib
    lib = _lib.load()
    assert lib.lz_torso_anchor_encode_backward(FAKE, FAKE, FAKE, 4, FAKE, None) == BAD        # the torso has three anchors
    assert lib.lz_torso_anchor_encode_backward(FAKE, None, FAKE, 3, FAKE, None) == BAD
    assert lib.lz_torso_anchor_encode_backward(FAKE, FAKE, FAKE, 3, None, None) == BAD
    assert lib.lz_torso_anchor_encode_backward(None, None, None, 0, None, None) == 0          # J = 0: nothing to do


def test_zero_pixels_is_a_no_op():
    """N = 0 returns LZ_OK before any pointer is looked at, even with no parameter block at all"""
    from lzzx_nerf_amd import _lib
    lib = _lib.load()
    assert lib.lz_torso_train_forward(None, None, 0, None, None, None, None) == 0
    assert lib.lz_torso_train_backward(None, None, 0, None, None, None, None, None, None) == 0


def test_new_kernels_neither_spill_nor_use_scratch():
    from lzzx_nerf_amd import build as B
    if not os.path.exists(B.RESOURCES) or not B.up_to_date():
        B.build(force=True)
    res = json.load(open(B.RESOURCES))
    kernels = res["lz_torso_train.hip"]
    names = set(kernels)
    for stem in ("lz_k_torso_train_forward", "lz_k_torso_train_backward", "lz_k_torso_train_combine", "lz_k_torso_anchor_encode_backward"):
        assert any(stem in k for k in names), stem
    for k, r in kernels.items():
        assert r.get("vgpr_spill", 0) == 0 and r.get("sgpr_spill", 0) == 0 and r.get("scratch", 0) == 0, (k, r)
    # the inference kernel keeps its shape after its chain moved into lz_torso_net.h
    inf = [r for k, r in res["lz_torso.hip"].items() if "lz_k_torso_forward" in k]
    assert len(inf) == 2 and all(r["vgpr_spill"] == 0 and r.get("scratch", 0) == 0 and r["occupancy"] >= 3 for r in inf), inf


def test_module_exposes_the_reference_state_dict_keys():
    """same keys as TorsoTrainNet (and the reference); constructing it touches no device"""
    from lzzx_nerf_amd.torso_train import FusedTorsoTrainNet, TorsoTrainNet
    a, b = FusedTorsoTrainNet(ind_dim_torso=8), TorsoTrainNet(ind_dim_torso=8)
    assert list(a.state_dict()) == list(b.state_dict())
    assert {k: tuple(v.shape) for k, v in a.state_dict().items()} == {k: tuple(v.shape) for k, v in b.state_dict().items()}
    with pytest.raises(ValueError):
        FusedTorsoTrainNet(ind_dim_torso=4)
