"""Audio encoder training (lzzx_nerf_amd.audio_train, csrc/lz_audio_train.hip) without a device: the new entries are declared, exported and
bound under ABI 11; argument errors come back before any launch (a call that got as far as a launch would report a HIP error on this box);
the kernels neither spill nor use scratch; the module has the reference's state-dict keys and shapes and optimizer groups, and building it
touches no device."""
import ctypes as C
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "reference_audio_train.npz")
NEW = ("lz_audio_train_backward", "lz_audio_train_workspace")
FAKE = 0x10000   # never dereferenced: every case below is rejected on the host
BAD, UNSUPPORTED = -2, -1   # LZ_ERR_BAD_ARGUMENT, LZ_ERR_UNSUPPORTED


def test_new_symbols_declared_exported_bound():
    from test_cabi import _declared
    from lzzx_nerf_amd import _lib
    names = _declared()
    lib = C.CDLL(_lib.SO_PATH)
    for n in NEW:
        assert n in names and hasattr(lib, n) and n in _lib.ALL_SYMBOLS, n
    bound = _lib.load()
    assert bound.lz_abi_version() == _lib.ABI_VERSION == 11
    assert bound.lz_audio_train_workspace() >= 8 * 32 * 8 * 4


def _params(dim_in=29, dim_aud=32, n_win=8, att=1, null=None):
    from lzzx_nerf_amd import _lib
    p = _lib.AudioParams()
    for f, n in (("c_w", 4), ("c_b", 4), ("fc_w", 2), ("fc_b", 2), ("ac_w", 5), ("ac_b", 5)):
        arr = getattr(p, f)
        for i in range(n):
            arr[i] = None if null == (f, i) else FAKE
    p.al_w, p.al_b = (None if null == ("al_w", 0) else FAKE), (None if null == ("al_b", 0) else FAKE)
    p.dim_in, p.dim_aud, p.n_win, p.use_att = dim_in, dim_aud, n_win, att
    return p


def _grads(null=None):
    from lzzx_nerf_amd import _lib
    g = _lib.AudioGrads()
    for f, n in (("g_c_w", 4), ("g_c_b", 4), ("g_fc_w", 2), ("g_fc_b", 2), ("g_ac_w", 5), ("g_ac_b", 5)):
        arr = getattr(g, f)
        for i in range(n):
            arr[i] = None if null == (f, i) else FAKE
    g.g_al_w, g.g_al_b = (None if null == ("g_al_w", 0) else FAKE), (None if null == ("g_al_b", 0) else FAKE)
    return g


def _bwd(p, g, a=FAKE, conv1=None, d_enc=FAKE, ws=FAKE):
    from lzzx_nerf_amd import _lib
    lib = _lib.load()
    rc = lib.lz_audio_train_backward(C.byref(p) if p is not None else None, a, conv1, d_enc, C.byref(g) if g is not None else None, ws, None)
    return rc, lib.lz_last_error().decode()


CASES = {
    "null_params": (lambda: (None, _grads(), {}), BAD),
    "null_grads": (lambda: (_params(), None, {}), BAD),
    "null_a": (lambda: (_params(), _grads(), {"a": None}), BAD),
    "null_d_enc_a": (lambda: (_params(), _grads(), {"d_enc": None}), BAD),
    "null_workspace": (lambda: (_params(), _grads(), {"ws": None}), BAD),
    "missing_conv_weight": (lambda: (_params(null=("c_w", 2)), _grads(), {}), BAD),
    "missing_fc_bias": (lambda: (_params(null=("fc_b", 1)), _grads(), {}), BAD),
    "missing_att_conv_weight": (lambda: (_params(null=("ac_w", 4)), _grads(), {}), BAD),
    "missing_att_linear": (lambda: (_params(null=("al_w", 0)), _grads(), {}), BAD),
    "missing_conv_grad": (lambda: (_params(), _grads(null=("g_c_w", 0)), {}), BAD),
    "missing_fc_grad": (lambda: (_params(), _grads(null=("g_fc_w", 1)), {}), BAD),
    "missing_att_conv_grad": (lambda: (_params(), _grads(null=("g_ac_b", 3)), {}), BAD),
    "missing_att_linear_grad": (lambda: (_params(), _grads(null=("g_al_b", 0)), {}), BAD),
    "n_win_0": (lambda: (_params(n_win=0, att=0), _grads(), {}), UNSUPPORTED),
    "n_win_9": (lambda: (_params(n_win=9, att=0), _grads(), {}), UNSUPPORTED),
    "dim_aud_65": (lambda: (_params(dim_aud=65), _grads(), {}), UNSUPPORTED),
    "att_with_4_windows": (lambda: (_params(n_win=4), _grads(), {}), UNSUPPORTED),
    "wide_without_conv1_out": (lambda: (_params(dim_in=1024), _grads(), {}), BAD),
    "wide_without_workspace": (lambda: (_params(dim_in=1024), _grads(), {"conv1": FAKE, "ws": None}), BAD),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_backward_argument_errors_before_any_launch(case):
    make, want = CASES[case]
    p, g, kw = make()
    rc, msg = _bwd(p, g, **kw)
    assert rc == want, (case, rc, msg)
    assert "launch" not in msg.lower() and "hip error" not in msg.lower(), msg


def test_new_kernels_neither_spill_nor_use_scratch():
    from lzzx_nerf_amd import build as B
    if not os.path.exists(B.RESOURCES) or not B.up_to_date():
        B.build(force=True)
    res = json.load(open(B.RESOURCES))
    kernels = res["lz_audio_train.hip"]
    for stem in ("lz_k_audio_train_chain", "lz_k_audio_train_conv1_grad"):
        assert any(stem in k for k in kernels), stem
    for k, r in kernels.items():
        assert r.get("vgpr_spill", 0) == 0 and r.get("sgpr_spill", 0) == 0 and r.get("scratch", 0) == 0, (k, r)
        assert r["lds"] <= 64 * 1024, (k, r)
    # the inference kernels keep their shape after their helpers moved into lz_audio_net.h
    inf = res["lz_audio.hip"]
    for stem in ("lz_k_audio_encode", "lz_k_audio_conv1_wide"):
        rs = [r for k, r in inf.items() if stem in k]
        assert len(rs) == 1 and rs[0]["vgpr_spill"] == 0 and rs[0].get("sgpr_spill", 0) == 0 and rs[0].get("scratch", 0) == 0, (stem, rs)


@pytest.mark.parametrize("att", [True, False])
def test_state_dict_keys_and_shapes_are_the_references(att):
    """the keys (in order) and shapes of the reference's audio_net / audio_att_net parameters, as recorded in the fixture"""
    from lzzx_nerf_amd.audio_train import FusedAudioTrainNet
    z = np.load(GOLDEN)
    for dim_in in (29, 44):
        tag = "%d_%s" % (dim_in, "att" if att else "noatt")
        net = FusedAudioTrainNet(dim_in=dim_in, dim_aud=32, att=att)
        sd = net.state_dict()
        assert list(sd) == list(z[tag + "/keys"])
        for k, v in sd.items():
            assert tuple(v.shape) == z[tag + "/f64/grad/" + k].shape, k
            assert v.dtype.is_floating_point and v.device.type == "cpu"   # constructing the module touches no device


def test_state_dict_moves_to_the_inference_encoder_layout():
    """FusedAudioEncoder reads exactly these keys (it needs no device to be checked here: its constructor copies to the device it is given)"""
    from lzzx_nerf_amd.audio_train import FusedAudioTrainNet
    from test_audio_oracle import audio_state
    for att in (True, False):
        net = FusedAudioTrainNet(dim_in=1024, dim_aud=32, att=att)
        ref = audio_state(1024, 32, att)
        assert set(net.state_dict()) == set(ref)
        assert all(tuple(net.state_dict()[k].shape) == ref[k].shape for k in ref)


def test_param_groups_are_get_params():
    """network.py:333 (audio_net: lr_net, wd) and 344 (audio_att_net: 5 lr_net, 1e-4)"""
    from lzzx_nerf_amd.audio_train import FusedAudioTrainNet
    net = FusedAudioTrainNet(dim_in=29, att=True)
    g = net.param_groups(1e-3, wd=5e-4)
    assert [(x["lr"], x["weight_decay"]) for x in g] == [(1e-3, 5e-4), (5e-3, 1e-4)]
    assert [len(x["params"]) for x in g] == [12, 12]
    ids = [id(p) for x in g for p in x["params"]]
    assert sorted(ids) == sorted(id(p) for p in net.parameters())
    assert all(p is q for p, q in zip(g[0]["params"], net.audio_net.parameters()))
    g = FusedAudioTrainNet(dim_in=29, att=False).param_groups(2e-3)
    assert len(g) == 1 and g[0]["lr"] == 2e-3 and g[0]["weight_decay"] == 0


def test_unsupported_configurations_raise():
    from lzzx_nerf_amd.audio_train import FusedAudioTrainNet
    with pytest.raises(NotImplementedError, match="emb"):
        FusedAudioTrainNet(dim_in=29, emb=True)
    with pytest.raises(ValueError):
        FusedAudioTrainNet(dim_in=29, dim_aud=65)
    import torch
    with pytest.raises(RuntimeError, match="GPU"):
        FusedAudioTrainNet(dim_in=29)(torch.zeros(8, 29, 16))
