"""The host side of the perceptual loss (csrc/lz_lpips.hip, lzzx_nerf_amd/perceptual.py), without a GPU: the C ABI additions, argument
errors before any launch, the state-dict reader, the packed weight images unpacked again, the kernels' resource report, and the checker
(tests/lpips_checker.py) held to known answers."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch

import lpips_cases as LC
import lpips_checker as K
from lzzx_nerf_amd import _lib, perceptual
from lzzx_nerf_amd.synthetic import lpips_alex_state

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("lz_lpips_packed_floats", "lz_lpips_pack", "lz_lpips_workspace_bytes", "lz_lpips_forward", "lz_lpips_backward", "lz_objective_pred_backward")
CIN, CINP, COUT, KS = (3, 64, 192, 384, 256), (4, 64, 192, 384, 256), (64, 192, 384, 256, 256), (11, 5, 3, 3, 3)


def test_entries_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "lzzx_nerf_hip.h")).read()
    lib = _lib.load()
    for name in ENTRIES:
        assert re.search(r"^\s*(?:int|size_t)\s+%s\s*\(" % name, hdr, flags=re.M), name
        assert hasattr(C.CDLL(_lib.SO_PATH), name) and name in _lib.ALL_SYMBOLS, name
    for name in ENTRIES[:5]:       # each declaration's comment names what it replaces
        m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*(?:int|size_t)\s+%s\s*\(" % name, hdr, flags=re.S)
        assert m and "lpips.LPIPS(net='alex')" in m.group(1) and "TrainerUtil.py:283,309" in m.group(1), name
    assert lib.lz_abi_version() == _lib.ABI_VERSION == 11


def test_bad_arguments_come_back_before_any_launch():
    lib = _lib.load()
    p = lambda: C.c_void_p(0x10000)      # fake non-null, 16-byte aligned pointers: a call that reached a launch would report a HIP error

    def fwd(P, H, W, **null):
        a = dict(packed=p(), pred=p(), target=p(), ws=p(), value=p())
        a.update({k: None for k in null})
        return lib.lz_lpips_forward(a["packed"], a["pred"], a["target"], P, H, W, a["ws"], a["value"], None)

    assert fwd(0, 64, 64) == 0 and lib.lz_lpips_backward(None, None, 0, 0, 0, None, None, None) == 0       # no patches: nothing to do
    for H, W in ((30, 64), (64, 30), (257, 64), (64, 300), (0, 0)):
        assert fwd(1, H, W) == -1, (H, W)
        assert lib.lz_lpips_backward(p(), p(), 1, H, W, p(), p(), None) == -1, (H, W)
        assert lib.lz_lpips_workspace_bytes(1, H, W) == 0
        assert b"launch" not in lib.lz_last_error()
    assert fwd(1 << 20, 64, 64) == -1
    for k in ("packed", "pred", "target", "ws", "value"):
        assert fwd(1, 64, 64, **{k: True}) == -2, k
    assert lib.lz_lpips_forward(C.c_void_p(0x10004), p(), p(), 1, 64, 64, p(), p(), None) == -2             # misaligned
    assert lib.lz_lpips_backward(p(), p(), 1, 64, 64, C.c_void_p(0x10008), p(), None) == -2
    assert lib.lz_lpips_backward(p(), None, 1, 64, 64, p(), p(), None) == -2
    assert lib.lz_lpips_workspace_bytes(1, 64, 64) > 0 and lib.lz_lpips_workspace_bytes(0, 64, 64) == 0
    assert lib.lz_lpips_pack(None, p(), 1 << 30) == -2
    assert lib.lz_objective_pred_backward(None, None, None, None, 0, 1.0, 0, None, None, None) == 0
    assert lib.lz_objective_pred_backward(p(), p(), p(), None, 2, 1.0, 4, p(), p(), None) == -2            # bg_mode 2 without bg
    assert lib.lz_objective_pred_backward(p(), p(), p(), p(), 4, 1.0, 4, p(), p(), None) == -2
    with pytest.raises(_lib.LzError):                                                                      # too small a packed buffer
        w = _lib.LpipsWeights()
        _lib.call("lz_lpips_pack", C.byref(w), p(), 8)


def test_workspace_size():
    """the workspace holds the scaled input, five taps and two pooled maps of both images, and the gradients of one"""
    lib = _lib.load()
    for P, H, W in ((1, 31, 31), (2, 35, 47), (1, 256, 256)):
        h0, w0 = (H - 7) // 4 + 1, (W - 7) // 4 + 1
        h1, w1 = (h0 - 3) // 2 + 1, (w0 - 3) // 2 + 1
        h2, w2 = (h1 - 3) // 2 + 1, (w1 - 3) // 2 + 1
        feat = h0 * w0 * 64 + h1 * w1 * (64 + 192) + h2 * w2 * (192 + 384 + 256 + 256)
        assert lib.lz_lpips_workspace_bytes(P, H, W) == 4 * P * (2 * H * W * 4 + 3 * feat)


def test_state_dict_reader():
    sd = lpips_alex_state(3)
    conv_w, conv_b, lin_w, shift, scale = perceptual.read_state(sd)
    assert [w.shape for w in conv_w] == list(perceptual.CONV_SHAPES) and [l.shape for l in lin_w] == [(c,) for c in COUT]
    assert np.array_equal(conv_w[2], sd["net.slice3.6.weight"]) and np.array_equal(lin_w[1], sd["lin1.model.1.weight"].reshape(-1))
    assert all((l >= 0).all() for l in lin_w)
    # the lins.* duplicates alone, tensors instead of arrays, and the default scaling constants
    alt = {k.replace("lin", "lins.", 1) if k.startswith("lin") else k: torch.from_numpy(v) for k, v in sd.items() if not k.startswith("scaling_layer")}
    assert "lins.4.model.1.weight" in alt and "lin4.model.1.weight" not in alt
    _, _, lin2, shift2, scale2 = perceptual.read_state(alt)
    assert all(np.array_equal(a, b) for a, b in zip(lin_w, lin2))
    assert np.array_equal(shift2, np.array((-.030, -.088, -.188), np.float32)) and np.array_equal(scale2, np.array((.458, .448, .450), np.float32))
    assert np.array_equal(shift, shift2) and np.array_equal(scale, scale2)
    for key in ("net.slice1.0.weight", "net.slice5.10.bias", "lin3.model.1.weight"):
        bad = dict(sd)
        del bad[key]
        with pytest.raises(ValueError, match=re.escape(key)):
            perceptual.read_state(bad)
    bad = dict(sd)
    bad["net.slice2.3.weight"] = np.zeros((192, 64, 3, 3), np.float32)
    with pytest.raises(ValueError, match=r"net\.slice2\.3\.weight.*\(192, 64, 3, 3\)"):
        perceptual.read_state(bad)
    bad = dict(sd)
    bad["lin0.model.1.weight"] = -sd["lin0.model.1.weight"]
    with pytest.raises(ValueError, match="negative"):
        perceptual.read_state(bad)


def _unpack(img, n_out, taps, C):
    """a pack [n_out/16][ceil(taps C / 16)][64][4] -> dense [n_out, KB * 16] by k, the layout stated in include/lzzx_nerf_hip.h"""
    KB = (taps * C + 15) // 16
    a = img.reshape(n_out // 16, KB, 4, 16, 4)          # t, jj, lane >> 4, lane & 15, c
    return a.transpose(0, 3, 1, 2, 4).reshape(n_out, KB * 16)     # n = 16 t + (lane & 15), k = 16 jj + 4 (lane >> 4) + c


def test_packed_images_hold_every_weight_exactly_once():
    sd = lpips_alex_state(1)
    for i, k in enumerate(perceptual.CONV_KEYS):        # distinct integers as weights: a weight is found by its value
        n = sd[k + ".weight"].size
        sd[k + ".weight"] = (1 + np.arange(n, dtype=np.float32)).reshape(sd[k + ".weight"].shape)
        assert n < 1 << 24
    packed = perceptual.pack_weights(sd).numpy()
    assert packed.size == _lib.load().lz_lpips_packed_floats()
    o = 8
    assert np.array_equal(packed[:8], np.array([-.030, -.088, -.188, 0, .458, .448, .450, 0], np.float32))
    for l, key in enumerate(perceptual.CONV_KEYS):      # forward packs: n = co, k = (ky KS + kx) Cin' + ci
        W, taps = sd[key + ".weight"], KS[l] * KS[l]
        size = (COUT[l] // 16) * ((taps * CINP[l] + 15) // 16) * 256
        d = _unpack(packed[o:o + size], COUT[l], taps, CINP[l])
        want = np.zeros((COUT[l], d.shape[1]), np.float32)
        want[:, :taps * CINP[l]].reshape(COUT[l], taps, CINP[l])[:, :, :CIN[l]] = W.reshape(COUT[l], CIN[l], taps).transpose(0, 2, 1)
        assert np.array_equal(d, want), key
        assert np.array_equal(np.sort(d[d != 0]), 1 + np.arange(W.size, dtype=np.float32)), key      # every weight once, zeros elsewhere
        o += size
        assert np.array_equal(packed[o:o + COUT[l]], sd[key + ".bias"])
        o += COUT[l]
    for l in range(1, 5):                               # transposed packs: n = ci, k = (flipped tap) Cout + co
        W, taps = sd[perceptual.CONV_KEYS[l] + ".weight"], KS[l] * KS[l]
        size = (CIN[l] // 16) * (taps * COUT[l] // 16) * 256
        d = _unpack(packed[o:o + size], CIN[l], taps, COUT[l]).reshape(CIN[l], taps, COUT[l])
        want = W.reshape(COUT[l], CIN[l], taps)[:, :, ::-1].transpose(1, 2, 0)
        assert np.array_equal(d, want), l
        assert np.array_equal(np.sort(d.reshape(-1)), 1 + np.arange(W.size, dtype=np.float32)), l
        o += size
    g = packed[o:o + 121 * 64 * 4].reshape(121, 64, 4)   # conv1's gather pack
    W = sd[perceptual.CONV_KEYS[0] + ".weight"].reshape(64, 3, 121)
    assert np.array_equal(g[:, :, :3], W.transpose(2, 0, 1)) and (g[:, :, 3] == 0).all()
    o += 121 * 64 * 4
    for l in range(5):
        assert np.array_equal(packed[o:o + COUT[l]], sd[f"lin{l}.model.1.weight"].reshape(-1))
        o += COUT[l]
    assert o == packed.size


def test_new_kernels_use_no_scratch_and_spill_nothing():
    from lzzx_nerf_amd import build as B
    if not os.path.exists(B.RESOURCES) or not B.up_to_date():
        B.build(force=True)
    res = json.load(open(B.RESOURCES))
    assert "lz_lpips.hip" in res
    ker = res["lz_lpips.hip"]
    for stem in ("lz_k_lpips_prep", "lz_k_lpips_conv", "lz_k_lpips_pool", "lz_k_lpips_pool_backward", "lz_k_lpips_conv1_dgrad", "lz_k_lpips_taps_forward",
                 "lz_k_lpips_taps_backward"):
        assert any(stem in k for k in ker), stem
    assert sum("lz_k_lpips_convI" in k for k in ker) == 6          # five forward shapes (conv5's serves two data gradients) and conv2's data gradient
    pred = [r for k, r in res["lz_objective.hip"].items() if "lz_k_obj_pred_backward" in k]
    assert len(pred) == 1
    for k, r in list(ker.items()) + [("pred_backward", pred[0])]:
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, (k, r)


def test_checker_known_answers():
    pred, target = LC.images("min31")
    v, g = K.value_and_grad(LC.state(), pred, pred.copy(), torch.float64)
    assert (v == 0).all() and (g == 0).all()
    v, _ = LC.reference("min31")
    plain = K.plain_value(LC.state(), pred[0], target[0])
    assert v.shape == (1,) and v[0] > 1e-3
    assert abs(v[0] - plain) <= 1e-12 * plain, (v[0], plain)
    with pytest.raises(RuntimeError):                                # below the minimum size torch has no pool output
        K.value_and_grad(LC.state(), np.zeros((1, 3, 30, 31), np.float32), np.zeros((1, 3, 30, 31), np.float32), torch.float64)


def test_recorded_bars_are_the_measured_ones():
    """MEASURED in tests/lpips_cases.py is what `--measure` gives, to the printed digits (the f32 evaluation is torch's: allow the last
    digits to move between builds, never the magnitude)"""
    for name in LC.CASES:
        dv, dg = LC.deviations(*LC.reference(name, "float32"), name)
        assert dv <= 2 * LC.MEASURED["value_rel"] and dg <= 2 * LC.MEASURED["grad_rel"], (name, dv, dg)
    assert LC.BARS == {k: 8 * v for k, v in LC.MEASURED.items()}
    assert 1e-8 < LC.MEASURED["value_rel"] < 1e-6 and 1e-7 < LC.MEASURED["grad_rel"] < 1e-5
