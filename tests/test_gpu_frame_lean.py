"""The f32 slice's dense-level table loads as 8-byte buffer loads (lz_head_gather.h: PAIR0) change no bit: the stand-alone f32 head and the
fused frame against oracle.head / oracle.render and the mode="loop" renderer -- on the box's faces, edges and corners (coordinates exactly
+-bound, where the x + 1 corner is the entry behind a row's last cell), in the last column of levels 0..3, with and without the eye input
and ind_code, with level 0 hashed (the one-load-per-corner branch), on partial 16-ray tiles, and through a head whose ReLU inputs are
exactly 0, all negative or all positive."""
import itertools

import numpy as np
import pytest
import torch

from conftest import ellipsoid_bitfield
from oracle import oracle as O
from oracle.head import TriplaneSpec, head_forward
from test_gpu_frame_sh_partial import KEYS, _checker, _render, _setup, dev

pytestmark = pytest.mark.gpu
NAMES = ("sigma", "rgb", "amb_aud", "amb_eye", "unc")
RELU_LAYERS = ("aud_ch_att_net.net.0.weight", "eye_att_net.net.0.weight", "sigma_net.net.0.weight", "sigma_net.net.1.weight",
               "color_net.net.0.weight")


def _points(bound=1.0, n=100):
    """corners, edges, faces, last-column points and interior points, dealt round-robin so that the first 16 hold some of each (the first
    sample is a corner); the last cell of a row at levels 0..3 starts at x01 >= 62.5 / 63, so 1 - 2^-10 of the bound lies in it at all four"""
    rng = np.random.default_rng(77)
    rnd = lambda: rng.uniform(-0.97, 0.97)
    kinds = {0: [], 1: [], 2: []}                       # number of free coordinates -> points on corners / edges / faces
    for s in itertools.product((1.0, 0.0, -1.0), repeat=3):
        free = sum(c == 0.0 for c in s)
        if free < 3:
            kinds[free].append([c * bound if c else rnd() * bound for c in s])
    near = bound * (1.0 - 2.0 ** -10)
    last = [[near, rnd(), rnd()], [rnd(), near, rnd()], [rnd(), rnd(), near], [near, near, near], [near, -near, rnd()], [-near, rnd(), near]]
    cats = [kinds[0], kinds[1], kinds[2], last]
    out = []
    for i in range(max(map(len, cats))):
        out += [c[i] for c in cats if i < len(c)]
    while len(out) < n:
        out.append([rnd() * bound, rnd() * bound, rnd() * bound])
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.asarray(out[:n], np.float32), d.astype(np.float32)


def _hashed0(params):
    """the same network on 2^12-entry levels: 65^2 > 4096, so level 0 (and every other) is hashed and LZ_LVTAB_DENSE0 is 0"""
    spec = TriplaneSpec(1.0)
    spec.offsets = O.grid_offsets(2, 12, spec.per_level_scale, 64, 12)
    spec.n_params = int(spec.offsets[-1])
    assert int(spec.offsets[1] - spec.offsets[0]) == 4096
    p = dict(params)
    rng = np.random.default_rng(4321)
    for name in ("xy", "yz", "xz"):
        p["encoder_%s.offsets" % name] = np.asarray(spec.offsets, dtype=params["encoder_xy.offsets"].dtype)
        p["encoder_%s.embeddings" % name] = rng.uniform(-1, 1, (spec.n_params, 1)).astype(np.float32)
    return spec, p


def _signed_rows(params):
    """every layer in front of a ReLU: rows 0, 4, 8 .. zero, rows 1, 5 .. all negative, rows 2, 6 .. all positive, the rest as they are"""
    p = dict(params)
    for k in RELU_LAYERS:
        w = p[k].copy()
        w[0::4] = 0.0
        w[1::4] = -np.abs(w[1::4])
        w[2::4] = np.abs(w[2::4])
        p[k] = w
    return p


_cache = {}


def _case(params, golden, table, cond):
    """(spec, parameters, head, the checker's outputs on all 100 points), computed once per table layout and conditioning"""
    key = (table, cond)
    if key not in _cache:
        from lzzx_nerf_amd.head import FusedTriplaneHead
        spec, p = {"dense": lambda: (TriplaneSpec(1.0), params), "hashed0": lambda: _hashed0(params),
                   "signed": lambda: (TriplaneSpec(1.0), _signed_rows(params))}[table]()
        xyz, dirs = _points()
        # without the inputs the kernel skips their k-steps; the checker fed zeros adds exact zeros there (and a ReLU sits behind both)
        eye = golden["net_eye"] if cond else np.zeros_like(golden["net_eye"])
        ind = golden["net_ind"] if cond else np.zeros_like(golden["net_ind"])
        want = head_forward(spec, p, xyz, dirs, golden["net_enc_a"], ind, eye, testing=True)
        head = FusedTriplaneHead({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in p.items()}, bound=1.0)
        _cache[key] = (head, xyz, dirs, want)
    return _cache[key]


def _check_head(params, golden, table, cond, n, names=NAMES):
    head, xyz, dirs, want = _case(params, golden, table, cond)
    got = head.forward(dev(xyz[:n]), dev(dirs[:n]), dev(golden["net_enc_a"]), dev(golden["net_ind"]) if cond else None,
                       dev(golden["net_eye"]) if cond else None, testing=True)
    for name, g, w in zip(NAMES, got, want):
        if name not in names:
            continue
        if name == "amb_eye" and not cond:
            assert float(g.abs().max()) == 0.0          # no eye input: the head leaves the eye attention at 0
            continue
        assert np.array_equal(g.cpu().numpy(), w[:n]), (name, n)


@pytest.mark.parametrize("cond", [True, False], ids=["eye_ind", "no_eye_no_ind"])
@pytest.mark.parametrize("n", [1, 16, 17, 100])
def test_head_dense_levels_paired_branch(params, golden, n, cond):
    assert list(np.diff(params["encoder_xy.offsets"])[:4]) == [4232, 6248, 9032, 13000]      # levels 0..3 dense
    _check_head(params, golden, "dense", cond, n)


@pytest.mark.parametrize("cond", [True, False], ids=["eye_ind", "no_eye_no_ind"])
@pytest.mark.parametrize("n", [1, 16, 17, 100])
def test_head_level_0_hashed_branch(params, golden, n, cond):
    _check_head(params, golden, "hashed0", cond, n)


def test_head_relu_inputs_zero_negative_positive(params, golden):
    _check_head(params, golden, "signed", True, 100, names=("sigma", "rgb"))


def _frame_refs(params, golden, H, W, scene, fold):
    key = ("frame", H, W, scene, fold)
    if key not in _cache:
        head, ro, rd = _setup(params, golden, H, W, fold_geo=fold)
        bits = np.full(128 ** 3 // 8, 255, np.uint8) if scene == "ones" else ellipsoid_bitfield()[0]
        cond = (dev(golden["net_enc_a"]), dev(golden["net_ind"]), dev(golden["net_eye"]))
        loop = _render(head, bits, ro, rd, cond, "loop", max_steps=24)
        ck = ("checker", H, W, scene)
        if ck not in _cache:
            _cache[ck] = _checker(params, golden, ro, rd, bits, golden["net_eye"], (1, 8), max_steps=24)
        _cache[key] = (head, ro, rd, bits, cond, loop) + _cache[ck]
    return _cache[key]


@pytest.mark.parametrize("fold", [False, True], ids=["plain", "fold_geo"])
@pytest.mark.parametrize("S", [1, 4])
@pytest.mark.parametrize("scene", ["ones", "ellipsoid"])
@pytest.mark.parametrize("H,W", [(24, 24), (17, 9)])
def test_fused_frame_equals_loop_and_checker(params, golden, H, W, scene, S, fold):
    """576 rays and 153 rays (a partial last 16-ray tile).  fold_geo reassociates the colour net (head.py), so against the checker it is
    held on what the colours do not enter: sigma is the same bits, hence depth, the weight / attention sums and the sample counts"""
    head, ro, rd, bits, cond, loop, ref, st = _frame_refs(params, golden, H, W, scene, fold)
    fused = _render(head, bits, ro, rd, cond, "fused", steps_per_pass=S, max_steps=24)
    for k in KEYS:
        assert torch.equal(fused[k], loop[k]), k
    for k in ("depth", "weights_sum", "amb_aud_sum", "amb_eye_sum", "uncertainty_sum") + (() if fold else ("image",)):
        assert np.array_equal(fused[k].cpu().numpy(), ref[k]), k
    assert np.array_equal(fused["ray_counts"].cpu().numpy().astype(np.int64), st["samples_per_ray"])
    assert int(fused["ray_counts"].sum()) > 0
