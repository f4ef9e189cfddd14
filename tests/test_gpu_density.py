"""NeRFNetwork.density on the fused head (csrc/lz_density.hip; head.py: density, occupancy.py: density_only, ambient_grids,
density_field): the cut slice carries the forward's bits, geo_feat the checker's (f32) / the reference's autocast density() (f16), and the
lattice entries equal their restatement from parts that existed before them."""
import math
import os

import numpy as np
import pytest
import torch

from oracle.head import TriplaneSpec, density as oracle_density, encode_x
from oracle.occupancy import update_density_grid as oracle_update

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
_HEADS = {}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _params_for_bound(params, bound, rng):   # tests/test_gpu_occupancy.py
    if bound == 1.0:
        return params
    spec = TriplaneSpec(bound)
    p = dict(params)
    for n in ("xy", "yz", "xz"):
        p[f"encoder_{n}.embeddings"] = rng.uniform(-1, 1, (spec.n_params, 1)).astype(np.float32)
        p[f"encoder_{n}.offsets"] = spec.offsets.astype(np.int32)
    return p


def _head(params, bound=1.0, use_eye=True, precision="f32"):
    """(head, its numpy parameters), one per arrangement for the whole module"""
    from lzzx_nerf_amd.head import FusedTriplaneHead
    key = (bound, use_eye, precision)
    if key not in _HEADS:
        p = _params_for_bound(params, bound, np.random.default_rng(int(bound * 10)))
        if not use_eye:
            p = dict(p)
            p["sigma_net.net.0.weight"] = np.ascontiguousarray(p["sigma_net.net.0.weight"][:, :68])
        _HEADS[key] = (FusedTriplaneHead({k: torch.from_numpy(v) for k, v in p.items()}, bound=bound, exp_eye=use_eye, precision=precision), p)
    return _HEADS[key]


def _points(M, bound, seed):
    """uniform in the box, the eight corners +-bound first (as many as fit)"""
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(-bound, bound, (M, 3)).astype(np.float32)
    corners = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], np.float32) * np.float32(bound)
    xyz[:min(M, 8)] = corners[:min(M, 8)]
    return xyz


@pytest.mark.parametrize("precision", ["f32", "f16"])
@pytest.mark.parametrize("use_eye", [True, False])
@pytest.mark.parametrize("bound", [1.0, 2.0])
@pytest.mark.parametrize("M", [1, 15, 16, 17, 31, 32, 33, 1029])
def test_density_has_the_forwards_bits(params, golden, M, bound, use_eye, precision):
    head, _ = _head(params, bound, use_eye, precision)
    xyz = dev(_points(M, bound, M))
    dirs = torch.zeros(M, 3, device="cuda")
    dirs[:, 2] = 1.0
    enc_a, eye = dev(golden["net_enc_a"]), dev(golden["net_eye"]) if use_eye else None
    sig, _, aud, ae, _ = head.forward(xyz, dirs, enc_a, None, eye)
    pad = 40   # rows behind M: must stay NaN
    nan = lambda *shape: torch.full(shape, float("nan"), device="cuda")
    out = dict(sigma=nan(M + pad), ambient_aud=nan(M + pad, 1), ambient_eye=nan(M + pad, 1))
    if not use_eye:
        del out["ambient_eye"]
    d = head.density(xyz, enc_a, eye, out=out)
    assert set(d) == {"sigma", "ambient_aud", "ambient_eye"}
    assert d["sigma"] is out["sigma"] and d["ambient_aud"] is out["ambient_aud"]
    assert torch.equal(d["sigma"][:M], sig) and torch.equal(d["ambient_aud"][:M], aud)
    assert bool(torch.isnan(d["sigma"][M:]).all()) and bool(torch.isnan(d["ambient_aud"][M:]).all())
    assert not bool(torch.isnan(sig).any()) and bool((aud > 0).all())
    if use_eye:
        assert torch.equal(d["ambient_eye"][:M], ae) and bool(torch.isnan(d["ambient_eye"][M:]).all())
    else:
        assert d["ambient_eye"] is None
    # fresh outputs: shapes of the reference's dict (network.py:306-311)
    f = head.density(xyz, enc_a, eye)
    assert f["sigma"].shape == (M,) and f["ambient_aud"].shape == (M, 1) and "geo_feat" not in f
    assert torch.equal(f["sigma"], sig) and torch.equal(f["ambient_aud"], aud)
    # with geo_feat the other outputs keep their bits
    g = head.density(xyz, enc_a, eye, geo_feat=True, out=dict(geo_feat=torch.full((M + pad, 64), float("nan"), device="cuda",
                                                                                 dtype=torch.float16 if precision == "f16" else torch.float32)))
    assert torch.equal(g["sigma"], sig) and torch.equal(g["ambient_aud"], aud)
    assert not bool(torch.isnan(g["geo_feat"][:M]).any()) and bool(torch.isnan(g["geo_feat"][M:]).all())


@pytest.mark.parametrize("precision", ["f32", "f16"])
@pytest.mark.parametrize("count", [0, 17, 40])
def test_device_count_bounds_the_rows(params, golden, count, precision):
    """`count` as lz_triplane_head_forward reads it: min(M, *count) rows are evaluated and stored, the rest is left alone"""
    head, _ = _head(params, 1.0, True, precision)
    M = 33
    xyz, enc_a, eye = dev(_points(M, 1.0, 9)), dev(golden["net_enc_a"]), dev(golden["net_eye"])
    full = head.density(xyz, enc_a, eye, geo_feat=True)
    cnt = torch.tensor([count], dtype=torch.int32, device="cuda")
    out = {k: torch.full_like(v, float("nan")) for k, v in full.items()}
    d = head.density(xyz, enc_a, eye, geo_feat=True, count_ptr=cnt.data_ptr(), out=out)
    n = min(M, count)
    for k in ("sigma", "ambient_aud", "ambient_eye", "geo_feat"):
        assert torch.equal(d[k][:n], full[k][:n]) and bool(torch.isnan(d[k][n:]).all()), k


@pytest.mark.parametrize("use_eye", [True, False])
def test_f32_density_equals_the_checker(params, golden, use_eye):
    head, p = _head(params, 1.0, use_eye, "f32")
    M = 33
    xyz = _points(M, 1.0, 5)
    enc_a, eye = golden["net_enc_a"], golden["net_eye"] if use_eye else None
    spec = TriplaneSpec(1.0)
    ref = oracle_density(spec, p, encode_x(spec, xyz, p), enc_a, eye)
    d = head.density(dev(xyz), dev(enc_a), None if eye is None else dev(eye), geo_feat=True)
    assert d["geo_feat"].dtype == torch.float32 and d["geo_feat"].shape == (M, 64)
    assert np.array_equal(d["sigma"].cpu().numpy(), ref["sigma"])
    assert np.array_equal(d["ambient_aud"].cpu().numpy(), ref["ambient_aud"])
    assert np.array_equal(d["geo_feat"].cpu().numpy(), ref["geo_feat"])
    if use_eye:
        assert np.array_equal(d["ambient_eye"].cpu().numpy(), ref["ambient_eye"])
    else:
        assert d["ambient_eye"] is None and ref["ambient_eye"] is None


def test_f16_density_against_the_references_autocast_density(params, golden):
    """tests/golden/reference_autocast.npz holds NeRFNetwork.density's own output under autocast on the fixture's points: sigma under the
    rule tests/test_gpu_parity.py applies to the forward (<= 4 half ulps, > 0.85 equal), geo_feat within the 8 half ulps
    tests/test_golden_autocast.py grants the checker against h_density_geo."""
    ac = np.load(os.path.join(HERE, "golden", "reference_autocast.npz"), allow_pickle=False)
    head, _ = _head(params, 1.0, True, "f16")
    d = head.density(dev(golden["net_xyz"]), dev(golden["net_enc_a"]), dev(golden["net_eye"]), geo_feat=True)
    F16 = np.float16

    def ulps(a, b):
        a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
        return np.abs(a - b) / 2.0 ** (np.floor(np.log2(np.maximum(np.maximum(np.abs(a), np.abs(b)), 2.0 ** -10))) - 10)
    sg = d["sigma"].cpu().numpy()
    us, same = ulps(sg.astype(F16), ac["h_density_sigma"]).max(), np.mean(sg.astype(F16) == ac["h_density_sigma"])
    geo = d["geo_feat"].cpu().numpy()
    assert geo.dtype == F16 and geo.shape == (sg.shape[0], 64)
    n = ac["h_density_geo"].shape[0]
    ug = ulps(geo[:n], ac["h_density_geo"]).max()
    print("f16 density vs the reference's autocast density(): sigma %.2f half ulps, %.3f equal; geo_feat %.2f half ulps" % (us, same, ug))
    assert us <= 4 and same > 0.85
    assert ug <= 8


def _grid_case(bound, G, seed):
    rng = np.random.default_rng(seed)
    C = 1 + int(math.ceil(math.log2(bound)))
    cells = G ** 3
    grid0 = rng.uniform(0, 2, (C, cells)).astype(np.float32)
    grid0[rng.uniform(size=grid0.shape) < 0.2] = -1.0      # untrained cells stay untouched (renderer.py:763)
    grid0[rng.uniform(size=grid0.shape) < 0.2] = 0.0
    noise = rng.uniform(0, 1, (C, cells, 3)).astype(np.float32)
    return C, cells, grid0, noise


@pytest.mark.parametrize("precision", ["f32", "f16"])
@pytest.mark.parametrize("bound,G", [(1.0, 16), (2.0, 16), (1.5, 16)])
def test_density_only_grid_update_keeps_every_bit(params, golden, bound, G, precision):
    from lzzx_nerf_amd.occupancy import update_density_grid
    head, p = _head(params, bound, True, precision)
    C, cells, grid0, noise = _grid_case(bound, G, int(bound * 10) + G)
    assert (grid0 == -1).any() and (grid0 == 0).any()
    enc_a, eye = golden["net_enc_a"], golden["net_eye"]
    res = []
    for only in (False, True):
        dg = dev(grid0)
        bf = torch.zeros(C * cells // 8, dtype=torch.uint8, device="cuda")
        mean, thresh = update_density_grid(head, dg, bf, dev(enc_a), dev(eye), bound=bound, noise=dev(noise), density_only=only)
        res.append((dg, bf, mean, thresh))
    for a, b in zip(res[0], res[1]):
        assert torch.equal(a, b)
    assert not torch.equal(res[1][0], dev(grid0)) and int((res[1][0] == -1).sum()) == int((grid0 == -1).sum())
    if (bound, precision) == (1.0, "f32"):     # and the checker's grid and bitfield, bit for bit
        ref_grid = grid0.copy()
        _, _, bits_o = oracle_update(TriplaneSpec(bound), p, ref_grid, enc_a, eye, bound, noise)
        assert np.array_equal(res[1][0].cpu().numpy(), ref_grid) and np.array_equal(res[1][1].cpu().numpy(), bits_o)


@pytest.mark.parametrize("use_eye", [True, False])
@pytest.mark.parametrize("bound", [1.0, 2.0])
def test_ambient_grids_equal_their_restatement(params, golden, bound, use_eye):
    """get_audio_grid / get_eye_grid (renderer.py:823-933) from parts that exist without the lattice kernel: lz_density_grid_points ->
    head.density -> scatter by morton3D -> morton3D_dilation"""
    from lzzx_nerf_amd import raymarching
    from lzzx_nerf_amd._util import call, ptr, stream
    from lzzx_nerf_amd.occupancy import ambient_grids
    head, _ = _head(params, bound, use_eye, "f32")
    G = 8
    C, cells, _, noise = _grid_case(bound, G, 3)
    enc_a, eye, noise = dev(golden["net_enc_a"]), dev(golden["net_eye"]) if use_eye else None, dev(noise)
    aud, eyg = ambient_grids(head, enc_a, eye, bound, grid_size=G, noise=noise)
    xyzs = torch.empty(C * cells, 3, device="cuda")
    call("lz_density_grid_points", ptr(noise), C, G, float(bound), ptr(xyzs), stream())
    d = head.density(xyzs, enc_a, eye)
    ax = torch.arange(G, dtype=torch.int32, device="cuda")
    coords = torch.stack(torch.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)
    idx = raymarching.morton3D(coords).long()

    def restate(v):
        tmp = torch.zeros(C, cells, device="cuda")
        for cas in range(C):
            tmp[cas, idx] = v.reshape(C, cells)[cas]
        return raymarching.morton3D_dilation(tmp)
    assert aud.shape == (C, cells) and torch.equal(aud, restate(d["ambient_aud"])) and bool((aud > 0).all())
    if use_eye:
        assert torch.equal(eyg, restate(d["ambient_eye"])) and bool((eyg > 0).all())
    else:
        assert eyg is None


@pytest.mark.parametrize("precision", ["f32", "f16"])
@pytest.mark.parametrize("R", [1, 5])
def test_density_field_equals_density_on_the_meshgrid(params, golden, R, precision):
    """extract_fields (utils.py:348-363) on a box that is not a cube"""
    from lzzx_nerf_amd.occupancy import density_field
    head, _ = _head(params, 1.0, True, precision)
    enc_a, eye = dev(golden["net_enc_a"]), dev(golden["net_eye"])
    lo, hi = (-1.0, -0.6, -0.25), (0.9, 0.7, 1.0)
    u = density_field(head, enc_a, eye, lo, hi, R)
    axes = [torch.linspace(lo[k], hi[k], R, device="cuda") for k in range(3)]
    pts = torch.stack(torch.meshgrid(*axes, indexing="ij"), -1).reshape(-1, 3).contiguous()
    ref = head.density(pts, enc_a, eye)["sigma"].reshape(R, R, R)
    assert u.shape == (R, R, R) and u.dtype == torch.float32 and u.is_cuda
    assert torch.equal(u, ref)
    if R > 1:
        assert len(torch.unique(u)) > R        # a field, not a constant


@pytest.mark.parametrize("precision", ["f32", "f16"])
def test_empty_inputs(params, golden, precision):
    from lzzx_nerf_amd.occupancy import density_field
    head, _ = _head(params, 1.0, True, precision)
    enc_a, eye = dev(golden["net_enc_a"]), dev(golden["net_eye"])
    d = head.density(torch.empty(0, 3, device="cuda"), enc_a, eye, geo_feat=True)
    assert d["sigma"].shape == (0,) and d["ambient_aud"].shape == (0, 1) and d["ambient_eye"].shape == (0, 1) and d["geo_feat"].shape == (0, 64)
    assert density_field(head, enc_a, eye, (-1, -1, -1), (1, 1, 1), 0).shape == (0, 0, 0)
    torch.cuda.synchronize()


def test_c_entry_rejects_a_null_sigma(params, golden):
    import ctypes as C
    from lzzx_nerf_amd import _lib
    head, _ = _head(params, 1.0, True, "f32")
    xyz, aud = torch.zeros(4, 3, device="cuda"), torch.zeros(4, device="cuda")
    p, _ = head._density_inputs(dev(golden["net_enc_a"]), dev(golden["net_eye"]))
    lib = _lib.load()
    vp = lambda t: C.c_void_p(t.data_ptr())
    assert lib.lz_triplane_head_density(C.byref(p), vp(xyz), 4, None, None, vp(aud), None, None, None) == -2
    assert b"null" in lib.lz_last_error()
    assert lib.lz_triplane_density_lattice(C.byref(p), _lib.LZ_LATTICE_AXES, None, 0, 0, vp(xyz), 2, vp(xyz), 2, vp(xyz), 2, None, None, None, None) == -2
