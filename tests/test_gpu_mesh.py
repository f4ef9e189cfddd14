"""Marching cubes on the device (csrc/lz_mesh.hip, lzzx_nerf_amd/mesh.py): vertices and triangles are bit-equal to the numpy
restatement of the definition (tests/mesh_checker.py) on every lattice below, and extract_geometry / save_mesh carry that
mesh through the reference's affine (utils.py:377) into a PLY."""
import itertools

import numpy as np
import pytest
import torch

import mesh_checker as M

pytestmark = pytest.mark.gpu

LZM_TILE = 256        # csrc/lz_mesh.hip: nodes of a lattice row per workgroup; a row longer than this is split into tiles
LZM_SCAN_WG = 1024    # csrc/lz_mesh.hip: tiles per workgroup of the first scan level; beyond LZM_SCAN_WG^2 tiles a thread of the second
                      # level, one workgroup, scans several group sums


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def check_equal(u, thr):
    from lzzx_nerf_amd.mesh import marching_cubes
    v, t = marching_cubes(dev(u), thr)
    rv, rt = M.marching_cubes(u, thr)
    assert v.dtype == torch.float32 and t.dtype == torch.int32 and v.is_cuda and t.is_cuda
    assert v.shape == rv.shape and t.shape == rt.shape, (v.shape, rv.shape, t.shape, rt.shape)
    assert torch.equal(t.cpu(), torch.from_numpy(rt))
    assert np.array_equal(v.cpu().numpy().view(np.uint32), rv.view(np.uint32))     # bits (NaN-proof, -0 != +0)
    return v, t


def test_all_cases_lattice():
    v, t = check_equal(M.all_cases_lattice(), 0.5)
    assert len(v) == 4608 and len(t) == 7796


def _tiles(shape):
    return shape[0] * shape[1] * ((shape[2] + LZM_TILE - 1) // LZM_TILE)


# (33, 17, 65): odd extents, rows that end inside a wave, 561 tiles.  (3, 5, 300): rows of two tiles, the cells and the z edges across
# the tile boundary.  (35, 31, 7): 1085 tiles > LZM_SCAN_WG, two groups of the first scan level, the second one partly filled.
@pytest.mark.parametrize("shape", [(9, 7, 11), (33, 17, 65), (3, 5, 300), (35, 31, 7)])
def test_random_fields(shape):
    if shape == (3, 5, 300):
        assert shape[2] > LZM_TILE
    if shape == (35, 31, 7):
        assert LZM_SCAN_WG < _tiles(shape) < 2 * LZM_SCAN_WG
    v, t = check_equal(M.random_field(shape, 0), 0.5)
    if shape == (9, 7, 11):
        assert len(v) == 538 and len(t) == 1084


def test_more_tiles_than_the_scan_levels_hold_at_one_per_thread():
    """1025 x 1024 rows: 1 049 600 tiles > LZM_SCAN_WG^2, so the second scan level runs with two group sums per thread (and none for
    the last threads).  The smallest lattice that gets there has two nodes per row; it cannot have a border of zeros."""
    shape = (1025, 1024, 2)
    assert _tiles(shape) > LZM_SCAN_WG ** 2
    u = np.random.default_rng(6).random(shape).astype(np.float32)
    check_equal(u, 0.9)


def test_integer_field_keeps_degenerate_triangles():
    """thr equal to node values: t = 0, vertices coincide with nodes, triangles of zero area stay"""
    u = np.random.default_rng(1).integers(0, 4, (13, 9, 11)).astype(np.float32)
    v, t = check_equal(u, 2.0)
    v = v.cpu().numpy()
    assert len(t) > 0 and (v == np.round(v)).all(axis=1).any()
    p = v[t.cpu().numpy().astype(np.int64)]
    assert (np.abs(np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])).sum(1) == 0).any()     # degenerate triangles are kept


def test_non_finite_field():
    rng = np.random.default_rng(2)
    u = M.random_field((12, 10, 9), 2)
    kind = rng.integers(0, 12, u.shape)
    u[kind == 0], u[kind == 1], u[kind == 2] = np.inf, -np.inf, np.nan
    v, t = check_equal(u, 0.5)
    rv, rt = M.marching_cubes(u, 0.5)
    assert len(v) == len(rv) > 0 and len(t) == len(rt) > 0
    v, t = v.cpu().numpy(), t.cpu().numpy()
    assert t.min() >= 0 and t.max() < len(v)
    assert np.isfinite(v).all()
    frac = v - np.floor(v)           # every vertex inside its lattice edge: at most one coordinate off a node, by t in [0, 1]
    assert ((frac != 0).sum(1) <= 1).all()
    assert (v >= 0).all() and (v <= np.array(u.shape, np.float32) - 1).all()


@pytest.mark.parametrize("shape,fill,thr", [((6, 5, 7), 0.0, 0.5), ((6, 5, 7), 1.0, 0.5), ((1, 5, 5), 0.0, -1.0), ((5, 1, 5), 1.0, 0.5),
                                            ((5, 5, 1), 1.0, 0.5), ((0, 3, 3), 0.0, 0.5)])
def test_empty_outputs(shape, fill, thr):
    from lzzx_nerf_amd.mesh import marching_cubes
    u = torch.full(shape, fill, dtype=torch.float32, device="cuda")
    if min(shape) == 1:
        u.view(-1)[::2] = 5.0          # solid and empty nodes alternate, and still no cell
    v, t = marching_cubes(u, thr)
    assert v.shape == (0, 3) and t.shape == (0, 3) and v.dtype == torch.float32 and t.dtype == torch.int32
    torch.cuda.synchronize()


def test_non_cubic_extents_and_transposes():
    base = M.random_field((5, 7, 9), 3)
    v0, _ = check_equal(base, 0.5)
    rows0 = np.sort(v0.cpu().numpy().view([("x", "f4"), ("y", "f4"), ("z", "f4")]).ravel())
    for perm in itertools.permutations(range(3)):
        u = np.ascontiguousarray(base.transpose(perm))
        v, t = check_equal(u, 0.5)
        back = np.empty_like(v.cpu().numpy())
        back[:, list(perm)] = v.cpu().numpy()        # axis perm[d] of the base is axis d of the transpose
        rows = np.sort(np.ascontiguousarray(back).view([("x", "f4"), ("y", "f4"), ("z", "f4")]).ravel())
        assert np.array_equal(rows, rows0), perm     # the same vertices, numbered otherwise


def test_padded_outputs_stay_untouched():
    """40 rows of NaN / -1 behind V and T stay as they are, also when lz_mc_emit gets capacities below the true totals"""
    from lzzx_nerf_amd import _lib
    from lzzx_nerf_amd._util import call, ptr, stream
    u_np = M.random_field((33, 17, 65), 4)
    rv, rt = M.marching_cubes(u_np, 0.5)
    u = dev(u_np)
    ws = torch.empty(_lib.load().lz_mc_workspace(*u.shape), dtype=torch.uint8, device="cuda")
    totals = torch.zeros(2, dtype=torch.int32, device="cuda")
    call("lz_mc_count", ptr(u), *u.shape, 0.5, ptr(ws), ptr(totals), stream())
    V, T = totals.tolist()
    assert (V, T) == (len(rv), len(rt))
    pad = 40
    for v_cap, t_cap in ((V, T), (V - 5, T - 7), (V // 2, 3), (1, T)):
        vb = torch.full((V + pad, 3), float("nan"), device="cuda")
        tb = torch.full((T + pad, 3), -1, dtype=torch.int32, device="cuda")
        call("lz_mc_emit", ptr(u), *u.shape, 0.5, ptr(ws), v_cap, t_cap, ptr(vb), ptr(tb), stream())
        assert torch.equal(vb[:v_cap].cpu(), torch.from_numpy(rv[:v_cap])) and torch.equal(tb[:t_cap].cpu(), torch.from_numpy(rt[:t_cap]))
        assert torch.isnan(vb[v_cap:]).all() and (tb[t_cap:] == -1).all()


def test_repeatable():
    from lzzx_nerf_amd.mesh import marching_cubes
    u = dev(M.random_field((33, 17, 65), 5))
    v0, t0 = marching_cubes(u, 0.5)
    v1, t1 = marching_cubes(u, 0.5)
    assert torch.equal(v0, v1) and torch.equal(t0, t1) and len(v0) > 0


@pytest.mark.parametrize("precision", ["f32", "f16"])
def test_extract_geometry_end_to_end(params, golden, precision):
    """the non-cubic box of test_density_field_equals_density_on_the_meshgrid at resolution 12, cut at the field's median"""
    from lzzx_nerf_amd.mesh import extract_geometry, marching_cubes
    from lzzx_nerf_amd.occupancy import density_field
    from test_gpu_density import _head
    head, _ = _head(params, 1.0, True, precision)
    enc_a, eye = dev(golden["net_enc_a"]), dev(golden["net_eye"])
    lo, hi, R = (-1.0, -0.6, -0.25), (0.9, 0.7, 1.0), 12
    u = density_field(head, enc_a, eye, lo, hi, R)
    thr = float(u.median())
    v, t = extract_geometry(head, enc_a, eye, lo, hi, R, thr)
    rv, rt = M.marching_cubes(u.cpu().numpy(), thr)
    assert len(rv) > 0 and v.is_cuda and t.is_cuda and v.dtype == torch.float32 and t.dtype == torch.int32
    vi, ti = marching_cubes(u, thr)
    assert torch.equal(vi.cpu(), torch.from_numpy(rv)) and torch.equal(ti.cpu(), torch.from_numpy(rt)) and torch.equal(t, ti)
    lo64, hi64 = np.array(lo, np.float32).astype(np.float64), np.array(hi, np.float32).astype(np.float64)
    world = (rv.astype(np.float64) / (R - 1.0) * (hi64 - lo64)[None] + lo64[None]).astype(np.float32)
    assert np.array_equal(v.cpu().numpy(), world)


def test_pipeline_save_mesh(params, golden, tmp_path):
    from conftest import ellipsoid_bitfield
    from lzzx_nerf_amd.mesh import extract_geometry
    from lzzx_nerf_amd.occupancy import density_field
    from lzzx_nerf_amd.pipeline import TalkingHeadFrame
    from test_audio_oracle import audio_state
    sd = dict(params)
    sd.update(audio_state(29, 32, True))
    frame = TalkingHeadFrame({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, dev(ellipsoid_bitfield()[0]), bound=1.0)
    auds = dev(np.random.default_rng(9).normal(size=(8, 29, 16)).astype(np.float32))
    eye = dev(golden["net_eye"])
    enc_a = frame.audio(auds)
    aabb = frame.renderer.aabb
    thr = float(density_field(frame.head, enc_a, eye, aabb[:3], aabb[3:], 12).median())
    path = str(tmp_path / "meshes" / "head.ply")
    v, t = frame.save_mesh(path, auds, eye=eye, resolution=12, threshold=thr)
    pv, pt = M.parse_ply(path)
    assert len(pv) > 0 and len(pt) > 0
    assert np.array_equal(pv, v.cpu().numpy()) and np.array_equal(pt, t.cpu().numpy())
    ev, et = extract_geometry(frame.head, enc_a, eye, aabb[:3], aabb[3:], 12, thr)
    assert torch.equal(ev, v) and torch.equal(et, t)
    v2, t2 = frame.save_mesh(str(tmp_path / "again.ply"), enc_a, eye=eye, resolution=12, threshold=thr)     # an audio code instead of windows
    assert torch.equal(v2, v) and torch.equal(t2, t)
