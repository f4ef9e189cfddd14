"""Mesh extraction without a GPU: the generated case table, the meshes of the numpy checker that the GPU tests compare against
(tests/mesh_checker.py -- table and checker share one source, so these properties are what stands between a wrong table and a
green GPU run), the C ABI of csrc/lz_mesh.hip, its kernels' resources and the PLY writer."""
import ctypes as C
import json
import os
import re

import numpy as np

import mesh_checker as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the table ----
def test_table_facts():
    g = M.gen_mc_tables
    tab = g.table()
    assert len(tab) == 256 and sum(len(t) for t in tab) == 820 and max(len(t) for t in tab) == 5
    assert tab[0] == [] and tab[255] == []
    for c in range(256):
        cut = set(g.cut_edges(c))
        used = {e for t in tab[c] for e in t}
        assert used == cut, c                                   # every row's edges are cut edges of that case, and all of them
        assert all(len(set(t)) == 3 for t in tab[c]), c
        assert all(s != 0 for s in g.case_loops(c)[1]), c       # the orientation sum is never 0


def test_committed_header_is_the_generators_output():
    assert open(os.path.join(ROOT, "include", "lzzx_mc_tables.h")).read() == M.gen_mc_tables.emit()


# ---- the checker's own meshes ----
def test_all_cases_lattice_is_closed_and_oriented():
    u = M.all_cases_lattice()
    assert u.shape == (49, 49, 4)
    v, t = M.marching_cubes(u, 0.5)
    assert t.min() >= 0 and t.max() < len(v)
    assert M.every_vertex_used(v, t) and M.edges_balanced(t)
    assert M.signed_volume(v, t) > 0


def test_every_case_alone_is_closed_with_positive_volume():
    for c in range(1, 256):
        v, t = M.marching_cubes(M.single_case_lattice(c), 0.5)
        assert len(t) > 0 and M.edges_balanced(t) and M.every_vertex_used(v, t) and M.signed_volume(v, t) > 0, c


def test_sphere_and_torus():
    h = 2.0 / 23.0          # node spacing of 24^3 over [-1, 1]^3
    for field, chi, analytic, tol in ((M.sphere_field(), 2, 4.0 / 3.0 * np.pi * 0.7 ** 3, 0.02),
                                      (M.torus_field(), 0, 2.0 * np.pi ** 2 * 0.6 * 0.25 ** 2, 0.04)):
        v, t = M.marching_cubes(field, 0.0)
        assert M.edges_once(t) and M.every_vertex_used(v, t)
        assert M.euler_characteristic(v, t) == chi
        vol = M.signed_volume(v, t) * h ** 3
        print("volume", vol, "analytic", analytic, "deficit", 1 - vol / analytic)
        assert analytic * (1 - tol) <= vol <= analytic          # the chordal surface lies inside


def test_random_field_counts():
    v, t = M.marching_cubes(M.random_field((9, 7, 11), 0), 0.5)
    assert (len(v), len(t)) == (538, 1084)
    assert M.edges_balanced(t) and M.every_vertex_used(v, t)
    assert sum(1 for c in M.directed_edge_counts(t).values() if c == 2) == 4     # fan diagonals that coincide across an ambiguous face


def test_vertex_rule_on_non_finite_and_equal_nodes():
    u = np.zeros((2, 2, 3), np.float32)
    u[0, 0] = (np.inf, -np.inf, np.nan)
    u[1, 1] = (2.0, 0.5, 0.5)
    v, t = M.marching_cubes(u, 0.5)
    assert np.isfinite(v).all() and (v >= 0).all() and (v <= np.array([1, 1, 2], np.float32)).all()
    assert t.max() < len(v)


# ---- C ABI ----
def _header():
    src = open(os.path.join(ROOT, "include", "lzzx_nerf_hip.h")).read()
    return src, re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_entries_are_declared_exported_and_bound():
    from lzzx_nerf_amd import _lib
    src, code = _header()
    for n in ("lz_mc_workspace", "lz_mc_count", "lz_mc_emit"):
        assert re.search(r"\b%s\s*\(" % n, code), n
        assert n in _lib.ALL_SYMBOLS
    assert "utils.py:366-378" in src
    lib = _lib.load()
    assert lib.lz_abi_version() == _lib.ABI_VERSION == 11
    assert len(_lib.SIGNATURES["lz_mc_count"]) == 8 and len(_lib.SIGNATURES["lz_mc_emit"]) == 11
    # tile totals (8 bytes per tile of 256 nodes of a row) + their sums per 1024 tiles + one 16-bit word per node, each 16-byte aligned
    assert lib.lz_mc_workspace(256, 256, 256) == 8 * 256 * 256 + 8 * 64 + 2 * 256 ** 3
    assert lib.lz_mc_workspace(3, 5, 300) == 8 * 3 * 5 * 2 + 16 + (2 * 3 * 5 * 300 + 15) // 16 * 16      # rows of two tiles
    assert lib.lz_mc_workspace(5, 1, 5) == 0


def test_bad_arguments_are_rejected_before_any_launch():
    """no device here: a call that got as far as a launch would come back as a HIP error, not as LZ_ERR_BAD_ARGUMENT"""
    from lzzx_nerf_amd import _lib
    lib = _lib.load()
    p = C.c_void_p(0x10000)
    assert lib.lz_mc_count(None, 4, 4, 4, 0.5, p, p, None) == -2
    assert lib.lz_mc_count(p, 4, 4, 4, 0.5, None, p, None) == -2
    assert lib.lz_mc_count(p, 4, 4, 4, 0.5, p, None, None) == -2
    assert "null" in lib.lz_last_error().decode()
    assert lib.lz_mc_emit(None, 4, 4, 4, 0.5, p, 4, 4, p, p, None) == -2
    assert lib.lz_mc_emit(p, 4, 4, 4, 0.5, None, 4, 4, p, p, None) == -2
    assert lib.lz_mc_emit(p, 4, 4, 4, 0.5, p, 4, 4, None, p, None) == -2
    assert lib.lz_mc_emit(p, 4, 4, 4, 0.5, p, 4, 4, p, None, None) == -2
    assert lib.lz_mc_count(p, 4, 4, 4, 0.5, C.c_void_p(0x10008), p, None) == -2       # workspace alignment
    # 3 nodes >= 2^31: 896^3 * 3 = 2157969408
    for dims in ((896, 896, 896), (65536, 65536, 2), (2, 2, 357913942)):
        assert 3 * dims[0] * dims[1] * dims[2] >= 2 ** 31
        assert lib.lz_mc_count(p, *dims, 0.5, p, p, None) == -2, dims
        assert "2^31" in lib.lz_last_error().decode()
        assert lib.lz_mc_emit(p, *dims, 0.5, p, 4, 4, p, p, None) == -2, dims
        assert lib.lz_mc_workspace(*dims) == 0
    assert 3 * 2 * 2 * 178956970 < 2 ** 31 and lib.lz_mc_workspace(2, 2, 178956970) > 0   # the largest row that still fits


def test_empty_lattice_is_ok_without_a_launch():
    from lzzx_nerf_amd import _lib
    lib = _lib.load()
    for dims in ((0, 0, 0), (1, 5, 5), (5, 1, 5), (5, 5, 1)):
        assert lib.lz_mc_count(None, *dims, 0.5, None, None, None) == 0, dims
        assert lib.lz_mc_emit(None, *dims, 0.5, None, 4, 4, None, None, None) == 0, dims
    assert lib.lz_mc_emit(None, 4, 4, 4, 0.5, None, 0, 0, None, None, None) == 0          # nothing to write


def test_python_rejects_oversize_and_wrong_inputs():
    import pytest
    import torch
    from lzzx_nerf_amd import mesh
    with pytest.raises(RuntimeError):
        mesh.marching_cubes(torch.zeros(4, 4, 4), 0.5)             # not on the device
    with pytest.raises(RuntimeError):
        mesh.marching_cubes(torch.zeros(4, 4), 0.5)


# ---- resources ----
def test_mesh_kernels_do_not_spill():
    from lzzx_nerf_amd import build as B
    if not os.path.exists(B.RESOURCES) or not B.up_to_date():
        B.build(force=True)
    assert "lz_mesh.hip" in B.SOURCES
    res = json.load(open(B.RESOURCES))["lz_mesh.hip"]
    names = sorted(res)
    assert len(names) == 4 and all(any(k in n for n in names) for k in ("lz_k_mc_count", "lz_k_mc_scan_tiles", "lz_k_mc_scanP", "lz_k_mc_emit")), names
    for n, r in res.items():
        assert r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch"] == 0, (n, r)
        assert r["lds"] <= 8192, (n, r)


# ---- PLY ----
def test_ply_round_trip(tmp_path):
    import torch
    from lzzx_nerf_amd.mesh import save_mesh, to_world
    v, t = M.marching_cubes(M.sphere_field(12), 0.0)
    path = str(tmp_path / "sphere.ply")
    save_mesh(path, torch.from_numpy(v), torch.from_numpy(t))
    head = open(path, "rb").read(200).decode("ascii", "replace")
    assert head.startswith("ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % len(v)) and "element face %d\n" % len(t) in head
    pv, pt = M.parse_ply(path)
    assert pv.dtype == np.float32 and pt.dtype == np.int32
    assert np.array_equal(pv, v) and np.array_equal(pt, t)
    save_mesh(path, v[:0], t[:0])                                   # an empty mesh is a valid file
    pv, pt = M.parse_ply(path)
    assert pv.shape == (0, 3) and pt.shape == (0, 3)
    # utils.py:377 in float64 from the f32 operands, rounded once
    lo, hi = (-1.0, -0.6, -0.25), (0.9, 0.7, 1.0)
    w = to_world(torch.from_numpy(v), lo, hi, 12).numpy()
    lo64, hi64 = np.array(lo, np.float32).astype(np.float64), np.array(hi, np.float32).astype(np.float64)
    assert np.array_equal(w, (v.astype(np.float64) / 11.0 * (hi64 - lo64)[None] + lo64[None]).astype(np.float32))
