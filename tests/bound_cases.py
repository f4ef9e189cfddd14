"""Inputs for the tests of the box-to-unit mapping `(x + bound) / (2 * bound)` (gridencoder/grid.py:143) at bounds where 2 bound is no
power of two -- shared by tests/test_bound_mapping_host.py (CPU) and tests/test_gpu_bound_mapping.py.  TEST INFRASTRUCTURE ONLY.

The line can be evaluated in two f32 arithmetics, named here once and never used one for the other:
  map01_div   the true division, one rounding: numpy, torch on the CPU
  map01_rcp   the add, then a multiplication by the f32 reciprocal of 2 bound, two roundings: torch on the device for a tensor divided by
              a host scalar (tests/test_gpu_bound_mapping.py::test_device_division_by_scalar_is_a_reciprocal_multiply)
They agree bit for bit when 2 bound is a power of two and on about two thirds of all coordinates otherwise.  Most disagreements move a
feature by an ulp of the interpolation fraction; a few move `floor(x01 * scale + 0.5)`, the CELL of some level, and those coordinates
("cell-flipping") are searched for and placed in the batches below, so that a kernel in the wrong arithmetic reads other table entries."""
import functools

import numpy as np

from oracle import oracle as O
from oracle.head import TriplaneSpec

F32 = np.float32
BOUNDS = (1.5, 0.75)                      # every test; cascades 1 + ceil(log2(bound)) = 2 and 1
ENCODER_BOUNDS = (1.5, 0.75, 2.5625)      # encoder-level tests: at 2.5625 the box surface x = +bound maps to 1 (div) or 1 - 2^-24 (rcp)
N_DRAWS = 1 << 22
MAX_FLIPS = 48                            # cell-flipping coordinates placed per batch
CFG2 = dict(num_levels=16, base_resolution=16, desired_resolution=2048, log2_hashmap_size=19)     # get_encoder('hashgrid') defaults


def map01_div(x, bound):
    b = F32(bound)
    return ((np.asarray(x, F32) + b) / (F32(2) * b)).astype(F32)


def map01_rcp(x, bound):
    b = F32(bound)
    return ((np.asarray(x, F32) + b) * (F32(1) / (F32(2) * b))).astype(F32)


def cascades(bound):
    return 1 + int(np.ceil(np.log2(bound)))


@functools.lru_cache(maxsize=None)
def draws(bound):
    """2^22 seeded f32 coordinates, uniform in [-bound, bound]; shared, read-only"""
    u = np.random.default_rng(int(round(bound * 10000))).random(N_DRAWS, dtype=F32)
    x = ((u * F32(2) - F32(1)) * F32(bound)).astype(F32)
    x.setflags(write=False)
    return x


def level_scales(kind, bound):
    """the per-level scale as oracle.grid_encode_forward forms it (S narrowed to float at the binding; the checker's level parameters)"""
    if kind == "triplane":
        spec = TriplaneSpec(bound)
        return O.grid_level_params(spec.num_levels, F32(np.log2(spec.per_level_scale)), spec.base_resolution)[0]
    pls = np.exp2(np.log2(CFG2["desired_resolution"] / CFG2["base_resolution"]) / (CFG2["num_levels"] - 1))
    return O.grid_level_params(CFG2["num_levels"], F32(np.log2(pls)), CFG2["base_resolution"])[0]


def cells(x01, scale):
    """floor(x01 * scale + 0.5) in f32, the product and sum rounded once (the kernels' and the checker's fma)"""
    return np.floor((np.asarray(x01, np.float64) * np.float64(scale) + 0.5).astype(F32)).astype(np.int64)


@functools.lru_cache(maxsize=None)
def flips(kind, bound):
    """the draws at which, for some level, the cell differs between the two candidates; in draw order, read-only"""
    x = draws(bound)
    a, b = map01_div(x, bound), map01_rcp(x, bound)
    hit = np.zeros(x.shape, bool)
    for s in level_scales(kind, bound):
        hit |= cells(a, s) != cells(b, s)
    out = x[hit].copy()
    out.setflags(write=False)
    return out


FIRST_FLIP_ROW = 8


def flip_rows(kind, bound, B):
    """(rows, columns) of the cell-flipping coordinates in points(bound, B, kind)"""
    n = min(len(flips(kind, bound)), MAX_FLIPS, B - 1 - FIRST_FLIP_ROW)
    return FIRST_FLIP_ROW + np.arange(n), np.arange(n) % 3


@functools.lru_cache(maxsize=None)
def points(bound, B, kind="triplane"):
    """[B, 3] f32: seeded uniform points in the box; rows 0 .. 5 and B - 1 as tests/test_gpu_triplane_encoder.points places them (corners
    exactly at +-bound, one coordinate outside per row, one just outside by 2^-20, the last row on the surface); from row 8 on one
    cell-flipping coordinate per row, as x, y, z in turn (the other two coordinates stay uniform).  Read-only."""
    assert B >= 32
    b = F32(bound)
    rng = np.random.default_rng(99 + B)
    x = ((rng.random((B, 3), dtype=F32) * F32(2) - F32(1)) * b).astype(F32)
    x[0] = (b, b, b)
    x[1] = (-b, -b, -b)
    x[2] = (b, -b, F32(0.25) * b)
    x[3, 0] = F32(1.25) * b
    x[4, 1] = F32(-1.5) * b
    x[5, 2] = b * F32(1 + 2.0 ** -20)
    x[B - 1] = (-b, F32(0.5) * b, b)
    rows, cols = flip_rows(kind, bound, B)
    x[rows, cols] = flips(kind, bound)[:len(rows)]
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def dirs(B):
    d = np.random.default_rng(7 + B).normal(size=(B, 3)).astype(F32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def triplane_tables(bound):
    """the three planes' tables for TriplaneSpec(bound), uniform in [-1, 1] (the recipe of tests/test_gpu_occupancy._params_for_bound)"""
    spec = TriplaneSpec(bound)
    rng = np.random.default_rng(int(round(bound * 10000)) + 1)
    p = {}
    for n in ("xy", "yz", "xz"):
        p[f"encoder_{n}.embeddings"] = rng.uniform(-1, 1, (spec.n_params, 1)).astype(F32)
        p[f"encoder_{n}.offsets"] = spec.offsets.astype(np.int32)
    return p


def triplane_params(params, bound):
    """the fixture's network weights with the tables of triplane_tables(bound)"""
    p = dict(params)
    p.update(triplane_tables(bound))
    return p


def encode_x_with(map01, spec, xyz, P):
    """oracle.head.encode_x with the mapping passed in: the checker's features under one NAMED candidate"""
    xyz = np.ascontiguousarray(xyz, F32)
    out = []
    for n, c in (("xy", [0, 1]), ("yz", [1, 2]), ("xz", [0, 2])):
        f, _ = O.grid_encode_forward(map01(xyz[:, c], spec.bound), P[f"encoder_{n}.embeddings"], spec.offsets, spec.per_level_scale,
                                     spec.base_resolution)
        out.append(f)
    return np.concatenate(out, 1)
