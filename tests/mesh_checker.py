"""numpy restatement of the mesh definition of DESIGN 4.13 (csrc/lz_mesh.hip), shared by test_mesh_host.py and test_gpu_mesh.py.

    vertices [V,3] f32, triangles [T,3] int32 = marching_cubes(u [Rx,Ry,Rz] f32, thr)

The case table comes from tools/gen_mc_tables.py, the generator of include/lzzx_mc_tables.h; every arithmetic step is one f32
operation.  Also here: the lattices the tests use and the mesh properties they assert.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_mc_tables  # noqa: E402

_TAB = gen_mc_tables.table()
NTRI = np.array([len(t) for t in _TAB], dtype=np.int64)
TRI = np.zeros((256, 5, 3), dtype=np.int64)
for _c, _t in enumerate(_TAB):
    for _r, _e in enumerate(_t):
        TRI[_c, _r] = _e


def marching_cubes(u, thr):
    u = np.ascontiguousarray(u, dtype=np.float32)
    thr = np.float32(thr)
    Rx, Ry, Rz = u.shape
    if min(u.shape) < 2:
        return np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)
    assert 3 * u.size < 2 ** 31
    with np.errstate(all="ignore"):
        solid = u >= thr                                  # false for NaN
        keys, pos = [], []
        for a in range(3):
            lo_s = [slice(None)] * 3
            hi_s = [slice(None)] * 3
            lo_s[a], hi_s[a] = slice(0, -1), slice(1, None)
            lo_s, hi_s = tuple(lo_s), tuple(hi_s)
            cut = solid[lo_s] != solid[hi_s]
            idx = np.argwhere(cut)                        # lower node (i, j, k), C order
            u_lo, u_hi = u[lo_s][cut], u[hi_s][cut]
            t = (thr - u_lo) / (u_hi - u_lo)              # each operation rounded to f32
            t = np.where(t >= 0, t, np.float32(0))
            t = np.where(t > 1, np.float32(1), t).astype(np.float32)
            p = idx.astype(np.float32)
            p[:, a] = p[:, a] + t
            keys.append(3 * ((idx[:, 0] * Ry + idx[:, 1]) * Rz + idx[:, 2]) + a)
            pos.append(p)
    keys, pos = np.concatenate(keys), np.concatenate(pos)
    order = np.argsort(keys, kind="stable")
    vertices = np.ascontiguousarray(pos[order], dtype=np.float32)
    vid = np.full(3 * u.size, -1, dtype=np.int64)
    vid[keys[order]] = np.arange(len(order))

    s = solid.astype(np.int64)
    case = np.zeros((Rx - 1, Ry - 1, Rz - 1), dtype=np.int64)
    for b in range(8):
        dx, dy, dz = b >> 2 & 1, b >> 1 & 1, b & 1
        case |= s[dx:Rx - 1 + dx, dy:Ry - 1 + dy, dz:Rz - 1 + dz] << b
    nt = NTRI[case]
    cells = np.argwhere(nt > 0)                           # cell index ascending
    cnt = nt[nt > 0]
    cell_of = np.repeat(np.arange(len(cells)), cnt)
    r = np.arange(len(cell_of)) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    ijk = cells[cell_of]
    e = TRI[case[ijk[:, 0], ijk[:, 1], ijk[:, 2]], r]     # [T, 3] cell edges
    a, p, q = e >> 2, e >> 1 & 1, e & 1
    dx = np.where(a == 0, 0, p)
    dy = np.where(a == 0, p, np.where(a == 1, 0, q))
    dz = np.where(a == 2, 0, q)
    node = ((ijk[:, 0:1] + dx) * Ry + ijk[:, 1:2] + dy) * Rz + ijk[:, 2:3] + dz
    tri = vid[3 * node + a]
    assert (tri >= 0).all()
    return vertices, np.ascontiguousarray(tri, dtype=np.int32).reshape(-1, 3)


# ---- lattices ----
def all_cases_lattice():
    """all 256 cases in one 49 x 49 x 4 lattice: case c in its own 2 x 2 x 2 block of nodes at (1 + 3 (c // 16), 1 + 3 (c % 16), 1),
    blocks separated by empty planes; solid 1, empty 0, to be cut at 0.5"""
    u = np.zeros((49, 49, 4), dtype=np.float32)
    for c in range(256):
        x, y = 1 + 3 * (c // 16), 1 + 3 * (c % 16)
        for b in range(8):
            if c >> b & 1:
                u[x + (b >> 2 & 1), y + (b >> 1 & 1), 1 + (b & 1)] = 1.0
    return u


def single_case_lattice(c):
    """case c alone in a 4^3 lattice of empty nodes"""
    u = np.zeros((4, 4, 4), dtype=np.float32)
    for b in range(8):
        if c >> b & 1:
            u[1 + (b >> 2 & 1), 1 + (b >> 1 & 1), 1 + (b & 1)] = 1.0
    return u


def random_field(shape, seed=0):
    """uniform-random in [0, 1) with a border of zeros"""
    u = np.random.default_rng(seed).random(shape).astype(np.float32)
    u[0], u[-1], u[:, 0], u[:, -1], u[:, :, 0], u[:, :, -1] = 0, 0, 0, 0, 0, 0
    return u


def _grid(R):
    ax = np.linspace(-1.0, 1.0, R)
    return np.meshgrid(ax, ax, ax, indexing="ij")


def sphere_field(R=24, radius=0.7):
    """solid (positive) inside; cut at 0"""
    x, y, z = _grid(R)
    return (radius - np.sqrt(x * x + y * y + z * z)).astype(np.float32)


def torus_field(R=24, major=0.6, minor=0.25):
    x, y, z = _grid(R)
    return (minor - np.sqrt((np.sqrt(x * x + y * y) - major) ** 2 + z * z)).astype(np.float32)


# ---- properties ----
def directed_edge_counts(tri):
    """{(a, b): count} over the three directed edges of every triangle"""
    t = np.asarray(tri, dtype=np.int64)
    e = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
    k, c = np.unique(e[:, 0] * (1 << 32) + e[:, 1], return_counts=True)
    return dict(zip(k.tolist(), c.tolist()))


def edges_balanced(tri):
    """count(directed edge) == count(its reverse) for every edge"""
    d = directed_edge_counts(tri)
    return all(d.get((k & 0xFFFFFFFF) << 32 | k >> 32, 0) == c for k, c in d.items())


def edges_once(tri):
    d = directed_edge_counts(tri)
    return edges_balanced(tri) and all(c == 1 for c in d.values())


def signed_volume(v, tri):
    p = np.asarray(v, dtype=np.float64)[np.asarray(tri, dtype=np.int64)]
    return float(np.einsum("ij,ij->i", p[:, 0], np.cross(p[:, 1], p[:, 2])).sum() / 6.0)


def euler_characteristic(v, tri):
    d = directed_edge_counts(tri)
    und = {(min(k >> 32, k & 0xFFFFFFFF), max(k >> 32, k & 0xFFFFFFFF)) for k in d}
    return len(v) - len(und) + len(tri)


def every_vertex_used(v, tri):
    return len(np.unique(np.asarray(tri))) == len(v)


def parse_ply(path):
    """the binary little-endian PLY of lzzx_nerf_amd.mesh.save_mesh -> (vertices [V,3] f32, triangles [T,3] int32)"""
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    lines = raw[:end].decode("ascii").split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    el = [ln.split() for ln in lines if ln.startswith("element")]
    props = [ln for ln in lines if ln.startswith("property")]
    assert [e[1] for e in el] == ["vertex", "face"]
    assert props == ["property float x", "property float y", "property float z", "property list uchar int vertex_indices"]
    V, T = int(el[0][2]), int(el[1][2])
    assert len(raw) == end + 12 * V + 13 * T
    v = np.frombuffer(raw, dtype="<f4", count=3 * V, offset=end).reshape(V, 3)
    f = np.frombuffer(raw, dtype=np.dtype([("n", "u1"), ("v", "<i4", (3,))]), count=T, offset=end + 12 * V)
    assert (f["n"] == 3).all()
    return v.copy(), f["v"].astype(np.int32).reshape(T, 3)
