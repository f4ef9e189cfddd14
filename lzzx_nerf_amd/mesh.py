"""Mesh extraction on the device: `extract_geometry` and `save_mesh` of the reference (nerf_triplane/utils.py:366-378,
TrainerUtil.py:444-463) without `mcubes` and `trimesh` -- marching cubes as HIP kernels (csrc/lz_mesh.hip) on the lattice
`occupancy.density_field` writes, and a PLY writer.

    vertices, triangles = marching_cubes(u, threshold)                                          # mcubes.marching_cubes
    vertices, triangles = extract_geometry(head, enc_a, eye, bound_min, bound_max, resolution, threshold)
    save_mesh(path, vertices, triangles)                                                        # trimesh.Trimesh(...).export(path)

The mesh is defined by this project, a function of (u, threshold) alone with the same bits on every call: it is the
surface `mcubes` extracts up to vertex numbering and triangle order on unambiguous cells; its treatment of ambiguous faces is this
project's own (solid corners are cut off) and is not pinned against `mcubes`.
"""
import numpy as np
import torch

from . import _lib
from ._util import call, ptr, stream


@torch.no_grad()
def marching_cubes(u, threshold):
    """u [Rx, Ry, Rz] f32 on the device, solid where u >= threshold -> (vertices [V, 3] f32 in INDEX coordinates, as mcubes returns
    them; triangles [T, 3] int32), both on the device.  Two launches to count and scan, ONE host synchronisation to read (V, T) back
    and size the outputs -- a mesh is not a per-frame product -- then one launch to emit."""
    if u.dim() != 3 or u.dtype != torch.float32 or not u.is_cuda:
        raise RuntimeError("u must be a float32 [Rx, Ry, Rz] CUDA tensor")
    u = u.contiguous()
    dev = u.device
    Rx, Ry, Rz = u.shape
    if min(Rx, Ry, Rz) < 2:          # no cells
        return torch.empty(0, 3, dtype=torch.float32, device=dev), torch.empty(0, 3, dtype=torch.int32, device=dev)
    if 3 * Rx * Ry * Rz >= 2 ** 31:
        raise _lib.LzError("marching_cubes: the lattice must have 3 Rx Ry Rz < 2^31")
    thr = float(threshold)
    nbytes = _lib.load().lz_mc_workspace(Rx, Ry, Rz)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    totals = torch.empty(2, dtype=torch.int32, device=dev)     # two uint32 words; T < 2^31 * 5 / 3 is read back unsigned
    call("lz_mc_count", ptr(u), Rx, Ry, Rz, thr, ptr(ws), ptr(totals), stream())
    V, T = [int(v) & 0xFFFFFFFF for v in totals.tolist()]       # the one host synchronisation
    vertices = torch.empty(V, 3, dtype=torch.float32, device=dev)
    triangles = torch.empty(T, 3, dtype=torch.int32, device=dev)
    if V or T:
        call("lz_mc_emit", ptr(u), Rx, Ry, Rz, thr, ptr(ws), V, T, ptr(vertices) if V else None, ptr(triangles) if T else None, stream())
    return vertices, triangles


def to_world(vertices, bound_min, bound_max, resolution):
    """utils.py:377, `v / (resolution - 1) * (bmax - bmin) + bmin`, evaluated in float64 from the f32 operands and rounded once to f32"""
    dev = vertices.device
    lo = torch.as_tensor(bound_min, dtype=torch.float32).to(dev).double().reshape(1, 3)
    hi = torch.as_tensor(bound_max, dtype=torch.float32).to(dev).double().reshape(1, 3)
    return (vertices.double() / (float(resolution) - 1.0) * (hi - lo) + lo).float()


@torch.no_grad()
def extract_geometry(head, enc_a, eye, bound_min, bound_max, resolution, threshold):
    """`extract_geometry` (utils.py:366-378) with `query_func` = the head's density: `occupancy.density_field` (extract_fields), then
    `marching_cubes`, then the affine of line 377 (`to_world`).  Returns DEVICE tensors, vertices [V, 3] float32 in world coordinates
    and triangles [T, 3] int32: the reference returns numpy arrays with float64 vertices -- the only dtype difference; here the affine
    is evaluated in float64 and rounded once."""
    from .occupancy import density_field
    u = density_field(head, enc_a, eye, bound_min, bound_max, resolution)
    vertices, triangles = marching_cubes(u, threshold)
    return to_world(vertices, bound_min, bound_max, resolution), triangles


def save_mesh(path, vertices, triangles):
    """Binary little-endian PLY: `element vertex V` with float x y z, `element face T` with `property list uchar int vertex_indices`
    -- the layout of `trimesh.Trimesh(vertices, triangles, process=False).export(path)` for a .ply path (TrainerUtil.py:462-463), as far
    as it can be stated without trimesh (not pinned).  vertices / triangles: tensors (any device) or arrays."""
    v = np.ascontiguousarray(torch.as_tensor(vertices).detach().cpu().numpy(), dtype="<f4").reshape(-1, 3)
    t = np.ascontiguousarray(torch.as_tensor(triangles).detach().cpu().numpy(), dtype="<i4").reshape(-1, 3)
    header = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
              "element face %d\nproperty list uchar int vertex_indices\nend_header\n" % (len(v), len(t)))
    faces = np.empty(len(t), dtype=[("n", "u1"), ("v", "<i4", (3,))])
    faces["n"] = 3
    faces["v"] = t
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(v.tobytes())
        f.write(faces.tobytes())
