// lz_density_cell.h -- THE query point of an occupancy-grid cell (update_extra_state, nerf_triplane/renderer.py:739-751), shared by the
// kernel that writes the points to memory (lz_raymarch.hip: lz_k_density_points) and the one that makes them in registers
// (lz_density.hip: lz_triplane_density_lattice), so that both hand the head the same bits.
#ifndef LZ_DENSITY_CELL_H
#define LZ_DENSITY_CELL_H
#include <math.h>

#include "lz_common.h"

// row n of C * G^3: cascade n / G^3, cell in custom_meshgrid order (x slowest, z fastest); noise [C, G^3, 3] in [0, 1)
__device__ __forceinline__ void lz_density_cell_point(const float* __restrict__ noise, uint32_t n, uint32_t G, float bound, float (&xyz)[3]) {
    const uint32_t G3 = G * G * G;
    const uint32_t cas = n / G3, p = n - cas * G3;
    // custom_meshgrid(xs, ys, zs) flattened: x slowest, z fastest (renderer.py:739-741)
    const uint32_t c[3] = {p / (G * G), (p / G) % G, p % G};
    // python doubles, then narrowed where torch multiplies an f32 tensor by a python scalar (renderer.py:747-751)
    const double bc = fmin((double)(1u << cas), (double)bound);
    const double half = bc / (double)G;
    const float scale = (float)(bc - half), hgs = (float)half;
#pragma unroll
    for (int d = 0; d < 3; d++) {
        float v = (2.0f * (float)c[d]) / (float)(G - 1) - 1.0f;     // 2 * coords.float() / (grid_size - 1) - 1
        v = v * scale;                                              // xyzs * (bound - half_grid_size)
        const float nz = (noise[(size_t)n * 3 + d] * 2.0f - 1.0f) * hgs;   // (rand * 2 - 1) * half_grid_size
        xyz[d] = v + nz;
    }
}
#endif
