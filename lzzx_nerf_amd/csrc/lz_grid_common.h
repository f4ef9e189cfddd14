// lz_grid_common.h -- what every grid-encoder kernel shares: the per-level constants, one level record, one cell, one corner.
// Used by lz_grid.hip (the gridencoder operator) and lz_triplane_enc.hip (the three-plane encoder), so that both produce the same bits.
#ifndef LZ_GRID_COMMON_H
#define LZ_GRID_COMMON_H
#include "lz_common.h"
#include "lzzx_detmath.h"
#include <math.h>

#define LZ_MAX_LEVELS 32

struct LzGridLevels {
    float scale[LZ_MAX_LEVELS];
    uint32_t res[LZ_MAX_LEVELS];
};

static int lz_fill_levels(LzGridLevels& lv, uint32_t L, float S, uint32_t H) {
    if (L > LZ_MAX_LEVELS) return -1;
    for (uint32_t l = 0; l < L; l++) {
        // gridencoder.cu:125-126, evaluated on the host with the same libm call the CPU checker uses
        const float sc = exp2f((float)l * S) * (float)H - 1.0f;
        lv.scale[l] = sc;
        lv.res[l] = (uint32_t)ceilf(sc) + 1u;
    }
    return 0;
}

template <uint32_t D>
__device__ __forceinline__ uint32_t lz_grid_index(uint32_t C, uint32_t gridtype, bool align_corners, uint32_t hashmap_size,
                                                  uint32_t resolution, const uint32_t (&pos_grid)[D]) {
    constexpr uint32_t primes[7] = {1u, 2654435761u, 805459861u, 3674653429u, 2097192037u, 1434869437u, 2165219737u};
    uint32_t stride = 1, index = 0;
#pragma unroll
    for (uint32_t d = 0; d < D; d++) {
        if (stride <= hashmap_size) {
            index += pos_grid[d] * stride;
            stride *= align_corners ? resolution : (resolution + 1);
        }
    }
    if (gridtype == 0 && stride > hashmap_size) {
        uint32_t h = 0;
#pragma unroll
        for (uint32_t d = 0; d < D; d++) h ^= pos_grid[d] * primes[d];
        index = h;
    }
    return (index % hashmap_size) * C;
}

// ---- the arithmetic every kernel below shares: one level record, one cell, one corner ------------------------------
// A level's mode says how a corner's index reaches the table, exactly as get_grid_index does it:
//   0  dense: every stride fitted, so index < size and the modulo is the identity;
//   1  hashed with a power-of-two table: the modulo is a mask;
//   2  anything else: the generic (index % size) of lz_grid_index.
// Two exclusions send a level to mode 2.  Very fine levels: the reference's uint32 stride wraps, and only the generic path keeps its
// exact (index % size).  align_corners: side = res, so the +1 corner of x = 1 lands one stride past the level (gridencoder.cu:71
// wraps it), and no level is dense.
template <uint32_t D>
__device__ __forceinline__ uint32_t lz_grid_level_mode(uint32_t hs, uint32_t res, uint32_t gridtype, bool align_corners) {
    // replay the stride loop of get_grid_index (gridencoder.cu:56-69)
    uint32_t stride = 1;
    uint64_t stride_exact = 1;   // the same product without 32-bit wrap-around
    for (uint32_t d = 0; d < D; d++)
        if (stride <= hs) {
            stride *= align_corners ? res : (res + 1);
            stride_exact *= align_corners ? res : (res + 1);
        }
    const bool wrapped = stride_exact != (uint64_t)stride;
    const bool hashed = gridtype == 0 && stride > hs;
    const bool dense = stride <= hs && !wrapped && !align_corners;
    const bool pow2 = (hs & (hs - 1u)) == 0u;
    return dense ? 0u : ((hashed && pow2 && !wrapped) ? 1u : 2u);
}

struct LzGridLevel {
    uint32_t off0, hs, res;   // first entry of the level, its size (entries), its resolution
    float scale;
    uint32_t mode;            // lz_grid_level_mode
};

// CLASSIFY = false puts every level in mode 2, which is exact for all of them: the one-lane-per-(sample, level) kernels that serve the
// other layouts, dy_dx and the plain scatter keep a single index path (and their code size).
template <uint32_t D, bool CLASSIFY = true>
__device__ __forceinline__ LzGridLevel lz_grid_level(const int* __restrict__ offsets, const LzGridLevels& lv, uint32_t level,
                                                     uint32_t gridtype, bool align_corners) {
    LzGridLevel r;
    r.off0 = (uint32_t)offsets[level];
    r.hs = (uint32_t)offsets[level + 1] - r.off0;
    r.res = lv.res[level];
    r.scale = lv.scale[level];
    r.mode = CLASSIFY ? lz_grid_level_mode<D>(r.hs, r.res, gridtype, align_corners) : 2u;
    return r;
}

// The cell of x in a level: lower corner pg, fraction pos, and whether some x[d] lies outside [0, 1] (a NaN does not).  CLAMP clamps x
// for addressing only, in the kernels that compute every row and write zeros for the out-of-range ones; the others skip those rows
// before they touch the table, so they leave x as it is (which matters for a NaN).
template <uint32_t D> struct LzGridCell {
    uint32_t pg[D];
    float pos[D];
    bool oob;
};
template <uint32_t D, bool CLAMP>
__device__ __forceinline__ LzGridCell<D> lz_grid_cell(const float (&x)[D], float scale, bool align_corners) {
    LzGridCell<D> c;
    c.oob = false;
#pragma unroll
    for (uint32_t d = 0; d < D; d++) {
        if (x[d] < 0 || x[d] > 1) c.oob = true;
        const float xc = CLAMP ? lz_fminf(lz_fmaxf(x[d], 0.0f), 1.0f) : x[d];
        c.pos[d] = lz_fmaf(xc, scale, align_corners ? 0.0f : 0.5f);
        c.pg[d] = (uint32_t)floorf(c.pos[d]);
        c.pos[d] -= (float)c.pg[d];
    }
    return c;
}

// Weight of corner idx (bit d set: the upper corner in dimension d): the product over d in increasing order, starting from w.  The
// forward's dy_dx starts from the level's scale and leaves out the dimension it differentiates (skip).
template <uint32_t D>
__device__ __forceinline__ float lz_grid_weight(const LzGridCell<D>& c, uint32_t idx, float w = 1.0f, uint32_t skip = D) {
#pragma unroll
    for (uint32_t d = 0; d < D; d++) {
        if (d == skip) continue;
        if ((idx & (1u << d)) == 0) w *= 1 - c.pos[d];
        else w *= c.pos[d];
    }
    return w;
}

// Index terms per dimension for the dense (mode 0) and power-of-two hashed (mode 1) levels: term[d][0] belongs to the lower cell
// coordinate pg[d], term[d][1] to pg[d] + 1 -- the lower one plus a constant modulo 2^32, exactly the reference's uint32 arithmetic
// (gridencoder.cu:60-98: index += pos * stride / result ^= pos * prime).  A corner's index is then the sum (dense) or the xor (hashed)
// of D terms: one 32-bit multiply per dimension and sample, spelled out (the compiler found the same common subexpressions in the
// per-corner form: measured, no change in the triplane plane or the cfg2 gather -- neither is bound by the index arithmetic).
// Mode 2 does not use them.
template <uint32_t D>
__device__ __forceinline__ void lz_grid_terms(const LzGridLevel& lvl, const LzGridCell<D>& c, bool align_corners, uint32_t (&term)[D][2]) {
    constexpr uint32_t primes[7] = {1u, 2654435761u, 805459861u, 3674653429u, 2097192037u, 1434869437u, 2165219737u};
    uint32_t stride = 1;
#pragma unroll
    for (uint32_t d = 0; d < D; d++) {
        const uint32_t k = lvl.mode == 1u ? primes[d] : stride;
        term[d][0] = d == 0 ? c.pg[d] : c.pg[d] * k;      // primes[0] == 1 and the first stride is 1
        term[d][1] = term[d][0] + k;
        stride *= align_corners ? lvl.res : (lvl.res + 1);
    }
}
template <uint32_t D>
__device__ __forceinline__ uint32_t lz_grid_corner(const uint32_t (&term)[D][2], uint32_t idx, uint32_t mode, uint32_t hs) {
    uint32_t lin = 0, h = 0;
#pragma unroll
    for (uint32_t d = 0; d < D; d++) {
        const uint32_t t = term[d][(idx >> d) & 1u];
        lin += t;
        h ^= t;
    }
    return mode == 1u ? (h & (hs - 1u)) : lin;
}
// Element offset (index * C) of corner idx in the level's table, the same value in every mode
template <uint32_t D>
__device__ __forceinline__ uint32_t lz_grid_corner_index(const LzGridLevel& lvl, const LzGridCell<D>& c, const uint32_t (&term)[D][2],
                                                         uint32_t idx, uint32_t C, uint32_t gridtype, bool align_corners) {
    if (lvl.mode == 2u) {
        uint32_t pl[D];
#pragma unroll
        for (uint32_t d = 0; d < D; d++) pl[d] = c.pg[d] + ((idx >> d) & 1u);
        return lz_grid_index<D>(C, gridtype, align_corners, lvl.hs, lvl.res, pl);
    }
    return lz_grid_corner<D>(term, idx, lvl.mode, lvl.hs) * C;
}

// lz_grid.hip: launches its lz_k_grid_input_backward<float, D, C> (kernel_input_backward, gridencoder.cu:316-342) for D 2 / 3 and C 1 / 2,
// for the entry of lz_grid_fixed.hip; nothing is launched for other shapes
void lz_grid_input_backward_f32(const float* grad, const float* dy_dx, float* grad_inputs, uint32_t B, uint32_t D, uint32_t C, uint32_t L,
                                bool sample_major, hipStream_t st);
#endif
