// lz_train_wgrad.h -- the weight-gradient skeleton of the fused training backwards (lz_torso_train.hip, lz_ngp_train.hip): samples as the
// k dimension of v_mfma_f32_16x16x4_f32, reduced without float atomics in one fixed order, so every weight gradient has the same bits on
// every call and is exactly linear in the upstream gradient.
//
// A wave stages a 16-sample slice's output gradients G and layer inputs X in its LDS as [feature][16 samples] rows, reads them back four
// samples per lane as one 16-byte load and accumulates G^T . X over its slices into 16 x 16 tiles (one lz_f4 per tile: register r of lane
// l = D[4 (l >> 4) + r][l & 15]).  The workgroup's waves are folded in wave order, ((w0 + w1) + w2) + w3, each workgroup writes one
// partial image, and the combine kernel adds the partials per tile element: four threads over interleaved quarters of the workgroups,
// each in workgroup order, then ((q0 + q1) + q2) + q3.
// lz_head_gradw.hip's reduce kernel is not built on this: it keeps four sums in flight, (s0 + s1) + (s2 + s3), so sharing would change bits.
#pragma once
#include "lz_common.h"

typedef float lz_f4 __attribute__((ext_vector_type(4)));   // as lz_head_layers.h

#define LZ_WG_MAX_GROUPS 512   // partial images the workspace holds = the most workgroups a backward launches

// a wave's own LDS traffic: stores before, loads after
__device__ __forceinline__ void lz_wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// B-layout registers (register i = feature 4 i + q of sample s) -> staging rows
template <int NREG>
__device__ __forceinline__ void lz_wg_stage_b(float* __restrict__ rows, int lane, const float (&v)[NREG]) {
#pragma unroll
    for (int i = 0; i < NREG; i++) rows[i * 64 + lane] = v[i];   // row 4 i + q, column s: (4 i + q) * 16 + s
}

// D-layout registers (register 4 ft + rr = feature 16 ft + 4 q + rr of sample s) -> staging rows
template <int NT>
__device__ __forceinline__ void lz_wg_stage_d(float* __restrict__ rows, int s, int q, const float* v) {
#pragma unroll
    for (int ft = 0; ft < NT; ft++)
#pragma unroll
        for (int rr = 0; rr < 4; rr++) rows[(16 * ft + 4 * q + rr) * 16 + s] = v[4 * ft + rr];
}

// rows [16 t, 16 t + 16) of a staging block as an MFMA operand with samples as k: lane l -> row 16 t + (l & 15), samples 4 (l >> 4) + 0..3
__device__ __forceinline__ lz_f4 lz_wg_rows(const float* __restrict__ rows, int t, int lane) {
    return *reinterpret_cast<const lz_f4*>(rows + (16 * t + (lane & 15)) * 16 + 4 * (lane >> 4));
}
// the same for a block of n_rows rows: zero past its end
__device__ __forceinline__ lz_f4 lz_wg_rows(const float* __restrict__ rows, int t, int n_rows, int lane) {
    return 16 * t + (lane & 15) < n_rows ? lz_wg_rows(rows, t, lane) : lz_f4{0, 0, 0, 0};
}

// acc[o * OSTRIDE + k] += G^T . X for FO x FK tiles; BOUND: G has g_n rows and X has a_n (else whole 16-row blocks, and no compare)
template <int FO, int FK, int OSTRIDE = FK, bool BOUND = true>
__device__ __forceinline__ void lz_wg_tiles(lz_f4* __restrict__ acc, const float* g_rows, int g_n, const float* a_rows, int a_n, int lane) {
    lz_f4 av[FK];
#pragma unroll
    for (int k = 0; k < FK; k++) av[k] = BOUND ? lz_wg_rows(a_rows, k, a_n, lane) : lz_wg_rows(a_rows, k, lane);
#pragma unroll
    for (int o = 0; o < FO; o++) {
        const lz_f4 gv = BOUND ? lz_wg_rows(g_rows, o, g_n, lane) : lz_wg_rows(g_rows, o, lane);
#pragma unroll
        for (int k = 0; k < FK; k++)
#pragma unroll
            for (int ks = 0; ks < 4; ks++) acc[o * OSTRIDE + k] = __builtin_amdgcn_mfma_f32_16x16x4f32(gv[ks], av[k][ks], acc[o * OSTRIDE + k], 0, 0, 0);
    }
}
template <int FO, int FK>
__device__ __forceinline__ void lz_wg_tiles(lz_f4* __restrict__ acc, const float* g_rows, const float* a_rows, int lane) {
    lz_wg_tiles<FO, FK, FK, false>(acc, g_rows, 0, a_rows, 0, lane);
}

// the workgroup's WAVES waves folded in wave order into stage (TILES * 256 floats of LDS, free to overwrite), then its partial image
template <int TILES, int WAVES>
__device__ __forceinline__ void lz_wg_fold_and_store(const lz_f4 (&gw)[TILES], float* __restrict__ stage, float* __restrict__ out, int lane, int wave) {
    __syncthreads();
#pragma unroll
    for (int w = 0; w < WAVES; w++) {
        if (wave == w) {
#pragma unroll
            for (int t = 0; t < TILES; t++)
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    float* p = stage + t * 256 + r * 64 + lane;
                    *p = w == 0 ? gw[t][r] : *p + gw[t][r];
                }
        }
        __syncthreads();
    }
    for (uint32_t i = threadIdx.x; i < TILES * 64; i += WAVES * 64) reinterpret_cast<float4*>(out)[i] = reinterpret_cast<const float4*>(stage)[i];
}

// tile element e = (tile t, register r, lane l) <-> D[row][col] of tile t
struct LzWgElem { int t, row, col; };
__device__ __forceinline__ int lz_wg_elem(int t, int row, int col) { return t * 256 + (row & 3) * 64 + 16 * (row >> 2) + col; }
__device__ __forceinline__ LzWgElem lz_wg_elem(int e) { return LzWgElem{e >> 8, 4 * ((e & 63) >> 4) + ((e >> 6) & 3), e & 15}; }

// combine kernels (256 threads, 64 elements per block): element e of the n_groups partial images of ELEMS floats, summed as above.
// All threads call it; those of quarter 0 (threadIdx.x < 64) get the sum.
template <int ELEMS>
__device__ __forceinline__ float lz_wg_combine(const float* __restrict__ partials, uint32_t n_groups, int e, float (&red)[4][64]) {
    const int slot = threadIdx.x & 63, part = threadIdx.x >> 6;
    float v = 0.0f;
    for (uint32_t g = part; g < n_groups; g += 4) v += partials[(size_t)g * ELEMS + e];
    red[part][slot] = v;
    __syncthreads();
    return ((red[0][slot] + red[1][slot]) + red[2][slot]) + red[3][slot];
}

// ---- host side: the workspace of a backward with `tiles` tiles; its grid ----
static inline size_t lz_wg_workspace_bytes(int tiles) { return (size_t)LZ_WG_MAX_GROUPS * tiles * 256 * sizeof(float); }
// workgroups of `waves` waves for n samples: four slices per wave before the grid grows, at most what the chip holds at a time
static inline uint32_t lz_wg_grid(uint32_t n, uint32_t waves, uint32_t wg_per_cu) {
    const uint32_t grid = lz_div_up(n, 16 * waves * 4), chip = (uint32_t)lz_cu_count() * wg_per_cu;
    const uint32_t cap = chip > LZ_WG_MAX_GROUPS ? LZ_WG_MAX_GROUPS : chip;
    return grid < 1 ? 1 : (grid > cap ? cap : grid);
}
