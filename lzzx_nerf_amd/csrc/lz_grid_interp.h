// lz_grid_interp.h -- the interpolation of ONE (sample, level) of the grid encoder as device functions: element arithmetic per table
// type, the mapping of a world position to the unit cube, the eight corner offsets of the cell and the weighted sum in the reference's
// corner order.  Used by the level-major pass (lz_grid.hip: lz_k_grid_forward_lmp, which splits the corner LOADS over a lane pair) and
// by the persistent hash-grid frame kernel (lz_ngp_frame.hip, one lane per (sample, level)): both produce a feature from the same source.
#ifndef LZ_GRID_INTERP_H
#define LZ_GRID_INTERP_H
#include "lz_grid_common.h"
#include <hip/hip_fp16.h>

template <typename T> struct LzElem;
template <> struct LzElem<float> {
    static __device__ __forceinline__ float ld(const float* p) { return *p; }
    static __device__ __forceinline__ float acc(float r, float w, float g) { return lz_fmaf(w, g, r); }
    static __device__ __forceinline__ float accd(float r, float w, float gr, float gl) { return lz_fmaf(w, gr - gl, r); }
    static __device__ __forceinline__ float st(float v) { return v; }
};
template <> struct LzElem<__half> {
    static __device__ __forceinline__ float rh(float v) { return __half2float(__float2half_rn(v)); }
    static __device__ __forceinline__ float ld(const __half* p) { return __half2float(*p); }
    // at::Half semantics: the f32 product is rounded to f32 FIRST, then to half.  The opaque asm keeps the compiler from
    // selecting v_fma_mixlo_f16 for cvt(mul(cvt(g), w)), which rounds the exact product once and differs in ~2^-13 of cases.
    static __device__ __forceinline__ float mul32(float a, float b) { float p = a * b; asm("" : "+v"(p)); return p; }
    static __device__ __forceinline__ float sum32(float a, float b) { float p = a + b; asm("" : "+v"(p)); return p; }
    static __device__ __forceinline__ float acc(float r, float w, float g) { return rh(sum32(r, rh(mul32(w, g)))); }
    static __device__ __forceinline__ float accd(float r, float w, float gr, float gl) { return rh(sum32(r, rh(mul32(w, rh(sum32(gr, -gl)))))); }
    static __device__ __forceinline__ __half st(float v) { return __float2half_rn(v); }
};

template <typename T, uint32_t C> struct LzVec {
    T v[C];
};

// bound > 0: x arrives in [-bound, bound] and is mapped like GridEncoder.forward (grid.py:143; lz_map01, lz_common.h); 0: already in [0, 1].
// inv2b = 1.0f / (2.0f * bound): formed once per thread by the caller, outside its loops (unused when bound is 0)
__device__ __forceinline__ float lz_grid_unit(float x, float bound, float inv2b) { return bound > 0.0f ? lz_map01(x, bound, inv2b) : x; }

// element offsets (index * C) of the 2^D corners of `cell` in the level's table, corner idx = bit d set: upper corner in dimension d
template <uint32_t D>
__device__ __forceinline__ void lz_grid_corner_offsets(const LzGridLevel& lvl, const LzGridCell<D>& cell, uint32_t C, uint32_t gridtype,
                                                       bool align_corners, uint32_t (&index)[1u << D]) {
    uint32_t term[D][2];
    lz_grid_terms<D>(lvl, cell, align_corners, term);
#pragma unroll
    for (uint32_t idx = 0; idx < (1u << D); idx++) index[idx] = lz_grid_corner_index<D>(lvl, cell, term, idx, C, gridtype, align_corners);
}

// the level's feature from the 2^D corner values: weights and fma chain in corner order (gridencoder.cu:128-165), zero for a sample
// outside [0, 1] (its cell was clamped for addressing only), rounded to the table's type
template <typename T, uint32_t D, uint32_t C>
__device__ __forceinline__ LzVec<T, C> lz_grid_interp(const LzGridCell<D>& cell, const LzVec<T, C> (&cv)[1u << D]) {
    float res[C];
#pragma unroll
    for (uint32_t ch = 0; ch < C; ch++) res[ch] = 0.0f;
#pragma unroll
    for (uint32_t idx = 0; idx < (1u << D); idx++) {
        const float wc = lz_grid_weight<D>(cell, idx);
#pragma unroll
        for (uint32_t ch = 0; ch < C; ch++) res[ch] = LzElem<T>::acc(res[ch], wc, LzElem<T>::ld(&cv[idx].v[ch]));
    }
    LzVec<T, C> o;
#pragma unroll
    for (uint32_t ch = 0; ch < C; ch++) o.v[ch] = LzElem<T>::st(cell.oob ? 0.0f : res[ch]);
    return o;
}
#endif
