// lz_ngp_chain.h -- the f32 cfg2 network of one pass of 16-sample slices as device functions, shared by the inference kernel
// (lz_ngp.hip: lz_k_ngp_head) and the recomputing backward (lz_ngp_train.hip: lz_k_ngp_head_backward).  Both read the same fragments in
// the same k order, so the backward's recomputed sigma / rgb are the forward's bits.
//
// Shape: v_mfma_f32_16x16x4_f32, lane l = (s = l & 15: sample of the slice, q = l >> 4).  D register rr of tile ft holds output
// 16 ft + 4 q + rr of sample s, and every hidden layer consumes the previous accumulator tile in place ("chained" k order).
#ifndef LZ_NGP_CHAIN_H
#define LZ_NGP_CHAIN_H
#include "lz_common.h"
#include "lzzx_detmath.h"
#include "lzzx_sh_eval.h"
#include "lz_head_layers.h"
#include <hip/hip_fp16.h>

// fragment (ks, ft) of a layer: 64 floats, lane l = W[16 ft + (l & 15)][k(ks, l >> 4)]
#define LZN_S1 0       // 32 -> 64: 8 k-steps x 4 tiles
#define LZN_S2 32      // 64 -> 16: 16 x 1
#define LZN_C1 48      // 32 slots (SH 16 | sigma_net output 16, slot of its row 0 weighted 0) -> 64: 8 x 4
#define LZN_C2 80      // 64 -> 3 (one tile, rows 3..15 zero): 16 x 1
static_assert(LZN_C2 + 16 == LZ_NGP_FRAGS, "fragment count mismatch with the header");

// the inputs of a pass of T slices: features as the B operands of sigma_net.0 (levels q, q + 4, q + 8, q + 12 of sample s, both
// channels), the direction
template <int T>
struct LznIn {
    uint32_t row[T];
    bool valid[T];
    float b1[T][8], dx[T], dy[T], dz[T];
};

// FEAT: 0 = row-major f32 [n_rows, 32]; 1 = tiled f32 (lz_grid_encode_forward_tiled); 2 = tiled f16.  n_rows: rows of feats / dirs (the
// encoder's B: it fixes the packing of the last, partial tile); rows: rows in use (<= n_rows)
template <int FEAT, int T>
__device__ __forceinline__ void lzn_load(const void* feats, const float* dirs, uint32_t n_rows, uint32_t rows, int s, int q, uint32_t slice0,
                                         LznIn<T>& I) {
    constexpr uint32_t Tn = LZ_GRID_TILE_ROWS;
#pragma unroll
    for (int u = 0; u < T; u++) {
        I.row[u] = (slice0 + u) * 16u + (uint32_t)s;
        I.valid[u] = I.row[u] < rows;
        const uint32_t r = I.valid[u] ? I.row[u] : rows - 1u;
        if constexpr (FEAT == 0) {
            const float2* f = reinterpret_cast<const float2*>(reinterpret_cast<const float*>(feats) + (size_t)r * 32);
#pragma unroll
            for (int i = 0; i < 4; i++) { const float2 v = f[q + 4 * i]; I.b1[u][2 * i] = v.x; I.b1[u][2 * i + 1] = v.y; }
        } else {
            const uint32_t tile = r / Tn, t = r - tile * Tn, b0 = tile * Tn, n = (n_rows - b0 < Tn) ? n_rows - b0 : Tn;
            if constexpr (FEAT == 1) {
                const float2* f = reinterpret_cast<const float2*>(reinterpret_cast<const float*>(feats) + (size_t)b0 * 32);
#pragma unroll
                for (int i = 0; i < 4; i++) { const float2 v = f[(size_t)(q + 4 * i) * n + t]; I.b1[u][2 * i] = v.x; I.b1[u][2 * i + 1] = v.y; }
            } else {
                const __half2* f = reinterpret_cast<const __half2*>(reinterpret_cast<const __half*>(feats) + (size_t)b0 * 32);
#pragma unroll
                for (int i = 0; i < 4; i++) { const float2 v = __half22float2(f[(size_t)(q + 4 * i) * n + t]); I.b1[u][2 * i] = v.x; I.b1[u][2 * i + 1] = v.y; }
            }
        }
        I.dx[u] = dirs[(size_t)r * 3]; I.dy[u] = dirs[(size_t)r * 3 + 1]; I.dz[u] = dirs[(size_t)r * 3 + 2];
    }
}

// what the chain leaves per slice u (lane (s, q)):
//   h1[u][4 ft + rr]  sigma_net.0 after ReLU, output 16 ft + 4 q + rr     h[u][rr]   sigma_net.1, output 4 q + rr (row 0 -> sigma)
//   shq[u][ks]        SH component 4 ks + q                               c1[u][..]  colour_net.0 after ReLU (as h1)
//   c[u][rr]          colour_net.1 pre-activation, channel rr on q == 0
template <int T>
struct LznOut {
    float h1[T][16];
    lz_f4 h[T];
    float shq[T][4];
    float c1[T][16];
    lz_f4 c[T];
};

// T slices per pass: every A fragment is read from LDS once and feeds T MFMAs, and the T accumulation chains interleave (the 16-deep
// chains of the two 64 -> N layers are dependent MFMAs otherwise); wl: the LZ_NGP_FRAGS fragments
// The chain in two halves, so that a caller whose SH components are a per-ray constant (lz_ngp_frame.hip keeps them in its ray slots)
// supplies o.shq itself between them; lzn_chain below is both with lz_sh_eval of the sample's direction in between.
template <int T>
__device__ __forceinline__ void lzn_chain_sigma(const float* __restrict__ wl, int lane, const float (&b1)[T][8], LznOut<T>& o) {
    // ---------------- sigma_net: 32 -> 64 (ReLU) -> 16 ----------------
    {
        lz_f4 acc[T][4];
#pragma unroll
        for (int u = 0; u < T; u++)
#pragma unroll
            for (int ft = 0; ft < 4; ft++) acc[u][ft] = lz_f4{0, 0, 0, 0};
#pragma unroll
        for (int ks = 0; ks < 8; ks++)
#pragma unroll
            for (int ft = 0; ft < 4; ft++) {
                const float a = wl[(LZN_S1 + ks * 4 + ft) * 64 + lane];
#pragma unroll
                for (int u = 0; u < T; u++) acc[u][ft] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b1[u][ks], acc[u][ft], 0, 0, 0);
            }
#pragma unroll
        for (int u = 0; u < T; u++)
#pragma unroll
            for (int ft = 0; ft < 4; ft++)
#pragma unroll
                for (int rr = 0; rr < 4; rr++) o.h1[u][4 * ft + rr] = lz_relu(acc[u][ft][rr]);
    }
#pragma unroll
    for (int u = 0; u < T; u++) o.h[u] = lz_f4{0, 0, 0, 0};
#pragma unroll
    for (int ks = 0; ks < 16; ks++) {
        const float a = wl[(LZN_S2 + ks) * 64 + lane];
#pragma unroll
        for (int u = 0; u < T; u++) o.h[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, o.h1[u][ks], o.h[u], 0, 0, 0);
    }
}
// colour_net on o.shq (this lane's SH components 4 ks + q) and sigma_net's o.h
template <int T>
__device__ __forceinline__ void lzn_chain_colour(const float* __restrict__ wl, int lane, LznOut<T>& o) {
    // ---------------- colour_net: [SH(4) of the direction | geometry] -> 64 (ReLU) -> 3 ----------------
    {
        lz_f4 acc[T][4];
#pragma unroll
        for (int u = 0; u < T; u++)
#pragma unroll
            for (int ft = 0; ft < 4; ft++) acc[u][ft] = lz_f4{0, 0, 0, 0};
#pragma unroll
        for (int ks = 0; ks < 8; ks++)
#pragma unroll
            for (int ft = 0; ft < 4; ft++) {
                const float a = wl[(LZN_C1 + ks * 4 + ft) * 64 + lane];
#pragma unroll
                for (int u = 0; u < T; u++)      // SH component 4 ks + q, then sigma_net output 4 q + (ks - 4)
                    acc[u][ft] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, ks < 4 ? o.shq[u][ks] : o.h[u][ks - 4], acc[u][ft], 0, 0, 0);
            }
#pragma unroll
        for (int u = 0; u < T; u++)
#pragma unroll
            for (int ft = 0; ft < 4; ft++)
#pragma unroll
                for (int rr = 0; rr < 4; rr++) o.c1[u][4 * ft + rr] = lz_relu(acc[u][ft][rr]);
    }
#pragma unroll
    for (int u = 0; u < T; u++) o.c[u] = lz_f4{0, 0, 0, 0};
#pragma unroll
    for (int ks = 0; ks < 16; ks++) {
        const float a = wl[(LZN_C2 + ks) * 64 + lane];
#pragma unroll
        for (int u = 0; u < T; u++) o.c[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, o.c1[u][ks], o.c[u], 0, 0, 0);
    }
}
template <int T>
__device__ __forceinline__ void lzn_chain(const float* __restrict__ wl, int lane, int q, const LznIn<T>& in, LznOut<T>& o) {
    lzn_chain_sigma<T>(wl, lane, in.b1, o);
#pragma unroll
    for (int u = 0; u < T; u++) {
        float sh[16];
        lz_sh_eval(in.dx[u], in.dy[u], in.dz[u], 4, sh, nullptr, nullptr, nullptr);
#pragma unroll
        for (int ks = 0; ks < 4; ks++) o.shq[u][ks] = q == 0 ? sh[4 * ks] : (q == 1 ? sh[4 * ks + 1] : (q == 2 ? sh[4 * ks + 2] : sh[4 * ks + 3]));
    }
    lzn_chain_colour<T>(wl, lane, o);
}
#endif
