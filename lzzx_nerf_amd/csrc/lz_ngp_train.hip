// lz_ngp_train.hip -- training pass of the BASELINE cfg2 hash-grid NeRF (lzzx_nerf_amd/ngp_train.py: FusedHashgridTrainNeRF): the backward
// of sigma_net / color_net (network.py:73-94 under autograd: two bias-free MLPs, cat, exp, sigmoid) behind the level-major gather.
//
// Forward: lz_ngp_head_forward itself (tiled f32 features).  Backward: nothing is recorded.  Each wave recomputes the forward of a
// 16-sample slice with lz_ngp_chain.h (the inference kernel's code: same fragments, same k order, so sigma / rgb are its bits), applies
// torch's activation backward formulas (ExpBackward: g * result; SigmoidBackward: g * (1 - y) * y) and runs the data gradients back
// through the layers on the same v_mfma_f32_16x16x4_f32 shape with TRANSPOSED weight fragments (D[input, sample] = W^T . G), each layer
// consuming the previous D tile in place (chained k order over the forward layer's outputs):
//     colour_net.1^T  1 k-step (k = channel q) x 4 tiles   ->  ReLU mask of colour_net.0's output
//     colour_net.0^T  16 x 1: the geometry columns only (slot j = sigma_net output j, slot 0 zero; the SH columns need no gradient)
//     sigma_net.1^T   4 x 4 (output 0 fed from sigma alone)  ->  ReLU mask  ->  sigma_net.0^T 16 x 2  ->  d feats, [L, B, C]
// 68 MFMAs, plus the 96 of the recomputed forward.  The table gradient is not formed here: d feats is grad_layout 0 of
// lz_grid_encode_backward, whose scatter uses float atomics like the reference (gridencoder.cu:226-313).
//
// Weight gradients take samples as the MFMA's k dimension (lz_train_wgrad.h, shared with lz_torso_train.hip): per layer the slice's
// output gradients and inputs are staged in the wave's LDS and accumulated over the wave's slices into 24 16 x 16 tiles (96 registers);
// the fold and the combine are the header's: no float atomics, the same bits on every call, and every weight gradient is linear in the
// upstream gradient (a power-of-two scale passes through exactly).
#include "lz_ngp_chain.h"
#include "lz_train_wgrad.h"

#ifndef LZNB_WG_PER_CU
#define LZNB_WG_PER_CU 2u   // 66 KB of LDS per workgroup: two per CU
#endif
#define LZNB_WG 256
#define LZNB_WAVES (LZNB_WG / 64)
// backward fragments, lane l of fragment (ks, ft) = W[k(ks, l >> 4)][16 ft + (l & 15)] (k over the forward layer's outputs)
#define LZNB_C2 0      // colour_net.1^T: k = channel (l >> 4) < 3; 4 tiles of colour_net.0's outputs
#define LZNB_C1 4      // colour_net.0^T geometry columns: 16 k-steps (64 outputs, chained) x 1 tile of slots
#define LZNB_S2 20     // sigma_net.1^T: 4 k-steps (k = 4 q + ks) x 4 tiles of sigma_net.0's outputs
#define LZNB_S1 36     // sigma_net.0^T: 16 k-steps x 2 tiles of features
#define LZNB_FRAGS 68
// weight-gradient tiles (fo: 16-row block of a layer's outputs, fk: 16-column block of its per-sample inputs)
//   0-3 colour_net.1 (1 x 4)  4-11 colour_net.0 (4 x 2, inputs [SH 16 | sigma_net outputs 16])  12-15 sigma_net.1 (1 x 4)  16-23 sigma_net.0 (4 x 2)
#define LZNB_TILES 24
#define LZNB_ELEMS (LZNB_TILES * 256)
#define LZNB_ROWS 96                       // staging rows per wave: region A = rows 0-63, region B = rows 64-95
static_assert(LZNB_WAVES * LZNB_ROWS * 16 == LZNB_ELEMS, "the wave fold reuses the staging rows");

struct LzNgpBwdK {
    const float* packed;
    const float *ws0, *ws1, *wc0, *wc1;   // sigma_net.0 [64, 32], sigma_net.1 [16, 64], color_net.0 [64, 31], color_net.1 [3, 64]
    const float* feats;                    // tiled f32
    const float* dirs;
    const int* count;
    const float* g_sigma;
    const float* g_rgb;
    float* d_feats;                        // [L, rows, C]
    float* partials;
    uint32_t rows;
};

__global__ void __launch_bounds__(LZNB_WG, 2) lz_k_ngp_head_backward(LzNgpBwdK P) {
    __shared__ __align__(16) float wl[LZ_NGP_FRAGS * 64];
    __shared__ __align__(16) float wb[LZNB_FRAGS * 64];
    __shared__ __align__(16) float stage[LZNB_ELEMS];
    {
        const float4* src = reinterpret_cast<const float4*>(P.packed);
        float4* dst = reinterpret_cast<float4*>(wl);
        for (uint32_t i = threadIdx.x; i < LZ_NGP_FRAGS * 16; i += LZNB_WG) dst[i] = src[i];
        for (uint32_t i = threadIdx.x; i < LZNB_FRAGS * 64; i += LZNB_WG) {   // transposed fragments, zero outside the matrices
            const int fr = (int)(i >> 6), q = (int)(i >> 4) & 3, m = (int)i & 15;
            float v;
            if (fr < LZNB_C1) {                         // colour_net.1 [3, 64]: row q, column 16 ft + m
                v = q < 3 ? P.wc1[q * 64 + 16 * fr + m] : 0.0f;
            } else if (fr < LZNB_S2) {                  // colour_net.0 [64, 31]: row k(ks, q), column 16 + slot - 1
                const int ks = fr - LZNB_C1, o = 16 * (ks >> 2) + 4 * q + (ks & 3);
                v = m >= 1 ? P.wc0[o * 31 + 15 + m] : 0.0f;
            } else if (fr < LZNB_S1) {                  // sigma_net.1 [16, 64]: row 4 q + ks, column 16 ft + m
                const int ks = (fr - LZNB_S2) >> 2, ft = (fr - LZNB_S2) & 3;
                v = P.ws1[(4 * q + ks) * 64 + 16 * ft + m];
            } else {                                    // sigma_net.0 [64, 32]: row k(ks, q), column 16 ft + m
                const int ks = (fr - LZNB_S1) >> 1, ft = (fr - LZNB_S1) & 1, o = 16 * (ks >> 2) + 4 * q + (ks & 3);
                v = P.ws0[o * 32 + 16 * ft + m];
            }
            wb[i] = v;
        }
    }
    __syncthreads();
    uint32_t rows = P.rows;
    if (P.count) {
        const int c = *P.count;
        rows = c < 0 ? 0u : ((uint32_t)c < rows ? (uint32_t)c : rows);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, s = lane & 15, q = lane >> 4;
    float* const stA = stage + wave * (LZNB_ROWS * 16);
    float* const stB = stA + 64 * 16;
    lz_f4 gw[LZNB_TILES];
#pragma unroll
    for (int t = 0; t < LZNB_TILES; t++) gw[t] = lz_f4{0, 0, 0, 0};
    const uint32_t n_slices = (rows + 15u) / 16u, stride = gridDim.x * LZNB_WAVES;
    for (uint32_t slice = blockIdx.x * LZNB_WAVES + (uint32_t)wave; slice < n_slices; slice += stride) {
        LznIn<1> in;
        lzn_load<1, 1>(P.feats, P.dirs, P.rows, rows, s, q, slice, in);
        LznOut<1> f;
        lzn_chain<1>(wl, lane, q, in, f);
        const uint32_t row = in.row[0];
        const bool valid = in.valid[0];
        // ---- output gradients: lane (s, q) owns colour channel q < 3 of sample s; q == 0 also sigma ----
        const float cs0 = __shfl(f.c[0][0], s, 64), cs1 = __shfl(f.c[0][1], s, 64), cs2 = __shfl(f.c[0][2], s, 64);
        const float y = lz_sigmoidf(q == 0 ? cs0 : (q == 1 ? cs1 : cs2));
        const float gr = (valid && q < 3 && P.g_rgb) ? P.g_rgb[(size_t)row * 3 + q] : 0.0f;
        const float gc = q < 3 ? gr * (1.0f - y) * y : 0.0f;                  // SigmoidBackward
        const float gs = (valid && q == 0 && P.g_sigma) ? P.g_sigma[row] : 0.0f;
        const float gh0 = q == 0 ? gs * lz_expf(f.h[0][0]) : 0.0f;             // ExpBackward (the result)
        // ---- colour_net.1^T -> ReLU mask ----
        float gc1[16];
        {
            lz_f4 acc[4];
#pragma unroll
            for (int ft = 0; ft < 4; ft++) acc[ft] = __builtin_amdgcn_mfma_f32_16x16x4f32(wb[(LZNB_C2 + ft) * 64 + lane], gc, lz_f4{0, 0, 0, 0}, 0, 0, 0);
#pragma unroll
            for (int ft = 0; ft < 4; ft++)
#pragma unroll
                for (int rr = 0; rr < 4; rr++) gc1[4 * ft + rr] = f.c1[0][4 * ft + rr] > 0.0f ? acc[ft][rr] : 0.0f;
        }
        // weight gradient of colour_net.1: G = gc (rows 0..3 of region B), inputs c1 (region A)
        stB[q * 16 + s] = gc;
        lz_wg_stage_d<4>(stA, s, q, f.c1[0]);
        lz_wave_lds_sync();
        lz_wg_tiles<1, 4>(gw + 0, stB, stA, lane);
        lz_wave_lds_sync();
        // ---- colour_net.0^T (geometry slots) -> sigma_net outputs 1..15; output 0 from sigma ----
        float gh[4];
        {
            lz_f4 acc = lz_f4{0, 0, 0, 0};
#pragma unroll
            for (int ks = 0; ks < 16; ks++) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wb[(LZNB_C1 + ks) * 64 + lane], gc1[ks], acc, 0, 0, 0);
#pragma unroll
            for (int rr = 0; rr < 4; rr++) gh[rr] = acc[rr];
            if (q == 0) gh[0] = gh0;
        }
        // weight gradient of colour_net.0: G = gc1 (region A), inputs [SH 16 | sigma_net outputs 16] (region B)
        lz_wg_stage_d<4>(stA, s, q, gc1);
#pragma unroll
        for (int ks = 0; ks < 4; ks++) stB[(4 * ks + q) * 16 + s] = f.shq[0][ks];
#pragma unroll
        for (int rr = 0; rr < 4; rr++) stB[(16 + 4 * q + rr) * 16 + s] = f.h[0][rr];
        lz_wave_lds_sync();
        lz_wg_tiles<4, 2>(gw + 4, stA, stB, lane);
        lz_wave_lds_sync();
        // ---- sigma_net.1^T -> ReLU mask ----
        float gh1[16];
        {
            lz_f4 acc[4];
#pragma unroll
            for (int ft = 0; ft < 4; ft++) acc[ft] = lz_f4{0, 0, 0, 0};
#pragma unroll
            for (int ks = 0; ks < 4; ks++)
#pragma unroll
                for (int ft = 0; ft < 4; ft++) acc[ft] = __builtin_amdgcn_mfma_f32_16x16x4f32(wb[(LZNB_S2 + ks * 4 + ft) * 64 + lane], gh[ks], acc[ft], 0, 0, 0);
#pragma unroll
            for (int ft = 0; ft < 4; ft++)
#pragma unroll
                for (int rr = 0; rr < 4; rr++) gh1[4 * ft + rr] = f.h1[0][4 * ft + rr] > 0.0f ? acc[ft][rr] : 0.0f;
        }
        // weight gradient of sigma_net.1: G = gh (rows 0..15 of region B), inputs h1 (region A)
        lz_wg_stage_d<1>(stB, s, q, gh);
        lz_wg_stage_d<4>(stA, s, q, f.h1[0]);
        lz_wave_lds_sync();
        lz_wg_tiles<1, 4>(gw + 12, stB, stA, lane);
        lz_wave_lds_sync();
        // ---- sigma_net.0^T -> d feats: feature 16 ft + 4 q + rr = level 8 ft + 2 q + (rr >> 1), channel rr & 1 ----
        {
            lz_f4 acc[2] = {lz_f4{0, 0, 0, 0}, lz_f4{0, 0, 0, 0}};
#pragma unroll
            for (int ks = 0; ks < 16; ks++)
#pragma unroll
                for (int ft = 0; ft < 2; ft++) acc[ft] = __builtin_amdgcn_mfma_f32_16x16x4f32(wb[(LZNB_S1 + ks * 2 + ft) * 64 + lane], gh1[ks], acc[ft], 0, 0, 0);
            if (valid) {
#pragma unroll
                for (int ft = 0; ft < 2; ft++)
#pragma unroll
                    for (int h = 0; h < 2; h++) {
                        const uint32_t level = 8 * ft + 2 * q + h;
                        *reinterpret_cast<float2*>(P.d_feats + ((size_t)level * P.rows + row) * 2) = make_float2(acc[ft][2 * h], acc[ft][2 * h + 1]);
                    }
            }
        }
        // weight gradient of sigma_net.0: G = gh1 (region A), inputs the features (region B; b1[ks] = feature 2 (q + 4 (ks >> 1)) + (ks & 1))
        lz_wg_stage_d<4>(stA, s, q, gh1);
#pragma unroll
        for (int ks = 0; ks < 8; ks++) stB[(2 * (q + 4 * (ks >> 1)) + (ks & 1)) * 16 + s] = in.b1[0][ks];
        lz_wave_lds_sync();
        lz_wg_tiles<4, 2>(gw + 16, stA, stB, lane);
        lz_wave_lds_sync();
    }
    // ---- the waves folded in wave order into the staging rows, then one partial per workgroup ----
    lz_wg_fold_and_store<LZNB_TILES, LZNB_WAVES>(gw, stage, P.partials + (size_t)blockIdx.x * LZNB_ELEMS, lane, wave);
}

// ---- combine: the workgroup partials in workgroup order (lz_wg_combine) -> the four weight gradients --------------------------------
struct LzNgpGradOut {
    float *gs0, *gs1, *gc0, *gc1;
};

__global__ void __launch_bounds__(256) lz_k_ngp_head_grad_combine(const float* __restrict__ partials, uint32_t n_groups, LzNgpGradOut G) {
    __shared__ float red[4][64];
    const int e = blockIdx.x * 64 + (threadIdx.x & 63);
    const float v = lz_wg_combine<LZNB_ELEMS>(partials, n_groups, e, red);
    if (threadIdx.x >= 64) return;
    const auto [t, row, col] = lz_wg_elem(e);
    if (t < 4) {                // colour_net.1 [3, 64]
        if (row < 3) G.gc1[row * 64 + 16 * t + col] = v;
    } else if (t < 12) {        // colour_net.0 [64, 31]: input k < 16 = SH column k; k = 16 + j = sigma_net output j -> column 15 + j (j >= 1)
        const int o = 16 * ((t - 4) >> 1) + row, k = 16 * ((t - 4) & 1) + col;
        if (k != 16) G.gc0[o * 31 + (k < 16 ? k : k - 1)] = v;
    } else if (t < 16) {        // sigma_net.1 [16, 64]
        G.gs1[row * 64 + 16 * (t - 12) + col] = v;
    } else {                    // sigma_net.0 [64, 32]
        G.gs0[(16 * ((t - 16) >> 1) + row) * 32 + 16 * ((t - 16) & 1) + col] = v;
    }
}

// ---- entry points ----------------------------------------------------------------------------------------------------------------
extern "C" size_t lz_ngp_train_workspace(void) { return lz_wg_workspace_bytes(LZNB_TILES); }

extern "C" int lz_ngp_head_backward(const float* packed, const float* sigma_w0, const float* sigma_w1, const float* color_w0, const float* color_w1,
                                    const float* feats, const float* dirs, uint32_t rows, const int32_t* count, const float* g_sigma, const float* g_rgb,
                                    float* d_feats, float* g_sigma_w0, float* g_sigma_w1, float* g_color_w0, float* g_color_w1, void* workspace,
                                    lz_stream_t stream) {
    if (rows == 0) return LZ_OK;
    LZ_REQUIRE(packed && sigma_w0 && sigma_w1 && color_w0 && color_w1 && feats && dirs && d_feats, LZ_ERR_BAD_ARGUMENT, "ngp_head_backward: null tensor");
    LZ_REQUIRE(g_sigma_w0 && g_sigma_w1 && g_color_w0 && g_color_w1 && workspace, LZ_ERR_BAD_ARGUMENT, "ngp_head_backward: null gradient or workspace");
    LzNgpBwdK K{packed, sigma_w0, sigma_w1, color_w0, color_w1, feats, dirs, count, g_sigma, g_rgb, d_feats, static_cast<float*>(workspace), rows};
    // as lz_ngp_head_forward: as many workgroups as the chip holds at a time (each stages 42 KB of fragments once), each looping over its
    // share of the slices, fewer when there are not four slices per wave
    const uint32_t grid = lz_wg_grid(rows, LZNB_WAVES, LZNB_WG_PER_CU);
    hipStream_t st = lz_st(stream);
    hipLaunchKernelGGL(lz_k_ngp_head_backward, dim3(grid), dim3(LZNB_WG), 0, st, K);
    LZ_CHECK_LAUNCH("ngp_head_backward");
    LzNgpGradOut G{g_sigma_w0, g_sigma_w1, g_color_w0, g_color_w1};
    hipLaunchKernelGGL(lz_k_ngp_head_grad_combine, dim3(LZNB_ELEMS / 64), dim3(256), 0, st, static_cast<const float*>(workspace), grid, G);
    LZ_CHECK_LAUNCH("ngp_head_grad_combine");
    return LZ_OK;
}
