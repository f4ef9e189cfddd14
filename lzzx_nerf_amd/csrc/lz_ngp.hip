// lz_ngp.hip -- BASELINE cfg2: a generic hash-grid NeRF ("256 x 256, 128 samples / ray, hash-grid L = 16 F = 2, forward render") on the
// operators of encoding.get_encoder (encoding.py:6-37): hashgrid (D 3, L 16, C 2, T 2^19; gridencoder.cu:75-223) -> sigma MLP 32-64-16,
// SH(4) of the view direction + 15 geometry features -> colour MLP 31-64-3, bias-free Linear + ReLU (network.py:73-94), sigma = exp,
// rgb = sigmoid -- and the reference's inference loop around it (renderer.py:495-548).
//
// MI355X design.  The hash-grid gather wants to run LEVEL-major: with level the slow launch dimension the whole chip reads one or two
// <= 4 MB levels at a time and they stay resident in the 4 MB L2 of every XCD (69 % of the HBM roofline in march order), whereas a kernel
// in which every wave touches all 16 levels at once (a persistent frame kernel like lz_frame.hip) has the whole 49 MB table as its L2
// working set and was measured at 16 %.  So the gather stays the level-major pass of lz_grid.hip and everything else is fused around it:
//     lz_loop_march            state advance + compaction + march of the survivors                    (lz_raymarch.hip)
//     lz_k_grid_forward_lmp    level-major gather, TILED output, rows bounded by the device-side sample count, no untile pass
//     lz_k_ngp_head            per 16-sample slice: B operands straight from the tiles -> sigma MLP -> SH(4) -> colour MLP on
//                              v_mfma_f32_16x16x4_f32 (96 MFMAs), sigma / rgb out -- replaces 4 Linear launches + cat + activations + copies
//     lz_loop_composite_plain  accumulate, kill, count survivors
// four launches per iteration of the reference's loop, enqueued back to back by lz_ngp_loop_run with the loop state in device memory.
//
// The 16 % above is a stand-alone gather.  The WHOLE frame as a persistent kernel was built and measured since (lz_ngp_frame.hip,
// HashgridRenderer(mode = "fused")): with three waves per SIMD, 32 corner loads in flight per lane and the march, the matrix
// chain and the compositing of other waves under the misses, the 256^2 x 128-step frame takes 1.07 ms against this loop's 3.14 under the
// reference's schedule (1, 8) and 1.98 under (8, 8) (f32; f16 head 0.73 against 2.54 / 1.75), and 0.30 against 0.62 ms at max_steps 16.
// The loop wins only on a 64^2 tile with the f16 head under the fat schedule (0.48 against 0.59 ms).  It stays the default mode.
//
// Arithmetic: every Linear is an fma chain in MFMA k order (oracle/ngp.py spells the order per layer); the first layer's k order follows
// the tiled layout (lane q of a sample reads levels q, q + 4, q + 8, q + 12, both channels: one 8-byte load each), the hidden layers
// consume the previous accumulator tile in place ("chained" order, as lz_head.hip).
#include "lz_ngp_chain.h"       // fragment layout, the feature load and the f32 chain of lz_k_ngp_head (shared with lz_ngp_train.hip)
#include "lz_ngp16_chain.h"     // lz_k_ngp_head16: the f16 chain on v_mfma_f32_32x32x16_f16 (shared with lz_ngp_frame.hip)
#include <hip/hip_fp16.h>

#ifndef LZN_WG_PER_CU
#define LZN_WG_PER_CU 3u
#endif
#ifndef LZN_T
#define LZN_T 1     // 16-sample slices a wave takes through the head together (2: every fragment read feeds two MFMAs, but 179 registers = two waves per SIMD instead of three: the frame takes the same 2.15 ms)
#endif

struct LzNgpK {
    const float* packed;
    const void* feats;
    const float* dirs;
    const int* count;
    float* sigmas;
    float* rgbs;
    uint32_t rows;        // rows of feats / dirs (the encoder's B: it fixes the packing of the last, partial tile)
};

// FEAT: 0 = row-major f32 [rows, 32]; 1 = tiled f32 (lz_grid_encode_forward_tiled); 2 = tiled f16
#ifndef LZN_WG
#define LZN_WG 512     /* threads per workgroup: the 24 KB weight image is copied once per workgroup (256 -> 512 and 4 -> 8 passes per wave: cfg2 frame 2.07 -> 2.03 ms) */
#endif
#ifndef LZN_PASSES
#define LZN_PASSES 8   /* passes per wave the grid is sized for when there are rows enough for two workgroups per CU; halved until there are */
#endif
template <int FEAT>
__global__ void __launch_bounds__(LZN_WG) lz_k_ngp_head(LzNgpK P) {
    __shared__ __align__(16) float wl[LZ_NGP_FRAGS * 64];
    {
        const float4* src = reinterpret_cast<const float4*>(P.packed);
        float4* dst = reinterpret_cast<float4*>(wl);
        for (uint32_t i = threadIdx.x; i < LZ_NGP_FRAGS * 16; i += blockDim.x) dst[i] = src[i];
    }
    __syncthreads();
    uint32_t rows = P.rows;
    if (P.count) {
        const int c = *P.count;
        rows = c < 0 ? 0u : ((uint32_t)c < rows ? (uint32_t)c : rows);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, s = lane & 15, q = lane >> 4;
    const uint32_t n_slices = (rows + 15u) / 16u;
    constexpr int T = LZN_T;
    const uint32_t stride = gridDim.x * (LZN_WG / 64u) * T;
    uint32_t slice0 = (blockIdx.x * (LZN_WG / 64u) + (uint32_t)wave) * T;
    if (rows == 0 || slice0 >= n_slices) return;
    LznIn<T> nxt;
    lzn_load<FEAT, T>(P.feats, P.dirs, P.rows, rows, s, q, slice0, nxt);
    for (; slice0 < n_slices; slice0 += stride) {
        // the next pass's inputs are requested before this pass's 96 MFMAs (a wave's pass otherwise starts with a round trip to the tiles)
        const LznIn<T> cur = nxt;
        if (slice0 + stride < n_slices) lzn_load<FEAT, T>(P.feats, P.dirs, P.rows, rows, s, q, slice0 + stride, nxt);
        LznOut<T> o;
        lzn_chain<T>(wl, lane, q, cur, o);
#pragma unroll
        for (int u = 0; u < T; u++)
            if (q == 0 && cur.valid[u]) {
                P.sigmas[cur.row[u]] = lz_expf(o.h[u][0]);
                P.rgbs[(size_t)cur.row[u] * 3] = lz_sigmoidf(o.c[u][0]);
                P.rgbs[(size_t)cur.row[u] * 3 + 1] = lz_sigmoidf(o.c[u][1]);
                P.rgbs[(size_t)cur.row[u] * 3 + 2] = lz_sigmoidf(o.c[u][2]);
            }
    }
}

extern "C" int lz_ngp_head_forward(const float* packed, const void* feats, int feat_layout, const float* dirs, uint32_t rows, const int32_t* count,
                                   float* sigmas, float* rgbs, lz_stream_t stream) {
    if (rows == 0) return LZ_OK;
    LZ_REQUIRE(packed && feats && dirs && sigmas && rgbs, LZ_ERR_BAD_ARGUMENT, "ngp_head_forward: null tensor");
    LZ_REQUIRE(feat_layout >= 0 && feat_layout <= 2, LZ_ERR_BAD_ARGUMENT, "ngp_head_forward: feat_layout 0 (row-major f32), 1 (tiled f32) or 2 (tiled f16)");
    LzNgpK K{packed, feats, dirs, count, sigmas, rgbs, rows};
    uint32_t passes = LZN_PASSES;      // the reference schedule's iterations hold one sample per ray: few rows, keep every CU busy
    while (passes > 1 && lz_div_up(rows, 16 * (LZN_WG / 64) * passes * LZN_T) < 512) passes >>= 1;
    uint32_t grid = lz_div_up(rows, 16 * (LZN_WG / 64) * passes * LZN_T);
    // every workgroup stages the 24 KB of weights once: as many workgroups as the chip holds at a time (3 waves per SIMD = 3 of these 4-wave
    // workgroups per CU), each looping over its share of the slices, not one per 16 slices
    const uint32_t cap = (uint32_t)lz_cu_count() * LZN_WG_PER_CU;
    grid = grid < 1 ? 1 : (grid > cap ? cap : grid);
    hipStream_t st = lz_st(stream);
    if (feat_layout == 0) hipLaunchKernelGGL((lz_k_ngp_head<0>), dim3(grid), dim3(LZN_WG), 0, st, K);
    else if (feat_layout == 1) hipLaunchKernelGGL((lz_k_ngp_head<1>), dim3(grid), dim3(LZN_WG), 0, st, K);
    else hipLaunchKernelGGL((lz_k_ngp_head<2>), dim3(grid), dim3(LZN_WG), 0, st, K);
    LZ_CHECK_LAUNCH("ngp_head_forward");
    return LZ_OK;
}

// ==================================================================================================================================
// lz_k_ngp_head16: the same network in the arithmetic the reference renders in by default (`-O` => --fp16: torch.autocast, CUDA policy)
//   features   half, straight from the f16 tiled gather (grid.py:38-39 gathers from a half copy of the table under autocast)
//   Linear     half input and weight, f32 accumulation, half output (nn.Linear is on autocast's half list); ReLU on the half value
//   sigma      exp of the half pre-activation in f32 (exp is on CUDA autocast's fp32 list): lz_expf, so its bits follow from the
//              pre-activation's
//   colour in  cat([SH f32, geometry half]) promotes to f32; colour_net.0's cast rounds SH to half (the geometry is already half)
//   rgb        sigmoid of the half output, rounded to half (sigmoid is not listed: it runs in the input type)
// tests/ngp_fp16_checker.py restates the sequence; tests/golden/reference_ngp_autocast.npz pins it to the reference's own modules.
//
// Shape: 32-sample slices on v_mfma_f32_32x32x16_f16, the layout of lz_head_f16w_slice.h (lane l = (s = l & 31, h = l >> 5), B operand
// of k-step ks = k slots 16 ks + 8 h + j of sample s, D register i = output row (i & 3) + 8 (i >> 2) + 4 h).  Per 32 samples:
//   sigma_net.0  32 -> 64   2 k-steps x 2 tiles   B: the gathered halves, k slot = feature (lane half h reads levels 8 ks + 4 h .. + 3)
//   sigma_net.1  64 -> 16   4 x 1                 B: sigma_net.0's D tiles in registers (w_chain); tile rows 16..31 zero
//   colour_net.0 32 -> 64   2 x 2                 k-step 0: SH components 8 h + j; k-step 1: sigma_net.1's tile (w_chain), sigma's row 0
//   colour_net.1 64 -> 3    4 x 1                 B: colour_net.0's D tiles (w_chain)
// 16 MFMAs where the f32 head issues 192 v_mfma_f32_16x16x4_f32.  The packer (ngp.py: pack_weights_f16) permutes two sets of rows so
// that the four transcendentals of a sample sit two per lane: sigma_net output 0 (sigma) at tile row 4 and output 4 at row 0; colour
// channels 0 / 1 / 2 at tile rows 0 / 4 / 1.  Lane half 0 then holds channel 0 (register 0) and channel 2 (register 1), lane half 1
// channel 1 (register 0) and the sigma pre-activation (sigma_net.1's register 0).
struct LzNgp16K {
    const lz_h8* packed;
    const uint32_t* feats;  // tiled f16 features, one half2 (both channels of a level) per word
    const float* dirs;
    const int* count;
    float* sigmas;
    float* rgbs;
    uint32_t rows;
};

__global__ void __launch_bounds__(LZN_WG) lz_k_ngp_head16(LzNgp16K P) {
    __shared__ lz_h8 wl[LZN16_FRAGS * 64];
    for (uint32_t i = threadIdx.x; i < LZN16_FRAGS * 64; i += blockDim.x) wl[i] = P.packed[i];
    __syncthreads();
    uint32_t rows = P.rows;
    if (P.count) {
        const int c = *P.count;
        rows = c < 0 ? 0u : ((uint32_t)c < rows ? (uint32_t)c : rows);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, s = lane & 31, h = lane >> 5;
    const uint32_t n_slices = (rows + 31u) / 32u, Tn = LZ_GRID_TILE_ROWS;
    // the inputs of a pass: this lane's eight feature words (levels 8 ks + 4 h + i, i < 4, of sample s) and the direction
    struct In { uint32_t row; bool valid; uint32_t f[8]; float dx, dy, dz; };
    auto load = [&](uint32_t slice, In& I) {
        I.row = slice * 32u + (uint32_t)s;
        I.valid = I.row < rows;
        const uint32_t r = I.valid ? I.row : rows - 1u;
        const uint32_t tile = r / Tn, t = r - tile * Tn, b0 = tile * Tn, n = (P.rows - b0 < Tn) ? P.rows - b0 : Tn;
        const uint32_t* f = P.feats + (size_t)b0 * 16;
#pragma unroll
        for (int ks = 0; ks < 2; ks++)
#pragma unroll
            for (int i = 0; i < 4; i++) I.f[4 * ks + i] = f[(size_t)(8 * ks + 4 * h + i) * n + t];
        I.dx = P.dirs[(size_t)r * 3]; I.dy = P.dirs[(size_t)r * 3 + 1]; I.dz = P.dirs[(size_t)r * 3 + 2];
    };
    const uint32_t stride = gridDim.x * (LZN_WG / 64u);
    uint32_t slice = blockIdx.x * (LZN_WG / 64u) + (uint32_t)wave;
    if (rows == 0 || slice >= n_slices) return;
    In nxt;
    load(slice, nxt);
    for (; slice < n_slices; slice += stride) {
        const In cur = nxt;     // the next pass's loads are in flight under this pass's 16 MFMAs
        if (slice + stride < n_slices) load(slice + stride, nxt);
        // SH(4) of the sample's direction as the packed halves of this lane half (components 8 h .. 8 h + 7), then the 16-MFMA chain
        uint32_t shw[4];
        {
            float sh[16];
            lz_sh_eval(cur.dx, cur.dy, cur.dz, 4, sh, nullptr, nullptr, nullptr);
            lzn16_sh_words(sh, h, shw);
        }
        float rgb_a, b_out;
        lzn16_chain(wl, lane, h, cur.f, shw, rgb_a, b_out);
        if (cur.valid) {
            float* rgb = P.rgbs + (size_t)cur.row * 3;
            rgb[h] = rgb_a;
            if (h) P.sigmas[cur.row] = b_out;
            else rgb[2] = b_out;
        }
    }
}

extern "C" int lz_ngp_head_forward_f16(const void* packed16, const void* feats, int feat_layout, const float* dirs, uint32_t rows, const int32_t* count,
                                       float* sigmas, float* rgbs, lz_stream_t stream) {
    if (rows == 0) return LZ_OK;
    LZ_REQUIRE(packed16 && feats && dirs && sigmas && rgbs, LZ_ERR_BAD_ARGUMENT, "ngp_head_forward_f16: null tensor");
    LZ_REQUIRE(feat_layout == 2, LZ_ERR_BAD_ARGUMENT, "ngp_head_forward_f16: feat_layout must be 2 (tiled f16)");
    LzNgp16K K{reinterpret_cast<const lz_h8*>(packed16), reinterpret_cast<const uint32_t*>(feats), dirs, count, sigmas, rgbs, rows};
    uint32_t passes = LZN_PASSES;
    while (passes > 1 && lz_div_up(rows, 32 * (LZN_WG / 64) * passes) < 512) passes >>= 1;
    uint32_t grid = lz_div_up(rows, 32 * (LZN_WG / 64) * passes);
    const uint32_t cap = (uint32_t)lz_cu_count() * LZN_WG_PER_CU;
    grid = grid < 1 ? 1 : (grid > cap ? cap : grid);
    hipLaunchKernelGGL(lz_k_ngp_head16, dim3(grid), dim3(LZN_WG), 0, lz_st(stream), K);
    LZ_CHECK_LAUNCH("ngp_head_forward_f16");
    return LZ_OK;
}

// enqueue `n_iterations` iterations of the reference's inference loop (renderer.py:503-548) around the hash-grid NeRF: march -> gather ->
// head -> composite, four launches each, no host round trip; iterations past the end of the frame are no-ops on the device.
// packed16 == nullptr: the f32 head on f->packed, else the f16 head on packed16 (f->emb_f16 == 1, checked by the caller)
static int ngp_loop(const lz_frame_ngp* f, const void* packed16, uint32_t parity, uint32_t n_iterations, lz_stream_t stream) {
    LZ_REQUIRE(f->state && f->workspace && (packed16 || f->packed) && f->embeddings && f->offsets, LZ_ERR_BAD_ARGUMENT, "ngp_loop_run: incomplete lz_frame_ngp");
    if (f->N == 0) return LZ_OK;                 // no ray: nothing to enqueue
    LZ_REQUIRE(f->rays_alive[0] && f->rays_alive[1] && f->feats, LZ_ERR_BAD_ARGUMENT, "ngp_loop_run: incomplete lz_frame_ngp");
    uint32_t cur = parity & 1u;
    const int32_t* count = reinterpret_cast<const int32_t*>(f->state) + LZ_LOOP_NEXT + 2;  // n_samples of the iteration in flight
    const uint32_t rows = f->sample_budget > f->N ? f->sample_budget : f->N;  // capacity of the sample buffers
    for (uint32_t it = 0; it < n_iterations; it++) {
        const uint32_t nxt = cur ^ 1u;
        int rc = lz_loop_march(f->state, f->N, f->sample_budget, f->n_step_cap, f->rays_alive[cur], f->rays_alive[nxt], f->workspace, f->rays_t,
                               f->rays_o, f->rays_d, f->bound, f->dt_gamma, f->max_steps, f->C, f->H, f->grid, f->nears, f->fars, f->xyzs,
                               f->dirs, f->deltas, f->ray_counts, stream);
        if (rc != LZ_OK) return rc;
        rc = lz_grid_encode_forward_tiled(f->xyzs, f->embeddings, f->offsets, f->feats, rows, count, f->bound, 3, 2, f->enc_L, f->enc_S, f->enc_H, 0,
                                          0, f->emb_f16, stream);
        if (rc != LZ_OK) return rc;
        rc = packed16 ? lz_ngp_head_forward_f16(packed16, f->feats, 2, f->dirs, rows, count, f->sigmas, f->rgbs, stream)
                      : lz_ngp_head_forward(f->packed, f->feats, f->emb_f16 ? 2 : 1, f->dirs, rows, count, f->sigmas, f->rgbs, stream);
        if (rc != LZ_OK) return rc;
        rc = lz_loop_composite_plain(f->state, f->N, f->T_thresh, f->rays_alive[nxt], f->rays_t, f->sigmas, f->rgbs, f->deltas, f->weights_sum,
                                     f->depth, f->image, f->workspace, stream);
        if (rc != LZ_OK) return rc;
        cur = nxt;
    }
    return LZ_OK;
}

extern "C" int lz_ngp_loop_run(const lz_frame_ngp* f, uint32_t parity, uint32_t n_iterations, lz_stream_t stream) {
    LZ_REQUIRE(f, LZ_ERR_BAD_ARGUMENT, "ngp_loop_run: null");
    return ngp_loop(f, nullptr, parity, n_iterations, stream);
}

// the same loop with lz_k_ngp_head16 as its network: half tables and half features (emb_f16 == 1) are part of that arithmetic
extern "C" int lz_ngp_loop_run_f16(const lz_frame_ngp* f, const void* packed16, uint32_t parity, uint32_t n_iterations, lz_stream_t stream) {
    LZ_REQUIRE(f && packed16, LZ_ERR_BAD_ARGUMENT, "ngp_loop_run_f16: null");
    LZ_REQUIRE(f->emb_f16 == 1, LZ_ERR_BAD_ARGUMENT, "ngp_loop_run_f16: the f16 head reads half features (emb_f16 = 1)");
    return ngp_loop(f, packed16, parity, n_iterations, stream);
}
