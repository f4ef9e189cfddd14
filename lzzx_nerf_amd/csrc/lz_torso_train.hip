// lz_torso_train.hip -- the torso stage's training pass (train.py --torso: "fix head and train torso"): run_torso's masked query
// (nerf_triplane/renderer.py:572-631) + forward_torso (network.py:170-205) forward and backward, for FusedTorsoTrainNet
// (lzzx_nerf_amd/torso_train.py).
//
// Forward: lz_k_torso_forward's chain (lz_torso_net.h, the same code), so alpha / colour / deform are the inference kernel's bits; the
// occupancy threshold comes from device memory and the colour is optionally mixed with the background.
//
// Backward: nothing is recorded.  Each wave recomputes the forward of a 16-pixel slice (the chain of lz_torso_net.h) and runs the data
// gradients back through the layers on the same v_mfma_f32_16x16x4_f32 shape with TRANSPOSED weight fragments (D[k, pixel] =
// W^T . G): torso net 4 -> 32 -> 32 -> grid features 32 (the enc_x columns need no gradient: x is an input), the grid's dy/dx and
// the clamp, deform net 2 -> 32 -> 32.  The table gradient is scattered with float atomics, or (the ROWS instantiations) the
// encoder-output gradient is written out for the grid encoder's ordered / order-free table-gradient kernels.  Weight gradients take pixels as the
// MFMA's k dimension: the slice's layer inputs and output gradients are staged in the wave's LDS as [feature][16 pixels] rows, read
// back four pixels per lane as one 16-byte load, and accumulated over the wave's slices into 28 16 x 16 tiles (112 registers).
// Pixel row 34 of the staged frequency features is set to 1, so the tiles' column 34 carries the pixel sums of the first layers'
// output gradients: the gradients of the frame-constant inputs (anchor encoding, individual code) and of their weight columns are
// formed from those sums by the combine kernel.  The staging, the wave fold and the fixed-order combine are lz_train_wgrad.h's: no
// float atomics, same bits on every call.
#include "lz_torso_net.h"
#include "lz_train_wgrad.h"

// backward (transposed) fragments: lane l of fragment (ks, ft) = W[4 ks + (l >> 4)][16 ft + (l & 15)]
enum { LZTB_T2 = 0, LZTB_T1, LZTB_T0G, LZTB_D2, LZTB_D1, LZTB_LAYERS };
constexpr int LZTB_KS[LZTB_LAYERS] = {1, 8, 8, 1, 8};   // k = the forward layer's outputs: 4, 32, 32, 2, 32
constexpr int lztb_base(int layer) {
    int b = 0;
    for (int i = 0; i < layer; i++) b += LZTB_KS[i] * 2;
    return b;
}
constexpr int LZTB_FRAGS = lztb_base(LZTB_LAYERS);   // 52 fragments
// per-wave staging rows ([feature][16 pixels] floats)
enum : int {
    LZTS_EX = 0,                  // 36 rows: frequency features 0-33, row 34 = 1 (pixel sums), row 35 = 0
    LZTS_RD1 = LZTS_EX + 36 * 16, // deform net ReLU outputs (inputs of layers 1, 2)
    LZTS_RD2 = LZTS_RD1 + 512,
    LZTS_GX = LZTS_RD2 + 512,     // grid features
    LZTS_RT1 = LZTS_GX + 512,     // torso net ReLU outputs
    LZTS_RT2 = LZTS_RT1 + 512,
    LZTS_GZ0 = LZTS_RT2 + 512,    // output gradients of deform layers 0, 1, 2
    LZTS_GZ1 = LZTS_GZ0 + 512,
    LZTS_GDX = LZTS_GZ1 + 512,    // 4 rows (2 used)
    LZTS_GT0 = LZTS_GDX + 64,     // output gradients of torso layers 0, 1, 2
    LZTS_GT1 = LZTS_GT0 + 512,
    LZTS_GO = LZTS_GT1 + 512,     // 4 rows
    LZTS_WAVE = LZTS_GO + 64,     // 5312 floats per wave
};
// weight-gradient tiles (fo: 16-row block of outputs, fk: 16-column block of the layer's per-pixel inputs)
//   0-5 D0 (2 x 3, inputs ex)  6-9 D1 (2 x 2)  10-11 D2 (1 x 2)  12-21 T0 (2 x 5, inputs [grid 32 | ex 36])  22-25 T1  26-27 T2
#define LZTG_TILES 28
#define LZTG_ELEMS (LZTG_TILES * 256)
#define LZTS_SIZE (LZTG_ELEMS > 4 * LZTS_WAVE ? LZTG_ELEMS : 4 * LZTS_WAVE)   // staging rows, reused by the wave fold

struct LzTorsoTrainArgs {
    LzTorsoArgs a;
    const float* thresh;
    const float* bg;
    float bg_scalar;
    uint32_t mix;
};

__device__ __forceinline__ bool lzt_masked(const LzTorsoTrainArgs& T, float bx, float by) {
    const lz_torso_params& P = T.a.p;
    if (!P.density_grid) return true;
    const float th = T.thresh ? *T.thresh : P.density_thresh;
    return lzt_occupancy(P.density_grid, P.G, bx, by) > th;
}

__device__ __forceinline__ float lzt_bg(const LzTorsoTrainArgs& T, uint32_t n, int ch) { return T.bg ? T.bg[(size_t)n * 3 + ch] : T.bg_scalar; }

template <int IND>
__global__ void __launch_bounds__(LZT_WG)
lz_k_torso_train_forward(LzTorsoTrainArgs T, const float* __restrict__ bg_coords, uint32_t N, float* __restrict__ alpha_out,
                         float* __restrict__ color_out, float* __restrict__ deform_out) {
    constexpr int H = LZ_TORSO_HID;
    __shared__ float wl[LZT_FRAGS * 64];
    __shared__ __align__(16) float cd[H], ct[H];
    lzt_setup<IND>(T.a.p, wl, cd, ct);
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int s = lane & 15, q = lane >> 4;
    const uint32_t n_slices = (N + 15) / 16, stride = gridDim.x * (LZT_WG / 64);
    for (uint32_t slice = blockIdx.x * (LZT_WG / 64) + wave; slice < n_slices; slice += stride) {
        const uint32_t n_raw = slice * 16 + s;
        const bool valid = n_raw < N;
        const uint32_t n = valid ? n_raw : N - 1;
        const float bx = bg_coords[(size_t)n * 2], by = bg_coords[(size_t)n * 2 + 1];
        const bool masked = lzt_masked(T, bx, by);
        float out[4] = {0.0f, 0.0f, 0.0f, 0.0f}, dx[2] = {0.0f, 0.0f};
        if (__ballot(masked && valid)) {
            LztFwd f;
            lzt_forward<IND>(T.a, wl, cd, ct, lane, bx, by, f);
            if (masked) {
#pragma unroll
                for (int o = 0; o < 4; o++) out[o] = lzt_out(f.o[o]);
                dx[0] = f.dx[0]; dx[1] = f.dx[1];
            }
        }
        if (q == 0 && valid) {
            alpha_out[n] = out[0];
#pragma unroll
            for (int ch = 0; ch < 3; ch++)   // renderer.py:621, torch's op order: c * a + bg * (1 - a)
                color_out[(size_t)n * 3 + ch] = T.mix ? out[1 + ch] * out[0] + lzt_bg(T, n, ch) * (1.0f - out[0]) : out[1 + ch];
            if (deform_out) { deform_out[(size_t)n * 2] = dx[0]; deform_out[(size_t)n * 2 + 1] = dx[1]; }
        }
    }
}

template <int KS>
__device__ __forceinline__ void lztb_layer(const float* __restrict__ frag0, int lane, const float (&b)[KS], lzt_f4 (&acc)[2]) {
    const float* frag = frag0 + lane;
#pragma unroll
    for (int ks = 0; ks < KS; ks++)
#pragma unroll
        for (int ft = 0; ft < 2; ft++) acc[ft] = __builtin_amdgcn_mfma_f32_16x16x4f32(frag[(ks * 2 + ft) * 64], b[ks], acc[ft], 0, 0, 0);
}

// D tiles of an input gradient -> B layout (register 4 t + j = feature 16 t + 4 j + q), times the ReLU mask of the forward's output
__device__ __forceinline__ void lztb_to_b(lzt_f4 (&acc)[2], const float (&relu_out)[8], float (&g)[8]) {
#pragma unroll
    for (int t = 0; t < 2; t++) {
        lzt_transpose(acc[t]);
#pragma unroll
        for (int j = 0; j < 4; j++) g[4 * t + j] = relu_out[4 * t + j] > 0.0f ? acc[t][j] : 0.0f;
    }
}

// rows variant: lane (s, q)'s element of pixel n at level q >> 1, channel q & 1; level 2 i + (q >> 1) lies 4 i N floats further on
__device__ __forceinline__ float* lzt_rows_at(float* __restrict__ denc, uint32_t N, uint32_t n, int q) {
    return denc + ((size_t)(q >> 1) * N + n) * 2 + (q & 1);
}

// ROWS = false: the table gradient is scattered into g_emb with float atomics.  ROWS = true: g_emb is not touched; the kernel hands the
// encoder-output gradient to the grid encoder's table-gradient kernels (lz_grid_encode_backward_ordered / _fixed) instead: denc, level-major
// [16, N, 2] (their grad_layout 0; lane (s, q) writes element (l N + n) 2 + ch with l = 2 i + (q >> 1), ch = q & 1, so one store
// instruction fills one 128-byte run per level for the slice's 16 pixels x 2 channels), and u_out [N, 2], the [0, 1] coordinates the
// table was gathered at.  Every pixel n < N gets its rows, so neither buffer needs initialisation, and a pixel's rows do not depend on
// its place in a slice.  A pixel that is masked out or out of range, and every pixel of a skipped slice, gets zeros and u = LZT_ROWS_NO_U,
// a coordinate outside [0, 1]: every table-gradient kernel of the grid encoder drops such a row before it touches the table.  u = 0 would
// add the same nothing, but all those rows would then meet in the corner entries of every level: measured on the whole frame with 12 % of
// it masked out, the step took 2.97 instead of 0.97 ms under "fixed" (same-address LDS atomics) and 137 instead of 12.9 ms under
// "ordered" (one thread walks an entry's segment).
#define LZT_ROWS_NO_U (-1.0f)
template <int IND, bool ROWS>
__global__ void __launch_bounds__(LZT_WG)
lz_k_torso_train_backward(LzTorsoTrainArgs T, const float* __restrict__ bg_coords, uint32_t N, const float* __restrict__ g_alpha,
                          const float* __restrict__ g_color, const float* __restrict__ g_deform, float* __restrict__ g_emb,
                          float* __restrict__ partials, float* __restrict__ denc, float* __restrict__ u_out) {
    constexpr int H = LZ_TORSO_HID, KC = LZ_TORSO_ANCHOR + IND, K1 = LZ_TORSO_GRIDF + LZ_TORSO_FREQ + KC;
    __shared__ float wl[LZT_FRAGS * 64];
    __shared__ __align__(16) float wb[LZTB_FRAGS * 64];
    __shared__ __align__(16) float stage[LZTS_SIZE];
    __shared__ __align__(16) float cd[H], ct[H];
    const lz_torso_params& P = T.a.p;
    lzt_setup<IND>(P, wl, cd, ct);
    {   // transposed fragments; zero outside the matrix
        auto packt = [&](int layer, const float* __restrict__ w, int ld, int n_rows, int n_cols) {
            const int cnt = LZTB_KS[layer] * 2 * 64;
            float* dst = wb + lztb_base(layer) * 64;
            for (int i = threadIdx.x; i < cnt; i += LZT_WG) {
                const int fr = i >> 6, l = i & 63, ks = fr >> 1, ft = fr & 1;
                const int row = 4 * ks + (l >> 4), col = 16 * ft + (l & 15);
                dst[i] = (row < n_rows && col < n_cols) ? w[(size_t)row * ld + col] : 0.0f;
            }
        };
        packt(LZTB_T2, P.torso_w2, H, 4, H);
        packt(LZTB_T1, P.torso_w1, H, H, H);
        packt(LZTB_T0G, P.torso_w0, K1, H, LZ_TORSO_GRIDF);
        packt(LZTB_D2, P.deform_w2, H, 2, H);
        packt(LZTB_D1, P.deform_w1, H, H, H);
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int s = lane & 15, q = lane >> 4;
    float* st = stage + wave * LZTS_WAVE;
    const uint32_t n_slices = (N + 15) / 16, stride = gridDim.x * (LZT_WG / 64);
    if constexpr (ROWS) {   // the rows of the slices that the loop below skips, in a loop of their own: a second way round that one, with
                            // stores in it, makes the compiler keep the 28 accumulator tiles twice
        for (uint32_t slice = blockIdx.x * (LZT_WG / 64) + wave; slice < n_slices; slice += stride) {
            const uint32_t n = slice * 16 + s;
            const bool valid = n < N;
            const size_t nc = valid ? n : N - 1;
            const bool live = lzt_masked(T, bg_coords[nc * 2], bg_coords[nc * 2 + 1]) && valid;
            if (__ballot(live) || !valid) continue;
            float* drow = lzt_rows_at(denc, N, n, q);
#pragma unroll
            for (int i = 0; i < 8; i++) drow[(size_t)i * 4 * N] = 0.0f;
            if (q < 2) u_out[(size_t)n * 2 + q] = LZT_ROWS_NO_U;
        }
    }
    lzt_f4 gw[LZTG_TILES];
#pragma unroll
    for (int t = 0; t < LZTG_TILES; t++) gw[t] = lzt_f4{0, 0, 0, 0};
    for (uint32_t slice = blockIdx.x * (LZT_WG / 64) + wave; slice < n_slices; slice += stride) {
        const uint32_t n_raw = slice * 16 + s;
        const bool valid = n_raw < N;
        const uint32_t n = valid ? n_raw : N - 1;
        const float bx = bg_coords[(size_t)n * 2], by = bg_coords[(size_t)n * 2 + 1];
        const bool live = lzt_masked(T, bx, by) && valid;
        if (!__ballot(live)) continue;   // masked-out pixels contribute nothing
        LztFwd f;
        lzt_forward<IND>(T.a, wl, cd, ct, lane, bx, by, f);
        // ---- output gradients: lane (s, q) owns output q (alpha, r, g, b) of pixel s ----
        float y[4];
#pragma unroll
        for (int o = 0; o < 4; o++) y[o] = lz_sigmoidf(__shfl(f.o[o], s, 64));
        const float a = y[0] * 1.002f - 0.001f;
        float g_out = 0.0f;
        if (live) {
            if (q == 0) {
                g_out = g_alpha ? g_alpha[n] : 0.0f;
                if (T.mix && g_color)   // d(c a + bg (1 - a)) / da = c - bg
                    for (int ch = 0; ch < 3; ch++) g_out += g_color[(size_t)n * 3 + ch] * ((y[1 + ch] * 1.002f - 0.001f) - lzt_bg(T, n, ch));
            } else if (g_color) {
                g_out = g_color[(size_t)n * 3 + q - 1];
                if (T.mix) g_out *= a;
            }
        }
        const float yq = q == 0 ? y[0] : q == 1 ? y[1] : q == 2 ? y[2] : y[3];
        const float go[1] = {g_out * 1.002f * (yq * (1.0f - yq))};
        // ---- torso net backward ----
        float gt1[8], gt0[8], gg[8];
        {
            lzt_f4 acc[2] = {lzt_f4{0, 0, 0, 0}, lzt_f4{0, 0, 0, 0}};
            lztb_layer<1>(wb + lztb_base(LZTB_T2) * 64, lane, go, acc);
            lztb_to_b(acc, f.bt2, gt1);
            lzt_f4 acc1[2] = {lzt_f4{0, 0, 0, 0}, lzt_f4{0, 0, 0, 0}};
            lztb_layer<8>(wb + lztb_base(LZTB_T1) * 64, lane, gt1, acc1);
            lztb_to_b(acc1, f.bt1, gt0);
            lzt_f4 acc0[2] = {lzt_f4{0, 0, 0, 0}, lzt_f4{0, 0, 0, 0}};
            lztb_layer<8>(wb + lztb_base(LZTB_T0G) * 64, lane, gt0, acc0);
#pragma unroll
            for (int t = 0; t < 2; t++) {
                lzt_transpose(acc0[t]);
#pragma unroll
                for (int j = 0; j < 4; j++) gg[4 * t + j] = acc0[t][j];
            }
        }
        // ---- grid: scatter into the table, dy/dx into u (gridencoder.cu's backward and its dy_dx) ----
        float du[2] = {0.0f, 0.0f};
        {
            const bool oob = f.u[0] < 0 || f.u[0] > 1 || f.u[1] < 0 || f.u[1] > 1;
            const int ch = q & 1;
            float* drow = nullptr;
            if constexpr (ROWS) {   // lanes q = 0, 1 of a pixel write its two coordinates: 128 contiguous bytes per slice
                drow = lzt_rows_at(denc, N, n, q);
                if (valid && q < 2) u_out[(size_t)n * 2 + q] = (live && !oob) ? (q == 0 ? f.u[0] : f.u[1]) : LZT_ROWS_NO_U;
            }
#pragma unroll
            for (int i = 0; i < 8; i++) {
                const int l = 2 * i + (q >> 1);
                const uint32_t off0 = (uint32_t)P.offsets[l], hs = (uint32_t)P.offsets[l + 1] - off0;
                const float sc = T.a.scale[l];
                const LztCell cl = lzt_cell(f.u, sc);
                const float* g = P.emb + (size_t)off0 * 2 + ch;
                float e[4];
                if constexpr (ROWS) {   // the terms w gg are formed by the table-gradient kernel, from the same cell and weights
                    if (valid) *drow = (live && !oob) ? gg[i] : 0.0f;
                    drow += (size_t)4 * N;
#pragma unroll
                    for (int c = 0; c < 4; c++) e[c] = g[lz_torso_grid_index(P.gridtype, hs, T.a.res[l], cl.g0 + (c & 1), cl.g1 + (c >> 1))];
                } else {
                    float* gd = g_emb + (size_t)off0 * 2 + ch;
#pragma unroll
                    for (int c = 0; c < 4; c++) {
                        const uint32_t index = lz_torso_grid_index(P.gridtype, hs, T.a.res[l], cl.g0 + (c & 1), cl.g1 + (c >> 1));
                        e[c] = g[index];
                        const float w = ((c & 1) ? cl.f0 : 1 - cl.f0) * ((c >> 1) ? cl.f1 : 1 - cl.f1);
                        if (live && !oob && gg[i] != 0.0f) unsafeAtomicAdd(gd + index, w * gg[i]);
                    }
                }
                if (live && !oob) {
                    du[0] += gg[i] * sc * ((1 - cl.f1) * (e[1] - e[0]) + cl.f1 * (e[3] - e[2]));
                    du[1] += gg[i] * sc * ((1 - cl.f0) * (e[2] - e[0]) + cl.f0 * (e[3] - e[1]));
                }
            }
        }
#pragma unroll
        for (int d = 0; d < 2; d++) {   // the pixel's four lanes, fixed order
            du[d] += __shfl_xor(du[d], 16, 64);
            du[d] += __shfl_xor(du[d], 32, 64);
        }
        // u = (clamp(x + dx, -1, 1) + 1) / 2: the clamp passes where -1 <= v <= 1 (torch); the upstream deform gradient on top
        float gdx[2];
#pragma unroll
        for (int d = 0; d < 2; d++) {
            const float v = f.x[d] + f.dx[d];
            gdx[d] = (v >= -1.0f && v <= 1.0f) ? du[d] * 0.5f : 0.0f;
            if (live && g_deform) gdx[d] += g_deform[(size_t)n * 2 + d];
            if (!live) gdx[d] = 0.0f;
        }
        const float gdb[1] = {q == 0 ? gdx[0] : q == 1 ? gdx[1] : 0.0f};
        // ---- deform net backward ----
        float gz1[8], gz0[8];
        {
            lzt_f4 acc[2] = {lzt_f4{0, 0, 0, 0}, lzt_f4{0, 0, 0, 0}};
            lztb_layer<1>(wb + lztb_base(LZTB_D2) * 64, lane, gdb, acc);
            lztb_to_b(acc, f.bd2, gz1);
            lzt_f4 acc1[2] = {lzt_f4{0, 0, 0, 0}, lzt_f4{0, 0, 0, 0}};
            lztb_layer<8>(wb + lztb_base(LZTB_D1) * 64, lane, gz1, acc1);
            lztb_to_b(acc1, f.bd1, gz0);
        }
        // ---- stage the slice and accumulate the weight gradients (pixels as k) ----
        float ex[9];
#pragma unroll
        for (int i = 0; i < 9; i++) ex[i] = f.ex[i];
        if (q == 2) ex[8] = 1.0f;   // row 34: the pixel sums of the first layers' output gradients
        lz_wg_stage_b<9>(st + LZTS_EX, lane, ex);
        lz_wg_stage_b<8>(st + LZTS_RD1, lane, f.bd1);
        lz_wg_stage_b<8>(st + LZTS_RD2, lane, f.bd2);
        lz_wg_stage_b<8>(st + LZTS_GX, lane, f.gx);
        lz_wg_stage_b<8>(st + LZTS_RT1, lane, f.bt1);
        lz_wg_stage_b<8>(st + LZTS_RT2, lane, f.bt2);
        lz_wg_stage_b<8>(st + LZTS_GZ0, lane, gz0);
        lz_wg_stage_b<8>(st + LZTS_GZ1, lane, gz1);
        lz_wg_stage_b<1>(st + LZTS_GDX, lane, gdb);
        lz_wg_stage_b<8>(st + LZTS_GT0, lane, gt0);
        lz_wg_stage_b<8>(st + LZTS_GT1, lane, gt1);
        lz_wg_stage_b<1>(st + LZTS_GO, lane, go);
        lz_wave_lds_sync();
        lz_wg_tiles<2, 3>(gw + 0, st + LZTS_GZ0, 32, st + LZTS_EX, 36, lane);
        lz_wg_tiles<2, 2>(gw + 6, st + LZTS_GZ1, 32, st + LZTS_RD1, 32, lane);
        lz_wg_tiles<1, 2>(gw + 10, st + LZTS_GDX, 4, st + LZTS_RD2, 32, lane);
        lz_wg_tiles<2, 2, 5>(gw + 12, st + LZTS_GT0, 32, st + LZTS_GX, 32, lane);   // T0 (2 x 5): grid columns
        lz_wg_tiles<2, 3, 5>(gw + 14, st + LZTS_GT0, 32, st + LZTS_EX, 36, lane);   //            frequency columns
        lz_wg_tiles<2, 2>(gw + 22, st + LZTS_GT1, 32, st + LZTS_RT1, 32, lane);
        lz_wg_tiles<1, 2>(gw + 26, st + LZTS_GO, 4, st + LZTS_RT2, 32, lane);
        lz_wave_lds_sync();   // the next slice overwrites the rows just read
    }
    // ---- the waves folded in wave order into the staging rows, then one partial per workgroup ----
    lz_wg_fold_and_store<LZTG_TILES, LZT_WG / 64>(gw, stage, partials + (size_t)blockIdx.x * LZTG_ELEMS, lane, wave);
}

// ---- combine: the workgroup partials in workgroup order -> the weight gradients; the frame-constant gradients ----------------------
// Blocks 0 .. LZTG_ELEMS / 64 - 1: 64 tile elements each, four threads per element over interleaved quarters of the partials, the
// quarters added in order.  The last block: the 64 pixel sums (column 34 of the D0 / T0 frequency tiles) the same way, then the weight
// columns of the frame-constant inputs (sum x input) and g_enc_anchor / g_ind_code (W^T . sum, fixed order).
struct LzTorsoGradOut {
    float *dw0, *dw1, *dw2, *tw0, *tw1, *tw2, *g_enc, *g_ind;
};
#define LZTC_BLOCKS (LZTG_ELEMS / 64)

template <int IND>
__global__ void __launch_bounds__(256) lz_k_torso_train_combine(const float* __restrict__ partials, uint32_t n_groups, lz_torso_params P,
                                                                LzTorsoGradOut G) {
    constexpr int K0 = LZ_TORSO_FREQ + LZ_TORSO_ANCHOR + IND, K1 = LZ_TORSO_GRIDF + K0, H = LZ_TORSO_HID;
    __shared__ float red[4][64];
    __shared__ float sums[64];
    const int slot = threadIdx.x & 63;
    const bool last = blockIdx.x == LZTC_BLOCKS;
    int e = blockIdx.x * 64 + slot;
    if (last) {   // slot o < 32: sum of deform layer 0's output gradient o (D0 tile (o >> 4, 2), column 2); o >= 32: torso layer 0's (T0 tile (., 4))
        const int o = slot & 31;
        e = slot < 32 ? lz_wg_elem((o >> 4) * 3 + 2, o & 15, 2) : lz_wg_elem(12 + (o >> 4) * 5 + 4, o & 15, 2);
    }
    const float v = lz_wg_combine<LZTG_ELEMS>(partials, n_groups, e, red);
    if (!last) {
        if (threadIdx.x >= 64) return;
        const auto [t, row, col] = lz_wg_elem(e);
        if (t < 6) {            // D0: per-pixel columns 0-33
            const int o = 16 * (t / 3) + row, k = 16 * (t % 3) + col;
            if (k < LZ_TORSO_FREQ) G.dw0[o * K0 + k] = v;
        } else if (t < 10) {
            G.dw1[(16 * ((t - 6) >> 1) + row) * H + 16 * ((t - 6) & 1) + col] = v;
        } else if (t < 12) {
            if (row < 2) G.dw2[row * H + 16 * (t - 10) + col] = v;
        } else if (t < 22) {    // T0: [grid 32 | ex 34] = columns 0-65
            const int o = 16 * ((t - 12) / 5) + row, fk = (t - 12) % 5;
            const int k = fk < 2 ? 16 * fk + col : 16 * (fk - 2) + col;
            if (fk < 2) G.tw0[o * K1 + k] = v;
            else if (k < LZ_TORSO_FREQ) G.tw0[o * K1 + LZ_TORSO_GRIDF + k] = v;
        } else if (t < 26) {
            G.tw1[(16 * ((t - 22) >> 1) + row) * H + 16 * ((t - 22) & 1) + col] = v;
        } else {
            if (row < 4) G.tw2[row * H + 16 * (t - 26) + col] = v;
        }
        return;
    }
    if (threadIdx.x < 64) sums[slot] = v;
    __syncthreads();
    constexpr int KC = LZ_TORSO_ANCHOR + IND;
    for (int i = threadIdx.x; i < 2 * H * KC; i += 256) {   // weight columns of the constant inputs: sum_o x input_k
        const bool tor = i >= H * KC;
        const int j = tor ? i - H * KC : i, o = j / KC, k = j % KC;
        const float in = k < LZ_TORSO_ANCHOR ? P.enc_anchor[k] : P.ind_code[k - LZ_TORSO_ANCHOR];
        if (tor) G.tw0[o * K1 + LZ_TORSO_GRIDF + LZ_TORSO_FREQ + k] = sums[H + o] * in;
        else G.dw0[o * K0 + LZ_TORSO_FREQ + k] = sums[o] * in;
    }
    if (threadIdx.x < KC) {   // gradients of the constant inputs: both first layers, o in order
        const int k = threadIdx.x;
        float acc = 0.0f;
        for (int o = 0; o < H; o++) acc += P.deform_w0[o * K0 + LZ_TORSO_FREQ + k] * sums[o];
        for (int o = 0; o < H; o++) acc += P.torso_w0[o * K1 + LZ_TORSO_GRIDF + LZ_TORSO_FREQ + k] * sums[H + o];
        if (k < LZ_TORSO_ANCHOR) G.g_enc[k] = acc;
        else G.g_ind[k - LZ_TORSO_ANCHOR] = acc;
    }
}

// ---- anchor backward (network.py:179-183) ----------------------------------------------------------------------------------------
// enc = freq3(w6), w6 = (w0 / w3 / w2, w1 / w3 / w2) per anchor, w = pose^-1 a.  One thread in double; the inverse by cofactors
// (constant indices: no local-memory array, and no pivot -- torch.inverse's singularity check, a host synchronisation, has no counterpart)
__global__ void __launch_bounds__(64) lz_k_torso_anchor_encode_backward(const float* __restrict__ pose, const float* __restrict__ anchors,
                                                                        const float* __restrict__ g_enc, float* __restrict__ g_anchors) {
    if (threadIdx.x != 0) return;
    double m[16];
#pragma unroll
    for (int i = 0; i < 16; i++) m[i] = (double)pose[i];
    const double s0 = m[0] * m[5] - m[4] * m[1], s1 = m[0] * m[6] - m[4] * m[2], s2 = m[0] * m[7] - m[4] * m[3];
    const double s3 = m[1] * m[6] - m[5] * m[2], s4 = m[1] * m[7] - m[5] * m[3], s5 = m[2] * m[7] - m[6] * m[3];
    const double c5 = m[10] * m[15] - m[14] * m[11], c4 = m[9] * m[15] - m[13] * m[11], c3 = m[9] * m[14] - m[13] * m[10];
    const double c2 = m[8] * m[15] - m[12] * m[11], c1 = m[8] * m[14] - m[12] * m[10], c0 = m[8] * m[13] - m[12] * m[9];
    const double id = 1.0 / (s0 * c5 - s1 * c4 + s2 * c3 + s3 * c2 - s4 * c1 + s5 * c0);
    double b[16];   // the inverse, row-major
    b[0] = (m[5] * c5 - m[6] * c4 + m[7] * c3) * id;   b[1] = (-m[1] * c5 + m[2] * c4 - m[3] * c3) * id;
    b[2] = (m[13] * s5 - m[14] * s4 + m[15] * s3) * id; b[3] = (-m[9] * s5 + m[10] * s4 - m[11] * s3) * id;
    b[4] = (-m[4] * c5 + m[6] * c2 - m[7] * c1) * id;  b[5] = (m[0] * c5 - m[2] * c2 + m[3] * c1) * id;
    b[6] = (-m[12] * s5 + m[14] * s2 - m[15] * s1) * id; b[7] = (m[8] * s5 - m[10] * s2 + m[11] * s1) * id;
    b[8] = (m[4] * c4 - m[5] * c2 + m[7] * c0) * id;   b[9] = (-m[0] * c4 + m[1] * c2 - m[3] * c0) * id;
    b[10] = (m[12] * s4 - m[13] * s2 + m[15] * s0) * id; b[11] = (-m[8] * s4 + m[9] * s2 - m[11] * s0) * id;
    b[12] = (-m[4] * c3 + m[5] * c1 - m[6] * c0) * id; b[13] = (m[0] * c3 - m[1] * c1 + m[2] * c0) * id;
    b[14] = (-m[12] * s3 + m[13] * s1 - m[14] * s0) * id; b[15] = (m[8] * s3 - m[9] * s1 + m[10] * s0) * id;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        double w[4];
#pragma unroll
        for (int r = 0; r < 4; r++) {
            w[r] = 0.0;
#pragma unroll
            for (int c = 0; c < 4; c++) w[r] += b[r * 4 + c] * (double)anchors[i * 4 + c];
        }
        double g6[2];
#pragma unroll
        for (int h = 0; h < 2; h++) {   // value 2 i + h of the six: itself, then sin / cos of 2^f times it (phase pi / 2 for cos)
            const int d = 2 * i + h;
            const double v = w[h] / w[3] / w[2];
            double g = (double)g_enc[d];
#pragma unroll
            for (int col = 0; col < 6; col++) {
                const double sc = (double)(1 << (col / 2));
                g += (double)g_enc[6 * (col + 1) + d] * cos(v * sc + (col % 2) * (3.141592653589793 / 2)) * sc;
            }
            g6[h] = g;
        }
        const double den = w[3] * w[2];
        double gw[4];
        gw[0] = g6[0] / den;
        gw[1] = g6[1] / den;
        const double num = -(g6[0] * w[0] + g6[1] * w[1]);
        gw[3] = num / (w[3] * den);
        gw[2] = num / (w[2] * den);
#pragma unroll
        for (int c = 0; c < 4; c++) {   // w = B a: dL/da = B^T dL/dw
            double acc = 0.0;
#pragma unroll
            for (int r = 0; r < 4; r++) acc += b[r * 4 + c] * gw[r];
            g_anchors[i * 4 + c] = (float)acc;
        }
    }
}

// ---- entry points ----------------------------------------------------------------------------------------------------------------
static int lzt_check(const lz_torso_train_params* p, const char* what) {
    LZ_REQUIRE(p, LZ_ERR_BAD_ARGUMENT, "%s: null lz_torso_train_params", what);
    const lz_torso_params& n = p->net;
    LZ_REQUIRE(n.deform_w0 && n.deform_w1 && n.deform_w2 && n.torso_w0 && n.torso_w1 && n.torso_w2 && n.emb && n.offsets && n.enc_anchor,
               LZ_ERR_BAD_ARGUMENT, "%s: incomplete lz_torso_params", what);
    LZ_REQUIRE(n.ind_dim == 0 || n.ind_dim == 8, LZ_ERR_BAD_ARGUMENT, "%s: ind_dim_torso must be 0 or 8 (the reference's default)", what);
    LZ_REQUIRE(n.ind_dim == 0 || n.ind_code, LZ_ERR_BAD_ARGUMENT, "%s: ind_code required when ind_dim > 0", what);
    LZ_REQUIRE(p->n_offsets == 17, LZ_ERR_BAD_ARGUMENT, "%s: the torso encoder has 16 levels (17 offsets), got %u", what, p->n_offsets);
    LZ_REQUIRE(n.gridtype <= 1, LZ_ERR_BAD_ARGUMENT, "%s: gridtype must be 0 (hash) or 1 (tiled)", what);
    LZ_REQUIRE(!n.density_grid || n.G >= 2, LZ_ERR_BAD_ARGUMENT, "%s: density grid needs G >= 2", what);
    return LZ_OK;
}

static LzTorsoTrainArgs lzt_train_args(const lz_torso_train_params* p) {
    LzTorsoTrainArgs t;
    t.a = lzt_args(p->net);
    t.thresh = p->density_thresh;
    t.bg = p->bg;
    t.bg_scalar = p->bg_scalar;
    t.mix = p->mix;
    return t;
}

extern "C" size_t lz_torso_train_workspace(void) { return lz_wg_workspace_bytes(LZTG_TILES); }

extern "C" int lz_torso_train_forward(const lz_torso_train_params* p, const float* bg_coords, uint32_t N, float* alpha, float* color,
                                      float* deform, lz_stream_t stream) {
    if (N == 0) return LZ_OK;
    LZ_REQUIRE(bg_coords && alpha && color, LZ_ERR_BAD_ARGUMENT, "torso_train_forward: null tensor");
    const int rc = lzt_check(p, "torso_train_forward");
    if (rc != LZ_OK) return rc;
    const LzTorsoTrainArgs t = lzt_train_args(p);
    uint32_t nwg = lz_div_up(N, 16 * (LZT_WG / 64));
    const uint32_t cap = (uint32_t)lz_cu_count() * 3u;   // lz_torso_forward's geometry
    if (nwg > cap) nwg = cap;
    hipStream_t st = lz_st(stream);
    if (p->net.ind_dim == 8) hipLaunchKernelGGL((lz_k_torso_train_forward<8>), dim3(nwg), dim3(LZT_WG), 0, st, t, bg_coords, N, alpha, color, deform);
    else hipLaunchKernelGGL((lz_k_torso_train_forward<0>), dim3(nwg), dim3(LZT_WG), 0, st, t, bg_coords, N, alpha, color, deform);
    LZ_CHECK_LAUNCH("torso_train_forward");
    return LZ_OK;
}

// both backward entries: denc / u non-null selects the rows-emitting kernel, which leaves grads->g_emb alone
template <int IND, bool ROWS>
static void lzt_launch_backward(const LzTorsoTrainArgs& t, const lz_torso_params& net, uint32_t nwg, const float* bg_coords, uint32_t N,
                                const float* g_alpha, const float* g_color, const float* g_deform, float* g_emb, float* part, float* denc,
                                float* u, const LzTorsoGradOut& G, hipStream_t st) {
    hipLaunchKernelGGL((lz_k_torso_train_backward<IND, ROWS>), dim3(nwg), dim3(LZT_WG), 0, st, t, bg_coords, N, g_alpha, g_color, g_deform, g_emb,
                       part, denc, u);
    hipLaunchKernelGGL((lz_k_torso_train_combine<IND>), dim3(LZTC_BLOCKS + 1), dim3(256), 0, st, part, nwg, net, G);
}

static int lzt_backward(const char* what, const lz_torso_train_params* p, const float* bg_coords, uint32_t N, const float* g_alpha,
                        const float* g_color, const float* g_deform, const lz_torso_grads* grads, void* workspace, float* denc, float* u,
                        bool rows, lz_stream_t stream) {
    LZ_REQUIRE(bg_coords && grads && workspace && (!rows || (denc && u)), LZ_ERR_BAD_ARGUMENT, "%s: null tensor", what);
    const int rc = lzt_check(p, what);
    if (rc != LZ_OK) return rc;
    LZ_REQUIRE(grads->g_deform_w0 && grads->g_deform_w1 && grads->g_deform_w2 && grads->g_torso_w0 && grads->g_torso_w1 && grads->g_torso_w2 &&
                   (rows || grads->g_emb) && grads->g_enc_anchor && (p->net.ind_dim == 0 || grads->g_ind_code),
               LZ_ERR_BAD_ARGUMENT, "%s: incomplete lz_torso_grads", what);
    const LzTorsoTrainArgs t = lzt_train_args(p);
    // one workgroup per CU (the staging rows and the 28 accumulator tiles fill the LDS and half the register file), at least four
    // slices per wave before the grid is full
    const uint32_t nwg = lz_wg_grid(N, LZT_WG / 64, 1);
    float* part = static_cast<float*>(workspace);
    LzTorsoGradOut G{grads->g_deform_w0, grads->g_deform_w1, grads->g_deform_w2, grads->g_torso_w0, grads->g_torso_w1, grads->g_torso_w2,
                     grads->g_enc_anchor, grads->g_ind_code};
    hipStream_t st = lz_st(stream);
    const bool ind = p->net.ind_dim == 8;
    if (rows) {
        if (ind) lzt_launch_backward<8, true>(t, p->net, nwg, bg_coords, N, g_alpha, g_color, g_deform, nullptr, part, denc, u, G, st);
        else lzt_launch_backward<0, true>(t, p->net, nwg, bg_coords, N, g_alpha, g_color, g_deform, nullptr, part, denc, u, G, st);
    } else {
        if (ind) lzt_launch_backward<8, false>(t, p->net, nwg, bg_coords, N, g_alpha, g_color, g_deform, grads->g_emb, part, nullptr, nullptr, G, st);
        else lzt_launch_backward<0, false>(t, p->net, nwg, bg_coords, N, g_alpha, g_color, g_deform, grads->g_emb, part, nullptr, nullptr, G, st);
    }
    LZ_CHECK_LAUNCH(what);
    return LZ_OK;
}

extern "C" int lz_torso_train_backward(const lz_torso_train_params* p, const float* bg_coords, uint32_t N, const float* g_alpha,
                                       const float* g_color, const float* g_deform, const lz_torso_grads* grads, void* workspace,
                                       lz_stream_t stream) {
    if (N == 0) return LZ_OK;
    return lzt_backward("torso_train_backward", p, bg_coords, N, g_alpha, g_color, g_deform, grads, workspace, nullptr, nullptr, false, stream);
}

extern "C" int lz_torso_train_backward_rows(const lz_torso_train_params* p, const float* bg_coords, uint32_t N, const float* g_alpha,
                                            const float* g_color, const float* g_deform, const lz_torso_grads* grads, void* workspace,
                                            float* denc, float* u, lz_stream_t stream) {
    if (N == 0) return LZ_OK;
    return lzt_backward("torso_train_backward_rows", p, bg_coords, N, g_alpha, g_color, g_deform, grads, workspace, denc, u, true, stream);
}

extern "C" int lz_torso_anchor_encode_backward(const float* pose, const float* anchor_points, const float* g_enc_anchor, uint32_t J,
                                               float* g_anchor_points, lz_stream_t stream) {
    if (J == 0) return LZ_OK;
    LZ_REQUIRE(pose && anchor_points && g_enc_anchor && g_anchor_points, LZ_ERR_BAD_ARGUMENT, "torso_anchor_encode_backward: null tensor");
    LZ_REQUIRE(J == 3, LZ_ERR_BAD_ARGUMENT, "torso_anchor_encode_backward: the torso has 3 anchor points (network.py:158), got %u", J);
    hipLaunchKernelGGL(lz_k_torso_anchor_encode_backward, dim3(1), dim3(64), 0, lz_st(stream), pose, anchor_points, g_enc_anchor, g_anchor_points);
    LZ_CHECK_LAUNCH("torso_anchor_encode_backward");
    return LZ_OK;
}
