// lz_torso.hip -- the torso branch of the frame: NeRFRenderer.run_torso (nerf_triplane/renderer.py:572-631)
// + NeRFNetwork.forward_torso (nerf_triplane/network.py:170-205) as ONE kernel, one lane per pixel.
//
// Reference per pixel: 2-D occupancy lookup (F.grid_sample, bilinear, align_corners) -> boolean mask -> for the masked pixels:
// shrink, frequency-encode (2 -> 34), cat with the frame-constant anchor encoding (42) and individual code, deform MLP
// (-> 32 -> 32 -> 2), x + dx clamped, tiled-grid encode (D = 2, L = 16, C = 2 -> 32), torso MLP (-> 32 -> 32 -> 4), sigmoids;
// scatter back into zero-filled [N,1] / [N,3] tensors, then mix with the background.  ~25 launches, a mask.any() sync and two
// boolean-mask gathers / scatters per frame.  Here nothing is materialised: a lane owns a pixel from lookup to alpha/colour.
//
// Arithmetic (restated bit for bit by oracle/torso.py): everything is an explicit f32 fma chain on the VALU (the MLPs are
// 5.4 kMAC per pixel: not worth the matrix cores at 2.6e5 pixels per frame).  Chain order of the two first layers: the
// frame-constant inputs (anchor encoding, individual code) first -- their partial sums are computed once per workgroup -- then
// the per-pixel inputs in natural order; all other layers natural order.
#include "lz_torso_net.h"

template <int IND>
__global__ void __launch_bounds__(LZT_WG)
lz_k_torso_forward(LzTorsoArgs A, const float* __restrict__ bg_coords, uint32_t N, float* __restrict__ alpha_out,
                   float* __restrict__ color_out, float* __restrict__ deform_out) {
    constexpr int H = LZ_TORSO_HID;
    __shared__ float wl[LZT_FRAGS * 64];
    __shared__ __align__(16) float cd[H], ct[H];
    const lz_torso_params& P = A.p;
    lzt_setup<IND>(P, wl, cd, ct);
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int s = lane & 15, q = lane >> 4;
    const uint32_t n_slices = (N + 15) / 16, stride = gridDim.x * (LZT_WG / 64);
    for (uint32_t slice = blockIdx.x * (LZT_WG / 64) + wave; slice < n_slices; slice += stride) {
        const uint32_t n_raw = slice * 16 + s;
        const bool valid = n_raw < N;
        const uint32_t n = valid ? n_raw : N - 1;     // clamped lanes compute a real pixel again and store nothing
        const float bx = bg_coords[(size_t)n * 2], by = bg_coords[(size_t)n * 2 + 1];
        const bool masked = P.density_grid ? lzt_occupancy(P.density_grid, P.G, bx, by) > P.density_thresh : true;
        if (!__ballot(masked && valid)) {     // wave-uniform: nothing to evaluate in this slice (renderer.py:609-610: zeros)
            if (q == 0 && valid) {
                alpha_out[n] = 0.0f;
                color_out[(size_t)n * 3] = 0.0f; color_out[(size_t)n * 3 + 1] = 0.0f; color_out[(size_t)n * 3 + 2] = 0.0f;
                if (deform_out) { deform_out[(size_t)n * 2] = 0.0f; deform_out[(size_t)n * 2 + 1] = 0.0f; }
            }
            continue;
        }
        LztFwd f;
        lzt_forward<IND>(A, wl, cd, ct, lane, bx, by, f);
        if (q == 0 && valid) {
            alpha_out[n] = masked ? lzt_out(f.o[0]) : 0.0f;
            color_out[(size_t)n * 3] = masked ? lzt_out(f.o[1]) : 0.0f;
            color_out[(size_t)n * 3 + 1] = masked ? lzt_out(f.o[2]) : 0.0f;
            color_out[(size_t)n * 3 + 2] = masked ? lzt_out(f.o[3]) : 0.0f;
            if (deform_out) { deform_out[(size_t)n * 2] = masked ? f.dx[0] : 0.0f; deform_out[(size_t)n * 2 + 1] = masked ? f.dx[1] : 0.0f; }
        }
    }
}

// The same forward with the background mix of run_torso (renderer.py:621) in the store: the colour written is
// fl(fl(c a) + fl(b fl(1 - a))) per channel, FusedTorso.mix_background's bits, instead of four element-wise launches over the frame.
// A pixel the occupancy mask drops has a = c = 0 and goes through the same formula (it gives b; +0 for b = -0, as torch does).
__device__ __forceinline__ float lzt_mix(float c, float a, float b) {
    const float ca = c * a, ia = 1.0f - a;
    const float bi = b * ia;
    return ca + bi;
}
template <int IND>
__global__ void __launch_bounds__(LZT_WG)
lz_k_torso_mixed(LzTorsoArgs A, const float* __restrict__ bg_coords, uint32_t N, const float* __restrict__ bg, float bg_scalar,
                         float* __restrict__ alpha_out, float* __restrict__ color_out, float* __restrict__ deform_out) {
    constexpr int H = LZ_TORSO_HID;
    __shared__ float wl[LZT_FRAGS * 64];
    __shared__ __align__(16) float cd[H], ct[H];
    const lz_torso_params& P = A.p;
    lzt_setup<IND>(P, wl, cd, ct);
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int s = lane & 15, q = lane >> 4;
    const uint32_t n_slices = (N + 15) / 16, stride = gridDim.x * (LZT_WG / 64);
    for (uint32_t slice = blockIdx.x * (LZT_WG / 64) + wave; slice < n_slices; slice += stride) {
        const uint32_t n_raw = slice * 16 + s;
        const bool valid = n_raw < N;
        const uint32_t n = valid ? n_raw : N - 1;
        const float bx = bg_coords[(size_t)n * 2], by = bg_coords[(size_t)n * 2 + 1];
        const bool masked = P.density_grid ? lzt_occupancy(P.density_grid, P.G, bx, by) > P.density_thresh : true;
        float a = 0.0f, c[3] = {0.0f, 0.0f, 0.0f}, dx[2] = {0.0f, 0.0f};
        if (__ballot(masked && valid)) {      // wave-uniform, as in lz_k_torso_forward
            LztFwd f;
            lzt_forward<IND>(A, wl, cd, ct, lane, bx, by, f);
            if (masked) {
                a = lzt_out(f.o[0]);
                c[0] = lzt_out(f.o[1]); c[1] = lzt_out(f.o[2]); c[2] = lzt_out(f.o[3]);
                dx[0] = f.dx[0]; dx[1] = f.dx[1];
            }
        }
        if (q == 0 && valid) {
            alpha_out[n] = a;
#pragma unroll
            for (int ch = 0; ch < 3; ch++) color_out[(size_t)n * 3 + ch] = lzt_mix(c[ch], a, bg ? bg[(size_t)n * 3 + ch] : bg_scalar);
            if (deform_out) { deform_out[(size_t)n * 2] = dx[0]; deform_out[(size_t)n * 2 + 1] = dx[1]; }
        }
    }
}

// ---- the frame-constant anchor encoding (network.py:179-183) as one launch -------------------------------------------------------------
// wrapped = anchor_points @ inverse(pose^T): row i is pose^-1 . a_i; (x / w / z, y / w / z) per anchor; frequency encoding of the 6 values,
// degree 3 (lz_k_freq_forward's formula and order).  The 4 x 4 inverse is a Gauss-Jordan elimination with partial pivoting in double by
// one thread -- torch runs an LU factorisation in f32 through a dozen library launches for it; the results agree to a few f32 ulp.
__global__ void __launch_bounds__(64) lz_k_torso_anchor_encode(const float* __restrict__ pose, const float* __restrict__ anchors, float* __restrict__ enc) {
    __shared__ float w6[6];
    if (threadIdx.x == 0) {
        double a[4][8];
        for (int r = 0; r < 4; r++)
            for (int c = 0; c < 4; c++) { a[r][c] = (double)pose[r * 4 + c]; a[r][4 + c] = r == c ? 1.0 : 0.0; }
        for (int col = 0; col < 4; col++) {
            int piv = col;
            for (int r = col + 1; r < 4; r++)
                if (fabs(a[r][col]) > fabs(a[piv][col])) piv = r;
            if (piv != col)
                for (int c = 0; c < 8; c++) { const double t = a[col][c]; a[col][c] = a[piv][c]; a[piv][c] = t; }
            const double inv = 1.0 / a[col][col];
            for (int c = 0; c < 8; c++) a[col][c] *= inv;
            for (int r = 0; r < 4; r++) {
                if (r == col) continue;
                const double f = a[r][col];
                for (int c = 0; c < 8; c++) a[r][c] -= f * a[col][c];
            }
        }
        for (int i = 0; i < 3; i++) {
            double w[4];
            for (int r = 0; r < 4; r++) {
                w[r] = 0.0;
                for (int c = 0; c < 4; c++) w[r] += a[r][4 + c] * (double)anchors[i * 4 + c];
            }
            w6[2 * i] = (float)(w[0] / w[3] / w[2]);
            w6[2 * i + 1] = (float)(w[1] / w[3] / w[2]);
        }
    }
    __syncthreads();
    const uint32_t c = threadIdx.x;
    if (c < 42) {
        float v;
        if (c < 6) v = w6[c];
        else {
            const uint32_t col = c / 6 - 1, d = c % 6, freq = col / 2;
            const float phase = (float)(col % 2) * (3.141592653589793f / 2);
            v = lz_sinf(lz_scalbnf(w6[d], (int)freq) + phase);
        }
        enc[c] = v;
    }
}

// The anchor encodings of a clip's K poses in one launch: workgroup k is lz_k_torso_anchor_encode on pose k -- the same elimination, the
// same operations on the same values in the same order, so the same bits.  Only the row exchange is written differently: the pivot row
// is swapped in by a select per candidate row instead of an index into the local array, every loop has a constant trip count, and the
// 4 x 8 doubles stay in registers (no scratch).
__global__ void __launch_bounds__(64)
lz_k_torso_anchor_encode_batch(const float* __restrict__ poses, const float* __restrict__ anchors, float* __restrict__ enc) {
    __shared__ float w6[6];
    const float* pose = poses + (size_t)blockIdx.x * 16;
    if (threadIdx.x == 0) {
        double a[4][8];
#pragma unroll
        for (int r = 0; r < 4; r++)
#pragma unroll
            for (int c = 0; c < 4; c++) { a[r][c] = (double)pose[r * 4 + c]; a[r][4 + c] = r == c ? 1.0 : 0.0; }
#pragma unroll
        for (int col = 0; col < 4; col++) {
            int piv = col;
            double best = fabs(a[col][col]);
#pragma unroll
            for (int r = col + 1; r < 4; r++)
                if (fabs(a[r][col]) > best) { best = fabs(a[r][col]); piv = r; }
#pragma unroll
            for (int r = col + 1; r < 4; r++) {
                const bool sw = piv == r;
#pragma unroll
                for (int c = 0; c < 8; c++) {
                    const double x = a[col][c], y = a[r][c];
                    a[col][c] = sw ? y : x;
                    a[r][c] = sw ? x : y;
                }
            }
            const double inv = 1.0 / a[col][col];
#pragma unroll
            for (int c = 0; c < 8; c++) a[col][c] *= inv;
#pragma unroll
            for (int r = 0; r < 4; r++) {
                if (r == col) continue;
                const double f = a[r][col];
#pragma unroll
                for (int c = 0; c < 8; c++) a[r][c] -= f * a[col][c];
            }
        }
#pragma unroll
        for (int i = 0; i < 3; i++) {
            double w[4];
#pragma unroll
            for (int r = 0; r < 4; r++) {
                w[r] = 0.0;
#pragma unroll
                for (int c = 0; c < 4; c++) w[r] += a[r][4 + c] * (double)anchors[i * 4 + c];
            }
            w6[2 * i] = (float)(w[0] / w[3] / w[2]);
            w6[2 * i + 1] = (float)(w[1] / w[3] / w[2]);
        }
    }
    __syncthreads();
    const uint32_t c = threadIdx.x;
    if (c < 42) {
        float v;
        if (c < 6) v = w6[c];
        else {
            const uint32_t col = c / 6 - 1, d = c % 6, freq = col / 2;
            const float phase = (float)(col % 2) * (3.141592653589793f / 2);
            v = lz_sinf(lz_scalbnf(w6[d], (int)freq) + phase);
        }
        enc[(size_t)blockIdx.x * 42 + c] = v;
    }
}

extern "C" int lz_torso_anchor_encode_batch(const float* poses, const float* anchor_points, float* enc_anchor, uint32_t K, lz_stream_t stream) {
    if (K == 0) return LZ_OK;
    LZ_REQUIRE(poses && anchor_points && enc_anchor, LZ_ERR_BAD_ARGUMENT, "torso_anchor_encode_batch: null tensor");
    hipLaunchKernelGGL(lz_k_torso_anchor_encode_batch, dim3(K), dim3(64), 0, lz_st(stream), poses, anchor_points, enc_anchor);
    LZ_CHECK_LAUNCH("torso_anchor_encode_batch");
    return LZ_OK;
}

extern "C" int lz_torso_anchor_encode(const float* pose, const float* anchor_points, float* enc_anchor, lz_stream_t stream) {
    LZ_REQUIRE(pose && anchor_points && enc_anchor, LZ_ERR_BAD_ARGUMENT, "torso_anchor_encode: null tensor");
    hipLaunchKernelGGL(lz_k_torso_anchor_encode, dim3(1), dim3(64), 0, lz_st(stream), pose, anchor_points, enc_anchor);
    LZ_CHECK_LAUNCH("torso_anchor_encode");
    return LZ_OK;
}

extern "C" int lz_torso_forward(const lz_torso_params* p, const float* bg_coords, uint32_t N, float* alpha, float* color, float* deform,
                                lz_stream_t stream) {
    if (N == 0) return LZ_OK;
    LZ_REQUIRE(p && bg_coords && alpha && color, LZ_ERR_BAD_ARGUMENT, "torso_forward: null tensor");
    LZ_REQUIRE(p->deform_w0 && p->deform_w1 && p->deform_w2 && p->torso_w0 && p->torso_w1 && p->torso_w2 && p->emb && p->offsets &&
                   p->enc_anchor, LZ_ERR_BAD_ARGUMENT, "torso_forward: incomplete lz_torso_params");
    LZ_REQUIRE(p->ind_dim == 0 || p->ind_code, LZ_ERR_BAD_ARGUMENT, "torso_forward: ind_code required when ind_dim > 0");
    const LzTorsoArgs a = lzt_args(*p);
    // four waves per workgroup, a wave walks 16-pixel slices with the grid's stride; the weights are packed into LDS once per workgroup
    uint32_t nwg = lz_div_up(N, 16 * (LZT_WG / 64));
    const uint32_t cap = (uint32_t)lz_cu_count() * 3u;     // three workgroups per CU are resident (126 registers: three waves per SIMD)
    if (nwg > cap) nwg = cap;
    const dim3 grid(nwg), block(LZT_WG);
    hipStream_t st = lz_st(stream);
    switch (p->ind_dim) {
        case 0: hipLaunchKernelGGL((lz_k_torso_forward<0>), grid, block, 0, st, a, bg_coords, N, alpha, color, deform); break;
        case 8: hipLaunchKernelGGL((lz_k_torso_forward<8>), grid, block, 0, st, a, bg_coords, N, alpha, color, deform); break;
        default: lz_set_error("torso_forward: ind_dim_torso must be 0 or 8 (the reference's default)"); return LZ_ERR_UNSUPPORTED;
    }
    LZ_CHECK_LAUNCH("torso_forward");
    return LZ_OK;
}

extern "C" int lz_torso_forward_mixed(const lz_torso_params* p, const float* bg_coords, uint32_t N, const float* bg, float bg_scalar, float* alpha,
                                      float* color_mixed, float* deform, lz_stream_t stream) {
    if (N == 0) return LZ_OK;
    LZ_REQUIRE(p && bg_coords && alpha && color_mixed, LZ_ERR_BAD_ARGUMENT, "torso_forward_mixed: null tensor");
    LZ_REQUIRE(p->deform_w0 && p->deform_w1 && p->deform_w2 && p->torso_w0 && p->torso_w1 && p->torso_w2 && p->emb && p->offsets &&
                   p->enc_anchor, LZ_ERR_BAD_ARGUMENT, "torso_forward_mixed: incomplete lz_torso_params");
    LZ_REQUIRE(p->ind_dim == 0 || p->ind_code, LZ_ERR_BAD_ARGUMENT, "torso_forward_mixed: ind_code required when ind_dim > 0");
    const LzTorsoArgs a = lzt_args(*p);
    uint32_t nwg = lz_div_up(N, 16 * (LZT_WG / 64));       // the launch geometry of lz_torso_forward
    const uint32_t cap = (uint32_t)lz_cu_count() * 3u;
    if (nwg > cap) nwg = cap;
    const dim3 grid(nwg), block(LZT_WG);
    hipStream_t st = lz_st(stream);
    switch (p->ind_dim) {
        case 0: hipLaunchKernelGGL((lz_k_torso_mixed<0>), grid, block, 0, st, a, bg_coords, N, bg, bg_scalar, alpha, color_mixed, deform); break;
        case 8: hipLaunchKernelGGL((lz_k_torso_mixed<8>), grid, block, 0, st, a, bg_coords, N, bg, bg_scalar, alpha, color_mixed, deform); break;
        default: lz_set_error("torso_forward_mixed: ind_dim_torso must be 0 or 8 (the reference's default)"); return LZ_ERR_UNSUPPORTED;
    }
    LZ_CHECK_LAUNCH("torso_forward_mixed");
    return LZ_OK;
}
