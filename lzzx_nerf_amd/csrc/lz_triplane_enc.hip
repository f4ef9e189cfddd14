// lz_triplane_enc.hip -- the triplane position encoder as ONE operator: xyz [B, 3] -> [B, 3 L] (xy | yz | xz), with its backward.
//
// Replaces NeRFNetwork.encode_x (nerf_triplane/network.py:208-223: split_xyz, three GridEncoder calls, torch.cat) and, per plane, the
// Python side of GridEncoder.forward / _grid_encode (gridencoder/grid.py:18-84) for callers that keep the reference's torch network.
// The arithmetic per (sample, plane, level) is that of lz_grid.hip for D = 2, C = 1, f32 tables, hash gridtype, align_corners off,
// through the same helpers (lz_grid_common.h), so the result is the three-operator path's bits.
//
// MI355X design notes
//   * forward: one lane per sample, levels in a loop, the three planes inside it.  A level's record is wave-uniform (scalar registers),
//     the cell of (x, y, z) in that level is computed once and shared by the planes that use a coordinate.  A wave's 64 samples own ONE
//     contiguous span of 64 x 3 L x 4 bytes of the output (9 216 bytes for L = 12, always a multiple of 256): the features go through a
//     per-wave LDS tile (row pitch odd, so the writes are conflict-free) and leave as 16-byte stores, 1 KB per wave instruction, whole
//     128-byte lines.  The stand-alone plane encoder writes 4 bytes per lane, 48 bytes apart.
//   * backward: one workgroup per (plane, level, sample chunk), all 3 L of them in one launch; the gradient is read in place at row
//     pitch 3 L.  Large batches accumulate in the 64-bit fixed-point LDS table of lz_k_grid_backward_lds_fx (same scale rule) and
//     flush with contiguous float atomics; small ones (and levels that do not fit LDS) add with global float atomics.
//   * the input gradient is a kernel of its own over the three per-plane Jacobians.
#include "lz_common.h"
#include "lzzx_detmath.h"
#include "lz_grid_common.h"
#include <math.h>

#define LZ_TRI_MAX_LEVELS 16u
#define LZ_TRI_WAVES 4u               // waves (64-sample tiles) per forward workgroup
#define LZ_TRI_FX_LDS_BYTES 131072    // the backward's accumulator: 8 bytes per entry of one level
#define LZ_TRI_LDS_MIN_B 16384u       // batches from this size on take the LDS accumulator (as GridEncoder's backward does)

struct LzTriTables {
    const float* t[3];   // xy, yz, xz
};
struct LzTriGrads {
    float* t[3];
};

// (x + bound) / (2 bound) is lz_map01 (lz_common.h): what GridEncoder.forward computes on the device, measured to be the add followed by a
// multiplication with inv2b = 1.0f / (2 bound), which the host forms.

// The plane's two coordinates: xy = (x, y), yz = (y, z), xz = (x, z) (network.py:210-212)
__device__ __forceinline__ constexpr uint32_t lz_tri_d0(uint32_t plane) { return plane == 1u ? 1u : 0u; }
__device__ __forceinline__ constexpr uint32_t lz_tri_d1(uint32_t plane) { return plane == 0u ? 1u : 2u; }

template <bool JAC>
__global__ void __launch_bounds__(64 * LZ_TRI_WAVES)
lz_k_triplane_encode(const float* __restrict__ xyz, LzTriTables emb, const int* __restrict__ offsets, float* __restrict__ out,
                     float* __restrict__ dy_dx, uint32_t B, uint32_t L, LzGridLevels lv, float bound, float inv2b) {
    extern __shared__ __align__(16) float lz_tri_tile[];
    const uint32_t W = 3u * L, Wp = W | 1u;                    // LDS row pitch odd: lane s writes bank (s Wp + k) % 32, all different
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    float* tile = lz_tri_tile + wave * 64u * Wp;
    const uint32_t b0 = (blockIdx.x * LZ_TRI_WAVES + wave) * 64u;
    const uint32_t n = b0 < B ? (B - b0 < 64u ? B - b0 : 64u) : 0u;   // rows of this wave; wave-uniform
    const uint32_t b = b0 + lane;
    if (n != 0u) {
        float c01[3];
        bool oobc[3];
#pragma unroll
        for (uint32_t d = 0; d < 3; d++) {
            const float v = lane < n ? xyz[(size_t)b * 3 + d] : 0.0f;   // idle lanes of the last wave gather at the centre and store nothing
            c01[d] = lz_map01(v, bound, inv2b);
            oobc[d] = c01[d] < 0 || c01[d] > 1;
        }
#pragma unroll 2
        for (uint32_t level = 0; level < L; level++) {
            const LzGridLevel lvl = lz_grid_level<2>(offsets, lv, level, 0u, false);
            // per coordinate the arithmetic of lz_grid_cell<2>: clamped for addressing only, the feature is zeroed by a select below
            const LzGridCell<3> c3 = lz_grid_cell<3, true>(c01, lvl.scale, false);
#pragma unroll
            for (uint32_t plane = 0; plane < 3; plane++) {
                const uint32_t d0 = lz_tri_d0(plane), d1 = lz_tri_d1(plane);
                LzGridCell<2> cell;
                cell.pg[0] = c3.pg[d0], cell.pg[1] = c3.pg[d1];
                cell.pos[0] = c3.pos[d0], cell.pos[1] = c3.pos[d1];
                cell.oob = oobc[d0] || oobc[d1];           // gridencoder.cu:98-122
                const float* g = emb.t[plane] + lvl.off0;
                uint32_t term[2][2];
                lz_grid_terms<2>(lvl, cell, false, term);
                float res = 0.0f;
#pragma unroll
                for (uint32_t idx = 0; idx < 4; idx++) {
                    const float w = lz_grid_weight<2>(cell, idx);
                    const uint32_t index = lz_grid_corner_index<2>(lvl, cell, term, idx, 1u, 0u, false);
                    res = lz_fmaf(w, g[index], res);
                }
                tile[lane * Wp + plane * L + level] = cell.oob ? 0.0f : res;
                if constexpr (JAC) {   // gridencoder.cu:179-222, [plane][B, L, 2]
                    float2 jac;
#pragma unroll
                    for (uint32_t gd = 0; gd < 2; gd++) {
                        const uint32_t lo = 0u, hi = 1u << (1u - gd);          // the two corners that vary in the other dimension
                        float rg = 0.0f;
#pragma unroll
                        for (uint32_t k = 0; k < 2; k++) {
                            const uint32_t cl = k ? hi : lo;
                            const float w = lz_grid_weight<2>(cell, cl, lvl.scale, gd);
                            const uint32_t il = lz_grid_corner_index<2>(lvl, cell, term, cl, 1u, 0u, false);
                            const uint32_t ir = lz_grid_corner_index<2>(lvl, cell, term, cl | (1u << gd), 1u, 0u, false);
                            rg = lz_fmaf(w, g[ir] - g[il], rg);
                        }
                        if (gd == 0) jac.x = cell.oob ? 0.0f : rg;
                        else jac.y = cell.oob ? 0.0f : rg;
                    }
                    if (lane < n) *reinterpret_cast<float2*>(dy_dx + (((size_t)plane * B + b) * L + level) * 2) = jac;
                }
            }
        }
    }
    __syncthreads();
    if (n == 0u) return;
    // The wave's rows are n W consecutive floats of `out`, starting 16-byte aligned (64 W floats per full wave).  Lane l takes the
    // 16-byte pieces l, l + 64, ...: flat element e = 4 (l + 64 j) is (row e / W, column e % W), advanced without a division.
    const uint32_t total = n * W;
    float* gout = out + (size_t)b0 * W;
    uint32_t e = 4u * lane, r = e / W, col = e - r * W;
    const uint32_t dr = 256u / W, dc = 256u - dr * W;
    for (; e < total; e += 256u) {
        float v[4];
        uint32_t rr = r, cc = col;
#pragma unroll
        for (uint32_t i = 0; i < 4; i++) {          // e + i < 64 W: inside the tile even where it is past `total`
            v[i] = tile[rr * Wp + cc];
            if (++cc == W) { cc = 0u; ++rr; }
        }
        if (e + 4u <= total) {
            *reinterpret_cast<float4*>(gout + e) = make_float4(v[0], v[1], v[2], v[3]);
        } else {                                    // the last piece of a partial wave when n W is no multiple of 4: never past row B
#pragma unroll
            for (uint32_t i = 0; i < 4; i++)
                if (e + i < total) gout[e + i] = v[i];
        }
        col += dc, r += dr;
        if (col >= W) { col -= W; ++r; }
    }
}

// ---- backward: table gradients of all 3 L (plane, level) pairs in one launch ----------------------------------------------------------
// add(entry, w * g) for the four corners of sample b in (plane, level); out-of-range samples contribute nothing (gridencoder.cu:262-266)
template <typename Add>
__device__ __forceinline__ void lz_tri_sample_terms(const float* __restrict__ xyz, uint32_t b, uint32_t d0, uint32_t d1, float bound,
                                                    float inv2b, const LzGridLevel& lvl, float g, Add&& add) {
    const float x[2] = {lz_map01(xyz[(size_t)b * 3 + d0], bound, inv2b), lz_map01(xyz[(size_t)b * 3 + d1], bound, inv2b)};
    const LzGridCell<2> cell = lz_grid_cell<2, false>(x, lvl.scale, false);
    if (cell.oob) return;
    uint32_t term[2][2];
    lz_grid_terms<2>(lvl, cell, false, term);
#pragma unroll
    for (uint32_t idx = 0; idx < 4; idx++) {
        const float w = lz_grid_weight<2>(cell, idx);
        add(lz_grid_corner_index<2>(lvl, cell, term, idx, 1u, 0u, false), w * g);
    }
}

__device__ __forceinline__ float lz_tri_abs_nan_inf(float g) {   // |g| with NaN mapped to +inf (fmaxf drops NaN operands)
    const float a = fabsf(g);
    return a == a ? a : INFINITY;
}

__global__ void __launch_bounds__(1024)
lz_k_triplane_encode_backward(const float* __restrict__ grad, const float* __restrict__ xyz, const int* __restrict__ offsets, LzTriGrads gt,
                              uint32_t B, uint32_t L, LzGridLevels lv, float bound, float inv2b, uint32_t chunk, uint32_t use_lds) {
    extern __shared__ __align__(16) unsigned long long lz_tri_acc64[];
    __shared__ float wmax[16];
    const uint32_t W = 3u * L;
    const uint32_t pl = blockIdx.x % W, c = blockIdx.x / W;
    const uint32_t plane = pl / L, level = pl - plane * L;
    const uint32_t d0 = lz_tri_d0(plane), d1 = lz_tri_d1(plane);
    const LzGridLevel lvl = lz_grid_level<2>(offsets, lv, level, 0u, false);
    const uint32_t b0 = c * chunk, b1 = (B - b0 < chunk) ? B : b0 + chunk;
    float* gg = (plane == 0u ? gt.t[0] : (plane == 1u ? gt.t[1] : gt.t[2])) + lvl.off0;
    const float* gcol = grad + pl;                        // this (plane, level)'s column of the [B, 3 L] gradient
    const uint32_t n = lvl.hs;
    auto scatter_global = [&]() {
        for (uint32_t b = b0 + threadIdx.x; b < b1; b += blockDim.x)
            lz_tri_sample_terms(xyz, b, d0, d1, bound, inv2b, lvl, gcol[(size_t)b * W], [&](uint32_t index, float p) { atomicAdd(gg + index, p); });
    };
    if (!use_lds || (size_t)n * 8 > LZ_TRI_FX_LDS_BYTES) {   // workgroup-uniform
        scatter_global();
        return;
    }
    // 64-bit fixed-point accumulation in LDS, the design (and the scale rule) of lz_k_grid_backward_lds_fx: largest |grad| of the chunk,
    // a power-of-two scale with headroom for 4 * chunk additions in 51 bits, integer LDS atomics, one contiguous float-atomic flush
    float gm = 0.0f;
    for (uint32_t b = b0 + threadIdx.x; b < b1; b += blockDim.x) gm = fmaxf(gm, lz_tri_abs_nan_inf(gcol[(size_t)b * W]));
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) gm = fmaxf(gm, __shfl_xor(gm, off, 64));
    if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = gm;
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) lz_tri_acc64[i] = 0ull;
    __syncthreads();
    gm = wmax[0];
    for (uint32_t w = 1; w < (blockDim.x >> 6); w++) gm = fmaxf(gm, wmax[w]);
    if (!(gm > 0.0f) || !(gm < INFINITY)) {   // nothing to add, or non-finite gradients: those keep the float path's semantics
        if (gm > 0.0f) scatter_global();
        return;
    }
    int ex;
    (void)frexpf(gm, &ex);                                    // gm < 2^ex
    int hb = 2;
    while ((1u << hb) < (b1 - b0) * 4u) hb++;
    int e = 51 - hb - ex;
    e = e > 100 ? 100 : (e < -100 ? -100 : e);
    const float inv = ldexpf(1.0f, -e);
    const double fxd = (double)ldexpf(1.0f, e);
    // The fixed-point grid has steps of 2^-e = 2^(hb + ex - 51).  A term of at least 2^(ex - 24) is rounded to it with a relative error of
    // at most 2^(hb - 28) <= chunk 2^-25, an eighth of what reordering n = 4 B float additions may cost (n 2^-24); a smaller term -- a
    // corner weight near zero, about one term in 10^7 -- would lose more than that, so it skips the table and goes out as a float atomic.
    const float tiny = ldexpf(1.0f, ex - 24);
    for (uint32_t b = b0 + threadIdx.x; b < b1; b += blockDim.x)
        lz_tri_sample_terms(xyz, b, d0, d1, bound, inv2b, lvl, gcol[(size_t)b * W], [&](uint32_t index, float p) {
            if (fabsf(p) < tiny) {
                if (p != 0.0f) atomicAdd(gg + index, p);
                return;
            }
            // round(p * 2^e) through the double addition's own rounding (|p * 2^e| < 2^51), see lz_k_grid_backward_lds_fx
            const double t = __builtin_fma((double)p, fxd, 6755399441055744.0);
            __hip_atomic_fetch_add(lz_tri_acc64 + index, (unsigned long long)(__double_as_longlong(t) - 0x4338000000000000ll), __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_WORKGROUP);
        });
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
        const long long a = (long long)lz_tri_acc64[i];
        if (a != 0) atomicAdd(gg + i, __ll2float_rn(a) * inv);
    }
}

// d_xyz from the three per-plane Jacobians.  Per plane the sum is kernel_input_backward's (gridencoder.cu:316-342: fma over the levels in
// order), times 1 / (2 bound) -- the backward of grid.py:143 -- and the planes are added left to right:
// d_x = g_xy[0] + g_xz[0], d_y = g_xy[1] + g_yz[0], d_z = g_yz[1] + g_xz[1]
__global__ void __launch_bounds__(256)
lz_k_triplane_input_backward(const float* __restrict__ grad, const float* __restrict__ dy_dx, float* __restrict__ grad_xyz, uint32_t B,
                             uint32_t L, float inv2b) {
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const uint32_t W = 3u * L;
    float g[3][2];
#pragma unroll
    for (uint32_t plane = 0; plane < 3; plane++) {
        const float* gr = grad + (size_t)b * W + plane * L;
        const float2* jj = reinterpret_cast<const float2*>(dy_dx) + ((size_t)plane * B + b) * L;
        float r0 = 0.0f, r1 = 0.0f;
        for (uint32_t l = 0; l < L; l++) {
            const float2 j = jj[l];
            r0 = lz_fmaf(gr[l], j.x, r0);
            r1 = lz_fmaf(gr[l], j.y, r1);
        }
        g[plane][0] = r0 * inv2b;
        g[plane][1] = r1 * inv2b;
    }
    grad_xyz[(size_t)b * 3 + 0] = g[0][0] + g[2][0];
    grad_xyz[(size_t)b * 3 + 1] = g[0][1] + g[1][0];
    grad_xyz[(size_t)b * 3 + 2] = g[1][1] + g[2][1];
}

// ---- host entries -------------------------------------------------------------------------------------------------------------------------
static int lz_tri_check(const char* who, uint32_t B, uint32_t L, uint32_t H, float bound) {
    LZ_REQUIRE(L >= 1u && L <= LZ_TRI_MAX_LEVELS, LZ_ERR_BAD_ARGUMENT, "%s: num_levels must be 1 .. %u (got %u)", who, LZ_TRI_MAX_LEVELS, L);
    LZ_REQUIRE(H >= 1u, LZ_ERR_BAD_ARGUMENT, "%s: base_resolution must be >= 1", who);
    LZ_REQUIRE(bound > 0.0f && bound < INFINITY, LZ_ERR_BAD_ARGUMENT, "%s: bound must be positive and finite (got %g)", who, (double)bound);
    LZ_REQUIRE(B <= 0x7fffff00u, LZ_ERR_BAD_ARGUMENT, "%s: at most 2^31 - 256 samples per call (got %u)", who, B);
    return LZ_OK;
}

extern "C" int lz_triplane_encode_forward(const float* xyz, const float* emb_xy, const float* emb_yz, const float* emb_xz,
                                          const int32_t* offsets, float* out, float* dy_dx, uint32_t B, uint32_t L, float S, uint32_t H,
                                          float bound, lz_stream_t stream) {
    if (B == 0) return LZ_OK;
    LZ_REQUIRE(xyz && emb_xy && emb_yz && emb_xz && offsets && out, LZ_ERR_BAD_ARGUMENT, "triplane_encode_forward: null tensor");
    const int rc = lz_tri_check("triplane_encode_forward", B, L, H, bound);
    if (rc != LZ_OK) return rc;
    LZ_REQUIRE((reinterpret_cast<uintptr_t>(out) & 15u) == 0u && (reinterpret_cast<uintptr_t>(dy_dx) & 7u) == 0u, LZ_ERR_BAD_ARGUMENT,
               "triplane_encode_forward: out must be 16-byte aligned, dy_dx 8-byte aligned");
    LzGridLevels lv;
    LZ_REQUIRE(lz_fill_levels(lv, L, S, H) == 0, LZ_ERR_BAD_ARGUMENT, "triplane_encode_forward: at most %d levels", LZ_MAX_LEVELS);
    const LzTriTables emb = {{emb_xy, emb_yz, emb_xz}};
    const float inv2b = 1.0f / (2.0f * bound);
    const dim3 grid(lz_div_up(B, 64u * LZ_TRI_WAVES)), block(64u * LZ_TRI_WAVES);
    const size_t lds = (size_t)LZ_TRI_WAVES * 64u * ((3u * L) | 1u) * sizeof(float);
    if (dy_dx) hipLaunchKernelGGL((lz_k_triplane_encode<true>), grid, block, lds, lz_st(stream), xyz, emb, offsets, out, dy_dx, B, L, lv, bound, inv2b);
    else hipLaunchKernelGGL((lz_k_triplane_encode<false>), grid, block, lds, lz_st(stream), xyz, emb, offsets, out, dy_dx, B, L, lv, bound, inv2b);
    LZ_CHECK_LAUNCH("triplane_encode_forward");
    return LZ_OK;
}

extern "C" int lz_triplane_encode_backward(const float* grad, const float* xyz, const int32_t* offsets, float* grad_emb_xy, float* grad_emb_yz,
                                           float* grad_emb_xz, const float* dy_dx, float* grad_xyz, uint32_t B, uint32_t L, float S,
                                           uint32_t H, float bound, lz_stream_t stream) {
    if (B == 0) return LZ_OK;
    const bool tables = grad_emb_xy || grad_emb_yz || grad_emb_xz;
    LZ_REQUIRE(grad && xyz && offsets, LZ_ERR_BAD_ARGUMENT, "triplane_encode_backward: null tensor");
    LZ_REQUIRE(!tables || (grad_emb_xy && grad_emb_yz && grad_emb_xz), LZ_ERR_BAD_ARGUMENT,
               "triplane_encode_backward: the three table gradients come together (all, or none for the input gradient alone)");
    LZ_REQUIRE((dy_dx != nullptr) == (grad_xyz != nullptr), LZ_ERR_BAD_ARGUMENT, "triplane_encode_backward: dy_dx and grad_xyz come together");
    LZ_REQUIRE(tables || grad_xyz, LZ_ERR_BAD_ARGUMENT, "triplane_encode_backward: nothing to compute (no table gradient, no grad_xyz)");
    const int rc = lz_tri_check("triplane_encode_backward", B, L, H, bound);
    if (rc != LZ_OK) return rc;
    LZ_REQUIRE((reinterpret_cast<uintptr_t>(dy_dx) & 7u) == 0u, LZ_ERR_BAD_ARGUMENT, "triplane_encode_backward: dy_dx must be 8-byte aligned");
    LzGridLevels lv;
    LZ_REQUIRE(lz_fill_levels(lv, L, S, H) == 0, LZ_ERR_BAD_ARGUMENT, "triplane_encode_backward: at most %d levels", LZ_MAX_LEVELS);
    const float inv2b = 1.0f / (2.0f * bound);
    hipStream_t st = lz_st(stream);
    if (tables) {
        const LzTriGrads gt = {{grad_emb_xy, grad_emb_yz, grad_emb_xz}};
        const uint32_t W = 3u * L, use_lds = B >= LZ_TRI_LDS_MIN_B ? 1u : 0u;
        uint32_t chunk = 1024u;                   // small batches: one sample per thread, global float atomics
        size_t lds = 0;
        if (use_lds) {                            // ~1024 workgroups (128 KB of LDS each: one per CU and round), never less than 4096 samples each
            uint32_t n_chunks = lz_div_up(B, 4096u);
            const uint32_t cap = 1024u / W > 0u ? 1024u / W : 1u;
            if (n_chunks > cap) n_chunks = cap;
            chunk = lz_div_up(B, n_chunks);
            lds = LZ_TRI_FX_LDS_BYTES;
            static bool attr_set = false;         // more than 64 KB of dynamic LDS has to be requested once
            if (!attr_set) {
                (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&lz_k_triplane_encode_backward), hipFuncAttributeMaxDynamicSharedMemorySize,
                                          LZ_TRI_FX_LDS_BYTES);
                attr_set = true;
            }
        }
        const uint32_t n_chunks = lz_div_up(B, chunk);
        hipLaunchKernelGGL(lz_k_triplane_encode_backward, dim3(n_chunks * W), dim3(1024), lds, st, grad, xyz, offsets, gt, B, L, lv, bound, inv2b,
                           chunk, use_lds);
    }
    if (grad_xyz)
        hipLaunchKernelGGL(lz_k_triplane_input_backward, dim3(lz_div_up(B, 256u)), dim3(256), 0, st, grad, dy_dx, grad_xyz, B, L, inv2b);
    LZ_CHECK_LAUNCH("triplane_encode_backward");
    return LZ_OK;
}
