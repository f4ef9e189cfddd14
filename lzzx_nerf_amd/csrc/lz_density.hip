// lz_density.hip -- NeRFNetwork.density (nerf_triplane/network.py:283-311) for gfx950: the fused triplane head cut off behind sigma_net.
//
// Replaces what the reference runs wherever it wants the field and not a pixel -- update_extra_state (renderer.py:749: sigma),
// get_audio_grid / get_eye_grid (renderer.py:823-933: ambient_aud, ambient_eye), extract_fields (utils.py:348-363: sigma) -- each a Python
// loop of meshgrid + cat + density() per block.  Here the slice of lz_k_triplane_head (lz_head_slice.h, CUT) and of its f16 twin
// (lz_head_f16w_slice.h) stops at the sigma row: gather, aud_ch_att_net, eye_att_net, sigma_net.0 / .1, the sigma row, exp -- 209 of
// the forward's 353 f32 MFMAs per 16 samples (273 with geo_feat), 36 of its 60 f16 MFMAs per 32 samples (44 with geo_feat).  Same
// fragments, same k order, same packed weights: sigma, ambient_aud and ambient_eye carry the forward's bits.
//
// Same workgroup shape, LDS staging and slice queue as the forward kernels (lz_head.hip, lz_head_f16.hip).  The point of a row comes from
// memory (lz_triplane_head_density) or is made in the kernel (lz_triplane_density_lattice): a cell of the occupancy grid
// (lz_density_cell.h, the rule of lz_density_grid_points) or a node of three axes (extract_fields' custom_meshgrid).
#include "lz_density_cell.h"
#include "lz_head_f16w_slice.h"   // and, through it, lz_head_slice.h

#define LZD_WG 1024        // threads per workgroup, as lz_k_triplane_head / lz_k_triplane_head_f16w

// where a row's point comes from
enum { LZD_ROWS = 0, LZD_LATTICE = 1 };
struct LzDensityPoints {
    const float* xyzs;                 // LZD_ROWS: [M, 3]
    uint32_t source;                   // LZD_LATTICE: LZ_LATTICE_CELLS / LZ_LATTICE_AXES
    const float* noise;                // cells: [C, G^3, 3]
    uint32_t G;
    float bound;
    const float *X, *Y, *Z;            // axes
    uint32_t Ry, Rz;
};

template <int SRC>
__device__ __forceinline__ void lzd_point(const LzDensityPoints& ps, uint32_t m, float (&xyz)[3]) {
    if constexpr (SRC == LZD_ROWS) {
        xyz[0] = ps.xyzs[(size_t)m * 3]; xyz[1] = ps.xyzs[(size_t)m * 3 + 1]; xyz[2] = ps.xyzs[(size_t)m * 3 + 2];
    } else if (ps.source == LZ_LATTICE_CELLS) {     // (launch-uniform)
        lz_density_cell_point(ps.noise, m, ps.G, ps.bound, xyz);
    } else {
        const uint32_t ij = m / ps.Rz, k = m - ij * ps.Rz;
        const uint32_t i = ij / ps.Ry, j = ij - i * ps.Ry;
        xyz[0] = ps.X[i]; xyz[1] = ps.Y[j]; xyz[2] = ps.Z[k];
    }
}

__device__ __forceinline__ uint32_t lzd_rows(uint32_t M, const int* __restrict__ count) {
    if (!count) return M;
    const int c = *count;
    return c < 0 ? 0u : ((uint32_t)c < M ? (uint32_t)c : M);
}

// ---- f32: 16-sample slices on v_mfma_f32_16x16x4_f32 (p->precision 0 / 2) ----
template <bool GEO, int SRC>
__global__ void __launch_bounds__(LZD_WG, LZD_WG / 256)
lz_k_triplane_density(LzHeadArgs P, LzDensityPoints ps, uint32_t M, const int* __restrict__ count, float* __restrict__ sigmas,
                      float* __restrict__ amb_aud, float* __restrict__ amb_eye, float* __restrict__ geo_feat) {
    __shared__ float wl[LzHeadLds<false>::FLOATS];
    const uint32_t Meff = lzd_rows(M, count);
    const uint32_t n_slices = (Meff + 15) / 16;
    const uint32_t slice_lo = (uint32_t)(((uint64_t)n_slices * blockIdx.x) / gridDim.x);
    const uint32_t slice_hi = (uint32_t)(((uint64_t)n_slices * (blockIdx.x + 1)) / gridDim.x);
    if (slice_lo >= slice_hi) return;
    const int lane = threadIdx.x & 63;
    const int s = lane & 15, q = lane >> 4;
    LzHeadCtx ctx;
    lz_head_stage<false>(P, wl, LZD_WG, q, ctx);
    __syncthreads();
    int* queue = reinterpret_cast<int*>(wl + LzHeadLds<false>::TAB) + LZ_LVTAB_QUEUE;
    for (;;) {
        int slice = 0;
        if (lane == 0) slice = atomicAdd(queue, 1);
        slice = __builtin_amdgcn_readfirstlane(slice);
        if (slice_lo + (uint32_t)slice >= slice_hi) break;
        const uint32_t base = (slice_lo + (uint32_t)slice) * 16;
        uint32_t m = base + s;
        if (m >= Meff) m = Meff - 1;  // clamp: computed, never stored
        float xyz[3];
        lzd_point<SRC>(ps, m, xyz);
        LzHeadOut o;
        float geo[16];
        lz_head_slice<false, false, false, false, GEO ? LZ_CUT_DENSITY_GEO : LZ_CUT_DENSITY>(ctx, lane, xyz[0], xyz[1], xyz[2], LzShNone(), o, geo);
        if (base + s < Meff) {
            if (q == 0) {
                if (sigmas) sigmas[m] = o.sigma;
                if (amb_aud) amb_aud[m] = o.ambaud;
                if (amb_eye) amb_eye[m] = o.eyeatt;
            }
            if constexpr (GEO) {   // lane (s, q) holds features 16 ft + 4 q + r: four 16-byte stores, the sample's row 256 contiguous bytes
#pragma unroll
                for (int ft = 0; ft < 4; ft++)
                    *reinterpret_cast<lz_f4*>(geo_feat + (size_t)m * 64 + 16 * ft + 4 * q) = lz_f4{geo[4 * ft], geo[4 * ft + 1], geo[4 * ft + 2], geo[4 * ft + 3]};
            }
        }
    }
}

// ---- f16 (autocast rounding): 32-sample slices on v_mfma_f32_32x32x16_f16 (p->precision 1) ----
template <bool GEO, int SRC>
__global__ void __launch_bounds__(LZD_WG, LZD_WG / 256)
lz_k_triplane_density_f16w(LzHead16Args P, LzDensityPoints ps, uint32_t M, const int* __restrict__ count, float* __restrict__ sigmas,
                           float* __restrict__ amb_aud, float* __restrict__ amb_eye, _Float16* __restrict__ geo_feat) {
    __shared__ lz_h8 wl[LZ_HEAD16W_LDS_H8];
    const uint32_t Meff = lzd_rows(M, count);
    const uint32_t n_slices = (Meff + 31) / 32;
    const uint32_t slice_lo = (uint32_t)(((uint64_t)n_slices * blockIdx.x) / gridDim.x);
    const uint32_t slice_hi = (uint32_t)(((uint64_t)n_slices * (blockIdx.x + 1)) / gridDim.x);
    if (slice_lo >= slice_hi) return;
    LzHead16Ctx ctx;
    lz_head16w_stage(P, wl, LZD_WG, ctx);
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int s = lane & 31, h = lane >> 5;
    int* queue = reinterpret_cast<int*>(wl + W_FRAGS * 64) + LZ_LVTAB_QUEUE;
    for (;;) {
        int slice = 0;
        if (lane == 0) slice = atomicAdd(queue, 1);
        slice = __builtin_amdgcn_readfirstlane(slice);
        if (slice_lo + (uint32_t)slice >= slice_hi) break;
        const uint32_t base = (slice_lo + (uint32_t)slice) * 32;
        uint32_t m = base + s;
        if (m >= Meff) m = Meff - 1;  // clamp: computed, never stored
        float xyz[3];
        lzd_point<SRC>(ps, m, xyz);
        LzHead16wOut o;
        lz_h8 geo[4];
        lz_head16w_slice<false, false, GEO ? LZ_CUT_DENSITY_GEO : LZ_CUT_DENSITY>(ctx, lane, xyz[0], xyz[1], xyz[2], LzShNone(), o, geo);
        if (base + s < Meff) {
            if (h == 0) {   // lane half 0 owns the per-sample scalars, lane half 1 sigma (lz_k_triplane_head_f16w)
                if (amb_aud) amb_aud[m] = o.ambaud;
                if (amb_eye) amb_eye[m] = o.eyeatt;
            } else if (sigmas) {
                sigmas[m] = o.b;
            }
            if constexpr (GEO) {   // geo[2 t + u][j] = feature 32 t + 16 u + 8 (j >> 2) + 4 h + (j & 3): eight 8-byte stores
                typedef _Float16 lz_h4 __attribute__((ext_vector_type(4)));
#pragma unroll
                for (int k = 0; k < 4; k++)
#pragma unroll
                    for (int g = 0; g < 2; g++)
                        *reinterpret_cast<lz_h4*>(geo_feat + (size_t)m * 64 + 16 * k + 8 * g + 4 * h) =
                            lz_h4{geo[k][4 * g], geo[k][4 * g + 1], geo[k][4 * g + 2], geo[k][4 * g + 3]};
            }
        }
    }
}

// ---- host ----
template <int SRC>
static int lzd_launch(const lz_head_params* p, const LzDensityPoints& ps, uint32_t M, const int32_t* count, float* sigma, float* amb_aud,
                      float* amb_eye, void* geo_feat, hipStream_t st, const char* who) {
    LZ_REQUIRE(p->emb_xy && p->emb_yz && p->emb_xz && p->offsets && p->packed && p->enc_a, LZ_ERR_BAD_ARGUMENT, "%s: incomplete lz_head_params", who);
    LZ_REQUIRE(p->precision >= 0 && p->precision <= 2, LZ_ERR_BAD_ARGUMENT, "%s: precision must be 0 (f32), 1 (f16) or 2 (f32, folded geo)", who);
    float scale[12];
    uint32_t res[12];
    for (int l = 0; l < 12; l++) {  // gridencoder.cu:125-126 on the host, same libm call as the CPU checker (lz_triplane_head_forward)
        scale[l] = exp2f((float)l * p->S) * (float)p->H - 1.0f;
        res[l] = (uint32_t)ceilf(scale[l]) + 1u;
    }
    const uint32_t n_cu = (uint32_t)lz_cu_count();
    if (p->precision == 1) {
        LzHead16Args a;
        a.emb[0] = p->emb_xy; a.emb[1] = p->emb_yz; a.emb[2] = p->emb_xz;
        a.offsets = p->offsets; a.packed = reinterpret_cast<const lz_h8*>(p->packed); a.enc_a = p->enc_a; a.ind_code = nullptr;
        a.eye = p->eye; a.bound = p->bound;
        for (int l = 0; l < 12; l++) { a.scale[l] = scale[l]; a.res[l] = res[l]; }
        const uint32_t tiles = lz_div_up(M, LZD_WG / 64 * 32);
        const dim3 grid(tiles < n_cu ? tiles : n_cu), block(LZD_WG);
        _Float16* geo = reinterpret_cast<_Float16*>(geo_feat);
        if (SRC == LZD_ROWS && geo) hipLaunchKernelGGL((lz_k_triplane_density_f16w<true, LZD_ROWS>), grid, block, 0, st, a, ps, M, count, sigma, amb_aud, amb_eye, geo);
        else hipLaunchKernelGGL((lz_k_triplane_density_f16w<false, SRC>), grid, block, 0, st, a, ps, M, count, sigma, amb_aud, amb_eye, geo);
    } else {
        LzHeadArgs a;
        a.emb[0] = p->emb_xy; a.emb[1] = p->emb_yz; a.emb[2] = p->emb_xz;
        a.offsets = p->offsets; a.packed = reinterpret_cast<const float*>(p->packed); a.enc_a = p->enc_a; a.ind_code = nullptr; a.eye = p->eye;
        a.bound = p->bound; a.testing = 1;
        for (int l = 0; l < 12; l++) { a.scale[l] = scale[l]; a.res[l] = res[l]; }
        const uint32_t tiles = lz_div_up(M, LZD_WG / 64 * 16);
        const dim3 grid(tiles < n_cu ? tiles : n_cu), block(LZD_WG);
        float* geo = reinterpret_cast<float*>(geo_feat);
        if (SRC == LZD_ROWS && geo) hipLaunchKernelGGL((lz_k_triplane_density<true, LZD_ROWS>), grid, block, 0, st, a, ps, M, count, sigma, amb_aud, amb_eye, geo);
        else hipLaunchKernelGGL((lz_k_triplane_density<false, SRC>), grid, block, 0, st, a, ps, M, count, sigma, amb_aud, amb_eye, geo);
    }
    LZ_CHECK_LAUNCH(who);
    return LZ_OK;
}

extern "C" int lz_triplane_head_density(const lz_head_params* p, const float* xyzs, uint32_t M, const int32_t* count, float* sigma,
                                        float* amb_aud, float* amb_eye, void* geo_feat, lz_stream_t stream) {
    if (M == 0) return LZ_OK;
    LZ_REQUIRE(p && xyzs && sigma && amb_aud, LZ_ERR_BAD_ARGUMENT, "triplane_head_density: null tensor");
    LzDensityPoints ps = {};
    ps.xyzs = xyzs;
    return lzd_launch<LZD_ROWS>(p, ps, M, count, sigma, amb_aud, amb_eye, geo_feat, lz_st(stream), "triplane_head_density");
}

extern "C" int lz_triplane_density_lattice(const lz_head_params* p, uint32_t source, const float* noise, uint32_t C, uint32_t G,
                                           const float* X, uint32_t Rx, const float* Y, uint32_t Ry, const float* Z, uint32_t Rz,
                                           float* sigma, float* amb_aud, float* amb_eye, lz_stream_t stream) {
    LZ_REQUIRE(source == LZ_LATTICE_CELLS || source == LZ_LATTICE_AXES, LZ_ERR_BAD_ARGUMENT, "triplane_density_lattice: source must be LZ_LATTICE_CELLS or LZ_LATTICE_AXES");
    LzDensityPoints ps = {};
    ps.source = source;
    uint64_t rows;
    if (source == LZ_LATTICE_CELLS) {
        if (C * G == 0) return LZ_OK;
        LZ_REQUIRE(p && noise, LZ_ERR_BAD_ARGUMENT, "triplane_density_lattice: null tensor");
        LZ_REQUIRE(C <= 8 && G >= 2 && G <= 1024, LZ_ERR_BAD_ARGUMENT, "triplane_density_lattice: cascade <= 8, 2 <= grid_size <= 1024");
        rows = (uint64_t)C * G * G * G;
        ps.noise = noise; ps.G = G; ps.bound = p->bound;
    } else {
        rows = (uint64_t)Rx * Ry * Rz;
        if (rows == 0) return LZ_OK;
        LZ_REQUIRE(p && X && Y && Z, LZ_ERR_BAD_ARGUMENT, "triplane_density_lattice: null tensor");
        ps.X = X; ps.Y = Y; ps.Z = Z; ps.Ry = Ry; ps.Rz = Rz;
    }
    // the kernel's row index is 32-bit
    LZ_REQUIRE(rows < (1ull << 32), LZ_ERR_BAD_ARGUMENT, "triplane_density_lattice: the lattice must have fewer than 2^32 points");
    LZ_REQUIRE(sigma || amb_aud || amb_eye, LZ_ERR_BAD_ARGUMENT, "triplane_density_lattice: no output requested");
    return lzd_launch<LZD_LATTICE>(p, ps, (uint32_t)rows, nullptr, sigma, amb_aud, amb_eye, nullptr, lz_st(stream), "triplane_density_lattice");
}
