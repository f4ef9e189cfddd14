// lz_grid_fixed.hip -- the ORDER-FREE table gradient of the grid encoder: lz_grid_encode_backward_fixed (table_grad "fixed").
//
// Float atomics (lz_grid_encode_backward) give other bits on every call; the ordered sum (lz_grid_encode_backward_ordered) repeats, but
// follows the order of the samples and pays a sort per level.  Here every term t = fl32(w g) of a level is quantised to the integer
// q(t) = rint((double)t 2^e) with ONE power-of-two scale per level, the integers of a table entry are added as int64 -- integer addition
// is associative, so neither the order of arrival nor the launch geometry, the chunking or a permutation of the rows can change the sum --
// and the sum is rounded to f32 once: grad_embeddings[i] += fl32((double)A_i 2^-e) for every entry with A_i != 0.  The result is a
// function of the SET of samples.  The scale, with m = max |g| over the level's whole gradient (out-of-range rows included, NaN as inf):
//     m < 2^ex (frexpf),  hb = max(2, ceil(log2(B 2^D))),  e = clamp(51 - hb - ex, -100, 100)
// so |q| < 2^(51 - hb), at most 2^hb terms meet in an entry, |A_i| < 2^51 cannot overflow and (double)A_i 2^-e is exact.  Per entry
// |fl32(A_i 2^-e) - S_i| <= n_i 2^-(e+1) + 1/2 ulp for the real sum S_i of its n_i terms.  A level with m == 0 writes nothing; a level
// whose m is not finite takes float atomics into grad_embeddings, as lz_grid_encode_backward does (its bits are not promised).
//
// One call is: a memset of the workspace, then five launches, each over ALL levels with the level as the slow grid dimension.
//   max      per-level max |g|: wave and workgroup reduction, then an integer atomicMax on the float's bit pattern (non-negative floats order like
//            their bits) into the workspace header
//   scale    one thread per level turns the maximum into e (or one of the markers below) in the header
//   lds      levels whose 8-byte accumulators fit LZ_GRID_FIXED_LDS_BYTES of LDS (the 12 levels of a triplane plane, level 0 of cfg2):
//            a workgroup owns one (level, chunk of rows), accumulates in LDS with the level's GLOBAL scale and flushes the non-zero
//            entries with contiguous int64 atomics into the workspace, so chunks combine exactly
//   scatter  every other level: int64 global atomics into the workspace, lanes arranged like lz_k_grid_backward_xc; also the float
//            atomics of a non-finite level
//   convert  one thread per (entry, channel): the write rule above
// WHO ZEROES THE ACCUMULATORS: the call does, with the memset at its start (header and accumulators in one piece); convert leaves them
// as they are.  So the workspace needs no initialisation and may be shared with anything else between two calls.
// LAUNCH ORDER: one grid over all levels' accumulators (8 bytes per table element, 101 MB for cfg2) rather than sixteen rounds over one
// level's.  With the level as the slow grid dimension the workgroups of one level are dispatched together, so the atomics of a moment
// still aim at one level's accumulators (8 MB for a 2^19 x 2 level) as in the per-level arrangement, while the per-level arrangement
// would add three launches per level (48 for cfg2) to save a memset and a convert pass that stream 101 MB each -- tens of
// microseconds next to a scatter of milliseconds (DESIGN 4.9 has the trace split).
//
// Indices, cells and weights are lz_grid_common.h's, the checker's by construction.
#include "lz_grid_common.h"

#define LZ_GRID_FIXED_LDS_BYTES 131072     // = LZ_GRID_FX_LDS_BYTES (lz_grid.hip): what lz_k_grid_backward_lds_fx holds
#define LZ_GRID_FIXED_HEADER 256u          // bytes: uint32 max bits [32] | int32 e [32]; the int64 accumulators follow
#define LZ_GRID_FIXED_EMPTY 0x7fffffff     // markers in place of e: m == 0, nothing to add
#define LZ_GRID_FIXED_FLOAT 0x7ffffffe     //   m not finite: float atomics
#define LZ_GRID_FIXED_NOFIT 0x7ffffffd     //   the level's accumulators lie past the end of the workspace

// |g| with NaN mapped to +inf (fmaxf drops a NaN operand), as lz_abs_nan_inf in lz_grid.hip
__device__ __forceinline__ float lz_fixed_abs(float g) {
    const float a = fabsf(g);
    return a == a ? a : INFINITY;
}

// element (b, level, ch) of the gradient: [L, B, C], or sample-major rows of `pitch` elements (L C unless the rows belong to a wider matrix)
__device__ __forceinline__ size_t lz_fixed_grad_at(uint32_t b, uint32_t level, uint32_t ch, uint32_t B, uint32_t C, uint32_t pitch, bool sample_major) {
    return sample_major ? (size_t)b * pitch + level * C + ch : ((size_t)level * B + b) * C + ch;
}

// One atomic per workgroup, few workgroups per level: atomics on one address retire one after another (a wave-level atomicMax from 5 600
// workgroups cost 0.26 ms on the cfg2 batch, ten times the read itself).
__global__ void __launch_bounds__(256)
lz_k_grid_fixed_max(const float* __restrict__ grad, uint32_t* __restrict__ maxbits, uint32_t B, uint32_t C, uint32_t pitch, bool sample_major) {
    __shared__ float wmax[4];
    const uint32_t level = blockIdx.y;
    const uint64_t n = (uint64_t)B * C, stride = (uint64_t)gridDim.x * blockDim.x;
    float gm = 0.0f;
#pragma unroll 4
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint32_t b = (uint32_t)(i / C), ch = (uint32_t)(i - (uint64_t)b * C);
        gm = fmaxf(gm, lz_fixed_abs(grad[lz_fixed_grad_at(b, level, ch, B, C, pitch, sample_major)]));
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) gm = fmaxf(gm, __shfl_xor(gm, off, 64));
    if ((threadIdx.x & 63u) == 0u) wmax[threadIdx.x >> 6] = gm;
    __syncthreads();
    if (threadIdx.x == 0) {
        gm = fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));
        if (gm > 0.0f) atomicMax(maxbits + level, __float_as_uint(gm));
    }
}

__global__ void __launch_bounds__(64)
lz_k_grid_fixed_scale(const uint32_t* __restrict__ maxbits, int* __restrict__ e_out, const int* __restrict__ offsets, uint32_t L, uint32_t C,
                      int hb, uint64_t cap) {
    const uint32_t level = threadIdx.x;
    if (level >= L) return;
    const float m = __uint_as_float(maxbits[level]);
    int e;
    if (!(m > 0.0f)) e = LZ_GRID_FIXED_EMPTY;
    else if (!(m < INFINITY)) e = LZ_GRID_FIXED_FLOAT;           // needs no accumulators
    else if ((uint64_t)(uint32_t)offsets[level + 1] * C > cap) e = LZ_GRID_FIXED_NOFIT;
    else {
        int ex;
        (void)frexpf(m, &ex);                                     // m < 2^ex
        e = 51 - hb - ex;
        e = e > 100 ? 100 : (e < -100 ? -100 : e);
    }
    e_out[level] = e;
}

// rint(v 2^e) as a 64-bit integer: in double, v 2^e + 1.5 2^52 is rounded to an integer by the addition itself (to nearest, ties to even;
// |v 2^e| < 2^51) and the integer sits in the low mantissa bits -- to_fixed of lz_k_grid_backward_lds_fx
__device__ __forceinline__ unsigned long long lz_fixed_q(float v, double fxd) {
    const double t = __builtin_fma((double)v, fxd, 6755399441055744.0);
    return (unsigned long long)(__double_as_longlong(t) - 0x4338000000000000ll);
}

// Levels that do not fit LDS.  lane = (sample, x bit of the corner, channel), as lz_k_grid_backward_xc and for its reason: the x and x + 1
// corners of a cell are adjacent entries on dense levels and share a line on hashed ones (prime_x = 1), so 2 C lanes of an instruction
// aim at one line instead of one.  The same terms w * g as there; a level marked FLOAT adds them as floats into the table gradient.
template <uint32_t D, uint32_t C>
__global__ void __launch_bounds__(256)
lz_k_grid_fixed_scatter(const float* __restrict__ grad, const float* __restrict__ inputs, const int* __restrict__ offsets,
                        const int* __restrict__ e_in, unsigned long long* __restrict__ acc, float* __restrict__ grad_grid, uint32_t B, uint32_t L,
                        uint32_t pitch, LzGridLevels lv, uint32_t gridtype, bool align_corners, bool sample_major) {
    constexpr uint32_t LPS = 2 * C;                     // lanes per sample
    const uint32_t level = blockIdx.y;
    const int e = e_in[level];
    if (e == LZ_GRID_FIXED_EMPTY || e == LZ_GRID_FIXED_NOFIT) return;
    const bool as_float = e == LZ_GRID_FIXED_FLOAT;
    const LzGridLevel lvl = lz_grid_level<D, false>(offsets, lv, level, gridtype, align_corners);
    if (!as_float && (size_t)lvl.hs * C * 8 <= LZ_GRID_FIXED_LDS_BYTES) return;      // lz_k_grid_fixed_lds has this level
    const double fxd = __builtin_ldexp(1.0, as_float ? 0 : e);
    unsigned long long* a = acc + (size_t)lvl.off0 * C;
    float* gg = grad_grid + (size_t)lvl.off0 * C;
    const uint64_t total = (uint64_t)B * LPS, stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
        const uint32_t b = (uint32_t)(t / LPS), sub = (uint32_t)(t - (uint64_t)b * LPS), xb = sub / C, ch = sub - xb * C;
        float x[D];
#pragma unroll
        for (uint32_t d = 0; d < D; d++) x[d] = inputs[(size_t)b * D + d];
        const LzGridCell<D> cell = lz_grid_cell<D, false>(x, lvl.scale, align_corners);
        if (cell.oob) continue;
        const float g = grad[lz_fixed_grad_at(b, level, ch, B, C, pitch, sample_major)];
        uint32_t term[D][2];
        lz_grid_terms<D>(lvl, cell, align_corners, term);
#pragma unroll
        for (uint32_t h = 0; h < (1u << (D - 1)); h++) {
            const uint32_t idx = (h << 1) | xb;
            const uint32_t index = lz_grid_corner_index<D>(lvl, cell, term, idx, C, gridtype, align_corners) + ch;
            const float v = lz_grid_weight<D>(cell, idx) * g;
            if (as_float) atomicAdd(gg + index, v);
            else atomicAdd(a + index, lz_fixed_q(v, fxd));
        }
    }
}

// Levels whose accumulators fit LDS: a workgroup owns one (level, chunk of rows).  The level's scale is the global one, so what a chunk
// flushes is added to the other chunks' as integers.  WHICH rows a thread takes: lane-major segments, as in lz_k_grid_backward_lds_fx and
// for the reason given there -- the 64 lanes of an instruction must not sit in the same cell (same-address LDS atomics retire one lane
// at a time), and consecutive rows do exactly that under both sample orders of the march.  The chunk is cut into 64 segments of 64 T
// rows, lane l walks segment l, and the 16 waves x 4 rows x T trips cover the segment: row = b0 + l 64 T + (16 k + w) 4 + i.
template <uint32_t D, uint32_t C>
__global__ void __launch_bounds__(1024)
lz_k_grid_fixed_lds(const float* __restrict__ grad, const float* __restrict__ inputs, const int* __restrict__ offsets,
                    const int* __restrict__ e_in, unsigned long long* __restrict__ acc, uint32_t B, uint32_t L, uint32_t pitch, LzGridLevels lv,
                    uint32_t gridtype, bool align_corners, bool sample_major, uint32_t chunk) {
    extern __shared__ __align__(16) unsigned long long lz_fixed_acc64[];
    const uint32_t level = blockIdx.x % L, c = blockIdx.x / L;
    const int e = e_in[level];
    if (e == LZ_GRID_FIXED_EMPTY || e == LZ_GRID_FIXED_NOFIT || e == LZ_GRID_FIXED_FLOAT) return;
    const LzGridLevel lvl = lz_grid_level<D>(offsets, lv, level, gridtype, align_corners);
    const uint32_t n = lvl.hs * C;
    if ((size_t)n * 8 > LZ_GRID_FIXED_LDS_BYTES) return;                            // lz_k_grid_fixed_scatter has this level
    const uint32_t b0 = c * chunk, b1 = (B - b0 < chunk) ? B : b0 + chunk;
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) lz_fixed_acc64[i] = 0ull;
    __syncthreads();
    const double fxd = __builtin_ldexp(1.0, e);
    const uint32_t T = (b1 - b0 + 4095u) / 4096u, seg = 64u * T;
    const uint32_t row0 = b0 + (threadIdx.x & 63u) * seg + (threadIdx.x >> 6) * 4u;   // + 64 k + i
    for (uint32_t k = 0; k < T; k++) {
#pragma unroll
        for (uint32_t i = 0; i < 4; i++) {
            const uint32_t b = row0 + 64u * k + i;
            if (b >= b1) continue;
            float x[D];
#pragma unroll
            for (uint32_t d = 0; d < D; d++) x[d] = inputs[(size_t)b * D + d];
            const LzGridCell<D> cell = lz_grid_cell<D, false>(x, lvl.scale, align_corners);
            if (cell.oob) continue;
            float gcur[C];
#pragma unroll
            for (uint32_t ch = 0; ch < C; ch++) gcur[ch] = grad[lz_fixed_grad_at(b, level, ch, B, C, pitch, sample_major)];
            uint32_t term[D][2];
            lz_grid_terms<D>(lvl, cell, align_corners, term);
#pragma unroll
            for (uint32_t idx = 0; idx < (1u << D); idx++) {
                const float w = lz_grid_weight<D>(cell, idx);
                const uint32_t index = lz_grid_corner_index<D>(lvl, cell, term, idx, C, gridtype, align_corners);
#pragma unroll
                for (uint32_t ch = 0; ch < C; ch++)
                    __hip_atomic_fetch_add(lz_fixed_acc64 + index + ch, lz_fixed_q(w * gcur[ch], fxd), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
        }
    }
    __syncthreads();
    unsigned long long* a = acc + (size_t)lvl.off0 * C;
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
        const unsigned long long v = lz_fixed_acc64[i];
        if (v != 0ull) atomicAdd(a + i, v);
    }
}

// grad_embeddings[i] += fl32((double)A_i 2^-e) where A_i != 0: |A_i| < 2^51 converts exactly, the power of two scales exactly, the
// conversion to f32 is the one rounding.  A level marked NOFIT leaves a NaN in its first entry: offsets live on the device, so only the
// device can see that the caller's workspace is shorter than lz_grid_fixed_workspace(offsets[L], C), and it must not pass for a gradient.
__global__ void __launch_bounds__(256)
lz_k_grid_fixed_convert(const unsigned long long* __restrict__ acc, const int* __restrict__ e_in, const int* __restrict__ offsets,
                        float* __restrict__ grad_grid, uint32_t C) {
    const uint32_t level = blockIdx.y;
    const int e = e_in[level];
    const uint32_t off0 = (uint32_t)offsets[level], hs = (uint32_t)offsets[level + 1] - off0;
    if (e == LZ_GRID_FIXED_NOFIT && blockIdx.x == 0 && threadIdx.x == 0) grad_grid[(size_t)off0 * C] = __uint_as_float(0x7fc00000u);
    if (e == LZ_GRID_FIXED_EMPTY || e == LZ_GRID_FIXED_NOFIT || e == LZ_GRID_FIXED_FLOAT) return;
    const unsigned long long* a = acc + (size_t)off0 * C;
    float* gg = grad_grid + (size_t)off0 * C;
    const uint64_t n = (uint64_t)hs * C, stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const long long v = (long long)a[i];
        if (v != 0) gg[i] = gg[i] + (float)__builtin_ldexp((double)v, -e);
    }
}

extern "C" size_t lz_grid_fixed_workspace(uint32_t n_entries, uint32_t C) {
    if (C != 1u && C != 2u) return 0;
    return (size_t)LZ_GRID_FIXED_HEADER + (size_t)n_entries * C * 8u;
}

template <uint32_t D, uint32_t C>
static void lz_grid_fixed_run(const float* grad, const float* inputs, const int* offsets, float* gemb, uint32_t B, uint32_t L, uint32_t pitch,
                              const LzGridLevels& lv, uint32_t gridtype, bool ac, bool sm, unsigned char* ws, uint64_t ws_bytes, hipStream_t st) {
    uint32_t* maxbits = reinterpret_cast<uint32_t*>(ws);
    int* e = reinterpret_cast<int*>(ws + 128);
    unsigned long long* acc = reinterpret_cast<unsigned long long*>(ws + LZ_GRID_FIXED_HEADER);
    const uint64_t cap = (ws_bytes - LZ_GRID_FIXED_HEADER) / 8u;       // accumulators the workspace holds
    int hb = 2;
    while ((1ull << hb) < ((uint64_t)B << D)) hb++;
    (void)hipMemsetAsync(ws, 0, LZ_GRID_FIXED_HEADER + cap * 8u, st);
    uint32_t nb = lz_div_up((uint64_t)B * C, 256u * 8u);
    hipLaunchKernelGGL(lz_k_grid_fixed_max, dim3(nb < 128u ? nb : 128u, L), dim3(256), 0, st, grad, maxbits, B, C, pitch, sm);
    hipLaunchKernelGGL(lz_k_grid_fixed_scale, dim3(1), dim3(64), 0, st, maxbits, e, offsets, L, C, hb, cap);
    {   // about 1024 workgroups (the 128 KB of LDS leave one per compute unit at a time), never less than 4096 rows each
        uint32_t n_chunks = lz_div_up(B, 4096);
        const uint32_t most = 1024 / L > 0 ? 1024 / L : 1;
        if (n_chunks > most) n_chunks = most;
        const uint32_t chunk = lz_div_up(B, n_chunks);
        n_chunks = lz_div_up(B, chunk);
        static bool attr_set = false;   // per instantiation: more than 64 KB of dynamic LDS has to be requested once
        if (!attr_set) {
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&lz_k_grid_fixed_lds<D, C>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      LZ_GRID_FIXED_LDS_BYTES);
            attr_set = true;
        }
        hipLaunchKernelGGL((lz_k_grid_fixed_lds<D, C>), dim3(n_chunks * L), dim3(1024), LZ_GRID_FIXED_LDS_BYTES, st, grad, inputs, offsets, e, acc, B,
                           L, pitch, lv, gridtype, ac, sm, chunk);
    }
    nb = lz_div_up((uint64_t)B * 2 * C, 256);
    const uint32_t most = (uint32_t)lz_cu_count() * 32u;     // the workgroups of a level that does not take this kernel return at once: keep them few
    hipLaunchKernelGGL((lz_k_grid_fixed_scatter<D, C>), dim3(nb < most ? nb : most, L), dim3(256), 0, st, grad, inputs, offsets, e, acc, gemb, B, L,
                       pitch, lv, gridtype, ac, sm);
    hipLaunchKernelGGL(lz_k_grid_fixed_convert, dim3(512, L), dim3(256), 0, st, acc, e, offsets, gemb, C);
}

extern "C" int lz_grid_encode_backward_fixed(const void* grad, const float* inputs, const void* embeddings, const int32_t* offsets,
                                             void* grad_embeddings, uint32_t B, uint32_t D, uint32_t C, uint32_t L, float S, uint32_t H,
                                             const void* dy_dx, void* grad_inputs, uint32_t gridtype, int align_corners, int emb_f16,
                                             int grad_layout, void* workspace, uint32_t workspace_bytes_lo, uint32_t workspace_bytes_hi,
                                             uint32_t grad_row_stride, lz_stream_t stream) {
    (void)embeddings;
    if (B == 0) return LZ_OK;
    LZ_REQUIRE(grad && inputs && offsets && grad_embeddings && workspace, LZ_ERR_BAD_ARGUMENT, "grid_encode_backward_fixed: null tensor");
    LZ_REQUIRE(L >= 1 && H >= 1 && gridtype <= 1u, LZ_ERR_BAD_ARGUMENT, "grid_encode_backward_fixed: num_levels and base_resolution must be >= 1, gridtype 0 (hash) or 1 (tiled)");
    LZ_REQUIRE(grad_layout == 0 || grad_layout == 1, LZ_ERR_BAD_ARGUMENT, "grid_encode_backward_fixed: grad_layout must be 0 ([L, B, C]) or 1 ([B, L*C])");
    LZ_REQUIRE(!grad_inputs || dy_dx, LZ_ERR_BAD_ARGUMENT, "grid_encode_backward_fixed: grad_inputs needs dy_dx");
    LZ_REQUIRE(!emb_f16, LZ_ERR_UNSUPPORTED, "grid_encode_backward_fixed: f32 tables only (half tables take lz_grid_encode_backward)");
    LZ_REQUIRE(D == 2u || D == 3u, LZ_ERR_UNSUPPORTED, "grid_encode_backward_fixed: D must be 2 or 3 (other D take lz_grid_encode_backward)");
    LZ_REQUIRE(C == 1u || C == 2u, LZ_ERR_UNSUPPORTED, "grid_encode_backward_fixed: C must be 1 or 2 (C 4 and 8 take lz_grid_encode_backward or lz_grid_encode_backward_ordered)");
    LZ_REQUIRE(((uint64_t)B << D) < 0x80000000ull, LZ_ERR_UNSUPPORTED, "grid_encode_backward_fixed: B * 2^D must stay below 2^31 (got B = %u, D = %u)", B, D);
    LZ_REQUIRE(grad_row_stride == 0u || (grad_layout == 1 && grad_row_stride >= L * C && grad_row_stride % C == 0u && !(dy_dx && grad_inputs)),
               LZ_ERR_BAD_ARGUMENT, "grid_encode_backward_fixed: grad_row_stride (%u) needs grad_layout 1, a multiple of C that is at least L * C, and no grad_inputs",
               grad_row_stride);
    LZ_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15u) == 0u, LZ_ERR_BAD_ARGUMENT, "grid_encode_backward_fixed: workspace must be 16-byte aligned");
    LzGridLevels lv;
    LZ_REQUIRE(lz_fill_levels(lv, L, S, H) == 0, LZ_ERR_UNSUPPORTED, "grid_encode_backward_fixed: at most %d levels", LZ_MAX_LEVELS);
    // every level holds at least 8 entries (grid.py:115-118); the true size, offsets[L], is on the device and checked there
    const uint64_t ws_bytes = ((uint64_t)workspace_bytes_hi << 32) | workspace_bytes_lo;
    LZ_REQUIRE(ws_bytes >= lz_grid_fixed_workspace(8u * L, C), LZ_ERR_BAD_ARGUMENT,
               "grid_encode_backward_fixed: the workspace (%llu bytes) does not hold %u levels; lz_grid_fixed_workspace(entries, C) sizes it",
               (unsigned long long)ws_bytes, L);
    const bool sm = grad_layout == 1, ac = align_corners != 0;
    const uint32_t pitch = grad_row_stride ? grad_row_stride : L * C;
    hipStream_t st = lz_st(stream);
    unsigned char* ws = static_cast<unsigned char*>(workspace);
    const float* g = (const float*)grad;
    float* ge = (float*)grad_embeddings;
    if (D == 2u) {
        if (C == 1u) lz_grid_fixed_run<2, 1>(g, inputs, offsets, ge, B, L, pitch, lv, gridtype, ac, sm, ws, ws_bytes, st);
        else lz_grid_fixed_run<2, 2>(g, inputs, offsets, ge, B, L, pitch, lv, gridtype, ac, sm, ws, ws_bytes, st);
    } else {
        if (C == 1u) lz_grid_fixed_run<3, 1>(g, inputs, offsets, ge, B, L, pitch, lv, gridtype, ac, sm, ws, ws_bytes, st);
        else lz_grid_fixed_run<3, 2>(g, inputs, offsets, ge, B, L, pitch, lv, gridtype, ac, sm, ws, ws_bytes, st);
    }
    if (dy_dx && grad_inputs)   // kernel_input_backward (gridencoder.cu:316-342): already a fixed order
        lz_grid_input_backward_f32(g, (const float*)dy_dx, (float*)grad_inputs, B, D, C, L, sm, st);
    LZ_CHECK_LAUNCH("grid_encode_backward_fixed");
    return LZ_OK;
}
