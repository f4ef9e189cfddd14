// lz_ngp_frame_common.h -- what the two persistent kernels of the hash-grid NeRF frame share: lz_k_ngp_frame (lz_ngp_frame.hip, one sample
// per ray and pass) and lz_k_ngp_frame_spp (lz_ngp_frame_spp.hip, S samples per ray and pass).  The kernel-argument record, the slot
// fields and the LDS layout are read by both.  A slot taking a ray from the queue, the march's set-up from the slot and the gather of
// four levels are lz_k_ngp_frame's text as functions, called by lz_k_ngp_frame_spp only: lz_k_ngp_frame keeps them written out, because
// routed through these functions its three instantiations compile to a different instruction stream (compared as gfx950 assembly),
// and with the definitions merely moved here they compile to the instruction stream they had before this header existed.
// Library-internal: nothing here is part of the C ABI.
#ifndef LZ_NGP_FRAME_COMMON_H
#define LZ_NGP_FRAME_COMMON_H
#include "lz_frame_common.h"
#include "lz_grid_interp.h"
#include "lz_ngp_chain.h"
#include "lz_ngp16_chain.h"

#define LZNF_WG 256
#define LZNF_WAVES (LZNF_WG / 64)
#define LZNF_MARCH_PROBES 2      // empty cells a slot may cross per march attempt (as lz_k_frame: the other slots of the wave do not wait for a crossing)
#define LZNF_LEVELS 16
#define LZNF_SPP 13              // state word: S of the lz_k_ngp_frame_spp launch that rendered the frame (0: the S = 1 kernels did)

struct LzNgpFrameArgs {
    const void* packed;          // PREC 0: LZ_NGP_FRAGS * 64 floats; 1: LZ_NGP_PACKED_F16_BYTES of half fragments
    const void* emb;             // hash table, f32 or half [offsets[16], 2]
    const int* offsets;          // [17]
    LzGridLevels lv;
    float inv2b;                 // 1.0f / (2 bound): lz_map01's factor
};

// slot state in LDS, per wave [field][NS]
enum { NF_RAY = 0, NF_T, NF_FAR, NF_DT, NF_WS, NF_D, NF_R, NF_G, NF_B, NF_CNT,
       NF_RD,                    // 1 / direction (3), origin (3), direction (3): LzMarch::init reads LDS
       NF_SH = NF_RD + 9 };      // SH(4) of the direction: 16 floats (f32 head) or 8 words of packed halves (f16 head); behind it the
                                 // f16 head's parked outputs (rgb[0], rgb[1], rgb[2], sigma: they come out on two lane halves)
// level records in LDS, [field][16]
enum { NL_OFF0 = 0, NL_HS, NL_RES, NL_SCALE, NL_MODE, NL_FIELDS };

// words of the weight image in front of the level records (PREC 0: f32 fragments; 1: half fragments)
template <int PREC> struct LznfLds {
    static constexpr int W_WORDS = PREC == 1 ? LZN16_FRAGS * 64 * 4 : LZ_NGP_FRAGS * 64;
    static constexpr int FIXED_WORDS = W_WORDS + NL_FIELDS * LZNF_LEVELS + LZF_LUT;     // weights, level records, Morton table
};

// slot `sl` of a wave takes ray `ray` off the queue: start / end time, accumulators (zero, or what phase 1 parked in the output arrays),
// the march's per-ray constants and SH(4) of the direction the march hands every sample of the ray (lz_loop_march: dirs = rays_d) -- ONCE
// per ray.  NS: the stride of a field.
template <int PREC, int NS>
__device__ __forceinline__ void lznf_take_ray(const LzFrameK& F, bool ph2, int ray, int cnt_base, float* slot, int sl) {
    int* sloti = reinterpret_cast<int*>(slot);
    sloti[NF_RAY * NS + sl] = ray;
    slot[NF_T * NS + sl] = F.rays_t[ray];
    slot[NF_FAR * NS + sl] = F.occ ? F.t_end[ray] : F.fars[ray];     // the march's end: clipped to the occupied cells' box
    if (ph2) {                                   // the accumulators phase 1 parked in the output arrays
        slot[NF_WS * NS + sl] = F.weights_sum[ray];
        slot[NF_D * NS + sl] = F.depth[ray];
        slot[NF_R * NS + sl] = F.image[(size_t)ray * 3];
        slot[NF_G * NS + sl] = F.image[(size_t)ray * 3 + 1];
        slot[NF_B * NS + sl] = F.image[(size_t)ray * 3 + 2];
    } else {
#pragma unroll
        for (int f = NF_WS; f <= NF_B; f++) slot[f * NS + sl] = 0.0f;
    }
    sloti[NF_CNT * NS + sl] = cnt_base;
    const float* ro = F.rays_o + (size_t)ray * 3;
    const float* rd = F.rays_d + (size_t)ray * 3;
    const float d0 = rd[0], d1 = rd[1], d2 = rd[2];
    slot[NF_RD * NS + sl] = 1 / d0; slot[(NF_RD + 1) * NS + sl] = 1 / d1; slot[(NF_RD + 2) * NS + sl] = 1 / d2;
    slot[(NF_RD + 3) * NS + sl] = ro[0]; slot[(NF_RD + 4) * NS + sl] = ro[1]; slot[(NF_RD + 5) * NS + sl] = ro[2];
    slot[(NF_RD + 6) * NS + sl] = d0; slot[(NF_RD + 7) * NS + sl] = d1; slot[(NF_RD + 8) * NS + sl] = d2;
    float sh[16];
    lz_sh_eval(d0, d1, d2, 4, sh, nullptr, nullptr, nullptr);
    if constexpr (PREC == 1) {
#pragma unroll
        for (int k = 0; k < 8; k++) slot[(NF_SH + k) * NS + sl] = __uint_as_float(h_cvt2(sh[2 * k], sh[2 * k + 1], false));
    } else {
#pragma unroll
        for (int k = 0; k < 16; k++) slot[(NF_SH + k) * NS + sl] = sh[k];
    }
}

// the march of slot `sl` set up from its LDS fields
template <int NS>
__device__ __forceinline__ void lznf_march_init(LzMarch& m, const LzFrameK& F, const float* slot, int sl, bool use_lut, const uint32_t* mlut) {
    const float go[3] = {slot[(NF_RD + 3) * NS + sl], slot[(NF_RD + 4) * NS + sl], slot[(NF_RD + 5) * NS + sl]};
    const float gd[3] = {slot[(NF_RD + 6) * NS + sl], slot[(NF_RD + 7) * NS + sl], slot[(NF_RD + 8) * NS + sl]};
    m.init(go, gd, slot[NF_RD * NS + sl], slot[(NF_RD + 1) * NS + sl], slot[(NF_RD + 2) * NS + sl], F.bound, F.dt_gamma, F.mf, F.C, F.H, F.grid);
    if (use_lut) m.morton_lut = mlut;
}

// four levels l0 + i * dl of the sample at xin (unit cube): all 32 corner loads in flight, then the interpolation.  out[i]: both channels
template <typename TT>
__device__ __forceinline__ void lznf_gather4(const TT* table, const uint32_t* lvtab, const float (&xin)[3], int l0, int dl, LzVec<TT, 2> (&out)[4]) {
    LzGridCell<3> cell[4];
    LzVec<TT, 2> cv[4][8];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int l = l0 + dl * i;
        LzGridLevel lvl;
        lvl.off0 = lvtab[NL_OFF0 * LZNF_LEVELS + l]; lvl.hs = lvtab[NL_HS * LZNF_LEVELS + l]; lvl.res = lvtab[NL_RES * LZNF_LEVELS + l];
        lvl.scale = __uint_as_float(lvtab[NL_SCALE * LZNF_LEVELS + l]); lvl.mode = lvtab[NL_MODE * LZNF_LEVELS + l];
        cell[i] = lz_grid_cell<3, true>(xin, lvl.scale, false);
        uint32_t index[8];
        lz_grid_corner_offsets<3>(lvl, cell[i], 2u, 0u, false, index);
        const TT* g = table + (size_t)lvl.off0 * 2;
#pragma unroll
        for (int c = 0; c < 8; c++) __builtin_memcpy(&cv[i][c], __builtin_assume_aligned(g + index[c], sizeof(TT) * 2), sizeof(TT) * 2);
    }
#pragma unroll
    for (int i = 0; i < 4; i++) out[i] = lz_grid_interp<TT, 3, 2>(cell[i], cv[i]);
}

// ---- host side: lz_ngp_frame.hip owns the C entries and the S = 1 launch, lz_ngp_frame_spp.hip the S > 1 kernels and the auto rule ----
// launch lz_k_ngp_frame_spp<variant, S> (variant: 0 = f32 tables + f32 head, 1 = half tables + f16 head, 2 = half tables + f32 head; S in 2, 4, 8, 16)
void lznf_spp_launch(int variant, uint32_t S, uint32_t N, const LzNgpFrameArgs& a, const LzFrameK& K, hipStream_t st);
// steps_per_pass = 0: S from the ray count, the head's slot width, the CU count and the cap
uint32_t lznf_spp_auto(int variant, uint32_t N, uint32_t max_steps);
#endif
