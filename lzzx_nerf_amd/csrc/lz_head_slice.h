// lz_head_slice.h -- the f32 fused triplane head for ONE 16-sample slice of a wave (v_mfma_f32_16x16x4_f32), shared by the stand-alone
// head kernel (lz_head.hip: lz_k_triplane_head) and the fused frame kernel (lz_frame.hip: lz_k_frame), so that both evaluate
// NeRFNetwork.forward (nerf_triplane/network.py:252-311) with the same instruction sequence, bit for bit.  Lane (s = lane & 15,
// q = lane >> 4) owns sample s and a quarter of its features; see lz_head.hip for the layer chaining and the summation orders.
// NeRFNetwork.density (lz_density.hip) is the same function cut off behind sigma_net by a compile-time switch (CUT, below).
#ifndef LZ_HEAD_SLICE_H
#define LZ_HEAD_SLICE_H
#include "lz_common.h"
#include "lzzx_detmath.h"
#include "lzzx_sh_eval.h"
#include "lz_head_gather.h"
#include "lz_head_layers.h"

#define LZ_T 1             // sample tiles (of 16) per wave pass

// per-workgroup context: the packed weights and small tables staged in LDS (lz_head_stage), per-launch constants
struct LzHeadCtx {
    const float* wl;        // LDS: packed A fragments, then the VALU-layer rows
    const int* tab;         // LDS: the level table (lz_head_gather.h: LZ_LVTAB_*)
    const float* lenca;     // LDS: enc_a [32]
    const float* emb[3];    // the three planes' tables (global)
    float bound, two_bound, eye_v, indq;
    const float* lind;      // LDS: ind_code [4] (0 without one)
    bool has_eye, has_ind;
    bool young;             // lz_wave_prio (lz_head_gather.h): the fused frame kernel sets it per wave, false elsewhere
};

struct LzHeadOut {
    float sigma, rgb[3], ambaud, eyeatt, unc;   // every lane of a sample ends with the same bits
};

// LDS floats the stage needs: fragments + VALU rows + the level table (lz_head_gather.h: LZ_LVTAB_WORDS, enc_a inside)
template <bool TRAIN_UNC>
struct LzHeadLds {
    static constexpr int NFRAG = TRAIN_UNC ? LZ_FRAGS_ALL : LZ_FRAGS_INFER;
    static constexpr int WV = NFRAG * 64, TAB = WV + LZ_WV_FLOATS, FLOATS = TAB + LZ_LVTAB_WORDS;
};

// stage weights + tables into LDS (all threads of the workgroup; caller synchronises afterwards) and fill the context
template <bool TRAIN_UNC>
__device__ __forceinline__ void lz_head_stage(const LzHeadArgs& P, float* wl, uint32_t n_threads, int q, LzHeadCtx& hc) {
    using L = LzHeadLds<TRAIN_UNC>;
    const float4* src = reinterpret_cast<const float4*>(P.packed);
    float4* dst = reinterpret_cast<float4*>(wl);
    for (uint32_t i = threadIdx.x; i < (uint32_t)L::NFRAG * 16; i += n_threads) dst[i] = src[i];   // 16 B per lane per step, coalesced
    if (threadIdx.x < LZ_WV_FLOATS) wl[L::WV + threadIdx.x] = P.packed[LZ_FRAGS_ALL * 64 + threadIdx.x];
    // per-level table (indexed per lane in the gather) + the slice queue head of the stand-alone kernel
    int* tab = reinterpret_cast<int*>(wl + L::TAB);
    lz_level_table_fill(tab, P.offsets, P.scale, P.res);
    if (threadIdx.x < 32) wl[L::TAB + LZ_LVTAB_ENCA + threadIdx.x] = P.enc_a[threadIdx.x];
    hc.wl = wl;
    hc.tab = tab;
    hc.lenca = wl + L::TAB + LZ_LVTAB_ENCA;
    hc.emb[0] = P.emb[0]; hc.emb[1] = P.emb[1]; hc.emb[2] = P.emb[2];
    hc.bound = P.bound;
    hc.two_bound = 2.0f * P.bound;
    hc.has_eye = P.eye != nullptr;
    hc.eye_v = hc.has_eye ? P.eye[0] : 0.0f;
    hc.indq = P.ind_code ? P.ind_code[q] : 0.0f;
    hc.has_ind = P.ind_code != nullptr;
    if (threadIdx.x < 4) wl[L::TAB + LZ_LVTAB_IND + threadIdx.x] = P.ind_code ? P.ind_code[threadIdx.x] : 0.0f;
    hc.lind = wl + L::TAB + LZ_LVTAB_IND;
    hc.young = false;
}

// SH(4) source that evaluates the polynomials from a direction fetched on demand (the stand-alone kernels: dirs are per sample)
template <typename DirFn>
struct LzShFromDir {
    DirFn dirfn;
    float o[16];
    static constexpr bool C1_PARTIAL = false;    // the slice runs all of colour_net.0
    __device__ __forceinline__ explicit LzShFromDir(DirFn f) : dirfn(f) {}
    __device__ __forceinline__ void issue(int) {}
    __device__ __forceinline__ void prepare() {
        float dx, dy, dz;
        dirfn(dx, dy, dz);
        lz_sh_eval(dx, dy, dz, 4, o, nullptr, nullptr, nullptr);
    }
    __device__ __forceinline__ float comp_iq(int i, int q) const {    // component 4 i + q (i compile-time after unrolling)
        return q == 0 ? o[4 * i] : (q == 1 ? o[4 * i + 1] : (q == 2 ? o[4 * i + 2] : o[4 * i + 3]));
    }
    __device__ __forceinline__ float comp_qj(int q, int j) const {    // component 4 q + j
        return q == 0 ? o[j] : (q == 1 ? o[4 + j] : (q == 2 ? o[8 + j] : o[12 + j]));
    }
};
template <typename DirFn>
__device__ __forceinline__ LzShFromDir<DirFn> lz_sh_from_dir(DirFn f) { return LzShFromDir<DirFn>(f); }

// Per-ray SH partial of colour_net.0.  The layer's input is [SH 16 | geo 64 | ind 4] and its accumulators start at zero, so after k-step 3
// (the 16 SH components) they hold an fma chain over the view direction and the weights alone: the same bits for every sample of a ray.
// lz_c1_sh_partial runs those 4 k-steps x 4 tiles once for 16 rays (lane (s, q): ray s); the fused frame stores the result per ray, 64 f32
// in the lane order the slice consumes -- lane (s, q) owns features 16 ft + 4 q + r at floats 16 q + 4 ft + r of its ray's row, 4 x 16 B --
// and its slices resume the chain at k-step 4 (LzShPartial).  Same instruction, same operands, same order: nothing moves by a bit.
constexpr int LZ_C1_SH_KS = 4;             // k-steps of colour_net.0 that consume SH only
constexpr int LZ_C1_SH_FLOATS = 64;        // per ray
template <typename ShFn>
__device__ __forceinline__ void lz_c1_sh_partial(const float* __restrict__ wl, int lane, ShFn& sh, lz_f4 (&acc)[4][1]) {
    const int q = lane >> 4;
    float b[1][LZ_KS[LZ_L_C1]];
    sh.prepare();
#pragma unroll
    for (int i = 0; i < LZ_KS[LZ_L_C1]; i++) b[0][i] = i < LZ_C1_SH_KS ? sh.comp_iq(i, q) : 0.0f;
#pragma unroll
    for (int ft = 0; ft < 4; ft++) acc[ft][0] = lz_f4{0, 0, 0, 0};
    lz_layer_ks<LZ_L_C1, 1, 0, LZ_C1_SH_KS>(wl, lane, b, acc);
}
// the slice's SH source when the partial exists: `row` = this lane's 16 floats of its ray's partial (null: no ray in the slot -- the
// sample's outputs are discarded).  issue() starts the 4 loads well ahead of colour_net.0 (the other waves' MFMAs cover them).
struct LzShPartial {
    static constexpr bool C1_PARTIAL = true;
    const float* row;
    lz_f4 p[4];
    __device__ __forceinline__ void issue(int) {
#pragma unroll
        for (int ft = 0; ft < 4; ft++) p[ft] = row ? *reinterpret_cast<const lz_f4*>(row + 4 * ft) : lz_f4{0, 0, 0, 0};
    }
    __device__ __forceinline__ lz_f4 part(int ft) const { return p[ft]; }
};

// The slice's ReLU as ONE integer instruction (v_max_i32): max((int)bits(v), 0).  lz_relu (`v > 0 ? v : 0`) on an MFMA result compiles to
// two v_max_f32 -- a canonicalising v_max_f32 v, v, v, which the compiler cannot prove away for MFMA outputs, and the maximum itself -- 68
// times per slice between the MFMAs.  Same bits for every f32 that is no NaN: -0 and every negative value have the sign bit set, a negative
// integer, and become +0; +0, positive denormals, normals and +inf are positive integers and pass.  A NaN of positive sign PASSES (lz_relu
// turns every NaN into 0; np.maximum in oracle/head.py passes it too); a NaN of negative sign becomes +0.  For lz_head_slice only: the
// training chains keep lz_relu (the shared helper changed this way costs lz_k_triplane_head_forward_rec 32 registers and a spill).
// LZ_SLICE_RELU_I32 = 0 restores lz_relu (A/B switch).
#ifndef LZ_SLICE_RELU_I32
#define LZ_SLICE_RELU_I32 1
#endif
__device__ __forceinline__ float lz_slice_relu(float v) {
#if LZ_SLICE_RELU_I32
    const int b = (int)__float_as_uint(v);
    return __uint_as_float((uint32_t)(b > 0 ? b : 0));
#else
    return lz_relu(v);
#endif
}

// Behind each ReLU block of the slice: no vector instruction and no MFMA crosses (scalar, LDS and memory instructions do).  Left alone the
// scheduler deals the ReLUs out one by one among the next layer's MFMAs, and beside f32 MFMAs it is OPENING a gap that is dear -- 7 cycles
// per MFMA and SIMD for the first vector instruction of a gap, 2 to 2.5 for each further one (tools/probes/mfma_f32_fill_probe.hip).  With
// the fence a layer's ReLUs stand together: gaps holding one vector instruction 39 -> 17 in lz_k_frame<0, 1, 1>, 120 -> 117 VGPRs, the
// frame 0.3 % faster in every run of an A/B.  LZ_SLICE_RELU_FENCE = 0 takes it out (A/B switch).
#ifndef LZ_SLICE_RELU_FENCE
#define LZ_SLICE_RELU_FENCE 1
#endif
__device__ __forceinline__ void lz_slice_relu_fence() {
#if LZ_SLICE_RELU_FENCE
    __builtin_amdgcn_sched_barrier(0x94);
#endif
}

// The vector instructions that still stood alone between two MFMAs of the wave's own chain (17 in lz_k_frame<0, 1, 1>; tools/isa_census.py
// --gaps names them) were of two kinds.  Five v_mul_f32 of the sigma net's enc_a * att inputs, which the scheduler sinks to the k-step that
// consumes each: a fence behind the eight products keeps them ahead of the layer's first MFMA.  Twelve v_max_i32 of sigma_net.0's ReLU:
// the SH partial's loads (LzShPartial::issue: a load under a per-lane condition, so a branch) stood between the ReLU block's fence and
// sigma_net.1, a scheduling barrier holds only inside its basic block, and the ReLUs had been sunk into the block behind the branch.  The
// loads are issued ahead of the ReLU block instead.  LZ_SLICE_GAP_FENCE = 0 restores the former order (A/B switch).
#ifndef LZ_SLICE_GAP_FENCE
#define LZ_SLICE_GAP_FENCE 1
#endif

// one slice: (px, py, pz) = this lane's sample position; shfn supplies SH(4) of its view direction when the colour net needs it
// (LzShFromDir: evaluated here from the direction, like the reference per sample), or the colour net's SH partial of the sample's ray
// (LzShPartial: the fused frame kernel, which evaluates k-steps 0 .. 3 of colour_net.0 once per ray)
// FOLD (inference only): geo = Wg s2 feeds colour_net.0 with nothing but a linear map in between (network.py:304-306), so
// W_c0[:, geo] (Wg s2) = (W_c0[:, geo] Wg) s2: the host packs the 64 x 64 product into colour_net.0's geo columns (head.py: fold_geo) and
// the slice hands s2 to the colour net directly -- 64 of the 361 MFMAs per slice are never issued.  sigma (the VALU row of sigma_net.2 on
// s2) is unchanged bit for bit; rgb moves by the reassociation, a few 1e-7.
// CUT: NeRFNetwork.density (network.py:283-311), the slice cut off behind sigma_net (lz_density.hip).  LZ_CUT_DENSITY stops at the sigma
// row: no geo rows of sigma_net.2, no SH, no colour net, no uncertainty constant; out.sigma / ambaud / eyeatt are the full slice's bits
// (the same fragments in the same k order; sigma = lz_expf on the same argument).  LZ_CUT_DENSITY_GEO also runs the geo rows and hands
// this lane's 16 geo_feat values (feature 16 ft + 4 q + r at [4 ft + r]) to `geo_out`.  out.rgb / out.unc are not written.
enum { LZ_CUT_NONE = 0, LZ_CUT_DENSITY = 1, LZ_CUT_DENSITY_GEO = 2 };
// the SH source of a cut slice: nothing asks it for a value
struct LzShNone {
    static constexpr bool C1_PARTIAL = false;
    __device__ __forceinline__ void issue(int) {}
    __device__ __forceinline__ void prepare() {}
    __device__ __forceinline__ float comp_iq(int, int) const { return 0.0f; }
    __device__ __forceinline__ float comp_qj(int, int) const { return 0.0f; }
};
template <bool TRAIN_UNC, bool FOLD = false, bool IN_RANGE = false, bool YIELD = false, int CUT = LZ_CUT_NONE, typename ShFn>
__device__ __forceinline__ void lz_head_slice(const LzHeadCtx& hc, int lane, float px, float py, float pz, ShFn shfn, LzHeadOut& out,
                                              float* geo_out = nullptr) {
    static_assert(!(TRAIN_UNC && FOLD), "the folded colour net is an inference arrangement");
    static_assert(CUT == LZ_CUT_NONE || !(TRAIN_UNC || FOLD), "a density query has neither an uncertainty net nor a colour net to fold into");
    constexpr int WV = LzHeadLds<TRAIN_UNC>::WV;
    const int q = lane >> 4;
    // ---------------- gather: enc_x features f = 4i + q of sample s -> B operands (lz_head_gather.h) ----------------
    float encx[LZ_T][9];
    lz_head_gather<IN_RANGE, LZ_GATHER_PACK32, YIELD, true>(hc.emb, hc.tab, px, py, pz, q, hc.bound, hc.two_bound, encx[0], hc.young);
    __builtin_amdgcn_sched_barrier(0);  // the tile's 36 reads in flight at a time: bounds the register footprint

    // ---------------- audio channel attention: 36 -> 64 -> 32 ----------------
    float att[LZ_T][8];   // chained layout: [t*4 + r] = feature 16t + 4q + r
    {
        lz_f4 acc1[4][LZ_T];
#pragma unroll
        for (int ft = 0; ft < 4; ft++)
#pragma unroll
            for (int j = 0; j < LZ_T; j++) acc1[ft][j] = lz_f4{0, 0, 0, 0};
        lz_layer<LZ_L_A1, LZ_T>(hc.wl, lane, encx, acc1);
        float b2[LZ_T][16];
#pragma unroll
        for (int j = 0; j < LZ_T; j++)
#pragma unroll
            for (int ft = 0; ft < 4; ft++)
#pragma unroll
                for (int r = 0; r < 4; r++) b2[j][4 * ft + r] = lz_slice_relu(acc1[ft][j][r]);
        lz_slice_relu_fence();
        lz_f4 acc2[2][LZ_T];
#pragma unroll
        for (int ft = 0; ft < 2; ft++)
#pragma unroll
            for (int j = 0; j < LZ_T; j++) acc2[ft][j] = lz_f4{0, 0, 0, 0};
        lz_layer<LZ_L_A2, LZ_T>(hc.wl, lane, b2, acc2);
#pragma unroll
        for (int j = 0; j < LZ_T; j++)
#pragma unroll
            for (int ft = 0; ft < 2; ft++)
#pragma unroll
                for (int r = 0; r < 4; r++) att[j][4 * ft + r] = acc2[ft][j][r];
    }
    // ambient_aud = || att ||_2 : sum of squares in the lane-partial order (att is its own weight row), then sqrt
    float ambaud[LZ_T];
#pragma unroll
    for (int j = 0; j < LZ_T; j++) {
        float acc = 0.0f;
#pragma unroll
        for (int k = 0; k < 8; k++) acc = lz_fmaf(att[j][k], att[j][k], acc);
        acc += __shfl_xor(acc, 16, 64);
        acc += __shfl_xor(acc, 32, 64);
        ambaud[j] = sqrtf(acc);
    }
    // ---------------- eye attention: 36 -> 16 -> 1, sigmoid ----------------
    float eyeatt[LZ_T];
#pragma unroll
    for (int j = 0; j < LZ_T; j++) eyeatt[j] = 0.0f;
    if (hc.has_eye) {
        lz_f4 acce[1][LZ_T];
#pragma unroll
        for (int j = 0; j < LZ_T; j++) acce[0][j] = lz_f4{0, 0, 0, 0};
        lz_layer<LZ_L_E1, LZ_T>(hc.wl, lane, encx, acce);
        float be[LZ_T][4];
#pragma unroll
        for (int j = 0; j < LZ_T; j++)
#pragma unroll
            for (int r = 0; r < 4; r++) be[j][r] = lz_slice_relu(acce[0][j][r]);
        lz_slice_relu_fence();
#pragma unroll
        for (int j = 0; j < LZ_T; j++) eyeatt[j] = lz_sigmoidf(lz_lane_dot<1>(hc.wl + WV + LZ_WV_E2, q, be[j]));
    }
    // ---------------- uncertainty ----------------
    float uncv[LZ_T];
    if constexpr (TRAIN_UNC) {
        lz_f4 accu[2][LZ_T];
#pragma unroll
        for (int ft = 0; ft < 2; ft++)
#pragma unroll
            for (int j = 0; j < LZ_T; j++) accu[ft][j] = lz_f4{0, 0, 0, 0};
        lz_layer<LZ_L_U1, LZ_T>(hc.wl, lane, encx, accu);
        float bu[LZ_T][8];
#pragma unroll
        for (int j = 0; j < LZ_T; j++)
#pragma unroll
            for (int ft = 0; ft < 2; ft++)
#pragma unroll
                for (int r = 0; r < 4; r++) bu[j][4 * ft + r] = lz_slice_relu(accu[ft][j][r]);
        lz_slice_relu_fence();
#pragma unroll
        for (int j = 0; j < LZ_T; j++) uncv[j] = lz_softplusf(lz_lane_dot<2>(hc.wl + WV + LZ_WV_U2, q, bu[j]));
    } else if constexpr (CUT == LZ_CUT_NONE) {
#pragma unroll
        for (int j = 0; j < LZ_T; j++) uncv[j] = lz_softplusf(0.0f);   // network.py:243-249, 278
    }
    // ---------------- sigma net: [enc_x 36 | enc_a * att 32 | eye * eye_att 1] -> 64 -> 64 -> 65 ----------------
    float geo[LZ_T][16];
    float sig_pre[LZ_T];      // row 0 of sigma_net.2, before the exp (evaluated with the colours' sigmoids at the end)
    {
        float b1[LZ_T][18];
#pragma unroll
        for (int j = 0; j < LZ_T; j++) {
#pragma unroll
            for (int i = 0; i < 9; i++) b1[j][i] = encx[j][i];
#pragma unroll
            for (int t = 0; t < 2; t++)
#pragma unroll
                for (int r = 0; r < 4; r++) b1[j][9 + 4 * t + r] = hc.lenca[16 * t + 4 * q + r] * att[j][4 * t + r];
            b1[j][17] = 0.0f;           // (k-step 17 runs on the VALU below)
        }
        if constexpr (LZ_SLICE_GAP_FENCE != 0) lz_slice_relu_fence();
        lz_f4 acc1[4][LZ_T];
#pragma unroll
        for (int ft = 0; ft < 4; ft++)
#pragma unroll
            for (int j = 0; j < LZ_T; j++) acc1[ft][j] = lz_f4{0, 0, 0, 0};
        lz_layer_ks<LZ_L_S1, LZ_T, 0, 17>(hc.wl, lane, b1, acc1);
        // k-step 17 = [eye * eye_att | 0 0 0] (input 68, then padding) and the last link of the chain: its MFMA adds W[n, 68] e on top of
        // k-step 16, then three products 0 * 0, which can flip nothing but the sign of a zero accumulator -- and the ReLU behind maps both
        // zeros to +0.  So it is one fma per output feature on the VALU: every lane of a sample holds the same eyeatt bits (lz_lane_dot),
        // and lane (s, q) needs W[16 ft + 4 q + r, 68] = entries 4 q .. 4 q + 3 of the A fragment (17, ft): one 16-byte LDS read per tile,
        // 16 fmas instead of 4 MFMAs.  Without the eye input the k-step adds zeros only: skipped.
        if (hc.has_eye) {
            const float* w68 = hc.wl + (lz_frag_base(LZ_L_S1) + 17 * LZ_NT[LZ_L_S1]) * 64 + 4 * q;
#pragma unroll
            for (int j = 0; j < LZ_T; j++) {
                const float e = hc.eye_v * eyeatt[j];
#pragma unroll
                for (int ft = 0; ft < 4; ft++) {
                    const lz_f4 w = *reinterpret_cast<const lz_f4*>(w68 + 64 * ft);
#pragma unroll
                    for (int r = 0; r < 4; r++) acc1[ft][j][r] = lz_fmaf(w[r], e, acc1[ft][j][r]);
                }
            }
        }
        // the per-ray SH partial of colour_net.0 (LzShPartial): its loads fly under sigma_net.1 / .2
        if constexpr (LZ_SLICE_GAP_FENCE != 0) shfn.issue(q);
        float b2[LZ_T][16];
#pragma unroll
        for (int j = 0; j < LZ_T; j++)
#pragma unroll
            for (int ft = 0; ft < 4; ft++)
#pragma unroll
                for (int r = 0; r < 4; r++) b2[j][4 * ft + r] = lz_slice_relu(acc1[ft][j][r]);
        lz_slice_relu_fence();
        if constexpr (LZ_SLICE_GAP_FENCE == 0) shfn.issue(q);
        lz_f4 acc2[4][LZ_T];
#pragma unroll
        for (int ft = 0; ft < 4; ft++)
#pragma unroll
            for (int j = 0; j < LZ_T; j++) acc2[ft][j] = lz_f4{0, 0, 0, 0};
        lz_layer<LZ_L_S2, LZ_T>(hc.wl, lane, b2, acc2);
        float b3[LZ_T][16];
#pragma unroll
        for (int j = 0; j < LZ_T; j++)
#pragma unroll
            for (int ft = 0; ft < 4; ft++)
#pragma unroll
                for (int r = 0; r < 4; r++) b3[j][4 * ft + r] = lz_slice_relu(acc2[ft][j][r]);
        lz_slice_relu_fence();
        if constexpr (CUT == LZ_CUT_DENSITY) {
            // density without geo_feat: the 64 geo MFMAs are never issued
        } else if constexpr (FOLD) {
#pragma unroll
            for (int j = 0; j < LZ_T; j++)
#pragma unroll
                for (int k = 0; k < 16; k++) geo[j][k] = b3[j][k];   // s2 itself: the geo projection lives in the packed colour_net.0
        } else {
            lz_f4 acc3[4][LZ_T];
#pragma unroll
            for (int ft = 0; ft < 4; ft++)
#pragma unroll
                for (int j = 0; j < LZ_T; j++) acc3[ft][j] = lz_f4{0, 0, 0, 0};
            lz_layer<LZ_L_S3, LZ_T>(hc.wl, lane, b3, acc3);
#pragma unroll
            for (int j = 0; j < LZ_T; j++)
#pragma unroll
                for (int ft = 0; ft < 4; ft++)
#pragma unroll
                    for (int r = 0; r < 4; r++) geo[j][4 * ft + r] = acc3[ft][j][r];   // geo_feat, no activation (network.py:304)
        }
#pragma unroll
        for (int j = 0; j < LZ_T; j++) sig_pre[j] = lz_lane_dot<4>(hc.wl + WV + LZ_WV_SIG, q, b3[j]);     // row 0 of sigma_net.2 on the VALU
    }
    if constexpr (CUT != LZ_CUT_NONE) {   // density(): sigma = exp(h0) (network.py:302) on every lane of the sample; nothing below is reached
        out.sigma = lz_expf(sig_pre[0]);
        out.ambaud = ambaud[0];
        out.eyeatt = eyeatt[0];
        if constexpr (CUT == LZ_CUT_DENSITY_GEO) {
#pragma unroll
            for (int k = 0; k < 16; k++) geo_out[k] = geo[0][k];
        }
        return;
    }
    // ---------------- colour net: [SH 16 | geo 64 | ind 4] -> 64 -> 3 ----------------
    float rgb[LZ_T][3];
    {
        float b1[LZ_T][21];
        lz_f4 acc1[4][LZ_T];
#pragma unroll
        for (int j = 0; j < LZ_T; j++) {
            if constexpr (ShFn::C1_PARTIAL) {
                // k-steps 0 .. 3 done per ray (lz_c1_sh_partial): the chain resumes from their accumulators
#pragma unroll
                for (int i = 0; i < LZ_C1_SH_KS; i++) b1[j][i] = 0.0f;
#pragma unroll
                for (int ft = 0; ft < 4; ft++) acc1[ft][j] = shfn.part(ft);
            } else {
                // SH(4) of the view direction (constant per ray, recomputed per sample like the reference): this lane
                // keeps components 4i + q
                shfn.prepare();
#pragma unroll
                for (int i = 0; i < 4; i++) b1[j][i] = shfn.comp_iq(i, q);     // SH component 4 i + q
#pragma unroll
                for (int ft = 0; ft < 4; ft++) acc1[ft][j] = lz_f4{0, 0, 0, 0};
            }
#pragma unroll
            for (int k = 0; k < 16; k++) b1[j][4 + k] = geo[j][k];
            b1[j][20] = 0.0f;           // (k-step 20, ind_code, runs on the VALU below)
        }
        lz_layer_ks<LZ_L_C1, LZ_T, ShFn::C1_PARTIAL ? LZ_C1_SH_KS : 0, LZ_KS[LZ_L_C1] - 1>(hc.wl, lane, b1, acc1);
        // k-step 20 = the 4 ind_code inputs, the same for every sample and the last link of the chain: on the VALU, acc = fma(W[n, 80 + k],
        // ind[k], acc) for k = 0 .. 3 in the MFMA's order (an f32 MFMA is a k-ordered fma chain).  Lane (s, q) needs W[16 ft + 4 q + r, 80 + k]
        // = entries 16 k + 4 q .. 16 k + 4 q + 3 of the A fragment (20, ft): 16 ds_read_b128 and 64 fmas instead of 4 MFMAs (measured: the
        // f32 frame 1.1 % faster; the same move for a per-sample k-step, whose B values first cross lanes, was 3-6 % SLOWER).  Without
        // ind_code the k-step adds zeros only: skipped.  (The folded kernels kept this k-step on the matrix pipe while the VALU form spilled
        // them; built without the SLP vectoriser -- build.py: FILE_FLAGS -- it does not, and they issue 273 MFMAs per slice instead of 277.)
        if constexpr (YIELD && LZF_PRIO_TAIL != 0) lz_wave_prio(true, hc.young);     // the slice's vector tail, held through the compositing
        if (hc.has_ind) {
            const float* w80 = hc.wl + (lz_frag_base(LZ_L_C1) + 20 * LZ_NT[LZ_L_C1]) * 64 + 4 * q;
            const lz_f4 ind = *reinterpret_cast<const lz_f4*>(hc.lind);      // (one broadcast read)
#pragma unroll
            for (int j = 0; j < LZ_T; j++)
#pragma unroll
                for (int k = 0; k < 4; k++)
#pragma unroll
                    for (int ft = 0; ft < 4; ft++) {
                        const lz_f4 w = *reinterpret_cast<const lz_f4*>(w80 + 64 * ft + 16 * k);
#pragma unroll
                        for (int r = 0; r < 4; r++) acc1[ft][j][r] = lz_fmaf(w[r], ind[k], acc1[ft][j][r]);
                    }
        }
        float b2[LZ_T][16];
#pragma unroll
        for (int j = 0; j < LZ_T; j++)
#pragma unroll
            for (int ft = 0; ft < 4; ft++)
#pragma unroll
                for (int r = 0; r < 4; r++) b2[j][4 * ft + r] = lz_slice_relu(acc1[ft][j][r]);
        lz_slice_relu_fence();
        // colour_net.1 (64 -> 3) on the VALU (network.py:275), then the four transcendentals of a sample -- sigma = exp(h0) (network.py:302)
        // and three sigmoids (:310) -- ONE per lane instead of four per lane: after the lane-partial sums every lane of a sample holds all
        // four pre-activations, so lane q evaluates the q-th (q < 3: sigmoid = 1 / (1 + exp(-x)), q == 3: exp) with the same lz_expf on
        // the same argument -- the same bits -- and the sample's lanes fetch each other's result (~120 vector instructions per slice less;
        // the exp is a 30-instruction polynomial because its bits are part of the parity contract)
#pragma unroll
        for (int j = 0; j < LZ_T; j++) {
            float d[3];
#pragma unroll
            for (int c = 0; c < 3; c++) d[c] = lz_lane_dot<4>(hc.wl + WV + LZ_WV_C2 + 64 * c, q, b2[j]);
            const float arg = q == 0 ? -d[0] : (q == 1 ? -d[1] : (q == 2 ? -d[2] : sig_pre[j]));
            const float e = lz_expf(arg);
            const float v = q == 3 ? e : (1.0f / (1.0f + e)) * 1.002f - 0.001f;
            const int s0 = lane & 15;
#pragma unroll
            for (int c = 0; c < 3; c++) rgb[j][c] = __shfl(v, s0 + 16 * c, 64);
            sig_pre[j] = __shfl(v, s0 + 48, 64);      // now sigma itself
        }
    }
    out.sigma = sig_pre[0];
    out.rgb[0] = rgb[0][0]; out.rgb[1] = rgb[0][1]; out.rgb[2] = rgb[0][2];
    out.ambaud = ambaud[0];
    out.eyeatt = eyeatt[0];
    out.unc = uncv[0];
}
#endif
