// lz_ngp16_chain.h -- the f16 cfg2 network of one 32-sample slice as a device function, shared by the stand-alone head (lz_ngp.hip:
// lz_k_ngp_head16) and the persistent frame kernel (lz_ngp_frame.hip): same fragments, same k order, same bits.  The arithmetic and the
// operand layout are described at lz_k_ngp_head16.
#ifndef LZ_NGP16_CHAIN_H
#define LZ_NGP16_CHAIN_H
#include "lz_head_f16w_slice.h"   // the 32x32x16 f16 operand layout, w_pack / w_zero, h_cvt2 / h_round
#include "lzzx_sh_eval.h"
#include <hip/hip_fp16.h>

#define LZN16_S1 0     // fragment bases (fragment (ks, ft) at base + ks * NT + ft; 64 lanes x 8 halves each)
#define LZN16_S2 4
#define LZN16_C1 8
#define LZN16_C2 12
#define LZN16_FRAGS 16
static_assert(LZN16_FRAGS * 64 * 16 == LZ_NGP_PACKED_F16_BYTES, "half image size mismatch with the header");

template <int KS, int NT>
__device__ __forceinline__ void lzn16_layer(const lz_h8* __restrict__ frags, int lane, const lz_h8 (&b)[KS], lz_f16v (&acc)[NT]) {
#pragma unroll
    for (int ft = 0; ft < NT; ft++) acc[ft] = w_zero();
#pragma unroll
    for (int ks = 0; ks < KS; ks++)
#pragma unroll
        for (int ft = 0; ft < NT; ft++) acc[ft] = __builtin_amdgcn_mfma_f32_32x32x16_f16(frags[(ks * NT + ft) * 64 + lane], b[ks], acc[ft], 0, 0, 0);
}

// the SH(4) components 8 h .. 8 h + 7 as four words of packed halves: k-step 0 of colour_net.0 on lane half h
__device__ __forceinline__ void lzn16_sh_words(const float (&sh)[16], int h, uint32_t (&w)[4]) {
#pragma unroll
    for (int j = 0; j < 4; j++) w[j] = h_cvt2(h ? sh[8 + 2 * j] : sh[2 * j], h ? sh[9 + 2 * j] : sh[1 + 2 * j], false);
}

// lane (s = lane & 31, h = lane >> 5).  f: the eight feature words (half2: both channels) of levels 8 ks + 4 h + i at f[4 ks + i]; shw:
// lzn16_sh_words of the sample's direction.  Leaves rgb channel h in rgb_a and, in b_out, channel 2 (h = 0) or sigma (h = 1).
__device__ __forceinline__ void lzn16_chain(const lz_h8* __restrict__ wl, int lane, int h, const uint32_t (&f)[8], const uint32_t (&shw)[4],
                                            float& rgb_a, float& b_out) {
    // ---------------- sigma_net: 32 -> 64 (ReLU) -> 16 ----------------
    lz_h8 b1[2];
#pragma unroll
    for (int ks = 0; ks < 2; ks++) {
        const lz_u4v w = {f[4 * ks], f[4 * ks + 1], f[4 * ks + 2], f[4 * ks + 3]};
        b1[ks] = __builtin_bit_cast(lz_h8, w);
    }
    lz_f16v s1[2];
    lzn16_layer<2, 2>(wl + LZN16_S1 * 64, lane, b1, s1);
    const lz_h8 b2[4] = {w_pack(s1[0], 0, true), w_pack(s1[0], 1, true), w_pack(s1[1], 0, true), w_pack(s1[1], 1, true)};
    lz_f16v s2[1];
    lzn16_layer<4, 1>(wl + LZN16_S2 * 64, lane, b2, s2);
    // ---------------- colour_net: [SH(4) | sigma_net's 16 outputs, sigma's weighted 0] -> 64 (ReLU) -> 3 ----------------
    lz_h8 c1in[2];
    {
        const lz_u4v w = {shw[0], shw[1], shw[2], shw[3]};
        c1in[0] = __builtin_bit_cast(lz_h8, w);
    }
    c1in[1] = w_pack(s2[0], 0, false);
    lz_f16v c1[2];
    lzn16_layer<2, 2>(wl + LZN16_C1 * 64, lane, c1in, c1);
    const lz_h8 c2in[4] = {w_pack(c1[0], 0, true), w_pack(c1[0], 1, true), w_pack(c1[1], 0, true), w_pack(c1[1], 1, true)};
    lz_f16v c2[1];
    lzn16_layer<4, 1>(wl + LZN16_C2 * 64, lane, c2in, c2);
    // ---------------- two transcendentals per lane, one instruction sequence each ----------------
    // chain A: colour channel h (register 0).  chain B: channel 2 (register 1) on h = 0, sigma on h = 1.  sigmoid(x) = 1 / (1 + exp(-x))
    // is lz_sigmoidf's own sequence, so both chains are lz_expf / lz_sigmoidf bit for bit.
    const float pa = (float)h_round(c2[0][0]);
    const float pb = h ? (float)h_round(s2[0][0]) : (float)h_round(c2[0][1]);
    const float ea = lz_expf(-pa), eb = lz_expf(h ? pb : -pb);
    rgb_a = (float)h_round(1.0f / (1.0f + ea));
    b_out = h ? eb : (float)h_round(1.0f / (1.0f + eb));
}
#endif
