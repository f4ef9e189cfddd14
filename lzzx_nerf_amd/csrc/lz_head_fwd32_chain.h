// lz_head_fwd32_chain.h -- the MLP part of the f32 TRAINING forward (v_mfma_f32_16x16x4_f32, 16-sample slices; the instruction sequence
// of lz_k_triplane_head<true>, so the outputs have the same bits) as ONE function of the slice's gathered enc_x, shared by
//   * the recording forward (lz_head_rec.hip: lz_k_triplane_head_forward_rec): its sink stores the X half of the record and the state
//     row to memory, and
//   * the recomputing f32 backward (lz_head_rec.hip: lz_k_triplane_head_backward_rec<0, 0, 0, 1>): its sink stores the same X
//     half and keeps the state row in registers.
// One source for both, so the values the backward differentiates are bit for bit the values the forward produced.
//
// Sink interface (one call per record slot, in this order; the eye call only with an eye input):
//   x_a1(a1)                     LZ_BWD_X_A1: aud_ch_att_net.1's input (chained layout, 16 values)
//   st_att(att)                  LZ_ST_ATT: att (8)
//   st_e1(e1)                    LZ_ST_E1: eye_att_net.1's input (4)
//   st_u1(u1)                    LZ_ST_U1: unc_net.1's input (8)
//   x_sig0(encx, encw, eterm)    LZ_BWD_X_SIG0: sigma_net.0's input [enc_x 36 | enc_a * att 32 | eye * eye_att 1] (the eye term on lanes q == 0)
//   x_s1(s1), x_s2(s2)           LZ_BWD_X_S1, LZ_BWD_X_S2C: sigma_net.1's / .2's inputs (16 each)
//   x_c1(sh0..sh3, indq)         LZ_BWD_X_S2C + 64 ..: colour_net.0's SH columns 4 i + q and ind_code[q] (geo = s2 . Wg^T is not stored:
//                                its weight gradient is finished from sum G_c1^T s2)
//   st_c1(c1)                    LZ_ST_C1: colour_net.1's input (16)
// The ReLU masks and the scalars (LZ_ST_MK, LZ_ST_CLR) come back in LzFwd32Out.
#ifndef LZ_HEAD_FWD32_CHAIN_H
#define LZ_HEAD_FWD32_CHAIN_H
#include "lz_head_bwd_common.h"
#include "lz_head_slice.h"
#include "lzzx_sh_eval.h"

struct LzFwd32Out {
    float norm, eyeatt, upre, sigma, cpre[3];                  // ||att||, eye attention, pre-activations of unc / (sigma = exp) / colour: on every lane of the sample
    uint32_t mk_a1, mk_s1, mk_s2, mk_c1, mk_u1, mk_e1;         // ReLU masks of this lane's values (bit k <-> chained index k)
};

// encx: the lane's nine gathered features 4 i + q; (dx, dy, dz): the sample's view direction; hc: lz_head_stage<true>'s context
template <typename Sink>
__device__ __forceinline__ void lz_fwd32_chain(const LzHeadCtx& hc, int lane, const float (&encx)[9], float dx, float dy, float dz, Sink& sink,
                                               LzFwd32Out& out) {
    const int q = lane >> 4;
    const float* wl = hc.wl;
    const float* wv = wl + LzHeadLds<true>::WV;
    const float bx[1][9] = {{encx[0], encx[1], encx[2], encx[3], encx[4], encx[5], encx[6], encx[7], encx[8]}};
    // audio channel attention
    float att[8];
    {
        lz_f4 acc1[4][1] = {{lz_f4{0, 0, 0, 0}}, {lz_f4{0, 0, 0, 0}}, {lz_f4{0, 0, 0, 0}}, {lz_f4{0, 0, 0, 0}}};
        lz_layer<LZ_L_A1, 1>(wl, lane, bx, acc1);
        float a1[1][16];
#pragma unroll
        for (int ft = 0; ft < 4; ft++)
#pragma unroll
            for (int r = 0; r < 4; r++) a1[0][4 * ft + r] = lz_relu(acc1[ft][0][r]);
        out.mk_a1 = lz_mask_pos(a1[0]);
        sink.x_a1(a1[0]);
        lz_f4 acc2[2][1] = {{lz_f4{0, 0, 0, 0}}, {lz_f4{0, 0, 0, 0}}};
        lz_layer<LZ_L_A2, 1>(wl, lane, a1, acc2);
#pragma unroll
        for (int ft = 0; ft < 2; ft++)
#pragma unroll
            for (int r = 0; r < 4; r++) att[4 * ft + r] = acc2[ft][0][r];
    }
    sink.st_att(att);
    {
        float acc = 0.0f;
#pragma unroll
        for (int k = 0; k < 8; k++) acc = lz_fmaf(att[k], att[k], acc);
        acc += __shfl_xor(acc, 16, 64);
        acc += __shfl_xor(acc, 32, 64);
        out.norm = sqrtf(acc);
    }
    // eye attention
    float eyeatt = 0.0f;
    out.mk_e1 = 0;
    if (hc.has_eye) {
        lz_f4 acce[1][1] = {{lz_f4{0, 0, 0, 0}}};
        lz_layer<LZ_L_E1, 1>(wl, lane, bx, acce);
        float e1[4];
#pragma unroll
        for (int r = 0; r < 4; r++) e1[r] = lz_relu(acce[0][0][r]);
        out.mk_e1 = lz_mask_pos(e1);
        sink.st_e1(e1);
        eyeatt = lz_sigmoidf(lz_lane_dot<1>(wv + LZ_WV_E2, q, e1));
    }
    out.eyeatt = eyeatt;
    // uncertainty
    {
        lz_f4 accu[2][1] = {{lz_f4{0, 0, 0, 0}}, {lz_f4{0, 0, 0, 0}}};
        lz_layer<LZ_L_U1, 1>(wl, lane, bx, accu);
        float u1[8];
#pragma unroll
        for (int ft = 0; ft < 2; ft++)
#pragma unroll
            for (int r = 0; r < 4; r++) u1[4 * ft + r] = lz_relu(accu[ft][0][r]);
        out.mk_u1 = lz_mask_pos(u1);
        sink.st_u1(u1);
        out.upre = lz_lane_dot<2>(wv + LZ_WV_U2, q, u1);
    }
    // sigma net
    float spre;
    float geo[1][16];
    {
        float b1[1][18];
#pragma unroll
        for (int i = 0; i < 9; i++) b1[0][i] = encx[i];
        float encw[8];
#pragma unroll
        for (int t = 0; t < 2; t++)
#pragma unroll
            for (int r = 0; r < 4; r++) encw[4 * t + r] = hc.lenca[16 * t + 4 * q + r] * att[4 * t + r];
#pragma unroll
        for (int k = 0; k < 8; k++) b1[0][9 + k] = encw[k];
        b1[0][17] = (hc.has_eye && q == 0) ? hc.eye_v * eyeatt : 0.0f;
        sink.x_sig0(encx, encw, b1[0][17]);
        lz_f4 acc1[4][1] = {{lz_f4{0, 0, 0, 0}}, {lz_f4{0, 0, 0, 0}}, {lz_f4{0, 0, 0, 0}}, {lz_f4{0, 0, 0, 0}}};
        lz_layer<LZ_L_S1, 1>(wl, lane, b1, acc1);
        float s1[1][16];
#pragma unroll
        for (int ft = 0; ft < 4; ft++)
#pragma unroll
            for (int r = 0; r < 4; r++) s1[0][4 * ft + r] = lz_relu(acc1[ft][0][r]);
        out.mk_s1 = lz_mask_pos(s1[0]);
        sink.x_s1(s1[0]);
        lz_f4 acc2[4][1] = {{lz_f4{0, 0, 0, 0}}, {lz_f4{0, 0, 0, 0}}, {lz_f4{0, 0, 0, 0}}, {lz_f4{0, 0, 0, 0}}};
        lz_layer<LZ_L_S2, 1>(wl, lane, s1, acc2);
        float s2[1][16];
#pragma unroll
        for (int ft = 0; ft < 4; ft++)
#pragma unroll
            for (int r = 0; r < 4; r++) s2[0][4 * ft + r] = lz_relu(acc2[ft][0][r]);
        out.mk_s2 = lz_mask_pos(s2[0]);
        sink.x_s2(s2[0]);
        lz_f4 acc3[4][1] = {{lz_f4{0, 0, 0, 0}}, {lz_f4{0, 0, 0, 0}}, {lz_f4{0, 0, 0, 0}}, {lz_f4{0, 0, 0, 0}}};
        lz_layer<LZ_L_S3, 1>(wl, lane, s2, acc3);
#pragma unroll
        for (int ft = 0; ft < 4; ft++)
#pragma unroll
            for (int r = 0; r < 4; r++) geo[0][4 * ft + r] = acc3[ft][0][r];
        spre = lz_lane_dot<4>(wv + LZ_WV_SIG, q, s2[0]);
    }
    // colour net
    {
        float o[16];
        lz_sh_eval(dx, dy, dz, 4, o, nullptr, nullptr, nullptr);
        float b1[1][21];
#pragma unroll
        for (int i = 0; i < 4; i++) b1[0][i] = q == 0 ? o[4 * i] : (q == 1 ? o[4 * i + 1] : (q == 2 ? o[4 * i + 2] : o[4 * i + 3]));
#pragma unroll
        for (int k = 0; k < 16; k++) b1[0][4 + k] = geo[0][k];
        b1[0][20] = hc.indq;
        sink.x_c1(b1[0][0], b1[0][1], b1[0][2], b1[0][3], hc.indq);
        lz_f4 acc1[4][1] = {{lz_f4{0, 0, 0, 0}}, {lz_f4{0, 0, 0, 0}}, {lz_f4{0, 0, 0, 0}}, {lz_f4{0, 0, 0, 0}}};
        lz_layer<LZ_L_C1, 1>(wl, lane, b1, acc1);
        float c1[16];
#pragma unroll
        for (int ft = 0; ft < 4; ft++)
#pragma unroll
            for (int r = 0; r < 4; r++) c1[4 * ft + r] = lz_relu(acc1[ft][0][r]);
        out.mk_c1 = lz_mask_pos(c1);
        sink.st_c1(c1);
#pragma unroll
        for (int c = 0; c < 3; c++) out.cpre[c] = lz_lane_dot<4>(wv + LZ_WV_C2 + 64 * c, q, c1);
    }
    out.sigma = lz_expf(spre);
}
#endif
