// lz_torso_net.h -- forward_torso (nerf_triplane/network.py:170-205) on the matrix cores, shared by the one-launch inference kernel
// (lz_torso.hip) and the training kernels (lz_torso_train.hip): one instance of the arithmetic, so both give the same bits.
#pragma once
#include "lz_common.h"
#include "lzzx_detmath.h"

#define LZ_TORSO_FREQ 34      // 2 + 2 * 2 * 8   (get_encoder('frequency', input_dim=2, multires=8), network.py:160)
#define LZ_TORSO_ANCHOR 42    // 6 + 2 * 6 * 3   (input_dim=6, multires=3, network.py:162)
#define LZ_TORSO_GRIDF 32     // 16 levels x 2   (tiledgrid, network.py:166)
#define LZ_TORSO_HID 32
#define LZ_PI_F 3.141592653589793f

struct LzTorsoArgs {
    lz_torso_params p;
    float scale[16];
    uint32_t res[16];
};

static inline LzTorsoArgs lzt_args(const lz_torso_params& p) {
    LzTorsoArgs a;
    a.p = p;
    for (int l = 0; l < 16; l++) {   // gridencoder.cu:125-126 on the host, same libm call as the CPU checker
        const float sc = exp2f((float)l * p.S) * (float)p.H - 1.0f;
        a.scale[l] = sc;
        a.res[l] = (uint32_t)ceilf(sc) + 1u;
    }
    return a;
}

// get_grid_index (gridencoder.cu:54-72), D = 2, generic form (tiled grids wrap with a true modulo).  The modulo itself is ~25
// instructions per corner; it is the identity on a dense level (index < (res + 1)^2 <= hs) and a mask when hs is a power of two (every
// wrapped level of the reference's torso encoder: hs = 2^16), so the division only runs for table sizes that are neither
__device__ __forceinline__ uint32_t lz_torso_grid_index(uint32_t gridtype, uint32_t hs, uint32_t resolution, uint32_t p0, uint32_t p1) {
    uint32_t stride = 1, index = 0;
    if (stride <= hs) { index += p0 * stride; stride *= resolution + 1; }
    if (stride <= hs) { index += p1 * stride; stride *= resolution + 1; }
    if (gridtype == 0 && stride > hs) index = p0 ^ (p1 * 2654435761u);
    if ((hs & (hs - 1u)) == 0u) index &= hs - 1u;
    else if (index >= hs) index %= hs;
    return index * 2u;
}

// ---- the kernel: sixteen pixels per wave pass on v_mfma_f32_16x16x4_f32 ---------------------------------------------------------------
// Lane (s = lane & 15, q = lane >> 4) works on pixel s of the wave's slice.  Orientation D[feature, pixel] = W . X as in the fused head
// (lz_head.hip): A = weights (16 features x 4 k), B = inputs (4 k x 16 pixels; lane (s, q) supplies k = 4 ks + q), and in a D tile lane
// (s, q) register r holds feature 16 t + 4 q + r.  The checker's chains run over the inputs in NATURAL order from the frame-constant
// partial sum, and a k-step of this MFMA is bit for bit that fma chain over its four k -- so the layers keep natural order: the first
// layers' per-pixel inputs are produced by the lane that supplies them (frequency features 4 i + q, grid features 4 i + q = level
// 2 i + (q >> 1), channel q & 1), the accumulators start from the constant partial sums, and between layers a D tile becomes four B
// operands by a 4 x 4 transpose across the pixel's four lanes: two v_permlane32_swap + two v_permlane16_swap (gfx950) per tile.
// Round 1-2's form -- one lane per pixel, 5.4 kMAC of scalar fma chains with a broadcast LDS read per weight, 256 registers, one wave
// per SIMD -- took 0.19 ms per 512^2 frame; k-steps that run past a layer's width multiply zeros (fma(0, 0, acc) = acc).
#define LZT_WG 256
typedef float lzt_f4 __attribute__((ext_vector_type(4)));
enum { LZT_D0 = 0, LZT_D1, LZT_D2, LZT_T0, LZT_T1, LZT_T2, LZT_LAYERS };
//                                   D0  D1  D2  T0  T1  T2
constexpr int LZT_KS[LZT_LAYERS] = {  9,  8,  8, 17,  8,  8 };   // k-steps of 4: 34 -> 36, 32, 32, 66 -> 68, 32, 32
constexpr int LZT_NT[LZT_LAYERS] = {  2,  2,  1,  2,  2,  1 };   // feature tiles of 16: 32, 32, 2 -> 16, 32, 32, 4 -> 16
constexpr int lzt_base(int layer) {
    int b = 0;
    for (int i = 0; i < layer; i++) b += LZT_KS[i] * LZT_NT[i];
    return b;
}
constexpr int LZT_FRAGS = lzt_base(LZT_LAYERS);   // 100 fragments x 64 lanes x 4 B = 25.6 KB of LDS

template <int LAYER>
__device__ __forceinline__ void lzt_layer(const float* __restrict__ wl, int lane, const float (&b)[LZT_KS[LAYER]], lzt_f4 (&acc)[LZT_NT[LAYER]]) {
    constexpr int KS = LZT_KS[LAYER], NT = LZT_NT[LAYER];
    const float* frag = wl + lzt_base(LAYER) * 64 + lane;
#pragma unroll
    for (int ks = 0; ks < KS; ks++)
#pragma unroll
        for (int ft = 0; ft < NT; ft++) acc[ft] = __builtin_amdgcn_mfma_f32_16x16x4f32(frag[(ks * NT + ft) * 64], b[ks], acc[ft], 0, 0, 0);
}
// D tile (register r of lane q = feature 16 t + 4 q + r) -> register j of lane q = feature 16 t + 4 j + q: the B operands of k-steps 4 t + j
__device__ __forceinline__ void lzt_transpose(lzt_f4& v) {
    uint32_t r0 = __float_as_uint(v[0]), r1 = __float_as_uint(v[1]), r2 = __float_as_uint(v[2]), r3 = __float_as_uint(v[3]);
    auto a = __builtin_amdgcn_permlane32_swap(r0, r2, false, false);    // register bit 1 <-> lane bit 5
    auto b = __builtin_amdgcn_permlane32_swap(r1, r3, false, false);
    auto c = __builtin_amdgcn_permlane16_swap(a[0], b[0], false, false);   // register bit 0 <-> lane bit 4
    auto d = __builtin_amdgcn_permlane16_swap(a[1], b[1], false, false);
    v[0] = __uint_as_float(c[0]); v[1] = __uint_as_float(c[1]); v[2] = __uint_as_float(d[0]); v[3] = __uint_as_float(d[1]);
}


// ---- the pieces of lz_k_torso_forward shared with the training kernels (lz_torso_train.hip) --------------------------------------------
// A fragments: lane l of fragment (layer, ks, ft) = W[16 ft + (l & 15)][4 ks + (l >> 4)] over the layer's PER-PIXEL columns, zero outside
template <int LAYER>
__device__ __forceinline__ void lzt_pack(float* __restrict__ wl, const float* __restrict__ w, int ld, int n_rows, int n_cols) {
    constexpr int NT = LZT_NT[LAYER], CNT = LZT_KS[LAYER] * NT * 64;
    float* dst = wl + lzt_base(LAYER) * 64;
    for (int i = threadIdx.x; i < CNT; i += LZT_WG) {
        const int fr = i >> 6, l = i & 63;
        const int ks = NT == 2 ? fr >> 1 : fr, ft = NT == 2 ? fr & 1 : 0;
        const int row = 16 * ft + (l & 15), col = 4 * ks + (l >> 4);
        dst[i] = (row < n_rows && col < n_cols) ? w[(size_t)row * ld + col] : 0.0f;
    }
}

// the six forward layers' fragments and the two frame-constant partial sums of the first layers (the caller synchronises)
template <int IND>
__device__ __forceinline__ void lzt_setup(const lz_torso_params& P, float* __restrict__ wl, float* __restrict__ cd, float* __restrict__ ct) {
    constexpr int KC = LZ_TORSO_ANCHOR + IND, K0 = LZ_TORSO_FREQ + KC, K1 = LZ_TORSO_GRIDF + K0, H = LZ_TORSO_HID;
    constexpr int KP = LZ_TORSO_GRIDF + LZ_TORSO_FREQ;
    lzt_pack<LZT_D0>(wl, P.deform_w0, K0, H, LZ_TORSO_FREQ);
    lzt_pack<LZT_D1>(wl, P.deform_w1, H, H, H);
    lzt_pack<LZT_D2>(wl, P.deform_w2, H, 2, H);
    lzt_pack<LZT_T0>(wl, P.torso_w0, K1, H, KP);
    lzt_pack<LZT_T1>(wl, P.torso_w1, H, H, H);
    lzt_pack<LZT_T2>(wl, P.torso_w2, H, 4, H);
    if (threadIdx.x < 2 * H) {   // constant partial sums: fma chain over [anchor 42 | ind] in natural order
        const int o = threadIdx.x % H;
        const bool tor = threadIdx.x >= H;
        const float* w = tor ? P.torso_w0 + (size_t)o * K1 + KP : P.deform_w0 + (size_t)o * K0 + LZ_TORSO_FREQ;
        float acc = 0.0f;
        for (int k = 0; k < LZ_TORSO_ANCHOR; k++) acc = lz_fmaf(w[k], P.enc_anchor[k], acc);
        for (int k = 0; k < IND; k++) acc = lz_fmaf(w[LZ_TORSO_ANCHOR + k], P.ind_code[k], acc);
        (tor ? ct : cd)[o] = acc;
    }
}

// 2-D occupancy (renderer.py:603-606): F.grid_sample(bilinear, zeros padding, align_corners=True) of density_grid [G*G] at (bx, by)
__device__ __forceinline__ float lzt_occupancy(const float* __restrict__ grid, uint32_t G, float bx, float by) {
    const float ix = ((bx + 1.0f) / 2.0f) * (float)(G - 1), iy = ((by + 1.0f) / 2.0f) * (float)(G - 1);
    const float x0f = floorf(ix), y0f = floorf(iy);
    const int x0 = (int)x0f, y0 = (int)y0f, x1 = x0 + 1, y1 = y0 + 1;
    // corner weights as torch forms them: nw = (ix_se - ix) * (iy_se - iy), ... (GridSampler.cuh)
    const float x1f = x0f + 1.0f, y1f = y0f + 1.0f;
    const float nw = (x1f - ix) * (y1f - iy), ne = (ix - x0f) * (y1f - iy), sw = (x1f - ix) * (iy - y0f), se = (ix - x0f) * (iy - y0f);
    auto at = [&](int xx, int yy) { return (xx >= 0 && yy >= 0 && xx < (int)G && yy < (int)G) ? grid[(size_t)yy * G + xx] : 0.0f; };
    float occ = 0.0f;   // `out_acc += value * weight` in nw, ne, sw, se order, contracted to fma by nvcc's default -fmad=true
    occ = lz_fmaf(at(x0, y0), nw, occ);
    occ = lz_fmaf(at(x1, y0), ne, occ);
    occ = lz_fmaf(at(x0, y1), sw, occ);
    occ = lz_fmaf(at(x1, y1), se, occ);
    return occ;
}

// per-level geometry of the torso encoder's cell of u in [0,1]^2: cell corner g, fractions f (grid.py:143, gridencoder.cu)
struct LztCell {
    uint32_t g0, g1;
    float f0, f1;
};
__device__ __forceinline__ LztCell lzt_cell(const float (&u)[2], float sc) {
    const float p0 = lz_fmaf(u[0], sc, 0.5f), p1 = lz_fmaf(u[1], sc, 0.5f);
    LztCell c;
    c.g0 = (uint32_t)floorf(p0); c.g1 = (uint32_t)floorf(p1);
    c.f0 = p0 - (float)c.g0; c.f1 = p1 - (float)c.g1;
    return c;
}

// What one wave pass of forward_torso leaves per lane (s, q) -- pixel s of the slice.  B-operand layout: register i holds feature 4 i + q.
struct LztFwd {
    float x[2];          // the shrunk coordinates
    float ex[9];         // frequency features (34, 35: padding)
    float bd1[8], bd2[8];// deform net: ReLU outputs of layers 0 and 1
    float dx[2];         // deform net output (every lane of the pixel)
    float u[2];          // (clamp(x + dx) + 1) / 2
    float gx[8];         // grid features
    float bt1[8], bt2[8];// torso net: ReLU outputs of layers 0 and 1
    lzt_f4 o;            // torso net output rows 0-3 (lanes q == 0)
};

// forward_torso (network.py:170-205) for pixel (bx, by) of lane (s, q): the fragments `wl` and partial sums cd / ct of lzt_setup
template <int IND>
__device__ __forceinline__ void lzt_forward(const LzTorsoArgs& A, const float* __restrict__ wl, const float* __restrict__ cd,
                                            const float* __restrict__ ct, int lane, float bx, float by, LztFwd& f) {
    const lz_torso_params& P = A.p;
    const int s = lane & 15, q = lane >> 4;
    const float x0 = bx * P.torso_shrink, x1 = by * P.torso_shrink;   // selected by value below: a lane-dependent index into f.x
    f.x[0] = x0; f.x[1] = x1;                                               // would put the whole record in scratch
    // frequency features 4 i + q of [x, sin(2^f x), cos(2^f x)]_f (freqencoder.cu:30-66; cos as sin(. + pi/2)); 34 and 35 are padding
#pragma unroll
    for (int i = 0; i < 9; i++) {
        const int c = 4 * i + q;
        float v = 0.0f;
        if (c < 2) v = (c & 1) ? x1 : x0;
        else if (c < LZ_TORSO_FREQ) {
            const int col = c / 2 - 1, d = c % 2, freq = col / 2;
            v = lz_sinf(lz_scalbnf(d ? x1 : x0, freq) + (float)(col % 2) * (LZ_PI_F / 2));
        }
        f.ex[i] = v;
    }
    auto relu4 = [](lzt_f4& v) {
#pragma unroll
        for (int r = 0; r < 4; r++) v[r] = v[r] > 0.0f ? v[r] : 0.0f;
    };
    auto init2 = [&](const float* c0, lzt_f4 (&acc)[2]) {
#pragma unroll
        for (int t = 0; t < 2; t++) acc[t] = *reinterpret_cast<const lzt_f4*>(c0 + 16 * t + 4 * q);
    };
    // hidden pair of a net: D tiles -> ReLU -> transpose -> eight B operands
    auto to_b = [&](lzt_f4 (&acc)[2], float (&b)[8]) {
#pragma unroll
        for (int t = 0; t < 2; t++) {
            relu4(acc[t]);
            lzt_transpose(acc[t]);
#pragma unroll
            for (int j = 0; j < 4; j++) b[4 * t + j] = acc[t][j];
        }
    };
    {
        lzt_f4 a0[2];
        init2(cd, a0);
        lzt_layer<LZT_D0>(wl, lane, f.ex, a0);
        to_b(a0, f.bd1);
        lzt_f4 a1[2] = {lzt_f4{0, 0, 0, 0}, lzt_f4{0, 0, 0, 0}};
        lzt_layer<LZT_D1>(wl, lane, f.bd1, a1);
        to_b(a1, f.bd2);
        lzt_f4 a2[1] = {lzt_f4{0, 0, 0, 0}};
        lzt_layer<LZT_D2>(wl, lane, f.bd2, a2);
        f.dx[0] = __shfl(a2[0][0], s, 64);      // rows 0, 1 of the tile sit in lane (s, q = 0)
        f.dx[1] = __shfl(a2[0][1], s, 64);
    }
    // x = (x + dx).clamp(-1, 1); torso_encoder(x, bound=1) (network.py:193-195, grid.py:143): this lane's grid features 4 i + q =
    // channel q & 1 of level 2 i + (q >> 1)
    {
#pragma unroll
        for (int d = 0; d < 2; d++) f.u[d] = (lz_fminf(lz_fmaxf(f.x[d] + f.dx[d], -1.0f), 1.0f) + 1.0f) / 2.0f;
        const bool oob = f.u[0] < 0 || f.u[0] > 1 || f.u[1] < 0 || f.u[1] > 1;   // cannot happen after the clamp; kept for NaN-free parity
        const int ch = q & 1;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const int l = 2 * i + (q >> 1);
            const uint32_t off0 = (uint32_t)P.offsets[l], hs = (uint32_t)P.offsets[l + 1] - off0;
            const uint32_t resolution = A.res[l];
            const float* g = P.emb + (size_t)off0 * 2 + ch;
            const LztCell cl = lzt_cell(f.u, A.scale[l]);
            float r0 = 0.0f;
#pragma unroll
            for (int c = 0; c < 4; c++) {
                const float w = ((c & 1) ? cl.f0 : 1 - cl.f0) * ((c >> 1) ? cl.f1 : 1 - cl.f1);
                const uint32_t index = lz_torso_grid_index(P.gridtype, hs, resolution, cl.g0 + (c & 1), cl.g1 + (c >> 1));
                r0 = lz_fmaf(w, g[index], r0);
            }
            f.gx[i] = oob ? 0.0f : r0;
        }
    }
    // torso net: [grid 32 | enc_x 34 | anchor | ind] -> 32 -> 32 -> 4
    {
        float b0[17];
#pragma unroll
        for (int i = 0; i < 8; i++) b0[i] = f.gx[i];
#pragma unroll
        for (int i = 0; i < 9; i++) b0[8 + i] = f.ex[i];
        lzt_f4 a0[2];
        init2(ct, a0);
        lzt_layer<LZT_T0>(wl, lane, b0, a0);
        to_b(a0, f.bt1);
        lzt_f4 a1[2] = {lzt_f4{0, 0, 0, 0}, lzt_f4{0, 0, 0, 0}};
        lzt_layer<LZT_T1>(wl, lane, f.bt1, a1);
        to_b(a1, f.bt2);
        lzt_f4 a2[1] = {lzt_f4{0, 0, 0, 0}};
        lzt_layer<LZT_T2>(wl, lane, f.bt2, a2);
        f.o = a2[0];
    }
}

// network.py:202-203
__device__ __forceinline__ float lzt_out(float o) { return lz_sigmoidf(o) * 1.002f - 0.001f; }
