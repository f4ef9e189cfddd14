// lz_lpips.hip -- LPIPS v0.1 on the AlexNet trunk (lpips.LPIPS(net='alex').forward as called at nerf_triplane/TrainerUtil.py:283,309),
// value and gradient with respect to the first image, in f32, for gfx950.  The operation is defined in DESIGN 4.14:
//
//   x = (image - shift) / scale                                   images [P,3,H,W] in [-1, 1], 31 <= H, W <= 256
//   f0 = relu(conv 3->64 k11 s4 p2 (x))      f1 = relu(conv 64->192 k5 p2 (maxpool 3/2 (f0)))
//   f2 = relu(conv 192->384 k3 p1 (maxpool 3/2 (f1)))             f3 = relu(conv 384->256 k3 p1 (f2))    f4 = relu(conv 256->256 k3 p1 (f3))
//   per tap t: n = f / (sqrt(sum_c f^2) + 1e-10);  d = sum_c w_c (n_pred - n_target)^2;  mean over the tap's pixels;  value = sum over taps
//
// The workload is 1 .. a few hundred output pixels against 10 MB of frozen weights: M tiny, K = 363 .. 3456 large.  So:
//
//   lz_k_lpips_prep     both images, NCHW -> scaled NHWC with the channels padded to 4 (a k-step of conv1 is then one pixel, one 16-byte load)
//   lz_k_lpips_conv     implicit GEMM on v_mfma_f32_16x16x4_f32 in the fragment convention of lz_linear.hip: D[pixel, n] = A (16 pixels x 4 k)
//                       . B (4 k x 16 n), k = (ky, kx, ci) with ci innermost, so a lane's four k of a 16-block are 16 contiguous bytes of the
//                       NHWC activation, gathered straight from it (no im2col buffer; zero outside the image).  The weights are packed once,
//                       [n-tile][16-block][lane][4], a lane's fragment of a block being one 16-byte load.  A workgroup is one tile of 16 pixels
//                       x 16 output channels; its four waves take every fourth 16-block of K and the partial tiles are summed through LDS in wave
//                       order -- no atomics, the same bits on every call.  Bias, an addend and ReLU sit in the epilogue.  The 2P images of both
//                       branches are rows of the one GEMM, so both branches share one arithmetic: equal images give equal features.
//                       The data gradient of a stride-1 convolution is the same kernel on a second pack (channels transposed, taps flipped),
//                       with the ReLU select (f > 0 ? g : 0) applied to the operand as it is gathered and the tap's own gradient as the addend.
//   lz_k_lpips_pool / lz_k_lpips_pool_backward   maxpool 3/2; the backward is a gather that recomputes the arg-max (first maximum in
//                       row-major window order) and adds into the tap gradient below it
//   lz_k_lpips_conv1_dgrad   conv1's stride-4 data gradient as a gather: an input pixel sums over the <= 3 x 3 output positions whose windows
//                       hold it (ky = (iy + 2) mod 4 + 4 j), 64 channels each, four lanes per pixel, and lands as d value / d pred in NCHW
//   lz_k_lpips_taps_forward / _backward   normalise, difference, lin, spatial mean, sum over the taps; one workgroup per patch forward (fixed
//                       order), one wave per pixel and tap backward (the tap's gradient for the pred branch, before any select)
//
// Nine launches forward, eight backward.  Gradient flows to the first image only; the second branch and all weights are constants.
#include "lz_common.h"

typedef float lz_f4 __attribute__((ext_vector_type(4)));

#define LZP_LAYERS 5
#define LZP_EPS 1e-10f
#define LZP_MAX_P 4096u

static const uint32_t lzp_cin[LZP_LAYERS] = {3, 64, 192, 384, 256}, lzp_cinp[LZP_LAYERS] = {4, 64, 192, 384, 256},
                      lzp_cout[LZP_LAYERS] = {64, 192, 384, 256, 256}, lzp_ks[LZP_LAYERS] = {11, 5, 3, 3, 3};

// ---- the packed weight image (floats): header | forward packs and biases | transposed packs of conv2..5 | conv1's gather pack | lin ----
struct LzpPack {
    size_t fw[LZP_LAYERS], bias[LZP_LAYERS], bw[LZP_LAYERS], lin[LZP_LAYERS], total;
};

static inline size_t lzp_pack_size(uint32_t n_out, uint32_t taps, uint32_t cin) { return (size_t)(n_out / 16) * ((taps * cin + 15) / 16) * 256; }

static LzpPack lzp_pack_layout() {
    LzpPack L;
    size_t o = 8;      // shift[3], 0, scale[3], 0
    for (int l = 0; l < LZP_LAYERS; l++) {
        L.fw[l] = o; o += lzp_pack_size(lzp_cout[l], lzp_ks[l] * lzp_ks[l], lzp_cinp[l]);
        L.bias[l] = o; o += lzp_cout[l];
    }
    for (int l = 1; l < LZP_LAYERS; l++) { L.bw[l] = o; o += lzp_pack_size(lzp_cin[l], lzp_ks[l] * lzp_ks[l], lzp_cout[l]); }
    L.bw[0] = o; o += (size_t)121 * 64 * 4;
    for (int l = 0; l < LZP_LAYERS; l++) { L.lin[l] = o; o += lzp_cout[l]; }
    L.total = o;
    return L;
}

extern "C" size_t lz_lpips_packed_floats(void) { return lzp_pack_layout().total; }

extern "C" int lz_lpips_pack(const lz_lpips_weights* w, float* packed, size_t packed_floats) {
    LZ_REQUIRE(w && packed, LZ_ERR_BAD_ARGUMENT, "lpips_pack: null argument");
    const LzpPack L = lzp_pack_layout();
    LZ_REQUIRE(packed_floats >= L.total, LZ_ERR_BAD_ARGUMENT, "lpips_pack: packed holds %zu floats, %zu needed", packed_floats, L.total);
    for (int l = 0; l < LZP_LAYERS; l++)
        LZ_REQUIRE(w->conv_w[l] && w->conv_b[l] && w->lin_w[l], LZ_ERR_BAD_ARGUMENT, "lpips_pack: null weights of layer %d", l);
    for (int c = 0; c < 3; c++) LZ_REQUIRE(w->scale[c] != 0.0f, LZ_ERR_BAD_ARGUMENT, "lpips_pack: scale[%d] is 0", c);
    memset(packed, 0, L.total * sizeof(float));
    for (int c = 0; c < 3; c++) { packed[c] = w->shift[c]; packed[4 + c] = w->scale[c]; }
    for (int l = 0; l < LZP_LAYERS; l++) {
        const uint32_t ci_n = lzp_cin[l], cp = lzp_cinp[l], co_n = lzp_cout[l], ks = lzp_ks[l], taps = ks * ks;
        const float* W = w->conv_w[l];      // [co][ci][ky][kx]
        {   // forward: n = co, k = (tap, ci)
            const uint32_t KB = (taps * cp + 15) / 16;
            float* o = packed + L.fw[l];
            for (uint32_t t = 0; t < co_n / 16; t++)
                for (uint32_t jj = 0; jj < KB; jj++)
                    for (uint32_t lane = 0; lane < 64; lane++)
                        for (uint32_t c = 0; c < 4; c++) {
                            const uint32_t n = 16 * t + (lane & 15), k = 16 * jj + 4 * (lane >> 4) + c, tap = k / cp, ci = k % cp;
                            if (tap < taps && ci < ci_n) o[(((size_t)t * KB + jj) * 64 + lane) * 4 + c] = W[((size_t)n * ci_n + ci) * taps + tap];
                        }
        }
        memcpy(packed + L.bias[l], w->conv_b[l], co_n * sizeof(float));
        memcpy(packed + L.lin[l], w->lin_w[l], co_n * sizeof(float));
        if (l == 0) {   // the gather pack of conv1: [tap][co][4]
            float* o = packed + L.bw[0];
            for (uint32_t tap = 0; tap < taps; tap++)
                for (uint32_t co = 0; co < co_n; co++)
                    for (uint32_t ci = 0; ci < ci_n; ci++) o[((size_t)tap * co_n + co) * 4 + ci] = W[((size_t)co * ci_n + ci) * taps + tap];
        } else {        // data gradient: n = ci, k = (flipped tap, co)
            const uint32_t KB = taps * co_n / 16;
            float* o = packed + L.bw[l];
            for (uint32_t t = 0; t < ci_n / 16; t++)
                for (uint32_t jj = 0; jj < KB; jj++)
                    for (uint32_t lane = 0; lane < 64; lane++)
                        for (uint32_t c = 0; c < 4; c++) {
                            const uint32_t n = 16 * t + (lane & 15), k = 16 * jj + 4 * (lane >> 4) + c, tap = k / co_n, co = k % co_n;
                            o[(((size_t)t * KB + jj) * 64 + lane) * 4 + c] = W[((size_t)co * ci_n + n) * taps + (taps - 1 - tap)];
                        }
        }
    }
    return LZ_OK;
}

// ---- the workspace (floats): scaled input | features | pooled features | tap gradients | pooled gradients ----
struct LzpGeom {
    uint32_t P, H, W;
    uint32_t h[LZP_LAYERS], w[LZP_LAYERS];      // tap sizes
    uint32_t hp[2], wp[2];                      // pooled sizes behind taps 0 and 1
    size_t x0, f[LZP_LAYERS], pl[2], g[LZP_LAYERS], gpl[2], total;
};

static inline bool lzp_shape_ok(uint32_t P, uint32_t H, uint32_t W) { return P >= 1 && P <= LZP_MAX_P && H >= 31 && H <= 256 && W >= 31 && W <= 256; }

static LzpGeom lzp_geom(uint32_t P, uint32_t H, uint32_t W) {
    LzpGeom G;
    G.P = P; G.H = H; G.W = W;
    G.h[0] = (H - 7) / 4 + 1; G.w[0] = (W - 7) / 4 + 1;
    G.hp[0] = (G.h[0] - 3) / 2 + 1; G.wp[0] = (G.w[0] - 3) / 2 + 1;
    G.h[1] = G.hp[0]; G.w[1] = G.wp[0];
    G.hp[1] = (G.h[1] - 3) / 2 + 1; G.wp[1] = (G.w[1] - 3) / 2 + 1;
    for (int l = 2; l < LZP_LAYERS; l++) { G.h[l] = G.hp[1]; G.w[l] = G.wp[1]; }
    size_t o = 0;
    G.x0 = o; o += (size_t)2 * P * H * W * 4;
    for (int l = 0; l < LZP_LAYERS; l++) { G.f[l] = o; o += (size_t)2 * P * G.h[l] * G.w[l] * lzp_cout[l]; }
    for (int l = 0; l < 2; l++) { G.pl[l] = o; o += (size_t)2 * P * G.hp[l] * G.wp[l] * lzp_cout[l]; }
    for (int l = 0; l < LZP_LAYERS; l++) { G.g[l] = o; o += (size_t)P * G.h[l] * G.w[l] * lzp_cout[l]; }
    for (int l = 0; l < 2; l++) { G.gpl[l] = o; o += (size_t)P * G.hp[l] * G.wp[l] * lzp_cout[l]; }
    G.total = o;
    return G;
}

extern "C" size_t lz_lpips_workspace_bytes(uint32_t P, uint32_t H, uint32_t W) {
    if (!lzp_shape_ok(P, H, W)) return 0;
    return lzp_geom(P, H, W).total * sizeof(float);
}

// ---- kernels ----
// x0 [2P][H][W][4] = ((image - shift) / scale, 0); images 0 .. P-1 are pred, P .. 2P-1 target
__global__ void __launch_bounds__(256)
lz_k_lpips_prep(const float* __restrict__ pred, const float* __restrict__ target, const float* __restrict__ hdr, uint32_t P, uint32_t HW,
                float* __restrict__ x0) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= 2 * P * HW) return;
    const uint32_t img = i / HW, px = i - img * HW;
    const float* src = img < P ? pred + (size_t)img * 3 * HW : target + (size_t)(img - P) * 3 * HW;
    lz_f4 v;
    v.x = (src[px] - hdr[0]) / hdr[4];
    v.y = (src[HW + px] - hdr[1]) / hdr[5];
    v.z = (src[2 * HW + px] - hdr[2]) / hdr[6];
    v.w = 0.0f;
    reinterpret_cast<lz_f4*>(x0)[i] = v;
}

struct LzpConv {
    uint32_t Hin, Win, Hout, Wout, M, Cout;     // M = images * Hout * Wout
};

template <int CIN, int KS, int STRIDE, int PAD>
__global__ void __launch_bounds__(256)
lz_k_lpips_conv(const float* __restrict__ in, const float* __restrict__ mask, const float* __restrict__ wp, const float* __restrict__ bias,
                const float* addend, float* out, LzpConv g, int relu) {
    constexpr int Q = CIN / 4;                              // 4-channel groups per tap
    constexpr int KB = (KS * KS * CIN + 15) / 16;           // 16-blocks of K
    __shared__ float red[4 * 4 * 64];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6, s = lane & 15, kk = lane >> 4;
    const uint32_t m = blockIdx.x * 16 + s;
    const bool m_ok = m < g.M;
    uint32_t img = 0, oy = 0, ox = 0;
    if (m_ok) {
        img = m / (g.Hout * g.Wout);
        const uint32_t rem = m - img * (g.Hout * g.Wout);
        oy = rem / g.Wout; ox = rem - oy * g.Wout;
    }
    const int iy0 = (int)oy * STRIDE - PAD, ix0 = (int)ox * STRIDE - PAD;
    const size_t ibase = (size_t)img * g.Hin * g.Win * CIN;
    const lz_f4* wt = reinterpret_cast<const lz_f4*>(wp + (size_t)blockIdx.y * KB * 256) + lane;
    lz_f4 acc = lz_f4{0, 0, 0, 0};
#pragma unroll 4
    for (int jj = (int)wave; jj < KB; jj += 4) {
        const int q4 = 4 * jj + (int)kk;
        const int tap = q4 / Q, ci = (q4 - tap * Q) * 4;
        const int ky = tap / KS, kx = tap - ky * KS;
        const int iy = iy0 + ky, ix = ix0 + kx;
        lz_f4 a = lz_f4{0, 0, 0, 0};
        if (m_ok && tap < KS * KS && iy >= 0 && iy < (int)g.Hin && ix >= 0 && ix < (int)g.Win) {
            const size_t off = ibase + ((size_t)iy * g.Win + ix) * CIN + ci;
            a = *reinterpret_cast<const lz_f4*>(in + off);
            if (mask) {
                const lz_f4 k = *reinterpret_cast<const lz_f4*>(mask + off);
                a.x = k.x > 0.0f ? a.x : 0.0f; a.y = k.y > 0.0f ? a.y : 0.0f; a.z = k.z > 0.0f ? a.z : 0.0f; a.w = k.w > 0.0f ? a.w : 0.0f;
            }
        }
        const lz_f4 b = wt[(size_t)jj * 64];
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, acc, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 4; r++) red[(wave * 4 + r) * 64 + lane] = acc[r];
    __syncthreads();
    // thread (r = wave, lane): D row 4 (lane >> 4) + r, column lane & 15; the four waves' partials in wave order
    const uint32_t r = wave;
    float v = red[r * 64 + lane];
    v += red[(4 + r) * 64 + lane];
    v += red[(8 + r) * 64 + lane];
    v += red[(12 + r) * 64 + lane];
    const uint32_t om = blockIdx.x * 16 + 4 * kk + r, n = blockIdx.y * 16 + s;
    if (om < g.M) {
        const size_t o = (size_t)om * g.Cout + n;
        if (bias) v += bias[n];
        if (addend) v += addend[o];
        if (relu) v = v > 0.0f ? v : 0.0f;
        out[o] = v;
    }
}

// maxpool 3 / 2 on [NI][H][W][C]; one thread per output pixel and four channels
__global__ void __launch_bounds__(256)
lz_k_lpips_pool(const float* __restrict__ in, uint32_t NI, uint32_t H, uint32_t W, uint32_t Ho, uint32_t Wo, uint32_t C4, float* __restrict__ out) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= NI * Ho * Wo * C4) return;
    const uint32_t c = i % C4, px = i / C4, ox = px % Wo, t = px / Wo, oy = t % Ho, img = t / Ho;
    const lz_f4* src = reinterpret_cast<const lz_f4*>(in) + ((size_t)(img * H + 2 * oy) * W + 2 * ox) * C4 + c;
    lz_f4 v = src[0];
#pragma unroll
    for (int dy = 0; dy < 3; dy++)
#pragma unroll
        for (int dx = 0; dx < 3; dx++) {
            const lz_f4 u = src[((size_t)dy * W + dx) * C4];
            v.x = u.x > v.x ? u.x : v.x; v.y = u.y > v.y ? u.y : v.y; v.z = u.z > v.z ? u.z : v.z; v.w = u.w > v.w ? u.w : v.w;
        }
    reinterpret_cast<lz_f4*>(out)[i] = v;
}

// g[img][y][x][c] += sum over the windows (oy, ox) that hold (y, x) and whose first maximum in row-major order it is, of gp[img][oy][ox][c];
// f: the pooled features of the pred images (the first NI images of the feature buffer); windows in ascending (oy, ox)
__global__ void __launch_bounds__(256)
lz_k_lpips_pool_backward(const float* __restrict__ f, const float* __restrict__ gp, uint32_t NI, uint32_t H, uint32_t W, uint32_t Ho, uint32_t Wo,
                         uint32_t C, float* __restrict__ g) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= NI * H * W * C) return;
    const uint32_t c = i % C, px = i / C, x = px % W, t = px / W, y = t % H, img = t / H;
    const float v = f[i];
    const uint32_t oy_lo = y >= 2 ? (y - 1) / 2 : 0, ox_lo = x >= 2 ? (x - 1) / 2 : 0;      // ceil((y - 2) / 2)
    float sum = 0.0f;
    for (uint32_t oy = oy_lo; oy <= y / 2 && oy < Ho; oy++)
        for (uint32_t ox = ox_lo; ox <= x / 2 && ox < Wo; ox++) {
            bool first = true;
#pragma unroll
            for (uint32_t dy = 0; dy < 3; dy++)
#pragma unroll
                for (uint32_t dx = 0; dx < 3; dx++) {
                    const uint32_t yy = 2 * oy + dy, xx = 2 * ox + dx;
                    const float u = f[((size_t)(img * H + yy) * W + xx) * C + c];
                    const bool before = yy < y || (yy == y && xx < x);
                    if (before ? u >= v : u > v) first = false;
                }
            if (first) sum += gp[((size_t)(img * Ho + oy) * Wo + ox) * C + c];
        }
    g[i] += sum;
}

// conv1's data gradient: g_pred[p][ci][iy][ix] = (sum over (ky, kx, co) of select(g0, f0)[p][oy][ox][co] W[co][ci][ky][kx]) / scale[ci],
// oy = (iy + 2 - ky) / 4 where that is a whole number in range.  Four lanes per pixel, 16 output channels each, summed in a fixed order.
__global__ void __launch_bounds__(256)
lz_k_lpips_conv1_dgrad(const float* __restrict__ g0, const float* __restrict__ f0, const float* __restrict__ wd, const float* __restrict__ hdr,
                       uint32_t P, uint32_t H, uint32_t W, uint32_t H1, uint32_t W1, float* __restrict__ g_pred) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    const uint32_t px = i >> 2, sub = i & 3;
    const bool ok = px < P * H * W;          // (no early return: the shuffles below want whole quads, and the grid is padded to whole workgroups)
    const uint32_t q = ok ? px : 0;
    const uint32_t ix = q % W, t = q / W, iy = t % H, p = t / H;
    float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f;
    for (uint32_t ky = (iy + 2) & 3; ky < 11; ky += 4) {
        if (iy + 2 < ky) continue;
        const uint32_t oy = (iy + 2 - ky) >> 2;
        if (oy >= H1) continue;
        for (uint32_t kx = (ix + 2) & 3; kx < 11; kx += 4) {
            if (ix + 2 < kx) continue;
            const uint32_t ox = (ix + 2 - kx) >> 2;
            if (ox >= W1) continue;
            const size_t off = ((size_t)(p * H1 + oy) * W1 + ox) * 64 + 16 * sub;
            const lz_f4* wq = reinterpret_cast<const lz_f4*>(wd) + (size_t)(ky * 11 + kx) * 64 + 16 * sub;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const lz_f4 gz = *reinterpret_cast<const lz_f4*>(g0 + off + 4 * j);
                const lz_f4 fz = *reinterpret_cast<const lz_f4*>(f0 + off + 4 * j);
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    const float z = fz[e] > 0.0f ? gz[e] : 0.0f;
                    const lz_f4 w = wq[4 * j + e];
                    a0 += z * w.x; a1 += z * w.y; a2 += z * w.z;
                }
            }
        }
    }
    a0 += __shfl_xor(a0, 1, 64); a1 += __shfl_xor(a1, 1, 64); a2 += __shfl_xor(a2, 1, 64);
    a0 += __shfl_xor(a0, 2, 64); a1 += __shfl_xor(a1, 2, 64); a2 += __shfl_xor(a2, 2, 64);
    if (ok && sub == 0) {
        const size_t HW = (size_t)H * W, o = (size_t)p * 3 * HW + (size_t)iy * W + ix;
        g_pred[o] = a0 / hdr[4];
        g_pred[o + HW] = a1 / hdr[5];
        g_pred[o + 2 * HW] = a2 / hdr[6];
    }
}

struct LzpTaps {
    const float* f[LZP_LAYERS];      // [2P][hw][c]
    const float* lin[LZP_LAYERS];    // [c]
    float* g[LZP_LAYERS];            // [P][hw][c] (backward)
    uint32_t hw[LZP_LAYERS], c[LZP_LAYERS];
};

__device__ __forceinline__ float lzp_wave_sum(float v) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// sum_c f^2 of both branches at one pixel, by one wave
__device__ __forceinline__ void lzp_norms(const float* __restrict__ f0, const float* __restrict__ f1, uint32_t C, uint32_t lane, float& s0, float& s1) {
    float a = 0.0f, b = 0.0f;
    for (uint32_t c = lane; c < C; c += 64) {
        const float u = f0[c], v = f1[c];
        a += u * u; b += v * v;
    }
    s0 = lzp_wave_sum(a); s1 = lzp_wave_sum(b);
}

#define LZP_TAPS_THREADS 1024
__global__ void __launch_bounds__(LZP_TAPS_THREADS)
lz_k_lpips_taps_forward(LzpTaps T, uint32_t P, float* __restrict__ value) {
    __shared__ float part[LZP_TAPS_THREADS / 64];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6, p = blockIdx.x;
    float val = 0.0f;
#pragma unroll
    for (int t = 0; t < LZP_LAYERS; t++) {
        const uint32_t hw = T.hw[t], C = T.c[t];
        const float* lin = T.lin[t];
        float acc = 0.0f;
        for (uint32_t px = wave; px < hw; px += LZP_TAPS_THREADS / 64) {
            const float* f0 = T.f[t] + ((size_t)p * hw + px) * C;
            const float* f1 = T.f[t] + ((size_t)(P + p) * hw + px) * C;
            float s0, s1;
            lzp_norms(f0, f1, C, lane, s0, s1);
            const float r0 = sqrtf(s0) + LZP_EPS, r1 = sqrtf(s1) + LZP_EPS;
            float d = 0.0f;
            for (uint32_t c = lane; c < C; c += 64) {
                const float e = f0[c] / r0 - f1[c] / r1;
                d += lin[c] * (e * e);
            }
            acc += lzp_wave_sum(d);
        }
        if (lane == 0) part[wave] = acc;
        __syncthreads();
        if (threadIdx.x == 0) {
            float s = 0.0f;
            for (int w = 0; w < LZP_TAPS_THREADS / 64; w++) s += part[w];
            val += s / (float)hw;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) value[p] = val;
}

// the tap's gradient for the pred branch: grid (pixels / 4, taps, P), one wave per pixel
__global__ void __launch_bounds__(256)
lz_k_lpips_taps_backward(LzpTaps T, uint32_t P, const float* __restrict__ g_value) {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6, t = blockIdx.y, p = blockIdx.z;
    const uint32_t hw = T.hw[t], C = T.c[t], px = blockIdx.x * 4 + wave;
    if (px >= hw) return;
    const float* lin = T.lin[t];
    const float* f0 = T.f[t] + ((size_t)p * hw + px) * C;
    const float* f1 = T.f[t] + ((size_t)(P + p) * hw + px) * C;
    float* g = T.g[t] + ((size_t)p * hw + px) * C;
    float s0, s1;
    lzp_norms(f0, f1, C, lane, s0, s1);
    const float q0 = sqrtf(s0), r0 = q0 + LZP_EPS, r1 = sqrtf(s1) + LZP_EPS;
    const float gs = g_value[p] / (float)hw;
    float dot = 0.0f;
    for (uint32_t c = lane; c < C; c += 64) {
        const float u = f0[c];
        const float dn = gs * (2.0f * lin[c] * (u / r0 - f1[c] / r1));
        dot += dn * u;
    }
    dot = lzp_wave_sum(dot);
    const float back = dot / (r0 * r0);
    for (uint32_t c = lane; c < C; c += 64) {
        const float u = f0[c];
        const float dn = gs * (2.0f * lin[c] * (u / r0 - f1[c] / r1));
        const float dir = q0 > 0.0f ? u / q0 : 0.0f;          // d sqrt(s) / d f; a pixel of zeros has f = 0 everywhere and the ReLU select drops it
        g[c] = dn / r0 - back * dir;
    }
}

// ---- host ----
template <int CIN, int KS, int STRIDE, int PAD>
static void lzp_conv(hipStream_t st, const float* in, const float* mask, const float* wp, const float* bias, const float* addend, float* out,
                     uint32_t NI, uint32_t Hin, uint32_t Win, uint32_t Hout, uint32_t Wout, uint32_t Cout, int relu) {
    const LzpConv g{Hin, Win, Hout, Wout, NI * Hout * Wout, Cout};
    hipLaunchKernelGGL((lz_k_lpips_conv<CIN, KS, STRIDE, PAD>), dim3(lz_div_up(g.M, 16), Cout / 16), dim3(256), 0, st, in, mask, wp, bias, addend, out, g,
                       relu);
}

static void lzp_taps(LzpTaps& T, const LzpGeom& G, const LzpPack& L, const float* packed, float* ws) {
    for (int l = 0; l < LZP_LAYERS; l++) {
        T.f[l] = ws + G.f[l]; T.lin[l] = packed + L.lin[l]; T.g[l] = ws + G.g[l];
        T.hw[l] = G.h[l] * G.w[l]; T.c[l] = lzp_cout[l];
    }
}

static int lzp_check(uint32_t P, uint32_t H, uint32_t W, const void* workspace, const char* who) {
    LZ_REQUIRE(P <= LZP_MAX_P, LZ_ERR_UNSUPPORTED, "%s: P = %u patches (at most %u)", who, P, LZP_MAX_P);
    LZ_REQUIRE(H >= 31 && W >= 31, LZ_ERR_UNSUPPORTED, "%s: %u x %u image, the trunk needs at least 31 x 31", who, H, W);
    LZ_REQUIRE(H <= 256 && W <= 256, LZ_ERR_UNSUPPORTED, "%s: %u x %u image, at most 256 x 256", who, H, W);
    LZ_REQUIRE(((uintptr_t)workspace & 15) == 0, LZ_ERR_BAD_ARGUMENT, "%s: workspace must be 16-byte aligned", who);
    return LZ_OK;
}

extern "C" int lz_lpips_forward(const float* packed, const float* pred, const float* target, uint32_t P, uint32_t H, uint32_t W, void* workspace,
                                float* value, lz_stream_t stream) {
    if (P == 0) return LZ_OK;
    LZ_REQUIRE(packed && pred && target && workspace && value, LZ_ERR_BAD_ARGUMENT, "lpips_forward: null tensor");
    LZ_REQUIRE(((uintptr_t)packed & 15) == 0, LZ_ERR_BAD_ARGUMENT, "lpips_forward: packed must be 16-byte aligned");
    const int rc = lzp_check(P, H, W, workspace, "lpips_forward");
    if (rc != LZ_OK) return rc;
    const LzpGeom G = lzp_geom(P, H, W);
    const LzpPack L = lzp_pack_layout();
    float* ws = reinterpret_cast<float*>(workspace);
    hipStream_t st = lz_st(stream);
    const uint32_t NI = 2 * P;
    hipLaunchKernelGGL(lz_k_lpips_prep, dim3(lz_div_up((uint64_t)NI * H * W, 256)), dim3(256), 0, st, pred, target, packed, P, H * W, ws + G.x0);
    LZ_CHECK_LAUNCH("lpips_forward (prep)");
    lzp_conv<4, 11, 4, 2>(st, ws + G.x0, nullptr, packed + L.fw[0], packed + L.bias[0], nullptr, ws + G.f[0], NI, H, W, G.h[0], G.w[0], 64, 1);
    LZ_CHECK_LAUNCH("lpips_forward (conv1)");
    hipLaunchKernelGGL(lz_k_lpips_pool, dim3(lz_div_up((uint64_t)NI * G.hp[0] * G.wp[0] * 16, 256)), dim3(256), 0, st, ws + G.f[0], NI, G.h[0], G.w[0],
                       G.hp[0], G.wp[0], 16u, ws + G.pl[0]);
    LZ_CHECK_LAUNCH("lpips_forward (pool1)");
    lzp_conv<64, 5, 1, 2>(st, ws + G.pl[0], nullptr, packed + L.fw[1], packed + L.bias[1], nullptr, ws + G.f[1], NI, G.hp[0], G.wp[0], G.h[1], G.w[1], 192, 1);
    LZ_CHECK_LAUNCH("lpips_forward (conv2)");
    hipLaunchKernelGGL(lz_k_lpips_pool, dim3(lz_div_up((uint64_t)NI * G.hp[1] * G.wp[1] * 48, 256)), dim3(256), 0, st, ws + G.f[1], NI, G.h[1], G.w[1],
                       G.hp[1], G.wp[1], 48u, ws + G.pl[1]);
    LZ_CHECK_LAUNCH("lpips_forward (pool2)");
    const uint32_t h = G.h[2], w = G.w[2];
    lzp_conv<192, 3, 1, 1>(st, ws + G.pl[1], nullptr, packed + L.fw[2], packed + L.bias[2], nullptr, ws + G.f[2], NI, h, w, h, w, 384, 1);
    LZ_CHECK_LAUNCH("lpips_forward (conv3)");
    lzp_conv<384, 3, 1, 1>(st, ws + G.f[2], nullptr, packed + L.fw[3], packed + L.bias[3], nullptr, ws + G.f[3], NI, h, w, h, w, 256, 1);
    LZ_CHECK_LAUNCH("lpips_forward (conv4)");
    lzp_conv<256, 3, 1, 1>(st, ws + G.f[3], nullptr, packed + L.fw[4], packed + L.bias[4], nullptr, ws + G.f[4], NI, h, w, h, w, 256, 1);
    LZ_CHECK_LAUNCH("lpips_forward (conv5)");
    LzpTaps T;
    lzp_taps(T, G, L, packed, ws);
    hipLaunchKernelGGL(lz_k_lpips_taps_forward, dim3(P), dim3(LZP_TAPS_THREADS), 0, st, T, P, value);
    LZ_CHECK_LAUNCH("lpips_forward (taps)");
    return LZ_OK;
}

extern "C" int lz_lpips_backward(const float* packed, const float* g_value, uint32_t P, uint32_t H, uint32_t W, void* workspace, float* g_pred,
                                 lz_stream_t stream) {
    if (P == 0) return LZ_OK;
    LZ_REQUIRE(packed && g_value && workspace && g_pred, LZ_ERR_BAD_ARGUMENT, "lpips_backward: null tensor");
    LZ_REQUIRE(((uintptr_t)packed & 15) == 0, LZ_ERR_BAD_ARGUMENT, "lpips_backward: packed must be 16-byte aligned");
    const int rc = lzp_check(P, H, W, workspace, "lpips_backward");
    if (rc != LZ_OK) return rc;
    const LzpGeom G = lzp_geom(P, H, W);
    const LzpPack L = lzp_pack_layout();
    float* ws = reinterpret_cast<float*>(workspace);
    hipStream_t st = lz_st(stream);
    LzpTaps T;
    lzp_taps(T, G, L, packed, ws);
    uint32_t max_hw = 0;
    for (int l = 0; l < LZP_LAYERS; l++) max_hw = T.hw[l] > max_hw ? T.hw[l] : max_hw;
    hipLaunchKernelGGL(lz_k_lpips_taps_backward, dim3(lz_div_up(max_hw, 4), LZP_LAYERS, P), dim3(256), 0, st, T, P, g_value);
    LZ_CHECK_LAUNCH("lpips_backward (taps)");
    // the pred images are the first P of every feature buffer
    const uint32_t h = G.h[2], w = G.w[2];
    lzp_conv<256, 3, 1, 1>(st, ws + G.g[4], ws + G.f[4], packed + L.bw[4], nullptr, ws + G.g[3], ws + G.g[3], P, h, w, h, w, 256, 0);
    LZ_CHECK_LAUNCH("lpips_backward (conv5)");
    lzp_conv<256, 3, 1, 1>(st, ws + G.g[3], ws + G.f[3], packed + L.bw[3], nullptr, ws + G.g[2], ws + G.g[2], P, h, w, h, w, 384, 0);
    LZ_CHECK_LAUNCH("lpips_backward (conv4)");
    lzp_conv<384, 3, 1, 1>(st, ws + G.g[2], ws + G.f[2], packed + L.bw[2], nullptr, nullptr, ws + G.gpl[1], P, h, w, h, w, 192, 0);
    LZ_CHECK_LAUNCH("lpips_backward (conv3)");
    hipLaunchKernelGGL(lz_k_lpips_pool_backward, dim3(lz_div_up((uint64_t)P * G.h[1] * G.w[1] * 192, 256)), dim3(256), 0, st, ws + G.f[1], ws + G.gpl[1], P,
                       G.h[1], G.w[1], G.hp[1], G.wp[1], 192u, ws + G.g[1]);
    LZ_CHECK_LAUNCH("lpips_backward (pool2)");
    lzp_conv<192, 5, 1, 2>(st, ws + G.g[1], ws + G.f[1], packed + L.bw[1], nullptr, nullptr, ws + G.gpl[0], P, G.h[1], G.w[1], G.hp[0], G.wp[0], 64, 0);
    LZ_CHECK_LAUNCH("lpips_backward (conv2)");
    hipLaunchKernelGGL(lz_k_lpips_pool_backward, dim3(lz_div_up((uint64_t)P * G.h[0] * G.w[0] * 64, 256)), dim3(256), 0, st, ws + G.f[0], ws + G.gpl[0], P,
                       G.h[0], G.w[0], G.hp[0], G.wp[0], 64u, ws + G.g[0]);
    LZ_CHECK_LAUNCH("lpips_backward (pool1)");
    hipLaunchKernelGGL(lz_k_lpips_conv1_dgrad, dim3(lz_div_up((uint64_t)P * H * W * 4, 256)), dim3(256), 0, st, ws + G.g[0], ws + G.f[0], packed + L.bw[0],
                       packed, P, H, W, G.h[0], G.w[0], g_pred);
    LZ_CHECK_LAUNCH("lpips_backward (conv1)");
    return LZ_OK;
}
