// lz_audio.hip -- audio conditioning front-end: NeRFNetwork.encode_audio (nerf_triplane/network.py:226-240)
// = AudioNet (network.py:40-70: four stride-2 Conv1d + LeakyReLU over a 16-frame window, two Linear) on each of the seq_len
// windows, then AudioAttNet (network.py:9-37: five Conv1d over the window axis, Linear + softmax, attention-weighted sum).
// The reference spends 10-16 % of its frame time here on ~25 tiny cuDNN / cuBLAS launches.  The whole thing is a few
// MMAC with strictly sequential layers, so it is ONE workgroup: every layer is a loop over its outputs, activations ping-pong
// between two LDS buffers, weights stream from L2.  Arithmetic = explicit f32 fma chains (input channel outer, tap inner; bias
// added after the chain), restated by oracle/audio.py.
#include "lz_audio_net.h"   // lz_conv1d_k3, lz_fc, lz_lrelu, softmax: shared with the training backward (lz_audio_train.hip)

// First AudioNet layer for wide inputs (HuBERT: dim_in = 1024, a 3072-term dot product per output): one WAVE per output, lane l
// owns input channels l, l + 64, ... (fma chain, channel outer, tap inner), the 64 partial sums are combined by an xor-shuffle
// tree (32, 16, ..., 1), bias added last.  2048 outputs spread over the whole chip instead of 3072 dependent loads per lane of
// a single workgroup (0.88 ms -> a few microseconds).  y [n, 32, 8] goes to a small scratch buffer.
__global__ void __launch_bounds__(256)
lz_k_audio_conv1_wide(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ b, float* __restrict__ y, uint32_t n,
                      uint32_t Cin) {
    const uint32_t lane = threadIdx.x & 63, idx = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (idx >= n * 32 * 8) return;
    const uint32_t t = idx % 8, o = (idx / 8) % 32, win = idx / 256;
    const float* xr = x + (size_t)win * Cin * 16;
    const float* wr = w + (size_t)o * Cin * 3;
    float acc = 0.0f;
    for (uint32_t ci = lane; ci < Cin; ci += 64)
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const int pos = (int)(t * 2) + k - 1;
            if (pos >= 0 && pos < 16) acc = lz_fmaf(wr[ci * 3 + k], xr[(size_t)ci * 16 + pos], acc);
        }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
    if (lane == 0) y[idx] = lz_lrelu(acc + b[o]);
}

__global__ void __launch_bounds__(LZ_AUDIO_THREADS)
lz_k_audio_encode(lz_audio_params P, const float* __restrict__ a, float* __restrict__ enc_a, const float* __restrict__ conv1) {
    __shared__ float A[LZ_AUDIO_BUF], B[LZ_AUDIO_BUF], feat[8 * 64];
    const uint32_t n = P.n_win, da = P.dim_aud;
    // ---- AudioNet on every window: [n, dim_in, 16] -> [n, dim_aud]  (win_size 16: the slice x[:, :, 0:16] is the whole window)
    if (conv1) {   // first layer already done by lz_k_audio_conv1_wide
        for (uint32_t i = threadIdx.x; i < n * 32 * 8; i += blockDim.x) A[i] = conv1[i];
        __syncthreads();
    } else {
        lz_conv1d_k3(a, P.c_w[0], P.c_b[0], A, n, P.dim_in, 32, 16, 2);   // [n, 32, 8]
    }
    lz_conv1d_k3(A, P.c_w[1], P.c_b[1], B, n, 32, 32, 8, 2);          // [n, 32, 4]
    lz_conv1d_k3(B, P.c_w[2], P.c_b[2], A, n, 32, 64, 4, 2);          // [n, 64, 2]
    lz_conv1d_k3(A, P.c_w[3], P.c_b[3], B, n, 64, 64, 2, 2);          // [n, 64, 1]
    lz_fc(B, P.fc_w[0], P.fc_b[0], A, n, 64, 64, true);
    lz_fc(A, P.fc_w[1], P.fc_b[1], feat, n, 64, da, false);           // feat [n, dim_aud]
    if (!P.use_att) {
        for (uint32_t i = threadIdx.x; i < n * da; i += blockDim.x) enc_a[i] = feat[i];
        return;
    }
    // ---- AudioAttNet: y = feat^T [1, dim_aud, n] -> convs over the window axis -> [1, 1, n] -> Linear(n, n) -> softmax -> weighted sum
    lz_audio_transpose(feat, A, n, da);                               // permute(0, 2, 1)
    lz_conv1d_k3(A, P.ac_w[0], P.ac_b[0], B, 1, da, 16, n, 1);
    lz_conv1d_k3(B, P.ac_w[1], P.ac_b[1], A, 1, 16, 8, n, 1);
    lz_conv1d_k3(A, P.ac_w[2], P.ac_b[2], B, 1, 8, 4, n, 1);
    lz_conv1d_k3(B, P.ac_w[3], P.ac_b[3], A, 1, 4, 2, n, 1);
    lz_conv1d_k3(A, P.ac_w[4], P.ac_b[4], B, 1, 2, 1, n, 1);          // B[0..n)
    lz_fc(B, P.al_w, P.al_b, A, 1, n, n, false);                      // logits A[0..n)
    lz_audio_softmax(A, B, n);                                        // weights B[0..n)
    for (uint32_t c = threadIdx.x; c < da; c += blockDim.x) {         // torch.sum(y * x, dim=1)
        float acc = 0.0f;
        for (uint32_t t = 0; t < n; t++) acc = lz_fmaf(B[t], feat[t * da + c], acc);
        enc_a[c] = acc;
    }
}

extern "C" int lz_audio_encode(const lz_audio_params* p, const float* a, float* enc_a, void* workspace, lz_stream_t stream) {
    LZ_REQUIRE(p && a && enc_a, LZ_ERR_BAD_ARGUMENT, "audio_encode: null tensor");
    for (int i = 0; i < 4; i++) LZ_REQUIRE(p->c_w[i] && p->c_b[i], LZ_ERR_BAD_ARGUMENT, "audio_encode: missing encoder_conv weights");
    LZ_REQUIRE(p->fc_w[0] && p->fc_b[0] && p->fc_w[1] && p->fc_b[1], LZ_ERR_BAD_ARGUMENT, "audio_encode: missing encoder_fc1 weights");
    LZ_REQUIRE(p->n_win >= 1 && p->n_win <= 8 && p->dim_aud >= 1 && p->dim_aud <= 64 && p->dim_in >= 1, LZ_ERR_UNSUPPORTED,
               "audio_encode: 1..8 windows, dim_aud <= 64");
    if (p->use_att) {
        for (int i = 0; i < 5; i++) LZ_REQUIRE(p->ac_w[i] && p->ac_b[i], LZ_ERR_BAD_ARGUMENT, "audio_encode: missing attentionConvNet weights");
        LZ_REQUIRE(p->al_w && p->al_b, LZ_ERR_BAD_ARGUMENT, "audio_encode: missing attentionNet weights");
    }
    const float* conv1 = nullptr;
    if (p->dim_in >= LZ_AUDIO_WIDE) {
        LZ_REQUIRE(workspace, LZ_ERR_BAD_ARGUMENT, "audio_encode: workspace (n_win * 256 floats) required for dim_in >= %d", LZ_AUDIO_WIDE);
        const uint32_t outs = p->n_win * 32 * 8;
        hipLaunchKernelGGL(lz_k_audio_conv1_wide, dim3(lz_div_up(outs, 4)), dim3(256), 0, lz_st(stream), a, p->c_w[0], p->c_b[0],
                           reinterpret_cast<float*>(workspace), p->n_win, p->dim_in);
        conv1 = reinterpret_cast<const float*>(workspace);
    }
    hipLaunchKernelGGL(lz_k_audio_encode, dim3(1), dim3(LZ_AUDIO_THREADS), 0, lz_st(stream), *p, a, enc_a, conv1);
    LZ_CHECK_LAUNCH("audio_encode");
    return LZ_OK;
}

// ---- the whole track at once ------------------------------------------------------------------------------------------
// A clip's frames share their windows (att_mode 2: frame i reads rows [i - 4, i + 4) of the track), so AudioNet runs ONCE per row the
// frames touch plus once on a window of zeros (the padding of both ends), and the attention part gathers eight of those results per
// frame.  Every stage is the helpers of lz_audio_net.h on the same operands as lz_k_audio_encode: the same fma chains, the same bits.
#define LZ_AUDIO_TRACK_WIN 8   // windows per stage-A workgroup: what LZ_AUDIO_BUF holds

// Stage A.  Workgroup b < gridDim.x - 1: rows [lo + 8 b, ...) of the track -> feat rows 8 b ...; the last workgroup: the zero window ->
// feat_zero.  conv1 (wide inputs): the first layer's outputs, rows in the same order, the zero window's behind them.
__global__ void __launch_bounds__(LZ_AUDIO_THREADS)
lz_k_audio_track_net(lz_audio_params P, const float* __restrict__ features, const float* __restrict__ zero_win, const float* __restrict__ conv1,
                     float* __restrict__ feat, float* __restrict__ feat_zero, uint32_t lo, uint32_t nrows) {
    __shared__ float A[LZ_AUDIO_BUF], B[LZ_AUDIO_BUF];
    const bool zero = blockIdx.x == gridDim.x - 1;
    const uint32_t r0 = zero ? nrows : blockIdx.x * LZ_AUDIO_TRACK_WIN;
    const uint32_t n = zero ? 1u : (nrows - r0 < LZ_AUDIO_TRACK_WIN ? nrows - r0 : (uint32_t)LZ_AUDIO_TRACK_WIN);
    if (conv1) {
        for (uint32_t i = threadIdx.x; i < n * 32 * 8; i += blockDim.x) A[i] = conv1[(size_t)r0 * 256 + i];
        __syncthreads();
    } else {
        lz_conv1d_k3(zero ? zero_win : features + (size_t)(lo + r0) * P.dim_in * 16, P.c_w[0], P.c_b[0], A, n, P.dim_in, 32, 16, 2);
    }
    lz_conv1d_k3(A, P.c_w[1], P.c_b[1], B, n, 32, 32, 8, 2);
    lz_conv1d_k3(B, P.c_w[2], P.c_b[2], A, n, 32, 64, 4, 2);
    lz_conv1d_k3(A, P.c_w[3], P.c_b[3], B, n, 64, 64, 2, 2);
    lz_fc(B, P.fc_w[0], P.fc_b[0], A, n, 64, 64, true);
    lz_fc(A, P.fc_w[1], P.fc_b[1], zero ? feat_zero : feat + (size_t)r0 * P.dim_aud, n, 64, P.dim_aud, false);
}

// Stage B.  One workgroup per frame: window t of frame i is track row i - 8 + t (att_mode 1) or i - 4 + t (att_mode 2), a row outside
// [0, T) is the zero window (pipeline.audio_window); then AudioAttNet as in lz_k_audio_encode.
#define LZ_AUDIO_ATT_THREADS 128
__global__ void __launch_bounds__(LZ_AUDIO_ATT_THREADS)
lz_k_audio_track_att(lz_audio_params P, const float* __restrict__ feat_rows, float* __restrict__ enc_a, uint32_t T, uint32_t att_mode, uint32_t start,
                     uint32_t lo, uint32_t nrows) {
    __shared__ float A[8 * 64], B[8 * 64], feat[8 * 64];
    const uint32_t n = 8, da = P.dim_aud;
    const int64_t first = (int64_t)start + blockIdx.x - (att_mode == 1 ? 8 : 4);
    for (uint32_t j = threadIdx.x; j < n * da; j += blockDim.x) {
        const int64_t r = first + j / da;
        const uint32_t row = (r < 0 || r >= (int64_t)T) ? nrows : (uint32_t)(r - lo);
        feat[j] = feat_rows[(size_t)row * da + j % da];
    }
    __syncthreads();
    lz_audio_transpose(feat, A, n, da);
    lz_conv1d_k3(A, P.ac_w[0], P.ac_b[0], B, 1, da, 16, n, 1);
    lz_conv1d_k3(B, P.ac_w[1], P.ac_b[1], A, 1, 16, 8, n, 1);
    lz_conv1d_k3(A, P.ac_w[2], P.ac_b[2], B, 1, 8, 4, n, 1);
    lz_conv1d_k3(B, P.ac_w[3], P.ac_b[3], A, 1, 4, 2, n, 1);
    lz_conv1d_k3(A, P.ac_w[4], P.ac_b[4], B, 1, 2, 1, n, 1);
    lz_fc(B, P.al_w, P.al_b, A, 1, n, n, false);
    lz_audio_softmax(A, B, n);
    for (uint32_t c = threadIdx.x; c < da; c += blockDim.x) {
        float acc = 0.0f;
        for (uint32_t t = 0; t < n; t++) acc = lz_fmaf(B[t], feat[t * da + c], acc);
        enc_a[(size_t)blockIdx.x * da + c] = acc;
    }
}

// Stage C.  opt.smooth_lips (renderer.py:254-258, 456-460) over the clip: e[k] = w_prev e[k-1] + w_cur own[k], two products and a sum
// each rounded to f32 (torch's `l * prev + (1 - l) * enc_a`), sequential over frames, one lane per channel, in place.
__global__ void __launch_bounds__(64)
lz_k_audio_track_smooth(float* __restrict__ enc_a, const float* __restrict__ prev, uint32_t count, uint32_t da, float w_prev, float w_cur) {
    const uint32_t c = threadIdx.x;
    if (c >= da) return;
    uint32_t k = 0;
    float e;
    if (prev) e = prev[c];
    else { e = enc_a[c]; k = 1; }
    for (; k < count; k++) {
        const float a = w_prev * e, b = w_cur * enc_a[(size_t)k * da + c];
        e = a + b;
        enc_a[(size_t)k * da + c] = e;
    }
}

// rows of the track the frames [start, start + count) read: [lo, lo + nrows)
static void lz_audio_track_rows(uint32_t T, uint32_t att_mode, uint32_t start, uint32_t count, uint32_t* lo, uint32_t* nrows) {
    int64_t a = start, b = (int64_t)start + count;
    if (att_mode == 1) { a -= 8; b -= 1; }
    if (att_mode == 2) { a -= 4; b += 3; }
    if (a < 0) a = 0;
    if (b > (int64_t)T) b = T;
    *lo = (uint32_t)a;
    *nrows = b > a ? (uint32_t)(b - a) : 0u;
}

// workspace floats: [zero window dim_in * 16 | feat (count + 8) * dim_aud | conv1 (count + 8) * 256 when wide]
extern "C" size_t lz_audio_track_workspace(uint32_t count, uint32_t dim_in, uint32_t dim_aud) {
    const size_t rows = (size_t)count + 8;   // at most count + 7 rows of the track, and the zero window
    return sizeof(float) * ((size_t)dim_in * 16 + rows * dim_aud + (dim_in >= LZ_AUDIO_WIDE ? rows * 256 : 0));
}

extern "C" int lz_audio_encode_track(const lz_audio_params* p, const float* features, uint32_t T, uint32_t att_mode, uint32_t start, uint32_t count,
                                     float w_prev, float w_cur, const float* enc_a_prev, float* enc_a, void* workspace, lz_stream_t stream) {
    if (count == 0) return LZ_OK;
    LZ_REQUIRE(p && features && enc_a && workspace, LZ_ERR_BAD_ARGUMENT, "audio_encode_track: null tensor");
    LZ_REQUIRE((uint64_t)start + count <= T, LZ_ERR_BAD_ARGUMENT, "audio_encode_track: frames [%u, %u + %u) outside the track of %u", start, start, count, T);
    LZ_REQUIRE(att_mode <= 2, LZ_ERR_UNSUPPORTED, "audio_encode_track: att_mode %u (0, 1 or 2)", att_mode);
    for (int i = 0; i < 4; i++) LZ_REQUIRE(p->c_w[i] && p->c_b[i], LZ_ERR_BAD_ARGUMENT, "audio_encode_track: missing encoder_conv weights");
    LZ_REQUIRE(p->fc_w[0] && p->fc_b[0] && p->fc_w[1] && p->fc_b[1], LZ_ERR_BAD_ARGUMENT, "audio_encode_track: missing encoder_fc1 weights");
    LZ_REQUIRE(p->dim_aud >= 1 && p->dim_aud <= 64 && p->dim_in >= 1, LZ_ERR_UNSUPPORTED, "audio_encode_track: dim_aud <= 64");
    if (att_mode) {
        LZ_REQUIRE(p->use_att && p->al_w && p->al_b, LZ_ERR_UNSUPPORTED, "audio_encode_track: att_mode %u needs the attention net's weights", att_mode);
        for (int i = 0; i < 5; i++) LZ_REQUIRE(p->ac_w[i] && p->ac_b[i], LZ_ERR_UNSUPPORTED, "audio_encode_track: missing attentionConvNet weights");
    }
    uint32_t lo, nrows;
    lz_audio_track_rows(T, att_mode, start, count, &lo, &nrows);
    hipStream_t st = lz_st(stream);
    float* zero_win = reinterpret_cast<float*>(workspace);
    float* feat = zero_win + (size_t)p->dim_in * 16;
    float* feat_zero = feat + (size_t)nrows * p->dim_aud;
    float* conv1 = nullptr;
    const size_t win = (size_t)p->dim_in * 16;
    if (hipMemsetAsync(zero_win, 0, win * sizeof(float), st) != hipSuccess) {
        lz_set_error("audio_encode_track: clearing the zero window failed");
        return LZ_ERR_BAD_ARGUMENT;
    }
    if (p->dim_in >= LZ_AUDIO_WIDE) {
        conv1 = feat + ((size_t)count + 8) * p->dim_aud;
        if (nrows)
            hipLaunchKernelGGL(lz_k_audio_conv1_wide, dim3(lz_div_up((uint64_t)nrows * 256, 4)), dim3(256), 0, st, features + lo * win, p->c_w[0], p->c_b[0],
                               conv1, nrows, p->dim_in);
        hipLaunchKernelGGL(lz_k_audio_conv1_wide, dim3(64), dim3(256), 0, st, zero_win, p->c_w[0], p->c_b[0], conv1 + (size_t)nrows * 256, 1u, p->dim_in);
    }
    // att_mode 0: the code of frame i is AudioNet of row i -- stage A writes enc_a itself (lo = start, nrows = count)
    hipLaunchKernelGGL(lz_k_audio_track_net, dim3(lz_div_up(nrows, LZ_AUDIO_TRACK_WIN) + 1), dim3(LZ_AUDIO_THREADS), 0, st, *p, features, zero_win, conv1,
                       att_mode ? feat : enc_a, feat_zero, lo, nrows);
    if (att_mode)
        hipLaunchKernelGGL(lz_k_audio_track_att, dim3(count), dim3(LZ_AUDIO_ATT_THREADS), 0, st, *p, feat, enc_a, T, att_mode, start, lo, nrows);
    if (w_prev != 0.0f || w_cur != 0.0f)
        hipLaunchKernelGGL(lz_k_audio_track_smooth, dim3(1), dim3(64), 0, st, enc_a, enc_a_prev, count, p->dim_aud, w_prev, w_cur);
    LZ_CHECK_LAUNCH("audio_encode_track");
    return LZ_OK;
}
