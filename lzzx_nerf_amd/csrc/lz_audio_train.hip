// lz_audio_train.hip -- backward of NeRFNetwork.encode_audio (nerf_triplane/network.py:226-240) for training: the gradients of every
// AudioNet (network.py:40-70) and AudioAttNet (network.py:9-37) parameter, which the reference's head-stage step hands to its optimizer
// (get_params, network.py:333, 344).  The forward is lz_audio_encode (lz_audio.hip) unchanged.  Two launches:
//   1. lz_k_audio_train_chain, ONE workgroup like lz_k_audio_encode: recompute every activation into LDS with the inference kernel's
//      own helpers (lz_audio_net.h: the same bits), then walk the layers backwards -- weighted sum, softmax, attentionNet.0, the five
//      attention convs, encoder_fc1, encoder_conv.6 / .4 / .2 -- writing each layer's weight and bias gradients and keeping the input
//      gradient in LDS; the gradient at encoder_conv.0's pre-activation goes to the workspace.
//   2. lz_k_audio_train_conv1_grad: encoder_conv.0's gradients (32 x dim_in x 3 weights + 32 biases; 98 304 weights for HuBERT), one
//      output per thread over the whole chip.
// Every gradient element is one thread's sum in a fixed order (windows outer, positions inner; output channels outer, taps inner for
// input gradients, written as a gather over outputs): no atomics, the same bits on every call, and exactly linear in the upstream
// gradient (a power-of-two scale of d_enc_a scales every gradient by exactly that power).
#include "lz_audio_net.h"

// d/dv of nn.LeakyReLU(0.02, inplace=True): torch tests the in-place OUTPUT, y > 0 (0 takes the slope branch)
__device__ __forceinline__ float lz_lrelu_bwd(float y, float g) { return y > 0.0f ? g : 0.02f * g; }

// Backward of y = lrelu(conv1d(x, w, stride, padding 1) + b) (lz_conv1d_k3's layer).  gy [n][Cout][Lout] -> gp (pre-activation
// gradient, LDS), gw [Cout][Cin][3] and gb [Cout] (written), and when gx is not null the input gradient gx [n][Cin][Lin] (may alias gy:
// gy is read only before the first barrier).
__device__ __forceinline__ void lz_conv1d_k3_bwd(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ w,
                                                 const float* gy, float* __restrict__ gp, float* __restrict__ gw, float* __restrict__ gb,
                                                 float* gx, uint32_t n, uint32_t Cin, uint32_t Cout, uint32_t Lin, uint32_t stride) {
    const uint32_t Lout = (Lin - 1) / stride + 1;
    for (uint32_t i = threadIdx.x; i < n * Cout * Lout; i += blockDim.x) gp[i] = lz_lrelu_bwd(y[i], gy[i]);
    __syncthreads();
    const uint32_t nw = Cout * Cin * 3, total = nw + Cout + (gx ? n * Cin * Lin : 0u);
    for (uint32_t idx = threadIdx.x; idx < total; idx += blockDim.x) {
        if (idx < nw) {   // dL/dw[o][ci][k] = sum over windows, output positions of gp[win][o][t] x[win][ci][t*stride + k - 1]
            const uint32_t k = idx % 3, o = idx / 3 / Cin, ci = idx / 3 - o * Cin;
            float acc = 0.0f;
            for (uint32_t win = 0; win < n; win++)
                for (uint32_t t = 0; t < Lout; t++) {
                    const int pos = (int)(t * stride + k) - 1;
                    if (pos >= 0 && pos < (int)Lin) acc = lz_fmaf(gp[(win * Cout + o) * Lout + t], x[(size_t)(win * Cin + ci) * Lin + pos], acc);
                }
            gw[idx] = acc;
        } else if (idx < nw + Cout) {
            const uint32_t o = idx - nw;
            float acc = 0.0f;
            for (uint32_t win = 0; win < n; win++)
                for (uint32_t t = 0; t < Lout; t++) acc += gp[(win * Cout + o) * Lout + t];
            gb[o] = acc;
        } else {          // dL/dx[win][ci][p] = sum over o, k with p = t*stride + k - 1 of gp[win][o][t] w[o][ci][k]
            const uint32_t j = idx - nw - Cout, p = j % Lin, win = n == 1 ? 0u : j / Lin / Cin, ci = j / Lin - win * Cin;
            float acc = 0.0f;
            for (uint32_t o = 0; o < Cout; o++)
#pragma unroll
                for (uint32_t k = 0; k < 3; k++) {
                    const int q = (int)(p + 1) - (int)k;   // t * stride
                    if (q >= 0 && q % (int)stride == 0 && q / (int)stride < (int)Lout)
                        acc = lz_fmaf(gp[(win * Cout + o) * Lout + q / stride], w[(o * Cin + ci) * 3 + k], acc);
                }
            gx[j] = acc;
        }
    }
    __syncthreads();
}

// Backward of y = act(x w^T + b) (lz_fc's layer; y null: no activation).  gy [n][N] -> gp (LDS), gw [N][K], gb [N] (written), gx [n][K]
// when not null (may alias gy)
__device__ __forceinline__ void lz_fc_bwd(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ w, const float* gy,
                                          float* __restrict__ gp, float* __restrict__ gw, float* __restrict__ gb, float* gx, uint32_t n, uint32_t K,
                                          uint32_t N) {
    for (uint32_t i = threadIdx.x; i < n * N; i += blockDim.x) gp[i] = y ? lz_lrelu_bwd(y[i], gy[i]) : gy[i];
    __syncthreads();
    const uint32_t nw = N * K, total = nw + N + (gx ? n * K : 0u);
    for (uint32_t idx = threadIdx.x; idx < total; idx += blockDim.x) {
        if (idx < nw) {
            const uint32_t o = idx / K, k = idx % K;
            float acc = 0.0f;
            for (uint32_t r = 0; r < n; r++) acc = lz_fmaf(gp[r * N + o], x[r * K + k], acc);
            gw[idx] = acc;
        } else if (idx < nw + N) {
            const uint32_t o = idx - nw;
            float acc = 0.0f;
            for (uint32_t r = 0; r < n; r++) acc += gp[r * N + o];
            gb[o] = acc;
        } else {
            const uint32_t j = idx - nw - N, r = j / K, k = j % K;
            float acc = 0.0f;
            for (uint32_t o = 0; o < N; o++) acc = lz_fmaf(w[o * K + k], gp[r * N + o], acc);
            gx[j] = acc;
        }
    }
    __syncthreads();
}

__global__ void __launch_bounds__(LZ_AUDIO_THREADS)
lz_k_audio_train_chain(lz_audio_params P, lz_audio_grads G, const float* __restrict__ a, const float* __restrict__ conv1,
                       const float* __restrict__ g_enc, float* __restrict__ g_pre1) {
    // activations of the forward (8 windows at most): AudioNet, then AudioAttNet's transposed input, its five conv outputs, logits, weights
    __shared__ float y1[8 * 32 * 8], y2[8 * 32 * 4], y3[8 * 64 * 2], h0[8 * 64], h1[8 * 64], feat[8 * 64];
    __shared__ float z0[64 * 8], z1[16 * 8], z2[8 * 8], z3[4 * 8], z4[2 * 8], z5[8], logit[8], s[8], gs[8], gl[8];
    __shared__ float GA[LZ_AUDIO_BUF], GB[LZ_AUDIO_BUF], gfeat[8 * 64];   // gradients: a layer's input / pre-activation, AudioNet's output
    const uint32_t n = P.n_win, da = P.dim_aud;

    // ---- forward, in lz_k_audio_encode's order and arithmetic
    if (conv1) {
        for (uint32_t i = threadIdx.x; i < n * 32 * 8; i += blockDim.x) y1[i] = conv1[i];
        __syncthreads();
    } else {
        lz_conv1d_k3(a, P.c_w[0], P.c_b[0], y1, n, P.dim_in, 32, 16, 2);
    }
    lz_conv1d_k3(y1, P.c_w[1], P.c_b[1], y2, n, 32, 32, 8, 2);
    lz_conv1d_k3(y2, P.c_w[2], P.c_b[2], y3, n, 32, 64, 4, 2);
    lz_conv1d_k3(y3, P.c_w[3], P.c_b[3], h0, n, 64, 64, 2, 2);
    lz_fc(h0, P.fc_w[0], P.fc_b[0], h1, n, 64, 64, true);
    lz_fc(h1, P.fc_w[1], P.fc_b[1], feat, n, 64, da, false);
    if (P.use_att) {   // n_win = 8 (checked on the host): the window count is a constant on this branch
        constexpr uint32_t T = 8;
        lz_audio_transpose(feat, z0, T, da);
        lz_conv1d_k3(z0, P.ac_w[0], P.ac_b[0], z1, 1, da, 16, T, 1);
        lz_conv1d_k3(z1, P.ac_w[1], P.ac_b[1], z2, 1, 16, 8, T, 1);
        lz_conv1d_k3(z2, P.ac_w[2], P.ac_b[2], z3, 1, 8, 4, T, 1);
        lz_conv1d_k3(z3, P.ac_w[3], P.ac_b[3], z4, 1, 4, 2, T, 1);
        lz_conv1d_k3(z4, P.ac_w[4], P.ac_b[4], z5, 1, 2, 1, T, 1);
        lz_fc(z5, P.al_w, P.al_b, logit, 1, T, T, false);
        lz_audio_softmax(logit, s, T);

        // ---- enc_a[c] = sum_t s[t] feat[t][c]:  dL/ds[t] = sum_c g[c] feat[t][c]
        for (uint32_t t = threadIdx.x; t < T; t += blockDim.x) {
            float acc = 0.0f;
            for (uint32_t c = 0; c < da; c++) acc = lz_fmaf(g_enc[c], feat[t * da + c], acc);
            gs[t] = acc;
        }
        __syncthreads();
        if (threadIdx.x == 0) {   // softmax: dL/dlogit[t] = s[t] (gs[t] - sum_u s[u] gs[u]), the sum in index order
            float dot = 0.0f;
            for (uint32_t u = 0; u < T; u++) dot = lz_fmaf(s[u], gs[u], dot);
            for (uint32_t t = 0; t < T; t++) gl[t] = s[t] * (gs[t] - dot);
        }
        __syncthreads();
        lz_fc_bwd(z5, nullptr, P.al_w, gl, GB, G.g_al_w, G.g_al_b, GA, 1, T, T);                // GA = dL/dz5 [1, T]
        lz_conv1d_k3_bwd(z4, z5, P.ac_w[4], GA, GB, G.g_ac_w[4], G.g_ac_b[4], GA, 1, 2, 1, T, 1);
        lz_conv1d_k3_bwd(z3, z4, P.ac_w[3], GA, GB, G.g_ac_w[3], G.g_ac_b[3], GA, 1, 4, 2, T, 1);
        lz_conv1d_k3_bwd(z2, z3, P.ac_w[2], GA, GB, G.g_ac_w[2], G.g_ac_b[2], GA, 1, 8, 4, T, 1);
        lz_conv1d_k3_bwd(z1, z2, P.ac_w[1], GA, GB, G.g_ac_w[1], G.g_ac_b[1], GA, 1, 16, 8, T, 1);
        lz_conv1d_k3_bwd(z0, z1, P.ac_w[0], GA, GB, G.g_ac_w[0], G.g_ac_b[0], GA, 1, da, 16, T, 1);   // GA = dL/dz0 [da, T]
        // feat feeds both the weighted sum (s[t] g[c]) and, transposed, the attention convs (dL/dz0[c][t])
        for (uint32_t j = threadIdx.x; j < T * da; j += blockDim.x) {
            const uint32_t c = j / T, t = j % T;
            gfeat[t * da + c] = s[t] * g_enc[c] + GA[j];
        }
    } else {
        for (uint32_t i = threadIdx.x; i < n * da; i += blockDim.x) gfeat[i] = g_enc[i];
    }
    __syncthreads();

    // ---- AudioNet, last layer first
    lz_fc_bwd(h1, nullptr, P.fc_w[1], gfeat, GB, G.g_fc_w[1], G.g_fc_b[1], GA, n, 64, da);        // GA = dL/dh1
    lz_fc_bwd(h0, h1, P.fc_w[0], GA, GB, G.g_fc_w[0], G.g_fc_b[0], GA, n, 64, 64);                 // GA = dL/dh0 = dL/dy4 [n, 64, 1]
    lz_conv1d_k3_bwd(y3, h0, P.c_w[3], GA, GB, G.g_c_w[3], G.g_c_b[3], GA, n, 64, 64, 2, 2);       // GA = dL/dy3 [n, 64, 2]
    lz_conv1d_k3_bwd(y2, y3, P.c_w[2], GA, GB, G.g_c_w[2], G.g_c_b[2], GA, n, 32, 64, 4, 2);       // GA = dL/dy2 [n, 32, 4]
    lz_conv1d_k3_bwd(y1, y2, P.c_w[1], GA, GB, G.g_c_w[1], G.g_c_b[1], GA, n, 32, 32, 8, 2);       // GA = dL/dy1 [n, 32, 8]
    for (uint32_t i = threadIdx.x; i < n * 32 * 8; i += blockDim.x) g_pre1[i] = lz_lrelu_bwd(y1[i], GA[i]);
}

// encoder_conv.0's gradients from its pre-activation gradient gp [n, 32, 8] (staged in LDS) and the windows a [n, Cin, 16]: thread idx
// < 32 * Cin * 3 owns weight (o, ci, k), the next 32 the biases; each sums its n * 8 terms, windows outer, positions inner
__global__ void __launch_bounds__(256)
lz_k_audio_train_conv1_grad(const float* __restrict__ a, const float* __restrict__ g_pre1, float* __restrict__ gw, float* __restrict__ gb, uint32_t n,
                            uint32_t Cin) {
    __shared__ float gp[8 * 32 * 8];
    for (uint32_t i = threadIdx.x; i < n * 256; i += blockDim.x) gp[i] = g_pre1[i];
    __syncthreads();
    const uint32_t nw = 32 * Cin * 3, idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx < nw) {
        const uint32_t k = idx % 3, ci = (idx / 3) % Cin, o = idx / (3 * Cin);
        float acc = 0.0f;
        for (uint32_t win = 0; win < n; win++) {
            const float* xr = a + ((size_t)win * Cin + ci) * 16;
#pragma unroll
            for (uint32_t t = 0; t < 8; t++) {
                const int pos = (int)(2 * t + k) - 1;
                if (pos >= 0) acc = lz_fmaf(gp[win * 256 + o * 8 + t], xr[pos], acc);   // pos <= 15 always
            }
        }
        gw[idx] = acc;
    } else if (idx < nw + 32) {
        const uint32_t o = idx - nw;
        float acc = 0.0f;
        for (uint32_t win = 0; win < n; win++)
            for (uint32_t t = 0; t < 8; t++) acc += gp[win * 256 + o * 8 + t];
        gb[o] = acc;
    }
}

extern "C" size_t lz_audio_train_workspace(void) { return 8 * 32 * 8 * sizeof(float); }

extern "C" int lz_audio_train_backward(const lz_audio_params* p, const float* a, const float* conv1_out, const float* d_enc_a, const lz_audio_grads* g,
                                       void* workspace, lz_stream_t stream) {
    LZ_REQUIRE(p && g, LZ_ERR_BAD_ARGUMENT, "audio_train_backward: null parameter or gradient block");
    LZ_REQUIRE(a && d_enc_a, LZ_ERR_BAD_ARGUMENT, "audio_train_backward: null tensor");
    LZ_REQUIRE(workspace, LZ_ERR_BAD_ARGUMENT, "audio_train_backward: workspace (lz_audio_train_workspace() bytes) required");
    for (int i = 0; i < 4; i++) LZ_REQUIRE(p->c_w[i] && p->c_b[i], LZ_ERR_BAD_ARGUMENT, "audio_train_backward: missing encoder_conv weights");
    LZ_REQUIRE(p->fc_w[0] && p->fc_b[0] && p->fc_w[1] && p->fc_b[1], LZ_ERR_BAD_ARGUMENT, "audio_train_backward: missing encoder_fc1 weights");
    LZ_REQUIRE(p->n_win >= 1 && p->n_win <= 8 && p->dim_aud >= 1 && p->dim_aud <= 64 && p->dim_in >= 1, LZ_ERR_UNSUPPORTED,
               "audio_train_backward: 1..8 windows, dim_aud <= 64");
    for (int i = 0; i < 4; i++) LZ_REQUIRE(g->g_c_w[i] && g->g_c_b[i], LZ_ERR_BAD_ARGUMENT, "audio_train_backward: missing encoder_conv gradient");
    LZ_REQUIRE(g->g_fc_w[0] && g->g_fc_b[0] && g->g_fc_w[1] && g->g_fc_b[1], LZ_ERR_BAD_ARGUMENT, "audio_train_backward: missing encoder_fc1 gradient");
    if (p->use_att) {
        LZ_REQUIRE(p->n_win == 8, LZ_ERR_UNSUPPORTED, "audio_train_backward: AudioAttNet takes 8 windows, got %u", p->n_win);
        for (int i = 0; i < 5; i++) {
            LZ_REQUIRE(p->ac_w[i] && p->ac_b[i], LZ_ERR_BAD_ARGUMENT, "audio_train_backward: missing attentionConvNet weights");
            LZ_REQUIRE(g->g_ac_w[i] && g->g_ac_b[i], LZ_ERR_BAD_ARGUMENT, "audio_train_backward: missing attentionConvNet gradient");
        }
        LZ_REQUIRE(p->al_w && p->al_b, LZ_ERR_BAD_ARGUMENT, "audio_train_backward: missing attentionNet weights");
        LZ_REQUIRE(g->g_al_w && g->g_al_b, LZ_ERR_BAD_ARGUMENT, "audio_train_backward: missing attentionNet gradient");
    }
    const bool wide = p->dim_in >= LZ_AUDIO_WIDE;
    LZ_REQUIRE(!wide || conv1_out, LZ_ERR_BAD_ARGUMENT, "audio_train_backward: conv1_out (lz_audio_encode's workspace) required for dim_in >= %d",
               LZ_AUDIO_WIDE);
    float* g_pre1 = reinterpret_cast<float*>(workspace);
    hipLaunchKernelGGL(lz_k_audio_train_chain, dim3(1), dim3(LZ_AUDIO_THREADS), 0, lz_st(stream), *p, *g, a, wide ? conv1_out : nullptr, d_enc_a, g_pre1);
    const uint32_t outs = 32 * p->dim_in * 3 + 32;
    hipLaunchKernelGGL(lz_k_audio_train_conv1_grad, dim3(lz_div_up(outs, 256)), dim3(256), 0, lz_st(stream), a, g_pre1, g->g_c_w[0], g->g_c_b[0],
                       p->n_win, p->dim_in);
    LZ_CHECK_LAUNCH("audio_train_backward");
    return LZ_OK;
}
