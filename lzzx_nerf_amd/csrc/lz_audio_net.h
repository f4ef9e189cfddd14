// lz_audio_net.h -- the layer arithmetic of NeRFNetwork.encode_audio (nerf_triplane/network.py:226-240), shared by the one-launch
// inference kernel (lz_audio.hip) and the training backward (lz_audio_train.hip): one instance of the forward arithmetic, so the
// backward's recomputed activations are the inference kernel's bits.  Every helper is a loop of the whole workgroup over its outputs,
// ending in a barrier.  Arithmetic = explicit f32 fma chains (input channel outer, tap inner; bias added after the chain), restated by
// oracle/audio.py.
#pragma once
#include "lz_common.h"
#include "lzzx_detmath.h"

#define LZ_AUDIO_THREADS 1024
#define LZ_AUDIO_BUF 2048   // floats: largest activation is [8, 32, 8]
#define LZ_AUDIO_WIDE 128   // dim_in from which the wide first layer is used; part of the arithmetic contract (oracle/audio.py)

__device__ __forceinline__ float lz_lrelu(float v) { return v > 0.0f ? v : 0.02f * v; }   // nn.LeakyReLU(0.02)

// y[n][Cout][Lout] = lrelu(conv1d(x[n][Cin][Lin], w[Cout][Cin][3], stride, padding 1) + b)
__device__ __forceinline__ void lz_conv1d_k3(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ b,
                                             float* __restrict__ y, uint32_t n, uint32_t Cin, uint32_t Cout, uint32_t Lin, uint32_t stride) {
    const uint32_t Lout = (Lin - 1) / stride + 1;   // (Lin + 2 - 3) / stride + 1
    for (uint32_t idx = threadIdx.x; idx < n * Cout * Lout; idx += blockDim.x) {
        const uint32_t t = idx % Lout, o = (idx / Lout) % Cout, win = idx / (Lout * Cout);
        const float* xr = x + (size_t)win * Cin * Lin;
        const float* wr = w + (size_t)o * Cin * 3;
        float acc = 0.0f;
        for (uint32_t ci = 0; ci < Cin; ci++)
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const int pos = (int)(t * stride) + k - 1;
                if (pos >= 0 && pos < (int)Lin) acc = lz_fmaf(wr[ci * 3 + k], xr[(size_t)ci * Lin + pos], acc);
            }
        y[idx] = lz_lrelu(acc + b[o]);
    }
    __syncthreads();
}

// y[n][N] = act(x[n][K] . w[N][K]^T + b)
__device__ __forceinline__ void lz_fc(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ b, float* __restrict__ y,
                                      uint32_t n, uint32_t K, uint32_t N, bool lrelu) {
    for (uint32_t idx = threadIdx.x; idx < n * N; idx += blockDim.x) {
        const uint32_t o = idx % N, r = idx / N;
        float acc = 0.0f;
        for (uint32_t k = 0; k < K; k++) acc = lz_fmaf(w[(size_t)o * K + k], x[(size_t)r * K + k], acc);
        acc += b[o];
        y[idx] = lrelu ? lz_lrelu(acc) : acc;
    }
    __syncthreads();
}

// AudioAttNet's input: y[c][t] = feat[t][c]   (x.permute(0, 2, 1), network.py:33); indexed by the output, so a constant n folds
__device__ __forceinline__ void lz_audio_transpose(const float* __restrict__ feat, float* __restrict__ y, uint32_t n, uint32_t da) {
    for (uint32_t j = threadIdx.x; j < n * da; j += blockDim.x) y[j] = feat[(j % n) * da + j / n];
    __syncthreads();
}

// nn.Softmax(dim=1) over n <= 8 logits on one thread: max, exp, sum in index order, divide
__device__ __forceinline__ void lz_audio_softmax(const float* __restrict__ logit, float* __restrict__ s, uint32_t n) {
    if (threadIdx.x == 0) {
        float m = logit[0];
        for (uint32_t i = 1; i < n; i++) m = lz_fmaxf(m, logit[i]);
        float sum = 0.0f;
        for (uint32_t i = 0; i < n; i++) { s[i] = lz_expf(logit[i] - m); sum += s[i]; }
        for (uint32_t i = 0; i < n; i++) s[i] = s[i] / sum;
    }
    __syncthreads();
}
