// lz_objective.hip -- the reference's training objective (TrainerUtil.train_step, TrainerUtil.py:233-367) on the device.
//
// Head:  P = clamp(image_raw + (1 - ws) bg, 0, 1) (renderer.py:380-382), the per-ray MSE, the uncertainty weighting and its NLL /
//        static terms, the weights-sum entropy, the two ambient attention terms: two launches forward (softmax statistics of the
//        uncertainty, then the per-ray terms), one elementwise launch backward.
// Torso: the colour MSE plus the anchor term (the function returns at :244, before the torso-alpha entropy).
// Jitter regulariser (:346-365): sum of the enabled means of (raw - reg)^2 over the samples, forward and backward.
//
// Reductions: every workgroup reduces its items in f64 through a fixed LDS tree and stores its partials; the last workgroup to take the
// ticket (agent-scope release before the add, acquire after it) combines the partials in index order, writes the result and puts the
// ticket back to 0.  No float atomics, no host synchronisation; the grid is a function of the item count alone, so the same inputs give
// the same bits on every call.  The per-item arithmetic is f32 in the reference's operation order; only the sums are wider.
#include "lz_common.h"
#include "lzzx_detmath.h"

#define LZO_THREADS 256
#define LZO_SLOTS 8                      // f64 partials per workgroup
#define LZO_TICKETS_BYTES 64
// the entropy's clamp bounds as torch sees the Python scalars 1e-5 and 1 - 1e-5 (a double, rounded once to f32)
#define LZO_A_LO ((float)1e-5)
#define LZO_A_HI ((float)(1.0 - 1e-5))
enum { LZO_T_SOFTMAX = 0, LZO_T_HEAD = 1, LZO_T_TORSO = 2, LZO_T_JITTER = 3 };

static_assert(LZ_OBJECTIVE_MAX_GROUPS * LZO_SLOTS * 8 + LZO_TICKETS_BYTES == LZ_OBJECTIVE_WS_BYTES, "workspace layout");

static inline uint32_t lzo_groups(uint32_t n) {
    const uint32_t g = lz_div_up(n, LZO_THREADS);
    return g < LZ_OBJECTIVE_MAX_GROUPS ? g : LZ_OBJECTIVE_MAX_GROUPS;
}

__device__ __forceinline__ int32_t* lzo_ticket(void* ws, int which) { return reinterpret_cast<int32_t*>(ws) + which; }
__device__ __forceinline__ double* lzo_partials(void* ws) { return reinterpret_cast<double*>(reinterpret_cast<char*>(ws) + LZO_TICKETS_BYTES); }

// fixed-order tree over the workgroup: red[k * LZO_THREADS + tid] holds thread tid's value k on entry, the workgroup's sum at red[k * LZO_THREADS]
template <int K>
__device__ __forceinline__ void lzo_tree_sum(double* red) {
#pragma unroll
    for (int s = LZO_THREADS / 2; s > 0; s >>= 1) {
        __syncthreads();
        if ((int)threadIdx.x < s) {
#pragma unroll
            for (int k = 0; k < K; ++k) red[k * LZO_THREADS + threadIdx.x] += red[k * LZO_THREADS + threadIdx.x + s];
        }
    }
    __syncthreads();
}

// Publish this workgroup's partials (already stored by thread 0) and take the ticket; true in every thread of the last workgroup, after
// which all partials are visible to it.  The recipe: stores drained, agent release, drained again (the compiler may drop the fence's own
// wait), relaxed agent add; the last arriver acquires at agent scope before anyone reads.  `flag` is a word of the caller's LDS array.
__device__ __forceinline__ bool lzo_arrive_last(int32_t* ticket, double* flag) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const int t = __hip_atomic_fetch_add(ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const bool last = t == (int)gridDim.x - 1;
        if (last) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __hip_atomic_store(ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // ready for the next launch: no memset
        }
        *flag = last ? 1.0 : 0.0;
    }
    __syncthreads();
    return *flag != 0.0;
}

// the last workgroup's combine: red[k * LZO_THREADS] = sum over workgroups g = 0, 1, ... of partial k (each thread a fixed stride of g, then the tree)
template <int K>
__device__ __forceinline__ void lzo_combine(const double* part, double* red) {
    double acc[K];
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = 0.0;
    for (uint32_t g = threadIdx.x; g < gridDim.x; g += LZO_THREADS)
#pragma unroll
        for (int k = 0; k < K; ++k) acc[k] += part[(size_t)g * LZO_SLOTS + k];
#pragma unroll
    for (int k = 0; k < K; ++k) red[k * LZO_THREADS + threadIdx.x] = acc[k];
    lzo_tree_sum<K>(red);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// head: softmax statistics of the uncertainty (TrainerUtil.py:259): stats[0] = max u, stats[1] = sum exp(u - max u)
// ---------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(LZO_THREADS) lz_k_obj_softmax_stats(const float* __restrict__ u, uint32_t N, float* __restrict__ stats, void* ws) {
    __shared__ double red[LZO_THREADS + 1];
    float* redf = reinterpret_cast<float*>(red);
    const uint32_t stride = gridDim.x * LZO_THREADS;
    float m = -INFINITY;
    for (uint32_t i = blockIdx.x * LZO_THREADS + threadIdx.x; i < N; i += stride) m = lz_fmaxf(m, u[i]);
    redf[threadIdx.x] = m;
    for (int s = LZO_THREADS / 2; s > 0; s >>= 1) {
        __syncthreads();
        if ((int)threadIdx.x < s) redf[threadIdx.x] = lz_fmaxf(redf[threadIdx.x], redf[threadIdx.x + s]);
    }
    __syncthreads();
    const float mb = redf[0];
    __syncthreads();
    double sum = 0.0;
    for (uint32_t i = blockIdx.x * LZO_THREADS + threadIdx.x; i < N; i += stride) sum += (double)lz_expf(u[i] - mb);
    red[threadIdx.x] = sum;
    lzo_tree_sum<1>(red);
    double* part = lzo_partials(ws);
    if (threadIdx.x == 0) {
        part[(size_t)blockIdx.x * LZO_SLOTS + 0] = (double)mb;
        part[(size_t)blockIdx.x * LZO_SLOTS + 1] = red[0];
    }
    if (!lzo_arrive_last(lzo_ticket(ws, LZO_T_SOFTMAX), &red[LZO_THREADS])) return;
    // max over the workgroups' maxima, then their sums rescaled to it, in workgroup order
    m = -INFINITY;
    for (uint32_t g = threadIdx.x; g < gridDim.x; g += LZO_THREADS) m = lz_fmaxf(m, (float)part[(size_t)g * LZO_SLOTS]);
    redf[threadIdx.x] = m;
    for (int s = LZO_THREADS / 2; s > 0; s >>= 1) {
        __syncthreads();
        if ((int)threadIdx.x < s) redf[threadIdx.x] = lz_fmaxf(redf[threadIdx.x], redf[threadIdx.x + s]);
    }
    __syncthreads();
    const float M = redf[0];
    __syncthreads();
    sum = 0.0;
    for (uint32_t g = threadIdx.x; g < gridDim.x; g += LZO_THREADS)
        sum += part[(size_t)g * LZO_SLOTS + 1] * (double)lz_expf((float)part[(size_t)g * LZO_SLOTS] - M);
    red[threadIdx.x] = sum;
    lzo_tree_sum<1>(red);
    if (threadIdx.x == 0) {
        stats[0] = M;
        stats[1] = (float)red[0];
    }
}

struct LzObjHead {
    const float* image;     // [N,3] image_raw
    const float* ws;        // [N]
    const float* bg;        // bg_mode 1: [1], 2: [3], 3: [N,3]
    const float* target;    // [N,3]
    const uint8_t* face;    // [N] 0 / 1
    const float* unc;       // [N]
    const float* aud;       // [N]
    const float* eye;       // [N]
    const float* stats;     // aux + 6: max u, sum exp(u - max)
    uint32_t N, bg_mode, flags;
    float bg_scalar, sf, one_minus_sf, sf_static, lam, max_steps;
};

__device__ __forceinline__ float lzo_bg(const LzObjHead& A, uint32_t i, int c) {
    switch (A.bg_mode) {
        case 0: return A.bg_scalar;
        case 1: return A.bg[0];
        case 2: return A.bg[c];
        default: return A.bg[(size_t)i * 3 + c];
    }
}

__device__ __forceinline__ float lzo_log2(float x) { return lz_logf(x) * 1.44269502162933349609375f; }

// everything one ray contributes, forward (acc) and, with BWD, the gradients' ingredients
struct LzObjRay {
    float v[3], d[3], b[3], sq, factor, beta, nrm, lb, A;
    bool f;
};

__device__ __forceinline__ void lzo_ray(const LzObjHead& A, uint32_t i, LzObjRay& r, float* P, double acc[6]) {
    const float w_s = A.ws[i];
    const float one_m_ws = 1.0f - w_s;
    r.sq = 0.0f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        r.b[c] = lzo_bg(A, i, c);
        r.v[c] = A.image[(size_t)i * 3 + c] + one_m_ws * r.b[c];      // two roundings, as the torch expression
        P[c] = lz_clampf(r.v[c], 0.0f, 1.0f);
        r.d[c] = P[c] - A.target[(size_t)i * 3 + c];
    }
    r.sq = r.d[0] * r.d[0] + r.d[1] * r.d[1] + r.d[2] * r.d[2];
    const float mse = r.sq / 3.0f;
    r.f = A.face[i] != 0;
    r.factor = 1.0f;
    acc[1] = acc[2] = acc[4] = acc[5] = 0.0;
    if (A.flags & LZ_OBJ_UNC) {
        const float u = A.unc[i];
        const float w = lz_expf(u - A.stats[0]) / A.stats[1] * (float)A.N;            // softmax(u) * N, detached
        r.factor = 0.2f + 0.8f * lz_clampf(A.one_minus_sf + A.sf * w, 0.0f, 10.0f);
        r.beta = u + 1.0f;
        r.nrm = sqrtf(r.sq);                                                             // ||P - T||, detached
        r.lb = lz_logf(r.beta);
        const float nll = r.nrm / (2.0f * (r.beta * r.beta)) + r.lb * r.lb / 2.0f;
        if (r.f) acc[1] = (double)(A.sf * nll);
        else acc[2] = (double)(A.sf_static * u);
    }
    acc[0] = (double)(mse * r.factor);
    r.A = lz_clampf(w_s, LZO_A_LO, LZO_A_HI);
    const float omA = 1.0f - r.A;
    acc[3] = (double)(-r.A * lzo_log2(r.A) - omA * lzo_log2(omA));
    if (A.flags & LZ_OBJ_AMB_AUD) {
        if (!r.f) acc[4] = (double)A.aud[i];
        if ((A.flags & LZ_OBJ_AMB_EYE) && r.f) acc[5] = (double)(A.eye[i] / A.max_steps * A.aud[i]);
    }
}

__global__ void __launch_bounds__(LZO_THREADS) lz_k_obj_head_forward(LzObjHead A, float* __restrict__ pred, float* __restrict__ loss,
                                                                    float* __restrict__ aux, void* ws) {
    __shared__ double red[6 * LZO_THREADS + 1];
    const uint32_t stride = gridDim.x * LZO_THREADS;
    double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (uint32_t i = blockIdx.x * LZO_THREADS + threadIdx.x; i < A.N; i += stride) {
        LzObjRay r;
        float P[3];
        double a[6];
        lzo_ray(A, i, r, P, a);
#pragma unroll
        for (int c = 0; c < 3; ++c) pred[(size_t)i * 3 + c] = P[c];
#pragma unroll
        for (int k = 0; k < 6; ++k) acc[k] += a[k];
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) red[k * LZO_THREADS + threadIdx.x] = acc[k];
    lzo_tree_sum<6>(red);
    double* part = lzo_partials(ws);
    if (threadIdx.x == 0)
        for (int k = 0; k < 6; ++k) part[(size_t)blockIdx.x * LZO_SLOTS + k] = red[k * LZO_THREADS];
    if (!lzo_arrive_last(lzo_ticket(ws, LZO_T_HEAD), &red[6 * LZO_THREADS])) return;
    lzo_combine<6>(part, red);
    if (threadIdx.x == 0) {
        const double n = (double)A.N;
        const double t[6] = {red[0] / n, red[LZO_THREADS] / n, red[2 * LZO_THREADS] / n, 1e-4 * red[3 * LZO_THREADS] / n,
                             (double)A.lam * red[4 * LZO_THREADS] / n, (double)A.lam * red[5 * LZO_THREADS] / n};
        double L = 0.0;
        for (int k = 0; k < 6; ++k) {
            aux[k] = (float)t[k];
            L += t[k];
        }
        loss[0] = (float)L;
    }
}

struct LzObjHeadGrads {
    float* image;  float* ws;  float* unc;  float* aud;  float* eye;
};

__global__ void __launch_bounds__(LZO_THREADS) lz_k_obj_head_backward(LzObjHead A, const float* __restrict__ grad, LzObjHeadGrads G) {
    const uint32_t i = blockIdx.x * LZO_THREADS + threadIdx.x;
    if (i >= A.N) return;
    LzObjRay r;
    float P[3];
    double a[6];
    lzo_ray(A, i, r, P, a);
    const float gN = grad[0] / (float)A.N;                      // d mean / d l_i; the upstream gradient enters by multiplication only
    const float gl = gN * r.factor;
    float g_ws = 0.0f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float gP = gl * (2.0f * r.d[c] / 3.0f);
        const float gv = (r.v[c] >= 0.0f && r.v[c] <= 1.0f) ? gP : 0.0f;    // clamp(0, 1): passes where 0 <= v <= 1
        G.image[(size_t)i * 3 + c] = gv;
        g_ws -= gv * r.b[c];
    }
    const float ws = A.ws[i];
    if (ws >= LZO_A_LO && ws <= LZO_A_HI)
        g_ws += gN * 1e-4f * (lzo_log2(1.0f - r.A) - lzo_log2(r.A));           // d/dA of the binary entropy in bits
    G.ws[i] = g_ws;
    if (G.unc) {
        float gu = 0.0f;
        if (A.flags & LZ_OBJ_UNC)
            gu = r.f ? gN * (A.sf * (r.lb / r.beta - r.nrm / (r.beta * r.beta * r.beta))) : gN * A.sf_static;
        G.unc[i] = gu;
    }
    if (G.aud) G.aud[i] = ((A.flags & LZ_OBJ_AMB_AUD) && !r.f) ? gN * A.lam : 0.0f;
    if (G.eye) G.eye[i] = ((A.flags & LZ_OBJ_AMB_EYE) && r.f) ? gN * A.lam * (A.aud[i] / A.max_steps) : 0.0f;
}

static int lzo_head_args(LzObjHead& A, const float* image_raw, const float* weights_sum, const float* bg, uint32_t bg_mode, float bg_scalar,
                         const float* target, const uint8_t* face_mask, const float* unc, const float* amb_aud, const float* amb_eye, uint32_t N,
                         uint32_t flags, float step_factor, float lambda_amb, float max_steps, const char* who) {
    LZ_REQUIRE(image_raw && weights_sum && target && face_mask, LZ_ERR_BAD_ARGUMENT, "%s: null tensor", who);
    LZ_REQUIRE(bg_mode <= 3 && (bg_mode == 0 || bg), LZ_ERR_BAD_ARGUMENT, "%s: bg_mode %u (0 scalar, 1 [1], 2 [3], 3 [N,3]) or null bg", who, bg_mode);
    LZ_REQUIRE((flags & ~7u) == 0 && (!(flags & LZ_OBJ_AMB_EYE) || (flags & LZ_OBJ_AMB_AUD)), LZ_ERR_BAD_ARGUMENT,
               "%s: flags 0x%x (amb_eye needs amb_aud)", who, flags);
    LZ_REQUIRE(!(flags & LZ_OBJ_UNC) || unc, LZ_ERR_BAD_ARGUMENT, "%s: null uncertainty", who);
    LZ_REQUIRE(!(flags & LZ_OBJ_AMB_AUD) || amb_aud, LZ_ERR_BAD_ARGUMENT, "%s: null amb_aud", who);
    LZ_REQUIRE(!(flags & LZ_OBJ_AMB_EYE) || amb_eye, LZ_ERR_BAD_ARGUMENT, "%s: null amb_eye", who);
    A = LzObjHead{image_raw, weights_sum, bg, target, face_mask, unc, amb_aud, amb_eye, nullptr, N, bg_mode, flags, bg_scalar, step_factor,
                  (float)(1.0 - (double)step_factor), (float)(1e-3 * (double)step_factor), (float)((double)step_factor * (double)lambda_amb), max_steps};
    return LZ_OK;
}

extern "C" int lz_objective_head_forward(const float* image_raw, const float* weights_sum, const float* bg, uint32_t bg_mode, float bg_scalar,
                                         const float* target, const uint8_t* face_mask, const float* unc, const float* amb_aud, const float* amb_eye,
                                         uint32_t N, uint32_t flags, float step_factor, float lambda_amb, float max_steps, float* pred, float* loss,
                                         float* aux, void* workspace, lz_stream_t stream) {
    if (N == 0) return LZ_OK;
    LzObjHead A;
    const int rc = lzo_head_args(A, image_raw, weights_sum, bg, bg_mode, bg_scalar, target, face_mask, unc, amb_aud, amb_eye, N, flags, step_factor,
                                 lambda_amb, max_steps, "objective_head_forward");
    if (rc != LZ_OK) return rc;
    LZ_REQUIRE(pred && loss && aux && workspace, LZ_ERR_BAD_ARGUMENT, "objective_head_forward: null pred / loss / aux / workspace");
    A.stats = aux + 6;
    const uint32_t G = lzo_groups(N);
    if (flags & LZ_OBJ_UNC) {
        hipLaunchKernelGGL(lz_k_obj_softmax_stats, dim3(G), dim3(LZO_THREADS), 0, lz_st(stream), unc, N, aux + 6, workspace);
        LZ_CHECK_LAUNCH("objective_softmax_stats");
    }
    hipLaunchKernelGGL(lz_k_obj_head_forward, dim3(G), dim3(LZO_THREADS), 0, lz_st(stream), A, pred, loss, aux, workspace);
    LZ_CHECK_LAUNCH("objective_head_forward");
    return LZ_OK;
}

extern "C" int lz_objective_head_backward(const float* grad_loss, const float* image_raw, const float* weights_sum, const float* bg, uint32_t bg_mode,
                                          float bg_scalar, const float* target, const uint8_t* face_mask, const float* unc, const float* amb_aud,
                                          const float* amb_eye, const float* aux, uint32_t N, uint32_t flags, float step_factor, float lambda_amb,
                                          float max_steps, float* g_image_raw, float* g_weights_sum, float* g_unc, float* g_amb_aud, float* g_amb_eye,
                                          lz_stream_t stream) {
    if (N == 0) return LZ_OK;
    LzObjHead A;
    const int rc = lzo_head_args(A, image_raw, weights_sum, bg, bg_mode, bg_scalar, target, face_mask, unc, amb_aud, amb_eye, N, flags, step_factor,
                                 lambda_amb, max_steps, "objective_head_backward");
    if (rc != LZ_OK) return rc;
    LZ_REQUIRE(grad_loss && aux && g_image_raw && g_weights_sum, LZ_ERR_BAD_ARGUMENT, "objective_head_backward: null grad_loss / aux / gradient");
    LZ_REQUIRE(!(flags & LZ_OBJ_AMB_EYE) || g_amb_eye, LZ_ERR_BAD_ARGUMENT, "objective_head_backward: null g_amb_eye");
    A.stats = aux + 6;
    hipLaunchKernelGGL(lz_k_obj_head_backward, dim3(lz_div_up(N, LZO_THREADS)), dim3(LZO_THREADS), 0, lz_st(stream), A, grad_loss,
                       LzObjHeadGrads{g_image_raw, g_weights_sum, g_unc, g_amb_aud, g_amb_eye});
    LZ_CHECK_LAUNCH("objective_head_backward");
    return LZ_OK;
}

// pred's own gradient (a loss term that reads pred, the LPIPS terms): back through the clamp and the blend, in lzo_ray's arithmetic
__global__ void __launch_bounds__(LZO_THREADS) lz_k_obj_pred_backward(const float* __restrict__ g_pred, const float* __restrict__ image,
                                                                     const float* __restrict__ ws, const float* __restrict__ bg, uint32_t bg_mode,
                                                                     float bg_scalar, uint32_t N, float* __restrict__ g_image, float* __restrict__ g_ws) {
    const uint32_t i = blockIdx.x * LZO_THREADS + threadIdx.x;
    if (i >= N) return;
    const float one_m_ws = 1.0f - ws[i];
    float acc = 0.0f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float b = bg_mode == 0 ? bg_scalar : (bg_mode == 1 ? bg[0] : (bg_mode == 2 ? bg[c] : bg[(size_t)i * 3 + c]));
        const float v = image[(size_t)i * 3 + c] + one_m_ws * b;
        const float gv = (v >= 0.0f && v <= 1.0f) ? g_pred[(size_t)i * 3 + c] : 0.0f;    // clamp(0, 1): passes where 0 <= v <= 1
        g_image[(size_t)i * 3 + c] = gv;
        acc -= gv * b;
    }
    g_ws[i] = acc;
}

extern "C" int lz_objective_pred_backward(const float* g_pred, const float* image_raw, const float* weights_sum, const float* bg, uint32_t bg_mode,
                                          float bg_scalar, uint32_t N, float* g_image_raw, float* g_weights_sum, lz_stream_t stream) {
    if (N == 0) return LZ_OK;
    LZ_REQUIRE(g_pred && image_raw && weights_sum && g_image_raw && g_weights_sum, LZ_ERR_BAD_ARGUMENT, "objective_pred_backward: null tensor");
    LZ_REQUIRE(bg_mode <= 3 && (bg_mode == 0 || bg), LZ_ERR_BAD_ARGUMENT, "objective_pred_backward: bg_mode %u (0 scalar, 1 [1], 2 [3], 3 [N,3]) or null bg",
               bg_mode);
    hipLaunchKernelGGL(lz_k_obj_pred_backward, dim3(lz_div_up(N, LZO_THREADS)), dim3(LZO_THREADS), 0, lz_st(stream), g_pred, image_raw, weights_sum, bg,
                       bg_mode, bg_scalar, N, g_image_raw, g_weights_sum);
    LZ_CHECK_LAUNCH("objective_pred_backward");
    return LZ_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// torso (TrainerUtil.py:238-244): mean_i mean_c (C - T)^2 + mean_j (1 - anchor[j, 3])^2
// ---------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(LZO_THREADS) lz_k_obj_torso_forward(const float* __restrict__ color, const float* __restrict__ target,
                                                                     const float* __restrict__ anchors, uint32_t J, uint32_t N, float* __restrict__ loss,
                                                                     float* __restrict__ aux, void* ws) {
    __shared__ double red[LZO_THREADS + 1];
    const uint32_t stride = gridDim.x * LZO_THREADS;
    double acc = 0.0;
    for (uint32_t i = blockIdx.x * LZO_THREADS + threadIdx.x; i < N; i += stride) {
        const float d0 = color[(size_t)i * 3] - target[(size_t)i * 3], d1 = color[(size_t)i * 3 + 1] - target[(size_t)i * 3 + 1],
                    d2 = color[(size_t)i * 3 + 2] - target[(size_t)i * 3 + 2];
        acc += (double)((d0 * d0 + d1 * d1 + d2 * d2) / 3.0f);
    }
    red[threadIdx.x] = acc;
    lzo_tree_sum<1>(red);
    double* part = lzo_partials(ws);
    if (threadIdx.x == 0) part[(size_t)blockIdx.x * LZO_SLOTS] = red[0];
    if (!lzo_arrive_last(lzo_ticket(ws, LZO_T_TORSO), &red[LZO_THREADS])) return;
    lzo_combine<1>(part, red);
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (uint32_t j = 0; j < J; ++j) {
            const float e = 1.0f - anchors[(size_t)j * 4 + 3];
            s += (double)(e * e);
        }
        const double t0 = red[0] / (double)N, t1 = J ? s / (double)J : 0.0;
        aux[0] = (float)t0;
        aux[1] = (float)t1;
        loss[0] = (float)(t0 + t1);
    }
}

__global__ void __launch_bounds__(LZO_THREADS) lz_k_obj_torso_backward(const float* __restrict__ grad, const float* __restrict__ color,
                                                                      const float* __restrict__ target, const float* __restrict__ anchors, uint32_t J,
                                                                      uint32_t N, float* __restrict__ g_color, float* __restrict__ g_anchors) {
    const uint32_t t = blockIdx.x * LZO_THREADS + threadIdx.x;
    if (t < N) {
        const float gN = grad[0] / (float)N;
#pragma unroll
        for (int c = 0; c < 3; ++c) g_color[(size_t)t * 3 + c] = gN * (2.0f * (color[(size_t)t * 3 + c] - target[(size_t)t * 3 + c]) / 3.0f);
    }
    if (g_anchors && t < J * 4)
        g_anchors[t] = (t & 3) == 3 ? (grad[0] / (float)J) * (-2.0f * (1.0f - anchors[t])) : 0.0f;
}

extern "C" int lz_objective_torso_forward(const float* torso_color, const float* target, const float* anchor_points, uint32_t J, uint32_t N,
                                          float* loss, float* aux, void* workspace, lz_stream_t stream) {
    if (N == 0) return LZ_OK;
    LZ_REQUIRE(torso_color && target && loss && aux && workspace && (J == 0 || anchor_points), LZ_ERR_BAD_ARGUMENT, "objective_torso_forward: null tensor");
    hipLaunchKernelGGL(lz_k_obj_torso_forward, dim3(lzo_groups(N)), dim3(LZO_THREADS), 0, lz_st(stream), torso_color, target, anchor_points, J, N,
                       loss, aux, workspace);
    LZ_CHECK_LAUNCH("objective_torso_forward");
    return LZ_OK;
}

extern "C" int lz_objective_torso_backward(const float* grad_loss, const float* torso_color, const float* target, const float* anchor_points, uint32_t J,
                                           uint32_t N, float* g_torso_color, float* g_anchor_points, lz_stream_t stream) {
    if (N == 0) return LZ_OK;
    LZ_REQUIRE(grad_loss && torso_color && target && g_torso_color && (J == 0 || anchor_points), LZ_ERR_BAD_ARGUMENT,
               "objective_torso_backward: null tensor");
    const uint64_t n = N > (uint64_t)J * 4 ? N : (uint64_t)J * 4;
    hipLaunchKernelGGL(lz_k_obj_torso_backward, dim3(lz_div_up(n, LZO_THREADS)), dim3(LZO_THREADS), 0, lz_st(stream), grad_loss, torso_color, target,
                       anchor_points, J, N, g_torso_color, g_anchor_points);
    LZ_CHECK_LAUNCH("objective_torso_backward");
    return LZ_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// jitter regulariser (TrainerUtil.py:346-365): scale * sum over the enabled k of mean_m (raw_k - reg_k)^2, scale = step_factor * 1e-5
// ---------------------------------------------------------------------------------------------------------------------------------
struct LzObjJitter {
    const float* raw[3];
    const float* reg[3];
    uint32_t M, flags;
    float scale;
};

__global__ void __launch_bounds__(LZO_THREADS) lz_k_obj_jitter_forward(LzObjJitter J, float* __restrict__ loss, float* __restrict__ aux, void* ws) {
    __shared__ double red[3 * LZO_THREADS + 1];
    const uint32_t stride = gridDim.x * LZO_THREADS;
    double acc[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (!(J.flags & (1u << k))) continue;                  // uniform
        const float* __restrict__ a = J.raw[k];
        const float* __restrict__ b = J.reg[k];
        for (uint32_t m = blockIdx.x * LZO_THREADS + threadIdx.x; m < J.M; m += stride) {
            const float d = a[m] - b[m];
            acc[k] += (double)(d * d);
        }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) red[k * LZO_THREADS + threadIdx.x] = acc[k];
    lzo_tree_sum<3>(red);
    double* part = lzo_partials(ws);
    if (threadIdx.x == 0)
        for (int k = 0; k < 3; ++k) part[(size_t)blockIdx.x * LZO_SLOTS + k] = red[k * LZO_THREADS];
    if (!lzo_arrive_last(lzo_ticket(ws, LZO_T_JITTER), &red[3 * LZO_THREADS])) return;
    lzo_combine<3>(part, red);
    if (threadIdx.x == 0) {
        double L = 0.0;
        for (int k = 0; k < 3; ++k) {
            const double t = (double)J.scale * (red[k * LZO_THREADS] / (double)J.M);
            aux[k] = (float)t;
            L += t;
        }
        loss[0] = (float)L;
    }
}

__global__ void __launch_bounds__(LZO_THREADS) lz_k_obj_jitter_backward(LzObjJitter J, const float* __restrict__ grad, float* g0, float* g1, float* g2) {
    const uint32_t m = blockIdx.x * LZO_THREADS + threadIdx.x;
    if (m >= J.M) return;
    const float gs = grad[0] / (float)J.M * J.scale;
    float* g[3] = {g0, g1, g2};
#pragma unroll
    for (int k = 0; k < 3; ++k)
        if (J.flags & (1u << k)) g[k][m] = gs * (-2.0f * (J.raw[k][m] - J.reg[k][m]));   // d/d reg of (raw - reg)^2: reg carries the gradient
}

static int lzo_jitter_args(LzObjJitter& J, const float* raw_unc, const float* raw_aud, const float* raw_eye, const float* reg_unc, const float* reg_aud,
                           const float* reg_eye, uint32_t M, uint32_t flags, float scale, const char* who) {
    LZ_REQUIRE((flags & ~7u) == 0, LZ_ERR_BAD_ARGUMENT, "%s: flags 0x%x", who, flags);
    J = LzObjJitter{{raw_unc, raw_aud, raw_eye}, {reg_unc, reg_aud, reg_eye}, M, flags, scale};
    for (int k = 0; k < 3; ++k) LZ_REQUIRE(!(flags & (1u << k)) || (J.raw[k] && J.reg[k]), LZ_ERR_BAD_ARGUMENT, "%s: null tensor %d", who, k);
    return LZ_OK;
}

extern "C" int lz_objective_jitter_forward(const float* raw_unc, const float* raw_aud, const float* raw_eye, const float* reg_unc, const float* reg_aud,
                                           const float* reg_eye, uint32_t M, uint32_t flags, float scale, float* loss, float* aux, void* workspace,
                                           lz_stream_t stream) {
    if (M == 0) return LZ_OK;
    LzObjJitter J;
    const int rc = lzo_jitter_args(J, raw_unc, raw_aud, raw_eye, reg_unc, reg_aud, reg_eye, M, flags, scale, "objective_jitter_forward");
    if (rc != LZ_OK) return rc;
    LZ_REQUIRE(loss && aux && workspace, LZ_ERR_BAD_ARGUMENT, "objective_jitter_forward: null loss / aux / workspace");
    hipLaunchKernelGGL(lz_k_obj_jitter_forward, dim3(lzo_groups(M)), dim3(LZO_THREADS), 0, lz_st(stream), J, loss, aux, workspace);
    LZ_CHECK_LAUNCH("objective_jitter_forward");
    return LZ_OK;
}

extern "C" int lz_objective_jitter_backward(const float* grad_loss, const float* raw_unc, const float* raw_aud, const float* raw_eye, const float* reg_unc,
                                            const float* reg_aud, const float* reg_eye, uint32_t M, uint32_t flags, float scale, float* g_reg_unc,
                                            float* g_reg_aud, float* g_reg_eye, lz_stream_t stream) {
    if (M == 0) return LZ_OK;
    LzObjJitter J;
    const int rc = lzo_jitter_args(J, raw_unc, raw_aud, raw_eye, reg_unc, reg_aud, reg_eye, M, flags, scale, "objective_jitter_backward");
    if (rc != LZ_OK) return rc;
    float* g[3] = {g_reg_unc, g_reg_aud, g_reg_eye};
    LZ_REQUIRE(grad_loss, LZ_ERR_BAD_ARGUMENT, "objective_jitter_backward: null grad_loss");
    for (int k = 0; k < 3; ++k) LZ_REQUIRE(!(flags & (1u << k)) || g[k], LZ_ERR_BAD_ARGUMENT, "objective_jitter_backward: null gradient %d", k);
    hipLaunchKernelGGL(lz_k_obj_jitter_backward, dim3(lz_div_up(M, LZO_THREADS)), dim3(LZO_THREADS), 0, lz_st(stream), J, grad_loss, g_reg_unc,
                       g_reg_aud, g_reg_eye);
    LZ_CHECK_LAUNCH("objective_jitter_backward");
    return LZ_OK;
}
