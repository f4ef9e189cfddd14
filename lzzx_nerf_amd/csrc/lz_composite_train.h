// lz_composite_train.h -- the rules the training march and the training compositing kernels of lz_raymarch.hip share, each written once: the
// rays[] entry and its drop rule, the per-sample forward and backward arithmetic of compositing, the zero rows, the row walk of the
// step-major layout, the scan entry -> rays[] entry of the march's write pass and the start of a ray's march.  Device code only; the
// kernels stay in lz_raymarch.hip.  Not every kernel takes every rule from here: the step-major kernels keep the pieces whose shared form
// cost them measured time ("Shared rules of the training march and compositing" lists which, with the readings).
#ifndef LZ_COMPOSITE_TRAIN_H
#define LZ_COMPOSITE_TRAIN_H
#include "lz_march.h"

// ------------------------------------------------------------------------------------------------
// rays[] = (ray id, first row, samples) per ray, and the drop rule
// ------------------------------------------------------------------------------------------------
// a ray whose rows do not fit the M rows of the sample buffers is dropped (raymarching.cu:457, 1905); the dropped rays are a suffix of rays[]
__device__ __forceinline__ bool lz_train_ray_dropped(uint32_t offset, uint32_t count, uint32_t M) { return offset + count > M; }

struct LzTrainRay {
    uint32_t index, offset, count;    // rays[n]; zeros for n >= N
    bool dropped;
    __device__ __forceinline__ uint32_t ns() const { return dropped ? 0u : count; }     // the samples to walk: none of a dropped ray
};
__device__ __forceinline__ LzTrainRay lz_train_ray(const int* __restrict__ rays, uint32_t n, uint32_t N, uint32_t M) {
    LzTrainRay r = {0u, 0u, 0u, false};
    if (n < N) {
        r.index = (uint32_t)rays[(size_t)n * 3];
        r.offset = (uint32_t)rays[(size_t)n * 3 + 1];
        r.count = (uint32_t)rays[(size_t)n * 3 + 2];
        r.dropped = lz_train_ray_dropped(r.offset, r.count, M);
    }
    return r;
}

// ------------------------------------------------------------------------------------------------
// zero rows
// ------------------------------------------------------------------------------------------------
// Rows nobody writes read ZERO, as the reference's wrappers left them (torch.zeros, raymarching.py:246-248, 649-653) -- written by the kernels,
// so that the caller need not fill the buffers first (round 5: 3 + 5 of the 19 fill launches of a training step, ~360 MB)
__device__ __forceinline__ void lz_zero_sample_row(uint32_t r, float* __restrict__ xyzs, float* __restrict__ dirs, float* __restrict__ deltas) {
#pragma unroll
    for (int k = 0; k < 3; k++) { xyzs[(size_t)r * 3 + k] = 0.0f; dirs[(size_t)r * 3 + k] = 0.0f; }
    deltas[(size_t)r * 2] = 0.0f; deltas[(size_t)r * 2 + 1] = 0.0f;
}
template <int NAMB, bool UNC>
__device__ __forceinline__ void lz_zero_grad_row(size_t i, float* __restrict__ grad_sigmas, float* __restrict__ grad_rgbs,
                                                 float* __restrict__ grad_amb0, float* __restrict__ grad_amb1, float* __restrict__ grad_unc) {
    grad_sigmas[i] = 0.0f;
    grad_rgbs[i * 3] = 0.0f; grad_rgbs[i * 3 + 1] = 0.0f; grad_rgbs[i * 3 + 2] = 0.0f;
    if (NAMB > 0) grad_amb0[i] = 0.0f;
    if (NAMB > 1) grad_amb1[i] = 0.0f;
    if (UNC) grad_unc[i] = 0.0f;
}
// the sample rows in front of the step's first row (base[0], a non-zero counter) and behind its last (total[0]), spread over the
// launch (`thread` = the global thread index)
__device__ __forceinline__ void lz_zero_sample_margins(uint32_t thread, const int* __restrict__ base, const int* __restrict__ total, uint32_t M,
                                                       float* __restrict__ xyzs, float* __restrict__ dirs, float* __restrict__ deltas) {
    const uint32_t first = (uint32_t)base[0] < M ? (uint32_t)base[0] : M, last = (uint32_t)total[0] < M ? (uint32_t)total[0] : M;
    const uint32_t nthreads = gridDim.x * blockDim.x, span = first + (M - last);
    for (uint32_t q = thread; q < span; q += nthreads) lz_zero_sample_row(q < first ? q : last + (q - first), xyzs, dirs, deltas);
}

// ------------------------------------------------------------------------------------------------
// the march's write pass: scan entry -> rays[] entry
// ------------------------------------------------------------------------------------------------
// Entry i of the exclusive scan (ray n) becomes rays[base[1] + i] = (n, first row, samples); a ray's own count is the difference to its
// successor's offset.  Returns the rows the caller is to write from `point_index` on: 0 when the ray marched nothing or is dropped for lack
// of room.  The first dropped ray clears what is left of the buffers (every later one clears a part of that again).
__device__ __forceinline__ uint32_t lz_train_ray_emit(uint32_t i, uint32_t n, uint32_t N, uint32_t M, const int* __restrict__ offsets,
                                                      const int* __restrict__ base, const int* __restrict__ total, int* __restrict__ rays,
                                                      float* __restrict__ xyzs, float* __restrict__ dirs, float* __restrict__ deltas,
                                                      uint32_t& point_index) {
    const uint32_t off = (uint32_t)offsets[i];
    const uint32_t nxt = (i + 1 < N) ? (uint32_t)offsets[i + 1] : (uint32_t)(total[0] - base[0]);
    const uint32_t num_steps = nxt - off;
    point_index = (uint32_t)base[0] + off;
    const uint32_t ray_index = (uint32_t)base[1] + i;
    rays[(size_t)ray_index * 3] = (int)n;
    rays[(size_t)ray_index * 3 + 1] = (int)point_index;
    rays[(size_t)ray_index * 3 + 2] = (int)num_steps;
    if (!lz_train_ray_dropped(point_index, num_steps, M)) return num_steps;
    if (num_steps != 0)
        for (uint32_t r = point_index; r < M; r++) lz_zero_sample_row(r, xyzs, dirs, deltas);
    return 0u;
}

// a ray's march before its first probe: LzMarch::init, the workgroup's Morton table (`mlut`, staged by the caller) and the perturbed start
// t = near + clamp(near * dt_gamma) * noise (raymarching.cu:407-411); returns t, and the ray's far end in `far`
__device__ __forceinline__ float lz_march_train_start(LzMarch& m, const float* __restrict__ rays_o, const float* __restrict__ rays_d, uint32_t n,
                                                      float bound, float dt_gamma, uint32_t max_steps, uint32_t C, uint32_t H,
                                                      const uint8_t* __restrict__ grid, const uint32_t* mlut, const float* __restrict__ nears,
                                                      const float* __restrict__ fars, const float* __restrict__ noises, float& far) {
    m.init(rays_o + (size_t)n * 3, rays_d + (size_t)n * 3, bound, dt_gamma, max_steps, C, H, grid);
    if (H <= LZ_MORTON_LUT) m.morton_lut = mlut;
    far = fars[n];
    const float t = nears[n];
    return lz_fmaf(lz_clampf(t * dt_gamma, m.dt_min, m.dt_max), noises[n], t);
}

// ------------------------------------------------------------------------------------------------
// the row walk of the step-major layout (see "STEP-MAJOR sample layout" in lz_raymarch.hip)
// ------------------------------------------------------------------------------------------------
#ifndef LZ_TRAIN_GROUP
#define LZ_TRAIN_GROUP 64       /* rays per group of the step-major layout: 16, 32 or 64 (lz_train_group_size()) */
#endif
static_assert(LZ_TRAIN_GROUP == 16 || LZ_TRAIN_GROUP == 32 || LZ_TRAIN_GROUP == 64, "group = 16, 32 or 64 lanes of a wave");
// lanes of this lane's group
__device__ __forceinline__ unsigned long long lz_tg_mask(uint32_t lane) {
    return LZ_TRAIN_GROUP == 64 ? ~0ull : (((1ull << LZ_TRAIN_GROUP) - 1ull) << (lane & ~(uint32_t)(LZ_TRAIN_GROUP - 1)));
}
// the group's first row: rays[] offset of the group's first lane (that lane always holds a ray when any lane of the group does)
__device__ __forceinline__ uint32_t lz_tg_base(uint32_t offset, uint32_t lane) {
    if (LZ_TRAIN_GROUP == 64) return (uint32_t)__builtin_amdgcn_readfirstlane((int)offset);
    return (uint32_t)__shfl((int)offset, (int)(lane & ~(uint32_t)(LZ_TRAIN_GROUP - 1)), 64);
}

// Lane j = ray j of the wave's rays[] entries, `offset` its rays[] offset.  The WHOLE wave calls step(has) once per step k = 0, 1, ... with
// has = (k < the lane's sample count), then row() where it wants the lane's row at that step -- gb + sum_i min(c_i, k) + #{i < j : c_i > k}
// over its group, meaningful where `has` -- and next() to move on.  The row depends on `has` alone, so a lane that stopped consuming its
// samples still learns its rows (the backward zeroes them).
struct LzGroupWalk {
    uint32_t gb, S;
    unsigned long long gm, below, alive;     // lanes of this lane's group / those of them below this lane / those with a sample at this step
    __device__ __forceinline__ void start(uint32_t offset, uint32_t lane) {
        gb = lz_tg_base(offset, lane);
        gm = lz_tg_mask(lane); below = ((1ull << lane) - 1ull) & gm;
        S = 0;
    }
    __device__ __forceinline__ unsigned long long step(bool has) { const unsigned long long all = __ballot(has); alive = all & gm; return all; }
    __device__ __forceinline__ size_t row() const { return (size_t)gb + S + (uint32_t)__popcll(alive & below); }
    __device__ __forceinline__ void next() { S += (uint32_t)__popcll(alive); }
};

// ------------------------------------------------------------------------------------------------
// the per-sample arithmetic of training compositing (raymarching.cu:1877-2133), same operations in the same order in both layouts
// ------------------------------------------------------------------------------------------------
// NOT the step of the inference kernel (lz_k_composite_rays): that one forms T = 1 - weight_sum every step, not the running product.
template <int NAMB, bool AMBW, bool UNC>
struct LzCompositeFwd {
    float T = 1.0f, r = 0, g = 0, b = 0, ws = 0, d = 0, a0 = 0, a1 = 0, u = 0;
    // values of unused channels are ignored
    __device__ __forceinline__ void step(float sigma, float dt, float t, float c0, float c1, float c2, float amb0, float amb1, float unc) {
        const float alpha = 1.0f - lz_expf(-sigma * dt);
        const float weight = alpha * T;
        r = lz_fmaf(weight, c0, r);
        g = lz_fmaf(weight, c1, g);
        b = lz_fmaf(weight, c2, b);
        d = lz_fmaf(weight, t, d);
        ws += weight;
        if (NAMB > 0) a0 = AMBW ? lz_fmaf(weight, amb0, a0) : a0 + amb0;
        if (NAMB > 1) a1 = AMBW ? lz_fmaf(weight, amb1, a1) : a1 + amb1;
        if (UNC) u = lz_fmaf(weight, unc, u);
        T *= 1.0f - alpha;
    }
    __device__ __forceinline__ void store(uint32_t index, float* __restrict__ weights_sum, float* __restrict__ amb0_sum, float* __restrict__ amb1_sum,
                                          float* __restrict__ unc_sum, float* __restrict__ depth, float* __restrict__ image) const {
        weights_sum[index] = ws;
        if (NAMB > 0) amb0_sum[index] = a0;
        if (NAMB > 1) amb1_sum[index] = a1;
        if (UNC) unc_sum[index] = u;
        depth[index] = d;
        image[(size_t)index * 3] = r; image[(size_t)index * 3 + 1] = g; image[(size_t)index * 3 + 2] = b;
    }
};

// The backward re-runs the forward sums next to the ray's finals.  Of a sample's gradients step() returns d sigma and the weight: the gradients
// of the colour, ambient and uncertainty inputs are the incoming gradients (gi0 .. gu below) times the weight, or as they are, and the caller
// stores them its own way.  `av` is read by the weighted-ambient variant only, `uv` with UNC.
template <int NAMB, bool AMBW, bool UNC>
struct LzCompositeBwd {
    float gi0 = 0, gi1 = 0, gi2 = 0, gws = 0, ga0 = 0, ga1 = 0, gu = 0;                                        // incoming gradients
    float r_final = 0, g_final = 0, b_final = 0, ws_final = 0, amb_final = 0, unc_final = 0;                   // the forward's results
    float T = 1.0f, r = 0, g = 0, b = 0, ws = 0, amb = 0, u = 0;
    __device__ __forceinline__ void load(uint32_t index, const float* __restrict__ grad_weights_sum, const float* __restrict__ grad_amb0_sum,
                                         const float* __restrict__ grad_amb1_sum, const float* __restrict__ grad_unc_sum,
                                         const float* __restrict__ grad_image, const float* __restrict__ weights_sum,
                                         const float* __restrict__ amb0_sum, const float* __restrict__ unc_sum, const float* __restrict__ image) {
        gi0 = grad_image[(size_t)index * 3]; gi1 = grad_image[(size_t)index * 3 + 1]; gi2 = grad_image[(size_t)index * 3 + 2];
        gws = grad_weights_sum[index];
        if (NAMB > 0) ga0 = grad_amb0_sum[index];
        if (NAMB > 1) ga1 = grad_amb1_sum[index];
        if (UNC) gu = grad_unc_sum[index];
        r_final = image[(size_t)index * 3]; g_final = image[(size_t)index * 3 + 1]; b_final = image[(size_t)index * 3 + 2];
        ws_final = weights_sum[index];
        if (NAMB > 0 && AMBW) amb_final = amb0_sum[index];
        if (UNC) unc_final = unc_sum[index];
    }
    struct Grad { float sigma, weight; };
    __device__ __forceinline__ Grad step(float sigma, float dt, float c0, float c1, float c2, float av, float uv) {
        const float alpha = 1.0f - lz_expf(-sigma * dt);
        const float weight = alpha * T;
        r = lz_fmaf(weight, c0, r);
        g = lz_fmaf(weight, c1, g);
        b = lz_fmaf(weight, c2, b);
        if (NAMB > 0 && AMBW) amb = lz_fmaf(weight, av, amb);
        if (UNC) u = lz_fmaf(weight, uv, u);
        ws += weight;
        T *= 1.0f - alpha;
        float s = gi0 * lz_fmaf(T, c0, -(r_final - r));
        s = lz_fmaf(gi1, lz_fmaf(T, c1, -(g_final - g)), s);
        s = lz_fmaf(gi2, lz_fmaf(T, c2, -(b_final - b)), s);
        if (NAMB > 0 && AMBW) s = lz_fmaf(ga0, lz_fmaf(T, av, -(amb_final - amb)), s);
        if (UNC) s = lz_fmaf(gu, lz_fmaf(T, uv, -(unc_final - u)), s);
        s = lz_fmaf(gws, 1 - ws_final, s);
        return {dt * s, weight};
    }
};

#endif
