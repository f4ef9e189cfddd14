// lz_frame_common.h -- what the persistent frame kernels share (lz_frame.hip: the triplane head; lz_ngp_frame.hip: the hash-grid NeRF):
// the frame's kernel-argument record and state words, the per-ray output side (a pixel, a ray leaving its slot) and the host-side
// launches around the persistent kernel -- prepare / queue order, the cap histogram + schedule replay, the count fix-up -- which live
// in lz_frame.hip.  Library-internal: nothing here is part of the C ABI.
#ifndef LZ_FRAME_COMMON_H
#define LZ_FRAME_COMMON_H
#include "lz_march.h"

#define LZF_BINS 256
#define LZF_LUT 256          // Morton bit-spread table in LDS, for grids up to 256^3 (the reference hard-codes 128, renderer.py:94)
// device state words (LZ_FRAME_STATE_INTS int32, zeroed per frame by lz_frame_render).  Words 3, 5, 6 and 72 sit where the
// multi-launch loop keeps done / total_samples / iterations / rows (lz_loop_state, LZ_LOOP_STAT_ROWS), so a caller reads both alike.
#define LZF_Q_HEAD 0      // queue cursor
#define LZF_Q_SIZE 1      // rays in the queue (those with at least one sample)
#define LZF_DONE 3        // 1 (the frame is complete in stream order)
#define LZF_SAMPLES 5     // marched = composited samples
#define LZF_ITER 6        // 1: one persistent launch
#define LZF_ROWS 72       // sample rows handed to the head (16 per slice)
// cap_mode 1 (the reference's cap, see "the cap" below)
#define LZF_P_HEAD 8      // phase 2: queue cursor over the rays phase 1 parked at max_steps
#define LZF_P_SIZE 9      // rays parked by phase 1 that phase 2 continues (0 when C_eff == max_steps)
#define LZF_CEFF 10       // C_eff: samples a ray alive at the cap receives under the reference's schedule
#define LZF_SCHED_K 11    // iterations the reference's loop runs
#define LZF_TICKET 12     // workgroups of lz_k_frame_cap_hist that have flushed
#define LZF_CAP_MAX_STEPS 4096   // LDS histogram / schedule tables of the cap kernels
#define LZF_HIST 128      // [256] rays per key
#define LZF_CURSOR 384    // [256] scatter cursors

struct LzFrameK {
    const float* rays_o; const float* rays_d; const uint8_t* grid; const float* aabb;
    float* nears; float* fars; float* rays_t;
    int* order; int* state; uint8_t* keys;
    float* weights_sum; float* depth; float* image; float* amb0_sum; float* amb1_sum; float* unc_sum;
    float* out; const float* bg; uint8_t* out_rgb24; int* ray_counts;
    float bg_scalar, bound, dt_gamma, T_thresh, min_near;
    uint32_t N, max_steps, C, H;
    const float* noises;
    const float* occ;     // [6] or null: bounds of the occupied cells (lz_occupied_bounds); the march is confined to them
    float* t_end;         // [N] with occ: where a ray's march ends (far, clipped to occ); the persistent kernel reads it instead of fars
    // ---- the cap (cap_mode 1) ----
    int* ray_last;        // [N]: L of every ray = the last chunk boundary it can survive, min(box samples, tau - 1), max_steps = parked at the cap
    int* cap_ws;          // [0 .. max_steps] histogram of L (what ranks all-reduce), then the schedule tables (lz_k_frame_schedule)
    uint32_t cap_mode, phase2, N_total;
    LzMarchFrame mf;      // the march's frame-wide quotients (lz_march_frame on the host)
    float* c1sh;          // f32 heads: [N][LZ_C1_SH_FLOATS] per-ray SH partial of colour_net.0 (lz_k_frame_c1sh; library-internal, see lzf_c1sh_alloc)
};

// The per-ray OUTPUT side of LzFrameK (eleven pointers, the background, the cap's buffers) is touched once per ray, when it leaves its slot.
// Read as ordinary kernel arguments these fields are loop-invariant scalars, the compiler keeps all of them in scalar registers through every
// pass, and the f32 frame kernel -- short of scalar registers next to the head's -- spills them to vector lanes and restores them inside the
// pass loop (round 4 measured that: ten more live scalars = +0.9 % on the headline frame).  LzfOut reads a field from the kernel-argument
// segment AT THE POINT OF USE instead (a volatile scalar load: not hoisted), for the price of a few s_load per finished ray.
typedef const char __attribute__((address_space(4))) lz_kernarg_t;
struct LzfOut {
    lz_kernarg_t* f;      // where the kernel's LzFrameK argument sits in its kernel-argument segment
    template <typename T> __device__ __forceinline__ T get(size_t off) const {
        return *reinterpret_cast<const volatile T __attribute__((address_space(4)))*>(f + off);
    }
};
#define LZF_OUT(o, name) ((o).template get<decltype(LzFrameK::name)>(__builtin_offsetof(LzFrameK, name)))
// the hand-computed offset assumes that LzFrameK is laid out in the kernel-argument segment like any 8-byte-aligned trivially copyable struct
// argument, directly behind ARGS_BEFORE bytes of arguments rounded up to 8 (lz_k_frame_prep: first argument; lz_k_frame: behind HD::Args)
static_assert(alignof(LzFrameK) == 8 && __is_trivially_copyable(LzFrameK), "LZF_OUT reads LzFrameK from the kernel-argument segment at round8(ARGS_BEFORE)");
template <size_t ARGS_BEFORE>    // bytes of kernel arguments in front of the LzFrameK (0: it is the first)
__device__ __forceinline__ LzfOut lzf_out() {
    return LzfOut{(lz_kernarg_t*)__builtin_amdgcn_kernarg_segment_ptr() + ((ARGS_BEFORE + 7) & ~size_t(7))};
}

__device__ __forceinline__ void lzf_write_pixel(const LzfOut& O, int ray, float ws, float d, float r, float g, float b, float a0, float a1,
                                                float u, int cnt) {
    LZF_OUT(O, weights_sum)[ray] = ws;
    LZF_OUT(O, depth)[ray] = d;
    const float rgb[3] = {r, g, b};
    float* image = LZF_OUT(O, image);
    float* out = LZF_OUT(O, out);
    const float* bg = LZF_OUT(O, bg);
    uint8_t* out_rgb24 = LZF_OUT(O, out_rgb24);
    const float bg_scalar = LZF_OUT(O, bg_scalar);
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const size_t t = (size_t)ray * 3 + c;
        image[t] = rgb[c];
        const float bgv = bg ? bg[t] : bg_scalar;
        const float v = rgb[c] + (1.0f - ws) * bgv;              // renderer.py:559, two roundings like lz_k_final_blend
        const float cl = lz_fminf(lz_fmaxf(v, 0.0f), 1.0f);
        out[t] = cl;
        if (out_rgb24) out_rgb24[t] = (uint8_t)(cl * 255.0f);
    }
    LZF_OUT(O, amb0_sum)[ray] = a0;
    LZF_OUT(O, amb1_sum)[ray] = a1;
    LZF_OUT(O, unc_sum)[ray] = u;
    int* ray_counts = LZF_OUT(O, ray_counts);
    if (ray_counts) ray_counts[ray] = cnt;
}

// a ray leaves its slot.  kind: how it ended -- LZF_END_BOX no further sample in the box (`composited` = all it has), LZF_END_T the
// compositing cut it at its `composited`-th sample (T < T_thresh), LZF_END_CAP alive after `composited` = cap samples.  cap_mode 1
// records L for the schedule (phase 1), parks a capped ray's t for phase 2, and flags the count of a T-cut ray (negative, its t kept)
// for lz_k_frame_counts; `report` is the count written otherwise.
enum { LZF_END_BOX = 0, LZF_END_T = 1, LZF_END_CAP = 2 };
__device__ __forceinline__ void lzf_ray_end(const LzfOut& O, bool ph2, int ray, int kind, int composited, int report, float t, float ws, float d,
                                            float r, float g, float b, float a0, float a1, float u) {
    if (__builtin_expect(LZF_OUT(O, cap_mode) != 0, 0)) {
        report = composited;
        if (kind == LZF_END_T) {
            if (LZF_OUT(O, ray_counts)) { report = -composited; LZF_OUT(O, rays_t)[ray] = t; }
            if (!ph2) LZF_OUT(O, ray_last)[ray] = composited - 1;
        } else if (!ph2) {
            LZF_OUT(O, ray_last)[ray] = composited;          // LZF_END_CAP: composited == max_steps, the bin of the rays phase 2 continues
            if (kind == LZF_END_CAP) LZF_OUT(O, rays_t)[ray] = t;
        }
    }
    lzf_write_pixel(O, ray, ws, d, r, g, b, a0, a1, u, report);
}

// ---- host side, defined in lz_frame.hip --------------------------------------------------------------------------------------------
// zero the state words, then lz_k_frame_prepare (near / far, first occupied cell, background pixels, sort keys) and lz_k_frame_scatter
// (the queue, longest rays first)
int lzf_enqueue_queue(const LzFrameK& K, hipStream_t st);
// cap_mode 1, behind phase 1: histogram of ray_last, parked rays into the queue; sched: the last workgroup replays the schedule (C_eff)
void lzf_enqueue_cap_hist(const LzFrameK& K, bool sched, hipStream_t st);
// cap_mode 1, behind a histogram enqueued with sched = false (and summed over the tiles of the frame): the schedule replay on its own
void lzf_enqueue_schedule(const LzFrameK& K, hipStream_t st);
// cap_mode 1 with ray_counts, behind phase 2: marched counts of the rays the compositing cut inside a chunk
void lzf_enqueue_counts(const LzFrameK& K, hipStream_t st);
#endif
