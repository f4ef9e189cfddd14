// lz_ngp_frame.hip -- one inference frame of the hash-grid NeRF (BASELINE cfg2) as ONE persistent kernel: march -> 16-level hash-grid
// gather -> sigma / colour MLP (MFMA) -> composite per ray, the slot design of lz_frame.hip (lz_k_frame at one sample per ray and pass)
// around the network of lz_ngp.hip.  The launch loop it replaces (lz_ngp_loop_run: four launches per iteration of the reference's loop,
// 308 for a 256^2 x 128-step frame under the reference's schedule) moves xyzs / dirs / deltas / feats / sigmas / rgbs through HBM per
// sample; here a sample lives in registers from the march to the compositing, and a frame is 3 launches + 1 memset (cap_mode 0) or 6.
//
// What it computes is lz_ngp_loop_run's frame, bit for bit: the march is LzMarch::probe (lz_loop_march), a level's feature is
// lz_grid_interp on the same cell / corner offsets as lz_k_grid_forward_lmp (lz_grid_interp.h), the network is lzn_chain_sigma /
// lzn_chain_colour (f32 head, lz_ngp_chain.h) or lzn16_chain (f16 head, lz_ngp16_chain.h) -- a sample's sigma / rgb do not depend on
// which other samples share its slice -- and the compositing is lz_loop_composite_plain's arithmetic in its order.  Near / far, first
// occupied cell, background pixels, longest-first queue, the reference's cap (histogram of the last surviving chunk boundary, schedule
// replay, phase 2 over the parked rays) and the count fix-up are lz_frame.hip's own kernels (lz_frame_common.h).  So are the options of
// lz_ngp_frame_render_opts: perturb draws and the occupied cells' box (lz_k_frame_prepare; the persistent kernels take a ray's march end
// from t_end then), RGB24 pixels (lzf_write_pixel), and a tile of a larger frame, whose call stops behind the histogram and goes on in
// lz_ngp_frame_finish once the caller has summed it over the tiles (lz_frame_render / lz_frame_finish with defer_finish).
//
// MI355X shape
//   * A wave owns 16 ray slots with the f32 head (the B-operand columns of a 16x16x4 slice: lane (s, q) gathers levels q, q + 4, q + 8,
//     q + 12 of sample s -- exactly the k order lzn_load hands sigma_net.0) and 32 with the f16 head (a 32x32x16 slice: lane (s, h)
//     gathers levels 8 ks + 4 h + i, as lz_k_ngp_head16's load).  All 64 lanes gather; the slot lanes march and composite.
//   * Ray state lives in LDS between passes, with SH(4) of the ray's direction evaluated ONCE, when the slot takes the ray.
//   * Finished slots are refilled from the global queue with one wave-aggregated atomic; a wave leaves when the queue is dry and its slots
//     are empty.  No communication between workgroups, every loop bounded by the queue or the cap: the grid always drains.
//   * 256-thread workgroups: the f32 chain next to 32 eight-byte corner loads in flight does not fit the 128 registers of a 1024-thread
//     workgroup.  The 24 KB / 16 KB weight image, the level records, the Morton table and the slots take ~30 KB of LDS per workgroup;
//     as many workgroups per CU as the registers allow (asked from the runtime once per kernel), see kernel_resources.json.
//   * The whole table (49 MB f32, 24.5 MB half) is the L2 working set of every pass.  A stand-alone gather of this shape ran at 16 % of
//     the HBM roofline against 69 % level-major (lz_ngp.hip); inside the frame kernel -- three waves per SIMD, 32 corner loads in flight
//     per lane, other waves' march / matrix chain / compositing under the misses -- that did not carry over.  Measured:
//     fused beats the loop everywhere (256^2 x 128 steps f32 1.07 against 3.14 / 1.98 ms, 0.67 of the byte roofline) except on a 64^2
//     tile with the f16 head under the schedule (8, 8) (0.59 against 0.48 ms) -- a ray's ~75 dependent passes set a tile's time: for
//     tiles lz_ngp_frame_spp.hip runs S samples per ray and pass (lz_ngp_frame_render_spp; 0.18 ms in that cell).
#include <string.h>

#include <mutex>

#include "lz_ngp_frame_common.h"     // the argument record, the slot fields and what the S > 1 kernels (lz_ngp_frame_spp.hip) share

// PREC: 0 = f32 head (v_mfma_f32_16x16x4_f32), 1 = f16 head (v_mfma_f32_32x32x16_f16); TT: the table's element type
template <int PREC, typename TT>
__global__ void __launch_bounds__(LZNF_WG) lz_k_ngp_frame(LzNgpFrameArgs P, LzFrameK F) {
    static_assert(PREC == 0 || sizeof(TT) == 2, "the f16 head reads half features: half tables");
    constexpr int NS = PREC == 1 ? 32 : 16;                          // ray slots per wave = samples of a slice
    constexpr int SH_WORDS = PREC == 1 ? 8 : 16;
    constexpr int NF_OUT = NF_SH + SH_WORDS, NF = NF_OUT + (PREC == 1 ? 4 : 0);
    constexpr int W_WORDS = PREC == 1 ? LZN16_FRAGS * 64 * 4 : LZ_NGP_FRAGS * 64;
    constexpr int SLOT_WORDS = LZNF_WAVES * NF * NS;
    __shared__ __align__(16) float lds[W_WORDS + NL_FIELDS * LZNF_LEVELS + LZF_LUT + SLOT_WORDS + 4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool slot_lane = lane < NS;                                // the lane that marches / composites slot `lane`
    const int sl = lane;
    static_assert(alignof(LzNgpFrameArgs) <= 8 && sizeof(LzNgpFrameArgs) % 8 == 0, "F sits at sizeof(LzNgpFrameArgs) of the kernel-argument segment");
    const LzfOut OUT = lzf_out<sizeof(LzNgpFrameArgs)>();
    const bool ph2 = F.phase2 != 0;
    if (ph2 && F.state[LZF_P_SIZE] <= 0) return;                     // no ray parked at the cap (or C_eff == max_steps)
    {
        const float4* src = reinterpret_cast<const float4*>(P.packed);
        float4* dst = reinterpret_cast<float4*>(lds);
        for (uint32_t i = threadIdx.x; i < W_WORDS / 4; i += LZNF_WG) dst[i] = src[i];
    }
    uint32_t* lvtab = reinterpret_cast<uint32_t*>(lds + W_WORDS);
#pragma unroll
    for (int l = 0; l < LZNF_LEVELS; l++)                            // (unrolled: P.lv is read at constant offsets of the kernel arguments)
        if (threadIdx.x == (uint32_t)l) {
            const LzGridLevel r = lz_grid_level<3>(P.offsets, P.lv, l, 0u, false);
            lvtab[NL_OFF0 * LZNF_LEVELS + l] = r.off0; lvtab[NL_HS * LZNF_LEVELS + l] = r.hs; lvtab[NL_RES * LZNF_LEVELS + l] = r.res;
            lvtab[NL_SCALE * LZNF_LEVELS + l] = __float_as_uint(r.scale); lvtab[NL_MODE * LZNF_LEVELS + l] = r.mode;
        }
    uint32_t* mlut = lvtab + NL_FIELDS * LZNF_LEVELS;
    const bool use_lut = F.H <= LZF_LUT;
    if (use_lut) for (uint32_t i = threadIdx.x; i < LZF_LUT; i += LZNF_WG) mlut[i] = lz_expand_bits(i);
    float* slot = reinterpret_cast<float*>(mlut + LZF_LUT) + wave * NF * NS;     // this wave's slots: slot[field * NS + s]
    int* sloti = reinterpret_cast<int*>(slot);
    int* wg_stat = reinterpret_cast<int*>(lds + W_WORDS + NL_FIELDS * LZNF_LEVELS + LZF_LUT + SLOT_WORDS);   // [0] samples, [1] slices, [2] waves done
    if (slot_lane) sloti[NF_RAY * NS + sl] = -1;
    if (threadIdx.x < 4) wg_stat[threadIdx.x] = 0;
    __syncthreads();
    const int n_queue = F.state[ph2 ? LZF_P_SIZE : LZF_Q_SIZE];
    int* q_head = F.state + (ph2 ? LZF_P_HEAD : LZF_Q_HEAD);
    // samples at which a ray still alive is stopped: max_steps (cap_mode 0, and phase 1 of cap_mode 1), the schedule's C_eff in phase 2
    const int cap = ph2 ? F.state[LZF_CEFF] : (int)F.max_steps;
    const int cnt_base = ph2 ? (int)F.max_steps : 0;                 // samples a ray brings along when it takes a slot
    const TT* table = reinterpret_cast<const TT*>(P.emb);
    LzMarch m;
    bool dry = n_queue <= 0;
    int my_samples = 0, my_slices = 0;

    for (;;) {
        // ---------------- refill + march: every slot ends with a sample, crossing empty space, or empty with the queue dry ----------------
        int ray = slot_lane ? sloti[NF_RAY * NS + sl] : -1;
        bool have = false;
        float x = 0.0f, y = 0.0f, z = 0.0f;
        for (int attempt = 0; attempt < 4; attempt++) {
            const bool need = slot_lane && ray < 0 && !dry;
            const unsigned long long mask = __ballot(need);
            if (mask) {
                const int leader = __ffsll((long long)mask) - 1, take = __popcll(mask);
                int base = 0;
                if (lane == leader) base = atomicAdd(q_head, take);
                base = __shfl(base, leader, 64);
                if (need) {
                    const int idx = base + __popcll(mask & ((1ull << lane) - 1ull));
                    if (idx < n_queue) {
                        ray = F.order[idx];
                        sloti[NF_RAY * NS + sl] = ray;
                        slot[NF_T * NS + sl] = F.rays_t[ray];
                        slot[NF_FAR * NS + sl] = F.occ ? F.t_end[ray] : F.fars[ray];     // the march's end: clipped to the occupied cells' box
                        if (ph2) {                                   // the accumulators phase 1 parked in the output arrays
                            slot[NF_WS * NS + sl] = F.weights_sum[ray];
                            slot[NF_D * NS + sl] = F.depth[ray];
                            slot[NF_R * NS + sl] = F.image[(size_t)ray * 3];
                            slot[NF_G * NS + sl] = F.image[(size_t)ray * 3 + 1];
                            slot[NF_B * NS + sl] = F.image[(size_t)ray * 3 + 2];
                        } else {
#pragma unroll
                            for (int f = NF_WS; f <= NF_B; f++) slot[f * NS + sl] = 0.0f;
                        }
                        sloti[NF_CNT * NS + sl] = cnt_base;
                        const float* ro = F.rays_o + (size_t)ray * 3;
                        const float* rd = F.rays_d + (size_t)ray * 3;
                        const float d0 = rd[0], d1 = rd[1], d2 = rd[2];
                        slot[NF_RD * NS + sl] = 1 / d0; slot[(NF_RD + 1) * NS + sl] = 1 / d1; slot[(NF_RD + 2) * NS + sl] = 1 / d2;
                        slot[(NF_RD + 3) * NS + sl] = ro[0]; slot[(NF_RD + 4) * NS + sl] = ro[1]; slot[(NF_RD + 5) * NS + sl] = ro[2];
                        slot[(NF_RD + 6) * NS + sl] = d0; slot[(NF_RD + 7) * NS + sl] = d1; slot[(NF_RD + 8) * NS + sl] = d2;
                        // SH(4) of the direction the march hands every sample of the ray (lz_loop_march: dirs = rays_d): once per ray
                        float sh[16];
                        lz_sh_eval(d0, d1, d2, 4, sh, nullptr, nullptr, nullptr);
                        if constexpr (PREC == 1) {
#pragma unroll
                            for (int k = 0; k < 8; k++) slot[(NF_SH + k) * NS + sl] = __uint_as_float(h_cvt2(sh[2 * k], sh[2 * k + 1], false));
                        } else {
#pragma unroll
                            for (int k = 0; k < 16; k++) slot[(NF_SH + k) * NS + sl] = sh[k];
                        }
                    }
                }
                if (base + take >= n_queue) dry = true;              // wave-uniform
            }
            if (slot_lane && ray >= 0 && !have) {
                const float go[3] = {slot[(NF_RD + 3) * NS + sl], slot[(NF_RD + 4) * NS + sl], slot[(NF_RD + 5) * NS + sl]};
                const float gd[3] = {slot[(NF_RD + 6) * NS + sl], slot[(NF_RD + 7) * NS + sl], slot[(NF_RD + 8) * NS + sl]};
                m.init(go, gd, slot[NF_RD * NS + sl], slot[(NF_RD + 1) * NS + sl], slot[(NF_RD + 2) * NS + sl], F.bound, F.dt_gamma, F.mf, F.C, F.H, F.grid);
                if (use_lut) m.morton_lut = mlut;
                float t = slot[NF_T * NS + sl], dt = 0.0f;
                const float far = slot[NF_FAR * NS + sl];
                int probes = 0;
                while (t < far && probes < LZNF_MARCH_PROBES) {
                    if (m.probe(t, x, y, z, dt)) { have = true; break; }
                    probes++;
                }
                if (have) {
                    slot[NF_T * NS + sl] = t;
                    slot[NF_DT * NS + sl] = dt;
                } else if (t < far) {                                // still in empty space: resume from here in the next pass
                    slot[NF_T * NS + sl] = t;
                    x = y = z = 0.0f;
                } else {                                             // the ray left the box: no further sample
                    const int c0 = sloti[NF_CNT * NS + sl];
                    lzf_ray_end(OUT, ph2, ray, LZF_END_BOX, c0, c0, t, slot[NF_WS * NS + sl], slot[NF_D * NS + sl], slot[NF_R * NS + sl],
                                slot[NF_G * NS + sl], slot[NF_B * NS + sl], 0.0f, 0.0f, 0.0f);
                    my_samples += c0 - cnt_base;
                    ray = -1;
                    sloti[NF_RAY * NS + sl] = -1;
                    x = y = z = 0.0f;
                }
            }
            if (!__ballot(slot_lane && ray < 0 && !dry)) break;
        }
        __builtin_amdgcn_wave_barrier();     // the slots the slot lanes just wrote are read by the other lanes of this wave: keep the LDS order
        if (!__ballot(have)) {
            if (dry && !__ballot(slot_lane && ray >= 0)) break;      // queue dry and every slot empty: this wave is done
            continue;                                                // slots still crossing empty space
        }
        // ---------------- gather + network: exactly a slice of the stand-alone gather and head ----------------
        float sg = 0.0f, c0 = 0.0f, c1 = 0.0f, c2 = 0.0f;            // the sample's sigma / rgb on its slot lane
        if constexpr (PREC == 0) {
            const int s = lane & 15, q = lane >> 4;
            // (slots without a sample carry the position 0: in range, its loads are harmless and its columns are dropped)
            const float xin[3] = {lz_grid_unit(__shfl(x, s, 64), F.bound, P.inv2b), lz_grid_unit(__shfl(y, s, 64), F.bound, P.inv2b), lz_grid_unit(__shfl(z, s, 64), F.bound, P.inv2b)};
            LzGridCell<3> cell[4];
            LzVec<TT, 2> cv[4][8];
#pragma unroll
            for (int i = 0; i < 4; i++) {                            // levels q, q + 4, q + 8, q + 12: all 32 corner loads in flight
                const int l = q + 4 * i;
                LzGridLevel lvl;
                lvl.off0 = lvtab[NL_OFF0 * LZNF_LEVELS + l]; lvl.hs = lvtab[NL_HS * LZNF_LEVELS + l]; lvl.res = lvtab[NL_RES * LZNF_LEVELS + l];
                lvl.scale = __uint_as_float(lvtab[NL_SCALE * LZNF_LEVELS + l]); lvl.mode = lvtab[NL_MODE * LZNF_LEVELS + l];
                cell[i] = lz_grid_cell<3, true>(xin, lvl.scale, false);
                uint32_t index[8];
                lz_grid_corner_offsets<3>(lvl, cell[i], 2u, 0u, false, index);
                const TT* g = table + (size_t)lvl.off0 * 2;
#pragma unroll
                for (int c = 0; c < 8; c++) __builtin_memcpy(&cv[i][c], __builtin_assume_aligned(g + index[c], sizeof(TT) * 2), sizeof(TT) * 2);
            }
            float b1[1][8];
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const LzVec<TT, 2> o = lz_grid_interp<TT, 3, 2>(cell[i], cv[i]);
                b1[0][2 * i] = (float)o.v[0]; b1[0][2 * i + 1] = (float)o.v[1];      // half tables: widened, as lzn_load does for tiled f16 features
            }
            const float* wl = lds;
            LznOut<1> o;
            lzn_chain_sigma<1>(wl, lane, b1, o);
#pragma unroll
            for (int ks = 0; ks < 4; ks++) o.shq[0][ks] = slot[(NF_SH + 4 * ks + q) * NS + s];
            lzn_chain_colour<1>(wl, lane, o);
            my_slices += 1;
            if (q == 0) {                                            // lanes q == 0 hold valid bits: they are the slot lanes
                sg = lz_expf(o.h[0][0]);
                c0 = lz_sigmoidf(o.c[0][0]); c1 = lz_sigmoidf(o.c[0][1]); c2 = lz_sigmoidf(o.c[0][2]);
            }
        } else {
            const int s = lane & 31, h = lane >> 5;
            const float xin[3] = {lz_grid_unit(__shfl(x, s, 64), F.bound, P.inv2b), lz_grid_unit(__shfl(y, s, 64), F.bound, P.inv2b), lz_grid_unit(__shfl(z, s, 64), F.bound, P.inv2b)};
            uint32_t fw[8];
#pragma unroll
            for (int ks = 0; ks < 2; ks++) {                         // levels 8 ks + 4 h + i: 32 four-byte corner loads in flight per k-step
                LzGridCell<3> cell[4];
                LzVec<TT, 2> cv[4][8];
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    const int l = 8 * ks + 4 * h + i;
                    LzGridLevel lvl;
                    lvl.off0 = lvtab[NL_OFF0 * LZNF_LEVELS + l]; lvl.hs = lvtab[NL_HS * LZNF_LEVELS + l]; lvl.res = lvtab[NL_RES * LZNF_LEVELS + l];
                    lvl.scale = __uint_as_float(lvtab[NL_SCALE * LZNF_LEVELS + l]); lvl.mode = lvtab[NL_MODE * LZNF_LEVELS + l];
                    cell[i] = lz_grid_cell<3, true>(xin, lvl.scale, false);
                    uint32_t index[8];
                    lz_grid_corner_offsets<3>(lvl, cell[i], 2u, 0u, false, index);
                    const TT* g = table + (size_t)lvl.off0 * 2;
#pragma unroll
                    for (int c = 0; c < 8; c++) __builtin_memcpy(&cv[i][c], __builtin_assume_aligned(g + index[c], sizeof(TT) * 2), sizeof(TT) * 2);
                }
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    const LzVec<TT, 2> o = lz_grid_interp<TT, 3, 2>(cell[i], cv[i]);
                    __builtin_memcpy(&fw[4 * ks + i], &o, 4);        // one half2 word: both channels of the level
                }
            }
            uint32_t shw[4];
#pragma unroll
            for (int k = 0; k < 4; k++) shw[k] = __float_as_uint(slot[(NF_SH + 4 * h + k) * NS + s]);
            float rgb_a, b_out;
            lzn16_chain(reinterpret_cast<const lz_h8*>(lds), lane, h, fw, shw, rgb_a, b_out);
            my_slices += 2;
            // a sample's four values come out two per lane half: parked for the slot lanes (OUT + 0 .. 2 = rgb, + 3 = sigma)
            slot[(NF_OUT + h) * NS + s] = rgb_a;
            slot[(NF_OUT + 2 + h) * NS + s] = b_out;
            __builtin_amdgcn_wave_barrier();
            if (slot_lane) {
                c0 = slot[NF_OUT * NS + sl]; c1 = slot[(NF_OUT + 1) * NS + sl]; c2 = slot[(NF_OUT + 2) * NS + sl];
                sg = slot[(NF_OUT + 3) * NS + sl];
            }
        }
        // ---------------- composite (lz_loop_composite_plain, one sample): the slot lanes ----------------
        if (have) {
            const float dt = slot[NF_DT * NS + sl];
            float ws = slot[NF_WS * NS + sl];
            const float alpha = 1.0f - lz_expf(-sg * dt);
            const float T = 1 - ws;
            const float w = alpha * T;
            ws += w;
            const float t = slot[NF_T * NS + sl] + dt;
            const float d = lz_fmaf(w, t, slot[NF_D * NS + sl]);
            const float r = lz_fmaf(w, c0, slot[NF_R * NS + sl]);
            const float g = lz_fmaf(w, c1, slot[NF_G * NS + sl]);
            const float b = lz_fmaf(w, c2, slot[NF_B * NS + sl]);
            const int cnt = sloti[NF_CNT * NS + sl] + 1;
            if (T < F.T_thresh || cnt >= cap) {
                lzf_ray_end(OUT, ph2, ray, T < F.T_thresh ? LZF_END_T : LZF_END_CAP, cnt, cnt, t, ws, d, r, g, b, 0.0f, 0.0f, 0.0f);
                my_samples += cnt - cnt_base;
                sloti[NF_RAY * NS + sl] = -1;
            } else {
                slot[NF_T * NS + sl] = t;
                slot[NF_WS * NS + sl] = ws; slot[NF_D * NS + sl] = d;
                slot[NF_R * NS + sl] = r; slot[NF_G * NS + sl] = g; slot[NF_B * NS + sl] = b;
                sloti[NF_CNT * NS + sl] = cnt;
            }
        }
    }
    // ---------------- statistics: wave -> workgroup (LDS) -> one pair of global atomics by the last wave out ----------------
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) my_samples += __shfl_xor(my_samples, off, 64);
    if (lane == 0) {
        atomicAdd(&wg_stat[0], my_samples);
        atomicAdd(&wg_stat[1], my_slices);
        __threadfence_block();
        if (atomicAdd(&wg_stat[2], 1) == LZNF_WAVES - 1) {
            const int a = atomicAdd(&wg_stat[0], 0), b = atomicAdd(&wg_stat[1], 0);
            if (a) atomicAdd(F.state + LZF_SAMPLES, a);
            if (b) atomicAdd(F.state + LZF_ROWS, 16 * b);
        }
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
// workgroups of `kernel` a CU holds at a time (registers and LDS decide): asked from the runtime once per device and variant -- a host
// call without synchronisation -- and kept under a lock, like lz_frame.hip's per-device pool
template <typename K>
static int lznf_wg_per_cu(K kernel, int variant) {
    static std::mutex mu;
    static int cache[64][3] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 1;
    std::lock_guard<std::mutex> lock(mu);
    if (cache[dev][variant] <= 0) {
        int n = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kernel, LZNF_WG, 0) != hipSuccess || n < 1) n = 1;
        cache[dev][variant] = n;
    }
    return cache[dev][variant];
}

// variant: 0 = f32 tables + f32 head, 1 = half tables + f16 head, 2 = half tables + f32 head
static void lznf_launch(int variant, uint32_t N, const LzNgpFrameArgs& a, const LzFrameK& K, hipStream_t st) {
    const int slots = variant == 1 ? 32 : 16;
    int wg = 1;
    if (variant == 0) wg = lznf_wg_per_cu(lz_k_ngp_frame<0, float>, 0);
    else if (variant == 1) wg = lznf_wg_per_cu(lz_k_ngp_frame<1, __half>, 1);
    else wg = lznf_wg_per_cu(lz_k_ngp_frame<0, __half>, 2);
    uint32_t grid = lz_div_up(N, (uint32_t)slots * LZNF_WAVES);      // no more workgroups than there are rays for one slot row per wave
    const uint32_t cap = (uint32_t)lz_cu_count() * (uint32_t)wg;
    grid = grid < 1 ? 1 : (grid > cap ? cap : grid);
    if (variant == 0) hipLaunchKernelGGL((lz_k_ngp_frame<0, float>), dim3(grid), dim3(LZNF_WG), 0, st, a, K);
    else if (variant == 1) hipLaunchKernelGGL((lz_k_ngp_frame<1, __half>), dim3(grid), dim3(LZNF_WG), 0, st, a, K);
    else hipLaunchKernelGGL((lz_k_ngp_frame<0, __half>), dim3(grid), dim3(LZNF_WG), 0, st, a, K);
}

// what is refused whatever N is: the descriptor's modes, and the option rules of lz_ngp_frame_render_opts (o may be null)
static int lznf_check_modes(const lz_frame_ngp_fused* f, const lz_frame_ngp_fused_opts* o) {
    LZ_REQUIRE(f, LZ_ERR_BAD_ARGUMENT, "ngp_frame_render: null");
    LZ_REQUIRE(f->precision == 0 || f->precision == 1, LZ_ERR_BAD_ARGUMENT, "ngp_frame_render: precision must be 0 (f32 head) or 1 (f16 head)");
    LZ_REQUIRE(f->cap_mode == LZ_FRAME_CAP_PER_RAY || f->cap_mode == LZ_FRAME_CAP_REFERENCE, LZ_ERR_BAD_ARGUMENT,
               "ngp_frame_render: cap_mode must be 0 (per ray) or 1 (the reference's schedule)");
    if (f->cap_mode == LZ_FRAME_CAP_REFERENCE)
        LZ_REQUIRE(f->max_steps <= LZF_CAP_MAX_STEPS, LZ_ERR_UNSUPPORTED, "ngp_frame_render: cap_mode 1 supports max_steps <= %d", LZF_CAP_MAX_STEPS);
    if (o) {
        LZ_REQUIRE(!o->occupied_aabb || o->t_end, LZ_ERR_BAD_ARGUMENT, "ngp_frame_render_opts: occupied_aabb needs the t_end scratch buffer");
        LZ_REQUIRE(!o->defer_finish || f->cap_mode == LZ_FRAME_CAP_REFERENCE, LZ_ERR_BAD_ARGUMENT,
                   "ngp_frame_render_opts: defer_finish splits the reference's cap (cap_mode 1); cap_mode 0 has no second phase");
    }
    return LZ_OK;
}

// the rest of the descriptor, and the two kernel-argument records filled from it (N > 0)
static int lznf_fill(const lz_frame_ngp_fused* f, const lz_frame_ngp_fused_opts* o, LzNgpFrameArgs& a, LzFrameK& K) {
    LZ_REQUIRE(f->state, LZ_ERR_BAD_ARGUMENT, "ngp_frame_render: null state");
    LZ_REQUIRE((f->precision == 1 ? f->packed16 != nullptr : f->packed != nullptr) && f->embeddings && f->offsets, LZ_ERR_BAD_ARGUMENT,
               "ngp_frame_render: incomplete network (packed for precision 0, packed16 for precision 1, embeddings, offsets)");
    LZ_REQUIRE(f->precision == 0 || f->emb_f16 == 1, LZ_ERR_BAD_ARGUMENT, "ngp_frame_render: the f16 head reads half features (emb_f16 = 1)");
    LZ_REQUIRE(f->enc_L == LZNF_LEVELS && f->enc_H >= 1, LZ_ERR_UNSUPPORTED, "ngp_frame_render: num_levels must be %d (get_encoder('hashgrid') defaults)", LZNF_LEVELS);
    LZ_REQUIRE(f->rays_o && f->rays_d && f->grid && f->aabb && f->nears && f->fars && f->rays_t && f->order && f->keys && f->scratch &&
                   f->weights_sum && f->depth && f->image && f->out,
               LZ_ERR_BAD_ARGUMENT, "ngp_frame_render: incomplete lz_frame_ngp_fused");
    LZ_REQUIRE(f->C >= 1 && f->C <= 8 && f->H > 0 && f->bound > 0.0f, LZ_ERR_BAD_ARGUMENT, "ngp_frame_render: cascade in [1, 8], grid size and bound positive");
    if (f->cap_mode == LZ_FRAME_CAP_REFERENCE) {
        LZ_REQUIRE(f->ray_last && f->cap_ws, LZ_ERR_BAD_ARGUMENT, "ngp_frame_render: cap_mode 1 needs the ray_last and cap_ws buffers");
        LZ_REQUIRE(f->N_total == 0 || f->N_total >= f->N, LZ_ERR_BAD_ARGUMENT, "ngp_frame_render: N_total is the schedule's ray budget (>= N)");
    }
    a.packed = f->precision == 1 ? f->packed16 : static_cast<const void*>(f->packed);
    a.emb = f->embeddings;
    a.offsets = f->offsets;
    a.inv2b = 1.0f / (2.0f * f->bound);
    LZ_REQUIRE(lz_fill_levels(a.lv, f->enc_L, f->enc_S, f->enc_H) == 0, LZ_ERR_UNSUPPORTED, "ngp_frame_render: at most %d levels", LZ_MAX_LEVELS);
    memset(&K, 0, sizeof(K));
    K.rays_o = f->rays_o; K.rays_d = f->rays_d; K.grid = f->grid; K.aabb = f->aabb;
    K.nears = f->nears; K.fars = f->fars; K.rays_t = f->rays_t;
    K.order = f->order; K.state = f->state; K.keys = f->keys;
    K.weights_sum = f->weights_sum; K.depth = f->depth; K.image = f->image;
    K.amb0_sum = K.amb1_sum = K.unc_sum = f->scratch;               // the shared pixel writer's three extra channels: no such outputs here
    K.out = f->out; K.bg = f->bg; K.out_rgb24 = nullptr; K.ray_counts = f->ray_counts;
    K.bg_scalar = f->bg_scalar; K.bound = f->bound; K.dt_gamma = f->dt_gamma; K.T_thresh = f->T_thresh; K.min_near = f->min_near;
    K.N = f->N; K.max_steps = f->max_steps; K.C = f->C; K.H = f->H;
    K.ray_last = f->ray_last; K.cap_ws = f->cap_ws; K.cap_mode = f->cap_mode; K.phase2 = 0; K.N_total = f->N_total;
    K.mf = lz_march_frame(f->bound, f->max_steps, f->C, f->H);
    if (o) {                                                         // lz_ngp_frame_render_opts: what lz_k_frame_prepare and lzf_write_pixel already do
        K.noises = o->noises;
        K.occ = o->occupied_aabb; K.t_end = o->t_end;
        K.out_rgb24 = o->out_rgb24;
    }
    return LZ_OK;
}

static int lznf_variant(const lz_frame_ngp_fused* f) { return f->precision == 1 ? 1 : (f->emb_f16 ? 2 : 0); }

// the persistent kernel over the queue (phase 1) or over the rays parked at the cap (K.phase2), S samples per ray and pass
static void lznf_launch_persistent(int variant, uint32_t S, uint32_t N, const LzNgpFrameArgs& a, const LzFrameK& K, hipStream_t st) {
    if (S == 1) lznf_launch(variant, N, a, K, st);
    else lznf_spp_launch(variant, S, N, a, K, st);
}

// the frame at `steps_per_pass` samples per ray and pass: 1 = lz_k_ngp_frame, 2 .. 16 = lz_k_ngp_frame_spp, 0 = lznf_spp_auto's choice
static int lznf_render(const lz_frame_ngp_fused* f, const lz_frame_ngp_fused_opts* o, uint32_t steps_per_pass, lz_timing* timing, lz_stream_t stream) {
    int rc = lznf_check_modes(f, o);
    if (rc != LZ_OK) return rc;
    hipStream_t st = lz_st(stream);
    const bool defer = o && o->defer_finish;
    if (f->N == 0) {                                                 // no ray: nothing to launch; a state buffer says "no samples"
        hipError_t e = hipSuccess;
        if (f->state) e = hipMemsetAsync(f->state, 0, LZ_FRAME_STATE_INTS * sizeof(int32_t), st);
        // an empty tile of a larger frame: its words of the histogram the caller sums over the tiles read zero
        if (e == hipSuccess && defer && f->cap_ws) e = hipMemsetAsync(f->cap_ws, 0, LZ_FRAME_CAP_WS_INTS((size_t)f->max_steps) * sizeof(int32_t), st);
        if (e != hipSuccess) { lz_set_error("ngp_frame_render: memset: %s", hipGetErrorString(e)); return (int)e; }
        return LZ_OK;
    }
    LzNgpFrameArgs a;
    LzFrameK K;
    rc = lznf_fill(f, o, a, K);
    if (rc != LZ_OK) return rc;
    const int variant = lznf_variant(f);
    const uint32_t S = steps_per_pass ? steps_per_pass : lznf_spp_auto(variant, f->N, f->max_steps);
    rc = lzf_enqueue_queue(K, st);                                   // memset + prepare + scatter (lz_frame.hip)
    if (rc != LZ_OK) return rc;
    if (timing) (void)lz_timing_mark(timing, 0, stream);             // the event pair brackets the phase-1 persistent kernel alone
    lznf_launch_persistent(variant, S, f->N, a, K, st);
    if (timing) (void)lz_timing_mark(timing, 1, stream);
    if (f->cap_mode == LZ_FRAME_CAP_REFERENCE) {
        // histogram of ray_last, parked rays queued; a whole frame also replays the schedule there (C_eff), a tile leaves that to
        // lz_ngp_frame_finish, behind the caller's sum of the histogram over the tiles
        lzf_enqueue_cap_hist(K, !defer, st);
        if (!defer) {
            K.phase2 = 1;
            // the parked rays up to C_eff (an early-out launch when none), in phase 1's launch shape: N bounds their number
            lznf_launch_persistent(variant, S, f->N, a, K, st);
            if (f->ray_counts) lzf_enqueue_counts(K, st);
        }
    }
    LZ_CHECK_LAUNCH("ngp_frame_render");
    return LZ_OK;
}

static bool lznf_spp_valid(uint32_t S) { return S == 0 || S == 1 || S == 2 || S == 4 || S == 8 || S == 16; }

extern "C" int lz_ngp_frame_render(const lz_frame_ngp_fused* f, lz_timing* timing, lz_stream_t stream) {
    return lznf_render(f, nullptr, 1, timing, stream);
}

extern "C" int lz_ngp_frame_render_spp(const lz_frame_ngp_fused* f, uint32_t steps_per_pass, lz_timing* timing, lz_stream_t stream) {
    LZ_REQUIRE(lznf_spp_valid(steps_per_pass), LZ_ERR_BAD_ARGUMENT, "ngp_frame_render_spp: steps_per_pass must be 0 (auto), 1, 2, 4, 8 or 16, not %u",
               steps_per_pass);
    return lznf_render(f, nullptr, steps_per_pass, timing, stream);
}

extern "C" int lz_ngp_frame_render_opts(const lz_frame_ngp_fused* f, const lz_frame_ngp_fused_opts* o, uint32_t steps_per_pass, lz_timing* timing,
                                        lz_stream_t stream) {
    LZ_REQUIRE(lznf_spp_valid(steps_per_pass), LZ_ERR_BAD_ARGUMENT, "ngp_frame_render_opts: steps_per_pass must be 0 (auto), 1, 2, 4, 8 or 16, not %u",
               steps_per_pass);
    return lznf_render(f, o, steps_per_pass, timing, stream);
}

// the second half of a frame begun with defer_finish, behind the caller's sum of cap_ws[0 .. max_steps] over the tiles: the schedule replay
// (C_eff, the chunk boundaries), phase 2 in phase 1's launch shape -- S from the same rule on the same arguments: nothing is kept between
// the two calls -- and the count fix-up.  lz_frame_finish is the model.
extern "C" int lz_ngp_frame_finish(const lz_frame_ngp_fused* f, const lz_frame_ngp_fused_opts* o, uint32_t steps_per_pass, lz_stream_t stream) {
    LZ_REQUIRE(lznf_spp_valid(steps_per_pass), LZ_ERR_BAD_ARGUMENT, "ngp_frame_finish: steps_per_pass must be 0 (auto), 1, 2, 4, 8 or 16, not %u",
               steps_per_pass);
    int rc = lznf_check_modes(f, o);
    if (rc != LZ_OK) return rc;
    LZ_REQUIRE(f->cap_mode == LZ_FRAME_CAP_REFERENCE, LZ_ERR_BAD_ARGUMENT, "ngp_frame_finish: only after lz_ngp_frame_render_opts with cap_mode 1");
    if (f->N == 0) return LZ_OK;                                     // an empty tile
    LzNgpFrameArgs a;
    LzFrameK K;
    rc = lznf_fill(f, o, a, K);
    if (rc != LZ_OK) return rc;
    hipStream_t st = lz_st(stream);
    const int variant = lznf_variant(f);
    const uint32_t S = steps_per_pass ? steps_per_pass : lznf_spp_auto(variant, f->N, f->max_steps);
    lzf_enqueue_schedule(K, st);
    K.phase2 = 1;
    lznf_launch_persistent(variant, S, f->N, a, K, st);
    if (f->ray_counts) lzf_enqueue_counts(K, st);
    LZ_CHECK_LAUNCH("ngp_frame_finish");
    return LZ_OK;
}
