// lz_ngp_frame_spp.hip -- the persistent kernel of the hash-grid NeRF frame (lz_ngp_frame.hip) with S = 2, 4, 8 or 16 samples per ray
// and pass: lz_k_ngp_frame_spp<PREC, TT, S>, reached through lz_ngp_frame_render_spp.
//
// Why: at one sample per pass a ray of ~75 samples is ~75 DEPENDENT passes (march -> 16-level gather -> MLP -> composite), whatever the
// number of rays.  A full frame hides that behind other waves; a tile, a crop or a preview has too few rays to fill the chip's slots, and
// the dependent chain sets the frame time.  Here a slice keeps its NS columns (16 with the f32 head, 32 with the f16 head), but they
// hold NS / S rays with S consecutive samples each, so a ray needs ~75 / S passes (lz_frame.hip's S > 1 layout, "group leaders").
//
// A pass:
//   march      the group leader (lane r S of ray r's S columns) marches up to S samples in sequence with LzMarch::probe, sample j + 1
//              starting at t + dt of sample j -- lz_k_march_rays under n_step > 1, the same f32 operations in the same order -- and
//              stages position, dt and end t per column in LDS.  A group is SHORT when the ray leaves the box, when the cap is
//              nearer than S samples, or when the empty-cell budget of the attempt (LZNF_MARCH_PROBES) runs out.
//   gather/MLP all 64 lanes, over the staged columns: lznf_gather4, lzn_chain_sigma / lzn_chain_colour or lzn16_chain as at S = 1 (a
//              sample's sigma / rgb do not depend on its slice-mates); the outputs are parked per column in LDS.
//   composite  the leader walks its staged samples in order with lz_loop_composite_plain's arithmetic and stops at the first
//              T < T_thresh or at the cap; what it staged beyond that is dropped.
//
// S is a launch shape only: a ray stops EXACTLY at the cap (max_steps in phase 1, C_eff in phase 2), also in the middle of a group, so
// image, image_raw, weights_sum, depth, per-ray counts, ray_last, the parked accumulators and state[LZF_SAMPLES] are those of S = 1
// bit for bit under either cap mode.  state[LZF_ROWS] counts the slices actually run (columns, used or not) and differs with S.
// Refill (one wave-aggregated atomic), SH(4) once per ray, queue / cap bounded loops, the statistics: as lz_k_ngp_frame.
#include <mutex>

#include "lz_ngp_frame_common.h"

// staging fields of a column, behind the ray fields of lz_ngp_frame_common.h (which sit at the leader's column)
template <int PREC> struct LznfSppFields {
    static constexpr int SH_WORDS = PREC == 1 ? 8 : 16;
    static constexpr int KK = NF_SH + SH_WORDS;       // leader: samples staged in this pass
    static constexpr int X = KK + 1, Y = X + 1, Z = Y + 1, SDT = Z + 1, TE = SDT + 1;     // position, dt, end t of the column's sample
    static constexpr int OUT = TE + 1;                // rgb[0], rgb[1], rgb[2], sigma of the column's sample
    static constexpr int COUNT = OUT + 4;
};

// PREC: 0 = f32 head (v_mfma_f32_16x16x4_f32), 1 = f16 head (v_mfma_f32_32x32x16_f16); TT: the table's element type; S: samples per ray and pass
template <int PREC, typename TT, int S>
__global__ void __launch_bounds__(LZNF_WG) lz_k_ngp_frame_spp(LzNgpFrameArgs P, LzFrameK F) {
    static_assert(PREC == 0 || sizeof(TT) == 2, "the f16 head reads half features: half tables");
    static_assert(S == 2 || S == 4 || S == 8 || S == 16, "samples per ray and pass");
    constexpr int NS = PREC == 1 ? 32 : 16;                          // columns of a slice = NS / S rays x S samples
    using FL = LznfSppFields<PREC>;
    constexpr int NF = FL::COUNT;
    constexpr int W_WORDS = LznfLds<PREC>::W_WORDS;
    constexpr int SLOT_WORDS = LZNF_WAVES * NF * NS;
    __shared__ __align__(16) float lds[LznfLds<PREC>::FIXED_WORDS + SLOT_WORDS + 4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int s = lane & (NS - 1), j = s & (S - 1), lead = s - j;    // column s = sample j of the ray whose state sits at column `lead`
    const bool leader = lane < NS && j == 0;                         // the lane that marches / composites the ray at column `lane`
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
    float* slot = reinterpret_cast<float*>(mlut + LZF_LUT) + wave * NF * NS;     // this wave's columns: slot[field * NS + s]
    int* sloti = reinterpret_cast<int*>(slot);
    int* wg_stat = reinterpret_cast<int*>(lds + LznfLds<PREC>::FIXED_WORDS + SLOT_WORDS);   // [0] samples, [1] slices, [2] waves done
    if (lane < NS) { sloti[NF_RAY * NS + lane] = -1; sloti[FL::KK * NS + lane] = 0; }
    if (threadIdx.x < 4) wg_stat[threadIdx.x] = 0;
    if (!ph2 && blockIdx.x == 0 && threadIdx.x == 0) F.state[LZNF_SPP] = S;
    __syncthreads();
    const int n_queue = F.state[ph2 ? LZF_P_SIZE : LZF_Q_SIZE];
    int* q_head = F.state + (ph2 ? LZF_P_HEAD : LZF_Q_HEAD);
    // samples at which a ray still alive is stopped: max_steps (cap_mode 0, and phase 1 of cap_mode 1), the schedule's C_eff in phase 2
    const int cap = ph2 ? F.state[LZF_CEFF] : (int)F.max_steps;
    const int cnt_base = ph2 ? (int)F.max_steps : 0;                 // samples a ray brings along when it takes a slot
    const TT* table = reinterpret_cast<const TT*>(P.emb);
    bool dry = n_queue <= 0;
    int my_samples = 0, my_slices = 0;

    for (;;) {
        // ---------------- refill + march (group leaders): every ray ends with up to S staged samples, crossing empty space, or gone ----------------
        int ray = leader ? sloti[NF_RAY * NS + lane] : -1;
        int kk = 0;                                                  // samples staged in this pass
        bool left = false;                                           // the ray left the box behind its staged samples
        for (int attempt = 0; attempt < 4; attempt++) {
            const bool need = leader && ray < 0 && !dry;
            const unsigned long long mask = __ballot(need);
            if (mask) {
                const int first = __ffsll((long long)mask) - 1, take = __popcll(mask);
                int base = 0;
                if (lane == first) base = atomicAdd(q_head, take);
                base = __shfl(base, first, 64);
                if (need) {
                    const int idx = base + __popcll(mask & ((1ull << lane) - 1ull));
                    if (idx < n_queue) {
                        ray = F.order[idx];
                        lznf_take_ray<PREC, NS>(F, ph2, ray, cnt_base, slot, lane);
                    }
                }
                if (base + take >= n_queue) dry = true;              // wave-uniform
            }
            if (leader && ray >= 0 && kk == 0) {
                LzMarch m;
                lznf_march_init<NS>(m, F, slot, lane, use_lut, mlut);
                float t = slot[NF_T * NS + lane];
                const float far = slot[NF_FAR * NS + lane];
                const int c0 = sloti[NF_CNT * NS + lane];
                const int want = min(S, cap - c0);                   // >= 1: a ray at the cap has left its slot
                int probes = 0;
                while (t < far && kk < want && probes < LZNF_MARCH_PROBES) {
                    float x, y, z, dt;
                    if (m.probe(t, x, y, z, dt)) {                   // lz_k_march_rays: the sample, then t += dt
                        const int col = lane + kk;                   // < NS: kk < S
                        slot[FL::X * NS + col] = x; slot[FL::Y * NS + col] = y; slot[FL::Z * NS + col] = z;
                        slot[FL::SDT * NS + col] = dt;
                        t += dt;
                        slot[FL::TE * NS + col] = t;
                        kk++;
                    } else probes++;
                }
                slot[NF_T * NS + lane] = t;                          // where the next pass (or the next attempt, in empty space) resumes
                left = !(t < far);
                if (left && kk == 0) {                               // the ray left the box: no further sample
                    lzf_ray_end(OUT, ph2, ray, LZF_END_BOX, c0, c0, t, slot[NF_WS * NS + lane], slot[NF_D * NS + lane], slot[NF_R * NS + lane],
                                slot[NF_G * NS + lane], slot[NF_B * NS + lane], 0.0f, 0.0f, 0.0f);
                    my_samples += c0 - cnt_base;
                    ray = -1;
                    sloti[NF_RAY * NS + lane] = -1;
                    left = false;
                }
            }
            if (!__ballot(leader && ray < 0 && !dry)) break;
        }
        if (leader) sloti[FL::KK * NS + lane] = kk;
        __builtin_amdgcn_wave_barrier();     // what the leaders staged is read by the other lanes of this wave: keep the LDS order
        if (!__ballot(kk > 0)) {
            if (dry && !__ballot(leader && ray >= 0)) break;         // queue dry and every slot empty: this wave is done
            continue;                                                // rays still crossing empty space
        }
        // ---------------- gather + network over the staged columns: exactly a slice of the stand-alone gather and head ----------------
        // (columns without a sample carry the position 0: in range, its loads are harmless and its outputs are not read)
        const bool live = j < sloti[FL::KK * NS + lead];
        const float xin[3] = {lz_grid_unit(live ? slot[FL::X * NS + s] : 0.0f, F.bound, P.inv2b), lz_grid_unit(live ? slot[FL::Y * NS + s] : 0.0f, F.bound, P.inv2b),
                              lz_grid_unit(live ? slot[FL::Z * NS + s] : 0.0f, F.bound, P.inv2b)};
        if constexpr (PREC == 0) {
            const int q = lane >> 4;
            LzVec<TT, 2> lv4[4];
            lznf_gather4<TT>(table, lvtab, xin, q, 4, lv4);          // levels q, q + 4, q + 8, q + 12: the k order lzn_load hands sigma_net.0
            float b1[1][8];
#pragma unroll
            for (int i = 0; i < 4; i++) { b1[0][2 * i] = (float)lv4[i].v[0]; b1[0][2 * i + 1] = (float)lv4[i].v[1]; }     // half tables: widened, as lzn_load does
            const float* wl = lds;
            LznOut<1> o;
            lzn_chain_sigma<1>(wl, lane, b1, o);
#pragma unroll
            for (int ks = 0; ks < 4; ks++) o.shq[0][ks] = slot[(NF_SH + 4 * ks + q) * NS + lead];
            lzn_chain_colour<1>(wl, lane, o);
            my_slices += 1;
            if (q == 0) {                                            // lanes q == 0 hold valid bits: lane = column
                slot[FL::OUT * NS + s] = lz_sigmoidf(o.c[0][0]); slot[(FL::OUT + 1) * NS + s] = lz_sigmoidf(o.c[0][1]);
                slot[(FL::OUT + 2) * NS + s] = lz_sigmoidf(o.c[0][2]);
                slot[(FL::OUT + 3) * NS + s] = lz_expf(o.h[0][0]);
            }
        } else {
            const int h = lane >> 5;
            uint32_t fw[8];
#pragma unroll
            for (int ks = 0; ks < 2; ks++) {                         // levels 8 ks + 4 h + i: 32 four-byte corner loads in flight per k-step
                LzVec<TT, 2> lv4[4];
                lznf_gather4<TT>(table, lvtab, xin, 8 * ks + 4 * h, 1, lv4);
#pragma unroll
                for (int i = 0; i < 4; i++) __builtin_memcpy(&fw[4 * ks + i], &lv4[i], 4);       // one half2 word: both channels of the level
            }
            uint32_t shw[4];
#pragma unroll
            for (int k = 0; k < 4; k++) shw[k] = __float_as_uint(slot[(NF_SH + 4 * h + k) * NS + lead]);
            float rgb_a, b_out;
            lzn16_chain(reinterpret_cast<const lz_h8*>(lds), lane, h, fw, shw, rgb_a, b_out);
            my_slices += 2;
            // a sample's four values come out two per lane half (OUT + 0 .. 2 = rgb, + 3 = sigma)
            slot[(FL::OUT + h) * NS + s] = rgb_a;
            slot[(FL::OUT + 2 + h) * NS + s] = b_out;
        }
        __builtin_amdgcn_wave_barrier();
        // ---------------- composite (lz_loop_composite_plain, the staged samples in order): the leaders ----------------
        if (kk > 0) {
            float ws = slot[NF_WS * NS + lane], d = slot[NF_D * NS + lane];
            float r = slot[NF_R * NS + lane], g = slot[NF_G * NS + lane], b = slot[NF_B * NS + lane];
            float t = 0.0f;
            int cnt = sloti[NF_CNT * NS + lane];
            bool cut = false;
            for (int step = 0; step < kk; step++) {
                const int col = lane + step;
                const float alpha = 1.0f - lz_expf(-slot[(FL::OUT + 3) * NS + col] * slot[FL::SDT * NS + col]);
                const float T = 1 - ws;
                const float w = alpha * T;
                ws += w;
                t = slot[FL::TE * NS + col];
                d = lz_fmaf(w, t, d);
                r = lz_fmaf(w, slot[FL::OUT * NS + col], r);
                g = lz_fmaf(w, slot[(FL::OUT + 1) * NS + col], g);
                b = lz_fmaf(w, slot[(FL::OUT + 2) * NS + col], b);
                cnt++;
                if (T < F.T_thresh) { cut = true; break; }           // the samples staged behind it are dropped
            }
            // (kk <= cap - count: the cap can only be reached by the last staged sample)
            if (cut || cnt >= cap || left) {
                lzf_ray_end(OUT, ph2, ray, cut ? LZF_END_T : (cnt >= cap ? LZF_END_CAP : LZF_END_BOX), cnt, cnt, t, ws, d, r, g, b, 0.0f, 0.0f, 0.0f);
                my_samples += cnt - cnt_base;
                sloti[NF_RAY * NS + lane] = -1;
            } else {
                slot[NF_WS * NS + lane] = ws; slot[NF_D * NS + lane] = d;
                slot[NF_R * NS + lane] = r; slot[NF_G * NS + lane] = g; slot[NF_B * NS + lane] = b;
                sloti[NF_CNT * NS + lane] = cnt;
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
#define LZNF_SPP_VARIANTS(X, SS) X(0, float, SS, 0) X(1, __half, SS, 1) X(0, __half, SS, 2)
#define LZNF_SPP_ALL(X) LZNF_SPP_VARIANTS(X, 2) LZNF_SPP_VARIANTS(X, 4) LZNF_SPP_VARIANTS(X, 8) LZNF_SPP_VARIANTS(X, 16)

static int lznf_spp_index(uint32_t S) { return S == 2 ? 0 : (S == 4 ? 1 : (S == 8 ? 2 : 3)); }

// workgroups of a kernel a CU holds at a time, asked from the runtime once per device and instantiation (as lznf_wg_per_cu)
static int lznf_spp_wg_per_cu(int variant, uint32_t S) {
    static std::mutex mu;
    static int cache[64][3][4] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 1;
    std::lock_guard<std::mutex> lock(mu);
    int& c = cache[dev][variant][lznf_spp_index(S)];
    if (c <= 0) {
        int n = 0;
        hipError_t e = hipErrorInvalidValue;
#define LZNF_X(PREC, TT, SS, V) if (variant == V && S == SS) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, lz_k_ngp_frame_spp<PREC, TT, SS>, LZNF_WG, 0);
        LZNF_SPP_ALL(LZNF_X)
#undef LZNF_X
        c = (e == hipSuccess && n >= 1) ? n : 1;
    }
    return c;
}

void lznf_spp_launch(int variant, uint32_t S, uint32_t N, const LzNgpFrameArgs& a, const LzFrameK& K, hipStream_t st) {
    const uint32_t columns = variant == 1 ? 32 : 16;
    // no more workgroups than there are groups of S columns for one slice per wave
    uint32_t grid = lz_div_up((uint64_t)N * S, (uint64_t)columns * LZNF_WAVES);
    const uint32_t cap = (uint32_t)lz_cu_count() * (uint32_t)lznf_spp_wg_per_cu(variant, S);
    grid = grid < 1 ? 1 : (grid > cap ? cap : grid);
#define LZNF_X(PREC, TT, SS, V) if (variant == V && S == SS) hipLaunchKernelGGL((lz_k_ngp_frame_spp<PREC, TT, SS>), dim3(grid), dim3(LZNF_WG), 0, st, a, K);
    LZNF_SPP_ALL(LZNF_X)
#undef LZNF_X
}

// steps_per_pass = 0.  S is doubled while the groups (N S columns) still fit the columns of the waves the chip holds at a time -- CUs x
// workgroups per CU x 4 waves x 16 or 32: more groups than that only queue, and until then a larger S means more workgroups per CU to hide
// a wave's gather latency behind, and 1 / S of the dependent passes.  So S = 1 whenever the rays fill half of those columns: a 256^2 frame
// runs lz_k_ngp_frame.  From S = 8 on, one step back when half of S already gives every CU a full workgroup: the leader marches its S
// samples serially, which then costs more than the further workgroups bring.  And S <= max_steps / 2: under a short cap a longer group
// leaves its columns empty on every ray.
// (profiles/cfg2_spp_sweep.json, MI355X, all-ones occupancy, configurations alternated in one process, three rounds, ms of the frame at
// S = 1 / 2 / 4 / 8 / 16, max_steps 128 -- f32 tables + f32 head, 3 workgroups per CU: 32^2 0.485 / 0.298 / 0.199 / 0.152 / 0.137, 64^2
// 0.484 / 0.294 / 0.215 / 0.238 / 0.305, 128^2 0.484 / 0.429 / 0.537 / 0.610 / 0.767, 256^2 1.044 / 1.082 / 1.317 / 1.663 / 2.458; half
// tables + f16 head, 2 per CU: 32^2 0.621 / 0.371 / 0.238 / 0.169 / 0.138, 64^2 0.581 / 0.348 / 0.230 / 0.178 / 0.202, 128^2 0.554 / 0.355 /
// 0.317 / 0.377 / 0.510, 256^2 0.692 / 0.773 / 0.891 / 1.149 / 1.648; half tables + f32 head: the first's fastest S, its 64^2 a tie of S = 4
// and 8.  The rule picks the fastest S in all twelve cells.  max_steps 16: 32^2 f32 0.127 / 0.089 / 0.071 / 0.065 / 0.073, hence the
// bound by max_steps; there the rule is within 0.004 ms of the fastest S in every cell.)
uint32_t lznf_spp_auto(int variant, uint32_t N, uint32_t max_steps) {
    const uint64_t per_wg = (uint64_t)LZNF_WAVES * (variant == 1 ? 32 : 16), n_cu = (uint64_t)lz_cu_count();
    uint32_t S = 1;
    while (S < 16 && 2 * S <= max_steps / 2 && (uint64_t)N * (2 * S) <= n_cu * (uint64_t)lznf_spp_wg_per_cu(variant, 2 * S) * per_wg) S *= 2;
    if (S >= 8 && (uint64_t)N * (S / 2) >= n_cu * per_wg) S /= 2;
    return S;
}
