// How do the waves of a SIMD share issue between f32 MFMAs and other vector work?  mfma_f32_fill_probe.hip ran four IDENTICAL waves with
// v_fma_f32 fillers inside each wave's own MFMA stream; this probe gives the waves of a SIMD different roles and other filler kinds.
//   hipcc --offload-arch=gfx950 -O3 -ffp-contract=off tools/probes/mfma_f32_mix_probe.hip -o tools/probes/mfma_f32_mix_probe
//   tools/probes/mfma_f32_mix_probe [out.json]          (default: profiles/r8_mfma_f32_mix_probe.json)
// One workgroup per CU (96 KB of LDS each, so that two cannot share one), 1 - 4 waves per SIMD; a wave's SIMD is read from HW_ID, its age
// rank on the SIMD is its order in the workgroup (wave index / 4: dispatch order is not guaranteed by the architecture).  Every measured
// loop is bracketed by s_memtime behind a workgroup barrier; every instruction of a loop body is volatile inline assembly.
//
// Roles.  M: independent v_mfma_f32_16x16x4_f32 on four accumulators, 32 matrix-pipe cycles each.  V(kind): fillers of one kind, as an
// independent stream (8 registers in turn) or as a dependent chain (one register): v_fma_f32; v_add_u32 / v_and_b32 in turn; v_max_i32;
// v_mul_u32_u24 / v_mad_u32_u24 in turn; v_cndmask_b32; v_exp_f32; ds_read_b128 followed by its s_waitcnt (chain: the address of a read is
// the first word of the read before it, wait for all; stream: wait until at most three are outstanding); and v_max_f32 and v_med3_f32,
// the float forms a ReLU could take instead of the slice's v_max_i32.
//
// Arrangements.
//  (a) "mix": three M waves and one V wave on every SIMD.  The V wave issues a fixed number of fillers and raises a flag in LDS; the M waves
//      run until they see it (or to a fixed cap), so both roles are active through the whole window.  V at priority 0 or 2, V the first- or
//      the last-dispatched wave of the four.  Reported per SIMD (median over SIMDs): the window in cycles, the MFMAs the three M waves
//      issued in it, cycles per MFMA (window / MFMAs: 32 = the fillers were free), cycles per filler (window / fillers), and the fillers'
//      cost on the matrix pipe, (window - 32 MFMAs) / fillers, and whether the M waves stopped on the flag (if they ran to the cap the V
//      wave outlasted them and the window holds a tail of it alone).  Baselines: three M waves alone; one V wave per SIMD alone.
//  (b) "burst": identical waves (one and four per SIMD) alternate runs of R MFMAs with bursts of B fillers, B / R = 2.1 (the f32 frame
//      kernel's 720 : 337), R = 1, 4, 16, 64, 337.  Cycles per MFMA and SIMD = the SIMD's span / all its waves' MFMAs.
//  (c) "burst_young": (b) at four waves per SIMD with the second-dispatched half of the workgroup at s_setprio 1 throughout.
// Sizes are fixed; no loop depends on another wave for its end (the M waves of (a) stop at the cap at the latest).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <vector>

typedef float f4 __attribute__((ext_vector_type(4)));
typedef uint32_t u4 __attribute__((ext_vector_type(4)));

enum { K_FMA, K_ADDAND, K_MAXI, K_MUL24, K_CND, K_EXP, K_DS, K_MAXF, K_MED3, K_COUNT };
static const char* const kKindName[K_COUNT] = {"v_fma_f32", "v_add_u32/v_and_b32", "v_max_i32", "v_mul_u32_u24/v_mad_u32_u24", "v_cndmask_b32",
                                               "v_exp_f32", "ds_read_b128+s_waitcnt", "v_max_f32", "v_med3_f32"};
constexpr int LDS_ENTRIES = 6144;      // 96 KB: one workgroup per CU

struct Fill {
    float x[8];
    uint32_t u[8];
    u4 d[4];
    uint32_t addr;
    float m, c;
    uint32_t ku, kand;
    unsigned long long mask;
};

// filler number j of a burst (j is a constant once the caller's loop is unrolled)
template <int KIND, bool DEP>
__device__ __forceinline__ void filler(Fill& f, int j) {
    const int r = DEP ? 0 : (j & 7);
    if constexpr (KIND == K_FMA) {
        asm volatile("v_fma_f32 %0, %0, %1, %2" : "+v"(f.x[r]) : "v"(f.m), "v"(f.c));       // x <- x / 2 + 1 / 4: converges
    } else if constexpr (KIND == K_ADDAND) {
        if (j & 1) asm volatile("v_and_b32 %0, %0, %1" : "+v"(f.u[r]) : "v"(f.kand));
        else asm volatile("v_add_u32 %0, %0, %1" : "+v"(f.u[r]) : "v"(f.ku));
    } else if constexpr (KIND == K_MAXI) {
        asm volatile("v_max_i32 %0, %0, %1" : "+v"(f.u[r]) : "v"(f.ku));
    } else if constexpr (KIND == K_MUL24) {
        if (j & 1) asm volatile("v_mad_u32_u24 %0, %0, %1, %2" : "+v"(f.u[r]) : "v"(f.ku), "v"(f.kand));
        else asm volatile("v_mul_u32_u24 %0, %0, %1" : "+v"(f.u[r]) : "v"(f.ku));
    } else if constexpr (KIND == K_CND) {
        asm volatile("v_cndmask_b32_e64 %0, %0, %1, %2" : "+v"(f.u[r]) : "v"(f.ku), "s"(f.mask));
    } else if constexpr (KIND == K_MAXF) {
        asm volatile("v_max_f32 %0, %0, %1" : "+v"(f.x[r]) : "v"(f.c));
    } else if constexpr (KIND == K_MED3) {
        asm volatile("v_med3_f32 %0, %0, 0, %1" : "+v"(f.x[r]) : "v"(f.c));
    } else if constexpr (KIND == K_EXP) {
        asm volatile("v_exp_f32_e64 %0, -%0" : "+v"(f.x[r]));                                 // x <- 2^-x: converges to 0.641
    } else {
        if constexpr (DEP) {
            u4 t;
            asm volatile("ds_read_b128 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=&v"(t) : "v"(f.addr));
            f.addr = t[0];                     // every entry's first word is its own address: the chain stays where it is
            f.d[0] = t;
        } else {
            asm volatile("ds_read_b128 %0, %1\n\ts_waitcnt lgkmcnt(3)" : "=&v"(f.d[j & 3]) : "v"(f.addr));
        }
    }
}

__device__ __forceinline__ void mfma(f4& acc, float a, float b) { asm volatile("v_mfma_f32_16x16x4_f32 %0, %1, %2, %0" : "+v"(acc) : "v"(a), "v"(b)); }

__device__ __forceinline__ void fill_init(Fill& f, const float* __restrict__ in, u4* lds, int lane, float a, float b) {
#pragma unroll
    for (int j = 0; j < 8; j++) {
        f.x[j] = a + 0.125f * (float)j;
        f.u[j] = (uint32_t)(lane * 8 + j);
    }
    f.m = in[128];
    f.c = in[129];
    f.ku = 3u + (uint32_t)(a > 1.0f);        // (3: a is below 1)
    f.kand = 0x00ffffffu;
    f.mask = 0x5555555555555555ull + (unsigned long long)(blockDim.x > 4096u);     // wave-uniform: a scalar register pair
    f.addr = (uint32_t)(size_t)&lds[lane];     // the low half of a generic LDS address is the LDS offset
#pragma unroll
    for (int k = 0; k < 4; k++) f.d[k] = u4{0, 0, 0, 0};
}

__device__ __forceinline__ float fill_sum(const Fill& f) {
    float s = 0.0f;
#pragma unroll
    for (int j = 0; j < 8; j++) s += f.x[j] + (float)f.u[j];
#pragma unroll
    for (int k = 0; k < 4; k++) s += (float)(f.d[k][0] ^ f.d[k][1] ^ f.d[k][2] ^ f.d[k][3]);
    return s + (float)f.addr;
}

struct WaveRec { unsigned long long t0, t1; uint32_t simd, mfmas; };

__device__ __forceinline__ uint32_t simd_id() { return __builtin_amdgcn_s_getreg(4 | (4 << 6) | (1 << 11)); }   // HW_ID bits 5:4

__device__ __forceinline__ void prologue(u4* lds, int* flag) {     // flag[4]: one per SIMD
    for (uint32_t i = threadIdx.x; i < 64; i += blockDim.x) lds[i] = u4{(uint32_t)(size_t)&lds[i], i, i, i};
    if (threadIdx.x < 4) flag[threadIdx.x] = 0;
    if (threadIdx.x == 0) {
        lds[LDS_ENTRIES - 1] = u4{0, 0, 0, 0};      // (the whole array stays allocated)
    }
    __syncthreads();
}

// (a): the waves of rank v_rank (wave index / 4) are V, the others M; v_rank = -1: M only; v_rank = 4: every wave V (run at one wave per SIMD).
// A V wave raises the flag of its own SIMD (HW_ID), which that SIMD's M waves poll once per 64 MFMAs.
template <int KIND, bool DEP>
__global__ void __launch_bounds__(1024) k_mix(const float* __restrict__ in, int v_rank, int v_prio, uint32_t v_iters, uint32_t m_cap,
                                              WaveRec* __restrict__ rec, float* __restrict__ out) {
    __shared__ u4 lds[LDS_ENTRIES];
    __shared__ int flag[4];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const float a = in[lane], b = in[64 + lane];
    f4 acc[4];
#pragma unroll
    for (int i = 0; i < 4; i++) acc[i] = f4{a, b, a, b};
    Fill f;
    fill_init(f, in, lds, lane, a, b);
    prologue(lds, flag);
    const bool is_v = v_rank == 4 || (wave >> 2) == v_rank;       // wave-uniform: `wave` is a scalar
    uint32_t mfmas = 0;
    const uint32_t simd = simd_id();
    __builtin_amdgcn_s_waitcnt(0);
    unsigned long long t0, t1;
    if (is_v) {
        if (v_prio == 2) __builtin_amdgcn_s_setprio(2);
        t0 = __builtin_amdgcn_s_memtime();
#pragma unroll 1
        for (uint32_t it = 0; it < v_iters; it++) {
#pragma unroll
            for (int j = 0; j < 64; j++) filler<KIND, DEP>(f, j);
        }
        __builtin_amdgcn_s_waitcnt(0);
        t1 = __builtin_amdgcn_s_memtime();
        __builtin_amdgcn_s_setprio(0);
        if (lane == 0) atomicAdd(&flag[simd_id()], 1);
    } else {
        t0 = __builtin_amdgcn_s_memtime();
#pragma unroll 1
        for (uint32_t it = 0; it < m_cap; it++) {
#pragma unroll
            for (int i = 0; i < 64; i++) mfma(acc[i & 3], a, b);
            mfmas += 64;
            if (__builtin_amdgcn_readfirstlane(__hip_atomic_load(&flag[simd], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) > 0) break;
        }
        asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");
        __builtin_amdgcn_s_waitcnt(0);
        t1 = __builtin_amdgcn_s_memtime();
    }
    float s = fill_sum(f);
#pragma unroll
    for (int i = 0; i < 4; i++) s += acc[i][0] + acc[i][1] + acc[i][2] + acc[i][3];
    if (lane == 0) rec[blockIdx.x * (blockDim.x >> 6) + wave] = WaveRec{t0, t1, simd_id(), mfmas};
    if (s == 123.456f) out[0] = s;      // never true: keeps the arithmetic
}

// (b), (c): every wave alternates R MFMAs and B fillers, `reps` times; waves of the second-dispatched half run at priority young_prio
template <int KIND, bool DEP, int R, int B>
__global__ void __launch_bounds__(1024) k_burst(const float* __restrict__ in, uint32_t reps, int young_prio, WaveRec* __restrict__ rec,
                                                float* __restrict__ out) {
    __shared__ u4 lds[LDS_ENTRIES];
    __shared__ int flag[4];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const float a = in[lane], b = in[64 + lane];
    f4 acc[4];
#pragma unroll
    for (int i = 0; i < 4; i++) acc[i] = f4{a, b, a, b};
    Fill f;
    fill_init(f, in, lds, lane, a, b);
    prologue(lds, flag);
    if (young_prio == 1 && 2 * wave >= (int)(blockDim.x >> 6)) __builtin_amdgcn_s_setprio(1);      // a scalar branch: `wave` is a scalar
    __builtin_amdgcn_s_waitcnt(0);
    const unsigned long long t0 = __builtin_amdgcn_s_memtime();
#pragma unroll 1
    for (uint32_t it = 0; it < reps; it++) {
#pragma unroll
        for (int i = 0; i < R; i++) mfma(acc[i & 3], a, b);
#pragma unroll
        for (int j = 0; j < B; j++) filler<KIND, DEP>(f, j);
    }
    asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");
    __builtin_amdgcn_s_waitcnt(0);
    const unsigned long long t1 = __builtin_amdgcn_s_memtime();
    __builtin_amdgcn_s_setprio(0);
    float s = fill_sum(f);
#pragma unroll
    for (int i = 0; i < 4; i++) s += acc[i][0] + acc[i][1] + acc[i][2] + acc[i][3];
    if (lane == 0) rec[blockIdx.x * (blockDim.x >> 6) + wave] = WaveRec{t0, t1, simd_id(), reps * R};
    if (s == 123.456f) out[0] = s;
}

typedef void (*MixFn)(const float*, int, int, uint32_t, uint32_t, WaveRec*, float*);
typedef void (*BurstFn)(const float*, uint32_t, int, WaveRec*, float*);
constexpr int kR[5] = {1, 4, 16, 64, 337}, kB[5] = {2, 8, 34, 134, 720};
struct Kind { int kind; bool dep; MixFn mix; BurstFn burst[5]; };
#define KIND_ROW(K, D) {K, D, k_mix<K, D>, {k_burst<K, D, 1, 2>, k_burst<K, D, 4, 8>, k_burst<K, D, 16, 34>, k_burst<K, D, 64, 134>, k_burst<K, D, 337, 720>}}
static const Kind kKinds[] = {KIND_ROW(K_FMA, false), KIND_ROW(K_FMA, true), KIND_ROW(K_ADDAND, false), KIND_ROW(K_ADDAND, true),
                              KIND_ROW(K_MAXI, false), KIND_ROW(K_MAXI, true), KIND_ROW(K_MUL24, false), KIND_ROW(K_MUL24, true),
                              KIND_ROW(K_CND, false), KIND_ROW(K_CND, true), KIND_ROW(K_EXP, false), KIND_ROW(K_EXP, true),
                              KIND_ROW(K_DS, false), KIND_ROW(K_DS, true), KIND_ROW(K_MAXF, false), KIND_ROW(K_MAXF, true),
                              KIND_ROW(K_MED3, false), KIND_ROW(K_MED3, true)};

constexpr uint32_t BLOCKS = 256;
static float* d_in;
static float* d_out;
static WaveRec* d_rec;

static double median(std::vector<double>& v) {
    if (v.empty()) return 0.0;
    std::sort(v.begin(), v.end());
    return v[v.size() / 2];
}

struct SimdStat { double window, mfmas, v_cycles; int simds, irregular; };

// per SIMD of every workgroup: the span from its first wave's start to its last wave's end, its M waves' MFMAs, its V wave's own time
static bool collect(int threads, int v_rank, SimdStat& st) {
    const int wpb = threads / 64, wps = wpb / 4;
    if (hipDeviceSynchronize() != hipSuccess) {
        fprintf(stderr, "launch failed\n");
        return false;
    }
    std::vector<WaveRec> r(BLOCKS * wpb);
    (void)hipMemcpy(r.data(), d_rec, r.size() * sizeof(WaveRec), hipMemcpyDeviceToHost);
    std::vector<double> win, mf, vc;
    st.irregular = 0;
    for (uint32_t blk = 0; blk < BLOCKS; blk++)
        for (uint32_t simd = 0; simd < 4; simd++) {
            unsigned long long lo = ~0ull, hi = 0, v = 0;
            double m = 0;
            int n = 0;
            for (int w = 0; w < wpb; w++) {
                const WaveRec& x = r[blk * wpb + w];
                if (x.simd != simd) continue;
                n++;
                lo = std::min(lo, x.t0);
                hi = std::max(hi, x.t1);
                const bool is_v = v_rank == 4 || (w >> 2) == v_rank;
                if (is_v) v = x.t1 - x.t0;
                m += x.mfmas;
            }
            if (n != wps) { st.irregular++; continue; }      // the waves were not dealt out evenly: left out
            win.push_back((double)(hi - lo));
            mf.push_back(m);
            vc.push_back((double)v);
        }
    st.simds = (int)win.size();
    st.window = median(win);
    st.mfmas = median(mf);
    st.v_cycles = median(vc);
    return true;
}

int main(int argc, char** argv) {
    const char* path = argc > 1 ? argv[1] : "profiles/r8_mfma_f32_mix_probe.json";
    float h_in[130];
    for (int i = 0; i < 128; i++) h_in[i] = 0.001f * (float)(i % 7);
    h_in[128] = 0.5f;
    h_in[129] = 0.25f;
    if (hipMalloc(&d_in, sizeof(h_in)) != hipSuccess || hipMalloc(&d_out, 4) != hipSuccess || hipMalloc(&d_rec, BLOCKS * 16 * sizeof(WaveRec)) != hipSuccess) {
        fprintf(stderr, "no device memory\n");
        return 1;
    }
    (void)hipMemcpy(d_in, h_in, sizeof(h_in), hipMemcpyHostToDevice);
    FILE* o = fopen(path, "w");
    if (!o) {
        fprintf(stderr, "cannot write %s\n", path);
        return 1;
    }
    const uint32_t m_cap = 256;            // x 64 MFMAs: at most 16 384 per M wave, 1.6 M cycles for the three of a SIMD
    fprintf(o, "{\"mfma\": \"v_mfma_f32_16x16x4_f32\", \"workgroups\": %u, \"lds_bytes_per_workgroup\": %d, \"clock\": \"s_memtime\",\n", BLOCKS, LDS_ENTRIES * 16);
    // ---------------- (a) ----------------
    SimdStat st;
    hipLaunchKernelGGL(kKinds[0].mix, dim3(BLOCKS), dim3(1024), 0, 0, d_in, -1, 0, 0u, m_cap, d_rec, d_out);     // warm-up
    hipLaunchKernelGGL(kKinds[0].mix, dim3(BLOCKS), dim3(768), 0, 0, d_in, -1, 0, 0u, m_cap, d_rec, d_out);
    if (!collect(768, -1, st)) return 1;
    fprintf(o, " \"mix_baseline_three_M_waves\": {\"mfmas_per_simd\": %.0f, \"window_cycles\": %.0f, \"cycles_per_mfma\": %.3f, \"simds\": %d, \"irregular_simds\": %d},\n",
            st.mfmas, st.window, st.window / st.mfmas, st.simds, st.irregular);
    fprintf(o, " \"mix\": [\n");
    bool first = true;
    for (const Kind& k : kKinds) {
        // x 64 fillers: few enough that the V wave is done well inside the M waves' cap even at 200 cycles per filler, so that the M
        // waves stop on its flag and both roles are active through the whole window
        const uint32_t v_iters = k.kind == K_DS ? 16 : 64;
        const double fillers = 64.0 * v_iters;
        hipLaunchKernelGGL(k.mix, dim3(BLOCKS), dim3(256), 0, 0, d_in, 4, 0, v_iters, m_cap, d_rec, d_out);
        if (!collect(256, 4, st)) return 1;
        const double alone = st.v_cycles / fillers;
        for (int v_rank : {0, 3})
            for (int v_prio : {0, 2}) {
                hipLaunchKernelGGL(k.mix, dim3(BLOCKS), dim3(1024), 0, 0, d_in, v_rank, v_prio, v_iters, m_cap, d_rec, d_out);
                if (!collect(1024, v_rank, st)) return 1;
                fprintf(o, "%s  {\"filler\": \"%s\", \"chain\": %s, \"v_wave\": \"%s\", \"v_prio\": %d, \"fillers\": %.0f, \"alone_cycles_per_filler\": %.2f, "
                           "\"m_waves_stopped_on_flag\": %s, "
                           "\"v_cycles_per_filler\": %.2f, \"window_cycles\": %.0f, \"mfmas_in_window\": %.0f, \"cycles_per_mfma\": %.3f, "
                           "\"matrix_pipe_cycles_lost_per_filler\": %.3f, \"simds\": %d, \"irregular_simds\": %d}",
                        first ? "" : ",\n", kKindName[k.kind], k.dep ? "true" : "false", v_rank == 0 ? "oldest" : "youngest", v_prio, fillers, alone,
                        st.mfmas < 3.0 * 64.0 * m_cap ? "true" : "false",
                        st.v_cycles / fillers, st.window, st.mfmas, st.window / st.mfmas, (st.window - 32.0 * st.mfmas) / fillers, st.simds, st.irregular);
                first = false;
            }
    }
    fprintf(o, "\n ],\n");
    // ---------------- (b), (c) ----------------
    fprintf(o, " \"burst\": [\n");
    first = true;
    for (const Kind& k : kKinds)
        for (int ri = 0; ri < 5; ri++) {
            const uint32_t reps = 5392 / kR[ri];
            double fig[3];
            int irr = 0;
            const int threads[3] = {256, 1024, 1024}, young[3] = {0, 0, 1};
            for (int c = 0; c < 3; c++) {
                hipLaunchKernelGGL(k.burst[ri], dim3(BLOCKS), dim3(threads[c]), 0, 0, d_in, reps, young[c], d_rec, d_out);
                if (!collect(threads[c], -1, st)) return 1;
                fig[c] = st.window / st.mfmas;
                irr += st.irregular;
            }
            fprintf(o, "%s  {\"filler\": \"%s\", \"chain\": %s, \"R\": %d, \"B\": %d, \"reps\": %u, \"cycles_per_mfma_1_wave\": %.3f, "
                       "\"cycles_per_mfma_4_waves\": %.3f, \"cycles_per_mfma_4_waves_young_prio_1\": %.3f, \"irregular_simds\": %d}",
                    first ? "" : ",\n", kKindName[k.kind], k.dep ? "true" : "false", kR[ri], kB[ri], reps, fig[0], fig[1], fig[2], irr);
            first = false;
        }
    fprintf(o, "\n ]\n}\n");
    fclose(o);
    printf("wrote %s\n", path);
    return 0;
}
