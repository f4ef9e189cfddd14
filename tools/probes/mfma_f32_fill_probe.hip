// Do vector instructions hide beside f32 MFMAs?  A loop of four independent v_mfma_f32_16x16x4_f32 accumulators with F independent
// v_fma_f32 (or v_pk_fma_f32) placed between consecutive MFMAs; cycles per MFMA from s_memtime around the loop, on 256 workgroups of 256
// threads (one wave per SIMD) and of 1024 threads (four waves per SIMD, the frame kernels' occupancy).  A 16x16x4 f32 MFMA occupies the
// matrix pipe for 32 cycles: a filler is hidden while the figure stays at 32 per SIMD, and costs its issue once it rises.
//   hipcc --offload-arch=gfx950 -O3 -ffp-contract=off tools/probes/mfma_f32_fill_probe.hip -o /tmp/mfma_f32_fill_probe && /tmp/mfma_f32_fill_probe
// prints one JSON object: per configuration the median wave's cycles per MFMA, that figure per SIMD (divided by the waves of a SIMD), and
// the fastest and slowest wave's per SIMD.  At four waves per SIMD the oldest wave wins the matrix pipe, so the waves of a SIMD finish one
// after the other: the slowest wave's figure ("max") is what the SIMD needs per MFMA, the fastest's ("min") is a wave running as if alone.
// The loop body is volatile inline assembly: MFMA, F fillers, four times, in that order in the ISA.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <vector>

typedef float f4 __attribute__((ext_vector_type(4)));
typedef float f2 __attribute__((ext_vector_type(2)));

template <int F, bool PK>
__global__ void __launch_bounds__(1024) k_fill(const float* __restrict__ in, uint32_t iters, unsigned long long* __restrict__ ticks, float* __restrict__ out) {
    const float a = in[threadIdx.x & 63], b = in[64 + (threadIdx.x & 63)], m = in[128], c = in[129];
    f4 acc[4];
#pragma unroll
    for (int i = 0; i < 4; i++) acc[i] = f4{a, b, a, b};
    float x[8];
    f2 y[2];
#pragma unroll
    for (int j = 0; j < 8; j++) x[j] = a + (float)j;
    y[0] = f2{a, b};
    y[1] = f2{b, a};
    const f2 m2 = {m, m}, c2 = {c, c};
    __builtin_amdgcn_s_waitcnt(0);
    const unsigned long long t0 = __builtin_amdgcn_s_memtime();
    // every instruction of the body is a volatile asm statement: the compiler keeps their order and can neither fold the filler chains
    // nor pack them.  No operand of a filler is an MFMA register, and an accumulator returns only with the fourth MFMA after its own
#pragma unroll 1
    for (uint32_t it = 0; it < iters; it++) {
#pragma unroll
        for (int i = 0; i < 4; i++) {
            asm volatile("v_mfma_f32_16x16x4_f32 %0, %1, %2, %0" : "+v"(acc[i]) : "v"(a), "v"(b));
            if constexpr (PK) {
#pragma unroll
                for (int j = 0; j < F; j++) asm volatile("v_pk_fma_f32 %0, %0, %1, %2" : "+v"(y[j]) : "v"(m2), "v"(c2));
            } else {
#pragma unroll
                for (int j = 0; j < F; j++) asm volatile("v_fma_f32 %0, %0, %1, %2" : "+v"(x[j]) : "v"(m), "v"(c));
            }
        }
    }
    asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");     // the last MFMAs' results land before anything reads them
    __builtin_amdgcn_s_waitcnt(0);
    const unsigned long long t1 = __builtin_amdgcn_s_memtime();
    float s = 0.0f;
#pragma unroll
    for (int i = 0; i < 4; i++) s += acc[i][0] + acc[i][1] + acc[i][2] + acc[i][3];
#pragma unroll
    for (int j = 0; j < 8; j++) s += x[j];
    s += y[0][0] + y[0][1] + y[1][0] + y[1][1];
    if ((threadIdx.x & 63) == 0) ticks[blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)] = t1 - t0;
    if (s == 123.456f) out[0] = s;      // never true: keeps the arithmetic
}

struct Cfg { const char* filler; int F; void (*k)(const float*, uint32_t, unsigned long long*, float*); };

int main() {
    const Cfg cfgs[] = {{"v_fma_f32", 0, k_fill<0, false>}, {"v_fma_f32", 1, k_fill<1, false>}, {"v_fma_f32", 2, k_fill<2, false>},
                        {"v_fma_f32", 4, k_fill<4, false>}, {"v_fma_f32", 6, k_fill<6, false>}, {"v_fma_f32", 8, k_fill<8, false>},
                        {"v_pk_fma_f32", 1, k_fill<1, true>}, {"v_pk_fma_f32", 2, k_fill<2, true>}};
    const uint32_t iters = 4096, blocks = 256;
    float h_in[130];
    for (int i = 0; i < 128; i++) h_in[i] = 0.001f * (float)(i % 7);
    h_in[128] = 0.5f;       // the fillers converge (x <- x / 2 + c): no overflow, no denormals
    h_in[129] = 0.25f;
    float *d_in, *d_out;
    unsigned long long* d_t;
    if (hipMalloc(&d_in, sizeof(h_in)) != hipSuccess || hipMalloc(&d_out, 4) != hipSuccess || hipMalloc(&d_t, blocks * 16 * 8) != hipSuccess) {
        fprintf(stderr, "no device memory\n");
        return 1;
    }
    (void)hipMemcpy(d_in, h_in, sizeof(h_in), hipMemcpyHostToDevice);
    printf("{\"mfma\": \"v_mfma_f32_16x16x4_f32\", \"accumulators\": 4, \"iterations\": %u, \"workgroups\": %u, \"rows\": [\n", iters, blocks);
    bool first = true;
    for (int threads : {256, 1024}) {
        const int waves = blocks * threads / 64, per_simd = threads / 256;
        for (const Cfg& c : cfgs) {
            std::vector<unsigned long long> t(waves);
            for (int rep = 0; rep < 3; rep++) hipLaunchKernelGGL(c.k, dim3(blocks), dim3(threads), 0, 0, d_in, iters, d_t, d_out);   // the last launch counts
            if (hipDeviceSynchronize() != hipSuccess) {
                fprintf(stderr, "launch failed\n");
                return 1;
            }
            (void)hipMemcpy(t.data(), d_t, waves * 8, hipMemcpyDeviceToHost);
            std::sort(t.begin(), t.end());
            const double med = (double)t[waves / 2] / (4.0 * iters);
            printf("%s {\"threads\": %d, \"waves_per_simd\": %d, \"filler\": \"%s\", \"fillers_per_gap\": %d, \"wave_cycles_per_mfma\": %.2f, "
                   "\"simd_cycles_per_mfma\": %.2f, \"min\": %.2f, \"max\": %.2f}",
                   first ? " " : ",\n ", threads, per_simd, c.filler, c.F, med, med / per_simd, (double)t[0] / (4.0 * iters) / per_simd,
                   (double)t[waves - 1] / (4.0 * iters) / per_simd);
            first = false;
        }
    }
    printf("\n]}\n");
    return 0;
}
