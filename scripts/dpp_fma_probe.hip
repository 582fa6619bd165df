// Issue cost of v_fmac_f64_dpp (row_newbcast) against plain v_fmac_f64 on gfx950.
// One workgroup on one CU; eight independent accumulators per lane, no memory traffic in the timed loop.
// 256 threads = one wave per SIMD, 768 threads = three waves per SIMD.
// A stand-alone program: hipcc --offload-arch=gfx950 -O3 -std=c++17 -o dpp_fma_probe scripts/dpp_fma_probe.hip
// Prints one JSON line per form and occupancy (profiles/r10_a_dpp_fma_probe.jsonl).
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include <algorithm>

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); std::exit(2); } } while (0)

constexpr int ITER = 2000, UNROLL = 4;      // 8 * UNROLL FMAs per trip

#define FMA_PLAIN(a) asm volatile("v_fmac_f64 %0, %1, %2" : "+v"(a) : "v"(d), "v"(x))
#define FMA_DPP(a, L) asm volatile("v_fmac_f64_dpp %0, %1, %2 row_newbcast:" #L " row_mask:0xf bank_mask:0xf" : "+v"(a) : "v"(d), "v"(x))

template <int MODE>
__global__ void __launch_bounds__(768) probe(double* out, long long* ticks, const double* in)
{
    double d = in[threadIdx.x & 63], x = in[64 + (threadIdx.x & 63)];
    double a0 = 0, a1 = 0, a2 = 0, a3 = 0, a4 = 0, a5 = 0, a6 = 0, a7 = 0;
    __syncthreads();
    const long long t0 = clock64();
    for (int it = 0; it < ITER; ++it) {
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            if (MODE == 0) {
                FMA_PLAIN(a0); FMA_PLAIN(a1); FMA_PLAIN(a2); FMA_PLAIN(a3);
                FMA_PLAIN(a4); FMA_PLAIN(a5); FMA_PLAIN(a6); FMA_PLAIN(a7);
            } else {
                FMA_DPP(a0, 0); FMA_DPP(a1, 3); FMA_DPP(a2, 5); FMA_DPP(a3, 7);
                FMA_DPP(a4, 8); FMA_DPP(a5, 11); FMA_DPP(a6, 13); FMA_DPP(a7, 15);
            }
        }
    }
    const long long t1 = clock64();
    out[threadIdx.x] = a0 + a1 + a2 + a3 + a4 + a5 + a6 + a7;
    if ((threadIdx.x & 63) == 0) ticks[threadIdx.x >> 6] = t1 - t0;
}

template <int MODE>
static void run(const char* name, int threads, double* out, long long* ticks, const double* in)
{
    const int nw = threads / 64;
    std::vector<long long> h(nw);
    std::vector<double> med;
    float best_ms = 1e30f;
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0)); CHECK(hipEventCreate(&e1));
    for (int rep = 0; rep < 7; ++rep) {
        CHECK(hipEventRecord(e0));
        hipLaunchKernelGGL(probe<MODE>, dim3(1), dim3(threads), 0, 0, out, ticks, in);
        CHECK(hipEventRecord(e1));
        CHECK(hipDeviceSynchronize());
        float ms; CHECK(hipEventElapsedTime(&ms, e0, e1));
        best_ms = std::min(best_ms, ms);
        CHECK(hipMemcpy(h.data(), ticks, sizeof(long long) * nw, hipMemcpyDeviceToHost));
        med.push_back((double)*std::max_element(h.begin(), h.end()));
    }
    std::sort(med.begin(), med.end());
    const double nfma = (double)ITER * UNROLL * 8;
    // per wave: ticks of clock64 per FMA; per SIMD: the same divided by the waves sharing the SIMD
    std::printf("{\"probe\": \"%s\", \"waves_per_simd\": %d, \"clock64_ticks_per_fma_per_wave\": %.4f, "
                "\"clock64_ticks_per_fma_per_simd\": %.4f, \"event_ns_per_fma_per_simd\": %.4f}\n",
                name, nw / 4, med[3] / nfma, med[3] / nfma / (nw / 4), best_ms * 1e6 / nfma / (nw / 4));
}

int main()
{
    double *out, *in; long long* ticks;
    CHECK(hipMalloc(&out, 768 * sizeof(double)));
    CHECK(hipMalloc(&in, 128 * sizeof(double)));
    CHECK(hipMalloc(&ticks, 12 * sizeof(long long)));
    std::vector<double> hin(128);
    for (int i = 0; i < 128; ++i) hin[i] = 1.0 / (i + 3);
    CHECK(hipMemcpy(in, hin.data(), 128 * sizeof(double), hipMemcpyHostToDevice));
    for (int threads : {256, 768}) {
        run<0>("v_fmac_f64", threads, out, ticks, in);
        run<1>("v_fmac_f64_dpp row_newbcast", threads, out, ticks, in);
    }
    // the DPP form computes what it should: acc = sum over the eight lanes' broadcasts
    std::vector<double> ho(64);
    CHECK(hipMemcpy(ho.data(), out, 64 * sizeof(double), hipMemcpyDeviceToHost));
    std::printf("{\"lane0_sum\": %.17g, \"lane17_sum\": %.17g}\n", ho[0], ho[17]);
    return 0;
}
