// kern_mp2.hip -- RI-MP2 correlation energy of a converged, density-fitted closed-shell batch.
//
// Everything the stage needs is what the SCF loop leaves on the device: the fitted tensor df_b [naux][npair] (ANY square
// root of the metric gives the same (ia|jb) = sum_P B^P_ia B^P_jb, so the Cholesky fit of kern_df.hip serves as well as
// the symmetric J^{-1/2}), the orbitals C [mu][orbital], their energies eps and the number of kept orbitals nmo (istate).
//
//   mp2_transform_kernel   X_P = C_occ^T B_P C_virt for every auxiliary row P   -> Bia[f][i][P][a], a fastest
//   mp2_pair_kernel        per (fragment, pair i >= j): V1 = Bi^T Bj, V2 = Bj^T Bi (= V1^T) on 16 x 16 tiles, denominators,
//                          one opposite-spin and one same-spin partial per pair
//   mp2_reduce_kernel      the partials of a fragment summed in pair order (no floating-point atomics anywhere:
//                          the result does not depend on scheduling)
//
//   e_os = sum_ij sum_ab V_ab V_ab / D,   e_ss = sum_ij sum_ab V_ab (V_ab - V_ba) / D,   D = e_i + e_j - e_a - e_b,
//   E_corr = e_os + e_ss.
//
// Active occupied orbitals are n_frozen .. nocc-1, virtuals nocc .. nmo-1.  nmo is read per fragment: the orthogonaliser
// drops near-null modes of the overlap, and the columns of C beyond nmo are not orbitals.  The layout of Bia is sized by
// n - nocc for the whole batch; virtual columns a fragment does not have are written as zeros and never meet 1/D.
// Both GEMM stages run on v_mfma_f64_16x16x4_f64: A takes element (row = lane & 15, k = lane >> 4), B takes
// (k = lane >> 4, col = lane & 15), the accumulator register r of a lane is element (row = (lane >> 4) + 4 r, col = lane & 15).
#include "engine.hpp"
#include <algorithm>
#include <cstdio>
#include <cstdlib>

typedef double v4f64 __attribute__((ext_vector_type(4)));

namespace mqc {

constexpr int MP2_NW = 4;             // waves per workgroup of the pair kernel
constexpr int MP2_PF = 20;            // transform: rows of up to 64 x 20 pairs (n <= 50) are prefetched into registers
constexpr int MP2_TW = 8;            // most waves per workgroup of the transform (it launches as many as the LDS holds)

struct Mp2View {
    int nfz, no;                      // frozen orbitals, active occupied orbitals
    int nvpad, napad;                 // n - nocc rounded up to 16, naux rounded up to 4: the padding of Bia holds zeros
    int npairs;                       // no (no + 1) / 2
    int oc, ts;                       // transform: occupied orbitals per pass (multiple of 16), row stride of T in LDS
    double* Bia;                      // [nfrag][no][napad][nvpad]
    double* part;                     // [nfrag][npairs][2]
    double* out;                      // [nfrag][2] = e_os, e_ss
};

// the fragments whose SCF converged with every occupied orbital in place; the others get zeros
__device__ __forceinline__ bool mp2_runs(const BatchView& bv, int f)
{
    return bv.istate[4 * f] == ST_DONE && bv.istate[4 * f + 3] != 0 && bv.istate[4 * f + 2] >= bv.nocc;
}

// Workgroup = (block of auxiliary rows, fragment); every wave owns one row P at a time: the packed row in a wave-private
// LDS buffer, T_P = B_P C_occ [n][occupied pass] next to it (C is streamed from L2: at n = 140 it alone is 157 KB), then
// X_P = T_P^T C_virt straight to Bia.  The row and T belong to one wave, so what orders a lane's LDS writes before the
// other lanes' reads is the wave's own program order (mp2_wave_sync keeps the compiler to it): the waves of a workgroup
// drift apart, and one wave's loads overlap another's matrix-core steps.
// CLDS (the MBE fragment sizes): the active occupied and the virtual columns of C, zero padded to [4 nks][nop + nvpad],
// sit in LDS for the whole workgroup -- with C read from L2 inside the k loops every matrix-core step waited for a load
// (3.7 Tflop/s on the benchmark's dimers).  NPF > 0: rows of at most 64 NPF pairs; the next row is in flight, in
// registers, while this one is transformed.
__device__ __forceinline__ void mp2_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <bool CLDS, int NPF>
__global__ void __launch_bounds__(64 * MP2_TW) mp2_transform_kernel(BatchView bv, Mp2View mv)
{
    extern __shared__ double lds[];
    const int f = blockIdx.y;
    if (!mp2_runs(bv, f)) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = (int)blockDim.x >> 6, lo = lane & 15, hi = lane >> 4;
    const int n = bv.n, na = bv.naux, np = bv.npair, nocc = bv.nocc;
    const int nv = bv.istate[4 * f + 2] - nocc;
    const int nt = (n + 15) >> 4, nks = (n + 3) >> 2, nvt = mv.nvpad >> 4, ts = mv.ts;
    const int nop = (mv.no + 15) & ~15, cs = nop + mv.nvpad;
    const double* __restrict__ Bf = bv.df_b + (size_t)f * na * (size_t)np;
    const double* __restrict__ C = bv.C + (size_t)f * n * n;
    double* __restrict__ Bia = mv.Bia + (size_t)f * mv.no * mv.napad * (size_t)mv.nvpad;
    double* Cs = lds;
    double* rowbuf = lds + (CLDS ? (size_t)4 * nks * cs : 0) + (size_t)wave * ((size_t)np + (size_t)16 * nt * ts);
    double* T = rowbuf + np;
    if (CLDS)
        for (int idx = tid; idx < 4 * nks * cs; idx += (int)blockDim.x) {
            const int mu = idx / cs, c = idx - mu * cs;
            double v = 0.0;
            if (mu < n) {
                if (c < nop) { if (c < mv.no) v = C[(size_t)mu * n + mv.nfz + c]; }
                else if (c - nop < nv) v = C[(size_t)mu * n + nocc + c - nop];
            }
            Cs[idx] = v;
        }
    const int stride = (int)gridDim.x * nw;
    int P = (int)blockIdx.x * nw + wave;
    double nxt[NPF > 0 ? NPF : 1];
    if (NPF > 0 && P < mv.napad) {
#pragma unroll
        for (int k = 0; k < NPF; ++k) { const int idx = lane + 64 * k; nxt[k] = (idx < np && P < na) ? Bf[(size_t)P * np + idx] : 0.0; }
    }
    __syncthreads();                                      // Cs complete: the only workgroup barrier
    for (; P < mv.napad; P += stride) {                   // rows na .. napad-1 are the zero padding of Bia
        if (NPF > 0) {
#pragma unroll
            for (int k = 0; k < NPF; ++k) { const int idx = lane + 64 * k; if (idx < np) rowbuf[idx] = nxt[k]; }
            const int Pn = P + stride;
            if (Pn < mv.napad) {
#pragma unroll
                for (int k = 0; k < NPF; ++k) { const int idx = lane + 64 * k; nxt[k] = (idx < np && Pn < na) ? Bf[(size_t)Pn * np + idx] : 0.0; }
            }
        } else {
            for (int idx = lane; idx < np; idx += 64) rowbuf[idx] = P < na ? Bf[(size_t)P * np + idx] : 0.0;
        }
        mp2_wave_sync();
        for (int i0 = 0; i0 < mv.no; i0 += mv.oc) {
            const int nio = min(mv.oc, mv.no - i0), not_ = (nio + 15) >> 4;
            for (int mt = 0; mt < nt; ++mt) {
                const int mu = 16 * mt + lo;
                const int tri = mu * (mu + 1) / 2;
                for (int ot = 0; ot < not_; ++ot) {
                    const int ii = i0 + 16 * ot + lo;
                    v4f64 acc = (v4f64){0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
                    for (int ks = 0; ks < nks; ++ks) {
                        const int nu = 4 * ks + hi;
                        const double a = (mu < n && nu < n) ? rowbuf[mu >= nu ? tri + nu : nu * (nu + 1) / 2 + mu] : 0.0;
                        const double b = CLDS ? Cs[nu * cs + ii] : (nu < n && ii < mv.no) ? C[(size_t)nu * n + mv.nfz + ii] : 0.0;
                        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
                    }
#pragma unroll
                    for (int r = 0; r < 4; ++r) T[(16 * mt + hi + 4 * r) * ts + 16 * ot + lo] = acc[r];
                }
            }
            mp2_wave_sync();
            for (int ot = 0; ot < not_; ++ot)
                for (int vt = 0; vt < nvt; ++vt) {
                    const int av = 16 * vt + lo;
                    v4f64 acc = (v4f64){0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
                    for (int ks = 0; ks < nks; ++ks) {
                        const int mu = 4 * ks + hi;               // < 16 nt: the rows of T beyond n hold zeros
                        const double a = T[mu * ts + 16 * ot + lo];
                        const double b = CLDS ? Cs[mu * cs + nop + av] : (mu < n && av < nv) ? C[(size_t)mu * n + nocc + av] : 0.0;
                        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
                    }
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int i = i0 + 16 * ot + hi + 4 * r;
                        if (i < mv.no) Bia[((size_t)i * mv.napad + P) * mv.nvpad + av] = acc[r];
                    }
                }
            mp2_wave_sync();                              // T and the row are free for the next pass / row
        }
    }
}

// Wave = (fragment, pair i >= j).  Tiles (ta >= tb) of the virtual-virtual block: V2 of tile (ta, tb) is V1 of tile
// (tb, ta) transposed, so an off-diagonal tile stands for its mirror image as well:
//   os: V_ab^2 + V_ba^2,   ss: V_ab (V_ab - V_ba) + V_ba (V_ba - V_ab) = (V_ab - V_ba)^2.
// A lane reads Bi[P0 + (lane >> 4)][a0 + (lane & 15)]: sixteen consecutive doubles per k-slice.
__global__ void __launch_bounds__(64 * MP2_NW) mp2_pair_kernel(BatchView bv, Mp2View mv)
{
    const int f = blockIdx.y;
    if (!mp2_runs(bv, f)) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lo = lane & 15, hi = lane >> 4;
    const int pair = (int)blockIdx.x * MP2_NW + wave;
    if (pair >= mv.npairs) return;
    int i = (int)((sqrt(8.0 * pair + 1.0) - 1.0) * 0.5);
    while ((i + 1) * (i + 2) / 2 <= pair) ++i;
    while (i * (i + 1) / 2 > pair) --i;
    const int j = pair - i * (i + 1) / 2;
    const int n = bv.n, nocc = bv.nocc, nv = bv.istate[4 * f + 2] - nocc;
    const int nvp = mv.nvpad, nvt = (nv + 15) >> 4;
    const double* __restrict__ eps = bv.eps + (size_t)f * n;
    const double eij = eps[mv.nfz + i] + eps[mv.nfz + j];
    const size_t slab = (size_t)mv.napad * nvp;
    const double* __restrict__ Bi = mv.Bia + ((size_t)f * mv.no + i) * slab + (size_t)hi * nvp + lo;
    const double* __restrict__ Bj = mv.Bia + ((size_t)f * mv.no + j) * slab + (size_t)hi * nvp + lo;
    double eos = 0.0, ess = 0.0;
    for (int ta = 0; ta < nvt; ++ta)
        for (int tb = 0; tb <= ta; ++tb) {
            v4f64 v1 = (v4f64){0.0, 0.0, 0.0, 0.0}, v2 = (v4f64){0.0, 0.0, 0.0, 0.0};
            const double *pia = Bi + 16 * ta, *pja = Bj + 16 * ta, *pib = Bi + 16 * tb, *pjb = Bj + 16 * tb;
#pragma unroll 4
            for (int P0 = 0; P0 < mv.napad; P0 += 4) {
                const size_t off = (size_t)P0 * nvp;
                const double ai = pia[off], aj = pja[off], bi = pib[off], bj = pjb[off];
                v1 = __builtin_amdgcn_mfma_f64_16x16x4f64(ai, bj, v1, 0, 0, 0);
                v2 = __builtin_amdgcn_mfma_f64_16x16x4f64(aj, bi, v2, 0, 0, 0);
            }
            const int b = 16 * tb + lo;
            if (b < nv) {                                  // a padded column has no orbital energy: no 1/D for it
                const double eb = eps[nocc + b];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int a = 16 * ta + hi + 4 * r;
                    if (a < nv) {
                        const double d = 1.0 / (eij - eps[nocc + a] - eb), x = v1[r], y = v2[r];
                        if (ta == tb) { eos += x * x * d; ess += x * (x - y) * d; }
                        else { eos += (x * x + y * y) * d; ess += (x - y) * (x - y) * d; }
                    }
                }
            }
        }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { eos += __shfl_xor(eos, off, 64); ess += __shfl_xor(ess, off, 64); }
    if (lane == 0) {
        const double w = i == j ? 1.0 : 2.0;
        double* p = mv.part + ((size_t)f * mv.npairs + pair) * 2;
        p[0] = w * eos; p[1] = w * ess;
    }
}

__global__ void mp2_reduce_kernel(BatchView bv, Mp2View mv)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= bv.nfrag) return;
    double eos = 0.0, ess = 0.0;
    if (mp2_runs(bv, f)) {
        const double* p = mv.part + (size_t)f * mv.npairs * 2;
        for (int k = 0; k < mv.npairs; ++k) { eos += p[2 * k]; ess += p[2 * k + 1]; }
    }
    mv.out[2 * f] = eos; mv.out[2 * f + 1] = ess;
}

static Mp2View mp2_shape(int n, int nocc, int naux, int n_frozen)
{
    Mp2View mv{};
    mv.nfz = n_frozen; mv.no = nocc - n_frozen;
    mv.nvpad = (n - nocc + 15) & ~15; mv.napad = (naux + 3) & ~3;
    mv.npairs = mv.no * (mv.no + 1) / 2;
    return mv;
}

// device bytes per fragment of the stage: Bia, the pair partials and the two results (each array rounded up to 256 bytes
// per chunk, which the callers' budgets absorb)
size_t rimp2_fragment_bytes(int n, int nocc, int naux, int n_frozen)
{
    const Mp2View mv = mp2_shape(n, nocc, naux, n_frozen);
    return sizeof(double) * ((size_t)mv.no * mv.napad * mv.nvpad + 2 * (size_t)mv.npairs + 2);
}


// The transform's route for a chunk of nf fragments: host arithmetic only (mqc_hip_rimp2_stage reports it without a device).
// Per wave the LDS holds the packed row and T [16 nt][oc + 1]; fewer waves, then a narrower occupied pass, until it fits.
// For n <= 140 neither the narrowing nor the refusal is reached: one wave with a 64-orbital pass needs 153 840 bytes at
// n = 140 (tests/test_rimp2_stage_cases.py walks every (n, nocc)).
bool rimp2_route(int nf, int n, int nocc, int naux, int n_frozen, int gx_cap, Mp2Route& r, std::string& err)
{
    const Mp2View mv = mp2_shape(n, nocc, naux, n_frozen);
    r = Mp2Route{};
    r.napad = mv.napad; r.nvpad = mv.nvpad; r.npairs = mv.npairs;
    if (mv.no < 1) { err = "RI-MP2: no active occupied orbital"; return false; }
    if (mv.nvpad == 0) return true;                     // no virtual orbital: nothing to correlate, nothing launched
    const int npair = n * (n + 1) / 2;
    const int nt = (n + 15) / 16, nop = (mv.no + 15) & ~15;
    const size_t lds_max = 160 * 1024 - 512;
    auto lds_of = [&](int w, int oc) { return sizeof(double) * (size_t)w * ((size_t)npair + (size_t)16 * nt * (oc + 1)); };
    // C in LDS where it leaves room for at least two waves' buffers (one workgroup per CU, up to eight waves) ...
    const size_t c_lds = sizeof(double) * (size_t)(4 * ((n + 3) / 4)) * (nop + mv.nvpad);
    // (MQC_HIP_MP2_C_LDS=0: never, the A/B switch of the two variants)
    static const bool clds_on = env_on("MQC_HIP_MP2_C_LDS");
    r.clds = clds_on && nop <= 64 && c_lds + lds_of(2, nop) <= lds_max;
    r.nw = MP2_TW;
    if (r.clds) {
        r.oc = nop;
        while (c_lds + lds_of(r.nw, r.oc) > lds_max) r.nw >>= 1;
        r.lds = c_lds + lds_of(r.nw, r.oc);
        r.npf = npair <= 64 * MP2_PF ? MP2_PF : 0;
    } else {
        // ... else C from L2, two workgroups per CU while that leaves a workgroup more than one wave
        r.nw = 4;
        r.oc = std::min(nop, 64);
        while (lds_of(r.nw, r.oc) > (r.nw > 1 ? lds_max / 2 : lds_max)) {
            if (r.nw > 1) r.nw >>= 1;
            else if (r.oc > 16) { r.oc -= 16; ++r.narrowed; }
            else { err = "RI-MP2: a packed row of the fitted tensor does not fit the LDS"; return false; }
        }
        r.lds = lds_of(r.nw, r.oc);
    }
    r.gx = (2048 + nf - 1) / nf;                        // workgroups per fragment: every wave should see several rows
    const int maxg = (mv.napad + r.nw - 1) / r.nw;
    if (r.gx > maxg) r.gx = maxg;
    if (gx_cap > 0 && r.gx > gx_cap) r.gx = gx_cap;
    if (r.gx < 1) r.gx = 1;
    r.passes = (mv.no + r.oc - 1) / r.oc;
    r.rows = (mv.napad + r.gx * r.nw - 1) / (r.gx * r.nw);
    return true;
}

// Bia, the pair partials and the results of the chunk from the slot's pool (static, grow-only, reused across calls)
bool rimp2_carve(const BatchView& bv, int n_frozen, Mp2Pool& p, std::string& err)
{
    static DevicePool pool[2];
    const Mp2View mv = mp2_shape(bv.n, bv.nocc, bv.naux, n_frozen);
    const size_t nf = (size_t)bv.nfrag;
    auto up = [](size_t b) { return (b + 255) & ~size_t(255); };
    p.u_bia = sizeof(double) * nf * mv.no * mv.napad * mv.nvpad;
    p.u_part = sizeof(double) * nf * mv.npairs * 2;
    p.u_out = sizeof(double) * nf * 2;
    p.b_bia = up(p.u_bia); p.b_part = up(p.u_part); p.b_out = up(p.u_out);
    p.base = (char*)pool[bv.slot & 1].ensure(p.b_bia + p.b_part + p.b_out);
    if (!p.base) { err = "out of device memory (RI-MP2 transformed tensor)"; return false; }
    return true;
}

bool rimp2_enqueue(const BatchView& bv, int n_frozen, const Mp2Route& r, const Mp2Pool& p, double* h_out, hipStream_t s, std::string& err)
{
    const int nf = bv.nfrag, n = bv.n;
    Mp2View mv = mp2_shape(n, bv.nocc, bv.naux, n_frozen);
    mv.Bia = (double*)p.base; mv.part = (double*)(p.base + p.b_bia); mv.out = (double*)(p.base + p.b_bia + p.b_part);
    mv.oc = r.oc; mv.ts = r.oc + 1;
    // MQC_HIP_MP2_TIMING=1 (measurement): the span of this stage on stderr, per chunk
    static const bool timing = env_opt_in("MQC_HIP_MP2_TIMING");
    hipEvent_t ev[3] = {};
    if (timing) for (auto& e : ev) { (void)hipEventCreate(&e); }
    if (timing) (void)hipEventRecord(ev[0], s);
    auto kern = !r.clds ? mp2_transform_kernel<false, 0> : r.npf > 0 ? mp2_transform_kernel<true, MP2_PF> : mp2_transform_kernel<true, 0>;
    (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)r.lds);
    hipLaunchKernelGGL(kern, dim3(r.gx, nf), dim3(64 * r.nw), r.lds, s, bv, mv);
    if (timing) (void)hipEventRecord(ev[1], s);
    hipLaunchKernelGGL(mp2_pair_kernel, dim3((mv.npairs + MP2_NW - 1) / MP2_NW, nf), dim3(64 * MP2_NW), 0, s, bv, mv);
    hipLaunchKernelGGL(mp2_reduce_kernel, dim3((nf + 255) / 256), dim3(256), 0, s, bv, mv);
    if (hipMemcpyAsync(h_out, mv.out, sizeof(double) * (size_t)nf * 2, hipMemcpyDeviceToHost, s) != hipSuccess) {
        err = "RI-MP2: the copy of the pair energies failed";
        return false;
    }
    if (timing) {
        (void)hipEventRecord(ev[2], s);
        (void)hipEventSynchronize(ev[2]);
        float all = 0.f, pairs = 0.f;
        (void)hipEventElapsedTime(&all, ev[0], ev[2]);
        (void)hipEventElapsedTime(&pairs, ev[1], ev[2]);
        std::fprintf(stderr, "mqc_hip rimp2: n=%d nfrag=%d occupied %d virtual %d naux %d: total %.3f ms, transform %.3f ms, pairs %.3f ms\n",
                     n, nf, mv.no, n - bv.nocc, bv.naux, all, all - pairs, pairs);
        for (auto& e : ev) (void)hipEventDestroy(e);
    }
    return true;
}

// e_os, e_ss of every fragment of the chunk copied to h_out [nfrag][2] (zeros for fragments whose SCF did not converge),
// everything enqueued on s: the caller joins the stream before it reads h_out
bool launch_rimp2(const BatchView& bv, int n_frozen, double* h_out, hipStream_t s, std::string& err)
{
    if (bv.naux <= 0 || !bv.df_b) { err = "RI-MP2 uses the fitted tensor of a density-fitted SCF"; return false; }
    Mp2Route r;
    if (!rimp2_route(bv.nfrag, bv.n, bv.nocc, bv.naux, n_frozen, 0, r, err)) return false;
    if (r.nvpad == 0) {                                 // no virtual orbital: nothing to correlate
        for (int k = 0; k < 2 * bv.nfrag; ++k) h_out[k] = 0.0;
        return true;
    }
    Mp2Pool p;
    return rimp2_carve(bv, n_frozen, p, err) && rimp2_enqueue(bv, n_frozen, r, p, h_out, s, err);
}

}  // namespace mqc
