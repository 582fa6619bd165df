// kern_cphf.hip -- static dipole polarizabilities: the three-density J/K stream over the square in-core tensor and the
// batched coupled-perturbed Hartree-Fock solve that drives it (mqc_hip_polarizability_batch, mqc_hip_jk_multi_batch).
//
// Model (closed-shell RHF, orbitals C, energies eps, nocc occupied, nvirt = nmo - nocc virtual orbitals), per direction
// d = x, y, z with b = C_v^T r_d C_o and Delta_ai = eps_a - eps_i:
//   D1 = 2 (C_v U C_o^T + C_o U^T C_v^T),   G(U) = C_v^T [J(D1) - K(D1) / 2] C_o,   Delta o U + G(U) = -b,
//   alpha_cd = -tr(D1_d r_c).
// Conjugate gradients preconditioned by 1 / Delta; the three directions of every fragment of the chunk advance together
// and each iteration needs J and K of three symmetric densities.  The single-density stream (kern_fock.hip) would read
// the tensor three times for that; jk_multi_kernel reads each pair row ONCE and contracts it with all three: one global
// load, one LDS write, one LDS read and one packed-triangle address per element for 15 FMAs instead of 5.
#include "engine.hpp"
#include "jk_helpers.hpp"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <vector>

namespace mqc {

constexpr int JKM_ND = 3;       // densities per launch: the kernel is instantiated for three, fewer run with zero densities

// the densities, Coulomb and exchange matrices of a launch, direction-major: [JKM_ND][nfrag][n * n]
struct JkMultiArgs {
    const double* D;
    double *J, *K;
    const double* Dpk;          // [nfrag][JKM_ND][npair] packed (2 - delta) D, written by jk_multi_pack_kernel
    size_t dstride;             // nfrag * n * n
};

__global__ void jk_multi_pack_kernel(BatchView bv, JkMultiArgs a, double* __restrict__ Dpk, int only_active)
{
    const int f = blockIdx.y, d = blockIdx.z;
    if ((only_active & 1) && bv.istate[4 * f] == ST_DONE) return;
    const int n = bv.n, np = bv.npair;
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= np) return;
    int k, l;
    unpack_pair(idx, k, l);
    const double v = a.D[(size_t)d * a.dstride + (size_t)f * n * n + (size_t)k * n + l];
    Dpk[((size_t)f * JKM_ND + d) * np + idx] = (k == l) ? v : 2.0 * v;
}

// One wave's exchange work for the row in `rowbuf` (packed lower triangle of V^{ij}) and ND densities: every element
// is read from LDS once and enters 2 ND FMAs.  The density rows D_d[i, .], D_d[j, .] are wave-uniform global rows
// and arrive through the scalar cache, as in row_exchange (kern_fock.hip); l runs in blocks of eight whose LDS reads
// are issued back to back.  Lanes beyond n read a clamped address and are dropped at the flush; l beyond n reads
// element (n - 1, .) and is weighted by zero.
template <int ND, int KCH>
__device__ __forceinline__ void row_exchange_multi(const double* __restrict__ rowbuf, const double* __restrict__ Di,
                                                   const double* __restrict__ Dj, size_t dstride, int n, int lane,
                                                   double (&acc_i)[ND][KCH], double (&acc_j)[ND][KCH])
{
    typedef double double8 __attribute__((ext_vector_type(8)));
    typedef const double8 __attribute__((address_space(4))) * scalar_ptr8;
    typedef const double __attribute__((address_space(4))) * scalar_ptr;
#pragma unroll
    for (int d = 0; d < ND; ++d)
#pragma unroll
        for (int c = 0; c < KCH; ++c) { acc_i[d][c] = 0.0; acc_j[d][c] = 0.0; }
    constexpr int U = 8;
    int kk[KCH], tri[KCH];
#pragma unroll
    for (int c = 0; c < KCH; ++c) {
        const int k = lane + 64 * c;
        kk[c] = k < n ? k : n - 1;
        tri[c] = kk[c] * (kk[c] + 1) / 2;
    }
    for (int l0 = 0; l0 < n; l0 += U) {
        double v[U][KCH];
        const bool full = l0 + U <= n;                          // wave-uniform
        if (full) {
            int lbase = l0 * (l0 + 1) / 2;                      // tri(l + 1) = tri(l) + l + 1
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int l = l0 + u;
#pragma unroll
                for (int c = 0; c < KCH; ++c) {
                    const int ia = tri[c] + l, ib = lbase + kk[c];
                    v[u][c] = rowbuf[ia > ib ? ia : ib];        // tri(max) + min is the larger of the two forms
                }
                lbase += l + 1;
            }
        } else {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int l = (l0 + u < n) ? l0 + u : n - 1;
                const int lbase = l * (l + 1) / 2;
#pragma unroll
                for (int c = 0; c < KCH; ++c) {
                    const int ia = tri[c] + l, ib = lbase + kk[c];
                    v[u][c] = rowbuf[ia > ib ? ia : ib];
                }
            }
        }
#pragma unroll
        for (int d = 0; d < ND; ++d) {
            const double* __restrict__ di = Di + (size_t)d * dstride;
            const double* __restrict__ dj = Dj + (size_t)d * dstride;
            double dil[U], djl[U];
            if (full) {
                const double8 x = *(scalar_ptr8)(di + l0), y = *(scalar_ptr8)(dj + l0);
#pragma unroll
                for (int u = 0; u < U; ++u) { dil[u] = x[u]; djl[u] = y[u]; }
            } else {
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const bool live = l0 + u < n;
                    const int lr = live ? l0 + u : n - 1;
                    dil[u] = live ? ((scalar_ptr)di)[lr] : 0.0;
                    djl[u] = live ? ((scalar_ptr)dj)[lr] : 0.0;
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int c = 0; c < KCH; ++c) {
                    acc_i[d][c] += v[u][c] * djl[u];
                    acc_j[d][c] += v[u][c] * dil[u];
                }
        }
    }
}

// The three-density stream over the SQUARE tensor, in the structure of jk_incore_kernel: a wave owns a pair row (ij),
// loads it contiguously (MAXU > 0: the whole row in registers, the next row issued before this one is contracted;
// MAXU == 0: chunks of 16 x 64), parks it in its private LDS buffer and forms
//   J_d[ij] = sum_kl M[ij, kl] D'_d[kl]   and the exchange mat-vecs   K_d[i, .] += V^{ij} D_d[., j],  K_d[j, .] += V^{ij} D_d[., i]
// for d = 0 .. ND - 1 in one pass.
//   DPLDS: the ND packed densities sit in LDS behind the row buffers, else they are read from the packed copy in global
//          memory (L2), coalesced with the row itself -- three packed densities of n = 116 alone exceed the LDS;
//   KLDS:  the ND exchange accumulators (ND n^2 doubles) sit in LDS and are flushed once per workgroup, else every row
//          adds into global memory.
template <int ND, int KCH, bool KLDS, bool DPLDS, int NW, int MAXU>
__global__ void __launch_bounds__(64 * NW) jk_multi_kernel(BatchView bv, JkMultiArgs a, int only_active)
{
    extern __shared__ double lds[];
    const int f = blockIdx.y;
    if ((only_active & 1) && bv.istate[4 * f] == ST_DONE) return;
    const int n = bv.n, np = bv.npair;
    const size_t nn = (size_t)n * n;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    constexpr int NTH = 64 * NW;
    const double* __restrict__ Dg = a.D + (size_t)f * nn;          // density d at + d * dstride
    double* __restrict__ Jg = a.J + (size_t)f * nn;
    double* __restrict__ Kg = a.K + (size_t)f * nn;
    const double* __restrict__ M = bv.eri + (size_t)f * np * np;
    const double* __restrict__ Dpg = a.Dpk + (size_t)f * ND * np;
    double* rowbuf = lds + (size_t)wave * np;                       // NW private row buffers
    double* Dp = lds + (size_t)NW * np;                             // [ND][np] (DPLDS)
    double* Kl = Dp + (DPLDS ? (size_t)ND * np : 0);                // [ND][n * n] (KLDS)
    if (DPLDS)
        for (int idx = tid; idx < ND * np; idx += NTH) Dp[idx] = Dpg[idx];
    if (KLDS)
        for (int idx = tid; idx < ND * (int)nn; idx += NTH) Kl[idx] = 0.0;
    if (DPLDS || KLDS) __syncthreads();
    const double* Dps = DPLDS ? Dp : Dpg;

    const int stride = gridDim.x * NW;
    int row = blockIdx.x * NW + wave;
    constexpr int CH = 16;
    double v[MAXU > 0 ? MAXU : 1];
    auto load_row = [&](int r) {
        const double* __restrict__ src = M + (size_t)r * np;
#pragma unroll
        for (int u = 0; u < MAXU; ++u) { const int idx = lane + 64 * u; v[u] = idx < np ? src[idx] : 0.0; }
    };
    if (MAXU > 0 && row < np) load_row(row);
    while (row < np) {
        int i, j;
        unpack_pair(row, i, j);
        double accj[ND];
#pragma unroll
        for (int d = 0; d < ND; ++d) accj[d] = 0.0;
        const int nrow = row + stride;
        if constexpr (MAXU > 0) {
#pragma unroll
            for (int u = 0; u < MAXU; ++u) {
                const int idx = lane + 64 * u;
                if (idx < np) {
                    rowbuf[idx] = v[u];
#pragma unroll
                    for (int d = 0; d < ND; ++d) accj[d] += v[u] * Dps[(size_t)d * np + idx];
                }
            }
            // the next row's loads go out now and complete while this row is contracted
            if (nrow < np) load_row(nrow);
        } else {
            const double* __restrict__ src = M + (size_t)row * np;
            for (int base = 0; base < np; base += 64 * CH) {
                double w[CH];
#pragma unroll
                for (int u = 0; u < CH; ++u) { const int idx = base + lane + 64 * u; w[u] = idx < np ? src[idx] : 0.0; }
#pragma unroll
                for (int u = 0; u < CH; ++u) {
                    const int idx = base + lane + 64 * u;
                    if (idx < np) {
                        rowbuf[idx] = w[u];
#pragma unroll
                        for (int d = 0; d < ND; ++d) accj[d] += w[u] * Dps[(size_t)d * np + idx];
                    }
                }
            }
        }
        // the exchange reads, lane k, what other lanes of this wave stored above: LDS operations of one wave execute in
        // program order; the wavefront-scope fence (no instruction) keeps the compiler from moving the reads up
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
#pragma unroll
        for (int d = 0; d < ND; ++d) {
            const double s = wave_sum_top(accj[d]);
            if (lane == 63) { Jg[(size_t)d * a.dstride + (size_t)i * n + j] = s; Jg[(size_t)d * a.dstride + (size_t)j * n + i] = s; }
        }
        double acc_i[ND][KCH], acc_j[ND][KCH];
        const int iu = __builtin_amdgcn_readfirstlane(i), ju = __builtin_amdgcn_readfirstlane(j);
        row_exchange_multi<ND, KCH>(rowbuf, Dg + (size_t)iu * n, Dg + (size_t)ju * n, a.dstride, n, lane, acc_i, acc_j);
#pragma unroll
        for (int d = 0; d < ND; ++d)
#pragma unroll
            for (int c = 0; c < KCH; ++c) {
                const int k = lane + 64 * c;
                if (k < n) {
                    double* Kt = KLDS ? Kl + (size_t)d * nn : Kg + (size_t)d * a.dstride;
                    atomicAdd(&Kt[(size_t)i * n + k], acc_i[d][c]);
                    if (i != j) atomicAdd(&Kt[(size_t)j * n + k], acc_j[d][c]);
                }
            }
        // the next row's stores must not pass this row's reads
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        row = nrow;
    }
    if (KLDS) {
        __syncthreads();
        for (int idx = tid; idx < ND * (int)nn; idx += NTH) {
            const double kv = Kl[idx];
            const int d = idx / (int)nn;
            if (kv != 0.0) atomicAdd(&Kg[(size_t)d * a.dstride + (idx - d * (int)nn)], kv);
        }
    }
}

template <int KCH, bool KLDS, bool DPLDS, int NW, int MAXU>
static JkMultiRoute jk_multi_launch(const BatchView& bv, const JkMultiArgs& a, int oa, size_t lds, hipStream_t s)
{
    auto kern = jk_multi_kernel<JKM_ND, KCH, KLDS, DPLDS, NW, MAXU>;
    (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    // enough workgroups to cover the card several times, few enough that the per-workgroup prologue (packed densities,
    // the K accumulators zeroed) and flush stay amortised over many rows
    int gx = (4096 + bv.nfrag - 1) / bv.nfrag;
    const int maxx = (bv.npair + NW - 1) / NW;
    if (gx < 1) gx = 1;
    if (gx > maxx) gx = maxx;
    hipLaunchKernelGGL(kern, dim3(gx, bv.nfrag), dim3(64 * NW), lds, s, bv, a, oa);
    return {KCH, NW, MAXU, gx, KLDS, DPLDS};
}

static DevicePool g_jkm_pack_pool[2];

// Where the accumulators and the packed densities live (doubles of LDS against the 159 KB a workgroup may take):
//   n <= 48 (npair <= 1176): eight row buffers, three packed densities and three K accumulators -- everything in LDS;
//   n = 49 .. 55: four row buffers, the rest as above;
//   n = 56 .. 81: four row buffers and the packed densities; K through global atomics (3 n^2 doubles no longer fit);
//   n = 82 .. 100: four row buffers only; packed densities from global memory;
//   n = 101 .. 116: two row buffers only.
// J, K and D hold JKM_ND matrices per fragment, direction-major [JKM_ND][nfrag][n * n]; nd < JKM_ND: the densities beyond
// nd are zeroed here and their J and K come out as zeros.  false: no instance for this shape (n > 116).
bool launch_jk_multi(const BatchView& bv, int nd, double* D, double* J, double* K, bool only_active, hipStream_t s, JkMultiRoute* route,
                     std::string& err)
{
    const int n = bv.n, np = bv.npair, nf = bv.nfrag;
    const size_t nn = (size_t)n * n, L = (160 * 1024 - 1024) / sizeof(double);
    if (bv.eri_tri || !bv.eri) { err = "the multi-density J/K stream reads the square in-core tensor"; return false; }
    double* Dpk = (double*)g_jkm_pack_pool[bv.slot & 1].ensure(sizeof(double) * (size_t)nf * JKM_ND * np + 256);
    if (!Dpk) { err = "out of device memory (packed densities)"; return false; }
    JkMultiArgs a{D, J, K, Dpk, (size_t)nf * nn};
    const int oa = only_active ? 1 : 0;
    if (nd < JKM_ND) (void)hipMemsetAsync(D + (size_t)nd * a.dstride, 0, sizeof(double) * (size_t)(JKM_ND - nd) * a.dstride, s);
    (void)hipMemsetAsync(K, 0, sizeof(double) * JKM_ND * a.dstride, s);
    hipLaunchKernelGGL(jk_multi_pack_kernel, dim3((np + 255) / 256, nf, JKM_ND), dim3(256), 0, s, bv, a, Dpk, oa);
    const size_t np_ = (size_t)np, dp = JKM_ND * np_, kl = JKM_ND * nn;
    const int kch = (n + 63) / 64;
    JkMultiRoute r{};
    auto bytes = [](size_t doubles) { return sizeof(double) * doubles; };
    if (kch == 1 && 8 * np_ + dp + kl <= L && np <= 19 * 64) {
        if (np <= 5 * 64) r = jk_multi_launch<1, true, true, 8, 5>(bv, a, oa, bytes(8 * np_ + dp + kl), s);
        else if (np <= 10 * 64) r = jk_multi_launch<1, true, true, 8, 10>(bv, a, oa, bytes(8 * np_ + dp + kl), s);
        else r = jk_multi_launch<1, true, true, 8, 19>(bv, a, oa, bytes(8 * np_ + dp + kl), s);
    } else if (kch == 1 && 4 * np_ + dp + kl <= L) r = jk_multi_launch<1, true, true, 4, 0>(bv, a, oa, bytes(4 * np_ + dp + kl), s);
    else if (kch == 1 && 4 * np_ + dp <= L) r = jk_multi_launch<1, false, true, 4, 0>(bv, a, oa, bytes(4 * np_ + dp), s);
    else if (kch == 2 && 4 * np_ + dp <= L) r = jk_multi_launch<2, false, true, 4, 0>(bv, a, oa, bytes(4 * np_ + dp), s);
    else if (kch == 2 && 4 * np_ <= L) r = jk_multi_launch<2, false, false, 4, 0>(bv, a, oa, bytes(4 * np_), s);
    else if (kch == 2 && 2 * np_ <= L) r = jk_multi_launch<2, false, false, 2, 0>(bv, a, oa, bytes(2 * np_), s);
    else { err = "the multi-density J/K stream has no instance for n_ao = " + std::to_string(n); return false; }
    if (route) *route = r;
    return true;
}

std::string jk_multi_route_name(const JkMultiRoute& r)
{
    char buf[64];
    std::snprintf(buf, sizeof(buf), "multi<%d,%d,%s,%s,%d,%d>", JKM_ND, r.kch, r.klds ? "lds" : "global", r.dplds ? "lds" : "mem", r.nw, r.maxu);
    return buf;
}

bool cphf_multi_on()
{
    static const bool on = env_on("MQC_HIP_CPHF_MULTI");
    return on;
}

// ---------------------------------------------------------------------------------------------------------------
// The per-fragment kernels of the solve.  One workgroup per (direction, fragment); none of them is a hot path.
constexpr int CPHF_NT = 256;

struct CphfView {
    int nfrag, n, nocc, max_iter, nvs;     // nvs = (n - nocc) * nocc: stride of the occupied-virtual vectors
    double tol;
    const double *C, *eps;                 // the SCF's orbitals [nfrag][n * n] (column = orbital) and energies [nfrag][n]
    const int* scf_istate;                 // the SCF's [nfrag][4]: state, iterations, nmo, converged
    int* state;                            // [nfrag][4]: ST_ITER / ST_DONE, iterations, CPHF_* status, nvirt -- the istate of the J/K launches
    double* R;                             // [nfrag][3][n * n] dipole matrices
    double *D1, *J, *K;                    // [3][nfrag][n * n]
    double *U, *r, *p, *Ap;                // [nfrag][3][nvs]
    double* dots;                          // [nfrag][3][4]: r.z, max |r|, 1 = p.Ap <= 0 met, -
    double* alpha;                         // [nfrag][9]
    int* counter;                          // [1] fragments still iterating
};

__device__ __forceinline__ double block_sum(double v, double* red)
{
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) red[wave] = v;
    __syncthreads();
    double s = 0.0;
    for (int w = 0; w < CPHF_NT / 64; ++w) s += red[w];
    return s;
}
__device__ __forceinline__ double block_max(double v, double* red)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_down(v, off, 64));
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) red[wave] = v;
    __syncthreads();
    double s = 0.0;
    for (int w = 0; w < CPHF_NT / 64; ++w) s = fmax(s, red[w]);
    return s;
}

__global__ void cphf_init_kernel(CphfView cv)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= cv.nfrag) return;
    const int nmo = cv.scf_istate[4 * f + 2];
    const bool solve = cv.scf_istate[4 * f + 3] != 0 && cv.scf_istate[4 * f] == ST_DONE && nmo >= cv.nocc && nmo <= cv.n;
    cv.state[4 * f] = solve ? ST_ITER : ST_DONE;
    cv.state[4 * f + 1] = 0;
    cv.state[4 * f + 2] = CPHF_NOT_SOLVED;
    cv.state[4 * f + 3] = solve ? nmo - cv.nocc : 0;
}

// T[mu][i] = sum_nu A[mu, nu] C[nu, i] for the occupied orbitals, into LDS
__device__ __forceinline__ void half_transform(const double* __restrict__ A, const double* __restrict__ C, int n, int nocc, double* T)
{
    for (int e = threadIdx.x; e < n * nocc; e += CPHF_NT) {
        const int mu = e / nocc, i = e - mu * nocc;
        double t = 0.0;
        for (int nu = 0; nu < n; ++nu) t += A[(size_t)mu * n + nu] * C[(size_t)nu * n + i];
        T[e] = t;
    }
    __syncthreads();
}

// b = C_v^T r_d C_o; U = 0, r = -b, p = z = r / Delta; r.z and max |r|
__global__ void __launch_bounds__(CPHF_NT) cphf_setup_kernel(CphfView cv)
{
    extern __shared__ double T[];
    __shared__ double red[CPHF_NT / 64];
    const int d = blockIdx.x, f = blockIdx.y;
    if (cv.state[4 * f] == ST_DONE) return;
    const int n = cv.n, nocc = cv.nocc, nvirt = cv.state[4 * f + 3];
    const double* __restrict__ C = cv.C + (size_t)f * n * n;
    const double* __restrict__ eps = cv.eps + (size_t)f * n;
    half_transform(cv.R + ((size_t)f * 3 + d) * n * n, C, n, nocc, T);
    const size_t o = ((size_t)f * 3 + d) * cv.nvs;
    double rz = 0.0, rmax = 0.0;
    for (int e = threadIdx.x; e < nvirt * nocc; e += CPHF_NT) {
        const int av = e / nocc, i = e - av * nocc;
        double b = 0.0;
        for (int mu = 0; mu < n; ++mu) b += C[(size_t)mu * n + nocc + av] * T[mu * nocc + i];
        const double r = -b, z = r / (eps[nocc + av] - eps[i]);
        cv.U[o + e] = 0.0; cv.r[o + e] = r; cv.p[o + e] = z;
        rz += r * z;
        rmax = fmax(rmax, fabs(r));
    }
    rz = block_sum(rz, red);
    rmax = block_max(rmax, red);
    if (threadIdx.x == 0) {
        double* dt = cv.dots + ((size_t)f * 3 + d) * 4;
        dt[0] = rz; dt[1] = rmax; dt[2] = 0.0; dt[3] = 0.0;
    }
}

// D1 = 2 (C_v X C_o^T + C_o X^T C_v^T), X = the search direction p of a fragment still iterating, or (final) the solution
// U of a converged one.  The lower triangle is formed and mirrored, so D1 is symmetric to the bit.
__global__ void __launch_bounds__(CPHF_NT) cphf_density_kernel(CphfView cv, int final)
{
    extern __shared__ double T[];
    const int d = blockIdx.x, f = blockIdx.y;
    if (final ? cv.state[4 * f + 2] != CPHF_CONVERGED : cv.state[4 * f] == ST_DONE) return;
    const int n = cv.n, nocc = cv.nocc, nvirt = cv.state[4 * f + 3];
    const double* __restrict__ C = cv.C + (size_t)f * n * n;
    const double* __restrict__ X = (final ? cv.U : cv.p) + ((size_t)f * 3 + d) * cv.nvs;
    for (int e = threadIdx.x; e < n * nocc; e += CPHF_NT) {
        const int mu = e / nocc, i = e - mu * nocc;
        double t = 0.0;
        for (int av = 0; av < nvirt; ++av) t += C[(size_t)mu * n + nocc + av] * X[av * nocc + i];
        T[e] = t;
    }
    __syncthreads();
    double* __restrict__ D1 = cv.D1 + ((size_t)d * cv.nfrag + f) * n * n;
    for (int e = threadIdx.x; e < n * n; e += CPHF_NT) {
        const int mu = e / n, nu = e - mu * n;
        if (nu > mu) continue;
        double t = 0.0;
        for (int i = 0; i < nocc; ++i) t += T[mu * nocc + i] * C[(size_t)nu * n + i] + C[(size_t)mu * n + i] * T[nu * nocc + i];
        D1[(size_t)mu * n + nu] = 2.0 * t;
        D1[(size_t)nu * n + mu] = 2.0 * t;
    }
}

// One step of the preconditioned conjugate gradients for (direction, fragment): A p = Delta o p + C_v^T [J - K / 2] C_o,
// step length r.z / p.A p, U and r updated, z = r / Delta, the new direction.  A direction whose residual is exactly
// zero stays as it is; p.A p <= 0 with a non-zero residual marks the reference as unstable.
__global__ void __launch_bounds__(CPHF_NT) cphf_update_kernel(CphfView cv)
{
    extern __shared__ double T[];
    __shared__ double red[CPHF_NT / 64];
    const int d = blockIdx.x, f = blockIdx.y;
    if (cv.state[4 * f] == ST_DONE) return;
    const int n = cv.n, nocc = cv.nocc, nvirt = cv.state[4 * f + 3], nvo = nvirt * nocc;
    const double* __restrict__ C = cv.C + (size_t)f * n * n;
    const double* __restrict__ eps = cv.eps + (size_t)f * n;
    const double* __restrict__ J = cv.J + ((size_t)d * cv.nfrag + f) * n * n;
    const double* __restrict__ K = cv.K + ((size_t)d * cv.nfrag + f) * n * n;
    for (int e = threadIdx.x; e < n * nocc; e += CPHF_NT) {
        const int mu = e / nocc, i = e - mu * nocc;
        double t = 0.0;
        for (int nu = 0; nu < n; ++nu) t += (J[(size_t)mu * n + nu] - 0.5 * K[(size_t)mu * n + nu]) * C[(size_t)nu * n + i];
        T[e] = t;
    }
    __syncthreads();
    const size_t o = ((size_t)f * 3 + d) * cv.nvs;
    double* dt = cv.dots + ((size_t)f * 3 + d) * 4;
    double pap = 0.0;
    for (int e = threadIdx.x; e < nvo; e += CPHF_NT) {
        const int av = e / nocc, i = e - av * nocc;
        double g = 0.0;
        for (int mu = 0; mu < n; ++mu) g += C[(size_t)mu * n + nocc + av] * T[mu * nocc + i];
        const double p = cv.p[o + e], ap = (eps[nocc + av] - eps[i]) * p + g;
        cv.Ap[o + e] = ap;
        pap += p * ap;
    }
    pap = block_sum(pap, red);
    const double rz = dt[0];
    const bool live = rz > 0.0, unstable = live && !(pap > 0.0);
    const double step = (live && !unstable) ? rz / pap : 0.0;
    double rz_new = 0.0, rmax = 0.0;
    for (int e = threadIdx.x; e < nvo; e += CPHF_NT) {
        const int av = e / nocc, i = e - av * nocc;
        const double r = cv.r[o + e] - step * cv.Ap[o + e];
        cv.U[o + e] += step * cv.p[o + e];
        cv.r[o + e] = r;
        rz_new += r * r / (eps[nocc + av] - eps[i]);
        rmax = fmax(rmax, fabs(r));
    }
    rz_new = block_sum(rz_new, red);
    rmax = block_max(rmax, red);
    const double beta = live ? rz_new / rz : 0.0;
    for (int e = threadIdx.x; e < nvo; e += CPHF_NT) {
        const int av = e / nocc, i = e - av * nocc;
        cv.p[o + e] = cv.r[o + e] / (eps[nocc + av] - eps[i]) + beta * cv.p[o + e];
    }
    if (threadIdx.x == 0) { dt[0] = rz_new; dt[1] = rmax; if (unstable) dt[2] = 1.0; }
}

// per fragment: count the iteration, then converged / unstable / out of iterations / still running (counted)
__global__ void cphf_flag_kernel(CphfView cv, int first)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= cv.nfrag || cv.state[4 * f] == ST_DONE) return;
    if (!first) cv.state[4 * f + 1] += 1;
    const double* dt = cv.dots + (size_t)f * 12;
    const double rmax = fmax(dt[1], fmax(dt[5], dt[9]));
    const bool unstable = dt[2] != 0.0 || dt[6] != 0.0 || dt[10] != 0.0;
    int status = -1;
    if (unstable) status = CPHF_UNSTABLE;
    else if (rmax <= cv.tol) status = CPHF_CONVERGED;          // a NaN residual never converges: it runs out of iterations
    else if (cv.state[4 * f + 1] >= cv.max_iter) status = CPHF_NOT_CONVERGED;
    if (status >= 0) { cv.state[4 * f] = ST_DONE; cv.state[4 * f + 2] = status; }
    else atomicAdd(cv.counter, 1);
}

// alpha_cd = -tr(D1_d r_c), row c, column d, of the converged fragments
__global__ void __launch_bounds__(CPHF_NT) cphf_alpha_kernel(CphfView cv)
{
    __shared__ double red[CPHF_NT / 64];
    const int d = blockIdx.x, f = blockIdx.y;
    if (cv.state[4 * f + 2] != CPHF_CONVERGED) return;
    const int n = cv.n;
    const double* __restrict__ D1 = cv.D1 + ((size_t)d * cv.nfrag + f) * n * n;
    const double* __restrict__ R = cv.R + (size_t)f * 3 * n * n;
    double t[3] = {0.0, 0.0, 0.0};
    for (int e = threadIdx.x; e < n * n; e += CPHF_NT) {
        const double x = D1[e];
#pragma unroll
        for (int c = 0; c < 3; ++c) t[c] += x * R[(size_t)c * n * n + e];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double s = block_sum(t[c], red);
        if (threadIdx.x == 0) cv.alpha[(size_t)f * 9 + 3 * c + d] = -s;
    }
}

// kern_int1e.hip: <mu| x, y, z |nu> about the origin of every fragment into out [nfrag][3][n * n]
void launch_dipole_matrices(const BatchView& bv, const Topology& topo, double* out, hipStream_t s);

// device bytes per fragment of the solve: 3 x (D1, J, K), the dipole matrices, four conjugate-gradient vectors and the
// packed densities of the stream, each array rounded up to 256 bytes per chunk (the callers' budgets absorb that)
size_t cphf_fragment_bytes(int n, int nocc, int nmo)
{
    const size_t nn = (size_t)n * n, nvo = (size_t)std::max(0, nmo - nocc) * nocc, np = (size_t)n * (n + 1) / 2;
    return sizeof(double) * (9 * nn + 3 * nn + 4 * 3 * nvo + 3 * np + 12 + 9) + sizeof(int) * 4;
}

static DevicePool g_cphf_pool[2];

// The solve of one converged in-core chunk (bv: tensor, orbitals and energies still in place), everything on s with one
// counter read per iteration.  h_alpha [nfrag][9], h_iter [nfrag], h_status [nfrag] (CPHF_*) are complete on return.
bool launch_cphf(const BatchView& bv, const Topology& topo, double tol, int max_iter, double* h_alpha, int* h_iter, int* h_status,
                 int* h_counter, hipStream_t s, std::string& err)
{
    const int nf = bv.nfrag, n = bv.n, nocc = bv.nocc;
    const size_t nn = (size_t)n * n;
    CphfView cv{};
    cv.nfrag = nf; cv.n = n; cv.nocc = nocc; cv.max_iter = max_iter; cv.tol = tol;
    cv.nvs = std::max(1, (n - nocc) * nocc);
    cv.C = bv.C; cv.eps = bv.eps; cv.scf_istate = bv.istate;
    auto up = [](size_t b) { return (b + 255) & ~size_t(255); };
    const size_t b_mat = up(sizeof(double) * 3 * (size_t)nf * nn), b_vec = up(sizeof(double) * 3 * (size_t)nf * cv.nvs);
    const size_t b_dots = up(sizeof(double) * 12 * (size_t)nf), b_alpha = up(sizeof(double) * 9 * (size_t)nf), b_state = up(sizeof(int) * 4 * (size_t)nf);
    char* base = (char*)g_cphf_pool[bv.slot & 1].ensure(4 * b_mat + 4 * b_vec + b_dots + b_alpha + b_state + 256);
    if (!base) { err = "out of device memory (CPHF)"; return false; }
    auto take = [&base](size_t b) { char* p = base; base += b; return p; };
    cv.R = (double*)take(b_mat); cv.D1 = (double*)take(b_mat); cv.J = (double*)take(b_mat); cv.K = (double*)take(b_mat);
    cv.U = (double*)take(b_vec); cv.r = (double*)take(b_vec); cv.p = (double*)take(b_vec); cv.Ap = (double*)take(b_vec);
    cv.dots = (double*)take(b_dots); cv.alpha = (double*)take(b_alpha); cv.state = (int*)take(b_state);
    cv.counter = (int*)take(256);

    const size_t lds = sizeof(double) * (size_t)n * std::max(1, nocc);
    for (const void* k : {(const void*)cphf_setup_kernel, (const void*)cphf_update_kernel})
        (void)hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    (void)hipFuncSetAttribute((const void*)cphf_density_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    auto fail_hip = [&](const char* what) { err = std::string("CPHF: ") + what + " failed"; return false; };

    (void)hipMemsetAsync(cv.alpha, 0, sizeof(double) * 9 * (size_t)nf, s);
    hipLaunchKernelGGL(cphf_init_kernel, dim3((nf + 255) / 256), dim3(256), 0, s, cv);
    launch_dipole_matrices(bv, topo, cv.R, s);
    hipLaunchKernelGGL(cphf_setup_kernel, dim3(3, nf), dim3(CPHF_NT), lds, s, cv);
    auto poll = [&](int first, int& remaining) {
        if (hipMemsetAsync(cv.counter, 0, sizeof(int), s) != hipSuccess) return false;
        hipLaunchKernelGGL(cphf_flag_kernel, dim3((nf + 255) / 256), dim3(256), 0, s, cv, first);
        if (hipMemcpyAsync(h_counter, cv.counter, sizeof(int), hipMemcpyDeviceToHost, s) != hipSuccess) return false;
        if (hipStreamSynchronize(s) != hipSuccess) return false;
        remaining = h_counter[0];
        return true;
    };
    int remaining = 0;
    if (!poll(1, remaining)) return fail_hip("the setup");

    // the J/K launches see the solve's own state: finished fragments are skipped as ST_DONE fragments are in the SCF loop
    BatchView vj = bv;
    vj.istate = cv.state; vj.jk_loaded = nullptr; vj.jk_q = nullptr;
    const bool multi = cphf_multi_on();
    // MQC_HIP_CPHF_TIMING=1 (measurement): every iteration runs BOTH routes (the three single-density launches first, the
    // default's results last) between HIP events; one line per chunk on stderr
    static const bool timing = env_opt_in("MQC_HIP_CPHF_TIMING");
    hipEvent_t ev[4] = {};
    if (timing) for (auto& e : ev) (void)hipEventCreate(&e);
    double t_multi = 0.0, t_single = 0.0, bytes = 0.0;
    int launches = 0;
    auto run_single = [&]() {
        for (int d = 0; d < 3; ++d) {
            BatchView v1 = vj;
            v1.D = cv.D1 + (size_t)d * nf * nn; v1.J = cv.J + (size_t)d * nf * nn; v1.K = cv.K + (size_t)d * nf * nn;
            launch_jk_incore(v1, true, s);
        }
        return true;
    };
    auto run_multi = [&]() { return launch_jk_multi(vj, 3, cv.D1, cv.J, cv.K, true, s, nullptr, err); };
    for (int it = 0; remaining > 0 && it < max_iter; ++it) {
        hipLaunchKernelGGL(cphf_density_kernel, dim3(3, nf), dim3(CPHF_NT), lds, s, cv, 0);
        if (timing) {
            (void)hipEventRecord(ev[0], s);
            if (multi) run_single(); else if (!run_multi()) return false;
            (void)hipEventRecord(ev[1], s);
            (void)hipEventRecord(ev[2], s);
        }
        if (multi) { if (!run_multi()) return false; } else run_single();
        if (timing) (void)hipEventRecord(ev[3], s);
        hipLaunchKernelGGL(cphf_update_kernel, dim3(3, nf), dim3(CPHF_NT), lds, s, cv);
        const int active = remaining;
        if (!poll(0, remaining)) return fail_hip("an iteration");
        if (timing) {
            float other = 0.f, own = 0.f;
            (void)hipEventElapsedTime(&other, ev[0], ev[1]);
            (void)hipEventElapsedTime(&own, ev[2], ev[3]);
            (multi ? t_single : t_multi) += other * 1e-3;
            (multi ? t_multi : t_single) += own * 1e-3;
            bytes += 8.0 * (double)active * (double)bv.npair * (double)bv.npair;
            ++launches;
        }
    }
    if (timing) {
        std::fprintf(stderr, "mqc_hip cphf timing: n=%d nfrag=%d launches %d: multi-density stream %.3f ms per launch, %.3f GB read per launch, %.3f of 8 TB/s; "
                             "three single-density launches %.3f ms per launch (%.3f GB)\n",
                     n, nf, launches, launches ? t_multi * 1e3 / launches : 0.0, launches ? bytes * 1e-9 / launches : 0.0,
                     t_multi > 0 ? bytes / t_multi / 8.0e12 : 0.0, launches ? t_single * 1e3 / launches : 0.0, launches ? 3.0 * bytes * 1e-9 / launches : 0.0);
        for (auto& e : ev) (void)hipEventDestroy(e);
    }
    // the first-order densities of the converged fragments from their solutions, then alpha
    hipLaunchKernelGGL(cphf_density_kernel, dim3(3, nf), dim3(CPHF_NT), lds, s, cv, 1);
    hipLaunchKernelGGL(cphf_alpha_kernel, dim3(3, nf), dim3(CPHF_NT), 0, s, cv);
    std::vector<int> st((size_t)nf * 4);
    if (hipMemcpyAsync(h_alpha, cv.alpha, sizeof(double) * 9 * (size_t)nf, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipMemcpyAsync(st.data(), cv.state, sizeof(int) * 4 * (size_t)nf, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
        return fail_hip("the copy of the results");
    for (int f = 0; f < nf; ++f) { h_iter[f] = st[4 * (size_t)f + 1]; h_status[f] = st[4 * (size_t)f + 2]; }
    return true;
}

}  // namespace mqc
