// kern_pcm.hip -- C-PCM implicit solvation (conductor-like polarisable continuum) for a whole batch.
//
// The term the reference's cuestPCMPotentialCompute adds to the Fock matrix ("C-PCM charges + V_pcm",
// mqc_cuest_integrals.f90:974-1366), with this engine's own discretisation (the cavity itself is
// built on the host, pcm_cavity.hpp).  With T tesserae s_t of area a_t on the cavity of a fragment:
//     S_tt = zeta_t sqrt(2/pi),  S_tu = erf(zeta_tu r_tu)/r_tu,  zeta_t = 4.90/sqrt(a_t),  zeta_tu = zeta_t zeta_u/sqrt(zeta_t^2 + zeta_u^2)
//     A[t][mu nu] = (mu| 1/|r - s_t| |nu)         packed pairs, mu >= nu
//     v = v_nuc - A d,   q = -f S^-1 v,   E_pcm = q.v / 2,   V_pcm = -sum_t q_t A[t]          f = (eps - 1)/eps
// SETUP (once per geometry): S, its Cholesky factor L and L^-1, A, B = L^-1 A, b = L^-1 v_nuc.  The factorisation and
// B are the density fitting's kernels (kern_df.hip: blocked Cholesky and L^-1 A3 on the FP64 matrix cores) run on a view
// whose "auxiliary basis" is the chunk's tessera stride: beyond a fragment's own count S continues as the identity and
// A as zeros, so L = diag(L_f, 1) and the padding rows of B are zeros -- one size for the whole chunk, ragged counts.
// ITERATION: c = b - B d,  E_pcm = -f/2 c.c,  V_pcm = f sum_P c_P B^P  (q never forms): two passes over B, the shape
// of the density-fitted J, one workgroup per fragment.  V_pcm and E_pcm reach the Fock matrix the way V_xc and E_xc do:
// half of V_pcm into both mirror elements of the un-symmetrised accumulator bv.Vxc, E_pcm added to scal[5]; the SCF-step
// kernels are untouched.
#include "engine.hpp"
#include "md_integrals.hpp"
#include <vector>

namespace mqc {

constexpr int PCM_NT = 256;
constexpr double PCM_ZETA = 4.90;

// ---- setup ----------------------------------------------------------------------------------------------------------
// cavity matrix of every fragment, identity beyond its own tesserae
__global__ void __launch_bounds__(PCM_NT) pcm_s_kernel(PcmView pv)
{
    const int f = blockIdx.y, ts = pv.stride;
    const size_t idx = (size_t)blockIdx.x * PCM_NT + threadIdx.x;
    if (idx >= (size_t)ts * ts) return;
    const int i = (int)(idx / ts), j = (int)(idx - (size_t)i * ts), nt = pv.nt[f];
    double val;
    if (i >= nt || j >= nt) val = (i == j) ? 1.0 : 0.0;
    else {
        const double* pi = pv.pts + ((size_t)f * ts + i) * 4;
        const double zi = PCM_ZETA / sqrt(pi[3]);
        if (i == j) val = zi * 0.79788456080286535588;      // sqrt(2/pi)
        else {
            const double* pj = pv.pts + ((size_t)f * ts + j) * 4;
            const double zj = PCM_ZETA / sqrt(pj[3]);
            const double zij = zi * zj / sqrt(zi * zi + zj * zj);
            const double dx = pi[0] - pj[0], dy = pi[1] - pj[1], dz = pi[2] - pj[2];
            const double r = sqrt(dx * dx + dy * dy + dz * dz);
            val = erf(zij * r) / r;
        }
    }
    pv.S[(size_t)f * ts * ts + idx] = val;
}

// potential of the nuclei at the tesserae (ghosts carry no charge), zero beyond a fragment's own tesserae
__global__ void __launch_bounds__(PCM_NT) pcm_vnuc_kernel(BatchView bv, PcmView pv)
{
    const int f = blockIdx.y, ts = pv.stride, t = blockIdx.x * PCM_NT + threadIdx.x;
    if (t >= ts) return;
    double v = 0.0;
    if (t < pv.nt[f]) {
        const double* p = pv.pts + ((size_t)f * ts + t) * 4;
        const double* xyz = bv.xyz + (size_t)f * bv.topo.natoms * 3;
        for (int a = 0; a < bv.topo.natoms; ++a) {
            const double z = bv.topo.zeff[a];
            if (z == 0.0) continue;
            const double dx = p[0] - xyz[3 * a], dy = p[1] - xyz[3 * a + 1], dz = p[2] - xyz[3 * a + 2];
            v += z / sqrt(dx * dx + dy * dy + dz * dz);
        }
    }
    pv.vnuc[(size_t)f * ts + t] = v;
}

// A[t][pair]: the nuclear-attraction integral of int1e_kernel with the sum over centres kept open.  One thread per
// (tessera, shell pair, fragment), the tessera fastest: a wave shares its shell pair (one control flow, the
// contraction data through the scalar cache) and reads 64 consecutive tesserae.
template <int LA, int LB>
__global__ void __launch_bounds__(64) pcm_a_kernel(BatchView bv, PcmView pv, const int* __restrict__ pairs)
{
    constexpr int NCA = ncart(LA), NCB = ncart(LB), L = LA + LB;
    const int f = blockIdx.z, ip = blockIdx.y, ts = pv.stride, t = blockIdx.x * 64 + threadIdx.x;
    if (t >= ts) return;
    const int A = pairs[2 * ip], B = pairs[2 * ip + 1];
    const TopologyDev& tp = bv.topo;
    const bool live = t < pv.nt[f];
    double acc[NCA * NCB];
#pragma unroll
    for (int i = 0; i < NCA * NCB; ++i) acc[i] = 0.0;
    if (live) {
        const double* xyz = bv.xyz + (size_t)f * tp.natoms * 3;
        const int atA = tp.sh_atom[A], atB = tp.sh_atom[B];
        const double ax = xyz[3 * atA], ay = xyz[3 * atA + 1], az = xyz[3 * atA + 2];
        const double bx = xyz[3 * atB], by = xyz[3 * atB + 1], bz = xyz[3 * atB + 2];
        const double ab2 = (ax - bx) * (ax - bx) + (ay - by) * (ay - by) + (az - bz) * (az - bz);
        const double* pt = pv.pts + ((size_t)f * ts + t) * 4;
        const double cx = pt[0], cy = pt[1], cz = pt[2];
        const int npa = tp.sh_nprim[A], npb = tp.sh_nprim[B];
        const double* ea = tp.exps + tp.sh_poff[A]; const double* ca = tp.coefs + tp.sh_poff[A];
        const double* eb = tp.exps + tp.sh_poff[B]; const double* cb = tp.coefs + tp.sh_poff[B];
        for (int ipr = 0; ipr < npa; ++ipr)
            for (int jpr = 0; jpr < npb; ++jpr) {
                const double a = ea[ipr], b = eb[jpr], p = a + b, ip_ = 1.0 / p;
                const double kab = exp(-a * b * ip_ * ab2) * ca[ipr] * cb[jpr];
                const double px = (a * ax + b * bx) * ip_, py = (a * ay + b * by) * ip_, pz = (a * az + b * bz) * ip_;
                E1D<LA, LB> ex, ey, ez;
                ex.build(px - ax, px - bx, 0.5 * ip_);
                ey.build(py - ay, py - by, 0.5 * ip_);
                ez.build(pz - az, pz - bz, 0.5 * ip_);
                double R[nherm(L)];
                hermite_r<L>(p, px - cx, py - cy, pz - cz, bv.boys, R);
                const double pref = 2.0 * M_PI * ip_ * kab;
                int k = 0;
#pragma unroll
                for (int i0 = LA; i0 >= 0; --i0)
#pragma unroll
                    for (int i1 = LA - i0; i1 >= 0; --i1) {
                        const int i2 = LA - i0 - i1;
#pragma unroll
                        for (int j0 = LB; j0 >= 0; --j0)
#pragma unroll
                            for (int j1 = LB - j0; j1 >= 0; --j1) {
                                const int j2 = LB - j0 - j1;
                                double v = 0.0;
#pragma unroll
                                for (int tt = 0; tt <= i0 + j0; ++tt)
#pragma unroll
                                    for (int u = 0; u <= i1 + j1; ++u)
#pragma unroll
                                        for (int w = 0; w <= i2 + j2; ++w)
                                            v += ex.get(i0, j0, tt) * ey.get(i1, j1, u) * ez.get(i2, j2, w) * R[hidx(tt, u, w)];
                                acc[k] += pref * v;
                                ++k;
                            }
                    }
            }
    }
    // cart -> sph, then the packed pair index (a shell with itself: the lower triangle of its block)
    constexpr int NSA = nsph(LA), NSB = nsph(LB);
    const int oa = tp.sh_aoff[A], ob = tp.sh_aoff[B];
    double* out = pv.A + ((size_t)f * ts + t) * (size_t)bv.npair;
#pragma unroll
    for (int i = 0; i < NSA; ++i)
#pragma unroll
        for (int j = 0; j < NSB; ++j) {
            double v = 0.0;
#pragma unroll
            for (int ia = 0; ia < NCA; ++ia) {
                const double wa = c2s_coef<LA>(bv.c2s, i, ia);
                if (wa == 0.0) continue;
#pragma unroll
                for (int ib = 0; ib < NCB; ++ib) v += wa * c2s_coef<LB>(bv.c2s, j, ib) * acc[ia * NCB + ib];
            }
            const int r = oa + i, c = ob + j;
            if (A == B && c > r) continue;
            const int mu = r > c ? r : c, nu = r > c ? c : r;
            out[(size_t)mu * (mu + 1) / 2 + nu] = v;
        }
}

// y = M x for the LOWER-TRIANGULAR stride x stride matrix M of every fragment (b = L^-1 v_nuc): one wave per row.  Only
// j <= row is read: the blocked factorisation never writes the upper triangle of L^-1.
__global__ void __launch_bounds__(PCM_NT) pcm_matvec_kernel(PcmView pv, const double* __restrict__ M, const double* __restrict__ x,
                                                            double* __restrict__ y)
{
    const int f = blockIdx.y, ts = pv.stride, lane = threadIdx.x & 63;
    const int row = blockIdx.x * (PCM_NT / 64) + (threadIdx.x >> 6);
    if (row >= ts) return;
    const double* __restrict__ m = M + ((size_t)f * ts + row) * ts;
    const double* __restrict__ xv = x + (size_t)f * ts;
    double s = 0.0;
    for (int j = lane; j <= row; j += 64) s += m[j] * xv[j];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    if (lane == 0) y[(size_t)f * ts + row] = s;
}

// ---- iteration ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void pcm_unpack(int idx, int& k, int& l)
{
    k = (int)((sqrt(8.0 * idx + 1.0) - 1.0) * 0.5);
    while ((k + 1) * (k + 2) / 2 <= idx) ++k;
    while (k * (k + 1) / 2 > idx) --k;
    l = idx - k * (k + 1) / 2;
}

// One workgroup per fragment that is not done: pass 1 c = b - B d (a wave per row of B), pass 2 V = f sum_P c_P B^P (a
// thread per packed pair, consecutive threads on consecutive pairs of a row).  Only the fragment's own rows are read.
__global__ void __launch_bounds__(PCM_NT) pcm_iter_kernel(BatchView bv, PcmView pv, int add)
{
    extern __shared__ double cl[];        // [stride] c, then the reduction scratch
    const int f = blockIdx.x, tid = threadIdx.x, n = bv.n, np = bv.npair, ts = pv.stride;
    if (bv.istate[4 * f] == ST_DONE) return;
    const int nt = pv.nt[f], lane = tid & 63, wave = tid >> 6;
    const size_t nn = (size_t)n * n;
    const double* __restrict__ Bf = pv.B + (size_t)f * ts * (size_t)np;
    const double* __restrict__ D = bv.D + (size_t)f * nn;
    const double* __restrict__ Db = bv.uhf ? bv.Db + (size_t)f * nn : nullptr;
    double* __restrict__ dp = pv.dp + (size_t)f * np;
    for (int idx = tid; idx < np; idx += PCM_NT) {
        int k, l;
        pcm_unpack(idx, k, l);
        double d = D[k * n + l];
        if (Db) d += Db[k * n + l];
        dp[idx] = k == l ? d : 2.0 * d;
    }
    __syncthreads();
    const double* __restrict__ bvec = pv.b + (size_t)f * ts;
    double* __restrict__ cg = pv.c + (size_t)f * ts;
    double e = 0.0;
    for (int R = wave; R < nt; R += PCM_NT / 64) {
        const double* __restrict__ row = Bf + (size_t)R * np;
        double s = 0.0;
        for (int idx = lane; idx < np; idx += 64) s += row[idx] * dp[idx];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
        const double c = bvec[R] - s;
        if (lane == 0) { cl[R] = c; cg[R] = c; e += c * c; }
    }
    for (int R = nt + tid; R < ts; R += PCM_NT) cg[R] = 0.0;
    double* red = cl + ts;
    if (lane == 0) red[wave] = e;
    __syncthreads();
    const double f_eps = pv.f;
    for (int idx = tid; idx < np; idx += PCM_NT) {
        double s = 0.0;
        for (int R = 0; R < nt; ++R) s += Bf[(size_t)R * np + idx] * cl[R];
        const double half = 0.5 * f_eps * s;
        int k, l;
        pcm_unpack(idx, k, l);
        for (int spin = 0; spin <= (bv.uhf ? 1 : 0); ++spin) {
            double* __restrict__ Vx = bv.Vxc + ((size_t)(spin ? bv.nfrag : 0) + f) * nn;
            if (add) {
                Vx[k * n + l] += half;
                if (k != l) Vx[l * n + k] += half;
            } else {
                Vx[k * n + l] = half;
                if (k != l) Vx[l * n + k] = half;
            }
        }
    }
    if (tid == 0) {
        double tot = 0.0;
        for (int w = 0; w < PCM_NT / 64; ++w) tot += red[w];
        const double e_pcm = -0.5 * f_eps * tot;
        // the step kernel adds scal[5] to the energy: after the quadrature it holds E_xc, which is kept apart here
        const double e_xc = add ? bv.scal[(size_t)f * 8 + 5] : 0.0;
        pv.scal[(size_t)f * 8] = e_pcm;
        pv.scal[(size_t)f * 8 + 1] = e_xc;
        bv.scal[(size_t)f * 8 + 5] = e_xc + e_pcm;
    }
}

// stage entry only: v = v_nuc - A d and q = -f L^-T c of the last iteration, a wave per tessera (q goes where b was)
__global__ void __launch_bounds__(PCM_NT) pcm_charges_kernel(BatchView bv, PcmView pv)
{
    const int f = blockIdx.y, ts = pv.stride, np = bv.npair, lane = threadIdx.x & 63;
    const int t = blockIdx.x * (PCM_NT / 64) + (threadIdx.x >> 6);
    if (t >= ts) return;
    double v = 0.0, q = 0.0;
    if (t < pv.nt[f]) {
        const double* __restrict__ row = pv.A + ((size_t)f * ts + t) * (size_t)np;
        const double* __restrict__ dp = pv.dp + (size_t)f * np;
        const double* __restrict__ Li = pv.Linv + (size_t)f * ts * ts;
        const double* __restrict__ c = pv.c + (size_t)f * ts;
        for (int idx = lane; idx < np; idx += 64) v += row[idx] * dp[idx];
        for (int P = t + lane; P < ts; P += 64) q += Li[(size_t)P * ts + t] * c[P];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) { v += __shfl_xor(v, off, 64); q += __shfl_xor(q, off, 64); }
        v = pv.vnuc[(size_t)f * ts + t] - v;
        q = -pv.f * q;
    }
    if (lane == 0) { pv.v[(size_t)f * ts + t] = v; pv.b[(size_t)f * ts + t] = q; }
}

// ---- launchers ------------------------------------------------------------------------------------------------------
template <int LA, int LB>
static void pcm_a_launch(const BatchView& bv, const PcmView& pv, const std::vector<int>& list, int* d, hipStream_t s)
{
    if (list.empty()) return;
    const int npairs = (int)list.size() / 2;
    (void)hipMemcpyAsync(d, list.data(), list.size() * sizeof(int), hipMemcpyHostToDevice, s);
    hipLaunchKernelGGL((pcm_a_kernel<LA, LB>), dim3((pv.stride + 63) / 64, npairs, bv.nfrag), dim3(64), 0, s, bv, pv, d);
}

void launch_pcm_setup(const BatchView& bv, const PcmView& pv, const Topology& topo, hipStream_t s)
{
    const int ts = pv.stride, nf = bv.nfrag;
    const size_t mm = (size_t)ts * ts;
    hipLaunchKernelGGL(pcm_s_kernel, dim3((unsigned)((mm + PCM_NT - 1) / PCM_NT), nf), dim3(PCM_NT), 0, s, pv);
    hipLaunchKernelGGL(pcm_vnuc_kernel, dim3((ts + PCM_NT - 1) / PCM_NT, nf), dim3(PCM_NT), 0, s, bv, pv);
    // the shell pairs by class, as the one-electron stage buckets them; the host lists outlive the asynchronous uploads
    // (the next call of this slot comes after its stream has been drained)
    static DevicePool scratch_slot[2];
    static std::vector<int> bucket_slot[2][LMAX_AO + 1][LMAX_AO + 1];
    auto& bucket = bucket_slot[bv.slot & 1];
    for (auto& row : bucket) for (auto& b : row) b.clear();
    for (size_t k = 0; k + 1 < topo.pairs.size(); k += 2) {
        int A = topo.pairs[k], B = topo.pairs[k + 1];
        int la = topo.shells[A].l, lb = topo.shells[B].l;
        if (la < lb) { std::swap(A, B); std::swap(la, lb); }
        bucket[la][lb].push_back(A);
        bucket[la][lb].push_back(B);
    }
    int* d = (int*)scratch_slot[bv.slot & 1].ensure((topo.pairs.size() + 16) * sizeof(int));
    size_t off = 0;
#define PCM_CASE(a, b) pcm_a_launch<a, b>(bv, pv, bucket[a][b], d + off, s); off += bucket[a][b].size();
    PCM_CASE(0, 0) PCM_CASE(1, 0) PCM_CASE(1, 1) PCM_CASE(2, 0) PCM_CASE(2, 1) PCM_CASE(2, 2)
    PCM_CASE(3, 0) PCM_CASE(3, 1) PCM_CASE(3, 2) PCM_CASE(3, 3)
#undef PCM_CASE
    // S = L L^T in place, L^-1 and B = L^-1 A by the density fitting's kernels on a view of the PCM arrays; the flag of
    // a fragment whose factorisation failed lands in pv.scal[8 f + 7]
    (void)hipMemsetAsync(pv.scal, 0, sizeof(double) * 8 * (size_t)nf, s);
    BatchView fit = bv;
    fit.naux = ts;
    fit.df_metric = pv.S; fit.df_linv = pv.Linv; fit.df_work = pv.work; fit.df_a3 = pv.A; fit.df_b = pv.B;
    fit.scal = pv.scal;
    launch_df_fit(fit, s);
    hipLaunchKernelGGL(pcm_matvec_kernel, dim3((ts + PCM_NT / 64 - 1) / (PCM_NT / 64), nf), dim3(PCM_NT), 0, s, pv, pv.Linv, pv.vnuc, pv.b);
}

void launch_pcm_iteration(const BatchView& bv, const PcmView& pv, bool add, hipStream_t s)
{
    const size_t lds = sizeof(double) * ((size_t)pv.stride + 8);
    hipLaunchKernelGGL(pcm_iter_kernel, dim3(bv.nfrag), dim3(PCM_NT), lds, s, bv, pv, add ? 1 : 0);
}

void launch_pcm_charges(const BatchView& bv, const PcmView& pv, hipStream_t s)
{
    hipLaunchKernelGGL(pcm_charges_kernel, dim3((pv.stride + PCM_NT / 64 - 1) / (PCM_NT / 64), bv.nfrag), dim3(PCM_NT), 0, s, bv, pv);
}

}  // namespace mqc
