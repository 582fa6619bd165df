// hermite_records.hpp -- the Hermite-record stage shared by kern_esp.hip and kern_grad_pc.hip.
//
// The potential of a density at a point r, and its derivatives, are sums over primitive pairs of a Hermite density
// X_tuv against the Hermite-Coulomb integrals R_tuv(p, P - r).  Everything that does not depend on r is formed once per
// (shell pair a >= b, fragment) and kept as a RECORD per primitive pair:
//     {p, Px, Py, Pz, X_tuv (t + u + v <= L)}                                                       L = LA + LB
//     {p, Px, Py, Pz, atom of a, atom of b, X_tuv (order L), XA^x_tuv, XA^y_tuv, XA^z_tuv (order L + 1)}    (DERIV)
// X is the Cartesian density block folded with the E coefficients, XA^c the same block folded with
// 2a E(a + 1_c, b) - a_c E(a - 1_c, b) (the function on A differentiated along c); the prefactor (2 pi / p) K_ab c_a c_b
// is folded in.  p = 0 marks a record of a screened primitive pair, which the point kernels skip.
//
// hermite_density_kernel<LA, LB, DERIV> runs one wave per (shell pair, fragment): the density block goes to Cartesian
// components in LDS, every lane takes primitive pairs and writes their records.  Records are grouped by L and, with
// by_atom_pair, ordered by atom pair inside a group (hermite_lists); launch_hermite_density issues the ten classes.
// The per-pair arithmetic is __host__ __device__: tests/host/check_device_math.cpp runs it without a GPU.
#pragma once
#include "engine.hpp"
#include "md_integrals.hpp"
#include <algorithm>
#include <string>
#include <vector>

namespace mqc {

constexpr int HERMITE_LMAX = 2 * KERNEL_LMAX;   // f shells on both sides

MQC_HD constexpr int hermite_head(bool deriv) { return deriv ? 6 : 4; }
MQC_HD constexpr int hermite_rec_doubles(int L, bool deriv) { return hermite_head(deriv) + nherm(L) + (deriv ? 3 * nherm(L + 1) : 0); }

// the blocks of a DERIV record are folded one at a time: the accumulators of a finished block are dead before the next
#if defined(__HIP_DEVICE_COMPILE__)
#define HERMITE_FENCE() __builtin_amdgcn_sched_barrier(0)
#else
#define HERMITE_FENCE() ((void)0)
#endif

// The coefficient of axis AX in block C: C < 0 the plain Hermite density (order LA + LB); C = 0, 1, 2 the function on A
// differentiated along axis C (order LA + LB + 1), which needs E tables one unit higher on A (EA = LA + 1).
template <int EA, int LB, int C, int AX>
MQC_HD double hermite_coef(const E1D<EA, LB>& e, int i, int j, int t, double a2)
{
    if constexpr (C == AX) {
        double v = a2 * e.get(i + 1, j, t);
        if (i > 0) v -= i * e.get(i - 1, j, t);      // E(i - 1, j, t) is zero above t = i - 1 + j (build() zeroes the table)
        return v;
    } else {
        return e.get(i, j, t);
    }
}

// One block of a record: the Cartesian density block dc folded with the E coefficients of extent EA on A.
template <int EA, int LA, int LB, int C>
MQC_HD void hermite_fold(const double* __restrict__ dc, const E1D<EA, LB>& ex, const E1D<EA, LB>& ey, const E1D<EA, LB>& ez, double a2,
                         double pref, double* __restrict__ out)
{
    static_assert(C < 0 || EA > LA, "a derivative block reads E(i + 1, j, t)");
    constexpr int NH = nherm(LA + LB + (C >= 0 ? 1 : 0));
    constexpr int UX = C == 0 ? 1 : 0, UY = C == 1 ? 1 : 0, UZ = C == 2 ? 1 : 0;
    double X[NH];
#pragma unroll
    for (int k = 0; k < NH; ++k) X[k] = 0.0;
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
                    const double d = dc[k];
#pragma unroll
                    for (int t = 0; t <= i0 + j0 + UX; ++t) {
                        const double dx = d * hermite_coef<EA, LB, C, 0>(ex, i0, j0, t, a2);
#pragma unroll
                        for (int u = 0; u <= i1 + j1 + UY; ++u) {
                            const double dxy = dx * hermite_coef<EA, LB, C, 1>(ey, i1, j1, u, a2);
#pragma unroll
                            for (int w = 0; w <= i2 + j2 + UZ; ++w) X[hidx(t, u, w)] += dxy * hermite_coef<EA, LB, C, 2>(ez, i2, j2, w, a2);
                        }
                    }
                    ++k;
                }
        }
#pragma unroll
    for (int h = 0; h < NH; ++h) out[h] = pref * X[h];
}

// The record r of one primitive pair (exponents a, b, coefficients ca, cb) of a shell pair on centres A and B.
template <int LA, int LB, bool DERIV>
MQC_HD void hermite_record(const double* __restrict__ dc, double a, double b, double ca, double cb, double ax, double ay, double az, double bx,
                           double by, double bz, int atA, int atB, double* __restrict__ r)
{
    constexpr int EA = DERIV ? LA + 1 : LA, HEAD = hermite_head(DERIV);
    const double ab2 = (ax - bx) * (ax - bx) + (ay - by) * (ay - by) + (az - bz) * (az - bz);
    const double p = a + b, ip_ = 1.0 / p;
    const double ex_arg = a * b * ip_ * ab2;
    if (ex_arg > PRIM_EXP_CUTOFF) { r[0] = 0.0; return; }          // p = 0 marks a record the point kernels skip
    const double pref = 2.0 * M_PI * ip_ * exp(-ex_arg) * ca * cb;
    const double px = (a * ax + b * bx) * ip_, py = (a * ay + b * by) * ip_, pz = (a * az + b * bz) * ip_;
    E1D<EA, LB> ex, ey, ez;
    ex.build(px - ax, px - bx, 0.5 * ip_);
    ey.build(py - ay, py - by, 0.5 * ip_);
    ez.build(pz - az, pz - bz, 0.5 * ip_);
    r[0] = p; r[1] = px; r[2] = py; r[3] = pz;
    hermite_fold<EA, LA, LB, -1>(dc, ex, ey, ez, 2.0 * a, pref, r + HEAD);
    if constexpr (DERIV) {
        constexpr int NH = nherm(LA + LB), NH1 = nherm(LA + LB + 1);
        r[4] = (double)atA; r[5] = (double)atB;
        HERMITE_FENCE();
        hermite_fold<EA, LA, LB, 0>(dc, ex, ey, ez, 2.0 * a, pref, r + HEAD + NH);
        HERMITE_FENCE();
        hermite_fold<EA, LA, LB, 1>(dc, ex, ey, ez, 2.0 * a, pref, r + HEAD + NH + NH1);
        HERMITE_FENCE();
        hermite_fold<EA, LA, LB, 2>(dc, ex, ey, ez, 2.0 * a, pref, r + HEAD + NH + 2 * NH1);
    }
}

// Element e of the Cartesian density block of the shell pair at AO offsets (oa, ob) of the spherical density D [n][n];
// an off-diagonal shell pair stands for (a, b) and (b, a)
template <int LA, int LB>
MQC_HD double cart_density_element(const double* __restrict__ D, int n, int oa, int ob, bool offdiag, const double* __restrict__ c2s, int e)
{
    constexpr int NCB = ncart(LB), NSA = nsph(LA), NSB = nsph(LB);
    const int ia = e / NCB, ib = e % NCB;
    double acc = 0.0;
    for (int i = 0; i < NSA; ++i) {
        const double wa = c2s_coef<LA>(c2s, i, ia);
        if (wa == 0.0) continue;
        for (int j = 0; j < NSB; ++j) {
            const double wb = c2s_coef<LB>(c2s, j, ib);
            if (wb == 0.0) continue;
            double d = D[(size_t)(oa + i) * n + ob + j];
            if (offdiag) d += D[(size_t)(ob + j) * n + oa + i];
            acc += wa * wb * d;
        }
    }
    return acc;
}

struct HermiteView {
    const double* xyz;       // [nfrag][natoms][3]
    const double* D;         // [nfrag][n*n]
    double* rec;             // [nfrag][rec_stride]: per L group, records of hermite_rec_doubles(L, DERIV)
    size_t rec_stride;
    int n;
};

template <int LA, int LB, bool DERIV>
__global__ void __launch_bounds__(64) hermite_density_kernel(TopologyDev tp, HermiteView hv, const double* __restrict__ c2s,
                                                             const int* __restrict__ pairs /* A, B, first record */, size_t group_off)
{
    constexpr int NCA = ncart(LA), NCB = ncart(LB), RD = hermite_rec_doubles(LA + LB, DERIV);
    __shared__ double dc[NCA * NCB];
    const int f = blockIdx.y, ip = blockIdx.x, lane = threadIdx.x;
    const int A = pairs[3 * ip], B = pairs[3 * ip + 1], rec0 = pairs[3 * ip + 2];
    // the pair's wave-uniform data first: nothing is stored before these loads, so they go through the scalar path
    const double* xyz = hv.xyz + (size_t)f * tp.natoms * 3;
    const int atA = tp.sh_atom[A], atB = tp.sh_atom[B];
    const double ax = xyz[3 * atA], ay = xyz[3 * atA + 1], az = xyz[3 * atA + 2];
    const double bx = xyz[3 * atB], by = xyz[3 * atB + 1], bz = xyz[3 * atB + 2];
    const int npa = tp.sh_nprim[A], npb = tp.sh_nprim[B];
    const double* ea = tp.exps + tp.sh_poff[A]; const double* ca = tp.coefs + tp.sh_poff[A];
    const double* eb = tp.exps + tp.sh_poff[B]; const double* cb = tp.coefs + tp.sh_poff[B];
    const double* D = hv.D + (size_t)f * hv.n * hv.n;
    const int oa = tp.sh_aoff[A], ob = tp.sh_aoff[B];
    for (int e = lane; e < NCA * NCB; e += 64) dc[e] = cart_density_element<LA, LB>(D, hv.n, oa, ob, A != B, c2s, e);
    __syncthreads();
    double* recs = hv.rec + (size_t)f * hv.rec_stride + group_off + (size_t)rec0 * RD;
    for (int pp = lane; pp < npa * npb; pp += 64) {
        const int ipa = pp / npb, jp = pp % npb;
        hermite_record<LA, LB, DERIV>(dc, ea[ipa], eb[jp], ca[ipa], cb[jp], ax, ay, az, bx, by, bz, atA, atB, recs + (size_t)pp * RD);
    }
}

// record counts per L group and the (A, B, first record) triples per (la, lb) class
struct HermiteLists {
    std::vector<int> cls[KERNEL_LMAX + 1][KERNEL_LMAX + 1];
    int nrec[HERMITE_LMAX + 1] = {};
    size_t group_off[HERMITE_LMAX + 1] = {};
    size_t rec_stride = 0;
};

// by_atom_pair: the records of an L group are ordered by atom pair, so that a point kernel meets each pair as one run
// per group; otherwise they keep the topology's order
template <bool DERIV>
HermiteLists hermite_lists(const Topology& topo, bool by_atom_pair)
{
    struct P { int A, B, la, lb, key; };
    std::vector<P> byL[HERMITE_LMAX + 1];
    for (size_t k = 0; k + 1 < topo.pairs.size(); k += 2) {
        int A = topo.pairs[k], B = topo.pairs[k + 1];
        int la = topo.shells[A].l, lb = topo.shells[B].l;
        if (la < lb) { std::swap(A, B); std::swap(la, lb); }
        byL[la + lb].push_back({A, B, la, lb, topo.shells[A].atom * topo.natoms + topo.shells[B].atom});
    }
    HermiteLists hl;
    size_t off = 0;
    for (int L = 0; L <= HERMITE_LMAX; ++L) {
        if (by_atom_pair) std::stable_sort(byL[L].begin(), byL[L].end(), [](const P& x, const P& y) { return x.key < y.key; });
        for (const P& p : byL[L]) {
            auto& c = hl.cls[p.la][p.lb];
            c.push_back(p.A); c.push_back(p.B); c.push_back(hl.nrec[L]);
            hl.nrec[L] += topo.shells[p.A].nprim * topo.shells[p.B].nprim;
        }
        hl.group_off[L] = off;
        off += (size_t)hl.nrec[L] * hermite_rec_doubles(L, DERIV);
    }
    hl.rec_stride = (off + 31) & ~size_t(31);
    return hl;
}

// doubles of records per fragment (the order of the records does not change their number)
template <bool DERIV>
size_t hermite_record_doubles(const Topology& topo) { return hermite_lists<DERIV>(topo, false).rec_stride; }

// The record stage of one chunk of nfrag fragments: uploads the class lists through the caller's pool and host vector
// (which must stay alive while the upload is in flight) and issues one launch per (la, lb) class.
template <bool DERIV>
bool launch_hermite_density(const TopologyDev& td, const HermiteView& hv, int nfrag, const double* c2s, const HermiteLists& hl, DevicePool& pool,
                            std::vector<int>& host_lists, hipStream_t s, std::string& err)
{
    if (nfrag > 65535) { err = "Hermite records: chunk above the launch grid's limit"; return false; }
    host_lists.clear();
    for (int la = 0; la <= KERNEL_LMAX; ++la)
        for (int lb = 0; lb <= la; ++lb) host_lists.insert(host_lists.end(), hl.cls[la][lb].begin(), hl.cls[la][lb].end());
    const int* d_lists = (const int*)pool.ensure((host_lists.size() + 16) * sizeof(int));
    if (!d_lists) { err = "out of device memory (Hermite record lists)"; return false; }
    (void)hipMemcpyAsync((void*)d_lists, host_lists.data(), host_lists.size() * sizeof(int), hipMemcpyHostToDevice, s);
    size_t off = 0;
#define HERMITE_D(a, b)                                                                                                                  \
    if (const size_t len = hl.cls[a][b].size()) {                                                                                        \
        hipLaunchKernelGGL((hermite_density_kernel<a, b, DERIV>), dim3((unsigned)(len / 3), nfrag), dim3(64), 0, s, td, hv, c2s, d_lists + off, \
                           hl.group_off[a + b]);                                                                                         \
        off += len;                                                                                                                      \
    }
    HERMITE_D(0, 0) HERMITE_D(1, 0) HERMITE_D(1, 1) HERMITE_D(2, 0) HERMITE_D(2, 1) HERMITE_D(2, 2) HERMITE_D(3, 0) HERMITE_D(3, 1) HERMITE_D(3, 2)
    HERMITE_D(3, 3)
#undef HERMITE_D
    return true;
}

}  // namespace mqc
