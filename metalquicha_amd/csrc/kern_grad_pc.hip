// kern_grad_pc.hip -- the point charges' part of the analytic gradient of an embedded fragment, for a whole batch.
//
// The embedding operator u = -sum_g q_g (a| 1/|r - R_g| |b) sits in the one-electron Hamiltonian, so the energy-weighted
// density of grad1e_kernel already carries it; what is left is sum_ab Dt_ab du_ab/dR.  For a shell pair (a on A, b on B)
// and a charge g there are three derivatives: v_A (the function on A moves), v_C (the charge moves) and, by translational
// invariance, v_B = -(v_A + v_C).  grad1e_kernel takes one centre at a time per wave (a wave-cooperative Boys evaluation
// per centre): fine for the nuclei, hopeless for the hundreds of charges of an FMO / EE-MBE fragment.  The two stages of
// kern_esp.hip instead:
//   gradpc_hermite_density_kernel<LA, LB>  one wave per (shell pair a >= b, fragment), a lane per primitive pair: the
//       Cartesian density block is folded with the E coefficients into a record
//           {p, P, atom of a, atom of b, X_tuv (order L), XA^x_tuv, XA^y_tuv, XA^z_tuv (order L + 1)},   L = LA + LB,
//       X the ESP record, XA^c the same block folded with 2a E(a + 1_c, b) - a_c E(a - 1_c, b); (2 pi / p) K_ab c_a c_b
//       folded in.  Records are grouped by L and, inside a group, by atom pair.
//   gradpc_points_kernel<L>  lane = charge, workgroup = (tile of GRADPC_TILE charges, fragment): records staged through
//       LDS; per record one Boys evaluation F_0..F_{L+1}, the Hermite recursion in registers and six dot products,
//           v_A^c = -q sum XA^c_tuv R_tuv,      v_C^c = +q sum X_tuv R_{tuv + 1_c}      (d R_tuv(P - C) / dC_c = -R_{tuv + 1_c}).
//       A lane owns its charge's gradient (plain stores, launches of one chunk are ordered by the stream); the atoms'
//       parts are kept per lane over a run of records of one atom pair, summed over the tile once per run and added with
//       atomicAdd into the gradient grad1e_kernel and eri_grad_kernel accumulate.  Charges with q = 0 are skipped.
// L + 1 reaches 7 for f-f pairs; the same register kernel serves every L (no private segment at L = 6).
#include "engine.hpp"
#include "md_integrals.hpp"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

namespace mqc {

#if defined(__HIP_DEVICE_COMPILE__)
#define GRADPC_FENCE() __builtin_amdgcn_sched_barrier(0)
#else
#define GRADPC_FENCE() ((void)0)
#endif

constexpr int GRADPC_LMAX = 2 * KERNEL_LMAX;    // f shells on both sides: R_tuv up to order 7
constexpr int GRADPC_TILE = 64;                 // charges per workgroup: one wave, the run sums are wave reductions
constexpr int GRADPC_STAGE_DOUBLES = 4096;      // LDS staging buffer of the point kernel, 32 KB
constexpr int GRADPC_HEAD = 6;                  // p, Px, Py, Pz, atom of a, atom of b

__host__ __device__ constexpr int gradpc_rec_doubles(int L) { return GRADPC_HEAD + nherm(L) + 3 * nherm(L + 1); }

struct GradPcView {
    const double* xyz;       // [nfrag][natoms][3]
    const double* D;         // [nfrag][n*n] total density
    double* rec;             // [nfrag][rec_stride]: per L group, records of gradpc_rec_doubles(L)
    const double* pc;        // [npc][x, y, z, q][nfrag], fragment fastest (BatchView::pc)
    double* grad;            // [nfrag][natoms][3], accumulated
    double* pcgrad;          // [nfrag][npc][3]
    size_t rec_stride;
    int npc, nfrag, n, natoms;
};

// One block of a record: C < 0 the plain Hermite density X (order LA + LB); C = 0, 1, 2 the block of the function on A
// differentiated along axis C (order LA + LB + 1).  The E tables are built one unit higher on A.
template <int LA, int LB, int C, int AX>
__device__ __forceinline__ double gradpc_coef(const E1D<LA + 1, LB>& e, int i, int j, int t, double a2)
{
    if constexpr (C == AX) {
        double v = a2 * e.get(i + 1, j, t);
        if (i > 0) v -= i * e.get(i - 1, j, t);      // E(i - 1, j, t) is zero above t = i - 1 + j (build() zeroes the table)
        return v;
    } else {
        return e.get(i, j, t);
    }
}

template <int LA, int LB, int C>
__device__ __forceinline__ void gradpc_fold(const double* __restrict__ dc, const E1D<LA + 1, LB>& ex, const E1D<LA + 1, LB>& ey,
                                            const E1D<LA + 1, LB>& ez, double a2, double pref, double* __restrict__ out)
{
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
                        const double dx = d * gradpc_coef<LA, LB, C, 0>(ex, i0, j0, t, a2);
#pragma unroll
                        for (int u = 0; u <= i1 + j1 + UY; ++u) {
                            const double dxy = dx * gradpc_coef<LA, LB, C, 1>(ey, i1, j1, u, a2);
#pragma unroll
                            for (int w = 0; w <= i2 + j2 + UZ; ++w) X[hidx(t, u, w)] += dxy * gradpc_coef<LA, LB, C, 2>(ez, i2, j2, w, a2);
                        }
                    }
                    ++k;
                }
        }
#pragma unroll
    for (int h = 0; h < NH; ++h) out[h] = pref * X[h];
}

template <int LA, int LB>
__global__ void __launch_bounds__(64) gradpc_hermite_density_kernel(TopologyDev tp, GradPcView gv, const double* __restrict__ c2s,
                                                                     const int* __restrict__ pairs /* A, B, first record */, size_t group_off)
{
    constexpr int NCA = ncart(LA), NCB = ncart(LB), NSA = nsph(LA), NSB = nsph(LB);
    constexpr int L = LA + LB, NH = nherm(L), NH1 = nherm(L + 1), RD = gradpc_rec_doubles(L);
    __shared__ double dc[NCA * NCB];
    const int f = blockIdx.y, ip = blockIdx.x, lane = threadIdx.x;
    const int A = pairs[3 * ip], B = pairs[3 * ip + 1], rec0 = pairs[3 * ip + 2];
    const int n = gv.n;
    const double* D = gv.D + (size_t)f * n * n;
    const int oa = tp.sh_aoff[A], ob = tp.sh_aoff[B];
    // Cartesian density block; an off-diagonal shell pair stands for (a, b) and (b, a)
    for (int e = lane; e < NCA * NCB; e += 64) {
        const int ia = e / NCB, ib = e % NCB;
        double acc = 0.0;
        for (int i = 0; i < NSA; ++i) {
            const double wa = c2s_coef<LA>(c2s, i, ia);
            if (wa == 0.0) continue;
            for (int j = 0; j < NSB; ++j) {
                const double wb = c2s_coef<LB>(c2s, j, ib);
                if (wb == 0.0) continue;
                double d = D[(size_t)(oa + i) * n + ob + j];
                if (A != B) d += D[(size_t)(ob + j) * n + oa + i];
                acc += wa * wb * d;
            }
        }
        dc[e] = acc;
    }
    __syncthreads();
    const double* xyz = gv.xyz + (size_t)f * tp.natoms * 3;
    const int atA = tp.sh_atom[A], atB = tp.sh_atom[B];
    const double ax = xyz[3 * atA], ay = xyz[3 * atA + 1], az = xyz[3 * atA + 2];
    const double bx = xyz[3 * atB], by = xyz[3 * atB + 1], bz = xyz[3 * atB + 2];
    const double ab2 = (ax - bx) * (ax - bx) + (ay - by) * (ay - by) + (az - bz) * (az - bz);
    const int npa = tp.sh_nprim[A], npb = tp.sh_nprim[B];
    const double* ea = tp.exps + tp.sh_poff[A]; const double* ca = tp.coefs + tp.sh_poff[A];
    const double* eb = tp.exps + tp.sh_poff[B]; const double* cb = tp.coefs + tp.sh_poff[B];
    double* recs = gv.rec + (size_t)f * gv.rec_stride + group_off + (size_t)rec0 * RD;
    for (int pp = lane; pp < npa * npb; pp += 64) {
        const int ipa = pp / npb, jp = pp % npb;
        const double a = ea[ipa], b = eb[jp], p = a + b, ip_ = 1.0 / p;
        double* r = recs + (size_t)pp * RD;
        const double ex_arg = a * b * ip_ * ab2;
        if (ex_arg > PRIM_EXP_CUTOFF) { r[0] = 0.0; continue; }       // p = 0 marks a record the point kernel skips
        const double pref = 2.0 * M_PI * ip_ * exp(-ex_arg) * ca[ipa] * cb[jp];
        const double px = (a * ax + b * bx) * ip_, py = (a * ay + b * by) * ip_, pz = (a * az + b * bz) * ip_;
        E1D<LA + 1, LB> ex, ey, ez;
        ex.build(px - ax, px - bx, 0.5 * ip_);
        ey.build(py - ay, py - by, 0.5 * ip_);
        ez.build(pz - az, pz - bz, 0.5 * ip_);
        r[0] = p; r[1] = px; r[2] = py; r[3] = pz; r[4] = (double)atA; r[5] = (double)atB;
        // one block at a time: the accumulators of a finished block are dead before the next one starts
        gradpc_fold<LA, LB, -1>(dc, ex, ey, ez, 2.0 * a, pref, r + GRADPC_HEAD);
        GRADPC_FENCE();
        gradpc_fold<LA, LB, 0>(dc, ex, ey, ez, 2.0 * a, pref, r + GRADPC_HEAD + NH);
        GRADPC_FENCE();
        gradpc_fold<LA, LB, 1>(dc, ex, ey, ez, 2.0 * a, pref, r + GRADPC_HEAD + NH + NH1);
        GRADPC_FENCE();
        gradpc_fold<LA, LB, 2>(dc, ex, ey, ez, 2.0 * a, pref, r + GRADPC_HEAD + NH + 2 * NH1);
    }
}

__device__ __forceinline__ double gradpc_wave_sum(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

template <int L>
__global__ void __launch_bounds__(GRADPC_TILE) gradpc_points_kernel(GradPcView gv, const double* __restrict__ boys_table, size_t group_off,
                                                                    int nrec)
{
    constexpr int NH = nherm(L), NH1 = nherm(L + 1), RD = gradpc_rec_doubles(L);
    constexpr int CHUNK = GRADPC_STAGE_DOUBLES / RD;      // records per staged chunk (9 at L = 6)
    static_assert(CHUNK >= 1, "a record must fit the staging buffer");
    __shared__ double stage[CHUNK * RD];
    const int f = blockIdx.y, lane = threadIdx.x;
    const int g = blockIdx.x * GRADPC_TILE + lane;
    double cx = 0.0, cy = 0.0, cz = 0.0, q = 0.0;
    if (g < gv.npc) {
        const double* c = gv.pc + (size_t)g * 4 * gv.nfrag + f;
        cx = c[0]; cy = c[(size_t)gv.nfrag]; cz = c[2 * (size_t)gv.nfrag]; q = c[3 * (size_t)gv.nfrag];
    }
    const bool live = q != 0.0;
    const double* recs = gv.rec + (size_t)f * gv.rec_stride + group_off;
    double* gf = gv.grad + (size_t)f * gv.natoms * 3;
    double gA[3] = {0.0, 0.0, 0.0}, gB[3] = {0.0, 0.0, 0.0}, gC[3] = {0.0, 0.0, 0.0};
    int curA = -1, curB = -1;                              // atom pair of the run being summed (wave-uniform)
    auto flush = [&]() {
        if (curA < 0) return;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double ta = gradpc_wave_sum(gA[c]), tb = gradpc_wave_sum(gB[c]);
            if (lane == 0) {
                if (ta != 0.0) atomicAdd(&gf[3 * curA + c], ta);
                if (tb != 0.0) atomicAdd(&gf[3 * curB + c], tb);
            }
            gA[c] = 0.0; gB[c] = 0.0;
        }
    };
    for (int r0 = 0; r0 < nrec; r0 += CHUNK) {
        const int nr = min(CHUNK, nrec - r0);
        __syncthreads();
        for (int e = lane; e < nr * RD; e += GRADPC_TILE) stage[e] = recs[(size_t)r0 * RD + e];
        __syncthreads();
        for (int k = 0; k < nr; ++k) {
            const double* rec = stage + k * RD;
            const double p = rec[0];
            if (p == 0.0) continue;
            const int atA = (int)rec[4], atB = (int)rec[5];
            if (atA != curA || atB != curB) { flush(); curA = atA; curB = atB; }
            if (!live) continue;
            double R[NH1];
            hermite_r<L + 1>(p, rec[1] - cx, rec[2] - cy, rec[3] - cz, boys_table, R);
            const double* x = rec + GRADPC_HEAD;
            const double* xa = x + NH;
            double va[3] = {0.0, 0.0, 0.0}, vc[3] = {0.0, 0.0, 0.0};
#pragma unroll
            for (int h = 0; h < NH1; ++h) {
                va[0] += xa[h] * R[h]; va[1] += xa[NH1 + h] * R[h]; va[2] += xa[2 * NH1 + h] * R[h];
            }
#pragma unroll
            for (int N = 0; N <= L; ++N)
#pragma unroll
                for (int t = N; t >= 0; --t)
#pragma unroll
                    for (int u = N - t; u >= 0; --u) {
                        const int v = N - t - u;
                        const double xv = x[hidx(t, u, v)];
                        vc[0] += xv * R[hidx(t + 1, u, v)]; vc[1] += xv * R[hidx(t, u + 1, v)]; vc[2] += xv * R[hidx(t, u, v + 1)];
                    }
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const double a = -q * va[c], cc = q * vc[c];
                gA[c] += a; gC[c] += cc; gB[c] -= a + cc;      // translational invariance of the three-centre integral
            }
        }
    }
    flush();
    if (g < gv.npc) {
        double* out = gv.pcgrad + ((size_t)f * gv.npc + g) * 3;
        if (L == 0) { out[0] = gC[0]; out[1] = gC[1]; out[2] = gC[2]; }         // the L = 0 launch initialises
        else if (live) { out[0] += gC[0]; out[1] += gC[1]; out[2] += gC[2]; }
    }
}

// record counts per L group and the (A, B, first record) triples per (la, lb) class; records of an L group are ordered
// by atom pair, so that the point kernel meets each pair as one run per group
struct GradPcLists {
    std::vector<int> cls[KERNEL_LMAX + 1][KERNEL_LMAX + 1];
    int nrec[GRADPC_LMAX + 1] = {};
    size_t group_off[GRADPC_LMAX + 1] = {};
    size_t rec_stride = 0;
};

static void gradpc_lists(const Topology& topo, GradPcLists& gl)
{
    struct P { int A, B, la, lb, key; };
    std::vector<P> byL[GRADPC_LMAX + 1];
    for (size_t k = 0; k + 1 < topo.pairs.size(); k += 2) {
        int A = topo.pairs[k], B = topo.pairs[k + 1];
        int la = topo.shells[A].l, lb = topo.shells[B].l;
        if (la < lb) { std::swap(A, B); std::swap(la, lb); }
        byL[la + lb].push_back({A, B, la, lb, topo.shells[A].atom * topo.natoms + topo.shells[B].atom});
    }
    for (int L = 0; L <= GRADPC_LMAX; ++L) {
        std::stable_sort(byL[L].begin(), byL[L].end(), [](const P& x, const P& y) { return x.key < y.key; });
        for (const P& p : byL[L]) {
            auto& c = gl.cls[p.la][p.lb];
            c.push_back(p.A); c.push_back(p.B); c.push_back(gl.nrec[L]);
            gl.nrec[L] += topo.shells[p.A].nprim * topo.shells[p.B].nprim;
        }
    }
    size_t off = 0;
    for (int L = 0; L <= GRADPC_LMAX; ++L) { gl.group_off[L] = off; off += (size_t)gl.nrec[L] * gradpc_rec_doubles(L); }
    gl.rec_stride = (off + 31) & ~size_t(31);
}

size_t gradpc_record_doubles(const Topology& topo)
{
    GradPcLists gl;
    gradpc_lists(topo, gl);
    return gl.rec_stride;
}

template <int LA, int LB>
static void gradpc_launch_density(const TopologyDev& td, const GradPcView& gv, const double* c2s, const GradPcLists& gl, const int* d_lists,
                                  size_t& list_off, hipStream_t s)
{
    const auto& c = gl.cls[LA][LB];
    if (c.empty()) return;
    const int npairs = (int)c.size() / 3;
    for (int y0 = 0; y0 < gv.nfrag; y0 += 65535) {     // grid.y limit
        GradPcView v = gv;
        const int ny = std::min(65535, gv.nfrag - y0);
        v.xyz += (size_t)y0 * td.natoms * 3; v.D += (size_t)y0 * gv.n * gv.n; v.rec += (size_t)y0 * gv.rec_stride;
        hipLaunchKernelGGL((gradpc_hermite_density_kernel<LA, LB>), dim3(npairs, ny), dim3(64), 0, s, td, v, c2s, d_lists + list_off,
                           gl.group_off[LA + LB]);
    }
    list_off += c.size();
}

template <int L>
static void gradpc_launch_points(const GradPcView& gv, const double* boys_table, const GradPcLists& gl, hipStream_t s)
{
    if (L > 0 && gl.nrec[L] == 0) return;
    const int tiles = (gv.npc + GRADPC_TILE - 1) / GRADPC_TILE;
    // the fragment index of the charge array is the lane-fastest one: the view keeps the chunk's base and the kernel
    // takes blockIdx.y as the fragment, so a chunk is one launch (chunks hold at most 60000 fragments, below grid.y's limit)
    hipLaunchKernelGGL((gradpc_points_kernel<L>), dim3(tiles, gv.nfrag), dim3(GRADPC_TILE), 0, s, gv, boys_table, gl.group_off[L], gl.nrec[L]);
}

// The charges' part of the gradient of one chunk, after launch_gradient: adds the atoms' part into d_grad [nfrag][natoms][3]
// and writes the sites' gradient into d_pcgrad [nfrag][npc][3].  Dtot: the total density launch_gradient used; d_rec holds
// nfrag x gradpc_record_doubles(topo).
bool launch_pc_gradient(const BatchView& bv, const Topology& topo, const double* Dtot, double* d_grad, double* d_pcgrad, double* d_rec,
                        hipStream_t s, std::string& err)
{
    if (bv.npc <= 0 || !bv.pc) { err = "point-charge gradient: the fragment carries no charges"; return false; }
    if (topo.lmax > KERNEL_LMAX) { err = "analytic gradients cover s, p, d and f shells"; return false; }
    if (bv.nfrag > 65535) { err = "point-charge gradient: chunk above the launch grid's limit"; return false; }
    static DevicePool list_pool[2];
    static std::vector<int> host_lists[2];      // stays alive while the upload is in flight
    GradPcLists gl;
    gradpc_lists(topo, gl);
    auto& hl = host_lists[bv.slot & 1];
    hl.clear();
    for (int la = 0; la <= KERNEL_LMAX; ++la)
        for (int lb = 0; lb <= la; ++lb) hl.insert(hl.end(), gl.cls[la][lb].begin(), gl.cls[la][lb].end());
    int* d_lists = (int*)list_pool[bv.slot & 1].ensure((hl.size() + 16) * sizeof(int));
    if (!d_lists) { err = "out of device memory (point-charge gradient lists)"; return false; }
    // MQC_HIP_GRAD_TIMING=1 (measurement): the span of this stage on stderr, per chunk
    static const bool timing = [] { const char* e = std::getenv("MQC_HIP_GRAD_TIMING"); return e && e[0] == '1'; }();
    hipEvent_t ev[3] = {};
    if (timing) for (auto& e : ev) { (void)hipEventCreate(&e); }
    if (timing) (void)hipEventRecord(ev[0], s);
    (void)hipMemcpyAsync(d_lists, hl.data(), hl.size() * sizeof(int), hipMemcpyHostToDevice, s);
    GradPcView gv{bv.xyz, Dtot, d_rec, bv.pc, d_grad, d_pcgrad, gl.rec_stride, bv.npc, bv.nfrag, topo.nao, topo.natoms};
    size_t off = 0;
#define GPC_D(a, b) gradpc_launch_density<a, b>(bv.topo, gv, bv.c2s, gl, d_lists, off, s);
    GPC_D(0, 0) GPC_D(1, 0) GPC_D(1, 1) GPC_D(2, 0) GPC_D(2, 1) GPC_D(2, 2) GPC_D(3, 0) GPC_D(3, 1) GPC_D(3, 2) GPC_D(3, 3)
#undef GPC_D
    if (timing) (void)hipEventRecord(ev[1], s);
    gradpc_launch_points<0>(gv, bv.boys, gl, s);
    gradpc_launch_points<1>(gv, bv.boys, gl, s);
    gradpc_launch_points<2>(gv, bv.boys, gl, s);
    gradpc_launch_points<3>(gv, bv.boys, gl, s);
    gradpc_launch_points<4>(gv, bv.boys, gl, s);
    gradpc_launch_points<5>(gv, bv.boys, gl, s);
    gradpc_launch_points<6>(gv, bv.boys, gl, s);
    if (timing) {
        (void)hipEventRecord(ev[2], s);
        (void)hipEventSynchronize(ev[2]);
        float all = 0.f, pts = 0.f;
        (void)hipEventElapsedTime(&all, ev[0], ev[2]);
        (void)hipEventElapsedTime(&pts, ev[1], ev[2]);
        std::fprintf(stderr, "mqc_hip gradient: n=%d nfrag=%d point charges %d: total %.3f ms, records %.3f ms, charges %.3f ms\n", topo.nao,
                     bv.nfrag, bv.npc, all, all - pts, pts);
        for (auto& e : ev) (void)hipEventDestroy(e);
    }
    if (hipGetLastError() != hipSuccess) { err = "point-charge gradient: a kernel launch failed"; return false; }
    return true;
}

}  // namespace mqc
