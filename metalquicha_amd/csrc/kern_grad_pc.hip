// kern_grad_pc.hip -- the point charges' part of the analytic gradient of an embedded fragment, for a whole batch.
//
// The embedding operator u = -sum_g q_g (a| 1/|r - R_g| |b) sits in the one-electron Hamiltonian, so the energy-weighted
// density of grad1e_kernel already carries it; what is left is sum_ab Dt_ab du_ab/dR.  For a shell pair (a on A, b on B)
// and a charge g there are three derivatives: v_A (the function on A moves), v_C (the charge moves) and, by translational
// invariance, v_B = -(v_A + v_C).  grad1e_kernel takes one centre at a time per wave (a wave-cooperative Boys evaluation
// per centre): fine for the nuclei, hopeless for the hundreds of charges of an FMO / EE-MBE fragment.  The two stages of
// kern_esp.hip instead:
//   hermite_density_kernel<LA, LB, true>  (hermite_records.hpp) the records
//           {p, P, atom of a, atom of b, X_tuv (order L), XA^x_tuv, XA^y_tuv, XA^z_tuv (order L + 1)},   L = LA + LB,
//       of every primitive pair, grouped by L and, inside a group, by atom pair.
//   gradpc_points_kernel<L>  lane = charge, workgroup = (tile of GRADPC_TILE charges, fragment): records staged through
//       LDS; per record one Boys evaluation F_0..F_{L+1}, the Hermite recursion in registers and six dot products,
//           v_A^c = -q sum XA^c_tuv R_tuv,      v_C^c = +q sum X_tuv R_{tuv + 1_c}      (d R_tuv(P - C) / dC_c = -R_{tuv + 1_c}).
//       A lane owns its charge's gradient (plain stores, launches of one chunk are ordered by the stream); the atoms'
//       parts are kept per lane over a run of records of one atom pair, summed over the tile once per run and added with
//       atomicAdd into the gradient grad1e_kernel and eri_grad_kernel accumulate.  Charges with q = 0 are skipped.
// L + 1 reaches 7 for f-f pairs; the same register kernel serves every L (no private segment at L = 6).
#include "hermite_records.hpp"
#include <cstdio>
#include <cstdlib>

namespace mqc {

constexpr int GRADPC_TILE = 64;                 // charges per workgroup: one wave, the run sums are wave reductions
constexpr int GRADPC_STAGE_DOUBLES = 4096;      // LDS staging buffer of the point kernel, 32 KB
constexpr int GRADPC_HEAD = hermite_head(true); // p, Px, Py, Pz, atom of a, atom of b

constexpr int gradpc_rec_doubles(int L) { return hermite_rec_doubles(L, true); }

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

size_t gradpc_record_doubles(const Topology& topo) { return hermite_record_doubles<true>(topo); }

template <int L>
static void gradpc_launch_points(const GradPcView& gv, const double* boys_table, const HermiteLists& hl, hipStream_t s)
{
    if (L > 0 && hl.nrec[L] == 0) return;
    const int tiles = (gv.npc + GRADPC_TILE - 1) / GRADPC_TILE;
    // the fragment index of the charge array is the lane-fastest one: the view keeps the chunk's base and the kernel
    // takes blockIdx.y as the fragment, so a chunk is one launch (chunks hold at most 60000 fragments, below grid.y's limit)
    hipLaunchKernelGGL((gradpc_points_kernel<L>), dim3(tiles, gv.nfrag), dim3(GRADPC_TILE), 0, s, gv, boys_table, hl.group_off[L], hl.nrec[L]);
}

// The charges' part of the gradient of one chunk, after launch_gradient: adds the atoms' part into d_grad [nfrag][natoms][3]
// and writes the sites' gradient into d_pcgrad [nfrag][npc][3].  Dtot: the total density launch_gradient used; d_rec holds
// nfrag x gradpc_record_doubles(topo).
bool launch_pc_gradient(const BatchView& bv, const Topology& topo, const double* Dtot, double* d_grad, double* d_pcgrad, double* d_rec,
                        hipStream_t s, std::string& err)
{
    if (bv.npc <= 0 || !bv.pc) { err = "point-charge gradient: the fragment carries no charges"; return false; }
    if (topo.lmax > KERNEL_LMAX) { err = "analytic gradients cover s, p, d and f shells"; return false; }
    static DevicePool list_pool[2];
    static std::vector<int> host_lists[2];      // stays alive while the upload is in flight
    const HermiteLists hl = hermite_lists<true>(topo, true);
    // MQC_HIP_GRAD_TIMING=1 (measurement): the span of this stage on stderr, per chunk
    static const bool timing = env_opt_in("MQC_HIP_GRAD_TIMING");
    hipEvent_t ev[3] = {};
    if (timing) for (auto& e : ev) { (void)hipEventCreate(&e); }
    if (timing) (void)hipEventRecord(ev[0], s);
    GradPcView gv{bv.xyz, Dtot, d_rec, bv.pc, d_grad, d_pcgrad, hl.rec_stride, bv.npc, bv.nfrag, topo.nao, topo.natoms};
    if (!launch_hermite_density<true>(bv.topo, HermiteView{bv.xyz, Dtot, d_rec, hl.rec_stride, topo.nao}, bv.nfrag, bv.c2s, hl,
                                      list_pool[bv.slot & 1], host_lists[bv.slot & 1], s, err)) {
        if (timing) for (auto& e : ev) (void)hipEventDestroy(e);
        return false;
    }
    if (timing) (void)hipEventRecord(ev[1], s);
    gradpc_launch_points<0>(gv, bv.boys, hl, s);
    gradpc_launch_points<1>(gv, bv.boys, hl, s);
    gradpc_launch_points<2>(gv, bv.boys, hl, s);
    gradpc_launch_points<3>(gv, bv.boys, hl, s);
    gradpc_launch_points<4>(gv, bv.boys, hl, s);
    gradpc_launch_points<5>(gv, bv.boys, hl, s);
    gradpc_launch_points<6>(gv, bv.boys, hl, s);
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
