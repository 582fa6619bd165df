// kern_esp.hip -- electrostatic potential of a density at arbitrary points, for a whole batch.
//
//   V(r) = sum_A Z_A / |r - R_A|  -  sum_{mu nu} D_{mu nu} (mu| 1/|r' - r| |nu)
//
// The transpose of int1e_kernel's nuclear-attraction part: that kernel sums many charges into one matrix, this one
// contracts one density with the same Hermite-Coulomb integrals for many points.  Two stages:
//   esp_hermite_density_kernel<LA, LB>  one wave per (shell pair a >= b, fragment): the density block goes to Cartesian
//       components (LDS), every lane takes primitive pairs and contracts the block with the E coefficients into a
//       record {p, P, X_tuv (t + u + v <= LA + LB)} with the prefactor (2 pi / p) K_ab c_a c_b folded in, so that
//       V_elec(r) = sum_records sum_tuv X_tuv R_tuv(p, P - r).  Records are grouped by L = LA + LB.
//   esp_points_kernel<L>  lane = point, workgroup = (tile of ESP_TILE points, fragment): records are staged through LDS
//       in chunks; per record one Boys evaluation F_0..F_L, the Hermite recursion in registers and the dot product
//       with X_tuv (LDS broadcast reads).  The L = 0 launch initialises the output (nuclear term or zero), the others
//       accumulate; launches of one fragment chunk are ordered by the stream.
#include "engine.hpp"
#include "md_integrals.hpp"
#include <algorithm>
#include <vector>

namespace mqc {

constexpr int ESP_LMAX = 2 * KERNEL_LMAX;       // f shells on both sides: 84 Hermite terms
constexpr int ESP_TILE = 256;                   // points per workgroup (4 waves share the staged records)
constexpr int ESP_STAGE_DOUBLES = 2048;         // LDS staging buffer of the point kernel, 16 KB

__host__ __device__ constexpr int esp_rec_doubles(int L) { return 4 + nherm(L); }

struct EspView {
    const double* xyz;       // [nfrag][natoms][3]
    const double* D;         // [nfrag][n*n]
    double* rec;             // [nfrag][rec_stride]: per L group, records of esp_rec_doubles(L)
    const double* pts;       // [nfrag][max_points][3]
    const int* npts;         // [nfrag]
    double* out;             // [nfrag][max_points]
    size_t rec_stride;
    int max_points, nfrag, n;
};

template <int LA, int LB>
__global__ void __launch_bounds__(64) esp_hermite_density_kernel(TopologyDev tp, EspView ev, const double* __restrict__ c2s,
                                                                  const int* __restrict__ pairs /* A, B, first record */, size_t group_off)
{
    constexpr int NCA = ncart(LA), NCB = ncart(LB), NSA = nsph(LA), NSB = nsph(LB);
    constexpr int L = LA + LB, NH = nherm(L), RD = esp_rec_doubles(L);
    __shared__ double dc[NCA * NCB];
    const int f = blockIdx.y, ip = blockIdx.x, lane = threadIdx.x;
    const int A = pairs[3 * ip], B = pairs[3 * ip + 1], rec0 = pairs[3 * ip + 2];
    const int n = ev.n;
    const double* D = ev.D + (size_t)f * n * n;
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
    const double* xyz = ev.xyz + (size_t)f * tp.natoms * 3;
    const int atA = tp.sh_atom[A], atB = tp.sh_atom[B];
    const double ax = xyz[3 * atA], ay = xyz[3 * atA + 1], az = xyz[3 * atA + 2];
    const double bx = xyz[3 * atB], by = xyz[3 * atB + 1], bz = xyz[3 * atB + 2];
    const double ab2 = (ax - bx) * (ax - bx) + (ay - by) * (ay - by) + (az - bz) * (az - bz);
    const int npa = tp.sh_nprim[A], npb = tp.sh_nprim[B];
    const double* ea = tp.exps + tp.sh_poff[A]; const double* ca = tp.coefs + tp.sh_poff[A];
    const double* eb = tp.exps + tp.sh_poff[B]; const double* cb = tp.coefs + tp.sh_poff[B];
    double* recs = ev.rec + (size_t)f * ev.rec_stride + group_off + (size_t)rec0 * RD;
    for (int pp = lane; pp < npa * npb; pp += 64) {
        const int ipa = pp / npb, jp = pp % npb;
        const double a = ea[ipa], b = eb[jp], p = a + b, ip_ = 1.0 / p;
        double* r = recs + (size_t)pp * RD;
        const double ex_arg = a * b * ip_ * ab2;
        if (ex_arg > PRIM_EXP_CUTOFF) { r[0] = 0.0; continue; }       // p = 0 marks a record the point kernel skips
        const double pref = 2.0 * M_PI * ip_ * exp(-ex_arg) * ca[ipa] * cb[jp];
        const double px = (a * ax + b * bx) * ip_, py = (a * ay + b * by) * ip_, pz = (a * az + b * bz) * ip_;
        E1D<LA, LB> ex, ey, ez;
        ex.build(px - ax, px - bx, 0.5 * ip_);
        ey.build(py - ay, py - by, 0.5 * ip_);
        ez.build(pz - az, pz - bz, 0.5 * ip_);
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
                        for (int t = 0; t <= i0 + j0; ++t) {
                            const double dx = d * ex.get(i0, j0, t);
#pragma unroll
                            for (int u = 0; u <= i1 + j1; ++u) {
                                const double dxy = dx * ey.get(i1, j1, u);
#pragma unroll
                                for (int w = 0; w <= i2 + j2; ++w) X[hidx(t, u, w)] += dxy * ez.get(i2, j2, w);
                            }
                        }
                        ++k;
                    }
            }
        r[0] = p; r[1] = px; r[2] = py; r[3] = pz;
#pragma unroll
        for (int h = 0; h < NH; ++h) r[4 + h] = pref * X[h];
    }
}

template <int L>
__global__ void __launch_bounds__(ESP_TILE) esp_points_kernel(EspView ev, const double* __restrict__ boys_table, const double* __restrict__ zeff,
                                                              int natoms, size_t group_off, int nrec, int init, int include_nuclei)
{
    constexpr int NH = nherm(L), RD = esp_rec_doubles(L);
    constexpr int CHUNK = ESP_STAGE_DOUBLES / RD;      // records per staged chunk
    __shared__ double stage[CHUNK * RD];
    const int f = blockIdx.y;
    const int np = ev.npts[f];
    if ((int)(blockIdx.x * ESP_TILE) >= np) return;    // whole tile beyond this fragment's count (uniform)
    const int ipt = blockIdx.x * ESP_TILE + threadIdx.x;
    const bool live = ipt < np;
    double rx = 0.0, ry = 0.0, rz = 0.0;
    if (live) {
        const double* r = ev.pts + ((size_t)f * ev.max_points + ipt) * 3;
        rx = r[0]; ry = r[1]; rz = r[2];
    }
    const double* recs = ev.rec + (size_t)f * ev.rec_stride + group_off;
    double acc = 0.0;
    for (int r0 = 0; r0 < nrec; r0 += CHUNK) {
        const int nr = min(CHUNK, nrec - r0);
        __syncthreads();
        for (int e = threadIdx.x; e < nr * RD; e += ESP_TILE) stage[e] = recs[(size_t)r0 * RD + e];
        __syncthreads();
        for (int k = 0; k < nr; ++k) {
            const double* rec = stage + k * RD;
            const double p = rec[0];
            if (p == 0.0) continue;
            const double X = rec[1] - rx, Y = rec[2] - ry, Z = rec[3] - rz;
            double R[NH];
            hermite_r<L>(p, X, Y, Z, boys_table, R);
            double v = 0.0;
#pragma unroll
            for (int h = 0; h < NH; ++h) v += rec[4 + h] * R[h];
            acc += v;
        }
    }
    if (!live) return;
    double* out = ev.out + (size_t)f * ev.max_points + ipt;
    if (init) {
        double vn = 0.0;
        if (include_nuclei) {
            const double* xyz = ev.xyz + (size_t)f * natoms * 3;
            for (int a = 0; a < natoms; ++a) {
                const double z = zeff[a];
                if (z == 0.0) continue;
                const double dx = rx - xyz[3 * a], dy = ry - xyz[3 * a + 1], dz = rz - xyz[3 * a + 2];
                vn += z / sqrt(dx * dx + dy * dy + dz * dz);
            }
        }
        *out = vn - acc;
    } else {
        *out -= acc;
    }
}

// record counts per L group and the (A, B, first record) triples per (la, lb) class
struct EspLists {
    std::vector<int> cls[KERNEL_LMAX + 1][KERNEL_LMAX + 1];
    int nrec[ESP_LMAX + 1] = {};
    size_t group_off[ESP_LMAX + 1] = {};
    size_t rec_stride = 0;
};

static void esp_lists(const Topology& topo, EspLists& el)
{
    for (size_t k = 0; k + 1 < topo.pairs.size(); k += 2) {
        int A = topo.pairs[k], B = topo.pairs[k + 1];
        int la = topo.shells[A].l, lb = topo.shells[B].l;
        if (la < lb) { std::swap(A, B); std::swap(la, lb); }
        auto& c = el.cls[la][lb];
        c.push_back(A); c.push_back(B); c.push_back(el.nrec[la + lb]);
        el.nrec[la + lb] += topo.shells[A].nprim * topo.shells[B].nprim;
    }
    size_t off = 0;
    for (int L = 0; L <= ESP_LMAX; ++L) { el.group_off[L] = off; off += (size_t)el.nrec[L] * esp_rec_doubles(L); }
    el.rec_stride = (off + 31) & ~size_t(31);
}

size_t esp_record_doubles(const Topology& topo)
{
    EspLists el;
    esp_lists(topo, el);
    return el.rec_stride;
}

template <int LA, int LB>
static void esp_launch_density(const TopologyDev& td, const EspView& ev, const double* c2s, const EspLists& el, const int* d_lists,
                               size_t& list_off, hipStream_t s)
{
    const auto& c = el.cls[LA][LB];
    if (c.empty()) return;
    const int npairs = (int)c.size() / 3;
    for (int y0 = 0; y0 < ev.nfrag; y0 += 65535) {     // grid.y limit
        EspView v = ev;
        const int ny = std::min(65535, ev.nfrag - y0);
        v.xyz += (size_t)y0 * td.natoms * 3; v.D += (size_t)y0 * ev.n * ev.n; v.rec += (size_t)y0 * ev.rec_stride;
        hipLaunchKernelGGL((esp_hermite_density_kernel<LA, LB>), dim3(npairs, ny), dim3(64), 0, s, td, v, c2s, d_lists + list_off, el.group_off[LA + LB]);
    }
    list_off += c.size();
}

template <int L>
static void esp_launch_points(const TopologyDev& td, const EspView& ev, const double* boys_table, const EspLists& el, int include_nuclei,
                              hipStream_t s)
{
    if (L > 0 && el.nrec[L] == 0) return;
    const int tiles = (ev.max_points + ESP_TILE - 1) / ESP_TILE;
    for (int y0 = 0; y0 < ev.nfrag; y0 += 65535) {
        EspView v = ev;
        const int ny = std::min(65535, ev.nfrag - y0);
        v.xyz += (size_t)y0 * td.natoms * 3; v.rec += (size_t)y0 * ev.rec_stride; v.pts += (size_t)y0 * ev.max_points * 3;
        v.npts += y0; v.out += (size_t)y0 * ev.max_points;
        hipLaunchKernelGGL((esp_points_kernel<L>), dim3(tiles, ny), dim3(ESP_TILE), 0, s, v, boys_table, td.zeff, td.natoms, el.group_off[L],
                           el.nrec[L], L == 0 ? 1 : 0, include_nuclei);
    }
}

// One chunk of fragments: d_* are device arrays of the chunk (see EspView); d_rec holds nfrag x esp_record_doubles(topo)
void launch_esp(const TopologyDev& td, const Topology& topo, const double* boys_table, const double* c2s, int nfrag, const double* d_xyz,
                const double* d_D, double* d_rec, const double* d_pts, const int* d_npts, int max_points, int include_nuclei, double* d_out,
                hipStream_t s)
{
    static DevicePool list_pool;
    static std::vector<int> host_lists;      // stays alive while the upload is in flight
    EspLists el;
    esp_lists(topo, el);
    host_lists.clear();
    for (int la = 0; la <= KERNEL_LMAX; ++la)
        for (int lb = 0; lb <= la; ++lb) host_lists.insert(host_lists.end(), el.cls[la][lb].begin(), el.cls[la][lb].end());
    int* d_lists = (int*)list_pool.ensure((host_lists.size() + 16) * sizeof(int));
    if (!d_lists) return;
    (void)hipMemcpyAsync(d_lists, host_lists.data(), host_lists.size() * sizeof(int), hipMemcpyHostToDevice, s);
    EspView ev{d_xyz, d_D, d_rec, d_pts, d_npts, d_out, el.rec_stride, max_points, nfrag, topo.nao};
    size_t off = 0;
#define ESP_D(a, b) esp_launch_density<a, b>(td, ev, c2s, el, d_lists, off, s);
    ESP_D(0, 0) ESP_D(1, 0) ESP_D(1, 1) ESP_D(2, 0) ESP_D(2, 1) ESP_D(2, 2) ESP_D(3, 0) ESP_D(3, 1) ESP_D(3, 2) ESP_D(3, 3)
#undef ESP_D
    esp_launch_points<0>(td, ev, boys_table, el, include_nuclei, s);
    esp_launch_points<1>(td, ev, boys_table, el, include_nuclei, s);
    esp_launch_points<2>(td, ev, boys_table, el, include_nuclei, s);
    esp_launch_points<3>(td, ev, boys_table, el, include_nuclei, s);
    esp_launch_points<4>(td, ev, boys_table, el, include_nuclei, s);
    esp_launch_points<5>(td, ev, boys_table, el, include_nuclei, s);
    esp_launch_points<6>(td, ev, boys_table, el, include_nuclei, s);
}

}  // namespace mqc
