// kern_esp.hip -- electrostatic potential of a density at arbitrary points, for a whole batch.
//
//   V(r) = sum_A Z_A / |r - R_A|  -  sum_{mu nu} D_{mu nu} (mu| 1/|r' - r| |nu)
//
// The transpose of int1e_kernel's nuclear-attraction part: that kernel sums many charges into one matrix, this one
// contracts one density with the same Hermite-Coulomb integrals for many points.  Two stages:
//   hermite_density_kernel<LA, LB, false>  (hermite_records.hpp) the records {p, P, X_tuv (t + u + v <= LA + LB)} of every
//       primitive pair, so that V_elec(r) = sum_records sum_tuv X_tuv R_tuv(p, P - r); grouped by L = LA + LB, in the
//       topology's order.
//   esp_points_kernel<L>  lane = point, workgroup = (tile of ESP_TILE points, fragment): records are staged through LDS
//       in chunks; per record one Boys evaluation F_0..F_L, the Hermite recursion in registers and the dot product
//       with X_tuv (LDS broadcast reads).  The L = 0 launch initialises the output (nuclear term or zero), the others
//       accumulate; launches of one fragment chunk are ordered by the stream.
#include "hermite_records.hpp"

namespace mqc {

constexpr int ESP_TILE = 256;                   // points per workgroup (4 waves share the staged records)
constexpr int ESP_STAGE_DOUBLES = 2048;         // LDS staging buffer of the point kernel, 16 KB

constexpr int esp_rec_doubles(int L) { return hermite_rec_doubles(L, false); }

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

size_t esp_record_doubles(const Topology& topo) { return hermite_record_doubles<false>(topo); }

template <int L>
static void esp_launch_points(const TopologyDev& td, const EspView& ev, const double* boys_table, const HermiteLists& hl, int include_nuclei,
                              hipStream_t s)
{
    if (L > 0 && hl.nrec[L] == 0) return;
    const int tiles = (ev.max_points + ESP_TILE - 1) / ESP_TILE;
    hipLaunchKernelGGL((esp_points_kernel<L>), dim3(tiles, ev.nfrag), dim3(ESP_TILE), 0, s, ev, boys_table, td.zeff, td.natoms, hl.group_off[L],
                       hl.nrec[L], L == 0 ? 1 : 0, include_nuclei);
}

// One chunk of fragments (at most 65535, the launch grid's limit): d_* are device arrays of the chunk (see EspView);
// d_rec holds nfrag x esp_record_doubles(topo)
bool launch_esp(const TopologyDev& td, const Topology& topo, const double* boys_table, const double* c2s, int nfrag, const double* d_xyz,
                const double* d_D, double* d_rec, const double* d_pts, const int* d_npts, int max_points, int include_nuclei, double* d_out,
                hipStream_t s, std::string& err)
{
    static DevicePool list_pool;
    static std::vector<int> host_lists;      // stays alive while the upload is in flight
    const HermiteLists hl = hermite_lists<false>(topo, false);
    EspView ev{d_xyz, d_D, d_rec, d_pts, d_npts, d_out, hl.rec_stride, max_points, nfrag, topo.nao};
    if (!launch_hermite_density<false>(td, HermiteView{d_xyz, d_D, d_rec, hl.rec_stride, topo.nao}, nfrag, c2s, hl, list_pool, host_lists, s, err))
        return false;
    esp_launch_points<0>(td, ev, boys_table, hl, include_nuclei, s);
    esp_launch_points<1>(td, ev, boys_table, hl, include_nuclei, s);
    esp_launch_points<2>(td, ev, boys_table, hl, include_nuclei, s);
    esp_launch_points<3>(td, ev, boys_table, hl, include_nuclei, s);
    esp_launch_points<4>(td, ev, boys_table, hl, include_nuclei, s);
    esp_launch_points<5>(td, ev, boys_table, hl, include_nuclei, s);
    esp_launch_points<6>(td, ev, boys_table, hl, include_nuclei, s);
    if (hipGetLastError() != hipSuccess) { err = "esp: a kernel launch failed"; return false; }
    return true;
}

}  // namespace mqc
