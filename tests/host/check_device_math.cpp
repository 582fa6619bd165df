// check_device_math.cpp -- TEST-ONLY harness.  Compiles the `__host__ __device__` integral
// templates of metalquicha_amd/csrc/md_integrals.hpp and hermite_records.hpp for the HOST so that tests/ can compare
// the arithmetic the gfx950 kernels instantiate against the oracle here, without a GPU.
// It is never linked into libmqc_hip.so and is not a fallback path of the product.
#include "../../metalquicha_amd/csrc/md_integrals.hpp"
#include "../../metalquicha_amd/csrc/engine.hpp"
#include "../../metalquicha_amd/csrc/hermite_records.hpp"
#include <vector>
#include <set>
#include <array>
#include <algorithm>
#include <cstring>

namespace mqc {
void build_boys_table(std::vector<double>& table);
void build_c2s_tables(std::vector<double>& packed, int* offsets);
}
using namespace mqc;

static std::vector<double> g_boys, g_c2s;
static int g_off[8];

static void ensure_tables()
{
    if (g_boys.empty()) { build_boys_table(g_boys); build_c2s_tables(g_c2s, g_off); }
}

template <int LA, int LB, int LC, int LD>
static void run_class(const ShellRef* sh, double* out_sph)
{
    constexpr int NCA = ncart(LA), NCB = ncart(LB), NCC = ncart(LC), NCD = ncart(LD);
    std::vector<double> cart(NCA * NCB * NCC * NCD), tmp(NCA * NCB * NCC * NCD);
    eri_cart_block<LA, LB, LC, LD>(sh[0], sh[1], sh[2], sh[3], g_boys.data(), cart.data());
    const int L[4] = {LA, LB, LC, LD};
    int dims[4] = {NCA, NCB, NCC, NCD};
    for (int ax = 0; ax < 4; ++ax) {
        const int l = L[ax], nc = ncart(l), ns = nsph(l);
        int pre = 1, post = 1;
        for (int k = 0; k < ax; ++k) pre *= dims[k];
        for (int k = ax + 1; k < 4; ++k) post *= dims[k];
        const double* T = g_c2s.data() + g_off[l];
        for (int a = 0; a < pre; ++a)
            for (int s = 0; s < ns; ++s)
                for (int r = 0; r < post; ++r) {
                    double v = 0.0;
                    for (int c = 0; c < nc; ++c) v += T[s * nc + c] * cart[(a * nc + c) * post + r];
                    tmp[(a * ns + s) * post + r] = v;
                }
        dims[ax] = ns;
        cart.assign(tmp.begin(), tmp.begin() + pre * ns * post);
        cart.resize(NCA * NCB * NCC * NCD);
    }
    std::memcpy(out_sph, cart.data(), sizeof(double) * dims[0] * dims[1] * dims[2] * dims[3]);
}

struct HostSink {
    double* out; int nsb, nsc, nsd;
    void operator()(int i, int j, int k, int l, double v) { out[((i * nsb + j) * nsc + k) * nsd + l] = v; }
};

template <int LA, int LB, int LC, int LD>
static void run_class_passes(const ShellRef* sh, double* out_sph)
{
    constexpr int CH = eri_pass_chunk(LA, LB, LC, LD);
    std::vector<double> acc(ncart(LA) * ncart(LB) * CH);
    HostSink sink{out_sph, nsph(LB), nsph(LC), nsph(LD)};
    eri_passes_from<LA, LB, LC, LD, CH, 0>(sh[0], sh[1], sh[2], sh[3], g_boys.data(), g_c2s.data(), acc.data(), 1, sink);
}

// twin block vs the plain block of every member combination (Cartesian, before c2s): returns max |diff|
template <int LA, int LB, int LC, int LD>
static double run_twin(const ShellRef* sh, const double* const* second, const bool* is_twin)
{
    constexpr int NC = ncart(LA) * ncart(LB) * ncart(LC) * ncart(LD);
    constexpr int MA = twin_mult(true, LA), MB = twin_mult(true, LB), MC = twin_mult(true, LC), MD = twin_mult(true, LD);
    std::vector<double> acc(MA * MB * MC * MD * NC), ref(NC);
    TwinCoefs tw;
    tw.ca[0] = sh[0].coefs; tw.ca[1] = second[0]; tw.fa = is_twin[0] ? 1.0 : 0.0;
    tw.cb[0] = sh[1].coefs; tw.cb[1] = second[1]; tw.fb = is_twin[1] ? 1.0 : 0.0;
    tw.cc[0] = sh[2].coefs; tw.cc[1] = second[2]; tw.fc = is_twin[2] ? 1.0 : 0.0;
    tw.cd[0] = sh[3].coefs; tw.cd[1] = second[3]; tw.fd = is_twin[3] ? 1.0 : 0.0;
    eri_cart_block_twin<LA, LB, LC, LD>(sh[0], sh[1], sh[2], sh[3], tw, g_boys.data(), acc.data());
    double worst = 0.0;
    {
        // the partial blocks of eri_twin_wave_kernel (bra primitive pairs first, first + 3, ...) add up to the whole block
        std::vector<double> part(acc.size(), 0.0), tmp(acc.size());
        for (int first = 0; first < 3; ++first) {
            eri_cart_block_twin<LA, LB, LC, LD>(sh[0], sh[1], sh[2], sh[3], tw, g_boys.data(), tmp.data(), first, 3);
            for (size_t i = 0; i < acc.size(); ++i) part[i] += tmp[i];
        }
        double scale = 1.0;
        for (double v : acc) scale = std::max(scale, std::fabs(v));
        for (size_t i = 0; i < acc.size(); ++i) worst = std::max(worst, std::fabs(part[i] - acc[i]) / scale);
    }
    const int M[4] = {MA, MB, MC, MD};
    for (int ma = 0; ma < MA; ++ma) for (int mb = 0; mb < MB; ++mb) for (int mc = 0; mc < MC; ++mc) for (int md = 0; md < MD; ++md) {
        const int m[4] = {ma, mb, mc, md};
        ShellRef t[4];
        bool absent = false;
        for (int k = 0; k < 4; ++k) {
            t[k] = sh[k];
            if (m[k]) { if (!is_twin[k]) absent = true; else t[k].coefs = second[k]; }
        }
        (void)M;
        const double* got = acc.data() + (((ma * MB + mb) * MC + mc) * MD + md) * NC;
        if (absent) { for (int i = 0; i < NC; ++i) worst = std::max(worst, std::fabs(got[i])); continue; }
        eri_cart_block<LA, LB, LC, LD>(t[0], t[1], t[2], t[3], g_boys.data(), ref.data());
        double scale = 1.0;
        for (int i = 0; i < NC; ++i) scale = std::max(scale, std::fabs(ref[i]));
        for (int i = 0; i < NC; ++i) worst = std::max(worst, std::fabs(got[i] - ref[i]) / scale);
    }
    return worst;
}

// The records of one shell pair (hermite_records.hpp), both kinds, contracted at points as esp_points_kernel and
// gradpc_points_kernel contract them: one dot product for the potential, six for v_A and v_C.  D is the spherical
// density of the two shells alone (a first).  Returns the primitive pairs whose X blocks differ between the two kinds.
template <int LA, int LB>
static int run_hermite(const ShellRef* sh, const double* D, int npts, const double* pts, double* v, double* va, double* vc)
{
    constexpr int L = LA + LB, NH = nherm(L), NH1 = nherm(L + 1);
    constexpr int RD0 = hermite_rec_doubles(L, false), RD1 = hermite_rec_doubles(L, true), HEAD = hermite_head(true);
    double dc[ncart(LA) * ncart(LB)];
    for (int e = 0; e < ncart(LA) * ncart(LB); ++e)
        dc[e] = cart_density_element<LA, LB>(D, nsph(LA) + nsph(LB), 0, nsph(LA), true, g_c2s.data(), e);
    const int nrec = sh[0].nprim * sh[1].nprim;
    std::vector<double> r0((size_t)nrec * RD0, -1.0), r1((size_t)nrec * RD1, -1.0);
    int differ = 0;
    for (int pp = 0; pp < nrec; ++pp) {
        const int ia = pp / sh[1].nprim, ib = pp % sh[1].nprim;
        hermite_record<LA, LB, false>(dc, sh[0].exps[ia], sh[1].exps[ib], sh[0].coefs[ia], sh[1].coefs[ib], sh[0].x, sh[0].y, sh[0].z, sh[1].x,
                                      sh[1].y, sh[1].z, 0, 1, &r0[(size_t)pp * RD0]);
        hermite_record<LA, LB, true>(dc, sh[0].exps[ia], sh[1].exps[ib], sh[0].coefs[ia], sh[1].coefs[ib], sh[0].x, sh[0].y, sh[0].z, sh[1].x,
                                     sh[1].y, sh[1].z, 0, 1, &r1[(size_t)pp * RD1]);
        const double *a = &r0[(size_t)pp * RD0], *b = &r1[(size_t)pp * RD1];
        if (a[0] != b[0]) { ++differ; continue; }
        if (a[0] == 0.0) continue;
        if (std::memcmp(a, b, 4 * sizeof(double)) != 0 || std::memcmp(a + 4, b + HEAD, NH * sizeof(double)) != 0 || b[4] != 0.0 || b[5] != 1.0) ++differ;
    }
    for (int g = 0; g < npts; ++g) {
        const double cx = pts[3 * g], cy = pts[3 * g + 1], cz = pts[3 * g + 2];
        double acc = 0.0, gA[3] = {0.0, 0.0, 0.0}, gC[3] = {0.0, 0.0, 0.0};
        for (int k = 0; k < nrec; ++k) {
            {   // esp_points_kernel<L>
                const double* rec = &r0[(size_t)k * RD0];
                const double p = rec[0];
                if (p != 0.0) {
                    double R[NH];
                    hermite_r<L>(p, rec[1] - cx, rec[2] - cy, rec[3] - cz, g_boys.data(), R);
                    double s = 0.0;
                    for (int h = 0; h < NH; ++h) s += rec[4 + h] * R[h];
                    acc += s;
                }
            }
            {   // gradpc_points_kernel<L>
                const double* rec = &r1[(size_t)k * RD1];
                const double p = rec[0];
                if (p == 0.0) continue;
                double R[NH1];
                hermite_r<L + 1>(p, rec[1] - cx, rec[2] - cy, rec[3] - cz, g_boys.data(), R);
                const double* x = rec + HEAD;
                const double* xa = x + NH;
                double sa[3] = {0.0, 0.0, 0.0}, sc[3] = {0.0, 0.0, 0.0};
                for (int h = 0; h < NH1; ++h) {
                    sa[0] += xa[h] * R[h]; sa[1] += xa[NH1 + h] * R[h]; sa[2] += xa[2 * NH1 + h] * R[h];
                }
                for (int N = 0; N <= L; ++N)
                    for (int t = N; t >= 0; --t)
                        for (int u = N - t; u >= 0; --u) {
                            const int w = N - t - u;
                            const double xv = x[hidx(t, u, w)];
                            sc[0] += xv * R[hidx(t + 1, u, w)]; sc[1] += xv * R[hidx(t, u + 1, w)]; sc[2] += xv * R[hidx(t, u, w + 1)];
                        }
                for (int c = 0; c < 3; ++c) { gA[c] += sa[c]; gC[c] += sc[c]; }
            }
        }
        v[g] = acc;
        for (int c = 0; c < 3; ++c) { va[3 * g + c] = gA[c]; vc[3 * g + c] = gC[c]; }
    }
    return differ;
}

extern "C" {

// One shell pair (la >= lb) on two centres: v[g] = sum over records of X . R at point g, va[g][c] = sum XA^c . R and
// vc[g][c] = sum X . R_{+1_c} (d/dA_c of v is va, d/dC_c of v is -vc); *differ: see run_hermite.
int hostcheck_hermite_pair(const int* l, const int* nprim, const double* exps, const double* coefs, const double* xyz /* 2x3 */,
                           const double* D, int npts, const double* pts, double* v, double* va, double* vc, int* differ)
{
    ensure_tables();
    ShellRef sh[2];
    int off = 0;
    for (int k = 0; k < 2; ++k) {
        sh[k].nprim = nprim[k]; sh[k].exps = exps + off; sh[k].coefs = coefs + off;
        sh[k].x = xyz[3 * k]; sh[k].y = xyz[3 * k + 1]; sh[k].z = xyz[3 * k + 2];
        off += nprim[k];
    }
#define HCASE(a, b) case (a * 8 + b): *differ = run_hermite<a, b>(sh, D, npts, pts, v, va, vc); return 0;
    switch (l[0] * 8 + l[1]) {
        HCASE(0, 0) HCASE(1, 0) HCASE(1, 1) HCASE(2, 0) HCASE(2, 1) HCASE(2, 2) HCASE(3, 0) HCASE(3, 1) HCASE(3, 2) HCASE(3, 3)
    }
    return 1;
}

// hermite_lists of a topology.  out (cap ints): nshell, npairs, per shell (l, atom, nprim), the topology's pairs (A, B),
// then per class (la, lb), la >= lb, in launch order: its length and its (A, B, first record) triples, then nrec[0..6];
// offs: group_off[0..6], rec_stride.  Returns the ints written, -1 when the topology fails or cap is too small.
int hostcheck_hermite_lists(const mqc_hip_molecule_t* mol, const mqc_hip_basis_t* bas, int by_atom_pair, int deriv, int cap, int* out,
                            unsigned long long* offs)
{
    Topology topo;
    std::string err;
    if (build_topology(*mol, *bas, topo, err, KERNEL_LMAX, false) != MQC_HIP_OK) return -1;
    const HermiteLists hl = deriv ? hermite_lists<true>(topo, by_atom_pair != 0) : hermite_lists<false>(topo, by_atom_pair != 0);
    if (hl.rec_stride != (deriv ? hermite_record_doubles<true>(topo) : hermite_record_doubles<false>(topo))) return -1;
    std::vector<int> o{(int)topo.shells.size(), (int)topo.pairs.size() / 2};
    for (const HostShell& s : topo.shells) { o.push_back(s.l); o.push_back(s.atom); o.push_back(s.nprim); }
    o.insert(o.end(), topo.pairs.begin(), topo.pairs.end());
    for (int la = 0; la <= KERNEL_LMAX; ++la)
        for (int lb = 0; lb <= la; ++lb) {
            o.push_back((int)hl.cls[la][lb].size());
            o.insert(o.end(), hl.cls[la][lb].begin(), hl.cls[la][lb].end());
        }
    for (int L = 0; L <= HERMITE_LMAX; ++L) { o.push_back(hl.nrec[L]); offs[L] = hl.group_off[L]; }
    offs[HERMITE_LMAX + 1] = hl.rec_stride;
    if ((int)o.size() > cap) return -1;
    std::copy(o.begin(), o.end(), out);
    return (int)o.size();
}

// shells: for each of the 4 shells: nprim, then pointers are passed flat.
int hostcheck_eri_block(const int* l, const int* nprim, const double* exps, const double* coefs /* normalised, s/p factor folded */,
                        const double* xyz /* 4x3 */, double* out_sph)
{
    ensure_tables();
    ShellRef sh[4];
    int off = 0;
    for (int k = 0; k < 4; ++k) {
        sh[k].nprim = nprim[k]; sh[k].exps = exps + off; sh[k].coefs = coefs + off;
        sh[k].x = xyz[3 * k]; sh[k].y = xyz[3 * k + 1]; sh[k].z = xyz[3 * k + 2];
        off += nprim[k];
    }
    const int id = ((l[0] * 8 + l[1]) * 8 + l[2]) * 8 + l[3];
#define CASE(a, b, c, d) case (((a * 8 + b) * 8 + c) * 8 + d): run_class<a, b, c, d>(sh, out_sph); return 0;
    switch (id) {
        CASE(0, 0, 0, 0)
        CASE(1, 0, 0, 0) CASE(1, 0, 1, 0)
        CASE(1, 1, 0, 0) CASE(1, 1, 1, 0) CASE(1, 1, 1, 1)
        CASE(2, 0, 0, 0) CASE(2, 0, 1, 0) CASE(2, 0, 1, 1) CASE(2, 0, 2, 0)
        CASE(2, 1, 0, 0) CASE(2, 1, 1, 0) CASE(2, 1, 1, 1) CASE(2, 1, 2, 0) CASE(2, 1, 2, 1)
        CASE(2, 2, 0, 0) CASE(2, 2, 1, 0) CASE(2, 2, 1, 1) CASE(2, 2, 2, 0) CASE(2, 2, 2, 1) CASE(2, 2, 2, 2)
    }
    return 1;
}

int hostcheck_eri_block_passes(const int* l, const int* nprim, const double* exps, const double* coefs, const double* xyz, double* out_sph)
{
    ensure_tables();
    ShellRef sh[4];
    int off = 0;
    for (int k = 0; k < 4; ++k) {
        sh[k].nprim = nprim[k]; sh[k].exps = exps + off; sh[k].coefs = coefs + off;
        sh[k].x = xyz[3 * k]; sh[k].y = xyz[3 * k + 1]; sh[k].z = xyz[3 * k + 2];
        off += nprim[k];
    }
    const int id = ((l[0] * 8 + l[1]) * 8 + l[2]) * 8 + l[3];
#define PCASE(a, b, c, d) case (((a * 8 + b) * 8 + c) * 8 + d): run_class_passes<a, b, c, d>(sh, out_sph); return 0;
    switch (id) {
        PCASE(0, 0, 0, 0) PCASE(1, 0, 1, 0) PCASE(1, 1, 1, 1)
        PCASE(2, 0, 1, 1) PCASE(2, 0, 2, 0) PCASE(2, 1, 1, 0) PCASE(2, 1, 1, 1) PCASE(2, 1, 2, 0) PCASE(2, 1, 2, 1)
        PCASE(2, 2, 0, 0) PCASE(2, 2, 1, 0) PCASE(2, 2, 1, 1) PCASE(2, 2, 2, 0) PCASE(2, 2, 2, 1) PCASE(2, 2, 2, 2)
    }
    return 1;
}

// coefs2: second coefficient column for each shell (same layout as coefs); twin[k] != 0 marks twin positions
int hostcheck_eri_twin(const int* l, const int* nprim, const double* exps, const double* coefs, const double* coefs2,
                       const int* twin, const double* xyz, double* worst)
{
    ensure_tables();
    ShellRef sh[4];
    const double* second[4];
    bool tw[4];
    int off = 0;
    for (int k = 0; k < 4; ++k) {
        sh[k].nprim = nprim[k]; sh[k].exps = exps + off; sh[k].coefs = coefs + off; second[k] = coefs2 + off;
        sh[k].x = xyz[3 * k]; sh[k].y = xyz[3 * k + 1]; sh[k].z = xyz[3 * k + 2];
        tw[k] = twin[k] != 0 && l[k] == 0;
        off += nprim[k];
    }
    const int id = ((l[0] * 8 + l[1]) * 8 + l[2]) * 8 + l[3];
#define TCASE(a, b, c, d) case (((a * 8 + b) * 8 + c) * 8 + d): *worst = run_twin<a, b, c, d>(sh, second, tw); return 0;
    switch (id) {
        TCASE(0, 0, 0, 0) TCASE(1, 0, 0, 0) TCASE(1, 0, 1, 0) TCASE(1, 1, 0, 0)
        TCASE(1, 1, 1, 0) TCASE(2, 0, 0, 0) TCASE(2, 0, 1, 0) TCASE(2, 1, 0, 0)
    }
    return 1;
}

// Twin cut of the topology: entries expanded over their members + rest == the canonical quartet set, per class.
int hostcheck_twin_cut(const mqc_hip_molecule_t* mol, const mqc_hip_basis_t* bas, int* n_twin_first, int* n_twin_entries, int* n_bad)
{
    Topology topo;
    std::string err;
    if (build_topology(*mol, *bas, topo, err, KERNEL_LMAX, true) != MQC_HIP_OK) return 1;
    auto key = [](int a, int b, int c, int d) {
        if (a < b) std::swap(a, b);
        if (c < d) std::swap(c, d);
        if (std::make_pair(a, b) < std::make_pair(c, d)) { std::swap(a, c); std::swap(b, d); }
        return std::array<int, 4>{a, b, c, d};
    };
    *n_twin_first = 0; *n_twin_entries = 0; *n_bad = 0;
    for (int t : topo.twin_first) *n_twin_first += t;
    for (auto& cl : topo.classes) {
        std::set<std::array<int, 4>> full, cut;
        for (size_t q = 0; q + 3 < cl.quartets.size(); q += 4) full.insert(key(cl.quartets[q], cl.quartets[q + 1], cl.quartets[q + 2], cl.quartets[q + 3]));
        if (cl.twin_entries.empty()) { if (!cl.rest.empty()) ++*n_bad; continue; }
        for (size_t q = 0; q + 3 < cl.rest.size(); q += 4) {
            if (!cut.insert(key(cl.rest[q], cl.rest[q + 1], cl.rest[q + 2], cl.rest[q + 3])).second) ++*n_bad;   // duplicate
        }
        for (size_t q = 0; q + 3 < cl.twin_entries.size(); q += 4) {
            ++*n_twin_entries;
            int sh[4], m[4];
            for (int k = 0; k < 4; ++k) { sh[k] = cl.twin_entries[q + k] & 0xffff; m[k] = (cl.twin_entries[q + k] >> 16) ? 2 : 1; }
            std::set<std::array<int, 4>> mine;
            for (int a = 0; a < m[0]; ++a) for (int b = 0; b < m[1]; ++b) for (int c = 0; c < m[2]; ++c) for (int d = 0; d < m[3]; ++d)
                mine.insert(key(sh[0] + a, sh[1] + b, sh[2] + c, sh[3] + d));
            for (auto& k4 : mine) if (!cut.insert(k4).second) ++*n_bad;     // covered twice
        }
        if (cut != full) ++*n_bad;
    }
    return 0;
}

// carve_chunk for the plan of spec = {n, natoms, nshell, lmax, uhf, two_e, naux, rsh, npc, hx, ks, npts, rad_cache,
// ntot}: the bytes of a chunk of nfrag fragments (a carve with null bases), then the carve into host buffers of exactly
// those sizes.  nbad counts the arrays that fall outside their pool, are not 256-byte aligned or overlap another.
int hostcheck_carve(const int* spec, int nfrag, unsigned long long* pool_bytes, unsigned long long* frag_bytes, int* eri_tri,
                    unsigned long long* eri_stride, int* nbad)
{
    BatchPlan p;
    p.n = spec[0]; p.npair = spec[0] * (spec[0] + 1) / 2; p.natoms = spec[1];
    p.uhf = spec[4] != 0; p.two_e = spec[5]; p.naux = spec[6];
    p.rsh = spec[7] != 0; p.xc.omega = p.rsh ? 0.3 : 0.0;
    p.npc = spec[8]; p.hx = spec[9] != 0;
    p.xc.ncomp = spec[10] ? 1 : 0; p.npts = spec[11];
    plan_layout(p, spec[13], spec[2], spec[3], spec[12] != 0);
    BatchView probe{};
    const ChunkBytes need = carve_chunk(p, nfrag, nullptr, probe);
    std::vector<std::vector<char>> mem(NPOOL);
    char* bases[NPOOL];
    for (int k = 0; k < NPOOL; ++k) {
        mem[k].resize(need.pool[k] + 256);
        bases[k] = mem[k].data() + (256 - (uintptr_t)mem[k].data() % 256) % 256;
    }
    BatchView bv{};
    std::vector<CarvedArray> arrays;
    const ChunkBytes got = carve_chunk(p, nfrag, bases, bv, &arrays);
    *nbad = 0;
    for (int k = 0; k < NPOOL; ++k) if (got.pool[k] != need.pool[k]) ++*nbad;
    std::sort(arrays.begin(), arrays.end(), [](const CarvedArray& a, const CarvedArray& b) { return a.p < b.p; });
    for (size_t i = 0; i < arrays.size(); ++i) {
        const CarvedArray& a = arrays[i];
        const char* lo = (const char*)a.p;
        if ((uintptr_t)lo % 256 != 0 || lo < bases[a.pool] || lo + a.bytes > bases[a.pool] + need.pool[a.pool]) ++*nbad;
        if (i + 1 < arrays.size() && lo + a.bytes > (const char*)arrays[i + 1].p) ++*nbad;
    }
    for (int k = 0; k < NPOOL; ++k) pool_bytes[k] = need.pool[k];
    *frag_bytes = fragment_bytes(p);
    *eri_tri = bv.eri_tri;
    *eri_stride = bv.eri_stride;
    return 0;
}

// The triangular J/K layout as the engine decides it (host_setup.cpp): the block length of npair pair rows with its
// table ([(npair + 1) / 2] short-row starts, then [npair] the row of the packed triangle of every pair row; table may be
// null), whether a batch takes the triangle, and the triangular kernel's LDS bytes.
int hostcheck_jk_tri_block(int npair, int* table)
{
    std::vector<int> t;
    const int pb = jk_tri_block(npair, table ? &t : nullptr);
    if (table) std::memcpy(table, t.data(), sizeof(int) * t.size());
    return pb;
}

int hostcheck_jk_tri_layout(int n, int nfrag, int uhf) { return jk_tri_layout(n, n * (n + 1) / 2, nfrag, uhf != 0) ? 1 : 0; }

unsigned long long hostcheck_jk_tri_lds_bytes(int n) { return jk_tri_lds_bytes(n, n * (n + 1) / 2); }

// the chunk size of the batched stage entries (mqc_hip_coulomb_batch, _esp_batch, _xc_batch)
long long hostcheck_stage_chunk(unsigned long long free_bytes, unsigned long long per_fragment, long long nfrag, long long cap)
{
    return stage_chunk_fragments((size_t)free_bytes, (size_t)per_fragment, nfrag, cap);
}

// the scheduling arithmetic of the batch driver (run_batch, schedule_groups)
unsigned long long hostcheck_batch_budget(unsigned long long free_b, unsigned long long reservation, int lane, unsigned long long hbm_budget)
{
    return batch_budget_bytes((size_t)free_b, (size_t)reservation, lane, (size_t)hbm_budget);
}

long long hostcheck_batch_chunk(unsigned long long budget, unsigned long long per_frag, int ntot, int lane, int pipeline_chunks, int pipeline_min_fragments)
{
    return batch_chunk_fragments((size_t)budget, (size_t)per_frag, ntot, lane, pipeline_chunks, pipeline_min_fragments);
}

int hostcheck_defer_small_groups(const long long* nfrag, const int* nao, int ngroups, long long defer_min)
{
    std::vector<long> nf(nfrag, nfrag + ngroups);
    return defer_small_groups(nf.data(), nao, ngroups, (long)defer_min) ? 1 : 0;
}

void hostcheck_boys(int L, double T, double* F)
{
    ensure_tables();
    switch (L) {
        case 0: boys<0>(T, g_boys.data(), F); break;
        case 2: boys<2>(T, g_boys.data(), F); break;
        case 4: boys<4>(T, g_boys.data(), F); break;
        case 8: boys<8>(T, g_boys.data(), F); break;
        case 12: boys<12>(T, g_boys.data(), F); break;
        case 16: boys<16>(T, g_boys.data(), F); break;
    }
}

void hostcheck_c2s(int l, double* out)
{
    ensure_tables();
    std::memcpy(out, g_c2s.data() + g_off[l], sizeof(double) * nsph(l) * ncart(l));
}

}
