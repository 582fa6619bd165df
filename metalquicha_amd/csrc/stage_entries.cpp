// stage_entries.cpp -- the stage-level extern "C" entry points of libmqc_hip.so: one stage of the engine on the caller's
// inputs (one-electron integrals, the ERI tensor, J/K, Coulomb and potential batches, the XC quadrature, the terms of
// the analytic gradient, the eigen-solver, the DIIS coefficients).  They run on lane 0 with the driver's own pieces (driver.hpp).
#include "driver.hpp"
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

namespace mqc {
// kern_esp.hip: potential of nfrag densities at their points (device arrays of one chunk); doubles of records per fragment
bool launch_esp(const TopologyDev& td, const Topology& topo, const double* boys_table, const double* c2s, int nfrag, const double* d_xyz,
                const double* d_D, double* d_rec, const double* d_pts, const int* d_npts, int max_points, int include_nuclei, double* d_out,
                hipStream_t s, std::string& err);
size_t esp_record_doubles(const Topology& topo);
static DevicePool g_esp_pool;
// kern_grad.hip: the steps of launch_gradient
void grad_prepare_kernels();
double* launch_grad_densities(const BatchView& bv, double* work, hipStream_t s);
void launch_grad1e_pairs(const BatchView& bv, int la, int lb, const int* d_pairs, int npairs, const double* Dtot, const double* Wm,
                         double* d_grad, hipStream_t s);
bool launch_eri_grad_rows(const BatchView& bv, int la, int lb, int lc, int ld, const int* d_list, int nq, const double* Dtot,
                          const double* Dbeta, double* d_grad, int mode, const double* gam, hipStream_t s, std::string& err);
void df_gradient_lists(const Topology& topo, const Topology& aux, std::vector<int> (&t3)[4][4][4], std::vector<int> (&t2)[4][4]);
void grad_one_electron(const BatchView& bv, const Topology& topo, const double* Dtot, const double* Wm, double* d_grad, int* d_lists,
                       size_t& off, hipStream_t s);
bool grad_two_electron(const BatchView& bv, const Topology& topo, const Topology* aux, const double* Dtot, double* d_grad, int* d_lists,
                       size_t& off, const double* schwarz, double screen_tol, hipStream_t s, std::string& err);
size_t grad_list_ints(const BatchView& bv, const Topology& topo);

// every fragment has the elements (and ghosts) of the first, and its arrays: one topology per batched call
static bool same_elements(const mqc_hip_molecule_t* mols, int64_t nfrag)
{
    for (int64_t i = 0; i < nfrag; ++i)
        if (!mols[i].atomic_numbers || !mols[i].xyz || mols[i].n_atoms != mols[0].n_atoms ||
            std::memcmp(mols[i].atomic_numbers, mols[0].atomic_numbers, sizeof(int32_t) * mols[0].n_atoms) != 0 || mols[i].ghost != mols[0].ghost)
            return false;
    return true;
}

// the geometries of a chunk of nf fragments in one host vector [nf][natoms][3]
static void gather_xyz(const mqc_hip_molecule_t* mols, int nf, int natoms, std::vector<double>& hx)
{
    hx.resize((size_t)nf * natoms * 3);
    for (int f = 0; f < nf; ++f) std::memcpy(&hx[(size_t)f * natoms * 3], mols[f].xyz, sizeof(double) * natoms * 3);
}

// wait for the stream, then the error a kernel of it may have left
static int sync_and_check(hipStream_t s)
{
    HIP_CHECK_RET(hipStreamSynchronize(s));
    HIP_CHECK_RET(hipGetLastError());
    return MQC_HIP_OK;
}
}  // namespace mqc

using namespace mqc;

extern "C" {

// ---- stage-level entry points -----------------------------------------------------------
struct StageBatch {
    Topology topo;
    TopologyDev td;
    BatchView bv{};
};

// the plan of a stage-level call: closed shell, no exchange-correlation, the tensor layout of a batch of ntot
static BatchPlan stage_plan(const Topology& topo, int two_e, int ntot)
{
    BatchPlan p;
    p.n = topo.nao; p.npair = topo.npair; p.natoms = topo.natoms;
    p.two_e = two_e;
    plan_layout(p, ntot, (int)topo.shells.size(), topo.lmax, false);
    return p;
}

static int stage_setup(mqc_hip_context* ctx, const mqc_hip_molecule_t* mol, const mqc_hip_basis_t* bas, bool with_eri, StageBatch& sb,
                       int two_e = -1)
{
    if (!ctx || !mol || !bas) return fail(MQC_HIP_ERR_VALIDATION, "null argument");
    HIP_CHECK_RET(hipSetDevice(ctx->device));
    std::string err;
    int rc = build_topology(*mol, *bas, sb.topo, err);
    if (rc != MQC_HIP_OK) return fail(rc, err);
    if (with_eri && !incore_supported(sb.topo.nao)) return fail(MQC_HIP_ERR_UNSUPPORTED, "fragment too large for the in-core ERI path");
    rc = upload_topology(ctx, sb.topo, sb.td);
    if (rc != MQC_HIP_OK) return rc;
    if (two_e < 0) two_e = with_eri ? TWO_E_INCORE : TWO_E_NONE;
    rc = carve_slot(ctx, make_slot(ctx, 0, nullptr), stage_plan(sb.topo, two_e, 1), sb.td, 1, sb.bv);
    if (rc != MQC_HIP_OK) return rc;
    sb.bv.nocc = std::max(1, sb.topo.nelec / 2); sb.bv.exx = 1.0;
    HIP_CHECK_RET(hipMemcpy(sb.bv.xyz, mol->xyz, sizeof(double) * 3 * mol->n_atoms, hipMemcpyHostToDevice));
    HIP_CHECK_RET(hipMemset(sb.bv.istate, 0, sizeof(int) * 4));
    return MQC_HIP_OK;
}

int mqc_hip_int1e(mqc_hip_context* ctx, const mqc_hip_molecule_t* mol, const mqc_hip_basis_t* bas, double* S, double* T, double* V)
{
    StageBatch sb;
    int rc = stage_setup(ctx, mol, bas, false, sb);
    if (rc != MQC_HIP_OK) return rc;
    launch_int1e(sb.bv, sb.topo, ctx->lane[0].stream);
    if ((rc = sync_and_check(ctx->lane[0].stream)) != MQC_HIP_OK) return rc;
    const size_t nn = (size_t)sb.topo.nao * sb.topo.nao;
    if (S) HIP_CHECK_RET(hipMemcpy(S, sb.bv.S, sizeof(double) * nn, hipMemcpyDeviceToHost));
    if (T) HIP_CHECK_RET(hipMemcpy(T, sb.bv.W, sizeof(double) * nn, hipMemcpyDeviceToHost));
    if (V) HIP_CHECK_RET(hipMemcpy(V, sb.bv.W + nn, sizeof(double) * nn, hipMemcpyDeviceToHost));
    return MQC_HIP_OK;
}

// the packed tensor of one fragment: 1/r12 (omega = 0) or erf(omega r12)/r12
static int stage_eri_packed(mqc_hip_context* ctx, const mqc_hip_molecule_t* mol, const mqc_hip_basis_t* bas, double omega,
                            double schwarz_tol, double* M)
{
    StageBatch sb;
    int rc = stage_setup(ctx, mol, bas, true, sb);
    if (rc != MQC_HIP_OK) return rc;
    // stage-level check of the tensor: poison it first, so that an element no class list covers shows up as NaN
    HIP_CHECK_RET(hipMemsetAsync(sb.bv.eri, 0xFF, sizeof(double) * (size_t)sb.topo.npair * sb.topo.npair, ctx->lane[0].stream));
    launch_eri(sb.bv, sb.topo, schwarz_tol, ctx->lane[0].stream, nullptr, omega);
    if ((rc = sync_and_check(ctx->lane[0].stream)) != MQC_HIP_OK) return rc;
    const size_t np = (size_t)sb.topo.npair;
    HIP_CHECK_RET(hipMemcpy(M, sb.bv.eri, sizeof(double) * np * np, hipMemcpyDeviceToHost));
    return MQC_HIP_OK;
}

int mqc_hip_eri_packed(mqc_hip_context* ctx, const mqc_hip_molecule_t* mol, const mqc_hip_basis_t* bas, double schwarz_tol, double* M)
{
    return stage_eri_packed(ctx, mol, bas, 0.0, schwarz_tol, M);
}

int mqc_hip_eri_packed_attenuated(mqc_hip_context* ctx, const mqc_hip_molecule_t* mol, const mqc_hip_basis_t* bas, double omega,
                                  double schwarz_tol, double* M)
{
    if (!(omega > 0.0) || !std::isfinite(omega)) return fail(MQC_HIP_ERR_VALIDATION, "attenuated ERIs: omega must be positive and finite");
    return stage_eri_packed(ctx, mol, bas, omega, schwarz_tol, M);
}

// The PCM stage of one fragment for a given density: the SCF entry's setup and iteration kernels (kern_pcm.hip) on the
// arrays of a one-fragment chunk, everything in between copied out
int mqc_hip_pcm_stage(mqc_hip_context* ctx, const mqc_hip_molecule_t* mol, const mqc_hip_basis_t* bas, const mqc_hip_pcm_options_t* pcm,
                      const double* D, int32_t tessera_capacity, int64_t a_capacity, int32_t* n_tesserae, double* tesserae, double* areas,
                      double* A, double* v, double* q, double* e_pcm, double* V_pcm)
{
    if (!ctx || !mol || !bas || !pcm || !D || !n_tesserae) return fail(MQC_HIP_ERR_VALIDATION, "null argument");
    if (!mol->atomic_numbers || !mol->xyz || mol->n_atoms <= 0) return fail(MQC_HIP_ERR_VALIDATION, "fragment has no geometry");
    *n_tesserae = 0;
    std::string why;
    int rc = pcm_check_options(pcm, why);
    if (rc != MQC_HIP_OK) return fail(rc, why);
    pcm::Cavity cav;
    rc = pcm_build_cavity(*mol, *pcm, cav, why);
    *n_tesserae = cav.count;
    if (rc != MQC_HIP_OK) return fail(rc, why);
    HIP_CHECK_RET(hipSetDevice(ctx->device));
    StageBatch sb;
    if ((rc = build_topology(*mol, *bas, sb.topo, why)) != MQC_HIP_OK) return fail(rc, why);
    if (sb.topo.nao > 256) return fail(MQC_HIP_ERR_UNSUPPORTED, "fragment too large (n_ao <= 256)");
    const int T = cav.count, n = sb.topo.nao;
    const size_t np = (size_t)sb.topo.npair, nn = (size_t)n * n;
    if ((tesserae || areas || v || q) && tessera_capacity < T)
        return fail(MQC_HIP_ERR_VALIDATION, "PCM stage: tessera_capacity " + std::to_string(tessera_capacity) + " is below the " + std::to_string(T) + " tesserae of the cavity");
    if (A && a_capacity < (int64_t)((size_t)T * np))
        return fail(MQC_HIP_ERR_VALIDATION, "PCM stage: a_capacity is below n_tesserae x npair = " + std::to_string((size_t)T * np));
    if ((rc = upload_topology(ctx, sb.topo, sb.td)) != MQC_HIP_OK) return rc;
    BatchPlan plan = stage_plan(sb.topo, TWO_E_NONE, 1);
    plan.pcm_stride = pcm::chunk_stride(T);
    plan.pcm_f = (pcm->epsilon - 1.0) / pcm->epsilon;
    PcmView pv;
    if ((rc = carve_slot(ctx, make_slot(ctx, 0, nullptr), plan, sb.td, 1, sb.bv, &pv)) != MQC_HIP_OK) return rc;
    hipStream_t s = ctx->lane[0].stream;
    const size_t ts = (size_t)pv.stride;
    std::vector<double> hp(ts * 4, 0.0);
    std::memcpy(hp.data(), cav.xyza.data(), sizeof(double) * 4 * (size_t)T);
    HIP_CHECK_RET(hipMemcpyAsync(sb.bv.xyz, mol->xyz, sizeof(double) * 3 * mol->n_atoms, hipMemcpyHostToDevice, s));
    HIP_CHECK_RET(hipMemsetAsync(sb.bv.istate, 0, sizeof(int) * 4, s));
    HIP_CHECK_RET(hipMemcpyAsync(sb.bv.D, D, sizeof(double) * nn, hipMemcpyHostToDevice, s));
    HIP_CHECK_RET(hipMemcpyAsync(pv.pts, hp.data(), sizeof(double) * hp.size(), hipMemcpyHostToDevice, s));
    HIP_CHECK_RET(hipMemcpyAsync(pv.nt, &T, sizeof(int), hipMemcpyHostToDevice, s));
    // poison what the kernels must fill: an element they leave out reads as NaN
    HIP_CHECK_RET(hipMemsetAsync(pv.A, 0xFF, sizeof(double) * ts * np, s));
    HIP_CHECK_RET(hipMemsetAsync(pv.B, 0xFF, sizeof(double) * ts * np, s));
    HIP_CHECK_RET(hipMemsetAsync(pv.Linv, 0xFF, sizeof(double) * ts * ts, s));      // the factorisation leaves its upper triangle alone
    HIP_CHECK_RET(hipMemsetAsync(sb.bv.Vxc, 0xFF, sizeof(double) * nn, s));
    launch_pcm_setup(sb.bv, pv, sb.topo, s);
    launch_pcm_iteration(sb.bv, pv, false, s);
    launch_pcm_charges(sb.bv, pv, s);
    if ((rc = sync_and_check(s)) != MQC_HIP_OK) return rc;
    double sc[8];
    HIP_CHECK_RET(hipMemcpy(sc, pv.scal, sizeof(sc), hipMemcpyDeviceToHost));
    if (sc[7] != 0.0) return fail(MQC_HIP_ERR_GENERIC, "PCM: the cavity matrix S of this fragment could not be factorised (a pivot failed)");
    for (int t = 0; t < T; ++t) {
        if (tesserae) { tesserae[3 * t] = cav.xyza[4 * (size_t)t]; tesserae[3 * t + 1] = cav.xyza[4 * (size_t)t + 1]; tesserae[3 * t + 2] = cav.xyza[4 * (size_t)t + 2]; }
        if (areas) areas[t] = cav.xyza[4 * (size_t)t + 3];
    }
    if (A) HIP_CHECK_RET(hipMemcpy(A, pv.A, sizeof(double) * (size_t)T * np, hipMemcpyDeviceToHost));
    if (v) HIP_CHECK_RET(hipMemcpy(v, pv.v, sizeof(double) * (size_t)T, hipMemcpyDeviceToHost));
    if (q) HIP_CHECK_RET(hipMemcpy(q, pv.b, sizeof(double) * (size_t)T, hipMemcpyDeviceToHost));
    if (e_pcm) *e_pcm = sc[0];
    if (V_pcm) {
        std::vector<double> acc(nn);
        HIP_CHECK_RET(hipMemcpy(acc.data(), sb.bv.Vxc, sizeof(double) * nn, hipMemcpyDeviceToHost));
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < n; ++j) V_pcm[(size_t)i * n + j] = acc[(size_t)i * n + j] + acc[(size_t)j * n + i];
    }
    return MQC_HIP_OK;
}

// The gradient stage of one fragment on the caller's densities (include/mqc_hip.h): the steps of launch_gradient
// (kern_grad.hip) one at a time, every term into a buffer of its own
int mqc_hip_gradient_stage(mqc_hip_context* ctx, const mqc_hip_molecule_t* mol, const mqc_hip_basis_t* bas, const mqc_hip_basis_t* auxbas,
                           const mqc_hip_gradient_stage_t* a)
{
    if (!mol || !bas || !a) return fail(MQC_HIP_ERR_VALIDATION, "gradient stage: null argument");
    if (!mol->atomic_numbers || !mol->xyz || mol->n_atoms <= 0) return fail(MQC_HIP_ERR_VALIDATION, "gradient stage: fragment has no geometry");
    const bool want_rows = a->row_count > 0;
    const bool device_rows = want_rows && a->g_rows;
    const bool whole = a->w || a->g1e || a->g1e_pair || a->g2e;
    const bool uhf = a->D_beta != nullptr;
    const int mode = a->mode;
    // the rows alone are host work: only then may the context be missing
    if (!ctx && (whole || device_rows)) return fail(MQC_HIP_ERR_VALIDATION, "gradient stage: null argument (context)");
    if (mode < 0 || mode > 2) return fail(MQC_HIP_ERR_VALIDATION, "gradient stage: mode must be 0 (exact), 1 (three-centre) or 2 (two-centre)");
    if (want_rows && (!a->rows || !a->class_length)) return fail(MQC_HIP_ERR_VALIDATION, "gradient stage: null argument (rows, class_length)");
    if (want_rows && mode != 0 && !auxbas) return fail(MQC_HIP_ERR_VALIDATION, "gradient stage: null argument (the auxiliary basis of a density-fitted row)");
    if (device_rows && mode != 0 && !a->gam) return fail(MQC_HIP_ERR_VALIDATION, "gradient stage: null argument (gam)");
    const bool need_d = whole || (device_rows && mode == 0);
    if (need_d && !a->D) return fail(MQC_HIP_ERR_VALIDATION, "gradient stage: null argument (D)");
    const bool need_w = a->w || a->g1e || a->g1e_pair;
    if (need_w && (!a->C || !a->eps || (uhf && (!a->C_beta || !a->eps_beta))))
        return fail(MQC_HIP_ERR_VALIDATION, "gradient stage: null argument (C, eps)");
    if (want_rows)
        for (int k = 0; k < 4; ++k)
            if (a->row_class[k] < 0 || a->row_class[k] > KERNEL_LMAX)
                return fail(MQC_HIP_ERR_VALIDATION, "gradient stage: class with l = " + std::to_string(a->row_class[k]) + " (l > 3 is not covered: s, p, d and f shells)");
    std::string why;
    StageBatch sb;
    Topology xtopo;
    int rc = build_topology(*mol, *bas, sb.topo, why);
    if (rc != MQC_HIP_OK) return fail(rc, "gradient stage: " + why);
    const Topology& topo = sb.topo;
    if (topo.lmax > KERNEL_LMAX) return fail(MQC_HIP_ERR_VALIDATION, "gradient stage: a shell with l > 3 (s, p, d and f shells are covered)");
    if (topo.nao > 256) return fail(MQC_HIP_ERR_UNSUPPORTED, "fragment too large (n_ao <= 256)");
    if (want_rows && mode != 0) {
        if ((rc = build_topology(*mol, *auxbas, xtopo, why, AUX_LMAX, false)) != MQC_HIP_OK) return fail(rc, "gradient stage: auxiliary basis: " + why);
    }
    const int n = topo.nao, nat = topo.natoms, ns = (int)topo.shells.size(), na = xtopo.nao;
    const size_t nn = (size_t)n * n, g3 = (size_t)nat * 3;
    for (int k = 0; k < 3 * nat; ++k)
        if (!std::isfinite(mol->xyz[k])) return fail(MQC_HIP_ERR_VALIDATION, "gradient stage: non-finite input (a coordinate)");
    auto finite = [](const double* p, size_t count) {
        for (size_t k = 0; k < count; ++k) if (!std::isfinite(p[k])) return false;
        return true;
    };
    if (!std::isfinite(a->exx)) return fail(MQC_HIP_ERR_VALIDATION, "gradient stage: non-finite input (exx)");
    if (need_d && (!finite(a->D, nn) || (uhf && !finite(a->D_beta, nn)))) return fail(MQC_HIP_ERR_VALIDATION, "gradient stage: non-finite input (the density)");
    if (need_w) {
        if (!finite(a->C, nn) || !finite(a->eps, n) || (uhf && (!finite(a->C_beta, nn) || !finite(a->eps_beta, n))))
            return fail(MQC_HIP_ERR_VALIDATION, "gradient stage: non-finite input (C, eps)");
        if (a->n_occ < 0 || a->n_occ > n || (uhf && (a->n_beta < 0 || a->n_beta > n)))
            return fail(MQC_HIP_ERR_VALIDATION, "gradient stage: occupations outside 0..n_ao");
    }
    if (a->g2e && a->Q && (!finite(a->Q, (size_t)ns * ns) || !std::isfinite(a->q_thresh)))
        return fail(MQC_HIP_ERR_VALIDATION, "gradient stage: non-finite input (Q, q_thresh)");
    int pA = a->pair_a, pB = a->pair_b;
    if (a->g1e_pair) {
        if (pA < 0 || pB < 0 || pA >= ns || pB >= ns) return fail(MQC_HIP_ERR_VALIDATION, "gradient stage: the shell pair (pair_a, pair_b) does not exist");
        if (pA < pB) std::swap(pA, pB);                                           // the pair list's order, then la >= lb
        if (topo.shells[pA].l < topo.shells[pB].l) std::swap(pA, pB);
    }
    // ---- the rows of the per-row mode: a slice of the topology's own list, or of the density-fitted term's lists
    const std::vector<int>* list = nullptr;
    std::vector<int> t3[4][4][4], t2[4][4];
    const int* rcl = a->row_class;
    if (want_rows) {
        if (mode == 0) {
            for (auto& cl : topo.classes)
                if (cl.la == rcl[0] && cl.lb == rcl[1] && cl.lc == rcl[2] && cl.ld == rcl[3] && !cl.quartets.empty()) list = &cl.quartets;
        } else {
            if (rcl[3] != 0 || (mode == 2 && rcl[1] != 0)) return fail(MQC_HIP_ERR_VALIDATION, "gradient stage: the empty slots of a density-fitted class hold an s shell (l = 0)");
            df_gradient_lists(topo, xtopo, t3, t2);
            list = mode == 1 ? &t3[rcl[0]][rcl[1]][rcl[2]] : &t2[rcl[0]][rcl[2]];
            if (list->empty()) list = nullptr;
        }
        if (!list) return fail(MQC_HIP_ERR_VALIDATION, "gradient stage: the topology has no class (" + std::to_string(rcl[0]) + " " + std::to_string(rcl[1]) +
                                                       "|" + std::to_string(rcl[2]) + " " + std::to_string(rcl[3]) + ")");
        const int64_t len = (int64_t)(list->size() / 4);
        if (a->row_start < 0 || a->row_count > 4096 || a->row_start + a->row_count > len)
            return fail(MQC_HIP_ERR_VALIDATION, "gradient stage: slice outside the list (rows " + std::to_string(a->row_start) + " .. " +
                                                std::to_string(a->row_start + a->row_count) + " of " + std::to_string(len) + ", at most 4096 at a time)");
        if (device_rows && mode != 0 && !finite(a->gam, mode == 1 ? (size_t)na * nn : (size_t)na * na))
            return fail(MQC_HIP_ERR_VALIDATION, "gradient stage: non-finite input (gam)");
    }
    // ---- nothing refused from here on
    const size_t nrow = want_rows ? (size_t)a->row_count : 0;
    if (want_rows) {
        *a->class_length = (int64_t)(list->size() / 4);
        std::memcpy(a->rows, list->data() + 4 * (size_t)a->row_start, sizeof(int) * 4 * nrow);
    }
    if (!whole && !device_rows) return MQC_HIP_OK;
    HIP_CHECK_RET(hipSetDevice(ctx->device));
    if ((rc = upload_topology(ctx, topo, sb.td)) != MQC_HIP_OK) return rc;
    TopologyDev tdx{};
    if (device_rows && mode != 0 && (rc = upload_topology(ctx, xtopo, tdx, &ctx->lane[0].aux)) != MQC_HIP_OK) return rc;
    BatchPlan plan;
    plan.n = n; plan.npair = topo.npair; plan.natoms = nat; plan.two_e = TWO_E_NONE;
    plan.uhf = uhf; plan.nocc = a->n_occ; plan.nalpha = a->n_occ; plan.nbeta = a->n_beta;
    plan_layout(plan, 1, ns, topo.lmax, false);
    BatchView& bv = sb.bv;
    if ((rc = carve_slot(ctx, make_slot(ctx, 0, nullptr), plan, sb.td, 1, bv)) != MQC_HIP_OK) return rc;
    bv.nocc = a->n_occ; bv.nalpha = a->n_occ; bv.nbeta = a->n_beta; bv.exx = a->exx;
    hipStream_t s = ctx->lane[0].stream;
    // [g1e | pair | g2e | rows ...] gradients, [W | Dtot], Q, gam, then the lists
    const size_t gdoubles = ((3 + nrow) * g3 + 7) & ~size_t(7);
    const size_t gam_doubles = (device_rows && mode != 0) ? (mode == 1 ? (size_t)na * nn : (size_t)na * na) : 0;
    const size_t lint = grad_list_ints(bv, topo) + 64;
    static DevicePool pool;
    char* base = (char*)pool.ensure(sizeof(double) * (gdoubles + 2 * nn + (size_t)ns * ns + gam_doubles + 8) + sizeof(int) * (lint + 4 * nrow + 64));
    if (!base) return fail(MQC_HIP_ERR_DEVICE, "out of device memory (gradient stage)");
    double* d_g1e = (double*)base; double* d_pair = d_g1e + g3; double* d_g2e = d_pair + g3; double* d_rows = d_g2e + g3;
    double* work = d_g1e + gdoubles;
    double* d_q = work + 2 * nn;
    double* d_gam = d_q + (((size_t)ns * ns + 7) & ~size_t(7));
    int* d_lists = (int*)(d_gam + gam_doubles);
    int* d_rowlist = d_lists + lint;
    HIP_CHECK_RET(hipMemcpyAsync(bv.xyz, mol->xyz, sizeof(double) * g3, hipMemcpyHostToDevice, s));
    HIP_CHECK_RET(hipMemsetAsync(bv.istate, 0, sizeof(int) * 4, s));
    HIP_CHECK_RET(hipMemsetAsync(d_g1e, 0, sizeof(double) * gdoubles, s));
    if (need_d) HIP_CHECK_RET(hipMemcpyAsync(bv.D, a->D, sizeof(double) * nn, hipMemcpyHostToDevice, s));
    if (need_d && uhf) HIP_CHECK_RET(hipMemcpyAsync(bv.Db, a->D_beta, sizeof(double) * nn, hipMemcpyHostToDevice, s));
    if (need_w) {
        HIP_CHECK_RET(hipMemcpyAsync(bv.C, a->C, sizeof(double) * nn, hipMemcpyHostToDevice, s));
        HIP_CHECK_RET(hipMemcpyAsync(bv.eps, a->eps, sizeof(double) * n, hipMemcpyHostToDevice, s));
        if (uhf) {
            HIP_CHECK_RET(hipMemcpyAsync(bv.Cb, a->C_beta, sizeof(double) * nn, hipMemcpyHostToDevice, s));
            HIP_CHECK_RET(hipMemcpyAsync(bv.epsb, a->eps_beta, sizeof(double) * n, hipMemcpyHostToDevice, s));
        }
    } else {
        // the weighted-density kernel still runs (it is a step of the stage): on zeros
        HIP_CHECK_RET(hipMemsetAsync(bv.C, 0, sizeof(double) * nn, s));
        HIP_CHECK_RET(hipMemsetAsync(bv.eps, 0, sizeof(double) * n, s));
        if (uhf) { HIP_CHECK_RET(hipMemsetAsync(bv.Cb, 0, sizeof(double) * nn, s)); HIP_CHECK_RET(hipMemsetAsync(bv.epsb, 0, sizeof(double) * n, s)); }
        bv.nocc = bv.nalpha = bv.nbeta = 0;
    }
    if (!need_d) {
        HIP_CHECK_RET(hipMemsetAsync(bv.D, 0, sizeof(double) * nn, s));
        if (uhf) HIP_CHECK_RET(hipMemsetAsync(bv.Db, 0, sizeof(double) * nn, s));
    }
    grad_prepare_kernels();
    const double* Dtot = launch_grad_densities(bv, work, s);
    size_t off = 0;
    if (a->g1e) grad_one_electron(bv, topo, Dtot, work, d_g1e, d_lists, off, s);
    if (a->g1e_pair) {
        const int pr[2] = {pA, pB};
        HIP_CHECK_RET(hipMemcpyAsync(d_lists + off, pr, sizeof(pr), hipMemcpyHostToDevice, s));
        HIP_CHECK_RET(hipStreamSynchronize(s));                                   // pr lives on this frame
        launch_grad1e_pairs(bv, topo.shells[pA].l, topo.shells[pB].l, d_lists + off, 1, Dtot, work, d_pair, s);
        off += 2;
    }
    if (a->g2e) {
        if (a->Q) HIP_CHECK_RET(hipMemcpyAsync(d_q, a->Q, sizeof(double) * (size_t)ns * ns, hipMemcpyHostToDevice, s));
        if (!grad_two_electron(bv, topo, nullptr, Dtot, d_g2e, d_lists, off, a->Q ? d_q : nullptr, a->q_thresh, s, why))
            return fail(MQC_HIP_ERR_UNSUPPORTED, why);
    }
    if (device_rows) {
        HIP_CHECK_RET(hipMemcpyAsync(d_rowlist, a->rows, sizeof(int) * 4 * nrow, hipMemcpyHostToDevice, s));
        BatchView vx = bv;
        if (mode != 0) {
            vx.naux = na; vx.aux = tdx;
            HIP_CHECK_RET(hipMemcpyAsync(d_gam, a->gam, sizeof(double) * gam_doubles, hipMemcpyHostToDevice, s));
        }
        // one single-wave launch per row: a long slice goes round four streams of its own, which start after the uploads
        // above and which the lane's stream waits for
        struct Side {
            hipStream_t st[4] = {};
            hipEvent_t ev[5] = {};
            int n = 0;
            ~Side()
            {
                for (int k = 0; k < n; ++k) (void)hipStreamDestroy(st[k]);
                for (auto& e : ev) if (e) (void)hipEventDestroy(e);
            }
        } side;
        if (nrow >= 64) {
            for (auto& e : side.ev) HIP_CHECK_RET(hipEventCreateWithFlags(&e, hipEventDisableTiming));
            for (; side.n < 4; ++side.n) HIP_CHECK_RET(hipStreamCreateWithFlags(&side.st[side.n], hipStreamNonBlocking));
            HIP_CHECK_RET(hipEventRecord(side.ev[4], s));
            for (int k = 0; k < 4; ++k) HIP_CHECK_RET(hipStreamWaitEvent(side.st[k], side.ev[4], 0));
        }
        for (size_t r = 0; r < nrow; ++r)
            if (!launch_eri_grad_rows(vx, rcl[0], rcl[1], rcl[2], rcl[3], d_rowlist + 4 * r, 1, mode == 0 ? Dtot : nullptr,
                                      mode == 0 && uhf ? bv.Db : nullptr, d_rows + r * g3, mode, mode == 0 ? nullptr : d_gam,
                                      side.n ? side.st[r & 3] : s, why)) {
                (void)hipDeviceSynchronize();
                return fail(MQC_HIP_ERR_UNSUPPORTED, why);
            }
        for (int k = 0; k < side.n; ++k) {
            HIP_CHECK_RET(hipEventRecord(side.ev[k], side.st[k]));
            HIP_CHECK_RET(hipStreamWaitEvent(s, side.ev[k], 0));
        }
        if ((rc = sync_and_check(s)) != MQC_HIP_OK) return rc;          // before the side streams go
    }
    if ((rc = sync_and_check(s)) != MQC_HIP_OK) return rc;
    if (a->w) HIP_CHECK_RET(hipMemcpy(a->w, work, sizeof(double) * nn, hipMemcpyDeviceToHost));
    if (a->g1e) HIP_CHECK_RET(hipMemcpy(a->g1e, d_g1e, sizeof(double) * g3, hipMemcpyDeviceToHost));
    if (a->g1e_pair) HIP_CHECK_RET(hipMemcpy(a->g1e_pair, d_pair, sizeof(double) * g3, hipMemcpyDeviceToHost));
    if (a->g2e) HIP_CHECK_RET(hipMemcpy(a->g2e, d_g2e, sizeof(double) * g3, hipMemcpyDeviceToHost));
    if (device_rows) HIP_CHECK_RET(hipMemcpy(a->g_rows, d_rows, sizeof(double) * nrow * g3, hipMemcpyDeviceToHost));
    return MQC_HIP_OK;
}

int mqc_hip_jk_incore(mqc_hip_context* ctx, const mqc_hip_molecule_t* mol, const mqc_hip_basis_t* bas, const double* D, double* J, double* K)
{
    StageBatch sb;
    int rc = stage_setup(ctx, mol, bas, true, sb);
    if (rc != MQC_HIP_OK) return rc;
    const size_t nn = (size_t)sb.topo.nao * sb.topo.nao;
    launch_eri(sb.bv, sb.topo, 0.0, ctx->lane[0].stream);
    HIP_CHECK_RET(hipMemcpyAsync(sb.bv.D, D, sizeof(double) * nn, hipMemcpyHostToDevice, ctx->lane[0].stream));
    launch_jk_incore(sb.bv, false, ctx->lane[0].stream);
    if ((rc = sync_and_check(ctx->lane[0].stream)) != MQC_HIP_OK) return rc;
    HIP_CHECK_RET(hipMemcpy(J, sb.bv.J, sizeof(double) * nn, hipMemcpyDeviceToHost));
    HIP_CHECK_RET(hipMemcpy(K, sb.bv.K, sizeof(double) * nn, hipMemcpyDeviceToHost));
    return MQC_HIP_OK;
}

// J and K of one fragment by the direct build: no tensor, the digest kernels over every unique quartet
int mqc_hip_jk_direct(mqc_hip_context* ctx, const mqc_hip_molecule_t* mol, const mqc_hip_basis_t* bas, double schwarz_tol, double exx,
                      const double* D, double* J, double* K)
{
    if (!D || !J || !K) return fail(MQC_HIP_ERR_VALIDATION, "null argument");
    if (!(schwarz_tol >= 0.0) || !(exx >= 0.0) || !std::isfinite(schwarz_tol) || !std::isfinite(exx))
        return fail(MQC_HIP_ERR_VALIDATION, "direct J/K: schwarz_tol and exx must be finite and not negative");
    StageBatch sb;
    int rc = stage_setup(ctx, mol, bas, false, sb, TWO_E_DIRECT);
    if (rc != MQC_HIP_OK) return rc;
    if (sb.topo.nao > 256) return fail(MQC_HIP_ERR_UNSUPPORTED, "fragment too large (n_ao <= 256)");
    const size_t nn = (size_t)sb.topo.nao * sb.topo.nao;
    sb.bv.exx = exx;
    HIP_CHECK_RET(hipMemsetAsync(sb.bv.eri_count, 0, sizeof(unsigned long long), ctx->lane[0].stream));
    HIP_CHECK_RET(hipMemcpyAsync(sb.bv.D, D, sizeof(double) * nn, hipMemcpyHostToDevice, ctx->lane[0].stream));
    launch_direct_setup(sb.bv, sb.topo, ctx->lane[0].stream);
    launch_jk_direct(sb.bv, sb.topo, schwarz_tol, false, ctx->lane[0].stream);
    if ((rc = sync_and_check(ctx->lane[0].stream)) != MQC_HIP_OK) return rc;
    HIP_CHECK_RET(hipMemcpy(J, sb.bv.J, sizeof(double) * nn, hipMemcpyDeviceToHost));
    HIP_CHECK_RET(hipMemcpy(K, sb.bv.K, sizeof(double) * nn, hipMemcpyDeviceToHost));
    return MQC_HIP_OK;
}

int mqc_hip_coulomb_batch(mqc_hip_context* ctx, int64_t nfrag, const mqc_hip_molecule_t* mols, const mqc_hip_basis_t* bas,
                          int32_t n_source_atoms, const double* D, double* J)
{
    if (!ctx || nfrag < 0 || (nfrag > 0 && (!mols || !bas || !D || !J))) return fail(MQC_HIP_ERR_VALIDATION, "null argument");
    if (nfrag == 0) return MQC_HIP_OK;
    HIP_CHECK_RET(hipSetDevice(ctx->device));
    if (!same_elements(mols, nfrag))
        return fail(MQC_HIP_ERR_VALIDATION, "coulomb batch: every fragment must have the elements of the first (one topology per call)");
    Topology topo;
    std::string err;
    int rc = build_topology(mols[0], *bas, topo, err);
    if (rc != MQC_HIP_OK) return fail(rc, err);
    if (n_source_atoms < 0 || n_source_atoms >= topo.natoms) return fail(MQC_HIP_ERR_VALIDATION, "coulomb batch: n_source_atoms must be within 0 .. n_atoms - 1");
    const bool cross = n_source_atoms > 0;
    if (cross) {
        // keep the quartets that join a pair on the leading atoms with a pair on the source atoms (either side may be
        // the bra: the class fixes the order); twin entries are dropped with the rest, the plain lists cover everything
        const int first_src = topo.natoms - n_source_atoms;
        auto on_src = [&](int sh) { return topo.shells[sh].atom >= first_src; };
        for (auto& cl : topo.classes) {
            std::vector<int> q, sets;
            for (size_t e = 0; 4 * e + 3 < cl.quartets.size(); ++e) {
                const int* s4 = &cl.quartets[4 * e];
                const bool bra_src = on_src(s4[0]) && on_src(s4[1]), bra_lead = !on_src(s4[0]) && !on_src(s4[1]);
                const bool ket_src = on_src(s4[2]) && on_src(s4[3]), ket_lead = !on_src(s4[2]) && !on_src(s4[3]);
                if (!((bra_src && ket_lead) || (bra_lead && ket_src))) continue;
                q.insert(q.end(), s4, s4 + 4);
                if (e < cl.set_quartets.size()) sets.push_back(cl.set_quartets[e]);
            }
            cl.quartets.swap(q); cl.set_quartets.swap(sets);
            cl.twin_entries.clear(); cl.rest.clear(); cl.set_twin.clear(); cl.set_rest.clear();
        }
        topo.key += "|cross" + std::to_string(n_source_atoms);
    }
    TopologyDev td;
    rc = upload_topology(ctx, topo, td);
    if (rc != MQC_HIP_OK) return rc;
    const int n = topo.nao;
    const size_t nn = (size_t)n * n;
    // full mode: in-core (the packed tensor of every fragment of a chunk resident at once, chunks sized to the free HBM).
    // cross mode: the direct digest over the filtered lists -- no tensor at all, the few (leading | source) quartets
    // are contracted with the density as they are formed (Schwarz screening at 1e-12)
    static const bool cross_incore = env_opt_in("MQC_HIP_COULOMB_CROSS_INCORE");
    const bool direct = cross && !cross_incore;
    if (!direct && !incore_supported(topo.nao)) return fail(MQC_HIP_ERR_UNSUPPORTED, "fragment too large for the in-core ERI path");
    if (topo.nao > 256) return fail(MQC_HIP_ERR_UNSUPPORTED, "fragment too large (n_ao <= 256)");
    const BatchPlan plan = stage_plan(topo, direct ? TWO_E_DIRECT : TWO_E_INCORE, (int)std::min<int64_t>(nfrag, 1 << 30));
    size_t free_b = 0, total_b = 0;
    (void)hipMemGetInfo(&free_b, &total_b);
    free_b += ctx->lane[0].pool[POOL_MAIN].capacity() + ctx->lane[0].pool[POOL_ERI].capacity();
    const int64_t chunk = stage_chunk_fragments(free_b, fragment_bytes(plan), nfrag);
    const Slot sl0 = make_slot(ctx, 0, nullptr);
    std::vector<double> hx;
    for (int64_t start = 0; start < nfrag; start += chunk) {
        const int nf = (int)std::min<int64_t>(chunk, nfrag - start);
        BatchView bv{};
        rc = carve_slot(ctx, sl0, plan, td, nf, bv);
        if (rc != MQC_HIP_OK) return rc;
        // only J is read back: the direct digest skips its exchange updates when exx = 0; the in-core kernels
        // form K alongside J in the same pass over the tensor either way
        bv.nocc = std::max(1, topo.nelec / 2); bv.exx = direct ? 0.0 : 1.0;
        gather_xyz(mols + start, nf, topo.natoms, hx);
        HIP_CHECK_RET(hipMemcpyAsync(bv.xyz, hx.data(), sizeof(double) * hx.size(), hipMemcpyHostToDevice, ctx->lane[0].stream));
        HIP_CHECK_RET(hipMemsetAsync(bv.istate, 0, sizeof(int) * (size_t)nf * 4, ctx->lane[0].stream));
        HIP_CHECK_RET(hipMemsetAsync(bv.eri_count, 0, sizeof(unsigned long long), ctx->lane[0].stream));
        HIP_CHECK_RET(hipMemcpyAsync(bv.D, D + (size_t)start * nn, sizeof(double) * nn * nf, hipMemcpyHostToDevice, ctx->lane[0].stream));
        if (direct) {
            launch_direct_setup(bv, topo, ctx->lane[0].stream);
            launch_jk_direct(bv, topo, 1.0e-12, false, ctx->lane[0].stream);
        } else {
            // a restricted list leaves most of the tensor untouched: those blocks must read as zero
            if (cross) HIP_CHECK_RET(hipMemsetAsync(bv.eri, 0, sizeof(double) * (size_t)nf * bv.eri_stride, ctx->lane[0].stream));
            launch_eri(bv, topo, 0.0, ctx->lane[0].stream, hx.data());
            launch_jk_incore(bv, false, ctx->lane[0].stream);
        }
        if ((rc = sync_and_check(ctx->lane[0].stream)) != MQC_HIP_OK) return rc;
        HIP_CHECK_RET(hipMemcpy(J + (size_t)start * nn, bv.J, sizeof(double) * nn * nf, hipMemcpyDeviceToHost));
    }
    return MQC_HIP_OK;
}

// V(r) = sum_A Z_A/|r - R_A| - tr(D u_r) at the points of every fragment (kern_esp.hip).  Validation first (nothing is
// written on a refusal), then chunks of fragments sized to the free HBM: geometry, densities and points up, the
// primitive-pair records formed on the device, the point kernels, the potentials back.
int mqc_hip_esp_batch(mqc_hip_context* ctx, int64_t nfrag, const mqc_hip_molecule_t* mols, const mqc_hip_basis_t* bas, const double* D,
                      int32_t max_points, const int32_t* n_points, const double* points, int32_t include_nuclei, double* esp)
{
    if (!ctx || nfrag < 0 || max_points < 0) return fail(MQC_HIP_ERR_VALIDATION, "esp batch: null context or negative count");
    if (n_points)
        for (int64_t i = 0; i < nfrag; ++i)
            if (n_points[i] < 0 || n_points[i] > max_points)
                return fail(MQC_HIP_ERR_VALIDATION, "esp batch: n_points[" + std::to_string(i) + "] = " + std::to_string(n_points[i]) +
                                                        " is outside 0 .. max_points");
    if (nfrag == 0 || max_points == 0) return MQC_HIP_OK;
    if (!mols || !bas || !D || !points || !esp) return fail(MQC_HIP_ERR_VALIDATION, "null argument");
    HIP_CHECK_RET(hipSetDevice(ctx->device));
    const int na = mols[0].n_atoms;
    // fragment by fragment, elements before coordinates: the first fragment at fault names the refusal
    const bool same = same_elements(mols, nfrag);
    for (int64_t i = 0; i < nfrag; ++i) {
        if (!same && !same_elements(mols, i + 1))
            return fail(MQC_HIP_ERR_VALIDATION, "esp batch: every fragment must have the elements of the first (one topology per call)");
        for (int k = 0; k < 3 * na; ++k)
            if (!std::isfinite(mols[i].xyz[k])) return fail(MQC_HIP_ERR_VALIDATION, "esp batch: non-finite atomic coordinate in fragment " + std::to_string(i));
    }
    Topology topo;
    std::string err;
    int rc = build_topology(mols[0], *bas, topo, err, KERNEL_LMAX, false);
    if (rc != MQC_HIP_OK) return fail(rc, err);
    if (topo.nao > 256) return fail(MQC_HIP_ERR_UNSUPPORTED, "fragment too large (n_ao <= 256)");
    const size_t mp = (size_t)max_points;
    for (int64_t i = 0; i < nfrag; ++i) {
        const int np = n_points ? n_points[i] : max_points;
        const double* p = points + (size_t)i * 3 * mp;
        for (int k = 0; k < 3 * np; ++k)
            if (!std::isfinite(p[k])) return fail(MQC_HIP_ERR_VALIDATION, "esp batch: non-finite coordinate of point " + std::to_string(k / 3) + " of fragment " + std::to_string(i));
        if (!include_nuclei) continue;
        for (int a = 0; a < na; ++a) {
            if (topo.zeff[a] == 0.0) continue;
            const double* r = mols[i].xyz + 3 * a;
            for (int k = 0; k < np; ++k) {
                const double dx = p[3 * k] - r[0], dy = p[3 * k + 1] - r[1], dz = p[3 * k + 2] - r[2];
                if (dx * dx + dy * dy + dz * dz < 1.0e-20)
                    return fail(MQC_HIP_ERR_VALIDATION, "esp batch: point " + std::to_string(k) + " of fragment " + std::to_string(i) +
                                                            " lies on nucleus " + std::to_string(a) + " (the nuclear potential diverges; include_nuclei = 0 gives the electronic part)");
            }
        }
    }
    TopologyDev td;
    rc = upload_topology(ctx, topo, td);
    if (rc != MQC_HIP_OK) return rc;
    const size_t nn = (size_t)topo.nao * topo.nao, rec = esp_record_doubles(topo);
    auto up = [](size_t doubles) { return (doubles + 31) & ~size_t(31); };     // every array starts on 256 bytes
    const size_t per_frag = sizeof(double) * (up(3 * (size_t)na) + nn + rec + up(3 * mp) + up(mp) + 32) + 64;
    size_t free_b = 0, total_b = 0;
    (void)hipMemGetInfo(&free_b, &total_b);
    free_b += g_esp_pool.capacity();
    // MQC_HIP_ESP_CHUNK: a smaller cap on the fragments of one chunk (memory-tight hosts; the tests cross a chunk boundary with it)
    int64_t cap = 16384;
    if (const char* e = std::getenv("MQC_HIP_ESP_CHUNK")) cap = std::max(1, std::min(16384, std::atoi(e)));
    const int64_t chunk = stage_chunk_fragments(free_b, per_frag, nfrag, cap);
    std::vector<double> hx, hout;
    std::vector<int> hn;
    for (int64_t start = 0; start < nfrag; start += chunk) {
        const int nf = (int)std::min<int64_t>(chunk, nfrag - start);
        const size_t n_xyz = up((size_t)nf * 3 * na), n_D = up((size_t)nf * nn), n_rec = (size_t)nf * rec, n_pts = up((size_t)nf * 3 * mp),
                     n_out = up((size_t)nf * mp);
        double* base = (double*)g_esp_pool.ensure(sizeof(double) * (n_xyz + n_D + n_rec + n_pts + n_out) + sizeof(int) * ((size_t)nf + 64));
        if (!base) return fail(MQC_HIP_ERR_DEVICE, "out of device memory (esp batch)");
        double *d_xyz = base, *d_D = d_xyz + n_xyz, *d_rec = d_D + n_D, *d_pts = d_rec + n_rec, *d_out = d_pts + n_pts;
        int* d_np = (int*)(d_out + n_out);
        gather_xyz(mols + start, nf, na, hx);
        hn.resize(nf);
        for (int f = 0; f < nf; ++f) hn[f] = n_points ? n_points[start + f] : max_points;
        HIP_CHECK_RET(hipMemcpyAsync(d_xyz, hx.data(), sizeof(double) * hx.size(), hipMemcpyHostToDevice, ctx->lane[0].stream));
        HIP_CHECK_RET(hipMemcpyAsync(d_np, hn.data(), sizeof(int) * hn.size(), hipMemcpyHostToDevice, ctx->lane[0].stream));
        HIP_CHECK_RET(hipMemcpyAsync(d_D, D + (size_t)start * nn, sizeof(double) * nn * nf, hipMemcpyHostToDevice, ctx->lane[0].stream));
        // a fragment's points beyond its count are not touched on the host: each fragment's live part goes up on its own
        const bool full = std::all_of(hn.begin(), hn.end(), [&](int v) { return v == max_points; });
        if (full) HIP_CHECK_RET(hipMemcpyAsync(d_pts, points + (size_t)start * 3 * mp, sizeof(double) * 3 * mp * nf, hipMemcpyHostToDevice, ctx->lane[0].stream));
        for (int f = 0; f < nf && !full; ++f)
            if (hn[f] > 0)
                HIP_CHECK_RET(hipMemcpyAsync(d_pts + (size_t)f * 3 * mp, points + (size_t)(start + f) * 3 * mp, sizeof(double) * 3 * hn[f],
                                             hipMemcpyHostToDevice, ctx->lane[0].stream));
        if (!launch_esp(td, topo, ctx->d_boys, ctx->d_c2s, nf, d_xyz, d_D, d_rec, d_pts, d_np, max_points, include_nuclei ? 1 : 0, d_out, ctx->lane[0].stream, err))
            return fail(MQC_HIP_ERR_DEVICE, err);
        if ((rc = sync_and_check(ctx->lane[0].stream)) != MQC_HIP_OK) return rc;
        hout.resize((size_t)nf * mp);
        HIP_CHECK_RET(hipMemcpy(hout.data(), d_out, sizeof(double) * hout.size(), hipMemcpyDeviceToHost));
        for (int f = 0; f < nf; ++f) std::memcpy(esp + (size_t)(start + f) * mp, &hout[(size_t)f * mp], sizeof(double) * hn[f]);
    }
    return MQC_HIP_OK;
}

// The quadrature stage of an SCF iteration on given densities (include/mqc_hip.h).  Nothing here is private to the
// call: plan_batch and plan_layout decide what an SCF batch of nfrag fragments with this functional would get, carve_slot
// lays the chunk out, and the grid, the weights, the radial cache and launch_xc are the driver's own (prepare, scf_loop).
int mqc_hip_xc_batch(mqc_hip_context* ctx, int64_t nfrag, const mqc_hip_molecule_t* mols, const mqc_hip_basis_t* bas, const char* functional,
                     int32_t grid_level, int32_t unrestricted, const double* D, double* e_xc, double* n_electrons, double* V_xc)
{
    if (!ctx || !mols || !bas || !functional || !D || !e_xc || !n_electrons || !V_xc) return fail(MQC_HIP_ERR_VALIDATION, "xc batch: null argument");
    if (nfrag < 1) return fail(MQC_HIP_ERR_VALIDATION, "xc batch: n_fragments must be at least 1");
    HIP_CHECK_RET(hipSetDevice(ctx->device));
    if (mols[0].n_atoms <= 0 || !same_elements(mols, nfrag))
        return fail(MQC_HIP_ERR_VALIDATION, "xc batch: every fragment must have the elements of the first (one topology per call)");
    mqc_hip_scf_options_t opts;
    mqc_hip_default_options(&opts);
    if (std::strlen(functional) >= sizeof(opts.functional)) return fail(MQC_HIP_ERR_UNSUPPORTED, "xc batch: functional name too long");
    std::snprintf(opts.functional, sizeof(opts.functional), "%s", functional);
    opts.grid_level = grid_level;
    opts.unrestricted = unrestricted ? 1 : 0;
    Topology topo;
    std::string msg;
    int rc = build_topology(mols[0], *bas, topo, msg, KERNEL_LMAX, false);
    if (rc != MQC_HIP_OK) return fail(rc, msg);
    const int ntot = (int)std::min<int64_t>(nfrag, 1 << 30);
    BatchPlan plan;
    if ((rc = plan_batch(opts, topo, ntot, plan, msg)) != MQC_HIP_OK) return fail(rc, msg);
    if (plan.xc.ncomp == 0) return fail(MQC_HIP_ERR_VALIDATION, "xc batch: the functional has no grid part (Hartree-Fock)");
    if (plan.uhf && !unrestricted) return fail(MQC_HIP_ERR_VALIDATION, "xc batch: an open-shell fragment takes spin densities (unrestricted != 0)");
    Batch b{topo, nullptr, opts, nullptr};
    if ((rc = upload_topology(ctx, topo, b.td)) != MQC_HIP_OK) return rc;
    if ((rc = upload_grid(ctx, b, ctx->lane[0].grid, ctx->lane[0].stream)) != MQC_HIP_OK) return rc;
    plan.npts = b.grid.npts;
    plan_layout(plan, ntot, (int)topo.shells.size(), topo.lmax, xc_radial_cache_on());

    const int n = topo.nao, nspin = plan.uhf ? 2 : 1;
    const size_t nn = (size_t)n * n;
    constexpr size_t GUARD = 4096;         // bytes compared on either side of the accumulator
    size_t free_b = 0, total_b = 0;
    (void)hipMemGetInfo(&free_b, &total_b);
    free_b += ctx->lane[0].pool[POOL_MAIN].capacity() + ctx->lane[0].pool[POOL_ERI].capacity() + ctx->lane[0].pool[POOL_GRIDW].capacity();
    const int64_t chunk = stage_chunk_fragments(free_b, fragment_bytes(plan), nfrag);
    const Slot sl0 = make_slot(ctx, 0, nullptr);
    hipStream_t s = ctx->lane[0].stream;
    std::vector<double> hx, acc, scal;
    std::vector<unsigned char> before(2 * GUARD), after(2 * GUARD);
    for (int64_t start = 0; start < nfrag; start += chunk) {
        const int nf = (int)std::min<int64_t>(chunk, nfrag - start);
        {
            // room behind the last array of the quadrature's pool, so that the guard band exists where nothing follows V_xc
            BatchView probe{};
            const ChunkBytes need = carve_chunk(plan, nf, nullptr, probe);
            if (!sl0.lane->pool[POOL_GRIDW].ensure(need.pool[POOL_GRIDW] + GUARD + 256)) return fail(MQC_HIP_ERR_DEVICE, "out of device memory (grid weights)");
        }
        BatchView bv{};
        bv.nalpha = plan.nalpha; bv.nbeta = plan.nbeta; bv.nocc = plan.nocc;
        bv.exx = plan.rsh ? 1.0 : plan.xc.exx; bv.e_tol = opts.energy_tol; bv.d_tol = opts.density_tol;
        bv.max_iter = opts.max_iter; bv.diis_size = opts.diis_size;
        bv.xc = plan.xc; bv.grid = b.grid;
        if ((rc = carve_slot(ctx, sl0, plan, b.td, nf, bv)) != MQC_HIP_OK) return rc;
        gather_xyz(mols + start, nf, topo.natoms, hx);
        HIP_CHECK_RET(hipMemcpyAsync(bv.xyz, hx.data(), sizeof(double) * hx.size(), hipMemcpyHostToDevice, s));
        HIP_CHECK_RET(hipMemsetAsync(bv.istate, 0, sizeof(int) * (size_t)nf * 4, s));
        if (plan.uhf) {
            for (int f = 0; f < nf; ++f) {
                const double* d = D + (size_t)(start + f) * 2 * nn;
                HIP_CHECK_RET(hipMemcpyAsync(bv.D + (size_t)f * nn, d, sizeof(double) * nn, hipMemcpyHostToDevice, s));
                HIP_CHECK_RET(hipMemcpyAsync(bv.Db + (size_t)f * nn, d + nn, sizeof(double) * nn, hipMemcpyHostToDevice, s));
            }
        } else HIP_CHECK_RET(hipMemcpyAsync(bv.D, D + (size_t)start * nn, sizeof(double) * nn * nf, hipMemcpyHostToDevice, s));
        launch_becke_weights(bv, s);
        if (bv.grid.rad) launch_xc_radial_cache(bv, s);
        if ((rc = stage_check("grid weights")) != MQC_HIP_OK) return rc;
        // Poison.  launch_xc zeroes the accumulator itself, so a tile no workgroup owns reads as zero, not NaN, and the
        // comparison with the reference finds it; what the poison of the array cannot show is a write OUTSIDE it.  The
        // bytes on either side -- the end of the Becke weights in front, the radial cache behind or (where the plan has
        // none) poisoned spare room of the pool -- do not change in a quadrature launch: they are compared across it.
        const size_t vx_bytes = sizeof(double) * (size_t)nf * nn * nspin;
        unsigned char* lo = (unsigned char*)bv.Vxc - GUARD;
        unsigned char* hi = (unsigned char*)bv.Vxc + vx_bytes;
        if ((unsigned char*)bv.grid.weights > lo) return fail(MQC_HIP_ERR_DEVICE, "xc batch: the grid is smaller than the guard band");
        HIP_CHECK_RET(hipMemsetAsync(bv.Vxc, 0xFF, vx_bytes, s));
        if (!bv.grid.rad) HIP_CHECK_RET(hipMemsetAsync(hi, 0xFF, GUARD, s));
        HIP_CHECK_RET(hipMemcpyAsync(before.data(), lo, GUARD, hipMemcpyDeviceToHost, s));
        HIP_CHECK_RET(hipMemcpyAsync(before.data() + GUARD, hi, GUARD, hipMemcpyDeviceToHost, s));
        launch_xc(bv, false, s);
        HIP_CHECK_RET(hipMemcpyAsync(after.data(), lo, GUARD, hipMemcpyDeviceToHost, s));
        HIP_CHECK_RET(hipMemcpyAsync(after.data() + GUARD, hi, GUARD, hipMemcpyDeviceToHost, s));
        acc.resize((size_t)nf * nn * nspin); scal.resize((size_t)nf * 8);
        HIP_CHECK_RET(hipMemcpyAsync(acc.data(), bv.Vxc, vx_bytes, hipMemcpyDeviceToHost, s));
        HIP_CHECK_RET(hipMemcpyAsync(scal.data(), bv.scal, sizeof(double) * scal.size(), hipMemcpyDeviceToHost, s));
        HIP_CHECK_RET(hipStreamSynchronize(s));
        if ((rc = stage_check("exchange-correlation quadrature")) != MQC_HIP_OK) return rc;
        if (std::memcmp(before.data(), after.data(), 2 * GUARD) != 0)
            return fail(MQC_HIP_ERR_DEVICE, "xc batch: the quadrature wrote outside the V_xc accumulator");
        // V_xc = A + A^T (scf_step's Fock assembly); the beta accumulators follow the alpha ones of the whole chunk
        for (int f = 0; f < nf; ++f) {
            e_xc[start + f] = scal[8 * (size_t)f + 5];
            n_electrons[start + f] = scal[8 * (size_t)f + 6];
            for (int sp = 0; sp < nspin; ++sp) {
                const double* a = acc.data() + ((size_t)sp * nf + f) * nn;
                double* v = V_xc + ((size_t)(start + f) * nspin + sp) * nn;
                for (int i = 0; i < n; ++i)
                    for (int j = 0; j < n; ++j) v[(size_t)i * n + j] = a[(size_t)i * n + j] + a[(size_t)j * n + i];
            }
        }
    }
    return MQC_HIP_OK;
}

// The density-fitted J/K stage of an SCF iteration on given tensors (include/mqc_hip.h).  No molecule: the kernels read
// n, npair, naux, nocc, exx, D, C, df_b and istate only.  The arrays are the ones carve_slot gives a density-fitted
// batch of this shape, and launch_df_jk runs once, as jk_one runs it.
int mqc_hip_df_jk_batch(mqc_hip_context* ctx, int64_t nfrag, int32_t n_ao, int32_t n_occ, int32_t n_aux, double exx, const double* B,
                        const double* D, const double* C, double* J, double* K, char* route, int32_t route_len)
{
    if (!ctx || !B || !D || !C || !J || !K || !route || route_len < 1) return fail(MQC_HIP_ERR_VALIDATION, "df jk batch: null argument");
    if (nfrag < 1) return fail(MQC_HIP_ERR_VALIDATION, "df jk batch: n_fragments must be at least 1");
    if (n_ao < 1 || n_ao > 140) return fail(MQC_HIP_ERR_VALIDATION, "df jk batch: n_ao must be within 1..140");
    if (n_occ < 1 || n_occ > n_ao) return fail(MQC_HIP_ERR_VALIDATION, "df jk batch: n_occ must be within 1..n_ao");
    if (n_aux < 1) return fail(MQC_HIP_ERR_VALIDATION, "df jk batch: n_aux must be at least 1");
    if (!(exx >= 0.0) || !std::isfinite(exx)) return fail(MQC_HIP_ERR_VALIDATION, "df jk batch: exx must be finite and not negative");
    HIP_CHECK_RET(hipSetDevice(ctx->device));
    route[0] = 0;
    BatchPlan plan;
    plan.n = n_ao; plan.npair = n_ao * (n_ao + 1) / 2; plan.natoms = 1;
    plan.nalpha = plan.nbeta = plan.nocc = n_occ;
    plan.two_e = TWO_E_DF; plan.naux = n_aux;
    const int ntot = (int)std::min<int64_t>(nfrag, 1 << 30);
    plan_layout(plan, ntot, 1, 0, false);
    const size_t nn = (size_t)n_ao * n_ao, bstride = (size_t)n_aux * plan.npair;
    constexpr size_t GUARD = 1024;         // bytes compared in front of J and behind K (S .. C in front, W behind: never less)
    size_t free_b = 0, total_b = 0;
    (void)hipMemGetInfo(&free_b, &total_b);
    free_b += ctx->lane[0].pool[POOL_MAIN].capacity() + ctx->lane[0].pool[POOL_DF].capacity();
    const int64_t chunk = stage_chunk_fragments(free_b, fragment_bytes(plan), nfrag);
    const Slot sl0 = make_slot(ctx, 0, nullptr);
    const TopologyDev td{};
    hipStream_t s = ctx->lane[0].stream;
    int rc;
    for (int64_t start = 0; start < nfrag; start += chunk) {
        const int nf = (int)std::min<int64_t>(chunk, nfrag - start);
        BatchView bv{};
        bv.nalpha = bv.nbeta = bv.nocc = n_occ; bv.exx = exx;
        if ((rc = carve_slot(ctx, sl0, plan, td, nf, bv)) != MQC_HIP_OK) return rc;
        const size_t jk_bytes = sizeof(double) * (size_t)nf * nn;
        unsigned char* lo = (unsigned char*)bv.J - GUARD;
        unsigned char* mid = (unsigned char*)bv.J + jk_bytes;            // the padding between J and K (under 256 bytes)
        unsigned char* hi = (unsigned char*)bv.K + jk_bytes;
        const size_t pad = (size_t)((unsigned char*)bv.K - mid);
        if (lo < (unsigned char*)bv.xyz || pad > 256) return fail(MQC_HIP_ERR_DEVICE, "df jk batch: J and K are not where the guard band expects them");
        HIP_CHECK_RET(hipMemsetAsync(bv.istate, 0, sizeof(int) * (size_t)nf * 4, s));
        HIP_CHECK_RET(hipMemcpyAsync(bv.df_b, B + (size_t)start * bstride, sizeof(double) * bstride * nf, hipMemcpyHostToDevice, s));
        HIP_CHECK_RET(hipMemcpyAsync(bv.D, D + (size_t)start * nn, jk_bytes, hipMemcpyHostToDevice, s));
        HIP_CHECK_RET(hipMemcpyAsync(bv.C, C + (size_t)start * nn, jk_bytes, hipMemcpyHostToDevice, s));
        // Poison: an element the stage neither zeroes nor writes reads as NaN.  What the poison cannot show is a write
        // OUTSIDE J and K: the bytes in front of J (the end of C), between the two and behind K (the start of W) do not
        // change in a J/K launch and are compared across it.
        HIP_CHECK_RET(hipMemsetAsync(bv.J, 0xFF, jk_bytes, s));
        HIP_CHECK_RET(hipMemsetAsync(bv.K, 0xFF, jk_bytes, s));
        if (pad) HIP_CHECK_RET(hipMemsetAsync(mid, 0xFF, pad, s));
        HIP_CHECK_RET(hipMemsetAsync(hi, 0xFF, GUARD, s));
        std::vector<unsigned char> before(2 * GUARD + 256), after(2 * GUARD + 256);
        HIP_CHECK_RET(hipMemcpyAsync(before.data(), lo, GUARD, hipMemcpyDeviceToHost, s));
        HIP_CHECK_RET(hipMemcpyAsync(before.data() + GUARD, hi, GUARD, hipMemcpyDeviceToHost, s));
        if (pad) HIP_CHECK_RET(hipMemcpyAsync(before.data() + 2 * GUARD, mid, pad, hipMemcpyDeviceToHost, s));
        const DfJkRoute r = launch_df_jk(bv, false, s);
        HIP_CHECK_RET(hipMemcpyAsync(after.data(), lo, GUARD, hipMemcpyDeviceToHost, s));
        HIP_CHECK_RET(hipMemcpyAsync(after.data() + GUARD, hi, GUARD, hipMemcpyDeviceToHost, s));
        if (pad) HIP_CHECK_RET(hipMemcpyAsync(after.data() + 2 * GUARD, mid, pad, hipMemcpyDeviceToHost, s));
        HIP_CHECK_RET(hipMemcpyAsync(J + (size_t)start * nn, bv.J, jk_bytes, hipMemcpyDeviceToHost, s));
        HIP_CHECK_RET(hipMemcpyAsync(K + (size_t)start * nn, bv.K, jk_bytes, hipMemcpyDeviceToHost, s));
        HIP_CHECK_RET(hipStreamSynchronize(s));
        if ((rc = stage_check("density-fitted J/K")) != MQC_HIP_OK) return rc;
        if (std::memcmp(before.data(), after.data(), 2 * GUARD + pad) != 0)
            return fail(MQC_HIP_ERR_DEVICE, "df jk batch: the stage wrote outside J and K");
        if (r.family == DF_JK_WAVE) std::snprintf(route, (size_t)route_len, "wave<%d,%d>", r.a, r.b);
        else if (r.family == DF_JK_MFMA) std::snprintf(route, (size_t)route_len, "mfma<%d,%d,%s>", r.a, r.b, r.flag ? "K" : "J");
        else std::snprintf(route, (size_t)route_len, "v1<%d,%s>", r.a, r.flag ? "lds" : "global");
    }
    return MQC_HIP_OK;
}

// The RI-MP2 stage on given tensors (include/mqc_hip.h).  No molecule: the kernels read n, npair, naux, nocc, df_b, C, eps
// and istate only.  The arrays are the ones carve_slot gives a density-fitted batch of this shape; the launcher's three
// steps (kern_mp2.hip: route, carve, enqueue) run once over all fragments, as launch_rimp2 runs them, with the stage's
// pool region poisoned in between.  ctx == nullptr: the route alone, no device call.
int mqc_hip_rimp2_stage(mqc_hip_context* ctx, int64_t nfrag, int32_t n_ao, int32_t n_occ, int32_t n_aux, int32_t n_frozen, int32_t gx_cap,
                        const double* B, const double* C, const double* eps, const int32_t* nmo, const int32_t* runs, double* e, double* part,
                        double* Bia, int32_t* route)
{
    if (!route) return fail(MQC_HIP_ERR_VALIDATION, "rimp2 stage: null argument (route)");
    if (ctx && (!B || !C || !eps || !nmo || !runs || !e || !part)) return fail(MQC_HIP_ERR_VALIDATION, "rimp2 stage: null argument");
    if (nfrag < 1 || nfrag > (1 << 20)) return fail(MQC_HIP_ERR_VALIDATION, "rimp2 stage: n_fragments must be within 1..2^20");
    if (n_ao < 1 || n_ao > 140) return fail(MQC_HIP_ERR_VALIDATION, "rimp2 stage: n_ao must be within 1..140");
    if (n_occ < 1 || n_occ > n_ao) return fail(MQC_HIP_ERR_VALIDATION, "rimp2 stage: n_occ must be within 1..n_ao");
    if (n_frozen < 0 || n_frozen >= n_occ) return fail(MQC_HIP_ERR_VALIDATION, "rimp2 stage: n_frozen must be within 0..n_occ-1");
    if (n_aux < 1) return fail(MQC_HIP_ERR_VALIDATION, "rimp2 stage: n_aux must be at least 1");
    if (gx_cap < 0) return fail(MQC_HIP_ERR_VALIDATION, "rimp2 stage: workgroups_per_fragment must not be negative");
    if (ctx)
        for (int64_t f = 0; f < nfrag; ++f)
            if (nmo[f] < 0 || nmo[f] > n_ao) return fail(MQC_HIP_ERR_VALIDATION, "rimp2 stage: nmo[" + std::to_string(f) + "] is outside 0..n_ao");
    const int nf = (int)nfrag;
    std::string why;
    Mp2Route r;
    if (!rimp2_route(nf, n_ao, n_occ, n_aux, n_frozen, gx_cap, r, why)) return fail(MQC_HIP_ERR_UNSUPPORTED, why);
    const int32_t rec[MQC_HIP_RIMP2_ROUTE_LEN] = {r.clds ? 1 : 0, r.npf, r.nw, r.oc, r.gx, (int32_t)r.lds, r.napad, r.nvpad,
                                                  r.npairs, r.passes, r.rows, r.narrowed, 0, 0, 0, 0};
    std::memcpy(route, rec, sizeof(rec));
    if (!ctx) return MQC_HIP_OK;
    const int no = n_occ - n_frozen;
    const size_t nn = (size_t)n_ao * n_ao, c_part = (size_t)nf * r.npairs * 2, c_bia = (size_t)nf * no * r.napad * r.nvpad;
    const double nan = std::nan("");
    std::fill(e, e + 2 * (size_t)nf, nan);
    std::fill(part, part + c_part, nan);
    if (Bia) std::fill(Bia, Bia + c_bia, nan);
    if (r.nvpad == 0) {                                 // no virtual orbital: the launcher launches nothing
        std::fill(e, e + 2 * (size_t)nf, 0.0);
        std::fill(part, part + c_part, 0.0);
        return MQC_HIP_OK;
    }
    HIP_CHECK_RET(hipSetDevice(ctx->device));
    BatchPlan plan;
    plan.n = n_ao; plan.npair = n_ao * (n_ao + 1) / 2; plan.natoms = 1;
    plan.nalpha = plan.nbeta = plan.nocc = n_occ;
    plan.two_e = TWO_E_DF; plan.naux = n_aux;
    plan_layout(plan, nf, 1, 0, false);
    size_t free_b = 0, total_b = 0;
    (void)hipMemGetInfo(&free_b, &total_b);
    free_b += ctx->lane[0].pool[POOL_MAIN].capacity() + ctx->lane[0].pool[POOL_DF].capacity();
    // one launch over all fragments (the route depends on their number): no chunks
    if (stage_chunk_fragments(free_b, fragment_bytes(plan) + rimp2_fragment_bytes(n_ao, n_occ, n_aux, n_frozen), nfrag, nfrag) < nfrag)
        return fail(MQC_HIP_ERR_UNSUPPORTED, "rimp2 stage: the batch does not fit the free device memory in one chunk");
    const TopologyDev td{};
    hipStream_t s = ctx->lane[0].stream;
    BatchView bv{};
    bv.nalpha = bv.nbeta = bv.nocc = n_occ; bv.exx = 1.0;
    int rc;
    if ((rc = carve_slot(ctx, make_slot(ctx, 0, nullptr), plan, td, nf, bv)) != MQC_HIP_OK) return rc;
    std::vector<int> st(4 * (size_t)nf);
    for (int f = 0; f < nf; ++f) {
        st[4 * f] = runs[f] ? ST_DONE : ST_ITER; st[4 * f + 1] = 0; st[4 * f + 2] = nmo[f]; st[4 * f + 3] = runs[f] ? 1 : 0;
    }
    HIP_CHECK_RET(hipMemcpyAsync(bv.istate, st.data(), sizeof(int) * st.size(), hipMemcpyHostToDevice, s));
    HIP_CHECK_RET(hipMemcpyAsync(bv.df_b, B, sizeof(double) * (size_t)nf * n_aux * plan.npair, hipMemcpyHostToDevice, s));
    HIP_CHECK_RET(hipMemcpyAsync(bv.C, C, sizeof(double) * nf * nn, hipMemcpyHostToDevice, s));
    HIP_CHECK_RET(hipMemcpyAsync(bv.eps, eps, sizeof(double) * (size_t)nf * n_ao, hipMemcpyHostToDevice, s));
    Mp2Pool p;
    if (!rimp2_carve(bv, n_frozen, p, why)) return fail(MQC_HIP_ERR_DEVICE, why);
    if (p.u_bia != sizeof(double) * c_bia || p.u_part != sizeof(double) * c_part)
        return fail(MQC_HIP_ERR_DEVICE, "rimp2 stage: the stage's arrays are not the size the entry expects");
    // Poison: the pool is static and reused across calls, so without it an element the pair kernel reads from the padding
    // of Bia, or the reduction from a pair nobody wrote, would be whatever the last call left.  What the poison cannot
    // show is a write OUTSIDE the three arrays: the roundings behind each are compared across the launch.
    const size_t total = p.b_bia + p.b_part + p.b_out;
    HIP_CHECK_RET(hipMemsetAsync(p.base, 0xFF, total, s));
    const size_t g0 = p.b_bia - p.u_bia, g1 = p.b_part - p.u_part, g2 = p.b_out - p.u_out;
    std::vector<double> h_out(2 * (size_t)nf, nan);
    if (!rimp2_enqueue(bv, n_frozen, r, p, h_out.data(), s, why)) return fail(MQC_HIP_ERR_DEVICE, why);
    std::vector<unsigned char> gaps(g0 + g1 + g2 + 1, 0);
    if (g0) HIP_CHECK_RET(hipMemcpyAsync(gaps.data(), p.base + p.u_bia, g0, hipMemcpyDeviceToHost, s));
    if (g1) HIP_CHECK_RET(hipMemcpyAsync(gaps.data() + g0, p.base + p.b_bia + p.u_part, g1, hipMemcpyDeviceToHost, s));
    if (g2) HIP_CHECK_RET(hipMemcpyAsync(gaps.data() + g0 + g1, p.base + p.b_bia + p.b_part + p.u_out, g2, hipMemcpyDeviceToHost, s));
    HIP_CHECK_RET(hipMemcpyAsync(part, p.base + p.b_bia, p.u_part, hipMemcpyDeviceToHost, s));
    if (Bia) HIP_CHECK_RET(hipMemcpyAsync(Bia, p.base, p.u_bia, hipMemcpyDeviceToHost, s));
    HIP_CHECK_RET(hipStreamSynchronize(s));
    if ((rc = stage_check("RI-MP2")) != MQC_HIP_OK) return rc;
    for (size_t k = 0; k < g0 + g1 + g2; ++k)
        if (gaps[k] != 0xFF) return fail(MQC_HIP_ERR_DEVICE, "rimp2 stage: the stage wrote outside Bia, the pair partials and the results");
    std::memcpy(e, h_out.data(), sizeof(double) * h_out.size());
    return MQC_HIP_OK;
}

// the plan of an in-core SCF batch of ntot fragments of n functions: plan_layout picks the square or the triangle
static BatchPlan jk_incore_plan(int n, int ntot, bool uhf)
{
    BatchPlan plan;
    plan.n = n; plan.npair = n * (n + 1) / 2; plan.natoms = 1;
    plan.uhf = uhf;
    plan.nalpha = plan.nbeta = plan.nocc = 1;
    plan.two_e = TWO_E_INCORE;
    plan_layout(plan, ntot, 1, 0, false);
    return plan;
}

int mqc_hip_jk_tensor_layout(int32_t n_ao, int64_t nfrag, int32_t unrestricted, int32_t* triangular, int64_t* block_doubles,
                             int64_t* stride_doubles)
{
    if (!triangular || !block_doubles || !stride_doubles) return fail(MQC_HIP_ERR_VALIDATION, "jk tensor layout: null argument");
    if (n_ao < 1 || n_ao > 256 || nfrag < 1) return fail(MQC_HIP_ERR_VALIDATION, "jk tensor layout: n_ao must be within 1..256 and n_fragments at least 1");
    const BatchPlan plan = jk_incore_plan(n_ao, (int)std::min<int64_t>(nfrag, 1 << 30), unrestricted != 0);
    BatchView probe{};
    carve_chunk(plan, 1, nullptr, probe);
    *triangular = probe.eri_tri;
    *block_doubles = probe.eri_tri_pb;
    *stride_doubles = (int64_t)probe.eri_stride;
    return MQC_HIP_OK;
}

// The in-core J/K stage of an SCF iteration on given tensors (include/mqc_hip.h).  No molecule: the kernels read n, npair,
// the tensor with its layout, D, istate and -- the triangle under screening -- three fields of the topology (nshell,
// sh_aoff, sh_l), the bounds and their threshold.  The arrays are the ones carve_slot gives an in-core batch of this
// shape (the layout is plan_layout's choice, the block table carve_slot's upload), and launch_jk_incore runs once over
// all fragments, as jk_one runs it.  The launchers zero K, and for the triangle with several workgroups per fragment
// J too, with one memset over the WHOLE batch: an element of a finished fragment (done[f] != 0) comes back as the
// poison or as zero, never as anything else.
int mqc_hip_jk_incore_batch(mqc_hip_context* ctx, int64_t nfrag, int32_t n_ao, int32_t unrestricted, const double* tensor, int64_t stride,
                            const double* D, const int32_t* done, int32_t n_shells, const int32_t* shell_l, const double* Q, double q_thresh,
                            double* J, double* K, int32_t* loaded, char* route, int32_t route_len, int32_t* grid_x)
{
    if (!ctx || !tensor || !D || !J || !K || !loaded || !route || route_len < 1 || !grid_x) return fail(MQC_HIP_ERR_VALIDATION, "jk incore batch: null argument");
    if (nfrag < 1 || nfrag > (1 << 20)) return fail(MQC_HIP_ERR_VALIDATION, "jk incore batch: n_fragments must be within 1..2^20");
    if (n_ao < 1 || !incore_supported(n_ao)) return fail(MQC_HIP_ERR_VALIDATION, "jk incore batch: n_ao must be within 1..116 (the in-core limit)");
    const bool screen = n_shells != 0;
    std::vector<int> sh_l, sh_aoff;
    if (screen) {
        if (n_shells < 0 || !shell_l || !Q) return fail(MQC_HIP_ERR_VALIDATION, "jk incore batch: screening needs shell_l and Q");
        if (n_ao > 64) return fail(MQC_HIP_ERR_VALIDATION, "jk incore batch: screening is for n_ao <= 64 (the triangular kernel)");
        if (!std::isfinite(q_thresh)) return fail(MQC_HIP_ERR_VALIDATION, "jk incore batch: q_thresh must be finite");
        int64_t fun = 0;
        for (int k = 0; k < n_shells; ++k) {
            if (shell_l[k] < 0 || shell_l[k] > 32) return fail(MQC_HIP_ERR_VALIDATION, "jk incore batch: shell_l out of range");
            sh_l.push_back(shell_l[k]); sh_aoff.push_back((int)fun);
            fun += 2 * shell_l[k] + 1;
            if (fun > n_ao) break;
        }
        if (fun != n_ao) return fail(MQC_HIP_ERR_VALIDATION, "jk incore batch: shell_l does not add up to n_ao functions");
    }
    const int nf = (int)nfrag, n = n_ao;
    const BatchPlan plan = jk_incore_plan(n, nf, unrestricted != 0);
    {
        BatchView probe{};
        carve_chunk(plan, 1, nullptr, probe);
        if (stride < 0 || (size_t)stride != probe.eri_stride)
            return fail(MQC_HIP_ERR_VALIDATION, "jk incore batch: stride " + std::to_string(stride) + " is not the layout's (" +
                                                    std::to_string(probe.eri_stride) + " doubles per fragment, mqc_hip_jk_tensor_layout)");
    }
    HIP_CHECK_RET(hipSetDevice(ctx->device));
    route[0] = 0; *grid_x = 0;
    const size_t nn = (size_t)n * n;
    constexpr size_t GUARD = 1024;         // bytes compared in front of J and behind K (S .. C in front, W behind: never less)
    const Slot sl0 = make_slot(ctx, 0, nullptr);
    hipStream_t s = ctx->lane[0].stream;
    int rc;
    // one chunk: the dispatch depends on the number of fragments of the launch.  A batch beyond the memory is refused.
    BatchView bv{};
    bv.nalpha = bv.nbeta = bv.nocc = 1; bv.exx = 1.0;
    TopologyDev td{};
    const double* jk_q = nullptr;
    if (screen) {
        // the three fields of the topology jk_tri_kernel reads, and the bounds behind them
        auto up = [](size_t b) { return (b + 255) & ~size_t(255); };
        const size_t ib = up(sizeof(int) * (size_t)n_shells), qb = sizeof(double) * (size_t)nf * n_shells * n_shells;
        char* base = (char*)ctx->lane[0].topo.ensure(2 * ib + up(qb));
        if (!base) return fail(MQC_HIP_ERR_DEVICE, "out of device memory (screening tables)");
        td.sh_l = (int*)base; td.sh_aoff = (int*)(base + ib);
        td.nshell = n_shells; td.nao = n; td.npair = plan.npair; td.natoms = 1;
        HIP_CHECK_RET(hipMemcpyAsync(td.sh_l, sh_l.data(), sizeof(int) * (size_t)n_shells, hipMemcpyHostToDevice, s));
        HIP_CHECK_RET(hipMemcpyAsync(td.sh_aoff, sh_aoff.data(), sizeof(int) * (size_t)n_shells, hipMemcpyHostToDevice, s));
        HIP_CHECK_RET(hipMemcpyAsync(base + 2 * ib, Q, qb, hipMemcpyHostToDevice, s));
        HIP_CHECK_RET(hipStreamSynchronize(s));    // the caller's Q and the host tables are done with
        jk_q = (const double*)(base + 2 * ib);
    }
    if ((rc = carve_slot(ctx, sl0, plan, td, nf, bv)) != MQC_HIP_OK) return rc;
    bv.jk_q = jk_q; bv.jk_qthresh = q_thresh;
    const size_t jk_bytes = sizeof(double) * (size_t)nf * nn;
    unsigned char* lo = (unsigned char*)bv.J - GUARD;
    unsigned char* mid = (unsigned char*)bv.J + jk_bytes;            // the padding between J and K (under 256 bytes)
    unsigned char* hi = (unsigned char*)bv.K + jk_bytes;
    const size_t pad = (size_t)((unsigned char*)bv.K - mid);
    if (lo < (unsigned char*)bv.xyz || pad > 256 || hi + GUARD > (unsigned char*)bv.diis_state)
        return fail(MQC_HIP_ERR_DEVICE, "jk incore batch: J and K are not where the guard band expects them");
    // Poison first (the band behind K reaches into the work matrices, nothing the launch reads), then the inputs
    HIP_CHECK_RET(hipMemsetAsync(bv.J, 0xFF, jk_bytes, s));
    HIP_CHECK_RET(hipMemsetAsync(bv.K, 0xFF, jk_bytes, s));
    if (pad) HIP_CHECK_RET(hipMemsetAsync(mid, 0xFF, pad, s));
    HIP_CHECK_RET(hipMemsetAsync(hi, 0xFF, GUARD, s));
    if (bv.jk_loaded) HIP_CHECK_RET(hipMemsetAsync(bv.jk_loaded, 0xFF, sizeof(int) * (size_t)nf, s));
    std::vector<int> ist((size_t)nf * 4, 0);
    for (int f = 0; f < nf && done; ++f)
        if (done[f]) ist[4 * (size_t)f] = ST_DONE;
    HIP_CHECK_RET(hipMemcpyAsync(bv.istate, ist.data(), sizeof(int) * ist.size(), hipMemcpyHostToDevice, s));
    HIP_CHECK_RET(hipMemcpyAsync(bv.eri, tensor, sizeof(double) * (size_t)nf * bv.eri_stride, hipMemcpyHostToDevice, s));
    HIP_CHECK_RET(hipMemcpyAsync(bv.D, D, jk_bytes, hipMemcpyHostToDevice, s));
    std::vector<unsigned char> before(2 * GUARD + 256), after(2 * GUARD + 256);
    HIP_CHECK_RET(hipMemcpyAsync(before.data(), lo, GUARD, hipMemcpyDeviceToHost, s));
    HIP_CHECK_RET(hipMemcpyAsync(before.data() + GUARD, hi, GUARD, hipMemcpyDeviceToHost, s));
    if (pad) HIP_CHECK_RET(hipMemcpyAsync(before.data() + 2 * GUARD, mid, pad, hipMemcpyDeviceToHost, s));
    const JkRoute r = launch_jk_incore(bv, done != nullptr, s);
    HIP_CHECK_RET(hipMemcpyAsync(after.data(), lo, GUARD, hipMemcpyDeviceToHost, s));
    HIP_CHECK_RET(hipMemcpyAsync(after.data() + GUARD, hi, GUARD, hipMemcpyDeviceToHost, s));
    if (pad) HIP_CHECK_RET(hipMemcpyAsync(after.data() + 2 * GUARD, mid, pad, hipMemcpyDeviceToHost, s));
    HIP_CHECK_RET(hipMemcpyAsync(J, bv.J, jk_bytes, hipMemcpyDeviceToHost, s));
    HIP_CHECK_RET(hipMemcpyAsync(K, bv.K, jk_bytes, hipMemcpyDeviceToHost, s));
    if (bv.jk_loaded) HIP_CHECK_RET(hipMemcpyAsync(loaded, bv.jk_loaded, sizeof(int) * (size_t)nf, hipMemcpyDeviceToHost, s));
    HIP_CHECK_RET(hipStreamSynchronize(s));
    if ((rc = stage_check("in-core J/K")) != MQC_HIP_OK) return rc;
    if (!bv.jk_loaded) std::fill(loaded, loaded + nf, -1);
    if (std::memcmp(before.data(), after.data(), 2 * GUARD + pad) != 0)
        return fail(MQC_HIP_ERR_DEVICE, "jk incore batch: the stage wrote outside J and K");
    if (r.family == JK_TRI) std::snprintf(route, (size_t)route_len, "tri<%d,%d>", r.nw, r.maxu);
    else if (r.family == JK_ROWCOOP) std::snprintf(route, (size_t)route_len, "rowcoop<%d,%d>", r.kch, r.maxu);
    else std::snprintf(route, (size_t)route_len, "wave<%d,%s,%d,%d,%s%s>", r.kch, r.klds ? "lds" : "global", r.nw, r.maxu, r.dreg ? "reg" : "mem",
                       r.full8 ? ",full8" : "");
    *grid_x = r.grid_x;
    return MQC_HIP_OK;
}

// The multi-density J/K stage of a CPHF iteration on given square tensors (include/mqc_hip.h).  The tensor and the state
// words are the ones carve_slot gives an in-core batch planned with the square layout, as the polarizability entry plans
// its batches; D, J and K sit direction-major [3][nfrag][n * n] in a pool of this entry, J and K between two guard
// bands, and launch_jk_multi (or, MQC_HIP_CPHF_MULTI=0, launch_jk_incore once per density) runs once over all fragments.
// Both launchers zero K with one memset over the whole batch, so an element of a finished fragment comes back as the
// poison (J) or as zero (K).
int mqc_hip_jk_multi_batch(mqc_hip_context* ctx, int64_t nfrag, int32_t n_ao, int32_t n_densities, const double* tensor, const double* D,
                           const int32_t* done, double* J, double* K, char* route, int32_t route_len)
{
    static DevicePool pool;
    if (!ctx || !tensor || !D || !J || !K || !route || route_len < 1) return fail(MQC_HIP_ERR_VALIDATION, "jk multi batch: null argument");
    if (nfrag < 1 || nfrag > (1 << 20)) return fail(MQC_HIP_ERR_VALIDATION, "jk multi batch: n_fragments must be within 1..2^20");
    if (n_ao < 1 || n_ao > 116 || !incore_supported(n_ao)) return fail(MQC_HIP_ERR_VALIDATION, "jk multi batch: n_ao must be within 1..116 (the in-core limit)");
    if (n_densities < 1 || n_densities > 3) return fail(MQC_HIP_ERR_VALIDATION, "jk multi batch: n_densities must be within 1..3");
    const int nf = (int)nfrag, n = n_ao, nd = n_densities;
    BatchPlan plan;
    plan.n = n; plan.npair = n * (n + 1) / 2; plan.natoms = 1;
    plan.nalpha = plan.nbeta = plan.nocc = 1;
    plan.two_e = TWO_E_INCORE;
    plan.square_only = true;
    plan_layout(plan, nf, 1, 0, false);
    HIP_CHECK_RET(hipSetDevice(ctx->device));
    route[0] = 0;
    const size_t nn = (size_t)n * n, np = (size_t)plan.npair;
    constexpr size_t GUARD = 1024;
    hipStream_t s = ctx->lane[0].stream;
    int rc;
    BatchView bv{};
    bv.nalpha = bv.nbeta = bv.nocc = 1; bv.exx = 1.0;
    TopologyDev td{};
    if ((rc = carve_slot(ctx, make_slot(ctx, 0, nullptr), plan, td, nf, bv)) != MQC_HIP_OK) return rc;
    const size_t mat = sizeof(double) * 3 * (size_t)nf * nn;         // three slots, whatever n_densities is
    unsigned char* base = (unsigned char*)pool.ensure(3 * mat + 2 * GUARD);
    if (!base) return fail(MQC_HIP_ERR_DEVICE, "out of device memory (jk multi batch)");
    unsigned char* lo = base;
    double* dJ = (double*)(base + GUARD);
    double* dK = (double*)(base + GUARD + mat);
    unsigned char* hi = base + GUARD + 2 * mat;
    double* dD = (double*)(hi + GUARD);
    // poison the outputs and their neighbours, then the inputs: fragment f's density d from [f][d] to [d][f]
    HIP_CHECK_RET(hipMemsetAsync(lo, 0xFF, 2 * GUARD + 2 * mat, s));
    std::vector<int> ist((size_t)nf * 4, 0);
    for (int f = 0; f < nf && done; ++f)
        if (done[f]) ist[4 * (size_t)f] = ST_DONE;
    HIP_CHECK_RET(hipMemcpyAsync(bv.istate, ist.data(), sizeof(int) * ist.size(), hipMemcpyHostToDevice, s));
    HIP_CHECK_RET(hipMemcpyAsync(bv.eri, tensor, sizeof(double) * (size_t)nf * np * np, hipMemcpyHostToDevice, s));
    const size_t row = sizeof(double) * nn;
    for (int d = 0; d < nd; ++d)
        HIP_CHECK_RET(hipMemcpy2DAsync(dD + (size_t)d * nf * nn, row, D + (size_t)d * nn, row * nd, row, (size_t)nf, hipMemcpyHostToDevice, s));
    std::vector<unsigned char> before(2 * GUARD), after(2 * GUARD);
    HIP_CHECK_RET(hipMemcpyAsync(before.data(), lo, GUARD, hipMemcpyDeviceToHost, s));
    HIP_CHECK_RET(hipMemcpyAsync(before.data() + GUARD, hi, GUARD, hipMemcpyDeviceToHost, s));
    std::string name;
    if (cphf_multi_on()) {
        JkMultiRoute r{};
        std::string err;
        if (!launch_jk_multi(bv, nd, dD, dJ, dK, done != nullptr, s, &r, err)) return fail(MQC_HIP_ERR_DEVICE, "jk multi batch: " + err);
        name = jk_multi_route_name(r);
    } else {
        JkRoute r{};
        for (int d = 0; d < nd; ++d) {
            BatchView v1 = bv;
            v1.D = dD + (size_t)d * nf * nn; v1.J = dJ + (size_t)d * nf * nn; v1.K = dK + (size_t)d * nf * nn;
            v1.jk_loaded = nullptr;
            r = launch_jk_incore(v1, done != nullptr, s);
        }
        char buf[64];
        std::snprintf(buf, sizeof(buf), "single:wave<%d,%s,%d,%d,%s%s>", r.kch, r.klds ? "lds" : "global", r.nw, r.maxu, r.dreg ? "reg" : "mem",
                      r.full8 ? ",full8" : "");
        name = r.family == JK_ROWCOOP ? "single:rowcoop" : buf;
    }
    HIP_CHECK_RET(hipMemcpyAsync(after.data(), lo, GUARD, hipMemcpyDeviceToHost, s));
    HIP_CHECK_RET(hipMemcpyAsync(after.data() + GUARD, hi, GUARD, hipMemcpyDeviceToHost, s));
    for (int d = 0; d < nd; ++d) {
        HIP_CHECK_RET(hipMemcpy2DAsync(J + (size_t)d * nn, row * nd, dJ + (size_t)d * nf * nn, row, row, (size_t)nf, hipMemcpyDeviceToHost, s));
        HIP_CHECK_RET(hipMemcpy2DAsync(K + (size_t)d * nn, row * nd, dK + (size_t)d * nf * nn, row, row, (size_t)nf, hipMemcpyDeviceToHost, s));
    }
    HIP_CHECK_RET(hipStreamSynchronize(s));
    if ((rc = stage_check("multi-density J/K")) != MQC_HIP_OK) return rc;
    if (std::memcmp(before.data(), after.data(), 2 * GUARD) != 0)
        return fail(MQC_HIP_ERR_DEVICE, "jk multi batch: the stage wrote outside J and K");
    std::snprintf(route, (size_t)route_len, "%s", name.c_str());
    return MQC_HIP_OK;
}

// The build of the fitted tensor alone (include/mqc_hip.h): the plan and the arrays of a density-fitted SCF batch of
// nfrag fragments, launch_df_integrals, the metric copied out, launch_df_fit -- the two halves of launch_df_build.
int mqc_hip_df_fit_batch(mqc_hip_context* ctx, int64_t nfrag, const mqc_hip_molecule_t* mols, const mqc_hip_basis_t* orbital,
                         const mqc_hip_basis_t* aux, double* A3, double* metric, double* B, double* fit_flag)
{
    if (!ctx || !mols || !orbital || !aux || !A3 || !metric || !B || !fit_flag) return fail(MQC_HIP_ERR_VALIDATION, "df fit batch: null argument");
    if (nfrag < 1) return fail(MQC_HIP_ERR_VALIDATION, "df fit batch: n_fragments must be at least 1");
    HIP_CHECK_RET(hipSetDevice(ctx->device));
    if (mols[0].n_atoms <= 0 || !same_elements(mols, nfrag))
        return fail(MQC_HIP_ERR_VALIDATION, "df fit batch: every fragment must have the elements of the first (one topology per call)");
    mqc_hip_scf_options_t opts;
    mqc_hip_default_options(&opts);
    opts.density_fitting = 1;
    Topology topo, xtopo;
    std::string msg;
    int rc = build_topology(mols[0], *orbital, topo, msg, KERNEL_LMAX, false);
    if (rc != MQC_HIP_OK) return fail(rc, msg);
    if ((rc = build_topology(mols[0], *aux, xtopo, msg, AUX_LMAX, false)) != MQC_HIP_OK) return fail(rc, "auxiliary basis: " + msg);
    const int ntot = (int)std::min<int64_t>(nfrag, 1 << 30);
    BatchPlan plan;
    if ((rc = plan_batch(opts, topo, ntot, plan, msg)) != MQC_HIP_OK) return fail(rc, msg);
    plan.naux = xtopo.nao;
    plan_layout(plan, ntot, (int)topo.shells.size(), topo.lmax, false);
    TopologyDev td{}, tdx{};
    if ((rc = upload_topology(ctx, topo, td)) != MQC_HIP_OK) return rc;
    if ((rc = upload_topology(ctx, xtopo, tdx, &ctx->lane[0].aux)) != MQC_HIP_OK) return rc;
    const size_t na = (size_t)xtopo.nao, a3 = na * (size_t)topo.npair, mm = na * na;
    size_t free_b = 0, total_b = 0;
    (void)hipMemGetInfo(&free_b, &total_b);
    free_b += ctx->lane[0].pool[POOL_MAIN].capacity() + ctx->lane[0].pool[POOL_DF].capacity();
    const int64_t chunk = stage_chunk_fragments(free_b, fragment_bytes(plan), nfrag);
    const Slot sl0 = make_slot(ctx, 0, nullptr);
    hipStream_t s = ctx->lane[0].stream;
    std::vector<double> hx, scal;
    for (int64_t start = 0; start < nfrag; start += chunk) {
        const int nf = (int)std::min<int64_t>(chunk, nfrag - start);
        BatchView bv{};
        bv.nalpha = plan.nalpha; bv.nbeta = plan.nbeta; bv.nocc = plan.nocc; bv.aux = tdx; bv.exx = 1.0;
        if ((rc = carve_slot(ctx, sl0, plan, td, nf, bv)) != MQC_HIP_OK) return rc;
        HIP_CHECK_RET(hipMemsetAsync(bv.scal, 0, sizeof(double) * (size_t)nf * 8, s));          // as prepare() does
        gather_xyz(mols + start, nf, topo.natoms, hx);
        HIP_CHECK_RET(hipMemcpyAsync(bv.xyz, hx.data(), sizeof(double) * hx.size(), hipMemcpyHostToDevice, s));
        HIP_CHECK_RET(hipMemsetAsync(bv.istate, 0, sizeof(int) * (size_t)nf * 4, s));
        // poison: an element of (P|mu nu), of the metric or of the fitted tensor that no task covers reads as NaN
        HIP_CHECK_RET(hipMemsetAsync(bv.df_a3, 0xFF, sizeof(double) * a3 * nf, s));
        HIP_CHECK_RET(hipMemsetAsync(bv.df_metric, 0xFF, sizeof(double) * mm * nf, s));
        HIP_CHECK_RET(hipMemsetAsync(bv.df_b, 0xFF, sizeof(double) * a3 * nf, s));
        launch_df_integrals(bv, topo, xtopo, s);
        if ((rc = stage_check("three- and two-centre integrals")) != MQC_HIP_OK) return rc;
        // the factorisation overwrites the metric in place: it is copied out between the two halves
        HIP_CHECK_RET(hipMemcpyAsync(metric + (size_t)start * mm, bv.df_metric, sizeof(double) * mm * nf, hipMemcpyDeviceToHost, s));
        launch_df_fit(bv, s);
        scal.resize((size_t)nf * 8);
        HIP_CHECK_RET(hipMemcpyAsync(A3 + (size_t)start * a3, bv.df_a3, sizeof(double) * a3 * nf, hipMemcpyDeviceToHost, s));
        HIP_CHECK_RET(hipMemcpyAsync(B + (size_t)start * a3, bv.df_b, sizeof(double) * a3 * nf, hipMemcpyDeviceToHost, s));
        HIP_CHECK_RET(hipMemcpyAsync(scal.data(), bv.scal, sizeof(double) * scal.size(), hipMemcpyDeviceToHost, s));
        HIP_CHECK_RET(hipStreamSynchronize(s));
        if ((rc = stage_check("density fit")) != MQC_HIP_OK) return rc;
        for (int f = 0; f < nf; ++f) fit_flag[start + f] = scal[8 * (size_t)f + 7];
    }
    return MQC_HIP_OK;
}

int mqc_hip_syev(mqc_hip_context* ctx, int32_t n, const double* A, double* w, double* V)
{
    if (!ctx || !A || !w || !V || n <= 0) return fail(MQC_HIP_ERR_VALIDATION, "bad arguments");
    if (n > 256) return fail(MQC_HIP_ERR_UNSUPPORTED, "matrix too large for the Jacobi solver (n <= 256)");
    HIP_CHECK_RET(hipSetDevice(ctx->device));
    const size_t nn = (size_t)n * n;
    double* d = (double*)ctx->lane[0].pool[POOL_MAIN].ensure(sizeof(double) * (2 * nn + n) + 1024);
    if (!d) return fail(MQC_HIP_ERR_DEVICE, "out of device memory");
    HIP_CHECK_RET(hipMemcpy(d, A, sizeof(double) * nn, hipMemcpyHostToDevice));
    launch_syev(n, d, d + 2 * nn, d + nn, ctx->lane[0].stream);
    const int rc = sync_and_check(ctx->lane[0].stream);
    if (rc != MQC_HIP_OK) return rc;
    HIP_CHECK_RET(hipMemcpy(w, d + 2 * nn, sizeof(double) * n, hipMemcpyDeviceToHost));
    HIP_CHECK_RET(hipMemcpy(V, d + nn, sizeof(double) * nn, hipMemcpyDeviceToHost));
    return MQC_HIP_OK;
}

int mqc_hip_diis_coefficients(mqc_hip_context* ctx, int32_t n_stored, const double* overlap, double* coefficients, int32_t* ok)
{
    if (!ctx || !overlap || !coefficients || !ok) return fail(MQC_HIP_ERR_VALIDATION, "bad arguments");
    if (n_stored < 1 || n_stored > DIIS_MAX) return fail(MQC_HIP_ERR_VALIDATION, "n_stored must be within 1..8");
    HIP_CHECK_RET(hipSetDevice(ctx->device));
    double* d = (double*)ctx->lane[0].pool[POOL_MISC].ensure(4096);
    if (!d) return fail(MQC_HIP_ERR_DEVICE, "out of device memory");
    HIP_CHECK_RET(hipMemcpy(d + 32, overlap, sizeof(double) * n_stored * n_stored, hipMemcpyHostToDevice));
    launch_diis_coeff(n_stored, d + 32, d + 128, (int*)d, ctx->lane[0].stream);
    HIP_CHECK_RET(hipStreamSynchronize(ctx->lane[0].stream));
    HIP_CHECK_RET(hipMemcpy(coefficients, d + 128, sizeof(double) * n_stored, hipMemcpyDeviceToHost));
    int okv = 0;
    HIP_CHECK_RET(hipMemcpy(&okv, d, sizeof(int), hipMemcpyDeviceToHost));
    *ok = okv;
    return MQC_HIP_OK;
}

}  // extern "C"
