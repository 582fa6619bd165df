// engine.cpp -- context, batch driver and the SCF extern "C" entry points of libmqc_hip.so (the stage-level entry
// points are in stage_entries.cpp; driver.hpp declares what the two share).
//
// Host control flow of one batch (the device-resident SCF loop of
// backends/cuest/backend/mqc_cuest_scf.f90:281-611, re-cut for whole batches):
//   upload geometry -> int1e -> orthogonaliser -> ERI tensor -> guess ->
//   repeat { J/K stream ; scf_step ; read ONE int (fragments still running) } -> fetch results
// Only that one integer crosses the bus per iteration.
#include "driver.hpp"
#include "md_integrals.hpp"
#include <algorithm>
#include <array>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <sstream>
#include <atomic>
#include <thread>

namespace mqc {
const std::string& last_error_string();
void eri_plan_lists(const BatchView& bv, const Topology& topo, hipStream_t s, const double* host_xyz);   // kern_eri.hip
bool launch_gradient(const BatchView& bv, const Topology& topo, const Topology* aux, double* d_grad, double* work, int* d_lists,
                     size_t list_capacity_ints, hipStream_t s, std::string& err, const double* schwarz, double screen_tol);          // kern_grad.hip
const double* direct_schwarz_view(int slot);                                                                                    // kern_eri.hip
void launch_scale(double* p, size_t count, double f, hipStream_t s);      // kern_df.hip
void int1e_reset_state();                                                 // kern_int1e.hip: fan-out streams of small batches
void eri_schwarz_view(int slot, const double** q, double* thresh);        // kern_eri.hip
void launch_jk_direct_incremental(const BatchView& bv, const Topology& topo, double thresh, bool only_active, hipStream_t s);   // kern_eri.hip
static DevicePool g_grad_pool[2];
// kern_grad_pc.hip: the point charges' part of an embedded fragment's gradient (atoms' part added into d_grad, the sites'
// gradient into d_pcgrad [nfrag][npc][3]); doubles of records per fragment
bool launch_pc_gradient(const BatchView& bv, const Topology& topo, const double* Dtot, double* d_grad, double* d_pcgrad, double* d_rec,
                        hipStream_t s, std::string& err);
size_t gradpc_record_doubles(const Topology& topo);
// kern_mp2.hip (launch_rimp2, rimp2_fragment_bytes: engine.hpp, shared with the stage entry)
// kern_cphf.hip: the CPHF solve of a converged in-core chunk with the square tensor -- alpha [nfrag][9], iterations and
// CPHF_* status per fragment, complete on return (h_counter: the slot's pinned word); device bytes per fragment
bool launch_cphf(const BatchView& bv, const Topology& topo, double tol, int max_iter, double* h_alpha, int* h_iter, int* h_status,
                 int* h_counter, hipStream_t s, std::string& err);
size_t cphf_fragment_bytes(int n, int nocc, int nmo);

int stage_check(const char* stage)
{
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(MQC_HIP_ERR_DEVICE, std::string("HIP error after stage '") + stage + "': " + hipGetErrorString(e));
    return MQC_HIP_OK;
}

static double now_s()
{
    using namespace std::chrono;
    return duration<double>(steady_clock::now().time_since_epoch()).count();
}

// Scratch (private segment).  The first time a kernel with a private segment runs on a hardware queue, ROCm reserves
// that kernel's bytes per lane x 64 lanes x every wave slot of the device (CUs x 32) FOR THAT QUEUE, and aborts the
// process (HSA_STATUS_ERROR_OUT_OF_RESOURCES, recorded in rounds 1 and 2) when the memory is not there.  No kernel the
// dispatchers launch carries more than SCRATCH_BOUND_PER_LANE (scripts/scratch_report.py lists them from the code
// objects; tests/test_host_logic.py asserts the bound on every build; the classes above it -- (dd|dp), (dd|dd), the (dd|
// Schwarz bounds -- go through the LDS kernel, which has none), so the worst case is the bound on every hardware queue
// the process may use, and the pools' HBM budget leaves that much alone.
constexpr size_t SCRATCH_BOUND_PER_LANE = 8192;
static size_t scratch_reservation_bytes(const mqc_hip_context* ctx)
{
    int queues = 4;                                         // the runtime's default
    if (const char* e = std::getenv("GPU_MAX_HW_QUEUES")) queues = std::max(1, std::atoi(e));
    const size_t waves = (size_t)std::max(1, ctx->prop.multiProcessorCount) * 32;
    return (size_t)queues * SCRATCH_BOUND_PER_LANE * 64 * waves;
}

int upload_topology(mqc_hip_context* ctx, const Topology& topo, TopologyDev& td, DevicePool* pool, hipStream_t stream)
{
    if (!pool) pool = &ctx->lane[0].topo;
    const int ns = (int)topo.shells.size();
    std::vector<int> l(ns), np(ns), po(ns), at(ns), ao(ns);
    for (int s = 0; s < ns; ++s) {
        l[s] = topo.shells[s].l; np[s] = topo.shells[s].nprim; po[s] = topo.shells[s].poff;
        at[s] = topo.shells[s].atom; ao[s] = topo.shells[s].aoff;
    }
    const size_t ib = sizeof(int) * (size_t)ns;
    const size_t nprim = topo.exps.size();
    // radial groups (see TopologyDev)
    std::vector<int> gfirst, gcount, gnprim, gpoff, gcoff;
    std::vector<double> gex, gco;
    for (int sidx = 0; sidx < ns; ++sidx) {
        const auto& sh = topo.shells[sidx];
        bool joined = false;
        if (!gfirst.empty()) {
            const int g = (int)gfirst.size() - 1;
            const auto& lead = topo.shells[gfirst[g]];
            if (gfirst[g] + gcount[g] == sidx && gcount[g] < XC_GROUP_MAX && lead.atom == sh.atom && lead.l == sh.l) {
                std::vector<int> where(sh.nprim, -1);
                bool all = true;
                for (int i = 0; i < sh.nprim && all; ++i) {
                    for (int k = 0; k < lead.nprim; ++k)
                        if (topo.exps[lead.poff + k] == topo.exps[sh.poff + i]) { where[i] = k; break; }
                    all = where[i] >= 0;
                }
                if (all) {
                    gco.resize(gco.size() + lead.nprim, 0.0);
                    double* row = gco.data() + gcoff[g] + (size_t)gcount[g] * lead.nprim;
                    for (int i = 0; i < sh.nprim; ++i) row[where[i]] += topo.coefs[sh.poff + i];
                    gcount[g] += 1;
                    joined = true;
                }
            }
        }
        if (!joined) {
            gfirst.push_back(sidx); gcount.push_back(1); gnprim.push_back(sh.nprim);
            gpoff.push_back((int)gex.size()); gcoff.push_back((int)gco.size());
            for (int i = 0; i < sh.nprim; ++i) { gex.push_back(topo.exps[sh.poff + i]); gco.push_back(topo.coefs[sh.poff + i]); }
        }
    }
    const int ng = (int)gfirst.size();
    {
        // deepest groups first: the lanes of a wave take consecutive groups (16 points each), so groups of equal
        // primitive count side by side keep the primitive loop's trip count uniform inside a wave
        std::vector<int> order(ng);
        for (int g = 0; g < ng; ++g) order[g] = g;
        std::stable_sort(order.begin(), order.end(), [&](int a, int b) {
            if (gnprim[a] != gnprim[b]) return gnprim[a] > gnprim[b];
            return gcount[a] > gcount[b];
        });
        auto permute = [&](std::vector<int>& v) { std::vector<int> t(ng); for (int g = 0; g < ng; ++g) t[g] = v[order[g]]; v.swap(t); };
        permute(gfirst); permute(gcount); permute(gnprim); permute(gpoff); permute(gcoff);
    }
    const size_t gib = sizeof(int) * (size_t)ng;
    const size_t bytes = 5 * ((ib + 255) & ~size_t(255)) + 3 * ((sizeof(double) * (nprim + topo.natoms) + 255) & ~size_t(255)) + 1024
                       + 5 * ((gib + 255) & ~size_t(255)) + ((sizeof(double) * gex.size() + 255) & ~size_t(255))
                       + ((sizeof(double) * gco.size() + 255) & ~size_t(255));
    char* base = (char*)pool->ensure(bytes);
    if (!base) return fail(MQC_HIP_ERR_DEVICE, "out of device memory (topology)");
    auto take = [&base](size_t b) { char* p = base; base += (b + 255) & ~size_t(255); return p; };
    td.sh_l = (int*)take(ib); td.sh_nprim = (int*)take(ib); td.sh_poff = (int*)take(ib);
    td.sh_atom = (int*)take(ib); td.sh_aoff = (int*)take(ib);
    td.exps = (double*)take(sizeof(double) * nprim); td.coefs = (double*)take(sizeof(double) * nprim);
    td.zeff = (double*)take(sizeof(double) * topo.natoms);
    td.grp_first = (int*)take(gib); td.grp_count = (int*)take(gib); td.grp_nprim = (int*)take(gib);
    td.grp_poff = (int*)take(gib); td.grp_coff = (int*)take(gib);
    td.gexps = (double*)take(sizeof(double) * gex.size()); td.gcoefs = (double*)take(sizeof(double) * gco.size());
    td.ngroup = ng;
    td.gprim_total = (int)gex.size(); td.gcoef_total = (int)gco.size();
    td.nshell = ns; td.nao = topo.nao; td.npair = topo.npair; td.natoms = topo.natoms; td.lmax = topo.lmax;
    hipStream_t s = stream ? stream : ctx->lane[0].stream;
    HIP_CHECK_RET(hipMemcpyAsync(td.sh_l, l.data(), ib, hipMemcpyHostToDevice, s));
    HIP_CHECK_RET(hipMemcpyAsync(td.sh_nprim, np.data(), ib, hipMemcpyHostToDevice, s));
    HIP_CHECK_RET(hipMemcpyAsync(td.sh_poff, po.data(), ib, hipMemcpyHostToDevice, s));
    HIP_CHECK_RET(hipMemcpyAsync(td.sh_atom, at.data(), ib, hipMemcpyHostToDevice, s));
    HIP_CHECK_RET(hipMemcpyAsync(td.sh_aoff, ao.data(), ib, hipMemcpyHostToDevice, s));
    HIP_CHECK_RET(hipMemcpyAsync(td.exps, topo.exps.data(), sizeof(double) * nprim, hipMemcpyHostToDevice, s));
    HIP_CHECK_RET(hipMemcpyAsync(td.coefs, topo.coefs.data(), sizeof(double) * nprim, hipMemcpyHostToDevice, s));
    HIP_CHECK_RET(hipMemcpyAsync(td.zeff, topo.zeff.data(), sizeof(double) * topo.natoms, hipMemcpyHostToDevice, s));
    HIP_CHECK_RET(hipMemcpyAsync(td.grp_first, gfirst.data(), gib, hipMemcpyHostToDevice, s));
    HIP_CHECK_RET(hipMemcpyAsync(td.grp_count, gcount.data(), gib, hipMemcpyHostToDevice, s));
    HIP_CHECK_RET(hipMemcpyAsync(td.grp_nprim, gnprim.data(), gib, hipMemcpyHostToDevice, s));
    HIP_CHECK_RET(hipMemcpyAsync(td.grp_poff, gpoff.data(), gib, hipMemcpyHostToDevice, s));
    HIP_CHECK_RET(hipMemcpyAsync(td.grp_coff, gcoff.data(), gib, hipMemcpyHostToDevice, s));
    HIP_CHECK_RET(hipMemcpyAsync(td.gexps, gex.data(), sizeof(double) * gex.size(), hipMemcpyHostToDevice, s));
    HIP_CHECK_RET(hipMemcpyAsync(td.gcoefs, gco.data(), sizeof(double) * gco.size(), hipMemcpyHostToDevice, s));
    HIP_CHECK_RET(hipStreamSynchronize(s));   // the host vectors go out of scope
    return MQC_HIP_OK;
}

int carve_slot(mqc_hip_context* ctx, const Slot& sl, const BatchPlan& plan, const TopologyDev& td, int nfrag, BatchView& bv, PcmView* pcm)
{
    static const char* const what[NPOOL] = {"SCF matrices", "ERI tensor", "counters", "grid weights", "fitted tensor", "PCM arrays"};
    BatchView probe{};
    const ChunkBytes need = carve_chunk(plan, nfrag, nullptr, probe);
    char* bases[NPOOL] = {};
    for (int k = 0; k < NPOOL; ++k)
        if (need.pool[k] && !(bases[k] = (char*)sl.lane->pool[k].ensure(need.pool[k])))
            return fail(MQC_HIP_ERR_DEVICE, std::string("out of device memory (") + what[k] + ")");
    carve_chunk(plan, nfrag, bases, bv, nullptr, pcm);
    bv.topo = td; bv.slot = sl.id; bv.boys = ctx->d_boys; bv.c2s = ctx->d_c2s; bv.unit = ctx->d_unit;
    if (bv.eri_tri) {
        static std::vector<int> sb_host[2];      // stays alive while the copy is in flight
        std::vector<int>& sbh = sb_host[sl.id & 1];
        jk_tri_block(plan.npair, &sbh);
        if (hipMemcpyAsync((void*)bv.eri_tri_sb, sbh.data(), sizeof(int) * sbh.size(), hipMemcpyHostToDevice, sl.lane->stream) != hipSuccess)
            return fail(MQC_HIP_ERR_DEVICE, "upload of the tensor block table failed");
    }
    return MQC_HIP_OK;
}

bool incore_supported(int n)
{
    // the J/K kernel stages whole packed rows through LDS: 3 row-sized buffers must fit 160 KB
    const size_t np = (size_t)n * (n + 1) / 2;
    return n <= 256 && (sizeof(double) * 3 * np <= 160 * 1024 - 512);
}

static int validate_options(const mqc_hip_scf_options_t& o, const Topology& topo, const BatchPlan& p, std::string& msg)
{
    if (p.xc.gga == 2 && topo.nao > 140) { msg = "meta-GGA functionals are available up to n_ao = 140"; return MQC_HIP_ERR_UNSUPPORTED; }
    if (p.xc.ncomp > 0 && topo.natoms > 64) { msg = "XC grid: fragments above 64 atoms are not supported yet"; return MQC_HIP_ERR_UNSUPPORTED; }
    if (p.rsh) {
        // range-separated hybrids need K_lr from a second in-core tensor of erf(omega r12)/r12: nothing else forms it
        std::string fn(o.functional);
        std::transform(fn.begin(), fn.end(), fn.begin(), [](unsigned char c) { return (char)std::tolower(c); });
        const std::string rs = "range-separated functionals (" + fn + ")";
        if (o.density_fitting) { msg = rs + " need exact long-range exchange K_lr: density fitting with erf-attenuated fits is not built; use exact in-core ERIs"; return MQC_HIP_ERR_UNSUPPORTED; }
        if (o.eri_mode == MQC_HIP_ERI_DIRECT) { msg = rs + " run on the in-core exact-ERI path only: the direct path forms no long-range exchange K_lr"; return MQC_HIP_ERR_UNSUPPORTED; }
        if (!incore_supported(topo.nao) || topo.nao > 116) { msg = rs + " run on the in-core exact-ERI path only (n_ao <= 116); larger fragments would need a direct K_lr, which is not built"; return MQC_HIP_ERR_UNSUPPORTED; }
        if (o.want_gradient) { msg = "analytic gradients of " + rs + " are not built (energies only)"; return MQC_HIP_ERR_UNSUPPORTED; }
    }
    if (o.want_gradient) {
        if (p.xc.gga == 2) { msg = "analytic gradients of meta-GGA functionals are not built (energies only)"; return MQC_HIP_ERR_UNSUPPORTED; }
        if (topo.lmax > 3) { msg = "analytic gradients cover s, p, d and f shells"; return MQC_HIP_ERR_UNSUPPORTED; }
    }
    if (p.uhf) {
        // the occupation checks of run_libcint_uhf (mqc_libcint_rhf.f90:768-793)
        if (topo.multiplicity < 1) { msg = "UHF: multiplicity must be at least 1"; return MQC_HIP_ERR_VALIDATION; }
        if ((topo.nelec + topo.multiplicity - 1) % 2 != 0) { msg = "UHF: an electron count and multiplicity that cannot be paired -- their parities disagree"; return MQC_HIP_ERR_VALIDATION; }
        if (p.nbeta < 0 || p.nalpha < 0) { msg = "UHF: multiplicity asks for more unpaired electrons than the system has"; return MQC_HIP_ERR_VALIDATION; }
        if (p.nalpha < 1) { msg = "UHF: no electrons to place"; return MQC_HIP_ERR_VALIDATION; }
        if (p.xc.ncomp > 0 && topo.nao > 140) { msg = "unrestricted Kohn-Sham is available up to n_ao = 140"; return MQC_HIP_ERR_UNSUPPORTED; }
    } else if (topo.nelec < 2) { msg = "RHF: no electrons to place"; return MQC_HIP_ERR_VALIDATION; }
    if (o.guess < MQC_HIP_GUESS_AUTO || o.guess > MQC_HIP_GUESS_SAC) { msg = "unknown initial guess"; return MQC_HIP_ERR_VALIDATION; }
    if (o.guess == MQC_HIP_GUESS_SAC && p.uhf) { msg = "the SAC guess (free atoms' own spin densities) is available for restricted runs; unrestricted runs take sad, gwh or core"; return MQC_HIP_ERR_UNSUPPORTED; }
    if (o.max_iter < 1) { msg = "max_iter must be positive"; return MQC_HIP_ERR_VALIDATION; }
    if (o.use_diis && (o.diis_size < 0 || o.diis_size > DIIS_MAX)) { msg = "diis_size must be within 0..8"; return MQC_HIP_ERR_VALIDATION; }
    if (!o.density_fitting && o.eri_mode == MQC_HIP_ERI_INCORE && !incore_supported(topo.nao)) { msg = "fragment too large for the in-core exact-ERI path (n_ao <= 116); use eri_mode auto/direct or density fitting"; return MQC_HIP_ERR_UNSUPPORTED; }
    // f classes are digested by the LDS kernel: the exact-ERI paths cover them
    if (o.density_fitting && topo.lmax > 3) { msg = "density fitting covers orbital shells up to f"; return MQC_HIP_ERR_UNSUPPORTED; }
    // n_ao <= 140: the Fock matrix is diagonalised in LDS; up to 256 it is rotated in global memory (L2), exact-ERI
    // direct path and the quadrature's z-split; density fitting keeps the 140 limit (its J/K kernels tile n in LDS)
    if (topo.nao > 256) { msg = "fragment too large for the eigen-solver (n_ao <= 256)"; return MQC_HIP_ERR_UNSUPPORTED; }
    if (topo.nao > 140 && o.density_fitting) { msg = "density fitting is available up to n_ao = 140; larger fragments run on the direct exact-ERI path"; return MQC_HIP_ERR_UNSUPPORTED; }
    return MQC_HIP_OK;
}

static bool runs_unrestricted(const mqc_hip_scf_options_t& o, int multiplicity, int nelec);
int plan_batch(const mqc_hip_scf_options_t& o, const Topology& topo, int ntot, BatchPlan& p, std::string& msg)
{
    p.n = topo.nao; p.npair = topo.npair; p.natoms = topo.natoms;
    if (!parse_functional(o.functional, p.xc, msg)) return MQC_HIP_ERR_UNSUPPORTED;
    p.rsh = p.xc.omega > 0.0;
    p.uhf = runs_unrestricted(o, topo.multiplicity, topo.nelec);
    p.nalpha = p.uhf ? (topo.nelec + topo.multiplicity - 1) / 2 : topo.nelec / 2;
    p.nbeta = p.uhf ? topo.nelec - p.nalpha : topo.nelec / 2;
    p.nocc = p.nalpha;
    // exact-ERI path selection (mqc_libcint_bridge.f90:819-892 with an HBM budget instead of 2 GB of host memory)
    p.two_e = o.density_fitting ? TWO_E_DF
            : (o.eri_mode == MQC_HIP_ERI_DIRECT || (o.eri_mode == MQC_HIP_ERI_AUTO && !incore_supported(topo.nao))) ? TWO_E_DIRECT : TWO_E_INCORE;
    p.direct_tol = o.schwarz_tol > 0.0 ? o.schwarz_tol : 1.0e-11;   // mqc_libcint_direct.f90:61
    // Schwarz screening of the in-core build pays for itself through the quartets it drops; for a handful of fragments
    // the bounds (one thread per shell pair walking its primitive quartets: 1.6 ms for one cc-pVDZ water dimer) cost
    // more than the screened quartets save, and the unscreened tensor needs no zero fill.  Energies move by < 1e-11 Eh
    // either way (that is what the threshold means); MQC_HIP_SCHWARZ_MIN_FRAGMENTS=0 screens always.
    static const int schwarz_min = env_int("MQC_HIP_SCHWARZ_MIN_FRAGMENTS", 9);
    p.stol = (o.schwarz_tol > 0.0 && ntot >= schwarz_min) ? o.schwarz_tol : 0.0;
    return validate_options(o, topo, p, msg);
}

// restricted iff multiplicity 1, even electron count and not forced (mqc_cuest_driver.f90:127)
static bool runs_unrestricted(const mqc_hip_scf_options_t& o, int multiplicity, int nelec)
{
    return o.unrestricted || multiplicity != 1 || (nelec % 2) != 0;
}

static void fill_error(mqc_hip_scf_result_t* r, const std::string& msg)
{
    r->has_error = 1;
    std::snprintf(r->message, sizeof(r->message), "%s", msg.c_str());
}

// a batch that does not run: every fragment carries the reason
static int refuse(const std::vector<FragmentIO>& frags, int code, const std::string& msg)
{
    for (const FragmentIO& f : frags) { fill_error(f.result, msg); f.result->scf_status = MQC_HIP_SCF_NOT_RUN; }
    return fail(code, msg);
}

static DevicePool g_guess_pool[2];
static DevicePool g_restart_pool[2];     // per slot: which fragments of the chunk restart from a supplied density

struct Job {
    const FragmentIO* frag = nullptr;      // the chunk's fragments: nf consecutive records of the batch
    int nf = 0;
    BatchView bv{};
    std::vector<double> hx, hpc;
    std::vector<int> restart;      // per fragment of the chunk: 1 = starts from its supplied density
    PcmView pcm{};                 // C-PCM arrays of the chunk (stride 0: none), tesserae and counts as uploaded
    std::vector<double> hpcm;
    std::vector<int> hnt;
};

// MQC_HIP_PCM_TIMING=1: HIP-event times of the PCM setup and of its per-iteration kernel, one line per batch call.
// Everything is per lane: two topology groups of one call run on a lane each, from two host threads.
struct PcmTiming {
    hipEvent_t ev[2][4] = {};      // setup begin / end, iteration begin / end
    bool ready = false;
    double setup_s[2] = {}, iter_s[2] = {}, iter_bytes[2] = {};
    long launches[2] = {};
};
static PcmTiming g_pcm_timing;
static bool pcm_timing_on()
{
    // a function-local static: two lanes' host threads may come here at once, the events are made once
    static const bool on = [] {
        const bool want = env_opt_in("MQC_HIP_PCM_TIMING");
        if (want) {
            for (auto& lane : g_pcm_timing.ev) for (hipEvent_t& e : lane) (void)hipEventCreate(&e);
            g_pcm_timing.ready = true;
        }
        return want;
    }();
    return on;
}

bool xc_radial_cache_on()
{
    static const bool on = env_on("MQC_HIP_XC_RADIAL_CACHE");
    return on;
}

// ---- exchange-correlation: per-element grid templates and the per-topology point list
int upload_grid(mqc_hip_context* ctx, Batch& b, DevicePool& pool, hipStream_t s)
{
    const Topology& topo = b.topo;
    std::map<int, std::pair<int, int>> tmpl_of_z;     // Z -> (offset, count) in the packed template arrays
    std::vector<double> txyz, tw, sb(topo.natoms);
    std::vector<int> pt_atom, pt_tmpl;
    for (int a = 0; a < topo.natoms; ++a) {
        // a ghost centre enters the grid builder with Z = 0 (numbers = nint(mol%charges), mqc_libcint_xc.F90:181-183):
        // period-1 sizes, xi(0) = 1, Bragg radius(0) = 2 Angstrom -- it still owns grid points
        const int z = (topo.zeff[a] == 0.0) ? 0 : topo.Z[a];
        sb[a] = std::sqrt(bragg_radius_bohr(z)) + 1e-200;
        if (!tmpl_of_z.count(z)) {
            std::vector<double> x, w; std::string e;
            if (!build_atom_template(z, b.opts.grid_level, b.opts.radial_points, b.opts.angular_points, x, w, e))
                return refuse(b.frags, MQC_HIP_ERR_UNSUPPORTED, e);
            tmpl_of_z[z] = {(int)tw.size(), (int)w.size()};
            txyz.insert(txyz.end(), x.begin(), x.end());
            tw.insert(tw.end(), w.begin(), w.end());
        }
        const auto oc = tmpl_of_z[z];
        for (int k = 0; k < oc.second; ++k) { pt_atom.push_back(a); pt_tmpl.push_back(oc.first + k); }
    }
    GridDev& grid = b.grid;
    grid.npts = (int)pt_atom.size();
    const size_t b_int = (sizeof(int) * pt_atom.size() + 255) & ~size_t(255);
    const size_t b_xyz = (sizeof(double) * txyz.size() + 255) & ~size_t(255);
    const size_t b_w = (sizeof(double) * tw.size() + 255) & ~size_t(255);
    const size_t b_sb = (sizeof(double) * sb.size() + 255) & ~size_t(255);
    char* gb = (char*)pool.ensure(2 * b_int + b_xyz + b_w + b_sb + 1024);
    if (!gb) return fail(MQC_HIP_ERR_DEVICE, "out of device memory (grid templates)");
    int* d_pa = (int*)gb; int* d_pt = (int*)(gb + b_int);
    double* d_x = (double*)(gb + 2 * b_int); double* d_w = (double*)(gb + 2 * b_int + b_xyz);
    double* d_sb = (double*)(gb + 2 * b_int + b_xyz + b_w);
    HIP_CHECK_RET(hipMemcpyAsync(d_pa, pt_atom.data(), sizeof(int) * pt_atom.size(), hipMemcpyHostToDevice, s));
    HIP_CHECK_RET(hipMemcpyAsync(d_pt, pt_tmpl.data(), sizeof(int) * pt_tmpl.size(), hipMemcpyHostToDevice, s));
    HIP_CHECK_RET(hipMemcpyAsync(d_x, txyz.data(), sizeof(double) * txyz.size(), hipMemcpyHostToDevice, s));
    HIP_CHECK_RET(hipMemcpyAsync(d_w, tw.data(), sizeof(double) * tw.size(), hipMemcpyHostToDevice, s));
    HIP_CHECK_RET(hipMemcpyAsync(d_sb, sb.data(), sizeof(double) * sb.size(), hipMemcpyHostToDevice, s));
    HIP_CHECK_RET(hipStreamSynchronize(s));     // the host vectors go out of scope
    grid.pt_atom = d_pa; grid.pt_tmpl = d_pt; grid.tmpl_xyz = d_x; grid.tmpl_w = d_w; grid.sqrt_bragg = d_sb;
    return MQC_HIP_OK;
}

// J and K of the density in bv by the batch's two-electron path.  In the SCF loop (in_loop) the fragments that are
// done are skipped and a restricted direct build may go incrementally; an unrestricted view always builds in full.
static void jk_one(const BatchPlan& plan, const Topology& topo, const BatchView& bv, bool in_loop, hipStream_t s)
{
    if (plan.two_e == TWO_E_DF) launch_df_jk(bv, in_loop, s);
    else if (plan.two_e == TWO_E_INCORE) launch_jk_incore(bv, in_loop, s);
    else if (in_loop) launch_jk_direct_incremental(bv, topo, plan.direct_tol, true, s);     // restricted: G_ref += G(D - D_ref)
    else launch_jk_direct(bv, topo, plan.direct_tol, false, s);
}

// J/K of one SCF iteration: the alpha (or closed-shell) density, the beta density of an unrestricted run, then the
// long-range exchange of a range-separated hybrid folded into K
static int build_jk(const BatchPlan& plan, const Topology& topo, const BatchView& bv, hipStream_t s)
{
    jk_one(plan, topo, bv, true, s);
    if (plan.uhf) {
        BatchView vb = bv;
        vb.D = bv.Db; vb.J = bv.Jb; vb.K = bv.Kb;
        if (plan.two_e == TWO_E_DF) {
            // unrestricted density fitting, as run_uks_scf of the cuEST path (mqc_cuest_scf.f90:637-1009): J from each
            // spin density, K_s = sum_P (B_P C_s)(B_P C_s)^T; the kernels return the closed-shell 2 W W^T
            const size_t tot = (size_t)bv.nfrag * plan.n * plan.n;
            launch_scale(bv.K, tot, 0.5, s);
            if (plan.nbeta > 0) {
                vb.C = bv.Cb; vb.nocc = plan.nbeta;
                launch_df_jk(vb, true, s);
                launch_scale(bv.Kb, tot, 0.5, s);
            } else {
                HIP_CHECK_RET(hipMemsetAsync(bv.Jb, 0, sizeof(double) * tot, s));
                HIP_CHECK_RET(hipMemsetAsync(bv.Kb, 0, sizeof(double) * tot, s));
            }
        } else jk_one(plan, topo, vb, true, s);      // the same stream over the tensor, or the direct integrals formed again
    }
    if (plan.rsh) {
        // K_lr of each spin density from the long-range tensor (its J is not used), folded into K
        BatchView vl = bv;
        vl.eri = bv.eri_lr; vl.J = bv.Jlr; vl.K = bv.Klr; vl.jk_loaded = nullptr;
        launch_jk_incore(vl, true, s);
        launch_exchange_fold(bv, bv.K, bv.Klr, plan.xc.exx, plan.xc.exx_lr, s);
        if (plan.uhf) {
            vl.D = bv.Db; vl.K = bv.Klrb;
            launch_jk_incore(vl, true, s);
            launch_exchange_fold(bv, bv.Kb, bv.Klrb, plan.xc.exx, plan.xc.exx_lr, s);
        }
    }
    return MQC_HIP_OK;
}

// ---- stage 1 of a chunk: everything up to (and including) the guess, enqueued on the slot's stream
static int prepare(mqc_hip_context* ctx, const BatchPlan& plan, Batch& b, const Slot& sl, Job& job)
{
    const Topology& topo = b.topo;
    const mqc_hip_scf_options_t& opts = b.opts;
    const int nf = job.nf, n = plan.n;
    const FragmentIO* frag = job.frag;
    hipStream_t s = sl.lane->stream;
    const double t0 = now_s();
    BatchView& bv = job.bv;
    // range-separated hybrids: K is folded to exx K + exx_lr K_lr before the step, which then takes all of it
    bv.nalpha = plan.nalpha; bv.nbeta = plan.nbeta; bv.nocc = plan.nocc; bv.aux = b.tdx;
    bv.exx = plan.rsh ? 1.0 : plan.xc.exx; bv.e_tol = opts.energy_tol; bv.d_tol = opts.density_tol;
    bv.max_iter = opts.max_iter; bv.diis_size = opts.use_diis ? opts.diis_size : 0;
    bv.xc = plan.xc; bv.grid = b.grid;
    int rc = carve_slot(ctx, sl, plan, b.td, nf, bv, &job.pcm);
    if (rc != MQC_HIP_OK) return rc;
    if (plan.two_e == TWO_E_DF) HIP_CHECK_RET(hipMemsetAsync(bv.scal, 0, sizeof(double) * (size_t)nf * 8, s));
    if (plan.pcm_stride > 0) {
        // the tesserae of every fragment at the chunk's stride (the padding is never read as a position) and their counts
        const size_t ts = (size_t)plan.pcm_stride;
        job.hpcm.assign((size_t)nf * ts * 4, 0.0);
        job.hnt.resize(nf);
        for (int f = 0; f < nf; ++f) {
            const pcm::Cavity& cav = *frag[f].cavity;
            job.hnt[f] = cav.count;
            std::memcpy(&job.hpcm[(size_t)f * ts * 4], cav.xyza.data(), sizeof(double) * 4 * (size_t)cav.count);
        }
        HIP_CHECK_RET(hipMemcpyAsync(job.pcm.pts, job.hpcm.data(), sizeof(double) * job.hpcm.size(), hipMemcpyHostToDevice, s));
        HIP_CHECK_RET(hipMemcpyAsync(job.pcm.nt, job.hnt.data(), sizeof(int) * (size_t)nf, hipMemcpyHostToDevice, s));
    }
    job.hx.resize((size_t)nf * topo.natoms * 3);
    for (int f = 0; f < nf; ++f) std::memcpy(&job.hx[(size_t)f * topo.natoms * 3], frag[f].mol->xyz, sizeof(double) * topo.natoms * 3);
    HIP_CHECK_RET(hipMemcpyAsync(bv.xyz, job.hx.data(), sizeof(double) * job.hx.size(), hipMemcpyHostToDevice, s));
    if (plan.npc > 0) {
        // layout [charge][x, y, z, q][fragment], FRAGMENT FASTEST: the lanes of a wave are consecutive fragments, so a
        // wave reads a charge's component as one contiguous 512-byte line -- with [fragment][charge][4] every lane
        // streamed its own 49 KB array and a wave-load touched 64 cache lines (int1e: 40 % of a 512-fragment FMO run)
        job.hpc.resize((size_t)nf * plan.npc * 4);
        for (int f = 0; f < nf; ++f) {
            const mqc_hip_molecule_t* m = frag[f].mol;
            for (int g = 0; g < plan.npc; ++g) {
                double* q = &job.hpc[(size_t)g * 4 * nf + f];
                q[0] = m->point_charge_xyz[3 * g]; q[(size_t)nf] = m->point_charge_xyz[3 * g + 1]; q[2 * (size_t)nf] = m->point_charge_xyz[3 * g + 2];
                q[3 * (size_t)nf] = m->point_charges[g];
            }
        }
        HIP_CHECK_RET(hipMemcpyAsync((void*)bv.pc, job.hpc.data(), sizeof(double) * job.hpc.size(), hipMemcpyHostToDevice, s));
    }
    if (plan.hx)
        for (int f = 0; f < nf; ++f)
            HIP_CHECK_RET(hipMemcpyAsync((void*)(bv.Hx + (size_t)f * n * n), frag[f].mol->h_extra, sizeof(double) * n * n, hipMemcpyHostToDevice, s));
    HIP_CHECK_RET(hipMemsetAsync(bv.istate, 0, sizeof(int) * (size_t)nf * 4, s));
    HIP_CHECK_RET(hipMemsetAsync(bv.eri_count, 0, sizeof(unsigned long long), s));
    const double t1 = now_s();
    b.stats.t_setup += t1 - t0;

    const bool incore = plan.two_e == TWO_E_INCORE;
    if (incore) launch_eri_bounds(bv, topo, plan.stol, s);     // screened build: bounds run next to the 1e stage
    // The one-electron stage, the orthogonaliser and the starting guess need the geometry (S, H) only and are
    // latency-bound (six class launches; one workgroup per fragment, Jacobi sweeps): they run on a side stream next
    // to the compute-bound two-electron stage, which does not wait for them (0.7 ms of a single-fragment call)
    hipStream_t so = sl.lane->side[b.chain_side];
    HIP_CHECK_RET(hipEventRecord(sl.lane->chain[0], s));             // uploads and resets above are in
    HIP_CHECK_RET(hipStreamWaitEvent(so, sl.lane->chain[0], 0));
    launch_int1e(bv, topo, so);
    // block-sharing plan and class lists of the integral stage: host work that depends on the geometry only, done
    // here while the bounds and one-electron kernels run
    if (incore) eri_plan_lists(bv, topo, s, job.hx.data());
    if ((rc = stage_check("int1e")) != MQC_HIP_OK) return rc;
    launch_orthogonalizer(bv, so);
    if ((rc = stage_check("orthogonalizer")) != MQC_HIP_OK) return rc;
    // fragments that bring a starting density are projected below; a chunk made of them alone needs no other guess
    int n_restart = 0;
    if (b.any_d0) {
        job.restart.assign(nf, 0);
        for (int f = 0; f < nf; ++f) if (frag[f].d0) { job.restart[f] = 1; ++n_restart; }
    }
    const bool all_restart = n_restart == nf;
    if (!b.guess && !all_restart) launch_guess(bv, opts.guess == MQC_HIP_GUESS_CORE ? MQC_HIP_GUESS_CORE : MQC_HIP_GUESS_GWH, so);
    if ((rc = stage_check("guess")) != MQC_HIP_OK) return rc;
    HIP_CHECK_RET(hipEventRecord(sl.lane->chain[1], so));
    if (plan.xc.ncomp > 0) { launch_becke_weights(bv, s); if (bv.grid.rad) launch_xc_radial_cache(bv, s); }
    if ((rc = stage_check("grid weights")) != MQC_HIP_OK) return rc;
    const double t2 = now_s();
    b.stats.t_int1e += t2 - t1;

    HIP_CHECK_RET(hipEventRecord(sl.lane->eri[0], s));
    if (plan.two_e == TWO_E_DF) launch_df_build(bv, topo, *b.aux, s);
    else if (plan.two_e == TWO_E_DIRECT) launch_direct_setup(bv, topo, s);
    else {
        launch_eri(bv, topo, plan.stol, s, job.hx.data());
        if (plan.rsh) {
            // the long-range tensor: same lists, screening (the Coulomb bounds bound it) and block sharing
            BatchView vl = bv;
            vl.eri = bv.eri_lr;
            launch_eri(vl, topo, plan.stol, s, job.hx.data(), plan.xc.omega);
        }
        // the bounds of a screened build tell the J/K kernel which pair rows are all zeros (triangular tensor only)
        if (plan.stol > 0.0 && bv.eri_tri) eri_schwarz_view(bv.slot, &bv.jk_q, &bv.jk_qthresh);
    }
    HIP_CHECK_RET(hipEventRecord(sl.lane->eri[1], s));
    if ((rc = stage_check("two-electron setup")) != MQC_HIP_OK) return rc;
    if (plan.pcm_stride > 0) {
        // C-PCM setup, once per geometry, behind the two-electron stage on the lane's stream
        const bool timed = pcm_timing_on();
        if (timed) HIP_CHECK_RET(hipEventRecord(g_pcm_timing.ev[sl.id & 1][0], s));
        launch_pcm_setup(bv, job.pcm, topo, s);
        if (timed) HIP_CHECK_RET(hipEventRecord(g_pcm_timing.ev[sl.id & 1][1], s));
        if ((rc = stage_check("PCM setup")) != MQC_HIP_OK) return rc;
    }
    b.stats.eri_quartets += topo.n_quartets * nf;
    HIP_CHECK_RET(hipStreamWaitEvent(s, sl.lane->chain[1], 0));      // join: X, C, D of the guess are ready
    if (b.guess && !all_restart) {
        // superposed atoms (build_restricted_guess / atomic_guess_fock, mqc_libcint_atomic_guess.f90:168-212,
        // mqc_libcint_rhf.f90:1382-1411): the same block-diagonal density in every fragment of the topology, its
        // Hartree-Fock Fock matrix from the two-electron stage just built (full exchange), then the usual
        // diagonalisation and occupation -- both spins of an unrestricted run start from it
        const size_t nn = (size_t)n * n;
        double* d0 = (double*)g_guess_pool[sl.id & 1].ensure(sizeof(double) * 2 * nn + 256);
        if (!d0) return fail(MQC_HIP_ERR_DEVICE, "out of device memory (guess density)");
        HIP_CHECK_RET(hipMemcpyAsync(d0, b.guess->D0.data(), sizeof(double) * nn, hipMemcpyHostToDevice, s));
        launch_broadcast(bv.D, d0, nn, nf, s);
        BatchView vg = bv;
        vg.exx = 1.0; vg.uhf = 0;
        if (plan.two_e == TWO_E_DF) {
            HIP_CHECK_RET(hipMemcpyAsync(d0 + nn, b.guess->Cp.data(), sizeof(double) * nn, hipMemcpyHostToDevice, s));
            launch_broadcast(bv.C, d0 + nn, nn, nf, s);
            vg.nocc = b.guess->nmodes;
        }
        jk_one(plan, topo, vg, false, s);
        launch_guess(bv, MQC_HIP_GUESS_SAD, s);
        if ((rc = stage_check("atomic guess")) != MQC_HIP_OK) return rc;
    }
    if (n_restart > 0) {
        // supplied densities: each into its fragment's W0 (alpha, beta of an unrestricted run: W0, W1), then the
        // projection onto an SCF state of this geometry (kern_scf.hip, restart_kernel) over what the guess left there
        const size_t nn = (size_t)n * n, cnt = plan.uhf ? 2 * nn : nn;
        for (int f = 0; f < nf; ++f)
            if (job.restart[f])
                HIP_CHECK_RET(hipMemcpyAsync(bv.W + (size_t)f * 6 * nn, frag[f].d0, sizeof(double) * cnt, hipMemcpyHostToDevice, s));
        const int* d_flags = nullptr;
        if (!all_restart) {
            int* df = (int*)g_restart_pool[sl.id & 1].ensure(sizeof(int) * (size_t)nf + 256);
            if (!df) return fail(MQC_HIP_ERR_DEVICE, "out of device memory (restart flags)");
            HIP_CHECK_RET(hipMemcpyAsync(df, job.restart.data(), sizeof(int) * (size_t)nf, hipMemcpyHostToDevice, s));
            d_flags = df;
        }
        launch_restart(bv, d_flags, s);
        if ((rc = stage_check("restart projection")) != MQC_HIP_OK) return rc;
    }
    b.stats.t_eri += now_s() - t2;      // host time to enqueue; the kernels are timed by the lane's eri events
    return MQC_HIP_OK;
}

// ---- stage 2: the SCF loop, one int back per iteration (or per block of iterations)
static int scf_loop(const BatchPlan& plan, Batch& b, const Slot& sl, Job& job)
{
    const int nf = job.nf, n = plan.n;
    const double np = (double)plan.npair;
    Lane& lane = *sl.lane;
    hipStream_t s = lane.stream;
    BatchView& bv = job.bv;
    Stats& st = b.stats;
    const bool df = plan.two_e == TWO_E_DF, ks = plan.xc.ncomp > 0;
    const bool pcm_on = plan.pcm_stride > 0, pcm_timed = pcm_on && pcm_timing_on();
    int rc;
    const double t3 = now_s();
    HIP_CHECK_RET(hipStreamSynchronize(s));
    if ((rc = stage_check("integrals")) != MQC_HIP_OK) return rc;
    if (pcm_timed) {
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, g_pcm_timing.ev[sl.id & 1][0], g_pcm_timing.ev[sl.id & 1][1]);
        g_pcm_timing.setup_s[sl.id & 1] += ms * 1e-3;
    }
    if (b.gate) b.gate->open();         // deferred small groups start now: from here on this batch uses one stream
    {
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, lane.eri[0], lane.eri[1]);
        st.eri_kernel_seconds += ms * 1e-3;
    }
    int remaining = nf;
    int guard = 0;
    double tri_doubles_per_fragment = -1.0;      // read back after the first J/K launch of the chunk
    // Small batches are latency-bound: the host round trip after every iteration (one int back, ~50 us) costs as
    // much as the kernels.  They run BLOCKS of iterations between two reads of the counter -- finished fragments
    // drop out of every kernel by themselves (state machine), so an iteration enqueued past convergence is three
    // empty launches.  Large batches keep one read per iteration (MQC_HIP_SCF_SYNC_BLOCK overrides: 1 = always).
    static const int sync_block_env = env_int("MQC_HIP_SCF_SYNC_BLOCK", 0);
    static const int block_max_frag = env_int("MQC_HIP_SCF_BLOCK_MAX_FRAGMENTS", 256);
    const bool blocked = sync_block_env != 1 && nf <= block_max_frag;
    const int max_guard = b.opts.max_iter + 2;
    int blocks_done = 0;
    while (remaining > 0 && guard < max_guard) {
        int block_len = 1;
        if (blocked) block_len = sync_block_env > 1 ? sync_block_env : (blocks_done == 0 ? 8 : 4);
        if (block_len > max_guard - guard) block_len = max_guard - guard;
        ++blocks_done;
        for (int bi = 0; bi < block_len; ++bi) {
            HIP_CHECK_RET(hipEventRecord(lane.fock[0], s));
            if ((rc = build_jk(plan, b.topo, bv, s)) != MQC_HIP_OK) return rc;
            HIP_CHECK_RET(hipEventRecord(lane.fock[1], s));
            if (guard == 0 && (rc = stage_check("J/K build")) != MQC_HIP_OK) return rc;
            if (ks) {
                HIP_CHECK_RET(hipEventRecord(lane.xc[0], s));
                launch_xc(bv, true, s);
                HIP_CHECK_RET(hipEventRecord(lane.xc[1], s));
            }
            if (pcm_on) {
                // V_pcm and E_pcm of this density into the accumulator and scal[5], after the quadrature (which zeroes both)
                if (pcm_timed) HIP_CHECK_RET(hipEventRecord(g_pcm_timing.ev[sl.id & 1][2], s));
                launch_pcm_iteration(bv, job.pcm, ks, s);
                if (pcm_timed) HIP_CHECK_RET(hipEventRecord(g_pcm_timing.ev[sl.id & 1][3], s));
            }
            HIP_CHECK_RET(hipEventRecord(lane.step[0], s));
            launch_scf_step(bv, s);
            HIP_CHECK_RET(hipEventRecord(lane.step[1], s));
            if (bi + 1 < block_len) { ++guard; continue; }
            HIP_CHECK_RET(hipMemcpyAsync(sl.h_counter, bv.counters, sizeof(int), hipMemcpyDeviceToHost, s));
            HIP_CHECK_RET(hipStreamSynchronize(s));
            float ms = 0.f;
            if (pcm_timed) {
                // bytes of the kernel's two passes over the rows of B the active fragments own
                (void)hipEventElapsedTime(&ms, g_pcm_timing.ev[sl.id & 1][2], g_pcm_timing.ev[sl.id & 1][3]);
                double rows = 0.0;
                for (int v : job.hnt) rows += v;
                g_pcm_timing.iter_s[sl.id & 1] += ms * 1e-3 * block_len;
                g_pcm_timing.iter_bytes[sl.id & 1] += 2.0 * 8.0 * rows * np * ((double)remaining / nf) * block_len;
                g_pcm_timing.launches[sl.id & 1] += block_len;
            }
            (void)hipEventElapsedTime(&ms, lane.step[0], lane.step[1]);
            st.scf_step_seconds += ms * 1e-3 * block_len;
            (void)hipEventElapsedTime(&ms, lane.fock[0], lane.fock[1]);
            if (df) {
                st.df_bytes += (double)remaining * 8.0 * (double)plan.naux * (double)n * (double)n * block_len;
                st.df_flops += (double)remaining * 4.0 * (double)plan.naux * (double)n * (double)n * (1.0 + (plan.xc.exx != 0.0 ? (double)plan.nocc : 0.0)) * block_len;
            }
            // density fitting: the J/K kernel reads the fitted tensor once, and it is stored packed [naux][npair] -- about
            // half of SURVEY 8d's 8 n^2 A (df_bytes keeps that figure; fock_bytes is what the kernel really streams)
            // in-core: the tensor as stored -- the square, or its lower triangle (BatchView::eri_tri) -- once per spin density;
            // the triangular kernel skips rows the Schwarz bounds prove zero and reports the chunks it did read
            if (bv.eri_tri && bv.jk_loaded && tri_doubles_per_fragment < 0.0) {
                std::vector<int> ld(nf);
                // on this batch's own stream (it was joined a few lines up): a copy on the null stream waits for every blocking
                // stream of the process, the other lane's included -- for its whole integral stage when that has just begun
                if (hipMemcpyAsync(ld.data(), bv.jk_loaded, sizeof(int) * (size_t)nf, hipMemcpyDeviceToHost, s) == hipSuccess &&
                    hipStreamSynchronize(s) == hipSuccess) {
                    double sum = 0.0;
                    for (int v : ld) sum += v;
                    tri_doubles_per_fragment = 128.0 * sum / (double)nf;
                } else tri_doubles_per_fragment = (double)bv.eri_stride;
            }
            const double tensor_doubles = (bv.eri_tri && tri_doubles_per_fragment >= 0.0) ? tri_doubles_per_fragment
                                                                                         : (bv.eri_stride ? (double)bv.eri_stride : np * np);
            const double launch_bytes = df ? (double)remaining * (double)plan.naux * np * 8.0
                                           : (double)remaining * tensor_doubles * 8.0 * (plan.uhf ? 2.0 : 1.0);
            st.fock_kernel_seconds += ms * 1e-3 * block_len;
            st.fock_bytes += launch_bytes * block_len;
            st.fock_launches += block_len;
            if (launch_bytes >= 1073741824.0) {
                st.fock_big_launches += 1; st.fock_big_seconds += ms * 1e-3; st.fock_big_bytes += launch_bytes;
            }
            if (ks) {
                float mx = 0.f;
                (void)hipEventElapsedTime(&mx, lane.xc[0], lane.xc[1]);
                st.xc_kernel_seconds += mx * 1e-3 * block_len;
                st.xc_points += (double)remaining * plan.npts * block_len;
                st.xc_flops += (double)remaining * plan.npts * (plan.xc.gga ? 8.0 : 4.0) * (double)n * (double)n * block_len;
            }
            remaining = sl.h_counter[0];
            ++guard;
        }
    }
    if ((rc = stage_check("SCF loop")) != MQC_HIP_OK) return rc;
    st.t_fock += now_s() - t3;
    return MQC_HIP_OK;
}

// + nuclear repulsion: dE_nuc/dR_A = -sum_B Z_A Z_B (R_A - R_B)/|R_AB|^3 (ghosts carry no charge)
static void nuclear_gradient(const Topology& topo, const double* x, const double* g_elec, double* g)
{
    for (int a = 0; a < topo.natoms; ++a) {
        double g3[3] = {g_elec[3 * a], g_elec[3 * a + 1], g_elec[3 * a + 2]};
        for (int b = 0; b < topo.natoms; ++b) {
            if (b == a || topo.zeff[a] == 0.0 || topo.zeff[b] == 0.0) continue;
            const double dx = x[3 * a] - x[3 * b], dy = x[3 * a + 1] - x[3 * b + 1], dz = x[3 * a + 2] - x[3 * b + 2];
            const double r2 = dx * dx + dy * dy + dz * dz, r3 = r2 * std::sqrt(r2);
            const double zz = topo.zeff[a] * topo.zeff[b] / r3;
            g3[0] -= zz * dx; g3[1] -= zz * dy; g3[2] -= zz * dz;
        }
        g[3 * a] = g3[0]; g[3 * a + 1] = g3[1]; g[3 * a + 2] = g3[2];
    }
}

// <S^2> = S_z (S_z + 1) + n_beta - sum_ij |<a_i|S|b_j>|^2  (spin_contamination, mqc_libcint_rhf.f90)
static double s_squared(int n, int nalpha, int nbeta, const double* Ca, const double* Cb, const double* S)
{
    double ov2 = 0.0;
    std::vector<double> SCb((size_t)n * std::max(nbeta, 1));
    for (int mu = 0; mu < n; ++mu)
        for (int j = 0; j < nbeta; ++j) {
            double t = 0.0;
            for (int nu = 0; nu < n; ++nu) t += S[(size_t)mu * n + nu] * Cb[(size_t)nu * n + j];
            SCb[(size_t)mu * nbeta + j] = t;
        }
    for (int i = 0; i < nalpha; ++i)
        for (int j = 0; j < nbeta; ++j) {
            double t = 0.0;
            for (int mu = 0; mu < n; ++mu) t += Ca[(size_t)mu * n + i] * SCb[(size_t)mu * nbeta + j];
            ov2 += t * t;
        }
    const double sz = 0.5 * (nalpha - nbeta);
    return sz * (sz + 1.0) + nbeta - ov2;
}

// mu = sum_A Z_A (R_A - O) - [tr(D r) - O tr(D S)], O = centre of nuclear charge, tr(D S) = N_electrons
// (system_compute_dipole, mqc_cuest_integrals.f90:1443-1521); dr = tr(D x), tr(D y), tr(D z) about the origin
static void dipole(const Topology& topo, const double* x, const double* dr, double* mu_out)
{
    double ztot = 0.0, o[3] = {0, 0, 0}, mu[3] = {0, 0, 0};
    for (int a = 0; a < topo.natoms; ++a) { ztot += topo.zeff[a]; for (int c = 0; c < 3; ++c) o[c] += topo.zeff[a] * x[3 * a + c]; }
    if (ztot > 0.0) for (int c = 0; c < 3; ++c) o[c] /= ztot; else for (int c = 0; c < 3; ++c) o[c] = 0.0;
    for (int a = 0; a < topo.natoms; ++a) for (int c = 0; c < 3; ++c) mu[c] += topo.zeff[a] * (x[3 * a + c] - o[c]);
    for (int c = 0; c < 3; ++c) mu_out[c] = mu[c] - (dr[c] - o[c] * (double)topo.nelec);
}

// what the embedded callers read besides the energy: tr(D u), u itself (U != nullptr), Mulliken populations
// (inner_scf / fragment_charges, mqc_libcint_fmo.f90:1992-2021)
static void embedding_and_mulliken(const Topology& topo, const double* D, const double* U, const double* S, mqc_hip_scf_result_t* r)
{
    const int n = topo.nao;
    const size_t nn = (size_t)n * n;
    if (U) {
        double e = 0.0;
        for (size_t k = 0; k < nn; ++k) e += D[k] * U[k];
        r->e_embedding = e;
        if (r->embedding_matrix) std::memcpy(r->embedding_matrix, U, sizeof(double) * nn);
    }
    if (r->mulliken_charges) {
        for (int a = 0; a < topo.natoms; ++a) r->mulliken_charges[a] = topo.zeff[a];
        for (size_t sh = 0; sh < topo.shells.size(); ++sh) {
            const int a = topo.shells[sh].atom, o0 = topo.shells[sh].aoff, nf_sh = 2 * topo.shells[sh].l + 1;
            for (int mu = o0; mu < o0 + nf_sh; ++mu) {
                double pop = 0.0;
                for (int nu = 0; nu < n; ++nu) pop += D[(size_t)mu * n + nu] * S[(size_t)nu * n + mu];
                r->mulliken_charges[a] -= pop;
            }
        }
    }
}

// what a chunk's results are made of, read back once after its SCF loop
struct ChunkOut {
    std::vector<double> scal, eps, epsb, dip, grad, pcgrad, mp2, pcm, alpha;
    std::vector<int> cphf_iter, cphf_status;
    std::vector<double> D, U, S;      // total density, embedding operator, overlap: only where a caller reads them
    std::vector<double> Da, Db;       // spin densities of an unrestricted chunk, where a caller asked for them
    std::vector<int> ist;
};

// the result record of fragment f of the chunk
static int write_result(const BatchPlan& plan, Batch& b, const Job& job, const ChunkOut& o, int f, hipStream_t s)
{
    const Topology& topo = b.topo;
    const int n = plan.n, nocc = plan.nocc;
    const size_t nn = (size_t)n * n;
    const FragmentIO& io = job.frag[f];
    mqc_hip_scf_result_t* r = io.result;
    const double* x = io.mol->xyz;
    const int nmo = o.ist[4 * f + 2];
    r->n_ao = n; r->n_mo = nmo; r->n_occ = nocc;
    if (nocc > nmo) {
        // nmo check: more occupied orbitals than the basis supports after dropping near-null modes
        fill_error(r, plan.uhf ? "UHF: more alpha electrons than the basis supports after near-null modes were dropped"
                               : "RHF: more occupied orbitals than the basis supports after near-null modes were dropped");
        r->scf_status = MQC_HIP_SCF_NOT_RUN;
        return MQC_HIP_OK;
    }
    r->e_nuclear = nuclear_repulsion(topo, x);
    r->e_electronic = o.scal[8 * f + 4];
    r->e_total = r->e_electronic + r->e_nuclear;
    r->e_xc = plan.xc.ncomp > 0 ? o.scal[8 * f + 5] : 0.0;
    if (plan.pcm_stride > 0) r->e_xc = plan.xc.ncomp > 0 ? o.pcm[8 * f + 1] : 0.0;      // scal[5] holds E_xc + E_pcm there
    r->iterations = o.ist[4 * f + 1];
    const bool conv = o.ist[4 * f + 3] != 0 && o.ist[4 * f] == ST_DONE;
    r->scf_status = conv ? MQC_HIP_SCF_CONVERGED : MQC_HIP_SCF_NOT_CONVERGED;
    r->homo = o.eps[(size_t)f * n + nocc - 1];
    r->lumo = nocc < nmo ? o.eps[(size_t)f * n + nocc] : 0.0;
    r->has_orbitals = 1;
    r->n_alpha = plan.nalpha; r->n_beta = plan.nbeta; r->s_squared = 0.0;
    if (b.opts.want_gradient && r->gradient) {
        nuclear_gradient(topo, x, &o.grad[(size_t)f * topo.natoms * 3], r->gradient);
        r->has_gradient = 1;
    }
    // the charges stay out of E_nuc, so their gradient is the device's as it stands
    if (b.opts.want_gradient && plan.npc > 0 && io.pcgrad)
        std::memcpy(io.pcgrad, &o.pcgrad[(size_t)f * plan.npc * 3], sizeof(double) * (size_t)plan.npc * 3);
    if (plan.uhf) {
        std::vector<double> Ca(nn), Cb(nn), Sm(nn);
        HIP_CHECK_RET(hipMemcpyAsync(Ca.data(), job.bv.C + (size_t)f * nn, sizeof(double) * nn, hipMemcpyDeviceToHost, s));
        HIP_CHECK_RET(hipMemcpyAsync(Cb.data(), job.bv.Cb + (size_t)f * nn, sizeof(double) * nn, hipMemcpyDeviceToHost, s));
        HIP_CHECK_RET(hipMemcpyAsync(Sm.data(), job.bv.S + (size_t)f * nn, sizeof(double) * nn, hipMemcpyDeviceToHost, s));
        HIP_CHECK_RET(hipStreamSynchronize(s));
        r->s_squared = s_squared(n, plan.nalpha, plan.nbeta, Ca.data(), Cb.data(), Sm.data());
        if (r->orbital_energies_beta) std::memcpy(r->orbital_energies_beta, &o.epsb[(size_t)f * n], sizeof(double) * nmo);
    }
    dipole(topo, x, &o.dip[4 * f], r->dipole);
    r->has_dipole = 1;
    if (r->orbital_energies) std::memcpy(r->orbital_energies, &o.eps[(size_t)f * n], sizeof(double) * nmo);
    const bool embedded = plan.npc > 0 || plan.hx;
    if (embedded || r->mulliken_charges)
        embedding_and_mulliken(topo, o.D.data() + f * nn, embedded ? o.U.data() + f * nn : nullptr,
                               r->mulliken_charges ? o.S.data() + f * nn : nullptr, r);
    if (r->density) std::memcpy(r->density, o.D.data() + f * nn, sizeof(double) * nn);
    if (plan.uhf && io.spin_out) {
        std::memcpy(io.spin_out, o.Da.data() + f * nn, sizeof(double) * nn);
        std::memcpy(io.spin_out + nn, o.Db.data() + f * nn, sizeof(double) * nn);
    }
    r->has_error = 0; r->message[0] = '\0';
    if (plan.two_e == TWO_E_DF && o.scal[8 * f + 7] == 1.0)
        fill_error(r, "density fitting: the auxiliary metric (P|Q) could not be factorised or diagonalised");
    else if (plan.pcm_stride > 0 && o.pcm[8 * f + 7] != 0.0)
        fill_error(r, "PCM: the cavity matrix S of this fragment could not be factorised (a pivot failed)");
    else if (!std::isfinite(r->e_total)) fill_error(r, "SCF produced a non-finite energy");
    else if (!conv && !b.opts.allow_crap_scf)
        fill_error(r, "SCF did not converge in " + std::to_string(r->iterations) + " iterations");
    if (plan.pcm_stride > 0 && io.e_pcm && !r->has_error) *io.e_pcm = o.pcm[8 * f];
    if (b.mp2_frozen >= 0 && conv && !r->has_error) {
        // the correlation energy belongs to converged orbitals only; everything else keeps the entry's zeros
        *io.mp2_os = o.mp2[2 * f];
        *io.mp2_ss = o.mp2[2 * f + 1];
        *io.mp2_done = 1;
    }
    if (b.cphf && conv && !r->has_error) {
        // alpha belongs to a converged solve on converged orbitals; everything else keeps the entry's zeros
        const int status = o.cphf_status[f];
        *io.cphf_iter = o.cphf_iter[f];
        if (status == CPHF_CONVERGED) {
            std::memcpy(io.alpha, &o.alpha[(size_t)9 * f], sizeof(double) * 9);
            *io.alpha_done = 1;
        } else if (status == CPHF_UNSTABLE)
            fill_error(r, "CPHF: the RHF solution is unstable (a search direction with p.Ap <= 0)");
        else
            fill_error(r, "CPHF did not converge in " + std::to_string(o.cphf_iter[f]) + " iterations");
    }
    b.stats.scf_iterations_total += r->iterations;
    return MQC_HIP_OK;
}

// ---- stage 3: gradient, dipole integrals and the chunk's arrays back to the host, then the result records
static int fetch_results(const BatchPlan& plan, Batch& b, const Slot& sl, Job& job)
{
    const Topology& topo = b.topo;
    const int nf = job.nf, n = plan.n;
    const size_t tot = (size_t)nf * n * n;
    const FragmentIO* frag = job.frag;
    hipStream_t s = sl.lane->stream;
    const BatchView& bv = job.bv;
    const double t4 = now_s();
    ChunkOut o;
    o.scal.resize((size_t)nf * 8); o.eps.resize((size_t)nf * n); o.dip.resize((size_t)nf * 4); o.ist.resize((size_t)nf * 4);
    unsigned long long formed = 0;
    // ---- analytic gradient (compute_scf_gradient, mqc_cuest_gradient.f90:91-175): device terms here, E_nuc' on the host
    if (b.opts.want_gradient) {
        size_t lint = topo.pairs.size() + 64;
        for (auto& cl : topo.classes) lint += cl.quartets.size();
        const size_t nnh = (size_t)n * n;
        // embedded fragments: the sites' gradient [nf][npc][3] and the Hermite records of the charges' part
        const size_t pcg = plan.npc > 0 ? (((size_t)nf * plan.npc * 3 + 7) & ~size_t(7)) : 0;
        const size_t pcrec = plan.npc > 0 ? (size_t)nf * gradpc_record_doubles(topo) : 0;
        const size_t bytes = sizeof(double) * ((size_t)nf * topo.natoms * 3 + 2 * (size_t)nf * nnh + 8 + pcg + pcrec) + sizeof(int) * (lint + 64);
        char* gb = (char*)g_grad_pool[sl.id & 1].ensure(bytes);
        if (!gb) return fail(MQC_HIP_ERR_DEVICE, "out of device memory (gradient)");
        double* d_grad = (double*)gb;
        double* gwork = d_grad + (((size_t)nf * topo.natoms * 3 + 7) & ~size_t(7));
        double* d_pcgrad = gwork + 2 * (size_t)nf * nnh;
        double* d_pcrec = d_pcgrad + pcg;
        int* glists = (int*)(d_pcrec + pcrec);
        // above n_ao = 140 the two-electron term skips the (quartet, fragment) tasks the direct path's Schwarz bounds
        // (still resident in this slot) prove below 1e-3 of its threshold: a derivative integral exceeds the bound of
        // its undifferentiated quartet, and at the threshold itself the dropped tasks moved a (H2O)6 / cc-pVDZ
        // gradient by 3.8e-9.  MQC_HIP_GRAD_SCREEN=0 forms them all (A/B switch)
        static const bool grad_screen = env_on("MQC_HIP_GRAD_SCREEN");
        const double* gq = (grad_screen && plan.two_e == TWO_E_DIRECT && n > 140) ? direct_schwarz_view(bv.slot) : nullptr;
        std::string gerr;
        if (!launch_gradient(bv, topo, b.aux, d_grad, gwork, glists, lint, s, gerr, gq, 1.0e-3 * plan.direct_tol)) return fail(MQC_HIP_ERR_UNSUPPORTED, gerr);
        if (plan.npc > 0) {
            // launch_gradient leaves the total density of an unrestricted run behind its energy-weighted density
            const double* Dtot = plan.uhf ? gwork + (size_t)nf * nnh : bv.D;
            if (!launch_pc_gradient(bv, topo, Dtot, d_grad, d_pcgrad, d_pcrec, s, gerr)) return fail(MQC_HIP_ERR_UNSUPPORTED, gerr);
            o.pcgrad.resize((size_t)nf * plan.npc * 3);
            HIP_CHECK_RET(hipMemcpyAsync(o.pcgrad.data(), d_pcgrad, sizeof(double) * o.pcgrad.size(), hipMemcpyDeviceToHost, s));
        }
        o.grad.resize((size_t)nf * topo.natoms * 3);
        HIP_CHECK_RET(hipMemcpyAsync(o.grad.data(), d_grad, sizeof(double) * o.grad.size(), hipMemcpyDeviceToHost, s));
    }
    // ---- RI-MP2 (mqc_hip_rimp2_batch): the fitted tensor, the orbitals and their energies of this chunk are still in place
    if (b.mp2_frozen >= 0) {
        o.mp2.assign((size_t)nf * 2, 0.0);
        std::string merr;
        if (!launch_rimp2(bv, b.mp2_frozen, o.mp2.data(), s, merr)) return fail(MQC_HIP_ERR_DEVICE, merr);
        int mrc = stage_check("RI-MP2");
        if (mrc != MQC_HIP_OK) return mrc;
    }
    // ---- CPHF (mqc_hip_polarizability_batch): the square tensor, the orbitals and their energies are still in place
    if (b.cphf) {
        o.alpha.assign((size_t)nf * 9, 0.0); o.cphf_iter.assign(nf, 0); o.cphf_status.assign(nf, CPHF_NOT_SOLVED);
        std::string cerr;
        if (!launch_cphf(bv, topo, b.cphf->tol, b.cphf->max_iter, o.alpha.data(), o.cphf_iter.data(), o.cphf_status.data(), sl.h_counter, s, cerr))
            return fail(MQC_HIP_ERR_DEVICE, cerr);
        int crc = stage_check("CPHF");
        if (crc != MQC_HIP_OK) return crc;
    }
    launch_dipole(bv, topo, s);
    if (plan.uhf) {
        BatchView vb = bv;
        vb.D = bv.Db;
        launch_dipole(vb, topo, s, true);      // total density = D_a + D_b
        o.epsb.resize((size_t)nf * n);
        HIP_CHECK_RET(hipMemcpyAsync(o.epsb.data(), bv.epsb, sizeof(double) * o.epsb.size(), hipMemcpyDeviceToHost, s));
    }
    HIP_CHECK_RET(hipMemcpyAsync(o.dip.data(), bv.dip, sizeof(double) * o.dip.size(), hipMemcpyDeviceToHost, s));
    HIP_CHECK_RET(hipMemcpyAsync(&formed, bv.eri_count, sizeof(formed), hipMemcpyDeviceToHost, s));
    HIP_CHECK_RET(hipMemcpyAsync(o.scal.data(), bv.scal, sizeof(double) * o.scal.size(), hipMemcpyDeviceToHost, s));
    if (plan.pcm_stride > 0) {
        o.pcm.resize((size_t)nf * 8);
        HIP_CHECK_RET(hipMemcpyAsync(o.pcm.data(), job.pcm.scal, sizeof(double) * o.pcm.size(), hipMemcpyDeviceToHost, s));
    }
    HIP_CHECK_RET(hipMemcpyAsync(o.eps.data(), bv.eps, sizeof(double) * o.eps.size(), hipMemcpyDeviceToHost, s));
    HIP_CHECK_RET(hipMemcpyAsync(o.ist.data(), bv.istate, sizeof(int) * o.ist.size(), hipMemcpyDeviceToHost, s));
    // matrices the callers asked for (total density, embedding operator, overlap): the whole chunk in one copy each
    // (one synchronous copy per matrix and fragment cost seconds of a 130 000-pair batch)
    const bool embedded = plan.npc > 0 || plan.hx;
    bool want_d = embedded, want_s = false;
    for (int f = 0; f < nf; ++f) {
        const mqc_hip_scf_result_t* r = frag[f].result;
        if (r->mulliken_charges) { want_d = true; want_s = true; }
        if (r->density) want_d = true;
    }
    auto fetch = [&](std::vector<double>& h, const double* d) {
        h.resize(tot);
        return hipMemcpyAsync(h.data(), d, sizeof(double) * tot, hipMemcpyDeviceToHost, s);
    };
    if (want_d) HIP_CHECK_RET(fetch(o.D, bv.D));
    if (embedded) HIP_CHECK_RET(fetch(o.U, bv.U));
    if (want_s) HIP_CHECK_RET(fetch(o.S, bv.S));
    bool want_spin = false;
    if (plan.uhf)
        for (int f = 0; f < nf; ++f) want_spin = want_spin || frag[f].spin_out != nullptr;
    if (want_spin) { HIP_CHECK_RET(fetch(o.Da, bv.D)); HIP_CHECK_RET(fetch(o.Db, bv.Db)); }
    if (want_d && plan.uhf) {
        std::vector<double> db;
        HIP_CHECK_RET(fetch(db, bv.Db));
        HIP_CHECK_RET(hipStreamSynchronize(s));
        for (size_t k = 0; k < tot; ++k) o.D[k] += db[k];          // total density = alpha + beta
    }
    HIP_CHECK_RET(hipStreamSynchronize(s));
    b.stats.eri_survivors += (int64_t)formed;
    for (int f = 0; f < nf; ++f) {
        const int rc = write_result(plan, b, job, o, f, s);
        if (rc != MQC_HIP_OK) return rc;
    }
    b.stats.t_scf_step += now_s() - t4;
    return MQC_HIP_OK;
}

// One topology group of a batch call, in the caller's order: what run_batch runs and where its status goes
struct Work {
    std::shared_ptr<Topology> topo, aux;
    std::vector<FragmentIO> frags;
    bool embedded_entry = false;         // the call came through mqc_hip_scf_gradient_embedded_batch
    bool any_d0 = false;                 // mqc_hip_scf_run_batch_restart: some fragment of the group brought a starting density
    int mp2_frozen = -1;                 // mqc_hip_rimp2_batch only: frozen orbitals of the topology (>= 0)
    double pcm_f = -1.0;                 // mqc_hip_scf_pcm_batch only: (epsilon - 1) / epsilon, and the fragments' cavities
    const mqc_hip_cphf_options_t* cphf = nullptr;   // mqc_hip_polarizability_batch only: the settings of the solve
    std::vector<pcm::Cavity> cavities;   // (reserved up front: the fragment records point into it)
    std::shared_ptr<AtomicGuess> guess;
    // deferred small groups (schedule_groups): the largest group's batch opens the gate, the others wait at it
    GroupGate* opens = nullptr;
    GroupGate* waits = nullptr;
    int rc = MQC_HIP_OK;
    std::string msg;
};

// lane < 0: the batch owns both lanes (chunks alternate, next chunk prepared ahead); lane 0/1: it runs on that
// lane only, so that two topology groups can be driven by two host threads at once
static int run_batch(mqc_hip_context* ctx, const Work& w, const mqc_hip_scf_options_t& opts, int lane)
{
    const Topology& topo = *w.topo;
    const Topology* aux = w.aux.get();
    Lane& own = ctx->lane[lane == 1 ? 1 : 0];        // where the per-batch tables go
    const double t_begin = now_s();
    const int ntot = (int)w.frags.size();
    Batch b{topo, aux, opts, w.guess.get()};
    b.embedded_entry = w.embedded_entry; b.any_d0 = w.any_d0; b.mp2_frozen = w.mp2_frozen; b.pcm_f = w.pcm_f;
    b.cphf = w.cphf;
    b.gate = w.opens;
    if (w.waits && lane == 1) b.chain_side = 1;      // deferred on lane 1: its third side stream stays idle (schedule_groups)
    // whichever way this batch ends (refusal, error return, no chunk that reaches scf_loop), the waiting groups go on
    struct GateOpener { GroupGate* g; ~GateOpener() { if (g) g->open(); } } const opener{w.opens};
    BatchPlan plan;
    plan.square_only = w.cphf != nullptr;      // the multi-density stream reads the square tensor: the chunks are sized for it
    // external point charges (FMO / EE-MBE embedding) and h_extra: the same in every fragment of the group (its key says so)
    plan.npc = ntot > 0 ? w.frags[0].mol->n_point_charges : 0;
    plan.hx = ntot > 0 && w.frags[0].mol->h_extra != nullptr;
    const bool embedded = plan.npc > 0 || plan.hx;
    {
        // Order the batch by compactness (nuclear repulsion, most compact first).  Lanes of a wave are
        // consecutive fragments: with similar geometries side by side, the primitive-pair screening and
        // the Schwarz ballot drop the same work in every lane, so whole waves skip it.
        std::vector<std::pair<double, int>> key(ntot);
        for (int i = 0; i < ntot; ++i) key[i] = {-nuclear_repulsion(topo, w.frags[i].mol->xyz), i};
        std::stable_sort(key.begin(), key.end());
        for (auto& k : key) b.frags.push_back(w.frags[k.second]);      // a whole record: inputs and destinations move together
    }
    std::string msg;
    int rc = plan_batch(opts, topo, ntot, plan, msg);
    if (rc == MQC_HIP_OK && w.pcm_f >= 0.0) {
        // C-PCM: one stride for every chunk of the batch, the largest tessera count rounded up to 64
        int largest = 0;
        for (const FragmentIO& f : b.frags) largest = std::max(largest, f.cavity->count);
        plan.pcm_stride = pcm::chunk_stride(largest);
        plan.pcm_f = w.pcm_f;
    }
    if (rc == MQC_HIP_OK && embedded && opts.want_gradient) {
        if (!b.embedded_entry) {
            msg = "analytic gradients of a fragment embedded in point charges or an extra one-electron operator are not returned by this entry "
                  "(the result record has no slot for the charges' own gradient): point charges go through mqc_hip_scf_gradient_embedded_batch";
            rc = MQC_HIP_ERR_UNSUPPORTED;
        } else if (plan.hx) {
            msg = "analytic gradients of a fragment with an extra one-electron operator (h_extra) are not built: the engine does not know its derivative";
            rc = MQC_HIP_ERR_UNSUPPORTED;
        }
    }
    if (rc == MQC_HIP_OK && plan.npc > 0)
        for (int k = 0; k < ntot && rc == MQC_HIP_OK; ++k)
            if (!b.frags[k].mol->point_charge_xyz || !b.frags[k].mol->point_charges) { msg = "point charges announced but their arrays are NULL"; rc = MQC_HIP_ERR_VALIDATION; }
    if (rc == MQC_HIP_OK && plan.two_e == TWO_E_DF && !aux) { msg = "density fitting needs an auxiliary basis"; rc = MQC_HIP_ERR_VALIDATION; }
    if (rc != MQC_HIP_OK) return refuse(b.frags, rc, msg);
    if (w.waits) w.waits->wait();       // nothing of a deferred group is enqueued before the large group's integrals are done
    rc = upload_topology(ctx, topo, b.td, &own.topo, own.stream);
    if (rc != MQC_HIP_OK) return rc;
    if (plan.two_e == TWO_E_DF) {
        rc = upload_topology(ctx, *aux, b.tdx, &own.aux, own.stream);
        if (rc != MQC_HIP_OK) return rc;
        plan.naux = aux->nao;
    }
    if (plan.xc.ncomp > 0 && (rc = upload_grid(ctx, b, own.grid, own.stream)) != MQC_HIP_OK) return rc;
    plan.npts = b.grid.npts;
    plan_layout(plan, ntot, (int)topo.shells.size(), topo.lmax, xc_radial_cache_on());

    size_t per_frag = fragment_bytes(plan);
    // the charges' part of an embedded gradient: Hermite records and the sites' gradient, from the gradient pool
    if (opts.want_gradient && plan.npc > 0) per_frag += sizeof(double) * (gradpc_record_doubles(topo) + 3 * (size_t)plan.npc);
    // RI-MP2: the transformed tensor and the pair partials, from the stage's own pool
    if (w.mp2_frozen >= 0) per_frag += rimp2_fragment_bytes(plan.n, plan.nocc, plan.naux, w.mp2_frozen);
    // CPHF: first-order densities with their J and K, dipole matrices and the solver's vectors, from the stage's own pool
    if (w.cphf) per_frag += cphf_fragment_bytes(plan.n, plan.nocc, plan.n);
    size_t free_b = 0, total_b = 0;
    (void)hipMemGetInfo(&free_b, &total_b);
    // what the lanes' pools hold is free to this batch (the counters' few hundred bytes are not counted)
    for (const Lane& l : ctx->lane)
        for (int k = 0; k < NPOOL; ++k)
            if (k != POOL_MISC) free_b += l.pool[k].capacity();
    const size_t budget = batch_budget_bytes(free_b, scratch_reservation_bytes(ctx), lane, ctx->hbm_budget_bytes);
    const long chunk = batch_chunk_fragments(budget, per_frag, ntot, lane, ctx->pipeline_chunks, ctx->pipeline_min_fragments);
    if (chunk < 1) return fail(MQC_HIP_ERR_DEVICE, "not enough device memory for one fragment");
    std::vector<Job> jobs;
    for (int start = 0; start < ntot; start += (int)chunk) {
        Job j; j.frag = &b.frags[start]; j.nf = (int)std::min<long>(chunk, ntot - start);
        jobs.push_back(std::move(j));
    }

    int* h_counter = nullptr;
    HIP_CHECK_RET(hipHostMalloc((void**)&h_counter, 256));
    Slot slots[2] = {make_slot(ctx, 0, h_counter), make_slot(ctx, 1, h_counter + 32)};
    auto finish = [&](Slot& sl, Job& job) {
        int r = scf_loop(plan, b, sl, job);
        if (r == MQC_HIP_OK) r = fetch_results(plan, b, sl, job);
        std::vector<double>().swap(job.hx);
        return r;
    };
    const int njobs = (int)jobs.size();
    // chunks that alternate between the lanes: prepare(k + 1) has to return before finish(k) can start, so the integral
    // stage must not keep the host; a single chunk and a lane go from prepare straight into finish, which blocks anyway
    const bool alternating = lane < 0 && njobs > 1;
    if (alternating) { eri_host_may_wait(0, false); eri_host_may_wait(1, false); }
    if (lane >= 0) {
        // one lane only: chunks strictly one after the other
        Slot& sl = slots[lane & 1];
        for (int k = 0; k < njobs && rc == MQC_HIP_OK; ++k)
            if ((rc = prepare(ctx, plan, b, sl, jobs[k])) == MQC_HIP_OK) rc = finish(sl, jobs[k]);
    } else {
        rc = prepare(ctx, plan, b, slots[0], jobs[0]);
        for (int k = 0; k < njobs && rc == MQC_HIP_OK; ++k) {
            // chunk k+1's integrals go onto the other stream before the host starts iterating chunk k
            if (k + 1 < njobs) rc = prepare(ctx, plan, b, slots[(k + 1) & 1], jobs[k + 1]);
            if (rc == MQC_HIP_OK) rc = finish(slots[k & 1], jobs[k]);
        }
    }
    if (alternating) { eri_host_may_wait(0, true); eri_host_may_wait(1, true); }
    if (rc != MQC_HIP_OK) {
        // drain the streams before the error return hands the pools back
        if (lane != 1) (void)hipStreamSynchronize(ctx->lane[0].stream);
        if (lane != 0) (void)hipStreamSynchronize(ctx->lane[1].stream);
    }
    (void)hipHostFree(h_counter);
    if (rc != MQC_HIP_OK) return rc;
    b.stats.t_total += now_s() - t_begin;
    std::lock_guard<std::mutex> lock(ctx->stats_mutex);
    ctx->stats += b.stats;
    if (plan.pcm_stride > 0 && pcm_timing_on()) {
        // the lanes this batch ran on: both (chunks alternate) or its own
        PcmTiming& t = g_pcm_timing;
        double setup_s = 0, iter_s = 0, bytes = 0;
        long launches = 0;
        for (int l = 0; l < 2; ++l) {
            if (lane >= 0 && l != (lane & 1)) continue;
            setup_s += t.setup_s[l]; iter_s += t.iter_s[l]; bytes += t.iter_bytes[l]; launches += t.launches[l];
            t.setup_s[l] = t.iter_s[l] = t.iter_bytes[l] = 0.0; t.launches[l] = 0;
        }
        std::fprintf(stderr, "mqc_hip: pcm timing: %d fragments in %d chunks, stride %d, setup %.3f ms, iterations %.3f ms in %ld launches, %.3f GB read, %.1f GB/s\n",
                     ntot, njobs, plan.pcm_stride, setup_s * 1e3, iter_s * 1e3, launches, bytes * 1e-9, iter_s > 0 ? bytes * 1e-9 / iter_s : 0.0);
    }
    return MQC_HIP_OK;
}

}  // namespace mqc

// =========================================================================================
using namespace mqc;

// ---- superposed free atoms (mqc_libcint_atomic_guess.f90) ---------------------------------------------------------
// Ground-state multiplicity of a free atom by Hund's first rule over the Madelung filling
// (hund_multiplicity, src/core/mqc_atomic_guess_common.f90:19-54).
static int hund_multiplicity(int z)
{
    static const int cap[16] = {2, 2, 6, 2, 6, 2, 10, 6, 2, 10, 6, 2, 14, 10, 6, 2};
    int remaining = z, unpaired = 0;
    for (int i = 0; i < 16 && remaining > 0; ++i) {
        const int deg = cap[i] / 2, in_shell = std::min(remaining, cap[i]);
        remaining -= in_shell;
        unpaired = in_shell <= deg ? in_shell : 2 * deg - in_shell;
    }
    return unpaired + 1;
}

// eigen-decomposition of a small symmetric matrix (cyclic Jacobi, host): a[n*n] -> eigenvalues w, vectors v (columns)
static void host_jacobi(int n, std::vector<double>& a, std::vector<double>& w, std::vector<double>& v)
{
    v.assign((size_t)n * n, 0.0);
    for (int i = 0; i < n; ++i) v[(size_t)i * n + i] = 1.0;
    for (int sweep = 0; sweep < 64; ++sweep) {
        double off = 0.0;
        for (int i = 0; i < n; ++i) for (int j = 0; j < i; ++j) off += a[(size_t)i * n + j] * a[(size_t)i * n + j];
        if (off < 1e-30) break;
        for (int p = 0; p < n; ++p)
            for (int q = p + 1; q < n; ++q) {
                const double apq = a[(size_t)p * n + q];
                if (std::fabs(apq) < 1e-300) continue;
                const double th = (a[(size_t)q * n + q] - a[(size_t)p * n + p]) / (2.0 * apq);
                const double t = (th >= 0 ? 1.0 : -1.0) / (std::fabs(th) + std::sqrt(th * th + 1.0));
                const double c = 1.0 / std::sqrt(t * t + 1.0), sn = t * c;
                for (int k = 0; k < n; ++k) {
                    const double akp = a[(size_t)k * n + p], akq = a[(size_t)k * n + q];
                    a[(size_t)k * n + p] = c * akp - sn * akq; a[(size_t)k * n + q] = sn * akp + c * akq;
                }
                for (int k = 0; k < n; ++k) {
                    const double apk = a[(size_t)p * n + k], aqk = a[(size_t)q * n + k];
                    a[(size_t)p * n + k] = c * apk - sn * aqk; a[(size_t)q * n + k] = sn * apk + c * aqk;
                }
                for (int k = 0; k < n; ++k) {
                    const double vkp = v[(size_t)k * n + p], vkq = v[(size_t)k * n + q];
                    v[(size_t)k * n + p] = c * vkp - sn * vkq; v[(size_t)k * n + q] = sn * vkp + c * vkq;
                }
            }
    }
    w.resize(n);
    for (int i = 0; i < n; ++i) w[i] = a[(size_t)i * n + i];
}

// One free atom per distinct (element, shells): unrestricted Hartree-Fock at Hund's multiplicity in exactly the basis
// functions the atom contributes, GWH start, 1e-8 / 1e-6, 200 cycles (solve_free_atom :380-429) -- run through this
// same engine as a one-atom fragment -- cached for the life of the context; the blocks are dropped on the diagonal
// (build_atomic_guess :295-378; ghosts carry nothing).  SAD: the spherical average of the total density
// (spherical_average :235-293; spherical bases only reach this engine); SAC: the total as converged.
static int build_atomic_guess(mqc_hip_context* ctx, const mqc_hip_molecule_t& mol, const mqc_hip_basis_t& bas, const Topology& topo,
                              int kind, bool with_pseudo_orbitals, AtomicGuess& out, std::string& err)
{
    const int n = topo.nao;
    out.D0.assign((size_t)n * n, 0.0);
    size_t sh0 = 0, pr0 = 0;
    int ao0 = 0;
    for (int a = 0; a < mol.n_atoms; ++a) {
        const int ns = (int)bas.nshell_per_atom[a];
        size_t npr = 0;
        int nao_a = 0;
        for (int k = 0; k < ns; ++k) { npr += bas.shell_nprim[sh0 + k]; nao_a += 2 * bas.shell_l[sh0 + k] + 1; }
        const int z = mol.atomic_numbers[a];
        const bool ghost = mol.ghost && mol.ghost[a];
        if (z > 0 && !ghost && ns > 0) {
            // the key is the element and the very shells of this atom
            std::ostringstream ks;
            ks << z << ':';
            uint64_t h = 1469598103934665603ull;
            auto mix = [&h](const void* p, size_t nb) { const unsigned char* b = (const unsigned char*)p; for (size_t i = 0; i < nb; ++i) { h ^= b[i]; h *= 1099511628211ull; } };
            for (int k = 0; k < ns; ++k) ks << bas.shell_l[sh0 + k] << '.' << bas.shell_nprim[sh0 + k] << ',';
            mix(bas.exponents + pr0, sizeof(double) * npr); mix(bas.coefficients + pr0, sizeof(double) * npr);
            ks << '#' << h;
            auto it = ctx->atom_cache.find(ks.str());
            std::shared_ptr<std::vector<double>> dens;
            if (it != ctx->atom_cache.end()) dens = it->second;
            else {
                const int32_t zz = z; const double origin[3] = {0.0, 0.0, 0.0}; const int64_t nsa = ns;
                mqc_hip_molecule_t am{}; am.n_atoms = 1; am.atomic_numbers = &zz; am.xyz = origin; am.ghost = nullptr;
                am.charge = 0; am.multiplicity = hund_multiplicity(z); am.nelec = z;
                mqc_hip_basis_t ab{}; ab.spherical = 1; ab.n_atoms = 1; ab.nshell_per_atom = &nsa; ab.n_shells = ns;
                ab.shell_l = bas.shell_l + sh0; ab.shell_nprim = bas.shell_nprim + sh0; ab.exponents = bas.exponents + pr0; ab.coefficients = bas.coefficients + pr0;
                mqc_hip_scf_options_t ao; mqc_hip_default_options(&ao);
                ao.unrestricted = 1; ao.guess = MQC_HIP_GUESS_GWH; ao.energy_tol = 1.0e-8; ao.density_tol = 1.0e-6; ao.max_iter = 200;
                ao.use_diis = 1; ao.diis_size = 8; ao.density_fitting = 0; ao.functional[0] = 0; ao.want_gradient = 0;
                dens = std::make_shared<std::vector<double>>((size_t)nao_a * nao_a, 0.0);
                mqc_hip_scf_result_t ar; std::memset(&ar, 0, sizeof(ar));
                ar.density = dens->data();
                const int rc = mqc_hip_scf_run_batch(ctx, 1, &am, &ab, nullptr, &ao, &ar);
                if (rc != MQC_HIP_OK || ar.has_error || ar.scf_status != MQC_HIP_SCF_CONVERGED) {
                    err = "atomic guess: the free atom Z=" + std::to_string(z) + " did not converge (" + std::string(ar.message) + ")";
                    return MQC_HIP_ERR_VALIDATION;
                }
                if (ctx->atom_cache.size() >= 64) { err = "atomic guess: solution cache exhausted"; return MQC_HIP_ERR_VALIDATION; }
                ctx->atom_cache[ks.str()] = dens;
            }
            // this atom's block: as converged (SAC) or averaged over m within each pair of subshells of equal l (SAD)
            std::vector<int> first(ns), ang(ns);
            { int o = 0; for (int k = 0; k < ns; ++k) { first[k] = o; ang[k] = bas.shell_l[sh0 + k]; o += 2 * ang[k] + 1; } }
            const std::vector<double>& d = *dens;
            if (kind == MQC_HIP_GUESS_SAC) {
                for (int i = 0; i < nao_a; ++i) for (int j = 0; j < nao_a; ++j) out.D0[(size_t)(ao0 + i) * n + ao0 + j] = d[(size_t)i * nao_a + j];
            } else {
                for (int ka = 0; ka < ns; ++ka)
                    for (int kb = 0; kb < ns; ++kb) {
                        if (ang[ka] != ang[kb]) continue;
                        const int nc = 2 * ang[ka] + 1;
                        double mean = 0.0;
                        for (int m = 0; m < nc; ++m) mean += d[(size_t)(first[ka] + m) * nao_a + first[kb] + m];
                        mean /= nc;
                        for (int m = 0; m < nc; ++m) out.D0[(size_t)(ao0 + first[ka] + m) * n + ao0 + first[kb] + m] = mean;
                    }
            }
        }
        sh0 += ns; pr0 += npr; ao0 += nao_a;
    }
    if (ao0 != n) { err = "atomic guess: the atoms' basis functions do not add up to the molecule's"; return MQC_HIP_ERR_VALIDATION; }
    out.nmodes = 0;
    out.Cp.assign((size_t)n * n, 0.0);
    if (with_pseudo_orbitals) {
        std::vector<double> a = out.D0, w, v;
        host_jacobi(n, a, w, v);
        for (int i = 0; i < n; ++i) {
            if (!(w[i] > 1.0e-12)) continue;                  // OCCUPATION_FLOOR
            const double sc = std::sqrt(0.5 * w[i]);
            for (int mu = 0; mu < n; ++mu) out.Cp[(size_t)mu * n + out.nmodes] = v[(size_t)mu * n + i] * sc;
            out.nmodes += 1;
        }
        if (out.nmodes == 0) { err = "atomic guess: the guess density carries no occupation"; return MQC_HIP_ERR_VALIDATION; }
    }
    return MQC_HIP_OK;
}

static mqc_hip_context* g_ctx = nullptr;

extern "C" {

int mqc_hip_abi_version(void) { return MQC_HIP_ABI_VERSION; }

const char* mqc_hip_last_error(void) { return last_error_string().c_str(); }

int mqc_hip_backend_available(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n > 0 ? 1 : 0;
}

void mqc_hip_default_options(mqc_hip_scf_options_t* o)
{
    std::memset(o, 0, sizeof(*o));
    o->grid_level = 3;
    o->max_iter = 100;            // src/methods/mqc_method_config.f90:24-29
    o->energy_tol = 1.0e-8;
    o->density_tol = 1.0e-6;
    o->use_diis = 1;
    o->diis_size = 8;
    o->guess = MQC_HIP_GUESS_AUTO;
    o->eri_mode = MQC_HIP_ERI_AUTO;
    o->schwarz_tol = 0.0;
}

// streams, events and tables of a new context on its device; whatever exists when a step fails is the caller's to destroy
static int create_context(mqc_hip_context* ctx)
{
    HIP_CHECK_RET(hipSetDevice(ctx->device));
    HIP_CHECK_RET(hipGetDeviceProperties(&ctx->prop, ctx->device));
    // creation order matters: streams take the 4 hardware queues round-robin, so each lane's main stream and its
    // three side streams land on four different queues
    for (Lane& l : ctx->lane) {
        HIP_CHECK_RET(hipStreamCreate(&l.stream));
        for (hipStream_t& s : l.side) HIP_CHECK_RET(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    }
    for (Lane& l : ctx->lane) for (hipEvent_t& e : l.chain) HIP_CHECK_RET(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    for (int l = 0; l < 2; ++l) eri_set_side_streams(l, ctx->lane[l].side, 3);
    for (Lane& l : ctx->lane)
        for (hipEvent_t* pair : {l.fock, l.xc, l.step, l.eri})
            for (int k = 0; k < 2; ++k) HIP_CHECK_RET(hipEventCreate(&pair[k]));
    std::vector<double> boys;
    build_boys_table(boys);
    HIP_CHECK_RET(hipMalloc((void**)&ctx->d_boys, sizeof(double) * boys.size()));
    HIP_CHECK_RET(hipMemcpy(ctx->d_boys, boys.data(), sizeof(double) * boys.size(), hipMemcpyHostToDevice));
    {
        const double unit[2] = {0.0, 1.0};
        HIP_CHECK_RET(hipMalloc((void**)&ctx->d_unit, sizeof(unit)));
        HIP_CHECK_RET(hipMemcpy(ctx->d_unit, unit, sizeof(unit), hipMemcpyHostToDevice));
    }
    build_c2s_tables(ctx->h_c2s, ctx->c2s_off);
    HIP_CHECK_RET(hipMalloc((void**)&ctx->d_c2s, sizeof(double) * ctx->h_c2s.size()));
    HIP_CHECK_RET(hipMemcpy(ctx->d_c2s, ctx->h_c2s.data(), sizeof(double) * ctx->h_c2s.size(), hipMemcpyHostToDevice));
    return MQC_HIP_OK;
}

// Everything a context holds, complete or not (null handles are skipped): mqc_hip_finalize, and mqc_hip_context_get
// when a device call fails midway
static void destroy_context(mqc_hip_context* ctx)
{
    (void)hipSetDevice(ctx->device);
    for (Lane& l : ctx->lane) if (l.stream) (void)hipStreamSynchronize(l.stream);
    for (Lane& l : ctx->lane) for (hipStream_t s : l.side) if (s) (void)hipStreamSynchronize(s);
    // launcher state bound to this device (side streams, fork/join events, list caches), then every pool:
    // the context's own and the launchers' function-static ones -- a later context_get starts from nothing
    eri_reset_state();
    int1e_reset_state();
    release_all_pools();
    for (Lane& l : ctx->lane) {
        for (hipStream_t s : l.side) if (s) (void)hipStreamDestroy(s);
        for (hipEvent_t* pair : {l.chain, l.fock, l.xc, l.step, l.eri})
            for (int k = 0; k < 2; ++k) if (pair[k]) (void)hipEventDestroy(pair[k]);
    }
    if (ctx->d_unit) (void)hipFree(ctx->d_unit);
    if (ctx->d_boys) (void)hipFree(ctx->d_boys);
    if (ctx->d_c2s) (void)hipFree(ctx->d_c2s);
    for (Lane& l : ctx->lane) if (l.stream) (void)hipStreamDestroy(l.stream);
    delete ctx;
}

int mqc_hip_context_get(int32_t local_rank, mqc_hip_context** out)
{
    if (!out) return fail(MQC_HIP_ERR_VALIDATION, "null context pointer");
    if (g_ctx) { *out = g_ctx; return MQC_HIP_OK; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(MQC_HIP_ERR_NO_DEVICE, "no HIP device is visible: the MI355X backend has no CPU fallback");
    auto* ctx = new mqc_hip_context();
    ctx->device = ((local_rank % ndev) + ndev) % ndev;    // mqc_cuest_context.f90:188
    const int rc = create_context(ctx);
    if (rc != MQC_HIP_OK) { destroy_context(ctx); return rc; }
    if (const char* env = std::getenv("MQC_HIP_HBM_BUDGET_GB")) ctx->hbm_budget_bytes = (size_t)(std::atof(env) * 1024.0 * 1024.0 * 1024.0);
    // Two-stream chunk pipeline: measured on (H2O)64 MBE-2 RHF/cc-pVDZ it does not pay (1 chunk 261 ms,
    // 2: 251 ms, 4: 281 ms, 8: 340 ms per evaluation -- the ERI kernels and the J/K stream each fill the
    // chip, co-running them only slows both), so it is off unless MQC_HIP_PIPELINE_CHUNKS asks for it.
    // Batches that exceed the HBM budget still alternate between the two lanes.
    ctx->pipeline_chunks = std::max(1, env_int("MQC_HIP_PIPELINE_CHUNKS", 1));
    ctx->pipeline_min_fragments = std::max(2, env_int("MQC_HIP_PIPELINE_MIN_FRAGMENTS", ctx->pipeline_min_fragments));
    // MQC_HIP_CONCURRENT_GROUPS=0: topology groups of a batch call run one after the other
    ctx->concurrent_groups = env_int("MQC_HIP_CONCURRENT_GROUPS", 1) != 0;
    g_ctx = ctx;
    *out = ctx;
    return MQC_HIP_OK;
}

int mqc_hip_finalize(void)
{
    if (g_ctx) destroy_context(g_ctx);
    g_ctx = nullptr;
    return MQC_HIP_OK;
}

int mqc_hip_device_name(mqc_hip_context* ctx, char* buf, int32_t len)
{
    if (!ctx || !buf || len <= 0) return fail(MQC_HIP_ERR_VALIDATION, "bad arguments");
    std::snprintf(buf, (size_t)len, "%s (%s, %d CUs)", ctx->prop.name, ctx->prop.gcnArchName, ctx->prop.multiProcessorCount);
    return MQC_HIP_OK;
}

int mqc_hip_get_stats(mqc_hip_context* ctx, mqc_hip_stats_t* st)
{
    if (!ctx || !st) return fail(MQC_HIP_ERR_VALIDATION, "bad arguments");
    std::lock_guard<std::mutex> lock(ctx->stats_mutex);
    st->t_setup = ctx->stats.t_setup; st->t_int1e = ctx->stats.t_int1e; st->t_eri = ctx->stats.t_eri;
    st->t_fock = ctx->stats.t_fock; st->t_scf_step = ctx->stats.t_scf_step; st->t_total = ctx->stats.t_total;
    st->fock_launches = ctx->stats.fock_launches; st->eri_quartets = ctx->stats.eri_quartets;
    st->scf_iterations_total = ctx->stats.scf_iterations_total;
    st->fock_kernel_seconds = ctx->stats.fock_kernel_seconds; st->fock_bytes = ctx->stats.fock_bytes;
    st->eri_kernel_seconds = ctx->stats.eri_kernel_seconds;
    st->xc_kernel_seconds = ctx->stats.xc_kernel_seconds; st->xc_points = ctx->stats.xc_points;
    st->fock_big_launches = ctx->stats.fock_big_launches; st->fock_big_seconds = ctx->stats.fock_big_seconds;
    st->fock_big_bytes = ctx->stats.fock_big_bytes;
    st->xc_flops = ctx->stats.xc_flops; st->scf_step_seconds = ctx->stats.scf_step_seconds;
    st->eri_survivors = ctx->stats.eri_survivors; st->df_flops = ctx->stats.df_flops; st->df_bytes = ctx->stats.df_bytes;
    ctx->stats = Stats();
    return MQC_HIP_OK;
}

static void init_result(mqc_hip_scf_result_t* r)
{
    double* oe = r->orbital_energies; double* dn = r->density; double* gr = r->gradient; double* ob = r->orbital_energies_beta;
    double* em = r->embedding_matrix; double* mq = r->mulliken_charges;
    std::memset(r, 0, sizeof(*r));
    r->orbital_energies = oe; r->density = dn; r->gradient = gr; r->orbital_energies_beta = ob;
    r->embedding_matrix = em; r->mulliken_charges = mq;
    r->scf_status = MQC_HIP_SCF_NOT_RUN;
}

struct BatchExtras {            // what the plain batch entry does not have
    bool embedded_entry = false;
    double* const* site_gradients = nullptr;        // mqc_hip_scf_gradient_embedded_batch
    const double* const* initial_density = nullptr; // mqc_hip_scf_run_batch_restart (either may be NULL)
    double* const* spin_densities_out = nullptr;
    bool mp2 = false;                               // mqc_hip_rimp2_batch: [n] arrays of the caller
    bool frozen_core = false;
    double *e_os = nullptr, *e_ss = nullptr;
    int32_t* mp2_done = nullptr;
    const mqc_hip_pcm_options_t* pcm = nullptr;     // mqc_hip_scf_pcm_batch: the settings (checked) and the [n] outputs
    double* e_pcm = nullptr;
    int32_t* n_tesserae = nullptr;
    const mqc_hip_cphf_options_t* cphf = nullptr;   // mqc_hip_polarizability_batch: the settings (checked) and the [n] outputs
    double* alpha = nullptr;
    int32_t *cphf_iter = nullptr, *alpha_done = nullptr;
};

// frozen-core orbitals of a topology: per real atom 0 for Z <= 2, 1 for Z = 3-10, 5 for Z = 11-18, 9 for Z = 19-36
// (ghost atoms carry basis functions and no core)
static int frozen_core_orbitals(const Topology& topo)
{
    int nfz = 0;
    for (int a = 0; a < topo.natoms; ++a) {
        if (topo.zeff[a] == 0.0) continue;
        const int z = topo.Z[a];
        nfz += z <= 2 ? 0 : z <= 10 ? 1 : z <= 18 ? 5 : 9;
    }
    return nfz;
}

// what a batch entry was called with
struct BatchCall {
    mqc_hip_context* ctx;
    int64_t nfrag;
    const mqc_hip_molecule_t* mols;
    const mqc_hip_basis_t *orbitals, *auxes;
    const mqc_hip_scf_options_t* opts;
    mqc_hip_scf_result_t* results;
    bool fitted() const { return opts->density_fitting && auxes; }
};

// Step 1: the fragments of a call by topology key; one without geometry or basis fails alone
static std::map<std::string, std::vector<int64_t>> group_fragments(const BatchCall& c)
{
    const mqc_hip_molecule_t* mols = c.mols; const mqc_hip_basis_t *orbitals = c.orbitals, *auxes = c.auxes;
    std::map<std::string, std::vector<int64_t>> groups;
    int64_t last = -1;
    std::string last_key;
    std::vector<int64_t>* last_group = nullptr;
    for (int64_t i = 0; i < c.nfrag; ++i) {
        if (!mols[i].atomic_numbers || !mols[i].xyz || mols[i].n_atoms <= 0 || !orbitals[i].shell_l ||
            !orbitals[i].nshell_per_atom || !orbitals[i].shell_nprim || !orbitals[i].exponents || !orbitals[i].coefficients) {
            fill_error(&c.results[i], "fragment has no geometry or basis");
            continue;
        }
        // consecutive fragments that point at the very same element and basis arrays share their key
        const bool same_as_last = last >= 0 && mols[i].n_atoms == mols[last].n_atoms && mols[i].atomic_numbers == mols[last].atomic_numbers &&
                                  mols[i].ghost == mols[last].ghost && mols[i].nelec == mols[last].nelec && mols[i].charge == mols[last].charge &&
                                  mols[i].multiplicity == mols[last].multiplicity && mols[i].n_point_charges == mols[last].n_point_charges && (mols[i].h_extra != nullptr) == (mols[last].h_extra != nullptr) &&
                                  std::memcmp(&orbitals[i], &orbitals[last], sizeof(mqc_hip_basis_t)) == 0 &&
                                  (!c.fitted() || std::memcmp(&auxes[i], &auxes[last], sizeof(mqc_hip_basis_t)) == 0);
        if (!same_as_last) {
            last_key = topology_key(mols[i], orbitals[i]);
            if (c.fitted()) last_key += "//" + topology_key(mols[i], auxes[i]);
            if (mols[i].n_point_charges > 0) last_key += "//pc" + std::to_string(mols[i].n_point_charges);
            if (mols[i].h_extra) last_key += "//hx";
            last_group = &groups[last_key];
        }
        last = i;
        last_group->push_back(i);
    }
    return groups;
}

// the topology of a molecule and basis from the context's cache, or built now and cached
static int cached_topology(mqc_hip_context* ctx, const mqc_hip_molecule_t& mol, const mqc_hip_basis_t& bas, int max_l, bool quartets,
                           std::shared_ptr<Topology>& out, std::string& err)
{
    const std::string k = topology_key(mol, bas) + (quartets ? "|q" : "|n") + std::to_string(max_l);
    auto it = ctx->topo_cache.find(k);
    if (it != ctx->topo_cache.end()) { out = it->second; return MQC_HIP_OK; }
    auto t = std::make_shared<Topology>();
    const int rc = build_topology(mol, bas, *t, err, max_l, quartets);
    if (rc != MQC_HIP_OK) return rc;
    if (ctx->topo_cache.size() >= 16) ctx->topo_cache.clear();
    ctx->topo_cache[k] = t;
    out = t;
    return MQC_HIP_OK;
}

// Step 2: one topology group becomes a Work -- its topologies from the cache (or built now), the entry's refusals, one
// record per fragment that runs, the atomic guess.  Returns MQC_HIP_OK, or the code of what kept a fragment (w.frags
// may still hold the others) or the whole group (w.frags empty) from running, the reason written to their results.
static int admit_group(const BatchCall& c, const BatchExtras& extras, const std::vector<int64_t>& idx, Work& w)
{
    const mqc_hip_molecule_t& mol0 = c.mols[idx[0]];
    const mqc_hip_basis_t& orb0 = c.orbitals[idx[0]];
    auto refuse_group = [&](int code, const std::string& why, const char* prefix = "") {
        for (auto i : idx) fill_error(&c.results[i], prefix + why);
        set_error(why);
        return code;
    };
    std::string err;
    int rc = cached_topology(c.ctx, mol0, orb0, KERNEL_LMAX, !c.fitted(), w.topo, err);
    if (rc != MQC_HIP_OK) return refuse_group(rc, err);
    if (c.fitted() && (rc = cached_topology(c.ctx, mol0, c.auxes[idx[0]], AUX_LMAX, false, w.aux, err)) != MQC_HIP_OK)
        return refuse_group(rc, err, "auxiliary basis: ");
    const bool uhf = runs_unrestricted(*c.opts, w.topo->multiplicity, w.topo->nelec);
    if (extras.mp2) {
        // closed shells only, and at least one active occupied orbital: a refused group runs no SCF
        const int nocc = w.topo->nelec / 2;
        w.mp2_frozen = extras.frozen_core ? frozen_core_orbitals(*w.topo) : 0;
        if (uhf)
            return refuse_group(MQC_HIP_ERR_UNSUPPORTED, "RI-MP2 is built for closed-shell restricted references: unrestricted MP2 (open shells, multiplicity != 1, odd electron counts) is not built");
        if (w.mp2_frozen >= nocc)
            return refuse_group(MQC_HIP_ERR_VALIDATION, "RI-MP2: the frozen core (" + std::to_string(w.mp2_frozen) + " orbitals) leaves no active occupied orbital of " + std::to_string(nocc));
    }
    if (extras.cphf) {
        // closed shells on the in-core path only: a refused group runs no SCF
        if (uhf)
            return refuse_group(MQC_HIP_ERR_UNSUPPORTED, "polarizabilities are built for closed-shell restricted references: the unrestricted CPHF (open shells, multiplicity != 1, odd electron counts) is not built");
        if (!incore_supported(w.topo->nao) || w.topo->nao > 116)
            return refuse_group(MQC_HIP_ERR_UNSUPPORTED, "polarizabilities stream the in-core ERI tensor (n_ao <= 116): a fragment of " + std::to_string(w.topo->nao) + " functions has no tensor to stream");
        w.cphf = extras.cphf;
    }
    w.embedded_entry = extras.embedded_entry;
    // supplied densities: their size follows from the run's spin treatment; one with a non-finite entry fails its own
    // fragment and nothing else
    int worst = MQC_HIP_OK;
    bool all_d0 = extras.initial_density != nullptr;
    const size_t nn = (size_t)w.topo->nao * w.topo->nao, cnt = uhf ? 2 * nn : nn;
    if (extras.pcm) {
        w.pcm_f = (extras.pcm->epsilon - 1.0) / extras.pcm->epsilon;
        w.cavities.reserve(idx.size());
    }
    for (auto i : idx) {
        FragmentIO io{&c.mols[i], &c.results[i]};
        if (extras.pcm) {
            // the cavity of this geometry; a fragment the continuum refuses fails alone
            pcm::Cavity cav;
            std::string why;
            const int prc = pcm_build_cavity(c.mols[i], *extras.pcm, cav, why);
            extras.n_tesserae[i] = cav.count;
            if (prc != MQC_HIP_OK) {
                fill_error(io.result, why);
                set_error(why);
                worst = prc;
                continue;
            }
            w.cavities.push_back(std::move(cav));
            io.cavity = &w.cavities.back();
            io.e_pcm = extras.e_pcm + i;
        }
        if (extras.embedded_entry && extras.site_gradients) io.pcgrad = extras.site_gradients[i];
        if (extras.initial_density) io.d0 = extras.initial_density[i];
        if (extras.spin_densities_out) io.spin_out = extras.spin_densities_out[i];
        if (extras.mp2) { io.mp2_os = extras.e_os + i; io.mp2_ss = extras.e_ss + i; io.mp2_done = extras.mp2_done + i; }
        if (extras.cphf) { io.alpha = extras.alpha + 9 * i; io.cphf_iter = extras.cphf_iter + i; io.alpha_done = extras.alpha_done + i; }
        bool finite = true;
        if (io.d0) for (size_t k = 0; k < cnt && finite; ++k) finite = std::isfinite(io.d0[k]);
        if (!finite) {
            fill_error(io.result, "initial density: a non-finite entry");
            set_error("initial density of fragment " + std::to_string(i) + ": a non-finite entry");
            worst = MQC_HIP_ERR_VALIDATION;
            continue;
        }
        w.frags.push_back(io);
        if (io.d0) w.any_d0 = true; else all_d0 = false;
    }
    if (w.frags.empty()) return worst;
    if ((c.opts->guess == MQC_HIP_GUESS_SAD || c.opts->guess == MQC_HIP_GUESS_SAC) && !all_d0) {
        // the free atoms are solved here, before any group of this call holds the pools (nested one-atom calls)
        w.guess = std::make_shared<AtomicGuess>();
        rc = build_atomic_guess(c.ctx, mol0, orb0, *w.topo, c.opts->guess, c.opts->density_fitting != 0, *w.guess, err);
        if (rc != MQC_HIP_OK) {
            // "a guess that will not build is a reason to start elsewhere, not to fail the run" (:175-178): GWH, loudly
            std::fprintf(stderr, "mqc_hip: initial guess: %s -- falling back to gwh\n", err.c_str());
            w.guess.reset();
        }
    }
    return worst;
}

// Step 3: the groups one after the other, each on both lanes; or, with several groups (monomers and dimers of an MBE
// list), two at a time, each on its own lane: the small group's latency-bound stages hide behind the large one.
static void schedule_groups(mqc_hip_context* ctx, std::vector<Work>& work, const mqc_hip_scf_options_t& opts)
{
    auto run_one = [&](Work& w, int lane) {
        (void)hipSetDevice(ctx->device);
        w.rc = run_batch(ctx, w, opts, lane);
        if (w.rc != MQC_HIP_OK) w.msg = mqc_hip_last_error();      // the error text is thread-local
    };
    if (work.size() < 2 || !ctx->concurrent_groups) {
        for (auto& w : work) run_one(w, -1);
        return;
    }
    // largest group first on lane 0; the others queue up on lane 1, then lane 0 helps with what is left
    std::sort(work.begin(), work.end(), [](const Work& a, const Work& b) { return a.frags.size() > b.frags.size(); });
    // A large group's integral stage wants all four hardware queues: its streams alias pairwise onto the queues of
    // the other lane's streams, and behind the small groups' latency-bound launches (0.1-2.6 ms each) they started
    // 2.6-12 ms late ((H2O)64 MBE-2: 2016 dimers behind 64 monomers, profiles/r04_b_..._task_stream.txt).  So when
    // the largest group has at least DEFER_MIN fragments and every other group holds at most one eighth of its
    // stored integrals (fragments x n_ao^4: a monomer group as numerous as its dimers still is 1/16 of them), the
    // other groups wait -- on the host -- until the large group's first chunk has joined its integral stage; they
    // then run next to its SCF loop, which uses one stream (defer_small_groups, host_setup.cpp).
    // MQC_HIP_DEFER_SMALL_GROUPS_MIN overrides the border; 0: never defer.  The border is
    // ERI_TASK_STREAM_MIN_FRAGMENTS' (kern_eri.hip).
    static const long defer_min = [] { const char* e = std::getenv("MQC_HIP_DEFER_SMALL_GROUPS_MIN"); return e ? std::atol(e) : 1024L; }();
    std::vector<long> group_nfrag;
    std::vector<int> group_nao;
    for (const Work& w : work) { group_nfrag.push_back((long)w.frags.size()); group_nao.push_back(w.topo->nao); }
    const bool defer = defer_small_groups(group_nfrag.data(), group_nao.data(), (int)work.size(), defer_min);
    // The deferred groups then run next to the large group's SCF loop, which is one stream on one hardware queue;
    // lane 1's third side stream shares that queue, and a kernel of the loop waits behind whatever sits there (2.3 ms
    // of the first iteration behind the monomers' one-electron chain and class launches, profiles/r05_e_...).  So a
    // deferring call keeps lane 1 to its other streams, the one-electron chain on the second side stream.
    GroupGate gate;
    if (defer) {
        work[0].opens = &gate;
        for (size_t k = 1; k < work.size(); ++k) work[k].waits = &gate;
        eri_limit_side_streams(1, 2, 1);
        // MQC_HIP_DEFER_SMALL_GROUPS_TRACE=1: one line per deferring call (the tests read it)
        static const bool trace = env_opt_in("MQC_HIP_DEFER_SMALL_GROUPS_TRACE");
        if (trace) std::fprintf(stderr, "mqc_hip: %zu small groups deferred behind a group of %zu fragments\n", work.size() - 1, work[0].frags.size());
    }
    // a deferring call hands the large group to lane 0 itself: lane 1's thread may come first to the counter
    std::atomic<size_t> next{defer ? 1u : 0u};
    auto worker = [&](int lane) {
        for (;;) {
            const size_t k = next.fetch_add(1);
            if (k >= work.size()) return;
            run_one(work[k], lane);
        }
    };
    std::thread t1(worker, 1);
    if (defer) run_one(work[0], 0);
    worker(0);
    t1.join();
    if (defer) eri_limit_side_streams(1, 1 << 20, 2);
}

// Step 4: a group that failed as a whole marks its fragments that carry no reason of their own; the call's status
static int collate(const std::vector<Work>& work, int worst)
{
    for (const Work& w : work) {
        if (w.rc == MQC_HIP_OK) continue;
        worst = w.rc;
        set_error(w.msg);
        for (const FragmentIO& f : w.frags)
            if (!f.result->has_error) fill_error(f.result, w.msg);
    }
    return worst;      // a single-fragment call thus reports the fragment's failure as the call's status, like run_cuest_scf
}

// the body of the batch entries
static int scf_run_batch_impl(mqc_hip_context* ctx, int64_t nfrag, const mqc_hip_molecule_t* mols,
                              const mqc_hip_basis_t* orbitals, const mqc_hip_basis_t* auxes,
                              const mqc_hip_scf_options_t* opts, mqc_hip_scf_result_t* results, const BatchExtras& extras)
{
    if (!ctx) return fail(MQC_HIP_ERR_VALIDATION, "null context (call mqc_hip_context_get first)");
    if (nfrag < 0 || (nfrag > 0 && (!mols || !orbitals || !opts || !results)))
        return fail(MQC_HIP_ERR_VALIDATION, "null argument");
    HIP_CHECK_RET(hipSetDevice(ctx->device));
    for (int64_t i = 0; i < nfrag; ++i) init_result(&results[i]);
    const BatchCall call{ctx, nfrag, mols, orbitals, auxes, opts, results};
    int worst = MQC_HIP_OK;
    std::vector<Work> work;
    for (const auto& kv : group_fragments(call)) {
        Work w;
        const int rc = admit_group(call, extras, kv.second, w);
        if (rc != MQC_HIP_OK) worst = rc;
        if (!w.frags.empty()) work.push_back(std::move(w));
    }
    schedule_groups(ctx, work, *opts);
    return collate(work, worst);
}

int mqc_hip_scf_run_batch(mqc_hip_context* ctx, int64_t nfrag, const mqc_hip_molecule_t* mols,
                          const mqc_hip_basis_t* orbitals, const mqc_hip_basis_t* auxes,
                          const mqc_hip_scf_options_t* opts, mqc_hip_scf_result_t* results)
{
    return scf_run_batch_impl(ctx, nfrag, mols, orbitals, auxes, opts, results, BatchExtras());
}

int mqc_hip_scf_run_batch_restart(mqc_hip_context* ctx, int64_t nfrag, const mqc_hip_molecule_t* mols,
                                  const mqc_hip_basis_t* orbitals, const mqc_hip_basis_t* auxes,
                                  const mqc_hip_scf_options_t* opts, mqc_hip_scf_result_t* results,
                                  const double* const* initial_density, double* const* spin_densities_out)
{
    BatchExtras extras;
    extras.initial_density = initial_density;
    extras.spin_densities_out = spin_densities_out;
    return scf_run_batch_impl(ctx, nfrag, mols, orbitals, auxes, opts, results, extras);
}

int mqc_hip_scf_gradient_embedded_batch(mqc_hip_context* ctx, int64_t nfrag, const mqc_hip_molecule_t* mols,
                                        const mqc_hip_basis_t* orbitals, const mqc_hip_basis_t* auxes,
                                        const mqc_hip_scf_options_t* opts, mqc_hip_scf_result_t* results,
                                        double* const* point_charge_gradients)
{
    if (!opts) return fail(MQC_HIP_ERR_VALIDATION, "null argument");
    if (!point_charge_gradients && mols)
        for (int64_t i = 0; i < nfrag; ++i)
            if (mols[i].n_point_charges > 0)
                return fail(MQC_HIP_ERR_VALIDATION, "point_charge_gradients is NULL but fragment " + std::to_string(i) + " carries point charges");
    mqc_hip_scf_options_t o = *opts;
    o.want_gradient = 1;
    BatchExtras extras;
    extras.embedded_entry = true;
    extras.site_gradients = point_charge_gradients;
    return scf_run_batch_impl(ctx, nfrag, mols, orbitals, auxes, &o, results, extras);
}

int mqc_hip_rimp2_batch(mqc_hip_context* ctx, int64_t nfrag, const mqc_hip_molecule_t* mols,
                        const mqc_hip_basis_t* orbitals, const mqc_hip_basis_t* auxes,
                        const mqc_hip_scf_options_t* opts, mqc_hip_scf_result_t* results,
                        int32_t frozen_core, double* e_os, double* e_ss, int32_t* mp2_done)
{
    if (!opts) return fail(MQC_HIP_ERR_VALIDATION, "null argument");
    if (nfrag > 0 && (!e_os || !e_ss || !mp2_done)) return fail(MQC_HIP_ERR_VALIDATION, "RI-MP2: e_os, e_ss and mp2_done must not be NULL");
    for (int64_t i = 0; i < nfrag; ++i) { e_os[i] = 0.0; e_ss[i] = 0.0; mp2_done[i] = 0; }
    // what the whole call refuses: no fragment runs an SCF
    std::string why;
    if (!opts->density_fitting || !auxes) why = "RI-MP2 uses the fitted tensor of a density-fitted SCF: set density_fitting and pass an auxiliary basis";
    else if (opts->functional[0] != '\0') why = "RI-MP2 on a Kohn-Sham reference: double hybrids are not built";
    else if (opts->unrestricted) why = "RI-MP2 is built for closed-shell restricted references: unrestricted MP2 is not built";
    else if (opts->want_gradient) why = "analytic RI-MP2 gradients are not built (energies only)";
    if (!why.empty()) {
        if (results)
            for (int64_t i = 0; i < nfrag; ++i) { init_result(&results[i]); fill_error(&results[i], why); }
        return fail(MQC_HIP_ERR_UNSUPPORTED, why);
    }
    BatchExtras extras;
    extras.mp2 = true;
    extras.frozen_core = frozen_core != 0;
    extras.e_os = e_os; extras.e_ss = e_ss; extras.mp2_done = mp2_done;
    return scf_run_batch_impl(ctx, nfrag, mols, orbitals, auxes, opts, results, extras);
}

void mqc_hip_default_cphf_options(mqc_hip_cphf_options_t* o)
{
    if (!o) return;
    o->tol = 1.0e-8;
    o->max_iter = 64;
}

int mqc_hip_polarizability_batch(mqc_hip_context* ctx, int64_t nfrag, const mqc_hip_molecule_t* mols, const mqc_hip_basis_t* orbitals,
                                 const mqc_hip_scf_options_t* opts, const mqc_hip_cphf_options_t* cphf, mqc_hip_scf_result_t* results,
                                 double* alpha, int32_t* cphf_iterations, int32_t* alpha_done)
{
    if (!opts || !cphf) return fail(MQC_HIP_ERR_VALIDATION, "null argument");
    if (nfrag > 0 && (!alpha || !cphf_iterations || !alpha_done))
        return fail(MQC_HIP_ERR_VALIDATION, "polarizability: alpha, cphf_iterations and alpha_done must not be NULL");
    for (int64_t i = 0; i < nfrag; ++i) { cphf_iterations[i] = 0; alpha_done[i] = 0; for (int k = 0; k < 9; ++k) alpha[9 * i + k] = 0.0; }
    // what the whole call refuses: no fragment runs an SCF
    std::string why;
    int code = MQC_HIP_ERR_UNSUPPORTED;
    if (!std::isfinite(cphf->tol) || !(cphf->tol > 0.0)) { why = "CPHF: tol must be positive and finite"; code = MQC_HIP_ERR_VALIDATION; }
    else if (cphf->max_iter < 1) { why = "CPHF: max_iter must be at least 1"; code = MQC_HIP_ERR_VALIDATION; }
    else if (opts->density_fitting) why = "polarizabilities stream the exact in-core ERI tensor: the density-fitted CPHF is not built";
    else if (opts->eri_mode == MQC_HIP_ERI_DIRECT) why = "polarizabilities stream the in-core ERI tensor: the direct path (eri_mode = direct) keeps no tensor to stream";
    else if (opts->functional[0] != '\0') why = "polarizabilities of a Kohn-Sham reference (CPKS) need the second derivatives of the XC kernel, which are not built";
    else if (opts->unrestricted) why = "polarizabilities are built for closed-shell restricted references: the unrestricted CPHF is not built";
    else if (opts->want_gradient) why = "polarizability derivatives are not built: the entry takes no want_gradient";
    if (!why.empty()) {
        if (results)
            for (int64_t i = 0; i < nfrag; ++i) { init_result(&results[i]); fill_error(&results[i], why); }
        return fail(code, why);
    }
    mqc_hip_scf_options_t o = *opts;
    o.eri_mode = MQC_HIP_ERI_INCORE;
    BatchExtras extras;
    extras.cphf = cphf; extras.alpha = alpha; extras.cphf_iter = cphf_iterations; extras.alpha_done = alpha_done;
    return scf_run_batch_impl(ctx, nfrag, mols, orbitals, nullptr, &o, results, extras);
}

void mqc_hip_default_pcm_options(mqc_hip_pcm_options_t* p)
{
    if (!p) return;
    p->epsilon = 78.39;          // water
    p->angular_points = 110;
    p->radius_scale = 1.2;
    p->radii_by_z = nullptr;
}

int mqc_hip_scf_pcm_batch(mqc_hip_context* ctx, int64_t nfrag, const mqc_hip_molecule_t* mols,
                          const mqc_hip_basis_t* orbitals, const mqc_hip_basis_t* auxes,
                          const mqc_hip_scf_options_t* opts, const mqc_hip_pcm_options_t* pcm,
                          mqc_hip_scf_result_t* results, double* e_pcm, int32_t* n_tesserae)
{
    if (!opts || !pcm) return fail(MQC_HIP_ERR_VALIDATION, "null argument");
    if (nfrag > 0 && (!e_pcm || !n_tesserae)) return fail(MQC_HIP_ERR_VALIDATION, "PCM: e_pcm and n_tesserae must not be NULL");
    for (int64_t i = 0; i < nfrag; ++i) { e_pcm[i] = 0.0; n_tesserae[i] = 0; }
    // what the whole call refuses: no fragment runs an SCF
    std::string why;
    int code = pcm_check_options(pcm, why);
    if (code == MQC_HIP_OK && opts->want_gradient) {
        why = "analytic gradients in the PCM are not built: the cavity surface is cut sharply and is not differentiable (energies only)";
        code = MQC_HIP_ERR_UNSUPPORTED;
    }
    if (code != MQC_HIP_OK) {
        if (results)
            for (int64_t i = 0; i < nfrag; ++i) { init_result(&results[i]); fill_error(&results[i], why); }
        return fail(code, why);
    }
    BatchExtras extras;
    extras.pcm = pcm; extras.e_pcm = e_pcm; extras.n_tesserae = n_tesserae;
    return scf_run_batch_impl(ctx, nfrag, mols, orbitals, auxes, opts, results, extras);
}

int mqc_hip_scf_run(mqc_hip_context* ctx, const mqc_hip_molecule_t* mol, const mqc_hip_basis_t* orbital,
                    const mqc_hip_basis_t* aux, const mqc_hip_scf_options_t* opts, mqc_hip_scf_result_t* result)
{
    return mqc_hip_scf_run_batch(ctx, 1, mol, orbital, aux, opts, result);
}

}  // extern "C"
