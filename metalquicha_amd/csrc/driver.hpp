// driver.hpp -- what the batch driver (engine.cpp) and the stage-level entry points (stage_entries.cpp) share.
// Declarations only; everything here is defined in engine.cpp.
#pragma once
#include "engine.hpp"
#include "pcm_cavity.hpp"
#include <condition_variable>
#include <mutex>

namespace mqc {

// the HIP error a stage left behind, as the call's failure
int stage_check(const char* stage);

// A lane of the context as the stages of one chunk see it (mqc_hip_context::Lane: stream, pools, events), with its
// index and the pinned word the SCF loop reads its counter into
using Lane = mqc_hip_context::Lane;
struct Slot {
    int id;
    Lane* lane;
    int* h_counter;
};
inline Slot make_slot(mqc_hip_context* ctx, int id, int* h_counter) { return {id, &ctx->lane[id], h_counter}; }
// carve one chunk's arrays out of the slot's pools (carve_chunk) and upload the block table of a triangular tensor
int carve_slot(mqc_hip_context* ctx, const Slot& sl, const BatchPlan& plan, const TopologyDev& td, int nfrag, BatchView& bv,
               PcmView* pcm = nullptr);
int upload_topology(mqc_hip_context* ctx, const Topology& topo, TopologyDev& td, DevicePool* pool = nullptr, hipStream_t stream = nullptr);

bool incore_supported(int n);
// The decisions of a batch call of ntot fragments that do not wait for the grid: functional, spin, two-electron path,
// Schwarz thresholds; then the refusals of validate_options
int plan_batch(const mqc_hip_scf_options_t& o, const Topology& topo, int ntot, BatchPlan& p, std::string& msg);

// Starting density of the superposed-atom guesses (one per topology: it does not depend on the geometry) and, for
// the density-fitted exchange, its pseudo-orbitals v_i sqrt(n_i / 2) (density_pseudo_orbitals, mqc_libcint_rhf.f90:1413-1462)
struct AtomicGuess {
    std::vector<double> D0;      // [n*n] total density, block-diagonal over the atoms
    std::vector<double> Cp;      // [n*n] row-major, nmodes columns used
    int nmodes = 0;
};

// A batch call that defers its small topology groups (schedule_groups): the largest group's batch opens the gate
// once its first chunk's integrals are done, the other groups' batches wait at it before they enqueue anything.  Host
// side only: a wait packet in a hardware queue would hold up the large group's own streams that share that queue.
struct GroupGate {
    std::mutex m;
    std::condition_variable cv;
    bool is_open = false;
    void open() { { std::lock_guard<std::mutex> lock(m); is_open = true; } cv.notify_all(); }
    void wait() { std::unique_lock<std::mutex> lock(m); cv.wait(lock, [this] { return is_open; }); }
};

// One fragment of a batch call: what the caller gave and where its answers go
struct FragmentIO {
    const mqc_hip_molecule_t* mol;     // geometry (mol->xyz), point charges, h_extra
    mqc_hip_scf_result_t* result;
    double* pcgrad;                    // mqc_hip_scf_gradient_embedded_batch: the sites' gradient, or null
    const double* d0;                  // mqc_hip_scf_run_batch_restart: starting density (null: opts.guess)
    double* spin_out;                  // mqc_hip_scf_run_batch_restart: where an unrestricted run's spin densities go, or null
    double *mp2_os, *mp2_ss;           // mqc_hip_rimp2_batch: where the opposite-spin and same-spin correlation energies
    int32_t* mp2_done;                 // and the done flag go
    const pcm::Cavity* cavity;         // mqc_hip_scf_pcm_batch: the fragment's tesserae, and where E_pcm goes
    double* e_pcm;
    double* alpha;                     // mqc_hip_polarizability_batch: where the tensor [9], the iterations of the solve
    int32_t *cphf_iter, *alpha_done;   // and the done flag go
};

// What the stages of one batch call share besides the plan: the fragments, ordered by compactness, the device topology
// and grid, and the statistics, gathered locally (two lanes may run at once) and merged at the end
struct Batch {
    const Topology& topo;
    const Topology* aux;
    const mqc_hip_scf_options_t& opts;
    const AtomicGuess* guess;
    std::vector<FragmentIO> frags;
    bool embedded_entry = false;                     // the call came through mqc_hip_scf_gradient_embedded_batch
    bool any_d0 = false;                             // some fragment brought a starting density
    int mp2_frozen = -1;                             // mqc_hip_rimp2_batch only: the frozen orbitals of this topology (>= 0)
    double pcm_f = -1.0;                             // mqc_hip_scf_pcm_batch only: (epsilon - 1) / epsilon (>= 0)
    const mqc_hip_cphf_options_t* cphf = nullptr;    // mqc_hip_polarizability_batch only: the settings of the solve
    TopologyDev td{}, tdx{};
    GridDev grid;
    Stats stats;
    GroupGate* gate = nullptr;                       // opened when the first chunk's integral stage has been joined (scf_loop)
    int chain_side = 2;                              // side stream of the one-electron chain (prepare)
};

// C-PCM, host side (host_setup.cpp, the one place that instantiates pcm_cavity.hpp's builders).  The refusals of the
// settings themselves (MQC_HIP_ERR_VALIDATION: epsilon, the rule) and of a molecule in the continuum (UNSUPPORTED: point
// charges, h_extra; VALIDATION: an element without a radius, too many tesserae), then its cavity
int pcm_check_options(const mqc_hip_pcm_options_t* pcm, std::string& msg);
int pcm_build_cavity(const mqc_hip_molecule_t& mol, const mqc_hip_pcm_options_t& pcm, pcm::Cavity& cav, std::string& msg);

// radial cache of the quadrature: MQC_HIP_XC_RADIAL_CACHE=0 turns it off
bool xc_radial_cache_on();
// exchange-correlation: per-element grid templates and the per-topology point list
int upload_grid(mqc_hip_context* ctx, Batch& b, DevicePool& pool, hipStream_t s);

// The integral stage of lane `slot` uses its first `count` side streams only, and charges the one-electron chain of the
// chunk (prepare) to side stream `chain_side` (kern_eri.hip).  Set between calls of the stage, never inside one.
void eri_limit_side_streams(int slot, int count, int chain_side);
// Whether the host may wait inside the integral stage of lane `slot` until its launches are handed out (the dispatcher of
// launch_eri, kern_eri.hip): true unless the host has another chunk's SCF loop to run meanwhile.  Default: true.
void eri_host_may_wait(int slot, bool yes);

}  // namespace mqc
