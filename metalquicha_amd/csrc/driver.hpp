// driver.hpp -- what the batch driver (engine.cpp) and the stage-level entry points (stage_entries.cpp) share.
// Declarations only; everything here is defined in engine.cpp.
#pragma once
#include "engine.hpp"
#include <condition_variable>
#include <mutex>

namespace mqc {

// the HIP error a stage left behind, as the call's failure
int stage_check(const char* stage);

// One pipeline slot: a stream with its own pools and events.  While the SCF loop of chunk k runs on
// one slot, the integrals of chunk k+1 are formed on the other (compute-bound ERI kernels fill the
// gaps the HBM-bound J/K stream and the per-iteration host round trip leave).
struct Slot {
    int id;
    hipStream_t s;
    DevicePool* pool[NPOOL];          // indexed by POOL_*
    hipEvent_t e0, e1, e2, e3, q0, q1, s0, s1;
    int* h_counter;
};
Slot make_slot(mqc_hip_context* ctx, int id, int* h_counter);
// carve one chunk's arrays out of the slot's pools (carve_chunk) and upload the block table of a triangular tensor
int carve_slot(mqc_hip_context* ctx, const Slot& sl, const BatchPlan& plan, const TopologyDev& td, int nfrag, BatchView& bv);
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

// A batch call that defers its small topology groups (scf_run_batch_impl): the largest group's batch opens the gate
// once its first chunk's integrals are done, the other groups' batches wait at it before they enqueue anything.  Host
// side only: a wait packet in a hardware queue would hold up the large group's own streams that share that queue.
struct GroupGate {
    std::mutex m;
    std::condition_variable cv;
    bool is_open = false;
    void open() { { std::lock_guard<std::mutex> lock(m); is_open = true; } cv.notify_all(); }
    void wait() { std::unique_lock<std::mutex> lock(m); cv.wait(lock, [this] { return is_open; }); }
};

// What the stages of one batch call share besides the plan: the inputs, ordered by compactness, the device topology
// and grid, and the statistics, gathered locally (two lanes may run at once) and merged at the end
struct Batch {
    const Topology& topo;
    const Topology* aux;
    const mqc_hip_scf_options_t& opts;
    const AtomicGuess* guess;
    std::vector<const double*> xyz;
    std::vector<mqc_hip_scf_result_t*> results;
    std::vector<const mqc_hip_molecule_t*> mols;     // embedded groups only (point charges, h_extra)
    std::vector<double*> pcgrad;                     // mqc_hip_scf_gradient_embedded_batch only: the callers' site gradients (or null)
    // mqc_hip_scf_run_batch_restart only: the callers' starting densities (null entry: opts.guess) and where an
    // unrestricted run's spin densities go (null entry: nowhere); empty when the call brought none
    std::vector<const double*> d0;
    std::vector<double*> spin_out;
    // mqc_hip_rimp2_batch only (mp2_frozen >= 0: the frozen orbitals of this topology): where each fragment's
    // opposite-spin and same-spin correlation energies and its done flag go
    int mp2_frozen = -1;
    std::vector<double*> mp2_os, mp2_ss;
    std::vector<int32_t*> mp2_done;
    TopologyDev td{}, tdx{};
    GridDev grid;
    Stats stats;
    GroupGate* gate = nullptr;                       // opened when the first chunk's integral stage has been joined (scf_loop)
    int chain_side = 2;                              // side stream of the one-electron chain (prepare)
};

// radial cache of the quadrature: MQC_HIP_XC_RADIAL_CACHE=0 turns it off
bool xc_radial_cache_on();
// exchange-correlation: per-element grid templates and the per-topology point list
int upload_grid(mqc_hip_context* ctx, Batch& b, DevicePool& pool, hipStream_t s);


// The integral stage of `slot` uses its first `count` side streams only, and charges the one-electron chain of the
// chunk (prepare) to side stream `chain_side` (kern_eri.hip).  Set between calls of the stage, never inside one.
void eri_limit_side_streams(int slot, int count, int chain_side);
// Whether the host may wait inside the integral stage of `slot` until its launches are handed out (the dispatcher of
// launch_eri, kern_eri.hip): true unless the host has another chunk's SCF loop to run meanwhile.  Default: true.
void eri_host_may_wait(int slot, bool yes);

}  // namespace mqc
