/*
 * mqc_hip.h -- C ABI of libmqc_hip.so, the MI355X (gfx950) SCF engine that drops in
 * behind metalquicha's qc_method_t where the cuEST backend sits today.
 *
 * Boundary being replaced (all paths relative to the reference tree):
 *   run_cuest_scf(settings, fragment, result, want_gradient)
 *       backends/cuest/backend/mqc_cuest_bridge.f90:32-39  (module-level Fortran ABI)
 *       backends/cuest/backend/mqc_cuest_driver.f90:37-276 (what it does)
 *   cuest_backend_available()
 *       backends/cuest/backend/mqc_cuest_bridge.f90:20-30
 *   get_cuest_context / context_create / context_destroy
 *       backends/cuest/backend/mqc_cuest_context.f90:166-306
 * The Fortran shim that binds these (fortran/mqc_hip_bridge.f90, shown in
 * INTEGRATION.md) keeps basis-file parsing and error_t on the Fortran side and hands
 * the engine plain arrays: nothing but pointers, sizes and PODs crosses this header.
 *
 * Conventions
 *   - all floating point is IEEE double; geometry in Bohr, energies in Hartree
 *   - every entry point returns an int status: 0 = ok, never aborts or throws;
 *     mqc_hip_last_error() gives the message for the calling thread's last failure
 *     (the shim turns it into result%error%set(...), mqc_cuest_driver.f90:385-393)
 *   - the caller owns every host array for the duration of the call; the engine owns
 *     all device memory (grow-only pools, released by mqc_hip_finalize), like
 *     device_pool_t in mqc_cuest_context.f90:40-53,142-156
 *   - one calling thread per process (the context is a process-wide singleton,
 *     mqc_cuest_context.f90:134-138); no re-entrancy
 *   - the engine FAILS (MQC_HIP_ERR_NO_DEVICE) when no HIP device is present: there is
 *     no CPU fallback behind this ABI.
 */
#ifndef MQC_HIP_H
#define MQC_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MQC_HIP_ABI_VERSION 3

/* status codes (0 = ok).  VALIDATION mirrors ERROR_VALIDATION, GENERIC mirrors ERROR_GENERIC
 * (src/utils/mqc_error.f90:22-44). */
enum {
    MQC_HIP_OK = 0,
    MQC_HIP_ERR_VALIDATION = 1,
    MQC_HIP_ERR_GENERIC = 2,
    MQC_HIP_ERR_NO_DEVICE = 3,
    MQC_HIP_ERR_UNSUPPORTED = 4,
    MQC_HIP_ERR_DEVICE = 5
};

/* scf_status values, same meaning as the reference's tri-state
 * (backends/cuest/backend/mqc_cuest_driver.f90:219-224). */
enum { MQC_HIP_SCF_NOT_RUN = 0, MQC_HIP_SCF_CONVERGED = 1, MQC_HIP_SCF_NOT_CONVERGED = 2 };

/* initial guess (cuest_scf_settings_t%guess, src/methods/mqc_cuest_iface.f90:104-121).
 * AUTO resolves to GWH, as the cuEST backend does. */
enum { MQC_HIP_GUESS_AUTO = 0, MQC_HIP_GUESS_CORE = 1, MQC_HIP_GUESS_GWH = 2, MQC_HIP_GUESS_SAD = 3,
       MQC_HIP_GUESS_SAC = 4 };   /* AUTO = GWH, as run_cuest_scf's default (mqc_cuest_driver.f90:107-114); SAD / SAC =
                                     superposed free-atom densities, spherically averaged / as converged
                                     (mqc_libcint_atomic_guess.f90:295-378; SAC restricted only) */

/* two-electron path.  AUTO = in-core packed ERIs in HBM when they fit the per-fragment
 * budget, else the direct build (the reference's choice at mqc_libcint_bridge.f90:819-892,
 * with the 2 GB host limit replaced by an HBM budget). */
enum { MQC_HIP_ERI_AUTO = 0, MQC_HIP_ERI_INCORE = 1, MQC_HIP_ERI_DIRECT = 2 };

typedef struct mqc_hip_context mqc_hip_context;   /* opaque, process-wide singleton */

/* physical_fragment_t flattened (src/fragmentation/common/mqc_physical_fragment.f90:45-94) */
typedef struct {
    int32_t n_atoms;
    const int32_t *atomic_numbers;   /* [n_atoms] */
    const double *xyz;               /* [3*n_atoms], atom-major, Bohr */
    const uint8_t *ghost;            /* [n_atoms] or NULL; ghost = basis functions, Z = 0 */
    int32_t charge;
    int32_t multiplicity;
    int32_t nelec;                   /* excludes ghosts */
    /* ABI 3: external point charges -- the embedding field of the FMO / EE-MBE callers
     * (embedding_operator with esp = "ptc", backends/libcint/mqc_libcint_fmo.f90:1077-1160): the operator
     * u = -sum_g q_g / |r - R_g| is added to the one-electron Hamiltonian, exactly as run_libcint_rhf's h_extra
     * (mqc_libcint_rhf.f90:479-484); the charges do NOT enter the nuclear repulsion. */
    int32_t n_point_charges;         /* 0 = none */
    const double *point_charge_xyz;  /* [3*n_point_charges], Bohr */
    const double *point_charges;     /* [n_point_charges] */
    const double *h_extra;           /* [n_ao*n_ao] row-major symmetric, or NULL: any further one-electron operator added to
                                        H as it stands (run_libcint_rhf's h_extra) -- the exact Coulomb field of near
                                        fragments' electrons in FMO (local_coulomb, mqc_libcint_fmo.f90:1337-1406).
                                        Counted in e_embedding and embedding_matrix together with the charges' part. */
} mqc_hip_molecule_t;

/* molecular_basis_type flattened (src/basis/mqc_cgto.f90); RAW Basis-Set-Exchange
 * coefficients of unnormalised primitives -- the engine normalises exactly as
 * backends/libcint/mqc_libcint_integrals.F90:519-555 does. */
typedef struct {
    int32_t spherical;               /* must be 1: Cartesian sets are refused
                                        (mqc_cuest_driver.f90:331-341) */
    int32_t n_atoms;
    const int64_t *nshell_per_atom;  /* [n_atoms] */
    int32_t n_shells;                /* = sum nshell_per_atom */
    const int32_t *shell_l;          /* [n_shells] */
    const int32_t *shell_nprim;      /* [n_shells] */
    const double *exponents;         /* [sum nprim] */
    const double *coefficients;      /* [sum nprim] */
} mqc_hip_basis_t;

/* the subset of cuest_scf_settings_t the engine acts on (mqc_cuest_iface.f90:35-142) */
typedef struct {
    char functional[32];             /* "" = Hartree-Fock */
    int32_t density_fitting;
    int32_t grid_level;              /* 1..5, default 3 */
    int32_t radial_points;           /* 0 = from grid_level */
    int32_t angular_points;          /* 0 = from grid_level */
    int32_t max_iter;                /* default 100 */
    double energy_tol;               /* default 1e-8 */
    double density_tol;              /* default 1e-6 */
    int32_t use_diis;
    int32_t diis_size;               /* default 8 */
    int32_t guess;                   /* MQC_HIP_GUESS_* */
    int32_t unrestricted;            /* force UHF / UKS (open shells take it by themselves, mqc_cuest_driver.f90:127) */
    int32_t want_gradient;           /* analytic gradient into result->gradient: HF and Kohn-Sham, exact ERIs, s-d shells */
    int32_t allow_crap_scf;
    int32_t verbose;
    int32_t eri_mode;                /* MQC_HIP_ERI_* */
    double schwarz_tol;              /* 0 = default 1e-11 (mqc_libcint_direct.f90:61) */
} mqc_hip_scf_options_t;

/* what run_cuest_scf writes into calculation_result_t (mqc_cuest_driver.f90:211-275) */
typedef struct {
    double e_total;                  /* energy%scf */
    double e_electronic;
    double e_nuclear;
    double e_xc;
    int32_t scf_status;              /* MQC_HIP_SCF_* */
    int32_t iterations;
    int32_t n_ao;
    int32_t n_mo;
    int32_t n_occ;
    double homo;                     /* orbital energies, Hartree */
    double lumo;
    int32_t has_orbitals;
    double *orbital_energies;        /* optional out [n_mo capacity >= n_ao] or NULL (alpha spin when unrestricted) */
    double *density;                 /* optional out [n_ao*n_ao] row-major or NULL (total density) */
    int32_t has_error;
    char message[256];
    /* ABI 2 */
    double dipole[3];                /* result%dipole, electron-Bohr, origin = centre of nuclear charge
                                        (system_compute_dipole, mqc_cuest_integrals.f90:1443-1521) */
    int32_t has_dipole;
    double *gradient;                /* optional out [3*n_atoms] atom-major, Hartree/Bohr: result%gradient(3,n_atoms);
                                        filled when opts->want_gradient and the pointer is not NULL */
    int32_t has_gradient;
    double *orbital_energies_beta;   /* optional out [n_ao] or NULL; written by unrestricted runs */
    int32_t n_alpha, n_beta;         /* occupied orbitals per spin (n_occ = n_alpha) */
    double s_squared;                /* <S^2> of the unrestricted determinant, 0 for restricted */
    /* ABI 3 */
    double e_embedding;              /* tr(D u): the part of e_total that is the interaction with the point charges
                                        (inner_scf subtracts it, mqc_libcint_fmo.f90:1992-1997); 0 without charges */
    double *embedding_matrix;        /* optional out [n_ao*n_ao] or NULL: u itself (nmer_term needs tr(D_split u), :1266-1272) */
    double *mulliken_charges;        /* optional out [n_atoms] or NULL: q_A = Z_A - sum_{mu on A} (D S)_mu,mu
                                        (fragment_charges, mqc_libcint_fmo.f90:2001-2021; ghosts carry Z = 0) */
} mqc_hip_scf_result_t;

/* ---- lifecycle -------------------------------------------------------------------- */
/* cuest_backend_available(): 1 if a HIP device is visible, else 0 */
int mqc_hip_backend_available(void);
/* get_cuest_context(): lazy singleton; device = local_rank mod device_count
 * (mqc_cuest_context.f90:188) */
int mqc_hip_context_get(int32_t local_rank, mqc_hip_context **ctx);
int mqc_hip_finalize(void);
const char *mqc_hip_last_error(void);
int mqc_hip_abi_version(void);
void mqc_hip_default_options(mqc_hip_scf_options_t *opts);

/* ---- the hot path ----------------------------------------------------------------- */
/* run_cuest_scf for ONE fragment */
int mqc_hip_scf_run(mqc_hip_context *ctx, const mqc_hip_molecule_t *mol,
                    const mqc_hip_basis_t *orbital, const mqc_hip_basis_t *aux /* NULL unless DF */,
                    const mqc_hip_scf_options_t *opts, mqc_hip_scf_result_t *result);

/* The same for MANY fragments at once (batch-submit API).
 * Fragments are independent (do_fragment_work has no cross-fragment state,
 * src/fragmentation/mbe/mqc_mbe_mpi_fragment_distribution_scheme.F90:156-238); the engine
 * groups them by topology and advances whole groups through each SCF stage in single
 * launches.  Per-fragment failures are reported in results[i] and do not fail the call. */
int mqc_hip_scf_run_batch(mqc_hip_context *ctx, int64_t n_fragments,
                          const mqc_hip_molecule_t *mols, const mqc_hip_basis_t *orbitals,
                          const mqc_hip_basis_t *auxes /* NULL unless DF */,
                          const mqc_hip_scf_options_t *opts, mqc_hip_scf_result_t *results);

/* ---- stage-level entry points (same kernels, used by the parity tests) ------------- */
/* S, T, V (n_ao x n_ao, row-major):  compute_overlap/kinetic/potential,
 * mqc_cuest_integrals.f90:1525-1634 <-> one_electron, mqc_libcint_integrals.F90:843-911 */
int mqc_hip_int1e(mqc_hip_context *ctx, const mqc_hip_molecule_t *mol, const mqc_hip_basis_t *orbital,
                  double *S, double *T, double *V);
/* packed in-core ERI matrix M[pair(i,j)][pair(k,l)], pair(i,j) = i(i+1)/2 + j, i >= j
 * (molecule_eris, mqc_libcint_integrals.F90:1449) */
int mqc_hip_eri_packed(mqc_hip_context *ctx, const mqc_hip_molecule_t *mol, const mqc_hip_basis_t *orbital,
                       double schwarz_tol, double *M /* [npair*npair] */);
/* the same packed matrix for the long-range operator erf(omega r12)/r12, omega > 0 (the K_lr integrals of
 * range-separated hybrids, mqc_libcint_rhf.f90:1045-1065); screened with the Coulomb Schwarz bounds, which bound it */
int mqc_hip_eri_packed_attenuated(mqc_hip_context *ctx, const mqc_hip_molecule_t *mol, const mqc_hip_basis_t *orbital,
                                  double omega, double schwarz_tol, double *M /* [npair*npair] */);
/* J[D], K[D] from the in-core tensor (build_fock, mqc_libcint_rhf.f90:1491-1574) */
int mqc_hip_jk_incore(mqc_hip_context *ctx, const mqc_hip_molecule_t *mol, const mqc_hip_basis_t *orbital,
                      const double *D, double *J, double *K);
/* J[D], K[D] of ONE fragment by the direct (integral-recomputing) build, no tensor (build_fock_direct,
 * mqc_libcint_direct.f90:306-620): the Schwarz bounds, then the digest kernels over the unique shell quartets, n_ao <= 256.
 * schwarz_tol is the density-weighted screen of that build (a quartet is kept iff
 * Q_ab Q_cd deg max(max(Dab, Dcd)/2, (exx/8) max(Dac, Dad, Dbc, Dbd)) >= schwarz_tol; 0 keeps every quartet); exx is the
 * exact-exchange fraction the screen weighs K with.  K is the plain exchange matrix, NOT scaled by exx.  exx = 0 skips the
 * exchange digest: K is then written as all zeros (J is the same as for any other exx, up to the screen). */
int mqc_hip_jk_direct(mqc_hip_context *ctx, const mqc_hip_molecule_t *mol, const mqc_hip_basis_t *orbital,
                      double schwarz_tol, double exx, const double *D, double *J, double *K);
/* symmetric eigen-decomposition by the engine's LDS Jacobi kernel: A (n x n) -> w ascending,
 * V columns = eigenvectors, row-major (diagonalize_fock_device, mqc_cuest_scf.f90:1132-1221) */
/* J[D] for MANY fragments of ONE topology (same elements and basis, n geometries, n densities) in single launches:
 * the batched form of local_coulomb (backends/libcint/mqc_libcint_fmo.f90:1337-1406), where the FMO driver needs the
 * Coulomb operator of a neighbour's density over the supersystem fragment + neighbour for every (fragment, neighbour)
 * pair of a pass.  D and J are [n][n_ao*n_ao] row-major, contiguous; in-core exact ERIs (n_ao <= 116) for the full matrix.
 * n_source_atoms > 0 says that only the LAST n_source_atoms atoms carry density and only the block of J over the
 * other (leading) atoms is wanted -- exactly local_coulomb's use -- so only the shell quartets (leading pair | source
 * pair) are formed -- contracted with the density on the fly by the direct-path digest kernels (Schwarz bound 1e-12,
 * no integral tensor, n_ao <= 256); the rest of J is then not meaningful.  0 = the full Coulomb matrix of the full density. */
int mqc_hip_coulomb_batch(mqc_hip_context *ctx, int64_t n_fragments, const mqc_hip_molecule_t *mols,
                          const mqc_hip_basis_t *orbital, int32_t n_source_atoms, const double *D, double *J);

/* Electrostatic potential of converged (or any) densities at arbitrary points, for MANY fragments of ONE topology:
 *     V(r) = sum_A Z_A / |r - R_A|  -  sum_{mu nu} D_{mu nu} (mu| 1/|r' - r| |nu)          (ghost atoms: Z = 0)
 * the quantity behind ESP maps and potential-fitted (CHELPG) charges.  D is [n][n_ao*n_ao] row-major (symmetric), points
 * is [n][3*max_points] (x, y, z per point, Bohr), esp is [n][max_points].  Point counts may be ragged: n_points[i] <=
 * max_points points of fragment i are used (NULL = max_points each); entries beyond a fragment's count are neither read
 * nor written.  include_nuclei = 0 returns the electronic part alone (minus sign included); a point on a nucleus is
 * then legal.  n_ao <= 256, s-f shells; fragments are processed in chunks sized to the free HBM.
 * MQC_HIP_ERR_VALIDATION: non-finite coordinates, a negative count or one above max_points, a fragment whose elements
 * differ from the first's, or -- with include_nuclei = 1 -- a point within 1e-10 Bohr of a nucleus with Z > 0.
 * max_points = 0 or n_fragments = 0 returns MQC_HIP_OK and writes nothing.  (Added without an ABI bump: no struct changed.) */
int mqc_hip_esp_batch(mqc_hip_context *ctx, int64_t n_fragments, const mqc_hip_molecule_t *mols,
                      const mqc_hip_basis_t *orbital, const double *D /* [n][n_ao*n_ao] */,
                      int32_t max_points, const int32_t *n_points /* [n] or NULL = max_points each */,
                      const double *points /* [n][3*max_points], Bohr */, int32_t include_nuclei,
                      double *esp /* [n][max_points] */);

/* The exchange-correlation quadrature of GIVEN densities, for MANY fragments of ONE topology: what one SCF iteration's
 * quadrature stage computes, alone.  The call takes the plan of an SCF batch of n_fragments with this functional (spin,
 * two-electron path, radial cache, point buffer: the same device layout), builds the grid and the Becke weights, fills the
 * radial cache where the plan has one and runs the SCF driver's own dispatch once.  Per fragment: e_xc, the integrated
 * electron number, and V_xc = A + A^T of the kernels' accumulator A, as the Fock assembly forms it.
 * Restricted: D and V_xc are [n][n_ao*n_ao] (D the total density).  unrestricted != 0: [n][2][n_ao*n_ao], alpha then beta
 * (spin densities C_s C_s^T, not doubled); an open-shell molecule needs unrestricted != 0.  Range-separated functionals:
 * the semi-local grid part only (K_lr belongs to the J/K stage).  The accumulator is poisoned before the launch and its
 * neighbours in the pool are compared before and after (MQC_HIP_ERR_DEVICE when the quadrature wrote outside).
 * Refused with the SCF's own codes: whatever an SCF of these settings refuses (n_ao > 256, meta-GGA or unrestricted
 * above 140, more than 64 atoms, unknown functional); MQC_HIP_ERR_VALIDATION: null pointers, n_fragments < 1, a
 * functional without a grid part, fragments of different elements.  (Added without an ABI bump: no struct changed.) */
int mqc_hip_xc_batch(mqc_hip_context *ctx, int64_t n_fragments, const mqc_hip_molecule_t *mols,
                     const mqc_hip_basis_t *orbital, const char *functional, int32_t grid_level, int32_t unrestricted,
                     const double *D, double *e_xc /* [n] */, double *n_electrons /* [n] */, double *V_xc);

/* The density-fitted J/K stage on GIVEN tensors, for n_fragments of one shape: what one SCF iteration's J/K stage
 * computes, alone.  No molecule: the kernels read the sizes, exx, D, C and the fitted tensor only.
 *     B [n][n_aux][npair]   the fitted tensor, packed pairs (mu >= nu, index mu (mu + 1) / 2 + nu) fastest
 *     D [n][n_ao*n_ao]      the (symmetric) density
 *     C [n][n_ao*n_ao]      row-major, columns are orbitals, the first n_occ are occupied
 *     J, K [n][n_ao*n_ao]   J = sum_P B_P tr(B_P D), K = 2 sum_P (B_P C_occ)(B_P C_occ)^T
 * The arrays are those of a density-fitted SCF batch of this shape and the SCF driver's own dispatch runs once over all
 * fragments; route (route_len bytes, NUL-terminated) receives the kernel it chose: wave<NTC,NLW>, mfma<JMAX,NLD,K|J> or
 * v1<NV,lds|global>.  J and K are poisoned before the launch and their neighbours in the pool are compared before and
 * after (MQC_HIP_ERR_DEVICE when the stage wrote outside).  exx = 0 (a pure functional) specifies J only; K then holds
 * zeros on the mfma route (its J-only instance) and the plain exchange on the v1 route.
 * MQC_HIP_ERR_VALIDATION: null pointers, n_fragments < 1, n_ao outside 1..140, n_occ outside 1..n_ao, n_aux < 1, exx
 * negative or not finite.  (Added without an ABI bump: no struct changed.) */
int mqc_hip_df_jk_batch(mqc_hip_context *ctx, int64_t n_fragments, int32_t n_ao, int32_t n_occ, int32_t n_aux, double exx,
                        const double *B, const double *D, const double *C, double *J, double *K,
                        char *route, int32_t route_len);

/* The layout of the in-core tensor an SCF batch of n_fragments fragments of n_ao functions gets (host only, no device
 * call): triangular = 1 for the triangular block layout (block t = [pair row npair-1-t | pair row t], each padded with
 * zeros to the end of its last row of the packed triangle, diagonal elements halved), block_doubles its block length (0
 * for the square), stride_doubles the doubles per fragment (npair^2, or (npair + 1) / 2 blocks).
 * MQC_HIP_ERR_VALIDATION: null pointers, n_ao or n_fragments < 1.  (Added without an ABI bump: no struct changed.) */
int mqc_hip_jk_tensor_layout(int32_t n_ao, int64_t n_fragments, int32_t unrestricted, int32_t *triangular,
                             int64_t *block_doubles, int64_t *stride_doubles);

/* The in-core J/K stage on GIVEN tensors, for n_fragments of one shape: what one SCF iteration's J/K stream computes,
 * alone.  No molecule: the kernels read the sizes, the tensor, D and the fragment states only.
 *     tensor [n][stride]     the pair matrix as stored, stride and layout as mqc_hip_jk_tensor_layout reports them
 *     D [n][n_ao*n_ao]       the (symmetric) density
 *     done [n] or NULL       non-zero: the fragment is marked finished and the launch is made with only_active set
 *     J, K [n][n_ao*n_ao]    J_ij = sum_kl (ij|kl) D_kl, K_ik = sum_jl (ij|kl) D_jl
 *     loaded [n]             chunks of 128 doubles the triangular kernel read per fragment (-1: the plan has no counter,
 *                            or the fragment was finished and one workgroup per fragment ran)
 * n_shells > 0 adds the zero-row screening of the triangular kernel: shell_l [n_shells] (2l + 1 functions each, n_ao in
 * all, n_ao <= 64), Q [n][n_shells*n_shells] and q_thresh; a pair row whose shell pair has Q times the fragment's
 * largest Q below q_thresh must be all zeros as stored, and is neither loaded nor contracted.
 * The arrays are those of an in-core SCF batch of this shape (plain or unrestricted; unrestricted runs the alpha view)
 * and the SCF driver's own dispatch runs once over all fragments; route (route_len bytes, NUL-terminated) receives the
 * kernel it chose -- wave<KCH,lds|global,NW,MAXU,reg|mem[,full8]>, rowcoop<2,8> or tri<12,10> -- and grid_x the x extent
 * of its grid.  J and K are poisoned before the launch and their neighbours in the pool are compared before and after
 * (MQC_HIP_ERR_DEVICE when the stage wrote outside).  The launchers zero K -- and with several workgroups per fragment
 * on the triangle J too -- for the WHOLE batch: an element of a finished fragment comes back as the poison or as zero.
 * MQC_HIP_ERR_VALIDATION: null pointers, n_fragments < 1, n_ao < 1 or beyond the in-core limit (116), a stride that is
 * not the layout's, shell_l that does not add up to n_ao, screening with n_ao > 64.
 * (Added without an ABI bump: no struct changed.) */
int mqc_hip_jk_incore_batch(mqc_hip_context *ctx, int64_t n_fragments, int32_t n_ao, int32_t unrestricted,
                            const double *tensor, int64_t stride, const double *D, const int32_t *done /* or NULL */,
                            int32_t n_shells /* 0: no screening */, const int32_t *shell_l, const double *Q, double q_thresh,
                            double *J, double *K, int32_t *loaded /* [n] */, char *route, int32_t route_len,
                            int32_t *grid_x);

/* The build of the fitted tensor alone, for MANY fragments of ONE topology: the integral half and the fit half of a
 * density-fitted SCF's build stage, with the metric copied out between them (the factor overwrites it in place).
 *     A3 [n][n_aux][npair]       (P|mu nu)
 *     metric [n][n_aux*n_aux]    (P|Q), both triangles
 *     B [n][n_aux][npair]        the fitted tensor: L^-1 A3 (Cholesky) or J^-1/2 A3 (eigen path, eigenvalues above 1e-10)
 *     fit_flag [n]               0: Cholesky, 2: eigen path (a near-singular metric), 1: the fit failed
 * The three arrays are poisoned first: an element no task covers reads as NaN.  Refused as a density-fitted SCF refuses:
 * n_ao > 140, orbital shells above f, a Cartesian basis; MQC_HIP_ERR_VALIDATION: null pointers, n_fragments < 1,
 * fragments of different elements.  (Added without an ABI bump: no struct changed.) */
int mqc_hip_df_fit_batch(mqc_hip_context *ctx, int64_t n_fragments, const mqc_hip_molecule_t *mols,
                         const mqc_hip_basis_t *orbital, const mqc_hip_basis_t *aux, double *A3, double *metric,
                         double *B, double *fit_flag /* [n] */);

/* Analytic gradients of fragments EMBEDDED IN POINT CHARGES (FMO / EE-MBE / QM-MM callers): mqc_hip_scf_run_batch with
 * opts->want_gradient forced on -- grouping by topology, chunking and per-fragment failures in results[i] as there -- and
 * two outputs per fragment, both exact derivatives of the e_total the engine reports (which contains tr(D u) and does NOT
 * contain the nuclei-charge term sum Z_A q_g / R_Ag: the charges stay out of E_nuc, so that term and its derivative are the
 * caller's):
 *     results[i].gradient          [3*n_atoms]          d e_total / d R_A, the charges held fixed
 *     point_charge_gradients[i]    [3*n_point_charges]  d e_total / d R_g, index 3*g + c
 * Fragments with n_point_charges = 0 get the plain gradient and their pointer entry is ignored; a NULL array is legal when
 * no fragment carries charges (MQC_HIP_ERR_VALIDATION otherwise); a NULL entry for a fragment that has charges skips its
 * site gradient only.  A fragment with h_extra != NULL is refused with MQC_HIP_ERR_UNSUPPORTED (the engine does not know
 * that operator's derivative), and every refusal of a plain gradient applies unchanged: meta-GGA and range-separated
 * functionals, g shells, density fitting above n_ao = 140.  mqc_hip_scf_run_batch keeps refusing want_gradient with
 * charges: its result record has no slot for the second output.  (Added without an ABI bump: no struct changed.) */
int mqc_hip_scf_gradient_embedded_batch(mqc_hip_context *ctx, int64_t n_fragments, const mqc_hip_molecule_t *mols,
                                        const mqc_hip_basis_t *orbitals, const mqc_hip_basis_t *auxes /* NULL unless DF */,
                                        const mqc_hip_scf_options_t *opts, mqc_hip_scf_result_t *results,
                                        double *const *point_charge_gradients /* [n_fragments]; entry i -> [3*n_point_charges_i] or NULL */);

/* mqc_hip_scf_run_batch started from SUPPLIED DENSITIES: the previous step of a trajectory, the previous pass of an FMO
 * loop, the block-diagonal sum of two monomers for their dimer.  Grouping by topology, chunking under
 * MQC_HIP_HBM_BUDGET_GB, concurrent groups, per-fragment failures in results[i] and every refusal are those of
 * mqc_hip_scf_run_batch; so is the convergence test (a converged result needs more than one iteration, so a restart
 * from an already converged density takes exactly 2).
 *     initial_density[i]      NULL: fragment i starts from opts->guess and gives what mqc_hip_scf_run_batch gives.
 *                             Otherwise row-major [n_ao*n_ao], the TOTAL density, when the fragment runs restricted, and
 *                             [2][n_ao*n_ao], alpha then beta (C_s C_s^T, not doubled), when it runs unrestricted.  Which
 *                             one is decided as everywhere: unrestricted iff opts->unrestricted, multiplicity != 1 or an
 *                             odd electron count -- the expected size follows from that decision, not from the caller.
 *     spin_densities_out[i]   NULL, or [2][n_ao*n_ao]: the converged alpha and beta densities of an unrestricted run
 *                             (results[i].density stays the total density); restricted runs write nothing there.
 * Either array may be NULL; with both NULL the call is mqc_hip_scf_run_batch.
 * The density need not be good.  It is projected on the device onto the nearest SCF state of THIS geometry: the
 * generalised eigenproblem of -S D0s S (D0s = D0 symmetrised) in the metric S yields D0's natural orbitals, the n_occ
 * most occupied ones are filled (per spin in an unrestricted run), and the run starts from their idempotent density and
 * orbitals.  A wrong trace, a density that is not idempotent in the new overlap, all zeros: all legal.  A density
 * that already is an SCF state of this overlap is reproduced.  A non-finite entry gives MQC_HIP_ERR_VALIDATION, reported in
 * that fragment's record only (the other fragments of the call run).  A group in which every fragment brings a density
 * skips the free-atom solves of the SAD / SAC guesses.  (Added without an ABI bump: no struct changed.) */
int mqc_hip_scf_run_batch_restart(mqc_hip_context *ctx, int64_t n_fragments, const mqc_hip_molecule_t *mols,
                                  const mqc_hip_basis_t *orbitals, const mqc_hip_basis_t *auxes /* NULL unless DF */,
                                  const mqc_hip_scf_options_t *opts, mqc_hip_scf_result_t *results,
                                  const double *const *initial_density /* NULL, or [n_fragments]; entry i NULL or -> density */,
                                  double *const *spin_densities_out /* NULL, or [n_fragments]; entry i NULL or -> [2][n_ao*n_ao] */);

/* RI-MP2 correlation energies on top of a density-fitted closed-shell Hartree-Fock batch.  The SCF part IS
 * mqc_hip_scf_run_batch -- grouping by topology, chunking under MQC_HIP_HBM_BUDGET_GB, deferred groups, per-fragment
 * failures in results[i], results[i].e_total the SCF energy -- and after the SCF loop of a chunk, while its fitted
 * tensor B^P_(mu nu), orbitals and orbital energies are still on the device, the stage of kern_mp2.hip forms
 *     (ia|jb) = sum_P B^P_ia B^P_jb,   e_os = sum (ia|jb)^2 / D,   e_ss = sum (ia|jb) [(ia|jb) - (ib|ja)] / D,
 *     D = e_i + e_j - e_a - e_b,       E_corr = e_os + e_ss        (SCS-MP2: 6/5 e_os + 1/3 e_ss)
 * over the active occupied (i, j) and the virtual (a, b) orbitals of every fragment whose SCF converged:
 *     mp2_done[i] = 1 and e_os[i], e_ss[i] written;  every other fragment gets mp2_done[i] = 0, e_os[i] = e_ss[i] = 0.
 * frozen_core != 0 freezes, per atom, 0 orbitals for Z <= 2, 1 for Z = 3-10, 5 for Z = 11-18, 9 for Z = 19-36 (ghost
 * atoms none): the lowest orbitals of the fragment stay out of the sums.  Point charges and h_extra are legal: the
 * orbitals carry the field.
 * MQC_HIP_ERR_UNSUPPORTED (the refused fragments run no SCF): no density fitting (RI-MP2 uses the fitted tensor of a
 * density-fitted SCF), a functional (double hybrids are not built), an unrestricted run (opts->unrestricted, multiplicity
 * != 1, an odd electron count), want_gradient.  MQC_HIP_ERR_VALIDATION: a NULL output array, a frozen core that leaves no
 * active occupied orbital.  Whatever the density-fitted SCF refuses (n_ao > 140, g shells) keeps its own refusal.
 * (Added without an ABI bump: no struct changed.) */
int mqc_hip_rimp2_batch(mqc_hip_context *ctx, int64_t n_fragments, const mqc_hip_molecule_t *mols,
                        const mqc_hip_basis_t *orbitals, const mqc_hip_basis_t *auxes,
                        const mqc_hip_scf_options_t *opts, mqc_hip_scf_result_t *results,
                        int32_t frozen_core,
                        double *e_os /* [n] */, double *e_ss /* [n] */, int32_t *mp2_done /* [n] */);

/* The RI-MP2 stage on GIVEN tensors, for n_fragments of one shape: what mqc_hip_rimp2_batch runs after the SCF loop of a
 * chunk (the three kernels of kern_mp2.hip, once), alone.  No molecule: the kernels read the sizes, the fitted tensor,
 * the orbitals, their energies and the fragment states only.
 *     B [n][n_aux][npair]     the fitted tensor, packed pairs (mu >= nu, index mu (mu + 1) / 2 + nu) fastest
 *     C [n][n_ao*n_ao]        row-major, columns are orbitals: n_frozen frozen, then the active occupied ones up to n_occ,
 *                             then the virtuals up to nmo; columns beyond nmo are not orbitals and are never read into a result
 *     eps [n][n_ao]           orbital energies
 *     nmo [n], runs [n]       kept orbitals of each fragment; runs = 0 marks a fragment whose SCF is not finished.  The entry
 *                             writes the state {done or iterating, 0, nmo, converged} from them; a fragment with runs = 0 or
 *                             nmo < n_occ gets zeros, as in the batch entry
 *     e [n][2]                e_os, e_ss
 *     part [n][npairs][2]     the partial of every pair i >= j (pair index i (i + 1) / 2 + j over the n_occ - n_frozen active
 *                             orbitals) before the reduction, weight 1 or 2 included
 *     Bia (or NULL)           [n][n_occ - n_frozen][napad][nvpad] the transformed tensor WITH its padding: napad = n_aux
 *                             rounded up to 4, nvpad = n_ao - n_occ rounded up to 16 (route[6], route[7])
 *     route [16]              0: C in LDS (1) or from L2 (0); 1: pairs of a row prefetched per lane (NPF, 0: none); 2: waves per
 *                             workgroup of the transform; 3: occupied orbitals per pass; 4: workgroups per fragment; 5: dynamic
 *                             LDS bytes; 6: napad; 7: nvpad; 8: npairs; 9: passes over the occupied orbitals; 10: auxiliary
 *                             rows the busiest wave walks (padding rows included); 11: times the launcher narrowed the pass to
 *                             make the transform fit the LDS; 12-15: zero
 * workgroups_per_fragment = 0 leaves the transform's grid to the launcher (as the batch entry does); a positive value may
 * only LOWER the workgroups per fragment: it reproduces with a few fragments the rows per wave of a batch of thousands.
 * e, part and Bia are filled with NaN first, and the stage's device arrays and the roundings between and behind them are
 * poisoned before the launch: an element the kernels read without having written it shows as NaN.  The roundings are
 * compared across the launch (MQC_HIP_ERR_DEVICE when the stage wrote outside its arrays).
 * ctx = NULL runs no device code and reads none of the arrays (all may be NULL): route alone is written, the launcher's
 * decision for this shape and n_fragments.  n_occ = n_ao (no virtual orbital): zeros, route[7] = 0.
 * MQC_HIP_ERR_VALIDATION: null pointers, n_fragments < 1, n_ao outside 1..140, n_occ outside 1..n_ao, n_frozen outside
 * 0..n_occ-1, n_aux < 1, workgroups_per_fragment < 0, nmo[i] outside 0..n_ao.  (Added without an ABI bump: no struct changed.) */
#define MQC_HIP_RIMP2_ROUTE_LEN 16
int mqc_hip_rimp2_stage(mqc_hip_context *ctx, int64_t n_fragments, int32_t n_ao, int32_t n_occ, int32_t n_aux,
                        int32_t n_frozen, int32_t workgroups_per_fragment, const double *B, const double *C,
                        const double *eps, const int32_t *nmo, const int32_t *runs, double *e, double *part,
                        double *Bia /* or NULL */, int32_t *route /* [MQC_HIP_RIMP2_ROUTE_LEN] */);

/* ---- static dipole polarizabilities (CPHF) ---------------------------------------------- */
/* Settings of the coupled-perturbed Hartree-Fock solve: a fragment is converged when the largest element, over the three
 * directions, of the residual Delta o U + G(U) + b is at most tol; max_iter bounds its conjugate-gradient iterations. */
typedef struct {
    double tol;                      /* > 0 and finite; default 1e-8 */
    int32_t max_iter;                /* >= 1; default 64 */
} mqc_hip_cphf_options_t;
void mqc_hip_default_cphf_options(mqc_hip_cphf_options_t *o);   /* 1e-8, 64 */

/* Static dipole polarizabilities of closed-shell Hartree-Fock fragments.  The SCF part IS mqc_hip_scf_run_batch --
 * grouping by topology, chunking under MQC_HIP_HBM_BUDGET_GB, deferred groups, per-fragment failures in results[i],
 * results[i] unchanged in meaning -- on the in-core path with the SQUARE tensor at every batch size (the chunks are sized
 * for it), and after the SCF loop of a chunk, while its tensor, orbitals C and energies e are still on the device, the
 * stage of kern_cphf.hip solves, per direction d = x, y, z with H(F) = H + sum_d F_d r_d (r_d the electron position
 * integrals about the coordinate origin), b = C_v^T r_d C_o and Delta_ai = e_a - e_i,
 *     Delta o U + G(U) = -b,   G(U) = C_v^T [J(D1) - K(D1)/2] C_o,   D1 = 2 (C_v U C_o^T + C_o U^T C_v^T),
 *     alpha_cd = -d2E / dF_c dF_d = -tr(D1_d r_c)                      (atomic units, the laboratory frame)
 * by conjugate gradients preconditioned with 1/Delta; the three directions of all fragments of the chunk advance
 * together, one three-density J/K launch per iteration (MQC_HIP_CPHF_MULTI=0: three single-density launches), finished
 * fragments skipped.  For every fragment whose SCF converged and whose solve converged:
 *     alpha_done[i] = 1, alpha[9 i + 3 c + d] written, cphf_iterations[i] = its iterations;
 * every other fragment gets alpha_done[i] = 0 and zeros.  A solve that meets a direction with p.Ap <= 0 ends that
 * fragment with "the RHF solution is unstable" in results[i]; one that reaches max_iter ends it with an error naming the
 * CPHF; the other fragments are unaffected.  Point charges and h_extra are legal: the orbitals carry the field.
 * MQC_HIP_ERR_UNSUPPORTED (the refused fragments run no SCF): density fitting, eri_mode = direct or n_ao > 116 (no
 * tensor to stream), a functional (CPKS needs the second derivatives of the XC kernel), an unrestricted run
 * (opts->unrestricted, multiplicity != 1, an odd electron count), want_gradient.  MQC_HIP_ERR_VALIDATION: a NULL cphf or
 * output array, tol <= 0 or not finite, max_iter < 1.  The plain entry's own refusals keep their text.
 * (Added without an ABI bump: no struct changed.) */
int mqc_hip_polarizability_batch(mqc_hip_context *ctx, int64_t n_fragments, const mqc_hip_molecule_t *mols,
                                 const mqc_hip_basis_t *orbitals, const mqc_hip_scf_options_t *opts,
                                 const mqc_hip_cphf_options_t *cphf, mqc_hip_scf_result_t *results,
                                 double *alpha /* [n][9], row-major */, int32_t *cphf_iterations /* [n] */,
                                 int32_t *alpha_done /* [n] */);

/* The multi-density J/K stage of a CPHF iteration alone, on given SQUARE tensors [n_fragments][npair*npair] (packed
 * pairs mu >= nu, index mu (mu + 1) / 2 + nu) and n_densities = 1..3 symmetric densities per fragment
 * D [n_fragments][n_densities][n_ao*n_ao]: J and K in the layout of D from ONE pass over the tensor (MQC_HIP_CPHF_MULTI=0:
 * one launch of the single-density stream per density).  J and K are poisoned (NaN) before the launch; an element of a
 * fragment marked finished (done[f] != 0; done may be NULL) comes back as the poison or as zero, never as anything
 * else; the pool bytes next to J and K are compared before and after.  route receives the instance chosen:
 * "multi<3,KCH,lds|global,lds|mem,NW,MAXU>" (K accumulated in LDS or global memory, packed densities in LDS or memory,
 * waves per workgroup, register chunks of a row), or "single:" and the single-density instance.
 * MQC_HIP_ERR_VALIDATION: null pointers, n_fragments < 1, n_ao outside 1..116, n_densities outside 1..3.
 * (Added without an ABI bump: no struct changed.) */
int mqc_hip_jk_multi_batch(mqc_hip_context *ctx, int64_t n_fragments, int32_t n_ao, int32_t n_densities,
                           const double *tensor, const double *D, const int32_t *done, double *J, double *K,
                           char *route, int32_t route_len);

/* ---- C-PCM implicit solvation -------------------------------------------------------- */
/* The SCF in a conductor-like polarisable continuum (the reference's cuestPCMPotentialCompute term: "C-PCM charges +
 * V_pcm", F = H + J - K + V_xc + V_pcm, mqc_cuest_integrals.f90:974-1366).  The discretisation is this engine's own
 * (DESIGN.md section 9), no parity with the reference's closed library is claimed:
 *   spheres    one per real (non-ghost) atom, radius = radius_scale x Bondi radius (H 1.20, He 1.40, Li 1.82, C 1.70,
 *              N 1.55, O 1.52, F 1.47, Ne 1.54, Na 2.27, Mg 1.73, Si 2.10, P 1.80, S 1.80, Cl 1.75, Ar 1.88 Angstrom), or
 *              radii_by_z[Z] where that is non-zero (Bohr, NOT scaled)
 *   tesserae   the Lebedev rule of angular_points points on every sphere, s = R_I + rho_I u_k, a = 4 pi rho_I^2 w_k
 *              (sum w = 1), kept iff |s - R_J| >= rho_J for every other real atom J; ordered by atom, then by the rule
 *   cavity     S_ii = zeta_i sqrt(2/pi), S_ij = erf(zeta_ij r_ij)/r_ij, zeta_i = 4.90/sqrt(a_i),
 *              zeta_ij = zeta_i zeta_j / sqrt(zeta_i^2 + zeta_j^2)
 *   response   v_i = sum_A Z_A/|s_i - R_A| - sum D_mn (m| 1/|r - s_i| |n),  q = -f S^-1 v,  f = (epsilon - 1)/epsilon,
 *              E_pcm = q.v / 2,  (V_pcm)_mn = -sum_i q_i (m| 1/|r - s_i| |n)   (the same for both spins)
 *   energy     1/2 tr D (H + F0) + E_xc + E_pcm + E_nuc, F0 the Fock matrix without V_xc and V_pcm
 * The surface cut is sharp: energies only. */
#define MQC_HIP_PCM_RADII_LEN 119
typedef struct {
    double epsilon;                  /* dielectric constant, >= 1 and finite; 1 is the vacuum */
    int32_t angular_points;          /* a Lebedev rule of the engine up to 590 points; default 110 */
    double radius_scale;             /* default 1.2 */
    const double *radii_by_z;        /* NULL, or [MQC_HIP_PCM_RADII_LEN] indexed by atomic number: Bohr, unscaled, 0 = built-in */
} mqc_hip_pcm_options_t;
void mqc_hip_default_pcm_options(mqc_hip_pcm_options_t *pcm);   /* epsilon 78.39 (water), 110 points, scale 1.2, no table */

/* mqc_hip_scf_run_batch in the continuum: grouping by topology, chunking under MQC_HIP_HBM_BUDGET_GB, concurrent
 * groups, the blocked SCF loop and per-fragment failures in results[i] as there; every two-electron path, restricted and
 * unrestricted, Hartree-Fock and every functional of the plain entry, ghost atoms (basis functions, no sphere, no charge).
 * results[i].e_total and e_electronic contain E_pcm (the convergence test sees it, as it sees E_xc); e_xc stays the XC
 * energy.  e_pcm[i] = E_pcm and n_tesserae[i] = T of fragment i; e_pcm[i] = 0 for a fragment that failed.
 * MQC_HIP_ERR_UNSUPPORTED: opts->want_gradient (the cut surface is not differentiable), a fragment that carries point
 * charges or h_extra.  MQC_HIP_ERR_VALIDATION: epsilon < 1 or not finite, an angular_points that is no rule of the engine
 * up to 590, an element without a radius, a NULL pcm / e_pcm / n_tesserae; per fragment: more than 4096 tesserae, a cavity
 * matrix that could not be factorised.  (Added without an ABI bump: no struct changed.) */
int mqc_hip_scf_pcm_batch(mqc_hip_context *ctx, int64_t n_fragments, const mqc_hip_molecule_t *mols,
                          const mqc_hip_basis_t *orbitals, const mqc_hip_basis_t *auxes /* NULL unless DF */,
                          const mqc_hip_scf_options_t *opts, const mqc_hip_pcm_options_t *pcm,
                          mqc_hip_scf_result_t *results, double *e_pcm /* [n] */, int32_t *n_tesserae /* [n] */);

/* The PCM stage of ONE fragment for a GIVEN total density D [n_ao*n_ao] (symmetric): the setup and one iteration's
 * kernels of the SCF entry, with everything in between copied out.  n_tesserae receives T; arrays the caller passes as
 * NULL are skipped; the others must hold at least
 *     tesserae [3*T], areas [T], v [T], q [T]      -- tessera_capacity >= T
 *     A [T*npair], packed pairs (mu >= nu, index mu (mu + 1) / 2 + nu) fastest -- a_capacity (doubles) >= T*npair
 *     e_pcm [1], V_pcm [n_ao*n_ao]
 * MQC_HIP_ERR_VALIDATION when a capacity is too small (n_tesserae is still written), plus the entry's own refusals above. */
int mqc_hip_pcm_stage(mqc_hip_context *ctx, const mqc_hip_molecule_t *mol, const mqc_hip_basis_t *orbital,
                      const mqc_hip_pcm_options_t *pcm, const double *D, int32_t tessera_capacity, int64_t a_capacity,
                      int32_t *n_tesserae, double *tesserae, double *areas, double *A, double *v, double *q,
                      double *e_pcm, double *V_pcm);

/* The gradient stage of ONE fragment on the CALLER'S densities: the device terms of the analytic gradient, each returned
 * on its own -- never summed with each other or with E_nuc' (kern_grad.hip: grad_weighted_density_kernel, grad1e_kernel,
 * eri_grad_kernel, the screening kernels).  Nothing has to be converged; the matrices are row-major.
 *   inputs    D [n*n] (total density; the alpha density when D_beta is given), D_beta [n*n] or NULL, C [n*n] (AO x MO),
 *             eps [n], n_occ (n_alpha when unrestricted); C_beta, eps_beta, n_beta when unrestricted; exx
 *   w         [n*n] the energy-weighted density occ sum_i eps_i C_i C_i^T
 *   g1e       [natoms*3] sum D (T' + V') - W S' over all shell pairs; g1e_pair: the same for the one pair of shells
 *             (pair_a, pair_b), or NULL
 *   g2e       [natoms*3] the exact two-electron term over every class list; with Q [nshell*nshell] (Schwarz bounds) it is
 *             the screened route with threshold q_thresh instead
 *   rows      per-row mode, row_count > 0: the slice [row_start, row_start + row_count) of the list of class
 *             (la lb|lc ld) = row_class, exactly as the topology holds it (mode 0), or of the lists of the density-fitted
 *             term (mode 1: (A B|P -), orbital A >= B, auxiliary P, class (la lb|lp 0); mode 2: (P -|Q -), auxiliary
 *             P >= Q, class (lp 0|lq 0)) with Gamma from gam ([naux][n*n] or [naux][naux]) and the auxiliary basis aux.
 *             rows [row_count*4] receives the rows, class_length the length of the list, g_rows [row_count][natoms*3]
 *             one launch's result per row; g_rows NULL: rows and class_length only, no device work for them.
 * Outputs passed as NULL are not computed.  Refusals (MQC_HIP_ERR_VALIDATION, nothing written): null arguments, a shell
 * or a class with l > 3, a class the topology does not have, a slice outside the list, a shell pair that does not exist,
 * occupations outside 0..n_ao, non-finite input.  (Added without an ABI bump: no existing struct changed.) */
typedef struct {
    const double *D, *D_beta, *C, *eps, *C_beta, *eps_beta;
    int32_t n_occ, n_beta;
    double exx;
    double *w, *g1e, *g1e_pair, *g2e;
    int32_t pair_a, pair_b;
    const double *Q;
    double q_thresh;
    int32_t mode;              /* 0 exact, 1 three-centre, 2 two-centre */
    int32_t row_class[4];
    int64_t row_start, row_count;
    const double *gam;
    int32_t *rows;
    int64_t *class_length;
    double *g_rows;
} mqc_hip_gradient_stage_t;
int mqc_hip_gradient_stage(mqc_hip_context *ctx, const mqc_hip_molecule_t *mol, const mqc_hip_basis_t *orbital,
                           const mqc_hip_basis_t *aux /* NULL unless mode 1 or 2 */, const mqc_hip_gradient_stage_t *args);

int mqc_hip_syev(mqc_hip_context *ctx, int32_t n, const double *A, double *w, double *V);
/* DIIS coefficients from an age-ordered overlap matrix, the device routine's algorithm
 * (diis_coefficients/solve_diis, src/methods/mqc_diis.f90:164-273) */
int mqc_hip_diis_coefficients(mqc_hip_context *ctx, int32_t n_stored, const double *overlap /* [n*n] */,
                              double *coefficients /* [n_stored] */, int32_t *ok);

/* ---- introspection ----------------------------------------------------------------- */
typedef struct {
    double t_setup, t_int1e, t_eri, t_fock, t_scf_step, t_total;   /* seconds, last batch call */
    int64_t fock_launches, eri_quartets, scf_iterations_total;
    double fock_kernel_seconds;   /* HIP-event time of the in-core J/K kernel, last batch */
    double fock_bytes;            /* algorithmic bytes it streamed */
    double eri_kernel_seconds;
    double xc_kernel_seconds;     /* HIP-event time of the XC quadrature kernel, last batch */
    double xc_points;             /* grid points it integrated (fragments x points, summed over launches) */
    /* the same three J/K figures restricted to launches that streamed >= 1 GiB (the dominant kernel of a large batch) */
    int64_t fock_big_launches;
    double fock_big_seconds, fock_big_bytes;
    /* ABI 2 */
    double xc_flops;              /* 8 P n^2 per GGA launch (4 P n^2 LDA), summed: SURVEY.md section 8d's algorithmic count */
    double scf_step_seconds;      /* HIP-event time of the per-iteration SCF-step kernel */
    int64_t eri_survivors;        /* shell quartets the integral stage actually formed (Schwarz survivors, shared blocks once) */
    double df_flops, df_bytes;    /* DF J/K: 4 n^2 A (1 + o) flop and 8 n^2 A bytes per fragment-iteration, summed */
} mqc_hip_stats_t;
int mqc_hip_get_stats(mqc_hip_context *ctx, mqc_hip_stats_t *stats);
int mqc_hip_device_name(mqc_hip_context *ctx, char *buf, int32_t len);

#ifdef __cplusplus
}
#endif
#endif /* MQC_HIP_H */
