"""Method layer: the host-side mirror of the reference's L3 boundary for the SCF hot path.

  PhysicalFragment    <- physical_fragment_t   (src/fragmentation/common/mqc_physical_fragment.f90:45-94)
  ScfSettings         <- cuest_scf_settings_t  (src/methods/mqc_cuest_iface.f90:35-142)
  CalculationResult   <- calculation_result_t  (src/core/mqc_result_types.f90:92-196), the fields
                         run_cuest_scf fills (backends/cuest/backend/mqc_cuest_driver.f90:211-275)
  run_hip_scf         <- run_cuest_scf         (backends/cuest/backend/mqc_cuest_bridge.f90:32-39)
  hip_backend_available <- cuest_backend_available (:20-30)
  HFMethod.calc_energy  <- hf_calc_energy / hf_run (src/methods/mqc_method_hf.F90:113-217)
  run_hip_scf_batch   <- the batch-submit entry the worker loop would use; with
                         initial_densities it goes through mqc_hip_scf_run_batch_restart (no counterpart)
  run_hip_embedded_gradients <- (no counterpart) gradients of fragments in point charges, on atoms and on the charges
                         (mqc_hip_scf_gradient_embedded_batch)
  run_hip_esp         <- (no counterpart) the potential of converged densities at arbitrary points (mqc_hip_esp_batch)
  run_hip_rimp2_batch, run_hip_rimp2_groups <- (no counterpart: the reference's MP2 is conventional) density-fitted RHF
                         and the RI-MP2 correlation energy of every converged fragment (mqc_hip_rimp2_batch)
  CphfSettings, run_hip_polarizability_batch, run_hip_polarizability_groups <- (no counterpart) closed-shell RHF on the
                         in-core path and the static dipole polarizability of every converged fragment by a batched
                         CPHF solve (mqc_hip_polarizability_batch)
  PcmSettings, run_hip_scf_pcm_batch, run_hip_scf_pcm_groups <- the SCF with cuestPCMPotentialCompute's term ("C-PCM
                         charges + V_pcm", mqc_cuest_integrals.f90:974-1366), this engine's own discretisation
                         (mqc_hip_scf_pcm_batch)

Same names, argument meaning and error behaviour; the numerics all happen in libmqc_hip.so.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import List, Optional, Sequence

import numpy as np

from . import capi
from .basis import ANGSTROM_TO_BOHR, FlatBasis, build_flat_basis, BasisError, SYMBOL_TO_Z

SCF_NOT_RUN, SCF_CONVERGED, SCF_NOT_CONVERGED = capi.SCF_NOT_RUN, capi.SCF_CONVERGED, capi.SCF_NOT_CONVERGED
BACKEND_AUTO, BACKEND_HIP, BACKEND_LIBCINT = 0, 1, 2


def parse_backend_name(name: str) -> int:
    """auto|hip|gpu|cuest -> this engine; libcint|cpu -> the CPU backend (not part of this repo).
    Mirrors parse_backend_name, src/methods/mqc_cuest_iface.f90:146-180."""
    n = (name or "auto").strip().lower()
    if n in ("auto",):
        return BACKEND_AUTO
    if n in ("hip", "gpu", "cuest", "mi355x"):
        return BACKEND_HIP
    if n in ("libcint", "cpu"):
        return BACKEND_LIBCINT
    raise ValueError("unknown backend '%s'" % name)


@dataclass
class PhysicalFragment:
    element_numbers: np.ndarray           # (n_atoms,) int
    coordinates: np.ndarray               # (3, n_atoms) Bohr, column per atom like the reference
    charge: int = 0
    multiplicity: int = 1
    ghost: Optional[np.ndarray] = None    # (n_atoms,) bool
    nelec: Optional[int] = None

    def __post_init__(self):
        self.element_numbers = np.asarray(self.element_numbers, dtype=np.int32)
        self.coordinates = np.asarray(self.coordinates, dtype=np.float64)
        if self.coordinates.shape != (3, len(self.element_numbers)):
            raise ValueError("coordinates must be (3, n_atoms) in Bohr")
        if self.ghost is not None:
            self.ghost = np.asarray(self.ghost, dtype=bool)
        if self.nelec is None:
            real = self.element_numbers if self.ghost is None else self.element_numbers[~self.ghost]
            self.nelec = int(np.sum(real)) - int(self.charge)     # compute_nelec, :73-83

    @property
    def n_atoms(self) -> int:
        return int(len(self.element_numbers))

    @classmethod
    def from_angstrom(cls, symbols: Sequence[str], xyz_angstrom, **kw) -> "PhysicalFragment":
        z = [SYMBOL_TO_Z[s.lower()] for s in symbols]
        xyz = np.asarray(xyz_angstrom, dtype=np.float64).reshape(-1, 3) * ANGSTROM_TO_BOHR
        return cls(np.array(z), xyz.T.copy(), **kw)


@dataclass
class ScfSettings:
    basis_set: str = "sto-3g"
    aux_basis_set: str = "def2-universal-jkfit"
    density_fitting: bool = False
    functional: str = ""
    spherical: bool = True
    verbose: bool = False
    guess: str = "auto"
    device_rank: int = 0
    unrestricted: bool = False
    allow_crap_scf: bool = False
    max_iter: int = 100
    energy_tol: float = 1.0e-8
    density_tol: float = 1.0e-6
    use_diis: bool = True
    diis_size: int = 8
    grid_level: int = 3
    radial_points: int = 0
    angular_points: int = 0
    backend: int = BACKEND_AUTO
    schwarz_tol: float = 0.0
    eri_mode: str = "auto"          # auto | incore | direct


@dataclass
class EnergyT:
    scf: float = 0.0
    mp2_os: float = 0.0        # opposite-spin and same-spin parts of the RI-MP2 correlation energy (run_hip_rimp2_batch)
    mp2_ss: float = 0.0
    pcm: float = 0.0           # E_pcm = q.v / 2 of a run in the continuum (run_hip_scf_pcm_batch); already part of scf

    @property
    def mp2(self) -> float:
        return self.mp2_os + self.mp2_ss

    def total(self) -> float:
        return self.scf + self.mp2


@dataclass
class PcmSettings:
    """C-PCM implicit solvation (mqc_hip_pcm_options_t): the dielectric constant (1 = vacuum), the Lebedev rule on
    every atomic sphere, the scale of the built-in Bondi radii, and optionally the caller's own radii by atomic number
    (Bohr, unscaled; a dict {Z: radius} or an array indexed by Z, 0 = built-in)."""
    epsilon: float = 78.39
    angular_points: int = 110
    radius_scale: float = 1.2
    radii_by_z: Optional[object] = None

    def radii_table(self) -> Optional[np.ndarray]:
        if self.radii_by_z is None:
            return None
        table = np.zeros(capi.PCM_RADII_LEN)
        if isinstance(self.radii_by_z, dict):
            for z, r in self.radii_by_z.items():
                table[int(z)] = float(r)
        else:
            given = np.asarray(self.radii_by_z, dtype=np.float64).reshape(-1)
            table[:min(len(given), len(table))] = given[:len(table)]
        return table

    def options(self, keep: list) -> capi.PcmOptions:
        """The C struct; `keep` receives the array it points into."""
        o = capi.PcmOptions()
        o.epsilon = float(self.epsilon); o.angular_points = int(self.angular_points); o.radius_scale = float(self.radius_scale)
        table = self.radii_table()
        if table is not None:
            keep.append(table)
            o.radii_by_z = capi.dptr(table)
        return o


@dataclass
class CphfSettings:
    """The coupled-perturbed Hartree-Fock solve (mqc_hip_cphf_options_t): a fragment is converged when the largest
    element of its residual, over the three field directions, is at most `tol`; `max_iter` bounds the iterations."""
    tol: float = 1.0e-8
    max_iter: int = 64

    def options(self) -> capi.CphfOptions:
        o = capi.CphfOptions()
        o.tol = float(self.tol); o.max_iter = int(self.max_iter)
        return o


@dataclass
class CalculationResult:
    energy: EnergyT = field(default_factory=EnergyT)
    has_energy: bool = False
    has_mp2: bool = False
    scf_status: int = SCF_NOT_RUN
    scf_iterations: int = 0
    homo: float = 0.0
    lumo: float = 0.0
    has_orbitals: bool = False
    has_error: bool = False
    error_code: int = 0
    error_message: str = ""
    distance: float = 0.0
    e_nuclear: float = 0.0
    e_electronic: float = 0.0
    orbital_energies: Optional[np.ndarray] = None
    dipole: Optional[np.ndarray] = None     # (3,) electron-Bohr, origin = centre of nuclear charge
    has_dipole: bool = False
    gradient: Optional[np.ndarray] = None   # (3, n_atoms) Hartree/Bohr, like result%gradient
    has_gradient: bool = False
    s_squared: float = 0.0
    orbital_energies_beta: Optional[np.ndarray] = None
    n_alpha: int = 0
    n_beta: int = 0
    hessian: Optional[np.ndarray] = None               # (3 n_atoms, 3 n_atoms) Hartree/Bohr^2, atom-major like result%hessian
    has_hessian: bool = False
    dipole_derivatives: Optional[np.ndarray] = None    # (3, 3 n_atoms) d mu / d R
    has_dipole_derivatives: bool = False
    # filled by the restart path (run_hip_scf_batch / run_hip_scf with starting densities): what the next start needs
    density: Optional[np.ndarray] = None               # (n_ao, n_ao) total density
    spin_densities: Optional[np.ndarray] = None        # (2, n_ao, n_ao) alpha, beta: unrestricted runs only
    # filled by run_hip_polarizability_batch
    polarizability: Optional[np.ndarray] = None        # (3, 3) static dipole polarizability, atomic units, laboratory frame
    has_polarizability: bool = False
    cphf_iterations: int = 0


DEFAULT_DISPLACEMENT = 0.005         # Bohr, src/core/mqc_calculation_defaults.f90:13

_GUESS = {"auto": capi.GUESS_AUTO, "gwh": capi.GUESS_GWH, "core": capi.GUESS_CORE, "sad": capi.GUESS_SAD, "sac": capi.GUESS_SAC}


def hip_backend_available() -> bool:
    try:
        return bool(capi.load_library().mqc_hip_backend_available())
    except capi.HipBackendError:
        return False


def _options(settings: ScfSettings, want_gradient: bool) -> capi.ScfOptions:
    o = capi.default_options()
    o.functional = settings.functional.encode()[:31]
    o.density_fitting = int(settings.density_fitting)
    o.grid_level = settings.grid_level
    o.radial_points = settings.radial_points
    o.angular_points = settings.angular_points
    o.max_iter = settings.max_iter
    o.energy_tol = settings.energy_tol
    o.density_tol = settings.density_tol
    o.use_diis = int(settings.use_diis)
    o.diis_size = settings.diis_size
    g = settings.guess.strip().lower()
    if g not in _GUESS:
        # the cuEST path refuses guesses it does not implement rather than running another one
        raise capi.HipBackendError(capi.ERR_UNSUPPORTED, "initial guess '%s' is not available on the HIP backend "
                                                         "(core, gwh, auto, sad, sac)" % settings.guess)
    o.guess = _GUESS[g]
    o.unrestricted = int(settings.unrestricted)
    o.want_gradient = int(want_gradient)
    o.allow_crap_scf = int(settings.allow_crap_scf)
    o.verbose = int(settings.verbose)
    o.schwarz_tol = settings.schwarz_tol
    o.eri_mode = {"auto": capi.ERI_AUTO, "incore": capi.ERI_INCORE, "direct": capi.ERI_DIRECT}[settings.eri_mode.lower()]
    return o


class _Marshalled:
    """Keeps the numpy arrays alive for as long as the C structs that point into them."""

    def __init__(self, fragment: PhysicalFragment, fb: FlatBasis, aux: Optional[FlatBasis] = None):
        self.z = np.ascontiguousarray(fragment.element_numbers, dtype=np.int32)
        self.xyz = np.ascontiguousarray(fragment.coordinates.T, dtype=np.float64)   # atom-major
        self.ghost = None if fragment.ghost is None else np.ascontiguousarray(fragment.ghost, dtype=np.uint8)
        self.fb = fb
        self.mol = capi.Molecule(fragment.n_atoms, self.z.ctypes.data_as(capi.c_int32_p), capi.dptr(self.xyz),
                                 None if self.ghost is None else self.ghost.ctypes.data_as(capi.c_uint8_p),
                                 int(fragment.charge), int(fragment.multiplicity), int(fragment.nelec))
        self.bas = capi.Basis(1 if fb.spherical else 0, fragment.n_atoms,
                              fb.nshell_per_atom.ctypes.data_as(capi.c_int64_p), fb.nshell,
                              fb.shell_l.ctypes.data_as(capi.c_int32_p), fb.shell_nprim.ctypes.data_as(capi.c_int32_p),
                              capi.dptr(fb.exps), capi.dptr(fb.coefs))
        self.aux = aux
        self.aux_bas = None
        if aux is not None:
            self.aux_bas = capi.Basis(1 if aux.spherical else 0, fragment.n_atoms,
                                      aux.nshell_per_atom.ctypes.data_as(capi.c_int64_p), aux.nshell,
                                      aux.shell_l.ctypes.data_as(capi.c_int32_p), aux.shell_nprim.ctypes.data_as(capi.c_int32_p),
                                      capi.dptr(aux.exps), capi.dptr(aux.coefs))


_BASIS_CACHE = {}


def _flat_basis_z(name: str, element_numbers) -> FlatBasis:
    # flattened shells cached per (basis, element sequence): SURVEY.md 8f item 4
    key = (name.lower(), tuple(int(z) for z in element_numbers))
    if key not in _BASIS_CACHE:
        _BASIS_CACHE[key] = build_flat_basis(name, element_numbers)
    return _BASIS_CACHE[key]


def _flat_basis(name: str, fragment: PhysicalFragment) -> FlatBasis:
    return _flat_basis_z(name, fragment.element_numbers)


def _fill(result: CalculationResult, r: capi.ScfResult, eps: Optional[np.ndarray]) -> CalculationResult:
    result.scf_status = int(r.scf_status)
    result.scf_iterations = int(r.iterations)
    if r.has_error:
        # driver: result%error%set(...), has_error = .true., has_energy = .false. (:385-393)
        result.has_error = True
        result.error_code = capi.ERR_GENERIC
        result.error_message = r.message.decode(errors="replace")
        result.has_energy = False
        return result
    result.energy.scf = float(r.e_total)
    result.e_nuclear = float(r.e_nuclear)
    result.e_electronic = float(r.e_electronic)
    result.has_energy = True
    result.homo = float(r.homo)
    result.lumo = float(r.lumo)
    result.has_orbitals = bool(r.has_orbitals)
    if eps is not None:
        result.orbital_energies = eps[: int(r.n_mo)].copy()
    if r.has_dipole:
        result.dipole = np.array([r.dipole[0], r.dipole[1], r.dipole[2]])
        result.has_dipole = True
    result.s_squared = float(r.s_squared)
    result.n_alpha = int(r.n_alpha); result.n_beta = int(r.n_beta)
    return result


def runs_unrestricted(settings: ScfSettings, multiplicity: int, nelec: int) -> bool:
    """The engine's own decision (plan_batch): unrestricted iff forced, multiplicity != 1 or an odd electron count."""
    return bool(settings.unrestricted) or int(multiplicity) != 1 or int(nelec) % 2 != 0


def run_hip_scf(settings: ScfSettings, fragment: PhysicalFragment, result: Optional[CalculationResult] = None,
                want_gradient: bool = False, initial_density: Optional[np.ndarray] = None) -> CalculationResult:
    """One fragment through the engine: the drop-in for run_cuest_scf.  `initial_density` ((n_ao, n_ao) total density of
    a restricted run, (2, n_ao, n_ao) alpha and beta of an unrestricted one) starts the SCF from it
    (run_hip_scf_batch); the result then carries `density` and, unrestricted, `spin_densities`."""
    if initial_density is not None:
        if want_gradient:
            raise ValueError("run_hip_scf: initial_density and want_gradient do not combine; converge first, then ask for the gradient")
        r = run_hip_scf_batch(settings, [fragment], initial_densities=[initial_density])[0]
        if result is None:
            return r
        result.__dict__.update(r.__dict__)
        return result
    result = result if result is not None else CalculationResult()
    try:
        lib = capi.load_library()
        ctx = capi.get_context(settings.device_rank)
        opts = _options(settings, want_gradient)
        fb = _flat_basis(settings.basis_set, fragment)
        aux = _flat_basis(settings.aux_basis_set, fragment) if settings.density_fitting else None
        m = _Marshalled(fragment, fb, aux)
        eps = np.zeros(fb.nao)
        epsb = np.zeros(fb.nao)
        r = capi.ScfResult()
        r.orbital_energies = capi.dptr(eps)
        r.orbital_energies_beta = capi.dptr(epsb)
        grad = np.zeros((fragment.n_atoms, 3)) if want_gradient else None
        if grad is not None:
            r.gradient = capi.dptr(grad)
        rc = lib.mqc_hip_scf_run(ctx, C.byref(m.mol), C.byref(m.bas), C.byref(m.aux_bas) if aux is not None else None,
                                 C.byref(opts), C.byref(r))
        if rc != capi.MQC_HIP_OK and not r.has_error:
            capi.check(rc)
        _fill(result, r, eps)
        if grad is not None and r.has_gradient and not r.has_error:
            result.gradient = grad.T.copy()              # (3, n_atoms) like result%gradient
            result.has_gradient = True
        if result.has_energy and (int(r.n_alpha) != int(r.n_beta) or settings.unrestricted):
            result.orbital_energies_beta = epsb[: int(r.n_mo)].copy()
        return result
    except (capi.HipBackendError, BasisError) as e:
        result.has_error = True
        result.has_energy = False
        result.error_code = getattr(e, "code", capi.ERR_VALIDATION)
        result.error_message = str(getattr(e, "message", e))
        return result


_MOL_DTYPE = np.dtype({"names": ["n_atoms", "atomic_numbers", "xyz", "ghost", "charge", "multiplicity", "nelec",
                                 "n_point_charges", "point_charge_xyz", "point_charges", "h_extra"],
                       "formats": ["<i4", "<u8", "<u8", "<u8", "<i4", "<i4", "<i4", "<i4", "<u8", "<u8", "<u8"],
                       "offsets": [0, 8, 16, 24, 32, 36, 40, 44, 48, 56, 64], "itemsize": C.sizeof(capi.Molecule)})
_BAS_DTYPE = np.dtype({"names": ["spherical", "n_atoms", "nshell_per_atom", "n_shells", "shell_l", "shell_nprim",
                                 "exponents", "coefficients"],
                       "formats": ["<i4", "<i4", "<u8", "<i4", "<u8", "<u8", "<u8", "<u8"],
                       "offsets": [0, 4, 8, 16, 24, 32, 40, 48], "itemsize": C.sizeof(capi.Basis)})


def _basis_record(fb: FlatBasis, n_atoms: int):
    return (1 if fb.spherical else 0, n_atoms, fb.nshell_per_atom.ctypes.data, fb.nshell, fb.shell_l.ctypes.data,
            fb.shell_nprim.ctypes.data, fb.exps.ctypes.data, fb.coefs.ctypes.data)


def _struct_dtype(struct) -> np.dtype:
    """numpy view of a ctypes struct (pointers as u8, char arrays as bytes) with the C offsets."""
    names, formats, offsets = [], [], []
    for name, ctype in struct._fields_:
        size = C.sizeof(ctype)
        if ctype is C.c_double:
            fmt = "<f8"
        elif ctype is C.c_int32:
            fmt = "<i4"
        elif ctype is C.c_int64:
            fmt = "<i8"
        elif issubclass(ctype, C.Array) and ctype._type_ is C.c_char:
            fmt = "S%d" % size
        elif issubclass(ctype, C.Array) and ctype._type_ is C.c_double:
            fmt = ("<f8", (ctype._length_,))
        else:
            fmt = "<u8"          # pointers
        names.append(name); formats.append(fmt); offsets.append(getattr(struct, name).offset)
    return np.dtype({"names": names, "formats": formats, "offsets": offsets, "itemsize": C.sizeof(struct)})


_RES_DTYPE = _struct_dtype(capi.ScfResult)


@dataclass
class FragmentGroup:
    """Fragments that share their element sequence: the unit the engine batches over."""
    element_numbers: np.ndarray            # (n_atoms,)
    xyz: np.ndarray                        # (m, n_atoms, 3) Bohr
    charge: np.ndarray                     # (m,)
    multiplicity: Optional[np.ndarray] = None
    ghost: Optional[np.ndarray] = None     # (n_atoms,) bool, same for the whole group
    nelec: Optional[np.ndarray] = None     # (m,), default sum(Z of real atoms) - charge
    point_charge_xyz: Optional[np.ndarray] = None   # (m, n_pc, 3) Bohr: the embedding field of an FMO / EE-MBE fragment
    point_charges: Optional[np.ndarray] = None      # (m, n_pc)
    h_extra: Optional[np.ndarray] = None            # (m, n_ao, n_ao): a further one-electron operator added to H (run_libcint_rhf's h_extra)
    basis_set: Optional[str] = None                 # this group's orbital basis where it is not settings.basis_set (one call, several bases)


def run_hip_scf_groups(settings: ScfSettings, groups: Sequence[FragmentGroup], want_gradient: bool = False,
                       gradients_out: Optional[list] = None, extras: Sequence[str] = (),
                       extras_out: Optional[list] = None, site_gradients_out: Optional[list] = None,
                       status_out: Optional[list] = None, initial_densities: Optional[Sequence] = None,
                       spin_densities_out: Optional[list] = None, rimp2: Optional[dict] = None,
                       pcm: Optional[dict] = None, cphf: Optional[dict] = None) -> List[np.ndarray]:
    """All fragments of all groups in ONE mqc_hip_scf_run_batch call; returns, per group, a structured array
    viewing the engine's result records (fields of capi.ScfResult: e_total, iterations, has_error, message ...).

    The C structs are filled as numpy structured arrays with the header's exact layout
    (tests/test_host_logic.py checks the sizes), so marshalling a few thousand fragments is a
    handful of vector operations rather than a Python loop over ctypes objects.

    `extras` names per-fragment arrays to bring back besides the records -- "density" (m, n, n), "embedding_matrix"
    (m, n, n), "mulliken_charges" (m, n_atoms) -- appended to `extras_out` as one dict per group.

    `site_gradients_out` (a list) sends the batch through mqc_hip_scf_gradient_embedded_batch instead: the gradient is
    forced on, and one (m, n_pc, 3) array per group (n_pc = 0 for a group without charges) is appended to it -- the
    derivative of e_total with respect to the charges' positions.  `status_out` receives the call's status code.

    `initial_densities` and `spin_densities_out` send the batch through mqc_hip_scf_run_batch_restart.
    `initial_densities` holds one entry per group: None (the whole group starts from settings.guess) or m entries, each
    None or that fragment's starting density -- (n_ao, n_ao), the total density, when the fragment runs restricted,
    (2, n_ao, n_ao), alpha and beta, when it runs unrestricted (runs_unrestricted: forced, multiplicity != 1 or an odd
    electron count).  Any finite density of the right size is legal: the engine projects it onto an SCF state of the new
    geometry.  `spin_densities_out` (a list) receives one (m, 2, n_ao, n_ao) array per group, written for the fragments
    that ran unrestricted (zeros elsewhere).

    `rimp2` (a dict, see run_hip_rimp2_groups) sends the batch through mqc_hip_rimp2_batch; `pcm` (a dict, see
    run_hip_scf_pcm_groups) through mqc_hip_scf_pcm_batch; `cphf` (a dict, see run_hip_polarizability_groups) through
    mqc_hip_polarizability_batch."""
    embedded = site_gradients_out is not None
    restart = initial_densities is not None or spin_densities_out is not None
    if restart and embedded:
        raise ValueError("starting densities and the embedded-gradient entry do not combine")
    if rimp2 is not None and (restart or embedded):
        raise ValueError("RI-MP2 combines with neither starting densities nor the embedded-gradient entry")
    if pcm is not None and (restart or embedded or rimp2 is not None):
        raise ValueError("PCM combines with neither starting densities, the embedded-gradient entry nor RI-MP2")
    if cphf is not None and (restart or embedded or rimp2 is not None or pcm is not None):
        raise ValueError("polarizabilities combine with neither starting densities, the embedded-gradient entry, RI-MP2 nor PCM")
    if initial_densities is not None and len(initial_densities) != len(groups):
        raise ValueError("initial_densities must hold one entry per group")
    want_gradient = bool(want_gradient) or embedded
    sizes = [int(g.xyz.shape[0]) for g in groups]
    n = int(sum(sizes))
    if n == 0:
        if rimp2 is not None:
            rimp2.update(e_os=[np.zeros(0) for _ in groups], e_ss=[np.zeros(0) for _ in groups],
                         mp2_done=[np.zeros(0, dtype=np.int32) for _ in groups])
        if pcm is not None:
            pcm.update(e_pcm=[np.zeros(0) for _ in groups], n_tesserae=[np.zeros(0, dtype=np.int32) for _ in groups])
        if cphf is not None:
            cphf.update(alpha=[np.zeros((0, 3, 3)) for _ in groups], cphf_iterations=[np.zeros(0, dtype=np.int32) for _ in groups],
                        alpha_done=[np.zeros(0, dtype=np.int32) for _ in groups])
        return [np.zeros(0, dtype=_RES_DTYPE) for _ in groups]
    lib = capi.load_library()
    ctx = capi.get_context(settings.device_rank)
    opts = _options(settings, want_gradient)
    df = settings.density_fitting
    mols = np.zeros(n, dtype=_MOL_DTYPE)
    bass = np.zeros(n, dtype=_BAS_DTYPE)
    auxs = np.zeros(n, dtype=_BAS_DTYPE) if df else None
    keep = []                                   # arrays the structs point into
    lo = 0
    for g, m in zip(groups, sizes):
        sl = slice(lo, lo + m)
        lo += m
        if m == 0:
            continue
        z = np.ascontiguousarray(g.element_numbers, dtype=np.int32)
        na = int(len(z))
        ghost = None if g.ghost is None else np.ascontiguousarray(g.ghost, dtype=np.uint8)
        xyz = np.ascontiguousarray(g.xyz, dtype=np.float64)
        if xyz.shape != (m, na, 3):
            raise ValueError("FragmentGroup.xyz must be (m, n_atoms, 3) in Bohr")
        charge = np.broadcast_to(np.asarray(g.charge, dtype=np.int32), (m,))
        if g.nelec is None:
            zsum = int(np.sum(z if ghost is None else z[ghost == 0]))
            nelec = zsum - charge                                        # compute_nelec, :73-83
        else:
            nelec = np.asarray(g.nelec, dtype=np.int32)
        fb = _flat_basis_z(g.basis_set or settings.basis_set, z)
        keep += [z, ghost, xyz, fb]
        mols["n_atoms"][sl] = na
        mols["atomic_numbers"][sl] = z.ctypes.data
        mols["xyz"][sl] = xyz.ctypes.data + np.arange(m, dtype=np.uint64) * np.uint64(na * 3 * 8)
        mols["ghost"][sl] = 0 if ghost is None else ghost.ctypes.data
        mols["charge"][sl] = charge
        mols["multiplicity"][sl] = 1 if g.multiplicity is None else np.asarray(g.multiplicity, dtype=np.int32)
        mols["nelec"][sl] = nelec
        if g.point_charges is not None:
            pq = np.ascontiguousarray(g.point_charges, dtype=np.float64)
            px = np.ascontiguousarray(g.point_charge_xyz, dtype=np.float64)
            npc = int(pq.shape[1])
            if pq.shape != (m, npc) or px.shape != (m, npc, 3):
                raise ValueError("FragmentGroup.point_charges must be (m, n_pc) with point_charge_xyz (m, n_pc, 3)")
            keep += [pq, px]
            mols["n_point_charges"][sl] = npc
            mols["point_charges"][sl] = pq.ctypes.data + np.arange(m, dtype=np.uint64) * np.uint64(npc * 8)
            mols["point_charge_xyz"][sl] = px.ctypes.data + np.arange(m, dtype=np.uint64) * np.uint64(npc * 3 * 8)
        if g.h_extra is not None:
            hx = np.ascontiguousarray(g.h_extra, dtype=np.float64)
            if hx.shape != (m, fb.nao, fb.nao):
                raise ValueError("FragmentGroup.h_extra must be (m, n_ao, n_ao)")
            keep.append(hx)
            mols["h_extra"][sl] = hx.ctypes.data + np.arange(m, dtype=np.uint64) * np.uint64(fb.nao * fb.nao * 8)
        bass[sl] = _basis_record(fb, na)
        if df:
            ab = _flat_basis_z(settings.aux_basis_set, z)
            keep.append(ab)
            auxs[sl] = _basis_record(ab, na)
    res = (capi.ScfResult * n)()
    grads = []
    if want_gradient:
        # one (m, n_atoms, 3) array per group; every record points at its own slice
        rec0 = np.frombuffer(res, dtype=_RES_DTYPE)
        lo = 0
        for g, m in zip(groups, sizes):
            na = int(len(g.element_numbers))
            ga = np.zeros((m, na, 3))
            grads.append(ga)
            if m:
                rec0["gradient"][lo:lo + m] = ga.ctypes.data + np.arange(m, dtype=np.uint64) * np.uint64(na * 3 * 8)
            lo += m
        if gradients_out is not None:
            gradients_out.extend(grads)
    if extras:
        rec0 = np.frombuffer(res, dtype=_RES_DTYPE)
        lo = 0
        for g, m in zip(groups, sizes):
            z = np.ascontiguousarray(g.element_numbers, dtype=np.int32)
            nao = _flat_basis_z(g.basis_set or settings.basis_set, z).nao
            got = {}
            for name in extras:
                if name not in ("density", "embedding_matrix", "mulliken_charges"):
                    raise ValueError("unknown extra output " + name)
                width = len(z) if name == "mulliken_charges" else nao * nao
                arr = np.zeros((m, width))
                if m:
                    rec0[name][lo:lo + m] = arr.ctypes.data + np.arange(m, dtype=np.uint64) * np.uint64(width * 8)
                got[name] = arr if name == "mulliken_charges" else arr.reshape(m, nao, nao)
            lo += m
            if extras_out is not None:
                extras_out.append(got)
            keep.append(got)
    if restart:
        d0_ptr = np.zeros(n, dtype=np.uint64)
        spin_ptr = np.zeros(n, dtype=np.uint64)
        lo = 0
        for gi, (g, m) in enumerate(zip(groups, sizes)):
            z = np.ascontiguousarray(g.element_numbers, dtype=np.int32)
            nao = _flat_basis_z(g.basis_set or settings.basis_set, z).nao
            entries = None if initial_densities is None else initial_densities[gi]
            if entries is not None and m:
                if len(entries) != m:
                    raise ValueError("initial_densities[%d] must hold one entry per fragment of the group" % gi)
                mult = np.broadcast_to(mols["multiplicity"][lo:lo + m], (m,))
                nel = np.broadcast_to(mols["nelec"][lo:lo + m], (m,))
                for k, d in enumerate(entries):
                    if d is None:
                        continue
                    a = np.ascontiguousarray(d, dtype=np.float64)
                    want = (2, nao, nao) if runs_unrestricted(settings, mult[k], nel[k]) else (nao, nao)
                    if a.shape != want:
                        raise ValueError("initial density of fragment %d of group %d has shape %s; this run needs %s"
                                         % (k, gi, a.shape, want))
                    keep.append(a)
                    d0_ptr[lo + k] = a.ctypes.data
            if spin_densities_out is not None:
                sd = np.zeros((m, 2, nao, nao))
                spin_densities_out.append(sd)
                if m:
                    spin_ptr[lo:lo + m] = sd.ctypes.data + np.arange(m, dtype=np.uint64) * np.uint64(2 * nao * nao * 8)
            lo += m
        rc = lib.mqc_hip_scf_run_batch_restart(ctx, n, mols.ctypes.data_as(C.POINTER(capi.Molecule)),
                                               bass.ctypes.data_as(C.POINTER(capi.Basis)),
                                               auxs.ctypes.data_as(C.POINTER(capi.Basis)) if df else None, C.byref(opts), res,
                                               d0_ptr.ctypes.data_as(C.POINTER(capi.c_double_p)) if initial_densities is not None else None,
                                               spin_ptr.ctypes.data_as(C.POINTER(capi.c_double_p)) if spin_densities_out is not None else None)
    elif embedded:
        # one (m, n_pc, 3) array per group; entry i of the pointer array is fragment i's slice (0 = no charges)
        site_ptr = np.zeros(n, dtype=np.uint64)
        sites, lo = [], 0
        for g, m in zip(groups, sizes):
            npc = 0 if g.point_charges is None else int(np.asarray(g.point_charges).shape[1])
            sg = np.zeros((m, npc, 3))
            sites.append(sg)
            if m and npc:
                site_ptr[lo:lo + m] = sg.ctypes.data + np.arange(m, dtype=np.uint64) * np.uint64(npc * 3 * 8)
            lo += m
        site_gradients_out.extend(sites)
        rc = lib.mqc_hip_scf_gradient_embedded_batch(ctx, n, mols.ctypes.data_as(C.POINTER(capi.Molecule)),
                                                     bass.ctypes.data_as(C.POINTER(capi.Basis)),
                                                     auxs.ctypes.data_as(C.POINTER(capi.Basis)) if df else None, C.byref(opts), res,
                                                     site_ptr.ctypes.data_as(C.POINTER(capi.c_double_p)))
    elif rimp2 is not None:
        e_os, e_ss, done = np.zeros(n), np.zeros(n), np.zeros(n, dtype=np.int32)
        rc = lib.mqc_hip_rimp2_batch(ctx, n, mols.ctypes.data_as(C.POINTER(capi.Molecule)),
                                     bass.ctypes.data_as(C.POINTER(capi.Basis)),
                                     auxs.ctypes.data_as(C.POINTER(capi.Basis)) if df else None, C.byref(opts), res,
                                     1 if rimp2.get("frozen_core", True) else 0, capi.dptr(e_os), capi.dptr(e_ss),
                                     done.ctypes.data_as(capi.c_int32_p))
        cuts = np.cumsum(sizes)[:-1]
        rimp2.update(e_os=np.split(e_os, cuts), e_ss=np.split(e_ss, cuts), mp2_done=np.split(done, cuts))
    elif pcm is not None:
        e_pcm, n_tess = np.zeros(n), np.zeros(n, dtype=np.int32)
        popts = pcm["settings"].options(keep)
        rc = lib.mqc_hip_scf_pcm_batch(ctx, n, mols.ctypes.data_as(C.POINTER(capi.Molecule)),
                                       bass.ctypes.data_as(C.POINTER(capi.Basis)),
                                       auxs.ctypes.data_as(C.POINTER(capi.Basis)) if df else None, C.byref(opts), C.byref(popts), res,
                                       capi.dptr(e_pcm), n_tess.ctypes.data_as(capi.c_int32_p))
        cuts = np.cumsum(sizes)[:-1]
        pcm.update(e_pcm=np.split(e_pcm, cuts), n_tesserae=np.split(n_tess, cuts))
    elif cphf is not None:
        alpha, its, done = np.zeros((n, 3, 3)), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
        copts = cphf["settings"].options()
        rc = lib.mqc_hip_polarizability_batch(ctx, n, mols.ctypes.data_as(C.POINTER(capi.Molecule)),
                                              bass.ctypes.data_as(C.POINTER(capi.Basis)), C.byref(opts), C.byref(copts), res,
                                              capi.dptr(alpha), its.ctypes.data_as(capi.c_int32_p), done.ctypes.data_as(capi.c_int32_p))
        cuts = np.cumsum(sizes)[:-1]
        cphf.update(alpha=np.split(alpha, cuts), cphf_iterations=np.split(its, cuts), alpha_done=np.split(done, cuts))
    else:
        rc = lib.mqc_hip_scf_run_batch(ctx, n, mols.ctypes.data_as(C.POINTER(capi.Molecule)),
                                       bass.ctypes.data_as(C.POINTER(capi.Basis)),
                                       auxs.ctypes.data_as(C.POINTER(capi.Basis)) if df else None, C.byref(opts), res)
    if status_out is not None:
        status_out.append(int(rc))
    rec = np.frombuffer(res, dtype=_RES_DTYPE)
    if rc != capi.MQC_HIP_OK and not np.any(rec["has_error"]):
        capi.check(rc)
    del keep
    out, lo = [], 0
    for m in sizes:
        out.append(rec[lo:lo + m])
        lo += m
    return out


def run_hip_embedded_gradients(settings: ScfSettings, groups: Sequence[FragmentGroup], extras: Sequence[str] = (),
                               extras_out: Optional[list] = None, status_out: Optional[list] = None):
    """Analytic gradients of fragments embedded in point charges, all groups in ONE mqc_hip_scf_gradient_embedded_batch
    call -> (records, atom_gradients, site_gradients): per group the result records (as run_hip_scf_groups), the
    gradient on the fragment's atoms (m, n_atoms, 3) with the charges held fixed, and the gradient on the charges' sites
    (m, n_pc, 3).  Both are derivatives of the records' e_total, which holds tr(D u) but not the classical
    nuclei-charge term sum Z_A q_g / R_Ag: that term and its derivative are the caller's.  Groups without charges get
    the plain gradient and an (m, 0, 3) site array; a group with h_extra is refused in its records."""
    atom, site = [], []
    rec = run_hip_scf_groups(settings, groups, want_gradient=True, gradients_out=atom, extras=extras, extras_out=extras_out,
                             site_gradients_out=site, status_out=status_out)
    if not atom:      # an empty batch
        atom = [np.zeros((0, len(g.element_numbers), 3)) for g in groups]
        site = [np.zeros((0, 0, 3)) for g in groups]
    return rec, atom, site


def run_hip_esp(settings: ScfSettings, group: FragmentGroup, densities, points, n_points=None,
                include_nuclei: bool = True, out: Optional[np.ndarray] = None) -> np.ndarray:
    """Electrostatic potential V(r) = sum_A Z_A/|r - R_A| - sum D_uv (u|1/|r' - r||v) of the m fragments of one group at
    their own points, in ONE mqc_hip_esp_batch call.

    densities (m, n_ao, n_ao); points (m, max_points, 3) in Bohr; n_points (m,) or None = max_points each (ragged
    counts: entries of `points` beyond a fragment's count are not read, and the matching entries of the result stay as
    they were: 0, or what the caller's `out` (m, max_points) held).  include_nuclei = False gives the electronic part
    alone.  -> (m, max_points) in Hartree per unit charge."""
    xyz = np.ascontiguousarray(group.xyz, dtype=np.float64)
    z = np.ascontiguousarray(group.element_numbers, dtype=np.int32)
    m, na = int(xyz.shape[0]), int(len(z))
    if xyz.shape != (m, na, 3):
        raise ValueError("FragmentGroup.xyz must be (m, n_atoms, 3) in Bohr")
    fb = _flat_basis_z(settings.basis_set, z)
    D = np.ascontiguousarray(densities, dtype=np.float64)
    if D.shape != (m, fb.nao, fb.nao):
        raise ValueError("densities must be (m, n_ao, n_ao)")
    pts = np.ascontiguousarray(points, dtype=np.float64)
    if pts.ndim != 3 or pts.shape[0] != m or pts.shape[2] != 3:
        raise ValueError("points must be (m, max_points, 3) in Bohr")
    max_points = int(pts.shape[1])
    counts = None if n_points is None else np.ascontiguousarray(n_points, dtype=np.int32)
    if counts is not None and counts.shape != (m,):
        raise ValueError("n_points must be (m,)")
    if out is None:
        out = np.zeros((m, max_points))
    elif out.shape != (m, max_points) or out.dtype != np.float64 or not out.flags["C_CONTIGUOUS"]:
        raise ValueError("out must be a C-contiguous float64 array of shape (m, max_points)")
    lib = capi.load_library()
    ctx = capi.get_context(settings.device_rank)
    ghost = None if group.ghost is None else np.ascontiguousarray(group.ghost, dtype=np.uint8)
    mols = np.zeros(max(m, 1), dtype=_MOL_DTYPE)
    mols["n_atoms"] = na; mols["atomic_numbers"] = z.ctypes.data
    mols["xyz"][:m] = xyz.ctypes.data + np.arange(m, dtype=np.uint64) * np.uint64(na * 3 * 8)
    mols["ghost"] = 0 if ghost is None else ghost.ctypes.data
    mols["multiplicity"] = 1
    mols["nelec"] = int(np.sum(z if ghost is None else z[ghost == 0]))
    bas = np.zeros(1, dtype=_BAS_DTYPE); bas[0] = _basis_record(fb, na)
    capi.check(lib.mqc_hip_esp_batch(ctx, m, mols.ctypes.data_as(C.POINTER(capi.Molecule)), bas.ctypes.data_as(C.POINTER(capi.Basis)),
                                     capi.dptr(D), max_points, None if counts is None else counts.ctypes.data_as(capi.c_int32_p),
                                     capi.dptr(pts), 1 if include_nuclei else 0, capi.dptr(out)))
    return out


def _groups_of(fragments: Sequence[PhysicalFragment]):
    """Fragments sorted into FragmentGroups by element sequence and ghost flags -> (groups, index), index[g][k] the
    position in `fragments` of the k-th fragment of group g."""
    by_key = {}
    for i, f in enumerate(fragments):
        key = (f.element_numbers.tobytes(), None if f.ghost is None else f.ghost.tobytes())
        by_key.setdefault(key, []).append(i)
    groups, index = [], []
    for idx in by_key.values():
        f0 = fragments[idx[0]]
        groups.append(FragmentGroup(f0.element_numbers, np.stack([fragments[i].coordinates.T for i in idx]),
                                    np.array([fragments[i].charge for i in idx], dtype=np.int32),
                                    np.array([fragments[i].multiplicity for i in idx], dtype=np.int32),
                                    f0.ghost, np.array([fragments[i].nelec for i in idx], dtype=np.int32)))
        index.append(idx)
    return groups, index


def frozen_core_count(element_numbers, ghost=None) -> int:
    """Frozen-core orbitals of a fragment, the engine's table (mqc_hip_rimp2_batch): per atom 0 for Z <= 2, 1 for
    Z = 3-10, 5 for Z = 11-18, 9 for Z = 19-36; ghost atoms freeze none.  Water: 1; a water dimer: 2; H2: 0."""
    z = np.asarray(element_numbers, dtype=np.int64).reshape(-1)
    if np.any(z > 36):
        raise ValueError("frozen_core_count: the table ends at Z = 36")
    per_atom = np.where(z <= 2, 0, np.where(z <= 10, 1, np.where(z <= 18, 5, 9)))
    if ghost is not None:
        per_atom = np.where(np.asarray(ghost, dtype=bool).reshape(-1), 0, per_atom)
    return int(per_atom.sum())


def run_hip_rimp2_groups(settings: ScfSettings, groups: Sequence[FragmentGroup], frozen_core: bool = True,
                         extras: Sequence[str] = (), extras_out: Optional[list] = None, status_out: Optional[list] = None):
    """All fragments of all groups in ONE mqc_hip_rimp2_batch call: the density-fitted closed-shell SCF of
    run_hip_scf_groups followed, per converged fragment, by its RI-MP2 correlation energy.
    -> (records, e_os, e_ss, mp2_done): per group the result records (e_total stays the SCF energy) and three arrays
    (m,): the opposite-spin and same-spin parts (E_corr = e_os + e_ss) and 1 where they were formed -- 0, with zeros
    for both parts, where the SCF failed or did not converge.  `frozen_core` leaves frozen_core_count(...) lowest
    orbitals of each fragment out of the sums.  Refusals (no density fitting, a functional, open shells) arrive in the
    records' messages, the call's status in `status_out`."""
    box = {"frozen_core": bool(frozen_core)}
    rec = run_hip_scf_groups(settings, groups, extras=extras, extras_out=extras_out, status_out=status_out, rimp2=box)
    return rec, box["e_os"], box["e_ss"], box["mp2_done"]


def run_hip_rimp2_batch(settings: ScfSettings, fragments: Sequence[PhysicalFragment], frozen_core: bool = True) -> List[CalculationResult]:
    """Many independent fragments through mqc_hip_rimp2_batch, results as CalculationResult objects: energy.scf, and
    where has_mp2 is set energy.mp2_os / energy.mp2_ss (energy.total() = scf + mp2).  A fragment whose SCF converged
    without a correlation energy does not exist: has_mp2 is False exactly where the record carries an error or the SCF
    did not converge."""
    results = [CalculationResult() for _ in range(len(fragments))]
    if not fragments:
        return results
    groups, index = _groups_of(fragments)
    recs, e_os, e_ss, done = run_hip_rimp2_groups(settings, groups, frozen_core)
    for idx, rec, os_, ss_, dn in zip(index, recs, e_os, e_ss, done):
        for pos, (i, r) in enumerate(zip(idx, rec)):
            _fill_record(results[i], r)
            if results[i].has_energy and dn[pos]:
                results[i].energy.mp2_os = float(os_[pos]); results[i].energy.mp2_ss = float(ss_[pos])
                results[i].has_mp2 = True
    return results


def run_hip_polarizability_groups(settings: ScfSettings, groups: Sequence[FragmentGroup], cphf: Optional[CphfSettings] = None,
                                  extras: Sequence[str] = (), extras_out: Optional[list] = None, status_out: Optional[list] = None):
    """All fragments of all groups in ONE mqc_hip_polarizability_batch call: the closed-shell Hartree-Fock SCF of
    run_hip_scf_groups on the in-core path followed, per converged fragment, by the CPHF solve for its static dipole
    polarizability.  -> (records, alpha, cphf_iterations, alpha_done): per group the result records and three arrays:
    alpha (m, 3, 3) in atomic units in the laboratory frame, the iterations of each solve (m,) and 1 where alpha was
    formed -- 0, with zeros, where the SCF or the solve failed (the record then says why).  Refusals (density fitting, a
    functional, open shells, a gradient, the direct path, n_ao > 116) arrive in the records' messages, the call's status
    in `status_out`."""
    box = {"settings": cphf or CphfSettings()}
    rec = run_hip_scf_groups(settings, groups, extras=extras, extras_out=extras_out, status_out=status_out, cphf=box)
    return rec, box["alpha"], box["cphf_iterations"], box["alpha_done"]


def run_hip_polarizability_batch(settings: ScfSettings, fragments: Sequence[PhysicalFragment],
                                 cphf: Optional[CphfSettings] = None) -> List[CalculationResult]:
    """Many independent fragments through mqc_hip_polarizability_batch, results as CalculationResult objects: energy.scf,
    and where has_polarizability is set `polarizability` (3, 3) and `cphf_iterations`."""
    results = [CalculationResult() for _ in range(len(fragments))]
    if not fragments:
        return results
    groups, index = _groups_of(fragments)
    recs, alpha, its, done = run_hip_polarizability_groups(settings, groups, cphf)
    for idx, rec, al, it, dn in zip(index, recs, alpha, its, done):
        for pos, (i, r) in enumerate(zip(idx, rec)):
            _fill_record(results[i], r)
            results[i].cphf_iterations = int(it[pos])
            if results[i].has_energy and dn[pos]:
                results[i].polarizability = np.array(al[pos], dtype=float)
                results[i].has_polarizability = True
    return results


def run_hip_scf_pcm_groups(settings: ScfSettings, pcm: PcmSettings, groups: Sequence[FragmentGroup], want_gradient: bool = False,
                           extras: Sequence[str] = (), extras_out: Optional[list] = None, status_out: Optional[list] = None):
    """All fragments of all groups in ONE mqc_hip_scf_pcm_batch call: run_hip_scf_groups in the C-PCM continuum `pcm`
    describes.  -> (records, e_pcm, n_tesserae): per group the result records (e_total and e_electronic contain E_pcm)
    and two arrays (m,): E_pcm (0 where the fragment failed) and the tesserae of its cavity.  Refusals (a gradient,
    point charges, h_extra, a bad epsilon or rule, an element without a radius) arrive in the records' messages, the
    call's status in `status_out`."""
    box = {"settings": pcm}
    rec = run_hip_scf_groups(settings, groups, want_gradient=want_gradient, extras=extras, extras_out=extras_out,
                             status_out=status_out, pcm=box)
    return rec, box["e_pcm"], box["n_tesserae"]


def run_hip_scf_pcm_batch(settings: ScfSettings, pcm: PcmSettings, fragments: Sequence[PhysicalFragment]) -> List[CalculationResult]:
    """Many independent fragments through mqc_hip_scf_pcm_batch, results as CalculationResult objects: energy.scf is the
    total energy in the continuum and energy.pcm the part of it that is E_pcm."""
    results = [CalculationResult() for _ in range(len(fragments))]
    if not fragments:
        return results
    groups, index = _groups_of(fragments)
    recs, e_pcm, _ = run_hip_scf_pcm_groups(settings, pcm, groups)
    for idx, rec, ep in zip(index, recs, e_pcm):
        for pos, (i, r) in enumerate(zip(idx, rec)):
            _fill_record(results[i], r)
            if results[i].has_energy:
                results[i].energy.pcm = float(ep[pos])
    return results


def run_hip_scf_batch(settings: ScfSettings, fragments: Sequence[PhysicalFragment],
                      initial_densities: Optional[Sequence] = None) -> List[CalculationResult]:
    """Many independent fragments in one call (mqc_hip_scf_run_batch), results as CalculationResult objects.

    `initial_densities` (one entry per fragment: None, or a starting density as run_hip_scf_groups describes) sends the
    call through mqc_hip_scf_run_batch_restart; every result then carries its converged `density` and, where the
    fragment ran unrestricted, its `spin_densities` -- what the next restart takes."""
    n = len(fragments)
    if initial_densities is not None and len(initial_densities) != n:
        raise ValueError("initial_densities must hold one entry per fragment")
    results = [CalculationResult() for _ in range(n)]
    if n == 0:
        return results
    groups, index = _groups_of(fragments)
    if initial_densities is None:
        for idx, rec in zip(index, run_hip_scf_groups(settings, groups)):
            for i, r in zip(idx, rec):
                _fill_record(results[i], r)
        return results
    extras_out: list = []
    spin_out: list = []
    recs = run_hip_scf_groups(settings, groups, extras=("density",), extras_out=extras_out,
                              initial_densities=[[initial_densities[i] for i in idx] for idx in index], spin_densities_out=spin_out)
    for idx, rec, ex, sd in zip(index, recs, extras_out, spin_out):
        for pos, (i, r) in enumerate(zip(idx, rec)):
            _fill_record(results[i], r)
            if results[i].has_energy:
                results[i].density = ex["density"][pos].copy()
                if runs_unrestricted(settings, fragments[i].multiplicity, fragments[i].nelec):
                    results[i].spin_densities = sd[pos].copy()
    return results


def _fill_record(result: CalculationResult, r) -> CalculationResult:
    """_fill for one row of the structured result view."""
    result.scf_status = int(r["scf_status"])
    result.scf_iterations = int(r["iterations"])
    if r["has_error"]:
        result.has_error = True
        result.error_code = capi.ERR_GENERIC
        result.error_message = bytes(r["message"]).split(b"\0", 1)[0].decode(errors="replace")
        result.has_energy = False
        return result
    result.energy.scf = float(r["e_total"])
    result.e_nuclear = float(r["e_nuclear"])
    result.e_electronic = float(r["e_electronic"])
    result.has_energy = True
    result.homo = float(r["homo"])
    result.lumo = float(r["lumo"])
    result.has_orbitals = bool(r["has_orbitals"])
    if r["has_dipole"]:
        result.dipole = np.array(r["dipole"], dtype=float)
        result.has_dipole = True
    result.s_squared = float(r["s_squared"])
    return result


class HFMethod:
    """qc_method_t for Hartree-Fock (src/methods/mqc_method_base.f90:13-60, mqc_method_hf.F90)."""

    def __init__(self, settings: Optional[ScfSettings] = None, **kw):
        self.settings = settings or ScfSettings(**kw)

    def calc_energy(self, fragment: PhysicalFragment, result: Optional[CalculationResult] = None) -> CalculationResult:
        backend = self.settings.backend
        if backend == BACKEND_LIBCINT:
            r = result or CalculationResult()
            r.has_error = True
            r.error_message = "the libcint CPU backend is not part of this build; use backend hip|auto"
            return r
        return run_hip_scf(self.settings, fragment, result)

    def calc_gradient(self, fragment, result=None):
        """hf_calc_gradient (src/methods/mqc_method_hf.F90): the SCF with want_gradient, result%gradient (3, n_atoms)."""
        return run_hip_scf(self.settings, fragment, result, want_gradient=True)

    def calc_hessian(self, fragment, result=None):
        """hf_calc_hessian -> finite_difference_hessian (src/methods/mqc_method_hf.F90:228-257,
        src/methods/mqc_semi_numerical_hessian.f90): central differences of analytic gradients at +-0.005 Bohr,
        H[i, j] = (g_j(x_i + h) - g_j(x_i - h)) / 2h, symmetrised (finite_diff_hessian_from_gradients,
        src/utils/mqc_finite_differences.f90); the dipoles of the same displacements give d mu / d R; the undisplaced
        point supplies energy, gradient and dipole.  The reference walks the 6 N + 1 geometries one SCF at a time; here
        they are ONE batch of the engine (one topology group)."""
        h = DEFAULT_DISPLACEMENT
        na = len(fragment.element_numbers)
        base = np.asarray(fragment.coordinates, dtype=float)              # (3, n_atoms)
        coords = [base.T.copy()]
        for a in range(na):
            for c in range(3):
                for sgn in (+1.0, -1.0):
                    x = base.T.copy(); x[a, c] += sgn * h
                    coords.append(x)
        m = len(coords)
        group = FragmentGroup(fragment.element_numbers, np.stack(coords), np.full(m, fragment.charge, dtype=np.int32),
                              np.full(m, fragment.multiplicity, dtype=np.int32), fragment.ghost, np.full(m, fragment.nelec, dtype=np.int32))
        grads: list = []
        rec = run_hip_scf_groups(self.settings, [group], want_gradient=True, gradients_out=grads)[0]
        r = result or CalculationResult()
        bad = [k for k in range(m) if rec["has_error"][k] or not rec["has_gradient"][k]]
        if bad:
            k = bad[0]
            r.has_error = True
            r.error_message = ("Hessian: the gradient at displaced geometry %d failed: " % k) + \
                bytes(rec["message"][k]).split(b"\0", 1)[0].decode(errors="replace")
            return r
        _fill_record(r, rec[0])
        g = grads[0]                                                        # (m, n_atoms, 3)
        r.gradient = g[0].T.copy(); r.has_gradient = True
        hess = np.zeros((3 * na, 3 * na))
        dmu = np.zeros((3, 3 * na))
        have_dip = all(bool(rec["has_dipole"][k]) for k in range(m))
        for i in range(3 * na):
            fwd, bwd = 1 + 2 * i, 2 + 2 * i
            hess[i, :] = (g[fwd] - g[bwd]).reshape(-1) / (2.0 * h)
            if have_dip:
                dmu[:, i] = (np.array(rec["dipole"][fwd]) - np.array(rec["dipole"][bwd])) / (2.0 * h)
        r.hessian = 0.5 * (hess + hess.T); r.has_hessian = True
        if have_dip:
            r.dipole_derivatives = dmu; r.has_dipole_derivatives = True
        return r


def get_stats() -> capi.Stats:
    st = capi.Stats()
    capi.check(capi.load_library().mqc_hip_get_stats(capi.get_context(), C.byref(st)))
    return st
