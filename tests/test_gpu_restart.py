"""SCFs restarted from supplied densities (mqc_hip_scf_run_batch_restart; kern_scf.hip, restart_kernel): the device
projection of a density onto an SCF state of the current geometry, per fragment, on every route of the batch driver.

The references are tests/restart_reference.py's (numpy, on the oracle); tests/test_restart_reference.py checks on the CPU
that every displaced-geometry and dimer case used here starts closer than GWH, so the iteration counts below are compared
with the reference's and none is written down by hand."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from metalquicha_amd import capi, fmo, mbe, methods
from tests import restart_cases as rc
from tests import workload_cases as wc
from tests.helpers import fragment_bohr, w3_system, water_at

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIGHT = dict(energy_tol=rc.E_TOL, density_tol=rc.D_TOL, guess="gwh")


def group_of(frags):
    f0 = frags[0]
    return methods.FragmentGroup(f0.element_numbers, np.stack([f.coordinates.T for f in frags]),
                                 np.array([f.charge for f in frags], dtype=np.int32),
                                 np.array([f.multiplicity for f in frags], dtype=np.int32), f0.ghost,
                                 np.array([f.nelec for f in frags], dtype=np.int32))


def solve(settings, frags, start=None, spin=False, restart_entry=None):
    """Fragments of ONE element sequence in one call -> (records, total densities, spin densities or None, status).
    start: None (the plain entry, unless spin or restart_entry ask for the restart entry) or one entry per fragment."""
    ex, sp, status = [], [] if spin else None, []
    kw = {}
    if start is not None:
        kw["initial_densities"] = [start]
    elif restart_entry:
        kw["initial_densities"] = [None]
    if spin:
        kw["spin_densities_out"] = sp
    rec = methods.run_hip_scf_groups(settings, [group_of(frags)], extras=("density",), extras_out=ex, status_out=status, **kw)[0]
    return rec, ex[0]["density"], (sp[0] if spin else None), status[0]


def message(rec, k):
    return bytes(rec["message"][k]).split(b"\0", 1)[0].decode(errors="replace")


def water6():
    rng = np.random.default_rng(3)
    return fragment_bohr([8, 1, 1] * 6, np.vstack([water_at(rng, [5.6 * (i % 3), 5.6 * (i // 3), 0.3 * i]) for i in range(6)]))


OH = dict(Z=[8, 1], xyz=[[0.0, 0.0, 0.0], [0.0, 0.0, 1.8324]])
CH3 = dict(Z=[6, 1, 1, 1], xyz=[[0.0, 0.0, 0.05], [2.04, 0.0, -0.05], [-1.02, 1.7667, -0.05], [-1.02, -1.7667, -0.05]])
FIXED_POINT = {
    "rhf-incore": (rc.water, dict(basis_set="cc-pvdz", eri_mode="incore")),
    "rhf-direct": (rc.water, dict(basis_set="cc-pvdz", eri_mode="direct")),
    "rhf-df": (rc.water, dict(basis_set="cc-pvdz", density_fitting=True, aux_basis_set=wc.AUX)),
    "b3lyp": (rc.water, dict(basis_set="cc-pvdz", functional="b3lyp")),
    "tpss-631g": (rc.water, dict(basis_set="6-31g", functional="tpss")),
    "uhf-oh": (lambda: fragment_bohr(OH["Z"], OH["xyz"], multiplicity=2), dict(basis_set="cc-pvdz")),
    "uks-pbe-ch3": (lambda: fragment_bohr(CH3["Z"], CH3["xyz"], multiplicity=2), dict(basis_set="6-31g", functional="pbe")),
    "global-jacobi-n144": (water6, dict(basis_set="cc-pvdz", eri_mode="direct")),
}


@pytest.mark.parametrize("name", list(FIXED_POINT))
def test_restart_from_the_converged_density_is_a_fixed_point(name):
    """Converged with the plain entry (unrestricted: the restart entry with no density, for the spin densities), then
    restarted from what came back: the projection reproduces the density, so the run needs the two iterations the
    convergence test asks for and lands on the same energy."""
    make, kw = FIXED_POINT[name]
    frag, st = make(), methods.ScfSettings(**kw, **TIGHT)
    unrestricted = methods.runs_unrestricted(st, frag.multiplicity, frag.nelec)
    rec0, dens, spin, status = solve(st, [frag], spin=unrestricted)
    assert status == 0 and not rec0["has_error"][0], message(rec0, 0)
    assert rec0["scf_status"][0] == methods.SCF_CONVERGED
    if unrestricted:
        assert np.max(np.abs(spin[0][0] + spin[0][1] - dens[0])) < 1e-13       # results[i].density stays the total
    rec1, dens1, _, status = solve(st, [frag], start=[spin[0] if unrestricted else dens[0]], spin=unrestricted)
    assert status == 0 and not rec1["has_error"][0], message(rec1, 0)
    print("%s: n_ao %d, %d iterations from GWH, %d restarted, dE = %.2e" % (name, rec0["n_ao"][0], rec0["iterations"][0],
                                                                          rec1["iterations"][0], rec1["e_total"][0] - rec0["e_total"][0]))
    assert rec1["scf_status"][0] == methods.SCF_CONVERGED
    assert rec1["iterations"][0] == 2
    assert abs(rec1["e_total"][0] - rec0["e_total"][0]) < 1e-9
    if name == "global-jacobi-n144":
        assert rec0["n_ao"][0] == 144


def engine_start(name):
    """The engine's own converged densities of the case's sources (old geometry, or the two monomers), block-diagonal."""
    _, basis, functional, sources = rc.CASES[name]
    st = methods.ScfSettings(basis_set=basis, functional=functional, **TIGHT)
    src = {"water": rc.water, "monomer0": lambda: rc.dimer_monomers()[0], "monomer1": lambda: rc.dimer_monomers()[1]}
    frags = [src[s]() for s in sources]
    rec, dens, _, status = solve(st, frags)
    assert status == 0 and not np.any(rec["has_error"])
    return fmo.block_diagonal([dens[k] for k in range(len(frags))]), st


_SINGLE = {}


def single_restart(name):
    """(restarted record, GWH-started record) of the engine on the case's fragment, one fragment per call; shared."""
    if name not in _SINGLE:
        start, st = engine_start(name)
        frag = rc.case_fragment(name)
        plain, _, _, s0 = solve(st, [frag])
        again, _, _, s1 = solve(st, [frag], start=[start])
        assert s0 == 0 and s1 == 0 and not plain["has_error"][0] and not again["has_error"][0], (message(plain, 0), message(again, 0))
        _SINGLE[name] = (again, plain, start, st)
    return _SINGLE[name]


@pytest.mark.parametrize("name", sorted(rc.CASES))
def test_restart_at_another_geometry_and_of_a_dimer_from_its_monomers(name):
    """displaced-*: converged water, every atom moved by up to 0.05 Bohr, restarted at the new geometry.  dimer-*: the
    water dimer (cc-pVDZ: n = 48, the benchmark's shape; 6-31G: the twin-shell route) from its monomers' densities side by
    side.  Same energy as the GWH-started engine run and as the reference (1e-8, the project's parity bound; all runs are
    converged to 1e-11), and the reference's iteration count."""
    again, plain, _, _ = single_restart(name)
    ref, ref_plain = rc.reference_restart(name)
    print("%s: engine %d iterations restarted (%d from GWH), reference %d (%d); E - E_gwh = %.2e, E - E_ref = %.2e"
          % (name, again["iterations"][0], plain["iterations"][0], ref.iterations, ref_plain.iterations,
             again["e_total"][0] - plain["e_total"][0], again["e_total"][0] - ref.energy))
    assert again["scf_status"][0] == methods.SCF_CONVERGED and ref.converged
    assert abs(again["e_total"][0] - plain["e_total"][0]) < 1e-8
    assert abs(again["e_total"][0] - ref.energy) < 1e-8
    assert again["iterations"][0] == ref.iterations


@pytest.mark.parametrize("kind", ["zeros", "half"])
def test_poor_densities_are_legal_starts(kind):
    """All zeros (every natural occupation 0: the projection fills the first orbitals of the orthogonaliser) and the
    converged density scaled by 0.5 (wrong trace, right orbitals): both converge to the GWH-started energy."""
    st = methods.ScfSettings(basis_set="cc-pvdz", **TIGHT)
    frag = rc.water()
    plain, dens, _, _ = solve(st, [frag])
    start = np.zeros_like(dens[0]) if kind == "zeros" else 0.5 * dens[0]
    rec, _, _, status = solve(st, [frag], start=[start])
    print("%s: %d iterations (GWH %d), dE = %.2e" % (kind, rec["iterations"][0], plain["iterations"][0], rec["e_total"][0] - plain["e_total"][0]))
    assert status == 0 and not rec["has_error"][0], message(rec, 0)
    assert rec["scf_status"][0] == methods.SCF_CONVERGED
    assert abs(rec["e_total"][0] - plain["e_total"][0]) < 1e-8


# ---- one call, two topologies, every second entry NULL -------------------------------------------------------------------
def mixed_batch():
    """8 waters and 8 water dimers.  Odd entries are the displaced water / the dimer of the cases above and restart from
    the reference's densities; even entries are other geometries and bring no density."""
    rng = np.random.default_rng(91)
    waters = [rc.displaced_water() if k % 2 else fragment_bohr([8, 1, 1], water_at(rng, [0.0, 0.0, 0.0])) for k in range(8)]
    dimers = [rc.dimer() if k % 2 else fragment_bohr([8, 1, 1, 8, 1, 1], np.vstack([water_at(rng, [0.0, 0.0, 0.0]), water_at(rng, [5.2 + 0.2 * k, 0.5, 0.1 * k])]))
              for k in range(8)]
    dw, dd = rc.case_start("displaced-rhf"), rc.case_start("dimer-ccpvdz")
    start = [[dw if k % 2 else None for k in range(8)], [dd if k % 2 else None for k in range(8)]]
    return [group_of(waters), group_of(dimers)], start


def mixed_batch_restart(start="cases"):
    groups, cases = mixed_batch()
    st = methods.ScfSettings(basis_set="cc-pvdz", **TIGHT)
    if start == "plain":
        recs = methods.run_hip_scf_groups(st, groups)
    else:
        recs = methods.run_hip_scf_groups(st, groups, initial_densities=cases if start == "cases" else [None, None])
    return np.concatenate(recs)


_MIXED = {}


def mixed(which):
    if which not in _MIXED:
        _MIXED[which] = mixed_batch_restart(which)
    return _MIXED[which]


def test_mixed_batch_null_entries_take_the_guess_and_the_others_restart():
    rec, plain, null = mixed("cases"), mixed("plain"), mixed("null")
    assert not np.any(rec["has_error"]) and not np.any(plain["has_error"]) and not np.any(null["has_error"])
    # a NULL array is the plain call
    assert np.array_equal(null["iterations"], plain["iterations"])
    assert np.max(np.abs(null["e_total"] - plain["e_total"])) < 1e-11
    # NULL entries: the plain entry's iteration counts, its energies to the batch-versus-single bound of test_gpu_parity.py
    even = np.arange(16) % 2 == 0
    assert np.array_equal(rec["iterations"][even], plain["iterations"][even])
    assert np.max(np.abs(rec["e_total"][even] - plain["e_total"][even])) < 1e-11
    # restarted entries: what the same restart gives alone in a call (the reference's densities here, the engine's in the
    # single calls above: the same start to 1e-9, so the same count; the energies to the parity bound)
    st = methods.ScfSettings(basis_set="cc-pvdz", **TIGHT)
    for name, first in (("displaced-rhf", 1), ("dimer-ccpvdz", 9)):
        alone, _, _, status = solve(st, [rc.case_fragment(name)], start=[rc.case_start(name)])
        assert status == 0
        for k in range(first, first + 8, 2):
            assert rec["iterations"][k] == alone["iterations"][0], (name, k)
            assert abs(rec["e_total"][k] - alone["e_total"][0]) < 1e-11, (name, k)
        assert alone["iterations"][0] == single_restart(name)[0]["iterations"][0]
        assert abs(alone["e_total"][0] - single_restart(name)[0]["e_total"][0]) < 1e-8


@pytest.mark.parametrize("route", ["chunked", "narrow"])
def test_mixed_batch_on_the_chunked_route_and_the_256_thread_kernels(route, tmp_path):
    """chunked: MQC_HIP_HBM_BUDGET_GB = 0.03 (32 MB) holds two cc-pVDZ dimers (31 n^2 doubles of SCF matrices + the
    1176^2 pair matrix = 11.7 MB each), so the eight dimers run as four chunks, each with its own mix of restarted and
    NULL entries.  narrow: MQC_HIP_SCF_WIDE_MAX = 0 sends the batch through the 256-thread build of the SCF kernels."""
    env = dict(os.environ)
    env.update({"chunked": {"MQC_HIP_HBM_BUDGET_GB": "0.03"}, "narrow": {"MQC_HIP_SCF_WIDE_MAX": "0"}}[route])
    out = str(tmp_path / "restart.json")
    p = subprocess.run([sys.executable, "-m", "tests.restart_child", out], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    got = json.load(open(out))
    rec = mixed("cases")
    assert not any(got["err"])
    assert got["it"] == [int(v) for v in rec["iterations"]]
    assert np.max(np.abs(np.array(got["e"]) - rec["e_total"])) < 1e-11


def test_spin_densities_come_back_in_the_callers_order():
    """The driver runs a batch in the order of compactness (nuclear repulsion, most compact first) and hands every answer
    back to the caller's slot.  Three water monomers in STO-3G (n = 7), O-H lengths 2.0, 1.8 and 1.6 bohr, passed least
    compact first -- the reverse of the order they run in -- and forced unrestricted: each fragment's spin densities,
    total density and energy are those of the same fragment alone in a call.  Bounds: the energies to the
    batch-versus-single bound of test_gpu_parity.py; the densities to 100 x D_TOL (a run ends once an iteration moves
    the density by less than D_TOL rms, so two runs of one fragment that differ in rounding agree far inside that,
    while neighbouring fragments' densities differ in the second decimal)."""
    st = methods.ScfSettings(basis_set="sto-3g", unrestricted=True, **TIGHT)
    half = np.deg2rad(104.5) / 2.0
    frags = [fragment_bohr([8, 1, 1], [[0.0, 0.0, 0.0], [0.0, r * np.sin(half), r * np.cos(half)], [0.0, -r * np.sin(half), r * np.cos(half)]])
             for r in (2.0, 1.8, 1.6)]
    rec, dens, spin, status = solve(st, frags, spin=True)
    assert status == 0 and not np.any(rec["has_error"])
    assert min(np.max(np.abs(dens[a] - dens[b])) for a, b in ((0, 1), (1, 2), (0, 2))) > 1e-3       # a swap would show
    for k, f in enumerate(frags):
        one, dens1, spin1, status = solve(st, [f], spin=True)
        assert status == 0 and not one["has_error"][0]
        assert abs(rec["e_total"][k] - one["e_total"][0]) < 1e-11, k
        assert np.max(np.abs(spin[k] - spin1[0])) < 100 * rc.D_TOL, k
        assert np.max(np.abs(dens[k] - dens1[0])) < 100 * rc.D_TOL, k
        assert np.max(np.abs(spin[k][0] + spin[k][1] - dens[k])) < 1e-13, k


# ---- validation ------------------------------------------------------------------------------------------------------------
def test_a_non_finite_density_fails_its_own_fragment_only():
    st = methods.ScfSettings(basis_set="6-31g", **TIGHT)
    rng = np.random.default_rng(17)
    frags = [fragment_bohr([8, 1, 1], water_at(rng, [0.0, 0.0, 0.0])) for _ in range(3)]
    plain, dens, _, _ = solve(st, frags)
    bad = dens[1].copy()
    bad[3, 7] = np.nan
    rec, _, _, status = solve(st, frags, start=[dens[0], bad, None])
    assert status == capi.ERR_VALIDATION
    assert rec["has_error"][1] and "non-finite" in message(rec, 1) and rec["scf_status"][1] == methods.SCF_NOT_RUN
    for k in (0, 2):
        assert not rec["has_error"][k] and abs(rec["e_total"][k] - plain["e_total"][k]) < 1e-9
    assert rec["iterations"][0] == 2 and rec["iterations"][2] == plain["iterations"][2]
    # the Python layer refuses a density of the wrong size before the engine reads past its end
    with pytest.raises(ValueError):
        solve(st, frags, start=[dens[0][:5, :5], None, None])


@pytest.mark.parametrize("kw, gradient", [(dict(basis_set="sto-3g", functional="tpss"), True),
                                          (dict(basis_set="sto-3g", functional="wb97x", density_fitting=True, aux_basis_set=wc.AUX), False)],
                         ids=["tpss-gradient", "wb97x-df"])
def test_refusals_are_those_of_the_plain_entry(kw, gradient):
    st = methods.ScfSettings(**kw)
    g = group_of([rc.water()])
    s0, s1 = [], []
    a = methods.run_hip_scf_groups(st, [g], want_gradient=gradient, status_out=s0)[0]
    b = methods.run_hip_scf_groups(st, [g], want_gradient=gradient, status_out=s1, initial_densities=[[np.eye(7)]])[0]
    assert s0[0] == s1[0] == capi.ERR_UNSUPPORTED
    assert a["has_error"][0] and b["has_error"][0] and message(a, 0) == message(b, 0)


# ---- callers ---------------------------------------------------------------------------------------------------------------
def iterations_of(run):
    methods.get_stats()                      # reading resets the counters
    out = run()
    return out, int(methods.get_stats().scf_iterations_total)


def test_fmo2_restart_gives_the_same_energy_in_no_more_iterations():
    system, st = wc.fmo_df_rks_system(), wc.fmo_df_rks_settings()
    plain, it_plain = iterations_of(lambda: fmo.run_fmo2(system, st, expansion="fmo"))
    again, it_again = iterations_of(lambda: fmo.run_fmo2(system, st, expansion="fmo", restart=True))
    print("FMO2 (H2O)8 DF-B3LYP: scf_iterations_total %d plain, %d with restart; dE = %.2e" % (it_plain, it_again, again.energy - plain.energy))
    assert plain.converged and again.converged and not again.errors
    assert abs(again.energy - plain.energy) < 2e-9
    assert again.outer_iterations == plain.outer_iterations
    assert it_again <= it_plain


def test_mbe_restart_gives_the_same_energies_in_no_more_iterations():
    system = w3_system()
    st = methods.ScfSettings(basis_set="6-31g", energy_tol=1e-10, density_tol=1e-8, guess="gwh")
    plain, it_plain = iterations_of(lambda: mbe.run_mbe(system, st, level=2))
    again, it_again = iterations_of(lambda: mbe.run_mbe(system, st, level=2, restart=True))
    print("MBE2 (H2O)3 RHF/6-31G: scf_iterations_total %d plain, %d with restart" % (it_plain, it_again))
    assert not plain.errors and not again.errors
    assert np.max(np.abs(again.energies - plain.energies)) < 1e-8
    assert abs(mbe.compute_mbe(again.terms, again.energies)[0] - mbe.compute_mbe(plain.terms, plain.energies)[0]) < 1e-8
    assert it_again <= it_plain
    assert set(again.densities) == set(map(tuple, again.terms))
    # a trajectory caller hands the densities back: every term is then a fixed point
    third = mbe.run_mbe(system, st, level=2, initial_densities=again.densities)
    assert np.all(third.iterations == 2) and np.max(np.abs(third.energies - plain.energies)) < 1e-8
