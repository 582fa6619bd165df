"""The numpy RI-MP2 reference the GPU tests compare against (tests/rimp2_reference.py), checked on its own, and the host
side of the feature: the frozen-core table and the assembly of run_mbe_rimp2 with a fake solver.  No GPU."""
import numpy as np
import pytest

from metalquicha_amd import mbe, methods
from metalquicha_amd.methods import ScfSettings, frozen_core_count
from oracle import scf_oracle as so
from tests import rimp2_reference as ref
from tests import workload_cases as wc
from tests.helpers import fragment_bohr, oracle_mol, w3_system

H2 = fragment_bohr([1, 1], [[0.0, 0.0, 0.0], [0.0, 0.0, 1.4]])
WATER = fragment_bohr([8, 1, 1], wc.DF_GRAD_XYZ)


def test_ri_agrees_with_conventional_mp2_on_h2():
    mol, aux = oracle_mol("sto-3g", H2), oracle_mol(wc.AUX, H2)
    B = so.df_tensor(mol, aux)
    o = so.run_rhf(mol, 2, 200, 1e-12, 1e-10, aux=aux, B=B)
    assert o.converged
    ri = ref.pair_energies(B, o.C, o.eps, 1)
    conv = ref.conventional_mp2(so.eri4(mol), o.C, o.eps, 1)
    print("H2 STO-3G: RI %.10f conventional %.10f" % (sum(ri), sum(conv)))
    assert abs(sum(ri) - sum(conv)) < 1e-5, sum(ri) - sum(conv)
    assert sum(ri) < 0.0
    # one occupied orbital: V_ab - V_ba vanishes term by term
    assert ri[1] == 0.0 and conv[1] == 0.0


def test_water_values_and_square_root_invariance():
    mol, aux = oracle_mol("cc-pvdz", WATER), oracle_mol(wc.AUX, WATER)
    B = so.df_tensor(mol, aux)
    o = so.run_rhf(mol, 10, 200, 1e-12, 1e-10, aux=aux, B=B)
    assert o.converged
    e_os, e_ss = ref.pair_energies(B, o.C, o.eps, 5, 1)
    assert (5 - 1, o.C.shape[1] - 5, B.shape[2]) == (4, 19, 126)
    assert abs(e_os - (-0.153174310268)) < 1e-10, e_os
    assert abs(e_ss - (-0.051324351783)) < 1e-10, e_ss
    # any square root of the metric gives the same (ia|jb): the Cholesky factor the engine fits with
    c_os, c_ss = ref.pair_energies(ref.cholesky_df_tensor(mol, aux), o.C, o.eps, 5, 1)
    assert abs(c_os - e_os) < 1e-12 and abs(c_ss - e_ss) < 1e-12, (c_os - e_os, c_ss - e_ss)
    # the module's front door gives the same numbers
    r = ref.rimp2_cached(WATER, "cc-pvdz", wc.AUX)
    assert abs(r["e_os"] - e_os) < 1e-12 and abs(r["e_ss"] - e_ss) < 1e-12 and abs(r["scf"] - o.energy) < 1e-12
    # all-electron: one more occupied orbital, more correlation
    a_os, a_ss = ref.pair_energies(B, o.C, o.eps, 5, 0)
    assert a_os < e_os and a_ss < e_ss


def test_frozen_core_count():
    assert frozen_core_count([1]) == 0 and frozen_core_count([1, 1]) == 0 and frozen_core_count([2]) == 0
    assert frozen_core_count([8]) == 1 and frozen_core_count([8, 1, 1]) == 1 and frozen_core_count([3]) == 1 and frozen_core_count([10]) == 1
    assert frozen_core_count([11]) == 5 and frozen_core_count([18]) == 5
    assert frozen_core_count([19]) == 9 and frozen_core_count([36]) == 9
    assert frozen_core_count([8, 1, 1, 8, 1, 1]) == 2
    assert frozen_core_count([8, 1, 1, 8, 1, 1], ghost=[False, False, False, True, True, True]) == 1
    assert frozen_core_count([11, 17], ghost=[True, False]) == 5
    with pytest.raises(ValueError):
        frozen_core_count([37])


def test_energy_record_defaults():
    e = methods.EnergyT(scf=-1.5)
    assert e.mp2 == 0.0 and e.total() == -1.5
    e = methods.EnergyT(scf=-1.5, mp2_os=-0.2, mp2_ss=-0.05)
    assert abs(e.mp2 + 0.25) < 1e-15 and abs(e.total() + 1.75) < 1e-15
    assert methods.CalculationResult().has_mp2 is False


def _fake_solver(fail_term_size=None):
    """Stands in for methods.run_hip_rimp2_groups: energies that are closed forms of the fragment's geometry."""
    def solve(groups):
        recs, os_, ss_, done = [], [], [], []
        for g in groups:
            m = g.xyz.shape[0]
            rec = np.zeros(m, dtype=methods._RES_DTYPE)
            r2 = np.sum(g.xyz ** 2, axis=(1, 2))
            rec["e_total"] = -float(np.sum(g.element_numbers)) - 1e-3 * r2
            rec["iterations"] = 7
            a = -0.01 * len(g.element_numbers) - 1e-5 * r2
            b = -0.004 * len(g.element_numbers) - 2e-5 * r2
            d = np.ones(m, dtype=np.int32)
            if fail_term_size == len(g.element_numbers):
                d[0] = 0; a[0] = 0.0; b[0] = 0.0
            recs.append(rec); os_.append(a); ss_.append(b); done.append(d)
        return recs, os_, ss_, done
    return solve


def test_run_mbe_rimp2_assembly_and_scs():
    system = w3_system()
    st = ScfSettings(basis_set="6-31g", density_fitting=True, aux_basis_set=wc.AUX)
    run = mbe.run_mbe_rimp2(system, st, level=3, solver=_fake_solver())
    assert not run.errors and len(run.terms) == 7
    assert run.correlation_os is not None and run.correlation_ss is not None and run.gradient is None
    scf = run.energies - run.correlation_os - run.correlation_ss
    xyz = np.ascontiguousarray(system.coordinates.T)
    for k, t in enumerate(run.terms):
        atoms = np.concatenate([system.monomers[m] for m in t])
        r2 = float(np.sum(xyz[atoms] ** 2))
        assert abs(scf[k] - (-float(np.sum(system.element_numbers[atoms])) - 1e-3 * r2)) < 1e-12
        assert abs(run.correlation_os[k] - (-0.01 * len(atoms) - 1e-5 * r2)) < 1e-15
        assert abs(run.correlation_ss[k] - (-0.004 * len(atoms) - 2e-5 * r2)) < 1e-15
        assert run.iterations[k] == 7
    # full order: the expansion of the sum is the whole system's value
    total, _, _ = mbe.compute_mbe(run.terms, run.energies)
    assert abs(total - run.energies[run.terms.index((0, 1, 2))]) < 1e-10
    # scs scales the parts before the sum
    scs = mbe.run_mbe_rimp2(system, st, level=3, solver=_fake_solver(), scs=(1.2, 1.0 / 3.0))
    assert np.max(np.abs(scs.correlation_os - 1.2 * run.correlation_os)) < 1e-15
    assert np.max(np.abs(scs.correlation_ss - run.correlation_ss / 3.0)) < 1e-15
    assert np.max(np.abs(scs.energies - (scf + 1.2 * run.correlation_os + run.correlation_ss / 3.0))) < 1e-12
    # two ranks: disjoint zero-padded shares that add up to the one-rank vectors
    parts = [mbe.run_mbe_rimp2(system, st, level=3, rank=r, world=2, solver=_fake_solver()) for r in range(2)]
    assert np.max(np.abs(parts[0].energies + parts[1].energies - run.energies)) < 1e-12
    assert np.max(np.abs(parts[0].correlation_os + parts[1].correlation_os - run.correlation_os)) < 1e-15
    assert sorted(list(parts[0].owned) + list(parts[1].owned)) == list(range(7))


def test_run_mbe_rimp2_term_without_mp2_is_an_error():
    system = w3_system()
    st = ScfSettings(basis_set="6-31g", density_fitting=True, aux_basis_set=wc.AUX)
    run = mbe.run_mbe_rimp2(system, st, level=2, solver=_fake_solver(fail_term_size=6))
    assert len(run.errors) == 1 and "RI-MP2" in run.errors[0]
    bad = [k for k, t in enumerate(run.terms) if len(t) == 2 and run.energies[k] == 0.0]
    assert len(bad) == 1 and run.correlation_os[bad[0]] == 0.0 and run.correlation_ss[bad[0]] == 0.0


def test_run_mbe_fields_untouched():
    fields = [f for f in mbe.MbeRun.__dataclass_fields__]
    assert fields[:7] == ["terms", "energies", "iterations", "owned", "errors", "gradient", "densities"]
    r = mbe.MbeRun([], np.zeros(0), np.zeros(0), np.zeros(0), [])
    assert r.correlation_os is None and r.correlation_ss is None
