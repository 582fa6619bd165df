"""Stage test of the exchange-correlation quadrature (mqc_hip_xc_batch: the SCF driver's own plan, grid, weights, radial
cache and launch_xc, on given densities) against the CPU oracle, element by element, for one case per dispatch bucket
of kern_xc.hip (tests/xc_stage_cases.py) on every route the environment switches select.

Why: the SCF energy is stationary in the density, so a V_xc that is wrong by eps moves a converged energy by O(eps^2);
the `< 1e-8 Eh` energy tests cannot see a 1e-6 slip in one output tile or one spin block.  Here every element of V_xc is
compared, with E_xc, the integrated electron number, and -- independent of the oracle's closed forms -- the kernel's own
E_xc against its own V_xc by a central difference.

Tolerances (xc_stage_cases.bounds): eps_ref x 50, never looser than 1e-10 max(1, max |V_ref|) for V_xc and 1e-10 for the
scalars; the margin's derivation is next to MARGIN there.  eps_ref = the reference's own noise floor, the larger of block
4096 against block 509 and against an evaluation whose sums over the grid run in np.longdouble
(tests/test_xc_stage_cases.py, measure_eps_ref: one point per block up to n = 24, 127 above), worst case of the class on
the CPU.  `kernel` = worst |V_gpu - V_ref| over the cases of the class on that route, measured on an MI355X:

  class  eps_ref V (worst case)      recorded  bound V   kernel: default  tile     pipe     no-radial-cache  narrow-tile  no-radial-lds  no-fast-slab
  lda    2.7e-15 (oh-w5-dz-usvwn)    3e-15     1.5e-13           5.3e-15  4.4e-15  2.8e-15  4.4e-15          5.8e-15      4.4e-15        3.8e-15
  gga    6.2e-15 (w1-sto3g-pbe)      7e-15     3.5e-13           8.0e-15  5.3e-15  4.9e-15  6.7e-15          7.6e-15      6.7e-15        5.8e-15
  mgga   1.3e-15 (w1-dz-tpss)        7e-15     3.5e-13           1.4e-14  -        -        -                -            -              -
  rsh    8.9e-16 (w1-dz-cam-b3lyp)   7e-15     3.5e-13           4.4e-15  4.9e-15  -        5.8e-15          2.9e-15      4.4e-15        4.4e-15
  (-: the route's switches do not change that class's kernel; it runs on the default route only)

  scalars, per ten electrons: eps_ref E_xc 3.6e-15, N_e 5.3e-15; recorded 4e-15 and 6e-15; bounds 2e-13 and 3e-13 for one
  water.  Kernel: |dE| at most 0.39 of its bound on every route (1.6e-12 against 4.2e-12 for (H2O)21, 210 electrons),
  |dN| at most 6.5e-13 (same case, bound 6.3e-12).  The kernels sit at the reference's own noise floor: no route needs
  more than a twentieth of its bound, none comes near the 1e-10 cap.
  E_xc against V_xc by central differences (theta = 3e-5 in all three cases): kernel residuals of 7e-16 to 7e-15 over
  three runs (atomic adds: they differ from run to run) against oracle residuals 5.3e-15 (pbe), 1.7e-15 (unrestricted
  pbe, alpha), 7.3e-15 (tpss) and a bound of 2e-13.

No grid point is masked: points within a factor 10 of DENS_THRESHOLD carry no weight a double can see
(test_xc_stage_cases.test_low_density_points_carry_no_weight)."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from metalquicha_amd import capi
from oracle import scf_oracle as so
from tests import stages, xc_stage_cases as xs
from tests.helpers import fragment_bohr, oracle_mol, water_at

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def _setup(name, shift=0.0, seed_offset=0):
    case = xs.BY_NAME[name]
    frag = xs.fragment(case, shift)
    mol = oracle_mol(case.basis, frag)
    S, _, _ = so.int1e(mol)
    D, C = xs.density(case, frag, S, mol, seed_offset)
    return case, frag, mol, D, C


@functools.lru_cache(maxsize=None)
def _reference(name, shift=0.0, seed_offset=0):
    """The oracle's (E_xc, N_e, V_xc) of a case: computed once, shared by every route and test, never modified."""
    case, frag, mol, D, _ = _setup(name, shift, seed_offset)
    e, nel, V = xs.reference(case, xs.oracle_for(case, mol), D)
    V.setflags(write=False)
    return e, nel, V


_ROUTE_OUTCOME = {}       # route -> results of its child, or the text of its failure: a child is started ONCE


def _route(route, tmp):
    """One child process per route (the switches are read once per process): every case of the route, results from a
    file.  The outcome is kept, a failure included: after a child that failed, faulted or ran into its time limit every
    other test of the route fails from the stored text and nothing is started on the GPU again."""
    if route not in _ROUTE_OUTCOME:
        out = os.path.join(tmp, "xc_stage_%s.npz" % route)
        env = dict(os.environ, **xs.ROUTES[route])
        try:
            p = subprocess.run([sys.executable, "-m", "tests.xc_stage_child", route, out], cwd=ROOT, env=env, capture_output=True,
                               text=True, timeout=600)
            if p.returncode != 0:
                _ROUTE_OUTCOME[route] = "route %s: child failed (%d)\n%s\n%s" % (route, p.returncode, p.stdout[-2000:], p.stderr[-4000:])
            else:
                info = json.loads(p.stdout.strip().splitlines()[-1])
                if info["cases"] != [c.name for c in xs.route_cases(route)]:
                    _ROUTE_OUTCOME[route] = "route %s: child ran %s" % (route, info["cases"])
                else:
                    _ROUTE_OUTCOME[route] = dict(np.load(out))
        except Exception as exc:       # the time limit, unreadable output: kept like any other failure
            _ROUTE_OUTCOME[route] = "route %s: %r" % (route, exc)
    got = _ROUTE_OUTCOME[route]
    if isinstance(got, str):
        pytest.fail(got)
    return got


def _compare(case, e, nel, V, ref, nelec, label):
    e0, n0, V0 = ref
    bv, be, bn = xs.bounds(case, float(np.max(np.abs(V0))), nelec)
    assert V.shape == V0.shape
    assert not np.isnan(V).any(), "%s: NaN in V_xc" % label
    dv = float(np.max(np.abs(V - V0)))
    asym = float(np.max(np.abs(V - np.swapaxes(V, -1, -2))))
    print("XCSTAGE %s class=%s n=%d dV=%.3e bound=%.3e asym=%.1e dE=%.3e boundE=%.3e dN=%s" % (
        label, xs.case_class(case), case.n, dv, bv, asym, abs(e - e0), be, "%.3e" % abs(nel - n0)))
    assert dv <= bv, "%s: V_xc off by %.3e (bound %.3e) at %s" % (label, dv, bv, np.unravel_index(np.argmax(np.abs(V - V0)), V.shape))
    # V_xc = A + A^T is formed on the host from the kernels' accumulator A, as scf_step_kernel forms it on the device:
    # the sum is symmetric by construction, so this guards the stage entry's own transpose, not the kernels (an error
    # of A, antisymmetric or not, shows in the comparison with the reference above: A^T enters every element)
    assert asym <= bv
    assert abs(e - e0) <= be, "%s: E_xc off by %.3e (bound %.3e)" % (label, abs(e - e0), be)
    assert abs(nel - n0) <= bn, "%s: N_e off by %.3e (bound %.3e)" % (label, abs(nel - n0), bn)
    # the true electron count, to the grid's own accuracy: that accuracy is the oracle's error, not the kernel's
    assert abs(nel - nelec) <= abs(n0 - nelec) + bn


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return str(tmp_path_factory.mktemp("xc_stage"))


_PAIRS = [(r, c.name) for r in xs.ROUTES for c in xs.route_cases(r)]


@pytest.mark.parametrize("route,name", _PAIRS, ids=["%s-%s" % p for p in _PAIRS])
def test_quadrature_matches_oracle(route, name, tmp):
    case, frag, _, _, _ = _setup(name)
    got = _route(route, tmp)
    _compare(case, float(got["E:" + name]), float(got["N:" + name]), got["V:" + name], _reference(name), float(frag.nelec),
             "%s/%s" % (route, name))


def test_batch_of_three_and_batch_of_one(tmp):
    """m = 3 dimers of one topology (three geometries, three densities) against the oracle, and m = 1 of the first: the
    first fragment agrees between the calls to summation-order noise (the grid of the batch is dealt to other workgroup
    counts), and no other fragment equals it."""
    name = xs.BATCH_CASE.name
    sets = [_setup(name, sh, k) for k, sh in enumerate(xs.BATCH_SHIFTS)]
    case = sets[0][0]
    frags = [s[1] for s in sets]
    D = np.stack([s[3] for s in sets])
    e3, n3, V3 = stages.xc_batch(case.basis, frags, case.functional, D, case.level)
    e1, n1, V1 = stages.xc_batch(case.basis, frags[:1], case.functional, D[:1], case.level)
    for k, sh in enumerate(xs.BATCH_SHIFTS):
        _compare(case, e3[k], n3[k], V3[k], _reference(name, sh, k), float(frags[k].nelec), "batch3[%d]" % k)
    _compare(case, e1[0], n1[0], V1[0], _reference(name, 0.0, 0), float(frags[0].nelec), "batch1")
    bv, be, bn = xs.bounds(case, float(np.max(np.abs(V1))), float(frags[0].nelec))
    assert np.max(np.abs(V3[0] - V1[0])) <= bv and abs(e3[0] - e1[0]) <= be and abs(n3[0] - n1[0]) <= bn
    for k in (1, 2):
        assert np.max(np.abs(V3[k] - V3[0])) > 1e-6 and abs(e3[k] - e3[0]) > 1e-8


def _rotated(case, D, C, o, v, theta):
    """The density with occupied orbital o rotated into virtual v by theta (alpha spin when unrestricted): positive for
    every theta, and D(theta) - D(-theta) = sin(2 theta) delta exactly, delta = occ (c_o c_v^T + c_v c_o^T)."""
    occ = 1.0 if case.unrestricted else 2.0
    co, cv = C[:, o], C[:, v]
    new = np.cos(theta) * co + np.sin(theta) * cv
    d = occ * (np.outer(new, new) - np.outer(co, co))
    out = D.copy()
    if case.unrestricted:
        out[0] += d
    else:
        out += d
    return out, occ * (np.outer(co, cv) + np.outer(cv, co))


@pytest.mark.parametrize("name", ["w1-dz-pbe", "oh-dz-upbe", "w1-dz-tpss"])
def test_energy_and_potential_are_consistent(name):
    """E_xc[D(theta)] - E_xc[D(-theta)] = sin(2 theta) tr(delta V_xc[D]) + O(theta^3), the kernel's energy against the
    kernel's potential: a wrong derivative shows even where oracle and kernel share a transcription mistake.  theta is
    the oracle's choice -- where its own central difference meets its own trace best -- and the bound is that residual
    x 10 (the kernel's truncation error is the same function's; its rounding error is another draw of the oracle's),
    not below the bound of E_xc itself and never looser than 1e-10."""
    case, frag, mol, D, C = _setup(name)
    occ = xs.occupations(case, frag)
    o, v = 0, (occ[0] if case.unrestricted else occ) + 1
    ref = xs.oracle_for(case, mol)
    V0 = _reference(name)[2]

    def trace(V, delta):
        return float(np.sum(delta * (V[0] if case.unrestricted else V)))

    best = None
    for theta in (1e-2, 3e-3, 1e-3, 3e-4, 1e-4, 3e-5):
        dp, delta = _rotated(case, D, C, o, v, theta)
        dm, _ = _rotated(case, D, C, o, v, -theta)
        res = abs(xs.reference(case, ref, dp)[0] - xs.reference(case, ref, dm)[0] - np.sin(2 * theta) * trace(V0, delta))
        if best is None or res < best[1]:
            best = (theta, res)
    theta, res = best
    dp, delta = _rotated(case, D, C, o, v, theta)
    dm, _ = _rotated(case, D, C, o, v, -theta)
    e, _, V = stages.xc_batch(case.basis, [frag] * 3, case.functional, np.stack([D, dp, dm]), case.level, case.unrestricted)
    got = abs(e[1] - e[2] - np.sin(2 * theta) * trace(V[0], delta))
    # floor: the bound of E_xc itself (eps_ref x MARGIN, xc_stage_cases.bounds) -- the smallest of six oracle residuals is
    # rounding noise and can come out luckily small; a 1e-6 relative error of V_xc still shows as 2 theta slope 1e-6,
    # some 1e-11 here, fifty times the floor
    floor = xs.bounds(case, 1.0, float(frag.nelec))[1]
    bound = min(max(10.0 * res, floor), 1e-10)
    print("XCSTAGE consistency %s theta=%.0e oracle residual=%.3e kernel residual=%.3e bound=%.3e slope=%.3e" % (
        name, theta, res, got, bound, trace(V[0], delta)))
    assert abs(trace(V0, delta)) > 1e-4          # a direction the energy does depend on
    assert got <= bound


def test_refusals():
    """Null pointers, an unknown functional, m < 1, and what an SCF of the same settings refuses: n_ao > 256, meta-GGA and
    unrestricted Kohn-Sham above 140, more than 64 atoms.  Each returns its error and writes nothing."""
    import ctypes as C
    rng = np.random.default_rng(5)
    case, frag, _, D, _ = _setup("w1-dz-pbe")

    def refused(code, text, *a, **kw):
        with pytest.raises(capi.HipBackendError) as ei:
            stages.xc_batch(*a, **kw)
        assert ei.value.code == code and text in ei.value.message, ei.value.message

    refused(capi.ERR_VALIDATION, "null", case.basis, [frag], None, D[None], 1)
    refused(capi.ERR_UNSUPPORTED, "not available", case.basis, [frag], "m06-l", D[None], 1)
    refused(capi.ERR_VALIDATION, "no grid part", case.basis, [frag], "", D[None], 1)
    m = stages._marshal(case.basis, frag)
    lib, ctx = capi.load_library(), capi.get_context()
    one = np.zeros(1)
    V = np.full_like(D, np.nan)
    args = [ctx, 1, C.byref(m.mol), C.byref(m.bas), b"pbe", 1, 0, capi.dptr(D), capi.dptr(one), capi.dptr(one), capi.dptr(V)]
    for k in (0, 2, 3, 4, 7, 8, 9, 10):
        bad = list(args); bad[k] = None
        assert lib.mqc_hip_xc_batch(*bad) == capi.ERR_VALIDATION
    for nfrag in (0, -1):
        bad = list(args); bad[1] = nfrag
        assert lib.mqc_hip_xc_batch(*bad) == capi.ERR_VALIDATION
    assert np.isnan(V).all()

    def waters(k, dx=5.6):
        return fragment_bohr([8, 1, 1] * k, np.vstack([water_at(rng, [dx * i, 0.0, 0.0]) for i in range(k)]))

    def zeros(f, basis, uks=False):
        n = oracle_mol(basis, f).nao
        return np.zeros((1, 2, n, n) if uks else (1, n, n))

    w11, w6, w22 = waters(11), waters(6), waters(22)
    refused(capi.ERR_UNSUPPORTED, "n_ao <= 256", "cc-pvdz", [w11], "pbe", zeros(w11, "cc-pvdz"), 1)                  # n = 264
    refused(capi.ERR_UNSUPPORTED, "meta-GGA", "cc-pvdz", [w6], "tpss", zeros(w6, "cc-pvdz"), 1)                       # n = 144
    refused(capi.ERR_UNSUPPORTED, "unrestricted Kohn-Sham", "cc-pvdz", [w6], "pbe", zeros(w6, "cc-pvdz", True), 1, True)
    refused(capi.ERR_UNSUPPORTED, "64 atoms", "sto-3g", [w22], "svwn", zeros(w22, "sto-3g"), 1)                       # 66 atoms
    oh = xs.fragment(xs.BY_NAME["oh-dz-upbe"])
    refused(capi.ERR_VALIDATION, "open-shell", "cc-pvdz", [oh], "pbe", zeros(oh, "cc-pvdz"), 1)
    refused(capi.ERR_VALIDATION, "elements of the first", "cc-pvdz", [frag, oh], "pbe", np.zeros((2, 24, 24)), 1)
