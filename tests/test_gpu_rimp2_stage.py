"""Stage tests of RI-MP2: mqc_hip_rimp2_stage (the three kernels of kern_mp2.hip, once, on given tensors) against a plain
numpy reference, element by element -- Bia with its padding, every pair's partial, the fragment energies -- at one case
per route of the transform and per edge of the pair kernel (tests/rimp2_stage_cases.py), on the routes the environment
switch selects: default and no-clds (MQC_HIP_MP2_C_LDS=0, the L2 kernel with more than one wave).

Why: every other RI-MP2 test is two scalars of a molecule at 1e-8 Eh with at most 12 occupied orbitals, 72 functions and
70 fragments.  None of them runs a wave's second auxiliary row (the register prefetch, the reuse of the row buffer and
of T behind a wave-level fence, the walk into the zero padding rows), a second occupied tile or pass, a fragment whose
orthogonaliser dropped modes, or a pool that another shape left behind.  Every case names the route it must land on and
the test asserts the route the entry reports; the entry poisons the stage's pool before the launch.

Tolerances (rimp2_stage_cases.py).  Integer family: Bia EXACTLY equal, padding included.  Everything else: MARGIN (50,
derivation next to the import there) x eps_ref, never looser than 1e-11 max(1, max |ref|) for elements (Bia, pair
partials) and 1e-8 max(1, max |e_ref|) for the energies; eps_ref, per case and per quantity, is the larger of the
float64 reference against np.longdouble and against float64 with the auxiliary index reversed, not below one unit in the
last place of the largest reference value.

Measured on an MI355X (59 passed in 8.5 s), one row per transform instance, wave count and family; `rows` = compared
fragments that land on it (cases, capped runs, the 300-fragment batch, the ragged batch, the stale-pool pair); eps_ref,
bound and kernel deviation are those of the fragment with the worst ratio of deviation to bound.  Bia in absolute terms
(max |Bia| is 0.3 .. 1.3 in the real family; the integer family is compared exactly), pair partials and energies
relative to the largest reference value of the fragment:

  route    instance     waves family rows  Bia: eps_ref bound    kernel  | part/max: eps_ref bound    kernel  | e/max: eps_ref bound    kernel
  default  prefetch     8     int     19   exact    0        0        | 2.2e-16  1.1e-14  3.9e-16 | 2.2e-16  1.1e-14  2.1e-16
  default  prefetch     8     real    19   3.4e-16  1.7e-14  5.6e-16 | 2.2e-16  1.1e-14  3.7e-16 | 2.2e-16  1.1e-14  1.8e-16
  default  prefetch     4     int      1   exact    0        0        | 2.2e-16  1.1e-14  1.6e-16 | 2.2e-16  1.1e-14  0.0e+00
  default  prefetch     4     real     1   3.9e-16  1.9e-14  0.0e+00 | 2.2e-16  1.1e-14  1.6e-16 | 2.2e-16  1.1e-14  0.0e+00
  default  no-prefetch  4     int      5   exact    0        0        | 2.2e-16  1.1e-14  2.8e-16 | 2.2e-16  1.1e-14  9.4e-17
  default  no-prefetch  4     real     5   3.2e-16  1.6e-14  0.0e+00 | 2.2e-16  1.1e-14  1.8e-16 | 2.2e-16  1.1e-14  0.0e+00
  default  prefetch     2     int      1   exact    0        0        | 2.2e-16  1.1e-14  9.1e-17 | 9.8e-16  4.9e-14  0.0e+00
  default  prefetch     2     real     1   6.7e-16  3.3e-14  6.7e-16 | 3.4e-16  1.7e-14  4.1e-16 | 5.9e-16  3.0e-14  1.5e-16
  default  no-prefetch  2     int      2   exact    0        0        | 2.2e-16  1.1e-14  1.6e-16 | 2.2e-16  1.1e-14  4.7e-17
  default  no-prefetch  2     real     2   3.7e-16  1.9e-14  6.7e-16 | 2.6e-16  1.3e-14  3.9e-16 | 2.2e-16  1.1e-14  1.2e-16
  default  l2           1     int      9   exact    0        0        | 2.2e-16  1.1e-14  2.1e-16 | 7.4e-16  3.7e-14  2.0e-16
  default  l2           1     real     9   7.8e-16  3.9e-14  1.0e-15 | 1.3e-15  6.5e-14  1.8e-15 | 2.2e-16  1.1e-14  1.4e-16
  no-clds  l2           4     int      3   exact    0        0        | 2.2e-16  1.1e-14  3.2e-16 | 2.2e-16  1.1e-14  0.0e+00
  no-clds  l2           4     real     3   4.4e-16  2.2e-14  5.6e-16 | 3.1e-16  1.5e-14  3.1e-16 | 2.2e-16  1.1e-14  0.0e+00
  no-clds  l2           2     int      1   exact    0        0        | 2.2e-16  1.1e-14  1.5e-16 | 4.0e-16  2.0e-14  1.3e-16
  no-clds  l2           2     real     1   7.2e-16  3.6e-14  5.6e-16 | 7.6e-16  3.8e-14  7.0e-16 | 1.1e-15  5.3e-14  3.9e-16

  No element of any case is wrong.  Every deviation sits at the reference's own noise floor: no row above exceeds
  2 x eps_ref or needs more than a twenty-fifth of its bound.  The capped runs (3 .. 24 rows per wave) and the launcher's own
  three-row grid at 300 fragments equal the one-row runs bit for bit; the ragged batch equals its fragments run alone
  bit for bit; a pool left behind by (48, 10, 252, 2) changes no bit of (13, 5, 126, 1).  Mutants tried by hand on
  scratch builds (profiles/r13_b_rimp2_stage_mutants.txt): the prefetch guarded by the current row, and the pass offset
  dropped from the Bia row, pass every earlier RI-MP2 test and fail here.

The full table, one row per run, is profiles/r13_a_rimp2_stage_deviations.txt."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from metalquicha_amd import capi
from tests import rimp2_stage_cases as rs, stages

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_ROUTE_OUTCOME = {}       # route -> results of its child, or the text of its failure: a child is started ONCE
_ABNORMAL = []            # a child killed by a signal or by its time limit: no other route's child is started after it


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return str(tmp_path_factory.mktemp("rimp2_stage"))


def _route(route, tmp):
    """One child process per route (the switch is read once per process): every run of the route, results from a file.
    The outcome is kept, a failure included: after a child that failed, faulted or ran into its time limit every other
    test of the route fails from the stored text and nothing is started on the GPU again; after a child that was killed
    (a signal, the time limit) the other route does not start either."""
    if route not in _ROUTE_OUTCOME and _ABNORMAL:
        _ROUTE_OUTCOME[route] = "route %s: not started after %s" % (route, _ABNORMAL[0])
    if route not in _ROUTE_OUTCOME:
        out = os.path.join(tmp, "rimp2_stage_%s.npz" % route)
        env = {k: v for k, v in os.environ.items() if k != "MQC_HIP_MP2_C_LDS"}
        env.update(rs.ROUTES[route])
        try:
            p = subprocess.run([sys.executable, "-m", "tests.rimp2_stage_child", route, out], cwd=ROOT, env=env, capture_output=True,
                               text=True, timeout=300)
            if p.returncode != 0:
                _ROUTE_OUTCOME[route] = "route %s: child failed (%d)\n%s\n%s" % (route, p.returncode, p.stdout[-2000:], p.stderr[-4000:])
                if p.returncode < 0 or p.returncode > 128:
                    _ABNORMAL.append("route %s ended with status %d" % (route, p.returncode))
            else:
                info = json.loads(p.stdout.strip().splitlines()[-1])
                _ROUTE_OUTCOME[route] = dict(np.load(out)) if info["runs"] == rs.run_labels(route) else "route %s: child ran %s" % (route, info["runs"])
        except Exception as exc:       # the time limit, unreadable output: kept like any other failure
            _ROUTE_OUTCOME[route] = "route %s: %r" % (route, exc)
            if isinstance(exc, subprocess.TimeoutExpired):
                _ABNORMAL.append("route %s ran into its time limit" % route)
    got = _ROUTE_OUTCOME[route]
    if isinstance(got, str):
        pytest.fail(got)
    return got


def _get(got, label):
    rt = dict(zip(stages.RIMP2_ROUTE_FIELDS, (int(v) for v in got["R:" + label])))
    return got["E:" + label], got["P:" + label], got["B:" + label], rt


def _assert_route(label, c, rt, gx=None, rows=None):
    want = c.expected_route()
    assert {k: rt[k] for k in want} == want, "%s: the launcher reports %s, the case expects %s" % (label, rt, want)
    if gx is not None:
        assert (rt["gx"], rt["rows"]) == (gx, rows), "%s: gx = %d, %d rows per wave" % (label, rt["gx"], rt["rows"])


def _compare(label, c, fam, ref, e, part, bia, nmo=None):
    """One fragment against its reference: e (2,), part (npairs, 2), bia (no, napad, nvpad)."""
    nv = (c.n if nmo is None else nmo) - c.nocc
    B0 = rs.pad_bia(ref["Bia"], c)
    assert bia.shape == B0.shape and part.shape == ref["part"].shape and e.shape == (2,)
    nan = int(np.isnan(bia).sum()), int(np.isnan(part).sum()), int(np.isnan(e).sum())
    db, dp, de = (float(np.max(np.abs(a - b))) if a.size else 0.0 for a, b in ((bia, B0), (part, ref["part"]), (e, ref["e"])))
    bb = 0.0 if fam == "int" else rs.elem_bound(ref["eps_bia"], ref["Bia"])
    bp, be = rs.elem_bound(ref["eps_part"], ref["part"]), rs.energy_bound(ref["eps_e"], ref["e"])
    pad_ok = not bia[:, c.naux:, :].any() and not bia[:, :, nv:].any()
    print("RIMP2STAGE %s instance=%s waves=%d oc=%d passes=%d | Bia: eps_ref=%.3e bound=%.3e dev=%.3e max=%.3e | part: eps_ref=%.3e bound=%.3e "
          "dev=%.3e max=%.3e | e: eps_ref=%.3e bound=%.3e dev=%.3e max=%.3e" % (
              label, c.instance, c.waves, c.oc, c.passes, ref["eps_bia"], bb, db, float(np.max(np.abs(B0))), ref["eps_part"], bp, dp,
              float(np.max(np.abs(ref["part"]))), ref["eps_e"], be, de, float(np.max(np.abs(ref["e"])))))
    assert nan == (0, 0, 0), "%s: NaN in Bia, the partials, the energies: %s (elements read or left unwritten)" % (label, nan)
    assert pad_ok, "%s: the padding of Bia is not exactly zero" % label
    if fam == "int":
        assert np.array_equal(bia, B0), "%s: Bia differs at %s (off by %g)" % (label, np.unravel_index(np.argmax(np.abs(bia - B0)), bia.shape), db)
    else:
        assert db <= bb, "%s: Bia off by %.3e (bound %.3e) at %s" % (label, db, bb, np.unravel_index(np.argmax(np.abs(bia - B0)), bia.shape))
    assert dp <= bp, "%s: a pair partial off by %.3e (bound %.3e) at %s" % (label, dp, bp, np.unravel_index(np.argmax(np.abs(part - ref["part"])), part.shape))
    assert de <= be, "%s: a fragment energy off by %.3e (bound %.3e)" % (label, de, be)
    if c.no == 1:
        assert part[0, 1] == 0.0 and e[1] == 0.0, "%s: e_ss of a single occupied orbital is exactly zero" % label


_TRIPLES = [(c.route, c.name, f) for c in rs.CASES for f in rs.FAMILIES]


@pytest.mark.parametrize("route,name,fam", _TRIPLES, ids=["%s-%s-%s" % t for t in _TRIPLES])
def test_stage_matches_reference(route, name, fam, tmp):
    c = rs.BY_KEY[(route, name)]
    e, part, bia, rt = _get(_route(route, tmp), "%s/%s" % (name, fam))
    label = "%s/%s/%s" % (route, name, fam)
    _assert_route(label, c, rt, (c.napad + c.waves - 1) // c.waves, 1)
    _compare(label, c, fam, rs.reference_with_eps((route, name), fam), e[0], part[0], bia[0])


_ROWS = [(k[1], f, cap) for k in rs.ROWS_SHAPES for f in rs.FAMILIES for cap in rs.ROWS_CAPS]


@pytest.mark.parametrize("name,fam,cap", _ROWS, ids=["%s-%s-cap%d" % t for t in _ROWS])
def test_several_rows_per_wave(name, fam, cap, tmp):
    """workgroups_per_fragment = 1 and 2: every wave walks three rows or more (the prefetch of the next row, the reuse of
    the row buffer and of T, the padding rows on a later iteration).  Bit for bit the uncapped run, and the reference."""
    c = rs.BY_KEY[("default", name)]
    got = _route("default", tmp)
    e, part, bia, rt = _get(got, "rows/%s/%s/cap%d" % (name, fam, cap))
    e0, part0, bia0, rt0 = _get(got, "rows/%s/%s/cap0" % (name, fam))
    rows = -(-c.napad // (cap * c.waves))
    label = "rows/%s/%s/cap%d" % (name, fam, cap)
    _assert_route(label, c, rt, cap, rows)
    _assert_route(label + " (uncapped)", c, rt0, (c.napad + c.waves - 1) // c.waves, 1)
    assert rows >= 3
    for k in range(rs.ROWS_M):
        _compare("%s[%d] rows=%d" % (label, k, rows), c, fam, rs.reference_with_eps(("default", name), fam, k), e[k], part[k], bia[k])
    assert np.array_equal(bia, bia0) and np.array_equal(part, part0) and np.array_equal(e, e0), "%s: not the uncapped run bit for bit" % label


@pytest.mark.parametrize("fam", rs.FAMILIES)
def test_launchers_own_grid_walks_three_rows(fam, tmp):
    """300 fragments (six distinct inputs tiled): the launcher itself picks gx = 7, three rows per wave."""
    c = rs.BY_KEY[rs.TILED]
    e, part, bia, rt = _get(_route("default", tmp), "tiled/%s" % fam)
    _assert_route("tiled/%s" % fam, c, rt, rs.TILED_GX, rs.TILED_ROWS)
    assert e.shape[0] == rs.TILED_M
    for k in range(rs.TILED_DISTINCT):
        _compare("tiled/%s[%d] rows=%d" % (fam, k, rs.TILED_ROWS), c, fam, rs.reference_with_eps(rs.TILED, fam, k), e[k], part[k], bia[k])
    idx = np.arange(rs.TILED_M) % rs.TILED_DISTINCT
    assert np.array_equal(bia, bia[idx]) and np.array_equal(part, part[idx]) and np.array_equal(e, e[idx]), "equal fragments, different results"


@pytest.mark.parametrize("fam", rs.FAMILIES)
def test_ragged_batch(fam, tmp):
    """nmo = n, n - 3, nocc (no virtuals), a fragment that does not run, nocc - 1; C and eps beyond nmo are NaN."""
    c = rs.BY_KEY[rs.RAGGED]
    got = _route("default", tmp)
    e, part, bia, rt = _get(got, "ragged/%s" % fam)
    _assert_route("ragged/%s" % fam, c, rt)
    for f, (nmo, runs) in enumerate(zip(rs.RAGGED_NMO, rs.RAGGED_RUNS)):
        label = "ragged/%s[%d] nmo=%d runs=%d" % (fam, f, nmo, runs)
        e1, part1, bia1, _ = _get(got, "ragged/%s/%d" % (fam, f))
        if runs and nmo > c.nocc:
            _compare(label, c, fam, rs.reference_with_eps(rs.RAGGED, fam, f, nmo), e[f], part[f], bia[f], nmo)
        elif runs and nmo == c.nocc:          # no virtual orbital: the transform writes zeros, every pair sums nothing
            assert not e[f].any() and not part[f].any() and not bia[f].any(), label
        else:                                  # the kernels leave the fragment alone: the poison stays, the energies are zeros
            assert not e[f].any() and np.isnan(part[f]).all() and np.isnan(bia[f]).all(), label
        # the neighbours change nothing: bit for bit the fragment on its own
        assert np.array_equal(e[f], e1[0]) and np.array_equal(part[f], part1[0], equal_nan=True) and np.array_equal(bia[f], bia1[0], equal_nan=True), label


@pytest.mark.parametrize("fam", rs.FAMILIES)
def test_stale_pool(fam, tmp):
    """(13, 5, 126, 1) right after (48, 10, 252, 2) in one process equals the first call of a fresh process bit for bit."""
    got = _route("default", tmp)
    e, part, bia, rt = _get(got, "stale/%s" % fam)
    e0, part0, bia0, rt0 = _get(got, "fresh/%s" % fam)
    assert rt == rt0
    assert np.array_equal(bia, bia0) and np.array_equal(part, part0) and np.array_equal(e, e0)
    assert not np.isnan(bia).any() and not np.isnan(part).any() and not np.isnan(e).any()
    _compare("stale/%s" % fam, rs.BY_KEY[rs.STALE[1]], fam, rs.reference_with_eps(rs.STALE[1], fam), e[0], part[0], bia[0])


def test_refusals():
    """Null pointers and sizes out of range: each returns its error and writes nothing."""
    import ctypes as C
    lib, ctx = capi.load_library(), capi.get_context()
    c = rs.BY_KEY[("default", "n2-o1-a5-f0")]
    B, Cm, eps = rs.inputs(c, "real")
    nmo, runs = np.array([2], dtype=np.int32), np.array([1], dtype=np.int32)
    e, part, route = np.full((1, 2), np.nan), np.full((1, 1, 2), np.nan), np.full(16, -1, dtype=np.int32)
    ip = lambda a: a.ctypes.data_as(capi.c_int32_p)
    args = [ctx, 1, 2, 1, 5, 0, 0, capi.dptr(B), capi.dptr(Cm), capi.dptr(eps), ip(nmo), ip(runs), capi.dptr(e), capi.dptr(part), None, ip(route)]
    for k in (7, 8, 9, 10, 11, 12, 13, 15):
        bad = list(args); bad[k] = None
        assert lib.mqc_hip_rimp2_stage(*bad) == capi.ERR_VALIDATION, k
    for k, v in ((1, 0), (1, -1), (2, 0), (2, 141), (3, 0), (3, 3), (4, 0), (5, 1), (5, -1), (6, -1)):
        bad = list(args); bad[k] = v
        assert lib.mqc_hip_rimp2_stage(*bad) == capi.ERR_VALIDATION, (k, v)
    for v in (-1, 3):
        wrong = np.array([v], dtype=np.int32)
        bad = list(args); bad[10] = ip(wrong)
        assert lib.mqc_hip_rimp2_stage(*bad) == capi.ERR_VALIDATION, v
    assert np.isnan(e).all() and np.isnan(part).all()
    # no virtual orbital: zeros, nothing launched
    e2, part2, bia2, rt = stages.rimp2_stage(B, Cm, eps, 2, 0)
    assert rt["nvpad"] == 0 and not e2.any() and not part2.any() and bia2.size == 0
