"""What the broadcast exchange of jk_tri_kernel (kern_fock.hip) can get wrong: density rows in registers, D[l] taken as
lane l % 16 of register l / 16 by the FMA itself, the l loop unrolled in groups of eight with its LDS reads kept in
flight.  The cases are stated in tests/jk_broadcast_cases.py; n = 40 and 48 are the sizes the triangle takes, 64 fragments
the smallest batch it takes, `wg1` (one workgroup per fragment, the benchmark's path) and `default` the routes.  Exact
cases: integer inputs, zero tolerance.  The float case: np.longdouble reference, the derived bound of jk_bounds.

One child process per route (the switches are read once per process), started once; every test of a route reads its
results, and after a child that failed nothing is started on the GPU again.

Measured on an MI355X: every exact case on both routes, zero elements differ; the float case well inside its bound.

Sharpness, three wrong-answer edits of kern_fock.hip tried one at a time on a scratch build (none is in the tree); each
fails all 13 tests of this file (every exact case has rows that reach the edited step, and the float case is off by
10^12 to 10^13 bounds):
  * acc_i takes lane (l + 1) % 16 instead of l % 16: unit cases, K differs in 1 to 10 elements per fragment (the slice
    of the neighbouring function); partial and outlive cases in 1480 to 2301 elements per fragment.
  * acc_j takes the density register (l / 16 + 1) % 3: unit cases, K differs in 46 to 54 elements per fragment; partial
    case first noticed at the rows (6, .): 46 elements of K.
  * density rows not zeroed beyond l = i: unit cases, ONE element of K per fragment (the re-read element (k, i) times the
    density entry that should not count); rows (6, .): 43 elements of K."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import jk_broadcast_cases as bc, jk_stage_cases as jc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return str(tmp_path_factory.mktemp("jk_broadcast"))


@functools.lru_cache(maxsize=None)
def _reference(kind, n):
    """Computed once per set of inputs, shared by both routes, never modified."""
    out = bc.case_reference(kind, n)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _float_reference():
    out = jc.case_reference(bc.FLOAT_CASE)
    for a in out:
        a.setflags(write=False)
    return out


_OUTCOME = {}
_ABNORMAL = []


def _route(route, tmp):
    if route not in _OUTCOME and _ABNORMAL:
        _OUTCOME[route] = "route %s: not started after %s" % (route, _ABNORMAL[0])
    if route not in _OUTCOME:
        out = os.path.join(tmp, "jk_broadcast_%s.npz" % route)
        env = dict(os.environ, **jc.ROUTES[route])
        want = [t for t, _, _ in bc.route_cases(route)] + ([bc.FLOAT_CASE.name] if route == bc.FLOAT_CASE.route else [])
        try:
            p = subprocess.run([sys.executable, "-m", "tests.jk_broadcast_child", route, out], cwd=ROOT, env=env, capture_output=True,
                               text=True, timeout=300)
            if p.returncode != 0:
                _OUTCOME[route] = "route %s: child failed (%d)\n%s\n%s" % (route, p.returncode, p.stdout[-2000:], p.stderr[-4000:])
                if p.returncode < 0 or p.returncode > 128:
                    _ABNORMAL.append("route %s ended with status %d" % (route, p.returncode))
            else:
                info = json.loads(p.stdout.strip().splitlines()[-1])
                _OUTCOME[route] = dict(np.load(out)) if info["cases"] == want else "route %s: child ran %s" % (route, info["cases"])
        except Exception as exc:
            _OUTCOME[route] = "route %s: %r" % (route, exc)
            if isinstance(exc, subprocess.TimeoutExpired):
                _ABNORMAL.append("route %s ran into its time limit" % route)
    got = _OUTCOME[route]
    if isinstance(got, str):
        pytest.fail(got)
    return got


def _exact(route, kind, n, tmp):
    """J, K, loaded of an exact case, the instance checked; (J0, K0) its reference."""
    got = _route(route, tmp)
    tag = "%s-n%d" % (kind, n)
    assert (str(got["I:" + tag]), int(got["G:" + tag])) == jc.instance_of(n, bc.NFRAG, False, jc.ROUTES[route])
    assert str(got["I:" + tag]).startswith("tri")
    return got["J:" + tag], got["K:" + tag], got["L:" + tag], _reference(kind, n)


def _differs(X, X0):
    bad = X != X0              # NaN (an element nothing wrote) differs from everything
    return int(bad.sum()), (tuple(int(v) for v in np.argwhere(bad)[0]) if bad.any() else None)


@pytest.mark.parametrize("n", bc.SIZES)
@pytest.mark.parametrize("route", bc.ROUTES)
def test_broadcast_lane_and_register(route, n, tmp):
    """D = E_ab + E_ba: K and J are single slices of the tensor, one (a, b) per fragment over the edges of the groups of
    eight and of the rows of 16 lanes."""
    J, K, _, (J0, K0) = _exact(route, "unit", n, tmp)
    pairs, _ = bc.unit_pairs(n)
    for f, (a, b) in enumerate(pairs):
        nk, wk = _differs(K[f], K0[f])
        nj, wj = _differs(J[f], J0[f])
        print("JKBCAST %s n%d unit (a, b) = (%d, %d): K %d, J %d elements differ" % (route, n, a, b, nk, nj))
        assert nk == 0, "%s n = %d, D = E(%d,%d) + E(%d,%d): %d elements of K differ, first at %s" % (route, n, a, b, b, a, nk, wk)
        assert nj == 0, "%s n = %d, D = E(%d,%d) + E(%d,%d): %d elements of J differ, first at %s" % (route, n, a, b, b, a, nj, wj)


@pytest.mark.parametrize("n", bc.SIZES)
@pytest.mark.parametrize("route", bc.ROUTES)
def test_partial_last_group(route, n, tmp):
    """Dense density, the pair rows of one i per fragment, i + 1 no multiple of eight: row by row."""
    J, K, _, (J0, K0) = _exact(route, "partial", n, tmp)
    rows = bc.partial_rows(n)
    for i in rows:         # not vacuous: every i has fragments whose reference is not zero (a single row (0, 0) can be)
        assert any(K0[f].any() and J0[f].any() for f in range(bc.NFRAG) if rows[f % len(rows)] == i)
    for f in range(bc.NFRAG):
        i = rows[f % len(rows)]
        nk, wk = _differs(K[f], K0[f])
        nj, wj = _differs(J[f], J0[f])
        print("JKBCAST %s n%d partial i = %d (fragment %d): K %d, J %d elements differ" % (route, n, i, f, nk, nj))
        assert nk == 0, "%s n = %d, rows (%d, .), fragment %d: %d elements of K differ, first at %s" % (route, n, i, f, nk, wk)
        assert nj == 0, "%s n = %d, rows (%d, .), fragment %d: %d elements of J differ, first at %s" % (route, n, i, f, nj, wj)


@pytest.mark.parametrize("n", bc.SIZES)
@pytest.mark.parametrize("route", bc.ROUTES)
def test_one_row_of_a_block_outlives_the_other(route, n, tmp):
    """One row of the first, the middle or the last block taken for zero, the other kept: J, K and the chunks read."""
    J, K, loaded, (J0, K0) = _exact(route, "outlive", n, tmp)
    full = jc.expected_loaded(n)
    for f in range(bc.NFRAG):
        pos, row = bc.SPLIT_KINDS[f % len(bc.SPLIT_KINDS)]
        nk, wk = _differs(K[f], K0[f])
        nj, wj = _differs(J[f], J0[f])
        want = jc.expected_loaded(n, bc.split_row_flags(n, f))
        print("JKBCAST %s n%d outlive %s block, %s row zero (fragment %d): K %d, J %d elements differ, chunks %d (expected %d, unscreened %d)" % (
            route, n, pos, row, f, nk, nj, int(loaded[f]), want, full))
        assert nk == 0, "%s n = %d, %s block without its %s row: %d elements of K differ, first at %s" % (route, n, pos, row, nk, wk)
        assert nj == 0, "%s n = %d, %s block without its %s row: %d elements of J differ, first at %s" % (route, n, pos, row, nj, wj)
        assert int(loaded[f]) == want and want <= full


def test_float_inputs_one_workgroup(tmp):
    """n = 48, 64 fragments on the one-workgroup route, normal deviates over twelve decades against np.longdouble."""
    c = bc.FLOAT_CASE
    got = _route(c.route, tmp)
    assert (str(got["I:" + c.name]), int(got["G:" + c.name])) == c.expect and c.expect == ("tri<12,10>", 1)
    J, K = got["J:" + c.name], got["K:" + c.name]
    J0, K0, bj, bk = _float_reference()
    nan = int(np.isnan(J).sum() + np.isnan(K).sum())
    with np.errstate(invalid="ignore", divide="ignore"):
        ej, ek = np.abs(J - J0), np.abs(K - K0)
        rj, rk = float(np.nanmax(ej / bj)), float(np.nanmax(ek / bk))
    print("JKBCAST %s %s float: J dev/bound worst %.3e (max dev %.3e) | K dev/bound worst %.3e (max dev %.3e)" % (
        c.route, c.name, rj, float(np.nanmax(ej)), rk, float(np.nanmax(ek))))
    assert nan == 0, "%d NaN (elements nothing wrote)" % nan
    assert np.all(bj > 0) and np.all(bk > 0)
    assert np.all(ej <= bj), "J beyond its bound by a factor %.3g" % rj
    assert np.all(ek <= bk), "K beyond its bound by a factor %.3g" % rk
