"""The cases of the RI-MP2 stage tests (tests/rimp2_stage_cases.py) checked on the CPU: the numpy reference against
tests/rimp2_reference.pair_energies, the exactness claims of the integer family, and -- through the host-only half of
mqc_hip_rimp2_stage, which runs the launcher's own arithmetic without a device -- that every case lands on the route it
names, that the table reaches every route the launcher has, and that for n <= 140 the launcher neither narrows the
occupied pass nor refuses.  No GPU."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import rimp2_reference, rimp2_stage_cases as rs, stages

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_KEYS = sorted({("default", c.name) for c in rs.CASES if c.route == "default"} | {(c.route, c.name) for c in rs.CASES})


def test_reference_matches_pair_energies():
    """The stage reference (packed B, pair by pair) against the reference of the end-to-end tests (unpacked B, one
    einsum over all pairs) on a generic input, frozen orbital and dropped modes included."""
    c = rs.BY_KEY[("default", "n13-o5-a126-f1")]
    Bf, C, eps = rs.inputs_one(c, "real")
    for nmo in (c.n, c.n - 2):
        Bia, part, e, _ = rs.reference(Bf, C, eps, c.nocc, c.nfz, nmo)
        Bu = np.ascontiguousarray(np.moveaxis(rs.unpack(Bf), 0, -1))
        e_os, e_ss = rimp2_reference.pair_energies(Bu, C[:, :nmo], eps[:nmo], c.nocc, c.nfz)
        assert Bia.shape == (c.no, c.naux, nmo - c.nocc) and part.shape == (c.no * (c.no + 1) // 2, 2)
        assert abs(e[0] - e_os) <= 1e-12 * abs(e_os) and abs(e[1] - e_ss) <= 1e-12 * abs(e_ss)
    assert np.array_equal(rs.unpack(Bf), np.swapaxes(rs.unpack(Bf), 1, 2))


@pytest.mark.parametrize("key", _KEYS, ids=["%s-%s" % k for k in _KEYS])
def test_integer_family_is_exact_and_not_zero(key):
    c = rs.BY_KEY[key]
    r = rs.reference_with_eps(key, "int")
    Bia = r["Bia"]
    print("RIMP2CASE %s/%s int: max|Bia| = %g, max|V| = %g, rel eps_part = %.1e, rel eps_e = %.1e" % (
        key[0], key[1], np.max(np.abs(Bia)), r["vmax"], r["eps_part"] / np.max(np.abs(r["part"])), r["eps_e"] / np.max(np.abs(r["e"]))))
    assert Bia.any(), "the reference Bia of %s is identically zero: pick another salt" % c.name
    assert r["exact"], "float64, longdouble and the reversed order differ on Bia"
    # whatever the draw and the order of the sums: |Bia| <= 2 n^2 and |V| <= n_aux (2 n^2)^2, every partial sum included,
    # and that is below 2^53 for every case (the draws themselves stay under 1e3 and 1e6)
    top = 2.0 * c.n ** 2
    assert np.array_equal(Bia, np.rint(Bia)) and np.max(np.abs(Bia)) <= top
    assert r["vmax"] == np.rint(r["vmax"]) and r["vmax"] <= c.naux * top ** 2 < 2.0 ** 53
    Bf, C, eps = rs.inputs_one(c, "int")
    assert set(np.unique(Bf)) <= {-2.0, -1.0, 0.0, 1.0, 2.0} and set(np.unique(C)) <= {-1.0, 0.0, 1.0}
    assert np.array_equal(eps * 16, np.rint(eps * 16)) and eps[c.nocc - 1] == -0.5 and eps[c.nocc] == 0.25
    if c.no == 1:
        assert r["part"][0, 1] == 0.0 and r["e"][1] == 0.0


def test_real_family_has_its_gap():
    for c in rs.CASES:
        Bf, C, eps = rs.inputs_one(c, "real")
        assert eps[c.nocc] - eps[c.nocc - 1] >= 0.3 and np.all(np.diff(eps[:c.nocc]) >= 0) and np.all(np.diff(eps[c.nocc:]) >= 0)
        assert np.max(np.abs(C.T @ C - np.eye(c.n))) < 1e-13


_CHILD = """
import json, sys
from tests import stages
print(json.dumps([stages.rimp2_route(*q) for q in json.loads(sys.stdin.read())]))
"""
_ROUTED = {}


def _routes(route, queries):
    """The launcher's routes for (n, nocc, naux, nfz, m, cap) queries through the host-only half of the entry.  The
    switch MQC_HIP_MP2_C_LDS is a function-static read once per process: each route's queries run in a child with the
    route's environment, whatever this process was started with."""
    missing = [q for q in queries if (route, q) not in _ROUTED]
    if missing:
        env = {k: v for k, v in os.environ.items() if k != "MQC_HIP_MP2_C_LDS"}
        env.update(rs.ROUTES[route])
        p = subprocess.run([sys.executable, "-c", _CHILD], input=json.dumps(missing), cwd=ROOT, env=env, capture_output=True, text=True,
                           timeout=120)
        assert p.returncode == 0, p.stderr[-2000:]
        for q, r in zip(missing, json.loads(p.stdout.strip().splitlines()[-1])):
            _ROUTED[(route, q)] = r
    return [_ROUTED[(route, q)] for q in queries]


def _route_of(c, m=1, cap=0):
    return _routes(c.route, [(c.n, c.nocc, c.naux, c.nfz, m, cap)])[0]


def _check(c, got):
    want = c.expected_route()
    assert {k: got[k] for k in want} == want, "%s/%s: the launcher reports %s" % (c.route, c.name, got)


@pytest.mark.parametrize("route", list(rs.ROUTES))
def test_cases_land_on_their_routes(route):
    cs = rs.route_cases(route)
    for c, got in zip(cs, _routes(route, [(c.n, c.nocc, c.naux, c.nfz, 1, 0) for c in cs])):
        _check(c, got)
        assert got["gx"] == (c.napad + c.waves - 1) // c.waves and got["rows"] == 1       # one fragment: a row per wave
        assert got["lds"] <= rs.LDS_MAX


def test_case_table_reaches_every_route():
    cs = rs.CASES
    assert {c.instance for c in cs if c.route == "default"} == {"prefetch", "no-prefetch", "l2"}
    assert {c.waves for c in cs if c.clds} == {8, 4, 2}                  # C in LDS: the launcher halves from eight to two
    assert {c.waves for c in cs if not c.clds} == {4, 2, 1}              # C from L2: four, two, one
    assert {c.passes for c in cs} == {1, 2, 3}
    assert {c.oc for c in cs if c.clds} == {16, 32, 48, 64} and {c.oc for c in cs if not c.clds} == {16, 32, 48, 64}
    assert {c.naux % 4 for c in cs} == {0, 1, 2, 3}
    assert {1, 15, 16, 17} <= {c.n - c.nocc for c in cs}
    assert any(c.n % 16 and c.n % 4 for c in cs) and {48, 64, 80} <= {c.n for c in cs}
    assert any(c.no == 1 for c in cs) and any(c.nfz > 0 for c in cs) and any((c.no * (c.no + 1) // 2) % 4 for c in cs)
    # a last pass over a single orbital
    assert any(c.passes > 1 and c.no % c.oc == 1 for c in cs)


def test_capped_grids_walk_several_rows():
    """workgroups_per_fragment may only lower gx; at 1 and 2 every instance walks at least three rows per wave, padding
    rows included, and the 300-fragment batch gets there by the launcher's own choice."""
    seen = set()
    for key in rs.ROWS_SHAPES:
        c = rs.BY_KEY[key]
        free = _route_of(c, rs.ROWS_M)
        assert free["rows"] == 1
        for cap in rs.ROWS_CAPS:
            got = _route_of(c, rs.ROWS_M, cap)
            _check(c, got)
            assert got["gx"] == cap and got["rows"] == -(-c.napad // (cap * c.waves)) >= 3
            assert (got["rows"] - 1) * cap * c.waves < c.napad         # the last row of the walk exists
        assert _route_of(c, rs.ROWS_M, 10 ** 6) == free                 # a cap above the launcher's choice changes nothing
        seen.add(c.instance)
    assert seen == {"prefetch", "no-prefetch", "l2"}
    c = rs.BY_KEY[rs.TILED]
    got = _route_of(c, rs.TILED_M)
    _check(c, got)
    assert (got["gx"], got["rows"]) == (rs.TILED_GX, rs.TILED_ROWS)
    assert rs.TILED_M * c.naux * rs.npair_of(c.n) * 8 < 28e6
    # production: 2080 waters' worth of fragments, one workgroup per fragment, sixteen rows per wave
    assert _route_of(c, 4096)["gx"] == 1 and _route_of(c, 4096)["rows"] == 16


def test_no_shape_narrows_the_pass_or_is_refused():
    """For every (n, nocc) with n <= 140 -- no frozen orbital, and the most that can be frozen -- the launcher neither
    narrows the occupied pass (oc -= 16) nor refuses: one wave with a 64-orbital pass fits at n = 140."""
    worst = 0
    for n in range(1, 141):
        for nocc in range(1, n + 1):
            for nfz in {0, nocc - 1}:
                r = stages.rimp2_route(n, nocc, 18, nfz)
                assert r["narrowed"] == 0 and r["lds"] <= rs.LDS_MAX, (n, nocc, nfz, r)
                if nocc < n:
                    assert r["waves"] in (1, 2, 4, 8) and r["oc"] in (16, 32, 48, 64) and r["passes"] * r["oc"] >= nocc - nfz
                    if not r["clds"]:
                        worst = max(worst, r["lds"])
    assert worst == 153840 or os.environ.get("MQC_HIP_MP2_C_LDS", "1")[0] == "0"
    # the same walk with C never in LDS (every shape on the L2 kernel)
    qs = [(n, nocc, 18, 0, 1, 0) for n in range(1, 141) for nocc in range(1, n)]
    rr = _routes("no-clds", qs)
    assert all(r["narrowed"] == 0 and r["clds"] == 0 and r["lds"] <= rs.LDS_MAX for r in rr) and max(r["lds"] for r in rr) == 153840


def test_host_only_refusals():
    from metalquicha_amd import capi
    for bad in ((0, 1, 5, 0), (141, 1, 5, 0), (5, 0, 5, 0), (5, 6, 5, 0), (5, 2, 0, 0), (5, 2, 5, 2), (5, 2, 5, -1)):
        with pytest.raises(capi.HipBackendError) as ei:
            stages.rimp2_route(*bad)
        assert ei.value.code == capi.ERR_VALIDATION, bad
    with pytest.raises(capi.HipBackendError):
        stages.rimp2_route(5, 2, 5, 0, 0)
    with pytest.raises(capi.HipBackendError):
        stages.rimp2_route(5, 2, 5, 0, 1, -1)
    assert stages.rimp2_route(5, 5, 5, 0)["nvpad"] == 0
