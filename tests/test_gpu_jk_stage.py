"""Stage tests of the in-core J/K stream (kern_fock.hip): mqc_hip_jk_incore_batch runs launch_jk_incore once on given
tensors and densities, and J and K are compared element by element with the plain contraction of the same pair matrix
(tests/jk_stage_cases.py), at one case per instance and edge of the dispatch, on every route the environment switches
select: default, tri0 (MQC_HIP_ERI_TRI=0), wg1 / wg5 / wg1000 (MQC_HIP_JK_TRI_WG: one workgroup per fragment -- the path
of batches from 768 fragments on, plain stores and nothing zeroed --, a stride that does not divide the block count, the
clamp to one block per wave), rowcoop0 (MQC_HIP_JK_ROWCOOP=0).

Why: every batch route was tested through converged SCF energies only, and the energy is stationary in the density.
The kernel that runs is picked by size, batch and switches; every case names the instance and the grid it must land
on and the test asserts what the launcher reports.

Exact cases (the main test): symmetric integer tensors in [-7, 7] and densities in [-3, 3]; every partial sum is a
multiple of 0.5 below 2^20, so J and K are the same in any order of summation, and the tolerance is ZERO.
Float cases (one per instance): normal deviates over twelve decades against np.longdouble; the bound is derived, not
measured -- m eps (|M| contracted with |D|) elementwise, m = npair for J and n^2 for K.
Finished fragments (only_active): every element is the poison or zero; the running ones are exact and bitwise the
same whichever other fragments are finished.  Screening (triangle): the stored rows of the flagged pairs are zero, the
result is the plain reference exactly, and the chunks read are those of tests/jk_stage_cases.expected_loaded.

Measured on an MI355X.  Every exact case on every route: zero elements differ.  Float cases -- `dev/bound` is the worst
ratio of an element's deviation to its own derived bound over the case (the bound is 1), `max dev` the largest deviation,
against elements of up to `max |ref|`:

  instance                      route     case          J dev/bound  max dev   max |J|   K dev/bound  max dev   max |K|
  wave<1,lds,4,5,reg>           default   n24-m3        5.0e-03      4.9e-04   3.2e+12   6.3e-03      7.3e-04   1.5e+12
  wave<1,lds,4,10,reg>          default   n25-m3        6.0e-03      9.8e-04   5.2e+12   3.6e-03      7.3e-04   4.9e+12
  wave<1,lds,4,19,reg>          default   n36-m3        3.4e-03      2.4e-03   8.5e+12   2.4e-03      1.5e-03   5.9e+12
  wave<1,lds,4,0,reg>           default   n49-m3        1.8e-03      2.0e-03   1.2e+13   1.6e-03      4.4e-03   6.1e+12
  wave<2,lds,4,0,mem>           default   n65-m3        1.0e-03      3.9e-03   1.2e+13   8.3e-04      4.9e-03   8.8e+12
  rowcoop<2,8>                  default   n67-m3        7.3e-04      3.9e-03   1.6e+13   6.1e-04      3.9e-03   7.4e+12
  wave<2,global,2,0,mem>        default   n90-m3        5.5e-04      5.9e-03   1.1e+13   3.5e-04      5.9e-03   8.0e+12
  wave<1,lds,12,10,reg>         default   n25-m64       7.8e-03      2.0e-03   9.1e+12   6.0e-03      1.8e-03   9.1e+12
  wave<1,lds,12,19,reg>         default   n41-m64       3.1e-03      3.9e-03   1.2e+13   2.1e-03      3.9e-03   9.4e+12
  tri<12,10>                    default   n40-m64       4.2e-03      4.9e-03   1.5e+13   2.2e-03      2.9e-03   8.3e+12
  wave<1,lds,12,19,reg,full8>   default   n40-m64-uhf   2.9e-03      2.9e-03   1.5e+13   2.4e-03      3.9e-03   8.3e+12
  wave<2,global,4,0,mem>        rowcoop0  n67-m3        1.2e-03      3.9e-03   1.6e+13   7.9e-04      4.9e-03   7.4e+12

  No kernel needs more than a hundredth of its bound.  The tie (the engine's own tensor of a water dimer through the
  triangle): 5.7e-14 against 1e-10.

Sharpness, three wrong-answer edits of kern_fock.hip tried one at a time on a scratch build (none is in the tree):
  * row_exchange_tri without its partial last block: 53 tests fail -- every triangle case (n = 40 and 48; default, wg1,
    wg5, wg1000; plain, all screening patterns but `all`, the batch of 65, the float case, both only_active cases and the
    tie); K differs in 97 047 of 102 400 elements at n = 40 (by up to 576) and in 141 037 of 147 456 at n = 48 (by up to
    717), J in none.
  * the one-workgroup flush without the transpose (Kg = Kl): 13 tests fail -- exactly the wg1 cases (n = 40 and 48,
    plain and five screening patterns each, and the only_active case); K differs in 102 234 elements at n = 40 (by up to
    1 570) and in 147 259 at n = 48 (by up to 1 620).  No other route notices: this path had no test before.
  * c1 = (sen + 126) >> 7 in load_block: NOTHING fails, and nothing can.  The two forms differ only for a block whose
    padded end is 1 modulo 128, and neither triangle an admissible shape reaches (n = 40: blocks of 874; n = 48: 1240)
    has such a block (n = 56 would have eleven, and is refused: 1672 doubles exceed ten chunks).  The edit changes no
    load, no counter and no result at any reachable size; tests/test_jk_stage_cases.py asserts that arithmetic, so that
    a layout that does get such a block is noticed.

Unreachable instances: see tests/jk_stage_cases.py."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import jk_stage_cases as jc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return str(tmp_path_factory.mktemp("jk_stage"))


@functools.lru_cache(maxsize=None)
def _reference(key):
    """J and K of the inputs of a case (and the bounds of a float case): computed once per set of inputs, shared by every
    route and test that runs them, never modified."""
    kind, n, nfrag, pattern = key
    out = jc.case_reference(jc.Case("default", n, nfrag, kind=kind, pattern=pattern))
    for a in out:
        if a is not None:
            a.setflags(write=False)
    return out


_ROUTE_OUTCOME = {}       # route -> results of its child, or the text of its failure: a child is started ONCE
_ABNORMAL = []            # a child killed by a signal or by its time limit: no other route's child is started after it


def _route(route, tmp):
    """One child process per route (the switches are read once per process): every case of the route, results from a
    file.  The outcome is kept, a failure included: after a child that failed, faulted or ran into its time limit every
    other test of the route fails from the stored text and nothing is started on the GPU again; after a child that was
    killed (a signal, the time limit) no other route starts either."""
    if route not in _ROUTE_OUTCOME and _ABNORMAL:
        _ROUTE_OUTCOME[route] = "route %s: not started after %s" % (route, _ABNORMAL[0])
    if route not in _ROUTE_OUTCOME:
        out = os.path.join(tmp, "jk_stage_%s.npz" % route)
        env = dict(os.environ, **jc.ROUTES[route])
        want = [c.name for c in jc.route_cases(route)]
        try:
            p = subprocess.run([sys.executable, "-m", "tests.jk_stage_child", route, out], cwd=ROOT, env=env, capture_output=True,
                               text=True, timeout=600)
            if p.returncode != 0:
                _ROUTE_OUTCOME[route] = "route %s: child failed (%d)\n%s\n%s" % (route, p.returncode, p.stdout[-2000:], p.stderr[-4000:])
                if p.returncode < 0 or p.returncode > 128:
                    _ABNORMAL.append("route %s ended with status %d" % (route, p.returncode))
            else:
                info = json.loads(p.stdout.strip().splitlines()[-1])
                _ROUTE_OUTCOME[route] = dict(np.load(out)) if info["cases"] == want else "route %s: child ran %s" % (route, info["cases"])
        except Exception as exc:       # the time limit, unreadable output: kept like any other failure
            _ROUTE_OUTCOME[route] = "route %s: %r" % (route, exc)
            if isinstance(exc, subprocess.TimeoutExpired):
                _ABNORMAL.append("route %s ran into its time limit" % route)
    got = _ROUTE_OUTCOME[route]
    if isinstance(got, str):
        pytest.fail(got)
    return got


def _check_route_report(c, got, tag):
    inst, gx = str(got["I:" + tag]), int(got["G:" + tag])
    assert (inst, gx) == c.expect, "%s/%s: the dispatch reports %s with grid x %d, the case expects %s with %d" % ((c.route, tag, inst, gx) + c.expect)
    assert tuple(int(v) for v in got["Y:" + tag]) == tuple(int(v) for v in jc.tensor_layout(c.n, c.nfrag, c.uhf, jc.ROUTES[c.route]))
    return inst, gx


def _worst(X, X0):
    bad = X != X0          # NaN (an element nothing wrote) differs from everything
    where = tuple(int(v) for v in np.argwhere(bad)[0]) if bad.any() else None
    with np.errstate(invalid="ignore"):
        return int(bad.sum()), float(np.nanmax(np.abs(X - X0))) if not np.isnan(X).all() else float("nan"), where


_PLAIN = [(c.route, c.name) for c in jc.CASES if not c.done]


@pytest.mark.parametrize("route,name", _PLAIN, ids=["%s-%s" % p for p in _PLAIN])
def test_jk_matches_reference(route, name, tmp):
    c = jc.BY_NAME[(route, name)]
    got = _route(route, tmp)
    inst, gx = _check_route_report(c, got, name)
    J, K, loaded = got["J:" + name], got["K:" + name], got["L:" + name]
    J0, K0, bj, bk = _reference(c.key)
    assert J.shape == J0.shape and K.shape == K0.shape
    label = "%s/%s %s x%d" % (route, name, inst, gx)
    if c.kind == "exact":
        nj, dj, wj = _worst(J, J0)
        nk, dk, wk = _worst(K, K0)
        print("JKSTAGE %s exact: J %d elements differ (max %.3g), K %d elements differ (max %.3g), NaN %d" % (
            label, nj, dj, nk, dk, int(np.isnan(J).sum() + np.isnan(K).sum())))
        assert nj == 0, "%s: %d elements of J differ, by up to %.3g, first at %s" % (label, nj, dj, wj)
        assert nk == 0, "%s: %d elements of K differ, by up to %.3g, first at %s" % (label, nk, dk, wk)
    else:
        nan = int(np.isnan(J).sum() + np.isnan(K).sum())
        with np.errstate(invalid="ignore", divide="ignore"):
            ej, ek = np.abs(J - J0), np.abs(K - K0)
            rj, rk = float(np.nanmax(ej / bj)), float(np.nanmax(ek / bk))
        print("JKSTAGE %s float: J dev/bound worst %.3e (max dev %.3e, max |J| %.3e) | K dev/bound worst %.3e (max dev %.3e, max |K| %.3e)" % (
            label, rj, float(np.nanmax(ej)), float(np.max(np.abs(J0))), rk, float(np.nanmax(ek)), float(np.max(np.abs(K0)))))
        assert nan == 0, "%s: %d NaN (elements nothing wrote)" % (label, nan)
        assert np.all(bj > 0) and np.all(bk > 0)
        assert np.all(ej <= bj), "%s: J beyond its bound by a factor %.3g at %s" % (label, rj, np.unravel_index(np.argmax(ej / bj), ej.shape))
        assert np.all(ek <= bk), "%s: K beyond its bound by a factor %.3g at %s" % (label, rk, np.unravel_index(np.argmax(ek / bk), ek.shape))
    # the read counters: the triangle counts the chunks it asked for, every other plan has no counter
    if inst.startswith("tri"):
        want = [jc.expected_loaded(c.n, jc.row_flags(c.n, jc.shell_flags(c.n, c.pattern, f)) if c.pattern else None) for f in range(c.nfrag)]
        assert loaded.tolist() == want, "%s: chunks read %s, expected %s" % (label, loaded.tolist()[:8], want[:8])
        full = jc.expected_loaded(c.n)
        if c.pattern == "cross":
            assert all(v < full for v in loaded)
        if c.pattern == "all":
            assert not loaded.any() and not J.any() and not K.any()
    else:
        assert (loaded == -1).all()


_DONE = [(c.route, c.name) for c in jc.CASES if c.done]


@pytest.mark.parametrize("route,name", _DONE, ids=["%s-%s" % p for p in _DONE])
def test_finished_fragments_are_left_alone(route, name, tmp):
    """only_active with a mix of finished and running fragments: the running ones are exact; every element of a finished
    one is the poison (NaN) or zero -- the launchers zero K, and for the triangle with several workgroups J too, for the
    whole batch; the running fragments come out bitwise the same whichever others are finished."""
    c = jc.BY_NAME[(route, name)]
    got = _route(route, tmp)
    J0, K0, _, _ = _reference(c.key)
    runs = []
    for k, done in enumerate(c.done):
        tag = "%s:%d" % (name, k)
        inst, gx = _check_route_report(c, got, tag)
        J, K = got["J:" + tag], got["K:" + tag]
        live = np.array([f not in done for f in range(c.nfrag)])
        assert 0 < live.sum() < c.nfrag
        assert np.array_equal(J[live], J0[live]), "%s/%s: J of a running fragment is off" % (route, tag)
        assert np.array_equal(K[live], K0[live]), "%s/%s: K of a running fragment is off" % (route, tag)
        for X in (J[~live], K[~live]):
            assert np.all(np.isnan(X) | (X == 0.0)), "%s/%s: a finished fragment was written" % (route, tag)
        # what the launchers zero for everyone: K always; J only by the triangle's several workgroups
        assert not K[~live].any() or (inst.startswith("tri") and gx == 1 and np.isnan(K[~live]).all())
        assert np.isnan(J[~live]).all() or (inst.startswith("tri") and gx > 1 and not J[~live].any())
        runs.append((live, J, K))
    both = runs[0][0] & runs[1][0]
    assert both.sum() > 0
    assert runs[0][1][both].tobytes() == runs[1][1][both].tobytes() and runs[0][2][both].tobytes() == runs[1][2][both].tobytes()


def test_engine_tensor_through_the_batch_entry(tmp):
    """The tie to the single-fragment entries: mqc_hip_eri_packed of a water dimer (n = 48) repeated as 64 fragments with
    64 different exact densities through the batch entry (the triangle), against the numpy contraction of the same
    tensor at 1e-10 -- the bound and, for the first two fragments, the reference (_jk_from_packed, a full four-index
    tensor each) of test_jk_incore_larger_fragments_all_kernel_variants; every fragment against jk_reference."""
    from tests.test_gpu_parity import _jk_from_packed
    got = _route("default", tmp)
    M, J, K = got["M:tie"], got["J:tie"], got["K:tie"]
    assert (str(got["I:tie"]), int(got["G:tie"])) == jc.instance_of(jc.TIE_N, jc.TIE_NFRAG)
    assert float(got["S:tie"]) == 0.0           # the square is stored with both mirror elements alike
    D = jc.tie_densities(jc.TIE_N, jc.TIE_NFRAG)
    worst = 0.0
    for f in range(jc.TIE_NFRAG):
        Jr, Kr = jc.jk_reference(M, D[f])
        if f < 2:
            Jp, Kp = _jk_from_packed(M, D[f])
            assert np.max(np.abs(Jp - Jr)) < 1e-11 and np.max(np.abs(Kp - Kr)) < 1e-11
            assert np.max(np.abs(J[f] - Jp)) < 1e-10 and np.max(np.abs(K[f] - Kp)) < 1e-10
        worst = max(worst, float(np.max(np.abs(J[f] - Jr))), float(np.max(np.abs(K[f] - Kr))))
    print("JKSTAGE tie: worst deviation %.3e" % worst)
    assert worst < 1e-10
    assert np.max(np.abs(J[0] - J[1])) > 1e-3


def test_refusals():
    """n = 117 and everything else the entry validates: each returns MQC_HIP_ERR_VALIDATION and writes nothing."""
    import ctypes as C
    from metalquicha_amd import capi
    from tests import stages
    lib, ctx = capi.load_library(), capi.get_context()
    n, m = 8, 2
    tri, pb, stride = stages.jk_tensor_layout(n, m)
    assert (tri, pb, stride) == jc.tensor_layout(n, m)
    T, D = jc.case_tensor(jc.Case("default", n, m), (tri, pb, stride))
    J, K = np.full_like(D, np.nan), np.full_like(D, np.nan)
    loaded = np.full(m, -2, dtype=np.int32)
    route, gx = C.create_string_buffer(48), C.c_int32(-5)
    ip = lambda a: a.ctypes.data_as(capi.c_int32_p)
    sl = np.array([0, 1, 1, 0], dtype=np.int32)          # 1 + 3 + 3 + 1 = 8 functions
    Q = np.ones((m, 4, 4))
    args = [ctx, m, n, 0, capi.dptr(T), stride, capi.dptr(D), None, 0, None, None, C.c_double(0.0), capi.dptr(J), capi.dptr(K), ip(loaded),
            route, len(route), C.byref(gx)]
    for k in (0, 4, 6, 12, 13, 14, 15, 17):
        bad = list(args); bad[k] = None
        assert lib.mqc_hip_jk_incore_batch(*bad) == capi.ERR_VALIDATION, k
    scr = list(args); scr[8], scr[9], scr[10], scr[11] = 4, ip(sl), capi.dptr(Q), C.c_double(1e-6)
    for k, v in ((1, 0), (1, -3), (2, 0), (2, -1), (2, 117), (5, stride - 1), (5, stride + 1), (5, 0), (16, 0)):
        bad = list(args); bad[k] = v
        assert lib.mqc_hip_jk_incore_batch(*bad) == capi.ERR_VALIDATION, (k, v)
    long_l, neg_l = np.array([0, 1, 1, 1], dtype=np.int32), np.array([0, 1, -1, 0], dtype=np.int32)
    for k, v in ((9, None), (10, None), (8, 3), (8, -1), (9, ip(long_l)), (9, ip(neg_l)), (11, C.c_double(float("nan")))):
        bad = list(scr); bad[k] = v
        assert lib.mqc_hip_jk_incore_batch(*bad) == capi.ERR_VALIDATION, (k, v)
    # screening is the triangular kernel's: n_ao <= 64
    n2 = 65
    T2, D2 = np.zeros((1, jc.npair(n2) ** 2)), np.zeros((1, n2, n2))
    J2, K2 = np.full_like(D2, np.nan), np.full_like(D2, np.nan)
    one_l, one_q = np.array([32], dtype=np.int32), np.ones((1, 1, 1))
    big = [ctx, 1, n2, 0, capi.dptr(T2), T2.shape[1], capi.dptr(D2), None, 1, ip(one_l), capi.dptr(one_q), C.c_double(1e-6), capi.dptr(J2),
           capi.dptr(K2), ip(loaded), route, len(route), C.byref(gx)]
    assert lib.mqc_hip_jk_incore_batch(*big) == capi.ERR_VALIDATION
    assert np.isnan(J).all() and np.isnan(K).all() and np.isnan(J2).all() and (loaded == -2).all() and gx.value == -5
    # the layout query
    t, b, s = C.c_int32(), C.c_int64(), C.c_int64()
    assert lib.mqc_hip_jk_tensor_layout(0, 1, 0, C.byref(t), C.byref(b), C.byref(s)) == capi.ERR_VALIDATION
    assert lib.mqc_hip_jk_tensor_layout(8, 0, 0, C.byref(t), C.byref(b), C.byref(s)) == capi.ERR_VALIDATION
    assert lib.mqc_hip_jk_tensor_layout(8, 1, 0, None, C.byref(b), C.byref(s)) == capi.ERR_VALIDATION
    assert stages.jk_tensor_layout(48, 64) == jc.tensor_layout(48, 64) and stages.jk_tensor_layout(48, 64, True) == jc.tensor_layout(48, 64, True)
    # and the same call, untouched, runs
    assert lib.mqc_hip_jk_incore_batch(*args) == 0 and route.value.decode() == jc.instance_of(n, m)[0]
    J0, K0, _, _ = _reference(("exact", n, m, None))
    assert np.array_equal(J, J0) and np.array_equal(K, K0)
    assert lib.mqc_hip_jk_incore_batch(*scr) == 0            # screening fields on a square plan: set, and not read
    assert np.array_equal(J, J0) and np.array_equal(K, K0)
