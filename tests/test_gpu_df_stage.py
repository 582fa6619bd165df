"""Stage tests of density fitting: the J/K stage (mqc_hip_df_jk_batch: launch_df_jk, once, on given tensors) and the build
of the fitted tensor (mqc_hip_df_fit_batch: the integral half and the fit half of launch_df_build) against the CPU
oracle, element by element, at one case per instance and edge of kern_df.hip (tests/df_stage_cases.py) on every route
the environment switches select: default, no-wave (MQC_HIP_DF_WAVE=0), v1 (MQC_HIP_DF_V1=1), chol-v1
(MQC_HIP_DF_CHOL_V1=1, fit cases only).

Why: every other density-fitting test is an SCF energy at 1e-8 to 1e-9 Eh, and the energy is stationary in the density:
one wrong tile of J or K shows at second order only.  The kernel that runs is picked by size and by switches; every case
names the instance it must land on and the test asserts the instance the launcher reports.

Tolerances (df_stage_cases.py).  J and K: MARGIN (50, derivation next to the import there) x eps_ref, never looser than
1e-11 max(1, max |ref|); eps_ref, per case and for J and K apart, is the larger of build_jk_df in float64 against the same
contraction in np.longdouble and against float64 with the auxiliary index reversed, not below one unit in the last
place.  A3 and the metric: 1e-11 against eri3c and eri2c; the metric exactly symmetric.  The fitted B is compared
through G = B^T B against A3^T M^+ A3 (eigenvalues above 1e-10): MARGIN x eps_G, eps_G the float64 difference between the
oracle's eigen fit and a Cholesky fit of the same integrals (flagged case: the eigen fit at two block orders).

`kernel` = worst deviation over the cases of the row, measured on an MI355X; eps_ref and bound are those of the case
with the worst ratio of deviation to bound (`cases`: how many cases of df_stage_cases.JK_CASES land on the row):

  instance       route    cases  eps_ref J  bound J   kernel J   eps_ref K  bound K   kernel K
  wave<1,3>      default  3      2.1e-15    1.1e-13   2.7e-15    1.6e-14    8.0e-13   1.6e-14
  wave<2,9>      default  2      2.9e-15    1.4e-13   3.6e-15    7.0e-16    3.5e-14   8.9e-16
  wave<3,19>     default  6      9.8e-15    4.9e-13   1.4e-14    3.6e-14    1.8e-12   4.3e-14
  mfma<1,2,J>    default  1      1.7e-15    8.6e-14   8.9e-16    -          -         zero
  mfma<1,2,K>    no-wave  3      1.4e-14    7.1e-13   1.7e-14    1.6e-14    8.0e-13   2.3e-14
  mfma<1,33,J>   default  1      2.4e-13    1.2e-11   2.5e-13    -          -         zero
  mfma<1,5,J>    default  3      2.8e-14    1.4e-12   4.7e-14    -          -         zero
  mfma<2,5,K>    default  1      3.7e-14    1.8e-12   3.9e-14    6.0e-14    3.0e-12   4.6e-14
  mfma<2,5,K>    no-wave  4      1.7e-14    8.3e-13   2.5e-14    3.6e-14    1.8e-12   3.9e-14
  mfma<3,9,K>    no-wave  5      4.8e-14    2.4e-12   8.9e-14    7.1e-14    3.6e-12   7.8e-14
  mfma<6,19,K>   no-wave  2      5.0e-14    2.5e-12   5.7e-14    7.1e-14    3.6e-12   5.7e-14
  mfma<9,33,K>   default  1      2.1e-13    1.1e-11   2.1e-13    1.1e-13    5.7e-12   8.5e-14
  mfma<9,33,K>   no-wave  1      1.7e-13    8.5e-12   1.9e-13    4.3e-14    2.1e-12   3.6e-14
  v1<10,lds>     v1       5      2.4e-14    1.2e-12   6.8e-14    3.2e-14    1.6e-12   4.6e-14
  v1<29,lds>     v1       4      6.5e-15    3.3e-13   8.9e-15    2.8e-14    1.4e-12   2.8e-14
  v1<54,lds>     v1       2      2.3e-13    1.2e-11   2.4e-13    3.6e-14    1.8e-12   3.6e-14
  v1<77,global>  default  3      2.3e-13    1.1e-11   2.6e-13    1.4e-13    7.1e-12   1.1e-13
  v1<77,global>  v1       3      5.8e-14    2.9e-12   8.2e-14    7.4e-14    3.7e-12   7.1e-14
  v1<77,lds>     v1       2      1.1e-13    5.4e-12   1.2e-13    8.9e-15    4.4e-13   8.9e-15

  fit case             route    (P|mu nu)  (P|Q)     eps_ref G  bound G   kernel G   lambda_min
  spd-generic-et       default  6.2e-15    7.1e-14   1.3e-13    6.4e-12   1.3e-13    1.9e-05
  spd-stretched-et     default  6.2e-15    7.1e-14   3.7e-13    1.8e-11   3.7e-13    2.0e-05
  spdf-generic-et      default  6.2e-15    7.1e-14   1.3e-13    6.4e-12   1.3e-13    1.9e-05
  spdf-stretched-et    default  6.2e-15    7.1e-14   3.7e-13    1.8e-11   3.7e-13    2.0e-05
  spdf-generic-self    default  4.4e-15    4.3e-14   3.6e-14    1.8e-12   3.7e-14    3.5e-02
  spd-jitter3-et       default  6.2e-15    4.3e-14   2.1e-13    1.0e-11   2.3e-13    1.9e-05
  water-dz-dup         default  1.1e-14    1.4e-14   1.1e-13    5.7e-12   7.4e-14    2.0e-05
  spd-generic-et       chol-v1  6.2e-15    7.1e-14   1.3e-13    6.4e-12   1.2e-13    1.9e-05
  spdf-generic-self    chol-v1  4.4e-15    4.3e-14   3.6e-14    1.8e-12   4.0e-14    3.5e-02
  water-dz-dup         chol-v1  1.1e-14    1.4e-14   1.1e-13    5.7e-12   7.4e-14    2.0e-05

  (J-only instances: K is specified as zero and compared with zero.)  The end-to-end tie (engine's fitted B of
  spd-generic-et through the J/K stage, wave<3,19>): J off by 7.2e-13 and K by 1.0e-13 against 6.7e-12 and 6.6e-12, the
  sum of the J/K bound (2.1e-13, 1.1e-13) and the bound of G (6.4e-12).
  Every kernel sits at the reference's own noise floor: no deviation of a row exceeds 3 x eps_ref and none needs more
  than a seventeenth of its bound (the tie: a ninth).  With the v1
  selection as it stood, (118, 5) and (130, 5) reported v1<54,lds> and K was off by 11.5 and 11.0 (its last 100 and
  3 076 elements zero); a late auxiliary row dropped in the mfma kernel fails exactly the cases that walk three rows
  or more (J off by 17.8 at n = 48, m = 256); a fit that ignores the last ragged block of the metric fails every fit
  case (B^T B off by 28.5 for n_aux = 68) -- all three checked by hand on a scratch build.

Metric spectra of the fit cases (tests/test_df_stage_cases.py prints them): the smallest kept eigenvalue of every
unflagged case is above 1e-8 and nothing lies in [1e-12, 1e-8]; the duplicated-shell case has exactly one eigenvalue
below 1e-12.  The bound of G follows the conditioning: eps_G is eps(float64) x cond x max |G| to within a factor 100
(asserted on the CPU)."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from metalquicha_amd import capi
from tests import df_stage_cases as ds, stages

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    d = tmp_path_factory.mktemp("df_stage")
    ds.write_basis_files(d)
    mp = pytest.MonkeyPatch()
    mp.setenv("MQC_BASIS_PATH", str(d))
    yield str(d)
    mp.undo()


@functools.lru_cache(maxsize=None)
def _jk_reference(key):
    """The oracle's J and K of a case with their noise floors: computed once, shared by every test, never modified."""
    c = ds.JK_BY_KEY[key]
    B, D, C = ds.jk_inputs(c)
    J, K, ej, ek = ds.jk_reference(c, B, D, C)
    J.setflags(write=False); K.setflags(write=False)
    return J, K, ej, ek


@functools.lru_cache(maxsize=None)
def _fit_reference(name):
    c = ds.FIT_BY_NAME[name]
    return [ds.fit_reference(c, f) for f in ds.fit_fragments(c)]


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
        out = os.path.join(tmp, "df_stage_%s.npz" % route)
        env = dict(os.environ, MQC_BASIS_PATH=tmp, **ds.ROUTES[route])
        want = [c.name for c in ds.route_jk_cases(route)] + [c.name for c in ds.route_fit_cases(route)]
        try:
            p = subprocess.run([sys.executable, "-m", "tests.df_stage_child", route, out], cwd=ROOT, env=env, capture_output=True,
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


def _compare_jk(label, inst, expect, J, K, J0, K0, bj, bk, eps_j, eps_k, j_only=False):
    assert J.shape == J0.shape and K.shape == K0.shape
    nan_j, nan_k = int(np.isnan(J).sum()), int(np.isnan(K).sum())
    dj = float(np.max(np.abs(J - J0))) if not nan_j else float("nan")
    dk = float(np.max(np.abs(K - K0))) if not nan_k else float("nan")
    aj, ak = float(np.max(np.abs(J - np.swapaxes(J, -1, -2)))), float(np.max(np.abs(K - np.swapaxes(K, -1, -2))))
    print("DFSTAGE %s instance=%s J: eps_ref=%.3e dev=%.3e bound=%.3e asym=%.1e | K: eps_ref=%.3e dev=%.3e bound=%.3e asym=%.1e%s" % (
        label, inst, eps_j, dj, bj, aj, eps_k, dk, bk, ak, "  (J only: K must be zero)" if j_only else ""))
    assert inst == expect, "%s: the dispatch reports %s, the case expects %s" % (label, inst, expect)
    assert nan_j == 0, "%s: %d NaN in J (elements nothing wrote)" % (label, nan_j)
    assert nan_k == 0, "%s: %d NaN in K (elements nothing wrote)" % (label, nan_k)
    assert dj <= bj, "%s: J off by %.3e (bound %.3e) at %s" % (label, dj, bj, np.unravel_index(np.argmax(np.abs(J - J0)), J.shape))
    assert aj <= bj
    if j_only:
        assert not K.any(), "%s: the J-only instance left something in K" % label      # include/mqc_hip.h: zeros on the mfma route
    else:
        assert dk <= bk, "%s: K off by %.3e (bound %.3e) at %s" % (label, dk, bk, np.unravel_index(np.argmax(np.abs(K - K0)), K.shape))
        assert ak <= bk


_JK_PAIRS = [(c.route, c.name) for c in ds.JK_CASES]


@pytest.mark.parametrize("route,name", _JK_PAIRS, ids=["%s-%s" % p for p in _JK_PAIRS])
def test_jk_matches_oracle(route, name, tmp):
    c = ds.JK_BY_KEY[(route, name)]
    got = _route(route, tmp)
    J0, K0, ej, ek = _jk_reference((route, name))
    _compare_jk("%s/%s rows=%.1f" % (route, name, ds.rows_per_workgroup(c)), str(got["I:" + name]), c.expect, got["J:" + name],
                got["K:" + name], J0, K0, ds.jk_bound(ej, J0), ds.jk_bound(ek, K0), ej, ek,
                j_only=c.exx == 0.0 and c.expect.startswith("mfma"))


_FIT_PAIRS = [(r, c.name) for r in ds.ROUTES for c in ds.route_fit_cases(r)]


@pytest.mark.parametrize("route,name", _FIT_PAIRS, ids=["%s-%s" % p for p in _FIT_PAIRS])
def test_fit_matches_oracle(route, name, tmp):
    c = ds.FIT_BY_NAME[name]
    got = _route(route, tmp)
    refs = _fit_reference(name)
    A3, M, B, flag = got["A3:" + name], got["M:" + name], got["B:" + name], got["F:" + name]
    assert len(refs) == A3.shape[0] == M.shape[0] == B.shape[0] == len(flag)
    for k, r in enumerate(refs):
        label = "%s/%s[%d]" % (route, name, k)
        nan = int(np.isnan(A3[k]).sum() + np.isnan(M[k]).sum() + np.isnan(B[k]).sum())
        d3 = float(np.nanmax(np.abs(A3[k] - r["A3"])))
        d2 = float(np.nanmax(np.abs(M[k] - r["M"])))
        G = B[k].T @ B[k]
        dg, bg = float(np.max(np.abs(G - r["G"]))) if not nan else float("nan"), ds.g_bound(r["eps_G"])
        print("DFSTAGE %s flag=%d n=%d n_aux=%d A3: dev=%.3e M: dev=%.3e bound=%.0e | G: eps_ref=%.3e dev=%.3e bound=%.3e max|G|=%.2e lambda_min=%.2e" % (
            label, int(flag[k]), r["mol"].nao, r["aux"].nao, d3, d2, ds.INT_TOL, r["eps_G"], dg, bg, float(np.max(np.abs(r["G"]))),
            float(np.min(r["w"][r["w"] > 1e-10]))))
        assert nan == 0, "%s: %d NaN (elements no task covers)" % (label, nan)
        assert int(flag[k]) == c.flag, "%s: fit flag %d, expected %d" % (label, int(flag[k]), c.flag)
        assert A3[k].shape == r["A3"].shape
        assert d3 <= ds.INT_TOL, "%s: (P|mu nu) off by %.3e at %s" % (label, d3, np.unravel_index(np.nanargmax(np.abs(A3[k] - r["A3"])), A3[k].shape))
        assert d2 <= ds.INT_TOL, "%s: (P|Q) off by %.3e" % (label, d2)
        assert np.array_equal(M[k], M[k].T), "%s: the metric is not exactly symmetric" % label
        assert dg <= bg, "%s: B^T B off by %.3e (bound %.3e)" % (label, dg, bg)
    for k in range(1, len(refs)):
        assert np.max(np.abs(A3[k] - A3[0])) > 1e-4            # each fragment its own integrals


def test_fitted_tensor_through_the_jk_stage(tmp):
    """The end-to-end tie: B of mqc_hip_df_fit_batch fed into mqc_hip_df_jk_batch with a synthetic D and C gives the J
    and K of build_jk_df(df_tensor(...)) within the sum of the two bounds (the J/K stage's and the fit's)."""
    from oracle import scf_oracle as so
    got = _route("default", tmp)
    r = _fit_reference(ds.TIE_CASE)[0]
    Bu = so.df_tensor(r["mol"], r["aux"])
    D, C = ds.tie_inputs(r["mol"].nao)
    J0, K0, ej, ek = ds.jk_reference_one(Bu, D, np.ascontiguousarray(C[:, :ds.TIE_NOCC]))
    ej, ek = ds.eps_floor(ej, J0), ds.eps_floor(ek, K0)
    bg = ds.g_bound(r["eps_G"])
    n, o = r["mol"].nao, ds.TIE_NOCC
    _compare_jk("default/tie", str(got["I:tie"]), ds.instance_of("default", n, o, 1.0), got["J:tie"], got["K:tie"], J0, K0,
                ds.jk_bound(ej, J0) + bg, ds.jk_bound(ek, K0) + bg, ej, ek)


def test_refusals(tmp):
    """Null pointers and sizes out of range (J/K stage), and what a density-fitted SCF refuses (fit): each returns its
    error and writes nothing."""
    import ctypes as C
    from tests.helpers import fragment_bohr
    lib, ctx = capi.load_library(), capi.get_context()
    c = ds.JK_BY_KEY[("default", "n7-o5-x1-a24-m1")]
    B, D, Cm = ds.jk_inputs(c)
    J, K = np.full_like(D, np.nan), np.full_like(D, np.nan)
    route = C.create_string_buffer(32)
    args = [ctx, 1, 7, 5, 24, C.c_double(1.0), capi.dptr(B), capi.dptr(D), capi.dptr(Cm), capi.dptr(J), capi.dptr(K), route, 32]
    for k in (0, 6, 7, 8, 9, 10, 11):
        bad = list(args); bad[k] = None
        assert lib.mqc_hip_df_jk_batch(*bad) == capi.ERR_VALIDATION
    for k, v in ((1, 0), (1, -1), (2, 0), (2, 141), (3, 0), (3, 8), (4, 0), (5, C.c_double(-0.5)), (5, C.c_double(float("nan"))),
                 (5, C.c_double(float("inf")))):
        bad = list(args); bad[k] = v
        assert lib.mqc_hip_df_jk_batch(*bad) == capi.ERR_VALIDATION, (k, v)
    assert np.isnan(J).all() and np.isnan(K).all()

    def refused(code, text, *a):
        with pytest.raises(capi.HipBackendError) as ei:
            stages.df_fit_batch(*a)
        assert ei.value.code == code and text in ei.value.message, ei.value.message

    rng = np.random.default_rng(3)
    from tests.helpers import water_at
    w6 = fragment_bohr([8, 1, 1] * 6, np.vstack([water_at(rng, [5.6 * i, 0.0, 0.0]) for i in range(6)]))        # n = 144
    water, oh = fragment_bohr(*ds.WATER), fragment_bohr([8, 1], [[0.0, 0.0, 0.0], [0.0, 0.0, 1.8]], multiplicity=2)
    refused(capi.ERR_UNSUPPORTED, "n_ao = 140", "cc-pvdz", ds.ET, [w6])
    refused(capi.ERR_VALIDATION, "elements of the first", "cc-pvdz", ds.ET, [water, oh])
    with pytest.raises(Exception) as ei:
        stages.df_fit_batch("6-31g*", ds.ET, [water])
    assert "artesian" in str(ei.value)
