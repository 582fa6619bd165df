"""Stage tests of the multi-density J/K stream (kern_cphf.hip): mqc_hip_jk_multi_batch runs launch_jk_multi once on
given square tensors and up to three densities per fragment.  The inputs are the exact-integer fragments of
tests/jk_stage_cases.py, on which J and K are exact in FP64 in any order of summation, so the stream must EQUAL the
reference for each density.  The reference is jk_brute where its element-by-element Python loop over n^4 integrals is
affordable (n <= 24) and jk_reference at every size; the two are asserted equal wherever both run, and on exact inputs
they are equal at every size by construction (tests/test_jk_stage_cases.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from metalquicha_amd import capi
from tests import cphf_stage as cs
from tests import jk_stage_cases as jc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (1, 2, 7, 24, 48, 50, 63, 64, 65, 89, 90, 116)      # 50: four waves with K in LDS, the one instance the others miss
BRUTE_MAX = 24


def _check_exact(n, nd, Ms, D, J, K, label):
    for f in range(cs.NFRAG):
        if f == cs.DONE:
            # a finished fragment: the poison or zero, never anything else
            for X in (J[f], K[f]):
                assert np.all(np.isnan(X) | (X == 0.0)), "%s: the finished fragment was written" % label
            continue
        for d in range(nd):
            J0, K0 = jc.jk_reference(Ms[f], D[f, d])
            if n <= BRUTE_MAX:
                Jb, Kb = jc.jk_brute(Ms[f], D[f, d])
                assert np.array_equal(Jb, J0) and np.array_equal(Kb, K0)
                J0, K0 = Jb, Kb
            bad_j, bad_k = int(np.sum(J[f, d] != J0)), int(np.sum(K[f, d] != K0))
            assert bad_j == 0 and bad_k == 0, "%s fragment %d density %d: %d elements of J and %d of K differ" % (label, f, d, bad_j, bad_k)
            if not D[f, d].any():
                assert not J[f, d].any() and not K[f, d].any()


@pytest.mark.parametrize("n", SIZES)
def test_three_densities_exact(n):
    Ms, D, J, K, route = cs.run_exact(n, 3)
    print("JKMULTI n=%d route %s" % (n, route))
    assert route.startswith("multi<3,")
    _check_exact(n, 3, Ms, D, J, K, "n=%d %s" % (n, route))


@pytest.mark.parametrize("n", (7, 65))
@pytest.mark.parametrize("nd", (1, 2))
def test_fewer_densities_exact(n, nd):
    Ms, D, J, K, route = cs.run_exact(n, nd)
    _check_exact(n, nd, Ms, D, J, K, "n=%d nd=%d %s" % (n, nd, route))


def test_float_inputs_within_rounding_bounds():
    """Normal deviates over twelve decades (n = 25, three fragments, none finished): every element within the bound of
    an FP64 evaluation in any order, against a long-double reference."""
    n = 25
    Ms, Ds = [], []
    for f in range(cs.NFRAG):
        M, Da = jc.float_fragment(n, f)
        Ms.append(M)
        Ds.append(np.stack([Da, np.zeros_like(Da), jc.float_fragment(n, f, seed=778)[1]]))
    D = np.stack(Ds)
    J, K, route = cs.jk_multi_batch(np.stack([M.reshape(-1) for M in Ms]), D)
    assert not np.isnan(J).any() and not np.isnan(K).any()
    for f in range(cs.NFRAG):
        for d in (0, 2):
            Jl, Kl = jc.jk_reference(Ms[f].astype(np.longdouble), D[f, d].astype(np.longdouble))
            bj, bk = jc.jk_bounds(Ms[f], D[f, d])
            ej, ek = np.abs(J[f, d] - Jl.astype(np.float64)), np.abs(K[f, d] - Kl.astype(np.float64))
            print("JKMULTI float f=%d d=%d: J dev/bound %.3e, K dev/bound %.3e" % (f, d, float(np.max(ej / bj)), float(np.max(ek / bk))))
            assert np.all(bj > 0) and np.all(bk > 0)
            assert np.all(ej <= bj) and np.all(ek <= bk)
        assert not J[f, 1].any() and not K[f, 1].any()


def test_single_density_route_gives_the_same_answers(tmp_path):
    """MQC_HIP_CPHF_MULTI=0 in a fresh process: three launches of the single-density stream, the same J and K on n = 48."""
    out = str(tmp_path / "single.npz")
    p = subprocess.run([sys.executable, "-m", "tests.cphf_stage", "48", out], cwd=ROOT, env=dict(os.environ, MQC_HIP_CPHF_MULTI="0"),
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    got = np.load(out)
    assert str(got["route"]).startswith("single:")
    Ms, D = cs.exact_inputs(48, 3)
    _check_exact(48, 3, Ms, D, got["J"], got["K"], "n=48 single")


def test_refusals():
    lib, ctx = capi.load_library(), capi.get_context()
    n = 2
    T, D = np.zeros((1, 9)), np.zeros((1, 3, n, n))
    J, K = np.zeros_like(D), np.zeros_like(D)
    route = __import__("ctypes").create_string_buffer(64)
    ok = [ctx, 1, n, 3, capi.dptr(T), capi.dptr(D), None, capi.dptr(J), capi.dptr(K), route, len(route)]
    assert lib.mqc_hip_jk_multi_batch(*ok) == 0
    for k, v in ((4, None), (5, None), (7, None), (8, None), (9, None), (2, 0), (2, 117), (3, 0), (3, 4), (1, 0)):
        bad = list(ok)
        bad[k] = v
        assert lib.mqc_hip_jk_multi_batch(*bad) == capi.ERR_VALIDATION, (k, v)
