"""Host checks of tests/df_stage_cases.py: every instance of launch_df_jk has a case that lands on it, the multi-row
cases walk the rows they claim, every reference is self-consistent between float64 and np.longdouble, every bound stays
under the project's 1e-11 cap; the fit cases cover every three- and two-centre class on different atoms and their metrics
keep clear of the 1e-10 eigenvalue cut.  No GPU.

`python -m tests.test_df_stage_cases` prints eps_ref and the bound of every case."""
import functools
import re

import numpy as np
import pytest

from tests import df_stage_cases as ds


# ---- J/K cases -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ds.JK_CASES, ids=lambda c: "%s-%s" % (c.route, c.name))
def test_jk_case_lands_on_its_instance(case):
    n, o = case.n, case.nocc
    assert 1 <= o <= n <= 140 and case.naux >= 1 and case.m >= 1
    assert ds.instance_of(case.route, n, o, case.exx) == case.expect
    # the invariant of the v1 selection, and the rules recomputed from kern_df.hip's expressions
    if case.expect.startswith("v1"):
        nv, lds = int(re.findall(r"\d+", case.expect)[1]), case.expect.endswith("lds>")
        assert nv * 256 >= n * n
        assert lds == (8 * (n * (n + 1) + n * o + n * (o + 1) + 8) <= 150 * 1024)
    elif case.expect.startswith("wave"):
        ntc, nlw = [int(x) for x in re.findall(r"\d+", case.expect)]
        assert n <= 48 and o <= 16 and case.exx != 0.0 and case.route == "default"
        assert ntc == -(-n // 16) and nlw * 64 >= ds.npair_of(n)
    else:
        jm, nld = [int(x) for x in re.findall(r"\d+", case.expect)]
        nt = -(-n // 16)
        assert nld * 256 >= ds.npair_of(n)
        assert (case.exx != 0.0) == case.expect.endswith("K>")
        if case.exx != 0.0:
            assert jm * 4 >= nt * (nt + 1) // 2
    assert case.m * case.naux * ds.npair_of(n) * 8 < 256e6            # B of one case under 256 MB


def test_every_instance_and_edge_has_a_case():
    assert {c.expect for c in ds.JK_CASES} == set(ds.REQUIRED_INSTANCES)
    have = {(c.route, c.n, c.nocc) for c in ds.JK_CASES if c.exx != 0.0}
    table = {"default": [(7, 5), (16, 16), (17, 1), (32, 16), (33, 9), (48, 10), (48, 17), (128, 32), (128, 33), (129, 30)],
             "no-wave": [(7, 5), (31, 9), (32, 9), (48, 10), (49, 12), (64, 20), (65, 7), (96, 24), (97, 19)],
             "v1": [(7, 5), (50, 10), (51, 10), (86, 14), (87, 20), (117, 10), (118, 5), (130, 5), (118, 30), (140, 35)]}
    for route, shapes in table.items():
        assert {(route,) + s for s in shapes} <= have
    assert {("default", 7, 5), ("default", 48, 10), ("default", 128, 20)} <= {(c.route, c.n, c.nocc) for c in ds.JK_CASES if c.exx == 0.0}
    for fam in ("wave", "mfma", "v1"):
        mine = [c for c in ds.JK_CASES if c.expect.startswith(fam)]
        assert {1, 37} <= {c.naux for c in mine if c.m == 1}
        assert any(c.m == 3 for c in mine) and any(c.m >= 2048 and c.n == 7 for c in mine)
        assert any(c.rows and ds.rows_per_workgroup(c) >= 3.0 for c in mine)
    # the multi-row shapes the issue names
    multi = {(c.expect[:4], c.n, c.nocc) for c in ds.JK_CASES if c.rows and ds.rows_per_workgroup(c) >= 3.0}
    assert {("wave", 48, 10), ("mfma", 48, 10), ("mfma", 64, 20), ("v1<1", 50, 10)} <= multi
    # the mfma route gives up exactly where the table says: three orbital tiles at n = 128, nt = 9
    assert ds.mfma_instance(128, 32, 1.0) and not ds.mfma_instance(128, 33, 1.0) and not ds.mfma_instance(129, 1, 1.0)


def test_rows_figures_are_the_grid_formulas():
    for c in ds.JK_CASES:
        if c.rows:
            figure = float(re.findall(r"[\d.]+", c.rows)[-1])
            assert abs(figure - ds.rows_per_workgroup(c)) < 0.06, (c.name, c.rows, ds.rows_per_workgroup(c))


@functools.lru_cache(maxsize=None)
def _jk_measured(key):
    c = ds.JK_BY_KEY[key]
    B, D, C = ds.jk_inputs(c)
    return (c, B, D, C) + ds.jk_reference(c, B, D, C)


# one case per instance, the largest shapes and the n_aux edges: the references of the large batches are formed on the GPU
# machine's CPU in the GPU test, by the same function
_MEASURED = [k for k, c in ds.JK_BY_KEY.items() if c.m == 1]


@pytest.mark.parametrize("key", _MEASURED, ids=["%s-%s" % k for k in _MEASURED])
def test_jk_reference_is_self_consistent_and_bounded(key):
    c, B, D, C, J, K, eps_j, eps_k = _jk_measured(key)
    assert np.allclose(np.swapaxes(C, 1, 2) @ C, np.eye(c.n), atol=1e-12) and np.array_equal(D, np.swapaxes(D, 1, 2))
    assert B.shape == (c.m, c.naux, ds.npair_of(c.n))
    assert c.m == 1 or np.max(np.abs(B[0] - B[1])) > 0.1               # every fragment its own tensor
    # float64 against longdouble and against the reversed order: the same contraction to rounding, far below the cap
    for what, ref, eps in (("J", J, eps_j), ("K", K, eps_k)):
        scale = max(1.0, float(np.max(np.abs(ref))))
        bound = ds.jk_bound(eps, ref)
        print("DFSTAGE-CPU %s/%s %s max|ref|=%.3e eps_ref=%.3e bound=%.3e cap=%.3e" % (key + (what, scale, eps, bound, ds.JK_CAP * scale)))
        assert np.isfinite(ref).all() and np.max(np.abs(ref - np.swapaxes(ref, 1, 2))) <= bound
        assert eps <= 1e-13 * scale
        assert 0.0 < bound <= ds.JK_CAP * scale
    # K against the density form of the exchange, K = B D' B with D' = 2 C_occ C_occ^T: the occupied block is what is used
    from oracle import scf_oracle as so
    Co = C[0][:, :c.nocc]
    _, Kd = so.build_jk_df(ds.unpack(B[0]), 2.0 * Co @ Co.T)
    assert np.max(np.abs(Kd - K[0])) <= 1e-11 * max(1.0, float(np.max(np.abs(K))))


# ---- fit cases -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def basis_dir(tmp_path_factory):
    d = tmp_path_factory.mktemp("df_stage_basis")
    ds.write_basis_files(d)
    mp = pytest.MonkeyPatch()
    mp.setenv("MQC_BASIS_PATH", str(d))
    yield d
    mp.undo()


@functools.lru_cache(maxsize=None)
def _fit_measured(name):
    c = ds.FIT_BY_NAME[name]
    return c, [ds.fit_reference(c, f) for f in ds.fit_fragments(c)]


def test_every_integral_class_occurs_on_different_atoms(basis_dir):
    c3, c2 = set(), set()
    for c in ds.FIT_CASES:
        if c.flag == 0:
            r = _fit_measured(c.name)[1][0]
            a, b = ds.classes_seen(r["mol"], r["aux"])
            c3 |= a
            c2 |= b
    assert len(ds.DF3C_CLASSES) == 24 and len(ds.DF2C_CLASSES) == 10
    assert set(ds.DF3C_CLASSES) <= c3 and set(ds.DF3C_GENERAL) <= c3 and set(ds.DF2C_CLASSES) <= c2
    # the spd probe with the even-tempered set alone already has every non-f class
    r = _fit_measured("spd-generic-et")[1][0]
    assert set(ds.DF3C_CLASSES) <= ds.classes_seen(r["mol"], r["aux"])[0]
    sizes = {c.name: (_fit_measured(c.name)[1][0]["mol"].nao, _fit_measured(c.name)[1][0]["aux"].nao) for c in ds.FIT_CASES}
    assert sizes["spd-generic-et"][0] == 40 and sizes["spdf-generic-et"][0] == 68
    assert sizes["spdf-generic-self"][1] == 68 and 68 % 16 == 4         # a ragged last Cholesky block
    assert sizes["spd-generic-et"][1] % 16 != 0
    # no vanishing coordinate, four distinct centres
    for g in ("generic", "stretched"):
        xyz = ds.cc.CASES[g]().coordinates.T
        assert np.min(np.abs(xyz)) > 0.2 and len({tuple(x) for x in xyz}) == 4


@pytest.mark.parametrize("name", [c.name for c in ds.FIT_CASES])
def test_fit_case_conditioning_and_bound(name, basis_dir):
    c, refs = _fit_measured(name)
    for k, r in enumerate(refs):
        w, G, eps = r["w"], r["G"], r["eps_G"]
        gap_lo = float(np.max(w[w < 1e-10])) if (w < 1e-10).any() else 0.0
        print("DFSTAGE-CPU fit %s[%d] n=%d n_aux=%d lambda_min kept=%.3e largest cut=%.3e cond(kept)=%.3e max|G|=%.3e eps_G=%.3e bound=%.3e" % (
            name, k, r["mol"].nao, r["aux"].nao, float(np.min(w[w > 1e-10])), gap_lo, float(w[-1] / np.min(w[w > 1e-10])),
            float(np.max(np.abs(G))), eps, ds.g_bound(eps)))
        assert ds.conditioning_ok(c, w), w[:4]
        assert np.array_equal(r["M"], r["M"].T) or np.max(np.abs(r["M"] - r["M"].T)) < 1e-14
        assert np.isfinite(G).all() and np.max(np.abs(G - G.T)) <= eps
        # the two fits agree to the conditioning of the kept spectrum: eps(float64) x cond x max |G|, with room of 100
        cond = float(w[-1] / np.min(w[w > 1e-10]))
        assert eps <= 100.0 * np.finfo(np.float64).eps * cond * float(np.max(np.abs(G)))
    if len(refs) > 1:
        for k in range(1, len(refs)):
            assert np.max(np.abs(refs[k]["A3"] - refs[0]["A3"])) > 1e-4          # no fragment's A3 equals another's


def test_routes_cover_the_switches():
    assert set(ds.ROUTES) == {"default", "no-wave", "v1", "chol-v1"}
    assert ds.ROUTES["no-wave"] == {"MQC_HIP_DF_WAVE": "0"} and ds.ROUTES["v1"] == {"MQC_HIP_DF_V1": "1"}
    assert ds.ROUTES["chol-v1"] == {"MQC_HIP_DF_CHOL_V1": "1"}
    assert not ds.route_jk_cases("chol-v1") and ds.route_fit_cases("chol-v1") and not ds.route_fit_cases("v1")
    assert {c.name for c in ds.route_fit_cases("default")} == set(ds.FIT_BY_NAME)


if __name__ == "__main__":
    import tempfile, os
    for key in ds.JK_BY_KEY:
        c, B, D, C, J, K, ej, ek = _jk_measured(key)
        print("%-8s %-22s %-14s eps_J=%.2e bound_J=%.2e eps_K=%.2e bound_K=%.2e" % (key + (c.expect, ej, ds.jk_bound(ej, J), ek, ds.jk_bound(ek, K))))
    with tempfile.TemporaryDirectory() as d:
        ds.write_basis_files(d)
        os.environ["MQC_BASIS_PATH"] = d
        for c in ds.FIT_CASES:
            for r in _fit_measured(c.name)[1]:
                print("%-20s eps_G=%.2e bound=%.2e max|G|=%.2e" % (c.name, r["eps_G"], ds.g_bound(r["eps_G"]), np.max(np.abs(r["G"]))))
