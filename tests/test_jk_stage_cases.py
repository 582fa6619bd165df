"""CPU checks of what tests/test_gpu_jk_stage.py stands on (tests/jk_stage_cases.py): the Python statement of the
triangular layout against the engine's jk_tri_block, the dispatch model against the host build of jk_tri_layout and
jk_tri_lds_bytes, the reference against a brute-force four-index einsum, the exactness of the integer inputs, the float
bound, and the case list (every reachable instance has a case)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import jk_stage_cases as jc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def hostcheck():
    subprocess.check_call(["bash", os.path.join(ROOT, "tests", "host", "build.sh")], stdout=subprocess.DEVNULL)
    lib = ctypes.CDLL(os.path.join(ROOT, "tests", "host", "libhostcheck.so"))
    lib.hostcheck_jk_tri_lds_bytes.restype = ctypes.c_ulonglong
    return lib


def test_layout_matches_the_engine(hostcheck):
    for n in range(8, 65):
        np_ = jc.npair(n)
        nblk = (np_ + 1) // 2
        tab = np.zeros(nblk + np_, dtype=np.int32)
        pb = hostcheck.hostcheck_jk_tri_block(np_, tab.ctypes.data_as(ctypes.POINTER(ctypes.c_int)))
        mine_pb, sb, se, rows = jc.tri_table(np_)
        assert pb == mine_pb, n
        assert tab[:nblk].tolist() == list(sb), n
        assert tab[nblk:].tolist() == list(rows), n
        assert max(se) <= pb and pb % 2 == 0
        assert hostcheck.hostcheck_jk_tri_lds_bytes(n) == jc.tri_lds_bytes(n), n
    assert jc.tri_table(jc.npair(40))[0] == 874 and jc.tri_table(jc.npair(48))[0] == 1240
    assert jc.tri_table(jc.npair(56))[0] == 1672 and jc.tri_table(jc.npair(64))[0] == 2171 + 1


def test_layout_decision_matches_the_engine(hostcheck):
    for n in range(1, 118):
        for nfrag in (1, 3, 63, 64, 65, 768, 2016):
            for uhf in (0, 1):
                assert bool(hostcheck.hostcheck_jk_tri_layout(n, nfrag, uhf)) == jc.tri_layout(n, nfrag, bool(uhf)), (n, nfrag, uhf)
    assert [n for n in range(1, 118) if jc.tri_layout(n, 64)] == [40, 48]
    assert jc.tensor_layout(48, 64) == (True, 1240, 588 * 1240) and jc.tensor_layout(48, 63) == (False, 0, 1176 ** 2)
    assert jc.tensor_layout(48, 64, env=jc.ROUTES["tri0"])[0] is False


@pytest.mark.parametrize("n", [1, 2, 3, 5, 8, 13, 40])
def test_pack_round_trip_and_placement(n):
    rng = np.random.default_rng(n)
    np_ = jc.npair(n)
    M = rng.integers(1, 100, size=(np_, np_)).astype(np.float64)
    M = np.tril(M) + np.tril(M, -1).T
    T = jc.tri_pack(M)
    pb, sb, se, rows = jc.tri_table(np_)
    assert T.shape == ((np_ + 1) // 2 * pb,)
    assert np.array_equal(jc.tri_unpack(T, np_), M)
    # element by element, from the comment: block t = [row np-1-t, zeros | row t, zeros, zeros to the block's end]
    for t in range((np_ + 1) // 2):
        blk, rl = T[t * pb:(t + 1) * pb], np_ - 1 - t
        want = np.zeros(pb)
        want[:rl + 1] = M[rl, :rl + 1]; want[rl] *= 0.5
        if t < rl:
            want[sb[t]:sb[t] + t + 1] = M[t, :t + 1]; want[sb[t] + t] *= 0.5
            assert sb[t] >= rl + 1
        assert np.array_equal(blk, want), (n, t)


def test_dispatch_table():
    """The ranges of the instances, as the sizes give them."""
    def span(nfrag, uhf=False, env=None):
        out = {}
        for n in range(1, jc.N_MAX + 1):
            out.setdefault(jc.instance_of(n, nfrag, uhf, env)[0], []).append(n)
        return {k: (v[0], v[-1], len(v)) for k, v in out.items()}

    small = span(3)
    assert small == {"wave<1,lds,4,5,reg>": (1, 24, 24), "wave<1,lds,4,10,reg>": (25, 35, 11), "wave<1,lds,4,19,reg>": (36, 48, 13),
                     "wave<1,lds,4,0,reg>": (49, 64, 16), "wave<2,lds,4,0,mem>": (65, 66, 2), "rowcoop<2,8>": (67, 89, 23),
                     "wave<2,global,2,0,mem>": (90, 116, 27)}
    big = span(64)
    assert big["wave<1,lds,12,10,reg>"] == (25, 35, 11) and big["tri<12,10>"] == (40, 48, 2)
    assert big["wave<1,lds,12,19,reg>"] == (36, 47, 11) and "wave<1,lds,12,19,reg,full8>" not in big
    for k in ("wave<1,lds,4,5,reg>", "wave<1,lds,4,0,reg>", "wave<2,lds,4,0,mem>", "rowcoop<2,8>", "wave<2,global,2,0,mem>"):
        assert big[k] == small[k]
    assert span(64, uhf=True)["wave<1,lds,12,19,reg,full8>"] == (40, 48, 2)
    assert span(64, env=jc.ROUTES["tri0"])["wave<1,lds,12,19,reg,full8>"] == (40, 48, 2)
    assert span(3, env=jc.ROUTES["rowcoop0"])["wave<2,global,4,0,mem>"] == (67, 89, 23)
    assert jc.incore_supported(116) and not jc.incore_supported(117)
    assert 8 * 3 * jc.npair(116) == 162864
    # the triangle's grid: one workgroup per fragment from 768 fragments on; the overrides
    assert jc.instance_of(48, 64)[1] == 12 and jc.instance_of(48, 768)[1] == 1 and jc.instance_of(48, 2016)[1] == 1
    assert jc.instance_of(48, 64, env=jc.ROUTES["wg1"])[1] == 1 and jc.instance_of(40, 64, env=jc.ROUTES["wg5"])[1] == 5
    assert jc.instance_of(40, 64, env=jc.ROUTES["wg1000"])[1] == 35 and jc.instance_of(48, 64, env=jc.ROUTES["wg1000"])[1] == 49
    # no admissible shape has three or four chunks of 64 functions
    assert not any(i.startswith(("wave<3", "wave<4")) for i in jc.reachable_instances())


def test_every_reachable_instance_has_a_case():
    covered = {(c.expect[0]) for c in jc.CASES}
    assert covered == jc.reachable_instances()
    floats = {c.expect[0] for c in jc.CASES if c.kind == "float"}
    assert floats == jc.reachable_instances()
    for c in jc.CASES:
        if c.pattern or (c.route.startswith("wg")):
            assert c.expect[0] == "tri<12,10>"
    assert {c.expect[1] for c in jc.CASES if c.route == "wg1"} == {1}
    assert jc.BY_NAME[("tri0", "n48-m64")].expect[0] == "wave<1,lds,12,19,reg,full8>"
    assert jc.BY_NAME[("rowcoop0", "n89-m3")].expect[0] == "wave<2,global,4,0,mem>"


@pytest.mark.parametrize("n", [1, 2, 5, 12])
def test_reference_against_brute_force(n):
    for maker in (jc.exact_fragment, jc.float_fragment):
        M, D = maker(n, 0)
        assert np.array_equal(M, M.T) and np.array_equal(D, D.T)
        J, K = jc.jk_reference(M.astype(np.longdouble), D.astype(np.longdouble))
        Jb, Kb = jc.jk_brute(M.astype(np.longdouble), D.astype(np.longdouble))
        scale = float(np.max(np.abs(Kb))) + float(np.max(np.abs(Jb))) + 1.0
        assert float(np.max(np.abs(J - Jb))) <= 1e-17 * scale * n * n and float(np.max(np.abs(K - Kb))) <= 1e-17 * scale * n * n
        assert np.array_equal(J, J.T)


@pytest.mark.parametrize("n", [7, 25, 48])
def test_exact_inputs_do_not_depend_on_the_order_of_summation(n):
    M, D = jc.exact_fragment(n, 1)
    assert np.max(np.abs(M)) <= 7 and np.max(np.abs(D)) <= 3 and np.array_equal(M, np.round(M))
    J, K = jc.jk_reference(M, D)
    J2, K2 = jc.jk_reference(M, D, flip=True)
    assert J.tobytes() == J2.tobytes() and K.tobytes() == K2.tobytes()
    Jl, Kl = jc.jk_reference(M.astype(np.longdouble), D.astype(np.longdouble))
    assert np.array_equal(J, Jl.astype(np.float64)) and np.array_equal(K, Kl.astype(np.float64))
    # the same through the triangle with its halved diagonal: multiples of 0.5
    T = jc.tri_pack(M)
    assert np.array_equal(2 * T, np.round(2 * T)) and np.array_equal(jc.tri_unpack(T, M.shape[0]), M)
    # the largest partial sum any order can meet, at the largest admissible size
    assert jc.npair(jc.N_MAX) * 7 * 6 < 2 ** 20 and jc.N_MAX ** 2 * 7 * 3 < 2 ** 20


def test_float_bound_holds_for_float64_and_is_not_slack():
    """float64 evaluations in two orders stay within the bound of the longdouble reference; an element dropped from
    the tensor does not."""
    c = jc.Case("default", 25, 3, kind="float")
    M, D = jc.fragment_inputs(c, 0)
    Jl, Kl = jc.jk_reference(M.astype(np.longdouble), D.astype(np.longdouble))
    bj, bk = jc.jk_bounds(M, D)
    for flip in (False, True):
        J, K = jc.jk_reference(M, D, flip=flip)
        assert np.all(np.abs(J - Jl.astype(np.float64)) <= bj) and np.all(np.abs(K - Kl.astype(np.float64)) <= bk)
    big = np.unravel_index(np.argmax(np.abs(M) * (np.abs(D[np.tril_indices(25)])[None, :] > 1e-3)), M.shape)
    Mx = M.copy(); Mx[big] = 0.0; Mx[big[::-1]] = 0.0
    J, K = jc.jk_reference(Mx, D)
    assert np.any(np.abs(J - Jl.astype(np.float64)) > bj)


def test_screening_inputs():
    for n in (40, 48):
        assert int(np.sum(2 * jc.shell_l(n) + 1)) == n
        np_ = jc.npair(n)
        full = jc.expected_loaded(n)
        _, _, se, _ = jc.tri_table(np_)
        assert full == sum(min(-(-e // 128), 10) for e in se)
        for p in jc.PATTERNS:
            F = jc.shell_flags(n, p, 5)
            rz = jc.row_flags(n, F)
            assert np.array_equal(F, F.T) and rz.shape == (np_,)
            if p == "first":
                assert np.flatnonzero(rz).tolist() == [0]
            if p == "last":
                assert np.flatnonzero(rz).tolist() == [np_ - 1]
            if p == "cross":
                assert rz.sum() == (n // 2) ** 2 and jc.expected_loaded(n, rz) < full
            if p == "third":
                assert 0 < rz.sum() < np_
            if p == "all":
                assert rz.all() and jc.expected_loaded(n, rz) == 0
            if p == "none":
                assert not rz.any() and jc.expected_loaded(n, rz) == full
            # powers of two, nothing on the threshold
            q = np.where(F, jc.Q_DEAD, jc.Q_LIVE)
            prod = q * q.max()
            assert np.all((prod < jc.Q_THRESH / 1e3) | (prod > jc.Q_THRESH * 1e3))
            assert np.array_equal(prod < jc.Q_THRESH, F)
        # no block of a reachable triangle ends one element into a chunk: there ceil(se / 128) is also (se + 126) >> 7,
        # and a kernel that rounded the last chunk that way could not be told apart (n = 56 has such blocks, and is refused)
        assert not [e for e in se if e % 128 == 1]
        c = jc.Case("wg1", n, 64, pattern="cross")
        M, _ = jc.fragment_inputs(c, 2)
        rz = jc.row_flags(n, jc.shell_flags(n, "cross", 2))
        assert np.array_equal(M, M.T) and not np.tril(M)[rz].any() and np.triu(M, 1)[rz].any()
        T = jc.tri_pack(M)
        assert np.array_equal(jc.tri_unpack(T, np_), M)


def test_refused_triangle_has_blocks_one_element_into_a_chunk():
    assert len([e for e in jc.tri_table(jc.npair(56))[2] if e % 128 == 1]) > 0 and not jc.tri_layout(56, 64)


def test_fragments_of_a_case_are_distinct():
    for kind, maker in (("exact", jc.exact_fragment), ("float", jc.float_fragment)):
        a, b = maker(25, 0), maker(25, 1)
        assert not np.array_equal(a[0], b[0]) and not np.array_equal(a[1], b[1])
    a, b = jc.done_sets(64)
    assert 18 <= len(a) <= 24 and 18 <= len(b) <= 24 and not set(a) & set(b) and len(set(range(64)) - set(a) - set(b)) > 10
