"""CPU checks of tests/jk_broadcast_cases.py: the GPU test (tests/test_gpu_jk_broadcast.py) must not pass vacuously."""
import numpy as np
import pytest

from tests import jk_broadcast_cases as bc, jk_stage_cases as jc


@pytest.mark.parametrize("n", bc.SIZES)
def test_unit_pairs_cover_every_edge(n):
    """Every boundary of a group of eight and of a row of 16 lanes below n, from both sides, the first and the last
    function, on and off the diagonal -- each as a and as b within the 64 fragments."""
    pairs, distinct = bc.unit_pairs(n)
    assert len(pairs) == bc.NFRAG and distinct <= bc.NFRAG and len(set(pairs)) == distinct
    a_seen, b_seen = {a for a, _ in pairs}, {b for _, b in pairs}
    edges = {v for v in bc.EDGES if v < n}
    assert a_seen == edges and b_seen == edges
    assert {0, n - 1} <= edges
    for g16 in range(0, n, 16):            # every register of 16: its first and its last lane in use
        assert {g16, min(g16 + 15, n - 1)} <= edges
    for g8 in range(0, n, 8):              # every group of eight has an element, at its first or its last place
        assert edges & {g8, g8 + 7}
    assert {7, 8} <= edges and {15, 16, 17} <= edges     # a boundary of eight inside a register, and one between registers, from both sides
    assert any(a == b for a, b in pairs) and any(a != b for a, b in pairs)
    assert all(a >= b for a, b in pairs)
    for f in (0, 1, bc.NFRAG - 1):
        D = bc.unit_density(n, f)
        a, b = pairs[f]
        assert D.sum() == 2.0 and D[a, b] == D[b, a] == (2.0 if a == b else 1.0) and np.array_equal(D, D.T)


@pytest.mark.parametrize("n", bc.SIZES)
def test_partial_rows_are_partial(n):
    rows = bc.partial_rows(n)
    assert rows and all((i + 1) % 8 for i in rows) and all(i < n for i in rows)
    # the first group, groups inside the first and the second register, and at n = 48 the last group of the last register
    assert {i // 8 for i in rows} == ({0, 1, 2, 5} if n == 48 else {0, 1, 2})
    assert 0 in rows and any(i % 8 == 6 for i in rows) and any(i % 8 == 0 for i in rows)
    for f in range(len(rows)):
        M, D, i = bc.partial_fragment(n, f)
        assert i == rows[f] and np.array_equal(M, M.T)
        k, _ = np.tril_indices(n)
        L = np.tril(M)
        assert not L[k != i].any() and L[k == i].any()
        assert np.count_nonzero(D) > n * n // 2


@pytest.mark.parametrize("n", bc.SIZES)
def test_split_patterns_split_their_block(n):
    """Each of the six kinds flags exactly one row of its block and keeps the other; the flagged block is read short."""
    np_ = jc.npair(n)
    assert int(np.sum(2 * bc.split_shell_l(n) + 1)) == n
    full = jc.expected_loaded(n)
    seen = set()
    for f in range(len(bc.SPLIT_KINDS)):
        pos, row = bc.SPLIT_KINDS[f]
        rz = bc.split_row_flags(n, f)
        t = bc.split_block(n, pos)
        rl = np_ - 1 - t
        assert t < rl
        assert (bool(rz[rl]), bool(rz[t])) == ((True, False) if row == "long" else (False, True))
        assert 0 < jc.expected_loaded(n, rz) <= full         # the one-element short row of the first block saves no chunk
        assert (jc.expected_loaded(n, rz) < full) == ((pos, row) != ("first", "short"))
        M, _ = bc.split_fragment(n, f)
        L = np.tril(M)
        assert not L[rz].any() and L[rl if row == "short" else t].any()
        seen.add((pos, row))
    assert len(seen) == 6 and bc.NFRAG >= 6
    assert bc.split_block(n, "first") == 0 and bc.split_block(n, "last") == (np_ + 1) // 2 - 1
    Q = bc.split_q(n)
    assert Q.shape == (bc.NFRAG, len(bc.SPLIT_L[n]), len(bc.SPLIT_L[n])) and set(np.unique(Q)) == {jc.Q_DEAD, jc.Q_LIVE}


def test_the_cases_take_the_triangle():
    for n in bc.SIZES:
        for route in bc.ROUTES:
            inst, gx = jc.instance_of(n, bc.NFRAG, False, jc.ROUTES[route])
            assert inst == "tri<12,10>" and (gx == 1) == (route == "wg1")
    assert bc.FLOAT_CASE.expect == ("tri<12,10>", 1)
