"""Cases of the broadcast tests of the triangular J/K stream (tests/test_jk_broadcast_cases.py on the CPU,
tests/test_gpu_jk_broadcast.py with tests/jk_broadcast_child.py on the GPU).  Test infrastructure; layouts, inputs and
references are those of tests/jk_stage_cases.py.

The exchange of jk_tri_kernel keeps a density row in registers, 16 values per register pair, and an FMA takes D[l] as
the broadcast of lane l % 16 of register l / 16; the l loop is unrolled in groups of eight with the reads of a group in
flight under the FMAs of the one before.  What that can get wrong, and the stage tests only catch by accident:
  unit     one density element per fragment, E_ab + E_ba, (a, b) over the edges of the groups of eight and of the rows of
           16 lanes: a wrong lane or register moves exactly one slice of the tensor into K.
  partial  a dense density against a tensor with the pair rows (i, .) of ONE i per fragment, i + 1 no multiple of eight:
           the last group of a row is partial, and the density beyond i must count for nothing.
  outlive  screening that takes ONE row of a block for zero and keeps the other, the long or the short one, in the
           first, the middle and the last block: each row's exchange must stand on its own.
  float    the one-workgroup route at n = 48 (the benchmark's), bound by jk_bounds."""
from __future__ import annotations

import numpy as np

from tests import jk_stage_cases as jc

SIZES = (40, 48)
ROUTES = ("wg1", "default")
NFRAG = 64
EDGES = (0, 7, 8, 15, 16, 17, 31, 32, 39, 47)
PARTIAL_I = (0, 6, 8, 14, 16, 22, 40, 46)


def unit_pairs(n):
    """[NFRAG] (a, b), a >= b: every pair of edges below n once, then the list again from its start."""
    e = [v for v in EDGES if v < n]
    pairs = [(a, b) for a in e for b in e if a >= b]
    return [pairs[f % len(pairs)] for f in range(NFRAG)], len(pairs)


def unit_density(n, f):
    a, b = unit_pairs(n)[0][f]
    D = np.zeros((n, n))
    D[a, b] += 1.0
    D[b, a] += 1.0
    return D


def partial_rows(n):
    return [i for i in PARTIAL_I if i < n]


def partial_fragment(n, f):
    """(M, D, i): the exact fragment with every STORED pair row zeroed but the rows (i, j), j <= i, of one i."""
    M, D = jc.exact_fragment(n, f)
    i = partial_rows(n)[f % len(partial_rows(n))]
    k, _ = np.tril_indices(n)
    return jc.screened(M, k != i), D, i


# ---- screening that splits a block ----------------------------------------------------------------------------------
# Shells of one function (s) and three (p) only, so that the two rows of the first, the middle and the last block lie
# in different shell pairs (with the d shells of jk_stage_cases.SHELLS the two rows of the last block share one).
SPLIT_L = {40: [0] + [1] * 13, 48: [1] * 16}
SPLIT_KINDS = tuple((pos, row) for pos in ("first", "middle", "last") for row in ("long", "short"))


def split_shell_l(n):
    return np.array(SPLIT_L[n], dtype=np.int32)


def _ao2sh(n):
    l = split_shell_l(n)
    return np.repeat(np.arange(len(l)), 2 * l + 1)


def split_block(n, pos):
    nblk = (jc.npair(n) + 1) // 2
    return {"first": 0, "middle": nblk // 2, "last": nblk - 1}[pos]


def split_flags(n, f):
    """(ns, ns) symmetric shell-pair flags of fragment f: the shell pair of ONE row of one block, kind f % 6."""
    pos, row = SPLIT_KINDS[f % len(SPLIT_KINDS)]
    t = split_block(n, pos)
    r = jc.npair(n) - 1 - t if row == "long" else t
    i = jc.tri_row(r)
    j = r - i * (i + 1) // 2
    sh = _ao2sh(n)
    F = np.zeros((len(SPLIT_L[n]),) * 2, dtype=bool)
    F[sh[i], sh[j]] = F[sh[j], sh[i]] = True
    return F


def split_row_flags(n, f):
    sh = _ao2sh(n)
    k, l = np.tril_indices(n)
    return split_flags(n, f)[sh[k], sh[l]]


def split_q(n):
    return np.stack([np.where(split_flags(n, f), jc.Q_DEAD, jc.Q_LIVE) for f in range(NFRAG)])


def split_fragment(n, f):
    M, D = jc.exact_fragment(n, f)
    return jc.screened(M, split_row_flags(n, f)), D


# ---- cases ----------------------------------------------------------------------------------------------------------
KINDS = ("unit", "partial", "outlive")
FLOAT_CASE = jc.Case("wg1", 48, NFRAG, kind="float")


def fragment_inputs(kind, n, f):
    if kind == "unit":
        return jc.exact_fragment(n, f)[0], unit_density(n, f)
    if kind == "partial":
        return partial_fragment(n, f)[:2]
    if kind == "outlive":
        return split_fragment(n, f)
    raise ValueError(kind)


def case_tensor(kind, n, layout):
    tri, _, stride = layout
    assert tri
    T, D = np.empty((NFRAG, stride)), np.empty((NFRAG, n, n))
    for f in range(NFRAG):
        M, D[f] = fragment_inputs(kind, n, f)
        T[f] = jc.tri_pack(M)
    return T, D


def case_reference(kind, n):
    J, K = np.empty((NFRAG, n, n)), np.empty((NFRAG, n, n))
    for f in range(NFRAG):
        J[f], K[f] = jc.jk_reference(*fragment_inputs(kind, n, f))
    return J, K


def route_cases(route):
    """(tag, kind, n) of every exact case of a route; the float case runs on wg1 behind them."""
    return [("%s-n%d" % (kind, n), kind, n) for n in SIZES for kind in KINDS]
