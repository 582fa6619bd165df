"""Child process of tests/test_gpu_jk_stage.py: the switches of the in-core J/K stream (MQC_HIP_ERI_TRI,
MQC_HIP_JK_TRI_WG, MQC_HIP_JK_ROWCOOP) are function-statics read once per process, so every route runs its cases in a
process of its own: `python -m tests.jk_stage_child ROUTE OUT.npz`, with the route's environment set by the parent.
Writes J, K, the read counters, the reported instance with its grid and the layout the engine asked for of every case
(cases with finished fragments: one set per run), and on the default route the tie to the single-fragment entries, to
OUT.npz, and prints one JSON line.  Test infrastructure."""
import json
import sys

import numpy as np

from tests import jk_stage_cases as jc, stages


def run_case(c, res):
    layout = stages.jk_tensor_layout(c.n, c.nfrag, c.uhf)
    T, D = jc.case_tensor(c, layout)
    kw = {}
    if c.pattern:
        kw = dict(shell_l=jc.shell_l(c.n), Q=jc.case_q(c), q_thresh=jc.Q_THRESH)
    for k, done in enumerate(c.done or (None,)):
        flags = None
        if done is not None:
            flags = np.zeros(c.nfrag, dtype=np.int32)
            flags[list(done)] = 1 + k            # any non-zero value marks a finished fragment
        J, K, loaded, inst, gx = stages.jk_incore_batch(T, D, unrestricted=c.uhf, done=flags, **kw)
        tag = "%s%s" % (c.name, ":%d" % k if c.done else "")
        res["J:" + tag], res["K:" + tag], res["L:" + tag] = J, K, loaded
        res["I:" + tag], res["G:" + tag], res["Y:" + tag] = np.array(inst), np.array(gx), np.array(layout, dtype=np.int64)


def run_tie(res):
    """The engine's own tensor of a water dimer (n = 48, the single-fragment entry), repeated as 64 fragments with 64
    different exact densities, through the batch entry."""
    from tests.helpers import fragment_bohr, water_at
    rng = np.random.default_rng(12)
    frag = fragment_bohr([8, 1, 1] * 2, np.vstack([water_at(rng, c) for c in ([0, 0, 0], [5.4, 0.4, -0.3])]))
    M = stages.eri_packed("cc-pvdz", frag)
    assert M.shape == (jc.npair(jc.TIE_N),) * 2
    layout = stages.jk_tensor_layout(jc.TIE_N, jc.TIE_NFRAG)
    one = jc.tri_pack(M) if layout[0] else M.reshape(-1)        # the triangle: the elements col <= row as they are
    D = jc.tie_densities(jc.TIE_N, jc.TIE_NFRAG)
    J, K, loaded, inst, gx = stages.jk_incore_batch(np.tile(one, (jc.TIE_NFRAG, 1)), D)
    res["M:tie"], res["S:tie"] = M, np.array(float(np.max(np.abs(M - M.T))))
    res["J:tie"], res["K:tie"], res["I:tie"], res["G:tie"] = J, K, np.array(inst), np.array(gx)


def main(route, out):
    res, done = {}, []
    for c in jc.route_cases(route):
        run_case(c, res)
        done.append(c.name)
    if route == "default":
        run_tie(res)
    np.savez(out, **res)
    print(json.dumps({"route": route, "cases": done, "file": out}))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
