"""Child process of tests/test_gpu_rimp2_stage.py: MQC_HIP_MP2_C_LDS is a function-static read once per process, so every
route runs its cases in a process of its own: `python -m tests.rimp2_stage_child ROUTE OUT.npz`, with the route's
environment set by the parent.  Per run it writes e ("E:"), the pair partials ("P:"), Bia with its padding ("B:") and the
route record ("R:", in the order of stages.RIMP2_ROUTE_FIELDS) to OUT.npz, and prints one JSON line.

The default route also runs, in this order: the second case of the stale-pool pair as the FIRST call of the process
("fresh"), every case, the capped runs (several rows per wave) next to their uncapped twins, the 300-fragment batch,
the ragged batch with its fragments one at a time, and the stale-pool pair.
Test infrastructure."""
import json
import sys

import numpy as np

from tests import rimp2_stage_cases as rs, stages


def main(route, out):
    res, done = {}, []

    def run(label, c, B, C, eps, **kw):
        e, part, bia, rt = stages.rimp2_stage(B, C, eps, c.nocc, c.nfz, **kw)
        res["E:" + label], res["P:" + label], res["B:" + label] = e, part, bia
        res["R:" + label] = np.array([rt[k] for k in stages.RIMP2_ROUTE_FIELDS], dtype=np.int64)
        done.append(label)

    if route == "default":
        c = rs.BY_KEY[rs.STALE[1]]
        for fam in rs.FAMILIES:
            run("fresh/%s" % fam, c, *rs.inputs(c, fam))
    for c in rs.route_cases(route):
        for fam in rs.FAMILIES:
            run("%s/%s" % (c.name, fam), c, *rs.inputs(c, fam))
    if route == "default":
        for key in rs.ROWS_SHAPES:
            c = rs.BY_KEY[key]
            for fam in rs.FAMILIES:
                inp = rs.inputs(c, fam, rs.ROWS_M)
                for cap in (0,) + rs.ROWS_CAPS:
                    run("rows/%s/%s/cap%d" % (c.name, fam, cap), c, *inp, workgroups_per_fragment=cap)
        c = rs.BY_KEY[rs.TILED]
        for fam in rs.FAMILIES:
            run("tiled/%s" % fam, c, *rs.tiled_inputs(c, fam))
        c = rs.BY_KEY[rs.RAGGED]
        for fam in rs.FAMILIES:
            B, C, eps = rs.ragged_inputs(c, fam)
            run("ragged/%s" % fam, c, B, C, eps, nmo=rs.RAGGED_NMO, runs=rs.RAGGED_RUNS)
            for f in range(len(rs.RAGGED_NMO)):
                run("ragged/%s/%d" % (fam, f), c, B[f:f + 1], C[f:f + 1], eps[f:f + 1], nmo=rs.RAGGED_NMO[f:f + 1], runs=rs.RAGGED_RUNS[f:f + 1])
        first, second = rs.BY_KEY[rs.STALE[0]], rs.BY_KEY[rs.STALE[1]]
        for fam in rs.FAMILIES:
            run("stale-first/%s" % fam, first, *rs.inputs(first, fam))
            run("stale/%s" % fam, second, *rs.inputs(second, fam))
    np.savez(out, **res)
    print(json.dumps({"route": route, "runs": done, "file": out}))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
