"""Child process of tests/test_gpu_jk_broadcast.py, as tests/jk_stage_child.py is of the stage tests (the switches of
the J/K stream are read once per process): `python -m tests.jk_broadcast_child ROUTE OUT.npz` runs every case of
tests/jk_broadcast_cases.py on the route through mqc_hip_jk_incore_batch, writes J, K, the read counters and the
instance with its grid to OUT.npz and prints one JSON line.  Test infrastructure."""
import json
import sys

import numpy as np

from tests import jk_broadcast_cases as bc, jk_stage_cases as jc, jk_stage_child, stages


def main(route, out):
    res, done = {}, []
    for tag, kind, n in bc.route_cases(route):
        layout = stages.jk_tensor_layout(n, bc.NFRAG)
        T, D = bc.case_tensor(kind, n, layout)
        kw = dict(shell_l=bc.split_shell_l(n), Q=bc.split_q(n), q_thresh=jc.Q_THRESH) if kind == "outlive" else {}
        J, K, loaded, inst, gx = stages.jk_incore_batch(T, D, **kw)
        res["J:" + tag], res["K:" + tag], res["L:" + tag] = J, K, loaded
        res["I:" + tag], res["G:" + tag] = np.array(inst), np.array(gx)
        done.append(tag)
    if route == bc.FLOAT_CASE.route:
        jk_stage_child.run_case(bc.FLOAT_CASE, res)
        done.append(bc.FLOAT_CASE.name)
    np.savez(out, **res)
    print(json.dumps({"route": route, "cases": done, "file": out}))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
