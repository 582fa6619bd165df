"""Child process of tests/test_gpu_df_stage.py: the density-fitting switches (MQC_HIP_DF_*) are function-statics read
once per process, so every route runs its cases in a process of its own: `python -m tests.df_stage_child ROUTE OUT.npz`,
with the route's environment (and MQC_BASIS_PATH, for the probe basis sets) set by the parent.  Writes J, K and the
reported instance of every J/K case, A3, the metric, B and the flags of every fit case, and on the default route the
end-to-end tie (the engine's own fitted B through the J/K stage) to OUT.npz, and prints one JSON line.
Test infrastructure."""
import json
import sys

import numpy as np

from tests import df_stage_cases as ds, stages


def main(route, out):
    res, done = {}, []
    for c in ds.route_jk_cases(route):
        B, D, C = ds.jk_inputs(c)
        J, K, inst = stages.df_jk_batch(B, D, C, c.nocc, c.exx)
        res["J:" + c.name], res["K:" + c.name], res["I:" + c.name] = J, K, np.array(inst)
        done.append(c.name)
    for c in ds.route_fit_cases(route):
        A3, M, B, flag = stages.df_fit_batch(c.basis, c.aux, ds.fit_fragments(c))
        res["A3:" + c.name], res["M:" + c.name], res["B:" + c.name], res["F:" + c.name] = A3, M, B, flag
        done.append(c.name)
        if route == "default" and c.name == ds.TIE_CASE:
            n = int((np.sqrt(8 * B.shape[2] + 1) - 1) / 2)
            D, C = ds.tie_inputs(n)
            J, K, inst = stages.df_jk_batch(B, D[None], C[None], ds.TIE_NOCC, 1.0)
            res["J:tie"], res["K:tie"], res["I:tie"] = J[0], K[0], np.array(inst)
    np.savez(out, **res)
    print(json.dumps({"route": route, "cases": done, "file": out}))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
