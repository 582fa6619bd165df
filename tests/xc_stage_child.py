"""Child process of tests/test_gpu_xc_stage.py: the quadrature switches (MQC_HIP_XC_*) are read once per process, so
every route runs its cases in a process of its own: `python -m tests.xc_stage_child ROUTE OUT.npz`, with the route's
environment set by the parent.  Writes E_xc, N_e and V_xc of every case of the route to OUT.npz and prints one JSON line.
Test infrastructure."""
import json
import sys

import numpy as np

from oracle import scf_oracle as so
from tests import stages, xc_stage_cases as xs
from tests.helpers import oracle_mol


def main(route, out):
    res, done = {}, []
    for case in xs.route_cases(route):
        frag = xs.fragment(case)
        mol = oracle_mol(case.basis, frag)
        S, _, _ = so.int1e(mol)
        D, _ = xs.density(case, frag, S, mol)
        e, nel, V = stages.xc_batch(case.basis, [frag], case.functional, D[None], case.level, case.unrestricted)
        res["E:" + case.name], res["N:" + case.name], res["V:" + case.name] = e[0], nel[0], V[0]
        done.append(case.name)
    np.savez(out, **res)
    print(json.dumps({"route": route, "cases": done, "file": out}))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
