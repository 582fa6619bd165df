#!/usr/bin/env python3
"""Measurement aid: what the polarizability entry costs on the benchmark-shaped evaluation, which J/K route of its CPHF
iterations is faster, and that the plain entry is untouched.

(H2O)64, RHF/cc-pVDZ, exact in-core ERIs, the benchmark's tolerances and screening: the 2080 MBE-2 fragments (64
monomers, 2016 dimers) in ONE call per evaluation.  One warm-up, then five runs; median / min / max of the wall time.

    python scripts/cphf_probe.py plain [--root DIR] [n_side]     mbe.run_mbe
    python scripts/cphf_probe.py polar [n_side]                  mbe.run_mbe_polarizability (tol 1e-8)

--root DIR imports the package from another checkout of this repository: the same script times the parent commit's
plain entry.  The J/K route of the CPHF iterations is a per-process switch: run `polar` once as it is (the three-density
stream) and once with MQC_HIP_CPHF_MULTI=0 (three launches of the single-density stream on the same square tensor).
With MQC_HIP_CPHF_TIMING=1 every iteration runs both routes between HIP events and the library prints, per chunk, the
time per launch of each, the bytes the three-density stream reads and its fraction of the 8 TB/s peak; those lines are
printed here as they come, and the wall times of such a run include the extra launches."""
import json
import os
import sys
import time

args = sys.argv[1:]
mode = args.pop(0) if args else "polar"
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "--root" in args:
    k = args.index("--root")
    root = os.path.abspath(args[k + 1])
    del args[k:k + 2]
sys.path.insert(0, root)

import numpy as np                                  # noqa: E402

from metalquicha_amd import mbe, methods            # noqa: E402


def main():
    side = int(args[0]) if args else 4
    system = mbe.water_cluster(side)
    terms = mbe.generate_mbe_term_list(system, 2)
    st = methods.ScfSettings(basis_set="cc-pvdz", guess="gwh", energy_tol=1e-10, density_tol=1e-8, schwarz_tol=1e-12)
    if mode == "plain":
        evaluate = lambda: mbe.run_mbe(system, st, level=2, terms=terms)
    else:
        evaluate = lambda: mbe.run_mbe_polarizability(system, st, level=2, terms=terms, cphf=methods.CphfSettings())
    run = evaluate()                                 # the warm-up: pools, topologies, the first launches
    if run.errors:
        raise SystemExit("a fragment failed: " + run.errors[0])
    times = []
    for _ in range(5):
        t0 = time.perf_counter()
        run = evaluate()
        times.append(time.perf_counter() - t0)
    out = {"mode": mode, "root": root, "fragments": len(terms), "multi": os.environ.get("MQC_HIP_CPHF_MULTI", "1") != "0",
           "timing_switch": os.environ.get("MQC_HIP_CPHF_TIMING", "0") == "1",
           "wall_ms": {"median": 1e3 * float(np.median(times)), "min": 1e3 * min(times), "max": 1e3 * max(times)},
           "mbe2_energy": mbe.compute_mbe(terms, run.energies)[0], "scf_iterations": int(np.sum(run.iterations))}
    if mode != "plain":
        out["cphf_iterations"] = {"total": int(np.sum(run.cphf_iterations)), "max": int(np.max(run.cphf_iterations))}
        out["alpha_iso"] = float(np.trace(run.polarizability)) / 3.0
        out["alpha"] = [[float(x) for x in row] for row in run.polarizability]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
