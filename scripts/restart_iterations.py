"""SCF iterations with and without restart: prints scf_iterations_total (mqc_hip_get_stats) of
  1. FMO2, density-fitted B3LYP, (H2O)8 / cc-pVDZ (tests/workload_cases.py, fmo_df_rks_*): fmo.run_fmo2(restart=...)
  2. MBE-2 RHF/cc-pVDZ on the benchmark's (H2O)64 cluster (64 monomers + 2016 dimers, GWH, 1e-10 / 1e-8): mbe.run_mbe(restart=...)
once from the settings' guess and once restarted, with the energy difference.  Counts, not times.
    python scripts/restart_iterations.py [--side 4]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from metalquicha_amd import fmo, mbe, methods      # noqa: E402
from tests import workload_cases as wc             # noqa: E402


def counted(run):
    methods.get_stats()                            # reading resets the counters
    out = run()
    return out, int(methods.get_stats().scf_iterations_total)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=4, help="the MBE cluster is (H2O)_{side^3}")
    args = ap.parse_args()
    system, st = wc.fmo_df_rks_system(), wc.fmo_df_rks_settings()
    plain, n0 = counted(lambda: fmo.run_fmo2(system, st, expansion="fmo"))
    again, n1 = counted(lambda: fmo.run_fmo2(system, st, expansion="fmo", restart=True))
    print("FMO2 DF-B3LYP (H2O)8/cc-pVDZ: scf_iterations_total %d from GWH, %d restarted; %d outer passes both; dE = %.2e"
          % (n0, n1, again.outer_iterations, again.energy - plain.energy), flush=True)
    cluster = mbe.water_cluster(args.side)
    sm = methods.ScfSettings(basis_set="cc-pvdz", guess="gwh", energy_tol=1e-10, density_tol=1e-8)
    plain, n0 = counted(lambda: mbe.run_mbe(cluster, sm, level=2))
    again, n1 = counted(lambda: mbe.run_mbe(cluster, sm, level=2, restart=True))
    de = mbe.compute_mbe(again.terms, again.energies)[0] - mbe.compute_mbe(plain.terms, plain.energies)[0]
    print("MBE-2 RHF/cc-pVDZ (H2O)%d, %d SCFs: scf_iterations_total %d from GWH, %d restarted; dE = %.2e; errors %d/%d"
          % (cluster.n_monomers, len(plain.terms), n0, n1, de, len(plain.errors), len(again.errors)), flush=True)


if __name__ == "__main__":
    main()
