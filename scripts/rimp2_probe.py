#!/usr/bin/env python3
"""Measurement aid: what the RI-MP2 stage adds to a density-fitted MBE-2 evaluation of the benchmark cluster.

(H2O)64, cc-pVDZ, mqc-even-tempered-jkfit: the 2080 MBE-2 fragments (64 monomers, 2016 dimers) as DF-RHF through
mbe.run_mbe and through mbe.run_mbe_rimp2 (frozen core), the benchmark's tolerances and screening.  One warm-up of
each, then five runs each, alternating; median / min / max of the wall time per evaluation, their difference, and the
spans MQC_HIP_MP2_TIMING prints per chunk (set here; the library writes them to stderr, which this script points at a
temporary file for the length of a call and sums per evaluation).  The FP64 matrix-core rate is the stage's operation
count over its span: per fragment 2 naux (n^2 no + n no nv) for the transform and 2 naux nv^2 no (no + 1) for the
pair contraction (both accumulators of every pair i >= j).
    python scripts/rimp2_probe.py [n_side]"""
import os
import sys
import tempfile
import time

os.environ.setdefault("MQC_HIP_MP2_TIMING", "1")
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np                                  # noqa: E402

from metalquicha_amd import mbe, methods            # noqa: E402


def main():
    side = int(sys.argv[1]) if len(sys.argv) > 1 else 4
    system = mbe.water_cluster(side)
    terms = mbe.generate_mbe_term_list(system, 2)
    st = methods.ScfSettings(basis_set="cc-pvdz", guess="gwh", energy_tol=1e-10, density_tol=1e-8, density_fitting=True,
                             aux_basis_set="mqc-even-tempered-jkfit", schwarz_tol=1e-12)
    # the library's timing lines go to file descriptor 2: point it at a file for the length of a call
    spans = tempfile.TemporaryFile(mode="w+b")
    saved = os.dup(2)

    def timed(fn):
        sys.stderr.flush()
        spans.seek(0); spans.truncate()
        os.dup2(spans.fileno(), 2)
        t0 = time.perf_counter()
        try:
            run = fn()
        finally:
            dt = time.perf_counter() - t0
            os.dup2(saved, 2)
        spans.seek(0)
        lines = [ln for ln in spans.read().decode(errors="replace").splitlines() if ln.startswith("mqc_hip rimp2:")]
        return run, dt, lines

    def scf():
        return mbe.run_mbe(system, st, level=2, terms=terms)

    def mp2():
        return mbe.run_mbe_rimp2(system, st, level=2, terms=terms)

    for fn in (scf, mp2):                           # warm-up: pools, topology cache, code objects
        run, _, _ = timed(fn)
        assert not run.errors, run.errors[:3]
    t_scf, t_mp2, stage, transform, pairs = [], [], [], [], []
    last = None
    for _ in range(5):
        run, dt, _ = timed(scf)
        t_scf.append(dt)
        run2, dt2, lines = timed(mp2)
        t_mp2.append(dt2)
        last = (run, run2)
        tot = tr = pr = 0.0
        for ln in lines:
            f = ln.replace(",", " ").split()
            tot += float(f[f.index("total") + 1]); tr += float(f[f.index("transform") + 1]); pr += float(f[f.index("pairs") + 1])
        stage.append(tot); transform.append(tr); pairs.append(pr)
    os.close(saved)

    def mmm(v):
        return "median %.2f min %.2f max %.2f" % (float(np.median(v)), min(v), max(v))
    run, run2 = last
    e_scf, _, _ = mbe.compute_mbe(terms, run.energies)
    e_mp2, _, _ = mbe.compute_mbe(terms, run2.energies)
    print("(H2O)%d MBE-2, %d fragments, DF-RHF/cc-pVDZ: E(SCF) = %.8f  E(RI-MP2) = %.8f  E_corr = %.8f"
          % (system.n_monomers, len(terms), e_scf, e_mp2, e_mp2 - e_scf))
    print("run_mbe        ms per evaluation: " + mmm([1e3 * t for t in t_scf]))
    print("run_mbe_rimp2  ms per evaluation: " + mmm([1e3 * t for t in t_mp2]))
    print("difference     ms per evaluation: " + mmm([1e3 * (b - a) for a, b in zip(t_scf, t_mp2)]))
    print("MQC_HIP_MP2_TIMING, all chunks of an evaluation, ms: stage %s | transform %s | pairs %s" % (mmm(stage), mmm(transform), mmm(pairs)))
    # operation counts of the dimers and monomers of this cluster (n, nocc, frozen, naux per water: 24, 5, 1, 126)
    flop_t = flop_p = 0.0
    for t in terms:
        k = len(t)
        n, no, nv, na = 24 * k, 4 * k, 19 * k, 126 * k
        flop_t += 2.0 * na * (n * n * no + n * no * nv)
        flop_p += 2.0 * na * nv * nv * no * (no + 1)
    ms_t, ms_p = float(np.median(transform)), float(np.median(pairs))
    if ms_t > 0 and ms_p > 0:
        print("FP64 matrix-core rate: transform %.1f Gflop in %.2f ms = %.2f Tflop/s; pairs %.1f Gflop in %.2f ms = %.2f Tflop/s"
              % (flop_t * 1e-9, ms_t, flop_t / ms_t * 1e-9, flop_p * 1e-9, ms_p, flop_p / ms_p * 1e-9))


if __name__ == "__main__":
    main()
