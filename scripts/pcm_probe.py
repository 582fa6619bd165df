#!/usr/bin/env python3
"""Measurement aid: what the C-PCM stage costs on the benchmark-shaped evaluation, and that the plain entry is untouched.

(H2O)64, RHF/cc-pVDZ, exact in-core ERIs, the benchmark's tolerances and screening: the 2080 MBE-2 fragments (64
monomers, 2016 dimers) in ONE call of the plain entry (run_hip_scf_groups) and in ONE call of the PCM entry
(run_hip_scf_pcm_groups: epsilon 78.39, 110 points, scale 1.2).  One warm-up of each, then five runs each, alternating;
median / min / max of the wall time per evaluation, and the line MQC_HIP_PCM_TIMING prints per topology group (set
here; the library writes it to stderr, which this script points at a temporary file for the length of a call): HIP-event
time of the setup (cavity matrix, factorisation, A, B = L^-1 A, b) and of the per-iteration kernel, with the bytes of
its two passes over the fragments' own rows of B.  The kernel's bytes over time is compared with the HBM peak
(8 TB/s) as jk_tri_kernel's is in DESIGN.md section 10 (0.41 of peak on its own bytes).

    python scripts/pcm_probe.py [--plain-only] [--root DIR] [n_side]

--root DIR imports the package from another checkout of this repository (one without the PCM entry measures the plain
entry alone, as --plain-only does): the same script times the parent commit and this tree in one session."""
import os
import sys
import tempfile
import time

os.environ.setdefault("MQC_HIP_PCM_TIMING", "1")
args = sys.argv[1:]
plain_only = "--plain-only" in args
if plain_only:
    args.remove("--plain-only")
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "--root" in args:
    k = args.index("--root")
    root = os.path.abspath(args[k + 1])
    del args[k:k + 2]
sys.path.insert(0, root)

import numpy as np                                  # noqa: E402

from metalquicha_amd import mbe, methods            # noqa: E402

HBM_PEAK = 8.0e12


def main():
    side = int(args[0]) if args else 4
    system = mbe.water_cluster(side)
    terms = mbe.generate_mbe_term_list(system, 2)
    groups, _ = mbe.build_fragment_groups(system, terms)
    st = methods.ScfSettings(basis_set="cc-pvdz", guess="gwh", energy_tol=1e-10, density_tol=1e-8, schwarz_tol=1e-12)
    with_pcm = not plain_only and hasattr(methods, "run_hip_scf_pcm_groups")
    spans = tempfile.TemporaryFile(mode="w+b")
    saved = os.dup(2)

    def timed(fn):
        sys.stderr.flush()
        spans.seek(0); spans.truncate()
        os.dup2(spans.fileno(), 2)
        t0 = time.perf_counter()
        try:
            out = fn()
        finally:
            dt = time.perf_counter() - t0
            os.dup2(saved, 2)
        spans.seek(0)
        lines = [ln for ln in spans.read().decode(errors="replace").splitlines() if ln.startswith("mqc_hip: pcm timing:")]
        return out, dt, lines

    def plain():
        rec = methods.run_hip_scf_groups(st, groups)
        assert not any(np.any(r["has_error"]) for r in rec)
        return rec

    def pcm():
        rec, e_pcm, nt = methods.run_hip_scf_pcm_groups(st, methods.PcmSettings(78.39, 110, 1.2), groups)
        assert not any(np.any(r["has_error"]) for r in rec)
        return rec, e_pcm, nt

    runs = [plain] + ([pcm] if with_pcm else [])
    for fn in runs:                                 # warm-up: pools, topology cache, code objects
        timed(fn)
    t_plain, t_pcm, setup, iters, gbs, launches = [], [], [], [], [], []
    last = None
    for _ in range(5):
        rec, dt, _ = timed(plain)
        t_plain.append(dt)
        if not with_pcm:
            continue
        last, dt2, lines = timed(pcm)
        t_pcm.append(dt2)
        s = i = b = 0.0
        n = 0
        for ln in lines:
            f = ln.replace(",", " ").split()
            s += float(f[f.index("setup") + 1]); i += float(f[f.index("iterations") + 1])
            n += int(f[f.index("launches") - 1]); b += float(f[f.index("GB") - 1])
        setup.append(s); iters.append(i); gbs.append(b); launches.append(n)
    os.close(saved)

    def mmm(v):
        return "median %.2f min %.2f max %.2f" % (float(np.median(v)), min(v), max(v))
    its = int(sum(int(np.sum(r["iterations"])) for r in rec))
    print("tree %s" % root)
    print("(H2O)%d MBE-2, %d fragments, RHF/cc-pVDZ, %d SCF iterations in all" % (system.n_monomers, len(terms), its))
    print("plain entry  ms per evaluation: " + mmm([1e3 * t for t in t_plain]))
    if not with_pcm:
        return
    rec2, e_pcm, nt = last
    print("PCM entry    ms per evaluation: " + mmm([1e3 * t for t in t_pcm]))
    print("difference   ms per evaluation: " + mmm([1e3 * (b - a) for a, b in zip(t_plain, t_pcm)]))
    print("tesserae per fragment: %s; sum of E_pcm %.6f Eh; %d SCF iterations in all"
          % (", ".join("%d-%d" % (int(t.min()), int(t.max())) for t in nt), float(sum(np.sum(e) for e in e_pcm)),
             int(sum(int(np.sum(r["iterations"])) for r in rec2))))
    print("MQC_HIP_PCM_TIMING, both groups of an evaluation, ms: setup %s | per-iteration kernel, all launches %s (%d launches)"
          % (mmm(setup), mmm(iters), int(np.median(launches))))
    ms, gb = float(np.median(iters)), float(np.median(gbs))
    if ms > 0:
        rate = gb * 1e9 / (ms * 1e-3)
        print("per-iteration kernel: %.2f GB of B in %.2f ms = %.2f TB/s = %.2f of HBM peak (jk_tri_kernel: 0.41 on its own bytes)"
              % (gb, ms, rate * 1e-12, rate / HBM_PEAK))


if __name__ == "__main__":
    main()
