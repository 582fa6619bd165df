"""Times the gradient stage of the EE-MBE pair phase on the bench's cluster: (H2O)64 RHF/cc-pVDZ, 2016 dimers, each in the
186 fixed charges (O -0.8, H +0.4) of the other 62 molecules, through mqc_hip_scf_gradient_embedded_batch.
MQC_HIP_GRAD_TIMING=1 is set here: per chunk the library prints the span of the plain gradient stage ("total ... ms")
and of the point charges' part ("point charges ...: total ... ms, records ..., charges ...") on stderr.
    python scripts/embedded_gradient_probe.py [n_side] [plain]     -- "plain": the same dimers without charges through
                                                                      mqc_hip_scf_run_batch (the yardstick)"""
import itertools
import os
import sys
import time

os.environ.setdefault("MQC_HIP_GRAD_TIMING", "1")
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np                                  # noqa: E402

from metalquicha_amd import mbe, methods            # noqa: E402
from metalquicha_amd.methods import FragmentGroup, ScfSettings   # noqa: E402

n_side = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 4
plain = "plain" in sys.argv[1:]
system = mbe.water_cluster(n_side)
st = ScfSettings(basis_set="cc-pvdz", energy_tol=1e-9, density_tol=1e-7, guess="gwh")
z = np.asarray(system.element_numbers, dtype=np.int32)
xyz = np.ascontiguousarray(system.coordinates.T)
q_all = np.where(z == 8, -0.8, 0.4)
pairs = list(itertools.combinations(range(system.n_monomers), 2))
atoms = [np.concatenate([system.monomers[i], system.monomers[j]]) for i, j in pairs]
group = FragmentGroup(z[atoms[0]], np.stack([xyz[a] for a in atoms]), np.zeros(len(pairs), dtype=np.int32))
if not plain:
    outside = [np.setdiff1d(np.arange(len(z)), a) for a in atoms]
    group.point_charge_xyz = np.stack([xyz[o] for o in outside])
    group.point_charges = np.stack([q_all[o] for o in outside])
for rep in range(2):
    t = time.time()
    if plain:
        grads = []
        rec = methods.run_hip_scf_groups(st, [group], want_gradient=True, gradients_out=grads)[0]
        worst = float(np.max(np.abs(grads[0].sum(axis=1))))
    else:
        recs, atom, site = methods.run_hip_embedded_gradients(st, [group])
        rec = recs[0]
        worst = float(np.max(np.abs(atom[0].sum(axis=1) + site[0].sum(axis=1))))
    dt = time.time() - t
    print("%s: %d dimers, %d charges each, %.3f s, errors %d, largest |sum of a fragment's gradient| %.2e" %
          ("plain" if plain else "embedded", len(pairs), 0 if plain else group.point_charges.shape[1], dt,
           int(np.sum(rec["has_error"])), worst), flush=True)
