"""A/B of the two consumers of the Hermite-record stage (kern_esp.hip, kern_grad_pc.hip) between two builds of the library.
One invocation runs the cases with the library MQC_HIP_LIBRARY selects and writes every output as .npy; a second compares.

    MQC_HIP_LIBRARY=<lib> python scripts/hermite_records_ab.py write DIR
    python scripts/hermite_records_ab.py compare TREE_DIR PARENT_DIR [PARENT_DIR_2 PARENT_DIR_3 ...]
    MQC_HIP_LIBRARY=<lib> python scripts/hermite_records_ab.py time-esp

Cases: one and three water molecules (different geometries) in 6-31G, cc-pVDZ and def2-TZVP (s/p, d and f pairs) with
synthetic densities.  run_hip_esp at 300 points per fragment (two tiles of 256, the second partial) and, for the three
fragments, at ragged counts (300, 1, 257); run_hip_embedded_gradients in 3 and in 65 charges (one wave tile and two).
compare requires np.array_equal for every potential, every site gradient and the atom gradients of the 3-charge cases
(one tile per fragment: the atomic adds are ordered by the stream).  In 65 charges two tiles race on atomicAdd: the first
directory's largest difference from the second must not exceed the largest difference among the further directories and
the second (runs of one build); both figures are printed.  Exit status 1 when a requirement fails.

As measured when the record stage became shared (profiles/r09_a_hermite_records_parent_vs_tree.log): the nine potentials are
bitwise equal; the gradient requirements are NOT met, by the tree or by the parent build against itself, because the SCF
in front of the gradient stage does not reproduce its density bit for bit from run to run -- site gradients differ by up to
1.8e-15 (parent run to run 2.2e-15), 3-charge atom gradients by 2.1e-14 (parent 3.2e-14), 65-charge atom gradients by
2.9e-14 (parent 4.3e-14).  The requirements stay as they are; for each array that misses, the parent's own figure is printed.

time-esp: wall time of the second run_hip_esp call on the 2016 cc-pVDZ dimers of scripts/embedded_gradient_probe.py with
1000 points each."""
import itertools
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np                                                # noqa: E402

from metalquicha_amd import basis as basis_mod, mbe, methods     # noqa: E402
from metalquicha_amd.methods import FragmentGroup, ScfSettings   # noqa: E402
from tests.helpers import synthetic_density, water_at            # noqa: E402

BASES = ("6-31g", "cc-pvdz", "def2-tzvp")
Z = np.array([8, 1, 1], dtype=np.int32)


def waters(m):
    rng = np.random.default_rng(20261020)
    return np.stack([water_at(rng, c) for c in ([0.0, 0.0, 0.0], [0.4, -0.3, 0.2], [-0.2, 0.5, 0.1])[:m]])


def around(rng, xyz, count):
    """count points 2.5 to 9 Bohr from the fragment's centre, none within 1.5 Bohr of an atom."""
    out = []
    while len(out) < count:
        d = rng.normal(size=3)
        p = xyz.mean(axis=0) + d / np.linalg.norm(d) * rng.uniform(2.5, 9.0)
        if np.min(np.linalg.norm(xyz - p, axis=1)) > 1.5:
            out.append(p)
    return np.array(out)


def write(out_dir):
    os.makedirs(out_dir, exist_ok=True)
    for basis, m in itertools.product(BASES, (1, 3)):
        tag = "%s_m%d" % (basis, m)
        xyz = waters(m)
        rng = np.random.default_rng(7 + m)
        nao = basis_mod.build_flat_basis(basis, Z).nao
        D = np.stack([synthetic_density(nao) * (1.0 + 0.1 * f) for f in range(m)])
        group = FragmentGroup(Z, xyz, np.zeros(m, dtype=np.int32))
        st = ScfSettings(basis_set=basis, energy_tol=1e-10, density_tol=1e-8, guess="gwh")
        pts = np.stack([around(rng, xyz[f], 300) for f in range(m)])
        np.save(os.path.join(out_dir, "esp_%s_full.npy" % tag), methods.run_hip_esp(st, group, D, pts))
        if m == 3:
            np.save(os.path.join(out_dir, "esp_%s_ragged.npy" % tag), methods.run_hip_esp(st, group, D, pts, n_points=[300, 1, 257]))
        for npc in (3, 65):
            group.point_charge_xyz = np.stack([around(rng, xyz[f], npc) for f in range(m)])
            group.point_charges = np.stack([rng.uniform(0.2, 0.8, size=npc) * rng.choice([-1.0, 1.0], size=npc) for f in range(m)])
            rec, atom, site = methods.run_hip_embedded_gradients(st, [group])
            if rec[0]["has_error"].any():
                raise SystemExit("%s in %d charges: %s" % (tag, npc, rec[0]["message"]))
            np.save(os.path.join(out_dir, "site%d_%s.npy" % (npc, tag)), site[0])
            np.save(os.path.join(out_dir, "atom%d_%s.npy" % (npc, tag)), atom[0])
        print("wrote", tag, flush=True)


def compare(dirs):
    tree, parent, repeats = dirs[0], dirs[1], dirs[2:]
    names = sorted(os.listdir(parent))
    if names != sorted(os.listdir(tree)) or len(names) != 6 * 5 + 3:
        raise SystemExit("the directories do not hold the same %d arrays" % (6 * 5 + 3))
    ok, racing_tree, racing_parent = True, 0.0, 0.0
    for name in names:
        a, b = np.load(os.path.join(tree, name)), np.load(os.path.join(parent, name))
        if not np.all(np.isfinite(b)) or not np.any(b != 0.0):
            ok = False
            print("%-36s EMPTY OR NOT FINITE" % name)
        if name.startswith("atom65_"):
            d_tree = float(np.max(np.abs(a - b)))
            d_parent = max([float(np.max(np.abs(np.load(os.path.join(r, name)) - b))) for r in repeats], default=0.0)
            racing_tree, racing_parent = max(racing_tree, d_tree), max(racing_parent, d_parent)
            print("%-36s racing atomicAdd: tree - parent %.3e, parent run to run %.3e" % (name, d_tree, d_parent))
        else:
            same = a.shape == b.shape and np.array_equal(a, b)
            ok = ok and same
            own = max([float(np.max(np.abs(np.load(os.path.join(r, name)) - b))) for r in repeats], default=0.0)
            print("%-36s %s" % (name, "bitwise equal" if same else "DIFFERS by %.3e (parent run to run %.3e)" % (float(np.max(np.abs(a - b))), own)))
    print("65-charge atom gradients: largest tree - parent %.3e, largest parent run to run %.3e (%d further runs)"
          % (racing_tree, racing_parent, len(repeats)))
    if racing_tree > racing_parent:
        ok = False
    print("PASS" if ok else "FAIL")
    return 0 if ok else 1


def time_esp():
    system = mbe.water_cluster(4)
    z = np.asarray(system.element_numbers, dtype=np.int32)
    xyz = np.ascontiguousarray(system.coordinates.T)
    atoms = [np.concatenate([system.monomers[i], system.monomers[j]]) for i, j in itertools.combinations(range(system.n_monomers), 2)]
    group = FragmentGroup(z[atoms[0]], np.stack([xyz[a] for a in atoms]), np.zeros(len(atoms), dtype=np.int32))
    st = ScfSettings(basis_set="cc-pvdz")
    rng = np.random.default_rng(1)
    pts = group.xyz.mean(axis=1)[:, None, :] + rng.uniform(-9.0, 9.0, size=(len(atoms), 1000, 3))
    D = np.broadcast_to(synthetic_density(48), (len(atoms), 48, 48)).copy()
    for rep in range(2):
        t = time.time()
        v = methods.run_hip_esp(st, group, D, pts, include_nuclei=False)
        print("esp: %d dimers, 1000 points each, call %d: %.4f s, checksum %.12e" % (len(atoms), rep + 1, time.time() - t, float(v.sum())), flush=True)


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "write":
        write(sys.argv[2])
    elif len(sys.argv) >= 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2:]))
    elif len(sys.argv) == 2 and sys.argv[1] == "time-esp":
        time_esp()
    else:
        raise SystemExit(__doc__)
