"""Host test of the PCM cavity builder (metalquicha_amd/csrc/pcm_cavity.hpp): tests/host/check_pcm_cavity.cpp is compiled
for the host with the address and undefined-behaviour sanitizers, as a stand-alone program, and run.  The program checks
counts and areas against closed forms (one sphere; two equal spheres at distance d), ghosts, the tessera cap and the
radius overrides; its `dump` mode prints a cavity, which is compared with the numpy reference (tests/pcm_reference.py).
No GPU: the header has no HIP in it."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import pcm_reference as pr
from tests.helpers import water_at

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "check_pcm_cavity.cpp")
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def compilers():
    """g++ or clang++ with the sanitizer runtimes linked into the program itself (it must not depend on what the
    environment preloads)."""
    found = []
    if shutil.which("g++"):
        found.append(["g++", "-static-libasan", "-static-libubsan"])
    for clang in (shutil.which("clang++"), "/opt/rocm/lib/llvm/bin/clang++"):
        if clang and os.path.isfile(clang):
            found.append([clang, "-static-libsan"])
            break
    return found


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("pcm_cavity") / "check_pcm_cavity")
    errors = []
    for cxx in compilers():
        r = subprocess.run(cxx + ["-std=c++17", "-O1", "-g"] + SANITIZE + [SRC, "-o", out], capture_output=True, text=True, timeout=300)
        if r.returncode == 0:
            return out
        errors.append("%s: %s" % (cxx[0], r.stderr[-2000:]))
    raise AssertionError("no host compiler built the sanitized check program:\n" + "\n".join(errors))


def test_header_has_no_hip():
    text = open(os.path.join(ROOT, "metalquicha_amd", "csrc", "pcm_cavity.hpp")).read()
    code = "\n".join(line.split("//")[0] for line in text.splitlines())
    assert "hip" not in code.lower() and "__global__" not in code and "__device__" not in code


def test_closed_forms_ghosts_cap_and_radii(program):
    r = subprocess.run([program], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    print(r.stderr)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "ok"
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr
    assert all(any(l.startswith("(%s)" % k) for l in lines) for k in "abcde")


def dimer():
    rng = np.random.default_rng(11)
    return [8, 1, 1, 8, 1, 1], np.concatenate([water_at(rng, [0.0, 0.0, 0.0]), water_at(rng, [5.2, 0.4, -0.3])])


@pytest.mark.parametrize("pts,ghost", [(110, None), (50, None), (194, [0, 0, 0, 1, 1, 1]), (302, None)])
def test_cavity_equals_the_numpy_reference(program, pts, ghost):
    numbers, xyz = dimer()
    args = [program, "dump", str(pts), "1.2"]
    for k, (z, x) in enumerate(zip(numbers, xyz)):
        args += [str(z), str(0 if ghost is None else ghost[k])] + [repr(float(c)) for c in x]
    r = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr
    rows = r.stdout.strip().splitlines()
    got = np.array([[float(v) for v in row.split()] for row in rows[1:]])
    t, a, owner = pr.cavity(numbers, xyz, pts, ghost=ghost)
    assert int(rows[0]) == len(a) == len(got)
    assert np.array_equal(got[:, 0].astype(int), owner)
    # same tables, same formulas: the difference is the rounding of s = R + rho u and a = 4 pi rho^2 w (a few ulp of ~10)
    assert np.max(np.abs(got[:, 1:4] - t)) < 1e-13
    assert np.max(np.abs(got[:, 4] - a)) < 1e-13
