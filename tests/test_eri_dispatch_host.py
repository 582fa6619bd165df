"""Host test of the integral stage's placement rule (metalquicha_amd/csrc/eri_dispatch.hpp): tests/host/check_eri_dispatch.cpp
is compiled for the host with the address and undefined-behaviour sanitizers, as a stand-alone program, and run.  The
program checks (a) the rule's properties over every small state, (b) that a discrete-event replay of the 23 recorded dense
launches of the (H2O)64 dimer batch through the rule ends within 6 % of the lower bound (sum + 8.57 + 17.96) / 4 = 24.53 ms at
depth 1 and 2 while the recorded static placement (29.24 ms) does not, and (c) that every launch is issued exactly once.
No GPU: the header has no HIP in it."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "check_eri_dispatch.cpp")
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
    out = str(tmp_path_factory.mktemp("eri_dispatch") / "check_eri_dispatch")
    errors = []
    for cxx in compilers():
        r = subprocess.run(cxx + ["-std=c++17", "-O1", "-g"] + SANITIZE + [SRC, "-o", out], capture_output=True, text=True, timeout=300)
        if r.returncode == 0:
            return out
        errors.append("%s: %s" % (cxx[0], r.stderr[-2000:]))
    raise AssertionError("no host compiler built the sanitized check program:\n" + "\n".join(errors))


def test_header_has_no_hip():
    text = open(os.path.join(ROOT, "metalquicha_amd", "csrc", "eri_dispatch.hpp")).read()
    code = "\n".join(line.split("//")[0] for line in text.splitlines())
    assert "#include" not in code and "hip" not in code.lower()


def test_rule_replay_and_completion(program):
    r = subprocess.run([program], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    print(r.stderr)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "ok"
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr
    assert any(l.startswith("(a)") for l in lines) and any(l.startswith("(c)") for l in lines)
    assert sum("depth" in l for l in lines) == 2 and any("static placement" in l for l in lines)
