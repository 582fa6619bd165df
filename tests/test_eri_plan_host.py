"""Host test of the integral stage's planned launch sequence (metalquicha_amd/csrc/eri_plan.hpp): tests/host/check_eri_plan.cpp
is compiled for the host with the address and undefined-behaviour sanitizers, as a stand-alone program, and run.  The
program checks (a) that the planner returns the dense order, the lanes and the task order which the build before it used
in three recorded calls (profiles/r07_a_launch_sequence_parent_vs_tree.log: plain spread, static task stream, one side
stream), (b) the plan's properties over 16000 randomised small tables with many equal and zero costs, and (c) that the walk
over the two queues issues every item once, the copy once and right behind the last task item, whatever the lane source
answers, and reproduces the recorded interleaving of the static task stream.  No GPU: the header has no HIP in it."""
import os
import subprocess

import pytest

from tests.test_eri_dispatch_host import ROOT, SANITIZE, compilers

SRC = os.path.join(ROOT, "tests", "host", "check_eri_plan.cpp")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("eri_plan") / "check_eri_plan")
    errors = []
    for cxx in compilers():
        r = subprocess.run(cxx + ["-std=c++17", "-O1", "-g"] + SANITIZE + [SRC, "-o", out], capture_output=True, text=True, timeout=300)
        if r.returncode == 0:
            return out
        errors.append("%s: %s" % (cxx[0], r.stderr[-2000:]))
    raise AssertionError("no host compiler built the sanitized check program:\n" + "\n".join(errors))


def test_header_has_no_hip():
    text = open(os.path.join(ROOT, "metalquicha_amd", "csrc", "eri_plan.hpp")).read()
    code = "\n".join(line.split("//")[0] for line in text.splitlines())
    assert "hip" not in code.lower() and "engine.hpp" not in code
    includes = [line.split()[1] for line in code.splitlines() if line.strip().startswith("#include")]
    assert all(i == '"eri_dispatch.hpp"' or i.startswith("<") for i in includes), includes


def test_goldens_properties_and_walk(program):
    r = subprocess.run([program], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    print(r.stderr)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "ok"
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr
    assert all(any(l.startswith(tag) for l in lines) for tag in ("(a) 3 recorded calls", "(b)", "(c)"))
    assert any("configuration c" in l for l in lines)
