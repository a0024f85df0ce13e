"""The range planner of the streamed database merge (metabuli_amd/csrc/host/merge_plan.h, pure host C++): tests/emu/merge_plan_check.cpp
plans seeded random sets of 1 to 9 databases -- empty and all-zero split tables, very different checkpoint densities -- and checks
coverage (every entry in exactly one range, inside its input's slice), ascending amino-acid aligned bounds, the budget, the CAPACITY
case and the single-interval case.  Run once plain and once under AddressSanitizer + UBSan (a stand-alone host program)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "emu", "merge_plan_check.cpp")


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]], ids=["plain", "asan_ubsan"])
def test_merge_plan(tmp_path, flags):
    exe = str(tmp_path / "merge_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + ["-o", exe, SRC])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.startswith("OK "), r.stdout[-3000:] + r.stderr[-3000:]
    assert int(r.stdout.split()[1]) > 300
