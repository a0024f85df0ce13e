"""The host side of the database audit (metabuli_amd/csrc/host/audit_plan.h, pure host C++): tests/emu/audit_plan_check.cpp checks
which split records are judged and by which chunk of the stream, the words behind the last end word, and the file checks.  Run once
plain and once under AddressSanitizer + UBSan (a stand-alone host program)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "emu", "audit_plan_check.cpp")


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]], ids=["plain", "asan_ubsan"])
def test_audit_plan(tmp_path, flags):
    exe = str(tmp_path / "audit_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + ["-o", exe, SRC])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.startswith("OK "), r.stdout[-3000:] + r.stderr[-3000:]
    assert int(r.stdout.split()[1]) > 3000
