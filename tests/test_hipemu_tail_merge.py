"""The tail merge of k_score_fast on a machine without a GPU: every case of tests/test_gpu_fast_tail_merge.py (`-m gpu`) run in a
subprocess against the library's sources built for the emulator of tests/hipemu (see tests/test_hipemu.py for what that build is and
is not) -- the permutation the merge computes, the hand-over counts and the results against the oracle, before a GPU sees them.
The emulator runs a workgroup's lanes in a fixed order, so one order of the tails is checked here; the orders the join's atomics
produce are the GPU run's.  MTB_HIPEMU_DIR: reuse a build between runs; without it the build tests/test_hipemu.py made earlier in the
same session is taken if it is there (the build is skipped when it is newer than the sources)."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def emulated_lib(tmp_path_factory):
    sys.path.insert(0, os.path.join(ROOT, "tests", "hipemu"))
    import build_emulated
    d = os.environ.get("MTB_HIPEMU_DIR")
    if not d:
        earlier = tmp_path_factory.getbasetemp() / "hipemu0"
        d = str(earlier) if (earlier / "libmtb_hipemu.so").exists() else str(tmp_path_factory.mktemp("hipemu_tail_merge"))
    return build_emulated.build(d)


def test_tail_merge_cases_on_the_emulator(emulated_lib):
    env = dict(os.environ, MTB_HIPEMU="1", MTB_LIB=emulated_lib)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_fast_tail_merge.py"), "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider"],
                       env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    tail = r.stdout[-3000:]
    assert r.returncode == 0, tail
    assert "8 passed" in tail and " failed" not in tail and " skipped" not in tail, tail      # (every case ran: none renamed away silently)
