"""The k-mer coverage kernels on a machine without a GPU: groups 1, 2, 4 and 8 of tests/test_gpu_coverage.py (`-m gpu`) run in a
subprocess against the library's sources built for the emulator of tests/hipemu (see tests/test_hipemu.py for what that build is and
is not).  MTB_HIPEMU_DIR: reuse a build between runs; without it the build tests/test_hipemu.py made earlier in the same session is
taken if it is there (the build is skipped when it is newer than the sources)."""
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
        d = str(earlier) if (earlier / "libmtb_hipemu.so").exists() else str(tmp_path_factory.mktemp("hipemu_coverage"))
    return build_emulated.build(d)


def _run(lib, select, timeout=900):
    env = dict(os.environ, MTB_HIPEMU="1", MTB_LIB=lib)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_coverage.py"), "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider", "-k", select],
                       env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=timeout)
    tail = r.stdout[-3000:]
    assert r.returncode == 0, tail
    assert " passed" in tail and " failed" not in tail and " skipped" not in tail, tail
    return tail


def test_stage_call_and_refusals_on_the_emulator(emulated_lib):
    """groups 1 and 8: the stage call on indices of 1 .. 4097 entries with queries at every edge; every refusal"""
    tail = _run(emulated_lib, "test_stage_call_at_the_edges or test_refusals")
    assert "10 passed" in tail, tail


def test_index_states_and_fused_path_on_the_emulator(emulated_lib):
    """groups 2 and 4: the stage call against the array in each of its states; the hook of the fused path on short, paired and long reads"""
    tail = _run(emulated_lib, "test_index_states or test_fused_path")
    assert "9 passed" in tail, tail
