"""The block scan's kernels on a machine without a GPU: the stage-call cases of tests/test_gpu_blocks.py (`-m gpu`) run in a subprocess
against the library's sources built for the emulator of tests/hipemu (see tests/test_hipemu.py for what that build is and is not).
MTB_HIPEMU_DIR: reuse a build between runs; without it the build tests/test_hipemu.py made earlier in the same session is taken if
it is there (the build is skipped when it is newer than the sources)."""
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
        d = str(earlier) if (earlier / "libmtb_hipemu.so").exists() else str(tmp_path_factory.mktemp("hipemu_blocks"))
    return build_emulated.build(d)


def _run(lib, select, timeout=900):
    env = dict(os.environ, MTB_HIPEMU="1", MTB_LIB=lib)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_blocks.py"), "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider", "-k", select],
                       env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=timeout)
    tail = r.stdout[-3000:]
    assert r.returncode == 0, tail
    assert " passed" in tail and " failed" not in tail and " skipped" not in tail, tail
    return tail


def test_extract_blocks_on_the_emulator(emulated_lib):
    """every scenario of mtb_extract_blocks, dense and syncmer: piece boundaries, both strands, invalid bases, 70 000 blocks"""
    tail = _run(emulated_lib, "test_extract_blocks_against_oracle")
    assert "18 passed" in tail, tail


def test_capacity_and_refusals_on_the_emulator(emulated_lib):
    tail = _run(emulated_lib, "test_capacity_too_small_returns_the_required_size or test_argument_errors or test_unknown_taxid_and_old_format_are_refused "
                              "or test_builder_records_carry_the_taxid_of_the_blocks_sequence")
    assert "7 passed" in tail, tail
