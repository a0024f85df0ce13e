"""The database audit's kernels on a machine without a GPU: the stage cases of tests/test_gpu_audit.py (`-m gpu`) run in a subprocess
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
        d = str(earlier) if (earlier / "libmtb_hipemu.so").exists() else str(tmp_path_factory.mktemp("hipemu_audit"))
    return build_emulated.build(d)


def _run(lib, select, timeout=900):
    env = dict(os.environ, MTB_HIPEMU="1", MTB_LIB=lib)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_audit.py"), "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider", "-k", select],
                       env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=timeout)
    tail = r.stdout[-3000:]
    assert r.returncode == 0, tail
    assert " passed" in tail and " failed" not in tail and " skipped" not in tail, tail
    return tail


def test_reports_on_the_emulator(emulated_lib):
    """the sound database, disagreeing counts, order defects on both sides of every chunk boundary, ids, checkpoints, the large taxonomy"""
    tail = _run(emulated_lib, "test_untouched_database_is_canonical or test_species_count_file or test_one_chunk_gives_the_same_report or test_counts_that_disagree "
                              "or test_order_defects_at_chunk_edges or test_ids_against_the_taxonomy or test_legacy_database_bit_31_is_masked or test_large_taxonomy "
                              "or test_checkpoints")
    assert "20 passed" in tail, tail


def test_refusals_and_library_outputs_on_the_emulator(emulated_lib):
    tail = _run(emulated_lib, "test_cap_too_small or test_file_problems or test_reduced_alphabet_is_refused or test_builder_and_merge_outputs_are_canonical")
    assert "12 passed" in tail, tail
