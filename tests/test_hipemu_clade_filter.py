"""The clade filter's kernels and the filtered merge on a machine without a GPU: groups 1 - 6 of tests/test_gpu_clade_filter.py
(`-m gpu`) run in a subprocess against the library's sources built for the emulator of tests/hipemu (see tests/test_hipemu.py for what
that build is and is not).  MTB_HIPEMU_DIR: reuse a build between runs; without it the build tests/test_hipemu.py made earlier in the
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
        d = str(earlier) if (earlier / "libmtb_hipemu.so").exists() else str(tmp_path_factory.mktemp("hipemu_clade"))
    return build_emulated.build(d)


def _run(lib, select, timeout=1800):
    env = dict(os.environ, MTB_HIPEMU="1", MTB_LIB=lib)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_clade_filter.py"), "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider", "-k", select],
                       env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=timeout)
    tail = r.stdout[-3000:]
    assert r.returncode == 0, tail
    assert " passed" in tail and " failed" not in tail and " skipped" not in tail, tail
    return tail


def test_kernels_at_tile_edges_on_the_emulator(emulated_lib):
    """group 1: every size and pattern of the stage call, and the key outside the table"""
    tail = _run(emulated_lib, "test_filter_kernels_at_tile_edges or test_filter_refuses_a_key_outside_the_table")
    assert "7 passed" in tail, tail


def test_filtered_merges_on_the_emulator(emulated_lib):
    """groups 2 - 6: subsets against builds of the kept records, the range cut, several / legacy / foreign inputs, refusals, statistics"""
    tail = _run(emulated_lib, "test_subset_equals_a_build_of_the_kept_species or test_range_cut_does_not_matter or test_several_inputs or test_legacy_input "
                              "or test_input_built_under_another_taxonomy or test_refusals or test_unmatched_ids_are_reported")
    assert "12 passed" in tail, tail
