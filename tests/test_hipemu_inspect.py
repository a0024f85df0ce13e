"""The database inspection's kernels on a machine without a GPU: cases of tests/test_gpu_inspect.py (`-m gpu`) run in a subprocess
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
        d = str(earlier) if (earlier / "libmtb_hipemu.so").exists() else str(tmp_path_factory.mktemp("hipemu_inspect"))
    return build_emulated.build(d)


def _run(lib, select, timeout=900):
    env = dict(os.environ, MTB_HIPEMU="1", MTB_LIB=lib)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_inspect.py"), "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider", "-k", select],
                       env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=timeout)
    tail = r.stdout[-3000:]
    assert r.returncode == 0, tail
    assert " passed" in tail and " failed" not in tail and " skipped" not in tail, tail
    return tail


def test_stage_call_on_the_emulator(emulated_lib):
    """groups of one, sizes 2..9 on every lane, wave, tile and pass edge at both levels, the list's ends, the long level-1 groups, the
    boundary lengths, unknown ids, bit 31, the sparse taxonomy, both skews"""
    tail = _run(emulated_lib, "test_groups_of_one or test_groups_on_every_edge or test_a_key_that_comes_back_is_a_new_group or test_first_and_last_entry or test_long_groups_at_level_1 or test_a_list_that_is_one_group "
                              "or test_small_and_boundary_lengths or test_unknown_ids or test_bit_31_with_and_without_the_legacy_mask or test_large_sparse_taxonomy "
                              "or test_most_groups_meet_at_the_root or test_every_group_stays_inside_its_species")
    assert "23 passed" in tail, tail


def test_directory_call_refusals_and_program_on_the_emulator(emulated_lib):
    tail = _run(emulated_lib, "test_directory_call or test_report_writer or test_cap_too_small or test_a_missing_file or test_reduced_alphabet_is_refused or test_a_bad_level "
                              "or test_mtb_build")
    assert "16 passed" in tail, tail
