"""The database side's shared code on a machine without a GPU -- the range decode every reader goes through (partitions of an open, slices
of a merge, the writer's second look), the two-sort and the group reduction that the builder and the merge share: cases of
tests/test_gpu_merge_stream.py, tests/test_gpu_build.py and tests/test_partitioned.py (`-m gpu`) run in a subprocess against the
library's sources built for the emulator of tests/hipemu (see tests/test_hipemu.py for what that build is and is not).
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
        d = str(earlier) if (earlier / "libmtb_hipemu.so").exists() else str(tmp_path_factory.mktemp("hipemu_dbio"))
    return build_emulated.build(d)


def _run(lib, module, select, timeout=900):
    env = dict(os.environ, MTB_HIPEMU="1", MTB_LIB=lib)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", module), "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider", "-k", select],
                       env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=timeout)
    tail = r.stdout[-3000:]
    assert r.returncode == 0, tail
    assert " passed" in tail and " failed" not in tail and " skipped" not in tail, tail
    return tail


def test_merge_ranges_and_resorted_slices_on_the_emulator(emulated_lib):
    """slices decoded from checkpoint to checkpoint under two split_num and two budgets (one range / many), groups that straddle inputs and
    ranges; an input that is out of order under the merge's taxonomy goes through the two sorts the builder uses"""
    tail = _run(emulated_lib, "test_gpu_merge_stream.py", "test_groups_straddle_inputs_and_ranges or test_input_out_of_order_under_the_merges_taxonomy")
    assert "5 passed" in tail, tail


def test_builder_groups_and_update_on_the_emulator(emulated_lib):
    """the group reduction on every group shape (long groups included), and a written database updated and merged: writer, checkpoints, reopen"""
    tail = _run(emulated_lib, "test_gpu_build.py", "test_group_shapes or test_update_and_merge")
    assert "2 passed" in tail, tail


def test_partitions_of_an_open_on_the_emulator(emulated_lib):
    """every partition's range decoded on its own: the partitions concatenate to the whole index; more partitions than checkpoints"""
    tail = _run(emulated_lib, "test_partitioned.py", "test_gpu_partitions_concatenate_to_the_index or test_gpu_partitions_with_empty_ranges")
    assert "2 passed" in tail, tail
