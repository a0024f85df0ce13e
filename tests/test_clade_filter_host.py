"""The host side of the filtered merge (metabuli_amd/csrc/host/clade_filter.h, pure host C++): tests/clade_filter_check.cpp prints
keep[], the refusals and the statistics for the toy tree of tests/clade_filter_spec.py and for a deep chain; the output is compared
with the spec.  Run once plain and once under AddressSanitizer + UBSan (a stand-alone host program)."""
import os
import subprocess

import numpy as np
import pytest

import clade_filter_spec as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "clade_filter_check.cpp")

RECORD_IDS = [111, 112, 12, 900, 21, 211, 1, 30, 901, 2]
CASES = [([10], []), ([10], [12]), ([], [1]), ([1], []), ([], [30]), ([], [900]), ([900], []), ([11, 30], []), ([10, 11], [10]), ([], [20, 22]), ([22, 31], [900]),
         ([2], [21, 10]), ([111], []), ([], [901]), ([211], []), ([10], [311]), ([777], []), ([10], [5000]), ([], [0]), ([], [])]


@pytest.fixture(scope="module", params=[["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]], ids=["plain", "asan_ubsan"])
def exe(request, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("clade_filter_check") / "clade_filter_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror"] + request.param + ["-o", path, SRC])
    return path


def _arg(ids):
    return ",".join(str(i) for i in ids) if len(ids) else "-"


def _run(exe, taxdir, select, exclude, record_ids=None):
    r = subprocess.run([exe, taxdir, _arg(select), _arg(exclude)] + ([_arg(record_ids)] if record_ids is not None else []), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return r.stdout.strip().split("\n")


def _compare(exe, taxdir, tax, aliases, select, exclude, record_ids):
    lines = _run(exe, taxdir, select, exclude, record_ids)
    try:
        keep = S.keep_table(tax, aliases, select, exclude)
    except S.Refusal as e:
        assert lines == [f"refused {e.kind} {e.taxid if e.taxid is not None else 0}"], (select, exclude, lines)
        return "refused"
    assert lines[0] == "keep " + "".join("1" if k else "0" for k in keep), (select, exclude)
    st = S.statistics(tax, aliases, select, exclude, record_ids)
    assert lines[1] == "stats {n_records_in} {n_records_kept} {n_species_kept} {n_species_dropped} {n_unmatched} {first_unmatched}".format(**st), (select, exclude, lines[1])
    return "kept"


def test_toy_tree(exe, tmp_path):
    tax, aliases = S.toy_tree()
    taxdir = S.write_taxonomy(tax, aliases, str(tmp_path / "tax"))
    seen = [_compare(exe, taxdir, tax, aliases, sel, exc, RECORD_IDS) for sel, exc in CASES]
    assert seen.count("refused") == 8 and seen.count("kept") == 12


def test_deep_chain_and_wide_fan(exe, tmp_path):
    """a chain of 1000 clades above one genus (the climb is iterative and every node is folded once) beside a genus with 500 species"""
    from metabuli_amd import synth
    tax = synth.Taxonomy()
    tax.add(1, 1, "no rank", "root")
    prev = 1
    for k in range(1000):
        tax.add(10 + k, prev, "clade", f"c{k}")
        prev = 10 + k
    tax.add(5000, prev, "genus", "deep genus"); tax.add(5001, 5000, "species", "deep species"); tax.add(5002, 5001, "no rank", "deep strain")
    tax.add(6000, 1, "genus", "wide genus")
    for k in range(500):
        tax.add(6001 + k, 6000, "species", f"w{k}")
    taxdir = S.write_taxonomy(tax, {}, str(tmp_path / "tax"))
    rng = np.random.default_rng(3)
    ids = [5002, 5001] + [int(x) for x in rng.integers(6001, 6501, 40)]
    for sel, exc in (([500], []), ([], [10]), ([6000], [6007, 6100]), ([5000, 6499], [999]), ([], [5002])):
        _compare(exe, taxdir, tax, {}, sel, exc, ids)
