"""tests/inspect_spec.py on hand-written cases whose answers are written out here, its invariants, one report in full, and a
brute-force grouping against the run-based one.  No library code runs."""
import numpy as np
import pytest

import inspect_spec as S

# root 1 -> domain 2 -> genera 10, 20, 30 -> three species each -> two strains each
PARENT = {1: 1, 2: 1}
RANK = {1: "no rank", 2: "superkingdom"}
NAME = {1: "root", 2: "Bacteria"}
for g in (10, 20, 30):
    PARENT[g] = 2; RANK[g] = "genus"; NAME[g] = f"G{g}"
    for s in (1, 2, 3):
        sp = g + s
        PARENT[sp] = g; RANK[sp] = "species"; NAME[sp] = f"G{g} s{s}"
        for k in (1, 2):
            st = sp * 10 + k
            PARENT[st] = sp; RANK[st] = "strain"; NAME[st] = f"G{g} s{s} strain {k}"
PARENT[40] = 1; RANK[40] = "genus"; NAME[40] = "G40 outside the domain"
PARENT[41] = 40; RANK[41] = "species"; NAME[41] = "G40 s1"
TAX = S.Tax(PARENT, RANK, NAME, aliases={999: 212})
UNKNOWN = 5000


def v(aa, dna=0):
    return (aa << 24) | dna


def run(rows, level=0, mask=0xFFFFFFFF):
    values = np.array([r[0] for r in rows], np.uint64); info = np.array([r[1] for r in rows], np.uint32)
    return S.inspect(values, info, TAX, level, mask)


def bins(arr):
    return {int(t): int(arr[t]) for t in np.flatnonzero(arr)}


def test_two_strains_of_one_species_meet_at_the_species():
    R, d, e = run([(v(1), 111), (v(1), 112)])
    assert bins(d) == {11: 1} and bins(e) == {11: 2} and R["n_groups"] == 1 and R["max_group"] == 2 and R["first_max_group"] == 0


def test_two_species_of_a_genus_meet_at_the_genus():
    R, d, e = run([(v(1), 111), (v(1), 121), (v(1), 131)])
    assert bins(d) == {10: 1} and bins(e) == {10: 3}


def test_species_of_two_genera_meet_at_their_parent():
    R, d, e = run([(v(1), 111), (v(1), 211)])
    assert bins(d) == {2: 1} and bins(e) == {2: 2}
    R, d, e = run([(v(1), 111), (v(1), 41)])
    assert bins(d) == {1: 1} and bins(e) == {1: 2}


def test_an_unknown_id_is_skipped_and_counted_in_the_size():
    R, d, e = run([(v(1), 111), (v(1), UNKNOWN), (v(1), 112)])
    assert bins(d) == {11: 1} and bins(e) == {11: 3} and R["n_orphan_groups"] == 0 and R["size_hist"][1] == 1


def test_a_group_of_unknown_ids_is_an_orphan():
    R, d, e = run([(v(1), UNKNOWN), (v(1), UNKNOWN + 1), (v(2), 111)])
    assert bins(d) == {111: 1} and bins(e) == {111: 1}
    assert R["n_orphan_groups"] == 1 and R["n_orphan_entries"] == 2 and R["n_groups"] == 2 and R["n_entries"] == 3


def test_an_alias_counts_as_its_current_node():
    R, d, e = run([(v(1), 999)])
    assert bins(d) == {212: 1} and bins(e) == {212: 1}                                  # a group of one: the canonical node
    R, d, e = run([(v(1), 999), (v(1), 211)])
    assert bins(d) == {21: 1} and bins(e) == {21: 2}


def test_the_last_entry_belongs_to_its_group():
    R, d, e = run([(v(1), 111), (v(2), 211), (v(2), 221)])
    assert bins(d) == {111: 1, 20: 1} and bins(e) == {111: 1, 20: 2} and R["n_groups"] == 2
    R, d, e = run([(v(1), 111), (v(2), 211)])                                           # ... and alone in it
    assert bins(d) == {111: 1, 211: 1} and R["n_groups"] == 2


def test_level_1_joins_values_that_differ_in_the_low_24_bits():
    rows = [(v(7, 1), 111), (v(7, 2), 121), (v(7, 0xFFFFFF), 211), (v(8, 0), 311)]
    R0, d0, e0 = run(rows, level=0)
    assert bins(d0) == {111: 1, 121: 1, 211: 1, 311: 1} and R0["n_groups"] == 4 and R0["size_hist"][0] == 4
    R1, d1, e1 = run(rows, level=1)
    assert bins(d1) == {2: 1, 311: 1} and bins(e1) == {2: 3, 311: 1} and R1["n_groups"] == 2
    assert R1["max_group"] == 3 and R1["first_max_group"] == 0 and R1["size_hist"][:2] == [1, 1]


def test_bit_31_is_masked_by_the_legacy_mask_only():
    rows = [(v(1), 111 | (1 << 31)), (v(1), 112)]
    R, d, e = run(rows, mask=0x7FFFFFFF)
    assert bins(d) == {11: 1}
    R, d, e = run(rows)                                                                  # the departure: no unconditional masking
    assert bins(d) == {112: 1} and bins(e) == {112: 2}


def test_an_empty_list_and_the_first_of_equal_largest_groups():
    R, d, e = run([])
    assert R["n_groups"] == 0 and R["max_group"] == 0 and R["first_max_group"] == S.NONE and not d.any()
    R, d, e = run([(v(1), 111), (v(2), 111), (v(2), 111), (v(3), 111), (v(3), 111)])
    assert R["max_group"] == 2 and R["first_max_group"] == 1 and R["size_hist"][:2] == [1, 2]


CASE = [(v(1), 111), (v(1), 112), (v(2), 111), (v(2), 121), (v(3), 211), (v(3), 311), (v(3), UNKNOWN), (v(4), UNKNOWN), (v(5), 41), (v(5), 111), (v(6), 999)]


def test_invariants():
    for level in (0, 1):
        R, d, e = run(CASE, level)
        assert int(d.sum()) + R["n_orphan_groups"] == R["n_groups"] == sum(R["size_hist"])
        assert int(e.sum()) + R["n_orphan_entries"] == R["n_entries"] == len(CASE)


def test_clade_sums_and_the_report_in_full():
    R, d, e = run(CASE)
    assert bins(d) == {11: 1, 10: 1, 2: 1, 1: 1, 212: 1} and bins(e) == {11: 2, 10: 2, 2: 3, 1: 2, 212: 1}
    assert R["n_orphan_groups"] == 1 and R["n_orphan_entries"] == 1 and R["n_groups"] == 6
    dc, ec = S.clade_sums(TAX, d), S.clade_sums(TAX, e)
    assert bins(dc) == {1: 5, 2: 4, 10: 2, 11: 1, 20: 1, 21: 1, 212: 1} and bins(ec) == {1: 10, 2: 8, 10: 4, 11: 2, 20: 1, 21: 1, 212: 1}
    assert S.report_text(TAX, d, e) == (
        "original_taxid\trank\tname\tdistinct\tentries\tdistinct_clade\tentries_clade\n"
        "1\tno rank\troot\t1\t2\t5\t10\n"
        "2\tsuperkingdom\tBacteria\t1\t3\t4\t8\n"
        "10\tgenus\tG10\t1\t2\t2\t4\n"
        "11\tspecies\tG10 s1\t1\t2\t1\t2\n"
        "20\tgenus\tG20\t0\t0\t1\t1\n"
        "21\tspecies\tG20 s1\t0\t0\t1\t1\n"
        "212\tstrain\tG20 s1 strain 2\t1\t1\t1\t1\n")
    assert S.summary_text(TAX, d, e, R["n_groups"]) == (
        "Common k-mers count by rank:\nroot: 2\nsuperkingdom: 3\ngenus: 2\nspecies: 2\nstrain: 1\n"
        "Total distinct common k-mers count: 6\n"
        "Distinct common k-mers count by rank:\nroot: 1\nsuperkingdom: 1\ngenus: 1\nspecies: 1\nstrain: 1\n")


@pytest.mark.parametrize("level", [0, 1])
def test_brute_force_grouping_agrees(level):
    rng = np.random.default_rng(11)
    leaves = [t for t in PARENT if RANK[t] == "strain"] + [41, 999, UNKNOWN, UNKNOWN + 1]
    aa = np.sort(rng.integers(1, 900, size=5000)).astype(np.uint64)
    dna = rng.integers(0, 4, size=5000).astype(np.uint64)
    values = (aa << np.uint64(24)) | dna
    values = values[np.lexsort((dna, aa))]
    info = rng.choice(leaves, size=5000).astype(np.uint32)
    info[rng.random(5000) < 0.3] = UNKNOWN                                               # enough unknown ids for orphan groups
    R, d, e = S.inspect(values, info, TAX, level)
    bd, be, orphan, n_groups = S.brute_force(values, info, TAX, level)
    assert (bd == d).all() and (be == e).all() and orphan == [R["n_orphan_groups"], R["n_orphan_entries"]] and n_groups == R["n_groups"]
    assert R["n_orphan_groups"] > 0 and R["max_group"] > 4
