"""tests/coverage_spec.py (the k-mer coverage rule) on inputs whose answer is written out here, on the toy databases against figures
taken independently of it, and its formatter of <JobID>_kmer_coverage.tsv.  No GPU: the library is compared with the spec in
tests/test_gpu_coverage.py."""
import numpy as np
import pytest

import coverage_spec as cs
from helpers import kmer_dt, result_dt

# ids: 1 root, 2 a genus, 3 / 4 / 5 its species A / B / C, 6 a strain of A, 7 species D
SPECIES = np.array([0, 0, 0, 3, 4, 5, 3, 7])
A, B, C_, D = 3, 4, 5, 7
#          t0  t1  t2  t3  t4  t5  t6  t7
VALUES = [10, 20, 20, 20, 30, 30, 40, 50]
INFO = [3, 3, 4, 5, 6, 3, 2, 7]            # value 20 under three species; (30, A) twice (a strain's entry and the species'); a genus-labelled entry


def _q(value, read, pos=0, frame=0):
    return (value, (pos & 0xFFFFFFFF) | (read << 32) | (frame << 61))


def _results(rows):
    r = np.zeros(len(rows), result_dt)
    for i, (cls, ok) in enumerate(rows):
        r[i]["classification"] = cls; r[i]["is_classified"] = ok
    return r


#                   r1      r2      r3       r4      r5 unclassified  r6 at the genus  r7 at a strain of A
RESULTS = _results([(A, 1), (B, 1), (C_, 1), (D, 1), (A, 0), (2, 1), (6, 1)])
QUERIES = np.array([
    _q(20, 1), _q(20, 2), _q(20, 3),       # the read's species first, in the middle, last in the run of value 20
    _q(20, 4),                             # ... and absent from it
    _q(30, 1),                             # a duplicate (value, species): both entries are marked, one hit
    _q(20, 0),                             # a blank record
    _q(20, 5),                             # an unclassified read
    _q(20, 6), _q(40, 6),                  # a read classified at a genus: nothing, not even the genus-labelled entry
    _q(10, 7, pos=3, frame=1), _q(10, 7, pos=90, frame=4),      # both mates of a pair (read 7) hold the metamer: two hits, one entry
    _q(50, 1), _q(50, 4),                  # the entry of another species; its own
    _q(21, 1),                             # one bit off value 20: another metamer
], dtype=kmer_dt)


def test_hand_made_batch():
    r = cs.Coverage(VALUES, INFO, SPECIES).add_batch(QUERIES, RESULTS).report()
    want = np.zeros(8, np.uint64)

    def arr(**kw):
        a = want.copy()
        for k, v in kw.items():
            a[int(k[1:])] = v
        return a
    assert np.array_equal(r["total"], arr(s3=4, s4=1, s5=1, s7=1))
    assert np.array_equal(r["distinct"], arr(s3=4, s4=1, s5=1, s7=1))          # t0, t1, t4, t5 | t2 | t3 | t7
    assert np.array_equal(r["hits"], arr(s3=4, s4=1, s5=1, s7=1))              # A: value 20, value 30, value 10 twice
    assert r["n_marked"] == 7 and r["n_hits"] == 7 and r["n_targets"] == 8
    assert r["n_queries"] == 13 and r["n_queries_counted"] == 10 and r["n_batches"] == 1


def test_each_hand_made_case_on_its_own():
    def one(q, res=RESULTS):
        c = cs.Coverage(VALUES, INFO, SPECIES).add_batch(np.array(q, dtype=kmer_dt), res)
        return sorted(np.flatnonzero(c.marked).tolist()), {int(s): int(n) for s, n in enumerate(c.hits) if n}
    assert one([_q(20, 1)]) == ([1], {A: 1})
    assert one([_q(20, 2)]) == ([2], {B: 1})
    assert one([_q(20, 3)]) == ([3], {C_: 1})
    assert one([_q(20, 4)]) == ([], {})
    assert one([_q(30, 1)]) == ([4, 5], {A: 1})
    assert one([_q(30, 7)]) == ([4, 5], {A: 1})                               # the strain's species
    assert one([_q(20, 0)]) == ([], {})
    assert one([_q(20, 5)]) == ([], {})
    assert one([_q(20, 6), _q(40, 6)]) == ([], {})
    assert one([_q(10, 7, 3, 1), _q(10, 7, 90, 4)]) == ([0], {A: 2})
    assert one([_q(50, 1)]) == ([], {}) and one([_q(50, 4)]) == ([7], {D: 1})   # the last entry counts
    assert one([_q(21, 1)]) == ([], {}) and one([_q(9, 1)]) == ([], {}) and one([_q(51, 4)]) == ([], {})
    assert one([], RESULTS) == ([], {})


def test_batches_accumulate_and_marks_are_idempotent():
    c = cs.Coverage(VALUES, INFO, SPECIES).add_batch(QUERIES, RESULTS)
    once = c.report()
    twice = c.add_batch(QUERIES, RESULTS).report()
    assert np.array_equal(twice["distinct"], once["distinct"]) and np.array_equal(twice["hits"], 2 * once["hits"]) and twice["n_batches"] == 2
    halves = cs.Coverage(VALUES, INFO, SPECIES).add_batch(QUERIES[:7], RESULTS).add_batch(QUERIES[7:], RESULTS).report()
    assert np.array_equal(halves["distinct"], once["distinct"]) and np.array_equal(halves["hits"], once["hits"])


def test_legacy_mask_and_ids_outside_the_table():
    info = np.array(INFO, np.uint32); info[1] |= np.uint32(1 << 31)            # the redundancy bit of a Skip_redundancy 0 database
    r = cs.Coverage(VALUES, info, SPECIES, info_mask=0x7FFFFFFF).add_batch(QUERIES, RESULTS).report()
    assert int(r["distinct"][A]) == 4 and int(r["total"][A]) == 4
    r = cs.Coverage(VALUES, info, SPECIES).add_batch(QUERIES, RESULTS).report()    # unmasked: an id beyond the table, species 0
    assert int(r["distinct"][A]) == 3 and int(r["total"][A]) == 3
    res = RESULTS.copy(); res[0]["classification"] = 1000                       # a classification beyond the table
    assert int(cs.Coverage(VALUES, INFO, SPECIES).add_batch(QUERIES[:1], res).report()["n_hits"]) == 0


# T, reads, reads with a species, species with a distinct k-mer, sum of distinct, sum of hits: worked out apart from the spec, with the
# species of every id taken from the synthetic world's own taxonomy
TOY_FIGURES = {
    "sync_se": (507238, 400, 364, 12, 34446, 35543),
    "dense_pe": (996784, 400, 356, 12, 128978, 140934),
    "sync_long": (505672, 40, 38, 12, 33599, 35021),
}


def toy_spec(orc, t):
    """the spec's report of one pass of a conftest.Toy's reads, from the oracle's metamers and results; the species table is the one
    KmerMatcher::loadTaxIdList builds (helpers.tax2species_table)"""
    from helpers import tax2species_table
    table = tax2species_table(orc, t.tax, t.taxids, max(t.world.tax.parent))
    return cs.Coverage(t.values, t.taxids.astype(np.uint32), table), table


@pytest.mark.parametrize("mode", sorted(TOY_FIGURES))
def test_toy_figures(orc, tmp_path, mode):
    from conftest import Toy, TOY_MODES
    t = Toy(orc, tmp_path, **TOY_MODES[mode])
    c, table = toy_spec(orc, t)
    world_species = np.array([t.world.tax.species_of(i) if i in t.world.tax.parent else 0 for i in range(len(table))])
    listed = np.unique(t.taxids)
    assert (table[listed] == world_species[listed]).all()
    r = c.add_batch(t.ref["kmers"], t.ref["results"]).report()
    counted = int((c.read_species(t.ref["results"]) != 0).sum())
    got = (r["n_targets"], len(t.ref["results"]), counted, int((r["distinct"] > 0).sum()), int(r["distinct"].sum()), int(r["hits"].sum()))
    assert got == TOY_FIGURES[mode]
    assert r["n_marked"] == int(r["distinct"].sum()) and int(r["total"].sum()) == r["n_targets"]
    # no toy read is classified above species rank: that case is the hand-made one
    cls = t.ref["results"]
    assert counted == int((cls["is_classified"] != 0).sum())


def test_rows_and_formatter():
    species = SPECIES
    distinct = np.array([0, 0, 0, 4, 0, 1, 0, 1], np.uint64); hits = np.array([0, 0, 0, 9, 0, 1, 0, 3], np.uint64)
    total = np.array([0, 0, 0, 4, 1, 3, 0, 1000000], np.uint64)
    counts = {0: 5, 2: 7, 3: 2, 6: 3, 4: 1, 7: 6}                              # unclassified, at the genus, A and its strain, B, D; C has no reads
    original = {3: 900, 4: 30, 5: 31, 7: 29}
    rws = cs.rows(counts, species, distinct, hits, total, original)
    assert rws == [(29, 7, 6, 3, 1, 1000000), (30, 4, 1, 0, 0, 1), (900, 3, 5, 9, 4, 4)]
    name = {3: "Species A", 4: "B b", 5: "C", 7: "D"}
    assert cs.format_rows(rws, name) == (
        "#taxID\tname\treads\tkmer_hits\tdistinct_kmers\tdb_kmers\tcoverage\tduplication\n"
        "29\tD\t6\t3\t1\t1000000\t0.000001\t3.000\n"
        "30\tB b\t1\t0\t0\t1\t0.000000\t0.000\n"
        "900\tSpecies A\t5\t9\t4\t4\t1.000000\t2.250\n")
    assert cs.rows({3: 0}, species, distinct, hits, total) == []
