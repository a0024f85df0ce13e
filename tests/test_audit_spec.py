"""The numpy restatement of the database audit (tests/audit_spec.py) against values worked out by hand on a 12-entry database, its
15-bit-group coder against the oracle's on ascending input, its species counts against a plain loop.  No GPU, no library."""
import numpy as np

import audit_spec as A

# root -> Bacteria -> genus 10 -> species 11 (strains 21, 22), species 12 (strains 23, 24); 15 and 99 do not exist
PARENT = {1: 1, 2: 1, 10: 2, 11: 10, 12: 10, 21: 11, 22: 11, 23: 12, 24: 12}
RANK = {1: "no rank", 2: "superkingdom", 10: "genus", 11: "species", 12: "species", 21: "no rank", 22: "no rank", 23: "no rank", 24: "no rank"}
LISTED = [21, 22, 23]
E40, E50 = 1 << 40, 1 << 50
#          entry:  0    1    2    3      4      5      6    7        8        9   10       11
VALUES = [100, 100, 250, 250, 40000, 39999, 39999, E40, E40 + 1, E40 + 1, E50, E50 + 5]
TAXIDS = [21, 23, 22, 21, 23, 21, 15, 99, 24, 10, 23, 22]
WORDS_PER_ENTRY = [1, 1, 1, 1, 2, 5, 1, 3, 1, 1, 4, 1]          # deltas 100, 0, 150, 0, 39750, 2^64 - 1 (wrapped), 0, ~2^40, 1, 0, ~2^50, 5
SPLIT = [(0, 0, 0), (250, 4, 4), (E40, 15, 8), (E50, 21, 10)]   # record 3 claims 10 end words before word 21: there are 11


def _db():
    d16 = A.encode_values(np.array(VALUES, np.uint64))
    return d16, np.array(TAXIDS, np.uint32), np.array(SPLIT, np.uint64)


def test_tables_of_the_hand_taxonomy():
    species, known = A.taxonomy_tables(PARENT, RANK, LISTED)
    assert len(species) == 25 and [int(species[t]) for t in (21, 22, 23, 24, 11, 12, 10, 2, 1)] == [11, 11, 12, 0, 11, 12, 0, 0, 0]
    assert known[24] and known[10] and not known[15] and not known[0]
    species, _ = A.taxonomy_tables(PARENT, RANK, LISTED + [10])                             # a listed genus is its own "species"
    assert species[10] == 10


def test_hand_worked_report():
    d16, info, split = _db()
    assert len(d16) == sum(WORDS_PER_ENTRY) == 22
    assert [int(x) for x in np.diff(np.concatenate([[-1], np.flatnonzero(d16 & 0x8000)]))] == WORDS_PER_ENTRY
    values, _ = A.decode_words(d16)
    assert values.tolist() == VALUES
    species, known = A.taxonomy_tables(PARENT, RANK, LISTED)
    R, counts = A.audit(d16.tobytes(), info.tobytes(), split.tobytes(), species, known, LISTED)
    assert R == dict(n_words=22, n_end_words=12, n_trailing_words=0, n_info_entries=12, n_entries=12,
                     n_value_descents=1, first_value_descent=5,                            # 39999 behind 40000
                     n_group_disorder=3, first_group_disorder=3,                           # entries 3 (11 after 11), 6 and 9 (species 0 after 11 / after 0)
                     n_unknown_ids=2, first_unknown_id=6,                                  # ids 15 and 99
                     n_unlisted_ids=2, first_unlisted_id=8, n_no_species=2,                # strain 24 and genus 10: known, not listed, no species
                     n_checkpoints=3, n_bad_checkpoints=1, first_bad_checkpoint=3,
                     n_species=2, valid=0, canonical=0)
    assert counts[11] == 5 and counts[12] == 3 and counts.sum() == 8                      # entries 0 2 3 5 11 / 1 4 10
    assert A.species_counts_text(counts) == "11 5\n12 3\n"
    assert (A.parse_species_counts("11 5\n12 3\n", 25) == counts).all()


def test_hand_worked_variants():
    d16, info, split = _db()
    species, known = A.taxonomy_tables(PARENT, RANK, LISTED)
    R, _ = A.audit(np.concatenate([d16, np.array([7, 9], np.uint16)]), info, split, species, known, LISTED)
    assert R["n_words"] == 24 and R["n_trailing_words"] == 2 and R["n_end_words"] == 12
    R, counts = A.audit(d16, info[:-1], split, species, known, LISTED)
    assert R["n_entries"] == 11 and R["n_info_entries"] == 11 and counts[11] == 4
    assert R["n_checkpoints"] == 3                                                        # record 3: info_off 10 <= 11 entries, still usable
    # the sound part alone: entries 0 .. 2 with the first checkpoint moved onto entry 2
    R, _ = A.audit(A.encode_values(np.array(VALUES[:3], np.uint64)), info[:3], np.array([(0, 0, 0), (250, 3, 3)], np.uint64), species, known, LISTED)
    assert R["valid"] == 1 and R["canonical"] == 1 and R["n_checkpoints"] == 1 and R["first_bad_checkpoint"] == A.NONE
    # bit 31 of a legacy database
    R, _ = A.audit(A.encode_values(np.array(VALUES[:3], np.uint64)), info[:3] | np.uint32(1 << 31), np.zeros(3, np.uint64), species, known, LISTED, info_mask=0x7FFFFFFF)
    assert R["n_unknown_ids"] == 0
    R, _ = A.audit(A.encode_values(np.array(VALUES[:3], np.uint64)), info[:3] | np.uint32(1 << 31), np.zeros(3, np.uint64), species, known, LISTED)
    assert R["n_unknown_ids"] == 3


def test_coder_against_the_oracle(orc):
    rng = np.random.default_rng(9)
    v = np.sort(rng.integers(0, 1 << 63, size=4000).astype(np.uint64))
    v[0] = 0; v[100] = v[99]; v[200] = v[199] + np.uint64(0x7FFF); v[201] = v[200] + np.uint64(0x8000); v[-1] = np.uint64((1 << 64) - 1)
    v = np.sort(v)
    words = A.encode_values(v)
    assert (words == orc.diffidx_encode(v)).all()
    got, ends = A.decode_words(words)
    assert (got == v).all() and (got == orc.diffidx_decode(words)).all() and len(ends) == len(v)
    w = v.copy()
    w[1234] = w[1233] - np.uint64(1)                                                      # a descent survives the round trip as a wrapped delta
    got, _ = A.decode_words(A.encode_values(w))
    assert (got == w).all()


def test_species_counts_against_a_plain_loop():
    rng = np.random.default_rng(4)
    species, known = A.taxonomy_tables(PARENT, RANK, LISTED)
    ids = rng.choice([21, 22, 23, 24, 10, 15, 99, 0], size=3000).astype(np.uint32)
    values = np.sort(rng.integers(1, 1 << 60, size=3000).astype(np.uint64))
    _, counts = A.audit(A.encode_values(values), ids, np.zeros(3, np.uint64), species, known, LISTED)
    want = [0] * len(species)
    for t in ids.tolist():
        if t < len(species) and known[t] and species[t]:
            want[species[t]] += 1
    assert counts.tolist() == want
