"""The k-mer coverage rule (mtb_index_coverage_*, `mtb_classify --kmer-coverage 1`), stated once -- numpy only, TEST INFRASTRUCTURE ONLY.

An index has entries t = 0 .. T-1 with
    id[t] = info[t] & info_mask
    sp[t] = species(id[t])                   (mtb_tax_species: the dense table `species`, 0 for an id beyond it or without a species)
Every entry counts, the last one too (the join's "last entry is never a candidate" is no part of this).

A batch has reads r = 0 .. n-1 with result rows res[r] and query metamers q = (value, qinfo); seq(q) = bits 32..60 of qinfo, 1-based,
seq == 0 marks a blank record.
    rs[r] = species(res[r].classification) if res[r].is_classified else 0
A read classified above species rank has rs = 0 and contributes nothing.

    hit          a pair (q, t) with s = rs[seq(q) - 1] != 0, value[t] == value(q) on all 64 bits and sp[t] == s.  A match at hamming
                 distance 1 is another database metamer: not observed.
    marked       the set of all t that occur in a hit, over every batch since the start.  A database that files (value, species) twice
                 has both entries marked.
    hits[s]      the number of query metamers q (every occurrence: every frame, both mates) with at least one hit, s = rs[seq(q) - 1]
    distinct[s]  #{t in marked : sp[t] == s}
    total[s]     #{t : sp[t] == s}           (== mtb_database_audit's species_counts[s] for s != 0)
Integers throughout, independent of any order: every comparison with this file is ==.

The driver's file: `rows` / `format_rows` below."""
import numpy as np

U64 = np.uint64
HEADER = "#taxID\tname\treads\tkmer_hits\tdistinct_kmers\tdb_kmers\tcoverage\tduplication\n"


def seq_of(qinfo):
    return ((np.asarray(qinfo, dtype=U64) >> U64(32)) & U64(0x1FFFFFFF)).astype(np.int64)


def species_lookup(species, ids):
    """species(id) for an array of ids: the table's entry, 0 outside it or where the entry is no valid species id"""
    species = np.asarray(species, dtype=np.int64)
    ids = np.asarray(ids, dtype=np.int64)
    inside = (ids >= 0) & (ids < len(species))
    s = np.where(inside, species[np.where(inside, ids, 0)], 0)
    return np.where((s > 0) & (s < len(species)), s, 0)


class Coverage:
    """values / info: the index's entries in their order (values ascending); species: dense table id -> species over [0, max id]"""

    def __init__(self, values, info, species, info_mask=0xFFFFFFFF):
        self.values = np.asarray(values, dtype=U64)
        assert (self.values[1:] >= self.values[:-1]).all()
        self.species = np.asarray(species, dtype=np.int64)
        self.n_bins = len(self.species)
        self.sp = species_lookup(self.species, (np.asarray(info, dtype=np.uint32) & np.uint32(info_mask)).astype(np.int64))
        self.marked = np.zeros(len(self.values), bool)
        self.hits = np.zeros(self.n_bins, U64)
        self.n_queries = self.n_queries_counted = self.n_batches = 0

    def read_species(self, results):
        return np.where(results["is_classified"] != 0, species_lookup(self.species, results["classification"]), 0)

    def add_batch(self, kmers, results):
        """one classify call (or stage call) that succeeded"""
        self.n_batches += 1
        rs = self.read_species(results)
        seq = seq_of(kmers["qinfo"])
        assert (seq <= len(results)).all()
        live = seq != 0
        s = np.where(live, rs[np.where(live, seq - 1, 0)], 0) if len(results) else np.zeros(len(seq), np.int64)
        self.n_queries += int(live.sum()); self.n_queries_counted += int((s != 0).sum())
        qv = np.asarray(kmers["value"], dtype=U64)[s != 0]; qs = s[s != 0]
        lo = np.searchsorted(self.values, qv, side="left"); hi = np.searchsorted(self.values, qv, side="right")
        n = hi - lo                                                                       # entries with the query's value
        q_of = np.repeat(np.arange(len(qv)), n)
        t = np.repeat(lo, n) + (np.arange(int(n.sum())) - np.repeat(np.cumsum(n) - n, n))
        ok = self.sp[t] == qs[q_of]
        self.marked[t[ok]] = True
        hit = np.zeros(len(qv), bool); hit[q_of[ok]] = True
        self.hits += np.bincount(qs[hit], minlength=self.n_bins).astype(U64)
        return self

    def report(self):
        total = np.bincount(self.sp, minlength=self.n_bins).astype(U64); total[0] = 0
        distinct = np.bincount(self.sp[self.marked], minlength=self.n_bins).astype(U64); distinct[0] = 0
        return dict(distinct=distinct, hits=self.hits.copy(), total=total, n_targets=len(self.values), n_marked=int(self.marked.sum()),
                    n_hits=int(self.hits.sum()), n_queries=self.n_queries, n_queries_counted=self.n_queries_counted, n_batches=self.n_batches)


def same_report(got, want):
    """the library's report dict against this file's: every array and every counter (the time excepted)"""
    for k in ("distinct", "hits", "total"):
        assert np.array_equal(np.asarray(got[k], dtype=U64), want[k]), k
    for k in ("n_targets", "n_marked", "n_hits", "n_queries", "n_queries_counted", "n_batches"):
        assert int(got[k]) == int(want[k]), (k, int(got[k]), int(want[k]))


def rows(tax_counts, species, distinct, hits, total, original=None):
    """(printed id, species, reads, hits, distinct, db) of every species with reads, ascending by the printed id.  tax_counts: reads
    per classification {id: n}; reads of species s = the sum over the ids c with species(c) == s; original: id -> printed id"""
    reads = {}
    for c, n in tax_counts.items():
        s = int(species_lookup(species, [c])[0])
        if s and n:
            reads[s] = reads.get(s, 0) + int(n)
    out = [((original[s] if original is not None else s), s, n, int(hits[s]), int(distinct[s]), int(total[s])) for s, n in reads.items()]
    return sorted(out)


def format_rows(rws, name):
    """<JobID>_kmer_coverage.tsv: coverage = distinct / db_kmers as %.6f, duplication = hits / distinct as %.3f (0.000 without a distinct k-mer)"""
    text = HEADER
    for printed, s, reads, h, d, db in rws:
        text += "%d\t%s\t%d\t%d\t%d\t%d\t%.6f\t%.3f\n" % (printed, name[s], reads, h, d, db, (d / db) if db else 0.0, (h / d) if d else 0.0)
    return text
