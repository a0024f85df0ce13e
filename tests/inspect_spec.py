"""The rule of the database inspection (mtb_database_inspect, mtb_inspect_records, mtb_inspect_write_report; include/mtb.h) in numpy and
plain Python -- test infrastructure, no library code.  Everything else is checked against this file.

The question is the reference's expert command count-common-kmers (src/util/count_common_kmers.cpp:43-105) and kraken2-inspect's: for
every distinct k-mer of a database, at which node of the taxonomy do its owners meet, and how many k-mers does each node hold that way.

Input      entries 0..n-1 of a database in file order: values (u64) and info (u32); from files, n = min(end words, info entries).
Id         info & info_mask, as everywhere in the library.  DEPARTURE: the reference masks bit 31 unconditionally (:56, :74).
Key        level 0 ("dna"): the 64-bit value (the reference's rule); level 1 ("aa"): value >> 24, for both k-mer formats.
Group      a maximal run of consecutive entries with equal keys, in file order.  Nothing is sorted or validated: on an unsound
           database the numbers are defined and meaningless.  DEPARTURE: the reference's loop leaves the database's last entry out
           of its group when the readers complete (:71-79); here it is a member.
LCA        t(g) = the fold of the pairwise LCA over the ids of the members the taxonomy knows (after merged.dmp aliasing); the result
           is a canonical node, for a group of one known id that id's canonical node (NcbiTaxonomy::LCA(vector), which skips absent
           ids, :80).
Bins       distinct[t(g)] += 1 and entries[t(g)] += |g| (all members, unknown ones included): taxon2UniqKmerCount / taxon2Count.
Orphans    a group none of whose ids is known has no LCA (the reference would dereference null): n_orphan_groups += 1,
           n_orphan_entries += |g|, and no bin.
Histogram  size_hist[k], k = 0..39, counts the groups with floor(log2 |g|) == k.
Totals     n_entries, n_groups, max_group, first_max_group (entry index of the first member of the first largest group; NONE if n = 0).
Invariants sum(distinct) + n_orphan_groups == n_groups == sum(size_hist);  sum(entries) + n_orphan_entries == n_entries.
"""
import numpy as np

NONE = (1 << 64) - 1
U64 = np.uint64
HIST = 40
REPORT_FIELDS = ("n_entries", "n_groups", "max_group", "first_max_group", "n_orphan_groups", "n_orphan_entries")
RANK_ORDER = ("root", "superkingdom", "phylum", "class", "order", "family", "genus", "species", "subspecies", "no rank")     # count_common_kmers.cpp:107-109
TSV_HEADER = "original_taxid\trank\tname\tdistinct\tentries\tdistinct_clade\tentries_clade\n"
TSV_NAME = {0: "kmer_lca_report.tsv", 1: "kmer_lca_report_aa.tsv"}


class Tax:
    """a dump-file taxonomy: parent / rank / name by node id (the root is its own parent), aliases = merged.dmp {old id: current id}"""

    def __init__(self, parent, rank, name=None, aliases=None, max_id=None):
        self.parent, self.rank = dict(parent), dict(rank)
        self.name = dict(name) if name else {t: "" for t in parent}
        self.aliases = dict(aliases or {})
        self.max_id = max(list(self.parent) + list(self.aliases)) if max_id is None else max_id

    def canon(self, t):
        """the canonical node of an id, or -1 if the taxonomy does not know it"""
        t = int(t)
        if t in self.parent:
            return t
        t = self.aliases.get(t, -1)
        return t if t in self.parent else -1

    def lineage(self, t):
        out = [t]
        while self.parent[t] != t:
            t = self.parent[t]
            out.append(t)
        return out

    def lca(self, a, b):
        """of two canonical nodes"""
        up = set(self.lineage(a))
        for x in self.lineage(b):
            if x in up:
                return x
        raise ValueError("two roots")


def keys_of(values, level):
    v = np.asarray(values, dtype=U64)
    if level not in (0, 1):
        raise ValueError("level 0 or 1")
    return v >> U64(24) if level == 1 else v


def group_lca(tax, ids):
    """t(g) of a member list, or -1 for an orphan group"""
    acc = -1
    for t in ids:
        c = tax.canon(t)
        if c >= 0:
            acc = c if acc < 0 else tax.lca(acc, c)
    return acc


def inspect(values, info, tax, level=0, info_mask=0xFFFFFFFF):
    """-> (report dict with REPORT_FIELDS and size_hist, distinct u64[max_id + 1], entries u64[max_id + 1])"""
    key = keys_of(values, level)
    ids = (np.asarray(info, dtype=np.uint32) & np.uint32(info_mask)).astype(np.int64)
    n = len(key)
    assert len(ids) == n
    distinct = np.zeros(tax.max_id + 1, U64); entries = np.zeros(tax.max_id + 1, U64)
    hist = np.zeros(HIST, U64)
    R = dict(n_entries=n, n_groups=0, max_group=0, first_max_group=NONE, n_orphan_groups=0, n_orphan_entries=0)
    starts = np.flatnonzero(np.concatenate([[True], key[1:] != key[:-1]])) if n else np.zeros(0, np.int64)
    ends = np.concatenate([starts[1:], [n]]) if n else starts
    for s, e in zip(starts.tolist(), ends.tolist()):
        size = e - s
        t = group_lca(tax, ids[s:e].tolist())
        R["n_groups"] += 1
        hist[size.bit_length() - 1] += U64(1)
        if size > R["max_group"]:
            R["max_group"], R["first_max_group"] = size, s
        if t < 0:
            R["n_orphan_groups"] += 1; R["n_orphan_entries"] += size
        else:
            distinct[t] += U64(1); entries[t] += U64(size)
    R["size_hist"] = [int(x) for x in hist]
    assert int(distinct.sum()) + R["n_orphan_groups"] == R["n_groups"] == sum(R["size_hist"])
    assert int(entries.sum()) + R["n_orphan_entries"] == R["n_entries"]
    return R, distinct, entries


def clade_sums(tax, own):
    """a node's own bin plus its descendants', u64 throughout (the classify report's counts are 32-bit and overflow like the
    reference's: they are not used here)"""
    out = np.array(own, dtype=U64)
    depth = {t: len(tax.lineage(t)) for t in tax.parent}
    for t in sorted(tax.parent, key=lambda t: -depth[t]):
        if tax.parent[t] != t:
            out[tax.parent[t]] += out[t]
    return out


def report_text(tax, distinct, entries, original_id=None):
    """the TSV: the header, then one row per canonical node with a non-zero clade sum, ascending internal id"""
    dc, ec = clade_sums(tax, distinct), clade_sums(tax, entries)
    rows = [TSV_HEADER]
    for t in sorted(tax.parent):
        if dc[t] or ec[t]:
            o = original_id(t) if original_id else t
            rows.append(f"{o}\t{tax.rank[t]}\t{tax.name[t]}\t{int(distinct[t])}\t{int(entries[t])}\t{int(dc[t])}\t{int(ec[t])}\n")
    return "".join(rows)


def summary_text(tax, distinct, entries, n_groups):
    """the by-rank summary with the reference's wording (:127-158): ranks in the reference's order, taxon 1 counted as `root`, then
    DEPARTURE every other rank that has a count, alphabetically (the reference drops those silently)"""
    def by_rank(arr):
        out = {}
        for t in tax.parent:
            if arr[t]:
                r = "root" if t == 1 else tax.rank[t]
                out[r] = out.get(r, 0) + int(arr[t])
        order = [r for r in RANK_ORDER if r in out] + sorted(r for r in out if r not in RANK_ORDER)
        return "".join(f"{r}: {out[r]}\n" for r in order)
    return ("Common k-mers count by rank:\n" + by_rank(entries) + f"Total distinct common k-mers count: {n_groups}\n"
            "Distinct common k-mers count by rank:\n" + by_rank(distinct))


def brute_force(values, info, tax, level=0, info_mask=0xFFFFFFFF):
    """the same bins by another route, for lists whose equal keys are contiguous: a dict of member lists per key"""
    key = keys_of(values, level).tolist()
    ids = (np.asarray(info, dtype=np.uint32) & np.uint32(info_mask)).tolist()
    members = {}
    for k, t in zip(key, ids):
        members.setdefault(k, []).append(t)
    distinct = np.zeros(tax.max_id + 1, U64); entries = np.zeros(tax.max_id + 1, U64)
    orphan = [0, 0]
    for k, m in members.items():
        known = [tax.canon(t) for t in m if tax.canon(t) >= 0]
        if not known:
            orphan[0] += 1; orphan[1] += len(m)
            continue
        common = None
        for c in known:
            line = tax.lineage(c)
            common = line if common is None else [x for x in common if x in set(line)]
        distinct[common[0]] += U64(1); entries[common[0]] += U64(len(m))
    return distinct, entries, orphan, len(members)
