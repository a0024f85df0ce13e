"""The selection rule of the filtered merge (mtb_merge_databases_filtered; metabuli_amd/csrc/host/clade_filter.h) restated in plain
Python over a synth.Taxonomy: parents, ranks, aliases -> keep[], the refusals, and the statistics the call reports.  Nothing is
memoised here: every node walks its own lineage.

  species key of an id   = the node at which a climb from the id first meets species rank or above (Taxonomy::at_rank in host_db.h:
                           "no rank" and unknown ranks count as below everything; the root and ids the taxonomy lacks have key 0)
  key s is kept          iff (select is empty or a selected taxon is s or an ancestor of s) and no excluded taxon is s or an ancestor
  key 0 is kept          iff select is empty and the root is not excluded
  refused                both lists empty; an id the taxonomy does not know (after aliasing); an id strictly below its species key
"""
import numpy as np

RANKS = {"forma": 1, "varietas": 2, "subspecies": 3, "species": 4, "species subgroup": 5, "species group": 6, "subgenus": 7, "genus": 8, "subtribe": 9,
         "tribe": 10, "subfamily": 11, "family": 12, "superfamily": 13, "parvorder": 14, "infraorder": 15, "suborder": 16, "order": 17, "superorder": 18,
         "infraclass": 19, "subclass": 20, "class": 21, "superclass": 22, "subphylum": 23, "phylum": 24, "superphylum": 25, "subkingdom": 26,
         "kingdom": 27, "superkingdom": 28, "domain": 28}
SPECIES = RANKS["species"]


class Refusal(ValueError):
    """kind: 'no_ids', 'unknown' or 'below_species'; taxid: the id as it was listed (None for 'no_ids')"""

    def __init__(self, kind, taxid=None):
        super().__init__(f"{kind} {taxid}")
        self.kind, self.taxid = kind, taxid


def canonical(tax, aliases, t):
    """the node an id names: itself, or the target of its merged.dmp line; None if the taxonomy does not know it"""
    if t in tax.parent:
        return t
    a = (aliases or {}).get(t)
    return a if a in tax.parent else None


def max_id(tax, aliases):
    return max([1] + list(tax.parent) + list(tax.parent.values()) + list(aliases or {}) + list((aliases or {}).values()))


def is_root(tax, c):
    return tax.parent[c] == c


def species_key(tax, aliases, t):
    c = canonical(tax, aliases, t)
    if t == 0 or t == 1 or c is None:
        return 0
    cur = c
    for _ in range(30):
        if RANKS.get(tax.rank[cur], -1) >= SPECIES:
            return cur
        cur = tax.parent[cur]
    return t


def _listed(tax, aliases, ids):
    out = []
    for t in ids:
        c = canonical(tax, aliases, int(t))
        if c is None:
            raise Refusal("unknown", int(t))
        if not is_root(tax, c) and species_key(tax, aliases, c) != c:
            raise Refusal("below_species", int(t))
        out.append(c)
    return out


def keep_table(tax, aliases, select, exclude):
    """-> uint8 array over [0, max_id], indexed by species key; raises Refusal"""
    select, exclude = list(select or []), list(exclude or [])
    if not select and not exclude:
        raise Refusal("no_ids")
    sel, exc = set(_listed(tax, aliases, select)), set(_listed(tax, aliases, exclude))
    keep = np.zeros(max_id(tax, aliases) + 1, np.uint8)
    for t in range(1, len(keep)):
        c = canonical(tax, aliases, t)
        if c is None:
            continue
        line = set(tax.lineage(c))
        keep[t] = (not sel or bool(line & sel)) and not (line & exc)
    keep[0] = not sel and not any(is_root(tax, c) for c in exc)
    return keep


def record_keys(tax, aliases, taxids):
    """species key of every record id"""
    return np.array([species_key(tax, aliases, int(t)) for t in taxids], np.int64)


def statistics(tax, aliases, select, exclude, taxids):
    """what mtb_filter_stats reports for records with these ids (one record per entry of `taxids`): a dict"""
    keep = keep_table(tax, aliases, select, exclude)
    keys = record_keys(tax, aliases, taxids)
    met = sorted(set(int(k) for k in keys))
    under = set()
    for s in met:
        if s:
            under.update(tax.lineage(canonical(tax, aliases, s)))
    unmatched = []
    for t in list(select or []) + list(exclude or []):
        c = canonical(tax, aliases, int(t))
        if c not in under and not (0 in met and is_root(tax, c)):
            unmatched.append(int(t))
    return dict(n_records_in=len(keys), n_records_kept=int(keep[keys].astype(bool).sum()),
                n_species_kept=sum(1 for s in met if keep[s]), n_species_dropped=sum(1 for s in met if not keep[s]),
                n_unmatched=len(unmatched), first_unmatched=unmatched[0] if unmatched else 0)


# ---------------------------------------------------------------------------------------------------------------------
# the toy tree of the CPU tests: three genera, strains of three kinds of rank, two aliases
# ---------------------------------------------------------------------------------------------------------------------
def toy_tree():
    """1 root - 2 Bacteria - genus 10 {species 11 {111, 112 (no rank)}, species 12}, genus 20 {species 21 {211 (strain)}, species 22},
    genus 30 {species 31 {311 (subspecies)}}; merged.dmp: 900 -> 12, 901 -> 111.  -> (synth.Taxonomy, aliases)"""
    from metabuli_amd import synth
    tax = synth.Taxonomy()
    tax.add(1, 1, "no rank", "root"); tax.add(2, 1, "superkingdom", "Bacteria")
    for g in (10, 20, 30):
        tax.add(g, 2, "genus", f"G{g}")
    for s, g in ((11, 10), (12, 10), (21, 20), (22, 20), (31, 30)):
        tax.add(s, g, "species", f"s{s}")
    tax.add(111, 11, "no rank", "strain111"); tax.add(112, 11, "no rank", "strain112")
    tax.add(211, 21, "strain", "strain211"); tax.add(311, 31, "subspecies", "subsp311")
    return tax, {900: 12, 901: 111}


def write_taxonomy(tax, aliases, d):
    """nodes.dmp / names.dmp / merged.dmp of the tree in directory d"""
    import os
    tax.write(d)
    with open(os.path.join(d, "merged.dmp"), "w") as f:
        for a, t in sorted((aliases or {}).items()):
            f.write(f"{a}\t|\t{t}\t|\n")
    return d
