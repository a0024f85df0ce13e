"""Test infrastructure: an independent numpy restatement of what mtb_builder_finish computes (include/mtb.h, "database build
and merge"), over the dump files a test wrote.  No library code: lexsort, group boundaries, parent-walk LCA.

    s = species of the taxid (first node of rank `species` on the way to the root)
    order by (value, s, taxid); one entry per distinct (value, s); info = LCA of the group's taxids (canonical ids:
    merged.dmp aliases resolved, so a group of one gives the alias target)
"""
import os

import numpy as np


class DumpTaxonomy:
    def __init__(self, taxdir):
        self.parent, self.rank, self.alias = {}, {}, {}
        for line in open(os.path.join(taxdir, "nodes.dmp")):
            c = [x.strip() for x in line.split("|")]
            if len(c) >= 3 and c[0]:
                self.parent[int(c[0])] = int(c[1]); self.rank[int(c[0])] = c[2]
        mp = os.path.join(taxdir, "merged.dmp")
        if os.path.exists(mp):
            for line in open(mp):
                c = [x.strip() for x in line.split("|")]
                if len(c) >= 2 and c[0]:
                    self.alias[int(c[0])] = int(c[1])

    def canon(self, t):
        t = int(t)
        if t in self.parent:
            return t
        t = self.alias[t]                      # KeyError: an id the taxonomy does not know (the builder refuses those)
        assert t in self.parent
        return t

    def lineage(self, t):
        t = self.canon(t)
        out = [t]
        while self.parent[t] != t:
            t = self.parent[t]
            out.append(t)
        return out

    def species(self, t):
        for x in self.lineage(t):
            if self.rank[x] == "species":
                return x
        raise AssertionError(f"taxid {t} is not at or below a species: outside what this restatement covers")

    def lca(self, ids):
        ids = [self.canon(t) for t in ids]
        common = self.lineage(ids[0])
        for t in ids[1:]:
            s = set(self.lineage(t))
            common = [x for x in common if x in s]
        return common[0]                       # lineages run leaf -> root: the first common node is the lowest


def spec_finish(values, taxids, taxdir):
    """-> (values u64, info u32) of the index mtb_builder_finish must return for these records"""
    tax = DumpTaxonomy(taxdir)
    values = np.asarray(values, dtype=np.uint64); taxids = np.asarray(taxids, dtype=np.int32)
    sp_of = {int(t): tax.species(t) for t in np.unique(taxids)}
    sp = np.array([sp_of[int(t)] for t in taxids], dtype=np.int64)
    order = np.lexsort((taxids, sp, values))
    v, t, s = values[order], taxids[order], sp[order]
    head = np.ones(len(v), bool)
    head[1:] = (v[1:] != v[:-1]) | (s[1:] != s[:-1])
    starts = np.flatnonzero(head)
    ends = np.append(starts[1:], len(v))
    info = np.zeros(len(starts), np.uint32)
    for g, (a, b) in enumerate(zip(starts, ends)):
        info[g] = tax.lca(np.unique(t[a:b]))
    return v[starts].copy(), info, dict(order=order, starts=starts, ends=ends)
