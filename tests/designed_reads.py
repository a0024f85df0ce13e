"""Designed reads: a hand-made taxonomy, genomes that are the reads themselves with chosen edits, and per case the precondition -- as code
over what the CPU side computed -- that says which edge of the scoring rules the case sits on.

TEST INFRASTRUCTURE ONLY (a helper module, not a conftest).  The CPU side is the oracle's matches (oracle/oracle.cpp) scored once more by
tests/bruteforce.py::ReadScorer, whose trace (`ReadScorer.last`: emitted paths with depth / multi_pred / tied_chains, the combine trace,
the per-species scores) is what the preconditions read.  tests/test_designed_reads_spec.py asserts the preconditions and the agreement of
oracle, ReadScorer and the host build of the kernel arithmetic; tests/test_gpu_designed_reads.py runs every case through every scorer.

Every locus is drawn from a seeded generator (SEED below, one stream per case name); all cases share ONE world (one database, syncmer
mode), so a GPU test opens one index.  A strain's genome is the concatenation of the loci the cases file under it, separated by runs of N
(no window spans two loci).  A case that needs a read at an exact edge (a path count, a chain depth, a used length) cuts a longer read
base by base at its end against the finished database until the CPU side reports the edge -- the way `World.tuned` of
test_gpu_scorer_tiers.py lands a read in a metamer band."""
from __future__ import annotations

import os
import zlib

import numpy as np

import bruteforce as bf
from helpers import build_toy_db, default_params

SEED = 20240611
SYNCMER, SMER_LEN = 1, 5
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
N = ord("N")

# ---------------------------------------------------------------------------------------------- taxonomy (fixed, by hand)
ROOT, BACTERIA, EUKARYOTA = 1, 2, 3
GEN_A, GEN_B, GEN_C, GEN_E = 10, 11, 12, 13
SP_A1, SP_A2, SP_A3, SP_B1, SP_C1, SP_E1, SP_E2 = 20, 21, 22, 23, 24, 25, 26
SUB_A1 = 30                                  # A1 has a three-level tail: species -> subspecies -> strains
ST_A1a, ST_A1b = 31, 32
ST_A2a, ST_A2b = 34, 35                      # A2: two sibling strains
ST_A3acc, ST_A3b = 36, 37                    # A3: one child of the rank accession_level = 2 removes, one strain
ST_B1, ST_C1, ST_E1, ST_E2 = 38, 39, 40, 41
TAXONOMY = [
    (ROOT, ROOT, "no rank", "root"), (BACTERIA, ROOT, "superkingdom", "Bacteria"), (EUKARYOTA, ROOT, "superkingdom", "Eukaryota"),
    (GEN_A, BACTERIA, "genus", "Aa"), (GEN_B, BACTERIA, "genus", "Bb"), (GEN_C, BACTERIA, "genus", "Cc"), (GEN_E, EUKARYOTA, "genus", "Ee"),
    (SP_A1, GEN_A, "species", "Aa one"), (SP_A2, GEN_A, "species", "Aa two"), (SP_A3, GEN_A, "species", "Aa three"),
    (SP_B1, GEN_B, "species", "Bb one"), (SP_C1, GEN_C, "species", "Cc one"), (SP_E1, GEN_E, "species", "Ee one"), (SP_E2, GEN_E, "species", "Ee two"),
    (SUB_A1, SP_A1, "subspecies", "Aa one sub"), (ST_A1a, SUB_A1, "strain", "Aa one sub a"), (ST_A1b, SUB_A1, "strain", "Aa one sub b"),
    (ST_A2a, SP_A2, "strain", "Aa two a"), (ST_A2b, SP_A2, "strain", "Aa two b"),
    (ST_A3acc, SP_A3, "accession", "Aa three acc"), (ST_A3b, SP_A3, "strain", "Aa three b"),
    (ST_B1, SP_B1, "strain", "Bb one a"), (ST_C1, SP_C1, "strain", "Cc one a"), (ST_E1, SP_E1, "strain", "Ee one a"), (ST_E2, SP_E2, "strain", "Ee two a"),
]


def taxonomy():
    from metabuli_amd import synth
    t = synth.Taxonomy()
    for row in TAXONOMY:
        t.add(*row)
    return t


# ---------------------------------------------------------------------------------------------- edit primitives on base arrays
def rng_of(name):
    return np.random.default_rng([SEED, zlib.crc32(name.encode())])


def locus(rng, n):
    return ACGT[rng.integers(0, 4, size=n)].copy()


def substitute(seq, positions):
    """another base at every given position (A->C->G->T->A)"""
    out = seq.copy()
    for p in np.atleast_1d(positions):
        out[p] = ACGT[(int(np.searchsorted(ACGT, out[p])) + 1) % 4]
    return out


def scramble(seq, lo, hi, rng):
    """fresh bases on [lo, hi), each different from the one it replaces"""
    out = seq.copy()
    step = rng.integers(1, 4, size=hi - lo)
    out[lo:hi] = ACGT[(np.searchsorted(ACGT, out[lo:hi]) + step) % 4]
    return out


def insert(seq, pos, bases):
    return np.concatenate([seq[:pos], np.asarray(bases, np.uint8), seq[pos:]])


def delete(seq, pos, n):
    return np.concatenate([seq[:pos], seq[pos + n:]])


def mask_n(seq, positions):
    out = seq.copy()
    out[np.atleast_1d(positions)] = N
    return out


def synonymous_variant(seq, frame, every, T=None, skip=0, pick=0):
    """`seq` with the third base of every `every`-th codon of `frame` replaced by the `pick`-th other base that keeps the amino acid
    (tables of tests/golden/ref_codon_tables.txt; a codon with fewer such bases stays); returns (variant, codon starts changed)"""
    T = T or bf.ref_tables()
    out, changed = seq.copy(), []
    for j, c in enumerate(range(frame, len(seq) - 2, 3)):
        if j % every != skip % every:
            continue
        a, b, x = (int(T["fwd"][v]) for v in seq[c:c + 3])
        alts = [alt for alt in range(4) if alt != x and T["aa"][a, b, alt] == T["aa"][a, b, x]]
        if pick < len(alts):
            out[c + 2] = next(ch for ch in ACGT if int(T["fwd"][ch]) == alts[pick])
            changed.append(c)
    return out, changed


class Batch:
    """reads of one case: single (seq_mode 1), paired (2) or long (3)"""

    def __init__(self, reads, seq_mode, names=None):
        self.seq_mode = seq_mode
        self.reads = [(r, None) if isinstance(r, np.ndarray) else r for r in reads]
        assert all((m2 is not None) == (seq_mode == 2) for _, m2 in self.reads)
        self.names = names or [str(i) for i in range(len(self.reads))]
        self.b1, self.o1 = self._cat([a for a, _ in self.reads])
        self.b2, self.o2 = self._cat([b for _, b in self.reads]) if seq_mode == 2 else (None, None)

    @staticmethod
    def _cat(seqs):
        offs = np.zeros(len(seqs) + 1, np.uint64)
        offs[1:] = np.cumsum([len(s) for s in seqs])
        return (np.concatenate(seqs).astype(np.uint8) if offs[-1] else np.zeros(0, np.uint8)), offs

    @property
    def n(self):
        return len(self.reads)

    def index(self, name):
        return self.names.index(name)


class Case:
    """name; genomes = {strain taxid: [locus, ...]}; `finish(world)` sets self.batch (it may cut reads against the finished database);
    runs = [(label, parameter overrides)], every run classifies the same batch; precondition(world, {label: Analysis}) asserts the edge."""
    seq_mode = 1
    runs = [("default", {})]

    def __init__(self):
        self.name = type(self).__name__
        self.rng = rng_of(self.name)
        self.genomes = {}
        self.batch = None

    def place(self, strain, seq):
        self.genomes.setdefault(strain, []).append(np.asarray(seq, np.uint8))

    def design(self):
        raise NotImplementedError

    def finish(self, W):
        pass

    def precondition(self, W, an):
        raise NotImplementedError


class Analysis:
    """the CPU side of one run of one case: the oracle's full answer and ReadScorer's answer + trace per read"""

    def __init__(self, W, batch, overrides):
        self.p = W.oparams(batch.seq_mode, **overrides)
        self.ref = W.orc.classify(W.db(batch.seq_mode), W.tax, self.p, batch.b1, batch.o1, batch.b2, batch.o2)
        p = self.p
        sc = bf.ReadScorer(W.world.tax, p.syncmer, p.smer_len, p.seq_mode, kmer_format=p.kmer_format, min_cons_cnt=p.min_cons_cnt,
                           min_cons_cnt_euk=p.min_cons_cnt_euk, min_score=p.min_score, min_sp_score=p.min_sp_score, tie_ratio=p.tie_ratio,
                           accession_level=p.accession_level, eukaryota=EUKARYOTA)
        self.scorer = sc
        m = self.ref["matches"]
        rd = ((m["qinfo"] >> np.uint64(32)) & np.uint64(0x1FFFFFFF)).astype(np.int64)
        self.by_read = [[] for _ in range(batch.n)]
        for rec, r in zip(m.tolist(), rd.tolist()):
            self.by_read[r - 1].append(tuple(rec[:6]))
        k = self.ref["kmers"]
        kr = ((k["qinfo"] >> np.uint64(32)) & np.uint64(0x1FFFFFFF)).astype(np.int64)
        self.n_metamers = np.bincount(kr, minlength=batch.n + 1)[1:]
        self.reads = []
        ro = self.ref["results"]
        for i in range(batch.n):
            cls, score, is_cls, taxcnt = sc.score_read(self.by_read[i], int(ro["qlen"][i]), int(ro["qlen2"][i]))      # TooManyChains propagates: a condition
            last = sc.last
            ms = self.by_read[i]
            groups = {}
            for q in ms:
                groups[(q[2], q[0] >> 61, q[0] & 0xFFFFFFFF)] = groups.get((q[2], q[0] >> 61, q[0] & 0xFFFFFFFF), 0) + 1
            self.reads.append(dict(cls=cls, score=np.float32(score), is_cls=is_cls, taxcnt=taxcnt, species=last["species"], tied=last["tied"],
                                   n_paths=sum(len(s["paths"]) for s in last["species"]), n_matches=len(ms),
                                   n_matched_metamers=len({q[0] for q in ms}), s2=any(c > 1 for c in groups.values())))

    def paths(self, i, species=None):
        return [p for s in self.reads[i]["species"] if species in (None, s["species"]) for p in s["paths"]]

    def trace(self, i):
        return [t for s in self.reads[i]["species"] for t in s["trace"]]

    def species_score(self, i, species):
        return next(s for s in self.reads[i]["species"] if s["species"] == species)


def f32_neighbours(x):
    x = np.float32(x)
    return np.nextafter(x, np.float32(-np.inf)), x, np.nextafter(x, np.float32(np.inf))


class DesignedWorld:
    """all cases' loci in one database; `analysis(case, label)` is computed once and shared, unchanged, among the tests"""

    def __init__(self, orc, dbdir, cases=None):
        from metabuli_amd import synth
        self.orc = orc
        self.cases = [c() for c in (cases or CASES)]
        tax = taxonomy()
        per_strain = {}
        for c in self.cases:
            c.design()
            for strain, loci in c.genomes.items():
                assert tax.rank[strain] in ("strain", "accession"), strain
                for s in loci:
                    per_strain.setdefault(strain, []).extend([s, np.full(32, N, np.uint8)])
        genomes = [(t, np.concatenate(per_strain[t])) for t in sorted(per_strain)]
        self.world = synth.World(tax, genomes, [t for t, r in tax.rank.items() if r == "species"])
        self.dbdir = str(dbdir)
        os.makedirs(self.dbdir, exist_ok=True)
        self.values, self.taxids = build_toy_db(orc, self.world, self.oparams(1), self.dbdir)
        self.tax = orc.load_taxonomy(os.path.join(self.dbdir, "taxonomy"))
        self._dbs, self._an = {}, {}
        for c in self.cases:
            c.finish(self)
            assert c.batch is not None and c.batch.seq_mode == c.seq_mode, c.name

    def oparams(self, seq_mode, **kw):
        return default_params(seq_mode=seq_mode, syncmer=SYNCMER, smer_len=SMER_LEN, **kw)

    def db(self, seq_mode):
        if seq_mode not in self._dbs:
            self._dbs[seq_mode] = self.orc.open_db(self.dbdir, self.tax, self.oparams(seq_mode))
        return self._dbs[seq_mode]

    def case(self, name):
        return next(c for c in self.cases if c.name == name)

    def analysis(self, case, label):
        key = (case.name, label)
        if key not in self._an:
            self._an[key] = Analysis(self, case.batch, dict(case.runs)[label])
        return self._an[key]

    def analyses(self, case):
        return {label: self.analysis(case, label) for label, _ in case.runs}

    def probe(self, reads, seq_mode, **overrides):
        """an Analysis of a trial batch (used by `finish` while a read is cut to its edge)"""
        return Analysis(self, Batch(reads, seq_mode), overrides)


CASES = []


def case(cls):
    CASES.append(cls)
    return cls


def revcomp(seq):
    from metabuli_amd import synth
    return synth.revcomp(seq)


def prefixes(W, read, lengths, seq_mode=1, **overrides):
    """one Analysis over the prefixes of `read` of the given lengths"""
    lengths = list(lengths)
    return lengths, W.probe([read[:n].copy() for n in lengths], seq_mode, **overrides)


# ============================================================================================== 1. ties (a17)
@case
class Ties(Case):
    """the same locus in two species of one genus / of two genera / of the two domains: the LCA of the tied species.  With tie_ratio = 1
    the cut is the best score itself: only `>=` keeps the equal scores tied"""
    runs = [("default", {}), ("ratio1", dict(tie_ratio=1.0))]
    PLACES = [("genus", (ST_A1a, ST_A2a), GEN_A), ("bacteria", (ST_A1a, ST_B1), BACTERIA), ("root", (ST_A1a, ST_E1), ROOT),
              ("genus3", (ST_A1b, ST_A2b, ST_A3b), GEN_A)]

    def design(self):
        self.loci = [locus(self.rng, 150) for _ in self.PLACES]
        for s, (_, strains, _) in zip(self.loci, self.PLACES):
            for t in strains:
                self.place(t, s)

    def finish(self, W):
        self.batch = Batch(self.loci, 1, [n for n, _, _ in self.PLACES])

    def precondition(self, W, an):
        for a in an.values():
            for i, (name, strains, lca) in enumerate(self.PLACES):
                r = a.reads[i]
                assert len(r["tied"]) == len(strains) and len({float(s) for _, s in r["tied"]}) == 1, (name, r["tied"])
                assert r["cls"] == lca and r["is_cls"] == 1 and r["taxcnt"] == {}, (name, r["cls"])


def sum_groupings(scores):
    """the three sums fp32 addition can give for three numbers: (a + b) + c in list order, (b + c) + a, (a + c) + b"""
    f = np.float32
    a, b, c = (f(x) for x in scores)
    return [f(f(x + y) + z).view(np.uint32).item() for x, y, z in ((a, b, c), (b, c, a), (a, c, b))]


def order_hits(a):
    """per other grouping, the reads of an Analysis whose three tied, different scores sum to other bits than in list order"""
    out = {1: [], 2: []}
    for i, r in enumerate(a.reads):
        sc = [s for _, s in r["tied"]]
        if len(sc) == 3 and len({float(s) for s in sc}) == 3:
            g = sum_groupings(sc)
            for k in (1, 2):
                if g[k] != g[0]:
                    out[k].append(i)
    return out


@case
class TieSum(Case):
    """three tied species with three different scores whose fp32 sum depends on the order of the additions (list order = rising species id)"""
    runs = [("ratio0.7", dict(tie_ratio=0.7))]
    N_CAND = 36

    def design(self):
        self.loci = []
        for j in range(self.N_CAND):
            s = locus(self.rng, 150 + j % 3)
            self.loci.append(s)
            for strain, nsub in ((ST_A1a, 1 + j % 2), (ST_A2a, 2 + j % 3), (ST_A3b, 3 + j % 4)):
                self.place(strain, substitute(s, 2 + 3 * self.rng.choice(48, size=nsub, replace=False)))      # third bases of frame 0

    def finish(self, W):
        self.batch = Batch(self.loci, 1)

    def precondition(self, W, an):
        a = an["ratio0.7"]
        hits = order_hits(a)
        assert hits[1] and hits[2], f"no read whose three tied scores sum differently in another order: {hits}"
        for i in hits[1] + hits[2]:
            assert a.reads[i]["cls"] == GEN_A and [s for s, _ in a.reads[i]["tied"]] == [SP_A1, SP_A2, SP_A3]


@case
class TieRatio(Case):
    """two scoring species; tie_ratio on either side of where sc2 >= float32(best * tie_ratio) flips.  Below 1 a step of tie_ratio moves
    the product by less than a step of sc2, so the last ratio that ties gives the product sc2 itself: equality, which `>` would miss"""

    def design(self):
        self.read = locus(self.rng, 150)
        self.place(ST_A1a, self.read)
        self.place(ST_B1, substitute(self.read, [32, 92]))

    def finish(self, W):
        self.batch = Batch([self.read], 1)
        a = W.probe([self.read], 1, tie_ratio=0.0)
        sc = dict(a.reads[0]["tied"])
        best, sc2 = max(sc.values()), min(sc.values())
        assert len(sc) == 2 and np.float32(0) < sc2 < best, sc
        t = np.float32(sc2 / best)
        while np.float32(best * t) <= sc2:
            t = np.nextafter(t, np.float32(2))
        while np.float32(best * t) > sc2:
            t = np.nextafter(t, np.float32(0))
        self.t_in, self.t_out = t, np.nextafter(t, np.float32(2))
        self.best, self.sc2 = best, sc2
        self.runs = [("ratio_in", dict(tie_ratio=float(self.t_in))), ("ratio_out", dict(tie_ratio=float(self.t_out)))]

    def precondition(self, W, an):
        assert self.sc2 == np.float32(self.best * self.t_in) and not self.sc2 >= np.float32(self.best * self.t_out)
        assert np.nextafter(self.t_in, np.float32(2)) == self.t_out
        assert an["ratio_in"].reads[0]["cls"] == BACTERIA and len(an["ratio_in"].reads[0]["tied"]) == 2
        assert an["ratio_out"].reads[0]["cls"] == ST_A1a and len(an["ratio_out"].reads[0]["tied"]) == 1


# ============================================================================================== 2. thresholds
@case
class Thresholds(Case):
    """min_score / min_sp_score at the read's fp32 score and at its two fp32 neighbours"""

    def design(self):
        self.read = locus(self.rng, 150)
        self.place(ST_C1, substitute(self.read, [62]))

    def finish(self, W):
        self.batch = Batch([self.read], 1)
        self.score = W.probe([self.read], 1).reads[0]["score"]
        lo, eq, hi = (float(x) for x in f32_neighbours(self.score))
        self.runs = [("min_score_below", dict(min_score=lo)), ("min_score_equal", dict(min_score=eq)), ("min_score_above", dict(min_score=hi)),
                     ("min_sp_below", dict(min_sp_score=lo)), ("min_sp_equal", dict(min_sp_score=eq)), ("min_sp_above", dict(min_sp_score=hi))]

    def precondition(self, W, an):
        assert np.float32(0) < self.score < np.float32(1)
        for label, want in (("min_score_below", ST_C1), ("min_score_equal", ST_C1), ("min_score_above", 0),
                            ("min_sp_below", ST_C1), ("min_sp_equal", ST_C1), ("min_sp_above", GEN_C)):
            r = an[label].reads[0]
            assert r["cls"] == want and r["is_cls"] == (want != 0), (label, r["cls"])
            if want:
                assert r["score"].view(np.uint32) == self.score.view(np.uint32), label


# ============================================================================================== 3. cap at 1.0
@case
class Cap(Case):
    """species scores at the cap: a raw score of exactly 1.0, raw scores above 1.0 (a frame change lets two paths cover more than the used
    length), and two species that tie at the capped 1.0"""
    N_CAND = 8

    def design(self):
        self.exact = locus(self.rng, 150)
        self.place(ST_C1, self.exact)
        self.over = [locus(self.rng, 150) for _ in range(self.N_CAND)]
        for j, s in enumerate(self.over):
            g = delete(s, 75 + j, 1) if j % 2 else insert(s, 75 + j, [ACGT[j % 4]])
            self.place(ST_B1, g)
            self.place(ST_A2a, g)

    def finish(self, W):
        self.batch = Batch([self.exact] + self.over, 1)

    def precondition(self, W, an):
        a = an["default"]
        s = a.species_score(0, SP_C1)
        assert s["raw"] == np.float32(1.0) and a.reads[0]["score"] == np.float32(1.0) and a.reads[0]["cls"] == ST_C1
        over = [i for i in range(1, len(a.reads)) if len(a.reads[i]["species"]) == 2 and all(x["raw"] > np.float32(1.0) for x in a.reads[i]["species"])]
        assert over, "no read whose raw species score exceeds 1"
        for i in over:
            r = a.reads[i]
            assert [float(x) for _, x in r["tied"]] == [1.0, 1.0] and r["score"] == np.float32(1.0) and r["cls"] == BACTERIA


# ============================================================================================== 4. depth (a15)
@case
class Depth(Case):
    """one sequence under a bacterial and a eukaryotic species; prefixes whose best chain is exactly d codons deep, for the d on either side
    of min_cons_cnt (4; 6) and min_cons_cnt_euk (9; 12); min_cons_cnt = 1 lets single matches stand as paths"""
    runs = [("default", {}), ("mcc1", dict(min_cons_cnt=1)), ("mcc6_12", dict(min_cons_cnt=6, min_cons_cnt_euk=12))]
    DEPTHS = [3, 4, 5, 6, 8, 9, 11, 12]
    N_CAND = 6

    def design(self):
        self.loci = [locus(self.rng, 110) for _ in range(self.N_CAND)]
        for s in self.loci:
            self.place(ST_B1, s)
            self.place(ST_E1, s)

    @staticmethod
    def best_depth(a, i):
        return max((p["depth"] for p in a.paths(i)), default=0)

    def finish(self, W):
        reads, names = [], []
        found = {}
        for s in self.loci:
            ns, a = prefixes(W, s, range(len(s), 30, -1), min_cons_cnt=1, min_cons_cnt_euk=1)
            by_depth = {}
            for j, n in enumerate(ns):
                by_depth.setdefault(self.best_depth(a, j), n)          # the longest prefix of that depth
            for lo in self.DEPTHS[0::2]:
                if lo in by_depth and lo + 1 in by_depth and lo not in found:
                    found[lo] = (s[:by_depth[lo]].copy(), s[:by_depth[lo + 1]].copy())
        assert sorted(found) == self.DEPTHS[0::2], sorted(found)
        for lo in self.DEPTHS[0::2]:
            reads += list(found[lo]); names += [f"d{lo}", f"d{lo + 1}"]
        for j, s in enumerate(self.loci[:3]):           # a lone window before a gap of N: a single match that links to nothing
            lone = s.copy(); lone[27:60] = N
            reads.append(lone); names.append(f"lone{j}")
        self.batch = Batch(reads, 1, names)

    def precondition(self, W, an):
        probe = W.probe([r for r, _ in self.batch.reads], 1, min_cons_cnt=1, min_cons_cnt_euk=1)
        for i, d in enumerate(self.DEPTHS):
            assert self.best_depth(probe, i) == d, (d, self.best_depth(probe, i))
        for label, mcc, euk in (("default", 4, 9), ("mcc1", 1, 9), ("mcc6_12", 6, 12)):
            a = an[label]
            for i, d in enumerate(self.DEPTHS):
                sp = {s["species"] for s in a.reads[i]["species"]}
                assert sp == ({SP_B1} if d >= mcc else set()) | ({SP_E1} if d >= euk else set()), (label, d, sp)
                want = 0 if not sp else ROOT if len(sp) == 2 else ST_B1
                assert a.reads[i]["cls"] == want, (label, d, a.reads[i]["cls"])
        lone = range(len(self.DEPTHS), self.batch.n)
        assert any(p["depth"] == 1 for i in lone for p in an["mcc1"].paths(i)), "no single-match path under min_cons_cnt = 1"
        assert not any(p["depth"] < 4 for i in lone for p in an["default"].paths(i))


# ============================================================================================== 5. many paths
class _Islands(Case):
    """a genome equal to the read with 12 bases scrambled every 60: every island of 48 bases emits a path per frame.  The reads that are
    to stay on the slot path carry N over the scrambled stretches (no metamers there), the others are the plain locus."""
    PERIOD, ISLAND = 60, 48

    def island_locus(self, n, strains):
        s = locus(self.rng, n)
        g = s.copy()
        for lo in range(self.ISLAND, n, self.PERIOD):
            g = scramble(g, lo, min(lo + self.PERIOD - self.ISLAND, n), self.rng)
        for t in strains:
            self.place(t, g)
        return s

    def masked(self, s):
        out = s.copy()
        for lo in range(self.ISLAND, len(s), self.PERIOD):
            out[lo:lo + self.PERIOD - self.ISLAND] = N
        return out

    def cut_to_paths(self, W, read, targets, seq_mode=1, mate1=None, have=0):
        """{target: piece of `read` (of mate 2 when mate1 is given, which emits `have` paths alone) that emits exactly `target` paths}: the
        prefixes around the expected length (six paths an island; the count moves with every third base), cut base by base at the end;
        where two frames gain their path at one base, bases go from the start too"""
        out = {}
        for off in range(0, self.ISLAND):
            piece = read[off:]
            for t in targets:
                if t in out:
                    continue
                mid = (t - have) * self.PERIOD // 6
                lens = [n for n in range(min(len(piece), mid + 45), max(40, mid - 45), -1)]
                a = W.probe([piece[:n].copy() if mate1 is None else (mate1, piece[:n].copy()) for n in lens], seq_mode)
                hit = [n for j, n in enumerate(lens) if a.reads[j]["n_paths"] == t]
                if hit:
                    out[t] = piece[:hit[0]].copy()
            if len(out) == len(targets):
                return out
        raise AssertionError(f"no piece of the read emits {sorted(set(targets) - set(out))} paths")


@case
class ManyPaths(_Islands):
    """one species emitting exactly 16, 17 (the reference's std::sort regime starts above 16), 64 and 65 (the fast scorer's S3) paths; every
    read within the slot path's 336 metamers and 128 position buckets, one match per metamer: S3 alone decides who scores the read"""
    TARGETS = [16, 17, 64, 65]

    def design(self):
        self.locus = self.island_locus(1440, [ST_C1])

    def finish(self, W):
        m = self.masked(self.locus)
        cut = self.cut_to_paths(W, m, self.TARGETS)
        self.batch = Batch([cut[t] for t in self.TARGETS], 1, [f"p{t}" for t in self.TARGETS])

    def precondition(self, W, an):
        a = an["default"]
        for i, t in enumerate(self.TARGETS):
            assert a.reads[i]["n_paths"] == t and len(a.reads[i]["species"]) == 1 and a.reads[i]["cls"] == ST_C1, (t, a.reads[i]["n_paths"])
            assert a.n_metamers[i] <= 336 and a.reads[i]["n_matches"] == a.reads[i]["n_matched_metamers"], (t, a.n_metamers[i])
            assert (int(a.ref["results"]["qlen"][i]) + 3) // 9 + 2 <= 128


@case
class ManyPathsBig(_Islands):
    """at least 128 paths from reads below 2047 bases: the plain locus (the prototype's read) and its masked twin"""

    def design(self):
        self.locus = self.island_locus(1440, [ST_C1])

    def finish(self, W):
        self.batch = Batch([self.masked(self.locus), self.locus], 1, ["masked128", "plain128"])

    def precondition(self, W, an):
        a = an["default"]
        for i in (0, 1):
            assert a.reads[i]["n_paths"] >= 128 and a.reads[i]["cls"] == ST_C1, a.reads[i]["n_paths"]
            assert len(self.batch.reads[i][0]) < 2047


@case
class ManyPathsPaired(_Islands):
    """the islands spread over both mates: 64 and 65 paths of the pair"""
    seq_mode = 2
    TARGETS = [64, 65]

    def design(self):
        self.locus = self.island_locus(840, [ST_C1])

    def finish(self, W):
        m = self.masked(self.locus)
        mate1, rest = m[:360].copy(), revcomp(m[360:])
        have = W.probe([mate1], 1).reads[0]["n_paths"]
        cut = self.cut_to_paths(W, rest, self.TARGETS, seq_mode=2, mate1=mate1, have=have)
        pairs = [(mate1, cut[t]) for t in self.TARGETS]
        self.batch = Batch(pairs, 2, [f"p{t}" for t in self.TARGETS])

    def precondition(self, W, an):
        a = an["default"]
        for i, t in enumerate(self.TARGETS):
            assert a.reads[i]["n_paths"] == t and a.reads[i]["cls"] == ST_C1 and a.n_metamers[i] <= 336, (t, a.reads[i]["n_paths"], a.n_metamers[i])
            assert a.reads[i]["n_matches"] == a.reads[i]["n_matched_metamers"]
            per_mate = [sum(1 for p in a.paths(i) if (p["start"] >= int(a.ref["results"]["qlen"][i]) + 3) == second) for second in (False, True)]
            assert min(per_mate) >= 12, per_mate


@case
class ManyPathsLong(_Islands):
    """the twin beyond 2047 bases (two-word sort key, seq_mode 3), next to the 65-path read"""
    seq_mode = 3

    def design(self):
        self.locus = self.island_locus(2400, [ST_C1])

    def finish(self, W):
        m = self.masked(self.locus)
        self.batch = Batch([self.locus, self.cut_to_paths(W, m, [65], seq_mode=3)[65], m], 3, ["plain", "p65", "masked"])

    def precondition(self, W, an):
        a = an["default"]
        assert len(self.batch.reads[0][0]) > 2047 and a.reads[0]["n_paths"] >= 128 and a.reads[2]["n_paths"] >= 128
        assert a.reads[1]["n_paths"] == 65
        assert all(r["cls"] == ST_C1 for r in a.reads)


# ============================================================================================== 6. combination (a16)
@case
class Combine(Case):
    """frame changes: the genome is the read with 1- or 2-base insertions / deletions, so the read's paths lie in different frames and
    overlap at the change.  One change past / before the middle puts the longer, higher-scoring path on the left / right (right / left
    trims of the other); two changes leave a middle segment that is trimmed twice.  The precondition is the set of branches seen."""
    WANT = {("left", 0), ("left", 1), ("left", 2), ("right", 0), ("right", 1), ("right", 2), "inside", "ge24_not_first", "trimmed_twice",
            "right_trim_higher_on_the_left"}

    def design(self):
        self.reads, self.names = [], []
        edits = [("ins", 1), ("ins", 2), ("del", 1), ("del", 2)]
        for kind, k in edits:                                        # one change, past and before the middle, at three phases of the codon
            for pos in (48, 49, 50, 97, 98, 99):
                s = locus(self.rng, 150)
                g = insert(s, pos, locus(self.rng, k)) if kind == "ins" else delete(s, pos, k)
                self.place(ST_B1, g)
                self.reads.append(s); self.names.append(f"{kind}{k}@{pos}")
        for (k1, n1), (k2, n2) in [(edits[a], edits[b]) for a in range(4) for b in range(4)]:      # two changes: segments of 75, 42 and 75 bases
            s = locus(self.rng, 192)
            g = insert(s, 117, locus(self.rng, n2)) if k2 == "ins" else delete(s, 117, n2)
            g = insert(g, 75, locus(self.rng, n1)) if k1 == "ins" else delete(g, 75, n1)
            self.place(ST_B1, g)
            self.reads.append(s); self.names.append(f"{k1}{n1}@75+{k2}{n2}@117")

    def finish(self, W):
        self.batch = Batch(self.reads, 1, self.names)

    @staticmethod
    def branches(a):
        seen = set()
        for i, r in enumerate(a.reads):
            for s in r["species"]:
                order = sorted(s["paths"], key=lambda p: (-float(p["score"]), p["ham"], -p["start"]))
                for t, p in zip(s["trace"], order):
                    seen.update(t["trims"])
                    if t["drop"] == "inside":
                        seen.add("inside")
                    if t["drop"] == "ge24" and t["against"] > 0:
                        seen.add("ge24_not_first")
                    if len(t["trims"]) >= 2 and t["drop"] is None and {side for side, _ in t["trims"]} == {"left", "right"}:
                        seen.add("trimmed_twice")
                    if t["trims"] and t["trims"][0][0] == "right" and t["drop"] is None and p["start"] > order[0]["start"]:
                        seen.add("right_trim_higher_on_the_left")
                    if t["equal_key"]:
                        seen.add("equal_key")
        return seen

    def precondition(self, W, an):
        a = an["default"]
        seen = self.branches(a)
        assert self.WANT <= seen, sorted(map(str, self.WANT - seen))
        assert all(r["cls"] == ST_B1 for r in a.reads)


# ============================================================================================== 7. several matches per position (S2), chain choice
@case
class TwoPerPosition(Case):
    """two strains of one species that differ by substitutions which keep the amino acid (third bases of frame 0, at different codons), and a
    read that differs from both in the same way: its metamers match both strains' targets at one position"""
    N_CAND = 6

    def design(self):
        T = bf.ref_tables()
        self.reads = []
        for j in range(self.N_CAND):                     # one changed codon in ten: a window of eight holds at most one
            s = locus(self.rng, 150)
            self.place(ST_A2a, s)
            self.place(ST_A2b, synonymous_variant(s, 0, 10, T, skip=j, pick=0)[0])
            self.reads.append(synonymous_variant(s, 0, 10, T, skip=j, pick=1)[0])

    def finish(self, W):
        self.batch = Batch(self.reads, 1)

    def precondition(self, W, an):
        a = an["default"]
        s2 = [i for i, r in enumerate(a.reads) if r["s2"]]
        assert s2, "no position group with two matches"
        assert any(p["multi_pred"] for i in s2 for p in a.paths(i)), "no match with two predecessors on an emitted chain"
        assert any(p["tied_chains"] for i in s2 for p in a.paths(i)), "no two chains of equal score to one end"
        assert all(r["is_cls"] == 1 and r["cls"] in (SP_A2, ST_A2a, ST_A2b) for r in a.reads), [r["cls"] for r in a.reads]
        # the redundancy filter: a position bucket whose minimum-hamming matches come from the two strains takes the species
        def two_strain_bucket(i):
            best = {}
            for m in a.by_read[i]:
                q = (m[0] & 0xFFFFFFFF) // 9
                if q not in best or m[5] < best[q][0]:
                    best[q] = (m[5], {m[1]})
                elif m[5] == best[q][0]:
                    best[q][1].add(m[1])
            return any(t == {ST_A2a, ST_A2b} for _, t in best.values())
        assert any(two_strain_bucket(i) and a.reads[i]["taxcnt"].get(SP_A2, 0) > 0 for i in s2), "no bucket whose best matches come from two strains"


# ============================================================================================== 8. redundancy filter and descent (a18)
@case
class Descent(Case):
    """Sibling strains that share a locus but for one base: the shared windows are filed under the strains' LCA, the windows over the base
    under the strain.  A position bucket (9 bases) counts for the strain only if every window in it covers the base, so a base at 8..16
    gives the child a clade count of 1 and a base at 17..23 a count of 2.  The reference descends to a child that alone reaches
    (len - 1) // 100 (Taxonomer.cpp: `>` takes the maximum, `==` joins it, one member descends).  The used length is always a multiple of 3
    (LocalUtil.h:51-59), so the lengths next to the steps of that threshold are 99 | 102, 198 | 201 and 300 | 303: per count the read is cut
    to each, and the count exceeds the threshold by one, equals it, and falls one short of it.  Two children that both reach it tie and
    the parent stays.  All of it again with accession_level = 2, which takes the child of rank "accession" out of the descent."""
    runs = [("default", {}), ("acc2", dict(accession_level=2))]
    FAMILIES = {"two": (SP_A2, ST_A2a, ST_A2b, SP_A2), "three": (SP_A1, ST_A1a, ST_A1b, SUB_A1), "acc": (SP_A3, ST_A3acc, ST_A3b, SP_A3)}
    USED = (99, 102, 198, 201, 300, 303)
    AT = {1: 12, 2: 20}                                   # base that differs, per child count
    TIED_ENDS = range(2, 26, 2)

    def design(self):
        self.loci, self.tied = {}, {}
        for fam, (_, a, b, _) in self.FAMILIES.items():
            for count, p in self.AT.items():
                s = locus(self.rng, 310)
                self.place(a, s)
                self.place(b, substitute(s, [p]))
                self.loci[(fam, count)] = s
            for e in self.TIED_ENDS:                           # strain b differs at base 12 and at a base near the end
                s = locus(self.rng, 105)
                self.place(a, s)
                self.place(b, substitute(s, [12, 104 - e]))
                self.tied[(fam, e)] = substitute(s, [104 - e])

    def finish(self, W):
        reads, names = [], []
        for fam, (sp, a, b, shared) in self.FAMILIES.items():
            for count in self.AT:
                for u in self.USED:
                    reads.append(self.loci[(fam, count)][:u + 3].copy()); names.append(f"{fam}-count{count}-used{u}")
            pr = W.probe([self.tied[(fam, e)] for e in self.TIED_ENDS], 1)
            e = next((e for j, e in enumerate(self.TIED_ENDS) if pr.reads[j]["taxcnt"].get(a, 0) == pr.reads[j]["taxcnt"].get(b, 0) == 1), None)
            assert e is not None, f"no locus of family {fam} with tied children"
            reads.append(self.tied[(fam, e)]); names.append(f"{fam}-tied")
        self.batch = Batch(reads, 1, names)

    def precondition(self, W, an):
        d, acc = an["default"], an["acc2"]
        ql = d.ref["results"]["qlen"]
        margins = set()
        for fam, (sp, a, b, shared) in self.FAMILIES.items():
            stay = shared if fam == "three" else sp              # three levels: the subspecies holds every bucket and is always entered
            for count in self.AT:
                for u in self.USED:
                    i = self.batch.index(f"{fam}-count{count}-used{u}")
                    r = d.reads[i]
                    assert int(ql[i]) == u and r["taxcnt"].get(a, 0) == count and set(r["taxcnt"]) == {a, shared}, (fam, count, u, r["taxcnt"])
                    thr = (u - 1) // 100
                    margins.add(count - thr)
                    assert r["cls"] == (a if count >= thr else stay), (fam, count, u, r["cls"])
                    want2 = sp if (fam == "acc" and count >= thr) else r["cls"]
                    assert acc.reads[i]["cls"] == want2, (fam, count, u, acc.reads[i]["cls"])
            i = self.batch.index(f"{fam}-tied")
            r = d.reads[i]
            assert int(ql[i]) == 102 and r["taxcnt"].get(a, 0) == r["taxcnt"].get(b, 0) == 1 == (int(ql[i]) - 1) // 100
            assert r["cls"] == stay, (fam, r["cls"])
            assert acc.reads[i]["cls"] == (ST_A3b if fam == "acc" else stay), (fam, acc.reads[i]["cls"])
        assert {1, 0, -1} <= margins, margins
        # the redundancy filter: position buckets whose minimum-hamming matches come from the strain and from the LCA entry take the LCA
        i = self.batch.index("two-count1-used99")
        both = [q for q in {(m[0] & 0xFFFFFFFF) // 9 for m in d.by_read[i]} if {m[1] for m in d.by_read[i] if (m[0] & 0xFFFFFFFF) // 9 == q} == {ST_A2a, SP_A2}]
        assert both, "no bucket that mixes the strain's and the species' entries"


# ============================================================================================== 9. N and nothing
@case
class NAndNothing(_Islands):
    """a read of only N and a read with no match, first and last in a batch with scoring reads; an island read with an N inside every
    second island"""

    def design(self):
        self.locus = self.island_locus(600, [ST_B1])
        self.plain = locus(self.rng, 150)
        self.place(ST_C1, self.plain)
        self.nomatch = [locus(self.rng, 150), locus(self.rng, 150)]

    def finish(self, W):
        holed = mask_n(self.masked(self.locus), np.arange(24, len(self.locus), 2 * self.PERIOD))
        reads = [np.full(150, N, np.uint8), self.plain, self.nomatch[0], holed, self.masked(self.locus), np.full(31, N, np.uint8), self.plain[:120].copy(), self.nomatch[1]]
        self.batch = Batch(reads, 1, ["allN", "plain", "nomatch", "holed", "islands", "shortN", "plain120", "nomatch_last"])

    def precondition(self, W, an):
        a = an["default"]
        b = self.batch
        for name in ("allN", "shortN"):
            assert a.n_metamers[b.index(name)] == 0
        for name in ("nomatch", "nomatch_last"):
            assert a.n_metamers[b.index(name)] > 0 and a.reads[b.index(name)]["n_matches"] == 0
        for name in ("allN", "shortN", "nomatch", "nomatch_last"):
            r = a.reads[b.index(name)]
            assert r["is_cls"] == 0 and r["cls"] == 0 and r["score"] == 0
        h, f = a.reads[b.index("holed")], a.reads[b.index("islands")]
        assert 0 < h["n_paths"] < f["n_paths"] and h["cls"] == f["cls"] == ST_B1 and 0 < h["score"] < f["score"]
        assert b.names[0] == "allN" and b.names[-1] == "nomatch_last"


# ============================================================================================== reads that overflow their slot tails
@case
class Overflow(_Islands):
    """an island read (case 5) and a read with two matches per position (case 7) whose every metamer also matches a second species:
    twice as many matches as ordinal slots, the tails overflow and the reads are deferred (k_score_many, or exact segments)"""

    def design(self):
        T = bf.ref_tables()
        self.islands = self.island_locus(660, [ST_C1, ST_B1])
        s = locus(self.rng, 150)
        for strain in (ST_A2a, ST_B1, ST_C1):
            self.place(strain, s)
        self.place(ST_A2b, synonymous_variant(s, 0, 10, T, skip=3, pick=0)[0])
        self.two = synonymous_variant(s, 0, 10, T, skip=3, pick=1)[0]
        self.plain = [locus(self.rng, 150) for _ in range(6)]
        for x in self.plain:
            self.place(ST_A3b, x)

    def finish(self, W):
        self.batch = Batch(self.plain[:3] + [self.masked(self.islands), self.two] + self.plain[3:], 1,
                           ["plain0", "plain1", "plain2", "islands", "two", "plain3", "plain4", "plain5"])

    def precondition(self, W, an):
        a = an["default"]
        i, j = self.batch.index("islands"), self.batch.index("two")
        assert a.reads[i]["n_paths"] > 64 and a.reads[i]["cls"] == BACTERIA and len(a.reads[i]["tied"]) == 2
        assert a.reads[j]["s2"] and len(a.reads[j]["species"]) == 3
        for k in (i, j):
            assert a.reads[k]["n_matches"] >= 2 * a.reads[k]["n_matched_metamers"] and a.n_metamers[k] <= 336


# ============================================================================================== ties the register-resident scorer decides itself
@case
class DisjointTies(Case):
    """Tied species that share no metamer of the read: each holds its own stretch of the read, so every metamer has one match, the slot
    tails stay empty and k_score_fast takes the whole decision (the ties above overflow their tails and are deferred).  Two halves that
    score the same (tie_ratio 0.95 and 1); three stretches with three different scores whose fp32 sum depends on the order."""
    runs = [("default", {}), ("ratio1", dict(tie_ratio=1.0)), ("ratio0.7", dict(tie_ratio=0.7))]
    HALVES = range(69, 82)
    N_THIRDS = 30

    def design(self):
        self.reads, self.names = [], []
        for h in self.HALVES:
            s = locus(self.rng, 150)
            self.place(ST_A1a, s[:h]); self.place(ST_A2a, s[h:])
            self.reads.append(s); self.names.append(f"halves@{h}")
        for j in range(self.N_THIRDS):
            s = locus(self.rng, 240 + j % 3)
            a, b = 84 + j % 7, 162 + j % 5
            self.place(ST_A1a, s[:a]); self.place(ST_A2a, s[a:b]); self.place(ST_A3b, s[b:])
            self.reads.append(s); self.names.append(f"thirds{j}")

    def finish(self, W):
        self.batch = Batch(self.reads, 1, self.names)

    def precondition(self, W, an):
        for a in an.values():
            assert all(r["n_matches"] == r["n_matched_metamers"] and not r["s2"] for r in a.reads), "a metamer with two matches"
        for label in ("default", "ratio1"):
            a = an[label]
            equal = [i for i, n in enumerate(self.names) if n.startswith("halves") and len(a.reads[i]["tied"]) == 2
                     and a.reads[i]["tied"][0][1] == a.reads[i]["tied"][1][1]]
            assert equal, "no read whose halves score the same"
            assert all(a.reads[i]["cls"] == GEN_A for i in equal)
        assert any(len(r["tied"]) == 1 for r in an["ratio1"].reads[:len(self.HALVES)]), "no halves that differ"      # (the other side of tie_ratio = 1)
        hits = order_hits(an["ratio0.7"])
        assert hits[1] and hits[2], f"no read whose three tied scores sum differently in another order: {hits}"
        assert all(an["ratio0.7"].reads[i]["cls"] == GEN_A for i in hits[1] + hits[2])


@case
class DisjointTieRatio(TieRatio):
    """the ratio boundary again with the two species on disjoint stretches of the read: k_score_fast compares sc2 with the cut"""

    def design(self):
        self.read = locus(self.rng, 150)
        self.place(ST_A1a, self.read[:90])
        self.place(ST_B1, self.read[90:])


# ============================================================================================== the same designs as long reads (seq_mode 3)
def _as_long(base):
    """the design and precondition of `base` on loci of its own, classified in seq_mode 3: k_seg_order + k_score_long and the exact segments"""
    class Long(base):
        seq_mode = 3

        def finish(self, W):
            super().finish(W)
            self.batch = Batch([r for r, _ in self.batch.reads], 3, self.batch.names)
    Long.__name__ = Long.__qualname__ = base.__name__ + "Long"
    Long.__doc__ = f"{base.__name__} as long reads"
    return case(Long)


CombineLong = _as_long(Combine)
TwoPerPositionLong = _as_long(TwoPerPosition)
DisjointTiesLong = _as_long(DisjointTies)
DepthLong = _as_long(Depth)
