"""The tail merge of k_score_fast (kernels_score_fast.h): reads whose metamers have a second match in another species keep those matches
in their tail slots, i.e. at the END of their species' run of the compacted list; the merge moves every tail match to its (frame,
position) place among the run's direct matches, so that the read stays on the register-resident scorer -- single reads and pairs.

Designed reads (tests/designed_reads.py): a locus filed under one species in full and a stretch of it under a second (and third) one.
Every metamer of the stretch then has one match per species: one of them lands in the metamer's direct slot, the other in the tail,
whichever the join's atomics decide -- so both species' runs hold direct and tail matches, and the stretch at the start, in the middle
and at the end of the locus puts the tail keys below, between and above the direct keys of their runs.  Every read is compared bit for
bit with the oracle (classification, is_classified, fp32 score bits, n_taxcnt, taxID:count lists), and mtb_batch_stats must show that
k_score_fast kept exactly the reads the CPU side says it can keep: after the merge that no longer depends on the atomics' order.

`plan` mirrors the hand-over from the CPU side: a read whose tails overflow (more second matches than tail slots) is deferred; a read
with two matches in one position group (S2), more than 64 paths (S3), too many position buckets or more than 64 tail matches goes to
k_score<SLOT>; every other read is decided by k_score_fast.

Two keys that are equal in every field (species, frame, position, hamming, dna) need one metamer value filed twice under one species;
the database keeps one entry per value and species, so the nearest a read gets is two matches of one species at one position with
different hamming / dna bits (one metamer value matched by two targets of a species: the `s2-*` reads of Single3, tail and direct match in one position
group, and two tail matches in one when a third species takes the direct slot) -- those reads are S2 once merged and must reach the
generic kernel."""
import numpy as np
import pytest

import bruteforce as bf
import designed_reads as D
from test_gpu_designed_reads import mparams, same_as_oracle
from test_gpu_scorer_tiers import K_SCORE_FAST, slot_plan

pytestmark = pytest.mark.gpu

SLOT_BUCKETS, FAST_MAX_PATHS, MERGE_MAX_TAILS = 128, 64, 64       # kernels_score_fast.h: MTB_FAST_BKT, S3, the lanes that own the tail matches
PLACES = ("start", "middle", "end")


def stretch(s, x, where):
    lo = {"start": 0, "middle": (len(s) - x) // 2, "end": len(s) - x}[where]
    return s[lo:lo + x]


class _Shared(D.Case):
    """reads = loci filed under ST_A1a in full, stretches of them under other strains"""
    tail_min = 0
    bucket = None                                        # the k_score_fast instantiation the batch must select

    def __init__(self):
        super().__init__()
        self.reads, self.names = [], []

    def shared(self, name, length, pieces):
        """a locus under ST_A1a and, per (strain, x, where), a stretch of x bases of it under that strain"""
        s = D.locus(self.rng, length)
        self.place(D.ST_A1a, s)
        for strain, x, where in pieces:
            self.place(strain, stretch(s, x, where))
        self.reads.append(s); self.names.append(name)
        return s

    def finish(self, W):
        self.batch = D.Batch(self.reads, self.seq_mode, self.names)

    def precondition(self, W, an):
        pass


class Single2(_Shared):
    """fast<2>: second species on 24..45 bases at the start, in the middle, at the end -- 1 tail match up to the tail's capacity (16) and
    beyond (deferred); a second species with ONE match (lonely: dropped before the merge, in the tail or not); two species that overlap
    on 24..30 bases only (one tail match, neither species lonely)"""
    bucket = "fast<2>"

    def design(self):
        for where in PLACES:
            for x in range(24, 46):
                self.shared(f"{where}-x{x}", 110, [(D.ST_B1, x, where)])
        for ov in range(24, 31):                             # A1 on [0, 60 + ov), B1 on [60, 120)
            s = D.locus(self.rng, 120)
            self.place(D.ST_A2a, s[:60 + ov]); self.place(D.ST_B1, s[60:])
            self.reads.append(s); self.names.append(f"overlap{ov}")

    def precondition(self, W, an):
        t = tails(an)
        cur = [x["cur"] for x in t]
        assert {1, 15, 16, 17} <= set(cur), sorted(set(cur))                           # one tail match; the capacity and one beyond
        for where in PLACES:
            assert any(0 < x["cur"] <= 16 and n.startswith(where) for x, n in zip(t, self.names)), where
        assert any(x["cur"] == 1 and min(x["per_species"].values()) == 1 for x in t), "no lonely second species"
        assert any(x["cur"] == 1 and min(x["per_species"].values()) > 1 and n.startswith("overlap") for x, n in zip(t, self.names)), "no single tail match between two scoring species"


class Single3(_Shared):
    """fast<3>: tail matches in the runs of two and three species; one metamer value matched by two targets of one species (S2 once
    merged); compacted lists of 64 | 65 and 128 | 129 matches (one, two, three register slots)"""
    bucket = "fast<3>"
    LENGTHS = (64, 65, 128, 129)

    def design(self):
        T = bf.ref_tables()
        for x, y in ((30, 30), (36, 28), (28, 40)):
            self.shared(f"two-runs-{x}-{y}", 175, [(D.ST_B1, x, "start"), (D.ST_C1, y, "end")])
            self.shared(f"same-stretch-{x}", 175, [(D.ST_B1, x, "middle"), (D.ST_C1, x, "middle")])
        self.s2 = []
        for j in range(3):                                   # TwoPerPosition of tests/designed_reads.py, and a third species on a stretch
            s = D.locus(self.rng, 170)
            self.place(D.ST_A2a, s)
            self.place(D.ST_A2b, D.synonymous_variant(s, 0, 10, T, skip=j, pick=0)[0])
            read = D.synonymous_variant(s, 0, 10, T, skip=j, pick=1)[0]
            self.place(D.ST_E1, read[40:80])
            self.s2.append(read)
        self.cut = [D.locus(self.rng, 175) for _ in range(3)]
        for s in self.cut:
            self.place(D.ST_A1a, s); self.place(D.ST_B1, s[:34])

    def finish(self, W):
        for j, r in enumerate(self.s2):
            self.reads.append(r); self.names.append(f"s2-{j}")
        found = {}
        for s in self.cut:                                   # prefixes of one locus: the compacted length moves by one or two per base
            ns, a = D.prefixes(W, s, range(60, len(s) + 1))
            for j, n in enumerate(ns):
                r = a.reads[j]
                if r["n_matches"] in self.LENGTHS and r["n_matches"] > r["n_matched_metamers"]:
                    found.setdefault(r["n_matches"], s[:n].copy())
        assert sorted(found) == sorted(self.LENGTHS), sorted(found)
        for n in self.LENGTHS:
            self.reads.append(found[n]); self.names.append(f"n{n}")
        super().finish(W)

    def precondition(self, W, an):
        t = tails(an)
        for n in self.LENGTHS:
            x = t[self.batch.index(f"n{n}")]
            assert x["n_matches"] == n and 0 < x["cur"] <= 16 and min(x["per_species"].values()) > 1, (n, x)
        for name in self.names:
            x = t[self.batch.index(name)]
            if name.startswith(("two-runs", "same-stretch")):
                assert len(x["per_species"]) == 3 and min(x["per_species"].values()) > 1 and 0 < x["cur"], (name, x)
            if name.startswith("s2"):
                assert x["s2"] and 0 < x["cur"], (name, x)
        assert any(n.startswith("two-runs") and t[i]["cur"] <= 16 for i, n in enumerate(self.names))
        assert any(n.startswith("s2") and t[i]["cur"] <= 16 and t[i]["tail_pairs"] for i, n in enumerate(self.names)), "no S2 read within its tail"


class Single4(_Shared):
    """fast<4>"""
    bucket = "fast<4>"

    def design(self):
        for where in PLACES:
            for x in (28, 36, 44):
                self.shared(f"{where}-x{x}", 225, [(D.ST_B1, x, where)])


class Single72(_Shared):
    """tails of 72 slots (MTB_TAIL_MIN): 58 .. 72 tail matches -- up to 64 the merge takes them, from 65 the read is handed over"""
    tail_min = 72
    bucket = "fast<4>"

    def design(self):
        for where in PLACES:
            for x in range(82, 96):
                self.shared(f"{where}-x{x}", 165, [(D.ST_B1, x, where)])

    def precondition(self, W, an):
        cur = {x["cur"] for x in tails(an)}
        assert {63, 64, 65, 66} <= cur and max(cur) <= 80, sorted(cur)


class Single56(_Shared):
    """fast<5,6,false> (a slot stride above 256)"""
    bucket = "fast<5,6,false>"

    def design(self):
        for where in PLACES:
            for x in (30, 44):
                self.shared(f"{where}-x{x}", 300, [(D.ST_B1, x, where)])


class _Pairs(_Shared):
    """the locus read as a pair: mate 1 its first `MATE` bases, mate 2 the reverse complement of its last `MATE`; second species on a
    stretch inside either mate and over both"""
    seq_mode = 2
    MATE = 80

    def design(self):
        m = self.MATE
        for x in (30, 40):
            for where in PLACES:
                self.shared(f"{where}-x{x}", 2 * m + 10, [(D.ST_B1, x, where)])
            self.shared(f"both-x{x}", 2 * m + 10, [(D.ST_B1, x, "start"), (D.ST_C1, x, "end")])

    def finish(self, W):
        m = self.MATE
        self.reads = [(s[:m].copy(), D.revcomp(s[-m:])) for s in self.reads]
        super().finish(W)


class Pairs3(_Pairs):
    bucket = "fast<3,3,true>"


class Pairs4(_Pairs):
    bucket = "fast<4,4,true>"
    MATE = 115


class Pairs56(_Pairs):
    bucket = "fast<5,6,true>"
    MATE = 150


CASES = [Single2, Single3, Single4, Single72, Single56, Pairs3, Pairs4, Pairs56]      # a world of their own, not the designed-reads world's
CASE_NAMES = [c.__name__ for c in CASES]


def tails(an):
    """per read of the case's default run: the matches beyond the first of their metamer (`cur`: what the join puts into the tail), the
    matches per species, and whether some metamer has two matches of one species (`tail_pairs`)"""
    a = an["default"] if isinstance(an, dict) else an
    out = []
    for i, r in enumerate(a.reads):
        per_species, per_metamer = {}, {}
        for q in a.by_read[i]:
            per_species[q[2]] = per_species.get(q[2], 0) + 1
            per_metamer.setdefault(q[0], []).append(q[2])
        out.append(dict(cur=r["n_matches"] - r["n_matched_metamers"], n_matches=r["n_matches"], s2=r["s2"], n_paths=r["n_paths"], per_species=per_species,
                        tail_pairs=any(len(v) != len(set(v)) for v in per_metamer.values())))
    return out


def plan(case, a):
    """(slot plan, counts) of a batch from the CPU side alone: `over` reads deferred for their tails, `generic` reads k_score_fast hands to
    k_score<SLOT> (S2, S3, position buckets, more than 64 tail matches) and of those the ones k_score<SLOT> defers in turn (`generic_big`:
    more live records than its staging of slot_plan's `cap` holds, or too many position buckets), `merged` reads with tail matches that
    k_score_fast decides itself"""
    ro = a.ref["results"]
    qlt = (ro["qlen"] + ro["qlen2"]).astype(np.int64)
    p = slot_plan(a.n_metamers, qlt, case.seq_mode == 2, tail_min=case.tail_min)
    assert p["slot"] and not p["route_off"], p
    tail_cap = p["stride"] - p["direct"]
    n = dict(over=0, generic=0, generic_big=0, merged=0, handed_for_tails=0)
    for i, x in enumerate(tails(a)):
        buckets = (int(qlt[i]) + 3) // 9 + 2 > SLOT_BUCKETS
        big = buckets or x["n_matches"] > p["cap"]
        if x["cur"] > tail_cap:
            n["over"] += 1
        elif buckets or x["s2"] or x["n_paths"] > FAST_MAX_PATHS:
            n["generic"] += 1; n["generic_big"] += big
        elif x["cur"] > MERGE_MAX_TAILS:
            n["generic"] += 1; n["handed_for_tails"] += 1; n["generic_big"] += big
        elif x["cur"] > 0:
            n["merged"] += 1
    return p, tail_cap, n


@pytest.fixture(scope="module")
def world(orc, tmp_path_factory):
    return D.DesignedWorld(orc, tmp_path_factory.mktemp("tail_merge"), cases=CASES)


@pytest.fixture(scope="module")
def gpu(world):
    import metabuli_amd as M
    c = M.Context(0)
    c.set_profiling(True)
    ix = c.open_index(world.dbdir, M.default_params(seq_mode=1, syncmer=D.SYNCMER, smer_len=D.SMER_LEN))
    yield c, ix
    ix.close(); c.close()


@pytest.mark.parametrize("name", CASE_NAMES)
def test_tail_matches_are_merged_and_the_read_stays(gpu, world, name):
    ctx, ix = gpu
    c = world.case(name)
    a = world.analysis(c, "default")
    c.precondition(world, {"default": a})
    p, tail_cap, n = plan(c, a)
    assert p["bucket"] == c.bucket, (name, p)
    t = tails(a)
    if name != "Single72":                                   # `merged`: reads with tail matches, all within the tail, no S2 / S3
        assert n["merged"] > 0 and n["handed_for_tails"] == 0, (name, n)
    else:
        assert tail_cap == 72 and n["merged"] > 0 and n["handed_for_tails"] > 0 and n["over"] > 0, (tail_cap, n)
    assert all(x["n_paths"] <= FAST_MAX_PATHS for x in t)
    if c.tail_min:
        ctx.set_option("MTB_TAIL_MIN", str(c.tail_min))
    try:
        b = c.batch
        res, tt, tc = ctx.classify_batch(ix, mparams(a), b.b1, b.o1, b.b2, b.o2)
        st = ctx.last_stats()
    finally:
        if c.tail_min:
            ctx.set_option("MTB_TAIL_MIN", None)
    tag = (name, p, n, st.n_generic_reads, st.n_deferred_reads)
    same_as_oracle(a.ref, res, tt, tc, tag)
    assert st.n_reads == b.n and st.n_slot_reads == b.n and st.n_matches == len(a.ref["matches"]), tag
    assert st.n_launch[K_SCORE_FAST] == 1, tag
    assert st.n_generic_reads == n["generic"], tag           # exact: the reads with tail matches stay, whatever order the atomics filled the tails in
    assert st.n_deferred_reads == n["over"] + n["generic_big"], tag      # exact too: no read is deferred that should stay
