"""The designed reads of tests/designed_reads.py through every scorer: the exact segments of k_score (`ctx.score`), the fused batch at
defaults (k_score_fast, k_score<SLOT> for what it hands over, the deferred tiers for what overflows; long reads: k_seg_order +
k_score_long), and the switches that move reads between them.  Every read is compared with the oracle on classification, is_classified,
the fp32 score bits, n_taxcnt and the taxID:count lists -- no read is masked: tests/test_designed_reads_spec.py asserts that the oracle
flags none.  One world, one context and one open index for the whole file.

`fast_plan` mirrors, from the CPU side alone, what k_score_fast does with every read of a slot batch (kernels_score_fast.h: tail
overflow -> deferred; more than 128 position buckets, S2 or S3 -> handed to k_score<SLOT>; S1 holds by construction when every metamer
has one match).  The one thing it cannot know is the order in which a single-end read's few tail matches were appended (atomics): such
reads count as "either", and the cases that sit on S2 / S3 assert that they have none, so their n_generic_reads is exact."""
import numpy as np
import pytest

import designed_reads as D
from test_gpu_scorer_tiers import K_SCORE_FAST, K_SCORE_MANY, slot_plan

pytestmark = pytest.mark.gpu

CASE_NAMES = [c.__name__ for c in D.CASES]
SLOT_BUCKETS, FAST_MAX_PATHS = 128, 64                   # kernels_score_fast.h MTB_FAST_BKT = kernels_score.h MTB_SCORE_BKT; S3
# cases whose hand-over count must be decidable (value: the count; None: as planned, one per read with two matches in a position group)
EXACT_GENERIC = {"ManyPaths": 1, "ManyPathsPaired": 1, "TwoPerPosition": None, "Combine": 0, "Descent": 0, "DisjointTies": 0, "DisjointTieRatio": 0}
FAST_DECIDES = ("DisjointTies", "DisjointTieRatio")      # no read leaves k_score_fast: the tie arithmetic under test is its own


@pytest.fixture(scope="module")
def world(orc, tmp_path_factory):
    return D.DesignedWorld(orc, tmp_path_factory.mktemp("designed_gpu"))


@pytest.fixture(scope="module")
def gpu(world):
    import metabuli_amd as M
    c = M.Context(0)
    c.set_profiling(True)
    ix = c.open_index(world.dbdir, M.default_params(seq_mode=1, syncmer=D.SYNCMER, smer_len=D.SMER_LEN))
    yield c, ix
    ix.close(); c.close()


def mparams(a):
    import metabuli_amd as M
    p = a.p
    return M.default_params(seq_mode=p.seq_mode, syncmer=p.syncmer, smer_len=p.smer_len, kmer_format=p.kmer_format, min_cons_cnt=p.min_cons_cnt,
                            min_cons_cnt_euk=p.min_cons_cnt_euk, min_score=p.min_score, min_sp_score=p.min_sp_score, tie_ratio=p.tie_ratio,
                            accession_level=p.accession_level)


def same_as_oracle(ref, res, tt, tc, tag):
    ro = ref["results"]
    for f in ("classification", "is_classified", "n_taxcnt", "qlen", "qlen2"):
        assert (res[f] == ro[f]).all(), (tag, f, np.flatnonzero(res[f] != ro[f])[:5], res[f][:8], ro[f][:8])
    assert (res["score"].view(np.uint32) == ro["score"].view(np.uint32)).all(), (tag, "score", res["score"][:8], ro["score"][:8])
    for i in range(len(ro)):
        a, b, n = int(res["taxcnt_off"][i]), int(ro["taxcnt_off"][i]), int(ro["n_taxcnt"][i])
        assert (tt[a:a + n] == ref["tc_tax"][b:b + n]).all() and (tc[a:a + n] == ref["tc_cnt"][b:b + n]).all(), (tag, i)


def fast_plan(case, a):
    """what becomes of every read of a short-read batch, from the CPU side alone -> (slot_plan, counts): `over` reads whose tails overflow
    (deferred by either slot scorer), `sure` / `maybe` reads k_score_fast hands to k_score<SLOT>, and of each kind those that k_score<SLOT>
    defers in turn (more live records than its staging holds, or too many position buckets): `*_big`; `all_big` the same over every read
    that does not overflow (MTB_NO_FAST_SCORER)"""
    ro = a.ref["results"]
    qlt = (ro["qlen"] + ro["qlen2"]).astype(np.int64)
    paired = case.seq_mode == 2
    plan = slot_plan(a.n_metamers, qlt, paired)
    n = dict(over=0, sure=0, maybe=0, sure_big=0, maybe_big=0, all_big=0)
    if not plan["slot"]:
        return plan, n
    assert not plan["route_off"]
    tail_cap = plan["stride"] - plan["direct"]
    for i, r in enumerate(a.reads):
        cur = r["n_matches"] - r["n_matched_metamers"]              # matches beyond the first of their metamer go to the read's tail
        if cur > tail_cap:
            n["over"] += 1
            continue
        buckets = (int(qlt[i]) + 3) // 9 + 2 > SLOT_BUCKETS
        big = buckets or r["n_matches"] > plan["cap"]
        n["all_big"] += big
        assert r["n_matches"] <= 320                                 # (what every k_score_fast instantiation holds in registers)
        if buckets or r["s2"] or r["n_paths"] > FAST_MAX_PATHS:
            n["sure"] += 1; n["sure_big"] += big
        elif cur > 0 and not paired:                                 # tail matches stay where the atomics put them: in order or not
            n["maybe"] += 1; n["maybe_big"] += big
    return plan, n


@pytest.mark.parametrize("name", CASE_NAMES)
def test_exact_segments(gpu, world, name):
    """k_score on the oracle's sorted matches"""
    ctx, ix = gpu
    c = world.case(name)
    for label, _ in c.runs:
        a = world.analysis(c, label)
        ref = a.ref
        res, tt, tc = ctx.score(ix, mparams(a), ref["matches"], c.batch.n, ref["qlen"], ref["qlen2"])
        same_as_oracle(ref, res, tt, tc, (name, label))


def _classify(ctx, ix, c, a, tag):
    b = c.batch
    res, tt, tc = ctx.classify_batch(ix, mparams(a), b.b1, b.o1, b.b2, b.o2)
    st = ctx.last_stats()
    same_as_oracle(a.ref, res, tt, tc, tag)
    assert st.n_reads == b.n and st.n_kmers == len(a.ref["kmers"]) and st.n_matches == len(a.ref["matches"]), (tag, st.n_kmers, st.n_matches)
    return st


SHORT = [n for n in CASE_NAMES if D.CASES[CASE_NAMES.index(n)].seq_mode != 3]
LONG = [n for n in CASE_NAMES if D.CASES[CASE_NAMES.index(n)].seq_mode == 3]


@pytest.mark.parametrize("name", SHORT)
def test_fused_batch_and_who_scores_what(gpu, world, name):
    """defaults: k_score_fast hands exactly the reads that break S2 / S3 (or have too many position buckets) to k_score<SLOT>, and defers
    those whose tails overflow; MTB_NO_FAST_SCORER: k_score<SLOT> takes every read; pairs again with MTB_NO_FAST_PAIRS"""
    ctx, ix = gpu
    c = world.case(name)
    switches = [None, "MTB_NO_FAST_SCORER"] + (["MTB_NO_FAST_PAIRS"] if c.seq_mode == 2 else [])
    try:
        for label, _ in c.runs:
            a = world.analysis(c, label)
            plan, n = fast_plan(c, a)
            if name in EXACT_GENERIC:
                assert n["maybe"] == 0 and plan["bucket"].startswith("fast"), (name, plan, n)
                assert EXACT_GENERIC[name] in (None, n["sure"]), (name, n)
            if name in FAST_DECIDES:
                assert n["over"] == 0, (name, n)
            if name == "TwoPerPosition":
                assert n["sure"] == sum(r["s2"] for r in a.reads) > 0
            for sw in switches:
                if sw:
                    ctx.set_option(sw, "1")
                st = _classify(ctx, ix, c, a, (name, label, sw))
                tag = (name, label, sw, plan, n, st.n_generic_reads, st.n_deferred_reads, st.n_many_reads)
                assert st.n_slot_reads == (c.batch.n if plan["slot"] else 0), tag
                fast = sw is None and plan["slot"] and plan["bucket"].startswith("fast")
                assert st.n_launch[K_SCORE_FAST] == (1 if fast else 0), tag
                if fast:
                    assert n["sure"] <= st.n_generic_reads <= n["sure"] + n["maybe"], tag
                    assert n["over"] + n["sure_big"] <= st.n_deferred_reads <= n["over"] + n["sure_big"] + n["maybe_big"], tag
                else:
                    assert st.n_generic_reads == c.batch.n, tag
                    if plan["slot"]:
                        assert st.n_deferred_reads == n["over"] + n["all_big"], tag
                if sw:
                    ctx.set_option(sw, None)
    finally:
        for sw in switches[1:]:
            ctx.set_option(sw, None)


LONG_SWITCHES = [(), (("MTB_NO_LONG_SCORER", "1"),), (("MTB_NO_LONG_SLOTS", "1"),), (("MTB_NO_LONG_SLOTS", "1"), ("MTB_NO_LONG_SCORER", "1"))]


@pytest.mark.parametrize("name", LONG)
def test_long_reads_on_slot_ranges_and_exact_segments(gpu, world, name):
    """seq_mode 3: the per-read slot ranges with k_score_long, MTB_NO_LONG_SLOTS (regroup + segment sort), MTB_NO_LONG_SCORER on either"""
    ctx, ix = gpu
    c = world.case(name)
    names = {k for sws in LONG_SWITCHES for k, _ in sws}
    try:
        for label, _ in c.runs:
            a = world.analysis(c, label)
            for sws in LONG_SWITCHES:
                for k in names:
                    ctx.set_option(k, None)
                for k, v in sws:
                    ctx.set_option(k, v)
                st = _classify(ctx, ix, c, a, (name, label, sws))
                tag = (name, label, sws, st.n_slot_reads, st.n_generic_reads)
                if "MTB_NO_LONG_SLOTS" not in dict(sws):
                    assert st.n_slot_reads == c.batch.n, tag
                else:
                    assert st.n_slot_reads == 0, tag
                    if "MTB_NO_LONG_SCORER" in dict(sws):
                        assert st.n_generic_reads == c.batch.n, tag
    finally:
        for k in names:
            ctx.set_option(k, None)


def test_overflowing_tails_are_deferred_and_scored_by_either_tier(gpu, world):
    """the island read and the two-per-position read with twice as many matches as ordinal slots: deferred, taken by k_score_many; with
    MTB_NO_SCORE_MANY by the tiers behind it"""
    ctx, ix = gpu
    c = world.case("Overflow")
    a = world.analysis(c, "default")
    plan, n = fast_plan(c, a)
    assert n["over"] == 2 and n["sure"] == n["maybe"] == 0 and plan["bucket"].startswith("fast"), (plan, n)
    try:
        st = _classify(ctx, ix, c, a, "default")
        assert st.n_deferred_reads == 2 and st.n_many_reads > 0 and st.n_launch[K_SCORE_MANY] == 1, (st.n_deferred_reads, st.n_many_reads)
        ctx.set_option("MTB_NO_SCORE_MANY", "1")
        st = _classify(ctx, ix, c, a, "MTB_NO_SCORE_MANY")
        assert st.n_deferred_reads == 2 and st.n_many_reads == 0 and st.n_launch[K_SCORE_MANY] == 0, (st.n_deferred_reads, st.n_many_reads)
    finally:
        ctx.set_option("MTB_NO_SCORE_MANY", None)
