"""The score stage with its deferred tier on the side stream (score_fixed_slots in mtb_api.hip): the reads whose tails overflowed (list A,
made from the join's cursors by k_list_overflowed before any scorer runs) go through k_score_many, k_many_sort and k_score_long BESIDE
k_score_fast; the reads the generic slot kernel defers afterwards (list B) get a run of the tier of their own behind the join of the
two streams; what neither run scored takes the exact-segment path as one list.

Every batch runs three ways -- a context as it comes (tier on the side stream: score_overlapped = 1), a context with profiling on (the same
launches on one stream, score_overlapped = 0) and the oracle -- and rows and taxID:count lists must be bit-equal across the three, with the
exact n_generic_reads / n_deferred_reads / n_many_reads that `plan` mirrors from the oracle's matches alone.

Forged world as in tests/test_gpu_score_many_edges.py: error-free 150-base reads cut from genome 0, chosen metamers of a read filed once
more under new species, so k copies add exactly k tail / overflow entries.  One copy per new species: dead, dropped before the staging;
a species with many copies survives with all of them."""
import numpy as np
import pytest

import designed_reads as D
from test_gpu_designed_reads import same_as_oracle
from test_gpu_score_many_edges import MANY_HASH, Forge, _world, as_reads, copies, cut, forged_batch, per_read, single_values
from test_gpu_scorer_tiers import Reads, metamers_per_read, slot_plan

pytestmark = pytest.mark.gpu

MERGE_MAX_TAILS = 64                                     # kernels_score_fast.h: more tail matches than lanes -> the generic kernel
SORT_SMALL, SORT_BIG = 2048, 4096                        # k_many_sort's two instantiations: survivors each holds
N_OVF = 17                                               # plain overflow reads: enough for a list of 17
STAGE193, BEYOND4096, B66, B72, A75, A80 = N_OVF, N_OVF + 1, N_OVF + 2, N_OVF + 3, N_OVF + 4, N_OVF + 5
PLAIN = list(range(N_OVF + 6, N_OVF + 11))               # five reads nothing is filed for
MATE = 75


def _mp(seq_mode):
    import metabuli_amd as M
    return M.default_params(seq_mode=seq_mode, syncmer=1)


def _op(seq_mode):
    from helpers import default_params
    return default_params(seq_mode=seq_mode, syncmer=1)


@pytest.fixture(scope="module")
def base(orc, tmp_path_factory):
    return Forge(orc, tmp_path_factory.mktemp("overlap_base"))


@pytest.fixture(scope="module")
def forged(orc, base, tmp_path_factory):
    """reads 0 .. 16: one to five overflow entries of dead species; a read with 193 survivors (one more than k_score_many<.., 192> stages: the
    small k_many_sort takes it); a read with more than 4096 survivors (beyond both k_many_sort instantiations: exact segments); reads with
    66, 72 (of one further species), 75 and 80 (dead) tail matches (with tails of 72 slots: two reads k_score_fast hands to the generic
    kernel, which cannot stage them, and two that overflow); five plain reads"""
    def want(i, f, tail_cap, free, singles):
        assert f["cur"] == 0 and len(singles) >= 100, (i, f, len(singles))
        dead = free + np.arange(200)
        if i < N_OVF:
            return copies(singles, tail_cap + 1 + i % 5, dead)
        if i == STAGE193:
            return copies(singles, 193 - f["kept"], [free + 200])
        if i == BEYOND4096:
            return copies(singles, SORT_BIG + 100, free + 300 + np.arange(150))
        if i in (B66, B72):                                  # one species that survives: dead species' matches are dropped before k_score_fast counts its tail matches
            return copies(singles, {B66: 66, B72: 72}[i], [free + 201])
        if i in (A75, A80):
            return copies(singles, {A75: 75, A80: 80}[i], dead)
        return None
    return forged_batch(orc, base, tmp_path_factory.mktemp("overlap_forged"), 150, [1000 + 400 * i for i in range(PLAIN[-1] + 1)], want)


def pick(r, idx):
    return as_reads([r.b1[int(r.o1[i]):int(r.o1[i + 1])] for i in idx])


def plan(ref, n_reads, paired=False, tail_min=0):
    """what becomes of every read, from the oracle's answer alone -> counts: `a` reads whose tails overflow, `generic` reads k_score_fast hands
    to the generic kernel for their tail matches, `b` those of them it cannot stage; of a + b the reads k_score_many scores (`many`), the ones
    it hands on and k_many_sort + k_score_long take (`sorted`) and the ones left to the exact segments (`exact`)"""
    counts = metamers_per_read(ref["kmers"], n_reads)
    qlt = (ref["results"]["qlen"] + ref["results"]["qlen2"]).astype(np.int64)
    p = slot_plan(counts, qlt, paired, tail_min=tail_min)
    assert p["slot"] and not p["route_off"] and p["stride"] <= 384 and p["bucket"].startswith("fast"), p
    cap = 192 if p["stride"] <= 192 else 320
    tail_cap = p["stride"] - p["direct"]
    n = dict(a=0, generic=0, b=0, many=0, sorted=0, exact=0)
    for f in per_read(ref, n_reads):
        if f["cur"] > tail_cap:
            n["a"] += 1
        elif f["cur"] > MERGE_MAX_TAILS and not paired:
            n["generic"] += 1
            if f["n"] <= p["cap"]:
                continue
            n["b"] += 1
        else:
            continue
        if f["cur"] <= 3 * cap and f["species"] <= MANY_HASH // 4 * 3 and f["kept"] <= cap:
            n["many"] += 1
        elif f["kept"] <= SORT_BIG and f["species"] <= SORT_BIG // 4 * 3:
            n["sorted"] += 1
        else:
            n["exact"] += 1
    return p, n


@pytest.fixture(scope="module")
def gpus():
    """the context as it comes and the one with profiling on: every kernel on one stream, one after another"""
    import metabuli_amd as M
    c, s = M.Context(0), M.Context(0)
    s.set_profiling(True)
    yield c, s
    c.close(); s.close()


def three_ways(gpus, w, batches, seq_mode=1, tail_min=0):
    """each batch of `batches` in turn on either context (one index per context, open over all of them) and through the oracle"""
    import metabuli_amd as M
    out = []
    refs = [w.orc.classify(w.db, w.tax, _op(seq_mode), r.b1, r.o1, r.b2, r.o2) for r in batches]
    got = {}
    for name, ctx in zip(("overlap", "serial"), gpus):
        if tail_min:
            ctx.set_option("MTB_TAIL_MIN", str(tail_min))
        ix = ctx.open_index(w.dbdir, _mp(seq_mode))
        try:
            got[name] = []
            for r in batches:
                res, tt, tc = ctx.classify_batch(ix, _mp(seq_mode), r.b1, r.o1, r.b2, r.o2)
                got[name].append((res.copy(), tt.copy(), tc.copy(), ctx.last_stats()))
        finally:
            ix.close()
            if tail_min:
                ctx.set_option("MTB_TAIL_MIN", None)
    for k, (r, ref) in enumerate(zip(batches, refs)):
        assert (ref["results"]["flag"] == 0).all()                    # nothing masked
        p, n = plan(ref, r.n, paired=seq_mode == 2, tail_min=tail_min)
        (ro, to, co, so), (rs, ts, cs, ss) = got["overlap"][k], got["serial"][k]
        for name, (res, tt, tc, st) in (("overlap", got["overlap"][k]), ("serial", got["serial"][k])):
            tag = (name, k, p, n, st.n_generic_reads, st.n_deferred_reads, st.n_many_reads)
            same_as_oracle(ref, res, tt, tc, tag)
            assert st.n_matches == len(ref["matches"]) and st.n_slot_reads == r.n, tag
            assert st.score_overlapped == (1 if name == "overlap" else 0), tag
            assert (st.n_generic_reads, st.n_deferred_reads, st.n_many_reads) == (n["generic"], n["a"] + n["b"], n["many"] + n["sorted"]), tag
        assert ro.tobytes() == rs.tobytes() and (to == ts).all() and (co == cs).all(), k
        out.append((p, n))
    return out


def test_a_no_read_overflows(gpus, forged):
    """list A empty: fork and join with an idle side stream"""
    w, r = forged
    (p, n), = three_ways(gpus, w, [pick(r, PLAIN)])
    assert (n["a"], n["b"], n["generic"]) == (0, 0, 0), n


def test_b_every_read_overflows(gpus, forged):
    """k_score_fast scores nothing"""
    w, r = forged
    (p, n), = three_ways(gpus, w, [pick(r, range(N_OVF))])
    assert (n["a"], n["many"], n["b"]) == (N_OVF, N_OVF, 0) and p["stride"] <= 192, (p, n)


@pytest.mark.parametrize("n_list", (1, 15, 16, 17))
def test_c_d_list_a_around_the_claim_block(gpus, forged, n_list):
    """list A of 1, 15, 16 and 17 reads between plain ones: k_score_many's claim blocks of 16 under a fixed grid"""
    w, r = forged
    (p, n), = three_ways(gpus, w, [pick(r, PLAIN[:2] + list(range(n_list)) + PLAIN[2:])])
    assert (n["a"], n["many"], n["b"]) == (n_list, n_list, 0), n


def test_e_list_b_behind_list_a(gpus, forged):
    """tails of 72 slots: two reads overflow (A), two keep 66 and 72 tail matches -- more than k_score_fast merges, and with them more
    matches than the generic kernel stages (B): the tier runs again for B behind the join of the streams"""
    w, r = forged
    (p, n), = three_ways(gpus, w, [pick(r, PLAIN[:2] + [B66, A75, B72, A80] + PLAIN[2:])], tail_min=72)
    assert p["stride"] - p["direct"] == 72 and (n["a"], n["generic"], n["b"], n["many"]) == (2, 2, 2, 4), (p, n)


def test_f_reads_the_first_tier_kernel_hands_on(gpus, forged):
    """193 survivors: k_many_sort<11, 2048> + k_score_long; more than 4096: flagged by both k_many_sort launches, exact segments behind the join"""
    w, r = forged
    (p, n), = three_ways(gpus, w, [pick(r, PLAIN[:1] + [0, STAGE193, 1, BEYOND4096, 2] + PLAIN[1:])])
    assert (n["a"], n["many"], n["sorted"], n["exact"], n["b"]) == (5, 3, 1, 1, 0), n


def test_g_two_batches_back_to_back(gpus, forged):
    """events, lists and counters are the context's: a batch of 22 reads (list A of 17, one read for each later tier), then one of 3 (list A of 1)"""
    w, r = forged
    (p1, n1), (p2, n2) = three_ways(gpus, w, [pick(r, list(range(N_OVF)) + [STAGE193, BEYOND4096] + PLAIN[:3]), pick(r, [PLAIN[3], 5, PLAIN[4]])])
    assert (n1["a"], n1["sorted"], n1["exact"]) == (N_OVF + 2, 1, 1) and (n2["a"], n2["many"]) == (1, 1), (n1, n2)


def test_h_pairs(orc, gpus, base, tmp_path):
    """fast<3,3,true>: pairs of 75-base mates, the first mate's metamers filed under dead species beyond the tail for four of the seven"""
    pairs = [cut(20000 - 1200 - 400 * i, 2 * MATE + 40) for i in range(7)]
    m1 = [s[:MATE].copy() for s in pairs]
    m2 = [D.revcomp(s[-MATE:]) for s in pairs]
    a, b = as_reads(m1), as_reads(m2)
    rr = Reads(a.b1, a.o1, b.b1, b.o1)
    ref0 = orc.classify(base.db, base.tax, _op(2), rr.b1, rr.o1, rr.b2, rr.o2)
    p0, _ = plan(ref0, rr.n, paired=True)
    assert p0["bucket"] == "fast<3,3,true>", p0
    tail_cap, free = p0["stride"] - p0["direct"], max(_world().tax.parent) + 1
    f0 = per_read(ref0, rr.n)
    parts = [copies(single_values(orc, m1[i]), tail_cap - f0[i]["cur"] + 1 + i, free + 1000 + np.arange(200)) for i in range(4)]
    w = Forge(orc, tmp_path / "pairs", (np.concatenate([q[0] for q in parts]), np.concatenate([q[1] for q in parts])))
    (p, n), = three_ways(gpus, w, [rr], seq_mode=2)
    assert p["bucket"] == "fast<3,3,true>" and (n["a"], n["many"], n["b"]) == (4, 4, 0), (p, n)
