"""The long-read slot path at the edges of its tables and tails, against the oracle: score_long_slots (mtb_api.hip), k_join_dir<.., LONG>
(kernels_dir.h), k_seg_order / k_lbig_count / k_lbig_copy / k_lslot_sizes (kernels_seg_order.h) and the second dev_score_long launch on
the reads k_seg_order lists.  The forged edge cases and `quarters` compare every row bit for bit, nothing masked; loop-640 and
order-inside-a-species rest on chosen seeds and mask the few rows the oracle flags as ambiguous.  Every case asserts through
mtb_batch_stats (lslot_tail_factor, n_lslot_big_reads, n_slot_reads) that the batch took the route its id names.

`long_slot_plan` mirrors the dispatch from the oracle's answer alone.  The rules and where they stand:

  per read r
    d_r      its metamers: the extractor's per-read count (classify_attempt: xo.d_counts), here the oracle's k-mer list
    t_r      its tail matches = matches - matched metamers.  k_join_dir<.., LONG> (kernels_dir.h, `first = ord < direct`; "the selected candidate
             with the lowest index takes the query's ordinal slot, the others the read's tail"): the first selected candidate of a metamer
             is stored at slot ord, every further one advances the read's tail cursor (sa.cursor[r])
    tcap     mtb_lslot_tail(d, tf) = ((d * tf) >> 2) + 16 for d > 0, else 0 (mtb_core.h); a match at cursor >= tcap is only counted
             (ovf_put: `if (LONG) return`), and dev_join then reports MTB_ERR_CAPACITY
    cand_r   species that enter k_seg_order's exact table: those whose bucket so_bloom(species) = (species * 0x85EBCA6B mod 2^32) >> 16 was
             marked twice in pass 1 (`twice`), i.e. holds at least two of the read's matches -- of one species or of several
  batch (score_long_slots' loop `for (tf = c->lslot_tf_start; tf <= 4 && !*done; tf *= 4)`)
    tf       the first of (tf_start, 4) with t_r <= tcap(d_r, tf) for every read; tf_start is 1 on a fresh context and 4 after a batch whose
             join overflowed at 1 (`c->lslot_tf_start = 4`).  None: *done stays false, classify_one redoes the range on exact segments --
             n_slot_reads == 0 and lslot_tail_factor == 0
  read     big (fail_list -> k_lbig_count / k_lbig_copy -> k_segsort_lds -> the second dev_score_long) iff t_r > MTB_SO_TAIL = 2048
           (`cur > MTB_SO_TAIL`) or cand_r > MTB_SO_MAXSP = 768 (slot_of: `atomicAdd(&s_nsp, 1u) >= MTB_SO_MAXSP`)

Forged worlds (as test_gpu_parity.py::test_many_matches_per_query_take_the_large_segment_path): the two-genus world of conftest.HotToy, an
error-free read cut from genome 0, and chosen metamers of that read filed once more, unchanged, under new species of genus 0.  An exact
copy has hamming 0 -- always selected -- and stands behind the genome's own entry in the index (same value, higher species id), so k
copies under one species add exactly k tail matches and one species.  Every size is derived inside the test from the oracle's counts of
the unforged world, and every case asserts the forged world's plan before it looks at the library.
So that the rows are MADE of forged tail matches (a species of a few scattered copies never reaches a row), most edge reads are a short
genome cut followed by random filler that matches nothing (`chimera`: the metamers, and with them the slot range and the tail, follow the
whole length), and one forged species -- the rival -- files every metamer of the genome part (tail matches) and some filler metamers
(direct slots of its own): it beats the genome's species, and classification, score and count list are its own (`assert_edge_read`).

The emulated build runs the same cases but the last (tests/test_hipemu.py); atomics, wave barriers and work stealing are the GPU's."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K_JOIN = 4                                             # include/mtb.h MTB_K_JOIN (mtb_batch_stats.n_launch, profiling on)
SO_TAIL, SO_MAXSP, SO_HASH = 2048, 768, 1024           # kernels_seg_order.h MTB_SO_TAIL / MTB_SO_MAXSP / MTB_SO_HASH
SO_GRID = 512                                          # score_long_slots: k_seg_order runs min(n_reads, 512) workgroups
WORLD_SEED = 91
GENUS0 = 4                                             # synth.make_world: root 1, Bacteria 2, Eukaryota 3, the first genus 4


# ------------------------------------------------------------------ the dispatch, mirrored
def so_bloom(species):
    """kernels_seg_order.h so_bloom: the 16-bit bucket of the seen-once / seen-twice bit arrays"""
    return ((np.asarray(species).astype(np.uint64) * np.uint64(0x85EBCA6B)) & np.uint64(0xFFFFFFFF)) >> np.uint64(16)


def so_hash(species):
    """kernels_seg_order.h so_hash: the 10-bit home slot in the exact species table"""
    return ((np.asarray(species).astype(np.uint64) * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)) >> np.uint64(22)


def tcap(d, tf):
    """mtb_core.h mtb_lslot_tail"""
    d = np.asarray(d, np.int64)
    return np.where(d > 0, ((d * tf) >> 2) + 16, 0)


def match_reads(m):
    """0-based read of every match (or of every qinfo value)"""
    q = m["qinfo"] if m.dtype.names else m
    return (((q >> np.uint64(32)) & np.uint64(0x1FFFFFFF)).astype(np.int64)) - 1


def long_slot_plan(ref, n_reads, tf_start):
    """score_long_slots' route for a batch from the oracle's k-mers and matches (module docstring): per read d, t, cand and big; the
    batch's tail factor (0: redone on exact segments), n_slot_reads, the big reads, and the factor the next batch starts with"""
    from test_gpu_scorer_tiers import metamers_per_read
    d = metamers_per_read(ref["kmers"], n_reads).astype(np.int64)
    m = ref["matches"]
    rd = match_reads(m)
    n_m = np.bincount(rd, minlength=n_reads)
    n_q = np.bincount(match_reads(np.unique(m["qinfo"])), minlength=n_reads)           # matched metamers: one (read, frame, position) each
    t = n_m - n_q
    sp = m["species_id"].astype(np.int64)
    rb, rb_cnt = np.unique((rd << 16) | so_bloom(sp).astype(np.int64), return_counts=True)          # (read, bucket) -> matches
    cand = np.zeros(n_reads, np.int64)
    if len(m):
        rs = np.unique(np.stack([rd, sp], 1), axis=0)                                                # (read, species)
        hot = rb_cnt[np.searchsorted(rb, (rs[:, 0] << 16) | so_bloom(rs[:, 1]).astype(np.int64))] >= 2
        cand = np.bincount(rs[hot, 0], minlength=n_reads)
    tries = [tf_start] if tf_start == 4 else [tf_start, 4]
    tf = next((f for f in tries if (t <= tcap(d, f)).all()), 0)
    big = ((t > SO_TAIL) | (cand > SO_MAXSP)) if tf else np.zeros(n_reads, bool)
    tf_next = 4 if tf_start == 4 or (t > tcap(d, 1)).any() else 1
    return dict(d=d, t=t, cand=cand, tf=tf, big=np.flatnonzero(big), n_slot_reads=n_reads if tf else 0, tf_next=tf_next, joins=tries.index(tf) + 1 if tf else None)


# ------------------------------------------------------------------ worlds
def _p3():
    from helpers import default_params
    return default_params(seq_mode=3, syncmer=1)


def _world():
    from metabuli_amd import synth
    return synth.make_world(seed=WORLD_SEED, n_genera=2, species_per_genus=2, strains_per_species=1, genome_len=20000, with_euk=False)


class Db:
    """the two-genus world, optionally with forged entries (values, taxids) under new species of genus 0, and the oracle on it"""

    def __init__(self, orc, dbdir, forged=None):
        from helpers import build_toy_db
        self.orc, self.dbdir, self.world = orc, str(dbdir), _world()
        os.makedirs(self.dbdir, exist_ok=True)
        extra = None
        if forged is not None:
            fv, ft = forged
            for s in np.unique(ft):
                self.world.tax.add(int(s), GENUS0, "species", f"forged{int(s)}")
            extra = (np.asarray(fv, np.uint64), np.asarray(ft, np.int32))
        self.values, self.taxids = build_toy_db(orc, self.world, _p3(), self.dbdir, extra=extra)
        self.tax = orc.load_taxonomy(os.path.join(self.dbdir, "taxonomy"))
        self.db = orc.open_db(self.dbdir, self.tax, _p3())

    def classify(self, r):
        return self.orc.classify(self.db, self.tax, _p3(), r.b1, r.o1)


def one_read(bases):
    from test_gpu_scorer_tiers import Reads
    return Reads(np.ascontiguousarray(bases), np.array([0, len(bases)], np.uint64))


def cut(start, length):
    """an error-free read of genome 0"""
    return one_read(_world().genomes[0][1][start:start + length].copy())


def first_free_taxid():
    return max(_world().tax.parent) + 1


def single_values(orc, r, last=None):
    """the metamer values that occur exactly once in the one read r -- a copy of one of them under a new species adds exactly one match --
    those of the read `last` (if given) at the end"""
    k, _, _ = orc.extract_batch(_p3(), r.b1, r.o1)
    v, c = np.unique(k["value"], return_counts=True)
    v = v[c == 1]
    if last is not None:
        kl, _, _ = orc.extract_batch(_p3(), last.b1, last.o1)
        inl = np.isin(v, kl["value"])
        v = np.concatenate([v[~inl], v[inl]])
    return v


def spread(values, n_copies, species):
    """n_copies distinct (value, species) entries: values in turn, species in turn (shifted by one on every further lap over the values)"""
    j = np.arange(n_copies, dtype=np.int64)
    v, s = j % len(values), (j + j // len(values)) % len(species)
    assert len(np.unique(v * len(species) + s)) == n_copies, (n_copies, len(values), len(species))
    return np.asarray(values)[v], np.asarray(species, np.int32)[s]


def chimera(g_len, total, start=3000, filler_first=False):
    """a read of `total` bases of which g_len are an error-free cut of genome 0 and the rest seeded random filler that matches nothing: the
    read's metamers (and so its slot range and its tail) follow `total`, its own species scores on the genome part only"""
    g = _world().genomes[0][1][start:start + g_len]
    fill = np.frombuffer(b"ACGT", np.uint8)[np.random.default_rng(1000 * g_len + total).integers(0, 4, size=total - g_len)]
    return one_read(np.concatenate([fill, g] if filler_first else [g, fill]))


def rival_values(orc, base, r):
    """what makes a forged species the WINNER of the one read r, so that the row (classification, score, count list) is made of forged
    matches: (tail, direct) = the read's single metamer values the unforged index holds -- a copy stands behind the genome's own entry: a
    tail match each -- and the filler's single values, in the extractor's order -- nothing else matches them: filed, they take their
    metamers' direct slots.  The rival files all of `tail` and enough of `direct` to beat the genome's species beyond the tie ratio."""
    k, _, _ = orc.extract_batch(_p3(), r.b1, r.o1)
    v, c = np.unique(k["value"], return_counts=True)
    single = v[c == 1]
    held = np.isin(single, base.values)
    kv = k["value"][np.isin(k["value"], single[~held])]
    return single[held], kv


def rival_entries(tail, direct, rival):
    """the rival's entries: every tail value and a fifth as many (at least 40) filler values"""
    n_direct = min(len(direct), max(40, len(tail) // 5))
    fv = np.concatenate([tail, direct[len(direct) - n_direct:]])
    return fv, np.full(len(fv), rival, np.int32)


def join_entries(*parts):
    return np.concatenate([p[0] for p in parts]), np.concatenate([np.asarray(p[1], np.int32) for p in parts])


@pytest.fixture(scope="module")
def base(orc, tmp_path_factory):
    return Db(orc, tmp_path_factory.mktemp("lslot_base"))


def base_counts(base, r):
    """(d, t, cand) of the one read r in the unforged world"""
    pl = long_slot_plan(base.classify(r), 1, 1)
    return int(pl["d"][0]), int(pl["t"][0]), int(pl["cand"][0])


# ------------------------------------------------------------------ running a batch
def check_rows(ref, res, tt, tc, tag, masked=None):
    """classification, fp32 score bits, n_taxcnt and the taxID:count lists of every read not in `masked`"""
    ro = ref["results"]
    keep = np.ones(len(ro), bool) if masked is None else ~masked
    assert len(res) == len(ro), tag
    assert (res["classification"] == ro["classification"])[keep].all(), (tag, np.flatnonzero((res["classification"] != ro["classification"]) & keep)[:8])
    assert (res["score"].view(np.uint32) == ro["score"].view(np.uint32))[keep].all(), (tag, np.flatnonzero((res["score"].view(np.uint32) != ro["score"].view(np.uint32)) & keep)[:8])
    assert (res["n_taxcnt"] == ro["n_taxcnt"])[keep].all(), tag
    for i in np.flatnonzero(keep):
        a, b, n = int(res["taxcnt_off"][i]), int(ro["taxcnt_off"][i]), int(ro["n_taxcnt"][i])
        assert (tt[a:a + n] == ref["tc_tax"][b:b + n]).all() and (tc[a:a + n] == ref["tc_cnt"][b:b + n]).all(), (tag, i)


def run_route(dbdir, r, ref, tag, calls=2, masked=None, ctx=None):
    """the batch `calls` times on one fresh context (so the second call starts with the tail factor the first left behind), then under
    MTB_NO_LONG_SLOTS: the oracle's rows, the plan's counters, identical arrays.  Returns the plans of the calls."""
    import metabuli_amd as M
    c = ctx or M.Context(0)
    c.set_profiling(True)
    p = M.default_params(seq_mode=3, syncmer=1)
    ix = c.open_index(dbdir, p)
    plans = []
    try:
        tf_start, first = 1, None
        for call in range(calls):
            pl = long_slot_plan(ref, r.n, tf_start)
            res, tt, tc = c.classify_batch(ix, p, r.b1, r.o1)
            st = c.last_stats()
            t2 = (tag, "call", call, "plan", pl["tf"], pl["big"], "got", st.lslot_tail_factor, st.n_lslot_big_reads, st.n_slot_reads)
            assert (st.lslot_tail_factor, st.n_lslot_big_reads, st.n_slot_reads) == (pl["tf"], len(pl["big"]), pl["n_slot_reads"]), t2
            assert st.n_matches == len(ref["matches"]) and st.n_reads == r.n, (t2, st.n_matches, len(ref["matches"]))
            check_rows(ref, res, tt, tc, t2, masked)
            if first is None:
                first = (res.copy(), tt.copy(), tc.copy(), st.n_launch[K_JOIN])
            elif pl["joins"] and plans[0]["joins"]:                 # joins of this call against the first call's, by the plans' attempts
                assert st.n_launch[K_JOIN] * plans[0]["joins"] == first[3] * pl["joins"], (t2, st.n_launch[K_JOIN], first[3])
            plans.append(pl)
            tf_start = pl["tf_next"]
        c.set_option("MTB_NO_LONG_SLOTS", "1")
        res, tt, tc = c.classify_batch(ix, p, r.b1, r.o1)
        st = c.last_stats()
        assert (st.lslot_tail_factor, st.n_lslot_big_reads, st.n_slot_reads) == (0, 0, 0), tag
        assert st.n_matches == len(ref["matches"]), tag
        assert (res == first[0]).all() and (tt == first[1]).all() and (tc == first[2]).all(), tag
    finally:
        c.set_option("MTB_NO_LONG_SLOTS", None)
        ix.close()
        if ctx is None:
            c.close()
    return plans


def assert_edge_read(ref, i=0, winner=None):
    """an edge read is compared unmasked: the oracle must have scored it without an ambiguity flag -- and, where a forged species is
    to carry the row, for that species, with its count list"""
    row = ref["results"][i]
    assert row["flag"] == 0 and row["is_classified"] != 0, row
    if winner is not None:
        a, n = int(row["taxcnt_off"]), int(row["n_taxcnt"])
        assert row["classification"] == winner and ref["tc_tax"][a:a + n].tolist() == [winner] and ref["tc_cnt"][a] > 10, (row, ref["tc_tax"][a:a + n])


# ------------------------------------------------------------------ the tables' edges
SPECIES_GENOME = (3000, 110)                          # the genome part of the species-768 / 769 read: (start, bases)


def species_world(orc, base, tmpdir, n_cand):
    """a 6.5 kb read whose candidate species number n_cand: the genome's, a rival that wins the read with tail copies of every metamer of
    the short genome part, and further species with two of those metamers each -- all inside the tail of a quarter"""
    r = chimera(SPECIES_GENOME[1], 6500, start=SPECIES_GENOME[0])
    d, t0, cand0 = base_counts(base, r)
    tail, direct = rival_values(orc, base, r)
    rival = first_free_taxid()
    n_sp = n_cand - cand0 - 1
    sp = rival + 1 + np.arange(n_sp)
    j = np.arange(2 * n_sp)
    two_each = (tail[j % len(tail)], sp[j // 2])                       # (consecutive values: two different ones per species)
    assert len(tail) >= 2 and t0 + len(tail) + 2 * n_sp <= min(tcap(d, 1), SO_TAIL), (d, t0, cand0, len(tail))       # the species limit alone decides
    return Db(orc, tmpdir, join_entries(rival_entries(tail, direct, rival), two_each)), r, rival


@pytest.mark.parametrize("n_cand", [SO_MAXSP, SO_MAXSP + 1], ids=["species-768", "species-769"])
def test_candidate_species_at_the_table_limit(orc, base, tmp_path, n_cand):
    """768 candidate species fill k_seg_order's exact table to its cap; the 769th insertion hands the read on: fail list, k_lbig_count /
    k_lbig_copy, k_segsort_lds, second dev_score_long.  The read's winner is a forged species whose matches lie in the tail."""
    w, r, rival = species_world(orc, base, tmp_path / "db", n_cand)
    ref = w.classify(r)
    pl = long_slot_plan(ref, 1, 1)
    assert pl["cand"][0] == n_cand and pl["t"][0] <= min(SO_TAIL, tcap(pl["d"][0], 1)), pl
    assert (pl["tf"], len(pl["big"])) == (1, int(n_cand > SO_MAXSP)), pl
    assert_edge_read(ref, winner=rival)
    run_route(w.dbdir, r, ref, f"species-{n_cand}")


@pytest.mark.parametrize("n_tail", [SO_TAIL, SO_TAIL + 1], ids=["tail-2048", "tail-2049"])
def test_tail_matches_at_the_lds_limit(orc, base, tmp_path, n_tail):
    """2048 tail matches fill t_key / t_idx / t_diff and the bitonic network's full width; 2049 (inside the read's tail slots: a 9 kb read)
    are beyond them.  The read's winner is a forged species with some 1800 of those tail matches; 63 more species share the rest."""
    r = chimera(1800, 9000)
    d, t0, cand0 = base_counts(base, r)
    assert tcap(d, 1) >= SO_TAIL + 1, d
    tail, direct = rival_values(orc, base, r)
    rival = first_free_taxid()
    rest = n_tail - t0 - len(tail)
    assert rest >= 2 * 63, (n_tail, t0, len(tail))
    w = Db(orc, tmp_path / "db", join_entries(rival_entries(tail, direct, rival), spread(tail, rest, rival + 1 + np.arange(63))))
    ref = w.classify(r)
    pl = long_slot_plan(ref, 1, 1)
    assert pl["t"][0] == n_tail and pl["cand"][0] == cand0 + 64, pl
    assert (pl["tf"], len(pl["big"])) == (1, int(n_tail > SO_TAIL)), pl
    assert_edge_read(ref, winner=rival)
    run_route(w.dbdir, r, ref, f"tail-{n_tail}")


# ------------------------------------------------------------------ the tails' edges
@pytest.mark.parametrize("tf,over", [(1, 0), (1, 1), (4, 0), (4, 1)], ids=["tf1-full", "tf1-over", "tf4-full", "tf4-over"])
def test_tail_cursor_at_the_slot_range_limit(orc, base, tmp_path, tf, over):
    """a read whose tail cursor ends at mtb_lslot_tail(d, tf) exactly, and one above: tf 1 full stays at 1; one above goes to 4 and the
    context keeps 4 (the second call joins once; a read without tail matches reports 4 there and 1 on a fresh context); tf 4 full stays
    at 4; one above is redone on exact segments, call after call.  The read's winner is a forged species whose matches fill most of the
    tail (tf 4: more tail matches than a quarter -- a second species over the same metamers brings them up to the limit)."""
    import metabuli_amd as M
    r, short = chimera(280 if tf == 1 else 1000, 1200), cut(9000, 300)
    d, t0, cand0 = base_counts(base, r)
    n_tail = int(tcap(d, tf)) + over
    tail, direct = rival_values(orc, base, r)
    rival = first_free_taxid()
    rest = n_tail - t0 - len(tail)
    sp = rival + 1 + np.arange(7 if tf == 1 else 1)
    assert 2 * len(sp) <= rest <= len(tail), (n_tail, t0, len(tail))
    w = Db(orc, tmp_path / "db", join_entries(rival_entries(tail, direct, rival), spread(tail, rest, sp)))
    ref = w.classify(r)
    pl = long_slot_plan(ref, 1, 1)
    assert pl["d"][0] == d and pl["t"][0] == n_tail and n_tail <= SO_TAIL and pl["cand"][0] <= SO_MAXSP, pl
    want = {(1, 0): (1, 1, 1), (1, 1): (4, 4, 2), (4, 0): (4, 4, 2), (4, 1): (0, 4, None)}[(tf, over)]
    assert (pl["tf"], pl["tf_next"], pl["joins"]) == want and len(pl["big"]) == 0, pl
    assert_edge_read(ref, winner=rival)
    plans = run_route(w.dbdir, r, ref, f"tf{tf}-{'over' if over else 'full'}")
    assert (plans[1]["tf"], plans[1]["joins"]) == (want[0], 1 if want[0] else None), plans[1]
    if (tf, over) == (1, 1):
        refs = w.classify(short)
        ps = long_slot_plan(refs, 1, 1)
        assert ps["tf"] == 1 and ps["tf_next"] == 1 and long_slot_plan(refs, 1, 4)["tf"] == 4, ps
        p = M.default_params(seq_mode=3, syncmer=1)
        for sticky in (True, False):
            c = M.Context(0)
            ix = c.open_index(w.dbdir, p)
            try:
                if sticky:
                    c.classify_batch(ix, p, r.b1, r.o1)
                    assert c.last_stats().lslot_tail_factor == 4
                res, tt, tc = c.classify_batch(ix, p, short.b1, short.o1)
                st = c.last_stats()
                assert (st.lslot_tail_factor, st.n_lslot_big_reads, st.n_slot_reads) == (4 if sticky else 1, 0, 1), sticky
                check_rows(refs, res, tt, tc, ("short", sticky))
            finally:
                ix.close(); c.close()


# ------------------------------------------------------------------ the wave quarters
QUARTER_D = [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025]


def test_quarters(orc, base):
    """k_seg_order cuts a read's direct slots into four wave quarters of whole 64-slot steps (q_len): reads of 1, 63 / 64 / 65, 255 / 256 /
    257 and 1023 / 1024 / 1025 metamers (one partial step, one step, quarters of one and of four steps and one slot more) without a tail
    match, a read too short for a metamer and a random read without a match, in one batch"""
    from test_gpu_scorer_tiers import Reads, metamers_per_read
    g0 = base.world.genomes[0][1]
    reads = []
    for want in QUARTER_D:                        # prefixes of cuts of genome 0: the oracle's counts pick start and length
        found = None
        for start in range(3000, 3040):
            lens = np.arange(max(24, want - 40), want + 120)
            offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
            bases = np.concatenate([g0[start:start + n] for n in lens])
            k, _, _ = orc.extract_batch(_p3(), bases, offs)
            hit = np.flatnonzero(metamers_per_read(k, len(lens)) == want)
            for h in hit:
                cand = one_read(g0[start:start + lens[h]].copy())
                if long_slot_plan(base.classify(cand), 1, 1)["t"][0] == 0:
                    found = cand
                    break
            if found is not None:
                break
        assert found is not None, want
        reads.append(found)
    reads.append(one_read(g0[100:120].copy()))
    reads.append(one_read(np.frombuffer(b"ACGT", np.uint8)[np.random.default_rng(5).integers(0, 4, size=700)]))
    r = reads[0]
    for x in reads[1:]:
        r = r + x
    ref = base.classify(r)
    pl = long_slot_plan(ref, r.n, 1)
    assert pl["d"].tolist() == QUARTER_D + [0, pl["d"][-1]] and pl["d"][-1] > 0 and (pl["t"] == 0).all(), pl
    assert np.bincount(match_reads(ref["matches"]), minlength=r.n)[-2:].tolist() == [0, 0]
    assert (pl["tf"], len(pl["big"])) == (1, 0), pl
    ro = ref["results"]
    # unmasked: no flag anywhere; every read of a full step and more is classified (a read of one metamer, of none and the random read cannot be)
    assert (ro["flag"] == 0).all() and (ro["is_classified"][1:len(QUARTER_D)] != 0).all(), ro
    run_route(base.dbdir, r, ref, "quarters")


# ------------------------------------------------------------------ bloom collisions and dropped markers
def test_bloom_collision(orc, base, tmp_path):
    """Two species D0, D1 with ONE match each whose ids share a 16-bit bucket: the bucket is seen twice, both enter the exact table, both
    are dropped by the exact count and leave their markers in the probe chains.  K1, the forged WINNER of the read, and K2 (two matches)
    have D0's home slot in the table: whichever of the three is inserted first, a kept species stands behind D0's marker unless D0 comes
    last -- and D0's match is a filler metamer at the read's start (a direct slot of the first wave's first step), K1's and K2's are
    tail matches, which every wave reaches after its direct slots.  A lookup that stops at a foreign marker loses the winner.  A species
    with one match and a bucket of its own never enters the table.  The dropped matches still count in n_matches."""
    r = chimera(280, 1200, filler_first=True)
    ref0 = base.classify(r)
    own = np.unique(ref0["matches"]["species_id"])
    ids = first_free_taxid() + np.arange(1 << 17)             # (consecutive ids spread evenly over the buckets: the nearest pair is tens of thousands apart)
    b, h = so_bloom(ids), so_hash(ids)
    free = ~np.isin(b, so_bloom(own))                         # buckets that no species of the unforged read has
    o = np.argsort(b, kind="stable")
    adj = np.flatnonzero((b[o][1:] == b[o][:-1]) & free[o][1:])
    at = adj[np.argmin(ids[o][adj + 1])]                      # two ids with one bucket, the pair with the lowest ids ...
    pair = (int(ids[o][at]), int(ids[o][at + 1]))
    free &= ~np.isin(b, so_bloom(pair))
    k1, k2 = (int(x) for x in ids[np.flatnonzero(free & (h == so_hash(pair[0])))[:2]])       # ... two more with the home slot of the first and buckets of their own ...
    assert so_bloom(k1) != so_bloom(k2)
    free &= ~np.isin(b, so_bloom([k1, k2]))
    lone = int(ids[np.flatnonzero(free & (h != so_hash(pair[0])) & (h != so_hash(pair[1])))[0]])      # ... a fifth that shares nothing with them
    tail, direct = rival_values(orc, base, r)
    fv, ft = join_entries(rival_entries(tail, direct, k1), (direct[:2], pair), (tail[[100, 200]], [k2, k2]), (tail[[150]], [lone]))
    w = Db(orc, tmp_path / "db", (fv, ft))
    ref = w.classify(r)
    m = ref["matches"]
    per = {s: int((m["species_id"] == s).sum()) for s in pair + (k2, lone)}
    assert per == {pair[0]: 1, pair[1]: 1, k2: 2, lone: 1}, per
    assert so_bloom(pair[0]) == so_bloom(pair[1]) and so_hash(k1) == so_hash(k2) == so_hash(pair[0])
    first = m[m["species_id"] == pair[0]][0]                   # D0's match: alone at its metamer (a direct slot), in the first 64 bases of frame 0 / 1 / 2
    assert (m["qinfo"] == first["qinfo"]).sum() == 1 and int(first["qinfo"] & np.uint64(0xFFFFFFFF)) < 64, first
    others = np.setdiff1d(np.unique(m["species_id"]), [lone])
    assert so_bloom(lone) not in set(so_bloom(others).tolist())
    pl0, pl = long_slot_plan(ref0, 1, 1), long_slot_plan(ref, 1, 1)
    assert pl["cand"][0] == pl0["cand"][0] + 4 and pl["t"][0] == pl0["t"][0] + len(tail) + 3, (pl0, pl)
    assert (pl["tf"], len(pl["big"])) == (1, 0), pl
    assert_edge_read(ref, winner=k1)
    run_route(w.dbdir, r, ref, "bloom-collision")


# ------------------------------------------------------------------ more reads than workgroups
def test_loop_640(orc, base, tmp_path):
    """640 reads on a grid of 512 workgroups: a workgroup that comes back for another read clears the aliased LDS again and starts from
    s_bad = 0 -- after one of the four species-769 reads (beyond the exact table) as after any other; 20-base reads without a metamer in
    between.  The other reads are cuts of genome 0 that keep clear of the metamers the 769 species are filed on."""
    from test_gpu_scorer_tiers import Reads
    w, big, rival = species_world(orc, base, tmp_path / "db", SO_MAXSP + 1)
    g0 = w.world.genomes[0][1]
    rng = np.random.default_rng(640)
    lo, hi = SPECIES_GENOME[0], SPECIES_GENOME[0] + SPECIES_GENOME[1]

    def clear_cut(n):
        while True:
            st = int(rng.integers(0, len(g0) - n))
            if st + n <= lo or st >= hi:
                return g0[st:st + n]
    seqs = []
    for i in range(640):
        seqs.append(big.b1 if i % 160 == 159 else clear_cut(20) if i % 97 == 96 else clear_cut(int(rng.integers(200, 901))))
    r = Reads(np.concatenate(seqs), np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.uint64))
    assert r.n == 640 > SO_GRID
    ref = w.classify(r)
    pl = long_slot_plan(ref, r.n, 1)
    assert pl["big"].tolist() == [159, 319, 479, 639] and pl["tf"] in (1, 4) and pl["n_slot_reads"] == 640, pl
    assert (pl["d"][96::97] == 0).all()
    masked = ref["results"]["flag"] != 0
    assert masked.sum() * 50 <= r.n and not masked[pl["big"]].any(), masked.sum()
    for i in pl["big"]:
        assert_edge_read(ref, int(i), winner=rival)
    run_route(w.dbdir, r, ref, "loop-640", masked=masked)


# ------------------------------------------------------------------ rank merge of tail against direct matches
ORDER_SEED = 12


def hamming_orders(m):
    """pairs of matches of ONE species at ONE (read, frame, position) with different hamming: how many have the smaller hamming at the
    lower target index (the direct slot) and how many at the higher (the tail).  Two targets of a species that one query matches share
    the amino-acid part, so the index orders them by their DNA part."""
    o = np.lexsort((m["dna"], m["species_id"], m["qinfo"]))
    a, b = m[o][:-1], m[o][1:]
    same = (a["qinfo"] == b["qinfo"]) & (a["species_id"] == b["species_id"]) & (a["ham"] != b["ham"])
    rd = match_reads(a)
    return rd[same & (a["ham"] < b["ham"])], rd[same & (a["ham"] > b["ham"])]


def test_order_inside_a_species(orc, tmp_path):
    """noisy lognormal long reads on a world with two strains per species (conftest TOY_MODES["sync_long"], another seed): a metamer matches
    both strains' entries of one species with different hamming -- the one in the direct slot is the lower target index, not the smaller
    hamming, so k_seg_order's rank merge has to put a tail match BEFORE a direct match of the same species and position, and after it.
    (On the emulated build, a merge that ranks every direct match before its species' tail, or that forgets the other species' share of
    the difference array, fails here and in no other case of this file.  The scorers do not look at the order of two matches of one
    position, so a sort key without the hamming bits still passes: that order is beyond what a result can show.)"""
    from conftest import Toy, TOY_MODES
    from test_gpu_scorer_tiers import Reads
    t = Toy(orc, tmp_path / "db", **dict(TOY_MODES["sync_long"], seed=ORDER_SEED))
    r = Reads(t.b1, t.o1)
    lower_first, higher_first = hamming_orders(t.ref["matches"])
    assert len(lower_first) and len(higher_first) and len(np.intersect1d(lower_first, higher_first)), (len(lower_first), len(higher_first))
    pl = long_slot_plan(t.ref, r.n, 1)
    assert pl["tf"] in (1, 4) and pl["n_slot_reads"] == r.n, pl
    masked = t.ref["results"]["flag"] != 0
    assert masked.sum() * 50 <= r.n and not masked[pl["big"]].any(), masked.sum()
    both = np.intersect1d(lower_first, higher_first)
    assert (~masked[both]).any() and (t.ref["results"]["is_classified"][both[~masked[both]]] != 0).any()
    run_route(t.dbdir, r, t.ref, "order-inside-a-species", masked=masked)
