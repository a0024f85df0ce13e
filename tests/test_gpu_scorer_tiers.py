"""Every run-time choice of the short-read path against the oracle: the k_score_fast instantiations by slot stride, the generic
slot k_score by LDS cap, the tiers of the deferred reads (k_score_many, k_many_sort + k_score_long, exact segments), the slot
buffer's clearing and placement, the long-read scorers, the fused amino-acid sort and the partitioned stage calls -- each with the
MTB_* switches that select among them (mtb_options.h: "none changes a result").  One oracle answer per synthetic world, reused for
every switch setting on one context; every case compares bit for bit and asserts through mtb_batch_stats that its path ran.

`slot_plan` mirrors the dispatch of mtb_api.hip (classify_attempt, slot_geometry, dev_score, score_fixed_slots) from the oracle's
metamer counts, and every case asserts that it landed in the bucket its id names -- so the parametrisation cannot drift from the
boundaries it is there to cover.  SWITCH_CASES lists which case covers which switch; test_abi.py checks it against mtb_options.h."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K_EXTRACT_EMIT, K_SCORE, K_SCORE_FAST, K_SCORE_MANY = 1, 7, 9, 10           # include/mtb.h kernel ids (mtb_batch_stats.n_launch, profiling on)
SLOT_MAX_Q, SLOT_MAX_POS = 384, 4096                    # mtb_core.h MTB_SLOT_MAX_Q / MTB_SLOT_MAX_POS
SORT_TILE = 512 * 8                                      # the fused sort's scatter tile (512 threads x MTB_SORT_ITEMS)

# every MTB_* switch of mtb_options.h and the case(s) of this file that run it against the oracle (checked by test_abi.py)
SWITCH_CASES = {
    "MTB_JOIN_VARIANT": "test_gpu_parity.py::test_target_windows_staged_in_lds_give_the_same_matches",
    "MTB_JOIN_WIN": "test_fused_sort_variants_at_tile_edges, test_long_read_scorer_switches",
    "MTB_JOIN_WIN_QT": "test_fused_sort_variants_at_tile_edges",
    "MTB_JOIN_COOP_MIN": "test_gpu_parity.py::test_runs_of_a_dozen_candidates_inside_and_outside_a_window",
    "MTB_SORT_LSD": "test_fused_sort_variants_at_tile_edges",
    "MTB_SORT_NO_XCD": "test_fused_sort_variants_at_tile_edges",
    "MTB_SORT_PAIRS": "test_fused_sort_variants_at_tile_edges",
    "MTB_NO_SCORE_MANY": "test_deferred_chain",
    "MTB_NO_MANY_SORT": "test_deferred_chain",
    "MTB_MANY_CAP": "test_deferred_chain",
    "MTB_NO_FAST_SCORER": "test_stride_matrix",
    "MTB_NO_FAST_PAIRS": "test_stride_matrix",
    "MTB_NO_LONG_SCORER": "test_long_read_scorer_switches",
    "MTB_NO_LONG_SLOTS": "test_long_read_scorer_switches",
    "MTB_TAIL_MIN": "test_deferred_chain",
    "MTB_SCRATCH_ALIAS": "test_deferred_chain",
    "MTB_NO_DIR": "test_partitioned.py::test_gpu_partitioned_long_runs_and_the_bisection_fallback",
    "MTB_DIR_DEPTH": "test_fused_sort_variants_at_tile_edges",
    "MTB_NO_PACK": "test_fused_sort_on_an_unpacked_index_and_chunked_streams",
    "MTB_OPEN_PACKED": "test_gpu_parity.py::test_database_opens_chunk_by_chunk",
    "MTB_OPEN_CHUNK": "test_gpu_parity.py::test_database_opens_chunk_by_chunk",
    "MTB_PART_EXACT": "test_partitioned_exact_stage_calls",
    "MTB_SEGM_PAD": "test_slot_buffer_lifecycle",
    "MTB_SEGM_CLEAR": "test_slot_buffer_lifecycle",
    "MTB_NO_PLACEMENT_PROBE": "test_slot_buffer_lifecycle",
    "MTB_PLACEMENT_PROBE": "test_slot_buffer_lifecycle",
    "MTB_CHUNKS_PER_STREAM": "test_fused_sort_on_an_unpacked_index_and_chunked_streams",
}
# switches that are deliberately not run for parity
SWITCH_EXEMPT = {
    "MTB_JOIN_VERBOSE": "only prints",
    "MTB_MANY_VERBOSE": "only prints",
    "MTB_LSLOT_VERBOSE": "only prints",
    "MTB_PLACEMENT_VERBOSE": "only prints",
    "MTB_HOST_TIMING": "only times host phases",
    "MTB_LANE_STAGGER_MS": "only delays the start of the stream lanes",
    "MTB_SEGM_CONTIG": "known to lose slots: contiguous VRAM is not coherent across kernels (tests/README.md)",
}


# ------------------------------------------------------------------ the dispatch, mirrored
def metamers_per_read(kmers, n_reads):
    """metamers of every read as the extractor's `total` counts them (kernels_extract.h: both mates of a pair together)"""
    rd = ((kmers["qinfo"] >> np.uint64(32)) & np.uint64(0x1FFFFFFF)).astype(np.int64)
    return np.bincount(rd, minlength=n_reads + 1)[1:]


def slot_geometry(max_q, tail_min=0):
    """mtb_api.hip slot_geometry: (direct, stride)"""
    tail = max(8, tail_min) & ~7 if tail_min > 0 else 16
    direct = max(8, (max_q + 7) & ~7)
    return direct, direct + max(tail, (direct // 8 + 7) & ~7)


def fast_bucket(stride, paired):
    """the k_score_fast instantiation dev_score launches for a slot stride (None: above 384, the fast scorer does not run)"""
    if stride > 384:
        return None
    if paired:
        return "fast<3,3,true>" if stride <= 192 else "fast<4,4,true>" if stride <= 256 else "fast<5,6,true>"
    return "fast<2>" if stride <= 128 else "fast<3>" if stride <= 192 else "fast<4>" if stride <= 256 else "fast<5,6,false>"


def slot_plan(counts, qlen_total, paired, tail_min=0):
    """classify_attempt's choices for a short-read batch from the per-read metamer counts and used lengths: slot path or not, the reads
    routed around the slots, the slot geometry, the fast-scorer bucket and the generic k_score's LDS cap (score_fixed_slots)"""
    n = len(counts)
    off = (counts > SLOT_MAX_Q) | (qlen_total + 3 >= SLOT_MAX_POS)
    n_off = int(off.sum())
    route_off = 0 < n_off < n and n_off * 4 <= n
    max_q = int(counts[~off].max()) if route_off else int(counts.max())
    slot = route_off or (max_q <= SLOT_MAX_Q and int((qlen_total + 3).max()) < SLOT_MAX_POS)
    if not slot:
        return dict(slot=False, route_off=False, max_q=max_q, direct=None, stride=None, bucket="exact", cap=None)
    direct, stride = slot_geometry(max_q, tail_min)
    want = min(direct, int(float(counts.sum()) / float(n) * 1.12) + 1)
    cap = 144 if want <= 144 else 160 if want <= 160 else 224 if want <= 224 else 288 if want <= 288 else 320
    return dict(slot=True, route_off=route_off, max_q=max_q, direct=direct, stride=stride, bucket=fast_bucket(stride, paired) or "generic", cap=cap)


# ------------------------------------------------------------------ worlds
class World:
    """a toy database (one per syncmer mode) and read sets classified by the oracle"""

    def __init__(self, orc, dbdir, syncmer, seed=40):
        from helpers import build_toy_db, default_params
        from metabuli_amd import synth
        self.orc, self.syncmer = orc, syncmer
        self.world = synth.make_world(seed=seed, n_genera=3, species_per_genus=2, strains_per_species=1, genome_len=30000, genus_div=0.3)
        self.dbdir = str(dbdir)
        os.makedirs(self.dbdir, exist_ok=True)
        p = default_params(seq_mode=1, syncmer=syncmer)
        self.values, self.taxids = build_toy_db(orc, self.world, p, self.dbdir)
        self.tax = orc.load_taxonomy(os.path.join(self.dbdir, "taxonomy"))
        self.dbs = {}

    def oparams(self, seq_mode):
        from helpers import default_params
        return default_params(seq_mode=seq_mode, syncmer=self.syncmer)

    def db(self, seq_mode):
        if seq_mode not in self.dbs:
            self.dbs[seq_mode] = self.orc.open_db(self.dbdir, self.tax, self.oparams(seq_mode))
        return self.dbs[seq_mode]

    def sample(self, seq_mode, n, length, seed, **kw):
        from metabuli_amd import synth
        out = synth.sample_reads(np.random.default_rng(seed), self.world, n, length=length, err=0.01, paired=seq_mode == 2, **kw)
        return Reads(*out[:4]) if seq_mode == 2 else Reads(out[0], out[1])

    def count(self, seq_mode, r):
        k, ql, ql2 = self.orc.extract_batch(self.oparams(seq_mode), r.b1, r.o1, r.b2, r.o2)
        return metamers_per_read(k, r.n), ql + ql2

    def tuned(self, seq_mode, lo, hi, seed, mate1_len=60):
        """one read (a pair: mate 1 of mate1_len bases) cut base by base at its end (a pair: mate 2's end) until the oracle counts
        lo..hi metamers for it"""
        for s in range(seed, seed + 20):
            r = self.sample(seq_mode, 1, 300 if seq_mode == 2 else 600, s, frac_random=0.0)
            if seq_mode == 2:
                r = Reads(r.b1[:mate1_len].copy(), np.array([0, mate1_len], np.uint64), r.b2, r.o2)
            full = r.b2 if seq_mode == 2 else r.b1
            for cut in range(len(full), 30, -1):
                c = r.cut_last(cut, mate2=seq_mode == 2)
                if lo <= int(self.count(seq_mode, c)[0][0]) <= hi:
                    return c
        raise AssertionError(f"no read with {lo}..{hi} metamers")

    def classify(self, seq_mode, r):
        return self.orc.classify(self.db(seq_mode), self.tax, self.oparams(seq_mode), r.b1, r.o1, r.b2, r.o2)


class Reads:
    def __init__(self, b1, o1, b2=None, o2=None):
        self.b1, self.o1, self.b2, self.o2 = b1, np.asarray(o1, np.uint64), b2, None if o2 is None else np.asarray(o2, np.uint64)

    @property
    def n(self):
        return len(self.o1) - 1

    def cut_last(self, length, mate2=False):
        """the last read (pair: its mate 2) cut to `length` bases"""
        if mate2:
            o2 = self.o2.copy(); o2[-1] = o2[-2] + np.uint64(length)
            return Reads(self.b1, self.o1, self.b2[:int(o2[-1])], o2)
        o1 = self.o1.copy(); o1[-1] = o1[-2] + np.uint64(length)
        return Reads(self.b1[:int(o1[-1])], o1, self.b2, self.o2)

    def __add__(self, other):
        def cat(b, o, b2, o2):
            return np.concatenate([b, b2]), np.concatenate([o[:-1], o2 + o[-1]])
        b1, o1 = cat(self.b1, self.o1, other.b1, other.o1)
        if self.b2 is None:
            return Reads(b1, o1)
        b2, o2 = cat(self.b2, self.o2, other.b2, other.o2)
        return Reads(b1, o1, b2, o2)

    def rows(self, lo, hi):
        o1 = self.o1[lo:hi + 1] - self.o1[lo]
        b1 = self.b1[int(self.o1[lo]):int(self.o1[hi])]
        if self.b2 is None:
            return Reads(b1, o1)
        return Reads(b1, o1, self.b2[int(self.o2[lo]):int(self.o2[hi])], self.o2[lo:hi + 1] - self.o2[lo])


def check(ref, res, tt, tc, st, tag, lo=0, n_matches=True):
    """bit-exact against the oracle's rows lo .. lo + len(res) (ambiguous rows masked as everywhere in the suite)"""
    ro = ref["results"][lo:lo + len(res)]
    amb = ro["flag"] != 0
    assert ((res["classification"] == ro["classification"]) | amb).all(), tag
    assert ((res["score"].view(np.uint32) == ro["score"].view(np.uint32)) | amb).all(), tag
    assert ((res["n_taxcnt"] == ro["n_taxcnt"]) | amb).all(), tag
    for i in np.flatnonzero(~amb):
        a, b = int(res["taxcnt_off"][i]), int(ro["taxcnt_off"][i])
        n = int(ro["n_taxcnt"][i])
        assert (tt[a:a + n] == ref["tc_tax"][b:b + n]).all() and (tc[a:a + n] == ref["tc_cnt"][b:b + n]).all(), (tag, i)
    if n_matches:
        assert st.n_matches == len(ref["matches"]), (tag, st.n_matches, len(ref["matches"]))


@pytest.fixture(scope="module")
def worlds(orc, tmp_path_factory):
    return {s: World(orc, tmp_path_factory.mktemp(f"tiers_sync{s}"), s) for s in (1, 0)}


@pytest.fixture(scope="module")
def ctx():
    import metabuli_amd as M
    c = M.Context(0)
    c.set_profiling(True)
    yield c
    c.close()


def _mparams(seq_mode, syncmer):
    import metabuli_amd as M
    return M.default_params(seq_mode=seq_mode, syncmer=syncmer)


def _reset(c, names):
    for n in names:
        c.set_option(n, None)


# ------------------------------------------------------------------ (a) stride matrix
# (seq_mode, syncmer, band of the longest read's metamers or None, bulk read length, expected fast bucket, expected generic cap); the bulk
# (48 reads) stays below the band, one read cut to land in it.  Lengths from the oracle's metamer counts of this file's worlds.
STRIDE_CASES = [
    (1, 1, (105, 112), 115, "fast<2>", 144), (1, 1, (113, 120), 120, "fast<3>", 144),
    (1, 1, (161, 168), 170, "fast<3>", 224), (1, 1, (169, 176), 175, "fast<4>", 224),
    (1, 1, (217, 224), 220, "fast<4>", 224), (1, 1, (225, 232), 225, "fast<5,6,false>", 288),
    (1, 1, (329, 336), 325, "fast<5,6,false>", 320), (1, 1, (337, 344), 340, "generic", 320), (1, 1, (377, 384), 380, "generic", 320),
    (1, 1, None, 450, "exact", None), (1, 1, "route", 150, "fast<3>", 144),
    (1, 0, (105, 112), 75, "fast<2>", 144), (1, 0, (113, 120), 75, "fast<3>", 144),
    (1, 0, (161, 168), 100, "fast<3>", 224), (1, 0, (169, 176), 105, "fast<4>", 224),
    (1, 0, (217, 224), 130, "fast<4>", 224), (1, 0, (225, 232), 135, "fast<5,6,false>", 288),
    (1, 0, (329, 336), 185, "fast<5,6,false>", 320), (1, 0, (337, 344), 190, "generic", 320), (1, 0, (377, 384), 210, "generic", 320),
    (1, 0, None, 250, "exact", None),
    (2, 1, (105, 112), 70, "fast<3,3,true>", 144), (2, 1, (113, 120), 70, "fast<3,3,true>", 144),
    (2, 1, (161, 168), 90, "fast<3,3,true>", 160), (2, 1, (169, 176), 100, "fast<4,4,true>", 224),
    (2, 1, (217, 224), 120, "fast<4,4,true>", 224), (2, 1, (225, 232), 130, "fast<5,6,true>", 288),
    (2, 1, (329, 336), 175, "fast<5,6,true>", 320), (2, 1, (337, 344), 180, "generic", 320), (2, 1, (377, 384), 195, "generic", 320),
    (2, 1, None, 250, "exact", None),
    (2, 0, (105, 112), 45, "fast<3,3,true>", 144), (2, 0, (161, 168), 60, "fast<3,3,true>", 224),
    (2, 0, (217, 224), 75, "fast<4,4,true>", 224), (2, 0, (225, 232), 75, "fast<5,6,true>", 288),
    (2, 0, (329, 336), 105, "fast<5,6,true>", 320), (2, 0, (337, 344), 105, "generic", 320),
    (2, 0, None, 150, "exact", None),
]


STRIDE_SWITCH_CASES = [None, "MTB_NO_FAST_SCORER", "MTB_NO_FAST_PAIRS"]      # (MTB_NO_FAST_PAIRS: pairs only)


def _stride_id(case):
    seq_mode, syncmer, band, length, bucket, cap = case
    q = "all>384" if band is None else "one>384" if band == "route" else f"q{band[0]}-{band[1]}"
    return f"{'pe' if seq_mode == 2 else 'se'}-{'sync' if syncmer else 'dense'}-{q}-{bucket}-cap{cap}"


def _stride_reads(w, case):
    seq_mode, syncmer, band, length, bucket, cap = case
    r = w.sample(seq_mode, 48, length, 7)
    if band == "route":                                           # one read beyond MTB_SLOT_MAX_Q among 48 that fit
        r = r + w.sample(seq_mode, 1, 300 if seq_mode == 2 else 560, 8, frac_random=0.0)
    elif band is not None:
        r = r + w.tuned(seq_mode, band[0], band[1], seed=9, mate1_len=length)
    return r


@pytest.mark.parametrize("case", STRIDE_CASES, ids=_stride_id)
def test_stride_matrix(ctx, worlds, case):
    """k_score_fast by slot stride (<2> / <3> / <4> / <5,6,false>, pairs <3,3> / <4,4> / <5,6>), just below and above every edge; 337..384
    metamers (stride > 384: neither the register-resident scorer nor k_score_many runs); beyond 384 (the batch leaves the slot path, or one
    read is routed around it); again with MTB_NO_FAST_SCORER / MTB_NO_FAST_PAIRS, where the generic slot k_score takes every read at the
    LDS cap the batch's mean metamer count selects."""
    seq_mode, syncmer, band, length, bucket, cap = case
    w = worlds[syncmer]
    r = _stride_reads(w, case)
    counts, qlt = w.count(seq_mode, r)
    plan = slot_plan(counts, qlt, seq_mode == 2)
    if band not in (None, "route"):
        assert band[0] <= plan["max_q"] <= band[1] and counts[:-1].max() < band[0], (plan, counts.max())
    assert (plan["bucket"], plan["cap"]) == (bucket, cap), plan
    assert plan["route_off"] == (band == "route"), plan
    ref = w.classify(seq_mode, r)
    assert len(ref["kmers"]) == counts.sum()
    p = _mparams(seq_mode, syncmer)
    ix = ctx.open_index(w.dbdir, p)
    switches = STRIDE_SWITCH_CASES if seq_mode == 2 else STRIDE_SWITCH_CASES[:2]
    try:
        for sw in switches:
            if sw:
                ctx.set_option(sw, "1")
            res, tt, tc = ctx.classify_batch(ix, p, r.b1, r.o1, r.b2, r.o2)
            st = ctx.last_stats()
            tag = (_stride_id(case), sw, plan)
            check(ref, res, tt, tc, st, tag)
            assert st.n_kmers == counts.sum(), tag
            assert st.n_slot_reads == (r.n if plan["slot"] else 0), tag
            fast = sw is None and plan["bucket"].startswith("fast")
            assert st.n_launch[K_SCORE_FAST] == (1 if fast else 0), tag
            if fast:
                assert st.n_generic_reads < r.n, tag
            else:
                assert st.n_generic_reads == r.n, tag
            if plan["slot"] and plan["stride"] > 384:
                assert st.n_launch[K_SCORE_MANY] == 0 and st.n_many_reads == 0, tag
            if plan["route_off"]:
                assert st.n_deferred_reads >= 1, tag                     # (the routed read is scored from an exact segment)
            if sw:
                ctx.set_option(sw, None)
    finally:
        _reset(ctx, switches[1:])
        ix.close()


# ------------------------------------------------------------------ (b) deferred chain
DEFERRED_WORLDS = [(1, 75, "short"), (1, 150, "le192"), (1, 330, "gt192"), (2, 75, "le192"), (2, 165, "gt192")]
DEFERRED_CASES = [("MTB_MANY_CAP", "192"), ("MTB_MANY_CAP", "320"), ("MTB_NO_MANY_SORT", "1"), ("MTB_NO_SCORE_MANY", "1"),
                  ("MTB_TAIL_MIN", "8"), ("MTB_TAIL_MIN", "64"), ("MTB_TAIL_MIN", "96"), ("MTB_SCRATCH_ALIAS", "-1"), ("MTB_SCRATCH_ALIAS", "1")]


@pytest.fixture(scope="module")
def hot_toys(orc, tmp_path_factory):
    from conftest import HotToy
    return {m: HotToy(orc, tmp_path_factory.mktemp(f"tiers_hot{m}"), seq_mode=m, n_reads=200, n_hot=160, keep=0.06) for m in (1, 2)}


@pytest.mark.parametrize("seq_mode,length,geo", DEFERRED_WORLDS, ids=lambda v: str(v))
def test_deferred_chain(ctx, orc, hot_toys, seq_mode, length, geo):
    """Reads of a conserved gene filed sparsely under 160 species overflow their tails and are deferred: k_score_many<K64, 192 | 320>,
    then k_many_sort + k_score_long, then exact segments.  MTB_MANY_CAP picks either staging on either geometry; MTB_NO_MANY_SORT and
    MTB_NO_SCORE_MANY skip tiers; MTB_TAIL_MIN moves the tails (and with 96 the stride beyond 384: the fast and many-species kernels
    stay out); MTB_SCRATCH_ALIAS places the tiers' temporaries.  Every setting gives the oracle's rows."""
    from metabuli_amd import synth
    t = hot_toys[seq_mode]
    out = synth.sample_reads(np.random.default_rng(length), t.world, 160, length=length, err=0.01, frac_random=0.1, paired=seq_mode == 2)
    r = Reads(*out[:4]) if seq_mode == 2 else Reads(out[0], out[1])
    ref = orc.classify(t.db, t.tax, t.p, r.b1, r.o1, r.b2, r.o2)
    counts = metamers_per_read(ref["kmers"], r.n)
    qlt = ref["qlen"] + ref["qlen2"]
    plan = slot_plan(counts, qlt, seq_mode == 2)
    assert plan["slot"] and not plan["route_off"]
    assert {"short": plan["direct"] <= 64, "le192": 64 < plan["direct"] and plan["stride"] <= 192,
            "gt192": plan["stride"] > 192 and plan["direct"] > 288}[geo], plan
    p = _mparams(seq_mode, 1)
    ix = ctx.open_index(t.dbdir, p)
    try:
        res, tt, tc = ctx.classify_batch(ix, p, r.b1, r.o1, r.b2, r.o2)
        st0 = ctx.last_stats()
        check(ref, res, tt, tc, st0, ("default", plan))
        assert st0.n_deferred_reads > 5 and st0.n_many_reads > 0 and st0.n_launch[K_SCORE_MANY] == 1, (st0.n_deferred_reads, st0.n_many_reads)
        seen = {}
        for name, val in DEFERRED_CASES:
            ctx.set_option(name, val)
            res, tt, tc = ctx.classify_batch(ix, p, r.b1, r.o1, r.b2, r.o2)
            st = seen[(name, val)] = ctx.last_stats()
            ctx.set_option(name, None)
            tm = int(val) if name == "MTB_TAIL_MIN" else 0
            pl = slot_plan(counts, qlt, seq_mode == 2, tail_min=tm)
            tag = (geo, name, val, pl, st.n_deferred_reads, st.n_many_reads)
            check(ref, res, tt, tc, st, tag)
            fast_ran = st.n_launch[K_SCORE_FAST] == 1
            assert fast_ran == (pl["stride"] <= 384), tag
            if name == "MTB_MANY_CAP":
                assert st.n_many_reads > 0 and st.n_deferred_reads == st0.n_deferred_reads, tag
            elif name == "MTB_NO_MANY_SORT":
                assert st.n_deferred_reads == st0.n_deferred_reads and st.n_many_reads <= st0.n_many_reads, tag
            elif name == "MTB_NO_SCORE_MANY":
                assert st.n_many_reads == 0 and st.n_launch[K_SCORE_MANY] == 0 and st.n_deferred_reads == st0.n_deferred_reads, tag
            elif name == "MTB_TAIL_MIN":
                if pl["stride"] > 384:                                      # nothing but the generic scorer and exact segments
                    assert st.n_launch[K_SCORE_MANY] == 0 and st.n_many_reads == 0 and st.n_generic_reads == r.n, tag
                elif pl["stride"] < plan["stride"]:
                    assert st.n_deferred_reads > st0.n_deferred_reads, tag     # shorter tails: more overflow
                elif pl["stride"] == plan["stride"]:
                    assert (st.n_deferred_reads, st.n_many_reads) == (st0.n_deferred_reads, st0.n_many_reads), tag
                else:
                    assert st.n_deferred_reads <= st0.n_deferred_reads, tag
            else:
                assert (st.n_deferred_reads, st.n_many_reads) == (st0.n_deferred_reads, st0.n_many_reads), tag
                assert (ctx.last_scratch_bytes > 0) == (val == "1"), tag
        # the default staging is the one MTB_MANY_CAP pins for this stride (192 records up to 192 slots per read, else 320); more staging never takes fewer reads
        pinned = seen[("MTB_MANY_CAP", "192" if plan["stride"] <= 192 else "320")]
        assert (st0.n_many_reads, st0.n_many_kept) == (pinned.n_many_reads, pinned.n_many_kept), (geo, plan)
        assert seen[("MTB_MANY_CAP", "320")].n_many_reads >= seen[("MTB_MANY_CAP", "192")].n_many_reads, geo
    finally:
        _reset(ctx, {n for n, _ in DEFERRED_CASES})
        ix.close()


# ------------------------------------------------------------------ (c) slot buffer lifecycle
LIFECYCLE_CASES = [(None, None), ("MTB_SEGM_CLEAR", "kernel"), ("MTB_SEGM_CLEAR", "always"), ("MTB_SEGM_CLEAR", "sync"), ("MTB_SEGM_PAD", "1"),
                   ("MTB_NO_PLACEMENT_PROBE", "1"), ("MTB_PLACEMENT_PROBE", "1")]


@pytest.mark.parametrize("name,val", LIFECYCLE_CASES, ids=lambda v: str(v))
def test_slot_buffer_lifecycle(worlds, name, val):
    """34 batches of varying size on one context -- past the 5-bit epoch's wrap -- under every clearing / placement switch of the slot
    buffer: every batch gives the oracle's rows (a stale slot read as live would add foreign matches).
    No statistic tells which clearing / placement branch ran (mtb_batch_stats has none for them), so these cases show result
    neutrality only.  The placement-probe switches act on slot buffers of 8 GB and more (ensure_placed); on toy batches both take the
    plain allocation, and these cases only show that setting them changes nothing."""
    import metabuli_amd as M
    w = worlds[1]
    r = w.sample(1, 160, 150, 21)
    ref = w.classify(1, r)
    c = M.Context(0)
    if name:
        c.set_option(name, val)
    p = _mparams(1, 1)
    ix = c.open_index(w.dbdir, p)
    sizes = [160, 37, 160, 1, 99, 128, 64, 150]
    rd = ((ref["matches"]["qinfo"] >> np.uint64(32)) & np.uint64(0x1FFFFFFF)).astype(np.int64)
    try:
        for it in range(34):
            n = sizes[it % len(sizes)]
            lo = (it * 13) % (160 - n + 1)
            rr = r.rows(lo, lo + n)
            res, tt, tc = c.classify_batch(ix, p, rr.b1, rr.o1)
            st = c.last_stats()
            check(ref, res, tt, tc, st, (name, val, it, lo, n), lo=lo, n_matches=False)
            assert st.n_slot_reads == n and st.n_matches == int(((rd > lo) & (rd <= lo + n)).sum()), (name, val, it)
    finally:
        ix.close(); c.close()


# ------------------------------------------------------------------ (d) long reads
LONG_CASES = [(("MTB_NO_LONG_SCORER", "1"), ("MTB_JOIN_WIN", w)) for w in ("1", "0")] + \
             [(("MTB_NO_LONG_SLOTS", "1"), ("MTB_JOIN_WIN", w)) for w in ("1", "0")] + \
             [(("MTB_NO_LONG_SLOTS", "1"), ("MTB_NO_LONG_SCORER", "1"), ("MTB_JOIN_WIN", w)) for w in ("1", "0")]


@pytest.mark.parametrize("mode", ["sync_long", "sync_xlong"])
def test_long_read_scorer_switches(orc, tmp_path, mode, monkeypatch):
    """Long reads without the per-read slot ranges (MTB_NO_LONG_SLOTS: regroup + segment sort, then k_score_long) and, on that path,
    without the workgroup-per-read scorer (MTB_NO_LONG_SCORER: the generic launch takes every read), each with the window join forced
    on and off on a depth-7 packed index.  The slot-range path always scores with k_score_long: MTB_NO_LONG_SCORER alone changes nothing
    there, and the statistics say so.  The window form exists for the slot ranges only (dev_join): forced on there, the statistics
    report it and its tiles; the exact-segment path (MTB_NO_LONG_SLOTS) joins by bisection whatever MTB_JOIN_WIN says."""
    import metabuli_amd as M
    from conftest import Toy, TOY_MODES
    t = Toy(orc, tmp_path / mode, **TOY_MODES[mode])
    monkeypatch.setenv("MTB_DIR_DEPTH", "7")
    c = M.Context(0)
    monkeypatch.delenv("MTB_DIR_DEPTH")
    c.set_profiling(True)
    p = _mparams(3, 1)
    ix = c.open_index(t.dbdir, p)
    names = {k for case in LONG_CASES for k, _ in case}
    try:
        res, tt, tc = c.classify_batch(ix, p, t.b1, t.o1)
        st0 = c.last_stats()
        check(t.ref, res, tt, tc, st0, (mode, "default"))
        assert st0.n_slot_reads == t.n_reads and st0.n_generic_reads < t.n_reads
        for case in LONG_CASES:
            _reset(c, names)
            for k, v in case:
                c.set_option(k, v)
            res, tt, tc = c.classify_batch(ix, p, t.b1, t.o1)
            st = c.last_stats()
            sws = dict(case)
            tag = (mode, case)
            check(t.ref, res, tt, tc, st, tag)
            variant = M.JOIN_VARIANTS[st.join_variant]
            if "MTB_NO_LONG_SLOTS" not in sws and sws["MTB_JOIN_WIN"] == "1":
                assert variant == "window" and st.join_tiles > 0 and st.join_tiles_windowed > 0 and st.join_tiles_outside == 0, (tag, variant)
            else:
                assert variant == "other" and st.join_tiles == 0, (tag, variant)
            if "MTB_NO_LONG_SLOTS" not in sws:
                assert st.n_slot_reads == t.n_reads and st.n_generic_reads == st0.n_generic_reads, tag
            elif "MTB_NO_LONG_SCORER" in sws:
                assert st.n_slot_reads == 0 and st.n_generic_reads == t.n_reads, tag
            else:
                assert st.n_slot_reads == 0 and st.n_generic_reads < t.n_reads, tag
    finally:
        _reset(c, names)
        ix.close(); c.close()


# ------------------------------------------------------------------ (e) fused sort
PACKED_INDEX_CASES = [("MTB_DIR_DEPTH", "7")]                    # index-open switches: through the environment around the context
SORT_JOIN_CASES = [(("MTB_JOIN_WIN", "1"), ("MTB_JOIN_WIN_QT", "5")), (("MTB_JOIN_WIN", "1"), ("MTB_JOIN_WIN_QT", "64"))]
SORT_VARIANTS = [(), (("MTB_SORT_LSD", "1"),), (("MTB_SORT_NO_XCD", "1"),), (("MTB_SORT_PAIRS", "1"),), (("MTB_SORT_PAIRS", "2"),), (("MTB_SORT_PAIRS", "3"),)]
# (name, bulk reads of 150 bases, band of the batch's metamer total the last read is cut to, or None)
SORT_SIZES = [("below-one-tile", 20, None), ("one-tile-minus", 20, (SORT_TILE - 8, SORT_TILE)), ("one-tile-plus", 20, (SORT_TILE + 1, SORT_TILE + 8)),
              ("eight-tiles", 160, None), ("nine-tiles", 180, None), ("bucket-over-tiles", 60, None)]
EXTRACT_BUF = 320                                        # kernels_extract.h MTB_EXTRACT_BUF


def sort_records(counts):
    """length of the list the fused sort orders (and the join reads) for a batch of at most 65536 short reads of at most MTB_EXTRACT_BUF
    metamers each: a wave per read, and a read with metamers flushes once into a chunk of need + 65 records (kernels_extract.h: one
    read still expected at produced / reads_done + 1 = 1 metamer, x 5/4, + 64); the unused tail is blank records.  st.n_kmers counts the
    real metamers only."""
    assert len(counts) <= 65536 and counts.max() <= EXTRACT_BUF
    return int(counts.sum() + 65 * (counts > 0).sum())


def _sort_batch(w, name, n_bulk, band):
    r = w.sample(1, n_bulk, 150, 31)
    if name == "bucket-over-tiles":
        # low-complexity reads (one codon repeated): all their metamers share a few amino-acid letter pairs, buckets of pass A wider
        # than one scatter tile -- the bucket-local passes then run several tiles per bucket
        rep = np.frombuffer(b"GCTGCAGCC" * 40, np.uint8)[:300]
        lc = Reads(np.tile(rep, 40), np.arange(41, dtype=np.uint64) * 300)
        return r + lc
    if band is None:
        return r
    total = sort_records(w.count(1, r)[0])
    r = r + w.sample(1, 1, 300, 32, frac_random=0.0)              # one longer read, cut until the list lands in the band
    full = int(r.o1[-1] - r.o1[-2])
    for cut in range(full, 30, -1):
        c = r.cut_last(cut)
        if band[0] <= total + sort_records(w.count(1, c.rows(c.n - 1, c.n))[0]) <= band[1]:
            return c
    raise AssertionError(band)


@pytest.fixture(scope="module")
def packed7(worlds):
    import metabuli_amd as M
    os.environ.update(PACKED_INDEX_CASES)
    try:
        c = M.Context(0)
    finally:
        for k, _ in PACKED_INDEX_CASES:
            del os.environ[k]
    c.set_profiling(True)
    ix = c.open_index(worlds[1].dbdir, _mparams(1, 1))
    yield c, ix
    ix.close(); c.close()


@pytest.mark.parametrize("name,n_bulk,band", SORT_SIZES, ids=lambda v: str(v))
def test_fused_sort_variants_at_tile_edges(worlds, packed7, name, n_bulk, band):
    """The fused path's amino-acid sort (MSD pass on the top letter pair, bucket-local passes from the plan, 2-byte digit side arrays,
    XCD tile mapping) and its variants -- three LSD passes, no XCD mapping, fewer letter pairs -- at batch sizes around the 4096-record
    scatter tile, at 8 and 9 tiles (the XCD mapping rounds the grid to a multiple of 8) and with buckets wider than a tile; window
    join pinned with tiles of 5 and 64 queries.  The directory join looks every query up on its own, so a misordered list still
    matches: on a list sorted on the announced bits no tile may find a query outside its window (join_tiles_outside == 0).
    The sorted list holds the extractor's blank records too (sort_records); its length is read back from a window join with tiles of
    one query, and the tile edges are placed on it."""
    import metabuli_amd as M
    w = worlds[1]
    c, ix = packed7
    r = _sort_batch(w, name, n_bulk, band)
    ref = w.classify(1, r)
    nk = len(ref["kmers"])
    counts = metamers_per_read(ref["kmers"], r.n)
    p = _mparams(1, 1)
    names = {k for v in SORT_JOIN_CASES + SORT_VARIANTS for k, _ in v}
    _reset(c, names)
    c.set_option("MTB_JOIN_WIN", "1"); c.set_option("MTB_JOIN_WIN_QT", "1")
    res, tt, tc = c.classify_batch(ix, p, r.b1, r.o1)
    st = c.last_stats()
    check(ref, res, tt, tc, st, (name, "qt1"))
    n_sorted = st.join_tiles                                   # tiles of one query: the length of the sorted list
    if name != "bucket-over-tiles":
        assert n_sorted == sort_records(counts), (n_sorted, sort_records(counts), nk)
    if band:
        assert band[0] <= n_sorted <= band[1], n_sorted
    tiles = -(-n_sorted // SORT_TILE)
    assert {"below-one-tile": tiles == 1 and n_sorted < SORT_TILE - 64, "one-tile-minus": tiles == 1, "one-tile-plus": tiles == 2,
            "eight-tiles": tiles == 8, "nine-tiles": tiles == 9, "bucket-over-tiles": tiles > 1}[name], (name, n_sorted, tiles)
    if name == "bucket-over-tiles":
        top = (ref["kmers"]["value"] >> np.uint64(54)).astype(np.int64)
        assert np.bincount(top).max() > SORT_TILE, np.bincount(top).max()
    try:
        for pin in SORT_JOIN_CASES:
            qt = dict(pin)["MTB_JOIN_WIN_QT"]
            for var in SORT_VARIANTS:
                _reset(c, names)
                for k, v in pin + var:
                    c.set_option(k, v)
                res, tt, tc = c.classify_batch(ix, p, r.b1, r.o1)
                st = c.last_stats()
                tag = (name, nk, qt, var)
                assert ix.state()["packed"] and ix.state()["dir_depth"] == int(dict(PACKED_INDEX_CASES)["MTB_DIR_DEPTH"]), (tag, ix.state())
                check(ref, res, tt, tc, st, tag)
                assert st.n_kmers == nk and M.JOIN_VARIANTS[st.join_variant] == "window", tag
                assert st.join_tiles == -(-n_sorted // int(qt)), (tag, st.join_tiles, n_sorted)          # the tiles dev_join launches
                assert st.join_tiles_outside == 0, tag
                pairs = dict(var).get("MTB_SORT_PAIRS")
                if pairs in ("1", "2"):              # sorted on fewer letters than the windows need: windows zeroed, every tile reads global memory
                    assert st.join_tiles_windowed == 0, tag
                elif qt == "5":
                    assert st.join_tiles_windowed > 0, tag
    finally:
        _reset(c, names)


UNPACKED_INDEX_CASES = [("MTB_DIR_DEPTH", "7"), ("MTB_NO_PACK", "1")]
STREAM_CASES = [("MTB_CHUNKS_PER_STREAM", None), ("MTB_CHUNKS_PER_STREAM", "2")]


def _tiled(r, ref, big):
    """the read set `big` times over, and the oracle's answer for it (rows are independent of the batch)"""
    o1 = np.concatenate([[0], np.cumsum(np.tile(np.diff(r.o1.astype(np.int64)), big))]).astype(np.uint64)
    rr = Reads(np.tile(r.b1, big), o1)
    ro = np.tile(ref["results"], big)
    ro["taxcnt_off"] += np.repeat(np.arange(big, dtype=np.uint32) * np.uint32(len(ref["tc_tax"])), r.n)
    return rr, dict(results=ro, tc_tax=np.tile(ref["tc_tax"], big), tc_cnt=np.tile(ref["tc_cnt"], big), matches=np.tile(ref["matches"], big))


def test_fused_sort_on_an_unpacked_index_and_chunked_streams(worlds, monkeypatch):
    """MTB_NO_PACK (a depth-7 directory over the flat array) on the nine-tile batch; MTB_CHUNKS_PER_STREAM=2 on two stream lanes with
    that batch tiled past 4096 reads per lane (mtb_classify_batch_device splits no smaller batch): the oracle's rows, the rows of the
    single-stream run, and one extraction launch per read range -- two ranges without the switch, four with it."""
    import metabuli_amd as M
    w = worlds[1]
    r = _sort_batch(w, "nine-tiles", 180, None)
    ref = w.classify(1, r)
    p = _mparams(1, 1)
    for k, v in UNPACKED_INDEX_CASES:
        monkeypatch.setenv(k, v)
    c = M.Context(0)
    for k, _ in UNPACKED_INDEX_CASES:
        monkeypatch.delenv(k)
    ix = c.open_index(w.dbdir, p)
    try:
        assert not ix.state()["packed"] and ix.state()["dir_depth"] == 7
        res, tt, tc = c.classify_batch(ix, p, r.b1, r.o1)
        check(ref, res, tt, tc, c.last_stats(), "no-pack")
        n_lanes = 2
        rt, reft = _tiled(r, ref, -(-4096 * n_lanes // r.n))
        c.set_profiling(True)
        r1, t1, c1 = c.classify_batch(ix, p, rt.b1, rt.o1)
        assert c.last_stats().n_launch[K_EXTRACT_EMIT] == 1
        c.set_streams(n_lanes)                                  # (lanes take the profiling state of their parent when they are made)
        for k, v in STREAM_CASES:
            c.set_option(k, v)
            res, tt, tc = c.classify_batch(ix, p, rt.b1, rt.o1)
            st = c.last_stats()
            tag = ("streams", k, v)
            check(reft, res, tt, tc, st, tag)
            assert (res == r1).all() and (tt == t1).all() and (tc == c1).all(), tag
            assert st.n_reads == rt.n and st.n_slot_reads == rt.n, tag
            assert st.n_launch[K_EXTRACT_EMIT] == n_lanes * int(v or 1), (tag, st.n_launch[K_EXTRACT_EMIT])     # one classify_one per read range
    finally:
        ix.close(); c.close()


# ------------------------------------------------------------------ (f) partitioned stage calls
PART_CASES = [("MTB_PART_EXACT", "1")]


@pytest.mark.parametrize("seq_mode", [1, 2])
def test_partitioned_exact_stage_calls(orc, tmp_path, seq_mode, monkeypatch):
    """MTB_PART_EXACT: the partitioned stage calls on exact-order runs (five binary passes, the bisection join at the owners,
    regroup + segment sort at home) instead of the ordinal-tagged slot path; two ranks on one device"""
    import torch.multiprocessing as mp
    from conftest import Toy
    from test_partitioned import _gpu_worker
    t = Toy(orc, tmp_path / "db", syncmer=1, paired=seq_mode == 2, seed=27, n_reads=200)
    npz = str(tmp_path / "in.npz"); out = str(tmp_path / "out.npz")
    if seq_mode == 2:
        np.savez(npz, bases=t.b1, offs=t.o1, bases2=t.b2, offs2=t.o2)
    else:
        np.savez(npz, bases=t.b1, offs=t.o1)
    for k, v in PART_CASES:
        monkeypatch.setenv(k, v)                 # (read when the workers create their contexts)
    mp.spawn(_gpu_worker, args=(2, 31300 + os.getpid() % 500 + 10 * seq_mode, t.dbdir, npz, out, seq_mode), nprocs=2, join=True)
    got = np.load(out); ro = t.ref["results"]; amb = ro["flag"] != 0
    assert ((got["cls"] == ro["classification"]) | amb).all()
    assert ((got["score"].view(np.uint32) == ro["score"].view(np.uint32)) | amb).all()
    if not amb.any():
        assert (got["tt"] == t.ref["tc_tax"]).all() and (got["tc"] == t.ref["tc_cnt"]).all()
    assert int(got["T"]) == len(t.values)
    assert not bool(got["slot_ok"])              # the exact-order runs really were taken: no read went through the slot segments
