"""The join at the ends of the target array.  A full toy index puts almost no query metamer past its last target's directory bucket, and
none there in a tile that is staged in LDS; these tests build indices whose ends ARE where the queries land and compare the HIP join with
the oracle and with tests/bruteforce.py's plain formulation of it:
  head cuts    the first 15 / 50 / 85 % of a toy index's targets: queries land past the last target (lo = hi = limit < the bucket's start);
  tail cut     the last 50 %: queries land before the first target;
  tiny         T = 1, 2, 3, 5 targets from buckets the reads hit (T = 1: limit = 0, nothing is a candidate);
  run at end   the index ends in a run of more than four targets with one amino-acid part, a block of equal values inside it: the rule
               "the last entry is never a candidate" cuts through a run that the window form's four-word read-ahead crosses.
Every case checks its own precondition first, so that it cannot quietly stop testing its edge.

  fused path   classify_batch with every join form pinned (sector-random q<Q>w<W>, the LDS window at several tile sizes and wave counts,
               auto, a flat index, no directory): match total, per-read answers and the taxID:count list of every read that is not ambiguous;
  stage API    ctx.match on hand-built query lists around the ends, byte for byte against join_spec and the oracle;
  views        Index.slice(lo, hi, is_last): the view's final entry is a candidate exactly when is_last is False."""
import os

import numpy as np
import pytest

import bruteforce as bf
from helpers import match_dt

pytestmark = pytest.mark.gpu

MODES = {
    "sync_se": dict(syncmer=1, paired=False, seed=31, n_reads=200),
    # (dense pairs of 100 bp: few enough metamers per read for the slot segments -- at 150 bp every read exceeds them and the batch takes
    # the exact-segment path, which joins by bisection without the directory)
    "dense_pe": dict(syncmer=0, paired=True, seed=4, length=100),
    "old_format_pe": dict(syncmer=0, paired=True, seed=6, kmer_format=1, length=100),
    "sync_long": dict(syncmer=1, paired=False, seed=5, n_reads=40, length=3000, seq_mode=3, err=0.05, lognormal=True),
}
CASES = ["head15", "head50", "head85", "tail50", "tiny1", "tiny2", "tiny3", "tiny5", "runend"]
_JOIN_OPTS = ("MTB_JOIN_VARIANT", "MTB_JOIN_WIN", "MTB_JOIN_WIN_QT")
# form -> (index kind, options, join variant the statistics must report on short reads)
FORMS = {
    "q1w6": ("depth7", dict(MTB_JOIN_VARIANT="q1w6"), "q1w6"),
    "q2w5": ("depth7", dict(MTB_JOIN_VARIANT="q2w5"), "q2w5"),
    "q1w5": ("depth7", dict(MTB_JOIN_VARIANT="q1w5"), "q1w5"),
    "q2w6": ("depth7", dict(MTB_JOIN_VARIANT="q2w6"), "q2w6"),
    "window_qt5": ("depth7", dict(MTB_JOIN_WIN="1", MTB_JOIN_WIN_QT="5"), "window"),
    "window_qt17": ("depth7", dict(MTB_JOIN_WIN="1", MTB_JOIN_WIN_QT="17"), "window"),
    "window_qt64": ("depth7", dict(MTB_JOIN_WIN="1", MTB_JOIN_WIN_QT="64"), "window"),
    "window_qt256": ("depth7", dict(MTB_JOIN_WIN="1", MTB_JOIN_WIN_QT="256"), "window"),
    "windoww5": ("depth7", dict(MTB_JOIN_VARIANT="windoww5"), "windoww5"),
    "windoww6": ("depth7", dict(MTB_JOIN_VARIANT="windoww6"), "windoww6"),
    "windoww7": ("depth7", dict(MTB_JOIN_VARIANT="windoww7"), "windoww7"),
    "auto": ("depth7", {}, None),
    "flat": ("flat", {}, "other"),
    "nodir": ("nodir", {}, "other"),
}
AA = np.uint64(24)


def _aa(v):
    return np.asarray(v, dtype=np.uint64) >> AA


def _seq(q):
    return (q["qinfo"] >> np.uint64(32)) & np.uint64(0x1FFFFFFF)


class Edge:
    """one edge index of a toy world: its database files, the oracle's answer for the world's reads, indices opened on demand"""

    def __init__(self, orc, t, case, d):
        vals, tids = self._cut(orc, t, case)
        self.case, self.t, self.dir = case, t, d
        self.values, self.taxids = vals, tids
        os.makedirs(d)
        t.world.tax.write(os.path.join(d, "taxonomy"))
        orc.write_db(d, vals, tids, t.p)
        self.tax = orc.load_taxonomy(os.path.join(d, "taxonomy"))
        self.db = orc.open_db(d, self.tax, t.p)
        self.ref = orc.classify(self.db, self.tax, t.p, t.b1, t.o1, t.b2, t.o2)
        self._check_precondition()
        self.ix = {}

    @staticmethod
    def _cut(orc, t, case):
        v, tx = t.values, t.taxids
        T = len(v)
        qa = np.unique(_aa(t.ref["kmers"]["value"]))
        if case.startswith("head"):
            n = T * int(case[4:]) // 100
            return v[:n], tx[:n]
        if case == "tail50":
            return v[T // 2:], tx[T // 2:]
        hit = np.flatnonzero(np.isin(_aa(v), qa))             # targets whose amino-acid part some query carries
        if case.startswith("tiny"):
            # the first n targets in buckets the reads hit (low buckets: a depth-7 directory is filled up to the first target by one thread)
            pos = hit[:int(case[4:])]
            return v[pos], tx[pos]
        assert case == "runend"
        # the amino-acid part of a target that many queries carry, in the middle of the index: the index ends with its run, lengthened by
        # a block of copies of one query's value (other species) and by variants of that value with DNA parts that differ in one or two codons
        qv = t.ref["kmers"]["value"]
        qcount = {int(a): int(c) for a, c in zip(*np.unique(_aa(qv), return_counts=True))}
        mid_hits = hit[len(hit) // 4: 3 * len(hit) // 4]
        a = max((int(x) for x in _aa(v[mid_hits])), key=lambda x: qcount.get(x, 0))
        q0 = int(qv[_aa(qv) == np.uint64(a)][0])
        keep = _aa(v) <= np.uint64(a)
        species = sorted({t.world.tax.species_of(int(x)) for x in tx})
        ev, et = [q0, q0, q0], list(species[:3])
        rng = np.random.default_rng(5)
        for i in range(4):
            dna = q0 & 0xFFFFFF
            for _ in range(1 + i % 2):
                pos = 3 * int(rng.integers(0, 8))
                dna = (dna & ~(7 << pos)) | (int(rng.integers(0, 8)) << pos)
            ev.append((q0 & ~0xFFFFFF) | dna); et.append(species[(3 + i) % len(species)])
        ev.append(((q0 & ~0xFFFFFF) | 0xFFFFFF)); et.append(species[-1])           # the last entry: the run's greatest DNA part
        vals = np.concatenate([v[keep], np.array(ev, np.uint64)]); tids = np.concatenate([tx[keep], np.array(et, np.int32)])
        sp = np.array([t.world.tax.species_of(int(x)) for x in tids], dtype=np.int32)
        order = np.lexsort((tids, sp, vals))                  # (value, species, taxid): the order of build_toy_db
        vals, tids, sp = vals[order], tids[order], sp[order]
        keep = np.ones(len(vals), bool)
        keep[1:] = (vals[1:] != vals[:-1]) | (sp[1:] != sp[:-1])
        return vals[keep], tids[keep]

    def _check_precondition(self):
        t, v = self.t, self.values
        qa = _aa(t.ref["kmers"]["value"])
        T = len(v)
        if self.case.startswith("head"):
            assert T < len(t.values) and (qa > _aa(v[-1])).sum() > 0          # queries land past the last target
        elif self.case == "tail50":
            assert (qa < _aa(v[0])).sum() > 0                                # queries land before the first target
        elif self.case.startswith("tiny"):
            assert T == int(self.case[4:]) and np.isin(_aa(v), qa).all()     # every target in a bucket some query hits
            if T == 1:
                assert len(self.ref["matches"]) == 0                         # limit = 0: nothing is a candidate
            else:
                assert len(self.ref["matches"]) > 0
        else:
            last = _aa(v[-1])
            run = int((_aa(v) == last).sum())
            tail = v[-run:]
            assert run > 4 and (_aa(v[-run:]) == last).all() and (qa == last).any()
            assert (tail[1:] == tail[:-1]).any() and tail[-1] != tail[-2]     # a block of equal values inside, the excluded last entry not in it
            assert len(self.ref["matches"]) > 0

    def index(self, ctx, kind, mp):
        if kind not in self.ix:
            ctx.set_option("MTB_DIR_DEPTH", "7" if kind == "depth7" else None)
            ctx.set_option("MTB_NO_DIR", "1" if kind == "nodir" else None)
            try:
                self.ix[kind] = ctx.open_index(self.dir, mp)
            finally:
                ctx.set_option("MTB_DIR_DEPTH", None); ctx.set_option("MTB_NO_DIR", None)
        return self.ix[kind]

    def close(self):
        for ix in self.ix.values():
            ix.close()
        self.ix = {}


@pytest.fixture(scope="module")
def ctx():
    import metabuli_amd as M
    c = M.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def worlds(orc, tmp_path_factory):
    from conftest import Toy
    cache = {}

    def get(mode):
        if mode not in cache:
            cache[mode] = Toy(orc, tmp_path_factory.mktemp("w_" + mode), **MODES[mode])
        return cache[mode]
    return get


@pytest.fixture(scope="module")
def edges(orc, worlds, ctx, tmp_path_factory):
    cache = {}

    def get(mode, case):
        if (mode, case) not in cache:
            cache[(mode, case)] = Edge(orc, worlds(mode), case, str(tmp_path_factory.mktemp("e") / f"{mode}_{case}"))
        for k, e in cache.items():              # the indices of one edge at a time (a depth-7 directory of a toy index takes gigabytes)
            if k != (mode, case):
                e.close()
        return cache[(mode, case)]
    yield get
    for e in cache.values():
        e.close()


def _mparams(t):
    import metabuli_amd as M
    p = t.p
    return M.default_params(seq_mode=p.seq_mode, syncmer=p.syncmer, smer_len=p.smer_len, kmer_format=p.kmer_format, accession_level=p.accession_level)


def _lists_differ(res, tt, tc, ref):
    """reads (not ambiguous in the oracle's answer) whose taxID:count list differs from the oracle's"""
    ro = ref["results"]
    bad = []
    for i in np.flatnonzero(ro["flag"] == 0):
        n = int(ro["n_taxcnt"][i])
        a, b = int(res["taxcnt_off"][i]), int(ro["taxcnt_off"][i])
        if int(res["n_taxcnt"][i]) != n or not (np.array_equal(tt[a:a + n], ref["tc_tax"][b:b + n]) and np.array_equal(tc[a:a + n], ref["tc_cnt"][b:b + n])):
            bad.append(int(i))
    return bad


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("mode", list(MODES))
def test_fused_join_at_the_ends_of_the_index(ctx, edges, mode, case, form):
    import metabuli_amd as M
    e = edges(mode, case)
    t = e.t
    kind, opts, variant = FORMS[form]
    mp = _mparams(t)
    ix = e.index(ctx, kind, mp)
    for k in _JOIN_OPTS:
        ctx.set_option(k, opts.get(k))
    try:
        res, tt, tc = ctx.classify_batch(ix, mp, t.b1, t.o1, t.b2, t.o2)
        st = ctx.last_stats()
    finally:
        for k in _JOIN_OPTS:
            ctx.set_option(k, None)
    ran = M.JOIN_VARIANTS.get(st.join_variant, st.join_variant)
    state = ix.state()
    tag = (mode, case, form, ran, state)
    # the index is in the state the form needs (T = 1: no directory at all -- the bisection join over limit = 0)
    if kind == "nodir" or len(e.values) < 2:
        assert state["dir_depth"] == 0, tag
    elif kind == "flat":
        assert state["dir_depth"] > 0 and not state["packed"], tag
    else:
        assert state["dir_depth"] == 7 and state["packed"], tag
    # the pinned join really ran (long reads: only the window form is reported; the other pins take the one-query-per-thread form)
    if len(e.values) < 2 or kind != "depth7":
        assert ran == "other", tag
    elif t.p.seq_mode == 3:
        assert (ran == "window") == (opts.get("MTB_JOIN_WIN") == "1") or variant is None, tag
    elif variant is not None:
        assert ran == variant and st.join_tuned == 0, tag
    assert st.join_tiles_outside == 0, tag
    ro = e.ref["results"]
    amb = ro["flag"] != 0
    assert st.n_matches == len(e.ref["matches"]), tag
    assert ((res["classification"] == ro["classification"]) | amb).all(), tag
    assert ((res["is_classified"] == ro["is_classified"]) | amb).all(), tag
    assert ((res["score"].view(np.uint32) == ro["score"].view(np.uint32)) | amb).all(), tag
    assert ((res["n_taxcnt"] == ro["n_taxcnt"]) | amb).all(), tag
    assert (res["qlen"] == ro["qlen"]).all() and (res["qlen2"] == ro["qlen2"]).all(), tag
    assert _lists_differ(res, tt, tc, e.ref) == [], tag
    assert (~amb).sum() > 0


# ---- stage API: hand-built query lists ----

def _forged_queries(values, kmer_format):
    """sorted queries around the ends of `values`: bucket 0, before / equal to the first target, equal to the second-to-last and the
    last, inside the last target's bucket and beyond it, all letters 20, letters >= 21, and blank slots (sequenceID 0)"""
    import metabuli_amd as M
    v = [int(x) for x in values]
    first, last = v[0], v[-1]
    q = [0x000000000012345, first, first ^ 0x1, last, last ^ 0x9, (last | 0xFFFFFF), (last & ~0xFFFFFF) + (1 << 24) + 0x42]
    if len(v) >= 2:
        q += [v[-2], v[-2] ^ 0x40]
    if first >> 24:
        q += [first - (1 << 24), (first & ~0xFFFFFF) - 1]
    if kmer_format == 2:
        # (letters of 5 bits, the first in the top bits): the last target's bucket holds the values that share its first seven letters
        q += [(last & ~((0x1F << 24) | 0xFFFFFF)) | (20 << 24) | 0x111, (last & ~((0x1F << 24) | 0xFFFFFF)) + (1 << 29)]
        all20 = 0
        for _ in range(8):
            all20 = (all20 << 5) | 20
        q += [(all20 << 24) | 0x0ABCDE, (21 << 59) | 0x123, (31 << 59) | (31 << 54) | 0xFFFFFF, (all20 << 24) | (21 << 24) | 0x5]
    else:
        top = 21 ** 8
        q += [((top - 1) << 24) | 0x0ABCDE, (top << 24) | 0x77, ((top + 5) << 24) | 0x1]
    q = [x & 0xFFFFFFFFFFFFFFFF for x in q if x >= 0]
    out = np.zeros(3 * len(q), M.kmer_dt)
    for i, x in enumerate(q):
        for j in range(3):
            seq = 0 if j == 2 else 1 + (i % 5)                 # every third slot is blank
            frame = (i + j) % 6
            out[3 * i + j] = (x, (frame << 61) | (seq << 32) | (7 * i + j))
    return np.sort(out, order=["value", "qinfo"])


def _as_records(ms):
    out = np.zeros(len(ms), match_dt)
    for i, (qi, tid, sp, dna, reh, ham) in enumerate(ms):
        out[i] = (qi, tid, sp, dna, reh, ham, 0)
    return out


@pytest.fixture(scope="module")
def T():
    return bf.ref_tables()


@pytest.mark.parametrize("case", ["full"] + CASES)
@pytest.mark.parametrize("mode", ["sync_se", "old_format_pe"])
def test_stage_join_of_forged_queries_at_the_ends(ctx, orc, worlds, edges, T, mode, case):
    if case == "full":
        t = worlds(mode)
        values, taxids, d, db = t.values, t.taxids, t.dbdir, t.db
    else:
        e = edges(mode, case)
        t = e.t
        values, taxids, d, db = e.values, e.taxids, e.dir, e.db
    q = _forged_queries(values, t.p.kmer_format)
    assert (_seq(q) == 0).any() and (q["value"] > values[-1]).any()
    assert (q["value"] < values[0]).any() or values[0] >> AA == 0
    ix = ctx.open_index(d, _mparams(t))
    try:
        m = ctx.sort_matches(ctx.match(ix, q), 6)
    finally:
        ix.close()
    spec = _as_records(bf.sort_matches_spec(bf.join_spec(T, values, taxids.view(np.uint32), t.world.tax.species_of, q["value"], q["qinfo"], kmer_format=t.p.kmer_format)))
    mo = orc.sort_matches(orc.match(db, q[_seq(q) != 0]))          # (blank slots are the HIP path's own: the oracle is never handed one)
    assert m.tobytes() == spec.tobytes(), (len(m), len(spec))
    assert m.tobytes() == mo.tobytes(), (len(m), len(mo))
    if len(values) >= 2:
        assert len(m) > 0                                         # the first target (a candidate) was met


# ---- views ----

@pytest.mark.parametrize("is_last", [False, True])
@pytest.mark.parametrize("cut", ["mid_run", "aa_boundary", "to_end"])
def test_view_final_entry_is_a_candidate_unless_the_view_is_last(ctx, worlds, T, cut, is_last):
    """Index.slice(lo, hi, is_last): the view [lower_bound(lo), lower_bound(hi)) of the parent; its final entry is a candidate exactly when
    is_last is False (join_spec(match_last=...)).  The views start and end inside runs of one amino-acid part, so the queries of those runs
    meet the view's first / final entry."""
    t = worlds("sync_se")
    v = t.values
    aa = _aa(v)
    inrun = np.flatnonzero(aa[1:] == aa[:-1]) + 1                  # entries whose predecessor has their amino-acid part
    inrun = inrun[v[inrun] != v[inrun - 1]]
    qa = set(int(x) for x in np.unique(_aa(t.ref["kmers"]["value"])))
    hit = [int(i) for i in inrun if int(aa[i]) in qa]
    assert len(hit) > 8
    lo_i, hi_i = hit[len(hit) // 5], hit[3 * len(hit) // 5]
    lo = int(v[lo_i])
    if cut == "mid_run":
        hi = int(v[hi_i])                                         # the view ends one entry before hi_i: its final entry's run continues
    elif cut == "aa_boundary":
        hi = (int(v[hi_i]) & ~0xFFFFFF) + (1 << 24)
    else:
        hi = 0xFFFFFFFFFFFFFFFF
    j0 = int(np.searchsorted(v, np.uint64(lo), side="left"))
    j1 = len(v) if hi == 0xFFFFFFFFFFFFFFFF else int(np.searchsorted(v, np.uint64(hi), side="left"))
    vv, vt = v[j0:j1], t.taxids[j0:j1]
    k = t.ref["kmers"]
    a0, a1 = _aa(vv[0]), _aa(vv[-1])
    near = (_aa(k["value"]) >= a0 - np.uint64(1)) & (_aa(k["value"]) <= a1 + np.uint64(1))
    q = k[near & ((_aa(k["value"]) <= a0 + np.uint64(40)) | (_aa(k["value"]) >= a1 - np.uint64(40)))]
    q = q[_seq(q) != 0]
    import metabuli_amd as M
    f = np.zeros(4, M.kmer_dt)                                    # and queries equal to / next to the view's first and final entries
    f["value"] = [vv[0], vv[0] ^ np.uint64(1), vv[-1], vv[-1] ^ np.uint64(8)]
    f["qinfo"] = (np.arange(1, 5, dtype=np.uint64) << np.uint64(32)) | np.uint64(3)
    q = np.sort(np.concatenate([q, f]), order=["value", "qinfo"])
    assert (_aa(q["value"]) == a1).any() and (_aa(q["value"]) == a0).any()       # queries meet the view's first and final runs
    spec = bf.join_spec(T, vv, vt.view(np.uint32), t.world.tax.species_of, q["value"], q["qinfo"], kmer_format=2, match_last=not is_last)
    ex = bf.join_spec(T, vv, vt.view(np.uint32), t.world.tax.species_of, q["value"], q["qinfo"], kmer_format=2, match_last=is_last)
    ix = ctx.open_index(t.dbdir, _mparams(t))
    view = ix.slice(lo, hi, is_last)
    try:
        assert view.num_targets == len(vv)
        m = ctx.sort_matches(ctx.match(view, q), t.n_reads)
    finally:
        view.close(); ix.close()
    exp = _as_records(bf.sort_matches_spec(spec))
    assert m.tobytes() == exp.tobytes(), (len(m), len(exp))
    assert len(spec) != len(ex)                                   # the final entry is met: the flag decides
