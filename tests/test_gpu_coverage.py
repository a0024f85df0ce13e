"""GPU tests of the k-mer coverage (mtb_index_coverage_*, kernels_coverage.h, the hook at the end of classify_attempt, `mtb_classify
--kmer-coverage 1`): the library's report against tests/coverage_spec.py, integer for integer.  The spec is fed the ORACLE's metamers
and results, so a test of the fused path also says that the device's sorted list and rows are the oracle's."""
import os
import subprocess

import numpy as np
import pytest

import coverage_spec as cs
from helpers import kmer_dt, result_dt, tax2species_table

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = np.uint64


def _ctx(**env):
    """a context made under index-open switches (they are read from the environment once, by mtb_ctx_create)"""
    import metabuli_amd as M
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return M.Context(0)
    finally:
        for k, v in old.items():                       # what the caller of pytest had set stays set
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def ctx():
    c = _ctx()
    yield c
    c.close()


class ToySpec:
    """a conftest.Toy, its species table as KmerMatcher::loadTaxIdList builds it, and the spec's report of one pass of its reads"""

    def __init__(self, orc, toy):
        self.toy = toy
        self.table = tax2species_table(orc, toy.tax, toy.taxids, max(toy.world.tax.parent))
        self.one = self.spec().add_batch(toy.ref["kmers"], toy.ref["results"]).report()

    def spec(self):
        t = self.toy
        return cs.Coverage(t.values, t.taxids.astype(np.uint32), self.table)

    def params(self):
        import metabuli_amd as M
        p = self.toy.p
        return M.default_params(seq_mode=p.seq_mode, syncmer=p.syncmer, kmer_format=p.kmer_format)

    def reads(self):
        t = self.toy
        return (t.b1, t.o1, t.b2, t.o2)


@pytest.fixture(scope="module")
def toys(orc, tmp_path_factory):
    from conftest import Toy, TOY_MODES
    made = {}

    def get(mode):
        if mode not in made:
            made[mode] = ToySpec(orc, Toy(orc, tmp_path_factory.mktemp("cov_" + mode), **TOY_MODES[mode]))
        return made[mode]
    return get


@pytest.fixture(scope="module")
def sync_se(toys):
    return toys("sync_se")


# ---- 1. the stage call at the edges -----------------------------------------------------------------------------------------------
def _metamers(rng, n):
    """n distinct format-2 words (eight amino-acid letters 0..20 above 24 DNA bits), ascending, none below 2^24"""
    letters = rng.integers(0, 21, size=(int(n * 1.2) + 64, 8)).astype(U64)
    v = rng.integers(0, 1 << 24, size=len(letters)).astype(U64)
    for k in range(8):
        v |= letters[:, k] << U64(24 + 5 * k)
    v = np.unique(v)
    v = v[v >= U64(1 << 24)]
    return np.sort(rng.choice(v, size=n, replace=False))


@pytest.fixture(scope="module")
def edge_world(tmp_path_factory):
    from metabuli_amd import synth
    w = synth.make_world(seed=3, n_genera=2, species_per_genus=2, strains_per_species=1, genome_len=100)
    d = str(tmp_path_factory.mktemp("cov_edge_tax"))
    w.tax.write(d)
    return w, d


def _q(value, read):
    return (int(value), read << 32)


@pytest.mark.parametrize("T", [1, 2, 31, 32, 33, 63, 64, 65, 4097])
def test_stage_call_at_the_edges(ctx, edge_world, T):
    import metabuli_amd as M
    w, taxdir = edge_world
    sp3 = w.species[:3]
    rng = np.random.default_rng(100 + T)
    values = _metamers(rng, T)
    taxids = np.array([sp3[i % 3] for i in range(T)], np.int32)
    p = M.default_params(seq_mode=1, syncmer=1)
    b = ctx.builder(taxdir, p)
    b.add_records(values, taxids)
    ix = b.finish()
    b.close()
    try:
        gv, gi = ix.download()
        assert (gv == values).all() and (gi == taxids.astype(np.uint32)).all()
        table = np.zeros(max(w.tax.parent) + 1, np.int64)
        for s in set(taxids.tolist()):                 # the builder's species table covers the ids that were added
            table[s] = s
        assert all(M.lib().mtb_tax_species(ix.h, int(s)) == int(table[s]) for s in range(len(table)) if s in sp3 or s == w.species[3])
        # reads 1..3: classified as the three species; read 4: the species no entry has; read 5: unclassified; reads 6..305: species sp3[0]
        res = np.zeros(305, result_dt)
        res["is_classified"] = 1; res[4]["is_classified"] = 0
        res["classification"] = sp3[0]
        for r in range(3):
            res[r]["classification"] = sp3[r]
        res[3]["classification"] = w.species[3]
        # entry 0, the entries on both sides of EVERY 32-bit word boundary of the bitmap, the last two entries
        at = sorted({t for t in [0, 1, T - 2, T - 1] + [b + d for b in range(32, T + 32, 32) for d in (-2, -1, 0, 1)] if 0 <= t < T})
        q = []
        for t in at:                                   # the entry's own species, another species, the unclassified read
            own = 1 + t % 3
            q += [_q(values[t], own), _q(values[t], 1 + (t + 1) % 3), _q(values[t], 4), _q(values[t], 5)]
        for r in (1, 2, 3):
            q += [_q(values[0] - U64(1), r), _q(0, r), _q(values[-1] + U64(1), r), _q((1 << 64) - 1, r),          # below the first value, above the last
                  _q((U64(20) << U64(59)) | (values[-1] & U64((1 << 59) - 1)), r)]                               # ... with valid letters too
        if T >= 2:
            gaps = np.flatnonzero(values[1:] - values[:-1] > U64(1))
            for g in gaps[:: max(1, len(gaps) // 6)]:                                                            # between two entries: an empty bucket, or an absent value in a full one
                q += [_q(values[g] + U64(1), 1 + int(g) % 3), _q(values[g] + (values[g + 1] - values[g]) // U64(2), 1 + (int(g) + 1) % 3)]
        hot = values[0]                                # entry 0 is sp3[0]'s: 300 reads of one species, more than a wave on one bit
        q += [_q(hot, r) for r in range(6, 306)]
        q.append((int(hot), 0))                        # a blank record
        q = np.array(q, dtype=kmer_dt)
        q = q[np.random.default_rng(T).permutation(len(q))]
        spec = cs.Coverage(values, taxids.astype(np.uint32), table).add_batch(q, res).report()
        assert int(spec["hits"][sp3[0]]) >= 300 and spec["n_marked"] == len(at)
        ix.coverage_begin()
        before = ix.state()
        ctx.coverage_mark(ix, q, res)
        got = ix.coverage_report()
        cs.same_report(got, spec)
        assert got["n_marked"] == len(at) and ix.state() == before
        # the hot query alone, on a fresh bitmap: hits 300, distinct 1
        ix.coverage_end(); ix.coverage_begin()
        ctx.coverage_mark(ix, np.array([_q(hot, r) for r in range(6, 306)], dtype=kmer_dt), res)
        got = ix.coverage_report()
        assert int(got["hits"][sp3[0]]) == 300 and int(got["distinct"][sp3[0]]) == 1 and got["n_marked"] == 1 and got["n_hits"] == 300
        ix.coverage_end()
    finally:
        ix.close()


# ---- 2. index states ------------------------------------------------------------------------------------------------------------------
STATES = {
    "no-directory": (dict(MTB_NO_DIR="1"), None, dict(dir_depth=0, packed=False, sealed=False)),
    "shallow-directory": (dict(), None, dict(packed=False, sealed=False)),
    "depth-7-flat": (dict(MTB_DIR_DEPTH="7", MTB_NO_PACK="1"), None, dict(dir_depth=7, packed=False, sealed=False)),
    "packed": (dict(MTB_DIR_DEPTH="7"), "classify", dict(dir_depth=7, packed=True, sealed=False)),
    "sealed": (dict(MTB_DIR_DEPTH="7"), "seal", dict(dir_depth=7, packed=True, sealed=True)),
}


@pytest.mark.parametrize("state", list(STATES))
def test_index_states(sync_se, state):
    env, prepare, want = STATES[state]
    t = sync_se.toy
    c = _ctx(**env)
    p = sync_se.params()
    ix = c.open_index(t.dbdir, p)
    try:
        if prepare == "classify":                      # the fused path packs a depth-7 index
            c.classify_batch(ix, p, t.b1[:int(t.o1[8])], t.o1[:9])
        elif prepare == "seal":
            ix.seal()
        before = ix.state()
        assert all(before[k] == v for k, v in want.items()), before
        if state == "shallow-directory":
            assert 0 < before["dir_depth"] < 7
        ix.coverage_begin()
        c.coverage_mark(ix, t.ref["kmers"], t.ref["results"])
        got = ix.coverage_report()
        assert ix.state() == before                    # coverage never converts the index
        cs.same_report(got, sync_se.one)
        assert got["n_marked"] == 34446 and got["n_hits"] == 35543
    finally:
        ix.close(); c.close()


# ---- 3. long equal-value runs ---------------------------------------------------------------------------------------------------------
def test_long_equal_value_runs(orc, tmp_path):
    from conftest import HotToy
    h = HotToy(orc, tmp_path / "hot")
    ts = ToySpec(orc, h)
    run = np.diff(np.flatnonzero(np.concatenate([[True], h.values[1:] != h.values[:-1], [True]]))).max()
    assert run >= 20, run                              # entries with one 64-bit value: the species with identical codons
    c = _ctx()
    p = ts.params()
    ix = c.open_index(h.dbdir, p)
    try:
        ix.coverage_begin()
        res, tt, tc = c.classify_batch(ix, p, h.b1, h.o1)
        assert (res["classification"] == h.ref["results"]["classification"]).all()
        got = ix.coverage_report()
        cs.same_report(got, ts.one)
        assert got["n_marked"] > 0
    finally:
        ix.close(); c.close()


# ---- 4. the fused path ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["sync_se", "dense_pe", "sync_long", "old_format_pe"])      # (the last one: kmer_format 1, base-21 amino-acid parts)
def test_fused_path(toys, ctx, mode):
    ts = toys(mode)
    t = ts.toy
    p = ts.params()
    ix = ctx.open_index(t.dbdir, p)
    try:
        off = ctx.classify_batch_packed(ix, p, *ts.reads())
        ix.coverage_begin()
        on = ctx.classify_batch_packed(ix, p, *ts.reads())
        got = ix.coverage_report()
        cs.same_report(got, ts.one)
        for a, b in zip(off, on):                      # rows and taxID:count lists: byte-equal to the run with coverage off
            assert a.tobytes() == b.tobytes()
        assert (on[0]["classification"] == t.ref["results"]["classification"]).all()
        rep, counts = ctx.audit_database(t.dbdir)
        assert rep["valid"] and np.array_equal(got["total"][1:], counts[1:].astype(U64))
        again = ix.coverage_report()                   # nothing is cleared
        cs.same_report(again, ts.one)
        ix.coverage_end()
        after = ctx.classify_batch_packed(ix, p, *ts.reads())
        assert all(a.tobytes() == b.tobytes() for a, b in zip(off, after))
    finally:
        ix.close()


# ---- 5. accumulation ------------------------------------------------------------------------------------------------------------------
def _tiled(t, k):
    """the reads of a single-end toy k times over, and the oracle's metamers and rows of that batch"""
    n = t.n_reads
    o1 = np.concatenate([[0], np.cumsum(np.tile(np.diff(t.o1.astype(np.int64)), k))]).astype(U64)
    km = np.tile(t.ref["kmers"], k)
    km["qinfo"] += np.repeat(np.arange(k, dtype=U64) * U64(n), len(t.ref["kmers"])) << U64(32)
    return np.tile(t.b1, k), o1, km, np.tile(t.ref["results"], k)


def test_accumulation_over_batches_sub_batches_and_streams(sync_se):
    t = sync_se.toy
    p = sync_se.params()
    c = _ctx()
    ix = c.open_index(t.dbdir, p)
    try:
        # two batches
        ix.coverage_begin()
        half = t.n_reads // 2
        cut = int(t.o1[half])
        c.classify_batch(ix, p, t.b1[:cut], t.o1[:half + 1])
        c.classify_batch(ix, p, t.b1[cut:], (t.o1[half:] - t.o1[half]).astype(U64))
        want = dict(sync_se.one, n_batches=2)
        cs.same_report(ix.coverage_report(), want)
        # the same batch again: hits double, distinct stays
        c.classify_batch(ix, p, t.b1, t.o1)
        got = ix.coverage_report()
        assert np.array_equal(got["hits"], 2 * sync_se.one["hits"]) and np.array_equal(got["distinct"], sync_se.one["distinct"])
        assert got["n_marked"] == sync_se.one["n_marked"] and got["n_batches"] == 3
        ix.coverage_end()
        # one batch in at least three sub-batches
        ix.coverage_begin()
        c.set_workspace_limit(max(int(t.o1[-1]) * 20, 200_000))
        c.classify_batch(ix, p, t.b1, t.o1)
        assert c.last_sub_batches >= 3, c.last_sub_batches
        c.set_workspace_limit(0)
        cs.same_report(ix.coverage_report(), sync_se.one)
        ix.coverage_end()
        # two stream lanes: the batch tiled past 4096 reads per lane (no smaller batch is split)
        k = -(-4096 * 2 // t.n_reads)
        b1, o1, km, rows = _tiled(t, k)
        want = sync_se.spec().add_batch(km, rows).report()
        assert np.array_equal(want["hits"], U64(k) * sync_se.one["hits"]) and np.array_equal(want["distinct"], sync_se.one["distinct"])
        ix.coverage_begin()
        c.classify_batch(ix, p, b1, o1)
        single = ix.coverage_report()
        cs.same_report(single, want)
        ix.coverage_end(); ix.coverage_begin()
        c.set_streams(2)
        c.set_profiling(True)
        res, tt, tc = c.classify_batch(ix, p, b1, o1)
        assert c.last_stats().n_launch[1] == 2         # MTB_K_EXTRACT_EMIT: one extraction per lane, the lanes path ran
        c.set_streams(1)
        assert (res["classification"] == rows["classification"]).all()
        cs.same_report(ix.coverage_report(), want)
        ix.coverage_end()
    finally:
        ix.close(); c.close()


# ---- 6. a failed call -----------------------------------------------------------------------------------------------------------------
def test_failed_call_counts_nothing(sync_se):
    import ctypes as C
    import metabuli_amd as M
    t = sync_se.toy
    p = sync_se.params()
    c = _ctx()
    ix = c.open_index(t.dbdir, p)
    try:
        ix.coverage_begin()
        c.set_workspace_limit(max(int(t.o1[-1]) * 20, 200_000))
        n = t.n_reads
        res = np.zeros(n, result_dt); tt = np.zeros(8, np.int32); tc = np.zeros(8, np.uint32); cnt = C.c_uint64()
        st = c.L.mtb_classify_batch(c.h, ix.h, C.byref(p), M._p(t.b1), M._p(t.o1), None, None, C.c_uint64(n), M._p(res), M._p(tt), M._p(tc), C.c_uint64(8), C.byref(cnt))
        assert st == M.MTB_ERR_CAPACITY and cnt.value > 8 and c.last_sub_batches >= 2
        failed = ix.coverage_report()
        assert failed["n_hits"] == 0 and failed["n_batches"] == 0 and failed["n_queries"] == 0      # (the marks of the finished sub-batches may stand)
        got_rows, _, _ = c.classify_batch(ix, p, t.b1, t.o1)                                       # the caller repeats the batch, with room
        assert (got_rows["classification"] == t.ref["results"]["classification"]).all()
        cs.same_report(ix.coverage_report(), sync_se.one)
        # ... and through the binding's own exact-size retry
        ix.coverage_end(); ix.coverage_begin()
        c.classify_batch(ix, p, t.b1, t.o1, taxcnt_cap=8)
        assert c.last_capacity_retries >= 1
        cs.same_report(ix.coverage_report(), sync_se.one)
    finally:
        ix.close(); c.close()


# ---- 7. merge ---------------------------------------------------------------------------------------------------------------------------
def test_merge_of_a_clone(sync_se, ctx):
    import metabuli_amd as M
    t = sync_se.toy
    p = sync_se.params()
    c2 = _ctx()
    ix = ctx.open_index(t.dbdir, p)
    clone = c2.clone_index(ix)
    other = None
    try:
        ix.coverage_begin()
        with pytest.raises(M.MtbError) as e:           # the clone's coverage is off
            ix.coverage_merge(clone)
        assert e.value.status == M.MTB_ERR_ARG
        clone2 = ctx.clone_index(ix)                   # a clone of an index with coverage on starts with coverage off
        with pytest.raises(M.MtbError) as e:
            clone2.coverage_report()
        assert e.value.status == M.MTB_ERR_ARG
        clone2.close()
        clone.coverage_begin()
        half = t.n_reads // 2
        cut = int(t.o1[half])
        ctx.classify_batch(ix, p, t.b1[:cut], t.o1[:half + 1])
        c2.classify_batch(clone, p, t.b1[cut:], (t.o1[half:] - t.o1[half]).astype(U64))
        part = ix.coverage_report()
        assert 0 < part["n_marked"] < sync_se.one["n_marked"]
        ix.coverage_merge(clone)
        cs.same_report(ix.coverage_report(), dict(sync_se.one, n_batches=2))
        assert clone.coverage_report()["n_batches"] == 1                            # the source is unchanged
        with pytest.raises(M.MtbError) as e:
            ix.coverage_merge(ix)
        assert e.value.status == M.MTB_ERR_ARG
        # an index of another size
        b = ctx.builder(os.path.join(t.dbdir, "taxonomy"), p)
        b.add_records(t.values[:1000], t.taxids[:1000])
        other = b.finish(); b.close()
        other.coverage_begin()
        with pytest.raises(M.MtbError) as e:
            ix.coverage_merge(other)
        assert e.value.status == M.MTB_ERR_ARG
    finally:
        if other is not None:
            other.close()
        clone.close(); ix.close(); c2.close()


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals(sync_se, ctx):
    import metabuli_amd as M
    t = sync_se.toy
    p = sync_se.params()
    ix = ctx.open_index(t.dbdir, p)

    def refused(status, f, *a, **kw):
        with pytest.raises(M.MtbError) as e:
            f(*a, **kw)
        assert e.value.status == status, e.value

    try:
        km, rows = t.ref["kmers"], t.ref["results"]
        refused(M.MTB_ERR_ARG, ix.coverage_report)                         # report, mark and end without begin
        refused(M.MTB_ERR_ARG, ctx.coverage_mark, ix, km, rows)
        refused(M.MTB_ERR_ARG, ix.coverage_end)
        ix.coverage_begin()
        refused(M.MTB_ERR_ARG, ix.coverage_begin)                          # twice
        refused(M.MTB_ERR_CAPACITY, ix.coverage_report, cap=ix.max_taxid())
        bad = km[:64].copy()
        bad[17]["qinfo"] = (U64(len(rows) + 1) << U64(32)) | U64(5)        # a sequenceID beyond the rows: refused on the host, nothing is launched or counted
        refused(M.MTB_ERR_ARG, ctx.coverage_mark, ix, bad, rows)
        got = ix.coverage_report()
        assert got["n_marked"] == 0 and got["n_queries"] == 0 and got["n_batches"] == 0
        ix.coverage_end()
        ix.coverage_begin(); ix.coverage_end()                             # begin again after end
        v = ix.slice(int(t.values[100]), int(t.values[-100]), False)
        try:
            refused(M.MTB_ERR_UNSUPPORTED, v.coverage_begin)
        finally:
            v.close()
        part = ctx.open_index_part(t.dbdir, sync_se.params(), 0, 2)
        try:
            refused(M.MTB_ERR_UNSUPPORTED, part.coverage_begin)
        finally:
            part.close()
    finally:
        ix.close()


# ---- 9. the driver ----------------------------------------------------------------------------------------------------------------------
def _exe():
    import metabuli_amd as M
    d = os.path.dirname(M.LIB_PATH)
    if not os.environ.get("MTB_HIPEMU"):
        subprocess.check_call(["make", "-C", d, "mtb_classify"], stdout=subprocess.DEVNULL)
    return os.path.join(d, "mtb_classify")


def test_driver_writes_the_coverage_file(sync_se, tmp_path):
    t = sync_se.toy
    names = [f"read{i}" for i in range(t.n_reads)]
    fq = str(tmp_path / "r.fq")
    with open(fq, "w") as f:
        for i, nm in enumerate(names):
            s = bytes(t.b1[int(t.o1[i]):int(t.o1[i + 1])]).decode()
            f.write(f"@{nm}\n{s}\n+\n{'I' * len(s)}\n")
    outs = {}
    for tag, extra in (("plain", []), ("cov", ["--kmer-coverage", "1"]), ("cov2", ["--kmer-coverage", "1", "--devices", "0,0"]), ("off", ["--kmer-coverage", "0"])):
        d = tmp_path / tag
        d.mkdir()
        subprocess.check_call([_exe(), "--seq-mode", "1"] + extra + [fq, t.dbdir, str(d), "job"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        outs[tag] = {f: open(d / f, "rb").read() for f in sorted(os.listdir(d))}
    three = ["job_classifications.tsv", "job_krona.html", "job_report.tsv"]
    assert sorted(outs["plain"]) == three and sorted(outs["off"]) == three
    assert sorted(outs["cov"]) == sorted(three + ["job_kmer_coverage.tsv"]) == sorted(outs["cov2"])
    for f in three:
        assert outs["cov"][f] == outs["plain"][f] and outs["cov2"][f] == outs["plain"][f] and outs["off"][f] == outs["plain"][f], f
    counts = {}
    for x in t.ref["results"]["classification"].tolist():
        counts[x] = counts.get(x, 0) + 1
    one = sync_se.one
    want = cs.format_rows(cs.rows(counts, sync_se.table, one["distinct"], one["hits"], one["total"]), t.world.tax.name)
    assert want.count("\n") == 13                      # the header and twelve species
    assert outs["cov"]["job_kmer_coverage.tsv"].decode() == want
    assert outs["cov2"]["job_kmer_coverage.tsv"] == outs["cov"]["job_kmer_coverage.tsv"]
