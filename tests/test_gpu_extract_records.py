"""What k_extract<2> (the single-pass, ordinal-tagging extractor of kernels_extract.h) and the fused amino-acid sort of kernels_sort.h
WRITE, record by record, against the oracle's extraction -- the rest of the suite sees these two kernels only through the matches and
scores that follow them.

The seam is mtb_part_extract with one partition (bounds = [0]) and part_starts given (helpers.part_extract_records): exactly
dev_extract (single pass, tagged, with the digit side array) followed by dev_sort (MTB_SORT_AA6, all six letters); it returns the
sorted list, blank tail records included, and needs no index.  `check_records` states what that list must be: the oracle's metamers,
each exactly once, ordered on the leading amino-acid letters, every read's ordinal tags (bits 16..31 of the position field) the numbers
0 .. total-1 in the order (mate, frame, position rising), blanks all-zero -- and that the call really took the single pass.

Next to it: the capacity-overflow retry of dev_extract through the fused batch (where mtb_batch_stats shows the second launch), and
the two-pass stage kernels k_extract<0> / <1> (ctx.extract, exact emission order) at the same lane, staging and chunk edges -- the GPU
twin of test_core_vs_oracle.py::test_extract_edge_cases, which runs sequential calls of mtb_core.h and not the kernel's lane geometry.

Not reachable through this seam, and not covered here: the long-read single pass (seq_mode 3 with per-read counts), off_flags and its
counters, the ordinal clamp at 0xFFFF, and the per-read lengths the single pass writes (they stay on the device; the two-pass cases
compare theirs).  MTB_SORT_PAIRS does not reach this call either: mtb_part_extract always asks dev_sort for all six letters (shift 34);
only mtb_classify_batch's own sort reads the switch, so it has no case below.

Everything is integer and compared bit for bit.  A subset runs in the CPU suite on the emulated build (tests/test_hipemu.py)."""
import numpy as np
import pytest

from test_gpu_scorer_tiers import (EXTRACT_BUF, K_EXTRACT_EMIT, SLOT_MAX_POS, SLOT_MAX_Q, SORT_SIZES, SORT_TILE, Reads, World, _sort_batch, check,
                                   metamers_per_read, sort_records)

pytestmark = pytest.mark.gpu

EXTRACT_GRID = 256 * 256                                 # mtb_api.hip dev_extract: workgroups (one wave each) of a launch at most
ORD_BITS = np.uint64(0xFFFF0000)                         # the ordinal tag inside qinfo's position field
ACGT = np.frombuffer(b"ACGT", np.uint8)
ODD_BYTES = np.frombuffer(b"NnRY-*acgt\x00\x80\xff", np.uint8)


# ------------------------------------------------------------------ inputs
def random_reads(lengths, seed, odd=0.02):
    """one read per entry of `lengths`: random ACGT, a fraction `odd` of the bases replaced by ambiguity codes, lower case, gap and
    stop characters and bytes outside ASCII"""
    rng = np.random.default_rng(seed)
    offs = np.concatenate([[0], np.cumsum(np.asarray(lengths, np.int64))]).astype(np.uint64)
    b = ACGT[rng.integers(0, 4, size=int(offs[-1]))]
    if odd:
        m = rng.random(len(b)) < odd
        b[m] = ODD_BYTES[rng.integers(0, len(ODD_BYTES), size=int(m.sum()))]
    return Reads(b, offs)


def clean_and_odd(lengths, seed):
    """every length twice: one read of plain ACGT (the full window count of its length) and one with odd bytes"""
    return random_reads(lengths, seed, odd=0) + random_reads(lengths, seed + 1)


def permuted(r, seed):
    """the reads of r in another order (the mates of a pair batch)"""
    order = np.random.default_rng(seed).permutation(r.n)
    lens = np.diff(r.o1.astype(np.int64))[order]
    parts = [r.b1[int(r.o1[i]):int(r.o1[i + 1])] for i in order]
    return Reads(np.concatenate(parts) if parts else r.b1[:0], np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64))


def pair_up(r1, r2):
    assert r1.n == r2.n
    return Reads(r1.b1, r1.o1, r2.b1, r2.o1)


def params_of(**kw):
    """the same parameters for the oracle and for the library"""
    import metabuli_amd as M
    from helpers import default_params
    return default_params(**kw), M.default_params(**kw)


# ------------------------------------------------------------------ the checker
def single_pass_records(per):
    """length of the single pass's list for reads with `per` metamers each: read r goes to wave r % grid, a wave whose reads stay
    within MTB_EXTRACT_BUF together flushes once, at its end, into a chunk of need + 65 records (sort_records of
    test_gpu_scorer_tiers.py, for more than one read per wave); None where a wave flushes more than once"""
    grid = min(len(per), EXTRACT_GRID)
    wave = np.bincount(np.arange(len(per)) % grid, weights=per, minlength=grid).astype(np.int64)
    if wave.max(initial=0) > EXTRACT_BUF:
        return None
    return int(wave.sum() + 65 * (wave > 0).sum())


def check_records(rec, ok, ql, ql2, kmer_format, paired, tag):
    """rec: the sorted list mtb_part_extract returned; ok, ql, ql2: orc.extract_batch of the same reads"""
    n_reads = len(ql)
    u = np.uint64
    sid = ((rec["qinfo"] >> u(32)) & u(0x1FFFFFFF)).astype(np.int64)
    real = rec[sid != 0]
    blank = rec[sid == 0]
    per = metamers_per_read(ok, n_reads)
    # 1. the single pass, not mtb_part_extract's two-pass fallback: the batch fits the slot records, and blank tails exist
    assert per.max(initial=0) <= SLOT_MAX_Q, (tag, int(per.max()))
    assert (ql.astype(np.int64) + ql2 + 3 < SLOT_MAX_POS).all(), tag
    if len(ok):
        assert len(rec) > len(ok), (tag, len(rec), len(ok))
    want = single_pass_records(per)
    if want is not None:
        assert len(rec) == want, (tag, len(rec), want)
    # 2. blanks are all-zero, and every other record is one of the oracle's
    assert (blank["value"] == 0).all() and (blank["qinfo"] == 0).all(), tag
    assert len(real) == len(ok), (tag, len(real), len(ok))
    # 3. ordered on the leading amino-acid letters (kmer_format 1: on the upper word), blanks included
    key = rec["value"] >> u(34 if kmer_format == 2 else 32)
    assert (key[1:] >= key[:-1]).all(), (tag, int(np.flatnonzero(key[1:] < key[:-1])[0]))
    # 4. content: without the tags, in (read, ordinal) order = the oracle's records in (read, mate, frame, position) order
    rs = sid[sid != 0]
    ordinal = ((real["qinfo"] >> u(16)) & u(0xFFFF)).astype(np.int64)
    got = real[np.lexsort((ordinal, rs))]
    osid = ((ok["qinfo"] >> u(32)) & u(0x1FFFFFFF)).astype(np.int64)
    opos = (ok["qinfo"] & u(0xFFFFFFFF)).astype(np.int64)
    ofr = (ok["qinfo"] >> u(61)).astype(np.int64)
    assert opos.max(initial=0) < 1 << 16, tag
    omate = (opos >= ql.astype(np.int64)[osid - 1] + 3).astype(np.int64) if paired else np.zeros(len(ok), np.int64)
    exp = ok[np.lexsort((opos, ofr, omate, osid))]
    assert (got["value"] == exp["value"]).all(), (tag, int(np.flatnonzero(got["value"] != exp["value"])[0]))
    gq = got["qinfo"] & ~ORD_BITS
    assert (gq == exp["qinfo"]).all(), (tag, int(np.flatnonzero(gq != exp["qinfo"])[0]))
    # 5. ordinals: every read's tags are 0 .. total-1, in that order
    first = np.concatenate([[0], np.cumsum(per)])[:-1]
    want_ord = np.arange(len(ok), dtype=np.int64) - np.repeat(first, per)
    got_ord = ((got["qinfo"] >> u(16)) & u(0xFFFF)).astype(np.int64)
    assert (got_ord == want_ord).all(), (tag, int(np.flatnonzero(got_ord != want_ord)[0]))
    return per


def run_single_pass(ctx, orc, r, tag, **kw):
    from helpers import part_extract_records
    paired = r.b2 is not None
    po, pm = params_of(seq_mode=2 if paired else 1, **kw)
    ok, ql, ql2 = orc.extract_batch(po, r.b1, r.o1, r.b2, r.o2)
    rec = part_extract_records(ctx, pm, r.b1, r.o1, r.b2, r.o2)
    return check_records(rec, ok, ql, ql2, po.kmer_format, paired, tag)


# ------------------------------------------------------------------ fixtures
@pytest.fixture(scope="module")
def ctx():
    import metabuli_amd as M
    c = M.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def worlds(orc, tmp_path_factory):
    """the toy worlds of test_gpu_scorer_tiers.py by syncmer mode, each built when a case first asks for it"""
    class Lazy(dict):
        def __missing__(self, s):
            self[s] = World(orc, tmp_path_factory.mktemp(f"records_sync{s}"), s)
            return self[s]
    return Lazy()


# ------------------------------------------------------------------ (a) single pass: lane, staging and chunk edges
def _span(lo, hi):
    return list(range(lo, hi + 1))


# name -> (reads, extraction parameters, the per-read metamer counts the case is there to reach)
def _single_pass_case(name):
    if name == "dense-fmt2":
        # too-short reads, n_win 1..64 (6 n_win metamers: 384 at 216 bases; 219 would leave the slot records), 3 n_win across 64 / 128 / 192
        # lanes; from 183 bases on a read overfills the 320-record buffer and flushes mid-read
        return clean_and_odd(_span(0, 59) + _span(140, 216), 101), dict(syncmer=0), lambda per: per.max() == 384 and (per == 6).any()
    if name == "sync5-staging-edge":
        # MTB_EXTRACT_STAGE = 320 / 321: the last staged and the first unstaged length, the backwards walk with two chunks per frame
        return clean_and_odd(_span(300, 344), 103), dict(syncmer=1, smer_len=5), lambda per: per.min() > 64
    if name == "sync3-chunk-edge":
        # n_win = used_len / 3 - 7 of 127, 128, 129 at 408..416 bases: the 64-window chunk edge of the unstaged path
        return clean_and_odd(_span(396, 419) + [100, 30, 0, 500], 105), dict(syncmer=1, smer_len=3), lambda per: per.max() > 256
    if name == "sync7":
        # s = 7 selects every window: the dense counts through the syncmer arithmetic
        return clean_and_odd(_span(140, 216), 107), dict(syncmer=1, smer_len=7), lambda per: per.max() == 384
    if name == "oldfmt-dense":
        # kmer_format 1 is never staged, its FORWARD frames are the ones whose positions fall; the sort is the binary one on bits [32, 64)
        return clean_and_odd(_span(180, 216), 109), dict(syncmer=0, kmer_format=1), lambda per: per.max() == 384
    if name == "pairs-sync3":
        # a staged and an unstaged mate in either order, a pair skipped for one short mate, the mate-2 position offset
        m1 = clean_and_odd([100, 330, 25, 150, 60], 111)
        m2 = clean_and_odd([330, 100, 150, 25, 61], 113)
        return pair_up(m1, m2), dict(syncmer=1, smer_len=3), lambda per: (per == 0).sum() == 4 and per.max() > 128
    if name == "pairs-dense":
        r = clean_and_odd(_span(75, 100), 115)
        return pair_up(r, permuted(r, 116)), dict(syncmer=0), lambda per: per.max() > 256
    raise KeyError(name)


SINGLE_PASS_CASES = ["dense-fmt2", "sync5-staging-edge", "sync3-chunk-edge", "sync7", "oldfmt-dense", "pairs-sync3", "pairs-dense"]


@pytest.mark.parametrize("name", SINGLE_PASS_CASES)
def test_single_pass_records(ctx, orc, name):
    """k_extract<2> + the sort at the smallest shapes that cross each edge of the wave's geometry: 64 windows per step with the three
    frames of a strand laid end to end (staged reads), 8 codons read ahead behind a step, the 320-base staging edge, 64-window chunks
    walked backwards (unstaged reads), the 320-record LDS buffer flushed mid-read, both mates of a pair in one ordinal sequence."""
    r, kw, reached = _single_pass_case(name)
    per = run_single_pass(ctx, orc, r, name, **kw)
    assert reached(per), (name, int(per.max()), int(per.min()))


# ------------------------------------------------------------------ (b) flush and chunk edges
@pytest.mark.parametrize("n_metamers", [EXTRACT_BUF - 1, EXTRACT_BUF, EXTRACT_BUF + 1])
def test_buffer_flush_at_its_capacity(ctx, orc, worlds, n_metamers):
    """a read with exactly 319 / 320 / 321 metamers (MTB_EXTRACT_BUF = 320): the buffer just not full, exactly full (n_buf + c == 320 must
    not flush, and the store at slot 319 is the buffer's last), and one record over (a flush in the middle of the read, the chunk
    continued by the second flush); first of three reads, a wave per read"""
    w = worlds[1]
    r = w.tuned(1, n_metamers, n_metamers, seed=51) + w.sample(1, 2, 150, 52)
    per = run_single_pass(ctx, orc, r, n_metamers, syncmer=1)
    assert per[0] == n_metamers and r.n == 3


def test_two_reads_per_wave(ctx, orc):
    """more reads than the launch has waves (gridDim.x = 65536 < n_reads): the waves of the first reads take a second one, whose
    metamers join the first one's in the buffer and whose chunk is sized for a wave that has produced before"""
    n = 70000
    r = random_reads(np.random.default_rng(121).integers(30, 41, size=n), 122)
    assert r.n > EXTRACT_GRID
    per = run_single_pass(ctx, orc, r, "70000 reads", syncmer=0)
    assert ((per[:n - EXTRACT_GRID] > 0) & (per[EXTRACT_GRID:] > 0)).sum() > 1000       # waves whose two reads both have metamers


# ------------------------------------------------------------------ (c) the fused sort, record by record
SORT_VARIANTS = [None, "MTB_SORT_LSD", "MTB_SORT_NO_XCD"]


@pytest.mark.parametrize("name,n_bulk,band", SORT_SIZES, ids=lambda v: str(v))
def test_sorted_list_at_tile_edges(ctx, orc, worlds, name, n_bulk, band):
    """the batches of test_gpu_scorer_tiers.py::test_fused_sort_variants_at_tile_edges (lists of one scatter tile -8..0 and +1..+8 records,
    8 and 9 tiles, a top-letter bucket wider than a tile) under the default sort (MSD pass + bucket-local passes), MTB_SORT_LSD and
    MTB_SORT_NO_XCD: that test infers the order from the join's window statistics and the length from a tile count -- here every record
    of the list is accounted for, so a sort that drops one record and doubles another fails.  (MTB_SORT_PAIRS: see the module
    docstring.)"""
    from helpers import part_extract_records
    w = worlds[1]
    r = _sort_batch(w, name, n_bulk, band)
    po, pm = params_of(seq_mode=1, syncmer=1)
    ok, ql, ql2 = orc.extract_batch(po, r.b1, r.o1)
    per = metamers_per_read(ok, r.n)
    if name != "bucket-over-tiles":
        n_sorted = sort_records(per)
        assert single_pass_records(per) == n_sorted
        if band:
            assert band[0] <= n_sorted <= band[1], n_sorted
        tiles = -(-n_sorted // SORT_TILE)
        assert {"below-one-tile": tiles == 1, "one-tile-minus": tiles == 1, "one-tile-plus": tiles == 2, "eight-tiles": tiles == 8,
                "nine-tiles": tiles == 9}[name], (name, n_sorted)
    else:
        assert np.bincount((ok["value"] >> np.uint64(54)).astype(np.int64)).max() > SORT_TILE
    try:
        for sw in SORT_VARIANTS:
            if sw:
                ctx.set_option(sw, "1")
            rec = part_extract_records(ctx, pm, r.b1, r.o1)
            check_records(rec, ok, ql, ql2, 2, False, (name, sw))         # (with the list's length where sort_records applies)
            if sw:
                ctx.set_option(sw, None)
    finally:
        for sw in SORT_VARIANTS[1:]:
            ctx.set_option(sw, None)


# ------------------------------------------------------------------ (d) capacity overflow and the retry at the bound
def test_overflow_retry_through_the_fused_batch(orc, worlds):
    """dev_extract sizes the single pass's buffer from the previous batch's yield and repeats the launch at extract_bound when the
    extractor reports an overflow.  Batch A (3 reads and 97 reads of N only) leaves a yield near zero; batch B (600 reads, dense) then
    overflows the guessed buffer: two launches, the second into 2 n_bases + grid * 8192 records, and the oracle's rows from it; B again
    fits at the yield it left itself: one launch."""
    import metabuli_amd as M
    w = worlds[0]
    a = w.sample(1, 3, 150, 61) + Reads(np.full(97 * 150, ord("N"), np.uint8), np.arange(98, dtype=np.uint64) * 150)
    b = w.sample(1, 600, 150, 62)
    c = M.Context(0)
    c.set_profiling(True)
    p = M.default_params(seq_mode=1, syncmer=0)
    ix = c.open_index(w.dbdir, p)
    try:
        refs = {id(a): w.classify(1, a), id(b): w.classify(1, b)}
        launches = []
        for step, r in enumerate((a, b, b)):
            ref = refs[id(r)]
            res, tt, tc = c.classify_batch(ix, p, r.b1, r.o1)
            st = c.last_stats()
            check(ref, res, tt, tc, st, ("overflow", step))
            assert st.n_kmers == len(ref["kmers"]), (step, st.n_kmers, len(ref["kmers"]))
            launches.append(int(st.n_launch[K_EXTRACT_EMIT]))
        assert launches == [1, 2, 1], launches
    finally:
        ix.close(); c.close()


# ------------------------------------------------------------------ (e) the two-pass stage kernels at the same edges
TWO_PASS_LENGTHS = _span(0, 44) + _span(208, 223) + _span(315, 325) + _span(400, 415) + [1001, 4099]
TWO_PASS_PARAMS = {"dense": dict(syncmer=0), "sync3": dict(syncmer=1, smer_len=3), "sync5": dict(syncmer=1, smer_len=5),
                   "sync7": dict(syncmer=1, smer_len=7), "oldfmt": dict(syncmer=0, kmer_format=1)}


@pytest.mark.parametrize("paired", [False, True], ids=["se", "pe"])
@pytest.mark.parametrize("mode", list(TWO_PASS_PARAMS))
def test_two_pass_extract_at_lane_edges(ctx, orc, mode, paired):
    """k_extract<0> (count) and <1> (emit) through mtb_extract: the oracle's records in the oracle's order, and its used lengths, for
    reads around the too-short limit, one and several 64-window steps, the staging edge, and long unstaged reads -- alone and as pairs
    against a permutation of themselves"""
    r = random_reads(TWO_PASS_LENGTHS, 131)
    if paired:
        r = pair_up(r, permuted(r, 132))
    po, pm = params_of(seq_mode=2 if paired else 1, **TWO_PASS_PARAMS[mode])
    ok, ql, ql2 = orc.extract_batch(po, r.b1, r.o1, r.b2, r.o2)
    k, gl, gl2 = ctx.extract(pm, r.b1, r.o1, r.b2, r.o2)
    assert len(ok) > 5000 and (metamers_per_read(ok, r.n) == 0).any()
    assert (gl == ql).all() and (gl2 == ql2).all()
    assert len(k) == len(ok)
    assert (k["value"] == ok["value"]).all() and (k["qinfo"] == ok["qinfo"]).all()
