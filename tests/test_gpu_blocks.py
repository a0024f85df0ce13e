"""GPU tests of the block scan (mtb_extract_blocks, mtb_builder_add_blocks; kernels_extract_blocks.h): exact values, exact order and
exact block indices against the oracle's six-frame scan (tests/blocks_spec.py says how a block is one frame of it), on the shapes
at which the piece decomposition can go wrong.  P = MTB_BLOCK_PIECE_WINDOWS is read from the header."""
import ctypes as C
import os

import numpy as np
import pytest

import blocks_spec
from blocks_spec import make_blocks

pytestmark = pytest.mark.gpu

P = blocks_spec.piece_windows()
ACGT = np.frombuffer(b"ACGT", np.uint8)


@pytest.fixture(scope="module")
def ctx():
    import metabuli_amd as M
    c = M.Context(0)
    yield c
    c.close()


def _one(seq):
    return seq, np.array([0, len(seq)], np.uint64)


def _span(n_win, extra=0):
    """bases of a block with n_win windows (+ 0..2 bases that belong to no codon)"""
    return 3 * (n_win + 7) + extra


# ---------------------------------------------------------------------------------------------------------------------
# scenarios: name -> (bases, offs, blocks)
# ---------------------------------------------------------------------------------------------------------------------
def sc_short(rng):
    """1, 2, 23, 24, 25, 26 bases, both strands (the empty block, end = start - 1, is an argument error: test_argument_errors)"""
    seq = rng.choice(ACGT, size=100)
    rows = [(0, st, 30, 30 + n - 1) for n in (1, 2, 23, 24, 25, 26) for st in (1, -1)]
    return (*_one(seq), make_blocks(rows))


def sc_window_counts(rng):
    """63 .. 65, 127 .. 129, P - 1 .. P + 1, 2P + 1 windows; the block length leaves 0, 1 or 2 bases over; both strands; odd starts"""
    seq = rng.choice(ACGT, size=_span(2 * P + 1, 2) + 11)
    rows = []
    for i, n_win in enumerate((63, 64, 65, 127, 128, 129, P - 1, P, P + 1, 2 * P + 1)):
        for st in (1, -1):
            start = (i * 5 + (st > 0)) % 11
            rows.append((0, st, start, start + _span(n_win, i % 3) - 1))
    return (*_one(seq), make_blocks(rows))


def sc_ends(rng):
    """a block that touches base 0, one that touches the last base, the whole sequence -- on both strands, in two sequences of which the
    second starts right behind the first (a read past an end would take the neighbour's bases)"""
    a, b = rng.choice(ACGT, size=200), rng.choice(ACGT, size=331)
    rows = []
    for s, L in ((0, 200), (1, 331)):
        for st in (1, -1):
            rows += [(s, st, 0, 52), (s, st, L - 61, L - 1), (s, st, 0, L - 1)]
    return np.concatenate([a, b]), np.array([0, 200, 531], np.uint64), make_blocks(rows)


def sc_same_range_both_strands(rng):
    seq = rng.choice(ACGT, size=900)
    return (*_one(seq), make_blocks([(0, 1, 100, 700), (0, -1, 100, 700)]))


def sc_overlap(rng):
    """two overlapping blocks in one frame: the shared windows come out twice"""
    seq = rng.choice(ACGT, size=900)
    return (*_one(seq), make_blocks([(0, 1, 90, 450), (0, 1, 300, 720), (0, -1, 90, 450), (0, -1, 240, 450)]))


def sc_invalid_bases(rng):
    """an N at every codon phase; an N in a codon shared by the last window of a piece and the first window of the next one"""
    L = _span(P + 40)
    seq = rng.choice(ACGT, size=L + 10)
    rows = []
    for phase in range(3):
        seq[60 + 30 * phase + phase] = ord("N")
    fwd = seq.copy(); fwd[5 + 3 * (P + 3) + 1] = ord("N")            # codon P + 3 of the forward block below: windows P - 4 .. P + 3
    rev = seq.copy(); rev[5 + L - 1 - 3 * (P + 3) - 1] = ord("n")    # the same codon of the reverse block
    rows = [(0, 1, 5, 5 + L - 1), (1, -1, 5, 5 + L - 1), (0, -1, 0, 200), (1, 1, 2, 200)]
    return np.concatenate([fwd, rev]), np.array([0, L + 10, 2 * (L + 10)], np.uint64), make_blocks(rows)


def sc_many_blocks(rng):
    """70 000 blocks of 24 .. 60 bases over 200 kb: more pieces than one workgroup sweep of the count scan's first level (2048 per tile), so the
    scan recurses, and blocks without a window sit between the others"""
    seq = rng.choice(ACGT, size=200_000)
    seq[rng.integers(0, len(seq), size=300)] = ord("N")
    n = 70_000
    lens = rng.integers(24, 61, size=n)
    lens[::97] = rng.integers(1, 24, size=len(lens[::97]))         # some yield nothing
    start = rng.integers(0, len(seq) - 60, size=n)
    b = np.zeros(n, blocks_spec.block_dt)
    b["seq"] = 0; b["strand"] = np.where(rng.random(n) < 0.5, 1, -1); b["start"] = start; b["end"] = start + lens - 1
    return (*_one(seq), b)


def sc_three_sequences(rng):
    seqs = [rng.choice(ACGT, size=L) for L in (700, 1201, 333)]
    offs = np.zeros(4, np.uint64); offs[1:] = np.cumsum([len(s) for s in seqs])
    rows = [(2, 1, 3, 300), (0, -1, 10, 650), (1, 1, 0, 1200), (0, 1, 1, 699), (2, -1, 0, 332), (1, -1, 500, 900)]
    return np.concatenate(seqs), offs, make_blocks(rows)


def sc_no_blocks(rng):
    return (*_one(rng.choice(ACGT, size=100)), make_blocks([]))


SCENARIOS = {"short": sc_short, "window_counts": sc_window_counts, "ends": sc_ends, "same_range_both_strands": sc_same_range_both_strands,
             "overlap": sc_overlap, "invalid_bases": sc_invalid_bases, "many_blocks": sc_many_blocks, "three_sequences": sc_three_sequences,
             "no_blocks": sc_no_blocks}
MIN_VALUES = {"short": 1, "window_counts": 4 * P, "ends": 100, "same_range_both_strands": 100, "overlap": 100, "invalid_bases": P, "many_blocks": 100_000,
              "three_sequences": 500, "no_blocks": 0}


@pytest.mark.parametrize("syncmer", [0, 1], ids=["dense", "syncmer"])
@pytest.mark.parametrize("name", list(SCENARIOS))
def test_extract_blocks_against_oracle(ctx, orc, name, syncmer):
    import metabuli_amd as M
    bases, offs, blocks = SCENARIOS[name](np.random.default_rng(sum(map(ord, name))))
    ev, eb = blocks_spec.oracle_blocks(orc, syncmer, bases, offs, blocks)
    assert len(ev) >= (MIN_VALUES[name] if not syncmer else MIN_VALUES[name] // 4)
    gv, gb = ctx.extract_blocks(M.default_params(seq_mode=3, syncmer=syncmer), bases, offs, blocks)
    assert len(gv) == len(ev)
    assert (gb == eb).all()
    assert (gv == ev).all()
    gv2, none = ctx.extract_blocks(M.default_params(seq_mode=3, syncmer=syncmer), bases, offs, blocks, want_block_of=False)
    assert none is None and (gv2 == ev).all()
    if name == "same_range_both_strands":
        assert set(gv[gb == 0].tolist()) != set(gv[gb == 1].tolist())
    if name == "overlap" and not syncmer:
        assert len(np.unique(gv)) < len(gv)                             # duplicates are kept
    if name == "short":
        assert set(gb.tolist()) <= {6, 7, 8, 9, 10, 11}                 # only the blocks of 24 bases and more


def _raw_extract(ctx, p, bases, offs, blocks, values, block_of, cap):
    cnt = C.c_uint64(12345)
    st = ctx.L.mtb_extract_blocks(ctx.h, C.byref(p), bases.ctypes.data_as(C.c_void_p), offs.ctypes.data_as(C.c_void_p), C.c_uint64(len(offs) - 1),
                                  blocks.ctypes.data_as(C.c_void_p), C.c_uint64(len(blocks)), values.ctypes.data_as(C.c_void_p),
                                  None if block_of is None else block_of.ctypes.data_as(C.c_void_p), C.c_uint64(cap), C.byref(cnt))
    return st, cnt.value


def test_capacity_too_small_returns_the_required_size(ctx, orc):
    import metabuli_amd as M
    bases, offs, blocks = sc_three_sequences(np.random.default_rng(1))
    ev, eb = blocks_spec.oracle_blocks(orc, 0, bases, offs, blocks)
    p = M.default_params(seq_mode=3, syncmer=0)
    GUARD, GUARD32 = np.uint64(0xA5A5A5A5DEADBEEF), np.uint32(0xDEADBEEF)
    for cap in (0, 7, len(ev) - 1):
        v = np.full(len(ev) + 8, GUARD, np.uint64); bo = np.full(len(ev) + 8, GUARD32, np.uint32)
        st, n = _raw_extract(ctx, p, bases, offs, blocks, v, bo, cap)
        assert st == M.MTB_ERR_CAPACITY and n == len(ev)
        assert (v[cap:] == GUARD).all() and (bo[cap:] == GUARD32).all()                      # nothing past cap
    v = np.full(len(ev) + 8, GUARD, np.uint64); bo = np.full(len(ev) + 8, GUARD32, np.uint32)
    st, n = _raw_extract(ctx, p, bases, offs, blocks, v, bo, len(ev))
    assert st == M.MTB_OK and n == len(ev) and (v[:n] == ev).all() and (bo[:n] == eb).all()
    assert (v[n:] == GUARD).all() and (bo[n:] == GUARD32).all()


@pytest.fixture(scope="module")
def three_taxa(tmp_path_factory):
    from metabuli_amd import synth
    tax = synth.Taxonomy()
    tax.add(1, 1, "no rank", "root"); tax.add(2, 1, "superkingdom", "Bacteria"); tax.add(10, 2, "genus", "G")
    tax.add(11, 10, "species", "G a"); tax.add(12, 10, "species", "G b")
    tax.add(21, 11, "no rank", "a1"); tax.add(22, 11, "no rank", "a2"); tax.add(23, 12, "no rank", "b1")
    d = str(tmp_path_factory.mktemp("three_taxa"))
    tax.write(d)
    return d


BAD_BLOCKS = {
    "seq_out_of_range": ((3, 1, 0, 50), "block 2"),
    "end_before_start": ((0, 1, 40, 39), "block 2"),                # also the only way to spell a block of 0 bases
    "end_beyond_sequence": ((2, -1, 300, 333), "block 2"),
}


@pytest.mark.parametrize("case", list(BAD_BLOCKS))
def test_argument_errors(ctx, three_taxa, case):
    import metabuli_amd as M
    bases, offs, blocks = sc_three_sequences(np.random.default_rng(1))
    bad = blocks.copy()
    bad[2] = BAD_BLOCKS[case][0]
    p = M.default_params(seq_mode=3, syncmer=1)
    with pytest.raises(M.MtbError) as e:
        ctx.extract_blocks(p, bases, offs, bad)
    assert e.value.status == M.MTB_ERR_ARG and BAD_BLOCKS[case][1] in str(e.value)
    b = ctx.builder(three_taxa, p)
    b.add_blocks(bases, offs, [21, 22, 23], blocks[:2])
    held = b.num_records
    assert held > 0
    with pytest.raises(M.MtbError) as e:
        b.add_blocks(bases, offs, [21, 22, 23], bad)
    assert e.value.status == M.MTB_ERR_ARG and BAD_BLOCKS[case][1] in str(e.value)
    assert b.num_records == held
    b.close()


def test_unknown_taxid_and_old_format_are_refused(ctx, three_taxa):
    import metabuli_amd as M
    bases, offs, blocks = sc_three_sequences(np.random.default_rng(1))
    p = M.default_params(seq_mode=3, syncmer=1)
    b = ctx.builder(three_taxa, p)
    b.add_blocks(bases, offs, [21, 22, 23], blocks[:2])
    held = b.num_records
    with pytest.raises(M.MtbError) as e:
        b.add_blocks(bases, offs, [21, 424242, 23], blocks)
    assert e.value.status == M.MTB_ERR_ARG and "424242" in str(e.value) and b.num_records == held
    b.close()
    p1 = M.default_params(seq_mode=3, syncmer=0, kmer_format=1)
    with pytest.raises(M.MtbError) as e:
        ctx.extract_blocks(p1, bases, offs, blocks)
    assert e.value.status == M.MTB_ERR_UNSUPPORTED
    b1 = ctx.builder(three_taxa, p1)
    with pytest.raises(M.MtbError) as e:
        b1.add_blocks(bases, offs, [21, 22, 23], blocks)
    assert e.value.status == M.MTB_ERR_UNSUPPORTED and b1.num_records == 0
    b1.close()


@pytest.mark.parametrize("syncmer", [0, 1], ids=["dense", "syncmer"])
def test_builder_records_carry_the_taxid_of_the_blocks_sequence(ctx, orc, three_taxa, syncmer):
    """blocks in three sequences with three taxids, added in two calls behind records the builder already holds: finish() = the spec's
    sort + per-species LCA dedup of the oracle's (value, taxid of the block's sequence) records"""
    import metabuli_amd as M
    from build_spec import spec_finish
    bases, offs, blocks = sc_three_sequences(np.random.default_rng(1))
    taxids = np.array([21, 22, 23], np.int32)
    ev, eb = blocks_spec.oracle_blocks(orc, syncmer, bases, offs, blocks)
    et = taxids[blocks["seq"][eb]]
    b = ctx.builder(three_taxa, M.default_params(seq_mode=1, syncmer=syncmer))
    b.add_records(ev[:5], et[:5])
    b.add_blocks(bases, offs, taxids, blocks[:4])
    b.add_blocks(bases, offs, taxids, make_blocks([]))
    b.add_blocks(bases, offs, taxids, blocks[4:])
    assert b.num_records == len(ev) + 5
    ix = b.finish()
    sv, si, _ = spec_finish(np.concatenate([ev[:5], ev]), np.concatenate([et[:5], et]), three_taxa)
    gv, gi = ix.download()
    assert len(gv) == len(sv) and (gv == sv).all() and (gi == si).all()
    assert len(set(gi.tolist())) >= 3
    ix.close(); b.close()
