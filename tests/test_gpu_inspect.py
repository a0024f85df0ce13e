"""GPU tests of the database inspection (mtb_database_inspect, mtb_inspect_records, mtb_inspect_write_report; kernels_inspect.h):
every bin, counter and histogram slot equal to tests/inspect_spec.py.  The stage call runs lists built here -- group edges on every
lane, wave, tile and pass boundary -- through the device code of the directory call in passes of a few thousand entries; then a
~20 000-entry database written through the oracle, and mtb_build."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import audit_spec as A
import inspect_spec as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = 4096                                   # words per forced chunk of the directory call
PASS = 2500                                    # entries per pass of the stage call: tiles of 1024, 1024 and 452 entries
UNKNOWN = 4000                                 # an id the toy taxonomy does not have
ALIAS = 900                                    # merged.dmp: 900 -> the first strain


@pytest.fixture(scope="module")
def ctx():
    import metabuli_amd as M
    c = M.Context(0)
    yield c
    c.close()


class World:
    """root -> {Bacteria, Eukaryota} -> three genera (the last one under Eukaryota) -> three species each -> two strains each, one
    alias in merged.dmp; as dump files and as the spec's tables"""

    def __init__(self, d, far=()):
        from metabuli_amd import synth
        self.w = w = synth.make_world(seed=21, n_genera=3, species_per_genus=3, strains_per_species=2, genome_len=3000)
        for t, par, rank in far:
            w.tax.add(t, par, rank, f"far {t}")
        self.taxdir = os.path.join(str(d), "taxonomy")
        w.tax.write(self.taxdir)
        self.strains = sorted(t for t in w.tax.parent if w.tax.rank[t] == "no rank" and t != 1)
        self.by_species = {}
        for t in self.strains:
            self.by_species.setdefault(w.tax.parent[t], []).append(t)
        self.species = sorted(self.by_species)
        with open(os.path.join(self.taxdir, "merged.dmp"), "w") as f:
            f.write(f"{ALIAS}\t|\t{self.strains[0]}\t|\n")
        self.tax = S.Tax(w.tax.parent, w.tax.rank, w.tax.name, aliases={ALIAS: self.strains[0]})
        assert UNKNOWN not in w.tax.parent and self.tax.max_id == max(max(w.tax.parent), ALIAS)


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    return World(tmp_path_factory.mktemp("inspect_world"))


@pytest.fixture(scope="module")
def tile():
    import metabuli_amd as M
    t = M.inspect_tile_entries()
    assert t == 1024 and PASS % 4 == 0 and 2 * t < PASS < 3 * t                          # the cases below place their groups by these
    return t


def _check(ctx, world, values, info, level, per_pass=PASS, mask=0xFFFFFFFF):
    """the stage call against the spec: every field but the times and n_chunks, every histogram slot, every bin"""
    want, wd, we = S.inspect(values, info, world.tax, level, mask)
    rep, d, e = ctx.inspect_records(values, info, taxonomy_dir=world.taxdir, level=level, info_mask=mask, entries_per_pass=per_pass)
    got = {k: rep[k] for k in S.REPORT_FIELDS}
    assert got == {k: want[k] for k in S.REPORT_FIELDS}, {k: (got[k], want[k]) for k in got if got[k] != want[k]}
    assert rep["size_hist"] == want["size_hist"]
    assert d.dtype == np.uint64 and len(d) == len(wd) == rep["n_taxa"] and (d == wd).all(), np.flatnonzero(d != wd)[:8]
    assert len(e) == len(we) and (e == we).all(), np.flatnonzero(e != we)[:8]
    if per_pass:
        assert rep["n_chunks"] == (len(values) + per_pass - 1) // per_pass
    return rep


def _both(ctx, world, values, info, level, mask=0xFFFFFFFF):
    """in passes of PASS entries and in one pass: the same report except n_chunks and the times"""
    a = _check(ctx, world, values, info, level, PASS, mask)
    b = _check(ctx, world, values, info, level, 0, mask)
    assert {k: v for k, v in a.items() if k != "n_chunks" and not k.startswith("ms_")} == {k: v for k, v in b.items() if k != "n_chunks" and not k.startswith("ms_")}
    assert b["n_chunks"] == (1 if len(values) else 0)
    return a


def _layout(n, groups):
    """sizes of consecutive groups covering [0, n): the given (start, size) groups, groups of one everywhere else"""
    sizes, at = [], 0
    for start, size in sorted(groups):
        assert start >= at and start + size <= n, (start, size, at, n)
        sizes += [1] * (start - at) + [size]
        at = start + size
    return np.array(sizes + [1] * (n - at), np.int64)


def _entries(world, sizes, level, rng, ids=None):
    """values and ids of groups of the given sizes.  Level 0: the members of a group share the value; level 1: they share the
    amino-acid part and count up in the DNA part.  ids: per entry, default a random strain"""
    sizes = np.asarray(sizes, np.int64)
    n = int(sizes.sum())
    group = np.repeat(np.arange(len(sizes)), sizes)
    member = np.arange(n) - np.repeat(np.cumsum(sizes) - sizes, sizes)
    assert level == 0 or int(sizes.max(initial=0)) <= 1 << 24
    values = ((group.astype(np.uint64) + np.uint64(1)) << np.uint64(24)) | (member.astype(np.uint64) if level else np.uint64(5))
    info = rng.choice(world.strains, size=n).astype(np.uint32) if ids is None else np.asarray(ids, np.uint32)
    return values, info


def _edges(kind, tile, n):
    """entry indices (> 16, < n - 16) of the edges of one kind, for passes of PASS entries"""
    if kind == "lane":
        e = [x for x in range(20, n - 16, 44) if x % 256]
    elif kind == "wave":
        e = [p + x for p in range(0, n, PASS) for x in range(256, PASS, 256) if x % tile]
    elif kind == "tile":
        e = [p + x for p in range(0, n, PASS) for x in range(tile, PASS, tile)]
    else:
        e = list(range(PASS, n, PASS))
    return [x for x in e if 16 < x < n - 16]


# ---------------------------------------------------------------------------------------------------------------------
# the stage call: group edges
# ---------------------------------------------------------------------------------------------------------------------
def test_groups_of_one(ctx, world, tile):
    rng = np.random.default_rng(1)
    for level in (0, 1):
        v, t = _entries(world, np.ones(3 * PASS + 77, np.int64), level, rng)
        rep = _both(ctx, world, v, t, level)
        assert rep["n_groups"] == len(v) and rep["max_group"] == 1 and rep["first_max_group"] == 0


@pytest.mark.parametrize("level", [0, 1])
@pytest.mark.parametrize("kind", ["lane", "wave", "tile", "pass"])
def test_groups_on_every_edge(ctx, world, tile, kind, level):
    """sizes 2..9: one group that ends exactly at an edge with one that starts exactly there, and one that straddles the next edge"""
    n = {"lane": 2 * PASS, "wave": 2 * PASS + 600, "tile": 8 * PASS + 100, "pass": 16 * PASS + 40}[kind]
    edges = _edges(kind, tile, n)
    assert len(edges) >= 16
    groups = []
    for k, size in enumerate(range(2, 10)):
        a, b = edges[2 * k], edges[2 * k + 1]
        groups += [(a - size, size), (a, size), (b - size // 2, size)]
    sizes = _layout(n, groups)
    v, t = _entries(world, sizes, level, np.random.default_rng(2))
    starts = np.cumsum(sizes) - sizes
    for k, size in enumerate(range(2, 10)):                                              # what the case is about
        a, b = edges[2 * k], edges[2 * k + 1]
        assert a in starts and a - size in starts and sizes[list(starts).index(a)] == size and b - size // 2 in starts
    rep = _both(ctx, world, v, t, level)
    assert rep["max_group"] == 9 and rep["n_groups"] == len(sizes)


@pytest.mark.parametrize("level", [0, 1])
def test_first_and_last_entry(ctx, world, tile, level):
    rng = np.random.default_rng(3)
    n = 2 * PASS + 10
    for first, last in ((1, 1), (5, 7), (1, 6), (4, 1)):
        sizes = _layout(n, [(0, first), (n - last, last)])
        v, t = _entries(world, sizes, level, rng)
        _both(ctx, world, v, t, level)


def test_long_groups_at_level_1(ctx, world, tile):
    """longer than a tile and shorter than a pass, longer than a pass, longer than three passes, one that fills a tile exactly"""
    rng = np.random.default_rng(4)
    n = 9 * PASS
    groups = [(300, tile + 700), (PASS + tile, tile), (2 * PASS - 40, PASS + 300), (4 * PASS + 123, 3 * PASS + 500)]
    assert tile < groups[0][1] < PASS and groups[1][0] % PASS == tile and groups[2][1] > PASS and groups[3][1] > 3 * PASS
    sizes = _layout(n, groups)
    v, t = _entries(world, sizes, 1, rng)
    rep = _both(ctx, world, v, t, 1)
    assert rep["max_group"] == 3 * PASS + 500 and rep["first_max_group"] == 4 * PASS + 123
    assert rep["size_hist"][10] == 2 and rep["size_hist"][11] == 1 and rep["size_hist"][12] == 1
    # the long groups inside one species each: the fold must not leave it
    ids = rng.choice(world.strains, size=n).astype(np.uint32)
    for (start, size), sp in zip(groups, world.species):
        ids[start:start + size] = rng.choice(world.by_species[sp], size=size)
    _both(ctx, world, v, ids, 1)


def test_a_list_that_is_one_group(ctx, world, tile):
    rng = np.random.default_rng(5)
    for n in (2 * PASS + 300, tile, 7):
        v, t = _entries(world, [n], 1, rng)
        rep = _both(ctx, world, v, t, 1)
        assert rep["n_groups"] == 1 and rep["max_group"] == n and rep["first_max_group"] == 0 and sum(rep["size_hist"]) == 1


@pytest.mark.parametrize("level", [0, 1])
def test_small_and_boundary_lengths(ctx, world, tile, level):
    rng = np.random.default_rng(6)
    for n in (0, 1, 3, tile - 1, tile, tile + 1, PASS - 1, PASS, PASS + 1):
        sizes = rng.integers(1, 4, size=n)
        sizes = sizes[np.cumsum(sizes) <= n]
        sizes = np.concatenate([sizes, np.ones(n - int(sizes.sum()), np.int64)])
        v, t = _entries(world, sizes, level, rng)
        assert len(v) == n
        rep = _both(ctx, world, v, t, level)
        assert rep["n_entries"] == n
        if n == 0:
            assert rep["first_max_group"] == S.NONE and rep["n_groups"] == 0


# ---------------------------------------------------------------------------------------------------------------------
# the stage call: nothing is sorted or validated -- a key that comes back begins a new group
# ---------------------------------------------------------------------------------------------------------------------
def _with_key(values, level, spans, aa):
    """`values` with the entries of every [a, b) in `spans` given the amino-acid part `aa` (level 0: one value; level 1: DNA parts that count up)"""
    v = values.copy()
    for a, b in spans:
        v[a:b] = (np.uint64(aa) << np.uint64(24)) | (np.arange(b - a).astype(np.uint64) if level else np.uint64(5))
    return v


@pytest.mark.parametrize("level", [0, 1])
def test_a_key_that_comes_back_is_a_new_group(ctx, world, tile, level):
    """A.., B.., A..: the same key at both ends of a tile, of a pass and of the list, in runs that lie inside a tile and that cross
    tile and pass edges, with one other entry or a thousand between them; then a list in descending and one in shuffled order"""
    rng = np.random.default_rng(12)
    n = 3 * PASS + 200
    base, t = _entries(world, np.ones(n, np.int64), level, rng)
    KEY = 1 << 30                                                                        # beyond every key of `base`
    cases = {
        "ends of a tile": [(0, 10), (tile - 14, tile)],
        "ends of a tile of the second pass": [(PASS, PASS + 10), (PASS + tile - 14, PASS + tile)],
        "ends of a pass": [(0, 10), (PASS - 14, PASS)],
        "ends of the list": [(0, 3), (n - 5, n)],
        "runs across tile edges": [(tile - 6, tile + 9), (2 * tile - 3, 2 * tile + 4)],
        "runs across pass edges": [(PASS - 6, PASS + 9), (2 * PASS - 3, 2 * PASS + 4), (3 * PASS - 1, 3 * PASS + 1)],
        "one entry between": [(100, 104), (105, 109), (tile - 2, tile), (tile + 1, tile + 3), (PASS - 2, PASS), (PASS + 1, PASS + 3)],
        "whole tiles": [(0, tile), (tile + 1, 2 * tile), (PASS, PASS + tile), (PASS + tile + 5, PASS + 2 * tile)],
    }
    for name, spans in cases.items():
        v = _with_key(base, level, spans, KEY)
        want, _, _ = S.inspect(v, t, world.tax, level)
        assert want["n_groups"] == n - sum(b - a for a, b in spans) + len(spans), name   # every span is a group of its own
        _both(ctx, world, v, t, level)
    sizes = rng.integers(1, 6, size=n)
    sizes = sizes[np.cumsum(sizes) <= n]
    v, t = _entries(world, sizes, level, rng)
    _both(ctx, world, v[::-1].copy(), t[::-1].copy(), level)                             # descending
    pieces = np.split(np.arange(len(v)), np.sort(rng.choice(np.arange(1, len(v)), size=300, replace=False)))
    order = np.concatenate([pieces[k] for k in rng.permutation(len(pieces))])
    _both(ctx, world, v[order], t[order], level)                                         # pieces of the list in shuffled order
    few = np.repeat(rng.integers(1, 4, size=len(sizes)), sizes).astype(np.uint64)        # three amino-acid parts only: equal keys meet by chance
    _both(ctx, world, (few << np.uint64(24)) | (v & np.uint64(0xFFFFFF)), t, level)


# ---------------------------------------------------------------------------------------------------------------------
# the stage call: ids
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", [0, 1])
def test_unknown_ids(ctx, world, tile, level):
    """alone in a group; first, middle and last member; in a group across a pass edge; an orphan group across a tile edge; the alias"""
    rng = np.random.default_rng(7)
    n = 3 * PASS
    groups = [(40, 1), (100, 5), (200, 5), (300, 5), (PASS - 3, 7), (tile - 2, 5), (PASS + tile - 1, 3), (2 * PASS - 1, 2), (2 * PASS + 50, 4)]
    sizes = _layout(n, groups)
    v, t = _entries(world, sizes, level, rng)
    t[40] = UNKNOWN
    t[100] = UNKNOWN; t[202] = UNKNOWN; t[304] = UNKNOWN
    t[PASS - 1] = UNKNOWN; t[PASS] = UNKNOWN + 1
    t[tile - 2:tile + 3] = UNKNOWN                                                       # orphan across the first tile edge
    t[PASS + tile - 1:PASS + tile + 2] = UNKNOWN + 2                                     # ... and across a tile edge of the second pass
    t[2 * PASS - 1:2 * PASS + 1] = UNKNOWN                                               # ... and across a pass edge
    t[2 * PASS + 50] = ALIAS; t[2 * PASS + 51] = world.strains[1]
    rep = _both(ctx, world, v, t, level)
    assert rep["n_orphan_groups"] == 4 and rep["n_orphan_entries"] == 1 + 5 + 3 + 2


def test_bit_31_with_and_without_the_legacy_mask(ctx, world, tile):
    rng = np.random.default_rng(8)
    sizes = rng.integers(1, 5, size=2200)
    v, t = _entries(world, sizes, 0, rng)
    t[::3] |= np.uint32(1 << 31)
    a = _both(ctx, world, v, t, 0, mask=0x7FFFFFFF)
    assert a["n_orphan_groups"] == 0
    b = _both(ctx, world, v, t, 0)                                                       # bit 31 kept: those ids are unknown
    assert b["n_orphan_groups"] > 0


def test_large_sparse_taxonomy(ctx, tile, tmp_path):
    """ids beyond 10^5: bins and replicas beyond one page"""
    far = [(150001, 2, "genus"), (150777, 150001, "species"), (1203456, 150777, "no rank"), (1203457, 150777, "no rank"), (987654, 150001, "species"), (1000001, 987654, "no rank")]
    wd = World(tmp_path, far=far)
    rng = np.random.default_rng(9)
    n = 2 * PASS + 500
    for level in (0, 1):
        sizes = rng.integers(1, 6, size=n)
        sizes = sizes[np.cumsum(sizes) <= n]
        ids = rng.choice(wd.strains + [1203456, 1203457, 1000001], size=int(sizes.sum())).astype(np.uint32)
        ids[rng.random(len(ids)) < 0.5] = rng.choice([1203456, 1203457, 1000001])
        v, t = _entries(wd, sizes, level, rng, ids=ids)
        rep = _check(ctx, wd, v, t, level)
        assert rep["n_taxa"] == 1203458


# ---------------------------------------------------------------------------------------------------------------------
# skew: the hot-bin and the no-fold paths of the weighted add
# ---------------------------------------------------------------------------------------------------------------------
def test_most_groups_meet_at_the_root(ctx, world, tile):
    rng = np.random.default_rng(10)
    sizes = rng.integers(2, 7, size=8000)
    sizes = sizes[np.cumsum(sizes) <= 20000]
    sizes = np.concatenate([sizes, np.ones(20000 - int(sizes.sum()), np.int64)])
    bact = [t for t in world.strains if 2 in world.tax.lineage(t)]
    euk = [t for t in world.strains if 3 in world.tax.lineage(t)]
    ids = rng.choice(world.strains, size=20000).astype(np.uint32)
    starts = np.cumsum(sizes) - sizes
    for s, z in zip(starts, sizes):
        if z >= 2 and rng.random() < 0.85:                                               # one member of each domain
            ids[s] = rng.choice(bact); ids[s + 1] = rng.choice(euk)
    v, t = _entries(world, sizes, 1, rng, ids=ids)
    want, wd, _ = S.inspect(v, t, world.tax, 1)
    assert wd[1] > 0.6 * want["n_groups"]
    _check(ctx, world, v, t, 1)


def test_every_group_stays_inside_its_species(ctx, world, tile):
    rng = np.random.default_rng(11)
    sizes = rng.integers(1, 7, size=8000)
    sizes = sizes[np.cumsum(sizes) <= 20000]
    sizes = np.concatenate([sizes, np.ones(20000 - int(sizes.sum()), np.int64)])
    sp = np.repeat(rng.choice(world.species, size=len(sizes)), sizes)
    ids = np.array([world.by_species[int(s)][int(k)] for s, k in zip(sp, rng.integers(0, 2, size=20000))], np.uint32)
    v, t = _entries(world, sizes, 1, rng, ids=ids)
    want, wd, _ = S.inspect(v, t, world.tax, 1)
    assert not wd[[1, 2, 3]].any() and all(wd[g] == 0 for g in set(world.tax.parent[s] for s in world.species))
    _check(ctx, world, v, t, 1)


# ---------------------------------------------------------------------------------------------------------------------
# the directory call
# ---------------------------------------------------------------------------------------------------------------------
DB_FILES = ("diffIdx", "info", "split", "taxID_list", "db.parameters")


class Base:
    """~20 000 entries in (value, species) order as the oracle writes them: ~18 000 values, one to five per amino-acid part, every
    eighth value filed under two or three species"""

    def __init__(self, orc, world, d):
        from helpers import default_params
        self.world = world
        self.p = default_params(seq_mode=1, syncmer=1)
        rng = np.random.default_rng(5)
        letters = rng.integers(0, 21, size=(6000, 8)).astype(np.uint64)                  # eight amino-acid letters 0..20 above 24 DNA bits
        aa = np.zeros(6000, np.uint64)
        for k in range(8):
            aa |= letters[:, k] << np.uint64(5 * k)
        aa = np.unique(aa[aa > 0])
        aa = np.repeat(aa, rng.integers(1, 6, size=len(aa)))                             # one to five values per amino-acid part
        vals = np.unique((aa << np.uint64(24)) | rng.integers(0, 1 << 24, size=len(aa)).astype(np.uint64))
        sp = rng.choice(world.species, size=len(vals)).astype(np.int64)
        shared = np.flatnonzero(np.arange(len(vals)) % 8 == 0)
        extra_v, extra_s = [], []
        for k in shared:
            others = [s for s in world.species if s != sp[k]]
            for s in rng.choice(others, size=int(rng.integers(1, 3)), replace=False):
                extra_v.append(vals[k]); extra_s.append(int(s))
        vals = np.concatenate([vals, np.array(extra_v, np.uint64)]); sp = np.concatenate([sp, np.array(extra_s, np.int64)])
        order = np.lexsort((sp, vals))
        self.values, sp = vals[order], sp[order]
        self.taxids = np.array([world.by_species[int(s)][int(k)] for s, k in zip(sp, rng.integers(0, 2, size=len(sp)))], np.int32)
        self.n = len(self.values)
        self.dir = str(d)
        shutil.copytree(world.taxdir, os.path.join(self.dir, "taxonomy"))
        orc.write_db(self.dir, self.values, self.taxids, self.p, split_num=12)
        self.files = {f: open(os.path.join(self.dir, f), "rb").read() for f in DB_FILES}
        assert 19000 <= self.n <= 23000


@pytest.fixture(scope="module")
def base(orc, world, tmp_path_factory):
    return Base(orc, world, tmp_path_factory.mktemp("inspect_base"))


def _decoded(d):
    """(values, info) of a database directory's files, by the audit spec's coder"""
    values, _ = A.decode_words(np.frombuffer(open(os.path.join(d, "diffIdx"), "rb").read(), np.uint16))
    info = np.frombuffer(open(os.path.join(d, "info"), "rb").read(), np.uint32)
    n = min(len(values), len(info))
    return values[:n], info[:n]


@pytest.mark.parametrize("level", ["dna", "aa"])
@pytest.mark.parametrize("chunk_words", [CHUNK, 0])
def test_directory_call(ctx, world, base, level, chunk_words):
    lv = {"dna": 0, "aa": 1}[level]
    values, info = _decoded(base.dir)
    assert len(values) == base.n and (values == base.values).all()
    want, wd, we = S.inspect(values, info, world.tax, lv)
    rep, d, e = ctx.inspect_database(base.dir, level=level, chunk_words=chunk_words)
    assert {k: rep[k] for k in S.REPORT_FIELDS} == {k: want[k] for k in S.REPORT_FIELDS} and rep["size_hist"] == want["size_hist"]
    assert (d == wd).all() and (e == we).all() and len(d) == world.tax.max_id + 1
    assert rep["n_chunks"] >= 8 if chunk_words else rep["n_chunks"] == 1
    srep, sd, se = ctx.inspect_records(values, info, taxonomy_dir=world.taxdir, level=lv, entries_per_pass=PASS)
    assert {k: srep[k] for k in S.REPORT_FIELDS} == {k: rep[k] for k in S.REPORT_FIELDS} and srep["size_hist"] == rep["size_hist"]
    assert (sd == d).all() and (se == e).all()
    if lv == 1:
        assert rep["max_group"] >= 4 and wd[1] > 0                                       # runs of values, and groups that meet at the root


def test_report_writer(ctx, world, base, tmp_path):
    import metabuli_amd as M
    rep, d, e = ctx.inspect_database(base.dir, level="aa", chunk_words=CHUNK)
    path = str(tmp_path / "r.tsv")
    text = M.write_inspect_report(d, e, rep["n_groups"], tsv_path=path, dbdir=base.dir)
    assert open(path).read() == S.report_text(world.tax, d, e) and text == S.summary_text(world.tax, d, e, rep["n_groups"])
    assert M.write_inspect_report(d, e, rep["n_groups"], taxonomy_dir=world.taxdir) == text


# ---------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------
def _status(ctx, d, cap=None, level=0):
    import ctypes as C
    import metabuli_amd as M
    r = M.InspectReport()
    p = M.default_params()
    a = np.full(max(cap or 1, 1), 0xABCD, np.uint64); b = a.copy()
    st = ctx.L.mtb_database_inspect(ctx.h, d.encode(), None, C.byref(p), C.c_uint64(CHUNK), C.c_int(level), a.ctypes.data_as(C.c_void_p) if cap is not None else None,
                                    b.ctypes.data_as(C.c_void_p) if cap is not None else None, C.c_uint64(cap or 0), C.byref(r))
    return st, ctx.L.mtb_last_error().decode(), a, b, r


def _copy(base, d, **edits):
    d = str(d)
    os.makedirs(d, exist_ok=True)
    shutil.copytree(os.path.join(base.dir, "taxonomy"), os.path.join(d, "taxonomy"), dirs_exist_ok=True)
    for f in DB_FILES:
        data = edits.get(f.replace(".", "_"), base.files[f])
        if data is not None:
            open(os.path.join(d, f), "wb").write(data)
    return d


def test_cap_too_small(ctx, world, base):
    import metabuli_amd as M
    need = world.tax.max_id + 1
    st, msg, a, b, r = _status(ctx, base.dir, cap=need - 1)
    assert st == M.MTB_ERR_CAPACITY and str(need) in msg and r.n_taxa == need and (a == 0xABCD).all() and (b == 0xABCD).all()
    st, _, a, _, _ = _status(ctx, base.dir, cap=need)
    assert st == M.MTB_OK and not (a == 0xABCD).any()


@pytest.mark.parametrize("f,needle", [("diffIdx", "\"diffIdx\" file is missing"), ("info", "\"info\" file is missing"), ("split", "\"split\" file is missing")])
def test_a_missing_file(ctx, base, tmp_path, f, needle):
    import metabuli_amd as M
    st, msg, *_ = _status(ctx, _copy(base, tmp_path / "db", **{f: None}))
    assert st == M.MTB_ERR_IO and needle in msg, msg


def test_reduced_alphabet_is_refused(ctx, base, tmp_path):
    import metabuli_amd as M
    par = base.files["db.parameters"].replace(b"Reduced_alphabet\t0", b"Reduced_alphabet\t1")
    assert par != base.files["db.parameters"]
    st, msg, *_ = _status(ctx, _copy(base, tmp_path / "db", db_parameters=par))
    assert st == M.MTB_ERR_UNSUPPORTED and "Reduced_alphabet" in msg


def test_a_bad_level(ctx, world, base):
    import metabuli_amd as M
    for level in (2, -1):
        st, msg, *_ = _status(ctx, base.dir, level=level)
        assert st == M.MTB_ERR_ARG and "level" in msg
    with pytest.raises(M.MtbError) as err:
        ctx.inspect_records(np.zeros(4, np.uint64), np.zeros(4, np.uint32), taxonomy_dir=world.taxdir, level=3)
    assert err.value.status == M.MTB_ERR_ARG


# ---------------------------------------------------------------------------------------------------------------------
# the program
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mtb_build(tmp_path_factory):
    """mtb_build next to the library under test; against the emulated library it is compiled here"""
    import metabuli_amd as M
    tmp = tmp_path_factory.mktemp("inspect_mtb_build")
    d = os.path.dirname(M.LIB_PATH)
    if os.environ.get("MTB_HIPEMU"):
        exe = os.path.join(str(tmp), "mtb_build")
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-pthread", "-o", exe, os.path.join(ROOT, "metabuli_amd", "csrc", "host", "build_main.cpp"),
                               "-L" + d, "-lmtb", "-lz", "-Wl,-rpath," + d])
        return exe
    subprocess.check_call(["make", "-C", d, "mtb_build"], stdout=subprocess.DEVNULL)
    return os.path.join(d, "mtb_build")


def _summary_of(stdout, level):
    """the by-rank summary printed for one level: from its first line up to the `Inspected` line"""
    part = stdout.split(f"({'aa' if level else 'dna'} level)\n", 1)[1]
    return part.split("Inspected (", 1)[0]


def test_mtb_build_inspect_both_levels(world, base, tmp_path, mtb_build):
    exe = mtb_build
    d = _copy(base, tmp_path / "db")
    r = subprocess.run([exe, "--inspect", "1", "--inspect-level", "both", "--audit", "1", "-", "-", os.path.join(d, "taxonomy"), d], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "valid 1, canonical 1" in r.stdout                                            # the audit of the same invocation
    values, info = _decoded(d)
    for level in (0, 1):
        want, wd, we = S.inspect(values, info, world.tax, level)
        assert open(os.path.join(d, S.TSV_NAME[level])).read() == S.report_text(world.tax, wd, we)
        assert _summary_of(r.stdout, level) == S.summary_text(world.tax, wd, we, want["n_groups"])
        assert f"{want['n_groups']} groups" in r.stdout and f"largest group {want['max_group']} at entry {want['first_max_group']}" in r.stdout
    r = subprocess.run([exe, "--inspect", "1", "-", "-", os.path.join(d, "taxonomy"), _copy(base, tmp_path / "db2")], capture_output=True, text=True)
    assert r.returncode == 0 and os.path.exists(tmp_path / "db2" / S.TSV_NAME[0]) and not os.path.exists(tmp_path / "db2" / S.TSV_NAME[1])


def test_mtb_build_inspect_behind_a_filtered_merge(world, base, tmp_path, mtb_build):
    exe = mtb_build
    gone = world.w.tax.parent[world.species[0]]                                          # a genus
    out = str(tmp_path / "merged")
    r = subprocess.run([exe, "--inspect", "1", "--inspect-level", "aa", "--syncmer", "1", "--split-num", "12", "--add-db", base.dir, "--exclude-taxid", str(gone),
                        "-", "-", world.taxdir, out], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    values, info = _decoded(out)
    assert 0 < len(values) < base.n
    want, wd, we = S.inspect(values, info, world.tax, 1)
    text = open(os.path.join(out, S.TSV_NAME[1])).read()
    assert text == S.report_text(world.tax, wd, we)
    under = {t for t in world.tax.parent if gone in world.tax.lineage(t)}
    assert under and not any(int(row.split("\t")[0]) in under for row in text.splitlines()[1:])
    assert _summary_of(r.stdout, 1) == S.summary_text(world.tax, wd, we, want["n_groups"])


@pytest.mark.parametrize("flags", [["--inspect", "2"], ["--inspect", "yes"], ["--inspect", "1", "--inspect-level", "protein"]])
def test_mtb_build_refuses_bad_flag_values(base, mtb_build, flags):
    exe = mtb_build
    r = subprocess.run([exe] + flags + ["--device", "99", "-", "-", os.path.join(base.dir, "taxonomy"), base.dir], capture_output=True, text=True)
    assert r.returncode != 0 and flags[0] in r.stderr and "mtb_ctx_create" not in r.stderr   # refused before the (absent) device 99 is opened
    assert not os.path.exists(os.path.join(base.dir, S.TSV_NAME[0]))
