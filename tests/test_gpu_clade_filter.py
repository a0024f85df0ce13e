"""GPU tests of the filtered merge (mtb_merge_databases_filtered, mtb_filter_records; kernels_clade_filter.h, host/clade_filter.h):
the compaction kernels at their tile edges against numpy, subsets byte for byte against a build of only the kept species' records
(builder + add_records + finish + write) and against tests/build_spec.py, independence of the range cut, several / legacy / foreign
inputs, the refusals and statistics against tests/clade_filter_spec.py, the subset as a database (audit, classification), and
`mtb_build --select-taxid / --exclude-taxid`."""
import os
import re
import subprocess

import numpy as np
import pytest

import clade_filter_spec as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL_FILES = ("diffIdx", "info", "split", "taxID_list", "db.parameters")
GROUP_SIZES = (1, 2, 3, 15, 16, 17, 63, 64, 65, 200, 1200)
T = 2048                                                                                 # MTB_CLADE_TILE = MTB_MERGE_TILE


@pytest.fixture(scope="module")
def ctx():
    import metabuli_amd as M
    c = M.Context(0)
    yield c
    c.close()


# ---------------------------------------------------------------------------------------------------------------------
# 1. the kernels at tile edges
# ---------------------------------------------------------------------------------------------------------------------
SIZES = (0, 1, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049, 4097, 5000)
N_KEEP = 1000


def _wanted(pattern, n):
    i = np.arange(n)
    if pattern == "all":
        return np.ones(n, bool)
    if pattern == "none":
        return np.zeros(n, bool)
    if pattern == "alternating":
        return i % 2 == 1
    if pattern == "first":
        return i == 0
    if pattern == "last":
        return i == n - 1
    return (i // 700) % 2 == 0                                                           # kept runs of 700: records 1400 .. 2099 cross record 2048


@pytest.mark.parametrize("pattern", ["all", "none", "alternating", "first", "last", "runs"])
def test_filter_kernels_at_tile_edges(ctx, pattern):
    import metabuli_amd as M
    assert M.MERGE_TILE == T
    rng = np.random.default_rng(2)
    keep = (rng.random(N_KEEP) < 0.5).astype(np.uint8)
    keep[0], keep[N_KEEP - 1] = 1, 0                                                       # both ends of the table are used
    on, off = np.flatnonzero(keep), np.flatnonzero(keep == 0)
    for n in SIZES:
        want = _wanted(pattern, n)
        key = np.where(want, rng.choice(on, size=n), rng.choice(off, size=n)).astype(np.uint64)
        if n:
            key[0] = 0 if want[0] else N_KEEP - 1
        rec = np.zeros(n, M.kmer_dt)
        rec["value"] = rng.integers(0, 1 << 63, size=n, dtype=np.uint64)
        rec["qinfo"] = (key << np.uint64(32)) | rng.integers(0, 1 << 32, size=n, dtype=np.uint64)
        got = ctx.filter_records(rec, keep)
        ref = rec[keep[(rec["qinfo"] >> np.uint64(32)).astype(np.int64)] != 0]
        assert len(ref) == int(want.sum())
        assert len(got) == len(ref), (pattern, n)
        assert (got["value"] == ref["value"]).all() and (got["qinfo"] == ref["qinfo"]).all(), (pattern, n)


def test_filter_refuses_a_key_outside_the_table(ctx):
    import metabuli_amd as M
    keep = np.ones(10, np.uint8)
    for n, at in ((1, 0), (2049, 2048), (5000, 3000)):
        rec = np.zeros(n, M.kmer_dt)
        rec["qinfo"] = np.uint64(3) << np.uint64(32)
        rec["qinfo"][at] = np.uint64(10) << np.uint64(32)                                 # the first key the table lacks
        with pytest.raises(M.MtbError) as e:
            ctx.filter_records(rec, keep)
        assert e.value.status == M.MTB_ERR_ARG and f"record {at} " in str(e.value)
    assert len(ctx.filter_records(np.zeros(5, M.kmer_dt), np.zeros(1, np.uint8))) == 0


# ---------------------------------------------------------------------------------------------------------------------
# the Shapes world (as in tests/test_gpu_merge_stream.py): hand-made records over a toy taxonomy
# ---------------------------------------------------------------------------------------------------------------------
ALIAS = 9000
LOWEST = np.uint64(1)                                                                    # letters 0, DNA part 1
HIGHEST = np.uint64(sum(20 << (24 + 5 * k) for k in range(8)) | 0xFFFFFF)                # letters 20, DNA part all ones


class Shapes:
    """root -> Bacteria -> three genera -> species with 1 .. 1200 strains; merged.dmp: ALIAS -> the first strain of the 3-strain species"""

    def __init__(self, d):
        from metabuli_amd import synth
        tax = synth.Taxonomy()
        tax.add(1, 1, "no rank", "root"); tax.add(2, 1, "superkingdom", "Bacteria")
        nxt = 10
        self.strains, self.genera = {}, []                 # strains per species -> (species id, [strain ids]); genus ids
        for g, counts in enumerate([(1, 2, 3, 15), (16, 17, 63, 64), (65, 200, 600, 1200)]):
            gid = nxt; nxt += 1
            tax.add(gid, 2, "genus", f"G{g}")
            self.genera.append(gid)
            for n in counts:
                sid = nxt; nxt += 1
                tax.add(sid, gid, "species", f"G{g} s{n}")
                ids = list(range(nxt, nxt + n)); nxt += n
                for t in ids:
                    tax.add(t, sid, "no rank", f"strain{t}")
                self.strains[n] = (sid, ids)
        tax.add(nxt, 2, "genus", "G3 without genomes"); self.empty_genus = nxt; nxt += 1
        assert nxt < ALIAS
        self.tax, self.dir = tax, str(d)
        self.aliases = {ALIAS: self.strains[3][1][0]}
        S.write_taxonomy(tax, self.aliases, self.dir)

    def species(self, n):
        return self.strains[n][0]


def _metamers(rng, n):
    """n distinct valid format-2 words (eight amino-acid letters 0..20 above 24 DNA bits), ascending, strictly inside (lowest, highest)"""
    letters = rng.integers(0, 21, size=(int(n * 1.2) + 64, 8)).astype(np.uint64)
    v = rng.integers(0, 1 << 24, size=len(letters)).astype(np.uint64)
    for k in range(8):
        v |= letters[:, k] << np.uint64(24 + 5 * k)
    v = np.unique(v)
    v = v[(v > LOWEST) & (v < HIGHEST)]
    assert len(v) >= n
    return np.sort(rng.choice(v, size=n, replace=False))


def _shape_records(sh):
    """~10 k records (values, taxids): group sizes 1 .. 1200, exact duplicates, values shared by two and three species, merged.dmp alias
    cases, the lowest (65-strain species) and the highest (17-strain species) legal word"""
    rng = np.random.default_rng(42)
    big_sp, big = sh.strains[1200]
    all_strains = np.array([t for _, ids in sh.strains.values() for t in ids], np.int32)
    vals, tids = [], []

    def group(v, ids):
        vals.append(np.full(len(ids), v, np.uint64)); tids.append(np.asarray(ids, np.int32))

    pool = _metamers(rng, 9000)
    cut = 3735
    group(LOWEST, sh.strains[65][1])
    lo_singles, rest = pool[:cut], pool[cut:]
    group_600_value, rest = rest[0], rest[1:]
    for v in lo_singles:
        group(v, [rng.choice(all_strains)])
    group(group_600_value, sh.strains[600][1])
    it = iter(rest)
    for n in GROUP_SIZES:
        group(next(it), big[:n])
    for n in (15, 16, 17, 64, 65):
        group(next(it), sh.strains[n][1])
    group(next(it), [big[7]] * 17)                                                       # 17 exact duplicates
    v = next(it); group(v, sh.strains[3][1]); group(v, [sh.strains[3][1][1]] * 2)
    v = next(it); group(v, sh.strains[2][1]); group(v, sh.strains[3][1])                 # one value, two species (one genus)
    v = next(it); group(v, sh.strains[15][1][:4]); group(v, sh.strains[200][1][:40]); group(v, [sh.strains[1][1][0]])     # ... three species, two genera
    v = next(it); group(v, sh.strains[16][1][:5]); group(v, sh.strains[2][1]); group(v, big[:20])                        # ... three species, three genera
    group(next(it), [ALIAS])
    group(next(it), [ALIAS, sh.strains[3][1][1]])
    group(next(it), [ALIAS, sh.aliases[ALIAS]])
    group(next(it), [big_sp, big[3]])
    group(next(it), [big[5]] + big[100:130] + [big[5]])
    for v in it:
        group(v, [rng.choice(all_strains)])
    group(HIGHEST, sh.strains[17][1])
    return np.concatenate(vals), np.concatenate(tids)


def _params(**kw):
    import metabuli_amd as M
    return M.default_params(seq_mode=1, syncmer=1, **kw)


def _write_db(ctx, taxdir, vals, tids, d, split_num):
    """the database of these records, built on the device and written"""
    os.makedirs(d, exist_ok=True)
    b = ctx.builder(taxdir, _params())
    b.add_records(vals, tids)
    ix = b.finish()
    ix.write(d, split_num)
    ix.close(); b.close()
    return d


def _same_files(a, b, names=ALL_FILES):
    for name in names:
        x, y = open(os.path.join(a, name), "rb").read(), open(os.path.join(b, name), "rb").read()
        assert x == y, f"{name} differs ({len(x)} / {len(y)} bytes)"


def _download(ctx, d, taxdir):
    ix = ctx.open_index(d, _params(), taxonomy_dir=taxdir)
    v, i = ix.download()
    ix.close()
    return v, i


def _read_db(orc, d):
    """(values, info) of a database directory, decoded by the oracle's reader"""
    return orc.diffidx_decode(np.fromfile(os.path.join(d, "diffIdx"), dtype=np.uint16)), np.fromfile(os.path.join(d, "info"), dtype=np.uint32)


def _kept(tax, aliases, select, exclude, ids):
    """which of the records / entries with these ids the filter keeps, by the spec"""
    keep = S.keep_table(tax, aliases, select, exclude)
    uniq, inv = np.unique(np.asarray(ids, np.int64), return_inverse=True)
    return keep[S.record_keys(tax, aliases, uniq)[inv]] != 0


class World:
    """the shape records, their database (64 checkpoints), and the subsets the tests share: out directory, statistics, kept mask"""

    def __init__(self, ctx, sh, base):
        from build_spec import spec_finish
        self.ctx, self.sh, self.base = ctx, sh, base
        self.vals, self.tids = _shape_records(sh)
        assert 9000 < len(self.vals) < 12000
        self.db = _write_db(ctx, sh.dir, self.vals, self.tids, str(base / "full"), 64)
        self.entry_values, self.entry_ids, _ = spec_finish(self.vals, self.tids, sh.dir)
        self.n = 0
        self._subsets = {}

    def out(self):
        self.n += 1
        d = str(self.base / f"out{self.n}"); os.makedirs(d)
        return d

    def subset(self, select, exclude):
        """the filtered merge of the full database at the default range size (made once per filter)"""
        key = (tuple(select), tuple(exclude))
        if key not in self._subsets:
            d = self.out()
            st = self.ctx.merge_databases([self.db], self.sh.dir, _params(), d, split_num=64, select=select, exclude=exclude)
            self._subsets[key] = (d, st)
        return self._subsets[key]

    def cases(self):
        sh = self.sh
        return {"exclude_genus": ([], [sh.genera[1]]), "select_genus": ([sh.genera[2]], []), "select_genus_exclude_species": ([sh.genera[0]], [sh.species(3)]),
                "exclude_1200": ([], [sh.species(1200)]), "exclude_first": ([], [sh.species(65)]), "select_one_strain_species": ([sh.species(1)], [])}


@pytest.fixture(scope="module")
def shapes(tmp_path_factory):
    return Shapes(tmp_path_factory.mktemp("clade_tax"))


@pytest.fixture(scope="module")
def world(ctx, shapes, tmp_path_factory):
    return World(ctx, shapes, tmp_path_factory.mktemp("clade_world"))


# ---------------------------------------------------------------------------------------------------------------------
# 2. a subset equals a build of the kept species' records
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["exclude_genus", "select_genus", "select_genus_exclude_species", "exclude_1200"])
def test_subset_equals_a_build_of_the_kept_species(ctx, world, tmp_path, case):
    from build_spec import spec_finish
    sh = world.sh
    select, exclude = world.cases()[case]
    out, st = world.subset(select, exclude)
    kept = _kept(sh.tax, sh.aliases, select, exclude, world.tids)
    assert 0 < kept.sum() < len(kept)
    ref = _write_db(ctx, sh.dir, world.vals[kept], world.tids[kept], str(tmp_path / "ref"), 64)
    _same_files(out, ref)
    ev, ei, _ = spec_finish(world.vals[kept], world.tids[kept], sh.dir)
    gv, gi = _download(ctx, out, sh.dir)
    assert st["n_entries"] == len(ev) == len(gv) and (gv == ev).all() and (gi == ei).all()
    # the statistics, by the spec over the full database's entries
    want = S.statistics(sh.tax, sh.aliases, select, exclude, world.entry_ids)
    assert {k: st[k] for k in want} == want
    assert st["n_input_entries"] == st["n_records_in"] == len(world.entry_ids) and st["n_records_kept"] == st["n_entries"]
    assert st["n_species_dropped"] > 0 and st["ms_filter"] > 0


# ---------------------------------------------------------------------------------------------------------------------
# 3. independence of the range cut
# ---------------------------------------------------------------------------------------------------------------------
def _smallest_range(ctx, world, select, exclude):
    """the smallest max_range_records the planner accepts for the full database: what its refusal asks for"""
    import metabuli_amd as M
    with pytest.raises(M.MtbError) as e:
        ctx.merge_databases([world.db], world.sh.dir, _params(), world.out(), split_num=64, max_range_records=1, select=select, exclude=exclude)
    assert e.value.status == M.MTB_ERR_CAPACITY
    return int(re.search(r"room for (\d+) records", str(e.value)).group(1))


@pytest.mark.parametrize("case", ["exclude_genus", "exclude_first", "select_one_strain_species"])
def test_range_cut_does_not_matter(ctx, world, case):
    """exclude_genus drops the last entry of the database (the highest word, 17-strain species), exclude_first the first one (the lowest
    word, 65-strain species); select_one_strain_species keeps fewer entries than there are ranges: whole ranges are dropped"""
    sh = world.sh
    select, exclude = world.cases()[case]
    out, st0 = world.subset(select, exclude)
    assert st0["n_ranges"] == 1
    fv, fi = world.entry_values, world.entry_ids
    gv, _ = _download(ctx, out, sh.dir)
    if case == "exclude_genus":
        assert fv[-1] == HIGHEST and gv[-1] != HIGHEST
    if case == "exclude_first":
        assert fv[0] == LOWEST and gv[0] != LOWEST
    smallest = _smallest_range(ctx, world, select, exclude)
    for mrr in (len(fv) // 3, smallest):
        d = world.out()
        st = ctx.merge_databases([world.db], sh.dir, _params(), d, split_num=64, max_range_records=mrr, select=select, exclude=exclude)
        assert st["n_ranges"] >= 3 and st["max_range_records_used"] <= mrr
        if case == "select_one_strain_species" and mrr == smallest:
            assert st["n_ranges"] > st["n_entries"] > 0                                  # at least one range kept nothing
        _same_files(d, out)
        assert {k: st[k] for k in ("n_entries", "n_records_in", "n_records_kept", "n_species_kept", "n_species_dropped")} == \
               {k: st0[k] for k in ("n_entries", "n_records_in", "n_records_kept", "n_species_kept", "n_species_dropped")}


# ---------------------------------------------------------------------------------------------------------------------
# 4. several inputs
# ---------------------------------------------------------------------------------------------------------------------
def test_several_inputs(ctx, world, tmp_path):
    """the records dealt record by record over three databases (every larger species is split across them)"""
    sh = world.sh
    to = np.random.default_rng(9).integers(0, 3, len(world.vals))
    sp600 = np.isin(world.tids, sh.strains[600][1])
    assert all((sp600 & (to == k)).any() for k in range(3))
    dbs = [_write_db(ctx, sh.dir, world.vals[to == k], world.tids[to == k], str(tmp_path / f"in{k}"), 64) for k in range(3)]
    for case in ("exclude_genus", "select_genus_exclude_species"):
        select, exclude = world.cases()[case]
        single, st1 = world.subset(select, exclude)
        for mrr in (0, 1500):
            d = world.out()
            st = ctx.merge_databases(dbs, sh.dir, _params(), d, split_num=64, max_range_records=mrr, select=select, exclude=exclude)
            assert (st["n_ranges"] > 1) == (mrr != 0)
            _same_files(d, single)
            assert st["n_entries"] == st1["n_entries"] and st["n_records_kept"] >= st1["n_records_kept"]
            assert (st["n_species_kept"], st["n_species_dropped"]) == (st1["n_species_kept"], st1["n_species_dropped"])


# ---------------------------------------------------------------------------------------------------------------------
# 5. legacy and foreign inputs
# ---------------------------------------------------------------------------------------------------------------------
def _copy_db(src, dst):
    os.makedirs(dst)
    for name in ALL_FILES:
        open(os.path.join(dst, name), "wb").write(open(os.path.join(src, name), "rb").read())
    return dst


def _filtered_equals_unfiltered_without_the_dropped(ctx, orc, dbs, taxdir, tax, aliases, select, exclude, base, want_resorted, split_num=16):
    for mrr in (0, 1000):
        plain, filt = str(base / f"plain{mrr}"), str(base / f"filt{mrr}")
        os.makedirs(plain); os.makedirs(filt)
        st_plain = ctx.merge_databases(dbs, taxdir, _params(), plain, split_num=split_num, max_range_records=mrr)
        st = ctx.merge_databases(dbs, taxdir, _params(), filt, split_num=split_num, max_range_records=mrr, select=select, exclude=exclude)
        assert (st["n_resorted_slices"] > 0) == want_resorted and (st_plain["n_resorted_slices"] > 0) == want_resorted
        pv, pi = _read_db(orc, plain)
        gv, gi = _read_db(orc, filt)
        kept = _kept(tax, aliases, select, exclude, pi)
        assert 0 < kept.sum() < len(kept)
        assert len(gv) == kept.sum() == st["n_entries"] and (gv == pv[kept]).all() and (gi == pi[kept]).all()
        assert (np.fromfile(os.path.join(filt, "taxID_list"), sep="\n", dtype=np.int64) >= 0).all()


def test_legacy_input(ctx, orc, world, tmp_path):
    """Skip_redundancy 0 and bit 31 set on a third of the info entries: filtered as if the bit were clear"""
    sh = world.sh
    leg = _copy_db(world.db, str(tmp_path / "legacy"))
    info = np.fromfile(os.path.join(leg, "info"), dtype=np.uint32)
    flagged = np.random.default_rng(5).random(len(info)) < 0.33
    assert flagged.sum() > 100
    (info | (flagged.astype(np.uint32) << np.uint32(31))).astype(np.uint32).tofile(os.path.join(leg, "info"))
    txt = open(os.path.join(leg, "db.parameters")).read().replace("Skip_redundancy\t1", "Skip_redundancy\t0")
    assert "Skip_redundancy\t0" in txt
    open(os.path.join(leg, "db.parameters"), "w").write(txt)
    select, exclude = world.cases()["exclude_genus"]
    _filtered_equals_unfiltered_without_the_dropped(ctx, orc, [leg], sh.dir, sh.tax, sh.aliases, select, exclude, tmp_path, False, split_num=64)
    _same_files(str(tmp_path / "filt0"), world.subset(select, exclude)[0])


def test_input_built_under_another_taxonomy(ctx, orc, shapes, tmp_path):
    """A is built under T1.  T2 = T1 with one strain of the 2-strain species moved under the 15-strain species, whose id is larger than
    the 3-strain species' id: a value that carries this strain and a strain of the 3-strain species is stored (moved strain, other
    strain) in A and sorts the other way round under T2, so the slice is sorted again -- behind the filter."""
    import copy
    sp2, st2 = shapes.strains[2]; sp3, st3 = shapes.strains[3]; sp15, _ = shapes.strains[15]
    assert sp2 < sp3 < sp15
    moved = st2[0]
    tax2 = copy.deepcopy(shapes.tax)
    tax2.parent[moved] = sp15
    t2 = S.write_taxonomy(tax2, shapes.aliases, str(tmp_path / "t2"))
    rng = np.random.default_rng(23)
    strains = np.array(shapes.strains[1200][1][:30] + st2 + st3 + shapes.strains[16][1], np.int32)
    pool = _metamers(rng, 2501)
    vals = np.concatenate([pool[:2500], [pool[2500], pool[2500]]]).astype(np.uint64)
    tids = np.concatenate([rng.choice(strains, size=2500), [moved, st3[1]]]).astype(np.int32)
    a = _write_db(ctx, shapes.dir, vals, tids, str(tmp_path / "a"), 16)
    other = _write_db(ctx, shapes.dir, pool[:500], rng.choice(strains, size=500), str(tmp_path / "b"), 16)
    for tag, dbs, select, exclude in (("one", [a], [], [sp3]), ("two", [a, other], [shapes.genera[0]], [sp2])):
        base = tmp_path / tag; os.makedirs(base)
        _filtered_equals_unfiltered_without_the_dropped(ctx, orc, dbs, t2, tax2, shapes.aliases, select, exclude, base, True)


# ---------------------------------------------------------------------------------------------------------------------
# 6. refusals and statistics
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals(ctx, world, tmp_path):
    import metabuli_amd as M
    sh = world.sh
    out = str(tmp_path / "out"); os.makedirs(out)
    stale = os.path.join(out, "db.parameters")

    def refused(select, exclude, names, dbs=None, **kw):
        open(stale, "w").write("DB_name\tstale\n")                                       # a database that was here before must not survive a refused merge
        with pytest.raises(M.MtbError) as e:
            ctx.merge_databases(dbs or [world.db], sh.dir, _params(), out, split_num=64, select=select, exclude=exclude, **kw)
        assert e.value.status == M.MTB_ERR_ARG, str(e.value)
        assert names in str(e.value), str(e.value)
        assert not os.path.exists(stale)
        assert not os.path.exists(os.path.join(out, "split"))                            # nothing finished

    strain = sh.strains[64][1][5]
    refused([7777], [], "7777")                                                          # an id the taxonomy does not know
    refused([], [sh.genera[0], ALIAS + 1], str(ALIAS + 1))
    refused([strain], [], str(strain))                                                   # a strain
    refused([sh.genera[1]], [ALIAS], str(ALIAS))                                         # ... under its old id
    refused([], [], "nothing to filter")                                                 # both lists empty
    refused([], [1], "keeps none")                                                       # nothing kept: the root excluded,
    refused([sh.empty_genus], [], "keeps none")                                          # ... a genus without entries selected,
    refused([sh.genera[1]], [sh.genera[1]], "keeps none", max_range_records=1500)        # ... selected and excluded
    # an unknown id among the entries is an error even where the filter would drop it
    bad = _copy_db(world.db, str(tmp_path / "bad"))
    info = np.fromfile(os.path.join(bad, "info"), dtype=np.uint32)
    at = int(np.flatnonzero(np.isin(info, sh.strains[1200][1]))[3])
    info[at] = 777777
    info.tofile(os.path.join(bad, "info"))
    refused([], [sh.species(1200)], "777777", dbs=[bad])
    # the output directory is one of the inputs: refused with the input left as it was
    twin = _copy_db(world.db, str(tmp_path / "twin"))
    os.symlink(twin, str(tmp_path / "link"))
    for d in (twin, str(tmp_path / "link"), twin + "/."):
        with pytest.raises(M.MtbError) as e:
            ctx.merge_databases([world.db, twin], sh.dir, _params(), d, split_num=64, exclude=[sh.genera[1]])
        assert e.value.status == M.MTB_ERR_ARG
        _same_files(twin, world.db)
    # and the directory still takes a good merge afterwards
    select, exclude = world.cases()["exclude_genus"]
    ctx.merge_databases([world.db], sh.dir, _params(), out, split_num=64, select=select, exclude=exclude)
    _same_files(out, world.subset(select, exclude)[0])


def test_unmatched_ids_are_reported(ctx, world):
    """a listed genus the database holds nothing of: a warning's worth of statistics, not a silent no-op"""
    sh = world.sh
    sub, _ = world.subset([], [sh.genera[1]])                                            # a database without genus 1
    sv, si = _download(ctx, sub, sh.dir)
    for select, exclude in (([], [sh.genera[1], sh.species(15)]), ([sh.genera[0], sh.empty_genus], [sh.species(16), sh.species(3)])):
        d = world.out()
        st = ctx.merge_databases([sub], sh.dir, _params(), d, split_num=64, select=select, exclude=exclude)
        want = S.statistics(sh.tax, sh.aliases, select, exclude, si)
        assert {k: st[k] for k in want} == want
    assert (want["n_unmatched"], want["first_unmatched"]) == (2, sh.empty_genus)
    d = world.out()
    st = ctx.merge_databases([sub], sh.dir, _params(), d, split_num=64, exclude=[sh.genera[1], sh.species(15)])
    assert (st["n_unmatched"], st["first_unmatched"]) == (1, sh.genera[1])


# ---------------------------------------------------------------------------------------------------------------------
# 7. the result is a database
# ---------------------------------------------------------------------------------------------------------------------
def test_subsets_audit_canonical(ctx, world):
    sh = world.sh
    for case in ("exclude_genus", "select_genus_exclude_species"):
        out, st = world.subset(*world.cases()[case])
        rep, _ = ctx.audit_database(out, taxonomy_dir=sh.dir, params=_params())
        assert rep["valid"] == 1 and rep["canonical"] == 1 and rep["n_entries"] == st["n_entries"]


def test_classification_against_a_subset(ctx, orc, tmp_path):
    """reads of every genus classified against the subset without one genus = against the index finished in memory from the kept
    entries, and = the oracle on the subset's files"""
    import helpers
    import metabuli_amd as M
    from metabuli_amd import synth
    p = helpers.default_params(seq_mode=1, syncmer=1, kmer_format=2)
    w = synth.make_world(seed=11, n_genera=3, species_per_genus=2, strains_per_species=2, genome_len=20000)
    toy = str(tmp_path / "toy"); os.makedirs(toy)
    vals, tids = helpers.build_toy_db(orc, w, p, toy)
    taxdir = os.path.join(toy, "taxonomy")
    genus0 = 4
    assert w.tax.rank[genus0] == "genus"
    sub = str(tmp_path / "sub"); os.makedirs(sub)
    st = ctx.merge_databases([toy], taxdir, _params(), sub, exclude=[genus0])
    kept = _kept(w.tax, {}, [], [genus0], tids)
    assert 0 < kept.sum() < len(kept) and st["n_entries"] == kept.sum()
    w.tax.write(os.path.join(sub, "taxonomy"))
    b, o, _ = synth.sample_reads(np.random.default_rng(3), w, 200, length=150, err=0.01, with_n=0.1)
    mp = _params()
    ix = ctx.open_index(sub, mp)
    got = ctx.classify_batch(ix, mp, b, o)
    ix.close()
    bld = ctx.builder(taxdir, _params())
    bld.add_records(vals[kept], tids[kept])
    mem = bld.finish()
    want = ctx.classify_batch(mem, mp, b, o)
    mem.close(); bld.close()
    for x, y in zip(got, want):
        assert x.tobytes() == y.tobytes()
    assert (got[0]["is_classified"] != 0).sum() > 50
    tax = orc.load_taxonomy(taxdir)
    ref = orc.classify(orc.open_db(sub, tax, p), tax, p, b, o)
    ro, res = ref["results"], got[0]
    ok = (ro["flag"] != 0) | ((res["classification"] == ro["classification"]) & (res["score"].view(np.uint32) == ro["score"].view(np.uint32)))
    assert ok.all()
    # no read is classified into the genus that was taken out
    gone = [t for t in w.tax.parent if genus0 in w.tax.lineage(t)]
    assert not np.isin(res["classification"][res["is_classified"] != 0], gone).any()


# ---------------------------------------------------------------------------------------------------------------------
# 8. mtb_build --select-taxid / --exclude-taxid
# ---------------------------------------------------------------------------------------------------------------------
def _build_program(tmp):
    """mtb_build next to the library under test; against the emulated library it is compiled here"""
    import metabuli_amd as M
    d = os.path.dirname(M.LIB_PATH)
    if os.environ.get("MTB_HIPEMU"):
        exe = os.path.join(str(tmp), "mtb_build")
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-pthread", "-o", exe, os.path.join(ROOT, "metabuli_amd", "csrc", "host", "build_main.cpp"),
                               "-L" + d, "-lmtb", "-lz", "-Wl,-rpath," + d])
        return exe
    subprocess.check_call(["make", "-C", d, "mtb_build"], stdout=subprocess.DEVNULL)
    return os.path.join(d, "mtb_build")


def test_mtb_build_filter_flags(ctx, world, tmp_path):
    sh = world.sh
    exe = _build_program(tmp_path)
    flags = ["--syncmer", "1", "--kmer-format", "2", "--split-num", "64"]
    select, exclude = world.cases()["select_genus_exclude_species"]
    want, st = world.subset(select, exclude)
    out = str(tmp_path / "cli")
    r = subprocess.run([exe] + flags + ["--add-db", world.db, "--select-taxid", str(select[0]), "--exclude-taxid", f"{exclude[0]},{sh.empty_genus}", "--validate-db", "1",
                                        "-", "-", sh.dir, out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    _same_files(out, want)
    assert f"filter kept {st['n_records_kept']} of {st['n_records_in']} entries" in r.stderr
    assert f"{st['n_species_kept']} of {st['n_species_kept'] + st['n_species_dropped']} species" in r.stderr
    assert f"warning: no entry of the inputs lies under taxon {sh.empty_genus}" in r.stderr
    assert re.search(r"(\d+) ranges", r.stderr.strip().split("\n")[-1])
    assert "canonical 1" in r.stdout
    # two inputs, one flag
    select, exclude = world.cases()["exclude_genus"]
    out2 = str(tmp_path / "cli2")
    r = subprocess.run([exe] + flags + ["--add-db", world.db, "--add-db", want, "--exclude-taxid", str(exclude[0]), "-", "-", sh.dir, out2], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    _same_files(out2, world.subset(select, exclude)[0])
    # the flags filter a merge of databases, not a build from genomes
    fa, mp = str(tmp_path / "g.fa"), str(tmp_path / "g.tsv")
    open(fa, "w").write(">s1\n" + "ACGT" * 50 + "\n"); open(mp, "w").write(f"s1\t{sh.strains[2][1][0]}\n")
    for extra in (["--exclude-taxid", str(exclude[0])], ["--add-db", world.db, "--select-taxid", str(sh.genera[2])]):
        out3 = str(tmp_path / "cli3")
        r = subprocess.run([exe] + flags + extra + [fa, mp, sh.dir, out3], capture_output=True, text=True)
        assert r.returncode != 0 and "cannot be combined with genomes" in r.stderr, r.stderr[-2000:]
        assert not os.path.exists(os.path.join(out3, "db.parameters"))
    r = subprocess.run([exe] + flags + ["--add-db", world.db, "--exclude-taxid", "12,x", "-", "-", sh.dir, str(tmp_path / "cli4")], capture_output=True, text=True)
    assert r.returncode != 0 and "not a taxon id" in r.stderr
