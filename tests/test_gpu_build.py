"""GPU tests of the database builder (mtb_builder_*, kernels_build.h): the device sort + per-species LCA dedup against the numpy
restatement of tests/build_spec.py (pinned against synth.dedup_targets in tests/test_build_spec.py) and against the databases
helpers.build_toy_db writes through the oracle; update / merge through open databases; the refusals; the mtb_build program."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DB_FILES = ("diffIdx", "info", "split", "taxID_list")
GROUP_SIZES = (1, 2, 3, 15, 16, 17, 63, 64, 65, 200, 1200)


@pytest.fixture(scope="module")
def ctx():
    import metabuli_amd as M
    c = M.Context(0)
    yield c
    c.close()


# ---------------------------------------------------------------------------------------------------------------------
# hand-made records over a toy taxonomy
# ---------------------------------------------------------------------------------------------------------------------
ALIAS = 9000


class Shapes:
    """root -> Bacteria -> three genera -> species with 1 .. 1200 strains; merged.dmp: ALIAS -> the first strain of the 3-strain species"""

    def __init__(self, d):
        from metabuli_amd import synth
        tax = synth.Taxonomy()
        tax.add(1, 1, "no rank", "root"); tax.add(2, 1, "superkingdom", "Bacteria")
        nxt = 10
        self.strains = {}                                  # strains per species -> (species id, [strain ids])
        for g, counts in enumerate([(1, 2, 3, 15), (16, 17, 63, 64), (65, 200, 600, 1200)]):
            gid = nxt; nxt += 1
            tax.add(gid, 2, "genus", f"G{g}")
            for n in counts:
                sid = nxt; nxt += 1
                tax.add(sid, gid, "species", f"G{g} s{n}")
                ids = list(range(nxt, nxt + n)); nxt += n
                for t in ids:
                    tax.add(t, sid, "no rank", f"strain{t}")
                self.strains[n] = (sid, ids)
        assert nxt < ALIAS
        self.tax, self.dir = tax, str(d)
        tax.write(self.dir)
        self.alias_target = self.strains[3][1][0]
        with open(os.path.join(self.dir, "merged.dmp"), "w") as f:
            f.write(f"{ALIAS}\t|\t{self.alias_target}\t|\n")


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


LOWEST = np.uint64(1)                                                                    # letters 0, DNA part 1
HIGHEST = np.uint64(sum(20 << (24 + 5 * k) for k in range(8)) | 0xFFFFFF)                # letters 20, DNA part all ones


@pytest.fixture(scope="module")
def shapes(tmp_path_factory):
    return Shapes(tmp_path_factory.mktemp("shapes_tax"))


def _shape_records(sh):
    """~10 k records: (values, taxids, notes).  Layout by value: the lowest word is a group of 65 (the first output entry, folded by a wavefront);
    3735 single records; a group of 600 over records 3800 .. 4399 of the sorted list (straddles record 4096: a sort tile of 2048 x 2, a
    workgroup multiple); the group-size ladder, duplicates, two-species values, alias cases; singles; the highest word is a group of 17
    (the last output entry, ends at the end of the list)."""
    rng = np.random.default_rng(42)
    big_sp, big = sh.strains[1200]
    all_strains = np.array([t for _, ids in sh.strains.values() for t in ids], np.int32)
    vals, tids = [], []

    def group(v, ids):
        vals.append(np.full(len(ids), v, np.uint64)); tids.append(np.asarray(ids, np.int32))

    pool = _metamers(rng, 9000)
    cut = 3735
    group(LOWEST, sh.strains[65][1])                                                     # 65 members -> species of 65
    lo_singles, rest = pool[:cut], pool[cut:]
    group_600_value, rest = rest[0], rest[1:]
    for v in lo_singles:
        group(v, [rng.choice(all_strains)])
    group(group_600_value, sh.strains[600][1])
    it = iter(rest)
    for n in GROUP_SIZES:                                                                # n strains of one species: LCA = the species (n = 1: the strain)
        group(next(it), big[:n])
    for n in (15, 16, 17, 64, 65):                                                       # every strain of a species of exactly n strains
        group(next(it), sh.strains[n][1])
    group(next(it), [big[7]] * 17)                                                       # 17 exact duplicates: the strain itself, not its species
    v = next(it); group(v, sh.strains[3][1]); group(v, [sh.strains[3][1][1]] * 2)        # a group of 3 + 2 exact duplicates of one member
    v = next(it); group(v, sh.strains[2][1]); group(v, sh.strains[3][1])                 # one value, two species of one genus: two entries
    v = next(it); group(v, sh.strains[15][1][:4]); group(v, sh.strains[200][1][:40]); group(v, [sh.strains[1][1][0]])     # ... three species, two genera
    group(next(it), [ALIAS])                                                             # alone: the alias's target
    group(next(it), [ALIAS, sh.strains[3][1][1]])                                        # with a sibling: their species
    group(next(it), [ALIAS, sh.alias_target])                                            # alias + its own target: the target
    group(next(it), [big_sp, big[3]])                                                    # a species id next to one of its strains
    group(next(it), [big[5]] + big[100:130] + [big[5]])
    for v in it:
        group(v, [rng.choice(all_strains)])
    group(HIGHEST, sh.strains[17][1])
    vals, tids = np.concatenate(vals), np.concatenate(tids)
    return vals, tids, dict(group_600_value=group_600_value)


def test_group_shapes(ctx, shapes):
    import metabuli_amd as M
    from build_spec import spec_finish
    vals, tids, notes = _shape_records(shapes)
    assert 9000 < len(vals) < 12000
    ev, ei, sp = spec_finish(vals, tids, shapes.dir)
    sizes = sp["ends"] - sp["starts"]
    assert set(GROUP_SIZES) <= set(sizes.tolist())
    g600 = int(np.flatnonzero(ev == notes["group_600_value"])[0])
    assert sizes[g600] == 600 and sp["starts"][g600] < 4096 < sp["ends"][g600] - 1       # straddles record 4096 of the sorted list
    assert sizes[0] == 65 and sizes[-1] == 17 and ev[0] == LOWEST and ev[-1] == HIGHEST
    assert ALIAS not in ei and shapes.alias_target in ei
    rng = np.random.default_rng(7)
    perm = rng.permutation(len(vals))
    vals, tids = vals[perm], tids[perm]
    p = M.default_params(seq_mode=1, syncmer=1)
    b = ctx.builder(shapes.dir, p)
    cuts = [0, len(vals) // 3, len(vals) // 3 + 2500, len(vals)]
    for a, e in zip(cuts[:-1], cuts[1:]):
        b.add_records(vals[a:e], tids[a:e])
    assert b.num_records == len(vals)
    ix = b.finish()
    assert b.num_records == 0
    gv, gi = ix.download()
    st = b.last_finish_stats()
    assert st["n_records"] == len(vals) and st["n_entries"] == len(ev) and st["n_long_groups"] == int((sizes > 16).sum())
    assert len(gv) == len(ev) and (gv == ev).all() and (gi == ei).all()
    # reusable: a second, different build from the same builder
    b.add_records(vals[:100], tids[:100])
    ix2 = b.finish()
    ev2, ei2, _ = spec_finish(vals[:100], tids[:100], shapes.dir)
    gv2, gi2 = ix2.download()
    assert (gv2 == ev2).all() and (gi2 == ei2).all()
    ix2.close(); ix.close(); b.close()


@pytest.mark.parametrize("case", ["one_group", "no_duplicates", "single_record"])
def test_degenerate_inputs(ctx, shapes, case):
    import metabuli_amd as M
    from build_spec import spec_finish
    rng = np.random.default_rng(3)
    big = np.array(shapes.strains[1200][1], np.int32)
    if case == "one_group":
        vals = np.full(5000, _metamers(rng, 1)[0], np.uint64); tids = rng.choice(big, size=5000)
    elif case == "no_duplicates":
        vals = rng.permutation(_metamers(rng, 5000)); tids = rng.choice(big, size=5000)
    else:
        vals = _metamers(rng, 1); tids = big[:1]
    ev, ei, _ = spec_finish(vals, tids, shapes.dir)
    assert len(ev) == {"one_group": 1, "no_duplicates": 5000, "single_record": 1}[case]
    b = ctx.builder(shapes.dir, M.default_params(seq_mode=1, syncmer=1))
    b.add_records(vals, tids)
    ix = b.finish()
    gv, gi = ix.download()
    assert len(gv) == len(ev) and (gv == ev).all() and (gi == ei).all()
    ix.close(); b.close()


# ---------------------------------------------------------------------------------------------------------------------
# from sequences: the toy world of smoke(), against the database build_toy_db writes through the oracle
# ---------------------------------------------------------------------------------------------------------------------
class WorldDb:
    def __init__(self, orc, d, syncmer, kmer_format):
        from helpers import build_toy_db, default_params
        from metabuli_amd import synth
        import metabuli_amd as M
        self.world = synth.make_world(seed=11, n_genera=3, species_per_genus=2, strains_per_species=2, genome_len=20000)
        self.op = default_params(seq_mode=1, syncmer=syncmer, kmer_format=kmer_format)
        self.mp = lambda **kw: M.default_params(seq_mode=1, syncmer=syncmer, kmer_format=kmer_format, **kw)
        self.dbdir = str(d); os.makedirs(self.dbdir, exist_ok=True)
        self.vals, self.tids = build_toy_db(orc, self.world, self.op, self.dbdir)
        self.taxdir = os.path.join(self.dbdir, "taxonomy")

    def seqs(self, which=None):
        g = self.world.genomes if which is None else [self.world.genomes[i] for i in which]
        offs = np.zeros(len(g) + 1, np.uint64); offs[1:] = np.cumsum([len(s) for _, s in g])
        return np.concatenate([s for _, s in g]), offs, np.array([t for t, _ in g], np.int32)

    def build(self, ctx, which=None):
        b = ctx.builder(self.taxdir, self.mp())
        b.add_sequences(*self.seqs(which))
        ix = b.finish()
        b.close()
        return ix


WORLD_MODES = {"sync_f2": (1, 2), "dense_f2": (0, 2), "dense_f1": (0, 1)}


@pytest.fixture(scope="module", params=list(WORLD_MODES))
def wdb(request, orc, tmp_path_factory):
    return WorldDb(orc, tmp_path_factory.mktemp("wdb_" + request.param), *WORLD_MODES[request.param])


@pytest.fixture(scope="module")
def wsync(orc, tmp_path_factory):
    return WorldDb(orc, tmp_path_factory.mktemp("wdb_sync"), 1, 2)


def _same_files(a, b):
    for name in DB_FILES:
        x, y = open(os.path.join(a, name), "rb").read(), open(os.path.join(b, name), "rb").read()
        assert x == y, f"{name} differs ({len(x)} / {len(y)} bytes)"


def _equals(ix, w):
    gv, gi = ix.download()
    assert len(gv) == len(w.vals) and (gv == w.vals).all() and (gi == w.tids.astype(np.uint32)).all()


def test_build_from_sequences(ctx, wdb, tmp_path):
    """add_sequences + finish = the (values, taxids) build_toy_db returns; Index.write of it = the files the oracle's writer wrote
    (formats 2 and 1, syncmer and dense)"""
    ix = wdb.build(ctx)
    _equals(ix, wdb)
    st = ix.state()
    assert not st["packed"] and not st["sealed"]
    ix.write(str(tmp_path))
    _same_files(str(tmp_path), wdb.dbdir)
    ix.close()


def _half_dbs(ctx, w, base):
    """databases A (first half of the genomes) and B (second half), built on the device, written, reopened"""
    n = len(w.world.genomes)
    out = []
    for name, which in (("A", range(0, n // 2)), ("B", range(n // 2, n))):
        d = str(base / name); os.makedirs(d)
        ix = w.build(ctx, list(which))
        ix.write(d); ix.close()
        w.world.tax.write(os.path.join(d, "taxonomy"))
        out.append(d)
    return out


def test_update_and_merge(ctx, wsync, tmp_path):
    w = wsync
    n = len(w.world.genomes)
    da, db_ = _half_dbs(ctx, w, tmp_path)
    # updateDB: old database + new genomes
    a = ctx.open_index(da, w.mp())
    b = ctx.builder(w.taxdir, w.mp())
    b.add_index(a)
    assert b.num_records == a.num_targets
    b.add_sequences(*w.seqs(list(range(n // 2, n))))
    ix = b.finish()
    _equals(ix, w)
    ix.close()
    # merge of two databases
    bb = ctx.open_index(db_, w.mp())
    b.add_index(a); b.add_index(bb)
    ix = b.finish()
    _equals(ix, w)
    ix.close(); bb.close(); a.close()
    # a legacy database (Skip_redundancy 0, bit 31 set on a third of the entries) merges as if the bit were clear
    dl = str(tmp_path / "legacy"); os.makedirs(dl)
    for name in ("diffIdx", "split", "taxID_list"):
        open(os.path.join(dl, name), "wb").write(open(os.path.join(da, name), "rb").read())
    w.world.tax.write(os.path.join(dl, "taxonomy"))
    info = np.fromfile(os.path.join(da, "info"), dtype=np.uint32)
    flagged = np.random.default_rng(5).random(len(info)) < 0.33
    (info | (flagged.astype(np.uint32) << np.uint32(31))).astype(np.uint32).tofile(os.path.join(dl, "info"))
    txt = open(os.path.join(da, "db.parameters")).read().replace("Skip_redundancy\t1", "Skip_redundancy\t0")
    assert "Skip_redundancy\t0" in txt
    open(os.path.join(dl, "db.parameters"), "w").write(txt)
    lp = w.mp(skip_redundancy=0)
    leg = ctx.open_index(dl, lp)
    assert lp.skip_redundancy == 0 and (leg.download()[1] >> 31).sum() == flagged.sum() > 0
    b.add_index(leg)
    b.add_sequences(*w.seqs(list(range(n // 2, n))))
    ix = b.finish()
    _equals(ix, w)
    ix.close(); leg.close(); b.close()


def test_built_index_classifies(ctx, orc, wsync):
    """the index finish() returns, with no file round trip, against Oracle.classify on build_toy_db's files (what smoke() compares)"""
    from metabuli_amd import synth
    w = wsync
    tax = orc.load_taxonomy(w.taxdir)
    db = orc.open_db(w.dbdir, tax, w.op)
    bases, offs, _ = synth.sample_reads(np.random.default_rng(3), w.world, 200, length=150, err=0.01, with_n=0.1)
    ref = orc.classify(db, tax, w.op, bases, offs)
    ix = w.build(ctx)
    res, tt, tc = ctx.classify_batch(ix, w.mp(), bases, offs)
    ro = ref["results"]
    ok = (ro["flag"] != 0) | ((res["classification"] == ro["classification"]) & (res["score"].view(np.uint32) == ro["score"].view(np.uint32)))
    assert ok.all()
    assert (tt == ref["tc_tax"]).all() and (tc == ref["tc_cnt"]).all()
    assert (res["is_classified"] != 0).sum() > 100
    ix.close()


def test_refusals(ctx, wsync, tmp_path):
    import metabuli_amd as M
    w = wsync
    b = ctx.builder(w.taxdir, w.mp())
    with pytest.raises(M.MtbError) as e:
        b.finish()
    assert e.value.status == M.MTB_ERR_ARG
    keep_v, keep_t = w.vals[:500], w.tids[:500]
    b.add_records(keep_v, keep_t)
    # an id the taxonomy does not know: named in the message, nothing added
    bad_t = keep_t.copy(); bad_t[123] = 777777
    with pytest.raises(M.MtbError) as e:
        b.add_records(keep_v, bad_t)
    assert e.value.status == M.MTB_ERR_ARG and "777777" in str(e.value)
    bases, offs, st = w.seqs([0, 1])
    with pytest.raises(M.MtbError) as e:
        b.add_sequences(bases, offs, np.array([st[0], 424242], np.int32))
    assert e.value.status == M.MTB_ERR_ARG and "424242" in str(e.value)
    assert b.num_records == 500
    # an index of another k-mer format; a view
    full = w.build(ctx)
    other = ctx.builder(w.taxdir, M.default_params(seq_mode=1, syncmer=1, kmer_format=1))
    with pytest.raises(M.MtbError) as e:
        other.add_index(full)
    assert e.value.status == M.MTB_ERR_ARG
    other.close()
    view = full.slice(int(w.vals[10]), int(w.vals[200]), False)
    with pytest.raises(M.MtbError) as e:
        b.add_index(view)
    assert e.value.status == M.MTB_ERR_ARG
    view.close()
    # an index that holds an id the builder's taxonomy lacks
    from metabuli_amd import synth
    small = synth.make_world(seed=11, n_genera=1, species_per_genus=1, strains_per_species=1, genome_len=300)
    d = str(tmp_path / "small_tax")
    small.tax.write(d)
    nb = ctx.builder(d, w.mp())
    with pytest.raises(M.MtbError) as e:
        nb.add_index(full)
    assert e.value.status == M.MTB_ERR_ARG and "taxid" in str(e.value)
    assert nb.num_records == 0
    nb.close(); full.close()
    # after the refusals the builder still finishes with what it held
    assert b.num_records == 500
    ix = b.finish()
    gv, gi = ix.download()
    assert (gv == keep_v).all() and (gi == keep_t.astype(np.uint32)).all()
    ix.close(); b.close()


# ---------------------------------------------------------------------------------------------------------------------
# the command-line program
# ---------------------------------------------------------------------------------------------------------------------
def _programs(tmp):
    """(mtb_build, mtb_classify) next to the library under test; against the emulated library mtb_build is compiled here"""
    import metabuli_amd as M
    d = os.path.dirname(M.LIB_PATH)
    if os.environ.get("MTB_HIPEMU"):
        exe = os.path.join(str(tmp), "mtb_build")
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-pthread", "-o", exe, os.path.join(ROOT, "metabuli_amd", "csrc", "host", "build_main.cpp"),
                               "-L" + d, "-lmtb", "-lz", "-Wl,-rpath," + d])
        return exe, os.path.join(d, "mtb_classify")
    subprocess.check_call(["make", "-C", d, "mtb_build", "mtb_classify"], stdout=subprocess.DEVNULL)
    return os.path.join(d, "mtb_build"), os.path.join(d, "mtb_classify")


def _write_fasta(path, w, which, mapf):
    with open(path, "w") as f, open(mapf, "w") as m:
        for i in which:
            tid, g = w.world.genomes[i]
            s = bytes(g).decode()
            f.write(f">seq{i}.1 some description\n")
            for k in range(0, len(s), 70):
                f.write(s[k:k + 70] + "\n")
            m.write(f"seq{i}.1\t{tid}\n")


def test_mtb_build_program(ctx, orc, wsync, tmp_path):
    from metabuli_amd import synth
    w = wsync
    n = len(w.world.genomes)
    build_exe, classify_exe = _programs(tmp_path)
    flags = ["--syncmer", "1", "--kmer-format", "2"]
    fa, mp = str(tmp_path / "all.fa"), str(tmp_path / "all.tsv")
    _write_fasta(fa, w, range(n), mp)
    out = str(tmp_path / "out")
    subprocess.check_call([build_exe] + flags + [fa, mp, w.taxdir, out], stderr=subprocess.DEVNULL)
    _same_files(out, w.dbdir)
    assert os.path.exists(os.path.join(out, "taxonomy", "nodes.dmp"))
    # mtb_classify on OUTDB = on build_toy_db's directory
    bases, offs, _ = synth.sample_reads(np.random.default_rng(3), w.world, 200, length=150, err=0.01, with_n=0.1)
    fq = str(tmp_path / "reads.fq")
    with open(fq, "w") as f:
        for i in range(len(offs) - 1):
            s = bytes(bases[int(offs[i]):int(offs[i + 1])]).decode()
            f.write(f"@r{i}\n{s}\n+\n{'I' * len(s)}\n")
    rows = []
    for db in (out, w.dbdir):
        od = tmp_path / ("cls_" + os.path.basename(db)); od.mkdir()
        subprocess.check_call([classify_exe, "--seq-mode", "1", fq, db, str(od), "j"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        rows.append(open(od / "j_classifications.tsv").read())
    assert rows[0] == rows[1] and rows[0].count("\n") == 201          # a header line + one row per read
    # update: --add-db A + the second half = the full build
    da, _ = _half_dbs(ctx, w, tmp_path)
    fa2, mp2 = str(tmp_path / "half.fa"), str(tmp_path / "half.tsv")
    _write_fasta(fa2, w, range(n // 2, n), mp2)
    out2 = str(tmp_path / "out2")
    subprocess.check_call([build_exe] + flags + ["--add-db", da, fa2, mp2, w.taxdir, out2], stderr=subprocess.DEVNULL)
    _same_files(out2, w.dbdir)
    # an id the map lacks is a loud error
    open(mp2, "w").write("somethingelse\t5\n")
    r = subprocess.run([build_exe] + flags + [fa2, mp2, w.taxdir, str(tmp_path / "out3")], capture_output=True, text=True)
    assert r.returncode != 0 and "is not in" in r.stderr
