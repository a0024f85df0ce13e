"""GPU tests of the streamed database merge (mtb_merge_databases, mtb_merge_sorted; kernels_merge.h, host/merge_plan.h, the range
writer behind mtb_index_write): the merge kernel at its tile edges against numpy, merged databases byte for byte against the
in-memory route (builder + add_index + finish + write) and against the numpy restatement of tests/build_spec.py, inputs built under
another taxonomy, legacy inputs, the refusals, and `mtb_build --max-records`."""
import os
import re
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL_FILES = ("diffIdx", "info", "split", "taxID_list", "db.parameters")
DB_FILES = ALL_FILES[:4]
GROUP_SIZES = (1, 2, 3, 15, 16, 17, 63, 64, 65, 200, 1200)
T = 2048                                                                                 # MTB_MERGE_TILE (kernels_merge.h); checked against the binding below


@pytest.fixture(scope="module")
def ctx():
    import metabuli_amd as M
    c = M.Context(0)
    yield c
    c.close()


# ---------------------------------------------------------------------------------------------------------------------
# 1. the merge kernel at tile edges
# ---------------------------------------------------------------------------------------------------------------------
SIZES = (0, 1, T - 1, T, T + 1, 2 * T + 1, 5000)


def _lists(pattern, na, nb, rng):
    """two kmer_dt lists, each ascending in (value, qinfo)"""
    import metabuli_amd as M
    a, b = np.zeros(na, M.kmer_dt), np.zeros(nb, M.kmer_dt)
    if pattern == "a_below_b":
        a["value"] = np.arange(na) * 3 + 1; b["value"] = np.arange(nb) * 3 + 1 + 3 * na
        a["qinfo"] = rng.integers(0, 1 << 40, na); b["qinfo"] = rng.integers(0, 1 << 40, nb)
    elif pattern == "b_below_a":
        b["value"] = np.arange(nb) * 3 + 1; a["value"] = np.arange(na) * 3 + 1 + 3 * nb
        a["qinfo"] = rng.integers(0, 1 << 40, na); b["qinfo"] = rng.integers(0, 1 << 40, nb)
    elif pattern == "interleaved":
        a["value"] = np.arange(na) * 2; b["value"] = np.arange(nb) * 2 + 1
        a["qinfo"] = 7; b["qinfo"] = 9
    elif pattern == "all_equal":
        a["value"] = 5; b["value"] = 5; a["qinfo"] = 11; b["qinfo"] = 11
    else:                                                                                # runs of one value whose qinfo differ, of lengths that straddle tile edges
        for x, n, salt in ((a, na, 0), (b, nb, 1)):
            x["value"] = np.arange(n) // 700                                             # runs of 700: records 1400 .. 2099 of a list cross record 2048
            x["qinfo"] = (np.arange(n) % 700) * 2 + salt                                 # inside a run: a even, b odd
    return a, b


@pytest.mark.parametrize("pattern", ["a_below_b", "b_below_a", "interleaved", "all_equal", "runs"])
def test_merge_kernel_at_tile_edges(ctx, pattern):
    import metabuli_amd as M
    assert M.MERGE_TILE == T
    rng = np.random.default_rng(1)
    for na in SIZES:
        for nb in SIZES:
            if na + nb == 0:
                continue
            a, b = _lists(pattern, na, nb, rng)
            got = ctx.merge_sorted(a, b)
            cat = np.concatenate([a, b])
            want = cat[np.lexsort((cat["qinfo"], cat["value"]))]                         # (equal records are indistinguishable)
            assert len(got) == na + nb
            assert (got["value"] == want["value"]).all() and (got["qinfo"] == want["qinfo"]).all(), (pattern, na, nb)


# ---------------------------------------------------------------------------------------------------------------------
# hand-made records over a toy taxonomy (the shapes of tests/test_gpu_build.py)
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
        self.write(self.dir)
        self.alias_target = self.strains[3][1][0]

    def write(self, d):
        self.tax.write(d)
        with open(os.path.join(d, "merged.dmp"), "w") as f:
            f.write(f"{ALIAS}\t|\t{self.strains[3][1][0]}\t|\n")


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
    """~10 k records (values, taxids): group sizes 1 .. 1200, exact duplicates, two- and three-species values, merged.dmp alias cases,
    the lowest and the highest legal word"""
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
    v = next(it); group(v, sh.strains[2][1]); group(v, sh.strains[3][1])                 # one value, two species
    v = next(it); group(v, sh.strains[15][1][:4]); group(v, sh.strains[200][1][:40]); group(v, [sh.strains[1][1][0]])     # ... three species
    group(next(it), [ALIAS])
    group(next(it), [ALIAS, sh.strains[3][1][1]])
    group(next(it), [ALIAS, sh.alias_target])
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


def _in_memory(ctx, dbdirs, taxdir, out, split_num, open_params=None):
    """the route the merge must equal: a builder over the open inputs, finish, write"""
    os.makedirs(out, exist_ok=True)
    b = ctx.builder(taxdir, _params())
    for i, d in enumerate(dbdirs):
        ix = ctx.open_index(d, open_params[i] if open_params else _params(), taxonomy_dir=taxdir)
        b.add_index(ix)
        ix.close()
    ix = b.finish()
    ix.write(out, split_num)
    ix.close(); b.close()
    return out


def _same_files(a, b, names=ALL_FILES):
    for name in names:
        x, y = open(os.path.join(a, name), "rb").read(), open(os.path.join(b, name), "rb").read()
        assert x == y, f"{name} differs ({len(x)} / {len(y)} bytes)"


def _download(ctx, d, taxdir):
    ix = ctx.open_index(d, _params(), taxonomy_dir=taxdir)
    v, i = ix.download()
    ix.close()
    return v, i


class Dealt:
    """the shape records dealt record by record to three inputs, each written with 64 checkpoints; the in-memory merges to compare with"""

    def __init__(self, ctx, sh, base):
        self.sh, self.base = sh, base
        self.vals, self.tids = _shape_records(sh)
        assert 9000 < len(self.vals) < 12000
        to = np.random.default_rng(9).integers(0, 3, len(self.vals))
        self.dbs = [_write_db(ctx, sh.dir, self.vals[to == k], self.tids[to == k], str(base / f"in{k}"), 64) for k in range(3)]
        self.ref = {sn: _in_memory(ctx, self.dbs, sh.dir, str(base / f"ref{sn}"), sn) for sn in (64, 7)}


@pytest.fixture(scope="module")
def shapes(tmp_path_factory):
    return Shapes(tmp_path_factory.mktemp("merge_tax"))


@pytest.fixture(scope="module")
def dealt(ctx, shapes, tmp_path_factory):
    return Dealt(ctx, shapes, tmp_path_factory.mktemp("merge_dealt"))


# ---------------------------------------------------------------------------------------------------------------------
# 2. groups that straddle inputs and ranges
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split_num", [64, 7])
@pytest.mark.parametrize("max_range_records", [0, 1500])
def test_groups_straddle_inputs_and_ranges(ctx, dealt, tmp_path, split_num, max_range_records):
    from build_spec import spec_finish
    out = str(tmp_path / "out"); os.makedirs(out)
    st = ctx.merge_databases(dealt.dbs, dealt.sh.dir, _params(), out, split_num=split_num, max_range_records=max_range_records)
    if max_range_records:
        assert st["n_ranges"] >= 4 and st["max_range_records_used"] <= max_range_records
    else:
        assert st["n_ranges"] == 1
    assert st["n_resorted_slices"] == 0
    _same_files(out, dealt.ref[split_num])
    ev, ei, _ = spec_finish(dealt.vals, dealt.tids, dealt.sh.dir)
    gv, gi = _download(ctx, out, dealt.sh.dir)
    assert st["n_entries"] == len(ev) == len(gv) and (gv == ev).all() and (gi == ei).all()
    assert st["n_input_entries"] == sum(os.path.getsize(os.path.join(d, "info")) // 4 for d in dealt.dbs)


# ---------------------------------------------------------------------------------------------------------------------
# 3. disjoint and lopsided inputs
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["a_below_b", "single_entry", "one_db", "eight", "five"])
def test_disjoint_and_lopsided_inputs(ctx, shapes, tmp_path, case):
    from build_spec import spec_finish
    rng = np.random.default_rng(17)
    strains = np.array(shapes.strains[1200][1][:50] + shapes.strains[200][1][:50], np.int32)
    n = 3000
    vals = rng.choice(_metamers(rng, 1200), size=n)                                      # ~2.5 records per value: groups form across inputs
    tids = rng.choice(strains, size=n)
    if case == "a_below_b":
        cut = np.median(vals)
        parts = [vals < cut, vals >= cut]
    elif case == "single_entry":
        one = np.zeros(n, bool); one[rng.integers(n)] = True
        parts = [~one, one]
    elif case == "one_db":
        parts = [np.ones(n, bool)]
    else:
        k = 8 if case == "eight" else 5
        to = rng.integers(0, k, n)
        to[(to == 2) & (vals > np.quantile(vals, 0.3))] = 3                               # input 2 lives in the lowest values only: later ranges merge an odd number of lists
        parts = [to == j for j in range(k)]
    dbs = [_write_db(ctx, shapes.dir, vals[m], tids[m], str(tmp_path / f"in{j}"), 16) for j, m in enumerate(parts)]
    ref = _in_memory(ctx, dbs, shapes.dir, str(tmp_path / "ref"), 16)
    ev, ei, _ = spec_finish(vals, tids, shapes.dir)
    for mrr in (0, 900):
        out = str(tmp_path / f"out{mrr}"); os.makedirs(out)
        st = ctx.merge_databases(dbs, shapes.dir, _params(), out, split_num=16, max_range_records=mrr)
        assert st["n_resorted_slices"] == 0 and (st["n_ranges"] > 1) == (mrr != 0)
        _same_files(out, ref)
        gv, gi = _download(ctx, out, shapes.dir)
        assert len(gv) == len(ev) and (gv == ev).all() and (gi == ei).all()


# ---------------------------------------------------------------------------------------------------------------------
# 4. an input that is out of order under the merge's taxonomy
# ---------------------------------------------------------------------------------------------------------------------
def test_input_out_of_order_under_the_merges_taxonomy(ctx, shapes, tmp_path):
    """A is built under T1.  T2 = T1 with one strain of the 2-strain species moved under the 15-strain species, whose id is larger than the
    3-strain species' id: a value that carries this strain and a strain of the 3-strain species is stored (moved strain, other strain) in A
    and sorts the other way round under T2."""
    from build_spec import spec_finish
    sp2, st2 = shapes.strains[2]; sp3, st3 = shapes.strains[3]; sp15, _ = shapes.strains[15]
    assert sp2 < sp3 < sp15
    moved = st2[0]
    t2 = str(tmp_path / "t2")
    shapes.write(t2)
    nodes = open(os.path.join(t2, "nodes.dmp")).read()
    old, new = f"{moved}\t|\t{sp2}\t|", f"{moved}\t|\t{sp15}\t|"
    assert nodes.count("\n" + old) == 1
    open(os.path.join(t2, "nodes.dmp"), "w").write(nodes.replace("\n" + old, "\n" + new))
    rng = np.random.default_rng(23)
    strains = np.array(shapes.strains[1200][1][:30] + st2 + st3, np.int32)
    pool = _metamers(rng, 2501)
    vals = np.concatenate([pool[:2500], [pool[2500], pool[2500]]]).astype(np.uint64)
    tids = np.concatenate([rng.choice(strains, size=2500), [moved, st3[1]]]).astype(np.int32)
    a = _write_db(ctx, shapes.dir, vals, tids, str(tmp_path / "a"), 16)
    ai = np.fromfile(os.path.join(a, "info"), dtype=np.uint32)
    at = int(np.flatnonzero(ai == moved)[-1])
    assert ai[at + 1] == st3[1]                                                           # the pair, in T1's order
    other = _write_db(ctx, shapes.dir, pool[:500], rng.choice(strains, size=500), str(tmp_path / "b"), 16)
    for dbs, tag in (([a], "one"), ([a, other], "two")):
        ref = _in_memory(ctx, dbs, t2, str(tmp_path / ("ref_" + tag)), 16)
        for mrr in (0, 1000):
            out = str(tmp_path / f"out_{tag}{mrr}"); os.makedirs(out)
            st = ctx.merge_databases(dbs, t2, _params(), out, split_num=16, max_range_records=mrr)
            assert st["n_resorted_slices"] >= 1
            _same_files(out, ref)
    ev, ei, _ = spec_finish(vals, tids, t2)
    gv, gi = _download(ctx, str(tmp_path / "out_one0"), t2)
    assert (gv == ev).all() and (gi == ei).all()


# ---------------------------------------------------------------------------------------------------------------------
# 5. a legacy input
# ---------------------------------------------------------------------------------------------------------------------
def _copy_db(src, dst):
    os.makedirs(dst)
    for name in ALL_FILES:
        open(os.path.join(dst, name), "wb").write(open(os.path.join(src, name), "rb").read())
    return dst


def test_legacy_input(ctx, dealt, tmp_path):
    """Skip_redundancy 0 and bit 31 set on a third of the info entries: merged as if the bit were clear"""
    leg = _copy_db(dealt.dbs[0], str(tmp_path / "legacy"))
    info = np.fromfile(os.path.join(leg, "info"), dtype=np.uint32)
    flagged = np.random.default_rng(5).random(len(info)) < 0.33
    assert flagged.sum() > 100
    (info | (flagged.astype(np.uint32) << np.uint32(31))).astype(np.uint32).tofile(os.path.join(leg, "info"))
    txt = open(os.path.join(leg, "db.parameters")).read().replace("Skip_redundancy\t1", "Skip_redundancy\t0")
    assert "Skip_redundancy\t0" in txt
    open(os.path.join(leg, "db.parameters"), "w").write(txt)
    for mrr in (0, 1500):
        out = str(tmp_path / f"out{mrr}"); os.makedirs(out)
        ctx.merge_databases([leg] + dealt.dbs[1:], dealt.sh.dir, _params(), out, split_num=64, max_range_records=mrr)
        _same_files(out, dealt.ref[64])


# ---------------------------------------------------------------------------------------------------------------------
# 6. refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals(ctx, dealt, tmp_path):
    import metabuli_amd as M
    out = str(tmp_path / "out"); os.makedirs(out)
    stale = os.path.join(out, "db.parameters")

    def refused(dbs, params, status, **kw):
        open(stale, "w").write("DB_name\tstale\n")                                       # a database that was here before must not survive a failed merge
        with pytest.raises(M.MtbError) as e:
            ctx.merge_databases(dbs, dealt.sh.dir, params, out, split_num=64, **kw)
        assert e.value.status == status, str(e.value)
        assert not os.path.exists(stale)
        return str(e.value)

    refused(dealt.dbs, M.default_params(seq_mode=1, syncmer=0), M.MTB_ERR_ARG)              # the inputs say Syncmer 1
    bad = _copy_db(dealt.dbs[1], str(tmp_path / "bad"))
    info = np.fromfile(os.path.join(bad, "info"), dtype=np.uint32)
    info[len(info) // 2] = 777777
    info.tofile(os.path.join(bad, "info"))
    for mrr in (0, 1500):
        assert "777777" in refused([dealt.dbs[0], bad], _params(), M.MTB_ERR_ARG, max_range_records=mrr)
    msg = refused(dealt.dbs, _params(), M.MTB_ERR_CAPACITY, max_range_records=10)
    need = re.search(r"room for (\d+) records", msg)
    assert need and int(need.group(1)) > 10
    refused([], _params(), M.MTB_ERR_ARG)
    # and the directory still takes a good merge afterwards
    ctx.merge_databases(dealt.dbs, dealt.sh.dir, _params(), out, split_num=64, max_range_records=int(need.group(1)))
    _same_files(out, dealt.ref[64])


# ---------------------------------------------------------------------------------------------------------------------
# 7. mtb_build --max-records
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


def _write_fasta(path, world, which, mapf):
    with open(path, "w") as f, open(mapf, "w") as m:
        for i in which:
            tid, g = world.genomes[i]
            s = bytes(g).decode()
            f.write(f">seq{i}.1 some description\n")
            for k in range(0, len(s), 70):
                f.write(s[k:k + 70] + "\n")
            m.write(f"seq{i}.1\t{tid}\n")


def test_mtb_build_max_records(orc, tmp_path):
    from helpers import build_toy_db, default_params
    from metabuli_amd import synth
    world = synth.make_world(seed=11, n_genera=3, species_per_genus=2, strains_per_species=2, genome_len=20000)
    n = len(world.genomes)
    assert n == 12
    toy = str(tmp_path / "toy"); os.makedirs(toy)
    build_toy_db(orc, world, default_params(seq_mode=1, syncmer=1, kmer_format=2), toy)
    taxdir = os.path.join(toy, "taxonomy")
    exe = _build_program(tmp_path)
    flags = ["--syncmer", "1", "--kmer-format", "2"]
    fa, mp = str(tmp_path / "all.fa"), str(tmp_path / "all.tsv")
    _write_fasta(fa, world, range(n), mp)

    def run(out, args):
        r = subprocess.run([exe] + flags + args + [taxdir, out], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        return r.stderr.strip().split("\n")[-1]

    plain = str(tmp_path / "plain")
    closing = run(plain, [fa, mp])
    assert "parts" not in closing
    n_rec = int(re.search(r"(\d+) records", closing).group(1))
    spilled = str(tmp_path / "spilled")
    closing = run(spilled, ["--max-records", str(n_rec // 8), fa, mp])
    m = re.search(r"in (\d+) parts, (\d+) ranges", closing)
    assert m and int(m.group(1)) >= 3, closing
    assert f"{n_rec} records" in closing
    _same_files(spilled, plain)
    _same_files(spilled, toy, DB_FILES)
    assert not os.path.exists(os.path.join(spilled, "tmp_parts"))
    assert os.path.exists(os.path.join(spilled, "taxonomy", "nodes.dmp"))
    # --add-db of half the genomes (never enters a builder on the spilled route) + the other half as FASTA
    fa1, mp1, fa2, mp2 = str(tmp_path / "h1.fa"), str(tmp_path / "h1.tsv"), str(tmp_path / "h2.fa"), str(tmp_path / "h2.tsv")
    _write_fasta(fa1, world, range(0, n // 2), mp1); _write_fasta(fa2, world, range(n // 2, n), mp2)
    half1, half2 = str(tmp_path / "half1"), str(tmp_path / "half2")
    run(half1, [fa1, mp1]); run(half2, [fa2, mp2])
    updated = str(tmp_path / "updated")
    closing = run(updated, ["--max-records", str(n_rec // 8), "--add-db", half1, fa2, mp2])
    assert re.search(r"in (\d+) parts, (\d+) ranges", closing), closing
    _same_files(updated, plain)
    # the pure merge always streams
    merged = str(tmp_path / "merged")
    closing = run(merged, ["--add-db", half1, "--add-db", half2, "-", "-"])
    assert re.search(r"(\d+) ranges", closing), closing
    _same_files(merged, plain)
