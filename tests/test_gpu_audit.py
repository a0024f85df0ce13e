"""GPU tests of the database audit (mtb_database_audit, mtb_audit_write_species_counts; kernels_audit.h, host/audit_plan.h, the chunk
sink of decode_chunked): a ~20 000-entry database written through the oracle and then byte-edited, every case compared field by
field (times and n_chunks excepted) and count by count with the numpy restatement of tests/audit_spec.py; then the databases the
library itself writes, and the two programs."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import audit_spec as A

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = 4096                                   # words per forced chunk: the base database spans ~20 of them
N_DISTINCT, N_SHARED = 19000, 1000             # values; of these, values filed under a second species too
DB_FILES = ("diffIdx", "info", "split", "taxID_list", "db.parameters")


@pytest.fixture(scope="module")
def ctx():
    import metabuli_amd as M
    c = M.Context(0)
    yield c
    c.close()


def _metamers(rng, n):
    """n distinct format-2 words (eight amino-acid letters 0..20 above 24 DNA bits), ascending, none below 2^24"""
    letters = rng.integers(0, 21, size=(int(n * 1.2) + 64, 8)).astype(np.uint64)
    v = rng.integers(0, 1 << 24, size=len(letters)).astype(np.uint64)
    for k in range(8):
        v |= letters[:, k] << np.uint64(24 + 5 * k)
    v = np.unique(v)
    v = v[v >= np.uint64(1 << 24)]
    return np.sort(rng.choice(v, size=n, replace=False))


class Base:
    """the toy world's taxonomy, ~20 000 entries in (value, species) order -- one species owns more than 60 % of them, one exactly
    one --, the files as the oracle writes them (split_num 12), the taxonomy as the spec's tables"""

    def __init__(self, orc, d):
        from helpers import default_params
        from metabuli_amd import synth
        self.world = w = synth.make_world(seed=21, n_genera=3, species_per_genus=3, strains_per_species=2, genome_len=3000)
        self.p = default_params(seq_mode=1, syncmer=1)
        rng = np.random.default_rng(5)
        strains = {}                                                                     # species -> its strains
        for t, par in w.tax.parent.items():
            if w.tax.rank[t] == "no rank" and t != 1:
                strains.setdefault(par, []).append(t)
        self.species = sorted(strains)
        self.strains = strains
        self.big, self.lone = self.species[4], self.species[7]
        rest = [s for s in self.species if s not in (self.big, self.lone)]
        vals = _metamers(rng, N_DISTINCT)
        sp = np.where(rng.random(N_DISTINCT) < 0.66, self.big, rng.choice(rest, size=N_DISTINCT)).astype(np.int64)
        sp[N_DISTINCT // 3] = self.lone
        shared = rng.choice(np.flatnonzero(sp != self.lone), size=N_SHARED, replace=False)
        sp2 = np.where(sp[shared] == self.big, rng.choice(rest, size=N_SHARED), self.big)
        vals = np.concatenate([vals, vals[shared]]); sp = np.concatenate([sp, sp2])
        order = np.lexsort((sp, vals))
        self.values, sp = vals[order], sp[order]
        self.taxids = np.array([strains[int(s)][int(k)] for s, k in zip(sp, rng.integers(0, 2, size=len(sp)))], np.int32)
        self.n = len(self.values)
        self.dir = str(d)
        w.tax.write(os.path.join(self.dir, "taxonomy"))
        orc.write_db(self.dir, self.values, self.taxids, self.p, split_num=12)
        self.files = {f: open(os.path.join(self.dir, f), "rb").read() for f in DB_FILES}
        assert (sp == self.big).mean() >= 0.6 and (sp == self.lone).sum() == 1
        self.entry_species = sp
        self.unlisted_genus = w.tax.parent[self.big]                                     # known, not in taxID_list, no species
        self.unknown_id = max(w.tax.parent) + 7

    def listed(self, d=None):
        return [int(x) for x in open(os.path.join(d or self.dir, "taxID_list")).read().split()]

    def tables(self, listed, max_id=None, extra_nodes=()):
        tax = self.world.tax
        parent, rank = dict(tax.parent), dict(tax.rank)
        for t, par, r in extra_nodes:
            parent[t] = par; rank[t] = r
        return A.taxonomy_tables(parent, rank, listed, max_id=max_id)


@pytest.fixture(scope="module")
def base(orc, tmp_path_factory):
    return Base(orc, tmp_path_factory.mktemp("audit_base"))


def _copy(base, d, **edits):
    """the base database in directory d with files replaced (bytes) or removed (None)"""
    d = str(d)
    os.makedirs(d, exist_ok=True)
    shutil.copytree(os.path.join(base.dir, "taxonomy"), os.path.join(d, "taxonomy"), dirs_exist_ok=True)
    for f in DB_FILES:
        data = edits.get(f.replace(".", "_"), base.files[f])
        if data is not None:
            open(os.path.join(d, f), "wb").write(data)
    return d


def _resplit(split_bytes, d16):
    """the split table with every record's word offset and value taken from the words as they are now (info_off kept): an edit that
    changes word counts must not move the checkpoints off their entries"""
    spl = np.frombuffer(split_bytes, np.uint64).reshape(-1, 3).copy()
    values, ends = A.decode_words(d16)
    for r in range(len(spl)):
        io = int(spl[r, 2])
        if spl[r, 0] != 0 and 1 <= io <= len(ends):
            spl[r, 0] = values[io - 1]; spl[r, 1] = ends[io - 1] + 1
    return spl.tobytes()


def _spec(d, base, info_mask=0xFFFFFFFF, tables=None):
    rd = lambda f: open(os.path.join(d, f), "rb").read()
    listed = base.listed(d)
    species, known = tables if tables is not None else base.tables(listed)
    return A.audit(rd("diffIdx"), rd("info"), rd("split"), species, known, listed, info_mask)


def _check(ctx, d, base, chunk_words=CHUNK, info_mask=0xFFFFFFFF, tables=None, params=None, taxonomy_dir=None):
    """audit `d` on the device and by the spec: every field but the times and n_chunks, and every count"""
    want, want_counts = _spec(d, base, info_mask, tables)
    rep, counts = ctx.audit_database(d, taxonomy_dir=taxonomy_dir, params=params, chunk_words=chunk_words)
    got = {k: rep[k] for k in A.REPORT_FIELDS}
    assert got == want, {k: (got[k], want[k]) for k in got if got[k] != want[k]}
    assert counts.dtype == np.uint32 and len(counts) == len(want_counts) and (counts == want_counts).all()
    return rep, counts


def _boundaries(d16):
    """per forced chunk boundary: the last entry whose end word lies before word CHUNK * k (the last entry of chunk k - 1; the next
    entry is the first of chunk k) -- from the spec's end-word positions"""
    _, ends = A.decode_words(d16)
    return [int(np.searchsorted(ends, CHUNK * k, side="left")) - 1 for k in range(1, (len(d16) - 1) // CHUNK + 1)]


# ---------------------------------------------------------------------------------------------------------------------
# the sound database
# ---------------------------------------------------------------------------------------------------------------------
def test_untouched_database_is_canonical(ctx, base):
    rep, counts = _check(ctx, base.dir, base)
    assert rep["valid"] == 1 and rep["canonical"] == 1
    assert rep["n_entries"] == base.n and rep["n_checkpoints"] >= 8 and rep["n_bad_checkpoints"] == 0
    assert rep["n_chunks"] >= 8                                                          # the file spans several chunks
    assert (counts == np.bincount(base.entry_species, minlength=len(counts))).all()
    assert counts[base.big] >= 0.6 * base.n and counts[base.lone] == 1


def test_species_count_file(ctx, base, tmp_path):
    import metabuli_amd as M
    d = _copy(base, tmp_path / "db")
    _, counts = ctx.audit_database(d, chunk_words=CHUNK)
    M.write_species_counts(d, counts)
    text = open(os.path.join(d, "sp2uniqKmerCnt")).read()
    _, want = _spec(d, base)
    assert text == A.species_counts_text(want)
    assert (A.parse_species_counts(text, len(want)) == want).all()                       # read back with the reference's grammar


@pytest.mark.parametrize("chunk_words", [0, 1 << 22])
def test_one_chunk_gives_the_same_report(ctx, base, chunk_words):
    rep, _ = _check(ctx, base.dir, base, chunk_words=chunk_words)
    assert rep["n_chunks"] == 1 and rep["canonical"] == 1


# ---------------------------------------------------------------------------------------------------------------------
# counts that disagree
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["info_short", "info_long", "trailing_words"])
def test_counts_that_disagree(ctx, base, tmp_path, case):
    if case == "info_short":
        d = _copy(base, tmp_path / "db", info=base.files["info"][:-4])
    elif case == "info_long":
        d = _copy(base, tmp_path / "db", info=base.files["info"] + base.files["info"][:4])
    else:
        d = _copy(base, tmp_path / "db", diffIdx=base.files["diffIdx"] + np.array([0x0123, 0x0456], np.uint16).tobytes())
    rep, _ = _check(ctx, d, base)
    assert rep["valid"] == 0
    assert rep["n_trailing_words"] == (2 if case == "trailing_words" else 0)
    assert rep["n_entries"] == (base.n - 1 if case == "info_short" else base.n)


# ---------------------------------------------------------------------------------------------------------------------
# order: a wrapped delta, a repeated entry, descending species -- at entry 1, at the last entry and on both sides of every chunk boundary
# ---------------------------------------------------------------------------------------------------------------------
def _edit_order(base, kind, at):
    """(values, info) with the defect `kind` at every entry of `at` (entries >= 1; runs of neighbours allowed)"""
    v, t = base.values.copy(), base.taxids.copy()
    hi = sorted(base.species, reverse=True)
    for i in sorted(at):
        if kind == "descent":
            v[i] = v[i - 1] - np.uint64(1)
        elif kind == "repeat":
            v[i] = v[i - 1]; t[i] = t[i - 1]
        else:                                                                            # equal values, species descending
            v[i] = v[i - 1]
            if i - 1 not in at:
                t[i - 1] = base.strains[hi[0]][0]
            below = [s for s in hi if s < base.world.tax.parent[int(t[i - 1])]]
            t[i] = base.strains[below[0]][0]
    return v, t


def _place_at_boundaries(base, kind):
    """the defect at entry 1, at the last entry and at the last entry of chunk k / the first of chunk k + 1 for every boundary of the
    EDITED file (an edit changes word counts and so moves the boundaries at and behind it: they are settled from left to right)"""
    at = {1, base.n - 1}
    k = 0
    while True:
        bounds = _boundaries(A.encode_values(_edit_order(base, kind, at)[0]))
        if k >= len(bounds):
            break
        if bounds[k] in at and bounds[k] + 1 in at:
            k += 1                                                                       # settled: edits further right do not move it
        else:
            at |= {bounds[k], bounds[k] + 1}                                             # (an edit that moves the boundary leaves a defect next to it)
        assert len(at) < 400
    v, t = _edit_order(base, kind, at)
    d16 = A.encode_values(v)
    for b in _boundaries(d16):                                                           # what the case is about
        assert b in at and b + 1 in at
    return v, t, d16, at


@pytest.mark.parametrize("kind", ["descent", "repeat", "species_descending"])
def test_order_defects_at_chunk_edges(ctx, base, tmp_path, kind):
    v, t, d16, at = _place_at_boundaries(base, kind)
    d = _copy(base, tmp_path / "db", diffIdx=d16.tobytes(), info=t.astype(np.uint32).tobytes(), split=_resplit(base.files["split"], d16))
    rep, _ = _check(ctx, d, base)
    assert rep["n_chunks"] >= 8 and rep["n_bad_checkpoints"] == 0 and rep["n_checkpoints"] >= 8
    if kind == "descent":
        assert rep["valid"] == 0 and rep["n_value_descents"] == len(at) and rep["first_value_descent"] == 1
    else:
        assert rep["valid"] == 1 and rep["canonical"] == 0 and rep["n_value_descents"] == 0
        assert rep["n_group_disorder"] >= len(at) and rep["first_group_disorder"] == 1


# ---------------------------------------------------------------------------------------------------------------------
# ids
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["unknown", "unlisted", "ancestor"])
def test_ids_against_the_taxonomy(ctx, base, tmp_path, case):
    t = base.taxids.astype(np.uint32)
    listed = base.listed()
    if case == "unknown":
        t[[777, 9000]] = base.unknown_id
    elif case == "unlisted":                                                             # a strain the taxonomy knows and taxID_list does not name
        used = int(base.taxids[base.entry_species == base.lone][0])
        victim = [x for x in base.strains[base.lone] if x != used][0]                    # the lone species' other strain: in no entry
        listed = [x for x in listed if x != victim]
        t[[5, 4200, 4201]] = victim
    else:                                                                                # a genus: known, unlisted, no species
        t[[CHUNK, 15000]] = base.unlisted_genus
    d = _copy(base, tmp_path / "db", info=t.tobytes(), taxID_list="".join(f"{x}\n" for x in listed).encode())
    rep, _ = _check(ctx, d, base)
    if case == "unknown":
        assert rep["valid"] == 0 and rep["n_unknown_ids"] == 2 and rep["first_unknown_id"] == 777
    elif case == "unlisted":
        assert rep["valid"] == 1 and rep["canonical"] == 0 and rep["n_unlisted_ids"] == 3 and rep["first_unlisted_id"] == 5
    else:
        assert rep["n_no_species"] == 2 and rep["n_unlisted_ids"] == 2 and rep["canonical"] == 0


def test_legacy_database_bit_31_is_masked(ctx, base, tmp_path):
    t = base.taxids.astype(np.uint32)
    t[::3] |= np.uint32(1 << 31)
    par = base.files["db.parameters"].replace(b"Skip_redundancy\t1", b"Skip_redundancy\t0")
    assert par != base.files["db.parameters"]
    d = _copy(base, tmp_path / "db", info=t.tobytes(), db_parameters=par)
    import metabuli_amd as M
    rep, counts = _check(ctx, d, base, info_mask=0x7FFFFFFF, params=M.default_params(skip_redundancy=0))
    assert rep["valid"] == 1 and rep["n_unknown_ids"] == 0
    assert (counts == np.bincount(base.entry_species, minlength=len(counts))).all()


def test_large_taxonomy(ctx, base, tmp_path):
    """a taxonomy whose largest id is about 3 000 000: the bin array of a real database"""
    far_species, far_strain = 2999990, 3000000
    d = _copy(base, tmp_path / "db")
    with open(os.path.join(d, "taxonomy", "nodes.dmp"), "a") as f:
        f.write(f"{far_species}\t|\t{base.world.tax.parent[base.big]}\t|\tspecies\t|\t\t|\n{far_strain}\t|\t{far_species}\t|\tno rank\t|\t\t|\n")
    with open(os.path.join(d, "taxonomy", "names.dmp"), "a") as f:
        f.write(f"{far_species}\t|\tfar species\t|\t\t|\tscientific name\t|\n{far_strain}\t|\tfar strain\t|\t\t|\tscientific name\t|\n")
    t = base.taxids.astype(np.uint32)
    moved = np.flatnonzero(base.entry_species == base.species[0])                        # one species' entries move to the far one
    t[moved] = far_strain
    listed = base.listed() + [far_strain]
    open(os.path.join(d, "info"), "wb").write(t.tobytes())
    open(os.path.join(d, "taxID_list"), "w").write("".join(f"{x}\n" for x in listed))
    extra = [(far_species, base.world.tax.parent[base.big], "species"), (far_strain, far_species, "no rank")]
    rep, counts = _check(ctx, d, base, tables=base.tables(listed, extra_nodes=extra))
    assert len(counts) == far_strain + 1 and counts[far_species] == len(moved) and rep["valid"] == 1


# ---------------------------------------------------------------------------------------------------------------------
# checkpoints
# ---------------------------------------------------------------------------------------------------------------------
def _split(base):
    return np.frombuffer(base.files["split"], np.uint64).reshape(-1, 3).copy()


@pytest.mark.parametrize("case", ["info_off_plus_one", "wrong_ad", "inside_an_entry", "two_bad", "all_zero"])
def test_checkpoints(ctx, base, tmp_path, case):
    spl = _split(base)
    use = A.usable_checkpoints(spl, base.n, len(base.files["diffIdx"]) // 2)
    assert len(use) >= 8
    bad = []
    if case == "info_off_plus_one":
        spl[use[2], 2] += 1; bad = [use[2]]
    elif case == "wrong_ad":
        spl[use[3], 0] ^= np.uint64(1); bad = [use[3]]                                   # (the DNA part: the amino-acid order of the records stays)
    elif case == "inside_an_entry":
        _, ends = A.decode_words(np.frombuffer(base.files["diffIdx"], np.uint16))
        e = int(spl[use[4], 2])                                                          # the entry behind the checkpoint has several words
        assert ends[e] - ends[e - 1] >= 2
        spl[use[4], 1] += 1; bad = [use[4]]
    elif case == "two_bad":
        spl[use[1], 2] -= 1; spl[use[6], 0] += np.uint64(2); bad = [use[1], use[6]]
    else:
        spl[:] = 0
    d = _copy(base, tmp_path / "db", split=spl.tobytes())
    rep, _ = _check(ctx, d, base)
    if case == "all_zero":
        assert rep["n_checkpoints"] == 0 and rep["valid"] == 1 and rep["canonical"] == 1
    else:
        assert rep["n_bad_checkpoints"] == len(bad) and rep["first_bad_checkpoint"] == bad[0] and rep["valid"] == 0


# ---------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------
def _status(ctx, d, counts_cap=None, taxonomy_dir=None):
    import ctypes as C
    import metabuli_amd as M
    r = M.AuditReport()
    p = M.default_params()
    arr = np.full(max(counts_cap or 1, 1), 0xABCD, np.uint32)
    st = ctx.L.mtb_database_audit(ctx.h, d.encode(), taxonomy_dir.encode() if taxonomy_dir else None, C.byref(p), C.c_uint64(CHUNK),
                                  arr.ctypes.data_as(C.c_void_p) if counts_cap is not None else None, C.c_uint64(counts_cap or 0), C.byref(r))
    return st, ctx.L.mtb_last_error().decode(), arr


def test_cap_too_small(ctx, base):
    import metabuli_amd as M
    need = max(base.world.tax.parent) + 1
    st, msg, arr = _status(ctx, base.dir, counts_cap=need - 1)
    assert st == M.MTB_ERR_CAPACITY and str(need) in msg and (arr == 0xABCD).all()       # the size needed is named, nothing is written
    st, _, _ = _status(ctx, base.dir, counts_cap=need)
    assert st == M.MTB_OK


@pytest.mark.parametrize("case,needle", [("no_diffIdx", "\"diffIdx\" file is missing"), ("no_info", "\"info\" file is missing"), ("no_split", "\"split\" file is missing"),
                                         ("no_taxID_list", "\"taxID_list\" file is missing"), ("no_taxonomy", "taxonomy"), ("empty_diffIdx", "diffIdx file is empty"),
                                         ("empty_info", "info file is empty"), ("odd_diffIdx", "diffIdx file size is not a multiple of 2"),
                                         ("odd_info", "info file size is not a multiple of 4")])
def test_file_problems(ctx, base, tmp_path, case, needle):
    import metabuli_amd as M
    kind, _, f = case.partition("_")
    if case == "no_taxonomy":
        d = _copy(base, tmp_path / "db")
        shutil.rmtree(os.path.join(d, "taxonomy"))
    elif kind == "no":
        d = _copy(base, tmp_path / "db", **{f: None})
    elif kind == "empty":
        d = _copy(base, tmp_path / "db", **{f: b""})
    else:
        d = _copy(base, tmp_path / "db", **{f: base.files[f] + b"\x00"})
    st, msg, _ = _status(ctx, d)
    assert st == M.MTB_ERR_IO and needle in msg, msg


def test_reduced_alphabet_is_refused(ctx, base, tmp_path):
    import metabuli_amd as M
    par = base.files["db.parameters"].replace(b"Reduced_alphabet\t0", b"Reduced_alphabet\t1")
    assert par != base.files["db.parameters"]
    st, msg, _ = _status(ctx, _copy(base, tmp_path / "db", db_parameters=par))
    assert st == M.MTB_ERR_UNSUPPORTED and "Reduced_alphabet" in msg


# ---------------------------------------------------------------------------------------------------------------------
# what the library writes audits canonical
# ---------------------------------------------------------------------------------------------------------------------
def test_builder_and_merge_outputs_are_canonical(ctx, base, tmp_path):
    import metabuli_amd as M
    taxdir = os.path.join(base.dir, "taxonomy")
    p = M.default_params(seq_mode=1, syncmer=1)
    halves = []
    for k in range(2):
        b = ctx.builder(taxdir, p)
        b.add_records(base.values[k::2], base.taxids[k::2])
        ix = b.finish()
        d = str(tmp_path / f"half{k}"); os.makedirs(d)
        ix.write(d, split_num=8)
        ix.close(); b.close()
        halves.append(d)
        rep, counts = _check(ctx, d, base, taxonomy_dir=taxdir)
        assert rep["canonical"] == 1 and rep["n_entries"] == len(base.values[k::2]) and rep["n_checkpoints"] >= 4
    out = str(tmp_path / "merged"); os.makedirs(out)
    ctx.merge_databases(halves, taxdir, p, out, split_num=12, max_range_records=6000)
    rep, counts = _check(ctx, out, base, taxonomy_dir=taxdir)
    assert rep["canonical"] == 1 and rep["n_entries"] == base.n and rep["n_checkpoints"] >= 8
    assert (counts == np.bincount(base.entry_species, minlength=len(counts))).all()


# ---------------------------------------------------------------------------------------------------------------------
# the programs
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


def _corrupt(base, d):
    """one wrapped delta in the middle of the database"""
    v = base.values.copy()
    v[base.n // 2] = v[base.n // 2 - 1] - np.uint64(1)
    d16 = A.encode_values(v)
    return _copy(base, d, diffIdx=d16.tobytes(), split=_resplit(base.files["split"], d16))


def test_mtb_classify_validate_db(base, tmp_path):
    from metabuli_amd import synth
    _, classify_exe = _programs(tmp_path)
    bases, offs, _ = synth.sample_reads(np.random.default_rng(3), base.world, 40, length=150, err=0.01)
    fq = str(tmp_path / "reads.fq")
    with open(fq, "w") as f:
        for i in range(len(offs) - 1):
            s = bytes(bases[int(offs[i]):int(offs[i + 1])]).decode()
            f.write(f"@r{i}\n{s}\n+\n{'I' * len(s)}\n")
    rows = []
    for flags in ([], ["--validate-db", "1"]):
        od = tmp_path / ("out%d" % len(flags)); od.mkdir()
        r = subprocess.run([classify_exe, "--seq-mode", "1"] + flags + [fq, base.dir, str(od), "j"], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        rows.append(open(od / "j_classifications.tsv").read())
        if flags:
            for line in ("Validating database: " + base.dir, "Check if required files exist...", "All required files are present.",
                         "Check if the k-mer count and k-mer ID count are consistent...", f"Number of k-mers in diffIdx file: {base.n}",
                         f"Number of k-mer IDs in info file: {base.n}", "Number of k-mers in diffIdx file matches the number of k-mer IDs in info file.",
                         "Database validation completed successfully."):
                assert line in r.stdout, r.stdout
            assert "accepted for compatibility" not in r.stderr
    assert rows[0] == rows[1] and rows[0].count("\n") >= 40
    bad = _corrupt(base, tmp_path / "bad")
    od = tmp_path / "out_bad"; od.mkdir()
    r = subprocess.run([classify_exe, "--seq-mode", "1", "--validate-db", "1", fq, bad, str(od), "j"], capture_output=True, text=True)
    assert r.returncode == 1 and "Database validation failed." in r.stderr and f"the first is entry {base.n // 2}" in r.stderr
    assert not os.path.exists(od / "j_classifications.tsv")                              # it ended before classifying


def test_mtb_build_audit(base, tmp_path):
    build_exe, _ = _programs(tmp_path)
    d = _copy(base, tmp_path / "db")
    taxdir = os.path.join(d, "taxonomy")
    r = subprocess.run([build_exe, "--audit", "1", "-", "-", taxdir, d], capture_output=True, text=True)
    assert r.returncode == 0 and "valid 1, canonical 1" in r.stdout, r.stdout + r.stderr
    _, want = _spec(d, base)
    assert open(os.path.join(d, "sp2uniqKmerCnt")).read() == A.species_counts_text(want)
    bad = _corrupt(base, tmp_path / "bad")
    r = subprocess.run([build_exe, "--audit", "1", "-", "-", os.path.join(bad, "taxonomy"), bad], capture_output=True, text=True)
    assert r.returncode == 1 and "Database validation failed." in r.stderr and "valid 0" in r.stdout
    # --validate-db 1 behind a merge: the output is audited and is canonical
    out = str(tmp_path / "merged")
    r = subprocess.run([build_exe, "--validate-db", "1", "--syncmer", "1", "--split-num", "12", "--add-db", d, "-", "-", taxdir, out], capture_output=True, text=True)
    assert r.returncode == 0 and "valid 1, canonical 1" in r.stdout, r.stdout + r.stderr
