"""GPU tests of the CDS-guided database build: Builder.add_blocks over the blocks tests/cds_spec.py makes of a generated annotation, and
`mtb_build --cds-info`, against the oracle's records (tests/blocks_spec.py), the numpy restatement of the sort + dedup
(tests/build_spec.py) and the oracle's database writer."""
import os
import subprocess

import numpy as np
import pytest

import blocks_spec
import cds_spec

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DB_FILES = ("diffIdx", "info", "split", "taxID_list")


@pytest.fixture(scope="module")
def ctx():
    import metabuli_amd as M
    c = M.Context(0)
    yield c
    c.close()


def _annotate(rng, acc, L):
    """headers of a cds_from_genomic file for one genome: forward, complement, joined (2 and 3 exons), frames 2 and 3, an overlap, a pseudo
    gene, a hypothetical protein; gaps below and above 32 bases; the first CDS 8 bases from the start, the last one 10 from the end"""
    out, p, k = [], 8, 0
    while p + 1000 < L - 10:
        n = 3 * int(rng.integers(100, 300))
        a, b = p + 1, p + n                                         # 1-based, inclusive
        kind = k % 9
        tags = ["gene=g%d" % k, "protein=p%d" % k]
        if kind == 1:
            loc = f"complement({a}..{b})"
        elif kind == 2:
            m = a + 3 * (n // 9)
            loc = f"join({a}..{m},{m + 40}..{b})"
        elif kind == 3:
            m1, m2 = a + 3 * (n // 12), a + 3 * (n // 5)
            loc = f"complement(join({a}..{m1},{m1 + 50}..{m2},{m2 + 35}..{b}))"
        elif kind == 4:
            tags.append("frame=2"); loc = f"<{a}..{b}"
        elif kind == 5:
            tags.append("frame=3"); loc = f"complement({a}..>{b})"
        elif kind == 6:
            loc = f"{a - 60}..{b}"                                    # overlaps the CDS before it
        elif kind == 7:
            tags.append("pseudo=true"); loc = f"{a}..{b}"
        else:
            loc = f"{a}..{b}"
        if kind == 8:
            tags[1] = "protein=hypothetical protein"
        out.append(f"lcl|{acc}_cds_P{k}.1_{k + 1} " + " ".join(f"[{t}]" for t in tags + [f"protein_id=P{k}.1", f"location={loc}", "gbkey=CDS"]))
        p += n + int(rng.integers(10, 90))
        k += 1
    out.append(f"lcl|{acc}_cds_P{k}.1_{k + 1} [protein=last] [protein_id=P{k}.1] [location={L - 400}..{L - 10}]")
    return out


class CdsWorld:
    """smoke()'s toy world with an annotation for every genome but the last"""

    def __init__(self, d):
        from metabuli_amd import synth
        self.world = synth.make_world(seed=11, n_genera=3, species_per_genus=2, strains_per_species=2, genome_len=20000)
        rng = np.random.default_rng(5)
        self.names = [f"seq{i}.1" for i in range(len(self.world.genomes))]
        self.genomes = [(n, bytes(g).decode()) for n, (_, g) in zip(self.names, self.world.genomes)]
        self.taxids = [t for t, _ in self.world.genomes]
        self.headers = [h for n, (_, s) in zip(self.names[:-1], self.genomes[:-1]) for h in _annotate(rng, n, len(s))]
        self.dir = str(d)
        self.taxdir = os.path.join(self.dir, "taxonomy")
        self.world.tax.write(self.taxdir)
        self.blocks, self.plain = cds_spec.call_arrays(self.headers, self.genomes, self.taxids)

    def oracle_records(self, orc, syncmer):
        from helpers import default_params
        b = self.blocks
        v, bo = blocks_spec.oracle_blocks(orc, syncmer, b["bases"], b["offs"], b["blocks"])
        t = b["taxids"][b["blocks"]["seq"][bo]]
        k, _, _ = orc.extract_batch(default_params(seq_mode=3, syncmer=syncmer, kmer_format=2), self.plain["bases"], self.plain["offs"])
        seq = ((k["qinfo"] >> np.uint64(32)) & np.uint64(0x1FFFFFFF)).astype(np.int64) - 1
        return np.concatenate([v, k["value"]]), np.concatenate([t, self.plain["taxids"][seq]]).astype(np.int32), len(v), len(k)


@pytest.fixture(scope="module")
def cw(tmp_path_factory):
    return CdsWorld(tmp_path_factory.mktemp("cds_world"))


def _same_files(a, b):
    for name in DB_FILES:
        x, y = open(os.path.join(a, name), "rb").read(), open(os.path.join(b, name), "rb").read()
        assert x == y, f"{name} differs ({len(x)} / {len(y)} bytes)"


def _oracle_db(orc, cw, syncmer, d):
    """the entries the spec makes of the oracle's records, written by the oracle's writer -> (directory, values, info)"""
    from build_spec import spec_finish
    from helpers import default_params
    vals, tids, n_block, n_six = cw.oracle_records(orc, syncmer)
    ev, ei, _ = spec_finish(vals, tids, cw.taxdir)
    orc.write_db(str(d), ev, ei.astype(np.int32), default_params(seq_mode=1, syncmer=syncmer, kmer_format=2))
    cw.world.tax.write(os.path.join(str(d), "taxonomy"))
    return str(d), ev, ei, len(vals), n_block, n_six


@pytest.mark.parametrize("syncmer", [0, 1], ids=["dense", "syncmer"])
def test_add_blocks_builds_the_oracles_database(ctx, orc, cw, tmp_path, syncmer):
    import metabuli_amd as M
    odir, ev, ei, n_rec, n_block, n_six = _oracle_db(orc, cw, syncmer, tmp_path / "oracle")
    kinds = cw.blocks["blocks"]
    assert (kinds["strand"] < 0).sum() > 10 and (kinds["seq"] >= len(cw.genomes) - 1).sum() > 10 and n_block > 10000 and n_six > 1000
    b = ctx.builder(cw.taxdir, M.default_params(seq_mode=1, syncmer=syncmer))
    b.add_blocks(cw.blocks["bases"], cw.blocks["offs"], cw.blocks["taxids"], cw.blocks["blocks"])
    assert b.num_records == n_block
    b.add_sequences(cw.plain["bases"], cw.plain["offs"], cw.plain["taxids"])
    assert b.num_records == n_rec
    ix = b.finish()
    gv, gi = ix.download()
    assert len(gv) == len(ev) and (gv == ev).all() and (gi == ei).all()
    out = tmp_path / "written"; out.mkdir()
    ix.write(str(out))
    _same_files(str(out), odir)
    ix.close(); b.close()


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


def test_mtb_build_with_cds_info(orc, cw, tmp_path):
    build_exe, classify_exe = _programs(tmp_path)
    odir, ev, ei, n_rec, n_block, n_six = _oracle_db(orc, cw, 1, tmp_path / "oracle")
    fa, mp, cds, lst = (str(tmp_path / n) for n in ("all.fa", "all.tsv", "cds_from_genomic.fna", "cds.list"))
    with open(fa, "w") as f, open(mp, "w") as m:
        for (name, s), t in zip(cw.genomes, cw.taxids):
            f.write(f">{name} some description\n")
            for k in range(0, len(s), 70):
                f.write(s[k:k + 70] + "\n")
            m.write(f"{name}\t{t}\n")
    with open(cds, "w") as f:
        for h in cw.headers:
            f.write(f">{h}\nATGAAATAA\n")
    open(lst, "w").write(cds + "\n")
    out = str(tmp_path / "out")
    r = subprocess.run([build_exe, "--syncmer", "1", "--kmer-format", "2", "--cds-info", lst, fa, mp, cw.taxdir, out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    _same_files(out, odir)
    n = len(cw.genomes)
    assert f"{n} sequences" in r.stderr and f"{n_rec} records" in r.stderr
    assert f"{n - 1} sequences by blocks" in r.stderr and "1 sequences without a CDS entry in six frames" in r.stderr
    assert "Mask_mode\t1" not in open(os.path.join(out, "db.parameters")).read()
    # a --cds-info build in the legacy format is refused
    r1 = subprocess.run([build_exe, "--kmer-format", "1", "--cds-info", lst, fa, mp, cw.taxdir, str(tmp_path / "out1")], capture_output=True, text=True)
    assert r1.returncode != 0 and "--kmer-format 2" in r1.stderr
    # reads drawn from CDS of the annotated genomes classify, and as on the oracle-written database
    cdsmap, _ = cds_spec.parse_annotation(cw.headers)
    rng = np.random.default_rng(9)
    reads = []
    for gi_ in range(0, n - 1, 2):
        s = cw.genomes[gi_][1]
        for e in cdsmap[cw.names[gi_]]:
            if len(e["loc"]) == 1 and e["loc"][0][1] - e["loc"][0][0] > 300 and len(reads) < 60:
                a = int(rng.integers(e["loc"][0][0] - 1, e["loc"][0][1] - 150))
                reads.append((cw.taxids[gi_], s[a:a + 150]))
    assert len(reads) >= 40
    fq = str(tmp_path / "reads.fq")
    with open(fq, "w") as f:
        for i, (_, s) in enumerate(reads):
            f.write(f"@r{i}\n{s}\n+\n{'I' * len(s)}\n")
    rows = []
    for db in (out, odir):
        od = tmp_path / ("cls_" + os.path.basename(db)); od.mkdir()
        subprocess.check_call([classify_exe, "--seq-mode", "1", fq, db, str(od), "j"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        rows.append(open(od / "j_classifications.tsv").read())
    assert rows[0] == rows[1]
    lines = [l.split("\t") for l in rows[0].strip().split("\n")[1:]]
    assert len(lines) == len(reads)
    tax = cw.world.tax
    n_right = sum(1 for l, (t, _) in zip(lines, reads) if l[0] == "1" and int(l[2]) in tax.lineage(t))
    assert n_right >= 0.9 * len(reads), (n_right, len(reads))
