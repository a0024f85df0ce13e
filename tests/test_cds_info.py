"""CDS annotation -> blocks: metabuli_amd/csrc/host/cds_info.h (through tests/emu/cds_dump.cpp, a stand-alone program) against the Python
restatement tests/cds_spec.py on generated annotation, and against values worked out by hand."""
import os
import subprocess

import numpy as np
import pytest

import cds_spec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cds_dump(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("cds_dump") / "cds_dump")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "emu", "cds_dump.cpp"), "-lz"])
    return exe


def _genome(rng, L):
    return rng.choice(np.frombuffer(b"ACGT", np.uint8), size=L).tobytes().decode()


def _rec(acc, k, tags):
    return f"lcl|{acc}_cds_P{k}.1_{k} " + " ".join(f"[{t}]" for t in tags)


def _world():
    """three annotated genomes, one whose annotation carries a two-digit version (so it does not match), one without annotation"""
    rng = np.random.default_rng(77)
    genomes = [("NC_000001.1", _genome(rng, 3000)), ("NZ_AB12.2", _genome(rng, 1000)), ("NC_000003.12", _genome(rng, 800)), ("plain.1", _genome(rng, 500)),
               ("NC_000005.1", _genome(rng, 400))]
    g1 = [
        _rec("NC_000001.1", 1, ["gene=a", "protein=alpha", "protein_id=P1.1", "location=100..402", "gbkey=CDS"]),                    # forward
        _rec("NC_000001.1", 2, ["protein=beta", "protein_id=P2.1", "location=complement(500..799)"]),                               # complement
        _rec("NC_000001.1", 3, ["protein_id=P3.1", "location=join(900..1000,1100..1222)"]),                                         # two exons
        _rec("NC_000001.1", 4, ["protein_id=P4.1", "location=complement(join(1300..1350,1400..1450,1500..1591))"]),                 # three, complement
        _rec("NC_000001.1", 5, ["protein=gamma", "frame=2", "protein_id=P5.1", "location=<1700..1800"]),                            # frame 2 forward, '<'
        _rec("NC_000001.1", 6, ["frame=3", "protein_id=P6.1", "location=complement(1850..>1990)"]),                                 # frame 3 complement, '>'
        _rec("NC_000001.1", 7, ["protein_id=P7.1", "frame=3", "location=join(2000..2050,2080)"]),                                   # frame after protein_id; a single coordinate
        _rec("NC_000001.1", 8, ["frame=2", "protein_id=P8.1", "location=complement(join(<2100..2150,2200..>2260))"]),
        _rec("NC_000001.1", 9, ["pseudo=true", "protein_id=P9.1", "location=2300..2400"]),                                          # ends at pseudo
        _rec("NC_000001.1", 10, ["protein=hypothetical protein", "protein_id=P10.1", "location=2300..2400"]),                       # ends at hypothetical
        _rec("NC_000001.1", 11, ["protein_id=P11.1", "location=350..600"]),                                                         # overlaps 1 and 2
        _rec("NC_000001.1", 12, ["location=2500..2600"]),                                                                           # no protein_id: skipped, counted
        _rec("NC_000001.1", 13, ["protein_id=P13.1", "location=2950..2996"]),                                                       # 4 bases before the end: one step of extension
        _rec("NC_000001.1", 14, ["protein_id=P14.1", "location=8..70"]),                                                            # 7 bases after the start: two steps
        _rec("NC_000001.1", 15, ["protein_id=P15.1", "gbkey=CDS"]),                                                                 # no location at all
        _rec("NC_000001.1", 16, ["protein_id=P16.1", "location=2700"]),                                                             # a single coordinate on its own
    ]
    g2 = [_rec("NZ_AB12.2", 1, ["protein_id=Q1.1", "location=complement(1..1000)"])]                                                # the whole sequence: no room to extend
    g3 = [_rec("NC_000003.12", 1, ["protein_id=R1.1", "location=10..300"])]                                                         # key NC_000003.1: matches nothing
    g5 = [_rec("NC_000005.1", 1, ["protein_id=S1.1", "pseudo=true"])]                                                               # an entry with no location: by blocks, all non-CDS
    return genomes, [g1 + g2, g3 + g5]


def _write(tmp, genomes, files):
    paths = []
    for k, headers in enumerate(files):
        p = os.path.join(str(tmp), f"cds{k}.fna")
        with open(p, "w") as f:
            for h in headers:
                f.write(f">{h}\nATGAAATAG\n")
        paths.append(p)
    lst = os.path.join(str(tmp), "list.txt")
    open(lst, "w").write("\n".join(paths) + "\n")
    fa = os.path.join(str(tmp), "genomes.fa")
    with open(fa, "w") as f:
        for name, s in genomes:
            f.write(f">{name} some description\n")
            for k in range(0, len(s), 60):
                f.write(s[k:k + 60] + "\n")
    return lst, fa


def test_blocks_of_generated_annotation(cds_dump, tmp_path):
    genomes, files = _world()
    lst, fa = _write(tmp_path, genomes, files)
    r = subprocess.run([cds_dump, lst, fa], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    got = r.stdout.strip().split("\n")
    want = cds_spec.dump([h for f in files for h in f], genomes)
    assert got == want
    # ... and both against values worked out by hand
    assert got[0] == "stats records=19 cds=14 pseudo=2 hypothetical=1 orphan_location=1 no_location=1 two_digit_version=1 accessions=4"
    assert got[1:6] == ["seq 0 NC_000001.1 blocks", "seq 1 NZ_AB12.2 blocks", "seq 2 NC_000003.12 sixframes", "seq 3 plain.1 sixframes", "seq 4 NC_000005.1 blocks"]
    blocks = [tuple(map(int, l.split()[1:])) for l in got if l.startswith("block ")]
    for b in [(0, 1, 99 - 33, 401 + 33),                 # forward: 11 codons either side
              (0, -1, 499 - 33, 798 + 33),               # complement: the same range, strand -1
              (0, 1, 1700 - 33, 1799 + 33),              # frame 2: begin 1700 -> 1701 (1-based), 0-based 1700
              (0, -1, 1849 - 33, 1987 + 33),             # frame 3 on the complement strand: end 1990 -> 1988
              (0, 1, 2949 - 33, 2998),                   # 2995 + 3 = 2998 < 3000, 3001 is not
              (0, 1, 1, 69 + 33),                        # 7 -> 4 -> 1
              (0, 1, 2699 - 33, 2699 + 33),
              (1, -1, 0, 999),
              (4, 1, 0, 399)]:                           # an accession with an entry but no location: one non-CDS block
        assert b in blocks, b
    extras = [l.split() for l in got if l.startswith("extra ")]
    g = genomes[0][1]
    assert [e[1:3] for e in extras] == [["5", "0"], ["6", "0"], ["7", "0"], ["8", "0"]]
    assert extras[0][3] == g[899 - 33:1000] + g[1099:1222 + 33]
    assert extras[2][3] == g[2001 - 33:2050] + g[2079:2080 + 33]          # frame 3 moved the first begin by 2; the single coordinate is the last exon
    comp = {"A": "T", "C": "G", "G": "C", "T": "A"}
    assert extras[1][3] == "".join(comp[c] for c in reversed(g[1299 - 33:1350] + g[1399:1450] + g[1499:1591 + 33]))
    assert extras[3][3] == "".join(comp[c] for c in reversed(g[2099 - 33:2150] + g[2199:2259 + 33]))       # frame 2, complement: the last end 2260 -> 2259
    # non-CDS: the maximal uncovered runs of more than 32 bases, from the un-extended coordinates (70 .. 98 between CDS 14 and 1 is too short)
    assert (0, 1, 799, 898) in blocks and (0, 1, 1000, 1098) in blocks and (0, 1, 1222, 1298) in blocks
    assert not any(b[2] == 70 for b in blocks)
    assert (0, 1, 2259, 2698) in blocks                  # behind CDS 8 (end 2260 -> 2259 by its frame) up to CDS 16: records 9, 10 and 12 left no CDS behind


@pytest.mark.parametrize("location", ["2900..3001", "join(10..50,2990..3100)", "complement(0..90)", "700..600"])
def test_coordinates_outside_the_sequence_are_an_error(cds_dump, tmp_path, location):
    genomes, _ = _world()
    headers = [_rec("NC_000001.1", 1, ["protein_id=P1.1", "location=100..402"]), _rec("NC_000001.1", 2, ["protein_id=BAD7.1", f"location={location}"])]
    lst, fa = _write(tmp_path, genomes, [headers])
    r = subprocess.run([cds_dump, lst, fa], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "NC_000001.1_cds_P2.1_2" in r.stderr and "outside" in r.stderr, r.stderr[-2000:]
    with pytest.raises(cds_spec.CdsError):
        cds_spec.dump(headers, genomes)
