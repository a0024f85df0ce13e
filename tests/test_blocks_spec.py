"""The block-scan arithmetic of mtb_core.h (mtb_block_*) on the host -- tests/emu/blocks_check.cpp, a stand-alone program -- against the
oracle's six-frame scan and tests/bruteforce.py (tests/blocks_spec.py says how a block is one frame of a six-frame scan); then the same
program under -fsanitize=address,undefined on the edge shapes, where a read outside the sequence is an error."""
import os
import subprocess

import numpy as np
import pytest

import blocks_spec
from blocks_spec import make_blocks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "emu", "blocks_check.cpp")


def _build(tmp, flags=()):
    exe = os.path.join(str(tmp), "blocks_check" + ("_san" if flags else ""))
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", *flags, "-o", exe, SRC])
    return exe


def _run(exe, tmp, cases):
    """cases: (sequence bytes, start, end, strand, syncmer) -> list of uint64 arrays"""
    path = os.path.join(str(tmp), "cases.txt")
    with open(path, "w") as f:
        for seq, start, end, strand, syncmer in cases:
            f.write(f"{seq.decode() or '-'} {start} {end} {strand} {syncmer} 5\n")
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    out = []
    for line in r.stdout.strip().split("\n"):
        w = line.split()
        assert int(w[0]) == len(w) - 1
        out.append(np.array([int(x, 16) for x in w[1:]], np.uint64))
    assert len(out) == len(cases)
    return out


def _random_cases(rng, n):
    cases = []
    for i in range(n):
        L = int(rng.integers(1, 140))
        seq = rng.choice(np.frombuffer(b"ACGT", np.uint8), size=L)
        if i % 3 == 0:                                          # a few invalid bases; lower case and IUPAC codes the tables know
            for _ in range(int(rng.integers(1, 4))):
                seq[int(rng.integers(0, L))] = rng.choice(np.frombuffer(b"NnacgtRY", np.uint8))
        blen = int(rng.integers(1, min(L, 99) + 1))
        start = int(rng.integers(0, L - blen + 1))
        cases.append((seq.tobytes(), start, start + blen - 1, 1 if rng.random() < 0.5 else -1, int(rng.integers(0, 2))))
    return cases


def _expected(fn, cases):
    """per case through blocks_spec: one sequence and one block each"""
    out = []
    for syncmer in (0, 1):
        sel = [c for c in cases if c[4] == syncmer]
        bases = np.concatenate([np.frombuffer(c[0], np.uint8) for c in sel])
        offs = np.zeros(len(sel) + 1, np.uint64); offs[1:] = np.cumsum([len(c[0]) for c in sel])
        blocks = make_blocks([(i, c[3], c[1], c[2]) for i, c in enumerate(sel)])
        v, bo = fn(syncmer, bases, offs, blocks)
        out.append({id(c): v[bo == i] for i, c in enumerate(sel)})
    return [out[c[4]][id(c)] for c in cases]


def test_block_scan_against_oracle_and_bruteforce(orc, tmp_path):
    import bruteforce
    cases = _random_cases(np.random.default_rng(2024), 600)
    got = _run(_build(tmp_path), tmp_path, cases)
    T = bruteforce.ref_tables()
    want_o = _expected(lambda s, b, o, k: blocks_spec.oracle_blocks(orc, s, b, o, k), cases)
    want_b = _expected(lambda s, b, o, k: blocks_spec.brute_blocks(T, s, b, o, k), cases)
    n_nonempty = 0
    for c, g, wo, wb in zip(cases, got, want_o, want_b):
        assert len(g) == len(wo) == len(wb) and (g == wo).all() and (g == wb).all(), c
        n_nonempty += len(g) > 0
    assert n_nonempty > 200                                      # the comparison is not one of empty lists
    # both strands of one range give different lists unless both are empty
    assert sum(len(g) for g in got) > 2000


def test_block_scan_edges_under_sanitizers(orc, tmp_path):
    """lengths 0 .. 26 (0 as the empty range end = start - 1), a block at base 0 and one at the last base of a sequence allocated at exactly
    its length, windows 63 .. 65 and P - 1 .. P + 1 .. 2P + 1, an invalid base at every codon phase: no read outside the sequence, no
    undefined arithmetic, and the values of the oracle"""
    P = blocks_spec.piece_windows()
    rng = np.random.default_rng(5)
    cases = []
    for syncmer in (0, 1):
        for strand in (1, -1):
            for blen in (0, 1, 2, 23, 24, 25, 26):
                seq = rng.choice(np.frombuffer(b"ACGT", np.uint8), size=40).tobytes()
                cases.append((seq, 7, 7 + blen - 1, strand, syncmer))
                if blen:
                    cases.append((seq[:blen], 0, blen - 1, strand, syncmer))          # the block is the whole sequence: touches base 0 and the last base
                    cases.append((seq, 40 - blen, 39, strand, syncmer))
            for n_win in (63, 64, 65, P - 1, P, P + 1, 2 * P + 1):
                for extra in (0, 2):
                    L = 3 * (n_win + 7) + extra
                    seq = rng.choice(np.frombuffer(b"ACGT", np.uint8), size=L)
                    cases.append((seq.tobytes(), 0, L - 1, strand, syncmer))
            for phase in range(3):
                seq = rng.choice(np.frombuffer(b"ACGT", np.uint8), size=120)
                seq[60 + phase] = ord("N")
                cases.append((seq.tobytes(), 3, 116, strand, syncmer))
    exe = _build(tmp_path, ("-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    got = _run(exe, tmp_path, cases)
    live = [c for c in cases if c[2] >= c[1]]
    want = dict(zip(map(id, live), _expected(lambda s, b, o, k: blocks_spec.oracle_blocks(orc, s, b, o, k), live)))
    for c, g in zip(cases, got):
        w = want[id(c)] if id(c) in want else np.zeros(0, np.uint64)
        assert len(g) == len(w) and (g == w).all(), (c[1:], len(g), len(w))
        if c[2] - c[1] + 1 < 24:
            assert len(g) == 0
