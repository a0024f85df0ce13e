"""Block route against six-frame route of the database builder on the same genomes, beside index_build_measure.py.

    python profiles/scripts/block_build_measure.py [N_GENOMES=32] [GENOME_LEN=1e6] [OUT.md]

Genomes are random (seeded); the "annotation" is made directly as blocks, the way host/cds_info.h makes them from a
cds_from_genomic file: single-location CDS of 300 .. 1500 bases on alternating strands with gaps of 5 .. 200 bases, each extended by
up to 11 codons on either side, and the gaps of more than 32 bases as forward non-CDS blocks (no joined CDS).  Both routes run in
one process, each once after a small warm-up call that allocates the buffers and loads the kernels: wall time of the synchronous
add_blocks / add_sequences call (upload of the same bases included), records produced, and finish() by mtb_builder_last_finish_stats.
A single run: no repetitions."""
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def genome_blocks(rng, L, seq):
    """(seq, strand, start, end) rows of one genome of L bases"""
    n = L // 600
    lens = 3 * rng.integers(100, 501, size=n)
    gaps = rng.integers(5, 201, size=n)
    a = np.cumsum(lens + gaps) - lens                      # first base of every CDS
    keep = a + lens <= L
    a, lens = a[keep], lens[keep]
    b = a + lens - 1
    start = a - 3 * np.minimum(11, a // 3)
    end = b + 3 * np.minimum(11, (L - 1 - b) // 3)
    strand = np.where(np.arange(len(a)) % 2 == 0, 1, -1)
    g0 = np.concatenate([[0], b + 1]); g1 = np.concatenate([a - 1, [L - 1]])      # uncovered runs
    m = g1 - g0 + 1 > 32
    rows = np.zeros(len(a) + int(m.sum()), dtype=[("seq", "<u4"), ("strand", "<i4"), ("start", "<u8"), ("end", "<u8")])
    rows["seq"] = seq
    rows["strand"][:len(a)] = strand; rows["start"][:len(a)] = start; rows["end"][:len(a)] = end
    rows["strand"][len(a):] = 1; rows["start"][len(a):] = g0[m]; rows["end"][len(a):] = g1[m]
    return rows, int(lens.sum())


def main():
    import metabuli_amd as M
    from index_build_measure import make_taxonomy
    n_gen = int(float(sys.argv[1])) if len(sys.argv) > 1 else 32
    L = int(float(sys.argv[2])) if len(sys.argv) > 2 else 1_000_000
    out_md = sys.argv[3] if len(sys.argv) > 3 else None
    taxdir = tempfile.mkdtemp(prefix="mtb_block_measure_tax_")
    tax, first, count = make_taxonomy(taxdir)
    rng = np.random.default_rng(7)
    bases = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=n_gen * L)]
    offs = (np.arange(n_gen + 1, dtype=np.uint64) * np.uint64(L))
    taxids = (first[rng.integers(0, len(first), size=n_gen)]).astype(np.int32)
    parts, cds_bases = [], 0
    for g in range(n_gen):
        rows, cb = genome_blocks(rng, L, g)
        parts.append(rows); cds_bases += cb
    blocks = np.concatenate(parts)
    block_bases = int((blocks["end"] - blocks["start"] + np.uint64(1)).sum())
    ctx = M.Context(0)
    out = {}
    for syncmer in (1, 0):
        b = ctx.builder(taxdir, M.default_params(seq_mode=1, syncmer=syncmer, kmer_format=2))
        # warm-up: one genome through both routes
        b.add_blocks(bases[:L], offs[:2], taxids[:1], parts[0]); b.add_sequences(bases[:L], offs[:2], taxids[:1])
        b.finish().close()
        res = {}
        for route in ("blocks", "six_frames"):
            ctx.sync()
            t0 = time.perf_counter()
            if route == "blocks":
                b.add_blocks(bases, offs, taxids, blocks)
            else:
                b.add_sequences(bases, offs, taxids)
            add_ms = 1e3 * (time.perf_counter() - t0)
            n_rec = b.num_records
            ix = b.finish()
            st = b.last_finish_stats()
            res[route] = dict(add_ms=add_ms, records=n_rec, entries=int(ix.num_targets), finish_ms=st["total"], sorts_ms=st["sort_key"] + st["sort_value"])
            ix.close()
        b.close()
        out[syncmer] = res
    ctx.close()
    Lm = []
    Lm.append(f"input: {n_gen} random genomes of {L} bases ({n_gen * L} bases, seed 7), one taxid each; {len(blocks)} blocks covering {block_bases} bases "
              f"({cds_bases} bases of CDS before the extension)")
    Lm.append("")
    Lm.append("| mode | route | add call, wall ms | records | records per base | finish() device ms | of which the two sorts | entries |")
    Lm.append("|---|---|---|---|---|---|---|---|")
    for syncmer in (1, 0):
        for route in ("blocks", "six_frames"):
            r = out[syncmer][route]
            Lm.append(f"| {'syncmer' if syncmer else 'dense'} | {route} | {r['add_ms']:.1f} | {r['records']} | {r['records'] / (n_gen * L):.3f} | {r['finish_ms']:.2f} | {r['sorts_ms']:.2f} | {r['entries']} |")
    text = "\n".join(Lm)
    print(text)
    if out_md:
        os.makedirs(os.path.dirname(os.path.abspath(out_md)), exist_ok=True)
        open(out_md, "w").write(text + "\n")


if __name__ == "__main__":
    main()
