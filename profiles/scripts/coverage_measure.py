"""What k-mer coverage (mtb_index_coverage_*) costs a batch: the same batches with coverage off and on, in one process.

    python profiles/scripts/coverage_measure.py [TARGETS=4e9] [READS=2000000] [OUT.md] [REPS=5]

The world, the index and the reads are bench.py's (build_world_fast, extract_targets, mtb_synth_index, gen_reads; 2400 species of
1 Mbp -- 2.5 G targets of their own --, filler up to TARGETS, sealed index), at a size that leaves room on one GPU.  Two read sets:
from the indexed genomes, and from genomes that are NOT in the index (bench.py's novel leg: held-out species of indexed genera).  Per
set: four warm-up batches (the join tuner settles), then REPS batches with coverage off, REPS with coverage on, REPS off again -- the
same reads every time --: medians of ms_total and ms_score from mtb_last_batch_stats, the difference, ms_count of
mtb_index_coverage_report (one pass over the resident array), the bitmap's bytes and what the report says."""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def med(xs):
    return float(np.median(np.array(xs, dtype=np.float64)))


def main():
    import torch
    import bench as B
    import metabuli_amd as M
    args = sys.argv[1:]
    targets = int(float(args[0])) if args else 4_000_000_000
    n_reads = int(float(args[1])) if len(args) > 1 else 2_000_000
    out_md = args[2] if len(args) > 2 else None
    reps = int(args[3]) if len(args) > 3 else 5
    read_len, seed = 150, 1234
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    ctx = M.Context(0)
    ctx.set_placement_probe(True)
    params = M.default_params(seq_mode=1, syncmer=1, smer_len=5)
    world = B.build_world_fast(torch, dev, seed, 2400, 1_000_000, 130_000, conserved=True, n_heldout=200)
    taxdir = tempfile.mkdtemp(prefix="mtb_tax_")
    world.tax.write(taxdir)
    real_v, real_t, n_extras = B.extract_targets(ctx, M, world, params, torch, dev, hot_min=8, seed=seed)
    n_filler = targets - len(real_v)
    if n_filler < 0:
        raise SystemExit(f"TARGETS {targets} is the total: the genomes alone give {len(real_v)}")
    d_values = torch.empty(targets, dtype=torch.int64, device=dev); d_info = torch.empty(targets, dtype=torch.int32, device=dev)
    T = ctx.synth_index(seed, n_filler, world.filler_tax_lo, world.filler_tax_hi, real_v, real_t, d_values.data_ptr(), d_info.data_ptr())
    taxid_list = np.concatenate([np.unique(real_t), np.arange(world.filler_tax_lo, world.filler_tax_hi + 1, dtype=np.int32)])
    index = ctx.index_from_device(d_values.data_ptr(), d_info.data_ptr(), T, taxdir, taxid_list, params)
    read_sets = [("indexed", B.gen_reads(torch, dev, world.genomes, n_reads, read_len, 0.10, 0.005, seed + 17)),
                 ("held-out", B.gen_reads(torch, dev, world.heldout, n_reads, read_len, 0.10, 0.005, seed + 21))]
    index.seal(); d_info = None
    torch.cuda.empty_cache()
    d_res = torch.empty(n_reads * 24, dtype=torch.uint8, device=dev)
    tc_cap = n_reads * (20 + read_len // 9) + 1024
    d_tt = torch.empty(tc_cap, dtype=torch.int32, device=dev); d_tc = torch.empty(tc_cap, dtype=torch.int32, device=dev)

    def step(d_bases, d_offs):
        ctx.classify_batch_device(index, params, d_bases.data_ptr(), d_offs.data_ptr(), 0, 0, n_reads, n_reads * read_len, d_res.data_ptr(), d_tt.data_ptr(), d_tc.data_ptr(), tc_cap)
        st = ctx.last_stats()
        return float(st.ms_total), float(st.ms_score)

    def leg(reads):
        runs = [step(*reads) for _ in range(reps)]
        return med([r[0] for r in runs]), med([r[1] for r in runs]), runs

    bitmap = (T + 31) // 32 * 4
    L = [f"{T} targets (sealed, state {index.state()}), {n_reads} reads x {read_len} bp, {reps} batches per leg, medians; one process",
         f"bitmap: {bitmap} bytes ({bitmap / 2**20:.1f} MiB)"]
    for set_name, reads in read_sets:
        for _ in range(4):
            step(*reads)
        off1 = leg(reads)
        index.coverage_begin()
        on = leg(reads)
        rep = index.coverage_report()
        counts = [index.coverage_report()["ms_count"] for _ in range(reps)]
        index.coverage_end()
        off2 = leg(reads)
        L += measured(set_name, T, reps, off1, on, off2, rep, counts)
        print("\n".join(L[-9:]), flush=True)
    text = "\n".join(L)
    print(text, flush=True)
    if out_md:
        os.makedirs(os.path.dirname(os.path.abspath(out_md)), exist_ok=True)
        open(out_md, "w").write(text + "\n")
    index.close(); ctx.close()


def measured(set_name, T, reps, off1, on, off2, rep, counts):
    off_total, off_score = med([off1[0], off2[0]]), med([off1[1], off2[1]])
    L = ["", f"reads from {set_name} genomes", "", "| coverage | ms_total | ms_score | every batch: ms_total |", "|---|---|---|---|"]
    for name, (t, s, runs) in (("off (before)", off1), ("on", on), ("off (after)", off2)):
        L.append(f"| {name} | {t:.2f} | {s:.2f} | " + ", ".join(f"{r[0]:.2f}" for r in runs) + " |")
    L += ["", f"marking (read species + mark) per batch: ms_total on - off = {on[0] - off_total:.2f} ms, ms_score on - off = {on[1] - off_score:.2f} ms "
              f"({100 * (on[0] - off_total) / off_total:.1f} % of a batch)",
          f"report (k_cov_count + reduce + popcount), ms_count: {med(counts):.2f} ms ({T / med(counts) / 1e6:.2f} G entries/s); every call: " + ", ".join(f"{c:.2f}" for c in counts),
          f"hits bins: {(len(rep['hits']) + 4) * 8} bytes",
          f"after {reps} batches of the same reads: {rep['n_marked']} entries marked, {rep['n_hits']} hits, {rep['n_queries']} query metamers seen, "
          f"{rep['n_queries_counted']} of reads with a species, {int((rep['distinct'] > 0).sum())} species with a distinct k-mer, {rep['n_batches']} calls committed"]
    return L


if __name__ == "__main__":
    main()
