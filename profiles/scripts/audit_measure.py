"""The database audit (mtb_database_audit) on a synthetic database written to files, next to mtb_index_open on the same files.

    python profiles/scripts/audit_measure.py [N_ENTRIES=2e8] [OUT.md] [REPS=3]

One database of N entries (mtb_synth_index: values ascending, ids uniform over 2^18 strain ids; written with mtb_index_write, 4096
checkpoints) under two taxonomies: `uniform` -- 2^17 species of 2 strains: the bins that are hit span 0.5 MB --, `skewed` -- one
species owns 60 % of the strains, the others keep 2 each.  Per taxonomy, REPS times each: the audit (chunk size 0: the library's
choice) in every way of taking the species counts that mtb_debug_audit_mode offers -- in the check kernel with a hot species folded
in the wave and one bin array per XCD summed at the end (the default), not at all, one add per entry, and the last two into a single
bin array -- and
mtb_index_open (the decode the audit reuses: wall clock of the call, flat state).  Medians, one process."""
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
LO, N_IDS = 1_000_000, 1 << 18
MODES = ((0, "folded, bin array per XCD (default)"), (1, "no counts"), (2, "one add per entry, bin array per XCD"), (3, "folded, one bin array"), (4, "one add per entry, one bin array"))


def taxonomy(d, skewed):
    from metabuli_amd import synth
    tax = synth.Taxonomy()
    tax.add(1, 1, "no rank", "root"); tax.add(2, 1, "superkingdom", "Bacteria"); tax.add(10, 2, "genus", "G")
    hot = int(0.6 * N_IDS) if skewed else 0                       # strains of the hot species
    for k in range(N_IDS):
        sp = 100 + (0 if k < hot else 1 + (k - hot) // 2)
        if sp not in tax.parent:
            tax.add(sp, 10, "species", f"s{sp}")
        tax.add(LO + k, sp, "no rank", f"strain{k}")
    tax.write(d)


def med(xs):
    return float(np.median(np.array(xs, dtype=np.float64)))


def main():
    import torch
    import metabuli_amd as M
    args = sys.argv[1:]
    n = int(float(args[0])) if args else 200_000_000
    out_md = args[1] if len(args) > 1 else None
    reps = int(args[2]) if len(args) > 2 else 3
    base = tempfile.mkdtemp(prefix="mtb_audit_measure_")
    p = lambda: M.default_params(seq_mode=1, syncmer=1, kmer_format=2)
    ctx = M.Context(0)
    L = [f"{n} entries per database, {reps} repetitions, medians; one process", "",
         "| taxonomy | counts taken | entries | chunks | audit ms_read | ms_decode | ms_check (order + ids + counts + checkpoints) | ms_hist (bins clear + reduce + download) | ms_total | "
         "check Gentries/s | largest count | valid, canonical | mtb_index_open ms (wall) |", "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    db = os.path.join(base, "db"); os.makedirs(db)
    taxdir = os.path.join(base, "tax_uniform")
    taxonomy(taxdir, False)
    dv = torch.empty(n + 16, dtype=torch.int64, device="cuda"); di = torch.empty(n + 16, dtype=torch.int32, device="cuda")
    got = ctx.synth_index(4321, n, LO, LO + N_IDS - 1, np.zeros(0, np.uint64), np.zeros(0, np.int32), dv.data_ptr(), di.data_ptr())
    ix = ctx.index_from_device(dv.data_ptr(), di.data_ptr(), got, taxdir, np.arange(LO, LO + N_IDS, dtype=np.int32), p())
    t0 = time.perf_counter(); ix.write(db, 4096); tw = time.perf_counter() - t0
    ix.close(); del dv, di; torch.cuda.empty_cache()
    size = sum(os.path.getsize(os.path.join(db, f)) for f in ("diffIdx", "info"))
    L.insert(1, f"database: {got} entries, diffIdx + info = {size / 2**30:.2f} GiB, written in {tw:.1f} s")
    for name, skewed in (("uniform", False), ("skewed (one species 60 %)", True)):      # (the files are the same: the taxonomy decides the species)
        taxdir = os.path.join(base, "tax_skewed" if skewed else "tax_uniform")
        if skewed:
            taxonomy(taxdir, True)
        opens = []
        for r in range(reps):
            t0 = time.perf_counter()
            ix = ctx.open_index(db, p(), taxonomy_dir=taxdir)
            ctx.sync()
            opens.append((time.perf_counter() - t0) * 1e3)
            ix.close()
        for mode, label in MODES:
            M._chk(ctx.L.mtb_debug_audit_mode(ctx.h, mode))
            reports = []
            for r in range(reps):
                rep, counts = ctx.audit_database(db, taxonomy_dir=taxdir, params=p(), chunk_words=0)
                reports.append(rep)
            m = lambda k: med([x[k] for x in reports])
            L.append(f"| {name} | {label} | {rep['n_entries']} | {rep['n_chunks']} | {m('ms_read'):.0f} | {m('ms_decode'):.1f} | {m('ms_check'):.1f} | {m('ms_hist'):.1f} | {m('ms_total'):.0f} | "
                     f"{rep['n_entries'] / m('ms_check') / 1e6:.2f} | {int(counts.max())} ({counts.max() / rep['n_entries']:.2f}) | {rep['valid']}, {rep['canonical']} | {med(opens):.0f} |")
            print(L[-1], "   every repetition: ms_check " + ", ".join(f"{x['ms_check']:.1f}" for x in reports) + "; ms_decode " + ", ".join(f"{x['ms_decode']:.1f}" for x in reports), flush=True)
        M._chk(ctx.L.mtb_debug_audit_mode(ctx.h, 0))
    ctx.close()
    shutil.rmtree(base, ignore_errors=True)
    text = "\n".join(L)
    print(text)
    if out_md:
        os.makedirs(os.path.dirname(os.path.abspath(out_md)), exist_ok=True)
        open(out_md, "w").write(text + "\n")


if __name__ == "__main__":
    main()
