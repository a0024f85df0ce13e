"""The database inspection (mtb_database_inspect) on synthetic databases written to files, next to mtb_database_audit on the same files.

    python profiles/scripts/inspect_measure.py [N_ENTRIES=2e8] [OUT.md] [REPS=3]

Three databases:
  even        profiles/scripts/audit_measure.py's: N entries (mtb_synth_index: values ascending, ids uniform over 2^18 strain ids),
              2^17 species of two strains under one genus.
  skewed      the same files under audit_measure.py's second taxonomy: one species owns 60 % of the strains.
  root-heavy  N entries whose amino-acid parts repeat (four values per part on average), ids uniform over 2^18 strains that alternate
              between two domains: most level-1 groups of two or more members meet at the root.
Per database, REPS times each: the inspection at both levels with its times by stage, and mtb_database_audit of the SAME library
(ms_decode + ms_check: both read the same bytes once; to time another commit's audit, run this script there).  Medians, one process."""
import os
import shutil
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
LO, N_IDS = 1_000_000, 1 << 18


def two_domain_taxonomy(d):
    """strain k under species 100 + k // 2 under genus 10 + (k // 2) % 2 under domain 2 + (k // 2) % 2"""
    from metabuli_amd import synth
    tax = synth.Taxonomy()
    tax.add(1, 1, "no rank", "root"); tax.add(2, 1, "superkingdom", "Bacteria"); tax.add(3, 1, "superkingdom", "Eukaryota")
    tax.add(10, 2, "genus", "G0"); tax.add(11, 3, "genus", "G1")
    for k in range(N_IDS):
        sp = 100 + k // 2
        if sp not in tax.parent:
            tax.add(sp, 10 + (k // 2) % 2, "species", f"s{sp}")
        tax.add(LO + k, sp, "no rank", f"strain{k}")
    tax.write(d)


def med(xs):
    return float(np.median(np.array(xs, dtype=np.float64)))


def main():
    import torch
    import metabuli_amd as M
    from audit_measure import taxonomy
    args = sys.argv[1:]
    n = int(float(args[0])) if args else 200_000_000
    out_md = args[1] if len(args) > 1 else None
    reps = int(args[2]) if len(args) > 2 else 3
    base = tempfile.mkdtemp(prefix="mtb_inspect_measure_")
    p = lambda: M.default_params(seq_mode=1, syncmer=1, kmer_format=2)
    ctx = M.Context(0)
    listed = np.arange(LO, LO + N_IDS, dtype=np.int32)
    tax_even, tax_skew, tax_root = (os.path.join(base, x) for x in ("tax_even", "tax_skewed", "tax_root"))
    taxonomy(tax_even, False); taxonomy(tax_skew, True); two_domain_taxonomy(tax_root)
    # even / skewed: one set of files
    db_even = os.path.join(base, "db_even"); os.makedirs(db_even)
    dv = torch.empty(n + 16, dtype=torch.int64, device="cuda"); di = torch.empty(n + 16, dtype=torch.int32, device="cuda")
    got = ctx.synth_index(4321, n, LO, LO + N_IDS - 1, np.zeros(0, np.uint64), np.zeros(0, np.int32), dv.data_ptr(), di.data_ptr())
    ix = ctx.index_from_device(dv.data_ptr(), di.data_ptr(), got, tax_even, listed, p())
    ix.write(db_even, 4096); ix.close()
    # root-heavy: n / 4 amino-acid parts drawn n times, a random DNA part each, sorted (equal values are left in: a handful)
    db_root = os.path.join(base, "db_root"); os.makedirs(db_root)
    g = torch.Generator(device="cuda"); g.manual_seed(7)
    aa = torch.randint(1, max(n // 4, 2), (n,), dtype=torch.int64, device="cuda", generator=g)
    dna = torch.randint(0, 1 << 24, (n,), dtype=torch.int64, device="cuda", generator=g)
    dv[:n] = torch.sort((aa << 24) | dna).values
    di[:n] = torch.randint(LO, LO + N_IDS, (n,), dtype=torch.int64, device="cuda", generator=g).to(torch.int32)
    del aa, dna
    torch.cuda.synchronize()
    ix = ctx.index_from_device(dv.data_ptr(), di.data_ptr(), n, tax_root, listed, p())
    ix.write(db_root, 4096); ix.close()
    del dv, di; torch.cuda.empty_cache()
    L = [f"{n} entries per database, {reps} repetitions, medians; one process", "",
         "| database | pass | entries | chunks | ms_read | ms_decode | ms_inspect / ms_check | ms_bins / ms_hist | ms_total | decode + pass ms | ratio to the audit | groups | largest group | "
         "share of groups at the root | size histogram (floor log2) |", "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    ratios = {}
    for name, db, taxdir in (("even", db_even, tax_even), ("skewed (one species 60 %)", db_even, tax_skew), ("root-heavy", db_root, tax_root)):
        reports = [ctx.audit_database(db, taxonomy_dir=taxdir, params=p(), chunk_words=0, counts=True)[0] for _ in range(reps)]
        m = lambda k: med([x[k] for x in reports])
        audit_ms = m("ms_decode") + m("ms_check")
        rep = reports[-1]
        L.append(f"| {name} | audit | {rep['n_entries']} | {rep['n_chunks']} | {m('ms_read'):.0f} | {m('ms_decode'):.1f} | {m('ms_check'):.1f} | {m('ms_hist'):.1f} | {m('ms_total'):.0f} | {audit_ms:.1f} | 1.00 | | | | |")
        print(L[-1], flush=True)
        for level in ("dna", "aa"):
            runs = [ctx.inspect_database(db, taxonomy_dir=taxdir, level=level, chunk_words=0, params=p()) for _ in range(reps)]
            reports = [x[0] for x in runs]
            rep, distinct = reports[-1], runs[-1][1]
            m = lambda k: med([x[k] for x in reports])
            ms = m("ms_decode") + m("ms_inspect")
            ratios[(name, level)] = ms / audit_ms
            top = max(k for k in range(40) if rep["size_hist"][k]) if rep["n_groups"] else 0
            L.append(f"| {name} | inspect {level} | {rep['n_entries']} | {rep['n_chunks']} | {m('ms_read'):.0f} | {m('ms_decode'):.1f} | {m('ms_inspect'):.1f} | {m('ms_bins'):.1f} | {m('ms_total'):.0f} | {ms:.1f} | "
                     f"{ms / audit_ms:.2f} | {rep['n_groups']} | {rep['max_group']} | {int(distinct[1]) / max(rep['n_groups'], 1):.3f} | {' '.join(str(x) for x in rep['size_hist'][:top + 1])} |")
            print(L[-1], "   every repetition: ms_inspect " + ", ".join(f"{x['ms_inspect']:.1f}" for x in reports), flush=True)
    L += ["", "root-heavy against even, ratio of (decode + pass): " + ", ".join(f"{lv} {ratios[('root-heavy', lv)] / ratios[('even', lv)]:.2f}" for lv in ("dna", "aa"))]
    ctx.close()
    shutil.rmtree(base, ignore_errors=True)
    text = "\n".join(L)
    print(text)
    if out_md:
        os.makedirs(os.path.dirname(os.path.abspath(out_md)), exist_ok=True)
        open(out_md, "w").write(text + "\n")


if __name__ == "__main__":
    main()
