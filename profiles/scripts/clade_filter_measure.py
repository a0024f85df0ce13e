"""The filtered merge (mtb_merge_databases_filtered) next to the plain merge of the same database: where the filter's time goes.

    python profiles/scripts/clade_filter_measure.py make DIR [N_RECORDS=1.5e8]     # DIR/tax, DIR/db: one database of N / 1.25 entries
    python profiles/scripts/clade_filter_measure.py plain DIR                      # mtb_merge_databases of DIR/db -> one JSON line
    python profiles/scripts/clade_filter_measure.py filtered DIR                   # ... without every other genus -> one JSON line

The database is that of merge_stream_measure.py with k = 1 (distinct valid format-2 words under random strains, 4096 checkpoints).
`plain` uses nothing this measurement adds, so it also runs against a library built from an earlier commit (MTB_LIB=...): that is
how the unfiltered figure of profiles/merge_stream_notes.md ("Filtered merge") was taken.  Each call is one run; the output
directory is removed afterwards."""
import json
import os
import shutil
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main():
    import metabuli_amd as M
    from index_build_measure import make_taxonomy
    mode, base = sys.argv[1], sys.argv[2]
    taxdir, db, out = os.path.join(base, "tax"), os.path.join(base, "db"), os.path.join(base, "out_" + mode)
    ctx = M.Context(0)
    p = M.default_params(seq_mode=1, syncmer=1, kmer_format=2)
    if mode == "make":
        from merge_stream_measure import make_inputs
        n = int(float(sys.argv[3])) if len(sys.argv) > 3 else 150_000_000
        os.makedirs(taxdir, exist_ok=True)
        tax, first, count = make_taxonomy(taxdir)
        dirs, entries = make_inputs(ctx, M, taxdir, first, count, n, 1, base)
        os.rename(dirs[0], db)
        print(json.dumps(dict(mode=mode, n_records=n, n_entries=int(entries[0]))), flush=True)
    else:
        tax, _, _ = make_taxonomy(taxdir)
        genera = sorted(t for t, r in tax.rank.items() if r == "genus")
        shutil.rmtree(out, ignore_errors=True); os.makedirs(out)
        if mode == "plain":
            st = ctx.merge_databases([db], taxdir, p, out, split_num=4096)
        else:
            st = ctx.merge_databases([db], taxdir, p, out, split_num=4096, exclude=genera[::2])
        shutil.rmtree(out, ignore_errors=True)
        st.update(mode=mode, lib=os.path.basename(M.LIB_PATH))
        print(json.dumps(st), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
