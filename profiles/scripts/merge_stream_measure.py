"""The streamed merge (mtb_merge_databases) against the in-memory route (mtb_builder_add_index x k, mtb_builder_finish) on the same
databases, in ONE process.

    python profiles/scripts/merge_stream_measure.py [N_ENTRIES=2e8] [OUT.md] [KS=2,8] [REPS=3]
    python profiles/scripts/merge_stream_measure.py big [N_PER_DB=2.5e9] [OUT.md]        # two databases, more than 2^32 records in

Inputs (a pure function of the arguments): N / 1.25 distinct valid format-2 words; word g lives in database g mod k under a random
strain of a random species, and every fourth word also in database (g + 1) mod k under another random strain of the same species,
so a fifth of the output entries are groups of two that meet only in the merge.  Every database is built on the device and written
with 4096 checkpoints.  Then, REPS times each: the merge into a fresh directory with max_range_records = 0 (one range when the
device holds it: ms_merge + ms_reduce is the device part that the in-memory route spends in finish()), and the in-memory route
(open every database, add_index, finish: mtb_build_stats total).  The two results are compared file by file once per k.
`big`: the databases are synthetic filler indices (mtb_synth_index) written with mtb_index_write; the merge's statistics, the
re-opened output's entry count and the peak of device memory in use (sampled by a thread through hipMemGetInfo) are reported."""
import os
import shutil
import sys
import tempfile
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
CHUNK = 1 << 24


def mix(x, salt):
    x = (x + np.uint64(salt)) * np.uint64(0xBF58476D1CE4E5B9)
    x ^= x >> np.uint64(29)
    x *= np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(32))


def make_inputs(ctx, M, taxdir, first, count, n_entries, k, base):
    from index_build_measure import group_values
    p = M.default_params(seq_mode=1, syncmer=1, kmer_format=2)
    builders = [ctx.builder(taxdir, p) for _ in range(k)]
    n_groups = int(n_entries / 1.25)
    for g0 in range(0, n_groups, CHUNK):
        gn = np.arange(g0, min(g0 + CHUNK, n_groups), dtype=np.uint64)
        v = group_values(gn)
        sp = (mix(gn, 1) % np.uint64(len(first))).astype(np.int64)
        t0 = (first[sp] + (mix(gn, 2) % count[sp].astype(np.uint64)).astype(np.int64)).astype(np.int32)
        t1 = (first[sp] + (mix(gn, 3) % count[sp].astype(np.uint64)).astype(np.int64)).astype(np.int32)
        home = (gn % np.uint64(k)).astype(np.int64)
        dup = (mix(gn, 4) & np.uint64(3)) == 0
        for j in range(k):
            m = home == j
            builders[j].add_records(v[m], t0[m])
            m = dup & ((home + 1) % k == j)
            builders[j].add_records(v[m], t1[m])
    dirs, entries = [], []
    for j, b in enumerate(builders):
        d = os.path.join(base, f"in{k}_{j}"); os.makedirs(d)
        ix = b.finish()
        entries.append(ix.num_targets)
        ix.write(d, 4096)
        ix.close(); b.close()
        dirs.append(d)
    return dirs, entries


def med(xs):
    return float(np.median(np.array(xs, dtype=np.float64)))


def compare(M, ctx, taxdir, ks, n_entries, reps, L):
    from index_build_measure import make_taxonomy
    base = tempfile.mkdtemp(prefix="mtb_merge_measure_")
    tax, first, count = make_taxonomy(taxdir)
    p = lambda: M.default_params(seq_mode=1, syncmer=1, kmer_format=2)
    L.append(f"inputs: about {n_entries} entries over k databases (4096 checkpoints each); {reps} repetitions, medians; one process")
    L.append("")
    L.append("| k | input entries | output entries | ranges | merge ms_merge | ms_reduce | merge + reduce | builder finish total (sort_key, sort_value, reduce) | ratio builder / merge | "
             "merge ms_read_decode | ms_encode_write | ms_split | ms_total | files equal |")
    L.append("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    for k in ks:
        dirs, entries = make_inputs(ctx, M, taxdir, first, count, n_entries, k, base)
        ms, bs = [], []
        out = os.path.join(base, f"out{k}")
        for r in range(reps):
            shutil.rmtree(out, ignore_errors=True); os.makedirs(out)
            ms.append(ctx.merge_databases(dirs, taxdir, p(), out, split_num=4096, max_range_records=0))
        ref = os.path.join(base, f"ref{k}"); os.makedirs(ref)
        for r in range(reps):
            b = ctx.builder(taxdir, p())
            for d in dirs:
                ix = ctx.open_index(d, p(), taxonomy_dir=taxdir)
                b.add_index(ix)
                ix.close()
            ix = b.finish()
            bs.append(b.last_finish_stats())
            if r == 0:
                ix.write(ref, 4096)
            ix.close(); b.close()
        same = all(open(os.path.join(out, f), "rb").read() == open(os.path.join(ref, f), "rb").read() for f in ("diffIdx", "info", "split", "taxID_list", "db.parameters"))
        mr = med([s["ms_merge"] + s["ms_reduce"] for s in ms]); bt = med([s["total"] for s in bs])
        L.append(f"| {k} | {sum(entries)} | {ms[0]['n_entries']} | {ms[0]['n_ranges']} | {med([s['ms_merge'] for s in ms]):.2f} | {med([s['ms_reduce'] for s in ms]):.2f} | {mr:.2f} | "
                 f"{bt:.2f} ({med([s['sort_key'] for s in bs]):.2f}, {med([s['sort_value'] for s in bs]):.2f}, {med([s['reduce'] for s in bs]):.2f}) | {bt / mr:.2f} | "
                 f"{med([s['ms_read_decode'] for s in ms]):.0f} | {med([s['ms_encode_write'] for s in ms]):.0f} | {med([s['ms_split'] for s in ms]):.0f} | {med([s['ms_total'] for s in ms]):.0f} | {same} |")
        L.append("")
        L.append(f"k = {k}, every repetition: merge+reduce " + ", ".join(f"{s['ms_merge'] + s['ms_reduce']:.2f}" for s in ms) + " ms; builder total " + ", ".join(f"{s['total']:.2f}" for s in bs) + " ms")
        L.append("")
        print("\n".join(L[-4:]), flush=True)
        for d in dirs + [out, ref]:
            shutil.rmtree(d, ignore_errors=True)
    shutil.rmtree(base, ignore_errors=True)


def big(M, ctx, taxdir, n_per_db, L):
    import torch
    from metabuli_amd import synth
    base = tempfile.mkdtemp(prefix="mtb_merge_big_")
    free = shutil.disk_usage(base).free
    need = int(n_per_db * 2 * 2 * 9)                      # two inputs + the output, ~9 bytes per entry
    if free < need:
        L.append(f"a merge past 2^32 records: NOT RUN -- {base} has {free / 2**30:.0f} GiB free, the two inputs and the output need about {need / 2**30:.0f} GiB")
        return
    tax = synth.Taxonomy()
    tax.add(1, 1, "no rank", "root"); tax.add(2, 1, "superkingdom", "Bacteria"); tax.add(10, 2, "genus", "G")
    for s in range(64):
        tax.add(100 + s, 10, "species", f"s{s}")
        for t in range(8):
            tax.add(1000 + 8 * s + t, 100 + s, "no rank", f"strain{s}_{t}")
    tax.write(taxdir)
    p = lambda: M.default_params(seq_mode=1, syncmer=1, kmer_format=2)
    dirs = []
    for j in range(2):
        dv = torch.empty(int(n_per_db) + 16, dtype=torch.int64, device="cuda"); di = torch.empty(int(n_per_db) + 16, dtype=torch.int32, device="cuda")
        n = ctx.synth_index(1234 + j, int(n_per_db), 1000, 1000 + 511, np.zeros(0, np.uint64), np.zeros(0, np.int32), dv.data_ptr(), di.data_ptr())
        ix = ctx.index_from_device(dv.data_ptr(), di.data_ptr(), n, taxdir, np.arange(1000, 1512, dtype=np.int32), p())
        d = os.path.join(base, f"big{j}"); os.makedirs(d)
        t0 = time.perf_counter(); ix.write(d, 4096); tw = time.perf_counter() - t0
        ix.close(); del dv, di; torch.cuda.empty_cache()
        dirs.append(d)
        L.append(f"input {j}: {n} entries written in {tw:.0f} s")
        print(L[-1], flush=True)
    out = os.path.join(base, "out"); os.makedirs(out)
    peak = [0]; stop = threading.Event()

    def watch():
        while not stop.is_set():
            fr, tot = torch.cuda.mem_get_info()
            peak[0] = max(peak[0], tot - fr)
            time.sleep(0.05)
    th = threading.Thread(target=watch); th.start()
    st = ctx.merge_databases(dirs, taxdir, p(), out, split_num=4096, max_range_records=0)
    stop.set(); th.join()
    ix = ctx.open_index(out, p(), taxonomy_dir=taxdir)
    L.append(f"merge of {st['n_input_entries']} input entries (2^32 = {1 << 32}): {st['n_entries']} output entries, re-opened: {ix.num_targets}; {st['n_ranges']} ranges of at most "
             f"{st['max_range_records_used']} records; ms: read+decode {st['ms_read_decode']:.0f}, merge {st['ms_merge']:.0f}, reduce {st['ms_reduce']:.0f}, encode+write {st['ms_encode_write']:.0f}, "
             f"split {st['ms_split']:.0f}, total {st['ms_total']:.0f}; peak device memory in use during the merge {peak[0] / 2**30:.1f} GiB")
    ix.close()
    shutil.rmtree(base, ignore_errors=True)


def main():
    import metabuli_amd as M
    args = sys.argv[1:]
    L = []
    ctx = M.Context(0)
    taxdir = tempfile.mkdtemp(prefix="mtb_merge_measure_tax_")
    if args and args[0] == "big":
        out_md = args[2] if len(args) > 2 else None
        big(M, ctx, taxdir, float(args[1]) if len(args) > 1 else 2.5e9, L)
    else:
        n = int(float(args[0])) if args else 200_000_000
        out_md = args[1] if len(args) > 1 else None
        ks = [int(x) for x in args[2].split(",")] if len(args) > 2 else [2, 8]
        compare(M, ctx, taxdir, ks, n, int(args[3]) if len(args) > 3 else 3, L)
    ctx.close()
    shutil.rmtree(taxdir, ignore_errors=True)
    text = "\n".join(L)
    print(text)
    if out_md:
        os.makedirs(os.path.dirname(os.path.abspath(out_md)), exist_ok=True)
        open(out_md, "w").write(text + "\n")


if __name__ == "__main__":
    main()
