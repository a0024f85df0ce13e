"""One mtb_builder_finish of a synthetic input, by stage, next to the host numpy path on a slice of the same input.

    python profiles/scripts/index_build_measure.py [N_RECORDS=2e8] [OUT.md] [SLICE=1e6]

The input is a pure function of the seed: groups of records that share (value, species), lengths drawn from the heavy-tailed table
BUCKETS below (so the group-length histogram is known by construction and printed exactly), members = random strains of the
group's species (exact duplicates occur), every 20th group repeats its predecessor's value under another species, records shuffled
inside each chunk of 2^24.  Values are valid format-2 words, distinct per group (a bijection of the group number).
Writes a markdown report (stdout, and OUT.md if given): time per stage from mtb_builder_last_finish_stats, the histogram, the
host path (`synth.dedup_targets` style: lexsort, group boundaries, a Python fold with a host LCA) on the first SLICE records'
groups, and a check that the device result on that slice equals the host result.  A single run: no repetitions, no warm-up
beyond the slice build, which runs first."""
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

# (lowest length, highest length, share of the GROUPS)
BUCKETS = [(1, 1, 0.60), (2, 3, 0.20), (4, 7, 0.09), (8, 16, 0.05), (17, 64, 0.035), (65, 256, 0.018), (257, 1024, 0.006), (1025, 2048, 0.001)]
CHUNK = 1 << 24
N_GENERA, SPECIES_PER_GENUS = 4, 8          # species j of a genus has 16 << j strains (16 .. 2048)


def make_taxonomy(d):
    from metabuli_amd import synth
    tax = synth.Taxonomy()
    tax.add(1, 1, "no rank", "root"); tax.add(2, 1, "superkingdom", "Bacteria")
    nxt = 10
    first, count = [], []                        # per species: first strain id, strains
    for g in range(N_GENERA):
        gid = nxt; nxt += 1
        tax.add(gid, 2, "genus", f"G{g}")
        for j in range(SPECIES_PER_GENUS):
            sid = nxt; nxt += 1
            tax.add(sid, gid, "species", f"G{g} s{j}")
            n = 16 << j
            for t in range(nxt, nxt + n):
                tax.add(t, sid, "no rank", f"strain{t}")
            first.append(nxt); count.append(n); nxt += n
    tax.write(d)
    return tax, np.array(first, np.int64), np.array(count, np.int64)


def group_lengths(rng, n):
    """lengths of whole groups that sum to exactly n (the last one is cut)"""
    share = np.array([b[2] for b in BUCKETS]); share = share / share.sum()
    mean = sum(s * (lo + hi) / 2 for (lo, hi, _), s in zip(BUCKETS, share))
    lens = np.zeros(0, np.int64)
    while lens.sum() < n:
        g = int((n - lens.sum()) / mean * 1.05) + 16
        b = rng.choice(len(BUCKETS), size=g, p=share)
        lo = np.array([x[0] for x in BUCKETS])[b]; hi = np.array([x[1] for x in BUCKETS])[b]
        lens = np.concatenate([lens, rng.integers(lo, hi + 1)])
    cs = np.cumsum(lens)
    k = int(np.searchsorted(cs, n))
    lens = lens[:k + 1].copy()
    lens[k] -= cs[k] - n
    assert lens.sum() == n and (lens > 0).all()
    return lens


def group_values(g):
    """a distinct valid format-2 word per group number: 24 DNA bits, eight 5-bit amino-acid letters (0 .. 20) above them"""
    g = g.astype(np.uint64)
    x = (g * np.uint64(0x9E3779B97F4A7C15)) & np.uint64((1 << 39) - 1)          # odd multiplier: a bijection on 39 bits
    v = (x & np.uint64(0x7FFFFF)) | np.uint64(1 << 23)                          # DNA part: bit 23 set, so never the lowest word
    for k in range(4):                                                          # letters 4 .. 7 from the bijection (0 .. 15)
        v |= ((x >> np.uint64(23 + 4 * k)) & np.uint64(15)) << np.uint64(24 + 5 * (4 + k))
    h = g * np.uint64(0xD6E8FEB86659FD93)
    for k in range(4):                                                          # letters 0 .. 3: any valid letter
        v |= (((h >> np.uint64(20 + 8 * k)) & np.uint64(255)) % np.uint64(21)) << np.uint64(24 + 5 * k)
    return v


def records(rng, lens, g0, first, count):
    """(values, taxids, species index per group) of groups g0 .. g0 + len(lens)"""
    G = len(lens)
    gn = np.arange(g0, g0 + G, dtype=np.int64)
    sp = rng.integers(0, len(first), size=G)
    rep = (gn % 20 == 19) & (np.arange(G) > 0)                                  # repeats the predecessor's value under another species
    sp[rep] = (sp[np.flatnonzero(rep) - 1] + 1) % len(first)
    vg = group_values(np.where(rep, gn - 1, gn))
    spr = np.repeat(sp, lens)
    tids = (first[spr] + (rng.random(len(spr)) * count[spr]).astype(np.int64)).astype(np.int32)
    vals = np.repeat(vg, lens)
    return vals, tids


def host_path(tax, vals, tids):
    """synth.dedup_targets without the world: lexsort, boundaries on (value, species), a Python fold with the host LCA"""
    sp_of = {int(t): tax.species_of(int(t)) for t in np.unique(tids)}
    sps = np.array([sp_of[int(t)] for t in tids], np.int32)
    order = np.lexsort((tids, sps, vals))
    vals, tids, sps = vals[order], tids[order], sps[order]
    new = np.ones(len(vals), bool)
    new[1:] = (vals[1:] != vals[:-1]) | (sps[1:] != sps[:-1])
    starts = np.flatnonzero(new); ends = np.append(starts[1:], len(vals))
    out_t = tids[starts].copy()
    for gi in np.flatnonzero(ends - starts > 1):
        t = int(tids[starts[gi]])
        for j in range(starts[gi] + 1, ends[gi]):
            if int(tids[j]) != t:
                t = tax.lca(t, int(tids[j]))
        out_t[gi] = t
    return vals[starts], out_t


def main():
    import metabuli_amd as M
    n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 200_000_000
    out_md = sys.argv[2] if len(sys.argv) > 2 else None
    n_slice = int(float(sys.argv[3])) if len(sys.argv) > 3 else 1_000_000
    assert n < 1 << 32
    taxdir = tempfile.mkdtemp(prefix="mtb_build_measure_tax_")
    tax, first, count = make_taxonomy(taxdir)
    rng = np.random.default_rng(2024)
    lens = group_lengths(rng, n)
    ctx = M.Context(0)
    b = ctx.builder(taxdir, M.default_params(seq_mode=1, syncmer=1, kmer_format=2))

    # the slice: whole groups from the front of the input, on the host and on the device
    gs = int(np.searchsorted(np.cumsum(lens), n_slice, side="right"))
    gs = max(gs, 1)
    sv, st = records(np.random.default_rng(1), lens[:gs], 0, first, count)
    p = np.random.default_rng(2).permutation(len(sv)); sv, st = sv[p], st[p]
    t0 = time.perf_counter()
    hv, ht = host_path(tax, sv, st)
    host_s = time.perf_counter() - t0
    b.add_records(sv, st)
    ix = b.finish()
    gv, gi = ix.download()
    ix.close()
    slice_stats = b.last_finish_stats()
    same = len(gv) == len(hv) and bool((gv == hv).all()) and bool((gi == ht.astype(np.uint32)).all())

    # the whole input, about 2^24 records (whole groups) per add_records call, each chunk from its own seeded generator
    cs = np.cumsum(lens)
    t0 = time.perf_counter()
    g0 = 0
    k = 0
    while g0 < len(lens):
        base = cs[g0 - 1] if g0 else 0
        g1 = max(int(np.searchsorted(cs, base + CHUNK, side="right")), g0 + 1)
        v, t = records(np.random.default_rng(1000 + k), lens[g0:g1], g0, first, count)
        p = np.random.default_rng(5000 + k).permutation(len(v))
        b.add_records(v[p], t[p])
        g0 = g1; k += 1
        print(f"added {b.num_records} of {n} records", file=sys.stderr, flush=True)
    add_s = time.perf_counter() - t0
    assert b.num_records == n
    t0 = time.perf_counter()
    ix = b.finish()
    finish_wall_s = time.perf_counter() - t0
    s = b.last_finish_stats()
    n_entries = ix.num_targets
    ix.close(); b.close(); ctx.close()
    shutil.rmtree(taxdir, ignore_errors=True)

    L = []
    L.append(f"input: {n} records in {len(lens)} groups (generator seed 2024), {k} add_records calls; taxonomy: {N_GENERA} genera x {SPECIES_PER_GENUS} species, "
             f"16 .. 2048 strains each ({int(count.sum())} strains, highest id {int(first[-1] + count[-1] - 1)})")
    L.append("")
    L.append("| group length | groups | records | share of records |")
    L.append("|---|---|---|---|")
    for lo, hi, _ in BUCKETS:
        m = (lens >= lo) & (lens <= hi)
        L.append(f"| {lo}{'' if hi == lo else ' .. ' + str(hi)} | {int(m.sum())} | {int(lens[m].sum())} | {100.0 * lens[m].sum() / n:.1f} % |")
    L.append("")
    L.append(f"`mtb_builder_finish`, device time by stage (events), {s['n_records']} records -> {s['n_entries']} entries, {s['n_long_groups']} groups folded by a wavefront:")
    L.append("")
    L.append("| stage | ms | share | ns per record |")
    L.append("|---|---|---|---|")
    for name, label in (("keys", "keys"), ("sort_key", "sort on (species, taxid) + swap"), ("sort_value", "sort on the value"), ("heads_scan", "heads + scan"), ("reduce", "reduce (both tiers)"), ("total", "total")):
        L.append(f"| {label} | {s[name]:.2f} | {100.0 * s[name] / s['total']:.1f} % | {1e6 * s[name] / n:.3f} |")
    L.append("")
    L.append(f"host wall time of the finish() call (taxonomy upload, directory build, workspace release included): {finish_wall_s:.2f} s; "
             f"generating, shuffling and adding the records before it: {add_s:.1f} s")
    L.append("")
    L.append(f"host numpy path on the first {len(sv)} records ({gs} groups): {host_s:.2f} s = {1e9 * host_s / len(sv):.0f} ns per record; "
             f"the device finish of the same slice: {slice_stats['total']:.2f} ms (first launch of every kernel included); results equal: {same}")
    L.append(f"entries of the built index: {n_entries}")
    text = "\n".join(L)
    print(text)
    if out_md:
        os.makedirs(os.path.dirname(os.path.abspath(out_md)), exist_ok=True)
        open(out_md, "w").write(text + "\n")
    assert same, "device and host results differ on the slice"
    assert s["n_long_groups"] == int((lens > 16).sum()) and s["n_entries"] == len(lens) == n_entries


if __name__ == "__main__":
    main()
