"""numpy restatement of mtb_database_audit's report (include/mtb.h) -- test infrastructure, no library code.

Inputs are the bytes of the four files, the taxonomy as dense tables (id -> species, id -> known) and the listed ids; the output is
every field of mtb_audit_report except the times and n_chunks, plus the per-species counts and the text of sp2uniqKmerCnt.  The
delta coder here takes ARBITRARY deltas modulo 2^64: a value that descends can only exist in a file as a delta that wrapped."""
import numpy as np

NONE = (1 << 64) - 1
U64 = np.uint64
REPORT_FIELDS = ("n_words", "n_end_words", "n_trailing_words", "n_info_entries", "n_entries", "n_value_descents", "first_value_descent",
                 "n_group_disorder", "first_group_disorder", "n_unknown_ids", "first_unknown_id", "n_unlisted_ids", "first_unlisted_id",
                 "n_no_species", "n_checkpoints", "n_bad_checkpoints", "first_bad_checkpoint", "n_species", "valid", "canonical")

# rank order of NcbiTaxonomy::findRankIndex (public NCBI ranks; everything else, "no rank" included, is -1)
RANKS = {"forma": 1, "varietas": 2, "subspecies": 3, "species": 4, "species subgroup": 5, "species group": 6, "subgenus": 7, "genus": 8, "subtribe": 9, "tribe": 10,
         "subfamily": 11, "family": 12, "superfamily": 13, "parvorder": 14, "infraorder": 15, "suborder": 16, "order": 17, "superorder": 18, "infraclass": 19,
         "subclass": 20, "class": 21, "superclass": 22, "subphylum": 23, "phylum": 24, "superphylum": 25, "subkingdom": 26, "kingdom": 27, "superkingdom": 28, "domain": 28}


# ---- 15-bit-group coder ------------------------------------------------------------------------------------------------------------
def encode_values(values):
    """diffIdx words of a value list: entry i is coded as (value[i] - value[i-1]) mod 2^64 (value[-1] = 0) in 15-bit groups, most
    significant first, the last one flagged 0x8000; a zero delta is one word"""
    v = np.asarray(values, dtype=U64)
    if len(v) == 0:
        return np.zeros(0, np.uint16)
    with np.errstate(over="ignore"):
        d = v - np.concatenate([np.zeros(1, U64), v[:-1]])
    n = np.ones(len(d), np.int64)
    for bits in (15, 30, 45, 60):
        n += d >= U64(1 << bits)
    end = np.cumsum(n) - 1                                                               # each entry's end word
    out = np.zeros(int(end[-1]) + 1, np.uint16)
    for g in range(5):                                                                   # group g of an entry lies g words before its end word
        sel = n > g
        out[end[sel] - g] = ((d[sel] >> U64(15 * g)) & U64(0x7FFF)).astype(np.uint16) | np.uint16(0x8000 if g == 0 else 0)
    return out


def decode_words(d16):
    """(values of the entries the words code, index of each entry's end word); words behind the last end word code nothing; groups
    above bit 63 fall off, sums wrap modulo 2^64"""
    d16 = np.asarray(d16, dtype=np.uint16)
    ends = np.flatnonzero(d16 & 0x8000)
    if len(ends) == 0:
        return np.zeros(0, U64), ends
    used = d16[:ends[-1] + 1].astype(U64) & U64(0x7FFF)
    entry = np.searchsorted(ends, np.arange(len(used)), side="left")                     # the entry a word belongs to
    back = (ends[entry] - np.arange(len(used))).astype(U64)                              # groups behind it inside its entry
    assert back.max() <= 4, "an entry of more than five words"
    with np.errstate(over="ignore"):
        part = used << (U64(15) * back)
        starts = np.concatenate([[0], ends[:-1] + 1])
        deltas = np.add.reduceat(part, starts)
        return np.cumsum(deltas, dtype=U64), ends


# ---- the taxonomy as tables -----------------------------------------------------------------------------------------------------------
def taxonomy_tables(parent, rank, listed, aliases=None, max_id=None):
    """(species, known): dense tables over [0, max_id].  parent / rank: dicts of a dump-file taxonomy (root is its own parent), aliases:
    merged.dmp {old id: current id}, listed: the ids of taxID_list.  species restates KmerMatcher::loadTaxIdList: every listed id,
    and every node between it and its species, maps to the listed id's first ancestor-or-self of rank species or above."""
    aliases = aliases or {}
    mx = max(list(parent) + list(aliases) + list(aliases.values())) if max_id is None else max_id
    known = np.zeros(mx + 1, bool)
    for t in list(parent) + list(aliases):
        known[t] = True
    canon = lambda t: aliases.get(t, t)
    ridx = lambda t: RANKS.get(rank[t], -1)
    species = np.zeros(mx + 1, np.int32)
    for t in listed:
        t = int(t)
        if t < 0 or t > mx or not known[t]:
            continue
        cur = canon(t)
        if t in (0, 1):
            sp = 0
        else:
            sp, cnt = cur, 0
            while cnt < 30 and ridx(sp) < RANKS["species"]:
                sp = parent[sp]; cnt += 1
            if cnt == 30:
                sp = t
        if t != cur:
            species[t] = sp
        guard = 0
        while cur != sp and guard < 100000:
            species[cur] = sp
            if parent[cur] == cur:
                break
            cur = parent[cur]; guard += 1
        if 0 <= sp <= mx:
            species[sp] = sp
    return species, known


# ---- the report ----------------------------------------------------------------------------------------------------------------------
def usable_checkpoints(split, n_entries, n_words):
    """record numbers of the split records a reader may start from (the rule of merge_input_from_split, host/merge_plan.h)"""
    out, last_info, last_aa, any_ = [], 0, 0, False
    for i in range(1, len(split)):
        ad, diff_off, info_off = (int(x) for x in split[i])
        if ad == 0 or ad == NONE or info_off <= last_info or info_off > n_entries or diff_off > n_words:
            continue
        aa = ad & ~0xFFFFFF
        if any_ and aa <= last_aa:
            continue
        out.append(i); last_info, last_aa, any_ = info_off, aa, True
    return out


def audit(diffidx, info, split, species, known, listed, info_mask=0xFFFFFFFF):
    """-> (report dict, counts uint32[len(species)]).  diffidx / info / split: the files' bytes (or arrays of uint16 / uint32 / uint64)"""
    d16 = np.frombuffer(diffidx, np.uint16) if isinstance(diffidx, (bytes, bytearray)) else np.asarray(diffidx, np.uint16)
    inf = np.frombuffer(info, np.uint32) if isinstance(info, (bytes, bytearray)) else np.asarray(info, np.uint32)
    sp_raw = np.frombuffer(split, U64) if isinstance(split, (bytes, bytearray)) else np.asarray(split, U64).reshape(-1)
    spl = sp_raw[:len(sp_raw) // 3 * 3].reshape(-1, 3)
    mx = len(species) - 1
    is_listed = np.zeros(mx + 1, bool)
    for t in listed:
        if 0 <= int(t) <= mx:
            is_listed[int(t)] = True
    values, ends = decode_words(d16)
    R = dict(n_words=len(d16), n_end_words=len(ends), n_info_entries=len(inf))
    R["n_trailing_words"] = len(d16) - (int(ends[-1]) + 1 if len(ends) else 0)
    n = R["n_entries"] = min(len(ends), len(inf))
    v = values[:n]
    t = (inf[:n] & np.uint32(info_mask)).astype(np.int64)
    in_range = (t >= 0) & (t <= mx)
    tc = np.where(in_range, t, 0)
    kn = in_range & known[tc]
    sp = np.where(kn, species[tc], 0).astype(np.int64)

    def count(mask, name_n, name_first):
        idx = np.flatnonzero(mask)
        R[name_n] = len(idx)
        if name_first:
            R[name_first] = int(idx[0]) if len(idx) else NONE

    prev_lt = np.zeros(n, bool); prev_eq = np.zeros(n, bool)
    if n > 1:
        prev_lt[1:] = v[1:] < v[:-1]
        prev_eq[1:] = (v[1:] == v[:-1]) & (sp[1:] <= sp[:-1])
    count(prev_lt, "n_value_descents", "first_value_descent")
    count(prev_eq, "n_group_disorder", "first_group_disorder")
    count(~kn, "n_unknown_ids", "first_unknown_id")
    count(kn & ~is_listed[tc], "n_unlisted_ids", "first_unlisted_id")
    count(kn & (sp == 0), "n_no_species", None)
    counts = np.bincount(sp[kn & (sp > 0)], minlength=mx + 1).astype(np.uint32)
    R["n_species"] = int((counts > 0).sum())
    # checkpoints: words [0, diff_off) hold exactly info_off end words, word diff_off - 1 is one, value[info_off - 1] == ad
    is_end = (d16 & 0x8000) != 0
    ends_before = np.concatenate([[0], np.cumsum(is_end)])
    use = usable_checkpoints(spl, len(inf), len(d16))
    bad = []
    for i in use:
        ad, diff_off, info_off = (int(x) for x in spl[i])
        good = diff_off >= 1 and int(ends_before[diff_off]) == info_off and bool(is_end[diff_off - 1]) and 1 <= info_off <= len(values) and int(values[info_off - 1]) == ad
        if not good:
            bad.append(i)
    R["n_checkpoints"] = len(use); R["n_bad_checkpoints"] = len(bad); R["first_bad_checkpoint"] = bad[0] if bad else NONE
    R["valid"] = int(R["n_end_words"] == R["n_info_entries"] and R["n_trailing_words"] == 0 and R["n_value_descents"] == 0 and R["n_unknown_ids"] == 0
                     and R["n_bad_checkpoints"] == 0)
    R["canonical"] = int(R["valid"] and R["n_group_disorder"] == 0 and R["n_unlisted_ids"] == 0)
    return R, counts


def species_counts_text(counts):
    """DBDIR/sp2uniqKmerCnt (Classifier.cpp:433-437): "<id> <count>\\n" per non-zero count, ids ascending"""
    return "".join(f"{s} {int(c)}\n" for s, c in enumerate(counts) if c)


def parse_species_counts(text, size):
    """the reference's reader (Classifier.cpp:401-409): `>> taxId >> count` until either fails"""
    out = np.zeros(size, np.uint32)
    tok = text.split()
    for k in range(0, len(tok) - 1, 2):
        try:
            t, c = int(tok[k]), int(tok[k + 1])
        except ValueError:
            break
        if t < size:
            out[t] = c
    return out
