/* merge_plan.h -- which parts of a database's files decode on their own, from its `split` table and file sizes alone: the checkpoint
 * record, the checkpoints a reader may start from, the range of the files between two of them, and the planners built on those -- the
 * value ranges of a streamed merge (mtb_merge_databases), the partitions of an open (mtb_index_open_part).  Pure host C++, no HIP.
 *
 * A `split` checkpoint {ad, diff_off, info_off} sits on the FIRST entry of an amino-acid group (IndexCreator.cpp:848-857): entry
 * info_off - 1 has the value ad, the 16-bit words behind it start at diff_off.  So every entry whose amino-acid part is at least
 * ad's lies at or behind the checkpoint, and a database can be opened mid-stream there (KmerMatcher.cpp:157-205 does).
 *
 * The merge plan cuts the value axis into ranges [lo, hi) whose bounds are amino-acid parts (ad & ~0xFFFFFF) of checkpoints of ANY
 * input.  For one input a range is read from that input's last checkpoint at or below lo to its first checkpoint at or above hi (the
 * file's ends where there is none): a slice that may over-read at both ends and is trimmed on the device.  The cost of a range is the
 * sum of its slices' entries -- exact, from info_off -- and is kept at or below the budget (and below 2^32: the device dedup counts in
 * 32 bits).  Every entry of every input falls in exactly one range, because the ranges tile [0, 2^64).  A database whose split
 * table is empty or all zero (a small one) is a single interval: it is read whole for every range. */
#ifndef MTB_MERGE_PLAN_H
#define MTB_MERGE_PLAN_H
#include <algorithm>
#include <cstdint>
#include <vector>

namespace mtbhost {

struct MergeCheckpoint { uint64_t ad, diff_off, info_off; };       /* one record of `split`, as it lies in the file */
static_assert(sizeof(MergeCheckpoint) == 24, "the split file is an array of these");
struct MergeInput {
    std::vector<MergeCheckpoint> cps;      /* the usable checkpoints, amino-acid parts strictly ascending */
    uint64_t n_entries = 0, n_words = 0;   /* entries of info, 16-bit words of diffIdx */
};
/* a range of a database's files that can be decoded on its own (named for its first user, the slice of a merge range; also a
 * partition of an open and a slice the writer looks at again): words [diff_lo, diff_hi) of diffIdx code entries [info_lo + lead, info_hi + drop_last); with `lead` entry
 * info_lo is the checkpoint's own (value first_value, not coded in the word range); with `drop_last` one entry more is coded than
 * belongs to the range */
struct MergeSlice {
    uint64_t lead = 0, first_value = 0, diff_lo = 0, diff_hi = 0, info_lo = 0, info_hi = 0; bool drop_last = false;
    uint64_t records() const { return info_hi - info_lo; }
    uint64_t words() const { return diff_hi - diff_lo; }
    uint64_t coded_entries() const { return records() - lead + (drop_last ? 1 : 0); }       /* end words in the word range */
};
struct MergeRange {
    uint64_t lo = 0, hi = UINT64_MAX;      /* hi == UINT64_MAX: open */
    uint64_t records = 0;                  /* sum of the slices' entries */
    std::vector<MergeSlice> slices;        /* one per input */
};
enum { MERGE_PLAN_OK = 0, MERGE_PLAN_CAPACITY = 1 };

inline uint64_t merge_aa(uint64_t value) { return value & ~0xFFFFFFull; }

/* the checkpoints of a raw split table a reader may start from: record 0 and unused records are zero; a record that points outside
 * the files, or whose entry or amino-acid part does not ascend, is ignored */
inline void merge_input_from_split(const MergeCheckpoint *split, size_t n_split, uint64_t n_entries, uint64_t n_words, MergeInput *in) {
    in->cps.clear(); in->n_entries = n_entries; in->n_words = n_words;
    uint64_t last_info = 0, last_aa = 0; bool any = false;
    for (size_t i = 1; i < n_split; i++) {
        const MergeCheckpoint &s = split[i];
        if (s.ad == 0 || s.ad == UINT64_MAX || s.info_off <= last_info || s.info_off > n_entries || s.diff_off > n_words) continue;
        if (any && merge_aa(s.ad) <= last_aa) continue;
        in->cps.push_back(s); last_info = s.info_off; last_aa = merge_aa(s.ad); any = true;
    }
}

inline MergeSlice merge_slice(const MergeInput &in, uint64_t lo, uint64_t hi) {
    MergeSlice s;
    /* last checkpoint whose amino-acid part is <= lo */
    auto above_lo = std::upper_bound(in.cps.begin(), in.cps.end(), lo, [](uint64_t v, const MergeCheckpoint &c) { return v < merge_aa(c.ad); });
    if (above_lo != in.cps.begin()) { const MergeCheckpoint &c = *(above_lo - 1); s.lead = 1; s.first_value = c.ad; s.diff_lo = c.diff_off; s.info_lo = c.info_off - 1; }
    s.diff_hi = in.n_words; s.info_hi = in.n_entries;
    if (hi != UINT64_MAX) {
        /* first checkpoint whose amino-acid part is >= hi */
        auto at_hi = std::lower_bound(in.cps.begin(), in.cps.end(), hi, [](const MergeCheckpoint &c, uint64_t v) { return merge_aa(c.ad) < v; });
        if (at_hi != in.cps.end()) { s.drop_last = true; s.diff_hi = at_hi->diff_off; s.info_hi = at_hi->info_off - 1; }
    }
    return s;
}

/* How a database (its raw split table and file sizes) is cut into n_parts value ranges for mtb_index_open_part: with the file start
 * as element 0 of the U usable checkpoints, partition p starts at element p * U / n_parts; one whose start is the next one's too is
 * empty and inherits the next partition's bound (UINT64_MAX behind the last entry).  A non-empty partition is merge_slice of its
 * bound and the next partition's: no amino-acid group straddles a cut. */
struct PartPlan {
    struct Part { bool empty = true; MergeSlice r; };
    std::vector<Part> parts;
    std::vector<uint64_t> bounds;          /* lower amino-acid-part bound of every partition */
};
inline void plan_parts(const std::vector<MergeCheckpoint> &split, uint64_t n_entries, uint64_t n_words, uint32_t n_parts, PartPlan *plan) {
    MergeInput in;
    merge_input_from_split(split.data(), split.size(), n_entries, n_words, &in);
    plan->parts.assign(n_parts, PartPlan::Part()); plan->bounds.assign(n_parts, UINT64_MAX);
    const uint64_t U = in.cps.size() + 1;
    auto k = [&](uint32_t p) { return (size_t)((uint64_t)p * U / n_parts); };
    uint64_t next = UINT64_MAX;            /* the bound of the partition behind p */
    for (uint32_t p = n_parts; p-- > 0;) {
        if (k(p) != k(p + 1) && n_entries != 0) {
            const uint64_t lo = k(p) == 0 ? 0 : merge_aa(in.cps[k(p) - 1].ad);
            plan->parts[p].empty = false; plan->parts[p].r = merge_slice(in, lo, next);
            next = lo;
        }
        plan->bounds[p] = next;
    }
    if (n_entries == 0) plan->bounds[0] = 0;
}

inline uint64_t merge_cost(const std::vector<MergeInput> &in, uint64_t lo, uint64_t hi) {
    uint64_t c = 0;
    for (const MergeInput &x : in) c += merge_slice(x, lo, hi).records();
    return c;
}

/* max_range_records: the budget (values of 2^32 and above count as 2^32 - 1).  MERGE_PLAN_CAPACITY: one step between neighbouring
 * bounds does not fit; *needed = its records. */
inline int merge_plan(const std::vector<MergeInput> &in, uint64_t max_range_records, std::vector<MergeRange> *out, uint64_t *needed) {
    out->clear(); *needed = 0;
    const uint64_t budget = std::min<uint64_t>(max_range_records, 0xFFFFFFFFull);
    std::vector<uint64_t> cand;
    for (const MergeInput &x : in) for (const MergeCheckpoint &c : x.cps) if (merge_aa(c.ad) != 0) cand.push_back(merge_aa(c.ad));
    std::sort(cand.begin(), cand.end()); cand.erase(std::unique(cand.begin(), cand.end()), cand.end());
    cand.push_back(UINT64_MAX);                                       /* the open end */
    auto emit = [&](uint64_t lo, uint64_t hi) {
        MergeRange r; r.lo = lo; r.hi = hi;
        for (const MergeInput &x : in) { r.slices.push_back(merge_slice(x, lo, hi)); r.records += r.slices.back().records(); }
        out->push_back(std::move(r));
    };
    uint64_t lo = 0; bool have_best = false; uint64_t best = 0;
    for (size_t k = 0; k < cand.size();) {
        const uint64_t c = merge_cost(in, lo, cand[k]);
        if (c <= budget) { best = cand[k]; have_best = true; k++; continue; }
        if (!have_best) { *needed = c; out->clear(); return MERGE_PLAN_CAPACITY; }
        emit(lo, best); lo = best; have_best = false;                   /* cand[k] is tried again from the new lower bound */
    }
    emit(lo, UINT64_MAX);
    return MERGE_PLAN_OK;
}

} // namespace mtbhost
#endif
