/* merge_plan_check -- the range planner of the streamed merge (metabuli_amd/csrc/host/merge_plan.h) on seeded random databases.
 * Stand-alone, host only.  Every database is a sorted value list with the split table mtb_index_write's rule gives it (a checkpoint
 * armed at every size_of_split-th entry, recorded at the first later entry of another amino-acid part); 1 to 9 of them, with empty
 * and all-zero tables and very different checkpoint densities, are planned under several budgets.  Checked: bounds ascend, are
 * amino-acid aligned and tile [0, 2^64); every range's records are the sum of its slices and within the budget; every entry of every
 * input lies inside its input's slice of the one range that holds its value; a slice starts and ends where its checkpoints say; the
 * CAPACITY case names the records of the step that does not fit, and that budget then plans; a set of inputs without checkpoints is
 * one interval.
 * The partition planner of an open (plan_parts) runs on the same databases: for 1, 2, 3, 8, 16 and more partitions than there are
 * checkpoints its ranges and bounds equal, field for field, those of the arithmetic it replaced (restated below as the specification),
 * and every non-empty partition is merge_slice of its bounds; tables with out-of-file and non-ascending records are a case of their
 * own.  Prints "OK <plans>" or the first failure. */
#include <cstdio>
#include <cstdlib>
#include <random>
#include "../../metabuli_amd/csrc/host/merge_plan.h"

using namespace mtbhost;

struct Db { std::vector<uint64_t> v, word_behind; std::vector<MergeCheckpoint> split; MergeInput in; };

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { if (fails++ < 10) { printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #c); printf(__VA_ARGS__); printf("\n"); } } } while (0)

static Db make_db(std::mt19937_64 &rng, uint64_t n, int split_num, uint64_t aa_span, int table) {
    Db d;
    for (uint64_t i = 0; i < n; i++) d.v.push_back(((rng() % aa_span + 1) << 24) | (rng() & 0xFFFFFF));
    std::sort(d.v.begin(), d.v.end());
    uint64_t w = 0;
    for (uint64_t i = 0; i < n; i++) { w += 1 + rng() % 5; d.word_behind.push_back(w); }
    d.split.assign((size_t)split_num, MergeCheckpoint{0, 0, 0});
    if (table == 1) d.split.clear();                                 /* no table at all */
    const uint64_t sos = n / (uint64_t)(split_num - 1);
    if (table == 0 && sos) {
        size_t at = 0; uint64_t last = UINT64_MAX;
        for (uint64_t k = 1; k <= n / sos && at + 1 < (size_t)split_num; k++) {
            uint64_t j = k * sos;                                    /* armed at j - 1 */
            while (j < n && merge_aa(d.v[j]) == merge_aa(d.v[k * sos - 1])) j++;
            if (j < n && j != last) { d.split[++at] = MergeCheckpoint{d.v[j], d.word_behind[j], j + 1}; last = j; }
        }
    }
    merge_input_from_split(d.split.data(), d.split.size(), n, w, &d.in);
    return d;
}

static void check_plan(const std::vector<Db> &dbs, const std::vector<MergeRange> &R, uint64_t budget) {
    CHECK(!R.empty() && R.front().lo == 0 && R.back().hi == UINT64_MAX, "ends");
    for (size_t r = 0; r < R.size(); r++) {
        CHECK(R[r].lo < R[r].hi && (R[r].lo & 0xFFFFFF) == 0, "range %zu", r);
        if (r + 1 < R.size()) CHECK(R[r].hi == R[r + 1].lo && (R[r].hi & 0xFFFFFF) == 0, "range %zu does not meet the next", r);
        uint64_t sum = 0;
        CHECK(R[r].slices.size() == dbs.size(), "slices");
        for (size_t i = 0; i < dbs.size(); i++) {
            const MergeSlice &s = R[r].slices[i]; const Db &d = dbs[i];
            sum += s.records();
            CHECK(s.info_lo <= s.info_hi && s.info_hi <= d.v.size() && s.diff_lo <= s.diff_hi && s.diff_hi <= d.in.n_words, "slice %zu/%zu", r, i);
            if (s.lead) CHECK(s.info_lo < d.v.size() && s.first_value == d.v[s.info_lo] && s.diff_lo == d.word_behind[s.info_lo] && merge_aa(s.first_value) <= R[r].lo, "lead %zu/%zu", r, i);
            else CHECK(s.info_lo == 0 && s.diff_lo == 0, "head %zu/%zu", r, i);
            if (s.drop_last) CHECK(s.info_hi < d.v.size() && s.diff_hi == d.word_behind[s.info_hi] && merge_aa(d.v[s.info_hi]) >= R[r].hi, "drop_last %zu/%zu", r, i);
            else CHECK(s.info_hi == d.v.size() && s.diff_hi == d.in.n_words, "tail %zu/%zu", r, i);
        }
        CHECK(sum == R[r].records && sum <= budget && sum < (1ull << 32), "range %zu: %llu records, budget %llu", r, (unsigned long long)sum, (unsigned long long)budget);
    }
    /* every entry: inside its input's slice of the one range that holds its value */
    for (size_t i = 0; i < dbs.size(); i++)
        for (uint64_t e = 0; e < dbs[i].v.size(); e++) {
            size_t holders = 0;
            for (size_t r = 0; r < R.size(); r++) {
                const bool in_range = dbs[i].v[e] >= R[r].lo && (R[r].hi == UINT64_MAX || dbs[i].v[e] < R[r].hi);
                if (!in_range) continue;
                holders++;
                CHECK(e >= R[r].slices[i].info_lo && e < R[r].slices[i].info_hi, "entry %llu of input %zu is outside its slice of range %zu", (unsigned long long)e, i, r);
            }
            CHECK(holders == 1, "entry %llu of input %zu lies in %zu ranges", (unsigned long long)e, i, holders);
        }
}

/* ---- the partitions of an open (plan_parts) ----
 * THE SPECIFICATION: the arithmetic mtb_index_open_part used before the planner moved into the header, restated literally (its own
 * lenient checkpoint rule, its own fields).  Kept here, not shared with the header. */
struct SpecPart { bool empty = true, explicit_first = false, drop_last = false; uint64_t ad = 0, diff_lo = 0, diff_hi = 0, info_lo = 0, info_hi = 0; };
struct SpecPlan { std::vector<SpecPart> parts; std::vector<uint64_t> bounds; };
static SpecPlan spec_plan_parts(const std::vector<MergeCheckpoint> &sp, uint64_t T, uint64_t n16, uint32_t n_parts) {
    SpecPlan plan;
    std::vector<MergeCheckpoint> use; use.push_back(MergeCheckpoint{0, 0, 0});
    if (n_parts > 1)
        for (size_t i = 1; i < sp.size(); i++) if (sp[i].ad != 0 && sp[i].ad != UINT64_MAX && sp[i].info_off > use.back().info_off) use.push_back(sp[i]);
    plan.parts.assign(n_parts, SpecPart()); plan.bounds.assign(n_parts, UINT64_MAX);
    const size_t U = use.size();
    std::vector<size_t> k(n_parts + 1);
    for (uint32_t p = 0; p <= n_parts; p++) k[p] = (size_t)((uint64_t)p * U / n_parts);
    for (uint32_t p = 0; p < n_parts; p++) {
        SpecPart &P = plan.parts[p];
        if (k[p] == k[p + 1] || T == 0) continue;
        P.empty = false;
        const MergeCheckpoint &s0 = use[k[p]];
        if (k[p] == 0) { P.explicit_first = false; P.ad = 0; P.diff_lo = 0; P.info_lo = 0; }
        else { P.explicit_first = true; P.ad = s0.ad; P.diff_lo = s0.diff_off; P.info_lo = s0.info_off - 1; }
        if (k[p + 1] >= U) { P.drop_last = false; P.diff_hi = n16; P.info_hi = T; }
        else { P.drop_last = true; P.diff_hi = use[k[p + 1]].diff_off; P.info_hi = use[k[p + 1]].info_off - 1; }
        plan.bounds[p] = k[p] == 0 ? 0 : (s0.ad & ~0xFFFFFFull);
    }
    for (int64_t p = (int64_t)n_parts - 2; p >= 0; p--) if (plan.parts[(size_t)p].empty) plan.bounds[(size_t)p] = plan.bounds[(size_t)p + 1];
    if (T == 0) plan.bounds[0] = 0;
    return plan;
}
static bool same_range(const MergeSlice &a, const MergeSlice &b) {
    return a.lead == b.lead && a.first_value == b.first_value && a.diff_lo == b.diff_lo && a.diff_hi == b.diff_hi && a.info_lo == b.info_lo && a.info_hi == b.info_hi &&
           a.drop_last == b.drop_last;
}
/* the planner against the specification on one well-formed database, for every n_parts of the issue's list */
static unsigned check_parts(const Db &d) {
    const uint64_t T = d.v.size(), n16 = d.in.n_words;
    /* the precondition of the comparison: both checkpoint rules keep the same records of this table */
    size_t lenient = 0; uint64_t last = 0;
    for (size_t i = 1; i < d.split.size(); i++) if (d.split[i].ad != 0 && d.split[i].ad != UINT64_MAX && d.split[i].info_off > last) { lenient++; last = d.split[i].info_off; }
    CHECK(lenient == d.in.cps.size(), "the table is not well-formed: %zu records under the old rule, %zu under the new", lenient, d.in.cps.size());
    unsigned plans = 0;
    for (uint32_t n_parts : {1u, 2u, 3u, 8u, 16u, (uint32_t)d.in.cps.size() + 5u}) {
        const SpecPlan S = spec_plan_parts(d.split, T, n16, n_parts);
        PartPlan N;
        plan_parts(d.split, T, n16, n_parts, &N);
        plans++;
        CHECK(N.parts.size() == n_parts && N.bounds.size() == n_parts, "sizes");
        if (N.parts.size() != n_parts || N.bounds.size() != n_parts) continue;
        for (uint32_t p = 0; p < n_parts; p++) {
            const SpecPart &s = S.parts[p]; const MergeSlice &r = N.parts[p].r;
            CHECK(N.bounds[p] == S.bounds[p], "bound %u of %u: %llx, specification %llx", p, n_parts, (unsigned long long)N.bounds[p], (unsigned long long)S.bounds[p]);
            CHECK(N.parts[p].empty == s.empty, "emptiness of partition %u of %u", p, n_parts);
            if (s.empty || N.parts[p].empty) continue;
            CHECK(r.lead == (s.explicit_first ? 1u : 0u) && r.first_value == s.ad && r.diff_lo == s.diff_lo && r.diff_hi == s.diff_hi && r.info_lo == s.info_lo &&
                  r.info_hi == s.info_hi && r.drop_last == s.drop_last, "partition %u of %u differs from the specification", p, n_parts);
            uint64_t hi = UINT64_MAX;
            for (uint32_t q = n_parts; q-- > p + 1;) if (!N.parts[q].empty) hi = N.bounds[q];
            CHECK(same_range(r, merge_slice(d.in, N.bounds[p], hi)), "partition %u of %u is not merge_slice of its bounds", p, n_parts);
            CHECK(r.coded_entries() == r.records() - r.lead + (r.drop_last ? 1 : 0) && r.words() == r.diff_hi - r.diff_lo, "range arithmetic");
        }
    }
    return plans;
}
/* damaged tables: records that point outside the files, whose entries or amino-acid parts do not ascend, unused and ~0 records.  With
 * one partition per element the planner starts partition p at its (p - 1)-th checkpoint: these must be merge_input_from_split's */
static unsigned check_damaged_parts(std::mt19937_64 &rng) {
    unsigned plans = 0;
    for (int round = 0; round < 200; round++) {
        const uint64_t T = 1 + rng() % 3000, n16 = T + rng() % (4 * T);
        std::vector<MergeCheckpoint> split(1 + rng() % 40, MergeCheckpoint{0, 0, 0});
        uint64_t ad = 0, info = 0, word = 0;
        for (size_t i = 1; i < split.size(); i++) {
            ad += (1 + rng() % 1000) << 24; info += 1 + rng() % (T / 8 + 1); word += 1 + rng() % (n16 / 8 + 1);
            MergeCheckpoint c{ad | (rng() & 0xFFFFFF), word, info};
            switch (rng() % 8) {
            case 0: c.info_off = T + 1 + rng() % 100; break;                          /* behind info */
            case 1: c.diff_off = n16 + 1 + rng() % 100; break;                        /* behind diffIdx */
            case 2: c.ad = ((1 + rng() % (ad >> 24)) << 24) | 5; break;               /* an amino-acid part that (mostly) does not ascend */
            case 3: c.info_off = 1 + rng() % info; break;                             /* an entry that (mostly) does not ascend */
            case 4: c = MergeCheckpoint{0, 0, 0}; break;
            case 5: c.ad = UINT64_MAX; break;
            default: break;
            }
            split[i] = c;
        }
        MergeInput in;
        merge_input_from_split(split.data(), split.size(), T, n16, &in);
        const uint32_t n_parts = (uint32_t)in.cps.size() + 1;
        PartPlan N;
        plan_parts(split, T, n16, n_parts, &N);
        plans++;
        CHECK(N.parts.size() == n_parts && !N.parts[0].empty && N.parts[0].r.lead == 0 && N.parts[0].r.diff_lo == 0 && N.parts[0].r.info_lo == 0 && N.bounds[0] == 0, "head");
        for (uint32_t p = 0; p < n_parts; p++) {
            const MergeSlice &r = N.parts[p].r;
            CHECK(!N.parts[p].empty && r.info_lo <= r.info_hi && r.info_hi <= T && r.diff_lo <= r.diff_hi && r.diff_hi <= n16, "partition %u of %u leaves the files", p, n_parts);
            if (p == 0) continue;
            const MergeCheckpoint &c = in.cps[p - 1];
            CHECK(r.lead == 1 && r.first_value == c.ad && r.diff_lo == c.diff_off && r.info_lo == c.info_off - 1 && N.bounds[p] == merge_aa(c.ad), "partition %u does not start at kept checkpoint %u", p, p - 1);
            const MergeSlice &before = N.parts[p - 1].r;
            CHECK(before.drop_last && before.diff_hi == c.diff_off && before.info_hi == c.info_off - 1, "partition %u does not end at kept checkpoint %u", p - 1, p - 1);
        }
        CHECK(!N.parts[n_parts - 1].r.drop_last && N.parts[n_parts - 1].r.info_hi == T && N.parts[n_parts - 1].r.diff_hi == n16, "tail");
    }
    return plans;
}

int main() {
    std::mt19937_64 rng(20240611);
    unsigned plans = 0, capacity_seen = 0, multi = 0, part_plans = 0;
    unsigned no_table = 0, zero_table = 0, one_cp = 0, sparse = 0, dense = 0;      /* the shapes of table plan_parts met */
    auto parts_of = [&](const Db &d) {
        part_plans += check_parts(d);
        if (d.split.empty()) no_table++;
        else if (d.in.cps.empty()) zero_table++;
        else if (d.in.cps.size() == 1) one_cp++;
        else if (d.in.cps.size() <= 8) sparse++;
        else if (d.in.cps.size() >= 64) dense++;
    };
    const uint64_t sizes[] = {0, 1, 50, 700, 5000};
    const int split_nums[] = {2, 5, 64, 4096};
    for (int trial = 0; trial < 60; trial++) {
        const size_t k = 1 + (size_t)(trial % 9);
        std::vector<Db> dbs; std::vector<MergeInput> in;
        uint64_t total = 0;
        for (size_t i = 0; i < k; i++) {
            const int table = rng() % 5 == 0 ? 1 + (int)(rng() % 2) : 0;           /* 1: no table, 2: all zero */
            dbs.push_back(make_db(rng, sizes[rng() % 5], split_nums[rng() % 4], (rng() % 3 == 0) ? 40 : 100000, table));
            in.push_back(dbs.back().in); total += dbs.back().v.size();
            parts_of(dbs.back());
        }
        for (uint64_t budget : {UINT64_MAX, total, total / 2 + 1, total / 7 + 1, (uint64_t)37, (uint64_t)1}) {
            std::vector<MergeRange> R; uint64_t needed = 0;
            const int st = merge_plan(in, budget, &R, &needed);
            plans++;
            if (st == MERGE_PLAN_CAPACITY) {
                capacity_seen++;
                CHECK(needed > budget && R.empty(), "CAPACITY with %llu needed under budget %llu", (unsigned long long)needed, (unsigned long long)budget);
                /* the largest step any lower bound meets is what a retry may need: growing the budget to each `needed` in turn ends in a plan */
                uint64_t b = needed; int tries = 0;
                while ((merge_plan(in, b, &R, &needed)) == MERGE_PLAN_CAPACITY && tries++ < 100000) { CHECK(needed > b, "needed does not grow"); b = needed; }
                CHECK(!R.empty() && b <= total, "no plan under %llu", (unsigned long long)b);
                check_plan(dbs, R, b);
            } else {
                CHECK(budget >= total ? R.size() == 1 : true, "a budget that holds everything gives one range, not %zu", R.size());
                if (R.size() > 1) multi++;
                check_plan(dbs, R, std::min<uint64_t>(budget, 0xFFFFFFFFull));
            }
        }
    }
    {   /* inputs without checkpoints are one interval: one range if everything fits, CAPACITY with the whole count otherwise */
        std::vector<Db> dbs; std::vector<MergeInput> in;
        for (int i = 0; i < 3; i++) { dbs.push_back(make_db(rng, 100, 64, 1000, 1 + i % 2)); in.push_back(dbs.back().in); CHECK(in.back().cps.empty(), "table"); }
        std::vector<MergeRange> R; uint64_t needed = 0;
        CHECK(merge_plan(in, 300, &R, &needed) == MERGE_PLAN_OK && R.size() == 1 && R[0].records == 300, "single interval");
        check_plan(dbs, R, 300);
        CHECK(merge_plan(in, 299, &R, &needed) == MERGE_PLAN_CAPACITY && needed == 300, "single interval: needed %llu", (unsigned long long)needed);
        plans += 2;
    }
    {   /* a budget of 2^32 and above counts as 2^32 - 1 */
        MergeInput big; big.n_entries = 3ull << 31; big.n_words = 3ull << 31;
        std::vector<MergeRange> R; uint64_t needed = 0;
        CHECK(merge_plan({big}, UINT64_MAX, &R, &needed) == MERGE_PLAN_CAPACITY && needed == (3ull << 31), "2^32 cap");
        big.cps.push_back(MergeCheckpoint{5ull << 24, 3ull << 30, (3ull << 30) + 1});
        CHECK(merge_plan({big}, UINT64_MAX, &R, &needed) == MERGE_PLAN_OK && R.size() == 2 && R[0].records == (3ull << 30) && R[1].records == (3ull << 30), "two halves below 2^32");
        plans += 2;
    }
    for (uint64_t n : {0, 1, 2, 50, 700}) for (int split_num : {2, 3, 5}) for (int table : {0, 1, 2}) parts_of(make_db(rng, n, split_num, 100000, table));
    for (int rep = 0; rep < 12; rep++) { parts_of(make_db(rng, 50 + 2 * rep, 3, 100000, 0)); parts_of(make_db(rng, 3000 + 100 * rep, 512, 100000, 0)); }      /* one checkpoint; dense */
    CHECK(no_table > 10 && zero_table > 10 && one_cp > 10 && sparse > 10 && dense > 10, "plan_parts did not reach the cases: %u without a table, %u all zero, %u with one checkpoint, %u sparse, %u dense",
          no_table, zero_table, one_cp, sparse, dense);
    part_plans += check_damaged_parts(rng);
    CHECK(part_plans > 1000, "%u partition plans", part_plans);
    CHECK(capacity_seen > 10 && multi > 10, "the trials did not reach the cases: %u CAPACITY, %u multi-range", capacity_seen, multi);
    if (fails) { printf("%d failures\n", fails); return 1; }
    printf("OK %u\n", plans);
    return 0;
}
