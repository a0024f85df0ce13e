/* merge_plan_check -- the range planner of the streamed merge (metabuli_amd/csrc/host/merge_plan.h) on seeded random databases.
 * Stand-alone, host only.  Every database is a sorted value list with the split table mtb_index_write's rule gives it (a checkpoint
 * armed at every size_of_split-th entry, recorded at the first later entry of another amino-acid part); 1 to 9 of them, with empty
 * and all-zero tables and very different checkpoint densities, are planned under several budgets.  Checked: bounds ascend, are
 * amino-acid aligned and tile [0, 2^64); every range's records are the sum of its slices and within the budget; every entry of every
 * input lies inside its input's slice of the one range that holds its value; a slice starts and ends where its checkpoints say; the
 * CAPACITY case names the records of the step that does not fit, and that budget then plans; a set of inputs without checkpoints is
 * one interval.  Prints "OK <plans>" or the first failure. */
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

int main() {
    std::mt19937_64 rng(20240611);
    unsigned plans = 0, capacity_seen = 0, multi = 0;
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
    CHECK(capacity_seen > 10 && multi > 10, "the trials did not reach the cases: %u CAPACITY, %u multi-range", capacity_seen, multi);
    if (fails) { printf("%d failures\n", fails); return 1; }
    printf("OK %u\n", plans);
    return 0;
}
