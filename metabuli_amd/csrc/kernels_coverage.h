/* kernels_coverage.h -- which database entries the classified reads touched (mtb_index_coverage_*; gfx950, wave64).
 *
 * The rule is tests/coverage_spec.py.  State on the index: a bitmap of one bit per entry position (u32 words) and u64 `hits` bins per
 * species; a context adds its hits into pending bins of its own, which a commit kernel moves into the index's at the successful end
 * of a classify call.  The array is read in whatever state it is in: flat ({value, info}, with or without a directory) or packed
 * (kernels_dir.h: info << 29 | eighth letter << 24 | DNA, depth-7 directory).
 *   k_cov_read_species   rs[r] = species of read r's classification (0: unclassified, or classified above species rank).  The
 *                        marking reads these 4 bytes per query metamer instead of the 24-byte result row.
 *   k_cov_mark           one query metamer per lane: its equal-value run in the array (directory bucket + lower-bound bisection, or
 *                        bisection over the whole array), walked linearly; every entry of the read's species gets its bit set.
 *                        Bits: the word is read with a plain load first and the atomic is skipped where the bit already shows -- a
 *                        stale read costs one redundant atomic, never a mark; otherwise a no-return device-scope atomicOr.  Hits:
 *                        a batch is a few species deep, so the lanes of a wave that hold the same species add once
 *                        (MTB_COV_FOLD_ROUNDS leaders, then one add per lane left); adds to one address serialise
 *                        (kernels_audit.h).  The queries are sorted on their first six letters only: nothing here relies on
 *                        equal values being neighbours.
 *   k_cov_count          one streaming pass over the array, four entries per lane: the species of every entry into the `total`
 *                        bins, of every marked entry into the `distinct` bins (mtb_audit_hist_add and its per-XCD replicas).
 *   k_cov_accumulate     u64 bins += the u32 bins of one pass (a pass covers fewer than 2^32 entries), which are cleared.
 *   k_cov_or             dst |= src, word by word (mtb_index_coverage_merge, through a bounded staging buffer).
 *   k_cov_commit         index bins += a context's pending bins, which are cleared; the call counter.
 * Bytes: k_cov_mark reads 16 B per query record + 4 B of rs, and per counted query two directory words, ~3 bisection probes of 8 B
 * inside one or two cache lines (no directory: log2 T probes) and the run (8 B per entry, + 4 B of info in the flat state); it
 * writes at most one 4-byte atomic per entry of the read's species.  k_cov_count reads 8 B (packed) or 12 B (flat) + 1 bit per entry. */
#ifndef MTB_KERNELS_COVERAGE_H
#define MTB_KERNELS_COVERAGE_H
#include "../../include/mtb.h"
#include "dev_util.h"
#include "kernels_audit.h"
#include "kernels_dir.h"
#include "mtb_core.h"

#define MTB_COV_FOLD_ROUNDS 4
/* words behind the species bins of `hits` / pending arrays: query records seen (blanks excluded), of those with a species, committed calls */
enum { MTB_COV_N_QUERIES = 0, MTB_COV_N_COUNTED = 1, MTB_COV_N_BATCHES = 2, MTB_COV_EXTRA = 4 };

/* mtb_tax_species, and 0 for what cannot index a bin */
__device__ __forceinline__ int32_t mtb_cov_species(const int32_t *__restrict__ tax2species, int32_t max_taxid, int32_t id) {
    const int32_t s = mtb_build_species(tax2species, max_taxid, id);
    return (s > 0 && s <= max_taxid) ? s : 0;
}

__global__ __launch_bounds__(256) void k_cov_read_species(const mtb_result *__restrict__ res, uint64_t n, const int32_t *__restrict__ tax2species, int32_t max_taxid,
                                                           uint32_t *__restrict__ rs) {
    const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    rs[r] = res[r].is_classified ? (uint32_t)mtb_cov_species(tax2species, max_taxid, res[r].classification) : 0u;
}

/* the part of a value that tells entries of one depth-7 bucket apart (mtb_pack_word's low bits) */
__device__ __forceinline__ uint64_t mtb_cov_low(uint64_t value, int fmt) { return mtb_pack_word(value, 0u, fmt); }

/* q[0, n): query records in any order; rs[0, n_reads): k_cov_read_species' output (seq is 1-based; a seq beyond n_reads is skipped --
 * the callers refuse such input before the launch).  ix: the array as it is (ix.info unused when PACKED); dv: its directory (DIR).
 * pend: species bins [0, max_taxid] + MTB_COV_EXTRA words. */
template <bool PACKED, bool DIR>
__global__ __launch_bounds__(256) void k_cov_mark(const mtb_kmer *__restrict__ q, uint64_t n, const uint32_t *__restrict__ rs, uint64_t n_reads, mtb_index_view ix, mtb_dir_view dv,
                                                   uint32_t *bitmap, unsigned long long *__restrict__ pend) {
    static_assert(DIR || !PACKED, "the packed state has a depth-7 directory");
    const uint64_t T = ix.n_targets;
    const uint64_t LOW = (1ull << MTB_PACK_LOW) - 1;
    uint32_t seen = 0, counted = 0;
    for (uint64_t base = (uint64_t)blockIdx.x * 256; base < n; base += (uint64_t)gridDim.x * 256) {      /* (every lane of a wave runs the same number of rounds) */
        const uint64_t j = base + threadIdx.x;
        int32_t s = 0; uint64_t value = 0; bool live = false;
        if (j < n) {
            const mtb_kmer k = q[j];
            const uint32_t seq = mtb_q_seq(k.qinfo);
            if (seq != 0 && (uint64_t)seq <= n_reads) { live = true; s = (int32_t)rs[seq - 1]; value = k.value; }
        }
        bool hit = false;
        if (s != 0) {
            uint64_t lo = 0, hi = T;
            if (DIR) {
                const uint32_t b = mtb_dir_bucket(value, dv.L, dv.kmer_format);
                if (mtb_dir_letters_ok(value, dv.kmer_format) && b < dv.n_buckets) {
                    lo = dv.base[b >> 16] + dv.dir[b]; hi = dv.base[(b + 1) >> 16] + dv.dir[b + 1];
                    if (hi > T) hi = T;
                    if (lo > hi) lo = hi;
                } else hi = 0;                       /* a letter no entry of a directory index has: not in the database */
            }
            const uint64_t key = PACKED ? mtb_cov_low(value, dv.kmer_format) : value;
            uint64_t a = lo, z = hi;
            while (a < z) { const uint64_t mid = a + ((z - a) >> 1); const uint64_t w = ix.values[mid]; if ((PACKED ? (w & LOW) : w) < key) a = mid + 1; else z = mid; }
            for (uint64_t t = a; t < hi; t++) {
                const uint64_t w = ix.values[t];
                if ((PACKED ? (w & LOW) : w) != key) break;
                const int32_t id = (int32_t)((PACKED ? (uint32_t)(w >> MTB_PACK_LOW) : ix.info[t]) & ix.info_mask);
                if (mtb_cov_species(ix.tax2species, ix.max_taxid, id) != s) continue;
                hit = true;
                uint32_t *const word = bitmap + (t >> 5); const uint32_t bit = 1u << (t & 31u);
                if ((*word & bit) == 0) atomicOr(word, bit);
            }
        }
        seen += (uint32_t)__popcll(__ballot(live)); counted += (uint32_t)__popcll(__ballot(s != 0));
        /* hits[s] += 1 per query with a hit: the lanes that share the leader's species add once */
        bool pending = hit;
        for (int r = 0; r < MTB_COV_FOLD_ROUNDS; r++) {
            const uint64_t left = __ballot(pending);
            if (left == 0) break;
            const int leader = __ffsll((long long)left) - 1;
            const int32_t s0 = rl_i(s, leader);
            const bool mine = pending && s == s0;
            const uint32_t cnt = (uint32_t)__popcll(__ballot(mine));
            if ((int)lane_id() == leader) atomicAdd(pend + s0, (unsigned long long)cnt);
            if (mine) pending = false;
        }
        if (pending) atomicAdd(pend + s, 1ull);
    }
    if (lane_id() == 0) {
        unsigned long long *const extra = pend + (uint64_t)ix.max_taxid + 1;
        if (seen) atomicAdd(extra + MTB_COV_N_QUERIES, (unsigned long long)seen);
        if (counted) atomicAdd(extra + MTB_COV_N_COUNTED, (unsigned long long)counted);
    }
}

/* entries [t0, t0 + m) of the array, t0 a multiple of 32: total / distinct are u32 bin arrays with MTB_AUDIT_REPLICAS replicas
 * replica_stride apart (kernels_audit.h), either may be NULL */
template <bool PACKED>
__global__ __launch_bounds__(256) void k_cov_count(mtb_index_view ix, uint64_t t0, uint64_t m, const uint32_t *__restrict__ bitmap,
                                                    uint32_t *__restrict__ total, uint32_t *__restrict__ distinct, uint64_t replica_stride) {
    const uint64_t rep = (blockIdx.x & (MTB_AUDIT_REPLICAS - 1u)) * replica_stride;
    const uint64_t per_block = 256ull * MTB_AUDIT_PER_LANE;
    const uint64_t n_blocks = (m + per_block - 1) / per_block;
    for (uint64_t b = blockIdx.x; b < n_blocks; b += gridDim.x) {          /* (every lane of a wave runs the same number of rounds) */
        const uint64_t j0 = t0 + b * per_block + (uint64_t)threadIdx.x * MTB_AUDIT_PER_LANE;       /* a multiple of 4: one bitmap word */
        int32_t sp[MTB_AUDIT_PER_LANE]; bool all[MTB_AUDIT_PER_LANE], set[MTB_AUDIT_PER_LANE];
        const uint32_t bits = j0 < t0 + m ? bitmap[j0 >> 5] >> (j0 & 31u) : 0u;
#pragma unroll
        for (uint32_t k = 0; k < MTB_AUDIT_PER_LANE; k++) {
            const uint64_t t = j0 + k;
            sp[k] = 0; all[k] = false; set[k] = false;
            if (t >= t0 + m) continue;
            const int32_t id = (int32_t)((PACKED ? (uint32_t)(ix.values[t] >> MTB_PACK_LOW) : ix.info[t]) & ix.info_mask);
            sp[k] = mtb_cov_species(ix.tax2species, ix.max_taxid, id);
            all[k] = sp[k] != 0; set[k] = all[k] && ((bits >> k) & 1u);
        }
        if (total) mtb_audit_hist_add(total + rep, sp, all, MTB_AUDIT_FOLD_ROUNDS);
        if (distinct) mtb_audit_hist_add(distinct + rep, sp, set, MTB_AUDIT_FOLD_ROUNDS);
    }
}

__global__ __launch_bounds__(256) void k_cov_accumulate(unsigned long long *__restrict__ sum, uint32_t *__restrict__ bins, uint64_t n_bins) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_bins) return;
    sum[i] += bins[i]; bins[i] = 0;
}

__global__ __launch_bounds__(256) void k_cov_or(uint32_t *__restrict__ dst, const uint32_t *__restrict__ src, uint64_t n_words) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n_words; i += (uint64_t)gridDim.x * 256) { const uint32_t w = src[i]; if (w) dst[i] |= w; }
}

/* hits[i] += pend[i], pend[i] = 0 for i in [0, n_words); hits[batch_word] += calls.  Several contexts may commit into one index at
 * the same time: atomics. */
__global__ __launch_bounds__(256) void k_cov_commit(unsigned long long *__restrict__ hits, unsigned long long *__restrict__ pend, uint64_t n_words, uint64_t batch_word, uint32_t calls) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_words) return;
    unsigned long long v = pend[i];
    if (i == batch_word) v += calls;
    if (v) atomicAdd(hits + i, v);
    pend[i] = 0;
}

#endif
