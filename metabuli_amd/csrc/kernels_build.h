/* kernels_build.h -- database build and merge on the device (gfx950, wave64).
 *
 * Replaces, as a function of the multiset of (value, taxid) records:
 *   - SORT_PARALLEL(..., Kmer::compareTargetKmer) in IndexCreator::createIndex (IndexCreator.cpp:343-373; Kmer.h:77-87:
 *     value, then speciesId, then taxId),
 *   - filterKmers<DB_CREATION> (IndexCreator.h:476-615): one entry per (value, speciesId), its taxid =
 *     taxonomy->LCA(taxIds of the group),
 *   - mergeTargetFiles<DB_CREATION> (IndexCreator.h:323-472; updateDB.cpp:138-142): the same over several databases' entries,
 *     with bit 31 of legacy info entries masked off (:355, 400).
 *
 * Shape: k_build_keys -> stable radix sort on the secondary key -> k_build_swap -> stable radix sort on the value (together the
 * (value, species, taxid) order) -> k_build_heads -> exclusive scan -> k_build_reduce.  Group lengths are heavy-tailed (a conserved
 * metamer shared by a thousand strains of one species is one group of a thousand), so the reduce has the join's two tiers: the head's
 * lane folds groups of up to MTB_BUILD_LANE_MAX members, longer ones are listed (one atomic per workgroup, as k_list_flag2 lists)
 * and k_build_reduce_long gives each of them a wavefront.
 *
 * The reference folds a group left to right.  Here the fold associates in any order (lanes take strided members, a shuffle tree
 * combines them): the builder admits only ids that exist in the taxonomy, all nodes hang off one root, and the LCA of nodes of one
 * tree is associative and commutative -- the result is the same node.  The per-record arithmetic is in mtb_core.h (mtb_build_*). */
#ifndef MTB_KERNELS_BUILD_H
#define MTB_KERNELS_BUILD_H
#include "dev_util.h"
#include "mtb_core.h"

#define MTB_BUILD_LANE_MAX 16u     /* members the head's lane folds on its own */

/* caller records (mtb_builder_add_records): two host arrays -> the builder's {value, taxid} list */
__global__ __launch_bounds__(256) void k_build_pack(const uint64_t *__restrict__ values, const int32_t *__restrict__ taxids, uint64_t n, mtb_kmer *__restrict__ rec) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    mtb_kmer r; r.value = values[i]; r.qinfo = (uint64_t)(uint32_t)taxids[i];
    rec[i] = r;
}
/* extracted metamers (mtb_builder_add_sequences): qinfo carries the 1-based sequence number -> that sequence's taxid */
__global__ __launch_bounds__(256) void k_build_append(const mtb_kmer *__restrict__ k, uint64_t n, const int32_t *__restrict__ seq_taxid, uint64_t n_seqs, mtb_kmer *__restrict__ rec) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const mtb_kmer q = k[i];
    const uint32_t s = mtb_q_seq(q.qinfo);
    mtb_kmer r; r.value = q.value; r.qinfo = (s >= 1 && s <= n_seqs) ? (uint64_t)(uint32_t)seq_taxid[s - 1] : 0ull;
    rec[i] = r;
}
/* a resident flat index (mtb_builder_add_index): (value, info & info_mask); *first_bad = smallest entry whose id the builder's taxonomy
 * does not know (initialised to ~0) */
__global__ __launch_bounds__(256) void k_build_from_index(const uint64_t *__restrict__ values, const uint32_t *__restrict__ info, uint64_t n, uint32_t info_mask,
                                                           mtb_tax_view tax, mtb_kmer *__restrict__ rec, unsigned long long *__restrict__ first_bad) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t t = info[i] & info_mask;
    mtb_kmer r; r.value = values[i]; r.qinfo = (uint64_t)t;
    rec[i] = r;
    if (!mtb_tax_exists(&tax, (int32_t)t)) atomicMin(first_bad, (unsigned long long)i);
}
/* the ids that occur, as a byte map of max_taxid + 1 entries (every id was checked against the taxonomy when it was added) */
__global__ __launch_bounds__(256) void k_build_mark(const mtb_kmer *__restrict__ rec, uint64_t n, uint8_t *__restrict__ seen, int32_t max_taxid) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int32_t t = (int32_t)(uint32_t)rec[i].qinfo;
    if (t >= 0 && t <= max_taxid && !seen[t]) seen[t] = 1;
}

/* one thread per record: {value, taxid} -> {secondary sort key, value} */
__global__ __launch_bounds__(256) void k_build_keys(const mtb_kmer *__restrict__ rec, uint64_t n, const int32_t *__restrict__ tax2species, int32_t max_taxid, int bits,
                                                     mtb_kmer *__restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const mtb_kmer r = rec[i];
    const int32_t t = (int32_t)(uint32_t)r.qinfo;
    mtb_kmer o;
    o.value = mtb_build_sort_key(mtb_build_key(mtb_build_species(tax2species, max_taxid, t), t), bits);
    o.qinfo = r.value;
    out[i] = o;
}
/* after the key sort: {sort key, value} -> {value, (species << 32) | taxid}, ready for the value sort (src == dst is fine) */
__global__ __launch_bounds__(256) void k_build_swap(const mtb_kmer *src, uint64_t n, int bits, mtb_kmer *dst) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const mtb_kmer r = src[i];
    mtb_kmer o; o.value = r.qinfo; o.qinfo = mtb_build_unsort_key(r.value, bits);
    dst[i] = o;
}
/* head flag of every record of the (value, species, taxid)-ordered list */
__global__ __launch_bounds__(256) void k_build_heads(const mtb_kmer *__restrict__ s, uint64_t n, uint32_t *__restrict__ head) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const mtb_kmer r = s[i];
    bool h = true;
    if (i > 0) { const mtb_kmer p = s[i - 1]; h = mtb_build_is_head(p.value, p.qinfo, r.value, r.qinfo); }
    head[i] = h ? 1u : 0u;
}

/* Tier 1: the head's lane folds its group if it has at most MTB_BUILD_LANE_MAX members and writes the entry at its scanned position;
 * longer groups are listed by their head's record number (one atomic per workgroup). */
__global__ __launch_bounds__(256) void k_build_reduce(const mtb_kmer *__restrict__ s, uint64_t n, const uint32_t *__restrict__ head, const uint32_t *__restrict__ pos,
                                                       mtb_tax_view tax, uint64_t *__restrict__ out_value, uint32_t *__restrict__ out_info,
                                                       uint32_t *__restrict__ list, uint32_t *__restrict__ n_list) {
    __shared__ uint32_t s_w[4]; __shared__ uint32_t s_base;
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    bool is_long = false;
    if (i < n && head[i]) {
        const mtb_kmer r = s[i];
        int32_t acc = mtb_build_fold(&tax, -1, mtb_build_key_taxid(r.qinfo));
        uint64_t j = i + 1;
        uint32_t members = 1;
        while (j < n && !head[j] && members < MTB_BUILD_LANE_MAX) { acc = mtb_build_fold(&tax, acc, mtb_build_key_taxid(s[j].qinfo)); j++; members++; }
        is_long = j < n && !head[j];
        if (!is_long) { const uint32_t at = pos[i]; out_value[at] = r.value; out_info[at] = (uint32_t)acc; }
    }
    const uint64_t m = __ballot(is_long);
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    if (lane == 0) s_w[wv] = (uint32_t)__popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) { const uint32_t tot = s_w[0] + s_w[1] + s_w[2] + s_w[3]; s_base = tot ? atomicAdd(n_list, tot) : 0u; }
    __syncthreads();
    if (is_long) {
        uint32_t at = s_base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        for (uint32_t q = 0; q < wv; q++) at += s_w[q];
        list[at] = (uint32_t)i;
    }
}
/* Tier 2: one wavefront per listed group.  The lanes walk the group 64 members at a time (the first head flag behind the group's own ends
 * it), each folding the members it meets; a shuffle tree of LCAs combines the 64 partial results. */
__global__ __launch_bounds__(64) void k_build_reduce_long(const mtb_kmer *__restrict__ s, uint64_t n, const uint32_t *__restrict__ head, const uint32_t *__restrict__ pos,
                                                           mtb_tax_view tax, uint64_t *__restrict__ out_value, uint32_t *__restrict__ out_info,
                                                           const uint32_t *__restrict__ list, const uint32_t *__restrict__ n_list) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t n_groups = *n_list;
    for (uint32_t g = blockIdx.x; g < n_groups; g += gridDim.x) {
        const uint64_t i = list[g];
        int32_t acc = -1;
        if (lane == 0) acc = mtb_build_fold(&tax, -1, mtb_build_key_taxid(s[i].qinfo));
        for (uint64_t base = i + 1;; base += 64) {             /* base and the exit are wave-uniform */
            const uint64_t j = base + lane;
            const bool stop = j >= n || head[j] != 0;
            const uint64_t sm = __ballot(stop);
            const uint32_t first = sm ? (uint32_t)__builtin_ctzll(sm) : 64u;
            if (lane < first) acc = mtb_build_fold(&tax, acc, mtb_build_key_taxid(s[j].qinfo));
            if (sm) break;
        }
        for (int d = 32; d > 0; d >>= 1) {
            const int32_t o = __shfl_xor(acc, d, 64);
            acc = mtb_build_fold_join(&tax, acc, o);
        }
        if (lane == 0) { const uint32_t at = pos[i]; out_value[at] = s[i].value; out_info[at] = (uint32_t)acc; }
    }
}

#endif
