/* kernels_merge.h -- streamed merge of databases: sorted record lists are merged, not re-sorted (gfx950, wave64).
 *
 * Replaces mergeTargetFiles<DB_CREATION> (IndexCreator.h:323-472) for inputs that are databases: every input's entries are already in
 * (value, species) order with one entry per (value, species), so per value range the device
 *   k_merge_trim      bisects a decoded slice of an input (decoded from a checkpoint at or below the range to one at or above it)
 *                     to the range's bounds,
 *   k_merge_keys      turns {value, info & info_mask} into {value, (species << 32) | taxid} -- the layout k_build_swap leaves, so
 *                     k_build_heads / k_build_reduce / k_build_reduce_long run unchanged behind the merge --, finds ids the taxonomy
 *                     does not know and checks that the slice ascends under THIS taxonomy's species table,
 *   k_merge_partition finds, per output tile of MTB_MERGE_TILE records, how many of its predecessors come from the first list
 *   k_merge_tile      (merge path: a bisection along the tile's diagonal), then stages the tile's two input segments in LDS, lets
 *                     every lane bisect its own diagonal there, merge MTB_MERGE_PER_LANE records serially and stores the tile
 *                     coalesced.
 * Order: (value, species, taxid), i.e. value then the whole 64-bit key.  That refines the (value, species) order the reduce needs: an
 * input holds one entry per (value, species), so it ascends strictly in both orders, the merge of two lists that ascend in the full
 * order ascends in it, and the result is the list the builder's two sorts produce.  Ties take from the first list.
 * A slice that does not ascend (its database was built under another taxonomy) is sorted by the builder's radix path first
 * (k_merge_sort_key -> sort -> k_build_swap -> sort); nothing else is ever sorted.
 *
 * Tile: 2048 records = 32 KB of LDS (values and keys as two arrays of 8-byte words, which a lane reads 8 bytes at a time), 256
 * threads: five workgroups = 20 waves per CU fit the 160 KB; the kernel streams 16 B in and 16 B out per record and has the
 * occupancy of a copy.  The serial merges of a wave read LDS at lane-dependent addresses (bank conflicts are data dependent). */
#ifndef MTB_KERNELS_MERGE_H
#define MTB_KERNELS_MERGE_H
#include "dev_util.h"
#include "mtb_core.h"

#define MTB_MERGE_TILE 2048u
#define MTB_MERGE_THREADS 256u
#define MTB_MERGE_PER_LANE (MTB_MERGE_TILE / MTB_MERGE_THREADS)

/* a before b in (value, species, taxid) order */
MTB_HD bool mtb_merge_less(uint64_t av, uint64_t ak, uint64_t bv, uint64_t bk) { return av < bv || (av == bv && ak < bk); }

/* out[0] / out[1] = first entry of values[0, n) that is >= lo / >= hi (hi = UINT64_MAX: the range is open, out[1] = n) */
__global__ void k_merge_trim(const uint64_t *__restrict__ values, uint64_t n, uint64_t lo, uint64_t hi, uint64_t *__restrict__ out) {
    const uint32_t t = threadIdx.x;
    if (blockIdx.x != 0 || t > 1) return;
    const uint64_t bound = t ? hi : lo;
    uint64_t a = 0, b = n;
    if (t && hi == UINT64_MAX) a = n;
    while (a < b) { const uint64_t mid = a + ((b - a) >> 1); if (values[mid] < bound) a = mid + 1; else b = mid; }
    out[t] = a;
}

/* entries [0, n) of a trimmed slice -> records; *first_bad = smallest entry whose id the taxonomy does not know (initialised to ~0),
 * *unsorted != 0 if a record sorts before its predecessor */
__global__ __launch_bounds__(256) void k_merge_keys(const uint64_t *__restrict__ values, const uint32_t *__restrict__ info, uint64_t n, uint32_t info_mask,
                                                     mtb_tax_view tax, const int32_t *__restrict__ tax2species, mtb_kmer *__restrict__ rec,
                                                     unsigned long long *__restrict__ first_bad, uint32_t *__restrict__ unsorted) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int32_t t = (int32_t)(info[i] & info_mask);
    mtb_kmer r; r.value = values[i]; r.qinfo = mtb_build_key(mtb_build_species(tax2species, tax.max_taxid, t), t);
    rec[i] = r;
    if (!mtb_tax_exists(&tax, t)) atomicMin(first_bad, (unsigned long long)i);
    if (i > 0) {
        const int32_t pt = (int32_t)(info[i - 1] & info_mask);
        if (mtb_merge_less(r.value, r.qinfo, values[i - 1], mtb_build_key(mtb_build_species(tax2species, tax.max_taxid, pt), pt)) && !*unsorted) *unsorted = 1u;
    }
}
/* {value, key} -> {the builder's secondary sort key, value}, in place: the input of the builder's first sort */
__global__ __launch_bounds__(256) void k_merge_sort_key(mtb_kmer *rec, uint64_t n, int bits) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const mtb_kmer r = rec[i];
    mtb_kmer o; o.value = mtb_build_sort_key(r.qinfo, bits); o.qinfo = r.value;
    rec[i] = o;
}

/* merge path: split[t] = how many of the first min(t * MTB_MERGE_TILE, na + nb) output records come from a (ties take from a) */
__global__ __launch_bounds__(256) void k_merge_partition(const mtb_kmer *__restrict__ a, uint64_t na, const mtb_kmer *__restrict__ b, uint64_t nb, uint64_t n_tiles,
                                                          uint64_t *__restrict__ split) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t > n_tiles) return;
    const uint64_t total = na + nb;
    uint64_t d = t * MTB_MERGE_TILE; if (d > total) d = total;
    uint64_t lo = d > nb ? d - nb : 0, hi = d < na ? d : na;
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        const mtb_kmer x = a[mid], y = b[d - 1 - mid];
        if (!mtb_merge_less(y.value, y.qinfo, x.value, x.qinfo)) lo = mid + 1; else hi = mid;       /* a[mid] <= b[d - 1 - mid]: a[mid] is among the first d */
    }
    split[t] = lo;
}

__global__ __launch_bounds__(256) void k_merge_tile(const mtb_kmer *__restrict__ a, const mtb_kmer *__restrict__ b, uint64_t total, const uint64_t *__restrict__ split,
                                                     mtb_kmer *__restrict__ out) {
    __shared__ uint64_t s_v[MTB_MERGE_TILE];
    __shared__ uint64_t s_k[MTB_MERGE_TILE];
    const uint64_t t = blockIdx.x;
    const uint64_t o0 = t * MTB_MERGE_TILE, o1 = (o0 + MTB_MERGE_TILE < total) ? o0 + MTB_MERGE_TILE : total;
    const uint64_t a0 = split[t], a1 = split[t + 1], b0 = o0 - a0;
    const uint32_t la = (uint32_t)(a1 - a0), cnt = (uint32_t)(o1 - o0), lb = cnt - la;
    for (uint32_t x = threadIdx.x; x < cnt; x += MTB_MERGE_THREADS) {
        const mtb_kmer r = x < la ? a[a0 + x] : b[b0 + (x - la)];
        s_v[x] = r.value; s_k[x] = r.qinfo;
    }
    __syncthreads();
    /* this lane's diagonal inside the tile: i records of the a segment [0, la), d - i of the b segment [la, la + lb) come before it */
    uint32_t d = threadIdx.x * MTB_MERGE_PER_LANE; if (d > cnt) d = cnt;
    uint32_t lo = d > lb ? d - lb : 0, hi = d < la ? d : la;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1, y = la + d - 1 - mid;
        if (!mtb_merge_less(s_v[y], s_k[y], s_v[mid], s_k[mid])) lo = mid + 1; else hi = mid;
    }
    uint32_t i = lo, j = la + (d - lo);
    uint64_t ov[MTB_MERGE_PER_LANE], ok[MTB_MERGE_PER_LANE];
#pragma unroll
    for (uint32_t q = 0; q < MTB_MERGE_PER_LANE; q++) {
        const bool has_a = i < la, has_b = j < cnt;
        uint64_t av = 0, ak = 0, bv = 0, bk = 0;
        if (has_a) { av = s_v[i]; ak = s_k[i]; }
        if (has_b) { bv = s_v[j]; bk = s_k[j]; }
        const bool take_a = has_a && (!has_b || !mtb_merge_less(bv, bk, av, ak));
        ov[q] = take_a ? av : bv; ok[q] = take_a ? ak : bk;
        if (take_a) i++; else if (has_b) j++;
    }
    __syncthreads();
#pragma unroll
    for (uint32_t q = 0; q < MTB_MERGE_PER_LANE; q++) {
        const uint32_t x = d + q;
        if (threadIdx.x * MTB_MERGE_PER_LANE + q < cnt) { s_v[x] = ov[q]; s_k[x] = ok[q]; }
    }
    __syncthreads();
    for (uint32_t x = threadIdx.x; x < cnt; x += MTB_MERGE_THREADS) {
        mtb_kmer r; r.value = s_v[x]; r.qinfo = s_k[x];
        out[o0 + x] = r;
    }
}

/* split checkpoints of a database written range by range (mtb_index_write's rule, IndexCreator.cpp:848-857): armed[t] is an entry at
 * which a checkpoint is armed; j_out[t] = the first later entry of another amino-acid part inside the window [.., win_end) of the
 * output the caller holds decoded (values is indexed by the entry's number in the whole output), n if the window ends the output,
 * UINT64_MAX if the window ends first: the arming is then still pending at the first entry of the next window */
__global__ __launch_bounds__(256) void k_split_find_win(const uint64_t *values, uint64_t win_end, uint64_t n, const uint64_t *__restrict__ armed, uint32_t n_armed,
                                                         uint64_t *__restrict__ j_out) {
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t >= n_armed) return;
    const uint64_t i0 = armed[t];
    const uint64_t aa = values[i0] & ~0xFFFFFFull;
    uint64_t j = i0 + 1;
    while (j < win_end && (values[j] & ~0xFFFFFFull) == aa) j++;
    j_out[t] = j < win_end ? j : (win_end == n ? n : UINT64_MAX);
}

#endif
