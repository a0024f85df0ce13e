/* kernels_clade_filter.h -- stable compaction of keyed records by keep[species key] (gfx950, wave64): the filter of
 * mtb_merge_databases_filtered, placed right behind k_merge_keys, and of the stage call mtb_filter_records.
 *
 *   k_clade_count    per tile of MTB_CLADE_TILE records: how many are kept -> tile_count[tile]; marks every species key it meets in
 *                    met[] (a plain byte store of 1, no atomics, as k_mark_taxids does; skipped where the byte already reads 1)
 *   scan_launch      tile_count[] -> tile_base[] (exclusive), tile_base[n_tiles] = records kept
 *   k_clade_compact  the same flags again; record i of the tile is stored at out[tile_base[tile] + rank of i among the tile's kept]
 *
 * A lane takes MTB_CLADE_PER_LANE = 8 consecutive records with one 16-byte load each (a record is 16 B and 16-byte aligned), so a
 * lane's kept records are consecutive in the output as well.  keep[] is a byte table of the taxonomy's size (a few MB at most) that
 * is read through the cache and stays in L2.  Ranks inside a wave come from one ballot per record slot: the kept records of lower
 * lanes are the popcounts of the ballots below this lane's bit; the four wave totals of a tile go through LDS.  Order is preserved:
 * the merge's tie rule and "a slice ascends under this taxonomy" depend on it.
 * No workgroup ever waits for another (no decoupled look-back, no flag to spin on): two launches and the scan between them read each
 * record twice instead.  Traffic per record: 16 B read (count) + 16 B read + at most 16 B written (compact) = 48 B at most, plus
 * 12 B per tile for its count and base: both kernels are bound by HBM bandwidth, with the occupancy of a copy (no LDS beyond 16 B,
 * 32 VGPRs of records).
 * Tile = MTB_MERGE_TILE, so the edge cases (n % 2048 in {0, 1, 2047}) are those of the merge kernel. */
#ifndef MTB_KERNELS_CLADE_FILTER_H
#define MTB_KERNELS_CLADE_FILTER_H
#include "dev_util.h"
#include "mtb_core.h"
#include "kernels_merge.h"

#define MTB_CLADE_TILE 2048u
#define MTB_CLADE_THREADS 256u
#define MTB_CLADE_PER_LANE (MTB_CLADE_TILE / MTB_CLADE_THREADS)
static_assert(MTB_CLADE_TILE == MTB_MERGE_TILE, "the filter's tile is the merge's tile");
static_assert(MTB_CLADE_PER_LANE == 8 && sizeof(mtb_kmer) == 16, "8 records of 16 bytes per lane");

/* the species key of a record as loaded: {value lo, value hi, taxid, species} */
__device__ __forceinline__ uint32_t clade_species(const uint4 &r) { return r.w; }

/* sum of v over the workgroup's four waves, in every thread; *before = the sum over the waves below this one */
__device__ __forceinline__ uint32_t clade_block_sum(uint32_t wave_total, uint32_t *s_w, uint32_t *before) {
    const uint32_t w = threadIdx.x >> 6;
    if (lane_id() == 0) s_w[w] = wave_total;
    __syncthreads();
    const uint32_t t0 = s_w[0], t1 = s_w[1], t2 = s_w[2], t3 = s_w[3];
    *before = (w > 0 ? t0 : 0u) + (w > 1 ? t1 : 0u) + (w > 2 ? t2 : 0u);
    return t0 + t1 + t2 + t3;
}

/* tile_count[t] = records of tile t whose key indexes keep[] with a non-zero byte; met[key] = 1 for every key seen (met may be
 * NULL); *first_bad = smallest record whose key is >= n_keep (initialised to ~0; such a record counts as not kept) */
__global__ __launch_bounds__(256) void k_clade_count(const mtb_kmer *__restrict__ rec, uint64_t n, const uint8_t *__restrict__ keep, uint64_t n_keep, uint8_t *met,
                                                      uint32_t *__restrict__ tile_count, unsigned long long *__restrict__ first_bad) {
    __shared__ uint32_t s_w[4];
    const uint64_t i0 = (uint64_t)blockIdx.x * MTB_CLADE_TILE + (uint64_t)threadIdx.x * MTB_CLADE_PER_LANE;
    const uint4 *p = (const uint4 *)rec;
    uint32_t m = 0;
#pragma unroll
    for (uint32_t q = 0; q < MTB_CLADE_PER_LANE; q++) {
        const uint64_t i = i0 + q;
        if (i >= n) continue;
        const uint32_t s = clade_species(p[i]);
        if ((uint64_t)s >= n_keep) { atomicMin(first_bad, (unsigned long long)i); continue; }
        if (keep[s]) m |= 1u << q;
        if (met && !met[s]) met[s] = 1;
    }
    uint32_t wave_total = 0;
#pragma unroll
    for (uint32_t q = 0; q < MTB_CLADE_PER_LANE; q++) wave_total += (uint32_t)__popcll(__ballot((m >> q) & 1u));
    uint32_t before;
    const uint32_t total = clade_block_sum(wave_total, s_w, &before);
    if (threadIdx.x == 0) tile_count[blockIdx.x] = total;
}

/* out[tile_base[t] + r] = the r-th kept record of tile t */
__global__ __launch_bounds__(256) void k_clade_compact(const mtb_kmer *__restrict__ rec, uint64_t n, const uint8_t *__restrict__ keep, uint64_t n_keep,
                                                        const uint64_t *__restrict__ tile_base, mtb_kmer *__restrict__ out) {
    __shared__ uint32_t s_w[4];
    const uint64_t i0 = (uint64_t)blockIdx.x * MTB_CLADE_TILE + (uint64_t)threadIdx.x * MTB_CLADE_PER_LANE;
    const uint4 *p = (const uint4 *)rec;
    uint4 r[MTB_CLADE_PER_LANE];
    uint32_t m = 0;
#pragma unroll
    for (uint32_t q = 0; q < MTB_CLADE_PER_LANE; q++) {
        const uint64_t i = i0 + q;
        r[q] = make_uint4(0, 0, 0, 0);
        if (i >= n) continue;
        r[q] = p[i];
        const uint32_t s = clade_species(r[q]);
        if ((uint64_t)s < n_keep && keep[s]) m |= 1u << q;
    }
    const uint64_t lower = lanemask_lt();
    uint32_t wave_total = 0, below = 0;            /* kept records of the wave / of its lanes below this one */
#pragma unroll
    for (uint32_t q = 0; q < MTB_CLADE_PER_LANE; q++) {
        const uint64_t b = __ballot((m >> q) & 1u);
        wave_total += (uint32_t)__popcll(b); below += (uint32_t)__popcll(b & lower);
    }
    uint32_t before;
    clade_block_sum(wave_total, s_w, &before);
    uint4 *o = (uint4 *)out + tile_base[blockIdx.x] + before + below;
#pragma unroll
    for (uint32_t q = 0; q < MTB_CLADE_PER_LANE; q++)
        if ((m >> q) & 1u) *o++ = r[q];
}

#endif
