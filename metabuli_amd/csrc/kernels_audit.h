/* kernels_audit.h -- the checks of mtb_database_audit over one decoded chunk of a database (gfx950, wave64).
 *
 * The chunk is what decode_chunked leaves per step: value[0, n_values), the info entries of the first m of them, the chunk's
 * 16-bit words and the end-word prefix of its 2048-word tiles.  Nothing here depends on the size of the database.
 *   k_audit_order         every entry against its predecessor -- value[i] < value[i-1] (a descent; in a file: a delta that wrapped),
 *                         equal values with species[i] <= species[i-1] (group disorder) -- and against the taxonomy: ids it does
 *                         not know, known ids absent from taxID_list, known ids without a species.  The predecessor of the
 *                         chunk's first entry is the previous chunk's last one, kept in a device word pair (prev_in / prev_out: two
 *                         pairs used in turn, so that no workgroup reads what another one writes).  The per-species entry
 *                         counts are taken in the same pass, so that info is read once (mtb_audit_hist_add; `bins` may be NULL).
 *   k_audit_checkpoints   merge_plan.h's rule for the `split` records whose word offset falls into the chunk.
 * Counters: one wave-reduced no-return atomic per counter and wave (ballot + popcount), and only from waves that found something;
 * first positions by a 64-bit atomicMin from the wave's first flagged lane.  A sound database issues no counter atomic at all.
 * Bins: the entries are in value order, so neighbouring species are unrelated and millions of bins cannot be privatised in LDS: u32
 * no-return device-scope adds straight into global memory.  Adds to ONE address serialise at about 88 M/s (profiles/audit_notes.md:
 * 1.2 * 10^8 adds to the bin of a species that owns 60 % of a database took 1.36 s), adds spread over 0.5 MB of bins run at
 * 38 G/s.  So a hot species is folded in the wave before it reaches memory (mtb_audit_hist_add: one add per 256 entries), and
 * every XCD has a bin array of its own (MTB_AUDIT_REPLICAS, summed by k_audit_bins_reduce at the end), which divides what is left
 * on one address by eight and costs nothing where the species are even.
 * Loads: a lane takes four consecutive entries: two 16-byte loads of values, one of info (the chunk buffers are 256-byte aligned). */
#ifndef MTB_KERNELS_AUDIT_H
#define MTB_KERNELS_AUDIT_H
#include "dev_util.h"
#include "mtb_core.h"

#define MTB_AUDIT_PER_LANE 4u
#define MTB_AUDIT_FOLD_ROUNDS 2
#define MTB_AUDIT_REPLICAS 8u

/* the counters of k_audit_order, in the order of the report; MTB_AUDIT_FIRST + k is the first position of counter k */
enum { MTB_AUDIT_DESCENT = 0, MTB_AUDIT_DISORDER = 1, MTB_AUDIT_UNKNOWN = 2, MTB_AUDIT_UNLISTED = 3, MTB_AUDIT_NO_SPECIES = 4, MTB_AUDIT_COUNTERS = 5,
       MTB_AUDIT_FIRST = 5, MTB_AUDIT_BAD_CP = 10, MTB_AUDIT_FIRST_BAD_CP = 11, MTB_AUDIT_WORDS = 12 };

/* one record of `split` that a chunk has to judge: word and entry offsets are relative to the chunk */
typedef struct { uint64_t ad, diff_off, info_off, record; } mtb_audit_checkpoint;

/* what the taxonomy says of one info entry */
typedef struct { int32_t species; uint32_t flags; } mtb_audit_id;
__device__ __forceinline__ mtb_audit_id mtb_audit_lookup(uint32_t info, uint32_t info_mask, const mtb_tax_view &tax, const int32_t *__restrict__ tax2species,
                                                          const uint8_t *__restrict__ listed) {
    const int32_t t = (int32_t)(info & info_mask);
    mtb_audit_id r; r.species = 0; r.flags = 0;
    if (!mtb_tax_exists(&tax, t)) { r.flags = 1u << MTB_AUDIT_UNKNOWN; return r; }
    r.species = mtb_build_species(tax2species, tax.max_taxid, t);
    if (!listed[t]) r.flags |= 1u << MTB_AUDIT_UNLISTED;
    if (r.species <= 0 || r.species > tax.max_taxid) { r.species = 0; r.flags |= 1u << MTB_AUDIT_NO_SPECIES; }
    return r;
}

/* bins[sp[q]]++ for the lane's entries with on[q]; wave-uniform control flow.  A species that owns much of a database must not
 * take one add per entry (adds to one address serialise: see the head of this file): a lane that holds a species twice among its
 * four entries offers it, the wave takes the first offer, counts that species over all 256 entries (four ballots) and adds once;
 * `rounds` offers are taken, then every entry still pending adds one.  Without a repeat in any lane (a database of many even
 * species) this costs one ballot. */
__device__ __forceinline__ void mtb_audit_hist_add(uint32_t *__restrict__ bins, const int32_t sp[MTB_AUDIT_PER_LANE], bool on[MTB_AUDIT_PER_LANE], int rounds) {
    int32_t offer = 0;
#pragma unroll
    for (uint32_t a = 0; a + 1 < MTB_AUDIT_PER_LANE; a++)
#pragma unroll
        for (uint32_t b = a + 1; b < MTB_AUDIT_PER_LANE; b++) if (on[a] && on[b] && sp[a] == sp[b]) offer = sp[a];
    for (int r = 0; r < rounds; r++) {
        const uint64_t offers = __ballot(offer != 0);
        if (offers == 0) break;
        const int leader = __ffsll((long long)offers) - 1;
        const int32_t s0 = rl_i(offer, leader);
        uint32_t n = 0;
#pragma unroll
        for (uint32_t q = 0; q < MTB_AUDIT_PER_LANE; q++) {
            const bool hit = on[q] && sp[q] == s0;
            n += (uint32_t)__popcll(__ballot(hit));
            if (hit) on[q] = false;
        }
        if ((int)lane_id() == leader) atomicAdd(bins + s0, n);
        if (offer == s0) offer = 0;
    }
#pragma unroll
    for (uint32_t q = 0; q < MTB_AUDIT_PER_LANE; q++) if (on[q]) atomicAdd(bins + sp[q], 1u);
}

/* counter k += flagged entries of the wave, first[k] = min(first[k], the wave's first flagged entry); entries of a lane are
 * consecutive, so the first flagged lane holds the first flagged entry */
__device__ __forceinline__ void mtb_audit_count(unsigned long long *__restrict__ out, int k, const uint32_t fl[MTB_AUDIT_PER_LANE], uint64_t first_entry_of_lane) {
    const uint32_t bit = 1u << k;
    const uint32_t mine = (fl[0] | fl[1] | fl[2] | fl[3]) & bit;
    const uint64_t any = __ballot(mine != 0);
    if (any == 0) return;
    uint32_t n = 0;
#pragma unroll
    for (uint32_t q = 0; q < MTB_AUDIT_PER_LANE; q++) n += (uint32_t)__popcll(__ballot((fl[q] & bit) != 0));
    if ((int)lane_id() == __ffsll((long long)any) - 1) {
        uint32_t q = 0;
        while (!(fl[q] & bit)) q++;
        atomicAdd(out + k, (unsigned long long)n);
        atomicMin(out + MTB_AUDIT_FIRST + k, (unsigned long long)(first_entry_of_lane + q));
    }
}

/* entries [0, m) of a chunk; entry j of the chunk is entry g + j of the database.  prev_in = {value, species} of entry g - 1
 * (not read when g == 0); prev_out receives those of entry g + m - 1.  out: MTB_AUDIT_WORDS words (counters zero, firsts ~0 at the
 * start of the audit).  bins may be NULL (no counts); fold_rounds: MTB_AUDIT_FOLD_ROUNDS, or 0 for one add per entry (measurements);
 * replica_stride: the distance between MTB_AUDIT_REPLICAS bin arrays, of which a workgroup takes number blockIdx.x mod 8 -- the
 * one of its XCD -- and which k_audit_bins_reduce sums at the end; 0 for one bin array (measurements). */
__global__ __launch_bounds__(256) void k_audit_order(const uint64_t *__restrict__ values, const uint32_t *__restrict__ info, uint64_t m, uint64_t g, uint32_t info_mask,
                                                      mtb_tax_view tax, const int32_t *__restrict__ tax2species, const uint8_t *__restrict__ listed,
                                                      const uint64_t *__restrict__ prev_in, uint64_t *__restrict__ prev_out,
                                                      unsigned long long *__restrict__ out, uint32_t *__restrict__ bins, int fold_rounds, uint64_t replica_stride) {
    if (bins) bins += (blockIdx.x & (MTB_AUDIT_REPLICAS - 1u)) * replica_stride;          /* (workgroups go round the XCDs in launch order) */
    const uint64_t per_block = 256ull * MTB_AUDIT_PER_LANE;
    const uint64_t n_blocks = (m + per_block - 1) / per_block;
    for (uint64_t b = blockIdx.x; b < n_blocks; b += gridDim.x) {          /* (every lane of a wave runs the same number of rounds) */
        const uint64_t j0 = b * per_block + (uint64_t)threadIdx.x * MTB_AUDIT_PER_LANE;
        uint64_t v[MTB_AUDIT_PER_LANE]; uint32_t in[MTB_AUDIT_PER_LANE];
        if (j0 + MTB_AUDIT_PER_LANE <= m) {
            const uint4 a = *(const uint4 *)(values + j0), c = *(const uint4 *)(values + j0 + 2), i4 = *(const uint4 *)(info + j0);
            v[0] = a.x | ((uint64_t)a.y << 32); v[1] = a.z | ((uint64_t)a.w << 32); v[2] = c.x | ((uint64_t)c.y << 32); v[3] = c.z | ((uint64_t)c.w << 32);
            in[0] = i4.x; in[1] = i4.y; in[2] = i4.z; in[3] = i4.w;
        } else {
#pragma unroll
            for (uint32_t q = 0; q < MTB_AUDIT_PER_LANE; q++) { const bool has = j0 + q < m; v[q] = has ? values[j0 + q] : 0; in[q] = has ? info[j0 + q] : 0; }
        }
        uint32_t fl[MTB_AUDIT_PER_LANE]; int32_t sp[MTB_AUDIT_PER_LANE];
#pragma unroll
        for (uint32_t q = 0; q < MTB_AUDIT_PER_LANE; q++) {
            fl[q] = 0; sp[q] = 0;
            if (j0 + q >= m) continue;
            const mtb_audit_id id = mtb_audit_lookup(in[q], info_mask, tax, tax2species, listed);
            fl[q] = id.flags; sp[q] = id.species;
        }
        /* the entry before the lane's first one: the last one of the lane below; a wave's first lane reads it back (or the carried pair) */
        uint64_t pv = __shfl_up(v[MTB_AUDIT_PER_LANE - 1], 1); int32_t ps = __shfl_up(sp[MTB_AUDIT_PER_LANE - 1], 1);
        bool has_prev = j0 > 0;
        if (lane_id() == 0 && j0 < m) {
            if (j0 > 0) { pv = values[j0 - 1]; ps = mtb_audit_lookup(info[j0 - 1], info_mask, tax, tax2species, listed).species; }
            else if (g > 0) { pv = prev_in[0]; ps = (int32_t)prev_in[1]; has_prev = true; }
        }
#pragma unroll
        for (uint32_t q = 0; q < MTB_AUDIT_PER_LANE; q++) {
            if (j0 + q >= m) continue;
            if (has_prev) {
                if (v[q] < pv) fl[q] |= 1u << MTB_AUDIT_DESCENT;
                else if (v[q] == pv && sp[q] <= ps) fl[q] |= 1u << MTB_AUDIT_DISORDER;
            }
            pv = v[q]; ps = sp[q]; has_prev = true;
            if (j0 + q + 1 == m) { prev_out[0] = pv; prev_out[1] = (uint64_t)(uint32_t)ps; }
        }
#pragma unroll
        for (int k = 0; k < MTB_AUDIT_COUNTERS; k++) mtb_audit_count(out, k, fl, g + j0);
        if (bins) {
            bool on[MTB_AUDIT_PER_LANE];
#pragma unroll
            for (uint32_t q = 0; q < MTB_AUDIT_PER_LANE; q++) on[q] = j0 + q < m && sp[q] > 0;
            mtb_audit_hist_add(bins, sp, on, fold_rounds);
        }
    }
}

/* bins[i] += the same bin of the other replicas */
__global__ __launch_bounds__(256) void k_audit_bins_reduce(uint32_t *__restrict__ bins, uint64_t n_bins, uint64_t replica_stride) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_bins) return;
    uint32_t s = bins[i];
    for (uint32_t r = 1; r < MTB_AUDIT_REPLICAS; r++) s += bins[i + r * replica_stride];
    bins[i] = s;
}

/* One lane per checkpoint of the chunk.  words[0, n_words) are the chunk's words, tile_off[t] the end words before its 2048-word
 * tile t, values[0, n_values) its entries.  Record {ad, diff_off, info_off} (offsets relative to the chunk, 0 < diff_off <= n_words)
 * is good iff words [0, diff_off) hold exactly info_off end words, word diff_off - 1 is one, and value[info_off - 1] == ad. */
__global__ __launch_bounds__(64) void k_audit_checkpoints(const uint16_t *__restrict__ words, uint64_t n_words, const uint64_t *__restrict__ tile_off,
                                                           const uint64_t *__restrict__ values, uint64_t n_values, const mtb_audit_checkpoint *__restrict__ cps, uint32_t n,
                                                           unsigned long long *__restrict__ out) {
    const uint32_t t = blockIdx.x * 64 + threadIdx.x;
    if (t >= n) return;
    const mtb_audit_checkpoint c = cps[t];
    bool good = c.diff_off > 0 && c.diff_off <= n_words;
    if (good) {
        const uint64_t tile = c.diff_off / 2048;
        uint64_t ends = tile_off[tile];
        for (uint64_t w = tile * 2048; w < c.diff_off; w++) ends += words[w] >> 15;
        good = ends == c.info_off && (words[c.diff_off - 1] & 0x8000u) && ends >= 1 && ends <= n_values && values[ends - 1] == c.ad;
    }
    if (!good) { atomicAdd(out + MTB_AUDIT_BAD_CP, 1ull); atomicMin(out + MTB_AUDIT_FIRST_BAD_CP, (unsigned long long)c.record); }
}

#endif
