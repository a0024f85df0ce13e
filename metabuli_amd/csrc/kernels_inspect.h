/* kernels_inspect.h -- mtb_database_inspect over one decoded chunk of a database (gfx950, wave64): for every group of entries with
 * equal keys (the 64-bit value, or value >> 24: the amino-acid part), the LCA of its members' ids, binned per taxon.  The rule is
 * stated once, in tests/inspect_spec.py.  The chunk is decode_chunked's: values[0, m), info[0, m); its entry 0 is entry g0 of the
 * database.  Groups cross lanes, waves, workgroups and chunks:
 *   k_inspect_tiles   a workgroup takes tiles of MTB_INSPECT_TILE entries, four consecutive ones per lane (two 16-byte loads of values,
 *                     one of info; the chunk buffers are 256-byte aligned).  Head flags: key[i] != key[i-1]; a tile's entry 0 is no
 *                     head.  A lane folds its entries serially; across lanes and waves a SEGMENTED scan of {LCA so far, size, first
 *                     entry, has a head} combines the partial folds -- valid because the pairwise LCA is associative, commutative and
 *                     idempotent on the nodes of one tree --, so a group of a thousand members costs log2 steps and never falls to one
 *                     lane.  Groups that begin and end inside the tile are binned there.  The tile's first segment (it may continue a
 *                     group from the left) and its last one (open to the right) are not: they go to the tile's two records; a tile
 *                     that lies wholly inside one group writes one record and an empty one.
 *   k_inspect_walk    one wave walks the chunk's 2 * tiles records in order, 64 at a time, by the same segmented scan, in front of
 *                     them the record carried from the previous chunk; what closes is binned, what stays open is carried out (two
 *                     carry slots used in turn).  256 M entries are 512 k records.  With `final` the carry is closed: the database's
 *                     last entry is part of its group.
 * No workgroup waits for another and nothing depends on launch order.
 * Bins: distinct[t] += 1, entries[t] += |g|, u32 per pass (a chunk has fewer than 2^32 entries) in MTB_AUDIT_REPLICAS replicas that
 * k_audit_bins_reduce sums and k_cov_accumulate adds to the u64 sums after every chunk; the walk's few groups, whose sizes are
 * unbounded, add to the u64 sums directly.  Entries are in value order, so the LCAs of neighbouring groups are the SAME few high nodes
 * (the root, a domain), and adds to one address serialise at 88 M/s (kernels_audit.h): in mtb_inspect_hist_add a lane that holds a
 * taxon twice among its groups, or the taxon its neighbour lane holds, offers it (a taxon of share p is offered by a lane with
 * probability >= p^2: a hot one nearly always, a rare one hardly ever -- the audit's rule, profiles/audit_notes.md); the wave takes
 * the first offer, sums count and weight of every lane that holds that taxon by a wave reduction and adds once;
 * MTB_INSPECT_FOLD_ROUNDS such rounds at most, then what is left adds singly.  Without an offer this costs one shuffle and a ballot.
 * Group sizes, orphans and the largest group are gathered in LDS and leave a workgroup once, at its end.
 * Bytes: 12 B read per entry, one canon[] lookup per entry, depth[] / parent[] climbs only where two different nodes meet; 32 B
 * written per 1024 entries. */
#ifndef MTB_KERNELS_INSPECT_H
#define MTB_KERNELS_INSPECT_H
#include "dev_util.h"
#include "mtb_core.h"
#include "kernels_audit.h"

#define MTB_INSPECT_PER_LANE 4u
#define MTB_INSPECT_TILE (256u * MTB_INSPECT_PER_LANE)
#define MTB_INSPECT_FOLD_ROUNDS 3
#define MTB_INSPECT_HIST 40

/* the words of `out`: orphan groups / entries, the largest group closed inside a tile as (size << 48) | (2^48 - 1 - first entry) (0: none),
 * the largest one the walk closed (size, first entry), the size histogram */
enum { MTB_INSPECT_ORPHAN_GROUPS = 0, MTB_INSPECT_ORPHAN_ENTRIES = 1, MTB_INSPECT_TILE_MAX = 2, MTB_INSPECT_WALK_MAX = 3, MTB_INSPECT_WALK_FIRST = 4,
       MTB_INSPECT_HIST0 = 5, MTB_INSPECT_WORDS = MTB_INSPECT_HIST0 + MTB_INSPECT_HIST };
#define MTB_INSPECT_FIRST_MASK 0xFFFFFFFFFFFFull

/* an open part of a group: size 0 = none.  acc: the LCA of the known members so far, -1 = none known yet.  head: the part begins at a head
 * flag -- a tile's right record always does --, so it continues nothing, whatever its key: on an unsorted list a key may come back
 * (A.., B.., A..) and the rule keeps the two runs apart.  Without it the key of the entry before decides. */
typedef struct { uint64_t key, first, size; int32_t acc; int32_t head; } mtb_inspect_rec;

/* a segment of the scans: U = uint32_t inside a tile (sizes and first entries relative to the tile), uint64_t in the walk (of the database) */
template <typename U> struct mtb_inspect_seg_t { U size, first; int32_t acc; uint32_t head; };
typedef mtb_inspect_seg_t<uint32_t> mtb_inspect_seg;
typedef mtb_inspect_seg_t<uint64_t> mtb_inspect_wseg;

__device__ __forceinline__ uint64_t mtb_inspect_key(uint64_t value, int level) { return level ? value >> 24 : value; }
/* of two canonical nodes, -1 = none */
__device__ __forceinline__ int32_t mtb_inspect_join(const mtb_tax_view &tax, int32_t a, int32_t b) {
    if (a < 0) return b;
    if (b < 0 || a == b) return a;
    return mtb_lca(&tax, a, b);
}
/* L, then R behind it */
template <typename U>
__device__ __forceinline__ mtb_inspect_seg_t<U> mtb_inspect_combine(const mtb_tax_view &tax, const mtb_inspect_seg_t<U> &L, const mtb_inspect_seg_t<U> &R) {
    if (R.head || L.size == 0) return R;
    if (R.size == 0) return L;
    mtb_inspect_seg_t<U> o;
    o.acc = mtb_inspect_join(tax, L.acc, R.acc); o.size = L.size + R.size; o.first = L.first; o.head = L.head;
    return o;
}
template <typename U>
__device__ __forceinline__ mtb_inspect_seg_t<U> mtb_inspect_seg_up(const mtb_inspect_seg_t<U> &s, int d) {
    mtb_inspect_seg_t<U> o;
    o.acc = __shfl_up(s.acc, d, 64); o.size = __shfl_up(s.size, d, 64); o.first = __shfl_up(s.first, d, 64); o.head = __shfl_up(s.head, d, 64);
    return o;
}

/* distinct[t[q]] += 1, entries[t[q]] += w[q] for the lane's N groups with on[q]; wave-uniform control flow.  W: the weights' type, B:
 * the bins' (u32 bins of a pass from the tiles, the u64 sums from the walk).  A lane offers a taxon it holds twice, or the one its
 * neighbour lane holds too; the wave takes the first offer, sums count and weight over all lanes and adds once. */
template <int N, typename W, typename B>
__device__ __forceinline__ void mtb_inspect_hist_add(B *__restrict__ distinct, B *__restrict__ entries, const int32_t (&t)[N], const W (&w)[N], bool (&on)[N], int rounds) {
    for (int r = 0; r < rounds; r++) {
        int32_t mine = -1, offer = -1;
#pragma unroll
        for (int q = N - 1; q >= 0; q--) if (on[q]) mine = t[q];
#pragma unroll
        for (int a = 0; a + 1 < N; a++)
#pragma unroll
            for (int b = a + 1; b < N; b++) if (on[a] && on[b] && t[a] == t[b]) offer = t[a];
        const int32_t beside = __shfl_xor(mine, 1, 64);
        if (offer < 0 && mine >= 0 && mine == beside) offer = mine;
        const uint64_t have = __ballot(offer >= 0);
        if (have == 0) break;
        const int leader = __ffsll((long long)have) - 1;
        const int32_t t0 = rl_i(offer, leader);
        uint32_t n = 0; W sum = 0;
#pragma unroll
        for (int q = 0; q < N; q++) if (on[q] && t[q] == t0) { n++; sum += w[q]; on[q] = false; }
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) { n += __shfl_xor(n, d, 64); sum += __shfl_xor(sum, d, 64); }
        if ((int)lane_id() == leader) { atomicAdd(distinct + t0, (B)n); atomicAdd(entries + t0, (B)sum); }
    }
#pragma unroll
    for (int q = 0; q < N; q++) if (on[q]) { atomicAdd(distinct + t[q], (B)1); atomicAdd(entries + t[q], (B)w[q]); }
}

/* entries [0, m) of a chunk whose entry 0 is entry g0 of the database; recs: two records per tile; distinct / entries: u32 bins of
 * the pass, MTB_AUDIT_REPLICAS arrays replica_stride apart each, of which a workgroup takes the one of its XCD; out: MTB_INSPECT_WORDS words */
__global__ __launch_bounds__(256) void k_inspect_tiles(const uint64_t *__restrict__ values, const uint32_t *__restrict__ info, uint64_t m, uint64_t g0, uint32_t info_mask, int level,
                                                        mtb_tax_view tax, mtb_inspect_rec *__restrict__ recs, uint32_t *__restrict__ distinct, uint32_t *__restrict__ entries,
                                                        uint64_t replica_stride, int fold_rounds, unsigned long long *__restrict__ out) {
    __shared__ mtb_inspect_seg s_tot[4];
    __shared__ uint32_t s_hist[MTB_INSPECT_HIST];
    __shared__ uint32_t s_orphan[2];
    __shared__ unsigned long long s_max;
    distinct += (blockIdx.x & (MTB_AUDIT_REPLICAS - 1u)) * replica_stride;              /* (workgroups go round the XCDs in launch order) */
    entries += (blockIdx.x & (MTB_AUDIT_REPLICAS - 1u)) * replica_stride;
    if (threadIdx.x < MTB_INSPECT_HIST) s_hist[threadIdx.x] = 0;
    if (threadIdx.x < 2) s_orphan[threadIdx.x] = 0;
    if (threadIdx.x == 0) s_max = 0;
    const uint32_t wv = threadIdx.x >> 6, lane = lane_id();
    const uint32_t e0 = threadIdx.x * MTB_INSPECT_PER_LANE;                             /* the lane's first entry in the tile */
    const uint64_t n_tiles = (m + MTB_INSPECT_TILE - 1) / MTB_INSPECT_TILE;
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {               /* (every lane of a workgroup runs the same number of rounds) */
        const uint64_t base = tile * MTB_INSPECT_TILE, j0 = base + e0;
        const uint32_t mt = (uint32_t)(m - base < MTB_INSPECT_TILE ? m - base : MTB_INSPECT_TILE);      /* entries of the tile */
        uint64_t key[MTB_INSPECT_PER_LANE]; uint32_t in[MTB_INSPECT_PER_LANE];
        if (j0 + MTB_INSPECT_PER_LANE <= m) {
            const uint4 a = *(const uint4 *)(values + j0), c = *(const uint4 *)(values + j0 + 2), i4 = *(const uint4 *)(info + j0);
            key[0] = a.x | ((uint64_t)a.y << 32); key[1] = a.z | ((uint64_t)a.w << 32); key[2] = c.x | ((uint64_t)c.y << 32); key[3] = c.z | ((uint64_t)c.w << 32);
            in[0] = i4.x; in[1] = i4.y; in[2] = i4.z; in[3] = i4.w;
        } else {
#pragma unroll
            for (uint32_t q = 0; q < MTB_INSPECT_PER_LANE; q++) { const bool has = j0 + q < m; key[q] = has ? values[j0 + q] : 0; in[q] = has ? info[j0 + q] : 0; }
        }
#pragma unroll
        for (uint32_t q = 0; q < MTB_INSPECT_PER_LANE; q++) key[q] = mtb_inspect_key(key[q], level);
        /* the key before the lane's first one: the last one of the lane below; a wave's first lane reads it back */
        uint64_t pk = __shfl_up(key[MTB_INSPECT_PER_LANE - 1], 1, 64);
        if (lane == 0 && wv > 0 && j0 < m) pk = mtb_inspect_key(values[j0 - 1], level);
        /* the lane's own fold: `pre` is what lies before its first head, `cur` what lies from its last head on (all of it without a
         * head); the groups between two of its heads are closed here */
        mtb_inspect_seg pre, cur;
        pre.acc = -1; pre.size = 0; pre.first = e0; pre.head = 0; cur = pre;
        int32_t ct[MTB_INSPECT_PER_LANE]; uint32_t cw[MTB_INSPECT_PER_LANE], cf[MTB_INSPECT_PER_LANE];
        bool seen = false;
#pragma unroll
        for (uint32_t q = 0; q < MTB_INSPECT_PER_LANE; q++) {
            ct[q] = -1; cw[q] = 0; cf[q] = 0;
            if (e0 + q >= mt) continue;
            const int32_t id = mtb_tax_canon(&tax, (int32_t)(in[q] & info_mask));
            const bool head = q > 0 ? key[q] != key[q - 1] : (threadIdx.x > 0 && key[0] != pk);
            if (head) {
                if (!seen) { pre = cur; seen = true; }
                else { ct[q] = cur.acc; cw[q] = cur.size; cf[q] = cur.first; }
                cur.acc = id; cur.size = 1; cur.first = e0 + q; cur.head = 1;
            } else {
                cur.acc = mtb_inspect_join(tax, cur.acc, id); cur.size++;
            }
        }
        /* inclusive segmented scan of `cur` over the wave, then over the waves before this one */
        mtb_inspect_seg S = cur;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const mtb_inspect_seg o = mtb_inspect_seg_up(S, d);
            if ((int)lane >= d) S = mtb_inspect_combine(tax, o, S);
        }
        __syncthreads();                                                                /* s_tot of the previous tile has been read */
        if (lane == 63) s_tot[wv] = S;
        __syncthreads();
        mtb_inspect_seg carry;
        carry.acc = -1; carry.size = 0; carry.first = 0; carry.head = 0;
        for (uint32_t k = 0; k < wv; k++) carry = mtb_inspect_combine(tax, carry, s_tot[k]);
        S = mtb_inspect_combine(tax, carry, S);
        mtb_inspect_seg G = mtb_inspect_seg_up(S, 1);                                    /* everything before this lane, up to the last head */
        if (lane == 0) G = carry;
        /* the group that ends at the lane's first head */
        if (seen) {
            G = mtb_inspect_combine(tax, G, pre);
            if (G.head) { ct[0] = G.acc; cw[0] = G.size; cf[0] = G.first; }
            else {                                                                       /* it began at the tile's first entry: the tile's left record */
                mtb_inspect_rec r; r.key = mtb_inspect_key(values[base], level); r.first = g0 + base; r.size = G.size; r.acc = G.acc; r.head = 0;
                recs[2 * tile] = r;
            }
        }
        if (threadIdx.x == 255) {                                                       /* what is open at the tile's end */
            mtb_inspect_rec r, none; r.key = mtb_inspect_key(values[base + mt - 1], level); r.first = g0 + base + S.first; r.size = S.size; r.acc = S.acc; r.head = 1;
            none.key = 0; none.first = 0; none.size = 0; none.acc = -1; none.head = 0;
            if (S.head) recs[2 * tile + 1] = r;
            else { r.first = g0 + base; r.head = 0; recs[2 * tile] = r; recs[2 * tile + 1] = none; }   /* not one head: the tile lies inside one group */
        }
        /* the groups closed here: sizes, the largest, orphans, bins */
        bool on[MTB_INSPECT_PER_LANE];
        unsigned long long big = 0;
        uint32_t n_orphan = 0, w_orphan = 0;
#pragma unroll
        for (uint32_t q = 0; q < MTB_INSPECT_PER_LANE; q++) {
            on[q] = false;
            if (cw[q] == 0) continue;
            atomicAdd(&s_hist[31 - __clz((int)cw[q])], 1u);
            const unsigned long long p = ((unsigned long long)cw[q] << 48) | (MTB_INSPECT_FIRST_MASK - ((g0 + base + cf[q]) & MTB_INSPECT_FIRST_MASK));
            big = p > big ? p : big;
            if (ct[q] < 0) { n_orphan++; w_orphan += cw[q]; } else on[q] = true;
        }
        if (big) atomicMax(&s_max, big);
        if (n_orphan) { atomicAdd(&s_orphan[0], n_orphan); atomicAdd(&s_orphan[1], w_orphan); }
        mtb_inspect_hist_add(distinct, entries, ct, cw, on, fold_rounds);
    }
    __syncthreads();
    if (threadIdx.x < MTB_INSPECT_HIST && s_hist[threadIdx.x]) atomicAdd(out + MTB_INSPECT_HIST0 + threadIdx.x, (unsigned long long)s_hist[threadIdx.x]);
    if (threadIdx.x < 2 && s_orphan[threadIdx.x]) atomicAdd(out + MTB_INSPECT_ORPHAN_GROUPS + threadIdx.x, (unsigned long long)s_orphan[threadIdx.x]);
    if (threadIdx.x == 0 && s_max) atomicMax(out + MTB_INSPECT_TILE_MAX, s_max);
}

/* the wave's closed groups {t, w, first} (w == 0: none in this lane) into the u64 sums and `out`; *mx / *mx_first: the largest so far */
__device__ __forceinline__ void mtb_inspect_walk_close(int32_t t, uint64_t w, uint64_t first, unsigned long long *__restrict__ distinct_sum,
                                                       unsigned long long *__restrict__ entries_sum, unsigned long long *__restrict__ out, int rounds,
                                                       uint64_t *mx, uint64_t *mx_first) {
    if (__ballot(w != 0) == 0) return;
    /* the largest of them, the first of equals */
    uint64_t bw = w, bf = w ? first : ~0ull;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const uint64_t ow = __shfl_xor(bw, d, 64), of = __shfl_xor(bf, d, 64);
        if (ow > bw || (ow == bw && of < bf)) { bw = ow; bf = of; }
    }
    if (bw > *mx || (bw == *mx && bw != 0 && bf < *mx_first)) { *mx = bw; *mx_first = bf; }
    /* sizes: one add per slot of the histogram that the wave met */
    int slot = -1;
    if (w) { slot = 63 - __clzll((long long)w); slot = slot < MTB_INSPECT_HIST ? slot : MTB_INSPECT_HIST - 1; }
    for (uint64_t pending = __ballot(slot >= 0); pending;) {
        const int leader = __ffsll((long long)pending) - 1;
        const uint64_t same = __ballot(slot == rl_i(slot, leader));
        if ((int)lane_id() == leader) atomicAdd(out + MTB_INSPECT_HIST0 + slot, (unsigned long long)__popcll(same));
        pending &= ~same;
    }
    if (w && t < 0) { atomicAdd(out + MTB_INSPECT_ORPHAN_GROUPS, 1ull); atomicAdd(out + MTB_INSPECT_ORPHAN_ENTRIES, (unsigned long long)w); }
    const int32_t ts[1] = {t}; const uint64_t ws[1] = {w}; bool on[1] = {w != 0 && t >= 0};
    mtb_inspect_hist_add(distinct_sum, entries_sum, ts, ws, on, rounds);
}

/* One wave.  recs[0, n_recs): the chunk's tile records in order; carry_in: the open group before them (read iff has_carry);
 * carry_out receives the open group behind them -- or, with `final`, an empty record: the last group is closed. */
__global__ __launch_bounds__(64) void k_inspect_walk(const mtb_inspect_rec *__restrict__ recs, uint64_t n_recs, const mtb_inspect_rec *__restrict__ carry_in, int has_carry,
                                                      mtb_inspect_rec *__restrict__ carry_out, int final, mtb_tax_view tax, unsigned long long *__restrict__ distinct_sum,
                                                      unsigned long long *__restrict__ entries_sum, int fold_rounds, unsigned long long *__restrict__ out) {
    const uint32_t lane = lane_id();
    mtb_inspect_rec C;
    C.key = 0; C.first = 0; C.size = 0; C.acc = -1; C.head = 0;
    if (has_carry) C = *carry_in;
    uint64_t mx = out[MTB_INSPECT_WALK_MAX], mx_first = out[MTB_INSPECT_WALK_FIRST];
    mtb_inspect_rec none, next;
    none.key = 0; none.first = 0; none.size = 0; none.acc = -1; none.head = 0;
    next = lane < n_recs ? recs[lane] : none;
    for (uint64_t base = 0; base < n_recs; base += 64) {                                /* base, C, mx are wave-uniform */
        const mtb_inspect_rec r = next;
        next = base + 64 + lane < n_recs ? recs[base + 64 + lane] : none;                /* (in flight while these 64 are worked on) */
        const bool valid = r.size != 0;
        mtb_inspect_wseg Cs;
        Cs.size = C.size; Cs.first = C.first; Cs.acc = C.acc; Cs.head = 1;
        /* the usual case of a database with short groups: 64 records with entries, each of another group than the one before it
         * -- each closes its predecessor as it stands, and nothing is folded */
        const uint64_t before = __shfl_up(r.key, 1, 64);
        const bool alone = valid && (r.head != 0 || (lane == 0 ? (C.size == 0 || C.key != r.key) : before != r.key));
        if (__ballot(alone) == ~0ull) {
            mtb_inspect_wseg G;
            G.size = __shfl_up(r.size, 1, 64); G.first = __shfl_up(r.first, 1, 64); G.acc = __shfl_up(r.acc, 1, 64); G.head = 1;
            if (lane == 0) G = Cs;
            mtb_inspect_walk_close(G.acc, G.size, G.first, distinct_sum, entries_sum, out, fold_rounds, &mx, &mx_first);
            C.key = __shfl(r.key, 63, 64); C.size = __shfl(r.size, 63, 64); C.first = __shfl(r.first, 63, 64); C.acc = __shfl(r.acc, 63, 64);
            continue;
        }
        /* the key of the last record with entries at or before each lane, then before it */
        uint64_t k = r.key; uint32_t v = valid ? 1u : 0u;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint64_t ok = __shfl_up(k, d, 64); const uint32_t ov = __shfl_up(v, d, 64);
            if ((int)lane >= d && !v) { k = ok; v = ov; }
        }
        uint64_t pk = __shfl_up(k, 1, 64); uint32_t pv = __shfl_up(v, 1, 64);
        if (lane == 0) pv = 0;
        if (!pv) { pk = C.key; pv = C.size != 0 ? 1u : 0u; }
        mtb_inspect_wseg S;
        S.size = r.size; S.first = r.first; S.acc = r.acc; S.head = valid && (r.head != 0 || !pv || pk != r.key) ? 1u : 0u;
        const bool closes = S.head != 0;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const mtb_inspect_wseg o = mtb_inspect_seg_up(S, d);
            if ((int)lane >= d) S = mtb_inspect_combine(tax, o, S);
        }
        S = mtb_inspect_combine(tax, Cs, S);
        mtb_inspect_wseg G = mtb_inspect_seg_up(S, 1);
        if (lane == 0) G = Cs;
        mtb_inspect_walk_close(G.acc, closes ? G.size : 0, G.first, distinct_sum, entries_sum, out, fold_rounds, &mx, &mx_first);
        /* what is open behind the 64 records */
        const uint32_t any = __shfl(v, 63, 64);
        const uint64_t lk = __shfl(k, 63, 64);
        C.size = __shfl(S.size, 63, 64); C.first = __shfl(S.first, 63, 64); C.acc = __shfl(S.acc, 63, 64);
        if (any) C.key = lk;
    }
    if (final) {
        mtb_inspect_walk_close(C.acc, lane == 0 ? C.size : 0, C.first, distinct_sum, entries_sum, out, fold_rounds, &mx, &mx_first);
        C.key = 0; C.first = 0; C.size = 0; C.acc = -1;
    }
    if (lane == 0) { *carry_out = C; out[MTB_INSPECT_WALK_MAX] = mx; out[MTB_INSPECT_WALK_FIRST] = mx_first; }
}

#endif
