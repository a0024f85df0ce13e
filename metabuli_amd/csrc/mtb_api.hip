/* mtb_api.hip -- C ABI (include/mtb.h) over the HIP kernels.  gfx950 only.
 * The library never falls back to a CPU path: every entry point that computes
 * launches kernels on the context's stream and reports HIP errors.           */
#include <hip/hip_runtime.h>

#include <fcntl.h>
#include <limits.h>
#include <stdlib.h>
#include <sys/stat.h>
#include <unistd.h>

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <mutex>
#include <functional>
#include <map>
#include <string>
#include <thread>
#include <vector>

#include "../../include/mtb.h"
#include "host_db.h"
#include "host/merge_plan.h"
#include "host/audit_plan.h"
#include "host/clade_filter.h"
#include "kernels_extract.h"
#include "kernels_extract_blocks.h"
#include "kernels_index.h"
#include "kernels_join.h"
#include "kernels_build.h"
#include "kernels_merge.h"
#include "kernels_clade_filter.h"
#include "kernels_audit.h"
#include "kernels_coverage.h"
#include "kernels_inspect.h"
#include "kernels_dir.h"
#include "kernels_scan.h"
#include "kernels_score.h"
#include "kernels_score_fast.h"
#include "kernels_score_long.h"
#include "kernels_score_many.h"
#include "kernels_seg_order.h"
#include "kernels_sort.h"
#include "mtb_core.h"
#include "mtb_options.h"

#if defined(__HIP_DEVICE_COMPILE__) && defined(__AMDGCN__) && !defined(__gfx950__)
#error "libmtb is written for gfx950 (MI355X) only: 160 KB of LDS per CU (k_score_long holds 70 KB per workgroup), global_load_lds_dwordx4, wave64"
#endif

static thread_local std::string g_err;
static mtb_status fail(mtb_status s, const std::string &m) { g_err = m; return s; }

#define HIPCHK(x)                                                                                  \
    do {                                                                                           \
        hipError_t e_ = (x);                                                                       \
        if (e_ != hipSuccess)                                                                      \
            return fail(MTB_ERR_DEVICE, std::string(#x) + ": " + hipGetErrorString(e_));           \
    } while (0)
#define STCHK(x)                                                                                   \
    do { mtb_status s_ = (x); if (s_ != MTB_OK) return s_; } while (0)

/* Query::taxCnt lists packed back to back before they cross PCIe: the scorer leaves every read's entries inside a slot sized by
 * its bound (one per position bucket, 18 for a 150 bp read) while a read has one or two entries -- copying the slots moved 10 x
 * the payload over pageable D2H copies (the driver's GPU stage was 1.05 s per 8 M reads, the kernels 0.1 s of it). */
__global__ __launch_bounds__(256) void k_taxcnt_n(const mtb_result *__restrict__ res, uint64_t n, uint32_t *__restrict__ cnt) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) cnt[i] = res[i].n_taxcnt;
}
__global__ __launch_bounds__(256) void k_taxcnt_pack(mtb_result *__restrict__ res, uint64_t n, const uint64_t *__restrict__ new_off, const int32_t *__restrict__ tt,
                                                      const uint32_t *__restrict__ tc, int32_t *__restrict__ tt2, uint32_t *__restrict__ tc2) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t k = res[i].n_taxcnt, src = res[i].taxcnt_off;
    const uint64_t dst = new_off[i];
    for (uint32_t j = 0; j < k; j++) { tt2[dst + j] = tt[src + j]; tc2[dst + j] = tc[src + j]; }
    res[i].taxcnt_off = (uint32_t)dst;
}

/* 2-bit reads (mtb_classify_batch_packed): slots of 8 bases a read needs; bases of read r written as text behind offs[r] */
__global__ __launch_bounds__(256) void k_pack_slots(const uint32_t *__restrict__ lens, uint64_t n, uint32_t *__restrict__ slots) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) slots[i] = (lens[i] + 7u) >> 3;
}
__global__ __launch_bounds__(64) void k_unpack_reads(const uint8_t *__restrict__ packed2, const uint8_t *__restrict__ nmask, const uint64_t *__restrict__ offs,
                                                     const uint64_t *__restrict__ slot_off, uint64_t n, char *__restrict__ bases) {
    for (uint64_t r = blockIdx.x; r < n; r += gridDim.x) {
        const uint64_t o = offs[r], s0 = slot_off[r];
        const uint32_t L = (uint32_t)(offs[r + 1] - o);
        for (uint32_t k = threadIdx.x; k < L; k += 64) {            /* one base per lane: a wave writes 64 consecutive bytes */
            const uint64_t g = s0 + (k >> 3); const uint32_t j = k & 7u;
            const uint32_t w = (uint32_t)packed2[2 * g] | ((uint32_t)packed2[2 * g + 1] << 8);
            const bool bad = (nmask[g] >> j) & 1u;
            const uint32_t c = (w >> (2 * j)) & 3u;
            bases[o + k] = bad ? 'N' : (char)((0x47544341u >> (8 * c)) & 0xFFu);       /* "ACTG": GeneticCode's nuc2int order */
        }
    }
}

/* what an entry is, said by its first ensure(): BUF_IO = a call's inputs / outputs (host-buffer entry points), not workspace; BUF_FIXED = workspace that does not grow with the sub-batch (the slab pool) */
enum BufKind : uint8_t { BUF_WORK = 0, BUF_IO = 1, BUF_FIXED = 2 };
struct DevBuf { void *p = nullptr; size_t cap = 0; BufKind kind = BUF_WORK; };
/* the slab pool of the generic scorer's large-segment launches (reads beyond every LDS budget: 2 of 200 k long reads on the bench's index).  Round 6: 16 GiB
 * instead of 48 -- the 32 GiB went to the long-read sub-batches (200 k x 10 kb: two of 100 k reads instead of four of 50 k; denser sorted queries) */
#define MTB_SLAB_POOL_MAX (16ull << 30)
#define MTB_LONG_WIN_MAX_PER_Q 24.0   /* long reads: targets per query metamer up to which the window form is taken without being asked for */
#define MTB_OVF_STRIPES 256u
/* score stage of a short-read batch: the deferred tier beside k_score_fast on a side stream (score_fixed_slots); 0 = one stream, one kernel after
 * another (what a context with profiling on does in any build).  k_score_many's workgroups per CU while it shares the CUs. */
#ifndef MTB_SCORE_OVERLAP
#define MTB_SCORE_OVERLAP 1
#endif
#ifndef MTB_SCORE_OVERLAP_GRID
#define MTB_SCORE_OVERLAP_GRID 4u
#endif

/* The context's device scalars (mtb_ctx::d_scal), one 8-byte word per name.  Names cleared or read back with ONE call stay adjacent; two names share a word only where noted. */
enum Scal : uint32_t {
    SC_JOIN_COUNT = 0, SC_JOIN_OVERFLOW = 1,     /* dev_join: matches (slot modes: overflow entries) found; the kernels' overflow flag */
    SC_BAD_SEQ = SC_JOIN_OVERFLOW,               /* k_slot_place / k_count_reads: a sequenceID outside the batch.  Shared: k_slot_place runs in the join's place (mtb_part_score); count_reads reads its flag back before it returns */
    SC_N_LARGE = 2, SC_MAX_SEG = 3,              /* exact segments (dev_segsort, score_join_order): segments beyond the LDS sort, the largest segment */
    SC_MAX_LEN = 4, SC_OPEN_CARRY = 5,           /* dev_extract: longest read; index open (decode_chunked): last flat value of the previous chunk */
    SC_N_GENERIC = 6, SC_LONG_N_SECOND = 7,      /* reads a listing scorer left to the generic kernel (take_generic_reads); dev_score_long: reads flagged for its second launch */
    SC_EXTRACT = 8, SC_WIN_STATS = 16,           /* 8 words, struct ExtractCounters; 2 words: the window join's tiles with a window / outside it */
    SC_N_UNGROUPED = 18, SC_MAX_BIG_SEG = 19, SC_N_DEFERRED = 20, SC_DEFER_N_LARGE = 21,     /* score_fixed_slots' deferred reads: ungrouped overflow entries, largest segment, number, segments beyond the LDS sort */
    SC_SCORE_WORK = 22, SC_LONG_WORK = 24,       /* work counters: dev_score's two passes (2 words), k_score_long */
    SC_LS_N_FAIL = 25, SC_LS_N_ALL = 26, SC_LS_MAX_SEG = 27, SC_LS_WORK = 28,    /* long-read slot path: reads beyond k_seg_order's LDS tables, matches of the range, those reads' largest segment, k_seg_order's work counter */
    SC_OPEN_FLAGS = 29, SC_WORDS = 30            /* index open: the directory kernels' two 32-bit flags */
};
struct ExtractCounters { uint64_t records /* allocated, incl. blank tails */, overflow, real, max_q /* most metamers of a read */, off_max_q, off_reads, off_max_len /* marked-read statistics */, spare; };
static_assert(sizeof(ExtractCounters) == 8 * (SC_WIN_STATS - SC_EXTRACT) && SC_WIN_STATS + 2 <= SC_N_UNGROUPED && SC_SCORE_WORK + 2 <= SC_LONG_WORK && SC_OPEN_FLAGS < SC_WORDS, "scalar names overlap or leave the block");
struct mtb_ctx {
    int device = 0;
    int audit_mode = 0;              /* mtb_debug_audit_mode (measurements): how mtb_database_audit takes the species counts */
    hipStream_t stream = nullptr;
    mtb_tables *d_tabs = nullptr;
    mtb_tables h_tabs;
    std::map<std::string, DevBuf> bufs;
    std::mutex bufs_mu;              /* the buffer table may be grown from a helper thread (mtb_ctx_reserve) while the context's thread opens an index */
    std::mutex reserve_mu;           /* held by mtb_ctx_reserve for its whole run */
    std::atomic<bool> reserve_cancel{false};     /* an index open on this context found device memory short: a running reservation stops after its current buffer, a new one does nothing, and what was reserved is handed back (open_make_room) */
    uint64_t *d_scal = nullptr;      /* SC_WORDS device scalars, one 8-byte word per Scal name: scal<T>(c, SC_X) */
    unsigned long long *d_ovfctr = nullptr;      /* MTB_OVF_STRIPES counters of the striped overflow list, 64 bytes apart (JoinSegArgs::ovf_stripes) */
    uint64_t ovf_region = 0, ovf_max_region = 0; /* entries per region in the last slot-mode join; fullest region */
    hipEvent_t ev[8];
    mtb_batch_stats stats;
    int profiling = 0;
    struct KEv { int id; hipEvent_t a, b; };
    std::vector<KEv> kev;            /* events of the current batch      */
    std::vector<hipEvent_t> ev_pool; /* recycled events                  */
    std::vector<mtb_ctx *> lanes;    /* extra stream contexts (mtb_ctx_set_streams) */
    bool is_lane = false;            /* lanes share the parent's tables  */
    uint32_t seg_epoch = 0;          /* tag of the live slots in the "segm" buffer (1..MTB_SLOT_EPOCHS) */
    const void *seg_clean_p = nullptr; size_t seg_clean_cap = 0;     /* the allocation the epoch count belongs to: the one make_slots last cleared (another pointer or size, e.g. after mtb_ctx_reserve grew or created "segm", holds stale bytes) */
    double extract_yield = 0.0;      /* metamers per base of the previous batch (single-pass extraction buffer sizing) */
    uint64_t part_n_reads = 0; uint32_t part_max_len = 0;   /* batch state between mtb_part_extract and mtb_part_score */
    int part_mode = 0; uint32_t part_max_q = 0; uint64_t part_nk_real = 0;      /* part_mode 1: the batch's metamers carry ordinals, the matches come home into slot segments */
    bool placement_probe = false;    /* mtb_ctx_set_placement_probe: a new big slot buffer is chosen among candidate allocations */
    uint64_t ws_limit = 0;           /* workspace budget of a batch in bytes; 0 = what hipMemGetInfo reports free (+ what the context holds) */
    double ws_per_base = 0.0;        /* workspace bytes per base: what the buffers hold / the largest sub-batch they were grown for (HBM-budgeted batching) */
    uint64_t ws_max_sub_bases = 0;   /* bases of the largest sub-batch since the workspace was last released */
    int ws_seq_mode = 0;             /* the buffer sets of short and long reads differ: a change of mode releases the workspace */
    uint32_t last_sub_batches = 0;
    bool fast_used = false;          /* a scorer that lists what it leaves to the generic kernel ran (dev_score's k_score_fast, dev_score_long): SC_N_GENERIC holds the count (take_generic_reads) */
    const mtb_kmer *last_sorted = nullptr; uint64_t last_sorted_n = 0;       /* the last fused slot-path batch's sorted metamers (mtb_ctx_join_footprint) */
    /* what the join leaves dead until the next batch's extraction -- the metamer buffer that does NOT hold the sorted list, both digit arrays: the scorer's large
     * per-batch temporaries (the grouped overflow list, the deferred reads' segments) are carved out of them (scratch()) instead of being allocations of their own:
     * 10 M reads of held-out genomes need 133 instead of 154 GiB of workspace -- one sub-batch instead of two on a 288 GB part next to a 126 GiB index */
    struct DeadSeg { char *p; size_t cap, used; };
    DeadSeg dead[3]; int n_dead = 0;
    uint64_t last_scratch_bytes = 0;     /* mtb_ctx_last_scratch_bytes */
    /* upload of the NEXT batch's packed reads while the current batch computes (mtb_prefetch_batch_packed): a copy stream, two sets of
     * input buffers, and what the set that is being filled holds */
    hipStream_t copy_stream = nullptr; hipEvent_t copy_done[2] = {nullptr, nullptr};       /* per input buffer set: the prefetch into it is complete */
    hipEvent_t unpacked[2] = {nullptr, nullptr};     /* per set: the last classify call that read it has unpacked it (recorded on the compute stream; a prefetch into the set waits for it) */
    bool unpacked_rec[2] = {false, false};
    uint64_t prefetch_issued = 0, prefetch_used = 0; /* mtb_ctx_prefetch_stats */
    /* results on their way back while the next batch computes (mtb_classify_batch_packed_async): a download stream, the event that closes the
     * queued copies, and which of the two device-side result buffer sets the next call writes */
    hipStream_t down_stream = nullptr; hipEvent_t down_ready = nullptr, down_done = nullptr; bool down_pending = false; int res_set = 0;
    int pk_set = 0;                                  /* the set the last classify call read */
    /* the deferred tier of a short-read batch beside k_score_fast (score_fixed_slots): a side stream made right after the compute stream, so that the
     * two take neighbouring hardware queues, and the events of the fork (0), of the tier's first scorer being queued (1) and of the tier's end (2) */
    hipStream_t side_stream = nullptr; hipEvent_t side_ev[3] = {nullptr, nullptr, nullptr};
    uint32_t score_overlapped = 0;                   /* last slot-path batch: its deferred tier ran on the side stream */
    /* one record per set.  The protocol of mtb.h is prefetch(k+1), classify(k): when batch k+1 is prefetched, batch k (prefetched one call
     * earlier) is still waiting for its classify call, so TWO prefetches are outstanding for a moment -- with a single record classify(k)
     * found batch k+1's key, discarded it and uploaded k again */
    struct Prefetched { const void *key = nullptr, *key2 = nullptr; uint64_t n_reads = 0; bool valid = false; } pre[2];
    struct JoinTune { uint64_t key = 0; int calls = 0, pending = -1, best = -1; float ms[3] = {0.0f, 0.0f, 0.0f}; hipEvent_t e0 = nullptr, e1 = nullptr; } join_tunes[4]; uint32_t join_tune_next = 0;      /* dev_join: the short-read instantiation that is fastest for this index and batch size */
    uint64_t many_stats[4] = {0, 0, 0, 0};           /* last slot-path batch: reads deferred by the first scoring launches, of those scored by k_score_many, their matches, the survivors of the dead-species drop */
    uint32_t lslot_tf_start = 1;                     /* long-read slot ranges: tail factor the next batch starts with (1 = a quarter of the metamers, 4 = all) */
    /* k-mer coverage (mtb_index_coverage_*): the hits of the classify call in work, per species + MTB_COV_EXTRA words, committed into the index's bins at
     * its successful end (CovCall).  Outside the buffer table: an out-of-memory retry inside the call releases the workspace.  Lanes borrow the parent's. */
    unsigned long long *d_cov_pend = nullptr; uint64_t cov_pend_words = 0; bool cov_call = false;
    MtbOptions opt;                                  /* the experiment / diagnosis switches: the MTB_* environment at mtb_ctx_create, mtb_ctx_set_option afterwards (mtb_options.h) */
};
template <typename T> static T *scal(mtb_ctx *c, Scal s) { return (T *)(c->d_scal + s); }
static hipError_t scal_clear(mtb_ctx *c, Scal first, uint32_t words = 1) { return hipMemsetAsync(c->d_scal + first, 0, 8 * (size_t)words, c->stream); }
/* The buffer table is touched only by ensure / ensure_placed / release / buf_get and by the whole-table walks, all under bufs_mu. */
static DevBuf buf_get(mtb_ctx *c, const std::string &name) { std::lock_guard<std::mutex> lk(c->bufs_mu); auto it = c->bufs.find(name); return it == c->bufs.end() ? DevBuf() : it->second; }
static size_t buf_cap(mtb_ctx *c, const char *name) { return buf_get(c, name).cap; }
/* workspace held: all of it (upto = BUF_FIXED), or only what grows with the sub-batch (upto = BUF_WORK) */
static size_t held_bytes(mtb_ctx *c, BufKind upto) { std::lock_guard<std::mutex> lk(c->bufs_mu); size_t b = 0; for (auto &kv : c->bufs) if (kv.second.kind == BUF_WORK || kv.second.kind == upto) b += kv.second.cap; return b; }
static void release_workspace(mtb_ctx *c) {
    std::lock_guard<std::mutex> lk(c->bufs_mu);
    for (auto &kv : c->bufs) if (kv.second.p && kv.second.kind != BUF_IO) { hipError_t e = hipFree(kv.second.p); (void)e; kv.second.p = nullptr; kv.second.cap = 0; }
    c->ws_per_base = 0.0; c->ws_max_sub_bases = 0;
    c->seg_clean_p = nullptr; c->seg_clean_cap = 0;       /* a later "segm" at the same address is not the buffer that was cleared */
}

/* RAII bracket around one kernel launch (only when profiling is on) */
struct KTimer {
    mtb_ctx *c; int id; hipEvent_t a = nullptr, b = nullptr;
    KTimer(mtb_ctx *c_, int id_) : c(c_), id(id_) {
        if (!c->profiling) return;
        a = take(); b = take();
        hipError_t e = hipEventRecord(a, c->stream); (void)e;
    }
    ~KTimer() {
        if (!c->profiling) return;
        hipError_t e = hipEventRecord(b, c->stream); (void)e;
        c->kev.push_back({id, a, b});
    }
    hipEvent_t take() {
        hipEvent_t ev;
        if (!c->ev_pool.empty()) { ev = c->ev_pool.back(); c->ev_pool.pop_back(); return ev; }
        hipError_t e = hipEventCreate(&ev); (void)e;
        return ev;
    }
};
static void collect_kernel_times(mtb_ctx *c) {
    for (auto &k : c->kev) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, k.a, k.b) == hipSuccess) { c->stats.ms_kernel[k.id] += ms; c->stats.n_launch[k.id]++; }
        c->ev_pool.push_back(k.a); c->ev_pool.push_back(k.b);
    }
    c->kev.clear();
}

struct mtb_index {
    mtb_ctx *ctx = nullptr;
    uint64_t T = 0;
    uint64_t *d_values = nullptr; uint32_t *d_info = nullptr; bool own = false;
    bool own_tax = true;             /* slices share the parent's device taxonomy */
    bool match_last = false;         /* partitions other than the last one match their final entry too */
    mtbhost::Taxonomy tax;
    int32_t *d_canon = nullptr, *d_parent = nullptr, *d_depth = nullptr, *d_spparent = nullptr, *d_tax2species = nullptr;
    uint8_t *d_under = nullptr, *d_accleaf = nullptr;
    mtb_tax_node *d_node = nullptr;
    mtb_params params;
    uint32_t info_mask = 0xFFFFFFFFu;
    /* amino-acid prefix directory (kernels_dir.h); absent for views and for indices it cannot describe */
    uint32_t *d_dir = nullptr; uint64_t *d_dirbase = nullptr; int32_t dir_L = 0; uint32_t dir_buckets = 0;
    bool packed = false;             /* d_values holds packed words (kernels_dir.h): the fused join's state; everything else unpacks first */
    bool info_owned = false;         /* d_info was (re)allocated by the library although the value array is borrowed (after mtb_index_seal) */
    /* The flat <-> packed conversion rewrites the target array in place and is not idempotent: it happens under `state_mu`, only
     * while no kernel that reads the array is in flight (`users` = join launches between acquire and the end of their stream
     * sync, whatever context or stream they run on), and is complete (stream-synchronised) before the lock is released. */
    std::mutex state_mu; std::condition_variable state_cv; int users = 0;
    int views = 0;                   /* live mtb_index_slice views: they read the parent's flat arrays, so the parent stays flat */
    mtb_index *parent = nullptr;     /* of a view */
    uint64_t open_chunks = 0, open_chunk_words = 0, open_peak_bytes = 0, open_free0 = 0;      /* mtb_index_open_stats */
    void *ipc_stage[4] = {nullptr, nullptr, nullptr, nullptr};       /* mtb_index_export: copies of the arrays too small for an inter-process handle of their own */
    bool is_part = false;            /* opened by mtb_index_open_part */
    /* k-mer coverage (mtb_index_coverage_begin .. _end): one bit per entry position; hits per species + MTB_COV_EXTRA words */
    uint32_t *d_cov_bits = nullptr; unsigned long long *d_cov_hits = nullptr;
};

enum ResKind { RES_ROWS = 0, RES_TAX = 1, RES_CNT = 2 };    /* the two device-side result sets of the asynchronous path: rows, packed taxID:count lists */
static const char *res_name(ResKind k, int set) { static const char *const names[2][3] = {{"results", "tctax2", "tccnt2"}, {"resultsb", "tctax2b", "tccnt2b"}}; return names[set ? 1 : 0][k]; }
template <typename T>
static mtb_status ensure(mtb_ctx *c, const char *name, size_t elems, T **out, BufKind kind = BUF_WORK) {
    if (c->down_pending) {
        /* asynchronous results (mtb_classify_batch_packed_async): whoever asks for a buffer that queued copies still read waits for them first
         * (the asynchronous path itself asks for the other set) */
        const int fl = c->res_set ^ 1;
        if (!strcmp(name, res_name(RES_ROWS, fl)) || !strcmp(name, res_name(RES_TAX, fl)) || !strcmp(name, res_name(RES_CNT, fl))) { HIPCHK(hipEventSynchronize(c->down_done)); c->down_pending = false; }
    }
    std::lock_guard<std::mutex> lk(c->bufs_mu);
    DevBuf &b = c->bufs.emplace(name, DevBuf{nullptr, 0, kind}).first->second;      /* what the entry is stays what its first request said */
    size_t bytes = elems * sizeof(T);
    if (bytes == 0) bytes = 64;
    if (b.cap < bytes) {
        if (b.p) { hipError_t e = hipFree(b.p); (void)e; b.p = nullptr; b.cap = 0; }
        size_t want = bytes + bytes / 16 + 256;
        size_t fr = 0, tot = 0;
        HIPCHK(hipMemGetInfo(&fr, &tot));
        if (want > fr) { want = bytes; if (want > fr) return fail(MTB_ERR_OOM, std::string("not enough HBM for buffer ") + name); }
        hipError_t e = hipMalloc(&b.p, want);
        if (e != hipSuccess) {
            b.p = nullptr;
            (void)hipGetLastError();          /* the failure is reported here: do not leave it in the runtime's sticky slot for the next hipGetLastError() check */
            return fail(MTB_ERR_OOM, std::string("hipMalloc failed for ") + name + ": " + hipGetErrorString(e));
        }
        b.cap = want;
#ifdef MTB_POISON_ALLOC     /* robustness build (make libmtb_xpoison.so X=-DMTB_POISON_ALLOC): no kernel may rely on fresh device memory being zero */
        HIPCHK(hipMemsetAsync(b.p, 0xA5, want, c->stream));         /* on the library's stream: it must not overtake or trail the kernels that use the buffer */
        HIPCHK(hipStreamSynchronize(c->stream));                    /* ... nor a copy that another stream (mtb_prefetch_batch_packed) is about to make into it */
#endif
    }
    *out = (T *)b.p;
    return MTB_OK;
}
/* a per-batch temporary that is written before it is read: out of the buffers the join left dead (first fit, 256-byte aligned), else a buffer of its own */
template <typename T>
static mtb_status scratch(mtb_ctx *c, const char *name, size_t elems, T **out) {
    const size_t bytes = (elems * sizeof(T) + 255) & ~(size_t)255;
    for (int i = 0; i < c->n_dead; i++) {
        mtb_ctx::DeadSeg &d = c->dead[i];
        if (d.cap - d.used >= bytes) { *out = (T *)(d.p + d.used); d.used += bytes; c->last_scratch_bytes += bytes; return MTB_OK; }
    }
    return ensure(c, name, elems, out);
}
/* Placement of the slot buffer.  The join's 1.1 G scattered 16-byte slot stores miss the L1 TLB once each, and what a miss costs
 * depends on where the 27 GB buffer landed: the same process runs the join at 47.5 or at 56.5 ms depending on nothing but a
 * re-allocation of this buffer (profiles/scripts/join_vs_placement.py; the other buffers do not matter).  So a new slot buffer is
 * chosen among a few candidate allocations by a probe that does what the join does to it -- random 16-byte non-temporal stores
 * over the whole buffer -- and the losers are handed back.  One-time cost per (re)allocation of a big buffer: 0.3 - 1 s per candidate
 * (hipMalloc of tens of GB), at most ~2.5 s; buffers below 8 GB (host batches of the stand-alone driver) are allocated as they come.
 * Measured over processes on one box: join 45 / 57 / 57 / 57 ms without, 42.5 - 47.6 with (profiles/r02_notes.md). */
__global__ __launch_bounds__(256) void k_probe_scatter(mtb_slot16 *buf, uint64_t n_slots, uint32_t per_thread, uint32_t seed) {
    uint64_t x = ((uint64_t)blockIdx.x * 256 + threadIdx.x) * 0x9E3779B97F4A7C15ull + seed;
    for (uint32_t j = 0; j < per_thread; j++) {
        x ^= x >> 29; x *= 0xBF58476D1CE4E5B9ull; x ^= x >> 32;
        mtb_slot16 *p = buf + (x % n_slots);
        __builtin_nontemporal_store((uint64_t)0, &p->a); __builtin_nontemporal_store((uint64_t)0, &p->b);      /* epoch 0 = not live */
    }
}
__global__ __launch_bounds__(256) void k_clear_words(uint64_t *p, uint64_t n_words) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n_words; i += (uint64_t)gridDim.x * 256) p[i] = 0;
    MTB_END_RELEASE();
}
static mtb_status ensure_placed(mtb_ctx *c, const char *name, size_t elems, mtb_slot16 **out) {
    std::unique_lock<std::mutex> lk(c->bufs_mu);     /* held while this function allocates the entry itself -- a probe's seconds included: a reservation thread waits in ensure() that long, once per big slot buffer, which is accepted; let go of before the plain path (ensure locks on its own) */
    DevBuf &b = c->bufs[name];
    auto plain = [&] { lk.unlock(); return ensure(c, name, elems, out); };
    const size_t bytes = std::max<size_t>(elems * sizeof(mtb_slot16), 64);
    /* experiment switch (tests/test_gpu_contig.py, profiles/r03_notes.md): the slot buffer -- of ANY size -- from physically
     * contiguous VRAM, the configuration in which round 2 saw pair scores differ from the oracle's */
    if (c->opt.segm_contig) {
        if (b.cap >= bytes) { *out = (mtb_slot16 *)b.p; return MTB_OK; }
        if (b.p) { hipError_t e = hipFree(b.p); (void)e; b.p = nullptr; b.cap = 0; }
        const size_t want = bytes + bytes / 16 + 256 + (c->opt.segm_pad ? (1u << 20) : 0);
        hipError_t e = hipExtMallocWithFlags(&b.p, want, hipDeviceMallocContiguous);
        if (e != hipSuccess) { b.p = nullptr; (void)hipGetLastError(); return fail(MTB_ERR_OOM, std::string("contiguous allocation failed for ") + name + ": " + hipGetErrorString(e)); }
        b.cap = want;
        *out = (mtb_slot16 *)b.p;
        return MTB_OK;
    }
    /* Off unless the caller asks for it (mtb_ctx_set_placement_probe, or MTB_PLACEMENT_PROBE=1): in a process whose only device
     * allocations are the library's own (the stand-alone driver) a plain hipMalloc lands as well as any candidate
     * (profiles/scripts/alloc_probe.hip, profiles/r03_notes.md section 3), and the search costs the first big batch 2.5 - 3.8 s
     * (profiles/r03_e2e_driver_30Mreads.txt).  A process with a long allocation history of its own (bench.py under torch's caching
     * allocator) turns it on. */
    const bool no_probe = c->opt.no_placement_probe != 0, env_probe = c->opt.placement_probe != 0;
    if (b.cap >= bytes || bytes < (8ull << 30) || no_probe || !(c->placement_probe || env_probe)) return plain();
    if (b.p) { hipError_t e = hipFree(b.p); (void)e; b.p = nullptr; b.cap = 0; }
    const size_t want = bytes + bytes / 16 + 256;
    const auto t_begin = std::chrono::steady_clock::now();
    struct Cand { void *p; float ms; size_t bytes; };
    std::vector<Cand> held;                 /* the best candidate so far + rejected ones kept allocated so that the next one lands elsewhere */
    std::vector<float> seen; std::vector<void *> seen_p, pads; std::vector<size_t> sizes;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    struct Guard {                          /* every early return (a failing HIP call below) hands the candidates, the pads and the events back */
        std::vector<Cand> &held; std::vector<void *> &pads; hipEvent_t &e0, &e1; bool armed = true;
        ~Guard() { if (!armed) return; for (auto &h : held) { hipError_t e = hipFree(h.p); (void)e; } for (void *q : pads) { hipError_t e = hipFree(q); (void)e; }
                   if (e0) { hipError_t e = hipEventDestroy(e0); (void)e; } if (e1) { hipError_t e = hipEventDestroy(e1); (void)e; } }
    } guard{held, pads, e0, e1};
    HIPCHK(hipEventCreate(&e0)); HIPCHK(hipEventCreate(&e1));
    for (int attempt = 0; attempt < 8; attempt++) {
        if (attempt >= 2 && std::chrono::duration<double>(std::chrono::steady_clock::now() - t_begin).count() > 2.0) break;      /* one-time cost, bounded */
        size_t fr = 0, tot = 0;
        HIPCHK(hipMemGetInfo(&fr, &tot));
        if (want + (attempt ? (8ull << 30) : 0) > fr) {                /* no room for another candidate next to the ones held: drop the worst rejected one */
            if (held.size() < 2) break;
            size_t worst = 0; for (size_t k = 1; k < held.size(); k++) if (held[k].ms > held[worst].ms) worst = k;
            { hipError_t e = hipFree(held[worst].p); (void)e; } held.erase(held.begin() + (long)worst);
            /* the hole just freed would be handed out again as it is: park a few GB in it first so that the next candidate is
             * composed differently (part of the hole, part of what else is free) */
            void *pad = nullptr;
            if (hipMalloc(&pad, ((size_t)(attempt % 3) + 1) * (3ull << 30)) == hipSuccess) pads.push_back(pad); else (void)hipGetLastError();
            HIPCHK(hipMemGetInfo(&fr, &tot));
            if (want + (4ull << 30) > fr) break;
        }
        void *p = nullptr;
        const size_t ask = want;        /* (a power-of-two request -- one buddy block, if the device still has one -- probed 0.60 - 0.79 ms: no better) */
        if (hipMalloc(&p, ask) != hipSuccess) { (void)hipGetLastError(); break; }
        sizes.push_back(ask);
        float best = 1e30f;
        for (int rep = 0; rep < 3; rep++) {                             /* first repetition = warm-up of the translations */
            HIPCHK(hipEventRecord(e0, c->stream));
            hipLaunchKernelGGL(k_probe_scatter, dim3(8192), dim3(256), 0, c->stream, (mtb_slot16 *)p, (uint64_t)(bytes / sizeof(mtb_slot16)), 8u, 12345u + (uint32_t)rep);
            HIPCHK(hipEventRecord(e1, c->stream));
            HIPCHK(hipEventSynchronize(e1));
            float ms = 0; HIPCHK(hipEventElapsedTime(&ms, e0, e1));
            if (rep && ms < best) best = ms;
        }
        held.push_back({p, best, ask}); seen.push_back(best); seen_p.push_back(p);
        /* after four candidates: two placements within 3 % of the fastest one seen = that is as good as it gets here, stop looking
         * (two alone can agree on a mediocre kind: 0.596 / 0.582 ms when 0.545 existed) */
        float lo = 1e30f; for (float v : seen) lo = std::min(lo, v);
        int near = 0; for (float v : seen) if (v <= lo * 1.03f) near++;
        float hi = 0.0f; for (float v : seen) hi = std::max(hi, v);
        if (seen.size() >= 4 && near >= 2 && lo <= 0.9f * hi) break;   /* ... and clearly better than the worst one seen */
    }
    guard.armed = false;
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    for (void *q : pads) { hipError_t e = hipFree(q); (void)e; }
    if (held.empty()) return plain();            /* not even one candidate fitted: the plain path reports the error */
    size_t pick = 0;
    for (size_t k = 1; k < held.size(); k++) if (held[k].ms < held[pick].ms) pick = k;
    for (size_t k = 0; k < held.size(); k++) if (k != pick) { hipError_t e = hipFree(held[k].p); (void)e; }
    std::vector<Cand> &cands = held;
    if (c->opt.placement_verbose) { fprintf(stderr, "mtb: slot buffer placement probe:"); for (size_t k = 0; k < seen.size(); k++) fprintf(stderr, " %.3f@%p", seen[k], seen_p[k]); fprintf(stderr, " ms -> %.3f (%.0f ms spent)\n", cands[pick].ms, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count()); }
    b.p = cands[pick].p; b.cap = cands[pick].bytes;
    *out = (mtb_slot16 *)b.p;
    return MTB_OK;
}
static void release(mtb_ctx *c, const char *name) {
    std::lock_guard<std::mutex> lk(c->bufs_mu);
    auto it = c->bufs.find(name);
    if (it != c->bufs.end()) { if (it->second.p) { hipError_t e = hipFree(it->second.p); (void)e; } c->bufs.erase(it); }
}

extern "C" {

const char *mtb_version(void) { return "metabuli_amd 0.1 (gfx950)"; }
const char *mtb_last_error(void) { return g_err.c_str(); }

void mtb_default_params(mtb_params *p) {   /* setClassifyDefaults, classify.cpp:10-37: kmerFormat 1 unless db.parameters says otherwise */
    p->seq_mode = 2; p->syncmer = 0; p->smer_len = 5; p->kmer_format = 1; p->min_cons_cnt = 4; p->min_cons_cnt_euk = 9;
    p->min_score = 0.0f; p->min_sp_score = 0.0f; p->tie_ratio = 0.95f; p->accession_level = 0; p->skip_redundancy = 0;
}

/* the side stream of the score stage and its events (mtb_ctx::side_stream); called right after the context's compute stream exists (a lane's: the two are
 * created one after the other; a caller's stream: whenever the caller made it).  Leaves nothing behind when it fails. */
static hipError_t make_side_stream(mtb_ctx *c) {
    hipError_t e = hipStreamCreateWithFlags(&c->side_stream, hipStreamNonBlocking);
    if (e != hipSuccess) { c->side_stream = nullptr; return e; }
    for (int k = 0; k < 3 && e == hipSuccess; k++) { e = hipEventCreateWithFlags(&c->side_ev[k], hipEventDisableTiming); if (e != hipSuccess) c->side_ev[k] = nullptr; }
    if (e != hipSuccess) {
        for (int k = 0; k < 3; k++) if (c->side_ev[k]) { hipError_t e2 = hipEventDestroy(c->side_ev[k]); (void)e2; c->side_ev[k] = nullptr; }
        hipError_t e2 = hipStreamDestroy(c->side_stream); (void)e2; c->side_stream = nullptr;
    }
    return e;
}
mtb_status mtb_ctx_create(int device, void *stream, mtb_ctx **out) {
    if (!out) return fail(MTB_ERR_ARG, "out is NULL");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) return fail(MTB_ERR_DEVICE, "no HIP device available (this library has no CPU path)");
    if (device < 0 || device >= n) return fail(MTB_ERR_ARG, "bad device ordinal");
    HIPCHK(hipSetDevice(device));
    mtb_ctx *c = new mtb_ctx();
    c->device = device; c->stream = (hipStream_t)stream;
    {   const hipError_t es = make_side_stream(c);          /* before anything else the context owns: a failure here leaves nothing to free but the object */
        if (es != hipSuccess) { delete c; return fail(MTB_ERR_DEVICE, std::string("side stream of the score stage: ") + hipGetErrorString(es)); } }
    mtb_build_tables(&c->h_tabs);
    HIPCHK(hipMalloc((void **)&c->d_tabs, sizeof(mtb_tables)));
    HIPCHK(hipMemcpy(c->d_tabs, &c->h_tabs, sizeof(mtb_tables), hipMemcpyHostToDevice));
    HIPCHK(hipMalloc((void **)&c->d_scal, SC_WORDS * sizeof(uint64_t)));
    HIPCHK(hipMalloc((void **)&c->d_ovfctr, MTB_OVF_STRIPES * 64));
    for (int i = 0; i < 8; i++) HIPCHK(hipEventCreate(&c->ev[i]));
    memset(&c->stats, 0, sizeof(c->stats));
    mtbopt::from_environment(&c->opt);                 /* the ONLY place the library reads its MTB_* switches from the environment */
    *out = c;
    return MTB_OK;
}
void mtb_ctx_destroy(mtb_ctx *c) {
    if (!c) return;
    for (mtb_ctx *l : c->lanes) mtb_ctx_destroy(l);
    c->lanes.clear();
    hipError_t e = hipSetDevice(c->device); (void)e;
    e = hipStreamSynchronize(c->stream);
    { std::lock_guard<std::mutex> lk(c->bufs_mu); for (auto &kv : c->bufs) if (kv.second.p) e = hipFree(kv.second.p); }
    if (c->d_tabs && !c->is_lane) e = hipFree(c->d_tabs);
    if (c->d_scal) e = hipFree(c->d_scal);
    if (c->d_ovfctr) e = hipFree(c->d_ovfctr);
    if (c->d_cov_pend && !c->is_lane) e = hipFree(c->d_cov_pend);
    if (c->is_lane && c->stream) e = hipStreamDestroy(c->stream);
    if (c->down_stream) { e = hipStreamSynchronize(c->down_stream); e = hipStreamDestroy(c->down_stream); }
    if (c->down_ready) e = hipEventDestroy(c->down_ready);
    if (c->down_done) e = hipEventDestroy(c->down_done);
    if (c->copy_stream) { e = hipStreamSynchronize(c->copy_stream); e = hipStreamDestroy(c->copy_stream); }
    if (c->side_stream) { e = hipStreamSynchronize(c->side_stream); e = hipStreamDestroy(c->side_stream); }
    for (int k = 0; k < 3; k++) if (c->side_ev[k]) e = hipEventDestroy(c->side_ev[k]);
    for (int k = 0; k < 2; k++) { if (c->copy_done[k]) e = hipEventDestroy(c->copy_done[k]); if (c->unpacked[k]) e = hipEventDestroy(c->unpacked[k]); }
    for (int q = 0; q < 4; q++) if (c->join_tunes[q].e0) { e = hipEventDestroy(c->join_tunes[q].e0); e = hipEventDestroy(c->join_tunes[q].e1); }
    for (int i = 0; i < 8; i++) e = hipEventDestroy(c->ev[i]);
    for (auto &k : c->kev) { e = hipEventDestroy(k.a); e = hipEventDestroy(k.b); }
    for (auto &x : c->ev_pool) e = hipEventDestroy(x);
    delete c;
}
mtb_status mtb_ctx_sync(mtb_ctx *c) { HIPCHK(hipStreamSynchronize(c->stream)); return MTB_OK; }
mtb_status mtb_ctx_set_profiling(mtb_ctx *c, int on) {
    if (!c) return fail(MTB_ERR_ARG, "NULL ctx");
    c->profiling = on;
    for (mtb_ctx *l : c->lanes) l->profiling = on;
    return MTB_OK;
}
mtb_status mtb_ctx_set_placement_probe(mtb_ctx *c, int on) {
    if (!c) return fail(MTB_ERR_ARG, "NULL ctx");
    c->placement_probe = on != 0;
    for (mtb_ctx *l : c->lanes) l->placement_probe = on != 0;
    return MTB_OK;
}
mtb_status mtb_ctx_set_workspace_limit(mtb_ctx *c, uint64_t bytes) {
    if (!c) return fail(MTB_ERR_ARG, "NULL ctx");
    c->ws_limit = bytes;
    for (mtb_ctx *l : c->lanes) l->ws_limit = bytes;
    return MTB_OK;
}
mtb_status mtb_ctx_set_option(mtb_ctx *c, const char *name, const char *value) {
    if (!c || !name) return fail(MTB_ERR_ARG, "NULL ctx / name");
    if (!mtbopt::set(&c->opt, name, value)) return fail(MTB_ERR_ARG, std::string("unknown switch or bad value: ") + name + "=" + (value ? value : "(unset)"));
    for (mtb_ctx *l : c->lanes) l->opt = c->opt;
    return MTB_OK;
}
mtb_status mtb_ctx_set_join_variant(mtb_ctx *c, int variant) {
    static const char *const names[] = {"auto", "q1w6", "q2w5", "window"};
    if (!c || variant < 0 || variant > 3) return fail(MTB_ERR_ARG, "variant must be MTB_JOIN_AUTO .. MTB_JOIN_WINDOW");
    return mtb_ctx_set_option(c, "MTB_JOIN_VARIANT", names[variant]);
}
uint32_t mtb_ctx_last_sub_batches(const mtb_ctx *c) { return c ? c->last_sub_batches : 0; }
uint64_t mtb_ctx_last_scratch_bytes(const mtb_ctx *c) { return c ? c->last_scratch_bytes : 0; }
mtb_status mtb_ctx_set_streams(mtb_ctx *c, int n) {
    if (!c || n < 1 || n > 8) return fail(MTB_ERR_ARG, "streams must be 1..8");
    HIPCHK(hipSetDevice(c->device));
    while ((int)c->lanes.size() > (n == 1 ? 0 : n)) { mtb_ctx_destroy(c->lanes.back()); c->lanes.pop_back(); }
    while (n > 1 && (int)c->lanes.size() < n) {
        mtb_ctx *l = new mtb_ctx();
        l->device = c->device; l->is_lane = true; l->d_tabs = c->d_tabs; l->h_tabs = c->h_tabs; l->profiling = c->profiling; l->placement_probe = c->placement_probe; l->opt = c->opt;
        HIPCHK(hipStreamCreateWithFlags(&l->stream, hipStreamNonBlocking));
        HIPCHK(make_side_stream(l));
        HIPCHK(hipMalloc((void **)&l->d_scal, SC_WORDS * sizeof(uint64_t)));
        HIPCHK(hipMalloc((void **)&l->d_ovfctr, MTB_OVF_STRIPES * 64));
        for (int i = 0; i < 8; i++) HIPCHK(hipEventCreate(&l->ev[i]));
        memset(&l->stats, 0, sizeof(l->stats));
        c->lanes.push_back(l);
    }
    return MTB_OK;
}

} // extern "C"

/* ------------------------------------------------------------------ */
/* internal device-side stages                                         */
/* ------------------------------------------------------------------ */
static mtb_status d2h(mtb_ctx *c, void *dst, const void *src, size_t bytes, hipStream_t st) {
    HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return MTB_OK;
}
static mtb_status d2h(mtb_ctx *c, void *dst, const void *src, size_t bytes) { return d2h(c, dst, src, bytes, c->stream); }
static mtb_status h2d(mtb_ctx *c, void *dst, const void *src, size_t bytes) {
    if (bytes == 0) return MTB_OK;
    HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return MTB_OK;
}

/* fused-path sort: first pass on the top letter pair, the two lower pairs bucket-local (kernels_sort.h); MTB_SORT_LSD=1: the three LSD passes of round 2 (A/B) */
static bool sort_msd_first(const mtb_ctx *c) { return !c->opt.sort_lsd; }

/* records the single-pass extractor's output buffer is sized for: six frames x L/3 windows bound the output by 2 metamers per base;
 * syncmer selection keeps about half of them, so the buffer follows the previous batch's yield (first batch of a context: < 1 metamer
 * per base with s = 5 -- 0.86 measured --, 2 in dense mode) and the extractor reports an overflow if that was too optimistic */
static uint64_t extract_bound(uint64_t n_bases, uint32_t grid) { return 2 * n_bases + (uint64_t)grid * MTB_EXTRACT_CHUNK; }      /* + at most one partly used chunk per wave */
static uint64_t extract_cap_guess(const mtb_ctx *c, const mtb_params *p, uint64_t n_bases, uint32_t grid) {
    const double guess = c->extract_yield > 0.0 ? c->extract_yield : (p->syncmer ? 1.0 : 2.0);
    return std::min<uint64_t>(extract_bound(n_bases, grid), (uint64_t)((double)n_bases * guess * 1.15) + 4096 + (uint64_t)grid * 64);
}

struct Reads {                            /* a batch, or a read range of one, on the device */
    const char *d_bases = nullptr; const uint64_t *d_offs = nullptr; const char *d_bases2 = nullptr; const uint64_t *d_offs2 = nullptr; uint64_t n_reads = 0;
    Reads range(uint64_t lo, uint64_t cnt) const { Reads r = *this; r.d_offs += lo; if (r.d_offs2) r.d_offs2 += lo; r.n_reads = cnt; return r; }
};
struct ReadLens { const int32_t *d_ql = nullptr, *d_ql2 = nullptr; uint32_t max_len = 0; };         /* per-read lengths as the extractor left them; the longest read */
struct ResultSink { mtb_result *d_res = nullptr; int32_t *d_tc_tax = nullptr; uint32_t *d_tc_cnt = nullptr; uint64_t tc_cap = 0, tc_base = 0; };     /* a read range's rows and taxID:count slots: capacity, first slot in the caller's arrays */
struct ExtractOpts {
    bool single_pass = false;             /* fused path: the arithmetic once, every wave reserves its output with an atomic (run order arbitrary, which the radix sort does not mind) */
    bool tag_ordinals = false, want_digits = false;       /* single pass: the metamer's ordinal in its read rides in qinfo (slot paths); the first radix pass's digits in buffer "digA" */
    bool want_max_len = true;             /* read the longest read's length back */
    uint32_t *d_counts = nullptr;         /* single pass: metamers per read (long-read slot path) */
    uint8_t *d_off_reads = nullptr;       /* tagged single pass: reads the slot records cannot hold are marked here */
};
struct Extracted {
    mtb_kmer *d_k = nullptr; uint64_t nk = 0, nk_real = 0;      /* buffer "kmersA"; records (the single pass counts its blank tail records too), metamers */
    uint32_t max_len = 0, max_q = 0;      /* longest read; single pass: most metamers of a read */
    uint16_t *d_dig = nullptr; uint64_t n_bases = 0;            /* single pass: bases of the read range, from its offsets */
    uint64_t off_max_q = 0, off_reads = 0, off_max_len = 0;     /* d_off_reads: most metamers of an unmarked read, marked reads, longest unmarked read */
};
/* extract.  Two passes (counts -> offsets -> emit) give the reference's emission order (stage API); the fused path asks for the single pass. */
static mtb_status dev_extract(mtb_ctx *c, const mtb_params *p, const Reads &rd, int32_t *d_qlen, int32_t *d_qlen2, const ExtractOpts &opt, Extracted *ex) {
    const uint64_t n_reads = rd.n_reads;
    if (n_reads >= (1ull << 29)) return fail(MTB_ERR_ARG, "more than 2^29-1 reads per batch (sequenceID is 29 bits, Kmer.h:13)");
    if (p->kmer_format != 1 && p->kmer_format != 2) return fail(MTB_ERR_UNSUPPORTED, "only kmer_format 1 and 2 are implemented");
    if (p->syncmer && (p->smer_len < 1 || p->smer_len > 8)) return fail(MTB_ERR_ARG, "smer_len out of range");
    *ex = Extracted();
    if (n_reads == 0) return MTB_OK;
    const bool single_pass = opt.single_pass;
    ExtractArgs a{rd.d_bases, rd.d_offs, rd.d_bases2, rd.d_offs2, n_reads, p->seq_mode, p->syncmer, p->smer_len, p->kmer_format, (single_pass && opt.tag_ordinals) ? 1 : 0, sort_msd_first(c) ? 54 : 34};
    /* grid sweep, 10 M reads: 7424 workgroups 23.5 ms, 16384 18.7, 65536 17.3, 262144 17.7 (and more blank tail records) */
    uint32_t grid = (uint32_t)std::min<uint64_t>(n_reads, 256ull * 256);
    HIPCHK(scal_clear(c, SC_MAX_LEN));
    uint64_t &n_bases = ex->n_bases;
    if (single_pass) {
        /* exact number of bases of this read range (what the caller knows may be an estimate) */
        uint64_t o[2];
        STCHK(d2h(c, &o[0], rd.d_offs, 8)); STCHK(d2h(c, &o[1], rd.d_offs + n_reads, 8));
        n_bases = o[1] - o[0];
        if (p->seq_mode == 2 && rd.d_offs2) { STCHK(d2h(c, &o[0], rd.d_offs2, 8)); STCHK(d2h(c, &o[1], rd.d_offs2 + n_reads, 8)); n_bases += o[1] - o[0]; }
    }
    if (single_pass && n_bases) {
        /* the buffer from the previous batch's yield (extract_cap_guess); the bound if that was too optimistic */
        const uint64_t bound = extract_bound(n_bases, grid);
        uint64_t cap = extract_cap_guess(c, p, n_bases, grid);
        cap = std::max<uint64_t>(cap, std::min<uint64_t>(bound, buf_cap(c, "kmersA") / sizeof(mtb_kmer)));
        for (int attempt = 0; attempt < 2; attempt++) {
            mtb_kmer *d_k; uint16_t *d_dig = nullptr;
            STCHK(ensure(c, "kmersA", cap, &d_k));
            if (opt.want_digits) { STCHK(ensure(c, "digA", cap + 8, &d_dig)); ex->d_dig = d_dig; }      /* (+8: the bucket-local histograms read whole 16-byte chunks) */
            HIPCHK(scal_clear(c, SC_EXTRACT, 8));
            if (opt.d_off_reads) HIPCHK(hipMemsetAsync(opt.d_off_reads, 0, n_reads, c->stream));
            { KTimer kt(c, MTB_K_EXTRACT_EMIT);
            hipLaunchKernelGGL((k_extract<2>), dim3(grid), dim3(64), 0, c->stream, a, c->d_tabs, opt.d_counts, (const uint64_t *)nullptr,
                               d_k, d_qlen, d_qlen2, scal<uint32_t>(c, SC_MAX_LEN), scal<unsigned long long>(c, SC_EXTRACT), cap, d_dig, opt.d_off_reads); }
            HIPCHK(hipGetLastError());
            ExtractCounters sc;
            STCHK(d2h(c, &sc, scal<uint64_t>(c, SC_EXTRACT), sizeof(sc)));
            ex->off_max_q = sc.off_max_q; ex->off_reads = sc.off_reads; ex->off_max_len = sc.off_max_len;
            if (opt.want_max_len) { uint64_t ml = 0; STCHK(d2h(c, &ml, scal<uint64_t>(c, SC_MAX_LEN), 8)); ex->max_len = (uint32_t)ml; }
            if (sc.overflow == 0) {
                if (sc.records >= (1ull << 32)) return fail(MTB_ERR_ARG, "more than 2^32-1 query metamers in one batch; split the batch");
                c->extract_yield = (double)sc.records / (double)n_bases;
                ex->d_k = d_k; ex->nk = sc.records; ex->nk_real = sc.real; ex->max_q = (uint32_t)sc.max_q;
                return MTB_OK;
            }
            if (cap >= bound) return fail(MTB_ERR_DEVICE, "extract: output bound exceeded");
            cap = bound;
        }
    }
    uint32_t *d_cnt; uint64_t *d_koff; uint64_t *d_ws;
    STCHK(ensure(c, "counts", n_reads, &d_cnt)); STCHK(ensure(c, "koff", n_reads + 1, &d_koff));
    STCHK(ensure(c, "scanws", scan_ws_elems(n_reads + 1), &d_ws));
    { KTimer kt(c, MTB_K_EXTRACT_COUNT);
    hipLaunchKernelGGL((k_extract<0>), dim3(grid), dim3(64), 0, c->stream, a, c->d_tabs, d_cnt, (const uint64_t *)nullptr,
                       (mtb_kmer *)nullptr, d_qlen, d_qlen2, scal<uint32_t>(c, SC_MAX_LEN), (unsigned long long *)nullptr, (uint64_t)0); }
    { KTimer kt(c, MTB_K_SCAN); scan_launch<uint32_t, uint64_t, false>(c->stream, d_cnt, n_reads, true, d_koff, d_ws); }
    uint64_t total = 0;
    STCHK(d2h(c, &total, d_koff + n_reads, 8));
    if (opt.want_max_len) { uint64_t ml = 0; STCHK(d2h(c, &ml, scal<uint64_t>(c, SC_MAX_LEN), 8)); ex->max_len = (uint32_t)ml; }
    if (total >= (1ull << 32)) return fail(MTB_ERR_ARG, "more than 2^32-1 query metamers in one batch; split the batch");
    mtb_kmer *d_k;
    STCHK(ensure(c, "kmersA", total, &d_k));
    if (total) { KTimer kt(c, MTB_K_EXTRACT_EMIT);
        hipLaunchKernelGGL((k_extract<1>), dim3(grid), dim3(64), 0, c->stream, a, c->d_tabs, (uint32_t *)nullptr,
                           (const uint64_t *)d_koff, d_k, (int32_t *)nullptr, (int32_t *)nullptr, (uint32_t *)nullptr,
                           (unsigned long long *)nullptr, (uint64_t)0); }
    HIPCHK(hipGetLastError());
    ex->d_k = d_k; ex->nk = ex->nk_real = total;
    return MTB_OK;
}

/* first_bit >= 0: binary LSD passes over bits [first_bit, 64).  first_bit == MTB_SORT_AA6 (kmer_format 2): three
 * passes on amino-acid letter pairs = order by bits [34, 64) (kernels_sort.h). */
#define MTB_SORT_AA6 (-6)
static mtb_status dev_sort(mtb_ctx *c, mtb_kmer *d_a, uint64_t n, int first_bit, mtb_kmer **sorted, uint16_t *d_dig, int aa_first_shift) {
    *sorted = d_a;
    if (n == 0) return MTB_OK;
    const bool aa = first_bit == MTB_SORT_AA6;
    const uint32_t bins = aa ? 512u : 256u;
    mtb_kmer *d_b; uint32_t *d_hist; uint64_t *d_ws;
    STCHK(ensure(c, "kmersB", n, &d_b));
    STCHK(ensure(c, "hist", radix_hist_elems(n, bins), &d_hist));
    STCHK(ensure(c, "scanws", scan_ws_elems(radix_hist_elems(n, bins)), &d_ws));
    {
        const int xcd_map = c->opt.sort_no_xcd ? 0 : 1;
        const uint32_t sc_threads = aa ? 512u : 256u;
        const uint64_t tile = (uint64_t)sc_threads * MTB_SORT_ITEMS;  /* MTB_SORT_ITEMS records per scatter thread */
        uint32_t tiles = (uint32_t)((n + tile - 1) / tile);
        mtb_kmer *src = d_a, *dst = d_b;
        /* AA6 with a digit side array: every histogram reads 2-byte digits (the extractor wrote the first pass's, each
         * scatter writes the next pass's in output order) instead of the 16-byte records */
        uint16_t *dig_src = aa ? d_dig : nullptr, *dig_dst = nullptr;
        if (dig_src) STCHK(ensure(c, "digB", n + 8, &dig_dst));
        /* the directory join (kernels_dir.h) looks every query up on its own: the sort only buys locality of the directory /
         * target accesses, so the fused path may stop after fewer letter pairs (aa_first_shift: 34 = six letters, 44 = four, 54 = two) */
        if (aa && dig_src && aa_first_shift == 34 && sort_msd_first(c)) {
            /* pass A: the top letter pair, over the whole list (its digits came with the records); passes B, C: the low and the middle
             * pair inside every bucket of pass A */
            uint32_t *d_plan;
            STCHK(ensure(c, "sortplan", 1026, &d_plan));
            const uint32_t seg_tiles_max = tiles + MTB_SORT_NBKT;
            STCHK(ensure(c, "hist", (uint64_t)bins * seg_tiles_max, &d_hist));
            STCHK(ensure(c, "scanws", scan_ws_elems((uint64_t)bins * seg_tiles_max), &d_ws));
            { KTimer kt(c, MTB_K_RADIX_HIST);
              hipLaunchKernelGGL((k_radix_hist_dig<512, 512>), dim3((tiles + MTB_HIST_GROUP - 1) / MTB_HIST_GROUP), dim3(512), 0, c->stream, (const uint16_t *)dig_src, n, d_hist, tiles); }
            { KTimer kt(c, MTB_K_SCAN); scan_launch<uint32_t, uint32_t, false>(c->stream, d_hist, (uint64_t)bins * tiles, false, d_hist, (uint32_t *)d_ws); }
            hipLaunchKernelGGL(k_sort_plan, dim3(1), dim3(512), 0, c->stream, (const uint32_t *)d_hist, tiles, n, (uint32_t)tile, d_plan);
            { KTimer kt(c, MTB_K_RADIX_SCATTER);
              hipLaunchKernelGGL((k_radix_scatter<512, 1, 512>), dim3((tiles + 7u) / 8u * 8u), dim3(512), 0, c->stream, (const mtb_kmer *)src, dst, n, 54, (const uint32_t *)d_hist, tiles, dig_dst, 34, xcd_map); }
            { mtb_kmer *tmp = src; src = dst; dst = tmp; uint16_t *t2 = dig_src; dig_src = dig_dst; dig_dst = t2; }
            for (int shift = 34; shift <= 44; shift += 10) {
                const dim3 hg((seg_tiles_max + MTB_HIST_GROUP - 1) / MTB_HIST_GROUP), sg((seg_tiles_max + 7u) / 8u * 8u);
                { KTimer kt(c, MTB_K_RADIX_HIST);
                  hipLaunchKernelGGL((k_radix_hist_seg<512, 512>), hg, dim3(512), 0, c->stream, (const uint16_t *)dig_src, (const uint32_t *)d_plan, d_hist); }
                /* (the table's length is on the device: the scan covers the most it can be; entries behind the last tile are never read) */
                { KTimer kt(c, MTB_K_SCAN); scan_launch<uint32_t, uint32_t, false>(c->stream, d_hist, (uint64_t)bins * seg_tiles_max, false, d_hist, (uint32_t *)d_ws); }
                { KTimer kt(c, MTB_K_RADIX_SCATTER);
                  hipLaunchKernelGGL((k_radix_scatter<512, 1, 512>), sg, dim3(512), 0, c->stream, (const mtb_kmer *)src, dst, n, shift, (const uint32_t *)d_hist, tiles,
                                     shift == 34 ? dig_dst : (uint16_t *)nullptr, 44, xcd_map, (const uint32_t *)d_plan); }
                { mtb_kmer *tmp = src; src = dst; dst = tmp; uint16_t *t2 = dig_src; dig_src = dig_dst; dig_dst = t2; }
            }
            *sorted = src;
            HIPCHK(hipGetLastError());
            return MTB_OK;
        }
        for (int shift = aa ? aa_first_shift : first_bit; shift < 64; shift += aa ? 10 : 8) {
            { KTimer kt(c, MTB_K_RADIX_HIST);
              const dim3 hg((tiles + MTB_HIST_GROUP - 1) / MTB_HIST_GROUP);
              if (aa && dig_src) hipLaunchKernelGGL((k_radix_hist_dig<512, 512>), hg, dim3(512), 0, c->stream, (const uint16_t *)dig_src, n, d_hist, tiles);
              else if (aa) hipLaunchKernelGGL((k_radix_hist<512, 1, 512>), dim3(tiles), dim3(512), 0, c->stream, (const mtb_kmer *)src, n, shift, d_hist, tiles);
              else hipLaunchKernelGGL((k_radix_hist<256, 0, 256>), dim3(tiles), dim3(256), 0, c->stream, (const mtb_kmer *)src, n, shift, d_hist, tiles); }
            { KTimer kt(c, MTB_K_SCAN); scan_launch<uint32_t, uint32_t, false>(c->stream, d_hist, (uint64_t)bins * tiles, false, d_hist, (uint32_t *)d_ws); }
            { KTimer kt(c, MTB_K_RADIX_SCATTER);
              const dim3 sg((tiles + 7u) / 8u * 8u);
              uint16_t *dnext = (dig_src && shift + 10 < 64) ? dig_dst : (uint16_t *)nullptr;
              if (aa) hipLaunchKernelGGL((k_radix_scatter<512, 1, 512>), sg, dim3(512), 0, c->stream, (const mtb_kmer *)src, dst, n, shift, (const uint32_t *)d_hist, tiles, dnext, shift + 10, xcd_map);
              else hipLaunchKernelGGL((k_radix_scatter<256, 0, 256>), sg, dim3(256), 0, c->stream, (const mtb_kmer *)src, dst, n, shift, (const uint32_t *)d_hist, tiles); }
            mtb_kmer *tmp = src; src = dst; dst = tmp;
            if (dig_src) { uint16_t *t2 = dig_src; dig_src = dig_dst; dig_dst = t2; }
        }
        *sorted = src;
    }
    HIPCHK(hipGetLastError());
    return MTB_OK;
}

struct IndexUse;
static mtb_dir_view dir_view(const mtb_index *ix);
static mtb_index_view index_view(const mtb_index *ix) {
    mtb_index_view v;
    v.values = ix->d_values; v.info = ix->d_info; v.n_targets = ix->T; v.tax2species = ix->d_tax2species;
    v.max_taxid = ix->tax.max_id; v.info_mask = ix->info_mask; v.kmer_format = ix->params.kmer_format;
    return v;
}
static mtb_tax_view tax_view(const mtb_index *ix) {
    mtb_tax_view v;
    v.acc_leaf = ix->d_accleaf; v.canon = ix->d_canon; v.parent = ix->d_parent; v.depth = ix->d_depth; v.under_euk = ix->d_under; v.sp_parent = ix->d_spparent;
    v.max_taxid = ix->tax.max_id;
    v.node = ix->d_node;
    return v;
}

static mtb_status ensure_flat_locked(mtb_index *ix) {       /* caller holds state_mu and has seen users == 0 */
    if (!ix || !ix->packed) return MTB_OK;
    mtb_ctx *c = ix->ctx;
    if (!ix->d_info) {                                  /* sealed: info[] was let go of; the flat state needs it back */
        hipError_t e = hipMalloc((void **)&ix->d_info, std::max<uint64_t>(ix->T, 1) * 4);
        if (e != hipSuccess) { ix->d_info = nullptr; (void)hipGetLastError(); return fail(MTB_ERR_OOM, "no HBM to restore info[] of a sealed index"); }
        ix->info_owned = true;
    }
    hipLaunchKernelGGL(k_index_unpack, dim3((uint32_t)std::min<uint64_t>(((uint64_t)ix->dir_buckets + 255) / 256, 1u << 20)), dim3(256), 0, c->stream, ix->d_values, ix->d_info, dir_view(ix));
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));
    ix->packed = false;
    return MTB_OK;
}
static bool can_pack(const mtb_index *ix) {
    return ix->d_dir && ix->dir_L == 7 && ix->own_tax && ix->views == 0 && !(ix->ctx && ix->ctx->opt.no_pack);
}
static mtb_status ensure_packed_locked(mtb_index *ix) {
    if (ix->packed || !can_pack(ix)) return MTB_OK;
    mtb_ctx *c = ix->ctx;
    hipLaunchKernelGGL(k_index_pack, dim3((uint32_t)std::min<uint64_t>((ix->T + 255) / 256, 1u << 20)), dim3(256), 0, c->stream, ix->d_values, (const uint32_t *)ix->d_info, ix->T, ix->params.kmer_format);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));            /* complete before any other stream's join may read the array */
    ix->packed = true;
    return MTB_OK;
}
/* A view's arrays are its parent's: the state (and the lock) live there. */
static mtb_index *state_owner(mtb_index *ix) { return ix && ix->parent ? ix->parent : ix; }
/* Exclusive change of state for the synchronous entry points (download, write, seal, slice): waits for the joins in flight. */
static mtb_status ensure_flat(mtb_index *ix) {
    mtb_index *o = state_owner(ix);
    if (!o) return MTB_OK;
    std::unique_lock<std::mutex> lk(o->state_mu);
    o->state_cv.wait(lk, [&] { return o->users == 0; });
    return ensure_flat_locked(o);
}
static mtb_status ensure_packed(mtb_index *ix) {
    mtb_index *o = state_owner(ix);
    std::unique_lock<std::mutex> lk(o->state_mu);
    o->state_cv.wait(lk, [&] { return o->users == 0; });
    return ensure_packed_locked(o);
}
/* A join's hold on the state it was launched for: taken before the launch, released after the launching stream has been
 * synchronised.  Several lanes (mtb_ctx_set_streams) or contexts may hold the same state at once; a lane that needs the other
 * state waits until the holders are gone, converts, and holds in turn. */
struct IndexUse {
    mtb_index *o = nullptr;
    mtb_status acquire(mtb_index *ix, bool want_packed) {
        mtb_index *own = state_owner(ix);
        std::unique_lock<std::mutex> lk(own->state_mu);
        const bool target = want_packed && can_pack(own);
        own->state_cv.wait(lk, [&] { return own->users == 0 || own->packed == target; });
        if (own->packed != target) { mtb_status st = target ? ensure_packed_locked(own) : ensure_flat_locked(own); if (st != MTB_OK) return st; }
        own->users++; o = own;
        return MTB_OK;
    }
    /* the state as it is, unconverted (coverage): *packed says which */
    void hold(mtb_index *ix, bool *packed) {
        mtb_index *own = state_owner(ix);
        std::unique_lock<std::mutex> lk(own->state_mu);
        own->users++; o = own; *packed = own->packed;
    }
    void release() { if (!o) return; { std::lock_guard<std::mutex> lk(o->state_mu); o->users--; } o->state_cv.notify_all(); o = nullptr; }
    ~IndexUse() { release(); }
};

struct MatchList { mtb_match *d_out = nullptr; uint64_t cap = 0; uint32_t *d_read_cnt = nullptr; };     /* the join's dense output: cap records, optionally the matches per read; MatchList() = none (slot segments) */
/* join into `list`; *count = matches found (may exceed list.cap -> MTB_ERR_CAPACITY).
 * With `seg` (per-read slot segments, k_join<SEG>) matches go to seg->seg and the overflow list instead; *count is then
 * the number of overflow entries needed and MTB_ERR_CAPACITY refers to the overflow list.  sort_low_bits: the bits the queries are NOT sorted on. */
static mtb_status dev_join(mtb_ctx *c, mtb_index *ix, const mtb_kmer *d_q, uint64_t n, const MatchList &list, uint64_t *count, const JoinSegArgs *seg, int sort_low_bits) {
    mtb_match *const d_out = list.d_out; const uint64_t cap = list.cap; uint32_t *const d_read_cnt = list.d_read_cnt;
    *count = 0;
    if (n == 0) return MTB_OK;
    HIPCHK(scal_clear(c, SC_JOIN_COUNT, 2));
    uint32_t grid = (uint32_t)((n + MTB_JOIN_QPB - 1) / MTB_JOIN_QPB);
    uint64_t *d_bounds;
    STCHK(ensure(c, "jbounds", 2ull * grid, &d_bounds));
    uint64_t limit = ix->T ? ix->T - (ix->match_last ? 0 : 1) : 0;          /* the last entry of the (whole) index is never a candidate */
    IndexUse use;                     /* released after the stream sync below (the d2h of the counters) */
    uint32_t win_tiles = 0;           /* the window variant ran: tiles launched (their statistics sit in SC_WIN_STATS) */
    const bool striped = seg && ix->d_dir && !seg->list && !seg->dense_ovf;       /* the slot modes of the directory join: striped overflow list */
    if (seg && ix->d_dir) {
        STCHK(use.acquire(ix, true));
        KTimer kt(c, MTB_K_JOIN);
        JoinSegArgs sa = *seg; sa.ovf_counter = scal<unsigned long long>(c, SC_JOIN_COUNT); sa.coop_min = c->opt.join_coop_min > 0 ? (uint32_t)c->opt.join_coop_min : (uint32_t)MTB_JOIN_COOP_MIN;
        if (striped) {
            HIPCHK(hipMemsetAsync(c->d_ovfctr, 0, MTB_OVF_STRIPES * 64, c->stream));
            sa.ovf_counter = c->d_ovfctr; sa.ovf_stripes = MTB_OVF_STRIPES; sa.ovf_region = sa.ovf_cap / MTB_OVF_STRIPES;
            c->ovf_region = sa.ovf_region;
        }
        const uint32_t g2 = (uint32_t)((n + 256 * MTB_JOIN_DIR_QPT - 1) / (256 * MTB_JOIN_DIR_QPT));
        if (sa.list) {      /* owner side of the partitioned index: a dense list of Match records */
            if (state_owner(ix)->packed) hipLaunchKernelGGL((k_join_dir<true, 2>), dim3(g2), dim3(256), 0, c->stream, d_q, n, index_view(ix), limit, dir_view(ix), (const mtb_tables *)c->d_tabs, sa, scal<uint32_t>(c, SC_JOIN_OVERFLOW));
            else hipLaunchKernelGGL((k_join_dir<false, 2>), dim3(g2), dim3(256), 0, c->stream, d_q, n, index_view(ix), limit, dir_view(ix), (const mtb_tables *)c->d_tabs, sa, scal<uint32_t>(c, SC_JOIN_OVERFLOW));
        } else
        if (sa.rb) {        /* long reads: per-read slot ranges */
            if (state_owner(ix)->packed) {
                /* one query per thread at 6 waves per SIMD here too (43.2 -> 41.5 ms per 50 k x 10 kb; MTB_JOIN_VARIANT=q2w5: round 4's instantiation, A/B) */
                /* the window form for long reads (round 6): the same tiles and windows, where the (sub-)batch is dense enough (100 k x 10 kb = 0.86 G metamers
                 * against 16 G targets: 18.6 targets per query) */
                const double per_q = (double)ix->T / (double)std::max<uint64_t>(n, 1);
                uint32_t qt = 256;                   /* full tiles: measured at 18.6 targets per query (200 k x 10 kb in two sub-batches): 256 queries per tile 124.3 ms, 175 (the density rule
                                                      * of the short reads) 127.0, 128: 143.5, sector-random q1w6 146.3 -- tiles beyond the capacity read global memory at eight waves per SIMD */
                if (c->opt.join_win_qt > 0) qt = (uint32_t)std::min(256, c->opt.join_win_qt);
                const bool sorted_ok = ix->params.kmer_format == 2 ? sort_low_bits == 34 : (sort_low_bits >= 24 && sort_low_bits <= 32);
                const bool lwin = sorted_ok && (c->opt.join_variant == 0x100 || c->opt.join_win == 1 || (c->opt.join_variant == 0 && c->opt.join_win < 0 && per_q <= MTB_LONG_WIN_MAX_PER_Q));
                if (lwin) {
                    const uint32_t n_tiles = (uint32_t)((n + qt - 1) / qt);
                    mtb_tile_win *d_tw;
                    STCHK(ensure(c, "jtilewin", (size_t)n_tiles, &d_tw));
                    HIPCHK(scal_clear(c, SC_WIN_STATS, 2));
                    hipLaunchKernelGGL(k_join_tile_win, dim3((n_tiles + 255) / 256), dim3(256), 0, c->stream, d_q, n, qt, dir_view(ix), limit, sort_low_bits, d_tw, n_tiles, scal<unsigned long long>(c, SC_WIN_STATS));
                    hipLaunchKernelGGL((k_join_dir<true, 1, 1, MTB_JOIN_WIN_WAVES, true>), dim3(n_tiles), dim3(256), 0, c->stream, d_q, n, index_view(ix), limit, dir_view(ix), (const mtb_tables *)c->d_tabs, sa,
                                       scal<uint32_t>(c, SC_JOIN_OVERFLOW), qt, (const mtb_tile_win *)d_tw, scal<unsigned long long>(c, SC_WIN_STATS));
                    win_tiles = n_tiles; c->stats.join_variant = MTB_JOIN_WINDOW;
                } else
                if (c->opt.join_variant != 0x25) hipLaunchKernelGGL((k_join_dir<true, 1, 1, 6>), dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, c->stream, d_q, n, index_view(ix), limit, dir_view(ix), (const mtb_tables *)c->d_tabs, sa, scal<uint32_t>(c, SC_JOIN_OVERFLOW));
                else hipLaunchKernelGGL((k_join_dir<true, 1, MTB_JOIN_DIR_QPT, 5>), dim3(g2), dim3(256), 0, c->stream, d_q, n, index_view(ix), limit, dir_view(ix), (const mtb_tables *)c->d_tabs, sa, scal<uint32_t>(c, SC_JOIN_OVERFLOW));
            }
            else hipLaunchKernelGGL((k_join_dir<false, 1>), dim3(g2), dim3(256), 0, c->stream, d_q, n, index_view(ix), limit, dir_view(ix), (const mtb_tables *)c->d_tabs, sa, scal<uint32_t>(c, SC_JOIN_OVERFLOW));
        } else
        if (state_owner(ix)->packed) {
            /* the product instantiation, or one of its A/B variants (queries per thread x waves per SIMD) */
#define MTB_LAUNCH_JV(QV, WV) hipLaunchKernelGGL((k_join_dir<true, 0, QV, WV>), dim3((uint32_t)((n + 256 * QV - 1) / (256 * QV))), dim3(256), 0, c->stream, d_q, n, index_view(ix), limit, dir_view(ix), (const mtb_tables *)c->d_tabs, sa, scal<uint32_t>(c, SC_JOIN_OVERFLOW))
            /* Three exact instantiations of the short-read join on packed words (kernels_dir.h): sector-random lookups with one query per thread at 6 waves
             * per SIMD (q1w6) or two at 5 (q2w5), and the LDS window.  The window needs a batch dense enough that a tile of sorted queries addresses a
             * span of the target array that fits LDS -- a query owns T / n targets on average; qt queries per workgroup so that the expected window is
             * ~0.82 of the capacity; below 240 queries per workgroup (T / n > 13.5: smaller batches against a big index) idle lanes cost more than the
             * window saves (r05_notes.md).  Which one is fastest depends on the batch's locality, which the host cannot see: reads of a few genomes at
             * high coverage run best with two queries per thread, a metagenome of thousands of genomes with one, a dense one with the window.  So a
             * context TRIES them on its first batches of a shape (second to fourth join: one instantiation each, timed with a pair of events) and
             * keeps the fastest; a few (index, batch size) shapes are remembered.  The caller can pin the choice (mtb_ctx_set_join_variant, or
             * MTB_JOIN_VARIANT / MTB_JOIN_WIN in the environment of mtb_ctx_create); the choice and the tuner's timings are reported in
             * mtb_batch_stats (join_variant, join_tuned, join_tune_ms). */
            const double per_q = (double)ix->T / (double)std::max<uint64_t>(n, 1);
            /* FULL tiles (256 queries) whatever the density: a tile whose span exceeds the window reads global memory at eight waves per SIMD, which beat smaller
             * tiles with idle lanes everywhere it was measured (2 M pairs, 31 targets per query: 256 per tile 32.4 ms, 105 per tile 38.5, q1w6 37.0; long reads:
             * 124.3 vs 127.0 at 175).  Beyond ~48 targets per query hardly a tile has a window (2 M held-out reads, 62 per query: 48.6 vs 47.1 for q1w6): the
             * window form is not a candidate there */
            uint32_t qt = 256;
            const bool win_ok = per_q <= 48.0;
            if (c->opt.join_win_qt > 0) qt = (uint32_t)std::min(256, c->opt.join_win_qt);
            qt = std::max<uint32_t>(qt, 1);
            int choice = -1;                                 /* 0: q1w6, 1: q2w5, 2: window, 3 / 4: the A/B-only instantiations q1w5 / q2w6 */
            int win_waves = MTB_JOIN_WIN_WAVES;              /* the window form's instantiation: waves per SIMD (5..7: A/B only) */
            switch (c->opt.join_variant) { case 0x16: choice = 0; break; case 0x25: choice = 1; break; case 0x100: choice = 2; break; case 0x15: choice = 3; break; case 0x26: choice = 4; break;
                                           case 0x205: case 0x206: case 0x207: choice = 2; win_waves = c->opt.join_variant & 15; break; default: break; }
            if (choice < 0 && c->opt.join_win >= 0) choice = c->opt.join_win ? 2 : 0;
            const bool forced = choice >= 0;
            uint32_t lg_n = 0; for (uint64_t x = n; x > 1; x >>= 1) lg_n++;
            const uint64_t tune_key = (uint64_t)(uintptr_t)ix ^ ((uint64_t)lg_n << 56) ^ (ix->T << 8);
            int slot = -1;
            for (int q = 0; q < 4; q++) if (c->join_tunes[q].key == tune_key) slot = q;
            mtb_ctx::JoinTune *jt = slot >= 0 ? &c->join_tunes[slot] : nullptr;
            bool timing_this = false; int tuned_flag = 0;
            if (!forced && !c->is_lane && !sa.retry) {
                if (!jt) { slot = (int)(c->join_tune_next++ & 3u); jt = &c->join_tunes[slot]; const hipEvent_t k0 = jt->e0, k1 = jt->e1; *jt = mtb_ctx::JoinTune(); jt->key = tune_key; jt->e0 = k0; jt->e1 = k1; }
                if (jt->pending >= 0) {                      /* the previous join's time (that batch is long finished) */
                    float ms = 0.0f;
                    if (hipEventElapsedTime(&ms, jt->e0, jt->e1) == hipSuccess && ms > 0.0f) jt->ms[jt->pending] = ms; else { (void)hipGetLastError(); jt->ms[jt->pending] = 1e30f; }
                    jt->pending = -1;
                }
                jt->calls++;
                if (jt->best < 0 && jt->calls >= 2) {
                    int next = -1;
                    for (int v = 0; v < 3; v++) if (jt->ms[v] == 0.0f && (v != 2 || win_ok)) { next = v; break; }
                    if (next >= 0) {
                        if (!jt->e0) { HIPCHK(hipEventCreate(&jt->e0)); HIPCHK(hipEventCreate(&jt->e1)); }
                        choice = next; jt->pending = next; timing_this = true;
                        HIPCHK(hipEventRecord(jt->e0, c->stream));
                    } else {
                        jt->best = 0;
                        for (int v = 1; v < 3; v++) if (jt->ms[v] > 0.0f && jt->ms[v] < jt->ms[jt->best]) jt->best = v;
                        if (c->opt.join_verbose) fprintf(stderr, "mtb: join tuned for this index and batch size: q1w6 %.2f ms, q2w5 %.2f ms, window %.2f ms -> %s\n", jt->ms[0], jt->ms[1], jt->ms[2],
                                                         jt->best == 0 ? "q1w6" : jt->best == 1 ? "q2w5" : "window");
                    }
                }
            }
            /* a remembered choice serves every batch of its log2-size bucket: the window only where THIS batch is dense enough for it;
             * retries of a batch (overflow list too small) and lanes never time anything, they follow what is known */
            if (choice < 0 && jt && jt->best >= 0) { choice = (jt->best == 2 && !win_ok) ? 0 : jt->best; tuned_flag = 1; }
            if (choice < 0) choice = win_ok ? 2 : 0;         /* not tuned (yet): by density */
            c->stats.join_variant = choice == 0 ? MTB_JOIN_Q1W6 : choice == 1 ? MTB_JOIN_Q2W5 : choice == 2 ? (win_waves != MTB_JOIN_WIN_WAVES ? -(10 + win_waves) : MTB_JOIN_WINDOW) : -choice;
            c->stats.join_tuned = tuned_flag;
            if (jt) for (int v = 0; v < 3; v++) c->stats.join_tune_ms[v] = jt->ms[v] < 1e29f ? jt->ms[v] : 0.0f;
            if (choice == 2) {
                /* the tiles' windows first (k_join_tile_win): needs the list sorted on the announced bits (else every tile reads global memory) */
                const uint32_t n_tiles = (uint32_t)((n + qt - 1) / qt);
                mtb_tile_win *d_tw;
                const bool sorted_ok = ix->params.kmer_format == 2 ? sort_low_bits == 34 : (sort_low_bits >= 24 && sort_low_bits <= 32);
                STCHK(ensure(c, "jtilewin", (size_t)n_tiles, &d_tw));
                HIPCHK(scal_clear(c, SC_WIN_STATS, 2));
                if (sorted_ok) hipLaunchKernelGGL(k_join_tile_win, dim3((n_tiles + 255) / 256), dim3(256), 0, c->stream, d_q, n, qt, dir_view(ix), limit, sort_low_bits, d_tw, n_tiles,
                                                  scal<unsigned long long>(c, SC_WIN_STATS));
                else HIPCHK(hipMemsetAsync(d_tw, 0, (size_t)n_tiles * sizeof(mtb_tile_win), c->stream));
#define MTB_LAUNCH_JW(WV) hipLaunchKernelGGL((k_join_dir<true, 0, 1, WV, true>), dim3(n_tiles), dim3(256), 0, c->stream, d_q, n, index_view(ix), limit, dir_view(ix), \
                                   (const mtb_tables *)c->d_tabs, sa, scal<uint32_t>(c, SC_JOIN_OVERFLOW), qt, (const mtb_tile_win *)d_tw, scal<unsigned long long>(c, SC_WIN_STATS))
                switch (win_waves) {
                case 5: MTB_LAUNCH_JW(5); break;
                case 6: MTB_LAUNCH_JW(6); break;
                case 7: MTB_LAUNCH_JW(7); break;
                default: MTB_LAUNCH_JW(MTB_JOIN_WIN_WAVES); break;
                }
#undef MTB_LAUNCH_JW
                win_tiles = n_tiles;
            } else
            switch (choice) {
            case 1: MTB_LAUNCH_JV(2, 5); break;
            case 3: MTB_LAUNCH_JV(1, 5); break;
            case 4: MTB_LAUNCH_JV(2, 6); break;
            default: MTB_LAUNCH_JV(1, 6); break;
            }
#undef MTB_LAUNCH_JV
            if (timing_this) HIPCHK(hipEventRecord(jt->e1, c->stream));
        }
        else hipLaunchKernelGGL((k_join_dir<false>), dim3(g2), dim3(256), 0, c->stream, d_q, n, index_view(ix), limit, dir_view(ix), (const mtb_tables *)c->d_tabs, sa, scal<uint32_t>(c, SC_JOIN_OVERFLOW));
    } else
    { STCHK(use.acquire(ix, false));
    KTimer kt(c, MTB_K_JOIN);
    hipLaunchKernelGGL(k_join_bounds, dim3((grid + 255) / 256), dim3(256), 0, c->stream, d_q, n, (const uint64_t *)ix->d_values, limit,
                       (uint64_t)grid, d_bounds, sort_low_bits);
    if (seg) {
        JoinSegArgs sa = *seg; sa.ovf_counter = scal<unsigned long long>(c, SC_JOIN_COUNT);
        hipLaunchKernelGGL((k_join<true>), dim3(grid), dim3(256), 0, c->stream, d_q, n, index_view(ix), (const mtb_tables *)c->d_tabs,
                           (const uint64_t *)d_bounds, (mtb_match *)nullptr, (uint64_t)0, (unsigned long long *)nullptr, (uint32_t *)nullptr,
                           scal<uint32_t>(c, SC_JOIN_OVERFLOW), sa);
    } else {
        JoinSegArgs sa; memset(&sa, 0, sizeof(sa));
        hipLaunchKernelGGL((k_join<false>), dim3(grid), dim3(256), 0, c->stream, d_q, n, index_view(ix), (const mtb_tables *)c->d_tabs,
                           (const uint64_t *)d_bounds, d_out, cap, scal<unsigned long long>(c, SC_JOIN_COUNT), d_read_cnt, scal<uint32_t>(c, SC_JOIN_OVERFLOW), sa);
    } }
    HIPCHK(hipGetLastError());
    uint64_t sc[2];
    STCHK(d2h(c, sc, scal<uint64_t>(c, SC_JOIN_COUNT), 16));
    if (win_tiles) {
        uint64_t ws[2];
        STCHK(d2h(c, ws, scal<uint64_t>(c, SC_WIN_STATS), 16));
        c->stats.join_tiles = win_tiles; c->stats.join_tiles_windowed = (uint32_t)ws[0]; c->stats.join_tiles_outside = (uint32_t)ws[1];
    }
    if (striped) {
        /* entries per stripe: the list fits when the fullest region does; else the caller comes again with room for 256 x that */
        unsigned long long h[MTB_OVF_STRIPES * 8];
        STCHK(d2h(c, h, c->d_ovfctr, sizeof(h)));
        uint64_t tot = 0, mx = 0;
        for (uint32_t k = 0; k < MTB_OVF_STRIPES; k++) { tot += h[8 * k]; mx = std::max<uint64_t>(mx, h[8 * k]); }
        c->ovf_max_region = mx;
        if (seg->rb) {                                 /* long reads: counted only */
            *count = tot;
            if (tot > seg->ovf_cap) return fail(MTB_ERR_CAPACITY, "match buffer too small");
            return MTB_OK;
        }
        *count = mx > c->ovf_region ? (mx + mx / 8 + 64) * MTB_OVF_STRIPES : tot;          /* (>= tot: also enough for a dense list) */
        if (tot >= (1ull << 32)) return fail(MTB_ERR_ARG, "more than 2^32-1 matches in one batch; split the batch");
        if (mx > c->ovf_region) return fail(MTB_ERR_CAPACITY, "match buffer too small");
        return MTB_OK;
    }
    c->ovf_region = 0;
    *count = sc[0];
    if (sc[0] >= (1ull << 32)) return fail(MTB_ERR_ARG, "more than 2^32-1 matches in one batch; split the batch");
    if (sc[0] > (seg ? seg->ovf_cap : cap)) return fail(MTB_ERR_CAPACITY, "match buffer too small");
    return MTB_OK;
}

/* per-read counters -> seg_start (n_reads+1) -> regroup into d_out */
template <typename REC>
static mtb_status dev_regroup(mtb_ctx *c, const mtb_match *d_in, uint64_t m, uint64_t n_reads, uint32_t *d_read_cnt,
                              uint64_t **seg_start, REC *d_out) {
    uint64_t *d_seg; uint64_t *d_ws; uint32_t *d_cur;
    STCHK(ensure(c, "segstart", n_reads + 1, &d_seg));
    STCHK(ensure(c, "scanws", scan_ws_elems(n_reads + 1), &d_ws));
    STCHK(ensure(c, "cursor", n_reads, &d_cur));
    { KTimer kt(c, MTB_K_SCAN); scan_launch<uint32_t, uint64_t, false>(c->stream, d_read_cnt, n_reads, true, d_seg, d_ws); }
    HIPCHK(hipMemsetAsync(d_cur, 0, n_reads * 4, c->stream));
    if (m) { KTimer kt(c, MTB_K_REGROUP); hipLaunchKernelGGL((k_regroup<REC>), dim3((uint32_t)((m + 255) / 256)), dim3(256), 0, c->stream, d_in, m, (const uint64_t *)d_seg, d_cur, d_out); }
    HIPCHK(hipGetLastError());
    *seg_start = d_seg;
    return MTB_OK;
}

static mtb_status dev_segsort(mtb_ctx *c, mtb_match *d_m, const uint64_t *d_seg, uint64_t n_reads, uint32_t *max_seg) {
    uint32_t *d_large;
    STCHK(ensure(c, "large", n_reads, &d_large));
    HIPCHK(scal_clear(c, SC_N_LARGE, 2));
    uint32_t grid = (uint32_t)std::min<uint64_t>(n_reads, 256ull * 40);
    { KTimer kt(c, MTB_K_SEGSORT);
    hipLaunchKernelGGL(k_segsort_small, dim3(grid), dim3(64), 0, c->stream, d_m, d_seg, n_reads, d_large, scal<uint32_t>(c, SC_N_LARGE),
                       scal<uint32_t>(c, SC_MAX_SEG)); }
    hipLaunchKernelGGL((k_segsort_large<mtb_match>), dim3(1024), dim3(256), 0, c->stream, d_m, d_seg, (const uint32_t *)d_large,
                       scal<const uint32_t>(c, SC_N_LARGE));
    HIPCHK(hipGetLastError());
    if (max_seg) { uint64_t sc[2]; STCHK(d2h(c, sc, scal<uint64_t>(c, SC_N_LARGE), 16)); *max_seg = (uint32_t)sc[1]; }
    return MTB_OK;
}

/* where a scoring launch finds its segments */
struct ScoreSrc {
    const mtb_match *m = nullptr;
    const uint64_t *seg = nullptr;        /* seg_start (by read, or by list slot if seg_by_list)            */
    const uint32_t *cursor = nullptr;     /* slot mode (k_join<SEG>): read r owns m[r*stride .. +stride), cursor[r] = entries in its tail */
    uint32_t stride = 0, direct = 0, epoch = 0;
    uint32_t *big_list = nullptr, *n_big = nullptr;      /* slot mode: reads deferred to the large-segment path */
    uint32_t *cnt_out = nullptr;                         /* slot mode: live records per read */
    uint32_t cap = MTB_SCORE_LDS;                        /* matches staged in LDS per read: 160, or 320 (read pairs on the slot path) */
    const uint32_t *list = nullptr, *n_list = nullptr;   /* only these reads */
    int seg_by_list = 0;
    bool sort = false;                    /* segments arrive unordered: rank sort in the kernel */
    uint32_t max_seg = 0;                 /* largest segment this launch can meet */
    uint32_t max_len_deferred = 0;        /* the launch over the reads this one defers may meet longer reads than lens.max_len (reads routed around the slot segments) */
    uint32_t grid = 0;                    /* 0 = default */
    const uint8_t *only_flagged = nullptr; /* slot mode after k_score_fast: score only the reads it flagged */
    const uint32_t *seg_cnt = nullptr;     /* slab launches: matches per read when the segment does not fill [seg[r], seg[r + 1]) */
    const void *bound_by_buckets = nullptr; /* non-NULL: every read gets one taxcnt slot per position bucket (its match count is not in seg[]) */
    bool overflowed_listed = false;         /* slot mode: the caller lists the reads k_score_fast flags 2 itself (k_list_overflowed); big_list takes only what the generic kernel defers */
};

/* d_results/d_tc_* are device outputs; *n_tc = sum of per-read bounds.  `second` (optional) runs after the launch
 * over `first`, may build a source for the reads that launch deferred (large-segment path) and returns true to
 * have it launched with the same per-read taxcnt slots. */
struct ScoreLaunch { const uint64_t *d_tcoff; bool key64; mtb_score_params sp; ReadLens lens; ResultSink out; };     /* what dev_score has set up by the time `second` runs: enough to launch a scorer of its own */
typedef std::function<mtb_status(ScoreSrc *, bool *, const ScoreLaunch &)> ScoreSecond;
typedef std::function<mtb_status(const ScoreLaunch &)> ScoreFork;       /* optional: runs once the taxcnt layout exists, before the first scorer is launched (score_fixed_slots starts its deferred tier there) */
/* dev_score takes a slot batch's reads through the register-resident scorer first */
static bool fast_scorer_applies(const mtb_ctx *c, const mtb_index *ix, const mtb_params *p, const ReadLens &lens, uint32_t stride) {
    const bool key64 = ix->tax.max_id < (1 << 22) && lens.max_len + 3 < (1u << 11);
    return key64 && stride <= 384u && !c->opt.no_fast_scorer && !(p->seq_mode == 2 && c->opt.no_fast_pairs);
}
/* per-read bounds of the taxcnt slots (k_taxcnt_bound over seg / cnt) -> d_tcoff (n_reads + 1); *n_tc = their sum, checked against the sink */
static mtb_status taxcnt_layout(mtb_ctx *c, uint64_t n_reads, const uint64_t *d_seg, const uint32_t *d_cnt, const ReadLens &lens, const ResultSink &out, int dna_shift, uint64_t *d_tcoff, uint64_t *n_tc) {
    uint32_t *d_bound; uint64_t *d_ws;
    STCHK(ensure(c, "bound", n_reads, &d_bound)); STCHK(ensure(c, "scanws", scan_ws_elems(n_reads + 1), &d_ws));
    hipLaunchKernelGGL(k_taxcnt_bound, dim3((uint32_t)((n_reads + 63) / 64)), dim3(64), 0, c->stream, d_seg, d_cnt, lens.d_ql, lens.d_ql2, n_reads, dna_shift, d_bound);
    { KTimer kt(c, MTB_K_SCAN); scan_launch<uint32_t, uint64_t, false>(c->stream, d_bound, n_reads, true, d_tcoff, d_ws); }
    STCHK(d2h(c, n_tc, d_tcoff + n_reads, 8));
    if (*n_tc > out.tc_cap) return fail(MTB_ERR_CAPACITY, "taxcnt buffers too small");
    if (out.tc_base + *n_tc >= (1ull << 32)) return fail(MTB_ERR_ARG, "more than 2^32-1 taxcnt slots in one batch (mtb_result.taxcnt_off is 32 bits); split the batch");
    return MTB_OK;
}
static mtb_status dev_score(mtb_ctx *c, mtb_index *ix, const mtb_params *p, uint64_t n_reads, const ReadLens &lens, const ResultSink &out, uint64_t *n_tc,
                            const ScoreSrc &first, const ScoreSecond *second, const ScoreFork *fork = nullptr) {
    mtb_score_params sp; mtb_make_score_params(p, &sp);
    uint64_t *d_tcoff;
    STCHK(ensure(c, "tcoff", n_reads + 1, &d_tcoff));
    STCHK(taxcnt_layout(c, n_reads, first.seg, first.cursor ? first.cursor : (const uint32_t *)first.bound_by_buckets, lens, out, sp.dna_shift, d_tcoff, n_tc));
    /* single-word sort key when taxids < 2^22 and positions < 2^11 (hamming of a match is <= 7) */
    const bool key64 = ix->tax.max_id < (1 << 22) && lens.max_len + 3 < (1u << 11);
    const uint32_t max_nb_first = (uint32_t)mtb_num_buckets((int32_t)lens.max_len, sp.dna_shift);
    const uint32_t max_nb_second = (uint32_t)mtb_num_buckets((int32_t)std::max(lens.max_len, first.max_len_deferred), sp.dna_shift);
    if (max_nb_second > 65535u) return fail(MTB_ERR_ARG, "read too long for mtb_result.n_taxcnt (16 bits): more than 65535 position buckets");
    if (fork) {
        /* what the launches below ask for is asked for before the fork where it is known by now: an allocation synchronises the device, and the
         * batch that grows a buffer behind the fork runs its tier after k_score_fast instead of beside it.  Left behind the fork: the slab pool of
         * a batch with more than MTB_SCORE_BKT position buckets (reads beyond ~1100 bases among short ones; BUF_FIXED, it grows once per context). */
        uint8_t *d_slow_early;
        if (first.cursor && fast_scorer_applies(c, ix, p, lens, first.stride)) STCHK(ensure(c, "slowflag", n_reads, &d_slow_early));
        STCHK((*fork)(ScoreLaunch{d_tcoff, key64, sp, lens, out}));
    }
    ScoreSrc second_src;
    for (int pass = 0; pass < 2; pass++) {
        const uint32_t max_nb = pass ? max_nb_second : max_nb_first;
        const ScoreSrc *S = &first;
        if (pass == 1) {
            if (!second) break;
            bool go = false;
            const ScoreLaunch SL{d_tcoff, key64, sp, lens, out};
            STCHK((*second)(&second_src, &go, SL));
            if (!go) break;
            S = &second_src;
        }
        /* many more workgroups than resident slots (14 single-wave workgroups per CU): reads differ a lot in cost, and ~8 reads
         * per workgroup balanced best (10 M reads: 3584 workgroups 66.6 ms, 57 k 60.2, 1 M 59.1, 2.5 M 60.4, 10 M 66.8) */
        uint32_t grid = S->grid ? S->grid : (uint32_t)std::min<uint64_t>(n_reads, std::max<uint64_t>(256ull * 14, n_reads / 8));
        /* reads with a big segment OR many position buckets are scored entirely out of a slab */
        bool need_slab = S->max_seg > S->cap || max_nb > MTB_SCORE_BKT;
        uint32_t slab_n = need_slab ? std::max<uint32_t>(S->max_seg, 1) : 0;
        uint32_t slab_nb = need_slab ? max_nb : 0;
        uint64_t slab_bytes = need_slab ? score_slab_bytes(slab_n, slab_nb) : 0;
        uint8_t *d_slabs = nullptr;
        const bool dynamic = need_slab && !S->cursor;       /* slab launches claim reads from a counter: the grid is what is resident */
        if (dynamic) grid = std::min<uint32_t>(grid, 256u * 14u);
        if (slab_bytes) {
            while ((uint64_t)grid * slab_bytes > (MTB_SLAB_POOL_MAX) && grid > 64) grid /= 2;     /* keep the slab pool bounded (a halved grid halves the waves that hide the slab's HBM latency) */
            STCHK(ensure(c, "slabs", (size_t)grid * slab_bytes, &d_slabs, BUF_FIXED));
        }
        unsigned long long *d_work = nullptr;
        if (dynamic) { d_work = scal<unsigned long long>(c, SC_SCORE_WORK) + pass; HIPCHK(hipMemsetAsync(d_work, 0, 8, c->stream)); }
#define MTB_LAUNCH_SCORE(SRT, K, CAPV, DYNV, SLOTV) hipLaunchKernelGGL((k_score<SRT, K, mtb_match, CAPV, DYNV, SLOTV>), dim3(grid), dim3(64), 0, c->stream, S->m, S->seg, n_reads, lens.d_ql, \
        lens.d_ql2, tax_view(ix), sp, (const uint64_t *)d_tcoff, out.d_res, out.d_tc_tax, out.d_tc_cnt, out.tc_cap, d_slabs, slab_bytes, slab_n, slab_nb, (mtb_match *)nullptr,  \
        out.tc_base, S->list, S->n_list, S->cursor, S->stride, S->seg_by_list, S->direct, S->epoch, S->big_list, S->n_big, S->cnt_out, d_work, S->only_flagged, S->seg_cnt)
        ScoreSrc S_rest;
        const bool pairs = p->seq_mode == 2;
        if (S->cursor && pass == 0 && fast_scorer_applies(c, ix, p, lens, S->stride)) {
            /* slot mode: the register-resident scorer takes every read with the common structure (slots in compareMatches order
             * once the species -- for pairs the (species, frame) runs -- are laid one after another, one match per position
             * group) and lists the others for the generic kernel below */
            uint8_t *d_slow;
            STCHK(ensure(c, "slowflag", n_reads, &d_slow));
            HIPCHK(hipMemsetAsync(d_slow, 0, n_reads, c->stream));
            HIPCHK(scal_clear(c, SC_N_GENERIC));
#define MTB_LAUNCH_FAST(...) hipLaunchKernelGGL((k_score_fast<__VA_ARGS__>), dim3(grid), dim3(64), 0, c->stream, (const mtb_slot16 *)S->m, n_reads, lens.d_ql, lens.d_ql2, tax_view(ix), sp, \
            (const uint64_t *)d_tcoff, out.d_res, out.d_tc_tax, out.d_tc_cnt, out.tc_cap, out.tc_base, S->cursor, S->stride, S->direct, S->epoch, d_slow, S->cnt_out)
            { KTimer ktf(c, MTB_K_SCORE_FAST);
              if (pairs) { if (S->stride <= 192) MTB_LAUNCH_FAST(3, 3, true); else if (S->stride <= 256) MTB_LAUNCH_FAST(4, 4, true); else MTB_LAUNCH_FAST(5, 6, true); }
              else if (S->stride <= 128) MTB_LAUNCH_FAST(2); else if (S->stride <= 192) MTB_LAUNCH_FAST(3); else if (S->stride <= 256) MTB_LAUNCH_FAST(4); else MTB_LAUNCH_FAST(5, 6, false); }
#undef MTB_LAUNCH_FAST
            hipLaunchKernelGGL(k_count_flags, dim3(256), dim3(256), 0, c->stream, (const uint8_t *)d_slow, n_reads, scal<unsigned long long>(c, SC_N_GENERIC));
            if (S->big_list && S->n_big && !S->overflowed_listed) hipLaunchKernelGGL(k_list_flag2, dim3((uint32_t)((n_reads + 255) / 256)), dim3(256), 0, c->stream, (const uint8_t *)d_slow, n_reads, S->big_list, S->n_big);
            c->fast_used = true;
            S_rest = *S; S_rest.only_flagged = d_slow;
            S = &S_rest;
        }
        KTimer kt(c, pass == 0 ? MTB_K_SCORE : MTB_K_SEGSORT);      /* the deferred reads' launch is booked with the large-segment path */
        if (S->cursor) {              /* slot mode (always sorts in the kernel); LDS staging capacity chosen by the caller */
#define MTB_LAUNCH_SLOT(CAPV) do { if (key64) MTB_LAUNCH_SCORE(true, true, CAPV, false, true); else MTB_LAUNCH_SCORE(true, false, CAPV, false, true); } while (0)
            if (S->cap <= 144) MTB_LAUNCH_SLOT(144);
            else if (S->cap <= 160) MTB_LAUNCH_SLOT(160);
            else if (S->cap <= 224) MTB_LAUNCH_SLOT(224);
            else if (S->cap <= 288) MTB_LAUNCH_SLOT(288);
            else MTB_LAUNCH_SLOT(320);
#undef MTB_LAUNCH_SLOT
        } else if (dynamic) {
            if (!S->sort) MTB_LAUNCH_SCORE(false, false, MTB_SCORE_LDS, true, false);
            else if (key64) MTB_LAUNCH_SCORE(true, true, MTB_SCORE_LDS, true, false); else MTB_LAUNCH_SCORE(true, false, MTB_SCORE_LDS, true, false);
        }
        else if (S->sort) { if (key64) MTB_LAUNCH_SCORE(true, true, MTB_SCORE_LDS, false, false); else MTB_LAUNCH_SCORE(true, false, MTB_SCORE_LDS, false, false); }
        else if (S->cap >= 320) MTB_LAUNCH_SCORE(false, false, 320, false, false);      /* the deferred reads of a slot batch: a few hundred matches each stay in LDS, only the rest works out of slabs */
        else MTB_LAUNCH_SCORE(false, false, MTB_SCORE_LDS, false, false);
#undef MTB_LAUNCH_SCORE
    }
    HIPCHK(hipGetLastError());
    return MTB_OK;
}

struct LongSegs {                         /* the sorted exact segments k_score_long streams */
    const mtb_match *d_m = nullptr; const uint64_t *d_seg = nullptr; uint32_t max_seg = 0;
    const uint32_t *d_segcnt = nullptr, *d_list = nullptr; uint32_t n_list = 0;      /* matches per read when a segment does not fill [seg[r], seg[r + 1]) (slot ranges); only these reads: segments indexed by the list slot, taxcnt slots as laid out by a previous call */
};
/* Long reads (seq_mode 3): exact segments in compareMatches order -> k_score_long, one workgroup per read (kernels_score_long.h).
 * Reads it cannot take (LDS budgets) are flagged and scored by the generic slab launch of dev_score afterwards. */
static mtb_status dev_score_long(mtb_ctx *c, mtb_index *ix, const mtb_params *p, uint64_t n_reads, const ReadLens &lens, const ResultSink &out, uint64_t *n_tc, const LongSegs &sg) {
    mtb_score_params sp; mtb_make_score_params(p, &sp);
    uint64_t *d_tcoff; uint8_t *d_todo;
    STCHK(ensure(c, "tcoff", n_reads + 1, &d_tcoff)); STCHK(ensure(c, "slowflag", n_reads, &d_todo));
    if (!sg.d_list) {
        /* per-read taxcnt slots: one per position bucket (slot ranges: the match count is not known yet), else min(matches, buckets) */
        STCHK(taxcnt_layout(c, n_reads, sg.d_seg, sg.d_segcnt, lens, out, sp.dna_shift, d_tcoff, n_tc));
        const uint32_t max_nb = (uint32_t)mtb_num_buckets((int32_t)lens.max_len, sp.dna_shift);
        if (max_nb > 65535u) return fail(MTB_ERR_ARG, "read too long for mtb_result.n_taxcnt (16 bits): more than 65535 position buckets");
    }
    HIPCHK(hipMemsetAsync(d_todo, 0, n_reads, c->stream));
    unsigned long long *d_work = scal<unsigned long long>(c, SC_LONG_WORK);
    HIPCHK(hipMemsetAsync(d_work, 0, 8, c->stream));
    HIPCHK(scal_clear(c, SC_LONG_N_SECOND));
    {   KTimer kt(c, MTB_K_SCORE_FAST);       /* booked with the register-resident scorer's id: the workgroup-per-read kernel of long reads */
        /* two launches (round 6): <.., 512 paths, 2048 position buckets> first -- 33 KB of LDS, four workgroups per CU; reads up to ~18 kb with up to 512 emitted
         * paths: nearly all -- then the full budgets (70 KB, two per CU) for the reads the first one flagged */
        const uint64_t n_it = sg.d_list ? sg.n_list : n_reads;
        hipLaunchKernelGGL((k_score_long<MTB_LONG_MAXBLK, MTB_LONG_MAXSP, 512, 2048>), dim3((uint32_t)std::min<uint64_t>(n_it, 256ull * 4)), dim3(MTB_LONG_NT), 0, c->stream, sg.d_m, sg.d_seg, n_reads, lens.d_ql, lens.d_ql2, tax_view(ix), sp, (const uint64_t *)d_tcoff,
                           out.d_res, out.d_tc_tax, out.d_tc_cnt, out.tc_cap, out.tc_base, d_todo, d_work, sg.d_segcnt, sg.d_list, sg.n_list, 0u);
        hipLaunchKernelGGL(k_count_flags, dim3(256), dim3(256), 0, c->stream, (const uint8_t *)d_todo, n_reads, scal<unsigned long long>(c, SC_LONG_N_SECOND));
        uint64_t n_second = 0;
        STCHK(d2h(c, &n_second, scal<uint64_t>(c, SC_LONG_N_SECOND), 8));
        HIPCHK(scal_clear(c, SC_N_GENERIC));
        if (n_second) {
            HIPCHK(hipMemsetAsync(d_work, 0, 8, c->stream));
            hipLaunchKernelGGL((k_score_long<MTB_LONG_MAXBLK, MTB_LONG_MAXSP>), dim3((uint32_t)std::min<uint64_t>(n_it, 256ull * 2)), dim3(MTB_LONG_NT), 0, c->stream, sg.d_m, sg.d_seg, n_reads, lens.d_ql, lens.d_ql2, tax_view(ix), sp, (const uint64_t *)d_tcoff,
                               out.d_res, out.d_tc_tax, out.d_tc_cnt, out.tc_cap, out.tc_base, d_todo, d_work, sg.d_segcnt, sg.d_list, sg.n_list, 1u);
        }
#ifdef MTB_LONG_PHASE_CYCLES
    {   /* profiling build: cycles of thread 0 per phase of k_score_long, summed over the workgroups (and reset) */
        HIPCHK(hipStreamSynchronize(c->stream));
        unsigned long long h[16], z[16] = {0};
        HIPCHK(hipMemcpyFromSymbol(h, HIP_SYMBOL(mtb_long_cycles), sizeof(h)));
        HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(mtb_long_cycles), z, sizeof(z)));
        static const char *nm[10] = {"setup", "block list", "walk", "rank", "species ranges", "combination", "decision", "filter", "taxCnt gather", "descent + output + next read"};
        unsigned long long tot = 0; for (int k = 0; k < 10; k++) tot += h[k];
        fprintf(stderr, "k_score_long phases (%llu reads):", (unsigned long long)(sg.d_list ? sg.n_list : n_reads));
        for (int k = 0; k < 10; k++) fprintf(stderr, " %s %.1f %%;", nm[k], tot ? 100.0 * (double)h[k] / (double)tot : 0.0);
        fprintf(stderr, "\n");
    }
#endif
    }
    hipLaunchKernelGGL(k_count_flags, dim3(256), dim3(256), 0, c->stream, (const uint8_t *)d_todo, n_reads, scal<unsigned long long>(c, SC_N_GENERIC));
    HIPCHK(hipGetLastError());
    uint64_t n_left = 0;
    STCHK(d2h(c, &n_left, scal<uint64_t>(c, SC_N_GENERIC), 8));
    c->fast_used = true;
    if (n_left == 0) return MTB_OK;
    ScoreSrc a; a.m = sg.d_m; a.seg = sg.d_seg; a.sort = false; a.max_seg = std::max<uint32_t>(sg.max_seg, MTB_SCORE_LDS + 1); a.only_flagged = d_todo; a.seg_cnt = sg.d_segcnt;
    a.bound_by_buckets = sg.d_segcnt ? (const void *)sg.d_segcnt : (const void *)sg.d_list;      /* the same taxcnt layout as above */
    uint32_t *d_nl = nullptr;
    if (sg.d_list) { STCHK(ensure(c, "lnlist", 2, &d_nl)); STCHK(h2d(c, d_nl, &sg.n_list, 4)); a.list = sg.d_list; a.n_list = d_nl; a.seg_by_list = 1; }
    uint64_t n_tc2 = 0;
    STCHK(dev_score(c, ix, p, n_reads, lens, out, &n_tc2, a, /* nothing deferred */ nullptr));
    HIPCHK(scal_clear(c, SC_N_GENERIC));         /* put the count back */
    hipLaunchKernelGGL(k_count_flags, dim3(256), dim3(256), 0, c->stream, (const uint8_t *)d_todo, n_reads, scal<unsigned long long>(c, SC_N_GENERIC));
    return MTB_OK;
}
/* Reads of the batch the generic kernel scored (statistics): `all` unless a listing scorer ran since the last call and left its count in SC_N_GENERIC. */
static mtb_status take_generic_reads(mtb_ctx *c, uint64_t all, uint64_t *n) {
    *n = all; if (c->fast_used) { STCHK(d2h(c, n, scal<uint64_t>(c, SC_N_GENERIC), 8)); *n &= 0xFFFFFFFFull; c->fast_used = false; }
    return MTB_OK;
}

/* ------------------------------------------------------------------ */
/* index                                                               */
/* ------------------------------------------------------------------ */
/* per-read match counts of caller-supplied records; rejects sequenceIDs outside 1..n_reads */
static mtb_status count_reads(mtb_ctx *c, const mtb_match *d_in, uint64_t n, uint64_t n_reads, uint32_t *d_rc) {
    HIPCHK(hipMemsetAsync(d_rc, 0, n_reads * 4, c->stream));
    if (n == 0) return MTB_OK;
    HIPCHK(scal_clear(c, SC_BAD_SEQ));
    hipLaunchKernelGGL(k_count_reads, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, c->stream, d_in, n, d_rc, n_reads, scal<uint32_t>(c, SC_BAD_SEQ));
    uint64_t bad = 0;
    STCHK(d2h(c, &bad, scal<uint64_t>(c, SC_BAD_SEQ), 8));
    if (bad) return fail(MTB_ERR_ARG, "match records with a sequenceID outside 1..n_reads");
    return MTB_OK;
}

/* info entries of a database written without Skip_redundancy carry a flag in bit 31 (KmerMatcher.cpp:204-205, IndexCreator.h:355, 400) */
static uint32_t legacy_info_mask(int skip_redundancy) { return ~((uint32_t)(skip_redundancy == 0) << 31); }

static mtb_status upload_taxonomy(mtb_index *ix) {
    const mtbhost::Taxonomy &t = ix->tax;
    size_t n = (size_t)t.max_id + 1;
    HIPCHK(hipMalloc((void **)&ix->d_canon, n * 4)); HIPCHK(hipMalloc((void **)&ix->d_parent, n * 4));
    HIPCHK(hipMalloc((void **)&ix->d_depth, n * 4)); HIPCHK(hipMalloc((void **)&ix->d_spparent, n * 4));
    HIPCHK(hipMalloc((void **)&ix->d_tax2species, n * 4)); HIPCHK(hipMalloc((void **)&ix->d_under, n)); HIPCHK(hipMalloc((void **)&ix->d_accleaf, n));
    /* parent must be indexable for every canonical id; absent ids keep -1 (never dereferenced) */
    HIPCHK(hipMemcpy(ix->d_canon, t.canon.data(), n * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(ix->d_parent, t.parent.data(), n * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(ix->d_depth, t.depth.data(), n * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(ix->d_spparent, t.sp_parent.data(), n * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(ix->d_tax2species, t.tax2species.data(), n * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(ix->d_under, t.under_euk.data(), n, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(ix->d_accleaf, t.acc_leaf.data(), n, hipMemcpyHostToDevice));
    {   /* the same per taxid in one record (k_score_fast) */
        std::vector<mtb_tax_node> nodes(n);
        for (size_t i = 0; i < n; i++) {
            const int32_t c = t.canon[i];
            nodes[i].canon = c;
            nodes[i].depth = c >= 0 ? t.depth[(size_t)c] : 0;
            nodes[i].parent = c >= 0 ? t.parent[(size_t)c] : -1;
            nodes[i].flags = c >= 0 ? ((t.under_euk[(size_t)c] ? 1u : 0u) | (t.acc_leaf[(size_t)c] ? 2u : 0u)) : 0u;
        }
        HIPCHK(hipMalloc((void **)&ix->d_node, n * sizeof(mtb_tax_node)));
        HIPCHK(hipMemcpy(ix->d_node, nodes.data(), n * sizeof(mtb_tax_node), hipMemcpyHostToDevice));
    }
    return MTB_OK;
}

/* A taxonomy and its species table on the device without targets: what the merge and the audit look ids up in.  `tax` is the loaded
 * taxonomy, `ids` the ids the species table is built from (as for a database's taxID_list at index open). */
static mtb_status tax_holder_index(mtb_ctx *c, const mtb_params &params, mtbhost::Taxonomy &&tax, const std::vector<int32_t> &ids, mtb_index **out) {
    mtb_index *hold = new mtb_index();
    hold->ctx = c; hold->params = params; hold->own = true; hold->info_mask = legacy_info_mask(params.skip_redundancy);
    hold->tax = std::move(tax);
    mtbhost::build_tax2species(&hold->tax, ids.data(), ids.size());
    const mtb_status st = upload_taxonomy(hold);
    if (st != MTB_OK) { mtb_index_close(hold); return st; }
    *out = hold;
    return MTB_OK;
}

/* The amino-acid prefix directory of an index that owns (or borrows) a complete flat array: L letters with 21^L >= T / 8, at most
 * 7 (7.2 GB).  Not built (k_join is used) when the index holds a 5-bit letter >= 21 or a directory group spans 2^32 targets.
 * MTB_NO_DIR=1 disables it (A/B measurements). */
static mtb_status build_directory(mtb_ctx *c, mtb_index *ix) {
    if (ix->T < 2 || c->opt.no_dir) return MTB_OK;
    int L = 1;
    while (L < 7 && (uint64_t)mtb_pow21(L) < ix->T / 8) L++;
    if (c->opt.dir_depth > 0) L = std::max(1, std::min(7, c->opt.dir_depth));       /* tests force depth 7 (packed state) on toy indices */
    const uint32_t nbk = mtb_pow21(L);
    const uint32_t n_groups = (nbk >> 16) + 1;
    size_t fr = 0, tot = 0;
    HIPCHK(hipMemGetInfo(&fr, &tot));
    if (((size_t)nbk + 1) * 4 + ((size_t)n_groups + 2) * 8 + (64u << 20) > fr) return MTB_OK;       /* no room: the bisection join still works */
    uint32_t *d_flags = scal<uint32_t>(c, SC_OPEN_FLAGS);
    HIPCHK(hipMalloc((void **)&ix->d_dir, ((size_t)nbk + 1) * 4));
    HIPCHK(hipMalloc((void **)&ix->d_dirbase, ((size_t)n_groups + 2) * 8));
    HIPCHK(hipMemsetAsync(d_flags, 0, 8, c->stream));
    const int fmt = ix->params.kmer_format;
    hipLaunchKernelGGL(k_dir_base, dim3((n_groups + 1 + 255) / 256), dim3(256), 0, c->stream, (const uint64_t *)ix->d_values, ix->T, L, fmt, n_groups, ix->d_dirbase);
    hipLaunchKernelGGL(k_dir_fill, dim3((uint32_t)std::min<uint64_t>((ix->T + 255) / 256, 1u << 20)), dim3(256), 0, c->stream, (const uint64_t *)ix->d_values, ix->T, L, fmt,
                       nbk, (const uint64_t *)ix->d_dirbase, ix->d_dir, d_flags);
    hipLaunchKernelGGL(k_dir_tail, dim3(4096), dim3(256), 0, c->stream, (const uint64_t *)ix->d_values, ix->T, L, fmt, nbk, (const uint64_t *)ix->d_dirbase, ix->d_dir, d_flags);
    HIPCHK(hipGetLastError());
    uint32_t fl[2] = {0, 0};
    STCHK(d2h(c, fl, d_flags, 8));
    if (fl[0] || fl[1]) { hipError_t e = hipFree(ix->d_dir); e = hipFree(ix->d_dirbase); (void)e; ix->d_dir = nullptr; ix->d_dirbase = nullptr; return MTB_OK; }
    ix->dir_L = L; ix->dir_buckets = nbk;
    return MTB_OK;
}

static mtb_dir_view dir_view(const mtb_index *ix) {
    mtb_dir_view dv; dv.dir = ix->d_dir; dv.base = ix->d_dirbase; dv.L = ix->dir_L; dv.kmer_format = ix->params.kmer_format; dv.n_buckets = ix->dir_buckets;
    return dv;
}
/* the two states of the target array: flat {value[T], info[T]} (every stage-level entry point, download / write / slices) and packed
 * (the fused join; depth-7 directory only).  Conversions are in place, ~25 ms each at 16 G targets, and happen only on a change of use. */
/* The partitions of a database directory (host/merge_plan.h: plan_parts) from its file sizes and, for more than one, its `split` table */
static mtb_status plan_parts(const std::string &d, uint32_t n_parts, mtbhost::PartPlan *plan) {
    FILE *f = fopen((d + "/diffIdx").c_str(), "rb"); if (!f) return fail(MTB_ERR_IO, "cannot open " + d + "/diffIdx");
    fseek(f, 0, SEEK_END); const uint64_t n16 = (uint64_t)ftell(f) / 2; fclose(f);
    f = fopen((d + "/info").c_str(), "rb"); if (!f) return fail(MTB_ERR_IO, "cannot open " + d + "/info");
    fseek(f, 0, SEEK_END); const uint64_t T = (uint64_t)ftell(f) / 4; fclose(f);
    std::vector<mtbhost::MergeCheckpoint> sp;
    if (n_parts > 1 && !mtbhost::read_whole(d + "/split", &sp)) return fail(MTB_ERR_IO, "cannot read " + d + "/split");
    mtbhost::plan_parts(sp, T, n16, n_parts, plan);
    return MTB_OK;
}

/* bytes [off, off + len) of a file from / into a (pinned) host buffer, with a few threads: one pread stream tops out near 3 GB/s from
 * the page cache, the files of a GTDB-scale database are ~150 GB */
template <typename Op>
static bool pio_parallel(Op op, int fd, char *buf, uint64_t off, size_t len, int n_threads) {
    if (len == 0) return true;
    const int nt = (int)std::max<size_t>(1, std::min<size_t>((size_t)n_threads, len >> 22));
    std::vector<char> ok((size_t)nt, 1);
    auto part = [&](int t) {
        size_t lo = len * (size_t)t / (size_t)nt, hi = len * ((size_t)t + 1) / (size_t)nt;
        while (lo < hi) {
            const ssize_t r = op(fd, buf + lo, hi - lo, (off_t)(off + lo));
            if (r <= 0) { ok[(size_t)t] = 0; return; }
            lo += (size_t)r;
        }
    };
    if (nt == 1) part(0);
    else { std::vector<std::thread> th; for (int t = 0; t < nt; t++) th.emplace_back(part, t); for (auto &x : th) x.join(); }
    for (char k : ok) if (!k) return false;
    return true;
}
static bool pread_parallel(int fd, void *dst, uint64_t off, size_t len, int n_threads) { return pio_parallel(pread, fd, (char *)dst, off, len, n_threads); }
static bool pwrite_parallel(int fd, const void *src, uint64_t off, size_t len, int n_threads) { return pio_parallel(pwrite, fd, (char *)src, off, len, n_threads); }

/* The target list of a database (or of one value range of it) into HBM, decoded in CHUNKS of the diffIdx stream (the reference streams
 * the files too: KmerMatcher.cpp:212-217, 256-271, getNextTargetKmer KmerMatcher.h:282-297):
 *   chunk of 16-bit words (+ the words of a metamer cut by the previous chunk's end) -> terminators per tile -> offsets -> deltas
 *   written to their final places in value[] -> first delta += the previous chunk's last value -> 64-bit inclusive scan of the chunk
 *   -> the amino-acid directory rows of the chunk (k_dir_chunk_*) -> with `pack`, the chunk's info entries (streamed into a chunk
 *   buffer) are folded into packed 8-byte words at once (kernels_dir.h) and info[] is never resident.
 * Peak HBM: 8 bytes per target (+ 4 for info[] without `pack`) + the directory + one chunk (2 B per word, 4 B per metamer of it):
 * a 16 G-target database opens on one 288 GB GPU; the whole-file decode of round 3 held ~18 bytes per target at once.
 * What is decoded is a range of the files (host/merge_plan.h: MergeSlice), into value[R.records() + 1] and info[R.records()].
 * Only an open asks for more: the directory (and with `pack` the packed state) of the index the arrays belong to, and its statistics.
 * On return dir_ok says whether the directory is usable (else it has been freed); with `pack` a false dir_ok is an error to the
 * caller (the array is partly packed): it opens again without. */
/* 16-bit words per chunk: 128 M (256 MB), less when the context's workspace limit asks for it (a chunk costs ~16 bytes per word: the
 * words twice, tile tables, the info entries of its metamers, scan workspace) */
static uint64_t decode_chunk_words(const mtb_ctx *c) { return c->ws_limit ? std::max<uint64_t>(1u << 16, std::min<uint64_t>(128ull << 20, c->ws_limit / 16)) : 128ull << 20; }
struct OpenDirectory { mtb_index *ix = nullptr; bool want_dir = false; int L = 1; bool pack = false, dir_ok = false; };
/* the decode's chunk buffers in the context's workspace.  A caller declares one DecodeScratch around its decodes (not one per
 * decode: the merge decodes once per slice): they go back when it leaves the scope, whatever way the decodes ended */
static const char *const DECODE_WORDS = "diffraw", *const DECODE_TILE_COUNT = "difftc", *const DECODE_TILE_OFF = "difftoff", *const DECODE_INFO = "infochunk";
struct DecodeScratch { mtb_ctx *c; ~DecodeScratch() { for (const char *nm : {DECODE_WORDS, DECODE_TILE_COUNT, DECODE_TILE_OFF, DECODE_INFO}) release(c, nm); } };
/* A caller that looks at every decoded chunk instead of keeping the array (mtb_database_audit): with a sink, value[] and info[]
 * are CHUNK buffers (chunk_words + 9 values, as many info entries) that every chunk overwrites, the number of entries is
 * whatever the words hold (R.coded_entries() is not consulted; info entries are read while the file has them: R.records()) and on_chunk runs on
 * the stream behind each chunk's decode, before the buffers are reused. */
struct DecodedChunk {
    const uint16_t *d_words; uint64_t n_words, word0;      /* the chunk's words and the file offset (in words, from R.diff_lo) of the first */
    const uint64_t *d_tile_off;                            /* end words before each 2048-word tile of the chunk (and, last, all of them) */
    const uint64_t *d_values; uint64_t n_values;           /* entries first_entry .. first_entry + n_values */
    const uint32_t *d_info; uint64_t n_info;               /* info entries of the first n_info of them */
    uint64_t first_entry;
};
struct ChunkSink {
    uint64_t chunk_words = 0;                              /* 0: decode_chunked's own choice */
    std::function<mtb_status(const DecodedChunk &)> on_chunk;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};        /* recorded before a chunk's upload, behind its decode, behind on_chunk */
    uint64_t n_entries = 0, n_chunks = 0;
    std::atomic<uint64_t> us_read{0};                      /* host clock inside the file reads (they overlap the device) */
    float ms_decode = 0, ms_sink = 0;
};
static mtb_status decode_chunked(mtb_ctx *c, int fmt, const std::string &d, const mtbhost::MergeSlice &R, uint64_t *d_values, uint32_t *d_info, OpenDirectory *dir = nullptr, ChunkSink *sink = nullptr) {
    mtb_index *ix = dir ? dir->ix : nullptr;
    const bool want_dir = dir && dir->want_dir, pack = dir && dir->pack; const int L = dir ? dir->L : 1;
    const uint64_t T = R.records();
    hipStream_t st = c->stream;
    uint64_t CH = decode_chunk_words(c);                   /* MTB_OPEN_CHUNK: tests (a few dozen words) */
    if (c->opt.open_chunk > 0) CH = std::max<uint64_t>(16, (uint64_t)c->opt.open_chunk);
    if (sink && sink->chunk_words) CH = std::max<uint64_t>(16, sink->chunk_words);
    auto timed_read = [sink](int fd, void *dst, uint64_t off, size_t len, int n_threads) {
        const auto t0 = std::chrono::steady_clock::now();
        const bool ok = pread_parallel(fd, dst, off, len, n_threads);
        if (sink) sink->us_read += (uint64_t)std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
        return ok;
    };
    const uint32_t nbk = want_dir ? mtb_pow21(L) : 0, n_groups = want_dir ? (nbk >> 16) + 1 : 0;
    uint32_t *d_flags = scal<uint32_t>(c, SC_OPEN_FLAGS);
    uint64_t *d_carry = scal<uint64_t>(c, SC_OPEN_CARRY);                      /* last flat value of the previous chunk */
    if (want_dir) {
        HIPCHK(hipMalloc((void **)&ix->d_dir, ((size_t)nbk + 1) * 4));
        HIPCHK(hipMalloc((void **)&ix->d_dirbase, ((size_t)n_groups + 2) * 8));
        HIPCHK(hipMemsetAsync(d_flags, 0, 8, st));
    }
    const int fd_d = open((d + "/diffIdx").c_str(), O_RDONLY), fd_i = open((d + "/info").c_str(), O_RDONLY);
    struct Files { int a, b; ~Files() { if (a >= 0) close(a); if (b >= 0) close(b); } } files{fd_d, fd_i};
    if (fd_d < 0 || fd_i < 0) return fail(MTB_ERR_IO, "cannot open diffIdx / info in " + d);
    const uint64_t chunk_words = std::min<uint64_t>(CH, std::max<uint64_t>(R.words(), 1));
    const uint64_t info_cap = std::min<uint64_t>(chunk_words + 8, T + 1);      /* metamers of a chunk <= its words */
    struct Pinned { void *p[3] = {nullptr, nullptr, nullptr}; ~Pinned() { for (void *q : p) if (q) { hipError_t e = hipHostFree(q); (void)e; } } } pin;
    if (hipHostMalloc(&pin.p[0], (chunk_words + 8) * 2, hipHostMallocDefault) != hipSuccess || hipHostMalloc(&pin.p[1], (chunk_words + 8) * 2, hipHostMallocDefault) != hipSuccess ||
        hipHostMalloc(&pin.p[2], info_cap * 4, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return fail(MTB_ERR_OOM, "no pinned host memory for the index upload"); }
    uint16_t *d_chunk; uint32_t *d_tc; uint64_t *d_toff, *d_ws; uint32_t *d_ichunk = nullptr;
    const uint64_t max_tiles = (chunk_words + 8 + 2047) / 2048 + 1;
    STCHK(ensure(c, DECODE_WORDS, chunk_words + 8, &d_chunk)); STCHK(ensure(c, DECODE_TILE_COUNT, max_tiles, &d_tc)); STCHK(ensure(c, DECODE_TILE_OFF, max_tiles + 1, &d_toff));
    STCHK(ensure(c, "scanws", scan_ws_elems(std::max<uint64_t>(max_tiles + 1, info_cap + 1)), &d_ws));
    if (pack) STCHK(ensure(c, DECODE_INFO, info_cap, &d_ichunk));
    { const uint64_t c0 = R.lead ? R.first_value : 0; STCHK(h2d(c, d_carry, &c0, 8)); }
    if (R.lead) {
        /* a range that starts at a split checkpoint: its first metamer is given by the checkpoint, not coded in the byte range -- a chunk
         * of one entry (value, info entry, directory rows, packing) */
        STCHK(h2d(c, d_values, &R.first_value, 8));
        if (!pread_parallel(fd_i, pin.p[2], R.info_lo * 4, 4, 1)) return fail(MTB_ERR_IO, "short read from " + d + "/info");
        STCHK(h2d(c, pack ? d_ichunk : d_info, pin.p[2], 4));
        if (want_dir) {
            hipLaunchKernelGGL(k_dir_chunk_base, dim3(1), dim3(256), 0, st, (const uint64_t *)d_values, (uint64_t)0, (uint64_t)1, (const uint64_t *)d_carry, L, fmt, nbk, ix->d_dirbase, d_flags);
            hipLaunchKernelGGL(k_dir_chunk_fill, dim3(1), dim3(256), 0, st, (const uint64_t *)d_values, (uint64_t)0, (uint64_t)1, (const uint64_t *)d_carry, L, fmt, nbk,
                               (const uint64_t *)ix->d_dirbase, ix->d_dir, d_flags);
        }
        if (pack) hipLaunchKernelGGL(k_index_pack_chunk, dim3(1), dim3(256), 0, st, d_values, (const uint32_t *)d_ichunk, (uint64_t)0, (uint64_t)1, fmt);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(st));
    }
    if (ix) ix->open_chunk_words = chunk_words;
    uint64_t done_words = 0, g = R.lead, found = 0;       /* g: next free place in value[] */
    uint16_t carry_w[8]; uint32_t n_carry = 0;
    /* the first chunk is read here, every further one by a helper thread while the device works on its predecessor */
    uint64_t cur_new = std::min<uint64_t>(chunk_words, R.words());
    if (cur_new && !timed_read(fd_d, pin.p[0], (R.diff_lo + done_words) * 2, cur_new * 2, 16)) return fail(MTB_ERR_IO, "short read from " + d + "/diffIdx");
    int cur = 0;
    while (done_words < R.words()) {
        const uint64_t next_off = done_words + cur_new, next_new = std::min<uint64_t>(chunk_words, R.words() - next_off);
        bool next_ok = true;
        std::thread reader;
        if (next_new) reader = std::thread([&, next_off, next_new] { next_ok = timed_read(fd_d, pin.p[cur ^ 1], (R.diff_lo + next_off) * 2, next_new * 2, 16); });
        struct Join { std::thread &t; ~Join() { if (t.joinable()) t.join(); } } join_reader{reader};
        const uint16_t *hw = (const uint16_t *)pin.p[cur];
        /* words of a metamer cut by this chunk's end stay for the next one */
        uint32_t tail = 0;
        while (tail < 5 && tail < cur_new && !(hw[cur_new - 1 - tail] & 0x8000u)) tail++;
        if (tail == cur_new && cur_new < 5) { /* (a chunk of fewer than five words without a terminator: all of it is carried) */ }
        if (tail >= 5 || (next_new == 0 && tail != 0)) return fail(MTB_ERR_IO, "diffIdx is corrupt: a metamer without its terminator word");
        const uint64_t use_new = cur_new - tail, n_use = n_carry + use_new;
        if (sink) HIPCHK(hipEventRecord(sink->ev[0], st));
        if (n_carry) HIPCHK(hipMemcpyAsync(d_chunk, carry_w, n_carry * 2, hipMemcpyHostToDevice, st));
        if (use_new) HIPCHK(hipMemcpyAsync(d_chunk + n_carry, hw, use_new * 2, hipMemcpyHostToDevice, st));
        uint64_t n_k = 0;
        if (n_use) {
            const uint64_t tiles = (n_use + 2047) / 2048;
            hipLaunchKernelGGL(k_diff_tile_count, dim3((uint32_t)tiles), dim3(256), 0, st, (const uint16_t *)d_chunk, n_use, d_tc);
            scan_launch<uint32_t, uint64_t, false>(st, d_tc, tiles, true, d_toff, d_ws);
            STCHK(d2h(c, &n_k, d_toff + tiles, 8));
            if (!sink && found + n_k > R.coded_entries()) return fail(MTB_ERR_IO, "diffIdx holds more metamers than info and split announce (" + std::to_string(R.coded_entries()) + ")");
            if (n_k) {
                const uint64_t m = std::min<uint64_t>(g + n_k, T) - std::min<uint64_t>(g, T);       /* entries of the chunk that belong to the index (a dropped last one does not) */
                const uint64_t at = sink ? 0 : g;                  /* where the chunk goes in value[] / info[] */
                /* info entries of the chunk: into the chunk buffer (pack) or straight to their places */
                if (m) {
                    if (!timed_read(fd_i, pin.p[2], (R.info_lo + g) * 4, m * 4, 16)) return fail(MTB_ERR_IO, "short read from " + d + "/info");
                    HIPCHK(hipMemcpyAsync(pack ? d_ichunk : d_info + at, pin.p[2], m * 4, hipMemcpyHostToDevice, st));
                }
                hipLaunchKernelGGL(k_diff_assemble, dim3((uint32_t)tiles), dim3(256), 0, st, (const uint16_t *)d_chunk, n_use, (const uint64_t *)d_toff, d_values + at);
                hipLaunchKernelGGL(k_diff_add_carry, dim3(1), dim3(1), 0, st, d_values + at, (const uint64_t *)d_carry);
                scan_launch<uint64_t, uint64_t, true>(st, d_values + at, n_k, false, d_values + at, d_ws);
                if (want_dir && m) {
                    const dim3 grid((uint32_t)std::min<uint64_t>((m + 255) / 256, 1u << 16));
                    hipLaunchKernelGGL(k_dir_chunk_base, grid, dim3(256), 0, st, (const uint64_t *)d_values, g, m, (const uint64_t *)d_carry, L, fmt, nbk, ix->d_dirbase, d_flags);
                    hipLaunchKernelGGL(k_dir_chunk_fill, grid, dim3(256), 0, st, (const uint64_t *)d_values, g, m, (const uint64_t *)d_carry, L, fmt, nbk,
                                       (const uint64_t *)ix->d_dirbase, ix->d_dir, d_flags);
                }
                hipLaunchKernelGGL(k_save_last, dim3(1), dim3(1), 0, st, (const uint64_t *)(d_values + at + n_k - 1), d_carry);
                if (sink) {
                    HIPCHK(hipEventRecord(sink->ev[1], st));
                    DecodedChunk ck;
                    ck.d_words = d_chunk; ck.n_words = n_use; ck.word0 = done_words - n_carry; ck.d_tile_off = d_toff;
                    ck.d_values = d_values; ck.n_values = n_k; ck.d_info = d_info; ck.n_info = m; ck.first_entry = g;
                    STCHK(sink->on_chunk(ck));
                    HIPCHK(hipEventRecord(sink->ev[2], st));
                }
                if (pack && m) hipLaunchKernelGGL(k_index_pack_chunk, dim3((uint32_t)std::min<uint64_t>((m + 255) / 256, 1u << 16)), dim3(256), 0, st, d_values, (const uint32_t *)d_ichunk, g, m, fmt);
                HIPCHK(hipGetLastError());
                HIPCHK(hipStreamSynchronize(st));          /* the pinned buffers are refilled next */
                if (sink) {
                    float ms = 0;
                    HIPCHK(hipEventElapsedTime(&ms, sink->ev[0], sink->ev[1])); sink->ms_decode += ms;
                    HIPCHK(hipEventElapsedTime(&ms, sink->ev[1], sink->ev[2])); sink->ms_sink += ms;
                    sink->n_chunks++;
                }
                g += n_k; found += n_k;
                if (ix && (ix->open_chunks < 4 || (ix->open_chunks & 63u) == 0)) {        /* (a driver query: not for every one of thousands of tiny test chunks) */
                    size_t fr = 0, tot = 0; if (hipMemGetInfo(&fr, &tot) == hipSuccess && ix->open_free0 > fr) ix->open_peak_bytes = std::max<uint64_t>(ix->open_peak_bytes, ix->open_free0 - fr); }
                if (ix) ix->open_chunks++;
            }
        }
        for (uint32_t k = 0; k < tail; k++) carry_w[k] = hw[cur_new - tail + k];
        if (n_use == 0 && n_carry) { /* nothing decodable yet: keep the old carry in front (cannot happen: a carry is < 5 words and a metamer ends within 5) */
            return fail(MTB_ERR_IO, "diffIdx is corrupt: a metamer of more than five words"); }
        n_carry = tail;
        if (reader.joinable()) reader.join();
        if (!next_ok) return fail(MTB_ERR_IO, "short read from " + d + "/diffIdx");
        done_words = next_off; cur_new = next_new; cur ^= 1;
    }
    if (sink) sink->n_entries = found;
    else if (found != R.coded_entries())    /* validateDatabase.cpp:17-142: #terminators must equal #info entries */
        return fail(MTB_ERR_IO, "diffIdx holds " + std::to_string(found) + " metamers where info and split announce " + std::to_string(R.coded_entries()));
    if (want_dir) {
        /* (*d_carry = the last decoded value; with a dropped last entry the index's own last flat value is one before it: re-read it) */
        if (T && g > T) {
            if (pack) return fail(MTB_ERR_UNSUPPORTED, "pack on load of a range whose last coded metamer is dropped");       /* (never chosen: see open_impl) */
            hipLaunchKernelGGL(k_save_last, dim3(1), dim3(1), 0, st, (const uint64_t *)(d_values + T - 1), d_carry);
        }
        hipLaunchKernelGGL(k_dir_finish, dim3(64), dim3(256), 0, st, (const uint64_t *)d_carry, T, L, fmt, nbk, n_groups, ix->d_dirbase, ix->d_dir, d_flags, 0);
        hipLaunchKernelGGL(k_dir_finish, dim3(4096), dim3(256), 0, st, (const uint64_t *)d_carry, T, L, fmt, nbk, n_groups, ix->d_dirbase, ix->d_dir, d_flags, 1);
        HIPCHK(hipGetLastError());
        uint32_t fl[2] = {0, 0};
        STCHK(d2h(c, fl, d_flags, 8));
        if (fl[0] || fl[1]) { hipError_t e = hipFree(ix->d_dir); e = hipFree(ix->d_dirbase); (void)e; ix->d_dir = nullptr; ix->d_dirbase = nullptr; }
        else { ix->dir_L = L; ix->dir_buckets = nbk; dir->dir_ok = true; }
    }
    HIPCHK(hipStreamSynchronize(st));
    return MTB_OK;
}

/* An open that finds device memory short of what the index needs: the workspace a concurrent (or earlier) mtb_ctx_reserve took is worth
 * less than the directory or the database itself -- stop the reservation, give the workspace back (batches grow it again as they did
 * before there was a reservation).  Returns the free bytes afterwards. */
static size_t open_make_room(mtb_ctx *c) {
    c->reserve_cancel = true;
    /* nothing may still be reading the workspace that is handed back: batches queued on the compute stream (another index of this context),
     * results on their way down (asynchronous entry point), a prefetch into the input sets (those are I/O buffers and stay, but their
     * records must not outlive a context whose streams were drained) -- ADVICE r5 */
    { hipError_t e = hipStreamSynchronize(c->stream); (void)e;
      if (c->down_stream) { e = hipStreamSynchronize(c->down_stream); (void)e; c->down_pending = false; }
      if (c->copy_stream) { e = hipStreamSynchronize(c->copy_stream); (void)e; } }
    c->last_sorted = nullptr; c->last_sorted_n = 0;       /* (pointed into the workspace) */
    { std::lock_guard<std::mutex> lk(c->reserve_mu); release_workspace(c); }
    size_t fr = 0, tot = 0;
    hipError_t e = hipMemGetInfo(&fr, &tot); (void)e;
    return fr;
}

/* the taxonomy of a database directory and the ids of its taxID_list (the species table is built from them, KmerMatcher::
 * loadTaxIdList: build_tax2species): taxonomyDB if `have_bin` and it loads, else the dump files of `taxdir` (an unreadable taxonomyDB: DBDIR/taxonomy) */
static mtb_status load_database_taxonomy(const std::string &d, std::string taxdir, bool have_bin, mtbhost::Taxonomy *tax, std::vector<int32_t> *ids) {
    std::string err;
    bool tax_ok = false;
    if (have_bin) {
        tax_ok = mtbhost::load_taxonomy_db(d + "/taxonomyDB", tax, &err);
        if (!tax_ok) {
            const std::string fb = d + "/taxonomy";
            if (!mtbhost::file_exists(fb + "/nodes.dmp")) return fail(MTB_ERR_IO, err);
            taxdir = fb; err.clear();
        }
    }
    if (!tax_ok && !mtbhost::load_taxonomy(taxdir, tax, &err)) return fail(MTB_ERR_IO, err);
    if (!mtbhost::read_taxid_list(d + "/taxID_list", ids)) return fail(MTB_ERR_IO, "cannot open " + d + "/taxID_list");
    return MTB_OK;
}

static mtb_status open_impl(mtb_ctx *c, const char *dbdir, const char *taxonomy_dir, mtb_params *params, uint32_t part, uint32_t n_parts, mtb_index **out) {
    if (!c || !dbdir || !params || !out) return fail(MTB_ERR_ARG, "NULL argument");
    if (n_parts == 0 || part >= n_parts) return fail(MTB_ERR_ARG, "partition index out of range");
    HIPCHK(hipSetDevice(c->device));
    std::string d(dbdir);
    int reduced_aa = 0;
    mtbhost::load_db_parameters(d, params, &reduced_aa);
    if (reduced_aa) return fail(MTB_ERR_UNSUPPORTED, "database was built with the reduced amino-acid alphabet (Reduced_alphabet 1 in db.parameters); not implemented");
    if (params->kmer_format != 1 && params->kmer_format != 2) return fail(MTB_ERR_UNSUPPORTED, "database uses a k-mer format other than 1 or 2");
    /* loadTaxonomy (common.cpp:50-86): DBDIR/taxonomyDB wins when it is there and readable; else --taxonomy-path; else
     * DBDIR/taxonomy/.  (A taxonomyDB with an outdated serialization version makes the reference fall back to DBDIR/taxonomy.) */
    std::string taxdir = taxonomy_dir && *taxonomy_dir ? std::string(taxonomy_dir) : d + "/taxonomy";
    const bool have_bin = mtbhost::file_exists(d + "/taxonomyDB");
    if (!have_bin && !mtbhost::file_exists(taxdir + "/nodes.dmp"))
        return fail(MTB_ERR_IO, "no taxonomy: neither " + d + "/taxonomyDB nor dump files in " + taxdir);
    mtbhost::PartPlan plan;
    STCHK(plan_parts(d, n_parts, &plan));
    const bool empty = plan.parts[part].empty;
    const mtbhost::MergeSlice &R = plan.parts[part].r;
    mtb_index *ix = new mtb_index();
    /* every early return below hands the index (and what it holds on the device) back */
    struct Guard { mtb_index *ix; ~Guard() { if (ix) mtb_index_close(ix); } } guard{ix};
    ix->ctx = c; ix->params = *params; ix->own = true;
    for (uint32_t q = part + 1; q < n_parts; q++) if (!plan.parts[q].empty) ix->match_last = true;
    std::vector<int32_t> ids;
    STCHK(load_database_taxonomy(d, taxdir, have_bin, &ix->tax, &ids));
    mtbhost::build_tax2species(&ix->tax, ids.data(), ids.size());
    ix->info_mask = legacy_info_mask(params->skip_redundancy);
    STCHK(upload_taxonomy(ix));
    if (empty) { ix->T = 0; guard.ix = nullptr; *out = ix; return MTB_OK; }
    /* only this partition's byte ranges are read from the files, chunk by chunk through pinned buffers straight into HBM (the next
     * chunk is read while the device decodes the current one): no whole-file copy in host OR device memory, whatever the database size */
    const uint64_t T = R.records();
    /* the directory this index will have (build_directory's rule), decided before the load so that it is built chunk by chunk */
    int L = 1;
    while (L < 7 && (uint64_t)mtb_pow21(L) < T / 8) L++;
    if (c->opt.dir_depth > 0) L = std::max(1, std::min(7, c->opt.dir_depth));
    bool want_dir = T >= 2 && !c->opt.no_dir;
    struct CancelReset { mtb_ctx *c; ~CancelReset() { c->reserve_cancel = false; } } cancel_reset{c};
    if (want_dir) {
        size_t fr = 0, tot = 0;
        HIPCHK(hipMemGetInfo(&fr, &tot));
        const uint32_t nbk = mtb_pow21(L);
        /* directory + target words + (flat state) info[] + the chunk buffers of the decode */
        const bool pack_guess = L == 7 && !R.drop_last && !c->opt.no_pack && (c->opt.open_packed >= 0 ? c->opt.open_packed != 0 : T >= (1ull << 28));
        const size_t need_dir = ((size_t)nbk + 1) * 4 + ((size_t)(nbk >> 16) + 3) * 8 + (T + 1) * 8 + (64u << 20);
        const size_t need_all = need_dir + (pack_guess ? 0 : (size_t)T * 4) + (std::min<uint64_t>(R.words(), 1ull << 27) * 12 + (64u << 20));
        if (need_all > fr && held_bytes(c, BUF_FIXED) > 0) fr = open_make_room(c);      /* a reservation made for the first batches must not cost the index its directory */
        if (need_dir > fr) want_dir = false;        /* no room next to the values: the bisection join still works */
    }
    /* pack on load: big databases (>= 2^28 targets; MTB_OPEN_PACKED=1 / 0 forces it on toy databases / off) whose directory has depth 7
     * open in the SEALED state -- packed 8-byte words, info[] never resident (mtb_index_seal's state; everything that needs the flat
     * arrays unpacks on demand as for any sealed index) */
    bool pack = want_dir && L == 7 && !R.drop_last && !c->opt.no_pack && (c->opt.open_packed >= 0 ? c->opt.open_packed != 0 : T >= (1ull << 28));
    { size_t fr = 0, tot = 0; HIPCHK(hipMemGetInfo(&fr, &tot)); ix->open_free0 = fr; }
    for (int attempt = 0; attempt < 2; attempt++) {
        ix->open_chunks = 0; ix->open_peak_bytes = 0;
        {   /* short of memory with a workspace reservation in the way: hand the reservation back and try once more */
            hipError_t e = hipMalloc((void **)&ix->d_values, (T + 1) * 8);
            if (e == hipErrorOutOfMemory && held_bytes(c, BUF_FIXED) > 0) { (void)hipGetLastError(); open_make_room(c); e = hipMalloc((void **)&ix->d_values, (T + 1) * 8); }
            HIPCHK(e);
            if (!pack) {
                e = hipMalloc((void **)&ix->d_info, std::max<uint64_t>(T, 1) * 4);
                if (e == hipErrorOutOfMemory && held_bytes(c, BUF_FIXED) > 0) { (void)hipGetLastError(); open_make_room(c); e = hipMalloc((void **)&ix->d_info, std::max<uint64_t>(T, 1) * 4); }
                HIPCHK(e);
            }
        }
        OpenDirectory dir; dir.ix = ix; dir.want_dir = want_dir; dir.L = L; dir.pack = pack;
        {   DecodeScratch scratch{c};
            STCHK(decode_chunked(c, params->kmer_format, d, R, ix->d_values, ix->d_info, &dir)); }
        if (pack && !dir.dir_ok) {      /* a letter >= 21 or a bucket group of 2^32 targets: no directory, hence no packed state -- once more, flat */
            hipError_t e = hipFree(ix->d_values); (void)e; ix->d_values = nullptr;
            pack = false;
            continue;
        }
        if (pack) ix->packed = true;
        break;
    }
    ix->T = T;
    guard.ix = nullptr;
    *out = ix;
    return MTB_OK;
}

extern "C" {

mtb_status mtb_index_open(mtb_ctx *c, const char *dbdir, const char *taxonomy_dir, mtb_params *params, mtb_index **out) {
    return open_impl(c, dbdir, taxonomy_dir, params, 0, 1, out);
}
mtb_status mtb_index_open_part(mtb_ctx *c, const char *dbdir, const char *taxonomy_dir, mtb_params *params, uint32_t part, uint32_t n_parts,
                               mtb_index **out) {
    STCHK(open_impl(c, dbdir, taxonomy_dir, params, part, n_parts, out));
    (*out)->is_part = true;
    return MTB_OK;
}
mtb_status mtb_index_part_bounds(const char *dbdir, uint32_t n_parts, uint64_t *bounds) {
    if (!dbdir || !bounds || n_parts == 0) return fail(MTB_ERR_ARG, "NULL argument");
    mtbhost::PartPlan plan;
    STCHK(plan_parts(dbdir, n_parts, &plan));
    for (uint32_t p = 0; p < n_parts; p++) bounds[p] = plan.bounds[p];
    return MTB_OK;
}

mtb_status mtb_index_from_device(mtb_ctx *c, uint64_t *d_values, uint32_t *d_info, uint64_t n_targets, const char *taxonomy_dir,
                                 const int32_t *taxid_list, size_t n_taxids, const mtb_params *params, mtb_index **out) {
    if (!c || !taxonomy_dir || !params || !out) return fail(MTB_ERR_ARG, "NULL argument");
    HIPCHK(hipSetDevice(c->device));
    mtb_index *ix = new mtb_index();
    ix->ctx = c; ix->params = *params; ix->own = false;
    std::string err;
    if (!mtbhost::load_taxonomy(taxonomy_dir, &ix->tax, &err)) { delete ix; return fail(MTB_ERR_IO, err); }
    mtbhost::build_tax2species(&ix->tax, taxid_list, n_taxids);
    ix->info_mask = legacy_info_mask(params->skip_redundancy);
    ix->d_values = d_values; ix->d_info = d_info; ix->T = n_targets;
    mtb_status st = upload_taxonomy(ix);
    if (st != MTB_OK) { mtb_index_close(ix); return st; }
    if ((st = build_directory(c, ix)) != MTB_OK) { mtb_index_close(ix); return st; }
    *out = ix;
    return MTB_OK;
}

/* "load once, broadcast over xGMI".  The resident index of one GPU copied to another context's GPU with peer
 * copies (hipMemcpyPeerAsync: device to device over xGMI where the devices can reach each other; same-device contexts get a
 * device-to-device copy) -- the target words in the state they are in (packed / flat), info[] if it is resident, the directory --
 * and the taxonomy tables uploaded from the host copy.  A node that classifies on 8 GPUs reads and decodes the database files once
 * instead of 8 times.  The reference has one address space and no analogue (KmerMatcher.cpp:212-217 opens the files per thread). */
mtb_status mtb_index_clone(mtb_index *src, mtb_ctx *dst, mtb_index **out) {
    if (!src || !dst || !out) return fail(MTB_ERR_ARG, "NULL argument");
    if (src->parent) return fail(MTB_ERR_ARG, "a view cannot be cloned: clone its parent");
    mtb_ctx *sc = src->ctx;
    if (sc->device != dst->device) {
        int can = 0;
        if (hipDeviceCanAccessPeer(&can, dst->device, sc->device) == hipSuccess && can) {
            if (hipSetDevice(dst->device) == hipSuccess) { const hipError_t e = hipDeviceEnablePeerAccess(sc->device, 0); if (e != hipSuccess) (void)hipGetLastError(); }      /* (twice = "already on") */
        } else (void)hipGetLastError();
    }
    HIPCHK(hipSetDevice(dst->device));
    mtb_index *ix = new mtb_index();
    struct Guard { mtb_index *ix; ~Guard() { if (ix) mtb_index_close(ix); } } guard{ix};
    ix->ctx = dst; ix->params = src->params; ix->own = true; ix->tax = src->tax; ix->info_mask = src->info_mask; ix->match_last = src->match_last; ix->T = src->T;
    STCHK(upload_taxonomy(ix));
    IndexUse use;                                   /* the source keeps its state (and is not converted) while it is read */
    {
        std::unique_lock<std::mutex> lk(src->state_mu);
        src->users++; use.o = src;
    }
    const bool packed = src->packed;
    auto peer = [&](void *d, const void *s_, size_t bytes) -> mtb_status {
        const size_t CH = 1ull << 30;               /* 1 GiB pieces: progress is visible to the stream, a failure is local */
        for (size_t o = 0; o < bytes; o += CH) {
            const size_t nb = std::min(CH, bytes - o);
            if (sc->device == dst->device) HIPCHK(hipMemcpyAsync((char *)d + o, (const char *)s_ + o, nb, hipMemcpyDeviceToDevice, dst->stream));
            else HIPCHK(hipMemcpyPeerAsync((char *)d + o, dst->device, (const char *)s_ + o, sc->device, nb, dst->stream));
        }
        return MTB_OK;
    };
    HIPCHK(hipStreamSynchronize(sc->stream));       /* whatever the source context still had in flight on the arrays */
    HIPCHK(hipMalloc((void **)&ix->d_values, (src->T + 1) * 8));
    STCHK(peer(ix->d_values, src->d_values, src->T * 8));
    if (src->d_info) { HIPCHK(hipMalloc((void **)&ix->d_info, std::max<uint64_t>(src->T, 1) * 4)); STCHK(peer(ix->d_info, src->d_info, src->T * 4)); }
    if (src->d_dir) {
        const uint32_t n_groups = (src->dir_buckets >> 16) + 1;
        HIPCHK(hipMalloc((void **)&ix->d_dir, ((size_t)src->dir_buckets + 1) * 4));
        HIPCHK(hipMalloc((void **)&ix->d_dirbase, ((size_t)n_groups + 2) * 8));
        STCHK(peer(ix->d_dir, src->d_dir, ((size_t)src->dir_buckets + 1) * 4));
        STCHK(peer(ix->d_dirbase, src->d_dirbase, ((size_t)n_groups + 2) * 8));
        ix->dir_L = src->dir_L; ix->dir_buckets = src->dir_buckets;
    }
    HIPCHK(hipStreamSynchronize(dst->stream));
    ix->packed = packed;
    guard.ix = nullptr;
    *out = ix;
    return MTB_OK;
}

/* ---- the resident index handed to other PROCESSES of the node (include/mtb.h: mtb_index_share) ---- */
/* An allocation below a few MB is carved out of a larger block by the runtime and cannot be opened by another process (dmabuf handles name whole
 * blocks: hipIpcOpenMemHandle answered "invalid argument" for the 160 KB target array of a toy database): such an array is copied to a 4 MiB
 * allocation of its own first (`stage`, kept by the index until it is closed or exported again) and that one is handed over. */
static mtb_status ipc_describe(mtb_ctx *c, const void *p, size_t bytes, void **stage, uint8_t handle[64], uint64_t *off) {
    static_assert(sizeof(hipIpcMemHandle_t) <= 64, "handle record");
    memset(handle, 0, 64); *off = 0;
    if (*stage) { hipError_t e = hipFree(*stage); (void)e; *stage = nullptr; }
    if (!p) return MTB_OK;
    if (bytes < (4ull << 20)) {
        HIPCHK(hipMalloc(stage, 4ull << 20));
        HIPCHK(hipMemcpyAsync(*stage, p, bytes, hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        p = *stage;
    }
    hipDeviceptr_t base = nullptr; size_t size = 0;
    HIPCHK(hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)p));            /* the handle names the ALLOCATION (a torch tensor may sit inside a larger block) */
    hipIpcMemHandle_t h;
    HIPCHK(hipIpcGetMemHandle(&h, (void *)base));
    memcpy(handle, &h, sizeof(h));
    *off = (uint64_t)((const char *)p - (const char *)base);
    return MTB_OK;
}
mtb_status mtb_index_export(mtb_index *src, mtb_index_share *out) {
    if (!src || !out) return fail(MTB_ERR_ARG, "NULL argument");
    if (src->parent) return fail(MTB_ERR_ARG, "a view cannot be exported: export its parent");
    memset(out, 0, sizeof(*out));
    HIPCHK(hipSetDevice(src->ctx->device));
    HIPCHK(hipStreamSynchronize(src->ctx->stream));
    std::unique_lock<std::mutex> lk(src->state_mu);
    src->state_cv.wait(lk, [&] { return src->users == 0; });
    const uint32_t n_groups = (src->dir_buckets >> 16) + 1;
    STCHK(ipc_describe(src->ctx, src->d_values, src->T * 8, &src->ipc_stage[0], out->values_handle, &out->values_off));
    STCHK(ipc_describe(src->ctx, src->d_info, src->T * 4, &src->ipc_stage[1], out->info_handle, &out->info_off));
    STCHK(ipc_describe(src->ctx, src->d_dir, ((size_t)src->dir_buckets + 1) * 4, &src->ipc_stage[2], out->dir_handle, &out->dir_off));
    STCHK(ipc_describe(src->ctx, src->d_dirbase, ((size_t)n_groups + 2) * 8, &src->ipc_stage[3], out->dirbase_handle, &out->dirbase_off));
    out->n_targets = src->T; out->dir_buckets = src->dir_buckets; out->info_mask = src->info_mask; out->dir_depth = src->dir_L;
    out->packed = src->packed ? 1 : 0; out->has_info = src->d_info ? 1 : 0; out->match_last = src->match_last ? 1 : 0; out->device = src->ctx->device;
    out->exporter_pid = (int64_t)getpid();
    out->values_ptr = (uint64_t)(uintptr_t)src->d_values; out->info_ptr = (uint64_t)(uintptr_t)src->d_info;
    out->dir_ptr = (uint64_t)(uintptr_t)src->d_dir; out->dirbase_ptr = (uint64_t)(uintptr_t)src->d_dirbase;
    return MTB_OK;
}
mtb_status mtb_index_import(mtb_ctx *c, const mtb_index_share *sh, const char *taxonomy_dir, const int32_t *taxid_list, size_t n_taxids,
                            const mtb_params *params, mtb_index **out) {
    if (!c || !sh || !taxonomy_dir || !params || !out) return fail(MTB_ERR_ARG, "NULL argument");
    HIPCHK(hipSetDevice(c->device));
    mtb_index *ix = new mtb_index();
    struct Guard { mtb_index *ix; ~Guard() { if (ix) mtb_index_close(ix); } } guard{ix};
    ix->ctx = c; ix->params = *params; ix->own = true; ix->T = sh->n_targets; ix->info_mask = sh->info_mask; ix->match_last = sh->match_last != 0;
    std::string err;
    if (!mtbhost::load_taxonomy(taxonomy_dir, &ix->tax, &err)) return fail(MTB_ERR_IO, err);
    mtbhost::build_tax2species(&ix->tax, taxid_list, n_taxids);
    STCHK(upload_taxonomy(ix));
    const bool same_process = sh->exporter_pid == (int64_t)getpid();
    if (!same_process && sh->device != c->device) {                      /* the exporter's GPU is another one: copies go over the fabric */
        int can = 0;
        if (hipDeviceCanAccessPeer(&can, c->device, sh->device) == hipSuccess && can) { const hipError_t e = hipDeviceEnablePeerAccess(sh->device, 0); if (e != hipSuccess) (void)hipGetLastError(); }
        else (void)hipGetLastError();
    }
    void *opened[4] = {nullptr, nullptr, nullptr, nullptr};
    struct Closer { void **o; ~Closer() { for (int k = 0; k < 4; k++) if (o[k]) { hipError_t e = hipIpcCloseMemHandle(o[k]); (void)e; } } } closer{opened};
    /* array k of the exporter as a pointer this process may copy from */
    auto source = [&](int k, const uint8_t handle[64], uint64_t off, uint64_t direct, const void **p) -> mtb_status {
        *p = nullptr;
        if (same_process) { *p = (const void *)(uintptr_t)direct; return MTB_OK; }
        hipIpcMemHandle_t h; memcpy(&h, handle, sizeof(h));
        HIPCHK(hipIpcOpenMemHandle(&opened[k], h, hipIpcMemLazyEnablePeerAccess));
        *p = (const char *)opened[k] + off;
        return MTB_OK;
    };
    auto copy = [&](void *d, const void *s_, size_t bytes) -> mtb_status {
        const size_t CH = 1ull << 30;
        for (size_t o = 0; o < bytes; o += CH) HIPCHK(hipMemcpyAsync((char *)d + o, (const char *)s_ + o, std::min(CH, bytes - o), hipMemcpyDefault, c->stream));
        return MTB_OK;
    };
    const void *sp = nullptr;
    STCHK(source(0, sh->values_handle, sh->values_off, sh->values_ptr, &sp));
    HIPCHK(hipMalloc((void **)&ix->d_values, (ix->T + 1) * 8));
    STCHK(copy(ix->d_values, sp, ix->T * 8));
    if (sh->has_info) {
        STCHK(source(1, sh->info_handle, sh->info_off, sh->info_ptr, &sp));
        HIPCHK(hipMalloc((void **)&ix->d_info, std::max<uint64_t>(ix->T, 1) * 4));
        STCHK(copy(ix->d_info, sp, ix->T * 4));
    }
    if (sh->dir_depth > 0) {
        const uint32_t n_groups = (sh->dir_buckets >> 16) + 1;
        HIPCHK(hipMalloc((void **)&ix->d_dir, ((size_t)sh->dir_buckets + 1) * 4));
        HIPCHK(hipMalloc((void **)&ix->d_dirbase, ((size_t)n_groups + 2) * 8));
        STCHK(source(2, sh->dir_handle, sh->dir_off, sh->dir_ptr, &sp));
        STCHK(copy(ix->d_dir, sp, ((size_t)sh->dir_buckets + 1) * 4));
        STCHK(source(3, sh->dirbase_handle, sh->dirbase_off, sh->dirbase_ptr, &sp));
        STCHK(copy(ix->d_dirbase, sp, ((size_t)n_groups + 2) * 8));
        ix->dir_L = sh->dir_depth; ix->dir_buckets = sh->dir_buckets;
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    ix->packed = sh->packed != 0;
    guard.ix = nullptr;
    *out = ix;
    return MTB_OK;
}

void mtb_index_close(mtb_index *ix) {
    if (!ix) return;
    hipError_t e = hipSuccess;
    for (int k = 0; k < 4; k++) if (ix->ipc_stage[k]) { e = hipFree(ix->ipc_stage[k]); ix->ipc_stage[k] = nullptr; }
    if (ix->parent) {                /* a view: the parent may be packed again once the last view is gone */
        { std::lock_guard<std::mutex> lk(ix->parent->state_mu); ix->parent->views--; }
        if (ix->d_dir) e = hipFree(ix->d_dir);
        if (ix->d_dirbase) e = hipFree(ix->d_dirbase);
        (void)e;
        delete ix; return;
    }
    if (!ix->own && ix->packed && ix->d_values) {
        /* a borrowed target array (mtb_index_from_device) is handed back the way it was lent: flat.  A sealed index has let go of
         * info[] (the lender was told so and may have freed it): only the values are restored then. */
        std::unique_lock<std::mutex> lk(ix->state_mu);
        ix->state_cv.wait(lk, [&] { return ix->users == 0; });
        if (hipSetDevice(ix->ctx->device) == hipSuccess) {
            hipLaunchKernelGGL(k_index_unpack, dim3((uint32_t)std::min<uint64_t>(((uint64_t)ix->dir_buckets + 255) / 256, 1u << 20)), dim3(256), 0, ix->ctx->stream,
                               ix->d_values, ix->d_info, dir_view(ix));
            e = hipStreamSynchronize(ix->ctx->stream);
        }
        ix->packed = false;
    }
    if (ix->own) { if (ix->d_values) e = hipFree(ix->d_values); if (ix->d_info) e = hipFree(ix->d_info); }
    else if (ix->info_owned && ix->d_info) e = hipFree(ix->d_info);
    if (ix->d_dir) e = hipFree(ix->d_dir);
    if (ix->d_dirbase) e = hipFree(ix->d_dirbase);
    if (ix->d_canon) e = hipFree(ix->d_canon);
    if (ix->d_parent) e = hipFree(ix->d_parent);
    if (ix->d_depth) e = hipFree(ix->d_depth);
    if (ix->d_spparent) e = hipFree(ix->d_spparent);
    if (ix->d_tax2species) e = hipFree(ix->d_tax2species);
    if (ix->d_under) e = hipFree(ix->d_under);
    if (ix->d_accleaf) e = hipFree(ix->d_accleaf);
    if (ix->d_node) e = hipFree(ix->d_node);
    if (ix->d_cov_bits) e = hipFree(ix->d_cov_bits);
    if (ix->d_cov_hits) e = hipFree(ix->d_cov_hits);
    (void)e;
    delete ix;
}
uint64_t mtb_index_num_targets(const mtb_index *ix) { return ix ? ix->T : 0; }
mtb_status mtb_index_open_stats(const mtb_index *ix, uint64_t *out4) {
    if (!ix || !out4) return fail(MTB_ERR_ARG, "NULL argument");
    out4[0] = ix->open_chunks; out4[1] = ix->open_chunk_words; out4[2] = ix->open_peak_bytes; out4[3] = (ix->packed && !ix->d_info) ? 1 : 0;
    return MTB_OK;
}
mtb_status mtb_index_state(const mtb_index *ix, int32_t *dir_depth, int32_t *packed, int32_t *sealed) {
    if (!ix) return fail(MTB_ERR_ARG, "NULL index");
    const mtb_index *o = ix->parent ? ix->parent : ix;
    if (dir_depth) *dir_depth = ix->d_dir ? ix->dir_L : 0;
    if (packed) *packed = o->packed ? 1 : 0;
    if (sealed) *sealed = (o->packed && !o->d_info) ? 1 : 0;
    return MTB_OK;
}

mtb_status mtb_index_seal(mtb_index *ix) {
    if (!ix) return fail(MTB_ERR_ARG, "NULL index");
    mtb_ctx *c = ix->ctx;
    HIPCHK(hipSetDevice(c->device));
    if (!ix->d_dir || ix->dir_L != 7 || !ix->own_tax) return fail(MTB_ERR_UNSUPPORTED, "index has no depth-7 directory (too small, or a view): nothing to seal");
    std::unique_lock<std::mutex> lk(ix->state_mu);
    ix->state_cv.wait(lk, [&] { return ix->users == 0; });
    if (ix->views) return fail(MTB_ERR_UNSUPPORTED, "index has live views (mtb_index_slice): close them before sealing");
    STCHK(ensure_packed_locked(ix));
    if (!ix->packed) return fail(MTB_ERR_UNSUPPORTED, "packing is disabled");
    if (ix->d_info && (ix->own || ix->info_owned)) { hipError_t e = hipFree(ix->d_info); (void)e; }
    ix->d_info = nullptr; ix->info_owned = false;       /* a borrowed info[] now belongs to the caller alone */
    return MTB_OK;
}

mtb_status mtb_index_download(mtb_index *ix, uint64_t *values, uint32_t *info, uint64_t cap) {
    if (!ix) return fail(MTB_ERR_ARG, "NULL index");
    if (cap < ix->T) return fail(MTB_ERR_CAPACITY, "output too small");
    if (ix->T == 0) return MTB_OK;
    STCHK(ensure_flat(ix));
    if (values) HIPCHK(hipMemcpy(values, ix->d_values, ix->T * 8, hipMemcpyDeviceToHost));
    if (info) HIPCHK(hipMemcpy(info, ix->d_info, ix->T * 4, hipMemcpyDeviceToHost));
    return MTB_OK;
}
} // extern "C"

/* IndexCreator::writeTargetFilesAndSplits + writeDbParameters (IndexCreator.cpp:817-892, 1251-1272) and the taxID_list dump (:329-333)
 * for entries that are resident on the device -- all at once (mtb_index_write) or one value range after another (mtb_merge_databases:
 * mergeTargetFiles<DB_CREATION>, IndexCreator.h:323-472, streams its output the same way).  append(): the delta coder runs on the
 * device, a slice of targets at a time (words per entry -> exclusive scan -> every entry writes its 15-bit groups at its offset; the
 * first entry of an append is coded against the last value written before it), the coded slice and its info entries cross PCIe into
 * pinned buffers and a writer thread appends them to the files while the next slice is coded; the taxID_list map accumulates.
 * finish(): the split checkpoints -- armed at every size_of_split-th entry, recorded at the first later entry of another amino-acid
 * part -- need n, which only the end knows: every slice left the range of the files it became (its own checkpoint: the value
 * before it), and the slices that hold an arming are looked at again -- in the caller's array if it is still resident, else re-decoded
 * from the diffIdx just written, as exactly that range (decode_chunked).  An arming still pending at a slice's end is resolved in the next slice.
 * db.parameters is removed first and written last: a directory whose write failed cannot be opened as a database. */
struct IndexWriter {
    mtb_ctx *c = nullptr; std::string d; int fd = -1, fi = -1; int32_t max_id = 0; mtb_params params;
    uint64_t SLICE = 0, n = 0, diff_count = 0, last_value = 0;
    std::vector<mtbhost::MergeSlice> slices;        /* a written slice's m entries are the range's coded ones; it leads with the entry before them (none before entry 0) */
    const uint64_t *resident = nullptr;          /* the one appended array, if it stays on the device until finish() (mtb_index_write) */
    uint32_t *d_nw = nullptr; uint64_t *d_off = nullptr; uint16_t *d_enc = nullptr; uint8_t *d_seen = nullptr; int32_t *d_extra = nullptr; uint32_t *d_nextra = nullptr;
    void *pin_e[2] = {nullptr, nullptr}, *pin_i[2] = {nullptr, nullptr};
    std::thread writers[2]; std::atomic<bool> write_ok{true}; int cur = 0; bool begun = false;
    static constexpr uint32_t EXTRA_CAP = 1u << 20;
    void join() { for (int k = 0; k < 2; k++) if (writers[k].joinable()) writers[k].join(); }
    ~IndexWriter() {
        join();
        if (fd >= 0) close(fd);
        if (fi >= 0) close(fi);
        for (int k = 0; k < 2; k++) { if (pin_e[k]) { hipError_t x = hipHostFree(pin_e[k]); (void)x; } if (pin_i[k]) { hipError_t x = hipHostFree(pin_i[k]); (void)x; } }
        if (begun) { release(c, "wnw"); release(c, "woff"); release(c, "wenc"); release(c, "wseen"); release(c, "wextra"); }
    }
    /* slice_entries: the most entries one append will bring, if that is fewer than a slice of 2^25 (sizes the buffers of small databases) */
    mtb_status begin(mtb_ctx *ctx, const char *dbdir, int32_t tax_max_id, const mtb_params &p, uint64_t slice_entries) {
        c = ctx; d = dbdir; max_id = tax_max_id; params = p;
        unlink((d + "/db.parameters").c_str());
        fd = open((d + "/diffIdx").c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644); fi = open((d + "/info").c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
        if (fd < 0 || fi < 0) return fail(MTB_ERR_IO, "cannot create diffIdx/info in " + d);
        SLICE = std::min<uint64_t>(1ull << 25, std::max<uint64_t>(slice_entries, 1));
        begun = true;
        STCHK(ensure(c, "wnw", SLICE, &d_nw)); STCHK(ensure(c, "woff", SLICE + 1, &d_off));
        STCHK(ensure(c, "wenc", SLICE * 5, &d_enc)); STCHK(ensure(c, "wseen", (size_t)max_id + 2, &d_seen));
        STCHK(ensure(c, "wextra", EXTRA_CAP + 1, &d_extra)); d_nextra = (uint32_t *)(d_extra + EXTRA_CAP);
        HIPCHK(hipMemsetAsync(d_seen, 0, (size_t)max_id + 2, c->stream)); HIPCHK(hipMemsetAsync(d_nextra, 0, 4, c->stream));
        for (int k = 0; k < 2; k++)
            if (hipHostMalloc(&pin_e[k], SLICE * 10, hipHostMallocDefault) != hipSuccess || hipHostMalloc(&pin_i[k], SLICE * 4, hipHostMallocDefault) != hipSuccess) {
                (void)hipGetLastError(); return fail(MTB_ERR_OOM, "no pinned host memory for the index download"); }
        return MTB_OK;
    }
    /* m entries (device arrays), all above what was appended before */
    mtb_status append(const uint64_t *d_values, const uint32_t *d_info, uint64_t m) {
        hipStream_t st = c->stream;
        const uint64_t prev0 = last_value;
        uint64_t slice_prev = prev0;
        for (uint64_t s0 = 0; s0 < m; s0 += SLICE, cur ^= 1) {
            const uint64_t mm = std::min<uint64_t>(SLICE, m - s0);
            const dim3 grid((uint32_t)((mm + 255) / 256));
            uint64_t *d_ws;
            STCHK(ensure(c, "scanws", scan_ws_elems(SLICE + 1), &d_ws));
            hipLaunchKernelGGL(k_diff_nwords, grid, dim3(256), 0, st, d_values, s0, mm, prev0, d_nw);
            scan_launch<uint32_t, uint64_t, false>(st, d_nw, mm, true, d_off, d_ws);
            hipLaunchKernelGGL(k_diff_encode, grid, dim3(256), 0, st, d_values, s0, mm, prev0, (const uint64_t *)d_off, d_enc);
            hipLaunchKernelGGL(k_mark_taxids, grid, dim3(256), 0, st, d_info, s0, mm, d_seen, max_id, d_extra, EXTRA_CAP, d_nextra);
            HIPCHK(hipGetLastError());
            uint64_t words = 0, slice_last = 0;
            STCHK(d2h(c, &words, d_off + mm, 8));
            STCHK(d2h(c, &slice_last, d_values + s0 + mm - 1, 8));
            {   mtbhost::MergeSlice r;
                r.lead = n + s0 ? 1 : 0; r.first_value = slice_prev; r.diff_lo = diff_count; r.diff_hi = diff_count + words; r.info_lo = n + s0 - r.lead; r.info_hi = n + s0 + mm;
                slices.push_back(r); }
            slice_prev = slice_last;
            if (writers[cur].joinable()) writers[cur].join();  /* (two slices back: its buffers are `cur`'s) */
            if (!write_ok) return fail(MTB_ERR_IO, "short write while writing " + d);
            HIPCHK(hipMemcpyAsync(pin_e[cur], d_enc, words * 2, hipMemcpyDeviceToHost, st));          /* while the previous slice is being written from the other pair */
            HIPCHK(hipMemcpyAsync(pin_i[cur], d_info + s0, mm * 4, hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            if (writers[cur ^ 1].joinable()) writers[cur ^ 1].join();          /* file order */
            if (!write_ok) return fail(MTB_ERR_IO, "short write while writing " + d);
            const void *pe = pin_e[cur], *pi = pin_i[cur];
            const uint64_t at_d = diff_count * 2, at_i = (n + s0) * 4;
            std::atomic<bool> *ok = &write_ok; const int wfd = fd, wfi = fi;
            /* several pwrite streams per file: one stream into the page cache tops out near 2-3 GB/s, a 16 G-target database is 150 GB */
            writers[cur] = std::thread([ok, wfd, wfi, pe, pi, words, mm, at_d, at_i] {
                bool ok_i = true;
                std::thread ti([&] { ok_i = pwrite_parallel(wfi, pi, at_i, mm * 4, 6); });
                const bool ok_d = pwrite_parallel(wfd, pe, at_d, words * 2, 10);
                ti.join();
                if (!ok_d || !ok_i) *ok = false;
            });
            diff_count += words;
        }
        n += m; last_value = slice_prev;
        return MTB_OK;
    }
    /* the checkpoints: j[k] for every arming position k * size_of_split - 1; equal neighbours are one checkpoint (an arming inside a
     * run that is still armed changes nothing); at most split_num - 1 are kept */
    mtb_status find_splits(int split_num, std::vector<mtbhost::MergeCheckpoint> *splits) {
        hipStream_t st = c->stream;
        const uint64_t size_of_split = n / (uint64_t)(split_num - 1);
        if (!size_of_split || !n) return MTB_OK;
        const uint64_t n_k = std::min<uint64_t>(n / size_of_split, 1u << 24);
        size_t n_cp = 0; uint64_t last_j = UINT64_MAX; bool pending = false;
        std::vector<uint64_t> armed, hj, cpj, cpv, cpo;
        struct Scratch { mtb_ctx *c; ~Scratch() { release(c, "wdecv"); release(c, "wdeci"); release(c, "wsplitj"); release(c, "wcp"); } } scratch{c};
        DecodeScratch decode_scratch{c};
        for (size_t r = 0; r < slices.size() && n_cp + 1 < (size_t)split_num; r++) {
            const mtbhost::MergeSlice &R = slices[r];
            const uint64_t e = R.info_lo + R.lead, m = R.coded_entries(), end = R.info_hi, prev = R.first_value;
            armed.clear();
            if (pending) armed.push_back(e - 1);                    /* still armed at the previous slice's last entry: every entry since the arming shares its amino-acid part */
            pending = false;
            const uint64_t k_lo = std::max<uint64_t>(1, (e + 1 + size_of_split - 1) / size_of_split), k_hi = std::min<uint64_t>(n_k, end / size_of_split);
            for (uint64_t k = k_lo; k <= k_hi; k++) armed.push_back(k * size_of_split - 1);
            if (armed.empty()) continue;
            const uint64_t *vg = resident;                            /* indexed by the entry's number in the whole output */
            if (!vg) {
                uint64_t *dv; uint32_t *di;
                STCHK(ensure(c, "wdecv", m + 2, &dv)); STCHK(ensure(c, "wdeci", m + 2, &di));
                STCHK(decode_chunked(c, params.kmer_format, d, R, dv, di));
                vg = dv - R.info_lo;
            }
            const uint32_t na = (uint32_t)armed.size();
            uint64_t *d_j, *d_ws, *d_cp;
            STCHK(ensure(c, "wsplitj", 2 * (size_t)na, &d_j));
            STCHK(h2d(c, d_j, armed.data(), (size_t)na * 8));
            hipLaunchKernelGGL(k_split_find_win, dim3((na + 255) / 256), dim3(256), 0, st, vg, end, n, (const uint64_t *)d_j, na, d_j + na);
            HIPCHK(hipGetLastError());
            hj.resize(na);
            STCHK(d2h(c, hj.data(), d_j + na, (size_t)na * 8));
            cpj.clear();
            for (uint32_t t = 0; t < na && n_cp + cpj.size() + 1 < (size_t)split_num; t++) {
                if (hj[t] == UINT64_MAX) { pending = true; break; }
                if (hj[t] < n && hj[t] != last_j) { cpj.push_back(hj[t]); last_j = hj[t]; }
            }
            if (cpj.empty()) continue;
            /* value and word offset BEHIND each checkpoint's entry: the slice's words per entry, scanned again */
            const uint32_t q = (uint32_t)cpj.size();
            STCHK(ensure(c, "wcp", 3 * (size_t)q, &d_cp));
            STCHK(ensure(c, "scanws", scan_ws_elems(SLICE + 1), &d_ws));
            STCHK(h2d(c, d_cp, cpj.data(), (size_t)q * 8));
            hipLaunchKernelGGL(k_diff_nwords, dim3((uint32_t)((m + 255) / 256)), dim3(256), 0, st, vg, e, m, prev, d_nw);
            scan_launch<uint32_t, uint64_t, false>(st, d_nw, m, true, d_off, d_ws);
            hipLaunchKernelGGL(k_split_gather, dim3((q + 63) / 64), dim3(64), 0, st, vg, (const uint64_t *)d_off, e, (const uint64_t *)d_cp, q, d_cp + q, d_cp + 2 * (size_t)q);
            HIPCHK(hipGetLastError());
            cpv.resize(q); cpo.resize(q);
            STCHK(d2h(c, cpv.data(), d_cp + q, (size_t)q * 8)); STCHK(d2h(c, cpo.data(), d_cp + 2 * (size_t)q, (size_t)q * 8));
            for (uint32_t t = 0; t < q; t++) (*splits)[++n_cp] = mtbhost::MergeCheckpoint{cpv[t], R.diff_lo + cpo[t], cpj[t] + 1};
        }
        return MTB_OK;
    }
    mtb_status finish(int split_num) {
        join();
        if (!write_ok) return fail(MTB_ERR_IO, "short write while writing " + d);
        std::vector<mtbhost::MergeCheckpoint> splits((size_t)split_num, mtbhost::MergeCheckpoint{0, 0, 0});
        STCHK(find_splits(split_num, &splits));
        std::vector<uint8_t> seen((size_t)max_id + 2, 0);
        STCHK(d2h(c, seen.data(), d_seen, seen.size()));
        uint32_t n_extra = 0;
        STCHK(d2h(c, &n_extra, d_nextra, 4));
        if (n_extra > EXTRA_CAP) return fail(MTB_ERR_UNSUPPORTED, "more than 2^20 info entries outside the taxonomy's id range");
        std::vector<int32_t> extra_ids(n_extra);           /* ids outside the taxonomy's range (kept for taxID_list) */
        if (n_extra) STCHK(d2h(c, extra_ids.data(), d_extra, (size_t)n_extra * 4));
        FILE *f = fopen((d + "/split").c_str(), "wb"); if (!f) return fail(MTB_ERR_IO, "cannot create " + d + "/split");
        fwrite(splits.data(), sizeof(mtbhost::MergeCheckpoint), splits.size(), f); fclose(f);
        std::sort(extra_ids.begin(), extra_ids.end()); extra_ids.erase(std::unique(extra_ids.begin(), extra_ids.end()), extra_ids.end());
        f = fopen((d + "/taxID_list").c_str(), "w"); if (!f) return fail(MTB_ERR_IO, "cannot create " + d + "/taxID_list");
        {   size_t e = 0;
            for (size_t t = 0; t < seen.size(); t++) {
                while (e < extra_ids.size() && extra_ids[e] < (int32_t)t) fprintf(f, "%d\n", extra_ids[e++]);
                if (seen[t]) fprintf(f, "%zu\n", t);
            }
            while (e < extra_ids.size()) fprintf(f, "%d\n", extra_ids[e++]);
        }
        fclose(f);
        if (close(fd) != 0 || close(fi) != 0) { fd = fi = -1; return fail(MTB_ERR_IO, "cannot close diffIdx/info in " + d); }
        fd = fi = -1;
        f = fopen((d + "/db.parameters").c_str(), "w"); if (!f) return fail(MTB_ERR_IO, "cannot create " + d + "/db.parameters");
        const mtb_params &p = params;
        fprintf(f, "DB_name\t%s\nCreation_date\t-\nReduced_alphabet\t0\nAccession_level\t%d\n", "mtb", p.accession_level == 2 ? 1 : 0);
        fprintf(f, "Mask_mode\t0\nMask_prob\t0.900000\nSkip_redundancy\t%d\nSyncmer\t%d\n", p.skip_redundancy ? 1 : 0, p.syncmer);
        if (p.syncmer == 1) fprintf(f, "Syncmer_len\t%d\n", p.smer_len);
        fprintf(f, "Kmer_format\t%d\n", p.kmer_format);
        fclose(f);
        return MTB_OK;
    }
};

extern "C" {

mtb_status mtb_index_write(const mtb_index *cix, const char *dbdir, int split_num) {
    if (!cix || !dbdir || split_num < 2) return fail(MTB_ERR_ARG, "NULL argument / split_num < 2");
    mtb_index *ix = const_cast<mtb_index *>(cix);
    mtb_ctx *c = ix->ctx;
    HIPCHK(hipSetDevice(c->device));
    STCHK(ensure_flat(ix));
    IndexWriter w;
    STCHK(w.begin(c, dbdir, ix->tax.max_id, ix->params, ix->T));
    STCHK(w.append(ix->d_values, ix->d_info, ix->T));
    w.resident = ix->d_values;
    return w.finish(split_num);
}

int32_t mtb_tax_lca(const mtb_index *ix, int32_t a, int32_t b) { return ix->tax.lca(a, b); }
int32_t mtb_tax_species(const mtb_index *ix, int32_t t) { return (t >= 0 && t <= ix->tax.max_id) ? ix->tax.tax2species[(size_t)t] : 0; }
int32_t mtb_tax_parent(const mtb_index *ix, int32_t t) { int32_t c = ix->tax.cn(t); return c < 0 ? -1 : ix->tax.parent[(size_t)c]; }
int32_t mtb_tax_max_id(const mtb_index *ix) { return ix->tax.max_id; }
int32_t mtb_tax_original_id(const mtb_index *ix, int32_t t) { return (t >= 0 && t <= ix->tax.max_id) ? ix->tax.orig[(size_t)t] : t; }
int32_t mtb_tax_num_children(const mtb_index *ix, int32_t t) { int32_t c = ix->tax.cn(t); return c < 0 ? 0 : (int32_t)ix->tax.children_of(c).size(); }
int32_t mtb_tax_child(const mtb_index *ix, int32_t t, int32_t k) {
    int32_t c = ix->tax.cn(t); if (c < 0) return -1;
    const std::vector<int32_t> &v = ix->tax.children_of(c);
    return (k >= 0 && (size_t)k < v.size()) ? v[(size_t)k] : -1;
}
const char *mtb_tax_rank(const mtb_index *ix, int32_t t) { int32_t c = ix->tax.cn(t); return c < 0 ? "" : ix->tax.rank[(size_t)c].c_str(); }
const char *mtb_tax_name(const mtb_index *ix, int32_t t) { int32_t c = ix->tax.cn(t); return c < 0 ? "" : ix->tax.name[(size_t)c].c_str(); }

/* ------------------------------------------------------------------ */
/* stage-level entry points (host buffers)                             */
/* ------------------------------------------------------------------ */
static mtb_status upload_reads(mtb_ctx *c, const mtb_params *p, const char *bases, const uint64_t *offs, const char *bases2,
                               const uint64_t *offs2, uint64_t n_reads, char **d_b, uint64_t **d_o, char **d_b2, uint64_t **d_o2,
                               uint64_t *n_bases) {
    *d_b = nullptr; *d_o = nullptr; *d_b2 = nullptr; *d_o2 = nullptr; *n_bases = 0;
    if (n_reads == 0) return MTB_OK;
    if (!bases || !offs) return fail(MTB_ERR_ARG, "bases/offs NULL");
    uint64_t nb = offs[n_reads];
    STCHK(ensure(c, "bases", nb + 8, d_b, BUF_IO)); STCHK(ensure(c, "offs", n_reads + 1, d_o, BUF_IO));
    STCHK(h2d(c, *d_b, bases, nb)); STCHK(h2d(c, *d_o, offs, (n_reads + 1) * 8));
    *n_bases = nb;
    if (p->seq_mode == 2) {
        if (!bases2 || !offs2) return fail(MTB_ERR_ARG, "seq_mode 2 needs bases2/offs2");
        uint64_t nb2 = offs2[n_reads];
        STCHK(ensure(c, "bases2", nb2 + 8, d_b2, BUF_IO)); STCHK(ensure(c, "offs2", n_reads + 1, d_o2, BUF_IO));
        STCHK(h2d(c, *d_b2, bases2, nb2)); STCHK(h2d(c, *d_o2, offs2, (n_reads + 1) * 8));
        *n_bases += nb2;
    }
    return MTB_OK;
}

mtb_status mtb_extract(mtb_ctx *c, const mtb_params *p, const char *bases, const uint64_t *offs, const char *bases2, const uint64_t *offs2,
                       uint64_t n_reads, mtb_kmer *out, uint64_t cap, uint64_t *count, int32_t *qlen, int32_t *qlen2) {
    if (!c || !p || !count) return fail(MTB_ERR_ARG, "NULL argument");
    HIPCHK(hipSetDevice(c->device));
    *count = 0;
    if (n_reads == 0) return MTB_OK;
    char *d_b, *d_b2; uint64_t *d_o, *d_o2; uint64_t nb;
    STCHK(upload_reads(c, p, bases, offs, bases2, offs2, n_reads, &d_b, &d_o, &d_b2, &d_o2, &nb));
    int32_t *d_ql, *d_ql2;
    STCHK(ensure(c, "qlen", n_reads, &d_ql)); STCHK(ensure(c, "qlen2", n_reads, &d_ql2));
    ExtractOpts two_pass; two_pass.want_max_len = false;       /* the reference's emission order; nobody asks for the longest read */
    Extracted ex;
    STCHK(dev_extract(c, p, Reads{d_b, d_o, d_b2, d_o2, n_reads}, d_ql, d_ql2, two_pass, &ex));
    const uint64_t n = *count = ex.nk;
    if (qlen) STCHK(d2h(c, qlen, d_ql, n_reads * 4));
    if (qlen2) STCHK(d2h(c, qlen2, d_ql2, n_reads * 4));
    if (n > cap) return fail(MTB_ERR_CAPACITY, "k-mer buffer too small");
    if (n) STCHK(d2h(c, out, ex.d_k, n * sizeof(mtb_kmer)));
    return MTB_OK;
}

mtb_status mtb_sort_kmers(mtb_ctx *c, mtb_kmer *kmers, uint64_t n) {
    if (!c) return fail(MTB_ERR_ARG, "NULL ctx");
    HIPCHK(hipSetDevice(c->device));
    if (n == 0) return MTB_OK;
    if (n >= (1ull << 32)) return fail(MTB_ERR_ARG, "n must be < 2^32");
    mtb_kmer *d_a, *d_s;
    STCHK(ensure(c, "kmersA", n, &d_a));
    STCHK(h2d(c, d_a, kmers, n * sizeof(mtb_kmer)));
    STCHK(dev_sort(c, d_a, n, /* every bit */ 0, &d_s, /* binary passes: no digit array, no letter pairs */ nullptr, 0));
    STCHK(d2h(c, kmers, d_s, n * sizeof(mtb_kmer)));
    return MTB_OK;
}

mtb_status mtb_match_kmers(mtb_ctx *c, mtb_index *ix, const mtb_kmer *sorted, uint64_t n, mtb_match *out, uint64_t cap, uint64_t *count) {
    if (!c || !ix || !count) return fail(MTB_ERR_ARG, "NULL argument");
    HIPCHK(hipSetDevice(c->device));
    *count = 0;
    if (n == 0) return MTB_OK;
    mtb_kmer *d_q; mtb_match *d_m;
    STCHK(ensure(c, "kmersA", n, &d_q));
    STCHK(h2d(c, d_q, sorted, n * sizeof(mtb_kmer)));
    STCHK(ensure(c, "jtemp", cap, &d_m));
    mtb_status st = dev_join(c, ix, d_q, n, MatchList{d_m, cap}, count, /* no slot segments */ nullptr, /* sorted on every bit above */ 32);
    if (st != MTB_OK) return st;
    if (*count) STCHK(d2h(c, out, d_m, *count * sizeof(mtb_match)));
    return MTB_OK;
}

mtb_status mtb_sort_matches(mtb_ctx *c, mtb_match *matches, uint64_t n, uint64_t n_reads) {
    if (!c) return fail(MTB_ERR_ARG, "NULL ctx");
    HIPCHK(hipSetDevice(c->device));
    if (n == 0 || n_reads == 0) return MTB_OK;
    mtb_match *d_in, *d_out; uint32_t *d_rc; uint64_t *d_seg;
    STCHK(ensure(c, "jtemp", n, &d_in)); STCHK(ensure(c, "matches", n, &d_out)); STCHK(ensure(c, "readcnt", n_reads, &d_rc));
    STCHK(h2d(c, d_in, matches, n * sizeof(mtb_match)));
    STCHK(count_reads(c, d_in, n, n_reads, d_rc));
    STCHK(dev_regroup(c, d_in, n, n_reads, d_rc, &d_seg, d_out));
    STCHK(dev_segsort(c, d_out, d_seg, n_reads, nullptr));
    STCHK(d2h(c, matches, d_out, n * sizeof(mtb_match)));
    return MTB_OK;
}

mtb_status mtb_score(mtb_ctx *c, mtb_index *ix, const mtb_params *p, const mtb_match *sorted, uint64_t n_matches, uint64_t n_reads,
                     const int32_t *qlen, const int32_t *qlen2, mtb_result *results, int32_t *taxcnt_tax, uint32_t *taxcnt_cnt,
                     uint64_t taxcnt_cap, uint64_t *n_taxcnt) {
    if (!c || !ix || !p || !qlen || !results || !n_taxcnt) return fail(MTB_ERR_ARG, "NULL argument");
    HIPCHK(hipSetDevice(c->device));
    *n_taxcnt = 0;
    if (n_reads == 0) return MTB_OK;
    mtb_match *d_m; uint32_t *d_rc; uint64_t *d_seg; uint64_t *d_ws; int32_t *d_ql, *d_ql2;
    STCHK(ensure(c, "matches", n_matches, &d_m)); STCHK(ensure(c, "readcnt", n_reads, &d_rc));
    STCHK(ensure(c, "segstart", n_reads + 1, &d_seg)); STCHK(ensure(c, "scanws", scan_ws_elems(n_reads + 1), &d_ws));
    STCHK(ensure(c, "qlen", n_reads, &d_ql)); STCHK(ensure(c, "qlen2", n_reads, &d_ql2));
    STCHK(h2d(c, d_m, sorted, n_matches * sizeof(mtb_match)));
    STCHK(h2d(c, d_ql, qlen, n_reads * 4));
    if (qlen2) STCHK(h2d(c, d_ql2, qlen2, n_reads * 4)); else HIPCHK(hipMemsetAsync(d_ql2, 0, n_reads * 4, c->stream));
    STCHK(count_reads(c, d_m, n_matches, n_reads, d_rc));
    scan_launch<uint32_t, uint64_t, false>(c->stream, d_rc, n_reads, true, d_seg, d_ws);
    /* maxima for slab sizing */
    std::vector<uint32_t> rc(n_reads);
    STCHK(d2h(c, rc.data(), d_rc, n_reads * 4));
    uint32_t max_seg = 0, max_len = 0;
    for (uint64_t i = 0; i < n_reads; i++) { max_seg = std::max(max_seg, rc[i]); max_len = std::max<uint32_t>(max_len, (uint32_t)(qlen[i] + (qlen2 ? qlen2[i] : 0))); }
    mtb_result *d_res; int32_t *d_tt; uint32_t *d_tc;
    STCHK(ensure(c, res_name(RES_ROWS, 0), n_reads, &d_res, BUF_IO)); STCHK(ensure(c, "tctax", taxcnt_cap, &d_tt, BUF_IO)); STCHK(ensure(c, "tccnt", taxcnt_cap, &d_tc, BUF_IO));
    ScoreSrc src; src.m = d_m; src.seg = d_seg; src.sort = false; src.max_seg = max_seg;
    const ReadLens lens{d_ql, d_ql2, max_len};
    const ResultSink out{d_res, d_tt, d_tc, taxcnt_cap, /* tc_base */ 0};
    mtb_status st = (p->seq_mode == 3 && !c->opt.no_long_scorer)
        ? dev_score_long(c, ix, p, n_reads, lens, out, n_taxcnt, LongSegs{d_m, d_seg, max_seg})
        : dev_score(c, ix, p, n_reads, lens, out, n_taxcnt, src, /* nothing deferred */ nullptr);
    if (st != MTB_OK) return st;
    STCHK(d2h(c, results, d_res, n_reads * sizeof(mtb_result)));
    if (*n_taxcnt) { STCHK(d2h(c, taxcnt_tax, d_tt, *n_taxcnt * 4)); STCHK(d2h(c, taxcnt_cnt, d_tc, *n_taxcnt * 4)); }
    return MTB_OK;
}

/* ------------------------------------------------------------------ */
/* fused batch                                                         */
/* ------------------------------------------------------------------ */
} // extern "C"

/* Exact-segment tail of the pipeline: matches in join order (d_tmp, clobbered: it becomes the sort scratch) +
 * per-read counts -> scan, regroup, big segments sorted (chunk sort in LDS + rank merges), scoring.
 * Records ev[4] (regrouped) and ev[5] (sorted). */
static mtb_status score_join_order(mtb_ctx *c, mtb_index *ix, const mtb_params *p, mtb_match *d_tmp, uint64_t nm, uint64_t n_reads, uint32_t *d_rc,
                                   const ReadLens &lens, const ResultSink &out, uint64_t *n_taxcnt) {
    hipStream_t st = c->stream; mtb_match *d_m; uint64_t *d_seg;
    STCHK(ensure(c, "matches", nm, &d_m));
    STCHK(dev_regroup(c, d_tmp, nm, n_reads, d_rc, &d_seg, d_m));
    HIPCHK(hipEventRecord(c->ev[4], st));
    /* segments that fit LDS are sorted inside k_score; only the big ones are sorted here.  Long reads: k_score_long streams sorted
     * segments, so every segment of two or more matches is sorted here */
    const bool long_scorer = p->seq_mode == 3 && !c->opt.no_long_scorer;
    uint32_t max_seg = 0;
    {
        uint32_t *d_large;
        STCHK(ensure(c, "large", n_reads, &d_large));
        HIPCHK(scal_clear(c, SC_N_LARGE, 2));
        { KTimer kt(c, MTB_K_SEGSORT);
        hipLaunchKernelGGL(k_list_large, dim3((uint32_t)((n_reads + 255) / 256)), dim3(256), 0, st, (const uint64_t *)d_seg, n_reads,
                           long_scorer ? 1u : (uint32_t)MTB_SCORE_LDS, d_large, scal<uint32_t>(c, SC_N_LARGE), scal<uint32_t>(c, SC_MAX_SEG)); }
        uint64_t sc[2];
        STCHK(d2h(c, sc, scal<uint64_t>(c, SC_N_LARGE), 16));
        max_seg = (uint32_t)sc[1];
        if (sc[0]) {
            /* big segments: chunk sort in LDS + rank merges; the join-order buffer is the scratch */
            const size_t lds = (size_t)MTB_SEGLDS_CHUNK * 14;
            HIPCHK(hipFuncSetAttribute((const void *)k_segsort_lds<mtb_match>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            KTimer kt(c, MTB_K_SEGSORT);
            hipLaunchKernelGGL((k_segsort_lds<mtb_match>), dim3(std::min<uint32_t>((uint32_t)sc[0], 2048)), dim3(MTB_SEGLDS_THREADS), lds, st, d_m,
                               (const uint64_t *)d_seg, (const uint32_t *)d_large, scal<const uint32_t>(c, SC_N_LARGE), d_tmp);
        }
    }
    HIPCHK(hipEventRecord(c->ev[5], st));
    if (long_scorer) return dev_score_long(c, ix, p, n_reads, lens, out, n_taxcnt, LongSegs{d_m, d_seg, max_seg});
    ScoreSrc a; a.m = d_m; a.seg = d_seg; a.sort = true; a.max_seg = max_seg;
    return dev_score(c, ix, p, n_reads, lens, out, n_taxcnt, a, /* nothing deferred */ nullptr);
}

static void slot_geometry(const mtb_ctx *c, uint32_t max_q, uint32_t *direct, uint32_t *stride) {
    const uint32_t tail_min = c->opt.tail_min > 0 ? (uint32_t)std::max(8, c->opt.tail_min) & ~7u : 16u;      /* experiment switch: longer tails */
    *direct = std::max<uint32_t>(8, (max_q + 7) & ~7u);
    *stride = *direct + std::max<uint32_t>(tail_min, (*direct / 8 + 7) & ~7u);
}
/* The slot segments of a short-read batch: made once (make_slots), filled by the fused join or by k_slot_place, read by score_fixed_slots.
 * Live slots carry the batch's epoch tag; the buffer is cleared only when it is new or the tag wraps. */
struct SlotSegs {
    mtb_slot16 *d_segm = nullptr; uint32_t *d_rc = nullptr, stride = 0, direct = 0, epoch = 0;       /* n_reads x stride slots in buffer "segm"; per-read tail cursors */
    mtb_match *d_ovf = nullptr; uint64_t n_ovf = 0, ovf_region = 0;      /* the overflow list; ovf_region != 0: it is striped (dev_join) */
    const uint8_t *d_off_reads = nullptr; uint32_t max_len_off = 0;      /* reads routed around their slots (marked by the extractor); the longest of ALL reads then */
};
static mtb_status make_slots(mtb_ctx *c, uint64_t n_reads, uint32_t max_q, uint32_t *d_rc, SlotSegs *sl) {
    hipStream_t st = c->stream; *sl = SlotSegs(); sl->d_rc = d_rc;
    slot_geometry(c, max_q, &sl->direct, &sl->stride);
    STCHK(ensure_placed(c, "segm", n_reads * (uint64_t)sl->stride, &sl->d_segm));
    const DevBuf sb = buf_get(c, "segm");
    const char *clear_mode = c->opt.segm_clear[0] ? c->opt.segm_clear : nullptr;      /* experiment switch: kernel | sync | always (default: hipMemsetAsync when new / on epoch wrap) */
    const bool always = clear_mode && !strcmp(clear_mode, "always");
    /* cleared when the allocation is not the one this function cleared last (new, grown, or created by mtb_ctx_reserve: never
     * written by a clear), or when the tag wraps */
    if (sb.p != c->seg_clean_p || sb.cap != c->seg_clean_cap || c->seg_epoch == 0 || c->seg_epoch >= MTB_SLOT_EPOCHS || always) {
        if (clear_mode && !strcmp(clear_mode, "kernel")) hipLaunchKernelGGL(k_clear_words, dim3(2048), dim3(256), 0, st, (uint64_t *)sb.p, (uint64_t)(sb.cap / 8));
        else HIPCHK(hipMemsetAsync(sb.p, 0, sb.cap, st));
        if (clear_mode && !strcmp(clear_mode, "sync")) HIPCHK(hipDeviceSynchronize());
        c->seg_epoch = 0; c->seg_clean_p = sb.p; c->seg_clean_cap = sb.cap;
    }
    sl->epoch = ++c->seg_epoch;
    return MTB_OK;
}
/* capacity of the overflow list "ovf": what the buffer already holds or a 64th of the items that may overflow; after an attempt that reported n entries */
static uint64_t ovf_cap_first(mtb_ctx *c, uint64_t n_items) { return std::max<uint64_t>(buf_cap(c, "ovf") / sizeof(mtb_match), n_items / 64 + 4096); }
static uint64_t ovf_cap_regrown(uint64_t n) { return n + n / 16 + 1024; }

/* Scoring out of filled slot segments (fused path after the join; partitioned path after the matches came home): the
 * register-resident scorer, the generic one for the reads it flags, exact segments for the reads neither can take from their slots.
 * *nm_out = matches seen (statistics). */
static mtb_status score_fixed_slots(mtb_ctx *c, mtb_index *ix, const mtb_params *p, uint64_t n_reads, const ReadLens &lens, uint64_t nk_real, const SlotSegs &sl,
                                    const ResultSink &out, uint64_t *n_taxcnt, uint64_t *nm_out, bool may_overlap = true) {
    hipStream_t st = c->stream;
    uint64_t nm = 0;
    memset(c->many_stats, 0, sizeof(c->many_stats)); c->score_overlapped = 0;
    uint32_t *d_biglist, *d_bigcnt, *d_bigidx, *d_bigcur, *d_cnt; uint64_t *d_bigstart = nullptr, *d_ws2, *d_tot; mtb_match *d_big = nullptr;
    STCHK(ensure(c, "biglist", n_reads, &d_biglist)); STCHK(ensure(c, "bigidx", n_reads, &d_bigidx)); STCHK(ensure(c, "livecnt", n_reads, &d_cnt));
    STCHK(ensure(c, "segstart", n_reads + 1, &d_tot)); STCHK(ensure(c, "scanws", scan_ws_elems(n_reads + 1), &d_ws2));
    HIPCHK(hipMemsetAsync(d_cnt, 0, n_reads * 4, st));
    HIPCHK(scal_clear(c, SC_N_UNGROUPED, 3));            /* ..., SC_MAX_BIG_SEG, SC_N_DEFERRED */
    uint64_t big_total = 0;
    ScoreSrc a; a.m = (const mtb_match *)sl.d_segm; a.cursor = sl.d_rc;       /* slot mode: 16-byte slot records behind the pointer */ a.stride = sl.stride; a.direct = sl.direct; a.epoch = sl.epoch; a.sort = true; a.max_len_deferred = sl.max_len_off;
    /* LDS staging of the scorer = smallest instantiation that holds one match for every metamer of the longest read
     * (144 records: 16 waves per CU, 160: 14, 224: 10, 288: 8, 320: 7); reads with more live records are deferred */
    {   /* sized for the typical read (mean metamer count + 12 %), not the longest: the few reads beyond it take the deferred
           path, and 144 instead of 160 records is worth 10 % of the kernel on 150 bp reads (47.1 vs 52.3 ms) */
        const uint32_t want = std::min<uint32_t>(sl.direct, (uint32_t)((double)nk_real / (double)n_reads * 1.12) + 1);
        a.cap = want <= 144 ? 144 : want <= 160 ? 160 : want <= 224 ? 224 : want <= 288 ? 288 : 320;
    }
    a.max_seg = a.cap;
    a.big_list = d_biglist; a.n_big = scal<uint32_t>(c, SC_N_DEFERRED); a.cnt_out = d_cnt;
    /* ---- the deferred tier: the reads of conserved genes (kernels_score_many.h), scored straight from their slots + their overflow entries, dead
     * species dropped before anything is ordered; what k_score_many hands on goes through k_many_sort + k_score_long; what is left after both
     * takes the exact-segment path below.  Two lists come here:
     *   A  the reads whose tails overflowed, {r : cursor[r] > tail_cap} -- known from the join's cursors before any scorer runs (k_list_overflowed;
     *      k_score_fast flags exactly these 2 and touches nothing else of them), length in a word of its own (d_ms[MS_N_A]);
     *   B  the reads the generic slot kernel could not stage (d_biglist / SC_N_DEFERRED, appended to while that kernel runs).
     * `early` batches run the tier for A BESIDE k_score_fast on the context's side stream: the tier's kernels wait on memory with the VALUs
     * three quarters idle, k_score_fast is bound by VALU issue, the two sets of reads are disjoint and every output is per read.  The side
     * stream forks once the taxcnt layout exists, the compute stream is held until the tier's first scorer is queued (its few fat workgroups
     * must be resident before the flood of k_score_fast's thin ones), and joins before list B is looked at.  With profiling on (and in
     * -DMTB_SCORE_OVERLAP=0 builds) the same launches run on the compute stream in the same order: per-kernel times stay solo times.
     * Long reads never come here; the partitioned path (may_overlap = false), MTB_NO_FAST_SCORER, MTB_NO_FAST_PAIRS on pairs and strides beyond 384
     * keep the serial order of old -- k_score_fast, k_list_flag2, the generic kernel, then the tier over ONE list -- and MTB_NO_SCORE_MANY has no tier. ---- */
    const bool tiers = !c->opt.no_score_many && sl.stride <= 384u;
    const bool early = tiers && may_overlap && fast_scorer_applies(c, ix, p, lens, sl.stride);
    const bool overlap = early && MTB_SCORE_OVERLAP != 0 && !c->profiling && c->side_stream != nullptr;
    const bool have_ovf = sl.ovf_region ? c->ovf_max_region != 0 : sl.n_ovf != 0;
    const bool cap192 = c->opt.many_cap ? c->opt.many_cap <= 192 : sl.stride <= 192u;
    enum { MS_REST = 0, MS_WORK = 1, MS_STATS = 2, MS_LONG_WORK = 8, MS_N_FIN = 9, MS_N_A = 15, MS_RUN = 16 };      /* words of a run's block of d_ms; MS_N_FIN and MS_N_A: first block only */
    unsigned long long *d_ms = nullptr;          /* two blocks of MS_RUN words: the run over list A (or the only run), the run over list B */
    uint32_t *d_alist = nullptr, *d_rest[2] = {nullptr, nullptr}, *d_fin = nullptr, *d_novf = nullptr, *d_ocur = nullptr, *d_bc3 = nullptr, *d_segcnt = nullptr;
    uint64_t *d_ostart = nullptr, *d_bs3 = nullptr, *d_wss = d_ws2; uint8_t *d_todo = nullptr;
    mtb_match *d_ovfg = nullptr;                 /* the overflow list grouped by read, once the tier has built it */
    bool grouped = false, many_timed = false, sort_on = false;
    uint32_t n_a = 0, n_fin = 0, n_rest_all = 0;     /* reads of list A; reads no tier scored so far; reads k_score_many handed on so far */
    /* the tier's buffers.  Early batches ask for all of them before the fork, sized by the batch: an allocation synchronises the device.
     * (Not "manym", the handed-on reads' segments: its size is a read-back of the tier's.  It comes out of the join's dead buffers; a batch
     * that outgrows them allocates once, and that one batch's tier waits for k_score_fast.) */
    auto tier_buffers = [&](uint64_t n_sort) -> mtb_status {
        if (d_ms) return MTB_OK;
        STCHK(ensure(c, "manystat", 2 * MS_RUN, &d_ms)); STCHK(ensure(c, "restlist", n_reads, &d_rest[0])); STCHK(ensure(c, "restlist2", n_reads, &d_fin));
        if (early) { STCHK(ensure(c, "overflowed", n_reads, &d_alist)); STCHK(ensure(c, "restlistb", n_reads, &d_rest[1])); STCHK(ensure(c, "scanwsside", scan_ws_elems(n_reads + 1), &d_wss)); }
        if (have_ovf) {
            STCHK(ensure(c, "novf", n_reads, &d_novf)); STCHK(ensure(c, "ocur", n_reads, &d_ocur)); STCHK(ensure(c, "ovfstart", n_reads + 1, &d_ostart));
            STCHK(scratch(c, "ovfg", sl.n_ovf + 1, &d_ovfg));
        }
        STCHK(ensure(c, "bigcnt", n_sort, &d_bc3)); STCHK(ensure(c, "bigstart", n_sort + 1, &d_bs3)); STCHK(ensure(c, "bigseg", n_sort, &d_segcnt));
        STCHK(ensure(c, "todoflag", n_reads, &d_todo));
        HIPCHK(hipMemsetAsync(d_ms, 0, 2 * MS_RUN * 8, st));
        return MTB_OK;
    };
    /* the overflow list grouped by read (counts from the tail cursors); built once, by whichever run comes first */
    auto group_ovf = [&](hipStream_t sq) -> mtb_status {
        if (!have_ovf || grouped) return MTB_OK;
        grouped = true;
        HIPCHK(hipMemsetAsync(d_ocur, 0, n_reads * 4, sq));
        hipLaunchKernelGGL(k_ovf_count, dim3((uint32_t)((n_reads + 255) / 256)), dim3(256), 0, sq, (const uint32_t *)sl.d_rc, sl.d_off_reads, n_reads, sl.stride - sl.direct, d_novf);
        scan_launch<uint32_t, uint64_t, false>(sq, d_novf, n_reads, true, d_ostart, d_wss);
        if (sl.ovf_region) hipLaunchKernelGGL(k_ovf_group, dim3((uint32_t)((c->ovf_max_region + 255) / 256), MTB_OVF_STRIPES), dim3(256), 0, sq, (const mtb_match *)sl.d_ovf, sl.n_ovf,
                                           (const uint64_t *)d_ostart, (const uint32_t *)d_novf, d_ocur, d_ovfg, sl.ovf_region, (const unsigned long long *)c->d_ovfctr);
        else hipLaunchKernelGGL(k_ovf_group, dim3((uint32_t)((sl.n_ovf + 255) / 256)), dim3(256), 0, sq, (const mtb_match *)sl.d_ovf, sl.n_ovf,
                                (const uint64_t *)d_ostart, (const uint32_t *)d_novf, d_ocur, d_ovfg, (uint64_t)0, (const unsigned long long *)nullptr);
        return MTB_OK;
    };
    /* one run of the tier over a list whose length sits on the device.  run 0: list A (or the only list), run 1: list B behind it.
     * tier_begin queues k_score_many; tier_end reads its counters back (synchronising ONLY the run's stream), takes what it handed on
     * through k_many_sort + k_score_long and appends what is still unscored to the final list d_fin / d_ms[MS_N_FIN]. */
    auto tier_begin = [&](int run, hipStream_t sq, const uint32_t *d_list, const uint32_t *d_n, uint32_t grid, const ScoreLaunch &SL) -> mtb_status {
        unsigned long long *ms = d_ms + run * MS_RUN;
        sort_on = SL.key64 && !c->opt.no_many_sort;
        /* without the second tier kernels the hand-over list IS the final list: both runs append to the first one's */
        uint32_t *rest = sort_on ? d_rest[run] : d_rest[0]; uint32_t *n_rest = (uint32_t *)((sort_on ? ms : d_ms) + MS_REST);
#define MTB_LAUNCH_MANY(K64, CAPV) hipLaunchKernelGGL((k_score_many<K64, CAPV>), dim3(grid), dim3(64), 0, sq, (const mtb_slot16 *)sl.d_segm, sl.stride, sl.direct, sl.epoch, (const uint32_t *)sl.d_rc, sl.d_off_reads, \
        (const mtb_match *)d_ovfg, (const uint64_t *)d_ostart, d_list, d_n, SL.lens.d_ql, SL.lens.d_ql2, tax_view(ix), SL.sp, SL.d_tcoff, SL.out.d_res, \
        SL.out.d_tc_tax, SL.out.d_tc_cnt, SL.out.tc_cap, SL.out.tc_base, rest, n_rest, d_cnt, ms + MS_WORK, ms + MS_STATS)
        if (cap192) { if (SL.key64) MTB_LAUNCH_MANY(true, 192); else MTB_LAUNCH_MANY(false, 192); }
        else { if (SL.key64) MTB_LAUNCH_MANY(true, 320); else MTB_LAUNCH_MANY(false, 320); }
#undef MTB_LAUNCH_MANY
        HIPCHK(hipGetLastError());
        return MTB_OK;
    };
    auto tier_end = [&](int run, hipStream_t sq, uint32_t n_list, const ScoreLaunch &SL) -> mtb_status {
        unsigned long long *ms = d_ms + run * MS_RUN;
        uint64_t h[2 * MS_RUN];
        STCHK(d2h(c, h, d_ms, sizeof(h), sq));
        const uint64_t *hr = h + run * MS_RUN;
        if (run == 0 && early) n_list = n_a = (uint32_t)(h[MS_N_A] & 0xFFFFFFFFull);
        const uint32_t rest_seen = (uint32_t)((sort_on ? hr[MS_REST] : h[MS_REST]) & 0xFFFFFFFFull);
        const uint32_t n_rest = sort_on ? rest_seen : rest_seen - n_rest_all;
        n_rest_all += n_rest;
        c->many_stats[2] += hr[MS_STATS]; c->many_stats[3] += hr[MS_STATS + 1];
        if (c->opt.many_verbose) fprintf(stderr, "mtb: k_score_many: %u reads listed, %u handed on (routed off / buckets / counts %llu, species table full %llu, survivors beyond the staging %llu); %llu matches, %llu survive the dead-species drop\n",
                                                n_list, n_rest, (unsigned long long)hr[MS_STATS + 2], (unsigned long long)hr[MS_STATS + 3], (unsigned long long)hr[MS_STATS + 4], (unsigned long long)hr[MS_STATS], (unsigned long long)hr[MS_STATS + 1]);
        if (!sort_on) { n_fin = n_rest_all; return MTB_OK; }
        if (!n_rest) return MTB_OK;
        /* ---- reads beyond the staging (thousands of matches: conserved genes of organisms that are not in the index): a workgroup per
         * read gathers, drops dead species, sorts in LDS and writes the read's exact segment; k_score_long streams it ---- */
        const uint32_t *d_r = d_rest[run]; mtb_match *d_big3;
        if (!early) { STCHK(ensure(c, "bigcnt", n_rest, &d_bc3)); STCHK(ensure(c, "bigstart", (uint64_t)n_rest + 1, &d_bs3)); STCHK(ensure(c, "bigseg", n_rest, &d_segcnt)); }
        hipLaunchKernelGGL(k_big_count, dim3(std::min<uint32_t>(n_rest, 4096)), dim3(64), 0, sq, (const mtb_slot16 *)sl.d_segm, sl.stride, sl.direct, sl.epoch,
                           (const uint32_t *)sl.d_rc, d_r, n_rest, d_bc3, d_bigidx, scal<uint32_t>(c, SC_MAX_BIG_SEG), sl.d_off_reads);
        scan_launch<uint32_t, uint64_t, false>(sq, d_bc3, n_rest, true, d_bs3, d_wss);
        uint64_t total3 = 0;
        STCHK(d2h(c, &total3, d_bs3 + n_rest, 8, sq));
        STCHK(scratch(c, "manym", total3 + 1, &d_big3));
        HIPCHK(hipMemsetAsync(d_todo, 0, n_reads, sq));
        /* the small instantiation first (20 KB of LDS: eight workgroups per CU), the big one for the reads it flags 2 */
        hipLaunchKernelGGL((k_many_sort<11, 2048u>), dim3(std::min<uint32_t>(n_rest, 256u * 8u)), dim3(MTB_MSORT_NT), 0, sq, (const mtb_slot16 *)sl.d_segm, sl.stride, sl.direct, sl.epoch, (const uint32_t *)sl.d_rc, sl.d_off_reads,
                           (const mtb_match *)d_ovfg, (const uint64_t *)d_ostart, d_r, n_rest, SL.lens.d_ql, SL.lens.d_ql2, SL.sp.dna_shift, (const uint64_t *)d_bs3, d_big3, d_segcnt, d_todo, 0u, 2u);
        hipLaunchKernelGGL((k_many_sort<12, 4096u>), dim3(std::min<uint32_t>(n_rest, 256u * 3u)), dim3(MTB_MSORT_NT), 0, sq, (const mtb_slot16 *)sl.d_segm, sl.stride, sl.direct, sl.epoch, (const uint32_t *)sl.d_rc, sl.d_off_reads,
                           (const mtb_match *)d_ovfg, (const uint64_t *)d_ostart, d_r, n_rest, SL.lens.d_ql, SL.lens.d_ql2, SL.sp.dna_shift, (const uint64_t *)d_bs3, d_big3, d_segcnt, d_todo, 2u, 1u);
        hipLaunchKernelGGL((k_score_long<2048, 256, 256, 256>), dim3(std::min<uint32_t>(n_rest, 256u * 5u)), dim3(MTB_LONG_NT), 0, sq, (const mtb_match *)d_big3, (const uint64_t *)d_bs3, n_reads, SL.lens.d_ql, SL.lens.d_ql2,
                           tax_view(ix), SL.sp, SL.d_tcoff, SL.out.d_res, SL.out.d_tc_tax, SL.out.d_tc_cnt, SL.out.tc_cap, SL.out.tc_base, d_todo, ms + MS_LONG_WORK, (const uint32_t *)d_segcnt, d_r, n_rest);
        hipLaunchKernelGGL(k_list_flagged, dim3((n_rest + 255) / 256), dim3(256), 0, sq, d_r, n_rest, (const uint8_t *)d_todo, (const uint32_t *)d_bc3, d_fin, (uint32_t *)(d_ms + MS_N_FIN), d_cnt);
        HIPCHK(hipGetLastError());
        uint64_t left = 0;
        STCHK(d2h(c, &left, d_ms + MS_N_FIN, 8, sq));
        if (c->opt.many_verbose) fprintf(stderr, "mtb: k_many_sort + k_score_long: %u reads (%llu records), %llu in all left for the exact-segment path\n", n_rest, (unsigned long long)total3, (unsigned long long)(left & 0xFFFFFFFFull));
        n_fin = (uint32_t)(left & 0xFFFFFFFFull);
        return MTB_OK;
    };
    /* early batches: list A and its run of the tier, queued before the first scorer (dev_score calls this once the taxcnt layout exists) */
    ScoreFork fork = [&](const ScoreLaunch &SL) -> mtb_status {
        STCHK(tier_buffers(n_reads));
        hipStream_t ss = overlap ? c->side_stream : st;
        if (overlap) { HIPCHK(hipEventRecord(c->side_ev[0], st)); HIPCHK(hipStreamWaitEvent(ss, c->side_ev[0], 0)); }
        hipLaunchKernelGGL(k_list_overflowed, dim3((uint32_t)((n_reads + 255) / 256)), dim3(256), 0, ss, (const uint32_t *)sl.d_rc, n_reads, sl.stride - sl.direct, d_alist, (uint32_t *)(d_ms + MS_N_A));
        if (!overlap) {
            /* serial: the whole run here, and only if there is a list (the launch statistics count the tier once per batch that has deferred reads) */
            uint64_t na = 0;
            STCHK(d2h(c, &na, d_ms + MS_N_A, 8));
            n_a = (uint32_t)na;
            if (!n_a) return MTB_OK;
            KTimer ktm(c, MTB_K_SCORE_MANY); many_timed = true;
            STCHK(group_ovf(ss));
            STCHK(tier_begin(0, ss, d_alist, (const uint32_t *)(d_ms + MS_N_A), std::min<uint32_t>((uint32_t)na, 256u * (cap192 ? 12u : 7u)), SL));
            return tier_end(0, ss, (uint32_t)na, SL);
        }
        STCHK(group_ovf(ss));
        /* a fixed grid of a few workgroups per CU (k_score_many claims blocks of reads from a counter and needs no host-side count), and the
         * compute stream held until it is queued.  256 x 4 by measurement (2: +10.6 ms, 6 / 8 / 12: +0.35 / 0.65 / 1.0 ms): profiles/score_overlap_notes.md */
        HIPCHK(hipEventRecord(c->side_ev[1], ss));
        STCHK(tier_begin(0, ss, d_alist, (const uint32_t *)(d_ms + MS_N_A), 256u * MTB_SCORE_OVERLAP_GRID, SL));
        HIPCHK(hipStreamWaitEvent(st, c->side_ev[1], 0));
        c->score_overlapped = 1;
        return MTB_OK;
    };
    /* reads the first launches could not take from their slots: the tier for list B, then exact segments (live slots + overflow list), sorted in HBM */
    ScoreSecond second = [&](ScoreSrc *b, bool *go, const ScoreLaunch &SL) -> mtb_status {
        if (overlap) {        /* the side stream's part ends here; its read-backs wait for that stream alone */
            STCHK(tier_end(0, c->side_stream, 0, SL));
            HIPCHK(hipEventRecord(c->side_ev[2], c->side_stream)); HIPCHK(hipStreamWaitEvent(st, c->side_ev[2], 0));
        }
        uint64_t sc = 0;
        STCHK(d2h(c, &sc, scal<uint64_t>(c, SC_N_DEFERRED), 8));
        const uint32_t n_b = (uint32_t)sc;
        uint32_t n_big = n_a + n_b;
        *go = n_big != 0;
        if (!n_big) return MTB_OK;
        c->many_stats[0] = n_big; c->many_stats[1] = 0;
        if (tiers) {
            if (n_b) {
                /* list B (every deferred read where no list A was made).  Behind a timed run over A it is booked with the large-segment path */
                KTimer ktm(c, many_timed ? MTB_K_SEGSORT : MTB_K_SCORE_MANY);
                STCHK(tier_buffers(1));
                STCHK(group_ovf(st));
                const int run = early ? 1 : 0;
                STCHK(tier_begin(run, st, (const uint32_t *)d_biglist, scal<const uint32_t>(c, SC_N_DEFERRED), std::min<uint32_t>(n_b, 256u * (cap192 ? 12u : 7u)), SL));
                STCHK(tier_end(run, st, n_b, SL));
            }
            n_big = n_fin;
            c->many_stats[1] = c->many_stats[0] - n_big;
            *go = n_big != 0;
            if (!n_big) return MTB_OK;
            /* what is left goes the old way: the list of those reads, its length where the launches below read it */
            d_biglist = sort_on ? d_fin : d_rest[0];
            HIPCHK(hipMemcpyAsync(scal<uint64_t>(c, SC_N_DEFERRED), d_ms + (sort_on ? MS_N_FIN : MS_REST), 8, hipMemcpyDeviceToDevice, st));
        }
        KTimer kt(c, MTB_K_SEGSORT);
        HIPCHK(hipMemsetAsync(d_bigidx, 0xFF, n_reads * 4, st));        /* reads that are not listed (k_score_many took them) own entries of the overflow list too: k_big_ovf skips them */
        STCHK(ensure(c, "bigcnt", n_big, &d_bigcnt)); STCHK(ensure(c, "bigstart", (uint64_t)n_big + 1, &d_bigstart)); STCHK(ensure(c, "bigcur", n_big, &d_bigcur));
        hipLaunchKernelGGL(k_big_count, dim3(std::min<uint32_t>(n_big, 4096)), dim3(64), 0, st, (const mtb_slot16 *)sl.d_segm, sl.stride, sl.direct, sl.epoch,
                           (const uint32_t *)sl.d_rc, (const uint32_t *)d_biglist, n_big, d_bigcnt, d_bigidx, scal<uint32_t>(c, SC_MAX_BIG_SEG), sl.d_off_reads,
                           (const uint32_t *)(d_ovfg ? d_novf : nullptr), scal<unsigned long long>(c, SC_N_UNGROUPED));
        scan_launch<uint32_t, uint64_t, false>(st, d_bigcnt, n_big, true, d_bigstart, d_ws2);
        uint64_t mx = 0, n_ungrouped = 0;
        STCHK(d2h(c, &big_total, d_bigstart + n_big, 8));
        STCHK(d2h(c, &mx, scal<uint64_t>(c, SC_MAX_BIG_SEG), 8));
        STCHK(d2h(c, &n_ungrouped, scal<uint64_t>(c, SC_N_UNGROUPED), 8));
        STCHK(scratch(c, "bigm", big_total, &d_big));
        hipLaunchKernelGGL(k_big_copy, dim3(std::min<uint32_t>(n_big, 4096)), dim3(64), 0, st, (const mtb_slot16 *)sl.d_segm, sl.stride, sl.direct, sl.epoch,
                           (const uint32_t *)sl.d_rc, (const uint32_t *)d_biglist, (const uint64_t *)d_bigstart, n_big, d_bigcur, d_big,
                           (const mtb_match *)d_ovfg, (const uint64_t *)d_ostart, (const uint32_t *)(d_ovfg ? d_novf : nullptr));
        /* the pass over the whole overflow list: only for listed reads whose entries are not in the grouped list (all of them when there is none) */
        const uint32_t *skip_grouped = d_ovfg ? d_novf : nullptr;
        if (d_ovfg && n_ungrouped == 0) { /* every listed read's entries came from its group */ }
        else if (sl.ovf_region) {            /* striped list (the directory join's): every stripe's entries */
            if (c->ovf_max_region) hipLaunchKernelGGL(k_big_ovf, dim3((uint32_t)((c->ovf_max_region + 255) / 256), MTB_OVF_STRIPES), dim3(256), 0, st, (const mtb_match *)sl.d_ovf, sl.n_ovf,
                                                      (const uint32_t *)d_bigidx, (const uint64_t *)d_bigstart, d_bigcur, d_big, sl.ovf_region, (const unsigned long long *)c->d_ovfctr, skip_grouped);
        } else
        if (sl.n_ovf) hipLaunchKernelGGL(k_big_ovf, dim3((uint32_t)((sl.n_ovf + 255) / 256)), dim3(256), 0, st, (const mtb_match *)sl.d_ovf, sl.n_ovf,
                                      (const uint32_t *)d_bigidx, (const uint64_t *)d_bigstart, d_bigcur, d_big, (uint64_t)0, (const unsigned long long *)nullptr, skip_grouped);
        /* segments of up to 512 matches (nearly all: a read of a conserved gene brings a few hundred) are sorted in LDS by one wave
         * each; only the ones beyond go through the HBM-resident bitonic network (36 global-memory stages for 256 records: it cost
         * ~70 us per segment, and 7 % of the reads of a realistic batch come here) */
        uint32_t *d_lg;
        STCHK(ensure(c, "large", n_big, &d_lg));
        HIPCHK(scal_clear(c, SC_DEFER_N_LARGE));
        hipLaunchKernelGGL(k_segsort_small, dim3(std::min<uint32_t>(n_big, 256u * 40u)), dim3(64), 0, st, d_big, (const uint64_t *)d_bigstart, (uint64_t)n_big, d_lg,
                           scal<uint32_t>(c, SC_DEFER_N_LARGE), (uint32_t *)nullptr);
        hipLaunchKernelGGL((k_segsort_large<mtb_match>), dim3(std::min<uint32_t>(n_big, 1024)), dim3(256), 0, st, d_big, (const uint64_t *)d_bigstart,
                           (const uint32_t *)d_lg, scal<const uint32_t>(c, SC_DEFER_N_LARGE));
        HIPCHK(hipGetLastError());
        b->m = d_big; b->seg = d_bigstart; b->list = d_biglist; b->n_list = scal<const uint32_t>(c, SC_N_DEFERRED); b->seg_by_list = 1;
        /* one wave per workgroup, 14 of them resident per CU: a thousand workgroups left three quarters of the chip idle when hundreds of
         * thousands of reads come here (reads of conserved genes: hundreds of matches each); the slab pool stays bounded by dev_score */
        b->sort = false; b->max_seg = (uint32_t)mx; b->grid = std::min<uint32_t>(n_big, 256u * 14u); b->cap = 320;
        return MTB_OK;
    };
    a.overflowed_listed = early;
    {   const mtb_status rs = dev_score(c, ix, p, n_reads, lens, out, n_taxcnt, a, &second, early ? &fork : nullptr);
        if (rs != MTB_OK) { if (c->score_overlapped) { hipError_t e = hipStreamSynchronize(c->side_stream); (void)e; } return rs; } }       /* nothing of the batch stays in flight behind an error */
    /* number of matches (statistics): live records seen by the first launch + the deferred reads' segments */
    { KTimer kt(c, MTB_K_SCAN); scan_launch<uint32_t, uint64_t, false>(st, d_cnt, n_reads, true, d_tot, d_ws2); }
    STCHK(d2h(c, &nm, d_tot + n_reads, 8));
    nm += big_total;
    *nm_out = nm;
    return MTB_OK;
}

/* results of a batch to the host with the taxID:count lists packed on the device first: only what they hold crosses PCIe */
static mtb_status download_packed(mtb_ctx *c, mtb_result *d_res, const int32_t *d_tt, const uint32_t *d_tc, uint64_t n_reads, mtb_result *results,
                                  int32_t *taxcnt_tax, uint32_t *taxcnt_cnt, uint64_t *n_taxcnt, uint64_t host_cap = ~0ull, int async_set = -1 /* >= 0: queue the copies on the download stream, packed lists in buffer set async_set */) {
    uint32_t *d_n; uint64_t *d_off, *d_ws; int32_t *d_tt2; uint32_t *d_tc2;
    STCHK(ensure(c, "tcn", n_reads, &d_n)); STCHK(ensure(c, "tcnewoff", n_reads + 1, &d_off)); STCHK(ensure(c, "scanws", scan_ws_elems(n_reads + 1), &d_ws));
    hipLaunchKernelGGL(k_taxcnt_n, dim3((uint32_t)((n_reads + 255) / 256)), dim3(256), 0, c->stream, (const mtb_result *)d_res, n_reads, d_n);
    scan_launch<uint32_t, uint64_t, false>(c->stream, d_n, n_reads, true, d_off, d_ws);
    uint64_t total = 0;
    STCHK(d2h(c, &total, d_off + n_reads, 8));
    if (total > host_cap) { *n_taxcnt = total; return fail(MTB_ERR_CAPACITY, "taxcnt arrays too small for the batch's taxID:count lists"); }
    STCHK(ensure(c, res_name(RES_TAX, async_set == 1), total, &d_tt2)); STCHK(ensure(c, res_name(RES_CNT, async_set == 1), total, &d_tc2));
    hipLaunchKernelGGL(k_taxcnt_pack, dim3((uint32_t)((n_reads + 255) / 256)), dim3(256), 0, c->stream, d_res, n_reads, (const uint64_t *)d_off, d_tt, d_tc, d_tt2, d_tc2);
    HIPCHK(hipGetLastError());
    if (async_set >= 0) {
        /* the rows and the packed lists leave on the download stream once the pack kernel is through; the compute stream is free for the next batch */
        HIPCHK(hipEventRecord(c->down_ready, c->stream));
        HIPCHK(hipStreamWaitEvent(c->down_stream, c->down_ready, 0));
        HIPCHK(hipMemcpyAsync(results, d_res, n_reads * sizeof(mtb_result), hipMemcpyDeviceToHost, c->down_stream));
        if (total) { HIPCHK(hipMemcpyAsync(taxcnt_tax, d_tt2, total * 4, hipMemcpyDeviceToHost, c->down_stream)); HIPCHK(hipMemcpyAsync(taxcnt_cnt, d_tc2, total * 4, hipMemcpyDeviceToHost, c->down_stream)); }
        HIPCHK(hipEventRecord(c->down_done, c->down_stream));
        c->down_pending = true;
        *n_taxcnt = total;
        return MTB_OK;
    }
    STCHK(d2h(c, results, d_res, n_reads * sizeof(mtb_result)));
    if (total) { STCHK(d2h(c, taxcnt_tax, d_tt2, total * 4)); STCHK(d2h(c, taxcnt_cnt, d_tc2, total * 4)); }
    *n_taxcnt = total;
    return MTB_OK;
}

/* ---- k-mer coverage (include/mtb.h: mtb_index_coverage_*; kernels_coverage.h; the rule: tests/coverage_spec.py) ---- */
static uint64_t cov_bitmap_words(const mtb_index *ix) { return std::max<uint64_t>((ix->T + 31) / 32, 1); }
static uint64_t cov_bin_words(const mtb_index *ix) { return (uint64_t)ix->tax.max_id + 1 + MTB_COV_EXTRA; }
static dim3 cov_grid(uint64_t n, uint64_t per_block, uint64_t most) { return dim3((uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((n + per_block - 1) / per_block, most))); }
/* The pending hits of one top-level classify call (or stage call): cleared at its start, moved into the index's bins at its successful end, left
 * behind (and cleared by the next call) after a failure.  An entry point called by another one finds the call open and does nothing. */
struct CovCall {
    mtb_ctx *c = nullptr; mtb_index *ix = nullptr;
    mtb_status begin(mtb_ctx *c_, mtb_index *ix_) {
        if (!ix_->d_cov_bits || c_->cov_call) return MTB_OK;
        const uint64_t words = cov_bin_words(ix_);
        if (c_->cov_pend_words < words) {
            if (c_->d_cov_pend) { hipError_t e = hipFree(c_->d_cov_pend); (void)e; c_->d_cov_pend = nullptr; c_->cov_pend_words = 0; }
            if (hipMalloc((void **)&c_->d_cov_pend, words * 8) != hipSuccess) { c_->d_cov_pend = nullptr; (void)hipGetLastError(); return fail(MTB_ERR_OOM, "no HBM for the pending coverage bins"); }
            c_->cov_pend_words = words;
        }
        HIPCHK(hipMemsetAsync(c_->d_cov_pend, 0, words * 8, c_->stream));
        HIPCHK(hipStreamSynchronize(c_->stream));          /* the lanes add from streams of their own */
        for (mtb_ctx *l : c_->lanes) { l->d_cov_pend = c_->d_cov_pend; l->cov_pend_words = c_->cov_pend_words; }
        c = c_; ix = ix_; c->cov_call = true;
        return MTB_OK;
    }
    mtb_status end(mtb_status st) {
        if (!c) return st;
        mtb_ctx *cc = c; c = nullptr; cc->cov_call = false;
        if (st != MTB_OK) return st;
        const uint64_t words = cov_bin_words(ix);
        hipLaunchKernelGGL(k_cov_commit, cov_grid(words, 256, ~0u), dim3(256), 0, cc->stream, ix->d_cov_hits, cc->d_cov_pend, words, (uint64_t)ix->tax.max_id + 1 + MTB_COV_N_BATCHES, 1u);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(cc->stream));
        return MTB_OK;
    }
    ~CovCall() { if (c) c->cov_call = false; }
};
/* rs[0, n_reads) from the rows, then the marks and pending hits of d_q[0, n) (seq 1-based into the rows), on the context's stream.  `use` holds the
 * index in the state it is in; the caller releases it after the stream is synchronised. */
static mtb_status dev_cov_mark(mtb_ctx *c, mtb_index *ix, const mtb_kmer *d_q, uint64_t n, const mtb_result *d_res, uint64_t n_reads, uint32_t *d_rs, IndexUse *use) {
    if (!c->d_cov_pend || c->cov_pend_words < cov_bin_words(ix)) return fail(MTB_ERR_ARG, "k-mer coverage: no classify call is open on this context");
    if (n_reads == 0 || n == 0) return MTB_OK;
    hipStream_t st = c->stream;
    hipLaunchKernelGGL(k_cov_read_species, cov_grid(n_reads, 256, ~0u), dim3(256), 0, st, d_res, n_reads, (const int32_t *)ix->d_tax2species, ix->tax.max_id, d_rs);
    HIPCHK(hipGetLastError());
    bool packed = false;
    use->hold(ix, &packed);
    const mtb_index_view v = index_view(ix); const mtb_dir_view dv = dir_view(ix);
    const dim3 grid = cov_grid(n, 256, 1u << 14);
    if (packed) hipLaunchKernelGGL((k_cov_mark<true, true>), grid, dim3(256), 0, st, d_q, n, (const uint32_t *)d_rs, n_reads, v, dv, ix->d_cov_bits, c->d_cov_pend);
    else if (ix->d_dir) hipLaunchKernelGGL((k_cov_mark<false, true>), grid, dim3(256), 0, st, d_q, n, (const uint32_t *)d_rs, n_reads, v, dv, ix->d_cov_bits, c->d_cov_pend);
    else hipLaunchKernelGGL((k_cov_mark<false, false>), grid, dim3(256), 0, st, d_q, n, (const uint32_t *)d_rs, n_reads, v, dv, ix->d_cov_bits, c->d_cov_pend);
    HIPCHK(hipGetLastError());
    return MTB_OK;
}

extern "C" {

mtb_status mtb_index_coverage_begin(mtb_index *ix) {
    if (!ix) return fail(MTB_ERR_ARG, "NULL index");
    if (ix->parent || ix->is_part) return fail(MTB_ERR_UNSUPPORTED, "k-mer coverage needs a whole index: not a view (mtb_index_slice) or a part (mtb_index_open_part)");
    if (ix->d_cov_bits) return fail(MTB_ERR_ARG, "k-mer coverage is already on for this index");
    HIPCHK(hipSetDevice(ix->ctx->device));
    uint32_t *bits = nullptr; unsigned long long *hits = nullptr;
    const uint64_t words = cov_bitmap_words(ix), bins = cov_bin_words(ix);
    struct Guard { uint32_t *&b; unsigned long long *&h; ~Guard() { hipError_t e = hipSuccess; if (b) e = hipFree(b); if (h) e = hipFree(h); (void)e; } } guard{bits, hits};
    if (hipMalloc((void **)&bits, words * 4) != hipSuccess) { bits = nullptr; (void)hipGetLastError(); return fail(MTB_ERR_OOM, "no HBM for the coverage bitmap (" + std::to_string(words * 4) + " bytes)"); }
    if (hipMalloc((void **)&hits, bins * 8) != hipSuccess) { hits = nullptr; (void)hipGetLastError(); return fail(MTB_ERR_OOM, "no HBM for the coverage bins"); }
    HIPCHK(hipMemsetAsync(bits, 0, words * 4, ix->ctx->stream)); HIPCHK(hipMemsetAsync(hits, 0, bins * 8, ix->ctx->stream));
    HIPCHK(hipStreamSynchronize(ix->ctx->stream));
    ix->d_cov_bits = bits; ix->d_cov_hits = hits;
    bits = nullptr; hits = nullptr;
    return MTB_OK;
}

mtb_status mtb_index_coverage_end(mtb_index *ix) {
    if (!ix) return fail(MTB_ERR_ARG, "NULL index");
    if (!ix->d_cov_bits) return fail(MTB_ERR_ARG, "k-mer coverage is not on for this index");
    HIPCHK(hipSetDevice(ix->ctx->device));
    hipError_t e = hipFree(ix->d_cov_bits); e = hipFree(ix->d_cov_hits); (void)e;
    ix->d_cov_bits = nullptr; ix->d_cov_hits = nullptr;
    return MTB_OK;
}

mtb_status mtb_index_coverage_merge(mtb_index *dst, mtb_index *src) {
    if (!dst || !src || dst == src) return fail(MTB_ERR_ARG, "two different indices are needed");
    if (!dst->d_cov_bits || !src->d_cov_bits) return fail(MTB_ERR_ARG, "k-mer coverage is not on for both indices");
    if (dst->T != src->T || dst->tax.max_id != src->tax.max_id) return fail(MTB_ERR_ARG, "the indices differ in size: only a clone and its source can be merged");
    mtb_ctx *dc = dst->ctx, *sc = src->ctx;
    HIPCHK(hipSetDevice(sc->device)); HIPCHK(hipStreamSynchronize(sc->stream));
    HIPCHK(hipSetDevice(dc->device));
    hipStream_t st = dc->stream;
    const uint64_t words = cov_bitmap_words(dst), bins = cov_bin_words(dst);
    const uint64_t stage_bytes = std::min<uint64_t>(64ull << 20, std::max<uint64_t>(std::max(words * 4, bins * 8), 256));      /* a multiple of 8 */
    void *stage = nullptr;
    if (hipMalloc(&stage, stage_bytes) != hipSuccess) { (void)hipGetLastError(); return fail(MTB_ERR_OOM, "no HBM for the merge's staging buffer"); }
    struct Guard { void *p; ~Guard() { hipError_t e = hipFree(p); (void)e; } } guard{stage};
    auto fetch = [&](const void *from, size_t bytes) -> mtb_status {
        if (sc->device == dc->device) HIPCHK(hipMemcpyAsync(stage, from, bytes, hipMemcpyDeviceToDevice, st));
        else HIPCHK(hipMemcpyPeerAsync(stage, dc->device, from, sc->device, bytes, st));
        return MTB_OK;
    };
    for (uint64_t w = 0; w < words; w += stage_bytes / 4) {
        const uint64_t m = std::min<uint64_t>(stage_bytes / 4, words - w);
        STCHK(fetch(src->d_cov_bits + w, m * 4));
        hipLaunchKernelGGL(k_cov_or, cov_grid(m, 256, 1u << 14), dim3(256), 0, st, dst->d_cov_bits + w, (const uint32_t *)stage, m);
        HIPCHK(hipGetLastError());
    }
    for (uint64_t w = 0; w < bins; w += stage_bytes / 8) {
        const uint64_t m = std::min<uint64_t>(stage_bytes / 8, bins - w);
        STCHK(fetch(src->d_cov_hits + w, m * 8));
        hipLaunchKernelGGL(k_cov_commit, cov_grid(m, 256, ~0u), dim3(256), 0, st, dst->d_cov_hits + w, (unsigned long long *)stage, m, ~0ull, 0u);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipStreamSynchronize(st));
    return MTB_OK;
}

mtb_status mtb_index_coverage_report(mtb_index *ix, uint64_t *distinct, uint64_t *hits, uint64_t *total, uint64_t cap, mtb_coverage_stats *stats) {
    if (!ix) return fail(MTB_ERR_ARG, "NULL index");
    if (!ix->d_cov_bits) return fail(MTB_ERR_ARG, "k-mer coverage is not on for this index");
    const uint64_t n_bins = (uint64_t)ix->tax.max_id + 1;
    if ((distinct || hits || total) && cap < n_bins)
        return fail(MTB_ERR_CAPACITY, "the arrays hold " + std::to_string(cap) + " entries, the taxonomy needs " + std::to_string(n_bins));
    mtb_ctx *c = ix->ctx;
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    /* u32 bins of one pass: total and distinct, one array per XCD each; their u64 sums; the popcount */
    const uint64_t stride = (n_bins + 63) & ~63ull, pass_words = 2 * stride * MTB_AUDIT_REPLICAS;
    char *mem = nullptr;
    const size_t bytes = pass_words * 4 + 2 * n_bins * 8 + 8;
    if (hipMalloc((void **)&mem, bytes) != hipSuccess) { (void)hipGetLastError(); return fail(MTB_ERR_OOM, "no HBM for the coverage report's bins"); }
    hipEvent_t e0 = nullptr, e1 = nullptr;
    struct Guard { char *p; hipEvent_t &a, &b; ~Guard() { hipError_t e = hipFree(p); if (a) e = hipEventDestroy(a); if (b) e = hipEventDestroy(b); (void)e; } } guard{mem, e0, e1};
    HIPCHK(hipEventCreate(&e0)); HIPCHK(hipEventCreate(&e1));
    unsigned long long *d_sum = (unsigned long long *)mem, *d_pop = d_sum + 2 * n_bins;      /* [0, n_bins) total, [n_bins, 2 n_bins) distinct */
    uint32_t *d_pass = (uint32_t *)(d_pop + 1);
    HIPCHK(hipMemsetAsync(mem, 0, bytes, st));
    HIPCHK(hipEventRecord(e0, st));
    IndexUse use; bool packed = false;
    use.hold(ix, &packed);
    const mtb_index_view v = index_view(ix);
    const uint64_t SEG = 1ull << 31;                 /* entries per pass: a u32 bin cannot overflow */
    for (uint64_t t0 = 0; t0 < ix->T; t0 += SEG) {
        const uint64_t m = std::min<uint64_t>(SEG, ix->T - t0);
        const dim3 grid = cov_grid(m, 256ull * MTB_AUDIT_PER_LANE, 1u << 16);
        if (packed) hipLaunchKernelGGL(k_cov_count<true>, grid, dim3(256), 0, st, v, t0, m, (const uint32_t *)ix->d_cov_bits, d_pass, d_pass + stride * MTB_AUDIT_REPLICAS, stride);
        else hipLaunchKernelGGL(k_cov_count<false>, grid, dim3(256), 0, st, v, t0, m, (const uint32_t *)ix->d_cov_bits, d_pass, d_pass + stride * MTB_AUDIT_REPLICAS, stride);
        HIPCHK(hipGetLastError());
        for (int k = 0; k < 2; k++) {
            uint32_t *bins = d_pass + (uint64_t)k * stride * MTB_AUDIT_REPLICAS;
            hipLaunchKernelGGL(k_audit_bins_reduce, cov_grid(n_bins, 256, ~0u), dim3(256), 0, st, bins, n_bins, stride);
            hipLaunchKernelGGL(k_cov_accumulate, cov_grid(n_bins, 256, ~0u), dim3(256), 0, st, d_sum + (uint64_t)k * n_bins, bins, n_bins);
            HIPCHK(hipGetLastError());
            if (t0 + SEG < ix->T) HIPCHK(hipMemsetAsync(bins, 0, stride * MTB_AUDIT_REPLICAS * 4, st));       /* the other replicas, for the next pass */
        }
    }
    hipLaunchKernelGGL(k_popcount_words, cov_grid(cov_bitmap_words(ix), 256, 4096), dim3(256), 0, st, (const uint32_t *)ix->d_cov_bits, cov_bitmap_words(ix), d_pop);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(e1, st));
    HIPCHK(hipEventSynchronize(e1));
    use.release();
    std::vector<unsigned long long> h_hits(cov_bin_words(ix));
    unsigned long long n_marked = 0;
    if (total) STCHK(d2h(c, total, d_sum, n_bins * 8));
    if (distinct) STCHK(d2h(c, distinct, d_sum + n_bins, n_bins * 8));
    STCHK(d2h(c, h_hits.data(), ix->d_cov_hits, h_hits.size() * 8));
    STCHK(d2h(c, &n_marked, d_pop, 8));
    if (hits) for (uint64_t s = 0; s < n_bins; s++) hits[s] = h_hits[s];
    if (stats) {
        memset(stats, 0, sizeof(*stats));
        stats->n_targets = ix->T; stats->n_marked = n_marked;
        for (uint64_t s = 0; s < n_bins; s++) stats->n_hits += h_hits[s];
        stats->n_queries = h_hits[n_bins + MTB_COV_N_QUERIES]; stats->n_queries_counted = h_hits[n_bins + MTB_COV_N_COUNTED]; stats->n_batches = h_hits[n_bins + MTB_COV_N_BATCHES];
        HIPCHK(hipEventElapsedTime(&stats->ms_count, e0, e1));
    }
    return MTB_OK;
}

mtb_status mtb_index_coverage_mark(mtb_ctx *c, mtb_index *ix, const mtb_kmer *kmers, uint64_t n, const mtb_result *results, uint64_t n_reads) {
    if (!c || !ix || (n && !kmers) || (n_reads && !results)) return fail(MTB_ERR_ARG, "NULL argument");
    if (!ix->d_cov_bits) return fail(MTB_ERR_ARG, "k-mer coverage is not on for this index");
    for (uint64_t i = 0; i < n; i++)
        if ((uint64_t)mtb_q_seq(kmers[i].qinfo) > n_reads)
            return fail(MTB_ERR_ARG, "metamer " + std::to_string(i) + " names read " + std::to_string(mtb_q_seq(kmers[i].qinfo)) + " of " + std::to_string(n_reads));
    HIPCHK(hipSetDevice(c->device));
    if (n == 0 || n_reads == 0) return MTB_OK;
    CovCall cov;
    STCHK(cov.begin(c, ix));
    mtb_kmer *d_q; mtb_result *d_r; uint32_t *d_rs;
    STCHK(ensure(c, "kmersA", n, &d_q)); STCHK(ensure(c, "covrows", n_reads, &d_r)); STCHK(ensure(c, "covrs", n_reads, &d_rs));       /* (rows of their own: an asynchronous download may still read the result sets) */
    STCHK(h2d(c, d_q, kmers, n * sizeof(mtb_kmer))); STCHK(h2d(c, d_r, results, n_reads * sizeof(mtb_result)));
    IndexUse use;
    mtb_status st = dev_cov_mark(c, ix, d_q, n, d_r, n_reads, d_rs, &use);
    if (st == MTB_OK) { hipError_t e = hipStreamSynchronize(c->stream); if (e != hipSuccess) st = fail(MTB_ERR_DEVICE, std::string("hipStreamSynchronize: ") + hipGetErrorString(e)); }
    use.release();
    return cov.end(st);
}

} // extern "C"

/* the sorted query metamers of a read range, and what the extractor said about them */
struct SortedQueries {
    const mtb_kmer *d_s = nullptr; uint64_t nk = 0; int low_bits = 32;       /* low_bits: the bits the list is NOT sorted on (the join's tile windows follow the sort key) */
    uint32_t max_q = 0; const uint32_t *d_counts = nullptr;                  /* most metamers of a read (of those that use the slots); metamers per read (long-read slot path) */
};
/* What the slot join leaves dead until the next batch's extraction, for scratch(): the metamer buffer that does NOT hold the sorted list (that one is looked at after the batch), both digit arrays */
static void set_dead_segments(mtb_ctx *c, const mtb_kmer *d_sorted) {
    c->n_dead = 0;
    const size_t least = c->opt.scratch_alias > 0 ? 1 : (64u << 20);
    for (const char *name : {"kmersA", "kmersB", "digA", "digB"}) {
        const DevBuf b = buf_get(c, name);
        if (c->opt.scratch_alias < 0 || !b.p || b.p == (const void *)d_sorted || b.cap < least || c->n_dead == 3) continue;
        c->dead[c->n_dead++] = {(char *)b.p, b.cap, 0};
    }
}
/* Long reads on ordinal slots: join into per-read slot ranges, order every range by a stable species partition (k_seg_order), score.
 * *done = false (nothing scored): some read overran even the long tails; the caller redoes the range on exact segments. */
static mtb_status score_long_slots(mtb_ctx *c, mtb_index *ix, const mtb_params *p, uint64_t n_reads, const ReadLens &lens, const SortedQueries &q,
                                   const ResultSink &out, uint64_t *n_taxcnt, uint64_t *nm_out, bool *done) {
    hipStream_t st = c->stream; uint32_t *d_sizes, *d_live, *d_fail, *d_rc; uint64_t *d_rb, *d_ws2;
    STCHK(ensure(c, "lsizes", n_reads, &d_sizes)); STCHK(ensure(c, "lrb", n_reads + 1, &d_rb)); STCHK(ensure(c, "scanws", scan_ws_elems(n_reads + 1), &d_ws2));
    STCHK(ensure(c, "livecnt", n_reads, &d_live)); STCHK(ensure(c, "lfail", n_reads, &d_fail)); STCHK(ensure(c, "readcnt", n_reads, &d_rc));     /* the join's per-read cursors */
    *done = false;
    /* tail = a quarter of the read's metamers, then all of them; a context whose last batch needed the long tails starts with them
     * (a database with long candidate runs overflows the short ones batch after batch: the join ran twice every time) */
    for (uint32_t tf = c->lslot_tf_start; tf <= 4 && !*done; tf *= 4) {
        hipLaunchKernelGGL(k_lslot_sizes, dim3((uint32_t)((n_reads + 255) / 256)), dim3(256), 0, st, (const uint32_t *)q.d_counts, n_reads, tf, d_sizes);
        { KTimer kt(c, MTB_K_SCAN); scan_launch<uint32_t, uint64_t, false>(st, d_sizes, n_reads, true, d_rb, d_ws2); }
        uint64_t n_slots = 0;
        STCHK(d2h(c, &n_slots, d_rb + n_reads, 8));
        mtb_slot16 *d_segm; mtb_match *d_m; STCHK(ensure(c, "segm", n_slots, &d_segm));
        c->seg_epoch = MTB_SLOT_EPOCHS;                           /* (a later short-read batch starts from a cleared buffer) */
        HIPCHK(hipMemsetAsync(d_segm, 0, n_slots * sizeof(mtb_slot16), st));
        HIPCHK(hipMemsetAsync(d_rc, 0, n_reads * 4, st));
        JoinSegArgs sa; memset(&sa, 0, sizeof(sa)); uint64_t n_ovf = 0;
        sa.seg = d_segm; sa.cursor = d_rc; sa.rb = d_rb; sa.dcnt = q.d_counts; sa.tf = tf; sa.ovf = nullptr; sa.ovf_cap = 0;
        mtb_status s2 = dev_join(c, ix, q.d_s, q.nk, MatchList(), &n_ovf, &sa, q.low_bits);
        if (s2 == MTB_ERR_CAPACITY) {                              /* some read's tail overran: larger tails */
            c->lslot_tf_start = 4;
            if (c->opt.lslot_verbose) fprintf(stderr, "mtb: long-read slot path: %llu matches beyond the tails at tail factor %u/4\n", (unsigned long long)n_ovf, tf);
            continue;
        }
        if (s2 != MTB_OK) return s2;
        HIPCHK(hipEventRecord(c->ev[3], st));
        STCHK(ensure(c, "matches", n_slots, &d_m));
        HIPCHK(scal_clear(c, SC_LS_N_FAIL, 2));         /* ... and SC_LS_N_ALL */
        HIPCHK(scal_clear(c, SC_LS_WORK));
        { KTimer kt(c, MTB_K_SEGSORT);
          hipLaunchKernelGGL(k_seg_order, dim3((uint32_t)std::min<uint64_t>(n_reads, 256ull * 2)), dim3(MTB_SO_NT), 0, st, (const mtb_slot16 *)d_segm, (const uint64_t *)d_rb,
                             (const uint32_t *)q.d_counts, (const uint32_t *)d_rc, tf, n_reads, d_m, d_live, scal<uint32_t>(c, SC_LS_N_FAIL), d_fail, scal<unsigned long long>(c, SC_LS_WORK),
                             scal<unsigned long long>(c, SC_LS_N_ALL)); }
        HIPCHK(hipGetLastError());
#ifdef MTB_SO_PHASE_CYCLES
        {   HIPCHK(hipStreamSynchronize(st));
            unsigned long long h[8], z[8] = {0};
            HIPCHK(hipMemcpyFromSymbol(h, HIP_SYMBOL(mtb_so_cycles), sizeof(h)));
            HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(mtb_so_cycles), z, sizeof(z)));
            static const char *nm[8] = {"claim + clear", "pass 1 (bits)", "pass 2 (counts, tail keys)", "single-match species", "tail sort", "species sort + offsets", "scatter pass", "tail pass"};
            unsigned long long tot = 0; for (int k = 0; k < 8; k++) tot += h[k];
            fprintf(stderr, "k_seg_order phases (%llu reads):", (unsigned long long)n_reads);
            for (int k = 0; k < 8; k++) fprintf(stderr, " %s %.1f %%;", nm[k], tot ? 100.0 * (double)h[k] / (double)tot : 0.0);
            fprintf(stderr, "\n");
        }
#endif
        uint64_t sc2[2] = {0, 0};
        STCHK(d2h(c, sc2, scal<uint64_t>(c, SC_LS_N_FAIL), 16));
        if (c->opt.lslot_verbose) fprintf(stderr, "mtb: long-read slot path: %llu reads, tail factor %u/4, %llu slots, %llu matches, %llu reads beyond the LDS tables (sorted the general way)\n",
                                                 (unsigned long long)n_reads, tf, (unsigned long long)n_slots, (unsigned long long)sc2[1], (unsigned long long)(sc2[0] & 0xFFFFFFFFull));
        const uint32_t n_failed = (uint32_t)(sc2[0] & 0xFFFFFFFFull);
        /* reads beyond k_seg_order's LDS tables: their live slots -> exact segments, sorted the general way */
        mtb_match *d_big = nullptr; uint64_t *d_bigstart = nullptr; uint32_t big_max = 0; uint64_t big_total = 0;
        if (n_failed) {
            uint32_t *d_bigcnt; mtb_match *d_scr; uint64_t mx = 0;
            STCHK(ensure(c, "bigcnt", n_failed, &d_bigcnt)); STCHK(ensure(c, "bigstart", (uint64_t)n_failed + 1, &d_bigstart));
            HIPCHK(scal_clear(c, SC_LS_MAX_SEG));
            hipLaunchKernelGGL(k_lbig_count, dim3(std::min<uint32_t>(n_failed, 4096)), dim3(64), 0, st, (const mtb_slot16 *)d_segm, (const uint64_t *)d_rb, (const uint32_t *)q.d_counts,
                               (const uint32_t *)d_rc, tf, (const uint32_t *)d_fail, n_failed, d_bigcnt, scal<uint32_t>(c, SC_LS_MAX_SEG));
            scan_launch<uint32_t, uint64_t, false>(st, d_bigcnt, n_failed, true, d_bigstart, d_ws2);
            STCHK(d2h(c, &big_total, d_bigstart + n_failed, 8));
            STCHK(d2h(c, &mx, scal<uint64_t>(c, SC_LS_MAX_SEG), 8));
            big_max = (uint32_t)mx;
            STCHK(ensure(c, "lbigm", big_total, &d_big)); STCHK(ensure(c, "jtemp", big_total, &d_scr));
            hipLaunchKernelGGL(k_lbig_copy, dim3(std::min<uint32_t>(n_failed, 4096)), dim3(64), 0, st, (const mtb_slot16 *)d_segm, (const uint64_t *)d_rb, (const uint32_t *)q.d_counts,
                               (const uint32_t *)d_rc, tf, (const uint32_t *)d_fail, n_failed, (const uint64_t *)d_bigstart, d_big);
            const size_t lds = (size_t)MTB_SEGLDS_CHUNK * 14;
            HIPCHK(hipFuncSetAttribute((const void *)k_segsort_lds<mtb_match>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            { KTimer kt(c, MTB_K_SEGSORT);
              hipLaunchKernelGGL((k_segsort_lds<mtb_match>), dim3(std::min<uint32_t>(n_failed, 2048)), dim3(MTB_SEGLDS_THREADS), lds, st, d_big, (const uint64_t *)d_bigstart,
                                 (const uint32_t *)nullptr, scal<const uint32_t>(c, SC_LS_N_FAIL), d_scr); }
            HIPCHK(hipGetLastError());
        }
        HIPCHK(hipEventRecord(c->ev[4], st)); HIPCHK(hipEventRecord(c->ev[5], st));
        STCHK(dev_score_long(c, ix, p, n_reads, lens, out, n_taxcnt, LongSegs{d_m, d_rb, q.max_q + mtb_lslot_tail(q.max_q, tf), d_live}));
        uint64_t n_generic = 0;
        if (n_failed) {
            STCHK(d2h(c, &n_generic, scal<uint64_t>(c, SC_N_GENERIC), 8));        /* reads the first launch left to the generic kernel */
            uint64_t n_tc2 = 0, g2 = 0;
            STCHK(dev_score_long(c, ix, p, n_reads, lens, out, &n_tc2, LongSegs{d_big, d_bigstart, big_max, /* d_segcnt */ nullptr, d_fail, n_failed}));
            STCHK(d2h(c, &g2, scal<uint64_t>(c, SC_N_GENERIC), 8));
            n_generic = (n_generic & 0xFFFFFFFFull) + (g2 & 0xFFFFFFFFull);
            STCHK(h2d(c, scal<uint64_t>(c, SC_N_GENERIC), &n_generic, 8));
        }
        *nm_out = sc2[1] + big_total; *done = true;
        c->stats.lslot_tail_factor = tf; c->stats.n_lslot_big_reads = n_failed;
    }
    return MTB_OK;
}
/* One attempt at one read range on one stream; taxcnt slots of this range start at out.tc_base of the caller's arrays.  long_slots: long reads may take
 * the ordinal-slot path; *redo_exact is set (nothing scored) when its slot ranges overflowed: classify_one comes again without them. */
static mtb_status classify_attempt(mtb_ctx *c, mtb_index *ix, const mtb_params *p, const Reads &rd, const ResultSink &out, uint64_t *n_taxcnt, bool long_slots, bool *redo_exact) {
    HIPCHK(hipSetDevice(c->device));
    *n_taxcnt = 0; *redo_exact = false;
    collect_kernel_times(c);          /* drop events of stage-level calls */
    memset(&c->stats, 0, sizeof(c->stats));
    const uint64_t n_reads = rd.n_reads;
    if (n_reads == 0) return MTB_OK;
    hipStream_t st = c->stream; int32_t *d_ql, *d_ql2;
    STCHK(ensure(c, "qlen", n_reads, &d_ql)); STCHK(ensure(c, "qlen2", n_reads, &d_ql2));
    uint32_t *d_cov_rs = nullptr;                    /* k-mer coverage on: the reads' species, for the marking behind the scoring */
    if (ix->d_cov_bits) STCHK(ensure(c, "covrs", n_reads, &d_cov_rs));
    HIPCHK(hipEventRecord(c->ev[0], st));
    /* short reads: per-read slot segments, the query's ordinal (tagged into qinfo by the extractor) is the slot of its
     * first match.  Needs positions < 2^12 (16-byte slot records) and a moderate number of metamers per read; otherwise
     * exact segments. */
    bool fixed = p->seq_mode != 3;
    /* long reads: ordinal slots too, with per-read slot ranges (k_join_dir<.., LONG>, kernels_seg_order.h) -- needs the directory join,
     * positions and ordinals below 2^16; otherwise (and after a failed attempt) exact segments via regroup + segment sort */
    bool lslot = p->seq_mode == 3 && ix->d_dir && long_slots && !c->opt.no_long_slots;
    const bool aa6 = p->kmer_format == 2;           /* 5-bit amino-acid letters: three base-21 pair passes order bits [34,64); the single-pass extractor writes the first pass's digits */
    ExtractOpts xo; xo.single_pass = true; xo.tag_ordinals = fixed || lslot; xo.want_digits = aa6;
    if (lslot) { STCHK(ensure(c, "dcnt", n_reads, &xo.d_counts)); HIPCHK(hipMemsetAsync(xo.d_counts, 0, n_reads * 4, st)); }
    /* short-read batches: reads whose positions do not fit a slot record (>= 4093 used bases) or that carry more metamers than a segment
     * has direct slots for are marked by the extractor and routed AROUND the slot segments one by one (join: overflow list; scoring:
     * exact segments) -- a handful of long reads in an Illumina batch no longer send the whole batch down the exact-segment path */
    if (fixed && ix->d_dir) STCHK(ensure(c, "offreads", n_reads, &xo.d_off_reads));
    Extracted ex; STCHK(dev_extract(c, p, rd, d_ql, d_ql2, xo, &ex));
    ReadLens lens{d_ql, d_ql2, ex.max_len};
    uint32_t max_q = ex.max_q; const uint32_t max_len_all = ex.max_len; bool route_off = false;
    if (fixed && xo.d_off_reads && ex.off_reads > 0 && ex.off_reads * 4 <= n_reads && ex.max_len + 3 < 65536u && max_q < 65535u && ex.off_reads < n_reads) {
        route_off = true;
        max_q = (uint32_t)ex.off_max_q; lens.max_len = (uint32_t)ex.off_max_len;       /* the slot geometry and the first scoring launch follow the reads that use the slots */
    }
    if ((fixed && !route_off && (lens.max_len + 3 >= MTB_SLOT_MAX_POS || max_q > MTB_SLOT_MAX_Q)) || (lslot && (lens.max_len + 3 >= 65536u || max_q >= 65535u))) {
        fixed = false; lslot = false;      /* tags would collide with positions / segments would be huge: extract again untagged */
        ExtractOpts untagged; untagged.single_pass = true; untagged.want_digits = aa6;
        STCHK(dev_extract(c, p, rd, d_ql, d_ql2, untagged, &ex));
        lens.max_len = ex.max_len; max_q = ex.max_q;
    }
    HIPCHK(hipEventRecord(c->ev[1], st));
    /* the join needs tiles with a narrow amino-acid range, not a total order: kmer_format 2 sorts on the first six
     * amino-acid letters (three base-21 pair passes = bits [34,64)), kmer_format 1 on the top 32 bits (four binary
     * passes; three binary passes make the tiles too wide for the LDS window, measured); the tile's target window
     * comes from k_join_bounds */
    int aa_first_shift = 34;
    if (aa6 && fixed && ix->d_dir && c->opt.sort_pairs > 0) aa_first_shift = 64 - 10 * std::max(1, std::min(3, c->opt.sort_pairs));
    mtb_kmer *d_s; uint32_t *d_rc;
    STCHK(dev_sort(c, ex.d_k, ex.nk, aa6 ? MTB_SORT_AA6 : 32, &d_s, aa_first_shift == 34 ? ex.d_dig : nullptr, aa_first_shift));
    HIPCHK(hipEventRecord(c->ev[2], st));
    SortedQueries q; q.d_s = d_s; q.nk = ex.nk; q.low_bits = aa6 ? aa_first_shift : 32; q.max_q = max_q; q.d_counts = xo.d_counts;
    c->last_sorted = (fixed && ix->d_dir) ? d_s : nullptr; c->last_sorted_n = ex.nk;
    STCHK(ensure(c, "readcnt", n_reads, &d_rc));
    HIPCHK(hipMemsetAsync(d_rc, 0, n_reads * 4, st));
    uint64_t nm = 0;
    if (fixed) {
        /* ---- join straight into per-read slot segments, score out of them ---- */
        SlotSegs sl;
        STCHK(make_slots(c, n_reads, max_q, d_rc, &sl));
        if (route_off) { sl.d_off_reads = xo.d_off_reads; sl.max_len_off = max_len_all; }
        uint64_t ovf_cap = ovf_cap_first(c, q.nk);
        for (int attempt = 0; attempt < 3; attempt++) {       /* the overflow list regrown to what the failed attempt reported */
            STCHK(ensure(c, "ovf", ovf_cap, &sl.d_ovf));
            JoinSegArgs sa; memset(&sa, 0, sizeof(sa));
            sa.seg = sl.d_segm; sa.stride = sl.stride; sa.direct = sl.direct; sa.cursor = d_rc; sa.ovf = sl.d_ovf; sa.ovf_cap = ovf_cap;
            sa.ovf_counter = nullptr; sa.epoch = sl.epoch; sa.off = sl.d_off_reads;
            sa.dense_ovf = attempt == 2 ? 1u : 0u;            /* last attempt: one list that holds the total, whatever the stripes' fill */
            sa.retry = attempt > 0 ? 1u : 0u;
            mtb_status s2 = dev_join(c, ix, q.d_s, q.nk, MatchList(), &sl.n_ovf, &sa, q.low_bits);
            if (s2 == MTB_OK) break;
            if (s2 != MTB_ERR_CAPACITY || attempt == 2) return s2;
            ovf_cap = ovf_cap_regrown(sl.n_ovf);
            HIPCHK(hipMemsetAsync(d_rc, 0, n_reads * 4, st));     /* ordinal slots are rewritten identically; tail slots and the overflow list are filled anew (their order follows the atomics) */
        }
        sl.ovf_region = c->ovf_region;
        for (int k = 3; k <= 5; k++) HIPCHK(hipEventRecord(c->ev[k], st));
        set_dead_segments(c, d_s);
        struct DeadEnd { mtb_ctx *c; ~DeadEnd() { c->n_dead = 0; } } dead_end{c};
        STCHK(score_fixed_slots(c, ix, p, n_reads, lens, ex.nk_real, sl, out, n_taxcnt, &nm));
    } else if (lslot) {
        bool done = false;
        STCHK(score_long_slots(c, ix, p, n_reads, lens, q, out, n_taxcnt, &nm, &done));
        if (!done) { *redo_exact = true; return MTB_OK; }
    } else {
        /* ---- long reads: exact segments (temp buffer, per-read counters, scan, regroup) ---- */
        MatchList ml; ml.d_read_cnt = d_rc;
        ml.cap = std::max<uint64_t>(buf_cap(c, "jtemp") / sizeof(mtb_match), q.nk + q.nk / 2 + 1024);
        for (int attempt = 0; attempt < 3; attempt++) {
            STCHK(ensure(c, "jtemp", ml.cap, &ml.d_out));
            mtb_status s2 = dev_join(c, ix, q.d_s, q.nk, ml, &nm, /* no slot segments */ nullptr, q.low_bits);
            if (s2 == MTB_OK) break;
            if (s2 != MTB_ERR_CAPACITY || attempt == 2) return s2;
            ml.cap = nm + nm / 16 + 1024;                     /* the reference's retry (Classifier.cpp:127-131) with the exact size */
            HIPCHK(hipMemsetAsync(d_rc, 0, n_reads * 4, st));
        }
        HIPCHK(hipEventRecord(c->ev[3], st));
        STCHK(score_join_order(c, ix, p, ml.d_out, nm, n_reads, d_rc, lens, out, n_taxcnt));
    }
    /* k-mer coverage: the range is scored, so every metamer of it is counted once; the sorted list is still whole on all three branches (the
     * scorers' scratch() is carved from the buffers that do NOT hold it, the long-read paths write buffers of their own) */
    IndexUse cov_use;
    if (d_cov_rs) STCHK(dev_cov_mark(c, ix, d_s, ex.nk, out.d_res, n_reads, d_cov_rs, &cov_use));
    HIPCHK(hipEventRecord(c->ev[6], st));
    HIPCHK(hipEventSynchronize(c->ev[6]));
    cov_use.release();
    mtb_batch_stats &S = c->stats;
    float *const stage_ms[6] = {&S.ms_extract, &S.ms_sort, &S.ms_join, &S.ms_regroup, &S.ms_segsort, &S.ms_score};
    for (int k = 0; k < 6; k++) HIPCHK(hipEventElapsedTime(stage_ms[k], c->ev[k], c->ev[k + 1]));
    HIPCHK(hipEventElapsedTime(&S.ms_total, c->ev[0], c->ev[6]));
    collect_kernel_times(c);
    S.n_reads = n_reads; S.n_bases = ex.n_bases; S.n_kmers = ex.nk_real; S.n_matches = nm; S.n_targets = ix->T;
    STCHK(take_generic_reads(c, n_reads, &S.n_generic_reads));
    S.n_slot_reads = (fixed || lslot) ? n_reads : 0;
    if (fixed) { S.n_deferred_reads = c->many_stats[0]; S.n_many_reads = c->many_stats[1]; S.n_many_matches = c->many_stats[2]; S.n_many_kept = c->many_stats[3]; S.score_overlapped = c->score_overlapped; }
    return MTB_OK;
}
static mtb_status classify_one(mtb_ctx *c, mtb_index *ix, const mtb_params *p, const Reads &rd, const ResultSink &out, uint64_t *n_taxcnt) {
    bool redo_exact = false;
    STCHK(classify_attempt(c, ix, p, rd, out, n_taxcnt, /* long_slots */ true, &redo_exact));
    /* the long-read slot ranges overflowed: this range again without ordinal slots (tags stripped by a fresh extraction), on exact segments */
    return redo_exact ? classify_attempt(c, ix, p, rd, out, n_taxcnt, /* long_slots */ false, &redo_exact) : MTB_OK;
}

static void merge_stats(mtb_batch_stats &S, const mtb_batch_stats &L) {
    S.ms_extract += L.ms_extract; S.ms_sort += L.ms_sort; S.ms_join += L.ms_join; S.ms_regroup += L.ms_regroup;
    S.ms_segsort += L.ms_segsort; S.ms_score += L.ms_score;
    S.n_reads += L.n_reads; S.n_bases += L.n_bases; S.n_kmers += L.n_kmers; S.n_matches += L.n_matches; S.n_targets = L.n_targets;
    S.n_generic_reads += L.n_generic_reads; S.n_slot_reads += L.n_slot_reads;
    S.n_deferred_reads += L.n_deferred_reads; S.n_many_reads += L.n_many_reads; S.n_many_matches += L.n_many_matches; S.n_many_kept += L.n_many_kept;
    for (int i = 0; i < MTB_NUM_KERNELS; i++) { S.ms_kernel[i] += L.ms_kernel[i]; S.n_launch[i] += L.n_launch[i]; }
    S.join_variant = L.join_variant; S.join_tuned = L.join_tuned;                 /* (of the last range) */
    for (int v = 0; v < 3; v++) S.join_tune_ms[v] = L.join_tune_ms[v];
    S.join_tiles += L.join_tiles; S.join_tiles_windowed += L.join_tiles_windowed; S.join_tiles_outside += L.join_tiles_outside;
    S.score_overlapped |= L.score_overlapped; S.lslot_tail_factor = L.lslot_tail_factor; S.n_lslot_big_reads += L.n_lslot_big_reads;       /* (factor: of the last range) */
}

/* HBM-budgeted batching (the reference sizes a QuerySplit from --max-ram, QueryIndexer.cpp:62,132, and redoes
 * it with a bigger match buffer on overflow, Classifier.cpp:127-131).  Here the budget is HBM: what hipMemGetInfo
 * reports free plus what the context's own buffers already hold (or mtb_ctx_set_workspace_limit), and the per-base
 * workspace is known -- two 16-byte metamer buffers + two 2-byte digit arrays per extracted metamer, one 16-byte slot per
 * metamer plus the tail for short reads (24-byte match records twice for long reads), ~100 bytes of per-read tables -- and
 * is re-measured on every sub-batch.  The batch is cut into contiguous read ranges of equal size that fit; a range that
 * still runs out of memory is halved and redone.  Results land at their final places (d_results + lo, taxcnt slots
 * appended), so the caller sees one batch. */
static mtb_status classify_budgeted(mtb_ctx *c, mtb_index *ix, const mtb_params *p, const Reads &rd, uint64_t n_bases_total, const ResultSink &out, uint64_t *n_taxcnt) {
    const uint64_t n_reads = rd.n_reads, taxcnt_cap = out.tc_cap;
    HIPCHK(hipSetDevice(c->device));
    *n_taxcnt = 0;
    c->last_sub_batches = 0; c->last_scratch_bytes = 0;
    if (n_reads == 0) { memset(&c->stats, 0, sizeof(c->stats)); return MTB_OK; }
    if (c->ws_seq_mode != p->seq_mode) {             /* other buffer set: what the previous mode grew would only sit in the way */
        if (c->ws_seq_mode) { HIPCHK(hipStreamSynchronize(c->stream)); release_workspace(c); }
        c->ws_seq_mode = p->seq_mode;
    }
    size_t fr = 0, tot = 0;
    HIPCHK(hipMemGetInfo(&fr, &tot));
    const size_t held = held_bytes(c, BUF_FIXED);
    uint64_t budget = c->ws_limit ? c->ws_limit : (uint64_t)fr + held;
    if (!c->ws_limit) budget -= std::min<uint64_t>(budget / 16, 4ull << 30);          /* allocator granularity, kernel scratch, other users of the device */
    if (p->seq_mode == 3 && !c->ws_limit) budget -= std::min<uint64_t>(budget / 4, MTB_SLAB_POOL_MAX);     /* the slab pool of the large-segment scorer does not scale with the batch */
    const double mean_len = (double)n_bases_total / (double)n_reads;
    double per_base = c->ws_per_base;
    if (per_base <= 0.0) {
        const double yield = (c->extract_yield > 0.0 ? c->extract_yield : (p->syncmer ? 1.0 : 2.0)) * 1.15;
        per_base = yield * (16 + 16 + 2 + 2) + (p->seq_mode == 3 ? yield * 1.5 * 48 : yield * 1.2 * 16 + 24.0 * 16 / std::max(mean_len, 1.0)) + 100.0 / std::max(mean_len, 1.0);
    }
    const double safety = c->ws_per_base > 0.0 ? 1.02 : 1.08;                           /* measured on the previous batch / first-call estimate */
    uint64_t fit = (uint64_t)((double)budget / (per_base * safety * mean_len));        /* reads per sub-batch */
    fit = std::max<uint64_t>(fit, 1);
    uint64_t n_sub = (n_reads + fit - 1) / fit;
    if (c->opt.host_timing)
        fprintf(stderr, "mtb budget: free %.1f GiB + held %.1f GiB -> budget %.1f GiB; %.1f bytes per base (%s) x %.2f -> %llu reads fit, %llu sub-batch(es) for %llu reads\n",
                (double)fr / 1073741824.0, (double)held / 1073741824.0, (double)budget / 1073741824.0, per_base, c->ws_per_base > 0.0 ? "measured" : "estimate", safety,
                (unsigned long long)fit, (unsigned long long)n_sub, (unsigned long long)n_reads);
    mtb_batch_stats S; memset(&S, 0, sizeof(S));
    uint64_t tc_used = 0, lo = 0;
    uint32_t done = 0;
    while (lo < n_reads) {
        const uint64_t left_sub = std::max<uint64_t>(1, n_sub > done ? n_sub - done : 1);
        uint64_t cnt = (n_reads - lo + left_sub - 1) / left_sub;
        uint64_t n_tc = 0;
        mtb_status st;
        for (;;) {
            st = classify_one(c, ix, p, rd.range(lo, cnt),
                              ResultSink{out.d_res + lo, out.d_tc_tax + tc_used, out.d_tc_cnt + tc_used, taxcnt_cap - std::min(taxcnt_cap, tc_used), out.tc_base + tc_used}, &n_tc);
            if (st != MTB_ERR_OOM || cnt <= 1024) break;
            /* the estimate was too optimistic for this range: give the memory back, halve, redo */
            HIPCHK(hipStreamSynchronize(c->stream));
            if (c->opt.host_timing) fprintf(stderr, "mtb budget: %llu reads ran out of memory (%s); halving\n", (unsigned long long)cnt, mtb_last_error());
            release_workspace(c);
            cnt = (cnt + 1) / 2; n_sub *= 2; done *= 2;
        }
        if (st == MTB_ERR_CAPACITY) {
            /* taxcnt arrays too small: report what the whole batch needs (slots of the ranges done + this one + the rest pro rata) */
            const uint64_t rest = n_reads - lo - cnt;
            *n_taxcnt = std::max<uint64_t>(taxcnt_cap + 1, tc_used + n_tc + (uint64_t)((double)n_tc / (double)cnt * (double)rest * 1.05) + 64);
            return st;
        }
        if (st != MTB_OK) return st;
        /* the buffers only grow: what they hold belongs to the largest sub-batch they have seen, not to this one (dividing by a
         * smaller one inflates the figure, more sub-batches follow, and the next measurement is worse still) */
        c->ws_max_sub_bases = std::max<uint64_t>(c->ws_max_sub_bases, c->stats.n_bases);
        if (c->ws_max_sub_bases) c->ws_per_base = (double)held_bytes(c, BUF_WORK) / (double)c->ws_max_sub_bases;
        if (c->opt.host_timing) {
            std::lock_guard<std::mutex> lk(c->bufs_mu);
            fprintf(stderr, "mtb budget: sub-batch of %llu reads (%llu bases) done; buffers (GiB):", (unsigned long long)cnt, (unsigned long long)c->stats.n_bases);
            for (auto &kv : c->bufs) if (kv.second.cap >= (256u << 20)) fprintf(stderr, " %s %.2f", kv.first.c_str(), (double)kv.second.cap / 1073741824.0);
            fprintf(stderr, "\n");
        }
        merge_stats(S, c->stats); S.ms_total += c->stats.ms_total;
        tc_used += n_tc; lo += cnt; done++;
    }
    c->stats = S;
    c->last_sub_batches = done;
    *n_taxcnt = tc_used;
    return MTB_OK;
}

extern "C" {

static mtb_status classify_batch_device_impl(mtb_ctx *c, mtb_index *ix, const mtb_params *p, const char *d_bases, const uint64_t *d_offs,
                                             const char *d_bases2, const uint64_t *d_offs2, uint64_t n_reads, uint64_t n_bases_total,
                                             mtb_result *d_results, int32_t *d_taxcnt_tax, uint32_t *d_taxcnt_cnt, uint64_t taxcnt_cap,
                                             uint64_t *n_taxcnt) {
    const size_t L = c->lanes.size();
    if (L < 2 || n_reads < 4096 * L)
        return classify_budgeted(c, ix, p, Reads{d_bases, d_offs, d_bases2, d_offs2, n_reads}, n_bases_total, ResultSink{d_results, d_taxcnt_tax, d_taxcnt_cnt, taxcnt_cap, /* tc_base */ 0}, n_taxcnt);
    /* L contiguous read ranges, one host thread + one non-blocking stream each */
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));          /* inputs produced on the caller's stream are complete */
    auto t0 = std::chrono::steady_clock::now();
    std::vector<mtb_status> st(L, MTB_OK);
    std::vector<std::string> errs(L);
    std::vector<uint64_t> ntc(L, 0);
    std::vector<std::thread> th;
    /* `chunks` read ranges per stream, interleaved (range k runs on stream k % L) */
    const int chunks = std::max(1, c->opt.chunks_per_stream);   /* sweep: profiles/r01_notes.md */
    const size_t NC = L * (size_t)chunks;
    const uint64_t tc_share = taxcnt_cap / NC;
    std::vector<mtb_batch_stats> lane_stats(L);
    for (size_t i = 0; i < L; i++) memset(&lane_stats[i], 0, sizeof(mtb_batch_stats));
    for (size_t i = 0; i < L; i++) {
        th.emplace_back([&, i]() {
            mtb_ctx *l = c->lanes[i];
            /* experiment switch: lane i starts i * MTB_LANE_STAGGER_MS late, so that the lanes are in DIFFERENT stages at any moment
             * (the join is bound by store transactions, the sort by HBM bandwidth, extraction and scoring by VALU issue) */
            const int stagger_ms = c->opt.lane_stagger_ms;
            if (stagger_ms > 0 && i > 0) std::this_thread::sleep_for(std::chrono::milliseconds((long)stagger_ms * (long)i));
            for (size_t k = i; k < NC; k += L) {
                uint64_t lo = n_reads * k / NC, hi = n_reads * (k + 1) / NC;
                uint64_t n_tc = 0;
                mtb_status s = classify_one(l, ix, p, Reads{d_bases, d_offs, d_bases2, d_offs2, n_reads}.range(lo, hi - lo),
                                            ResultSink{d_results + lo, d_taxcnt_tax + tc_share * k, d_taxcnt_cnt + tc_share * k, tc_share, tc_share * k}, &n_tc);
                ntc[i] = std::max(ntc[i], n_tc * NC / L);
                if (s != MTB_OK) { st[i] = s; errs[i] = g_err; break; }
                merge_stats(lane_stats[i], l->stats);
            }
        });
    }
    for (auto &t : th) t.join();
    memset(&c->stats, 0, sizeof(c->stats));
    uint64_t need = 0;
    for (size_t i = 0; i < L; i++) { merge_stats(c->stats, lane_stats[i]); need = std::max(need, ntc[i] * L); }
    c->stats.ms_total = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    *n_taxcnt = taxcnt_cap;                             /* slots are spread over the whole array */
    for (size_t i = 0; i < L; i++)
        if (st[i] != MTB_OK) { if (st[i] == MTB_ERR_CAPACITY) *n_taxcnt = std::max<uint64_t>(need, taxcnt_cap + 1); return fail(st[i], errs[i]); }
    return MTB_OK;
}

/* (k-mer coverage: every public classify entry point brackets its work with a CovCall; the outermost one commits the hits) */
mtb_status mtb_classify_batch_device(mtb_ctx *c, mtb_index *ix, const mtb_params *p, const char *d_bases, const uint64_t *d_offs,
                                     const char *d_bases2, const uint64_t *d_offs2, uint64_t n_reads, uint64_t n_bases_total,
                                     mtb_result *d_results, int32_t *d_taxcnt_tax, uint32_t *d_taxcnt_cnt, uint64_t taxcnt_cap,
                                     uint64_t *n_taxcnt) {
    if (!c || !ix || !p || !n_taxcnt) return fail(MTB_ERR_ARG, "NULL argument");
    CovCall cov;
    STCHK(cov.begin(c, ix));
    return cov.end(classify_batch_device_impl(c, ix, p, d_bases, d_offs, d_bases2, d_offs2, n_reads, n_bases_total, d_results, d_taxcnt_tax, d_taxcnt_cnt, taxcnt_cap, n_taxcnt));
}

/* Device-side taxcnt slots of a batch: one per position bucket of every read (k_taxcnt_bound), sum floor((len + 3) / shift) + 2 <=
 * (bases + 3 reads) / shift + 2 reads.  The host arrays of the single-stream calls only receive the packed lists (download_packed), so their
 * capacity may be far smaller (2-3 entries per read is typical); MTB_ERR_CAPACITY reports what the lists need. */
static uint64_t taxcnt_device_slots(const mtb_params *p, uint64_t n_reads, uint64_t n_bases) {
    mtb_score_params sp; mtb_make_score_params(p, &sp);
    return (n_bases + 3 * n_reads) / (uint64_t)std::max(1, sp.dna_shift) + 2 * n_reads + 64;
}

static mtb_status classify_batch_impl(mtb_ctx *c, mtb_index *ix, const mtb_params *p, const char *bases, const uint64_t *offs, const char *bases2,
                                      const uint64_t *offs2, uint64_t n_reads, mtb_result *results, int32_t *taxcnt_tax, uint32_t *taxcnt_cnt,
                                      uint64_t taxcnt_cap, uint64_t *n_taxcnt) {
    HIPCHK(hipSetDevice(c->device));
    *n_taxcnt = 0;
    if (n_reads == 0) return MTB_OK;
    char *d_b, *d_b2; uint64_t *d_o, *d_o2; uint64_t nb;
    STCHK(upload_reads(c, p, bases, offs, bases2, offs2, n_reads, &d_b, &d_o, &d_b2, &d_o2, &nb));
    mtb_result *d_res; int32_t *d_tt; uint32_t *d_tc;
    /* one stream: the lists come back packed, the device arrays are sized here and taxcnt_cap only bounds what the host receives */
    const uint64_t dcap = c->lanes.size() < 2 ? std::max<uint64_t>(taxcnt_cap, taxcnt_device_slots(p, n_reads, nb)) : taxcnt_cap;
    STCHK(ensure(c, res_name(RES_ROWS, 0), n_reads, &d_res, BUF_IO)); STCHK(ensure(c, "tctax", dcap, &d_tt, BUF_IO)); STCHK(ensure(c, "tccnt", dcap, &d_tc, BUF_IO));
    mtb_status st = mtb_classify_batch_device(c, ix, p, d_b, d_o, d_b2, d_o2, n_reads, nb, d_res, d_tt, d_tc, dcap, n_taxcnt);
    if (st != MTB_OK) return st;
    if (c->lanes.size() < 2 && *n_taxcnt) return download_packed(c, d_res, d_tt, d_tc, n_reads, results, taxcnt_tax, taxcnt_cnt, n_taxcnt, taxcnt_cap);
    STCHK(d2h(c, results, d_res, n_reads * sizeof(mtb_result)));
    if (*n_taxcnt) { STCHK(d2h(c, taxcnt_tax, d_tt, *n_taxcnt * 4)); STCHK(d2h(c, taxcnt_cnt, d_tc, *n_taxcnt * 4)); }
    return MTB_OK;
}

mtb_status mtb_classify_batch(mtb_ctx *c, mtb_index *ix, const mtb_params *p, const char *bases, const uint64_t *offs, const char *bases2,
                              const uint64_t *offs2, uint64_t n_reads, mtb_result *results, int32_t *taxcnt_tax, uint32_t *taxcnt_cnt,
                              uint64_t taxcnt_cap, uint64_t *n_taxcnt) {
    if (!c || !ix || !p || !n_taxcnt) return fail(MTB_ERR_ARG, "NULL argument");
    CovCall cov;
    STCHK(cov.begin(c, ix));
    return cov.end(classify_batch_impl(c, ix, p, bases, offs, bases2, offs2, n_reads, results, taxcnt_tax, taxcnt_cnt, taxcnt_cap, n_taxcnt));
}

/* Host ingest at device rate: pinned host memory for the batch buffers, and the bases as 2-bit codes. */
void *mtb_host_alloc(size_t bytes) {
    void *p = nullptr;
    if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    return p;
}
void mtb_host_free(void *p) { if (p) { hipError_t e = hipHostFree(p); (void)e; } }

static uint64_t packed_slots(const uint32_t *lens, uint64_t n_reads) {
    uint64_t slots = 0;
    for (uint64_t i = 0; i < n_reads; i++) slots += (lens[i] + 7u) >> 3;
    return slots;
}
/* the three packed arrays of one mate into input buffer set `set`, on stream `on` */
static mtb_status copy_packed(mtb_ctx *c, const char *tag, int set, hipStream_t on, const uint8_t *packed2, const uint8_t *nmask, const uint32_t *lens,
                              uint64_t n_reads, uint64_t slots, uint8_t **d_p2, uint8_t **d_nm, uint32_t **d_len) {
    const std::string t = std::string(tag) + (set ? "#1" : "#0");
    STCHK(ensure(c, ("pk2" + t).c_str(), slots * 2 + 8, d_p2, BUF_IO)); STCHK(ensure(c, ("pkm" + t).c_str(), slots + 8, d_nm, BUF_IO)); STCHK(ensure(c, ("pklen" + t).c_str(), n_reads, d_len, BUF_IO));
    HIPCHK(hipMemcpyAsync(*d_p2, packed2, slots * 2, hipMemcpyHostToDevice, on));
    HIPCHK(hipMemcpyAsync(*d_nm, nmask, slots, hipMemcpyHostToDevice, on));
    HIPCHK(hipMemcpyAsync(*d_len, lens, n_reads * 4, hipMemcpyHostToDevice, on));
    return MTB_OK;
}
/* `prefetched`: the arrays already sit (or are arriving: the compute stream waits for the copy event) in set `set` */
static mtb_status upload_packed(mtb_ctx *c, const char *tag, int set, bool prefetched, const uint8_t *packed2, const uint8_t *nmask, const uint32_t *lens, uint64_t n_reads,
                                char **d_bases, uint64_t **d_offs, uint64_t *n_bases) {
    const std::string t(tag);
    uint8_t *d_p2, *d_nm; uint32_t *d_len, *d_sl; uint64_t *d_so, *d_ws;
    if (prefetched) {
        const std::string ts = t + (set ? "#1" : "#0");
        d_p2 = (uint8_t *)buf_get(c, "pk2" + ts).p; d_nm = (uint8_t *)buf_get(c, "pkm" + ts).p; d_len = (uint32_t *)buf_get(c, "pklen" + ts).p;
    } else STCHK(copy_packed(c, tag, set, c->stream, packed2, nmask, lens, n_reads, packed_slots(lens, n_reads), &d_p2, &d_nm, &d_len));
    STCHK(ensure(c, ("pksl" + t).c_str(), n_reads, &d_sl, BUF_IO)); STCHK(ensure(c, ("pkso" + t).c_str(), n_reads + 1, &d_so, BUF_IO));
    STCHK(ensure(c, ("offs" + t).c_str(), n_reads + 1, d_offs, BUF_IO)); STCHK(ensure(c, "scanws", scan_ws_elems(n_reads + 1), &d_ws));
    scan_launch<uint32_t, uint64_t, false>(c->stream, d_len, n_reads, true, *d_offs, d_ws);
    hipLaunchKernelGGL(k_pack_slots, dim3((uint32_t)((n_reads + 255) / 256)), dim3(256), 0, c->stream, (const uint32_t *)d_len, n_reads, d_sl);
    scan_launch<uint32_t, uint64_t, false>(c->stream, d_sl, n_reads, true, d_so, d_ws);
    uint64_t nb = 0;
    STCHK(d2h(c, &nb, *d_offs + n_reads, 8));
    STCHK(ensure(c, ("bases" + t).c_str(), nb + 8, d_bases, BUF_IO));
    hipLaunchKernelGGL(k_unpack_reads, dim3((uint32_t)std::min<uint64_t>(n_reads, 256ull * 64)), dim3(64), 0, c->stream, (const uint8_t *)d_p2, (const uint8_t *)d_nm,
                       (const uint64_t *)*d_offs, (const uint64_t *)d_so, n_reads, *d_bases);
    HIPCHK(hipGetLastError());
    *n_bases = nb;
    return MTB_OK;
}

} // extern "C"

static mtb_status wait_results(mtb_ctx *c) {
    if (c->down_pending) { HIPCHK(hipEventSynchronize(c->down_done)); c->down_pending = false; }
    return MTB_OK;
}

static mtb_status classify_packed_impl(mtb_ctx *c, mtb_index *ix, const mtb_params *p, const uint8_t *packed2, const uint8_t *nmask, const uint32_t *lens,
                                       const uint8_t *packed2_mate, const uint8_t *nmask_mate, const uint32_t *lens_mate, uint64_t n_reads,
                                       mtb_result *results, int32_t *taxcnt_tax, uint32_t *taxcnt_cnt, uint64_t taxcnt_cap, uint64_t *n_taxcnt, bool async) {
    if (!c || !ix || !p || !n_taxcnt) return fail(MTB_ERR_ARG, "NULL argument");
    HIPCHK(hipSetDevice(c->device));
    *n_taxcnt = 0;
    if (!async) STCHK(wait_results(c));          /* (a synchronous call after asynchronous ones: nothing stays in flight behind it) */
    if (n_reads == 0) return async ? wait_results(c) : MTB_OK;
    if (async && !c->down_stream) {
        HIPCHK(hipStreamCreateWithFlags(&c->down_stream, hipStreamNonBlocking));
        HIPCHK(hipEventCreateWithFlags(&c->down_ready, hipEventDisableTiming)); HIPCHK(hipEventCreateWithFlags(&c->down_done, hipEventDisableTiming));
    }
    /* asynchronous results: this call's rows and lists are built in the device buffer set the copies still in flight do not read */
    const int rset = async ? c->res_set : 0;
    if (!packed2 || !nmask || !lens) return fail(MTB_ERR_ARG, "packed2/nmask/lens NULL");
    char *d_b = nullptr, *d_b2 = nullptr; uint64_t *d_o = nullptr, *d_o2 = nullptr; uint64_t nb = 0, nb2 = 0;
    const bool timing = c->opt.host_timing != 0;      /* wall time of the call's three parts on stderr (the uploads are synchronised for it) */
    auto now = [] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double t0 = now();
    if (p->seq_mode == 2 && (!packed2_mate || !nmask_mate || !lens_mate)) return fail(MTB_ERR_ARG, "seq_mode 2 needs the mates");
    /* this batch may already be on its way (mtb_prefetch_batch_packed): then the compute stream only waits for the copy */
    int set = -1;
    for (int k = 0; k < 2; k++)
        if (c->pre[k].valid && c->pre[k].key == (const void *)packed2 && c->pre[k].n_reads == n_reads && (p->seq_mode != 2 || c->pre[k].key2 == (const void *)packed2_mate)) set = k;
    const bool pre = set >= 0;
    if (!pre) {
        /* not prefetched: upload on the compute stream into a set no outstanding prefetch (of a LATER batch) is filling */
        if (!c->pre[c->pk_set].valid) set = c->pk_set;
        else if (!c->pre[c->pk_set ^ 1].valid) set = c->pk_set ^ 1;
        else {      /* both sets hold prefetches nobody came for: let them finish, drop them */
            HIPCHK(hipStreamSynchronize(c->copy_stream));
            c->pre[0].valid = c->pre[1].valid = false; set = c->pk_set;
        }
    } else {
        c->pre[set].valid = false; c->prefetch_used++;
        HIPCHK(hipStreamWaitEvent(c->stream, c->copy_done[set], 0));
    }
    c->pk_set = set;
    STCHK(upload_packed(c, "", set, pre, packed2, nmask, lens, n_reads, &d_b, &d_o, &nb));
    if (p->seq_mode == 2) STCHK(upload_packed(c, "2", set, pre, packed2_mate, nmask_mate, lens_mate, n_reads, &d_b2, &d_o2, &nb2));
    if (c->unpacked[set]) { HIPCHK(hipEventRecord(c->unpacked[set], c->stream)); c->unpacked_rec[set] = true; }      /* the set may be overwritten by a prefetch from here on (stream order) */
    mtb_result *d_res; int32_t *d_tt; uint32_t *d_tc;
    const uint64_t dcap = c->lanes.size() < 2 ? std::max<uint64_t>(taxcnt_cap, taxcnt_device_slots(p, n_reads, nb + nb2)) : taxcnt_cap;     /* (as in mtb_classify_batch) */
    STCHK(ensure(c, res_name(RES_ROWS, rset), n_reads, &d_res, BUF_IO)); STCHK(ensure(c, "tctax", dcap, &d_tt, BUF_IO)); STCHK(ensure(c, "tccnt", dcap, &d_tc, BUF_IO));
    if (timing) HIPCHK(hipStreamSynchronize(c->stream));
    const double t1 = now();
    mtb_status st = mtb_classify_batch_device(c, ix, p, d_b, d_o, d_b2, d_o2, n_reads, nb + nb2, d_res, d_tt, d_tc, dcap, n_taxcnt);
    if (st != MTB_OK) return st;
    const double t2 = now();
    if (c->lanes.size() < 2 && *n_taxcnt) {
        if (async) {
            /* the previous call's copies have had this whole batch to finish: its results are the caller's from here on (mtb.h) */
            STCHK(wait_results(c));
            st = download_packed(c, d_res, d_tt, d_tc, n_reads, results, taxcnt_tax, taxcnt_cnt, n_taxcnt, taxcnt_cap, rset);
            if (st == MTB_OK) c->res_set ^= 1;
            return st;
        }
        st = download_packed(c, d_res, d_tt, d_tc, n_reads, results, taxcnt_tax, taxcnt_cnt, n_taxcnt, taxcnt_cap);
        if (timing) fprintf(stderr, "mtb_classify_batch_packed: %llu reads: upload + unpack %.1f ms, classify %.1f ms (device %.1f ms), pack + download %.1f ms\n",
                            (unsigned long long)n_reads, t1 - t0, t2 - t1, (double)c->stats.ms_total, now() - t2);
        return st;
    }
    /* (several streams, or a batch without a single taxID:count entry: plain copies) */
    if (async) STCHK(wait_results(c));
    STCHK(d2h(c, results, d_res, n_reads * sizeof(mtb_result)));
    if (*n_taxcnt) { STCHK(d2h(c, taxcnt_tax, d_tt, *n_taxcnt * 4)); STCHK(d2h(c, taxcnt_cnt, d_tc, *n_taxcnt * 4)); }
    return MTB_OK;
}

extern "C" {

mtb_status mtb_classify_batch_packed(mtb_ctx *c, mtb_index *ix, const mtb_params *p, const uint8_t *packed2, const uint8_t *nmask, const uint32_t *lens,
                                     const uint8_t *packed2_mate, const uint8_t *nmask_mate, const uint32_t *lens_mate, uint64_t n_reads,
                                     mtb_result *results, int32_t *taxcnt_tax, uint32_t *taxcnt_cnt, uint64_t taxcnt_cap, uint64_t *n_taxcnt) {
    if (!c || !ix || !p || !n_taxcnt) return fail(MTB_ERR_ARG, "NULL argument");
    CovCall cov;
    STCHK(cov.begin(c, ix));
    return cov.end(classify_packed_impl(c, ix, p, packed2, nmask, lens, packed2_mate, nmask_mate, lens_mate, n_reads, results, taxcnt_tax, taxcnt_cnt, taxcnt_cap, n_taxcnt, false));
}

/* The same with the results on their way back while the next batch computes: returns once the copies of the rows and of the packed
 * taxID:count lists into the caller's (pinned) arrays are QUEUED on a download stream of the context; *n_taxcnt is final on return
 * (MTB_ERR_CAPACITY as before, nothing queued).  The arrays of call k belong to the library until call k + 1 of this context returns --
 * whatever its status -- or until mtb_ctx_wait_results().  Two device-side result buffer sets alternate, so the batch in work never writes
 * what the copies in flight read.  (Classifier.cpp:81-125 hands a batch's results on when the batch is through; here the hand-over of
 * batch k happens one batch later and costs the device nothing.) */
mtb_status mtb_classify_batch_packed_async(mtb_ctx *c, mtb_index *ix, const mtb_params *p, const uint8_t *packed2, const uint8_t *nmask, const uint32_t *lens,
                                           const uint8_t *packed2_mate, const uint8_t *nmask_mate, const uint32_t *lens_mate, uint64_t n_reads,
                                           mtb_result *results, int32_t *taxcnt_tax, uint32_t *taxcnt_cnt, uint64_t taxcnt_cap, uint64_t *n_taxcnt) {
    if (!c || !ix || !p || !n_taxcnt) return fail(MTB_ERR_ARG, "NULL argument");
    CovCall cov;
    STCHK(cov.begin(c, ix));
    mtb_status st = cov.end(classify_packed_impl(c, ix, p, packed2, nmask, lens, packed2_mate, nmask_mate, lens_mate, n_reads, results, taxcnt_tax, taxcnt_cnt, taxcnt_cap, n_taxcnt, true));
    if (st != MTB_OK && c && c->down_pending) {     /* the contract holds on every path: the previous call's copies are complete when this one returns */
        hipError_t e = hipEventSynchronize(c->down_done); (void)e; c->down_pending = false;
    }
    return st;
}
mtb_status mtb_ctx_wait_results(mtb_ctx *c) {
    if (!c) return fail(MTB_ERR_ARG, "NULL argument");
    HIPCHK(hipSetDevice(c->device));
    return wait_results(c);
}

/* Starts the upload of the NEXT batch (the arrays mtb_classify_batch_packed will be called with) on the context's copy stream, into
 * the input buffer set the running batch does not use, and returns at once: the PCIe transfer of batch k+1 overlaps the kernels of
 * batch k (the serial producer this replaces: KmerExtractor.cpp:117-173 fills a batch, then the batch is processed).  Call it from the
 * context's thread right before the mtb_classify_batch_packed of batch k; the arrays must stay valid (pinned: mtb_host_alloc) until
 * the classify call for batch k+1 returns.  A prefetch that is not followed by its classify call is discarded. */
mtb_status mtb_prefetch_batch_packed(mtb_ctx *c, const mtb_params *p, const uint8_t *packed2, const uint8_t *nmask, const uint32_t *lens,
                                     const uint8_t *packed2_mate, const uint8_t *nmask_mate, const uint32_t *lens_mate, uint64_t n_reads) {
    if (!c || !p || !packed2 || !nmask || !lens) return fail(MTB_ERR_ARG, "NULL argument");
    HIPCHK(hipSetDevice(c->device));
    if (n_reads == 0 || c->lanes.size() > 1) return MTB_OK;
    if (p->seq_mode == 2 && (!packed2_mate || !nmask_mate || !lens_mate)) return fail(MTB_ERR_ARG, "seq_mode 2 needs the mates");
    if (!c->copy_stream) {
        HIPCHK(hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
        for (int k = 0; k < 2; k++) { HIPCHK(hipEventCreateWithFlags(&c->copy_done[k], hipEventDisableTiming)); HIPCHK(hipEventCreateWithFlags(&c->unpacked[k], hipEventDisableTiming)); }
    }
    /* the set that holds no outstanding prefetch: in protocol order (prefetch(k+1) right before classify(k)) batch k waits in one set and
     * the other was read by classify(k-1).  Both taken = the caller ran ahead of the protocol: nothing is prefetched, the batch is uploaded
     * by its own classify call. */
    int set = c->pk_set ^ 1;
    if (c->pre[set].valid) set ^= 1;
    if (c->pre[set].valid) return MTB_OK;
    if (c->unpacked_rec[set]) HIPCHK(hipStreamWaitEvent(c->copy_stream, c->unpacked[set], 0));     /* the call that last read the set has turned it into text */
    uint8_t *a, *b; uint32_t *l;
    const uint64_t s1 = packed_slots(lens, n_reads);
    STCHK(copy_packed(c, "", set, c->copy_stream, packed2, nmask, lens, n_reads, s1, &a, &b, &l));
    if (p->seq_mode == 2) STCHK(copy_packed(c, "2", set, c->copy_stream, packed2_mate, nmask_mate, lens_mate, n_reads, packed_slots(lens_mate, n_reads), &a, &b, &l));
    HIPCHK(hipEventRecord(c->copy_done[set], c->copy_stream));
    c->pre[set].key = packed2; c->pre[set].key2 = packed2_mate; c->pre[set].n_reads = n_reads; c->pre[set].valid = true;
    c->prefetch_issued++;
    return MTB_OK;
}

/* prefetches issued / prefetches a classify call found and used instead of uploading the batch itself (in protocol order: all of them) */
mtb_status mtb_ctx_prefetch_stats(mtb_ctx *c, uint64_t *issued, uint64_t *used) {
    if (!c) return fail(MTB_ERR_ARG, "NULL argument");
    if (issued) *issued = c->prefetch_issued;
    if (used) *used = c->prefetch_used;
    return MTB_OK;
}

/* ------------------------------------------------------------------ */
/* partitioned index: device-buffer stage calls  */
/* ------------------------------------------------------------------ */
} // extern "C"

/* pos[p] = number of entries of the sorted array with value < bounds[p]; stride in 8-byte words */
__global__ void k_lower_bounds(const uint64_t *__restrict__ v, uint64_t n, uint32_t stride, const uint64_t *__restrict__ bounds, uint32_t nb,
                               uint64_t *__restrict__ pos) {
    uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= nb) return;
    const uint64_t b = bounds[p];
    uint64_t lo = 0, hi = n;
    while (lo < hi) { uint64_t mid = (lo + hi) >> 1; if (v[mid * stride] < b) lo = mid + 1; else hi = mid; }
    pos[p] = lo;
}
static mtb_status lower_bounds(mtb_ctx *c, const uint64_t *d_v, uint64_t n, uint32_t stride, const uint64_t *bounds, uint32_t nb, uint64_t *pos) {
    uint64_t *d_b;
    STCHK(ensure(c, "lbounds", 2ull * nb, &d_b));
    STCHK(h2d(c, d_b, bounds, 8ull * nb));
    hipLaunchKernelGGL(k_lower_bounds, dim3((nb + 63) / 64), dim3(64), 0, c->stream, d_v, n, stride, (const uint64_t *)d_b, nb, d_b + nb);
    HIPCHK(hipGetLastError());
    return d2h(c, pos, d_b + nb, 8ull * nb);
}

extern "C" {

mtb_status mtb_index_slice(mtb_index *ix, uint64_t lo_value, uint64_t hi_value, int is_last, mtb_index **out) {
    if (!ix || !out) return fail(MTB_ERR_ARG, "NULL argument");
    mtb_ctx *c = ix->ctx;
    HIPCHK(hipSetDevice(c->device));
    uint64_t b[2] = {lo_value, hi_value}, pos[2] = {0, 0};
    if (ix->parent) return fail(MTB_ERR_ARG, "a view of a view: slice the parent instead");
    {   /* a view reads the parent's flat arrays: the parent goes flat now and stays flat while views are alive (ensure_packed /
           mtb_index_seal refuse, the fused join takes its flat-state kernel) */
        std::unique_lock<std::mutex> lk(ix->state_mu);
        ix->state_cv.wait(lk, [&] { return ix->users == 0; });
        STCHK(ensure_flat_locked(ix));
        ix->views++;
    }
    mtb_status st_lb = MTB_OK;
    if (ix->T) st_lb = lower_bounds(c, ix->d_values, ix->T, 1, b, 2, pos);
    if (st_lb != MTB_OK) { std::lock_guard<std::mutex> lk(ix->state_mu); ix->views--; return st_lb; }
    if (hi_value == UINT64_MAX) pos[1] = ix->T;
    mtb_index *sl = new mtb_index();
    sl->ctx = ix->ctx; sl->tax = ix->tax; sl->params = ix->params; sl->info_mask = ix->info_mask;
    sl->d_canon = ix->d_canon; sl->d_parent = ix->d_parent; sl->d_depth = ix->d_depth; sl->d_spparent = ix->d_spparent; sl->d_tax2species = ix->d_tax2species;
    sl->d_under = ix->d_under; sl->d_accleaf = ix->d_accleaf; sl->d_node = ix->d_node;
    sl->parent = ix;
    sl->own = false; sl->own_tax = false; sl->d_dir = nullptr; sl->d_dirbase = nullptr; sl->dir_L = 0;
    sl->d_values = ix->d_values + pos[0]; sl->d_info = ix->d_info + pos[0]; sl->T = pos[1] - pos[0];
    sl->match_last = !is_last || ix->match_last;
    {   /* a view gets a directory of its own (over its part of the parent's flat array): the owner side of the partitioned path joins through it */
        mtb_status sd = build_directory(c, sl);
        if (sd != MTB_OK) { mtb_index_close(sl); return sd; }
    }
    *out = sl;
    return MTB_OK;
}

mtb_status mtb_part_extract(mtb_ctx *c, const mtb_params *p, const char *d_bases, const uint64_t *d_offs, const char *d_bases2,
                            const uint64_t *d_offs2, uint64_t n_reads, const uint64_t *bounds, uint32_t n_parts, const mtb_kmer **d_sorted,
                            uint64_t *n_kmers, uint64_t *part_counts, uint64_t *part_starts) {
    if (!c || !p || !d_offs || !bounds || !d_sorted || !n_kmers || !part_counts || n_parts == 0) return fail(MTB_ERR_ARG, "NULL argument");
    HIPCHK(hipSetDevice(c->device));
    *d_sorted = nullptr; *n_kmers = 0;
    for (uint32_t q = 0; q < n_parts; q++) { part_counts[q] = 0; if (part_starts) part_starts[q] = 0; }
    c->part_n_reads = n_reads; c->part_max_len = 0; c->part_mode = 0; c->part_max_q = 0; c->part_nk_real = 0;
    if (n_reads == 0) return MTB_OK;
    int32_t *d_ql, *d_ql2;
    STCHK(ensure(c, "qlen", n_reads, &d_ql)); STCHK(ensure(c, "qlen2", n_reads, &d_ql2));
    mtb_kmer *d_s; Extracted ex; const Reads rd{d_bases, d_offs, d_bases2, d_offs2, n_reads};
    if (part_starts && p->seq_mode != 3 && !c->opt.part_exact) {
        /* the product path of short reads: single-pass extraction with ordinals, the sort on the leading amino-acid letters only (it is
         * there for the locality of the owners' directory joins) -- so a run is cut at PREFIX granularity and the metamers that share
         * their prefix with a bound go to both neighbours: a query finds candidates only in the range that holds its amino-acid
         * group (no group straddles a cut), the other owner emits nothing for it */
        const bool aa6 = p->kmer_format == 2;
        ExtractOpts tagged; tagged.single_pass = true; tagged.tag_ordinals = true; tagged.want_digits = aa6;
        STCHK(dev_extract(c, p, rd, d_ql, d_ql2, tagged, &ex));
        const uint64_t nk = ex.nk;
        if (ex.max_len + 3 < MTB_SLOT_MAX_POS && ex.max_q <= 384) {
            const int low_bits = aa6 ? 34 : 32;
            STCHK(dev_sort(c, ex.d_k, ex.nk, aa6 ? MTB_SORT_AA6 : 32, &d_s, ex.d_dig, /* all six letters */ 34));
            c->part_max_len = ex.max_len; c->part_mode = 1; c->part_max_q = ex.max_q; c->part_nk_real = ex.nk_real;
            std::vector<uint64_t> key(2 * n_parts), pos(2 * n_parts);
            for (uint32_t q = 0; q < n_parts; q++) {
                const uint64_t pre = bounds[q] >> low_bits;
                key[2 * q] = pre << low_bits;                                                       /* first record whose prefix is >= the bound's */
                key[2 * q + 1] = pre + 1 >= (1ull << (64 - low_bits)) ? UINT64_MAX : (pre + 1) << low_bits;      /* first record behind the bound's prefix group */
            }
            if (nk) STCHK(lower_bounds(c, (const uint64_t *)d_s, nk, 2, key.data(), 2 * n_parts, pos.data()));
            for (uint32_t q = 0; q < n_parts; q++) {
                const uint64_t lo = q == 0 ? 0 : pos[2 * q];
                const uint64_t hi = q + 1 < n_parts ? (key[2 * (q + 1) + 1] == UINT64_MAX ? nk : pos[2 * (q + 1) + 1]) : nk;
                part_starts[q] = lo; part_counts[q] = hi > lo ? hi - lo : 0;
            }
            *d_sorted = d_s; *n_kmers = nk;
            return MTB_OK;
        }
    }
    STCHK(dev_extract(c, p, rd, d_ql, d_ql2, /* two passes, untagged: exact order */ ExtractOpts(), &ex));
    const uint64_t nk = ex.nk;
    /* partition boundaries are amino-acid-part boundaries (bit 24), finer than the 32-bit tiles of the fused path: 5 passes */
    STCHK(dev_sort(c, ex.d_k, ex.nk, 24, &d_s, /* binary passes: no digit array, no letter pairs */ nullptr, 0));
    c->part_max_len = ex.max_len;
    std::vector<uint64_t> pos(n_parts);
    if (nk) STCHK(lower_bounds(c, (const uint64_t *)d_s, nk, 2, bounds, n_parts, pos.data()));
    for (uint32_t q = 0; q < n_parts; q++) { uint64_t hi = q + 1 < n_parts ? pos[q + 1] : nk; part_counts[q] = hi >= pos[q] ? hi - pos[q] : 0; if (part_starts) part_starts[q] = pos[q]; }
    if (nk && pos[0] != 0) return fail(MTB_ERR_ARG, "bounds[0] must be 0");
    *d_sorted = d_s; *n_kmers = nk;
    return MTB_OK;
}

mtb_status mtb_part_join(mtb_ctx *c, mtb_index *ix, const mtb_kmer *d_kmers, uint64_t n, mtb_match *d_out, uint64_t cap, uint64_t *count) {
    if (!c || !ix || !count) return fail(MTB_ERR_ARG, "NULL argument");
    HIPCHK(hipSetDevice(c->device));
    *count = 0;
    if (n == 0 || ix->T == 0) return MTB_OK;
    if (ix->d_dir && !c->opt.part_exact) {
        /* the directory join, matches to a dense list: every record keeps its query's qinfo (with the ordinal tag of a slot-mode
         * batch) and says in `pad` whether it is the query's first match */
        JoinSegArgs sa; memset(&sa, 0, sizeof(sa));
        sa.list = 1; sa.ovf = d_out; sa.ovf_cap = cap;
        return dev_join(c, ix, d_kmers, n, MatchList(), count, &sa, /* sort_low_bits: no window form for dense lists */ 32);
    }
    /* no directory over this range (MTB_NO_DIR, no room, a letter >= 21, a tiny range): the bisection join.  The runs of a slot-mode
     * batch are ordered on the leading amino-acid letters only (bits [34, 64) for kmer_format 2, mtb_part_extract), and k_join_bounds
     * derives a tile's target window from its first and last query under exactly that assumption -- so the sender's granularity is
     * passed on (the exact-order runs of the other modes are ordered on those bits too).  Records leave with pad = 0: the home rank
     * places them through the tails / the overflow list, which is slower but exact. */
    return dev_join(c, ix, d_kmers, n, MatchList{d_out, cap}, count, /* no slot segments */ nullptr, ix->params.kmer_format == 2 ? 34 : 32);
}

mtb_status mtb_part_score(mtb_ctx *c, mtb_index *ix, const mtb_params *p, mtb_match *d_matches, uint64_t n_matches, uint64_t n_reads,
                          mtb_result *results, int32_t *taxcnt_tax, uint32_t *taxcnt_cnt, uint64_t taxcnt_cap, uint64_t *n_taxcnt) {
    if (!c || !ix || !p || !results || !n_taxcnt) return fail(MTB_ERR_ARG, "NULL argument");
    if (n_reads != c->part_n_reads) return fail(MTB_ERR_ARG, "mtb_part_score must follow mtb_part_extract of the same batch on the same context");
    HIPCHK(hipSetDevice(c->device));
    *n_taxcnt = 0;
    if (n_reads == 0) return MTB_OK;
    if (n_matches >= (1ull << 32)) return fail(MTB_ERR_ARG, "more than 2^32-1 matches in one batch; split the batch");
    int32_t *d_ql, *d_ql2; uint32_t *d_rc; mtb_result *d_res; int32_t *d_tt; uint32_t *d_tc;
    STCHK(ensure(c, "qlen", n_reads, &d_ql)); STCHK(ensure(c, "qlen2", n_reads, &d_ql2));
    STCHK(ensure(c, "readcnt", n_reads, &d_rc));
    STCHK(ensure(c, res_name(RES_ROWS, 0), n_reads, &d_res, BUF_IO)); STCHK(ensure(c, "tctax", taxcnt_cap, &d_tt, BUF_IO)); STCHK(ensure(c, "tccnt", taxcnt_cap, &d_tc, BUF_IO));
    const ResultSink sink{d_res, d_tt, d_tc, taxcnt_cap, /* tc_base */ 0};
    if (c->part_mode == 1) {
        /* slot mode: the matches are placed into this rank's slot segments by their ordinal (what the fused join does at once),
         * then the slot scorers run */
        hipStream_t st = c->stream; SlotSegs sl;
        STCHK(make_slots(c, n_reads, c->part_max_q, d_rc, &sl));
        uint64_t ovf_cap = ovf_cap_first(c, n_matches);
        for (int attempt = 0; attempt < 3; attempt++) {
            STCHK(ensure(c, "ovf", ovf_cap, &sl.d_ovf));
            HIPCHK(hipMemsetAsync(d_rc, 0, n_reads * 4, st));
            HIPCHK(scal_clear(c, SC_JOIN_COUNT, 2));
            JoinSegArgs sa; memset(&sa, 0, sizeof(sa));
            sa.seg = sl.d_segm; sa.stride = sl.stride; sa.direct = sl.direct; sa.cursor = d_rc; sa.ovf = sl.d_ovf; sa.ovf_cap = ovf_cap; sa.ovf_counter = scal<unsigned long long>(c, SC_JOIN_COUNT); sa.epoch = sl.epoch;
            if (n_matches) hipLaunchKernelGGL(k_slot_place, dim3((uint32_t)((n_matches + 255) / 256)), dim3(256), 0, st, (const mtb_match *)d_matches, n_matches, sa, n_reads, scal<uint32_t>(c, SC_BAD_SEQ));
            HIPCHK(hipGetLastError());
            uint64_t sc[2]; STCHK(d2h(c, sc, scal<uint64_t>(c, SC_JOIN_COUNT), 16));       /* ... and SC_BAD_SEQ */
            if (sc[1] & 0xFFFFFFFFull) return fail(MTB_ERR_ARG, "match records with a sequenceID outside 1..n_reads");
            sl.n_ovf = sc[0];
            if (sl.n_ovf <= ovf_cap) break;
            if (attempt == 2) return fail(MTB_ERR_CAPACITY, "overflow list too small");
            ovf_cap = ovf_cap_regrown(sl.n_ovf);          /* slots written by the failed attempt are rewritten identically */
        }
        uint64_t nm = 0; memset(&c->stats, 0, sizeof(c->stats));
        STCHK(score_fixed_slots(c, ix, p, n_reads, ReadLens{d_ql, d_ql2, c->part_max_len}, c->part_nk_real, sl, sink, n_taxcnt, &nm, /* the partitioned path keeps the serial order */ false));
        c->stats.n_reads = n_reads; c->stats.n_matches = nm; c->stats.n_slot_reads = n_reads; c->stats.n_kmers = c->part_nk_real;
        STCHK(take_generic_reads(c, /* left at 0 when nothing was listed */ 0, &c->stats.n_generic_reads));
        return download_packed(c, d_res, d_tt, d_tc, n_reads, results, taxcnt_tax, taxcnt_cnt, n_taxcnt);
    }
    STCHK(count_reads(c, d_matches, n_matches, n_reads, d_rc));
    STCHK(score_join_order(c, ix, p, d_matches, n_matches, n_reads, d_rc, ReadLens{d_ql, d_ql2, c->part_max_len}, sink, n_taxcnt));
    return download_packed(c, d_res, d_tt, d_tc, n_reads, results, taxcnt_tax, taxcnt_cnt, n_taxcnt);
}

/* One batch on a group of contexts of THIS process, context k holding range k of the database (mtb_index_open_part(.., k, n)):
 * the C++ host's form of SURVEY 8(e) row 2 (metabuli_amd/parallel.py is the torch.distributed form of the same steps).
 *   1. every context: its contiguous share of the reads -> device, mtb_part_extract (ordinal tags, prefix-granular runs);
 *   2. exchange #1: run p of every context -> the owner of range p (hipMemcpyPeerAsync, device to device over xGMI), which joins
 *      every received run through its directory (mtb_part_join: runs stay sorted, no merge);
 *   3. exchange #2: the matches of source k's reads -> context k, which places them into its slot segments and scores
 *      (mtb_part_score);
 *   4. rows in input order, the taxID:count lists packed back to back behind taxcnt_off.
 * One host thread per context inside each step; the steps are separated by joins (the exchange needs every sender's counts). */
static mtb_status run_parallel_status(uint32_t n, const std::function<mtb_status(uint32_t)> &f, std::string *err) {
    std::vector<mtb_status> st(n, MTB_OK); std::vector<std::string> errs(n);
    std::vector<std::thread> th;
    for (uint32_t k = 0; k < n; k++) th.emplace_back([&, k] { st[k] = f(k); if (st[k] != MTB_OK) errs[k] = g_err; });
    for (auto &t : th) t.join();
    for (uint32_t k = 0; k < n; k++) if (st[k] != MTB_OK) { *err = errs[k]; return st[k]; }
    return MTB_OK;
}

mtb_status mtb_classify_batch_partitioned(mtb_ctx **ctxs, mtb_index **parts, uint32_t n, const uint64_t *bounds, const mtb_params *p,
                                          const char *bases, const uint64_t *offs, const char *bases2, const uint64_t *offs2, uint64_t n_reads,
                                          mtb_result *results, int32_t *taxcnt_tax, uint32_t *taxcnt_cnt, uint64_t taxcnt_cap, uint64_t *n_taxcnt) {
    if (!ctxs || !parts || !bounds || !p || !n_taxcnt || n == 0) return fail(MTB_ERR_ARG, "NULL argument");
    *n_taxcnt = 0;
    if (n_reads == 0) return MTB_OK;
    if (!bases || !offs || !results) return fail(MTB_ERR_ARG, "NULL argument");
    const bool paired = p->seq_mode == 2;
    if (paired && (!bases2 || !offs2)) return fail(MTB_ERR_ARG, "seq_mode 2 needs bases2/offs2");
    struct Rank {
        uint64_t lo = 0, hi = 0;                          /* its reads */
        const mtb_kmer *d_sorted = nullptr; uint64_t nk = 0;
        std::vector<uint64_t> counts, starts;             /* runs by owner */
        std::vector<uint64_t> m_count, m_start;           /* as an owner: matches per source, their start in its match buffer */
        mtb_match *d_matches = nullptr;                   /* as an owner */
        std::vector<mtb_result> res; std::vector<int32_t> tt; std::vector<uint32_t> tc; uint64_t ntc = 0;
    };
    /* direct device-to-device copies over xGMI where the devices can reach each other (without peer access hipMemcpyPeerAsync stages
     * through host memory); enabling it twice is reported as an error that means "already on" */
    for (uint32_t i = 0; i < n; i++) for (uint32_t j = 0; j < n; j++) {
        if (!ctxs[i] || !ctxs[j] || ctxs[i]->device == ctxs[j]->device) continue;
        int can = 0;
        if (hipDeviceCanAccessPeer(&can, ctxs[i]->device, ctxs[j]->device) != hipSuccess) { (void)hipGetLastError(); continue; }
        if (!can) continue;
        if (hipSetDevice(ctxs[i]->device) != hipSuccess) { (void)hipGetLastError(); continue; }
        const hipError_t e = hipDeviceEnablePeerAccess(ctxs[j]->device, 0);
        if (e != hipSuccess) (void)hipGetLastError();
    }
    std::vector<Rank> R(n);
    for (uint32_t k = 0; k < n; k++) { R[k].lo = n_reads * k / n; R[k].hi = n_reads * (k + 1) / n; R[k].counts.assign(n, 0); R[k].starts.assign(n, 0); R[k].m_count.assign(n, 0); R[k].m_start.assign(n, 0); }
    std::string err;
    /* 1. reads to their device, extraction */
    mtb_status st = run_parallel_status(n, [&](uint32_t k) -> mtb_status {
        mtb_ctx *c = ctxs[k]; Rank &r = R[k];
        const uint64_t m = r.hi - r.lo;
        if (m == 0) return MTB_OK;
        HIPCHK(hipSetDevice(c->device));
        std::vector<uint64_t> o(m + 1), o2(paired ? m + 1 : 0);
        for (uint64_t i = 0; i <= m; i++) o[i] = offs[r.lo + i] - offs[r.lo];
        if (paired) for (uint64_t i = 0; i <= m; i++) o2[i] = offs2[r.lo + i] - offs2[r.lo];
        char *d_b, *d_b2; uint64_t *d_o, *d_o2; uint64_t nb;
        STCHK(upload_reads(c, p, bases + offs[r.lo], o.data(), paired ? bases2 + offs2[r.lo] : nullptr, paired ? o2.data() : nullptr, m, &d_b, &d_o, &d_b2, &d_o2, &nb));
        return mtb_part_extract(c, p, d_b, d_o, d_b2, d_o2, m, bounds, n, &r.d_sorted, &r.nk, r.counts.data(), r.starts.data());
    }, &err);
    if (st != MTB_OK) return fail(st, err);
    /* 2. runs to their owners, joins */
    st = run_parallel_status(n, [&](uint32_t q) -> mtb_status {
        mtb_ctx *c = ctxs[q]; Rank &own = R[q];
        HIPCHK(hipSetDevice(c->device));
        uint64_t n_in = 0;
        for (uint32_t k = 0; k < n; k++) n_in += R[k].counts[q];
        if (n_in == 0) return MTB_OK;
        mtb_kmer *d_in;
        STCHK(ensure(c, "xkmers", n_in, &d_in));
        uint64_t at = 0;
        for (uint32_t k = 0; k < n; k++) {
            const uint64_t cnt = R[k].counts[q];
            if (cnt) HIPCHK(hipMemcpyPeerAsync(d_in + at, c->device, R[k].d_sorted + R[k].starts[q], ctxs[k]->device, cnt * sizeof(mtb_kmer), c->stream));
            at += cnt;
        }
        HIPCHK(hipStreamSynchronize(c->stream));
        uint64_t cap = n_in + n_in / 4 + 1024;
        for (int attempt = 0; attempt < 4; attempt++) {
            STCHK(ensure(c, "xmatches", cap, &own.d_matches));
            uint64_t used = 0, need = 0; bool again = false;
            at = 0;
            for (uint32_t k = 0; k < n && !again; k++) {
                const uint64_t cnt = R[k].counts[q];
                uint64_t got = 0;
                own.m_start[k] = used;
                if (cnt) {
                    mtb_status sj = mtb_part_join(c, parts[q], d_in + at, cnt, own.d_matches + used, cap - used, &got);
                    if (sj == MTB_ERR_CAPACITY) { again = true; need = used + got; }
                    else if (sj != MTB_OK) return sj;
                }
                own.m_count[k] = got; used += got; at += cnt;
            }
            if (!again) return MTB_OK;
            cap = need + need / 2 + 1024;                 /* (the runs behind the one that did not fit are not counted yet) */
        }
        return fail(MTB_ERR_CAPACITY, "match buffer of a range owner too small");
    }, &err);
    if (st != MTB_OK) return fail(st, err);
    /* 3. matches home, scoring */
    st = run_parallel_status(n, [&](uint32_t k) -> mtb_status {
        mtb_ctx *c = ctxs[k]; Rank &r = R[k];
        const uint64_t m = r.hi - r.lo;
        if (m == 0) return MTB_OK;
        HIPCHK(hipSetDevice(c->device));
        uint64_t nm = 0;
        for (uint32_t q = 0; q < n; q++) nm += R[q].m_count[k];
        mtb_match *d_home;
        STCHK(ensure(c, "xhome", nm, &d_home));
        uint64_t at = 0;
        for (uint32_t q = 0; q < n; q++) {
            const uint64_t cnt = R[q].m_count[k];
            if (cnt) HIPCHK(hipMemcpyPeerAsync(d_home + at, c->device, R[q].d_matches + R[q].m_start[k], ctxs[q]->device, cnt * sizeof(mtb_match), c->stream));
            at += cnt;
        }
        HIPCHK(hipStreamSynchronize(c->stream));
        r.res.resize(m);
        uint64_t cap = 24 * m + 4096;
        for (;;) {
            r.tt.resize(cap); r.tc.resize(cap);
            mtb_status ss = mtb_part_score(c, parts[k], p, d_home, nm, m, r.res.data(), r.tt.data(), r.tc.data(), cap, &r.ntc);
            if (ss == MTB_ERR_CAPACITY && r.ntc > cap) { cap = r.ntc; continue; }
            return ss;
        }
    }, &err);
    if (st != MTB_OK) return fail(st, err);
    /* 4. rows in input order, lists packed */
    uint64_t used = 0;
    for (uint32_t k = 0; k < n; k++) for (uint64_t i = 0; i < R[k].res.size(); i++) used += R[k].res[i].n_taxcnt;
    *n_taxcnt = used;
    if (used > taxcnt_cap) return fail(MTB_ERR_CAPACITY, "taxcnt buffers too small");
    if (used >= (1ull << 32)) return fail(MTB_ERR_ARG, "more than 2^32-1 taxcnt entries in one batch; split the batch");
    uint64_t at = 0;
    for (uint32_t k = 0; k < n; k++) {
        Rank &r = R[k];
        for (uint64_t i = 0; i < r.res.size(); i++) {
            mtb_result x = r.res[i];
            for (uint32_t j = 0; j < x.n_taxcnt; j++) { taxcnt_tax[at + j] = r.tt[x.taxcnt_off + j]; taxcnt_cnt[at + j] = r.tc[x.taxcnt_off + j]; }
            x.taxcnt_off = (uint32_t)at; at += x.n_taxcnt;
            results[r.lo + i] = x;
        }
    }
    return MTB_OK;
}

#ifdef MTB_SCORE_PHASE_CYCLES
/* profiling build only: read and reset the k_score phase cycle counters */
mtb_status mtb_debug_phase_cycles(mtb_ctx *c, unsigned long long *out4) {
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipMemcpyFromSymbol(out4, HIP_SYMBOL(mtb_phase_cycles), 8 * MTB_NPHASE));      /* out4: MTB_NPHASE (16) counters */
    unsigned long long z[MTB_NPHASE] = {0};
    HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(mtb_phase_cycles), z, 8 * MTB_NPHASE));
    /* join phases ride in out4[16..23] */
    HIPCHK(hipMemcpyFromSymbol(out4 + MTB_NPHASE, HIP_SYMBOL(mtb_join_cycles), 64));
    HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(mtb_join_cycles), z, 64));
    return MTB_OK;
}
#endif

#ifdef MTB_FAST_DEBUG
/* debugging build only: read and reset the k_score_fast exit counters */
mtb_status mtb_debug_fast_reasons(mtb_ctx *c, unsigned long long *out8) {
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipMemcpyFromSymbol(out8, HIP_SYMBOL(mtb_fast_reasons), 256));      /* 32 counters */
    unsigned long long z[32] = {0};
    HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(mtb_fast_reasons), z, 256));
    return MTB_OK;
}
#endif

#ifdef MTB_PLACEMENT_DEBUG
/* experiment build only (libmtb_place.so): release one workspace buffer and park `pad_bytes` of HBM so that its next allocation
 * lands somewhere else -- does the join's process-to-process spread follow the placement of the slot buffer? */
mtb_status mtb_debug_move_buffer(mtb_ctx *c, const char *name, unsigned long long pad_bytes) {
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    void *pad = nullptr;
    if (pad_bytes) { hipError_t e = hipMalloc(&pad, pad_bytes); if (e != hipSuccess) { (void)hipGetLastError(); pad = nullptr; } }   /* never freed: the process ends with the experiment */
    release(c, name);             /* after the pad is in place */
    return MTB_OK;
}
#endif

mtb_status mtb_ctx_join_footprint(mtb_ctx *c, mtb_index *ix, mtb_join_footprint *out) {
    if (!c || !ix || !out) return fail(MTB_ERR_ARG, "NULL argument");
    memset(out, 0, sizeof(*out));
    if (!c->last_sorted || !ix->d_dir || c->last_sub_batches != 1) return fail(MTB_ERR_UNSUPPORTED, "no directory join of a single sub-batch to look at");
    HIPCHK(hipSetDevice(c->device));
    const uint64_t nb = ix->dir_buckets, T = ix->T;
    const uint64_t w_b = (nb >> 5) + 1, w_d = (((nb + 1) * 4) >> 11) + 1, w_t = ((T * 8) >> 11) + 1;
    uint32_t *bm = nullptr; unsigned long long *d_cnt = nullptr;
    if (hipMalloc((void **)&bm, (w_b + w_d + w_t) * 4) != hipSuccess) { (void)hipGetLastError(); return fail(MTB_ERR_OOM, "no HBM for the footprint bitmaps"); }
    if (hipMalloc((void **)&d_cnt, 32) != hipSuccess) { (void)hipGetLastError(); (void)hipFree(bm); return fail(MTB_ERR_OOM, "no HBM for the footprint counters"); }
    mtb_status st = MTB_OK;
    hipError_t e = hipMemsetAsync(bm, 0, (w_b + w_d + w_t) * 4, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(d_cnt, 0, 32, c->stream);
    if (e == hipSuccess && c->last_sorted_n) {
        hipLaunchKernelGGL(k_join_footprint, dim3((uint32_t)((c->last_sorted_n + 255) / 256)), dim3(256), 0, c->stream, c->last_sorted, c->last_sorted_n, dir_view(ix), T,
                           bm, bm + w_b, bm + w_b + w_d, d_cnt);
        hipLaunchKernelGGL(k_popcount_words, dim3(2048), dim3(256), 0, c->stream, (const uint32_t *)bm, w_b, d_cnt + 1);
        hipLaunchKernelGGL(k_popcount_words, dim3(2048), dim3(256), 0, c->stream, (const uint32_t *)(bm + w_b), w_d, d_cnt + 2);
        hipLaunchKernelGGL(k_popcount_words, dim3(2048), dim3(256), 0, c->stream, (const uint32_t *)(bm + w_b + w_d), w_t, d_cnt + 3);
        e = hipGetLastError();
    }
    unsigned long long h[4] = {0, 0, 0, 0};
    if (e == hipSuccess) e = hipMemcpyAsync(h, d_cnt, 32, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) st = fail(MTB_ERR_DEVICE, std::string("join footprint: ") + hipGetErrorString(e));
    (void)hipFree(bm); (void)hipFree(d_cnt);
    out->n_queries = h[0]; out->distinct_buckets = h[1]; out->dir_sectors = h[2]; out->target_sectors = h[3]; out->n_buckets = nb; out->n_targets = T;
    return st;
}

mtb_status mtb_index_run_histogram(mtb_index *ix, uint64_t *hist64) {
    if (!ix || !hist64) return fail(MTB_ERR_ARG, "NULL argument");
    memset(hist64, 0, 64 * sizeof(uint64_t));
    if (ix->T == 0) return MTB_OK;
    mtb_ctx *c = ix->ctx;
    HIPCHK(hipSetDevice(c->device));
    STCHK(ensure_flat(ix));
    unsigned long long *d_h = nullptr;
    if (hipMalloc((void **)&d_h, 64 * 8) != hipSuccess) { (void)hipGetLastError(); return fail(MTB_ERR_OOM, "no HBM for the histogram"); }
    hipError_t e = hipMemsetAsync(d_h, 0, 64 * 8, c->stream);
    if (e == hipSuccess) { hipLaunchKernelGGL(k_index_run_hist, dim3((uint32_t)std::min<uint64_t>((ix->T + 255) / 256, 1u << 20)), dim3(256), 0, c->stream, (const uint64_t *)ix->d_values, ix->T, d_h); e = hipGetLastError(); }
    if (e == hipSuccess) e = hipMemcpyAsync(hist64, d_h, 64 * 8, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    (void)hipFree(d_h);
    if (e != hipSuccess) return fail(MTB_ERR_DEVICE, std::string("run histogram: ") + hipGetErrorString(e));
    return MTB_OK;
}

mtb_status mtb_ctx_join_run_histogram(mtb_ctx *c, mtb_index *ix, uint64_t *hist64) {
    if (!c || !ix || !hist64) return fail(MTB_ERR_ARG, "NULL argument");
    memset(hist64, 0, 64 * sizeof(uint64_t));
    if (!c->last_sorted || !ix->d_dir || c->last_sub_batches != 1) return fail(MTB_ERR_UNSUPPORTED, "no directory join of a single sub-batch to look at");
    HIPCHK(hipSetDevice(c->device));
    unsigned long long *d_h = nullptr;
    if (hipMalloc((void **)&d_h, 64 * 8) != hipSuccess) { (void)hipGetLastError(); return fail(MTB_ERR_OOM, "no HBM for the histogram"); }
    mtb_status st = MTB_OK;
    {
        IndexUse use;                                       /* the array keeps the state it is in while the kernel reads it */
        mtb_index *own = state_owner(ix);
        st = use.acquire(ix, own->packed);
        const uint64_t limit = ix->T ? ix->T - (ix->match_last ? 0 : 1) : 0;
        hipError_t e = st == MTB_OK ? hipMemsetAsync(d_h, 0, 64 * 8, c->stream) : hipSuccess;
        if (st == MTB_OK && e == hipSuccess && c->last_sorted_n) {
            const dim3 g((uint32_t)((c->last_sorted_n + 255) / 256));
            if (own->packed) hipLaunchKernelGGL((k_join_run_hist<true>), g, dim3(256), 0, c->stream, c->last_sorted, c->last_sorted_n, (const uint64_t *)ix->d_values, limit, dir_view(ix), d_h);
            else hipLaunchKernelGGL((k_join_run_hist<false>), g, dim3(256), 0, c->stream, c->last_sorted, c->last_sorted_n, (const uint64_t *)ix->d_values, limit, dir_view(ix), d_h);
            e = hipGetLastError();
        }
        if (st == MTB_OK && e == hipSuccess) e = hipMemcpyAsync(hist64, d_h, 64 * 8, hipMemcpyDeviceToHost, c->stream);
        if (st == MTB_OK && e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (st == MTB_OK && e != hipSuccess) st = fail(MTB_ERR_DEVICE, std::string("join run histogram: ") + hipGetErrorString(e));
    }
    (void)hipFree(d_h);
    return st;
}

/* db.parameters of a database directory applied to *p (what mtb_index_open does first), without opening anything */
mtb_status mtb_db_parameters(const char *dbdir, mtb_params *p) {
    if (!dbdir || !p) return fail(MTB_ERR_ARG, "NULL argument");
    int reduced = 0;
    mtbhost::load_db_parameters(dbdir, p, &reduced);
    return MTB_OK;
}

/* Grows the big workspace buffers of a short-read batch of that size ahead of time: the metamer buffers of the extractor and the sort,
 * their digit arrays, the slot segments (hipMalloc of ~35 GB for 4 M reads costs several hundred milliseconds -- the first batch of a
 * run used to pay them).  The sizes are those the first batch will ask for if its reads look like the estimate; a batch that needs
 * more simply grows a buffer as before.  MAY BE CALLED FROM ANOTHER THREAD while the context's thread is inside mtb_index_open (the
 * buffer table is locked per access): a driver hides the allocations behind the database load. */
mtb_status mtb_ctx_reserve(mtb_ctx *c, const mtb_params *p, uint64_t n_reads, uint64_t n_bases) {
    if (!c || !p) return fail(MTB_ERR_ARG, "NULL argument");
    if (n_reads == 0 || n_bases == 0 || p->seq_mode == 3) return MTB_OK;
    HIPCHK(hipSetDevice(c->device));
    std::lock_guard<std::mutex> rlk(c->reserve_mu);
    /* an index open on this context that runs short of device memory cancels the reservation (open_make_room): checked between buffers */
#define MTB_RESERVE_STEP(call) do { if (c->reserve_cancel) return MTB_OK; STCHK(call); } while (0)
    const uint32_t grid = (uint32_t)std::min<uint64_t>(n_reads, 256ull * 256);
    const uint64_t cap = extract_cap_guess(c, p, n_bases, grid);
    mtb_kmer *k; uint16_t *dg; mtb_slot16 *sg;
    MTB_RESERVE_STEP(ensure(c, "kmersA", cap, &k)); MTB_RESERVE_STEP(ensure(c, "kmersB", cap, &k));
    if (p->kmer_format == 2) { MTB_RESERVE_STEP(ensure(c, "digA", cap + 8, &dg)); MTB_RESERVE_STEP(ensure(c, "digB", cap + 8, &dg)); }
    /* slot segments: metamers of the longest read guessed from the mean length (six frames of L/3 - 7 windows per mate; syncmer
     * selection keeps a little over half), one direct slot each + the tail */
    const int mates = p->seq_mode == 2 ? 2 : 1;
    const double L = (double)n_bases / (double)n_reads / mates;
    const double per_read = std::max(0.0, L / 3.0 - 7.0) * 6.0 * mates * (p->syncmer ? 0.56 : 1.0) * 1.10;
    uint32_t direct, stride;
    slot_geometry(c, (uint32_t)std::min<double>(per_read, (double)MTB_SLOT_MAX_Q), &direct, &stride);
    MTB_RESERVE_STEP(ensure(c, "segm", n_reads * (uint64_t)stride, &sg));
#undef MTB_RESERVE_STEP
    return MTB_OK;
}

mtb_status mtb_last_batch_stats(mtb_ctx *c, mtb_batch_stats *out) {
    if (!c || !out) return fail(MTB_ERR_ARG, "NULL argument");
    *out = c->stats;
    return MTB_OK;
}

/* ------------------------------------------------------------------ */
/* synthetic index                                                     */
/* ------------------------------------------------------------------ */
mtb_status mtb_synth_index(mtb_ctx *c, uint64_t seed, uint64_t n_filler, int32_t filler_tax_lo, int32_t filler_tax_hi,
                           const uint64_t *real_values, const int32_t *real_taxids, uint64_t n_real, uint64_t *d_values,
                           uint32_t *d_info, uint64_t *n_out) {
    if (!c || !d_values || !d_info || !n_out) return fail(MTB_ERR_ARG, "NULL argument");
    HIPCHK(hipSetDevice(c->device));
    if (n_filler > MTB_AA_SPACE) return fail(MTB_ERR_ARG, "n_filler exceeds the amino-acid 8-mer space");
    if (n_filler && filler_tax_hi < filler_tax_lo) return fail(MTB_ERR_ARG, "empty filler taxon range");
    FillerParams P;
    memset(&P, 0, sizeof(P));
    P.seed = seed; P.n_filler = n_filler;
    uint64_t pairs = (n_filler + 1) / 2;
    P.stride = pairs ? MTB_AA_SPACE / pairs : 2;
    if (P.stride < 2) P.stride = 2;
    P.tax_lo = filler_tax_lo; P.tax_span = (uint32_t)(filler_tax_hi - filler_tax_lo + 1);
    for (int i = 0; i < 64; i++) {           /* valid codon ids per amino acid, ascending */
        uint32_t aa = c->h_tabs.codon[i] & 31u, cid = c->h_tabs.codon[i] >> 5;
        bool have = false;
        for (int k = 0; k < P.ncid[aa]; k++) have |= (P.cids[aa][k] == cid);
        if (!have) P.cids[aa][P.ncid[aa]++] = (uint8_t)cid;
    }
    for (int aa = 0; aa < 21; aa++) std::sort(P.cids[aa], P.cids[aa] + P.ncid[aa]);
    uint64_t *d_rv = nullptr, *d_pos = nullptr; int32_t *d_rt = nullptr;
    if (n_real) {
        for (uint64_t i = 1; i < n_real; i++) if (real_values[i] < real_values[i - 1]) return fail(MTB_ERR_ARG, "real_values must be sorted");
        STCHK(ensure(c, "synth_rv", n_real, &d_rv)); STCHK(ensure(c, "synth_rt", n_real, &d_rt)); STCHK(ensure(c, "synth_pos", n_real, &d_pos));
        STCHK(h2d(c, d_rv, real_values, n_real * 8)); STCHK(h2d(c, d_rt, real_taxids, n_real * 4));
        hipLaunchKernelGGL(k_synth_real_pos, dim3((uint32_t)((n_real + 255) / 256)), dim3(256), 0, c->stream, P, (const uint64_t *)d_rv, n_real, d_pos);
    }
    if (n_filler) hipLaunchKernelGGL(k_synth_fill, dim3((uint32_t)std::min<uint64_t>((n_filler + 255) / 256, 1ull << 20)), dim3(256), 0, c->stream, P, (const uint64_t *)d_rv, n_real, d_values, d_info);
    if (n_real) hipLaunchKernelGGL(k_synth_place_real, dim3((uint32_t)((n_real + 255) / 256)), dim3(256), 0, c->stream, (const uint64_t *)d_rv,
                                   (const int32_t *)d_rt, (const uint64_t *)d_pos, n_real, d_values, d_info);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));
    release(c, "synth_rv"); release(c, "synth_rt"); release(c, "synth_pos");
    *n_out = n_filler + n_real;
    return MTB_OK;
}

mtb_status mtb_extract_targets(mtb_ctx *c, const mtb_params *p, const char *genome, uint64_t len, uint64_t *values, uint64_t cap, uint64_t *count) {
    /* convenience wrapper: one sequence, long-read geometry, values only */
    if (!c || !p || !count) return fail(MTB_ERR_ARG, "NULL argument");
    mtb_params q = *p; q.seq_mode = 3;
    uint64_t offs[2] = {0, len};
    std::vector<mtb_kmer> tmp(cap);
    uint64_t n = 0;
    mtb_status st = mtb_extract(c, &q, genome, offs, nullptr, nullptr, 1, tmp.data(), cap, &n, nullptr, nullptr);
    *count = n;
    if (st != MTB_OK) return st;
    for (uint64_t i = 0; i < n; i++) values[i] = tmp[i].value;
    return MTB_OK;
}

} // extern "C"

/* ------------------------------------------------------------------ */
/* block scan (kernels_extract_blocks.h)                               */
/* ------------------------------------------------------------------ */
static mtb_status block_scan_params(const mtb_params *p) {
    if (p->kmer_format != 2) return fail(MTB_ERR_UNSUPPORTED, "block extraction implements kmer_format 2 only (what the reference's build passes to IndexCreator)");
    if (p->syncmer && (p->smer_len < 1 || p->smer_len > 8)) return fail(MTB_ERR_ARG, "smer_len out of range");
    return MTB_OK;
}
/* every block inside its sequence; the message names the first one that is not */
static mtb_status check_blocks(const uint64_t *offs, uint64_t n_seqs, const mtb_seq_block *blocks, uint64_t n_blocks) {
    if (n_blocks >= (1ull << 32)) return fail(MTB_ERR_ARG, "2^32 or more blocks in one call");
    for (uint64_t i = 0; i < n_seqs; i++)
        if (offs[i + 1] < offs[i]) return fail(MTB_ERR_ARG, "offs must not decrease (sequence " + std::to_string(i) + ")");
    for (uint64_t i = 0; i < n_blocks; i++) {
        const mtb_seq_block &k = blocks[i];
        const std::string who = "block " + std::to_string(i) + ": ";
        if (k.seq >= n_seqs) return fail(MTB_ERR_ARG, who + "seq " + std::to_string(k.seq) + " of " + std::to_string(n_seqs) + " sequences");
        if (k.end < k.start) return fail(MTB_ERR_ARG, who + "end " + std::to_string(k.end) + " before start " + std::to_string(k.start));
        const uint64_t len = offs[k.seq + 1] - offs[k.seq];
        if (k.end >= len) return fail(MTB_ERR_ARG, who + "end " + std::to_string(k.end) + " beyond sequence " + std::to_string(k.seq) + " of " + std::to_string(len) + " bases");
    }
    return MTB_OK;
}
struct BlockScan { BlockScanArgs a; uint64_t *d_base = nullptr; uint64_t total = 0; uint32_t grid = 0; };
/* checks, uploads, piece table, count launch, offsets: leaves what the emit launch needs.  total = records the blocks yield. */
static mtb_status dev_count_blocks(mtb_ctx *c, const mtb_params *p, const char *bases, const uint64_t *offs, uint64_t n_seqs,
                                   const mtb_seq_block *blocks, uint64_t n_blocks, BlockScan *bs) {
    *bs = BlockScan();
    STCHK(check_blocks(offs, n_seqs, blocks, n_blocks));
    if (n_blocks == 0) return MTB_OK;
    mtb_params q = *p; q.seq_mode = 3;
    char *d_b, *d_b2; uint64_t *d_o, *d_o2; uint64_t nb;
    STCHK(upload_reads(c, &q, bases, offs, nullptr, nullptr, n_seqs, &d_b, &d_o, &d_b2, &d_o2, &nb));
    mtb_seq_block *d_blk; uint32_t *d_np; uint64_t *d_ps, *d_ws;
    STCHK(ensure(c, "blk", n_blocks, &d_blk, BUF_IO)); STCHK(ensure(c, "blk_np", n_blocks, &d_np)); STCHK(ensure(c, "blk_ps", n_blocks + 1, &d_ps));
    STCHK(ensure(c, "scanws", scan_ws_elems(n_blocks + 1), &d_ws));
    STCHK(h2d(c, d_blk, blocks, n_blocks * sizeof(mtb_seq_block)));
    hipLaunchKernelGGL(k_block_pieces, dim3((uint32_t)((n_blocks + 255) / 256)), dim3(256), 0, c->stream, (const mtb_seq_block *)d_blk, n_blocks, d_np);
    scan_launch<uint32_t, uint64_t, false>(c->stream, d_np, n_blocks, true, d_ps, d_ws);
    HIPCHK(hipGetLastError());
    uint64_t n_pieces = 0;
    STCHK(d2h(c, &n_pieces, d_ps + n_blocks, 8));
    if (n_pieces == 0) return MTB_OK;
    uint32_t *d_cnt;
    STCHK(ensure(c, "blk_cnt", n_pieces, &d_cnt)); STCHK(ensure(c, "blk_base", n_pieces + 1, &bs->d_base));
    STCHK(ensure(c, "scanws", scan_ws_elems(n_pieces + 1), &d_ws));
    bs->a = BlockScanArgs{d_b, d_o, d_blk, n_blocks, d_ps, n_pieces, p->syncmer, p->smer_len};
    bs->grid = (uint32_t)std::min<uint64_t>(n_pieces, 256ull * 256);
    hipLaunchKernelGGL((k_extract_blocks<0>), dim3(bs->grid), dim3(64), 0, c->stream, bs->a, c->d_tabs, d_cnt, (const uint64_t *)nullptr,
                       (const int32_t *)nullptr, (mtb_kmer *)nullptr, (uint64_t *)nullptr, (uint32_t *)nullptr);
    scan_launch<uint32_t, uint64_t, false>(c->stream, d_cnt, n_pieces, true, bs->d_base, d_ws);
    HIPCHK(hipGetLastError());
    STCHK(d2h(c, &bs->total, bs->d_base + n_pieces, 8));
    return MTB_OK;
}

extern "C" {

mtb_status mtb_extract_blocks(mtb_ctx *c, const mtb_params *p, const char *bases, const uint64_t *offs, uint64_t n_seqs,
                              const mtb_seq_block *blocks, uint64_t n_blocks, uint64_t *values, uint32_t *block_of, uint64_t cap, uint64_t *count) {
    if (!c || !p || !count || (n_seqs && (!bases || !offs)) || (n_blocks && !blocks) || (cap && !values)) return fail(MTB_ERR_ARG, "NULL argument");
    HIPCHK(hipSetDevice(c->device));
    *count = 0;
    STCHK(block_scan_params(p));
    BlockScan bs;
    STCHK(dev_count_blocks(c, p, bases, offs, n_seqs, blocks, n_blocks, &bs));
    *count = bs.total;
    if (bs.total > cap) return fail(MTB_ERR_CAPACITY, "value buffer too small");
    if (bs.total == 0) return MTB_OK;
    uint64_t *d_v; uint32_t *d_bo = nullptr;
    STCHK(ensure(c, "blk_val", bs.total, &d_v, BUF_IO));
    if (block_of) STCHK(ensure(c, "blk_of", bs.total, &d_bo, BUF_IO));
    hipLaunchKernelGGL((k_extract_blocks<2>), dim3(bs.grid), dim3(64), 0, c->stream, bs.a, c->d_tabs, (uint32_t *)nullptr, (const uint64_t *)bs.d_base,
                       (const int32_t *)nullptr, (mtb_kmer *)nullptr, d_v, d_bo);
    HIPCHK(hipGetLastError());
    STCHK(d2h(c, values, d_v, bs.total * 8));
    if (block_of) STCHK(d2h(c, block_of, d_bo, bs.total * 4));
    return MTB_OK;
}

} // extern "C"

/* ------------------------------------------------------------------ */
/* database build / merge (kernels_build.h)                            */
/* ------------------------------------------------------------------ */
struct mtb_builder {
    mtb_ctx *ctx = nullptr;
    mtb_params params;
    mtbhost::Taxonomy tax;           /* loaded once; every index finish() returns starts from a copy */
    int32_t *d_canon = nullptr;      /* canon[] alone: what mtb_tax_exists reads (add_index checks its ids on the device) */
    mtb_kmer *d_rec = nullptr;       /* the records: {value, taxid in qinfo} */
    uint64_t n = 0, cap = 0;
    hipEvent_t ev[MTB_BUILD_STAGES] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};      /* stage boundaries of finish(): the builder's own, not the context's batch events */
    float ms[MTB_BUILD_STAGES] = {0, 0, 0, 0, 0, 0};
    uint64_t last_n = 0, last_groups = 0, last_long = 0;
};

/* room for `more` records behind the ones held (the list is copied when it grows) */
static mtb_status builder_reserve(mtb_builder *b, uint64_t more) {
    const uint64_t need = b->n + more;
    if (need <= b->cap) return MTB_OK;
    const uint64_t want = std::max<uint64_t>(need, b->cap + b->cap / 2);
    mtb_kmer *p = nullptr;
    hipError_t e = hipMalloc((void **)&p, want * sizeof(mtb_kmer));
    uint64_t got = want;
    if (e != hipSuccess && want > need) { (void)hipGetLastError(); got = need; e = hipMalloc((void **)&p, need * sizeof(mtb_kmer)); }
    if (e != hipSuccess) { (void)hipGetLastError(); return fail(MTB_ERR_OOM, "not enough HBM for the builder's record list (" + std::to_string(need) + " records)"); }
    if (b->n) {
        hipError_t e2 = hipMemcpyAsync(p, b->d_rec, b->n * sizeof(mtb_kmer), hipMemcpyDeviceToDevice, b->ctx->stream);
        if (e2 == hipSuccess) e2 = hipStreamSynchronize(b->ctx->stream);
        if (e2 != hipSuccess) { hipError_t e3 = hipFree(p); (void)e3; return fail(MTB_ERR_DEVICE, std::string("builder: copy of the record list: ") + hipGetErrorString(e2)); }
    }
    if (b->d_rec) { hipError_t e3 = hipFree(b->d_rec); (void)e3; }
    b->d_rec = p; b->cap = got;
    return MTB_OK;
}
static mtb_status builder_check_taxids(const mtb_builder *b, const int32_t *taxids, uint64_t n) {
    for (uint64_t i = 0; i < n; i++)
        if (b->tax.cn(taxids[i]) < 0) return fail(MTB_ERR_ARG, "taxid " + std::to_string(taxids[i]) + " is not in the taxonomy (nodes.dmp / merged.dmp)");
    return MTB_OK;
}
static dim3 grid256(uint64_t n) { return dim3((uint32_t)((n + 255) / 256)); }

/* Records keyed (species, taxid) above the value (k_build_keys, k_merge_sort_key) into the order (value, species, taxid): a stable sort
 * by (species, taxid), the swap of the key's halves back into `rec`, a stable sort by every bit.  dev_sort's other buffer is "kmersB";
 * *sorted = where the result lies.  `between`, if given, is recorded between the two sorts. */
static mtb_status dev_sort_groups(mtb_ctx *c, mtb_kmer *rec, uint64_t n, int bits, mtb_kmer **sorted, hipEvent_t between = nullptr) {
    STCHK(dev_sort(c, rec, n, mtb_build_key_first_bit(bits), sorted, nullptr, 0));
    hipLaunchKernelGGL(k_build_swap, grid256(n), dim3(256), 0, c->stream, (const mtb_kmer *)*sorted, n, bits, rec);
    HIPCHK(hipGetLastError());
    if (between) HIPCHK(hipEventRecord(between, c->stream));
    return dev_sort(c, rec, n, /* every bit */ 0, sorted, nullptr, 0);
}

/* Records in that order -> one entry per (value, species) group, its info the LCA of the group's taxids: heads -> scan -> the group
 * count G, for which `arrays` names the output (G + 1 values, G info entries; the builder allocates its index there, the merge takes
 * workspace) -> k_build_reduce, and k_build_reduce_long for the groups that one listed as too long for a lane. */
static mtb_status dev_reduce_groups(mtb_ctx *c, const mtb_kmer *d_s, uint64_t n, const mtb_tax_view &tv,
                                    const std::function<mtb_status(uint64_t groups, uint64_t **d_values, uint32_t **d_info)> &arrays, uint64_t *G, uint32_t *n_long) {
    hipStream_t st = c->stream;
    uint32_t *d_head, *d_pos, *d_list; uint64_t *d_ws;
    STCHK(ensure(c, "bhead", n, &d_head)); STCHK(ensure(c, "bpos", n + 1, &d_pos));
    STCHK(ensure(c, "scanws", scan_ws_elems(n + 1), &d_ws));
    hipLaunchKernelGGL(k_build_heads, grid256(n), dim3(256), 0, st, d_s, n, d_head);
    scan_launch<uint32_t, uint32_t, false>(st, d_head, n, true, d_pos, (uint32_t *)d_ws);
    HIPCHK(hipGetLastError());
    uint32_t n_groups = 0;
    STCHK(d2h(c, &n_groups, d_pos + n, 4));
    *G = n_groups;
    uint64_t *d_values = nullptr; uint32_t *d_info = nullptr;
    STCHK(arrays(*G, &d_values, &d_info));
    STCHK(ensure(c, "blist", n / (MTB_BUILD_LANE_MAX + 1) + 2, &d_list));
    uint32_t *d_nlist = scal<uint32_t>(c, SC_JOIN_COUNT);
    HIPCHK(scal_clear(c, SC_JOIN_COUNT));
    hipLaunchKernelGGL(k_build_reduce, grid256(n), dim3(256), 0, st, d_s, n, (const uint32_t *)d_head, (const uint32_t *)d_pos, tv, d_values, d_info, d_list, d_nlist);
    HIPCHK(hipGetLastError());
    STCHK(d2h(c, n_long, d_nlist, 4));
    if (*n_long) {
        hipLaunchKernelGGL(k_build_reduce_long, dim3(std::min<uint32_t>(*n_long, 1u << 16)), dim3(64), 0, st, d_s, n, (const uint32_t *)d_head, (const uint32_t *)d_pos, tv,
                           d_values, d_info, (const uint32_t *)d_list, (const uint32_t *)d_nlist);
        HIPCHK(hipGetLastError());
    }
    return MTB_OK;
}

extern "C" {

mtb_status mtb_builder_create(mtb_ctx *c, const char *taxonomy_dir, const mtb_params *params, mtb_builder **out) {
    if (!c || !taxonomy_dir || !params || !out) return fail(MTB_ERR_ARG, "NULL argument");
    if (params->kmer_format != 1 && params->kmer_format != 2) return fail(MTB_ERR_UNSUPPORTED, "only kmer_format 1 and 2 are implemented");
    if (params->syncmer && (params->smer_len < 1 || params->smer_len > 8)) return fail(MTB_ERR_ARG, "smer_len out of range");
    HIPCHK(hipSetDevice(c->device));
    {   /* Reduced_alphabet is a property of a database and mtb_params has no field for it: the one place a builder can meet it is a
         * taxonomy directory that sits inside such a database (DB/taxonomy), whose DB/db.parameters says so (documented in mtb.h) */
        mtb_params q = *params; int reduced_aa = 0;
        mtbhost::load_db_parameters(std::string(taxonomy_dir) + "/..", &q, &reduced_aa);
        if (reduced_aa) return fail(MTB_ERR_UNSUPPORTED, "Reduced_alphabet 1 is not implemented");
    }
    mtb_builder *b = new mtb_builder();
    b->ctx = c; b->params = *params; b->params.skip_redundancy = 1;
    std::string err;
    if (!mtbhost::load_taxonomy(taxonomy_dir, &b->tax, &err)) { delete b; return fail(MTB_ERR_IO, err); }
    const size_t nt = (size_t)b->tax.max_id + 1;
    hipError_t e = hipMalloc((void **)&b->d_canon, nt * 4);
    if (e != hipSuccess) { (void)hipGetLastError(); delete b; return fail(MTB_ERR_OOM, "not enough HBM for the builder's taxonomy table"); }
    e = hipMemcpy(b->d_canon, b->tax.canon.data(), nt * 4, hipMemcpyHostToDevice);
    for (int k = 0; k < MTB_BUILD_STAGES && e == hipSuccess; k++) e = hipEventCreate(&b->ev[k]);
    if (e != hipSuccess) { (void)hipGetLastError(); mtb_builder_destroy(b); return fail(MTB_ERR_DEVICE, std::string("builder: taxonomy upload / events: ") + hipGetErrorString(e)); }
    *out = b;
    return MTB_OK;
}

void mtb_builder_destroy(mtb_builder *b) {
    if (!b) return;
    hipError_t e = hipSuccess;
    if (b->d_rec) e = hipFree(b->d_rec);
    if (b->d_canon) e = hipFree(b->d_canon);
    for (int k = 0; k < MTB_BUILD_STAGES; k++) if (b->ev[k]) e = hipEventDestroy(b->ev[k]);
    (void)e;
    delete b;
}

uint64_t mtb_builder_num_records(const mtb_builder *b) { return b ? b->n : 0; }

mtb_status mtb_builder_capacity(const mtb_builder *b, uint64_t *max_records) {
    if (!b || !max_records) return fail(MTB_ERR_ARG, "NULL argument");
    HIPCHK(hipSetDevice(b->ctx->device));
    size_t fr = 0, tot = 0;
    HIPCHK(hipMemGetInfo(&fr, &tot));
    const uint64_t avail = (uint64_t)fr + b->cap * sizeof(mtb_kmer) + held_bytes(b->ctx, BUF_FIXED);
    *max_records = std::min<uint64_t>(avail / 72, 0xFFFFFFFFull);
    return MTB_OK;
}

mtb_status mtb_builder_add_records(mtb_builder *b, const uint64_t *values, const int32_t *taxids, uint64_t n) {
    if (!b || (n && (!values || !taxids))) return fail(MTB_ERR_ARG, "NULL argument");
    if (n == 0) return MTB_OK;
    mtb_ctx *c = b->ctx;
    HIPCHK(hipSetDevice(c->device));
    STCHK(builder_check_taxids(b, taxids, n));
    STCHK(builder_reserve(b, n));
    const uint64_t CHUNK = 1ull << 24;         /* staged through two small device arrays */
    uint64_t *d_v; int32_t *d_t;
    STCHK(ensure(c, "bvals", std::min(n, CHUNK), &d_v, BUF_IO)); STCHK(ensure(c, "btax", std::min(n, CHUNK), &d_t, BUF_IO));
    for (uint64_t i0 = 0; i0 < n; i0 += CHUNK) {
        const uint64_t m = std::min(CHUNK, n - i0);
        HIPCHK(hipMemcpyAsync(d_v, values + i0, m * 8, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(d_t, taxids + i0, m * 4, hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(k_build_pack, grid256(m), dim3(256), 0, c->stream, (const uint64_t *)d_v, (const int32_t *)d_t, m, b->d_rec + b->n + i0);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    if (n > CHUNK) { release(c, "bvals"); release(c, "btax"); }
    b->n += n;
    return MTB_OK;
}

mtb_status mtb_builder_add_sequences(mtb_builder *b, const char *bases, const uint64_t *offs, const int32_t *taxids, uint64_t n_seqs) {
    if (!b || (n_seqs && (!bases || !offs || !taxids))) return fail(MTB_ERR_ARG, "NULL argument");
    if (n_seqs == 0) return MTB_OK;
    mtb_ctx *c = b->ctx;
    HIPCHK(hipSetDevice(c->device));
    STCHK(builder_check_taxids(b, taxids, n_seqs));
    /* the toy and bench databases' geometry: every sequence in all six frames, long-read mode (no gene prediction) */
    mtb_params q = b->params; q.seq_mode = 3;
    char *d_b, *d_b2; uint64_t *d_o, *d_o2; uint64_t nb;
    STCHK(upload_reads(c, &q, bases, offs, nullptr, nullptr, n_seqs, &d_b, &d_o, &d_b2, &d_o2, &nb));
    int32_t *d_ql, *d_ql2, *d_t;
    STCHK(ensure(c, "qlen", n_seqs, &d_ql)); STCHK(ensure(c, "qlen2", n_seqs, &d_ql2)); STCHK(ensure(c, "btax", n_seqs, &d_t, BUF_IO));
    STCHK(h2d(c, d_t, taxids, n_seqs * 4));
    ExtractOpts two_pass; two_pass.want_max_len = false;
    Extracted ex;
    STCHK(dev_extract(c, &q, Reads{d_b, d_o, nullptr, nullptr, n_seqs}, d_ql, d_ql2, two_pass, &ex));
    if (ex.nk == 0) return MTB_OK;
    STCHK(builder_reserve(b, ex.nk));
    hipLaunchKernelGGL(k_build_append, grid256(ex.nk), dim3(256), 0, c->stream, (const mtb_kmer *)ex.d_k, ex.nk, (const int32_t *)d_t, n_seqs, b->d_rec + b->n);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));
    b->n += ex.nk;
    return MTB_OK;
}

mtb_status mtb_builder_add_blocks(mtb_builder *b, const char *bases, const uint64_t *offs, const int32_t *taxids, uint64_t n_seqs,
                                  const mtb_seq_block *blocks, uint64_t n_blocks) {
    if (!b || (n_seqs && (!bases || !offs || !taxids)) || (n_blocks && !blocks)) return fail(MTB_ERR_ARG, "NULL argument");
    mtb_ctx *c = b->ctx;
    HIPCHK(hipSetDevice(c->device));
    STCHK(block_scan_params(&b->params));
    STCHK(builder_check_taxids(b, taxids, n_seqs));
    BlockScan bs;
    STCHK(dev_count_blocks(c, &b->params, bases, offs, n_seqs, blocks, n_blocks, &bs));
    if (bs.total == 0) return MTB_OK;
    STCHK(builder_reserve(b, bs.total));
    int32_t *d_t;
    STCHK(ensure(c, "btax", n_seqs, &d_t, BUF_IO));
    STCHK(h2d(c, d_t, taxids, n_seqs * 4));
    /* the records go straight behind the builder's list: no intermediate metamer list, no append pass */
    hipLaunchKernelGGL((k_extract_blocks<1>), dim3(bs.grid), dim3(64), 0, c->stream, bs.a, c->d_tabs, (uint32_t *)nullptr, (const uint64_t *)bs.d_base,
                       (const int32_t *)d_t, b->d_rec + b->n, (uint64_t *)nullptr, (uint32_t *)nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));
    b->n += bs.total;
    return MTB_OK;
}

mtb_status mtb_builder_add_index(mtb_builder *b, mtb_index *ix) {
    if (!b || !ix) return fail(MTB_ERR_ARG, "NULL argument");
    if (ix->parent) return fail(MTB_ERR_ARG, "a view cannot be added to a builder: add its parent");
    mtb_ctx *c = b->ctx;
    if (ix->ctx->device != c->device) return fail(MTB_ERR_ARG, "the index lives on another device than the builder");
    if (ix->params.kmer_format != b->params.kmer_format || (ix->params.syncmer != 0) != (b->params.syncmer != 0) ||
        (b->params.syncmer && ix->params.smer_len != b->params.smer_len))
        return fail(MTB_ERR_ARG, "the index's kmer_format / syncmer / smer_len differ from the builder's");
    if (ix->T == 0) return MTB_OK;
    HIPCHK(hipSetDevice(c->device));
    STCHK(builder_reserve(b, ix->T));
    IndexUse use;                                /* a sealed or packed index goes back to {value[], info[]}, as for mtb_index_download, and stays flat (a join's hold) until the d2h below has synchronised the stream */
    STCHK(use.acquire(ix, false));
    unsigned long long *d_bad = scal<unsigned long long>(c, SC_JOIN_COUNT);
    HIPCHK(hipMemsetAsync(d_bad, 0xFF, 8, c->stream));
    mtb_tax_view tv; memset(&tv, 0, sizeof(tv)); tv.canon = b->d_canon; tv.max_taxid = b->tax.max_id;
    hipLaunchKernelGGL(k_build_from_index, grid256(ix->T), dim3(256), 0, c->stream, (const uint64_t *)ix->d_values, (const uint32_t *)ix->d_info, ix->T, ix->info_mask, tv,
                       b->d_rec + b->n, d_bad);
    HIPCHK(hipGetLastError());
    unsigned long long bad = 0;
    STCHK(d2h(c, &bad, d_bad, 8));
    if (bad != ~0ull) {
        mtb_kmer r;
        STCHK(d2h(c, &r, b->d_rec + b->n + bad, sizeof(r)));
        return fail(MTB_ERR_ARG, "taxid " + std::to_string((int32_t)(uint32_t)r.qinfo) + " of the index (entry " + std::to_string(bad) + ") is not in the builder's taxonomy");
    }
    b->n += ix->T;
    return MTB_OK;
}

mtb_status mtb_builder_finish(mtb_builder *b, mtb_index **out) {
    if (!b || !out) return fail(MTB_ERR_ARG, "NULL argument");
    *out = nullptr;
    const uint64_t n = b->n;
    if (n == 0) return fail(MTB_ERR_ARG, "the builder holds no records");
    if (n >= (1ull << 32)) return fail(MTB_ERR_ARG, "2^32 or more records in one finish (" + std::to_string(n) + "): the device sort takes fewer than 2^32; build in parts (mtb_build --max-records) and merge the written parts with mtb_merge_databases");
    mtb_ctx *c = b->ctx;
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    mtb_index *ix = new mtb_index();
    /* on every way out but the good one: the half-built index goes, and so do the input-sized sort and reduce buffers */
    struct Guard { mtb_index *ix; mtb_ctx *c; ~Guard() { if (!ix) return; mtb_index_close(ix); c->last_sorted = nullptr; c->last_sorted_n = 0; std::lock_guard<std::mutex> lk(c->reserve_mu); release_workspace(c); } } guard{ix, c};
    ix->ctx = c; ix->params = b->params; ix->own = true; ix->info_mask = 0xFFFFFFFFu;
    ix->tax = b->tax;
    {   /* the union of the ids added = the new database's taxID_list: the species table comes from it as at index open */
        const size_t nt = (size_t)b->tax.max_id + 1;
        uint8_t *d_seen;
        STCHK(ensure(c, "wseen", nt + 1, &d_seen));
        HIPCHK(hipMemsetAsync(d_seen, 0, nt + 1, st));
        hipLaunchKernelGGL(k_build_mark, grid256(n), dim3(256), 0, st, (const mtb_kmer *)b->d_rec, n, d_seen, b->tax.max_id);
        HIPCHK(hipGetLastError());
        std::vector<uint8_t> seen(nt);
        STCHK(d2h(c, seen.data(), d_seen, nt));
        release(c, "wseen");
        std::vector<int32_t> ids;
        for (size_t t = 0; t < nt; t++) if (seen[t]) ids.push_back((int32_t)t);
        mtbhost::build_tax2species(&ix->tax, ids.data(), ids.size());
    }
    STCHK(upload_taxonomy(ix));
    const int bits = mtb_build_tax_bits(b->tax.max_id);
    hipEvent_t *ev = b->ev;
    mtb_kmer *d_a, *d_s;
    STCHK(ensure(c, "kmersA", n, &d_a));
    HIPCHK(hipEventRecord(ev[0], st));
    hipLaunchKernelGGL(k_build_keys, grid256(n), dim3(256), 0, st, (const mtb_kmer *)b->d_rec, n, (const int32_t *)ix->d_tax2species, b->tax.max_id, bits, d_a);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(ev[1], st));
    STCHK(dev_sort_groups(c, d_a, n, bits, &d_s, ev[2]));
    HIPCHK(hipEventRecord(ev[3], st));
    uint64_t G = 0; uint32_t n_long = 0;
    STCHK(dev_reduce_groups(c, d_s, n, tax_view(ix), [&](uint64_t groups, uint64_t **d_values, uint32_t **d_info) -> mtb_status {
        HIPCHK(hipEventRecord(ev[4], st));
        hipError_t e = hipMalloc((void **)&ix->d_values, (groups + 1) * 8);
        if (e == hipSuccess) e = hipMalloc((void **)&ix->d_info, std::max<uint64_t>(groups, 1) * 4);
        if (e != hipSuccess) { (void)hipGetLastError(); return fail(MTB_ERR_OOM, "not enough HBM for the built index (" + std::to_string(groups) + " entries)"); }
        *d_values = ix->d_values; *d_info = ix->d_info; return MTB_OK; }, &G, &n_long));
    HIPCHK(hipEventRecord(ev[5], st));
    HIPCHK(hipStreamSynchronize(st));
    for (int k = 0; k < 5; k++) { float ms = 0; if (hipEventElapsedTime(&ms, ev[k], ev[k + 1]) != hipSuccess) (void)hipGetLastError(); b->ms[k] = ms; }
    { float ms = 0; if (hipEventElapsedTime(&ms, ev[0], ev[5]) != hipSuccess) (void)hipGetLastError(); b->ms[5] = ms; }
    b->last_n = n; b->last_groups = G; b->last_long = n_long;
    ix->T = G;
    /* the sort's and the reduce's buffers are as large as the input: the workspace goes back (as when an index open needs the room) before the directory is built */
    c->last_sorted = nullptr; c->last_sorted_n = 0;
    { std::lock_guard<std::mutex> lk(c->reserve_mu); release_workspace(c); }
    STCHK(build_directory(c, ix));
    { hipError_t e = hipFree(b->d_rec); (void)e; b->d_rec = nullptr; b->n = 0; b->cap = 0; }      /* empty, reusable */
    guard.ix = nullptr;
    *out = ix;
    return MTB_OK;
}

mtb_status mtb_builder_last_finish_stats(const mtb_builder *b, mtb_build_stats *out) {
    if (!b || !out) return fail(MTB_ERR_ARG, "NULL argument");
    for (int k = 0; k < MTB_BUILD_STAGES; k++) out->ms[k] = b->ms[k];
    out->n_records = b->last_n; out->n_entries = b->last_groups; out->n_long_groups = b->last_long;
    return MTB_OK;
}

} // extern "C"


/* ------------------------------------------------------------------ */
/* streamed merge of databases (kernels_merge.h, host/merge_plan.h)    */
/* ------------------------------------------------------------------ */
/* out[0, na + nb) = the merge of the sorted lists a and b (device pointers; out overlaps neither) */
static mtb_status dev_merge2(mtb_ctx *c, const mtb_kmer *a, uint64_t na, const mtb_kmer *b, uint64_t nb, mtb_kmer *out) {
    if (na == 0 || nb == 0) {
        if (na + nb) HIPCHK(hipMemcpyAsync(out, na ? a : b, (na + nb) * sizeof(mtb_kmer), hipMemcpyDeviceToDevice, c->stream));
        return MTB_OK;
    }
    const uint64_t total = na + nb, n_tiles = (total + MTB_MERGE_TILE - 1) / MTB_MERGE_TILE;
    uint64_t *d_split;
    STCHK(ensure(c, "mrgsplit", n_tiles + 1, &d_split));
    hipLaunchKernelGGL(k_merge_partition, dim3((uint32_t)((n_tiles + 1 + 255) / 256)), dim3(256), 0, c->stream, a, na, b, nb, n_tiles, d_split);
    hipLaunchKernelGGL(k_merge_tile, dim3((uint32_t)n_tiles), dim3(MTB_MERGE_THREADS), 0, c->stream, a, b, total, (const uint64_t *)d_split, out);
    HIPCHK(hipGetLastError());
    return MTB_OK;
}

/* k sorted lists that lie back to back in `ping` (list i = records [off[i], off[i + 1])) -> one sorted list: a pairwise tree between
 * the two buffers, an odd list of a level is copied.  *result = the buffer that holds it. */
static mtb_status dev_merge_tree(mtb_ctx *c, mtb_kmer *ping, mtb_kmer *pong, std::vector<uint64_t> off, mtb_kmer **result) {
    mtb_kmer *src = ping, *dst = pong;
    while (off.size() > 2) {
        std::vector<uint64_t> next;
        for (size_t i = 0; i + 1 < off.size(); i += 2) {
            next.push_back(off[i]);
            const uint64_t na = off[i + 1] - off[i], nb = i + 2 < off.size() ? off[i + 2] - off[i + 1] : 0;
            STCHK(dev_merge2(c, src + off[i], na, src + off[i + 1], nb, dst + off[i]));
        }
        next.push_back(off.back());
        off.swap(next);
        std::swap(src, dst);
    }
    *result = src;
    return MTB_OK;
}

namespace {
struct MergeSource { std::string dir; uint32_t info_mask = 0xFFFFFFFFu; };
double ms_since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
/* the device side of a clade filter: keep[] and met[] by species key, and the per-tile counts, bases and scan workspace */
struct CladeDev { const uint8_t *d_keep = nullptr; uint64_t n_keep = 0; uint8_t *d_met = nullptr; uint32_t *d_count = nullptr; uint64_t *d_base = nullptr, *d_ws = nullptr; };
}

/* out[0, *kept) = the records of rec[0, n) whose species key indexes keep[] with a non-zero byte, in order (device pointers; out
 * holds n records and does not overlap rec; f.d_count / d_base / d_ws hold n / 2048 + 1, + 2 and scan_ws_elems(n / 2048 + 2) entries).
 * *first_bad = the first record whose key is >= n_keep, ~0 if none.  Ends with the download of the count: the stream is idle. */
static mtb_status dev_clade_filter(mtb_ctx *c, const mtb_kmer *rec, uint64_t n, const CladeDev &f, mtb_kmer *out, uint64_t *kept, uint64_t *first_bad) {
    *kept = 0; *first_bad = ~0ull;
    if (n == 0) return MTB_OK;
    hipStream_t st = c->stream;
    const uint64_t n_tiles = (n + MTB_CLADE_TILE - 1) / MTB_CLADE_TILE;
    unsigned long long *d_bad = scal<unsigned long long>(c, SC_JOIN_COUNT);
    HIPCHK(hipMemsetAsync(d_bad, 0xFF, 8, st));
    hipLaunchKernelGGL(k_clade_count, dim3((uint32_t)n_tiles), dim3(MTB_CLADE_THREADS), 0, st, rec, n, f.d_keep, f.n_keep, f.d_met, f.d_count, d_bad);
    scan_launch<uint32_t, uint64_t, false>(st, (const uint32_t *)f.d_count, n_tiles, true, f.d_base, f.d_ws);
    hipLaunchKernelGGL(k_clade_compact, dim3((uint32_t)n_tiles), dim3(MTB_CLADE_THREADS), 0, st, rec, n, f.d_keep, f.n_keep, (const uint64_t *)f.d_base, out);
    HIPCHK(hipGetLastError());
    unsigned long long bad = 0;
    STCHK(d2h(c, kept, f.d_base + n_tiles, 8));
    STCHK(d2h(c, &bad, d_bad, 8));
    *first_bad = bad;
    return MTB_OK;
}

extern "C" {

mtb_status mtb_filter_records(mtb_ctx *c, const mtb_kmer *rec, uint64_t n, const uint8_t *keep, uint64_t n_keep, mtb_kmer *out, uint64_t *n_out) {
    if (!c || !n_out || (n && (!rec || !out)) || (n_keep && !keep)) return fail(MTB_ERR_ARG, "NULL argument");
    *n_out = 0;
    if (n == 0) return MTB_OK;
    if (n >> 32) return fail(MTB_ERR_ARG, "2^32 or more records in one call");
    HIPCHK(hipSetDevice(c->device));
    const uint64_t n_tiles = (n + MTB_CLADE_TILE - 1) / MTB_CLADE_TILE;
    mtb_kmer *d_in, *d_out; uint8_t *d_keep; CladeDev f;
    STCHK(ensure(c, "mrgA", n, &d_in)); STCHK(ensure(c, "mrgB", n, &d_out));
    STCHK(ensure(c, "cladekeep", n_keep + 1, &d_keep));
    STCHK(ensure(c, "bhead", n_tiles + 1, &f.d_count)); STCHK(ensure(c, "bpos", n_tiles + 2, &f.d_base));
    STCHK(ensure(c, "scanws", scan_ws_elems(n_tiles + 2), &f.d_ws));
    STCHK(h2d(c, d_in, rec, n * sizeof(mtb_kmer)));
    if (n_keep) STCHK(h2d(c, d_keep, keep, n_keep));
    f.d_keep = d_keep; f.n_keep = n_keep;
    uint64_t kept = 0, bad = 0;
    STCHK(dev_clade_filter(c, d_in, n, f, d_out, &kept, &bad));
    if (bad != ~0ull) return fail(MTB_ERR_ARG, "record " + std::to_string(bad) + " has species key " + std::to_string(rec[bad].qinfo >> 32) + ", keep[] holds " + std::to_string(n_keep) + " entries");
    if (kept) STCHK(d2h(c, out, d_out, kept * sizeof(mtb_kmer)));
    *n_out = kept;
    return MTB_OK;
}

mtb_status mtb_merge_sorted(mtb_ctx *c, const mtb_kmer *a, uint64_t n_a, const mtb_kmer *b, uint64_t n_b, mtb_kmer *out) {
    if (!c || (n_a && !a) || (n_b && !b) || ((n_a + n_b) && !out)) return fail(MTB_ERR_ARG, "NULL argument");
    if (n_a + n_b == 0) return MTB_OK;
    HIPCHK(hipSetDevice(c->device));
    mtb_kmer *d_in, *d_out;
    STCHK(ensure(c, "mrgA", n_a + n_b, &d_in)); STCHK(ensure(c, "mrgB", n_a + n_b, &d_out));
    if (n_a) STCHK(h2d(c, d_in, a, n_a * sizeof(mtb_kmer)));
    if (n_b) STCHK(h2d(c, d_in + n_a, b, n_b * sizeof(mtb_kmer)));
    STCHK(dev_merge2(c, d_in, n_a, d_in + n_a, n_b, d_out));
    STCHK(d2h(c, out, d_out, (n_a + n_b) * sizeof(mtb_kmer)));
    return MTB_OK;
}

/* mtb_merge_databases (flt == NULL) and mtb_merge_databases_filtered: one body */
static mtb_status merge_databases(mtb_ctx *c, const char *const *dbdirs, uint32_t n_dbs, const char *taxonomy_dir, const mtb_params *params,
                                  const char *outdir, int split_num, uint64_t max_range_records, const mtb_clade_filter *flt, mtb_merge_stats *stats,
                                  mtb_filter_stats *fstats) {
    if (!c || !taxonomy_dir || !params || !outdir || split_num < 2) return fail(MTB_ERR_ARG, "NULL argument / split_num < 2");
    if (flt && dbdirs) {
        /* a subset written over its own input would read what it has already overwritten: refused before anything in outdir is
         * touched, so the input stays the database it was */
        char ro[PATH_MAX], ri[PATH_MAX];
        if (realpath(outdir, ro))
            for (uint32_t i = 0; i < n_dbs; i++)
                if (dbdirs[i] && realpath(dbdirs[i], ri) && !strcmp(ro, ri)) return fail(MTB_ERR_ARG, std::string("the output directory is the input ") + dbdirs[i] + ": a filtered merge does not write over what it reads");
    }
    unlink((std::string(outdir) + "/db.parameters").c_str());          /* whatever happens below: no half-written database that opens */
    if (n_dbs == 0 || !dbdirs) return fail(MTB_ERR_ARG, "no databases to merge");
    mtb_filter_stats F; memset(&F, 0, sizeof(F));
    if (flt && flt->n_select + (uint64_t)flt->n_exclude == 0) return fail(MTB_ERR_ARG, "neither a selected nor an excluded taxon: nothing to filter (use mtb_merge_databases)");
    if (params->kmer_format != 1 && params->kmer_format != 2) return fail(MTB_ERR_UNSUPPORTED, "only kmer_format 1 and 2 are implemented");
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const auto t_all = std::chrono::steady_clock::now();
    mtb_merge_stats S; memset(&S, 0, sizeof(S));
    /* the inputs: parameters, checkpoints, sizes */
    std::vector<MergeSource> src(n_dbs);
    std::vector<mtbhost::MergeInput> inputs(n_dbs);
    for (uint32_t i = 0; i < n_dbs; i++) {
        if (!dbdirs[i]) return fail(MTB_ERR_ARG, "NULL database directory");
        MergeSource &s = src[i]; s.dir = dbdirs[i];
        /* what the database says of itself: the keys that db.parameters can only switch ON start switched off */
        mtb_params q = *params; q.syncmer = 0; int reduced_aa = 0;
        const bool have_par = mtbhost::file_exists(s.dir + "/db.parameters");
        if (have_par) q.skip_redundancy = 0;
        mtbhost::load_db_parameters(s.dir, &q, &reduced_aa);
        if (!have_par) q.syncmer = params->syncmer;
        if (reduced_aa) return fail(MTB_ERR_UNSUPPORTED, "database " + s.dir + " was built with the reduced amino-acid alphabet (Reduced_alphabet 1 in db.parameters); not implemented");
        if (q.kmer_format != params->kmer_format || (q.syncmer != 0) != (params->syncmer != 0) || (params->syncmer && q.smer_len != params->smer_len))
            return fail(MTB_ERR_ARG, "kmer_format / syncmer / smer_len of " + s.dir + " differ from the merge's parameters");
        s.info_mask = legacy_info_mask(q.skip_redundancy);
        struct stat sd, si;
        if (stat((s.dir + "/diffIdx").c_str(), &sd) != 0 || stat((s.dir + "/info").c_str(), &si) != 0) return fail(MTB_ERR_IO, "cannot open diffIdx / info in " + s.dir);
        std::vector<mtbhost::MergeCheckpoint> sp;
        if (mtbhost::file_exists(s.dir + "/split") && !mtbhost::read_whole(s.dir + "/split", &sp)) return fail(MTB_ERR_IO, "cannot read " + s.dir + "/split");
        mtbhost::merge_input_from_split(sp.data(), sp.size(), (uint64_t)si.st_size / 4, (uint64_t)sd.st_size / 2, &inputs[i]);
        S.n_input_entries += inputs[i].n_entries;
    }
    /* the taxonomy of the merge, on the device: a holder index without targets.  The species table covers every node: for an id that
     * occurs it holds what the table built from the ids that occur (mtb_builder_finish) holds. */
    mtb_index *hold = nullptr;
    {   std::string err;
        mtb_params q = *params; int reduced_aa = 0;
        mtbhost::load_db_parameters(std::string(taxonomy_dir) + "/..", &q, &reduced_aa);
        if (reduced_aa) return fail(MTB_ERR_UNSUPPORTED, "Reduced_alphabet 1 is not implemented");
        mtbhost::Taxonomy tax;
        if (!mtbhost::load_taxonomy(taxonomy_dir, &tax, &err)) return fail(MTB_ERR_IO, err);
        std::vector<int32_t> ids;
        for (int32_t t = 0; t <= tax.max_id; t++) if (tax.cn(t) >= 0) ids.push_back(t);
        q = *params; q.skip_redundancy = 1;
        STCHK(tax_holder_index(c, q, std::move(tax), ids, &hold)); }
    struct Guard { mtb_index *ix; ~Guard() { mtb_index_close(ix); } } guard{hold};
    const mtb_tax_view tv = tax_view(hold);
    const int bits = mtb_build_tax_bits(hold->tax.max_id);
    /* the filter: keep[] by species key from the host (host/clade_filter.h), uploaded once; met[] is cleared here and read at the end */
    struct FilterScratch { mtb_ctx *c; ~FilterScratch() { release(c, "cladekeep"); release(c, "clademet"); } } filter_scratch{c};
    mtbhost::CladeFilter cf;
    CladeDev fd;
    if (flt) {
        std::string err;
        if (!mtbhost::clade_filter_make(hold->tax, flt->select, flt->n_select, flt->exclude, flt->n_exclude, &cf, &err)) return fail(MTB_ERR_ARG, err);
        uint8_t *d_keep;
        fd.n_keep = cf.keep.size();
        STCHK(ensure(c, "cladekeep", cf.keep.size(), &d_keep)); STCHK(ensure(c, "clademet", cf.keep.size(), &fd.d_met));
        STCHK(h2d(c, d_keep, cf.keep.data(), cf.keep.size()));
        HIPCHK(hipMemsetAsync(fd.d_met, 0, cf.keep.size(), st));
        fd.d_keep = d_keep;
    }
    /* the ranges */
    uint64_t budget = max_range_records;
    if (budget == 0) {
        size_t fr = 0, tot = 0;
        HIPCHK(hipMemGetInfo(&fr, &tot));
        fr += held_bytes(c, BUF_WORK);
        const uint64_t fixed = 4ull << 30;                             /* decode chunks, the writer's slice buffers, scan workspace */
        budget = fr > 2 * fixed ? (fr - fixed) / MTB_MERGE_BYTES_PER_RECORD : std::max<uint64_t>(fr / (2 * MTB_MERGE_BYTES_PER_RECORD), 1);
    }
    budget = std::min<uint64_t>(budget, 0xFFFFFFFFull);
    std::vector<mtbhost::MergeRange> ranges;
    {   uint64_t needed = 0;
        if (mtbhost::merge_plan(inputs, budget, &ranges, &needed) != mtbhost::MERGE_PLAN_OK)
            return fail(MTB_ERR_CAPACITY, "one checkpoint interval of the inputs holds " + std::to_string(needed) + " records, more than max_range_records = " + std::to_string(budget) +
                                          ": the merge needs room for " + std::to_string(needed) + " records"); }
    uint64_t max_rec = 0;
    for (const mtbhost::MergeRange &r : ranges) max_rec = std::max(max_rec, r.records);
    S.n_ranges = ranges.size(); S.max_range_records_used = max_rec;
    IndexWriter w;
    STCHK(w.begin(c, outdir, hold->tax.max_id, hold->params, max_rec));
    struct Scratch { mtb_ctx *c; ~Scratch() { for (const char *nm : {"mrgA", "mrgB", "mrgsplit", "mrgov", "mrgoi", "bhead", "bpos", "blist", "kmersB", "hist"}) release(c, nm); } } scratch{c};
    DecodeScratch decode_scratch{c};
    unsigned long long *d_bad = scal<unsigned long long>(c, SC_JOIN_COUNT);
    uint32_t *d_unsorted = scal<uint32_t>(c, SC_JOIN_OVERFLOW);
    uint64_t *d_trim = scal<uint64_t>(c, SC_N_LARGE);                  /* two words: SC_N_LARGE, SC_MAX_SEG */
    for (const mtbhost::MergeRange &R : ranges) {
        if (R.records == 0) continue;
        mtb_kmer *d_a, *d_b;
        STCHK(ensure(c, "mrgA", R.records + 1, &d_a)); STCHK(ensure(c, "mrgB", R.records + 1, &d_b));
        if (flt) {
            /* tile counts and bases lie where the reduce keeps its head flags and positions, unused until then (asked for at the size
             * the reduce asks for at most, so that it does not allocate them again) */
            const uint64_t tiles = R.records / MTB_CLADE_TILE + 1;
            STCHK(ensure(c, "bhead", std::max<uint64_t>(R.records, tiles + 1), &fd.d_count));
            STCHK(ensure(c, "bpos", std::max<uint64_t>((R.records + 1) / 2 + 1, tiles + 2), &fd.d_base));
            STCHK(ensure(c, "scanws", scan_ws_elems(R.records + 1), &fd.d_ws));
        }
        std::vector<uint64_t> off(1, 0);
        auto t0 = std::chrono::steady_clock::now();
        for (uint32_t i = 0; i < n_dbs; i++) {
            const mtbhost::MergeSlice &sl = R.slices[i];
            const uint64_t T = sl.records();
            if (T == 0) continue;
            /* the slice is decoded into the buffer the merge has not written yet: T + 1 values, then T info entries */
            uint64_t *dv = (uint64_t *)d_b; uint32_t *di = (uint32_t *)(dv + T + 1);
            STCHK(decode_chunked(c, params->kmer_format, src[i].dir, sl, dv, di));
            hipLaunchKernelGGL(k_merge_trim, dim3(1), dim3(64), 0, st, (const uint64_t *)dv, T, R.lo, R.hi, d_trim);
            HIPCHK(hipGetLastError());
            uint64_t ab[2] = {0, 0};
            STCHK(d2h(c, ab, d_trim, 16));
            uint64_t cnt = ab[1] - ab[0];
            if (cnt == 0) continue;
            mtb_kmer *rec = d_a + off.back();
            HIPCHK(hipMemsetAsync(d_bad, 0xFF, 8, st)); HIPCHK(hipMemsetAsync(d_unsorted, 0, 8, st));
            hipLaunchKernelGGL(k_merge_keys, grid256(cnt), dim3(256), 0, st, (const uint64_t *)(dv + ab[0]), (const uint32_t *)(di + ab[0]), cnt, src[i].info_mask, tv,
                               (const int32_t *)hold->d_tax2species, rec, d_bad, d_unsorted);
            HIPCHK(hipGetLastError());
            uint64_t flags[2] = {0, 0};
            STCHK(d2h(c, flags, d_bad, 16));                            /* SC_JOIN_COUNT, SC_JOIN_OVERFLOW are adjacent */
            if (flags[0] != ~0ull) {
                mtb_kmer r;
                STCHK(d2h(c, &r, rec + flags[0], sizeof(r)));
                return fail(MTB_ERR_ARG, "taxid " + std::to_string(mtb_build_key_taxid(r.qinfo)) + " of " + src[i].dir + " (entry " + std::to_string(sl.info_lo + ab[0] + flags[0]) +
                                         ") is not in the merge's taxonomy");
            }
            if (flt) {
                /* the decoded slice in d_b is dead: the kept records are compacted into it and copied back */
                const auto tf = std::chrono::steady_clock::now();
                uint64_t kept = 0, bad = 0;
                STCHK(dev_clade_filter(c, rec, cnt, fd, d_b, &kept, &bad));
                if (bad != ~0ull) return fail(MTB_ERR_DEVICE, "a species key of " + src[i].dir + " lies outside the taxonomy (internal error)");
                if (kept && kept != cnt) { HIPCHK(hipMemcpyAsync(rec, d_b, kept * sizeof(mtb_kmer), hipMemcpyDeviceToDevice, st)); HIPCHK(hipStreamSynchronize(st)); }
                F.ms_filter += (float)ms_since(tf);
                F.n_records_in += cnt; F.n_records_kept += kept;
                cnt = kept;
                if (cnt == 0) continue;
            }
            if ((uint32_t)flags[1]) {
                /* built under another taxonomy: not ascending under this one -- the builder's two radix sorts, for this slice alone */
                mtb_kmer *d_s;
                hipLaunchKernelGGL(k_merge_sort_key, grid256(cnt), dim3(256), 0, st, rec, cnt, bits);
                STCHK(dev_sort_groups(c, rec, cnt, bits, &d_s));
                if (d_s != rec) HIPCHK(hipMemcpyAsync(rec, d_s, cnt * sizeof(mtb_kmer), hipMemcpyDeviceToDevice, st));
                HIPCHK(hipGetLastError());
                HIPCHK(hipStreamSynchronize(st));
                S.n_resorted_slices++;
            }
            off.push_back(off.back() + cnt);
        }
        S.ms_read_decode += (float)ms_since(t0);
        const uint64_t n = off.back();
        if (n == 0) continue;
        t0 = std::chrono::steady_clock::now();
        mtb_kmer *d_s;
        STCHK(dev_merge_tree(c, d_a, d_b, off, &d_s));
        HIPCHK(hipStreamSynchronize(st));
        S.ms_merge += (float)ms_since(t0);
        t0 = std::chrono::steady_clock::now();
        uint64_t *d_ov = nullptr; uint32_t *d_oi = nullptr;
        uint64_t G = 0; uint32_t n_long = 0;
        STCHK(dev_reduce_groups(c, d_s, n, tv, [&](uint64_t groups, uint64_t **d_values, uint32_t **d_info) -> mtb_status {
            STCHK(ensure(c, "mrgov", groups + 1, &d_ov)); STCHK(ensure(c, "mrgoi", groups + 1, &d_oi));
            *d_values = d_ov; *d_info = d_oi; return MTB_OK; }, &G, &n_long));
        HIPCHK(hipStreamSynchronize(st));
        S.ms_reduce += (float)ms_since(t0);
        t0 = std::chrono::steady_clock::now();
        STCHK(w.append(d_ov, d_oi, G));
        S.ms_encode_write += (float)ms_since(t0);
        S.n_entries += G;
    }
    if (flt) {
        /* before the writer finishes: a selection that keeps nothing leaves no database behind, not an empty one that opens */
        if (F.n_records_kept == 0) return fail(MTB_ERR_ARG, "the selection keeps none of the " + std::to_string(F.n_records_in) + " entries: nothing written");
        std::vector<uint8_t> met(cf.keep.size());
        STCHK(d2h(c, met.data(), fd.d_met, met.size()));
        const mtbhost::CladeFilterCounts k = mtbhost::clade_filter_counts(hold->tax, cf, met.data());
        F.n_species_kept = k.n_species_kept; F.n_species_dropped = k.n_species_dropped; F.n_unmatched = k.n_unmatched; F.first_unmatched = k.first_unmatched;
    }
    auto t0 = std::chrono::steady_clock::now();
    STCHK(w.finish(split_num));
    S.ms_split = (float)ms_since(t0);
    S.ms_total = (float)ms_since(t_all);
    if (stats) *stats = S;
    if (fstats) *fstats = F;
    return MTB_OK;
}

mtb_status mtb_merge_databases(mtb_ctx *c, const char *const *dbdirs, uint32_t n_dbs, const char *taxonomy_dir, const mtb_params *params,
                               const char *outdir, int split_num, uint64_t max_range_records, mtb_merge_stats *stats) {
    return merge_databases(c, dbdirs, n_dbs, taxonomy_dir, params, outdir, split_num, max_range_records, nullptr, stats, nullptr);
}

mtb_status mtb_merge_databases_filtered(mtb_ctx *c, const char *const *dbdirs, uint32_t n_dbs, const char *taxonomy_dir, const mtb_params *params,
                                        const char *outdir, int split_num, uint64_t max_range_records, const mtb_clade_filter *filter, mtb_merge_stats *stats,
                                        mtb_filter_stats *fstats) {
    if (!filter) { if (outdir) unlink((std::string(outdir) + "/db.parameters").c_str()); return fail(MTB_ERR_ARG, "NULL filter (use mtb_merge_databases)"); }
    return merge_databases(c, dbdirs, n_dbs, taxonomy_dir, params, outdir, split_num, max_range_records, filter, stats, fstats);
}

/* ---- audit of a database directory (mtb.h; kernels_audit.h, host/audit_plan.h) ---- */
mtb_status mtb_database_audit(mtb_ctx *c, const char *dbdir, const char *taxonomy_dir, mtb_params *params, uint64_t chunk_words, uint32_t *species_counts, uint64_t cap,
                              mtb_audit_report *out) {
    if (!c || !dbdir || !params || !out) return fail(MTB_ERR_ARG, "NULL argument");
    const auto t_all = std::chrono::steady_clock::now();
    const std::string d(dbdir);
    /* the files first: nothing below touches the device before they are sound */
    mtbhost::AuditFiles files;
    {   std::string err;
        if (!mtbhost::audit_check_files(d, taxonomy_dir, &files, &err)) return fail(MTB_ERR_IO, d + ": " + err + (files.note.empty() ? "" : " " + files.note)); }
    auto failed = [&](mtb_status s) { if (!files.note.empty()) g_err += " (" + files.note + ")"; return s; };
    int reduced_aa = 0;
    mtbhost::load_db_parameters(d, params, &reduced_aa);
    if (reduced_aa) return failed(fail(MTB_ERR_UNSUPPORTED, "database was built with the reduced amino-acid alphabet (Reduced_alphabet 1 in db.parameters); not implemented"));
    if (params->kmer_format != 1 && params->kmer_format != 2) return failed(fail(MTB_ERR_UNSUPPORTED, "database uses a k-mer format other than 1 or 2"));
    mtb_audit_report R; memset(&R, 0, sizeof(R));
    R.n_words = files.n_words; R.n_info_entries = files.n_info_entries;
    R.first_value_descent = R.first_group_disorder = R.first_unknown_id = R.first_unlisted_id = R.first_bad_checkpoint = UINT64_MAX;
    if (!mtbhost::audit_trailing_words(d + "/diffIdx", R.n_words, &R.n_trailing_words)) return failed(fail(MTB_ERR_IO, "cannot read " + d + "/diffIdx"));
    std::vector<mtbhost::MergeCheckpoint> split;
    if (!mtbhost::read_whole(d + "/split", &split)) return failed(fail(MTB_ERR_IO, "cannot read " + d + "/split"));
    const std::vector<mtbhost::AuditCheckpoint> cps = mtbhost::audit_usable_checkpoints(split, R.n_info_entries, R.n_words);
    R.n_checkpoints = cps.size();
    /* the taxonomy and species table of mtb_index_open, on the device: a holder index without targets */
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    mtbhost::Taxonomy tax;
    std::vector<int32_t> ids;
    {   const std::string taxdir = taxonomy_dir && *taxonomy_dir ? std::string(taxonomy_dir) : d + "/taxonomy";
        const mtb_status s = load_database_taxonomy(d, taxdir, mtbhost::file_exists(d + "/taxonomyDB"), &tax, &ids);
        if (s != MTB_OK) return failed(s); }
    const uint64_t n_bins = (uint64_t)tax.max_id + 1;
    if (species_counts && cap < n_bins) {
        out->n_species = n_bins;
        return failed(fail(MTB_ERR_CAPACITY, "species_counts holds " + std::to_string(cap) + " entries, the taxonomy needs " + std::to_string(n_bins)));
    }
    mtb_index *hold = nullptr;
    STCHK(tax_holder_index(c, *params, std::move(tax), ids, &hold));
    struct Guard { mtb_index *ix; ~Guard() { mtb_index_close(ix); } } guard{hold};
    const mtb_tax_view tv = tax_view(hold);
    /* chunk size: the caller's, else the decode's rule (128 M words, less under a workspace limit) within a 32nd of free HBM (a
     * chunk holds ~16 bytes per word on the device) */
    uint64_t CH = chunk_words;
    if (CH == 0) {
        CH = decode_chunk_words(c);
        size_t fr = 0, tot = 0;
        HIPCHK(hipMemGetInfo(&fr, &tot));
        CH = std::max<uint64_t>(1u << 16, std::min<uint64_t>(CH, (fr + held_bytes(c, BUF_WORK)) / 32));
    }
    CH = std::max<uint64_t>(16, std::min<uint64_t>(CH, std::max<uint64_t>(R.n_words, 16)));
    struct Scratch { mtb_ctx *c; ~Scratch() { for (const char *nm : {"auditv", "auditi", "auditbins", "auditlisted", "auditout", "auditcp"}) release(c, nm); } } scratch{c};
    DecodeScratch decode_scratch{c};
    uint64_t *d_v; uint32_t *d_i, *d_bins; uint8_t *d_listed; unsigned long long *d_out; mtb_audit_checkpoint *d_cp;
    const uint32_t CP_MAX = 4096;                                  /* checkpoints judged per launch */
    STCHK(ensure(c, "auditv", CH + 16, &d_v)); STCHK(ensure(c, "auditi", CH + 16, &d_i));
    /* how the counts are taken: in the check kernel, a hot species folded in the wave, one bin array per XCD summed at the end -- or,
     * for measurements (mtb_debug_audit_mode): 1 not at all, 2 one add per entry, 3 / 4 as 0 / 2 into a single bin array */
    const int mode = c->audit_mode;
    const bool replicated = mode == 0 || mode == 2;
    const int fold_rounds = mode == 2 || mode == 4 ? 0 : MTB_AUDIT_FOLD_ROUNDS;
    const uint64_t bin_stride = replicated ? ((n_bins + 63) & ~63ull) : 0, bin_words = replicated ? bin_stride * MTB_AUDIT_REPLICAS : n_bins;
    STCHK(ensure(c, "auditbins", bin_words, &d_bins)); STCHK(ensure(c, "auditlisted", n_bins + 1, &d_listed));
    STCHK(ensure(c, "auditout", (size_t)MTB_AUDIT_WORDS + 4, &d_out)); STCHK(ensure(c, "auditcp", (size_t)CP_MAX, &d_cp));
    uint64_t *d_prev = (uint64_t *)(d_out + MTB_AUDIT_WORDS);      /* two {value, species} pairs, used in turn */
    {   /* counters 0, first positions ~0; the listed ids as the byte map of k_mark_taxids */
        unsigned long long init[MTB_AUDIT_WORDS + 4];
        for (int k = 0; k < MTB_AUDIT_WORDS + 4; k++) init[k] = 0;
        for (int k = 0; k < MTB_AUDIT_COUNTERS; k++) init[MTB_AUDIT_FIRST + k] = ~0ull;
        init[MTB_AUDIT_FIRST_BAD_CP] = ~0ull;
        STCHK(h2d(c, d_out, init, sizeof(init)));
        std::vector<uint8_t> listed(n_bins + 1, 0);
        for (int32_t t : ids) if (t >= 0 && (uint64_t)t < n_bins) listed[(size_t)t] = 1;
        STCHK(h2d(c, d_listed, listed.data(), listed.size())); }
    float ms_hist = 0;
    {   const auto t0 = std::chrono::steady_clock::now();
        HIPCHK(hipMemsetAsync(d_bins, 0, bin_words * 4, st)); HIPCHK(hipStreamSynchronize(st));
        ms_hist += (float)ms_since(t0); }
    ChunkSink sink;
    struct Events { hipEvent_t *e; ~Events() { for (int k = 0; k < 3; k++) if (e[k]) { hipError_t x = hipEventDestroy(e[k]); (void)x; } } } events{sink.ev};
    for (int k = 0; k < 3; k++) HIPCHK(hipEventCreate(&sink.ev[k]));
    sink.chunk_words = CH;
    size_t next_cp = 0; uint64_t missed_cp = 0, first_missed_cp = UINT64_MAX; int turn = 0;
    std::vector<mtbhost::AuditCheckpoint> take; std::vector<mtb_audit_checkpoint> rel;
    sink.on_chunk = [&](const DecodedChunk &k) -> mtb_status {
        if (k.n_info) {
            const uint64_t blocks = (k.n_info + 256ull * MTB_AUDIT_PER_LANE - 1) / (256ull * MTB_AUDIT_PER_LANE);
            hipLaunchKernelGGL(k_audit_order, dim3((uint32_t)std::min<uint64_t>(blocks, 1u << 16)), dim3(256), 0, st, k.d_values, k.d_info, k.n_info, k.first_entry, hold->info_mask, tv,
                               (const int32_t *)hold->d_tax2species, (const uint8_t *)d_listed, (const uint64_t *)(d_prev + 2 * turn), d_prev + 2 * (turn ^ 1), d_out, mode == 1 ? (uint32_t *)nullptr : d_bins, fold_rounds, bin_stride);
            turn ^= 1;
        }
        mtbhost::audit_chunk_checkpoints(cps, &next_cp, k.word0, k.n_words, &take, &missed_cp, &first_missed_cp);
        for (size_t at = 0; at < take.size(); at += CP_MAX) {
            const uint32_t n = (uint32_t)std::min<size_t>(CP_MAX, take.size() - at);
            rel.resize(n);
            for (uint32_t q = 0; q < n; q++) {
                const mtbhost::AuditCheckpoint &a = take[at + q];
                rel[q].ad = a.cp.ad; rel[q].diff_off = a.cp.diff_off - k.word0; rel[q].info_off = a.cp.info_off - k.first_entry; rel[q].record = a.record;       /* (an info_off before the chunk wraps: never equal to a count) */
            }
            STCHK(h2d(c, d_cp, rel.data(), (size_t)n * sizeof(mtb_audit_checkpoint)));
            hipLaunchKernelGGL(k_audit_checkpoints, dim3((n + 63) / 64), dim3(64), 0, st, k.d_words, k.n_words, k.d_tile_off, k.d_values, k.n_values, (const mtb_audit_checkpoint *)d_cp, n, d_out);
        }
        HIPCHK(hipGetLastError());
        return MTB_OK;
    };
    {   mtbhost::MergeSlice whole;           /* every word before the trailing ones; how many entries they code is what the audit finds out */
        whole.diff_hi = R.n_words - R.n_trailing_words; whole.info_hi = R.n_info_entries;
        const mtb_status s = decode_chunked(c, params->kmer_format, d, whole, d_v, d_i, nullptr, &sink);
        if (s != MTB_OK) return failed(s); }
    /* checkpoints behind the last decoded word (among the trailing words) were never offered to a chunk */
    for (; next_cp < cps.size(); next_cp++) { missed_cp++; first_missed_cp = std::min(first_missed_cp, cps[next_cp].record); }
    unsigned long long h[MTB_AUDIT_WORDS];
    STCHK(d2h(c, h, d_out, sizeof(h)));
    R.n_end_words = sink.n_entries; R.n_entries = std::min(R.n_end_words, R.n_info_entries); R.n_chunks = sink.n_chunks;
    R.n_value_descents = h[MTB_AUDIT_DESCENT]; R.first_value_descent = h[MTB_AUDIT_FIRST + MTB_AUDIT_DESCENT];
    R.n_group_disorder = h[MTB_AUDIT_DISORDER]; R.first_group_disorder = h[MTB_AUDIT_FIRST + MTB_AUDIT_DISORDER];
    R.n_unknown_ids = h[MTB_AUDIT_UNKNOWN]; R.first_unknown_id = h[MTB_AUDIT_FIRST + MTB_AUDIT_UNKNOWN];
    R.n_unlisted_ids = h[MTB_AUDIT_UNLISTED]; R.first_unlisted_id = h[MTB_AUDIT_FIRST + MTB_AUDIT_UNLISTED];
    R.n_no_species = h[MTB_AUDIT_NO_SPECIES];
    R.n_bad_checkpoints = h[MTB_AUDIT_BAD_CP] + missed_cp; R.first_bad_checkpoint = std::min<uint64_t>(h[MTB_AUDIT_FIRST_BAD_CP], first_missed_cp);
    {   const auto t0 = std::chrono::steady_clock::now();
        std::vector<uint32_t> own;
        uint32_t *bins = species_counts;
        if (!bins) { own.resize(n_bins); bins = own.data(); }
        if (replicated) { hipLaunchKernelGGL(k_audit_bins_reduce, grid256(n_bins), dim3(256), 0, st, d_bins, n_bins, bin_stride); HIPCHK(hipGetLastError()); }
        STCHK(d2h(c, bins, d_bins, n_bins * 4));
        for (uint64_t s = 0; s < n_bins; s++) if (bins[s]) R.n_species++;
        ms_hist += (float)ms_since(t0); }
    R.valid = R.n_end_words == R.n_info_entries && !R.n_trailing_words && !R.n_value_descents && !R.n_unknown_ids && !R.n_bad_checkpoints;
    R.canonical = R.valid && !R.n_group_disorder && !R.n_unlisted_ids;
    R.ms_read = (float)sink.us_read.load() / 1000.0f; R.ms_decode = sink.ms_decode; R.ms_check = sink.ms_sink; R.ms_hist = ms_hist;
    R.ms_total = (float)ms_since(t_all);
    *out = R;
    return MTB_OK;
}

/* measurements only (profiles/scripts/audit_measure.py; not declared in mtb.h): see mtb_database_audit */
mtb_status mtb_debug_audit_mode(mtb_ctx *c, int mode) {
    if (!c || mode < 0 || mode > 4) return fail(MTB_ERR_ARG, "audit mode 0..4");
    c->audit_mode = mode;
    return MTB_OK;
}

mtb_status mtb_audit_write_species_counts(const char *dbdir, const uint32_t *species_counts, uint64_t n) {
    if (!dbdir || (!species_counts && n)) return fail(MTB_ERR_ARG, "NULL argument");
    const std::string path = std::string(dbdir) + "/sp2uniqKmerCnt";
    FILE *f = fopen(path.c_str(), "w");
    if (!f) return fail(MTB_ERR_IO, "cannot create " + path);
    for (uint64_t s = 0; s < n; s++) if (species_counts[s]) fprintf(f, "%llu %u\n", (unsigned long long)s, species_counts[s]);
    if (fclose(f) != 0) return fail(MTB_ERR_IO, "short write to " + path);
    return MTB_OK;
}

} // extern "C"

/* ---- inspection of a database: LCA k-mer counts per taxon (mtb.h; kernels_inspect.h; the rule: tests/inspect_spec.py) ---- */
/* The device passes of one inspection, whoever brings the chunks (decode_chunked's sink, or the stage call's uploads): begin, pass per
 * chunk in file order, finish.  u32 bins of one pass (distinct, then entries; one array per XCD each), their u64 sums, the counters,
 * two records per tile, two carry slots used in turn. */
struct InspectRun {
    mtb_ctx *c = nullptr;
    mtb_tax_view tv; uint32_t info_mask = 0; int level = 0;
    uint64_t n_bins = 0, stride = 0, n_entries = 0, n_passes = 0;
    uint32_t *d_pass = nullptr; unsigned long long *d_sum = nullptr, *d_out = nullptr;
    mtb_inspect_rec *d_rec = nullptr, *d_carry = nullptr;
    int turn = 0; bool any = false;
    float ms_bins = 0;
    ~InspectRun() { if (c) for (const char *nm : {"inspbins", "inspsum", "inspout", "insprec", "inspcarry"}) release(c, nm); }
    uint64_t pass_words() const { return 2 * stride * MTB_AUDIT_REPLICAS; }
    mtb_status begin(mtb_ctx *c_, const mtb_tax_view &tv_, uint32_t mask, int level_, uint64_t max_pass_entries) {
        c = c_; tv = tv_; info_mask = mask; level = level_;
        n_bins = (uint64_t)tv.max_taxid + 1; stride = (n_bins + 63) & ~63ull;
        const auto t0 = std::chrono::steady_clock::now();
        STCHK(ensure(c, "inspbins", pass_words(), &d_pass)); STCHK(ensure(c, "inspsum", 2 * n_bins, &d_sum));
        STCHK(ensure(c, "inspout", (size_t)MTB_INSPECT_WORDS, &d_out)); STCHK(ensure(c, "inspcarry", (size_t)2, &d_carry));
        STCHK(ensure(c, "insprec", 2 * ((max_pass_entries + MTB_INSPECT_TILE - 1) / MTB_INSPECT_TILE) + 2, &d_rec));
        hipStream_t st = c->stream;
        HIPCHK(hipMemsetAsync(d_pass, 0, pass_words() * 4, st)); HIPCHK(hipMemsetAsync(d_sum, 0, 2 * n_bins * 8, st));
        HIPCHK(hipMemsetAsync(d_carry, 0, 2 * sizeof(mtb_inspect_rec), st));
        unsigned long long init[MTB_INSPECT_WORDS];
        for (int k = 0; k < MTB_INSPECT_WORDS; k++) init[k] = 0;
        init[MTB_INSPECT_WALK_FIRST] = ~0ull;
        STCHK(h2d(c, d_out, init, sizeof(init)));
        HIPCHK(hipStreamSynchronize(st));
        ms_bins += (float)ms_since(t0);
        return MTB_OK;
    }
    /* entries [g0, g0 + m) of the database as a chunk on the device (256-byte aligned); asynchronous on the context's stream */
    mtb_status pass(const uint64_t *d_values, const uint32_t *d_info, uint64_t m, uint64_t g0) {
        if (m == 0) return MTB_OK;
        if (m >> 32) return fail(MTB_ERR_ARG, "a pass of the inspection holds fewer than 2^32 entries");
        hipStream_t st = c->stream;
        const uint64_t tiles = (m + MTB_INSPECT_TILE - 1) / MTB_INSPECT_TILE;
        STCHK(ensure(c, "insprec", 2 * tiles + 2, &d_rec));
        uint32_t *d_distinct = d_pass, *d_entries = d_pass + stride * MTB_AUDIT_REPLICAS;
        hipLaunchKernelGGL(k_inspect_tiles, dim3((uint32_t)std::min<uint64_t>(tiles, 4096)), dim3(256), 0, st, d_values, d_info, m, g0, info_mask, level, tv, d_rec, d_distinct, d_entries,
                           stride, (int)MTB_INSPECT_FOLD_ROUNDS, d_out);
        hipLaunchKernelGGL(k_inspect_walk, dim3(1), dim3(64), 0, st, (const mtb_inspect_rec *)d_rec, 2 * tiles, (const mtb_inspect_rec *)(d_carry + turn), any ? 1 : 0, d_carry + (turn ^ 1), 0, tv,
                           d_sum, d_sum + n_bins, (int)MTB_INSPECT_FOLD_ROUNDS, d_out);
        turn ^= 1; any = true;
        for (int k = 0; k < 2; k++) {
            uint32_t *bins = k ? d_entries : d_distinct;
            hipLaunchKernelGGL(k_audit_bins_reduce, grid256(n_bins), dim3(256), 0, st, bins, n_bins, stride);
            hipLaunchKernelGGL(k_cov_accumulate, grid256(n_bins), dim3(256), 0, st, d_sum + (uint64_t)k * n_bins, bins, n_bins);
        }
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemsetAsync(d_pass + stride, 0, (pass_words() - stride) * 4, st));       /* (k_cov_accumulate cleared the first array; this clears the other replicas and the second set) */
        n_entries += m; n_passes++;
        return MTB_OK;
    }
    /* closes the last group; the report's counts (not its times), the u64 bins */
    mtb_status finish(uint64_t *distinct, uint64_t *entries, mtb_inspect_report *R) {
        hipStream_t st = c->stream;
        hipLaunchKernelGGL(k_inspect_walk, dim3(1), dim3(64), 0, st, (const mtb_inspect_rec *)d_rec, (uint64_t)0, (const mtb_inspect_rec *)(d_carry + turn), any ? 1 : 0, d_carry + (turn ^ 1), 1, tv,
                           d_sum, d_sum + n_bins, (int)MTB_INSPECT_FOLD_ROUNDS, d_out);
        HIPCHK(hipGetLastError());
        const auto t0 = std::chrono::steady_clock::now();
        unsigned long long h[MTB_INSPECT_WORDS];
        STCHK(d2h(c, h, d_out, sizeof(h)));
        if (distinct) STCHK(d2h(c, distinct, d_sum, n_bins * 8));
        if (entries) STCHK(d2h(c, entries, d_sum + n_bins, n_bins * 8));
        ms_bins += (float)ms_since(t0);
        R->n_entries = n_entries; R->n_chunks = n_passes; R->n_taxa = n_bins;
        R->n_orphan_groups = h[MTB_INSPECT_ORPHAN_GROUPS]; R->n_orphan_entries = h[MTB_INSPECT_ORPHAN_ENTRIES];
        R->n_groups = 0;
        for (int k = 0; k < MTB_INSPECT_HIST; k++) { R->size_hist[k] = h[MTB_INSPECT_HIST0 + k]; R->n_groups += h[MTB_INSPECT_HIST0 + k]; }
        /* the largest group: among those closed inside a tile and those the walk closed; of equals the first */
        uint64_t mx = h[MTB_INSPECT_WALK_MAX], first = h[MTB_INSPECT_WALK_FIRST];
        if (h[MTB_INSPECT_TILE_MAX]) {
            const uint64_t ts = h[MTB_INSPECT_TILE_MAX] >> 48, tf = MTB_INSPECT_FIRST_MASK - (h[MTB_INSPECT_TILE_MAX] & MTB_INSPECT_FIRST_MASK);
            if (ts > mx || (ts == mx && tf < first)) { mx = ts; first = tf; }
        }
        R->max_group = mx; R->first_max_group = mx ? first : UINT64_MAX;
        return MTB_OK;
    }
};

/* the taxonomy a report is written against: an index's, a database directory's (mtb_database_inspect's rule), or dump files */
static mtb_status inspect_taxonomy(const mtb_index *ix, const char *dbdir, const char *taxonomy_dir, mtbhost::Taxonomy *own, const mtbhost::Taxonomy **use) {
    if (ix) { *use = &ix->tax; return MTB_OK; }
    *use = own;
    if (dbdir && *dbdir) {
        const std::string d(dbdir);
        std::vector<int32_t> ids;
        return load_database_taxonomy(d, taxonomy_dir && *taxonomy_dir ? std::string(taxonomy_dir) : d + "/taxonomy", mtbhost::file_exists(d + "/taxonomyDB"), own, &ids);
    }
    if (!taxonomy_dir || !*taxonomy_dir) return fail(MTB_ERR_ARG, "no taxonomy: an index, a database directory or a taxonomy directory is needed");
    std::string err;
    if (!mtbhost::load_taxonomy(taxonomy_dir, own, &err)) return fail(MTB_ERR_IO, err);
    return MTB_OK;
}

extern "C" {

uint32_t mtb_inspect_tile_entries(void) { return MTB_INSPECT_TILE; }

mtb_status mtb_database_inspect(mtb_ctx *c, const char *dbdir, const char *taxonomy_dir, mtb_params *params, uint64_t chunk_words, int level, uint64_t *distinct, uint64_t *entries,
                                uint64_t cap, mtb_inspect_report *out) {
    if (!c || !dbdir || !params || !out) return fail(MTB_ERR_ARG, "NULL argument");
    if (level != 0 && level != 1) return fail(MTB_ERR_ARG, "inspection level " + std::to_string(level) + ": 0 (dna) or 1 (aa)");
    const auto t_all = std::chrono::steady_clock::now();
    const std::string d(dbdir);
    /* the files first, as the audit does: nothing below touches the device before they are sound */
    mtbhost::AuditFiles files;
    {   std::string err;
        if (!mtbhost::audit_check_files(d, taxonomy_dir, &files, &err)) return fail(MTB_ERR_IO, d + ": " + err + (files.note.empty() ? "" : " " + files.note)); }
    auto failed = [&](mtb_status s) { if (!files.note.empty()) g_err += " (" + files.note + ")"; return s; };
    int reduced_aa = 0;
    mtbhost::load_db_parameters(d, params, &reduced_aa);
    if (reduced_aa) return failed(fail(MTB_ERR_UNSUPPORTED, "database was built with the reduced amino-acid alphabet (Reduced_alphabet 1 in db.parameters); not implemented"));
    if (params->kmer_format != 1 && params->kmer_format != 2) return failed(fail(MTB_ERR_UNSUPPORTED, "database uses a k-mer format other than 1 or 2"));
    uint64_t trailing = 0;
    if (!mtbhost::audit_trailing_words(d + "/diffIdx", files.n_words, &trailing)) return failed(fail(MTB_ERR_IO, "cannot read " + d + "/diffIdx"));
    HIPCHK(hipSetDevice(c->device));
    mtbhost::Taxonomy tax;
    std::vector<int32_t> ids;
    {   const std::string taxdir = taxonomy_dir && *taxonomy_dir ? std::string(taxonomy_dir) : d + "/taxonomy";
        const mtb_status s = load_database_taxonomy(d, taxdir, mtbhost::file_exists(d + "/taxonomyDB"), &tax, &ids);
        if (s != MTB_OK) return failed(s); }
    const uint64_t n_bins = (uint64_t)tax.max_id + 1;
    if ((distinct || entries) && cap < n_bins) {
        out->n_taxa = n_bins;
        return failed(fail(MTB_ERR_CAPACITY, "the arrays hold " + std::to_string(cap) + " entries, the taxonomy needs " + std::to_string(n_bins)));
    }
    mtb_index *hold = nullptr;
    STCHK(tax_holder_index(c, *params, std::move(tax), ids, &hold));
    struct Guard { mtb_index *ix; ~Guard() { mtb_index_close(ix); } } guard{hold};
    /* chunk size: the audit's rule */
    uint64_t CH = chunk_words;
    if (CH == 0) {
        CH = decode_chunk_words(c);
        size_t fr = 0, tot = 0;
        HIPCHK(hipMemGetInfo(&fr, &tot));
        CH = std::max<uint64_t>(1u << 16, std::min<uint64_t>(CH, (fr + held_bytes(c, BUF_WORK)) / 32));
    }
    CH = std::max<uint64_t>(16, std::min<uint64_t>(CH, std::max<uint64_t>(files.n_words, 16)));
    struct Scratch { mtb_ctx *c; ~Scratch() { for (const char *nm : {"inspv", "inspi"}) release(c, nm); } } scratch{c};
    DecodeScratch decode_scratch{c};
    uint64_t *d_v; uint32_t *d_i;
    STCHK(ensure(c, "inspv", CH + 16, &d_v)); STCHK(ensure(c, "inspi", CH + 16, &d_i));
    InspectRun run;
    STCHK(run.begin(c, tax_view(hold), hold->info_mask, level, CH + 16));
    ChunkSink sink;
    struct Events { hipEvent_t *e; ~Events() { for (int k = 0; k < 3; k++) if (e[k]) { hipError_t x = hipEventDestroy(e[k]); (void)x; } } } events{sink.ev};
    for (int k = 0; k < 3; k++) HIPCHK(hipEventCreate(&sink.ev[k]));
    sink.chunk_words = CH;
    sink.on_chunk = [&](const DecodedChunk &k) -> mtb_status { return run.pass(k.d_values, k.d_info, k.n_info, k.first_entry); };
    {   mtbhost::MergeSlice whole;           /* every word before the trailing ones, as the audit reads them */
        whole.diff_hi = files.n_words - trailing; whole.info_hi = files.n_info_entries;
        const mtb_status s = decode_chunked(c, params->kmer_format, d, whole, d_v, d_i, nullptr, &sink);
        if (s != MTB_OK) return failed(s); }
    mtb_inspect_report R; memset(&R, 0, sizeof(R));
    {   const mtb_status s = run.finish(distinct, entries, &R);
        if (s != MTB_OK) return failed(s); }
    R.n_chunks = sink.n_chunks;
    R.ms_read = (float)sink.us_read.load() / 1000.0f; R.ms_decode = sink.ms_decode; R.ms_inspect = sink.ms_sink; R.ms_bins = run.ms_bins;
    R.ms_total = (float)ms_since(t_all);
    *out = R;
    return MTB_OK;
}

mtb_status mtb_inspect_records(mtb_ctx *c, const mtb_index *ix, const char *taxonomy_dir, const uint64_t *values, const uint32_t *info, uint64_t n, uint32_t info_mask, int level,
                               uint64_t entries_per_pass, uint64_t *distinct, uint64_t *entries, uint64_t cap, mtb_inspect_report *out) {
    if (!c || !out || (n && (!values || !info))) return fail(MTB_ERR_ARG, "NULL argument");
    if (level != 0 && level != 1) return fail(MTB_ERR_ARG, "inspection level " + std::to_string(level) + ": 0 (dna) or 1 (aa)");
    if (ix && ix->ctx->device != c->device) return fail(MTB_ERR_ARG, "the index lives on another device");
    const auto t_all = std::chrono::steady_clock::now();
    HIPCHK(hipSetDevice(c->device));
    mtb_index *hold = nullptr;
    struct Guard { mtb_index *&ix; ~Guard() { if (ix) mtb_index_close(ix); } } guard{hold};
    if (!ix) {
        if (!taxonomy_dir || !*taxonomy_dir) return fail(MTB_ERR_ARG, "no taxonomy: an index or a taxonomy directory is needed");
        mtbhost::Taxonomy tax; std::string err;
        if (!mtbhost::load_taxonomy(taxonomy_dir, &tax, &err)) return fail(MTB_ERR_IO, err);
        mtb_params p; mtb_default_params(&p);
        STCHK(tax_holder_index(c, p, std::move(tax), std::vector<int32_t>(), &hold));
    }
    const mtb_index *t = ix ? ix : hold;
    const uint64_t n_bins = (uint64_t)t->tax.max_id + 1;
    if ((distinct || entries) && cap < n_bins) {
        out->n_taxa = n_bins;
        return fail(MTB_ERR_CAPACITY, "the arrays hold " + std::to_string(cap) + " entries, the taxonomy needs " + std::to_string(n_bins));
    }
    uint64_t P = entries_per_pass ? (entries_per_pass + 3) & ~3ull : std::max<uint64_t>(n, 4);
    if (P >> 32) P = 1ull << 31;
    struct Scratch { mtb_ctx *c; ~Scratch() { for (const char *nm : {"inspv", "inspi"}) release(c, nm); } } scratch{c};
    uint64_t *d_v; uint32_t *d_i;
    STCHK(ensure(c, "inspv", P + 16, &d_v)); STCHK(ensure(c, "inspi", P + 16, &d_i));
    InspectRun run;
    STCHK(run.begin(c, tax_view(t), info_mask, level, P));
    const auto t0 = std::chrono::steady_clock::now();
    for (uint64_t g0 = 0; g0 < n; g0 += P) {
        const uint64_t m = std::min<uint64_t>(P, n - g0);
        STCHK(h2d(c, d_v, values + g0, m * 8)); STCHK(h2d(c, d_i, info + g0, m * 4));
        STCHK(run.pass(d_v, d_i, m, g0));
        HIPCHK(hipStreamSynchronize(c->stream));          /* the chunk buffers are refilled next */
    }
    mtb_inspect_report R; memset(&R, 0, sizeof(R));
    STCHK(run.finish(distinct, entries, &R));
    R.ms_inspect = (float)ms_since(t0); R.ms_bins = run.ms_bins; R.ms_total = (float)ms_since(t_all);
    *out = R;
    return MTB_OK;
}

mtb_status mtb_inspect_write_report(const mtb_index *ix, const char *dbdir, const char *taxonomy_dir, const uint64_t *distinct, const uint64_t *entries, uint64_t n, uint64_t n_groups,
                                    const char *tsv_path, char *summary, uint64_t summary_cap) {
    if (!distinct || !entries) return fail(MTB_ERR_ARG, "NULL argument");
    mtbhost::Taxonomy own; const mtbhost::Taxonomy *tax = nullptr;
    STCHK(inspect_taxonomy(ix, dbdir, taxonomy_dir, &own, &tax));
    const uint64_t n_bins = (uint64_t)tax->max_id + 1;
    if (n < n_bins) return fail(MTB_ERR_CAPACITY, "the arrays hold " + std::to_string(n) + " entries, the taxonomy needs " + std::to_string(n_bins));
    auto node = [&](uint64_t t) { return tax->canon[t] == (int32_t)t; };
    if (tsv_path) {
        /* clade sums: children before parents, by descending depth */
        std::vector<uint64_t> dc(distinct, distinct + n_bins), ec(entries, entries + n_bins);
        std::vector<int32_t> order;
        for (uint64_t t = 0; t < n_bins; t++) if (node(t)) order.push_back((int32_t)t);
        std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return tax->depth[(size_t)a] > tax->depth[(size_t)b]; });
        for (int32_t t : order) {
            const int32_t p = tax->parent[(size_t)t];
            if (p != t && p >= 0) { dc[(size_t)p] += dc[(size_t)t]; ec[(size_t)p] += ec[(size_t)t]; }
        }
        FILE *f = fopen(tsv_path, "w");
        if (!f) return fail(MTB_ERR_IO, std::string("cannot create ") + tsv_path);
        fprintf(f, "original_taxid\trank\tname\tdistinct\tentries\tdistinct_clade\tentries_clade\n");
        for (uint64_t t = 0; t < n_bins; t++) {
            if (!node(t) || (!dc[t] && !ec[t])) continue;
            fprintf(f, "%d\t%s\t%s\t%llu\t%llu\t%llu\t%llu\n", tax->orig.empty() ? (int)t : (int)tax->orig[t], tax->rank[t].c_str(), tax->name[t].c_str(), (unsigned long long)distinct[t],
                    (unsigned long long)entries[t], (unsigned long long)dc[t], (unsigned long long)ec[t]);
        }
        if (fclose(f) != 0) return fail(MTB_ERR_IO, std::string("short write to ") + tsv_path);
    }
    if (summary) {
        static const char *const order[] = {"root", "superkingdom", "phylum", "class", "order", "family", "genus", "species", "subspecies", "no rank"};      /* count_common_kmers.cpp:107-109 */
        auto by_rank = [&](const uint64_t *arr) {
            std::map<std::string, uint64_t> sum;
            for (uint64_t t = 0; t < n_bins; t++) if (node(t) && arr[t]) sum[t == 1 ? std::string("root") : tax->rank[t]] += arr[t];
            std::string s;
            for (const char *r : order) { auto it = sum.find(r); if (it != sum.end()) { s += it->first + ": " + std::to_string(it->second) + "\n"; sum.erase(it); } }
            for (const auto &kv : sum) s += kv.first + ": " + std::to_string(kv.second) + "\n";      /* (the reference drops these; a map walks them alphabetically) */
            return s;
        };
        const std::string s = "Common k-mers count by rank:\n" + by_rank(entries) + "Total distinct common k-mers count: " + std::to_string(n_groups) + "\n" +
                              "Distinct common k-mers count by rank:\n" + by_rank(distinct);
        if (s.size() + 1 > summary_cap) return fail(MTB_ERR_CAPACITY, "the summary needs " + std::to_string(s.size() + 1) + " bytes");
        memcpy(summary, s.c_str(), s.size() + 1);
    }
    return MTB_OK;
}

} // extern "C"
