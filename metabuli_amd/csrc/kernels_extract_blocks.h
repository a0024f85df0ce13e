/* kernels_extract_blocks.h -- single-frame scan of sequence blocks (gfx950, wave64): what IndexCreator feeds its scanners when a
 * database is built from gene predictions or from a CDS annotation (KmerExtractor::extractTargetKmers, KmerExtractor.cpp:407-426;
 * the blocks: IndexCreator.cpp:1094-1127, SeqIterator.cpp:180-244).  A block {seq, strand, start, end} is scanned in one frame on
 * one strand (mtb_core.h, "Block scan").
 *
 * Decomposition: every window is independent of every other, so the unit of work is a PIECE -- up to MTB_BLOCK_PIECE_WINDOWS
 * consecutive windows of one block -- and not a block or a sequence (a genome-long non-coding block and a 30-base exon sit in one
 * list).  k_block_pieces counts the pieces of every block, a prefix sum gives the piece table, and one wavefront per piece finds
 * its block by bisection in that table.  Per step of 64 windows the lanes translate 64 + 7 codons into LDS as codon bytes, lane p
 * packs window p from aligned LDS words as k_extract does, and a ballot / popcount prefix ranks the selected windows.  Two
 * launches: FORM 0 counts per piece, a prefix sum gives base[piece], FORM 1 / 2 scan again and write at base[piece] + rank -- block
 * order, inside a block the scanner's order (rising positions on the forward strand, from the block's end downward on the
 * reverse one), no atomic per record.
 *   FORM 1: builder records {value, taxid of the block's sequence}, written straight behind the builder's list
 *   FORM 2: bare values and (optionally) the index of the block each came from (mtb_extract_blocks)
 * Algorithmic HBM bytes: one byte per base of every block per launch (the 21 bases two neighbouring steps share come from L2) +
 * 16 B per record; nowhere near the build's bound, which is the two sorts of finish() (profiles/index_build_notes.md). */
#ifndef MTB_KERNELS_EXTRACT_BLOCKS_H
#define MTB_KERNELS_EXTRACT_BLOCKS_H
#include "dev_util.h"
#include "mtb_core.h"

/* pieces of every block: the piece table is its exclusive prefix sum */
__global__ __launch_bounds__(256) void k_block_pieces(const mtb_seq_block *__restrict__ blocks, uint64_t n_blocks, uint32_t *__restrict__ n_pieces) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_blocks) return;
    n_pieces[i] = (uint32_t)mtb_block_pieces(blocks[i].start, blocks[i].end);
}

struct BlockScanArgs {
    const char *bases; const uint64_t *offs;            /* the call's sequences, concatenated; offs[n_seqs + 1] */
    const mtb_seq_block *blocks; uint64_t n_blocks;
    const uint64_t *piece_start;                        /* [n_blocks + 1]: first piece of every block; [n_blocks] = n_pieces */
    uint64_t n_pieces;
    int32_t syncmer, smer_len;
};

template <int FORM>
__global__ __launch_bounds__(64) void k_extract_blocks(BlockScanArgs a, const mtb_tables *__restrict__ tabs, uint32_t *__restrict__ counts,
                                                       const uint64_t *__restrict__ base, const int32_t *__restrict__ seq_taxid,
                                                       mtb_kmer *__restrict__ rec, uint64_t *__restrict__ values, uint32_t *__restrict__ block_of) {
    __shared__ mtb_tables s_tab;
    __shared__ __attribute__((aligned(8))) uint8_t s_cod[80];
    const uint32_t lane = threadIdx.x;
    for (uint32_t i = lane; i < sizeof(mtb_tables) / 4; i += 64) ((uint32_t *)&s_tab)[i] = ((const uint32_t *)tabs)[i];
    __syncthreads();
    for (uint64_t piece = blockIdx.x; piece < a.n_pieces; piece += gridDim.x) {          /* everything up to the ballots is wave-uniform */
        /* the block that owns the piece: the last one whose first piece is <= piece (blocks without a window own no piece and are stepped over) */
        uint64_t lo = 0, hi = a.n_blocks;
        while (hi - lo > 1) { const uint64_t mid = lo + ((hi - lo) >> 1); if (a.piece_start[mid] <= piece) lo = mid; else hi = mid; }
        const uint64_t b = lo;
        const mtb_seq_block blk = a.blocks[b];
        const char *seq = a.bases + a.offs[blk.seq];
        const bool fwd = blk.strand >= 0;
        const uint64_t n_cod = mtb_block_codons(blk.start, blk.end), n_win = mtb_block_windows(blk.start, blk.end);
        const uint64_t w_begin = (piece - a.piece_start[b]) * MTB_BLOCK_PIECE_WINDOWS;
        const uint64_t w_end = w_begin + MTB_BLOCK_PIECE_WINDOWS < n_win ? w_begin + MTB_BLOCK_PIECE_WINDOWS : n_win;
        uint64_t wpos = FORM != 0 ? base[piece] : 0;
        uint32_t total = 0;
        for (uint64_t w0 = w_begin; w0 < w_end; w0 += 64) {
            const uint64_t j = w0 + lane, j2 = w0 + 64 + lane;
            if (j < n_cod) s_cod[lane] = mtb_block_codon(&s_tab, seq, blk.start, blk.end, j, fwd);
            if (lane < 8 && j2 < n_cod) s_cod[64 + lane] = mtb_block_codon(&s_tab, seq, blk.start, blk.end, j2, fwd);
            __syncthreads();
            bool ok = false; uint64_t v = 0;
            if (j < w_end) {          /* the window's 8 codon bytes from three aligned LDS words + two byte alignments */
                const uint32_t *c32 = (const uint32_t *)s_cod;
                const uint32_t q = lane >> 2, sh = lane & 3u;
                const uint32_t x0 = c32[q], x1 = c32[q + 1], x2 = c32[q + 2];
                ok = mtb_window_metamer_words(__builtin_amdgcn_alignbyte(x1, x0, sh), __builtin_amdgcn_alignbyte(x2, x1, sh), a.syncmer, a.smer_len, &v);
            }
            const uint64_t mask = __ballot(ok);
            if (FORM != 0 && ok) {
                const uint64_t at = wpos + (uint64_t)__popcll(mask & lanemask_lt());
                if (FORM == 1) { mtb_kmer r; r.value = v; r.qinfo = (uint64_t)(uint32_t)seq_taxid[blk.seq]; rec[at] = r; }
                else { values[at] = v; if (block_of) block_of[at] = (uint32_t)b; }
            }
            const uint32_t c = (uint32_t)__popcll(mask);
            wpos += c; total += c;
            __syncthreads();
        }
        if (FORM == 0 && lane == 0) counts[piece] = total;
    }
}

#endif
