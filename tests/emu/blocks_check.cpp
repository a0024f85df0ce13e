/* TEST INFRASTRUCTURE ONLY: the block-scan functions of metabuli_amd/csrc/mtb_core.h (mtb_block_*) on the host, as a stand-alone
 * program, so that they can be compared with the oracle and run under -fsanitize=address,undefined (tests/test_blocks_spec.py).
 *
 *   blocks_check CASES.txt
 *
 * Every line of CASES.txt: <bases or "-" for none> <start> <end> <strand> <syncmer> <smer_len>.  The bases are copied into a heap
 * buffer of exactly their length (no terminator), so that a read outside the sequence is an error the sanitizer sees.  Per line
 * the program prints the number of windows emitted and their values in hexadecimal, in the scanner's order; it also walks the
 * block piece by piece (MTB_BLOCK_PIECE_WINDOWS) the way the kernel does and fails if that order differs. */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../metabuli_amd/csrc/mtb_core.h"

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: blocks_check CASES.txt\n"); return 2; }
    std::ifstream in(argv[1]);
    if (!in) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    mtb_tables tab;
    mtb_build_tables(&tab);
    std::string line;
    while (std::getline(in, line)) {
        if (line.empty()) continue;
        std::istringstream ls(line);
        std::string bases; unsigned long long start, end; int strand, syncmer, smer_len;
        if (!(ls >> bases >> start >> end >> strand >> syncmer >> smer_len)) { fprintf(stderr, "bad line: %s\n", line.c_str()); return 2; }
        if (bases == "-") bases.clear();
        char *seq = (char *)malloc(bases.size() ? bases.size() : 1);
        memcpy(seq, bases.data(), bases.size());
        const bool fwd = strand >= 0;
        std::vector<uint64_t> whole, pieced;
        const uint64_t n_win = mtb_block_windows(start, end);
        for (uint64_t p = 0; p < n_win; p++) {
            uint64_t v;
            if (mtb_block_window(&tab, seq, start, end, p, fwd, syncmer, smer_len, &v)) whole.push_back(v);
        }
        /* the kernel's walk: pieces of MTB_BLOCK_PIECE_WINDOWS windows, steps of 64, codon bytes staged for 64 + 7 codons */
        const uint64_t n_cod = mtb_block_codons(start, end);
        for (uint64_t piece = 0; piece < mtb_block_pieces(start, end); piece++) {
            const uint64_t w_begin = piece * MTB_BLOCK_PIECE_WINDOWS;
            const uint64_t w_end = w_begin + MTB_BLOCK_PIECE_WINDOWS < n_win ? w_begin + MTB_BLOCK_PIECE_WINDOWS : n_win;
            for (uint64_t w0 = w_begin; w0 < w_end; w0 += 64) {
                uint8_t cod[72];
                memset(cod, 0xEE, sizeof(cod));
                for (uint64_t l = 0; l < 72; l++) if (w0 + l < n_cod) cod[l] = mtb_block_codon(&tab, seq, start, end, w0 + l, fwd);
                for (uint64_t l = 0; l < 64 && w0 + l < w_end; l++) {
                    uint64_t v;
                    if (mtb_window_metamer(cod + l, syncmer, smer_len, &v)) pieced.push_back(v);
                }
            }
        }
        free(seq);
        if (whole != pieced) { fprintf(stderr, "piecewise walk differs from the window-by-window one: %s\n", line.c_str()); return 1; }
        printf("%zu", whole.size());
        for (uint64_t v : whole) printf(" %llx", (unsigned long long)v);
        printf("\n");
    }
    return 0;
}
