/* TEST INFRASTRUCTURE ONLY: prints what metabuli_amd/csrc/host/cds_info.h makes of an annotation and a genome file, for comparison with
 * the Python restatement tests/cds_spec.py (tests/test_cds_info.py).
 *
 *   cds_dump LIST GENOMES.fa
 *
 * LIST: one annotation FASTA path per line.  Output: a `stats` line; per genome record `seq <index> <name> blocks|sixframes`; then
 * every block (`block <seq> <strand> <start> <end>`) and every joined CDS (`extra <seq> <owner> <bases>`) of ONE call over all
 * genome records.  An error (coordinates outside a sequence, an unreadable coordinate) goes to stderr with exit status 1. */
#include <cstdio>
#include <string>

#include "../../metabuli_amd/csrc/host/fastx.h"
#include "../../metabuli_amd/csrc/host/cds_info.h"

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: cds_dump LIST GENOMES.fa\n"); return 2; }
    try {
        mtbhost::CdsMap cds;
        mtbhost::cds_load_list(argv[1], &cds);
        const mtbhost::CdsStats &s = cds.stats;
        printf("stats records=%llu cds=%llu pseudo=%llu hypothetical=%llu orphan_location=%llu no_location=%llu two_digit_version=%llu accessions=%zu\n",
               s.records, s.cds, s.pseudo, s.hypothetical, s.orphan_location, s.no_location, s.two_digit_version, cds.by_accession.size());
        mtbhost::FastxReader rd(argv[2], 1);
        mtbhost::FlatBatch g;
        g.clear();
        while (rd.next_batch(1u << 20, g)) {}
        mtbhost::CdsBlocks cb;
        for (size_t i = 0; i < g.size(); i++) {
            std::string id = g.name(i);
            id = id.substr(0, id.find_first_of(" \t"));
            auto it = cds.by_accession.find(id);
            printf("seq %zu %s %s\n", i, id.c_str(), it == cds.by_accession.end() ? "sixframes" : "blocks");
            if (it != cds.by_accession.end()) mtbhost::cds_divide(it->second, id, g.bases.data() + g.offs[i], g.offs[i + 1] - g.offs[i], (uint32_t)i, &cb);
        }
        mtbhost::cds_finish_extras(&cb, (uint32_t)g.size());
        for (const mtb_seq_block &b : cb.blocks) printf("block %u %d %llu %llu\n", b.seq, b.strand, (unsigned long long)b.start, (unsigned long long)b.end);
        size_t at = 0;
        for (size_t k = 0; k < cb.extra_lens.size(); k++) {
            printf("extra %zu %u %s\n", g.size() + k, cb.extra_owner[k], cb.extra_bases.substr(at, cb.extra_lens[k]).c_str());
            at += cb.extra_lens[k];
        }
        return 0;
    } catch (const std::exception &e) {
        fprintf(stderr, "cds_dump: %s\n", e.what());
        return 1;
    }
}
