/* mtb_build -- build, update or merge a database on the GPU (plain C++ over the C ABI, include/mtb.h).
 *
 *   mtb_build [--add-db OLDDB]... [--split-num N] [--syncmer 0|1] [--smer-len n] [--kmer-format 1|2] [--device d]
 *             GENOMES.fa[.gz] SEQID2TAXID.tsv TAXONOMYDIR OUTDB
 *
 * The sort + per-species LCA dedup of the reference's `build` (IndexCreator::createIndex) and the merge of `updateDB`
 * (mergeTargetFiles<DB_CREATION>): every FASTA record is extracted in ALL SIX FRAMES -- there is no gene prediction here, so the
 * result is not what the reference's Prodigal-guided `build` writes for the same genomes --, the first word of its header is looked up
 * in the two-column map (sequence id, taxid), and the entries of every --add-db database are merged in.  GENOMES.fa may be `-` when
 * only --add-db arguments are given (a pure merge; the map is not read then).  OUTDB receives diffIdx, info, split, taxID_list,
 * db.parameters (mtb_index_write) and a copy of TAXONOMYDIR's *.dmp files in OUTDB/taxonomy, so that `mtb_classify ... OUTDB` runs
 * with no further arguments. */
#include <dirent.h>
#include <sys/stat.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../../include/mtb.h"
#include "fastx.h"

static void die(const std::string &m) { throw std::runtime_error(m); }
static void chk(mtb_status s, const char *what) { if (s != MTB_OK) die(std::string(what) + ": " + mtb_last_error()); }

static void copy_file(const std::string &from, const std::string &to) {
    struct stat a, b;
    if (stat(from.c_str(), &a) == 0 && stat(to.c_str(), &b) == 0 && a.st_dev == b.st_dev && a.st_ino == b.st_ino) return;      /* OUTDB/taxonomy is TAXONOMYDIR */
    std::ifstream in(from, std::ios::binary);
    if (!in) die("cannot read " + from);
    std::ofstream out(to, std::ios::binary | std::ios::trunc);
    if (!out) die("cannot create " + to);
    std::vector<char> buf(1 << 20);
    while (in.read(buf.data(), (std::streamsize)buf.size()) || in.gcount() > 0) out.write(buf.data(), in.gcount());      /* (an empty merged.dmp is fine) */
    out.flush();
    if (!out) die("short write to " + to);
}

int main(int argc, char **argv) {
    try {
        std::vector<std::string> add_db, pos;
        int split_num = 4096, device = 0;
        mtb_params par;
        mtb_default_params(&par);
        par.kmer_format = 2; par.syncmer = 0; par.smer_len = 5; par.skip_redundancy = 1;
        for (int i = 1; i < argc; i++) {
            const std::string a = argv[i];
            auto val = [&]() -> std::string { if (i + 1 >= argc) die("flag " + a + " needs a value"); return argv[++i]; };
            if (a == "--add-db") add_db.push_back(val());
            else if (a == "--split-num") split_num = atoi(val().c_str());
            else if (a == "--syncmer") par.syncmer = atoi(val().c_str());
            else if (a == "--smer-len") par.smer_len = atoi(val().c_str());
            else if (a == "--kmer-format") par.kmer_format = atoi(val().c_str());
            else if (a == "--device") device = atoi(val().c_str());
            else if (a.size() > 2 && a.rfind("--", 0) == 0) die("unknown flag " + a);
            else pos.push_back(a);
        }
        if (pos.size() != 4) {
            fprintf(stderr, "usage: mtb_build [--add-db OLDDB]... [--split-num N] [--syncmer 0|1] [--smer-len n] [--kmer-format 1|2] [--device d] "
                            "GENOMES.fa[.gz] SEQID2TAXID.tsv TAXONOMYDIR OUTDB\n");
            return 1;
        }
        const std::string genomes = pos[0], map_path = pos[1], taxdir = pos[2], outdb = pos[3];
        if (genomes == "-" && add_db.empty()) die("nothing to build: no genomes and no --add-db");
        if (split_num < 2) die("--split-num must be at least 2");

        std::unordered_map<std::string, int32_t> seq2tax;
        if (genomes != "-") {
            std::ifstream in(map_path);
            if (!in) die("cannot open " + map_path);
            std::string line;
            while (std::getline(in, line)) {
                const size_t a = line.find_first_of(" \t");
                if (line.empty() || a == std::string::npos) continue;
                const size_t b = line.find_first_not_of(" \t", a);
                if (b == std::string::npos) continue;
                seq2tax[line.substr(0, a)] = (int32_t)strtol(line.c_str() + b, nullptr, 10);
            }
        }

        mtb_ctx *ctx = nullptr;
        chk(mtb_ctx_create(device, nullptr, &ctx), "mtb_ctx_create");
        mtb_builder *bld = nullptr;
        chk(mtb_builder_create(ctx, taxdir.c_str(), &par, &bld), "mtb_builder_create");

        for (const std::string &db : add_db) {
            mtb_params q = par;
            mtb_index *old = nullptr;
            chk(mtb_index_open(ctx, db.c_str(), taxdir.c_str(), &q, &old), ("open " + db).c_str());
            const mtb_status s = mtb_builder_add_index(bld, old);
            const std::string err = s == MTB_OK ? std::string() : std::string(mtb_last_error());
            const unsigned long long n_old = mtb_index_num_targets(old);
            mtb_index_close(old);
            if (s != MTB_OK) die("add " + db + ": " + err);
            fprintf(stderr, "mtb_build: %llu entries of %s\n", n_old, db.c_str());
        }

        unsigned long long n_seqs = 0, n_bases = 0;
        if (genomes != "-") {
            mtbhost::FastxReader rd(genomes, 4);
            mtbhost::FlatBatch batch;
            std::vector<int32_t> taxids;
            /* one add_sequences call (an upload, a two-pass extraction, a few stream synchronisations) per ~64 M bases, however many
             * records that is: a contig-level assembly set must not become millions of tiny GPU round trips */
            const size_t BATCH_BASES = 64u << 20, MAX_RECORDS = 1u << 16;
            for (;;) {
                batch.clear();
                size_t ask = 64;
                while (batch.bases.size() < BATCH_BASES && rd.next_batch(ask, batch)) {
                    const size_t avg = batch.bases.size() / batch.size() + 1;
                    ask = batch.bases.size() < BATCH_BASES ? std::min<size_t>(std::max<size_t>((BATCH_BASES - batch.bases.size()) / avg, 1), MAX_RECORDS) : 0;
                }
                if (batch.size() == 0) break;
                taxids.resize(batch.size());
                for (size_t i = 0; i < batch.size(); i++) {
                    std::string id = batch.name(i);
                    id = id.substr(0, id.find_first_of(" \t"));
                    auto it = seq2tax.find(id);
                    if (it == seq2tax.end()) die("sequence " + id + " of " + genomes + " is not in " + map_path);
                    taxids[i] = it->second;
                }
                chk(mtb_builder_add_sequences(bld, batch.bases.data(), batch.offs.data(), taxids.data(), batch.size()), "mtb_builder_add_sequences");
                n_seqs += batch.size(); n_bases += batch.offs[batch.size()];
            }
        }
        const unsigned long long n_rec = mtb_builder_num_records(bld);
        mtb_index *ix = nullptr;
        chk(mtb_builder_finish(bld, &ix), "mtb_builder_finish");
        mkdir(outdb.c_str(), 0755);
        chk(mtb_index_write(ix, outdb.c_str(), split_num), "mtb_index_write");
        const std::string otax = outdb + "/taxonomy";
        mkdir(otax.c_str(), 0755);
        {
            DIR *d = opendir(taxdir.c_str());
            if (!d) die("cannot list " + taxdir);
            std::vector<std::string> names;
            while (struct dirent *e = readdir(d)) { const std::string n = e->d_name; if (n.size() > 4 && n.compare(n.size() - 4, 4, ".dmp") == 0) names.push_back(n); }
            closedir(d);
            for (const std::string &n : names) copy_file(taxdir + "/" + n, otax + "/" + n);
        }
        fprintf(stderr, "mtb_build: %llu sequences (%llu bases), %llu records -> %llu entries in %s (six-frame extraction, no gene prediction)\n",
                n_seqs, n_bases, n_rec, (unsigned long long)mtb_index_num_targets(ix), outdb.c_str());
        mtb_index_close(ix);
        mtb_builder_destroy(bld);
        mtb_ctx_destroy(ctx);
        return 0;
    } catch (const std::exception &e) {
        fprintf(stderr, "mtb_build: %s\n", e.what());
        return 1;
    }
}
