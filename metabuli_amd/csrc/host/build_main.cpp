/* mtb_build -- build, update or merge a database on the GPU (plain C++ over the C ABI, include/mtb.h).
 *
 *   mtb_build [--add-db OLDDB]... [--cds-info LIST] [--max-records N] [--split-num N] [--syncmer 0|1] [--smer-len n] [--kmer-format 1|2]
 *             [--device d] GENOMES.fa[.gz] SEQID2TAXID.tsv TAXONOMYDIR OUTDB
 *
 * The sort + per-species LCA dedup of the reference's `build` (IndexCreator::createIndex) and the merge of `updateDB`
 * (mergeTargetFiles<DB_CREATION>).  Without --cds-info every FASTA record is extracted in ALL SIX FRAMES -- there is no gene
 * prediction here, so the result is not what the reference's Prodigal-guided `build` writes for the same genomes.  With
 * --cds-info LIST (a text file, one cds_from_genomic FASTA path per line, as the reference takes it) a record whose name has an
 * entry in the annotation is cut into its CDS and the regions between them, each scanned in one frame (host/cds_info.h,
 * mtb_builder_add_blocks): the reference's `build --cds-info LIST --mask 0` up to the departures cds_info.h lists; a record
 * without an entry has no gene predictor to fall back to and is extracted in six frames, and the closing line says how many
 * records took which route.  kmer_format 2 only.  The first word of a record's header is looked up
 * in the two-column map (sequence id, taxid), and the entries of every --add-db database are merged in.  GENOMES.fa may be `-` when
 * only --add-db arguments are given (a pure merge; the map is not read then).  OUTDB receives diffIdx, info, split, taxID_list,
 * db.parameters (mtb_index_write) and a copy of TAXONOMYDIR's *.dmp files in OUTDB/taxonomy, so that `mtb_classify ... OUTDB` runs
 * with no further arguments.
 * A build larger than one builder (IndexCreator::createIndex writes one partial index per RAM-sized batch and mergeTargetFiles
 * streams them together): when the builder holds --max-records N records (default: what mtb_builder_capacity reports for this
 * device, below 2^32) it is finished and written to OUTDB/tmp_parts/part_K, and at the end the parts and every --add-db database --
 * which then never enter a builder -- are merged by mtb_merge_databases, one value range at a time; tmp_parts is removed.  A pure
 * merge (GENOMES `-`) always takes that route.  A build that fits takes the in-memory one; the files are the same either way.
 *
 *   mtb_build --audit 1 - - TAXONOMYDIR DBDIR      audit only (mtb_database_audit): the report is printed, DBDIR/sp2uniqKmerCnt (the
 *             reference's per-species entry counts, Classifier.cpp:390-440) is written, exit 1 if the database is not valid
 *   --validate-db 1 on any build, update or merge: OUTDB is audited after it is written; the run fails if it is not canonical
 *   mtb_build --inspect 1 [--inspect-level dna|aa|both] - - TAXONOMYDIR DBDIR      inspect only (mtb_database_inspect): LCA k-mer counts per
 *   taxon in DBDIR/kmer_lca_report.tsv (dna) / kmer_lca_report_aa.tsv (aa), count-common-kmers' by-rank summary on stdout; with --audit 1
 *   both in one run.  --inspect 1 on any build, update or merge: OUTDB is inspected after it is written
 *
 *   mtb_build --add-db DB [--add-db DB2]... [--select-taxid A,B,..] [--exclude-taxid C,..] - - TAXONOMYDIR OUTDB
 *             a subset of a database, or a merge without a clade (mtb_merge_databases_filtered; the flag names and the comma syntax
 *             are classifiedRefiner's): only the entries of species under a selected taxon (all, if none is selected) and under no
 *             excluded one are written.  Ids at or above species rank; legal for a pure merge only (GENOMES `-`), and always
 *             streamed.  Prints the kept / dropped entries and species and one warning for listed ids under which nothing was met */
#include <dirent.h>
#include <sys/stat.h>
#include <unistd.h>

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
#include "cds_info.h"
#include "audit_plan.h"

static void die(const std::string &m) { throw std::runtime_error(m); }
static void chk(mtb_status s, const char *what) { if (s != MTB_OK) die(std::string(what) + ": " + mtb_last_error()); }

static void remove_tree(const std::string &dir) {
    DIR *d = opendir(dir.c_str());
    if (!d) return;
    std::vector<std::string> names;
    while (struct dirent *e = readdir(d)) { const std::string n = e->d_name; if (n != "." && n != "..") names.push_back(n); }
    closedir(d);
    for (const std::string &n : names) {
        const std::string p = dir + "/" + n;
        struct stat st;
        if (lstat(p.c_str(), &st) == 0 && S_ISDIR(st.st_mode)) remove_tree(p); else unlink(p.c_str());
    }
    rmdir(dir.c_str());
}
static unsigned long long entries_of(const std::string &db) {
    struct stat st;
    if (stat((db + "/info").c_str(), &st) != 0) die("cannot open " + db + "/info");
    return (unsigned long long)st.st_size / 4;
}

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

/* mtb_database_audit of `db` with its report printed; counts: also DBDIR/sp2uniqKmerCnt */
static mtb_audit_report audit(mtb_ctx *ctx, const std::string &db, const std::string &taxdir, mtb_params par, bool counts) {
    printf("Validating database: %s\n", db.c_str());
    std::vector<uint32_t> cnt;
    mtb_audit_report r;
    if (counts) {       /* the array's size is the taxonomy's: an array without room is refused with that number before any device work */
        uint32_t none = 0;
        const mtb_status q = mtb_database_audit(ctx, db.c_str(), taxdir.c_str(), &par, 0, &none, 0, &r);
        if (q != MTB_ERR_CAPACITY) chk(q, ("audit " + db).c_str());
        cnt.assign((size_t)r.n_species, 0);
    }
    const mtb_status s = mtb_database_audit(ctx, db.c_str(), taxdir.c_str(), &par, 0, counts ? cnt.data() : nullptr, cnt.size(), &r);
    chk(s, ("audit " + db).c_str());
    mtbhost::audit_print_counts(stdout, stderr, r);
    mtbhost::audit_print_findings(stderr, r);
    printf("Audited: %llu entries in %llu chunks, %llu checkpoints (%llu bad), %llu species, %llu ids without a species; valid %d, canonical %d; "
           "read %.1f ms, decode %.1f ms, check %.1f ms, counts %.1f ms, total %.1f ms\n",
           (unsigned long long)r.n_entries, (unsigned long long)r.n_chunks, (unsigned long long)r.n_checkpoints, (unsigned long long)r.n_bad_checkpoints,
           (unsigned long long)r.n_species, (unsigned long long)r.n_no_species, r.valid, r.canonical, r.ms_read, r.ms_decode, r.ms_check, r.ms_hist, r.ms_total);
    if (counts) chk(mtb_audit_write_species_counts(db.c_str(), cnt.data(), cnt.size()), "write sp2uniqKmerCnt");
    fflush(stdout);
    return r;
}

/* mtb_database_inspect of `db` at the chosen levels (bit 0: dna, bit 1: aa): DBDIR/kmer_lca_report.tsv / kmer_lca_report_aa.tsv, the
 * by-rank summary in count-common-kmers' wording and one line with the groups, the largest one and the size histogram */
static void inspect(mtb_ctx *ctx, const std::string &db, const std::string &taxdir, const mtb_params &par0, int levels) {
    for (int level = 0; level < 2; level++) {
        if (!(levels & (1 << level))) continue;
        printf("Counting common k-mers by taxonomic rank: %s (%s level)\n", db.c_str(), level ? "aa" : "dna");
        mtb_params par = par0;
        mtb_inspect_report r;
        uint64_t none = 0;       /* the arrays' size is the taxonomy's: arrays without room are refused with that number before any device work */
        const mtb_status q = mtb_database_inspect(ctx, db.c_str(), taxdir.c_str(), &par, 0, level, &none, &none, 0, &r);
        if (q != MTB_ERR_CAPACITY) chk(q, ("inspect " + db).c_str());
        std::vector<uint64_t> distinct((size_t)r.n_taxa, 0), entries((size_t)r.n_taxa, 0);
        chk(mtb_database_inspect(ctx, db.c_str(), taxdir.c_str(), &par, 0, level, distinct.data(), entries.data(), distinct.size(), &r), ("inspect " + db).c_str());
        const std::string tsv = db + (level ? "/kmer_lca_report_aa.tsv" : "/kmer_lca_report.tsv");
        std::vector<char> summary(1 << 16);
        chk(mtb_inspect_write_report(nullptr, db.c_str(), taxdir.c_str(), distinct.data(), entries.data(), distinct.size(), r.n_groups, tsv.c_str(), summary.data(), summary.size()),
            "write the inspection report");
        fputs(summary.data(), stdout);
        printf("Inspected (%s): %llu entries in %llu chunks, %llu groups (%llu groups, %llu entries in all, without a known id), largest group %llu at entry %lld; groups by floor(log2 size):",
               level ? "aa" : "dna", (unsigned long long)r.n_entries, (unsigned long long)r.n_chunks, (unsigned long long)r.n_groups, (unsigned long long)r.n_orphan_groups,
               (unsigned long long)r.n_orphan_entries, (unsigned long long)r.max_group, r.max_group ? (long long)r.first_max_group : -1ll);
        int top = 0;
        for (int k = 0; k < MTB_INSPECT_HIST_SLOTS; k++) if (r.size_hist[k]) top = k;
        for (int k = 0; k <= top; k++) printf(" %llu", (unsigned long long)r.size_hist[k]);
        printf("; read %.1f ms, decode %.1f ms, inspect %.1f ms, bins %.1f ms, total %.1f ms; report in %s\n", r.ms_read, r.ms_decode, r.ms_inspect, r.ms_bins, r.ms_total, tsv.c_str());
    }
    fflush(stdout);
}

int main(int argc, char **argv) {
    try {
        std::vector<std::string> add_db, pos;
        bool audit_only = false, validate_db = false;
        bool inspect_on = false; int inspect_level_bits = 1;       /* --inspect 1; --inspect-level: bit 0 dna (default), bit 1 aa */
        std::string cds_list;
        std::vector<int32_t> select_ids, exclude_ids;
        bool filter_given = false;
        auto id_list = [&](const std::string &flag, const std::string &v, std::vector<int32_t> *out) {      /* A,B,.. */
            filter_given = true;
            for (size_t at = 0; at <= v.size();) {
                const size_t end = std::min(v.find(',', at), v.size());
                const std::string tok = v.substr(at, end - at);
                char *stop = nullptr;
                const long id = strtol(tok.c_str(), &stop, 10);
                if (tok.empty() || *stop || id < 0 || id > 0x7FFFFFFFl) die(flag + ": '" + tok + "' is not a taxon id (expected A,B,..)");
                out->push_back((int32_t)id);
                at = end + 1;
            }
        };
        int split_num = 4096, device = 0;
        unsigned long long max_records = 0;          /* 0: from the device */
        mtb_params par;
        mtb_default_params(&par);
        par.kmer_format = 2; par.syncmer = 0; par.smer_len = 5; par.skip_redundancy = 1;
        for (int i = 1; i < argc; i++) {
            const std::string a = argv[i];
            auto val = [&]() -> std::string { if (i + 1 >= argc) die("flag " + a + " needs a value"); return argv[++i]; };
            if (a == "--add-db") add_db.push_back(val());
            else if (a == "--cds-info") cds_list = val();
            else if (a == "--split-num") split_num = atoi(val().c_str());
            else if (a == "--max-records") { max_records = strtoull(val().c_str(), nullptr, 10); if (max_records == 0) die("--max-records must be at least 1"); }
            else if (a == "--syncmer") par.syncmer = atoi(val().c_str());
            else if (a == "--smer-len") par.smer_len = atoi(val().c_str());
            else if (a == "--kmer-format") par.kmer_format = atoi(val().c_str());
            else if (a == "--device") device = atoi(val().c_str());
            else if (a == "--audit") audit_only = atoi(val().c_str()) != 0;
            else if (a == "--validate-db") validate_db = atoi(val().c_str()) != 0;
            else if (a == "--inspect") { const std::string v = val(); if (v != "0" && v != "1") die("--inspect: '" + v + "' is not 0 or 1"); inspect_on = v == "1"; }
            else if (a == "--inspect-level") {
                const std::string v = val();
                if (v == "dna") inspect_level_bits = 1; else if (v == "aa") inspect_level_bits = 2; else if (v == "both") inspect_level_bits = 3;
                else die("--inspect-level: '" + v + "' is not dna, aa or both");
            }
            else if (a == "--select-taxid") id_list(a, val(), &select_ids);
            else if (a == "--exclude-taxid") id_list(a, val(), &exclude_ids);
            else if (a.size() > 2 && a.rfind("--", 0) == 0) die("unknown flag " + a);
            else pos.push_back(a);
        }
        if (pos.size() != 4) {
            fprintf(stderr, "usage: mtb_build [--add-db OLDDB]... [--cds-info LIST] [--max-records N] [--split-num N] [--syncmer 0|1] [--smer-len n] [--kmer-format 1|2] [--device d] "
                            "[--validate-db 0|1] [--inspect 0|1 [--inspect-level dna|aa|both]] GENOMES.fa[.gz] SEQID2TAXID.tsv TAXONOMYDIR OUTDB\n"
                            "       mtb_build --audit 1 [--device d] - - TAXONOMYDIR DBDIR\n       mtb_build --inspect 1 [--inspect-level dna|aa|both] [--audit 1] [--device d] - - TAXONOMYDIR DBDIR\n"
                            "       mtb_build --add-db DB [--add-db DB2]... [--select-taxid A,B,..] [--exclude-taxid C,..] - - TAXONOMYDIR OUTDB\n");
            return 1;
        }
        const std::string genomes = pos[0], map_path = pos[1], taxdir = pos[2], outdb = pos[3];
        const int inspect_levels = inspect_on ? inspect_level_bits : 0;
        if (audit_only || (inspect_levels && genomes == "-" && add_db.empty())) {       /* an existing DBDIR: audited, inspected or both */
            mtb_ctx *actx = nullptr;
            chk(mtb_ctx_create(device, nullptr, &actx), "mtb_ctx_create");
            bool valid = true;
            if (audit_only) valid = audit(actx, outdb, taxdir, par, true).valid != 0;
            if (inspect_levels) inspect(actx, outdb, taxdir, par, inspect_levels);
            mtb_ctx_destroy(actx);
            if (!valid) { fprintf(stderr, "Database validation failed.\n"); return 1; }
            return 0;
        }
        if (genomes == "-" && add_db.empty()) die("nothing to build: no genomes and no --add-db");
        if (filter_given && genomes != "-")
            die("--select-taxid / --exclude-taxid filter a merge of databases only (--add-db DB ... - - TAXONOMYDIR OUTDB): they cannot be combined with genomes on the command line");
        if (split_num < 2) die("--split-num must be at least 2");
        if (!cds_list.empty() && par.kmer_format != 2) die("--cds-info needs --kmer-format 2 (block extraction implements no other)");

        mtbhost::CdsMap cds;
        if (!cds_list.empty() && genomes != "-") {
            mtbhost::cds_load_list(cds_list, &cds);
            fprintf(stderr, "mtb_build: CDS annotation: %llu records, %llu CDS of %zu sequences (%llu pseudo, %llu hypothetical, %llu without a location, "
                            "%llu locations without a protein_id skipped, %llu records with a two-digit accession version)\n",
                    cds.stats.records, cds.stats.cds, cds.by_accession.size(), cds.stats.pseudo, cds.stats.hypothetical, cds.stats.no_location,
                    cds.stats.orphan_location, cds.stats.two_digit_version);
        }

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

        const bool max_given = max_records != 0;
        if (!max_given) { uint64_t cap = 0; chk(mtb_builder_capacity(bld, &cap), "mtb_builder_capacity"); max_records = std::max<uint64_t>(cap - cap / 4, 1); }      /* a batch may overshoot */
        if (max_records >= (1ull << 32)) max_records = (1ull << 32) - 1;
        mkdir(outdb.c_str(), 0755);
        const std::string parts_dir = outdb + "/tmp_parts";
        std::vector<std::string> parts;
        unsigned long long n_rec = 0;
        /* the builder's records become a database of their own */
        auto spill = [&]() {
            if (parts.empty()) { remove_tree(parts_dir); mkdir(parts_dir.c_str(), 0755); }
            const std::string pd = parts_dir + "/part_" + std::to_string(parts.size());
            mkdir(pd.c_str(), 0755);
            n_rec += mtb_builder_num_records(bld);
            mtb_index *part = nullptr;
            chk(mtb_builder_finish(bld, &part), "mtb_builder_finish");
            const mtb_status s = mtb_index_write(part, pd.c_str(), split_num);
            const std::string err = s == MTB_OK ? std::string() : std::string(mtb_last_error());
            mtb_index_close(part);
            if (s != MTB_OK) die("write " + pd + ": " + err);
            parts.push_back(pd);
        };

        unsigned long long n_seqs = 0, n_bases = 0, n_by_blocks = 0, n_six_frames = 0, n_cds_single = 0, n_cds_joined = 0, n_noncds = 0;
        if (genomes != "-") {
            mtbhost::FastxReader rd(genomes, 4);
            mtbhost::FlatBatch batch;
            std::vector<int32_t> taxids;
            /* one add_sequences call (an upload, a two-pass extraction, a few stream synchronisations) per ~64 M bases, however many
             * records that is: a contig-level assembly set must not become millions of tiny GPU round trips */
            const size_t BATCH_BASES = (size_t)std::min<unsigned long long>(64u << 20, std::max<unsigned long long>(max_records / 4, 1)), MAX_RECORDS = 1u << 16;      /* a batch yields up to two records per base */
            for (;;) {
                batch.clear();
                size_t ask = BATCH_BASES < (64u << 20) ? 1 : 64;      /* a small --max-records: feel the way, a record at a time */
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
                n_seqs += batch.size(); n_bases += batch.offs[batch.size()];
                if (cds_list.empty()) {
                    chk(mtb_builder_add_sequences(bld, batch.bases.data(), batch.offs.data(), taxids.data(), batch.size()), "mtb_builder_add_sequences");
                    if (mtb_builder_num_records(bld) >= max_records) spill();
                    continue;
                }
                /* records with an annotation entry -> blocks; the others -> six frames, as one compacted call */
                mtbhost::CdsBlocks cb;
                std::vector<char> plain_bases; std::vector<uint64_t> plain_offs(1, 0); std::vector<int32_t> plain_tax;
                const size_t n0 = batch.size();
                for (size_t i = 0; i < n0; i++) {
                    std::string id = batch.name(i);
                    id = id.substr(0, id.find_first_of(" \t"));
                    const char *seq = batch.bases.data() + batch.offs[i];
                    const uint64_t len = batch.offs[i + 1] - batch.offs[i];
                    auto it = cds.by_accession.find(id);
                    if (it == cds.by_accession.end()) {
                        plain_bases.insert(plain_bases.end(), seq, seq + len); plain_offs.push_back(plain_bases.size()); plain_tax.push_back(taxids[i]);
                        n_six_frames++;
                    } else { mtbhost::cds_divide(it->second, id, seq, len, (uint32_t)i, &cb); n_by_blocks++; }
                }
                if (!plain_tax.empty())
                    chk(mtb_builder_add_sequences(bld, plain_bases.data(), plain_offs.data(), plain_tax.data(), plain_tax.size()), "mtb_builder_add_sequences");
                /* the joined CDS go behind the genomes as sequences of the same call */
                mtbhost::cds_finish_extras(&cb, (uint32_t)n0);
                batch.bases.append(cb.extra_bases.data(), cb.extra_bases.data() + cb.extra_bases.size());
                for (size_t k = 0; k < cb.extra_lens.size(); k++) { batch.offs.push_back(batch.offs[batch.offs.size() - 1] + cb.extra_lens[k]); taxids.push_back(taxids[cb.extra_owner[k]]); }
                if (!cb.blocks.empty())
                    chk(mtb_builder_add_blocks(bld, batch.bases.data(), batch.offs.data(), taxids.data(), taxids.size(), cb.blocks.data(), cb.blocks.size()), "mtb_builder_add_blocks");
                n_cds_single += cb.n_cds_single; n_cds_joined += cb.n_cds_joined; n_noncds += cb.n_noncds;
                if (mtb_builder_num_records(bld) >= max_records) spill();
            }
        }
        unsigned long long n_old = 0, n_entries = 0;
        for (const std::string &db : add_db) n_old += entries_of(db);
        const bool streamed = genomes == "-" || !parts.empty() || mtb_builder_num_records(bld) + n_old > max_records;
        mtb_merge_stats ms = mtb_merge_stats();
        mtb_filter_stats fs = mtb_filter_stats();
        if (!streamed) {
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
            n_rec = mtb_builder_num_records(bld);
            mtb_index *ix = nullptr;
            chk(mtb_builder_finish(bld, &ix), "mtb_builder_finish");
            chk(mtb_index_write(ix, outdb.c_str(), split_num), "mtb_index_write");
            n_entries = mtb_index_num_targets(ix);
            mtb_index_close(ix);
        } else {
            if (mtb_builder_num_records(bld)) spill();
            std::vector<const char *> dirs;
            for (const std::string &p : parts) dirs.push_back(p.c_str());
            for (const std::string &db : add_db) { dirs.push_back(db.c_str()); fprintf(stderr, "mtb_build: %llu entries of %s\n", entries_of(db), db.c_str()); }
            const mtb_clade_filter flt = {select_ids.data(), (uint32_t)select_ids.size(), exclude_ids.data(), (uint32_t)exclude_ids.size()};
            const mtb_status s = filter_given
                ? mtb_merge_databases_filtered(ctx, dirs.data(), (uint32_t)dirs.size(), taxdir.c_str(), &par, outdb.c_str(), split_num, max_given ? max_records : 0, &flt, &ms, &fs)
                : mtb_merge_databases(ctx, dirs.data(), (uint32_t)dirs.size(), taxdir.c_str(), &par, outdb.c_str(), split_num, max_given ? max_records : 0, &ms);
            const std::string err = s == MTB_OK ? std::string() : std::string(mtb_last_error());
            remove_tree(parts_dir);
            if (s != MTB_OK) die(std::string(filter_given ? "mtb_merge_databases_filtered: " : "mtb_merge_databases: ") + err);
            if (filter_given) {
                fprintf(stderr, "mtb_build: filter kept %llu of %llu entries (%llu dropped), %llu of %llu species (%llu dropped), %.1f ms\n",
                        (unsigned long long)fs.n_records_kept, (unsigned long long)fs.n_records_in, (unsigned long long)(fs.n_records_in - fs.n_records_kept),
                        (unsigned long long)fs.n_species_kept, (unsigned long long)(fs.n_species_kept + fs.n_species_dropped), (unsigned long long)fs.n_species_dropped, fs.ms_filter);
                if (fs.n_unmatched) fprintf(stderr, "mtb_build: warning: no entry of the inputs lies under taxon %d\n", fs.first_unmatched);
                if (fs.n_unmatched > 1) fprintf(stderr, "mtb_build: warning: ... nor under %u further listed taxa\n", fs.n_unmatched - 1);
            }
            n_entries = ms.n_entries;
        }
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
        char route[96] = "";
        if (streamed) snprintf(route, sizeof(route), " in %zu parts, %llu ranges", parts.size(), (unsigned long long)ms.n_ranges);
        if (genomes == "-")
            fprintf(stderr, "mtb_build: %zu databases (%llu entries) -> %llu entries in %s, merged in %llu ranges\n", add_db.size(), n_old, n_entries, outdb.c_str(),
                    (unsigned long long)ms.n_ranges);
        else if (cds_list.empty())
            fprintf(stderr, "mtb_build: %llu sequences (%llu bases), %llu records -> %llu entries in %s%s (six-frame extraction, no gene prediction)\n",
                    n_seqs, n_bases, n_rec, n_entries, outdb.c_str(), route);
        else
            fprintf(stderr, "mtb_build: %llu sequences (%llu bases), %llu records -> %llu entries in %s%s (CDS annotation: %llu sequences by blocks -- %llu CDS, "
                            "%llu joined CDS, %llu non-CDS regions --, %llu sequences without a CDS entry in six frames; no gene prediction, no masking)\n",
                    n_seqs, n_bases, n_rec, n_entries, outdb.c_str(), route, n_by_blocks, n_cds_single, n_cds_joined, n_noncds, n_six_frames);
        mtb_builder_destroy(bld);
        bool sound = true;
        if (validate_db) {
            sound = audit(ctx, outdb, taxdir, par, false).canonical != 0;
            if (!sound) fprintf(stderr, "mtb_build: %s is not a canonical database\nDatabase validation failed.\n", outdb.c_str());
        }
        if (inspect_levels) inspect(ctx, outdb, taxdir, par, inspect_levels);
        mtb_ctx_destroy(ctx);
        return sound ? 0 : 1;
    } catch (const std::exception &e) {
        fprintf(stderr, "mtb_build: %s\n", e.what());
        return 1;
    }
}
