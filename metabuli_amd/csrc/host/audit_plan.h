/* audit_plan.h -- the host side of mtb_database_audit that needs no device: the file checks of the reference's validateDatabase
 * (validateDatabase.cpp:26-69, 88-96, 114-121: same order, same wording), the words behind the last end word of diffIdx, which
 * checkpoints of `split` a chunk of the stream has to judge, and the lines the programs print for a report.  Pure host C++, no HIP:
 * mtb_classify runs the file checks before it touches a device. */
#ifndef MTB_AUDIT_PLAN_H
#define MTB_AUDIT_PLAN_H
#include <sys/stat.h>
#include <unistd.h>
#include <fcntl.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../../../include/mtb.h"
#include "merge_plan.h"

namespace mtbhost {

struct AuditFiles {
    uint64_t n_words = 0, n_info_entries = 0;
    bool all_present = false;              /* the presence checks passed (the size checks follow them) */
    std::string note;                      /* the reference's warnings (a missing db.parameters): not an error */
};

inline bool audit_is_file(const std::string &p, uint64_t *size = nullptr) {
    struct stat st;
    if (stat(p.c_str(), &st) != 0 || !S_ISREG(st.st_mode)) return false;
    if (size) *size = (uint64_t)st.st_size;
    return true;
}
inline bool audit_is_dir(const std::string &p) { struct stat st; return stat(p.c_str(), &st) == 0 && S_ISDIR(st.st_mode); }

/* false: *err holds the reference's message(s), each naming its file.  taxonomy_dir: as for mtb_index_open (NULL / empty:
 * DBDIR/taxonomy); the reference only warns when neither taxonomyDB nor a taxonomy directory is there, because --taxonomy-path may
 * still bring one -- here the path is known, so a database without any taxonomy fails. */
inline bool audit_check_files(const std::string &db, const char *taxonomy_dir, AuditFiles *out, std::string *err) {
    err->clear();
    auto add = [&](const std::string &m) { if (!err->empty()) *err += " "; *err += m; };
    if (!audit_is_dir(db)) { *err = "Error: Database directory does not exist: " + db; return false; }
    uint64_t sz_diff = 0, sz_info = 0;
    if (!audit_is_file(db + "/diffIdx", &sz_diff)) { *err = "Error: \"diffIdx\" file is missing in the database directory."; return false; }
    if (!audit_is_file(db + "/info", &sz_info)) add("Error: \"info\" file is missing in the database directory.");
    if (!audit_is_file(db + "/split")) add("Error: \"split\" file is missing in the database directory.");
    if (!audit_is_file(db + "/taxID_list")) add("Error: \"taxID_list\" file is missing in the database directory.");
    if (!audit_is_file(db + "/taxonomyDB")) {
        const bool own = !(taxonomy_dir && *taxonomy_dir);
        const std::string td = own ? db + "/taxonomy" : std::string(taxonomy_dir);
        const std::string where = own ? "\"DBDIR/taxonomy\"" : td;
        if (!audit_is_dir(td)) add("Error: \"taxonomyDB\" file is missing in the database directory and there is no taxonomy directory " + td + ".");
        else for (const char *f : {"nodes.dmp", "names.dmp", "merged.dmp"})
            if (!audit_is_file(td + "/" + f)) add(std::string("Error: \"") + f + "\" file is missing in the " + where + " directory.");
    }
    if (!audit_is_file(db + "/db.parameters"))
        out->note = "Warning: \"db.parameters\" file is missing in the database directory. It means the database was built using an old Metabuli version";
    if (!err->empty()) { add("Please check the database directory and make sure all required files are present."); return false; }
    out->all_present = true;
    if (sz_diff == 0) { *err = "Error: diffIdx file is empty."; return false; }
    if (sz_diff % 2 != 0) { *err = "Error: diffIdx file size is not a multiple of 2."; return false; }
    if (sz_info == 0) { *err = "Error: info file is empty."; return false; }
    if (sz_info % 4 != 0) { *err = "Error: info file size is not a multiple of 4."; return false; }
    out->n_words = sz_diff / 2; out->n_info_entries = sz_info / 4;
    return true;
}

/* 16-bit words of diffIdx behind its last end word (0x8000): they code no entry.  false: a read failed. */
inline bool audit_trailing_words(const std::string &path, uint64_t n_words, uint64_t *trailing) {
    *trailing = 0;
    const int fd = open(path.c_str(), O_RDONLY);
    if (fd < 0) return false;
    std::vector<uint16_t> buf(1u << 16);
    uint64_t end = n_words; bool ok = true, found = false;
    while (end > 0 && !found) {
        const uint64_t n = std::min<uint64_t>(buf.size(), end), at = end - n;
        uint64_t got = 0;
        while (got < n * 2) { const ssize_t r = pread(fd, (char *)buf.data() + got, n * 2 - got, (off_t)(at * 2 + got)); if (r <= 0) { ok = false; break; } got += (uint64_t)r; }
        if (!ok) break;
        for (uint64_t k = n; k-- > 0;) if (buf[k] & 0x8000u) { *trailing = n_words - (at + k + 1); found = true; break; }
        end = at;
    }
    close(fd);
    if (ok && !found) *trailing = n_words;
    return ok;
}

/* The records of a raw split table that the audit judges: merge_input_from_split's, with their record numbers.  (That rule skips
 * record 0 and records that no reader would start from; what it keeps is identified here by its info_off, which the rule makes
 * strictly ascending.) */
struct AuditCheckpoint { MergeCheckpoint cp; uint64_t record; };
inline std::vector<AuditCheckpoint> audit_usable_checkpoints(const std::vector<MergeCheckpoint> &split, uint64_t n_entries, uint64_t n_words) {
    MergeInput in;
    merge_input_from_split(split.data(), split.size(), n_entries, n_words, &in);
    std::vector<AuditCheckpoint> out;
    size_t r = 1;
    for (const MergeCheckpoint &c : in.cps) {
        while (r < split.size() && !(split[r].ad == c.ad && split[r].diff_off == c.diff_off && split[r].info_off == c.info_off)) r++;
        out.push_back(AuditCheckpoint{c, (uint64_t)r});
        r++;
    }
    std::stable_sort(out.begin(), out.end(), [](const AuditCheckpoint &a, const AuditCheckpoint &b) { return a.cp.diff_off < b.cp.diff_off; });
    return out;
}
/* the checkpoints (sorted by diff_off, from *next on) whose diff_off lies in (w0, w0 + n_use]: those of the chunk that holds file
 * words [w0, w0 + n_use); checkpoints at or below w0 that were not taken before can never be judged good: they are counted in *missed
 * (first one in *first_missed) */
inline void audit_chunk_checkpoints(const std::vector<AuditCheckpoint> &cps, size_t *next, uint64_t w0, uint64_t n_use, std::vector<AuditCheckpoint> *take,
                                    uint64_t *missed, uint64_t *first_missed) {
    take->clear();
    while (*next < cps.size() && cps[*next].cp.diff_off <= w0 + n_use) {
        const AuditCheckpoint &c = cps[*next];
        if (c.cp.diff_off > w0) take->push_back(c);
        else { ++*missed; *first_missed = std::min(*first_missed, c.record); }
        ++*next;
    }
}

/* what mtb_classify --validate-db 1 and mtb_build --audit / --validate-db print behind the reference's progress lines: one line per
 * non-zero finding of a report */
inline void audit_print_findings(FILE *f, const mtb_audit_report &r) {
    auto line = [&](const char *what, uint64_t n, uint64_t first, const char *unit) {
        if (!n) return;
        if (first == UINT64_MAX) fprintf(f, "Error: %llu %s.\n", (unsigned long long)n, what);
        else fprintf(f, "Error: %llu %s; the first is %s %llu.\n", (unsigned long long)n, what, unit, (unsigned long long)first);
    };
    line("16-bit words of diffIdx lie behind its last end word", r.n_trailing_words, UINT64_MAX, "");
    line("entries whose value is below their predecessor's", r.n_value_descents, r.first_value_descent, "entry");
    line("entries whose id is not in the taxonomy", r.n_unknown_ids, r.first_unknown_id, "entry");
    line("checkpoints of split do not lie where they claim to", r.n_bad_checkpoints, r.first_bad_checkpoint, "record");
    auto note = [&](const char *what, uint64_t n, uint64_t first) {
        if (!n) return;
        if (first == UINT64_MAX) fprintf(f, "Note: %llu %s.\n", (unsigned long long)n, what);
        else fprintf(f, "Note: %llu %s; the first is entry %llu.\n", (unsigned long long)n, what, (unsigned long long)first);
    };
    note("entries of equal value do not ascend in species (not canonical)", r.n_group_disorder, r.first_group_disorder);
    note("entries whose id is absent from taxID_list (not canonical)", r.n_unlisted_ids, r.first_unlisted_id);
    note("entries whose id has no species: counted for none", r.n_no_species, UINT64_MAX);
}
/* the reference's count lines (validateDatabase.cpp:110, 123-129); true if the counts agree */
inline bool audit_print_counts(FILE *out, FILE *err, const mtb_audit_report &r) {
    fprintf(out, "Number of k-mers in diffIdx file: %llu\n", (unsigned long long)r.n_end_words);
    fprintf(out, "Number of k-mer IDs in info file: %llu\n", (unsigned long long)r.n_info_entries);
    if (r.n_end_words != r.n_info_entries) {
        fprintf(err, "Error: Number of k-mers in diffIdx file (%llu) does not match the number of k-mer IDs in info file (%llu).\nPlease check the database files.\n",
                (unsigned long long)r.n_end_words, (unsigned long long)r.n_info_entries);
        return false;
    }
    fprintf(out, "Number of k-mers in diffIdx file matches the number of k-mer IDs in info file.\n");
    return true;
}

} // namespace mtbhost
#endif
