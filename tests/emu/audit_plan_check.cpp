/* TEST INFRASTRUCTURE ONLY: the host side of the database audit (metabuli_amd/csrc/host/audit_plan.h) as a stand-alone program, so
 * that it can run under AddressSanitizer + UBSan (tests/test_audit_plan.py).  Seeded random split tables and word streams:
 *   - audit_usable_checkpoints keeps exactly merge_input_from_split's records, with their record numbers, sorted by word offset;
 *   - audit_chunk_checkpoints hands every one of them to exactly one chunk of a random tiling of the stream (the chunk whose words
 *     (w0, w0 + n] hold its offset), or counts it as missed: offset 0, or behind the last chunk;
 *   - audit_trailing_words against a plain backward scan, across its read buffer's size;
 *   - audit_check_files: presence, emptiness, sizes, the taxonomy directory, the db.parameters note.
 * Prints "OK <checks>" and returns 0, or the first failure and 1. */
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>
#include <string>

#include "../../metabuli_amd/csrc/host/audit_plan.h"

using namespace mtbhost;

static long g_checks = 0;
#define CHECK(c) do { g_checks++; if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

static void put(const std::string &path, const std::string &bytes) { FILE *f = fopen(path.c_str(), "wb"); if (f) { fwrite(bytes.data(), 1, bytes.size(), f); fclose(f); } }

int main() {
    std::mt19937_64 rng(7);
    for (int round = 0; round < 300; round++) {
        const uint64_t n_entries = 1 + rng() % 5000, n_words = n_entries + rng() % (3 * n_entries);
        std::vector<MergeCheckpoint> split(rng() % 40);
        uint64_t ad = 0, info = 0;
        for (size_t r = 0; r < split.size(); r++) {
            ad += (rng() % 4) << 24; info += rng() % (n_entries / 8 + 2);
            MergeCheckpoint c{ad | (rng() & 0xFFFFFF), rng() % (n_words + 3), info};
            switch (rng() % 8) { case 0: c.ad = 0; break; case 1: c.ad = UINT64_MAX; break; case 2: c.info_off = rng() % (n_entries + 5); break; case 3: c.diff_off = 0; break; default: break; }
            split[r] = c;
        }
        if (round % 7 == 0) for (MergeCheckpoint &c : split) c = MergeCheckpoint{0, 0, 0};
        MergeInput in;
        merge_input_from_split(split.data(), split.size(), n_entries, n_words, &in);
        const std::vector<AuditCheckpoint> cps = audit_usable_checkpoints(split, n_entries, n_words);
        CHECK(cps.size() == in.cps.size());
        std::set<uint64_t> records;
        for (size_t k = 0; k < cps.size(); k++) {
            const AuditCheckpoint &a = cps[k];
            CHECK(a.record >= 1 && a.record < split.size());
            CHECK(split[a.record].ad == a.cp.ad && split[a.record].diff_off == a.cp.diff_off && split[a.record].info_off == a.cp.info_off);
            CHECK(records.insert(a.record).second);
            if (k) CHECK(cps[k - 1].cp.diff_off <= a.cp.diff_off);
        }
        {   /* the records in file order are the rule's, in its order */
            std::vector<uint64_t> by_record(records.begin(), records.end());
            for (size_t k = 0; k < by_record.size(); k++) CHECK(split[by_record[k]].info_off == in.cps[k].info_off && split[by_record[k]].ad == in.cps[k].ad);
        }
        /* a random tiling of the first `decoded` words */
        const uint64_t decoded = n_words - rng() % (n_words / 4 + 1);
        size_t next = 0; uint64_t missed = 0, first_missed = UINT64_MAX, taken = 0, w0 = 0;
        std::vector<AuditCheckpoint> take;
        std::set<uint64_t> seen;
        while (w0 < decoded) {
            const uint64_t n = std::min<uint64_t>(1 + rng() % 700, decoded - w0);
            audit_chunk_checkpoints(cps, &next, w0, n, &take, &missed, &first_missed);
            for (const AuditCheckpoint &a : take) { CHECK(a.cp.diff_off > w0 && a.cp.diff_off <= w0 + n); CHECK(seen.insert(a.record).second); taken++; }
            w0 += n;
        }
        uint64_t want_missed = 0, want_first = UINT64_MAX, behind = 0;
        for (const AuditCheckpoint &a : cps) {
            if (a.cp.diff_off == 0) { want_missed++; want_first = std::min(want_first, a.record); }
            else if (a.cp.diff_off > decoded) behind++;
        }
        CHECK(missed == want_missed && first_missed == want_first);
        CHECK(taken + missed + behind == cps.size() && cps.size() - next == behind);
    }
    char tmpl[] = "/tmp/audit_plan_check_XXXXXX";
    const char *dir = mkdtemp(tmpl);
    CHECK(dir != nullptr);
    const std::string d(dir);
    {   /* trailing words, across the 65536-word read buffer */
        const std::string path = d + "/words";
        for (uint64_t n : std::vector<uint64_t>{0, 1, 5, 65535, 65536, 65537, 200000})
            for (uint64_t last_end : std::vector<uint64_t>{UINT64_MAX, 0, n / 2, n > 0 ? n - 1 : 0}) {
                if (last_end != UINT64_MAX && last_end >= n) continue;
                std::vector<uint16_t> w(n);
                for (uint64_t i = 0; i < n; i++) w[i] = (uint16_t)(rng() & 0x7FFF) | (last_end != UINT64_MAX && i <= last_end && rng() % 3 == 0 ? 0x8000u : 0u);
                if (last_end != UINT64_MAX) w[last_end] |= 0x8000u;
                put(path, std::string((const char *)w.data(), n * 2));
                uint64_t t = 77;
                CHECK(audit_trailing_words(path, n, &t));
                CHECK(t == (last_end == UINT64_MAX ? n : n - 1 - last_end));
            }
        uint64_t t = 0;
        CHECK(!audit_trailing_words(d + "/absent", 4, &t));
    }
    {   /* the file checks */
        const std::string db = d + "/db";
        AuditFiles f; std::string err;
        CHECK(!audit_check_files(db, nullptr, &f, &err) && err.find("Database directory does not exist") != std::string::npos);
        mkdir(db.c_str(), 0755); mkdir((db + "/taxonomy").c_str(), 0755);
        CHECK(!audit_check_files(db, nullptr, &f, &err) && err == "Error: \"diffIdx\" file is missing in the database directory.");
        put(db + "/diffIdx", std::string(6, 'x'));
        CHECK(!audit_check_files(db, nullptr, &f, &err));
        for (const char *name : {"\"info\"", "\"split\"", "\"taxID_list\"", "\"nodes.dmp\"", "\"names.dmp\"", "\"merged.dmp\"", "Please check the database directory"}) CHECK(err.find(name) != std::string::npos);
        CHECK(!f.all_present && f.note.find("db.parameters") != std::string::npos);
        put(db + "/info", std::string(8, 'x')); put(db + "/split", ""); put(db + "/taxID_list", "");
        for (const char *name : {"nodes.dmp", "names.dmp", "merged.dmp"}) put(db + "/taxonomy/" + name, "");
        f = AuditFiles();
        CHECK(audit_check_files(db, nullptr, &f, &err) && f.n_words == 3 && f.n_info_entries == 2 && f.all_present && err.empty());
        put(db + "/db.parameters", "");
        f = AuditFiles();
        CHECK(audit_check_files(db, "", &f, &err) && f.note.empty());
        CHECK(!audit_check_files(db, (d + "/elsewhere").c_str(), &f, &err) && err.find(d + "/elsewhere") != std::string::npos);
        put(db + "/taxonomyDB", "x");
        CHECK(audit_check_files(db, (d + "/elsewhere").c_str(), &f, &err));                /* taxonomyDB wins, as for mtb_index_open */
        put(db + "/info", std::string(7, 'x'));
        CHECK(!audit_check_files(db, nullptr, &f, &err) && err == "Error: info file size is not a multiple of 4." && f.all_present);
        put(db + "/info", "");
        CHECK(!audit_check_files(db, nullptr, &f, &err) && err == "Error: info file is empty.");
        put(db + "/diffIdx", std::string(5, 'x'));
        CHECK(!audit_check_files(db, nullptr, &f, &err) && err == "Error: diffIdx file size is not a multiple of 2.");
        put(db + "/diffIdx", "");
        CHECK(!audit_check_files(db, nullptr, &f, &err) && err == "Error: diffIdx file is empty.");
    }
    if (system(("rm -rf '" + d + "'").c_str()) != 0) return 1;
    printf("OK %ld checks\n", g_checks);
    return 0;
}
