// test-only: metabuli_amd/csrc/host/clade_filter.h as a stand-alone host program (tests/test_clade_filter_host.py compares its output
// with tests/clade_filter_spec.py).
// usage: clade_filter_check TAXDIR SELECT EXCLUDE [TAXIDS]        lists: A,B,.. or - for none
//   refused <no_ids|unknown|below_species> <id>
//   keep <one 0/1 character per id of [0, max_id]>
//   stats <records in> <records kept> <species kept> <species dropped> <unmatched> <first unmatched>      (with TAXIDS: one record per id,
//         keyed by the species table a merge builds: build_tax2species over every id the taxonomy knows)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../metabuli_amd/csrc/host/clade_filter.h"

static std::vector<int32_t> ids_of(const char *arg) {
    std::vector<int32_t> out;
    if (!strcmp(arg, "-")) return out;
    const std::string v = arg;
    for (size_t at = 0; at <= v.size();) {
        const size_t end = std::min(v.find(',', at), v.size());
        out.push_back((int32_t)strtol(v.substr(at, end - at).c_str(), nullptr, 10));
        at = end + 1;
    }
    return out;
}

int main(int argc, char **argv) {
    if (argc < 4) { fprintf(stderr, "usage: clade_filter_check TAXDIR SELECT EXCLUDE [TAXIDS]\n"); return 2; }
    mtbhost::Taxonomy t;
    std::string err;
    if (!mtbhost::load_taxonomy(argv[1], &t, &err)) { fprintf(stderr, "error: %s\n", err.c_str()); return 1; }
    const std::vector<int32_t> sel = ids_of(argv[2]), exc = ids_of(argv[3]);
    mtbhost::CladeFilter f;
    if (!mtbhost::clade_filter_make(t, sel.data(), (uint32_t)sel.size(), exc.data(), (uint32_t)exc.size(), &f, &err)) {
        static const char *const kind[] = {"ok", "no_ids", "unknown", "below_species"};
        if (err.empty() || (f.refusal != mtbhost::CLADE_NO_IDS && err.find(std::to_string(f.refused_id)) == std::string::npos)) { fprintf(stderr, "error: the message does not name the id: %s\n", err.c_str()); return 1; }
        printf("refused %s %d\n", kind[f.refusal], f.refused_id);
        return 0;
    }
    std::string bits(f.keep.size(), '0');
    for (size_t i = 0; i < f.keep.size(); i++) if (f.keep[i]) bits[i] = '1';
    printf("keep %s\n", bits.c_str());
    if (argc > 4) {
        std::vector<int32_t> all;
        for (int32_t i = 0; i <= t.max_id; i++) if (t.cn(i) >= 0) all.push_back(i);
        mtbhost::build_tax2species(&t, all.data(), all.size());
        std::vector<uint8_t> met(f.keep.size(), 0);
        unsigned long long n_in = 0, n_kept = 0;
        for (int32_t id : ids_of(argv[4])) {
            const int32_t s = (id >= 0 && id <= t.max_id) ? t.tax2species[(size_t)id] : 0;
            met[(size_t)s] = 1; n_in++; n_kept += f.keep[(size_t)s] ? 1 : 0;
        }
        const mtbhost::CladeFilterCounts k = mtbhost::clade_filter_counts(t, f, met.data());
        printf("stats %llu %llu %llu %llu %u %d\n", n_in, n_kept, (unsigned long long)k.n_species_kept, (unsigned long long)k.n_species_dropped, k.n_unmatched, k.first_unmatched);
    }
    return 0;
}
