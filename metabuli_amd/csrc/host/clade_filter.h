/* clade_filter.h -- which species keys a filtered merge keeps (mtb_merge_databases_filtered; mtb_build --select-taxid / --exclude-taxid,
 * the reference's flag names and comma syntax from classifiedRefiner).  Pure host C++, no HIP.
 *
 * A database holds one entry per (value, species key) and the entry's id is the LCA of that species' own genomes, so taking out a
 * whole species -- or any clade at or above species rank -- leaves exactly the database a build without those genomes gives.  The
 * species key of an entry is what k_merge_keys puts into the high word of a record: tax2species[id] of the merge's taxonomy.
 *
 *   key s is KEPT iff (select is empty, or a selected taxon is s or an ancestor of s) and no excluded taxon is s or an ancestor of s
 *   key 0 (ids without a species: root-labelled entries) is kept iff select is empty and the root is not excluded
 *
 * Ids are read under the merge's taxonomy after merged.dmp aliasing.  Refused (the message names the id): an id the taxonomy does
 * not know; an id strictly below its own species key (Taxonomy::at_rank(cn(id), species) != cn(id), the root excepted): a strain
 * cannot be taken out of a species' LCA'd entries exactly; both lists empty.
 * keep[0 .. max_id] comes from one memoised climb over parent[]: every node is visited once. */
#ifndef MTB_CLADE_FILTER_H
#define MTB_CLADE_FILTER_H
#include <cstdint>
#include <string>
#include <vector>

#include "../host_db.h"

namespace mtbhost {

enum CladeRefusal { CLADE_OK = 0, CLADE_NO_IDS = 1, CLADE_UNKNOWN_ID = 2, CLADE_BELOW_SPECIES = 3 };

struct CladeFilter {
    CladeRefusal refusal = CLADE_OK; int32_t refused_id = 0;      /* why clade_filter_make said no, and about which id */
    std::vector<int32_t> select, exclude;          /* canonical ids, in the order listed */
    std::vector<int32_t> select_as_given, exclude_as_given;
    std::vector<uint8_t> keep;                     /* [0, max_id]: by species key */
};

struct CladeFilterCounts { uint64_t n_species_kept = 0, n_species_dropped = 0; uint32_t n_unmatched = 0; int32_t first_unmatched = 0; };

inline bool clade_is_root(const Taxonomy &t, int32_t c) { return c >= 0 && c <= t.max_id && t.parent[(size_t)c] == c; }

/* false: a refusal, *err names the id */
inline bool clade_filter_make(const Taxonomy &t, const int32_t *select, uint32_t n_select, const int32_t *exclude, uint32_t n_exclude, CladeFilter *out, std::string *err) {
    *out = CladeFilter();
    if (n_select + (uint64_t)n_exclude == 0) { out->refusal = CLADE_NO_IDS; *err = "neither a selected nor an excluded taxon: nothing to filter (use mtb_merge_databases)"; return false; }
    if ((n_select && !select) || (n_exclude && !exclude)) { out->refusal = CLADE_NO_IDS; *err = "NULL id list"; return false; }
    const int SPECIES = find_rank_index("species");
    const size_t sz = (size_t)t.max_id + 1;
    enum : uint8_t { DONE = 1, SEL = 2, EXC = 4 };
    std::vector<uint8_t> state(sz, 0);             /* SEL / EXC: listed here, until the climb has folded the ancestors in */
    bool root_excluded = false;
    for (int list = 0; list < 2; list++) {
        const int32_t *ids = list ? exclude : select;
        const uint32_t n = list ? n_exclude : n_select;
        for (uint32_t k = 0; k < n; k++) {
            const int32_t id = ids[k], c = t.cn(id);
            const char *what = list ? "excluded" : "selected";
            if (c < 0) { out->refusal = CLADE_UNKNOWN_ID; out->refused_id = id; *err = std::string(what) + " taxon " + std::to_string(id) + " is not in the taxonomy"; return false; }
            if (!clade_is_root(t, c) && t.at_rank(c, SPECIES) != c) {
                out->refusal = CLADE_BELOW_SPECIES; out->refused_id = id;
                *err = std::string(what) + " taxon " + std::to_string(id) + " lies below species rank (species " + std::to_string(t.at_rank(c, SPECIES)) +
                       "): a strain cannot be taken out of its species' entries";
                return false;
            }
            state[(size_t)c] |= list ? EXC : SEL;
            if (list && clade_is_root(t, c)) root_excluded = true;
            (list ? out->exclude : out->select).push_back(c);
            (list ? out->exclude_as_given : out->select_as_given).push_back(id);
        }
    }
    std::vector<int32_t> path;
    for (size_t n0 = 0; n0 < sz; n0++) {
        if (t.canon[n0] != (int32_t)n0 || (state[n0] & DONE)) continue;
        path.clear();
        int32_t c = (int32_t)n0;
        while (!(state[(size_t)c] & DONE) && !clade_is_root(t, c) && path.size() <= sz) { path.push_back(c); c = t.parent[(size_t)c]; }
        state[(size_t)c] |= DONE;                  /* the root (its own flags are all it has) or a node already folded */
        uint8_t above = state[(size_t)c] & (SEL | EXC);
        for (size_t k = path.size(); k-- > 0;) { uint8_t &s = state[(size_t)path[k]]; s |= above | DONE; above = s & (SEL | EXC); }
    }
    out->keep.assign(sz, 0);
    for (size_t n0 = 1; n0 < sz; n0++) {
        const int32_t c = t.canon[n0];             /* an alias follows its node */
        if (c < 0) continue;
        const uint8_t s = state[(size_t)c];
        out->keep[n0] = ((n_select == 0 || (s & SEL)) && !(s & EXC)) ? 1 : 0;
    }
    out->keep[0] = (n_select == 0 && !root_excluded) ? 1 : 0;
    return true;
}

/* met[s] != 0: a record with species key s was seen (s in [0, max_id]) -> distinct keys kept / dropped, and the listed taxa under
 * which no record was met (select first, then exclude, each listed id counted) */
inline CladeFilterCounts clade_filter_counts(const Taxonomy &t, const CladeFilter &f, const uint8_t *met) {
    CladeFilterCounts r;
    const size_t sz = (size_t)t.max_id + 1;
    std::vector<uint8_t> under(sz, 0);             /* a met key is this node or lies below it */
    for (size_t s = 0; s < sz; s++) {
        if (!met[s]) continue;
        if (f.keep[s]) r.n_species_kept++; else r.n_species_dropped++;
        int32_t c = s ? t.canon[s] : -1;
        size_t steps = 0;
        while (c >= 0 && !under[(size_t)c] && steps++ <= sz) { under[(size_t)c] = 1; if (clade_is_root(t, c)) break; c = t.parent[(size_t)c]; }
    }
    for (int list = 0; list < 2; list++) {
        const std::vector<int32_t> &ids = list ? f.exclude : f.select, &given = list ? f.exclude_as_given : f.select_as_given;
        for (size_t k = 0; k < ids.size(); k++) {
            const bool hit = under[(size_t)ids[k]] || (met[0] && clade_is_root(t, ids[k]));      /* key 0: records of the root */
            if (hit) continue;
            if (r.n_unmatched++ == 0) r.first_unmatched = given[k];
        }
    }
    return r;
}

} // namespace mtbhost
#endif
