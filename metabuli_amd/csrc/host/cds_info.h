/* cds_info.h -- CDS annotation -> sequence blocks for mtb_builder_add_blocks (host side of `mtb_build --cds-info LIST`).
 *
 * The reference's `build --cds-info LIST` reads the cds_from_genomic FASTA files that ship with RefSeq / GenBank assemblies
 * (IndexCreator::loadCdsInfo, IndexCreator.cpp:1275-1384), cuts every annotated genome into its CDS and the regions between them
 * (SeqIterator::devideToCdsAndNonCds, SeqIterator.cpp:180-244) and scans each piece in ONE frame, forward
 * (IndexCreator.cpp:1094-1127).  This header restates the two steps so that the pieces become blocks of the resident genome
 * instead of copies of it; only a CDS joined from several locations is copied (its exons are not adjacent in the genome).
 *
 * Header of an annotation record:   >lcl|NC_000913.3_cds_NP_414542.1_1 [gene=thrL] [protein_id=NP_414542.1] [location=190..255]
 *   - accession key: the text after the first '|', up to the first '.', plus ONE more character -- "NC_000913.3".  A two-digit
 *     version (".12") is therefore cut to ".1" and does not match its genome; reproduced, and counted (two_digit_version).
 *   - the [feature=value] tags in order: `pseudo`, or `protein=hypothetical protein`, ends the record; `frame` is remembered;
 *     `protein_id` opens a CDS; `location` is parsed into the open CDS and ends the record.
 *   - location: complement(...), join(...), a..b, a single coordinate, '<' / '>' marks; 1-based, inclusive.  frame != 1 moves the
 *     first location's begin up (forward strand) or the last location's end down (complement) by frame - 1.
 * CDS -> blocks: the first location is extended downwards and the last one upwards in steps of 3 bases, up to
 * MTB_CDS_EXTEND_CODONS times each while it stays inside the sequence (the loop conditions of SeqIterator.cpp:195 / :203;
 * SeqIterator's kmerLen is 12, SeqIterator.h:46, so 11 codons = 33 bases per side).  One location: a block of the genome, strand
 * +1, or -1 for complement -- the forward scan of the reverse complement of a substring is the reverse scan of the substring.
 * Several: the pieces are concatenated into an extra sequence, reverse-complemented for complement, scanned whole and forward.
 * Non-CDS: maximal runs of bases no location covers (frame-adjusted coordinates, no extension) longer than 32 bases, each scanned
 * forward from its first base.
 *
 * Departures from the reference:
 *   1. IndexCreator.cpp:1123 scans non-CDS string k over the length of CDS string k (out of range, or a neighbour's length);
 *      here every non-CDS region is scanned over its own length.
 *   2. a `location` with no `protein_id` before it in its record indexes an empty vector there (or extends the accession's
 *      previous CDS); here it is skipped and counted (orphan_location).
 *   3. coordinates outside the sequence read outside it there; here they are an error that names the record.
 * Also: the reference starts looking for the first '[' at the offset of the name's '.', and never leaves a record that has no
 * `location`; here every tag is walked and a record without a location simply ends.  Complementing goes through the base classes
 * of mtb_core.h (a code outside them becomes N), as the reverse scan does. */
#ifndef MTB_HOST_CDS_INFO_H
#define MTB_HOST_CDS_INFO_H
#include <stdint.h>
#include <zlib.h>

#include <cstdlib>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../../include/mtb.h"

namespace mtbhost {

#define MTB_CDS_EXTEND_CODONS 11      /* SeqIterator::kmerLen - 1 (SeqIterator.h:46, SeqIterator.cpp:195/203) */
#define MTB_CDS_MIN_NONCDS 32         /* a region between CDS counts if it is LONGER than this (SeqIterator.cpp:239) */

struct CdsLoc { long long first, second; };          /* 1-based, inclusive, as annotated (after the frame shift) */
struct CdsEntry { std::vector<CdsLoc> loc; bool complement = false; std::string name; };
struct CdsStats {
    unsigned long long records = 0, cds = 0, pseudo = 0, hypothetical = 0, orphan_location = 0, no_location = 0, two_digit_version = 0;
};
struct CdsMap {
    std::unordered_map<std::string, std::vector<CdsEntry>> by_accession;
    CdsStats stats;
};

namespace cds_detail {
inline long long coordinate(std::string s, const std::string &record) {
    while (!s.empty() && (s[0] == '<' || s[0] == '>' || s[0] == ' ')) s.erase(0, 1);
    while (!s.empty() && s.back() == ' ') s.pop_back();
    if (s.empty() || s.find_first_not_of("0123456789") != std::string::npos) throw std::runtime_error("CDS record " + record + ": cannot read the coordinate '" + s + "'");
    return atoll(s.c_str());
}
/* strips "word(" ... ")" if the text holds it */
inline bool unwrap(std::string *v, const char *word) {
    const std::string open = std::string(word) + "(";
    const size_t at = v->find(open);
    if (at == std::string::npos) return false;
    const size_t close = v->rfind(')');
    const size_t from = at + open.size();
    *v = v->substr(from, close == std::string::npos || close < from ? std::string::npos : close - from);
    return true;
}
}

/* One header line of an annotation file (without the '>'): first word = name, the rest = the tags. */
inline void cds_add_header(const std::string &header, CdsMap *map) {
    CdsStats &st = map->stats;
    st.records++;
    const size_t sp = header.find_first_of(" \t");
    const std::string name = header.substr(0, sp), comment = sp == std::string::npos ? std::string() : header.substr(sp + 1);
    const size_t bar = name.find('|'), from = bar == std::string::npos ? 0 : bar + 1, dot = name.find('.', from);
    const std::string key = dot == std::string::npos ? name.substr(from) : name.substr(from, dot - from + 2);
    if (dot != std::string::npos && dot + 2 < name.size() && name[dot + 2] >= '0' && name[dot + 2] <= '9') st.two_digit_version++;
    int frame = 1;
    bool open = false;
    size_t pos = 0;
    for (;;) {
        const size_t lb = comment.find('[', pos);
        if (lb == std::string::npos) break;
        const size_t rb = comment.find(']', lb);
        if (rb == std::string::npos) break;
        pos = rb + 1;
        const std::string tag = comment.substr(lb + 1, rb - lb - 1);
        const size_t eq = tag.find('=');
        const std::string feature = tag.substr(0, eq), value = eq == std::string::npos ? std::string() : tag.substr(eq + 1);
        if (feature == "pseudo") { st.pseudo++; return; }
        if (feature == "protein" && value == "hypothetical protein") { st.hypothetical++; return; }
        if (feature == "frame") frame = atoi(value.c_str());
        else if (feature == "protein_id") {
            CdsEntry e; e.name = name;
            map->by_accession[key].push_back(e);
            open = true;
        } else if (feature == "location") {
            if (!open) { st.orphan_location++; return; }
            CdsEntry &e = map->by_accession[key].back();
            std::string v = value;
            e.complement = cds_detail::unwrap(&v, "complement");
            cds_detail::unwrap(&v, "join");
            size_t a = 0;
            for (;;) {
                const size_t comma = v.find(',', a);
                const std::string piece = v.substr(a, comma == std::string::npos ? std::string::npos : comma - a);
                const size_t dd = piece.find("..");
                CdsLoc l;
                l.first = cds_detail::coordinate(dd == std::string::npos ? piece : piece.substr(0, dd), name);
                l.second = dd == std::string::npos ? l.first : cds_detail::coordinate(piece.substr(dd + 2), name);
                e.loc.push_back(l);
                if (comma == std::string::npos) break;
                a = comma + 1;
            }
            if (frame != 1) {
                if (!e.complement) e.loc.front().first += frame - 1;
                else e.loc.back().second -= frame - 1;
            }
            st.cds++;
            return;
        }
    }
    if (open) {          /* a protein_id without a location: nothing to scan */
        map->by_accession[key].pop_back();
        if (map->by_accession[key].empty()) map->by_accession.erase(key);
    }
    st.no_location++;
}

/* Every header line of one annotation file, plain or gzip (only the headers matter: the CDS sequences themselves are never used, the
 * genome is cut instead).  The FASTA reader of fastx.h keeps the first word of a header only, hence a line reader of its own. */
inline void cds_load_file(const std::string &path, CdsMap *map) {
    gzFile f = gzopen(path.c_str(), "rb");
    if (!f) throw std::runtime_error("cannot open " + path);
    std::vector<char> buf(1 << 16);
    std::string line;
    bool in_header = false, at_line_start = true;
    for (;;) {
        if (!gzgets(f, buf.data(), (int)buf.size())) break;
        const std::string part = buf.data();
        const bool ends = !part.empty() && part.back() == '\n';
        if (at_line_start) { in_header = !part.empty() && part[0] == '>'; line.clear(); }
        if (in_header) line += part;
        if (ends && in_header) {
            while (!line.empty() && (line.back() == '\n' || line.back() == '\r')) line.pop_back();
            cds_add_header(line.substr(1), map);
        }
        at_line_start = ends;
    }
    if (!at_line_start && in_header) { while (!line.empty() && line.back() == '\r') line.pop_back(); cds_add_header(line.substr(1), map); }
    gzclose(f);
}
/* LIST: one annotation file per line (IndexCreator.cpp:1283-1289) */
inline void cds_load_list(const std::string &list_path, CdsMap *map) {
    gzFile f = gzopen(list_path.c_str(), "rb");
    if (!f) throw std::runtime_error("cannot open " + list_path);
    std::vector<char> buf(1 << 16);
    while (gzgets(f, buf.data(), (int)buf.size())) {
        std::string path = buf.data();
        while (!path.empty() && (path.back() == '\n' || path.back() == '\r' || path.back() == ' ')) path.pop_back();
        if (!path.empty()) cds_load_file(path, map);
    }
    gzclose(f);
}

/* What one call of mtb_builder_add_blocks needs besides the genomes: blocks of the genomes (seq = the genome's index in the call)
 * and the joined CDS as extra sequences; extra k is sequence n_genomes + k of the call once the caller has appended extra_bases
 * behind the genomes (cds_finish_extras writes its blocks). */
struct CdsBlocks {
    std::vector<mtb_seq_block> blocks;
    std::string extra_bases; std::vector<uint64_t> extra_lens; std::vector<uint32_t> extra_owner;        /* owner: the genome's index (its taxid) */
    unsigned long long n_cds_single = 0, n_cds_joined = 0, n_noncds = 0;
    void clear() { *this = CdsBlocks(); }
};

inline char cds_complement(char c) {
    switch (c) {
        case 'A': case 'R': case 'W': case 'a': case 'r': case 'w': return 'T';
        case 'C': case 'M': case 'S': case 'c': case 'm': case 's': return 'G';
        case 'H': case 'T': case 'Y': case 'h': case 't': case 'y': return 'A';
        case 'B': case 'D': case 'G': case 'K': case 'U': case 'b': case 'd': case 'g': case 'k': case 'u': return 'C';
        default: return 'N';
    }
}

/* SeqIterator::devideToCdsAndNonCds for one genome (`seq`, `len` bases, index `seq_index` in the call) */
inline void cds_divide(const std::vector<CdsEntry> &cds, const std::string &accession, const char *seq, uint64_t len, uint32_t seq_index, CdsBlocks *out) {
    for (const CdsEntry &e : cds)
        for (const CdsLoc &l : e.loc)
            if (l.first < 1 || l.second < l.first || (unsigned long long)l.second > len)
                throw std::runtime_error("CDS record " + e.name + ": location " + std::to_string(l.first) + ".." + std::to_string(l.second) + " lies outside sequence " +
                                         accession + " of " + std::to_string(len) + " bases");
    std::string joined;
    for (const CdsEntry &e : cds) {
        const size_t n_loc = e.loc.size();
        joined.clear();
        for (size_t j = 0; j < n_loc; j++) {
            uint64_t begin = (uint64_t)e.loc[j].first - 1, end = (uint64_t)e.loc[j].second - 1;
            if (j == 0) for (int k = 0; k < MTB_CDS_EXTEND_CODONS && begin >= 3; k++) begin -= 3;
            if (j == n_loc - 1) for (int k = 0; k < MTB_CDS_EXTEND_CODONS && end + 3 < len; k++) end += 3;
            if (n_loc == 1) {
                mtb_seq_block b; b.seq = seq_index; b.strand = e.complement ? -1 : 1; b.start = begin; b.end = end;
                out->blocks.push_back(b);
                out->n_cds_single++;
            } else joined.append(seq + begin, end - begin + 1);
        }
        if (n_loc > 1) {
            if (e.complement) {
                std::string rc(joined.size(), 'N');
                for (size_t i = 0; i < joined.size(); i++) rc[joined.size() - 1 - i] = cds_complement(joined[i]);
                joined.swap(rc);
            }
            out->extra_bases += joined; out->extra_lens.push_back(joined.size()); out->extra_owner.push_back(seq_index);
            out->n_cds_joined++;
        }
    }
    std::vector<char> covered(len, 0);
    for (const CdsEntry &e : cds)
        for (const CdsLoc &l : e.loc)
            for (uint64_t k = (uint64_t)l.first - 1; k < (uint64_t)l.second; k++) covered[k] = 1;
    uint64_t i = 0;
    while (i < len) {
        uint64_t run = 0;
        while (i < len && !covered[i]) { i++; run++; }
        if (run > MTB_CDS_MIN_NONCDS) {
            mtb_seq_block b; b.seq = seq_index; b.strand = 1; b.start = i - run; b.end = i - 1;
            out->blocks.push_back(b);
            out->n_noncds++;
        }
        i++;          /* the walk steps over the base that ended the run (SeqIterator.cpp:242) */
    }
}

/* the joined CDS as blocks, once they sit behind n_genomes sequences: each whole, forward */
inline void cds_finish_extras(CdsBlocks *out, uint32_t n_genomes) {
    for (size_t k = 0; k < out->extra_lens.size(); k++) {
        mtb_seq_block b; b.seq = n_genomes + (uint32_t)k; b.strand = 1; b.start = 0; b.end = out->extra_lens[k] - 1;
        out->blocks.push_back(b);
    }
}

}  // namespace mtbhost
#endif
