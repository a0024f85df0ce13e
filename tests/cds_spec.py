"""CDS annotation -> sequence blocks, restated in Python from the description of the route (`mtb_build --cds-info`): the parser of the
annotation headers and the divider of a genome into CDS blocks, joined CDS and non-CDS blocks.  TEST INFRASTRUCTURE ONLY; it shares
no code with metabuli_amd/csrc/host/cds_info.h, which tests/test_cds_info.py compares it with.

Coordinates of a location are 1-based and inclusive; blocks are 0-based with an inclusive end (mtb_seq_block)."""
import re

import numpy as np

EXTEND = 11           # codons a CDS is extended by on either side while it stays inside the sequence
MIN_NONCDS = 32       # a region between CDS counts if it is longer than this

_COMP = {}
for _cls, _to in (("ARW", "T"), ("CMS", "G"), ("HTY", "A"), ("BDGKU", "C")):
    for _ch in _cls:
        _COMP[_ch] = _to; _COMP[_ch.lower()] = _to


class CdsError(Exception):
    pass


def accession_key(name):
    s = name.split("|", 1)[1] if "|" in name else name
    d = s.find(".")
    return (s if d < 0 else s[:d + 2]), (d >= 0 and len(s) > d + 2 and s[d + 2].isdigit())


def _coord(txt, name):
    txt = txt.strip().lstrip("<>").strip()
    if not txt.isdigit():
        raise CdsError(f"CDS record {name}: cannot read the coordinate '{txt}'")
    return int(txt)


def parse_location(value, name):
    """-> (complement, [(first, second), ...])"""
    comp = "complement(" in value
    for word in ("complement(", "join("):
        if word in value:
            value = value[value.index(word) + len(word):value.rindex(")")]
    locs = []
    for piece in value.split(","):
        if ".." in piece:
            a, b = piece.split("..", 1)
            locs.append([_coord(a, name), _coord(b, name)])
        else:
            locs.append([_coord(piece, name)] * 2)
    return comp, locs


def parse_annotation(headers):
    """headers: the header lines (without '>') of every annotation record, in file order -> (map accession -> list of CDS, stats);
    a CDS is dict(name, complement, loc)"""
    cds, st = {}, dict(records=0, cds=0, pseudo=0, hypothetical=0, orphan_location=0, no_location=0, two_digit_version=0)
    for h in headers:
        st["records"] += 1
        parts = re.split(r"[ \t]", h, maxsplit=1)
        name, comment = parts[0], (parts[1] if len(parts) > 1 else "")
        key, two = accession_key(name)
        st["two_digit_version"] += two
        frame, cur, done = 1, None, False
        for tag in re.findall(r"\[([^\]]*)\]", comment):
            feature, _, value = tag.partition("=")
            if feature == "pseudo":
                st["pseudo"] += 1; done = True; break
            if feature == "protein" and value == "hypothetical protein":
                st["hypothetical"] += 1; done = True; break
            if feature == "frame":
                frame = int(value)
            elif feature == "protein_id":
                cur = dict(name=name, complement=False, loc=[])
                cds.setdefault(key, []).append(cur)
            elif feature == "location":
                done = True
                if cur is None:
                    st["orphan_location"] += 1
                    break
                cur["complement"], cur["loc"] = parse_location(value, name)
                if frame != 1:
                    if cur["complement"]:
                        cur["loc"][-1][1] -= frame - 1
                    else:
                        cur["loc"][0][0] += frame - 1
                st["cds"] += 1
                break
        if not done:
            st["no_location"] += 1
            if cur is not None:
                cds[key].pop()
                if not cds[key]:
                    del cds[key]
    return cds, st


def divide(entries, accession, seq):
    """seq: the genome as a str -> (blocks [(strand, start, end)], joined [(str)], in the order: CDS in annotation order, then non-CDS)"""
    L = len(seq)
    for e in entries:
        for a, b in e["loc"]:
            if a < 1 or b < a or b > L:
                raise CdsError(f"CDS record {e['name']}: location {a}..{b} lies outside sequence {accession} of {L} bases")
    single, joined, non = [], [], []
    for e in entries:
        parts = []
        for j, (a, b) in enumerate(e["loc"]):
            begin, end = a - 1, b - 1
            if j == 0:
                k = 0
                while k < EXTEND and begin >= 3:
                    begin -= 3; k += 1
            if j == len(e["loc"]) - 1:
                k = 0
                while k < EXTEND and end + 3 < L:
                    end += 3; k += 1
            parts.append((begin, end))
        if len(parts) == 1:
            single.append((-1 if e["complement"] else 1, parts[0][0], parts[0][1]))
        elif len(parts) > 1:
            s = "".join(seq[a:b + 1] for a, b in parts)
            if e["complement"]:
                s = "".join(_COMP.get(c, "N") for c in reversed(s))
            joined.append(s)
    covered = np.zeros(L, bool)
    for e in entries:
        for a, b in e["loc"]:
            covered[a - 1:b] = True
    i = 0
    while i < L:
        run = 0
        while i < L and not covered[i]:
            i += 1; run += 1
        if run > MIN_NONCDS:
            non.append((1, i - run, i - 1))
        i += 1
    return single, joined, non


def dump(headers, genomes):
    """genomes: [(name, str)] -> the lines tests/emu/cds_dump.cpp prints"""
    cds, st = parse_annotation(headers)
    lines = ["stats " + " ".join(f"{k}={st[k]}" for k in ("records", "cds", "pseudo", "hypothetical", "orphan_location", "no_location", "two_digit_version")) +
             f" accessions={len(cds)}"]
    blocks, extras = [], []
    for i, (name, seq) in enumerate(genomes):
        lines.append(f"seq {i} {name} {'blocks' if name in cds else 'sixframes'}")
        if name in cds:
            single, joined, non = divide(cds[name], name, seq)
            # cds_info.h writes a genome's blocks in one list: single-location CDS in annotation order, then its non-CDS regions
            blocks += [(i, *b) for b in single] + [(i, *b) for b in non]
            extras += [(i, s) for s in joined]
    n = len(genomes)
    blocks += [(n + k, 1, 0, len(s) - 1) for k, (_, s) in enumerate(extras)]
    lines += [f"block {s} {st_} {a} {b}" for s, st_, a, b in blocks]
    lines += [f"extra {n + k} {o} {s}" for k, (o, s) in enumerate(extras)]
    return lines


def call_arrays(headers, genomes, taxids):
    """the arrays of ONE mtb_builder_add_blocks call over the annotated genomes, and the un-annotated ones for add_sequences ->
    dict(bases, offs, taxids, blocks) , dict(bases, offs, taxids)"""
    from blocks_spec import make_blocks
    cds, _ = parse_annotation(headers)
    seqs, tx, rows, extras, plain = [], [], [], [], []
    for (name, seq), t in zip(genomes, taxids):
        if name not in cds:
            plain.append((seq, t)); continue
        i = len(seqs)
        seqs.append(seq); tx.append(t)
        single, joined, non = divide(cds[name], name, seq)
        rows += [(i, *b) for b in single + non]
        extras += [(s, t) for s in joined]
    n = len(seqs)
    for k, (s, t) in enumerate(extras):
        seqs.append(s); tx.append(t); rows.append((n + k, 1, 0, len(s) - 1))

    def cat(ss):
        offs = np.zeros(len(ss) + 1, np.uint64); offs[1:] = np.cumsum([len(s) for s in ss])
        return np.frombuffer("".join(ss).encode(), np.uint8).copy(), offs
    b, o = cat(seqs)
    pb, po = cat([s for s, _ in plain])
    return dict(bases=b, offs=o, taxids=np.array(tx, np.int32), blocks=make_blocks(rows)), dict(bases=pb, offs=po, taxids=np.array([t for _, t in plain], np.int32))
