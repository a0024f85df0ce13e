"""k_score_many (kernels_score_many.h) at the edges of its register-resident loads, its staging, its species table and its claim blocks,
against the oracle: reads whose tails overflow are deferred, listed, and scored by one wavefront each from their slots and their grouped
overflow entries after the matches of species without two matches in one frame are dropped.

Forged worlds (as tests/test_gpu_long_slots.py): a two-genus world, error-free reads cut from genome 0, and chosen metamers of a read filed
once more, unchanged, under new species of genus 0.  An exact copy is always selected and stands behind the genome's own entry, so k
copies add exactly k matches beyond the first of their metamers -- k tail / overflow entries.  A new species with one copy is dead
(dropped before the staging); a `rival` species with many copies has two in some frame and survives with all of them.

`many_plan` mirrors the kernel's hand-on rules from the oracle's matches alone (tail overflow -> deferred; more than 3 x CAP tail +
overflow entries, a species table beyond 3/4 of 1024, survivors beyond the staging -> handed to the next tier), and every case asserts
n_deferred_reads, n_many_reads, n_many_matches and n_many_kept against it (`assert_stats`); every row is compared bit for bit with the oracle."""
import os

import numpy as np
import pytest

from test_gpu_scorer_tiers import K_SCORE_MANY, Reads, metamers_per_read, slot_plan

pytestmark = pytest.mark.gpu

MANY_HASH = 1024                                         # kernels_score_many.h MTB_MANY_HASH
WORLD_SEED, GENUS0 = 91, 4                               # synth.make_world: root 1, Bacteria 2, Eukaryota 3, the first genus 4
OVF = (1, 63, 64, 65, 127, 128, 129)                    # grouped overflow entries: one; around the one and two register rounds of 64
LIST_LENGTHS = (1, 15, 16, 17, 33)                      # deferred reads: around the claim block of 16 and its partial last block


def _p():
    from helpers import default_params
    return default_params(seq_mode=1, syncmer=1)


def _world():
    from metabuli_amd import synth
    return synth.make_world(seed=WORLD_SEED, n_genera=2, species_per_genus=2, strains_per_species=1, genome_len=20000, with_euk=False)


def cut(start, length):
    return _world().genomes[0][1][start:start + length].copy()


def as_reads(seqs):
    offs = np.zeros(len(seqs) + 1, np.uint64)
    offs[1:] = np.cumsum([len(s) for s in seqs])
    return Reads(np.concatenate(seqs), offs)


def per_read(ref, n_reads):
    """per read of an oracle answer: all matches, those beyond the first of their metamer (`cur`), distinct species, survivors of the
    dead-species drop (matches of species with two matches in one frame)"""
    m = ref["matches"]
    rd = (((m["qinfo"] >> np.uint64(32)) & np.uint64(0x1FFFFFFF)).astype(np.int64)) - 1
    out = []
    for r in range(n_reads):
        q = m[rd == r]
        sp, fr = q["species_id"].astype(np.int64), (q["qinfo"] >> np.uint64(61)).astype(np.int64)
        pairs, cnt = np.unique(sp * 8 + fr, return_counts=True)
        alive = np.unique(pairs[cnt >= 2] // 8)
        out.append(dict(n=len(q), cur=len(q) - len(np.unique(q["qinfo"])), species=len(np.unique(sp)), kept=int(np.isin(sp, alive).sum())))
    return out


def many_plan(ref, n_reads):
    """-> (slot plan, per-read facts, counts): the reads k_score<SLOT> / k_score_fast defer for their tails, and of those the ones
    k_score_many scores, with the matches it sees and keeps"""
    counts = metamers_per_read(ref["kmers"], n_reads)
    qlt = (ref["results"]["qlen"] + ref["results"]["qlen2"]).astype(np.int64)
    p = slot_plan(counts, qlt, False)
    assert p["slot"] and not p["route_off"] and p["stride"] <= 384, p
    cap = 192 if p["stride"] <= 192 else 320
    tail_cap = p["stride"] - p["direct"]
    facts = per_read(ref, n_reads)
    n = dict(deferred=0, many=0, matches=0, kept=0, why_tail=0, why_table=0, why_staging=0)
    for f in facts:
        f["ovf"] = max(0, f["cur"] - tail_cap)
        if f["cur"] <= tail_cap:
            continue
        n["deferred"] += 1
        if f["cur"] > 3 * cap:
            n["why_tail"] += 1
        elif f["species"] > MANY_HASH // 4 * 3:
            n["why_table"] += 1
        elif f["kept"] > cap:
            n["why_staging"] += 1
        else:
            n["many"] += 1; n["matches"] += f["n"]; n["kept"] += f["kept"]
    return p, cap, tail_cap, facts, n


class Forge:
    """the world with forged entries; `base` = the oracle on the unforged world (what a read brings before anything is filed)"""

    def __init__(self, orc, dbdir, forged=None):
        from helpers import build_toy_db
        self.orc, self.dbdir, self.world = orc, str(dbdir), _world()
        os.makedirs(self.dbdir, exist_ok=True)
        extra = None
        if forged is not None:
            fv, ft = forged
            for s in np.unique(ft):
                self.world.tax.add(int(s), GENUS0, "species", f"forged{int(s)}")
            extra = (np.asarray(fv, np.uint64), np.asarray(ft, np.int32))
        self.values, self.taxids = build_toy_db(orc, self.world, _p(), self.dbdir, extra=extra)
        self.tax = orc.load_taxonomy(os.path.join(self.dbdir, "taxonomy"))
        self.db = orc.open_db(self.dbdir, self.tax, _p())

    def classify(self, r):
        return self.orc.classify(self.db, self.tax, _p(), r.b1, r.o1)


def single_values(orc, seq):
    """the metamer values that occur exactly once in the read: a copy of one under a new species adds exactly one match"""
    k, _, _ = orc.extract_batch(_p(), seq, np.array([0, len(seq)], np.uint64))
    v, c = np.unique(k["value"], return_counts=True)
    return v[c == 1]


def copies(values, n, species):
    """n distinct (value, species) entries: values in turn, species in turn (shifted by one on every further lap over the values)"""
    j = np.arange(n, dtype=np.int64)
    v, s = j % len(values), (j + j // len(values)) % len(species)
    assert n >= 0 and len(np.unique(v * len(species) + s)) == n, (n, len(values), len(species))
    return np.asarray(values)[v], np.asarray(species, np.int32)[s]


@pytest.fixture(scope="module")
def base(orc, tmp_path_factory):
    return Forge(orc, tmp_path_factory.mktemp("many_base"))


@pytest.fixture(scope="module")
def ctx():
    import metabuli_amd as M
    c = M.Context(0)
    c.set_profiling(True)
    yield c
    c.close()


def run(ctx, w, r, ref, tag):
    import metabuli_amd as M
    from test_gpu_designed_reads import same_as_oracle
    p = M.default_params(seq_mode=1, syncmer=1)
    ix = ctx.open_index(w.dbdir, p)
    try:
        res, tt, tc = ctx.classify_batch(ix, p, r.b1, r.o1)
        st = ctx.last_stats()
    finally:
        ix.close()
    assert (ref["results"]["flag"] == 0).all(), tag                   # nothing masked
    same_as_oracle(ref, res, tt, tc, tag)
    assert st.n_matches == len(ref["matches"]) and st.n_slot_reads == r.n, tag
    return st


def assert_stats(st, n, tag):
    """n_many_matches / n_many_kept are k_score_many's own (the matches it saw and staged: they pin WHICH reads it scored);
    n_many_reads counts the reads of either deferred tier -- what k_score_many hands on here is within k_many_sort's budgets"""
    got = dict(deferred=st.n_deferred_reads, tiers=st.n_many_reads, matches=st.n_many_matches, kept=st.n_many_kept)
    assert got == dict(deferred=n["deferred"], tiers=n["deferred"], matches=n["matches"], kept=n["kept"]), (tag, got, n)
    assert st.n_launch[K_SCORE_MANY] == (1 if n["deferred"] else 0), tag


def forged_batch(orc, base, tmpdir, length, starts, want):
    """reads of `length` bases cut at `starts`; want(i, facts of read i in the unforged world, tail_cap, first free species id, its single
    values) -> the (values, species) entries to file for read i.  -> (world, reads)"""
    seqs = [cut(s, length) for s in starts]
    r = as_reads(seqs)
    _, _, tail_cap, facts, _ = many_plan(base.classify(r), r.n)
    free = max(_world().tax.parent) + 1
    parts = [want(i, facts[i], tail_cap, free, single_values(orc, seqs[i])) for i in range(r.n)]
    parts = [p for p in parts if p is not None]
    forged = (np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]))
    return Forge(orc, tmpdir, forged), r


@pytest.fixture(scope="module")
def le192(orc, base, tmp_path_factory):
    """stride <= 192 (k_score_many<.., 192>, slots and the first 128 overflow entries in registers): per overflow count of OVF a read with
    that many grouped overflow entries, all of dead species; two reads whose survivors are CAP and CAP + 1 (a rival species with the
    copies); three plain reads"""
    cap = 192

    def want(i, f, tail_cap, free, singles):
        if i < len(OVF):
            return copies(singles, tail_cap + OVF[i] - f["cur"], free + np.arange(200))
        if i < len(OVF) + 2:                                  # the read's own matches survive; the rival's copies fill the staging
            return copies(singles, cap + (i - len(OVF)) - f["kept"], [free + 200])
        return None
    return forged_batch(orc, base, tmp_path_factory.mktemp("many_le192"), 150, [1000 + 400 * i for i in range(len(OVF) + 2 + 3)], want)


def test_overflow_rounds_and_staging_edge(ctx, le192):
    w, r = le192
    ref = w.classify(r)
    p, cap, tail_cap, facts, n = many_plan(ref, r.n)
    assert cap == 192 and p["stride"] <= 192, p
    assert [f["ovf"] for f in facts[:len(OVF)]] == list(OVF), [f["ovf"] for f in facts]
    assert all(f["kept"] <= cap for f in facts[:len(OVF)])
    assert [f["kept"] for f in facts[len(OVF):len(OVF) + 2]] == [cap, cap + 1] and all(f["ovf"] > 0 for f in facts[len(OVF):len(OVF) + 2]), facts[len(OVF):]
    assert all(f["ovf"] == 0 for f in facts[len(OVF) + 2:])
    assert (n["deferred"], n["many"], n["why_staging"]) == (len(OVF) + 2, len(OVF) + 1, 1), n
    assert_stats(run(ctx, w, r, ref, "le192"), n, ("le192", facts))


@pytest.mark.parametrize("n_list", LIST_LENGTHS)
def test_deferred_list_lengths_around_the_claim_block(ctx, le192, n_list):
    """n_list deferred reads (the overflow reads of the batch above, in turn) between plain ones: whole and partial claim blocks"""
    w, r = le192
    pick = [len(OVF) + 2] + [i % len(OVF) for i in range(n_list)] + [len(OVF) + 3, len(OVF) + 4]
    rr = as_reads([r.b1[int(r.o1[i]):int(r.o1[i + 1])] for i in pick])
    ref = w.classify(rr)
    p, cap, tail_cap, facts, n = many_plan(ref, rr.n)
    assert cap == 192 and (n["deferred"], n["many"]) == (n_list, n_list), n
    assert_stats(run(ctx, w, rr, ref, ("list", n_list)), n, ("list", n_list))


@pytest.fixture(scope="module")
def gt192(orc, base, tmp_path_factory):
    """stride > 192 (k_score_many<.., 320>, the loops): distinct species just under, at and over 3/4 of the table -- one copy under each
    of so many new species -- and an overflow read of the ordinary kind; two plain reads"""
    limit = MANY_HASH // 4 * 3

    def want(i, f, tail_cap, free, singles):
        if i < 3:
            return copies(singles, limit - 1 + i - f["species"], free + np.arange(limit + 16))
        if i == 3:
            return copies(singles, tail_cap + 70 - f["cur"], free + np.arange(200))
        return None
    return forged_batch(orc, base, tmp_path_factory.mktemp("many_gt192"), 240, [1000 + 500 * i for i in range(6)], want)


def test_species_table_at_three_quarters_and_the_320_staging(ctx, gt192):
    w, r = gt192
    ref = w.classify(r)
    p, cap, tail_cap, facts, n = many_plan(ref, r.n)
    limit = MANY_HASH // 4 * 3
    assert cap == 320 and p["stride"] > 192, p
    assert [f["species"] for f in facts[:3]] == [limit - 1, limit, limit + 1] and all(tail_cap < f["cur"] <= 3 * cap for f in facts[:3]), facts[:3]
    assert facts[3]["ovf"] == 70 and all(f["ovf"] == 0 for f in facts[4:])
    assert (n["deferred"], n["many"], n["why_table"]) == (4, 3, 1), n
    assert_stats(run(ctx, w, r, ref, "gt192"), n, ("gt192", facts))
