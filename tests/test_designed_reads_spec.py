"""The designed reads of tests/designed_reads.py on the CPU: every case sits on the edge it names (its precondition, asserted over the
oracle's matches and ReadScorer's paths, chains and combine trace), and on every case the three CPU formulations agree bit for bit --
the oracle (oracle/oracle.cpp), the chain enumeration of tests/bruteforce.py::ReadScorer, and the host build of the kernel arithmetic
(tests/emu: the sequential core and the data-parallel phases of mtb_score_par.h, matches presorted and in random order, chain DP by
pointer doubling and round by round).  Conditions, not measurements: no read is flagged ambiguous by the oracle and no read exceeds
ReadScorer's chain budget (TooManyChains would propagate out of the world's analysis)."""
import numpy as np
import pytest

import designed_reads as D
from helpers import tax_arrays


@pytest.fixture(scope="module")
def world(orc, tmp_path_factory):
    return D.DesignedWorld(orc, tmp_path_factory.mktemp("designed"))


@pytest.fixture(scope="module")
def taxarr(world, orc):
    return tax_arrays(orc, world.tax, world.world.tax)


CASE_NAMES = [c.__name__ for c in D.CASES]


def runs_of(world, name):
    c = world.case(name)
    return c, [(label, world.analysis(c, label)) for label, _ in c.runs]


def same_as_oracle(ref, res, tt, tc, tag):
    """all four fields and the taxID:count lists, no read masked"""
    ro = ref["results"]
    for f in ("classification", "is_classified", "n_taxcnt"):
        assert (res[f] == ro[f]).all(), (tag, f, np.flatnonzero(res[f] != ro[f])[:5])
    assert (res["score"].view(np.uint32) == ro["score"].view(np.uint32)).all(), (tag, "score")
    for i in range(len(ro)):
        a, b, n = int(res["taxcnt_off"][i]), int(ro["taxcnt_off"][i]), int(ro["n_taxcnt"][i])
        assert (tt[a:a + n] == ref["tc_tax"][b:b + n]).all() and (tc[a:a + n] == ref["tc_cnt"][b:b + n]).all(), (tag, i)


BY_RULE = {"ties (a17)": ["Ties", "TieSum", "TieRatio", "DisjointTies", "DisjointTiesLong", "DisjointTieRatio"], "thresholds": ["Thresholds"], "cap at 1.0": ["Cap"],
           "depth (a15)": ["Depth", "DepthLong"], "many paths": ["ManyPaths", "ManyPathsBig", "ManyPathsPaired", "ManyPathsLong"], "combination (a16)": ["Combine", "CombineLong"],
           "several matches per position": ["TwoPerPosition", "TwoPerPositionLong"], "redundancy filter and descent (a18)": ["Descent"], "N and nothing": ["NAndNothing"],
           "overflowing slot tails": ["Overflow"]}


def test_every_case_is_listed_under_its_rule():
    assert sorted(n for names in BY_RULE.values() for n in names) == sorted(CASE_NAMES)


@pytest.mark.parametrize("name", CASE_NAMES)
def test_precondition_holds_and_no_read_is_flagged(world, name):
    c, runs = runs_of(world, name)
    for label, a in runs:
        assert (a.ref["results"]["flag"] == 0).all(), (name, label, np.flatnonzero(a.ref["results"]["flag"]))
    c.precondition(world, dict(runs))


@pytest.mark.parametrize("name", CASE_NAMES)
def test_chain_enumeration_equals_the_oracle(world, name):
    c, runs = runs_of(world, name)
    for label, a in runs:
        ro = a.ref["results"]
        for i, r in enumerate(a.reads):
            e = ro[i]
            tag = (name, label, c.batch.names[i])
            assert r["cls"] == e["classification"] and r["is_cls"] == e["is_classified"], (tag, r["cls"], e["classification"])
            assert r["score"].view(np.uint32) == e["score"].view(np.uint32), (tag, r["score"], e["score"])
            x = int(e["taxcnt_off"]); y = x + int(e["n_taxcnt"])
            assert sorted(r["taxcnt"].items()) == list(zip(a.ref["tc_tax"][x:y].tolist(), a.ref["tc_cnt"][x:y].tolist())), tag


@pytest.mark.parametrize("name", CASE_NAMES)
def test_kernel_arithmetic_equals_the_oracle(world, taxarr, emu, name):
    c, runs = runs_of(world, name)
    for label, a in runs:
        ref, n = a.ref, c.batch.n
        m, ql, ql2 = ref["matches"], ref["qlen"], ref["qlen2"]
        same_as_oracle(ref, *emu.score(taxarr, a.p, m, n, ql, ql2), (name, label, "sequential"))
        same_as_oracle(ref, *emu.score_par(taxarr, a.p, m, n, ql, ql2, presorted=True), (name, label, "parallel, presorted"))
        rd = (m["qinfo"] >> np.uint64(32)) & np.uint64(0x1FFFFFFF)
        sh = m[np.lexsort((np.random.default_rng(D.SEED).random(len(m)), rd))]          # the order k_regroup leaves: by read only
        same_as_oracle(ref, *emu.score_par(taxarr, a.p, sh, n, ql, ql2, presorted=False), (name, label, "parallel, shuffled, chains"))
        same_as_oracle(ref, *emu.score_par(taxarr, a.p, sh, n, ql, ql2, presorted=False, use_chain=False), (name, label, "parallel, shuffled, rounds"))
