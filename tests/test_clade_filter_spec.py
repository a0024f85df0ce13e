"""tests/clade_filter_spec.py (the selection rule of mtb_merge_databases_filtered, restated) against values worked out by hand on the
three-genus toy tree of that module:

    1 root - 2 Bacteria - genus 10 { species 11 { 111, 112 }, species 12 }      merged.dmp: 900 -> 12, 901 -> 111
                        - genus 20 { species 21 { 211 }, species 22 }
                        - genus 30 { species 31 { 311 } }
"""
import numpy as np
import pytest

import clade_filter_spec as S

NODES = [1, 2, 10, 11, 12, 20, 21, 22, 30, 31, 111, 112, 211, 311]
ALIASES = [900, 901]


@pytest.fixture(scope="module")
def tree():
    return S.toy_tree()


def _kept(keep):
    """the ids (nodes, aliases, and 0 for the key of ids without a species) whose byte is set; every other byte must be clear"""
    on = set(int(i) for i in np.flatnonzero(keep))
    assert on <= set(NODES + ALIASES + [0])
    return on


def test_table_covers_zero_to_the_largest_id(tree):
    assert len(S.keep_table(*tree, [10], [])) == 902


def test_select_genus(tree):
    assert _kept(S.keep_table(*tree, [10], [])) == {10, 11, 12, 111, 112, 900, 901}


def test_exclude_a_species_inside_a_selected_genus(tree):
    assert _kept(S.keep_table(*tree, [10], [12])) == {10, 11, 111, 112, 901}


def test_exclude_genus_keeps_the_rest_and_key_0(tree):
    assert _kept(S.keep_table(*tree, [], [30])) == set(NODES + ALIASES + [0]) - {30, 31, 311}


def test_exclude_root_keeps_nothing(tree):
    assert _kept(S.keep_table(*tree, [], [1])) == set()


def test_select_root_keeps_every_node_but_not_key_0(tree):
    assert _kept(S.keep_table(*tree, [1], [])) == set(NODES + ALIASES)


def test_key_0(tree):
    assert S.keep_table(*tree, [], [12])[0] == 1           # no selection, root not excluded
    assert S.keep_table(*tree, [2], [])[0] == 0            # any selection
    assert S.keep_table(*tree, [], [1, 12])[0] == 0        # root excluded
    assert S.keep_table(*tree, [], [2])[0] == 1            # the superkingdom is not the root


def test_an_aliased_id_names_its_node(tree):
    assert (S.keep_table(*tree, [], [900]) == S.keep_table(*tree, [], [12])).all()
    assert _kept(S.keep_table(*tree, [900], [])) == {12, 900}


def test_several_ids_and_overlap(tree):
    assert _kept(S.keep_table(*tree, [11, 30], [])) == {11, 111, 112, 901, 30, 31, 311}
    assert _kept(S.keep_table(*tree, [10, 11], [10])) == set()              # an excluded ancestor wins


@pytest.mark.parametrize("ids,bad", [([111], 111), ([10, 112], 112), ([901], 901), ([211], 211), ([311], 311)])
def test_a_strain_is_refused(tree, ids, bad):
    for sel, exc in ((ids, []), ([], ids)):
        with pytest.raises(S.Refusal) as e:
            S.keep_table(*tree, sel, exc)
        assert (e.value.kind, e.value.taxid) == ("below_species", bad)


@pytest.mark.parametrize("bad", [777, 5000, 0, -3, 902])
def test_an_unknown_id_is_refused(tree, bad):
    with pytest.raises(S.Refusal) as e:
        S.keep_table(*tree, [10], [bad])
    assert (e.value.kind, e.value.taxid) == ("unknown", bad)


def test_no_ids_is_refused(tree):
    with pytest.raises(S.Refusal) as e:
        S.keep_table(*tree, [], [])
    assert e.value.kind == "no_ids"


def test_species_keys(tree):
    got = S.record_keys(*tree, [111, 112, 11, 12, 900, 901, 211, 311, 10, 2, 1, 0, 777])
    assert got.tolist() == [11, 11, 11, 12, 12, 11, 21, 31, 10, 2, 0, 0, 0]


def test_statistics(tree):
    ids = [111, 112, 12, 900, 21, 211, 1, 30]              # keys 11 11 12 12 21 21 0 30
    assert S.statistics(*tree, [], [20, 22], ids) == dict(n_records_in=8, n_records_kept=6, n_species_kept=4, n_species_dropped=1, n_unmatched=1, first_unmatched=22)
    assert S.statistics(*tree, [10], [], ids) == dict(n_records_in=8, n_records_kept=4, n_species_kept=2, n_species_dropped=3, n_unmatched=0, first_unmatched=0)
    assert S.statistics(*tree, [22, 31], [900], ids) == dict(n_records_in=8, n_records_kept=0, n_species_kept=0, n_species_dropped=5, n_unmatched=2, first_unmatched=22)
    assert S.statistics(*tree, [], [1], [1, 1])["n_unmatched"] == 0        # root-labelled records lie under the root
