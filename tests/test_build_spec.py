"""The yardstick of tests/test_gpu_build.py, pinned on the CPU: build_spec.spec_finish -- an independent numpy restatement of
mtb_builder_finish (sort by (value, species, taxid), one entry per (value, species), info = LCA of the group) -- agrees with
synth.dedup_targets, the host path every toy database has been built with so far."""
import numpy as np
import pytest

from build_spec import DumpTaxonomy, spec_finish
from metabuli_amd import synth


def _records(world, per):
    vals = np.concatenate(per)
    tids = np.concatenate([np.full(len(v), tid, np.int32) for (tid, _), v in zip(world.genomes, per)])
    return vals, tids


@pytest.mark.parametrize("seed,shape", [(1, (3, 2, 2)), (2, (2, 3, 4)), (3, (4, 1, 3))])
def test_spec_equals_dedup_targets(tmp_path, seed, shape):
    world = synth.make_world(seed=seed, n_genera=shape[0], species_per_genus=shape[1], strains_per_species=shape[2], genome_len=300)
    world.tax.write(str(tmp_path))
    rng = np.random.default_rng(seed)
    pool = rng.integers(0, 1 << 62, size=400, dtype=np.uint64)           # a small pool: values shared inside and across species
    per = [rng.choice(pool, size=int(rng.integers(50, 300))) for _ in world.genomes]   # duplicates inside a genome included
    ref_v, ref_t = synth.dedup_targets(world, per)
    v, info, _ = spec_finish(*_records(world, per), str(tmp_path))
    assert (v == ref_v).all() and (info == ref_t.astype(np.uint32)).all()
    multi = np.flatnonzero(np.isin(info, world.species))
    assert len(multi) > 0, "the case must contain groups whose LCA is a species"


def test_spec_is_order_independent_and_resolves_aliases(tmp_path):
    world = synth.make_world(seed=5, n_genera=2, species_per_genus=2, strains_per_species=3, genome_len=300)
    world.tax.write(str(tmp_path))
    strain = world.genomes[0][0]
    with open(tmp_path / "merged.dmp", "w") as f:
        f.write(f"9000\t|\t{strain}\t|\n")
    tax = DumpTaxonomy(str(tmp_path))
    assert tax.canon(9000) == strain and tax.species(9000) == world.tax.species_of(strain)
    rng = np.random.default_rng(0)
    vals = rng.integers(0, 50, size=600).astype(np.uint64)
    tids = rng.choice(np.array([g[0] for g in world.genomes] + [9000], np.int32), size=600)
    v0, i0, _ = spec_finish(vals, tids, str(tmp_path))
    perm = rng.permutation(600)
    v1, i1, _ = spec_finish(vals[perm], tids[perm], str(tmp_path))
    assert (v0 == v1).all() and (i0 == i1).all()
    assert 9000 not in i0                                                 # info holds nodes, never an alias id
    # a group of one alias record yields its target
    v2, i2, _ = spec_finish(np.array([7], np.uint64), np.array([9000], np.int32), str(tmp_path))
    assert i2.tolist() == [strain]
