"""rt_host_update_vertices (include/rt_host.h): a prepared scene's vertices moved on its own
topology, on the host only -- no GPU, no HIP call.  The moved scenes are tests/update_cases.py's.

After HostScene.update_vertices(posB) on A:
  * vertex_pos is posB; vertex_normals equal, bit for bit, those of B loaded fresh through
    minirt.write_sce and the loader; face_normals[slot] equals fresh B's at the slot of the same
    triangle (through the two oracles' perm); the index and topology arrays are unchanged;
  * every reference box equals the exact union recomputed in numpy;
  * the device hierarchies built from the pair (rt_debug_tree_report: sbvh, sah, reference) are valid;
  * the raw scene moved too: an Oracle made afterwards renders fresh B's frame.
The inputs are not vacuous: the oracle's own counts for fresh B under A's camera have
closest_hits >= 0.25 x (primary + reflection rays) on the kept seeds."""
import numpy as np
import pytest

import pyoracle
import rtamd
import scale_scenes as ss
import update_cases as uc

TREES = ("sbvh", "sah", "reference")


def _check_boxes_and_trees(hs):
    lo, hi = uc.exact_boxes(hs)
    b = hs.bvh_arrays()
    assert np.array_equal(b["bb_min"], lo) and np.array_equal(b["bb_max"], hi)
    for tree in TREES:
        assert rtamd.tree_report(hs, tree=tree, build_threads=1).invalid == 0, tree


def test_kept_seeds_are_not_vacuous():
    kept = []
    for seed in uc.SEEDS:
        hits, rays = uc.hit_fraction(seed)
        print(f"seed {seed}: closest_hits {hits} of {rays} primary + reflection rays = {hits / rays:.3f}")
        if hits >= uc.MIN_HIT_FRACTION * rays:
            kept.append(seed)
    assert tuple(kept) == uc.KEPT and len(kept) >= 4


@pytest.mark.parametrize("seed", uc.KEPT)
def test_updated_fuzz_scene_equals_fresh_b(seed):
    hsA, orcA = uc.fuzz_a(seed)
    hsB, orcB = uc.fuzz_b(seed)
    before = uc.topology(hsA)
    posB = uc.pos_b(seed)
    assert not np.array_equal(posB, hsA.soa_arrays()["vertex_pos"])
    hsU = uc.updated(seed)
    got, fresh = hsU.soa_arrays(), hsB.soa_arrays()
    assert np.array_equal(got["vertex_pos"], posB)
    assert np.array_equal(got["vertex_normals"], fresh["vertex_normals"])
    permA, permB = orcA.bvh()["perm"], orcB.bvh()["perm"]
    slotB = np.argsort(permB)          # triangle -> fresh B's slot
    assert np.array_equal(got["face_normals"], fresh["face_normals"][slotB[permA]])
    assert not np.array_equal(got["face_normals"], hsA.soa_arrays()["face_normals"])
    after = uc.topology(hsU)
    for k, v in before.items():
        assert np.array_equal(after[k], v), k
    assert hsU.bvh.contents.n_nodes == hsA.bvh.contents.n_nodes
    _check_boxes_and_trees(hsU)


@pytest.mark.parametrize("seed", uc.KEPT[:2])
def test_raw_scene_moves_with_the_update(seed):
    hsB, orcB = uc.fuzz_b(seed)
    hsU = uc.updated(seed)
    p = hsU.render_params(0, 0, 1)
    want, cw = orcB.render(hsB.render_params(0, 0, 1), pyoracle.MODE_REFERENCE)
    got, cg = pyoracle.Oracle(hsU.raw, hsU).render(p, pyoracle.MODE_REFERENCE)
    assert np.array_equal(got, want) and ss.rays_counted(cg) == ss.rays_counted(cw)
    assert cg.closest_hits > 0


@pytest.mark.parametrize("name", uc.GENERATED)
def test_updated_generated_scene(name):
    hs = uc.generated(name)
    before = uc.topology(hs)
    old = {k: v.copy() for k, v in hs.soa_arrays().items()}
    posB = uc.generated_pos_b(hs)
    moved = np.any(posB != old["vertex_pos"], axis=1)
    assert moved.any() and not moved.all()
    hs.update_vertices(posB)
    got = hs.soa_arrays()
    assert np.array_equal(got["vertex_pos"], posB)
    # a translated mesh keeps its normals up to rounding; an unmoved one keeps them bit for bit
    assert np.array_equal(got["vertex_normals"][~moved], old["vertex_normals"][~moved])
    assert np.abs(got["vertex_normals"] - old["vertex_normals"]).max() < 1e-9
    assert np.abs(got["face_normals"] - old["face_normals"]).max() < 1e-9
    for k, v in before.items():
        assert np.array_equal(uc.topology(hs)[k], v), k
    _check_boxes_and_trees(hs)
    # and back: the prepared scene's own arrays, bit for bit
    hs.update_vertices(old["vertex_pos"])
    again = hs.soa_arrays()
    for k in ("vertex_pos", "vertex_normals", "face_normals"):
        assert np.array_equal(again[k], old[k]), k


def test_errors():
    hs = rtamd.HostScene.generate("cornell")
    P = np.zeros((4, 3))
    with pytest.raises(rtamd.RtError, match="not prepared"):
        hs.update_vertices(P)
    hs.prepare()
    n = hs.soa.contents.n_vertices
    with pytest.raises(rtamd.RtError, match="n_vertices"):
        hs.update_vertices(np.zeros((n + 1, 3)))
    with pytest.raises(ValueError):
        hs.update_vertices(np.zeros((n, 2)))
    hs.update_vertices(hs.soa_arrays()["vertex_pos"].copy())   # the identity is accepted
