"""The host side of the re-clipping update without a GPU: the clip regions the
builder records (rt_debug_clip_regions), their cover invariant, and rt_reclip.hpp's box
(rt_reclip_box_host, the device's function text) against a numpy fp64 Sutherland-Hodgman clip.

About "empty exactly when no vertex and no edge crossing lies in the region": with `candidates` =
the three vertices and the crossing points of the edges with the region's finite planes,
  * a candidate in the region => the box is non-empty, for every region (asserted for all cases);
  * no candidate in the region => the box is empty: a theorem only where the region cannot be
    pierced by the triangle's interior and the plane-by-plane intersection is exact in emptiness,
    i.e. at most three finite planes on at most two axes (a region bounded on two axes, four planes
    and more, can sit wholly inside a large triangle: triangle and region intersect, the box is
    rightly non-empty, and no candidate lies in the region).  Asserted for those cases; for the rest
    the box must still contain the numpy clip, which covers every case where the two intersect."""
import numpy as np
import pytest

import reclip_cases as rcs
import rtamd

N_POINTS = 1000
N_BOXES = 10000


# ---- the builder's regions ----
@pytest.mark.parametrize("oset", sorted(rcs.OPTION_SETS))
@pytest.mark.parametrize("scene", rcs.CUT_SEEDS + (rcs.PLAIN_SEED, "cornell"))
def test_regions_match_the_tree_report(scene, oset):
    hs = rcs.host_a(scene)
    clip, slot = rcs.regions(scene, oset)
    rep = rtamd.tree_report(hs, **rcs.options(scene, oset))
    assert len(clip) == len(slot) == rep.records == rcs.RECORDS[scene][oset == "split"]
    nt = hs.triangle_count
    assert nt == rcs.TRIANGLES[scene]
    assert slot.min() >= 0 and slot.max() < nt and len(np.unique(slot)) == nt   # valid, and every slot occurs
    assert not np.isnan(clip).any() and np.all(clip[:, :3] <= clip[:, 3:])
    assert np.all(clip[:, :3] < np.inf) and np.all(clip[:, 3:] > -np.inf)
    if (scene, oset) in rcs.UNCUT_FUZZ:
        assert len(clip) == nt and not np.isfinite(clip).any()
    else:
        rcs.assert_cut(scene, oset)
        # a triangle with one record was never cut
        once = np.bincount(slot, minlength=nt)[slot] == 1
        assert not np.isfinite(clip[once]).any()


@pytest.mark.parametrize("tree", ["sah", "reference"])
def test_trees_without_spatial_splits_have_infinite_regions(tree):
    for scene in (rcs.CUT_SEEDS[0], "cornell"):
        hs = rcs.host_a(scene)
        clip, slot = rtamd.clip_regions(hs, tree=tree)
        assert len(clip) == hs.triangle_count and np.array_equal(np.sort(slot), np.arange(len(slot)))
        assert np.all(clip[:, :3] == -np.inf) and np.all(clip[:, 3:] == np.inf)


def _cover_points(hs, clip, rng):
    """N_POINTS points in twice the root box, 300 of them with one to three coordinates placed
    exactly on recorded plane positions."""
    P = hs.soa_arrays()["vertex_pos"]
    lo, hi = P.min(axis=0), P.max(axis=0)
    mid, half = 0.5 * (lo + hi), hi - lo   # twice the box: half-extent = the whole extent
    pts = mid + half * rng.uniform(-1.0, 1.0, size=(N_POINTS, 3))
    planes = [np.concatenate([clip[:, k], clip[:, 3 + k]]) for k in range(3)]
    planes = [p[np.isfinite(p)] for p in planes]
    cut_axes = [k for k in range(3) if len(planes[k])]
    for i in range(300):
        for k in rng.choice(cut_axes, size=int(rng.integers(1, len(cut_axes) + 1)), replace=False):
            pts[i, k] = planes[k][rng.integers(len(planes[k]))]
    return pts


@pytest.mark.parametrize("scene,oset", list(rcs.CUT_FUZZ) + [("cornell", "default")])
def test_regions_of_every_triangle_cover_space(scene, oset):
    clip, slot = rcs.assert_cut(scene, oset)
    hs = rcs.host_a(scene)
    pts = _cover_points(hs, clip, np.random.default_rng(7))
    nt = hs.triangle_count
    covered = np.zeros((nt, N_POINTS), dtype=bool)
    for g in range(len(clip)):
        covered[slot[g]] |= np.all((pts >= clip[g, :3]) & (pts <= clip[g, 3:]), axis=1)
    assert covered.all(), f"{(~covered).sum()} (triangle, point) pairs lie in no record's region"
    on_plane = sum(int(np.isin(pts[:300, k], np.concatenate([clip[:, k], clip[:, 3 + k]])).sum()) for k in range(3))
    assert on_plane >= 300


# ---- the box ----
def _random_case(rng):
    scale = 2.0 ** rng.integers(-12, 13)
    centre = scale * rng.uniform(-4.0, 4.0, size=3)
    tri = centre + scale * rng.uniform(-1.0, 1.0, size=(3, 3))
    clip = np.array([-np.inf] * 3 + [np.inf] * 3)
    n_planes = int(rng.integers(0, 7))
    for j in rng.choice(6, size=n_planes, replace=False):
        k = j % 3
        if rng.uniform() < 0.1:
            clip[j] = tri[rng.integers(3), k]   # a plane exactly through a vertex
        else:
            clip[j] = centre[k] + scale * rng.uniform(-1.3, 1.3)
    for k in range(3):
        if clip[k] > clip[3 + k]:
            clip[k], clip[3 + k] = clip[3 + k], clip[k]
    return tri, clip, n_planes


def test_reclip_box_against_numpy_clip():
    rng = np.random.default_rng(11)
    seen = {"empty": 0, "nonempty": 0, "exact_rule": 0, "one_plane": 0, "pierced": 0}
    by_planes = np.zeros(7, dtype=int)
    for _ in range(N_BOXES):
        tri, clip, n_planes = _random_case(rng)
        by_planes[n_planes] += 1
        eps = 2.0 ** -40 * max(np.abs(tri).max(), np.abs(clip[np.isfinite(clip)]).max() if n_planes else 0.0)
        box = rtamd.reclip_box_host(tri[0], tri[1], tri[2], clip)
        poly = rcs.sh_clip(tri, clip)
        cand = any(rcs.in_region(p, clip) for p in rcs.candidates(tri, clip))
        axes = {j % 3 for j in range(6) if np.isfinite(clip[j])}
        if cand:
            assert box is not None, (tri, clip)
        elif n_planes <= 3 and len(axes) <= 2:
            assert box is None, (tri, clip)
            seen["exact_rule"] += 1
        elif box is not None and poly:
            seen["pierced"] += 1
        if poly:   # triangle and region intersect: the box contains the clipped polygon
            assert box is not None, (tri, clip)
            Q = np.array(poly)
            assert np.all(Q.min(axis=0) >= box[0] - eps) and np.all(Q.max(axis=0) <= box[1] + eps), (tri, clip)
        if box is None:
            seen["empty"] += 1
            continue
        seen["nonempty"] += 1
        lo, hi = box
        assert np.all(lo <= hi)
        assert np.all(lo >= np.maximum(tri.min(axis=0), clip[:3])) and np.all(hi <= np.minimum(tri.max(axis=0), clip[3:]))
        if n_planes == 1:
            Q = np.array(poly)
            assert np.all(np.abs(Q.min(axis=0) - lo) <= eps) and np.all(np.abs(Q.max(axis=0) - hi) <= eps), (tri, clip)
            seen["one_plane"] += 1
        if n_planes == 0:
            assert np.array_equal(lo, tri.min(axis=0)) and np.array_equal(hi, tri.max(axis=0))
    print(seen, by_planes)
    assert by_planes.min() >= N_BOXES // 14
    assert min(seen["empty"], seen["nonempty"]) >= N_BOXES // 10
    assert seen["exact_rule"] >= 200 and seen["one_plane"] >= 500 and seen["pierced"] >= 1


def test_reclip_box_edge_cases():
    inf = np.inf
    tri = np.array([[0.0, 0.0, 0.0], [4.0, 0.0, 0.0], [0.0, 4.0, 2.0]])
    lo, hi = rtamd.reclip_box_host(*tri, [-inf] * 3 + [inf] * 3)
    assert np.array_equal(lo, [0, 0, 0]) and np.array_equal(hi, [4, 4, 2])
    lo, hi = rtamd.reclip_box_host(*tri, [-inf, -inf, -inf, 2.0, inf, inf])   # x <= 2: crossings (2, 0, 0), (2, 2, 1)
    assert np.array_equal(lo, [0, 0, 0]) and np.array_equal(hi, [2, 4, 2])
    lo, hi = rtamd.reclip_box_host(*tri, [2.0, -inf, -inf, inf, inf, inf])    # x >= 2
    assert np.array_equal(lo, [2, 0, 0]) and np.array_equal(hi, [4, 2, 1])
    assert rtamd.reclip_box_host(*tri, [5.0, -inf, -inf, inf, inf, inf]) is None
    assert rtamd.reclip_box_host(*tri, [-inf, -inf, -inf, -1.0, inf, inf]) is None
    lo, hi = rtamd.reclip_box_host(*tri, [4.0, -inf, -inf, inf, inf, inf])    # touches the plane in one vertex
    assert np.array_equal(lo, [4, 0, 0]) and np.array_equal(hi, [4, 0, 0])
    # the triangle left the region altogether
    assert rtamd.reclip_box_host(*(tri + 100.0), [-inf, -inf, -inf, 2.0, 2.0, inf]) is None
    # a region inside a large triangle: pierced, no vertex and no crossing inside, rightly non-empty
    big = np.array([[-100.0, -100.0, 0.0], [100.0, -100.0, 0.0], [0.0, 100.0, 0.0]])
    lo, hi = rtamd.reclip_box_host(*big, [-1.0, -1.0, -1.0, 1.0, 1.0, 1.0])
    assert np.array_equal(lo, [-1, -1, 0]) and np.array_equal(hi, [1, 1, 0])
    with pytest.raises(ValueError):
        rtamd.reclip_box_host([0, 0], [0, 0, 0], [0, 0, 0], [0] * 6)
