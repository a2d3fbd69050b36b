"""rt_scene_update_vertices_ex with RT_UPDATE_RECLIP on the device (include/rt_hip.h):
the leaf boxes of an RT_TREE_SBVH scene re-clipped to the regions its spatial splits cut the records
to.  The scenes and option sets are tests/reclip_cases.py's; tests/test_reclip_host.py holds the
regions' cover invariant and the box arithmetic.

  1. against a fresh upload of the moved scene: frames, ray counts and query rows with ==;
  2. against the oracle on B = 2^10 A and 2^-10 A, fp64 frames within 1e-12 and exact ray counts,
     with leaf slots emptied (every triangle leaves most of its regions);
  3. against the plain refit of the same upload: every box inside, some strictly smaller;
  4. against the builder: after A -> A and A -> B -> A every bound within one fp32 step of the upload's;
  5. against brute force over all triangles: t with ==;
  6. edges: the flag on scenes without a table, plain and re-clipping updates queued on one stream,
     a reserve_cus scene, device bytes."""
import numpy as np
import pytest

import query_cases as qc
import radiance_cases as rc
import reclip_cases as rcs
import rtamd
import scale_scenes as ss
import update_cases as uc

pytestmark = pytest.mark.gpu

TOL64 = 1e-12
GW, GH = 160, 90          # frames of the generated scenes
OSETS = sorted(rcs.OPTION_SETS)
K_EMPTY = 0x7fffffff
K_LEAF = 0x80000000


@pytest.fixture(autouse=True)
def _gpu(gpu_available):
    return gpu_available


def _params(hs, w=0, h=0, spp=1, flags=0):
    p = hs.render_params(w, h, spp)
    p.out_format = rtamd.RT_OUT_RGB_F64
    p.flags = flags
    return p


def _rays(hs):
    P = hs.soa_arrays()["vertex_pos"]
    return np.concatenate([qc.random_rays(hs, 512), qc.vertex_rays(hs, P, 512)])


def _same_hits(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("t", "alpha", "beta", "normal", "slot", "mesh", "prim"))


def _check_against_fresh(dev, hs, p, **options):
    """The updated device scene against a fresh upload of the (updated) host scene: frame, ray counts
    and the rows of both queries, all with ==.  Returns the frame."""
    fresh = rtamd.DeviceScene(hs, 0, **options)
    img, st = dev.render(p)
    want, wst = fresh.render(p)
    assert np.array_equal(img, want)
    assert rc.counts(st) == rc.counts(wst) and st.pixels == wst.pixels
    rays = _rays(hs)
    got, qs = dev.trace(rays, stats=True)
    ref, rs = fresh.trace(rays, stats=True)
    assert _same_hits(got, ref) and qs.hits == rs.hits and qs.watchdog == 0
    assert np.array_equal(dev.trace(rays, occluded=True), fresh.trace(rays, occluded=True))
    assert rs.hits >= 64
    lo, hi = dev.bounds()
    flo, fhi = fresh.bounds()
    assert np.array_equal(lo, flo) and np.array_equal(hi, fhi)
    fresh.close()
    return img


def _boxes(n4):
    """(lo [n, 3, 4], hi [n, 3, 4] float32, refs [n, 4]) of a nodes4 image."""
    f = n4[:, :24].view(np.float32).reshape(len(n4), 3, 2, 4)
    return f[:, :, 0, :], f[:, :, 1, :], n4[:, 24:28]


def _leaf_slots(refs):
    return (refs != K_EMPTY) & ((refs & K_LEAF) != 0)


def _emptied(n4):
    """Leaf slots with a ref that hold the empty box [+inf, -inf] on every axis."""
    lo, hi, refs = _boxes(n4)
    return int((_leaf_slots(refs) & np.all(lo == np.inf, axis=1) & np.all(hi == -np.inf, axis=1)).sum())


def _steps_apart(a, b):
    """Bounds of float32 arrays a, b that are more than one fp32 step apart."""
    up, down = np.nextafter(a, np.float32(np.inf)), np.nextafter(a, np.float32(-np.inf))
    return int((~((a == b) | (up == b) | (down == b))).sum())


# ---- 1. against a fresh upload ----
@pytest.mark.parametrize("oset", OSETS)
@pytest.mark.parametrize("seed", uc.KEPT)
def test_reclipped_fuzz_scene_equals_fresh_upload(seed, oset):
    options = rcs.options(seed, oset)
    if (seed, oset) in rcs.CUT_FUZZ:
        rcs.assert_cut(seed, oset)
    hsA, hsU = rcs.host_a(seed), rcs.moved(seed)
    dev = rtamd.DeviceScene(hsA, 0, **options)
    before, _ = dev.render(_params(hsA))
    dev.update(hsU, reclip=True)
    spp = 4 if (seed, oset) == (1, "default") else 1
    img = _check_against_fresh(dev, hsU, _params(hsU, spp=spp), **options)
    assert len(np.unique(img.reshape(-1, 3), axis=0)) > 2
    if spp == 1:
        assert not np.array_equal(img, before)   # the scene did move in the view
    dev.close()


@pytest.mark.parametrize("name", uc.GENERATED)
def test_reclipped_generated_scene_equals_fresh_upload(name):
    rcs.assert_cut(name, "default")
    hs = uc.generated(name)
    dev = rtamd.DeviceScene(hs, 0)
    p = _params(hs, GW, GH)
    before, _ = dev.render(p)
    hs.update_vertices(uc.generated_pos_b(hs))
    dev.update(hs, reclip=True)
    img = _check_against_fresh(dev, hs, p)
    assert not np.array_equal(img, before)
    dev.close()


def test_reclipped_fans_and_camera_points_equal_fresh_upload():
    seed, oset = 1, "split"
    rcs.assert_cut(seed, oset)
    options = rcs.options(seed, oset)
    hsA, hsU = rcs.host_a(seed), rcs.moved(seed)
    dev = rtamd.DeviceScene(hsA, 0, **options)
    dev.update(hsU, reclip=True)
    fresh = rtamd.DeviceScene(hsU, 0, **options)
    p = _params(hsU)
    a, b = dev.camera(p, hits=True, points=True), fresh.camera(p, hits=True, points=True)
    pts = b["points"].cpu().numpy()
    assert _same_hits({k: v.cpu().numpy() for k, v in a["hits"].items()},
                      {k: v.cpu().numpy() for k, v in b["hits"].items()})
    assert np.array_equal(a["points"].cpu().numpy(), pts, equal_nan=True)
    assert np.isfinite(b["hits"]["t"].cpu().numpy()).sum() >= uc.MIN_HIT_FRACTION * uc.W * uc.H
    lo, hi = fresh.bounds()
    pts[:, 6] = 0.5 * float(np.sqrt(((hi - lo) ** 2).sum()))
    dirs = rtamd.ao_directions(8, 5, seed=1)
    want = fresh.ao(pts, dirs, seed=3, bias=1e-6)
    assert np.array_equal(dev.ao(pts, dirs, seed=3, bias=1e-6), want)
    assert np.any((want > 0) & (want < 8))
    pg = rc.params(hsU, 8, 8)
    gw, gst = fresh.gather(pts, dirs, pg, seed=3, bias=1e-6, stats=True)
    gg, st = dev.gather(pts, dirs, pg, seed=3, bias=1e-6, stats=True)
    assert np.array_equal(gg, gw) and rc.counts(st) == rc.counts(gst)
    assert len(np.unique(gw, axis=0)) >= 2
    dev.close()
    fresh.close()


# ---- 2. against the oracle: scaled geometry, emptied leaf slots ----
@pytest.mark.parametrize("seed,oset", rcs.CUT_FUZZ)
@pytest.mark.parametrize("tname", ["x2^10", "x2^-10"])
def test_scaled_reclip_matches_oracle(tname, seed, oset):
    rcs.assert_cut(seed, oset)
    options = rcs.options(seed, oset)
    keyA, keyB = ss.fuzz_key("identity", seed), ss.fuzz_key(tname, seed)
    (hsA, orcA), (hsB, orcB) = ss.case(keyA), ss.case(keyB)
    # the condition: power-of-two scaling keeps every comparison of the median split
    assert np.array_equal(orcA.bvh()["perm"], orcB.bvh()["perm"])
    assert np.array_equal(hsA.soa_arrays()["vertex_idx"], hsB.soa_arrays()["vertex_idx"])
    spp = ss.spp_of(seed)
    ref, cnt = ss.frame(keyB, spp, ss.REF)
    dev = rtamd.DeviceScene(hsA, 0, **options)
    n4 = dev.debug_scene_image("nodes4")
    assert _emptied(n4) == 0
    dev.update(hsB, reclip=True)
    img, st = dev.render(_params(hsB, spp=spp))
    err = float(np.abs(img - ref).max())
    m4 = dev.debug_scene_image("nodes4")
    emptied = _emptied(m4)
    print(f"{tname} seed {seed} {oset}: max |gpu - oracle| {err:.3e}, rays {rc.counts(st)}, emptied leaf slots {emptied}")
    assert err <= TOL64
    assert rc.counts(st) == ss.rays_counted(cnt)
    assert cnt.closest_hits > 0
    assert np.array_equal(n4[:, 24:], m4[:, 24:])   # an emptied slot keeps its ref
    # Cut records whose region the scaled triangle left, by the numpy clip.  With single-record leaves
    # ("split") each of them is an emptied slot; with the default leaves of up to two records both
    # records of a leaf would have to be left, so there the count is only printed.  Seed 2's two cut
    # records belong to a triangle that still straddles their plane at 2^10.
    clip, slot = rcs.regions(seed, oset)
    soa = hsB.soa_arrays()
    P, vidx = soa["vertex_pos"], soa["vertex_idx"].reshape(-1, 3)
    gone = sum(1 for g in np.flatnonzero(np.isfinite(clip).any(axis=1)) if not rcs.sh_clip(P[vidx[slot[g]]], clip[g]))
    assert gone >= 1 or (seed, tname) == (2, "x2^10")
    if oset == "split" and gone:
        assert emptied >= 1
    dev.close()


# ---- 3. against the plain refit ----
@pytest.mark.parametrize("scene,oset", list(rcs.CUT_FUZZ) + [("cornell", "default"), ("office", "default")])
def test_reclipped_boxes_lie_inside_the_plain_refit(scene, oset):
    rcs.assert_cut(scene, oset)
    options = rcs.options(scene, oset)
    hsA, hsU = rcs.host_a(scene), rcs.moved(scene)
    images = []
    for reclip in (False, True):
        dev = rtamd.DeviceScene(hsA, 0, **options)
        dev.update(hsU, reclip=reclip)
        images.append(dev.debug_scene_image("nodes4"))
        dev.close()
    plain, tight = images
    assert np.array_equal(plain[:, 24:], tight[:, 24:])   # refs and pad
    plo, phi, refs = _boxes(plain)
    tlo, thi, _ = _boxes(tight)
    assert np.all(tlo >= plo) and np.all(thi <= phi)
    leaf = np.broadcast_to(_leaf_slots(refs)[:, None, :], tlo.shape)
    smaller = int(((tlo > plo) & leaf).sum() + ((thi < phi) & leaf).sum())
    print(f"{scene} {oset}: {smaller} of {2 * int(leaf.sum())} leaf bounds strictly smaller")
    assert smaller > 0


# ---- 4. against the builder ----
@pytest.mark.parametrize("scene,oset", list(rcs.CUT_FUZZ) + [("cornell", "default")])
def test_round_trips_agree_with_the_builder(scene, oset):
    rcs.assert_cut(scene, oset)
    hs = rcs.moved(scene)   # a scene of its own to move
    posB = hs.soa_arrays()["vertex_pos"].copy()
    posA = rcs.host_a(scene).soa_arrays()["vertex_pos"].copy()
    hs.update_vertices(posA)
    dev = rtamd.DeviceScene(hs, 0, **rcs.options(scene, oset))
    first = {k: dev.debug_scene_image(k) for k in ("nodes4", "tris", "tnorm")}
    for trip in ((posA,), (posB, posA)):
        for pos in trip:
            hs.update_vertices(pos)
            dev.update(hs, reclip=True)
        again = {k: dev.debug_scene_image(k) for k in ("nodes4", "tris", "tnorm")}
        assert np.array_equal(first["tris"], again["tris"])
        assert np.array_equal(first["tnorm"].view(np.uint64), again["tnorm"].view(np.uint64))
        assert np.array_equal(first["nodes4"][:, 24:], again["nodes4"][:, 24:])
        a, b = first["nodes4"][:, :24].view(np.float32), again["nodes4"][:, :24].view(np.float32)
        far, differ = _steps_apart(a, b), int((a != b).sum())
        print(f"{scene} {oset} after {len(trip)} updates: {differ} bounds differ, {far} by more than one fp32 step")
        assert far == 0
    dev.close()


# ---- 5. against brute force ----
@pytest.mark.parametrize("seed,oset", [(1, "default"), (0, "split")])
def test_reclipped_scene_matches_brute_force(seed, oset):
    rcs.assert_cut(seed, oset)
    hsA, hsU = rcs.host_a(seed), rcs.moved(seed)
    soa = hsU.soa_arrays()
    P, vidx = soa["vertex_pos"], soa["vertex_idx"].reshape(-1, 3)
    rng = np.random.default_rng(13)
    n = 256
    o = qc.origins(hsU, rng.random((n, 3)))
    w = rng.dirichlet([1.0, 1.0, 1.0], size=n)   # interior points of random triangles
    target = (P[vidx[rng.integers(0, len(vidx), n)]] * w[:, :, None]).sum(axis=1)
    rays = qc.make_rays(o, target - o)
    want = ss.brute_force_t(hsU, rays)
    assert np.isfinite(want).sum() >= 200
    dev = rtamd.DeviceScene(hsA, 0, **rcs.options(seed, oset))
    dev.update(hsU, reclip=True)
    assert np.array_equal(dev.trace(rays)["t"], want)
    dev.close()


# ---- 6. edges ----
@pytest.mark.parametrize("seed,options", [(1, {"tree": "sah"}), (rcs.PLAIN_SEED, {}), (0, {})])
def test_flag_on_a_scene_without_a_table_is_the_plain_update(seed, options):
    hsA, hsU = rcs.host_a(seed), rcs.moved(seed)
    images = []
    for reclip in (False, True):
        dev = rtamd.DeviceScene(hsA, 0, **options)
        dev.update(hsU)   # allocates the update state: the bytes below are the flag's alone
        b0 = dev.device_bytes
        dev.update(hsU, reclip=reclip)
        assert dev.device_bytes == b0
        images.append({k: dev.debug_scene_image(k) for k in ("nodes4", "tris", "tnorm")})
        dev.close()
    for k in ("nodes4", "tris"):
        assert np.array_equal(images[0][k], images[1][k]), k
    assert np.array_equal(images[0]["tnorm"].view(np.uint64), images[1]["tnorm"].view(np.uint64))


def test_plain_and_reclipping_updates_queued_on_one_stream():
    import torch

    seed, oset = 1, "default"
    rcs.assert_cut(seed, oset)
    hs = rcs.moved(seed)
    posB = hs.soa_arrays()["vertex_pos"].copy()
    posA = rcs.host_a(seed).soa_arrays()["vertex_pos"].copy()
    posC = 0.5 * (posA + posB)
    hs.update_vertices(posA)
    dev = rtamd.DeviceScene(hs, 0)
    p = _params(hs)
    queue = ((posB, True), (posC, False), (posA, True))
    outs = [torch.zeros((uc.H, uc.W, 3), dtype=torch.float64, device="cuda:0") for _ in queue]
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    for (pos, reclip), out in zip(queue, outs):   # no host synchronisation in between
        hs.update_vertices(pos)
        dev.update(hs, stream=stream.cuda_stream, reclip=reclip)
        dev.launch(p, out.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    got = [o.cpu().numpy() for o in outs]
    for (pos, _), frame in zip(queue, got):
        hs.update_vertices(pos)
        fresh = rtamd.DeviceScene(hs, 0)
        assert np.array_equal(frame, fresh.render(p)[0])
        fresh.close()
    assert not np.array_equal(got[0], got[1]) and not np.array_equal(got[1], got[2])
    dev.close()


def test_reclip_follows_the_launches_onto_the_cu_masked_stream():
    import torch

    rcs.assert_cut("cornell", "default")
    hs = uc.generated("cornell")
    posA = hs.soa_arrays()["vertex_pos"].copy()
    dev = rtamd.DeviceScene(hs, 0, reserve_cus=32)
    p = _params(hs, GW, GH)
    outs = [torch.zeros((GH, GW, 3), dtype=torch.float64, device="cuda:0") for _ in range(2)]
    rays = torch.from_numpy(_rays(hs)).cuda()
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    dev.launch(p, outs[0].data_ptr(), stream=stream.cuda_stream)
    hs.update_vertices(uc.generated_pos_b(hs))
    dev.update(hs, stream=stream.cuda_stream, reclip=True)
    dev.launch(p, outs[1].data_ptr(), stream=stream.cuda_stream)
    hits = dev.trace(rays, stream=stream.cuda_stream)
    stream.synchronize()
    got = [o.cpu().numpy() for o in outs]
    hits = {k: v.cpu().numpy() for k, v in hits.items()}
    fresh = rtamd.DeviceScene(hs, 0)
    assert np.array_equal(got[1], fresh.render(p)[0])
    assert _same_hits(hits, {k: v.cpu().numpy() for k, v in fresh.trace(rays).items()})
    fresh.close()
    hs.update_vertices(posA)
    first = rtamd.DeviceScene(hs, 0)
    assert np.array_equal(got[0], first.render(p)[0]) and not np.array_equal(got[0], got[1])
    first.close()
    dev.close()


def test_device_bytes_grow_at_the_first_reclipping_update_only():
    clip, _ = rcs.assert_cut("cornell", "default")
    records, cut = len(clip), int(np.isfinite(clip).any(axis=1).sum())
    hs = uc.generated("cornell")
    s = hs.soa.contents
    plain, tight = rtamd.DeviceScene(hs, 0), rtamd.DeviceScene(hs, 0)
    b0 = plain.device_bytes
    assert tight.device_bytes == b0
    state = 2 * 24 * s.n_vertices + 24 * (s.n_vertex_idx // 3) + 4 * len(plain.debug_scene_image("nodes4"))
    for _ in range(3):
        plain.update(hs)
        assert plain.device_bytes == b0 + state   # never grows by the table
    tight.update(hs)
    assert tight.device_bytes == b0 + state
    for reclip in (True, False, True):
        tight.update(hs, reclip=reclip)
        assert tight.device_bytes == b0 + state + 4 * records + 48 * cut
    fresh = rtamd.DeviceScene(hs, 0)
    fresh.update(hs, reclip=True)   # a first update that re-clips allocates both
    assert fresh.device_bytes == b0 + state + 4 * records + 48 * cut
    p = _params(hs, GW, GH)
    assert np.array_equal(fresh.render(p)[0], plain.render(p)[0])
    for d in (plain, tight, fresh):
        d.close()
