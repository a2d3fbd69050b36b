"""The device against the CPU oracle on scaled, shifted and far-viewed scenes and on far-origin
rays (tests/scale_scenes.py; the oracle side is tests/test_scale_oracle.py, which also enforces
that these inputs are free of the reference's measure-zero divergences and not vacuous).

The 4-wide production kernels evaluate a box slab as one fused plane * inv - o * inv, which the
oracle does not model: it stays conservative only because the origin is first moved to the root
box's entry point in fp64 and the box growth delta = 2^-20 max|vertex| is relative.
That set-up exists twice (rt_render.hip, and rt_walk_body.inc, which the query, AO and camera kernels
include); both texts, and every kernel that holds one, are reached here.

Tolerances are those of tests/test_gpu_parity.py: fp64 output within 1e-12, fp32 output within 1e-6,
ray counts exact; query results bit for bit (query_cases.check_hits)."""
import ctypes as C

import numpy as np
import pytest

import query_cases as qc
import radiance_cases as rc
import rtamd
import scale_scenes as ss
from rtamd import abi

pytestmark = pytest.mark.gpu

TOL64 = 1e-12
TOL32 = 1e-6
REF, ORD = ss.REF, ss.ORD


@pytest.fixture(autouse=True)
def _gpu(gpu_available):
    return gpu_available


def _render64(dev, hs, spp, flags=0):
    p = hs.render_params(0, 0, spp)
    p.out_format = rtamd.RT_OUT_RGB_F64
    p.flags = flags
    return dev.render(p)


def _check_frame(key, spp, trees=(), fp32=False):
    """The keyed scene's own frame on the default tree against the oracle's reference mode; the
    other trees bit for bit against the default one.  Returns the oracle's Counts."""
    hs, orc = ss.case(key)
    ref, cnt = ss.frame(key, spp, REF)
    dev = rtamd.DeviceScene(hs, 0)
    img, st = _render64(dev, hs, spp)
    err = float(np.abs(img - ref).max())
    print(f"{key}: max |gpu - oracle| {err:.3e}, rays P/S/R {rc.counts(st)} (oracle {ss.rays_counted(cnt)})")
    assert err <= TOL64
    assert rc.counts(st) == ss.rays_counted(cnt)
    if fp32:
        p = hs.render_params(0, 0, spp)
        p.out_format = rtamd.RT_OUT_RGB_F32
        img32, _ = dev.render(p)
        assert img32.dtype == np.float32
        assert np.abs(img32.astype(np.float64) - ref).max() <= TOL32
    dev.close()
    for tree in trees:
        devt = rtamd.DeviceScene(hs, 0, tree=tree)
        imgt, stt = _render64(devt, hs, spp)
        assert np.array_equal(imgt, img) and rc.counts(stt) == rc.counts(st), tree
        devt.close()
    return cnt


# ---- 1. render parity ----
@pytest.mark.parametrize("seed", ss.SEEDS)
@pytest.mark.parametrize("tname", sorted(ss.TRANSFORMS))
def test_transformed_fuzz_scene_matches_oracle(tname, seed):
    both = seed in (0, 4)
    _check_frame(ss.fuzz_key(tname, seed), ss.spp_of(seed), trees=("reference", "sah") if both else (), fp32=both)


@pytest.mark.parametrize("tname", sorted(ss.TRANSFORMS))
def test_inputs_are_not_vacuous(tname):
    ss.check_not_vacuous(tname)


@pytest.mark.parametrize("name", ss.KAT_NAMES)
@pytest.mark.parametrize("tname", ss.BRUTE_TRANSFORMS)
def test_transformed_kat_scene_matches_oracle(tname, name):
    cnt = _check_frame(("kat", tname, name), 1)
    assert cnt.closest_hits > 0


# ---- 2. canonical counters: the 2-wide kernel's t_off / hi_c window at scale ----
@pytest.mark.parametrize("seed", range(4))
@pytest.mark.parametrize("tname", ["x2^10", "x2^-10", "shift1e6", "x2^-16"])
def test_canonical_counters_match_ordered_oracle(tname, seed):
    key, spp = ss.fuzz_key(tname, seed), ss.spp_of(seed)
    hs, _ = ss.case(key)
    _, cnt = ss.frame(key, spp, ORD)
    dev = rtamd.DeviceScene(hs, 0)
    _, st = _render64(dev, hs, spp, rtamd.RT_FLAG_TRAVERSAL_STATS)
    assert (st.node_visits, st.tri_tests, st.closest_hits) == (cnt.node_visits, cnt.tri_tests, cnt.closest_hits)
    assert st.node_visits > 0 and st.tri_tests > 0
    dev.close()


# ---- 3. a stray vertex, a far light, a far eye ----
@pytest.mark.parametrize("seed", ss.VARIANT_SEEDS)
@pytest.mark.parametrize("vname", sorted(ss.VARIANTS))
def test_variant_matches_oracle(vname, seed):
    cnt = _check_frame(("variant", vname, seed), 1)
    assert cnt.closest_hits > 0


# ---- 4. queries ----
_dev = {}


def _far_device(name, tree):
    """One upload per (generated scene, tree), shared by the far-ray cases."""
    if (name, tree) not in _dev:
        _dev[(name, tree)] = rtamd.DeviceScene(ss.far_scene(name)[0], 0, tree=tree)
    return _dev[(name, tree)]


def _check_queries(dev, rays, want, P, vidx, perm):
    """rt_trace_closest through check_hits and rt_trace_occluded against the oracle's hits cut at tmax."""
    cut = ss.within_tmax(want, rays)
    got, st = dev.trace(rays, stats=True)
    qc.check_hits(got, cut, rays, P, vidx, perm)
    assert st.rays == len(rays) and st.hits == int(cut["hit"].sum()) and st.watchdog == 0
    occ = dev.trace(rays, occluded=True)
    assert np.array_equal(occ.astype(bool), cut["hit"])


@pytest.mark.parametrize("tree", [None, "reference"])
@pytest.mark.parametrize("factor", ss.FAR_FACTORS)
@pytest.mark.parametrize("flavour", ss.FAR_FLAVOURS)
@pytest.mark.parametrize("name", ss.FAR_SCENES)
def test_far_rays_match_ordered_oracle(name, flavour, factor, tree):
    _, _, P, vidx, perm = ss.far_scene(name)
    rays, want = ss.far_case(name, flavour, factor)
    assert want["hit"].sum() >= 64
    _check_queries(_far_device(name, tree), rays, want, P, vidx, perm)


@pytest.mark.parametrize("tname", ["x2^10", "x2^-14", "shift1e6"])
def test_near_rays_on_transformed_scene_match_ordered_oracle(tname):
    hs, orc = ss.case(ss.fuzz_key(tname, 0))
    P, vidx, perm = ss.scene_arrays(hs, orc)
    for rays in (qc.random_rays(hs, 512), qc.vertex_rays(hs, P, 512)):
        want = qc.oracle_hits(orc, rays, ORD)
        assert want["hit"].sum() >= 64 and not want["hit"].all()
        for tree in (None, "reference"):
            dev = rtamd.DeviceScene(hs, 0, tree=tree)
            _check_queries(dev, rays, want, P, vidx, perm)
            dev.close()


# ---- 5. radiance of the telephoto camera's own rays (a large t_off in the render kernel's set-up) ----
@pytest.mark.parametrize("seed", [0, 1])
def test_radiance_of_telephoto_rays_equals_the_render(seed):
    hs, _ = ss.case(("variant", "telephoto1e4", seed))
    dev = rtamd.DeviceScene(hs, 0)
    p = hs.render_params(0, 0, 1)
    p.out_format = rtamd.RT_OUT_RGB_F64
    img, rst = dev.render(p)
    rgb, st = dev.radiance(rtamd.camera_rays(p), p, stats=True)
    assert np.array_equal(rgb.reshape(ss.H, ss.W, 3), img)
    assert rc.counts(st) == rc.counts(rst)
    assert len(np.unique(img.reshape(-1, 3), axis=0)) > 2
    dev.close()


# ---- 6. occlusion fans and gathers (rt_ao.inc's copy of the set-up) ----
def _fan_inputs(tname):
    """(HostScene, DeviceScene, point records of the frame's primary hits with half the root box's
    diagonal as radius, bias): the radius scales with the scene, the bias is 1e-6 s."""
    import torch

    hs, _ = ss.case(ss.fuzz_key(tname, 0))
    dev = rtamd.DeviceScene(hs, 0)
    rays = torch.from_numpy(rtamd.camera_rays(hs.render_params(0, 0, 1))).cuda()
    pts = rtamd.ao_points_from_hits(rays, dev.trace(rays)).cpu().numpy()
    assert pts.shape == (ss.W * ss.H, 8)
    lo, hi = dev.bounds()
    e = hi - lo
    pts[:, 6] = 0.5 * np.sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2])
    return hs, dev, pts, 1e-6 * ss.TRANSFORMS[tname][0]


@pytest.mark.parametrize("k", [5, 16])
@pytest.mark.parametrize("tname", ["x2^10", "x2^-10", "shift1e6"])
def test_ao_equals_the_written_out_fan(tname, k):
    hs, dev, pts, bias = _fan_inputs(tname)
    dirs = rtamd.ao_directions(k, 7, seed=1)
    occ = dev.trace(rtamd.ao_rays_host(pts, dirs, 3, bias), occluded=True)
    assert set(np.unique(occ)) <= {0, 1}
    occ = occ.reshape(len(pts), k).astype(np.int64)
    want = k - occ.sum(axis=1)
    got, st = dev.ao(pts, dirs, seed=3, bias=bias, stats=True)
    assert got.dtype == np.int32 and np.array_equal(got, want)
    assert st.rays == len(pts) * k and st.hits == int(occ.sum()) and st.watchdog == 0
    assert np.any((want > 0) & (want < k))   # partly open fans
    dev.close()


@pytest.mark.parametrize("k", [5, 16])
@pytest.mark.parametrize("tname", ["x2^10", "x2^-10", "shift1e6"])
def test_gather_equals_the_written_out_mean(tname, k):
    hs, dev, pts, bias = _fan_inputs(tname)
    dirs = rtamd.ao_directions(k, 7, seed=1)
    p = rc.params(hs, 8, 8)
    R, rst = dev.radiance(rtamd.ao_rays_host(pts, dirs, 3, bias), p, stats=True)
    R = R.reshape(len(pts), k, 3)
    acc = np.zeros((len(pts), 3))
    for s in range(k):   # in sample order, one add per sample (rt_hip.h, rt_trace_gather)
        acc = acc + R[:, s, :]
    want = acc / k
    got, st = dev.gather(pts, dirs, p, seed=3, bias=bias, stats=True)
    assert got.dtype == np.float64 and np.array_equal(got, want)
    assert rc.counts(st) == rc.counts(rst) and st.pixels == len(pts)
    got32 = dev.gather(pts, dirs, rc.copy_params(p, out_format=rtamd.RT_OUT_RGB_F32), seed=3, bias=bias)
    assert got32.dtype == np.float32 and np.array_equal(got32, want.astype(np.float32))
    assert len(np.unique(want, axis=0)) >= 2 and np.any(np.any(R != R[:, :1, :], axis=(1, 2)))
    dev.close()


# ---- 7. ray order keys in a box far from the origin ----
def test_order_keys_on_shifted_scene():
    hs, orc = ss.case(ss.fuzz_key("shift1e6", 0))
    P, _, _ = ss.scene_arrays(hs, orc)
    rays = np.concatenate([qc.random_rays(hs, 512), qc.vertex_rays(hs, P, 512)])
    dev = rtamd.DeviceScene(hs, 0)
    lo, hi = dev.bounds()
    perm, keys = dev.ray_order(rays, keys=True)
    want = rtamd.ray_keys_host(lo, hi, rays)
    assert np.array_equal(keys, want)
    assert np.array_equal(perm, np.argsort(want, kind="stable"))
    assert len(np.unique(want)) > 256 and np.all(want != abi.RT_ORDER_KEY_DEGENERATE)
    dev.close()


# ---- 8. the supported coordinate range (rt_hip.h at rt_scene_upload) ----
def test_top_of_the_supported_range_matches_oracle():
    # max|vertex| = 3.2 * 2^59 = 1.8e18, just below RT_MAX_COORDINATE: the fused slab's o * inv of an
    # axis-parallel ray (inv = 1e20) reaches 1.8e38 and is still finite
    key = ("scaled", ss.TOP_SCALE, 0)
    hs, orc = ss.case(key)
    assert 0.5 * abi.RT_MAX_COORDINATE < np.abs(hs.soa_arrays()["vertex_pos"]).max() <= abi.RT_MAX_COORDINATE
    cnt = _check_frame(key, 1, trees=("reference",), fp32=True)
    assert cnt.closest_hits > 0
    P, vidx, perm = ss.scene_arrays(hs, orc)
    dev = rtamd.DeviceScene(hs, 0)
    for flavour in ("axis", "vertex"):
        rays = ss.far_rays(hs, 1e2, 256, 2, flavour)
        want = qc.oracle_hits(orc, rays, ORD)
        assert want["hit"].sum() >= 64
        _check_queries(dev, rays, want, P, vidx, perm)
    dev.close()


def test_stray_vertex_at_the_limit_matches_oracle():
    cnt = _check_frame(("variant", "outlier2^61", 0), 1)
    assert cnt.closest_hits > 0


def _upload(hs):
    h = C.c_void_p()
    opt = rtamd.upload_options()
    rcode = rtamd.hip_lib().rt_scene_upload_ex(hs.soa, hs.bvh, 0, C.byref(opt), C.byref(h))
    return int(rcode), h


@pytest.mark.parametrize("key", [("variant", "outlier1e30", 0), ("variant", "outlier1e30", 1), ("scaled", 1e20, 0)],
                         ids=["outlier1e30-0", "outlier1e30-1", "x1e20"])
def test_coordinates_beyond_the_supported_range_are_refused(key):
    # At these magnitudes the fused slab's o * inv overflows fp32 for a clamped reciprocal (1e20)
    # and an axis-parallel ray misses every box: upload refuses the scene instead.
    rcode, h = _upload(ss.case(key)[0])
    assert rcode == abi.RT_ERR_UNSUPPORTED and not h.value
    assert b"coordinate" in rtamd.hip_lib().rt_last_error()
