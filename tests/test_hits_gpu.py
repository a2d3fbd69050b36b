"""rt_trace_hits on the device (include/rt_hip.h) against the hit lists of
hits_cases, which are built without the code under test.  Every comparison is bit for bit, on the
raw 64-byte rows and the counts: t, alpha, beta and the normal are IEEE fp64 operations in the CPU's
order without contraction, so a last-bit difference is a bug."""
import ctypes as C

import numpy as np
import pytest

import fuzz_scenes
import hits_cases as hc
import minirt
import kat_scenes
import query_cases as qc
import rtamd
import update_cases as uc
from rtamd import abi

pytestmark = pytest.mark.gpu

TREES = [None, "sah", "reference"]   # None: the default tree, the SBVH
# the smallest generated scene of query_cases whose rays spill the 8-entry LDS stack ring; at 256
# rays its lists are also the long ones (asserted of the reference below)
RANDOM_TRIS = 20000
GUARD_ROWS = 4


@pytest.fixture(autouse=True)
def _gpu(gpu_available):
    return gpu_available


def _scene(name):
    return qc.scene(name, qc.SCENES[name].get("n_triangles", 0))


_dev = {}


def _device(name, tree):
    """One upload per (scene, tree), shared by the tests of this module."""
    if (name, tree) not in _dev:
        _dev[(name, tree)] = rtamd.DeviceScene(_scene(name)[0], 0, tree=tree)
    return _dev[(name, tree)]


def _rays(name, kind, n):
    hs, orc, P, vidx, perm = _scene(name)
    if kind == "random":
        return qc.random_rays(hs, n)
    if kind == "vertex":
        return qc.vertex_rays(hs, P, n)
    return qc.axis_rays(hs, n)


def _lists(name, kind, n):
    return hc.hit_lists((name, kind, n), _scene(name)[0], _rays(name, kind, n))


def _keys(t, slot):
    rec = np.zeros(len(t), rtamd.HIT_KEY_DTYPE)
    rec["t"], rec["slot"] = t, slot
    rec["reserved_"] = 0x5A5A5A5A   # ignored by the call
    return rec


def _trace_hits(dev, rays, k, after=None, stats=False, stream=None):
    """One rt_trace_hits call through the C ABI on guarded buffers: (rows int64 [n, k, 8], count
    uint32 [n]) as numpy, and the QueryStats with stats=True.  The words behind the n * k rows and
    the n counts must come back untouched."""
    import torch

    n = len(rays)
    d_rays = rays if isinstance(rays, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(rays)).cuda()
    d_after = None if after is None else torch.from_numpy(after.view(np.int64).reshape(n, 2).copy()).cuda()
    out = torch.full((n * k + GUARD_ROWS, 8), 7.0, dtype=torch.float64, device="cuda")
    cnt = torch.full((n + GUARD_ROWS,), 0x7777, dtype=torch.int32, device="cuda")
    st = abi.QueryStats() if stats else None
    torch.cuda.synchronize()
    rc = rtamd.hip_lib().rt_trace_hits(dev._h, d_rays.data_ptr(), n, k, d_after.data_ptr() if after is not None else None,
                                       out.data_ptr(), cnt.data_ptr(), C.byref(st) if stats else None,
                                       C.c_void_p(stream) if stream else None)
    assert rc == abi.RT_OK, rtamd.hip_lib().rt_last_error()
    torch.cuda.synchronize()
    assert bool((out[n * k:] == 7.0).all()) and bool((cnt[n:] == 0x7777).all())
    rows = out[:n * k].cpu().numpy().view(np.int64).reshape(n, k, 8)
    count = cnt[:n].cpu().numpy().view(np.uint32)
    return (rows, count, st) if stats else (rows, count)


def _trace_closest(dev, rays):
    import torch

    n = len(rays)
    d_rays = torch.from_numpy(np.ascontiguousarray(rays)).cuda()
    out = torch.zeros((n, 8), dtype=torch.float64, device="cuda")
    assert rtamd.hip_lib().rt_trace_closest(dev._h, d_rays.data_ptr(), n, out.data_ptr(), None, None) == abi.RT_OK
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.int64)


def _check(got, lists, k, what=""):
    """The device's rows and counts against the lists' first k entries, bit for bit."""
    rows, count = got
    want, wcount = hc.rows(lists, k)
    bad = np.nonzero((rows != hc.raw(want).reshape(rows.shape)).any(axis=(1, 2)) | (count != wcount))[0]
    print(f"{what} k {k}: rays {len(lists)}, hits {int(wcount.sum())}, longest list {max(len(h) for h in lists)}, "
          f"differing rays {len(bad)}" + (f", first {bad[0]}: got count {count[bad[0]]} want {wcount[bad[0]]}" if len(bad) else ""))
    assert len(bad) == 0


# ---- k = 1 equals rt_trace_closest ----
@pytest.mark.parametrize("tree", TREES)
@pytest.mark.parametrize("name", sorted(qc.SCENES))
def test_k1_equals_closest(name, tree):
    dev = _device(name, tree)
    for kind in ("random", "vertex", "axis"):
        rays = _rays(name, kind, 512)
        rows, count = _trace_hits(dev, rays, 1)
        closest = _trace_closest(dev, rays)
        assert np.array_equal(rows.reshape(-1, 8), closest), kind
        hit = np.isfinite(closest.view(np.float64)[:, 0])
        assert np.array_equal(count, hit.astype(np.uint32)), kind
        assert hit.any()


# ---- the lists equal H ----
@pytest.mark.parametrize("k", [3, 8])
@pytest.mark.parametrize("name,n", [("cornell", 256), ("random_tris", 256), ("office", 128)])
def test_lists_equal_the_reference(name, n, k):
    lists = _lists(name, "random", n)
    length = np.array([len(h) for h in lists])
    if name == "random_tris":   # lists longer than one and than two rounds of the largest k
        assert qc.SCENES[name]["n_triangles"] == RANDOM_TRIS
        assert (length > 8).sum() >= 32 and (length > 16).sum() >= 1
    assert (length > 0).sum() >= n // 4
    for tree in (None, "reference"):
        _check(_trace_hits(_device(name, tree), _rays(name, "random", n), k), lists, k, f"{name} {tree}")


# ---- resumed rounds ----
@pytest.mark.parametrize("name,n", [("cornell", 256), ("random_tris", 256)])
def test_all_hits_equals_the_reference(name, n):
    lists = _lists(name, "random", n)
    rays = _rays(name, "random", n)
    dev = _device(name, None)
    got = dev.all_hits(rays, k=3)
    want = np.concatenate(lists)
    offsets = np.concatenate([[0], np.cumsum([len(h) for h in lists])])
    assert got["offsets"].dtype == np.int64 and np.array_equal(got["offsets"], offsets)
    for f in ("t", "alpha", "beta", "normal"):
        assert np.array_equal(got[f].view(np.int64), np.ascontiguousarray(want[f]).view(np.int64)), f
    for f in ("slot", "mesh", "prim"):
        assert got[f].dtype == np.int32 and np.array_equal(got[f], want[f]), f
    # a resumed call on exhausted lists: count 0 and all-miss rows
    some = np.array([i for i, h in enumerate(lists) if len(h)][:64])
    last = np.array([lists[i][-1] for i in some])
    rows, count = _trace_hits(dev, rays[some], 3, after=_keys(last["t"], last["slot"]))
    assert not count.any() and np.array_equal(rows, hc.raw(hc.rows([lists[0][:0]] * len(some), 3)[0]).reshape(rows.shape))


# ---- ties ----
@pytest.mark.parametrize("name", ["cornell", "office"])
def test_ties_are_ordered_by_slot(name):
    lists = _lists(name, "vertex", 256)
    tied = [h for h in lists if len(h) > 1 and (np.diff(h["t"]) == 0.0).any()]
    assert len(tied) >= 16
    for h in tied:
        same = np.diff(h["t"]) == 0.0
        assert np.all(np.diff(h["slot"])[same] > 0)
    rays = _rays(name, "vertex", 256)
    for tree in (None, "reference"):
        _check(_trace_hits(_device(name, tree), rays, 8), lists, 8, f"{name} vertex {tree}")
        _check(_trace_hits(_device(name, tree), rays, 2), lists, 2, f"{name} vertex {tree}")


@pytest.fixture(scope="module")
def twins(tmp_path_factory):
    """Four stacked quads, every triangle listed twice: coplanar twins with adjacent slots or not."""
    meshes = []
    for z, mode in ((0.0, "FLAT"), (-0.4, "PHONG"), (-0.9, "FLAT"), (-1.3, "PHONG")):
        v, t = kat_scenes.quad(-1.5 + 0.1 * z, 1.4, -1.2, 1.3 + 0.2 * z, z)
        meshes.append(minirt.Mesh(v, t + t, mode, kat_scenes.FLAT_MAT))
    cam = ((0.013, 0.021, 4.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 40.0, 9, 7)
    path = tmp_path_factory.mktemp("twins") / "twins.sce"
    minirt.write_sce(path, meshes, [((0.5, 0.7, 3.0), (0.9, 0.9, 0.9))], cam, (0.1, 0.2, 0.3), (0.2, 0.2, 0.2), 2)
    hs = rtamd.HostScene.load(path)
    hs.prepare()
    return hs


def test_coplanar_twins(twins):
    hs = twins
    assert len(hs.soa_arrays()["vertex_idx"]) == 16
    rng = np.random.default_rng(3)
    target = np.stack([rng.uniform(-1.2, 1.2, 128), rng.uniform(-1.0, 1.0, 128), np.full(128, -1.3)], 1)
    o = np.stack([0.5 * target[:, 0] + 0.1, 0.5 * target[:, 1] - 0.1, np.full(128, 3.0)], 1)
    through = qc.make_rays(o, target - o)   # most cross all four planes inside the quads
    rays = np.concatenate([through, qc.random_rays(hs, 64), qc.vertex_rays(hs, hs.soa_arrays()["vertex_pos"], 64)])
    lists = hc.hit_lists(("twins",), hs, rays)
    assert sum(len(h) == 8 for h in lists) >= 16
    for h in lists:   # every t twice, slots ascending
        assert len(h) % 2 == 0
        assert np.array_equal(h["t"][0::2], h["t"][1::2]) and np.all(h["slot"][0::2] < h["slot"][1::2])
    for tree in TREES:
        dev = rtamd.DeviceScene(hs, 0, tree=tree)
        for k in (1, 2, 3, 8):
            _check(_trace_hits(dev, rays, k), lists, k, f"twins {tree}")
        # resuming at the first of a tied pair returns its twin first
        full = np.array([i for i, h in enumerate(lists) if len(h) == 8])
        first = np.array([lists[i][2] for i in full])
        rows, count = _trace_hits(dev, rays[full], 8, after=_keys(first["t"], first["slot"]))
        _check((rows, count), [lists[i][3:] for i in full], 8, f"twins {tree} resumed")
        assert np.array_equal(rows[:, 0, 0].view(np.float64), first["t"])
        dev.close()


# ---- SBVH duplicates ----
def test_sbvh_duplicates_are_listed_once():
    hs = _scene("office")[0]
    clip, slot = rtamd.clip_regions(hs)
    cut = np.isfinite(clip).any(axis=1)
    assert cut.any() and len(slot) > len(np.unique(slot))   # triangles with several (cut) records
    split = np.unique(slot[cut])
    rays = np.concatenate([_rays("office", "random", 128), _rays("office", "vertex", 256)])
    lists = _lists("office", "random", 128) + _lists("office", "vertex", 256)
    assert sum(np.isin(h["slot"], split).any() for h in lists) >= 16   # split triangles are in the lists
    rows, count = _trace_hits(_device("office", None), rays, 8)
    slots = rows.view(np.int32)[:, :, 12]
    for i in range(len(rays)):
        s = slots[i, :count[i]]
        assert len(np.unique(s)) == len(s)
    sah = _trace_hits(_device("office", "sah"), rays, 8)
    assert np.array_equal(rows, sah[0]) and np.array_equal(count, sah[1])
    _check((rows, count), lists, 8, "office sbvh")


# ---- `after` ----
def test_after_semantics():
    name = "random_tris"
    lists = _lists(name, "random", 256)
    rays = _rays(name, "random", 256)
    dev = _device(name, None)
    n = len(rays)
    # {-inf, -1} equals NULL
    none = _trace_hits(dev, rays, 8)
    free = _trace_hits(dev, rays, 8, after=_keys(np.full(n, -np.inf), np.full(n, -1)))
    assert np.array_equal(none[0], free[0]) and np.array_equal(none[1], free[1])
    # a key from the middle of H returns exactly the tail; one below the first hit, all of H
    mid = [len(h) // 2 for h in lists]
    t = np.array([h["t"][m] if len(h) else 1.0 for h, m in zip(lists, mid)])
    s = np.array([h["slot"][m] if len(h) else 0 for h, m in zip(lists, mid)])
    tails = [h[m + 1:] for h, m in zip(lists, mid)]
    assert sum(len(x) > 0 for x in tails) >= 64
    for x, h, ti, si in zip(tails[:32], lists, t, s):
        assert np.array_equal(x, hc.after_filter(h, ti, si))
    for k in (3, 8):
        _check(_trace_hits(dev, rays, k, after=_keys(t, s)), tails, k, "tail")
    # the same t with the slot before: the entry itself comes first
    _check(_trace_hits(dev, rays, 8, after=_keys(t, s - 1)), [h[m:] for h, m in zip(lists, mid)], 8, "from the key's own entry")
    # a NaN t lists nothing
    rows, count = _trace_hits(dev, rays, 8, after=_keys(np.full(n, np.nan), np.full(n, -1)))
    assert not count.any() and np.all(rows.view(np.float64)[:, :, 0] == np.inf)
    # the Python layer's forms of `after`
    got = dev.hits(rays, 3, after=(t, s))
    want, wcount = hc.rows(tails, 3)
    assert got["t"].shape == (n, 3) and got["normal"].shape == (n, 3, 3) and got["count"].dtype == np.int32
    assert np.array_equal(got["count"], wcount.astype(np.int32))
    for f in ("t", "alpha", "beta", "normal", "slot", "mesh", "prim"):
        assert np.array_equal(got[f], want[f]), f


def test_tied_after_key_returns_the_twin_first():
    lists = _lists("cornell", "vertex", 256)
    rays = _rays("cornell", "vertex", 256)
    pick = [(i, int(np.nonzero(np.diff(h["t"]) == 0.0)[0][0])) for i, h in enumerate(lists)
            if len(h) > 1 and (np.diff(h["t"]) == 0.0).any()]
    assert len(pick) >= 16
    idx = np.array([i for i, _ in pick])
    first = np.array([lists[i][j] for i, j in pick])
    rows, count = _trace_hits(_device("cornell", None), rays[idx], 3, after=_keys(first["t"], first["slot"]))
    _check((rows, count), [lists[i][j + 1:] for i, j in pick], 3, "twin")
    assert np.array_equal(rows[:, 0, 0].view(np.float64), first["t"])
    assert np.all(rows.view(np.int32)[:, 0, 12] > first["slot"])


# ---- tmax, degenerate rays ----
def test_finite_tmax_cuts_the_list():
    lists = _lists("random_tris", "random", 256)
    rays = _rays("random_tris", "random", 256).copy()
    long = np.array([i for i, h in enumerate(lists) if len(h) >= 4])
    assert len(long) >= 32
    dev = _device("random_tris", None)
    third = np.array([lists[i]["t"][2] for i in long])
    for tmax, third_in in ((third, False), (np.nextafter(third, np.inf), True)):   # t < tmax: exclusive
        r = rays[long]
        r[:, 6] = tmax
        cut = hc.hit_lists(("random_tris", "tmax", third_in), _scene("random_tris")[0], r)
        for i, h, tm in zip(long, cut, tmax):
            assert np.array_equal(h, lists[i][lists[i]["t"] < tm]) and len(h) < len(lists[i])
            assert (len(h) >= 3 and h["t"][2] == lists[i]["t"][2]) if third_in else len(h) <= 2
        _check(_trace_hits(dev, r, 8), cut, 8, f"tmax, third hit {'in' if third_in else 'out'}")


def test_degenerate_rays_have_empty_lists():
    rays = _rays("cornell", "random", 256)
    lists = _lists("cornell", "random", 256)
    good = rays[[i for i, h in enumerate(lists) if len(h)]][:16]
    bad = []
    for col, val in ((0, np.nan), (1, np.inf), (2, -np.inf), (3, np.nan), (4, np.inf), (5, -np.inf),
                     (6, np.nan), (6, 0.0), (6, 1e-5), (6, -1.0)):
        r = good.copy()
        r[:, col] = val
        bad.append(r)
    z = good.copy()
    z[:, 3:6] = 0.0
    bad.append(z)
    r = np.concatenate(bad + [good])   # the good rays after them still hit
    nb = len(r) - len(good)
    dev = _device("cornell", None)
    rows, count, st = _trace_hits(dev, r, 3, stats=True)
    assert not count[:nb].any() and count[nb:].all()
    assert np.array_equal(rows[:nb], hc.raw(hc.rows([lists[0][:0]] * nb, 3)[0]).reshape(nb, 3, 8))
    assert st.hits == int(count.sum()) and dev.status() == abi.RT_OK


# ---- shapes ----
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_partial_waves_and_blocks(n):
    lists = _lists("random_tris", "random", 256) + _lists("random_tris", "vertex", 256)
    rays = np.concatenate([_rays("random_tris", "random", 256), _rays("random_tris", "vertex", 256)])
    dev = _device("random_tris", None)
    for k in (1, 3, 8):   # _trace_hits checks the guard words behind the n * k rows and n counts
        rows, count, st = _trace_hits(dev, rays[:n], k, stats=True)
        assert rows.shape == (n, k, 8) and count.shape == (n,)
        _check((rows, count), lists[:n], k, f"n {n}")
        assert (st.rays, st.hits, st.watchdog) == (n, int(count.sum()), 0)


def test_zero_rays_touch_nothing():
    import torch

    dev = _device("cornell", None)
    hits = torch.full((4, 8), 7.0, dtype=torch.float64, device="cuda")
    cnt = torch.full((4,), 7, dtype=torch.int32, device="cuda")
    st = abi.QueryStats(rays=-1)
    assert rtamd.hip_lib().rt_trace_hits(dev._h, hits.data_ptr(), 0, 8, None, hits.data_ptr(), cnt.data_ptr(),
                                         C.byref(st), None) == abi.RT_OK
    torch.cuda.synchronize()
    assert (st.rays, st.hits) == (0, 0) and bool((hits == 7.0).all()) and bool((cnt == 7).all())
    got = dev.hits(np.zeros((0, 8)), 3)
    assert got["t"].shape == (0, 3) and got["normal"].shape == (0, 3, 3) and got["count"].shape == (0,)
    assert dev.all_hits(np.zeros((0, 8)))["offsets"].tolist() == [0]


# ---- the spill path ----
def test_stack_spill_path():
    lists = _lists("random_tris", "random", 256)
    rays = _rays("random_tris", "random", 256)
    dev = _device("random_tris", "reference")
    for k in (3, 8):
        rows, count, st = _trace_hits(dev, rays, k, stats=True)
        assert st.stack_spills > 0   # without it this test proves nothing about the spill path
        _check((rows, count), lists, k, "spill")
        assert st.watchdog == 0


# ---- after an update ----
def test_lists_after_update_positions_with_reclip():
    hs = uc.generated("office")
    posB = uc.generated_pos_b(hs)
    dev = rtamd.DeviceScene(hs, 0, tree="sbvh")
    dev.set_triangle_order(hs.slot_triangles())
    rays = np.concatenate([qc.random_rays(hs, 128), qc.vertex_rays(hs, posB, 128)])
    before = _trace_hits(dev, rays, 8)
    dev.update_positions(posB, reclip=True)
    hs.update_vertices(posB)
    fresh = rtamd.DeviceScene(hs, 0, tree="sbvh")
    for k in (3, 8):
        got, want = _trace_hits(dev, rays, k), _trace_hits(fresh, rays, k)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert not np.array_equal(before[0], got[0]) and got[1].sum() >= 256
    slots = got[0].view(np.int32)[:, :, 12]
    assert all(len(np.unique(slots[i, :got[1][i]])) == got[1][i] for i in range(len(rays)))
    _check(got, hc.hit_lists(("office", "moved"), hs, rays), 8, "moved office")
    dev.close()
    fresh.close()


# ---- beside a render ----
def test_hits_beside_a_render_on_another_stream():
    import torch

    hs = _scene("office")[0]
    dev = _device("office", None)
    rays = torch.from_numpy(qc.random_rays(hs, 2048)).cuda()
    p = hs.render_params(96, 54, 1)
    p.out_format = rtamd.RT_OUT_RGB_F64
    serial = _trace_hits(dev, rays, 8)
    again = _trace_hits(dev, rays, 8)
    assert np.array_equal(serial[0], again[0]) and np.array_equal(serial[1], again[1])   # repeatable
    frames0 = torch.zeros((20, 54, 96, 3), dtype=torch.float64, device="cuda")
    dev.launch_frames(p, [frames0[f].data_ptr() for f in range(20)])
    torch.cuda.synchronize()
    frames = torch.zeros_like(frames0)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    dev.launch_frames(p, [frames[f].data_ptr() for f in range(20)], stream=s1.cuda_stream)
    got = _trace_hits(dev, rays, 8, stream=s2.cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(serial[0], got[0]) and np.array_equal(serial[1], got[1])
    assert bool((frames == frames0).all())
    assert dev.status() == abi.RT_OK


# ---- statistics ----
def test_stats():
    lists = _lists("office", "random", 128)
    rays = _rays("office", "random", 128)
    dev = _device("office", None)
    for k in (1, 3, 8):
        rows, count, st = _trace_hits(dev, rays, k, stats=True)
        assert (st.rays, st.hits, st.watchdog) == (128, sum(min(len(h), k) for h in lists), 0)
        assert st.hits == int(count.sum())
    got, st = dev.hits(rays, 8, stats=True)
    assert st.hits == int(got["count"].sum()) and st.rays == 128


# ---- refusals ----
def test_analytic_scene_is_refused(tmp_path):
    import torch

    hs = rtamd.HostScene.load(fuzz_scenes.write_analytic(tmp_path, 3, 64, 48))
    hs.prepare()
    assert hs.raw.contents.n_spheres >= 1
    dev = rtamd.DeviceScene(hs, 0, analytic=True)
    rays = torch.from_numpy(qc.random_rays(hs, 64)).cuda()
    out = torch.full((64 * 2, 8), 7.0, dtype=torch.float64, device="cuda")
    cnt = torch.full((64,), 7, dtype=torch.int32, device="cuda")
    lib = rtamd.hip_lib()
    assert lib.rt_trace_hits(dev._h, rays.data_ptr(), 64, 2, None, out.data_ptr(), cnt.data_ptr(), None,
                             None) == abi.RT_ERR_UNSUPPORTED
    msg = lib.rt_last_error()
    assert msg.startswith(b"rt_trace_hits:") and b"analytic" in msg
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((cnt == 7).all())
    with pytest.raises(rtamd.RtError, match="analytic"):
        dev.hits(rays, 2)
    assert dev.status() == abi.RT_OK
    dev.close()


def test_scene_with_its_watchdog_word_set_is_refused_before_a_launch():
    import torch

    hs = _scene("cornell")[0]
    bad = rtamd.DeviceScene(hs, 0)
    rays = torch.from_numpy(qc.random_rays(hs, 64)).cuda()
    bad.trace(rays)   # healthy first
    assert bad.status() == abi.RT_OK
    bad.debug_corrupt_hierarchy()
    with pytest.raises(rtamd.RtError, match="watchdog"):
        bad.trace(rays, stats=True)   # rt_trace_closest trips the watchdog: the word is set
    assert bad.status() == abi.RT_ERR_HIP
    out = torch.full((64 * 2, 8), 7.0, dtype=torch.float64, device="cuda")
    cnt = torch.full((64,), 7, dtype=torch.int32, device="cuda")
    lib = rtamd.hip_lib()
    # refused before it launches: the new kernel never walks the corrupt tree, the buffers stay
    assert lib.rt_trace_hits(bad._h, rays.data_ptr(), 64, 2, None, out.data_ptr(), cnt.data_ptr(), None,
                             None) == abi.RT_ERR_HIP
    assert b"watchdog" in lib.rt_last_error()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((cnt == 7).all())
    bad.close()
    # another scene of the same process is unaffected
    assert _trace_hits(_device("cornell", None), rays, 2)[1].any()


# ---- the existing order tools ----
@pytest.mark.parametrize("k", [3, 8])
def test_ray_order_and_permute_rows_compose(k):
    import torch

    hs = _scene("office")[0]
    dev = _device("office", None)
    rays = torch.from_numpy(np.concatenate([qc.random_rays(hs, 1000), qc.vertex_rays(hs, _scene("office")[2], 500)])).cuda()
    n = rays.shape[0]
    want = dev.hits(rays, k)
    perm = dev.ray_order(rays)
    assert not bool((perm == torch.arange(n, dtype=torch.int32, device="cuda")).all())
    got = dev.hits(rtamd.permute_rows(rays, perm), k)
    count = rtamd.permute_rows(got["count"].contiguous(), perm, inverse=True)
    assert bool((count == want["count"]).all()) and int(count.sum()) > n // 4
    # the k * 64-byte rows in chunks of at most 256 bytes (rt_permute_rows' row limit)
    words = got["t"]._base.view(torch.int64).view(n, k * 8)
    back = torch.cat([rtamd.permute_rows(words[:, c:c + 32].contiguous(), perm, inverse=True)
                      for c in range(0, k * 8, 32)], dim=1)
    assert bool((back == want["t"]._base.view(torch.int64).view(n, k * 8)).all())
