"""rtamd — Python host mirror of the MI355X render path.

Thin ctypes layer over the two C-ABIs built in-tree:
  lib/librt_host.so  (include/rt_host.h)  scene load / generate, normals,
                     SoA flattening, median-split BVH  (C++)
  lib/librt_hip.so   (include/rt_hip.h)   device upload + the flattened HIP
                     render kernel for gfx950
The classes mirror the reference's host flow (Raytracer::init_cuda,
mytracer.cpp:54-60; Raytracer::compute_image_cuda, mytracer.cpp:123-159).
There is no CPU fallback: if a library is missing every call fails loudly.
"""
import ctypes as C
import os
from pathlib import Path

import numpy as np

from . import abi
from .abi import RT_OK, RT_OUT_RGB_F32, RT_OUT_RGB_F64, RT_FLAG_TRAVERSAL_STATS, RT_FLAG_WIDE_STATS, RT_FLAG_TIMELINE  # noqa: F401

PKG_ROOT = Path(__file__).resolve().parent.parent
LIB_DIR = PKG_ROOT / "lib"
HOST_LIB = LIB_DIR / "librt_host.so"
HIP_LIB = Path(os.environ.get("RTAMD_HIP_LIB", LIB_DIR / "librt_hip.so"))   # override: kernel variants
MULTI_LIB = LIB_DIR / "librt_multi.so"

_host = None
_hip = None
_multi = None


class RtError(RuntimeError):
    pass


def host_lib():
    global _host
    if _host is None:
        if not HOST_LIB.exists():
            raise RtError(f"{HOST_LIB} not built: run `make -C my-raytracer_amd` or __graft_entry__.build()")
        _host = abi.bind(C.CDLL(str(HOST_LIB)), abi.HOST_SYMBOLS)
    return _host


def _one_hip_runtime():
    """PyTorch-ROCm ships its own HIP runtime (torch/lib/libamdhip64.so).  Load it before our
    libraries so that they bind to it: a process holding both that copy and /opt/rocm's
    (ours loaded first, torch imported later) sees no devices in one of them."""
    try:
        import torch  # noqa: F401
    except ImportError:
        pass


def hip_lib():
    global _hip
    if _hip is None:
        _one_hip_runtime()
        if not HIP_LIB.exists():
            raise RtError(f"{HIP_LIB} not built: run `make -C my-raytracer_amd` or __graft_entry__.build()")
        _hip = abi.bind(C.CDLL(str(HIP_LIB)), abi.HIP_SYMBOLS, partial="RTAMD_HIP_LIB" in os.environ)
    return _hip


def multi_lib():
    """librt_multi.so (include/rt_multi.h): the single-process multi-GPU driver (RCCL)."""
    global _multi
    if _multi is None:
        if not MULTI_LIB.exists():
            raise RtError(f"{MULTI_LIB} not built: run `make -C my-raytracer_amd` or __graft_entry__.build()")
        hip_lib()   # librt_multi links librt_hip: load the same copy first
        _multi = abi.bind(C.CDLL(str(MULTI_LIB)), abi.MULTI_SYMBOLS)
    return _multi


def _check_host(rc, what):
    if rc != RT_OK:
        raise RtError(f"{what}: {host_lib().rt_host_last_error().decode()}")


def _check_hip(rc, what):
    if rc != RT_OK:
        raise RtError(f"{what}: {hip_lib().rt_last_error().decode()}")


def usable_cpus():
    """CPUs this process may run on: the affinity mask, bounded by a cgroup CPU quota (the GPU
    box grants 16 CPUs of a 256-thread host per GPU)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = Path("/sys/fs/cgroup/cpu.max").read_text().split()[:2]
        if quota != "max":
            n = min(n, max(1, int(int(quota) // int(period))))
    except (OSError, ValueError):
        pass
    return max(1, n)


_TREES = {"sah": abi.RT_TREE_SAH, "reference": abi.RT_TREE_REFERENCE, "sbvh": abi.RT_TREE_SBVH}


def upload_options(tree=None, **fields):
    """rt_upload_options with the library defaults (rt_upload_options_init), the device tree
    (None = default, or "sbvh" / "sah" / "reference") and any other fields set.  build_threads
    defaults to usable_cpus() (the library would use every hardware thread)."""
    opt = abi.UploadOptions()
    hip_lib().rt_upload_options_init(C.byref(opt))
    opt.build_threads = usable_cpus()
    if tree is not None:
        if tree not in _TREES:
            raise ValueError(f"tree must be one of {sorted(_TREES)}")
        opt.device_tree = _TREES[tree]
    names = {n for n, _ in abi.UploadOptions._fields_ if n != "reserved_"}
    for k, v in fields.items():
        if k not in names:
            raise ValueError(f"unknown upload option {k!r}")
        setattr(opt, k, v)
    return opt


def tree_report(host_scene, tree=None, **options):
    """rt_debug_tree_report of a prepared HostScene: the device hierarchy these upload options
    give (tree_opt=-1 / 0 / n, ...), built on the host only -- no GPU needed.  Returns
    abi.TreeReport (as_dict())."""
    try:
        fn = hip_lib().rt_debug_tree_report
    except AttributeError:
        raise RtError("rt_debug_tree_report: not exported by this librt_hip.so (RTAMD_HIP_LIB)") from None
    opt = upload_options(tree, **options)
    rep = abi.TreeReport()
    rc = fn(host_scene.soa, host_scene.bvh, C.byref(opt), C.byref(rep))
    if rc != RT_OK:
        raise RtError(f"rt_debug_tree_report: error {rc}")
    return rep


def clip_regions(host_scene, tree=None, **options):
    """rt_debug_clip_regions of a prepared HostScene: (clip [records, 6] float64 -- lo xyz, hi xyz of
    the region each device record was cut to, -inf / +inf where uncut --, slot [records] int32) of
    the hierarchy these upload options give, built on the host only -- no GPU needed."""
    fn = _update_fn("rt_debug_clip_regions")
    opt = upload_options(tree, **options)
    n = int(fn(host_scene.soa, host_scene.bvh, C.byref(opt), None, None, 0))
    if n < 0:
        raise RtError(f"rt_debug_clip_regions: error {n}")
    clip = np.zeros((n, 6), dtype=np.float64)
    slot = np.zeros(n, dtype=np.int32)
    got = int(fn(host_scene.soa, host_scene.bvh, C.byref(opt), clip.ctypes.data_as(C.POINTER(C.c_double)),
                 slot.ctypes.data_as(C.POINTER(C.c_int)), n))
    if got != n:
        raise RtError(f"rt_debug_clip_regions: error {got}")
    return clip, slot


def reclip_box_host(p0, p1, p2, clip):
    """rt_reclip_box_host: the fp64 box the re-clipping refit gives triangle (p0, p1, p2) in region
    clip (lo xyz, hi xyz), the device's function text run on the host.  Returns (lo, hi) float64 [3]
    arrays, or None where nothing of the triangle's bounds is left in the region."""
    fn = _update_fn("rt_reclip_box_host")
    dp = C.POINTER(C.c_double)
    a = [np.ascontiguousarray(x, dtype=np.float64).reshape(-1) for x in (p0, p1, p2, clip)]
    if [len(x) for x in a] != [3, 3, 3, 6]:
        raise ValueError("p0, p1, p2 must hold 3 numbers and clip 6")
    lo, hi = np.zeros(3), np.zeros(3)
    rc = fn(*[x.ctypes.data_as(dp) for x in a], lo.ctypes.data_as(dp), hi.ctypes.data_as(dp))
    if rc < 0:
        raise RtError(f"rt_reclip_box_host: error {rc}")
    return (lo, hi) if rc == 1 else None


def _np(ptr, count, dtype):
    if count == 0:
        return np.zeros(0, dtype=dtype)
    return np.ctypeslib.as_array(ptr, shape=(count,)).view(dtype)


class HostScene:
    """Host-resident scene (rt_host_scene*)."""

    def __init__(self, handle):
        self._h = handle

    @classmethod
    def generate(cls, kind, width=0, height=0, n_triangles=0, seed=0, max_depth=-1, detail=0):
        gp = abi.GenParams(width=width, height=height, n_triangles=n_triangles, seed=seed,
                           max_depth=max_depth, detail=detail)
        h = C.c_void_p()
        _check_host(host_lib().rt_host_generate(kind.encode(), C.byref(gp), C.byref(h)), f"generate {kind}")
        return cls(h)

    @classmethod
    def load(cls, path):
        h = C.c_void_p()
        _check_host(host_lib().rt_host_load(str(path).encode(), C.byref(h)), f"load {path}")
        return cls(h)

    @property
    def handle(self):
        if self._h is None:
            raise RtError("scene closed")
        return self._h

    def close(self):
        if self._h is not None:
            host_lib().rt_host_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def prepare(self, build_threads=0):
        """compute_normals + build_Data + BVH::initSoA; build_threads 0 = the usable CPUs."""
        secs = C.c_double(0.0)
        _check_host(host_lib().rt_host_prepare_ex(self.handle, int(build_threads), C.byref(secs)), "prepare")
        return secs.value

    def update_vertices(self, pos):
        """rt_host_update_vertices: moves the prepared scene's vertices to pos ([n_vertices, 3] float64,
        global vertex order, as soa_arrays()["vertex_pos"]) and keeps its topology: normals recomputed,
        the SoA's vertex_pos / vertex_normals / face_normals rewritten in place (face normals in the
        existing leaf order), the reference tree's boxes refitted; indices, slots and node ids stay.
        raw and an Oracle made afterwards see the moved scene.  Feeds DeviceScene.update and a fresh
        DeviceScene alike."""
        pos = np.ascontiguousarray(pos, dtype=np.float64)
        if pos.ndim != 2 or pos.shape[1] != 3:
            raise ValueError("pos must be an [n_vertices, 3] float64 array")
        _check_host(host_lib().rt_host_update_vertices(self.handle, pos.ctypes.data_as(C.POINTER(C.c_double)),
                                                       len(pos)), "update_vertices")

    def slot_triangles(self):
        """rt_host_slot_triangles: [n_triangles] int32, leaf slot -> triangle index in the original
        order (the meshes' triangles concatenated); what DeviceScene.set_triangle_order takes.  A
        copy; update_vertices does not change it."""
        p = host_lib().rt_host_slot_triangles(self.handle)
        n = self.soa.contents.n_vertex_idx // 3
        if n and not p:
            raise RtError("scene not prepared")
        return _np(p, n, np.int32).copy()

    @property
    def raw(self):
        return host_lib().rt_host_raw(self.handle)

    @property
    def soa(self):
        p = host_lib().rt_host_soa(self.handle)
        if not p:
            raise RtError("scene not prepared")
        return p

    @property
    def bvh(self):
        p = host_lib().rt_host_bvh(self.handle)
        if not p:
            raise RtError("scene not prepared")
        return p

    def soa_arrays(self):
        s = self.soa.contents
        nt = s.n_vertex_idx // 3
        return {
            "vertex_pos": _np(s.vertex_pos, 3 * s.n_vertices, np.float64).reshape(-1, 3),
            "vertex_normals": _np(s.vertex_normals, 3 * s.n_vertices, np.float64).reshape(-1, 3),
            "vertex_mesh_id": _np(s.vertex_mesh_id, s.n_vertices, np.int32),
            "face_normals": _np(s.face_normals, 3 * nt, np.float64).reshape(-1, 3),
            "vertex_idx": _np(s.vertex_idx, s.n_vertex_idx, np.int32).reshape(-1, 3),
            "texture_idx": _np(s.texture_idx, s.n_vertex_idx, np.int32).reshape(-1, 3),
        }

    def bvh_arrays(self):
        b = self.bvh.contents
        n = b.n_nodes
        return {
            "bb_min": _np(b.bb_min, 3 * n, np.float64).reshape(-1, 3),
            "bb_max": _np(b.bb_max, 3 * n, np.float64).reshape(-1, 3),
            "left_child": _np(b.left_child, n, np.int32),
            "first_tri": _np(b.first_tri, n, np.int32),
            "tri_count": _np(b.tri_count, n, np.int32),
        }

    def camera(self, width=0, height=0):
        cam = abi.Camera()
        _check_host(host_lib().rt_host_camera(self.handle, width, height, C.byref(cam)), "camera")
        return cam

    def render_params(self, width=0, height=0, spp_n=1):
        p = abi.RenderParams()
        _check_host(host_lib().rt_host_render_params(self.handle, width, height, spp_n, C.byref(p)),
                    "render_params")
        return p

    def save(self, path):
        _check_host(host_lib().rt_host_save(self.handle, str(path).encode()), f"save {path}")

    @property
    def triangle_count(self):
        return int(host_lib().rt_host_triangle_count(self.handle))

    @property
    def bvh_depth(self):
        return int(host_lib().rt_host_bvh_depth(self.handle))


class DeviceScene:
    """Scene resident on one MI355X (rt_scene*), uploaded from a prepared HostScene."""

    def __init__(self, host_scene, device=0, analytic=False, tree=None, **options):
        """analytic=True also uploads the raw scene's spheres and planes (rt_scene_set_analytic,
        CPU intersect_scene semantics); the default traces meshes only, like the reference GPU
        path (mytracer_gpu.cu:314-328).  tree: None (library default, "sbvh": SAH with
        spatial splits), "sbvh", "sah" (object splits only) or "reference" -- the device
        traversal hierarchy (pixels and ray counts do not depend on it).  options: other
        rt_upload_options fields (stack_ring=16, lds_treelet=-1 (none), sbvh_leaf_max=1, ...)."""
        self._h = C.c_void_p()
        self.device = device
        opt = upload_options(tree, **options)
        _check_hip(hip_lib().rt_scene_upload_ex(host_scene.soa, host_scene.bvh, device, C.byref(opt),
                                                C.byref(self._h)), "rt_scene_upload_ex")
        self.tree = tree
        self.analytic = False
        if analytic:
            r = host_scene.raw.contents
            self.set_analytic(r.spheres, r.n_spheres, r.planes, r.n_planes)

    def set_analytic(self, spheres, n_spheres, planes, n_planes):
        """Replaces the analytic primitives (ctypes arrays/pointers of abi.Sphere / abi.Plane)."""
        _check_hip(hip_lib().rt_scene_set_analytic(self._h, spheres, n_spheres, planes, n_planes),
                   "rt_scene_set_analytic")
        self.analytic = (n_spheres + n_planes) > 0

    def close(self):
        if self._h:
            hip_lib().rt_scene_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def device_bytes(self):
        return int(hip_lib().rt_scene_device_bytes(self._h))

    @property
    def upload_seconds(self):
        """(build_s, copy_s) of rt_scene_upload: the device layout built on the host (hierarchy,
        collapse, records), then device allocation + H2D copies (rt_scene_upload_seconds)."""
        b, c = C.c_double(), C.c_double()
        _check_hip(hip_lib().rt_scene_upload_seconds(self._h, C.byref(b), C.byref(c)), "rt_scene_upload_seconds")
        return b.value, c.value

    def update(self, host_scene, stream=None, reclip=False):
        """rt_scene_update_vertices with the three arrays of a host scene's SoA: the HostScene this
        scene was uploaded from after HostScene.update_vertices, or any prepared scene of the same
        topology and slots.  reclip: as in update_vertices."""
        s = host_scene.soa.contents
        u = abi.SceneUpdate(n_vertices=s.n_vertices, n_triangles=s.n_vertex_idx // 3, vertex_pos=s.vertex_pos,
                            vertex_normals=s.vertex_normals, face_normals=s.face_normals)
        self._update(u, stream, reclip)

    def _update(self, u, stream, reclip):
        st = C.c_void_p(stream) if stream else None
        if reclip:
            _check_hip(_update_fn("rt_scene_update_vertices_ex")(self._h, C.byref(u), abi.RT_UPDATE_RECLIP, st),
                       "rt_scene_update_vertices_ex")
        else:
            _check_hip(_update_fn("rt_scene_update_vertices")(self._h, C.byref(u), st), "rt_scene_update_vertices")

    def update_vertices(self, vertex_pos, vertex_normals, face_normals, stream=None, reclip=False):
        """Moves the scene's vertices on the device (rt_scene_update_vertices): new positions and
        vertex normals ([n_vertices, 3] float64) and face normals ([n_triangles, 3] float64, leaf
        order of the uploaded SoA) on the uploaded topology; the triangle and normal records are
        rewritten and the 4-wide hierarchy's boxes refitted by kernels on `stream` (an int pointer,
        None = the null stream).  Afterwards every launch and query returns what a fresh upload of
        the moved scene returns, bit for bit.  The arrays may be reused when the call returns.
        reclip=True (rt_scene_update_vertices_ex with RT_UPDATE_RECLIP) bounds every
        record a spatial split of the upload cut by the part of its moved triangle inside the
        record's clip region, so a default (SBVH) tree keeps its clipped leaves; on a scene without
        cut records it is the plain refit.  The first such update copies the clip table to the
        device (4 B per record + 48 B per cut record).
        Upload a scene that will move far with tree="sah": under a plain update the default SBVH's
        clipped leaf boxes become whole-triangle boxes (correct, but 29-39x slower frames on the
        office proxy).  With reclip=True the office frame stays within 1.03x of a
        fresh upload's at a displacement of 0.01 of the box diagonal and 1.5-1.8x at 0.1-0.3, where
        the refitted SAH tree can be the faster one: never update a default tree
        without it."""
        arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in (vertex_pos, vertex_normals, face_normals)]
        for a in arrs:
            if a.ndim != 2 or a.shape[1] != 3:
                raise ValueError("vertex_pos, vertex_normals and face_normals must be [n, 3] float64 arrays")
        if len(arrs[0]) != len(arrs[1]):
            raise ValueError("vertex_pos and vertex_normals differ in length")
        dp = C.POINTER(C.c_double)
        u = abi.SceneUpdate(n_vertices=len(arrs[0]), n_triangles=len(arrs[2]), vertex_pos=arrs[0].ctypes.data_as(dp),
                            vertex_normals=arrs[1].ctypes.data_as(dp), face_normals=arrs[2].ctypes.data_as(dp))
        self._update(u, stream, reclip)

    def set_triangle_order(self, order):
        """rt_scene_set_triangle_order: order[slot] = the triangle's index in the mesh's original
        order, an int32 array such as HostScene.slot_triangles().  Once per scene, before
        update_positions; device_bytes grows by 60 B per triangle + 4 B per vertex + 4."""
        order = np.ascontiguousarray(order, dtype=np.int32)
        if order.ndim != 1:
            raise ValueError("order must be a one-dimensional int32 array")
        _check_hip(_update_fn("rt_scene_set_triangle_order")(self._h, order.ctypes.data_as(C.POINTER(C.c_int)),
                                                             len(order)), "rt_scene_set_triangle_order")

    def update_positions(self, pos, stream=None, reclip=False):
        """rt_scene_update_positions: moves the scene's vertices to pos, positions alone -- the face
        and vertex normals, max|vertex| and the root box are made on the device, bit for bit what
        HostScene.update_vertices + update() give.  pos: an [n_vertices, 3] float64
        numpy array (the host path: no synchronisation, the array may be reused at once) or a
        contiguous [n_vertices, 3] float64 torch tensor on this scene's device (the device path: no
        copy through the host; the call waits for the stream once, for max|vertex| and the box).  A
        tensor on another device, another dtype or another shape raises ValueError.  With an explicit
        `stream`, torch's current stream is synchronised first: the tensor was produced there.  Needs
        set_triangle_order.  reclip: as in update_vertices."""
        on_device = hasattr(pos, "data_ptr")   # a torch tensor
        if on_device:
            import torch
            dev = torch.device(f"cuda:{self.device}")
            if not (pos.is_cuda and pos.device == dev and pos.dtype == torch.float64 and pos.dim() == 2
                    and pos.shape[1] == 3 and pos.is_contiguous()):
                raise ValueError(f"pos must be a contiguous [n_vertices, 3] float64 tensor on {dev}")
            if stream:   # pos was made on torch's current stream
                torch.cuda.current_stream(dev).synchronize()
            addr = pos.data_ptr() if pos.shape[0] else None
        else:
            pos = np.ascontiguousarray(pos, dtype=np.float64)
            if pos.ndim != 2 or pos.shape[1] != 3:
                raise ValueError("pos must be an [n_vertices, 3] float64 array")
            addr = pos.ctypes.data
        p = abi.ScenePositions(n_vertices=int(pos.shape[0]), vertex_pos=addr, on_device=int(on_device))
        _check_hip(_update_fn("rt_scene_update_positions")(self._h, C.byref(p), abi.RT_UPDATE_RECLIP if reclip else 0,
                                                           C.c_void_p(stream) if stream else None),
                   "rt_scene_update_positions")

    def debug_scene_image(self, what):
        """Test hook (rt_debug_scene_image): the device's "nodes4" ([n, 32] uint32 view of the 128-B
        nodes: lo / hi of x, y, z for 4 slots as fp32 bits, 4 refs, 4 pad words), "tris" ([n, 20]
        uint32 view of the 80-B records) or "tnorm" ([n, 12] float64) as a host array.  Synchronises."""
        kinds = {"nodes4": (abi.RT_IMAGE_NODES4, np.uint32, 32), "tris": (abi.RT_IMAGE_TRIS, np.uint32, 20),
                 "tnorm": (abi.RT_IMAGE_TNORM, np.float64, 12)}
        if what not in kinds:
            raise ValueError(f"what must be one of {sorted(kinds)}")
        code, dtype, width = kinds[what]
        fn = _update_fn("rt_debug_scene_image")
        size = int(fn(self._h, code, None, 0))
        if size < 0:
            _check_hip(size, "rt_debug_scene_image")
        out = np.zeros(size // np.dtype(dtype).itemsize, dtype=dtype)
        got = int(fn(self._h, code, out.ctypes.data_as(C.c_void_p), size))
        if got < 0:
            _check_hip(got, "rt_debug_scene_image")
        return out.reshape(-1, width)

    def launch(self, params, d_out, stats=False, stream=None):
        """Asynchronous render into a device buffer (int pointer); returns Stats if stats=True."""
        st = abi.Stats() if stats else None
        _check_hip(hip_lib().rt_launch_compute_image(self._h, C.byref(params), C.c_void_p(d_out),
                                                     C.byref(st) if st is not None else None,
                                                     C.c_void_p(stream) if stream else None),
                   "rt_launch_compute_image")
        return st

    def launch_frames(self, params, d_outs, stats=False, stream=None):
        """Asynchronous render of len(d_outs) frames in ONE launch (rt_launch_frames); params is
        one RenderParams (every frame the same) or a list of them differing only in their camera
        vectors.  Returns Stats summed over the frames if stats=True."""
        n = len(d_outs)
        plist = params if isinstance(params, (list, tuple)) else [params] * n
        if len(plist) != n:
            raise ValueError("one params per output buffer")
        parr = (abi.RenderParams * n)(*plist)
        oarr = (C.c_void_p * n)(*[C.c_void_p(d) for d in d_outs])
        st = abi.Stats() if stats else None
        _check_hip(hip_lib().rt_launch_frames(self._h, parr, n, oarr, C.byref(st) if st is not None else None,
                                              C.c_void_p(stream) if stream else None), "rt_launch_frames")
        return st

    def launch_adaptive(self, params, d_primary, d_out, subp=4, threshold=0.02, stats=False, stream=None):
        """Adaptive supersampling pass (rt_launch_adaptive) over device buffers (int pointers);
        returns (Stats or None, number of re-rendered pixels)."""
        st = abi.Stats() if stats else None
        nsel = C.c_longlong(-1)   # only requested with stats (reading it synchronises)
        _check_hip(hip_lib().rt_launch_adaptive(self._h, C.byref(params), C.c_void_p(d_primary), C.c_void_p(d_out),
                                                subp, threshold, C.byref(st) if st is not None else None,
                                                C.byref(nsel) if stats else None,
                                                C.c_void_p(stream) if stream else None),
                   "rt_launch_adaptive")
        return st, int(nsel.value)

    def launch_adaptive_frames(self, params, d_primaries, d_outs, subp=4, threshold=0.02, stats=False, stream=None):
        """Adaptive pass over len(d_outs) full frames in one render launch (rt_launch_adaptive_frames);
        params as launch_frames.  Returns (Stats or None, re-rendered pixels over all frames)."""
        n = len(d_outs)
        plist = params if isinstance(params, (list, tuple)) else [params] * n
        if len(plist) != n or len(d_primaries) != n:
            raise ValueError("one params and one primary image per output buffer")
        parr = (abi.RenderParams * n)(*plist)
        parr_p = (C.c_void_p * n)(*[C.c_void_p(d) for d in d_primaries])
        oarr = (C.c_void_p * n)(*[C.c_void_p(d) for d in d_outs])
        st = abi.Stats() if stats else None
        nsel = C.c_longlong(-1)
        _check_hip(hip_lib().rt_launch_adaptive_frames(self._h, parr, n, parr_p, oarr, subp, threshold,
                                                       C.byref(st) if st is not None else None,
                                                       C.byref(nsel) if stats else None,
                                                       C.c_void_p(stream) if stream else None),
                   "rt_launch_adaptive_frames")
        return st, int(nsel.value)

    def launch_adaptive_shard(self, params, d_primary, d_halo, d_out, subp=4, threshold=0.02, stats=False,
                              stream=None):
        """Adaptive pass over a row shard (rt_launch_adaptive_shard): d_primary / d_out are the
        shard's packed rows, d_halo the rows adaptive_halo_rows(params) lists (0: none needed)."""
        st = abi.Stats() if stats else None
        nsel = C.c_longlong(-1)
        _check_hip(hip_lib().rt_launch_adaptive_shard(self._h, C.byref(params), C.c_void_p(d_primary),
                                                      C.c_void_p(d_halo) if d_halo else None, C.c_void_p(d_out),
                                                      subp, threshold, C.byref(st) if st is not None else None,
                                                      C.byref(nsel) if stats else None,
                                                      C.c_void_p(stream) if stream else None),
                   "rt_launch_adaptive_shard")
        return st, int(nsel.value)

    def render_adaptive(self, params, subp=4, threshold=0.02):
        """Primary pass (fp64) + adaptive pass, the reference's launch_compute_image_device
        (mytracer_gpu.cu:44-113); returns (image[H, W, 3], primary Stats, adaptive Stats, n_selected)."""
        import torch

        H, W = params.camera.height, params.camera.width
        prim = torch.zeros((H, W, 3), dtype=torch.float64, device=f"cuda:{self.device}")
        dtype = torch.float64 if params.out_format == RT_OUT_RGB_F64 else torch.float32
        out = torch.zeros((H, W, 3), dtype=dtype, device=f"cuda:{self.device}")
        q = abi.RenderParams.from_buffer_copy(params)
        q.out_format = RT_OUT_RGB_F64
        st0 = self.launch(q, prim.data_ptr(), stats=True)
        st1, nsel = self.launch_adaptive(params, prim.data_ptr(), out.data_ptr(), subp, threshold, stats=True)
        return out.cpu().numpy(), st0, st1, nsel

    def render_adaptive_to_host(self, params, subp=4, threshold=0.02, out=None):
        """rt_render_adaptive_to_host: primary + adaptive pass + copy in one synchronous call (the
        reference's launch_compute_image_device); out: a host array [H, W, 3] of params.out_format
        (numpy, or a pinned torch tensor's numpy view).  Returns (image, primary Stats, adaptive
        Stats, n_selected)."""
        H, W = params.camera.height, params.camera.width
        dtype = np.float64 if params.out_format == RT_OUT_RGB_F64 else np.float32
        img = np.zeros((H, W, 3), dtype=dtype) if out is None else out
        if img.shape != (H, W, 3) or img.dtype != dtype or not img.flags["C_CONTIGUOUS"]:
            raise ValueError("out must be a C-contiguous [H, W, 3] array of the output format")
        st0, st1, nsel = abi.Stats(), abi.Stats(), C.c_longlong(-1)
        _check_hip(hip_lib().rt_render_adaptive_to_host(self._h, C.byref(params), subp, threshold,
                                                        img.ctypes.data_as(C.c_void_p), C.byref(st0), C.byref(st1),
                                                        C.byref(nsel)), "rt_render_adaptive_to_host")
        return img, st0, st1, int(nsel.value)

    def render(self, params):
        """Synchronous render to host; returns (image[rows, W, 3], Stats)."""
        rows = rows_in_shard(params)
        dtype = np.float64 if params.out_format == RT_OUT_RGB_F64 else np.float32
        img = np.zeros((rows, params.camera.width, 3), dtype=dtype)
        st = abi.Stats()
        _check_hip(hip_lib().rt_render_to_host(self._h, C.byref(params), img.ctypes.data_as(C.c_void_p),
                                               C.byref(st)), "rt_render_to_host")
        return img, st

    def bounds(self):
        """(lo, hi) of the scene's root box (rt_scene_bounds): the box ray_order's keys quantise
        origins in; zeros for a scene without triangles."""
        lo, hi = (C.c_double * 3)(), (C.c_double * 3)()
        _check_hip(_order_fn("rt_scene_bounds")(self._h, lo, hi), "rt_scene_bounds")
        return np.array(lo[:]), np.array(hi[:])

    def ray_order(self, rays, origin_bits=None, keys=False, stream=None):
        """The coherent order of the caller's rays (rt_ray_order): perm, an int32 view of the uint32
        result, with perm[j] = the index of the ray that belongs at position j -- the stable
        ascending order of the rays' coherence keys (origin cell in bounds(), then octahedral
        direction cell; origin_bits per axis 0..10, None = the library default of 5; degenerate rays
        last).  rays as for trace(); keys=True returns (perm, keys), keys[i] the key of rays[i] as an
        int32 view.  The workspace is a torch byte tensor.  Tensors in, tensors out (asynchronous on
        `stream`, an int pointer, None = the null stream); numpy in, numpy out (uint32)."""
        import torch

        fn = _order_fn("rt_ray_order")
        host_in = isinstance(rays, np.ndarray)
        dev = torch.device(f"cuda:{self.device}")
        if host_in:
            if rays.ndim != 2 or rays.shape[1] != 8:
                raise ValueError("rays must be an [n, 8] float64 array")
            rays = torch.from_numpy(np.ascontiguousarray(rays, dtype=np.float64)).to(dev)
        if not (isinstance(rays, torch.Tensor) and rays.dtype == torch.float64 and rays.dim() == 2
                and rays.shape[1] == 8 and rays.is_contiguous() and rays.device == dev):
            raise ValueError(f"rays must be a contiguous [n, 8] float64 tensor on {dev}")
        n = rays.shape[0]
        perm = torch.empty((n,), dtype=torch.int32, device=dev)
        kt = torch.empty((n,), dtype=torch.int32, device=dev) if keys else None
        work = torch.empty((order_workspace_bytes(n),), dtype=torch.uint8, device=dev)
        if stream:   # the buffers above were made on torch's current stream
            torch.cuda.current_stream(dev).synchronize()
        _check_hip(fn(self._h, C.c_void_p(rays.data_ptr() if n else None), n,
                      -1 if origin_bits is None else int(origin_bits), C.c_void_p(perm.data_ptr() if n else None),
                      C.c_void_p(kt.data_ptr() if keys and n else None), C.c_void_p(work.data_ptr() if n else None),
                      C.c_void_p(stream) if stream else None), "rt_ray_order")
        if stream:   # the workspace returns to torch's allocator with this call
            torch.cuda.ExternalStream(stream, device=dev).synchronize()
        if host_in:
            torch.cuda.synchronize(dev)
            perm = perm.cpu().numpy().view(np.uint32)
            kt = kt.cpu().numpy().view(np.uint32) if keys else None
        return (perm, kt) if keys else perm

    def _resolve_order(self, order, rays, stream):
        """trace / radiance `order` argument -> int32 perm tensor on the device."""
        import torch

        n = rays.shape[0]
        if isinstance(order, str):
            if order != "auto":
                raise ValueError('order must be None, "auto" or a permutation')
            return self.ray_order(rays, stream=stream)
        if isinstance(order, np.ndarray):
            order = np.ascontiguousarray(order).astype(np.int64).astype(np.uint32).view(np.int32)   # uint32 entries
            order = torch.from_numpy(order).to(rays.device)
        if not (isinstance(order, torch.Tensor) and order.dtype == torch.int32 and order.dim() == 1
                and order.shape[0] == n and order.is_contiguous() and order.device == rays.device):
            raise ValueError(f"order must be a contiguous int32 tensor of {n} entries on {rays.device}")
        return order

    def trace(self, rays, occluded=False, stats=False, stream=None, order=None):
        """Batched ray query (rt_trace_closest / rt_trace_occluded).  rays: [n, 8] float64 rows
        (o xyz, d xyz, tmax, reserved) -- a CUDA tensor on the scene's device, used in place, or a
        numpy array, uploaded.  Closest hits come back as a dict of views of one [n, 8] float64
        result buffer (rt_hit rows): t, alpha, beta, normal [n, 3], and slot, mesh, prim as int32;
        occluded=True returns a uint8 array instead.  Tensors in, tensors out (asynchronous on
        `stream`, an int pointer, None = the null stream, unless stats=True); numpy in, numpy out.
        stats=True returns (result, QueryStats).
        order: None traces the rays in the caller's order.  "auto" sorts them into coherent waves
        first (ray_order with the default bits), a permutation (ray_order's, or any int32 tensor /
        integer array of n entries) uses that order: the rays are gathered, traced by the same entry
        point and the result rows scattered back, so the values sit at the caller's indices and are
        bit-identical to order=None.  With an order and a stream the call returns after the stream
        has finished (the sorted copies are torch temporaries)."""
        import torch

        host_in = isinstance(rays, np.ndarray)
        dev = torch.device(f"cuda:{self.device}")
        if host_in:
            if rays.ndim != 2 or rays.shape[1] != 8:
                raise ValueError("rays must be an [n, 8] float64 array")
            rays = torch.from_numpy(np.ascontiguousarray(rays, dtype=np.float64)).to(dev)
        if not (isinstance(rays, torch.Tensor) and rays.dtype == torch.float64 and rays.dim() == 2
                and rays.shape[1] == 8 and rays.is_contiguous() and rays.device == dev):
            raise ValueError(f"rays must be a contiguous [n, 8] float64 tensor on {dev}")
        n = rays.shape[0]
        perm = None
        if order is not None:   # the rays in the order's sequence; the result rows go back below
            perm = self._resolve_order(order, rays, stream)
            rays = permute_rows(rays, perm, stream=stream)
        st = abi.QueryStats() if stats else None
        if occluded:
            out = torch.zeros((n,), dtype=torch.uint8, device=dev)
            fn, what = hip_lib().rt_trace_occluded, "rt_trace_occluded"
        else:
            out = torch.zeros((n, 8), dtype=torch.float64, device=dev)
            fn, what = hip_lib().rt_trace_closest, "rt_trace_closest"
        if stream:   # the buffers above were made on torch's current stream
            torch.cuda.current_stream(dev).synchronize()
        _check_hip(fn(self._h, C.c_void_p(rays.data_ptr() if n else None), n, C.c_void_p(out.data_ptr() if n else None),
                      C.byref(st) if st is not None else None, C.c_void_p(stream) if stream else None), what)
        if perm is not None:
            out = permute_rows(out, perm, inverse=True, stream=stream)
            if stream:   # the sorted copies return to torch's allocator with this call
                torch.cuda.ExternalStream(stream, device=dev).synchronize()
        if host_in:
            torch.cuda.synchronize(dev)
            out = out.cpu()
        if occluded:
            res = out.numpy() if host_in else out
        else:
            res = _hit_views(out)
            if host_in:
                res = {k: v.numpy() for k, v in res.items()}
        return (res, st) if stats else res

    def hits(self, rays, k, after=None, stats=False, stream=None):
        """The k nearest hits of each ray (rt_trace_hits): the ray's hit list -- every triangle it
        crosses with 1e-5 < t < tmax, each once, ascending by (t, slot) -- cut after k entries.  rays
        as for trace(): [n, 8] float64 rows, a CUDA tensor on the scene's device, used in place, or a
        numpy array, uploaded.  Returns a dict of [n, k] views (t, alpha, beta, normal [n, k, 3], and
        slot, mesh, prim as int32) over one [n, k, 8] float64 result buffer of rt_hit rows, plus
        count, an int32 [n]: the entries of a ray that are hits; the others are miss records.
        count == k means the list may go on: call again with after = the last entry's key.
        after: the resume keys, only hits with (t, slot) greater than a ray's key are listed.  Either
        a pair (t, slot) of [n] arrays or tensors (float64 and integer), or one [n] numpy array of
        rtamd.HIT_KEY_DTYPE, or one [n, 2] float64 tensor / array whose rows are rt_hit_key records
        (t, then slot and a reserved int32 sharing the second word), used in place when it is a
        contiguous tensor on the device.  (-inf, -1) constrains nothing; a NaN t lists nothing.
        Tensors in, tensors out (asynchronous on `stream`, an int pointer, None = the null stream,
        unless stats=True, or a stream together with an `after` that had to be copied); numpy in,
        numpy out.  stats=True returns (result, QueryStats).  A scene with analytic primitives is
        refused (RtError)."""
        import torch

        host_in = isinstance(rays, np.ndarray)
        rays = self._hits_rays(rays)
        n = rays.shape[0]
        keys = None if after is None else _hit_keys(after, n, rays.device)
        st = abi.QueryStats() if stats else None
        out, count = self._hits_launch(rays, k, keys, st, stream)
        if stream and keys is not None and not (isinstance(after, torch.Tensor) and after.data_ptr() == keys.data_ptr()):
            torch.cuda.ExternalStream(stream, device=rays.device).synchronize()   # the key copy is a torch temporary
        if host_in:
            torch.cuda.synchronize(rays.device)
            out, count = out.cpu(), count.cpu()
        res = _hit_views(out.view(n * int(k), 8))
        res = {name: v.view((n, int(k)) + tuple(v.shape[1:])) for name, v in res.items()}
        res["count"] = count
        if host_in:
            res = {name: v.numpy() for name, v in res.items()}
        return (res, st) if stats else res

    def _hits_rays(self, rays):
        """hits / all_hits `rays` argument -> contiguous [n, 8] float64 tensor on the device."""
        import torch

        dev = torch.device(f"cuda:{self.device}")
        if isinstance(rays, np.ndarray):
            if rays.ndim != 2 or rays.shape[1] != 8:
                raise ValueError("rays must be an [n, 8] float64 array")
            rays = torch.from_numpy(np.ascontiguousarray(rays, dtype=np.float64)).to(dev)
        if not (isinstance(rays, torch.Tensor) and rays.dtype == torch.float64 and rays.dim() == 2
                and rays.shape[1] == 8 and rays.is_contiguous() and rays.device == dev):
            raise ValueError(f"rays must be a contiguous [n, 8] float64 tensor on {dev}")
        return rays

    def _hits_launch(self, rays, k, keys, st, stream):
        """One rt_trace_hits call: (the [n, k, 8] float64 buffer of rt_hit rows, count int32 [n]).
        keys: None or an [n, 2] int64 tensor of rt_hit_key records on the device."""
        import torch

        fn = _hits_fn("rt_trace_hits")
        dev = rays.device
        n, k = rays.shape[0], int(k)
        if not 1 <= k <= abi.RT_HITS_MAX_K:
            raise ValueError("k must be in [1, RT_HITS_MAX_K]")
        if n * k > abi.RT_HITS_MAX_ROWS:
            raise ValueError("n * k exceeds RT_HITS_MAX_ROWS")
        out = torch.zeros((n, k, 8), dtype=torch.float64, device=dev)
        count = torch.zeros((n,), dtype=torch.int32, device=dev)
        if stream:   # the buffers above (and the keys) were made on torch's current stream
            torch.cuda.current_stream(dev).synchronize()
        _check_hip(fn(self._h, C.c_void_p(rays.data_ptr() if n else None), n, k,
                      C.c_void_p(keys.data_ptr() if keys is not None and n else None),
                      C.c_void_p(out.data_ptr() if n else None), C.c_void_p(count.data_ptr() if n else None),
                      C.byref(st) if st is not None else None, C.c_void_p(stream) if stream else None), "rt_trace_hits")
        return out, count

    def all_hits(self, rays, k=8):
        """Every hit of every ray (the whole hit list of hits()), by rounds of hits(k): after each
        round the rays whose count is k are compacted on the device, their resume keys taken from
        their last entry, and traced again, until none is left.  Returns a dict in CSR form:
        offsets, an int64 [n + 1] (ray i's hits are the entries offsets[i] .. offsets[i + 1]), and
        the flat arrays t, alpha, beta, normal [m, 3], slot, mesh, prim in ray order, each ray's
        ascending by (t, slot).  rays as for hits(); tensors in, tensors out (the call synchronises);
        numpy in, numpy out."""
        import torch

        host_in = isinstance(rays, np.ndarray)
        cur = self._hits_rays(rays)
        dev = cur.device
        n, k = cur.shape[0], int(k)
        live = torch.arange(n, dtype=torch.int64, device=dev)   # the rays of this round
        keys = None
        col = torch.arange(k, device=dev)[None, :]
        rows, owner = [], []   # per round: the hit rows [m, 8] and the ray each belongs to
        while live.numel() > 0:
            out, cnt = self._hits_launch(cur, k, keys, None, None)
            kept = col < cnt[:, None]
            rows.append(out[kept])   # row-major: ray by ray, entry by entry
            owner.append(live[:, None].expand(-1, k)[kept])
            more = cnt == k
            if not bool(more.any()):
                break
            # the last entry of the rays that go on: words 0 (t) and 6 (slot | mesh) are an rt_hit_key
            keys = out.view(torch.int64)[more][:, k - 1, :][:, [0, 6]].contiguous()
            cur = cur[more].contiguous()
            live = live[more]
        flat = torch.cat(rows) if rows else torch.zeros((0, 8), dtype=torch.float64, device=dev)
        own = torch.cat(owner) if owner else torch.zeros((0,), dtype=torch.int64, device=dev)
        # a ray's later rounds hold its later hits: a stable sort by ray puts the list in order
        flat = flat[torch.sort(own, stable=True).indices].contiguous()
        offsets = torch.zeros((n + 1,), dtype=torch.int64, device=dev)
        if own.numel():
            offsets[1:] = torch.cumsum(torch.bincount(own, minlength=n), 0)
        res = _hit_views(flat)
        res["offsets"] = offsets
        torch.cuda.synchronize(dev)
        if host_in:
            res = {name: v.cpu().numpy() for name, v in res.items()}
        return res

    def radiance(self, rays, params, stats=False, stream=None, order=None):
        """Colours of the caller's rays (rt_trace_radiance): what a pixel whose one primary ray is
        rays[i] would hold, shaded by the render kernel with params' lights, max_depth, background,
        ambience and out_format (params.camera is ignored).  rays as for trace(): [n, 8] float64 rows
        (o xyz, d xyz, tmax, reserved), a CUDA tensor on the scene's device, used in place, or a numpy
        array, uploaded.  Returns [n, 3] of out_format's dtype -- tensors in, tensors out
        (asynchronous on `stream`, an int pointer, None = the null stream, unless stats=True); numpy
        in, numpy out.  stats=True returns (rgb, Stats).  A wave shades 64 consecutive rays: see
        tile_major() for a camera's coherent order, and order ("auto" or a permutation, as for
        trace()) for rays without an image grid: same bits, at the caller's indices."""
        import torch

        try:   # (a partial RTAMD_HIP_LIB, built from an older source, may lack it)
            fn = hip_lib().rt_trace_radiance
        except AttributeError:
            raise RtError("rt_trace_radiance: not exported by this librt_hip.so (RTAMD_HIP_LIB)") from None
        host_in = isinstance(rays, np.ndarray)
        dev = torch.device(f"cuda:{self.device}")
        if host_in:
            if rays.ndim != 2 or rays.shape[1] != 8:
                raise ValueError("rays must be an [n, 8] float64 array")
            rays = torch.from_numpy(np.ascontiguousarray(rays, dtype=np.float64)).to(dev)
        if not (isinstance(rays, torch.Tensor) and rays.dtype == torch.float64 and rays.dim() == 2
                and rays.shape[1] == 8 and rays.is_contiguous() and rays.device == dev):
            raise ValueError(f"rays must be a contiguous [n, 8] float64 tensor on {dev}")
        n = rays.shape[0]
        perm = None
        if order is not None:   # the rays in the order's sequence; the colours go back below
            perm = self._resolve_order(order, rays, stream)
            rays = permute_rows(rays, perm, stream=stream)
        dtype = torch.float64 if params.out_format == RT_OUT_RGB_F64 else torch.float32
        out = torch.zeros((n, 3), dtype=dtype, device=dev)
        st = abi.Stats() if stats else None
        if stream:   # the buffers above were made on torch's current stream
            torch.cuda.current_stream(dev).synchronize()
        _check_hip(fn(self._h, C.byref(params), C.c_void_p(rays.data_ptr() if n else None), n,
                      C.c_void_p(out.data_ptr() if n else None), C.byref(st) if st is not None else None,
                      C.c_void_p(stream) if stream else None), "rt_trace_radiance")
        if perm is not None:
            out = permute_rows(out, perm, inverse=True, stream=stream)
            if stream:   # the sorted copies return to torch's allocator with this call
                torch.cuda.ExternalStream(stream, device=dev).synchronize()
        if host_in:
            torch.cuda.synchronize(dev)
            out = out.cpu().numpy()
        return (out, st) if stats else out

    def ao(self, points, dirs, seed=0, bias=0.0, stats=False, stream=None):
        """Occlusion fans generated on the device (rt_trace_ao): for each surface point the number
        of its k fan rays that are NOT occluded, an int32 [n] result; divide by k for the open
        fraction.  points: [n, 8] float64 rows (p xyz, normal xyz, radius as tmax, reserved) -- a
        CUDA tensor on the scene's device, used in place, or a numpy array, uploaded; see
        ao_points_from_hits.  dirs: [n_sets, k, 3] float64 local directions, z along the normal
        (ao_directions), tensor or numpy likewise.  Point i uses set hash(i ^ seed) % n_sets and
        starts its rays at p + bias * N.  The rays are those ao_rays_host writes out and each is
        decided exactly as trace(..., occluded=True) decides it.  Tensors in, tensor out
        (asynchronous on `stream`, an int pointer, None = the null stream, unless stats=True); numpy
        points in, numpy out.  stats=True returns (counts, QueryStats): rays = n k, hits = the
        occluded fan rays."""
        import torch

        fn = _ao_fn("rt_trace_ao")
        host_in = isinstance(points, np.ndarray)
        dev = torch.device(f"cuda:{self.device}")
        if host_in:
            if points.ndim != 2 or points.shape[1] != 8:
                raise ValueError("points must be an [n, 8] float64 array")
            points = torch.from_numpy(np.ascontiguousarray(points, dtype=np.float64)).to(dev)
        dirs_uploaded = isinstance(dirs, np.ndarray)
        if dirs_uploaded:
            if dirs.ndim != 3 or dirs.shape[2] != 3:
                raise ValueError("dirs must be an [n_sets, k, 3] float64 array")
            dirs = torch.from_numpy(np.ascontiguousarray(dirs, dtype=np.float64)).to(dev)
        if not (isinstance(points, torch.Tensor) and points.dtype == torch.float64 and points.dim() == 2
                and points.shape[1] == 8 and points.is_contiguous() and points.device == dev):
            raise ValueError(f"points must be a contiguous [n, 8] float64 tensor on {dev}")
        if not (isinstance(dirs, torch.Tensor) and dirs.dtype == torch.float64 and dirs.dim() == 3
                and dirs.shape[2] == 3 and dirs.is_contiguous() and dirs.device == dev):
            raise ValueError(f"dirs must be a contiguous [n_sets, k, 3] float64 tensor on {dev}")
        n = points.shape[0]
        a = abi.AoParams(k=dirs.shape[1], n_sets=dirs.shape[0], seed=int(seed) & 0xffffffff, bias=float(bias),
                         d_dirs=dirs.data_ptr() if dirs.numel() else None)
        out = torch.zeros((n,), dtype=torch.int32, device=dev)
        st = abi.QueryStats() if stats else None
        if stream:   # the buffers above were made on torch's current stream
            torch.cuda.current_stream(dev).synchronize()
        _check_hip(fn(self._h, C.c_void_p(points.data_ptr() if n else None), n, C.byref(a),
                      C.c_void_p(out.data_ptr() if n else None), C.byref(st) if st is not None else None,
                      C.c_void_p(stream) if stream else None), "rt_trace_ao")
        if stream and (host_in or dirs_uploaded):   # the uploaded copies return to torch's allocator with this call
            torch.cuda.ExternalStream(stream, device=dev).synchronize()
        if host_in:
            torch.cuda.synchronize(dev)
            out = out.cpu().numpy()
        return (out, st) if stats else out

    def gather(self, points, dirs, params, seed=0, bias=0.0, stats=False, stream=None):
        """Mean radiance of device-generated fans (rt_trace_gather): for each surface point the mean,
        over its k fan rays, of the colour radiance() returns for that ray -- each clamped to 1 per
        channel before it is added -- an [n, 3] result of params.out_format's dtype.  points, dirs,
        seed and bias are ao()'s: [n, 8] float64 point records and [n_sets, k, 3] float64 local
        directions, CUDA tensors on the scene's device, used in place, or numpy arrays, uploaded.
        params gives the lights, max_depth, background, ambience and out_format (its camera is
        ignored).  The result equals radiance(ao_rays_host(points, dirs, seed, bias), params) in
        float64, summed per point in sample order and divided by k, bit for bit.  Tensors in, tensor
        out (asynchronous on `stream`, an int pointer, None = the null stream, unless stats=True);
        numpy points in, numpy out.  stats=True returns (rgb, Stats): primary_rays = the fan rays
        traced, pixels = n."""
        import torch

        fn = _ao_fn("rt_trace_gather")
        host_in = isinstance(points, np.ndarray)
        dirs_uploaded = isinstance(dirs, np.ndarray)
        dev = torch.device(f"cuda:{self.device}")
        if host_in and (points.ndim != 2 or points.shape[1] != 8):
            raise ValueError("points must be an [n, 8] float64 array")
        if dirs_uploaded and (dirs.ndim != 3 or dirs.shape[2] != 3):
            raise ValueError("dirs must be an [n_sets, k, 3] float64 array")
        for name, x, dims, last in (("points", points, 2, 8), ("dirs", dirs, 3, 3)):
            if isinstance(x, np.ndarray):
                continue
            if not (isinstance(x, torch.Tensor) and x.dtype == torch.float64 and x.dim() == dims
                    and x.shape[-1] == last and x.is_contiguous() and x.device == dev):
                shape = "[n, 8]" if dims == 2 else "[n_sets, k, 3]"
                raise ValueError(f"{name} must be a contiguous {shape} float64 tensor on {dev}")
        if host_in:
            points = torch.from_numpy(np.ascontiguousarray(points, dtype=np.float64)).to(dev)
        if dirs_uploaded:
            dirs = torch.from_numpy(np.ascontiguousarray(dirs, dtype=np.float64)).to(dev)
        n = points.shape[0]
        a = abi.AoParams(k=dirs.shape[1], n_sets=dirs.shape[0], seed=int(seed) & 0xffffffff, bias=float(bias),
                         d_dirs=dirs.data_ptr() if dirs.numel() else None)
        dtype = torch.float64 if params.out_format == RT_OUT_RGB_F64 else torch.float32
        out = torch.zeros((n, 3), dtype=dtype, device=dev)
        st = abi.Stats() if stats else None
        if stream:   # the buffers above were made on torch's current stream
            torch.cuda.current_stream(dev).synchronize()
        _check_hip(fn(self._h, C.byref(params), C.c_void_p(points.data_ptr() if n else None), n, C.byref(a),
                      C.c_void_p(out.data_ptr() if n else None), C.byref(st) if st is not None else None,
                      C.c_void_p(stream) if stream else None), "rt_trace_gather")
        if stream and (host_in or dirs_uploaded):   # the uploaded copies return to torch's allocator with this call
            torch.cuda.ExternalStream(stream, device=dev).synchronize()
        if host_in:
            torch.cuda.synchronize(dev)
            out = out.cpu().numpy()
        return (out, st) if stats else out

    def camera(self, params, hits=True, points=False, order="row", point_tmax=float("inf"), stats=False,
               stream=None):
        """A camera's closest hits and surface points made on the device (rt_trace_camera): per pixel
        of params' shard (camera, row range, stripes; spp_n = 1) the closest hit of its primary ray
        and / or the point record ao() and gather() start from, with no ray written out.  Returns a
        dict: "hits" = the views trace() returns over one [n, 8] float64 tensor of rt_hit rows,
        "points" = an [n, 8] float64 tensor (p xyz, the normal facing the eye, point_tmax, 0; a miss
        is a degenerate point: p = eye, zero normal), n = rows_in_shard(params) * width; both stay on
        the device.  order: "row" = the frame's layout (pixel (x, local row r) at r * W + x), "tile" =
        the records of tile_major(W, rows), the coherent order for ao() / gather().  The values equal
        trace(camera_rays_host(params, order)) and surface_points_host of them bit for bit.
        Asynchronous on `stream` (an int pointer, None = the null stream) unless stats=True, which
        returns (dict, QueryStats): rays = n, hits = the pixels that hit."""
        import torch

        fn = _camera_fn("rt_trace_camera")
        if order not in _CAMERA_ORDERS:
            raise ValueError(f"order must be one of {sorted(_CAMERA_ORDERS)}")
        if not (hits or points):
            raise ValueError("nothing requested: hits and points are both False")
        dev = torch.device(f"cuda:{self.device}")
        n = rows_in_shard(params) * params.camera.width
        if not 0 <= n <= abi.RT_CAMERA_MAX_PIXELS:
            raise ValueError("the shard holds more than RT_CAMERA_MAX_PIXELS pixels")
        ht = torch.zeros((n, 8), dtype=torch.float64, device=dev) if hits else None
        pt = torch.zeros((n, 8), dtype=torch.float64, device=dev) if points else None
        out = abi.CameraOut(d_hits=ht.data_ptr() if hits else None, d_points=pt.data_ptr() if points else None,
                            order=_CAMERA_ORDERS[order], point_tmax=float(point_tmax))
        st = abi.QueryStats() if stats else None
        if stream:   # the buffers above were made on torch's current stream
            torch.cuda.current_stream(dev).synchronize()
        if n:   # (an empty row range: nothing to trace, and torch gives empty tensors no address)
            _check_hip(fn(self._h, C.byref(params), C.byref(out), C.byref(st) if st is not None else None,
                          C.c_void_p(stream) if stream else None), "rt_trace_camera")
        res = {}
        if hits:
            res["hits"] = _hit_views(ht)
        if points:
            res["points"] = pt
        return (res, st) if stats else res

    def _fan_image(self, params, radius, trace):
        """ao_image / gather_image: tile-major surface points -> trace(points) -> image order."""
        import torch

        rows, W = rows_in_shard(params), params.camera.width
        pts = self.camera(params, hits=False, points=True, order="tile", point_tmax=radius)["points"]
        vals = trace(pts)
        perm = torch.from_numpy(tile_major(W, rows)).to(vals.device)
        img = torch.zeros_like(vals)
        img[perm] = vals   # record j is pixel perm[j] of the row-major shard
        return img

    def ao_image(self, params, dirs, seed=0, bias=0.0, radius=float("inf")):
        """Ambient occlusion of a camera's view, on the device end to end: [rows, W] float64 tensor,
        the unoccluded fraction count / k of each pixel's fan in image order (row 0 at the bottom).
        The composition camera(points, order="tile", point_tmax=radius) -> ao(points, dirs, seed,
        bias) -> the values scattered back with tile_major(W, rows); a pixel that sees the
        background reports 1.  params as for camera(), dirs as for ao()."""
        import torch

        k = dirs.shape[1]
        img = self._fan_image(params, radius, lambda pts: self.ao(pts, dirs, seed=seed, bias=bias))
        return (img.to(torch.float64) / float(k)).reshape(rows_in_shard(params), params.camera.width)

    def gather_image(self, params, dirs, seed=0, bias=0.0):
        """Mean fan radiance of a camera's view: [rows, W, 3] tensor in params.out_format's dtype, the
        colour gather() returns for each pixel's surface point, in image order.  The composition
        camera(points, order="tile") -> gather(points, dirs, params, seed, bias) -> the colours
        scattered back with tile_major(W, rows); a pixel that sees the background reports it."""
        img = self._fan_image(params, float("inf"), lambda pts: self.gather(pts, dirs, params, seed=seed, bias=bias))
        return img.reshape(rows_in_shard(params), params.camera.width, 3)

    def debug_counters(self):
        """Raw counter words of the last launch (see rt_debug_counters in rt_hip.h)."""
        buf = (C.c_ulonglong * 40)()
        n = hip_lib().rt_debug_counters(self._h, buf, 40)
        if n < 0:
            _check_hip(n, "rt_debug_counters")
        names = {16: "node_iters", 17: "node_lanes", 18: "leaf_iters", 19: "leaf_lanes", 20: "trav_cycles",
                 21: "shade_cycles", 22: "fetch_cycles", 23: "outer_iters", 24: "trav_rounds", 25: "trav_round_lanes",
                 26: "stack_spills", 27: "node_lines", 28: "leaf_lines", 29: "big_leaf_tests",
                 30: "node_lds_iters", 32: "gnode_uniform_iters", 33: "gnode_distinct", 34: "leaf_uniform_iters",
                 35: "anyhit_tri_tests", 36: "anyhit_own_record_tests", 37: "shadow_rays_skipped"}
        return {v: int(buf[k]) for k, v in names.items()}

    def wave_log(self, max_waves=1 << 16):
        """Per-wave {start, last fetch, end, pixels} of the last STATS launch (rt_debug_wave_log)."""
        buf = np.zeros(4 * max_waves, dtype=np.uint64)
        n = hip_lib().rt_debug_wave_log(self._h, buf.ctypes.data_as(C.POINTER(C.c_ulonglong)), len(buf))
        if n < 0:
            _check_hip(int(n), "rt_debug_wave_log")
        return buf[:n].reshape(-1, 4)

    def timeline(self, max_waves=1 << 14):
        """Per-round records [wave, round, 4] of the last RT_FLAG_TIMELINE launch (rt_debug_timeline)."""
        buf = np.zeros(8 * 256 * max_waves, dtype=np.uint64)
        n = hip_lib().rt_debug_timeline(self._h, buf.ctypes.data_as(C.POINTER(C.c_ulonglong)), len(buf))
        if n < 0:
            _check_hip(int(n), "rt_debug_timeline")
        return buf[:n].reshape(-1, 256, 8)

    def last_kernel_ms(self):
        ms = C.c_float(0.0)
        _check_hip(hip_lib().rt_last_kernel_ms(self._h, C.byref(ms)), "rt_last_kernel_ms")
        return ms.value

    def status(self):
        """rt_scene_status: RT_OK, or RT_ERR_HIP once a finished launch tripped the kernel watchdog."""
        return int(hip_lib().rt_scene_status(self._h))

    def last_grid(self):
        """(blocks, full_blocks) of the last launch's persistent grid (rt_debug_last_grid)."""
        b, f = C.c_longlong(0), C.c_longlong(0)
        _check_hip(hip_lib().rt_debug_last_grid(self._h, C.byref(b), C.byref(f)), "rt_debug_last_grid")
        return b.value, f.value

    def debug_corrupt_hierarchy(self):
        """Test hook (rt_debug_corrupt_hierarchy): the first 4-wide node becomes a cycle."""
        _check_hip(hip_lib().rt_debug_corrupt_hierarchy(self._h), "rt_debug_corrupt_hierarchy")


def _hit_views(out):
    """The dict of views trace() returns over one [n, 8] float64 tensor of rt_hit rows."""
    import torch

    ints = out.view(torch.int32)
    return {"t": out[:, 0], "alpha": out[:, 1], "beta": out[:, 2], "normal": out[:, 3:6],
            "slot": ints[:, 12], "mesh": ints[:, 13], "prim": ints[:, 14]}


HIT_KEY_DTYPE = np.dtype([("t", "<f8"), ("slot", "<i4"), ("reserved_", "<i4")])   # abi.HitKey rows


def _hit_keys(after, n, dev):
    """hits() `after` argument -> contiguous [n, 2] int64 tensor of rt_hit_key records on dev."""
    import torch

    if isinstance(after, (tuple, list)):
        if len(after) != 2:
            raise ValueError("after must be a pair (t, slot), a HIT_KEY_DTYPE array or [n, 2] key rows")
        t, slot = after
        if isinstance(t, torch.Tensor) or isinstance(slot, torch.Tensor):
            t = torch.as_tensor(t, dtype=torch.float64, device=dev).reshape(-1).contiguous()
            slot = torch.as_tensor(slot, device=dev).reshape(-1).to(torch.int64)
            if t.shape[0] != n or slot.shape[0] != n:
                raise ValueError(f"after must hold {n} keys")
            return torch.stack([t.view(torch.int64), slot & 0xFFFFFFFF], dim=1).contiguous()
        rec = np.zeros(np.shape(t), dtype=HIT_KEY_DTYPE)
        rec["t"], rec["slot"] = t, slot
        after = rec
    if isinstance(after, np.ndarray):
        if after.dtype == HIT_KEY_DTYPE and after.shape == (n,):
            words = np.ascontiguousarray(after).view(np.int64).reshape(n, 2)
        elif after.dtype == np.float64 and after.shape == (n, 2):
            words = np.ascontiguousarray(after).view(np.int64)
        else:
            raise ValueError(f"after must be {n} keys: a HIT_KEY_DTYPE array [n] or float64 rows [n, 2]")
        return torch.from_numpy(words.copy()).to(dev)
    if (isinstance(after, torch.Tensor) and after.dtype in (torch.float64, torch.int64) and tuple(after.shape) == (n, 2)
            and after.is_contiguous() and after.device == dev):
        return after.view(torch.int64)
    raise ValueError(f"after must be {n} keys: a pair (t, slot), a HIT_KEY_DTYPE array or contiguous [n, 2] rows on {dev}")


def _hits_fn(name):
    """An entry point of the hit-list feature (a partial RTAMD_HIP_LIB, built from an older source,
    may lack it)."""
    try:
        return getattr(hip_lib(), name)
    except AttributeError:
        raise RtError(f"{name}: not exported by this librt_hip.so (RTAMD_HIP_LIB)") from None


def _update_fn(name):
    """An entry point of the vertex-update feature (a partial RTAMD_HIP_LIB, built from an older
    source, may lack it)."""
    try:
        return getattr(hip_lib(), name)
    except AttributeError:
        raise RtError(f"{name}: not exported by this librt_hip.so (RTAMD_HIP_LIB)") from None


def _order_fn(name):
    """An entry point of the ray-order feature (a partial RTAMD_HIP_LIB, built from an older source,
    may lack it)."""
    try:
        return getattr(hip_lib(), name)
    except AttributeError:
        raise RtError(f"{name}: not exported by this librt_hip.so (RTAMD_HIP_LIB)") from None


def order_workspace_bytes(n):
    """Bytes of workspace rt_ray_order needs for n rays (rt_ray_order_workspace_bytes)."""
    return int(_order_fn("rt_ray_order_workspace_bytes")(int(n)))


def ray_keys_host(lo, hi, rays, origin_bits=None):
    """The coherence keys of host rays ([n, 8] float64) in box [lo, hi], computed on the CPU by the
    function the device runs (rt_ray_keys_host): uint32 [n]."""
    rays = np.ascontiguousarray(rays, dtype=np.float64)
    if rays.ndim != 2 or rays.shape[1] != 8:
        raise ValueError("rays must be an [n, 8] float64 array")
    keys = np.zeros(len(rays), dtype=np.uint32)
    lo_c, hi_c = (C.c_double * 3)(*[float(x) for x in lo]), (C.c_double * 3)(*[float(x) for x in hi])
    _check_hip(_order_fn("rt_ray_keys_host")(lo_c, hi_c, rays.ctypes.data_as(C.c_void_p), len(rays),
                                             -1 if origin_bits is None else int(origin_bits),
                                             keys.ctypes.data_as(C.POINTER(C.c_uint))), "rt_ray_keys_host")
    return keys


def permute_rows(src, perm, inverse=False, stream=None):
    """Rows of a contiguous 1-D or 2-D CUDA tensor moved by a permutation (rt_permute_rows): a new
    tensor dst with dst[j] = src[perm[j]], or with inverse=True dst[perm[j]] = src[j].  perm: a
    contiguous int32 tensor (the uint32 entries of DeviceScene.ray_order) of src.shape[0] entries on
    src's device; an entry >= n is skipped (its dst row stays zero).  A row is the bytes of src's
    row stride, 1..256.  Asynchronous on `stream` (an int pointer, None = the null stream)."""
    import torch

    fn = _order_fn("rt_permute_rows")
    if not (isinstance(src, torch.Tensor) and src.is_cuda and src.dim() in (1, 2) and src.is_contiguous()):
        raise ValueError("src must be a contiguous 1-D or 2-D CUDA tensor")
    n = src.shape[0]
    if not (isinstance(perm, torch.Tensor) and perm.dtype == torch.int32 and perm.dim() == 1 and perm.shape[0] == n
            and perm.is_contiguous() and perm.device == src.device):
        raise ValueError(f"perm must be a contiguous int32 tensor of {n} entries on {src.device}")
    row_bytes = (src.shape[1] if src.dim() == 2 else 1) * src.element_size()   # contiguous: the row stride
    dst = torch.zeros_like(src)
    if stream:   # dst was made on torch's current stream
        torch.cuda.current_stream(src.device).synchronize()
    _check_hip(fn(C.c_void_p(src.data_ptr() if n else None), C.c_void_p(dst.data_ptr() if n else None),
                  C.c_void_p(perm.data_ptr() if n else None), n, int(row_bytes), 1 if inverse else 0,
                  src.device.index or 0, C.c_void_p(stream) if stream else None), "rt_permute_rows")
    return dst


def _ao_fn(name):
    """An entry point of the occlusion-fan feature (a partial RTAMD_HIP_LIB, built from an older
    source, may lack it)."""
    try:
        return getattr(hip_lib(), name)
    except AttributeError:
        raise RtError(f"{name}: not exported by this librt_hip.so (RTAMD_HIP_LIB)") from None


def ao_rays_host(points, dirs, seed=0, bias=0.0):
    """The fan rays DeviceScene.ao traces, written out on the CPU by the function the device runs
    (rt_ao_rays_host): points [n, 8] and dirs [n_sets, k, 3] float64 numpy arrays -> [n * k, 8] rays
    for DeviceScene.trace, ray i * k + s = sample s of point i."""
    fn = _ao_fn("rt_ao_rays_host")
    points = np.ascontiguousarray(points, dtype=np.float64)
    dirs = np.ascontiguousarray(dirs, dtype=np.float64)
    if points.ndim != 2 or points.shape[1] != 8:
        raise ValueError("points must be an [n, 8] float64 array")
    if dirs.ndim != 3 or dirs.shape[2] != 3:
        raise ValueError("dirs must be an [n_sets, k, 3] float64 array")
    n, k = len(points), dirs.shape[1]
    rays = np.zeros((n * k, 8), dtype=np.float64)
    a = abi.AoParams(k=k, n_sets=dirs.shape[0], seed=int(seed) & 0xffffffff, bias=float(bias),
                     d_dirs=dirs.ctypes.data if dirs.size else None)
    _check_hip(fn(points.ctypes.data_as(C.c_void_p) if n else None, n, C.byref(a),
                  rays.ctypes.data_as(C.c_void_p) if n * k else None), "rt_ao_rays_host")
    return rays


def ao_directions(k, n_sets, seed=0, cosine=True):
    """Direction sets for DeviceScene.ao: [n_sets, k, 3] float64 unit vectors of the hemisphere
    z > 0, made on the host.  Each set holds k stratified samples -- sample j has its first
    coordinate in stratum j of k and its second in a stratum drawn by a random permutation (one
    sample per row and per column of the k x k grid) -- mapped cosine-weighted (density cos / pi:
    the mean of the unoccluded fraction is then the ambient-occlusion integral) or, with
    cosine=False, uniformly over the hemisphere (sky-view factor), and each set is rotated about z
    by its own random angle."""
    k, n_sets = int(k), int(n_sets)
    if not (1 <= k <= abi.RT_AO_MAX_SAMPLES and 1 <= n_sets <= abi.RT_AO_MAX_SETS):
        raise ValueError("k must be in [1, RT_AO_MAX_SAMPLES] and n_sets in [1, RT_AO_MAX_SETS]")
    rng = np.random.default_rng(seed)
    j = np.arange(k, dtype=np.float64)[None, :]
    u = (j + rng.random((n_sets, k))) / k                                        # in [0, 1)
    v = (rng.permuted(np.tile(np.arange(k, dtype=np.float64), (n_sets, 1)), axis=1) + rng.random((n_sets, k))) / k
    phi = 2.0 * np.pi * (v + rng.random((n_sets, 1)))                            # the set's own rotation
    if cosine:
        z = np.sqrt(1.0 - u)
        r = np.sqrt(u)
    else:
        z = 1.0 - u
        r = np.sqrt(np.maximum(0.0, 1.0 - z * z))
    d = np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=2)
    d[..., 2] = np.maximum(d[..., 2], 1e-9)                                       # z > 0 after rounding
    return np.ascontiguousarray(d / np.sqrt((d * d).sum(axis=2, keepdims=True)))


def ao_points_from_hits(rays, hits):
    """Point records for DeviceScene.ao from the closest hits of rays, on the device: rays [n, 8]
    float64 CUDA tensor, hits the dict DeviceScene.trace returned for it.  p = o + t * normalize(d),
    the normal is the hit's, flipped to face the ray's origin, tmax = +inf (set column 6 for a finite
    radius).  A ray that missed becomes a degenerate point (p = o, zero normal): it reports k."""
    import torch

    if not (isinstance(rays, torch.Tensor) and rays.is_cuda and rays.dtype == torch.float64 and rays.dim() == 2
            and rays.shape[1] == 8):
        raise ValueError("rays must be an [n, 8] float64 CUDA tensor")
    t, nrm = hits["t"], hits["normal"]
    hit = torch.isfinite(t)
    d = rays[:, 3:6]
    dn = d / torch.sqrt((d * d).sum(dim=1, keepdim=True))
    p = rays[:, 0:3] + torch.where(hit, t, torch.zeros_like(t))[:, None] * torch.where(hit[:, None], dn, torch.zeros_like(dn))
    facing = (nrm * d).sum(dim=1, keepdim=True) > 0.0
    nrm = torch.where(facing, -nrm, nrm)
    pts = torch.zeros_like(rays)
    pts[:, 0:3] = torch.where(hit[:, None], p, rays[:, 0:3])
    pts[:, 3:6] = torch.where(hit[:, None], nrm, torch.zeros_like(nrm))
    pts[:, 6] = float("inf")
    return pts


_CAMERA_ORDERS = {"row": abi.RT_CAMERA_ROW_MAJOR, "tile": abi.RT_CAMERA_TILE_MAJOR}


def _camera_fn(name):
    """An entry point of the camera feature (a partial RTAMD_HIP_LIB, built from an older source,
    may lack it)."""
    try:
        return getattr(hip_lib(), name)
    except AttributeError:
        raise RtError(f"{name}: not exported by this librt_hip.so (RTAMD_HIP_LIB)") from None


def camera_rays_host(params, order="row"):
    """The primary rays DeviceScene.camera traces, written out on the CPU by the function the device
    runs (rt_camera_rays_host): [n, 8] float64 rays (o = eye, d unnormalised, tmax = inf, 0) of
    params' shard -- its row range or stripes -- n = rows_in_shard(params) * width, in order "row"
    (pixel (x, local row r) at r * W + x) or "tile" (the records of tile_major(W, rows))."""
    fn = _camera_fn("rt_camera_rays_host")
    if order not in _CAMERA_ORDERS:
        raise ValueError(f"order must be one of {sorted(_CAMERA_ORDERS)}")
    n = rows_in_shard(params) * params.camera.width
    if not 0 <= n <= abi.RT_CAMERA_MAX_PIXELS:
        raise ValueError("the shard holds more than RT_CAMERA_MAX_PIXELS pixels")
    rays = np.zeros((n, 8), dtype=np.float64)
    _check_hip(fn(C.byref(params), _CAMERA_ORDERS[order], rays.ctypes.data_as(C.c_void_p) if n else None),
               "rt_camera_rays_host")
    return rays


def surface_points_host(rays, hits_rows, point_tmax=float("inf")):
    """The point records DeviceScene.camera writes, made on the CPU by the function the device runs
    (rt_surface_points_host): rays [n, 8] float64 and hits_rows [n, 8] float64 rt_hit rows (the
    buffer behind trace()'s views; only t and the normal are read) -> [n, 8] float64 point records
    (p = o + t * normalize(d), the normal facing the ray's origin, point_tmax, 0); a miss (t = inf)
    gives the degenerate point (o, zero normal)."""
    fn = _camera_fn("rt_surface_points_host")
    rays = np.ascontiguousarray(rays, dtype=np.float64)
    hits_rows = np.ascontiguousarray(hits_rows, dtype=np.float64)
    if rays.ndim != 2 or rays.shape[1] != 8:
        raise ValueError("rays must be an [n, 8] float64 array")
    if hits_rows.shape != rays.shape:
        raise ValueError("hits_rows must be an [n, 8] float64 array of rt_hit rows, one per ray")
    n = len(rays)
    pts = np.zeros((n, 8), dtype=np.float64)
    _check_hip(fn(rays.ctypes.data_as(C.c_void_p) if n else None, hits_rows.ctypes.data_as(C.c_void_p) if n else None,
                  n, float(point_tmax), pts.ctypes.data_as(C.c_void_p) if n else None), "rt_surface_points_host")
    return pts


def tile_shape():
    """(width, height) of the render kernel's work tile (rt_tile_shape)."""
    w, h = C.c_int(0), C.c_int(0)
    _check_hip(hip_lib().rt_tile_shape(C.byref(w), C.byref(h)), "rt_tile_shape")
    return w.value, h.value


def ipc_handle(d_ptr):
    """(handle bytes, offset) exporting the device allocation that holds d_ptr to other
    processes (rt_ipc_get_handle)."""
    h = C.create_string_buffer(abi.RT_IPC_HANDLE_BYTES)
    off = C.c_ulonglong(0)
    _check_hip(hip_lib().rt_ipc_get_handle(C.c_void_p(d_ptr), h, C.byref(off)), "rt_ipc_get_handle")
    return h.raw, off.value


def ipc_open(handle, offset, device, owner_device=-1):
    """Device pointer in this process (device `device` current) to the bytes another process
    exported with ipc_handle from its device `owner_device` (this process's numbering; -1 =
    unknown), with peer access from device to owner enabled (rt_ipc_open)."""
    if len(handle) != abi.RT_IPC_HANDLE_BYTES:
        raise ValueError("IPC handle must be RT_IPC_HANDLE_BYTES bytes")
    p = C.c_void_p(0)
    _check_hip(hip_lib().rt_ipc_open(handle, C.c_ulonglong(offset), int(device), int(owner_device), C.byref(p)),
               "rt_ipc_open")
    return int(p.value)


def ipc_close(d_ptr, offset):
    _check_hip(hip_lib().rt_ipc_close(C.c_void_p(d_ptr), C.c_ulonglong(offset)), "rt_ipc_close")


def rows_in_shard(params):
    return int(hip_lib().rt_rows_in_shard(C.byref(params)))


def adaptive_halo_rows(params):
    """Global rows rt_launch_adaptive_shard's halo must hold ([2s] below / [2s+1] above
    segment s; -1 = outside the frame), from the library itself (no GPU needed)."""
    n = int(hip_lib().rt_adaptive_halo_rows(C.byref(params), None, 0))
    _check_hip(min(n, 0), "rt_adaptive_halo_rows")
    buf = (C.c_int * max(1, n))()
    _check_hip(min(0, int(hip_lib().rt_adaptive_halo_rows(C.byref(params), buf, n))), "rt_adaptive_halo_rows")
    return np.array(buf[:n], dtype=np.int64)


def shard_rows(height, stripe_height, stripe_count, stripe_index):
    """Global row ids a shard renders, in output order (rt_render_params rules)."""
    y = np.arange(height)
    return y[(y // stripe_height) % stripe_count == stripe_index]


def camera_rays(params):
    """The primary rays of params.camera as [H * W, 8] float64 rows for DeviceScene.trace
    (o = eye, d, tmax = inf, reserved 0), row-major with row 0 at the bottom (pixel (x, y) at row
    y * W + x).  The direction is evaluated in the renderer's order,
    ((lower_left + x * x_dir) + y * y_dir) - eye, and left unnormalised (the query normalises)."""
    cam = params.camera
    W, H = cam.width, cam.height
    eye, ll = np.array(cam.eye[:]), np.array(cam.lower_left[:])
    xd, yd = np.array(cam.x_dir[:]), np.array(cam.y_dir[:])
    x = np.arange(W, dtype=np.float64)[None, :, None]
    y = np.arange(H, dtype=np.float64)[:, None, None]
    d = ((ll + x * xd) + y * yd) - eye
    rays = np.zeros((H * W, 8))
    rays[:, 0:3] = eye
    rays[:, 3:6] = d.reshape(-1, 3)
    rays[:, 6] = np.inf
    return rays


def panorama_rays(params, width, height):
    """Rays of an equirectangular 360 x 180 degree camera at params.camera.eye for
    DeviceScene.radiance / trace: [height * width, 8] float64 rows (o = eye, d, tmax = inf, reserved
    0), row-major with row 0 at the bottom.  Pixel (x, y) looks along
    d = cos(theta) sin(phi) right + sin(theta) up + cos(theta) cos(phi) forward with
    phi = 2 pi (x + 0.5) / width - pi and theta = pi (y + 0.5) / height - pi / 2, where right and up
    are the normalised x_dir and y_dir and forward is the normalised vector from the eye to the
    image centre, lower_left + W/2 x_dir + H/2 y_dir - eye (W, H the camera's own size)."""
    cam = params.camera
    eye, ll = np.array(cam.eye[:]), np.array(cam.lower_left[:])
    xd, yd = np.array(cam.x_dir[:]), np.array(cam.y_dir[:])
    fwd = ll + 0.5 * cam.width * xd + 0.5 * cam.height * yd - eye
    right, up, fwd = xd / np.linalg.norm(xd), yd / np.linalg.norm(yd), fwd / np.linalg.norm(fwd)
    phi = (2.0 * np.pi * (np.arange(width) + 0.5) / width - np.pi)[None, :, None]
    theta = (np.pi * (np.arange(height) + 0.5) / height - 0.5 * np.pi)[:, None, None]
    d = np.cos(theta) * np.sin(phi) * right + np.sin(theta) * up + np.cos(theta) * np.cos(phi) * fwd
    rays = np.zeros((height * width, 8))
    rays[:, 0:3] = eye
    rays[:, 3:6] = d.reshape(-1, 3)
    rays[:, 6] = np.inf
    return rays


def tile_major(width, height):
    """Permutation of range(height * width) that puts the rows of a row-major [height * width, ...]
    array into the render kernel's tile order (rt_tile_shape: 8 x 8): tiles row by row from the
    bottom-left one, a tile's pixels row-major and consecutive; the partial tiles at the right and
    top edges hold the pixels they have.  rays[perm] is then coherent per wave of 64 for
    DeviceScene.radiance / trace, and with inv = np.argsort(perm), rgb[inv] restores image order."""
    tw, th = tile_shape()
    ys, xs = np.meshgrid(np.arange(height), np.arange(width), indexing="ij")
    key = ((ys // th) * ((width + tw - 1) // tw) + xs // tw) * (tw * th) + (ys % th) * tw + xs % tw
    return np.argsort(key.ravel(), kind="stable")


def camera_orbit(params, angle):
    """Copy of params whose camera is turned rigidly by `angle` radians about the image's
    vertical axis (y_dir) through the point the image centre looks at (lower_left +
    W/2 x_dir + H/2 y_dir): eye, lower_left, x_dir and y_dir rotate together, so every frame
    is a valid pinhole camera of the same scene.  Frames of an animation path for
    rt_launch_frames, which lets frames differ only in these four vectors."""
    q = abi.RenderParams.from_buffer_copy(params)
    cam = q.camera
    eye, ll = np.array(cam.eye[:]), np.array(cam.lower_left[:])
    xd, yd = np.array(cam.x_dir[:]), np.array(cam.y_dir[:])
    c = ll + 0.5 * cam.width * xd + 0.5 * cam.height * yd
    k = yd / np.linalg.norm(yd)
    kx = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    R = np.eye(3) + np.sin(angle) * kx + (1.0 - np.cos(angle)) * (kx @ kx)   # Rodrigues
    for name, v in (("eye", c + R @ (eye - c)), ("lower_left", c + R @ (ll - c)), ("x_dir", R @ xd),
                    ("y_dir", R @ yd)):
        getattr(cam, name)[:] = [float(x) for x in v]
    return q


def write_ppm(path, img):
    img = np.ascontiguousarray(img, dtype=np.float32)
    h, w, _ = img.shape
    _check_host(host_lib().rt_write_ppm(str(path).encode(), img.ctypes.data_as(C.POINTER(C.c_float)), w, h),
                "rt_write_ppm")


class MultiScene:
    """One scene on several GPUs of this node, one process (rt_multi.h): every frame is cut
    into interleaved row stripes per GPU and assembled on devices[0] by one RCCL gather
    (assembly="gather") or by every GPU storing its rows into devices[0]'s frames ("peer")."""

    def __init__(self, host_scene, devices=(0,), tree=None, assembly="gather", **options):
        self._h = C.c_void_p()
        devs = (C.c_int * len(devices))(*devices)
        opt = upload_options(tree, **options)
        rc = multi_lib().rt_multi_create(host_scene.soa, host_scene.bvh, devs, len(devices), C.byref(opt),
                                         C.byref(self._h))
        if rc != RT_OK:
            raise RtError(f"rt_multi_create: {multi_lib().rt_multi_last_error().decode()}")
        self.devices = tuple(devices)
        modes = {"gather": abi.RT_MULTI_GATHER, "peer": abi.RT_MULTI_PEER}
        if assembly not in modes:
            self.close()
            raise ValueError(f"assembly must be one of {sorted(modes)}")
        if multi_lib().rt_multi_set_assembly(self._h, modes[assembly]) != RT_OK:
            err = multi_lib().rt_multi_last_error().decode()
            self.close()
            raise RtError(f"rt_multi_set_assembly: {err}")
        self.assembly = assembly

    @property
    def assembly_in_use(self):
        """"gather" or "peer": the assembly rt_multi_render* use now (the peer guard falls back to
        the gather when the peer stores did not assemble a bit-identical check frame)."""
        a = multi_lib().rt_multi_assembly(self._h)
        if a < 0:
            raise RtError(f"rt_multi_assembly: {multi_lib().rt_multi_last_error().decode()}")
        return "peer" if a == abi.RT_MULTI_PEER else "gather"

    def debug_inject(self, what):
        """Test hook (rt_multi_debug_inject): abi.RT_MULTI_DEBUG_PEER_MISMATCH, or 0."""
        if multi_lib().rt_multi_debug_inject(self._h, int(what)) != RT_OK:
            raise RtError(f"rt_multi_debug_inject: {multi_lib().rt_multi_last_error().decode()}")

    def render(self, params, stripe_height=16):
        """Synchronous render of the whole frame to host memory -> (image [H, W, 3], Stats, ms)."""
        dt = np.float64 if params.out_format == RT_OUT_RGB_F64 else np.float32
        img = np.zeros((params.camera.height, params.camera.width, 3), dtype=dt)
        st, ms = abi.Stats(), C.c_double()
        rc = multi_lib().rt_multi_render_to_host(self._h, C.byref(params), stripe_height, img.ctypes.data_as(C.c_void_p),
                                                 C.byref(st), C.byref(ms))
        if rc != RT_OK:
            raise RtError(f"rt_multi_render: {multi_lib().rt_multi_last_error().decode()}")
        return img, st, ms.value

    def render_frames(self, params, d_outs, stripe_height=16, stats=False):
        """Renders len(d_outs) frames into device buffers on devices[0] (int pointers) with
        rt_multi_render_frames (batched launches, two batches in flight); params: one
        RenderParams or one per frame.  Returns (Stats or None, wall ms)."""
        n = len(d_outs)
        plist = params if isinstance(params, (list, tuple)) else [params] * n
        if len(plist) != n:
            raise ValueError("one params per output buffer")
        parr = (abi.RenderParams * n)(*plist)
        oarr = (C.c_void_p * n)(*[C.c_void_p(d) for d in d_outs])
        st, ms = (abi.Stats() if stats else None), C.c_double()
        rc = multi_lib().rt_multi_render_frames(self._h, parr, n, stripe_height, oarr,
                                                C.byref(st) if st is not None else None, C.byref(ms))
        if rc != RT_OK:
            raise RtError(f"rt_multi_render_frames: {multi_lib().rt_multi_last_error().decode()}")
        return st, ms.value

    def close(self):
        if self._h:
            multi_lib().rt_multi_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def multi_interleave_frames_host(gathered, height, stripe_height, n):
    """Host restatement of rt_multi's batched assembly: gathered [n, frames, max_rows, W, C] ->
    [frames, H, W, C]."""
    g = np.ascontiguousarray(gathered)
    nf = g.shape[1]
    out = np.empty((nf, height) + g.shape[3:], dtype=g.dtype)
    ptrs = (C.c_void_p * nf)(*[C.c_void_p(out[f].ctypes.data) for f in range(nf)])
    rc = multi_lib().rt_multi_interleave_frames_host(g.ctypes.data_as(C.c_void_p), ptrs, nf, height, g.shape[3],
                                                     g.shape[4], g.itemsize, stripe_height, n)
    if rc != RT_OK:
        raise RtError(f"rt_multi_interleave_frames_host: {multi_lib().rt_multi_last_error().decode()}")
    return out


def multi_interleave_host(gathered, height, stripe_height, n):
    """Host restatement of rt_multi's frame assembly: gathered [n, max_rows, W, C] -> [H, W, C]."""
    g = np.ascontiguousarray(gathered)
    out = np.empty((height,) + g.shape[2:], dtype=g.dtype)
    rc = multi_lib().rt_multi_interleave_host(g.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), height,
                                              g.shape[2], g.shape[3], g.itemsize, stripe_height, n)
    if rc != RT_OK:
        raise RtError(f"rt_multi_interleave_host: {multi_lib().rt_multi_last_error().decode()}")
    return out


class Raytracer:
    """Mirror of the reference's Raytracer host flow on the MI355X path."""

    def __init__(self, scene="office", device=0, **gen):
        if str(scene).endswith(".sce") or os.path.sep in str(scene):
            self.host = HostScene.load(scene)
        else:
            self.host = HostScene.generate(scene, **gen)
        self.build_seconds = self.host.prepare()
        self.gpu = DeviceScene(self.host, device)

    def compute_image(self, width=0, height=0, spp_n=1, out_format=RT_OUT_RGB_F32):
        p = self.host.render_params(width, height, spp_n)
        p.out_format = out_format
        return self.gpu.render(p)
