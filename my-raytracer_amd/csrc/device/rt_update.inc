// rt_update.inc — moving a device scene's vertices: rt_scene_update_vertices(_ex), rt_debug_scene_image
// (include/rt_hip.h; DESIGN.md §24, §25).  Included by rt_render.hip.
//
// The topology stays: vertex ids, slots, child references and the records' order are the upload's.
// update_records_kernel rewrites every triangle record and its normals from the new arrays;
// refit_nodes4_kernel recomputes the fp32 boxes of the 4-wide nodes bottom-up, one launch per height
// of the tree (leaf-only nodes first), in stream order: no spin-wait, no grid barrier.  The closest
// hit is the smallest (t, slot) over a conservative superset of candidates (DESIGN.md §4), so pixels
// and ray counts equal those of a fresh upload of the moved scene, whatever hierarchy that builds.
//
// The per-thread bodies are __host__ __device__ functions over plain pointers, so a stand-alone
// host program can run the same text on a SceneImage (define RT_UPDATE_KERNELS_ONLY and include
// rt_layout.hpp, rt_refit.hpp and rt_reclip.hpp first).

namespace {

constexpr int kUpdBlock = 256;
typedef unsigned int upd_u32x4 __attribute__((ext_vector_type(4)));
struct UpdD2 { double a, b; };

__host__ __device__ inline upd_u32x4 upd_pack(double a, double b) {
  return __builtin_bit_cast(upd_u32x4, UpdD2{a, b});
}

// Record g: e1, e2, p2 from the record's three vertices (ids from shade[g]), mesh and meta as they
// are, in five 16-B stores; tnorm[g] = the slot's face normal and the three vertex normals, in six.
__host__ __device__ inline void update_record_body(long long g, GTri* tris, const TriShade* shade, double* tnorm,
                                                   const double* vpos, const double* vnorm, const double* fnorm) {
  const TriShade sh = shade[g];
  const int32_t mesh = tris[g].mesh;
  const uint32_t meta = tris[g].meta;
  const size_t slot = meta & kSlotMask;
  const double* p0 = vpos + 3 * (size_t)sh.v[0];
  const double* p1 = vpos + 3 * (size_t)sh.v[1];
  const double* p2 = vpos + 3 * (size_t)sh.v[2];
  double e1[3], e2[3], q2[3];
  rt_refit_record(p0, p1, p2, e1, e2, q2);
  upd_u32x4* T = reinterpret_cast<upd_u32x4*>(tris + g);
  T[0] = upd_pack(e1[0], e1[1]);
  T[1] = upd_pack(e1[2], e2[0]);
  T[2] = upd_pack(e2[1], e2[2]);
  T[3] = upd_pack(q2[0], q2[1]);
  upd_u32x4 last = upd_pack(q2[2], 0.0);
  last.z = (uint32_t)mesh;
  last.w = meta;
  T[4] = last;
  const double* n0 = vnorm + 3 * (size_t)sh.v[0];
  const double* n1 = vnorm + 3 * (size_t)sh.v[1];
  const double* n2 = vnorm + 3 * (size_t)sh.v[2];
  const double* f = fnorm + 3 * slot;
  upd_u32x4* N = reinterpret_cast<upd_u32x4*>(tnorm + 12 * (size_t)g);
  N[0] = upd_pack(f[0], f[1]);
  N[1] = upd_pack(f[2], n0[0]);
  N[2] = upd_pack(n0[1], n0[2]);
  N[3] = upd_pack(n1[0], n1[1]);
  N[4] = upd_pack(n1[2], n2[0]);
  N[5] = upd_pack(n2[1], n2[2]);
}

// Slot `slot` of node `node`.  A leaf slot: the fp64 min / max over the vertices of its records,
// first .. the one flagged kLastDev, read from the position array (p2 + e1 is not exact), grown by
// delta and rounded outward.  An internal slot: the fp32 union of the child node's four slots, which
// an earlier launch wrote.  An empty slot keeps [+inf, -inf].  Refs and pad are never written.
__host__ __device__ inline void refit_slot_body(uint32_t node, int slot, GNode4* nodes4, uint32_t n_nodes,
                                                const GTri* tris, const TriShade* shade, long long n_rec,
                                                const double* vpos, double delta) {
  GNode4& N = nodes4[node];
  const uint32_t ref = N.ref[slot];
  if (ref == kEmpty) return;
  float flo[3], fhi[3];
  if (ref & kLeaf) {
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (long long g = (long long)(ref & ~kLeaf); g < n_rec; ++g) {
      const TriShade sh = shade[g];
      for (int c = 0; c < 3; ++c) rt_refit_grow(lo, hi, vpos + 3 * (size_t)sh.v[c]);
      if (tris[g].meta & kLastDev) break;
    }
    rt_refit_leaf_box(lo, hi, delta, flo, fhi);
  } else {
    if (ref >= n_nodes) return;   // (no such reference in a layout build_image made)
    const GNode4& Cn = nodes4[ref];
    rt_refit_union4(Cn.lox, Cn.hix, &flo[0], &fhi[0]);
    rt_refit_union4(Cn.loy, Cn.hiy, &flo[1], &fhi[1]);
    rt_refit_union4(Cn.loz, Cn.hiz, &flo[2], &fhi[2]);
  }
  N.lox[slot] = flo[0]; N.hix[slot] = fhi[0];
  N.loy[slot] = flo[1]; N.hiy[slot] = fhi[1];
  N.loz[slot] = flo[2]; N.hiz[slot] = fhi[2];
}

// refit_slot_body with the leaf slots re-clipped (RT_UPDATE_RECLIP, DESIGN.md §25): a record whose
// clip_idx is >= 0 grows the slot's fp64 box by rt_reclip_box of its moved triangle in region
// clip_box[6 * clip_idx ..], by nothing where that is empty; an uncut record by its three vertices.
// A leaf slot whose records all came out empty gets [+inf, -inf], the box of an absent child, which
// every slab test misses, and keeps its ref.  Internal slots as in refit_slot_body.
__host__ __device__ inline void reclip_slot_body(uint32_t node, int slot, GNode4* nodes4, uint32_t n_nodes,
                                                 const GTri* tris, const TriShade* shade, long long n_rec,
                                                 const double* vpos, double delta, const int32_t* clip_idx,
                                                 const double* clip_box) {
  GNode4& N = nodes4[node];
  const uint32_t ref = N.ref[slot];
  if (ref == kEmpty) return;
  float flo[3], fhi[3];
  if (ref & kLeaf) {
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (long long g = (long long)(ref & ~kLeaf); g < n_rec; ++g) {
      const TriShade sh = shade[g];
      const int32_t row = clip_idx[g];
      if (row < 0) {
        for (int c = 0; c < 3; ++c) rt_refit_grow(lo, hi, vpos + 3 * (size_t)sh.v[c]);
      } else {
        double p[3][3], clip[6], blo[3], bhi[3];
        for (int c = 0; c < 3; ++c)
          for (int k = 0; k < 3; ++k) p[c][k] = vpos[3 * (size_t)sh.v[c] + k];
        for (int k = 0; k < 6; ++k) clip[k] = clip_box[6 * (size_t)row + k];
        if (rt_reclip_box(p[0], p[1], p[2], clip, blo, bhi)) {
          rt_refit_grow(lo, hi, blo);
          rt_refit_grow(lo, hi, bhi);
        }
      }
      if (tris[g].meta & kLastDev) break;
    }
    rt_refit_leaf_box(lo, hi, delta, flo, fhi);   // (+inf - delta and -inf + delta stay: the empty box)
  } else {
    if (ref >= n_nodes) return;   // (no such reference in a layout build_image made)
    const GNode4& Cn = nodes4[ref];
    rt_refit_union4(Cn.lox, Cn.hix, &flo[0], &fhi[0]);
    rt_refit_union4(Cn.loy, Cn.hiy, &flo[1], &fhi[1]);
    rt_refit_union4(Cn.loz, Cn.hiz, &flo[2], &fhi[2]);
  }
  N.lox[slot] = flo[0]; N.hix[slot] = fhi[0];
  N.loy[slot] = flo[1]; N.hiy[slot] = fhi[1];
  N.loz[slot] = flo[2]; N.hiz[slot] = fhi[2];
}

#if defined(__HIPCC__)
// one thread per device record
__global__ void __launch_bounds__(kUpdBlock) update_records_kernel(GTri* tris, const TriShade* shade, double* tnorm,
                                                                   const double* vpos, const double* vnorm,
                                                                   const double* fnorm, long long n_rec) {
  const long long g = (long long)blockIdx.x * kUpdBlock + threadIdx.x;
  if (g < n_rec) update_record_body(g, tris, shade, tnorm, vpos, vnorm, fnorm);
}

// one lane per (node, slot) of one height of the tree: order[0 .. n_level) are that height's node ids
__global__ void __launch_bounds__(kUpdBlock) refit_nodes4_kernel(GNode4* nodes4, uint32_t n_nodes, const uint32_t* order,
                                                                 long long n_level, const GTri* tris,
                                                                 const TriShade* shade, long long n_rec,
                                                                 const double* vpos, double delta) {
  const long long i = (long long)blockIdx.x * kUpdBlock + threadIdx.x;
  if (i >= 4 * n_level) return;
  const uint32_t node = order[i >> 2];
  if (node < n_nodes) refit_slot_body(node, (int)(i & 3), nodes4, n_nodes, tris, shade, n_rec, vpos, delta);
}

// the same schedule with re-clipped leaf slots
__global__ void __launch_bounds__(kUpdBlock) reclip_nodes4_kernel(GNode4* nodes4, uint32_t n_nodes, const uint32_t* order,
                                                                  long long n_level, const GTri* tris,
                                                                  const TriShade* shade, long long n_rec,
                                                                  const double* vpos, double delta,
                                                                  const int32_t* clip_idx, const double* clip_box) {
  const long long i = (long long)blockIdx.x * kUpdBlock + threadIdx.x;
  if (i >= 4 * n_level) return;
  const uint32_t node = order[i >> 2];
  if (node < n_nodes)
    reclip_slot_body(node, (int)(i & 3), nodes4, n_nodes, tris, shade, n_rec, vpos, delta, clip_idx, clip_box);
}
#endif

// Heights of the 4-wide nodes (the longest path to a leaf-only node) from their refs, and the node
// ids sorted by height: order[level_begin[h] .. level_begin[h + 1]) is height h.  Children carry
// larger ids than their parent (build_image), but ids are not in height order -- the treelet prefix
// is breadth-first -- hence the sort.  false: a reference that breaks the id rule.
inline bool refit_schedule(const std::vector<GNode4>& nodes4, std::vector<uint32_t>& order,
                           std::vector<long long>& level_begin) {
  const size_t n = nodes4.size();
  std::vector<int> height(n, 0);
  int top = 0;
  for (size_t i = n; i-- > 0;) {
    int h = 0;
    for (int s = 0; s < 4; ++s) {
      const uint32_t ref = nodes4[i].ref[s];
      if (ref == kEmpty || (ref & kLeaf)) continue;
      if (ref <= i || ref >= n) return false;
      h = std::max(h, height[ref] + 1);
    }
    height[i] = h;
    top = std::max(top, h);
  }
  level_begin.assign((size_t)top + 2, 0);
  for (size_t i = 0; i < n; ++i) level_begin[(size_t)height[i] + 1]++;
  for (size_t h = 1; h < level_begin.size(); ++h) level_begin[h] += level_begin[h - 1];
  order.resize(n);
  std::vector<long long> at(level_begin.begin(), level_begin.end() - 1);
  for (size_t i = 0; i < n; ++i) order[(size_t)at[(size_t)height[i]]++] = (uint32_t)i;
  return true;
}

}  // namespace

#ifndef RT_UPDATE_KERNELS_ONLY

// What a scene's first rt_scene_update_vertices allocates: device copies of the caller's three
// arrays, the refit schedule, and on the host the vertex ids the records reference (the root box).
struct UpdateState {
  double* d_vpos = nullptr;     // [3 * n_vertices]
  double* d_vnorm = nullptr;    // [3 * n_vertices]
  double* d_fnorm = nullptr;    // [3 * n_tris], by slot
  uint32_t* d_order = nullptr;  // [n_gnodes4] node ids sorted by height
  int32_t* d_clip_idx = nullptr;   // [n_rec], d_clip_box [6 * cut records]: the scene's clip table, copied by
  double* d_clip_box = nullptr;    // its first RT_UPDATE_RECLIP update
  std::vector<long long> level_begin;
  std::vector<int> used_vertices;   // sorted, unique
  hipEvent_t ev_in = nullptr, ev_out = nullptr;   // reserve_cus: the caller's stream joined to the masked one
  long long bytes = 0;
};

namespace {

void update_state_free(rt_scene* sc) {
  UpdateState* U = sc->update;
  if (!U) return;
  void* ptrs[] = {U->d_vpos, U->d_vnorm, U->d_fnorm, U->d_order, U->d_clip_idx, U->d_clip_box};
  for (void* q : ptrs)
    if (q) (void)hipFree(q);
  if (U->ev_in) (void)hipEventDestroy(U->ev_in);
  if (U->ev_out) (void)hipEventDestroy(U->ev_out);
  delete U;
  sc->update = nullptr;
}

// The schedule (the refs read back once), the referenced vertex ids and the device arrays of U.
int update_state_fill(const rt_scene* sc, UpdateState& U) {
  std::vector<GNode4> nodes4((size_t)sc->n_gnodes4);
  std::vector<TriShade> shade((size_t)sc->n_rec);
  HIP_TRY(hipMemcpy(nodes4.data(), sc->d_nodes4, nodes4.size() * sizeof(GNode4), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(shade.data(), sc->d_shade, shade.size() * sizeof(TriShade), hipMemcpyDeviceToHost));
  std::vector<uint32_t> order;
  if (!refit_schedule(nodes4, order, U.level_begin))
    return fail(RT_ERR_HIP, "rt_scene_update_vertices: the device hierarchy's references are not in id order");
  std::vector<uint8_t> used((size_t)sc->n_vertices, 0);
  for (const TriShade& sh : shade)
    for (int c = 0; c < 3; ++c) {
      if (sh.v[c] < 0 || sh.v[c] >= sc->n_vertices)
        return fail(RT_ERR_HIP, "rt_scene_update_vertices: a device record holds a vertex id out of range");
      used[(size_t)sh.v[c]] = 1;
    }
  for (long long v = 0; v < sc->n_vertices; ++v)
    if (used[(size_t)v]) U.used_vertices.push_back((int)v);
  const size_t vb = 3 * (size_t)sc->n_vertices * sizeof(double), fb = 3 * (size_t)sc->n_tris * sizeof(double);
  const size_t ob = order.size() * sizeof(uint32_t);
  HIP_TRY(hipMalloc(reinterpret_cast<void**>(&U.d_vpos), vb));
  HIP_TRY(hipMalloc(reinterpret_cast<void**>(&U.d_vnorm), vb));
  HIP_TRY(hipMalloc(reinterpret_cast<void**>(&U.d_fnorm), fb));
  HIP_TRY(hipMalloc(reinterpret_cast<void**>(&U.d_order), ob));
  HIP_TRY(hipMemcpy(U.d_order, order.data(), ob, hipMemcpyHostToDevice));
  U.bytes = (long long)(2 * vb + fb + ob);
  return RT_OK;
}

// First use.  A failed initialisation leaves the scene as it was.
int update_state_init(rt_scene* sc) {
  if (sc->update) return RT_OK;
  sc->update = new UpdateState();
  const int rc = update_state_fill(sc, *sc->update);
  if (rc != RT_OK) {
    update_state_free(sc);
    return rc;
  }
  sc->bytes += sc->update->bytes;
  return RT_OK;
}

// The first re-clipping update of a scene with a clip table: the table's device copy,
// 4 * records + 48 * cut records bytes.  A failure leaves the scene as it was.
int update_state_clip(rt_scene* sc) {
  UpdateState& U = *sc->update;
  if (U.d_clip_idx) return RT_OK;
  const ClipTable& C = *sc->clip;
  const size_t rows = C.box.size() / 6;
  if ((long long)C.idx.size() != sc->n_rec || rows == 0)
    return fail(RT_ERR_HIP, "rt_scene_update_vertices: the clip table does not match the device records");
  for (const int32_t r : C.idx)
    if (r < -1 || (r >= 0 && (size_t)r >= rows))
      return fail(RT_ERR_HIP, "rt_scene_update_vertices: a clip index out of range");
  const size_t ib = C.idx.size() * sizeof(int32_t), bb = C.box.size() * sizeof(double);
  int32_t* d_idx = nullptr;
  double* d_box = nullptr;
  if (hipMalloc(reinterpret_cast<void**>(&d_idx), ib) != hipSuccess ||
      hipMalloc(reinterpret_cast<void**>(&d_box), bb) != hipSuccess ||
      hipMemcpy(d_idx, C.idx.data(), ib, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(d_box, C.box.data(), bb, hipMemcpyHostToDevice) != hipSuccess) {
    if (d_idx) (void)hipFree(d_idx);
    if (d_box) (void)hipFree(d_box);
    return fail(RT_ERR_HIP, "rt_scene_update_vertices: copying the clip table failed");
  }
  U.d_clip_idx = d_idx;
  U.d_clip_box = d_box;
  U.bytes += (long long)(ib + bb);
  sc->bytes += (long long)(ib + bb);
  return RT_OK;
}

// The stream a render launch given `caller` would use (reserve_cus: the caller's CU-masked stream,
// which then waits for the work issued on `caller` so far).
int update_stream_begin(rt_scene* sc, hipStream_t caller, hipStream_t* st) {
  UpdateState& U = *sc->update;
  *st = caller;
  if (sc->reserve_cus > 0) {
    const int mrc = masked_stream(sc, caller, st);
    if (mrc != RT_OK) return mrc;
    if (!U.ev_in) HIP_TRY(hipEventCreateWithFlags(&U.ev_in, hipEventDisableTiming));
    if (!U.ev_out) HIP_TRY(hipEventCreateWithFlags(&U.ev_out, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(U.ev_in, caller));
    HIP_TRY(hipStreamWaitEvent(*st, U.ev_in, 0));
  }
  return RT_OK;
}

// With d_vpos, d_vnorm and d_fnorm written in the order of `st`: one kernel rewrites the records, one
// per height of the tree refits the boxes (leaf-only nodes first), `caller` is joined, and the
// scene's delta and root box ([lo, hi] grown by delta) switch.
int update_issue(rt_scene* sc, hipStream_t st, hipStream_t caller, bool reclip, double delta, const double lo[3],
                 const double hi[3]) {
  UpdateState& U = *sc->update;
  const long long n_rec = sc->n_rec;
  hipLaunchKernelGGL(update_records_kernel, dim3((unsigned)((n_rec + kUpdBlock - 1) / kUpdBlock)), dim3(kUpdBlock), 0, st,
                     sc->d_tris, sc->d_shade, sc->d_tnorm, U.d_vpos, U.d_vnorm, U.d_fnorm, n_rec);
  HIP_TRY(hipGetLastError());
  for (size_t h = 0; h + 1 < U.level_begin.size(); ++h) {   // leaf-only nodes first
    const long long n_level = U.level_begin[h + 1] - U.level_begin[h];
    if (n_level <= 0) continue;
    const dim3 grid((unsigned)((4 * n_level + kUpdBlock - 1) / kUpdBlock));
    if (reclip)
      hipLaunchKernelGGL(reclip_nodes4_kernel, grid, dim3(kUpdBlock), 0, st, sc->d_nodes4, (uint32_t)sc->n_gnodes4,
                         U.d_order + U.level_begin[h], n_level, sc->d_tris, sc->d_shade, n_rec, U.d_vpos, delta,
                         U.d_clip_idx, U.d_clip_box);
    else
      hipLaunchKernelGGL(refit_nodes4_kernel, grid, dim3(kUpdBlock), 0, st, sc->d_nodes4, (uint32_t)sc->n_gnodes4,
                         U.d_order + U.level_begin[h], n_level, sc->d_tris, sc->d_shade, n_rec, U.d_vpos, delta);
    HIP_TRY(hipGetLastError());
  }
  if (st != caller) {   // the caller's later work follows the update
    HIP_TRY(hipEventRecord(U.ev_out, st));
    HIP_TRY(hipStreamWaitEvent(caller, U.ev_out, 0));
  }
  sc->delta = delta;
  for (int k = 0; k < 3; ++k) {
    sc->root_lo[k] = lo[k] - delta;
    sc->root_hi[k] = hi[k] + delta;
  }
  sc->updated = true;
  return RT_OK;
}

}  // namespace

extern "C" {

int rt_scene_update_vertices(rt_scene* sc, const rt_scene_update* u, void* stream) {
  return rt_scene_update_vertices_ex(sc, u, 0u, stream);
}

int rt_scene_update_vertices_ex(rt_scene* sc, const rt_scene_update* u, unsigned flags, void* stream) {
  if (!sc || !u) return fail(RT_ERR_INVALID, "rt_scene_update_vertices: null argument");
  if (flags & ~(unsigned)RT_UPDATE_RECLIP) return fail(RT_ERR_INVALID, "rt_scene_update_vertices: unknown flag");
  if (!u->vertex_pos || !u->vertex_normals || !u->face_normals)
    return fail(RT_ERR_INVALID, "rt_scene_update_vertices: null array");
  if (u->n_vertices != sc->n_vertices || u->n_triangles != sc->n_tris)
    return fail(RT_ERR_INVALID, "rt_scene_update_vertices: n_vertices / n_triangles differ from the uploaded scene's");
  // delta as build_image computes it
  double M = 0.0;
  for (long long k = 0; k < 3LL * u->n_vertices; ++k) M = std::max(M, std::fabs(u->vertex_pos[k]));
  if (!(M > 0.0)) M = 1.0;
  if (M > RT_MAX_COORDINATE) {
    char msg[176];
    std::snprintf(msg, sizeof msg,
                  "rt_scene_update_vertices: vertex coordinate of magnitude %.3g beyond the supported 2^61 (2.3e18)", M);
    return fail(RT_ERR_UNSUPPORTED, msg);
  }
  const double delta = M * 9.5367431640625e-07;   // 2^-20
  if (guard_tripped(sc)) return fail(RT_ERR_HIP, kGuardMsg);
  if (sc->n_tris == 0) {   // nothing to refit: no launch
    sc->delta = delta;
    return RT_OK;
  }
  HIP_TRY(hipSetDevice(sc->device));
  const int irc = update_state_init(sc);
  if (irc != RT_OK) return irc;
  UpdateState& U = *sc->update;
  // without a clip table (no record was cut) the re-clipping refit is the plain one
  const bool reclip = (flags & RT_UPDATE_RECLIP) && sc->clip;
  if (reclip) {
    const int crc = update_state_clip(sc);
    if (crc != RT_OK) return crc;
  }
  // the root box: the referenced vertices' bounds, grown by delta (the reference root's box)
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (const int v : U.used_vertices) rt_refit_grow(lo, hi, u->vertex_pos + 3 * (size_t)v);

  const hipStream_t caller = reinterpret_cast<hipStream_t>(stream);
  hipStream_t st = caller;
  const int src = update_stream_begin(sc, caller, &st);
  if (src != RT_OK) return src;
  const size_t vb = 3 * (size_t)sc->n_vertices * sizeof(double), fb = 3 * (size_t)sc->n_tris * sizeof(double);
  // (pageable host memory: these return once the arrays were read)
  HIP_TRY(hipMemcpyAsync(U.d_vpos, u->vertex_pos, vb, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(U.d_vnorm, u->vertex_normals, vb, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(U.d_fnorm, u->face_normals, fb, hipMemcpyHostToDevice, st));
  return update_issue(sc, st, caller, reclip, delta, lo, hi);
}

long long rt_debug_scene_image(rt_scene* sc, int what, void* out, long long bytes) {
  if (!sc || bytes < 0 || (bytes > 0 && !out)) return fail(RT_ERR_INVALID, "rt_debug_scene_image: bad argument");
  const void* src = nullptr;
  long long have = 0;
  switch (what) {
    case RT_IMAGE_NODES4: src = sc->d_nodes4; have = (long long)sc->n_gnodes4 * (long long)sizeof(GNode4); break;
    case RT_IMAGE_TRIS: src = sc->d_tris; have = sc->n_rec * (long long)sizeof(GTri); break;
    case RT_IMAGE_TNORM: src = sc->d_tnorm; have = sc->n_rec * 12LL * (long long)sizeof(double); break;
    default: return fail(RT_ERR_INVALID, "rt_debug_scene_image: unknown array");
  }
  HIP_TRY(hipSetDevice(sc->device));
  HIP_TRY(hipDeviceSynchronize());
  const long long n = std::min(bytes, have);
  if (n > 0) HIP_TRY(hipMemcpy(out, src, (size_t)n, hipMemcpyDeviceToHost));
  return have;
}

}  // extern "C"

#endif   // !RT_UPDATE_KERNELS_ONLY
