// rt_normals.inc — a device scene moved by positions alone: rt_scene_set_triangle_order,
// rt_scene_update_positions, rt_normals_host (include/rt_hip.h; DESIGN.md §26).  Included by
// rt_render.hip after rt_update.inc.
//
// face_normals_kernel makes every slot's face normal and corner weights from the new positions,
// vertex_normals_kernel sums each vertex's corners in the mesh's triangle order (a CSR built once by
// rt_scene_set_triangle_order) -- rt_normals.hpp's text, HostMesh::compute_normals' bits --, and the
// record and refit kernels of rt_update.inc follow unchanged.  For positions that are already on the
// device, bounds_reduce_kernel and bounds_final_kernel bring max|vertex| and the referenced vertices'
// box to the host: min and max are order-free, so block partials and one small kernel are exact; no
// float atomics, no spin-wait, no grid barrier.
//
// The per-thread bodies are __host__ __device__ functions over plain pointers, so a stand-alone host
// program can run the same text (define RT_UPDATE_KERNELS_ONLY, include rt_update.inc and
// rt_normals.hpp first).

namespace {

constexpr int kRedBlocks = 256;   // most blocks, and so partials, of bounds_reduce_kernel
typedef int nrm_i32x4 __attribute__((ext_vector_type(4)));
typedef double nrm_f64x2 __attribute__((ext_vector_type(2)));

// Slot `slot`: its three vertex ids in one 16-B load (slot_vid[4 * slot ..], the fourth word unused),
// fnorm[slot] = the face normal, weight[4 * slot ..] = the three corner weights in two 16-B stores.
__host__ __device__ inline void face_normal_body(long long slot, const int32_t* slot_vid, const double* vpos,
                                                 double* fnorm, double* weight) {
  const nrm_i32x4 id = reinterpret_cast<const nrm_i32x4*>(slot_vid)[slot];
  double n[3], w[3];
  rt_normals_face(vpos + 3 * (size_t)id.x, vpos + 3 * (size_t)id.y, vpos + 3 * (size_t)id.z, n, w);
  double* f = fnorm + 3 * (size_t)slot;
  f[0] = n[0];
  f[1] = n[1];
  f[2] = n[2];
  upd_u32x4* W = reinterpret_cast<upd_u32x4*>(weight + 4 * (size_t)slot);
  W[0] = upd_pack(w[0], w[1]);
  W[1] = upd_pack(w[2], 0.0);
}

// Vertex v: the gather over corner[begin[v] .. begin[v + 1]), each 3 * slot + corner, in the stored
// order; a vertex without corners gets (0, 0, 0).
__host__ __device__ inline void vertex_normal_body(long long v, const uint32_t* begin, const uint32_t* corner,
                                                   const double* fnorm, const double* weight, double* vnorm) {
  double sum[3] = {0.0, 0.0, 0.0};
  const uint32_t end = begin[v + 1];
  for (uint32_t j = begin[v]; j < end; ++j) {
    const uint32_t idx = corner[j], slot = idx / 3u;
    rt_normals_add(sum, fnorm + 3 * (size_t)slot, weight[(size_t)idx + slot]);   // weight[4 * slot + corner]
  }
  rt_normals_normalize(sum);
  double* o = vnorm + 3 * (size_t)v;
  o[0] = sum[0];
  o[1] = sum[1];
  o[2] = sum[2];
}

// b = {M, lo xyz, hi xyz}: max|value| over all coordinates and the box of the referenced vertices,
// with the comparisons of std::max(M, fabs(x)) and rt_refit_grow: a NaN never wins.
__host__ __device__ inline void bounds_identity(double b[7]) {
  b[0] = 0.0;
  b[1] = b[2] = b[3] = INFINITY;
  b[4] = b[5] = b[6] = -INFINITY;
}
__host__ __device__ inline void bounds_abs(double b[7], double x) {
  const double a = fabs(x);
  b[0] = b[0] < a ? a : b[0];
}
__host__ __device__ inline void bounds_merge(double b[7], const double o[7]) {
  b[0] = b[0] < o[0] ? o[0] : b[0];
  for (int k = 0; k < 3; ++k) {
    b[1 + k] = o[1 + k] < b[1 + k] ? o[1 + k] : b[1 + k];
    b[4 + k] = o[4 + k] > b[4 + k] ? o[4 + k] : b[4 + k];
  }
}

// The share of thread `first` of `stride`: coordinates first, first + stride, .. of vpos[0 .. n_values)
// (in pairs, 16-B loads, where `aligned` says vpos allows it) and referenced vertices used[first], ..
__host__ __device__ inline void bounds_thread_body(long long first, long long stride, const double* vpos,
                                                   long long n_values, int aligned, const int32_t* used, long long n_used,
                                                   double b[7]) {
  const long long n_pairs = aligned ? n_values / 2 : 0;
  for (long long k = first; k < n_pairs; k += stride) {
    const nrm_f64x2 x = reinterpret_cast<const nrm_f64x2*>(vpos)[k];
    bounds_abs(b, x.x);
    bounds_abs(b, x.y);
  }
  for (long long k = 2 * n_pairs + first; k < n_values; k += stride) bounds_abs(b, vpos[k]);
  for (long long i = first; i < n_used; i += stride) rt_refit_grow(b + 1, b + 4, vpos + 3 * (size_t)used[i]);
}

#if defined(__HIPCC__)
// one thread per slot
__global__ void __launch_bounds__(kUpdBlock) face_normals_kernel(const int32_t* slot_vid, const double* vpos, double* fnorm,
                                                                 double* weight, long long n_slots) {
  const long long s = (long long)blockIdx.x * kUpdBlock + threadIdx.x;
  if (s < n_slots) face_normal_body(s, slot_vid, vpos, fnorm, weight);
}

// one thread per vertex
__global__ void __launch_bounds__(kUpdBlock) vertex_normals_kernel(const uint32_t* begin, const uint32_t* corner,
                                                                   const double* fnorm, const double* weight,
                                                                   double* vnorm, long long n_vertices) {
  const long long v = (long long)blockIdx.x * kUpdBlock + threadIdx.x;
  if (v < n_vertices) vertex_normal_body(v, begin, corner, fnorm, weight, vnorm);
}

// The block's b in thread 0: the wave's 64 lanes by shuffles, the block's 4 waves through LDS.
__device__ inline void bounds_block_reduce(double b[7]) {
  __shared__ double part[kUpdBlock / 64][7];
  for (int off = 32; off > 0; off >>= 1) {
    double o[7];
#pragma unroll
    for (int k = 0; k < 7; ++k) o[k] = __shfl_down(b[k], off, 64);
    bounds_merge(b, o);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0)
#pragma unroll
    for (int k = 0; k < 7; ++k) part[wave][k] = b[k];
  __syncthreads();
  if (threadIdx.x == 0)
    for (int w = 1; w < kUpdBlock / 64; ++w) bounds_merge(b, part[w]);
}

// grid-stride over the coordinates and the referenced vertices; partial[7 * block ..] = the block's b
__global__ void __launch_bounds__(kUpdBlock) bounds_reduce_kernel(const double* vpos, long long n_values, int aligned,
                                                                  const int32_t* used, long long n_used, double* partial) {
  double b[7];
  bounds_identity(b);
  bounds_thread_body((long long)blockIdx.x * kUpdBlock + threadIdx.x, (long long)gridDim.x * kUpdBlock, vpos, n_values,
                     aligned, used, n_used, b);
  bounds_block_reduce(b);
  if (threadIdx.x == 0)
#pragma unroll
    for (int k = 0; k < 7; ++k) partial[7 * (size_t)blockIdx.x + k] = b[k];
}

// one block: the n_partial <= kRedBlocks partials into out[0 .. 7) (page-locked host memory)
__global__ void __launch_bounds__(kUpdBlock) bounds_final_kernel(const double* partial, int n_partial, double* out) {
  double b[7];
  bounds_identity(b);
  for (int i = (int)threadIdx.x; i < n_partial; i += kUpdBlock) bounds_merge(b, partial + 7 * (size_t)i);
  bounds_block_reduce(b);
  if (threadIdx.x == 0)
#pragma unroll
    for (int k = 0; k < 7; ++k) out[k] = b[k];
}
#endif

// Is slot_triangle[0 .. n) a permutation of [0, n)?
inline bool normals_is_permutation(const int* slot_triangle, long long n) {
  std::vector<uint8_t> seen((size_t)n, 0);
  for (long long s = 0; s < n; ++s) {
    const long long t = slot_triangle[s];
    if (t < 0 || t >= n || seen[(size_t)t]) return false;
    seen[(size_t)t] = 1;
  }
  return true;
}

// The tables of the two normal kernels from the slots' vertex ids (ids[id_stride * slot + corner]) and
// the permutation slot_triangle: slot_vid[4 * slot ..] = the ids, and the CSR of every vertex's
// corners 3 * slot + corner sorted by (slot_triangle[slot], corner) -- triangles are visited in their
// own order, so a vertex's entries arrive sorted, a vertex named twice by one triangle twice.
// false: an id outside [0, n_vertices).
inline bool normals_tables(const int32_t* ids, int id_stride, const int* slot_triangle, long long n_vertices,
                           long long n_triangles, std::vector<int32_t>& slot_vid, std::vector<uint32_t>& begin,
                           std::vector<uint32_t>& corner) {
  slot_vid.assign(4 * (size_t)n_triangles, 0);
  begin.assign((size_t)n_vertices + 1, 0u);
  corner.assign(3 * (size_t)n_triangles, 0u);
  std::vector<uint32_t> tri_slot((size_t)n_triangles);
  for (long long s = 0; s < n_triangles; ++s) {
    tri_slot[(size_t)slot_triangle[s]] = (uint32_t)s;
    for (int c = 0; c < 3; ++c) {
      const int32_t v = ids[(size_t)id_stride * (size_t)s + c];
      if (v < 0 || v >= n_vertices) return false;
      slot_vid[4 * (size_t)s + c] = v;
      begin[(size_t)v + 1]++;
    }
  }
  for (size_t v = 1; v < begin.size(); ++v) begin[v] += begin[v - 1];
  std::vector<uint32_t> at(begin.begin(), begin.end() - 1);
  for (long long t = 0; t < n_triangles; ++t) {
    const uint32_t s = tri_slot[(size_t)t];
    for (int c = 0; c < 3; ++c) corner[at[(size_t)slot_vid[4 * (size_t)s + c]]++] = 3u * s + (uint32_t)c;
  }
  return true;
}

}  // namespace

#ifndef RT_UPDATE_KERNELS_ONLY

// What rt_scene_set_triangle_order allocates (the tables of the two normal kernels and the corner
// weights), and what the scene's first update from a device pointer adds (the reduction's scratch).
struct NormalState {
  int32_t* d_slot_vid = nullptr;   // [4 * n_tris]
  uint32_t* d_begin = nullptr;     // [n_vertices + 1]
  uint32_t* d_corner = nullptr;    // [3 * n_tris]
  double* d_weight = nullptr;      // [4 * n_tris]
  int32_t* d_used = nullptr;       // [referenced vertices]: UpdateState::used_vertices
  double* d_partial = nullptr;     // [7 * kRedBlocks]
  double* h_bounds = nullptr;      // 7 doubles of page-locked host memory, d_bounds as the kernel addresses them
  double* d_bounds = nullptr;
  long long n_used = 0;
  long long bytes = 0;
};

namespace {

void normal_state_free(rt_scene* sc) {
  NormalState* N = sc->normals;
  if (!N) return;
  void* ptrs[] = {N->d_slot_vid, N->d_begin, N->d_corner, N->d_weight, N->d_used, N->d_partial};
  for (void* q : ptrs)
    if (q) (void)hipFree(q);
  if (N->h_bounds) (void)hipHostFree(N->h_bounds);
  sc->bytes -= N->bytes;
  delete N;
  sc->normals = nullptr;
}

template <typename T>
int normal_upload(T** dst, const std::vector<T>& src, long long& bytes) {
  HIP_TRY(hipMalloc(reinterpret_cast<void**>(dst), src.size() * sizeof(T)));
  HIP_TRY(hipMemcpy(*dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice));
  bytes += (long long)(src.size() * sizeof(T));
  return RT_OK;
}

int normal_state_fill(const rt_scene* sc, const int* slot_triangle, NormalState& N) {
  const size_t nt = (size_t)sc->n_tris;
  std::vector<uint32_t> slot2dev(nt);
  std::vector<TriShade> shade((size_t)sc->n_rec);
  HIP_TRY(hipMemcpy(slot2dev.data(), sc->d_slot2dev, nt * sizeof(uint32_t), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(shade.data(), sc->d_shade, shade.size() * sizeof(TriShade), hipMemcpyDeviceToHost));
  std::vector<int32_t> ids(3 * nt);
  for (size_t s = 0; s < nt; ++s) {
    if (slot2dev[s] >= shade.size())
      return fail(RT_ERR_HIP, "rt_scene_set_triangle_order: a slot's device record is out of range");
    for (int c = 0; c < 3; ++c) ids[3 * s + c] = shade[slot2dev[s]].v[c];
  }
  std::vector<int32_t> slot_vid;
  std::vector<uint32_t> begin, corner;
  if (!normals_tables(ids.data(), 3, slot_triangle, sc->n_vertices, sc->n_tris, slot_vid, begin, corner))
    return fail(RT_ERR_HIP, "rt_scene_set_triangle_order: a device record holds a vertex id out of range");
  int rc = normal_upload(&N.d_slot_vid, slot_vid, N.bytes);
  if (rc == RT_OK) rc = normal_upload(&N.d_begin, begin, N.bytes);
  if (rc == RT_OK) rc = normal_upload(&N.d_corner, corner, N.bytes);
  if (rc != RT_OK) return rc;
  HIP_TRY(hipMalloc(reinterpret_cast<void**>(&N.d_weight), 4 * nt * sizeof(double)));
  N.bytes += (long long)(4 * nt * sizeof(double));
  return RT_OK;
}

// The first update from a device pointer: the referenced vertex ids on the device, the block
// partials and the 7 page-locked doubles.  A failure leaves the scene as it was.
int normal_state_reduce(rt_scene* sc) {
  NormalState& N = *sc->normals;
  if (N.d_partial) return RT_OK;
  const std::vector<int>& used = sc->update->used_vertices;
  const size_t ub = used.size() * sizeof(int32_t), pb = 7 * (size_t)kRedBlocks * sizeof(double);
  int32_t* d_used = nullptr;
  double *d_partial = nullptr, *h_bounds = nullptr, *d_bounds = nullptr;
  if (hipMalloc(reinterpret_cast<void**>(&d_used), std::max<size_t>(ub, 4)) != hipSuccess ||
      hipMalloc(reinterpret_cast<void**>(&d_partial), pb) != hipSuccess ||
      hipMemcpy(d_used, used.data(), ub, hipMemcpyHostToDevice) != hipSuccess ||
      hipHostMalloc(reinterpret_cast<void**>(&h_bounds), 64, hipHostMallocMapped) != hipSuccess ||
      hipHostGetDevicePointer(reinterpret_cast<void**>(&d_bounds), h_bounds, 0) != hipSuccess) {
    if (d_used) (void)hipFree(d_used);
    if (d_partial) (void)hipFree(d_partial);
    if (h_bounds) (void)hipHostFree(h_bounds);
    return fail(RT_ERR_HIP, "rt_scene_update_positions: allocating the reduction's scratch failed");
  }
  N.d_used = d_used;
  N.d_partial = d_partial;
  N.h_bounds = h_bounds;
  N.d_bounds = d_bounds;
  N.n_used = (long long)used.size();
  const long long add = (long long)(std::max<size_t>(ub, 4) + pb);
  N.bytes += add;
  sc->bytes += add;
  return RT_OK;
}

}  // namespace

extern "C" {

int rt_scene_set_triangle_order(rt_scene* sc, const int* slot_triangle, long long n_triangles) {
  if (!sc || !slot_triangle) return fail(RT_ERR_INVALID, "rt_scene_set_triangle_order: null argument");
  if (n_triangles < 0) return fail(RT_ERR_INVALID, "rt_scene_set_triangle_order: negative n_triangles");
  if (3 * n_triangles > (long long)INT32_MAX)
    return fail(RT_ERR_UNSUPPORTED, "rt_scene_set_triangle_order: 3 * n_triangles does not fit a 32-bit corner index");
  if (!normals_is_permutation(slot_triangle, n_triangles))
    return fail(RT_ERR_INVALID, "rt_scene_set_triangle_order: slot_triangle is not a permutation of [0, n_triangles)");
  if (n_triangles != sc->n_tris)
    return fail(RT_ERR_INVALID, "rt_scene_set_triangle_order: n_triangles differs from the uploaded scene's");
  auto* N = new NormalState();
  if (sc->n_tris > 0) {   // (a scene without triangles needs no table and no HIP call)
    int rc = hipSetDevice(sc->device) == hipSuccess ? RT_OK : fail(RT_ERR_HIP, "rt_scene_set_triangle_order: hipSetDevice failed");
    if (rc == RT_OK) rc = normal_state_fill(sc, slot_triangle, *N);
    if (rc != RT_OK) {
      void* ptrs[] = {N->d_slot_vid, N->d_begin, N->d_corner, N->d_weight};
      for (void* q : ptrs)
        if (q) (void)hipFree(q);
      delete N;
      return rc;
    }
  }
  if (sc->normals) {   // replaced: an update in flight may still read the old tables
    if (sc->n_tris > 0) (void)hipDeviceSynchronize();
    normal_state_free(sc);
  }
  sc->normals = N;
  sc->bytes += N->bytes;
  return RT_OK;
}

int rt_scene_update_positions(rt_scene* sc, const rt_scene_positions* p, unsigned flags, void* stream) {
  if (!sc || !p) return fail(RT_ERR_INVALID, "rt_scene_update_positions: null argument");
  if (flags & ~(unsigned)RT_UPDATE_RECLIP) return fail(RT_ERR_INVALID, "rt_scene_update_positions: unknown flag");
  if (!p->vertex_pos) return fail(RT_ERR_INVALID, "rt_scene_update_positions: null array");
  if (p->on_device != 0 && p->on_device != 1)
    return fail(RT_ERR_INVALID, "rt_scene_update_positions: on_device must be 0 or 1");
  if (p->n_vertices != sc->n_vertices)
    return fail(RT_ERR_INVALID, "rt_scene_update_positions: n_vertices differs from the uploaded scene's");
  if (!sc->normals)
    return fail(RT_ERR_INVALID, "rt_scene_update_positions: the scene has had no rt_scene_set_triangle_order call");
  const bool on_device = p->on_device == 1;
  const char* const kRange =
      "rt_scene_update_positions: vertex coordinate of magnitude %.3g beyond the supported 2^61 (2.3e18)";
  char msg[176];
  // host pointer: delta as build_image computes it, before any HIP call
  double M = 0.0;
  if (!on_device) {
    for (long long k = 0; k < 3LL * p->n_vertices; ++k) M = std::max(M, std::fabs(p->vertex_pos[k]));
    if (!(M > 0.0)) M = 1.0;
    if (M > RT_MAX_COORDINATE) {
      std::snprintf(msg, sizeof msg, kRange, M);
      return fail(RT_ERR_UNSUPPORTED, msg);
    }
  }
  if (guard_tripped(sc)) return fail(RT_ERR_HIP, kGuardMsg);
  if (sc->n_tris == 0) {   // nothing to refit: no launch (a device pointer is not read: delta stays)
    if (!on_device) sc->delta = M * 9.5367431640625e-07;
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
  if (on_device) {
    const int rrc = normal_state_reduce(sc);
    if (rrc != RT_OK) return rrc;
  }
  NormalState& N = *sc->normals;
  const hipStream_t caller = reinterpret_cast<hipStream_t>(stream);
  hipStream_t st = caller;
  const int src = update_stream_begin(sc, caller, &st);
  if (src != RT_OK) return src;

  // the root box: the referenced vertices' bounds (the reference root's box before delta)
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  const long long nv = sc->n_vertices, nt = sc->n_tris;
  const size_t vb = 3 * (size_t)nv * sizeof(double);
  if (!on_device) {
    for (const int v : U.used_vertices) rt_refit_grow(lo, hi, p->vertex_pos + 3 * (size_t)v);
    // (pageable host memory: this returns once the array was read)
    HIP_TRY(hipMemcpyAsync(U.d_vpos, p->vertex_pos, vb, hipMemcpyHostToDevice, st));
  } else {
    // M and the box from the caller's buffer: the call's one synchronisation; nothing of the scene
    // has been written before the range check
    const long long n_values = 3 * nv;
    const long long want = (std::max(n_values / 2, N.n_used) + kUpdBlock - 1) / kUpdBlock;
    const int blocks = (int)std::min<long long>(std::max<long long>(want, 1), kRedBlocks);
    const int aligned = (reinterpret_cast<uintptr_t>(p->vertex_pos) & 15u) == 0u;
    hipLaunchKernelGGL(bounds_reduce_kernel, dim3((unsigned)blocks), dim3(kUpdBlock), 0, st, p->vertex_pos, n_values,
                       aligned, N.d_used, N.n_used, N.d_partial);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(bounds_final_kernel, dim3(1), dim3(kUpdBlock), 0, st, N.d_partial, blocks, N.d_bounds);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    const volatile double* hb = N.h_bounds;
    M = hb[0];
    for (int k = 0; k < 3; ++k) {
      lo[k] = hb[1 + k];
      hi[k] = hb[4 + k];
    }
    if (!(M > 0.0)) M = 1.0;
    if (M > RT_MAX_COORDINATE) {
      std::snprintf(msg, sizeof msg, kRange, M);
      return fail(RT_ERR_UNSUPPORTED, msg);
    }
    HIP_TRY(hipMemcpyAsync(U.d_vpos, p->vertex_pos, vb, hipMemcpyDeviceToDevice, st));
  }
  const double delta = M * 9.5367431640625e-07;   // 2^-20
  hipLaunchKernelGGL(face_normals_kernel, dim3((unsigned)((nt + kUpdBlock - 1) / kUpdBlock)), dim3(kUpdBlock), 0, st,
                     N.d_slot_vid, U.d_vpos, U.d_fnorm, N.d_weight, nt);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(vertex_normals_kernel, dim3((unsigned)((nv + kUpdBlock - 1) / kUpdBlock)), dim3(kUpdBlock), 0, st,
                     N.d_begin, N.d_corner, U.d_fnorm, N.d_weight, U.d_vnorm, nv);
  HIP_TRY(hipGetLastError());
  return update_issue(sc, st, caller, reclip, delta, lo, hi);
}

int rt_normals_host(const int* vertex_idx, const int* slot_triangle, long long n_vertices, long long n_triangles,
                    const double* vertex_pos, double* vertex_normals_out, double* face_normals_out) {
  if (n_vertices < 0 || n_triangles < 0) return fail(RT_ERR_INVALID, "rt_normals_host: negative count");
  if ((n_triangles > 0 && (!vertex_idx || !slot_triangle || !face_normals_out)) ||
      (n_vertices > 0 && (!vertex_pos || !vertex_normals_out)))
    return fail(RT_ERR_INVALID, "rt_normals_host: null argument");
  if (3 * n_triangles > (long long)INT32_MAX)
    return fail(RT_ERR_UNSUPPORTED, "rt_normals_host: 3 * n_triangles does not fit a 32-bit corner index");
  if (!normals_is_permutation(slot_triangle, n_triangles))
    return fail(RT_ERR_INVALID, "rt_normals_host: slot_triangle is not a permutation of [0, n_triangles)");
  std::vector<int32_t> slot_vid;
  std::vector<uint32_t> begin, corner;
  if (!normals_tables(vertex_idx, 3, slot_triangle, n_vertices, n_triangles, slot_vid, begin, corner))
    return fail(RT_ERR_INVALID, "rt_normals_host: a vertex id out of range");
  std::vector<double> weight(4 * (size_t)n_triangles);
  for (long long s = 0; s < n_triangles; ++s)
    face_normal_body(s, slot_vid.data(), vertex_pos, face_normals_out, weight.data());
  for (long long v = 0; v < n_vertices; ++v)
    vertex_normal_body(v, begin.data(), corner.data(), face_normals_out, weight.data(), vertex_normals_out);
  return RT_OK;
}

}  // extern "C"

#endif   // !RT_UPDATE_KERNELS_ONLY
