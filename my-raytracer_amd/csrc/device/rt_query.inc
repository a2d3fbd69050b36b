// rt_query.inc — batched ray queries on the device scene (rt_trace_closest / rt_trace_occluded,
// include/rt_hip.h; DESIGN.md §15).  Part of rt_render.hip's translation unit, included after
// struct rt_scene: the kernels use the render path's device helpers (normalize, det3, load_tri,
// prim_hit, round_up_f / round_down_f, rcp_refined / div_by, trip_watchdog) unchanged.
//
// One kernel template over ANYHIT: 256-thread blocks, one ray per lane, a bounded grid with a
// grid-stride loop over blocks of 256 rays.  Each ray walks the 4-wide hierarchy with the render
// kernel's conservative fp32 box ray and is tested against the triangle records with the CPU's fp64
// operations in the CPU's order, so a hit is bit-identical to the oracle's (closest hit: the
// smallest (t, reference slot)).  The per-lane stack is an LDS ring laid out [entry][256] whose
// oldest entries spill to the query context's global array.  The walk itself is rt_walk_body.inc,
// the one text this kernel, ao_kernel (rt_ao.inc) and camera_kernel (rt_camera.inc) include; what
// those kernels and their entry points share around it -- the treelet prologue, the counter
// flush, the grid size, the query contexts and the steps around a launch -- is here (DESIGN.md §23).
namespace {

constexpr int kQRing = 8;           // LDS stack-ring entries per lane
constexpr int kQRingMask = kQRing - 1;
// top treelet: the first kQTop 4-wide nodes (breadth-first numbering) are copied into each block's
// LDS; a node iteration whose active lanes all sit in it reads LDS (the same bytes: results equal)
constexpr int kQTop = 64;
constexpr int kQContexts = 4;       // query contexts per scene (queries in flight on different streams)
// counter words of a query context; the guard word sits where trip_watchdog sets it
enum : int { QC_HITS = 0, QC_SPILLS = 1, QC_WATCHDOG = 2, QC_WORDS = CD_GUARD + 1 };

struct QParams {
  const GNode4* nodes4;
  const GTri* tris;
  const double* tnorm;       // [record][12]: face normal, then the 3 vertex normals
  const GMat* mats;
  const GPrim* prims;
  const rt_ray* rays;
  rt_hit* hits;              // closest-hit query
  unsigned char* occ;        // occlusion query
  unsigned long long* ctr;   // [QC_WORDS]
  uint32_t* spill;           // [spill_rows][nslots] stack entries below the LDS ring
  unsigned int* guard_host;  // the scene's watchdog word (trip_watchdog)
  size_t nslots;             // lanes of the grid
  long long n;
  int spill_rows;
  int n_gnodes, n_prims;
  int n_top;                 // 4-wide nodes cached in LDS (ids [0, n_top), at most kQTop)
  double root_lo[3], root_hi[3];
};

__device__ __forceinline__ bool q_finite(double x) { return fabs(x) <= DBL_MAX; }   // false for NaN / inf
__device__ __forceinline__ double q_pack(int lo, int hi) {
  return __builtin_bit_cast(double, u32x2_t{(uint32_t)lo, (uint32_t)hi});
}

// once per block: the top treelet -> LDS
template <class PT>
__device__ __forceinline__ void query_stage_treelet(float4* q_top, const PT& P) {
  const float4* src = reinterpret_cast<const float4*>(P.nodes4);
  for (int i = threadIdx.x; i < P.n_top * (int)(sizeof(GNode4) / sizeof(float4)); i += kBlock) q_top[i] = src[i];
  __syncthreads();
}

// counters: summed per wave, one atomic per wave and counter
template <class PT>
__device__ __forceinline__ void query_flush_counters(const PT& P, int lane, unsigned long long n_hits,
                                                     unsigned long long n_spills, unsigned long long n_trips) {
  const unsigned long long w_hits = wave_sum(n_hits), w_spills = wave_sum(n_spills), w_trips = wave_sum(n_trips);
  if (lane == 0) {
    if (w_hits) atomicAdd(&P.ctr[QC_HITS], w_hits);
    if (w_spills) atomicAdd(&P.ctr[QC_SPILLS], w_spills);
    if (w_trips) atomicAdd(&P.ctr[QC_WATCHDOG], w_trips);
  }
}

template <bool ANYHIT>
__global__ void __launch_bounds__(kBlock, kWavesPerEU * 256 / kBlock) query_kernel(QParams P) {
  __shared__ uint32_t q_ring[kQRing * kBlock];   // [entry][kBlock]: a lane's entries kBlock words apart
  __shared__ float4 q_top[kQTop * (sizeof(GNode4) / sizeof(float4))];
  query_stage_treelet(q_top, P);
  const int lane = threadIdx.x & 63;
  uint32_t* const spill = P.spill + (size_t)blockIdx.x * kBlock + threadIdx.x;
  unsigned long long n_hits = 0, n_spills = 0, n_trips = 0;

  for (long long base = (long long)blockIdx.x * kBlock; base < P.n; base += (long long)gridDim.x * kBlock) {
    // this block's 256 rays and results as raw buffers: the base is wave-uniform, a lane's offset one
    // VGPR, and the hardware drops the accesses of the lanes past the last ray
    const long long left = P.n - base;
    const int nb = left < (long long)kBlock ? (int)left : kBlock;
    const bool act0 = (int)threadIdx.x < nb;
    const __amdgpu_buffer_rsrc_t rr = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<rt_ray*>(P.rays + base), 0, nb * (int)sizeof(rt_ray), kBufWord3);
    const uint32_t vo = threadIdx.x * (uint32_t)sizeof(rt_ray);
    // the 64-B ray: four 16-B loads issued together
    const D2 q0 = buf_ld2(rr, vo, 0), q1 = buf_ld2(rr, vo + 16u, 0), q2 = buf_ld2(rr, vo + 32u, 0),
             q3 = buf_ld2(rr, vo + 48u, 0);
    const D3 ro = d3(q0.a, q0.b, q1.a);
    const D3 dv = d3(q1.b, q2.a, q2.b);
    const double tmax = q3.a;
#include "rt_walk_body.inc"

    if (ANYHIT) {
      if (act0) P.occ[base + threadIdx.x] = occluded ? 1 : 0;
      n_hits += occluded ? 1u : 0u;
    } else {
      // the rt_hit of the walk's closest hit; camera_kernel composes and stores the same record (as
      // a function shared by the two it moved both kernels' register allocation, DESIGN.md §23)
      const bool hit = best != kNoHit;
      n_hits += hit ? 1u : 0u;
      double ht = INFINITY, ha = 0.0, hb2 = 0.0;
      D3 hn = d3(0.0, 0.0, 0.0);
      int o_slot = -1, o_mesh = -1, o_prim = -1;
      if (hit) {
        ht = tlim;
        if (best & kPrimHit) {   // analytic hit: the oracle's normal
          o_prim = best & (kPrimHit - 1);
          const GPrim& G = P.prims[o_prim];
          hn = G.type == kPrimPlane ? d3(G.n[0], G.n[1], G.n[2])
                                    : d3((ro.x + ht * rd.x - G.c[0]) / G.r, (ro.y + ht * rd.y - G.c[1]) / G.r,
                                         (ro.z + ht * rd.z - G.c[2]) / G.r);
        } else {
          ha = best_a;
          hb2 = best_b;
          o_slot = best_slot;
          o_mesh = best_mesh;
          const double gamma = (1.0 - ha - hb2);
          const double* nr = P.tnorm + 12 * (size_t)best;
          if (P.mats[best_mesh].draw_mode == RT_DRAW_FLAT) {
            hn = d3(nr[0], nr[1], nr[2]);
          } else {   // alpha*vn0 + beta*vn1 + gamma*vn2, not renormalised
            hn = d3(ha * nr[3] + hb2 * nr[6] + gamma * nr[9], ha * nr[4] + hb2 * nr[7] + gamma * nr[10],
                    ha * nr[5] + hb2 * nr[8] + gamma * nr[11]);
          }
        }
      }
      // the 64-B hit: 8-B vector stores (DESIGN.md §4 "path state")
      const __amdgpu_buffer_rsrc_t hr =
          __builtin_amdgcn_make_buffer_rsrc(P.hits + base, 0, nb * (int)sizeof(rt_hit), kBufWord3);
      buf_st(hr, vo, 0, ht);
      buf_st(hr, vo + 8u, 0, ha);
      buf_st(hr, vo + 16u, 0, hb2);
      buf_st(hr, vo + 24u, 0, hn.x);
      buf_st(hr, vo + 32u, 0, hn.y);
      buf_st(hr, vo + 40u, 0, hn.z);
      buf_st(hr, vo + 48u, 0, q_pack(o_slot, o_mesh));
      buf_st(hr, vo + 56u, 0, q_pack(o_prim, 0));
    }
  }
  query_flush_counters(P, lane, n_hits, n_spills, n_trips);
}

// Per-query mutable state: counters, the stack-spill array and an event recorded after the query,
// waited on before the context is reused.  Allocated by the scene's first query.
struct QueryCtx {
  unsigned long long* d_ctr = nullptr;   // [QC_WORDS]
  uint32_t* d_spill = nullptr;           // [spill_rows][nslots]
  hipEvent_t done = nullptr;
  bool used = false;
};

}  // namespace

struct QueryRing {
  QueryCtx ctx[kQContexts];
  int next = 0;
  long long grid[2] = {1, 1};   // blocks of a full grid: closest, occluded
  size_t nslots = 0;            // lanes of the larger one
  int spill_rows = 0;
};

namespace {

void query_ring_free(rt_scene* sc) {
  QueryRing* Q = sc->query;
  if (!Q) return;
  for (QueryCtx& c : Q->ctx) {
    if (c.d_ctr) (void)hipFree(c.d_ctr);
    if (c.d_spill) (void)hipFree(c.d_spill);
    if (c.done) (void)hipEventDestroy(c.done);
  }
  delete Q;
  sc->query = nullptr;
}

// blocks of the walking kernel `fn` that fill one CU, as the render launch sizes its own grid (a
// property of the kernel and the architecture)
int query_blocks_per_cu(const void* fn) {
  int nb = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, fn, kBlock, 0) != hipSuccess || nb < 1) nb = 1;
  hipFuncAttributes fa;
  if (hipFuncGetAttributes(&fa, fn) == hipSuccess && fa.numRegs > 0) {
    const int waves_per_simd = 512 / ((fa.numRegs + 7) / 8 * 8);
    nb = std::min(nb, std::max(1, waves_per_simd * 4 / (kBlock / 64)));
  }
  return std::min(nb, (int)(160 * 1024 / (kQRing * kBlock * sizeof(uint32_t) + kQTop * sizeof(GNode4))));
}

int query_ring_init(rt_scene* sc) {
  if (sc->query) return RT_OK;
  auto* Q = new QueryRing();
  sc->query = Q;   // rt_scene_free releases whatever a failed initialisation leaves
  const void* fns[2] = {reinterpret_cast<const void*>(&query_kernel<false>),
                        reinterpret_cast<const void*>(&query_kernel<true>)};
  for (int v = 0; v < 2; ++v) {   // the grid that fills the device
    Q->grid[v] = (long long)std::max(1, sc->n_cu) * query_blocks_per_cu(fns[v]);
    Q->nslots = std::max(Q->nslots, (size_t)Q->grid[v] * kBlock);
  }
  Q->spill_rows = std::max(0, sc->stack_words - kQRing);
  for (QueryCtx& c : Q->ctx) {
    const size_t sb = std::max<size_t>(1, (size_t)Q->spill_rows) * Q->nslots * sizeof(uint32_t);
    if (hipMalloc(reinterpret_cast<void**>(&c.d_ctr), QC_WORDS * sizeof(unsigned long long)) != hipSuccess ||
        hipMalloc(reinterpret_cast<void**>(&c.d_spill), sb) != hipSuccess ||
        hipEventCreateWithFlags(&c.done, hipEventDisableTiming) != hipSuccess) {
      query_ring_free(sc);
      return fail(RT_ERR_HIP, "allocation of query contexts failed");
    }
  }
  return RT_OK;
}

// The scene's next query context, ready for a launch on `st`: the ring allocated, the context's
// previous query waited for and its counters zeroed.
int query_acquire(rt_scene* sc, hipStream_t st, QueryCtx** ctx) {
  HIP_TRY(hipSetDevice(sc->device));
  const int irc = query_ring_init(sc);
  if (irc != RT_OK) return irc;
  QueryRing& Q = *sc->query;
  QueryCtx& C = Q.ctx[Q.next];
  Q.next = (Q.next + 1) % kQContexts;
  // the context's previous query done before its counters and spill array are reused
  if (C.used && !event_done(C.done)) HIP_TRY(hipStreamWaitEvent(st, C.done, 0));
  HIP_TRY(hipMemsetAsync(C.d_ctr, 0, QC_WORDS * sizeof(unsigned long long), st));
  *ctx = &C;
  return RT_OK;
}

// The scene fields every walking kernel's parameter struct has (QParams, AoParams, CamParams), by name.
template <class PT>
void query_scene_params(PT& P, const rt_scene* sc, const QueryCtx& C) {
  const QueryRing& Q = *sc->query;
  P.nodes4 = sc->d_nodes4; P.tris = sc->d_tris; P.prims = sc->d_prims;
  P.ctr = C.d_ctr; P.spill = C.d_spill; P.guard_host = sc->d_guard;
  P.nslots = Q.nslots;
  P.spill_rows = Q.spill_rows;
  P.n_gnodes = sc->n_gnodes; P.n_prims = sc->n_prims;
  P.n_top = std::min(kQTop, sc->n_top_v[0]);   // the production render variant's count (rt_upload_options.lds_treelet)
  for (int k = 0; k < 3; ++k) { P.root_lo[k] = sc->root_lo[k]; P.root_hi[k] = sc->root_hi[k]; }
}

// the grid of a kernel that wants `want` blocks and fills a CU with `per_cu`: the device filled, inside
// the lanes the contexts' spill arrays were sized for
unsigned query_grid(const rt_scene* sc, long long want, int per_cu) {
  const long long full =
      std::min<long long>((long long)std::max(1, sc->n_cu) * per_cu, (long long)(sc->query->nslots / kBlock));
  return (unsigned)std::max<long long>(1, std::min(want, full));
}

// After the launch on context C: the launch error, the context's event, and for a caller that asked
// for statistics the counters of its `rays` rays (this waits for the stream) and the watchdog.
int query_finish(rt_scene* sc, QueryCtx& C, hipStream_t st, long long rays, rt_query_stats* stats) {
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(C.done, st));
  C.used = true;
  if (stats) {
    HIP_TRY(hipStreamSynchronize(st));
    unsigned long long c[QC_WORDS];
    HIP_TRY(hipMemcpy(c, C.d_ctr, sizeof c, hipMemcpyDeviceToHost));
    stats->rays = rays;
    stats->hits = (long long)c[QC_HITS];
    stats->stack_spills = (long long)c[QC_SPILLS];
    stats->watchdog = (long long)c[QC_WATCHDOG];
    if (c[CD_GUARD] != 0 || guard_tripped(sc)) return fail(RT_ERR_HIP, kGuardMsg);
  }
  return RT_OK;
}

int launch_query(rt_scene* sc, const rt_ray* d_rays, long long n, rt_hit* d_hits, unsigned char* d_occ, bool anyhit,
                 rt_query_stats* stats, void* stream) {
  const char* const name = anyhit ? "rt_trace_occluded" : "rt_trace_closest";
  if (!sc) return fail(RT_ERR_INVALID, std::string(name) + ": null scene");
  if (n < 0) return fail(RT_ERR_INVALID, std::string(name) + ": negative ray count");
  if (n > 0 && (!d_rays || (anyhit ? !d_occ : !d_hits)))
    return fail(RT_ERR_INVALID, std::string(name) + ": null ray or result buffer");
  if (guard_tripped(sc)) return fail(RT_ERR_HIP, kGuardMsg);
  if (stats) std::memset(stats, 0, sizeof *stats);
  if (n == 0) return RT_OK;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  QueryCtx* C;
  const int arc = query_acquire(sc, st, &C);
  if (arc != RT_OK) return arc;
  QParams P;
  std::memset(&P, 0, sizeof P);
  query_scene_params(P, sc, *C);
  P.tnorm = sc->d_tnorm; P.mats = sc->d_mats;
  P.rays = d_rays; P.hits = d_hits; P.occ = d_occ;
  P.n = n;
  const long long want = (n + kBlock - 1) / kBlock;
  const unsigned blocks = (unsigned)std::max<long long>(1, std::min<long long>(want, sc->query->grid[anyhit ? 1 : 0]));
  if (anyhit) hipLaunchKernelGGL(query_kernel<true>, dim3(blocks), dim3(kBlock), 0, st, P);
  else hipLaunchKernelGGL(query_kernel<false>, dim3(blocks), dim3(kBlock), 0, st, P);
  return query_finish(sc, *C, st, n, stats);
}

}  // namespace

extern "C" {

int rt_trace_closest(rt_scene* sc, const rt_ray* d_rays, long long n, rt_hit* d_hits, rt_query_stats* stats,
                     void* stream) {
  return launch_query(sc, d_rays, n, d_hits, nullptr, false, stats, stream);
}

int rt_trace_occluded(rt_scene* sc, const rt_ray* d_rays, long long n, unsigned char* d_occluded,
                      rt_query_stats* stats, void* stream) {
  return launch_query(sc, d_rays, n, nullptr, d_occluded, true, stats, stream);
}

}  // extern "C"
