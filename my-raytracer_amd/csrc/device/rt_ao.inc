// rt_ao.inc — occlusion fans generated on the device (rt_trace_ao, rt_ao_rays_host, include/rt_hip.h;
// DESIGN.md §19).  Part of rt_render.hip's translation unit, included after rt_query.inc: the kernel
// uses that file's stack ring, top treelet, counters, query contexts and launch steps and the render
// path's device helpers unchanged.
//
// One kernel: work item j in [0, n k) is sample j % k of point j / k, consecutive lanes on
// consecutive samples, so a wave holds 64 fan rays of at most ceil(64 / k) + 1 points and no lane
// idles for any k.  A lane builds its ray in registers (rt_ao_fan.hpp), walks the hierarchy with the
// any-hit traversal of query_kernel<true> -- the same text, rt_walk_body.inc, included here too, so
// a fan ray is occluded exactly when rt_trace_occluded says so of the ray rt_ao_rays_host writes
// out -- and the wave reduces: a ballot of the lanes that are not occluded, and per point one
// popcount of its run of lanes.
#include "rt_ao_fan.hpp"

static_assert(RT_AO_MAX_SAMPLES == RT_AO_MAX_SAMPLES_ && RT_AO_MAX_SETS == RT_AO_MAX_SETS_,
              "rt_ao_fan.hpp and rt_hip.h disagree");
static_assert((long long)RT_AO_MAX_SAMPLES * RT_AO_MAX_SETS * 24 < (1LL << 31),
              "the largest direction table is one raw buffer with 32-bit offsets");

namespace {

struct AoParams {
  const GNode4* nodes4;
  const GTri* tris;
  const GPrim* prims;
  const rt_ray* points;
  const double* dirs;        // [n_sets][k][3]
  unsigned int* out;         // [n] fan rays that are not occluded
  unsigned long long* ctr;   // [QC_WORDS]
  uint32_t* spill;           // [spill_rows][nslots] stack entries below the LDS ring
  unsigned int* guard_host;  // the scene's watchdog word (trip_watchdog)
  size_t nslots;             // lanes of the query contexts' spill array
  long long n;               // points
  long long total;           // n * k fan rays
  double bias;
  int k, n_sets;
  uint32_t seed;
  uint32_t dir_bytes;        // bytes of the direction table (the limits keep it below 2^31: one raw buffer)
  int spill_rows;
  int n_gnodes, n_prims;
  int n_top;                 // 4-wide nodes cached in LDS (ids [0, n_top), at most kQTop)
  double root_lo[3], root_hi[3];
};

__global__ void __launch_bounds__(kBlock, kWavesPerEU * 256 / kBlock) ao_kernel(AoParams P) {
  __shared__ uint32_t q_ring[kQRing * kBlock];   // [entry][kBlock]: a lane's entries kBlock words apart
  __shared__ float4 q_top[kQTop * (sizeof(GNode4) / sizeof(float4))];
  query_stage_treelet(q_top, P);
  const int lane = threadIdx.x & 63;
  uint32_t* const spill = P.spill + (size_t)blockIdx.x * kBlock + threadIdx.x;
  unsigned long long n_hits = 0, n_spills = 0, n_trips = 0;
  const uint32_t uk = (uint32_t)P.k;

  for (long long base = (long long)blockIdx.x * kBlock; base < P.total; base += (long long)gridDim.x * kBlock) {
    // this block's 256 fan rays: the base is wave-uniform, so its point and sample are derived once
    // (one 64-bit division per block and round); a lane's own are 32-bit from there
    const long long left = P.total - base;
    const int nb = left < (long long)kBlock ? (int)left : kBlock;
    const bool act0 = (int)threadIdx.x < nb;
    const long long point0 = base / P.k;
    const uint32_t samp0 = (uint32_t)(base - point0 * P.k);
    const uint32_t t = samp0 + threadIdx.x;   // < k + 256
    const uint32_t pl = t / uk;               // the lane's point, counted from point0
    const uint32_t s = t - pl * uk;           // ... and its sample
    // the points this block touches as a raw buffer: the hardware drops the loads of the lanes past
    // the last point
    const long long pleft = P.n - point0;
    const uint32_t pspan = (samp0 + (uint32_t)nb - 1u) / uk + 1u;   // <= 257
    const int np = pleft < (long long)pspan ? (int)pleft : (int)pspan;
    const __amdgpu_buffer_rsrc_t pr = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<rt_ray*>(P.points + point0), 0, np * (int)sizeof(rt_ray), kBufWord3);
    const uint32_t vo = pl * (uint32_t)sizeof(rt_ray);
    // the 64-B point: four 16-B loads issued together; the lanes of one point read the same line
    const D2 q0 = buf_ld2(pr, vo, 0), q1 = buf_ld2(pr, vo + 16u, 0), q2 = buf_ld2(pr, vo + 32u, 0),
             q3 = buf_ld2(pr, vo + 48u, 0);
    // the local direction: 24 B of the caller's table, bounded the same way
    const uint32_t set = rt_ao_set(point0 + pl, P.seed, P.n_sets);
    const __amdgpu_buffer_rsrc_t dr =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<double*>(P.dirs), 0, (int)P.dir_bytes, kBufWord3);
    const uint32_t dvo = (set * uk + s) * 24u;
    const D2 l01 = buf_ld2(dr, dvo, 0);
    const double l[3] = {l01.a, l01.b, buf_ld(dr, dvo + 16u, 0)};
    const double pp[3] = {q0.a, q0.b, q1.a}, pn[3] = {q1.b, q2.a, q2.b};
    const double tmax = q3.a;
    double fo[3], fw[3];
    rt_ao_fan_ray(pp, pn, tmax, l, P.bias, fo, fw);
    const D3 ro = d3(fo[0], fo[1], fo[2]);
    const D3 dv = d3(fw[0], fw[1], fw[2]);
    constexpr bool ANYHIT = true;   // the walk of query_kernel<true>
#include "rt_walk_body.inc"
    n_hits += occluded ? 1u : 0u;

    // ---- reduction: every lane is back here; no per-ray byte is written ----
    // A point's run in this wave is the lanes [first, end) that hold its samples.  The run's first
    // lane counts the run's bits of the ballot.  A run that holds all k samples is the point's only
    // one: a plain store; otherwise it adds to the count the call zeroed.
    const unsigned long long open = wballot(act0 && !occluded);
    const uint32_t ulane = (uint32_t)lane;
    const uint32_t first = s < ulane ? ulane - s : 0u;
    const uint32_t end = ulane + (uk - s) < 64u ? ulane + (uk - s) : 64u;
    if (act0 && ulane == first) {
      const unsigned long long below_end = end >= 64u ? ~0ull : (1ull << end) - 1ull;
      const unsigned long long run = below_end & ~((1ull << first) - 1ull);
      const unsigned int cnt = (unsigned int)__popcll(open & run);
      unsigned int* const dst = P.out + (point0 + pl);
      if (s == 0u && end - first == uk) *dst = cnt;
      else atomicAdd(dst, cnt);
    }
  }
  query_flush_counters(P, lane, n_hits, n_spills, n_trips);
}

// the argument checks rt_trace_ao and rt_ao_rays_host share (before any HIP call)
int ao_check(const char* name, const rt_ray* points, long long n, const rt_ao_params* a, const void* out) {
  const std::string who(name);
  if (!a) return fail(RT_ERR_INVALID, who + ": null parameters");
  if (n < 0) return fail(RT_ERR_INVALID, who + ": negative point count");
  if (n > RT_AO_MAX_POINTS) return fail(RT_ERR_INVALID, who + ": more than RT_AO_MAX_POINTS points");
  if (a->k < 1 || a->k > RT_AO_MAX_SAMPLES) return fail(RT_ERR_INVALID, who + ": k outside [1, RT_AO_MAX_SAMPLES]");
  if (a->n_sets < 1 || a->n_sets > RT_AO_MAX_SETS)
    return fail(RT_ERR_INVALID, who + ": n_sets outside [1, RT_AO_MAX_SETS]");
  if (!(std::fabs(a->bias) <= DBL_MAX)) return fail(RT_ERR_INVALID, who + ": bias is not finite");
  if (n > 0 && (!points || !a->d_dirs || !out))
    return fail(RT_ERR_INVALID, who + ": null point, direction or result buffer");
  return RT_OK;
}

int ao_blocks_per_cu() {
  static const int blocks = query_blocks_per_cu(reinterpret_cast<const void*>(&ao_kernel));
  return blocks;
}

}  // namespace

extern "C" {

int rt_ao_rays_host(const rt_ray* points, long long n, const rt_ao_params* a, rt_ray* rays_out) {
  const int rc = ao_check("rt_ao_rays_host", points, n, a, rays_out);
  if (rc != RT_OK) return rc;
  for (long long i = 0; i < n; ++i) {
    const rt_ray& pt = points[i];
    const size_t set = rt_ao_set(i, a->seed, a->n_sets);
    for (int s = 0; s < a->k; ++s) {
      rt_ray& r = rays_out[(size_t)i * a->k + s];
      rt_ao_fan_ray(pt.o, pt.d, pt.tmax, a->d_dirs + (set * a->k + s) * 3, a->bias, r.o, r.d);
      r.tmax = pt.tmax;
      r.reserved_ = 0.0;
    }
  }
  return RT_OK;
}

int rt_trace_ao(rt_scene* sc, const rt_ray* d_points, long long n, const rt_ao_params* a, unsigned int* d_unoccluded,
                rt_query_stats* stats, void* stream) {
  if (!sc) return fail(RT_ERR_INVALID, "rt_trace_ao: null scene");
  const int rc = ao_check("rt_trace_ao", d_points, n, a, d_unoccluded);
  if (rc != RT_OK) return rc;
  if (guard_tripped(sc)) return fail(RT_ERR_HIP, kGuardMsg);
  if (stats) std::memset(stats, 0, sizeof *stats);
  if (n == 0) return RT_OK;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  QueryCtx* C;
  const int arc = query_acquire(sc, st, &C);
  if (arc != RT_OK) return arc;
  // a run of k lanes that 64 does not divide may straddle waves: those points are summed by atomics
  if (64 % a->k != 0) HIP_TRY(hipMemsetAsync(d_unoccluded, 0, (size_t)n * sizeof(unsigned int), st));
  AoParams P;
  std::memset(&P, 0, sizeof P);
  query_scene_params(P, sc, *C);
  P.points = d_points; P.dirs = a->d_dirs; P.out = d_unoccluded;
  P.n = n;
  P.total = n * a->k;
  P.bias = a->bias;
  P.k = a->k; P.n_sets = a->n_sets; P.seed = a->seed;
  P.dir_bytes = (uint32_t)a->n_sets * (uint32_t)a->k * 24u;
  const unsigned blocks = query_grid(sc, (P.total + kBlock - 1) / kBlock, ao_blocks_per_cu());
  hipLaunchKernelGGL(ao_kernel, dim3(blocks), dim3(kBlock), 0, st, P);
  return query_finish(sc, *C, st, P.total, stats);
}

}  // extern "C"
