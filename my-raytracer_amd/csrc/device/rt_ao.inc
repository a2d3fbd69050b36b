// rt_ao.inc — occlusion fans generated on the device (rt_trace_ao, rt_ao_rays_host, include/rt_hip.h;
// DESIGN.md §19).  Part of rt_render.hip's translation unit, included after rt_query.inc: the kernel
// uses that file's stack ring, top treelet, counters and query contexts and the render path's device
// helpers unchanged.
//
// One kernel: work item j in [0, n k) is sample j % k of point j / k, consecutive lanes on
// consecutive samples, so a wave holds 64 fan rays of at most ceil(64 / k) + 1 points and no lane
// idles for any k.  A lane builds its ray in registers (rt_ao_fan.hpp), walks the hierarchy with the
// any-hit traversal of query_kernel<true> -- the same text, so a fan ray is occluded exactly when
// rt_trace_occluded says so of the ray rt_ao_rays_host writes out -- and the wave reduces: a ballot
// of the lanes that are not occluded, and per point one popcount of its run of lanes.
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
  {   // once per block: the top treelet -> LDS
    const float4* src = reinterpret_cast<const float4*>(P.nodes4);
    for (int i = threadIdx.x; i < P.n_top * (int)(sizeof(GNode4) / sizeof(float4)); i += kBlock) q_top[i] = src[i];
    __syncthreads();
  }
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
    // ---- from here to the reduction: the any-hit branch of query_kernel (rt_query.inc) ----
    // degenerate rays are misses and are never traversed
    const double dlen = sqrt(dot(dv, dv));
    const bool act = act0 && q_finite(ro.x) && q_finite(ro.y) && q_finite(ro.z) && q_finite(dv.x) &&
                     q_finite(dv.y) && q_finite(dv.z) && dlen > 0.0 && tmax > 1e-5;   // NaN tmax: false
    const D3 rd = normalize(dv);
    // a hit counts iff 1e-5 < t < tmax; t = DBL_MAX is never one (the oracle's "no hit" value)
    const double tlim = tmax < DBL_MAX ? tmax : DBL_MAX;
    bool occluded = false;
    uint32_t cur = kDone;
    double t_off = 0.0;
    // analytic primitives first, in scene order: a ray they block skips the hierarchy
    for (int k = 0; k < P.n_prims; ++k) {
      if (!act || occluded) break;
      const double tp = prim_hit(P.prims[k], ro, rd);
      if (tp < tlim) { occluded = true; break; }
    }
    if (act && P.n_gnodes > 0 && !occluded) {   // conservative fp32 box ray (oracle gray_setup)
      bool miss = false;
      const double o3[3] = {ro.x, ro.y, ro.z}, d3v[3] = {rd.x, rd.y, rd.z};
      bool inside = true;
#pragma unroll
      for (int k = 0; k < 3; ++k)
        if (!(o3[k] >= P.root_lo[k] && o3[k] <= P.root_hi[k])) inside = false;
      if (!inside) {
        double tn = -DBL_MAX, tf = DBL_MAX;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          if (d3v[k] == 0.0) {
            if (o3[k] < P.root_lo[k] || o3[k] > P.root_hi[k]) miss = true;
            continue;
          }
          double t0 = (P.root_lo[k] - o3[k]) / d3v[k];
          double t1 = (P.root_hi[k] - o3[k]) / d3v[k];
          if (t0 > t1) { const double tt = t0; t0 = t1; t1 = tt; }
          if (t0 > tn) tn = t0;
          if (t1 < tf) tf = t1;
        }
        if (tn > tf || tf < 0.0) miss = true;
        t_off = tn > 0.0 ? tn : 0.0;
      }
      if (miss) t_off = 0.0;
      else cur = 0;
    }
    float inv[3];
    {
      const double d3v[3] = {rd.x, rd.y, rd.z};
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        float df = (float)d3v[k];
        if (fabsf(df) < 1e-20f) df = signbit(d3v[k]) ? -1e-20f : 1e-20f;
        const float r0 = __builtin_amdgcn_rcpf(df);   // v_rcp_f32 + one Newton step
        inv[k] = __builtin_fmaf(__builtin_fmaf(-df, r0, 1.0f), r0, r0);
      }
    }
    const float ofx = (float)(ro.x + t_off * rd.x);
    const float ofy = (float)(ro.y + t_off * rd.y);
    const float ofz = (float)(ro.z + t_off * rd.z);
    const float ivx = inv[0], ivy = inv[1], ivz = inv[2];
    // per-ray near / far plane byte offsets in the node and o * inv: one FMA per slab
    const uint32_t nxo = ivx >= 0.f ? 0u : 16u, nyo = ivy >= 0.f ? 32u : 48u, nzo = ivz >= 0.f ? 64u : 80u;
    const float oix = ofx * ivx, oiy = ofy * ivy, oiz = ofz * ivz;
    const float lo_c = round_down_f(-t_off);
    const float hi_c = round_up_f(tlim - t_off);
    // logical stack [0, sp): the LDS ring holds [slo, sp), spill[] holds [0, slo)
    uint32_t sp = 0, slo = 0;
    bool overflow = false;
    auto ring = [&](uint32_t i) -> uint32_t& { return q_ring[(i & (uint32_t)kQRingMask) * kBlock + threadIdx.x]; };
    auto push = [&](uint32_t x) {
      if (sp - slo == (uint32_t)kQRing) {   // ring full: its bottom entry goes to the spill stack
        if ((int)slo < P.spill_rows) spill[(size_t)slo * P.nslots] = ring(slo);
        else overflow = true;   // deeper than the hierarchy's bound (never on a sound hierarchy)
        slo++;
        n_spills++;
      }
      ring(sp) = x;
      sp++;
    };
    auto pop = [&]() -> uint32_t {
      if (sp == 0) return kDone;
      sp--;
      if (sp >= slo) return ring(sp);
      slo = sp;
      return (int)sp < P.spill_rows ? spill[(size_t)sp * P.nslots] : kDone;
    };
    const D3 c3 = d3(-rd.x, -rd.y, -rd.z);
    auto guard_trip = [&]() {
      if (lane == __ffsll((long long)wballot(1)) - 1) {
        trip_watchdog(P.ctr, P.guard_host);
        n_trips++;
      }
    };
    // tests the records of leaf `lref` in order; true = the ray is blocked
    auto test_leaf = [&](uint32_t lref) -> bool {
      uint32_t i = lref & ~kLeaf;
      // a linear scan to the record flagged last of its leaf: it cannot cycle
      for (;;) {
        const TriOps T = load_tri(P.tris, i);
        // Mesh::intersect_triangle: the CPU's fp64 S, Da, Db, Dt (same operands, same order), with
        // the render kernel's division-free early rejections, which fire only where the CPU's
        // quotients certainly fail (DESIGN.md §4)
        D3 c4 = sub(ro, T.p2);
        const double S = det3(T.e1, T.e2, c3);
        asm volatile("" : "+v"(c4.x), "+v"(c4.y), "+v"(c4.z));   // the record's loads stay one batch
        if (fabs(S) >= 1e-10) {
          const double Da = det3(c4, T.e2, c3);
          const double Db = det3(T.e1, c4, c3);
          const double sS = S > 0.0 ? 1.0 : -1.0;
          const double aS = fabs(S);
          const double ua = Da * sS, ub = Db * sS;
          const double tiny = aS * 0x1p-1000, big = aS * (1.0 + 0x1p-48);
          const bool out = (ua < 0.0 && -ua >= tiny) || (ub < 0.0 && -ub >= tiny) || ua > big || ub > big ||
                           (Da + Db - S) * sS > 0x1p-40 * (fabs(Da) + fabs(Db) + aS);
          if (!out) {
            const double Dt = det3(T.e1, T.e2, c4);
            const double th = Dt / S;
            if (th > 1e-5 && th < tlim) {
              double alpha, beta;
              // one reciprocal of S for both quotients where that is bit-identical (rt_render.hip)
              const double lim = aS * 0x1p-900;
              if (fabs(Da) >= lim && fabs(Db) >= lim && aS < 0x1p1000) {
                const double r = rcp_refined(S);
                alpha = div_by(Da, S, r);
                beta = div_by(Db, S, r);
              } else {
                alpha = Da / S;
                beta = Db / S;
              }
              const double gamma = (1.0 - alpha - beta);
              const bool in = (0.0 <= alpha && alpha <= 1.0) && (0.0 <= beta && beta <= 1.0) &&
                              (0.0 <= gamma && gamma <= 1.0);
              if (in) return true;
            }
          }
        }
        if (T.meta & kLastDev) break;
        ++i;
      }
      return false;
    };
    uint32_t pleaf = kDone;   // postponed leaf
    uint32_t rounds = 0;
    while ((wballot(cur != kDone) | wballot(pleaf != kDone)) != 0) {
      if (++rounds > kTravGuard) {   // watchdog: abandon the rays (results void, scene flagged)
        guard_trip();
        cur = kDone;
        pleaf = kDone;
        break;
      }
      for (uint32_t it = 0; !(cur & kLeaf); ++it) {   // 4-wide node (kDone carries the leaf bit)
        if (it > kTravGuard) { guard_trip(); cur = kDone; pleaf = kDone; break; }
        uint32_t v[4];
        bool hb[4];
        float4 nx, fx, ny, fy, nz, fz;
        uint4 rf;
        const uint32_t nbo = cur * (uint32_t)sizeof(GNode4);
        // wave-uniform: every active lane's node is in the LDS treelet
        const bool in_lds = wballot(cur >= (uint32_t)P.n_top) == 0;
        const char* nbase = reinterpret_cast<const char*>(P.nodes4);
#define RT_AONODE_AT(off) (nbase + (uint32_t)(nbo + (off)))
        if (in_lds) {
          const unsigned char* lb = reinterpret_cast<const unsigned char*>(q_top) + nbo;
          nx = *reinterpret_cast<const float4*>(lb + nxo);
          fx = *reinterpret_cast<const float4*>(lb + (nxo ^ 16u));
          ny = *reinterpret_cast<const float4*>(lb + nyo);
          fy = *reinterpret_cast<const float4*>(lb + (nyo ^ 16u));
          nz = *reinterpret_cast<const float4*>(lb + nzo);
          fz = *reinterpret_cast<const float4*>(lb + (nzo ^ 16u));
          rf = *reinterpret_cast<const uint4*>(lb + 96);
        } else {
          nx = *reinterpret_cast<const float4*>(RT_AONODE_AT(nxo));
          fx = *reinterpret_cast<const float4*>(RT_AONODE_AT(nxo ^ 16u));
          ny = *reinterpret_cast<const float4*>(RT_AONODE_AT(nyo));
          fy = *reinterpret_cast<const float4*>(RT_AONODE_AT(nyo ^ 16u));
          nz = *reinterpret_cast<const float4*>(RT_AONODE_AT(nzo));
          fz = *reinterpret_cast<const float4*>(RT_AONODE_AT(nzo ^ 16u));
          rf = *reinterpret_cast<const uint4*>(RT_AONODE_AT(96u));
        }
#undef RT_AONODE_AT
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const float tx0 = __builtin_fmaf(f4c(nx, c), ivx, -oix), tx1 = __builtin_fmaf(f4c(fx, c), ivx, -oix);
          const float ty0 = __builtin_fmaf(f4c(ny, c), ivy, -oiy), ty1 = __builtin_fmaf(f4c(fy, c), ivy, -oiy);
          const float tz0 = __builtin_fmaf(f4c(nz, c), ivz, -oiz), tz1 = __builtin_fmaf(f4c(fz, c), ivz, -oiz);
          const float tn = fmaxf(fmaxf(tx0, ty0), fmaxf(tz0, lo_c));
          const float tf = fminf(fminf(tx1, ty1), fminf(tz1, hi_c));
          hb[c] = tn <= tf;   // absent children carry the empty box [+inf, -inf]
          v[c] = u4c(rf, c);
        }
        {   // any visit order gives the same answer: no sort
          uint32_t nxt = kDone;
#pragma unroll
          for (int c = 0; c < 4; ++c)
            if (hb[c]) {
              if (nxt != kDone) push(nxt);
              nxt = v[c];
            }
          cur = nxt == kDone ? pop() : nxt;
        }
        if ((cur & kLeaf) && cur != kDone && pleaf == kDone) {   // first leaf: postpone, keep going
          pleaf = cur;
          cur = pop();
        }
        if ((wballot(pleaf == kDone) & wballot(cur != kDone)) == 0) break;   // every lane holds a leaf
      }
      if (pleaf == kDone && cur != kDone) {   // stopped at a leaf without postponing one
        pleaf = cur;
        cur = pop();
      }
      while (pleaf != kDone) {
        if (test_leaf(pleaf)) {   // blocked: finished
          occluded = true;
          cur = kDone;
          pleaf = kDone;
          break;
        }
        pleaf = kDone;
        if ((cur & kLeaf) && cur != kDone) {
          pleaf = cur;
          cur = pop();
        }
      }
    }
    if (overflow) guard_trip();
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
  // counters: summed per wave, one atomic per wave and counter
  const unsigned long long w_hits = wave_sum(n_hits), w_spills = wave_sum(n_spills), w_trips = wave_sum(n_trips);
  if (lane == 0) {
    if (w_hits) atomicAdd(&P.ctr[QC_HITS], w_hits);
    if (w_spills) atomicAdd(&P.ctr[QC_SPILLS], w_spills);
    if (w_trips) atomicAdd(&P.ctr[QC_WATCHDOG], w_trips);
  }
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

// blocks of ao_kernel that fill one CU (a property of the kernel and the architecture)
int ao_blocks_per_cu() {
  static const int blocks = [] {
    const void* fn = reinterpret_cast<const void*>(&ao_kernel);
    int nb = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, fn, kBlock, 0) != hipSuccess || nb < 1) nb = 1;
    hipFuncAttributes fa;
    if (hipFuncGetAttributes(&fa, fn) == hipSuccess && fa.numRegs > 0) {
      const int waves_per_simd = 512 / ((fa.numRegs + 7) / 8 * 8);
      nb = std::min(nb, std::max(1, waves_per_simd * 4 / (kBlock / 64)));
    }
    return std::min(nb, (int)(160 * 1024 / (kQRing * kBlock * sizeof(uint32_t) + kQTop * sizeof(GNode4))));
  }();
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
  HIP_TRY(hipSetDevice(sc->device));
  const int irc = query_ring_init(sc);
  if (irc != RT_OK) return irc;
  QueryRing& Q = *sc->query;
  QueryCtx& C = Q.ctx[Q.next];
  Q.next = (Q.next + 1) % kQContexts;
  // the context's previous query done before its counters and spill array are reused
  if (C.used && !event_done(C.done)) HIP_TRY(hipStreamWaitEvent(st, C.done, 0));
  HIP_TRY(hipMemsetAsync(C.d_ctr, 0, QC_WORDS * sizeof(unsigned long long), st));
  // a run of k lanes that 64 does not divide may straddle waves: those points are summed by atomics
  if (64 % a->k != 0) HIP_TRY(hipMemsetAsync(d_unoccluded, 0, (size_t)n * sizeof(unsigned int), st));
  AoParams P;
  std::memset(&P, 0, sizeof P);
  P.nodes4 = sc->d_nodes4; P.tris = sc->d_tris; P.prims = sc->d_prims;
  P.points = d_points; P.dirs = a->d_dirs; P.out = d_unoccluded;
  P.ctr = C.d_ctr; P.spill = C.d_spill; P.guard_host = sc->d_guard;
  P.nslots = Q.nslots;
  P.n = n;
  P.total = n * a->k;
  P.bias = a->bias;
  P.k = a->k; P.n_sets = a->n_sets; P.seed = a->seed;
  P.dir_bytes = (uint32_t)a->n_sets * (uint32_t)a->k * 24u;
  P.spill_rows = Q.spill_rows;
  P.n_gnodes = sc->n_gnodes; P.n_prims = sc->n_prims;
  P.n_top = std::min(kQTop, sc->n_top_v[0]);   // as the queries
  for (int k = 0; k < 3; ++k) { P.root_lo[k] = sc->root_lo[k]; P.root_hi[k] = sc->root_hi[k]; }
  // the grid that fills the device, inside the lanes the contexts' spill arrays were sized for
  const long long want = (P.total + kBlock - 1) / kBlock;
  const long long full = std::min<long long>((long long)std::max(1, sc->n_cu) * ao_blocks_per_cu(),
                                             (long long)(Q.nslots / kBlock));
  const unsigned blocks = (unsigned)std::max<long long>(1, std::min(want, full));
  hipLaunchKernelGGL(ao_kernel, dim3(blocks), dim3(kBlock), 0, st, P);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(C.done, st));
  C.used = true;
  if (stats) {
    HIP_TRY(hipStreamSynchronize(st));
    unsigned long long c[QC_WORDS];
    HIP_TRY(hipMemcpy(c, C.d_ctr, sizeof c, hipMemcpyDeviceToHost));
    stats->rays = P.total;
    stats->hits = (long long)c[QC_HITS];
    stats->stack_spills = (long long)c[QC_SPILLS];
    stats->watchdog = (long long)c[QC_WATCHDOG];
    if (c[CD_GUARD] != 0 || guard_tripped(sc)) return fail(RT_ERR_HIP, kGuardMsg);
  }
  return RT_OK;
}

}  // extern "C"
