// rt_hits.inc — the k nearest hits of each ray, resumable past k (rt_trace_hits, include/rt_hip.h;
// DESIGN.md §27).  Part of rt_render.hip's translation unit, included after rt_query.inc: the kernel
// uses that file's stack ring, top treelet, counters, query contexts and launch steps and the render
// path's device helpers unchanged.
//
// One kernel: 256-thread blocks, one ray per lane, query_kernel's grid-stride loop.  The walk is
// rt_walk_body.inc in closest-hit mode with RT_WALK_KHITS defined: a triangle the fp64 test accepts
// goes into the lane's k-buffer, the k smallest (t, reference slot) keys past the resume key, kept
// sorted in LDS as [entry][kBlock] planes (a lane's entries kBlock elements apart, as the stack
// ring: no bank conflict, no register array indexed at run time).  Until the buffer is full the far
// bound is the ray's tmax; from then on it is the last entry's t, inclusive, and only shrinks -- an
// entry that fell off the end is never offered again below the bound, so the SBVH's duplicate
// records are told by a slot compare against the kept entries alone.  The epilogue makes each kept
// entry's rt_hit from its record with the walk's own operations (the same S, Da, Db and quotients:
// the bits rt_trace_closest gives that triangle).
static_assert(sizeof(rt_hit_key) == 16 && offsetof(rt_hit_key, slot) == 8, "rt_hit_key is 16 bytes: t, slot");
static_assert(RT_HITS_MAX_ROWS <= (1LL << 31), "a ray's first row index times 64 bytes is added to a 64-bit pointer");

namespace {

constexpr int kHitsK = RT_HITS_MAX_K;
// LDS of a block: the k-buffer (16 B per entry and lane), the stack ring and the treelet
constexpr size_t kHitsLds =
    (size_t)kHitsK * kBlock * 16 + kQRing * kBlock * sizeof(uint32_t) + kQTop * sizeof(GNode4);
// blocks that LDS lets a CU hold, as waves per SIMD: the register budget the compiler may use
constexpr int kHitsWavesPerEU = (int)(160 * 1024 / kHitsLds) * (kBlock / 64) / 4;
static_assert(kHitsWavesPerEU >= 1, "one block of hits_kernel fits a CU's LDS");
static_assert((size_t)kBlock * kHitsK * sizeof(rt_hit) < (1u << 31), "a block's rows are one raw buffer");

struct HitsParams {
  const GNode4* nodes4;
  const GTri* tris;
  const double* tnorm;       // [record][12]: face normal, then the 3 vertex normals
  const GMat* mats;
  const GPrim* prims;        // (not read: a scene with primitives is refused)
  const rt_ray* rays;
  const rt_hit_key* after;   // [n] resume keys, or null
  rt_hit* hits;              // [n][k]
  unsigned int* count;       // [n]
  unsigned long long* ctr;   // [QC_WORDS]
  uint32_t* spill;           // [spill_rows][nslots] stack entries below the LDS ring
  unsigned int* guard_host;  // the scene's watchdog word (trip_watchdog)
  size_t nslots;             // lanes of the query contexts' spill array
  long long n;
  int k;                     // 1 .. kHitsK
  int spill_rows;
  int n_gnodes, n_prims;
  int n_top;                 // 4-wide nodes cached in LDS (ids [0, n_top), at most kQTop)
  double root_lo[3], root_hi[3];
};

__global__ void __launch_bounds__(kBlock, kHitsWavesPerEU) hits_kernel(HitsParams P) {
  __shared__ uint32_t q_ring[kQRing * kBlock];   // [entry][kBlock]: a lane's entries kBlock words apart
  __shared__ float4 q_top[kQTop * (sizeof(GNode4) / sizeof(float4))];
  // the k-buffer, sorted ascending by (t, slot): three planes [entry][kBlock]
  __shared__ double kh_t[kHitsK * kBlock];
  __shared__ int kh_slot[kHitsK * kBlock];
  __shared__ uint32_t kh_rec[kHitsK * kBlock];   // the device record the entry was accepted from
  query_stage_treelet(q_top, P);
  const int lane = threadIdx.x & 63;
  uint32_t* const spill = P.spill + (size_t)blockIdx.x * kBlock + threadIdx.x;
  unsigned long long n_hits = 0, n_spills = 0, n_trips = 0;
  const int k = P.k;
  const uint32_t row_bytes = (uint32_t)k * (uint32_t)sizeof(rt_hit);

  for (long long base = (long long)blockIdx.x * kBlock; base < P.n; base += (long long)gridDim.x * kBlock) {
    // this block's 256 rays, keys and rows as raw buffers: the base is wave-uniform, a lane's offset
    // one VGPR, and the hardware drops the accesses of the lanes past the last ray
    const long long left = P.n - base;
    const int nb = left < (long long)kBlock ? (int)left : kBlock;
    const bool act0 = (int)threadIdx.x < nb;
    const __amdgpu_buffer_rsrc_t rr = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<rt_ray*>(P.rays + base), 0, nb * (int)sizeof(rt_ray), kBufWord3);
    const uint32_t vo = threadIdx.x * (uint32_t)sizeof(rt_ray);
    const D2 q0 = buf_ld2(rr, vo, 0), q1 = buf_ld2(rr, vo + 16u, 0), q2 = buf_ld2(rr, vo + 32u, 0),
             q3 = buf_ld2(rr, vo + 48u, 0);
    const D3 ro = d3(q0.a, q0.b, q1.a);
    const D3 dv = d3(q1.b, q2.a, q2.b);
    const double tmax = q3.a;
    // the resume key: only (t, slot) greater than it belongs to the list (NaN t: nothing does)
    double kh_after_t = -INFINITY;
    int kh_after_slot = -1;
    if (P.after) {
      const __amdgpu_buffer_rsrc_t ar = __builtin_amdgcn_make_buffer_rsrc(
          const_cast<rt_hit_key*>(P.after + base), 0, nb * (int)sizeof(rt_hit_key), kBufWord3);
      const D2 a = buf_ld2(ar, threadIdx.x * (uint32_t)sizeof(rt_hit_key), 0);
      kh_after_t = a.a;
      kh_after_slot = (int)__builtin_bit_cast(u32x2_t, a.b).x;
    }
    int kh_n = 0;           // entries kept
    bool kh_full = false;   // kh_n == k
    double kh_last_t = 0.0;
    auto at = [&](int j) -> int { return j * kBlock + (int)threadIdx.x; };
    auto kh_insert = [&](double t, int slot, uint32_t rec) -> bool {
      // another record of a kept triangle (an SBVH duplicate: same operands, same t)
      for (int j = 0; j < kh_n; ++j)
        if (kh_slot[at(j)] == slot) return false;
      int j = kh_n;   // the free place, or the last entry's: it falls off
      if (kh_full) {
        j = k - 1;
        const int ls = kh_slot[at(j)];
        if (!(t < kh_last_t || (t == kh_last_t && slot < ls))) return false;
      } else {
        kh_n++;
        kh_full = kh_n == k;
      }
      for (; j > 0; --j) {   // the larger keys move up one place
        const double pt = kh_t[at(j - 1)];
        const int ps = kh_slot[at(j - 1)];
        if (pt < t || (pt == t && ps < slot)) break;
        kh_t[at(j)] = pt;
        kh_slot[at(j)] = ps;
        kh_rec[at(j)] = kh_rec[at(j - 1)];
      }
      kh_t[at(j)] = t;
      kh_slot[at(j)] = slot;
      kh_rec[at(j)] = rec;
      if (!kh_full) return false;
      kh_last_t = kh_t[at(k - 1)];
      return true;
    };
    constexpr bool ANYHIT = false;   // the walk of query_kernel<false>, keeping k keys instead of one
#define RT_WALK_KHITS 1
#include "rt_walk_body.inc"
#undef RT_WALK_KHITS
    (void)best; (void)best_slot; (void)best_mesh; (void)best_a; (void)best_b; (void)occluded;

    n_hits += (unsigned)kh_n;
    if (act0) P.count[base + threadIdx.x] = (unsigned int)kh_n;
    // the lane's k rows; 8-B vector stores (DESIGN.md §4 "path state")
    const __amdgpu_buffer_rsrc_t hr = __builtin_amdgcn_make_buffer_rsrc(
        P.hits + base * k, 0, nb * (int)row_bytes, kBufWord3);
    for (int j = 0; j < k; ++j) {
      double ht = INFINITY, ha = 0.0, hb2 = 0.0;
      D3 hn = d3(0.0, 0.0, 0.0);
      int o_slot = -1, o_mesh = -1;
      if (j < kh_n) {
        // alpha and beta again from the record: test_leaf's operations on test_leaf's operands
        const uint32_t rec = kh_rec[at(j)];
        const TriOps T = load_tri(P.tris, rec);
        const D3 c4 = sub(ro, T.p2);
        const double S = det3(T.e1, T.e2, c3);
        const double Da = det3(c4, T.e2, c3);
        const double Db = det3(T.e1, c4, c3);
        const double aS = fabs(S);
        const double lim = aS * 0x1p-900;
        if (fabs(Da) >= lim && fabs(Db) >= lim && aS < 0x1p1000) {
          const double r = rcp_refined(S);
          ha = div_by(Da, S, r);
          hb2 = div_by(Db, S, r);
        } else {
          ha = Da / S;
          hb2 = Db / S;
        }
        ht = kh_t[at(j)];
        o_slot = kh_slot[at(j)];
        o_mesh = T.mesh;
        const double gamma = (1.0 - ha - hb2);
        const double* nr = P.tnorm + 12 * (size_t)rec;
        if (P.mats[o_mesh].draw_mode == RT_DRAW_FLAT) {
          hn = d3(nr[0], nr[1], nr[2]);
        } else {   // alpha*vn0 + beta*vn1 + gamma*vn2, not renormalised
          hn = d3(ha * nr[3] + hb2 * nr[6] + gamma * nr[9], ha * nr[4] + hb2 * nr[7] + gamma * nr[10],
                  ha * nr[5] + hb2 * nr[8] + gamma * nr[11]);
        }
      }
      const uint32_t ho = threadIdx.x * row_bytes + (uint32_t)j * (uint32_t)sizeof(rt_hit);
      buf_st(hr, ho, 0, ht);
      buf_st(hr, ho + 8u, 0, ha);
      buf_st(hr, ho + 16u, 0, hb2);
      buf_st(hr, ho + 24u, 0, hn.x);
      buf_st(hr, ho + 32u, 0, hn.y);
      buf_st(hr, ho + 40u, 0, hn.z);
      buf_st(hr, ho + 48u, 0, q_pack(o_slot, o_mesh));
      buf_st(hr, ho + 56u, 0, q_pack(-1, 0));
    }
  }
  query_flush_counters(P, lane, n_hits, n_spills, n_trips);
}

int hits_blocks_per_cu() {
  static const int blocks = std::min(query_blocks_per_cu(reinterpret_cast<const void*>(&hits_kernel)),
                                     (int)(160 * 1024 / kHitsLds));
  return blocks;
}

}  // namespace

extern "C" {

int rt_trace_hits(rt_scene* sc, const rt_ray* d_rays, long long n, int k, const rt_hit_key* d_after, rt_hit* d_hits,
                  unsigned int* d_count, rt_query_stats* stats, void* stream) {
  if (!sc) return fail(RT_ERR_INVALID, "rt_trace_hits: null scene");
  if (n < 0) return fail(RT_ERR_INVALID, "rt_trace_hits: negative ray count");
  if (k < 1 || k > RT_HITS_MAX_K) return fail(RT_ERR_INVALID, "rt_trace_hits: k outside [1, RT_HITS_MAX_K]");
  if (n > RT_HITS_MAX_ROWS / k) return fail(RT_ERR_INVALID, "rt_trace_hits: n * k exceeds RT_HITS_MAX_ROWS");
  if (n > 0 && (!d_rays || !d_hits || !d_count))
    return fail(RT_ERR_INVALID, "rt_trace_hits: null ray, result or count buffer");
  if (stats) std::memset(stats, 0, sizeof *stats);
  if (n == 0) return RT_OK;
  if (sc->n_prims > 0)
    return fail(RT_ERR_UNSUPPORTED, "rt_trace_hits: the scene holds analytic primitives (their hit lists are not defined)");
  if (guard_tripped(sc)) return fail(RT_ERR_HIP, kGuardMsg);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  QueryCtx* C;
  const int arc = query_acquire(sc, st, &C);
  if (arc != RT_OK) return arc;
  HitsParams P;
  std::memset(&P, 0, sizeof P);
  query_scene_params(P, sc, *C);
  P.n_prims = 0;
  P.tnorm = sc->d_tnorm; P.mats = sc->d_mats;
  P.rays = d_rays; P.after = d_after; P.hits = d_hits; P.count = d_count;
  P.n = n;
  P.k = k;
  const unsigned blocks = query_grid(sc, (n + kBlock - 1) / kBlock, hits_blocks_per_cu());
  hipLaunchKernelGGL(hits_kernel, dim3(blocks), dim3(kBlock), 0, st, P);
  return query_finish(sc, *C, st, n, stats);
}

}  // extern "C"
