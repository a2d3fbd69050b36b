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
// oldest entries spill to the query context's global array.
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

template <bool ANYHIT>
__global__ void __launch_bounds__(kBlock, kWavesPerEU * 256 / kBlock) query_kernel(QParams P) {
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
    // degenerate rays are misses and are never traversed
    const double dlen = sqrt(dot(dv, dv));
    const bool act = act0 && q_finite(ro.x) && q_finite(ro.y) && q_finite(ro.z) && q_finite(dv.x) &&
                     q_finite(dv.y) && q_finite(dv.z) && dlen > 0.0 && tmax > 1e-5;   // NaN tmax: false
    const D3 rd = normalize(dv);
    // a hit counts iff 1e-5 < t < tmax; t = DBL_MAX is never one (the oracle's "no hit" value)
    double tlim = tmax < DBL_MAX ? tmax : DBL_MAX;
    int best = kNoHit, best_slot = kNoHit, best_mesh = -1;
    double best_a = 0.0, best_b = 0.0;
    bool occluded = false;
    uint32_t cur = kDone;
    double t_off = 0.0;
    // analytic primitives first, in scene order (oracle intersect_scene): only a strictly closer
    // triangle replaces them; an occlusion ray they block skips the hierarchy
    for (int k = 0; k < P.n_prims; ++k) {
      if (!act || occluded) break;
      const double t = prim_hit(P.prims[k], ro, rd);
      if (t < tlim) {
        if (ANYHIT) { occluded = true; break; }
        tlim = t;
        best = kPrimHit | k;
        best_slot = -1;
      }
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
          if (t0 > t1) { const double t = t0; t0 = t1; t1 = t; }
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
    float hi_c = round_up_f(tlim - t_off);   // tightened as tlim shrinks
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
    // tests the records of leaf `lref` in order; true = the occlusion ray is blocked
    auto test_leaf = [&](uint32_t lref) -> bool {
      uint32_t i = lref & ~kLeaf;
      // a linear scan to the record flagged last of its leaf: it cannot cycle
      for (;;) {
        const TriOps T = load_tri(P.tris, i);
        const int slot = (int)(T.meta & kSlotMask);
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
            const double t = Dt / S;
            const bool cand = ANYHIT ? (t < tlim) : (t <= tlim);
            if (t > 1e-5 && cand) {
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
              if (in) {
                if (ANYHIT) return true;
                // strictly closer, or a tie with an earlier hit: smallest reference slot
                if (t < tlim || (best != kNoHit && slot < best_slot)) {
                  tlim = t;
                  best = (int)i;
                  best_slot = slot;
                  best_mesh = T.mesh;
                  best_a = alpha;
                  best_b = beta;
                  hi_c = round_up_f(tlim - t_off);
                }
              }
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
        float k[4];
        uint32_t v[4];
        bool hb[4];
        int cnt = 0;
        float4 nx, fx, ny, fy, nz, fz;
        uint4 rf;
        const uint32_t nbo = cur * (uint32_t)sizeof(GNode4);
        // wave-uniform: every active lane's node is in the LDS treelet
        const bool in_lds = wballot(cur >= (uint32_t)P.n_top) == 0;
        const char* nbase = reinterpret_cast<const char*>(P.nodes4);
#define RT_QNODE_AT(off) (nbase + (uint32_t)(nbo + (off)))
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
          nx = *reinterpret_cast<const float4*>(RT_QNODE_AT(nxo));
          fx = *reinterpret_cast<const float4*>(RT_QNODE_AT(nxo ^ 16u));
          ny = *reinterpret_cast<const float4*>(RT_QNODE_AT(nyo));
          fy = *reinterpret_cast<const float4*>(RT_QNODE_AT(nyo ^ 16u));
          nz = *reinterpret_cast<const float4*>(RT_QNODE_AT(nzo));
          fz = *reinterpret_cast<const float4*>(RT_QNODE_AT(nzo ^ 16u));
          rf = *reinterpret_cast<const uint4*>(RT_QNODE_AT(96u));
        }
#undef RT_QNODE_AT
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const float tx0 = __builtin_fmaf(f4c(nx, c), ivx, -oix), tx1 = __builtin_fmaf(f4c(fx, c), ivx, -oix);
          const float ty0 = __builtin_fmaf(f4c(ny, c), ivy, -oiy), ty1 = __builtin_fmaf(f4c(fy, c), ivy, -oiy);
          const float tz0 = __builtin_fmaf(f4c(nz, c), ivz, -oiz), tz1 = __builtin_fmaf(f4c(fz, c), ivz, -oiz);
          const float tn = fmaxf(fmaxf(tx0, ty0), fmaxf(tz0, lo_c));
          const float tf = fminf(fminf(tx1, ty1), fminf(tz1, hi_c));
          const bool h = tn <= tf;   // absent children carry the empty box [+inf, -inf]
          hb[c] = h;
          k[c] = h ? tn : INFINITY;
          v[c] = u4c(rf, c);
          cnt += h ? 1 : 0;
        }
        if (ANYHIT) {   // any visit order gives the same answer: no sort
          uint32_t nxt = kDone;
#pragma unroll
          for (int c = 0; c < 4; ++c)
            if (hb[c]) {
              if (nxt != kDone) push(nxt);
              nxt = v[c];
            }
          cur = nxt == kDone ? pop() : nxt;
        } else {   // nearest child first, the others pushed far-first
#define RT_QCSWAP(a, b)                                       \
  if (k[b] < k[a]) {                                          \
    const float tk = k[a]; k[a] = k[b]; k[b] = tk;            \
    const uint32_t tv = v[a]; v[a] = v[b]; v[b] = tv;         \
  }
          RT_QCSWAP(0, 1) RT_QCSWAP(2, 3) RT_QCSWAP(0, 2) RT_QCSWAP(1, 3) RT_QCSWAP(1, 2)
#undef RT_QCSWAP
          if (cnt == 0) {
            cur = pop();
          } else {
            if (cnt > 3) push(v[3]);
            if (cnt > 2) push(v[2]);
            if (cnt > 1) push(v[1]);
            cur = v[0];
          }
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
        if (test_leaf(pleaf)) {   // occlusion ray blocked: finished
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

    if (ANYHIT) {
      if (act0) P.occ[base + threadIdx.x] = occluded ? 1 : 0;
      n_hits += occluded ? 1u : 0u;
    } else {
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
  // counters: summed per wave, one atomic per wave and counter
  const unsigned long long w_hits = wave_sum(n_hits), w_spills = wave_sum(n_spills), w_trips = wave_sum(n_trips);
  if (lane == 0) {
    if (w_hits) atomicAdd(&P.ctr[QC_HITS], w_hits);
    if (w_spills) atomicAdd(&P.ctr[QC_SPILLS], w_spills);
    if (w_trips) atomicAdd(&P.ctr[QC_WATCHDOG], w_trips);
  }
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

int query_ring_init(rt_scene* sc) {
  if (sc->query) return RT_OK;
  auto* Q = new QueryRing();
  sc->query = Q;   // rt_scene_free releases whatever a failed initialisation leaves
  const void* fns[2] = {reinterpret_cast<const void*>(&query_kernel<false>),
                        reinterpret_cast<const void*>(&query_kernel<true>)};
  for (int v = 0; v < 2; ++v) {   // the grid that fills the device, as the render launch sizes its own
    int nb = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, fns[v], kBlock, 0) != hipSuccess || nb < 1) nb = 1;
    hipFuncAttributes fa;
    if (hipFuncGetAttributes(&fa, fns[v]) == hipSuccess && fa.numRegs > 0) {
      const int waves_per_simd = 512 / ((fa.numRegs + 7) / 8 * 8);
      nb = std::min(nb, std::max(1, waves_per_simd * 4 / (kBlock / 64)));
    }
    nb = std::min(nb, (int)(160 * 1024 / (kQRing * kBlock * sizeof(uint32_t) + kQTop * sizeof(GNode4))));
    Q->grid[v] = (long long)std::max(1, sc->n_cu) * nb;
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
  HIP_TRY(hipSetDevice(sc->device));
  const int irc = query_ring_init(sc);
  if (irc != RT_OK) return irc;
  QueryRing& Q = *sc->query;
  QueryCtx& C = Q.ctx[Q.next];
  Q.next = (Q.next + 1) % kQContexts;
  // the context's previous query done before its counters and spill array are reused
  if (C.used && !event_done(C.done)) HIP_TRY(hipStreamWaitEvent(st, C.done, 0));
  HIP_TRY(hipMemsetAsync(C.d_ctr, 0, QC_WORDS * sizeof(unsigned long long), st));
  QParams P;
  std::memset(&P, 0, sizeof P);
  P.nodes4 = sc->d_nodes4; P.tris = sc->d_tris; P.tnorm = sc->d_tnorm; P.mats = sc->d_mats; P.prims = sc->d_prims;
  P.rays = d_rays; P.hits = d_hits; P.occ = d_occ;
  P.ctr = C.d_ctr; P.spill = C.d_spill; P.guard_host = sc->d_guard;
  P.nslots = Q.nslots;
  P.n = n;
  P.spill_rows = Q.spill_rows;
  P.n_gnodes = sc->n_gnodes; P.n_prims = sc->n_prims;
  P.n_top = std::min(kQTop, sc->n_top_v[0]);   // the production render variant's count (rt_upload_options.lds_treelet)
  for (int k = 0; k < 3; ++k) { P.root_lo[k] = sc->root_lo[k]; P.root_hi[k] = sc->root_hi[k]; }
  const long long want = (n + kBlock - 1) / kBlock;
  const unsigned blocks = (unsigned)std::max<long long>(1, std::min<long long>(want, Q.grid[anyhit ? 1 : 0]));
  if (anyhit) hipLaunchKernelGGL(query_kernel<true>, dim3(blocks), dim3(kBlock), 0, st, P);
  else hipLaunchKernelGGL(query_kernel<false>, dim3(blocks), dim3(kBlock), 0, st, P);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(C.done, st));
  C.used = true;
  if (stats) {
    HIP_TRY(hipStreamSynchronize(st));
    unsigned long long c[QC_WORDS];
    HIP_TRY(hipMemcpy(c, C.d_ctr, sizeof c, hipMemcpyDeviceToHost));
    stats->rays = n;
    stats->hits = (long long)c[QC_HITS];
    stats->stack_spills = (long long)c[QC_SPILLS];
    stats->watchdog = (long long)c[QC_WATCHDOG];
    if (c[CD_GUARD] != 0 || guard_tripped(sc)) return fail(RT_ERR_HIP, kGuardMsg);
  }
  return RT_OK;
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
