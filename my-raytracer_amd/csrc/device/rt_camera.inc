// rt_camera.inc — a camera's closest hits and surface points made on the device (rt_trace_camera,
// rt_camera_rays_host, rt_surface_points_host, include/rt_hip.h; DESIGN.md §22).  Part of
// rt_render.hip's translation unit, included after rt_ao.inc: the kernel uses rt_query.inc's stack
// ring, top treelet, counters and query contexts and the render path's device helpers unchanged.
//
// One kernel: a wave takes one kTileW x kTileH (8 x 8) tile of the shard's packed rows (the render
// kernel's work tile), a block four consecutive tiles, a bounded grid strides over the tiles.  A lane builds its pixel's
// primary ray in registers (rt_camera_point.hpp), walks the hierarchy with the closest-hit traversal
// of query_kernel<false> -- the same text, so the hit is rt_trace_closest's of the ray
// rt_camera_rays_host writes out -- and stores what the caller asked for: the 64-B rt_hit, the 64-B
// surface-point record, or both, in the frame's row order or in tile order.  Nothing is read per pixel.
#include "rt_camera_point.hpp"

namespace {

struct CamParams {
  const GNode4* nodes4;
  const GTri* tris;
  const double* tnorm;       // [record][12]: face normal, then the 3 vertex normals
  const GMat* mats;
  const GPrim* prims;
  rt_hit* hits;              // optional
  rt_ray* points;            // optional
  unsigned long long* ctr;   // [QC_WORDS]
  uint32_t* spill;           // [spill_rows][nslots] stack entries below the LDS ring
  unsigned int* guard_host;  // the scene's watchdog word (trip_watchdog)
  size_t nslots;             // lanes of the query contexts' spill array
  double eye[3], ll[3], xd[3], yd[3];
  double point_tmax;
  int W, rows;               // the shard: rows packed rows of W pixels
  uint32_t tiles_x, n_tiles;
  int row_begin, stripe_h, stripe_count, stripe_index;
  int tile_major;            // record order: 0 = the frame's rows, 1 = tile after tile
  int spill_rows;
  int n_gnodes, n_prims;
  int n_top;                 // 4-wide nodes cached in LDS (ids [0, n_top), at most kQTop)
  double root_lo[3], root_hi[3];
};

// the global row of the shard's packed row lrow (the render launch's mapping: rt_render_params)
__host__ __device__ inline int cam_global_row(int row_begin, int stripe_h, int stripe_count, int stripe_index, int lrow) {
  if (stripe_count == 1) return row_begin + lrow;
  const uint32_t st = (uint32_t)lrow / (uint32_t)stripe_h;
  return (int)((st * (uint32_t)stripe_count + (uint32_t)stripe_index) * (uint32_t)stripe_h +
               ((uint32_t)lrow - st * (uint32_t)stripe_h));
}

// Five waves per SIMD, the occupancy query_kernel<false> reaches on its own (94 VGPRs): asked for, the
// kernel fits the 96 VGPRs of that occupancy without scratch; left to the render kernels' bound of
// four it takes 100 (make resource-usage, DESIGN.md §22).
constexpr int kCamWavesPerEU = 5;
constexpr uint32_t kCamTilesPerBlock = kBlock / 64;   // one tile per wave

__global__ void __launch_bounds__(kBlock, kCamWavesPerEU * 256 / kBlock) camera_kernel(CamParams P) {
  __shared__ uint32_t q_ring[kQRing * kBlock];   // [entry][kBlock]: a lane's entries kBlock words apart
  __shared__ float4 q_top[kQTop * (sizeof(GNode4) / sizeof(float4))];
  {   // once per block: the top treelet -> LDS
    const float4* src = reinterpret_cast<const float4*>(P.nodes4);
    for (int i = threadIdx.x; i < P.n_top * (int)(sizeof(GNode4) / sizeof(float4)); i += kBlock) q_top[i] = src[i];
    __syncthreads();
  }
  const int lane = threadIdx.x & 63;
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  uint32_t* const spill = P.spill + (size_t)blockIdx.x * kBlock + threadIdx.x;
  unsigned long long n_hits = 0, n_spills = 0, n_trips = 0;

  for (uint32_t t0 = blockIdx.x * kCamTilesPerBlock; t0 < P.n_tiles; t0 += gridDim.x * kCamTilesPerBlock) {
    // this wave's tile: everything about it is wave-uniform, a lane's own pixel and record 32-bit
    const bool wave_on = t0 + wave < P.n_tiles;   // the last block's waves past the last tile idle
    const uint32_t tile = wave_on ? t0 + wave : 0u;
    const uint32_t ty = tile / P.tiles_x, tx = tile - ty * P.tiles_x;
    const uint32_t wl = (uint32_t)P.W - tx * (uint32_t)kTileW, rl = (uint32_t)P.rows - ty * (uint32_t)kTileH;
    // a partial tile at the right / top edge
    const uint32_t tw = wl < (uint32_t)kTileW ? wl : (uint32_t)kTileW;
    const uint32_t th = rl < (uint32_t)kTileH ? rl : (uint32_t)kTileH;
    // the tile's records: its first one (64-bit, wave-uniform) and the records from the first to the
    // tile's last, the window the stores are bounded by
    const long long first = P.tile_major ? (long long)ty * kTileH * P.W + (long long)tx * kTileW * th
                                         : (long long)ty * kTileH * P.W + (long long)tx * kTileW;
    const uint32_t span = P.tile_major ? tw * th : (th - 1u) * (uint32_t)P.W + tw;
    // lane ln's pixel of the tile and the byte offset of its record from the tile's first; true = the
    // tile has that pixel.  Evaluated before the walk for the ray and again after it for the stores,
    // so that only the lane number lives across the walk.
    auto pixel = [&](uint32_t ln, int& px, int& py, uint32_t& vo) -> bool {
      const uint32_t jx = ln & (uint32_t)(kTileW - 1), jy = ln >> kTileWLog;
      px = (int)(tx * (uint32_t)kTileW + jx);
      py = cam_global_row(P.row_begin, P.stripe_h, P.stripe_count, P.stripe_index, (int)(ty * (uint32_t)kTileH + jy));
      vo = (P.tile_major ? jy * tw + jx : jy * (uint32_t)P.W + jx) * (uint32_t)sizeof(rt_ray);
      return wave_on && jx < tw && jy < th;
    };
    int px, py;
    uint32_t vo_ray;
    const bool act0 = pixel((uint32_t)lane, px, py, vo_ray);
    double co[3], cd[3];
    rt_camera_ray(P.eye, P.ll, P.xd, P.yd, px, py, co, cd);
    const D3 ro = d3(co[0], co[1], co[2]);
    const D3 dv = d3(cd[0], cd[1], cd[2]);
    const double tmax = INFINITY;
    // ---- from here to the final hit: the closest-hit branch of query_kernel (rt_query.inc) ----
    // degenerate rays are misses and are never traversed
    const double dlen = sqrt(dot(dv, dv));
    const bool act = act0 && q_finite(ro.x) && q_finite(ro.y) && q_finite(ro.z) && q_finite(dv.x) &&
                     q_finite(dv.y) && q_finite(dv.z) && dlen > 0.0 && tmax > 1e-5;   // NaN tmax: false
    const D3 rd = normalize(dv);
    // a hit counts iff 1e-5 < t < tmax; t = DBL_MAX is never one (the oracle's "no hit" value)
    double tlim = tmax < DBL_MAX ? tmax : DBL_MAX;
    int best = kNoHit, best_slot = kNoHit, best_mesh = -1;
    double best_a = 0.0, best_b = 0.0;
    uint32_t cur = kDone;
    double t_off = 0.0;
    // analytic primitives first, in scene order (oracle intersect_scene): only a strictly closer
    // triangle replaces them
    for (int k = 0; k < P.n_prims; ++k) {
      if (!act) break;
      const double t = prim_hit(P.prims[k], ro, rd);
      if (t < tlim) {
        tlim = t;
        best = kPrimHit | k;
        best_slot = -1;
      }
    }
    if (act && P.n_gnodes > 0) {   // conservative fp32 box ray (oracle gray_setup)
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
          double t0b = (P.root_lo[k] - o3[k]) / d3v[k];
          double t1b = (P.root_hi[k] - o3[k]) / d3v[k];
          if (t0b > t1b) { const double t = t0b; t0b = t1b; t1b = t; }
          if (t0b > tn) tn = t0b;
          if (t1b < tf) tf = t1b;
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
    // tests the records of leaf `lref` in order
    auto test_leaf = [&](uint32_t lref) {
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
            if (t > 1e-5 && t <= tlim) {
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
        int cnt = 0;
        float4 nx, fx, ny, fy, nz, fz;
        uint4 rf;
        const uint32_t nbo = cur * (uint32_t)sizeof(GNode4);
        // wave-uniform: every active lane's node is in the LDS treelet
        const bool in_lds = wballot(cur >= (uint32_t)P.n_top) == 0;
        const char* nbase = reinterpret_cast<const char*>(P.nodes4);
#define RT_CAMNODE_AT(off) (nbase + (uint32_t)(nbo + (off)))
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
          nx = *reinterpret_cast<const float4*>(RT_CAMNODE_AT(nxo));
          fx = *reinterpret_cast<const float4*>(RT_CAMNODE_AT(nxo ^ 16u));
          ny = *reinterpret_cast<const float4*>(RT_CAMNODE_AT(nyo));
          fy = *reinterpret_cast<const float4*>(RT_CAMNODE_AT(nyo ^ 16u));
          nz = *reinterpret_cast<const float4*>(RT_CAMNODE_AT(nzo));
          fz = *reinterpret_cast<const float4*>(RT_CAMNODE_AT(nzo ^ 16u));
          rf = *reinterpret_cast<const uint4*>(RT_CAMNODE_AT(96u));
        }
#undef RT_CAMNODE_AT
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const float tx0 = __builtin_fmaf(f4c(nx, c), ivx, -oix), tx1 = __builtin_fmaf(f4c(fx, c), ivx, -oix);
          const float ty0 = __builtin_fmaf(f4c(ny, c), ivy, -oiy), ty1 = __builtin_fmaf(f4c(fy, c), ivy, -oiy);
          const float tz0 = __builtin_fmaf(f4c(nz, c), ivz, -oiz), tz1 = __builtin_fmaf(f4c(fz, c), ivz, -oiz);
          const float tn = fmaxf(fmaxf(tx0, ty0), fmaxf(tz0, lo_c));
          const float tf = fminf(fminf(tx1, ty1), fminf(tz1, hi_c));
          const bool h = tn <= tf;   // absent children carry the empty box [+inf, -inf]
          k[c] = h ? tn : INFINITY;
          v[c] = u4c(rf, c);
          cnt += h ? 1 : 0;
        }
        {   // nearest child first, the others pushed far-first
#define RT_CAMCSWAP(a, b)                                     \
  if (k[b] < k[a]) {                                          \
    const float tk = k[a]; k[a] = k[b]; k[b] = tk;            \
    const uint32_t tv = v[a]; v[a] = v[b]; v[b] = tv;         \
  }
          RT_CAMCSWAP(0, 1) RT_CAMCSWAP(2, 3) RT_CAMCSWAP(0, 2) RT_CAMCSWAP(1, 3) RT_CAMCSWAP(1, 2)
#undef RT_CAMCSWAP
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
        test_leaf(pleaf);
        pleaf = kDone;
        if ((cur & kLeaf) && cur != kDone) {
          pleaf = cur;
          cur = pop();
        }
      }
    }
    if (overflow) guard_trip();

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
    // ---- the final hit; what the caller asked for, one bounded raw buffer over the tile's records
    // each, 8-B vector stores (DESIGN.md §4 "path state"), the active lanes only: in row order the
    // window also holds the neighbouring tiles' records ----
    uint32_t ln = (uint32_t)lane;
    asm volatile("" : "+v"(ln));   // the pixel again from the lane number
    int qx, qy;
    uint32_t vo;
    const bool on = pixel(ln, qx, qy, vo);
    if (P.hits) {
      const __amdgpu_buffer_rsrc_t hr =
          __builtin_amdgcn_make_buffer_rsrc(P.hits + first, 0, (int)(span * (uint32_t)sizeof(rt_hit)), kBufWord3);
      if (on) {
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
    if (P.points) {
      // the ray again too (the same operations on the same operands: the same bits), so that its
      // unnormalised direction is not kept live across the walk, then the header
      double so[3], sd[3], sp3[3], sn[3];
      rt_camera_ray(P.eye, P.ll, P.xd, P.yd, qx, qy, so, sd);
      const double nrm[3] = {hn.x, hn.y, hn.z};
      rt_surface_point(so, sd, ht, nrm, sp3, sn);
      const __amdgpu_buffer_rsrc_t pr =
          __builtin_amdgcn_make_buffer_rsrc(P.points + first, 0, (int)(span * (uint32_t)sizeof(rt_ray)), kBufWord3);
      if (on) {
        buf_st(pr, vo, 0, sp3[0]);
        buf_st(pr, vo + 8u, 0, sp3[1]);
        buf_st(pr, vo + 16u, 0, sp3[2]);
        buf_st(pr, vo + 24u, 0, sn[0]);
        buf_st(pr, vo + 32u, 0, sn[1]);
        buf_st(pr, vo + 40u, 0, sn[2]);
        buf_st(pr, vo + 48u, 0, P.point_tmax);
        buf_st(pr, vo + 56u, 0, 0.0);
      }
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

// The shard of a camera call: what rt_trace_camera and rt_camera_rays_host read from the render
// parameters, checked as rt_launch_compute_image checks it (before any HIP call).
struct CamShard {
  int W, rows, row_begin, stripe_h, stripe_count, stripe_index;
  long long n;
};

int camera_shard(const std::string& who, const rt_render_params* p, int order, CamShard* S) {
  if (!p) return fail(RT_ERR_INVALID, who + ": null parameters");
  if (order != RT_CAMERA_ROW_MAJOR && order != RT_CAMERA_TILE_MAJOR)
    return fail(RT_ERR_INVALID, who + ": unknown order (RT_CAMERA_ROW_MAJOR or RT_CAMERA_TILE_MAJOR)");
  if (p->spp_n != 1) return fail(RT_ERR_INVALID, who + ": spp_n must be 1 (one ray through each pixel)");
  if (p->flags & ~RT_FLAG_NATURAL_ORDER) return fail(RT_ERR_INVALID, who + ": only RT_FLAG_NATURAL_ORDER is accepted");
  if (p->camera.width <= 0 || p->camera.height <= 0) return fail(RT_ERR_INVALID, who + ": bad image size (1..65535 per side)");
  const int scount = p->stripe_count > 0 ? p->stripe_count : 1;
  if (p->stripe_index < 0 || p->stripe_index >= scount) return fail(RT_ERR_INVALID, who + ": stripe_index out of range");
  if (scount > 1 && (p->row_begin != 0 || (p->row_end > 0 && p->row_end != p->camera.height)))
    return fail(RT_ERR_INVALID, who + ": row ranges cannot be combined with stripe_count > 1");
  S->W = p->camera.width;
  S->rows = rt_rows_in_shard(p);
  S->row_begin = scount == 1 ? std::max(0, p->row_begin) : 0;
  S->stripe_h = p->stripe_height > 0 ? p->stripe_height : 1;
  S->stripe_count = scount;
  S->stripe_index = p->stripe_index;
  S->n = (long long)S->rows * S->W;
  if (S->n > RT_CAMERA_MAX_PIXELS) return fail(RT_ERR_INVALID, who + ": more than RT_CAMERA_MAX_PIXELS pixels");
  if (p->camera.width > 65535 || p->camera.height > 65535)
    return fail(RT_ERR_INVALID, who + ": bad image size (1..65535 per side)");
  return RT_OK;
}

// the tmax of the point records: a point with tmax > 1e-5 false is degenerate whatever its hit
int camera_point_tmax_check(const std::string& who, double point_tmax) {
  if (!(point_tmax > 1e-5)) return fail(RT_ERR_INVALID, who + ": point_tmax must be > 1e-5");   // NaN: refused
  return RT_OK;
}

// blocks of camera_kernel that fill one CU (a property of the kernel and the architecture)
int camera_blocks_per_cu() {
  static const int blocks = [] {
    const void* fn = reinterpret_cast<const void*>(&camera_kernel);
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

int rt_camera_rays_host(const rt_render_params* p, int order, rt_ray* rays_out) {
  CamShard S;
  const int rc = camera_shard("rt_camera_rays_host", p, order, &S);
  if (rc != RT_OK) return rc;
  if (S.n > 0 && !rays_out) return fail(RT_ERR_INVALID, "rt_camera_rays_host: null ray buffer");
  const rt_camera& cam = p->camera;
  const int tiles_x = (S.W + kTileW - 1) / kTileW, tiles_y = (S.rows + kTileH - 1) / kTileH;
  for (int ty = 0; ty < tiles_y; ++ty) {
    const int th = std::min(kTileH, S.rows - ty * kTileH);
    for (int tx = 0; tx < tiles_x; ++tx) {
      const int tw = std::min(kTileW, S.W - tx * kTileW);
      const size_t first = order == RT_CAMERA_TILE_MAJOR ? (size_t)ty * kTileH * S.W + (size_t)tx * kTileW * th
                                                         : (size_t)ty * kTileH * S.W + (size_t)tx * kTileW;
      for (int jy = 0; jy < th; ++jy)
        for (int jx = 0; jx < tw; ++jx) {
          const size_t rec = order == RT_CAMERA_TILE_MAJOR ? (size_t)jy * tw + jx : (size_t)jy * S.W + jx;
          rt_ray& r = rays_out[first + rec];
          const int py = cam_global_row(S.row_begin, S.stripe_h, S.stripe_count, S.stripe_index, ty * kTileH + jy);
          rt_camera_ray(cam.eye, cam.lower_left, cam.x_dir, cam.y_dir, tx * kTileW + jx, py, r.o, r.d);
          r.tmax = INFINITY;
          r.reserved_ = 0.0;
        }
    }
  }
  return RT_OK;
}

int rt_surface_points_host(const rt_ray* rays, const rt_hit* hits, long long n, double point_tmax, rt_ray* points_out) {
  const std::string who("rt_surface_points_host");
  if (n < 0) return fail(RT_ERR_INVALID, who + ": negative record count");
  if (n > RT_CAMERA_MAX_PIXELS) return fail(RT_ERR_INVALID, who + ": more than RT_CAMERA_MAX_PIXELS records");
  const int rc = camera_point_tmax_check(who, point_tmax);
  if (rc != RT_OK) return rc;
  if (n > 0 && (!rays || !hits || !points_out)) return fail(RT_ERR_INVALID, who + ": null ray, hit or point buffer");
  for (long long i = 0; i < n; ++i) {
    rt_ray& pt = points_out[i];
    rt_surface_point(rays[i].o, rays[i].d, hits[i].t, hits[i].normal, pt.o, pt.d);
    pt.tmax = point_tmax;
    pt.reserved_ = 0.0;
  }
  return RT_OK;
}

int rt_trace_camera(rt_scene* sc, const rt_render_params* p, const rt_camera_out* out, rt_query_stats* stats,
                    void* stream) {
  const std::string who("rt_trace_camera");
  if (!sc) return fail(RT_ERR_INVALID, who + ": null scene");
  if (!p) return fail(RT_ERR_INVALID, who + ": null parameters");
  if (!out) return fail(RT_ERR_INVALID, who + ": null output description");
  if (!out->d_hits && !out->d_points) return fail(RT_ERR_INVALID, who + ": neither hits nor points requested");
  CamShard S;
  const int rc = camera_shard(who, p, out->order, &S);
  if (rc != RT_OK) return rc;
  if (out->d_points) {
    const int trc = camera_point_tmax_check(who, out->point_tmax);
    if (trc != RT_OK) return trc;
  }
  if (stats) std::memset(stats, 0, sizeof *stats);
  if (S.n == 0) return RT_OK;   // an empty row range: nothing to trace, the scene is not touched
  if (guard_tripped(sc)) return fail(RT_ERR_HIP, kGuardMsg);
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
  CamParams P;
  std::memset(&P, 0, sizeof P);
  P.nodes4 = sc->d_nodes4; P.tris = sc->d_tris; P.tnorm = sc->d_tnorm; P.mats = sc->d_mats; P.prims = sc->d_prims;
  P.hits = out->d_hits; P.points = out->d_points;
  P.ctr = C.d_ctr; P.spill = C.d_spill; P.guard_host = sc->d_guard;
  P.nslots = Q.nslots;
  for (int k = 0; k < 3; ++k) {
    P.eye[k] = p->camera.eye[k]; P.ll[k] = p->camera.lower_left[k];
    P.xd[k] = p->camera.x_dir[k]; P.yd[k] = p->camera.y_dir[k];
    P.root_lo[k] = sc->root_lo[k]; P.root_hi[k] = sc->root_hi[k];
  }
  P.point_tmax = out->point_tmax;
  P.W = S.W; P.rows = S.rows;
  P.tiles_x = (uint32_t)((S.W + kTileW - 1) / kTileW);
  P.n_tiles = P.tiles_x * (uint32_t)((S.rows + kTileH - 1) / kTileH);   // at most 2^26
  P.row_begin = S.row_begin; P.stripe_h = S.stripe_h; P.stripe_count = S.stripe_count; P.stripe_index = S.stripe_index;
  P.tile_major = out->order == RT_CAMERA_TILE_MAJOR ? 1 : 0;
  P.spill_rows = Q.spill_rows;
  P.n_gnodes = sc->n_gnodes; P.n_prims = sc->n_prims;
  P.n_top = std::min(kQTop, sc->n_top_v[0]);   // as the queries
  // the grid that fills the device, inside the lanes the contexts' spill arrays were sized for
  const long long want = ((long long)P.n_tiles + kCamTilesPerBlock - 1) / kCamTilesPerBlock;
  const long long full = std::min<long long>((long long)std::max(1, sc->n_cu) * camera_blocks_per_cu(),
                                             (long long)(Q.nslots / kBlock));
  const unsigned blocks = (unsigned)std::max<long long>(1, std::min(want, full));
  hipLaunchKernelGGL(camera_kernel, dim3(blocks), dim3(kBlock), 0, st, P);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(C.done, st));
  C.used = true;
  if (stats) {
    HIP_TRY(hipStreamSynchronize(st));
    unsigned long long c[QC_WORDS];
    HIP_TRY(hipMemcpy(c, C.d_ctr, sizeof c, hipMemcpyDeviceToHost));
    stats->rays = S.n;
    stats->hits = (long long)c[QC_HITS];
    stats->stack_spills = (long long)c[QC_SPILLS];
    stats->watchdog = (long long)c[QC_WATCHDOG];
    if (c[CD_GUARD] != 0 || guard_tripped(sc)) return fail(RT_ERR_HIP, kGuardMsg);
  }
  return RT_OK;
}

}  // extern "C"
