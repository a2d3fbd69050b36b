// rt_camera.inc — a camera's closest hits and surface points made on the device (rt_trace_camera,
// rt_camera_rays_host, rt_surface_points_host, include/rt_hip.h; DESIGN.md §22).  Part of
// rt_render.hip's translation unit, included after rt_ao.inc: the kernel uses rt_query.inc's stack
// ring, top treelet, counters, query contexts and launch steps and the render path's device helpers
// unchanged.
//
// One kernel: a wave takes one kTileW x kTileH (8 x 8) tile of the shard's packed rows (the render
// kernel's work tile), a block four consecutive tiles, a bounded grid strides over the tiles.  A lane builds its pixel's
// primary ray in registers (rt_camera_point.hpp), walks the hierarchy with the closest-hit traversal
// of query_kernel<false> -- the same text, rt_walk_body.inc, included here too, so the hit is
// rt_trace_closest's of the ray rt_camera_rays_host writes out -- and stores what the caller asked
// for: the 64-B rt_hit, the 64-B surface-point record, or both, in the frame's row order or in tile
// order.  Nothing is read per pixel.
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
  query_stage_treelet(q_top, P);
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
    constexpr bool ANYHIT = false;   // the walk of query_kernel<false>
#include "rt_walk_body.inc"

    // the rt_hit of the walk's closest hit, as query_kernel<false> composes it
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
  query_flush_counters(P, lane, n_hits, n_spills, n_trips);
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

int camera_blocks_per_cu() {
  static const int blocks = query_blocks_per_cu(reinterpret_cast<const void*>(&camera_kernel));
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
  QueryCtx* C;
  const int arc = query_acquire(sc, st, &C);
  if (arc != RT_OK) return arc;
  CamParams P;
  std::memset(&P, 0, sizeof P);
  query_scene_params(P, sc, *C);
  P.tnorm = sc->d_tnorm; P.mats = sc->d_mats;
  P.hits = out->d_hits; P.points = out->d_points;
  for (int k = 0; k < 3; ++k) {
    P.eye[k] = p->camera.eye[k]; P.ll[k] = p->camera.lower_left[k];
    P.xd[k] = p->camera.x_dir[k]; P.yd[k] = p->camera.y_dir[k];
  }
  P.point_tmax = out->point_tmax;
  P.W = S.W; P.rows = S.rows;
  P.tiles_x = (uint32_t)((S.W + kTileW - 1) / kTileW);
  P.n_tiles = P.tiles_x * (uint32_t)((S.rows + kTileH - 1) / kTileH);   // at most 2^26
  P.row_begin = S.row_begin; P.stripe_h = S.stripe_h; P.stripe_count = S.stripe_count; P.stripe_index = S.stripe_index;
  P.tile_major = out->order == RT_CAMERA_TILE_MAJOR ? 1 : 0;
  const unsigned blocks =
      query_grid(sc, ((long long)P.n_tiles + kCamTilesPerBlock - 1) / kCamTilesPerBlock, camera_blocks_per_cu());
  hipLaunchKernelGGL(camera_kernel, dim3(blocks), dim3(kBlock), 0, st, P);
  return query_finish(sc, *C, st, S.n, stats);
}

}  // extern "C"
