// rt_order.inc — sorting caller-supplied rays into coherent waves (rt_ray_order, rt_permute_rows,
// include/rt_hip.h; DESIGN.md §18).  Part of rt_render.hip's translation unit, included after
// rt_query.inc: it uses the raw-buffer helpers and the host-side error plumbing of that file.
//
// rt_ray_order = one key kernel, then four passes of a stable LSD radix sort (8-bit digits, all 32
// key bits) over (key, ray index) pairs.  A pass is three launches on the caller's stream:
//   count    a bounded grid, each block owning a contiguous run of whole tiles of kRoTile keys,
//            writes its digit histogram into the [digit][block] table;
//   scan     one block turns the table, row-major, into its exclusive prefix;
//   scatter  the same grid ranks each tile's keys stably -- ballot match-ranking per wave, wave
//            offsets in LDS, waves in order -- and stores them at table[digit][block] + rank.
// No atomic decides where an element goes: the order is numpy's stable argsort of the keys.
// Every loop is bounded by n; all scratch is the caller's workspace.
#include "rt_order_key.hpp"

static_assert(RT_ORDER_KEY_DEGENERATE == RT_ORDER_KEY_DEGENERATE_, "rt_order_key.hpp and rt_hip.h disagree");

namespace {

constexpr int kRoItems = 4;                           // keys per thread and tile
constexpr int kRoTile = kBlock * kRoItems;            // = RT_ORDER_TILE
constexpr int kRoGroups = kRoItems * (kBlock / 64);   // 64-key groups (a wave's share of one item) in a tile
constexpr int kRoMaxBlocks = 1024;                    // grid cap: the count table has this many columns
constexpr int kRoScanBlock = 1024;                    // threads of the scan kernel
constexpr size_t kRoAlign = 256;
static_assert(kRoTile == RT_ORDER_TILE, "RT_ORDER_TILE is the sort's tile");

__host__ __device__ inline size_t order_align(size_t b) { return (b + kRoAlign - 1) / kRoAlign * kRoAlign; }

// the workspace: keys A | keys B | indices B | table[256][kRoMaxBlocks]
struct OrderWs {
  uint32_t *keys_a, *keys_b, *idx_b, *table;
};
inline OrderWs order_ws(void* ws, long long n) {
  char* p = static_cast<char*>(ws);
  const size_t col = order_align((size_t)n * sizeof(uint32_t));
  OrderWs W;
  W.keys_a = reinterpret_cast<uint32_t*>(p);
  W.keys_b = reinterpret_cast<uint32_t*>(p + col);
  W.idx_b = reinterpret_cast<uint32_t*>(p + 2 * col);
  W.table = reinterpret_cast<uint32_t*>(p + 3 * col);
  return W;
}
inline size_t order_ws_bytes(long long n) {
  if (n <= 0) return 0;
  return 3 * order_align((size_t)n * sizeof(uint32_t)) + 256 * (size_t)kRoMaxBlocks * sizeof(uint32_t);
}

struct OrderBox {
  double lo[3], hi[3];
};

// keys[i] = key of rays[i], idx[i] = i: one ray per lane, a bounded grid striding over blocks of rays
__global__ void __launch_bounds__(kBlock) order_key_kernel(const rt_ray* rays, long long n, OrderBox B, int origin_bits,
                                                           uint32_t* keys, uint32_t* idx) {
  for (long long base = (long long)blockIdx.x * kBlock; base < n; base += (long long)gridDim.x * kBlock) {
    const long long left = n - base;
    const int nb = left < (long long)kBlock ? (int)left : kBlock;
    // the block's rays as a raw buffer: the hardware drops the loads of the lanes past the last ray
    const __amdgpu_buffer_rsrc_t rr =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<rt_ray*>(rays + base), 0, nb * (int)sizeof(rt_ray), kBufWord3);
    const uint32_t vo = threadIdx.x * (uint32_t)sizeof(rt_ray);
    // the 64-B ray: four 16-B loads issued together (the last one: tmax)
    const D2 q0 = buf_ld2(rr, vo, 0), q1 = buf_ld2(rr, vo + 16u, 0), q2 = buf_ld2(rr, vo + 32u, 0),
             q3 = buf_ld2(rr, vo + 48u, 0);
    if ((int)threadIdx.x < nb) {
      const double o[3] = {q0.a, q0.b, q1.a}, d[3] = {q1.b, q2.a, q2.b};
      const long long i = base + threadIdx.x;
      keys[i] = rt_order_key(B.lo, B.hi, o, d, q3.a, origin_bits);
      idx[i] = (uint32_t)i;
    }
  }
}

// table[d * nblocks + b] = keys of block b's tiles whose digit is d
__global__ void __launch_bounds__(kBlock) order_count_kernel(const uint32_t* keys, long long n, int shift,
                                                             int tiles_per_block, uint32_t* table) {
  __shared__ uint32_t hist[256];
  hist[threadIdx.x] = 0u;
  __syncthreads();
  const long long t0 = (long long)blockIdx.x * tiles_per_block;
  for (int t = 0; t < tiles_per_block; ++t) {
    const long long tb = (t0 + t) * kRoTile;
    if (tb >= n) break;
#pragma unroll
    for (int r = 0; r < kRoItems; ++r) {
      const long long i = tb + r * kBlock + threadIdx.x;
      if (i < n) atomicAdd(&hist[(keys[i] >> shift) & 255u], 1u);   // a count: any order gives the same sum
    }
  }
  __syncthreads();
  table[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = hist[threadIdx.x];
}

__device__ __forceinline__ uint32_t order_wave_incl_scan(uint32_t x) {
  uint32_t incl = x;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t v = __shfl_up(incl, o);
    if ((int)(threadIdx.x & 63) >= o) incl += v;
  }
  return incl;
}

// One block: table[256][nblocks], taken as one row-major array, becomes its exclusive prefix, so
// that table[d][b] = the keys with a smaller digit + the keys of digit d in the blocks before b.
// Each wave owns the rows of 256 / 16 digits, a contiguous segment: it sums the segment, the wave
// totals are scanned through LDS, then it scans the segment 256 entries (16 B per lane) at a time.
__global__ void __launch_bounds__(kRoScanBlock) order_scan_kernel(uint32_t* table, int nblocks) {
  constexpr int kWaves = kRoScanBlock / 64;
  __shared__ uint32_t wtot[kWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int seg = (256 / kWaves) * nblocks;   // a multiple of 16: a lane's four entries are all inside or all outside
  uint32_t* const mine = table + (size_t)wave * seg + lane * 4;
  uint32_t sum = 0u;
#pragma unroll 4
  for (int i = lane * 4; i < seg; i += 256) {
    const u32x4_t v = *reinterpret_cast<const u32x4_t*>(mine + (i - lane * 4));
    sum += (v.x + v.y) + (v.z + v.w);
  }
  const uint32_t tot = __shfl(order_wave_incl_scan(sum), 63);
  if (lane == 0) wtot[wave] = tot;
  __syncthreads();
  uint32_t carry = 0u;
  for (int w = 0; w < wave; ++w) carry += wtot[w];
  for (int c0 = 0; c0 < seg; c0 += 256) {   // wave-uniform trip count: the shuffles see all 64 lanes
    const bool in = c0 + lane * 4 < seg;
    u32x4_t v = {0u, 0u, 0u, 0u};
    if (in) v = *reinterpret_cast<const u32x4_t*>(mine + c0);
    const uint32_t s4 = (v.x + v.y) + (v.z + v.w);
    const uint32_t incl = order_wave_incl_scan(s4);
    const uint32_t e0 = carry + incl - s4;
    const u32x4_t out = {e0, e0 + v.x, e0 + v.x + v.y, e0 + v.x + v.y + v.z};
    if (in) *reinterpret_cast<u32x4_t*>(mine + c0) = out;
    carry += __shfl(incl, 63);
  }
}

// Block b moves the keys of its tiles, in order, to table[d][b] (scanned) + (their rank among the
// block's keys of digit d).  Thread d carries digit d's next free position across the tiles.
__global__ void __launch_bounds__(kBlock) order_scatter_kernel(const uint32_t* keys_in, const uint32_t* idx_in,
                                                               uint32_t* keys_out, uint32_t* idx_out, long long n,
                                                               int shift, int tiles_per_block, const uint32_t* table) {
  __shared__ uint16_t cnt[kRoGroups][256];   // keys of a digit per 64-key group, then their exclusive prefix
  __shared__ uint32_t gbase[256];            // the tile's first position per digit
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long lt = (1ull << lane) - 1ull;
  uint32_t next = table[(size_t)threadIdx.x * gridDim.x + blockIdx.x];
  const long long t0 = (long long)blockIdx.x * tiles_per_block;
  for (int t = 0; t < tiles_per_block; ++t) {
    const long long tb = (t0 + t) * kRoTile;
    if (tb >= n) break;   // block-uniform
    {
      uint32_t* z = reinterpret_cast<uint32_t*>(&cnt[0][0]);
#pragma unroll
      for (int k = 0; k < kRoGroups * 256 / 2 / kBlock; ++k) z[k * kBlock + threadIdx.x] = 0u;
    }
    uint32_t key[kRoItems], val[kRoItems], rank[kRoItems];
    bool valid[kRoItems];
#pragma unroll
    for (int r = 0; r < kRoItems; ++r) {
      const long long i = tb + r * kBlock + threadIdx.x;
      valid[r] = i < n;
      key[r] = valid[r] ? keys_in[i] : 0u;
      val[r] = valid[r] ? idx_in[i] : 0u;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < kRoItems; ++r) {
      const uint32_t dg = (key[r] >> shift) & 255u;
      // the lanes of this wave whose key has the same digit
      unsigned long long m = wballot(valid[r]);
#pragma unroll
      for (int b = 0; b < 8; ++b) {
        const unsigned long long bal = wballot((dg >> b) & 1u);
        m &= ((dg >> b) & 1u) ? bal : ~bal;
      }
      rank[r] = (uint32_t)__popcll(m & lt);
      if (valid[r] && rank[r] == 0u) cnt[r * (kBlock / 64) + wave][dg] = (uint16_t)__popcll(m);
    }
    __syncthreads();
    {   // thread d: digit d's groups in order
      uint32_t run = 0u;
#pragma unroll
      for (int g = 0; g < kRoGroups; ++g) {
        const uint32_t c = cnt[g][threadIdx.x];
        cnt[g][threadIdx.x] = (uint16_t)run;
        run += c;
      }
      gbase[threadIdx.x] = next;
      next += run;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < kRoItems; ++r) {
      const uint32_t dg = (key[r] >> shift) & 255u;
      const uint32_t pos = gbase[dg] + cnt[r * (kBlock / 64) + wave][dg] + rank[r];
      if (valid[r] && (long long)pos < n) {
        keys_out[pos] = key[r];
        idx_out[pos] = val[r];
      }
    }
    __syncthreads();   // cnt and gbase are rewritten by the next tile
  }
}

// Rows of `ppr` pieces of type T; a block takes 256 / ppr rows at a time, consecutive lanes on
// consecutive pieces of a row.  INVERSE: dst row perm[j] = src row j, else dst row j = src row perm[j].
// The sequential side streams: nontemporal.
template <typename T, bool INVERSE>
__global__ void __launch_bounds__(kBlock) permute_rows_kernel(const T* src, T* dst, const uint32_t* perm, long long n,
                                                              int ppr) {
  const int rpb = kBlock / ppr;
  const int r = (int)threadIdx.x / ppr, c = (int)threadIdx.x - r * ppr;
  if (r >= rpb) return;
  for (long long j = (long long)blockIdx.x * rpb + r; j < n; j += (long long)gridDim.x * rpb) {
    const unsigned long long e = perm[j];
    if (e >= (unsigned long long)n) continue;   // skipped entry: nothing read, nothing written
    if (INVERSE) {
      dst[e * ppr + c] = __builtin_nontemporal_load(&src[j * ppr + c]);
    } else {
      __builtin_nontemporal_store(src[e * ppr + c], &dst[j * ppr + c]);
    }
  }
}

template <typename T>
void launch_permute(const void* src, void* dst, const uint32_t* perm, long long n, int ppr, bool inverse, hipStream_t st) {
  const int rpb = kBlock / ppr;
  const unsigned blocks = (unsigned)std::max<long long>(1, std::min<long long>((n + rpb - 1) / rpb, 1 << 20));
  if (inverse)
    hipLaunchKernelGGL((permute_rows_kernel<T, true>), dim3(blocks), dim3(kBlock), 0, st, static_cast<const T*>(src),
                       static_cast<T*>(dst), perm, n, ppr);
  else
    hipLaunchKernelGGL((permute_rows_kernel<T, false>), dim3(blocks), dim3(kBlock), 0, st, static_cast<const T*>(src),
                       static_cast<T*>(dst), perm, n, ppr);
}

}  // namespace

extern "C" {

int rt_scene_bounds(const rt_scene* sc, double lo[3], double hi[3]) {
  if (!sc || !lo || !hi) return fail(RT_ERR_INVALID, "rt_scene_bounds: null argument");
  for (int k = 0; k < 3; ++k) {
    lo[k] = sc->n_gnodes > 0 ? sc->root_lo[k] : 0.0;
    hi[k] = sc->n_gnodes > 0 ? sc->root_hi[k] : 0.0;
  }
  return RT_OK;
}

size_t rt_ray_order_workspace_bytes(long long n) { return order_ws_bytes(n); }

int rt_ray_keys_host(const double lo[3], const double hi[3], const rt_ray* rays, long long n, int origin_bits,
                     unsigned int* keys) {
  if (!lo || !hi) return fail(RT_ERR_INVALID, "rt_ray_keys_host: null box");
  if (n < 0) return fail(RT_ERR_INVALID, "rt_ray_keys_host: negative ray count");
  if (n > 0 && (!rays || !keys)) return fail(RT_ERR_INVALID, "rt_ray_keys_host: null ray or key buffer");
  if (origin_bits < -1 || origin_bits > 10) return fail(RT_ERR_INVALID, "rt_ray_keys_host: origin_bits outside [-1, 10]");
  for (long long i = 0; i < n; ++i) keys[i] = rt_order_key(lo, hi, rays[i].o, rays[i].d, rays[i].tmax, origin_bits);
  return RT_OK;
}

int rt_debug_set_order_grid(rt_scene* sc, int max_blocks) {
  if (!sc || max_blocks < 0) return fail(RT_ERR_INVALID, "rt_debug_set_order_grid: bad argument");
  sc->order_grid = max_blocks;
  return RT_OK;
}

int rt_ray_order(rt_scene* sc, const rt_ray* d_rays, long long n, int origin_bits, unsigned int* d_perm,
                 unsigned int* d_keys, void* d_workspace, void* stream) {
  if (!sc) return fail(RT_ERR_INVALID, "rt_ray_order: null scene");
  if (n < 0) return fail(RT_ERR_INVALID, "rt_ray_order: negative ray count");
  if (n > RT_ORDER_MAX_RAYS) return fail(RT_ERR_INVALID, "rt_ray_order: more than RT_ORDER_MAX_RAYS rays");
  if (n > 0 && (!d_rays || !d_perm || !d_workspace))
    return fail(RT_ERR_INVALID, "rt_ray_order: null ray, permutation or workspace buffer");
  if (origin_bits < -1 || origin_bits > 10) return fail(RT_ERR_INVALID, "rt_ray_order: origin_bits outside [-1, 10]");
  if (n > 0 && reinterpret_cast<uintptr_t>(d_workspace) % kRoAlign)
    return fail(RT_ERR_INVALID, "rt_ray_order: workspace not 256-byte aligned");
  if (guard_tripped(sc)) return fail(RT_ERR_HIP, kGuardMsg);
  if (n == 0) return RT_OK;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  HIP_TRY(hipSetDevice(sc->device));
  const OrderWs W = order_ws(d_workspace, n);
  OrderBox B;
  for (int k = 0; k < 3; ++k) {
    B.lo[k] = sc->n_gnodes > 0 ? sc->root_lo[k] : 0.0;
    B.hi[k] = sc->n_gnodes > 0 ? sc->root_hi[k] : 0.0;
  }
  // the grid of the sort: at most `cap` blocks, each a contiguous run of whole tiles
  const long long cap = std::max(1, std::min(kRoMaxBlocks, sc->order_grid > 0 ? sc->order_grid : 2 * std::max(1, sc->n_cu)));
  const long long ntiles = (n + kRoTile - 1) / kRoTile;
  const long long tpb = (ntiles + cap - 1) / cap;
  const int nblocks = (int)((ntiles + tpb - 1) / tpb);
  {
    const long long want = (n + kBlock - 1) / kBlock;
    const unsigned blocks = (unsigned)std::min<long long>(want, 8LL * std::max(1, sc->n_cu));
    uint32_t* k0 = d_keys ? d_keys : W.keys_a;   // the caller's copy doubles as the first pass's input
    hipLaunchKernelGGL(order_key_kernel, dim3(blocks), dim3(kBlock), 0, st, d_rays, n, B, origin_bits, k0, d_perm);
  }
  // four passes; (keys, indices) ping-pong (k0 | A, d_perm) -> (B, idx B) -> (A, d_perm) -> ...: the
  // fourth lands in d_perm
  const uint32_t* kin = d_keys ? d_keys : W.keys_a;
  const uint32_t* vin = d_perm;
  for (int pass = 0; pass < 4; ++pass) {
    uint32_t* kout = (pass & 1) ? W.keys_a : W.keys_b;
    uint32_t* vout = (pass & 1) ? d_perm : W.idx_b;
    const int shift = 8 * pass;
    hipLaunchKernelGGL(order_count_kernel, dim3(nblocks), dim3(kBlock), 0, st, kin, n, shift, (int)tpb, W.table);
    hipLaunchKernelGGL(order_scan_kernel, dim3(1), dim3(kRoScanBlock), 0, st, W.table, nblocks);
    hipLaunchKernelGGL(order_scatter_kernel, dim3(nblocks), dim3(kBlock), 0, st, kin, vin, kout, vout, n, shift, (int)tpb,
                       W.table);
    kin = kout;
    vin = vout;
  }
  HIP_TRY(hipGetLastError());
  return RT_OK;
}

int rt_permute_rows(const void* d_src, void* d_dst, const unsigned int* d_perm, long long n, int row_bytes, int inverse,
                    int device, void* stream) {
  if (n < 0) return fail(RT_ERR_INVALID, "rt_permute_rows: negative row count");
  if (n > (1LL << 32)) return fail(RT_ERR_INVALID, "rt_permute_rows: more rows than a 32-bit index addresses");
  if (row_bytes < 1 || row_bytes > 256) return fail(RT_ERR_INVALID, "rt_permute_rows: row_bytes outside [1, 256]");
  if (device < 0) return fail(RT_ERR_INVALID, "rt_permute_rows: negative device");
  if (n > 0 && (!d_src || !d_dst || !d_perm)) return fail(RT_ERR_INVALID, "rt_permute_rows: null buffer");
  const int unit = row_bytes % 16 == 0 ? 16 : row_bytes % 4 == 0 ? 4 : 1;
  const uintptr_t align = row_bytes % 16 == 0 ? 16 : row_bytes % 8 == 0 ? 8 : row_bytes % 4 == 0 ? 4 : row_bytes % 2 == 0 ? 2 : 1;
  const uintptr_t s = reinterpret_cast<uintptr_t>(d_src), d = reinterpret_cast<uintptr_t>(d_dst);
  if (n > 0 && (s % align || d % align))
    return fail(RT_ERR_INVALID, "rt_permute_rows: buffer not aligned for its row size");
  const uintptr_t len = (uintptr_t)n * (uintptr_t)row_bytes;
  if (n > 0 && s < d + len && d < s + len) return fail(RT_ERR_INVALID, "rt_permute_rows: source and destination overlap");
  if (n == 0) return RT_OK;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  HIP_TRY(hipSetDevice(device));
  if (unit == 16) launch_permute<u32x4_t>(d_src, d_dst, d_perm, n, row_bytes / 16, inverse != 0, st);
  else if (unit == 4) launch_permute<uint32_t>(d_src, d_dst, d_perm, n, row_bytes / 4, inverse != 0, st);
  else launch_permute<unsigned char>(d_src, d_dst, d_perm, n, row_bytes, inverse != 0, st);
  HIP_TRY(hipGetLastError());
  return RT_OK;
}

}  // extern "C"
