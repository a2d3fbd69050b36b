// rt_order_key.hpp — the coherence key of a ray (rt_ray_order, include/rt_hip.h).
// One function text for the device kernel, rt_ray_keys_host and stand-alone host programs: plain
// C++ in fp64 with + - * /, fabs, floor, comparisons and selects only, so that with fp contraction
// off every compiler -- and numpy -- gives the same bits.
#ifndef RT_ORDER_KEY_HPP
#define RT_ORDER_KEY_HPP

#include <cfloat>
#include <cmath>
#include <cstdint>

#if defined(__HIP__) || defined(__CUDACC__)
#define RT_ORDER_HD __host__ __device__
#else
#define RT_ORDER_HD
#endif

#define RT_ORDER_KEY_DEGENERATE_ 0x80000000u   // = RT_ORDER_KEY_DEGENERATE (rt_hip.h)

// direction bits per octahedral axis for `ob` origin bits per axis (ob in [0, 10])
RT_ORDER_HD inline int rt_order_dir_bits(int ob) {
  const int db = (31 - 3 * ob) / 2;
  return db < 15 ? db : 15;
}

// bit i of x -> bit 3i (x < 2^10)
RT_ORDER_HD inline uint32_t rt_order_spread3(uint32_t x) {
  x &= 0x3ffu;
  x = (x | (x << 16)) & 0x030000ffu;
  x = (x | (x << 8)) & 0x0300f00fu;
  x = (x | (x << 4)) & 0x030c30c3u;
  x = (x | (x << 2)) & 0x09249249u;
  return x;
}

// bit i of x -> bit 2i (x < 2^16)
RT_ORDER_HD inline uint32_t rt_order_spread2(uint32_t x) {
  x &= 0xffffu;
  x = (x | (x << 8)) & 0x00ff00ffu;
  x = (x | (x << 4)) & 0x0f0f0f0fu;
  x = (x | (x << 2)) & 0x33333333u;
  x = (x | (x << 1)) & 0x55555555u;
  return x;
}

RT_ORDER_HD inline bool rt_order_finite(double x) { return fabs(x) <= DBL_MAX; }   // false for NaN / inf

// floor(u * scale) held to [0, top] in double, before the conversion (a NaN gives 0)
RT_ORDER_HD inline uint32_t rt_order_cell(double u, double scale, double top) {
  double c = floor(u * scale);
  c = c >= 0.0 ? c : 0.0;
  c = c > top ? top : c;
  return (uint32_t)c;
}

// The key of ray (o, d, tmax) in the box [lo, hi]; origin_bits in [-1, 10], -1 = 5.
//   degenerate ray (the rays the queries never traverse) -> 0x80000000, every other key < 2^31
//   key = morton3(origin cell) << (2 db) | morton2(octahedral cell of d)
RT_ORDER_HD inline uint32_t rt_order_key(const double lo[3], const double hi[3], const double o[3], const double d[3],
                                         double tmax, int origin_bits) {
  const int ob = origin_bits < 0 ? 5 : origin_bits;
  const int db = rt_order_dir_bits(ob);
  // the queries' `act` predicate; sqrt(x) > 0 iff x > 0, so the dot product is compared itself
  const double dd = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
  const bool act = rt_order_finite(o[0]) && rt_order_finite(o[1]) && rt_order_finite(o[2]) && rt_order_finite(d[0]) &&
                   rt_order_finite(d[1]) && rt_order_finite(d[2]) && dd > 0.0 && tmax > 1e-5;   // NaN tmax: false
  if (!act) return RT_ORDER_KEY_DEGENERATE_;
  const double oscale = (double)(1u << ob), otop = oscale - 1.0;
  uint32_t mo = 0;
  for (int k = 0; k < 3; ++k) {
    const double e = hi[k] - lo[k];
    const uint32_t c = e > 0.0 ? rt_order_cell((o[k] - lo[k]) / e, oscale, otop) : 0u;
    mo |= rt_order_spread3(c) << k;
  }
  const double s = (fabs(d[0]) + fabs(d[1])) + fabs(d[2]);
  double px = d[0] / s, py = d[1] / s;
  if (d[2] < 0.0) {
    const double fx = (1.0 - fabs(py)) * (px >= 0.0 ? 1.0 : -1.0);
    const double fy = (1.0 - fabs(px)) * (py >= 0.0 ? 1.0 : -1.0);
    px = fx;
    py = fy;
  }
  const double dscale = (double)(1u << db), dtop = dscale - 1.0;
  const uint32_t qu = rt_order_cell(px * 0.5 + 0.5, dscale, dtop);
  const uint32_t qv = rt_order_cell(py * 0.5 + 0.5, dscale, dtop);
  const uint32_t md = rt_order_spread2(qu) | (rt_order_spread2(qv) << 1);
  return (mo << (2 * db)) | md;
}

#endif  // RT_ORDER_KEY_HPP
