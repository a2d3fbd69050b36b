// rt_refit.hpp — the arithmetic of moving a device scene's vertices (rt_scene_update_vertices,
// include/rt_hip.h): the triangle record of three vertices, the outward fp32
// rounding of a box bound, the box of a leaf slot and the union of a child node's four slots.
// One function text for the device kernels (rt_update.inc), the host builder (device_image.cpp) and
// stand-alone host programs: plain C++ with + - and comparisons in fp64, a cast and nextafterf's
// one-ulp step in fp32, so that with fp contraction off host and device give the same bits.
#ifndef RT_REFIT_HPP
#define RT_REFIT_HPP

#include <cmath>
#include <cstdint>
#include <cstring>

#if defined(__HIP__) || defined(__CUDACC__)
#define RT_REFIT_HD __host__ __device__
#else
#define RT_REFIT_HD
#endif

// The operands of the triangle test from the three vertices, as build_image writes them:
// e1 = p0 - p2, e2 = p1 - p2 and p2 itself.
RT_REFIT_HD inline void rt_refit_record(const double p0[3], const double p1[3], const double p2[3], double e1[3],
                                        double e2[3], double q2[3]) {
  for (int k = 0; k < 3; ++k) {
    e1[k] = p0[k] - p2[k];
    e2[k] = p1[k] - p2[k];
    q2[k] = p2[k];
  }
}

// The neighbour of a finite or infinite float towards -inf / +inf: nextafterf(f, -+INFINITY), written
// on the bit pattern so that host and device run the same text (+-0 steps to the smallest denormal of
// the other side, the infinity one steps towards stays, a NaN stays).
RT_REFIT_HD inline float rt_refit_step(float f, bool up) {
  if (f != f) return f;
  uint32_t u;
  memcpy(&u, &f, sizeof u);
  if ((u & 0x7fffffffu) == 0u) u = up ? 0x00000001u : 0x80000001u;
  else if (((u >> 31) == 0u) == up) u += (u & 0x7fffffffu) == 0x7f800000u ? 0u : 1u;   // away from zero
  else u -= 1u;                                                                        // towards zero
  memcpy(&f, &u, sizeof f);
  return f;
}

// Outward rounding of a box bound to fp32: cast, compare, one step (round_down_host / round_up_host
// of the upload).
RT_REFIT_HD inline float rt_refit_round_down(double x) {
  float f = (float)x;
  if ((double)f > x) f = rt_refit_step(f, false);
  return f;
}
RT_REFIT_HD inline float rt_refit_round_up(double x) {
  float f = (float)x;
  if ((double)f < x) f = rt_refit_step(f, true);
  return f;
}

// min / max as comparisons a NaN never wins: a NaN coordinate enters no box.
RT_REFIT_HD inline void rt_refit_grow(double lo[3], double hi[3], const double p[3]) {
  for (int k = 0; k < 3; ++k) {
    lo[k] = p[k] < lo[k] ? p[k] : lo[k];
    hi[k] = p[k] > hi[k] ? p[k] : hi[k];
  }
}

// The fp32 box of a leaf slot whose triangles' vertices span [lo, hi] in fp64, grown by delta.
RT_REFIT_HD inline void rt_refit_leaf_box(const double lo[3], const double hi[3], double delta, float flo[3],
                                          float fhi[3]) {
  for (int k = 0; k < 3; ++k) {
    flo[k] = rt_refit_round_down(lo[k] - delta);
    fhi[k] = rt_refit_round_up(hi[k] + delta);
  }
}

// One axis of the union of a child node's four slots (empty slots hold [+inf, -inf] and never win).
// Outward rounding is monotone, so the fp32 union equals the rounded fp64 union bit for bit.
RT_REFIT_HD inline void rt_refit_union4(const float lo4[4], const float hi4[4], float* lo, float* hi) {
  float l = lo4[0], h = hi4[0];
  for (int s = 1; s < 4; ++s) {
    l = lo4[s] < l ? lo4[s] : l;
    h = hi4[s] > h ? hi4[s] : h;
  }
  *lo = l;
  *hi = h;
}

#endif  // RT_REFIT_HPP
