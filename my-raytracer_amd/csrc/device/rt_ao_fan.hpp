// rt_ao_fan.hpp — the occlusion fan of a surface point (rt_trace_ao, include/rt_hip.h).
// One function text for the device kernel, rt_ao_rays_host and stand-alone host programs: plain
// C++ in fp64 with + - * /, sqrt, fabs, comparisons and selects only, so that with fp contraction
// off every compiler -- and numpy -- gives the same bits.
#ifndef RT_AO_FAN_HPP
#define RT_AO_FAN_HPP

#include <cfloat>
#include <cmath>
#include <cstdint>

#if defined(__HIP__) || defined(__CUDACC__)
#define RT_AO_HD __host__ __device__
#else
#define RT_AO_HD
#endif

#define RT_AO_MAX_SAMPLES_ 1024   // = RT_AO_MAX_SAMPLES (rt_hip.h)
#define RT_AO_MAX_SETS_ 65536     // = RT_AO_MAX_SETS (rt_hip.h)

// The 32-bit mixer that picks a point's direction set: xor-shift and multiply rounds, a bijection
// of the 32-bit integers.
RT_AO_HD inline uint32_t rt_ao_hash(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7feb352du;
  x ^= x >> 15;
  x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}

// the direction set of point i
RT_AO_HD inline uint32_t rt_ao_set(long long i, uint32_t seed, int n_sets) {
  return rt_ao_hash((uint32_t)i ^ seed) % (uint32_t)n_sets;
}

RT_AO_HD inline bool rt_ao_finite(double x) { return fabs(x) <= DBL_MAX; }   // false for NaN / inf

// the queries' rule for a ray they never traverse, applied to the point record (o, nrm, tmax);
// sqrt(x) > 0 iff x > 0, so the dot product is compared itself
RT_AO_HD inline bool rt_ao_point_valid(const double o[3], const double nrm[3], double tmax) {
  const double dd = nrm[0] * nrm[0] + nrm[1] * nrm[1] + nrm[2] * nrm[2];
  return rt_ao_finite(o[0]) && rt_ao_finite(o[1]) && rt_ao_finite(o[2]) && rt_ao_finite(nrm[0]) &&
         rt_ao_finite(nrm[1]) && rt_ao_finite(nrm[2]) && dd > 0.0 && tmax > 1e-5;   // NaN tmax: false
}

// The fan ray of point (p, nrm, tmax) along the local direction l (z along the normal):
//   N = nrm / |nrm|, (T, B) = the branch-free tangent frame of Duff et al. 2017,
//   origin = p + bias * N, w = (l.x * T + l.y * B) + l.z * N, each per component.
// A degenerate point gives origin = p, w = 0: a degenerate ray.  Nothing is clamped or rejected per
// direction: the traversal treats a zero or non-finite w as the queries treat such a d.
RT_AO_HD inline void rt_ao_fan_ray(const double p[3], const double nrm[3], double tmax, const double l[3], double bias,
                                   double origin[3], double w[3]) {
  if (!rt_ao_point_valid(p, nrm, tmax)) {
    for (int c = 0; c < 3; ++c) {
      origin[c] = p[c];
      w[c] = 0.0;
    }
    return;
  }
  const double len = sqrt(nrm[0] * nrm[0] + nrm[1] * nrm[1] + nrm[2] * nrm[2]);
  const double N[3] = {nrm[0] / len, nrm[1] / len, nrm[2] / len};
  const double sg = N[2] >= 0.0 ? 1.0 : -1.0;
  const double a = -1.0 / (sg + N[2]);
  const double b = N[0] * N[1] * a;
  const double T[3] = {1.0 + sg * N[0] * N[0] * a, sg * b, -sg * N[0]};
  const double B[3] = {b, sg + N[1] * N[1] * a, -N[1]};
  for (int c = 0; c < 3; ++c) {
    origin[c] = p[c] + bias * N[c];
    w[c] = (l[0] * T[c] + l[1] * B[c]) + l[2] * N[c];
  }
}

#endif  // RT_AO_FAN_HPP
