// rt_reclip.hpp — the arithmetic of re-clipping a moved triangle to the region a spatial split of
// the upload cut its record to (rt_scene_update_vertices_ex with RT_UPDATE_RECLIP, include/rt_hip.h;
// DESIGN.md §25).  One function text for the device kernel (rt_update.inc), rt_reclip_box_host and
// stand-alone host programs, in the manner of rt_refit.hpp: fp64 + - * / and comparisons, so that
// with fp contraction off host and device give the same bits.
//
// A clip region is six numbers, lo xyz then hi xyz, -inf / +inf where the record was never cut.  The
// box of a record is bounds(triangle), intersected per finite plane with the bounds of the part of
// the triangle on the region's side of that plane (the builder's split_ref edge walk: vertices by
// exact comparison, crossing points p = a + t (b - a), t = (pos - a[k]) / (b[k] - a[k]), p[k] = pos),
// clamped to the region.  The plane-by-plane intersection contains triangle ∩ region, which is all
// that correctness needs, it is what the builder's nested split_ref calls compute, and it needs no
// polygon array (dynamic indexing would live in scratch).  Only the crossing points carry rounding
// error, a few 2^-53 max|vertex|; the leaf box is then grown by delta = 2^-20 max|vertex|.
#ifndef RT_RECLIP_HPP
#define RT_RECLIP_HPP

#include "rt_refit.hpp"

// One edge a -> b against plane x[K] = pos: grows [lo, hi] by a where a lies on the kept side
// (UPPER: x[K] <= pos, else x[K] >= pos) and by the crossing point where the edge crosses.
template <int K, bool UPPER>
RT_REFIT_HD inline void rt_reclip_edge(const double a[3], const double b[3], double pos, double lo[3], double hi[3]) {
  if (UPPER ? a[K] <= pos : a[K] >= pos) rt_refit_grow(lo, hi, a);
  if ((a[K] < pos && b[K] > pos) || (a[K] > pos && b[K] < pos)) {
    const double t = (pos - a[K]) / (b[K] - a[K]);
    double p[3];
    for (int k = 0; k < 3; ++k) p[k] = a[k] + t * (b[k] - a[k]);
    p[K] = pos;
    rt_refit_grow(lo, hi, p);
  }
}

// [lo, hi] ∩= bounds of the part of triangle (p0, p1, p2) on the kept side of plane x[K] = pos.
template <int K, bool UPPER>
RT_REFIT_HD inline void rt_reclip_plane(const double p0[3], const double p1[3], const double p2[3], double pos,
                                        double lo[3], double hi[3]) {
  double hlo[3] = {INFINITY, INFINITY, INFINITY}, hhi[3] = {-INFINITY, -INFINITY, -INFINITY};
  rt_reclip_edge<K, UPPER>(p0, p1, pos, hlo, hhi);
  rt_reclip_edge<K, UPPER>(p1, p2, pos, hlo, hhi);
  rt_reclip_edge<K, UPPER>(p2, p0, pos, hlo, hhi);
  for (int k = 0; k < 3; ++k) {
    lo[k] = hlo[k] > lo[k] ? hlo[k] : lo[k];
    hi[k] = hhi[k] < hi[k] ? hhi[k] : hi[k];
  }
}

template <int K>
RT_REFIT_HD inline void rt_reclip_axis(const double p0[3], const double p1[3], const double p2[3], const double clip[6],
                                       double lo[3], double hi[3]) {
  if (clip[K] > -INFINITY) rt_reclip_plane<K, false>(p0, p1, p2, clip[K], lo, hi);
  if (clip[3 + K] < INFINITY) rt_reclip_plane<K, true>(p0, p1, p2, clip[3 + K], lo, hi);
}

// The fp64 box of triangle (p0, p1, p2) in region clip.  false: empty (an axis came out inverted),
// [lo, hi] is then of no use.
RT_REFIT_HD inline bool rt_reclip_box(const double p0[3], const double p1[3], const double p2[3], const double clip[6],
                                      double lo[3], double hi[3]) {
  for (int k = 0; k < 3; ++k) {
    lo[k] = INFINITY;
    hi[k] = -INFINITY;
  }
  rt_refit_grow(lo, hi, p0);
  rt_refit_grow(lo, hi, p1);
  rt_refit_grow(lo, hi, p2);
  rt_reclip_axis<0>(p0, p1, p2, clip, lo, hi);
  rt_reclip_axis<1>(p0, p1, p2, clip, lo, hi);
  rt_reclip_axis<2>(p0, p1, p2, clip, lo, hi);
  bool some = true;
  for (int k = 0; k < 3; ++k) {
    lo[k] = clip[k] > lo[k] ? clip[k] : lo[k];
    hi[k] = clip[3 + k] < hi[k] ? clip[3 + k] : hi[k];
    some = some && lo[k] <= hi[k];
  }
  return some;
}

#endif  // RT_RECLIP_HPP
