// rt_normals.hpp — the arithmetic of a mesh's normals (rt_scene_update_positions, rt_normals_host,
// include/rt_hip.h): the face normal and the three corner weights of a triangle, and
// the angle-weighted gather of a vertex's normal.  It restates HostMesh::compute_normals
// (host_scene.cpp, mymesh.cpp:103-163) operation for operation, and compute_normals calls it.
// One function text for the device kernels (rt_normals.inc), the host scene and stand-alone host
// programs: plain C++ in fp64 with + - * /, sqrt, fabs and comparisons only, so that with fp
// contraction off host and device give the same bits.
#ifndef RT_NORMALS_HPP
#define RT_NORMALS_HPP

#include <cmath>

#if defined(__HIP__) || defined(__CUDACC__)
#define RT_NORMALS_HD __host__ __device__
#else
#define RT_NORMALS_HD
#endif

// (a0 b0 + a1 b1) + a2 b2: the host's dot3, left to right
RT_NORMALS_HD inline double rt_normals_dot(const double a[3], const double b[3]) {
  return a[0] * b[0] + a[1] * b[1] + a[2] * b[2];
}

// The host's normalize3: v / |v|, v itself where |v| is not > 0 (a zero or a NaN length).
RT_NORMALS_HD inline void rt_normals_normalize(double v[3]) {
  const double len = sqrt(rt_normals_dot(v, v));
  if (len > 0.0) {
    v[0] = v[0] / len;
    v[1] = v[1] / len;
    v[2] = v[2] / len;
  }
}

// Triangle (p0, p1, p2): n = normalize(cross(p1 - p0, p2 - p0)), the cross product itself where its
// length is not > 0, and the weights of its three corners, w0 = |a||c| + a.(-c), w1 = |b||a| + b.(-a),
// w2 = |c||b| + c.(-b) with a = p1 - p0, b = p2 - p1, c = p0 - p2: |u||v| (1 + cos) of the corner's angle (near zero at a corner of almost pi).
RT_NORMALS_HD inline void rt_normals_face(const double p0[3], const double p1[3], const double p2[3], double n[3],
                                          double w[3]) {
  const double e1[3] = {p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]};
  const double e2[3] = {p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2]};
  n[0] = e1[1] * e2[2] - e1[2] * e2[1];
  n[1] = e1[2] * e2[0] - e1[0] * e2[2];
  n[2] = e1[0] * e2[1] - e1[1] * e2[0];
  rt_normals_normalize(n);
  const double a[3] = {p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]};
  const double b[3] = {p2[0] - p1[0], p2[1] - p1[1], p2[2] - p1[2]};
  const double c[3] = {p0[0] - p2[0], p0[1] - p2[1], p0[2] - p2[2]};
  const double na[3] = {-a[0], -a[1], -a[2]}, nb[3] = {-b[0], -b[1], -b[2]}, nc[3] = {-c[0], -c[1], -c[2]};
  const double la = sqrt(rt_normals_dot(a, a)), lb = sqrt(rt_normals_dot(b, b)), lc = sqrt(rt_normals_dot(c, c));
  w[0] = la * lc + rt_normals_dot(a, nc);
  w[1] = lb * la + rt_normals_dot(b, na);
  w[2] = lc * lb + rt_normals_dot(c, nb);
}

// One corner of a vertex's gather: sum += n / w, skipped (not added as zero) where |w| <= 1e-12 or w
// is a NaN.  The sum starts from +0.0 and ends with rt_normals_normalize.
RT_NORMALS_HD inline void rt_normals_add(double sum[3], const double n[3], double w) {
  if (fabs(w) > 1e-12) {
    sum[0] += n[0] / w;
    sum[1] += n[1] / w;
    sum[2] += n[2] / w;
  }
}

#endif  // RT_NORMALS_HPP
