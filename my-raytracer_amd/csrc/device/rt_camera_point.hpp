// rt_camera_point.hpp — a camera's primary ray and the surface point of a ray and its closest hit
// (rt_trace_camera, rt_camera_rays_host, rt_surface_points_host, include/rt_hip.h).
// One function text for the device kernel, the host functions and stand-alone host programs: plain
// C++ in fp64 with + - * /, sqrt, comparisons and selects only, so that with fp contraction off every
// compiler -- and numpy -- gives the same bits.
#ifndef RT_CAMERA_POINT_HPP
#define RT_CAMERA_POINT_HPP

#include <cmath>

#if defined(__HIP__) || defined(__CUDACC__)
#define RT_CAM_HD __host__ __device__
#else
#define RT_CAM_HD
#endif

// The primary ray of pixel (x, y): o = eye, d = ((lower_left + x * x_dir) + y * y_dir) - eye per
// component, left to right and unnormalised -- the render kernel's start_sample at one sample per
// pixel, and rtamd.camera_rays.
RT_CAM_HD inline void rt_camera_ray(const double eye[3], const double lower_left[3], const double x_dir[3],
                                    const double y_dir[3], int x, int y, double o[3], double d[3]) {
  const double X = (double)x, Y = (double)y;
  for (int c = 0; c < 3; ++c) {
    o[c] = eye[c];
    d[c] = ((lower_left[c] + X * x_dir[c]) + Y * y_dir[c]) - eye[c];
  }
}

// The surface point of ray (o, d) whose closest hit lies at distance t with normal nrm; the hit
// counts iff t < +inf.
//   hit:  rd = d / sqrt(dot(d, d)) (the renderer's normalize: d itself if that length is not > 0),
//         p = o + t * rd, n = nrm, negated if nrm.x * d.x + nrm.y * d.y + nrm.z * d.z > 0 (d
//         unnormalised): the normal faces the ray's origin
//   miss: p = o, n = (0, 0, 0): a degenerate point (rt_ao_fan.hpp)
RT_CAM_HD inline void rt_surface_point(const double o[3], const double d[3], double t, const double nrm[3],
                                       double p[3], double n[3]) {
  if (!(t < INFINITY)) {
    for (int c = 0; c < 3; ++c) {
      p[c] = o[c];
      n[c] = 0.0;
    }
    return;
  }
  const double len = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
  const bool unit = len > 0.0;
  const bool flip = nrm[0] * d[0] + nrm[1] * d[1] + nrm[2] * d[2] > 0.0;
  for (int c = 0; c < 3; ++c) {
    const double rd = unit ? d[c] / len : d[c];
    p[c] = o[c] + t * rd;
    n[c] = flip ? -nrm[c] : nrm[c];
  }
}

#endif  // RT_CAMERA_POINT_HPP
