// normals_check — the bodies of face_normals_kernel, vertex_normals_kernel and bounds_reduce_kernel
// (rt_normals.inc) run on the host against HostMesh::compute_normals, for sanitizer
// runs: no GPU is used and no HIP call is made (hipcc compiles it because the bodies are
// __host__ __device__).
//
//   make -C my-raytracer_amd
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -ffp-contract=off -Wno-unused-function \
//       -Xarch_host -fsanitize=address,undefined -Iinclude -Imy-raytracer_amd/csrc tools/normals_check.cpp \
//       -Lmy-raytracer_amd/lib -lrt_host -Wl,-rpath,$PWD/my-raytracer_amd/lib -lpthread -o /tmp/normals_check
//   /tmp/normals_check
//
// Office and cornell, as prepared and with the odd meshes moved: the tables are built from the SoA's
// leaf-order vertex ids and rt_host_slot_triangles, the bodies run slot by slot and vertex by
// vertex, and both normal arrays must equal the SoA's (compute_normals' results) byte for byte.  A
// fan of 100 triangles around one apex with an unreferenced vertex, and a mesh with a vertex named
// twice, a zero-area triangle and a corner weight under the threshold, are made as HostMesh and
// compared the same way, their triangles in a reversed slot order.  The reduction's bodies run as
// 1, 3 and 64 threads and must give max|value| and the referenced vertices' box of the sequential
// loops.  One line per case, "ok" at its end; exit status 1 if any differs.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "rt_host.h"
#include "host/host_scene.hpp"
#include "device/rt_layout.hpp"
#include "device/rt_refit.hpp"
#include "device/rt_reclip.hpp"
#include "device/rt_normals.hpp"
using namespace rtk;
#define RT_UPDATE_KERNELS_ONLY 1
#include "device/rt_update.inc"
#include "device/rt_normals.inc"

// the bodies over leaf-order ids: false if the tables cannot be built
static bool run_bodies(const int* vertex_idx, const int* slot_triangle, long long nv, long long nt, const double* pos,
                       std::vector<double>& vn, std::vector<double>& fn) {
  std::vector<int32_t> slot_vid;
  std::vector<uint32_t> begin, corner;
  if (!normals_is_permutation(slot_triangle, nt) ||
      !normals_tables(vertex_idx, 3, slot_triangle, nv, nt, slot_vid, begin, corner))
    return false;
  std::vector<double> weight(4 * (size_t)nt, NAN);
  vn.assign(3 * (size_t)nv, NAN);
  fn.assign(3 * (size_t)nt, NAN);
  for (long long s = 0; s < nt; ++s) face_normal_body(s, slot_vid.data(), pos, fn.data(), weight.data());
  for (long long v = 0; v < nv; ++v) vertex_normal_body(v, begin.data(), corner.data(), fn.data(), weight.data(), vn.data());
  return true;
}

static bool same(const std::vector<double>& a, const double* b) {
  return a.empty() || std::memcmp(a.data(), b, a.size() * sizeof(double)) == 0;
}

// bounds bodies as `threads` threads against the sequential loops of rt_scene_update_vertices_ex
static bool bounds_ok(const double* pos, long long nv, const std::vector<int32_t>& used, int threads, int aligned) {
  double M = 0.0, lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (long long k = 0; k < 3 * nv; ++k) M = std::max(M, std::fabs(pos[k]));
  for (const int32_t v : used) rt_refit_grow(lo, hi, pos + 3 * (size_t)v);
  double all[7];
  bounds_identity(all);
  for (int t = 0; t < threads; ++t) {
    double b[7];
    bounds_identity(b);
    bounds_thread_body(t, threads, pos, 3 * nv, aligned, used.data(), (long long)used.size(), b);
    bounds_merge(all, b);
  }
  bool ok = all[0] == M;
  for (int k = 0; k < 3; ++k) ok = ok && all[1 + k] == lo[k] && all[4 + k] == hi[k];
  return ok;
}

static int check_generated(const char* kind) {
  rt_host_scene* hs = nullptr;
  if (rt_host_generate(kind, nullptr, &hs) != RT_OK || rt_host_prepare(hs, nullptr) != RT_OK) return 2;
  const rt_scene_soa* s = rt_host_soa(hs);
  const long long nv = s->n_vertices, nt = s->n_vertex_idx / 3;
  const int* order = rt_host_slot_triangles(hs);
  std::vector<double> pos(s->vertex_pos, s->vertex_pos + 3 * (size_t)nv), vn, fn;
  std::vector<uint8_t> seen((size_t)nv, 0);
  std::vector<int32_t> used;
  for (long long i = 0; i < 3 * nt; ++i) seen[(size_t)s->vertex_idx[i]] = 1;
  for (long long v = 0; v < nv; ++v)
    if (seen[(size_t)v]) used.push_back((int32_t)v);
  int failures = 0;
  for (int moved = 0; moved < 2; ++moved) {
    if (moved) {
      for (long long v = 0; v < nv; ++v)
        if (s->vertex_mesh_id[v] & 1) {
          pos[3 * (size_t)v] += 0.37;
          pos[3 * (size_t)v + 1] -= 0.11;
          pos[3 * (size_t)v + 2] += 0.23;
        }
      if (rt_host_update_vertices(hs, pos.data(), nv) != RT_OK) return 2;
    }
    if (!run_bodies(s->vertex_idx, order, nv, nt, pos.data(), vn, fn)) return 2;
    const bool nrm = same(vn, s->vertex_normals) && same(fn, s->face_normals);
    bool bnd = true;
    for (int threads : {1, 3, 64}) bnd = bnd && bounds_ok(pos.data(), nv, used, threads, 1) && bounds_ok(pos.data(), nv, used, threads, 0);
    std::printf("%-10s %s: %lld vertices, %lld triangles; normals %s, bounds %s  %s\n", kind, moved ? "moved   " : "prepared",
                nv, nt, nrm ? "==" : "DIFFER", bnd ? "==" : "DIFFER", nrm && bnd ? "ok" : "FAILED");
    failures += !(nrm && bnd);
  }
  rt_host_free(hs);
  return failures;
}

// a HostMesh against the bodies, its triangles in reversed slot order
static int check_mesh(const char* name, rt::HostMesh& m) {
  m.compute_normals();
  const long long nv = m.n_vertices(), nt = m.n_triangles();
  std::vector<int> vidx(3 * (size_t)nt), order((size_t)nt);
  std::vector<double> want_fn(3 * (size_t)nt), vn, fn;
  for (long long s = 0; s < nt; ++s) {
    const long long t = nt - 1 - s;
    order[(size_t)s] = (int)t;
    for (int c = 0; c < 3; ++c) {
      vidx[3 * (size_t)s + c] = m.tri_vertex[3 * (size_t)t + c];
      want_fn[3 * (size_t)s + c] = m.face_normals[3 * (size_t)t + c];
    }
  }
  if (!run_bodies(vidx.data(), order.data(), nv, nt, m.positions.data(), vn, fn)) return 2;
  const bool ok = same(vn, m.vertex_normals.data()) && same(fn, want_fn.data());
  std::printf("%-10s as made : %lld vertices, %lld triangles; normals %s  %s\n", name, nv, nt, ok ? "==" : "DIFFER",
              ok ? "ok" : "FAILED");
  return !ok;
}

int main() {
  int failures = 0;
  for (const char* kind : {"office", "cornell"}) {
    const int rc = check_generated(kind);
    if (rc == 2) return 2;
    failures += rc;
  }
  {
    rt::HostMesh fan;
    const int n = 100;
    fan.positions = {0.0, 1.0, 0.0};
    for (int i = 0; i < n; ++i) {
      const double a = 2.0 * M_PI * i / n;
      fan.positions.insert(fan.positions.end(), {1.5 * std::cos(a), 0.3 * std::sin(7.0 * a), 1.5 * std::sin(a)});
    }
    fan.positions.insert(fan.positions.end(), {-50.0, 0.25, 0.5});   // referenced by no triangle
    for (int i = 0; i < n; ++i) fan.tri_vertex.insert(fan.tri_vertex.end(), {0, 1 + (i + 1) % n, 1 + i});
    failures += check_mesh("fan", fan);
  }
  {
    rt::HostMesh odd;
    odd.positions = {0, 0, 0,  1, 0, 0,  2, 0, 0,  -1, 0.5, 0,  1, 0.5, 0,  0, 0.5 + 1e-7, 0,  0, 1, 0,  1, 1.5, 0.2,
                     -1, -0.5, 0.5,  1, -0.5, 0.5,  0, 1.2, -0.5};
    odd.tri_vertex = {8, 9, 10,  6, 6, 7,  8, 10, 3,  0, 1, 2,  9, 4, 10,  5, 3, 4,  3, 10, 6,  0, 8, 5,  7, 4, 2};
    failures += check_mesh("degenerate", odd);
    // NaN positions: outside the bit-for-bit contract, but every index stays in range
    odd.positions[3 * 10 + 1] = NAN;
    std::vector<double> vn, fn;
    std::vector<int> order(odd.tri_vertex.size() / 3);
    for (size_t t = 0; t < order.size(); ++t) order[t] = (int)t;
    if (!run_bodies(odd.tri_vertex.data(), order.data(), odd.n_vertices(), odd.n_triangles(), odd.positions.data(), vn, fn))
      return 2;
    std::printf("%-10s with NaN: ran  ok\n", "degenerate");
  }
  return failures ? 1 : 0;
}
