// reclip_check — the body of reclip_nodes4_kernel (rt_update.inc) run on the host over
// build_image's SceneImage, for sanitizer runs: no GPU is used and no HIP call is made (hipcc
// compiles it because the bodies are __host__ __device__).
//
//   make -C my-raytracer_amd
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -ffp-contract=off -Wno-unused-function \
//       -Xarch_host -fsanitize=address,undefined -Iinclude -Imy-raytracer_amd/csrc tools/reclip_check.cpp \
//       -Wl,my-raytracer_amd/lib/device_image.o -Lmy-raytracer_amd/lib -lrt_host \
//       -Wl,-rpath,$PWD/my-raytracer_amd/lib -lpthread -o /tmp/reclip_check
//   /tmp/reclip_check
//
// Office and cornell, tree sbvh, with and without the breadth-first treelet numbering.  The odd
// meshes are moved (A -> B) and the boxes refitted height by height as rt_scene_update_vertices_ex
// does, once plainly and once re-clipped.  The program fails if after A -> B (re-clipped) a child's
// slot lies outside its parent's, if one of 32 barycentric samples of a record's triangle that falls
// in the record's clip region lies outside its leaf slot's box, if a re-clipped bound exceeds the
// plain refit's, if a reference changed, or if after A -> A (re-clipped, from the build's image) a
// bound is more than one fp32 step from the build's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "rt_host.h"
#include "host/device_image.hpp"
#include "device/rt_refit.hpp"
#include "device/rt_reclip.hpp"
using namespace rtk;
#define RT_UPDATE_KERNELS_ONLY 1
#include "device/rt_update.inc"

static bool apply(SceneImage& I, const rt_scene_soa* s, double delta, bool reclip) {
  const long long nrec = (long long)I.tris.size();
  for (long long g = 0; g < nrec; ++g)
    update_record_body(g, I.tris.data(), I.shade.data(), I.tnorm.data(), s->vertex_pos, s->vertex_normals,
                       s->face_normals);
  std::vector<uint32_t> order;
  std::vector<long long> lb;
  if (!refit_schedule(I.nodes4, order, lb)) return false;
  for (size_t h = 0; h + 1 < lb.size(); ++h)
    for (long long i = 4 * lb[h]; i < 4 * lb[h + 1]; ++i)
      if (reclip)
        reclip_slot_body(order[i >> 2], (int)(i & 3), I.nodes4.data(), (uint32_t)I.nodes4.size(), I.tris.data(),
                         I.shade.data(), nrec, s->vertex_pos, delta, I.clip->idx.data(), I.clip->box.data());
      else
        refit_slot_body(order[i >> 2], (int)(i & 3), I.nodes4.data(), (uint32_t)I.nodes4.size(), I.tris.data(),
                        I.shade.data(), nrec, s->vertex_pos, delta);
  return true;
}

static double delta_of(const rt_scene_soa* s) {
  double M = 0;
  for (long long k = 0; k < 3LL * s->n_vertices; ++k) M = std::max(M, std::fabs(s->vertex_pos[k]));
  if (!(M > 0)) M = 1;
  return M * 9.5367431640625e-07;
}

struct Bounds { float lo[3], hi[3]; };
static Bounds slot_box(const GNode4& N, int k) {
  return {{N.lox[k], N.loy[k], N.loz[k]}, {N.hix[k], N.hiy[k], N.hiz[k]}};
}

// child slots outside their parent's + samples of a record's triangle inside the record's region but
// outside the leaf slot's box + empty slots not [+inf, -inf]; *empty_leaves: leaf slots with the empty box
static long long violations(const SceneImage& I, const rt_scene_soa* s, long long* samples, long long* empty_leaves) {
  long long bad = 0;
  uint64_t rng = 0x9e3779b97f4a7c15ull;
  auto uni = [&]() {
    rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17;
    return (double)(rng >> 11) / 9007199254740992.0;
  };
  for (const GNode4& N : I.nodes4)
    for (int k = 0; k < 4; ++k) {
      const uint32_t ref = N.ref[k];
      const Bounds b = slot_box(N, k);
      if (ref == kEmpty) {
        for (int c = 0; c < 3; ++c) bad += !(b.lo[c] == INFINITY && b.hi[c] == -INFINITY);
      } else if (ref & kLeaf) {
        *empty_leaves += b.lo[0] == INFINITY && b.hi[0] == -INFINITY;
        for (size_t g = ref & ~kLeaf;; ++g) {
          const double* p[3];
          for (int c = 0; c < 3; ++c) p[c] = s->vertex_pos + 3 * (size_t)I.shade[g].v[c];
          const int32_t row = I.clip->idx[g];
          for (int n = 0; n < 32; ++n) {
            double u = uni(), v = uni();
            if (u + v > 1.0) { u = 1.0 - u; v = 1.0 - v; }
            if (n < 3) { u = n == 0; v = n == 1; }   // the vertices themselves
            bool in_region = true, in_box = true;
            for (int c = 0; c < 3; ++c) {
              const double x = p[2][c] + u * (p[0][c] - p[2][c]) + v * (p[1][c] - p[2][c]);
              if (row >= 0) in_region = in_region && x >= I.clip->box[6 * (size_t)row + c] && x <= I.clip->box[6 * (size_t)row + 3 + c];
              in_box = in_box && x >= b.lo[c] && x <= b.hi[c];
            }
            *samples += in_region;
            bad += in_region && !in_box;
          }
          if (I.tris[g].meta & kLastDev) break;
        }
      } else {
        const GNode4& C = I.nodes4[ref];
        for (int j = 0; j < 4; ++j) {
          if (C.ref[j] == kEmpty) continue;
          const Bounds c = slot_box(C, j);
          if (c.lo[0] == INFINITY && c.hi[0] == -INFINITY) continue;   // an emptied leaf slot lies in every box
          for (int a = 0; a < 3; ++a) bad += !(c.lo[a] >= b.lo[a] && c.hi[a] <= b.hi[a]);
        }
      }
    }
  return bad;
}

// bounds of X beyond Y's (X must lie inside Y), bounds where they differ, bounds more than one fp32 step apart
static void compare(const SceneImage& X, const SceneImage& Y, long long* beyond, long long* differ, long long* far,
                    long long* refs) {
  for (size_t n = 0; n < X.nodes4.size(); ++n)
    for (int k = 0; k < 4; ++k) {
      *refs += X.nodes4[n].ref[k] != Y.nodes4[n].ref[k];
      if (X.nodes4[n].ref[k] == kEmpty) continue;
      const Bounds x = slot_box(X.nodes4[n], k), y = slot_box(Y.nodes4[n], k);
      for (int c = 0; c < 3; ++c) {
        *beyond += (x.lo[c] < y.lo[c]) + (x.hi[c] > y.hi[c]);
        *differ += (x.lo[c] != y.lo[c]) + (x.hi[c] != y.hi[c]);
        *far += !(x.lo[c] == y.lo[c] || rt_refit_step(x.lo[c], true) == y.lo[c] || rt_refit_step(x.lo[c], false) == y.lo[c]);
        *far += !(x.hi[c] == y.hi[c] || rt_refit_step(x.hi[c], true) == y.hi[c] || rt_refit_step(x.hi[c], false) == y.hi[c]);
      }
    }
}

int main() {
  int failures = 0;
  for (const char* kind : {"office", "cornell"})
    for (int bfs : {73, 0}) {
      rt_host_scene* hs = nullptr;
      if (rt_host_generate(kind, nullptr, &hs) != RT_OK || rt_host_prepare(hs, nullptr) != RT_OK) return 2;
      const rt_scene_soa* s = rt_host_soa(hs);
      rt_upload_options o;
      upload_options_defaults(&o);
      o.device_tree = RT_TREE_SBVH;
      o.build_threads = 8;
      SceneImage A0;
      if (build_image(s, rt_host_bvh(hs), o, bfs, A0) != RT_OK) return 2;
      if (!A0.clip || A0.clip->idx.size() != A0.tris.size() || A0.tris.size() <= (size_t)A0.n_tris) return 2;
      long long cut = 0;
      for (const int32_t r : A0.clip->idx) {
        if (r < -1 || (r >= 0 && 6 * (size_t)r + 6 > A0.clip->box.size())) return 2;
        cut += r >= 0;
      }
      // A -> A, re-clipped, from the build's image
      SceneImage AA = A0;
      if (!apply(AA, s, delta_of(s), true)) return 2;
      long long aa_beyond = 0, aa_differ = 0, aa_far = 0, aa_refs = 0;
      compare(AA, A0, &aa_beyond, &aa_differ, &aa_far, &aa_refs);
      const bool recs_same = !std::memcmp(AA.tris.data(), A0.tris.data(), AA.tris.size() * sizeof(GTri));
      // A -> B, plain and re-clipped
      std::vector<double> posB(s->vertex_pos, s->vertex_pos + 3 * (size_t)s->n_vertices);
      for (int v = 0; v < s->n_vertices; ++v)
        if (s->vertex_mesh_id[v] & 1) {
          posB[3 * (size_t)v] += 0.37;
          posB[3 * (size_t)v + 1] -= 0.11;
          posB[3 * (size_t)v + 2] += 0.23;
        }
      if (rt_host_update_vertices(hs, posB.data(), s->n_vertices) != RT_OK) return 2;
      SceneImage P = A0, R = A0;
      if (!apply(P, s, delta_of(s), false) || !apply(R, s, delta_of(s), true)) return 2;
      long long samples = 0, empty_leaves = 0;
      const long long bad = violations(R, s, &samples, &empty_leaves);
      long long beyond = 0, differ = 0, far = 0, refs = 0;
      compare(R, P, &beyond, &differ, &far, &refs);
      const bool ok = bad == 0 && beyond == 0 && refs == 0 && differ > 0 && aa_far == 0 && aa_refs == 0 && recs_same &&
                      samples > (long long)A0.tris.size();
      std::printf("%-8s treelet %2d: %zu nodes, %zu records, %lld cut; A->A bounds differing %lld, beyond one step %lld; "
                  "A->B violations %lld of %lld samples, bounds beyond the plain refit's %lld, tighter %lld, emptied leaf "
                  "slots %lld  %s\n", kind, bfs, A0.nodes4.size(), A0.tris.size(), cut, aa_differ, aa_far, bad, samples,
                  beyond, differ, empty_leaves, ok ? "ok" : "FAILED");
      failures += !ok;
      rt_host_free(hs);
    }
  return failures ? 1 : 0;
}
