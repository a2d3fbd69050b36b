// refit_check — the bodies of update_records_kernel and refit_nodes4_kernel (rt_update.inc,
// DESIGN.md §24) run on the host over build_image's SceneImage, for sanitizer runs: no GPU is
// used and no HIP call is made (hipcc compiles it because the bodies are __host__ __device__).
//
//   make -C my-raytracer_amd
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -ffp-contract=off -Wno-unused-function \
//       -Xarch_host -fsanitize=address,undefined -Iinclude -Imy-raytracer_amd/csrc tools/refit_check.cpp \
//       -Wl,my-raytracer_amd/lib/device_image.o -Lmy-raytracer_amd/lib -lrt_host \
//       -Wl,-rpath,$PWD/my-raytracer_amd/lib -lpthread -o /tmp/refit_check
//   /tmp/refit_check
//
// Office and cornell, trees sah / sbvh / reference, with and without the breadth-first treelet
// numbering: the odd meshes are moved (A -> B) and moved back (B -> A), the records rewritten and
// the boxes refitted height by height as rt_scene_update_vertices does.  The program fails if after
// A -> B a record's vertex lies outside its leaf slot's box or a child's slot outside its parent's,
// if after A -> B -> A the records differ from the build's, if a reference changed, if a bound
// shrank below the build's, or -- trees without clipping, sah and reference -- if a node differs
// from the build's in any byte.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "rt_host.h"
#include "host/device_image.hpp"
#include "device/rt_refit.hpp"
using namespace rtk;
#define RT_UPDATE_KERNELS_ONLY 1
#include "device/rt_update.inc"

static bool apply(SceneImage& I, const rt_scene_soa* s, double delta) {
  const long long nrec = (long long)I.tris.size();
  for (long long g = 0; g < nrec; ++g)
    update_record_body(g, I.tris.data(), I.shade.data(), I.tnorm.data(), s->vertex_pos, s->vertex_normals,
                       s->face_normals);
  std::vector<uint32_t> order;
  std::vector<long long> lb;
  if (!refit_schedule(I.nodes4, order, lb)) return false;
  for (size_t h = 0; h + 1 < lb.size(); ++h)
    for (long long i = 4 * lb[h]; i < 4 * lb[h + 1]; ++i)
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

// records outside their leaf slot's box + child slots outside their parent's + empty slots not [+inf, -inf]
static long long violations(const SceneImage& I, const rt_scene_soa* s) {
  long long bad = 0;
  for (const GNode4& N : I.nodes4)
    for (int k = 0; k < 4; ++k) {
      const uint32_t ref = N.ref[k];
      if (ref == kEmpty) {
        bad += !(N.lox[k] == INFINITY && N.hix[k] == -INFINITY && N.loy[k] == INFINITY && N.hiy[k] == -INFINITY &&
                 N.loz[k] == INFINITY && N.hiz[k] == -INFINITY);
      } else if (ref & kLeaf) {
        for (size_t g = ref & ~kLeaf;; ++g) {
          for (int c = 0; c < 3; ++c) {
            const double* p = s->vertex_pos + 3 * (size_t)I.shade[g].v[c];
            bad += !(p[0] >= N.lox[k] && p[0] <= N.hix[k] && p[1] >= N.loy[k] && p[1] <= N.hiy[k] &&
                     p[2] >= N.loz[k] && p[2] <= N.hiz[k]);
          }
          if (I.tris[g].meta & kLastDev) break;
        }
      } else {
        const GNode4& C = I.nodes4[ref];
        for (int j = 0; j < 4; ++j)
          if (C.ref[j] != kEmpty)
            bad += !(C.lox[j] >= N.lox[k] && C.hix[j] <= N.hix[k] && C.loy[j] >= N.loy[k] && C.hiy[j] <= N.hiy[k] &&
                     C.loz[j] >= N.loz[k] && C.hiz[j] <= N.hiz[k]);
      }
    }
  return bad;
}

int main() {
  int failures = 0;
  for (const char* kind : {"office", "cornell"})
    for (int tree : {RT_TREE_SAH, RT_TREE_SBVH, RT_TREE_REFERENCE})
      for (int bfs : {73, 0}) {
        rt_host_scene* hs = nullptr;
        if (rt_host_generate(kind, nullptr, &hs) != RT_OK || rt_host_prepare(hs, nullptr) != RT_OK) return 2;
        const rt_scene_soa* s = rt_host_soa(hs);
        rt_upload_options o;
        upload_options_defaults(&o);
        o.device_tree = tree;
        o.build_threads = 8;
        SceneImage A;
        if (build_image(s, rt_host_bvh(hs), o, bfs, A) != RT_OK) return 2;
        const SceneImage A0 = A;
        std::vector<double> posA(s->vertex_pos, s->vertex_pos + 3 * (size_t)s->n_vertices), posB = posA;
        for (int v = 0; v < s->n_vertices; ++v)
          if (s->vertex_mesh_id[v] & 1) {
            posB[3 * (size_t)v] += 0.37;
            posB[3 * (size_t)v + 1] -= 0.11;
            posB[3 * (size_t)v + 2] += 0.23;
          }
        if (rt_host_update_vertices(hs, posB.data(), s->n_vertices) != RT_OK || !apply(A, s, delta_of(s))) return 2;
        const long long bad_b = violations(A, s);
        if (rt_host_update_vertices(hs, posA.data(), s->n_vertices) != RT_OK || !apply(A, s, delta_of(s))) return 2;
        const bool nodes_same = !std::memcmp(A.nodes4.data(), A0.nodes4.data(), A.nodes4.size() * sizeof(GNode4));
        const bool recs_same = !std::memcmp(A.tris.data(), A0.tris.data(), A.tris.size() * sizeof(GTri)) &&
                               !std::memcmp(A.tnorm.data(), A0.tnorm.data(), A.tnorm.size() * sizeof(double));
        long long grown = 0, shrunk = 0, refs = 0;
        for (size_t n = 0; n < A.nodes4.size(); ++n)
          for (int k = 0; k < 4; ++k) {
            const GNode4 &X = A.nodes4[n], &Y = A0.nodes4[n];
            refs += X.ref[k] != Y.ref[k];
            if (X.ref[k] == kEmpty) continue;
            const float xl[3] = {X.lox[k], X.loy[k], X.loz[k]}, xh[3] = {X.hix[k], X.hiy[k], X.hiz[k]};
            const float yl[3] = {Y.lox[k], Y.loy[k], Y.loz[k]}, yh[3] = {Y.hix[k], Y.hiy[k], Y.hiz[k]};
            for (int c = 0; c < 3; ++c) {
              shrunk += (xl[c] > yl[c]) + (xh[c] < yh[c]);
              grown += (xl[c] < yl[c]) + (xh[c] > yh[c]);
            }
          }
        const bool ok = bad_b == 0 && violations(A, s) == 0 && recs_same && refs == 0 && shrunk == 0 &&
                        (tree == RT_TREE_SBVH || nodes_same);
        std::printf("%-8s tree %d treelet %2d: %zu nodes, %zu records; A->B violations %lld; A->B->A nodes %s, records %s, "
                    "bounds grown %lld shrunk %lld  %s\n", kind, tree, bfs, A.nodes4.size(), A.tris.size(), bad_b,
                    nodes_same ? "same" : "differ", recs_same ? "same" : "differ", grown, shrunk, ok ? "ok" : "FAILED");
        failures += !ok;
        rt_host_free(hs);
      }
  return failures ? 1 : 0;
}
