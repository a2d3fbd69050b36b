// tree_opt_check — the hierarchy optimiser (rt_upload_options.tree_opt) as a
// stand-alone host program, for sanitizer runs: nothing here touches HIP or Python.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -ffp-contract=off \
//       -Iinclude tools/tree_opt_check.cpp my-raytracer_amd/csrc/host/device_image.cpp \
//       my-raytracer_amd/csrc/host/host_scene.cpp my-raytracer_amd/csrc/host/loader.cpp \
//       my-raytracer_amd/csrc/host/generators.cpp -lz -lpthread -o /tmp/tree_opt_check
//   python tests/tree_opt_scenes.py /tmp/tree_opt_scenes      # writes the hand-made scenes as .sce
//   /tmp/tree_opt_check office cornell:3 random_tris:20000 /tmp/tree_opt_scenes/*.sce
//
// Each argument is a generator ("kind", "kind:detail" or "random_tris:count") or a .sce path.  Every
// scene goes through rt_debug_tree_report with tree_opt -1, the default and RT_TREE_OPT_MAX, on 1 and
// 7 build threads; the program fails on a validity bit, a cost that rose, a converged run that is
// not a fixed point, or reports that differ between the thread counts.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "rt_hip.h"
#include "rt_host.h"

static bool same(const rt_tree_report& a, const rt_tree_report& b) {
  return a.binary_nodes == b.binary_nodes && a.wide_nodes == b.wide_nodes && a.records == b.records &&
         a.moved == b.moved && a.sah_before == b.sah_before && a.sah_after == b.sah_after &&
         a.dp_before == b.dp_before && a.dp_after == b.dp_after && a.passes == b.passes && a.stack4 == b.stack4 &&
         a.invalid == b.invalid && a.converged == b.converged;
}

int main(int argc, char** argv) {
  int failures = 0;
  for (int i = 1; i < argc; ++i) {
    const std::string arg = argv[i];
    rt_host_scene* hs = nullptr;
    int rc;
    if (arg.size() > 4 && arg.compare(arg.size() - 4, 4, ".sce") == 0) {
      rc = rt_host_load(arg.c_str(), &hs);
    } else {
      rt_gen_params gp;
      std::memset(&gp, 0, sizeof gp);
      gp.max_depth = -1;
      std::string kind = arg;
      const size_t colon = arg.find(':');
      if (colon != std::string::npos) {
        kind = arg.substr(0, colon);
        const long long v = std::atoll(arg.c_str() + colon + 1);
        if (kind == "random_tris") gp.n_triangles = v; else gp.detail = (int)v;
      }
      rc = rt_host_generate(kind.c_str(), &gp, &hs);
    }
    if (rc != RT_OK || rt_host_prepare(hs, nullptr) != RT_OK) {
      std::fprintf(stderr, "%s: cannot load or prepare the scene\n", arg.c_str());
      return 2;
    }
    const int modes[3] = {-1, 0, RT_TREE_OPT_MAX};
    rt_tree_report off{};
    for (int m = 0; m < 3; ++m) {
      rt_tree_report r[2];
      for (int t = 0; t < 2; ++t) {
        rt_upload_options o;   // zero fields = defaults / by size, then the shipped tree and collapse
        std::memset(&o, 0, sizeof o);
        o.device_tree = RT_TREE_SBVH;
        o.collapse = RT_COLLAPSE_SAH;
        o.sbvh_alpha = o.sbvh_budget = -1.0;
        o.build_threads = t == 0 ? 1 : 7;
        o.tree_opt = modes[m];
        if (rt_debug_tree_report(rt_host_soa(hs), rt_host_bvh(hs), &o, &r[t]) != RT_OK) {
          std::fprintf(stderr, "%s: rt_debug_tree_report failed\n", arg.c_str());
          return 2;
        }
      }
      if (m == 0) off = r[0];
      bool ok = r[0].invalid == 0 && same(r[0], r[1]) && r[0].sah_after <= r[0].sah_before &&
                r[0].dp_after <= r[0].dp_before && r[0].binary_nodes == off.binary_nodes && r[0].records == off.records;
      if (m == 0) ok = ok && r[0].passes == 0;
      if (m == 2) ok = ok && r[0].converged == 1;
      std::printf("%-40s tree_opt %3d: %s  nodes %lld wide %lld records %lld passes %d moved %lld sah %.4f -> %.4f "
                  "dp %.4f -> %.4f stack4 %d invalid %u\n", arg.c_str(), modes[m], ok ? "ok  " : "FAIL", r[0].binary_nodes,
                  r[0].wide_nodes, r[0].records, r[0].passes, r[0].moved, r[0].sah_before, r[0].sah_after, r[0].dp_before,
                  r[0].dp_after, r[0].stack4, r[0].invalid);
      failures += !ok;
    }
    rt_host_free(hs);
  }
  std::printf("%d failure(s)\n", failures);
  return failures ? 1 : 0;
}
