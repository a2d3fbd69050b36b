// rt_walk_body.inc — one ray per lane through the device hierarchy: the walk that query_kernel
// (rt_query.inc), ao_kernel (rt_ao.inc) and camera_kernel (rt_camera.inc) share (DESIGN.md §15, §23).
// Text, not a function (as a function it cost camera_kernel scratch, §23): no include guard, included
// once inside a kernel's per-item loop, at statement level.  It holds the degenerate-ray test, the
// analytic primitives, the conservative fp32 box ray, the LDS stack ring with its spill rows, the
// 4-wide node loop with the LDS treelet, the postponed leaf, both watchdog bounds and the CPU's fp64
// triangle test, so a ray's result is the same bits in every kernel that includes it.
//
// Expects in scope:
//   ANYHIT       compile-time bool: true = occlusion (first hit ends the walk, no child sort),
//                false = closest hit (the smallest (t, reference slot))
//   P            the kernel's parameter struct; read: nodes4, tris, prims, ctr, spill_rows, nslots,
//                guard_host, n_gnodes, n_prims, n_top, root_lo, root_hi
//   q_ring       __shared__ uint32_t[kQRing * kBlock], the stack ring [entry][kBlock]
//   q_top        __shared__ float4[], the top treelet (query_stage_treelet)
//   spill        uint32_t*: the lane's column of the context's spill array
//   lane         int: threadIdx.x & 63
//   act0         bool: the lane holds a ray
//   ro, dv       D3: origin and (unnormalised) direction
//   tmax         double
//   n_spills, n_trips   the lane's unsigned long long counters, added to
// Leaves behind (among its locals, which stay in scope):
//   rd           D3: the normalised direction
//   tlim         double: the hit's t where best != kNoHit
//   best, best_slot, best_mesh, best_a, best_b   closest hit: the record (kPrimHit | k for an
//                analytic primitive), its reference slot, mesh and barycentrics; best == kNoHit: a miss
//   occluded     bool: the any-hit answer
// With RT_WALK_KHITS defined before the #include (hits_kernel, rt_hits.inc, alone: the text the other
// kernels compile is unchanged) an accepted triangle goes into the lane's k-buffer instead of `best`,
// and the analytic primitives are left out.  Then also expected in scope, ANYHIT being false:
//   kh_after_t, kh_after_slot   double, int: the resume key (-inf, -1: none)
//   kh_full      bool: the buffer holds k entries
//   kh_last_t    double: then its last entry's t
//   kh_insert(t, slot, record) -> bool: keeps the candidate if it belongs; true = the bound moved
    // degenerate rays are misses and are never traversed
    const double dlen = sqrt(dot(dv, dv));
    const bool act = act0 && q_finite(ro.x) && q_finite(ro.y) && q_finite(ro.z) && q_finite(dv.x) &&
                     q_finite(dv.y) && q_finite(dv.z) && dlen > 0.0 && tmax > 1e-5;   // NaN tmax: false
    const D3 rd = normalize(dv);
    // a hit counts iff 1e-5 < t < tmax; t = DBL_MAX is never one (the oracle's "no hit" value)
    double tlim = tmax < DBL_MAX ? tmax : DBL_MAX;
    int best = kNoHit, best_slot = kNoHit, best_mesh = -1;
    double best_a = 0.0, best_b = 0.0;
    bool occluded = false;
    uint32_t cur = kDone;
    double t_off = 0.0;
    // analytic primitives first, in scene order (oracle intersect_scene): only a strictly closer
    // triangle replaces them; an occlusion ray they block skips the hierarchy
#ifndef RT_WALK_KHITS   // (a hit list holds triangles only: rt_trace_hits refuses a scene with primitives)
    for (int k = 0; k < P.n_prims; ++k) {
      if (!act || occluded) break;
      const double t = prim_hit(P.prims[k], ro, rd);
      if (t < tlim) {
        if (ANYHIT) { occluded = true; break; }
        tlim = t;
        best = kPrimHit | k;
        best_slot = -1;
      }
    }
#endif
    if (act && P.n_gnodes > 0 && !occluded) {   // conservative fp32 box ray (oracle gray_setup)
      bool miss = false;
      const double o3[3] = {ro.x, ro.y, ro.z}, d3v[3] = {rd.x, rd.y, rd.z};
      bool inside = true;
#pragma unroll
      for (int k = 0; k < 3; ++k)
        if (!(o3[k] >= P.root_lo[k] && o3[k] <= P.root_hi[k])) inside = false;
      if (!inside) {
        double tn = -DBL_MAX, tf = DBL_MAX;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          if (d3v[k] == 0.0) {
            if (o3[k] < P.root_lo[k] || o3[k] > P.root_hi[k]) miss = true;
            continue;
          }
          double t0 = (P.root_lo[k] - o3[k]) / d3v[k];
          double t1 = (P.root_hi[k] - o3[k]) / d3v[k];
          if (t0 > t1) { const double t = t0; t0 = t1; t1 = t; }
          if (t0 > tn) tn = t0;
          if (t1 < tf) tf = t1;
        }
        if (tn > tf || tf < 0.0) miss = true;
        t_off = tn > 0.0 ? tn : 0.0;
      }
      if (miss) t_off = 0.0;
      else cur = 0;
    }
    float inv[3];
    {
      const double d3v[3] = {rd.x, rd.y, rd.z};
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        float df = (float)d3v[k];
        if (fabsf(df) < 1e-20f) df = signbit(d3v[k]) ? -1e-20f : 1e-20f;
        const float r0 = __builtin_amdgcn_rcpf(df);   // v_rcp_f32 + one Newton step
        inv[k] = __builtin_fmaf(__builtin_fmaf(-df, r0, 1.0f), r0, r0);
      }
    }
    const float ofx = (float)(ro.x + t_off * rd.x);
    const float ofy = (float)(ro.y + t_off * rd.y);
    const float ofz = (float)(ro.z + t_off * rd.z);
    const float ivx = inv[0], ivy = inv[1], ivz = inv[2];
    // per-ray near / far plane byte offsets in the node and o * inv: one FMA per slab
    const uint32_t nxo = ivx >= 0.f ? 0u : 16u, nyo = ivy >= 0.f ? 32u : 48u, nzo = ivz >= 0.f ? 64u : 80u;
    const float oix = ofx * ivx, oiy = ofy * ivy, oiz = ofz * ivz;
    const float lo_c = round_down_f(-t_off);
    float hi_c = round_up_f(tlim - t_off);   // tightened as tlim shrinks
    // logical stack [0, sp): the LDS ring holds [slo, sp), spill[] holds [0, slo)
    uint32_t sp = 0, slo = 0;
    bool overflow = false;
    auto ring = [&](uint32_t i) -> uint32_t& { return q_ring[(i & (uint32_t)kQRingMask) * kBlock + threadIdx.x]; };
    auto push = [&](uint32_t x) {
      if (sp - slo == (uint32_t)kQRing) {   // ring full: its bottom entry goes to the spill stack
        if ((int)slo < P.spill_rows) spill[(size_t)slo * P.nslots] = ring(slo);
        else overflow = true;   // deeper than the hierarchy's bound (never on a sound hierarchy)
        slo++;
        n_spills++;
      }
      ring(sp) = x;
      sp++;
    };
    auto pop = [&]() -> uint32_t {
      if (sp == 0) return kDone;
      sp--;
      if (sp >= slo) return ring(sp);
      slo = sp;
      return (int)sp < P.spill_rows ? spill[(size_t)sp * P.nslots] : kDone;
    };
    const D3 c3 = d3(-rd.x, -rd.y, -rd.z);
    auto guard_trip = [&]() {
      if (lane == __ffsll((long long)wballot(1)) - 1) {
        trip_watchdog(P.ctr, P.guard_host);
        n_trips++;
      }
    };
    // tests the records of leaf `lref` in order; true = the occlusion ray is blocked
    auto test_leaf = [&](uint32_t lref) -> bool {
      uint32_t i = lref & ~kLeaf;
      // a linear scan to the record flagged last of its leaf: it cannot cycle
      for (;;) {
        const TriOps T = load_tri(P.tris, i);
        const int slot = (int)(T.meta & kSlotMask);
        // Mesh::intersect_triangle: the CPU's fp64 S, Da, Db, Dt (same operands, same order), with
        // the render kernel's division-free early rejections, which fire only where the CPU's
        // quotients certainly fail (DESIGN.md §4)
        D3 c4 = sub(ro, T.p2);
        const double S = det3(T.e1, T.e2, c3);
        asm volatile("" : "+v"(c4.x), "+v"(c4.y), "+v"(c4.z));   // the record's loads stay one batch
        if (fabs(S) >= 1e-10) {
          const double Da = det3(c4, T.e2, c3);
          const double Db = det3(T.e1, c4, c3);
          const double sS = S > 0.0 ? 1.0 : -1.0;
          const double aS = fabs(S);
          const double ua = Da * sS, ub = Db * sS;
          const double tiny = aS * 0x1p-1000, big = aS * (1.0 + 0x1p-48);
          const bool out = (ua < 0.0 && -ua >= tiny) || (ub < 0.0 && -ub >= tiny) || ua > big || ub > big ||
                           (Da + Db - S) * sS > 0x1p-40 * (fabs(Da) + fabs(Db) + aS);
          if (!out) {
            const double Dt = det3(T.e1, T.e2, c4);
            const double t = Dt / S;
#ifdef RT_WALK_KHITS
            // past the resume key, and inside tmax (exclusive) or the full buffer's last t (inclusive:
            // an equal t still reaches the slot tie-break)
            const bool cand = (kh_full ? t <= tlim : t < tlim) && (t > kh_after_t || (t == kh_after_t && slot > kh_after_slot));
#else
            const bool cand = ANYHIT ? (t < tlim) : (t <= tlim);
#endif
            if (t > 1e-5 && cand) {
              double alpha, beta;
              // one reciprocal of S for both quotients where that is bit-identical (rt_render.hip)
              const double lim = aS * 0x1p-900;
              if (fabs(Da) >= lim && fabs(Db) >= lim && aS < 0x1p1000) {
                const double r = rcp_refined(S);
                alpha = div_by(Da, S, r);
                beta = div_by(Db, S, r);
              } else {
                alpha = Da / S;
                beta = Db / S;
              }
              const double gamma = (1.0 - alpha - beta);
              const bool in = (0.0 <= alpha && alpha <= 1.0) && (0.0 <= beta && beta <= 1.0) &&
                              (0.0 <= gamma && gamma <= 1.0);
              if (in) {
                if (ANYHIT) return true;
#ifdef RT_WALK_KHITS
                // into the lane's k-buffer (rt_hits.inc); once it is full its last t is the far bound
                if (kh_insert(t, slot, i)) {
                  tlim = kh_last_t;
                  hi_c = round_up_f(tlim - t_off);
                }
#else
                // strictly closer, or a tie with an earlier hit: smallest reference slot
                if (t < tlim || (best != kNoHit && slot < best_slot)) {
                  tlim = t;
                  best = (int)i;
                  best_slot = slot;
                  best_mesh = T.mesh;
                  best_a = alpha;
                  best_b = beta;
                  hi_c = round_up_f(tlim - t_off);
                }
#endif
              }
            }
          }
        }
        if (T.meta & kLastDev) break;
        ++i;
      }
      return false;
    };
    uint32_t pleaf = kDone;   // postponed leaf
    uint32_t rounds = 0;
    while ((wballot(cur != kDone) | wballot(pleaf != kDone)) != 0) {
      if (++rounds > kTravGuard) {   // watchdog: abandon the rays (results void, scene flagged)
        guard_trip();
        cur = kDone;
        pleaf = kDone;
        break;
      }
      for (uint32_t it = 0; !(cur & kLeaf); ++it) {   // 4-wide node (kDone carries the leaf bit)
        if (it > kTravGuard) { guard_trip(); cur = kDone; pleaf = kDone; break; }
        float k[4];
        uint32_t v[4];
        bool hb[4];
        int cnt = 0;
        float4 nx, fx, ny, fy, nz, fz;
        uint4 rf;
        const uint32_t nbo = cur * (uint32_t)sizeof(GNode4);
        // wave-uniform: every active lane's node is in the LDS treelet
        const bool in_lds = wballot(cur >= (uint32_t)P.n_top) == 0;
        const char* nbase = reinterpret_cast<const char*>(P.nodes4);
#define RT_QNODE_AT(off) (nbase + (uint32_t)(nbo + (off)))
        if (in_lds) {
          const unsigned char* lb = reinterpret_cast<const unsigned char*>(q_top) + nbo;
          nx = *reinterpret_cast<const float4*>(lb + nxo);
          fx = *reinterpret_cast<const float4*>(lb + (nxo ^ 16u));
          ny = *reinterpret_cast<const float4*>(lb + nyo);
          fy = *reinterpret_cast<const float4*>(lb + (nyo ^ 16u));
          nz = *reinterpret_cast<const float4*>(lb + nzo);
          fz = *reinterpret_cast<const float4*>(lb + (nzo ^ 16u));
          rf = *reinterpret_cast<const uint4*>(lb + 96);
        } else {
          nx = *reinterpret_cast<const float4*>(RT_QNODE_AT(nxo));
          fx = *reinterpret_cast<const float4*>(RT_QNODE_AT(nxo ^ 16u));
          ny = *reinterpret_cast<const float4*>(RT_QNODE_AT(nyo));
          fy = *reinterpret_cast<const float4*>(RT_QNODE_AT(nyo ^ 16u));
          nz = *reinterpret_cast<const float4*>(RT_QNODE_AT(nzo));
          fz = *reinterpret_cast<const float4*>(RT_QNODE_AT(nzo ^ 16u));
          rf = *reinterpret_cast<const uint4*>(RT_QNODE_AT(96u));
        }
#undef RT_QNODE_AT
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const float tx0 = __builtin_fmaf(f4c(nx, c), ivx, -oix), tx1 = __builtin_fmaf(f4c(fx, c), ivx, -oix);
          const float ty0 = __builtin_fmaf(f4c(ny, c), ivy, -oiy), ty1 = __builtin_fmaf(f4c(fy, c), ivy, -oiy);
          const float tz0 = __builtin_fmaf(f4c(nz, c), ivz, -oiz), tz1 = __builtin_fmaf(f4c(fz, c), ivz, -oiz);
          const float tn = fmaxf(fmaxf(tx0, ty0), fmaxf(tz0, lo_c));
          const float tf = fminf(fminf(tx1, ty1), fminf(tz1, hi_c));
          const bool h = tn <= tf;   // absent children carry the empty box [+inf, -inf]
          hb[c] = h;
          k[c] = h ? tn : INFINITY;
          v[c] = u4c(rf, c);
          cnt += h ? 1 : 0;
        }
        if (ANYHIT) {   // any visit order gives the same answer: no sort
          uint32_t nxt = kDone;
#pragma unroll
          for (int c = 0; c < 4; ++c)
            if (hb[c]) {
              if (nxt != kDone) push(nxt);
              nxt = v[c];
            }
          cur = nxt == kDone ? pop() : nxt;
        } else {   // nearest child first, the others pushed far-first
#define RT_QCSWAP(a, b)                                       \
  if (k[b] < k[a]) {                                          \
    const float tk = k[a]; k[a] = k[b]; k[b] = tk;            \
    const uint32_t tv = v[a]; v[a] = v[b]; v[b] = tv;         \
  }
          RT_QCSWAP(0, 1) RT_QCSWAP(2, 3) RT_QCSWAP(0, 2) RT_QCSWAP(1, 3) RT_QCSWAP(1, 2)
#undef RT_QCSWAP
          if (cnt == 0) {
            cur = pop();
          } else {
            if (cnt > 3) push(v[3]);
            if (cnt > 2) push(v[2]);
            if (cnt > 1) push(v[1]);
            cur = v[0];
          }
        }
        if ((cur & kLeaf) && cur != kDone && pleaf == kDone) {   // first leaf: postpone, keep going
          pleaf = cur;
          cur = pop();
        }
        if ((wballot(pleaf == kDone) & wballot(cur != kDone)) == 0) break;   // every lane holds a leaf
      }
      if (pleaf == kDone && cur != kDone) {   // stopped at a leaf without postponing one
        pleaf = cur;
        cur = pop();
      }
      while (pleaf != kDone) {
        if (test_leaf(pleaf)) {   // occlusion ray blocked: finished
          occluded = true;
          cur = kDone;
          pleaf = kDone;
          break;
        }
        pleaf = kDone;
        if ((cur & kLeaf) && cur != kDone) {
          pleaf = cur;
          cur = pop();
        }
      }
    }
    if (overflow) guard_trip();
