// render_trip.h — one trip of render_kernel's loop (render_kernel.hip): the cast of one ray per active lane and the continuation.
//
// Not a header of its own: a fragment of render_kernel's body, included inside its `while` loop with CTR_TRIP_KIND defined as
// the kind of trip the copy is compiled for — TRIP_ANY, the generic body (what every lane casts for is per-lane state), or, in
// a phased build ("Phased builds" in render_kernel.hip), TRIP_RADIANCE and TRIP_SHADOW, one copy each behind a scalar branch.
// Included as text, not called as a lambda, so that the generic copy is compiled exactly as it was when it stood in the
// loop: a lambda is optimised once on its own before it is inlined, and every instantiation came out different.
// Everything it names — the lane's state, KArgs, the STK / PRK / CTR_MARK / TSTAMP macros — is render_kernel's.
    constexpr int K = CTR_TRIP_KIND;
    static_assert(K == TRIP_ANY || PHASED, "the kinds of trip: phased builds");
    constexpr int ctr_mark_base = K == TRIP_SHADOW ? 128 : 0;  // (shadows the file's: this copy's CTR_MARK ids)
    constexpr bool ctr_mark_fence = K != TRIP_ANY;             // (likewise: CTR_MARK in render_kernel.hip)
    (void)ctr_mark_base;
    (void)ctr_mark_fence;
    // the any-hit code of the cast (retiring lanes, the exits once all have retired): not in a radiance copy, which retires none
    constexpr bool AH = ANYHIT && K != TRIP_RADIANCE;
    // The shadow copy keeps no nearest hit.  All its continuation asks of the cast is `best < light_dist`, and that holds exactly
    // for the lanes that retired: a plane retires a lane iff its t0 < light_dist (and then best <= t0), one that does not leaves
    // best >= light_dist or untouched; the mesh writes `best` — to below light_dist — for retired lanes only, an any-hit cast
    // records no other mesh hit.  A dark lane made no cast and left alive_m at the trip head.  So the lanes of active_m that
    // are no longer in alive_m are the ones the generic body calls occluded, and best, bobj and btri are not written.
    constexpr bool NEAREST = K != TRIP_SHADOW;
    // the light of a shadow trip: per lane, or a scalar in a phased build's copies (0 in the radiance copy, whose phong prologue sets it)
    uint32_t li_k = K == TRIP_ANY ? li : (K == TRIP_SHADOW ? phase - 1u : 0u);
    asm volatile("" : "+s"(AK));
    typedef uint32_t u32x8 __attribute__((ext_vector_type(8)));
    const u32x8 hot = *(const CADDR u32x8 *)AK;  // KArgs' hot block
    const CADDR DPlanePair *const k_planes = (const CADDR DPlanePair *)(((uint64_t)hot[1] << 32) | hot[0]);
    const uint32_t k_plane_recs = hot[2], k_axis_recs = hot[3], k_n_oloop = ONE_MESH ? 0u : hot[4], k_mesh = hot[5];
    // (ONE_MESH: the top-level item is the leaf the scene head holds, whatever the argument says)
    const uint32_t k_tlas_root = ONE_MESH ? (BVH_LEAF_FLAG | CTR_TL_HEAD_FLAG) : hot[6];
    const bool k_has_mesh = (hot[7] & 1u) != 0u;
    // the scene head's axis triple, requested with the hot block whether it is filled or not (hot[7] says; constant addresses)
    typedef uint32_t u32x16 __attribute__((ext_vector_type(16)));
    typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
    const u32x16 hd_ax = *(const CADDR u32x16 *)&AK->head.ax[0][0];  // ax[0..5], ax_index[0..3]
    const u32x2 hd_ix = *(const CADDR u32x2 *)&AK->head.ax_index[4];
    const bool k_head_axis = (hot[7] & 2u) != 0u;
    const uint32_t hd_room_lights = ROOM_CODE ? AK->head.room_lights : 0u;  // "room-safe lanes" below: zero = no lane is
    TSTAMP(t_trip0);
    CTR_MARK(1);  // trip head: cast set-up
    typedef unsigned long long mask_t;
    const bool active = MSP_ACTIVE(msp);
    // (a phased copy: a constant — every lane that counts, the active ones, casts for the copy's kind)
    const bool shadow_cast = K == TRIP_ANY ? MSP_IS_SHADOW(msp) : K == TRIP_SHADOW;
    const mask_t active_m = BALLOT(active);
    const mask_t shadow_m = K == TRIP_ANY ? BALLOT(shadow_cast) : (K == TRIP_SHADOW ? active_m : 0ull);  // (taken here, straight from the compare: see alive_m below)
    n_casts += (unsigned long long)__builtin_popcountll(active_m);
    if (STATS) {
      st[0]++; st[5] += __builtin_popcountll(active_m);
      uint32_t kinds = 0;
      for (uint32_t d = 0; d < 16u; d++) {
        const mask_t r_m = BALLOT(MSP_IS_RADIANCE(msp) && (uint32_t)MSP_DEPTH(msp) == d);
        const mask_t s_m = BALLOT(shadow_cast && (uint32_t)MSP_DEPTH(msp) == d);
        kinds += (r_m != 0ull) + (s_m != 0ull);
        if (lane == 0) {
          if (r_m) { atomicAdd(&g_lane_stats[d], (unsigned long long)__builtin_popcountll(r_m)); atomicAdd(&g_lane_stats[32 + d], 1ull); }
          if (s_m) { atomicAdd(&g_lane_stats[16 + d], (unsigned long long)__builtin_popcountll(s_m)); atomicAdd(&g_lane_stats[48 + d], 1ull); }
        }
      }
      const mask_t img_m = BALLOT(in_image);
      if (lane == 0) {
        const uint32_t n_live = (uint32_t)__builtin_popcountll(active_m);
        atomicAdd(&g_lane_stats[64 + ((n_live - 1u) >> 3)], 1ull);
        atomicAdd(&g_lane_stats[72], 1ull);
        atomicAdd(&g_lane_stats[73], (unsigned long long)n_live);
        if (kinds > 1u) atomicAdd(&g_lane_stats[76], 1ull);
        if (first_trip) { atomicAdd(&g_lane_stats[74], 1ull); atomicAdd(&g_lane_stats[75], (unsigned long long)__builtin_popcountll(img_m)); }
      }
    }

    // =====================================================================
    // ray_cast (ray_cast.hpp:29-55): nearest hit of (ro, rd) over all objects
    // =====================================================================
    float best = INFINITY;
    int bobj = -1, btri = -1;
    // lanes still searching (any-hit mode retires occluded lanes), as a lane MASK: a per-lane bool that crosses blocks
    // is kept as a mask by the compiler anyway, and every BALLOT of it costs two vector instructions to get it back
    mask_t alive_m = active_m;
    // "dark lights": a dark lane needs no cast; a trip without any other lane skips set-up, planes and mesh in one go
    mask_t dark_m = 0ull;
    if constexpr (DARK_CODE && K != TRIP_RADIANCE) dark_m = BALLOT((msp & MSP_DARK) != 0u);  // (a radiance lane's msp has no such bit)
    if constexpr (DARK && K != TRIP_RADIANCE) alive_m &= ~dark_m;
    const bool all_dark = DARK && K != TRIP_RADIANCE && alive_m == 0ull;  // wave-uniform
    if (DARK_CODE && STATS && shadow_m != 0ull && (active_m & ~dark_m) == 0ull && lane == 0) atomicAdd(&g_lane_stats[91], 1ull);
    V3 rinv = mk(0, 0, 0);     // exact 1/dir (IEEE divisions), computed lazily: see the mesh branch
    bool have_rinv = false;    // wave-uniform
    V3 ria = mk(0, 0, 0);
    float ria_big = 0.f;
    float cmax = 0.f;
    if (k_has_mesh && !all_dark) {
      CTR_MARK(2);
      // 1-ulp reciprocals, clamped to +-1e30: an axis-parallel ray (d = 0 -> inf) then gives huge
      // FINITE slab distances with the right signs instead of inf - inf = NaN
      ria = mk(fminf(fmaxf(__builtin_amdgcn_rcpf(rd.x), -1e30f), 1e30f),
               fminf(fmaxf(__builtin_amdgcn_rcpf(rd.y), -1e30f), 1e30f),
               fminf(fmaxf(__builtin_amdgcn_rcpf(rd.z), -1e30f), 1e30f));
      ria_big = fmaxf(fmaxf(fabsf(ria.x), fabsf(ria.y)), fabsf(ria.z));
      cmax = fmaxf(fmaxf(fabsf(rd.x), fabsf(rd.y)), fabsf(rd.z));
    }

    TSTAMP(t_loop0);
    TACC(0, t_trip0, t_loop0);
    CTR_MARK(3);  // planes: set-up
    const bool anyhit_cast = ANYHIT && shadow_cast;
    const bool ign_now = IGNTR && first_trip;  // wave-uniform: this trip is the kernel.hpp:52 cast with ignore_transparent = true
    // Room-safe lanes: a shadow lane whose origin passed the room facts' predicate (MSP_ROOM) and whose light's bit is set in
    // room_lights casts a ray that no plane of the scene occludes (the facts are zero unless the head's triple holds every
    // plane).  When every live lane of the trip is one, the plane phase can only leave alive_m and best = INFINITY as they
    // are — a plane beyond the light would set best >= light_dist, which the continuation reads as "no occluder" as well —
    // and the whole wave branches over it.  A trip with any other live lane runs the phase for all of them, as before.
    bool skip_planes = false;  // wave-uniform
    if constexpr (ROOM_CODE && K == TRIP_SHADOW) {
      // (the shadow copy: the light's bit is a scalar test, and every live lane is a shadow lane)
      if (((hd_room_lights >> (li_k & 31u)) & 1u) != 0u) skip_planes = (alive_m & ~BALLOT((msp & MSP_ROOM) != 0u)) == 0ull;
    } else if constexpr (ROOM_CODE && K == TRIP_ANY) {
      if (hd_room_lights != 0u) {  // (the statistics builds run launches without room facts too)
        const mask_t safe_m = BALLOT((((hd_room_lights >> (li_k & 31u)) & (msp >> 29)) & 1u) != 0u);
        skip_planes = (alive_m & ~(shadow_m & safe_m)) == 0ull;
      }
      if (STATS && shadow_m != 0ull && lane == 0) {
        atomicAdd(&g_lane_stats[88], 1ull);
        atomicAdd(&g_lane_stats[89], skip_planes ? 1ull : 0ull);  // (no branch on the flag under the lane's: the compiler would thread it past the join)
      }
    }
    if constexpr (DARK) skip_planes = skip_planes || all_dark;
    // ---- planes: plane::intersect, default_schema.hpp:189-201, all in lane masks ----
    if (!skip_planes) {
      mask_t live_m = alive_m;
      // t0 = num/den is an IEEE division, and it is only worth doing where the quotient can matter.
      // Classification WITHOUT dividing (and without a reciprocal): with num' = num * sign(den) and
      // den' = |den| the quotient is num'/den', so
      //   t0 <= min_t for certain  if  num' < (min_t - 2^-21|min_t|) * den' - tiny
      //   t0 >  lim   for certain  if  num' > (lim   + 2^-21|lim|)   * den' + tiny
      // (2^-21 covers the roundings of the two products and of the division itself; tiny = 1e-37 covers
      // products that underflow; a NaN compares false = "needed"; den = 0 gives num' <> -+tiny, and the
      // quotient is then infinite or NaN, which plane::intersect rejects as not finite.)
      // lim = the light for a deciding shadow ray, else the nearest hit so far.
      const float mt_lo = min_t - fabsf(min_t) * 0x1p-21f;
      float lhv = anyhit_cast ? light_dist : best;
      lhv = lhv + fabsf(lhv) * 0x1p-21f;
      float tiny = 1e-37f;
      asm volatile("" : "+v"(tiny));  // keep it in a VGPR: a literal operand would halve the FMA's issue rate
      // one plane against the lanes in need_m; returns false when every lane has retired (any-hit)
      auto plane_exact = [&](uint32_t pidx, float num, float den, mask_t need_m, auto site) -> bool {
        CTR_MARK(110 + decltype(site)::value);  // a plane some lane needs the quotient of
        bool retire = false;
        if (INVB(need_m)) {
          const float t0 = num / den;
          // isfinite && min_t <= t0 (plane) && t0 > min_t (ray_cast.hpp:43)  ==  finite && t0 > min_t
          if (__builtin_isfinite(t0) && t0 > min_t) {
            // ray_cast.hpp:43: strict <, first object in scene order wins ties
            if (NEAREST && (t0 < best || (t0 == best && (int)pidx < bobj))) {
              best = t0; bobj = (int)pidx; btri = -1;
              if (!anyhit_cast) lhv = t0 + fabsf(t0) * 0x1p-21f;
            }
            if (anyhit_cast && t0 < light_dist) retire = true;
          }
        }
        if (AH) {
          live_m &= ~BALLOT(retire);
          if (live_m == 0ull) return false;
        }
        return true;
      };
      auto plane_test = [&](uint32_t pidx, float num, float den, auto site) -> bool {  // (site: which inlined copy, for CTR_MARK)
        CTR_MARK(100 + decltype(site)::value);  // one plane's classification
        const float nump = __uint_as_float(__float_as_uint(num) ^ (__float_as_uint(den) & 0x80000000u));
        const float denp = fabsf(den);
        const mask_t need_m = live_m & ~(FCMP(nump, __builtin_fmaf(mt_lo, denp, -tiny), FC_OLT) |
                                         FCMP(nump, __builtin_fmaf(lhv, denp, tiny), FC_OGT));
        if (need_m == 0ull) return true;
        return plane_exact(pidx, num, den, need_m, site);
      };
      // Two planes per 64-byte record with interleaved coordinates: the numerators (point - origin).normal
      // and denominators dir.normal of BOTH planes come from packed f32 multiplies and adds — the
      // reference's operations in the reference's order (vector.hpp dot: x*x' + y*y' + z*z' left to
      // right), two at a time.  Three records (six planes) are fetched and evaluated per trip, so a box
      // room costs ONE scalar-load round trip per cast instead of three dependent ones.
      const float2_ rox = {ro.x, ro.x}, roy = {ro.y, ro.y}, roz = {ro.z, ro.z};
      const float2_ rdx = {rd.x, rd.x}, rdy = {rd.y, rd.y}, rdz = {rd.z, rd.z};
      auto num_den = [&](const CADDR DPlanePair &P, float2_ &num, float2_ &den) {
        const float2_ nx = ldpair(P.n[0]), ny = ldpair(P.n[1]), nz = ldpair(P.n[2]);
        const float2_ dx = ldpair(P.p[0]) - rox, dy = ldpair(P.p[1]) - roy, dz = ldpair(P.p[2]) - roz;
        num = (dx * nx + dy * ny) + dz * nz;
        den = (rdx * nx + rdy * ny) + rdz * nz;
      };
      // Axis-aligned planes (the first n_axis_recs records, whole triples: two planes normal to x, two to y, two to z):
      // the reference's  dx*nx + dy*ny + dz*nz  with two of the normal's components zero is the one product that is
      // not multiplied by zero whenever that product is not zero itself (x + (+-0) = x), and a zero of either sign
      // otherwise.  A zero numerator gives t0 = +-0 or NaN and a zero denominator an infinite or NaN t0 — a miss
      // whatever the zero's sign as long as min_t > 0; so with fudge > 0 and every live lane's origin and direction
      // finite (0 x inf would be NaN in the reference) three packed instructions per record stand for thirteen.
      const uint32_t n_recs = k_plane_recs, n_axis = k_axis_recs;
      bool axis_fast = false;  // wave-uniform
      if (n_axis != 0u && A.fudge >= 1e-30f) {
        CTR_MARK(4);
        // NaN iff some component is not finite (or the sum overflows: then the general code, which is always right)
        // (the origin's components times 4: beyond 8.5e37 the product is inf, so the differences point - origin of the
        //  planes — whose points the upload bounds by 1e37 — cannot overflow either: an infinite difference times the normal's
        //  zero is a NaN in the reference, a miss, where the one-product form would report a hit)
        const float chk = __builtin_fmaf(ro.x, 4.0f, __builtin_fmaf(ro.y, 4.0f, __builtin_fmaf(ro.z, 4.0f, (rd.x + rd.y) + rd.z))) * 0.0f;
        axis_fast = (alive_m & ~FCMP(chk, 0.0f, FC_OEQ)) == 0ull;
      }
      // the six slots of a triple, in scene order; false: every lane has retired (any-hit)
      // (a slot without a plane: CTR_PLANE_PAD; IGNTR: tr.. != 0 = a plane whose material is transparent does not exist for this cast)
      auto triple_tests = [&](uint32_t i00, uint32_t i01, uint32_t i10, uint32_t i11, uint32_t i20, uint32_t i21, float2_ num0, float2_ den0,
                              float2_ num1, float2_ den1, float2_ num2, float2_ den2, uint32_t tr00, uint32_t tr01, uint32_t tr10,
                              uint32_t tr11, uint32_t tr20, uint32_t tr21) -> bool {
        if (i00 != CTR_PLANE_PAD && !(IGNTR && ign_now && tr00)) { if (!plane_test(i00, num0.x, den0.x, SITE(0))) return false; }
        if (i01 != CTR_PLANE_PAD && !(IGNTR && ign_now && tr01)) { if (!plane_test(i01, num0.y, den0.y, SITE(1))) return false; }
        if (i10 != CTR_PLANE_PAD && !(IGNTR && ign_now && tr10)) { if (!plane_test(i10, num1.x, den1.x, SITE(2))) return false; }
        if (i11 != CTR_PLANE_PAD && !(IGNTR && ign_now && tr11)) { if (!plane_test(i11, num1.y, den1.y, SITE(3))) return false; }
        if (i20 != CTR_PLANE_PAD && !(IGNTR && ign_now && tr20)) { if (!plane_test(i20, num2.x, den2.x, SITE(4))) return false; }
        if (i21 != CTR_PLANE_PAD && !(IGNTR && ign_now && tr21)) { if (!plane_test(i21, num2.y, den2.y, SITE(5))) return false; }
        return true;
      };
      uint32_t p = 0;
      bool more = true;  // wave-uniform
      // the scene head's axis triple first, as code of its own: inside the loop its values would be loop-invariant inputs of a
      // merge with the pointer path's (register copies per cast, and 13 VGPRs more in the builds without a mesh walk)
      if (k_head_axis && axis_fast) {
        CTR_MARK(59);  // the axis triple of the scene head: the same twelve floats and six indices, already here
        auto pr = [&](int k) -> float2_ { const float2_ v = {__uint_as_float(hd_ax[2 * k]), __uint_as_float(hd_ax[2 * k + 1])}; return v; };
        const float2_ nx = pr(1), ny = pr(3), nz = pr(5);
        uint32_t tr00 = 0u, tr01 = 0u, tr10 = 0u, tr11 = 0u, tr20 = 0u, tr21 = 0u;
        if (IGNTR && ign_now) {
          tr00 = AK->head.ax_transparent[0]; tr01 = AK->head.ax_transparent[1]; tr10 = AK->head.ax_transparent[2];
          tr11 = AK->head.ax_transparent[3]; tr20 = AK->head.ax_transparent[4]; tr21 = AK->head.ax_transparent[5];
        }
        p = 3u;
        more = triple_tests(hd_ax[12], hd_ax[13], hd_ax[14], hd_ax[15], hd_ix[0], hd_ix[1], (pr(0) - rox) * nx, rdx * nx, (pr(2) - roy) * ny,
                            rdy * ny, (pr(4) - roz) * nz, rdz * nz, tr00, tr01, tr10, tr11, tr20, tr21);
      }
      while (more && p < n_recs) {
        if (n_recs - p >= 3u) {
          float2_ num0, den0, num1, den1, num2, den2;
          uint32_t i00, i01, i10, i11, i20, i21;
          uint32_t tr00 = 0u, tr01 = 0u, tr10 = 0u, tr11 = 0u, tr20 = 0u, tr21 = 0u;  // IGNTR: the slots' transparency words
          const CADDR DPlanePair &P0 = k_planes[p], &P1 = k_planes[p + 1], &P2 = k_planes[p + 2];
          // (indices first: their loads then travel with the coordinates', one round trip for the triple)
          i00 = P0.index[0]; i01 = P0.index[1]; i10 = P1.index[0]; i11 = P1.index[1]; i20 = P2.index[0]; i21 = P2.index[1];
          if (IGNTR && ign_now) {
            tr00 = P0.transparent[0]; tr01 = P0.transparent[1]; tr10 = P1.transparent[0];
            tr11 = P1.transparent[1]; tr20 = P2.transparent[0]; tr21 = P2.transparent[1];
          }
          if (p < n_axis && axis_fast) {
            CTR_MARK(5);  // an axis triple
            const float2_ nx = ldpair(P0.n[0]), ny = ldpair(P1.n[1]), nz = ldpair(P2.n[2]);
            num0 = (ldpair(P0.p[0]) - rox) * nx; den0 = rdx * nx;
            num1 = (ldpair(P1.p[1]) - roy) * ny; den1 = rdy * ny;
            num2 = (ldpair(P2.p[2]) - roz) * nz; den2 = rdz * nz;
          } else {
            CTR_MARK(6);  // three plane records
            num_den(P0, num0, den0);
            num_den(P1, num1, den1);
            num_den(P2, num2, den2);
          }
          p += 3;
          if (!triple_tests(i00, i01, i10, i11, i20, i21, num0, den0, num1, den1, num2, den2, tr00, tr01, tr10, tr11, tr20, tr21)) break;
        } else {
          const CADDR DPlanePair &P0 = k_planes[p];
          CTR_MARK(7);  // one plane record
          float2_ num0, den0;
          num_den(P0, num0, den0);
          const uint32_t i00 = P0.index[0], i01 = P0.index[1];
          p += 1;
          if (!(IGNTR && ign_now && P0.transparent[0])) { if (!plane_test(i00, num0.x, den0.x, SITE(6))) break; }
          if (i01 != CTR_PLANE_PAD && !(IGNTR && ign_now && P0.transparent[1])) {
            if (!plane_test(i01, num0.y, den0.y, SITE(7))) break;
          }
        }
      }
      if (AH) alive_m = live_m;
    }
    TSTAMP(t_planes1);
    TACC(1, t_loop0, t_planes1);
    CTR_MARK(8);  // after the planes
    // ---- spheres and stand-alone triangles, scene order ----
    // sphere::intersect normalises the direction first (default_schema.hpp:227): once per cast (at the
    // first sphere the cast meets), not once per sphere
    V3 sph_d = mk(0, 0, 0);
    float sph_dd = 0.f;
    bool sph_have = false;  // wave-uniform
    for (uint32_t oi = 0; oi < k_n_oloop; ++oi) {
      if (ANYHIT) {
        if (alive_m == 0ull) break;
      }
      const CADDR DObj &O = AK->oloop[oi];
      const uint32_t i = O.index;
      const uint32_t type = O.type;
      if (IGNTR && ign_now && __float_as_uint(O.f[7]) != 0u) continue;  // ray_cast.hpp:40
      CTR_MARK(9);  // a sphere or stand-alone triangle
      bool ok = false;
      float cand = INFINITY;
      int ctri = -1;
      if (type == CTR_OBJ_SPHERE) {
        // ---- sphere::intersect, default_schema.hpp:226-251 ----
        if (!sph_have) {
          CTR_MARK(10);
          float sx_ = rd.x, sy_ = rd.y, sz_ = rd.z;
          PIN3(sx_, sy_, sz_);  // keeps the normalisation out of scenes without spheres (no hoisting)
          sph_d = vnormalized(mk(sx_, sy_, sz_));
          sph_dd = vdot(sph_d, sph_d);
          sph_have = true;
        }
        const V3 d = sph_d, c = mk(O.f[0], O.f[1], O.f[2]);
        const float R = O.f[3];
        const V3 ec = vsub(ro, c);
        const float dec = -vdot(d, ec);
        const float dd = sph_dd;
        const float sub = dec * dec - dd * (vdot(ec, ec) - R * R);
        // sub < 0: sqrt gives NaN, both roots are NaN, the sphere is missed (that IS how the reference
        // signals a miss) — so the square root and the two divisions run only if some live lane has
        // sub >= 0 or NaN (the exact reference value of sub decides, no margin involved)
        if ((alive_m & ~FCMP(sub, 0.0f, FC_OLT)) != 0ull) {
          CTR_MARK(11);  // sphere roots
          const float sq = sqrtf(sub);
          const float t0 = (dec - sq) / dd, t1 = (dec + sq) / dd;
          const bool t0v = __builtin_isfinite(t0) && min_t <= t0, t1v = __builtin_isfinite(t1) && min_t <= t1;
          ok = t0v || t1v;
          cand = (t0v && t1v) ? smin(t0, t1) : (t0v ? t0 : t1);
        }
      } else {
        // ---- stand-alone triangle, default_schema.hpp:57-78 ----
        const CADDR DTri &T = A.tris[O.tri_begin];
        const V3 a = mk(T.ab[0][0], T.ab[1][0], T.ab[2][0]), b = mk(T.ab[0][1], T.ab[1][1], T.ab[2][1]);
        const V3 d = mk(T.px - ro.x, T.py - ro.y, T.pz - ro.z);
        const float alpha = det3(a, b, rd);
        const float beta = det3(d, b, rd) / alpha;
        const float gamma = det3(a, d, rd) / alpha;
        const float t0 = det3(a, b, d) / alpha;
        ok = beta >= 0 && gamma >= 0 && beta + gamma <= 1 && __builtin_isfinite(t0) && min_t <= t0;
        cand = t0;
        ctri = (int)O.tri_begin;
      }
      CTR_MARK(12);  // object loop: candidate merge
      // ray_cast.hpp:43 — strict <, first object in scene order wins ties
      if (INVB(alive_m) && ok && cand > min_t && (cand < best || (cand == best && (int)i < bobj))) {
        best = cand;
        bobj = (int)i;
        btri = ctri;
      }
      if (ANYHIT) alive_m &= ~BALLOT(shadow_cast && ok && cand > min_t && cand < light_dist);
    }
    // ---- meshes, reached through a top-level BVH over their boxes (bvh.h layout, one mesh per leaf)
    //      so that a cast only looks at meshes some lane's ray can touch.  Visiting order does not
    //      matter: the winner is the lexicographic minimum of (t, scene index). ----
    TSTAMP(t_oloop1);
    TACC(2, t_planes1, t_oloop1);
    CTR_MARK(13);
    const mask_t st_shadow_entry = (STATS && ANYHIT) ? (alive_m & shadow_m) : 0ull;
    const mask_t st_recv_mesh = STATS ? BALLOT(recv_mesh) : 0ull;
    if (ONE_MESH || k_mesh != 0u) {
      uint32_t t_pend = k_tlas_root;             // next top-level item: inner node or mesh leaf
      uint32_t t_stack_v = 0, t_sp = 0;        // wave-uniform stack in the lanes of one VGPR
      // ---- mesh::bound_intersects, default_schema.hpp:99-114, for the lanes in `lanes` -> the lanes that pass ----
      // The reference's slab test needs three IEEE divisions (1/dir) per ray.  With 1-ulp
      // reciprocals every t is within 3 ulp of the exact one and tmin/tmax are 1-Lipschitz in
      // the t's, so lanes whose tmin/tmax differ by more than dl = 2^-20 * max|t| are decided
      // without them; only borderline lanes (or NaN/inf: axis-parallel rays) take the exact path.
      // (site 0: a mesh of the top-level walk; site 1: the merged walk's verification)
      auto box_test = [&](const CADDR DObj &R, mask_t lanes, auto site) -> mask_t {
        constexpr int MK = decltype(site)::value ? 83 : 18;
        (void)MK;
        const float a1x = (R.f[0] - ro.x) * ria.x, a2x = (R.f[3] - ro.x) * ria.x;
        const float a1y = (R.f[1] - ro.y) * ria.y, a2y = (R.f[4] - ro.y) * ria.y;
        const float a1z = (R.f[2] - ro.z) * ria.z, a2z = (R.f[5] - ro.z) * ria.z;
        const float lo_a = fmaxf(fmaxf(fmaxf(fminf(a1x, a2x), fminf(a1y, a2y)), fminf(a1z, a2z)), 0.0f);
        const float hi_a = fminf(fminf(fmaxf(a1x, a2x), fmaxf(a1y, a2y)), fmaxf(a1z, a2z));
        const float tabs = fmaxf(fmaxf(fmaxf(fabsf(a1x), fabsf(a2x)), fmaxf(fabsf(a1y), fabsf(a2y))),
                                 fmaxf(fabsf(a1z), fabsf(a2z)));
        const float dl = tabs * 0x1p-20f;
        const mask_t def_hit = FCMP(lo_a + dl, hi_a, FC_OLT);
        const mask_t def_miss = FCMP(lo_a - dl, hi_a, FC_OGT);
        // axis-parallel rays always take the exact path: the reference's inf/NaN min/max semantics
        // (0 x inf when the origin sits exactly on a box face) are not what finite arithmetic gives
        const mask_t border = lanes & (~(def_hit | def_miss) | FCMP(ria_big, 1e29f, FC_OGE));
        mask_t pass_m = lanes & def_hit & ~border;
        if (border != 0ull) {
          CTR_MARK(MK);  // exact AABB for borderline lanes
          if (!have_rinv) {  // wave-uniform: the exact reciprocals are computed at most once per cast
            CTR_MARK(MK + 1);
            float ox = rd.x, oy = rd.y, oz = rd.z;
            PIN3(ox, oy, oz);  // keeps the three IEEE divisions in this rarely-taken branch (no hoisting)
            rinv = mk(1.0f / ox, 1.0f / oy, 1.0f / oz);  // default_schema.hpp:103
            have_rinv = true;
          }
          CTR_MARK(MK + 2);
          float tmin = 0.0f, tmax = INFINITY;
          float t1 = (R.f[0] - ro.x) * rinv.x, t2 = (R.f[3] - ro.x) * rinv.x;
          tmin = smin(smax(t1, tmin), smax(t2, tmin));
          tmax = smax(smin(t1, tmax), smin(t2, tmax));
          t1 = (R.f[1] - ro.y) * rinv.y; t2 = (R.f[4] - ro.y) * rinv.y;
          tmin = smin(smax(t1, tmin), smax(t2, tmin));
          tmax = smax(smin(t1, tmax), smin(t2, tmax));
          t1 = (R.f[2] - ro.z) * rinv.z; t2 = (R.f[5] - ro.z) * rinv.z;
          tmin = smin(smax(t1, tmin), smax(t2, tmin));
          tmax = smax(smin(t1, tmax), smin(t2, tmax));
          pass_m |= border & FCMP(tmin, tmax, FC_OLE);
        }
        return pass_m;
      };
      for (;;) {
        TSTAMP(t_tl0);
        if (AH) {
          if (alive_m == 0ull) break;
        }
        // (nothing left: TL_NONE has no leaf flag, and without this test a scene's LAST mesh was followed by one more
        //  descent set-up — ~30 vector instructions per cast for nothing, found by the execution profile, scripts/dynamic_mix.py)
        if (t_pend == TL_NONE) break;
        // descend the top-level tree to the next mesh leaf
        if (!ONE_MESH && !(t_pend & BVH_LEAF_FLAG)) {
          CTR_MARK(14);  // top-level descent set-up
          const mask_t lv_m = alive_m;
          const float t_lim = anyhit_cast ? light_dist : best;
          // conservative box test constants, as in the per-mesh walk below (world-space margin
          // 2^-14 x G); recomputed per descent so that nothing stays live across the mesh code
          const float gx = fmaxf(fabsf(AK->tl_mn[0] - ro.x), fabsf(AK->tl_mx[0] - ro.x));
          const float gy = fmaxf(fabsf(AK->tl_mn[1] - ro.y), fabsf(AK->tl_mx[1] - ro.y));
          const float gz = fmaxf(fabsf(AK->tl_mn[2] - ro.z), fabsf(AK->tl_mx[2] - ro.z));
          // (+ 2^-21 x the origin's largest |coordinate|: what rounding ro + mw and its product takes back, see the per-mesh walk)
          const float mw = __builtin_fmaf(fmaxf(fmaxf(fabsf(ro.x), fabsf(ro.y)), fabsf(ro.z)), 0x1p-21f, fmaxf(fmaxf(gx, gy), gz) * 0x1p-14f);
          const V3 t_ka = mk((ro.x + mw) * ria.x, (ro.y + mw) * ria.y, (ro.z + mw) * ria.z);
          const V3 t_kb = mk((ro.x - mw) * ria.x, (ro.y - mw) * ria.y, (ro.z - mw) * ria.z);
          const uint32_t t_lead = (uint32_t)__builtin_ctzll(lv_m);
          const uint32_t t_neg =
              (((uint32_t)__builtin_amdgcn_readlane(__float_as_uint(rd.x), t_lead) >> 31) |
               (((uint32_t)__builtin_amdgcn_readlane(__float_as_uint(rd.y), t_lead) >> 31) << 1) |
               (((uint32_t)__builtin_amdgcn_readlane(__float_as_uint(rd.z), t_lead) >> 31) << 2)) ^
              ((ANYHIT && ((shadow_m >> t_lead) & 1ull) != 0ull) ? 7u : 0u);
          while (t_pend != TL_NONE && !(t_pend & BVH_LEAF_FLAG)) {
            const CADDR DNode &N = A.nodes[AK->tlas_begin + t_pend];
            CTR_MARK(15);  // top-level node
            auto t_hits = [&](int c) -> mask_t {
              const float t1x = __builtin_fmaf(N.mn[0][c], ria.x, -t_ka.x), t2x = __builtin_fmaf(N.mx[0][c], ria.x, -t_kb.x);
              const float t1y = __builtin_fmaf(N.mn[1][c], ria.y, -t_ka.y), t2y = __builtin_fmaf(N.mx[1][c], ria.y, -t_kb.y);
              const float t1z = __builtin_fmaf(N.mn[2][c], ria.z, -t_ka.z), t2z = __builtin_fmaf(N.mx[2][c], ria.z, -t_kb.z);
              // as in the per-mesh walk: a lane takes the child unless max(entry, min_t) > min(exit, limit) for certain
              // (v_min / v_max drop a NaN operand: that axis' constraint drops out; one compare instead of three)
              const float lo = slab_lo4(t1x, t2x, t1y, t2y, t1z, t2z, min_t);
              const float hi = slab_hi4(t1x, t2x, t1y, t2y, t1z, t2z, t_lim);
              return lv_m & ~FCMP(lo, hi, FC_OGT);
            };
            // visiting order as in the per-mesh walk (speed only): along the lead ray for nearest-hit casts, against
            // it for any-hit shadow casts
            const bool t_rev = ((t_neg >> N.axis) & 1u) != 0u;
            // (both children are VALUES here, fetched with the boxes: the compiler otherwise selects the ADDRESS and loads
            //  the one it wants after the test — a second dependent round trip per node)
            uint32_t n_left = N.left, n_right = N.right;
            asm volatile("" : "+s"(n_left), "+s"(n_right));
            // The two hit masks stay lane masks and the four cases are told apart by comparing them with zero (round 4: the
            // earlier form — hit counts folded into two bits of an integer, swapped by `t_rev`, then a chain of four equality
            // tests — cost 47 scalar instructions and 15 branches per node; this one about half of that).
            const mask_t tm0 = t_hits(0), tm1 = t_hits(1);
            const mask_t mN = t_rev ? tm1 : tm0, mF = t_rev ? tm0 : tm1;   // the nearer / the farther child along the lead ray
            const uint32_t dN = t_rev ? n_right : n_left, dF = t_rev ? n_left : n_right;
            if (mN != 0ull) {
              if (mF != 0ull) {
                t_stack_v = ctr_writelane(__builtin_amdgcn_readfirstlane(dF), __builtin_amdgcn_readfirstlane(t_sp), t_stack_v);
                t_sp++;
              }
              t_pend = dN;
            } else if (mF != 0ull) {
              t_pend = dF;
            } else if (t_sp != 0u) {
              t_sp--;
              t_pend = (uint32_t)__builtin_amdgcn_readlane((int)t_stack_v, (int)t_sp);
            } else {
              t_pend = TL_NONE;
            }
          }
        }
        CTR_MARK(16);
        if (t_pend == TL_NONE) break;
        // (the leaf the scene head holds: its record lies at a constant address of the argument block — no `meshes` to fetch first)
        const CADDR DObj *o_rec;
        if (ONE_MESH || (t_pend & CTR_TL_HEAD_FLAG)) o_rec = &AK->head.mesh;
        else o_rec = &AK->meshes[t_pend & 0xFFFFFFu];
        const CADDR DObj &O = *o_rec;
        // advance first, so that `continue` below moves on to the next mesh
        // (ONE_MESH: there is none — no stack, and the loop folds to its one pass)
        if constexpr (ONE_MESH) {
          t_pend = TL_NONE;
        } else if (t_sp != 0u) {
          t_sp--;
          t_pend = (uint32_t)__builtin_amdgcn_readlane((int)t_stack_v, (int)t_sp);
        } else {
          t_pend = TL_NONE;
        }
        if (IGNTR && ign_now && __float_as_uint(O.f[7]) != 0u) continue;  // ray_cast.hpp:40: a mesh with a transparent material
        CTR_MARK(17);  // a mesh: AABB test
        const uint32_t i = O.index;
        // (the whole record in one round trip: what the walk needs is requested with the box, not after its test)
        const uint32_t o_tri_begin = O.tri_begin, o_tri_count = O.tri_count, o_node_begin = O.node_begin, o_bvh_root = O.bvh_root;
        const bool merged = MERGE && i == 0xFFFFFFFFu;  // wave-uniform: the pseudo mesh (CTR_OBJ_MERGED) is no object of the scene
        bool ok = false;
        float cand = INFINITY;
        int ctri = -1;
        int obj_lane = (int)i;
        {
          // Everything in this branch works on 64-bit lane masks (v_cmp results kept in SGPRs and
          // combined on the scalar unit) instead of per-lane booleans.
          const mask_t live_m = alive_m;
          // One tree over the triangles of ALL meshes stands behind the pseudo mesh (scene_flatten.h Merged): every
          // live lane enters it; the AABB test of the mesh a lane's triangle belongs to is made after the walk, for the
          // lanes the walk decided something for ("merged walk" below).  A real mesh: the reference's test first.
          mask_t bb_m;
          if (merged) {
            // (a ray with a NaN or infinite component never meets a triangle — alpha or the numerators of
            //  default_schema.hpp:59-62 are then not finite and `isfinite(t0)` or a barycentric test fails — but the walk's
            //  box tests let a NaN through by design, so such a lane would drag its wave through the WHOLE tree on every
            //  cast; a mesh's own AABB test stops it in the two-level walk.  Reflections off zero-area triangles make
            //  them: C3-deep ran 15x longer for a handful of such waves)
            const float fin_chk = ((ro.x * 0.0f + ro.y * 0.0f) + (ro.z * 0.0f + rd.x * 0.0f)) + (rd.y * 0.0f + rd.z * 0.0f);
            // ... and a ray that misses the box of ALL meshes for certain misses every mesh's box for certain (each lies inside:
            // its slab distances lie between the union's, so its entry / exit gap is at least the union's and the rounding
            // of the reference's own test, 3 ulp of distances no larger than the union's, is far below dl).  That gate is
            // what keeps a ray whose ORIGIN is far away out of the walk — one that left the room through its open side and
            // met a wall plane a million units off: the box tests' world-space margin (2^-14 x the distance to the meshes)
            // then exceeds the room, every box test passes and the wave walks the whole tree on each such cast.
            const float a1x = (O.f[0] - ro.x) * ria.x, a2x = (O.f[3] - ro.x) * ria.x;
            const float a1y = (O.f[1] - ro.y) * ria.y, a2y = (O.f[4] - ro.y) * ria.y;
            const float a1z = (O.f[2] - ro.z) * ria.z, a2z = (O.f[5] - ro.z) * ria.z;
            const float lo_a = fmaxf(fmaxf(fmaxf(fminf(a1x, a2x), fminf(a1y, a2y)), fminf(a1z, a2z)), 0.0f);
            const float hi_a = fminf(fminf(fmaxf(a1x, a2x), fmaxf(a1y, a2y)), fmaxf(a1z, a2z));
            const float tabs = fmaxf(fmaxf(fmaxf(fabsf(a1x), fabsf(a2x)), fmaxf(fabsf(a1y), fabsf(a2y))),
                                     fmaxf(fabsf(a1z), fabsf(a2z)));
            const mask_t def_miss = FCMP(lo_a - tabs * 0x1p-20f, hi_a, FC_OGT) & ~FCMP(ria_big, 1e29f, FC_OGE);
            bb_m = live_m & FCMP(fin_chk, 0.0f, FC_OEQ) & ~def_miss;
            // A lane of those that starts more than 16 box sizes away (and still aims at the box: a shadow ray from such a hit
            // point to a light in the room) gets box margins of 0.1 % of the box and more, growing with its distance: the
            // cast goes through the two-level walk instead, where the meshes' own AABB tests — exact at any distance —
            // stand before the walk.
            const float g_far = fmaxf(fmaxf(fmaxf(fabsf(O.f[0] - ro.x), fabsf(O.f[3] - ro.x)), fmaxf(fabsf(O.f[1] - ro.y), fabsf(O.f[4] - ro.y))),
                                      fmaxf(fabsf(O.f[2] - ro.z), fabsf(O.f[5] - ro.z)));
            const float ext16 = 16.0f * fmaxf(fmaxf(O.f[3] - O.f[0], O.f[4] - O.f[1]), O.f[5] - O.f[2]);
            if ((bb_m & FCMP(g_far, ext16, FC_OGT)) != 0ull) {
              CTR_MARK(88);
              if (STATS && lane == 0) atomicAdd(&g_lane_stats[77], 1ull);
              t_pend = AK->tlas_root2;
              t_sp = 0u;
              continue;
            }
          } else bb_m = box_test(O, live_m, SITE(0));
          TSTAMP(t_bb);
          TACC(3, t_tl0, t_bb);
          CTR_MARK(21);
          if (bb_m == 0ull) continue;  // no lane of this wave needs the mesh
          CTR_MARK(22);  // mesh entered: walk set-up
          const uint32_t beg = o_tri_begin, cnt = o_tri_count;
          if (COUNT) n_aabb_tris += INVB(bb_m) ? (unsigned long long)cnt : 0ull;
          if (STATS) st[4]++;
          if (DARK_CODE && STATS && dark_m != 0ull && lane == 0) atomicAdd(&g_lane_stats[92], 1ull);
          uint32_t pl_nodes = 0, pl_tris = 0;  // STATS: this lane's own share of the mesh entry's node visits / triangle tests
          // ---- mesh::intersect, default_schema.hpp:125-144: smallest valid t, FIRST triangle in
          //      file order on ties (strict < over file order)  ==  lexicographic min of (t, orig) ----
          float mt = INFINITY;
          uint32_t morig = 0xFFFFFFFFu;
          const bool anyhit_now = ANYHIT && shadow_cast;
          const mask_t anyhit_m = ANYHIT ? shadow_m : 0ull;
          const bool t_filter = A.fudge >= 1e-30f;  // then min_t > 0 in every cast (wave-uniform)
          // no triangle/node beyond `lim` can matter: the light for a deciding shadow ray, else the
          // nearest hit so far (other objects, then this mesh)
          float lim = anyhit_now ? light_dist : best;

          const float2_ ro_xy = {ro.x, ro.y};
          // one triangle against the lanes in `lanes_m` (wave-uniform T: SGPR operands)
          auto tri_test = [&](const TriR &T, uint32_t tri_index, mask_t lanes_m) {
            CTR_MARK(23);  // triangle: prefilter stage 1
            mask_t c_m = lanes_m;
            if (STATS) { st[2]++; st[7] += __builtin_popcountll(lanes_m); pl_tris += INVB(lanes_m) ? 1u : 0u; }
            // d = p2 - start (default_schema.hpp:58): x and y in one packed subtraction (same IEEE result)
            const float2_ dxy = T.pxy - ro_xy;
            const float dx = dxy.x, dy = dxy.y, dz = T.pz - ro.z;
            uint32_t sgn = 0;
            float sA1 = 0.f, sA2 = 0.f, absa = 0.f, dmax = 0.f, E = 0.f;
            mask_t flat_m = 0ull;
            if (PREFILTER) {
              // Conservative reject test.  Same quantities as the exact test
              // (alpha = det[a b c], A1 = det[d b c], A2 = det[a d c]) evaluated with FMAs
              // as triple products; every comparison carries a slack E that bounds both this
              // evaluation's and the reference's rounding, and a
              // NaN anywhere makes the lane a candidate.
              const float alpha = __builtin_fmaf(rd.x, T.nx, __builtin_fmaf(rd.y, T.ny, rd.z * T.nz));
              float2_ q_xy, q_z;
              q_xy.x = __builtin_fmaf(dy, rd.z, -(dz * rd.y));
              q_xy.y = __builtin_fmaf(dz, rd.x, -(dx * rd.z));
              q_z.x = __builtin_fmaf(dx, rd.y, -(dy * rd.x));
              q_z.y = 0.0f;
              // (a.q, b.q) = (A2, -A1) together: the (a, b) pairs of the record times q, three packed instructions
              float2_ m;
              PKMULB(m, T.ab0, q_xy, 0);
              PKFMAB(m, T.ab1, q_xy, 1, m);
              PKFMAB(m, T.ab2, q_z, 0, m);
              // (s A2, s A1) with s = sign(alpha): multiply by (s, -s), exact
              sgn = __float_as_uint(alpha) & 0x80000000u;
              float2_ s1;
              s1.x = __uint_as_float(sgn | 0x3f800000u);
              s1.y = 0.0f;
              float2_ sm;
              asm("v_pk_mul_f32 %0, %1, %2 op_sel_hi:[1,0] neg_hi:[0,1]" : "=v"(sm) : "v"(m), "v"(s1));
              sA2 = sm.x;
              sA1 = sm.y;
              absa = fabsf(alpha);
              dmax = fmaxf(fmaxf(fabsf(dx), fabsf(dy)), fabsf(dz));
              // kappa * max(dmax,emax) * emax * cmax; both operands are >= 0, so the maximum is taken on the
              // bit patterns (fmaxf would first canonicalise the loaded ke2: one more VALU op per triangle)
              const uint32_t e_a = __float_as_uint(dmax * T.ke), e_b = __float_as_uint(T.ke2);
              E = __uint_as_float(e_a > e_b ? e_a : e_b) * cmax;
              // reject if  s A1 < -E  or  s A2 < -E  or  s A1 + s A2 > |alpha| + E:  ONE comparison of the smallest
              // of the three slacks (v_min3 drops a NaN operand: a lane is rejected only on a definite violation)
              float slack;
              {
                const float third = absa - (sA1 + sA2);
                asm("v_min3_f32 %0, %1, %2, %3" : "=v"(slack) : "v"(sA1), "v"(sA2), "v"(third));
              }
              const mask_t rej = FCMP(slack, -E, FC_OLT);
              flat_m = FCMP(absa, E, FC_OLE);  // alpha within rounding of 0: always a candidate
              c_m = lanes_m & (~rej | flat_m);
              if (c_m == 0ull) return;
              if (t_filter) {
                CTR_MARK(24);  // prefilter stage 2
                // Second stage, only when some lane survived the first: the ray parameter.
                // t0 = A0/alpha with A0 = det[a b d] = d.(a x b); E0 bounds the rounding of A0 the
                // way E does for the other three.  A lane whose t0 is certainly below min_t or
                // certainly beyond `lim` (the nearest hit so far / the light) cannot be affected by
                // this triangle — typically the triangle the ray starts on, and hits behind the
                // current best.
                const float A0 = __builtin_fmaf(dx, T.nx, __builtin_fmaf(dy, T.ny, dz * T.nz));
                const float sA0 = __uint_as_float(__float_as_uint(A0) ^ sgn);
                const float E0 = dmax * T.ke2;
                const float a_lo = (absa - E) * 0x1.fffep-1f, a_hi = (absa + E) * 0x1.0002p+0f;
                const mask_t near_m = FCMP(sA0 + E0, min_t * a_lo, FC_OLT);   // t0 < min_t for sure
                const mask_t far_m = FCMP(sA0 - E0, lim * a_hi, FC_OGT);      // t0 > lim for sure (inf/NaN: no)
#ifndef CTR_NO_TREJ
                c_m &= ~(near_m | far_m) | flat_m;
#endif
#ifndef CTR_NO_OCC
                if (anyhit_m != 0ull) {  // wave-uniform: lane masks must never be updated under a per-lane branch
                  CTR_MARK(25);
                  // a deciding shadow ray needs no value at all: clearly inside the triangle and
                  // clearly between min_t and the light = occluded, no exact test
                  const mask_t in_m = FCMP(sA1, E, FC_OGT) & FCMP(sA2, E, FC_OGT) & FCMP(sA1 + sA2, absa - E, FC_OLT);
                  const mask_t tin_m = FCMP(sA0 - E0, min_t * a_hi, FC_OGT) & FCMP(sA0 + E0, light_dist * a_lo, FC_OLT);
                  const mask_t occ_m = c_m & in_m & tin_m & ~flat_m & anyhit_m;
                  if (occ_m != 0ull) {
                    CTR_MARK(26);
                    // (which triangle decided the lane: the merged walk verifies that triangle's mesh afterwards)
                    if (MERGE) morig = INVB(occ_m) ? T.orig : morig;
                    bb_m &= ~occ_m;  // (retired: best / bobj are set once, where the mesh is left)
                    alive_m &= ~occ_m;
                    c_m &= ~occ_m;
                  }
                }
#endif
                CTR_MARK(27);
                if (c_m == 0ull) return;
              }
            }
            if (c_m == 0ull) return;
            if (STATS) { st[3]++; st[8] += __builtin_popcountll(c_m); }
            CTR_MARK(28);  // exact test
            bool retire = false;  // any-hit: this lane found its occluder
            if (INVB(c_m)) {
              // ---- triangle::intersect, default_schema.hpp:57-78: the four determinants in the
              //      reference's operation order ----
              const V3 a = mk(T.ab0.x, T.ab1.x, T.ab2.x), b = mk(T.ab0.y, T.ab1.y, T.ab2.y);
              const V3 d = mk(dx, dy, dz);
              const float alpha = det3(a, b, rd);
              const float A1 = det3(d, b, rd), A2 = det3(a, d, rd), A0 = det3(a, b, d);
              // The three IEEE divisions (beta, gamma, t0) decide five comparisons and deliver t0.
              // 1-ulp-reciprocal quotients are within 2^-21 relative of the exact ones, so with a
              // 2^-18 margin (and an absolute floor for zero/denormal quotients) most lanes are
              // decided without dividing; t0 itself is divided only where its value can matter.
              const float r = __builtin_amdgcn_rcpf(alpha);
              const float bq = A1 * r, gq = A2 * r, tq = A0 * r, sq = bq + gq;
              const float eb = fabsf(bq) * 0x1p-18f + 1e-30f, eg = fabsf(gq) * 0x1p-18f + 1e-30f;
              const float es = (fabsf(bq) + fabsf(gq) + 1.0f) * 0x1p-16f;
              const float et = fabsf(tq) * 0x1p-18f + 1e-30f;
              const bool def_rej = (bq < -eb) | (gq < -eg) | (sq > 1.0f + es) | (tq < min_t - et);
              const bool def_acc = (bq > eb) & (gq > eg) & (sq < 1.0f - es) & (tq > min_t + et) & (fabsf(tq) < 1e37f);
              bool acc = def_acc;
              float t0 = tq;
              bool exact_t = false;
              if (!(def_rej | def_acc)) {
                CTR_MARK(29);  // the reference's three divisions
                // borderline (or NaN/inf): the reference's own arithmetic
                const float beta = A1 / alpha, gamma = A2 / alpha;
                t0 = A0 / alpha;
                exact_t = true;
                acc = beta >= 0 && gamma >= 0 && beta + gamma <= 1 && __builtin_isfinite(t0) && min_t <= t0;
              }
              if (acc) {
                CTR_MARK(30);
                if (anyhit_now) {
                  CTR_MARK(121);
                  // A deciding shadow ray only asks whether some valid t lies in (min_t, light_dist).
                  // tq is within et of the exact t0 and already > min_t + et, so divide only when tq is
                  // within et of the light distance.
                  if (!exact_t && !(tq + et < light_dist) && !(tq - et >= light_dist)) { CTR_MARK(122); t0 = A0 / alpha; }
                  CTR_MARK(123);
                  if (t0 > min_t && t0 < light_dist) { retire = true; if (MERGE) morig = T.orig; }  // (best / bobj: where the mesh is left)
                } else {
                  CTR_MARK(124);
                  // the exact value of t0 matters only if it can beat or tie the nearest hit so far
                  if (!exact_t && !(tq - et > lim)) { CTR_MARK(125); t0 = A0 / alpha; exact_t = true; }
                  CTR_MARK(126);
                  const uint32_t orig = T.orig;
                  if (exact_t && (t0 < mt || (t0 == mt && orig < morig))) {
                    mt = t0; morig = orig;
                    lim = fminf(lim, mt);
                  }
                }
              }
            }
            CTR_MARK(31);
            if (AH) {
              const mask_t rm = BALLOT(retire);
              bb_m &= ~rm;
              alive_m &= ~rm;
            }
          };

#ifdef CTR_TIMING
          unsigned long long t_leaves = 0, t_w0 = 0;
#endif
          if (BVH) {
            // Walk of the mesh's four-wide BVH by the whole wave together (bvh.h, DNode4): one visit =
            // one 128-byte node = the boxes of FOUR children, tested with twelve v_pk_fma_f32 (two
            // children per instruction).  Leaves among the hit children are tested at once, inner
            // children wait on a wave-uniform stack kept in the lanes of ONE VGPR (v_writelane /
            // v_readlane), nearest first: the children are stored sorted along the node's order axis
            // and a wave whose lead ray points the other way takes them in reverse.
            // The box test is conservative: every box is widened in WORLD space by
            //   m = 2^-14 x (largest |coordinate difference| between the ray origin and the mesh box)
            //       + 2^-21 x (largest |coordinate| of the ray origin)
            // per axis ((mn - m - o)/d and (mx + m - o)/d, folded into the two FMA constants below), far
            // above the rounding of either this test or the reference's triangle test (DESIGN.md
            // §bvh); a NaN (0 x inf for an axis-parallel ray) drops that axis' constraint.
            const float gx = fmaxf(fabsf(O.f[0] - ro.x), fabsf(O.f[3] - ro.x));
            const float gy = fmaxf(fabsf(O.f[1] - ro.y), fabsf(O.f[4] - ro.y));
            const float gz = fmaxf(fabsf(O.f[2] - ro.z), fabsf(O.f[5] - ro.z));
            // The margin is folded into the ORIGIN's term: (ro + mw) and its product with 1/d are each rounded to 2^-24 of
            // |ro|, not of the distance to the box.  For a scene far off the origin that rounding exceeds 2^-14 x the distance
            // (from |ro| = 2^10 distances on) and the walk missed triangles the reference hits; so the margin also carries
            // 2^-21 x the origin's largest |coordinate|, four times what the two roundings can take back.
            const float mw = __builtin_fmaf(fmaxf(fmaxf(fabsf(ro.x), fabsf(ro.y)), fabsf(ro.z)), 0x1p-21f, fmaxf(fmaxf(gx, gy), gz) * 0x1p-14f);
            const V3 ka = mk((ro.x + mw) * ria.x, (ro.y + mw) * ria.y, (ro.z + mw) * ria.z);  // for box minima
            const V3 kb = mk((ro.x - mw) * ria.x, (ro.y - mw) * ria.y, (ro.z - mw) * ria.z);  // for box maxima
            const CADDR DNode4 *nodes4 = A.nodes4 + o_node_begin;
            // direction signs of the first lane that needs the mesh decide the visiting order (speed only)
            const uint32_t lead = (uint32_t)__builtin_ctzll(bb_m);
            // (readlane returns int: shift its bits as unsigned — only bits 0..2 are used below, but an arithmetic shift
            //  would smear the sign over the whole word)
            const uint32_t nb_x = (uint32_t)__builtin_amdgcn_readlane(__float_as_uint(rd.x), lead) >> 31,
                           nb_y = (uint32_t)__builtin_amdgcn_readlane(__float_as_uint(rd.y), lead) >> 31,
                           nb_z = (uint32_t)__builtin_amdgcn_readlane(__float_as_uint(rd.z), lead) >> 31;
            // Visiting order (speed only; any order gives the same hit).  Nearest-hit casts go near to far along the lead
            // ray — what they find prunes the rest.  Shadow casts go FAR to near: they start on a surface, whose own
            // neighbourhood is what a near-to-far walk would test first and what occludes least (bunny -2 %, the
            // 64 000-triangle mesh -8 % against near-to-far for both; profiles/r02/traversal_order.txt).
            // (only where a shadow cast stops at its first occluder; the ordered shadow loop of scenes with transparent
            //  materials is a nearest-hit cast)
            // (a phased copy: a constant — the lead lane is a live one, and every live lane casts for the copy's kind)
            const uint32_t lead_shadow = K != TRIP_ANY ? (K == TRIP_SHADOW ? 7u : 0u) : (ANYHIT && ((shadow_m >> lead) & 1ull) != 0ull) ? 7u : 0u;
            const uint32_t neg_bits = lead_shadow ^ (nb_x | (nb_y << 1) | (nb_z << 2));
            // the nine per-ray constants of the box test, two to a register pair; PKFMA picks the half it
            // needs with op_sel, so packing costs no extra registers
            const float2_ c_rxy = {ria.x, ria.y}, c_rzk = {ria.z, ka.x}, c_kyz = {ka.y, ka.z};
            const float2_ c_bxy = {kb.x, kb.y}, c_bz = {kb.z, 0.0f};
            // children (c, c+1) of one node: six v_pk_fma_f32 give the six slab distances of both boxes;
            // a lane takes a child unless it misses for certain: max(entry, min_t) > min(exit, lim)
            // (v_min/v_max drop a NaN operand, a NaN that survives compares false -> entered)
            auto box_hits2 = [&](const auto &N, int c, mask_t &ha, mask_t &hb) {
              float2_ t1x, t1y, t1z, t2x, t2y, t2z;
              PKFMA(t1x, (float2_{N.lo[0][c], N.lo[0][c + 1]}), c_rxy, 0, c_rzk, 1);
              PKFMA(t1y, (float2_{N.lo[1][c], N.lo[1][c + 1]}), c_rxy, 1, c_kyz, 0);
              PKFMA(t1z, (float2_{N.lo[2][c], N.lo[2][c + 1]}), c_rzk, 0, c_kyz, 1);
              PKFMA(t2x, (float2_{N.hi[0][c], N.hi[0][c + 1]}), c_rxy, 0, c_bxy, 0);
              PKFMA(t2y, (float2_{N.hi[1][c], N.hi[1][c + 1]}), c_rxy, 1, c_bxy, 1);
              PKFMA(t2z, (float2_{N.hi[2][c], N.hi[2][c + 1]}), c_rzk, 0, c_bz, 0);
              // both boxes' slab arithmetic as ONE statement (the same twenty-two instructions, interleaved): between separate
              // statements the compiler pads with s_nop for hazards it cannot rule out — eleven per node visit
              float u0, u1, u2, u3, w0, w1, w2, w3;
              mask_t ma, mb;
              asm("v_min_f32 %0, %10, %13\n\tv_min_f32 %4, %16, %19\n\t"
                  "v_min_f32 %1, %11, %14\n\tv_min_f32 %5, %17, %20\n\t"
                  "v_min_f32 %2, %12, %15\n\tv_min_f32 %6, %18, %21\n\t"
                  "v_max_f32 %3, %10, %13\n\tv_max_f32 %7, %16, %19\n\t"
                  "v_max3_f32 %0, %0, %1, %2\n\tv_max3_f32 %4, %4, %5, %6\n\t"
                  "v_max_f32 %1, %11, %14\n\tv_max_f32 %5, %17, %20\n\t"
                  "v_max_f32 %2, %12, %15\n\tv_max_f32 %6, %18, %21\n\t"
                  "v_max_f32 %0, %0, %22\n\tv_max_f32 %4, %4, %22\n\t"
                  "v_min3_f32 %1, %3, %1, %2\n\tv_min3_f32 %5, %7, %5, %6\n\t"
                  "v_min_f32 %1, %1, %23\n\tv_min_f32 %5, %5, %23\n\t"
                  "v_cmp_gt_f32_e64 %8, %0, %1\n\tv_cmp_gt_f32_e64 %9, %4, %5"
                  : "=&v"(u0), "=&v"(u1), "=&v"(u2), "=&v"(u3), "=&v"(w0), "=&v"(w1), "=&v"(w2), "=&v"(w3), "=&s"(ma), "=&s"(mb)
                  : "v"(t1x.x), "v"(t1y.x), "v"(t1z.x), "v"(t2x.x), "v"(t2y.x), "v"(t2z.x),
                    "v"(t1x.y), "v"(t1y.y), "v"(t1z.y), "v"(t2x.y), "v"(t2y.y), "v"(t2z.y), "v"(min_t), "v"(lim));
              ha = bb_m & ~ma;
              hb = bb_m & ~mb;
            };
            const CADDR DTri *tb_ = A.tris + beg;   // the mesh's first record: leaves address theirs by a 32-bit byte offset from it
            auto leaf = [&](uint32_t desc, mask_t lanes) {
              TSTAMP(t_leaf0);
              CTR_MARK(80);  // a leaf's triangles
              uint32_t t_off = (desc & 0xFFFFFFu) << 6;   // byte offset of the leaf's first record from the mesh's first
              const uint32_t n_l = (desc >> 24) & 0x7Fu;
              // The leaf's first triangle is fetched as one 64-byte record, and one dword of each of the next three cache
              // lines is requested with it, into a register nobody reads ("touch"): the loads of the leaf's other triangles —
              // one dependent round trip each — then find their lines in the scalar cache.  64 000 triangles -3 %, first
              // launch -5 %; a 1 000-triangle mesh, which stays in the scalar cache anyway, +-0.5 %
              // (profiles/r03/exp_leaf_touch.txt).  The wait is part of the statement, so the unread register is dead when it
              // ends.  (ctr_scene.cpp allocates 256 bytes beyond every array for requests past the last triangle.)
              // (no early exit for an empty leaf — the unused slots of a node, whose far-away point box no ray enters: it
              //  would only re-test the mesh's first triangle, which changes nothing, and the extra edge costs six register
              //  copies per leaf visit in the compiler's output)
              typedef uint32_t u32x16_ __attribute__((ext_vector_type(16)));
              u32x16_ t0;
              uint32_t touch_;
              asm volatile("s_load_dwordx16 %0, %2, %3\n\ts_load_dword %1, %2, %3 offset:0x40\n\ts_load_dword %1, %2, %3 offset:0x80\n\ts_load_dword %1, %2, %3 offset:0xc0\n\ts_waitcnt lgkmcnt(0)"
                           : "=&s"(t0), "=&s"(touch_) : "s"(tb_), "s"(t_off));
              TriR cur;
#define CTR_UNPACK_TRI()                                                                                                                              \
              cur.ab0.x = __uint_as_float(t0[0]); cur.ab0.y = __uint_as_float(t0[1]); cur.ab1.x = __uint_as_float(t0[2]); cur.ab1.y = __uint_as_float(t0[3]); \
              cur.ab2.x = __uint_as_float(t0[4]); cur.ab2.y = __uint_as_float(t0[5]); cur.pxy.x = __uint_as_float(t0[6]); cur.pxy.y = __uint_as_float(t0[7]); \
              cur.pz = __uint_as_float(t0[8]); cur.orig = t0[9]; cur.nx = __uint_as_float(t0[10]); cur.ny = __uint_as_float(t0[11]);                       \
              cur.nz = __uint_as_float(t0[12]); cur.ke = __uint_as_float(t0[13]); cur.ke2 = __uint_as_float(t0[14]);
              CTR_UNPACK_TRI()
              for (uint32_t k = 0;;) {
                tri_test(cur, 0u, lanes & bb_m);
                if (AH) {
                  if (bb_m == 0ull) break;
                }
                if (++k >= n_l) break;
                CTR_MARK(82);  // the leaf's next triangle
                // the leaf's next record: ONE 64-byte request at the running offset (the compiler's own form is a 64-bit address
                // and four requests for the record's fifteen words)
                t_off += 64u;
                asm volatile("s_load_dwordx16 %0, %1, %2\n\ts_waitcnt lgkmcnt(0)" : "=&s"(t0) : "s"(tb_), "s"(t_off));
                CTR_UNPACK_TRI()
              }
#ifdef CTR_TIMING
              t_leaves += __builtin_readcyclecounter() - t_leaf0;
#endif
            };
            // push one inner child (wave-uniform value and slot: both travel as SGPRs)
            uint32_t stack_v = 0;  // lane k of this VGPR = stack slot k (at most 3 per level, BVH4_MAX_DEPTH levels)
            uint32_t sp = 0;
            auto push = [&](uint32_t d) {
              stack_v = ctr_writelane(__builtin_amdgcn_readfirstlane(d), __builtin_amdgcn_readfirstlane(sp), stack_v);
              sp++;
            };
            // node 0 is the root (a mesh that fits one leaf has a root with one child).  A mesh with guard
            // records (triangles every lane must meet whatever their box, ctr_scene.cpp refresh_linear_meshes)
            // starts one node earlier, at an extra node whose children are the guard leaf and the root.
            uint32_t cur = o_bvh_root;
#ifdef CTR_TIMING
            t_w0 = __builtin_readcyclecounter();
            tm[4] += t_w0 - t_bb;
#endif
            for (;;) {
              if (STATS) st[1]++;
              CTR_MARK(32);  // BVH node
              // the node's 128 bytes as two requests at a 32-bit byte offset from the mesh's first node (one shift; the compiler's
              // own form was a 64-bit address — four scalar instructions — and five requests in three waits)
              typedef uint32_t u32x16n_ __attribute__((ext_vector_type(16)));
              u32x16n_ nq0, nq1;
              asm volatile("s_load_dwordx16 %0, %2, %3\n\ts_load_dwordx16 %1, %2, %3 offset:0x40\n\ts_waitcnt lgkmcnt(0)"
                           : "=&s"(nq0), "=&s"(nq1) : "s"(nodes4), "s"(cur << 7));
              struct NodeR { float lo[3][4], hi[3][4]; uint32_t child[4], axis; } N;
              for (int a_ = 0; a_ < 3; ++a_) for (int c_ = 0; c_ < 4; ++c_) N.lo[a_][c_] = __uint_as_float(nq0[a_ * 4 + c_]);
              for (int c_ = 0; c_ < 4; ++c_) N.hi[0][c_] = __uint_as_float(nq0[12 + c_]);
              for (int a_ = 1; a_ < 3; ++a_) for (int c_ = 0; c_ < 4; ++c_) N.hi[a_][c_] = __uint_as_float(nq1[(a_ - 1) * 4 + c_]);
              for (int c_ = 0; c_ < 4; ++c_) N.child[c_] = nq1[8 + c_];
              N.axis = nq1[12];
              mask_t h0, h1, h2, h3;
              box_hits2(N, 0, h0, h1);
              box_hits2(N, 2, h2, h3);
              // (round 4 tried NOT testing the second pair of a node that has only two children — a third of the bunny tree's
              //  nodes, unused slots come last: 28 of a visit's 56 box instructions saved there, and bunny +3.4 %, 64 000 triangles
              //  +2.7 %, C4 +3.3 % — the branch waits for the child descriptors before the second pair's arithmetic can issue)
              const uint32_t d0 = N.child[0], d1 = N.child[1], d2 = N.child[2], d3 = N.child[3], n_axis_ = N.axis;
              if (STATS) { st[6] += __builtin_popcountll(h0 | h1 | h2 | h3); pl_nodes += INVB(h0 | h1 | h2 | h3) ? 1u : 0u; }
              // children are stored sorted along the node's order axis; a wave whose lead ray points the other
              // way takes them in reverse: TWO copies of the dispatch below behind one scalar branch — selecting the four
              // descriptors and four masks into "nearest ... farthest" registers first was ten scalar instructions per visit
              // (round 4: bunny -3.4 %, 64 000 triangles -2.7 %; profiles/r04/exp_scalar_diet_ab.txt)
              const bool rev = ((neg_bits >> n_axis_) & 1u) != 0u;
              // ONE pass, farthest child first: a hit leaf is tested at once; a hit inner child becomes the node to
              // visit next and whatever was to be visited next is pushed — so the nearest inner child is visited
              // next and the stack pops nearest-first.  No per-child bookkeeping beyond two scalar tests.
              CTR_MARK(33);  // child dispatch
              uint32_t next = 0xFFFFFFFFu;
              bool done = false;
#define CTR_CHILD(e, g, id)                                         \
  CTR_MARK(id);                                                     \
  if (!done && (g) != 0ull) {                                       \
    CTR_MARK(id + 5);                                               \
    if ((e) & BVH_LEAF_FLAG) {                                      \
      leaf((e), (g));                                               \
      CTR_MARK(id + 10);                                            \
      if (AH) {                                                     \
        if (bb_m == 0ull) done = true;                              \
      }                                                             \
    } else {                                                        \
      CTR_MARK(id + 15);                                            \
      if (next != 0xFFFFFFFFu) push(next);                          \
      next = (e);                                                   \
    }                                                               \
  }
              if (rev) {
                CTR_CHILD(d0, h0, 60)
                CTR_CHILD(d1, h1, 61)
                CTR_CHILD(d2, h2, 62)
                CTR_CHILD(d3, h3, 63)
              } else {
                CTR_CHILD(d3, h3, 60)
                CTR_CHILD(d2, h2, 61)
                CTR_CHILD(d1, h1, 62)
                CTR_CHILD(d0, h0, 63)
              }
#undef CTR_CHILD
              CTR_MARK(34);
              if (done) break;
              if (next == 0xFFFFFFFFu) {
                CTR_MARK(81);
                if (sp == 0) break;
                sp--;
                next = __builtin_amdgcn_readlane(stack_v, sp);
              }
              cur = next;
            }
          } else {
            for (uint32_t k = 0; k < cnt; ++k) {
              tri_test(load_tri(A.tris[beg + k]), beg + k, bb_m);  // wave-uniform: one s_load_dwordx16
              if (ANYHIT) {
                if (bb_m == 0ull) break;
              }
            }
          }
          if (STATS) {
            for (int off = 32; off > 0; off >>= 1) {
              const uint32_t on = (uint32_t)__shfl_xor((int)pl_nodes, off), ot = (uint32_t)__shfl_xor((int)pl_tris, off);
              pl_nodes = on > pl_nodes ? on : pl_nodes;
              pl_tris = ot > pl_tris ? ot : pl_tris;
            }
            st[9] += (uint32_t)__builtin_amdgcn_readfirstlane((int)pl_nodes);
            st[10] += (uint32_t)__builtin_amdgcn_readfirstlane((int)pl_tris);
          }
          // ---- merged walk: the AABB test of the meshes the walk found something in ----
          // The walk above went through ONE tree over the triangles of all meshes; a lane's `morig` now names the triangle
          // that decided it (nearest valid hit, or the occluder of a deciding shadow ray) as (mesh rank << 24 | file index).
          // The reference tests a mesh's box BEFORE its triangles (default_schema.hpp:126): a ray that fails it misses the
          // mesh whatever the triangle test says — possible only within rounding of the box's faces, but then the lane's
          // result, and everything the walk pruned because of it, is wrong.  So: per mesh that decided a lane (usually
          // one or two per cast) the reference's test for those lanes.  Any lane failing it, or a mesh whose nearest valid
          // t equals min_t exactly (ray_cast.hpp:43 then rejects the whole mesh, strict >), and the cast walks the
          // scene's two-level structure instead, which has the reference's form — measure-zero events, not a fast path.
          int i_lane = merged ? 0 : (int)i;   // scene index of the mesh that decided the lane
          int ctri_lane = (int)(beg + morig); // its triangle's position in the normals array (file order within its mesh)
          if (MERGE && merged) {
            CTR_MARK(86);
            if (STATS && lane == 0) atomicAdd(&g_lane_stats[78], 1ull);
            mask_t todo = BALLOT(morig != 0xFFFFFFFFu);
            mask_t bad_m = BALLOT(mt != INFINITY && !(mt > min_t));
            while (todo != 0ull) {
              const uint32_t rk = (uint32_t)__builtin_amdgcn_readlane((int)morig, (int)__builtin_ctzll(todo)) >> 24;
              const mask_t same_m = todo & BALLOT((morig >> 24) == rk);
              const CADDR DObj &R = AK->meshes[k_mesh + 1u + rk];
              const uint32_t r_index = R.index, r_beg = R.tri_begin;
              bad_m |= same_m & ~box_test(R, same_m, SITE(1));
              if (INVB(same_m)) { i_lane = (int)r_index; ctri_lane = (int)(r_beg + (morig & 0xFFFFFFu)); }
              todo &= ~same_m;
            }
            if (bad_m != 0ull) {
              CTR_MARK(87);  // this cast again, through the top-level tree and the meshes' own trees
              if (STATS && lane == 0) atomicAdd(&g_lane_stats[77], 1ull);
              if (ANYHIT) {
                alive_m |= bad_m & anyhit_m;  // (a deciding shadow ray whose occluder does not count is alive again)
                if (INVB(anyhit_m & ~alive_m)) { best = fminf(0.5f * light_dist, 1e30f); bobj = i_lane; }
              }
              t_pend = AK->tlas_root2;
              t_sp = 0u;
              continue;
            }
          }
          CTR_MARK(35);  // mesh left
          if (ANYHIT) {
            // lanes retired inside the mesh (deciding shadow rays that met an occluder): the handler only asks
            // best < light_dist.  Written here, once, rather than in the triangle test: values a loop changes are copied
            // in and out of it by the compiler (six v_mov each way per leaf visit for six such values; now three).
            // (every deciding shadow ray that has retired by now, in this mesh or before it: writing the same again for the
            //  earlier ones is harmless — the handler never asks which object it was — and saves carrying the mesh's entry
            //  mask through the walk: scalar registers are what this kernel is shortest of)
            if (NEAREST && INVB(anyhit_m & ~alive_m)) { best = fminf(0.5f * light_dist, 1e30f); bobj = i_lane; }
          }
          ok = mt != INFINITY;  // default_schema.hpp:143 (lanes outside the AABB never set mt)
          cand = mt;
          ctri = ctri_lane;  // gnorm is indexed by the triangle's FILE-order position within its mesh
          obj_lane = i_lane;
#ifdef CTR_TIMING
          {
            const unsigned long long t_mesh1 = __builtin_readcyclecounter();
            if (t_w0 == 0) t_w0 = t_bb;  // linear walk
            tm[5] += (t_mesh1 - t_w0) - t_leaves;
            tm[6] += t_leaves;
          }
#endif

        }
        // ray_cast.hpp:43 — strict <, first object in scene order wins ties
        if (NEAREST && INVB(alive_m) && ok && cand > min_t && (cand < best || (cand == best && obj_lane < bobj))) {
          best = cand;
          bobj = obj_lane;
          btri = ctri;
        }
        // (no "a deciding shadow ray with a valid mesh hit stops searching" here: in the any-hit build such a lane never
        //  records a mesh hit — it retires inside the walk, above)
      }
    }
    if (STATS && st_shadow_entry != 0ull && lane == 0) {
      const bool planes_only = (st_recv_mesh & st_shadow_entry) == 0ull, none_occluded = (st_shadow_entry & ~alive_m) == 0ull;
      atomicAdd(&g_lane_stats[80], 1ull);
      if (planes_only) atomicAdd(&g_lane_stats[81], 1ull);
      if (planes_only && none_occluded) atomicAdd(&g_lane_stats[82], 1ull);
      if (none_occluded) atomicAdd(&g_lane_stats[83], 1ull);
    }
    const bool was_hit = bobj >= 0;
    TSTAMP(t_loop1);
    CTR_MARK(36);  // continuation

    // =====================================================================
    // continuation: what did this lane cast the ray for?
    // =====================================================================
    // the continuation's kernel arguments in ONE round trip (pointer by pointer, each was a scalar load the wave waited
    // for before it could even request the record behind it)
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    const u32x8 cold = *(const CADDR u32x8 *)&AK->objs;
    const u32x4 cold2 = *(const CADDR u32x4 *)&AK->n_light;
    const CADDR DObj *const k_objs = (const CADDR DObj *)(((uint64_t)cold[1] << 32) | cold[0]);
    const CADDR float *const k_gnorm = (const CADDR float *)(((uint64_t)cold[3] << 32) | cold[2]);
    const CADDR DLight *const k_lights = (const CADDR DLight *)(((uint64_t)cold[5] << 32) | cold[4]);
    const CADDR DMat *const k_mats = (const CADDR DMat *)(((uint64_t)cold[7] << 32) | cold[6]);
    const uint32_t k_n_light = cold2[0];
    const int k_bounces = (int)cold2[1];
    int act = ACT_NONE;
    float first_depth = 0.f;  // primary-hit depth of this lane, alive in the first trip only
    // the light the NEXT shadow ray goes to (type and position / direction), requested together with whatever else this
    // continuation reads first — the hit record, or the material and light being shaded — instead of in a round trip of its
    // own afterwards.  (lights[n_light] is inside the allocation: ctr_scene.cpp pads every array.)
    uint32_t nl_type = 0u;
    V3 nl_v = mk(0.f, 0.f, 0.f);
    // (a phased copy holds its own kind's branch alone, for the lanes that cast: the active ones)
    if (K == TRIP_ANY ? MSP_IS_RADIANCE(msp) : (K == TRIP_RADIANCE && active)) {
      const V3 ro_keep = ro;  // (IGNTR: the primary ray is cast once more, for ray_color)
      // ---- hit record: hit point, normal (per primitive), material ----
      V3 normal = mk(0, 0, 0);
      float tc_u = 0.0f, tc_v = 0.0f;  // (UV) uv{} of kernel.hpp:51 on a miss
      if (was_hit) {
        const CADDR DObj &H = k_objs[bobj];
        CTR_MARK(37);  // hit record
        // (type, material, the six floats and the triangle's normal are requested together, before the type decides
        //  which of them is used: one vector-memory round trip instead of two)
        const uint32_t ht = H.type;
        const float hf0 = H.f[0], hf1 = H.f[1], hf2 = H.f[2], hf3 = H.f[3], hf4 = H.f[4], hf5 = H.f[5];
        float gn0 = 0.f, gn1 = 0.f, gn2 = 0.f;
        if (btri >= 0) { gn0 = k_gnorm[4 * btri + 0]; gn1 = k_gnorm[4 * btri + 1]; gn2 = k_gnorm[4 * btri + 2]; }  // (a scene without triangles has no such array)
        mat_i = H.mat;
        if (STATS) recv_mesh = (ht == CTR_OBJ_MESH || ht == CTR_OBJ_TRIANGLE);
        { const CADDR DLight &L0 = k_lights[0]; nl_type = L0.type; nl_v = mk(L0.vx, L0.vy, L0.vz); }
        // (OPAQUE: the direction of the radiance ray just cast is `rd` — every radiance cast starts with rd = in_d and no cast
        //  writes it — so in_d is not read here, nor after)
        const V3 hit_d = OPAQUE ? rd : in_d;
        const V3 hit_pos = vadd(ro, vscale(hit_d, best));  // start + dist*dir (triangle/plane hit; shading.hpp:133,143)
        if constexpr (!OPAQUE) pos = hit_pos;
        float unused_n0;
        const V3 hit_dn = vnormalized_n(hit_d, unused_n0);
        CTR_MARK(92);
        set_in_dn(hit_dn);
        if constexpr (OPAQUE) {
          // one-mesh shape: the hit is a plane or the mesh (no sphere, no stand-alone triangle; no uv build), and the hit point
          // lives in `ro` alone until the bounce
          ro = hit_pos;
          normal = ht == CTR_OBJ_PLANE ? mk(hf3, hf4, hf5) : mk(gn0, gn1, gn2);
        } else if (ht == CTR_OBJ_SPHERE) {
          CTR_MARK(38);
          // default_schema.hpp:245-246: hit uses the NORMALIZED direction
          const V3 hit = vadd(ro, vscale(hit_dn, best));
          normal = vnormalized(vsub(hit, mk(hf0, hf1, hf2)));
          ro = hit;
          if (UV && first_trip) {  // default_schema.hpp:246-249: delta = (hit - center).normalized() is the normal again
            tc_u = 0.5f + (atan2f(normal.z, normal.x) / (2.0f * (float)M_PI));
            tc_v = 0.5f + (asinf(normal.y) / (float)M_PI);
          }
        } else if (ht == CTR_OBJ_PLANE) {
          ro = pos;
          normal = mk(hf3, hf4, hf5);
          if (UV && first_trip) {  // plane::uv_for, default_schema.hpp:169-178
            const V3 ax1 = vnormalized(mk(normal.y, -normal.x, 0.0f));
            const V3 ax2 = vcross(normal, ax1);
            const V3 mod_pt = vsub(mk(hf0, hf1, hf2), pos);
            tc_u = vdot(ax1, mod_pt);
            tc_v = vdot(ax2, mod_pt);
          }
        } else {
          ro = pos;
          normal = mk(gn0, gn1, gn2);
          if (UV && first_trip) {
            if (ht == CTR_OBJ_MESH) {  // mesh::intersect, default_schema.hpp:138-139
              tc_u = pos.x;
              tc_v = pos.y;
            } else {                   // triangle::uv_for, default_schema.hpp:37-46
              const CADDR DTri &T = A.tris[btri];
              const V3 p1 = mk(hf0, hf1, hf2), p2 = mk(T.px, T.py, T.pz), p3 = mk(hf3, hf4, hf5);
              const V3 p2p1 = vsub(p2, p1), p3p1 = vsub(p3, p1), xp1 = vsub(pos, p1);
              const V3 proj_u = vscale(p2p1, vdot(xp1, p2p1) / vdot(p2p1, p2p1));
              const V3 proj_v = vscale(p3p1, vdot(xp1, p3p1) / vdot(p3p1, p3p1));
              tc_u = vnorm(proj_u) / vnorm(p2p1);
              tc_v = vnorm(proj_v) / vnorm(p3p1);
            }
          }
        }
      }
      CTR_MARK(39);
      if (first_trip) {
        // kernel.hpp:55-56 (depth = +inf, normal = 0 on a miss)
        CTR_MARK(40);
        const size_t px_id = px_index();
        float *const k_depth_out = ((const CADDR KParams *)AK)->depth_out, *const k_normal_out = ((const CADDR KParams *)AK)->normal_out;
        if constexpr (SS) {
          if (ss_kept()) {
            k_depth_out[px_id] = best;
            store3(k_normal_out, px_id, normal);
          }
        } else {
          if (HOSTOUT) __hip_atomic_store(k_depth_out + px_id, best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          else k_depth_out[px_id] = best;
          store3(k_normal_out, px_id, normal);
        }
        if (UV) {
          float *const uvp = AK->uv_out;
          uvp[2 * px_id + 0] = tc_u;
          uvp[2 * px_id + 1] = tc_v;
        }
        first_depth = best;
      }
      CTR_MARK(41);
      if (IGNTR && ign_now) {
        // that was the cast of kernel.hpp:52; now ray_color's own first cast (shading.hpp:123, ignore_transparent = false) of the same ray
        ro = ro_keep;
        min_t = A.fudge;
      } else if (!was_hit) {
        out_rgb = mk(0.f, 0.f, 0.f);  // shading.hpp:119
        act = ACT_UNWIND;
      } else {
        // phong prologue, shading.hpp:66-76
        CTR_MARK(42);
        const CADDR DMat &M = k_mats[mat_i];
        fin = vscale(mk(M.cx, M.cy, M.cz), RAYS ? AK->ray_ambient : ambient);
        { float unused_n; const V3 nrm_ = vnormalized_n(normal, unused_n); CTR_MARK(93); set_nn(nrm_); }
        li_k = 0;
        act = ACT_LIGHT;
        if constexpr (ROOM_CODE) {
          // "room-safe lanes": the lane predicate of the room facts for the hit point every shadow ray of this hit starts from,
          // once for all its lights — the numerators (point - origin).normal of the head's triple exactly as the plane phase
          // forms them, none above room_delta, and the origin inside the box (a NaN fails a compare; all-zero facts fail the
          // box: 0 <= 0 needs the origin AT the centre, and then the trip head finds no light's bit).
          // (the triple's twelve floats are read again here, through a pointer of its own and only where a hit is shaded: kept
          //  from the trip head they would live in scalar registers through the mesh walk)
          const CADDR KArgs *AR = AK;
          asm volatile("" : "+s"(AR));
          const u32x8 rm_ax_lo = *(const CADDR u32x8 *)&AR->head.ax[0][0];
          const u32x4 rm_ax_hi = *(const CADDR u32x4 *)&AR->head.ax[4][0];
          const u32x2 rm_c01 = *(const CADDR u32x2 *)&AR->head.room_c[0];
          const u32x4 rm_rest = *(const CADDR u32x4 *)&AR->head.room_c[2];  // room_c[2], room_r, room_delta, room_lights
          auto rm_ax = [&](int i) -> uint32_t { return i < 8 ? rm_ax_lo[i] : rm_ax_hi[i - 8]; };
          if (rm_rest[3] != 0u) {  // (wave-uniform)
            auto pr = [&](int k) -> float2_ { const float2_ v = {__uint_as_float(rm_ax(2 * k)), __uint_as_float(rm_ax(2 * k + 1))}; return v; };
            const float2_ ox = {ro.x, ro.x}, oy = {ro.y, ro.y}, oz = {ro.z, ro.z};
            const float2_ n0 = (pr(0) - ox) * pr(1), n1 = (pr(2) - oy) * pr(3), n2 = (pr(4) - oz) * pr(5);
            const float num_max = fmaxf(fmaxf(fmaxf(n0.x, n0.y), n1.x), fmaxf(fmaxf(n1.y, n2.x), n2.y));
            const float room_r = __uint_as_float(rm_rest[1]);
            const bool in_box = fabsf(ro.x - __uint_as_float(rm_c01[0])) <= room_r && fabsf(ro.y - __uint_as_float(rm_c01[1])) <= room_r &&
                                fabsf(ro.z - __uint_as_float(rm_rest[0])) <= room_r;
            msp |= (in_box && num_max <= __uint_as_float(rm_rest[2])) ? MSP_ROOM : 0u;
          }
        }
      }
    } else if (K == TRIP_ANY ? MSP_IS_SHADOW(msp) : (K == TRIP_SHADOW && active)) {
      // ---- one iteration of shadow_intensity's loop, shading.hpp:32-42 ----
      CTR_MARK(43);
      { const CADDR DLight &L1 = k_lights[li_k + 1u]; nl_type = L1.type; nl_v = mk(L1.vx, L1.vy, L1.vz); }
      bool done_shadow;
      float shadow_fac = 0.f;
      // (a dark lane made no cast: it takes the occluded side, which adds nothing — as the lit side would, bit for bit)
      const bool dark_lane = DARK && K != TRIP_SHADOW && (msp & MSP_DARK) != 0u;
      // (the shadow copy: the lanes that left alive_m — retired by an occluder, or dark from the start: NEAREST above)
      if (K == TRIP_SHADOW ? !INVB(alive_m) : ((was_hit && best < light_dist) || dark_lane)) {
        // scenes without any transparency (the any-hit builds) need no material lookup here
        const float trans = ANYHIT ? 0.0f : k_mats[k_objs[bobj].mat].transparency;
        if (!ANYHIT) intensity += (1.0f - trans);
        if (ANYHIT || intensity >= 1.0f) { shadow_fac = 1.0f; done_shadow = true; }
        else {
          min_t = (float)((double)best + 1e-3);  // last_hit + 1e-3 is a double add, shading.hpp:32
          done_shadow = false;                   // cast again (same ray)
        }
      } else {
        shadow_fac = ANYHIT ? 0.0f : intensity;  // any-hit builds: the first occluder already ended the loop
        done_shadow = true;
      }
      if (done_shadow) {
        if (shadow_fac < 1.0f) {
          // shading.hpp:86-95
          CTR_MARK(44);  // shade one light
          const CADDR DMat &M = k_mats[mat_i];
          const CADDR DLight &Lg = k_lights[li_k];
          const V3 diffuse = mk(M.cx, M.cy, M.cz);
          const V3 specular = vscale(diffuse, M.specular);  // default_schema.hpp:328
          const V3 color = mk(Lg.cx, Lg.cy, Lg.cz);
          const V3 nd = rd;  // the shadow ray's direction IS the normalized direction to the light
          const V3 nn_ = get_nn();
          float fd, fs;
          const V3 ld = vmul(diffuse, color);
          if constexpr (DARK_CODE) {
            // the factors the light's set-up tested, by the same functions from the same rd (fd is made again, not kept: a
            // register through the whole cast would take the 6-wave host-delivery build from 79 to 81 VGPRs, and to 5 waves)
            fd = light_fd(nn_, nd);
            fs = light_fs<FASTPOW>(nn_, get_in_dn(), nd, M);
          } else {
            // (every other build: light_fd and light_fs written out, as they were — inlined from the functions the compiler
            //  orders this segment's loads differently, and these builds are to stay what they were instruction for instruction)
            fd = smax(0.0f, vdot(nn_, nd));
            const V3 hsum = vadd(vscale(get_in_dn(), -1.0f), nd);
            const V3 hv = FASTPOW ? vscale(hsum, __builtin_amdgcn_rsqf(vdot(hsum, hsum))) : vnormalized(hsum);
            const float sx = smax(0.0f, vdot(nn_, hv));
            if (FASTPOW) {
              fs = (M.phong_exp == 0.0f) ? 1.0f : __builtin_amdgcn_exp2f(M.phong_exp * __builtin_amdgcn_logf(sx));
            } else {
              fs = (float)pow((double)sx, (double)M.phong_exp);  // f64, rounded once: <= 1 ulp from glibc powf
            }
          }
          const V3 ls = vmul(specular, color);
          fin = vadd(fin, vscale(vadd(vscale(ld, fd), vscale(ls, fs)), 1 - shadow_fac));
        }
        CTR_MARK(45);
        if constexpr (K != TRIP_SHADOW) li_k++;  // (the shadow copy: the next light is `phase`, a scalar — below)
        act = ACT_LIGHT;
      }
    }

    TSTAMP(t_cont_mid);
    TACC(7, t_loop1, t_cont_mid);
    CTR_MARK(46);
    if (act == ACT_LIGHT) {
      if ((K == TRIP_SHADOW ? phase : li_k) < k_n_light) {  // (shadow copy: phase == li + 1, wave-uniform)
        // shading.hpp:79-85: direction/distance to light li, shadow ray from *hit
        CTR_MARK(47);  // next light
        const uint32_t lg_type = nl_type;
        const V3 lg_v = nl_v;
        V3 direction;
        float distance;
        if (lg_type == CTR_LIGHT_SUN) {  // default_schema.hpp:280-283
          direction = vscale(lg_v, -1.0f);
          distance = INFINITY;
        } else {                         // default_schema.hpp:305-308
          CTR_MARK(48);  // point light
          const V3 diff = vsub(lg_v, ro);  // ro == *hit
          direction = vnormalized_n(diff, distance);
          CTR_MARK(94);
        }
        CTR_MARK(49);
        float dir_norm;
        rd = vnormalized_n(direction, dir_norm);  // shadow ray {*hit, direction.normalized()}, shading.hpp:80
        CTR_MARK(95);
        light_dist = distance * dir_norm;
        intensity = 0.0f;
        min_t = (float)(0.0 + 1e-3);  // last_hit = 0
        if constexpr (DARK_CODE) {
          // "dark lights": is this light's term a signed zero that `fin` does not notice?  fd for every lane; fs and the guard on
          // `fin` only in a wave that has a lane with fd zero, for those lanes.  The bit lasts for one light: it is set or cleared
          // here, together with MSP_SHADOW.  A DARK build is launched only with the fact; the statistics builds read it (through a
          // pointer of its own, so that the load stays here).
          // (msp is written ONCE, after the test: written before it and or-ed into afterwards, the 6-wave host-delivery build
          //  takes 81 VGPRs instead of 79 and loses its sixth wave)
          uint32_t hd_dark = 1u;
          if constexpr (!DARK) {
            const CADDR KArgs *AD = AK;
            asm volatile("" : "+s"(AD));
            hd_dark = AD->head.mesh_dark & CTR_HEAD_DARK;
          }
          bool dark = false;
          if (hd_dark != 0u) {
            CTR_MARK(121);
            const V3 nn_ = get_nn();
            const bool fd_zero = (__float_as_uint(light_fd(nn_, rd)) & 0x7FFFFFFFu) == 0u;  // +0 or -0 as bits: a denormal is not zero
            if (BALLOT(fd_zero) != 0ull) {
              CTR_MARK(122);
              if (fd_zero) {
                const float fs = light_fs<FASTPOW>(nn_, get_in_dn(), rd, k_mats[mat_i]);
                dark = (__float_as_uint(fs) & 0x7FFFFFFFu) == 0u && __float_as_uint(fin.x) != 0x80000000u &&
                       __float_as_uint(fin.y) != 0x80000000u && __float_as_uint(fin.z) != 0x80000000u;
              }
              if (STATS) {
                const mask_t dk_m = BALLOT(dark);
                if (dk_m != 0ull && lane_now() == (uint32_t)__builtin_ctzll(dk_m)) atomicAdd(&g_lane_stats[90], (unsigned long long)__builtin_popcountll(dk_m));
              }
            }
          }
          // (a phased build keeps no mode bits: the kind of the next trip is `phase`)
          msp = (msp & ~MSP_DARK) | (PHASED ? 0u : MSP_SHADOW) | (dark ? MSP_DARK : 0u);
        } else {
          if constexpr (!PHASED) msp |= MSP_SHADOW;
        }
      } else {
        act = ACT_BOUNCE;  // phong returned `fin`
      }
    }

    if (act == ACT_BOUNCE) {
      // shading.hpp:126-150 with rgb = fin
      CTR_MARK(50);
      const CADDR DMat &M = k_mats[mat_i];
      const float reflective = M.reflexivity, translucent = OPAQUE ? 0.0f : M.transparency;  // (OPAQUE: the lemma; not read)
      const int sp = MSP_DEPTH(msp);
      const bool more = sp < k_bounces;  // `if constexpr (bounces != 0)`
      const bool do_refl = more && (double)reflective >= 1e-6;
      const bool do_trans = !OPAQUE && more && (double)translucent >= 1e-6;
      if (do_refl || do_trans) {
        CTR_MARK(51);  // push a frame, cast the child
        STK(sp, F_R) = fin.x; STK(sp, F_G) = fin.y; STK(sp, F_B) = fin.z;
        STK(sp, F_MAT) = __uint_as_float(mat_i | (do_refl ? 1u << 30 : 2u << 30));  // the material says reflective / translucent
        if constexpr (!OPAQUE) {
          if (do_refl && do_trans) {  // the pass-through child is cast after the reflection returns
            CTR_MARK(96);
            STK(sp, F_PX) = pos.x; STK(sp, F_PY) = pos.y; STK(sp, F_PZ) = pos.z;
            STK(sp, F_DX) = in_d.x; STK(sp, F_DY) = in_d.y; STK(sp, F_DZ) = in_d.z;
          }
        }
        CTR_MARK(120);
        msp = (uint32_t)(sp + 1);  // one frame deeper, a radiance cast
        if constexpr (OPAQUE) {
          // the child is the reflection (do_refl holds here); it starts at the hit point, which `ro` still is
          const V3 nn_ = get_nn(), dn_ = get_in_dn();
          rd = vsub(dn_, vscale(nn_, 2.0f * vdot(nn_, dn_)));
        } else {
          if (do_refl) {
            // reflect(nd, nn) = nd - (2*(nn.nd))*nn, vector.hpp:204-206
            const V3 nn_ = get_nn(), dn_ = get_in_dn();
            in_d = vsub(dn_, vscale(nn_, 2.0f * vdot(nn_, dn_)));
          }
          ro = pos; rd = in_d;
        }
        min_t = A.fudge;
      } else {
        out_rgb = fin;
        act = ACT_UNWIND;
      }
    }

    if (act == ACT_UNWIND) {
      // return `out_rgb` to the suspended callers
      int sp = MSP_DEPTH(msp);
      for (;;) {
        CTR_MARK(52);  // unwind one level
        if (sp == 0) {
          if constexpr (SS) {
            // parked, not stored: the sample's colour waits in the lane's own frame 0 (free from here on; A.frames >= 1)
            // for the reduction after the loop, where the wave has reconverged.  MSP_DONE | 1: "this lane has a sample"
            STK(0, F_R) = out_rgb.x; STK(0, F_G) = out_rgb.y; STK(0, F_B) = out_rgb.z;
            msp = MSP_DONE | 1u;
          } else {
            const size_t px_id = px_index();
            store3(((const CADDR KParams *)AK)->color_out, px_id, out_rgb);
            msp = MSP_DONE;
          }
          break;
        }
        CTR_MARK(53);
        --sp;
        V3 rgb = mk(STK(sp, F_R), STK(sp, F_G), STK(sp, F_B));
        const uint32_t f_mat = __float_as_uint(STK(sp, F_MAT));
        const CADDR DMat &FM = k_mats[f_mat & 0x3FFFFFFFu];
        if constexpr (OPAQUE) {
          // every frame waits for its reflection child (stage 1), and no material transmits: shading.hpp:138 alone
          out_rgb = vadd(rgb, vscale(out_rgb, FM.reflexivity));
          continue;
        }
        const float f_transl = FM.transparency;
        if ((f_mat >> 30) == 1u) {
          CTR_MARK(97);
          rgb = vadd(rgb, vscale(out_rgb, FM.reflexivity));  // shading.hpp:138
          if ((double)f_transl >= 1e-6) {
            CTR_MARK(98);
            STK(sp, F_R) = rgb.x; STK(sp, F_G) = rgb.y; STK(sp, F_B) = rgb.z;
            STK(sp, F_MAT) = __uint_as_float((f_mat & 0x3FFFFFFFu) | (2u << 30));
            in_d = mk(STK(sp, F_DX), STK(sp, F_DY), STK(sp, F_DZ));
            ro = mk(STK(sp, F_PX), STK(sp, F_PY), STK(sp, F_PZ));
            rd = in_d;
            msp = (uint32_t)(sp + 1);  // the frame stays; a radiance cast
            min_t = A.fudge;
            break;
          }
          out_rgb = rgb;
        } else {
          CTR_MARK(99);
          // shading.hpp:148
          out_rgb = vadd(vscale(rgb, 1.0f - f_transl), vscale(out_rgb, f_transl));
        }
      }
    }
    if (K != TRIP_SHADOW && first_trip) {  // (the first trip is a radiance trip)
      // max finite depth of the tile, reduced once here instead of carrying the depth to the end
      CTR_MARK(54);
      uint32_t dbits = (__builtin_isfinite(first_depth) && first_depth > 0.f) ? __float_as_uint(first_depth) : 0u;
      if constexpr (SS) dbits = ss_kept() ? dbits : 0u;  // the maximum of the depth buffer that is returned
      for (int off = 32; off > 0; off >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)dbits, off);
        dbits = o > dbits ? o : dbits;
      }
      wave_dbits = __builtin_amdgcn_readfirstlane(dbits);
      first_trip = false;
    }
    TSTAMP(t_cont1);
    TACC(8, t_cont_mid, t_cont1);
    CTR_MARK(55);
    if constexpr (K == TRIP_ANY) li = li_k;
    else phase_lights = k_n_light;
