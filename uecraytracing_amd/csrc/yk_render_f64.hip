// yk_render_f64.hip — the FP64 path kernel (yk_render_persistent, and yk_render_counting with the
// work counters): the execution model is described at the top of yk_pipeline.hip.
#include "yk_path.hpp"
#ifdef YK_DRAIN_DIAG
#include <algorithm>
#include <vector>
#endif

namespace {

// Diagnostic builds (YK_DRAIN_DIAG, tools/drain_probe.py): every FP64 render wave records when it
// starts and when it leaves the loop (s_memrealtime, 100 MHz) and where it ran (HW_ID, XCC_ID), per
// launch of the call: the per-launch drain — waves idle in a workgroup that still holds its CU,
// CUs between one launch's workgroup and the next — measured, not modelled
#ifdef YK_DRAIN_DIAG
constexpr uint32_t kDiagLaunches = 64, kDiagBlocks = 512, kDiagWaves = 16;
// per wave: {start, end, HW_ID | XCC_ID << 32}
__device__ unsigned long long yk_wave_times[kDiagLaunches * kDiagBlocks * kDiagWaves * 3];
#define YK_WAVE_STAMP(ka, k)                                                                          \
  do {                                                                                                \
    const uint32_t w_ = threadIdx.x >> 6;                                                             \
    if ((threadIdx.x & 63u) == 0 && (ka).diag_c < kDiagLaunches && blockIdx.x < kDiagBlocks) {        \
      unsigned long long* r_ =                                                                        \
          yk_wave_times + (((size_t)(ka).diag_c * kDiagBlocks + blockIdx.x) * kDiagWaves + w_) * 3;     \
      r_[(k)] = __builtin_amdgcn_s_memrealtime();                                                     \
      if ((k) == 0)                                                                                   \
        r_[2] = (unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 4) |                       \
                ((unsigned long long)__builtin_amdgcn_s_getreg((3 << 11) | 20) << 32);                \
    }                                                                                                 \
  } while (0)
#else
#define YK_WAVE_STAMP(ka, k) ((void)0)
#endif

// The reference's closest-hit scan verbatim (hittable_list.hpp:32-58 over sphere.hpp:25-48):
// tuple order, t_max shrinking to the last accepted root.  Used for rays the BVH cannot serve
// (degenerate direction, origin beyond the proven float range, candidate-list overflow) and,
// with kFlagLinearScan, as the A/B reference of the BVH path.
__device__ __noinline__ Hit scan_linear(const SphereGeo* __restrict__ geo, uint32_t n, v3 o, v3 d,
                                        double tmin) {
  const double a = ykd::len2(d);
  Hit h{INFINITY, -1, 0, 0, 0, 0};
  for (uint32_t i = 0; i < n; ++i) {
    const SphereGeo sg = geo[i];
    ++h.tests;
    const v3 oc = {o.x - sg.cx, o.y - sg.cy, o.z - sg.cz};
    const double hb = ykd::dot(oc, d);
    const double c = ykd::len2(oc) - sg.rr;
    const double disc = hb * hb - a * c;
    if (disc < 0) continue;
    ++h.sqrts;
    const double sq = ykd::nsqrt_c(disc, h.ncalls, h.nits);
    double root = (-hb - sq) / a;
    if (root < tmin || h.T < root) {
      root = (-hb + sq) / a;
      if (root < tmin || h.T < root) continue;
    }
    h.T = root;
    h.hid = (int)i;
  }
  return h;
}

__device__ __forceinline__ float safe_rcp(float x) {
  return fabsf(x) > 1e-30f ? 1.0f / x : copysignf(1e30f, x);
}

// n / a for a root (sphere.hpp:36-38), a's refined reciprocal shared by all candidates; a wave
// with any lane out of range takes the full division (divs_fast's rule)
__device__ __forceinline__ double root_div(double n, double a, double ra, bool a_ok) {
  double q = ykd::div_by(n, a, ra);
  if (__builtin_expect(__ballot(!(a_ok && ykd::num_range(n))) != 0, 0)) q = n / a;
  return q;
}
// Exact value of sphere i's root under the reference's acceptance rule, ignoring t_max
// (sphere.hpp:35-39): root1 if root1 >= t_min, else root2 if root2 >= t_min, else none — from the
// candidate's hb and disc (the reference's, bit for bit)
__device__ __forceinline__ void exact_root(uint32_t i, double hb, double disc, double a, double ra, bool a_ok,
                                           double tmin, Hit& best) {
  if (disc < 0) return;  // never taken: the candidate passed the same test
  ++best.sqrts;
  const double sq = ykd::nsqrt_c(disc, best.ncalls, best.nits);
  double r = root_div(-hb - sq, a, ra, a_ok);
  if (r < tmin) {
    r = root_div(-hb + sq, a, ra, a_ok);
    if (r < tmin) return;
  }
  // closest wins; an exact tie goes to the later tuple index (hittable_list.hpp:36-43)
  if (r < best.T || (r == best.T && (int)i > best.hid)) {
    best.T = r;
    best.hid = (int)i;
  }
}
// ... of a candidate whose hb and disc were not kept from its leaf test
__device__ __forceinline__ void exact_candidate(const SphereGeo* __restrict__ geo, uint32_t i,
                                                v3 o, v3 d, double a, double ra, bool a_ok,
                                                double tmin, Hit& best) {
  const SphereGeo sg = geo[i];
  const v3 oc = {o.x - sg.cx, o.y - sg.cy, o.z - sg.cz};
  const double hb = ykd::dot(oc, d);
  const double c = ykd::len2(oc) - sg.rr;
  const double disc = hb * hb - a * c;
  exact_root(i, hb, disc, a, ra, a_ok, tmin, best);
}

// kSceneInLds: the BVH nodes, the leaf-ordered sphere geometry and the leaf→tuple ids are copied
// into LDS by each workgroup once (33 KB for the 485-sphere scene), so a node visit is four
// ds_read_b128 instead of four dependent L2 round trips.  Larger scenes read them from global.

// kCount: the work counters of YK_FLAG_COUNT_WORK (an instance of its own, so the production
// instance carries neither their registers nor their adds)
// kMode bit 0: the work counters; bit 1: YK_SEED_RANDOM_DEVICE seeding (an instance of its own:
// the hash's 64-bit arithmetic and two more kernel arguments cost the counter-seeded production
// instance 0.6% through SGPR spills); bit 2: the yk::xor128 engine (YK_RNG_XOR128)
template <bool kSceneInLds, int kMode>
__device__ __forceinline__ void render_body(KernelArgs ka) {
  constexpr int kBlk = mode_block<kMode>();
  constexpr bool kCount = (kMode & 1) != 0;
  constexpr bool kRandomSeed = (kMode & 2) != 0;
  using Gen = typename std::conditional<(kMode & 4) != 0, ykd::X128Lane, ykd::MtLane>::type;
  const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63u;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const char* __restrict__ nodes = (const char*)ka.nodes;
  const SphereGeo* __restrict__ leaf_geo = ka.leaf_geo;
  const uint32_t* __restrict__ leaf_ids = ka.leaf_ids;
  const SphereGeo* __restrict__ geo = ka.geo;  // tuple order: candidates' roots, hit records
  const SphereMat* __restrict__ mat = ka.mat;  // shading, attenuation unwind
  if (kSceneInLds) {
    // the BVH, its leaf geometry and ids, and (tuple order) the geometry and materials
    const uint4* src[5] = {(const uint4*)ka.nodes, (const uint4*)ka.leaf_geo, (const uint4*)ka.leaf_ids,
                           (const uint4*)ka.geo, (const uint4*)ka.mat};
    const uint32_t off[5] = {0u, ka.lds_geo_off, ka.lds_ids_off, ka.lds_tgeo_off, ka.lds_mat_off};
    const uint32_t n16[5] = {(ka.n_nodes * (uint32_t)sizeof(DevNode) + 15u) / 16u, ka.nspheres * 2u,
                             (ka.nspheres + 3u) / 4u, ka.nspheres * 2u, ka.nspheres * 4u};
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      uint4* dst = (uint4*)(smem + off[k]);
      for (uint32_t i = threadIdx.x; i < n16[k]; i += kBlk) dst[i] = src[k][i];
    }
    __syncthreads();
    nodes = smem;
    // the child-code reads address the LDS copy from 0: the dynamic region must start there
    if ((uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)smem != 0u) __builtin_trap();
    leaf_geo = (const SphereGeo*)(smem + ka.lds_geo_off);
    leaf_ids = (const uint32_t*)(smem + ka.lds_ids_off);
    geo = (const SphereGeo*)(smem + ka.lds_tgeo_off);
    mat = (const SphereMat*)(smem + ka.lds_mat_off);
  }
  int32_t* const stk = (int32_t*)(smem + ka.lds_stack_off) + threadIdx.x;  // [sp * kBlk]
  // YK_FLAG_ONE_LANE (counting instance only): lanes 1..63 leave here, after the block's last
  // barrier, so every wave-instruction below is one lane's (the profiler's per-wave FP64 counters
  // then count that lane's executed operations exactly: DESIGN.md §5)
  if (kCount && (ka.flags & kFlagOneLane) && lane != 0) return;
  stk[0] = ykbvh::kEmptyLeaf;  // the sentinel below every traversal's entries
  // the warm-up waves sharing the SIMDs (priority 0) get only the issue slots the render leaves
  __builtin_amdgcn_s_setprio(1);
  YK_CLOCK_BEGIN(ka);
  YK_WAVE_STAMP(ka, 0);

  Gen g;
  rng_init(g, ka, gid);
  uint16_t* const id_spill = ka.id_scratch + (size_t)gid * ka.id_stride;

  uint32_t n_seg = 0, n_test = 0, n_sqrt = 0, n_fb = 0, n_node = 0, n_lin = 0, n_ncall = 0, n_nit = 0;
  uint32_t n_dpos = 0;  // leaf tests with disc >= 0 (their root bounds are computed)
  uint32_t n_lamb = 0, n_metal = 0, n_fuzz = 0, n_diel = 0;  // hits shaded per material kind
  // engine words drawn (the warm-up's start words among them) and scratch-engine twists
  uint32_t n_words = 0, n_swords = 0, n_twist = 0;

  YK_STAMPS_BEGIN(ka.counters, lane);
  uint32_t slot = 0, depth = 0, nstk = 0;
  uint32_t st0 = 0, st1 = 0, st2 = 0, st3 = 0;  // newest attenuation id in st0's low half
  v3 o = {0, 0, 0}, d = {0, 0, 0};
  bool in_path = false;
  // wave-level reserve of claimed sample slots (identical in every lane of the wave)
  uint32_t res_base = 0, res_left = 0;

  for (;;) {
    // ---- refill (claim_slots): lanes without a path take the next sample slots
    if (claim_slots(ka, in_path, lane, slot, res_base, res_left)) {
      YK_STAMPS_EXHAUSTED(ka.counters);
      break;
    }
    YK_STAMP(0);

    // ---- start sample s of the pixel: seed, jitter, camera ray (source.cpp:154-165) ------
    bool start = !in_path;
    // mt19937: the slot's StartRec, its four loads issued together and waited for once (every
    // slot of the launch, empty ones included, has a record, so the read is in bounds); it says
    // whether the slot is empty (kPadSlot) and holds the whole start, so neither the processing
    // order nor the pixel's seed is read here — the scratch engine recovers the seed from its
    // cursor (mt_slow).  xor128: the slot's pixel
    uint4 rq0 = {0, 0, 0, 0}, rq1 = {0, 0, 0, 0}, rq2 = {0, 0, 0, 0}, rq3 = {0, 0, 0, 0};
    uint32_t qpix = 0;
    if (start) {
      if constexpr (std::is_same<Gen, ykd::MtLane>::value) {
        const uint4* rp = (const uint4*)ka.start + 4u * slot;
        rq0 = rp[0];
        rq1 = rp[1];
        rq2 = rp[2];
        rq3 = rp[3];
        asm volatile("" ::"v"(rq0.x), "v"(rq0.y), "v"(rq0.z), "v"(rq0.w), "v"(rq1.x), "v"(rq1.y),
                     "v"(rq1.z), "v"(rq1.w), "v"(rq2.x), "v"(rq2.y), "v"(rq2.z), "v"(rq2.w), "v"(rq3.x),
                     "v"(rq3.y), "v"(rq3.z), "v"(rq3.w));
        start = rq3.w != kPadSlot;  // an empty slot of an edge block: take another next trip
      } else {
        const uint32_t sl = fdiv(slot, ka.nps_m, ka.nps_sh);
        qpix = ka.order[slot - sl * ka.npix_slots];
        start = qpix != kNoPixel;
      }
    }
    if (start) {
      // The start — the jitter canonicals, the lens point and the camera ray — and the engine
      // after its draws: precomputed for mt19937 by yk_mt_warmup (StartRec), so the divergent
      // loop only loads them; xor128, and the (never seen) record the warm-up could not
      // complete, start here
      bool pre = false;
      if constexpr (std::is_same<Gen, ykd::MtLane>::value) {
        StartRec r;  // (loaded above)
        __builtin_memcpy((char*)&r, &rq0, 16);
        __builtin_memcpy((char*)&r + 16, &rq1, 16);
        __builtin_memcpy((char*)&r + 32, &rq2, 16);
        __builtin_memcpy((char*)&r + 48, &rq3, 16);
        pre = r.j != kNoStart;
        if (pre) {
          if (kCount) n_swords += r.j;
          g.a0 = r.a0;
          g.a1 = r.a1;
          g.b = r.b;
          g.j = r.j;
          o = v3{r.ox, r.oy, r.oz};
          d = v3{r.dx, r.dy, r.dz};
        }
      }
      if (!pre) {
        // the pixel and its seed (uint32 wrap, source.cpp:154-158)
        const uint32_t sl = fdiv(slot, ka.nps_m, ka.nps_sh);
        if constexpr (std::is_same<Gen, ykd::MtLane>::value) qpix = ka.order[slot - sl * ka.npix_slots];
        const uint32_t s = ka.s0 + sl;
        const uint32_t tr = fdiv(qpix, ka.w_m, ka.w_sh);
        const uint32_t x = tile_col_x(ka.col_begin, ka.col_stride, ka.col_band, qpix - tr * ka.Wt);
        const uint32_t y = tile_row_y(ka.row_begin, ka.row_stride, ka.band_log2, tr);
        const uint32_t seed = ykd::sample_seed(kRandomSeed ? 1u : 0u, ka.seed_key, ka.seed0, y, x, ka.W, ka.spp, s);
        const bool lens = ka.cam.lens_radius > 0;
        rng_start_full(g, seed);
        const double uc = ykd::canonical<true>(g);  // (a fresh engine: its first words never need the scratch engine)
        const double vc = ykd::canonical<true>(g);
        double px = 0, py = 0;
        if (lens) {  // thin-lens extension: random_in_unit_disk by rejection
          do {
            px = ykd::uniform(g, -1, 1);
            py = ykd::uniform(g, -1, 1);
          } while (!(px * px + py * py < 1.0));
        }
        camera_ray(ka.cam, ka.w_d, ka.inv_w, ka.h_d, ka.inv_h, ka.H, x, y, uc, vc, lens, px, py, o, d);
      }
      depth = ka.max_depth;
      nstk = 0;
      in_path = true;
    }
    YK_STAMP(1);
    // ray_color prints its ray before the depth test (raytracer.hpp:21-25)
    if (kCount && (ka.flags & kFlagTrace) && in_path) trace_ray(ka, slot, ka.max_depth - depth, o, d);

    // ---- one segment of ray_color (raytracer.hpp:19-37) ----------------------------------
    // (a) closest hit: hittable_list::hit_impl (hittable_list.hpp:32-58) over
    //     sphere::hit_impl (sphere.hpp:25-48): tuple order, t_max shrinking to the last
    //     accepted root, so the closest hit wins and an exact tie goes to the later sphere.
    // depth == 0 → black (raytracer.hpp:23); lanes without a path (empty slot) sit this out
    const bool alive = in_path && depth != 0;
    Hit hit{INFINITY, -1, 0, 0, 0, 0};
    if (alive) {
      ++n_seg;
      const double a = ykd::len2(d);
      const double onorm = fmax(fabs(o.x), fmax(fabs(o.y), fabs(o.z)));
      bool linear = (ka.flags & kFlagLinearScan) || !(a > 0 && a < INFINITY) ||
                    !(onorm <= ka.origin_bound);
      if (!linear) {
        // BVH traversal: cull conservatively, keep every sphere whose exact root could be
        // the minimum.  Slab distances as one FMA each,
        // t = lo*(1/d) - o*(1/d): error relative 2^-22 plus an origin perturbation of
        // 2^-23|o| (< delta/4), inside the culling contract of yk_bvh.hpp.  This is culling
        // arithmetic only, so explicit FMAs are fine here.
        // 1/d from v_rcp_f32 (1 ulp): with d's rounding to float and the FMA's rounding the
        // slab distances stay within the 2^-22 relative error the culling contract assumes
        // (2^-24 + 2^-23 + 2^-24).  Components outside [1e-30, 1e30] (never seen) take the
        // correctly rounded division for the whole wave.
        const float dxf = (float)d.x, dyf = (float)d.y, dzf = (float)d.z;
        const float dmin = fminf(fminf(fabsf(dxf), fabsf(dyf)), fabsf(dzf));
        const float dmax = fmaxf(fmaxf(fabsf(dxf), fabsf(dyf)), fabsf(dzf));
        float ix, iy, iz;
        if (__ballot(!(dmin > 1e-30f && dmax < 1e30f)) == 0) {
          ix = __builtin_amdgcn_rcpf(dxf);
          iy = __builtin_amdgcn_rcpf(dyf);
          iz = __builtin_amdgcn_rcpf(dzf);
        } else {
          ix = safe_rcp(dxf);
          iy = safe_rcp(dyf);
          iz = safe_rcp(dzf);
        }
        const float oix = (float)o.x * ix, oiy = (float)o.y * iy, oiz = (float)o.z * iz;
        // this ray's (near x4, far x4) plane quads inside a WideNode (yk_bvh.hpp), as base
        // pointers: a visit then costs one address add per axis
        const char* const px = nodes + (ix < 0.0f ? 16u : 0u);
        const char* const py = nodes + 48u + (iy < 0.0f ? 16u : 0u);
        const char* const pz = nodes + 96u + (iz < 0.0f ? 16u : 0u);
        // Conservative interval test without per-visit relaxation: far distances
        // come out of the FMA already scaled by c = 1 + 2^-17 (scaled 1/d and o/d), near
        // distances are compared unscaled against tmin_lo = t_min (1 - 2^-17) and against
        // ustar_f (U* (1 + 2^-18)).  A box passes iff
        //   max(tn, tmin_lo) <= min(tf * c, ustar_f),
        // which holds whenever the former test with both distances relaxed by 2^-20 held.
        constexpr float kFar = 1.0f + 0x1p-17f;
        // scaled far terms: ONE rounding of the origin product, as for the near terms, so the
        // origin perturbation stays within delta/4 (yk_bvh.hpp); the rounding of ix*c is a
        // relative error inside the 2^-17 margin
        const float ixs = ix * kFar, iys = iy * kFar, izs = iz * kFar;
        const float ox_f = (float)o.x, oy_f = (float)o.y, oz_f = (float)o.z;
        const float tmin_lo = __double2float_rd(ka.t_min) * (1.0f - 0x1p-17f);
        // Distances measured from tmin_lo and scaled by kClampScale = 2^-24: per
        // axis (s/d, s(-o/d - tmin_lo)) (near) and (sc/d, s(-oc/d - tmin_lo)) (far).  The near
        // FMAs clamp to [0, 1], which IS the max with tmin_lo (distances below 2^24 + tmin_lo
        // never reach the clamp's 1; beyond, the clamp only lowers a near distance: more boxes
        // kept, never fewer), so a slot costs max3 + min3 + min + compare.  s is a power of two
        // (exact), the constants' subtraction one more rounding of the origin term
        // (<= 2^-24 (|o/d| + t_min): inside the delta budget with the origin perturbation).
        constexpr float kS = kClampScale;
        const f2 sxp = {ix * kS, (-oix - tmin_lo) * kS}, syp = {iy * kS, (-oiy - tmin_lo) * kS},
                 szp = {iz * kS, (-oiz - tmin_lo) * kS};
        const f2 fxp = {ixs * kS, (-(ox_f * ixs) - tmin_lo) * kS}, fyp = {iys * kS, (-(oy_f * iys) - tmin_lo) * kS},
                 fzp = {izs * kS, (-(oz_f * izs) - tmin_lo) * kS};
        const double ia = ykd::rcp_bound(a);  // bounds only: relative error < 2^-44
        double ustar = INFINITY;  // proven upper bound of the minimum exact root
        float ustar_f = INFINITY;  // >= ustar * (1 + 2^-18) (clamped distances: >= s (that - tmin_lo))
        // a lane whose 1/d could leave float's normal range once scaled (|d| >= 1e30, never seen)
        // is marked for the exact linear scan from the start (nc = 5, as an overflow)
        // the candidates' tuple ids as 16-bit halves (ids are < 2^16: ykgpu_set_scene's limit),
        // entry 0 in cp01's low half
        uint32_t nc = dmax < 1e30f ? 0u : 5u, cp01 = 0, cp23 = 0;
        // hb and disc of entry 0 (always the newest candidate: a compaction is followed by the
        // insertion that caused it), so its exact root needs no second discriminant
        double hb0 = 0, disc0 = 0;
        // candidate lower bounds kept as floats RN(L), compared with ustar_f >= RN(U*): by
        // monotone rounding (all bounds >= 0) L <= U* implies RN(L) <= ustar_f, so the float
        // comparison only ever keeps MORE candidates than the double comparison would
        float l0 = 0, l1 = 0, l2 = 0, l3 = 0;
        // overflow of the stack or of the candidate list is recorded as nc = 5, not as a flag of
        // its own: a bool carried round the traversal loop lives in a lane mask that every
        // divergent exit has to merge (-3.4% as a bool), an integer flag is one more loop-carried
        // register (nc = 5 instead: -0.8%)
        int32_t node = ka.bvh_root;
        // this lane's traversal stack as LDS byte addresses (entries kBlk words apart).  `top` holds
        // the address of the entry BELOW the top, kTopOff less than the top's (at the start: the
        // sentinel's), so the visit's read of that entry and the pushes at the top take constant
        // DS offsets.  (The expressions below spell the top's address less kTopOff out: the
        // compiler schedules two instances differently when they are folded by hand.)
        constexpr uint32_t kTopOff = kBlk * 4u;
        const uint32_t stk_b = (uint32_t)(uintptr_t)stk;
        uint32_t top = stk_b + kBlk * 4u - kTopOff;
        const uint32_t stk_cap = stk_b + ka.stack_cap * kBlk * 4u - kTopOff;
#define YK_STK(a) (*(__attribute__((address_space(3))) int32_t*)(uintptr_t)(a))
        for (;;) {
          if (node >= 0) {
           // the lane's run of interior nodes as a loop of its own tested at the bottom: its exit
           // value is the visit's own result, so the compiler keeps node / top / nc in place
           do {
            if (kCount) ++n_node;
            YK_STAMP_NODE_ITERATION(lane);
            // the entry below the top (the sentinel when the stack holds nothing), read with the
            // planes: the pushes below write at and above the top, never here
            const int32_t popped = YK_STK(top + kTopOff - kBlk * 4u);
            // near / far distances of the 4 slots per axis, one packed FMA per pair of slots:
            // t = plane*(1/d) - o*(1/d), the binary node's arithmetic per slot
            const f4 qnx = *(const f4*)(px + node), qfx = *(const f4*)(px + node + 16);
            const f4 qny = *(const f4*)(py + node), qfy = *(const f4*)(py + node + 16);
            const f4 qnz = *(const f4*)(pz + node), qfz = *(const f4*)(pz + node + 16);
            // the scene's LDS copy starts at LDS address 0 (the kernel's only LDS is the dynamic
            // region, checked at the kernel's start), so the child codes of node n sit at n + 144
            int4 ch;
            if (kSceneInLds) {
              typedef int i4v __attribute__((ext_vector_type(4)));
              const i4v c4 = *(__attribute__((address_space(3))) const i4v*)(uintptr_t)((uint32_t)node + 144u);
              ch = make_int4(c4.x, c4.y, c4.z, c4.w);
            } else {
              ch = *(const int4*)(nodes + node + 144);
            }
            bool hk[4];
            const f2 nx[2] = {slab_fma_clamp(qnx.xy, sxp), slab_fma_clamp(qnx.zw, sxp)};
            const f2 fx[2] = {slab_fma(qfx.xy, fxp), slab_fma(qfx.zw, fxp)};
            const f2 ny[2] = {slab_fma_clamp(qny.xy, syp), slab_fma_clamp(qny.zw, syp)};
            const f2 fy[2] = {slab_fma(qfy.xy, fyp), slab_fma(qfy.zw, fyp)};
            const f2 nz[2] = {slab_fma_clamp(qnz.xy, szp), slab_fma_clamp(qnz.zw, szp)};
            const f2 fz[2] = {slab_fma(qfz.xy, fzp), slab_fma(qfz.zw, fzp)};
#pragma unroll
            for (int h = 0; h < 2; ++h) {
              float tna, tfa, tnb, tfb;
              slab_cull2c(nx[h][0], ny[h][0], nz[h][0], fx[h][0], fy[h][0], fz[h][0], nx[h][1], ny[h][1], nz[h][1],
                          fx[h][1], fy[h][1], fz[h][1], ustar_f, tna, tfa, tnb, tfb);
              hk[2 * h] = tna <= tfa;
              hk[2 * h + 1] = tnb <= tfb;
            }
            // keep the child-code read in this block, issued with the plane reads (the compiler
            // would otherwise sink it into the branch below and wait for it there)
            asm volatile("" ::"v"(ch.x), "v"(ch.y), "v"(ch.z), "v"(ch.w));
            {
              // the last slot entered is visited next, the others entered are pushed in slot
              // order; none entered: the popped entry is next and the top moves down one
              const bool any = hk[0] || hk[1] || hk[2] || hk[3];
              node = hk[3] ? ch.w : (hk[2] ? ch.z : (hk[1] ? ch.y : (hk[0] ? ch.x : popped)));
              YK_STK(top + kTopOff) = ch.x;
              top += (hk[0] && (hk[1] || hk[2] || hk[3])) ? kBlk * 4u : 0u;
              YK_STK(top + kTopOff) = ch.y;
              top += (hk[1] && (hk[2] || hk[3])) ? kBlk * 4u : 0u;
              YK_STK(top + kTopOff) = ch.z;
              top += (hk[2] && hk[3]) ? kBlk * 4u : (any ? 0u : 0u - kBlk * 4u);
              // stack full: the top stays at the capacity and nc = 5 sends the lane to the scan
              // (only where the plan could not give the stack its proven depth: ka.stack_check)
              if (ka.stack_check) {
                asm volatile("");  // (a scalar branch: no selects on the uniform flag)
                // signed: the pop of the sentinel leaves `top` (the entry below the top) one entry below the
                // stack's base, below LDS address 0 for the low lanes of a scene with a small LDS
                // copy (unsigned, that wrapped past the capacity and the lane never left the loop)
                nc = (int32_t)top > (int32_t)stk_cap ? 5u : nc;
                top = (int32_t)top > (int32_t)stk_cap ? stk_cap : top;
              }
            }
           } while (node >= 0);
          }
          {
            YK_STAMP(2);  // interior nodes since the last stamp
            const uint32_t v = ~(uint32_t)node, first = v >> 4, cnt = v & 15u;
            // the FP64 tree has one sphere per leaf (max_leaf = 1: the builder's median fallback
            // never leaves more), so a leaf is tested without a loop (512 spp: -0.9%); the empty
            // leaf ~0 (cnt 0) tests nothing.  (`continue` inside the do-while(0) leaves the test.)
            static_assert(kLeafCapF64 == 1, "the FP64 leaf test handles one sphere");
            if (cnt != 0) do {
              const uint32_t k = 0;
              const SphereGeo sg = leaf_geo[first + k];
              // the tuple index read with the geometry: its latency then hides under the
              // discriminant instead of following the bounds on the insert path
              const uint32_t id = leaf_ids[first + k];
              asm volatile("" ::"v"(id));
              ++n_test;
              // the reference's discriminant, bit for bit (sphere.hpp:29-34)
              const v3 oc = {o.x - sg.cx, o.y - sg.cy, o.z - sg.cz};
              const double hb = ykd::dot(oc, d);
              const double c = ykd::len2(oc) - sg.rr;
              const double disc = hb * hb - a * c;
              if (disc < 0) continue;
              if (kCount) ++n_dpos;
              YK_STAMP_DISC_POS();
              // bounds of the exact root: |approx - exact| <= m (256x the error bound, §4)
              const double sq = ykd::sqrt_bound(disc);
              const double r1 = (-hb - sq) * ia, r2 = (-hb + sq) * ia;
              const double m = (fabs(hb) + sq) * ia * 0x1p-34 + 0x1p-1000;
              if (r2 + m < ka.t_min) continue;  // both roots certainly behind t_min
              const double lb = fmax(ka.t_min, r1 - m);
              const double ub = (r1 - m >= ka.t_min) ? r1 + m : ((r2 - m >= ka.t_min) ? r2 + m : INFINITY);
              if (!(lb <= ustar)) continue;
              if (ub < ustar) {
                ustar = ub;
                // s (RN(ub)(1 + 2^-18) - tmin_lo), rounded up by the factor 1 + 2^-22: >= s (the
                // unshifted bound - tmin_lo), positive (ub >= t_min > tmin_lo)
                ustar_f = ((float)ub * (1.0f + 0x1p-18f) - tmin_lo) * ((1.0f + 0x1p-22f) * kClampScale);
              }
              if (nc == 4) {  // compact: drop entries the new bound has excluded
                uint32_t m2 = 0;
                uint32_t c0 = 0, c1 = 0, c2 = 0, c3 = 0;
                const uint32_t d0 = cp01 & 0xffffu, d1 = cp01 >> 16, d2 = cp23 & 0xffffu, d3 = cp23 >> 16;
                float e0 = l0, e1 = l1, e2 = l2, e3 = l3;
                if (e0 <= ustar_f) { YK_CAND_SET(m2, d0, e0); ++m2; }
                if (e1 <= ustar_f) { YK_CAND_SET(m2, d1, e1); ++m2; }
                if (e2 <= ustar_f) { YK_CAND_SET(m2, d2, e2); ++m2; }
                if (e3 <= ustar_f) { YK_CAND_SET(m2, d3, e3); ++m2; }
                nc = m2;
                cp01 = c0 | (c1 << 16);
                cp23 = c2 | (c3 << 16);
              }
              if (nc < 4) {
                // shifted in at entry 0 — straight-line moves instead of a branch per list
                // position (evaluation order never matters: min root, later index on ties).
                // RN(lb), not rounded down: t_min >= 0 (checked by the host) makes every lb and
                // U* >= 0, and lb <= U* implies RN(lb) <= RN(U*) <= ustar_f (monotone rounding),
                // so the list still keeps every sphere that can be the minimum
                cp23 = __builtin_amdgcn_alignbit(cp23, cp01, 16u);  // (cp23 << 16) | (cp01 >> 16)
                cp01 = (cp01 << 16) | id;
                l3 = l2, l2 = l1, l1 = l0;
                hb0 = hb, disc0 = disc;
                // the same monotone map as ustar_f's: s RN(RN(lb) - tmin_lo) (one FMA, s a power of
                // two), so lb <= U* still implies l0 <= ustar_f
                l0 = __builtin_fmaf((float)lb, kClampScale, -tmin_lo * kClampScale);
                ++nc;
              } else {
                nc = 5;  // the list is full: overflow (the exact linear scan decides)
              }
            } while (0);
            YK_STAMP(6);  // this leaf
          }
          if (top + kTopOff <= stk_b + kBlk * 4u) break;  // only the sentinel left, or the sentinel just visited
          top -= kBlk * 4u;
          node = YK_STK(top + kTopOff);
#undef YK_STK
        }
        YK_STAMP(2);
        if (nc > 4) {
          linear = true;
        } else {
          // exact evaluation of the survivors; the roots' divisor a is the same for every
          // candidate of a ray, so its refined reciprocal is computed once
          const bool a_ok = ykd::div_range(a);
          const double ra = (nc > 0 && a_ok) ? ykd::rcp_refined(a) : 0.0;
          const uint32_t c0 = cp01 & 0xffffu, c1 = cp01 >> 16, c2 = cp23 & 0xffffu, c3 = cp23 >> 16;
          if (nc > 0 && l0 <= ustar_f) exact_root(c0, hb0, disc0, a, ra, a_ok, ka.t_min, hit);
          if (nc > 1 && l1 <= ustar_f) exact_candidate(geo, c1, o, d, a, ra, a_ok, ka.t_min, hit);
          if (nc > 2 && l2 <= ustar_f) exact_candidate(geo, c2, o, d, a, ra, a_ok, ka.t_min, hit);
          if (nc > 3 && l3 <= ustar_f) exact_candidate(geo, c3, o, d, a, ra, a_ok, ka.t_min, hit);
        }
      }
      if (linear) {
        hit = scan_linear(ka.geo, ka.nspheres, o, d, ka.t_min);
        n_test += hit.tests;
        ++n_lin;
      }
      n_sqrt += hit.sqrts;
      n_ncall += hit.ncalls;
      n_nit += hit.nits;
    }
    YK_STAMP(3);

    // (b) shade, material-uniform: every operation more than one material needs runs ONCE for all
    //     the lanes that need it, instead of once per material branch (a wave holds every kind
    //     almost every trip, so per-branch copies run one after the other):
    //   * one block of canonicals: lambertian's vec3::random (3), the fuzzed metal's length factor
    //     and vector (4), the dielectric's reflect-or-refract uniform (1, drawn speculatively:
    //     given back when total internal reflection means the reference never draws it);
    //   * one vector normalisation — the sky's normalized(dir) (raytracer.hpp:35), lambertian's
    //     random_unit_vector (material.hpp:33-36), metal's / dielectric's normalized(dir);
    //   * one more Newton square root: the fuzzed metal's |vector| or the dielectric's sin(theta).
    //   Each lane's own operations and their order are the reference's.
    bool ended = in_path && !alive;
    double L_r = 0, L_g = 0, L_b = 0;
    if (alive) {
      const int hid = hit.hid;
      const double T = hit.T;
      SphereGeo sg{0, 0, 0, 0};
      SphereMat m{};
      v3 p{0, 0, 0}, nrm{0, 0, 0};
      bool front = false;
      if (hid >= 0) {
        sg = geo[hid];
        m = mat[hid];
        // hit record (sphere.hpp:41-45, hittable.hpp:23-27)
        p = ykd::add(o, ykd::mul(d, T));
        const v3 outward = ykd::divs_fast_r(ykd::sub(p, v3{sg.cx, sg.cy, sg.cz}), m.radius, m.inv_r);
        front = ykd::dot(d, outward) < 0;
        nrm = front ? outward : ykd::neg(outward);
      }
      const bool lamb = hid >= 0 && m.kind == YK_MATERIAL_LAMBERTIAN;
      const bool fuzzy = hid >= 0 && m.kind == YK_MATERIAL_METAL && m.fuzz > 0;
      const bool diel = hid >= 0 && m.kind == YK_MATERIAL_DIELECTRIC;
      const bool spec = diel && ykd::rng_can_speculate(g);
      const Gen saved = g;  // the dielectric's engine before its speculative draw
      const uint32_t ncan = lamb ? 3u : (fuzzy ? 4u : (spec ? 1u : 0u));
      double c0 = 0, c1 = 0, c2 = 0, c3 = 0;
      if (__ballot(ncan > 0 && !ykd::rng_lazy_ok(g, 2 * ncan)) == 0) {
        // (almost always) no lane of the wave reaches the scratch engine's words: no checks
        if (ncan > 0) c0 = ykd::canonical<true>(g);
        if (ncan > 1) c1 = ykd::canonical<true>(g);
        if (ncan > 2) c2 = ykd::canonical<true>(g);
        if (ncan > 3) c3 = ykd::canonical<true>(g);
      } else {
        if (ncan > 0) c0 = ykd::canonical(g);
        if (ncan > 1) c1 = ykd::canonical(g);
        if (ncan > 2) c2 = ykd::canonical(g);
        if (ncan > 3) c3 = ykd::canonical(g);
      }
      // lambertian: vec3::random(gen, -1, 1), x then y then z (vec3.hpp:134-142); fuzzed metal:
      // random(-1,1).normalize() * uniform(0.01,0.99) with the factor drawn first — g++, the
      // reference's compiler, evaluates that product's operands right to left (pinned by the
      // reference-harness goldens, tests/golden/gen_golden.py)
      const v3 rv = lamb ? v3{ykd::uniform_of(c0, -1, 1), ykd::uniform_of(c1, -1, 1), ykd::uniform_of(c2, -1, 1)}
                         : v3{ykd::uniform_of(c1, -1, 1), ykd::uniform_of(c2, -1, 1), ykd::uniform_of(c3, -1, 1)};
      const v3 vn = lamb ? rv : d;
      const double len = ykd::nsqrt_c(ykd::len2(vn), n_ncall, n_nit);  // vec3::length(), vec3.hpp:127
      // vn / len is what every branch below divides (sky: d.y / len; lambertian: the random
      // vector; metal, dielectric: d), so it is computed once here, not once per branch
      const v3 un = ykd::divs_fast(vn, len);
      double ct = 0;  // dielectric: cos(theta) = min(dot(-unit, n), 1)
      if (diel) {
        ct = ykd::dot(ykd::neg(un), nrm);
        if (!(ct < 1.0)) ct = 1.0;
      }
      double sq2 = 0;  // fuzzed metal: |random vector|; dielectric: sin(theta)
      if (fuzzy || diel) sq2 = ykd::nsqrt_c(fuzzy ? ykd::len2(rv) : 1.0 - ct * ct, n_ncall, n_nit);
      if (hid < 0) {
        // sky (raytracer.hpp:35-36): t = (normalized(dir).y + 1)/2, lerp white → (.5,.7,1)
        const double t = (un.y + 1.0) / 2;
        L_r = (1.0 - t) * 1.0 + t * 0.5;
        L_g = (1.0 - t) * 1.0 + t * 0.7;
        L_b = (1.0 - t) * 1.0 + t * 1.0;
        ended = true;
      } else {
        bool scattered = true, push = true;
        v3 nd;
        if (m.kind == YK_MATERIAL_LAMBERTIAN) {  // material.hpp:50-59
          if (kCount) ++n_lamb;
          nd = ykd::add(nrm, un);
          if (ykd::near_zero(nd)) nd = nrm;
        } else if (m.kind == YK_MATERIAL_METAL) {  // material.hpp:67-75 (+ fuzz extension)
          if (kCount) ++n_metal;
          nd = ykd::reflect(un, nrm);
          if (fuzzy) {  // + fuzz * random_in_unit_sphere (material.hpp:27-30)
            if (kCount) ++n_fuzz;
            const double k = ykd::uniform_of(c0, 0.01, 0.99);
            const v3 ru = ykd::divs_fast(rv, sq2);
            nd = ykd::add(nd, ykd::mul(ykd::mul(ru, k), m.fuzz));
          }
          scattered = ykd::dot(nd, nrm) > 0;
        } else {  // dielectric extension (attenuation (1,1,1): multiplying by 1.0 is exact)
          if (kCount) ++n_diel;
          push = false;
          // 1/ior and Schlick's r0 of both sides precomputed on the host with the same IEEE
          // operations (ykgpu_set_scene: the dielectric's unused fuzz / albedo fields)
          const double ratio = front ? m.fuzz : m.ior;
          const double r0 = front ? m.ar : m.ag;
          const v3 unit = un;
          const double sn = sq2;
          const bool cannot = ratio * sn > 1.0;
          double u = 0;
          if (cannot) {
            if (spec) g = saved;  // `cannot || ...` never draws: give the word pair back
          } else {
            u = spec ? ykd::uniform_of(c0, 0, 1) : ykd::uniform(g, 0, 1);
          }
          if (cannot || ykd::reflectance_r0(ct, r0) > u) {
            nd = ykd::reflect(unit, nrm);
          } else {
            const v3 perp = ykd::mul(ykd::add(unit, ykd::mul(nrm, ct)), ratio);
            const double pl = 1.0 - ykd::len2(perp);
            nd = ykd::add(perp, ykd::mul(nrm, -ykd::nsqrt_c(pl < 0 ? -pl : pl, n_ncall, n_nit)));
          }
        }
        if (!scattered) {
          ended = true;  // absorbed: black (raytracer.hpp:30)
        } else {
          if (push) {
            if (nstk >= kStackRegs) id_spill[nstk - kStackRegs] = (uint16_t)(st3 >> 16);
            st3 = (st3 << 16) | (st2 >> 16);
            st2 = (st2 << 16) | (st1 >> 16);
            st1 = (st1 << 16) | (st0 >> 16);
            st0 = (st0 << 16) | (uint32_t)hid;
            ++nstk;
          }
          o = p;
          d = nd;
          --depth;
        }
      }
    }
    YK_STAMP(4);

    if (ended) {
      // unwind: attenuation_k * (...) from the deepest scatter outwards (raytracer.hpp:31)
      auto pop = [&]() {
        const uint32_t id = st0 & 0xffffu;
        st0 = (st0 >> 16) | (st1 << 16);
        st1 = (st1 >> 16) | (st2 << 16);
        st2 = (st2 >> 16) | (st3 << 16);
        st3 = (st3 >> 16) | (nstk > kStackRegs ? ((uint32_t)id_spill[nstk - kStackRegs - 1] << 16) : 0u);
        --nstk;
        return id;
      };
      if (__ballot(nstk > kStackRegs) == 0) {
        // no ending lane of the wave holds spilled ids: the register window alone, two ids per
        // round (the window moves by a whole register)
        while (nstk > 0) {
          const SphereMat m = mat[st0 & 0xffffu];
          L_r = m.ar * L_r;
          L_g = m.ag * L_g;
          L_b = m.ab * L_b;
          if (nstk > 1) {
            const SphereMat m2 = mat[st0 >> 16];
            L_r = m2.ar * L_r;
            L_g = m2.ag * L_g;
            L_b = m2.ab * L_b;
          }
          st0 = st1, st1 = st2, st2 = st3;
          nstk = nstk > 1 ? nstk - 2 : 0;
        }
      } else {
        while (nstk > 0) {
          const SphereMat m = mat[pop()];
          L_r = m.ar * L_r;
          L_g = m.ag * L_g;
          L_b = m.ab * L_b;
        }
      }
      if (ykd::mt_used_fallback(g)) ++n_fb;
      if (kCount) n_words += ykd::rng_words(g), n_twist += ykd::rng_twists(g);
      // the sample's colour; yk_reduce_samples adds them in sample order
      colour_store(ka.col, slot, L_r, L_g, L_b);
      in_path = false;
    }
    YK_STAMP(5);
  }

  YK_CLOCK_END(ka);
  YK_WAVE_STAMP(ka, 1);
  YK_STAMPS_END(ka.counters, lane);
  if (kCount) {
    atomicAdd(&ka.counters[0], (unsigned long long)n_seg);
    atomicAdd(&ka.counters[1], (unsigned long long)n_test);
    atomicAdd(&ka.counters[2], (unsigned long long)n_sqrt);
    atomicAdd(&ka.counters[4], (unsigned long long)n_node);
    atomicAdd(&ka.counters[5], (unsigned long long)n_lin);
    atomicAdd(&ka.counters[6], (unsigned long long)n_ncall);
    atomicAdd(&ka.counters[7], (unsigned long long)n_nit);
    atomicAdd(&ka.counters[24], (unsigned long long)n_dpos);
    atomicAdd(&ka.counters[25], (unsigned long long)n_lamb);
    atomicAdd(&ka.counters[26], (unsigned long long)n_metal);
    atomicAdd(&ka.counters[27], (unsigned long long)n_fuzz);
    atomicAdd(&ka.counters[28], (unsigned long long)n_diel);
    atomicAdd(&ka.counters[29], (unsigned long long)n_words);
    atomicAdd(&ka.counters[30], (unsigned long long)n_swords);
    atomicAdd(&ka.counters[31], (unsigned long long)n_twist);
  }
  if (n_fb) atomicAdd(&ka.counters[3], (unsigned long long)n_fb);
}

// The kernels.  Production instances at <= YK_RENDER_VGPRS (gfx950's amdgpu_num_vgpr counts the
// unified file, so the attribute takes half).
template <bool kSceneInLds, int kMode>
__global__ __launch_bounds__(mode_block<kMode>())
__attribute__((amdgpu_waves_per_eu(4, 8)))
__attribute__((amdgpu_num_vgpr(YK_RENDER_VGPRS / 2)))
void yk_render_persistent(KernelArgs ka) {
  render_body<kSceneInLds, kMode>(ka);
}
// the counting instances (kMode bit 0: diagnostic builds of the same body, YK_FLAG_COUNT_WORK)
// under a name of their own, their registers uncapped
template <bool kSceneInLds, int kMode>
__global__ __launch_bounds__(mode_block<kMode>()) __attribute__((amdgpu_waves_per_eu(1, 8)))
void yk_render_counting(KernelArgs ka) {
  render_body<kSceneInLds, kMode>(ka);
}

// The FP64 instance for (scene in LDS, kMode)
RenderKernel fp64_kernel(bool lds, int mode) {
  static const RenderKernel k[16] = {
      yk_render_persistent<false, 0>, yk_render_counting<false, 1>,  yk_render_persistent<false, 2>,
      yk_render_counting<false, 3>,   yk_render_persistent<false, 4>, yk_render_counting<false, 5>,
      yk_render_persistent<false, 6>, yk_render_counting<false, 7>,  yk_render_persistent<true, 0>,
      yk_render_counting<true, 1>,    yk_render_persistent<true, 2>,  yk_render_counting<true, 3>,
      yk_render_persistent<true, 4>,  yk_render_counting<true, 5>,    yk_render_persistent<true, 6>,
      yk_render_counting<true, 7>};
  return k[(lds ? 8 : 0) + (mode & 7)];
}

}  // namespace

const void* yk_fp64_kernel(bool lds, int mode) { return (const void*)fp64_kernel(lds, mode); }

#ifdef YK_DRAIN_DIAG
// (the records live in this unit, so their accessors do too: hipMemcpyFromSymbol needs the defining
// unit.  They report a HIP failure by code alone; the last-error text is yk_context.hip's.)
#define YK_DIAG_HIP(call) \
  do {                    \
    if ((call) != hipSuccess) return YK_ERR_DEVICE; \
  } while (0)
extern "C" {
// (diagnostic builds only, tools/drain_probe.py) the wave records since the last clear:
// [launch][block][wave] x {start, end, HW_ID | XCC_ID << 32}
int ykgpu_diag_wave_times(unsigned long long* out, size_t n) {
  const size_t cap = sizeof(yk_wave_times) / sizeof(unsigned long long);
  YK_DIAG_HIP(hipDeviceSynchronize());
  YK_DIAG_HIP(hipMemcpyFromSymbol(out, HIP_SYMBOL(yk_wave_times), std::min(n, cap) * sizeof(unsigned long long)));
  return YK_OK;
}
int ykgpu_diag_wave_times_clear(void) {
  YK_DIAG_HIP(hipDeviceSynchronize());
  static std::vector<unsigned long long> z(sizeof(yk_wave_times) / sizeof(unsigned long long), 0ull);
  YK_DIAG_HIP(hipMemcpyToSymbol(HIP_SYMBOL(yk_wave_times), z.data(), z.size() * sizeof(unsigned long long)));
  return YK_OK;
}
}  // extern "C"
#endif
