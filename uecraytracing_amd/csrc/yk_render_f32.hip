// yk_render_f32.hip — the FP32 path kernel (yk_render_f32), the one unit compiled under LLVM's
// max-ilp scheduler (FP32 512 spp: -1.3%; the same scheduler costs the FP64 kernel +1.5%,
// DESIGN.md §8).
#include "yk_path.hpp"

namespace {

// ---- render<float> (YK_PRECISION_FP32) ---------------------------------------------------
// The same persistent, sample-parallel structure as yk_render_persistent (refill, slots, start
// records from yk_mt_warmup, attenuation-id stack, SoA colours reduced by yk_reduce_samples),
// with the path in float (yk_device_f32.hpp).  Closest hit: the FP32 tree culls — its boxes and
// a per-ray cone carry the float sphere test's proven error — the spheres of an
// entered leaf get the reference's float discriminant and bounds of their float root, and the
// survivors' exact float roots are evaluated after the traversal: the minimum root wins, an exact
// tie goes to the later tuple index.  Rays outside the tree's proven range take the ordered scan
// (hittable_list.hpp:32-58).
template <class G>
__device__ __forceinline__ float f_uniform01(G& g) { return ykf::uniform(g, 0.0f, 1.0f); }

// sphere::hit_impl<float> (sphere.hpp:25-48) bit for bit, without t_max.  Returns 2 with the root
// in r (root1 if >= tmin, else root2: the reference accepts it iff r <= t_max, because root2 >=
// root1 under monotonic rounding), 1 when both roots lie below tmin, 0 when disc < 0.
// n / a for a root, a's refined reciprocal ra shared by the ray's candidates (ykf::div_by); a wave
// with any lane out of range takes the full division
__device__ __forceinline__ float f32_root_div(float n, float a, float ra, bool a_ok) {
  float q = ykf::div_by(n, a, ra);
  if (__builtin_expect(__ballot(!(a_ok && ykf::num_range(n))) != 0, 0)) q = n / a;
  return q;
}
__device__ __forceinline__ int f32_root(float4 sg, ykf::v3 o, ykf::v3 d, float a, float ra, bool a_ok, float tmin,
                                        float& r, uint32_t& nit) {
  const ykf::v3 oc = {o.x - sg.x, o.y - sg.y, o.z - sg.z};
  const float hb = ykf::dot(oc, d);
  const float c = ykf::len2(oc) - sg.w;
  const float disc = hb * hb - a * c;
  if (disc < 0) return 0;
  const float sq = ykf::nsqrt(disc, nit);
  r = f32_root_div(-hb - sq, a, ra, a_ok);
  if (r < tmin) {
    r = f32_root_div(-hb + sq, a, ra, a_ok);
    if (r < tmin) return 1;
  }
  return 2;
}

// the cone keeps a far bound on an axis with |d| >= kF32FarAt s, and gives the slow-axis bound
// to one with |d| < kF32SlowAt s (d - s sign d stays clear of 0 in both)
constexpr float kF32FarAt = 1.0f + 0x1p-10f, kF32SlowAt = 1.0f - 0x1p-10f;

// Bounds of the root f32_root returns, from the exact float discriminant: the
// approximation r = (-hb ∓ v_sqrt_f32(disc)) · v_rcp_f32(a) differs from the exact root by at most
// (|hb| + √disc)/a · 9u (one-step sqrt within 1.5u, v_sqrt/v_rcp within an ulp, three roundings;
// u = 2^-24); m takes 256u, plus an absolute term for underflowing products.  A disc outside the
// one-step square root's range [2^-100, 2^100] gets no bound (m = inf: always a candidate).
// Returns false when both roots certainly lie below tmin; else lb <= the accepted root <= ub
// (ub = inf when neither root is certainly >= tmin).  NaN anywhere keeps the sphere (every
// comparison that would drop it is false).
__device__ __forceinline__ bool f32_root_bounds(float hb, float disc, float ia, float tmin, float& lb, float& ub) {
  const float sq = __builtin_amdgcn_sqrtf(disc);
  const float r1 = (-hb - sq) * ia, r2 = (-hb + sq) * ia;
  float m = (fabsf(hb) + sq) * ia * 0x1p-16f + 0x1p-120f;
  if (!(disc >= 0x1p-100f && disc <= 0x1p100f)) m = INFINITY;
  if (r2 + m < tmin) return false;
  lb = fmaxf(tmin, r1 - m);
  ub = (r1 - m >= tmin) ? r1 + m : ((r2 - m >= tmin) ? r2 + m : INFINITY);
  return true;
}

// One axis of the ray's cone: near planes are crossed at (plane - o) * in, far
// planes at (plane - o) * jf, with in = 1/(d + s sign d) and jf = (1 + 2^-17)/(d - s sign d); an
// axis with |d| < kF32FarAt s keeps no far bound (jf = 0, constant +inf).  Slab FMA operands:
// plane * in + nc.  Culling arithmetic only: v_rcp_f32's ulp is inside the relative margins (d - s
// sign d is exact for |d| <= 2s, Sterbenz).
__device__ __forceinline__ void cone_axis(float dk, float ok, float s, f2& in2, f2& nc2, f2& jf2, f2& fc2) {
  const float sg = dk < 0.0f ? -s : s;
  const float in = __builtin_amdgcn_rcpf(dk + sg);
  const bool far = fabsf(dk) >= kF32FarAt * s;
  const float jf = far ? __builtin_amdgcn_rcpf(dk - sg) * (1.0f + 0x1p-17f) : 0.0f;
  const float nc = -(ok * in), fc = far ? -(ok * jf) : INFINITY;
  // the pairs (in, nc) and (jf, fc), read by op_sel (yk_slab.hpp); nc2 / fc2 are unused (dropping
  // the two dead parameters changes the FP32 kernels' schedule)
  in2 = f2{in, nc};
  jf2 = f2{jf, fc};
  nc2 = fc2 = f2{0.0f, 0.0f};
}

// kSceneInLds: the FP32 tree, its float4 leaf geometry and its leaf ids copied into LDS per
// workgroup, as in the FP64 kernel.  kMode bit 0: the work counters; bit 2: the yk::xor128
// engine (as for the FP64 kernel)
template <bool kSceneInLds, int kMode>
__global__ __launch_bounds__(mode_block<kMode>())
void yk_render_f32(KernelArgs ka) {
  constexpr int kBlk = mode_block<kMode>();
  constexpr bool kCount = (kMode & 1) != 0;
  using Gen = typename std::conditional<(kMode & 4) != 0, ykd::X128Lane, ykd::MtLane>::type;
  const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63u;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const char* __restrict__ nodes = (const char*)ka.nodes;
  const float4* __restrict__ leaf_geo = (const float4*)ka.leaf_geo;
  const uint32_t* __restrict__ leaf_ids = ka.leaf_ids;
  const float4* __restrict__ geo_f = ka.geo_f;  // tuple order: hit records
  const SphereMat* __restrict__ mat = ka.mat;   // shading, attenuation unwind
  if (kSceneInLds) {
    // as in the FP64 kernel: the BVH, its leaf geometry and ids, and the tuple-order tables
    const uint4* src[5] = {(const uint4*)ka.nodes, (const uint4*)ka.leaf_geo, (const uint4*)ka.leaf_ids,
                           (const uint4*)ka.geo_f, (const uint4*)ka.mat};
    const uint32_t off[5] = {0u, ka.lds_geo_off, ka.lds_ids_off, ka.lds_tgeo_off, ka.lds_mat_off};
    const uint32_t n16[5] = {(ka.n_nodes * (uint32_t)sizeof(DevNode) + 15u) / 16u, ka.nspheres,
                             (ka.nspheres + 3u) / 4u, ka.nspheres, ka.nspheres * 4u};
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      uint4* dst = (uint4*)(smem + off[k]);
      for (uint32_t i = threadIdx.x; i < n16[k]; i += kBlk) dst[i] = src[k][i];
    }
    __syncthreads();
    nodes = smem;
    leaf_geo = (const float4*)(smem + ka.lds_geo_off);
    leaf_ids = (const uint32_t*)(smem + ka.lds_ids_off);
    geo_f = (const float4*)(smem + ka.lds_tgeo_off);
    mat = (const SphereMat*)(smem + ka.lds_mat_off);
  }
  int32_t* const stk = (int32_t*)(smem + ka.lds_stack_off) + threadIdx.x;  // [sp * kBlk]
  __builtin_amdgcn_s_setprio(1);  // over the co-resident warm-up waves, as in FP64
  YK_CLOCK_BEGIN(ka);
  Gen g;
  rng_init(g, ka, gid);
  uint16_t* const id_spill = ka.id_scratch + (size_t)gid * ka.id_stride;
  uint32_t n_seg = 0, n_test = 0, n_sqrt = 0, n_fb = 0, n_nit = 0, n_ncall = 0, n_node = 0, n_lin = 0;
  uint32_t n_words = 0, n_swords = 0, n_twist = 0;  // as in yk_render_persistent
  YK_STAMPS_BEGIN(ka.counters, lane);
  const float tmin = (float)ka.t_min;  // world.hit(r, 0.001, ...) converts to T (hittable.hpp:32)
  uint32_t slot = 0, depth = 0, nstk = 0;
  uint32_t st0 = 0, st1 = 0, st2 = 0, st3 = 0;
  ykf::v3 o = {0, 0, 0}, d = {0, 0, 0};
  bool in_path = false;
  uint32_t res_base = 0, res_left = 0;

  for (;;) {
    if (claim_slots(ka, in_path, lane, slot, res_base, res_left)) {
      YK_STAMPS_EXHAUSTED(ka.counters);
      break;
    }
    YK_STAMP(0);

    // ---- start: seed, jitter, camera<float>::get_ray (source.cpp:154-165, camera.hpp:29-32)
    bool start = !in_path;
    uint32_t qpix = 0;
    // mt19937: the start (draws and camera<float> ray) comes precomputed (yk_mt_warmup<lens,
    // true>: StartRecF), which alone says whether the slot is empty, as in the FP64 kernel
    constexpr bool kRec = std::is_same<Gen, ykd::MtLane>::value;
    uint4 rq0 = {0, 0, 0, 0}, rq1 = {0, 0, 0, 0}, rq2 = {0, 0, 0, 0};
    if (start) {
      if constexpr (kRec) {
        const uint4* rp = (const uint4*)ka.start + 3u * slot;
        rq0 = rp[0];
        rq1 = rp[1];
        rq2 = rp[2];
        asm volatile("" ::"v"(rq0.x), "v"(rq0.y), "v"(rq0.z), "v"(rq0.w), "v"(rq1.x), "v"(rq1.y),
                     "v"(rq2.x), "v"(rq2.y), "v"(rq2.z), "v"(rq2.w));
        start = rq2.w != kPadSlot;
      } else {
        const uint32_t sl = fdiv(slot, ka.nps_m, ka.nps_sh);
        qpix = ka.order[slot - sl * ka.npix_slots];
        start = qpix != kNoPixel;
      }
    }
    if (start) {
      bool pre = false;
      if constexpr (kRec) {
        StartRecF r;
        __builtin_memcpy((char*)&r, &rq0, 16);
        __builtin_memcpy((char*)&r + 16, &rq1, 16);
        __builtin_memcpy((char*)&r + 32, &rq2, 16);
        pre = r.j != kNoStart;
        if (pre) {
          if (kCount) n_swords += r.j;
          g.a0 = r.a0;
          g.a1 = r.a1;
          g.b = r.b;
          g.j = r.j;
          o = ykf::v3{r.ox, r.oy, r.oz};
          d = ykf::v3{r.dx, r.dy, r.dz};
        }
      }
      if (!pre) {
        const uint32_t sl = fdiv(slot, ka.nps_m, ka.nps_sh);
        if constexpr (kRec) qpix = ka.order[slot - sl * ka.npix_slots];
        const uint32_t s = ka.s0 + sl;
        const uint32_t tr = fdiv(qpix, ka.w_m, ka.w_sh);
        const uint32_t x = tile_col_x(ka.col_begin, ka.col_stride, ka.col_band, qpix - tr * ka.Wt);
        const uint32_t y = tile_row_y(ka.row_begin, ka.row_stride, ka.band_log2, tr);
        const uint32_t seed = ykd::sample_seed(ka.seed_mode, ka.seed_key, ka.seed0, y, x, ka.W, ka.spp, s);
        const bool lens = ka.cam.lens_radius > 0;  // (decided in double, as for the warm-up)
        rng_start_full(g, seed);
        const float uc = f_uniform01(g);
        const float vc = f_uniform01(g);
        float px = 0, py = 0;
        if (lens) {  // thin-lens extension: random_in_unit_disk by rejection, x then y
          do {
            px = ykf::uniform(g, -1.0f, 1.0f);
            py = ykf::uniform(g, -1.0f, 1.0f);
          } while (!(px * px + py * py < 1.0f));
        }
        camera_ray_f32(ka.camf, ka.H, x, y, uc, vc, lens, px, py, o, d);
      }
      depth = ka.max_depth;
      nstk = 0;
      in_path = true;
    }

    YK_STAMP(1);
    if (kCount && (ka.flags & kFlagTrace) && in_path) trace_ray(ka, slot, ka.max_depth - depth, o, d);

    // ---- closest hit (hittable_list.hpp:32-58 over sphere.hpp:25-48, in float)
    const bool alive = in_path && depth != 0;
    float T = INFINITY;
    int hid = -1;
    if (alive) {
      ++n_seg;
      const float a = ykf::len2(d);
      const float onorm = fmaxf(fabsf(o.x), fmaxf(fabsf(o.y), fabsf(o.z)));
      // the tree serves the rays its bound is proven for: |d|^2 in [2^-60, 2^60],
      // origin within origin_bound (< 0: the scene is outside the proven scale); the rest scan
      bool linear = (ka.flags & kFlagLinearScan) || !(a >= 0x1p-60f && a <= 0x1p60f) ||
                    !((double)onorm <= ka.origin_bound);
      if (!linear) {
        const float s = __builtin_sqrtf(a) * ykbvh::kF32Cone;  // the cone's slope (>= kF32Cone |d|)
        const float tmin_lo = tmin * (1.0f - 0x1p-17f);
        float ustar_f = INFINITY;  // T (1 + 2^-18): every box that may hold a root <= T passes
        f2 inx, ncx, jfx, fcx, iny, ncy, jfy, fcy, inz, ncz, jfz, fcz;
        cone_axis(d.x, o.x, s, inx, ncx, jfx, fcx);
        cone_axis(d.y, o.y, s, iny, ncy, jfy, fcy);
        cone_axis(d.z, o.z, s, inz, ncz, jfz, fcz);
        // the (near x4, far x4) plane quads of the ray's direction signs inside a WideNode
        const char* const px = nodes + (d.x < 0.0f ? 16u : 0u);
        const char* const py = nodes + 48u + (d.y < 0.0f ? 16u : 0u);
        const char* const pz = nodes + 96u + (d.z < 0.0f ? 16u : 0u);
        // A slow axis (|d| < s, the cone opens both ways along it) has no far bound, but the cone
        // still enters a box that lies against the direction of travel only after its far-side
        // plane: o + (d - s sign d) t reaches it at t = (plane - o) / (d - s sign d) > 0, a lower
        // bound like a near distance (same FMA form and error).  Without it, a
        // ray grazing a field of boxes enters every box under its path.  One slow axis per ray
        // gets the bound (y, then x, then z); the others keep L = -inf.
        f2 jl2 = {0.0f, -INFINITY};  // the (jl, cl) pair
        const char* pl = px + 16;
        {
          const float slow = s * kF32SlowAt;
          const float dk[3] = {d.z, d.x, d.y}, ok[3] = {o.z, o.x, o.y};
          const char* const pk[3] = {pz, px, py};
#pragma unroll
          for (int k = 0; k < 3; ++k) {
            if (fabsf(dk[k]) < slow) {
              const float jl = __builtin_amdgcn_rcpf(dk[k] - (dk[k] < 0.0f ? -s : s));
              jl2 = f2{jl, -(ok[k] * jl)};  // (jl, cl), read by op_sel
              pl = pk[k] + 16;
            }
          }
        }
        // U*: proven upper bound of the minimum root (culls with ustar_f = U* (1 + 2^-18)); the
        // candidate list (tuple index, lower bound) as in the FP64 kernel, nc = 5 on overflow
        const float ia = __builtin_amdgcn_rcpf(a);  // a in [2^-60, 2^60] here
        float ustar = INFINITY;
        uint32_t nc = 0, c0 = 0, c1 = 0, c2 = 0, c3 = 0;
        float l0 = 0, l1 = 0, l2 = 0, l3 = 0;
        uint32_t overflow = 0;  // a VGPR, not a lane-mask bool (see the FP64 kernel)
        int32_t node = ka.bvh_root;
        int32_t* top = stk;
        const int32_t* const stk_cap = stk + ka.stack_cap * kBlk;
        for (;;) {
          if (node >= 0) {
            if (kCount) ++n_node;
            YK_STAMP_NODE_ITERATION(lane);
            // the FP64 kernel's visit (same planes, margins and visit order), the cone's operands
            const f4 qnx = *(const f4*)(px + node), qfx = *(const f4*)(px + node + 16);
            const f4 qny = *(const f4*)(py + node), qfy = *(const f4*)(py + node + 16);
            const f4 qnz = *(const f4*)(pz + node), qfz = *(const f4*)(pz + node + 16);
            const int4 ch = *(const int4*)(nodes + node + 144);
            bool hk[4];
            const f2 nx[2] = {slab_fma(qnx.xy, inx), slab_fma(qnx.zw, inx)};
            const f2 fx[2] = {slab_fma(qfx.xy, jfx), slab_fma(qfx.zw, jfx)};
            const f2 ny[2] = {slab_fma(qny.xy, iny), slab_fma(qny.zw, iny)};
            const f2 fy[2] = {slab_fma(qfy.xy, jfy), slab_fma(qfy.zw, jfy)};
            const f2 nz[2] = {slab_fma(qnz.xy, inz), slab_fma(qnz.zw, inz)};
            const f2 fz[2] = {slab_fma(qfz.xy, jfz), slab_fma(qfz.zw, jfz)};
            const f4 qsl = *(const f4*)(pl + node);
            const f2 sl[2] = {slab_fma(qsl.xy, jl2), slab_fma(qsl.zw, jl2)};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
              const float tn = slab_max3(slab_max3(nx[k >> 1][k & 1], ny[k >> 1][k & 1], nz[k >> 1][k & 1]),
                                         sl[k >> 1][k & 1], tmin_lo);
              const float tf = slab_min(slab_min3(fx[k >> 1][k & 1], fy[k >> 1][k & 1], fz[k >> 1][k & 1]), ustar_f);
              hk[k] = tn <= tf;
            }
            asm volatile("" ::"v"(ch.x), "v"(ch.y), "v"(ch.z), "v"(ch.w));
            if (hk[0] || hk[1] || hk[2] || hk[3]) {
              node = hk[3] ? ch.w : (hk[2] ? ch.z : (hk[1] ? ch.y : ch.x));
              *top = ch.x;
              top += (hk[0] && (hk[1] || hk[2] || hk[3])) ? kBlk : 0;
              *top = ch.y;
              top += (hk[1] && (hk[2] || hk[3])) ? kBlk : 0;
              *top = ch.z;
              top += (hk[2] && hk[3]) ? kBlk : 0;
              if (top > stk_cap) {  // stack full: abandon, the linear scan decides
                overflow = 1;
                top = stk;
                node = ykbvh::kEmptyLeaf;
              }
              continue;
            }
            if (top == stk) {  // as in the FP64 kernel
              node = ykbvh::kEmptyLeaf;
            } else {
              top -= kBlk;
              node = *top;
            }
            continue;
          } else {
            YK_STAMP(2);
            const uint32_t v = ~(uint32_t)node, first = v >> 4, cnt = v & 15u;
            // bound-then-evaluate, as in the FP64 kernel: the exact discriminant decides disc < 0,
            // the root gets bounds only, and the survivors' exact roots are evaluated after the
            // traversal, with the lanes converged
            // (the FP32 tree has at most two spheres per leaf: the loop unrolled, without a loop
            // counter or latch; FP32 512 spp: -2.7%)
#pragma unroll
            for (uint32_t k = 0; k < kLeafCapF32; ++k) {
              if (k >= cnt) break;
              const float4 sg = leaf_geo[first + k];
              const uint32_t id = leaf_ids[first + k];
              asm volatile("" ::"v"(id));
              if (kCount) ++n_test;
              const ykf::v3 oc = {o.x - sg.x, o.y - sg.y, o.z - sg.z};
              const float hb = ykf::dot(oc, d);
              const float c = ykf::len2(oc) - sg.w;
              const float disc = hb * hb - a * c;
              if (disc < 0) continue;
              YK_STAMP_DISC_POS();
              float lb, ub;
              if (!f32_root_bounds(hb, disc, ia, tmin, lb, ub)) continue;
              if (!(lb <= ustar)) continue;
              if (ub < ustar) {
                ustar = ub;
                ustar_f = ub * (1.0f + 0x1p-18f);
              }
              if (nc == 4) {  // compact: drop entries the new bound has excluded
                uint32_t m2 = 0;
                uint32_t d0 = c0, d1 = c1, d2 = c2, d3 = c3;
                float e0 = l0, e1 = l1, e2 = l2, e3 = l3;
                if (e0 <= ustar) { YK_CAND_SET(m2, d0, e0); ++m2; }
                if (e1 <= ustar) { YK_CAND_SET(m2, d1, e1); ++m2; }
                if (e2 <= ustar) { YK_CAND_SET(m2, d2, e2); ++m2; }
                if (e3 <= ustar) { YK_CAND_SET(m2, d3, e3); ++m2; }
                nc = m2;
              }
              if (nc < 4) {
                c3 = c2, l3 = l2, c2 = c1, l2 = l1, c1 = c0, l1 = l0;
                c0 = id, l0 = lb;
                ++nc;
              } else {
                nc = 5;  // the list is full: the ordered scan decides
              }
            }
            YK_STAMP(6);
          }
          if (top == stk) break;
          top -= kBlk;
          node = *top;
        }
        YK_STAMP(2);
        if (overflow != 0) linear = true;
        if (nc > 4) linear = true;
        if (!linear) {
          // the survivors' exact roots: the minimum wins, an exact tie goes to the later tuple
          // index (hittable_list.hpp:36-43); a candidate whose lower bound exceeds the final U*
          // cannot be the minimum
#define YK_F32_EVAL(C, L)                                                       \
  if ((L) <= ustar) {                                                           \
    float r = 0.0f;                                                             \
    const int res = f32_root(geo_f[C], o, d, a, ra, a_ok, tmin, r, n_nit);      \
    if (kCount && res > 0) ++n_sqrt, ++n_ncall;                                 \
    if (res == 2 && (r < T || (r == T && (int)(C) > hid))) T = r, hid = (int)(C); \
  }
          const bool a_ok = ykf::div_range(a);
          const float ra = ykf::rcp_refined(a);
          if (nc > 0) YK_F32_EVAL(c0, l0)
          if (nc > 1) YK_F32_EVAL(c1, l1)
          if (nc > 2) YK_F32_EVAL(c2, l2)
          if (nc > 3) YK_F32_EVAL(c3, l3)
#undef YK_F32_EVAL
        }
      }
      if (linear) {  // the reference's ordered scan in tuple order (wave-uniform scalar loads)
        ++n_lin;
        T = INFINITY;
        hid = -1;
        for (uint32_t i = 0; i < ka.nspheres; ++i) {
          const float4 sg = ka.geo_f[i];
          if (kCount) ++n_test;
          const ykf::v3 oc = {o.x - sg.x, o.y - sg.y, o.z - sg.z};
          const float hb = ykf::dot(oc, d);
          const float c = ykf::len2(oc) - sg.w;
          const float disc = hb * hb - a * c;
          if (disc < 0) continue;
          if (kCount) ++n_sqrt, ++n_ncall;
          const float sq = ykf::nsqrt(disc, n_nit);
          float root = (-hb - sq) / a;
          if (root < tmin || T < root) {
            root = (-hb + sq) / a;
            if (root < tmin || T < root) continue;
          }
          T = root;
          hid = (int)i;
        }
      }
    }

    YK_STAMP(3);
    // ---- shade (raytracer.hpp:25-36, material.hpp), material-uniform as in the FP64 kernel: one
    //      block of canonicals (float: one word each) for lambertian's vec3::random (3), the fuzzed
    //      metal's factor and vector (4) and the dielectric's uniform (1, drawn speculatively and
    //      given back on total internal reflection); one normalisation; one second square root
    //      (the fuzzed metal's |vector|, the dielectric's sin(theta)).  Each lane's own operations
    //      and their order are the reference's render<float>.
    bool ended = in_path && !alive;
    double L_r = 0, L_g = 0, L_b = 0;
    if (alive) {
      SphereMat m{};
      ykf::v3 p{0, 0, 0}, nrm{0, 0, 0};
      bool front = false;
      if (hid >= 0) {
        const float4 sg = geo_f[hid];
        m = mat[hid];
        p = ykf::add(o, ykf::mul(d, T));  // ray::at
        const ykf::v3 outward = ykf::divs_fast_r(ykf::sub(p, ykf::v3{sg.x, sg.y, sg.z}), (float)m.radius, m.inv_rf);
        front = ykf::dot(d, outward) < 0;
        nrm = front ? outward : ykf::neg(outward);
      }
      const bool lamb = hid >= 0 && m.kind == YK_MATERIAL_LAMBERTIAN;
      const bool fuzzy = hid >= 0 && m.kind == YK_MATERIAL_METAL && m.fuzz > 0;
      const bool diel = hid >= 0 && m.kind == YK_MATERIAL_DIELECTRIC;
      const bool spec = diel && ykd::rng_can_speculate(g);
      const Gen saved = g;  // the dielectric's engine before its speculative draw
      const uint32_t ncan = lamb ? 3u : (fuzzy ? 4u : (spec ? 1u : 0u));
      float c0 = 0, c1 = 0, c2 = 0, c3 = 0;
      if (__ballot(ncan > 0 && !ykd::rng_lazy_ok(g, ncan)) == 0) {
        if (ncan > 0) c0 = ykf::canonical<true>(g);
        if (ncan > 1) c1 = ykf::canonical<true>(g);
        if (ncan > 2) c2 = ykf::canonical<true>(g);
        if (ncan > 3) c3 = ykf::canonical<true>(g);
      } else {
        if (ncan > 0) c0 = ykf::canonical(g);
        if (ncan > 1) c1 = ykf::canonical(g);
        if (ncan > 2) c2 = ykf::canonical(g);
        if (ncan > 3) c3 = ykf::canonical(g);
      }
      // lambertian: vec3::random(-1, 1), x then y then z; fuzzed metal: the length factor first
      const ykf::v3 rv = lamb ? ykf::v3{ykf::uniform_of(c0, -1.0f, 1.0f), ykf::uniform_of(c1, -1.0f, 1.0f),
                                        ykf::uniform_of(c2, -1.0f, 1.0f)}
                              : ykf::v3{ykf::uniform_of(c1, -1.0f, 1.0f), ykf::uniform_of(c2, -1.0f, 1.0f),
                                        ykf::uniform_of(c3, -1.0f, 1.0f)};
      const ykf::v3 vn = lamb ? rv : d;
      if (kCount) ++n_ncall;
      const ykf::v3 un = ykf::divs_fast(vn, ykf::nsqrt(ykf::len2(vn), n_nit));
      float ct = 0;  // dielectric: cos(theta) = min(dot(-unit, n), 1)
      if (diel) {
        ct = ykf::dot(ykf::neg(un), nrm);
        if (!(ct < 1.0f)) ct = 1.0f;
      }
      float sq2 = 0;  // fuzzed metal: |random vector|; dielectric: sin(theta)
      if (fuzzy || diel) sq2 = ykf::nsqrt(fuzzy ? ykf::len2(rv) : 1.0f - ct * ct, n_nit);
      if (hid < 0) {
        // sky: normalized(dir).y is a float; + 1.0 and the lerp are double (raytracer.hpp:35-36)
        const double t = ((double)un.y + 1.0) / 2;
        L_r = (1.0 - t) * 1.0 + t * 0.5;
        L_g = (1.0 - t) * 1.0 + t * 0.7;
        L_b = (1.0 - t) * 1.0 + t * 1.0;
        ended = true;
      } else {
        bool scattered = true, push = true;
        ykf::v3 nd;
        if (m.kind == YK_MATERIAL_LAMBERTIAN) {
          nd = ykf::add(nrm, un);
          if (ykf::near_zero(nd)) nd = nrm;
        } else if (m.kind == YK_MATERIAL_METAL) {
          nd = ykf::reflect(un, nrm);
          if (fuzzy) {
            const float k = ykf::uniform_of(c0, 0.01f, 0.99f);
            const ykf::v3 ru = ykf::divs_fast(rv, sq2);
            nd = ykf::add(nd, ykf::mul(ykf::mul(ru, k), (float)m.fuzz));
          }
          scattered = ykf::dot(nd, nrm) > 0;
        } else {  // dielectric extension, in float
          push = false;
          const float ior = (float)m.ior;
          const float ratio = front ? (1.0f / ior) : ior;
          const bool cannot = ratio * sq2 > 1.0f;
          float u = 0;
          if (cannot) {
            if (spec) g = saved;  // `cannot || ...` never draws: give the word back
          } else {
            u = spec ? c0 : ykf::canonical(g);
          }
          if (cannot || ykf::reflectance(ct, ratio) > u) {
            nd = ykf::reflect(un, nrm);
          } else {
            const ykf::v3 perp = ykf::mul(ykf::add(un, ykf::mul(nrm, ct)), ratio);
            const float pl = 1.0f - ykf::len2(perp);
            nd = ykf::add(perp, ykf::mul(nrm, -ykf::nsqrt(pl < 0 ? -pl : pl, n_nit)));
          }
        }
        if (!scattered) {
          ended = true;
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
      // attenuation (double albedo) back to front, as in FP64 (raytracer.hpp:31)
      while (nstk > 0) {
        const uint32_t id = st0 & 0xffffu;
        st0 = (st0 >> 16) | (st1 << 16);
        st1 = (st1 >> 16) | (st2 << 16);
        st2 = (st2 >> 16) | (st3 << 16);
        st3 = (st3 >> 16) | (nstk > kStackRegs ? ((uint32_t)id_spill[nstk - kStackRegs - 1] << 16) : 0u);
        --nstk;
        const SphereMat m = mat[id];
        L_r = m.ar * L_r;
        L_g = m.ag * L_g;
        L_b = m.ab * L_b;
      }
      if (ykd::mt_used_fallback(g)) ++n_fb;
      if (kCount) n_words += ykd::rng_words(g), n_twist += ykd::rng_twists(g);
      colour_store(ka.col, slot, L_r, L_g, L_b);
      in_path = false;
    }
    YK_STAMP(5);
  }
  YK_CLOCK_END(ka);
  YK_STAMPS_END(ka.counters, lane);
  if (kCount) {
    atomicAdd(&ka.counters[0], (unsigned long long)n_seg);
    atomicAdd(&ka.counters[1], (unsigned long long)n_test);
    atomicAdd(&ka.counters[2], (unsigned long long)n_sqrt);
    atomicAdd(&ka.counters[4], (unsigned long long)n_node);
    atomicAdd(&ka.counters[5], (unsigned long long)n_lin);
    atomicAdd(&ka.counters[6], (unsigned long long)n_ncall);
    atomicAdd(&ka.counters[7], (unsigned long long)n_nit);
    atomicAdd(&ka.counters[29], (unsigned long long)n_words);
    atomicAdd(&ka.counters[30], (unsigned long long)n_swords);
    atomicAdd(&ka.counters[31], (unsigned long long)n_twist);
  }
  if (n_fb) atomicAdd(&ka.counters[3], (unsigned long long)n_fb);
}

// The FP32 instance for (scene in LDS, kMode)
RenderKernel f32_kernel(bool lds, int mode) {
  static const RenderKernel k[8] = {yk_render_f32<false, 0>, yk_render_f32<false, 1>, yk_render_f32<false, 4>,
                                    yk_render_f32<false, 5>, yk_render_f32<true, 0>,  yk_render_f32<true, 1>,
                                    yk_render_f32<true, 4>,  yk_render_f32<true, 5>};
  return k[(lds ? 4 : 0) + ((mode & 1) | ((mode & 4) >> 1))];
}

}  // namespace

const void* yk_f32_kernel(bool lds, int mode) { return (const void*)f32_kernel(lds, mode); }
