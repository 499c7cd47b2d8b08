// yk_pipeline.hip — a render call's launches: the kernels around the path kernels (the seed-walk
// warm-ups, the ordered reduce, the film folds) and the host code that plans, fills and enqueues
// them: the parameter checks and tile helpers, the processing order, the rings, launch().
//
// Replaces the reference's source.cpp:122-172 (for_each over (row,col) → transform_reduce over
// samples → to_color3b) and the recursion of yk/raytracer.hpp:19-37.
//
// Execution model:
//   * a render call is a sequence of LAUNCHES of K samples per pixel (a synced call: 4, 8, 16,
//     then at most kLaunchSpp = 32 for the frame: 1920x1080x512 is 4, 8, 16, 14 x 32, 18, 18; a
//     call enqueued while the previous one still runs: kLaunchSppOv = 64, 8 x 64; the rule is
//     yk_schedule.hpp's).  Per launch: yk_mt_warmup or yk_mt_warmup_defer (here; second stream:
//     every sample's mt19937 seeding walk and its start draws — jitter and lens — and camera ray,
//     as a StartRec), the path kernel (yk_render_persistent or yk_render_counting of
//     yk_render_f64.hip, yk_render_f32 of yk_render_f32.hip: the paths, on one of two top-priority
//     streams), then yk_reduce_samples (here: the reference's strictly sequential per-pixel sum
//     and to_color3b, third stream) or, for a film, yk_film_reduce / yk_film_reduce_masked.
//     Back-to-back calls overlap (launches numbered across calls).
//   * the blocks of the tile whose camera rays can hit nothing (sky blocks, yk_sky.hpp) are not in
//     the order those three kernels run over: yk_sky_samples (here, reduce stream) renders and
//     folds their samples, launch by launch (the production instance's one-shot calls only).
//   * a path kernel is one persistent grid of 768-thread workgroups, one per CU (12 waves,
//     3 per SIMD at 112 VGPRs, beside three 48-VGPR warm-up waves), with
//     the scene (BVH, geometry and material tables) in LDS, over SAMPLE SLOTS: a lane runs one path at a
//     time, one SEGMENT (closest hit + scatter) per trip round the loop, writes the sample's
//     colour when the path ends and takes the next slot from a wave-level reserve (one atomic
//     per 512 slots) — active-lane refill, so no lane idles while the launch has slots.
//   * the colour of a path is attenuation_1 * (attenuation_2 * (... * L)): double
//     multiplication does not associate, so the lane keeps the ids of the scattering spheres
//     on a small stack (8 in registers, the rest in a per-lane global spill) and multiplies
//     back to front at the end (raytracer.hpp:31).
//   * closest hit: a 4-wide BVH in LDS culls conservatively in float, the candidates' roots
//     are evaluated with the reference's exact arithmetic, ties to the later tuple index
//      — the result equals the reference's ordered scan bit for bit.
//   * every operation several lane kinds need runs once per trip for all of them (shared
//     canonical block, normalisation and second square root in shading): a wave pays for each
//     branch any of its lanes takes ("Uniform work per trip").
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "../../include/ykgpu.h"
#include "yk_film_internal.hpp"
#include "yk_host_internal.hpp"
#include "yk_schedule.hpp"
#include "yk_seed_table.hpp"
#include "yk_sky.hpp"

namespace {

// Seed walk and start of every sample of a launch, fully coherent, one sample per thread
// (grid-stride): the 397-step walk, then the start's draws with the lazy cursors (yk_device.hpp)
// and the camera ray, which thereby leave the divergent render loop.  kLens: the camera has a
// lens (the rejection loop is compiled only then: its registers cost co-resident waves); kF32:
// the FP32 kernel's start (one-word float canonicals, ykf::canonical; camera<float>).  The walk
// is ~400 dependent steps per sample (8.9e12 steps/s on the whole GPU, tools/walkbench.hip: 47 ms
// of a 512-spp frame if it ran alone), so these waves live on the render's idle issue cycles at
// lower priority.  One sample per thread (two or four interleaved: 204.6 -> 211.2 / 215.5 ms,
// 512-spp A/B): 32 VGPRs with a lens, so four of these waves fit beside the three 128-VGPR
// render waves of a SIMD (a record of the draws instead of the ray: 20 VGPRs and five waves,
// 0.5% slower, r03ab).
struct WarmArgs {
  uint32_t W, spp, seed0, row_begin, row_stride, s0, npix_slots, seed_mode, band_log2;
  uint32_t Wt, col_begin, col_stride, col_band;  // the tile's columns (as KernelArgs)
  uint32_t nps_m, nps_sh, w_m, w_sh;  // fdiv magic numbers of npix_slots and the tile width Wt
  uint32_t lens, H;                   // the camera has a lens (lens_radius > 0); image height
  uint64_t seed_key;
  yk_camera cam;
  CamF camf;
  double w_d, h_d, inv_w, inv_h;      // as in KernelArgs
  const uint32_t* order;
  uint64_t n;  // sample slots in the launch
  void* out;
  uint32_t* counter;  // the launch's sample-slot counter: cleared here (the render waits for this kernel)
  uint4* retry;         // yk_mt_warmup_defer: the lens retries, retry_cap records of 48 B per wave
  uint32_t retry_cap, retry_pad;
};

// The seed table's behaviours, as template instances (DESIGN.md §3 "Seed table"): kTabWalk is the
// walk alone; kTabFill walks and also stores each x_397 (the second consecutive eligible call
// of a key: the warm-ups and the sky kernel); kTabRead loads x_397 instead of walking (the sky kernel in the calls
// after it).  Everything after the walk is the same code.  The warm-ups have no reading instance:
// one was built and measured, and the render beside it slowed down by more than the walks cost
// (the frame 141 -> 150 ms; profiles/r23_seed_table/), so they keep walking.  Their
// fill instance stores every word all the same: a pixel it fills may be a sky pixel under the
// next camera.
constexpr int kTabWalk = 0, kTabFill = 1, kTabRead = 2;
constexpr uint64_t kNoTabIndex = ~0ull;  // (kTabFill) a slot without a pixel stores nothing
// the table as the kTabFill / kTabRead instances take it, behind the walking instances' own
// arguments (whose records, and so whose code, stay as they were): T its tile pixels
// (flip: xor-ed into every word the fill stores; 0 but under the test hook yk_seed_table_test)
struct SeedTab {
  uint32_t* tab;
  uint32_t T, flip;
};
struct WarmTabArgs {
  WarmArgs wa;
  SeedTab st;
};

// Thin-lens retries after the walks (yk_mt_warmup_defer): a sample whose first random_in_unit_disk candidate is
// rejected leaves its engine state (slot, seed, cursors, jitter canonicals) in its wave's ring and
// the wave draws the further candidates for 64 such samples at a time once its grid-stride walks
// are done, so no wave runs the rejection loop for its unluckiest lane (3.6 candidate draws per
// wave-sample against 1.27 per sample).  A sample that finds its wave's ring full is handed to the
// render as a start it makes itself (kNoStart), as a lens loop that runs out of lazy words is.
// records per wave: the rejections of the wave's slots (p = 1 - pi/4) + 6 sigma + a batch
inline uint32_t retry_cap_for(uint64_t slots_per_wave) {
  const double m = 0.2146 * (double)slots_per_wave, sd = std::sqrt(m * 0.7854);
  return ((uint32_t)(m + 6.0 * sd) + 64u + 63u) & ~63u;
}
__device__ __forceinline__ void retry_put(uint4* r, uint32_t i, const ykd::MtLane& g, double uc, double vc) {
  r[0] = make_uint4(i, g.seed, g.a0, g.a1);
  r[1] = make_uint4(g.b, g.j, 0u, 0u);
  *(double2*)(r + 2) = make_double2(uc, vc);
}
// (agent-scope relaxed loads: global_load ... sc1, past this CU's L1 — another lane of the wave
// wrote the record, and the ring's positions are rewritten)
__device__ __forceinline__ uint64_t ld_l2(const uint4* r, int k) {
  return __hip_atomic_load((const uint64_t*)r + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint32_t retry_get(const uint4* r, ykd::MtLane& g, double& uc, double& vc) {
  const uint64_t w0 = ld_l2(r, 0), w1 = ld_l2(r, 1), w2 = ld_l2(r, 2);
  g.state = nullptr;
  g.seed = (uint32_t)(w0 >> 32);
  g.a0 = (uint32_t)w1;
  g.a1 = (uint32_t)(w1 >> 32);
  g.b = (uint32_t)w2;
  g.j = (uint32_t)(w2 >> 32);
  uc = __longlong_as_double((long long)ld_l2(r, 4));
  vc = __longlong_as_double((long long)ld_l2(r, 5));
  return (uint32_t)w0;
}

// kIlp: the seed walks of kIlp slots interleaved per lane (i, i + stride, ...; the walk is a
// chain of dependent instructions), their starts then one after the other
template <bool kLens, bool kF32, bool kDefer, uint32_t kIlp, int kTab = kTabWalk>
__device__ __forceinline__ void mt_warmup_body(const WarmArgs& wa, const SeedTab& st = SeedTab{}) {
  static_assert(kTab == kTabWalk || (kTab == kTabFill && !kF32), "the FP64 production instance's warm-ups walk or fill");
  constexpr uint32_t kWarmBlock = 256;  // (every warm-up launches 256-thread blocks)
  // (32-bit indices: a launch keeps its slots below 2^31 and the grid below 2^21 threads)
  const uint32_t n = (uint32_t)wa.n;
  const uint32_t stride = gridDim.x * kWarmBlock;
  if (blockIdx.x == 0 && threadIdx.x == 0) *wa.counter = 0u;
  static_assert(!kDefer || (kLens && !kF32), "the deferred lens loop is the FP64 lens warm-up's");
  // kDefer: this wave's ring and how many records it holds (every lane of the wave enqueues in
  // step: a lane that has left the loop never holds the count alone, lane 0 leaves last)
  uint4* const ring =
      kDefer ? wa.retry + (size_t)__builtin_amdgcn_readfirstlane((blockIdx.x * kWarmBlock + threadIdx.x) >> 6) *
                              wa.retry_cap * 3
             : nullptr;
  uint32_t rcount = 0;
  // slot i's pixel (xx, y) and seed; an empty slot gets column kPadX (its record is marked).  ti
  // (kTabFill): the slot's word of the seed table; an empty slot stores none
  auto slot_seed = [&](uint32_t i, uint32_t& xx, uint32_t& y, uint64_t& ti) -> uint32_t {
    const uint32_t sl = fdiv(i, wa.nps_m, wa.nps_sh), pp = i - sl * wa.npix_slots;
    const uint32_t q = wa.order[pp];
    const uint32_t pix = q == kNoPixel ? 0u : q;
    const uint32_t tr = fdiv(pix, wa.w_m, wa.w_sh);
    xx = tile_col_x(wa.col_begin, wa.col_stride, wa.col_band, pix - tr * wa.Wt);
    y = tile_row_y(wa.row_begin, wa.row_stride, wa.band_log2, tr);
    const uint32_t seed = ykd::sample_seed(wa.seed_mode, wa.seed_key, wa.seed0, y, xx, wa.W, wa.spp, wa.s0 + sl);
    xx = q == kNoPixel ? kPadX : xx;
    if constexpr (kTab == kTabFill) ti = q == kNoPixel ? kNoTabIndex : ykseed::table_index(wa.s0 + sl, pix, st.T);
    return seed;
  };
  // the start of slot i after its walk: draws, lens, camera ray, record
  auto start_slot = [&](uint32_t i, uint32_t xx, uint32_t y, uint32_t seed, uint32_t x397) {
    ykd::MtLane g;
    g.state = nullptr;
    ykd::mt_start_from(g, seed, x397);
    bool failed = false;  // the lens loop would reach the scratch engine's words
    if constexpr (kF32) {
      const float uc = ykf::canonical<true>(g);  // source.cpp:162 with T = float
      const float vc = ykf::canonical<true>(g);  // source.cpp:163
      float px = 0.0f, py = 0.0f;
      if (kLens) {
        for (;;) {  // thin-lens extension: random_in_unit_disk by rejection, x then y
          if (!ykd::rng_lazy_ok(g, 2)) {
            failed = true;
            break;
          }
          px = ykf::uniform_of(ykf::canonical<true>(g), -1.0f, 1.0f);
          py = ykf::uniform_of(ykf::canonical<true>(g), -1.0f, 1.0f);
          if (px * px + py * py < 1.0f) break;
        }
      }
      ykf::v3 o, d;
      camera_ray_f32(wa.camf, wa.H, xx, y, uc, vc, kLens, px, py, o, d);
      uint4* const out = (uint4*)wa.out + 3 * (size_t)i;
      *(float4*)out = make_float4(o.x, o.y, o.z, d.x);
      *(float4*)(out + 1) = make_float4(d.y, d.z, 0.0f, 0.0f);
      out[2] = make_uint4(g.a0, g.a1, g.b, xx == kPadX ? kPadSlot : failed ? kNoStart : g.j);
    } else {
      const double uc = ykd::canonical<true>(g);  // source.cpp:162
      const double vc = ykd::canonical<true>(g);  // source.cpp:163
      double px = 0.0, py = 0.0;
      if constexpr (kDefer) {
        // the first candidate in line; a rejected sample goes to the ring while it has room
        bool again = false;
        if (!ykd::rng_lazy_ok(g, 4)) {
          failed = true;
        } else {
          px = ykd::uniform<true>(g, -1, 1);
          py = ykd::uniform<true>(g, -1, 1);
          again = !(px * px + py * py < 1.0);
        }
        const unsigned long long m = __ballot(again);
        const uint32_t nq = (uint32_t)__popcll(m);
        const bool room = rcount + nq <= wa.retry_cap;
        if (room) {
          if (again) {
            const uint32_t pos = rcount + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
            retry_put(ring + 3 * pos, i, g, uc, vc);
          }
          rcount += nq;
          if (again) return;
        } else if (again) {
          failed = true;  // (the ring is full: the render kernel starts this sample itself)
        }
      } else if (kLens) {
        for (;;) {
          if (!ykd::rng_lazy_ok(g, 4)) {
            failed = true;
            break;
          }
          px = ykd::uniform<true>(g, -1, 1);
          py = ykd::uniform<true>(g, -1, 1);
          if (px * px + py * py < 1.0) break;
        }
      }
      v3 o, d;
      camera_ray(wa.cam, wa.w_d, wa.inv_w, wa.h_d, wa.inv_h, wa.H, xx, y, uc, vc, kLens, px, py, o, d);
      uint4* const out = (uint4*)wa.out + 4 * (size_t)i;
      *(double2*)out = make_double2(o.x, o.y);
      *(double2*)(out + 1) = make_double2(o.z, d.x);
      *(double2*)(out + 2) = make_double2(d.y, d.z);
      out[3] = make_uint4(g.a0, g.a1, g.b, xx == kPadX ? kPadSlot : failed ? kNoStart : g.j);
    }
  };
  if constexpr (kIlp > 1) {
    for (uint32_t i = blockIdx.x * kWarmBlock + threadIdx.x; i < n; i += kIlp * stride) {
      uint32_t xx, y, x[kIlp];
      uint64_t ti = 0, tk = 0;
#pragma unroll
      for (uint32_t k = kIlp - 1; k > 0; --k) {
        const uint32_t ik = i + k * stride;
        x[k] = slot_seed(ik < n ? ik : i, xx, y, tk);
      }
      const uint32_t seed = slot_seed(i, xx, y, ti);
      x[0] = seed;
      ykd::mt_walk397xn<kIlp>(x);
      if constexpr (kTab == kTabFill)
        if (ti != kNoTabIndex) st.tab[ti] = (x[0] ^ st.flip);
      start_slot(i, xx, y, seed, x[0]);
#pragma unroll
      for (uint32_t k = 1; k < kIlp; ++k) {
        const uint32_t ik = i + k * stride;
        if (ik < n) {
          const uint32_t sk = slot_seed(ik, xx, y, tk);
          if constexpr (kTab == kTabFill)
            if (tk != kNoTabIndex) st.tab[tk] = (x[k] ^ st.flip);
          start_slot(ik, xx, y, sk, x[k]);
        }
      }
    }
  } else {
    for (uint32_t i = blockIdx.x * kWarmBlock + threadIdx.x; i < n; i += stride) {
      uint32_t xx, y;
      uint64_t ti = 0;
      const uint32_t seed = slot_seed(i, xx, y, ti);
      uint32_t x[1] = {seed};
      ykd::mt_walk397xn<1>(x);
      if constexpr (kTab == kTabFill)
        if (ti != kNoTabIndex) st.tab[ti] = (x[0] ^ st.flip);
      start_slot(i, xx, y, seed, x[0]);
    }
  }
  if constexpr (kDefer) {
    // the ring: one more candidate for up to 64 records per trip, the rejected re-queued at its end
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t head = 0, cnt = __builtin_amdgcn_readfirstlane(rcount);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the records are in L2
    while (cnt > 0u) {
      const uint32_t take = min(cnt, 64u);
      const bool act = lane < take;
      ykd::MtLane g;
      double uc = 0, vc = 0, px = 0, py = 0;
      uint32_t i = 0;
      bool again = false, failed = false;
      if (act) {
        uint32_t pos = head + lane;
        pos = pos >= wa.retry_cap ? pos - wa.retry_cap : pos;
        i = retry_get(ring + 3 * pos, g, uc, vc);
        if (!ykd::rng_lazy_ok(g, 4)) {
          failed = true;
        } else {
          px = ykd::uniform<true>(g, -1, 1);
          py = ykd::uniform<true>(g, -1, 1);
          again = !(px * px + py * py < 1.0);
        }
      }
      head += take;
      head = head >= wa.retry_cap ? head - wa.retry_cap : head;
      cnt -= take;
      const unsigned long long m = __ballot(again);
      if (again) {
        uint32_t pos = head + cnt + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
        pos = pos >= wa.retry_cap ? pos - wa.retry_cap : pos;
        retry_put(ring + 3 * pos, i, g, uc, vc);
      }
      cnt += (uint32_t)__popcll(m);
      if (act && !again) {
        const uint32_t sl = fdiv(i, wa.nps_m, wa.nps_sh), pp = i - sl * wa.npix_slots;
        const uint32_t q = wa.order[pp];
        const uint32_t pix = q == kNoPixel ? 0u : q;
        const uint32_t tr = fdiv(pix, wa.w_m, wa.w_sh);
        const uint32_t xx = tile_col_x(wa.col_begin, wa.col_stride, wa.col_band, pix - tr * wa.Wt);
        const uint32_t y = tile_row_y(wa.row_begin, wa.row_stride, wa.band_log2, tr);
        uint4* const out = (uint4*)wa.out + 4 * (size_t)i;
        out[3] = make_uint4(g.a0, g.a1, g.b, q == kNoPixel ? kPadSlot : failed ? kNoStart : g.j);
        v3 o, d;
        camera_ray(wa.cam, wa.w_d, wa.inv_w, wa.h_d, wa.inv_h, wa.H, xx, y, uc, vc, kLens, px, py, o, d);
        *(double2*)out = make_double2(o.x, o.y);
        *(double2*)(out + 1) = make_double2(o.z, d.x);
        *(double2*)(out + 2) = make_double2(d.y, d.z);
      }
      if (cnt > 0u) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
  }
}

// one walk per lane (the deferred FP64 lens warm-up below walks kWalkIlp slots at once)
template <bool kLens, bool kF32>
__global__ __launch_bounds__(256) void yk_mt_warmup(WarmArgs wa) {
  mt_warmup_body<kLens, kF32, false, 1>(wa);
}
// the FP64 lens warm-up with its retries deferred, at 48 VGPRs: two of its waves beside the three
// 128-VGPR render waves of a SIMD (the attribute counts gfx950's unified register file: twice)
__global__ __launch_bounds__(256) __attribute__((amdgpu_num_vgpr(YK_DEFER_VGPRS / 2))) void yk_mt_warmup_defer(WarmArgs wa) {
  mt_warmup_body<true, false, true, kWalkIlp>(wa);
}
// the FP64 warm-ups of a call that fills the seed table (kTabFill): the same
// grids, blocks and register budget as the walking instances above
template <bool kLens, int kTab>
__global__ __launch_bounds__(256) void yk_mt_warmup_tab(WarmTabArgs ta) {
  mt_warmup_body<kLens, false, false, 1, kTab>(ta.wa, ta.st);
}
template <int kTab>
__global__ __launch_bounds__(256) __attribute__((amdgpu_num_vgpr(YK_DEFER_VGPRS / 2))) void yk_mt_warmup_defer_tab(WarmTabArgs ta) {
  mt_warmup_body<true, false, true, kWalkIlp, kTab>(ta.wa, ta.st);
}

// Ordered sum of a launch's sample colours per pixel: pixel_color of source.cpp:137-167 is the
// left fold ((0 + c_0) + c_1) + ... in sample order, continued across launches through acc; after
// the last launch, to_color3b (source.cpp:73-83): /spp, math::sqrt, clamp [0, .999], *256,
// truncate.  One thread per processing slot, coalesced over the SoA colours.
struct ReduceArgs {
  const double* col;  // col[(s_local * npix_slots + p) * kColStride + c]
  double* acc;        // running sums, acc[c * npix_slots + p]
  const uint32_t* order;
  uint8_t* rgb;
  double* sums;
  uint32_t npix_slots, nsl, ks, spp;
  uint32_t first, last, pad0, pad1;
};
// tile pixel q's sums after its last sample: the sums themselves when asked for, and to_color3b
__device__ __forceinline__ void pixel_store(double* sums, uint8_t* rgb, uint32_t q, const double (&a)[3],
                                            uint32_t spp_u) {
  const size_t o3 = (size_t)q * 3;
  const double spp = (double)spp_u;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    if (sums) sums[o3 + c] = a[c];
    double v = ykd::nsqrt(a[c] / spp);
    v = (v < 0.0) ? 0.0 : (0.999 < v) ? 0.999 : v;
    rgb[o3 + c] = (uint8_t)(uint32_t)(v * 256);
  }
}
__device__ __forceinline__ void reduce_slot(const ReduceArgs& ra, uint32_t p) {
  const uint32_t q = ra.order[p];
  if (q == kNoPixel) return;
  double a[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) a[c] = ra.first ? 0.0 : ra.acc[(size_t)c * ra.npix_slots + p];
  for (uint32_t k = 0; k < ra.ks; ++k) {
    const size_t i = (size_t)k * ra.npix_slots + p;
#pragma unroll
    for (int c = 0; c < 3; ++c) a[c] = a[c] + ra.col[i * kColStride + c];
  }
  if (!ra.last) {
#pragma unroll
    for (int c = 0; c < 3; ++c) ra.acc[(size_t)c * ra.npix_slots + p] = a[c];
    return;
  }
  pixel_store(ra.sums, ra.rgb, q, a, ra.spp);
}
__global__ __launch_bounds__(256) void yk_reduce_samples(ReduceArgs ra) {
  for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p < ra.npix_slots; p += gridDim.x * blockDim.x)
    reduce_slot(ra, p);
}

// The samples of a launch for the pixels of the SKY BLOCKS (yk_sky.hpp): no camera ray
// of such a pixel can hit a sphere, so a sample is the sky of its camera ray (raytracer.hpp:35-36)
// and needs neither a start record, a slot of the path kernel nor a colour record.  One thread per
// sky slot runs the pixel's samples [s0, s0 + ks) in sample order: the warm-up's seed and walk
// (kWalkIlp consecutive samples of the pixel interleaved), the two jitter canonicals, the lens
// rejection loop, camera_ray, then the path kernel's own sky expression (yk_render_f64.hip: the
// shared normalisation's nsqrt and range-checked division, t = (un.y + 1) / 2, the three lerps) and
// the fold a = a + c that yk_reduce_samples performs, carried from launch to launch in acc; after
// the last launch pixel_store.  A pixel with a lens loop that outruns the lazy cursors (never seen:
// ~55 rejections) is left to yk_sky_redo.  Counter seeds only.  The warm-up's register budget: its waves share the SIMDs
// with the render's the same way.
struct SkyArgs {
  uint32_t W, H, spp, seed0, row_begin, row_stride, band_log2;
  uint32_t Wt, col_begin, col_stride, col_band;
  uint32_t w_m, w_sh;  // fdiv magic numbers of the tile width
  uint32_t lens, s0, ks, first, last;
  uint32_t n;  // sky slots
  yk_camera cam;
  double w_d, h_d, inv_w, inv_h;
  const uint32_t* list;  // sky slot → tile pixel (kNoPixel: empty slot of an edge block)
  double* acc;           // running sums, acc[c * n + p]
  uint8_t* rgb;
  double* sums;
  uint32_t* engines;             // [0]: slots listed for yk_sky_redo, [1, 1 + n): the list, then its 64 engines
  unsigned long long* counters;  // [3]: MT fallbacks
};
struct SkyTabArgs {
  SkyArgs sa;
  SeedTab st;
};
// the sky of the camera ray of pixel (xx, y) for the start's draws, added to the pixel's sums
__device__ __forceinline__ void sky_add(const SkyArgs& sa, uint32_t xx, uint32_t y, double uc, double vc, double px,
                                        double py, double (&a)[3]) {
  v3 o, d;
  camera_ray(sa.cam, sa.w_d, sa.inv_w, sa.h_d, sa.inv_h, sa.H, xx, y, uc, vc, sa.lens != 0, px, py, o, d);
  // sky (raytracer.hpp:35-36), as the path kernel's shade block computes it
  const double len = ykd::nsqrt(ykd::len2(d));
  const v3 un = ykd::divs_fast(d, len);
  const double t = (un.y + 1.0) / 2;
  a[0] = a[0] + ((1.0 - t) * 1.0 + t * 0.5);
  a[1] = a[1] + ((1.0 - t) * 1.0 + t * 0.7);
  a[2] = a[2] + ((1.0 - t) * 1.0 + t * 1.0);
}
// words the lens loop may draw from the lazy cursors (a test build lowers it, Makefile
// libykgpu_skylazy%.so: the pixels it lists then run yk_sky_redo, tests/test_gpu_fallbacks.py)
#ifdef YK_SKY_LAZY_FORCE
constexpr uint32_t kSkyLazyWords = YK_SKY_LAZY_FORCE;
#else
constexpr uint32_t kSkyLazyWords = ykd::kLazyDraws;
#endif
// kTab: the seed table, as the warm-up's (kTabFill stores the x_397 of the samples it walks, also
// those of a pixel it leaves to yk_sky_redo; kTabRead loads them)
template <int kTab>
__device__ __forceinline__ void sky_samples_body(const SkyArgs& sa, uint32_t* const tab = nullptr, const uint32_t tab_T = 0,
                                                 const uint32_t flip = 0) {
  const uint32_t p = blockIdx.x * 256u + threadIdx.x;
  if (p >= sa.n) return;
  const uint32_t q = sa.list[p];
  if (q == kNoPixel) return;
  const uint32_t tr = fdiv(q, sa.w_m, sa.w_sh);
  const uint32_t xx = tile_col_x(sa.col_begin, sa.col_stride, sa.col_band, q - tr * sa.Wt);
  const uint32_t y = tile_row_y(sa.row_begin, sa.row_stride, sa.band_log2, tr);
  // (the counter seed of sample s0; sample s0 + k is this + k in uint32 arithmetic)
  const uint32_t seed_s0 = ykd::sample_seed(0u, 0ull, sa.seed0, y, xx, sa.W, sa.spp, sa.s0);
  double a[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) a[c] = sa.first ? 0.0 : sa.acc[(size_t)c * sa.n + p];
  for (uint32_t k = 0; k < sa.ks; k += kWalkIlp) {
    uint32_t x[kWalkIlp];
#pragma unroll
    for (uint32_t j = 0; j < kWalkIlp; ++j) x[j] = seed_s0 + k + j;  // (past ks: walked, not used)
    if constexpr (kTab == kTabRead) {
#pragma unroll
      for (uint32_t j = 0; j < kWalkIlp; ++j)
        if (k + j < sa.ks) x[j] = tab[ykseed::table_index(sa.s0 + k + j, q, tab_T)];
    } else {
      ykd::mt_walk397xn<kWalkIlp>(x);
      if constexpr (kTab == kTabFill) {
#pragma unroll
        for (uint32_t j = 0; j < kWalkIlp; ++j)
          if (k + j < sa.ks) tab[ykseed::table_index(sa.s0 + k + j, q, tab_T)] = (x[j] ^ flip);
      }
    }
#pragma unroll
    for (uint32_t j = 0; j < kWalkIlp; ++j) {
      if (k + j >= sa.ks) break;
      ykd::MtLane g;
      g.state = nullptr;
      ykd::mt_start_from(g, seed_s0 + k + j, x[j]);
      const double uc = ykd::canonical<true>(g);  // source.cpp:162
      const double vc = ykd::canonical<true>(g);  // source.cpp:163
      double px = 0.0, py = 0.0;
      if (sa.lens) {
        for (;;) {  // thin-lens extension: random_in_unit_disk by rejection, x then y
          if (g.j + 4 > kSkyLazyWords) {
            // (never seen) the lens loop outran the lazy cursors: the pixel keeps its carried sums
            // and yk_sky_redo runs this launch's samples of it from a whole engine
            sa.engines[1 + atomicAdd(sa.engines, 1u)] = p;
            if constexpr (kTab == kTabFill) {
              // (the table still gets the launch's other samples of the pixel)
              for (uint32_t k2 = k + kWalkIlp; k2 < sa.ks; k2 += kWalkIlp) {
                uint32_t x2[kWalkIlp];
#pragma unroll
                for (uint32_t j2 = 0; j2 < kWalkIlp; ++j2) x2[j2] = seed_s0 + k2 + j2;
                ykd::mt_walk397xn<kWalkIlp>(x2);
#pragma unroll
                for (uint32_t j2 = 0; j2 < kWalkIlp; ++j2)
                  if (k2 + j2 < sa.ks) tab[ykseed::table_index(sa.s0 + k2 + j2, q, tab_T)] = (x2[j2] ^ flip);
              }
            }
            return;
          }
          px = ykd::uniform<true>(g, -1, 1);
          py = ykd::uniform<true>(g, -1, 1);
          if (px * px + py * py < 1.0) break;
        }
      }
      sky_add(sa, xx, y, uc, vc, px, py, a);
    }
  }
  if (!sa.last) {
#pragma unroll
    for (int c = 0; c < 3; ++c) sa.acc[(size_t)c * sa.n + p] = a[c];
    return;
  }
  pixel_store(sa.sums, sa.rgb, q, a, sa.spp);
}
__global__ __launch_bounds__(256) __attribute__((amdgpu_num_vgpr(YK_DEFER_VGPRS / 2))) void yk_sky_samples(SkyArgs sa) {
  sky_samples_body<kTabWalk>(sa);
}
template <int kTab>
__global__ __launch_bounds__(256) __attribute__((amdgpu_num_vgpr(YK_DEFER_VGPRS / 2))) void yk_sky_samples_tab(SkyTabArgs ta) {
  sky_samples_body<kTab>(ta.sa, ta.st.tab, ta.st.T, ta.st.flip);
}
// The sky slots yk_sky_samples listed (never seen: a lens loop of ~55 rejections): this launch's
// samples of each from the carried sums, every draw from a whole engine in global memory, seeded
// and twisted as random.hpp:69-81, 114-131 do, one engine per thread of the one block.  A sample
// that drew past the lazy cursors' words counts as an MT fallback, as a start the render makes
// itself would.  Clears the list.  (The same register budget: its one wave, which almost always
// finds the list empty, must fit beside the render's and the warm-up's waves without waiting.)
__global__ __launch_bounds__(64) __attribute__((amdgpu_num_vgpr(YK_DEFER_VGPRS / 2))) void yk_sky_redo(SkyArgs sa) {
  const uint32_t count = sa.engines[0];
  uint32_t fallbacks = 0;
  ykd::MtFull g;
  g.st = sa.engines + 1 + sa.n + (size_t)threadIdx.x * ykd::kMtN;
  for (uint32_t e = threadIdx.x; e < count; e += 64u) {
    const uint32_t p = sa.engines[1 + e], q = sa.list[p];
    const uint32_t tr = fdiv(q, sa.w_m, sa.w_sh);
    const uint32_t xx = tile_col_x(sa.col_begin, sa.col_stride, sa.col_band, q - tr * sa.Wt);
    const uint32_t y = tile_row_y(sa.row_begin, sa.row_stride, sa.band_log2, tr);
    double a[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) a[c] = sa.first ? 0.0 : sa.acc[(size_t)c * sa.n + p];
    for (uint32_t k = 0; k < sa.ks; ++k) {
      ykd::mt_full_seed(g, ykd::sample_seed(0u, 0ull, sa.seed0, y, xx, sa.W, sa.spp, sa.s0 + k));
      const double uc = ykd::canonical(g);
      const double vc = ykd::canonical(g);
      double px, py;
      do {  // (only a lens loop comes here)
        px = ykd::uniform(g, -1, 1);
        py = ykd::uniform(g, -1, 1);
      } while (!(px * px + py * py < 1.0));
      if (g.n > ykd::kLazyDraws) ++fallbacks;
      sky_add(sa, xx, y, uc, vc, px, py, a);
    }
    if (sa.last) {
      pixel_store(sa.sums, sa.rgb, q, a, sa.spp);
    } else {
#pragma unroll
      for (int c = 0; c < 3; ++c) sa.acc[(size_t)c * sa.n + p] = a[c];
    }
  }
  if (fallbacks) atomicAdd(&sa.counters[3], (unsigned long long)fallbacks);
  __syncthreads();
  if (threadIdx.x == 0) sa.engines[0] = 0u;
}

// The whole processing order split into the path's and the sky list (ensure_sky): block b's per
// slots go to place off[b] of the order its bit 31 names.
__global__ __launch_bounds__(256) void yk_sky_split(const uint32_t* order, const uint32_t* off, uint32_t* path,
                                                    uint32_t* list, uint32_t n, uint32_t per) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const uint32_t b = i / per, o = off[b];
  ((o & 0x80000000u) ? list : path)[(size_t)(o & 0x7fffffffu) * per + (i - b * per)] = order[i];
}

// A launch's sample colours folded into a film: s = s + c (the reference's left fold, continued
// from the film's sums: carry-in and carry-out are the planes) and q = q + (c * c), per sample in
// sample order.  A new film's planes are zero, so its first launch computes (0 + c_0) like
// yk_reduce_samples' `first`.  Slots without a pixel keep their zeros.
struct FilmReduceArgs {
  const double* col;  // as ReduceArgs::col
  double* plane;
  const uint32_t* order;  // the film's own
  uint32_t npix_slots, ks;
};
__global__ __launch_bounds__(256) void yk_film_reduce(FilmReduceArgs fa) {
  for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p < fa.npix_slots; p += gridDim.x * blockDim.x) {
    if (fa.order[p] == kNoPixel) continue;
    double s[3], q[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      s[c] = fa.plane[(size_t)c * fa.npix_slots + p];
      q[c] = fa.plane[(size_t)(3 + c) * fa.npix_slots + p];
    }
    for (uint32_t k = 0; k < fa.ks; ++k) {
      const double* rec = fa.col + ((size_t)k * fa.npix_slots + p) * kColStride;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const double v = rec[c];
        s[c] = film_add(s[c], v);
        q[c] = film_add(q[c], film_mul(v, v));
      }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      fa.plane[(size_t)c * fa.npix_slots + p] = s[c];
      fa.plane[(size_t)(3 + c) * fa.npix_slots + p] = q[c];
    }
  }
}

// yk_film_reduce for a group: slot a of the group's order reads its ks colours at the group's
// stride and carries in and out of the film's planes at slot map[a], whose count grows by ks.
struct FilmMaskedArgs {
  const double* col;  // col[(s_local * g_slots + a) * kColStride + c]
  double* plane;
  uint32_t* count;
  uint32_t* take;       // the group's last launch: the slot's take is cleared (it has left the group's count)
  const uint32_t* map;  // group slot → film slot, kNoPixel for the padding
  uint32_t npix_slots, g_slots, ks, pad;
};
__global__ __launch_bounds__(256) void yk_film_reduce_masked(FilmMaskedArgs fa) {
  for (uint32_t a = blockIdx.x * blockDim.x + threadIdx.x; a < fa.g_slots; a += gridDim.x * blockDim.x) {
    const uint32_t p = fa.map[a];
    if (p >= fa.npix_slots) continue;  // (padding)
    double s[3], q[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      s[c] = fa.plane[(size_t)c * fa.npix_slots + p];
      q[c] = fa.plane[(size_t)(3 + c) * fa.npix_slots + p];
    }
    for (uint32_t k = 0; k < fa.ks; ++k) {
      const double* rec = fa.col + ((size_t)k * fa.g_slots + a) * kColStride;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const double v = rec[c];
        s[c] = film_add(s[c], v);
        q[c] = film_add(q[c], film_mul(v, v));
      }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      fa.plane[(size_t)c * fa.npix_slots + p] = s[c];
      fa.plane[(size_t)(3 + c) * fa.npix_slots + p] = q[c];
    }
    fa.count[p] += fa.ks;
    if (fa.take) fa.take[p] = 0u;
  }
}

}  // namespace

// =========================================================================================
// Host side (the functions other units call are declared in yk_host_internal.hpp)
// =========================================================================================
// (the host-side tuning constants and the launch schedule rule: yk_schedule.hpp)
// the render kernel addresses a slot's start record as 4 * slot uint4s (FP32: 3) in 32-bit
// arithmetic
static_assert(kLaunchBytes / (8 * kColStride) * 4 < (1ull << 32), "4 * slot must fit 32 bits");
static_assert(yksched::kColourBytes == kColStride * sizeof(double), "yk_schedule.hpp's colour record");

namespace ykhost {

uint64_t host_row_y(const yk_render_params* p, uint32_t t) {
  const uint32_t L = p->row_band_log2;
  return (uint64_t)p->row_begin + ((((uint64_t)(t >> L)) * p->row_stride) << L) + (t & ((1u << L) - 1u));
}

// The tile's width: its column set's size, or the image width (col_count == 0)
uint32_t tile_width(const yk_render_params* p) { return p->col_count ? p->col_count : p->image_width; }
uint64_t host_col_x(const yk_render_params* p, uint32_t j) {
  if (!p->col_count) return j;
  const uint32_t L = p->col_band_log2;
  return (uint64_t)p->col_begin + ((((uint64_t)(j >> L)) * p->col_stride) << L) + (j & ((1u << L) - 1u));
}

// Magic numbers of fdiv (kernel side) for a divisor 1 <= d < 2^31
static void fastdiv(uint32_t d, uint32_t& m, uint32_t& sh) {
  uint32_t l = 0;
  while ((1ull << l) < d) ++l;
  sh = 31 + l;
  m = (uint32_t)(((1ull << sh) + d - 1) / d);
}

int check_params(const ykgpu_context* ctx, const yk_render_params* p) {
  if (!ctx || !p) return fail(YK_ERR_INVALID, "null context or params");
  if (!ctx->have_scene) return fail(YK_ERR_NO_SCENE, "ykgpu_set_scene was not called");
  if (!p->image_width || !p->image_height || !p->samples_per_pixel)
    return fail(YK_ERR_INVALID, "image_width, image_height and samples_per_pixel must be > 0");
  if (!p->row_count) return fail(YK_ERR_INVALID, "row_count must be > 0");
  if (!p->row_stride) return fail(YK_ERR_INVALID, "row_stride must be > 0");
  if (p->row_band_log2 > 10) return fail(YK_ERR_INVALID, "row_band_log2 must be <= 10");
  if (host_row_y(p, p->row_count - 1) >= p->image_height) return fail(YK_ERR_INVALID, "row range outside the image");
  if (p->col_count) {
    if (!p->col_stride) return fail(YK_ERR_INVALID, "col_stride must be > 0");
    if (p->col_band_log2 > 10) return fail(YK_ERR_INVALID, "col_band_log2 must be <= 10");
    if (host_col_x(p, p->col_count - 1) >= p->image_width) return fail(YK_ERR_INVALID, "column range outside the image");
  } else if (p->col_begin || p->col_stride || p->col_band_log2) {
    return fail(YK_ERR_INVALID, "col_count == 0 (every column) needs col_begin, col_stride, col_band_log2 == 0");
  }
  if ((uint64_t)p->row_count * tile_width(p) >= (1ull << 31))
    return fail(YK_ERR_INVALID, "tile larger than 2^31 pixels");
  if (p->precision != YK_PRECISION_FP64 && p->precision != YK_PRECISION_FP32)
    return fail(YK_ERR_UNSUPPORTED, "precision mode");
  if (p->rng != YK_RNG_MT19937 && p->rng != YK_RNG_XOR128) return fail(YK_ERR_UNSUPPORTED, "rng mode");
  if (p->seed_mode != YK_SEED_COUNTER && p->seed_mode != YK_SEED_RANDOM_DEVICE)
    return fail(YK_ERR_UNSUPPORTED, "seed mode");
  if (!(p->t_min >= 0)) return fail(YK_ERR_INVALID, "t_min must be >= 0");
  // the one-lane diagnostic exists only in the FP64 counting instance: anywhere else it would be
  // ignored and a profile reconciled against the one-lane model would read all-lane counters
  if ((p->flags & YK_FLAG_ONE_LANE) &&
      (!(p->flags & YK_FLAG_COUNT_WORK) || p->precision != YK_PRECISION_FP64))
    return fail(YK_ERR_INVALID, "YK_FLAG_ONE_LANE needs YK_FLAG_COUNT_WORK and FP64");
  return YK_OK;
}

// Waits for every stream of the context: before a buffer that an earlier call's kernels may still
// use is freed (with cross-call pipelining a call's first launches run beside the previous call's
// last ones, launch())
static int quiesce(ykgpu_context* ctx) {
  for (hipStream_t s : {ctx->aux, ctx->red, ctx->ren, ctx->alt, ctx->stream}) YK_HIP(hipStreamSynchronize(s));
  return YK_OK;
}

static int ensure_scratch(ykgpu_context* ctx, uint32_t max_depth, size_t lanes, bool need_mt) {
  // mt19937 fallback engines: 624 words per persistent lane (not needed by xor128)
  if (need_mt && (lanes > ctx->scratch_lanes || !ctx->d_mt)) {
    if (int rc = quiesce(ctx)) return rc;
    (void)hipFree(ctx->d_mt);
    ctx->d_mt = nullptr;
    ctx->scratch_lanes = 0;
    YK_HIP(hipMalloc(&ctx->d_mt, 2 * lanes * ykd::kMtN * sizeof(uint32_t)));  // two launches in flight
    ctx->scratch_lanes = lanes;
  }
  // attenuation-id spill: max_depth u16 per lane
  const uint32_t need = max_depth > kStackRegs ? max_depth : 1;
  if (need > ctx->id_stride || lanes > ctx->id_lanes || !ctx->d_ids) {
    if (int rc = quiesce(ctx)) return rc;
    if (ctx->d_ids) YK_HIP(hipFree(ctx->d_ids));
    ctx->d_ids = nullptr;
    ctx->id_stride = 0;
    ctx->id_lanes = 0;
    YK_HIP(hipMalloc(&ctx->d_ids, 2 * lanes * need * sizeof(uint16_t)));
    ctx->id_stride = need;
    ctx->id_lanes = lanes;
  }
  return YK_OK;
}

// The processing order of a tile of W x rows pixels (kernel comment at kNoPixel).  A function of
// the geometry only, so it is built once per size and kept on the device.  Blocks hold 64 tile
// pixels; for a tile of every stride-th image row (the N-GPU split) they are widened and
// flattened so that a block still covers a roughly square patch of the IMAGE (stride 1: 8 x 8;
// 2: 16 x 4 tile rows = 16 x 8 image rows; 4: 16 x 4 = 16 x 16; 8: 32 x 2 = 32 x 16): the rays a
// wave starts together stay coherent (8 x 8 tile blocks of a 4-way tile, 8 x 32 image pixels,
// cost 17% more per sample, measured).
uint32_t order_mode() {
  // (A/B knob: YKGPU_ORDER=1 takes the block rows bottom-up)
  const char* oe = ab_knob("YKGPU_ORDER");
  return oe ? (uint32_t)std::atoi(oe) : 0u;
}
// image rows per tile row, for the shape of the processing blocks (bands of >= 8 rows: 1, an
// 8 x 8 block stays inside one band)
uint32_t order_stride(const yk_render_params* p) {
  return p->row_count > 1 && p->row_band_log2 < 3 ? p->row_stride : 1;
}
std::vector<uint32_t> build_order(uint32_t W, uint32_t rows, uint32_t stride, uint32_t mode) {
  std::vector<uint32_t> ord;
  if (kTile == 0) {
    ord.resize((size_t)W * rows);
    for (size_t i = 0; i < ord.size(); ++i) ord[i] = (uint32_t)i;
  } else {
    uint32_t tw, th;
    order_block(stride, tw, th);
    const uint32_t bx = (W + tw - 1) / tw, by = (rows + th - 1) / th;
    ord.reserve((size_t)bx * by * tw * th);
    for (uint32_t jj = 0; jj < by; ++jj)
      for (uint32_t i = 0; i < bx; ++i)
        for (uint32_t k = 0; k < tw * th; ++k) {
          const uint32_t j = mode == 1 ? by - 1 - jj : jj;
          const uint32_t x = i * tw + k % tw, y = j * th + k / tw;
          ord.push_back(x < W && y < rows ? y * W + x : kNoPixel);
        }
  }
  return ord;
}
static int ensure_order(ykgpu_context* ctx, uint32_t W, uint32_t rows, uint32_t stride) {
  const uint32_t mode = order_mode();
  if (ctx->d_order && ctx->order_w == W && ctx->order_rows == rows && ctx->order_stride == stride &&
      ctx->order_mode == mode)
    return YK_OK;
  const std::vector<uint32_t> ord = build_order(W, rows, stride, mode);
  if (int rc = quiesce(ctx)) return rc;
  (void)hipFree(ctx->d_order);
  ctx->d_order = nullptr;
  ctx->order_w = ctx->order_rows = ctx->order_slots = 0;
  YK_HIP(hipMalloc(&ctx->d_order, ord.size() * sizeof(uint32_t)));
  YK_HIP(hipMemcpy(ctx->d_order, ord.data(), ord.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
  ctx->order_w = W;
  ctx->order_rows = rows;
  ctx->order_stride = stride;
  ctx->order_mode = mode;
  ctx->order_slots = (uint32_t)ord.size();
  return YK_OK;
}

// Sky blocks (yk_sky.hpp).  The production instance alone takes them: FP64, mt19937,
// counter seeds, no flags, a scene in LDS, a one-shot call (every launch() of the render entry
// points and of a device group renders its whole tile).  Everything else — the counting, trace,
// linear-scan and one-lane instances, random-device seeds, xor128, FP32, films, max_depth 0 (a
// black image, not sky) — keeps the whole processing order.  (A/B knob: YKGPU_SKY=0.)
static bool sky_eligible(const yk_render_params* p, const ykgpu_film* film, const DevTree::Plan& plan) {
  if (const char* e = ab_knob("YKGPU_SKY"))
    if (std::atoi(e) == 0) return false;
  return kTile != 0 && !film && p->precision == YK_PRECISION_FP64 && p->rng == YK_RNG_MT19937 &&
         p->seed_mode == YK_SEED_COUNTER && p->flags == 0 && p->max_depth > 0 && plan.in_lds;
}
// Seed table (yk_seed_table.hpp): the same production instance, whatever its scene
// and camera — FP64, mt19937, counter seeds, no flags, a one-shot call, which always covers the
// samples [0, spp) of its tile.  FP32, xor128, random-device seeds, the counting, trace and
// linear-scan instances and every film pass neither read nor write it.
// (test hook yk_seed_table_test, below: the word xor-ed into what a fill stores)
static std::atomic<uint32_t> g_seed_tab_flip{0};
static bool seed_table_eligible(const ykgpu_context* ctx, const yk_render_params* p, const ykgpu_film* film,
                                uint32_t s_begin, uint32_t s_end) {
  return ctx->seed_tab_on && !film && p->precision == YK_PRECISION_FP64 && p->rng == YK_RNG_MT19937 &&
         p->seed_mode == YK_SEED_COUNTER && p->flags == 0 && s_begin == 0 && s_end == p->samples_per_pixel;
}
// gives the table back (a call's rings need the room, or its next key has another size); false:
// there was none
static bool seed_table_drop(ykgpu_context* ctx) {
  if (!ctx->d_seed_tab) return false;
  for (hipStream_t s : {ctx->aux, ctx->red, ctx->ren, ctx->alt, ctx->stream}) (void)hipStreamSynchronize(s);
  (void)hipFree(ctx->d_seed_tab);
  ctx->d_seed_tab = nullptr;
  ctx->seed_tab_words = 0;
  ctx->seed_tab_filled = false;
  return true;
}

// The two orders of the call's tile: ctx->d_sky_path, the processing order over the blocks that can
// hit something (padded to whole warm-up blocks of 256 slots), and ctx->d_sky_list, the slots of
// the sky blocks.  A function of the scene, the camera and the geometry: built once per key and
// kept; without a sky block both stay empty and the call runs on ctx->d_order as ever.
static int ensure_sky(ykgpu_context* ctx, const yk_render_params* p) {
  const uint32_t Wt = tile_width(p), rows = p->row_count, stride = order_stride(p), mode = order_mode();
  const uint32_t col_begin = p->col_count ? p->col_begin : 0, col_stride = p->col_count ? p->col_stride : 1;
  const uint32_t col_band = p->col_count ? p->col_band_log2 : 0;
  const std::vector<uint64_t> key = {ctx->scene_gen, p->image_width, p->image_height, p->row_begin, rows,
                                     p->row_stride,  p->row_band_log2, col_begin,     Wt,           col_stride,
                                     col_band,       stride,           mode};
  if (ctx->sky_key == key) return YK_OK;
  // the whole order stays the geometry's (kept across scenes, as ever); the two orders are split
  // from it on the device, so a new scene or camera costs the classifier (~2 ms for the frame), a
  // word per block uploaded and one small kernel — no allocation while the tile's size stays
  if (int rc = ensure_order(ctx, Wt, rows, stride)) return rc;
  uint32_t tw, th;
  order_block(stride, tw, th);
  const yksky::Tile tile{p->image_width, p->image_height, p->row_begin, rows,       p->row_stride,
                         p->row_band_log2, col_begin,      Wt,           col_stride, col_band};
  const std::vector<uint8_t> flag = yksky::sky_blocks(ctx->cam, ctx->sky_centers.data(), ctx->sky_radii.data(),
                                                      ctx->nspheres, tile, tw, th);
  const uint32_t bx = (Wt + tw - 1) / tw, by = (rows + th - 1) / th, per = tw * th;
  // each block's place in its order (bit 31: the sky list), in the whole order's block sequence
  std::vector<uint32_t> off((size_t)bx * by);
  uint32_t npath = 0, nlist = 0;
  for (uint32_t jj = 0; jj < by; ++jj)
    for (uint32_t i = 0; i < bx; ++i) {
      const uint32_t j = mode == 1 ? by - 1 - jj : jj;  // (build_order's block rows)
      off[(size_t)jj * bx + i] = flag[(size_t)j * bx + i] ? (0x80000000u | nlist++) : npath++;
    }
  ctx->sky_key.clear();
  ctx->sky_path_slots = ctx->sky_slots = ctx->sky_full_slots = 0;
  if (nlist) {
    const size_t full = ctx->order_slots;  // == bx * by * per
    // (earlier calls may still read the orders about to be rewritten; after ykgpu_set_scene nothing runs)
    if (int rc = quiesce(ctx)) return rc;
    if (full > ctx->sky_cap) {
      for (void* q : {(void*)ctx->d_sky_path, (void*)ctx->d_sky_list, (void*)ctx->d_sky_acc, (void*)ctx->d_sky_mt,
                      (void*)ctx->d_sky_off})
        (void)hipFree(q);
      ctx->d_sky_path = ctx->d_sky_list = ctx->d_sky_mt = ctx->d_sky_off = nullptr;
      ctx->d_sky_acc = nullptr;
      ctx->sky_cap = 0;
      YK_HIP(hipMalloc(&ctx->d_sky_path, (full + 256) * sizeof(uint32_t)));
      YK_HIP(hipMalloc(&ctx->d_sky_list, full * sizeof(uint32_t)));
      YK_HIP(hipMalloc(&ctx->d_sky_acc, full * 3 * sizeof(double)));
      // yk_sky_redo's list (a count, then a word per sky slot) and its engines
      YK_HIP(hipMalloc(&ctx->d_sky_mt, (1 + full + (size_t)kSkyEngines * ykd::kMtN) * sizeof(uint32_t)));
      YK_HIP(hipMalloc(&ctx->d_sky_off, off.size() * sizeof(uint32_t)));
      ctx->sky_cap = full;
    }
    if (!ctx->sky_ev) YK_HIP(hipEventCreateWithFlags(&ctx->sky_ev, hipEventDisableTiming));
    const size_t path_slots = ((size_t)npath * per + 255) / 256 * 256;  // (whole warm-up blocks)
    YK_HIP(hipMemcpy(ctx->d_sky_off, off.data(), off.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(yk_sky_split, dim3((uint32_t)((full + 255) / 256)), dim3(256), 0, ctx->stream, ctx->d_order,
                       ctx->d_sky_off, ctx->d_sky_path, ctx->d_sky_list, (uint32_t)full, per);
    YK_HIP(hipGetLastError());
    if (path_slots > (size_t)npath * per)
      YK_HIP(hipMemsetAsync(ctx->d_sky_path + (size_t)npath * per, 0xff, (path_slots - (size_t)npath * per) * 4,
                            ctx->stream));  // kNoPixel
    YK_HIP(hipMemsetAsync(ctx->d_sky_mt, 0, sizeof(uint32_t), ctx->stream));
    YK_HIP(hipStreamSynchronize(ctx->stream));  // (the call's kernels run on other streams)
    ctx->sky_path_slots = (uint32_t)path_slots;
    ctx->sky_slots = nlist * per;
    ctx->sky_full_slots = (uint32_t)full;
  }
  ctx->sky_key = key;
  return YK_OK;
}

// Render streams get the device's top priority (YKGPU_RENDER_PRIO=0: default priority, A/B): when
// a launch drains, the queued warm-up and reduce blocks would otherwise take the CUs it frees
// before the next launch's workgroups (one per CU, 768 threads and most of the LDS) fit.
hipError_t create_render_stream(hipStream_t* s) {
  int least = 0, greatest = 0;
  const char* e = ab_knob("YKGPU_RENDER_PRIO");
  if ((e && std::atoi(e) == 0) || hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess)
    return hipStreamCreateWithFlags(s, hipStreamNonBlocking);
  return hipStreamCreateWithPriority(s, hipStreamNonBlocking, greatest);
}

// Colour buffers in flight (YKGPU_COL_RING overrides): render c writes buffer c % ring and waits
// for the reduce of launch c - ring.  Two suffice: a reduce (~0.6 ms for 32 spp of 1920x1080)
// ends long before the render after next needs its buffer; rings of 2 / 3 / 4 time the same
// (bench 171.8 / 171.8 / 172.1 ms; config-4 rank tile 174.0 vs 173.6 ms, profiles/r04_ab/rings/)
// and 2 holds 4.2 GB less at the headline size (call_bytes 22.3 -> 18.1 GB)
static uint32_t col_ring() {
  uint32_t r = YK_COL_RING;
  if (const char* e = ab_knob("YKGPU_COL_RING")) r = (uint32_t)std::max(2, std::min(8, std::atoi(e)));
  return r;
}

// Reduce grid: grid-stride over the slots, at most 4 blocks per CU (YKGPU_RED_BLOCKS overrides;
// 0 = one thread per slot), so a reduce never floods the CUs a render launch is about to take
static uint32_t reduce_blocks(const ykgpu_context* ctx, uint32_t nps) {
  uint32_t cap = (uint32_t)ctx->cus * 4;
  if (const char* e = ab_knob("YKGPU_RED_BLOCKS")) cap = (uint32_t)std::max(0, std::atoi(e));
  const uint32_t full = (nps + 255) / 256;
  return cap ? std::max(1u, std::min(full, cap)) : full;
}

// Warm-up grid: grid-stride, at most `per_cu` blocks (one wave per SIMD each) per CU
// (YKGPU_WARM_PER_CU overrides).  The FP64 StartRec warm-up is close to the render's critical
// path and takes every idle issue slot it can (32; 16: neutral, 8: +1.8%); the FP32 one has
// slack, and each resident warm-up wave delays the latency-bound render waves it shares a SIMD
// with (512-spp FP32 A/B: 32 -> 205.2 ms, 4 -> 202.4, 3 -> 202.4, 2 -> 201.3)
static uint32_t warm_per_cu(bool f32) {
  uint32_t per_cu = f32 ? 2u : (uint32_t)YK_WARM_PER_CU;
  if (const char* e = ab_knob("YKGPU_WARM_PER_CU")) per_cu = (uint32_t)std::max(1, std::atoi(e));
  return per_cu;
}
// A warm-up's blocks for n slots, at most cap: each thread walks n / grid slots, at least
// kWarmSlots; with ilp walks per lane the grid is trimmed so that a thread's slot count is a
// multiple of ilp (no lane walks a chain for a slot it does not have, but in the last blocks)
// (align: the slots per sample of a culled order, a multiple of 256, or 0.  The frame's launches
// have a grid whose stride is the slot count per sample — 8100 blocks x 256 = 1920 x 1080 — so a
// lane's ilp walks are consecutive samples of one pixel and their processing-order reads coincide;
// likewise the 8-way tile's, 8160 blocks = 8 x its slots; a culled order keeps that with a grid of
// j x align / 256 blocks, the largest below the cap whose threads walk a multiple of ilp slots:
// few blocks per CU — 897 for that tile's 256-spp launches at j = 1 — share the CUs unevenly, and
// the warm-up is close to the critical path: the tile's synced call +1.6%, profiles/r18_sky_blocks/)
inline uint32_t warm_blocks_for(uint64_t n, uint64_t cap, uint32_t ilp, uint64_t align = 0) {
  if (align && align / 256 <= cap && n % align == 0) {
    const uint64_t m = align / 256, ks = n / align;
    for (uint64_t j = std::min(cap / m, ks / ilp); j >= 1; --j)
      if (ks % (j * ilp) == 0 && ks / j >= kWarmSlots) return (uint32_t)(j * m);
  }
  uint64_t wb = std::min<uint64_t>((n + 256 * kWarmSlots - 1) / (256 * kWarmSlots), cap);
  if (ilp > 1 && wb > 0) {
    const uint64_t per = 256ull * ilp, it = (n + wb * per - 1) / (wb * per);
    wb = (n + per * it - 1) / (per * it);
  }
  return (uint32_t)wb;
}

// Renders samples [s_begin, s_end) of every pixel.  The one-shot entry points pass [0, spp) and no
// film: the fold starts from zero, runs through ctx->d_acc and ends in rgb_dev / sums_dev.  A film
// chunk (ykgpu_film_accumulate) passes its window and the film: the same schedule rule applied to
// the window's length, the same rings and streams, each launch folded into the film's own planes
// by yk_film_reduce (carry-in and carry-out), in the film's own processing order.
//
// launch() is four steps: plan_launch (the schedule, the ring depths, the lens-retry ring, the
// buffers grown), fill_args (the kernels' argument records), enqueue_launches (the event graph and
// the warm-up / render / reduce loop) and call_stats.

// What a call's first step settles and the others read
struct LaunchPlan {
  bool f32, x128;  // x128: no warm-ups, no MT scratch
  bool group;      // a group of an adaptive pass: the film's compacted order of the pixels that take this window
  // the tile has sky blocks: the path pipeline runs over ctx->d_sky_path and yk_sky_samples renders
  // the sky slots, launch by launch (sky_sched: the path's schedule, or the call's own when no
  // block is left for the path kernel); warm_align: warm_blocks_for's `align`
  bool culled;
  uint64_t warm_align;
  const DevTree* tree;
  const DevTree::Plan* plan;
  int grid, block;
  uint64_t seed_key;
  const uint32_t* order;
  uint32_t nps;  // processing slots (>= pixels)
  uint32_t spp;  // samples per pixel of this call (p->samples_per_pixel stays the stride of the seeds)
  std::vector<std::pair<uint32_t, uint32_t>> sched;  // (s0, samples)
  uint64_t shape;
  bool warm_first;
  uint32_t K, nlaunch, kWarmRing, kColRing, mem_shrinks;
  size_t welem;  // start records (StartRec, FP32 StartRecF: each sample's whole start)
  uint32_t retry_cap;  // records per wave
  size_t retry_n;
  // the seed table: kTabWalk (none), kTabFill or kTabRead; tab_part: which of its words the sky
  // kernel touches (the sky split's key; empty: none); tab_sync: that differs from the last call
  // that used the table, so the warm-up and the sky stream first wait for that call's kernels
  int tab_mode = 0;  // (kTabWalk; initialised: launch() reads it after a plan_launch that failed early)
  bool tab_sync = false;
  uint32_t tab_T = 0;
  std::vector<uint64_t> tab_part;
};

// slots per warm-up wave of an FP64 launch of nl slots
static uint64_t warm_wave_slots(const ykgpu_context* ctx, uint64_t nl, uint64_t align) {
  const uint64_t wb = warm_blocks_for(nl, (uint64_t)ctx->cus * warm_per_cu(false), kWalkIlp, align);
  return (nl + wb * 256 - 1) / (wb * 256) * 64;
}

static int plan_launch(ykgpu_context* ctx, const yk_render_params* p, uint32_t s_begin, uint32_t s_end,
                       ykgpu_film* film, LaunchPlan& lp) {
  const bool f32 = lp.f32 = p->precision == YK_PRECISION_FP32;
  const bool x128 = lp.x128 = p->rng == YK_RNG_XOR128;  // no warm-ups, no MT scratch
  const DevTree& tree = *(lp.tree = f32 ? &ctx->t32 : &ctx->t64);
  const DevTree::Plan& plan = *(lp.plan = &tree.plan[x128 ? 1 : 0]);
  const int grid = lp.grid = plan.grid, block = lp.block = block_of(x128);
  int rc = ensure_scratch(ctx, p->max_depth, (size_t)grid * block, !x128);
  if (rc) return rc;
  // YK_SEED_RANDOM_DEVICE without a key: one from std::random_device per call (source.cpp:159)
  uint64_t& seed_key = lp.seed_key = 0;
  if (p->seed_mode == YK_SEED_RANDOM_DEVICE) {
    seed_key = p->seed_key;
    if (!seed_key) {
      std::random_device rd;
      while (!seed_key) seed_key = ((uint64_t)rd() << 32) | rd();
    }
  }
  // (a film brings its own order, and leaves the context's alone)
  // (... and a tile with sky blocks runs the path pipeline over the other blocks only; a tile
  // without one runs on the context's order exactly as a call that never looked)
  bool& culled = lp.culled = false;
  if (sky_eligible(p, film, plan)) {
    if ((rc = ensure_sky(ctx, p))) return rc;
    culled = ctx->sky_slots != 0;
  }
  if (!film && !culled && (rc = ensure_order(ctx, tile_width(p), p->row_count, order_stride(p)))) return rc;
  // (a group of an adaptive pass: the film's compacted order of the pixels that take this window)
  const bool group = lp.group = film && film->g_slots != 0;
  lp.order = group ? film->d_gorder : film ? film->d_order : culled ? ctx->d_sky_path : ctx->d_order;
  // Launch schedule (samples per pixel per launch; the rule is yk_schedule.hpp's): a ramp up to
  // kmax (kLaunchSpp = 32, or more for a small tile), also capped by the colour budget (32 B per
  // sample slot, kLaunchBytes per launch); a short remainder is folded into the launches before
  // it.  Each launch ends with the tail of its longest paths (~0.1-0.2 ms of partly idle CUs), but
  // launches alternate between two streams, so that drain overlaps the next launch: many mid-sized
  // launches beat a few large ones.  Independent of the image size, which matters
  // for the per-rank tiles of N GPUs.
  const uint32_t nps = lp.nps = group    ? film->g_slots
                                : film   ? film->nps
                                : culled ? ctx->sky_path_slots
                                         : ctx->order_slots;  // processing slots (>= pixels)
  lp.warm_align = culled ? nps : 0;
  // samples per pixel of this call (p->samples_per_pixel stays the stride of the seeds)
  const uint32_t spp = lp.spp = s_end - s_begin;
  // the rings' launch size (an in-flight call's launches) and a synced call's, <= it.  A culled
  // call keeps the launch sizes of its whole tile (the samples per launch were tuned per image
  // size, and yk_sky_samples runs the same launches); its rings hold the path's slots only.
  const yksched::LaunchSizes sizes =
      yksched::launch_sizes(culled ? ctx->sky_full_slots : nps, spp, (uint64_t)grid * block);
  const uint32_t kideal = sizes.kideal, ksynced = sizes.ksynced, kfloor = sizes.kfloor;
  // A device short of memory (other contexts, other processes) makes the call slower, not fatal:
  // the rings are sized for launches of kmax samples per pixel, and when the device cannot hold
  // them — free memory (hipMemGetInfo) plus what this context's rings already hold, or a
  // hipMalloc that fails anyway — kmax halves, down to launches of kMemFloorSlots sample slots,
  // before the call fails with YK_ERR_NOMEM (yk_render_stats.launch_spp / mem_shrinks report it).
  uint32_t kmax = kideal;
  uint32_t& mem_shrinks = lp.mem_shrinks = 0;
  auto shrink = [&]() {
    kmax = std::max(kfloor, kmax / 2);
    ++mem_shrinks;
  };
  // a buffer follows the call: grown when it is too small, and given back when the call needs
  // less than half of it (device_bytes then reports about what the call holds) — but not by a group
  // of an adaptive pass: its next pass or chunk needs the frame's rings again, and giving 12 GB
  // back costs 15-35 ms, at times over a second (tools/adaptive_bench.py)
  auto grow = [&](auto*& ptr, size_t& cap, size_t need, size_t elem) -> int {
    if (need <= cap && (group || 2 * need >= cap)) return YK_OK;
    if (int q = quiesce(ctx)) return q;
    (void)hipFree(ptr);
    ptr = nullptr;
    cap = 0;
    YK_HIP(hipMalloc((void**)&ptr, need * elem));
    cap = need;
    return YK_OK;
  };
  std::vector<std::pair<uint32_t, uint32_t>>& sched = lp.sched;  // (s0, samples)
  uint64_t& shape = lp.shape = 0;
  bool inflight = false;
  uint32_t &K = lp.K = 0, &nlaunch = lp.nlaunch = 0, &kWarmRing = lp.kWarmRing = 0, &kColRing = lp.kColRing = 0;
  // start records (StartRec, FP32 StartRecF: each sample's whole start)
  const size_t welem = lp.welem = f32 ? sizeof(StartRecF) : sizeof(StartRec);
  // (diagnostic, timing only) YKGPU_ABL_WARM_FIRST=1: every launch's warm-up runs, and finishes,
  // before the first render: render_busy_ms then times the render kernels without the seed walks
  // beside them (same images)
  const bool warm_first = lp.warm_first = ab_knob("YKGPU_ABL_WARM_FIRST") != nullptr && !x128;
  for (;;) {
    // (only for a call of the previous one's shape, whose rings it can overlap: launch() `ov`)
    shape = ((uint64_t)nps << 24) ^ ((uint64_t)kmax << 2) ^ (f32 ? 2u : 0u) ^ (x128 ? 1u : 0u);
    inflight = false;
    if (ctx->prev_enqueued && ctx->prev_ok && !ctx->dirty && ctx->prev_shape == shape && ctx->prev_n > 0 &&
        ctx->lev.size() >= 6ull * ctx->prev_n)
      inflight = hipEventQuery(ctx->lev[6 * (ctx->prev_n - 1) + 5]) == hipErrorNotReady;
    yksched::launch_schedule(sched, spp, s_begin, kmax, ksynced, inflight);
    // a launch buffer of the rings holds kmax samples per pixel (every launch fits: above)
    K = kmax;
    nlaunch = (uint32_t)sched.size();
    if (nps == 0) break;  // (every block is a sky block: no path launch, no rings; launch())
    // rings as deep as kWarmRingDepth / col_ring() whatever the call's launch count (a call of two
    // launches reuses the buffers of the call before it, launch() `ov`); one buffer each for a
    // single-launch call
    kWarmRing = nlaunch > 1 ? kWarmRingDepth : 1;
    if (const char* e = ab_knob("YKGPU_WARM_RING"))  // (A/B) launch buffers in the ring
      kWarmRing = (uint32_t)std::min<uint64_t>(kDepRing - 1, (uint64_t)std::max(2, std::atoi(e)));
    if (warm_first) kWarmRing = nlaunch;
    // colour buffers: render c writes buffer c % ring and waits for the reduce of launch c - ring;
    // reduce c (stream red) overlaps the renders after it
    kColRing = nlaunch > 1 ? std::min(col_ring(), kDepRing - 1) : 1;
    // (a culled call's rings are the whole tile's: the path's slots change with every view, and a
    // ring that grew or shrank with them would be freed and allocated again at each new camera —
    // gigabytes, at times over a second; the launches use the front of each buffer)
    const size_t nps_ring = culled ? ctx->sky_full_slots : nps;
    const size_t need_warm = x128 ? 0 : (size_t)kWarmRing * nps_ring * K * welem;
    const size_t need_col = (size_t)kColRing * nps_ring * K * kColStride * sizeof(double);
    if (kmax > kfloor && (need_warm > ctx->warm_cap || need_col > ctx->col_cap * sizeof(double))) {
      // the rings must grow: does the device have room for them?
      size_t free_b = 0, total_b = 0;
      if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
        const size_t held = ctx->warm_cap + ctx->col_cap * sizeof(double);
        if (need_warm + need_col + kMemReserve > free_b + held) {
          // (the seed table goes before the launches shrink: it is never the cause of a shrink)
          if (!seed_table_drop(ctx)) shrink();
          continue;
        }
      }
    }
    rc = x128 ? YK_OK : grow(ctx->d_warm, ctx->warm_cap, need_warm, 1);
    if (!rc) rc = grow(ctx->d_col, ctx->col_cap, (size_t)kColRing * nps_ring * K * kColStride, sizeof(double));
    if (rc == YK_ERR_NOMEM && kmax > kfloor) {
      (void)hipGetLastError();  // (the failed hipMalloc's error must not surface at a later launch)
      if (!seed_table_drop(ctx)) shrink();
      continue;
    }
    if (rc) return rc;
    break;
  }
  if (!film && nps && sched.size() > 1 && (rc = grow(ctx->d_acc, ctx->acc_cap, (size_t)(culled ? ctx->sky_full_slots : nps) * 3, sizeof(double))))
    return rc;
  // The FP64 lens warm-ups of launches with at most kDeferSlots slots per warm-up wave draw their
  // lens retries after the walks (yk_mt_warmup_defer) from a ring per wave, sized to the largest
  // such launch (the frame's 32-spp launches: 640 records, 1.0 GB); longer launches run the
  // rejection loop in line (config 5's 128-spp launches: 8100 slots per wave; at 121 spp, 7600 per
  // wave, the deferral measured 0.7% slower)
  const bool lens_defer = !x128 && !f32 && nps && ctx->cam.lens_radius > 0;
  uint32_t& retry_cap = lp.retry_cap = 0;  // records per wave
  if (lens_defer)
    for (const auto& l : sched)
      if (warm_wave_slots(ctx, (uint64_t)nps * l.second, lp.warm_align) <= kDeferSlots)
        retry_cap =
            std::max(retry_cap, retry_cap_for(warm_wave_slots(ctx, (uint64_t)nps * l.second, lp.warm_align)));
  // a call whose launches were shrunk for want of memory runs the rejection loop in line: the
  // shrink loop above budgets the start-record and colour rings only, so the plan it settled on
  // is the plan the call runs (no ring allocated afterwards out of the reserve it kept)
  if (mem_shrinks) retry_cap = 0;
#ifdef YK_RETRY_CAP_FORCE
  // (test variants, tests/test_gpu_robust.py): the ring's capacity forced so that its fallbacks
  // run — 64 records per wave fill up (the samples that find it full reach the render as kNoStart
  // starts it makes itself), 0 is the in-line loop a failed ring allocation falls back to
  if (retry_cap) retry_cap = YK_RETRY_CAP_FORCE;
#endif
  size_t& retry_n = lp.retry_n = (size_t)ctx->cus * warm_per_cu(false) * 4u * retry_cap * 3u;
  if (retry_cap && (rc = grow(ctx->d_retry, ctx->retry_cap, retry_n, sizeof(uint4)))) {
    if (rc != YK_ERR_NOMEM) return rc;
    // a device short of memory runs the rejection loop in line instead (slower, never fatal)
    (void)hipGetLastError();
    retry_cap = 0;
    retry_n = 0;
  }
  // The seed table, last: the call's rings fit, and the table takes only room the device still has
  // beyond the reserve the rings leave (a call whose launches were shrunk has none to give).  Only
  // a call with sky slots takes part: the sky kernel is the table's one reader, so a view without a
  // sky block (an enclosed room) neither allocates nor fills nor reads, and keeps whatever table
  // the context holds for a later view (a camera that then shows sky under another key runs a
  // walking call and then a fill call).  A filled table of the call's key is read; the second
  // consecutive such call of a key fills — the same buffer when the size is the key's, a new one
  // otherwise.  Without room the call walks as ever.
  lp.tab_mode = kTabWalk;
  lp.tab_sync = false;
  lp.tab_T = 0;
  if (culled && seed_table_eligible(ctx, p, film, s_begin, s_end) && !warm_first && !mem_shrinks) {
    const ykseed::Key key = ykseed::make_key(p->seed0, p->image_width, p->samples_per_pixel, p->row_begin, p->row_count,
                                             p->row_stride, p->row_band_log2, p->col_begin, p->col_count,
                                             p->col_stride, p->col_band_log2);
    const uint64_t words = ykseed::table_words(key);
    lp.tab_T = ykseed::tile_pixels(key);
    if (words * sizeof(uint32_t) <= ctx->seed_tab_max_bytes) {
      if (ctx->d_seed_tab && ctx->seed_tab_filled && ykseed::same_key(ctx->seed_tab_key, key)) {
        lp.tab_mode = kTabRead;
      } else if (!(ctx->seed_tab_seen && ykseed::same_key(ctx->seed_tab_seen_key, key))) {
        // the first call of a key walks as ever: only a key that comes again is worth a fill (a
        // frame whose every call has a new seed0 measured +1.0% when each one filled, outside the
        // parent's run-to-run spread; profiles/r23_seed_table/)
      } else {
        if (ctx->d_seed_tab && ctx->seed_tab_words != words) seed_table_drop(ctx);
        if (!ctx->d_seed_tab) {
          size_t free_b = 0, total_b = 0;
          if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && words * sizeof(uint32_t) + kMemReserve <= free_b) {
            if (hipMalloc((void**)&ctx->d_seed_tab, words * sizeof(uint32_t)) == hipSuccess) {
              ctx->seed_tab_words = words;
            } else {
              (void)hipGetLastError();
              ctx->d_seed_tab = nullptr;
            }
          }
        }
        if (ctx->d_seed_tab) {
          if (!ctx->seed_ev_aux) YK_HIP(hipEventCreateWithFlags(&ctx->seed_ev_aux, hipEventDisableTiming));
          if (!ctx->seed_ev_red) YK_HIP(hipEventCreateWithFlags(&ctx->seed_ev_red, hipEventDisableTiming));
          ctx->seed_tab_key = key;
          ctx->seed_tab_filled = false;  // (until every launch of this call has been enqueued)
          lp.tab_mode = kTabFill;
        }
      }
    }
    ctx->seed_tab_seen_key = key;
    ctx->seed_tab_seen = true;
    if (lp.tab_mode != kTabWalk) {
      lp.tab_part = ctx->sky_key;
      lp.tab_sync = lp.tab_part != ctx->seed_tab_part;
    }
  }
  return YK_OK;
}

// The argument records of a call's kernels: everything but what changes from launch to launch
// (enqueue_launches sets that)
struct LaunchArgs {
  KernelArgs ka;
  WarmArgs wa;
  ReduceArgs ra;
  FilmReduceArgs fa;
  FilmMaskedArgs fm;
  SkyArgs sa;  // (a culled call's)
};

static int fill_args(const ykgpu_context* ctx, const yk_render_params* p, uint8_t* rgb_dev, double* sums_dev,
                     const ykgpu_film* film, const LaunchPlan& lp, LaunchArgs& la) {
  const DevTree& tree = *lp.tree;
  const DevTree::Plan& plan = *lp.plan;
  const int grid = lp.grid, block = lp.block;
  const uint32_t nps = lp.nps, retry_cap = lp.retry_cap;
  const uint32_t* const order = lp.order;
  const uint64_t seed_key = lp.seed_key;
  const bool group = lp.group;
  KernelArgs& ka = la.ka;
  ka.cam = ctx->cam;
  ka.pad_a = 0;
  {
    const yk_camera& c = ctx->cam;
    for (int k = 0; k < 3; ++k) {
      ka.camf.origin[k] = (float)c.origin[k];
      ka.camf.llc[k] = (float)c.lower_left_corner[k];
      ka.camf.horizontal[k] = (float)c.horizontal[k];
      ka.camf.vertical[k] = (float)c.vertical[k];
      ka.camf.lens_u[k] = (float)c.lens_u[k];
      ka.camf.lens_v[k] = (float)c.lens_v[k];
      ka.camf.pad[k] = 0.0f;
    }
    ka.camf.lens_radius = (float)c.lens_radius;
    ka.camf.w = (float)p->image_width;  // unsigned → float (source.cpp:162, T = float)
    ka.camf.h = (float)p->image_height;
  }
  ka.W = p->image_width;
  ka.Wt = tile_width(p);
  ka.col_begin = p->col_count ? p->col_begin : 0;
  ka.col_stride = p->col_count ? p->col_stride : 1;
  ka.col_band = p->col_count ? p->col_band_log2 : 0;
  ka.H = p->image_height;
  ka.spp = p->samples_per_pixel;
  ka.max_depth = p->max_depth;
  ka.seed0 = p->seed0;
  ka.row_begin = p->row_begin;
  ka.row_count = p->row_count;
  ka.row_stride = p->row_stride;
  ka.band_log2 = p->row_band_log2;
  ka.nspheres = ctx->nspheres;
  ka.flags = p->flags;
  ka.id_stride = ctx->id_stride;
  ka.start = nullptr;
  ka.order = order;
  ka.t_min = p->t_min;
  ka.origin_bound = tree.origin_bound;
  ka.inv_w = 1.0 / (double)ka.W;
  ka.inv_h = 1.0 / (double)ka.H;
  ka.w_d = (double)ka.W;
  ka.h_d = (double)ka.H;
  ka.bvh_root = tree.root;
  ka.n_nodes = tree.n_nodes;
  ka.lds_geo_off = tree.geo_off;
  ka.lds_ids_off = tree.ids_off;
  ka.lds_tgeo_off = plan.tgeo_off;
  ka.lds_mat_off = plan.mat_off;
  ka.lds_stack_off = plan.stack_off;
  ka.stack_cap = plan.stack_cap;
  ka.nodes = tree.nodes;
  ka.leaf_geo = (const SphereGeo*)tree.leaf_geo;  // float4 records for the FP32 kernel
  ka.leaf_ids = tree.leaf_ids;
  ka.geo = ctx->d_geo;
  ka.mat = ctx->d_mat;
  ka.geo_f = ctx->d_geo_f;
  ka.seed_mode = p->seed_mode;
  ka.seed_key = seed_key;
  ka.pixel_counter = ctx->d_counter;

  ka.counters = ctx->d_stats;
  ka.trace = ctx->d_trace;
  ka.trace_counts = ctx->d_trace_counts;
  ka.trace_cap = ctx->trace_cap;
  ka.claim_tail = (uint32_t)grid * (uint32_t)(block / 64) * kClaim * kClaimTailFactor;
  if ((ka.flags & YK_FLAG_TRACE_RAYS) && !(ctx->d_trace && (ka.flags & YK_FLAG_COUNT_WORK)))
    return fail(YK_ERR_INVALID, "YK_FLAG_TRACE_RAYS is set by ykgpu_render_trace only");
  WarmArgs& wa = la.wa;
  wa.W = p->image_width;
  wa.Wt = ka.Wt;
  wa.col_begin = ka.col_begin;
  wa.col_stride = ka.col_stride;
  wa.col_band = ka.col_band;
  wa.spp = p->samples_per_pixel;
  wa.seed0 = p->seed0;
  wa.row_begin = p->row_begin;
  wa.row_stride = p->row_stride;
  wa.band_log2 = p->row_band_log2;
  wa.out = ctx->d_warm;
  wa.retry = retry_cap ? ctx->d_retry : nullptr;
  wa.retry_cap = retry_cap;
  wa.retry_pad = 0;
  wa.lens = ctx->cam.lens_radius > 0 ? 1u : 0u;
  wa.H = p->image_height;
  wa.cam = ctx->cam;
  wa.camf = ka.camf;
  wa.w_d = ka.w_d;
  wa.h_d = ka.h_d;
  wa.inv_w = ka.inv_w;
  wa.inv_h = ka.inv_h;
  wa.npix_slots = nps;
  fastdiv(std::max(nps, 1u), wa.nps_m, wa.nps_sh);  // (0: a call of sky blocks only, no path launch)
  fastdiv(ka.Wt, wa.w_m, wa.w_sh);
  wa.seed_mode = p->seed_mode;
  wa.seed_key = seed_key;
  wa.order = order;
  ka.npix_slots = nps;
  ka.nps_m = wa.nps_m;
  ka.nps_sh = wa.nps_sh;
  ka.w_m = wa.w_m;
  ka.w_sh = wa.w_sh;
  ka.stack_check = plan.stack_check ? 1u : 0u;
  ReduceArgs& ra = la.ra;
  ra.acc = ctx->d_acc;
  ra.order = order;
  ra.rgb = rgb_dev;
  ra.sums = sums_dev;
  ra.npix_slots = nps;
  ra.spp = p->samples_per_pixel;
  ra.pad0 = ra.pad1 = 0;
  FilmReduceArgs& fa = la.fa = FilmReduceArgs{};
  FilmMaskedArgs& fm = la.fm = FilmMaskedArgs{};
  if (group) {
    fm.plane = film->d_plane;
    fm.count = film->d_count;
    fm.map = film->d_gmap;
    fm.npix_slots = film->nps;
    fm.g_slots = nps;
  } else if (film) {
    fa.plane = film->d_plane;
    fa.order = order;
    fa.npix_slots = nps;
  }
  SkyArgs& sa = la.sa = SkyArgs{};
  if (lp.culled) {
    sa.W = ka.W, sa.H = ka.H, sa.spp = ka.spp, sa.seed0 = ka.seed0;
    sa.row_begin = ka.row_begin, sa.row_stride = ka.row_stride, sa.band_log2 = ka.band_log2;
    sa.Wt = ka.Wt, sa.col_begin = ka.col_begin, sa.col_stride = ka.col_stride, sa.col_band = ka.col_band;
    sa.w_m = ka.w_m, sa.w_sh = ka.w_sh;
    sa.lens = wa.lens;
    sa.n = ctx->sky_slots;
    sa.cam = ctx->cam;
    sa.w_d = ka.w_d, sa.h_d = ka.h_d, sa.inv_w = ka.inv_w, sa.inv_h = ka.inv_h;
    sa.list = ctx->d_sky_list;
    sa.acc = ctx->d_sky_acc;
    sa.rgb = rgb_dev;
    sa.sums = sums_dev;
    sa.engines = ctx->d_sky_mt;
    sa.counters = ctx->d_stats;
  }
  return YK_OK;
}

// yk_sky_samples for samples [s0, s0 + ks) of the sky slots, on stream s.  The launch that ends the
// call writes the caller's image: a call that overlaps the one before it (wait_caller) has not made
// its streams wait for the caller's yet.
static int enqueue_sky(ykgpu_context* ctx, hipStream_t s, SkyArgs& sa, uint32_t s0, uint32_t ks, uint32_t s_end,
                       bool wait_caller, int tab_mode, uint32_t tab_T) {
  sa.s0 = s0;
  sa.ks = ks;
  sa.first = s0 == 0;
  sa.last = s0 + ks == s_end;
  if (sa.last && wait_caller) YK_HIP(hipStreamWaitEvent(s, ctx->ev0, 0));
  const SkyTabArgs ta{sa, SeedTab{ctx->d_seed_tab, tab_T, g_seed_tab_flip.load()}};
  if (tab_mode == kTabRead)
    hipLaunchKernelGGL(yk_sky_samples_tab<kTabRead>, dim3((sa.n + 255) / 256), dim3(256), 0, s, ta);
  else if (tab_mode == kTabFill)
    hipLaunchKernelGGL(yk_sky_samples_tab<kTabFill>, dim3((sa.n + 255) / 256), dim3(256), 0, s, ta);
  else
    hipLaunchKernelGGL(yk_sky_samples, dim3((sa.n + 255) / 256), dim3(256), 0, s, sa);
  YK_HIP(hipGetLastError());
  // (the lens: without one no sample can outrun the lazy cursors, and nothing is ever listed)
  if (sa.lens) {
    hipLaunchKernelGGL(yk_sky_redo, dim3(1), dim3(kSkyEngines), 0, s, sa);
    YK_HIP(hipGetLastError());
  }
  return YK_OK;
}

// A call whose every block is a sky block: no path launch, no rings, one yk_sky_samples over the
// call's samples, behind whatever the context still runs and the caller's stream.
// The seed table's ordering: warm-ups run in order on ctx->aux and sky kernels in
// order on ctx->red, and while the sky split stays what it was each word is touched by one of the
// two streams only, whatever the calls do with it (fill, read, fill again under a new seed0).  When
// the split changes (a new scene or camera, another tile) a word stored by one kernel may be read
// or stored again by the other: such a call (tab_sync) makes both streams wait for both kernels of
// the last call that used the table.  Every call that uses the table records the two events once
// its launches are enqueued (seed_table_used).  Stream waits only: nothing here waits on the host,
// and back-to-back calls of one view overlap exactly as without the table.
static int seed_table_wait(ykgpu_context* ctx, const LaunchPlan& lp) {
  if (!lp.tab_sync || !ctx->seed_ev_set) return YK_OK;
  for (hipStream_t s : {ctx->aux, ctx->red}) {
    YK_HIP(hipStreamWaitEvent(s, ctx->seed_ev_aux, 0));
    YK_HIP(hipStreamWaitEvent(s, ctx->seed_ev_red, 0));
  }
  return YK_OK;
}
static int seed_table_used(ykgpu_context* ctx, const LaunchPlan& lp) {
  if (lp.tab_mode == kTabWalk) return YK_OK;
  YK_HIP(hipEventRecord(ctx->seed_ev_aux, ctx->aux));
  YK_HIP(hipEventRecord(ctx->seed_ev_red, ctx->red));
  ctx->seed_ev_set = true;
  ctx->seed_tab_part = lp.tab_part;
  if (lp.tab_mode == kTabFill) ctx->seed_tab_filled = true;
  return YK_OK;
}

static int enqueue_sky_only(ykgpu_context* ctx, hipStream_t st, uint32_t s_begin, uint32_t s_end, const LaunchPlan& lp,
                            LaunchArgs& la) {
  int rc = YK_OK;
  // (yk_sky_redo adds to d_stats[3], the MT-fallback count, on ctx->red: a later call that clears
  // d_stats from another caller stream, or on ctx->aux when it overlaps this one, is not ordered
  // behind that add — the one counter, for samples never seen, may then miss them; images never)
  if (ctx->dirty && (rc = quiesce(ctx))) return rc;
  if (ctx->prev_enqueued && ctx->prev_n > 0)
    YK_HIP(hipStreamWaitEvent(st, ctx->lev[6 * (ctx->prev_n - 1) + 5], 0));
  ctx->prev_ok = false;
  ctx->dirty = true;
  YK_HIP(hipMemsetAsync(ctx->d_stats, 0, kCounters * sizeof(unsigned long long), st));
  YK_HIP(hipMemsetAsync(ctx->d_stats + 16, 0xff, 2 * sizeof(unsigned long long), st));  // minima
  YK_HIP(hipEventRecord(ctx->ev0, st));
  YK_HIP(hipStreamWaitEvent(ctx->red, ctx->ev0, 0));
  if ((rc = seed_table_wait(ctx, lp))) return rc;
  if ((rc = enqueue_sky(ctx, ctx->red, la.sa, s_begin, s_end - s_begin, s_end, false, lp.tab_mode, lp.tab_T))) return rc;
  YK_HIP(hipEventRecord(ctx->sky_ev, ctx->red));
  YK_HIP(hipStreamWaitEvent(st, ctx->sky_ev, 0));
  YK_HIP(hipEventRecord(ctx->ev1, st));
  // (no launch events: the next call waits for this one through the caller's stream and ctx->red)
  ctx->lev_used = 0;
  ctx->prev_n = 0;
  ctx->run_len = 0;
  ctx->prev_enqueued = false;
  ctx->dirty = false;
  return YK_OK;
}

// Enqueues the call's launches; *launches_out receives how many.
static int enqueue_launches(ykgpu_context* ctx, hipStream_t st, uint32_t s_end, const ykgpu_film* film,
                            const LaunchPlan& lp, LaunchArgs& la, uint32_t* launches_out) {
  const bool f32 = lp.f32, x128 = lp.x128, group = lp.group, warm_first = lp.warm_first;
  const DevTree::Plan& plan = *lp.plan;
  const int grid = lp.grid, block = lp.block;
  const uint32_t nps = lp.nps, K = lp.K, nlaunch = lp.nlaunch, kWarmRing = lp.kWarmRing, kColRing = lp.kColRing;
  const size_t welem = lp.welem;
  const std::vector<std::pair<uint32_t, uint32_t>>& sched = lp.sched;
  KernelArgs& ka = la.ka;
  WarmArgs& wa = la.wa;
  ReduceArgs& ra = la.ra;
  FilmReduceArgs& fa = la.fa;
  FilmMaskedArgs& fm = la.fm;
  int rc = YK_OK;
  // Cross-call pipelining: the launches are numbered across calls (ctx->g_next) and a launch's
  // ring slots (start records, colours, slot counter), scratch parity and render stream follow its
  // global number, so a call whose rings have the previous call's geometry needs no barrier
  // behind it: its warm-up c (c < ring) waits only for the previous call's render that last read
  // that start-record buffer, its render c only for the reduce that last read that colour
  // buffer, and only its last reduce, which writes the caller's image, waits for the caller's
  // stream (ev0).  Back-to-back calls then overlap like the launches inside a call: the next
  // call's first warm-up and renders take the CUs the last launch's draining blocks free.
  // YKGPU_OVERLAP=0 (A/B) keeps every call behind the caller's stream, as do xor128 calls (no
  // warm-up kernel to clear their slot counters) and any call after a failed one.
  const uint64_t g0 = ctx->g_next;
  // (every field that places a launch's start records, colours or per-lane scratch: a call whose
  // K, record size or lane count differs would address other offsets of the same buffers, and its
  // ring waits would not cover the previous call's launches there)
  ykgpu_context::RingGeom geom;
  geom.nps = nps;
  geom.K = K;
  geom.welem = welem;
  geom.warm_ring = kWarmRing;
  geom.col_ring = kColRing;
  geom.lanes = (uint64_t)grid * block;
  geom.id_stride = ctx->id_stride;
  geom.warm = ctx->d_warm;
  geom.col = ctx->d_col;
  geom.mt = ctx->d_mt;
  geom.ids = ctx->d_ids;
  const char* ove = std::getenv("YKGPU_OVERLAP");
  // (the last max(ring) launches, of however many calls, had this geometry: each buffer this call
  // reuses was last used by one of them, whose events ctx->gev holds)
  const bool same_run = ctx->prev_ok && ctx->prev_geom == geom;  // (ctx->run_len continues)
  const bool ov = !x128 && !warm_first && !(ove && std::atoi(ove) == 0) && ctx->prev_ok && ctx->prev_geom == geom &&
                  ctx->run_len >= std::max(kWarmRing, kColRing) && std::max(kWarmRing, kColRing) < kDepRing;
  if (ctx->dirty && (rc = quiesce(ctx))) return rc;  // a failed call's work: wait it out on the host
  const bool after_prev = ctx->prev_enqueued && !ctx->dirty && !ov;
  ctx->prev_ok = false;  // (until this call has been enqueued)
  ctx->dirty = true;
  // slot counters: one per launch of the call for xor128 (cleared here), one per start-record
  // buffer for mt19937 (cleared by the launch's warm-up kernel: a clear between launches as a
  // fill kernel of its own would wait for a free CU behind the warm-ups and reduces, up to 1.6 ms
  // per launch, measured)
  if (std::max(nlaunch, kWarmRing) > ctx->counter_cap) {
    if ((rc = quiesce(ctx))) return rc;
    (void)hipFree(ctx->d_counter);
    (void)hipFree(ctx->d_clk);
    ctx->d_counter = nullptr;
    ctx->d_clk = nullptr;
    ctx->counter_cap = 0;
    YK_HIP(hipMalloc(&ctx->d_counter, std::max(nlaunch, kWarmRing) * sizeof(uint32_t)));
    YK_HIP(hipMalloc(&ctx->d_clk, 4ull * std::max(nlaunch, kWarmRing) * sizeof(unsigned long long)));
    ctx->counter_cap = std::max(nlaunch, kWarmRing);
  }
  // per launch: [0] warm-up start, [1] warm-up end (aux), [2] render start, [3] render end (st),
  // [4] reduce start, [5] reduce end (red); the previous call's stay in lev_prev
  std::swap(ctx->lev, ctx->lev_prev);
  ctx->lev_prev_used = ctx->lev_used;
  while (ctx->lev.size() < 6ull * nlaunch) {
    hipEvent_t e;
    YK_HIP(hipEventCreate(&e));
    ctx->lev.push_back(e);
  }
  ctx->lev_used = 6 * nlaunch;
  // the caller's stream clears this call's slot counters (xor128) and work counters below: before
  // that it waits for the previous call, whose renders may still use both (it may have been
  // enqueued on another stream)
  if (after_prev) YK_HIP(hipStreamWaitEvent(st, ctx->lev_prev[6 * (ctx->prev_n - 1) + 5], 0));
  if (x128) YK_HIP(hipMemsetAsync(ctx->d_counter, 0, nlaunch * sizeof(uint32_t), st));
  if (!ov) {
    YK_HIP(hipMemsetAsync(ctx->d_stats, 0, kCounters * sizeof(unsigned long long), st));
    YK_HIP(hipMemsetAsync(ctx->d_stats + 16, 0xff, 2 * sizeof(unsigned long long), st));  // minima
  }
  YK_HIP(hipEventRecord(ctx->ev0, st));
  if (ov) {
    // (the previous call's last renders may still add their MT-fallback counts here)
    YK_HIP(hipMemsetAsync(ctx->d_stats, 0, kCounters * sizeof(unsigned long long), ctx->aux));
    YK_HIP(hipMemsetAsync(ctx->d_stats + 16, 0xff, 2 * sizeof(unsigned long long), ctx->aux));
  } else {
    // the caller's earlier work, and the whole previous call (its last reduce ends after every
    // launch of it: whichever stream the caller used then), come first
    for (hipStream_t s : {ctx->aux, ctx->red, ctx->alt, ctx->ren}) {
      YK_HIP(hipStreamWaitEvent(s, ctx->ev0, 0));
      if (after_prev) YK_HIP(hipStreamWaitEvent(s, ctx->lev_prev[6 * (ctx->prev_n - 1) + 5], 0));
    }
  }
  if ((rc = seed_table_wait(ctx, lp))) return rc;
  while (ctx->gev.size() < 2ull * kDepRing) {
    hipEvent_t e;
    YK_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    ctx->gev.push_back(e);
  }
  // the end of global launch g's render ([0]) or reduce ([1])
  auto gdep = [&](uint64_t g, int which) { return ctx->gev[2 * (g % kDepRing) + which]; };
  auto warm = [&](uint32_t c) -> int {
    hipEvent_t* ev = &ctx->lev[6 * c];
    // its buffer: the render that last read it (launch c - ring, possibly an earlier call's)
    if (c >= kWarmRing)
      YK_HIP(hipStreamWaitEvent(ctx->aux, ctx->lev[6 * (c - kWarmRing) + 3], 0));
    else if (ov)
      YK_HIP(hipStreamWaitEvent(ctx->aux, gdep(g0 + c - kWarmRing, 0), 0));
    wa.s0 = sched[c].first;
    wa.n = (uint64_t)nps * sched[c].second;
    wa.out = ctx->d_warm + (size_t)((g0 + c) % kWarmRing) * nps * K * welem;
    wa.counter = ctx->d_counter + (g0 + c) % kWarmRing;
    const bool defer =
        !x128 && !f32 && wa.lens && wa.retry_cap && warm_wave_slots(ctx, wa.n, lp.warm_align) <= kDeferSlots;
    const uint32_t wblocks =
        warm_blocks_for(wa.n, (uint64_t)ctx->cus * warm_per_cu(f32), defer ? kWalkIlp : 1u, lp.warm_align);
    YK_HIP(hipEventRecord(ev[0], ctx->aux));
    const WarmTabArgs ta{wa, SeedTab{ctx->d_seed_tab, lp.tab_T, g_seed_tab_flip.load()}};
    if (!x128) {
      if (f32 && wa.lens)
        hipLaunchKernelGGL((yk_mt_warmup<true, true>), dim3(wblocks), dim3(256), 0, ctx->aux, wa);
      else if (f32)
        hipLaunchKernelGGL((yk_mt_warmup<false, true>), dim3(wblocks), dim3(256), 0, ctx->aux, wa);
      else if (defer && lp.tab_mode == kTabFill)
        hipLaunchKernelGGL(yk_mt_warmup_defer_tab<kTabFill>, dim3(wblocks), dim3(256), 0, ctx->aux, ta);
      else if (defer)
        hipLaunchKernelGGL(yk_mt_warmup_defer, dim3(wblocks), dim3(256), 0, ctx->aux, wa);
      else if (lp.tab_mode == kTabFill && wa.lens)
        hipLaunchKernelGGL((yk_mt_warmup_tab<true, kTabFill>), dim3(wblocks), dim3(256), 0, ctx->aux, ta);
      else if (lp.tab_mode == kTabFill)
        hipLaunchKernelGGL((yk_mt_warmup_tab<false, kTabFill>), dim3(wblocks), dim3(256), 0, ctx->aux, ta);
      else if (wa.lens)
        hipLaunchKernelGGL((yk_mt_warmup<true, false>), dim3(wblocks), dim3(256), 0, ctx->aux, wa);
      else
        hipLaunchKernelGGL((yk_mt_warmup<false, false>), dim3(wblocks), dim3(256), 0, ctx->aux, wa);
      YK_HIP(hipGetLastError());
    }
    YK_HIP(hipEventRecord(ev[1], ctx->aux));
    return YK_OK;
  };
  for (uint32_t c = 0; c < std::min(kWarmRing, nlaunch); ++c)
    if ((rc = warm(c))) return rc;
  if (warm_first) YK_HIP(hipStreamSynchronize(ctx->aux));
  uint32_t launches = 0;
  for (uint32_t c = 0; c < nlaunch; ++c) {
    hipEvent_t* ev = &ctx->lev[6 * c];
    const uint32_t s0 = sched[c].first, ks = sched[c].second;
    const uint32_t nsl = nps * ks;
    const uint64_t g = g0 + c;  // the launch's global number (ring slots, parity, stream)
    char* const wring = x128 ? nullptr : ctx->d_warm + (size_t)(g % kWarmRing) * nps * K * welem;
    double* col = ctx->d_col + (size_t)(g % kColRing) * nps * K * kColStride;
    ka.s0 = s0;
    ka.nsl = nsl;
    ka.col = col;
    ka.start = (const void*)wring;
    // Render launches alternate between the caller's stream and ctx->alt: launch c + 1 depends
    // only on its own start records and colour buffer, so its blocks take the CUs that launch c's
    // draining blocks free (per-lane scratch, slot counter and colours are per launch parity)
    const hipStream_t rs = (g & 1) ? ctx->alt : ctx->ren;
    const size_t lanes = (size_t)grid * block;
    ka.mt_scratch = ctx->d_mt ? ctx->d_mt + (g & 1) * lanes * ykd::kMtN : nullptr;
    ka.id_scratch = ctx->d_ids + (g & 1) * lanes * ctx->id_stride;
    YK_HIP(hipStreamWaitEvent(rs, ev[1], 0));  // its start records
    // its colour buffer: the reduce that last read it
    if (c >= kColRing)
      YK_HIP(hipStreamWaitEvent(rs, ctx->lev[6 * (c - kColRing) + 5], 0));
    else if (ov)
      YK_HIP(hipStreamWaitEvent(rs, gdep(g0 + c - kColRing, 1), 0));
    ka.pixel_counter = ctx->d_counter + (x128 ? c : (uint32_t)(g % kWarmRing));
    ka.clk = ctx->d_clk + 4 * c;
#ifdef YK_DRAIN_DIAG
    ka.diag_c = c;
    ka.diag_pad = 0;
#endif
    YK_HIP(hipEventRecord(ev[2], rs));
    const bool count = (ka.flags & YK_FLAG_COUNT_WORK) != 0;
    if (f32)
      hipLaunchKernelGGL(f32_kernel(plan.in_lds, (count ? 1 : 0) | (x128 ? 4 : 0)), dim3(grid), dim3(block),
                         plan.lds_bytes, rs, ka);
    else
      hipLaunchKernelGGL(fp64_kernel(plan.in_lds, (count ? 1 : 0) | (ka.seed_mode == YK_SEED_RANDOM_DEVICE ? 2 : 0) |
                                                      (x128 ? 4 : 0)),
                         dim3(grid), dim3(block), plan.lds_bytes, rs, ka);
    YK_HIP(hipGetLastError());
    YK_HIP(hipEventRecord(ev[3], rs));
    YK_HIP(hipEventRecord(gdep(g, 0), rs));
    ra.col = col;
    ra.nsl = nsl;
    ra.ks = ks;
    ra.first = s0 == 0;
    ra.last = s0 + ks == s_end;
    // the launch's samples of the sky blocks, on the reduce stream ahead of the launch's reduce:
    // they run beside the render, in the gap the short reduces leave on that stream (behind the
    // warm-ups on ctx->aux, which is busy 97% of a step, they delayed every warm-up after them:
    // bench +1.2%, profiles/r18_sky_blocks/); the last one writes the caller's image, and the
    // call's last reduce, which the caller waits for, follows it
    if (lp.culled && (rc = enqueue_sky(ctx, ctx->red, la.sa, s0, ks, s_end, ov, lp.tab_mode, lp.tab_T))) return rc;
    YK_HIP(hipStreamWaitEvent(ctx->red, ev[3], 0));
    if (ov && !film && ra.last) YK_HIP(hipStreamWaitEvent(ctx->red, ctx->ev0, 0));  // the caller's image
    YK_HIP(hipEventRecord(ev[4], ctx->red));
    if (group) {
      fm.col = col;
      fm.ks = ks;
      // (a later group of the pass may have the count these slots now reach)
      fm.take = s0 + ks == s_end ? film->d_take : nullptr;
      hipLaunchKernelGGL(yk_film_reduce_masked, dim3(reduce_blocks(ctx, nps)), dim3(256), 0, ctx->red, fm);
    } else if (film) {
      // (the reduces of a chunk, and of the chunks before it, run in order on ctx->red)
      fa.col = col;
      fa.ks = ks;
      hipLaunchKernelGGL(yk_film_reduce, dim3(reduce_blocks(ctx, nps)), dim3(256), 0, ctx->red, fa);
    } else {
      hipLaunchKernelGGL(yk_reduce_samples, dim3(reduce_blocks(ctx, nps)), dim3(256), 0, ctx->red, ra);
    }
    YK_HIP(hipGetLastError());
    YK_HIP(hipEventRecord(ev[5], ctx->red));
    YK_HIP(hipEventRecord(gdep(g, 1), ctx->red));
    if (c + kWarmRing < nlaunch && (rc = warm(c + kWarmRing))) return rc;
    ++launches;
  }
  YK_HIP(hipStreamWaitEvent(st, ctx->lev[6 * (nlaunch - 1) + 5], 0));  // the caller sees the image
  YK_HIP(hipEventRecord(ctx->ev1, st));
  ctx->g_next = g0 + nlaunch;
  ctx->prev_n = nlaunch;
  ctx->run_len = (same_run ? ctx->run_len : 0) + nlaunch;
  ctx->prev_geom = geom;
  ctx->prev_shape = lp.shape;
  ctx->prev_ok = !x128 && !warm_first;
  ctx->prev_enqueued = true;
  ctx->dirty = false;
  *launches_out = launches;
  return YK_OK;
}

// The call's statistics, as far as the host knows them (finish_stats adds the device's)
static void call_stats(ykgpu_context* ctx, const yk_render_params* p, const double* sums_dev, const ykgpu_film* film,
                       const LaunchPlan& lp, uint32_t launches) {
  const bool x128 = lp.x128;
  const int grid = lp.grid, block = lp.block;
  const uint32_t nps = lp.nps, K = lp.K, nlaunch = lp.nlaunch, kWarmRing = lp.kWarmRing, kColRing = lp.kColRing;
  const size_t welem = lp.welem, retry_n = lp.retry_n;
  const uint32_t retry_cap = lp.retry_cap;
  ctx->stats = yk_render_stats{};
  ctx->stats.samples = (uint64_t)p->row_count * tile_width(p) * lp.spp;
  ctx->stats.launches = launches;
  ctx->stats.grid_blocks = (uint32_t)grid;
  ctx->stats.launch_spp = K;
  ctx->stats.mem_shrinks = lp.mem_shrinks;
  ctx->stats.seed_key = lp.seed_key;
  // what this call needed (device_bytes: what the context holds)
  {
    const uint64_t lanes = (uint64_t)grid * block;
    uint64_t cb = ctx->t64.bytes + ctx->t32.bytes +
                  (uint64_t)ctx->nspheres * (sizeof(SphereGeo) + sizeof(SphereMat) + sizeof(float4));
    cb += (uint64_t)kColRing * nps * K * kColStride * sizeof(double) + (x128 ? 0 : (uint64_t)kWarmRing * nps * K * welem);
    cb += (film ? (uint64_t)nps * 6 * sizeof(double) : nlaunch > 1 ? (uint64_t)nps * 3 * sizeof(double) : 0) +
          (uint64_t)nps * sizeof(uint32_t);
    cb += nlaunch * sizeof(uint32_t) + kCounters * sizeof(unsigned long long);
    if (retry_cap) cb += retry_n * sizeof(uint4);
    // (a culled call: the sky slots' order, sums and engines; its path order is counted above)
    if (lp.culled) cb += sky_bytes(ctx) - (uint64_t)nps * sizeof(uint32_t);
    if (!x128) cb += 2 * lanes * ykd::kMtN * sizeof(uint32_t);
    cb += 2 * lanes * std::max(1u, p->max_depth > kStackRegs ? p->max_depth : 1u) * sizeof(uint16_t);
    const uint64_t npix = (uint64_t)p->row_count * tile_width(p);
    cb += npix * 3 + (sums_dev ? npix * 3 * sizeof(double) : 0);
    ctx->stats.call_bytes = cb;
  }
  ctx->stats_pending = true;
}

int launch(ykgpu_context* ctx, const yk_render_params* p, uint8_t* rgb_dev, double* sums_dev, hipStream_t st,
           uint32_t s_begin, uint32_t s_end, ykgpu_film* film) {
  LaunchPlan lp;
  LaunchArgs la;
  uint32_t launches = 0;
  int rc = plan_launch(ctx, p, s_begin, s_end, film, lp);
  if (!rc) rc = fill_args(ctx, p, rgb_dev, sums_dev, film, lp, la);
  if (!rc && lp.culled && lp.nps == 0)
    rc = enqueue_sky_only(ctx, st, s_begin, s_end, lp, la);
  else if (!rc)
    rc = enqueue_launches(ctx, st, s_end, film, lp, la, &launches);
  if (!rc) rc = seed_table_used(ctx, lp);
  // A call that failed part-way may have enqueued table kernels under its split.  The two events
  // are recorded behind whatever it enqueued (best effort: the streams may be what failed) and the
  // split is set to a value no sky_key has, so the next call that uses the table makes both streams
  // wait for both events whatever its own split; the host wait ctx->dirty brings comes on top.
  if (rc && lp.tab_mode != kTabWalk) {
    if (ctx->seed_ev_aux && ctx->seed_ev_red && hipEventRecord(ctx->seed_ev_aux, ctx->aux) == hipSuccess &&
        hipEventRecord(ctx->seed_ev_red, ctx->red) == hipSuccess)
      ctx->seed_ev_set = true;
    else
      (void)hipGetLastError();
    ctx->seed_tab_part = {~0ull};
  }
  if (!rc) call_stats(ctx, p, sums_dev, film, lp, launches);
  return rc;
}

// (the hooks below)
bool seed_table_drop_hook(ykgpu_context* ctx) { return seed_table_drop(ctx); }
void seed_table_test_hook(uint32_t flip) { g_seed_tab_flip.store(flip); }

}  // namespace ykhost

extern "C" {

// The seed table's switches and its test hook: not part of the C-ABI (include/ykgpu.h does not
// declare them), like yk_features_sampled_lazy_words.  The library reads no environment variable
// for the table (tests/test_integration_doc.py pins the two it reads); the Python package reads YKGPU_SEED_TABLE and YKGPU_SEED_TABLE_MAX_MB when it
// creates a context and hands them over here.
// on == 0 turns the context's table off (and gives back one it holds); max_bytes caps its size.
void yk_seed_table_configure(ykgpu_context* ctx, int on, uint64_t max_bytes) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  ctx->seed_tab_on = on != 0;
  ctx->seed_tab_max_bytes = max_bytes;
  if (!on || ctx->seed_tab_words * sizeof(uint32_t) > max_bytes) ykhost::seed_table_drop_hook(ctx);
}
// For the tests (tests/test_gpu_seed_table.py), process-wide: flip is xor-ed into every word a fill
// stores from now on, so that the pixels of a kernel that reads the table come out different from
// those of one that walks, which proves the read ran.  (A hook and not a build with a -D, as the
// other fallback tests have: tests/test_build_knobs.py pins the Makefile's list of test variants.
// A caller that sets it gets wrong images from reading calls; nothing in the product calls it.)
void yk_seed_table_test(uint32_t flip) { ykhost::seed_table_test_hook(flip); }

}  // extern "C"
