// ykgpu_render.hip — the per-pixel sampling loop of UECRayTracing on gfx950 (MI355X), and the
// C-ABI (include/ykgpu.h) around it.
//
// Replaces /root/reference/source.cpp:122-172 (for_each over (row,col) → transform_reduce over
// samples → to_color3b) and the recursion of yk/raytracer.hpp:19-37.
//
// Execution model:
//   * a render call is a sequence of LAUNCHES of K samples per pixel (a synced call: 4, 8, 16,
//     then at most kLaunchSpp = 32 for the frame: 1920x1080x512 is 4, 8, 16, 14 x 32, 18, 18; a
//     call enqueued while the previous one still runs: kLaunchSppOv = 64, 8 x 64).  Per launch: yk_mt_warmup (second
//     stream: every sample's mt19937 seeding walk and its start draws — jitter and lens — and
//     camera ray, as a StartRec), yk_render_persistent (the paths, on one of two top-priority
//     streams), yk_reduce_samples (the reference's strictly sequential per-pixel sum and
//     to_color3b, third stream).  Back-to-back calls overlap (launches numbered across calls).
//   * yk_render_persistent is one persistent grid of 768-thread workgroups, one per CU (12 waves,
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
#include <chrono>
#include <random>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../include/ykgpu.h"
#include "yk_film_internal.hpp"
#include "yk_render_device.hpp"
#include "yk_schedule.hpp"

namespace {

thread_local std::string g_last_error;

int fail(int code, const std::string& msg) {
  g_last_error = msg;
  return code;
}

#define YK_HIP(call)                                                                      \
  do {                                                                                    \
    hipError_t e_ = (call);                                                               \
    if (e_ != hipSuccess)                                                                 \
      return fail(e_ == hipErrorOutOfMemory ? YK_ERR_NOMEM : YK_ERR_DEVICE,               \
                  std::string(#call) + ": " + hipGetErrorString(e_));                     \
  } while (0)

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
template <bool kLens, bool kF32, bool kDefer, uint32_t kIlp>
__device__ __forceinline__ void mt_warmup_body(const WarmArgs& wa) {
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
  // slot i's pixel (xx, y) and seed; an empty slot gets column kPadX (its record is marked)
  auto slot_seed = [&](uint32_t i, uint32_t& xx, uint32_t& y) -> uint32_t {
    const uint32_t sl = fdiv(i, wa.nps_m, wa.nps_sh), pp = i - sl * wa.npix_slots;
    const uint32_t q = wa.order[pp];
    const uint32_t pix = q == kNoPixel ? 0u : q;
    const uint32_t tr = fdiv(pix, wa.w_m, wa.w_sh);
    xx = tile_col_x(wa.col_begin, wa.col_stride, wa.col_band, pix - tr * wa.Wt);
    y = tile_row_y(wa.row_begin, wa.row_stride, wa.band_log2, tr);
    const uint32_t seed = ykd::sample_seed(wa.seed_mode, wa.seed_key, wa.seed0, y, xx, wa.W, wa.spp, wa.s0 + sl);
    xx = q == kNoPixel ? kPadX : xx;
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
#pragma unroll
      for (uint32_t k = kIlp - 1; k > 0; --k) {
        const uint32_t ik = i + k * stride;
        x[k] = slot_seed(ik < n ? ik : i, xx, y);
      }
      const uint32_t seed = slot_seed(i, xx, y);
      x[0] = seed;
      ykd::mt_walk397xn<kIlp>(x);
      start_slot(i, xx, y, seed, x[0]);
#pragma unroll
      for (uint32_t k = 1; k < kIlp; ++k) {
        const uint32_t ik = i + k * stride;
        if (ik < n) {
          const uint32_t sk = slot_seed(ik, xx, y);
          start_slot(ik, xx, y, sk, x[k]);
        }
      }
    }
  } else {
    for (uint32_t i = blockIdx.x * kWarmBlock + threadIdx.x; i < n; i += stride) {
      uint32_t xx, y;
      const uint32_t seed = slot_seed(i, xx, y);
      uint32_t x[1] = {seed};
      ykd::mt_walk397xn<1>(x);
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
  const size_t o3 = (size_t)q * 3;
  const double spp = (double)ra.spp;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    if (ra.sums) ra.sums[o3 + c] = a[c];
    double v = ykd::nsqrt(a[c] / spp);
    v = (v < 0.0) ? 0.0 : (0.999 < v) ? 0.999 : v;
    ra.rgb[o3 + c] = (uint8_t)(uint32_t)(v * 256);
  }
}
__global__ __launch_bounds__(256) void yk_reduce_samples(ReduceArgs ra) {
  for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p < ra.npix_slots; p += gridDim.x * blockDim.x)
    reduce_slot(ra, p);
}

// ---- progressive film (include/ykgpu.h) ------------------------------------------------------
// A film keeps, per processing slot p and channel c, the running sum s and the running second
// moment q as six planes plane[c * npix_slots + p] (s: c = 0..2, q: c = 3..5) — slot order, the
// order the launches' colours arrive in, so every access of the fold below is coalesced like
// yk_reduce_samples' — and its own copy of the slot → pixel order, so that neither the planes nor
// their meaning depend on what the context renders between two chunks.
// The arithmetic the host tests restate in numpy (film_add, film_sub, film_mul, film_div: each
// operation rounded on its own, never fused) is in yk_film_internal.hpp, shared with yk_denoise.hip.

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

// to_color3b (source.cpp:73-83) of a film's sums at the divisor `done`, as reduce_slot's last step;
// count (null for a uniform film): each slot's own divisor, 0 giving black
__global__ __launch_bounds__(256) void yk_film_resolve(const double* plane, const uint32_t* order, uint8_t* rgb,
                                                      uint32_t npix_slots, uint32_t done, const uint32_t* count) {
  for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p < npix_slots; p += gridDim.x * blockDim.x) {
    const uint32_t px = order[p];
    if (px == kNoPixel) continue;
    const uint32_t np = count ? count[p] : done;
    if (np == 0) {
      rgb[(size_t)px * 3] = rgb[(size_t)px * 3 + 1] = rgb[(size_t)px * 3 + 2] = 0;
      continue;
    }
    const double n = (double)np;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      double v = ykd::nsqrt(plane[(size_t)c * npix_slots + p] / n);
      v = (v < 0.0) ? 0.0 : (0.999 < v) ? 0.999 : v;
      rgb[(size_t)px * 3 + c] = (uint8_t)(uint32_t)(v * 256);
    }
  }
}

// e2 of slot p at n samples (include/ykgpu.h ykgpu_film_error): max(0, v_r, v_g, v_b),
// v_c = (q_c - (s_c * s_c) / n) / (n * (n - 1)), each operation rounded on its own
__device__ __forceinline__ double film_e2(const double* plane, uint32_t npix_slots, uint32_t p, double n) {
  const double den = film_mul(n, film_sub(n, 1.0));
  double e2 = 0.0;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double s = plane[(size_t)c * npix_slots + p], q = plane[(size_t)(3 + c) * npix_slots + p];
    const double v = film_div(film_sub(q, film_div(film_mul(s, s), n)), den);
    if (v > e2) e2 = v;
  }
  return e2;
}

// The error map of a film: per pixel film_e2.  Optionally stores the map (pixel order), and
// reduces the number of pixels with e2 > threshold2 and the maximum: each thread keeps its own
// over its grid-stride pixels, a wave combines them with lane exchanges, and lane 0 issues one
// atomic each per wave.  e2 >= 0, so doubles order like their bit patterns and the maximum is an
// integer atomicMax; both results are independent of the order of combination.  count (null for
// a uniform film): each slot's own n; below 2 the slot's e2 is +inf.
__global__ __launch_bounds__(256) void yk_film_error(const double* plane, const uint32_t* order, double* e2_out,
                                                    unsigned long long* result, uint32_t npix_slots, uint32_t done,
                                                    double threshold2, const uint32_t* count) {
  unsigned long long over = 0, top = 0;
  for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p < npix_slots; p += gridDim.x * blockDim.x) {
    const uint32_t px = order[p];
    if (px == kNoPixel) continue;
    const uint32_t np = count ? count[p] : done;
    const double e2 = np < 2 ? __longlong_as_double(0x7ff0000000000000ll) : film_e2(plane, npix_slots, p, (double)np);
    if (e2_out) e2_out[px] = e2;
    over += e2 > threshold2 ? 1u : 0u;
    const unsigned long long bits = (unsigned long long)__double_as_longlong(e2);
    top = bits > top ? bits : top;
  }
  // (every lane reaches this point: the loop above has no early exit)
  for (int off = 32; off > 0; off >>= 1) {
    over += __shfl_xor(over, off, 64);
    const unsigned long long o = __shfl_xor(top, off, 64);
    top = o > top ? o : top;
  }
  if ((threadIdx.x & 63u) == 0) {
    if (over) atomicAdd(&result[0], over);
    if (top) atomicMax(&result[1], top);
  }
}

// ---- adaptive passes (include/ykgpu.h "adaptive passes") ----------------------
// A film also keeps count[p], the samples slot p holds.  A pass gives samples only to selected
// slots: yk_film_select decides, per candidate count value yk_film_group_* compact the selected
// slots of that count into a processing order of their own (padded with kNoPixel to whole waves:
// the warm-up marks such slots kPadSlot, the render skips them) plus the map back to the film's
// slots, launch() renders that order, and yk_film_reduce_masked folds through the map.
constexpr uint32_t kFilmVals = 64;  // candidate count values per yk_film_select launch

__global__ __launch_bounds__(256) void yk_film_fill_counts(uint32_t* count, uint32_t npix_slots, uint32_t v) {
  for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p < npix_slots; p += gridDim.x * blockDim.x) count[p] = v;
}

// Selection on the state before the pass: slot p with n = count[p] is selected iff n < target and
// (n < 2 or e2 > threshold2), and then takes min(n_samples, target - n) samples; take[p] = 0
// otherwise.  first: vals[0..nvals) are the first candidates of the pass and take[] is written;
// later launches (more than kFilmVals candidates) only count.  Per candidate value v:
// hist[v] += the selected slots holding vals[v] — a wave ballot and one atomic per wave and value.
struct FilmSelectArgs {
  const double* plane;
  const uint32_t* order;
  const uint32_t* count;
  uint32_t* take;
  unsigned long long* hist;
  uint32_t npix_slots, target, n_samples, nvals, first, pad;
  double threshold2;
  uint32_t vals[kFilmVals];
};
__global__ __launch_bounds__(256) void yk_film_select(FilmSelectArgs sa) {
  // (whole waves run every trip: the ballots below need all lanes of a wave in step)
  const uint32_t trips = (sa.npix_slots + gridDim.x * blockDim.x - 1) / (gridDim.x * blockDim.x);
  for (uint32_t t = 0; t < trips; ++t) {
    const uint32_t p = (t * gridDim.x + blockIdx.x) * blockDim.x + threadIdx.x;
    const bool live = p < sa.npix_slots && sa.order[p] != kNoPixel;
    uint32_t n = 0, tk = 0;
    if (live) {
      n = sa.count[p];
      if (n < sa.target && (n < 2 || film_e2(sa.plane, sa.npix_slots, p, (double)n) > sa.threshold2))
        tk = min(sa.n_samples, sa.target - n);
    }
    if (sa.first && p < sa.npix_slots) sa.take[p] = tk;
    for (uint32_t v = 0; v < sa.nvals; ++v) {
      const unsigned long long sel = __ballot(tk != 0 && n == sa.vals[v]);
      if (sel && (threadIdx.x & 63u) == 0) atomicAdd(&sa.hist[v], (unsigned long long)__popcll(sel));
    }
  }
}

// Stable compaction of the selected slots holding `value`, in ascending slot order (the 8x8 block
// locality of the film's order survives), with no atomics on the output position: block b covers
// slots [256 b, 256 b + 256); yk_film_group_count leaves each block's total, yk_film_group_scan
// (one block) turns the totals into exclusive offsets, yk_film_group_write places every member at
// offset + members before it in its block (wave ballots and popcounts).
__device__ __forceinline__ bool film_member(const uint32_t* count, const uint32_t* take, uint32_t npix_slots,
                                            uint32_t p, uint32_t value) {
  return p < npix_slots && take[p] != 0 && count[p] == value;
}
__global__ __launch_bounds__(256) void yk_film_group_count(const uint32_t* count, const uint32_t* take,
                                                          uint32_t* block_tot, uint32_t npix_slots, uint32_t value) {
  __shared__ uint32_t wtot[4];
  const uint32_t p = blockIdx.x * 256u + threadIdx.x;
  const unsigned long long m = __ballot(film_member(count, take, npix_slots, p, value));
  if ((threadIdx.x & 63u) == 0) wtot[threadIdx.x >> 6] = (uint32_t)__popcll(m);
  __syncthreads();
  if (threadIdx.x == 0) block_tot[blockIdx.x] = wtot[0] + wtot[1] + wtot[2] + wtot[3];
}
__global__ __launch_bounds__(256) void yk_film_group_scan(uint32_t* block_tot, uint32_t nblocks) {
  __shared__ uint32_t wsum[4];
  __shared__ uint32_t carry_s;
  if (threadIdx.x == 0) carry_s = 0;
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  for (uint32_t base = 0; base < nblocks; base += 256u) {
    const uint32_t i = base + threadIdx.x;
    const uint32_t v = i < nblocks ? block_tot[i] : 0u;
    uint32_t inc = v;  // inclusive scan within the wave
    for (uint32_t off = 1; off < 64; off <<= 1) {
      const uint32_t o = __shfl_up(inc, off, 64);
      if (lane >= off) inc += o;
    }
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    uint32_t before = carry_s;
    for (uint32_t k = 0; k < w; ++k) before += wsum[k];
    if (i < nblocks) block_tot[i] = before + inc - v;
    __syncthreads();
    if (threadIdx.x == 255) carry_s = before + inc;
    __syncthreads();
  }
}
__global__ __launch_bounds__(256) void yk_film_group_write(const uint32_t* count, const uint32_t* take,
                                                          const uint32_t* order, const uint32_t* block_off,
                                                          uint32_t* g_order, uint32_t* g_map, uint32_t npix_slots,
                                                          uint32_t value, uint32_t g_slots) {
  __shared__ uint32_t wtot[4];
  const uint32_t p = blockIdx.x * 256u + threadIdx.x, w = threadIdx.x >> 6;
  const bool mem = film_member(count, take, npix_slots, p, value);
  const unsigned long long m = __ballot(mem);
  if ((threadIdx.x & 63u) == 0) wtot[w] = (uint32_t)__popcll(m);
  __syncthreads();
  if (!mem) return;
  uint32_t pos = block_off[blockIdx.x];
  for (uint32_t k = 0; k < w; ++k) pos += wtot[k];
  pos += __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
  if (pos < g_slots) {  // (always: g_slots holds the group, counted by yk_film_select)
    g_order[pos] = order[p];
    g_map[pos] = p;
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

// The refined reciprocal of every radius, by the same instructions the division sequence uses
// (rcp_refined), so the hit normal's (p - c) / radius reuses it (divs_fast_r: bit-identical to
// divs_fast).  Run once per set_scene.
__global__ void yk_mat_prep(SphereMat* m, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    m[i].inv_r = ykd::rcp_refined(m[i].radius);
    m[i].inv_rf = ykf::rcp_refined((float)m[i].radius);
  }
}

// ykgpu_math_div: the renderer's vector / scalar division (divs_fast) on a buffer (diagnostic).
__global__ __launch_bounds__(256) void yk_math_div(const double* num3, const double* den, double* out3,
                                                  uint64_t n) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const ykd::v3 q = ykd::divs_fast({num3[3 * i], num3[3 * i + 1], num3[3 * i + 2]}, den[i]);
  out3[3 * i] = q.x;
  out3[3 * i + 1] = q.y;
  out3[3 * i + 2] = q.z;
}

// ykgpu_math_div_f32: the FP32 kernel's vector / scalar division (ykf::divs_fast) on a buffer.
__global__ __launch_bounds__(256) void yk_math_div_f32(const float* num3, const float* den, float* out3, uint64_t n) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const ykf::v3 q = ykf::divs_fast({num3[3 * i], num3[3 * i + 1], num3[3 * i + 2]}, den[i]);
  out3[3 * i] = q.x;
  out3[3 * i + 1] = q.y;
  out3[3 * i + 2] = q.z;
}

// ykgpu_math_sqrt: the device's math::sqrt on a buffer (diagnostic entry point).
__global__ __launch_bounds__(256) void yk_math_sqrt(const double* in, double* out, uint64_t n) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = ykd::nsqrt(in[i]);
}

// ykgpu_math_sqrt_f32: the FP32 path's math::sqrt<float> on a buffer (diagnostic).
__global__ __launch_bounds__(256) void yk_math_sqrt_f32(const float* in, float* out, uint64_t n) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t it = 0;
  if (i < n) out[i] = ykf::nsqrt(in[i], it);
}

}  // namespace

// the render units' instances (yk_render_f64.hip, yk_render_f32.hip), by (scene in LDS, kMode)
namespace {
RenderKernel fp64_kernel(bool lds, int mode) { return (RenderKernel)yk_fp64_kernel(lds, mode); }
RenderKernel f32_kernel(bool lds, int mode) { return (RenderKernel)yk_f32_kernel(lds, mode); }
}  // namespace

// =========================================================================================
// C-ABI
// =========================================================================================
// (the host-side tuning constants and the launch schedule rule: yk_schedule.hpp)
// the render kernel addresses a slot's start record as 4 * slot uint4s (FP32: 3) in 32-bit
// arithmetic
static_assert(kLaunchBytes / (8 * kColStride) * 4 < (1ull << 32), "4 * slot must fit 32 bits");
static_assert(yksched::kColourBytes == kColStride * sizeof(double), "yk_schedule.hpp's colour record");

// A BVH on the device: the FP64 kernel's (boxes grown for the exact test's rounding, DESIGN.md
// §4) or the FP32 kernel's (grown for render<float>'s sphere test, §4.1), with its LDS layout
// [nodes][leaf geometry][leaf ids][traversal stacks] and the persistent grid it leaves room for.
struct DevTree {
  DevNode* nodes = nullptr;
  void* leaf_geo = nullptr;      // SphereGeo (FP64) or float4 (FP32), in leaf order
  uint32_t* leaf_ids = nullptr;  // leaf slot → tuple index
  int32_t root = 0;              // root code (byte offset of the root node, or a leaf code)
  uint32_t depth = 0, n_nodes = 0;
  double origin_bound = 0;  // |o|_inf beyond which a ray takes the linear scan (< 0: every ray)
  uint32_t geo_off = 0, ids_off = 0;  // leaf geometry and ids in LDS, after the nodes
  size_t bytes = 0;                   // device bytes of nodes, leaf geometry and ids
  // LDS plan per kernel shape: [0] kBlock threads (mt19937 instances), [1] kBlockX128 (xor128)
  struct Plan {
    bool in_lds = false;
    uint32_t lds_bytes = 0, stack_off = 0, stack_cap = 0, stack_entries = 0;
    bool stack_check = true;  // the kernel checks the stack top against stack_cap
    uint32_t tgeo_off = 0, mat_off = 0;  // shading tables in LDS (FP64 kernel), 0: none
    int grid = 0;                        // persistent blocks: occupancy x CUs
  } plan[2];
  void release() {
    (void)hipFree(nodes);
    (void)hipFree(leaf_geo);
    (void)hipFree(leaf_ids);
    nodes = nullptr;
    leaf_geo = nullptr;
    leaf_ids = nullptr;
    bytes = 0;
  }
};

struct ykgpu_context {
  int device = 0;
  int cus = 0;
  DevTree t64, t32;  // the FP64 and FP32 kernels' trees over the current scene
  size_t scratch_lanes = 0;
  char* d_warm = nullptr;  // warm-up ring: a StartRec (FP64) or StartRecF (FP32) per sample slot
  uint4* d_retry = nullptr;  // the FP64 warm-ups' lens-retry rings: retry_cap x 48 B per wave
  size_t retry_cap = 0;
  double* d_col = nullptr;     // sample colours of one launch (kColStride doubles per slot)
  double* d_acc = nullptr;     // running per-pixel sums between launches
  size_t col_cap = 0, acc_cap = 0;
  uint32_t* d_order = nullptr;  // processing slot → tile pixel, for (order_w, order_rows)
  uint32_t order_w = 0, order_rows = 0, order_slots = 0, order_stride = 0, order_mode = 0;
  size_t warm_cap = 0;
  hipStream_t stream = nullptr;
  hipStream_t aux = nullptr;  // the MT warm-ups run here, beside the render launches
  hipStream_t red = nullptr;  // the ordered reduces run here, beside the next render launch
  hipStream_t alt = nullptr;  // odd render launches: a launch starts while the previous drains
  hipStream_t ren = nullptr;  // even render launches (alt and ren: the device's top stream priority)
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  std::vector<hipEvent_t> lev;  // per launch: warm-up start, render start, reduce start, end
  uint32_t lev_used = 0;
  // Cross-call pipelining (launch()): the previous call's per-launch events and ring geometry, and
  // a global launch counter that numbers the ring slots, the scratch parity and the render
  // stream across calls
  std::vector<hipEvent_t> lev_prev;
  uint32_t lev_prev_used = 0;  // (events of the previous call in lev_prev: YKGPU_TIMELINE prints them)
  uint32_t prev_n = 0;
  // per global launch number g (mod kDepRing): its render's end and its reduce's end, the events a
  // later launch that reuses its start-record or colour buffer waits for, whichever call it was in
  std::vector<hipEvent_t> gev;
  // launches enqueued back to back with the current ring geometry (prev_geom), over calls: a call
  // overlaps the ones before it only when the last max(ring depths) launches had its geometry
  uint64_t run_len = 0;
  // the previous call's ring and scratch geometry: a call overlaps it only when every field is
  // equal (launch() `ov`; equal slot offsets in every ring buffer and scratch slice)
  struct RingGeom {
    uint64_t nps = 0, K = 0, welem = 0, warm_ring = 0, col_ring = 0, lanes = 0, id_stride = 0;
    const void *warm = nullptr, *col = nullptr, *mt = nullptr, *ids = nullptr;
    bool operator==(const RingGeom& o) const {
      return nps == o.nps && K == o.K && welem == o.welem && warm_ring == o.warm_ring && col_ring == o.col_ring &&
             lanes == o.lanes && id_stride == o.id_stride && warm == o.warm && col == o.col && mt == o.mt &&
             ids == o.ids;
    }
  } prev_geom;
  uint64_t prev_shape = 0;  // (nps, kmax, precision, engine) of the previous call: launch() `inflight`
  bool prev_ok = false;
  bool prev_enqueued = false;  // the previous call's launches were all enqueued (its events exist)
  bool dirty = false;          // a call failed part-way: its enqueued work is not tracked
  uint64_t g_next = 0;
  SphereGeo* d_geo = nullptr;
  SphereMat* d_mat = nullptr;
  float4* d_geo_f = nullptr;  // FP32 geometry (cx, cy, cz, r*r in float), tuple order
  uint32_t nspheres = 0;
  yk_camera cam{};
  bool have_scene = false;
  uint64_t scene_gen = 0;  // counts ykgpu_set_scene calls: a film renders only the scene it was created with
  uint32_t* d_counter = nullptr;        // sample-slot counters, one per launch of a call
  uint32_t counter_cap = 0;
  unsigned long long* d_clk = nullptr;  // shader-clock probes, 4 words per launch (YK_CLOCK_*)
  unsigned long long* d_stats = nullptr;  // kCounters counters
  uint32_t* d_mt = nullptr;            // grid*256*624 words
  uint16_t* d_ids = nullptr;            // grid*256*id_stride
  uint32_t id_stride = 0;
  size_t id_lanes = 0;
  uint8_t* d_rgb = nullptr;
  size_t rgb_cap = 0;
  double* d_sums = nullptr;
  size_t sums_cap = 0;
  yk_render_stats stats{};
  bool stats_pending = false;
  double* d_trace = nullptr;  // ykgpu_render_trace's buffers (only during that call)
  uint32_t* d_trace_counts = nullptr;
  uint32_t trace_cap = 0;
  std::chrono::steady_clock::time_point t0;
};

// A film (include/ykgpu.h): the accumulation state of one tile, owned by the film — the six planes
// (yk_film_reduce) and the processing order they are laid out in, on the device and on the host
// (read and write permute there) — plus what fixes its samples: the params, with the seed key
// drawn at create, and the scene generation.
struct ykgpu_film {
  ykgpu_context* ctx = nullptr;
  int device = 0;
  yk_render_params p{};
  uint64_t scene_gen = 0;
  uint32_t done = 0;
  uint32_t nps = 0;   // processing slots (>= pixels)
  uint64_t npix = 0;  // pixels of the tile
  double* d_plane = nullptr;   // 6 * nps
  uint32_t* d_order = nullptr;  // nps
  unsigned long long* d_result = nullptr;  // yk_film_error's count and maximum
  std::vector<uint32_t> order;
  bool torn = false;  // an accumulate failed part-way: the planes hold part of a chunk (until a write)
  // Adaptive passes.  hist: count value → pixels holding it (the host's whole knowledge of the
  // counts: a pass reads back one word per candidate value, never a per-pixel array).  While it
  // has one entry the film is uniform, `done` is that value and d_count is not kept up to date
  // (yk_film_reduce does not touch it): an adaptive pass fills it first.
  std::map<uint32_t, uint64_t> hist;
  uint32_t* d_count = nullptr;  // nps, slot order
  uint32_t* d_take = nullptr;   // nps: the pass's samples per slot, 0 = not selected
  uint32_t* d_blocks = nullptr;  // ceil(nps / 256): the compaction's block totals / offsets
  uint32_t* d_gorder = nullptr;  // the current group's processing order (g_slots of its nps-slot buffer)
  uint32_t* d_gmap = nullptr;    // ... and its slots' film slots
  unsigned long long* d_hist = nullptr;  // kFilmVals words
  uint32_t g_slots = 0;  // != 0: launch() renders the group (d_gorder, d_gmap) instead of the film's order
  // ykgpu_film_denoise's buffers (yk_denoise.hip), allocated at the film's first denoise
  void* d_denoise = nullptr;
  // ykgpu_film_features' planes (yk_features.hip), allocated at the first pass, and their grid
  void* d_features = nullptr;
  uint32_t feature_grid = 0;
  bool uniform() const { return hist.size() <= 1; }
};

struct ykgpu_group {
  std::vector<ykgpu_context*> ctx;  // one per entry of the device list
  std::vector<uint8_t*> tile;       // each entry's RGB8 tile on its device
  std::vector<size_t> tile_cap;
  std::vector<yk_render_stats> st;  // the last render's, per entry
  yk_render_stats total{};          // ... and of the whole call
};

namespace {

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
void fastdiv(uint32_t d, uint32_t& m, uint32_t& sh) {
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
int quiesce(ykgpu_context* ctx) {
  for (hipStream_t s : {ctx->aux, ctx->red, ctx->ren, ctx->alt, ctx->stream}) YK_HIP(hipStreamSynchronize(s));
  return YK_OK;
}

int ensure_scratch(ykgpu_context* ctx, uint32_t max_depth, size_t lanes, bool need_mt) {
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
    const uint32_t th = stride <= 1 ? kTile : (stride <= 4 ? std::max(1u, kTile / 2) : std::max(1u, kTile / 4));
    const uint32_t tw = kTile * kTile / th;
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
int ensure_order(ykgpu_context* ctx, uint32_t W, uint32_t rows, uint32_t stride) {
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
uint32_t col_ring() {
  uint32_t r = YK_COL_RING;
  if (const char* e = ab_knob("YKGPU_COL_RING")) r = (uint32_t)std::max(2, std::min(8, std::atoi(e)));
  return r;
}

// Reduce grid: grid-stride over the slots, at most 4 blocks per CU (YKGPU_RED_BLOCKS overrides;
// 0 = one thread per slot), so a reduce never floods the CUs a render launch is about to take
uint32_t reduce_blocks(const ykgpu_context* ctx, uint32_t nps) {
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
uint32_t warm_per_cu(bool f32) {
  uint32_t per_cu = f32 ? 2u : (uint32_t)YK_WARM_PER_CU;
  if (const char* e = ab_knob("YKGPU_WARM_PER_CU")) per_cu = (uint32_t)std::max(1, std::atoi(e));
  return per_cu;
}
// A warm-up's blocks for n slots, at most cap: each thread walks n / grid slots, at least
// kWarmSlots; with ilp walks per lane the grid is trimmed so that a thread's slot count is a
// multiple of ilp (no lane walks a chain for a slot it does not have, but in the last blocks)
inline uint32_t warm_blocks_for(uint64_t n, uint64_t cap, uint32_t ilp) {
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
};

// slots per warm-up wave of an FP64 launch of nl slots
uint64_t warm_wave_slots(const ykgpu_context* ctx, uint64_t nl) {
  const uint64_t wb = warm_blocks_for(nl, (uint64_t)ctx->cus * warm_per_cu(false), kWalkIlp);
  return (nl + wb * 256 - 1) / (wb * 256) * 64;
}

int plan_launch(ykgpu_context* ctx, const yk_render_params* p, uint32_t s_begin, uint32_t s_end,
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
  if (!film && (rc = ensure_order(ctx, tile_width(p), p->row_count, order_stride(p)))) return rc;
  // (a group of an adaptive pass: the film's compacted order of the pixels that take this window)
  const bool group = lp.group = film && film->g_slots != 0;
  lp.order = group ? film->d_gorder : film ? film->d_order : ctx->d_order;
  // Launch schedule (samples per pixel per launch; the rule is yk_schedule.hpp's): a ramp up to
  // kmax (kLaunchSpp = 32, or more for a small tile), also capped by the colour budget (32 B per
  // sample slot, kLaunchBytes per launch); a short remainder is folded into the launches before
  // it.  Each launch ends with the tail of its longest paths (~0.1-0.2 ms of partly idle CUs), but
  // launches alternate between two streams, so that drain overlaps the next launch: many mid-sized
  // launches beat a few large ones.  Independent of the image size, which matters
  // for the per-rank tiles of N GPUs.
  const uint32_t nps = lp.nps = group ? film->g_slots : film ? film->nps : ctx->order_slots;  // processing slots (>= pixels)
  // samples per pixel of this call (p->samples_per_pixel stays the stride of the seeds)
  const uint32_t spp = lp.spp = s_end - s_begin;
  // the rings' launch size (an in-flight call's launches) and a synced call's, <= it
  const yksched::LaunchSizes sizes = yksched::launch_sizes(nps, spp, (uint64_t)grid * block);
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
    const size_t need_warm = x128 ? 0 : (size_t)kWarmRing * nps * K * welem;
    const size_t need_col = (size_t)kColRing * nps * K * kColStride * sizeof(double);
    if (kmax > kfloor && (need_warm > ctx->warm_cap || need_col > ctx->col_cap * sizeof(double))) {
      // the rings must grow: does the device have room for them?
      size_t free_b = 0, total_b = 0;
      if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
        const size_t held = ctx->warm_cap + ctx->col_cap * sizeof(double);
        if (need_warm + need_col + kMemReserve > free_b + held) {
          shrink();
          continue;
        }
      }
    }
    rc = x128 ? YK_OK : grow(ctx->d_warm, ctx->warm_cap, need_warm, 1);
    if (!rc) rc = grow(ctx->d_col, ctx->col_cap, (size_t)kColRing * nps * K * kColStride, sizeof(double));
    if (rc == YK_ERR_NOMEM && kmax > kfloor) {
      (void)hipGetLastError();  // (the failed hipMalloc's error must not surface at a later launch)
      shrink();
      continue;
    }
    if (rc) return rc;
    break;
  }
  if (!film && sched.size() > 1 && (rc = grow(ctx->d_acc, ctx->acc_cap, (size_t)nps * 3, sizeof(double)))) return rc;
  // The FP64 lens warm-ups of launches with at most kDeferSlots slots per warm-up wave draw their
  // lens retries after the walks (yk_mt_warmup_defer) from a ring per wave, sized to the largest
  // such launch (the frame's 32-spp launches: 640 records, 1.0 GB); longer launches run the
  // rejection loop in line (config 5's 128-spp launches: 8100 slots per wave; at 121 spp, 7600 per
  // wave, the deferral measured 0.7% slower)
  const bool lens_defer = !x128 && !f32 && ctx->cam.lens_radius > 0;
  uint32_t& retry_cap = lp.retry_cap = 0;  // records per wave
  if (lens_defer)
    for (const auto& l : sched)
      if (warm_wave_slots(ctx, (uint64_t)nps * l.second) <= kDeferSlots)
        retry_cap = std::max(retry_cap, retry_cap_for(warm_wave_slots(ctx, (uint64_t)nps * l.second)));
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
};

int fill_args(const ykgpu_context* ctx, const yk_render_params* p, uint8_t* rgb_dev, double* sums_dev,
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
  fastdiv(nps, wa.nps_m, wa.nps_sh);
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
  return YK_OK;
}

// Enqueues the call's launches; *launches_out receives how many.
int enqueue_launches(ykgpu_context* ctx, hipStream_t st, uint32_t s_end, const ykgpu_film* film,
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
    const bool defer = !x128 && !f32 && wa.lens && wa.retry_cap && warm_wave_slots(ctx, wa.n) <= kDeferSlots;
    const uint32_t wblocks = warm_blocks_for(wa.n, (uint64_t)ctx->cus * warm_per_cu(f32), defer ? kWalkIlp : 1u);
    YK_HIP(hipEventRecord(ev[0], ctx->aux));
    if (!x128) {
      if (f32 && wa.lens)
        hipLaunchKernelGGL((yk_mt_warmup<true, true>), dim3(wblocks), dim3(256), 0, ctx->aux, wa);
      else if (f32)
        hipLaunchKernelGGL((yk_mt_warmup<false, true>), dim3(wblocks), dim3(256), 0, ctx->aux, wa);
      else if (defer)
        hipLaunchKernelGGL(yk_mt_warmup_defer, dim3(wblocks), dim3(256), 0, ctx->aux, wa);
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
void call_stats(ykgpu_context* ctx, const yk_render_params* p, const double* sums_dev, const ykgpu_film* film,
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
  if (!rc) rc = enqueue_launches(ctx, st, s_end, film, lp, la, &launches);
  if (!rc) call_stats(ctx, p, sums_dev, film, lp, launches);
  return rc;
}

// Device memory the context holds (yk_render_stats.device_bytes)
uint64_t device_bytes(const ykgpu_context* ctx) {
  uint64_t b = ctx->t64.bytes + ctx->t32.bytes;
  if (ctx->d_geo) b += (uint64_t)ctx->nspheres * (sizeof(SphereGeo) + sizeof(SphereMat) + sizeof(float4));
  b += ctx->warm_cap + ctx->col_cap * sizeof(double) + ctx->acc_cap * sizeof(double);
  b += ctx->retry_cap * sizeof(uint4);
  b += (uint64_t)ctx->order_slots * sizeof(uint32_t) + (uint64_t)ctx->counter_cap * sizeof(uint32_t);
  b += kCounters * sizeof(unsigned long long);
  if (ctx->d_mt) b += 2ull * ctx->scratch_lanes * ykd::kMtN * sizeof(uint32_t);
  if (ctx->d_ids) b += 2ull * ctx->id_lanes * ctx->id_stride * sizeof(uint16_t);
  b += ctx->rgb_cap + ctx->sums_cap * sizeof(double);
  return b;
}

int finish_stats(ykgpu_context* ctx) {
  if (!ctx->stats_pending) return YK_OK;
  YK_HIP(hipEventSynchronize(ctx->ev1));
  float ms = 0;
  YK_HIP(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
  unsigned long long c[kCounters];
  YK_HIP(hipMemcpy(c, ctx->d_stats, sizeof(c), hipMemcpyDeviceToHost));
  ctx->stats.node_visits = c[4];
  ctx->stats.linear_scans = c[5];
  ctx->stats.newton_calls = c[6];
  ctx->stats.newton_iters = c[7];
  for (int k = 0; k < 8; ++k) ctx->stats.phase_cycles[k] = c[8 + k];
  for (int k = 0; k < 3; ++k) ctx->stats.timeline[k] = c[16 + k];
  for (int k = 0; k < 4; ++k) ctx->stats.diag[k] = c[19 + k];
  for (int k = 0; k < 8; ++k) ctx->stats.work[k] = c[24 + k];
  ctx->stats.total_ms = ms;
  double tw = 0, tr = 0, tp = 0, busy = 0;
  for (uint32_t k = 0; k + 5 < ctx->lev_used; k += 6) {
    float a = 0, b = 0, c = 0;
    YK_HIP(hipEventSynchronize(ctx->lev[k + 5]));
    YK_HIP(hipEventElapsedTime(&a, ctx->lev[k], ctx->lev[k + 1]));
    YK_HIP(hipEventElapsedTime(&b, ctx->lev[k + 2], ctx->lev[k + 3]));
    YK_HIP(hipEventElapsedTime(&c, ctx->lev[k + 4], ctx->lev[k + 5]));
    tw += a, tr += b, tp += c;
    // union of the render spans: launch k/6 overlaps only the tail of the one before it
    float ov = 0;
    if (k >= 6) YK_HIP(hipEventElapsedTime(&ov, ctx->lev[k + 2], ctx->lev[k - 6 + 3]));
    busy += b - std::min<double>(b, std::max<double>(0.0, ov));
  }
  ctx->stats.render_busy_ms = busy;
  // the shader clock of each launch (YK_CLOCK_* probe: wave 0 of block 0), averaged over the call
  // weighted by the probe's real time
  const uint32_t nl = ctx->lev_used / 6;
  std::vector<unsigned long long> clk(4ull * nl);
  std::vector<double> mhz(nl, 0.0);
  if (nl) YK_HIP(hipMemcpy(clk.data(), ctx->d_clk, clk.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  double cyc = 0, real = 0;
  for (uint32_t k = 0; k < nl; ++k) {
    const double dc = (double)(clk[4 * k + 2] - clk[4 * k]), dr = (double)(clk[4 * k + 3] - clk[4 * k + 1]);
    if (dr > 0 && clk[4 * k + 3] > clk[4 * k + 1]) {
      mhz[k] = dc / dr * 100.0;  // s_memrealtime ticks at 100 MHz
      cyc += dc;
      real += dr;
    }
  }
  ctx->stats.sclk_mhz = real > 0 ? cyc / real * 100.0 : 0.0;
  if (std::getenv("YKGPU_TIMELINE")) {  // diagnostic: per-launch event times (ms from the call's start)
    // the previous call's launches on the same clock (negative: before this call's start), so the
    // handover between back-to-back calls shows
    for (uint32_t k = 0; k + 5 < ctx->lev_prev_used && k + 5 < ctx->lev_prev.size(); k += 6) {
      float t[6];
      bool ok = true;
      for (int q = 0; q < 6 && ok; ++q) ok = hipEventElapsedTime(&t[q], ctx->ev0, ctx->lev_prev[k + q]) == hipSuccess;
      if (!ok) {
        (void)hipGetLastError();
        break;
      }
      std::fprintf(stderr, "prev   %u: warm %8.3f %8.3f  render %8.3f %8.3f  reduce %8.3f %8.3f\n", k / 6, t[0],
                   t[1], t[2], t[3], t[4], t[5]);
    }
    for (uint32_t k = 0; k + 5 < ctx->lev_used; k += 6) {
      float t[6];
      for (int q = 0; q < 6; ++q) YK_HIP(hipEventElapsedTime(&t[q], ctx->ev0, ctx->lev[k + q]));
      std::fprintf(stderr, "launch %u: warm %8.3f %8.3f  render %8.3f %8.3f  reduce %8.3f %8.3f  sclk %7.1f MHz\n",
                   k / 6, t[0], t[1], t[2], t[3], t[4], t[5], mhz[k / 6]);
    }
    std::fprintf(stderr, "call %8.3f\n", ms);
  }
  ctx->stats.warmup_ms = tw;
  ctx->stats.kernel_ms = tr;
  ctx->stats.resolve_ms = tp;
  ctx->stats.segments = c[0];
  ctx->stats.sphere_tests = c[1];
  ctx->stats.sqrt_calls = c[2];
  ctx->stats.mt_fallbacks = c[3];
  ctx->stats.device_bytes = device_bytes(ctx);
  ctx->stats_pending = false;
  return YK_OK;
}

// Builds one BVH over the scene and uploads it into t: `geo` holds the tuple-order geometry the
// kernel's leaves read (`elem` bytes per sphere), stored in leaf order; kern[v][lds] are the kernel
// instances of workgroup size v (kBlock, kBlockX128) that read the tree from global memory / LDS
// (for the occupancy).
int upload_tree(ykgpu_context* ctx, DevTree& t, const std::vector<double>& centers, const std::vector<double>& radii,
                double cam_ext, const ykbvh::Options& opt, uint32_t leaf_cap, const void* geo, size_t elem,
                size_t tgeo_elem, const RenderKernel (&kern)[2][2], bool exact_stack) {
  const uint32_t count = (uint32_t)radii.size();
  if (opt.max_leaf > leaf_cap) return fail(YK_ERR_UNSUPPORTED, "BVH leaf size above the kernel's leaf capacity");
  const ykbvh::Built bvh = ykbvh::build(centers.data(), radii.data(), count, cam_ext, opt);
  if (bvh.depth > ykbvh::kMaxDepth) return fail(YK_ERR_INVALID, "BVH deeper than the traversal stack");
  std::vector<char> leaf_geo(count * elem);
  for (uint32_t i = 0; i < count; ++i)
    std::memcpy(leaf_geo.data() + i * elem, (const char*)geo + (size_t)bvh.order[i] * elem, elem);
  t.release();
  int32_t root_code = 0;
  uint32_t wdepth = 0;
  const std::vector<DevNode> snodes = ykbvh::wide_nodes(bvh, &root_code, &wdepth);
  // every leaf the kernel can reach must fit its leaf code (kLeafCapF64 / kLeafCapF32)
  auto leaf_fits = [&](int32_t code) { return code >= 0 || (((~(uint32_t)code) & 15u) <= leaf_cap); };
  bool fits = leaf_fits(root_code);
  for (const DevNode& w : snodes)
    for (int k = 0; k < 4; ++k) fits = fits && leaf_fits(w.child[k]);
  if (!fits) return fail(YK_ERR_UNSUPPORTED, "a BVH leaf holds more spheres than the kernel's leaf code tests");
  const size_t nn = std::max<size_t>(1, snodes.size());
  YK_HIP(hipMalloc(&t.nodes, nn * sizeof(DevNode)));
  YK_HIP(hipMalloc(&t.leaf_geo, count * elem));
  YK_HIP(hipMalloc(&t.leaf_ids, count * sizeof(uint32_t)));
  if (!snodes.empty())
    YK_HIP(hipMemcpy(t.nodes, snodes.data(), snodes.size() * sizeof(DevNode), hipMemcpyHostToDevice));
  YK_HIP(hipMemcpy(t.leaf_geo, leaf_geo.data(), count * elem, hipMemcpyHostToDevice));
  YK_HIP(hipMemcpy(t.leaf_ids, bvh.order.data(), count * sizeof(uint32_t), hipMemcpyHostToDevice));
  t.bytes = nn * sizeof(DevNode) + count * elem + count * sizeof(uint32_t);
  t.root = root_code;
  t.depth = bvh.depth;
  t.origin_bound = bvh.origin_bound;
  t.n_nodes = (uint32_t)snodes.size();
  // LDS layout: [nodes][leaf geometry][leaf ids][tuple-order geometry][materials][traversal
  // stacks].  The tables (tgeo_elem bytes of tuple-order geometry per sphere — the FP64 kernel's
  // SphereGeo, the FP32 kernel's float4 — and the SphereMat: candidate roots, shading, unwind) go
  // wherever the tree goes: the LDS instance reads both from LDS.  One
  // plan per workgroup size (the stacks are per lane).
  auto a16 = [](size_t b) { return (b + 15) & ~size_t(15); };
  const size_t scene_bytes = a16(t.n_nodes * sizeof(DevNode)) + a16(count * elem) + a16(count * sizeof(uint32_t));
  const size_t tgeo_bytes = tgeo_elem ? a16(count * tgeo_elem) : 0;
  const size_t mat_bytes = tgeo_elem ? a16(count * sizeof(SphereMat)) : 0;
  t.geo_off = (uint32_t)a16(t.n_nodes * sizeof(DevNode));
  t.ids_off = t.geo_off + (uint32_t)a16(count * elem);
  for (int v = 0; v < 2; ++v) {
    DevTree::Plan& pl = t.plan[v];
    // threads per workgroup = traversal stacks per workgroup
    const int blk = block_of(v == 1);
    const int rays = blk;
    // a CU holds one workgroup of >= 512 threads (768 / blk of smaller ones); 2 KB below the
    // share: the hardware's allocation granularity (3 blocks of 54144 bytes measured only 2
    // resident per CU)
    const size_t budget = (size_t)160 * 1024 / (blk >= 512 ? 1 : 768 / blk) - 2048;
    const size_t min_stacks = (size_t)12 * rays * 4;
    pl.in_lds = scene_bytes + tgeo_bytes + mat_bytes + min_stacks <= budget;
    const size_t tables = pl.in_lds ? tgeo_bytes + mat_bytes : 0;
    // Traversal stack per lane: up to 3 pushes per wide level suffice (3 * wdepth + 1 entries);
    // the capacity is what still fits the budget (at least 8); a lane that would exceed it
    // abandons the traversal for the exact linear scan.  Pushes write unconditionally at the
    // current top (up to 3 past the capacity): +4 entries.
    {
      const size_t used = pl.in_lds ? scene_bytes + tables : 0;
      const uint32_t fit = used + min_stacks <= budget ? (uint32_t)((budget - used) / (rays * 4)) : 12u;
      pl.stack_cap = std::max(8u, std::min(3 * wdepth + 1, fit - 4));
      pl.stack_entries = pl.stack_cap + 4;
      pl.stack_check = true;
      // The FP64 branch-free visit (exact_stack) with 3 * wdepth + 1 entries: a visit at inner
      // level k finds at most 3 entries per ancestor level on the stack (depth-first: what is left
      // of an ancestor's up to 3 pushes; the sentinel is entry 0), so its top is <= 3k + 1 <=
      // 3 * wdepth - 2, its writes (at the top and the next two entries) stay below entry
      // 3 * wdepth and its new top is <= 3 * wdepth + 1: no overflow, no check, no slack
      if (exact_stack && fit >= 3 * wdepth + 1) {
        pl.stack_cap = 3 * wdepth + 1;
        pl.stack_entries = pl.stack_cap;
        pl.stack_check = false;
      }
#ifdef YK_STACK_CAP_FORCE
      // (test builds, tests/test_gpu_robust.py: a checked stack this shallow overflows, and the
      // lanes that overflow take the exact linear scan)
      pl.stack_cap = YK_STACK_CAP_FORCE;
      pl.stack_entries = pl.stack_cap + 4;
      pl.stack_check = true;
#endif
    }
    pl.tgeo_off = pl.in_lds && tgeo_elem ? (uint32_t)scene_bytes : 0u;
    pl.mat_off = pl.in_lds && tgeo_elem ? (uint32_t)(scene_bytes + tgeo_bytes) : 0u;
    pl.stack_off = pl.in_lds ? (uint32_t)(scene_bytes + tables) : 0u;
    pl.lds_bytes = pl.stack_off + pl.stack_entries * rays * (uint32_t)sizeof(int32_t);
    int per_cu = 0;
    const RenderKernel k = kern[v][pl.in_lds ? 1 : 0];
    const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k, blk, pl.lds_bytes);
    if (e != hipSuccess || per_cu < 1) per_cu = 1;
    pl.grid = per_cu * ctx->cus;
  }
  return YK_OK;
}

}  // namespace

extern "C" {

uint32_t ykgpu_abi_version(void) { return YKGPU_ABI_VERSION; }

const char* ykgpu_last_error(void) { return g_last_error.c_str(); }

int ykgpu_device_count(int* count) {
  if (!count) return fail(YK_ERR_INVALID, "null count");
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) {
    *count = 0;
    return fail(YK_ERR_DEVICE, std::string("hipGetDeviceCount: ") + hipGetErrorString(e));
  }
  *count = n;
  return YK_OK;
}

int ykgpu_context_create(int device, ykgpu_context** out) {
  if (!out) return fail(YK_ERR_INVALID, "null out");
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n == 0)
    return fail(YK_ERR_DEVICE, "no HIP device (the renderer has no CPU fallback)");
  if (device < 0 || device >= n) return fail(YK_ERR_INVALID, "device index out of range");
  YK_HIP(hipSetDevice(device));
  hipDeviceProp_t prop;
  YK_HIP(hipGetDeviceProperties(&prop, device));
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(YK_ERR_DEVICE, std::string("built for gfx950, device is ") + prop.gcnArchName);
  auto* ctx = new ykgpu_context();
  ctx->device = device;
  ctx->cus = prop.multiProcessorCount;
  for (int k16 = 0; k16 < 16; ++k16)
    (void)hipFuncSetAttribute((const void*)fp64_kernel(k16 & 8, k16 & 7), hipFuncAttributeMaxDynamicSharedMemorySize,
                              160 * 1024);
  for (int k8 = 0; k8 < 8; ++k8)
    (void)hipFuncSetAttribute((const void*)f32_kernel(k8 & 4, (k8 & 1) | ((k8 & 2) << 1)),
                              hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess ||
      hipStreamCreateWithFlags(&ctx->aux, hipStreamNonBlocking) != hipSuccess ||
      hipStreamCreateWithFlags(&ctx->red, hipStreamNonBlocking) != hipSuccess ||
      create_render_stream(&ctx->alt) != hipSuccess || create_render_stream(&ctx->ren) != hipSuccess ||
      hipEventCreate(&ctx->ev0) != hipSuccess || hipEventCreate(&ctx->ev1) != hipSuccess ||
      hipMalloc(&ctx->d_stats, kCounters * sizeof(unsigned long long)) != hipSuccess) {
    ykgpu_context_destroy(ctx);
    return fail(YK_ERR_DEVICE, "context resources");
  }
  *out = ctx;
  return YK_OK;
}

int ykgpu_context_destroy(ykgpu_context* ctx) {
  if (!ctx) return YK_OK;
  (void)hipSetDevice(ctx->device);
  if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
  (void)hipFree(ctx->d_geo);
  (void)hipFree(ctx->d_mat);
  (void)hipFree(ctx->d_geo_f);
  (void)hipFree(ctx->d_counter);
  (void)hipFree(ctx->d_clk);
  (void)hipFree(ctx->d_stats);
  (void)hipFree(ctx->d_warm);
  (void)hipFree(ctx->d_retry);
  (void)hipFree(ctx->d_order);
  (void)hipFree(ctx->d_col);
  (void)hipFree(ctx->d_acc);
  ctx->t64.release();
  ctx->t32.release();
  (void)hipFree(ctx->d_mt);
  (void)hipFree(ctx->d_ids);
  (void)hipFree(ctx->d_rgb);
  (void)hipFree(ctx->d_sums);
  for (hipEvent_t e : ctx->lev) (void)hipEventDestroy(e);
  for (hipEvent_t e : ctx->lev_prev) (void)hipEventDestroy(e);
  for (hipEvent_t e : ctx->gev) (void)hipEventDestroy(e);
  if (ctx->ev0) (void)hipEventDestroy(ctx->ev0);
  if (ctx->ev1) (void)hipEventDestroy(ctx->ev1);
  if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
  if (ctx->aux) (void)hipStreamDestroy(ctx->aux);
  if (ctx->red) (void)hipStreamDestroy(ctx->red);
  if (ctx->alt) (void)hipStreamDestroy(ctx->alt);
  if (ctx->ren) (void)hipStreamDestroy(ctx->ren);
  delete ctx;
  return YK_OK;
}

int ykgpu_set_scene(ykgpu_context* ctx, const yk_sphere* spheres, uint32_t count,
                    const yk_camera* camera) {
  if (!ctx || !spheres || !camera) return fail(YK_ERR_INVALID, "null argument");
  if (count == 0 || count > 65535) return fail(YK_ERR_INVALID, "sphere count must be 1..65535");
  std::vector<SphereGeo> geo(count);
  std::vector<SphereMat> mat(count);
  std::vector<float4> geo_f(count);
  for (uint32_t i = 0; i < count; ++i) {
    const yk_sphere& s = spheres[i];
    if (s.material > YK_MATERIAL_DIELECTRIC) return fail(YK_ERR_INVALID, "unknown material kind");
    geo[i] = {s.center[0], s.center[1], s.center[2], s.radius * s.radius};
    // sphere<float>: centre and radius rounded to float, radius*radius a float product
    const float rf = (float)s.radius;
    geo_f[i] = make_float4((float)s.center[0], (float)s.center[1], (float)s.center[2], rf * rf);
    mat[i] = {s.albedo[0], s.albedo[1], s.albedo[2], s.fuzz, s.radius, s.ior, s.material, 0.0f, 0.0};  // inv_r*: yk_mat_prep
    if (s.material == YK_MATERIAL_DIELECTRIC) {
      // the FP64 kernel's dielectric reads 1/ior and Schlick's r0 for both sides of the surface
      // from its otherwise unused fields (never unwound: its attenuation is 1), computed here
      // with the operations and order of Schlick's formula as ykf::reflectance writes it (IEEE
      // double, no contraction)
      const double inv = 1.0 / s.ior;
      double r0f = (1 - inv) / (1 + inv), r0b = (1 - s.ior) / (1 + s.ior);
      r0f = r0f * r0f;
      r0b = r0b * r0b;
      mat[i].fuzz = inv;
      mat[i].ar = r0f;
      mat[i].ag = r0b;
    }
  }
  YK_HIP(hipSetDevice(ctx->device));
  // a render enqueued by ykgpu_render_async on the caller's stream (and its launches on the
  // context's own streams) may still read the scene: wait for this context's last call — ev1
  // follows the call's final reduce, which follows every launch of the call (launch()) — and for
  // its own stream (the diagnostic entry points), not for the rest of the device
  YK_HIP(hipEventSynchronize(ctx->ev1));
  YK_HIP(hipStreamSynchronize(ctx->stream));
  // ... and for every stream of the context: a launch() that failed part-way may have queued
  // warm-ups, renders or reduces without recording ev1 (still not the rest of the device)
  for (hipStream_t s : {ctx->aux, ctx->red, ctx->ren, ctx->alt}) YK_HIP(hipStreamSynchronize(s));
  ++ctx->scene_gen;  // from here on the device holds another scene: the context's films are over
  if (count > ctx->nspheres || !ctx->d_geo) {
    (void)hipFree(ctx->d_geo);
    (void)hipFree(ctx->d_mat);
    (void)hipFree(ctx->d_geo_f);
    ctx->d_geo = nullptr;
    ctx->d_mat = nullptr;
    ctx->d_geo_f = nullptr;
    YK_HIP(hipMalloc(&ctx->d_geo, count * sizeof(SphereGeo)));
    YK_HIP(hipMalloc(&ctx->d_mat, count * sizeof(SphereMat)));
    YK_HIP(hipMalloc(&ctx->d_geo_f, count * sizeof(float4)));
  }
  YK_HIP(hipMemcpy(ctx->d_geo, geo.data(), count * sizeof(SphereGeo), hipMemcpyHostToDevice));
  YK_HIP(hipMemcpy(ctx->d_geo_f, geo_f.data(), count * sizeof(float4), hipMemcpyHostToDevice));
  // the BVHs (culling only): the FP64 kernel's and the FP32 kernel's, whose boxes
  // also carry render<float>'s sphere-test error (§4.1)
  std::vector<double> centers(3 * size_t(count)), radii(count);
  double rmin = INFINITY;
  for (uint32_t i = 0; i < count; ++i) {
    for (int k = 0; k < 3; ++k) centers[3 * i + k] = spheres[i].center[k];
    radii[i] = spheres[i].radius;
    rmin = std::min(rmin, std::fabs(radii[i]));
  }
  double cam_ext = 0;
  for (int k = 0; k < 3; ++k) cam_ext = std::max(cam_ext, std::fabs(camera->origin[k]));
  // one sphere per leaf for the 4-wide FP64 tree: 64-spp A/B on the final scene 32.5 -> 31.7 ms
  // against two (three: 33.4); the FP32 tree keeps two (one or three: neutral)
  ykbvh::Options bopt;
  bopt.max_leaf = kLeafCapF64;  // the FP64 kernel tests one sphere per leaf, without a loop
  if (const char* e = ab_knob("YKGPU_BVH_BINS")) bopt.bins = std::max(2, std::min(256, std::atoi(e)));  // (A/B)
  // SAH over all three axes: 512-spp A/B 199.4 -> 198.3 ms (model: 5.51 -> 5.13 visits per segment)
  bopt.all_axes = true;
  if (const char* e = ab_knob("YKGPU_BVH_ALLAXES")) bopt.all_axes = std::atoi(e) != 0;                  // (A/B)
  const RenderKernel k64[2][2] = {{fp64_kernel(false, 0), fp64_kernel(true, 0)},
                                  {fp64_kernel(false, 4), fp64_kernel(true, 4)}};
  int rc = upload_tree(ctx, ctx->t64, centers, radii, cam_ext, bopt, kLeafCapF64, geo.data(), sizeof(SphereGeo),
                       sizeof(SphereGeo), k64, true);
  if (rc) return rc;
  ykbvh::Options fopt = bopt;
  fopt.max_leaf = kLeafCapF32;  // the FP32 kernel's leaf loop is unrolled for two spheres
  if (const char* e = ab_knob("YKGPU_BVH_ALLAXES_F32")) fopt.all_axes = std::atoi(e) != 0;  // (A/B; on: neutral)
  fopt.radius_grow = 2.0 * (double)ykbvh::kF32Cone;
  fopt.f32_big = ab_knob("YKGPU_F32_NO_BIG") == nullptr;  // (A/B: the cone bound alone)
  const RenderKernel k32[2][2] = {{f32_kernel(false, 0), f32_kernel(true, 0)},
                                  {f32_kernel(false, 4), f32_kernel(true, 4)}};
  rc = upload_tree(ctx, ctx->t32, centers, radii, cam_ext, fopt, kLeafCapF32, geo_f.data(), sizeof(float4),
                   sizeof(float4), k32, false);
  if (rc) return rc;
  // the float bound assumes neither underflow nor overflow: a scene outside that
  // scale renders FP32 with the linear scan throughout
  if (!(rmin >= 0x1p-20) || !(ctx->t32.origin_bound <= 0x1p20)) ctx->t32.origin_bound = -1.0;
  YK_HIP(hipMemcpy(ctx->d_mat, mat.data(), count * sizeof(SphereMat), hipMemcpyHostToDevice));
  hipLaunchKernelGGL(yk_mat_prep, dim3((count + 255) / 256), dim3(256), 0, ctx->stream, ctx->d_mat, count);
  YK_HIP(hipGetLastError());
  YK_HIP(hipStreamSynchronize(ctx->stream));
  ctx->nspheres = count;
  ctx->cam = *camera;
  ctx->have_scene = true;
  return YK_OK;
}

int ykgpu_render_async(ykgpu_context* ctx, const yk_render_params* p, void* rgb_device,
                       void* stream) {
  int rc = check_params(ctx, p);
  if (rc) return rc;
  if (!rgb_device) return fail(YK_ERR_INVALID, "null output");
  YK_HIP(hipSetDevice(ctx->device));
  hipStream_t st = stream ? (hipStream_t)stream : ctx->stream;
  ctx->t0 = std::chrono::steady_clock::now();
  return launch(ctx, p, (uint8_t*)rgb_device, nullptr, st, 0, p->samples_per_pixel, nullptr);
}

static int render_host(ykgpu_context* ctx, const yk_render_params* p, uint8_t* rgb_host,
                       double* sums_host) {
  int rc = check_params(ctx, p);
  if (rc) return rc;
  YK_HIP(hipSetDevice(ctx->device));
  const auto t0 = std::chrono::steady_clock::now();
  const size_t npix = (size_t)p->row_count * tile_width(p);
  if (npix * 3 > ctx->rgb_cap) {
    (void)hipFree(ctx->d_rgb);
    ctx->d_rgb = nullptr;
    YK_HIP(hipMalloc(&ctx->d_rgb, npix * 3));
    ctx->rgb_cap = npix * 3;
  }
  if (sums_host && npix * 3 > ctx->sums_cap) {
    (void)hipFree(ctx->d_sums);
    ctx->d_sums = nullptr;
    YK_HIP(hipMalloc(&ctx->d_sums, npix * 3 * sizeof(double)));
    ctx->sums_cap = npix * 3;
  }
  rc = launch(ctx, p, ctx->d_rgb, sums_host ? ctx->d_sums : nullptr, ctx->stream, 0, p->samples_per_pixel, nullptr);
  if (rc) return rc;
  if (rgb_host) YK_HIP(hipMemcpyAsync(rgb_host, ctx->d_rgb, npix * 3, hipMemcpyDeviceToHost, ctx->stream));
  if (sums_host)
    YK_HIP(hipMemcpyAsync(sums_host, ctx->d_sums, npix * 3 * sizeof(double), hipMemcpyDeviceToHost,
                          ctx->stream));
  YK_HIP(hipStreamSynchronize(ctx->stream));
  rc = finish_stats(ctx);
  ctx->stats.total_ms =
      std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return rc;
}

int ykgpu_render(ykgpu_context* ctx, const yk_render_params* p, uint8_t* rgb_host) {
  if (!rgb_host) return fail(YK_ERR_INVALID, "null output");
  return render_host(ctx, p, rgb_host, nullptr);
}

int ykgpu_render_trace(ykgpu_context* ctx, const yk_render_params* p, uint32_t max_rays, double* rays_host,
                       uint32_t* counts_host) {
  int rc = check_params(ctx, p);
  if (rc) return rc;
  if (!max_rays || !rays_host || !counts_host) return fail(YK_ERR_INVALID, "null output or max_rays == 0");
  const size_t n = (size_t)p->row_count * tile_width(p) * p->samples_per_pixel;
  YK_HIP(hipSetDevice(ctx->device));
  YK_HIP(hipMalloc(&ctx->d_trace, n * max_rays * 6 * sizeof(double)));
  if (hipMalloc(&ctx->d_trace_counts, n * sizeof(uint32_t)) != hipSuccess) {
    (void)hipFree(ctx->d_trace);
    ctx->d_trace = nullptr;
    return fail(YK_ERR_NOMEM, "ykgpu_render_trace: ray counts");
  }
  ctx->trace_cap = max_rays;
  yk_render_params q = *p;
  q.flags |= YK_FLAG_COUNT_WORK | YK_FLAG_TRACE_RAYS;
  rc = render_host(ctx, &q, nullptr, nullptr);
  hipError_t e = hipSuccess;
  if (!rc) e = hipMemcpy(rays_host, ctx->d_trace, n * max_rays * 6 * sizeof(double), hipMemcpyDeviceToHost);
  if (!rc && e == hipSuccess) e = hipMemcpy(counts_host, ctx->d_trace_counts, n * sizeof(uint32_t), hipMemcpyDeviceToHost);
  (void)hipFree(ctx->d_trace);
  (void)hipFree(ctx->d_trace_counts);
  ctx->d_trace = nullptr;
  ctx->d_trace_counts = nullptr;
  ctx->trace_cap = 0;
  if (rc) return rc;
  if (e != hipSuccess) return fail(YK_ERR_DEVICE, std::string("ykgpu_render_trace: ") + hipGetErrorString(e));
  return YK_OK;
}

int ykgpu_render_sums(ykgpu_context* ctx, const yk_render_params* p, double* sums_host) {
  if (!sums_host) return fail(YK_ERR_INVALID, "null output");
  return render_host(ctx, p, nullptr, sums_host);
}

int ykgpu_math_sqrt(ykgpu_context* ctx, const double* in, double* out, uint64_t n) {
  if (!ctx || (n && (!in || !out))) return fail(YK_ERR_INVALID, "null argument");
  if (n == 0) return YK_OK;
  YK_HIP(hipSetDevice(ctx->device));
  double* d = nullptr;
  YK_HIP(hipMalloc(&d, 2 * n * sizeof(double)));
  hipError_t e = hipMemcpy(d, in, n * sizeof(double), hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    const uint64_t blocks = (n + 255) / 256;
    hipLaunchKernelGGL(yk_math_sqrt, dim3((uint32_t)blocks), dim3(256), 0, ctx->stream, d, d + n, n);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e == hipSuccess) e = hipMemcpy(out, d + n, n * sizeof(double), hipMemcpyDeviceToHost);
  (void)hipFree(d);
  if (e != hipSuccess) return fail(YK_ERR_DEVICE, std::string("ykgpu_math_sqrt: ") + hipGetErrorString(e));
  return YK_OK;
}

int ykgpu_math_sqrt_f32(ykgpu_context* ctx, const float* in, float* out, uint64_t n) {
  if (!ctx || (n && (!in || !out))) return fail(YK_ERR_INVALID, "null argument");
  if (n == 0) return YK_OK;
  YK_HIP(hipSetDevice(ctx->device));
  float* d = nullptr;
  YK_HIP(hipMalloc(&d, 2 * n * sizeof(float)));
  hipError_t e = hipMemcpy(d, in, n * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    const uint64_t blocks = (n + 255) / 256;
    hipLaunchKernelGGL(yk_math_sqrt_f32, dim3((uint32_t)blocks), dim3(256), 0, ctx->stream, d, d + n, n);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e == hipSuccess) e = hipMemcpy(out, d + n, n * sizeof(float), hipMemcpyDeviceToHost);
  (void)hipFree(d);
  if (e != hipSuccess) return fail(YK_ERR_DEVICE, std::string("ykgpu_math_sqrt_f32: ") + hipGetErrorString(e));
  return YK_OK;
}

int ykgpu_math_div(ykgpu_context* ctx, const double* num3, const double* den, double* out3, uint64_t n) {
  if (!ctx || (n && (!num3 || !den || !out3))) return fail(YK_ERR_INVALID, "null argument");
  if (n == 0) return YK_OK;
  YK_HIP(hipSetDevice(ctx->device));
  double* d = nullptr;
  YK_HIP(hipMalloc(&d, 7 * n * sizeof(double)));
  hipError_t e = hipMemcpy(d, num3, 3 * n * sizeof(double), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d + 3 * n, den, n * sizeof(double), hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    const uint64_t blocks = (n + 255) / 256;
    hipLaunchKernelGGL(yk_math_div, dim3((uint32_t)blocks), dim3(256), 0, ctx->stream, d, d + 3 * n, d + 4 * n, n);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e == hipSuccess) e = hipMemcpy(out3, d + 4 * n, 3 * n * sizeof(double), hipMemcpyDeviceToHost);
  (void)hipFree(d);
  if (e != hipSuccess) return fail(YK_ERR_DEVICE, std::string("ykgpu_math_div: ") + hipGetErrorString(e));
  return YK_OK;
}

int ykgpu_math_div_f32(ykgpu_context* ctx, const float* num3, const float* den, float* out3, uint64_t n) {
  if (!ctx || (n && (!num3 || !den || !out3))) return fail(YK_ERR_INVALID, "null argument");
  if (n == 0) return YK_OK;
  YK_HIP(hipSetDevice(ctx->device));
  float* d = nullptr;
  YK_HIP(hipMalloc(&d, 7 * n * sizeof(float)));
  hipError_t e = hipMemcpy(d, num3, 3 * n * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d + 3 * n, den, n * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    const uint64_t blocks = (n + 255) / 256;
    hipLaunchKernelGGL(yk_math_div_f32, dim3((uint32_t)blocks), dim3(256), 0, ctx->stream, d, d + 3 * n, d + 4 * n, n);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e == hipSuccess) e = hipMemcpy(out3, d + 4 * n, 3 * n * sizeof(float), hipMemcpyDeviceToHost);
  (void)hipFree(d);
  if (e != hipSuccess) return fail(YK_ERR_DEVICE, std::string("ykgpu_math_div_f32: ") + hipGetErrorString(e));
  return YK_OK;
}

int ykgpu_get_stats(ykgpu_context* ctx, yk_render_stats* out) {
  if (!ctx || !out) return fail(YK_ERR_INVALID, "null argument");
  YK_HIP(hipSetDevice(ctx->device));
  int rc = finish_stats(ctx);
  if (rc) return rc;
  *out = ctx->stats;
  return YK_OK;
}

// ---- progressive film (include/ykgpu.h "progressive film") ------------------------------------
namespace {
int film_ready(const ykgpu_film* film) {
  if (!film) return fail(YK_ERR_INVALID, "null film");
  if (film->torn) return fail(YK_ERR_INVALID, "the film's last accumulate failed part-way: restore it with ykgpu_film_write");
  return YK_OK;
}
uint32_t film_blocks(const ykgpu_film* film) { return std::max(1u, std::min((film->nps + 255) / 256, (uint32_t)film->ctx->cus * 8)); }
}  // namespace

int ykgpu_film_create(ykgpu_context* ctx, const yk_render_params* params, ykgpu_film** out) {
  if (!out) return fail(YK_ERR_INVALID, "null out");
  *out = nullptr;
  if (!ctx || !params) return fail(YK_ERR_INVALID, "null context or params");
  yk_render_params p = *params;
  p.flags &= YK_FLAG_LINEAR_SCAN;  // the diagnostic flags (counting, one lane, tracing) are not a film's
  int rc = check_params(ctx, &p);
  if (rc) return rc;
  if (p.seed_mode == YK_SEED_RANDOM_DEVICE) {
    // the key of every chunk: the caller's, or one from std::random_device now (source.cpp:159)
    std::random_device rd;
    while (!p.seed_key) p.seed_key = ((uint64_t)rd() << 32) | rd();
  }
  YK_HIP(hipSetDevice(ctx->device));
  auto* film = new ykgpu_film();
  film->ctx = ctx;
  film->device = ctx->device;
  film->p = p;
  film->scene_gen = ctx->scene_gen;
  film->npix = (uint64_t)p.row_count * tile_width(&p);
  film->order = build_order(tile_width(&p), p.row_count, order_stride(&p), order_mode());
  film->nps = (uint32_t)film->order.size();
  const size_t plane_bytes = (size_t)film->nps * 6 * sizeof(double);
  hipError_t e = hipMalloc(&film->d_plane, plane_bytes);
  if (e == hipSuccess) e = hipMalloc(&film->d_order, film->nps * sizeof(uint32_t));
  if (e == hipSuccess) e = hipMalloc(&film->d_result, 2 * sizeof(unsigned long long));
  if (e == hipSuccess) e = hipMalloc(&film->d_count, film->nps * sizeof(uint32_t));
  const bool nomem = e == hipErrorOutOfMemory;
  if (e == hipSuccess) e = hipMemset(film->d_count, 0, film->nps * sizeof(uint32_t));
  if (e == hipSuccess) e = hipMemcpy(film->d_order, film->order.data(), film->nps * sizeof(uint32_t), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(film->d_plane, 0, plane_bytes);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    ykgpu_film_destroy(film);
    return fail(nomem ? YK_ERR_NOMEM : YK_ERR_DEVICE, std::string("ykgpu_film_create: ") + hipGetErrorString(e));
  }
  film->hist[0] = film->npix;
  *out = film;
  return YK_OK;
}

int ykgpu_film_destroy(ykgpu_film* film) {
  if (!film) return YK_OK;
  (void)hipSetDevice(film->device);
  (void)hipFree(film->d_plane);
  (void)hipFree(film->d_order);
  (void)hipFree(film->d_result);
  for (void* q : {(void*)film->d_count, (void*)film->d_take, (void*)film->d_blocks, (void*)film->d_gorder,
                  (void*)film->d_gmap, (void*)film->d_hist, film->d_denoise, film->d_features})
    (void)hipFree(q);
  delete film;
  return YK_OK;
}

int ykgpu_film_params(const ykgpu_film* film, yk_render_params* out) {
  if (!film || !out) return fail(YK_ERR_INVALID, "null argument");
  *out = film->p;
  return YK_OK;
}

int ykgpu_film_accumulate(ykgpu_film* film, uint32_t n_samples) {
  int rc = film_ready(film);
  if (rc) return rc;
  ykgpu_context* ctx = film->ctx;
  if (film->scene_gen != ctx->scene_gen)
    return fail(YK_ERR_INVALID, "the context's scene was set after the film was created");
  if (!film->uniform())
    return fail(YK_ERR_INVALID, "the film's pixels hold different sample counts: use ykgpu_film_accumulate_adaptive");
  if (n_samples == 0) return fail(YK_ERR_INVALID, "n_samples must be > 0");
  if (n_samples > film->p.samples_per_pixel - film->done)
    return fail(YK_ERR_INVALID, "the chunk passes the film's target (samples_per_pixel)");
  YK_HIP(hipSetDevice(ctx->device));
  const auto t0 = std::chrono::steady_clock::now();
  film->torn = true;  // (until the chunk is whole)
  rc = launch(ctx, &film->p, nullptr, nullptr, ctx->stream, film->done, film->done + n_samples, film);
  if (rc) return rc;
  YK_HIP(hipStreamSynchronize(ctx->stream));
  rc = finish_stats(ctx);
  if (rc) return rc;
  ctx->stats.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  film->done += n_samples;
  film->hist.clear();
  film->hist[film->done] = film->npix;
  film->torn = false;
  return YK_OK;
}

int ykgpu_film_resolve(ykgpu_film* film, uint8_t* rgb_host) {
  int rc = film_ready(film);
  if (rc) return rc;
  if (!rgb_host) return fail(YK_ERR_INVALID, "null output");
  if (film->uniform() && film->done < 1) return fail(YK_ERR_INVALID, "resolve needs at least one accumulated sample");
  ykgpu_context* ctx = film->ctx;
  YK_HIP(hipSetDevice(ctx->device));
  uint8_t* d_rgb = nullptr;
  YK_HIP(hipMalloc(&d_rgb, film->npix * 3));
  hipLaunchKernelGGL(yk_film_resolve, dim3(film_blocks(film)), dim3(256), 0, ctx->stream, film->d_plane, film->d_order,
                     d_rgb, film->nps, film->done, film->uniform() ? nullptr : film->d_count);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(rgb_host, d_rgb, film->npix * 3, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  (void)hipFree(d_rgb);
  if (e != hipSuccess) return fail(YK_ERR_DEVICE, std::string("ykgpu_film_resolve: ") + hipGetErrorString(e));
  return YK_OK;
}

int ykgpu_film_read(ykgpu_film* film, double* sums, double* sumsq, uint32_t* done) {
  int rc = film_ready(film);
  if (rc) return rc;
  if (done) *done = film->done;
  if (!sums && !sumsq) return YK_OK;
  YK_HIP(hipSetDevice(film->device));
  // the planes are in slot order: copied whole, and permuted to pixel order here
  const size_t nps = film->nps;
  std::vector<double> host(nps * 6);
  YK_HIP(hipMemcpy(host.data(), film->d_plane, host.size() * sizeof(double), hipMemcpyDeviceToHost));
  for (size_t p = 0; p < nps; ++p) {
    const uint32_t px = film->order[p];
    if (px == kNoPixel) continue;
    for (int c = 0; c < 3; ++c) {
      if (sums) sums[(size_t)px * 3 + c] = host[c * nps + p];
      if (sumsq) sumsq[(size_t)px * 3 + c] = host[(3 + c) * nps + p];
    }
  }
  return YK_OK;
}

int ykgpu_film_write(ykgpu_film* film, const double* sums, const double* sumsq, uint32_t done) {
  if (!film || !sums || !sumsq) return fail(YK_ERR_INVALID, "null argument");
  if (done > film->p.samples_per_pixel) return fail(YK_ERR_INVALID, "done passes the film's target (samples_per_pixel)");
  YK_HIP(hipSetDevice(film->device));
  const size_t nps = film->nps;
  std::vector<double> host(nps * 6, 0.0);
  for (size_t p = 0; p < nps; ++p) {
    const uint32_t px = film->order[p];
    if (px == kNoPixel) continue;
    for (int c = 0; c < 3; ++c) {
      host[c * nps + p] = sums[(size_t)px * 3 + c];
      host[(3 + c) * nps + p] = sumsq[(size_t)px * 3 + c];
    }
  }
  YK_HIP(hipMemcpy(film->d_plane, host.data(), host.size() * sizeof(double), hipMemcpyHostToDevice));
  film->done = done;
  film->hist.clear();
  film->hist[done] = film->npix;
  film->torn = false;
  return YK_OK;
}

int ykgpu_film_error(ykgpu_film* film, double threshold2, double* e2_host, yk_film_stats* stats) {
  int rc = film_ready(film);
  if (rc) return rc;
  if (film->uniform() && film->done < 2) return fail(YK_ERR_INVALID, "the error map needs at least two accumulated samples");
  ykgpu_context* ctx = film->ctx;
  YK_HIP(hipSetDevice(ctx->device));
  double* d_e2 = nullptr;
  if (e2_host) YK_HIP(hipMalloc(&d_e2, film->npix * sizeof(double)));
  unsigned long long res[2] = {0, 0};
  hipError_t e = hipMemsetAsync(film->d_result, 0, sizeof res, ctx->stream);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(yk_film_error, dim3(film_blocks(film)), dim3(256), 0, ctx->stream, film->d_plane, film->d_order,
                       d_e2, film->d_result, film->nps, film->done, threshold2, film->uniform() ? nullptr : film->d_count);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(res, film->d_result, sizeof res, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess && e2_host)
    e = hipMemcpyAsync(e2_host, d_e2, film->npix * sizeof(double), hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  (void)hipFree(d_e2);
  if (e != hipSuccess) return fail(YK_ERR_DEVICE, std::string("ykgpu_film_error: ") + hipGetErrorString(e));
  if (stats) {
    stats->pixels = film->npix;
    stats->pixels_over = res[0];
    std::memcpy(&stats->max_e2, &res[1], sizeof(double));
    stats->samples_done = film->done;
    stats->samples_target = film->p.samples_per_pixel;
  }
  return YK_OK;
}

// ---- adaptive passes (include/ykgpu.h "adaptive passes") ---------------------------------------
namespace {
uint32_t film_group_cap(const ykgpu_film* film) { return (film->nps + 63u) & ~63u; }
// the pass's scratch, 12 B per slot, allocated at the film's first adaptive pass
int film_pass_buffers(ykgpu_film* film) {
  const size_t cap = film_group_cap(film);
  if (!film->d_take) YK_HIP(hipMalloc(&film->d_take, film->nps * sizeof(uint32_t)));
  if (!film->d_blocks) YK_HIP(hipMalloc(&film->d_blocks, ((film->nps + 255) / 256) * sizeof(uint32_t)));
  if (!film->d_gorder) YK_HIP(hipMalloc(&film->d_gorder, cap * sizeof(uint32_t)));
  if (!film->d_gmap) YK_HIP(hipMalloc(&film->d_gmap, cap * sizeof(uint32_t)));
  if (!film->d_hist) YK_HIP(hipMalloc(&film->d_hist, kFilmVals * sizeof(unsigned long long)));
  return YK_OK;
}
// a pass's stats: the groups' calls summed (times, work, launches), the largest of what is a size
void add_stats(yk_render_stats& a, const yk_render_stats& b) {
  a.kernel_ms += b.kernel_ms;
  a.resolve_ms += b.resolve_ms;
  a.warmup_ms += b.warmup_ms;
  a.render_busy_ms += b.render_busy_ms;
  a.samples += b.samples;
  a.segments += b.segments;
  a.sphere_tests += b.sphere_tests;
  a.sqrt_calls += b.sqrt_calls;
  a.mt_fallbacks += b.mt_fallbacks;
  a.node_visits += b.node_visits;
  a.linear_scans += b.linear_scans;
  a.newton_calls += b.newton_calls;
  a.newton_iters += b.newton_iters;
  for (int k = 0; k < 8; ++k) a.work[k] += b.work[k];
  a.launches += b.launches;
  a.mem_shrinks += b.mem_shrinks;
  a.grid_blocks = b.grid_blocks;
  a.seed_key = b.seed_key;
  a.sclk_mhz = b.sclk_mhz;
  a.device_bytes = b.device_bytes;
  a.call_bytes = std::max(a.call_bytes, b.call_bytes);
  a.launch_spp = std::max(a.launch_spp, b.launch_spp);
}
}  // namespace

int ykgpu_film_accumulate_adaptive(ykgpu_film* film, double threshold2, uint32_t n_samples, yk_film_pass* out) {
  int rc = film_ready(film);
  if (rc) return rc;
  ykgpu_context* ctx = film->ctx;
  if (film->scene_gen != ctx->scene_gen)
    return fail(YK_ERR_INVALID, "the context's scene was set after the film was created");
  if (n_samples == 0) return fail(YK_ERR_INVALID, "n_samples must be > 0");
  YK_HIP(hipSetDevice(ctx->device));
  const auto t0 = std::chrono::steady_clock::now();
  const uint32_t target = film->p.samples_per_pixel;
  yk_film_pass pass{};
  // the candidate groups: the count values below the target, ascending
  std::vector<uint32_t> vals;
  for (const auto& h : film->hist)
    if (h.first < target && h.second) vals.push_back(h.first);
  std::vector<unsigned long long> nsel(vals.size(), 0);
  if (!vals.empty()) {
    if ((rc = film_pass_buffers(film))) return rc;
    // (a uniform film's counts live in `done`)
    if (film->uniform()) {
      hipLaunchKernelGGL(yk_film_fill_counts, dim3(film_blocks(film)), dim3(256), 0, ctx->stream, film->d_count, film->nps,
                         film->done);
      YK_HIP(hipGetLastError());
    }
    FilmSelectArgs sa{};
    sa.plane = film->d_plane;
    sa.order = film->d_order;
    sa.count = film->d_count;
    sa.take = film->d_take;
    sa.hist = film->d_hist;
    sa.npix_slots = film->nps;
    sa.target = target;
    sa.n_samples = n_samples;
    sa.threshold2 = threshold2;
    for (size_t v0 = 0; v0 < vals.size(); v0 += kFilmVals) {
      sa.nvals = (uint32_t)std::min<size_t>(kFilmVals, vals.size() - v0);
      sa.first = v0 == 0;
      for (uint32_t k = 0; k < sa.nvals; ++k) sa.vals[k] = vals[v0 + k];
      YK_HIP(hipMemsetAsync(film->d_hist, 0, kFilmVals * sizeof(unsigned long long), ctx->stream));
      hipLaunchKernelGGL(yk_film_select, dim3(film_blocks(film)), dim3(256), 0, ctx->stream, sa);
      YK_HIP(hipGetLastError());
      YK_HIP(hipMemcpyAsync(nsel.data() + v0, film->d_hist, sa.nvals * sizeof(unsigned long long), hipMemcpyDeviceToHost,
                            ctx->stream));
      YK_HIP(hipStreamSynchronize(ctx->stream));
    }
  }
  yk_render_stats sum{};
  const uint32_t nblk = (film->nps + 255) / 256;
  std::map<uint32_t, uint64_t> hist = film->hist;
  for (size_t v = 0; v < vals.size(); ++v) {
    if (!nsel[v]) continue;
    if (nsel[v] > film->hist[vals[v]]) return fail(YK_ERR_DEVICE, "ykgpu_film_accumulate_adaptive: a group larger than its count's pixels");
    const uint32_t n = vals[v], take = std::min(n_samples, target - n);
    const uint32_t g_slots = ((uint32_t)nsel[v] + 63u) & ~63u;
    // the group's order and map: padding first, then the members in ascending film-slot order
    YK_HIP(hipMemsetAsync(film->d_gorder, 0xff, g_slots * sizeof(uint32_t), ctx->stream));
    YK_HIP(hipMemsetAsync(film->d_gmap, 0xff, g_slots * sizeof(uint32_t), ctx->stream));
    hipLaunchKernelGGL(yk_film_group_count, dim3(nblk), dim3(256), 0, ctx->stream, film->d_count, film->d_take,
                       film->d_blocks, film->nps, n);
    hipLaunchKernelGGL(yk_film_group_scan, dim3(1), dim3(256), 0, ctx->stream, film->d_blocks, nblk);
    hipLaunchKernelGGL(yk_film_group_write, dim3(nblk), dim3(256), 0, ctx->stream, film->d_count, film->d_take,
                       film->d_order, film->d_blocks, film->d_gorder, film->d_gmap, film->nps, n, g_slots);
    YK_HIP(hipGetLastError());
    // (the warm-ups of a call that overlaps the one before it do not wait for the caller's stream)
    YK_HIP(hipStreamSynchronize(ctx->stream));
    film->torn = true;  // (until the pass is whole)
    film->g_slots = g_slots;
    rc = launch(ctx, &film->p, nullptr, nullptr, ctx->stream, n, n + take, film);
    film->g_slots = 0;
    if (rc) return rc;
    // (the next group reuses the order and map buffers)
    YK_HIP(hipStreamSynchronize(ctx->stream));
    if ((rc = finish_stats(ctx))) return rc;
    ctx->stats.samples = nsel[v] * take;
    add_stats(sum, ctx->stats);
    hist[n] -= nsel[v];
    if (!hist[n]) hist.erase(n);
    hist[n + take] += nsel[v];
    pass.pixels_selected += nsel[v];
    pass.samples_added += nsel[v] * take;
    ++pass.groups;
  }
  film->hist = hist;
  film->done = hist.begin()->first;
  film->torn = false;
  pass.launches = sum.launches;
  pass.min_count = hist.begin()->first;
  pass.max_count = hist.rbegin()->first;
  sum.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (!pass.groups) sum.device_bytes = device_bytes(ctx);
  ctx->stats = sum;
  ctx->stats_pending = false;
  if (out) *out = pass;
  return YK_OK;
}

int ykgpu_film_counts(ykgpu_film* film, uint32_t* counts_host, uint32_t* min_count, uint32_t* max_count) {
  int rc = film_ready(film);
  if (rc) return rc;
  if (min_count) *min_count = film->hist.begin()->first;
  if (max_count) *max_count = film->hist.rbegin()->first;
  if (!counts_host) return YK_OK;
  if (film->uniform()) {
    std::fill(counts_host, counts_host + film->npix, film->done);
    return YK_OK;
  }
  YK_HIP(hipSetDevice(film->device));
  std::vector<uint32_t> host(film->nps);
  YK_HIP(hipMemcpy(host.data(), film->d_count, host.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
  for (size_t p = 0; p < host.size(); ++p)
    if (film->order[p] != kNoPixel) counts_host[film->order[p]] = host[p];
  return YK_OK;
}

int ykgpu_film_write_counts(ykgpu_film* film, const double* sums, const double* sumsq, const uint32_t* counts) {
  if (!film || !sums || !sumsq || !counts) return fail(YK_ERR_INVALID, "null argument");
  std::map<uint32_t, uint64_t> hist;
  for (uint64_t i = 0; i < film->npix; ++i) {
    if (counts[i] > film->p.samples_per_pixel) return fail(YK_ERR_INVALID, "a count passes the film's target (samples_per_pixel)");
    ++hist[counts[i]];
  }
  std::vector<uint32_t> host(film->nps, 0u);
  for (size_t p = 0; p < host.size(); ++p)
    if (film->order[p] != kNoPixel) host[p] = counts[film->order[p]];
  int rc = ykgpu_film_write(film, sums, sumsq, hist.begin()->first);
  if (rc) return rc;
  film->torn = true;  // (until the counts are in)
  YK_HIP(hipMemcpy(film->d_count, host.data(), host.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
  film->hist = hist;
  film->torn = false;
  return YK_OK;
}

// ---- several devices in one process (include/ykgpu.h "several devices") ----------------------
// One context per entry; rows dealt cyclically over the entries (tile row t of the call's row set
// → entry t mod k, uecraytracing_amd/tiles.py's dealing); every entry renders its tile into a
// device buffer on its own streams, and the tile is copied from its device straight into its rows
// of the caller's host image by one strided 2-D copy: the image ends on the host anyway (stb
// writes it), so a device-side gather first would only add a hop.
int ykgpu_group_create(const int* devices, uint32_t n_devices, ykgpu_group** out) {
  if (!out) return fail(YK_ERR_INVALID, "null out");
  *out = nullptr;
  if (!devices || n_devices == 0) return fail(YK_ERR_INVALID, "empty device list");
  if (n_devices > 64) return fail(YK_ERR_INVALID, "at most 64 entries per group");
  auto* g = new ykgpu_group();
  for (uint32_t k = 0; k < n_devices; ++k) {
    ykgpu_context* c = nullptr;
    const int rc = ykgpu_context_create(devices[k], &c);
    if (rc) {
      const std::string msg = g_last_error;
      ykgpu_group_destroy(g);
      return fail(rc, "group entry " + std::to_string(k) + " (device " + std::to_string(devices[k]) + "): " + msg);
    }
    g->ctx.push_back(c);
  }
  g->tile.assign(n_devices, nullptr);
  g->tile_cap.assign(n_devices, 0);
  g->st.assign(n_devices, yk_render_stats{});
  *out = g;
  return YK_OK;
}

int ykgpu_group_destroy(ykgpu_group* g) {
  if (!g) return YK_OK;
  for (size_t k = 0; k < g->ctx.size(); ++k) {
    if (k < g->tile.size() && g->tile[k]) {
      (void)hipSetDevice(g->ctx[k]->device);
      (void)hipStreamSynchronize(g->ctx[k]->stream);
      (void)hipFree(g->tile[k]);
    }
    ykgpu_context_destroy(g->ctx[k]);
  }
  delete g;
  return YK_OK;
}

int ykgpu_group_size(const ykgpu_group* g, uint32_t* n) {
  if (!g || !n) return fail(YK_ERR_INVALID, "null argument");
  *n = (uint32_t)g->ctx.size();
  return YK_OK;
}

int ykgpu_group_set_scene(ykgpu_group* g, const yk_sphere* spheres, uint32_t count, const yk_camera* camera) {
  if (!g) return fail(YK_ERR_INVALID, "null group");
  for (ykgpu_context* c : g->ctx) {
    const int rc = ykgpu_set_scene(c, spheres, count, camera);
    if (rc) return rc;
  }
  return YK_OK;
}

int ykgpu_group_render(ykgpu_group* g, const yk_render_params* p, uint8_t* rgb_host) {
  if (!g || !p || !rgb_host) return fail(YK_ERR_INVALID, "null argument");
  const uint32_t k = (uint32_t)g->ctx.size();
  int rc = check_params(g->ctx[0], p);
  if (rc) return rc;
  if (k > 1 && p->row_band_log2 != 0)
    return fail(YK_ERR_UNSUPPORTED, "a group deals single rows: row_band_log2 must be 0");
  if (k > 1 && (uint64_t)p->row_stride * k >= (1ull << 32)) return fail(YK_ERR_INVALID, "row_stride * devices overflows");
  const auto t0 = std::chrono::steady_clock::now();
  const size_t row_bytes = (size_t)tile_width(p) * 3;
  std::vector<yk_render_params> sub(k, *p);
  std::vector<uint32_t> rows(k, 0);
  // 1. every entry's tile enqueued on its own device before any copy: the devices run together
  for (uint32_t e = 0; e < k; ++e) {
    rows[e] = p->row_count > e ? (p->row_count - e + k - 1) / k : 0;
    if (!rows[e]) continue;
    sub[e].row_begin = p->row_begin + e * p->row_stride;
    sub[e].row_stride = p->row_stride * k;
    sub[e].row_count = rows[e];
    ykgpu_context* c = g->ctx[e];
    YK_HIP(hipSetDevice(c->device));
    const size_t need = rows[e] * row_bytes;
    if (need > g->tile_cap[e]) {
      (void)hipStreamSynchronize(c->stream);
      (void)hipFree(g->tile[e]);
      g->tile[e] = nullptr;
      g->tile_cap[e] = 0;
      YK_HIP(hipMalloc(&g->tile[e], need));
      g->tile_cap[e] = need;
    }
    if ((rc = ykgpu_render_async(c, &sub[e], g->tile[e], nullptr))) return rc;
  }
  // 2. each tile into rows e, e + k, e + 2k, ... of the caller's image (ordered after its render
  //    on the entry's stream)
  for (uint32_t e = 0; e < k; ++e) {
    if (!rows[e]) continue;
    ykgpu_context* c = g->ctx[e];
    YK_HIP(hipSetDevice(c->device));
    YK_HIP(hipMemcpy2DAsync(rgb_host + e * row_bytes, row_bytes * k, g->tile[e], row_bytes, row_bytes, rows[e],
                            hipMemcpyDeviceToHost, c->stream));
  }
  yk_render_stats tot{};
  for (uint32_t e = 0; e < k; ++e) {
    g->st[e] = yk_render_stats{};
    if (!rows[e]) continue;
    ykgpu_context* c = g->ctx[e];
    YK_HIP(hipSetDevice(c->device));
    YK_HIP(hipStreamSynchronize(c->stream));
    if ((rc = finish_stats(c))) return rc;
    g->st[e] = c->stats;
    const yk_render_stats& s = c->stats;
    tot.samples += s.samples;
    tot.segments += s.segments;
    tot.sphere_tests += s.sphere_tests;
    tot.sqrt_calls += s.sqrt_calls;
    tot.mt_fallbacks += s.mt_fallbacks;
    tot.node_visits += s.node_visits;
    tot.linear_scans += s.linear_scans;
    tot.newton_calls += s.newton_calls;
    tot.newton_iters += s.newton_iters;
    for (int q = 0; q < 8; ++q) tot.work[q] += s.work[q];
    tot.launches += s.launches;
    tot.grid_blocks = std::max(tot.grid_blocks, s.grid_blocks);
    tot.kernel_ms = std::max(tot.kernel_ms, s.kernel_ms);
    tot.render_busy_ms = std::max(tot.render_busy_ms, s.render_busy_ms);
    tot.warmup_ms = std::max(tot.warmup_ms, s.warmup_ms);
    tot.resolve_ms = std::max(tot.resolve_ms, s.resolve_ms);
    tot.seed_key = s.seed_key;
    tot.device_bytes += s.device_bytes + g->tile_cap[e];
    tot.call_bytes += s.call_bytes + rows[e] * row_bytes;
    tot.sclk_mhz = std::max(tot.sclk_mhz, s.sclk_mhz);
    // (ABI 11) the largest launch of any entry, and every entry's memory-pressure shrinks
    tot.launch_spp = std::max(tot.launch_spp, s.launch_spp);
    tot.mem_shrinks += s.mem_shrinks;
  }
  tot.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  g->total = tot;
  return YK_OK;
}

int ykgpu_group_get_stats(ykgpu_group* g, int index, yk_render_stats* out) {
  if (!g || !out) return fail(YK_ERR_INVALID, "null argument");
  if (index == -1) {
    *out = g->total;
    return YK_OK;
  }
  if (index < 0 || (size_t)index >= g->ctx.size()) return fail(YK_ERR_INVALID, "entry index out of range");
  *out = g->st[index];
  return YK_OK;
}

int ykgpu_render_devices(const int* devices, uint32_t n_devices, const yk_sphere* spheres, uint32_t count,
                         const yk_camera* camera, const yk_render_params* p, uint8_t* rgb_host) {
  ykgpu_group* g = nullptr;
  int rc = ykgpu_group_create(devices, n_devices, &g);
  if (!rc) rc = ykgpu_group_set_scene(g, spheres, count, camera);
  if (!rc) rc = ykgpu_group_render(g, p, rgb_host);
  if (g) {
    const std::string msg = g_last_error;
    ykgpu_group_destroy(g);
    g_last_error = msg;
  }
  return rc;
}

}  // extern "C"

// ---- film denoise and features (yk_denoise.hip, yk_features.hip): those units' view of a film, and
// this unit's error slot
int yk_film_fail(int code, const char* msg) { return fail(code, msg); }

int yk_film_view_of(ykgpu_film* film, yk_film_view* out) {
  if (int rc = film_ready(film)) return rc;
  const yk_render_params& p = film->p;
  out->device = film->device;
  out->stream = film->ctx->stream;
  out->plane = film->d_plane;
  out->order = film->d_order;
  out->count = film->uniform() ? nullptr : film->d_count;
  out->nps = film->nps;
  out->done = film->done;
  out->rows = p.row_count;
  out->wt = tile_width(&p);
  // (both maps increase strictly, so the last entry tells whether any step was larger than one)
  out->consecutive = host_row_y(&p, p.row_count - 1) == (uint64_t)p.row_begin + p.row_count - 1 &&
                     host_col_x(&p, out->wt - 1) == (uint64_t)p.col_begin + out->wt - 1;
  out->scratch = &film->d_denoise;
  static_assert(sizeof(SphereGeo) == 4 * sizeof(double) && offsetof(SphereGeo, rr) == 3 * sizeof(double), "yk_film_view::geo");
  static_assert(sizeof(SphereMat) == kYkMatStride && offsetof(SphereMat, ar) == kYkMatAlbedo &&
                    offsetof(SphereMat, ab) == kYkMatAlbedo + 16 && offsetof(SphereMat, radius) == kYkMatRadius &&
                    offsetof(SphereMat, kind) == kYkMatKind, "yk_film_view::mat");
  const ykgpu_context* ctx = film->ctx;
  out->W = p.image_width;
  out->H = p.image_height;
  out->row_begin = p.row_begin;
  out->row_stride = p.row_stride;
  out->row_band = p.row_band_log2;
  out->col_begin = p.col_count ? p.col_begin : 0;
  out->col_stride = p.col_count ? p.col_stride : 1;
  out->col_band = p.col_count ? p.col_band_log2 : 0;
  out->t_min = p.t_min;
  out->stale = film->scene_gen != ctx->scene_gen;
  out->geo = (const double*)ctx->d_geo;
  out->mat = (const unsigned char*)ctx->d_mat;
  out->nspheres = ctx->nspheres;
  out->cam = ctx->cam;
  out->features = &film->d_features;
  out->feature_grid = &film->feature_grid;
  return YK_OK;
}
