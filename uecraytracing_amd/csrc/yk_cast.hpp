// yk_cast.hpp — ray queries (include/ykgpu.h "ray queries"): the reference's
// world.hit(r, t_min, t_max) for batches of arbitrary rays, closest hits and occlusion tests, in
// IEEE double so that numpy restates every record bit for bit (tests/cast_ref.py).
//
// Part of the unit yk_features.hip, which includes this file once at its end: the library's other
// first-hit query, kept in a file of its own (the list of units is fixed, tests/test_build_knobs.py).
// Everything here but the three C-ABI entry points lives in namespace ykcast.  One kernel, yk_cast,
// one ray per lane in 256-thread blocks, a plain launch: it traverses the context's FP64 tree
//  with a checked per-lane stack in LDS, tests leaves with the reference's exact
// arithmetic and keeps the minimum root, ties to the later tuple index — the ordered scan's answer
// whatever the visit order.  Rays the float slab test cannot serve take the ordered scan itself.
#ifndef YK_CAST_HPP
#define YK_CAST_HPP

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <string>

#include "../../include/ykgpu.h"
#include "yk_device.hpp"
#include "yk_host_internal.hpp"

namespace ykcast {
using namespace ykhost;
namespace {

constexpr uint32_t kThreads = 256;
constexpr uint64_t kChunk = 1ull << 22;  // rays per launch (and per staging round trip)
// stack entries per lane, the sentinel included: 3 x wide depth + 1 where that is at
// most kStackMax (51 KiB of LDS a block); the top is checked either way, and a lane that overflows
// takes the scan
constexpr uint32_t kStackMin = 4, kStackMax = 48;
// ... of every query kernel of the unit (this one, yk_radiance.hpp, yk_features_sampled.hpp): the
// kernel argument and the LDS size both come from it.  kYkQueryStackForce: yk_features.hip.
inline uint32_t query_stack_cap(const DevTree& t) {
  if (kYkQueryStackForce) return kYkQueryStackForce;
  return std::max(kStackMin, std::min(3 * t.wide_depth + 1, kStackMax));
}
// (the branch-free visit writes up to two entries past the capacity before its check)
inline size_t query_stack_lds(uint32_t stack_cap, uint32_t threads) {
  return (size_t)(stack_cap + 3) * threads * sizeof(int32_t);
}
constexpr uint32_t kKnownFlags = YK_CAST_ANY_HIT | YK_CAST_LINEAR_SCAN | YK_CAST_COUNT_WORK;
constexpr uint32_t kNoId = 0xFFFFFFFFu;

static_assert(sizeof(yk_ray) == 64 && sizeof(yk_hit) == 64 && sizeof(yk_cast_stats) == 64, "ray query records");
static_assert(offsetof(yk_hit, t) == 48 && offsetof(yk_hit, id) == 56 && offsetof(yk_hit, flags) == 60, "yk_hit");

struct CastArgs {
  const double* rays;  // 8 doubles per ray (yk_ray)
  double* hits;        // 8 doubles per hit (yk_hit: id and flags in the last)
  uint32_t n;          // rays of this launch (<= kChunk)
  uint32_t flags;      // YK_CAST_*
  const char* nodes;   // DevNode; child links are byte offsets
  const SphereGeo* leaf_geo;  // leaf order
  const uint32_t* leaf_ids;   // leaf slot -> tuple index
  const SphereGeo* geo;       // tuple order
  const SphereMat* mat;
  unsigned long long* counters;  // kCastStripes x kCastCounters words, or null (asynchronous casts)
  double extent;        // E of the domain rule
  double origin_bound;  // |o|_inf beyond which a ray takes the scan (< 0: every ray)
  int32_t root;
  uint32_t node_bytes, nspheres, stack_cap;
};

// x rounded to float towards +inf / towards -inf, for x >= 0 (bounds of the cull interval)
__device__ __forceinline__ float f32_up(double x) {
  float f = (float)x;
  if ((double)f < x) f = __uint_as_float(__float_as_uint(f) + 1u);
  return f;
}
__device__ __forceinline__ float f32_down(double x) {
  float f = (float)x;
  if ((double)f > x) f = __uint_as_float(__float_as_uint(f) - 1u);
  return f;
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  return v;
}

// the domain rule of include/ykgpu.h, operation for operation (tests/cast_ref.py restates it)
__device__ __forceinline__ bool in_domain(v3 o, v3 d, double tmin, double tmax, double E) {
  const double mo = fmax(fabs(o.x), fmax(fabs(o.y), fabs(o.z)));
  const double md = fmax(fabs(d.x), fmax(fabs(d.y), fabs(d.z)));
  const bool finite6 = fabs(o.x) < INFINITY && fabs(o.y) < INFINITY && fabs(o.z) < INFINITY &&
                       fabs(d.x) < INFINITY && fabs(d.y) < INFINITY && fabs(d.z) < INFINITY;
  if (!finite6) return false;
  if (!(tmin >= 0.0 && tmin < INFINITY)) return false;
  if (!(tmax >= tmin)) return false;
  if (!(md >= 0x1p-500 && md <= 0x1p500)) return false;
  const double s = mo + E;
  if (!(s <= 0x1p500)) return false;
  return md * s <= 0x1p500;
}

__global__ __launch_bounds__(kThreads) void yk_cast(CastArgs a) {
  extern __shared__ __attribute__((aligned(16))) int32_t stack[];  // [entry][lane]: (stack_cap + 3) x 256
  const uint32_t tid = threadIdx.x;
  const uint32_t i = blockIdx.x * kThreads + tid;
  const bool mine = i < a.n;
  const bool any_hit = (a.flags & YK_CAST_ANY_HIT) != 0;
  const bool count = (a.flags & YK_CAST_COUNT_WORK) != 0;

  v3 o = {0, 0, 0}, d = {0, 0, 0};
  double tmin = 0, tmax = 0;
  if (mine) {
    const double2* r = (const double2*)a.rays + (size_t)i * 4;  // (16-byte aligned: the host checks)
    const double2 r0 = r[0], r1 = r[1], r2 = r[2], r3 = r[3];
    o = {r0.x, r0.y, r1.x};
    d = {r1.y, r2.x, r2.y};
    tmin = r3.x;
    tmax = r3.y;
  }
  const bool dom = mine && in_domain(o, d, tmin, tmax, a.extent);

  // the guards that send a ray to the ordered scan: the flag, the host scale guard, an origin
  // beyond the tree's bound, a direction whose float reciprocal the slab test cannot use (zero,
  // |d_k| <= 1e-30 — o/d must stay finite for |o| <= 2^27 — or >= 1e30), and a direction so long
  // against the scene that the float distances fall below float's normal range (the box growth's
  // share of a distance, 2^-21 origin_bound / |d_k|, stays above 2^-111)
  const float dxf = (float)d.x, dyf = (float)d.y, dzf = (float)d.z;
  const float dmin = fminf(fminf(fabsf(dxf), fabsf(dyf)), fabsf(dzf));
  const float dmax = fmaxf(fmaxf(fabsf(dxf), fabsf(dyf)), fabsf(dzf));
  const double mo = fmax(fabs(o.x), fmax(fabs(o.y), fabs(o.z)));
  bool scan = (a.flags & YK_CAST_LINEAR_SCAN) || a.origin_bound < 0 || !(mo <= a.origin_bound) ||
              !(dmin > 1e-30f && dmax < 1e30f) || !(dmax * 0x1p-90f <= (float)a.origin_bound);

  const double aa = ykd::len2(d);
  double best = tmax;  // the cull interval's end: the ray's t_max, then the closest root so far
  int best_id = -1;
  uint32_t n_node = 0, n_test = 0;

  if (dom && !scan) {
    // §4's conservative slab test in float: planes times 1/d less o/d, the far distances scaled by
    // 1 + 2^-17, compared against t_min (1 - 2^-17) rounded down and best (1 + 2^-18) rounded up;
    // it keeps every box the plain test with both distances relaxed by 2^-20 keeps
    const float ix = 1.0f / dxf, iy = 1.0f / dyf, iz = 1.0f / dzf;
    constexpr float kFar = 1.0f + 0x1p-17f;
    const float ixs = ix * kFar, iys = iy * kFar, izs = iz * kFar;
    const float oxf = (float)o.x, oyf = (float)o.y, ozf = (float)o.z;
    const float nox = -(oxf * ix), noy = -(oyf * iy), noz = -(ozf * iz);
    const float fox = -(oxf * ixs), foy = -(oyf * iys), foz = -(ozf * izs);
    const float tmin_lo = f32_down(tmin) * (1.0f - 0x1p-17f);
    // the ray's (near x4, far x4) plane quads inside a WideNode (yk_bvh.hpp)
    const uint32_t qx = ix < 0.0f ? 16u : 0u, qy = 48u + (iy < 0.0f ? 16u : 0u), qz = 96u + (iz < 0.0f ? 16u : 0u);
    // The lane's stack, entries kThreads words apart; entry 0 holds the empty leaf as a sentinel, so
    // a pop never needs a test of its own: the traversal ends when the sentinel has been popped
    // (sp == 0).  sp is the next free entry.
    int32_t* const stk = stack + tid;
    stk[0] = ykbvh::kEmptyLeaf;
    uint32_t sp = 1;
    int32_t node = a.root;
    float ustar = f32_up(best) * (1.0f + 0x1p-18f);
    for (;;) {
      // a lane's run of interior nodes, a loop of its own: the wave tests leaves once every lane
      // holds one.  The visit has no branch: the last slot entered is visited next, the others
      // entered are pushed in slot order (written unconditionally at the top, which moves past what
      // was entered: up to two entries past the capacity, which the stack has), and with no slot
      // entered the entry below the top is next.
      while (node >= 0) {
        if ((uint32_t)node + (uint32_t)sizeof(DevNode) > a.node_bytes) {  // (never: a link outside the tree)
          scan = true;
          break;
        }
        ++n_node;
        const char* w = a.nodes + node;
        const float4 nx = *(const float4*)(w + qx), fx = *(const float4*)(w + qx + 16);
        const float4 ny = *(const float4*)(w + qy), fy = *(const float4*)(w + qy + 16);
        const float4 nz = *(const float4*)(w + qz), fz = *(const float4*)(w + qz + 16);
        const int4 ch = *(const int4*)(w + 144);
        const int32_t popped = stk[(sp - 1) * kThreads];
#define YK_CAST_SLOT(c)                                                                                   \
  (fmaxf(fmaxf(fmaxf(__builtin_fmaf(nx.c, ix, nox), __builtin_fmaf(ny.c, iy, noy)), __builtin_fmaf(nz.c, iz, noz)), \
         tmin_lo) <=                                                                                      \
   fminf(fminf(fminf(__builtin_fmaf(fx.c, ixs, fox), __builtin_fmaf(fy.c, iys, foy)), __builtin_fmaf(fz.c, izs, foz)), \
         ustar))
        const bool h0 = YK_CAST_SLOT(x), h1 = YK_CAST_SLOT(y), h2 = YK_CAST_SLOT(z), h3 = YK_CAST_SLOT(w);
#undef YK_CAST_SLOT
        node = h3 ? ch.w : (h2 ? ch.z : (h1 ? ch.y : (h0 ? ch.x : popped)));
        stk[sp * kThreads] = ch.x;
        sp += (h0 && (h1 || h2 || h3)) ? 1u : 0u;
        stk[sp * kThreads] = ch.y;
        sp += (h1 && (h2 || h3)) ? 1u : 0u;
        stk[sp * kThreads] = ch.z;
        sp += (h2 && h3) ? 1u : 0u;
        sp -= (h0 || h1 || h2 || h3) ? 0u : 1u;
        if (sp > a.stack_cap) {  // stack overflow: the ordered scan decides
          scan = true;
          break;
        }
      }
      if (scan) break;
      bool done = false;
      {
        const uint32_t v = ~(uint32_t)node, first = v >> 4, cnt = v & 15u;
        for (uint32_t k = 0; k < cnt; ++k) {
          const uint32_t slot = first + k;
          if (slot >= a.nspheres) break;  // (never: a leaf outside the table)
          const SphereGeo sg = a.leaf_geo[slot];
          const uint32_t id = a.leaf_ids[slot];
          ++n_test;
          // the reference's discriminant and root, bit for bit (sphere.hpp:29-39)
          const v3 oc = {o.x - sg.cx, o.y - sg.cy, o.z - sg.cz};
          const double hb = ykd::dot(oc, d);
          const double cc = ykd::len2(oc) - sg.rr;
          const double disc = hb * hb - aa * cc;
          if (disc < 0) continue;
          const double sq = ykd::nsqrt(disc);
          double r = (-hb - sq) / aa;
          if (r < tmin) r = (-hb + sq) / aa;
          // the minimum root wins, an exact tie goes to the later tuple index; best_id = -1 with
          // best = t_max: a first root equal to t_max is accepted, as the scan accepts it
          if (r >= tmin && (r < best || (r == best && (int)id > best_id))) {
            best = r;
            best_id = (int)id;
            ustar = f32_up(best) * (1.0f + 0x1p-18f);
            if (any_hit) {
              done = true;
              break;
            }
          }
        }
      }
      if (done || sp == 0) break;  // (sp == 0: the sentinel was this leaf)
      --sp;
      node = stk[sp * kThreads];
    }
  }

  if (dom && scan) {
    // hittable_list::hit_impl over sphere::hit_impl, the literal loop in tuple order
    best = tmax;
    best_id = -1;
    for (uint32_t k = 0; k < a.nspheres; ++k) {
      const SphereGeo sg = a.geo[k];
      ++n_test;
      const v3 oc = {o.x - sg.cx, o.y - sg.cy, o.z - sg.cz};
      const double hb = ykd::dot(oc, d);
      const double cc = ykd::len2(oc) - sg.rr;
      const double disc = hb * hb - aa * cc;
      if (disc < 0) continue;
      const double sq = ykd::nsqrt(disc);
      double root = (-hb - sq) / aa;
      if (root < tmin || best < root) {
        root = (-hb + sq) / aa;
        if (root < tmin || best < root) continue;
      }
      best = root;
      best_id = (int)k;
      if (any_hit) break;
    }
  }

  const bool hit = dom && best_id >= 0;
  if (mine) {
    double out[7] = {0, 0, 0, 0, 0, 0, 0};
    uint32_t id = kNoId, fl = dom ? 0u : (uint32_t)YK_HIT_OUT_OF_DOMAIN;
    if (hit) {
      fl = YK_HIT_HIT;
      if (!any_hit) {
        // hit record (sphere.hpp:41-45, hittable.hpp:23-27), once, from (best, best_id)
        const SphereGeo sg = a.geo[best_id];
        const double radius = a.mat[best_id].radius;
        const v3 p = ykd::add(o, ykd::mul(d, best));
        const v3 outward = ykd::divs(ykd::sub(p, v3{sg.cx, sg.cy, sg.cz}), radius);
        const bool front = ykd::dot(d, outward) < 0;
        const v3 nrm = front ? outward : ykd::neg(outward);
        out[0] = p.x, out[1] = p.y, out[2] = p.z;
        out[3] = nrm.x, out[4] = nrm.y, out[5] = nrm.z;
        out[6] = best;
        id = (uint32_t)best_id;
        if (front) fl |= YK_HIT_FRONT_FACE;
      }
    }
    double2* h = (double2*)a.hits + (size_t)i * 4;
    h[0] = make_double2(out[0], out[1]);
    h[1] = make_double2(out[2], out[3]);
    h[2] = make_double2(out[4], out[5]);
    h[3] = make_double2(out[6], __builtin_bit_cast(double, (uint64_t)id | ((uint64_t)fl << 32)));
  }

  // statistics: one atomic per wave and counter, from ballots (every lane of the block is here),
  // into one of kCastStripes copies of the counters chosen by the wave's number: atomics of many
  // waves on one address serialise (the host adds the copies up)
  if (a.counters) {
    unsigned long long* const cnt = a.counters + (size_t)((blockIdx.x * (kThreads / 64u) + tid / 64u) % kCastStripes) * kCastCounters;
    const unsigned long long m_rays = __ballot(mine), m_hits = __ballot(hit), m_ood = __ballot(mine && !dom),
                             m_scan = __ballot(dom && scan);
    uint32_t s_node = 0, s_test = 0;
    if (count) {
      s_node = wave_sum(n_node);
      s_test = wave_sum(n_test);
    }
    if ((tid & 63u) == 0) {
      if (m_rays) atomicAdd(cnt + 0, (unsigned long long)__popcll(m_rays));
      if (m_hits) atomicAdd(cnt + 1, (unsigned long long)__popcll(m_hits));
      if (m_ood) atomicAdd(cnt + 2, (unsigned long long)__popcll(m_ood));
      if (m_scan) atomicAdd(cnt + 3, (unsigned long long)__popcll(m_scan));
      if (s_node) atomicAdd(cnt + 4, (unsigned long long)s_node);
      if (s_test) atomicAdd(cnt + 5, (unsigned long long)s_test);
    }
  }
}

// one launch over rays [0, n), n <= kChunk, on st
hipError_t enqueue(const ykgpu_context* ctx, const void* rays, void* hits, uint32_t n, uint32_t flags,
                   unsigned long long* counters, hipStream_t st) {
  const DevTree& t = ctx->t64;
  CastArgs a{};
  a.rays = (const double*)rays;
  a.hits = (double*)hits;
  a.n = n;
  a.flags = flags;
  a.nodes = (const char*)t.nodes;
  a.leaf_geo = (const SphereGeo*)t.leaf_geo;
  a.leaf_ids = t.leaf_ids;
  a.geo = ctx->d_geo;
  a.mat = ctx->d_mat;
  a.counters = counters;
  a.extent = ctx->cast_extent;
  a.origin_bound = t.origin_bound;
  a.root = t.root;
  a.node_bytes = t.n_nodes * (uint32_t)sizeof(DevNode);
  a.nspheres = ctx->nspheres;
  a.stack_cap = query_stack_cap(t);
  const size_t lds = query_stack_lds(a.stack_cap, kThreads);
  hipLaunchKernelGGL(yk_cast, dim3((n + kThreads - 1) / kThreads), dim3(kThreads), lds, st, a);
  return hipGetLastError();
}

int check_call(const ykgpu_context* ctx, const void* rays, uint64_t n, uint32_t flags, const void* hits) {
  if (!ctx) return fail(YK_ERR_INVALID, "null context");
  if (flags & ~kKnownFlags) return fail(YK_ERR_INVALID, "cast: unknown flag bits");
  if (n && (!rays || !hits)) return fail(YK_ERR_INVALID, "cast: null rays or hits");
  if (n && !ctx->have_scene) return fail(YK_ERR_NO_SCENE, "cast before ykgpu_set_scene");
  return YK_OK;
}

}  // namespace
}  // namespace ykcast

extern "C" {

int ykgpu_cast_rays(ykgpu_context* ctx, const yk_ray* rays_host, uint64_t n, uint32_t flags, yk_hit* hits_host) {
  if (int rc = ykcast::check_call(ctx, rays_host, n, flags, hits_host)) return rc;
  if (n == 0) return YK_OK;
  const auto t0 = std::chrono::steady_clock::now();
  YK_HIP(hipSetDevice(ctx->device));
  const size_t need = (size_t)std::min<uint64_t>(n, ykcast::kChunk);
  if (need > ctx->cast_cap) {
    (void)hipFree(ctx->d_cast_rays);
    (void)hipFree(ctx->d_cast_hits);
    ctx->d_cast_rays = ctx->d_cast_hits = nullptr;
    ctx->cast_cap = 0;
    YK_HIP(hipMalloc(&ctx->d_cast_rays, need * sizeof(yk_ray)));
    YK_HIP(hipMalloc(&ctx->d_cast_hits, need * sizeof(yk_hit)));
    ctx->cast_cap = need;
  }
  constexpr size_t kCounterBytes = (size_t)kCastStripes * kCastCounters * sizeof(unsigned long long);
  if (!ctx->d_cast_counters) YK_HIP(hipMalloc(&ctx->d_cast_counters, kCounterBytes));
  const hipStream_t st = ctx->stream;
  hipEvent_t ev[2] = {nullptr, nullptr};
  hipError_t e = hipEventCreate(&ev[0]);
  if (e == hipSuccess) e = hipEventCreate(&ev[1]);
  if (e == hipSuccess) e = hipMemsetAsync(ctx->d_cast_counters, 0, kCounterBytes, st);
  double kernel_ms = 0;
  for (uint64_t base = 0; base < n && e == hipSuccess; base += ykcast::kChunk) {
    const uint32_t cnt = (uint32_t)std::min<uint64_t>(ykcast::kChunk, n - base);
    e = hipMemcpyAsync(ctx->d_cast_rays, rays_host + base, (size_t)cnt * sizeof(yk_ray), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipEventRecord(ev[0], st);
    if (e == hipSuccess) e = ykcast::enqueue(ctx, ctx->d_cast_rays, ctx->d_cast_hits, cnt, flags, ctx->d_cast_counters, st);
    if (e == hipSuccess) e = hipEventRecord(ev[1], st);
    if (e == hipSuccess)
      e = hipMemcpyAsync(hits_host + base, ctx->d_cast_hits, (size_t)cnt * sizeof(yk_hit), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    float ms = 0;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, ev[0], ev[1]);
    kernel_ms += ms;
  }
  unsigned long long stripes[kCastStripes][kCastCounters] = {}, c[kCastCounters] = {};
  if (e == hipSuccess) e = hipMemcpy(stripes, ctx->d_cast_counters, sizeof(stripes), hipMemcpyDeviceToHost);
  for (const auto& sc : stripes)
    for (int k = 0; k < kCastCounters; ++k) c[k] += sc[k];
  for (hipEvent_t v : ev)
    if (v) (void)hipEventDestroy(v);
  if (e != hipSuccess)
    return ykhost::fail(e == hipErrorOutOfMemory ? YK_ERR_NOMEM : YK_ERR_DEVICE,
                std::string("ykgpu_cast_rays: ") + hipGetErrorString(e));
  yk_cast_stats& s = ctx->cast_stats;
  s.kernel_ms = kernel_ms;
  s.rays = c[0];
  s.hits = c[1];
  s.out_of_domain = c[2];
  s.scan_rays = c[3];
  s.node_visits = c[4];
  s.sphere_tests = c[5];
  s.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return YK_OK;
}

int ykgpu_cast_rays_async(ykgpu_context* ctx, const void* rays_device, uint64_t n, uint32_t flags,
                          void* hits_device, void* stream) {
  if (int rc = ykcast::check_call(ctx, rays_device, n, flags, hits_device)) return rc;
  if (n == 0) return YK_OK;
  if (((uintptr_t)rays_device | (uintptr_t)hits_device) & 15u)
    return ykhost::fail(YK_ERR_INVALID, "cast: rays and hits must be 16-byte aligned");
  YK_HIP(hipSetDevice(ctx->device));
  const hipStream_t st = stream ? (hipStream_t)stream : ctx->stream;
  if (!ctx->cast_ev) YK_HIP(hipEventCreateWithFlags(&ctx->cast_ev, hipEventDisableTiming));
  for (uint64_t base = 0; base < n; base += ykcast::kChunk) {
    const uint32_t cnt = (uint32_t)std::min<uint64_t>(ykcast::kChunk, n - base);
    YK_HIP(ykcast::enqueue(ctx, (const yk_ray*)rays_device + base, (yk_hit*)hits_device + base, cnt, flags, nullptr, st));
  }
  YK_HIP(hipEventRecord(ctx->cast_ev, st));  // (ykgpu_set_scene waits for it)
  return YK_OK;
}

int ykgpu_cast_get_stats(ykgpu_context* ctx, yk_cast_stats* out) {
  if (!ctx || !out) return ykhost::fail(YK_ERR_INVALID, "null argument");
  *out = ctx->cast_stats;
  return YK_OK;
}

}  // extern "C"

#endif
