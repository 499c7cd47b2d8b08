// yk_cast.hpp — ray queries (include/ykgpu.h "ray queries"): the reference's
// world.hit(r, t_min, t_max) for batches of arbitrary rays, closest hits and occlusion tests, in
// IEEE double so that numpy restates every record bit for bit (tests/cast_ref.py).
//
// Part of the unit yk_features.hip, which includes this file once at its end: the library's other
// first-hit query, kept in a file of its own (the list of units is fixed, tests/test_build_knobs.py).
// Everything here but the three C-ABI entry points lives in namespace ykcast.  One kernel, yk_cast,
// one ray per lane in 256-thread blocks, a plain launch: the ray's record in, the query kernels'
// closest hit (ykquery::closest_hit, yk_query.hpp: the context's FP64 tree with a checked per-lane
// stack in LDS, the ordered scan for the rays the float slab test cannot serve), the hit's record and
// the statistics out.
#ifndef YK_CAST_HPP
#define YK_CAST_HPP

#include <chrono>
#include <string>

#include "yk_query.hpp"

namespace ykcast {
using namespace ykhost;
namespace {

constexpr uint32_t kThreads = 256;
constexpr uint64_t kChunk = 1ull << 22;  // rays per launch (and per staging round trip)
constexpr uint32_t kKnownFlags = YK_CAST_ANY_HIT | YK_CAST_LINEAR_SCAN | YK_CAST_COUNT_WORK;
constexpr uint32_t kNoId = 0xFFFFFFFFu;

static_assert(sizeof(yk_ray) == 64 && sizeof(yk_hit) == 64 && sizeof(yk_cast_stats) == 64, "ray query records");
static_assert(offsetof(yk_hit, t) == 48 && offsetof(yk_hit, id) == 56 && offsetof(yk_hit, flags) == 60, "yk_hit");

struct CastArgs {
  const double* rays;  // 8 doubles per ray (yk_ray)
  double* hits;        // 8 doubles per hit (yk_hit: id and flags in the last)
  uint32_t n;          // rays of this launch (<= kChunk)
  uint32_t flags;      // YK_CAST_*
  unsigned long long* counters;  // kCastStripes x kCastCounters words, or null (asynchronous casts)
  ykquery::QueryTree q;
};

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
  const bool dom = mine && ykquery::in_domain(o, d, tmin, tmax, a.q.extent);

  // world.hit(r, t_min, t_max): the tree's visit or the ordered scan (yk_query.hpp)
  const ykquery::Hit h = ykquery::closest_hit<kThreads>(a.q, stack + tid, dom, o, d, tmin, tmax,
                                                        (a.flags & YK_CAST_LINEAR_SCAN) != 0, any_hit);

  const bool hit = dom && h.id >= 0;
  if (mine) {
    double out[7] = {0, 0, 0, 0, 0, 0, 0};
    uint32_t id = kNoId, fl = dom ? 0u : (uint32_t)YK_HIT_OUT_OF_DOMAIN;
    if (hit) {
      fl = YK_HIT_HIT;
      if (!any_hit) {
        const ykquery::HitRecord rec = ykquery::hit_record(o, d, h.t, a.q.geo[h.id], a.q.mat[h.id].radius);
        out[0] = rec.p.x, out[1] = rec.p.y, out[2] = rec.p.z;
        out[3] = rec.nrm.x, out[4] = rec.nrm.y, out[5] = rec.nrm.z;
        out[6] = h.t;
        id = (uint32_t)h.id;
        if (rec.front) fl |= YK_HIT_FRONT_FACE;
      }
    }
    double2* w = (double2*)a.hits + (size_t)i * 4;
    w[0] = make_double2(out[0], out[1]);
    w[1] = make_double2(out[2], out[3]);
    w[2] = make_double2(out[4], out[5]);
    w[3] = make_double2(out[6], __builtin_bit_cast(double, (uint64_t)id | ((uint64_t)fl << 32)));
  }

  // statistics: one atomic per wave and counter, from ballots (every lane of the block is here),
  // into one of kCastStripes copies of the counters chosen by the wave's number: atomics of many
  // waves on one address serialise (the host adds the copies up)
  if (a.counters) {
    unsigned long long* const cnt = a.counters + (size_t)((blockIdx.x * (kThreads / 64u) + tid / 64u) % kCastStripes) * kCastCounters;
    const unsigned long long m_rays = __ballot(mine), m_hits = __ballot(hit), m_ood = __ballot(mine && !dom),
                             m_scan = __ballot(h.scanned);
    uint32_t s_node = 0, s_test = 0;
    if (count) {
      s_node = ykquery::wave_sum(h.nodes);
      s_test = ykquery::wave_sum(h.tests);
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
  CastArgs a{};
  a.rays = (const double*)rays;
  a.hits = (double*)hits;
  a.n = n;
  a.flags = flags;
  a.counters = counters;
  a.q = ykquery::query_tree(ctx);
  const size_t lds = ykquery::query_stack_lds(a.q.stack_cap, kThreads);
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
  if (int rc = ykquery::ensure_pair(ctx->d_cast_rays, ctx->d_cast_hits, ctx->cast_cap, need, sizeof(yk_ray),
                                    sizeof(yk_hit), nullptr))
    return rc;
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
  unsigned long long c[kCastCounters] = {};
  if (e == hipSuccess) e = ykquery::read_stripes(ctx->d_cast_counters, kCastStripes, kCastCounters, c);
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
