// yk_gather.hpp — gather queries (include/ykgpu.h "gather queries"): diffuse
// radiance at arbitrary points.  A point (p, n, seed, skip) stands for n_samples path rays, the
// reference's lambertian::scatter at a surface at p facing n (material.hpp:50-59), each followed by
// ray_color; the record is the fold of their colours.  tests/gather_ref.py restates every record
// bit for bit.
//
// Part of the unit yk_features.hip, which includes this file after yk_radiance.hpp.  A call is
// processed in chunks of whole points; a chunk of cnt points is three launches on one stream:
//   yk_gather_starts  one lane per kWalk sample slots (sample-major: slot j = s * cnt + i, so
//                     adjacent lanes read adjacent points and write adjacent rays): the seed walk
//                     to x_397 (mt19937; ykd::mt_walk397xn, as yk_radiance_starts), the discard,
//                     the scatter's six words and its direction; it writes the slot's yk_path_ray
//                     (p, d, seed + s, skip + 6) into the radiance queries' staging and x397[j];
//   yk_radiance_paths the radiance queries' path kernel as it is (ykrad::enqueue_paths), over the
//                     chunk's slots: its 256-ray claims cover neighbouring points;
//   yk_gather_fold    one lane per point: the records of s = 0 .. N-1 in order into sum, sumsq, open
//                     and flags, the 64-byte yk_gather as four 16-byte stores.
// The path kernel is reused, not copied: a gather ray IS a radiance query's ray, so the two cannot
// drift apart, and the scatter in front of it is the only arithmetic this file adds.
#ifndef YK_GATHER_HPP
#define YK_GATHER_HPP

#include "yk_radiance.hpp"

namespace ykgather {
using namespace ykhost;
namespace {

constexpr uint32_t kThreads = 256;
constexpr uint32_t kWalk = ykrad::kWalk;  // sample slots per lane of the starts kernel
constexpr uint32_t kMaxSamples = 65536;
// the scatter's six words lie inside mt19937's lazy words (ykd::kLazyDraws = 227)
constexpr uint32_t kMaxSkip = ykd::kLazyDraws - 6;
constexpr uint32_t kPointFlags = YK_RAD_OUT_OF_DOMAIN | YK_RAD_MT_FALLBACK;

static_assert(sizeof(yk_gather_point) == 64 && sizeof(yk_gather) == 64 && sizeof(yk_gather_params) == 32 &&
                  sizeof(yk_gather_stats) == 64, "gather query records");
static_assert(offsetof(yk_gather_point, n) == 24 && offsetof(yk_gather_point, seed) == 48 &&
                  offsetof(yk_gather_point, skip) == 52, "yk_gather_point");
static_assert(offsetof(yk_gather, sumsq) == 24 && offsetof(yk_gather, samples) == 48 && offsetof(yk_gather, open) == 52 &&
                  offsetof(yk_gather, flags) == 56, "yk_gather");
static_assert(offsetof(yk_gather_params, t_min) == 16, "yk_gather_params");
static_assert(offsetof(yk_gather_stats, points) == 32 && offsetof(yk_gather_stats, out_of_domain) == 56, "yk_gather_stats");
static_assert(kMaxSkip == 221, "include/ykgpu.h: skip <= 221");

struct StartArgs {
  const double* points;  // 8 doubles per point (yk_gather_point: seed and skip in the seventh)
  double* rays;          // 8 doubles per slot (yk_path_ray)
  uint32_t* x397;        // per slot (mt19937)
  uint32_t cnt;          // points of the chunk
  uint32_t slots;        // cnt * n_samples (<= kRadChunk)
};

struct FoldArgs {
  const double* rec;  // 8 doubles per slot (yk_radiance)
  double* out;        // 8 doubles per point (yk_gather)
  uint32_t cnt, n_samples;
};

template <class G>
__global__ __launch_bounds__(kThreads) void yk_gather_starts(StartArgs a) {
  constexpr bool kMt = __is_same(G, ykd::MtLane);
  const uint32_t base = blockIdx.x * (kThreads * kWalk) + threadIdx.x;
  uint32_t x[kWalk], pt[kWalk], smp[kWalk];
#pragma unroll
  for (uint32_t k = 0; k < kWalk; ++k) {
    const uint32_t j = base + k * kThreads;
    smp[k] = j / a.cnt;
    pt[k] = j - smp[k] * a.cnt;
    // yk_gather_point::seed + s, uint32 wrap
    x[k] = j < a.slots ? ((const uint32_t*)a.points)[(size_t)pt[k] * 16 + 12] + smp[k] : 0u;
  }
  uint32_t seed[kWalk];
#pragma unroll
  for (uint32_t k = 0; k < kWalk; ++k) seed[k] = x[k];
  if constexpr (kMt) ykd::mt_walk397xn(x);
#pragma unroll
  for (uint32_t k = 0; k < kWalk; ++k) {
    const uint32_t j = base + k * kThreads;
    if (j >= a.slots) continue;
    const double2* q = (const double2*)a.points + (size_t)pt[k] * 4;  // (16-byte aligned: the host checks)
    const double2 q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3];
    const v3 p = {q0.x, q0.y, q1.x}, n = {q1.y, q2.x, q2.y};
    const uint32_t skip = (uint32_t)(__builtin_bit_cast(uint64_t, q3.x) >> 32);
    v3 d = {0.0, 0.0, 0.0};
    // a point past the skip limit or with a zero normal does no arithmetic: the zero direction
    // puts its rays outside the path kernel's domain
    if (skip <= kMaxSkip && !(n.x == 0.0 && n.y == 0.0 && n.z == 0.0)) {
      G g;  // (its scratch is never read: a slot draws at most kMaxSkip + 6 = 227 lazy words)
      ykd::engine_start(g, seed[k], x[k]);
      for (uint32_t w = 0; w < skip; ++w) (void)ykd::rng_next<true>(g);  // discard(skip), with the lazy draw
      // lambertian::scatter (material.hpp:50-59), random_unit_vector (:33-36): vec3::random's x, y, z
      v3 ru;
      ru.x = ykd::uniform<true>(g, -1.0, 1.0);
      ru.y = ykd::uniform<true>(g, -1.0, 1.0);
      ru.z = ykd::uniform<true>(g, -1.0, 1.0);
      ru = ykd::divs(ru, ykd::nsqrt(ykd::len2(ru)));
      d = ykd::add(n, ru);
      if (ykd::near_zero(d)) d = n;
    }
    double2* r = (double2*)a.rays + (size_t)j * 4;
    r[0] = make_double2(p.x, p.y);
    r[1] = make_double2(p.z, d.x);
    r[2] = make_double2(d.y, d.z);
    r[3] = make_double2(__builtin_bit_cast(double, (uint64_t)seed[k] | ((uint64_t)(skip + 6u) << 32)), 0.0);
    if constexpr (kMt) a.x397[j] = x[k];
  }
}

__global__ __launch_bounds__(kThreads) void yk_gather_fold(FoldArgs a) {
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= a.cnt) return;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, q0 = 0.0, q1 = 0.0, q2 = 0.0;
  uint32_t open = 0, flags = 0;
  for (uint32_t s = 0; s < a.n_samples; ++s) {
    const double2* r = (const double2*)a.rec + ((size_t)s * a.cnt + i) * 4;
    const double2 r0 = r[0], r1 = r[1], r2 = r[2], r3 = r[3];
    const uint32_t segments = (uint32_t)(__builtin_bit_cast(uint64_t, r2.y) >> 32);
    const uint32_t fl = (uint32_t)__builtin_bit_cast(uint64_t, r3.x);
    s0 = s0 + r0.x;
    s1 = s1 + r0.y;
    s2 = s2 + r1.x;
    q0 = q0 + r0.x * r0.x;  // (the unit is compiled with -ffp-contract=off: product, then sum)
    q1 = q1 + r0.y * r0.y;
    q2 = q2 + r1.x * r1.x;
    open += ((fl & YK_RAD_SKY) && segments == 1) ? 1u : 0u;
    flags |= fl & kPointFlags;
  }
  double2* o = (double2*)a.out + (size_t)i * 4;
  o[0] = make_double2(s0, s1);
  o[1] = make_double2(s2, q0);
  o[2] = make_double2(q1, q2);
  o[3] = make_double2(__builtin_bit_cast(double, (uint64_t)a.n_samples | ((uint64_t)open << 32)),
                      __builtin_bit_cast(double, (uint64_t)flags));
}

// whole points per chunk: no fold is carried across chunks, and a chunk's slots fit the radiance
// queries' staging (kRadChunk rays)
inline uint64_t chunk_points(uint32_t n_samples) { return std::max<uint64_t>(1, kRadChunk / n_samples); }

inline yk_radiance_params path_params(const yk_gather_params* p) {
  yk_radiance_params r{};
  r.max_depth = p->max_depth;
  r.rng = p->rng;
  r.flags = p->flags;
  r.t_min = p->t_min;
  return r;
}

int check_call(const ykgpu_context* ctx, const yk_gather_params* p, const void* points, uint64_t n, const void* out) {
  if (!ctx || !p) return fail(YK_ERR_INVALID, "null argument");
  if (p->n_samples < 1 || p->n_samples > kMaxSamples) return fail(YK_ERR_INVALID, "gather: n_samples must be 1..65536");
  if (p->reserved) return fail(YK_ERR_INVALID, "gather: reserved fields must be 0");
  const yk_radiance_params rp = path_params(p);
  return ykrad::check_call(ctx, &rp, points, n, out);
}

// the three launches of one chunk on st: cnt points at `points` into cnt records at `out` (device
// memory); ev (may be null): four events around the launches
hipError_t enqueue_chunk(const ykgpu_context* ctx, const yk_gather_params* p, const yk_radiance_params* rp,
                         const ykrad::Plan& pl, const void* points, void* out, uint32_t cnt, hipStream_t st,
                         const hipEvent_t* ev) {
  const uint32_t slots = cnt * p->n_samples;
  if (ev)
    if (hipError_t e = hipEventRecord(ev[0], st)) return e;
  StartArgs sa{};
  sa.points = (const double*)points;
  sa.rays = (double*)ctx->d_rad_rays;
  sa.x397 = ctx->d_rad_x397;
  sa.cnt = cnt;
  sa.slots = slots;
  const uint32_t per = kThreads * kWalk;
  if (p->rng == YK_RNG_XOR128)
    hipLaunchKernelGGL(yk_gather_starts<ykd::X128Lane>, dim3((slots + per - 1) / per), dim3(kThreads), 0, st, sa);
  else
    hipLaunchKernelGGL(yk_gather_starts<ykd::MtLane>, dim3((slots + per - 1) / per), dim3(kThreads), 0, st, sa);
  if (hipError_t e = hipGetLastError()) return e;
  if (ev)
    if (hipError_t e = hipEventRecord(ev[1], st)) return e;
  if (hipError_t e = ykrad::enqueue_paths(ctx, rp, pl, ctx->d_rad_rays, ctx->d_rad_out, slots, nullptr, st)) return e;
  if (ev)
    if (hipError_t e = hipEventRecord(ev[2], st)) return e;
  FoldArgs fa{};
  fa.rec = (const double*)ctx->d_rad_out;
  fa.out = (double*)out;
  fa.cnt = cnt;
  fa.n_samples = p->n_samples;
  hipLaunchKernelGGL(yk_gather_fold, dim3((cnt + kThreads - 1) / kThreads), dim3(kThreads), 0, st, fa);
  if (hipError_t e = hipGetLastError()) return e;
  if (ev)
    if (hipError_t e = hipEventRecord(ev[3], st)) return e;
  return hipSuccess;
}

// the plan, the path kernel's scratch and the staging of a call's largest chunk
int prepare(ykgpu_context* ctx, const yk_gather_params* p, const yk_radiance_params* rp, uint64_t n, ykrad::Plan& pl) {
  if (int rc = ykrad::make_plan(ctx, rp, pl)) return rc;
  if (int rc = ykrad::ensure(ctx, rp, pl)) return rc;
  return ykrad::ensure_staging(ctx, (size_t)(std::min<uint64_t>(n, chunk_points(p->n_samples)) * p->n_samples));
}

}  // namespace
}  // namespace ykgather

extern "C" {

int ykgpu_gather_points(ykgpu_context* ctx, const yk_gather_params* params, const yk_gather_point* points_host,
                        uint64_t n, yk_gather* out_host) {
  if (int rc = ykgather::check_call(ctx, params, points_host, n, out_host)) return rc;
  if (n == 0) return YK_OK;
  const auto t0 = std::chrono::steady_clock::now();
  YK_HIP(hipSetDevice(ctx->device));
  const yk_radiance_params rp = ykgather::path_params(params);
  ykrad::Plan pl;
  if (int rc = ykgather::prepare(ctx, params, &rp, n, pl)) return rc;
  const uint64_t cp = ykgather::chunk_points(params->n_samples);
  const size_t need = (size_t)std::min<uint64_t>(n, cp);
  if (int rc = ykquery::ensure_pair(ctx->d_gat_points, ctx->d_gat_out, ctx->gat_cap, need, sizeof(yk_gather_point),
                                    sizeof(yk_gather), ctx->rad_ev))
    return rc;
  const hipStream_t st = ctx->stream;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  hipError_t e = hipStreamWaitEvent(st, ctx->rad_ev, 0);  // (after the context's queries on other streams)
  for (int k = 0; k < 4 && e == hipSuccess; ++k) e = hipEventCreate(&ev[k]);
  double kernel_ms = 0, starts_ms = 0, fold_ms = 0;
  for (uint64_t base = 0; base < n && e == hipSuccess; base += cp) {
    const uint32_t cnt = (uint32_t)std::min<uint64_t>(cp, n - base);
    e = hipMemcpyAsync(ctx->d_gat_points, points_host + base, (size_t)cnt * sizeof(yk_gather_point), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = ykgather::enqueue_chunk(ctx, params, &rp, pl, ctx->d_gat_points, ctx->d_gat_out, cnt, st, ev);
    if (e == hipSuccess)
      e = hipMemcpyAsync(out_host + base, ctx->d_gat_out, (size_t)cnt * sizeof(yk_gather), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    float ms = 0, ms0 = 0, ms1 = 0;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, ev[0], ev[3]);
    if (e == hipSuccess) e = hipEventElapsedTime(&ms0, ev[0], ev[1]);
    if (e == hipSuccess) e = hipEventElapsedTime(&ms1, ev[2], ev[3]);
    kernel_ms += ms;
    starts_ms += ms0;
    fold_ms += ms1;
  }
  for (hipEvent_t v : ev)
    if (v) (void)hipEventDestroy(v);
  if (e != hipSuccess)
    return ykhost::fail(e == hipErrorOutOfMemory ? YK_ERR_NOMEM : YK_ERR_DEVICE,
                        std::string("ykgpu_gather_points: ") + hipGetErrorString(e));
  // the statistics are counts over the records themselves
  uint64_t open = 0, ood = 0, fb = 0;
  for (uint64_t i = 0; i < n; ++i) {
    open += out_host[i].open;
    ood += (out_host[i].flags & YK_RAD_OUT_OF_DOMAIN) ? 1 : 0;
    fb += (out_host[i].flags & YK_RAD_MT_FALLBACK) ? 1 : 0;
  }
  yk_gather_stats& s = ctx->gat_stats;
  s.kernel_ms = kernel_ms;
  s.starts_ms = starts_ms;
  s.fold_ms = fold_ms;
  s.points = n;
  s.rays = n * params->n_samples;
  s.open = open;
  s.out_of_domain = ykrad::sat32(ood);
  s.mt_fallbacks = ykrad::sat32(fb);
  s.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return YK_OK;
}

int ykgpu_gather_points_async(ykgpu_context* ctx, const yk_gather_params* params, const void* points_device,
                              uint64_t n, void* out_device, void* stream) {
  if (int rc = ykgather::check_call(ctx, params, points_device, n, out_device)) return rc;
  if (n == 0) return YK_OK;
  if (((uintptr_t)points_device | (uintptr_t)out_device) & 15u)
    return ykhost::fail(YK_ERR_INVALID, "gather: points and records must be 16-byte aligned");
  YK_HIP(hipSetDevice(ctx->device));
  const yk_radiance_params rp = ykgather::path_params(params);
  ykrad::Plan pl;
  if (int rc = ykgather::prepare(ctx, params, &rp, n, pl)) return rc;
  const hipStream_t st = stream ? (hipStream_t)stream : ctx->stream;
  YK_HIP(hipStreamWaitEvent(st, ctx->rad_ev, 0));  // (the context's queries and gathers share staging and scratch)
  const uint64_t cp = ykgather::chunk_points(params->n_samples);
  for (uint64_t base = 0; base < n; base += cp) {
    const uint32_t cnt = (uint32_t)std::min<uint64_t>(cp, n - base);
    YK_HIP(ykgather::enqueue_chunk(ctx, params, &rp, pl, (const yk_gather_point*)points_device + base,
                                   (yk_gather*)out_device + base, cnt, st, nullptr));
  }
  YK_HIP(hipEventRecord(ctx->rad_ev, st));  // (ykgpu_set_scene and the next query or gather wait for it)
  return YK_OK;
}

int ykgpu_gather_get_stats(ykgpu_context* ctx, yk_gather_stats* out) {
  if (!ctx || !out) return ykhost::fail(YK_ERR_INVALID, "null argument");
  *out = ctx->gat_stats;
  return YK_OK;
}

}  // extern "C"

#endif
