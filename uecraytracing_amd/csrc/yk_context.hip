// yk_context.hip — a context and its scene: the calling thread's error slot, context create and
// destroy, the scene upload (yk_mat_prep, the two BVHs and their LDS plans, ykgpu_set_scene), the
// statistics of a call (device_bytes, finish_stats, ykgpu_get_stats) and the one-shot render calls
// of the C-ABI (include/ykgpu.h).  What a render call enqueues is yk_pipeline.hip's launch().
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/ykgpu.h"
#include "yk_host_internal.hpp"
#include "yk_schedule.hpp"

using namespace ykhost;

namespace {

thread_local std::string g_last_error;

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

}  // namespace

namespace ykhost {

int fail(int code, const std::string& msg) {
  g_last_error = msg;
  return code;
}
std::string& last_error() { return g_last_error; }

// Device memory the context holds (yk_render_stats.device_bytes)
uint64_t device_bytes(const ykgpu_context* ctx) {
  uint64_t b = ctx->t64.bytes + ctx->t32.bytes;
  if (ctx->d_geo) b += (uint64_t)ctx->nspheres * (sizeof(SphereGeo) + sizeof(SphereMat) + sizeof(float4));
  b += ctx->warm_cap + ctx->col_cap * sizeof(double) + ctx->acc_cap * sizeof(double);
  b += ctx->retry_cap * sizeof(uint4);
  b += (uint64_t)ctx->order_slots * sizeof(uint32_t) + (uint64_t)ctx->counter_cap * sizeof(uint32_t);
  b += kCounters * sizeof(unsigned long long);
  b += sky_bytes(ctx);
  b += ctx->seed_tab_words * sizeof(uint32_t);
  if (ctx->d_mt) b += 2ull * ctx->scratch_lanes * ykd::kMtN * sizeof(uint32_t);
  if (ctx->d_ids) b += 2ull * ctx->id_lanes * ctx->id_stride * sizeof(uint16_t);
  b += ctx->rgb_cap + ctx->sums_cap * sizeof(double);
  b += (uint64_t)ctx->cast_cap * (sizeof(yk_ray) + sizeof(yk_hit));
  if (ctx->d_cast_counters) b += (uint64_t)kCastStripes * kCastCounters * sizeof(unsigned long long);
  b += (uint64_t)ctx->rad_cap * (sizeof(yk_path_ray) + sizeof(yk_radiance));
  b += (uint64_t)ctx->gat_cap * (sizeof(yk_gather_point) + sizeof(yk_gather));
  if (ctx->d_rad_x397) b += kRadChunk * sizeof(uint32_t) + sizeof(uint32_t);
  b += (uint64_t)ctx->rad_mt_lanes * ykd::kMtN * sizeof(uint32_t);
  b += (uint64_t)ctx->rad_lanes * ctx->rad_id_stride * sizeof(uint16_t);
  if (ctx->d_rad_counters) b += (uint64_t)kRadStripes * kRadCounters * sizeof(unsigned long long);
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

}  // namespace ykhost

namespace {

// Builds one BVH over the scene and uploads it into t: `geo` holds the tuple-order geometry the
// kernel's leaves read (`elem` bytes per sphere), stored in leaf order; wopt orders the slots of
// its wide nodes; kern[v][lds] are the kernel
// instances of workgroup size v (kBlock, kBlockX128) that read the tree from global memory / LDS
// (for the occupancy).
int upload_tree(ykgpu_context* ctx, DevTree& t, const std::vector<double>& centers, const std::vector<double>& radii,
                double cam_ext, const ykbvh::Options& opt, uint32_t leaf_cap, const void* geo, size_t elem,
                size_t tgeo_elem, const RenderKernel (&kern)[2][2], bool exact_stack,
                const ykbvh::WideOptions& wopt) {
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
  const std::vector<DevNode> snodes = ykbvh::wide_nodes(bvh, &root_code, &wdepth, wopt);
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
  t.wide_depth = wdepth;
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
  (void)hipFree(ctx->d_sky_path);
  (void)hipFree(ctx->d_sky_list);
  (void)hipFree(ctx->d_sky_acc);
  (void)hipFree(ctx->d_sky_mt);
  (void)hipFree(ctx->d_sky_off);
  if (ctx->sky_ev) (void)hipEventDestroy(ctx->sky_ev);
  (void)hipFree(ctx->d_seed_tab);
  if (ctx->seed_ev_aux) (void)hipEventDestroy(ctx->seed_ev_aux);
  if (ctx->seed_ev_red) (void)hipEventDestroy(ctx->seed_ev_red);
  ctx->t64.release();
  ctx->t32.release();
  (void)hipFree(ctx->d_mt);
  (void)hipFree(ctx->d_ids);
  (void)hipFree(ctx->d_rgb);
  (void)hipFree(ctx->d_sums);
  (void)hipFree(ctx->d_cast_rays);
  (void)hipFree(ctx->d_cast_hits);
  (void)hipFree(ctx->d_cast_counters);
  if (ctx->cast_ev) (void)hipEventDestroy(ctx->cast_ev);
  for (void* q : {ctx->d_rad_rays, ctx->d_rad_out, (void*)ctx->d_rad_x397, (void*)ctx->d_rad_claim, (void*)ctx->d_rad_mt,
                  (void*)ctx->d_rad_ids, (void*)ctx->d_rad_counters, ctx->d_gat_points, ctx->d_gat_out})
    (void)hipFree(q);
  if (ctx->rad_ev) (void)hipEventDestroy(ctx->rad_ev);
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
  // ... and for the last ray query enqueued on a caller's stream (ykgpu_cast_rays_async)
  if (ctx->cast_ev) YK_HIP(hipEventSynchronize(ctx->cast_ev));
  // ... and for the last radiance query or gather (ykgpu_radiance_rays_async, ykgpu_gather_points_async)
  if (ctx->rad_ev) YK_HIP(hipEventSynchronize(ctx->rad_ev));
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
  // The slots of every wide node front to back from the camera, spanning leaves (the ground) last
  // (ykbvh::SlotOrder): both visits take the entered slots in descending index, so
  // this order is the traversal order.  It changes no result and not the stack's depth.  Same-box
  // A/B: bench 145.9 -> 142.8 ms, FP32 frame 190.1 -> 183.2 ms (profiles/r16_slot_order/).
  ykbvh::WideOptions wopt;
  wopt.view = camera->origin;
  if (const char* e = ab_knob("YKGPU_BVH_ORDER"))  // (A/B: 0 the binary tree's order, 1..3 a SlotOrder)
    wopt.order = (ykbvh::SlotOrder)std::max(0, std::min(3, std::atoi(e)));
  int rc = upload_tree(ctx, ctx->t64, centers, radii, cam_ext, bopt, kLeafCapF64, geo.data(), sizeof(SphereGeo),
                       sizeof(SphereGeo), k64, true, wopt);
  if (rc) return rc;
  // The FP64 visit's float distances assume neither overflow nor underflow.  With
  // B = origin_bound: the origin product o * (1/d), |1/d| < 1e30 < 2^100 (the kernel's own guard),
  // stays finite for B <= 2^27 (inf - inf would cull a box that holds the hit); and a scaled
  // distance 2^-24 t below float's normal range is off by up to 2^-126 absolutely, 2^-102 in t,
  // which the box growth's unused share delta |1/d| / 8 = 2^-24 B |1/d| covers with 2^18 to spare
  // for B >= 2^-60 max(1, D), D bounding the primary rays' direction components (secondary
  // directions have unit length).  A scene outside that scale renders FP64 with the linear scan.
  {
    double dmax = 1.0;
    for (int k = 0; k < 3; ++k)
      dmax = std::max(dmax, std::fabs(camera->lower_left_corner[k]) + std::fabs(camera->horizontal[k]) +
                                std::fabs(camera->vertical[k]) + std::fabs(camera->origin[k]) +
                                std::fabs(camera->lens_radius) *
                                    (std::fabs(camera->lens_u[k]) + std::fabs(camera->lens_v[k])));
    if (!(ctx->t64.origin_bound <= 0x1p27) || !(ctx->t64.origin_bound >= 0x1p-60 * dmax))
      ctx->t64.origin_bound = -1.0;
  }
  ykbvh::Options fopt = bopt;
  fopt.max_leaf = kLeafCapF32;  // the FP32 kernel's leaf loop is unrolled for two spheres
  if (const char* e = ab_knob("YKGPU_BVH_ALLAXES_F32")) fopt.all_axes = std::atoi(e) != 0;  // (A/B; on: neutral)
  fopt.radius_grow = 2.0 * (double)ykbvh::kF32Cone;
  fopt.f32_big = ab_knob("YKGPU_F32_NO_BIG") == nullptr;  // (A/B: the cone bound alone)
  const RenderKernel k32[2][2] = {{f32_kernel(false, 0), f32_kernel(true, 0)},
                                  {f32_kernel(false, 4), f32_kernel(true, 4)}};
  ykbvh::WideOptions fwopt = wopt;
  if (const char* e = ab_knob("YKGPU_BVH_ORDER_F32"))  // (A/B, as YKGPU_BVH_ORDER)
    fwopt.order = (ykbvh::SlotOrder)std::max(0, std::min(3, std::atoi(e)));
  rc = upload_tree(ctx, ctx->t32, centers, radii, cam_ext, fopt, kLeafCapF32, geo_f.data(), sizeof(float4),
                   sizeof(float4), k32, false, fwopt);
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
  // the sky-block classifier's view of the scene; its cached blocks are keyed by scene_gen
  ctx->sky_centers = centers;
  ctx->sky_radii = radii;
  // the ray queries' domain rule (include/ykgpu.h): E = max_i(max(|cx|, |cy|, |cz|) + |r|)
  double ext = 0;
  for (uint32_t i = 0; i < count; ++i) {
    const yk_sphere& s = spheres[i];
    const double e = std::fmax(std::fabs(s.center[0]), std::fmax(std::fabs(s.center[1]), std::fabs(s.center[2]))) +
                     std::fabs(s.radius);
    ext = e > ext || e != e ? e : ext;  // (a NaN stays: no ray is then in the domain)
    if (ext != ext) break;
  }
  ctx->cast_extent = ext;
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

int ykgpu_get_stats(ykgpu_context* ctx, yk_render_stats* out) {
  if (!ctx || !out) return fail(YK_ERR_INVALID, "null argument");
  YK_HIP(hipSetDevice(ctx->device));
  int rc = finish_stats(ctx);
  if (rc) return rc;
  *out = ctx->stats;
  return YK_OK;
}

}  // extern "C"
