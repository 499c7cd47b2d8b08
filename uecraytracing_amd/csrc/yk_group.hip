// yk_group.hip — several devices in one process (include/ykgpu.h "several devices"): ykgpu_group_*
// and ykgpu_render_devices.
// One context per entry; rows dealt cyclically over the entries (tile row t of the call's row set
// → entry t mod k, uecraytracing_amd/tiles.py's dealing); every entry renders its tile into a
// device buffer on its own streams, and the tile is copied from its device straight into its rows
// of the caller's host image by one strided 2-D copy: the image ends on the host anyway (stb
// writes it), so a device-side gather first would only add a hop.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <limits>
#include <map>
#include <random>
#include <string>
#include <thread>
#include <vector>

#include "../../include/ykgpu.h"
#include "yk_group_plan.hpp"
#include "yk_host_internal.hpp"

using namespace ykhost;

namespace {
// an entry's statistics into the call's (ykgpu_group_get_stats, index -1): work summed, times the
// largest entry's; dev_extra and call_extra: the group's own buffers for that entry
void add_entry_stats(yk_render_stats& tot, const yk_render_stats& s, size_t dev_extra, size_t call_extra) {
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
  tot.device_bytes += s.device_bytes + dev_extra;
  tot.call_bytes += s.call_bytes + call_extra;
  tot.sclk_mhz = std::max(tot.sclk_mhz, s.sclk_mhz);
  // (ABI 11) the largest launch of any entry, and every entry's memory-pressure shrinks
  tot.launch_spp = std::max(tot.launch_spp, s.launch_spp);
  tot.mem_shrinks += s.mem_shrinks;
}
}  // namespace

extern "C" {

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
      const std::string msg = last_error();
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
    add_entry_stats(tot, c->stats, g->tile_cap[e], rows[e] * row_bytes);
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
    const std::string msg = last_error();
    ykgpu_group_destroy(g);
    last_error() = msg;
  }
  return rc;
}

}  // extern "C"

// group films (ykgpu_group_film_*): the unit's other half, in a file of its own
#include "yk_group_film.hpp"
