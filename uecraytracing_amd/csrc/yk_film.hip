// yk_film.hip — the progressive film and its adaptive passes (include/ykgpu.h "progressive film",
// "adaptive passes"): the kernels that resolve a film, map its error and select and compact the
// pixels of a pass, and the entry points ykgpu_film_create … ykgpu_film_write_counts.  The folds
// of a launch into a film's planes (yk_film_reduce, yk_film_reduce_masked) are enqueued by
// launch() and live in yk_pipeline.hip; the denoise and feature passes are yk_denoise.hip and
// yk_features.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <map>
#include <random>
#include <string>
#include <vector>

#include "../../include/ykgpu.h"
#include "yk_film_internal.hpp"
#include "yk_host_internal.hpp"

using namespace ykhost;

// ---- progressive film (include/ykgpu.h) ------------------------------------------------------
// A film keeps, per processing slot p and channel c, the running sum s and the running second
// moment q as six planes plane[c * npix_slots + p] (s: c = 0..2, q: c = 3..5) — slot order, the
// order the launches' colours arrive in, so every access of the fold (yk_film_reduce,
// yk_pipeline.hip) is coalesced like yk_reduce_samples' — and its own copy of the slot → pixel order, so that neither the planes nor
// their meaning depend on what the context renders between two chunks.
// The arithmetic the host tests restate in numpy (film_add, film_sub, film_mul, film_div: each
// operation rounded on its own, never fused) is in yk_film_internal.hpp, shared with yk_denoise.hip.

namespace {

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

}  // namespace

// ---- progressive film (include/ykgpu.h "progressive film") ------------------------------------
int ykhost::film_ready(const ykgpu_film* film) {
  if (!film) return fail(YK_ERR_INVALID, "null film");
  if (film->torn) return fail(YK_ERR_INVALID, "the film's last accumulate failed part-way: restore it with ykgpu_film_write");
  return YK_OK;
}
// ykgpu_film_accumulate in two halves (a group film enqueues every entry's chunk before it waits
// for any): the checks and the launches on the context's stream ...
int ykhost::film_accumulate_enqueue(ykgpu_film* film, uint32_t n_samples) {
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
  film->torn = true;  // (until the chunk is whole)
  return launch(ctx, &film->p, nullptr, nullptr, ctx->stream, film->done, film->done + n_samples, film);
}
// ... and the wait, the statistics (total_ms from t0) and the film's new state
int ykhost::film_accumulate_finish(ykgpu_film* film, uint32_t n_samples, std::chrono::steady_clock::time_point t0) {
  ykgpu_context* ctx = film->ctx;
  YK_HIP(hipSetDevice(ctx->device));
  YK_HIP(hipStreamSynchronize(ctx->stream));
  int rc = finish_stats(ctx);
  if (rc) return rc;
  ctx->stats.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  film->done += n_samples;
  film->hist.clear();
  film->hist[film->done] = film->npix;
  film->torn = false;
  return YK_OK;
}
namespace {
uint32_t film_blocks(const ykgpu_film* film) { return std::max(1u, std::min((film->nps + 255) / 256, (uint32_t)film->ctx->cus * 8)); }
}  // namespace

extern "C" {

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
                  (void*)film->d_gmap, (void*)film->d_hist, film->d_denoise, film->d_features, film->d_mattes})
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
  const auto t0 = std::chrono::steady_clock::now();
  if (int rc = film_accumulate_enqueue(film, n_samples)) return rc;
  return film_accumulate_finish(film, n_samples, t0);
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

}  // extern "C"
