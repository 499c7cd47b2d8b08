// yk_features_sampled.hpp — the sampled feature pass (include/ykgpu.h "sampled film features",
// DESIGN.md §6.8): a film's 17 feature planes from the first hits of the film's own first n samples,
// so that a thin-lens render gets guides that are defocused where its colour is.  Every sample's
// start ray is yk_camera_sample_ray's bit for bit, its hit the ray queries' closest hit, and the
// channel rule and the folds are the pinhole pass's (yk_features.hip), one unfused IEEE double
// operation each, so numpy restates the planes byte for byte (tests/film_features_sampled_ref.py).
//
// Part of the unit yk_features.hip, which includes this file once at its end (the list of units is
// fixed, tests/test_build_knobs.py).  Everything but the C-ABI entry points lives in namespace ykfs.
// The per-sample loop is written once (sampled_block, sampled_redo) and takes a sink: the feature
// folds here, the id table of the film mattes in yk_mattes.hpp, included at this file's end.
// Two kernels on the context's stream, beside the render and not inside it:
//   yk_film_features_sampled<Gen>  one lane per pixel, a wave an 8 x 8 pixel block, the pixel's n
//                                  samples one after the other (the fold order is the definition's).
//                                  The start as yk_sky_samples makes it (yk_pipeline.hip): the seed
//                                  walk of four consecutive samples interleaved, the lazy cursors,
//                                  the lens rejection loop.  The closest hit is the ray queries'
//                                  (ykquery::closest_hit, yk_query.hpp) with t_max = +inf, the
//                                  ordered scan under YK_FLAG_LINEAR_SCAN.
//   yk_film_features_redo          the pixels whose lens loop outran the lazy cursors' words (listed
//                                  by the first kernel; ~55 rejections in a row, or a test's lowered
//                                  limit): all n samples again from a whole engine (ykd::MtFull), the
//                                  hit by the ordered scan (ykquery::scan_hit).  One block of
//                                  kRedoEngines threads.
#ifndef YK_FEATURES_SAMPLED_HPP
#define YK_FEATURES_SAMPLED_HPP

#include <atomic>
#include <cstring>
#include <string>
#include <type_traits>

#include "yk_film_internal.hpp"
#include "yk_query.hpp"

namespace ykfs {
using namespace ykhost;
namespace {

constexpr uint32_t kMaxSamples = 256;
// a workgroup: four waves side by side, each an 8 x 8 pixel block
constexpr uint32_t kWave = 8, kBlockW = 4 * kWave, kBlockH = kWave, kThreads = kBlockW * kBlockH;
constexpr uint32_t kWalk = 4;  // consecutive samples whose seed walks are interleaved
constexpr uint32_t kRedoEngines = 64;
constexpr uint32_t kLazyMin = 4;  // (the jitter's words: never checked)

static_assert(sizeof(yk_sampled_features_stats) == 32 && offsetof(yk_sampled_features_stats, samples) == 8 &&
                  offsetof(yk_sampled_features_stats, hits) == 16 &&
                  offsetof(yk_sampled_features_stats, redo_pixels) == 24,
              "yk_sampled_features_stats");

struct SfArgs {
  yk_camera cam;
  ykquery::QueryTree q;
  double* out;               // kYkFeatPlanes planes of npix doubles
  uint32_t* redo;            // [0]: pixels listed, [1, 1 + npix): the list, then kRedoEngines engines
  unsigned long long* hits;  // samples that hit a sphere
  // the film mattes' (yk_mattes.hpp): the table, the pixels' own sample counts in pixel order (null:
  // n for every pixel) and the counters of samples past the slots and of pixels that have some
  yk_matte_pixel* table;
  const uint32_t* counts;
  unsigned long long* tally;
  double t_min;
  uint64_t seed_key;
  uint32_t seed0, seed_mode, spp, n;
  uint32_t lazy_words;  // mt19937 words a start may draw from the lazy cursors (4..227)
  uint32_t scan_only;   // YK_FLAG_LINEAR_SCAN
  uint32_t W, H, rows, wt, npix;
  uint32_t row_begin, row_stride, row_band, col_begin, col_stride, col_band;
};

__device__ __forceinline__ uint32_t image_x(const SfArgs& a, uint32_t tj) {
  return a.col_begin + (((tj >> a.col_band) * a.col_stride) << a.col_band) + (tj & ((1u << a.col_band) - 1u));
}
__device__ __forceinline__ uint32_t image_y(const SfArgs& a, uint32_t ti) {
  return a.row_begin + (((ti >> a.row_band) * a.row_stride) << a.row_band) + (ti & ((1u << a.row_band) - 1u));
}

// yk_camera_sample_ray's ray (yk_host.cpp) from the start's draws, operation for operation: the
// jitter (source.cpp:160-164), camera::get_ray (camera.hpp:29-32) and the thin lens' offset
__device__ __forceinline__ void start_ray(const SfArgs& a, uint32_t x, uint32_t y, double uc, double vc, bool lens,
                                          double px, double py, v3& o, v3& d) {
  const double u = film_div(film_add((double)x, uc), (double)a.W);
  const double v = film_div(film_add((double)(a.H - y - 1), vc), (double)a.H);
  const v3 org = ld3(a.cam.origin);
  d = ykd::sub(ykd::add(ykd::add(ld3(a.cam.lower_left_corner), ykd::mul(ld3(a.cam.horizontal), u)),
                        ykd::mul(ld3(a.cam.vertical), v)),
               org);
  o = org;
  if (lens) {
    const double rx = px * a.cam.lens_radius, ry = py * a.cam.lens_radius;
    const v3 off = ykd::add(ykd::mul(ld3(a.cam.lens_u), rx), ykd::mul(ld3(a.cam.lens_v), ry));
    o = ykd::add(o, off);
    d = ykd::sub(d, off);
  }
}

// the channels of a sample from its hit (the pinhole pass's rule), folded into s and q
__device__ __forceinline__ void fold_sample(const SfArgs& a, v3 o, v3 d, int hid, double t, double (&s)[kYkFeatChannels],
                                            double (&q)[kYkFeatChannels]) {
  double f[kYkFeatChannels] = {1.0, 1.0, 1.0, 0.0, 0.0, 0.0, 0.0};
  if (hid >= 0) {
    const SphereMat& m = a.q.mat[hid];
    const v3 nrm = ykquery::hit_record(o, d, t, a.q.geo[hid], m.radius).nrm;
    if (m.kind != YK_MATERIAL_DIELECTRIC) {
      f[0] = m.ar;
      f[1] = m.ag;
      f[2] = m.ab;
    }
    f[3] = nrm.x;
    f[4] = nrm.y;
    f[5] = nrm.z;
    f[6] = t;
  }
#pragma unroll
  for (uint32_t c = 0; c < kYkFeatChannels; ++c) {
    s[c] = film_add(s[c], f[c]);
    q[c] = film_add(q[c], film_mul(f[c], f[c]));
  }
}

// F, U and the group sums of pixel `at` from the folds over n samples
__device__ __forceinline__ void store_planes(const SfArgs& a, size_t at, const double (&s)[kYkFeatChannels],
                                             const double (&q)[kYkFeatChannels]) {
  const double G = (double)a.n;
  const double den = film_mul(G, film_sub(G, 1.0));
  double U[kYkFeatChannels];
#pragma unroll
  for (uint32_t c = 0; c < kYkFeatChannels; ++c) {
    const double var = film_div(film_sub(q[c], film_div(film_mul(s[c], s[c]), G)), den);
    U[c] = a.n >= 2 && var > 0.0 ? var : 0.0;
    a.out[(size_t)c * a.npix + at] = film_div(s[c], G);
    a.out[(size_t)(kYkFeatChannels + c) * a.npix + at] = U[c];
  }
  a.out[(size_t)14 * a.npix + at] = film_add(film_add(U[0], U[1]), U[2]);
  a.out[(size_t)15 * a.npix + at] = film_add(film_add(U[3], U[4]), U[5]);
  a.out[(size_t)16 * a.npix + at] = U[6];
}

// whether the lens loop's next try (four words) stays inside the lazy cursors' words
__device__ __forceinline__ bool lens_try_ok(const ykd::MtLane& g, uint32_t lazy_words) { return g.j + 4 <= lazy_words; }
__device__ __forceinline__ bool lens_try_ok(const ykd::X128Lane&, uint32_t) { return true; }
template <class Gen>
__device__ __forceinline__ void walk(uint32_t (&x)[kWalk]) {
  if constexpr (std::is_same<Gen, ykd::MtLane>::value) ykd::mt_walk397xn<(int)kWalk>(x);
}

// The feature pass's sink of the per-sample loop below: the folds s and q of the seven channels
struct FeatureSink {
  double s[kYkFeatChannels], q[kYkFeatChannels];
  __device__ __forceinline__ void begin() {}
  __device__ __forceinline__ void init() {
#pragma unroll
    for (uint32_t c = 0; c < kYkFeatChannels; ++c) s[c] = q[c] = 0.0;
  }
  __device__ __forceinline__ uint32_t samples(const SfArgs& a, uint32_t) { return a.n; }
  __device__ __forceinline__ void add(const SfArgs& a, v3 o, v3 d, int hid, double t) { fold_sample(a, o, d, hid, t, s, q); }
  __device__ __forceinline__ void store(const SfArgs& a, size_t at) { store_planes(a, at, s, q); }
  __device__ __forceinline__ void tally(const SfArgs&, bool) {}
};

// The per-sample loop of the passes that read a film's own samples, written once: the sampled
// feature pass and the film mattes (yk_mattes.hpp) differ in the Sink that receives each sample's
// hit.  A sink says how many samples its pixel has (samples), takes them in order (add), writes the
// pixel (store) and adds what it counted to the pass's counters, once per wave (tally).
template <class Gen, class Sink>
__device__ __forceinline__ void sampled_block(const SfArgs& a) {
  extern __shared__ __attribute__((aligned(16))) int32_t fs_stack[];  // [entry][lane]: (stack_cap + 3) x kThreads
  const uint32_t tid = threadIdx.x;
  const uint32_t wave = tid / 64u, lane = tid & 63u;
  const uint32_t px = blockIdx.x * kBlockW + wave * kWave + (lane & (kWave - 1u));
  const uint32_t py = blockIdx.y * kBlockH + lane / kWave;
  const bool mine = py < a.rows && px < a.wt;
  uint32_t nh = 0;
  Sink sink;
  sink.begin();
  if (mine) {
    const uint32_t x = image_x(a, px), y = image_y(a, py);
    const bool lens = a.cam.lens_radius > 0;
    const uint32_t at = py * a.wt + px;
    sink.init();
    const uint32_t n = sink.samples(a, at);
    bool listed = false;
    for (uint32_t k = 0; k < n && !listed; k += kWalk) {
      uint32_t seed[kWalk], x397[kWalk];
#pragma unroll
      for (uint32_t j = 0; j < kWalk; ++j)  // (past n: walked, not used)
        x397[j] = seed[j] = ykd::sample_seed(a.seed_mode, a.seed_key, a.seed0, y, x, a.W, a.spp, k + j);
      walk<Gen>(x397);
#pragma unroll 1
      for (uint32_t j = 0; j < kWalk && k + j < n; ++j) {
        const uint32_t sj = j == 0 ? seed[0] : j == 1 ? seed[1] : j == 2 ? seed[2] : seed[3];
        const uint32_t xj = j == 0 ? x397[0] : j == 1 ? x397[1] : j == 2 ? x397[2] : x397[3];
        Gen g;
        ykd::engine_start(g, sj, xj);
        const double uc = ykd::canonical<true>(g);  // source.cpp:162
        const double vc = ykd::canonical<true>(g);  // source.cpp:163
        double lx = 0.0, ly = 0.0;
        if (lens) {
          for (;;) {  // random_in_unit_disk by rejection, x then y
            if (!lens_try_ok(g, a.lazy_words)) {
              listed = true;
              break;
            }
            lx = ykd::uniform<true>(g, -1, 1);
            ly = ykd::uniform<true>(g, -1, 1);
            if (lx * lx + ly * ly < 1.0) break;
          }
          if (listed) break;
        }
        v3 o, d;
        start_ray(a, x, y, uc, vc, lens, lx, ly, o, d);
        ykquery::Hit h = {0.0, -1, false, 0, 0};  // (outside the domain: a miss, and no arithmetic)
        if (ykquery::in_domain(o, d, a.t_min, INFINITY, a.q.extent))
          h = ykquery::closest_hit<kThreads>(a.q, fs_stack + tid, true, o, d, a.t_min, INFINITY, a.scan_only != 0, false);
        nh += h.id >= 0 ? 1u : 0u;
        sink.add(a, o, d, h.id, h.t);
      }
    }
    if (listed) {
      // the lens loop outran the lazy cursors: the pass's redo kernel runs the pixel's samples
      nh = 0;
      a.redo[1 + atomicAdd(a.redo, 1u)] = at;
    } else {
      sink.store(a, at);
    }
  }
  // one atomic per wave (every lane of the block is here)
  const uint32_t wh = ykquery::wave_sum(nh);
  if (lane == 0 && wh) atomicAdd(a.hits, (unsigned long long)wh);
  sink.tally(a, lane == 0);
}

// ... and its whole-engine form for the listed pixels: one block of kRedoEngines threads
template <class Sink>
__device__ __forceinline__ void sampled_redo(const SfArgs& a) {
  const uint32_t count = a.redo[0] < a.npix ? a.redo[0] : a.npix;
  ykd::MtFull g;
  g.st = a.redo + 1 + a.npix + (size_t)threadIdx.x * ykd::kMtN;
  uint32_t nh = 0;
  const bool lens = a.cam.lens_radius > 0;
  Sink sink;
  sink.begin();
  for (uint32_t e = threadIdx.x; e < count; e += kRedoEngines) {
    const uint32_t at = a.redo[1 + e];
    if (at >= a.npix) continue;  // (never)
    const uint32_t py = at / a.wt, px = at - py * a.wt;
    const uint32_t x = image_x(a, px), y = image_y(a, py);
    sink.init();
    const uint32_t n = sink.samples(a, at);
    for (uint32_t k = 0; k < n; ++k) {
      ykd::mt_full_seed(g, ykd::sample_seed(a.seed_mode, a.seed_key, a.seed0, y, x, a.W, a.spp, k));
      const double uc = ykd::canonical(g);
      const double vc = ykd::canonical(g);
      double lx = 0.0, ly = 0.0;
      if (lens) {
        do {
          lx = ykd::uniform(g, -1, 1);
          ly = ykd::uniform(g, -1, 1);
        } while (!(lx * lx + ly * ly < 1.0));
      }
      v3 o, d;
      start_ray(a, x, y, uc, vc, lens, lx, ly, o, d);
      ykquery::Hit h = {0.0, -1, false, 0, 0};
      if (ykquery::in_domain(o, d, a.t_min, INFINITY, a.q.extent))
        ykquery::scan_hit(a.q, o, d, ykd::len2(d), a.t_min, INFINITY, false, h);
      nh += h.id >= 0 ? 1u : 0u;
      sink.add(a, o, d, h.id, h.t);
    }
    sink.store(a, at);
  }
  const uint32_t wh = ykquery::wave_sum(nh);
  if (threadIdx.x == 0 && wh) atomicAdd(a.hits, (unsigned long long)wh);
  sink.tally(a, threadIdx.x == 0);
}

template <class Gen>
__global__ __launch_bounds__(kThreads) void yk_film_features_sampled(SfArgs a) {
  sampled_block<Gen, FeatureSink>(a);
}

__global__ __launch_bounds__(kRedoEngines) void yk_film_features_redo(SfArgs a) { sampled_redo<FeatureSink>(a); }

// the lazy-word limit of the next passes; 0: ykd::kLazyDraws (yk_features_sampled_lazy_words below)
std::atomic<uint32_t> g_lazy_words{0};

// n_samples against the film: 1..min(256, target)
int check_n(const ykgpu_film* film, uint32_t n) {
  if (n < 1 || n > kMaxSamples) return fail(YK_ERR_INVALID, "features: n_samples must be 1..256");
  if (n > film->p.samples_per_pixel) return fail(YK_ERR_INVALID, "features: n_samples is larger than the film's target");
  return YK_OK;
}

int check(const ykgpu_film* film, uint32_t n_samples) {
  if (int rc = check_n(film, n_samples)) return rc;
  if (film->scene_gen != film->ctx->scene_gen)
    return fail(YK_ERR_INVALID, "the context's scene was set after the film was created");
  return YK_OK;
}

// the arguments a pass over the film's tile shares (its outputs and work memory apart)
SfArgs film_args(const ykgpu_film* film, uint32_t n) {
  const ykgpu_context* ctx = film->ctx;
  const yk_render_params& p = film->p;
  SfArgs a{};
  a.cam = ctx->cam;
  a.q = ykquery::query_tree(ctx);
  a.t_min = p.t_min;
  a.seed_key = p.seed_key;
  a.seed0 = p.seed0;
  a.seed_mode = p.seed_mode == YK_SEED_RANDOM_DEVICE ? 1u : 0u;
  a.spp = p.samples_per_pixel;
  a.n = n;
  const uint32_t lw = g_lazy_words.load();
  a.lazy_words = lw ? std::max(kLazyMin, std::min(lw, ykd::kLazyDraws)) : ykd::kLazyDraws;
  a.scan_only = (p.flags & YK_FLAG_LINEAR_SCAN) ? 1u : 0u;
  a.W = p.image_width;
  a.H = p.image_height;
  a.rows = p.row_count;
  a.wt = tile_width(&p);
  a.npix = (uint32_t)((size_t)a.rows * a.wt);
  const TileCols cols = film_cols(film);
  a.row_begin = p.row_begin;
  a.row_stride = p.row_stride;
  a.row_band = p.row_band_log2;
  a.col_begin = cols.begin;
  a.col_stride = cols.stride;
  a.col_band = cols.band;
  return a;
}

// what a pass leaves in the head of its work memory: the counters and the redo list's count
struct PassBack {
  unsigned long long hits, tally[2], pad;
  uint32_t listed;
};
constexpr size_t kPassHead = offsetof(PassBack, listed);

// One pass on the context's stream, synchronous: the pass's own memory (the counters, the redo list
// and its engines), `launch(a, blocks, lds, stream, xor128)` between two events, the counters back.
template <class Launch>
int run_pass(const ykgpu_film* film, SfArgs& a, const char* who, PassBack* back, float* ms, Launch launch) {
  const hipStream_t stream = film->ctx->stream;  // (film calls are synchronous on it)
  const size_t redo_words = 1 + (size_t)a.npix + (size_t)kRedoEngines * ykd::kMtN;
  char* d_work = nullptr;
  YK_HIP(hipMalloc(&d_work, kPassHead + redo_words * sizeof(uint32_t)));
  a.hits = (unsigned long long*)d_work;
  a.tally = (unsigned long long*)(d_work + offsetof(PassBack, tally));
  a.redo = (uint32_t*)(d_work + kPassHead);
  hipEvent_t ev[2] = {nullptr, nullptr};
  hipError_t e = hipEventCreate(&ev[0]);
  if (e == hipSuccess) e = hipEventCreate(&ev[1]);
  if (e == hipSuccess) e = hipMemsetAsync(d_work, 0, kPassHead + sizeof(uint32_t), stream);  // the counters and the list's count
  if (e == hipSuccess) e = hipEventRecord(ev[0], stream);
  if (e == hipSuccess) {
    const dim3 blocks((a.wt + kBlockW - 1) / kBlockW, (a.rows + kBlockH - 1) / kBlockH);
    e = launch(a, blocks, ykquery::query_stack_lds(a.q.stack_cap, kThreads), stream, film->p.rng == YK_RNG_XOR128);
  }
  if (e == hipSuccess) e = hipEventRecord(ev[1], stream);
  if (e == hipSuccess) e = hipMemcpyAsync(back, d_work, kPassHead + sizeof(uint32_t), hipMemcpyDeviceToHost, stream);
  if (e == hipSuccess) e = hipStreamSynchronize(stream);
  if (e == hipSuccess) e = hipEventElapsedTime(ms, ev[0], ev[1]);
  for (hipEvent_t v : ev)
    if (v) (void)hipEventDestroy(v);
  (void)hipFree(d_work);
  if (e != hipSuccess)
    return fail(e == hipErrorOutOfMemory ? YK_ERR_NOMEM : YK_ERR_DEVICE, std::string(who) + ": " + hipGetErrorString(e));
  return YK_OK;
}

int ensure(ykgpu_film* film, uint32_t n, const double** planes, yk_sampled_features_stats* stats) {
  if (int rc = check(film, n)) return rc;
  YK_HIP(hipSetDevice(film->device));
  const size_t npix = (size_t)film->p.row_count * tile_width(&film->p);
  if (!film->d_features) {  // (a film's tile never changes size)
    film->feature_grid = film->feature_n = 0;
    YK_HIP(hipMalloc(&film->d_features, kYkFeatPlanes * npix * sizeof(double)));
  }
  *planes = (const double*)film->d_features;
  yk_sampled_features_stats st{};
  st.samples = (uint64_t)npix * n;
  if (film->feature_n == n) {  // (ms = 0: the cached pass)
    st.hits = film->feature_hits;
    st.redo_pixels = film->feature_redo;
    if (stats) *stats = st;
    return YK_OK;
  }
  film->feature_grid = film->feature_n = 0;  // (until the pass is whole)
  SfArgs a = film_args(film, n);
  a.out = (double*)film->d_features;
  PassBack back{};
  float ms = 0;
  if (int rc = run_pass(film, a, "ykgpu_film_features_sampled", &back, &ms,
                        [](const SfArgs& a, dim3 blocks, size_t lds, hipStream_t stream, bool x128) {
                          if (x128)
                            hipLaunchKernelGGL(yk_film_features_sampled<ykd::X128Lane>, blocks, dim3(kThreads), lds, stream, a);
                          else
                            hipLaunchKernelGGL(yk_film_features_sampled<ykd::MtLane>, blocks, dim3(kThreads), lds, stream, a);
                          hipError_t e = hipGetLastError();
                          if (e == hipSuccess && !x128) {  // (almost always finds its list empty)
                            hipLaunchKernelGGL(yk_film_features_redo, dim3(1), dim3(kRedoEngines), 0, stream, a);
                            e = hipGetLastError();
                          }
                          return e;
                        }))
    return rc;
  film->feature_n = n;
  film->feature_hits = back.hits;
  film->feature_redo = back.listed;
  st.ms = ms;
  st.hits = back.hits;
  st.redo_pixels = back.listed;
  if (stats) *stats = st;
  return YK_OK;
}

}  // namespace
}  // namespace ykfs

int ykhost::yk_film_features_sampled_check(const ykgpu_film* film, uint32_t n_samples) {
  return ykfs::check(film, n_samples);
}
int ykhost::yk_film_features_sampled_ensure(ykgpu_film* film, uint32_t n_samples, const double** planes,
                                            yk_sampled_features_stats* stats) {
  return ykfs::ensure(film, n_samples, planes, stats);
}

extern "C" {

// Lowers the words a start may draw from the lazy cursors for the passes that follow (clamped to
// 4..227; 0 restores the default), so that a test reaches yk_film_features_redo: 55 rejections in a
// row never happen on their own.  For the tests, like yk_schedule_plan: not part of the C-ABI
// (include/ykgpu.h does not declare it).
void yk_features_sampled_lazy_words(uint32_t words) { ykfs::g_lazy_words.store(words); }

int ykgpu_film_features_sampled(ykgpu_film* film, uint32_t n_samples, double* mean_host, double* var_host,
                                yk_sampled_features_stats* stats) {
  if (int rc = film_ready(film)) return rc;
  const double* planes = nullptr;
  yk_sampled_features_stats st{};
  if (int rc = yk_film_features_sampled_ensure(film, n_samples, &planes, &st)) return rc;
  if (int rc = yk_film_features_copy_out(film, planes, mean_host, var_host)) return rc;
  if (stats) *stats = st;
  return YK_OK;
}

}  // extern "C"

// ... and the film mattes (ykgpu_film_mattes ...), the same loop with a table of ids as its sink
#include "yk_mattes.hpp"

#endif
