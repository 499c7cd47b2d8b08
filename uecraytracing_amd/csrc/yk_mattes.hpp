// yk_mattes.hpp — film mattes (include/ykgpu.h "film mattes"): per pixel of a film's
// tile, which spheres the first hits of the pixel's own samples landed on and how many samples each
// got, and from that table antialiased coverage mattes of any set of ids without tracing again.
// The counts are integers, so tests/mattes_ref.py restates the table byte for byte.
//
// Part of the unit yk_features.hip: yk_features_sampled.hpp includes this file once at its end, and
// the pass is that file's per-sample loop (ykfs::sampled_block, ykfs::sampled_redo) with another
// sink: where the feature pass folds seven channels, MatteSink counts ids.  Kernels:
//   yk_film_mattes<Gen>     the sampled feature pass's mapping and start; the table of a pixel lives
//                           in registers (8 ids, 8 counts, three counters), searched and sorted with
//                           static indices only, and leaves as five 16-byte stores
//   yk_film_mattes_redo     the pixels whose lens loop outran the lazy words, from whole engines
//   yk_film_matte_counts    own-counts mode of a film whose counts differ: the counts from slot
//                           order into pixel order (a uniform film passes `done` instead)
//   yk_film_matte_coverage  one thread per pixel: the selected slots' counts over n; the ids sorted
//                           and deduplicated by the host, a binary search per slot in use
#ifndef YK_MATTES_HPP
#define YK_MATTES_HPP

namespace ykfs {
namespace {

constexpr uint32_t kMatteSlots = 8;
constexpr uint32_t kNoSlot = 0xffffffffu;  // a slot's id while it is unused (YK_MATTE_SKY's value)

static_assert(sizeof(yk_matte_pixel) == 80 && offsetof(yk_matte_pixel, count) == 32 && offsetof(yk_matte_pixel, n) == 64 &&
                  offsetof(yk_matte_pixel, used) == 76,
              "yk_matte_pixel");
static_assert(sizeof(yk_matte_stats) == 40 && offsetof(yk_matte_stats, samples) == 8 && offsetof(yk_matte_stats, hits) == 16 &&
                  offsetof(yk_matte_stats, other_samples) == 24 && offsetof(yk_matte_stats, overflow_pixels) == 32 &&
                  offsetof(yk_matte_stats, redo_pixels) == 36,
              "yk_matte_stats");
static_assert(sizeof(yk_matte_coverage_stats) == 32 && offsetof(yk_matte_coverage_stats, pixels_selected) == 8 &&
                  offsetof(yk_matte_coverage_stats, pixels_uncertain) == 16 &&
                  offsetof(yk_matte_coverage_stats, samples_selected) == 24,
              "yk_matte_coverage_stats");
static_assert(kNoSlot == YK_MATTE_SKY, "an unused slot reads as the sky's id");

// compare-exchange of two (count, id) keys: the larger count first, of equal counts the smaller id.
// The key is ~count above id, so an unused slot (count 0, id 0xffffffff) is the largest key of all.
__device__ __forceinline__ void matte_cx(uint64_t& a, uint64_t& b) {
  const uint64_t lo = a < b ? a : b, hi = a < b ? b : a;
  a = lo;
  b = hi;
}

// The table of one pixel, the sink of ykfs::sampled_block / sampled_redo.  Every index is a constant
// after unrolling, so the arrays are registers (a runtime index would send them to scratch).
struct MatteSink {
  uint32_t id[kMatteSlots], cnt[kMatteSlots];
  uint32_t n, miss, other, used;
  uint32_t sum_other, sum_over;  // of the pixels this lane stored: the wave's tally

  __device__ __forceinline__ void begin() { sum_other = sum_over = 0; }
  __device__ __forceinline__ void init() {
#pragma unroll
    for (uint32_t i = 0; i < kMatteSlots; ++i) {
      id[i] = kNoSlot;
      cnt[i] = 0;
    }
    n = miss = other = used = 0;
  }
  __device__ __forceinline__ uint32_t samples(const SfArgs& a, uint32_t at) {
    n = a.counts ? a.counts[at] : a.n;
    return n;
  }
  __device__ __forceinline__ void add(const SfArgs&, v3, v3, int hid, double) {
    if (hid < 0) {
      ++miss;
      return;
    }
    const uint32_t k = (uint32_t)hid;  // (never kNoSlot: a scene holds fewer spheres)
    bool held = false;
#pragma unroll
    for (uint32_t i = 0; i < kMatteSlots; ++i) {
      const bool here = id[i] == k;
      cnt[i] += here ? 1u : 0u;
      held = held || here;
    }
    if (held) return;
    if (used < kMatteSlots) {
#pragma unroll
      for (uint32_t i = 0; i < kMatteSlots; ++i) {
        const bool here = i == used;
        id[i] = here ? k : id[i];
        cnt[i] = here ? 1u : cnt[i];
      }
      ++used;
    } else {
      ++other;
    }
  }
  __device__ __forceinline__ void store(const SfArgs& a, size_t at) {
    uint64_t key[kMatteSlots];
#pragma unroll
    for (uint32_t i = 0; i < kMatteSlots; ++i) key[i] = ((uint64_t)~cnt[i] << 32) | id[i];
    // the 19 compare-exchanges of the optimal network for 8 keys (Knuth, TAOCP 3, 5.3.4)
    matte_cx(key[0], key[2]), matte_cx(key[1], key[3]), matte_cx(key[4], key[6]), matte_cx(key[5], key[7]);
    matte_cx(key[0], key[4]), matte_cx(key[1], key[5]), matte_cx(key[2], key[6]), matte_cx(key[3], key[7]);
    matte_cx(key[0], key[1]), matte_cx(key[2], key[3]), matte_cx(key[4], key[5]), matte_cx(key[6], key[7]);
    matte_cx(key[2], key[4]), matte_cx(key[3], key[5]);
    matte_cx(key[1], key[4]), matte_cx(key[3], key[6]);
    matte_cx(key[1], key[2]), matte_cx(key[3], key[4]), matte_cx(key[5], key[6]);
    uint32_t w[20];
#pragma unroll
    for (uint32_t i = 0; i < kMatteSlots; ++i) {
      w[i] = (uint32_t)key[i];
      w[kMatteSlots + i] = ~(uint32_t)(key[i] >> 32);
    }
    w[16] = n;
    w[17] = miss;
    w[18] = other;
    w[19] = used;
    uint4* out = reinterpret_cast<uint4*>(a.table + at);  // (80-byte records in hipMalloc'ed memory: 16-byte aligned)
#pragma unroll
    for (uint32_t i = 0; i < 5; ++i) out[i] = make_uint4(w[4 * i], w[4 * i + 1], w[4 * i + 2], w[4 * i + 3]);
    sum_other += other;
    sum_over += other ? 1u : 0u;
  }
  // one atomic per wave and counter (every lane of the wave is here)
  __device__ __forceinline__ void tally(const SfArgs& a, bool leader) {
    const uint32_t wo = ykquery::wave_sum(sum_other), wv = ykquery::wave_sum(sum_over);
    if (leader && wo) atomicAdd(a.tally, (unsigned long long)wo);
    if (leader && wv) atomicAdd(a.tally + 1, (unsigned long long)wv);
  }
};

template <class Gen>
__global__ __launch_bounds__(kThreads) void yk_film_mattes(SfArgs a) {
  sampled_block<Gen, MatteSink>(a);
}

__global__ __launch_bounds__(kRedoEngines) void yk_film_mattes_redo(SfArgs a) { sampled_redo<MatteSink>(a); }

// a film's counts live in slot order (d_order: slot -> pixel, 0xffffffff for padding)
__global__ __launch_bounds__(256) void yk_film_matte_counts(const uint32_t* count, const uint32_t* order, uint32_t* out,
                                                            uint32_t nps, uint32_t npix) {
  const uint32_t p = blockIdx.x * 256u + threadIdx.x;
  if (p >= nps) return;
  const uint32_t at = order[p];
  if (at < npix) out[at] = count[p];
}

struct CoverArgs {
  const yk_matte_pixel* table;
  const uint32_t* ids;  // ascending, no duplicates, the sky's id taken out
  double* cov;          // either may be null
  uint8_t* grey;
  unsigned long long* tally;  // pixels selected, pixels uncertain, samples selected
  uint32_t n_ids, sky, npix;
};

__global__ __launch_bounds__(256) void yk_film_matte_coverage(CoverArgs a) {
  const uint32_t at = blockIdx.x * 256u + threadIdx.x;
  uint32_t sel = 0, uncertain = 0;
  if (at < a.npix) {
    const uint4* rec = reinterpret_cast<const uint4*>(a.table + at);
    uint32_t w[20];
#pragma unroll
    for (uint32_t i = 0; i < 5; ++i) {
      const uint4 v = rec[i];
      w[4 * i] = v.x, w[4 * i + 1] = v.y, w[4 * i + 2] = v.z, w[4 * i + 3] = v.w;
    }
#pragma unroll
    for (uint32_t i = 0; i < kMatteSlots; ++i) {
      if (!w[kMatteSlots + i]) continue;  // (an unused slot)
      uint32_t lo = 0, hi = a.n_ids;      // the first id >= the slot's
      while (lo < hi) {
        const uint32_t mid = (lo + hi) / 2;
        if (a.ids[mid] < w[i])
          lo = mid + 1;
        else
          hi = mid;
      }
      if (lo < a.n_ids && a.ids[lo] == w[i]) sel += w[kMatteSlots + i];
    }
    if (a.sky) sel += w[17];
    uncertain = w[18] ? 1u : 0u;
    const double cov = w[16] == 0 ? 0.0 : film_div((double)sel, (double)w[16]);
    if (a.cov) a.cov[at] = cov;
    if (a.grey) {
      const double x = (cov < 0.0) ? 0.0 : (0.999 < cov) ? 0.999 : cov;
      a.grey[at] = (uint8_t)(int)film_mul(x, 256.0);
    }
  }
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t ws = ykquery::wave_sum(sel), wp = ykquery::wave_sum(sel ? 1u : 0u), wu = ykquery::wave_sum(uncertain);
  if (lane == 0 && wp) atomicAdd(a.tally, (unsigned long long)wp);
  if (lane == 0 && wu) atomicAdd(a.tally + 1, (unsigned long long)wu);
  if (lane == 0 && ws) atomicAdd(a.tally + 2, (unsigned long long)ws);
}

int mattes(ykgpu_film* film, uint32_t n_samples, yk_matte_pixel* table_host, yk_matte_stats* stats) {
  if (n_samples > film->p.samples_per_pixel)
    return fail(YK_ERR_INVALID, "mattes: n_samples is larger than the film's target");
  if (film->scene_gen != film->ctx->scene_gen)
    return fail(YK_ERR_INVALID, "the context's scene was set after the film was created");
  YK_HIP(hipSetDevice(film->device));
  const size_t npix = film->npix;
  if (!film->d_mattes) {  // (a film's tile never changes size)
    film->matte_valid = false;
    YK_HIP(hipMalloc(&film->d_mattes, npix * sizeof(yk_matte_pixel)));
  }
  yk_matte_stats st{};
  if (film->matte_valid && n_samples && film->matte_n == n_samples) {  // (ms = 0: the table is that pass's)
    st = film->matte_stats;
    st.ms = 0;
  } else {
    film->matte_valid = false;  // (until the pass is whole)
    // own counts: the film's `done` while they are all equal, else the counts in pixel order
    const bool own = n_samples == 0;
    uint32_t* d_counts = nullptr;
    if (own && !film->uniform()) YK_HIP(hipMalloc(&d_counts, npix * sizeof(uint32_t)));
    SfArgs a = film_args(film, own ? film->done : n_samples);
    a.table = (yk_matte_pixel*)film->d_mattes;
    a.counts = d_counts;
    for (const auto& h : film->hist) st.samples += own ? h.first * h.second : n_samples * h.second;
    PassBack back{};
    float ms = 0;
    const int rc = run_pass(film, a, "ykgpu_film_mattes", &back, &ms,
                            [&](const SfArgs& a, dim3 blocks, size_t lds, hipStream_t s, bool x128) {
                              if (d_counts)
                                hipLaunchKernelGGL(yk_film_matte_counts, dim3((film->nps + 255) / 256), dim3(256), 0, s,
                                                   film->d_count, film->d_order, d_counts, film->nps, a.npix);
                              if (x128)
                                hipLaunchKernelGGL(yk_film_mattes<ykd::X128Lane>, blocks, dim3(kThreads), lds, s, a);
                              else
                                hipLaunchKernelGGL(yk_film_mattes<ykd::MtLane>, blocks, dim3(kThreads), lds, s, a);
                              hipError_t e = hipGetLastError();
                              if (e == hipSuccess && !x128) {  // (almost always finds its list empty)
                                hipLaunchKernelGGL(yk_film_mattes_redo, dim3(1), dim3(kRedoEngines), 0, s, a);
                                e = hipGetLastError();
                              }
                              return e;
                            });
    (void)hipFree(d_counts);
    if (rc) return rc;
    st.ms = ms;
    st.hits = back.hits;
    st.other_samples = back.tally[0];
    st.overflow_pixels = (uint32_t)back.tally[1];
    st.redo_pixels = back.listed;
    film->matte_valid = true;
    film->matte_n = n_samples;
    film->matte_stats = st;
  }
  if (table_host) YK_HIP(hipMemcpy(table_host, film->d_mattes, npix * sizeof(yk_matte_pixel), hipMemcpyDeviceToHost));
  if (stats) *stats = st;
  return YK_OK;
}

int matte_coverage(ykgpu_film* film, const uint32_t* ids, uint32_t n_ids, double* cov_host, uint8_t* grey_host,
                   yk_matte_coverage_stats* stats) {
  if (!film->d_mattes || !film->matte_valid) return fail(YK_ERR_INVALID, "matte coverage: the film holds no matte table");
  if (n_ids == 0) return fail(YK_ERR_INVALID, "matte coverage: no ids");
  if (!ids) return fail(YK_ERR_INVALID, "matte coverage: null ids");
  if (!cov_host && !grey_host) return fail(YK_ERR_INVALID, "matte coverage: cov_host and grey_host are both null");
  std::vector<uint32_t> sorted;
  bool sky = false;
  for (uint32_t i = 0; i < n_ids; ++i) {
    if (ids[i] == YK_MATTE_SKY)
      sky = true;
    else if (ids[i] >= film->ctx->nspheres)
      return fail(YK_ERR_INVALID, "matte coverage: an id is neither a sphere's index nor YK_MATTE_SKY");
    else
      sorted.push_back(ids[i]);
  }
  std::sort(sorted.begin(), sorted.end());
  sorted.erase(std::unique(sorted.begin(), sorted.end()), sorted.end());
  YK_HIP(hipSetDevice(film->device));
  const hipStream_t stream = film->ctx->stream;
  const size_t npix = film->npix;
  // the call's own memory: the three counters, the ids, the two maps
  const size_t ids_at = 32, cov_at = ids_at + ((sorted.size() * sizeof(uint32_t) + 15) & ~(size_t)15),
               grey_at = cov_at + npix * sizeof(double);
  char* d_work = nullptr;
  YK_HIP(hipMalloc(&d_work, grey_at + npix));
  CoverArgs a{};
  a.table = (const yk_matte_pixel*)film->d_mattes;
  a.ids = (const uint32_t*)(d_work + ids_at);
  a.cov = cov_host ? (double*)(d_work + cov_at) : nullptr;
  a.grey = grey_host ? (uint8_t*)(d_work + grey_at) : nullptr;
  a.tally = (unsigned long long*)d_work;
  a.n_ids = (uint32_t)sorted.size();
  a.sky = sky ? 1u : 0u;
  a.npix = (uint32_t)npix;
  std::vector<double> cov(cov_host ? npix : 0);
  std::vector<uint8_t> grey(grey_host ? npix : 0);
  unsigned long long back[3] = {0, 0, 0};
  hipEvent_t ev[2] = {nullptr, nullptr};
  hipError_t e = hipEventCreate(&ev[0]);
  if (e == hipSuccess) e = hipEventCreate(&ev[1]);
  if (e == hipSuccess) e = hipMemsetAsync(d_work, 0, ids_at, stream);
  if (e == hipSuccess && !sorted.empty())
    e = hipMemcpyAsync(d_work + ids_at, sorted.data(), sorted.size() * sizeof(uint32_t), hipMemcpyHostToDevice, stream);
  if (e == hipSuccess) e = hipEventRecord(ev[0], stream);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(yk_film_matte_coverage, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, stream, a);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipEventRecord(ev[1], stream);
  if (e == hipSuccess) e = hipMemcpyAsync(back, d_work, sizeof(back), hipMemcpyDeviceToHost, stream);
  // (the caller's arrays are written only once the call cannot fail any more)
  if (e == hipSuccess && cov_host)
    e = hipMemcpyAsync(cov.data(), d_work + cov_at, npix * sizeof(double), hipMemcpyDeviceToHost, stream);
  if (e == hipSuccess && grey_host) e = hipMemcpyAsync(grey.data(), d_work + grey_at, npix, hipMemcpyDeviceToHost, stream);
  if (e == hipSuccess) e = hipStreamSynchronize(stream);
  float ms = 0;
  if (e == hipSuccess) e = hipEventElapsedTime(&ms, ev[0], ev[1]);
  for (hipEvent_t v : ev)
    if (v) (void)hipEventDestroy(v);
  (void)hipFree(d_work);
  if (e != hipSuccess)
    return fail(e == hipErrorOutOfMemory ? YK_ERR_NOMEM : YK_ERR_DEVICE,
                std::string("ykgpu_film_matte_coverage: ") + hipGetErrorString(e));
  if (cov_host) std::memcpy(cov_host, cov.data(), npix * sizeof(double));
  if (grey_host) std::memcpy(grey_host, grey.data(), npix);
  if (stats) {
    yk_matte_coverage_stats st{};
    st.ms = ms;
    st.pixels_selected = back[0];
    st.pixels_uncertain = back[1];
    st.samples_selected = back[2];
    *stats = st;
  }
  return YK_OK;
}

}  // namespace
}  // namespace ykfs

extern "C" {

int ykgpu_film_mattes(ykgpu_film* film, uint32_t n_samples, yk_matte_pixel* table_host, yk_matte_stats* stats) {
  if (int rc = film_ready(film)) return rc;
  return ykfs::mattes(film, n_samples, table_host, stats);
}

int ykgpu_film_matte_coverage(ykgpu_film* film, const uint32_t* ids, uint32_t n_ids, double* cov_host, uint8_t* grey_host,
                              yk_matte_coverage_stats* stats) {
  if (int rc = film_ready(film)) return rc;
  return ykfs::matte_coverage(film, ids, n_ids, cov_host, grey_host, stats);
}

}  // extern "C"

#endif
