// yk_host_internal.hpp — what more than one host unit of the library needs, defined once: the error
// slot and the YK_HIP macro, the structs behind the C-ABI's opaque handles (ykgpu_context,
// ykgpu_film, ykgpu_group, ykgpu_group_film) and the host functions that cross units (namespace ykhost).  Not part of
// the C-ABI, not installed.  Who defines what: yk_context.hip the error slot and the statistics,
// yk_pipeline.hip the parameter checks, the tile helpers, the processing order and launch(),
// yk_film.hip film_ready and the accumulate halves, yk_denoise.hip the steps of a group film's filter
// (yk_group_film.hpp in yk_group.hip runs them), yk_features.hip the feature pass, yk_cast.hpp the ray queries,
// yk_radiance.hpp the radiance queries.
#ifndef YK_HOST_INTERNAL_HPP
#define YK_HOST_INTERNAL_HPP

#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdint>
#include <map>
#include <string>
#include <vector>

#include "../../include/ykgpu.h"
#include "yk_render_device.hpp"
#include "yk_seed_table.hpp"

namespace ykhost {
// sets ykgpu_last_error's message for the calling thread and returns code
int fail(int code, const std::string& msg);
// that message (ykgpu_group_create and ykgpu_render_devices keep it across a clean-up)
std::string& last_error();
}  // namespace ykhost

#define YK_HIP(call)                                                                      \
  do {                                                                                    \
    hipError_t e_ = (call);                                                               \
    if (e_ != hipSuccess)                                                                 \
      return ykhost::fail(e_ == hipErrorOutOfMemory ? YK_ERR_NOMEM : YK_ERR_DEVICE,       \
                          std::string(#call) + ": " + hipGetErrorString(e_));             \
  } while (0)

// A BVH on the device: the FP64 kernel's (boxes grown for the exact test's rounding, DESIGN.md
// §4) or the FP32 kernel's (grown for render<float>'s sphere test, §4.1), with its LDS layout
// [nodes][leaf geometry][leaf ids][traversal stacks] and the persistent grid it leaves room for.
struct DevTree {
  DevNode* nodes = nullptr;
  void* leaf_geo = nullptr;      // SphereGeo (FP64) or float4 (FP32), in leaf order
  uint32_t* leaf_ids = nullptr;  // leaf slot → tuple index
  int32_t root = 0;              // root code (byte offset of the root node, or a leaf code)
  uint32_t depth = 0, n_nodes = 0;
  uint32_t wide_depth = 0;  // inner wide nodes on the longest root-to-leaf path
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

// counters of a synchronous ray query (yk_cast.hpp): rays, hits, out of domain, scan rays, node
// visits, sphere tests (8 words), in kCastStripes copies that the waves spread their atomics over
constexpr int kCastCounters = 8, kCastStripes = 64;
// ... and of a synchronous radiance query (yk_radiance.hpp): rays, out of domain, MT fallbacks,
// segments, words, scan segments, striped the same way; the fixed buffers of a query: the x_397 of
// a chunk's kRadChunk seeds and the claim counter
constexpr int kRadCounters = 8, kRadStripes = 64;
constexpr uint64_t kRadChunk = 1ull << 22;

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
  // Sky blocks (yk_sky.hpp): the scene on the host for the classifier, and for the
  // key — scene generation, image and tile geometry, block shape — the processing order over the
  // blocks that can hit something (the path pipeline's), the slots of the sky blocks
  // (yk_sky_samples'), that kernel's running sums (3 x sky_slots) and yk_sky_redo's list and
  // engines (a count, a word per sky slot, kSkyEngines x 624 words).  Built at most once per key
  // (ensure_sky).
  std::vector<double> sky_centers, sky_radii;
  std::vector<uint64_t> sky_key;
  uint32_t* d_sky_path = nullptr;
  uint32_t* d_sky_list = nullptr;
  double* d_sky_acc = nullptr;
  uint32_t* d_sky_mt = nullptr;
  uint32_t* d_sky_off = nullptr;  // a word per block: its place in its order (yk_sky_split)
  size_t sky_cap = 0;             // slots of the whole order the five buffers were allocated for
  uint32_t sky_path_slots = 0, sky_slots = 0, sky_full_slots = 0;
  hipEvent_t sky_ev = nullptr;  // the end of a call of sky blocks only (no reduce follows its samples)
  // Seed table (yk_seed_table.hpp): x_397 of every sample of the production
  // instance's tile, one word each, for one key (what the counter seeds depend on).  Only calls
  // with sky slots use it: the first such call of a key walks, the second consecutive one fills the
  // table beside its walks, in the calls after it the sky kernel reads it instead of walking.
  // seed_tab_filled: every launch of the fill call was enqueued.  seed_tab_part: the
  // sky split (sky_key; empty: no sky slots) of the last call that used the table, i.e. which words
  // the sky kernel touched and which the warm-up; a call under another split makes both streams
  // wait for both kernels of that call (seed_ev_aux after its last warm-up, seed_ev_red after its
  // last sky kernel; yk_pipeline.hip seed_table_wait).  Kept across ykgpu_set_scene; freed
  // when a call's rings need the room, and with the context.  seed_tab_on / seed_tab_max_bytes: the
  // switches yk_seed_table_configure sets (the Python package's YKGPU_SEED_TABLE=0 and
  // YKGPU_SEED_TABLE_MAX_MB, read when it creates the context).
  uint32_t* d_seed_tab = nullptr;
  uint64_t seed_tab_words = 0;
  ykseed::Key seed_tab_key{};
  // the key of the last call that could have used the table: a key is filled by its second
  // consecutive call, not its first (a caller that changes seed0 every call never pays a fill)
  ykseed::Key seed_tab_seen_key{};
  bool seed_tab_seen = false;
  bool seed_tab_filled = false, seed_ev_set = false;
  std::vector<uint64_t> seed_tab_part;
  hipEvent_t seed_ev_aux = nullptr, seed_ev_red = nullptr;
  bool seed_tab_on = true;
  uint64_t seed_tab_max_bytes = 8ull << 30;  // (the frame's table is 4.25 GB; config 5's 34 GB is not taken by default)
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
  // Ray queries (yk_cast.hpp): E = max_i(max |c_k| + |r|) of the scene (the domain rule of
  // include/ykgpu.h "ray queries"), the synchronous call's staging buffers (cast_cap rays and as
  // many hits), its counters and statistics, and the event after the last asynchronous cast
  double cast_extent = 0;
  void* d_cast_rays = nullptr;
  void* d_cast_hits = nullptr;
  size_t cast_cap = 0;
  unsigned long long* d_cast_counters = nullptr;
  hipEvent_t cast_ev = nullptr;
  yk_cast_stats cast_stats{};
  // Radiance queries (yk_radiance.hpp): the synchronous call's staging buffers (rad_cap rays and as
  // many records), the x_397 of a chunk's seeds, the path kernel's claim counter, its per-lane
  // scratch (624 engine words and rad_id_stride attenuation ids per resident lane, rad_lanes of
  // them), the counters and statistics, and the event after the last query (queries of a context
  // run one after the other: they share the scratch)
  void* d_rad_rays = nullptr;
  void* d_rad_out = nullptr;
  size_t rad_cap = 0;
  uint32_t* d_rad_x397 = nullptr;
  uint32_t* d_rad_claim = nullptr;
  uint32_t* d_rad_mt = nullptr;
  uint16_t* d_rad_ids = nullptr;
  size_t rad_lanes = 0, rad_id_stride = 0, rad_mt_lanes = 0;
  unsigned long long* d_rad_counters = nullptr;
  hipEvent_t rad_ev = nullptr;
  yk_radiance_stats rad_stats{};
  // Gather queries (yk_gather.hpp): the synchronous call's staging (gat_cap points and as many
  // records) and statistics; a chunk's rays and their records go through the radiance queries'
  // staging and scratch above, and rad_ev orders gathers and queries alike
  void* d_gat_points = nullptr;
  void* d_gat_out = nullptr;
  size_t gat_cap = 0;
  yk_gather_stats gat_stats{};
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
  // ykgpu_film_features' planes (yk_features.hip), allocated at the first pass, and their key: the
  // pinhole pass's grid or the sampled pass's n (yk_features_sampled.hpp), at most one of them not 0,
  // with the sampled pass's counts (yk_sampled_features_stats)
  void* d_features = nullptr;
  uint32_t feature_grid = 0;
  uint32_t feature_n = 0, feature_redo = 0;
  uint64_t feature_hits = 0;
  // ykgpu_film_mattes' table (yk_mattes.hpp), npix yk_matte_pixel records allocated at the first
  // pass, and its key: whether it holds a whole pass, that pass's n_samples (0: the film's own
  // counts, never reused) and its counts
  void* d_mattes = nullptr;
  bool matte_valid = false;
  uint32_t matte_n = 0;
  yk_matte_stats matte_stats{};
  bool uniform() const { return hist.size() <= 1; }
};

struct ykgpu_group {
  std::vector<ykgpu_context*> ctx;  // one per entry of the device list
  std::vector<uint8_t*> tile;       // each entry's RGB8 tile on its device
  std::vector<size_t> tile_cap;
  std::vector<yk_render_stats> st;  // the last render's, per entry
  yk_render_stats total{};          // ... and of the whole call
};

// A group film (include/ykgpu.h "group films"): per entry an ordinary film of the group render's
// sub-tile (null: the entry has no rows) and, for the filters, a band film: a film record without
// sample planes over the entry's band grown by the halo (yk_group_plan.hpp), which owns the
// band's denoise buffers and feature planes the way a film owns its own.
struct ykgpu_group_film {
  ykgpu_group* g = nullptr;
  yk_render_params p{};            // the whole tile's, with the seed key drawn at create
  uint32_t k = 0, wt = 0;
  std::vector<ykgpu_film*> film;   // per entry, the render side
  std::vector<uint32_t> rows;      // ... and its rows
  std::vector<uint64_t> gen;       // each context's scene generation at create
  std::vector<ykgpu_film*> band;   // per entry, the filter side, for `halo`
  uint32_t halo = 0;
  bool have_bands = false;
  bool torn = false;  // an entry's accumulate failed part-way (until a write)
};

// the render units' instances (yk_render_f64.hip, yk_render_f32.hip), by (scene in LDS, kMode).
// (Inline here, not in yk_pipeline.hip: KernelArgs lives in the anonymous namespace, so a function
// that returns a RenderKernel has internal linkage and cannot be declared across units.)
namespace {
inline RenderKernel fp64_kernel(bool lds, int mode) { return (RenderKernel)yk_fp64_kernel(lds, mode); }
inline RenderKernel f32_kernel(bool lds, int mode) { return (RenderKernel)yk_f32_kernel(lds, mode); }
}  // namespace

namespace ykhost {

// yk_pipeline.hip
int check_params(const ykgpu_context* ctx, const yk_render_params* p);
uint32_t tile_width(const yk_render_params* p);
uint64_t host_row_y(const yk_render_params* p, uint32_t t);
uint64_t host_col_x(const yk_render_params* p, uint32_t j);
uint32_t order_mode();
uint32_t order_stride(const yk_render_params* p);
std::vector<uint32_t> build_order(uint32_t W, uint32_t rows, uint32_t stride, uint32_t mode);
hipError_t create_render_stream(hipStream_t* s);
int launch(ykgpu_context* ctx, const yk_render_params* p, uint8_t* rgb_dev, double* sums_dev, hipStream_t st,
           uint32_t s_begin, uint32_t s_end, ykgpu_film* film);
// the sky blocks' device memory: both orders, the running sums, yk_sky_redo's list and engines
constexpr uint32_t kSkyEngines = 64;  // (one per thread of yk_sky_redo's block)
inline uint64_t sky_bytes(const ykgpu_context* ctx) {
  if (!ctx->sky_cap) return 0;
  const uint64_t full = ctx->sky_cap;  // (allocated for the whole tile, whatever the view flags)
  return (full + 256 + full + full / 64 + 1 + full + (uint64_t)kSkyEngines * ykd::kMtN) * sizeof(uint32_t) +
         full * 3 * sizeof(double);
}
// yk_context.hip
uint64_t device_bytes(const ykgpu_context* ctx);
int finish_stats(ykgpu_context* ctx);
// yk_film.hip: null or torn film: YK_ERR_INVALID with the last error set, like every film call
int film_ready(const ykgpu_film* film);
// ... and ykgpu_film_accumulate's two halves: the checks and the launches, then the wait, the
// statistics (total_ms counted from t0) and the film's new state
int film_accumulate_enqueue(ykgpu_film* film, uint32_t n_samples);
int film_accumulate_finish(ykgpu_film* film, uint32_t n_samples, std::chrono::steady_clock::time_point t0);
// yk_denoise.hip: the steps of a group film's filter.  The parameter checks of both filters;
int denoise_params_check(const yk_denoise_params& dp);
int feature_params_check(const yk_feature_params& fp);
// a film's denoise buffers, sized by its tile and allocated at first use: the m / v planes, the
// filtered mean, its RGB8 image and the counter of pixels whose count is below 2;
struct DenoiseBufs {
  double *mv, *out;
  uint8_t* rgb;
  unsigned long long* low;
};
int denoise_buffers(ykgpu_film* film, DenoiseBufs* out);
// yk_film_moments of the film into b.mv, enqueued on its context's stream (b.low is cleared first);
hipError_t denoise_moments_enqueue(ykgpu_film* film, const DenoiseBufs& b);
// the filter over the band film's whole tile, from b.mv into b.out, on its context's stream: the
// guided one when fp is given (feat: the band's feature planes), then the RGB8 image of the tile's
// rows [r0, r0 + n) when want_rgb.  The current device is the band's.
hipError_t denoise_band_enqueue(ykgpu_film* band, const DenoiseBufs& b, const yk_denoise_params& dp,
                                const yk_feature_params* fp, const double* feat, uint32_t r0, uint32_t n, bool want_rgb);
// yk_features.hip: the feature planes of the film at grid g (1..4) on the device, computed on the
// context's stream unless the film already holds them; *ms (may be null) receives the pass's device
// time, 0 when the cached planes were reused.  Synchronous.  YK_ERR_INVALID on a stale scene or a
// grid out of range.
int yk_film_features_ensure(ykgpu_film* film, uint32_t grid, const double** planes, double* ms);
// ... and from the first hits of the film's own first n samples (yk_features_sampled.hpp): the
// checks alone (n in 1..min(256, target), a stale scene: YK_ERR_INVALID), and the pass with them;
// *stats (may be null) receives the counts of the pass that made the planes, ms = 0 when they were
// reused.  Either kind of pass replaces the other's planes.
int yk_film_features_sampled_check(const ykgpu_film* film, uint32_t n_samples);
int yk_film_features_sampled_ensure(ykgpu_film* film, uint32_t n_samples, const double** planes,
                                    yk_sampled_features_stats* stats);
// the feature planes' F and U into the caller's pixel-major arrays (either may be null)
int yk_film_features_copy_out(ykgpu_film* film, const double* planes, double* mean_host, double* var_host);

// What the denoise and feature units derive from a film:
// its per-slot counts, null while the film is uniform (every count == done)
inline const uint32_t* film_counts(const ykgpu_film* film) { return film->uniform() ? nullptr : film->d_count; }
// the tile is image rows y0.. and image columns x0.. without gaps
// (both maps increase strictly, so the last entry tells whether any step was larger than one)
inline bool film_consecutive(const ykgpu_film* film) {
  const yk_render_params& p = film->p;
  return host_row_y(&p, p.row_count - 1) == (uint64_t)p.row_begin + p.row_count - 1 &&
         host_col_x(&p, tile_width(&p) - 1) == (uint64_t)p.col_begin + tile_width(&p) - 1;
}
// the tile's column set as the kernels take it: the whole width (col_count == 0) is 0, 1, 0
struct TileCols {
  uint32_t begin, stride, band;
};
inline TileCols film_cols(const ykgpu_film* film) {
  const yk_render_params& p = film->p;
  return p.col_count ? TileCols{p.col_begin, p.col_stride, p.col_band_log2} : TileCols{0, 1, 0};
}

}  // namespace ykhost

#endif
