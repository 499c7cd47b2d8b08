/*
 * ykgpu.h — C-ABI of the MI355X (gfx950) renderer for the per-pixel sampling loop of
 * yaito3014/UECRayTracing.  Plain C: no C++ or torch types cross this boundary.
 *
 * WHAT THIS REPLACES (reference file:line, /root/reference):
 *   - the render loop   source.cpp:122-172  (for_each over (row,col) → transform_reduce over
 *                       samples → image[y*W+x] = to_color3b(sum, spp))  → ykgpu_render*()
 *   - yk::render<T>()   source.cpp:98-178   (returns image_t = std::array<color3b, W*H>,
 *                       row-major, row 0 = top, RGB interleaved, stride 3W: source.cpp:70-71,
 *                       224-226) → the caller-owned uint8_t[W*rows*3] output
 *   - the world tuple   hittable_list.hpp:18-30 (objects in tuple order; the order defines
 *                       rec.id, tie-breaking and scatter dispatch, hittable_list.hpp:32-73)
 *                       → yk_sphere[] in the same order
 *   - camera<T>         camera.hpp:14-38 (public origin / lower_left_corner / horizontal /
 *                       vertical) → yk_camera
 *   - constants         source.cpp:57-66 (image_width, samples_per_pixel, max_depth),
 *                       t_min raytracer.hpp:27, seed source.cpp:118-120,154-159
 *                       → yk_render_params
 * The reference has no plugin/FFI layer of its own: these are the entry points a
 * C++ caller (our drop-in `raytrace`, or the reference's own source.cpp through
 * include/yk/ykgpu_bridge.hpp) binds.  See INTEGRATION.md.
 *
 * Conventions: every function returns YK_OK (0) or a YK_ERR_* code; the message of the last
 * failure on the calling thread is ykgpu_last_error().  No exceptions cross the ABI.  A context
 * owns one device's memory and stream; calls on one context are synchronous unless named
 * *_async and are NOT reentrant per context (the reference calls render() once from main).
 */
#ifndef YKGPU_H
#define YKGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define YKGPU_ABI_VERSION 11u

/* Material kinds.  LAMBERTIAN / METAL(fuzz == 0) are the reference's (material.hpp:37-69);
 * METAL with fuzz > 0 (reflected + fuzz * the reference's random_in_unit_sphere,
 * material.hpp:27-30) and DIELECTRIC are extensions needed by BASELINE configs 2-5.  The
 * reference has no code for them, but its integrator takes them: their images are pinned by
 * goldens rendered through the reference's ray_color / hittable_list / sphere / mt19937 with
 * these materials plugged in (oracle/ref_harness.cpp; only the scatter bodies are ours). */
enum { YK_MATERIAL_LAMBERTIAN = 0, YK_MATERIAL_METAL = 1, YK_MATERIAL_DIELECTRIC = 2 };

/* Arithmetic of the per-sample path (the T of yk::render<T>, source.cpp:98-99).
 * FP64 is render() as shipped (T = double), bit for bit.  FP32 is the same template with
 * T = float: geometry, camera, canonicals (generate_canonical<float> takes ONE 32-bit draw,
 * random.hpp:161-183) and math::sqrt in float; colours, attenuation and the per-pixel sum stay
 * double (raytracer<T, double>, lambertian<double>, source.cpp:100-111).  Sphere centres, radii
 * and camera vectors are the records' doubles rounded to float.  (As shipped, render<float>
 * does not compile — sphere's deduction guide rejects the double radius literals — so FP32 is
 * pinned against the reference's headers with the literals written as T(...): DESIGN.md §2.)
 * FP32 has its own BVH, whose boxes and per-ray cone carry the float sphere test's proven error
 * (DESIGN.md §4.1): its images equal the linear scan's bit for bit.
 * FP32 is a PARITY mode, not a speed mode: it reproduces render<float>'s images, and it is ~15%
 * SLOWER than FP64 on this chip (1920x1080x512: ~191 vs ~163 ms).  render<float>'s paths bounce
 * 7% more (its float sphere test), its tree needs the cone's extra plane read and wider boxes,
 * and the FP64 arithmetic the float path saves was not what bound the kernel.
 * Use FP64 (or xor128, the fast mode) for speed. */
enum { YK_PRECISION_FP64 = 0, YK_PRECISION_FP32 = 1 };

/* Per-sample engine (the Engine of source.cpp:155/159, seeded per sample as yk_render_params.
 * seed_mode says).  MT19937 = yk::mt19937 (random.hpp:148-151), render() as shipped.
 * XOR128 = the reference's other engine, yk::xor128 (random.hpp:18-41: Marsaglia's xorshift128,
 * x, y, z fixed, w = 88675123 ^ seed), swapped in for yk::mt19937: the fast mode.  Its state is
 * 4 words, so nothing needs the x_397 warm-up kernel.  (Consecutive counter seeds differ only in
 * w, so the first draws of neighbouring samples are correlated: that is the engine's, and the
 * image is the reference's with that engine, bit for bit.) */
enum { YK_RNG_MT19937 = 0, YK_RNG_XOR128 = 1 };

/* Per-sample seed of the mt19937 (yk_render_params.seed_mode).
 * COUNTER: seed0 + (y*W + x)*spp + s in uint32 arithmetic — the constexpr build
 *   (source.cpp:118-120,154-158); reproducible, the parity mode.
 * RANDOM_DEVICE: the runtime build seeds every sample from std::random_device (source.cpp:159).
 *   Here one 64-bit key per call (params.seed_key; 0 = draw it from std::random_device on the
 *   host, reported in yk_render_stats.seed_key) is hashed with the sample's linear index
 *   ((y*W + x)*spp + s, 64-bit): z = key + (idx+1)*0x9E3779B97F4A7C15, splitmix64 finaliser,
 *   seed = high 32 bits.  Independent seeds per sample like the reference's runtime build;
 *   reproducible when the key is given. */
enum { YK_SEED_COUNTER = 0, YK_SEED_RANDOM_DEVICE = 1 };

/* yk_render_params.flags */
enum {
  YK_FLAG_COUNT_WORK = 1u, /* count segments / sphere tests (ykgpu_get_stats)              */
  YK_FLAG_LINEAR_SCAN = 2u, /* closest hit by the reference's linear scan instead of the BVH
                              (same results; A/B and debugging)                              */
  YK_FLAG_ONE_LANE = 4u,    /* with COUNT_WORK, FP64 only (diagnostic): one lane per wave runs
                              paths, the other 63 idle.  The profiler's per-wave-instruction
                              counters (SQ_INSTS_VALU_FLOPS_FP64 ...) then read exactly the
                              instructions one lane executed: DESIGN.md §5 reconciliation   */
  YK_FLAG_TRACE_RAYS = 8u   /* internal to ykgpu_render_trace                                 */
};

enum {
  YK_OK = 0,
  YK_ERR_INVALID = 1,     /* bad argument (null pointer, zero size, row range outside image) */
  YK_ERR_DEVICE = 2,      /* HIP runtime failure / no device                                 */
  YK_ERR_NOMEM = 3,       /* device allocation failed                                        */
  YK_ERR_UNSUPPORTED = 4, /* a mode this build does not implement                            */
  YK_ERR_NO_SCENE = 5     /* render before ykgpu_set_scene                                   */
};

/* One sphere<T, M> of the world tuple (sphere.hpp:16-23), in tuple order. 80 bytes.
 * Every field is finite and the radius is not zero (math::sqrt need not end on a NaN or an
 * infinity); within that the kernels take every value as the reference's arithmetic does, pinned
 * bit for bit by tests/test_gpu_edge_materials.py:
 *   radius  may be negative for any material: the outward normal (p - c) / radius then points
 *           inwards, so the outside is the back face (a hollow shell inside a dielectric)
 *   albedo  any finite value: 0, above 1, negative and subnormal components are multiplied as
 *           they are.  (A pixel whose sum comes out negative is outside to_color3b's domain: the
 *           reference's math::sqrt need not end on a negative mean.)
 *   fuzz    any finite value, above 1 included; at or below 0 it means none (the reference's
 *           metal, no random draw).  It is tested as a double: a fuzz that is positive in double
 *           and 0 as a float still draws its four words under YK_PRECISION_FP32, as
 *           render<float> would, and adds nothing
 *   ior     any finite positive value, below 1 included (total internal reflection then happens
 *           on the front face) */
typedef struct yk_sphere {
  double center[3];
  double radius;    /* may be negative (any material; see above)                          */
  double albedo[3]; /* lambertian / metal albedo (material.hpp:39,57)                    */
  double fuzz;      /* metal only; <= 0: the reference's metal (no random draw)          */
  double ior;       /* dielectric only; > 0                                               */
  uint32_t material;/* YK_MATERIAL_*                                                      */
  uint32_t reserved;
} yk_sphere;

/* camera<T> public members (camera.hpp:34-37) plus the thin-lens basis of the defocus
 * extension.  lens_radius == 0 gives exactly the reference's get_ray (camera.hpp:29-32). */
typedef struct yk_camera {
  double origin[3];
  double lower_left_corner[3];
  double horizontal[3];
  double vertical[3];
  double lens_u[3];
  double lens_v[3];
  double lens_radius;
} yk_camera;

typedef struct yk_render_params {
  uint32_t image_width;       /* W  (constants::image_width, source.cpp:60)            */
  uint32_t image_height;      /* H  (source.cpp:61-62: uint32(W / (16/9)))             */
  uint32_t samples_per_pixel; /* spp (source.cpp:63)                                   */
  uint32_t max_depth;         /* source.cpp:64                                          */
  uint32_t seed0;             /* constexpr_seed (source.cpp:118-120); 404 = "00:00:00"  */
  uint32_t row_begin;         /* rendered rows: row_begin + i*row_stride, i < row_count */
  uint32_t row_count;         /*   (a tile of the image; the whole image: 0, H, 1), or   */
  uint32_t row_stride;        /*   in bands of 2^row_band_log2 rows (below)             */
  uint32_t precision;         /* YK_PRECISION_*                                         */
  uint32_t rng;               /* YK_RNG_*                                               */
  uint32_t flags;             /* YK_FLAG_*                                              */
  uint32_t seed_mode;         /* YK_SEED_*                                              */
  double t_min;               /* 0.001 in the reference (raytracer.hpp:27)              */
  uint64_t seed_key;          /* YK_SEED_RANDOM_DEVICE only (0: draw one per call)      */
  /* Banded row sets (the N-GPU split): with B = 2^row_band_log2, tile row i is image row
   * row_begin + (i / B) * row_stride * B + i % B — bands of B consecutive rows, every
   * row_stride-th band (rank k of N: row_begin = k*B, row_stride = N).  0: single rows.
   * Whole bands keep a wave's pixels adjacent in the image (coherent rays); DESIGN.md §7. */
  uint32_t row_band_log2;
  /* Column sets (ABI 10; the N-GPU split of uecraytracing_amd/tiles.py): col_count == 0 renders
   * every column (col_begin, col_stride and col_band_log2 must then be 0).  Otherwise, with
   * C = 2^col_band_log2, tile column j is image column col_begin + (j / C) * col_stride * C + j % C
   * — bands of C consecutive columns, every col_stride-th band — and the tile is
   * row_count x col_count pixels.  Seeds and the camera use the image position (y, x), so any
   * row and column set renders the image's own pixels.  Bands of 8 columns over every row keep a
   * rank's 8x8 processing blocks 8x8 in the image (coherent rays). */
  uint32_t col_begin;
  uint32_t col_count;
  uint32_t col_stride;
  uint32_t col_band_log2;
  uint32_t reserved0;
} yk_render_params;

typedef struct yk_render_stats {
  double kernel_ms;        /* path-tracing kernel, summed over its launches (HIP events on
                              the render streams around each launch; consecutive launches
                              overlap, so this can exceed the call)                      */
  double resolve_ms;       /* ordered per-pixel sum + to_color3b kernel, summed           */
  double total_ms;         /* whole call: host wall clock for ykgpu_render / _sums (with
                              the copies), first to last event for ykgpu_render_async   */
  double warmup_ms;        /* MT seed-walk kernel, summed over its launches (the fill call
                              of the seed table stores each walk's x_397 beside it)      */
  uint64_t samples;        /* primary samples rendered                                 */
  uint64_t segments;       /* ray_color calls that ran a closest-hit (flag COUNT_WORK) */
  uint64_t sphere_tests;   /* ray-sphere discriminant tests (flag COUNT_WORK)          */
  uint64_t sqrt_calls;     /* Newton square roots on hit candidates (flag COUNT_WORK)  */
  uint64_t mt_fallbacks;   /* samples that needed the full 624-word MT state           */
  uint64_t node_visits;    /* BVH inner nodes visited (flag COUNT_WORK)                */
  uint64_t linear_scans;   /* segments served by the exact linear scan (flag COUNT_WORK)*/
  uint64_t newton_calls;   /* math::sqrt evaluations (flag COUNT_WORK)                 */
  uint64_t newton_iters;   /* math::sqrt loop iterations (flag COUNT_WORK)             */
  uint64_t phase_cycles[8];/* diagnostic builds only (YK_ABLATE & 8): wave-cycles in refill,
                              sample start, traversal (interior nodes), candidates, shading,
                              path end, traversal (leaves), unused                        */
  uint64_t timeline[3];    /* diagnostic builds only: s_memrealtime (100 MHz) of the first wave start, of
                              the first refill that found no pixel left, of the last wave
                              exit (last launch of the call)                              */
  uint64_t diag[4];        /* diagnostic builds only: [0] leaf tests with disc >= 0       */
  uint64_t seed_key;       /* the key a YK_SEED_RANDOM_DEVICE render used (0 otherwise) */
  uint32_t launches;       /* path-tracing launches in the call                        */
  uint32_t grid_blocks;    /* persistent grid size                                     */
  double render_busy_ms;   /* union of the path-tracing launches' spans (wall time with at
                              least one launch running)                                 */
  uint64_t work[8];        /* flag COUNT_WORK (the flop and lane-op models):
                              FP64 only: [0] leaf tests with disc >= 0 (root bounds
                              computed), hits shaded as [1] lambertian, [2] metal, [3] of
                              them fuzzy, [4] dielectric; both precisions: [5] engine words
                              drawn by all samples, [6] of them by the seed-walk kernel
                              (the start's jitter and lens draws), [7] 624-word twists of
                              the full mt19937 state (samples past 227 words)            */
  uint64_t device_bytes;   /* device memory the context holds after the call: scene, BVHs,
                              processing order, start-record (xor128: colour) ring, running
                              sums, MT and attenuation scratch, the warm-ups' lens-retry rings,
                              the seed table (4 bytes per sample of the last FP64 / mt19937 /
                              counter-seed tile, kept across ykgpu_set_scene), output buffers
                              (DESIGN.md §6).
                              Buffers follow the calls: grown when a call needs more, given
                              back when it needs less than half                            */
  uint64_t call_bytes;     /* device memory THIS call needed (the same items sized to it):
                              1920x1080x512 FP64 ~19.1 GB; the 8-GPU split's tile of 3840x2160x1024
                              (480 columns) ~10.5 GB; 1920x1080x4096 (config 5) ~71 GB      */
  double sclk_mhz;         /* the shader clock the render launches ran at: s_memtime over
                              s_memrealtime (100 MHz) of one wave per launch, averaged      */
  uint32_t launch_spp;     /* samples per pixel of the call's largest launch (ABI 11)        */
  uint32_t mem_shrinks;    /* times the launch size was halved because the device could not
                              hold the rings (free memory short: slower, not an error; at
                              launches of 2^24 sample slots the call fails with NOMEM)      */
} yk_render_stats;

typedef struct ykgpu_context ykgpu_context;

uint32_t ykgpu_abi_version(void);
const char* ykgpu_last_error(void);

int ykgpu_device_count(int* count);
int ykgpu_context_create(int device, ykgpu_context** out);
int ykgpu_context_destroy(ykgpu_context* ctx);

/* Uploads the world (tuple order) and the camera to HBM.  Replaces building `world` and `cam`
 * inside render() (source.cpp:100-112).  Synchronous: first waits for the device (a render
 * still running from ykgpu_render_async reads the previous scene), then builds the BVHs on the
 * host and copies them with the spheres. */
int ykgpu_set_scene(ykgpu_context* ctx, const yk_sphere* spheres, uint32_t count,
                    const yk_camera* camera);

/* The render loop (source.cpp:122-172) for the rows (and columns) named by params, synchronous,
 * into a caller-owned host buffer of row_count * Wt * 3 bytes laid out like image_t, where the
 * tile width Wt is col_count, or W when col_count == 0. */
int ykgpu_render(ykgpu_context* ctx, const yk_render_params* params, uint8_t* rgb_host);

/* Same, into device memory (row_count * Wt * 3 bytes on ctx's device), ordered on `stream`
 * (a hipStream_t; NULL = the context's own stream): the writes to rgb_device come after the work
 * already queued on `stream`, and the image is complete for the work queued on `stream` after
 * the call.  Internally the kernels run on the context's own streams (render launches at the
 * device's top stream priority, the seed walks and the reduces below it) joined to `stream` by
 * events.  A call enqueued while this context's previous call still runs, with the same ring
 * geometry, overlaps it: its seed walks and renders start without waiting for `stream` (they
 * read only the scene and the context's own buffers) and only its last reduce, which writes
 * rgb_device, waits for `stream`.  YKGPU_OVERLAP=0 in the environment restores full ordering
 * (every kernel of the call after the work queued on `stream` and after the whole previous
 * call).  Does not synchronise. */
int ykgpu_render_async(ykgpu_context* ctx, const yk_render_params* params, void* rgb_device,
                       void* stream);

/* Diagnostics: the per-pixel colour sum before to_color3b (source.cpp:137-167), 3 doubles per
 * pixel, row_count * Wt * 3 doubles, host buffer. */
int ykgpu_render_sums(ykgpu_context* ctx, const yk_render_params* params, double* sums_host);

/* Verbose level 3 (raytracer.hpp:21-25: ray_color prints every ray it is called with, the one
 * reaching depth 0 included).  Renders the rows of params (COUNT_WORK instance) and records, for
 * every sample (index (row_t*Wt + col_t)*spp + s over the tile), the first max_rays rays of its path
 * as 6 doubles each (origin xyz, direction xyz; FP32 rays are floats widened exactly) into
 * rays_host[(index*max_rays + k)*6 ...] and the number of ray_color calls into counts_host[index]
 * (which may exceed max_rays).  row_count * Wt * spp * max_rays * 48 bytes of device memory are
 * used for the call, so callers render large images in row bands. */
int ykgpu_render_trace(ykgpu_context* ctx, const yk_render_params* params, uint32_t max_rays,
                       double* rays_host, uint32_t* counts_host);

/* Diagnostics: the device's math::sqrt (math.hpp:10-19) -- the routine every length, root and
 * to_color3b in the render uses -- on n host doubles (in and out may alias).  The tests check it
 * against the reference's loop. */
int ykgpu_math_sqrt(ykgpu_context* ctx, const double* in, double* out, uint64_t n);

/* Same for the FP32 path's math::sqrt<float> (loop in float, s / 2.0 and the halving in
 * double then rounded, exactly as math.hpp:10-19 reads for T = float) on n host floats. */
int ykgpu_math_sqrt_f32(ykgpu_context* ctx, const float* in, float* out, uint64_t n);

/* Diagnostics: the renderer's vector / scalar division (the normalisations and normals of
 * sphere.hpp / vec3.hpp) on n host triples: out3[3i+k] = num3[3i+k] / den[i].  It must equal
 * IEEE division bit for bit; the tests check it. */
int ykgpu_math_div(ykgpu_context* ctx, const double* num3, const double* den, double* out3, uint64_t n);
/* Diagnostic: the FP32 kernel's vector / scalar division (ykf::divs_fast: the compiler's float
 * division without its special-case steps, the reciprocal shared by the three components) on n
 * (3 numerators, denominator) pairs: out3 must equal num3 / den in IEEE float, bit for bit. */
int ykgpu_math_div_f32(ykgpu_context* ctx, const float* num3, const float* den, float* out3, uint64_t n);

/* Statistics of the last render on this context. */
int ykgpu_get_stats(ykgpu_context* ctx, yk_render_stats* out);

/* ---- several devices in one process (BASELINE config 4: the image row-tiled across the 8 GPUs
 * of a node) -------------------------------------------------------------------------------
 * The reference calls render() once from main (source.cpp:221) on one thread; a group lets that
 * one call use k devices.  A group holds one context per entry of `devices` (an entry may repeat:
 * {0, 0, 0} runs three contexts on device 0, which the tests use on one-GPU machines).  Rows of
 * the params' row set are dealt cyclically — tile row t goes to entry t mod k, the same dealing
 * as the torch.distributed bench (uecraytracing_amd/tiles.py) — every entry renders its tile with
 * ykgpu_render_async on its own streams, so the devices run concurrently, and each tile is
 * copied from its device straight into its rows of the caller's image (a strided 2-D copy: the
 * caller's image is on the host, so no device-side gather is needed before it).  Every row is
 * independent (source.cpp:154-158), so the image equals one device's byte for byte.
 * Row sets in bands (row_band_log2 > 0) are not dealt: YK_ERR_UNSUPPORTED when k > 1.
 * Not reentrant per group, like a context. */
typedef struct ykgpu_group ykgpu_group;

int ykgpu_group_create(const int* devices, uint32_t n_devices, ykgpu_group** out);
int ykgpu_group_destroy(ykgpu_group* group);
/* Number of entries (contexts) of the group. */
int ykgpu_group_size(const ykgpu_group* group, uint32_t* n);
/* ykgpu_set_scene on every entry (each device holds the scene and its BVHs in its own HBM). */
int ykgpu_group_set_scene(ykgpu_group* group, const yk_sphere* spheres, uint32_t count,
                          const yk_camera* camera);
/* The render loop over every entry; synchronous; rgb_host as for ykgpu_render
 * (row_count * tile width * 3 bytes, the rows of params in order).  The entries share the
 * params' column set; the rows are dealt. */
int ykgpu_group_render(ykgpu_group* group, const yk_render_params* params, uint8_t* rgb_host);
/* Statistics of the last group render: index < n the entry's own (its tile), index -1 the whole
 * call: samples and work counters summed over the entries, launches summed, kernel_ms /
 * render_busy_ms / warmup_ms / resolve_ms the largest entry's, total_ms the call's host wall
 * clock (copies included). */
int ykgpu_group_get_stats(ykgpu_group* group, int index, yk_render_stats* out);

/* One call for the whole drop-in: a group over `devices`, the scene, the render, the group
 * released (scene upload and BVH builds are inside the call). */
int ykgpu_render_devices(const int* devices, uint32_t n_devices, const yk_sphere* spheres,
                         uint32_t count, const yk_camera* camera, const yk_render_params* params,
                         uint8_t* rgb_host);

/* ---- progressive film: resumable accumulation with an error map ---------------------------
 * (Entry points added under ABI 11: nothing that existed changed size or meaning, so a caller
 * built against the earlier ABI 11 header keeps working; the version number stays.)
 *
 * A film is the device-resident accumulation state of one tile of one image: per pixel and
 * channel the running colour sum s_c (the left fold ((0 + c_0) + c_1) + ... of source.cpp:137-167)
 * and the running second moment q_c = q_c + (c*c) (product rounded to double, then the sum: no
 * fused multiply-add), 6 doubles per pixel.  It is filled by any sequence of sample chunks, can be
 * read at any point and can be saved and restored.
 *
 * ykgpu_film_create fixes, from params: the tile (rows, columns, bands), the mode (precision, rng,
 * seed mode, t_min, max_depth, YK_FLAG_LINEAR_SCAN; the diagnostic flags are dropped) and
 * samples_per_pixel, the film's TARGET.  The target stays the stride of the counter seed
 * seed0 + (y*W + x)*spp + s and of the RANDOM_DEVICE index, so sample s of a film is sample s of
 * the one-shot render with the same params: after any chunking the film's sums, and the image
 * resolved from them, equal ykgpu_render_sums / ykgpu_render bit for bit.  YK_SEED_RANDOM_DEVICE
 * with seed_key == 0 draws the key once, at create; every accumulate reports it in
 * yk_render_stats.seed_key, and ykgpu_film_params returns it.
 *
 * Film calls are synchronous.  A film owns its state (sums, second moments, its copy of the
 * processing order): other renders on its context between its calls, of any size or mode, do not
 * disturb it, nor it them; several films may share a context.  After ykgpu_set_scene on the
 * context a film's accumulate returns YK_ERR_INVALID (the scene generation it was created with
 * has passed).  A film must be destroyed before its context.  A film belongs to one context;
 * a device group has group films ("group films" below). */
typedef struct ykgpu_film ykgpu_film;

typedef struct yk_film_stats { /* 32 bytes */
  uint64_t pixels;             /* pixels of the tile                                      */
  uint64_t pixels_over;        /* those with e2 > threshold2                              */
  double max_e2;               /* the largest e2 of the tile                              */
  uint32_t samples_done;       /* samples per pixel accumulated so far                    */
  uint32_t samples_target;     /* params.samples_per_pixel                                */
} yk_film_stats;

int ykgpu_film_create(ykgpu_context* ctx, const yk_render_params* params, ykgpu_film** out);
int ykgpu_film_destroy(ykgpu_film* film);
/* The film's params as it keeps them (diagnostic flags dropped, the drawn seed_key filled in). */
int ykgpu_film_params(const ykgpu_film* film, yk_render_params* out);
/* Renders samples [done, done + n_samples) of every pixel and folds them, in sample order, into
 * the film.  n_samples == 0 or done + n_samples > target: YK_ERR_INVALID, nothing changes.
 * ykgpu_get_stats on the context then describes this chunk. */
int ykgpu_film_accumulate(ykgpu_film* film, uint32_t n_samples);
/* to_color3b (source.cpp:73-83) of the sums with the divisor `done` (/done, math::sqrt, clamp,
 * *256, truncate) into row_count * Wt * 3 host bytes; legal at any done >= 1. */
int ykgpu_film_resolve(ykgpu_film* film, uint8_t* rgb_host);
/* The state: sums and sumsq are row_count * Wt * 3 host doubles each, laid out like
 * ykgpu_render_sums (either may be NULL), *done the samples accumulated (may be NULL). */
int ykgpu_film_read(ykgpu_film* film, double* sums, double* sumsq, uint32_t* done);
/* Restores a state read earlier (checkpoint / resume); done <= target.  The caller vouches that
 * the state belongs to these params and this scene (yk_film_load returns both to compare). */
int ykgpu_film_write(ykgpu_film* film, const double* sums, const double* sumsq, uint32_t done);
/* The error map, done >= 2.  With n = (double)done, per pixel and channel
 *   v_c = (q_c - (s_c*s_c)/n) / (n*(n-1)),   e2 = max(0, v_r, v_g, v_b)
 * every operation IEEE double in exactly that order, uncontracted: the squared standard error of
 * the pixel mean, worst channel (no square root, so e2 > threshold2 is exact).  e2_host (NULL:
 * not wanted) receives row_count * Wt doubles; stats (NULL: not wanted) the count and the
 * maximum, which do not depend on the order of the reduction. */
int ykgpu_film_error(ykgpu_film* film, double threshold2, double* e2_host, yk_film_stats* stats);

/* Film files (host only, no device): a 32-byte header ("ykfilm1\0", the record sizes, done, the
 * pixel count, scene_hash), the yk_render_params record, then the sums and the second moments as
 * raw little-endian doubles (they round-trip exactly).  The pixel count is the params' tile,
 * row_count * Wt.  yk_film_load with sums == NULL and sumsq == NULL reads the header only;
 * otherwise capacity_pixels must hold the tile.  Truncated or foreign files: YK_ERR_INVALID. */
int yk_film_save(const char* path, const yk_render_params* params, uint64_t scene_hash, uint32_t done,
                 const double* sums, const double* sumsq);
int yk_film_load(const char* path, yk_render_params* params, uint64_t* scene_hash, uint32_t* done,
                 double* sums, double* sumsq, uint64_t capacity_pixels);
/* FNV-1a (64 bit) over every field of the spheres (tuple order; `reserved` excluded) and of the
 * camera, as their bit patterns: the scene a saved film belongs to. */
uint64_t yk_scene_hash(const yk_sphere* spheres, uint32_t count, const yk_camera* camera);

/* ---- adaptive passes: sample only the pixels still over the error bound ---------------------
 * (Added under ABI 11 like the film: nothing that existed changed size or meaning.)
 *
 * A film keeps a sample count per pixel (zero at create).  While all counts are equal the film is
 * UNIFORM and every call above behaves as described there.  ykgpu_film_accumulate_adaptive gives
 * samples only to the pixels that still need them, so counts may differ afterwards.
 *
 * Selection, on the state before the pass: pixel p with count n_p is selected iff
 *   n_p < target  and  (n_p < 2  or  e2_p > threshold2)
 * e2_p being ykgpu_film_error's formula with n = (double)n_p.  The comparison is strict.  e2 >= 0,
 * so threshold2 < 0 selects every unfinished pixel (on a fresh film: a uniform chunk).  A selected
 * pixel receives take_p = min(n_samples, target - n_p) samples: samples [n_p, n_p + take_p) of the
 * one-shot render (same seeds), folded in sample order.  So every pixel always holds exactly the
 * first n_p terms of the one-shot render's fold, bit for bit.
 *
 * n_samples == 0 or a stale scene: YK_ERR_INVALID.  Nothing selected: YK_OK, a zero pass (but for
 * min/max_count) and no launch.  ykgpu_get_stats then describes the whole pass: samples ==
 * samples_added, launches and times summed over the groups (all zero for an empty pass).
 *
 * On a non-uniform film: ykgpu_film_accumulate returns YK_ERR_INVALID; ykgpu_film_read's *done and
 * yk_film_stats.samples_done are the smallest count; ykgpu_film_resolve divides each pixel by its
 * own count (count 0: black); ykgpu_film_error uses each pixel's own count, and a count below 2
 * gives e2 = +inf (over any threshold, max_e2 = inf); ykgpu_film_write makes the film uniform. */
typedef struct yk_film_pass {   /* 32 bytes */
  uint64_t pixels_selected;     /* pixels that received samples in this pass            */
  uint64_t samples_added;       /* sum over them of the samples each received           */
  uint32_t groups;              /* distinct (count, take) groups rendered               */
  uint32_t launches;            /* path-tracing launches, summed over the groups        */
  uint32_t min_count, max_count;/* over the tile's pixels, after the pass               */
} yk_film_pass;

int ykgpu_film_accumulate_adaptive(ykgpu_film* film, double threshold2, uint32_t n_samples, yk_film_pass* out);
/* The counts: row_count * Wt host words in pixel order (NULL: not wanted), and their extremes. */
int ykgpu_film_counts(ykgpu_film* film, uint32_t* counts_host, uint32_t* min_count, uint32_t* max_count);
/* ykgpu_film_write with a count per pixel (each <= target). */
int ykgpu_film_write_counts(ykgpu_film* film, const double* sums, const double* sumsq, const uint32_t* counts);
/* "ykfilm2\0" files: the v1 header (done = the smallest count) and params record, then the counts
 * (uint32, little-endian), the sums and the second moments.  yk_film_load reads v1 only;
 * yk_film_load_counts reads v2, and v1 with every count equal to the header's done.  A count above
 * the target, a wrong pixel count, truncated or foreign files: YK_ERR_INVALID. */
int yk_film_save_counts(const char* path, const yk_render_params* params, uint64_t scene_hash,
                        const uint32_t* counts, const double* sums, const double* sumsq);
int yk_film_load_counts(const char* path, yk_render_params* params, uint64_t* scene_hash, uint32_t* counts,
                        double* sums, double* sumsq, uint64_t capacity_pixels);

/* ---- film denoise: a variance-guided non-local-means filter, defined exactly -----------------
 * (Added under ABI 11 like the film: nothing that existed changed size or meaning.)
 *
 * The film's tile is a grid of row_count x Wt pixels; the filter runs on that grid and never looks
 * outside it.  Pixel p = (i, j) with count n, sums s_c and second moments q_c has, with nd = (double)n,
 *   m_c = s_c / nd
 *   v_c = max(0, (q_c - (s_c*s_c)/nd) / (nd*(nd - 1)))            (ykgpu_film_error's v_c; v > 0 ? v : 0)
 * Window offsets d run row-major, dy = -R..R outside, dx inside.  For each d with q = p + d inside the tile:
 *   S = 0
 *   for o row-major over the patch (oy = -F..F outside, ox inside):
 *     p' = clamp(p + o), q' = clamp(q + o)                         (each coordinate clamped to the tile)
 *     for c in r, g, b:
 *       d   = m_c(p') - m_c(q')
 *       t_c = ((d*d) - alpha*(v_c(p') + min(v_c(q'), v_c(p')))) / (eps + k2*(v_c(p') + v_c(q')))
 *     S = S + ((t_r + t_g) + t_b)
 *   D = S / (double)(3*(2F+1)^2);  D = D > 0 ? D : 0
 *   t = 1 - 0.25*D;  t = t > 0 ? t : 0
 *   w = (t*t)*(t*t)                                                (compact stand-in for exp(-D))
 *   acc_c = acc_c + (w * m_c(q));  wsum = wsum + w
 * out_c(p) = acc_c / wsum.  Every + - * / is one IEEE double operation, rounded on its own and never
 * fused, in exactly that order, so numpy reproduces the result bit for bit.  The centre term has D = 0
 * and w = 1, so wsum >= 1; radius 0 returns m.  The RGB8 image is ykgpu_film_resolve's steps after its
 * division applied to out_c (math::sqrt, clamp to [0, 0.999], *256, truncate).
 *
 * ykgpu_film_denoise is synchronous and only reads the film: sums, second moments and counts stay as
 * they are.  It works on uniform and on adaptive (non-uniform) films, each pixel using its own count.
 * The buffers it needs (9 doubles and 3 bytes per pixel) are allocated at the film's first denoise and
 * freed with the film.  Errors, with nothing written to mean_host / rgb_host / stats:
 *   YK_ERR_INVALID      a parameter out of range (radius > 10, patch > 3, k2 <= 0, alpha < 0, eps <= 0)
 *                       or not finite; mean_host and rgb_host both NULL; any pixel's count below 2
 *   YK_ERR_UNSUPPORTED  the tile is not consecutive image rows and consecutive image columns (a strided
 *                       tile has no neighbours to filter over) */
typedef struct yk_denoise_params { /* 32 bytes */
  uint32_t radius;                 /* R, 0..10: the window is (2R+1)^2 neighbours    */
  uint32_t patch;                  /* F, 0..3: patches of (2F+1)^2 pixels            */
  double k2;                       /* > 0: the distance's variance scale             */
  double alpha;                    /* >= 0: the variance cancellation                */
  double eps;                      /* > 0: keeps the division defined at v = 0       */
} yk_denoise_params;

typedef struct yk_denoise_stats {  /* 24 bytes */
  double moments_ms;               /* the gather of m and v (device)                 */
  double filter_ms;                /* the filter and the RGB8 conversion (device)    */
  double total_ms;                 /* the call's host wall clock, copies included    */
} yk_denoise_stats;

/* radius 5, patch 1, k2 0.5, alpha 1.0, eps 1e-10 (host only) */
int yk_denoise_defaults(yk_denoise_params* out);
/* params NULL: the defaults.  mean_host: row_count * Wt * 3 doubles, pixel order (may be NULL);
 * rgb_host: row_count * Wt * 3 bytes (may be NULL); stats may be NULL. */
int ykgpu_film_denoise(ykgpu_film* film, const yk_denoise_params* params, double* mean_host, uint8_t* rgb_host,
                       yk_denoise_stats* stats);

/* ---- film features: first-hit albedo, normal and depth, and a filter guided by them ----------
 * (Added under ABI 11 like the film: nothing that existed changed size or meaning.)
 *
 * The feature pass makes seven channels per pixel of the film's tile from the scene and camera the
 * film was created with.  It is deterministic and draws no random numbers.  For image pixel (x, y)
 * (the tile's row and column sets map tile to image exactly as the render does) and a grid g in 1..4,
 * the sub-rays (i, j) run row-major, i = 0..g-1 outside and j inside:
 *   a = ((double)j + 0.5) / (double)g          b = ((double)i + 0.5) / (double)g
 *   u = ((double)x + a) / (double)W            v = ((double)(H - y - 1) + b) / (double)H
 *   o = origin,  d = ((lower_left_corner + horizontal*u) + vertical*v) - origin
 * That is the camera's pinhole ray: THE LENS IS IGNORED even when lens_radius > 0, so the features
 * are sharp where the colour is defocused (a guided filter keeps edges the defocus has blurred;
 * "sampled film features" below makes the planes from the render's own lens samples instead).
 * The closest hit is the reference's ordered scan over the spheres in tuple order, always in
 * double whatever the film's precision (features are guides, not the reference's arithmetic), with
 * t_min = params.t_min and t_max = +inf.  Per sphere (centre c, radius r), closest = t_max at first:
 *   oc = o - c;  a = (d.x*d.x + d.y*d.y) + d.z*d.z;  half_b = (oc.x*d.x + oc.y*d.y) + oc.z*d.z
 *   cc = ((oc.x*oc.x + oc.y*oc.y) + oc.z*oc.z) - r*r;  disc = half_b*half_b - a*cc;  disc < 0: no hit
 *   sq = math::sqrt(disc);  root = (-half_b - sq) / a
 *   if (root < t_min || closest < root) { root = (-half_b + sq) / a;  the same test: no hit }
 *   closest = root, the sphere is the hit (so of equal roots the later index wins)
 * and of the last accepted sphere k:  p = o + d*t,  outward = (p - c) / r,
 * normal = dot(d, outward) < 0 ? outward : -outward.  The channels of a sub-ray:
 *   f0..f2  the sphere's albedo (lambertian, metal) or (1, 1, 1) (dielectric);  a miss: (1, 1, 1)
 *   f3..f5  normal;                                                             a miss: (0, 0, 0)
 *   f6      t;                                                                  a miss: 0
 * Per channel, left folds over the sub-rays: s = s + f, q = q + (f*f).  With G = (double)(g*g):
 *   F = s / G                                                     the mean
 *   U = max(0, (q - (s*s)/G) / (G*(G - 1)))   (g = 1: U = 0)      the variance of the mean
 * Every + - * / is one IEEE double operation, rounded on its own and never fused, in that order.
 *
 * ykgpu_film_features computes the pass once per (film, grid) into planes the film owns (17 doubles
 * per pixel: F, U and three sums of U; allocated at first use, freed with the film; a later call
 * with the same grid reuses them and reports ms = 0, another grid replaces them) and copies out
 *   mean_host, var_host   row_count * Wt * 7 doubles each, pixel order (either may be NULL; both
 *                         NULL: compute and cache only);  ms may be NULL.
 * It works on any tile, strided ones included, and changes nothing of the film's state.
 *   YK_ERR_INVALID   grid outside 1..4; the context's scene was set after the film was created
 *
 * The guided filter is "film denoise" above with the weight w = min(wf, wc): wc is exactly that
 * section's w for the given yk_denoise_params, and for the same window offset and in-tile neighbour
 * q the feature weight is pointwise (no patch), over the groups A = channels 0..2, N = 3..5, Z = 6:
 *   V_k(x) = U(x) summed over the group's channels, left to right
 *   E_k    = (dF*dF) summed over the group's channels, left to right,   dF = F(p) - F(q)
 *   Phi_k  = (E_k - alpha_f*(V_k(p) + min(V_k(q), V_k(p)))) / (tau_k + k2_f*(V_k(p) + V_k(q)))
 *   DF     = max(max(max(0, Phi_A), Phi_N), Phi_Z)                 (x > y ? x : y; min: q < p ? q : p)
 *   tf = 1 - 0.25*DF;  tf = tf > 0 ? tf : 0;  wf = (tf*tf)*(tf*tf)
 *   w  = wf < wc ? wf : wc
 * then acc_c = acc_c + (w * m_c(q)), wsum = wsum + w and out_c = acc_c / wsum as before.  The centre
 * has Phi <= 0, so wf = 1 and wsum >= 1.  tau_k = +inf switches a group off; with all three infinite
 * the result is ykgpu_film_denoise's bit for bit.  ykgpu_film_denoise_guided is synchronous and only
 * reads the film; it computes the feature pass at feat->grid first unless the film holds it.
 * Errors, with nothing written to mean_host / rgb_host / stats:
 *   YK_ERR_INVALID      a colour parameter out of "film denoise"'s ranges; grid outside 1..4,
 *                       reserved != 0, k2_f <= 0 or not finite, alpha_f < 0 or not finite, a tau <= 0
 *                       or NaN; a stale scene; any pixel's count below 2; both outputs NULL
 *   YK_ERR_UNSUPPORTED  the tile is not consecutive image rows and consecutive image columns
 *
 * raytrace --aov writes F as three PNGs, each step one IEEE double operation:
 *   albedo  trunc(clamp(F_c, 0, 0.999) * 256), c = 0..2
 *   normal  trunc(clamp(0.5*F_c + 0.5, 0, 0.999) * 256), c = 3..5
 *   depth   trunc(clamp(F_6 / (1 + F_6), 0, 0.999) * 256), grey */
typedef struct yk_feature_params { /* 48 bytes */
  uint32_t grid;                   /* g, 1..4                                        */
  uint32_t reserved;               /* 0                                              */
  double k2, alpha;                /* k2_f > 0, alpha_f >= 0                         */
  double tau_albedo, tau_normal, tau_depth; /* > 0, +inf allowed                     */
} yk_feature_params;

typedef struct yk_guided_stats {   /* 32 bytes */
  double features_ms;              /* the feature pass (device); 0 when the cached pass was reused */
  double moments_ms;               /* the gather of m and v (device)                 */
  double filter_ms;                /* the filter and the RGB8 conversion (device)    */
  double total_ms;                 /* the call's host wall clock, copies included    */
} yk_guided_stats;

/* The pair tuned together (host only): colour radius 5, patch 1, k2 2.0, alpha 1.0,
 * eps 1e-10; features grid 2, k2 2.0, alpha 1.0, tau_albedo 1e-2, tau_normal 1e-1, tau_depth 1e-2.
 * Either pointer may be NULL, not both. */
int yk_guided_defaults(yk_denoise_params* colour, yk_feature_params* feat);
int ykgpu_film_features(ykgpu_film* film, uint32_t grid, double* mean_host, double* var_host, double* ms);
/* colour / feat NULL: that side of yk_guided_defaults.  Outputs as ykgpu_film_denoise's. */
int ykgpu_film_denoise_guided(ykgpu_film* film, const yk_denoise_params* colour, const yk_feature_params* feat,
                              double* mean_host, uint8_t* rgb_host, yk_guided_stats* stats);

/* ---- group films: progressive, adaptive and denoised films over a device group -----------------
 * (Added under ABI 11 like the film: nothing that existed changed size or meaning.  DESIGN.md 6.7.)
 *
 * A group film made from params P over the k entries of a group means exactly what
 * ykgpu_film_create(ctx, P) means on one context holding the same scene: every array below is in
 * the whole tile's pixel order and layout, and the sums, second moments and counts, resolve's RGB8,
 * the e2 map with pixels, pixels_over, max_e2, samples_done and samples_target, the feature means
 * and variances and the filtered mean and RGB8 of both filters are the single-context film's bytes.
 * So yk_film_save* / yk_film_load* files pass between a group film and a single-context film.  Only
 * the work is spread: the sample chunks by ykgpu_group_render's dealing, the filters' by bands.
 *
 * Dealing.  Entry e holds an ordinary film of ykgpu_group_render's sub-tile: rows row_begin +
 * e*row_stride with stride row_stride*k, ceil((row_count - e)/k) of them, the column set unchanged;
 * an entry without rows holds nothing.  row_band_log2 != 0 with k > 1: YK_ERR_UNSUPPORTED, as for the
 * group render.  Seeds and the camera go by image positions, so nothing else changes.  With
 * YK_SEED_RANDOM_DEVICE and seed_key == 0 the key is drawn once, at create, and given to every
 * entry; ykgpu_group_film_params returns it.
 *
 * State.  The single film's rules hold for the whole tile.  UNIFORM means all counts equal over all
 * entries: two entries that are each uniform at different counts make a non-uniform group film, on
 * which ykgpu_group_film_accumulate returns YK_ERR_INVALID, read's *done is the smallest count and
 * resolve, error and the filters use each pixel's own count.  After ykgpu_group_set_scene the
 * accumulates, ykgpu_group_film_features and ykgpu_group_film_denoise_guided return YK_ERR_INVALID
 * (a stale scene).  If an entry's accumulate fails part-way the group film is torn until a write.
 * Every error code of the film calls applies (a chunk past the target, n_samples == 0, a count below
 * 2 for the filters, both outputs NULL ...); YK_ERR_UNSUPPORTED of the filters refers to P's tile,
 * which must be consecutive image rows and columns, not to the entries' sub-tiles.  The message of a
 * failing entry names it: "group film entry e: ...".  A group film must be destroyed before its
 * group.  Calls are synchronous and not reentrant per group.
 *
 * Concurrency.  ykgpu_group_film_accumulate enqueues every entry's chunk before it waits for any;
 * an adaptive pass runs each entry's pass on a host thread of its own, joined before the call
 * returns.  No entry's work depends on another's progress, and no result on scheduling.
 * ykgpu_group_get_stats then describes the accumulate as it describes a group render (an entry by
 * index, -1 the call).  Of yk_film_pass, pixels_selected, samples_added, min_count and max_count are
 * the single film's; groups and launches are SUMS OVER THE ENTRIES.
 *
 * Filters.  "film denoise" is defined on the whole tile and reads, for a pixel, only rows within
 * R + F of it.  Entry e owns a band of consecutive tile rows (the first row_count % k bands one row
 * taller) and holds buffers for the band grown by the halo R + F, clipped at the tile.  A call runs
 * the moments on every entry's own film, moves the rows from the entries that rendered them to the
 * entries whose band or halo holds them (pitched device-to-device copies, ordered by events across
 * the entries' streams), runs the unchanged filter kernel on each band+halo as a tile of its own,
 * keeps the band rows and copies each band into the caller's arrays.  The guided filter computes the
 * feature pass for its band+halo rows itself (a function of scene and pixel: no exchange), cached
 * per (group film, grid, halo).  The count and tile checks are made before any kernel runs. */
typedef struct ykgpu_group_film ykgpu_group_film;

typedef struct yk_group_denoise_stats { /* 40 bytes */
  double features_ms;              /* each the largest entry's device time; features_ms is 0 for  */
  double moments_ms;               /* the colour-only filter and when every entry's pass was      */
  double exchange_ms;              /* cached; exchange_ms the copies between the entries          */
  double filter_ms;
  double total_ms;                 /* the call's host wall clock, copies included    */
} yk_group_denoise_stats;

int ykgpu_group_film_create(ykgpu_group* group, const yk_render_params* params, ykgpu_group_film** out);
int ykgpu_group_film_destroy(ykgpu_group_film* film);
int ykgpu_group_film_params(const ykgpu_group_film* film, yk_render_params* out);
int ykgpu_group_film_accumulate(ykgpu_group_film* film, uint32_t n_samples);
int ykgpu_group_film_accumulate_adaptive(ykgpu_group_film* film, double threshold2, uint32_t n_samples, yk_film_pass* out);
int ykgpu_group_film_resolve(ykgpu_group_film* film, uint8_t* rgb_host);
int ykgpu_group_film_read(ykgpu_group_film* film, double* sums, double* sumsq, uint32_t* done);
int ykgpu_group_film_write(ykgpu_group_film* film, const double* sums, const double* sumsq, uint32_t done);
int ykgpu_group_film_counts(ykgpu_group_film* film, uint32_t* counts_host, uint32_t* min_count, uint32_t* max_count);
int ykgpu_group_film_write_counts(ykgpu_group_film* film, const double* sums, const double* sumsq, const uint32_t* counts);
int ykgpu_group_film_error(ykgpu_group_film* film, double threshold2, double* e2_host, yk_film_stats* stats);
int ykgpu_group_film_features(ykgpu_group_film* film, uint32_t grid, double* mean_host, double* var_host, double* ms);
int ykgpu_group_film_denoise(ykgpu_group_film* film, const yk_denoise_params* params, double* mean_host,
                             uint8_t* rgb_host, yk_group_denoise_stats* stats);
int ykgpu_group_film_denoise_guided(ykgpu_group_film* film, const yk_denoise_params* colour,
                                    const yk_feature_params* feat, double* mean_host, uint8_t* rgb_host,
                                    yk_group_denoise_stats* stats);

/* ---- sampled film features: the guides from the film's own lens samples --------------------
 * (Added under ABI 11 like the film: nothing that existed changed size or meaning.  DESIGN.md 6.8.)
 *
 * A second way to fill a film's 17 feature planes ("film features" above): from the first hits of
 * the film's own first n samples instead of pinhole sub-rays, so that under a thin lens the guides
 * are defocused where the colour is.  For pixel (x, y) of the film's tile and n in
 * 1 .. min(256, samples_per_pixel), for s = 0 .. n-1 in order:
 *   ray       (o, d) = what yk_camera_sample_ray(camera, the film's params, y, x, s) returns: the
 *             sample's seed (counter, or keyed with the film's seed_key; stride = the film's target),
 *             the engine the film's rng names, the two jitter canonicals, the lens rejection loop
 *             and get_ray.  In double whatever the film's precision (features are guides): for an
 *             FP64 film exactly the primary rays its samples 0..n-1 were or will be rendered with.
 *   hit       "ray queries" below, closest mode, t_min = params.t_min, t_max = +inf; a ray outside
 *             that section's domain rule is a miss and does no arithmetic.
 *   f0..f6    the pinhole pass's rule, unchanged: albedo or (1, 1, 1) for a dielectric; the
 *             face-forward normal; t; a miss gives (1, 1, 1, 0, 0, 0, 0).
 *   folds     s = s + f, q = q + (f*f); with G = (double)n:  F = s / G,
 *             U = max(0, (q - (s*s)/G) / (G*(G - 1)))   (n = 1: U = 0), the group sums as before.
 * Every + - * / is one IEEE double operation, never fused.  The layout is the pinhole pass's, so
 * the guided filter runs unchanged on either.
 *
 * A film still holds ONE set of planes, keyed by (pinhole grid | sampled n): either kind of pass
 * replaces the other, a repeat call with the same key reuses the planes (ms = 0; samples, hits and
 * redo_pixels are those of the pass that made them).  ykgpu_film_features and
 * ykgpu_film_denoise_guided return the bytes they always returned, before and after a sampled call.
 * ykgpu_film_features_sampled works on any tile, strided ones included, and changes nothing of the
 * film's state; outputs as ykgpu_film_features'.  ykgpu_film_denoise_guided_sampled is
 * ykgpu_film_denoise_guided on the sampled planes: feat->grid is ignored and not validated,
 * feat->reserved must still be 0.  yk_guided_sampled_defaults (host only) is the point chosen by
 * tools/features_sampled_tune.py; any of its pointers may be NULL, not all.  The group calls mean
 * what the single film's mean, byte for byte; each entry's band+halo computes its own pass, cached
 * per (group film, key, halo); of yk_sampled_features_stats a group reports the largest entry's ms
 * and the sums of the entries' counts.
 * Errors, with nothing written:
 *   YK_ERR_INVALID      n_samples == 0, n_samples > 256, n_samples > the film's target; the
 *                       context's scene was set after the film was created; the guided calls add
 *                       ykgpu_film_denoise_guided's (a count below 2, both outputs NULL, the
 *                       parameter ranges)
 *   YK_ERR_UNSUPPORTED  the guided calls on a tile that is not consecutive rows and columns */
typedef struct yk_sampled_features_stats { /* 32 bytes */
  double ms;              /* device time of the pass; 0 when the cached pass was reused */
  uint64_t samples;       /* pixels * n, of the pass that made the planes */
  uint64_t hits;          /* of those, samples whose ray hit a sphere */
  uint32_t redo_pixels;   /* pixels finished by the whole-engine redo */
  uint32_t reserved;
} yk_sampled_features_stats;

int yk_guided_sampled_defaults(yk_denoise_params* colour, yk_feature_params* feat, uint32_t* n_samples);
int ykgpu_film_features_sampled(ykgpu_film* film, uint32_t n_samples, double* mean_host, double* var_host,
                                yk_sampled_features_stats* stats);
int ykgpu_film_denoise_guided_sampled(ykgpu_film* film, const yk_denoise_params* colour, const yk_feature_params* feat,
                                      uint32_t n_samples, double* mean_host, uint8_t* rgb_host, yk_guided_stats* stats);
int ykgpu_group_film_features_sampled(ykgpu_group_film* film, uint32_t n_samples, double* mean_host, double* var_host,
                                      yk_sampled_features_stats* stats);
int ykgpu_group_film_denoise_guided_sampled(ykgpu_group_film* film, const yk_denoise_params* colour,
                                            const yk_feature_params* feat, uint32_t n_samples, double* mean_host,
                                            uint8_t* rgb_host, yk_group_denoise_stats* stats);

/* ---- film mattes: per-pixel sphere-id coverage from the film's own samples -----------------
 * (Added under ABI 11 like the film: nothing that existed changed size or meaning.  DESIGN.md 6.10.)
 *
 * Which spheres are in a pixel and how much of each, antialiased and defocused exactly as the
 * film's colour is (the idea behind Cryptomatte).  For pixel (x, y) of the film's tile let
 * n_p = n_samples if n_samples > 0, else the pixel's own count in the film (ykgpu_film_counts').
 * For s = 0 .. n_p-1 in order:
 *   ray       what yk_camera_sample_ray(camera, the film's params, y, x, s) returns, exactly as in
 *             "sampled film features": in double whatever the film's precision, with the film's
 *             seed mode, key and engine.
 *   hit       "ray queries" below, closest mode, t_min = params.t_min, t_max = +inf; a ray outside
 *             that section's domain rule is a miss and does no arithmetic.
 *   table     8 slots, empty at first, miss = other = 0:
 *               a miss:                                              miss += 1
 *               a hit on sphere k, and k holds a slot:               that slot's count += 1
 *               a hit on k, no slot holds k, fewer than 8 in use:    a new slot (k, 1)
 *               otherwise:                                           other += 1
 *             so the slots hold the first 8 distinct ids in sample order (the rule depends on the
 *             order by design).
 *   result    the slots sorted by count descending, equal counts by id ascending; unused slots
 *             are (0xFFFFFFFF, 0).
 * The counts are integers: the table is reproducible bit for bit (tests/mattes_ref.py).
 *
 * ykgpu_film_mattes: n_samples is 0 (own counts) or 1 .. samples_per_pixel (the sampled features'
 * cap of 256 does not apply).  The film owns ONE table, allocated at first use and freed with the
 * film; a repeat call with the same n_samples > 0 reuses it (ms = 0, the counts those of the pass
 * that made it), n_samples = 0 always recomputes.  table_host (may be NULL) receives row_count *
 * tile width records in pixel order.  Works on any tile, strided ones included, and changes
 * nothing of the film's sums, counts or feature planes.
 * ykgpu_film_matte_coverage works on the table the film holds now, without tracing: ids are
 * sphere indices and/or YK_MATTE_SKY, duplicates count once.  Per pixel sel = the sum of the
 * counts of the selected slots, plus miss if the sky is selected;
 *   cov = n == 0 ? 0.0 : (double)sel / (double)n      (one IEEE division)
 *   grey = trunc(clamp(cov, 0, 0.999) * 256)
 * Either output may be NULL, not both.  A pixel with other > 0 is a lower bound.
 * The group calls return the single film's bytes in whole-tile pixel order; of the stats a group
 * reports the largest entry's ms and the sums of the entries' counts.
 * Errors, with nothing written:
 *   YK_ERR_INVALID      mattes: n_samples > the film's target; the context's scene was set after
 *                       the film was created.  coverage: the film holds no table; n_ids == 0; ids
 *                       NULL; an id at or above the sphere count that is not YK_MATTE_SKY; both
 *                       outputs NULL */
typedef struct yk_matte_pixel { /* 80 bytes */
  uint32_t id[8], count[8];
  uint32_t n, miss, other, used; /* count[0..7] + miss + other == n; used = slots in use */
} yk_matte_pixel;
enum { YK_MATTE_SKY = 0xFFFFFFFFu };

typedef struct yk_matte_stats { /* 40 bytes */
  double ms;                /* device time of the pass; 0 when the cached table was reused */
  uint64_t samples;         /* the sum of n over the pixels */
  uint64_t hits;            /* of those, samples whose ray hit a sphere */
  uint64_t other_samples;   /* ... and hits that found the 8 slots taken by other ids */
  uint32_t overflow_pixels; /* pixels with other > 0 */
  uint32_t redo_pixels;     /* pixels finished by the whole-engine redo */
} yk_matte_stats;

typedef struct yk_matte_coverage_stats { /* 32 bytes */
  double ms;                 /* device time of the coverage kernel */
  uint64_t pixels_selected;  /* pixels with sel > 0 */
  uint64_t pixels_uncertain; /* pixels with other > 0 */
  uint64_t samples_selected; /* the sum of sel */
} yk_matte_coverage_stats;

int ykgpu_film_mattes(ykgpu_film* film, uint32_t n_samples, yk_matte_pixel* table_host, yk_matte_stats* stats);
int ykgpu_film_matte_coverage(ykgpu_film* film, const uint32_t* ids, uint32_t n_ids, double* cov_host,
                              uint8_t* grey_host, yk_matte_coverage_stats* stats);
int ykgpu_group_film_mattes(ykgpu_group_film* film, uint32_t n_samples, yk_matte_pixel* table_host,
                            yk_matte_stats* stats);
int ykgpu_group_film_matte_coverage(ykgpu_group_film* film, const uint32_t* ids, uint32_t n_ids, double* cov_host,
                                    uint8_t* grey_host, yk_matte_coverage_stats* stats);

/* ---- ray queries (ABI 11) -------------------------------------------------
 * The reference's public world.hit(r, t_min, t_max) (hittable.hpp:32-34, hittable_list.hpp:32-58,
 * sphere.hpp:25-48) for batches of arbitrary rays against the scene of the last ykgpu_set_scene:
 * closest hits and occlusion tests, in double, bit for bit.  FP64 only: hit with T = float and
 * device groups are out of scope (a group's contexts can be queried one by one).
 *
 * CLOSEST MODE (default).  For a ray in the domain (below) the result is hittable_list::hit_impl's:
 * the ordered scan in tuple order with closest_so_far = the ray's t_max at first.  Per sphere
 * (centre c, radius r), o and d the ray's origin and direction:
 *   oc = o - c;  a = (d.x*d.x + d.y*d.y) + d.z*d.z;  half_b = (oc.x*d.x + oc.y*d.y) + oc.z*d.z
 *   cc = ((oc.x*oc.x + oc.y*oc.y) + oc.z*oc.z) - r*r;  disc = half_b*half_b - a*cc;  disc < 0: a miss
 *   sq = math::sqrt(disc);  root = (-half_b - sq) / a
 *   if (root < t_min || closest < root) { root = (-half_b + sq) / a;  the same test: a miss }
 *   closest = root, the sphere is the hit (so of equal roots the later index wins)
 * and of the last accepted sphere:  p = o + d*t,  outward = (p - c) / r,
 * front_face = dot(d, outward) < 0,  normal = front_face ? outward : -outward.
 * Every + - * / is one IEEE double operation, rounded on its own and never fused.
 * A hit: p, normal, t as above, id the sphere's tuple index, flags YK_HIT_HIT (| YK_HIT_FRONT_FACE).
 * A miss: every double +0.0, id 0xFFFFFFFF, flags 0.
 *
 * ANY-HIT MODE (YK_CAST_ANY_HIT).  flags carries YK_HIT_HIT exactly when closest mode would report
 * a hit; every other field is as for a miss (which sphere occludes is not reported, so the
 * traversal stops at the first accepted sphere and the output stays deterministic).
 *
 * DOMAIN.  math::sqrt does not terminate on a NaN or infinite discriminant, so the query never
 * feeds it one.  ykgpu_set_scene records E = max_i(max(|cx|, |cy|, |cz|) + |r|).  With
 * mo = max_k |o_k| and md = max_k |d_k|, a ray is in the domain iff
 *   its six components are finite;  t_min is finite and >= 0;  t_max >= t_min (so not NaN; +inf is
 *   allowed);  2^-500 <= md <= 2^500;  s = mo + E <= 2^500;  md*s <= 2^500
 * (then half_b^2 <= 9 * 2^1000 and a*cc <= 12 * 2^1000: every discriminant is finite).  A ray
 * outside the domain does no arithmetic: its doubles are +0.0, its id 0xFFFFFFFF and its flags
 * YK_HIT_OUT_OF_DOMAIN.  That is a per-ray status, not a call error: one bad ray does not void a
 * batch.
 *
 * YK_CAST_LINEAR_SCAN serves every ray by the ordered scan instead of the BVH (same bytes; A/B and
 * debugging); YK_CAST_COUNT_WORK counts node visits and sphere tests (slower).
 *
 * ykgpu_cast_rays is synchronous: it stages rays and hits through device buffers the context owns
 * (grown on demand, counted in yk_render_stats.device_bytes, released with the context), in chunks
 * of at most 2^22 rays, and sums the chunks' kernel times.  ykgpu_cast_rays_async launches on
 * `stream` (NULL: the context's), reads n yk_ray at rays_device and writes n yk_hit at hits_device
 * (both 16-byte aligned device memory); it neither synchronises nor records statistics.
 * ykgpu_set_scene waits for the context's casts, so it cannot pull the scene from under one.
 * Both calls are independent of the render's rings and streams and leave films untouched.
 * ykgpu_cast_get_stats reports the last synchronous cast.
 *   n == 0               YK_OK, nothing done
 *   YK_ERR_INVALID       a null pointer with n > 0; unknown flag bits
 *   YK_ERR_NO_SCENE      a call before ykgpu_set_scene */
typedef struct yk_ray {            /* 64 bytes */
  double origin[3], direction[3];
  double t_min, t_max;             /* t_max may be +inf */
} yk_ray;

typedef struct yk_hit {            /* 64 bytes */
  double p[3], normal[3], t;       /* hit_record (hittable.hpp:17-22) */
  uint32_t id;                     /* tuple index, 0xFFFFFFFF when none */
  uint32_t flags;                  /* YK_HIT_* */
} yk_hit;
enum { YK_HIT_HIT = 1u, YK_HIT_FRONT_FACE = 2u, YK_HIT_OUT_OF_DOMAIN = 4u };
enum { YK_CAST_ANY_HIT = 1u, YK_CAST_LINEAR_SCAN = 2u, YK_CAST_COUNT_WORK = 4u };

typedef struct yk_cast_stats {     /* 64 bytes */
  double kernel_ms, total_ms;      /* device time of the kernels; the call's host wall clock */
  uint64_t rays, hits, out_of_domain;
  uint64_t scan_rays;              /* rays served by the ordered scan */
  uint64_t node_visits, sphere_tests; /* YK_CAST_COUNT_WORK only, else 0 */
} yk_cast_stats;

int ykgpu_cast_rays(ykgpu_context* ctx, const yk_ray* rays_host, uint64_t n, uint32_t flags, yk_hit* hits_host);
int ykgpu_cast_rays_async(ykgpu_context* ctx, const void* rays_device, uint64_t n, uint32_t flags,
                          void* hits_device, void* stream);
int ykgpu_cast_get_stats(ykgpu_context* ctx, yk_cast_stats* out); /* the last synchronous cast */

/* ---- radiance queries (ABI 11) --------------------------------------------
 * The reference's third public call, raytracer<double,double>::ray_color(ray, world, depth, gen)
 * (raytracer.hpp:19-37), for batches of arbitrary rays against the scene of the last
 * ykgpu_set_scene: the colour a ray carries, bit for bit.  FP64 only: ray_color with T = float and
 * device groups are out of scope (a group's contexts can be queried one by one).
 *
 * MEANING.  For a ray in the domain the record is ray_color(ray, world, max_depth, gen) with
 * gen = Engine(seed) after gen.discard(skip) (Engine: mt19937 or xor128, yk_radiance_params.rng):
 *   - every segment is world.hit(r, t_min, +inf) exactly as the ray queries above define it;
 *   - a hit scatters by its sphere's material: lambertian (normal + random_unit_vector, the normal
 *     alone when near_zero), metal (reflect(normalized(d), n), plus fuzz * random_in_unit_sphere whose
 *     length factor uniform(0.01, 0.99) is drawn BEFORE its vector; absorbed unless dot(dir, n) > 0),
 *     dielectric (Schlick; the reflect-or-refract uniform is drawn only when refraction is possible);
 *   - a miss returns the sky: t = (normalized(d).y + 1.0) / 2, (1 - t) * 1 + t * (0.5, 0.7, 1.0);
 *   - depth 0 and an absorbed ray return (0, 0, 0);
 *   - the product a_1 * (a_2 * (... * L)) is multiplied back to front, so zeros keep their sign;
 *   - every + - * / is one IEEE double operation, never fused; square roots are math::sqrt.
 * colour is ray_color's value; t_first the first segment's root (+0.0 without a hit); id_first and
 * id_last the tuple index of the first and the last sphere hit (0xFFFFFFFF without); words the
 * engine words the reference's engine has produced when ray_color returns, skip included; segments
 * the ray_color calls that ran a closest hit; flags how the path ended (one of YK_RAD_SKY,
 * YK_RAD_ABSORBED, YK_RAD_DEPTH, YK_RAD_OUT_OF_DOMAIN) and YK_RAD_MT_FALLBACK when an mt19937 path
 * drew more than 227 words (it then ran the full 624-word engine: a cost, not a difference).
 * A record depends on its ray and the scene alone, never on the batch or the ray's place in it.
 * skip costs one draw per word.
 *
 * DOMAIN.  The start ray must pass the ray queries' domain rule with its t_max = +inf.  A ray that
 * does not does no arithmetic: doubles +0.0, both ids 0xFFFFFFFF, flags YK_RAD_OUT_OF_DOMAIN,
 * words = segments = 0.  Every later segment's ray is put through the same test before its hit; a
 * path that leaves the domain ends there with colour +0.0 and flags YK_RAD_OUT_OF_DOMAIN (|
 * YK_RAD_MT_FALLBACK), the other fields as they stood (DESIGN.md 6.6 on why this is believed never
 * to happen: after the first hit origins lie on spheres and directions have length O(1)).
 *
 * YK_RADIANCE_LINEAR_SCAN serves every segment by the ordered scan (same bytes);
 * YK_RADIANCE_COUNT_WORK also counts segments, words and scan segments in the statistics.
 *
 * ykgpu_radiance_rays is synchronous: it stages rays and records through device buffers the context
 * owns, in chunks of at most 2^22 rays, and records yk_radiance_stats.  ykgpu_radiance_rays_async
 * launches on `stream` (NULL: the context's), reads n yk_path_ray at rays_device and writes n
 * yk_radiance at out_device (both 16-byte aligned device memory); it neither synchronises nor
 * records statistics.  A context's queries run one after the other, whatever their streams (they
 * share the per-lane engine and attenuation scratch, which is sized by the resident lanes and
 * max_depth, never by n, allocated at the first query, counted in yk_render_stats.device_bytes and
 * released with the context).  ykgpu_set_scene waits for the context's queries.  Films, the rings
 * and the render streams are untouched.
 *   n == 0               YK_OK, nothing done
 *   YK_ERR_INVALID       a null pointer; unknown flag bits; max_depth outside 1..65535; t_min not
 *                        finite and >= 0; non-zero reserved fields of the params
 *   YK_ERR_NO_SCENE      a call before ykgpu_set_scene
 *   YK_ERR_UNSUPPORTED   an unknown rng */
typedef struct yk_path_ray {       /* 64 bytes */
  double origin[3], direction[3];
  uint32_t seed;                   /* the path's engine is Engine(seed) */
  uint32_t skip;                   /* engine words discarded before ray_color's first draw (mt19937::discard) */
  uint64_t reserved;               /* 0 */
} yk_path_ray;

typedef struct yk_radiance {       /* 64 bytes */
  double colour[3];                /* ray_color's return value */
  double t_first;                  /* t of the first segment's hit, +0.0 if none */
  uint32_t id_first, id_last;      /* tuple index of the first / last sphere hit, 0xFFFFFFFF if none */
  uint32_t words;                  /* engine words consumed, skip included */
  uint32_t segments;               /* ray_color calls that ran a closest hit */
  uint32_t flags;                  /* YK_RAD_* : how the path ended */
  uint32_t reserved[3];            /* 0 */
} yk_radiance;
enum { YK_RAD_SKY = 1u, YK_RAD_ABSORBED = 2u, YK_RAD_DEPTH = 4u, YK_RAD_OUT_OF_DOMAIN = 8u, YK_RAD_MT_FALLBACK = 16u };
enum { YK_RADIANCE_LINEAR_SCAN = 1u, YK_RADIANCE_COUNT_WORK = 2u };

typedef struct yk_radiance_params { /* 32 bytes */
  uint32_t max_depth;              /* 1 .. 65535; ray_color's depth argument */
  uint32_t rng;                    /* YK_RNG_MT19937 | YK_RNG_XOR128 */
  uint32_t flags;                  /* YK_RADIANCE_* */
  uint32_t reserved;
  double t_min;                    /* 0.001 in the reference; finite, >= 0 */
  uint64_t reserved1;
} yk_radiance_params;

typedef struct yk_radiance_stats { /* 64 bytes */
  double kernel_ms, total_ms;      /* device time of the kernels; the call's host wall clock */
  double starts_ms;                /* the part of kernel_ms in the starts kernel (mt19937's seed walks) */
  uint64_t rays;
  uint64_t segments, words;        /* YK_RADIANCE_COUNT_WORK only, else 0 */
  uint32_t out_of_domain;          /* rays with YK_RAD_OUT_OF_DOMAIN (32-bit counts stop at 0xFFFFFFFF) */
  uint32_t mt_fallbacks;           /* rays with YK_RAD_MT_FALLBACK */
  uint32_t scan_segments;          /* segments served by the ordered scan (YK_RADIANCE_COUNT_WORK only) */
  uint32_t lanes;                  /* resident lanes of the path kernel's grid */
} yk_radiance_stats;

int ykgpu_radiance_rays(ykgpu_context* ctx, const yk_radiance_params* params, const yk_path_ray* rays_host,
                        uint64_t n, yk_radiance* out_host);
int ykgpu_radiance_rays_async(ykgpu_context* ctx, const yk_radiance_params* params, const void* rays_device,
                              uint64_t n, void* out_device, void* stream);
int ykgpu_radiance_get_stats(ykgpu_context* ctx, yk_radiance_stats* out); /* the last synchronous query */

/* The ray, seed and skip with which render() enters ray_color for sample s of pixel (y, x) of the
 * image `params` names (host only, FP64, both engines): the counter or keyed seed, the two jitter
 * canonicals, the thin lens' rejection loop and get_ray, in the reference's operation order
 * (source.cpp:154-164, camera.hpp:29-32).  ykgpu_radiance_rays on a pixel's samples_per_pixel sample
 * rays with params' max_depth, t_min and rng, added up in sample order from +0.0, is that pixel of
 * ykgpu_render_sums. */
int yk_camera_sample_ray(const yk_camera* camera, const yk_render_params* params, uint32_t y, uint32_t x,
                         uint32_t s, yk_path_ray* out);
/* ... for n samples (ys[i], xs[i], ss[i]) into out[i]; returns the first sample's error, if any */
int yk_camera_sample_rays(const yk_camera* camera, const yk_render_params* params, const uint32_t* ys,
                          const uint32_t* xs, const uint32_t* ss, uint64_t n, yk_path_ray* out);

/* ---- gather queries (ABI 11) -----------------------------------------------
 * Diffuse radiance at arbitrary points: for a point p with a normal n, the colours of N rays
 * scattered the way the reference's lambertian scatters (material.hpp:50-59: lambertian::scatter,
 * then ray_color of the scattered ray), folded on the device.  A gather at (p, n) is "the colour a
 * white lambertian surface at p facing n returns".  FP64 only, one context only: T = float and
 * device groups are out of scope.
 * (Added under ABI 11 like the films: nothing that existed changed size or meaning.)
 *
 * MEANING.  For point i and s = 0 .. N-1, in order:
 *   g   = Engine(seed_i + s) after g.discard(skip_i)           (seed_i + s in uint32: it wraps)
 *   ru  = random(-1, 1)                  three uniforms, two words each: 6 words
 *   ru  = ru / math::sqrt(dot(ru, ru))
 *   d   = n_i + ru;   if (|d.x| < 1e-8 && |d.y| < 1e-8) d = n_i     (the reference's near_zero, x/y only)
 *   c_s = ray_color(ray(p_i, d), world, max_depth, g)               (g goes on from word skip_i + 6)
 * c_s and its flags are, by definition, the yk_radiance record of ykgpu_radiance_rays for the path
 * ray (p_i, d, seed_i + s, skip_i + 6), computed with the same max_depth, t_min, rng and flags;
 * yk_gather_sample_ray returns that path ray.  The record of the point is the fold of its samples:
 *   sum    = ((0 + c_0) + c_1) + ... + c_{N-1}
 *   sumsq  = q + (c*c) per sample: the product rounded to double, then the sum; no FMA
 *   open   = samples whose gather ray hit nothing (YK_RAD_SKY with segments == 1)
 *   flags  = OR over the samples of (record.flags & (YK_RAD_OUT_OF_DOMAIN | YK_RAD_MT_FALLBACK))
 *   - a sample ray outside the radiance queries' domain contributes colour +0.0 and sets
 *     YK_RAD_OUT_OF_DOMAIN;
 *   - a point with skip > 221 does no arithmetic: its path rays carry the direction (+0, +0, +0),
 *     so all its samples are out of domain: sums +0.0, open 0.  (The six scatter words must lie
 *     inside mt19937's 227 lazy words; xor128 has the same limit so that the contract has one
 *     rule.)  So does a point whose n is zero in all three components, which faces nowhere;
 *   - both are a per-point status, as out-of-domain rays are in the queries: one bad point does
 *     not void a batch;
 *   - every + - * / is one IEEE double operation, never fused;
 *   - a record depends on its point and the scene alone, never on the batch or the point's place
 *     in it.
 *
 * THE TIE TO THE RENDER.  For a camera sample whose first hit is a lambertian sphere with albedo a:
 * p and n that hit's p and normal as ykgpu_cast_rays returns them, seed and skip what
 * yk_camera_sample_ray returns, N = 1 and max_depth = D - 1.  Then a * sum (one multiplication per
 * channel) is the sample's colour bit for bit, and skip + 6 + the path's words its word count.
 *
 * The call is processed in chunks of max(1, floor(2^22 / N)) whole points (no fold is carried
 * across chunks) through the radiance queries' staging and scratch, so the gathers and the
 * radiance queries of one context run one after the other, whatever their streams, and
 * ykgpu_set_scene waits for both.  ykgpu_gather_points is synchronous and records yk_gather_stats
 * (ykgpu_gather_get_stats: the last synchronous call).  ykgpu_gather_points_async launches on
 * `stream` (NULL: the context's), reads n yk_gather_point at points_device and writes n yk_gather
 * at out_device (both 16-byte aligned device memory); it neither synchronises nor records
 * statistics.  Films, the rings and the render streams are untouched.
 *   n == 0               YK_OK, nothing done
 *   YK_ERR_INVALID       a null pointer; unknown flag bits; n_samples outside 1..65536; max_depth
 *                        outside 1..65535; t_min not finite and >= 0; non-zero reserved fields of
 *                        the params
 *   YK_ERR_NO_SCENE      a call before ykgpu_set_scene
 *   YK_ERR_UNSUPPORTED   an unknown rng */
typedef struct yk_gather_point {   /* 64 bytes */
  double p[3];                     /* origin of every gather ray                                   */
  double n[3];                     /* hit_record.normal of the scatter; used as given, never normalised */
  uint32_t seed;                   /* sample s draws from Engine(seed + s), uint32 wrap            */
  uint32_t skip;                   /* engine words discarded before the scatter's draws; <= 221     */
  uint64_t reserved;               /* 0 */
} yk_gather_point;

typedef struct yk_gather {         /* 64 bytes */
  double sum[3];                   /* ((0 + c_0) + c_1) + ... + c_{N-1}                             */
  double sumsq[3];                 /* q = q + (c*c): product rounded to double, then the sum; no FMA */
  uint32_t samples;                /* N */
  uint32_t open;                   /* samples whose gather ray hit nothing (YK_RAD_SKY with segments == 1) */
  uint32_t flags;                  /* OR over the samples of (record.flags & (YK_RAD_OUT_OF_DOMAIN | YK_RAD_MT_FALLBACK)) */
  uint32_t reserved;               /* 0 */
} yk_gather;

typedef struct yk_gather_params {  /* 32 bytes */
  uint32_t n_samples;              /* N, 1 .. 65536 */
  uint32_t max_depth;              /* 1 .. 65535: ray_color's depth argument for the gather ray */
  uint32_t rng, flags;             /* YK_RNG_*; YK_RADIANCE_LINEAR_SCAN | YK_RADIANCE_COUNT_WORK */
  double t_min;                    /* finite, >= 0 */
  uint64_t reserved;               /* 0 */
} yk_gather_params;

typedef struct yk_gather_stats {   /* 64 bytes */
  double kernel_ms, total_ms;      /* device time of the kernels; the call's host wall clock */
  double starts_ms, fold_ms;       /* the parts of kernel_ms in yk_gather_starts and yk_gather_fold */
  uint64_t points, rays;           /* rays = points * n_samples */
  uint64_t open;                   /* the records' open, added up */
  uint32_t out_of_domain;          /* POINTS with YK_RAD_OUT_OF_DOMAIN (32-bit counts stop at 0xFFFFFFFF) */
  uint32_t mt_fallbacks;           /* POINTS with YK_RAD_MT_FALLBACK */
} yk_gather_stats;

int ykgpu_gather_points(ykgpu_context* ctx, const yk_gather_params* params, const yk_gather_point* points_host,
                        uint64_t n, yk_gather* out_host);
int ykgpu_gather_points_async(ykgpu_context* ctx, const yk_gather_params* params, const void* points_device,
                              uint64_t n, void* out_device, void* stream);
int ykgpu_gather_get_stats(ykgpu_context* ctx, yk_gather_stats* out); /* the last synchronous gather */

/* The path ray of sample s of a gather point (host only, both engines): (p, d, seed + s, skip + 6)
 * with d as MEANING defines it, (+0, +0, +0) for a point with skip > 221 or a zero n.
 * ykgpu_radiance_rays on a point's N path rays, folded as above, is that point's yk_gather. */
int yk_gather_sample_ray(const yk_gather_point* point, uint32_t rng, uint32_t s, yk_path_ray* out);
/* ... for n_points points and s = 0 .. n_samples-1 into out[i * n_samples + s] */
int yk_gather_sample_rays(const yk_gather_point* points, uint64_t n_points, uint32_t rng, uint32_t n_samples,
                          yk_path_ray* out);

/* ---- host-side scene helpers (no device needed) ---------------------------------------- */

/* camera<double>{} of camera.hpp:16-27 (16:9, viewport height 2, focal length 1, origin 0). */
int yk_camera_reference(yk_camera* out);

/* Positionable thin-lens camera (extension for configs 2-5). vfov in degrees. */
int yk_camera_look(yk_camera* out, const double lookfrom[3], const double lookat[3],
                   const double vup[3], double vfov_deg, double aspect, double aperture,
                   double focus_dist);

/* Named scenes: "ref4" (source.cpp:103-112), "lambert3", "mixed12", "rtiow5" (config 2),
 * "final" (RTIOW final scene, ~488 spheres, configs 3/4), "glass" (dielectric-heavy, config 5).
 * `seed` drives the random generators of "final" / "glass".  Writes up to `capacity` spheres,
 * the count to *count and the scene's camera to *camera (either may be NULL to query). */
int yk_scene_build(const char* name, uint32_t seed, yk_sphere* spheres, uint32_t capacity,
                   uint32_t* count, yk_camera* camera);

/* Scene files (an on-disk format for generated scenes).  Text: a "yk-scene 1"
 * header, one "camera" line (origin, lower_left_corner, horizontal, vertical, lens_u, lens_v,
 * lens_radius) and one "sphere <lambertian|metal|dielectric> cx cy cz radius r g b fuzz ior"
 * line per sphere in tuple order; numbers as %.17g, so every double round-trips exactly.
 * yk_scene_read follows yk_scene_build's capacity/count/camera convention. */
int yk_scene_write(const char* path, const yk_sphere* spheres, uint32_t count, const yk_camera* camera);
int yk_scene_read(const char* path, yk_sphere* spheres, uint32_t capacity, uint32_t* count, yk_camera* camera);

/* Image height of the reference for a width: uint32(W / (16.0/9.0)) (source.cpp:61-62). */
uint32_t yk_image_height_for(uint32_t width);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* YKGPU_H */
