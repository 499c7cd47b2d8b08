// yk_render_device.hpp — what every kernel unit of the renderer shares: the execution model, the
// device-side records (scene tables, kernel arguments, start records), the kernel-side tuning block
// and the address and camera helpers the warm-up and both path kernels use.
// (The execution model is described at the top of yk_pipeline.hip.)
#ifndef YK_RENDER_DEVICE_HPP
#define YK_RENDER_DEVICE_HPP

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/ykgpu.h"
#include "yk_bvh.hpp"
#include "yk_device.hpp"
#include "yk_device_f32.hpp"

using ykd::v3;

// The render kernels' instances, by (scene in LDS, kMode): each unit hands out pointers to its own
// kernels (yk_render_f64.hip, yk_render_f32.hip), and yk_pipeline.hip launches through them
const void* yk_fp64_kernel(bool lds, int mode);
const void* yk_f32_kernel(bool lds, int mode);

namespace {

// Geometry of one sphere, as the closest-hit scan reads it (32 B: one scalar x8 load).
// rr = radius*radius computed on the host with the same IEEE multiply as sphere.hpp:33.
struct alignas(32) SphereGeo {
  double cx, cy, cz, rr;
};
// Shading data, read once per segment by the lane that hit the sphere.
struct alignas(16) SphereMat {
  double ar, ag, ab, fuzz;
  double radius, ior;
  uint32_t kind;
  float inv_rf;  // ykf::rcp_refined((float)radius) (FP32 kernel), computed on the device by yk_mat_prep
  double inv_r;  // ykd::rcp_refined(radius), computed on the device by yk_mat_prep
};
static_assert(sizeof(SphereMat) == 64, "SphereMat layout");

// ---- Kernel-side tuning constants (each overridable with -DYK_...: `make variant`,
// tools/build_variant.sh).  The host's are gathered in yk_schedule.hpp. ----
//
// One 768-thread workgroup per CU (12 waves, 3 per SIMD): the scene is copied into LDS once per
// CU instead of once per 256-thread block, which leaves room for the shading tables (sphere
// geometry and materials in tuple order) beside the BVH and the traversal stacks.  The fourth
// wave slot of each SIMD (128 of its 512 VGPRs) is left to the yk_mt_warmup waves, which run the
// next launch's seed walks in the render's idle issue cycles.  (1024 threads, 4 render waves per
// SIMD: the node loop is bound by LDS latency, so the render alone runs 4% faster — 184 vs 192 ms
// per 512-spp frame without the walks — but the walks can no longer overlap: 218 vs 215 ms.)
#ifndef YK_BLOCK
#define YK_BLOCK 768
#endif
// The xor128 instances draw no seed walks, so nothing needs the fourth wave slot of a SIMD: they
// run 1024-thread workgroups (4 render waves per SIMD; the node loop is bound by LDS latency, so
// the fourth wave pays)
#ifndef YK_BLOCK_X128
#define YK_BLOCK_X128 1024
#endif
// VGPRs of the production FP64 render instances: 3 render waves x 112 of a SIMD's 512 leave 176, three
// 48-VGPR warm-up waves and a reduce wave (bench -0.4% against the natural 114 -> 120; 104 spills
// and starves the render: +3.4%, profiles/r06_ab/vgpr/); the counting instances keep theirs
#ifndef YK_RENDER_VGPRS
#define YK_RENDER_VGPRS 112
#endif
// sample slots a wave claims per atomic ...
#ifndef YK_CLAIM
#define YK_CLAIM 512
#endif
// ... and near the end of a launch's slots: when fewer than kClaimTailFactor x kClaim slots per
// wave of the grid remain (as the wave last saw the counter), a wave claims kClaimTail slots at a
// time.  A wave's reserve holds up to kClaim slots (8 samples per lane) when the counter runs
// out, so with full claims to the end some waves still have ~8 samples per lane of work while
// others have none, and every launch drains for that long (0: full claims to the end).
#ifndef YK_CLAIM_TAIL
#define YK_CLAIM_TAIL 64
#endif
#ifndef YK_CLAIM_TAIL_FACTOR
#define YK_CLAIM_TAIL_FACTOR 2
#endif
// the FP64 lens warm-up's retries are drawn after its walks (yk_mt_warmup_defer) for launches of at
// most YK_DEFER_SLOTS slots per warm-up wave; larger launches run the rejection loop in line
#ifndef YK_DEFER_SLOTS
#define YK_DEFER_SLOTS 4096
#endif
// Walks per lane: the deferred FP64 lens warm-up (the headline frame's) walks four slots at once at
// 48 VGPRs, so two of its waves share a SIMD with the three render waves (eight walk chains per
// SIMD instead of four: bench -0.9%, r05_ab/walk/); the other warm-ups walk one
#ifndef YK_WALK_ILP
#define YK_WALK_ILP 4
#endif
// VGPRs of yk_mt_warmup_defer (the attribute counts gfx950's unified register file: twice)
#ifndef YK_DEFER_VGPRS
#define YK_DEFER_VGPRS 48
#endif
constexpr int kBlock = YK_BLOCK, kBlockX128 = YK_BLOCK_X128;
constexpr uint32_t kClaim = YK_CLAIM;
constexpr uint32_t kClaimTail = YK_CLAIM_TAIL, kClaimTailFactor = YK_CLAIM_TAIL_FACTOR;
static_assert(kClaimTail == 0 || (kClaimTail >= 64 && kClaimTail <= YK_CLAIM), "a tail claim serves a whole wave");
constexpr uint64_t kDeferSlots = YK_DEFER_SLOTS;
constexpr uint32_t kWalkIlp = YK_WALK_ILP;

template <int kMode>
constexpr int mode_block() {
  return (kMode & 4) ? kBlockX128 : kBlock;
}
constexpr int block_of(bool x128) { return x128 ? kBlockX128 : kBlock; }

// ---- The variants the kernels are built from.  Each was one side of a compile-time A/B; the losing
// sides are gone from the source (profiles/r11_knobs/README.md says where each one went). ----
//
// Both render kernels read the visit's slab constants as one op_sel-read register pair per axis and
// bound (yk_slab.hpp).  Round 4: FP64 123 -> 115 VGPRs and no faster (512 spp 173.9 -> 174.2 ms),
// FP32 125 -> 111 VGPRs and faster (195.3 -> 190.1 ms, profiles/r04_ab/f32/).  Round 6, on the
// branch-free visit: FP64 128 -> 114 VGPRs, bench -0.7% (the SIMD's spare registers take a third
// warm-up wave, profiles/r06_ab/vgpr/).  (Round 4's two-paths-per-lane kernel, which lost its A/B,
// is kept as a patch beside its evidence: profiles/r04_ab/dual/yk_dual.patch.)
// (Tried and removed in round 4, DESIGN.md §4.1: the FP32 slow-axis bound folded into the slow
// axis' far-plane FMA, +2.3%; the slow-axis read skipped in waves without a slow-axis ray, +3.8%.)
//
// The FP64 node visit has no branch (round 6): the stack's bottom entry holds the empty leaf (a
// sentinel), so "no slot entered" pops unconditionally and every lane of the visit runs the same
// instructions; a lane's run of interior nodes is a loop of its own (while-while), the entry below
// the top read with the planes.  The loop variable is the address of that entry (constant DS
// offsets for it and the pushes).  512 spp, same box (profiles/r06_ab/nodebf/): round 5's visit
// with its push / pop branches -> this one: bench 163.0 -> 159.5 ms.
// The visit's loop exists once, its stack check a uniform branch inside it (two copies, with and
// without the check: +0.4%, profiles/r06_ab/shade/r06an_*).
// The FP64 stack is sized to the tree's proven depth (3 x wide depth + 1 entries) where LDS allows,
// its overflow check then skipped (a scalar branch on KernelArgs::stack_check): bench 159.0 ->
// 156.2 ms on top of the branch-free visit.
// The visit's distances are measured from tmin_lo and scaled by kClampScale, the near FMAs clamp to
// [0, 1] in place of the max with tmin_lo: 4 VALU fewer per visit, bench 150.0 -> 147.0 ms, node
// visits unchanged, bit-exact (profiles/r06_ab/shade/r06ai_*).
// The visit's slab min / max run two slots per asm block (yk_slab.hpp slab_cull2c): one hazard
// pad per visit instead of eight, bench -0.2% (four of four same-box pairs, image hashes equal,
// profiles/r06_ab/shade/r06ag_*).
// The FP64 candidate list keeps its ids as 16-bit halves of two registers: the shift-in is one
// alignbit and one lshl_or instead of four moves, two VGPRs freed; bench -0.3...-0.6%, synced
// -0.4...-0.8%, image hash unchanged (r06_ab/shade/r06ax_*).
// The newest candidate's hb and disc are kept from its leaf test, so its exact root skips the second
// discriminant (17 FP64 operations): bench -0.4...-0.6%, synced -0.6%, the headline image's hash
// unchanged, no spill at 112 VGPRs (profiles/r06_ab/shade/r06ar_*).  Its v_rsq_f64, which
// math::sqrt's start repeats, is not kept (2 VGPRs more: three spills at 112), and the candidates'
// refined 1/a is computed on its own, not from the bounds' 1/a (one Newton step instead of rcp +
// two: neutral, profiles/r06_ab/shade/r06au_*).
// The FP64 dielectric's 1/ior and Schlick r0 (both sides) are precomputed on the host: two FP64
// divisions fewer per trip with a glass hit (bench -0.6%, profiles/r06_ab/shade/).
// The FP64 unwind skips the spill check when no ending lane of the wave spilled, two ids per
// round (bench 156.6 -> 156.0 ms, profiles/r06_ab/unwind/).
// Slot claims take the tail size from a kernel argument and the leader's counter by v_readlane (the
// claim's bookkeeping becomes scalar: 2 VGPRs fewer, profiles/r06_ab/vgpr/r06t_*).
constexpr float kClampScale = 0x1p-24f;
using DevNode = ykbvh::WideNode;  // 4-wide BVH nodes (yk_bvh.hpp)
constexpr int kCounters = 32;  // [16..18]: timeline, [19..22]: diag (stamp builds), [24..31]: work
// Spheres per BVH leaf the kernels' leaf code handles: the FP64 leaf test is loop-free for one
// sphere, the FP32 leaf loop is unrolled for two.  ykgpu_set_scene builds the trees with these
// as ykbvh::Options::max_leaf and upload_tree rejects a tree with a larger leaf (its extra spheres
// would be skipped silently).
constexpr uint32_t kLeafCapF64 = 1, kLeafCapF32 = 2;
constexpr uint32_t kStackRegs = 8;  // attenuation ids kept in registers (4 x 2 x u16)
constexpr uint32_t kFlagLinearScan = YK_FLAG_LINEAR_SCAN;
constexpr uint32_t kFlagOneLane = YK_FLAG_ONE_LANE;
constexpr uint32_t kFlagTrace = YK_FLAG_TRACE_RAYS;

// the camera rounded to float once on the host (camera<float>'s members, camera.hpp:10-27), and
// W, H as floats: the FP32 kernel's start converts nothing
struct CamF {
  float origin[3], llc[3], horizontal[3], vertical[3], lens_u[3], lens_v[3];
  float lens_radius, w, h, pad[3];
};
struct KernelArgs {
  yk_camera cam;
  CamF camf;
  uint32_t W, H, spp, max_depth;
  uint32_t seed0, row_begin, row_count, row_stride, band_log2;
  // stack_check: 0 when the FP64 traversal stack holds 3 x (wide depth) + 1 entries, so the
  // branch-free visit cannot overflow it and skips the check (upload_tree)
  uint32_t nspheres, stack_check, flags, id_stride;
  // A launch renders samples [s0, s0 + nsl / npix_slots) of every pixel: sample slot
  // i = s_local * npix_slots + p is sample s0 + s_local of tile pixel order[p].
  uint32_t s0, nsl, npix_slots, seed_mode;  // seed_mode: YK_SEED_*
  uint32_t nps_m, nps_sh, w_m, w_sh;  // fdiv magic numbers of npix_slots and the tile width Wt
  uint64_t seed_key;
  const uint32_t* __restrict__ order;  // p → tile pixel (kNoPixel: empty slot of an edge block)
  uint64_t pad_a;                      // (keeps the argument layout the kernels were tuned with)
  const void* __restrict__ start;      // StartRec per sample slot (mt19937 kernels)
  double t_min;
  double inv_w, inv_h;  // RN(1/W), RN(1/H) for the camera's exact divisions (div_markstein)
  double w_d, h_d;      // W, H as doubles (kernel arguments: no loop-hoisted conversion to hold)
  double origin_bound;  // |o|_inf beyond which the BVH's float culling is not proven sound
  int32_t bvh_root;
  uint32_t n_nodes;
  uint32_t lds_geo_off, lds_ids_off, lds_stack_off, stack_cap;  // stack_cap: entries a lane may hold
  uint32_t lds_tgeo_off, lds_mat_off;  // FP64 kernel: tuple-order geometry / materials in LDS
  const DevNode* __restrict__ nodes;  // child links are byte offsets from nodes
  const SphereGeo* __restrict__ leaf_geo;  // spheres in BVH leaf order
  const uint32_t* __restrict__ leaf_ids;   // leaf slot → tuple index
  const SphereGeo* __restrict__ geo;
  const SphereMat* __restrict__ mat;
  const float4* __restrict__ geo_f;  // FP32 path: (cx, cy, cz, r*r) rounded to float, tuple order
  double* col;                       // sample colours: a record per slot (colour_store)
  uint32_t* pixel_counter;           // sample-slot counter
  uint32_t* mt_scratch;
  uint16_t* id_scratch;
  unsigned long long* counters;  // [segments, sphere_tests, sqrt_calls, mt_fallbacks, nodes]
  double* trace;                 // YK_FLAG_TRACE_RAYS: rays [(q*spp + s)*trace_cap + k][6]
  uint32_t* trace_counts;        //   ray_color calls per sample [q*spp + s]
  uint32_t trace_cap;
  uint32_t claim_tail;  // slots left below which a wave claims kClaimTail: grid x waves x kClaim x factor
  unsigned long long* clk;  // this launch's shader-clock probe (YK_CLOCK_*): 4 words
  // the tile's columns (include/ykgpu.h yk_render_params; the whole width: Wt = W, 0, 1, 0)
  uint32_t Wt, col_begin, col_stride, col_band;
#ifdef YK_DRAIN_DIAG
  uint32_t diag_c, diag_pad;  // the launch's index in its call
#endif
};

// floor(n / d) for n < 2^31 with the host's magic numbers (fastdiv): ((uint64) n * m) >> sh, where
// l = ceil(log2 d), sh = 31 + l, m = ceil(2^sh / d) < 2^32 — exact for every 31-bit n (the
// round-up error n * (m d - 2^sh) / (d 2^sh) < 2^31 d / (d 2^sh) * d / 2^l <= 1/d).  A runtime
// divisor otherwise costs the ~20-instruction float-reciprocal sequence per division.
__device__ __forceinline__ uint32_t fdiv(uint32_t n, uint32_t m, uint32_t sh) {
  return (uint32_t)(((uint64_t)n * m) >> sh);
}

// Image row of tile row t (include/ykgpu.h yk_render_params: bands of 2^band_log2 rows, every
// row_stride-th band; band_log2 = 0 is the plain strided row set)
__device__ __forceinline__ uint32_t tile_row_y(uint32_t row_begin, uint32_t row_stride, uint32_t band_log2,
                                               uint32_t t) {
  return row_begin + (((t >> band_log2) * row_stride) << band_log2) + (t & ((1u << band_log2) - 1u));
}
// ... and image column of tile column j (bands of 2^col_band columns, every col_stride-th band)
__device__ __forceinline__ uint32_t tile_col_x(uint32_t col_begin, uint32_t col_stride, uint32_t col_band,
                                               uint32_t j) {
  return col_begin + (((j >> col_band) * col_stride) << col_band) + (j & ((1u << col_band) - 1u));
}

__device__ __forceinline__ v3 ld3(const double* p) { return {p[0], p[1], p[2]}; }

// Processing order: slot p of a call renders tile pixel order[p] (ykgpu_context::order, built on
// the host for the image geometry): 8x8 pixel blocks, so the lanes a wave refills together take
// neighbouring pixels in both directions.  Every pixel's samples are independent of the order.
constexpr uint32_t kNoPixel = 0xffffffffu;

// camera::get_ray (camera.hpp:29-32) for pixel (x, y) from the start's draws: the jitter
// canonicals uc, vc (source.cpp:162-163, (x + U01) / W correctly rounded by Markstein's form with
// the host's RN(1/W), yk_device.hpp) and the thin-lens point (px, py) when the camera has a lens.
// The warm-up and the render kernel's own start (xor128, or a record the warm-up could not
// complete) both call it, so a record's ray is the ray the render would have computed.
__device__ __forceinline__ void camera_ray(const yk_camera& cam, double w_d, double inv_w, double h_d,
                                           double inv_h, uint32_t H, uint32_t x, uint32_t y, double uc,
                                           double vc, bool lens, double px, double py, v3& o, v3& d) {
  const double u = ykd::div_markstein((double)x + ykd::uniform_of(uc, 0, 1), w_d, inv_w);
  const double v = ykd::div_markstein((double)(H - y - 1) + ykd::uniform_of(vc, 0, 1), h_d, inv_h);
  const v3 cam_o = ld3(cam.origin), cam_llc = ld3(cam.lower_left_corner);
  const v3 cam_h = ld3(cam.horizontal), cam_v = ld3(cam.vertical);
  d = ykd::sub(ykd::add(ykd::add(cam_llc, ykd::mul(cam_h, u)), ykd::mul(cam_v, v)), cam_o);
  o = cam_o;
  if (lens) {  // thin-lens offset
    const double rx = px * cam.lens_radius, ry = py * cam.lens_radius;
    const v3 off = ykd::add(ykd::mul(ld3(cam.lens_u), rx), ykd::mul(ld3(cam.lens_v), ry));
    o = ykd::add(o, off);
    d = ykd::sub(d, off);
  }
}
// the same in float (camera<float>, the host-rounded camera CamF; (x + U01) / W a float division)
__device__ __forceinline__ void camera_ray_f32(const CamF& cam, uint32_t H, uint32_t x, uint32_t y, float uc,
                                               float vc, bool lens, float px, float py, ykf::v3& o, ykf::v3& d) {
  const float u = ((float)x + uc) / cam.w;
  const float v = ((float)(H - y - 1) + vc) / cam.h;
  const ykf::v3 cam_o = ykf::off(cam.origin), cam_llc = ykf::off(cam.llc);
  const ykf::v3 cam_h = ykf::off(cam.horizontal), cam_v = ykf::off(cam.vertical);
  d = ykf::sub(ykf::add(ykf::add(cam_llc, ykf::mul(cam_h, u)), ykf::mul(cam_v, v)), cam_o);
  o = cam_o;
  if (lens) {
    const float rx = px * cam.lens_radius, ry = py * cam.lens_radius;
    const ykf::v3 off = ykf::add(ykf::mul(ykf::off(cam.lens_u), rx), ykf::mul(ykf::off(cam.lens_v), ry));
    o = ykf::add(o, off);
    d = ykf::sub(d, off);
  }
}

// A sample's start, precomputed by yk_mt_warmup for the mt19937 kernels: the camera ray of the
// sample (after the jitter canonicals and the thin-lens rejection loop) and the lazy cursors
// after those draws (x_j, x_{j+1}, x_{j+397}, j).  j == kNoStart: the lens loop would have
// reached the scratch engine's words (never seen: ~55 rejections), and the render kernel starts
// that sample itself.  FP64: 64 bytes (four 16-byte loads); FP32: 48.
struct alignas(16) StartRec {
  double ox, oy, oz, dx, dy, dz;
  uint32_t a0, a1, b, j;
};
static_assert(sizeof(StartRec) == 64, "StartRec layout");
struct alignas(16) StartRecF {
  float ox, oy, oz, dx, dy, dz;
  uint32_t pad0, pad1;
  uint32_t a0, a1, b, j;
};
static_assert(sizeof(StartRecF) == 48, "StartRecF layout");
constexpr uint32_t kNoStart = 0xffffffffu;
// j == kPadSlot: the slot is an empty slot of an edge block (kNoPixel in the processing order), so
// the render tells it from its StartRec alone and reads the order only for a start it makes itself
constexpr uint32_t kPadSlot = 0xfffffffeu;
constexpr uint32_t kPadX = 0xffffffffu;  // (the warm-up's column of such a slot)

// A sample's colour record: r, g, b as one aligned 32-byte record per sample slot (one 16-byte
// and one 8-byte store, the whole record in one 32-byte sector), in a colour buffer of the launch.
// yk_reduce_samples reads the records of consecutive slots, coalesced.  (Round 4 tried writing
// the colour over the slot's own StartRec instead — no colour buffer at all — and the frame got
// 3% slower: 174.1 -> 179.5 ms, profiles/r04_ab/; the reduce then reads 24 of every 64 bytes.)
constexpr size_t kColStride = 4;
__device__ __forceinline__ void colour_store(double* col, uint32_t slot, double r, double g, double b) {
  double* rec = col + (size_t)slot * kColStride;
  *(double2*)rec = make_double2(r, g);
  rec[2] = b;
}

using RenderKernel = void (*)(KernelArgs);

}  // namespace

#endif
