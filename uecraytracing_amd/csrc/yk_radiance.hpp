// yk_radiance.hpp — radiance queries (include/ykgpu.h "radiance queries"): the
// reference's raytracer<double,double>::ray_color(ray, world, depth, gen) for batches of arbitrary
// rays, each with an engine of its own (seed, skip), in IEEE double so that tests/radiance_ref.py
// restates every record bit for bit.
//
// Part of the unit yk_features.hip, which includes this file once at its end, after yk_cast.hpp (the
// list of units is fixed, tests/test_build_knobs.py).  A kernel beside the render: nothing here
// touches the render's kernels, rings or streams.  Two kernels:
//   yk_radiance_starts  mt19937 only: x_397 of every ray's seeding sequence, kWalk rays per lane
//                       (ykd::mt_walk397xn), 4 bytes per ray, so that the 397-step walk stays out of
//                       the divergent loop below;
//   yk_radiance_paths   a persistent grid sized to the device; a lane runs one path at a time, and
//                       every trip of the loop does one segment (domain test, closest hit, scatter)
//                       for all lanes; a lane whose path ended unwinds its attenuations back to
//                       front, writes its 64-byte record and takes the next ray from the wave's
//                       reserve (one atomic per wave and claim, small claims near the end).
// The closest hit and the hit record are the ray queries' (ykquery::closest_hit and hit_record,
// yk_query.hpp), with t_max = +inf.
// A path's record depends on its ray alone: the engine is the path's own, a lane's scratch is
// rewritten before it is read (mt_slow seeds all 624 words at word 227), and the unwind multiplies
// in the path's own order — so neither the batch nor the lane a ray lands on can change a byte.
#ifndef YK_RADIANCE_HPP
#define YK_RADIANCE_HPP

#include <chrono>
#include <string>

#include "yk_query.hpp"

namespace ykrad {
using namespace ykhost;
namespace {

constexpr uint32_t kThreads = 256;
constexpr uint32_t kWalk = 4;  // seed walks per lane of the starts kernel
// rays a wave claims per atomic (4 per lane), and near the end of the launch's rays: when fewer
// than 2 x kClaim rays per wave of the grid remain, as the wave last saw the counter
constexpr uint32_t kClaim = 256, kClaimTail = 64;
constexpr uint32_t kKnownFlags = YK_RADIANCE_LINEAR_SCAN | YK_RADIANCE_COUNT_WORK;
constexpr uint32_t kNoId = 0xFFFFFFFFu;
constexpr uint32_t kIdRegs = 8;  // attenuation ids kept in registers (4 x 2 x u16), then the lane's slice
// the attenuation ids' scratch never exceeds this: deeper queries run on a smaller grid
constexpr uint64_t kIdBudget = 512ull << 20;

static_assert(sizeof(yk_path_ray) == 64 && sizeof(yk_radiance) == 64 && sizeof(yk_radiance_params) == 32 &&
                  sizeof(yk_radiance_stats) == 64, "radiance query records");
static_assert(offsetof(yk_path_ray, seed) == 48 && offsetof(yk_path_ray, skip) == 52, "yk_path_ray");
static_assert(offsetof(yk_radiance, t_first) == 24 && offsetof(yk_radiance, id_first) == 32 &&
                  offsetof(yk_radiance, words) == 40 && offsetof(yk_radiance, segments) == 44 &&
                  offsetof(yk_radiance, flags) == 48, "yk_radiance");
static_assert(offsetof(yk_radiance_params, t_min) == 16, "yk_radiance_params");
static_assert(offsetof(yk_radiance_stats, rays) == 24 && offsetof(yk_radiance_stats, out_of_domain) == 48 &&
                  offsetof(yk_radiance_stats, lanes) == 60, "yk_radiance_stats");

struct RadArgs {
  const double* rays;    // 8 doubles per ray (yk_path_ray: seed and skip in the seventh)
  double* out;           // 8 doubles per record (yk_radiance)
  const uint32_t* x397;  // per ray of the launch (mt19937)
  uint32_t n;            // rays of this launch (<= kRadChunk)
  uint32_t flags;        // YK_RADIANCE_*
  uint32_t max_depth, claim_tail;
  double t_min;
  uint32_t* claim;                // the launch's ray counter
  uint32_t* mt_scratch;           // 624 words per resident lane
  uint16_t* id_scratch;           // id_stride ids per resident lane
  unsigned long long* counters;   // kRadStripes x kRadCounters words, or null (asynchronous queries)
  ykquery::QueryTree q;
  uint32_t id_stride;
};

__global__ __launch_bounds__(kThreads) void yk_radiance_starts(const uint32_t* rays, uint32_t n, uint32_t* x397) {
  const uint32_t base = blockIdx.x * (kThreads * kWalk) + threadIdx.x;
  uint32_t x[kWalk];
#pragma unroll
  for (uint32_t k = 0; k < kWalk; ++k) {
    const uint32_t i = base + k * kThreads;
    x[k] = i < n ? rays[(size_t)i * 16 + 12] : 0u;  // yk_path_ray::seed
  }
  ykd::mt_walk397xn(x);
#pragma unroll
  for (uint32_t k = 0; k < kWalk; ++k) {
    const uint32_t i = base + k * kThreads;
    if (i < n) x397[i] = x[k];
  }
}

// the engine of a lane and of a path
__device__ __forceinline__ void lane_init(ykd::MtLane& g, const RadArgs& a, uint32_t gid) {
  g.state = a.mt_scratch + (size_t)gid * ykd::kMtN;
  g.a0 = g.a1 = g.b = g.j = g.seed = 0;
}
__device__ __forceinline__ void lane_init(ykd::X128Lane& g, const RadArgs&, uint32_t) { g.x = g.y = g.z = g.w = g.n = 0; }
__device__ __forceinline__ void path_start(ykd::MtLane& g, const RadArgs& a, uint32_t idx, uint32_t seed) {
  ykd::mt_start_from(g, seed, a.x397[idx]);
}
__device__ __forceinline__ void path_start(ykd::X128Lane& g, const RadArgs&, uint32_t, uint32_t seed) {
  ykd::x128_start(g, seed);
}

template <class G>
__global__ __launch_bounds__(kThreads) void yk_radiance_paths(RadArgs a) {
  extern __shared__ __attribute__((aligned(16))) int32_t rad_stack[];  // [entry][lane]: (stack_cap + 3) x 256
  const uint32_t tid = threadIdx.x, lane = tid & 63u;
  const uint32_t gid = blockIdx.x * kThreads + tid;
  int32_t* const stk = rad_stack + tid;
  uint16_t* const id_spill = a.id_scratch + (size_t)gid * a.id_stride;
  const bool count = (a.flags & YK_RADIANCE_COUNT_WORK) != 0;
  G g;
  lane_init(g, a, gid);

  bool in_path = false, finished = false;  // finished: the launch has no ray left for this lane
  uint32_t idx = 0, res_base = 0, res_left = 0;  // the wave's reserve of claimed rays (wave-uniform)
  v3 o = {0, 0, 0}, d = {0, 0, 0};
  uint32_t depth = 0, skip = 0, segments = 0, scans = 0, id_first = kNoId, id_last = kNoId;
  uint32_t nstk = 0, st0 = 0, st1 = 0, st2 = 0, st3 = 0;  // attenuation ids, the newest in st0's low half
  double t_first = 0;
  uint32_t c_rays = 0, c_ood = 0, c_fb = 0, c_seg = 0, c_words = 0, c_scan = 0;

  for (;;) {
    // refill: lanes without a path take the next rays of the wave's reserve, one atomic per claim
    {
      const bool want = !in_path && !finished;
      const unsigned long long m = __ballot(want);
      if (m) {
        const uint32_t need = (uint32_t)__popcll(m);
        uint32_t fresh = 0, csize = kClaim;
        if (res_left < need) {
          const uint32_t seen = res_base + res_left;  // where the counter stood after the wave's last claim
          if (seen >= a.n || a.n - seen < a.claim_tail) csize = kClaimTail;
          const int leader = __ffsll((long long)m) - 1;
          if ((int)lane == leader) fresh = atomicAdd(a.claim, csize);
          fresh = __builtin_amdgcn_readlane(fresh, leader);
        }
        if (want) {
          const uint32_t r = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
          idx = r < res_left ? res_base + r : fresh + (r - res_left);
        }
        if (res_left < need) {
          res_base = fresh + (need - res_left);
          res_left = csize - (need - res_left);
        } else {
          res_base += need;
          res_left -= need;
        }
        if (want) {
          if (idx < a.n) {
            const double2* r = (const double2*)a.rays + (size_t)idx * 4;  // (16-byte aligned: the host checks)
            const double2 r0 = r[0], r1 = r[1], r2 = r[2], r3 = r[3];
            o = {r0.x, r0.y, r1.x};
            d = {r1.y, r2.x, r2.y};
            const uint64_t ss = __builtin_bit_cast(uint64_t, r3.x);
            path_start(g, a, idx, (uint32_t)ss);
            skip = (uint32_t)(ss >> 32);
            depth = a.max_depth;
            segments = scans = nstk = 0;
            st0 = st1 = st2 = st3 = 0;
            id_first = id_last = kNoId;
            t_first = 0;
            in_path = true;
          } else {
            finished = true;  // (the counter only grows: every later claim is past the end too)
          }
        }
      }
    }
    if (__ballot(in_path) == 0) break;  // (a lane without a path after the refill is finished)

    bool ended = false, unwind = true;
    uint32_t endfl = 0;
    double L_r = 0, L_g = 0, L_b = 0;
    if (in_path) {
      // the domain rule before every hit (include/ykgpu.h): no discriminant is NaN or infinite, so
      // math::sqrt's loop ends (ykd::nsqrt bounds it besides)
      if (!ykquery::in_domain(o, d, a.t_min, INFINITY, a.q.extent)) {
        ended = true;
        unwind = false;
        endfl = YK_RAD_OUT_OF_DOMAIN;
      } else {
        if (segments == 0)  // mt19937::discard(skip), with the ordinary draw
          for (uint32_t k = 0; k < skip; ++k) (void)ykd::rng_next(g);
        ++segments;
        // world.hit(r, t_min, +inf)
        const ykquery::Hit h = ykquery::closest_hit<kThreads>(a.q, stk, true, o, d, a.t_min, INFINITY,
                                                              (a.flags & YK_RADIANCE_LINEAR_SCAN) != 0, false);
        const double T = h.t;
        const int hid = h.id;
        if (h.scanned) ++scans;
        if (hid < 0) {
          // sky (raytracer.hpp:35-36): t = (normalized(dir).y + 1)/2, lerp white -> (.5,.7,1)
          const v3 un = ykd::normalized(d);
          const double t = (un.y + 1.0) / 2;
          L_r = (1.0 - t) * 1.0 + t * 0.5;
          L_g = (1.0 - t) * 1.0 + t * 0.7;
          L_b = (1.0 - t) * 1.0 + t * 1.0;
          ended = true;
          endfl = YK_RAD_SKY;
        } else {
          const SphereMat m = a.q.mat[hid];
          const ykquery::HitRecord rec = ykquery::hit_record(o, d, T, a.q.geo[hid], m.radius);
          const v3 p = rec.p, nrm = rec.nrm;
          const bool front = rec.front;
          if (segments == 1) {
            t_first = T;
            id_first = (uint32_t)hid;
          }
          id_last = (uint32_t)hid;
          bool scattered = true, push = true;
          v3 nd;
          if (m.kind == YK_MATERIAL_LAMBERTIAN) {  // material.hpp:50-59, random_unit_vector :33-36
            v3 ru = ykd::random_vec(g, -1.0, 1.0);
            ru = ykd::divs(ru, ykd::nsqrt(ykd::len2(ru)));
            nd = ykd::add(nrm, ru);
            if (ykd::near_zero(nd)) nd = nrm;
          } else if (m.kind == YK_MATERIAL_METAL) {  // material.hpp:67-75 (+ fuzz extension)
            nd = ykd::reflect(ykd::normalized(d), nrm);
            if (m.fuzz > 0) {  // the length factor is drawn before the vector (oracle/yk_oracle_path.h)
              const double k = ykd::uniform(g, 0.01, 0.99);
              v3 ru = ykd::random_vec(g, -1.0, 1.0);
              ru = ykd::divs(ru, ykd::nsqrt(ykd::len2(ru)));
              nd = ykd::add(nd, ykd::mul(ykd::mul(ru, k), m.fuzz));
            }
            scattered = ykd::dot(nd, nrm) > 0;
          } else {  // dielectric extension; its attenuation (1,1,1) is not pushed: 1.0 * L is L exactly
            push = false;
            // 1/ior and Schlick's r0 of both sides come from ykgpu_set_scene (the dielectric's unused
            // fuzz / albedo fields), computed with the reference's operations
            const double ratio = front ? m.fuzz : m.ior;
            const double r0 = front ? m.ar : m.ag;
            const v3 unit = ykd::normalized(d);
            double ct = ykd::dot(ykd::neg(unit), nrm);
            if (!(ct < 1.0)) ct = 1.0;
            const double sn = ykd::nsqrt(1.0 - ct * ct);
            const bool cannot = ratio * sn > 1.0;
            // (`cannot || ...`: total internal reflection draws nothing)
            if (cannot || ykd::reflectance_r0(ct, r0) > ykd::uniform(g, 0.0, 1.0)) {
              nd = ykd::reflect(unit, nrm);
            } else {
              const v3 perp = ykd::mul(ykd::add(unit, ykd::mul(nrm, ct)), ratio);
              const double pl = 1.0 - ykd::len2(perp);
              nd = ykd::add(perp, ykd::mul(nrm, -ykd::nsqrt(pl < 0 ? -pl : pl)));
            }
          }
          if (!scattered) {
            ended = true;  // absorbed: black (raytracer.hpp:30)
            endfl = YK_RAD_ABSORBED;
          } else {
            if (push) {
              if (nstk >= kIdRegs) id_spill[nstk - kIdRegs] = (uint16_t)(st3 >> 16);
              st3 = (st3 << 16) | (st2 >> 16);
              st2 = (st2 << 16) | (st1 >> 16);
              st1 = (st1 << 16) | (st0 >> 16);
              st0 = (st0 << 16) | (uint32_t)hid;
              ++nstk;
            }
            o = p;
            d = nd;
            if (--depth == 0) {  // the next ray_color call returns black without a hit (raytracer.hpp:20)
              ended = true;
              endfl = YK_RAD_DEPTH;
            }
          }
        }
      }
    }

    if (ended) {
      // unwind: attenuation_k * (...) from the deepest scatter outwards (raytracer.hpp:31); a path
      // that left the domain returns +0.0 flat
      while (unwind && nstk > 0) {
        const uint32_t id = st0 & 0xffffu;
        st0 = (st0 >> 16) | (st1 << 16);
        st1 = (st1 >> 16) | (st2 << 16);
        st2 = (st2 >> 16) | (st3 << 16);
        st3 = (st3 >> 16) | (nstk > kIdRegs ? ((uint32_t)id_spill[nstk - kIdRegs - 1] << 16) : 0u);
        --nstk;
        const SphereMat m = a.q.mat[id];
        L_r = m.ar * L_r;
        L_g = m.ag * L_g;
        L_b = m.ab * L_b;
      }
      const uint32_t words = ykd::rng_words(g);
      if (ykd::mt_used_fallback(g)) endfl |= YK_RAD_MT_FALLBACK;
      double2* r = (double2*)a.out + (size_t)idx * 4;
      r[0] = make_double2(L_r, L_g);
      r[1] = make_double2(L_b, t_first);
      r[2] = make_double2(__builtin_bit_cast(double, (uint64_t)id_first | ((uint64_t)id_last << 32)),
                          __builtin_bit_cast(double, (uint64_t)words | ((uint64_t)segments << 32)));
      r[3] = make_double2(__builtin_bit_cast(double, (uint64_t)endfl), 0.0);
      ++c_rays;
      if (endfl & YK_RAD_OUT_OF_DOMAIN) ++c_ood;
      if (endfl & YK_RAD_MT_FALLBACK) ++c_fb;
      if (count) c_seg += segments, c_words += words, c_scan += scans;
      in_path = false;
    }
  }

  // statistics: every lane of the wave is here; one atomic per wave and counter into one of
  // kRadStripes copies chosen by the wave's number (the host adds the copies up)
  if (a.counters) {
    unsigned long long* const cnt =
        a.counters + (size_t)((blockIdx.x * (kThreads / 64u) + tid / 64u) % kRadStripes) * kRadCounters;
    const uint32_t s_rays = ykquery::wave_sum(c_rays), s_ood = ykquery::wave_sum(c_ood), s_fb = ykquery::wave_sum(c_fb);
    uint32_t s_seg = 0, s_words = 0, s_scan = 0;
    if (count) {
      s_seg = ykquery::wave_sum(c_seg);
      s_words = ykquery::wave_sum(c_words);
      s_scan = ykquery::wave_sum(c_scan);
    }
    if (lane == 0) {
      if (s_rays) atomicAdd(cnt + 0, (unsigned long long)s_rays);
      if (s_ood) atomicAdd(cnt + 1, (unsigned long long)s_ood);
      if (s_fb) atomicAdd(cnt + 2, (unsigned long long)s_fb);
      if (s_seg) atomicAdd(cnt + 3, (unsigned long long)s_seg);
      if (s_words) atomicAdd(cnt + 4, (unsigned long long)s_words);
      if (s_scan) atomicAdd(cnt + 5, (unsigned long long)s_scan);
    }
  }
}

using PathKernel = void (*)(RadArgs);
inline PathKernel path_kernel(uint32_t rng) {
  return rng == YK_RNG_XOR128 ? yk_radiance_paths<ykd::X128Lane> : yk_radiance_paths<ykd::MtLane>;
}

// the grid and the scratch of a query: a persistent grid of the blocks the device holds at once
// (fewer when max_depth would take the attenuation ids past kIdBudget)
struct Plan {
  uint32_t grid = 0, id_stride = 0;
  size_t lds = 0;
};

int make_plan(ykgpu_context* ctx, const yk_radiance_params* p, Plan& pl) {
  pl.lds = ykquery::query_stack_lds(ykquery::query_stack_cap(ctx->t64), kThreads);
  int occ = 0;
  YK_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, (const void*)path_kernel(p->rng), (int)kThreads, pl.lds));
  if (occ < 1) return fail(YK_ERR_DEVICE, "radiance: the path kernel does not fit a compute unit");
  pl.id_stride = p->max_depth;
  const uint64_t fit = kIdBudget / ((uint64_t)kThreads * pl.id_stride * sizeof(uint16_t));
  pl.grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)occ * (uint64_t)std::max(ctx->cus, 1), fit));
  return YK_OK;
}

// the fixed buffers and the per-lane scratch, grown on demand (after the context's queries in flight)
int ensure(ykgpu_context* ctx, const yk_radiance_params* p, const Plan& pl) {
  if (!ctx->d_rad_x397) YK_HIP(hipMalloc(&ctx->d_rad_x397, kRadChunk * sizeof(uint32_t)));
  if (!ctx->d_rad_claim) YK_HIP(hipMalloc(&ctx->d_rad_claim, sizeof(uint32_t)));
  if (!ctx->rad_ev) YK_HIP(hipEventCreateWithFlags(&ctx->rad_ev, hipEventDisableTiming));
  const size_t lanes = (size_t)pl.grid * kThreads;
  if (p->rng == YK_RNG_MT19937 && lanes > ctx->rad_mt_lanes) {
    YK_HIP(hipEventSynchronize(ctx->rad_ev));
    (void)hipFree(ctx->d_rad_mt);
    ctx->d_rad_mt = nullptr;
    ctx->rad_mt_lanes = 0;
    YK_HIP(hipMalloc(&ctx->d_rad_mt, lanes * ykd::kMtN * sizeof(uint32_t)));
    ctx->rad_mt_lanes = lanes;
  }
  if (lanes * pl.id_stride > ctx->rad_lanes * ctx->rad_id_stride || !ctx->d_rad_ids) {
    YK_HIP(hipEventSynchronize(ctx->rad_ev));
    (void)hipFree(ctx->d_rad_ids);
    ctx->d_rad_ids = nullptr;
    ctx->rad_lanes = ctx->rad_id_stride = 0;
    YK_HIP(hipMalloc(&ctx->d_rad_ids, lanes * pl.id_stride * sizeof(uint16_t)));
    ctx->rad_lanes = lanes;
    ctx->rad_id_stride = pl.id_stride;
  }
  return YK_OK;
}

// the path launch alone over rays [0, n), n <= kRadChunk, on st: d_rad_x397 holds the rays' x_397
// (mt19937), written by yk_radiance_starts or by the gather's starts kernel (yk_gather.hpp)
hipError_t enqueue_paths(const ykgpu_context* ctx, const yk_radiance_params* p, const Plan& pl, const void* rays,
                         void* out, uint32_t n, unsigned long long* counters, hipStream_t st) {
  if (hipError_t e = hipMemsetAsync(ctx->d_rad_claim, 0, sizeof(uint32_t), st)) return e;
  RadArgs a{};
  a.rays = (const double*)rays;
  a.out = (double*)out;
  a.x397 = ctx->d_rad_x397;
  a.n = n;
  a.flags = p->flags;
  a.max_depth = p->max_depth;
  a.claim_tail = pl.grid * (kThreads / 64u) * kClaim * 2u;
  a.t_min = p->t_min;
  a.claim = ctx->d_rad_claim;
  a.mt_scratch = ctx->d_rad_mt;
  a.id_scratch = ctx->d_rad_ids;
  a.counters = counters;
  a.q = ykquery::query_tree(ctx);
  a.id_stride = pl.id_stride;
  hipLaunchKernelGGL(path_kernel(p->rng), dim3(pl.grid), dim3(kThreads), pl.lds, st, a);
  return hipGetLastError();
}

// the two launches over rays [0, n), n <= kRadChunk, on st; mid (may be null) is recorded between them
hipError_t enqueue(const ykgpu_context* ctx, const yk_radiance_params* p, const Plan& pl, const void* rays, void* out,
                   uint32_t n, unsigned long long* counters, hipStream_t st, hipEvent_t mid) {
  if (p->rng == YK_RNG_MT19937) {
    const uint32_t per = kThreads * kWalk;
    hipLaunchKernelGGL(yk_radiance_starts, dim3((n + per - 1) / per), dim3(kThreads), 0, st, (const uint32_t*)rays, n,
                       ctx->d_rad_x397);
    if (hipError_t e = hipGetLastError()) return e;
  }
  if (mid)
    if (hipError_t e = hipEventRecord(mid, st)) return e;
  return enqueue_paths(ctx, p, pl, rays, out, n, counters, st);
}

// the staging of the synchronous query and of a gather's sample slots (yk_gather.hpp): `need` rays
// and as many records, grown after the context's queries in flight
int ensure_staging(ykgpu_context* ctx, size_t need) {
  return ykquery::ensure_pair(ctx->d_rad_rays, ctx->d_rad_out, ctx->rad_cap, need, sizeof(yk_path_ray),
                              sizeof(yk_radiance), ctx->rad_ev);
}

int check_call(const ykgpu_context* ctx, const yk_radiance_params* p, const void* rays, uint64_t n, const void* out) {
  if (!ctx || !p) return fail(YK_ERR_INVALID, "null argument");
  if (p->flags & ~kKnownFlags) return fail(YK_ERR_INVALID, "radiance: unknown flag bits");
  if (p->reserved || p->reserved1) return fail(YK_ERR_INVALID, "radiance: reserved fields must be 0");
  if (p->max_depth < 1 || p->max_depth > 65535) return fail(YK_ERR_INVALID, "radiance: max_depth must be 1..65535");
  if (!(p->t_min >= 0.0 && p->t_min < INFINITY)) return fail(YK_ERR_INVALID, "radiance: t_min must be finite and >= 0");
  if (p->rng != YK_RNG_MT19937 && p->rng != YK_RNG_XOR128) return fail(YK_ERR_UNSUPPORTED, "radiance: unknown rng");
  if (n && (!rays || !out)) return fail(YK_ERR_INVALID, "radiance: null rays or records");
  if (n && !ctx->have_scene) return fail(YK_ERR_NO_SCENE, "radiance query before ykgpu_set_scene");
  return YK_OK;
}

inline uint32_t sat32(unsigned long long v) { return v > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)v; }

}  // namespace
}  // namespace ykrad

extern "C" {

int ykgpu_radiance_rays(ykgpu_context* ctx, const yk_radiance_params* params, const yk_path_ray* rays_host,
                        uint64_t n, yk_radiance* out_host) {
  if (int rc = ykrad::check_call(ctx, params, rays_host, n, out_host)) return rc;
  if (n == 0) return YK_OK;
  const auto t0 = std::chrono::steady_clock::now();
  YK_HIP(hipSetDevice(ctx->device));
  ykrad::Plan pl;
  if (int rc = ykrad::make_plan(ctx, params, pl)) return rc;
  if (int rc = ykrad::ensure(ctx, params, pl)) return rc;
  if (int rc = ykrad::ensure_staging(ctx, (size_t)std::min<uint64_t>(n, kRadChunk))) return rc;
  constexpr size_t kCounterBytes = (size_t)kRadStripes * kRadCounters * sizeof(unsigned long long);
  if (!ctx->d_rad_counters) YK_HIP(hipMalloc(&ctx->d_rad_counters, kCounterBytes));
  const hipStream_t st = ctx->stream;
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
  hipError_t e = hipStreamWaitEvent(st, ctx->rad_ev, 0);  // (after the context's queries on other streams)
  for (int k = 0; k < 3 && e == hipSuccess; ++k) e = hipEventCreate(&ev[k]);
  if (e == hipSuccess) e = hipMemsetAsync(ctx->d_rad_counters, 0, kCounterBytes, st);
  double kernel_ms = 0, starts_ms = 0;
  for (uint64_t base = 0; base < n && e == hipSuccess; base += kRadChunk) {
    const uint32_t cnt = (uint32_t)std::min<uint64_t>(kRadChunk, n - base);
    e = hipMemcpyAsync(ctx->d_rad_rays, rays_host + base, (size_t)cnt * sizeof(yk_path_ray), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipEventRecord(ev[0], st);
    if (e == hipSuccess)
      e = ykrad::enqueue(ctx, params, pl, ctx->d_rad_rays, ctx->d_rad_out, cnt, ctx->d_rad_counters, st, ev[1]);
    if (e == hipSuccess) e = hipEventRecord(ev[2], st);
    if (e == hipSuccess)
      e = hipMemcpyAsync(out_host + base, ctx->d_rad_out, (size_t)cnt * sizeof(yk_radiance), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    float ms = 0, ms0 = 0;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, ev[0], ev[2]);
    if (e == hipSuccess) e = hipEventElapsedTime(&ms0, ev[0], ev[1]);
    kernel_ms += ms;
    starts_ms += ms0;
  }
  unsigned long long c[kRadCounters] = {};
  if (e == hipSuccess) e = ykquery::read_stripes(ctx->d_rad_counters, kRadStripes, kRadCounters, c);
  for (hipEvent_t v : ev)
    if (v) (void)hipEventDestroy(v);
  if (e != hipSuccess)
    return ykhost::fail(e == hipErrorOutOfMemory ? YK_ERR_NOMEM : YK_ERR_DEVICE,
                        std::string("ykgpu_radiance_rays: ") + hipGetErrorString(e));
  yk_radiance_stats& s = ctx->rad_stats;
  s.kernel_ms = kernel_ms;
  s.starts_ms = params->rng == YK_RNG_MT19937 ? starts_ms : 0.0;
  s.rays = c[0];
  s.out_of_domain = ykrad::sat32(c[1]);
  s.mt_fallbacks = ykrad::sat32(c[2]);
  s.segments = c[3];
  s.words = c[4];
  s.scan_segments = ykrad::sat32(c[5]);
  s.lanes = pl.grid * ykrad::kThreads;
  s.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return YK_OK;
}

int ykgpu_radiance_rays_async(ykgpu_context* ctx, const yk_radiance_params* params, const void* rays_device,
                              uint64_t n, void* out_device, void* stream) {
  if (int rc = ykrad::check_call(ctx, params, rays_device, n, out_device)) return rc;
  if (n == 0) return YK_OK;
  if (((uintptr_t)rays_device | (uintptr_t)out_device) & 15u)
    return ykhost::fail(YK_ERR_INVALID, "radiance: rays and records must be 16-byte aligned");
  YK_HIP(hipSetDevice(ctx->device));
  ykrad::Plan pl;
  if (int rc = ykrad::make_plan(ctx, params, pl)) return rc;
  if (int rc = ykrad::ensure(ctx, params, pl)) return rc;
  const hipStream_t st = stream ? (hipStream_t)stream : ctx->stream;
  YK_HIP(hipStreamWaitEvent(st, ctx->rad_ev, 0));  // (the context's queries share its scratch: one after the other)
  for (uint64_t base = 0; base < n; base += kRadChunk) {
    const uint32_t cnt = (uint32_t)std::min<uint64_t>(kRadChunk, n - base);
    YK_HIP(ykrad::enqueue(ctx, params, pl, (const yk_path_ray*)rays_device + base, (yk_radiance*)out_device + base, cnt,
                          nullptr, st, nullptr));
  }
  YK_HIP(hipEventRecord(ctx->rad_ev, st));  // (ykgpu_set_scene and the next query wait for it)
  return YK_OK;
}

int ykgpu_radiance_get_stats(ykgpu_context* ctx, yk_radiance_stats* out) {
  if (!ctx || !out) return ykhost::fail(YK_ERR_INVALID, "null argument");
  *out = ctx->rad_stats;
  return YK_OK;
}

}  // extern "C"

#endif
