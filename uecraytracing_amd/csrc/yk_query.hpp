// yk_query.hpp — what the query kernels of the unit yk_features.hip share: the ray
// queries (yk_cast.hpp), the radiance and gather queries (yk_radiance.hpp, yk_gather.hpp) and the
// sampled feature pass (yk_features_sampled.hpp) all ask the reference's world.hit(r, t_min, t_max)
// of the context's FP64 tree, and this file holds the one copy of the answer: the domain rule, the
// traversal's arguments and their fill, the closest hit (the guards, the checked per-lane stack in
// LDS, the float slab test of DESIGN.md §4, the exact leaves with ties to the later tuple index, the
// ordered scan on a guard, an out-of-tree link or an overflow), the hit record, and the host's
// staging and counter helpers.  Everything lives in namespace ykquery.
#ifndef YK_QUERY_HPP
#define YK_QUERY_HPP

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/ykgpu.h"
#include "yk_device.hpp"
#include "yk_host_internal.hpp"

namespace ykquery {
using namespace ykhost;
namespace {

// stack entries per lane, the sentinel included: 3 x wide depth + 1 where that is at
// most kStackMax (51 KiB of LDS a block); the top is checked either way, and a lane that overflows
// takes the scan
constexpr uint32_t kStackMin = 4, kStackMax = 48;
// ... of every query kernel of the unit: the kernel argument and the LDS size both come from it.
// kYkQueryStackForce: yk_features.hip.
inline uint32_t query_stack_cap(const DevTree& t) {
  if (kYkQueryStackForce) return kYkQueryStackForce;
  return std::max(kStackMin, std::min(3 * t.wide_depth + 1, kStackMax));
}
// (the branch-free visit writes up to two entries past the capacity before its check)
inline size_t query_stack_lds(uint32_t stack_cap, uint32_t threads) {
  return (size_t)(stack_cap + 3) * threads * sizeof(int32_t);
}

// the arguments of a traversal
struct QueryTree {
  const char* nodes;          // DevNode; child links are byte offsets
  const SphereGeo* leaf_geo;  // leaf order
  const uint32_t* leaf_ids;   // leaf slot -> tuple index
  const SphereGeo* geo;       // tuple order
  const SphereMat* mat;
  double extent;        // E of the domain rule
  double origin_bound;  // |o|_inf beyond which a ray takes the scan (< 0: every ray)
  int32_t root;
  uint32_t node_bytes, nspheres, stack_cap;
};

inline QueryTree query_tree(const ykgpu_context* ctx) {
  const DevTree& t = ctx->t64;
  QueryTree q{};
  q.nodes = (const char*)t.nodes;
  q.leaf_geo = (const SphereGeo*)t.leaf_geo;
  q.leaf_ids = t.leaf_ids;
  q.geo = ctx->d_geo;
  q.mat = ctx->d_mat;
  q.extent = ctx->cast_extent;
  q.origin_bound = t.origin_bound;
  q.root = t.root;
  q.node_bytes = t.n_nodes * (uint32_t)sizeof(DevNode);
  q.nspheres = ctx->nspheres;
  q.stack_cap = query_stack_cap(t);
  return q;
}

// x rounded to float towards +inf / towards -inf, for x >= 0 (bounds of the cull interval)
__device__ __forceinline__ float f32_up(double x) {
  float f = (float)x;
  if ((double)f < x) f = __uint_as_float(__float_as_uint(f) + 1u);
  return f;
}
__device__ __forceinline__ float f32_down(double x) {
  float f = (float)x;
  if ((double)f > x) f = __uint_as_float(__float_as_uint(f) - 1u);
  return f;
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  return v;
}

// the domain rule of include/ykgpu.h, operation for operation (tests/cast_ref.py restates it)
__device__ __forceinline__ bool in_domain(v3 o, v3 d, double tmin, double tmax, double E) {
  const double mo = fmax(fabs(o.x), fmax(fabs(o.y), fabs(o.z)));
  const double md = fmax(fabs(d.x), fmax(fabs(d.y), fabs(d.z)));
  const bool finite6 = fabs(o.x) < INFINITY && fabs(o.y) < INFINITY && fabs(o.z) < INFINITY &&
                       fabs(d.x) < INFINITY && fabs(d.y) < INFINITY && fabs(d.z) < INFINITY;
  if (!finite6) return false;
  if (!(tmin >= 0.0 && tmin < INFINITY)) return false;
  if (!(tmax >= tmin)) return false;
  if (!(md >= 0x1p-500 && md <= 0x1p500)) return false;
  const double s = mo + E;
  if (!(s <= 0x1p500)) return false;
  return md * s <= 0x1p500;
}

// world.hit's answer: the root and the sphere's tuple index (id < 0: a miss, t = t_max), whether the
// ordered scan gave it, and the work it took
struct Hit {
  double t;
  int id;
  bool scanned;
  uint32_t nodes, tests;  // node visits, sphere tests
};

// hittable_list::hit_impl over sphere::hit_impl, the literal loop in tuple order (aa: len2(d)); the
// tests are added to h's
__device__ __forceinline__ void scan_hit(const QueryTree& q, v3 o, v3 d, double aa, double tmin, double tmax,
                                         bool any_hit, Hit& h) {
  double best = tmax;
  int best_id = -1;
  bool done = false;  // (any-hit: a flag in the loop's condition, as the visit's; a break here cost the cast's scan 15%)
  for (uint32_t k = 0; k < q.nspheres && !done; ++k) {
    const SphereGeo sg = q.geo[k];
    ++h.tests;
    const v3 oc = {o.x - sg.cx, o.y - sg.cy, o.z - sg.cz};
    const double hb = ykd::dot(oc, d);
    const double cc = ykd::len2(oc) - sg.rr;
    const double disc = hb * hb - aa * cc;
    if (disc < 0) continue;
    const double sq = ykd::nsqrt(disc);
    double root = (-hb - sq) / aa;
    if (root < tmin || best < root) {
      root = (-hb + sq) / aa;
      if (root < tmin || best < root) continue;
    }
    best = root;
    best_id = (int)k;
    done = any_hit;
  }
  h.t = best;
  h.id = best_id;
  h.scanned = true;
}

// world.hit(r, t_min, t_max) of a ray in the domain: the tree's visit, or the ordered scan — whose
// answer the visit's is, whatever its order: the minimum root, ties to the later tuple index.  stk:
// the lane's column of the block's stack in LDS, (stack_cap + 3) entries kStride words apart.
// live: the lane has a ray in the domain; a lane without one reads no memory and gets the miss (an
// argument and not the caller's branch: with the guards beside the domain test and not under it,
// yk_cast keeps the parent's rate).  any_hit: the first root accepted ends the search.
template <uint32_t kStride>
__device__ __forceinline__ Hit closest_hit(const QueryTree& q, int32_t* const stk, bool live, v3 o, v3 d, double tmin,
                                           double tmax, bool force_scan, bool any_hit) {
  // the guards that send a ray to the ordered scan: the flag, the host scale guard, an origin
  // beyond the tree's bound, a direction whose float reciprocal the slab test cannot use (zero,
  // |d_k| <= 1e-30 — o/d must stay finite for |o| <= 2^27 — or >= 1e30), and a direction so long
  // against the scene that the float distances fall below float's normal range (the box growth's
  // share of a distance, 2^-21 origin_bound / |d_k|, stays above 2^-111)
  const float dxf = (float)d.x, dyf = (float)d.y, dzf = (float)d.z;
  const float dmin = fminf(fminf(fabsf(dxf), fabsf(dyf)), fabsf(dzf));
  const float dmax = fmaxf(fmaxf(fabsf(dxf), fabsf(dyf)), fabsf(dzf));
  const double mo = fmax(fabs(o.x), fmax(fabs(o.y), fabs(o.z)));
  bool scan = force_scan || q.origin_bound < 0 || !(mo <= q.origin_bound) || !(dmin > 1e-30f && dmax < 1e30f) ||
              !(dmax * 0x1p-90f <= (float)q.origin_bound);

  const double aa = ykd::len2(d);
  double best = tmax;  // the cull interval's end: the ray's t_max, then the closest root so far
  int best_id = -1;
  Hit h = {tmax, -1, false, 0, 0};

  if (live && !scan) {
    // §4's conservative slab test in float: planes times 1/d less o/d, the far distances scaled by
    // 1 + 2^-17, compared against t_min (1 - 2^-17) rounded down and best (1 + 2^-18) rounded up;
    // it keeps every box the plain test with both distances relaxed by 2^-20 keeps
    const float ix = 1.0f / dxf, iy = 1.0f / dyf, iz = 1.0f / dzf;
    constexpr float kFar = 1.0f + 0x1p-17f;
    const float ixs = ix * kFar, iys = iy * kFar, izs = iz * kFar;
    const float oxf = (float)o.x, oyf = (float)o.y, ozf = (float)o.z;
    const float nox = -(oxf * ix), noy = -(oyf * iy), noz = -(ozf * iz);
    const float fox = -(oxf * ixs), foy = -(oyf * iys), foz = -(ozf * izs);
    const float tmin_lo = f32_down(tmin) * (1.0f - 0x1p-17f);
    // the ray's (near x4, far x4) plane quads inside a WideNode (yk_bvh.hpp)
    const uint32_t qx = ix < 0.0f ? 16u : 0u, qy = 48u + (iy < 0.0f ? 16u : 0u), qz = 96u + (iz < 0.0f ? 16u : 0u);
    // The lane's stack; entry 0 holds the empty leaf as a sentinel, so a pop never needs a test of
    // its own: the traversal ends when the sentinel has been popped (sp == 0).  sp is the next free
    // entry.
    stk[0] = ykbvh::kEmptyLeaf;
    uint32_t sp = 1;
    int32_t node = q.root;
    float ustar = f32_up(best) * (1.0f + 0x1p-18f);
    for (;;) {
      // a lane's run of interior nodes, a loop of its own: the wave tests leaves once every lane
      // holds one.  The visit has no branch: the last slot entered is visited next, the others
      // entered are pushed in slot order (written unconditionally at the top, which moves past what
      // was entered: up to two entries past the capacity, which the stack has), and with no slot
      // entered the entry below the top is next.
      while (node >= 0) {
        if ((uint32_t)node + (uint32_t)sizeof(DevNode) > q.node_bytes) {  // (never: a link outside the tree)
          scan = true;
          break;
        }
        ++h.nodes;
        const char* w = q.nodes + node;
        const float4 nx = *(const float4*)(w + qx), fx = *(const float4*)(w + qx + 16);
        const float4 ny = *(const float4*)(w + qy), fy = *(const float4*)(w + qy + 16);
        const float4 nz = *(const float4*)(w + qz), fz = *(const float4*)(w + qz + 16);
        const int4 ch = *(const int4*)(w + 144);
        const int32_t popped = stk[(sp - 1) * kStride];
#define YK_QUERY_SLOT(c)                                                                                  \
  (fmaxf(fmaxf(fmaxf(__builtin_fmaf(nx.c, ix, nox), __builtin_fmaf(ny.c, iy, noy)), __builtin_fmaf(nz.c, iz, noz)), \
         tmin_lo) <=                                                                                      \
   fminf(fminf(fminf(__builtin_fmaf(fx.c, ixs, fox), __builtin_fmaf(fy.c, iys, foy)), __builtin_fmaf(fz.c, izs, foz)), \
         ustar))
        const bool h0 = YK_QUERY_SLOT(x), h1 = YK_QUERY_SLOT(y), h2 = YK_QUERY_SLOT(z), h3 = YK_QUERY_SLOT(w);
#undef YK_QUERY_SLOT
        node = h3 ? ch.w : (h2 ? ch.z : (h1 ? ch.y : (h0 ? ch.x : popped)));
        stk[sp * kStride] = ch.x;
        sp += (h0 && (h1 || h2 || h3)) ? 1u : 0u;
        stk[sp * kStride] = ch.y;
        sp += (h1 && (h2 || h3)) ? 1u : 0u;
        stk[sp * kStride] = ch.z;
        sp += (h2 && h3) ? 1u : 0u;
        sp -= (h0 || h1 || h2 || h3) ? 0u : 1u;
        if (sp > q.stack_cap) {  // stack overflow: the ordered scan decides
          scan = true;
          break;
        }
      }
      if (scan) break;
      bool done = false;
      {
        const uint32_t v = ~(uint32_t)node, first = v >> 4, cnt = v & 15u;
        for (uint32_t k = 0; k < cnt; ++k) {
          const uint32_t slot = first + k;
          if (slot >= q.nspheres) break;  // (never: a leaf outside the table)
          const SphereGeo sg = q.leaf_geo[slot];
          const uint32_t id = q.leaf_ids[slot];
          ++h.tests;
          // the reference's discriminant and root, bit for bit (sphere.hpp:29-39)
          const v3 oc = {o.x - sg.cx, o.y - sg.cy, o.z - sg.cz};
          const double hb = ykd::dot(oc, d);
          const double cc = ykd::len2(oc) - sg.rr;
          const double disc = hb * hb - aa * cc;
          if (disc < 0) continue;
          const double sq = ykd::nsqrt(disc);
          double r = (-hb - sq) / aa;
          if (r < tmin) r = (-hb + sq) / aa;
          // the minimum root wins, an exact tie goes to the later tuple index; best_id = -1 with
          // best = t_max: a first root equal to t_max is accepted, as the scan accepts it
          if (r >= tmin && (r < best || (r == best && (int)id > best_id))) {
            best = r;
            best_id = (int)id;
            ustar = f32_up(best) * (1.0f + 0x1p-18f);
            if (any_hit) {
              done = true;
              break;
            }
          }
        }
      }
      if (done || sp == 0) break;  // (sp == 0: the sentinel was this leaf)
      --sp;
      node = stk[sp * kStride];
    }
  }
  h.t = best;
  h.id = best_id;
  if (live && scan) scan_hit(q, o, d, aa, tmin, tmax, any_hit, h);
  return h;
}

// the hit record (sphere.hpp:41-45, hittable.hpp:23-27) of the root t on the sphere (sg, radius)
struct HitRecord {
  v3 p, nrm;
  bool front;
};
__device__ __forceinline__ HitRecord hit_record(v3 o, v3 d, double t, const SphereGeo& sg, double radius) {
  const v3 p = ykd::add(o, ykd::mul(d, t));
  const v3 outward = ykd::divs(ykd::sub(p, v3{sg.cx, sg.cy, sg.cz}), radius);
  const bool front = ykd::dot(d, outward) < 0;
  return {p, front ? outward : ykd::neg(outward), front};
}

// a synchronous call's staging pair: `need` elements of sa and of sb bytes, grown on demand after
// wait_first (may be null: the work that may still read the pair)
int ensure_pair(void*& a, void*& b, size_t& cap, size_t need, size_t sa, size_t sb, hipEvent_t wait_first) {
  if (need <= cap) return YK_OK;
  if (wait_first) YK_HIP(hipEventSynchronize(wait_first));
  (void)hipFree(a);
  (void)hipFree(b);
  a = b = nullptr;
  cap = 0;
  YK_HIP(hipMalloc(&a, need * sa));
  YK_HIP(hipMalloc(&b, need * sb));
  cap = need;
  return YK_OK;
}

// the counters of a synchronous call, which the waves spread over `stripes` copies: their sums
hipError_t read_stripes(const unsigned long long* d, int stripes, int counters, unsigned long long* out) {
  std::vector<unsigned long long> h((size_t)stripes * counters);
  if (hipError_t e = hipMemcpy(h.data(), d, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost)) return e;
  for (int s = 0; s < stripes; ++s)
    for (int k = 0; k < counters; ++k) out[k] += h[(size_t)s * counters + k];
  return hipSuccess;
}

}  // namespace
}  // namespace ykquery

#endif
