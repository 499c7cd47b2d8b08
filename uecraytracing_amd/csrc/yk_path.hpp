// yk_path.hpp — the device helpers both path kernels (yk_render_f64.hip, yk_render_f32.hip) use: the
// launch's clock probe, the traced rays, the slab tests, the candidate list, the per-sample engines
// and the slot claims of the persistent loop.
#ifndef YK_PATH_HPP
#define YK_PATH_HPP

#include <type_traits>

#include "yk_render_device.hpp"
#include "yk_stamps.hpp"

namespace {

// Shader-clock probe of a launch: thread 0 of block 0 stores s_memtime (the shader clock) and
// s_memrealtime (100 MHz) when it starts and when it leaves the loop (vector stores, nothing held
// in registers across the loop) — the clock the launch ran at (ykgpu_get_stats sclk_mhz; the
// per-launch timeline).
#define YK_CLOCK_STAMP(ka, k)                                                              \
  do {                                                                                     \
    if (blockIdx.x == 0 && threadIdx.x == 0) {                                             \
      (ka).clk[(k)] = __builtin_amdgcn_s_memtime();                                        \
      (ka).clk[(k) + 1] = __builtin_amdgcn_s_memrealtime();                                \
    }                                                                                      \
  } while (0)
#define YK_CLOCK_BEGIN(ka) YK_CLOCK_STAMP(ka, 0)
#define YK_CLOCK_END(ka) YK_CLOCK_STAMP(ka, 2)

// -l 3 (raytracer.hpp:21-25): ray k of the path of the lane's sample slot (counting instance)
template <class V>
__device__ __forceinline__ void trace_ray(const KernelArgs& ka, uint32_t slot, uint32_t k, V o, V d) {
  const uint32_t sl = slot / ka.npix_slots, q = ka.order[slot - sl * ka.npix_slots];
  const size_t idx = (size_t)q * ka.spp + ka.s0 + sl;
  if (k < ka.trace_cap) {
    double* r = ka.trace + (idx * ka.trace_cap + k) * 6;
    r[0] = o.x, r[1] = o.y, r[2] = o.z, r[3] = d.x, r[4] = d.y, r[5] = d.z;
  }
  ka.trace_counts[idx] = k + 1;
}

struct Hit {
  double T;
  int hid;
  uint32_t tests, sqrts;
  uint32_t ncalls, nits;  // math::sqrt calls / loop iterations
};

typedef float f2 __attribute__((ext_vector_type(2)));
typedef float f4 __attribute__((ext_vector_type(4)));

#include "yk_slab.hpp"

// Candidate list entry insertion with static register indexing (no scratch).
#define YK_CAND_SET(K, ID, LB) \
  do {                         \
    if ((K) == 0) { c0 = ID; l0 = LB; }       \
    else if ((K) == 1) { c1 = ID; l1 = LB; }  \
    else if ((K) == 2) { c2 = ID; l2 = LB; }  \
    else { c3 = ID; l3 = LB; }                \
  } while (0)

// Refill of the persistent kernels: lanes without a path take the next sample slots from the
// wave's reserve, one atomic per kClaim slots.  Every lane runs it, so the reserve (res_base,
// res_left) stays wave-uniform.  (A pixel is not a lane's unit of work: the samples of a pixel
// are independent, only their SUM is ordered, and yk_reduce_samples does that.)  Returns true
// when this lane has no path and the launch has no slots left: the lane exits.
// The per-sample engine of a kernel instance (YK_RNG_*): lane set-up.
__device__ __forceinline__ void rng_init(ykd::MtLane& g, const KernelArgs& ka, uint32_t gid) {
  g.state = ka.mt_scratch + (size_t)gid * ykd::kMtN;
  g.a0 = g.a1 = g.b = g.j = g.seed = 0;
}
__device__ __forceinline__ void rng_init(ykd::X128Lane& g, const KernelArgs&, uint32_t) { g.x = g.y = g.z = g.w = g.n = 0; }

// A sample's engine from its seed alone (xor128, and an mt19937 start no StartRec serves):
// mt19937 walks its 397 seeding steps here
__device__ __forceinline__ void rng_start_full(ykd::MtLane& g, uint32_t seed) { ykd::mt_start(g, seed); }
__device__ __forceinline__ void rng_start_full(ykd::X128Lane& g, uint32_t seed) { ykd::x128_start(g, seed); }

__device__ __forceinline__ bool claim_slots(const KernelArgs& ka, bool in_path, uint32_t lane, uint32_t& slot,
                                            uint32_t& res_base, uint32_t& res_left) {
  const unsigned long long m = __ballot(!in_path);
  if (m) {
    const uint32_t need = (uint32_t)__popcll(m);
    uint32_t fresh = 0, csize = kClaim;
    if (res_left < need) {
      if (kClaimTail) {
        // res_base + res_left: where the counter stood after this wave's last claim
        const uint32_t seen = res_base + res_left;
        const uint32_t tail = ka.claim_tail;  // (the host's: no dispatch-packet load, no vmcnt wait)
        if (seen >= ka.nsl || ka.nsl - seen < tail) csize = kClaimTail;
      }
      const int leader = __ffsll((long long)m) - 1;
      if ((int)lane == leader) fresh = atomicAdd(ka.pixel_counter, csize);
      fresh = __builtin_amdgcn_readlane(fresh, leader);  // (the leader is wave-uniform)
    }
    if (!in_path) {
      const uint32_t r = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
      slot = r < res_left ? res_base + r : fresh + (r - res_left);
    }
    if (res_left < need) {
      res_base = fresh + (need - res_left);
      res_left = csize - (need - res_left);
    } else {
      res_base += need;
      res_left -= need;
    }
  }
  return !in_path && slot >= ka.nsl;
}

}  // namespace

#endif
