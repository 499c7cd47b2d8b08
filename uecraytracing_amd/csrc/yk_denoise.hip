// yk_denoise.hip — ykgpu_film_denoise (include/ykgpu.h "film denoise"): a
// variance-guided non-local-means filter over a film's own tile, defined operation by operation in
// IEEE double so that numpy restates it bit for bit (tests/film_denoise_ref.py).
//
// A unit of its own.  Three kernels on the context's stream:
//   yk_film_moments  slot-order sums and second moments → pixel-order planes m_c, v_c
//   yk_film_nlm      the filter, one workgroup per 32 x 8 pixels, m and v of the block and its
//                    halo in LDS
//   yk_film_rgb8     to_color3b's steps after its division on the filtered mean
// and, for ykgpu_film_denoise_guided ("film features"), yk_film_nlm_guided in
// yk_film_nlm's place: the same filter with the weight bounded by the feature planes' distance.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <initializer_list>
#include <string>

#include "../../include/ykgpu.h"
#include "yk_device.hpp"
#include "yk_film_internal.hpp"
#include "yk_host_internal.hpp"

using namespace ykhost;

namespace {

constexpr uint32_t kMaxRadius = 10, kMaxPatch = 3;
// The block of output pixels of one workgroup.  32 wide: a wave is two rows of 32 threads, and the
// 32 lanes an 8-byte LDS read is serviced in (ds_read_b64: two groups of 32 lanes over 64 banks of
// 4 B) are one row — 32 consecutive doubles, every bank once — whatever the plane's pitch and
// whatever the window offset.
constexpr uint32_t kBlockW = 32, kBlockH = 8, kThreads = kBlockW * kBlockH;

// m_c = s_c / nd and v_c = max(0, (q_c - (s_c*s_c)/nd) / (nd*(nd - 1))) (film_e2's v_c) of every
// slot, gathered through the film's slot → pixel order into six pixel-order planes
// mv[c * npix + px] (m: c = 0..2, v: 3..5).  count (null for a uniform film): each slot's own n.
// *low receives the number of pixels whose count is below 2 (their planes are zeroed), reduced like
// yk_film_error's results: per thread, then lane exchanges, then one atomic per wave.
__global__ __launch_bounds__(256) void yk_film_moments(const double* plane, const uint32_t* order,
                                                      const uint32_t* count, double* mv, unsigned long long* low,
                                                      uint32_t npix_slots, uint32_t npix, uint32_t done) {
  unsigned long long below = 0;
  for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p < npix_slots; p += gridDim.x * blockDim.x) {
    const uint32_t px = order[p];
    if (px == kNoPixel) continue;
    const uint32_t np = count ? count[p] : done;
    const bool ok = np >= 2;
    below += ok ? 0u : 1u;
    const double nd = (double)np;
    const double den = film_mul(nd, film_sub(nd, 1.0));
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double s = plane[(size_t)c * npix_slots + p], q = plane[(size_t)(3 + c) * npix_slots + p];
      const double m = film_div(s, nd);
      const double v = film_div(film_sub(q, film_div(film_mul(s, s), nd)), den);
      mv[(size_t)c * npix + px] = ok ? m : 0.0;
      mv[(size_t)(3 + c) * npix + px] = ok && v > 0.0 ? v : 0.0;
    }
  }
  // (every lane reaches this point: the loop above has no early exit)
  for (int off = 32; off > 0; off >>= 1) below += __shfl_xor(below, off, 64);
  if ((threadIdx.x & 63u) == 0 && below) atomicAdd(low, below);
}

struct NlmArgs {
  const double* mv;  // yk_film_moments' planes
  double* out;       // rows * wt * 3, pixel order
  uint32_t rows, wt, npix;
  uint32_t radius, patch;
  double k2, alpha, eps, npatch;  // npatch = (double)(3 * (2F+1)^2)
};

// The filter.  With H = R + F, a workgroup keeps m_c and v_c of its block grown by H on every side
// in LDS — six planes of (8 + 2H) x (32 + 2H) doubles, the coordinates clamped to the tile at load,
// so that clamp(u) is simply position u — and two planes of (8 + 2F) x (32 + 2F) doubles for the
// patch terms.  For every window offset d, row-major:
//   1. the term ((t_r + t_g) + t_b)(u) between clamp(u) and clamp(u + d) for every u of the block
//      grown by F: with u = p + o the term of (p, o) depends on u alone, so it is computed once
//      (3 divisions) and not once per patch that covers it;
//   2. after a barrier, each thread sums the (2F+1)^2 terms of its pixel in patch order — the
//      additions of the definition in the definition's order — and folds w * m(q) into its
//      registers when q = p + d is inside the tile.
// The term planes alternate, so step 1 of the next offset may begin while other waves are still in
// step 2 of this one: one barrier per offset.  Offsets for which no pixel of the block has its
// neighbour inside the tile are skipped by the whole workgroup.
__global__ __launch_bounds__(kThreads) void yk_film_nlm(NlmArgs a) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int R = (int)a.radius, F = (int)a.patch, H = R + F;
  const int pw = (int)kBlockW + 2 * H, ph = (int)kBlockH + 2 * H;  // the six m / v planes
  const int tw = (int)kBlockW + 2 * F, th = (int)kBlockH + 2 * F;  // the term planes
  const int plane = pw * ph;
  double* const term = lds + 6 * plane;
  const int rows = (int)a.rows, wt = (int)a.wt;
  const int x0 = (int)(blockIdx.x * kBlockW), y0 = (int)(blockIdx.y * kBlockH);
  const int tid = (int)threadIdx.x;

  for (int i = tid; i < plane; i += (int)kThreads) {
    const int ly = i / pw, lx = i - ly * pw;
    int gy = y0 - H + ly, gx = x0 - H + lx;
    gy = gy < 0 ? 0 : gy > rows - 1 ? rows - 1 : gy;
    gx = gx < 0 ? 0 : gx > wt - 1 ? wt - 1 : gx;
    const size_t g = (size_t)gy * a.wt + gx;
#pragma unroll
    for (int c = 0; c < 6; ++c) lds[c * plane + i] = a.mv[(size_t)c * a.npix + g];
  }
  __syncthreads();

  const int tx = tid & (int)(kBlockW - 1), ty = tid / (int)kBlockW;
  const int py = y0 + ty, px = x0 + tx;
  const bool mine = py < rows && px < wt;
  // the rows and columns of the block that exist in the tile (for the whole-block skip)
  const int by1 = (y0 + (int)kBlockH < rows ? y0 + (int)kBlockH : rows) - 1;
  const int bx1 = (x0 + (int)kBlockW < wt ? x0 + (int)kBlockW : wt) - 1;
  double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0, wsum = 0.0;
  int buf = 0;
  for (int dy = -R; dy <= R; ++dy) {
    if (by1 + dy < 0 || y0 + dy > rows - 1) continue;  // (uniform over the workgroup)
    for (int dx = -R; dx <= R; ++dx) {
      if (bx1 + dx < 0 || x0 + dx > wt - 1) continue;  // (uniform over the workgroup)
      double* const t = term + buf * (tw * th);
      for (int i = tid; i < tw * th; i += (int)kThreads) {
        const int uy = i / tw, ux = i - uy * tw;
        const int ip = (uy + R) * pw + (ux + R);  // u in the m / v planes: the term plane starts at -F, they at -H
        const int iq = ip + dy * pw + dx;         // u + d
        double s3[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const double mp = lds[c * plane + ip], mq = lds[c * plane + iq];
          const double vp = lds[(3 + c) * plane + ip], vq = lds[(3 + c) * plane + iq];
          const double d = film_sub(mp, mq);
          const double num = film_sub(film_mul(d, d), film_mul(a.alpha, film_add(vp, vq < vp ? vq : vp)));
          const double den = film_add(a.eps, film_mul(a.k2, film_add(vp, vq)));
          s3[c] = film_div(num, den);
        }
        t[i] = film_add(film_add(s3[0], s3[1]), s3[2]);
      }
      __syncthreads();
      if (mine && py + dy >= 0 && py + dy < rows && px + dx >= 0 && px + dx < wt) {
        double S = 0.0;
        for (int oy = 0; oy <= 2 * F; ++oy)
          for (int ox = 0; ox <= 2 * F; ++ox) S = film_add(S, t[(ty + oy) * tw + tx + ox]);
        double D = film_div(S, a.npatch);
        D = D > 0.0 ? D : 0.0;
        double w = film_sub(1.0, film_mul(0.25, D));
        w = w > 0.0 ? w : 0.0;
        w = film_mul(film_mul(w, w), film_mul(w, w));
        const int iq = (ty + H + dy) * pw + tx + H + dx;
        acc0 = film_add(acc0, film_mul(w, lds[iq]));
        acc1 = film_add(acc1, film_mul(w, lds[plane + iq]));
        acc2 = film_add(acc2, film_mul(w, lds[2 * plane + iq]));
        wsum = film_add(wsum, w);
      }
      buf ^= 1;
    }
  }
  if (mine) {
    double* o = a.out + ((size_t)py * a.wt + px) * 3;
    o[0] = film_div(acc0, wsum);
    o[1] = film_div(acc1, wsum);
    o[2] = film_div(acc2, wsum);
  }
}

struct GuidedArgs {
  NlmArgs c;           // the colour side, exactly yk_film_nlm's
  const double* feat;  // kYkFeatPlanes planes of npix doubles (yk_features.hip)
  double k2, alpha, tau[3];
};

// yk_film_nlm with w = min(wf, wc) (include/ykgpu.h "film features"): the colour weight wc is
// computed by the same statements in the same order; the feature weight is pointwise, between p and
// q = p + d.  The feature planes stay in global memory: the ten planes the weight reads (F0..F6, V_A,
// V_N, V_Z) grown by R would take 60 KiB of LDS beside the colour planes' 46.6 KiB at the defaults,
// and at R = 10, F = 3 the colour planes alone take 101 KiB of the CU's 160 KiB, so one layout that
// holds for every (R, F) reads them through L2: at a fixed offset the 32 lanes of a row read 32
// consecutive doubles of each plane, and neighbouring offsets read the same lines again.  A thread
// keeps its own pixel's ten values in registers.  Where wc is 0 the weight is 0 whatever wf is
// (wf >= 0 is never below it), so those neighbours' planes are not read.
__global__ __launch_bounds__(kThreads) void yk_film_nlm_guided(GuidedArgs ga) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const NlmArgs& a = ga.c;
  const int R = (int)a.radius, F = (int)a.patch, H = R + F;
  const int pw = (int)kBlockW + 2 * H, ph = (int)kBlockH + 2 * H;  // the six m / v planes
  const int tw = (int)kBlockW + 2 * F, th = (int)kBlockH + 2 * F;  // the term planes
  const int plane = pw * ph;
  double* const term = lds + 6 * plane;
  const int rows = (int)a.rows, wt = (int)a.wt;
  const int x0 = (int)(blockIdx.x * kBlockW), y0 = (int)(blockIdx.y * kBlockH);
  const int tid = (int)threadIdx.x;

  for (int i = tid; i < plane; i += (int)kThreads) {
    const int ly = i / pw, lx = i - ly * pw;
    int gy = y0 - H + ly, gx = x0 - H + lx;
    gy = gy < 0 ? 0 : gy > rows - 1 ? rows - 1 : gy;
    gx = gx < 0 ? 0 : gx > wt - 1 ? wt - 1 : gx;
    const size_t g = (size_t)gy * a.wt + gx;
#pragma unroll
    for (int c = 0; c < 6; ++c) lds[c * plane + i] = a.mv[(size_t)c * a.npix + g];
  }
  __syncthreads();

  const int tx = tid & (int)(kBlockW - 1), ty = tid / (int)kBlockW;
  const int py = y0 + ty, px = x0 + tx;
  const bool mine = py < rows && px < wt;
  const int by1 = (y0 + (int)kBlockH < rows ? y0 + (int)kBlockH : rows) - 1;
  const int bx1 = (x0 + (int)kBlockW < wt ? x0 + (int)kBlockW : wt) - 1;
  // this pixel's features: F0..F6 and the three group variances (planes 14..16)
  double fp[kYkFeatChannels], vp[3];
  {
    const size_t g = mine ? (size_t)py * a.wt + px : 0;
#pragma unroll
    for (uint32_t c = 0; c < kYkFeatChannels; ++c) fp[c] = ga.feat[(size_t)c * a.npix + g];
#pragma unroll
    for (uint32_t k = 0; k < 3; ++k) vp[k] = ga.feat[(size_t)(14 + k) * a.npix + g];
  }
  double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0, wsum = 0.0;
  int buf = 0;
  for (int dy = -R; dy <= R; ++dy) {
    if (by1 + dy < 0 || y0 + dy > rows - 1) continue;  // (uniform over the workgroup)
    for (int dx = -R; dx <= R; ++dx) {
      if (bx1 + dx < 0 || x0 + dx > wt - 1) continue;  // (uniform over the workgroup)
      double* const t = term + buf * (tw * th);
      for (int i = tid; i < tw * th; i += (int)kThreads) {
        const int uy = i / tw, ux = i - uy * tw;
        const int ip = (uy + R) * pw + (ux + R);
        const int iq = ip + dy * pw + dx;
        double s3[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const double mp = lds[c * plane + ip], mq = lds[c * plane + iq];
          const double vpc = lds[(3 + c) * plane + ip], vq = lds[(3 + c) * plane + iq];
          const double d = film_sub(mp, mq);
          const double num = film_sub(film_mul(d, d), film_mul(a.alpha, film_add(vpc, vq < vpc ? vq : vpc)));
          const double den = film_add(a.eps, film_mul(a.k2, film_add(vpc, vq)));
          s3[c] = film_div(num, den);
        }
        t[i] = film_add(film_add(s3[0], s3[1]), s3[2]);
      }
      __syncthreads();
      if (mine && py + dy >= 0 && py + dy < rows && px + dx >= 0 && px + dx < wt) {
        double S = 0.0;
        for (int oy = 0; oy <= 2 * F; ++oy)
          for (int ox = 0; ox <= 2 * F; ++ox) S = film_add(S, t[(ty + oy) * tw + tx + ox]);
        double D = film_div(S, a.npatch);
        D = D > 0.0 ? D : 0.0;
        double wc = film_sub(1.0, film_mul(0.25, D));
        wc = wc > 0.0 ? wc : 0.0;
        wc = film_mul(film_mul(wc, wc), film_mul(wc, wc));
        double w = wc;
        if (wc > 0.0) {
          const size_t gq = (size_t)(py + dy) * a.wt + (size_t)(px + dx);
          double e[kYkFeatChannels];
#pragma unroll
          for (uint32_t c = 0; c < kYkFeatChannels; ++c) {
            const double dF = film_sub(fp[c], ga.feat[(size_t)c * a.npix + gq]);
            e[c] = film_mul(dF, dF);
          }
          const double E[3] = {film_add(film_add(e[0], e[1]), e[2]), film_add(film_add(e[3], e[4]), e[5]), e[6]};
          double DF = 0.0;
#pragma unroll
          for (uint32_t k = 0; k < 3; ++k) {
            const double vq = ga.feat[(size_t)(14 + k) * a.npix + gq];
            const double num = film_sub(E[k], film_mul(ga.alpha, film_add(vp[k], vq < vp[k] ? vq : vp[k])));
            const double den = film_add(ga.tau[k], film_mul(ga.k2, film_add(vp[k], vq)));
            const double phi = film_div(num, den);
            DF = DF > phi ? DF : phi;
          }
          double wf = film_sub(1.0, film_mul(0.25, DF));
          wf = wf > 0.0 ? wf : 0.0;
          wf = film_mul(film_mul(wf, wf), film_mul(wf, wf));
          w = wf < wc ? wf : wc;
        }
        const int iq = (ty + H + dy) * pw + tx + H + dx;
        acc0 = film_add(acc0, film_mul(w, lds[iq]));
        acc1 = film_add(acc1, film_mul(w, lds[plane + iq]));
        acc2 = film_add(acc2, film_mul(w, lds[2 * plane + iq]));
        wsum = film_add(wsum, w);
      }
      buf ^= 1;
    }
  }
  if (mine) {
    double* o = a.out + ((size_t)py * a.wt + px) * 3;
    o[0] = film_div(acc0, wsum);
    o[1] = film_div(acc1, wsum);
    o[2] = film_div(acc2, wsum);
  }
}

// ykgpu_film_resolve's steps after its division on n values: math::sqrt, clamp to [0, 0.999],
// * 256, truncate
__global__ __launch_bounds__(256) void yk_film_rgb8(const double* mean, uint8_t* rgb, uint64_t n) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    double v = ykd::nsqrt(mean[i]);
    v = (v < 0.0) ? 0.0 : (0.999 < v) ? 0.999 : v;
    rgb[i] = (uint8_t)(uint32_t)(v * 256);
  }
}

size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

size_t nlm_lds_bytes(uint32_t R, uint32_t F) {
  const size_t H = R + F;
  return (6 * (kBlockW + 2 * H) * (kBlockH + 2 * H) + 2 * (kBlockW + 2 * F) * (kBlockH + 2 * F)) * sizeof(double);
}

NlmArgs nlm_args(const double* mv, double* out, uint32_t rows, uint32_t wt, const yk_denoise_params& dp) {
  NlmArgs a{};
  a.mv = mv;
  a.out = out;
  a.rows = rows;
  a.wt = wt;
  a.npix = rows * wt;
  a.radius = dp.radius;
  a.patch = dp.patch;
  a.k2 = dp.k2;
  a.alpha = dp.alpha;
  a.eps = dp.eps;
  a.npatch = (double)(3 * (2 * dp.patch + 1) * (2 * dp.patch + 1));
  return a;
}

GuidedArgs guided_args(const NlmArgs& a, const double* feat, const yk_feature_params& fp) {
  GuidedArgs g{};
  g.c = a;
  g.feat = feat;
  g.k2 = fp.k2;
  g.alpha = fp.alpha;
  g.tau[0] = fp.tau_albedo;
  g.tau[1] = fp.tau_normal;
  g.tau[2] = fp.tau_depth;
  return g;
}

}  // namespace

int ykhost::denoise_params_check(const yk_denoise_params& dp) {
  if (dp.radius > kMaxRadius) return fail(YK_ERR_INVALID, "denoise: radius must be <= 10");
  if (dp.patch > kMaxPatch) return fail(YK_ERR_INVALID, "denoise: patch must be <= 3");
  if (!(dp.k2 > 0) || !std::isfinite(dp.k2)) return fail(YK_ERR_INVALID, "denoise: k2 must be finite and > 0");
  if (!(dp.alpha >= 0) || !std::isfinite(dp.alpha)) return fail(YK_ERR_INVALID, "denoise: alpha must be finite and >= 0");
  if (!(dp.eps > 0) || !std::isfinite(dp.eps)) return fail(YK_ERR_INVALID, "denoise: eps must be finite and > 0");
  return YK_OK;
}

int ykhost::feature_params_check(const yk_feature_params& fp) {
  if (fp.grid < 1 || fp.grid > 4) return fail(YK_ERR_INVALID, "features: grid must be 1..4");
  if (fp.reserved) return fail(YK_ERR_INVALID, "features: reserved must be 0");
  if (!(fp.k2 > 0) || !std::isfinite(fp.k2)) return fail(YK_ERR_INVALID, "features: k2 must be finite and > 0");
  if (!(fp.alpha >= 0) || !std::isfinite(fp.alpha)) return fail(YK_ERR_INVALID, "features: alpha must be finite and >= 0");
  for (double tau : {fp.tau_albedo, fp.tau_normal, fp.tau_depth})
    if (!(tau > 0)) return fail(YK_ERR_INVALID, "features: tau must be > 0 (+inf switches a group off)");
  return YK_OK;
}

// [m, v planes: 6 npix doubles][out: 3 npix doubles][rgb: 3 npix bytes][low]
int ykhost::denoise_buffers(ykgpu_film* film, DenoiseBufs* out) {
  const size_t npix = (size_t)film->p.row_count * tile_width(&film->p);
  const size_t off_out = align256(6 * npix * sizeof(double)), off_rgb = off_out + align256(3 * npix * sizeof(double));
  const size_t off_low = off_rgb + align256(3 * npix), bytes = off_low + 256;
  if (!film->d_denoise) YK_HIP(hipMalloc(&film->d_denoise, bytes));  // (a film's tile never changes size)
  char* const base = (char*)film->d_denoise;
  out->mv = (double*)base;
  out->out = (double*)(base + off_out);
  out->rgb = (uint8_t*)(base + off_rgb);
  out->low = (unsigned long long*)(base + off_low);
  return YK_OK;
}

// ---- the steps of a group film's filter (yk_group.hip) -------------------------
hipError_t ykhost::denoise_moments_enqueue(ykgpu_film* film, const DenoiseBufs& b) {
  const hipStream_t stream = film->ctx->stream;
  hipError_t e = hipMemsetAsync(b.low, 0, sizeof(unsigned long long), stream);
  if (e != hipSuccess) return e;
  const uint32_t blocks = std::max(1u, std::min((film->nps + 255) / 256, 2048u));
  hipLaunchKernelGGL(yk_film_moments, dim3(blocks), dim3(256), 0, stream, film->d_plane, film->d_order,
                     film_counts(film), b.mv, b.low, film->nps, (uint32_t)film->npix, film->done);
  return hipGetLastError();
}

// The band entry: the band film's tile is the band grown by the halo, and the kernels run on it as
// on a tile of their own (the clamps fire only where the band's edge is the tile's edge).
hipError_t ykhost::denoise_band_enqueue(ykgpu_film* band, const DenoiseBufs& b, const yk_denoise_params& dp,
                                        const yk_feature_params* fp, const double* feat, uint32_t r0, uint32_t n,
                                        bool want_rgb) {
  const hipStream_t stream = band->ctx->stream;
  const uint32_t rows = band->p.row_count, wt = tile_width(&band->p);
  const NlmArgs a = nlm_args(b.mv, b.out, rows, wt, dp);
  const dim3 grid((wt + kBlockW - 1) / kBlockW, (rows + kBlockH - 1) / kBlockH);
  const size_t lds = nlm_lds_bytes(dp.radius, dp.patch);
  // (per call: the attribute belongs to the current device)
  hipError_t e = hipFuncSetAttribute(fp ? (const void*)yk_film_nlm_guided : (const void*)yk_film_nlm,
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)nlm_lds_bytes(kMaxRadius, kMaxPatch));
  if (e != hipSuccess) return e;
  if (fp)
    hipLaunchKernelGGL(yk_film_nlm_guided, grid, dim3(kThreads), lds, stream, guided_args(a, feat, *fp));
  else
    hipLaunchKernelGGL(yk_film_nlm, grid, dim3(kThreads), lds, stream, a);
  e = hipGetLastError();
  if (e == hipSuccess && want_rgb && n) {
    const size_t off = (size_t)r0 * wt * 3, cnt = (size_t)n * wt * 3;
    const uint32_t blocks = (uint32_t)std::max<size_t>(1, std::min<size_t>((cnt + 255) / 256, 2048));
    hipLaunchKernelGGL(yk_film_rgb8, dim3(blocks), dim3(256), 0, stream, b.out + off, b.rgb + off, (uint64_t)cnt);
    e = hipGetLastError();
  }
  return e;
}

namespace {

// The body of both denoise entry points: the checks, the film's denoise buffers, the moments, the
// caller's filter, the RGB8 conversion and the read-back.  `name` is the entry point's, for the
// error text.  The callers differ in three steps:
//   feature_checks()          after the colour parameters' checks and before the other checks
//                             (guided: the feature parameters and the scene's generation)
//   prepare()                 after every check: the filter kernel's dynamic-LDS attribute (per call:
//                             the attribute belongs to the current device; guided: the feature
//                             planes first)
//   filter(a, grid, lds, st)  enqueues the filter on st and returns the launch's error
// stats (may be null) receives moments_ms, filter_ms and total_ms.
template <typename Checks, typename Prepare, typename Filter>
int denoise_call(ykgpu_film* film, const char* name, const yk_denoise_params& dp, double* mean_host, uint8_t* rgb_host,
                 yk_denoise_stats* stats, Checks&& feature_checks, Prepare&& prepare, Filter&& filter) {
  const auto t0 = std::chrono::steady_clock::now();
  if (int rc = film_ready(film)) return rc;
  if (int rc = denoise_params_check(dp)) return rc;
  if (int rc = feature_checks()) return rc;
  if (!mean_host && !rgb_host) return fail(YK_ERR_INVALID, "denoise: mean_host and rgb_host are both null");
  if (!film_consecutive(film))
    return fail(YK_ERR_UNSUPPORTED, "denoise: the film's tile is not consecutive image rows and columns");
  const uint32_t* const count = film_counts(film);
  if (!count && film->done < 2) return fail(YK_ERR_INVALID, "denoise needs at least two samples in every pixel");

  YK_HIP(hipSetDevice(film->device));
  if (int rc = prepare()) return rc;
  const uint32_t rows = film->p.row_count, wt = tile_width(&film->p);
  const hipStream_t stream = film->ctx->stream;  // (film calls are synchronous on it)
  const size_t npix = (size_t)rows * wt;
  DenoiseBufs bufs{};
  if (int rc = denoise_buffers(film, &bufs)) return rc;
  double* const d_mv = bufs.mv;
  double* const d_out = bufs.out;
  uint8_t* const d_rgb = bufs.rgb;
  unsigned long long* const d_low = bufs.low;

  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
  hipError_t e = hipSuccess;
  for (int k = 0; k < 3 && stats && e == hipSuccess; ++k) e = hipEventCreate(&ev[k]);
  const auto record = [&](int k) {
    if (stats && e == hipSuccess) e = hipEventRecord(ev[k], stream);
  };
  unsigned long long low = 0;
  if (e == hipSuccess) e = hipMemsetAsync(d_low, 0, sizeof low, stream);
  record(0);
  if (e == hipSuccess) {
    const uint32_t blocks = std::max(1u, std::min((film->nps + 255) / 256, 2048u));
    hipLaunchKernelGGL(yk_film_moments, dim3(blocks), dim3(256), 0, stream, film->d_plane, film->d_order, count, d_mv,
                       d_low, film->nps, (uint32_t)npix, film->done);
    e = hipGetLastError();
  }
  record(1);
  // (the filter does not depend on the verdict: it is enqueued behind the moments, and its result
  // is dropped if a count turns out to be below 2)
  if (e == hipSuccess) {
    const NlmArgs a = nlm_args(d_mv, d_out, rows, wt, dp);
    const dim3 grid((wt + kBlockW - 1) / kBlockW, (rows + kBlockH - 1) / kBlockH);
    e = filter(a, grid, nlm_lds_bytes(dp.radius, dp.patch), stream);
  }
  if (e == hipSuccess && rgb_host) {
    const uint32_t blocks = (uint32_t)std::max<size_t>(1, std::min<size_t>((3 * npix + 255) / 256, 2048));
    hipLaunchKernelGGL(yk_film_rgb8, dim3(blocks), dim3(256), 0, stream, d_out, d_rgb, (uint64_t)(3 * npix));
    e = hipGetLastError();
  }
  record(2);
  if (e == hipSuccess) e = hipMemcpyAsync(&low, d_low, sizeof low, hipMemcpyDeviceToHost, stream);
  if (e == hipSuccess) e = hipStreamSynchronize(stream);
  // (the outputs are written only once the call is known to succeed)
  if (e == hipSuccess && low == 0) {
    if (mean_host) e = hipMemcpyAsync(mean_host, d_out, 3 * npix * sizeof(double), hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess && rgb_host) e = hipMemcpyAsync(rgb_host, d_rgb, 3 * npix, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
  }
  float ms_m = 0, ms_f = 0;
  if (stats && e == hipSuccess) e = hipEventElapsedTime(&ms_m, ev[0], ev[1]);
  if (stats && e == hipSuccess) e = hipEventElapsedTime(&ms_f, ev[1], ev[2]);
  for (hipEvent_t v : ev)
    if (v) (void)hipEventDestroy(v);
  if (e != hipSuccess)
    return fail(e == hipErrorOutOfMemory ? YK_ERR_NOMEM : YK_ERR_DEVICE, std::string(name) + ": " + hipGetErrorString(e));
  if (low) return fail(YK_ERR_INVALID, "denoise needs at least two samples in every pixel");
  if (stats) {
    stats->moments_ms = ms_m;
    stats->filter_ms = ms_f;
    stats->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  }
  return YK_OK;
}

// Both guided entry points: the filter over the pinhole planes at fp.grid (n_samples == 0) or over
// the sampled planes of the film's first n_samples samples (fp.grid ignored).
int guided_call(ykgpu_film* film, const char* name, const yk_denoise_params& dp, yk_feature_params fp, uint32_t n_samples,
                bool sampled, double* mean_host, uint8_t* rgb_host, yk_guided_stats* stats) {
  if (sampled) fp.grid = 1;  // (not read, so not validated)
  const double* d_feat = nullptr;
  double ms_feat = 0;
  yk_denoise_stats ds{};
  const int rc = denoise_call(
      film, name, dp, mean_host, rgb_host, stats ? &ds : nullptr,
      [&]() -> int {
        if (int rc = feature_params_check(fp)) return rc;
        if (sampled) return yk_film_features_sampled_check(film, n_samples);
        if (film->scene_gen != film->ctx->scene_gen)
          return fail(YK_ERR_INVALID, "the context's scene was set after the film was created");
        return YK_OK;
      },
      [&]() -> int {
        if (sampled) {
          yk_sampled_features_stats fs{};
          if (int rc = yk_film_features_sampled_ensure(film, n_samples, &d_feat, &fs)) return rc;
          ms_feat = fs.ms;
        } else if (int rc = yk_film_features_ensure(film, fp.grid, &d_feat, &ms_feat)) {
          return rc;
        }
        YK_HIP(hipFuncSetAttribute((const void*)yk_film_nlm_guided, hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)nlm_lds_bytes(kMaxRadius, kMaxPatch)));
        return YK_OK;
      },
      [&](const NlmArgs& a, dim3 grid, size_t lds, hipStream_t st) {
        const GuidedArgs g = guided_args(a, d_feat, fp);
        hipLaunchKernelGGL(yk_film_nlm_guided, grid, dim3(kThreads), lds, st, g);
        return hipGetLastError();
      });
  if (!rc && stats) {
    stats->features_ms = ms_feat;
    stats->moments_ms = ds.moments_ms;
    stats->filter_ms = ds.filter_ms;
    stats->total_ms = ds.total_ms;
  }
  return rc;
}

}  // namespace

extern "C" {

int yk_denoise_defaults(yk_denoise_params* out) {
  if (!out) return fail(YK_ERR_INVALID, "null out");
  out->radius = 5;
  out->patch = 1;
  out->k2 = 0.5;
  out->alpha = 1.0;
  out->eps = 1e-10;
  return YK_OK;
}

int ykgpu_film_denoise(ykgpu_film* film, const yk_denoise_params* params, double* mean_host, uint8_t* rgb_host,
                       yk_denoise_stats* stats) {
  yk_denoise_params dp;
  yk_denoise_defaults(&dp);
  if (params) dp = *params;
  return denoise_call(
      film, "ykgpu_film_denoise", dp, mean_host, rgb_host, stats, [] { return YK_OK; },
      []() -> int {
        YK_HIP(hipFuncSetAttribute((const void*)yk_film_nlm, hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)nlm_lds_bytes(kMaxRadius, kMaxPatch)));
        return YK_OK;
      },
      [](const NlmArgs& a, dim3 grid, size_t lds, hipStream_t st) {
        hipLaunchKernelGGL(yk_film_nlm, grid, dim3(kThreads), lds, st, a);
        return hipGetLastError();
      });
}

int yk_guided_defaults(yk_denoise_params* colour, yk_feature_params* feat) {
  if (!colour && !feat) return fail(YK_ERR_INVALID, "null out");
  if (colour) {
    yk_denoise_defaults(colour);
    colour->k2 = 2.0;  // the pair of DESIGN.md §6.4 (tools/features_tune.py)
  }
  if (feat) {
    feat->grid = 2;
    feat->reserved = 0;
    feat->k2 = 2.0;
    feat->alpha = 1.0;
    feat->tau_albedo = 1e-2;
    feat->tau_normal = 1e-1;
    feat->tau_depth = 1e-2;
  }
  return YK_OK;
}

int yk_guided_sampled_defaults(yk_denoise_params* colour, yk_feature_params* feat, uint32_t* n_samples) {
  if (!colour && !feat && !n_samples) return fail(YK_ERR_INVALID, "null out");
  // the point of DESIGN.md §6.8 (tools/features_sampled_tune.py)
  if (colour || feat) yk_guided_defaults(colour, feat);
  if (n_samples) *n_samples = 16;
  return YK_OK;
}

int ykgpu_film_denoise_guided(ykgpu_film* film, const yk_denoise_params* params, const yk_feature_params* fparams,
                              double* mean_host, uint8_t* rgb_host, yk_guided_stats* stats) {
  yk_denoise_params dp;
  yk_feature_params fp;
  yk_guided_defaults(&dp, &fp);
  if (params) dp = *params;
  if (fparams) fp = *fparams;
  return guided_call(film, "ykgpu_film_denoise_guided", dp, fp, 0, false, mean_host, rgb_host, stats);
}

int ykgpu_film_denoise_guided_sampled(ykgpu_film* film, const yk_denoise_params* params, const yk_feature_params* fparams,
                                      uint32_t n_samples, double* mean_host, uint8_t* rgb_host, yk_guided_stats* stats) {
  yk_denoise_params dp;
  yk_feature_params fp;
  yk_guided_sampled_defaults(&dp, &fp, nullptr);
  if (params) dp = *params;
  if (fparams) fp = *fparams;
  return guided_call(film, "ykgpu_film_denoise_guided_sampled", dp, fp, n_samples, true, mean_host, rgb_host, stats);
}

}  // extern "C"
