// yk_features.hip — ykgpu_film_features (include/ykgpu.h "film features"): the
// first-hit albedo, normal and depth of every pixel of a film's tile, defined operation by operation
// in IEEE double so that numpy restates it bit for bit (tests/film_features_ref.py).
//
// A unit of its own, like yk_denoise.hip: the render unit's kernels compile exactly as before, and
// this one reaches a film only through yk_film_view (yk_film_internal.hpp).  One kernel,
// yk_film_features, on the context's stream; its result lives in planes the film owns and is
// computed once per (film, grid).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/ykgpu.h"
#include "yk_device.hpp"
#include "yk_film_internal.hpp"

namespace {

using ykd::v3;

constexpr uint32_t kMaxGrid = 4;
// The block of pixels of one workgroup, yk_film_nlm's: a wave is two rows of 32 pixels.
constexpr uint32_t kBlockW = 32, kBlockH = 8, kThreads = kBlockW * kBlockH;
// Spheres staged in LDS at a time: 4 doubles each, 16 KiB a workgroup (ten workgroups fit a CU's
// 160 KiB, more than its waves allow), and the final scene's 485 spheres are one chunk.
constexpr uint32_t kChunk = 512;

#define YKF_HIP(call)                                                                             \
  do {                                                                                            \
    hipError_t e_ = (call);                                                                       \
    if (e_ != hipSuccess)                                                                         \
      return yk_film_fail(e_ == hipErrorOutOfMemory ? YK_ERR_NOMEM : YK_ERR_DEVICE,               \
                          (std::string(#call) + ": " + hipGetErrorString(e_)).c_str());           \
  } while (0)

struct FeatArgs {
  yk_camera cam;
  const double* geo;         // cx, cy, cz, radius*radius per sphere
  const unsigned char* mat;  // kYkMatStride bytes per sphere
  double* out;               // kYkFeatPlanes planes of npix doubles
  double t_min;
  uint32_t nspheres, grid;
  uint32_t W, H, rows, wt, npix;
  uint32_t row_begin, row_stride, row_band, col_begin, col_stride, col_band;
};

__device__ __forceinline__ v3 ld3(const double* p) { return {p[0], p[1], p[2]}; }

// One thread per pixel of the tile, its g x g sub-rays one after the other, row-major, the sums of
// f and f*f in registers: the fold order is the definition's.  Every ray leaves the camera's origin,
// so oc = o - c and cc = len2(oc) - r*r of sphere_hit are the same for every ray: the thread that
// stages a sphere computes them (the same operations on the same operands), and the scan reads
// (oc, cc) — all lanes the same sphere, a broadcast LDS read — and is left with half_b and disc.
// The square root and the roots are taken only where a wave has a lane with disc >= 0.  The scan
// keeps the closest root and its index alone; the hit record is computed from them afterwards
// (rec.p, outward and the normal depend on nothing else).  A scene larger than a chunk is staged
// chunk by chunk for every sub-ray, in index order, so the ordered scan stays ordered.
__global__ __launch_bounds__(kThreads) void yk_film_features(FeatArgs a) {
  __shared__ __attribute__((aligned(16))) double lds[kChunk * 4];
  const uint32_t tid = threadIdx.x;
  const uint32_t tx = tid & (kBlockW - 1), ty = tid / kBlockW;
  const uint32_t px = blockIdx.x * kBlockW + tx, py = blockIdx.y * kBlockH + ty;
  const bool mine = py < a.rows && px < a.wt;
  // (a thread outside the tile walks the scan with the tile's last pixel: it takes part in the
  // barriers and the ballots, and stores nothing)
  const uint32_t tj = px < a.wt ? px : a.wt - 1, ti = py < a.rows ? py : a.rows - 1;
  const uint32_t x = a.col_begin + (((tj >> a.col_band) * a.col_stride) << a.col_band) + (tj & ((1u << a.col_band) - 1u));
  const uint32_t y = a.row_begin + (((ti >> a.row_band) * a.row_stride) << a.row_band) + (ti & ((1u << a.row_band) - 1u));
  const v3 o = ld3(a.cam.origin), llc = ld3(a.cam.lower_left_corner);
  const v3 hor = ld3(a.cam.horizontal), ver = ld3(a.cam.vertical);
  const uint32_t n = a.nspheres, g = a.grid;
  const bool one_chunk = n <= kChunk;
  const double gd = (double)g, wd = (double)a.W, hd = (double)a.H;

  double s[kYkFeatChannels], q[kYkFeatChannels];
#pragma unroll
  for (uint32_t c = 0; c < kYkFeatChannels; ++c) s[c] = q[c] = 0.0;

  for (uint32_t i = 0; i < g; ++i) {
    for (uint32_t j = 0; j < g; ++j) {
      const double sa = film_div(film_add((double)j, 0.5), gd);
      const double sb = film_div(film_add((double)i, 0.5), gd);
      const double u = film_div(film_add((double)x, sa), wd);
      const double v = film_div(film_add((double)(a.H - y - 1), sb), hd);
      // camera::get_ray's pinhole branch (camera.hpp:29-32)
      const v3 d = ykd::sub(ykd::add(ykd::add(llc, ykd::mul(hor, u)), ykd::mul(ver, v)), o);
      const double aa = ykd::len2(d);
      double closest = INFINITY;
      int hid = -1;
      for (uint32_t base = 0; base < n; base += kChunk) {
        const uint32_t cnt = n - base < kChunk ? n - base : kChunk;
        if (!one_chunk || (i == 0 && j == 0)) {
          __syncthreads();  // (every wave has left the chunk before)
          for (uint32_t k = tid; k < cnt; k += kThreads) {
            const double* sg = a.geo + (size_t)(base + k) * 4;
            const v3 oc = ykd::sub(o, v3{sg[0], sg[1], sg[2]});
            lds[4 * k + 0] = oc.x;
            lds[4 * k + 1] = oc.y;
            lds[4 * k + 2] = oc.z;
            lds[4 * k + 3] = ykd::len2(oc) - sg[3];
          }
          __syncthreads();
        }
        for (uint32_t k = 0; k < cnt; ++k) {
          // sphere::hit_impl (sphere.hpp:25-48) from half_b on
          const v3 oc = {lds[4 * k + 0], lds[4 * k + 1], lds[4 * k + 2]};
          const double half_b = ykd::dot(oc, d);
          const double disc = half_b * half_b - aa * lds[4 * k + 3];
          const bool live = !(disc < 0);
          if (__ballot(live) == 0) continue;  // (uniform over the wave)
          // (a lane without a root takes the square root of 1: the iteration on a negative number
          // does not settle)
          const double sq = ykd::nsqrt(live ? disc : 1.0);
          double root = (-half_b - sq) / aa;
          bool ok = live;
          if (root < a.t_min || closest < root) {
            root = (-half_b + sq) / aa;
            if (root < a.t_min || closest < root) ok = false;
          }
          if (ok) {  // hittable_list::hit_impl: the last accepted object wins, ties included
            closest = root;
            hid = (int)(base + k);
          }
        }
      }
      double f[kYkFeatChannels] = {1.0, 1.0, 1.0, 0.0, 0.0, 0.0, 0.0};
      if (hid >= 0) {
        const double* sg = a.geo + (size_t)hid * 4;
        const unsigned char* m = a.mat + (size_t)hid * kYkMatStride;
        const double radius = *(const double*)(m + kYkMatRadius);
        const uint32_t kind = *(const uint32_t*)(m + kYkMatKind);
        const double* alb = (const double*)(m + kYkMatAlbedo);
        // hit record (sphere.hpp:41-45, hittable.hpp:23-27)
        const v3 p = ykd::add(o, ykd::mul(d, closest));
        const v3 outward = ykd::divs(ykd::sub(p, v3{sg[0], sg[1], sg[2]}), radius);
        const bool front = ykd::dot(d, outward) < 0;
        const v3 nrm = front ? outward : ykd::neg(outward);
        if (kind != YK_MATERIAL_DIELECTRIC) {
          f[0] = alb[0];
          f[1] = alb[1];
          f[2] = alb[2];
        }
        f[3] = nrm.x;
        f[4] = nrm.y;
        f[5] = nrm.z;
        f[6] = closest;
      }
#pragma unroll
      for (uint32_t c = 0; c < kYkFeatChannels; ++c) {
        s[c] = film_add(s[c], f[c]);
        q[c] = film_add(q[c], film_mul(f[c], f[c]));
      }
    }
  }
  if (!mine) return;
  const double G = (double)(g * g);
  const double den = film_mul(G, film_sub(G, 1.0));
  double U[kYkFeatChannels];
  const size_t at = (size_t)py * a.wt + px;
#pragma unroll
  for (uint32_t c = 0; c < kYkFeatChannels; ++c) {
    const double var = film_div(film_sub(q[c], film_div(film_mul(s[c], s[c]), G)), den);
    U[c] = g >= 2 && var > 0.0 ? var : 0.0;
    a.out[(size_t)c * a.npix + at] = film_div(s[c], G);
    a.out[(size_t)(kYkFeatChannels + c) * a.npix + at] = U[c];
  }
  a.out[(size_t)14 * a.npix + at] = film_add(film_add(U[0], U[1]), U[2]);
  a.out[(size_t)15 * a.npix + at] = film_add(film_add(U[3], U[4]), U[5]);
  a.out[(size_t)16 * a.npix + at] = U[6];
}

}  // namespace

int yk_film_features_ensure(const yk_film_view& f, uint32_t grid, const double** planes, double* ms) {
  if (grid < 1 || grid > kMaxGrid) return yk_film_fail(YK_ERR_INVALID, "features: grid must be 1..4");
  if (f.stale) return yk_film_fail(YK_ERR_INVALID, "the context's scene was set after the film was created");
  YKF_HIP(hipSetDevice(f.device));
  const size_t npix = (size_t)f.rows * f.wt;
  if (!*f.features) {  // (a film's tile never changes size)
    *f.feature_grid = 0;
    YKF_HIP(hipMalloc(f.features, kYkFeatPlanes * npix * sizeof(double)));
  }
  *planes = (const double*)*f.features;
  if (ms) *ms = 0.0;
  if (*f.feature_grid == grid) return YK_OK;
  *f.feature_grid = 0;  // (until the pass is whole)
  FeatArgs a{};
  a.cam = f.cam;
  a.geo = f.geo;
  a.mat = f.mat;
  a.out = (double*)*f.features;
  a.t_min = f.t_min;
  a.nspheres = f.nspheres;
  a.grid = grid;
  a.W = f.W;
  a.H = f.H;
  a.rows = f.rows;
  a.wt = f.wt;
  a.npix = (uint32_t)npix;
  a.row_begin = f.row_begin;
  a.row_stride = f.row_stride;
  a.row_band = f.row_band;
  a.col_begin = f.col_begin;
  a.col_stride = f.col_stride;
  a.col_band = f.col_band;
  hipEvent_t ev[2] = {nullptr, nullptr};
  hipError_t e = hipEventCreate(&ev[0]);
  if (e == hipSuccess) e = hipEventCreate(&ev[1]);
  if (e == hipSuccess) e = hipEventRecord(ev[0], f.stream);
  if (e == hipSuccess) {
    const dim3 blocks((f.wt + kBlockW - 1) / kBlockW, (f.rows + kBlockH - 1) / kBlockH);
    hipLaunchKernelGGL(yk_film_features, blocks, dim3(kThreads), 0, f.stream, a);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipEventRecord(ev[1], f.stream);
  if (e == hipSuccess) e = hipStreamSynchronize(f.stream);
  float t = 0;
  if (e == hipSuccess) e = hipEventElapsedTime(&t, ev[0], ev[1]);
  for (hipEvent_t v : ev)
    if (v) (void)hipEventDestroy(v);
  if (e != hipSuccess)
    return yk_film_fail(e == hipErrorOutOfMemory ? YK_ERR_NOMEM : YK_ERR_DEVICE,
                        (std::string("ykgpu_film_features: ") + hipGetErrorString(e)).c_str());
  *f.feature_grid = grid;
  if (ms) *ms = t;
  return YK_OK;
}

extern "C" {

int ykgpu_film_features(ykgpu_film* film, uint32_t grid, double* mean_host, double* var_host, double* ms) {
  yk_film_view f{};
  if (int rc = yk_film_view_of(film, &f)) return rc;
  const double* planes = nullptr;
  double t = 0;
  if (int rc = yk_film_features_ensure(f, grid, &planes, &t)) return rc;
  if (mean_host || var_host) {
    // the planes are channel-major (the filter's reads are rows of one channel); the caller's
    // arrays are pixel-major: transposed on the host, in memory of the call's own, so that nothing
    // is written when the copy fails
    const size_t npix = (size_t)f.rows * f.wt;
    std::vector<double> h(2 * kYkFeatChannels * npix);
    YKF_HIP(hipMemcpyAsync(h.data(), planes, h.size() * sizeof(double), hipMemcpyDeviceToHost, f.stream));
    YKF_HIP(hipStreamSynchronize(f.stream));
    for (uint32_t c = 0; c < kYkFeatChannels; ++c) {
      const double* m = h.data() + (size_t)c * npix;
      const double* v = m + kYkFeatChannels * npix;
      for (size_t p = 0; p < npix; ++p) {
        if (mean_host) mean_host[p * kYkFeatChannels + c] = m[p];
        if (var_host) var_host[p * kYkFeatChannels + c] = v[p];
      }
    }
  }
  if (ms) *ms = t;
  return YK_OK;
}

}  // extern "C"
