// yk_features.hip — ykgpu_film_features (include/ykgpu.h "film features"): the
// first-hit albedo, normal and depth of every pixel of a film's tile, defined operation by operation
// in IEEE double so that numpy restates it bit for bit (tests/film_features_ref.py).
//
// A unit of its own, like yk_denoise.hip (it also holds the ray queries, yk_cast.hpp, and the
// radiance queries, yk_radiance.hpp, and the gather queries, yk_gather.hpp, included at the end).  One kernel, yk_film_features, on the context's stream;
// its result lives in planes the film owns (ykgpu_film, yk_host_internal.hpp) and is computed once
// per (film, grid).  The sampled pass (yk_features_sampled.hpp) fills the same planes another way.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/ykgpu.h"
#include "yk_device.hpp"
#include "yk_film_internal.hpp"
#include "yk_host_internal.hpp"

using namespace ykhost;

namespace {

constexpr uint32_t kMaxGrid = 4;
// The block of pixels of one workgroup, yk_film_nlm's: a wave is two rows of 32 pixels.
constexpr uint32_t kBlockW = 32, kBlockH = 8, kThreads = kBlockW * kBlockH;
// Spheres staged in LDS at a time: 4 doubles each, 16 KiB a workgroup (ten workgroups fit a CU's
// 160 KiB, more than its waves allow), and the final scene's 485 spheres are one chunk.
constexpr uint32_t kChunk = 512;

// the device tables as the kernel reads them: the geometry as 4 doubles per sphere (cx, cy, cz,
// radius*radius), the materials as kYkMatStride bytes per sphere with the albedo, the radius and the
// kind at these offsets
constexpr size_t kYkMatStride = 64, kYkMatAlbedo = 0, kYkMatRadius = 32, kYkMatKind = 48;
static_assert(sizeof(SphereGeo) == 4 * sizeof(double) && offsetof(SphereGeo, rr) == 3 * sizeof(double), "FeatArgs::geo");
static_assert(sizeof(SphereMat) == kYkMatStride && offsetof(SphereMat, ar) == kYkMatAlbedo &&
                  offsetof(SphereMat, ab) == kYkMatAlbedo + 16 && offsetof(SphereMat, radius) == kYkMatRadius &&
                  offsetof(SphereMat, kind) == kYkMatKind, "FeatArgs::mat");

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

int ykhost::yk_film_features_ensure(ykgpu_film* film, uint32_t grid, const double** planes, double* ms) {
  if (grid < 1 || grid > kMaxGrid) return fail(YK_ERR_INVALID, "features: grid must be 1..4");
  const ykgpu_context* ctx = film->ctx;
  if (film->scene_gen != ctx->scene_gen)
    return fail(YK_ERR_INVALID, "the context's scene was set after the film was created");
  YK_HIP(hipSetDevice(film->device));
  const yk_render_params& p = film->p;
  const uint32_t rows = p.row_count, wt = tile_width(&p);
  const hipStream_t stream = ctx->stream;  // (film calls are synchronous on it)
  const size_t npix = (size_t)rows * wt;
  if (!film->d_features) {  // (a film's tile never changes size)
    film->feature_grid = film->feature_n = 0;
    YK_HIP(hipMalloc(&film->d_features, kYkFeatPlanes * npix * sizeof(double)));
  }
  *planes = (const double*)film->d_features;
  if (ms) *ms = 0.0;
  if (film->feature_grid == grid) return YK_OK;
  film->feature_grid = film->feature_n = 0;  // (until the pass is whole; a sampled pass's planes are replaced)
  const TileCols cols = film_cols(film);
  FeatArgs a{};
  a.cam = ctx->cam;
  a.geo = (const double*)ctx->d_geo;
  a.mat = (const unsigned char*)ctx->d_mat;
  a.out = (double*)film->d_features;
  a.t_min = p.t_min;
  a.nspheres = ctx->nspheres;
  a.grid = grid;
  a.W = p.image_width;
  a.H = p.image_height;
  a.rows = rows;
  a.wt = wt;
  a.npix = (uint32_t)npix;
  a.row_begin = p.row_begin;
  a.row_stride = p.row_stride;
  a.row_band = p.row_band_log2;
  a.col_begin = cols.begin;
  a.col_stride = cols.stride;
  a.col_band = cols.band;
  hipEvent_t ev[2] = {nullptr, nullptr};
  hipError_t e = hipEventCreate(&ev[0]);
  if (e == hipSuccess) e = hipEventCreate(&ev[1]);
  if (e == hipSuccess) e = hipEventRecord(ev[0], stream);
  if (e == hipSuccess) {
    const dim3 blocks((wt + kBlockW - 1) / kBlockW, (rows + kBlockH - 1) / kBlockH);
    hipLaunchKernelGGL(yk_film_features, blocks, dim3(kThreads), 0, stream, a);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipEventRecord(ev[1], stream);
  if (e == hipSuccess) e = hipStreamSynchronize(stream);
  float t = 0;
  if (e == hipSuccess) e = hipEventElapsedTime(&t, ev[0], ev[1]);
  for (hipEvent_t v : ev)
    if (v) (void)hipEventDestroy(v);
  if (e != hipSuccess)
    return fail(e == hipErrorOutOfMemory ? YK_ERR_NOMEM : YK_ERR_DEVICE,
                std::string("ykgpu_film_features: ") + hipGetErrorString(e));
  film->feature_grid = grid;
  if (ms) *ms = t;
  return YK_OK;
}

int ykhost::yk_film_features_copy_out(ykgpu_film* film, const double* planes, double* mean_host, double* var_host) {
  if (!mean_host && !var_host) return YK_OK;
  // the planes are channel-major (the filter's reads are rows of one channel); the caller's
  // arrays are pixel-major: transposed on the host, in memory of the call's own, so that nothing
  // is written when the copy fails
  const size_t npix = (size_t)film->p.row_count * tile_width(&film->p);
  std::vector<double> h(2 * kYkFeatChannels * npix);
  YK_HIP(hipMemcpyAsync(h.data(), planes, h.size() * sizeof(double), hipMemcpyDeviceToHost, film->ctx->stream));
  YK_HIP(hipStreamSynchronize(film->ctx->stream));
  for (uint32_t c = 0; c < kYkFeatChannels; ++c) {
    const double* m = h.data() + (size_t)c * npix;
    const double* v = m + kYkFeatChannels * npix;
    for (size_t p = 0; p < npix; ++p) {
      if (mean_host) mean_host[p * kYkFeatChannels + c] = m[p];
      if (var_host) var_host[p * kYkFeatChannels + c] = v[p];
    }
  }
  return YK_OK;
}

extern "C" {

int ykgpu_film_features(ykgpu_film* film, uint32_t grid, double* mean_host, double* var_host, double* ms) {
  if (int rc = film_ready(film)) return rc;
  const double* planes = nullptr;
  double t = 0;
  if (int rc = yk_film_features_ensure(film, grid, &planes, &t)) return rc;
  if (int rc = yk_film_features_copy_out(film, planes, mean_host, var_host)) return rc;
  if (ms) *ms = t;
  return YK_OK;
}

}  // extern "C"

// The query kernels' checked stack capacity (ykquery::query_stack_cap, yk_query.hpp: the cast, the
// radiance and gather queries, the sampled feature pass).  0: the tree's own.  A test build forces a
// shallow one (Makefile libykgpu_qstack%.so), so that lanes overflow it and take the ordered scan
// (tests/test_gpu_fallbacks.py).
#ifdef YK_QUERY_STACK_FORCE
constexpr uint32_t kYkQueryStackForce = YK_QUERY_STACK_FORCE;
static_assert(kYkQueryStackForce >= 1 && kYkQueryStackForce <= 48, "the forced query stack: 1..kStackMax entries");
#else
constexpr uint32_t kYkQueryStackForce = 0;
#endif

// what the query kernels below share: the closest hit of the context's FP64 tree
#include "yk_query.hpp"
// the ray queries (ykgpu_cast_rays ...): the unit's other first-hit query, in a file of its own
#include "yk_cast.hpp"
// ... and the radiance queries (ykgpu_radiance_rays ...), whose closest hit is the same
#include "yk_radiance.hpp"
// ... and the gather queries (ykgpu_gather_points ...), whose rays are radiance queries' rays
#include "yk_gather.hpp"
// ... and the sampled feature pass (ykgpu_film_features_sampled ...), whose closest hit is the same
#include "yk_features_sampled.hpp"
