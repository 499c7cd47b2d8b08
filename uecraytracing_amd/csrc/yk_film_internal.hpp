// yk_film_internal.hpp — what the film's two translation units share: the exactly rounded
// arithmetic of the film kernels, and the view of a film (ykgpu_render.hip owns ykgpu_film) that
// the denoise unit (yk_denoise.hip) and the feature unit (yk_features.hip) work through.  Not part
// of the C-ABI.
#ifndef YK_FILM_INTERNAL_HPP
#define YK_FILM_INTERNAL_HPP

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/ykgpu.h"

// The arithmetic the host tests restate in numpy: each operation rounded on its own, never fused.
// (the units are built with -ffp-contract=off; the pragma says so for these four whatever the flags)
__device__ __forceinline__ double film_add(double a, double b) {
#pragma clang fp contract(off)
  return __dadd_rn(a, b);
}
__device__ __forceinline__ double film_sub(double a, double b) {
#pragma clang fp contract(off)
  return __dsub_rn(a, b);
}
__device__ __forceinline__ double film_mul(double a, double b) {
#pragma clang fp contract(off)
  return __dmul_rn(a, b);
}
__device__ __forceinline__ double film_div(double a, double b) {
#pragma clang fp contract(off)
  return __ddiv_rn(a, b);
}

// A film as ykgpu_film_denoise sees it.  The planes are read only; `scratch` is the film's own
// slot for the denoise buffers (null until the first denoise, hipFree'd by ykgpu_film_destroy).
struct yk_film_view {
  int device;
  hipStream_t stream;     // the context's: film calls are synchronous on it
  const double* plane;    // 6 * nps, slot order (s: planes 0..2, q: 3..5)
  const uint32_t* order;  // slot → pixel of the tile (row * Wt + column), 0xffffffff: no pixel
  const uint32_t* count;  // per slot, null while the film is uniform (every count == done)
  uint32_t nps, done, rows, wt;
  bool consecutive;  // the tile is image rows y0.. and image columns x0.. without gaps
  void** scratch;
  // what the feature pass (yk_features.hip) needs: the image, the tile's row and column sets (tile
  // row t is image row row_begin + (((t >> row_band) * row_stride) << row_band) + (t & (2^row_band - 1)),
  // columns alike; the whole width is 0, 1, 0), and the scene the film was created with
  uint32_t W, H;
  uint32_t row_begin, row_stride, row_band, col_begin, col_stride, col_band;
  double t_min;
  bool stale;               // the context's scene was set after the film was created
  const double* geo;        // per sphere, tuple order: cx, cy, cz, radius*radius
  const unsigned char* mat; // per sphere kYkMatStride bytes: the albedo, the radius and the kind at the offsets below
  uint32_t nspheres;
  yk_camera cam;
  void** features;      // the film's slot for the feature planes (null until the first pass, freed with the film)
  uint32_t* feature_grid;  // the grid the planes hold (0: none yet)
};
// the device material table as the feature pass reads it (ykgpu_render.hip asserts the offsets)
constexpr size_t kYkMatStride = 64, kYkMatAlbedo = 0, kYkMatRadius = 32, kYkMatKind = 48;
// planes of a film's feature buffer, each rows * wt doubles in pixel order: the means F0..F6, the
// variances of the means U0..U6, and the group sums V_A = (U0 + U1) + U2, V_N = (U3 + U4) + U5, V_Z = U6
constexpr uint32_t kYkFeatChannels = 7, kYkFeatPlanes = 17;

// The feature planes of the film at grid g (1..4) on the device, computed on the view's stream
// unless the film already holds them; *ms (may be null) receives the pass's device time, 0 when the
// cached planes were reused.  Synchronous.  YK_ERR_INVALID on a stale scene or a grid out of range.
int yk_film_features_ensure(const yk_film_view& f, uint32_t grid, const double** planes, double* ms);

// null or torn film: YK_ERR_INVALID with the last error set, like every film call
int yk_film_view_of(ykgpu_film* film, yk_film_view* out);
// sets ykgpu_last_error's message for the calling thread and returns code
int yk_film_fail(int code, const char* msg);

#endif
