// yk_film_internal.hpp — what the film's two translation units share: the exactly rounded
// arithmetic of the film kernels, and the view of a film (ykgpu_render.hip owns ykgpu_film) that
// the denoise unit (yk_denoise.hip) works through.  Not part of the C-ABI.
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
};

// null or torn film: YK_ERR_INVALID with the last error set, like every film call
int yk_film_view_of(ykgpu_film* film, yk_film_view* out);
// sets ykgpu_last_error's message for the calling thread and returns code
int yk_film_fail(int code, const char* msg);

#endif
