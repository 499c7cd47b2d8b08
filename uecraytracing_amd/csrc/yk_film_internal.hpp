// yk_film_internal.hpp — what the film's device code shares (yk_pipeline.hip's folds, yk_film.hip,
// yk_denoise.hip, yk_features.hip): the exactly rounded arithmetic of the film kernels and the layout
// of the feature planes.  Not part of the C-ABI.
#ifndef YK_FILM_INTERNAL_HPP
#define YK_FILM_INTERNAL_HPP

#include <hip/hip_runtime.h>

#include <cstdint>

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

// planes of a film's feature buffer, each rows * wt doubles in pixel order: the means F0..F6, the
// variances of the means U0..U6, and the group sums V_A = (U0 + U1) + U2, V_N = (U3 + U4) + U5, V_Z = U6
constexpr uint32_t kYkFeatChannels = 7, kYkFeatPlanes = 17;

#endif
