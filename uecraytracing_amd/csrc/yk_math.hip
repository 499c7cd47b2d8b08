// yk_math.hip — the diagnostic math entry points (include/ykgpu.h ykgpu_math_*): the device's
// math::sqrt and vector / scalar division, FP64 and FP32, run on a caller's buffer so that the host
// tests compare them with the reference's arithmetic.  Built with the default flags:
// yk_math_sqrt_f32 is not compiled under the FP32 path kernel's max-ilp scheduler.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/ykgpu.h"
#include "yk_host_internal.hpp"

using namespace ykhost;

namespace {

// ykgpu_math_div: the renderer's vector / scalar division (divs_fast) on a buffer (diagnostic).
__global__ __launch_bounds__(256) void yk_math_div(const double* num3, const double* den, double* out3,
                                                  uint64_t n) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const ykd::v3 q = ykd::divs_fast({num3[3 * i], num3[3 * i + 1], num3[3 * i + 2]}, den[i]);
  out3[3 * i] = q.x;
  out3[3 * i + 1] = q.y;
  out3[3 * i + 2] = q.z;
}

// ykgpu_math_div_f32: the FP32 kernel's vector / scalar division (ykf::divs_fast) on a buffer.
__global__ __launch_bounds__(256) void yk_math_div_f32(const float* num3, const float* den, float* out3, uint64_t n) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const ykf::v3 q = ykf::divs_fast({num3[3 * i], num3[3 * i + 1], num3[3 * i + 2]}, den[i]);
  out3[3 * i] = q.x;
  out3[3 * i + 1] = q.y;
  out3[3 * i + 2] = q.z;
}

// ykgpu_math_sqrt: the device's math::sqrt on a buffer (diagnostic entry point).
__global__ __launch_bounds__(256) void yk_math_sqrt(const double* in, double* out, uint64_t n) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = ykd::nsqrt(in[i]);
}

// ykgpu_math_sqrt_f32: the FP32 path's math::sqrt<float> on a buffer (diagnostic).
__global__ __launch_bounds__(256) void yk_math_sqrt_f32(const float* in, float* out, uint64_t n) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t it = 0;
  if (i < n) out[i] = ykf::nsqrt(in[i], it);
}

// One call: the inputs (kA planes of n elements at a, kB at b; kB == 0: no second input) into one
// device buffer, one after the other and followed by the kOut output planes, the kernel over n
// elements on the context's stream, the output copied back.
template <typename T, auto kKernel, uint32_t kA, uint32_t kB, uint32_t kOut>
int math_call(ykgpu_context* ctx, const char* name, const T* a, const T* b, T* out, uint64_t n) {
  if (!ctx || (n && (!a || (kB && !b) || !out))) return fail(YK_ERR_INVALID, "null argument");
  if (n == 0) return YK_OK;
  YK_HIP(hipSetDevice(ctx->device));
  T* d = nullptr;
  YK_HIP(hipMalloc(&d, (kA + kB + kOut) * n * sizeof(T)));
  T* const d_out = d + (kA + kB) * n;
  hipError_t e = hipMemcpy(d, a, kA * n * sizeof(T), hipMemcpyHostToDevice);
  if (kB && e == hipSuccess) e = hipMemcpy(d + kA * n, b, kB * n * sizeof(T), hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    const uint64_t blocks = (n + 255) / 256;
    if constexpr (kB != 0)
      hipLaunchKernelGGL(kKernel, dim3((uint32_t)blocks), dim3(256), 0, ctx->stream, d, d + kA * n, d_out, n);
    else
      hipLaunchKernelGGL(kKernel, dim3((uint32_t)blocks), dim3(256), 0, ctx->stream, d, d_out, n);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e == hipSuccess) e = hipMemcpy(out, d_out, kOut * n * sizeof(T), hipMemcpyDeviceToHost);
  (void)hipFree(d);
  if (e != hipSuccess) return fail(YK_ERR_DEVICE, std::string(name) + ": " + hipGetErrorString(e));
  return YK_OK;
}

}  // namespace

extern "C" {

int ykgpu_math_sqrt(ykgpu_context* ctx, const double* in, double* out, uint64_t n) {
  return math_call<double, yk_math_sqrt, 1, 0, 1>(ctx, "ykgpu_math_sqrt", in, nullptr, out, n);
}

int ykgpu_math_sqrt_f32(ykgpu_context* ctx, const float* in, float* out, uint64_t n) {
  return math_call<float, yk_math_sqrt_f32, 1, 0, 1>(ctx, "ykgpu_math_sqrt_f32", in, nullptr, out, n);
}

int ykgpu_math_div(ykgpu_context* ctx, const double* num3, const double* den, double* out3, uint64_t n) {
  return math_call<double, yk_math_div, 3, 1, 3>(ctx, "ykgpu_math_div", num3, den, out3, n);
}

int ykgpu_math_div_f32(ykgpu_context* ctx, const float* num3, const float* den, float* out3, uint64_t n) {
  return math_call<float, yk_math_div_f32, 3, 1, 3>(ctx, "ykgpu_math_div_f32", num3, den, out3, n);
}

}  // extern "C"
