// class_pair_loss.hpp -- what the fused class-pair losses (gauss_pair_kernel.hip, log_euclidean_kernel.hip, jeffreys_kernel.hip,
// stein_kernel.hip) and the Gaussian class scores (gauss_scores_kernel.hip) share.
// Device side: the scalar overloads of namespace math, and PairLossParams -- per-class pre-stages, ONE pass over the ordered
// class pairs that writes per-class partial losses and {#NaN, #inf} counts under a uniform weight or a symmetric (n,n) weight
// matrix, and a one-workgroup reduction (class_pair_loss.hip).  A family's parameter struct derives from PairLossParams and
// adds its own pointers; its kernels read the weight and eps of their element type through pair_weight<T> / pair_eps<T>.
// (GaussParams declares the same ten fields itself, in the order its kernels were tuned with -- see gauss_pair_kernel.hip --
// so the accessors and the fill helper take any struct that has them.)
// Host side, the frame of an entry point: the workspace cursor, the argument checks the four pairwise entry points share,
// the dispatch on the dtype, and set_last_error.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include <cmath>

#include "../../include/sqfa_hip.h"

namespace sqfa {

// the scalar functions of both element types under one name each (pair_kernel.hpp keeps a Newton-step rsqrt of its own:
// different arithmetic)
namespace math {
__device__ __forceinline__ float sqrt(float x) { return sqrtf(x); }
__device__ __forceinline__ double sqrt(double x) { return ::sqrt(x); }
__device__ __forceinline__ float rsqrt(float x) { return 1.0f / sqrtf(x); }
__device__ __forceinline__ double rsqrt(double x) { return 1.0 / ::sqrt(x); }
__device__ __forceinline__ float log(float x) { return logf(x); }
__device__ __forceinline__ double log(double x) { return ::log(x); }
__device__ __forceinline__ float exp(float x) { return expf(x); }
__device__ __forceinline__ double exp(double x) { return ::exp(x); }
template <typename T> __device__ __forceinline__ T nan();
template <> __device__ __forceinline__ float nan<float>() { return __builtin_nanf(""); }
template <> __device__ __forceinline__ double nan<double>() { return __builtin_nan(""); }
template <typename T> __device__ __forceinline__ T neg_inf() { return -(T)INFINITY; }
}  // namespace math

struct PairLossParams {
  void* dist;           // (n,n) or nullptr
  double* loss_part;    // (n) per-class partial losses sum_{j<i} w_ij D_ij
  int* cnt_part;        // (n,2) per-class {#NaN, #inf} among j < i
  int n, m;
  double eps, weight;
  float epsf, weightf;  // the same two, rounded once on the host (scalar kernel arguments, no conversion per wave)
  const void* W;        // (n,n) symmetric per-pair weights (weighted kernels only; `weight` is then unused)
};

template <typename T, typename P> __device__ __forceinline__ T pair_weight(const P& p) {
  if constexpr (sizeof(T) == sizeof(float)) return p.weightf;
  else return p.weight;
}
template <typename T, typename P> __device__ __forceinline__ T pair_eps(const P& p) {
  if constexpr (sizeof(T) == sizeof(float)) return p.epsf;
  else return p.eps;
}

template <typename P>
inline void fill_pair_loss_params(P& p, int n, int m, double eps, const void* pair_weights, double uniform_weight,
                                  void* dist, double* loss_part, int* cnt_part) {
  p.dist = dist;
  p.loss_part = loss_part;
  p.cnt_part = cnt_part;
  p.n = n;
  p.m = m;
  p.eps = eps;
  p.weight = uniform_weight;
  p.epsf = (float)eps;
  p.weightf = (float)uniform_weight;
  p.W = pair_weights;
}

// workspace sections start on 256-byte boundaries
inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

// Carves a workspace: take(bytes) returns the offset of the next section and moves on to the next multiple of `align`
// (a power of two); `at` is then the total.
struct WorkspaceCursor {
  size_t align = 256, at = 0;
  size_t take(size_t bytes) {
    const size_t offset = at;
    at = (at + bytes + align - 1) & ~(align - 1);
    return offset;
  }
};

inline size_t dtype_bytes(int dtype) { return dtype == SQFA_F32 ? 4 : 8; }

// f(T{}) with T the element type of `dtype`:  dispatch_dtype(dtype, [&](auto t) { using T = decltype(t); ... });
template <typename F> inline auto dispatch_dtype(int dtype, F&& f) {
  if (dtype == SQFA_F32) return f(float{});
  return f(double{});
}

// sqfa_api.hip: the text sqfa_hip_last_error() returns
void set_last_error(const char* text);

// class_pair_loss.hip: the argument checks of the pairwise entry points, in their order: null inputs / n < 2 / m < 1, dtype,
// mode (sqrt_mode, or the Gaussian kind), the family's own check (`family_error`: nullptr where it passes, else the text),
// m > 64, workspace (`need` bytes: the family's layout, 0 where it has none for these sizes).  SQFA_OK or the code to return.
// `entry` names the entry point in the text for sqfa_hip_last_error(), which is cleared first; an entry point that sets no
// text passes nullptr, and the text is then left alone.  `inputs` is what the text calls the input pointers, `query` the
// family's workspace query.
int check_pair_loss_args(const char* entry, const char* inputs, bool inputs_null, int n, int m, int dtype, bool mode_ok,
                         const char* family_error, size_t need, const char* query, const void* workspace,
                         size_t workspace_bytes);

// class_pair_loss.hip: loss = sum of the per-class partial losses, {#NaN, #inf} = sums of the per-class counts
hipError_t launch_pair_loss_finalize(const double* loss_part, const int* cnt_part, int n, int dtype, void* loss_out,
                                     int* nonfinite_out, hipStream_t stream);

}  // namespace sqfa
