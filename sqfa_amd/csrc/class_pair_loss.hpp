// class_pair_loss.hpp -- what the fused class-pair losses share on the host side (gauss_pair_kernel.hip,
// log_euclidean_kernel.hip, jeffreys_kernel.hip): per-class pre-stages, ONE pass over the ordered class pairs that writes
// per-class partial losses and {#NaN, #inf} counts under a uniform weight or a symmetric (n,n) weight matrix, and a
// one-workgroup reduction (class_pair_loss.hip).  A family's parameter struct derives from PairLossParams and adds its own
// pointers; its kernels read the weight and eps of their element type through pair_weight<T> / pair_eps<T>.  (GaussParams
// declares the same ten fields itself, in the order its kernels were tuned with -- see gauss_pair_kernel.hip -- so the
// accessors and the fill helper take any struct that has them.)
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace sqfa {

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

// class_pair_loss.hip: loss = sum of the per-class partial losses, {#NaN, #inf} = sums of the per-class counts
hipError_t launch_pair_loss_finalize(const double* loss_part, const int* cnt_part, int n, int dtype, void* loss_out,
                                     int* nonfinite_out, hipStream_t stream);

}  // namespace sqfa
