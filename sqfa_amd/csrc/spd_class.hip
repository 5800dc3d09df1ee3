// spd_class.hip -- stage 1 of the Jeffreys and Stein losses: the inverse, and the log-determinant, of every class matrix
// (spd_class.hpp has the factorisation).
#include <hip/hip_runtime.h>

#include "class_pair_loss.hpp"
#include "spd_class.hpp"

namespace sqfa {

// One 64-thread workgroup (one wave) per class.
template <typename T>
__global__ __launch_bounds__(64) void spd_inverse_kernel(const T* __restrict__ Sin, T* __restrict__ P, double* __restrict__ ld,
                                                          int m) {
  constexpr int LD = SPD_LD;
  __shared__ double a[SPD_ELEMS];
  const int r = threadIdx.x, mm = m * m;
  T* out = P + (size_t)blockIdx.x * mm;
  spd_load_lower(a, Sin + (size_t)blockIdx.x * mm, m, r);
  double logdet;
  if (!spd_cholesky<false>(a, m, r, logdet)) {
    for (int idx = r; idx < mm; idx += 64) out[idx] = math::nan<T>();
    if (ld != nullptr && r == 0) ld[blockIdx.x] = math::nan<double>();
    return;
  }
  if (ld != nullptr && r == 0) ld[blockIdx.x] = logdet;
  spd_invert_lower(a, m, r);
  // P = X^T X: thread r computes P[r][b], b <= r, and writes both mirror entries
  if (r < m) {
    for (int b = 0; b <= r; ++b) {
      double acc = 0.0;
      for (int k = r; k < m; ++k) acc += a[k * LD + r] * a[k * LD + b];
      const T v = (T)acc;
      out[r * m + b] = v;
      out[b * m + r] = v;
    }
  }
}

hipError_t launch_spd_inverse(const void* S, int n, int m, int dtype, void* P, double* ld, hipStream_t stream) {
  dispatch_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL((spd_inverse_kernel<T>), dim3(n), dim3(64), 0, stream, static_cast<const T*>(S), static_cast<T*>(P), ld,
                       m);
  });
  return hipGetLastError();
}

}  // namespace sqfa
