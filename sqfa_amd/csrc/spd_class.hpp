// spd_class.hpp -- the per-class SPD factor stage: Cholesky in double and the inverse of the lower factor, of one (m,m)
// matrix, m <= 64, by ONE 64-thread workgroup (one wave).  The matrix lives in a 64 x SPD_LD array of doubles in LDS that
// the kernel declares (33 KB); thread r owns row r of the lower triangle.  Every function is called by the whole workgroup
// and holds its own barriers.  Users: spd_inverse_kernel (spd_class.hip; stage 1 of jeffreys_kernel.hip and stein_kernel.hip)
// and gauss_factor_kernel (gauss_scores_kernel.hip), gauss_nested_factor_kernel (gauss_nested_kernel.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

namespace sqfa {

constexpr int SPD_LD = 65;              // row pitch: column reads by the 64 rows hit distinct banks
constexpr int SPD_ELEMS = 64 * SPD_LD;  // __shared__ double a[SPD_ELEMS]

// the lower triangle of S (m,m) into a
template <typename T> __device__ __forceinline__ void spd_load_lower(double* a, const T* S, int m, int r) {
  constexpr int LD = SPD_LD;
  for (int idx = r; idx < m * m; idx += 64) {
    const int rr = idx / m, cc = idx % m;
    if (cc <= rr) a[rr * LD + cc] = (double)S[idx];
  }
  __syncthreads();
}

// Cholesky, right-looking: after step k column k holds L[:, k].  False, the same in every thread, at the first pivot that is
// not positive (FINITE: not positive and finite); a is then half factored.  logsum = sum_k log(pivot_k) = logdet S.
template <bool FINITE> __device__ __forceinline__ bool spd_cholesky(double* a, int m, int r, double& logsum) {
  constexpr int LD = SPD_LD;
  logsum = 0.0;
  for (int k = 0; k < m; ++k) {
    const double d = a[k * LD + k];   // the same value in every thread: the exit below is uniform
    if (!(d > 0.0 && (!FINITE || d < (double)INFINITY))) return false;
    logsum += log(d);
    const double root = sqrt(d), inv = 1.0 / root;
    __syncthreads();
    if (r == k) a[k * LD + k] = root;
    if (r > k && r < m) a[r * LD + k] *= inv;
    __syncthreads();
    if (r > k && r < m) {
      const double lrk = a[r * LD + k];
      for (int c = k + 1; c <= r; ++c) a[r * LD + c] -= lrk * a[c * LD + k];
    }
    __syncthreads();
  }
  return true;
}

// spd_cholesky with the running sums of the log-pivots kept: prefix[k] = sum_{i <= k} log(pivot_i) = logdet of the leading
// (k+1) x (k+1) block of S, accumulated in ascending order, so that prefix[m - 1] has the bits of spd_cholesky's logsum and
// a has the bits it leaves.  prefix: m doubles in LDS, written by thread 0, readable by all after a true return.
template <bool FINITE> __device__ __forceinline__ bool spd_cholesky_prefix(double* a, int m, int r, double* prefix) {
  constexpr int LD = SPD_LD;
  double logsum = 0.0;
  for (int k = 0; k < m; ++k) {
    const double d = a[k * LD + k];   // the same value in every thread: the exit below is uniform
    if (!(d > 0.0 && (!FINITE || d < (double)INFINITY))) return false;
    logsum += log(d);
    const double root = sqrt(d), inv = 1.0 / root;
    __syncthreads();
    if (r == 0) prefix[k] = logsum;
    if (r == k) a[k * LD + k] = root;
    if (r > k && r < m) a[r * LD + k] *= inv;
    __syncthreads();
    if (r > k && r < m) {
      const double lrk = a[r * LD + k];
      for (int c = k + 1; c <= r; ++c) a[r * LD + c] -= lrk * a[c * LD + k];
    }
    __syncthreads();
  }
  return true;
}

// X = L^-1 in place, last column first: X[r][j] L[j][j] = -sum_{k=j+1..r} X[r][k] L[k][j]
__device__ __forceinline__ void spd_invert_lower(double* a, int m, int r) {
  constexpr int LD = SPD_LD;
  for (int j = m - 1; j >= 0; --j) {
    const double xjj = 1.0 / a[j * LD + j];
    double sum = 0.0;
    if (r > j && r < m)
      for (int k = j + 1; k <= r; ++k) sum += a[r * LD + k] * a[k * LD + j];
    __syncthreads();
    if (r == j) a[j * LD + j] = xjj;
    if (r > j && r < m) a[r * LD + j] = -sum * xjj;
    __syncthreads();
  }
}

// spd_class.hip: P_c = S_c^-1 in the dtype, exactly symmetric, and, where ld is not null, ld_c = logdet S_c, for n matrices;
// a pivot that is not positive gives a NaN matrix and a NaN ld_c
hipError_t launch_spd_inverse(const void* S, int n, int m, int dtype, void* P, double* ld, hipStream_t stream);

}  // namespace sqfa
