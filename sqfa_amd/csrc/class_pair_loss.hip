// class_pair_loss.hip -- the first and the last step of every fused class-pair loss (sqfa_gauss_pairwise_loss,
// sqfa_log_euclidean_pairwise_loss, sqfa_jeffreys_pairwise_loss, sqfa_stein_pairwise_loss): the argument checks they share,
// and the per-class partials of the pass over the pairs becoming the loss and the two validity counters.
#include <hip/hip_runtime.h>
#include <stdio.h>

#include "../../include/sqfa_hip.h"
#include "class_pair_loss.hpp"

namespace sqfa {

// loss = sum of the per-class partial losses, {#NaN, #inf} = sums of the per-class counts: one workgroup, fixed order
template <typename T>
__global__ __launch_bounds__(256) void pair_loss_finalize_kernel(const double* loss_part, const int* cnt_part, int n,
                                                                  T* loss_out, int* nonfinite_out) {
  __shared__ double s_loss[256];
  __shared__ int s_cnt[256][2];
  const int tid = threadIdx.x;
  double l = 0.0;
  int nn = 0, ni = 0;
  for (int c = tid; c < n; c += 256) {
    l += loss_part[c];
    nn += cnt_part[2 * c];
    ni += cnt_part[2 * c + 1];
  }
  s_loss[tid] = l;
  s_cnt[tid][0] = nn;
  s_cnt[tid][1] = ni;
  __syncthreads();
  for (int d = 128; d > 0; d >>= 1) {
    if (tid < d) {
      s_loss[tid] += s_loss[tid + d];
      s_cnt[tid][0] += s_cnt[tid + d][0];
      s_cnt[tid][1] += s_cnt[tid + d][1];
    }
    __syncthreads();
  }
  if (tid == 0) {
    if (loss_out != nullptr) *loss_out = T(s_loss[0]);
    if (nonfinite_out != nullptr) {
      nonfinite_out[0] = s_cnt[0][0];
      nonfinite_out[1] = s_cnt[0][1];
    }
  }
}

hipError_t launch_pair_loss_finalize(const double* loss_part, const int* cnt_part, int n, int dtype, void* loss_out,
                                     int* nonfinite_out, hipStream_t stream) {
  dispatch_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL((pair_loss_finalize_kernel<T>), dim3(1), dim3(256), 0, stream, loss_part, cnt_part, n,
                       static_cast<T*>(loss_out), nonfinite_out);
  });
  return hipGetLastError();
}

int check_pair_loss_args(const char* entry, const char* inputs, bool inputs_null, int n, int m, int dtype, bool mode_ok,
                         const char* family_error, size_t need, const char* query, const void* workspace,
                         size_t workspace_bytes) {
  auto fail = [&](int rc, const char* what, const char* name = "", const char* rest = "") {
    if (entry != nullptr) {
      char text[256];
      snprintf(text, sizeof(text), "%s: %s%s%s", entry, what, name, rest);
      set_last_error(text);
    }
    return rc;
  };
  if (entry != nullptr) set_last_error("");
  if (inputs_null || n < 2 || m < 1) return fail(SQFA_ERR_BAD_ARGUMENT, "null ", inputs, ", n < 2 or m < 1");
  if (dtype != SQFA_F32 && dtype != SQFA_F64) return fail(SQFA_ERR_BAD_ARGUMENT, "dtype");
  if (!mode_ok) return fail(SQFA_ERR_BAD_ARGUMENT, "sqrt_mode outside {0, 1}");
  if (family_error != nullptr) return fail(SQFA_ERR_BAD_ARGUMENT, family_error);
  if (m > 64) return fail(SQFA_ERR_UNSUPPORTED_M, "m > 64");
  if (need == 0) return SQFA_ERR_UNSUPPORTED_M;   // the family's layout has nothing for these sizes: no text, as ever
  if (workspace == nullptr || workspace_bytes < need)
    return fail(SQFA_ERR_WORKSPACE, "workspace is null or smaller than ", query);
  return SQFA_OK;
}

}  // namespace sqfa
