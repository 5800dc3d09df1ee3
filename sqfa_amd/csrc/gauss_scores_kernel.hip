// gauss_scores_kernel.hip -- Gaussian class scores (quadratic discriminant analysis in feature space):
//     score[n][c] = -1/2 |L_c^-1 (z_n - mu_c)|^2 - sum_k log (L_c)_kk - K/2 log 2 pi + log pi_c  =  log p(z_n, c)
// for features z_n (K), class means mu_c, class covariances Sigma_c = L_c L_c^T and priors pi_c, with the argmax over the
// classes and the log evidence logsumexp_c score[n][c].  The whitened-difference form: the expanded quadratic
// z^T P z - 2 b^T z + const cancels in float32.
//
// Launches (caller's stream; nothing allocated, synchronised or read back; no float atomics, every sum in a fixed order:
// bitwise reproducible; every grid a function of (N, C, K) alone):
//   gauss_factor_kernel   once per classifier, one 64-thread workgroup per class, on the factor stage of spd_class.hpp:
//                         Cholesky in double in LDS, W_c = L_c^-1 in place, written lower triangular with exact zeros above
//                         the diagonal; offset_c = -sum log diag L_c - K/2 log 2 pi + log pi_c in double; a class with a
//                         pivot that is not positive and finite, a mean that is not finite or a log prior that is NaN or
//                         +inf gets NaN and is counted (integer atomic).
//   gauss_scores_kernel   workgroup (64 samples, split s of the classes) in the geometry of gauss_whiten.hpp, which has the
//                         stage of W_c, the product y = W_c (z - mu_c) and the order of its squares.  The 4 classes' partial
//                         sums of a group are reduced ACROSS the 4 lane quarters and transposed, so that lane (j, q) holds
//                         the full sum of class 4 g + q: one score, one compare and one exp per lane and group.  Every lane
//                         carries (max, index) and (max, sum exp) of its classes; the quarters are merged by a butterfly at
//                         the end (both partners compute the same bits: max and a + b commute).
//   gauss_merge_kernel    only where the classes are split (few sample tiles): merges the splits' partial (max, index),
//                         (max, sum exp) in the order s = 0, 1, ...
// A padded class scores -inf by select.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>

#include "../../include/sqfa_hip.h"
#include "class_pair_loss.hpp"   // namespace math, dispatch_dtype, WorkspaceCursor
#include "gauss_whiten.hpp"
#include "spd_class.hpp"

namespace sqfa {

// ---- the factor pass --------------------------------------------------------------------------------------------------------

template <typename T>
__global__ __launch_bounds__(64) void gauss_factor_kernel(const T* __restrict__ mu, const T* __restrict__ cov,
                                                          const double* __restrict__ log_prior, int C, int K,
                                                          T* __restrict__ W, double* __restrict__ offset,
                                                          int* __restrict__ bad_out) {
  constexpr int LD = SPD_LD;
  __shared__ double a[SPD_ELEMS];
  __shared__ int s_bad;
  const int r = threadIdx.x, kk = K * K, c = blockIdx.x;
  T* out = W + (size_t)c * kk;
  if (r == 0) s_bad = 0;
  spd_load_lower(a, cov + (size_t)c * kk, K, r);
  if (mu != nullptr && r < K) {
    const double v = (double)mu[(size_t)c * K + r];
    if (!(fabs(v) < (double)INFINITY)) s_bad = 1;   // every writer writes 1
  }
  __syncthreads();
  const double lp = log_prior != nullptr ? log_prior[c] : -log((double)C);
  bool bad = s_bad != 0 || !(lp < (double)INFINITY);   // NaN or +inf; -inf is a class that never wins
  double logdet = 0.0;   // sum_k log pivot_k = 2 sum_k log (L_c)_kk
  if (!bad) bad = !spd_cholesky<true>(a, K, r, logdet);
  if (bad) {
    for (int idx = r; idx < kk; idx += 64) out[idx] = math::nan<T>();
    if (r == 0) {
      offset[c] = math::nan<double>();
      atomicAdd(bad_out, 1);
    }
    return;
  }
  if (r == 0) offset[c] = -(0.5 * logdet) - 0.5 * K * 1.8378770664093454835606594728112 + lp;   // log 2 pi
  spd_invert_lower(a, K, r);
  for (int idx = r; idx < kk; idx += 64) {
    const int rr = idx / K, cc = idx % K;
    out[idx] = cc <= rr ? (T)a[rr * LD + cc] : (T)0;
  }
}

// ---- the scores ---------------------------------------------------------------------------------------------------------------

template <typename T> struct GsParams {
  const T* Z;
  long long N;
  const T* mu;
  const T* W;
  const double* offset;
  int C, K;
  T* scores;
  long long* argmax;
  T* best;
  T* lse;
  int* nonfinite;
  int groups_per_split, splits;   // groups of 4 classes
  // (splits, N) each, splits > 1 only; p_idx -1: the sample's row holds a NaN
  T* p_best;
  int* p_idx;
  T* p_m;
  T* p_sum;
};

// the running reductions of one sample over a set of classes
template <typename T> struct GsRun {
  T best;    // max score, -inf before the first
  int idx;   // its class, INT_MAX before the first
  T m, sum;  // logsumexp = m + log(sum); (-inf, 0) before the first finite score
  bool nan;
};

template <typename T> __device__ __forceinline__ void gs_take(GsRun<T>& a, T s, int c) {
  if (s != s) a.nan = true;
  if (s > a.best || (s == a.best && c < a.idx)) {
    a.best = s;
    a.idx = c;
  }
  const T d = s - a.m;
  const T e = math::exp(d > T(0) ? -d : d);   // exp(-|d|); d is NaN only for -inf - -inf, which neither branch below takes
  if (s > a.m) {
    a.sum = a.sum * e + T(1);
    a.m = s;
  } else if (s > math::neg_inf<T>()) {
    a.sum += e;
  }
}

// symmetric in its arguments bit for bit: both partners of a butterfly step compute the same values
template <typename T> __device__ __forceinline__ void gs_merge(GsRun<T>& a, T best, int idx, T m, T sum, bool nan) {
  if (best > a.best || (best == a.best && idx < a.idx)) {
    a.best = best;
    a.idx = idx;
  }
  const T mx = m > a.m ? m : a.m;
  if (mx > math::neg_inf<T>()) {
    const T lo = (m > a.m ? a.sum : sum) * math::exp((m > a.m ? a.m : m) - mx);   // the side with the smaller max, scaled
    const T hi = m > a.m ? sum : a.sum;
    a.sum = m == a.m ? a.sum + sum : hi + lo;
  }
  a.m = mx;
  a.nan = a.nan || nan;
}

template <typename T, int KB, bool MEANS>
__global__ __launch_bounds__(GW_THREADS) void gauss_scores_kernel(const GsParams<T> p) {
  using Stage = WhitenStage<T, KB>;
  constexpr int CS = Stage::CS, KP = Stage::KP, PITCH = Stage::PITCH;
  __shared__ T sW[Stage::W_ELEMS];
  __shared__ T sMu[Stage::MU_ELEMS];
  const int tid = threadIdx.x, l = tid & 63, wave = tid >> 6, q = l >> 4, j = l & 15;
  const int K = p.K, C = p.C, K4 = (K + 3) / 4;
  const long long N = p.N;
  const long long n = (long long)blockIdx.x * GW_ROWS + wave * 16 + j;
  const auto [g_lo, g_hi, c_end] = whiten_class_range(C, p.groups_per_split, blockIdx.y);

  T z[4 * KB];
  whiten_load_sample<T, KB>(z, p.Z, n, N, K, q);

  Stage stage(c_end, K, tid);
  stage.zero(sW);
  if (g_lo < g_hi) stage.template load<MEANS>(p.W, p.mu, 4 * g_lo);

  GsRun<T> run;
  run.best = math::neg_inf<T>();
  run.idx = INT_MAX;
  run.m = math::neg_inf<T>();
  run.sum = T(0);
  run.nan = false;

#pragma unroll 1
  for (int g = g_lo; g < g_hi; ++g) {
    const int c_mine = 4 * g + q;   // the class whose score this lane ends up with
    const T off = c_mine < C ? (T)p.offset[c_mine] : math::neg_inf<T>();
    if constexpr (CS == 4) {
      __syncthreads();   // the previous stage has been consumed (first pass: the zero fill is done)
      stage.template store<MEANS>(sW, sMu);
      __syncthreads();
      if (g + 1 < g_hi) stage.template load<MEANS>(p.W, p.mu, 4 * (g + 1));
    }
    T part[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      part[t] = T(0);
      if constexpr (CS == 1) {
        if (4 * g + t >= c_end) continue;   // uniform over the workgroup: a class past the end has no stage
        __syncthreads();
        stage.template store<MEANS>(sW, sMu);
        __syncthreads();
        if (4 * g + t + 1 < c_end) stage.template load<MEANS>(p.W, p.mu, 4 * g + t + 1);
      }
      T b[4 * KB];
      whiten_center<T, KB, MEANS>(b, z, sMu + (CS == 4 ? t : 0) * KP, K4, q);
      part[t] = whiten_sq_partial<T, KB>(sW + (CS == 4 ? t : 0) * KP * PITCH, b, K, K4, j, q);
    }
    const T tot = whiten_quarters_transpose(part, q);   // of class c_mine
    const T sc = c_mine < C ? T(-0.5) * tot + off : math::neg_inf<T>();
    if (c_mine < C) {
      if (p.scores != nullptr && n < N) p.scores[(size_t)n * C + c_mine] = sc;
      gs_take(run, sc, c_mine);
    }
  }

  // merge the quarters: a butterfly, the same bits in both partners
#pragma unroll
  for (int mask = 16; mask <= 32; mask *= 2) {
    const T ob = gw_shfl_xor(run.best, mask), om = gw_shfl_xor(run.m, mask), os = gw_shfl_xor(run.sum, mask);
    const int oi = __shfl_xor(run.idx, mask, 64), on = __shfl_xor(run.nan ? 1 : 0, mask, 64);
    gs_merge(run, ob, oi, om, os, on != 0);
  }
  const bool writer = q == 0 && n < N;
  if (p.splits > 1) {
    if (writer) {
      const size_t at = (size_t)blockIdx.y * N + n;
      p.p_best[at] = run.best;
      p.p_idx[at] = run.nan ? -1 : run.idx;
      p.p_m[at] = run.m;
      p.p_sum[at] = run.sum;
    }
    return;
  }
  if (writer) {
    if (p.argmax != nullptr) p.argmax[n] = run.nan ? -1 : run.idx;
    if (p.best != nullptr) p.best[n] = run.nan ? math::nan<T>() : run.best;
    if (p.lse != nullptr) p.lse[n] = run.nan ? math::nan<T>() : run.m + math::log(run.sum);
  }
  const unsigned long long bal = __ballot(writer && run.nan);
  if (l == 0 && bal != 0) atomicAdd(p.nonfinite, __popcll(bal));
}

// one thread per sample: the splits' partial reductions in the order s = 0, 1, ...
template <typename T>
__global__ __launch_bounds__(GW_THREADS) void gauss_merge_kernel(const GsParams<T> p) {
  const long long n = (long long)blockIdx.x * GW_THREADS + threadIdx.x;
  bool nan = false;
  if (n < p.N) {
    GsRun<T> run;
    run.best = p.p_best[n];
    run.idx = p.p_idx[n];
    run.m = p.p_m[n];
    run.sum = p.p_sum[n];
    run.nan = run.idx < 0;
    for (int s = 1; s < p.splits; ++s) {
      const size_t at = (size_t)s * p.N + n;
      const int idx = p.p_idx[at];
      gs_merge(run, p.p_best[at], idx < 0 ? INT_MAX : idx, p.p_m[at], p.p_sum[at], idx < 0);
    }
    nan = run.nan;
    if (p.argmax != nullptr) p.argmax[n] = nan ? -1 : run.idx;
    if (p.best != nullptr) p.best[n] = nan ? math::nan<T>() : run.best;
    if (p.lse != nullptr) p.lse[n] = nan ? math::nan<T>() : run.m + math::log(run.sum);
  }
  const unsigned long long bal = __ballot(nan);
  if ((threadIdx.x & 63) == 0 && bal != 0) atomicAdd(p.nonfinite, __popcll(bal));
}

// ---- host ---------------------------------------------------------------------------------------------------------------------

struct GsLayout {
  int groups_per_split, splits;
  size_t off_best, off_m, off_sum, off_idx, total;   // splits > 1: four (splits, N) arrays [best T][m T][sum T][idx int]
};

static bool gs_layout(long long N, int C, int K, int dtype, GsLayout* w) {
  if (!whiten_class_split(N, C, K, dtype, &w->groups_per_split, &w->splits)) return false;
  const size_t cells = w->splits > 1 ? (size_t)w->splits * (size_t)N : 0;
  WorkspaceCursor ws{1};   // the four arrays back to back
  w->off_best = ws.take(cells * dtype_bytes(dtype));
  w->off_m = ws.take(cells * dtype_bytes(dtype));
  w->off_sum = ws.take(cells * dtype_bytes(dtype));
  w->off_idx = ws.take(cells * sizeof(int));
  w->total = ws.at;
  return true;
}

template <typename T>
static hipError_t run_scores(const void* Z, long long N, const void* mu, const void* W, const double* offset, int C, int K,
                             void* scores, long long* argmax, void* best, void* lse, int* nonfinite, char* ws,
                             const GsLayout& lay, hipStream_t stream) {
  GsParams<T> p{};
  p.Z = static_cast<const T*>(Z);
  p.N = N;
  p.mu = static_cast<const T*>(mu);
  p.W = static_cast<const T*>(W);
  p.offset = offset;
  p.C = C;
  p.K = K;
  p.scores = static_cast<T*>(scores);
  p.argmax = argmax;
  p.best = static_cast<T*>(best);
  p.lse = static_cast<T*>(lse);
  p.nonfinite = nonfinite;
  p.groups_per_split = lay.groups_per_split;
  p.splits = lay.splits;
  if (lay.splits > 1) {
    p.p_best = reinterpret_cast<T*>(ws + lay.off_best);
    p.p_m = reinterpret_cast<T*>(ws + lay.off_m);
    p.p_sum = reinterpret_cast<T*>(ws + lay.off_sum);
    p.p_idx = reinterpret_cast<int*>(ws + lay.off_idx);
  }
  hipError_t e = hipMemsetAsync(nonfinite, 0, sizeof(int), stream);
  if (e != hipSuccess) return e;
  const dim3 grid((unsigned)((N + GW_ROWS - 1) / GW_ROWS), (unsigned)lay.splits);
  dispatch_kb(K, mu != nullptr, [&](auto kb, auto means) {
    hipLaunchKernelGGL((gauss_scores_kernel<T, decltype(kb)::value, decltype(means)::value>), grid, dim3(GW_THREADS), 0,
                       stream, p);
  });
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (lay.splits > 1) {
    hipLaunchKernelGGL((gauss_merge_kernel<T>), dim3((unsigned)((N + GW_THREADS - 1) / GW_THREADS)), dim3(GW_THREADS), 0,
                       stream, p);
    e = hipGetLastError();
  }
  return e;
}

}  // namespace sqfa

using namespace sqfa;

extern "C" size_t sqfa_gauss_scores_workspace_bytes(long long N, int C, int K, int dtype) {
  GsLayout w;
  if (!gs_layout(N, C, K, dtype, &w)) return 0;
  return w.total < 16 ? 16 : w.total;
}

extern "C" int sqfa_gauss_class_factors(const void* means, const void* cov, const double* log_priors, int C, int K, int dtype,
                                        void* W_out, double* offset_out, int* bad_out, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const bool nulls = cov == nullptr || W_out == nullptr || offset_out == nullptr || bad_out == nullptr || C < 1 || K < 1;
  const int rc = check_gauss_args("sqfa_gauss_class_factors", nulls, "null covariances or outputs, C < 1 or K < 1", dtype,
                                  nullptr, K, false, 0, nullptr, 0);
  if (rc != SQFA_OK) return rc;
  if (hipMemsetAsync(bad_out, 0, sizeof(int), stream) != hipSuccess) return SQFA_ERR_LAUNCH;
  dispatch_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL((gauss_factor_kernel<T>), dim3(C), dim3(64), 0, stream, static_cast<const T*>(means),
                       static_cast<const T*>(cov), log_priors, C, K, static_cast<T*>(W_out), offset_out, bad_out);
  });
  return hipGetLastError() == hipSuccess ? SQFA_OK : SQFA_ERR_LAUNCH;
}

extern "C" int sqfa_gauss_scores(const void* Z, long long N, const void* means, const void* W, const double* offset, int C,
                                 int K, int dtype, void* scores_out, long long* argmax_out, void* best_out,
                                 void* logsumexp_out, int* nonfinite_out, void* workspace, size_t workspace_bytes,
                                 void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  GsLayout lay;
  const size_t need = gs_layout(N, C, K, dtype, &lay) ? (lay.total < 16 ? 16 : lay.total) : 0;
  const bool nulls = Z == nullptr || W == nullptr || offset == nullptr || nonfinite_out == nullptr || N < 1 || C < 1 || K < 1;
  const int rc = check_gauss_args("sqfa_gauss_scores", nulls, "null samples, factors, offsets or counter, N < 1, C < 1 or K < 1",
                                  dtype, best_out != nullptr && argmax_out == nullptr ? "best_out without argmax_out" : nullptr,
                                  K, true, need, workspace, workspace_bytes);
  if (rc != SQFA_OK) return rc;
  const hipError_t e = dispatch_dtype(dtype, [&](auto t) {
    return run_scores<decltype(t)>(Z, N, means, W, offset, C, K, scores_out, argmax_out, best_out, logsumexp_out, nonfinite_out,
                                   static_cast<char*>(workspace), lay, stream);
  });
  return e == hipSuccess ? SQFA_OK : SQFA_ERR_LAUNCH;
}
