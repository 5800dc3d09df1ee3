// gauss_nested_kernel.hip -- nested Gaussian class scores: the K classifiers that see the first k = 1 .. K features, in one pass.
// With Sigma_c = L_c L_c^T and y = L_c^-1 (z - mu_c): L_c is lower triangular, its leading k x k block is the Cholesky factor
// of the leading block of Sigma_c, and y_0 .. y_{k-1} depend on the first k features only.  So
//     score_k[n][c] = -1/2 sum_{i<k} y_i^2 + offset_k[c],    offset_k[c] = -sum_{i<k} log (L_c)_ii - k/2 log 2 pi + log pi_c
// is a prefix sum over the rows of the y that gauss_scores_kernel.hip forms anyway (DESIGN Q3).
//
// Launches (caller's stream; nothing allocated, synchronised or read back; no float atomics, every sum in a fixed order:
// bitwise reproducible and independent of which outputs are asked for; every grid a function of (N, C, K) alone):
//   gauss_nested_factor_kernel  gauss_factor_kernel (gauss_scores_kernel.hip) on the same stage of spd_class.hpp with the
//                         running sums of the log-pivots kept: W_c with the same bits, offset_k[c] for every k.
//   gauss_nested_kernel   workgroup (64 samples, split s of the classes) in the geometry of gauss_whiten.hpp: its stage of
//                         W_c, its product.  Lane (j, q) holds y[16 rb + acc_row(q, reg)] of sample j; the inclusive prefix of
//                         y^2 over the row index is a scan over the lane's registers, an exclusive scan across the four lane
//                         quarters (two cross-lane moves) and a carry from one row block to the next (one move).  float32
//                         has acc_row = 4 q + reg: rows contiguous per quarter, one quarter scan per row block; float64 has
//                         acc_row = q + 4 reg: rows interleaved, a quarter scan per register.  Every lane then owns the
//                         prefixes of its 4 KB rows for every class and carries (best, index) and (max, sum exp) for each of
//                         them across the classes: no class transposition.  offset_k[c] rides through LDS with the stage.
//   gauss_nested_merge_kernel   only where the classes are split: one thread per (sample, k), the splits in the order 0, 1, ...
//   gauss_nested_label_kernel   the label pass of the log-loss with prefixes: one sample per lane, the label range-checked
//                         before it addresses anything, y = W_y (z - mu_y) in double with a running sum of squares.
// A sample is flagged when any of its K prefix rows holds a NaN: all K of its columns are -1 / NaN and it counts once.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <type_traits>

#include "../../include/sqfa_hip.h"
#include "class_pair_loss.hpp"   // namespace math, dispatch_dtype, WorkspaceCursor
#include "gauss_whiten.hpp"
#include "spd_class.hpp"

namespace sqfa {

// ---- the factor pass --------------------------------------------------------------------------------------------------------

template <typename T>
__global__ __launch_bounds__(64) void gauss_nested_factor_kernel(const T* __restrict__ mu, const T* __restrict__ cov,
                                                                 const double* __restrict__ log_prior, int C, int K,
                                                                 T* __restrict__ W, double* __restrict__ offsets,
                                                                 int* __restrict__ bad_out) {
  constexpr int LD = SPD_LD;
  __shared__ double a[SPD_ELEMS];
  __shared__ double s_prefix[64];   // sum_{i <= k} log pivot_i = 2 sum_{i <= k} log (L_c)_ii
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
  if (!bad) bad = !spd_cholesky_prefix<true>(a, K, r, s_prefix);
  if (bad) {
    for (int idx = r; idx < kk; idx += 64) out[idx] = math::nan<T>();
    if (r < K) offsets[(size_t)c * K + r] = math::nan<double>();
    if (r == 0) atomicAdd(bad_out, 1);
    return;
  }
  // the terms of gauss_factor_kernel's offset with k = r + 1 in the place of K (equal to rounding: contraction may differ)
  if (r < K) offsets[(size_t)c * K + r] = -(0.5 * s_prefix[r]) - 0.5 * (r + 1) * 1.8378770664093454835606594728112 + lp;
  spd_invert_lower(a, K, r);
  for (int idx = r; idx < kk; idx += 64) {
    const int rr = idx / K, cc = idx % K;
    out[idx] = cc <= rr ? (T)a[rr * LD + cc] : (T)0;
  }
}

// ---- the running reductions: the tie rule and the merges of gs_take / gs_merge (gauss_scores_kernel.hip), argmax and
// log-sum-exp apart, so that a pass that wants one pays nothing for the other ----------------------------------------------

template <typename T> __device__ __forceinline__ void gn_take_arg(T& best, int& idx, T s, int c) {
  if (s > best || (s == best && c < idx)) {
    best = s;
    idx = c;
  }
}

template <typename T> __device__ __forceinline__ void gn_take_lse(T& m, T& sum, T s) {
  const T d = s - m;
  const T e = math::exp(d > T(0) ? -d : d);   // exp(-|d|); d is NaN only for -inf - -inf, which neither branch below takes
  if (s > m) {
    sum = sum * e + T(1);
    m = s;
  } else if (s > math::neg_inf<T>()) {
    sum += e;
  }
}

template <typename T> __device__ __forceinline__ void gn_merge_lse(T& am, T& asum, T m, T sum) {
  const T mx = m > am ? m : am;
  if (mx > math::neg_inf<T>()) {
    const T lo = (m > am ? asum : sum) * math::exp((m > am ? am : m) - mx);   // the side with the smaller max, scaled
    const T hi = m > am ? sum : asum;
    asum = m == am ? asum + sum : hi + lo;
  }
  am = mx;
}

// ---- the scan ---------------------------------------------------------------------------------------------------------------

// v of lane quarter q - d (the same j), 0 where there is none
template <typename T> __device__ __forceinline__ T gn_from_below(T v, int d, int q) {
  const T o = __shfl_up(v, 16 * d, 64);
  return q >= d ? o : T(0);
}

// pre[reg] = carry + sum of y[i]^2 over the rows i <= acc_row(q, reg) of this row block; returns carry + the block's total,
// the same bits in the four quarters
template <typename T>
__device__ __forceinline__ T gn_scan_block(T (&pre)[4], const typename ProjTraits<T>::Acc& y, T carry, int q, int j) {
  if constexpr (std::is_same_v<T, float>) {   // acc_row = 4 q + reg: the lane's rows are contiguous
    T loc[4];
    loc[0] = y[0] * y[0];
#pragma unroll
    for (int reg = 1; reg < 4; ++reg) loc[reg] = loc[reg - 1] + y[reg] * y[reg];
    const T a = gn_from_below(loc[3], 1, q);        // t_{q-1}
    const T b = gn_from_below(loc[3] + a, 2, q);    // t_{q-2} + t_{q-3}
    const T base = carry + (a + b);
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) pre[reg] = base + loc[reg];
    return __shfl(pre[3], 48 + j, 64);
  } else {                                    // acc_row = q + 4 reg: one scan across the quarters per register
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const T v = y[reg] * y[reg];
      const T a = gn_from_below(v, 1, q);
      const T b = gn_from_below(v + a, 2, q);
      pre[reg] = (carry + (a + b)) + v;
      carry = __shfl(pre[reg], 48 + j, 64);
    }
    return carry;
  }
}

// ---- the scores -------------------------------------------------------------------------------------------------------------

template <typename T> struct GnParams {
  const T* Z;
  long long N;
  const T* mu;
  const T* W;
  const double* offsets;   // (C, K)
  int C, K;
  long long* argmax;       // (N, K) or nullptr
  T* lse;                  // (N, K) or nullptr
  int* nonfinite;
  int groups_per_split, splits;   // groups of 4 classes
  // (splits, N, K) each, splits > 1 only; p_idx -1: the sample holds a NaN
  T* p_best;
  int* p_idx;
  T* p_m;
  T* p_sum;
};

template <typename T, int KB, bool MEANS, bool ARG, bool LSE>
__global__ __launch_bounds__(GW_THREADS) void gauss_nested_kernel(const GnParams<T> p) {
  using Tr = ProjTraits<T>;
  using Stage = WhitenStage<T, KB>;
  constexpr int CS = Stage::CS, KP = Stage::KP, PITCH = Stage::PITCH;
  __shared__ T sW[Stage::W_ELEMS];
  __shared__ T sMu[Stage::MU_ELEMS];
  constexpr int T_UNROLL = CS == 4 && KB == 1 ? 4 : 1;   // the class loop: unrolled only where a class is 4 MFMAs
  __shared__ T sOff[CS * KP];   // offset_k of the stage's classes, -inf from K on
  const int tid = threadIdx.x, l = tid & 63, wave = tid >> 6, q = l >> 4, j = l & 15;
  const int K = p.K, C = p.C, K4 = (K + 3) / 4;
  const long long N = p.N;
  const long long n = (long long)blockIdx.x * GW_ROWS + wave * 16 + j;
  const WhitenClassRange range = whiten_class_range(C, p.groups_per_split, blockIdx.y);
  const int g_lo = range.g_lo, g_hi = range.g_hi, c_end = range.c_end;

  T z[4 * KB];
  whiten_load_sample<T, KB>(z, p.Z, n, N, K, q);

  Stage stage(c_end, K, tid);
  stage.zero(sW);
  // the offsets ride with the stage: global memory to a register with load(), to LDS with store()
  T ov = math::neg_inf<T>();
  auto load_offsets = [&](int cb) {
    const int cls = tid / KP, k = tid % KP;
    const bool ok = tid < CS * KP && cb + cls < c_end && k < K;
    const double v = p.offsets[ok ? (size_t)(cb + cls) * K + k : 0];
    ov = ok ? (T)v : math::neg_inf<T>();
  };
  auto store_offsets = [&]() {
    if (tid < CS * KP) sOff[tid] = ov;
  };
  if (g_lo < g_hi) {
    stage.template load<MEANS>(p.W, p.mu, 4 * g_lo);
    load_offsets(4 * g_lo);
  }

  T best[KB][4], m[KB][4], sum[KB][4];
  int idx[KB][4];
#pragma unroll
  for (int rb = 0; rb < KB; ++rb) {
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      best[rb][reg] = math::neg_inf<T>();
      idx[rb][reg] = INT_MAX;
      m[rb][reg] = math::neg_inf<T>();
      sum[rb][reg] = T(0);
    }
  }
  bool nan = false;

#pragma unroll 1
  for (int g = g_lo; g < g_hi; ++g) {
    if constexpr (CS == 4) {
      __syncthreads();   // the previous stage has been consumed (first pass: the zero fill is done)
      stage.template store<MEANS>(sW, sMu);
      store_offsets();
      __syncthreads();
      if (g + 1 < g_hi) {
        stage.template load<MEANS>(p.W, p.mu, 4 * (g + 1));
        load_offsets(4 * (g + 1));
      }
    }
#pragma unroll T_UNROLL
    for (int t = 0; t < 4; ++t) {
      const int c = 4 * g + t;
      if (c >= c_end) continue;   // uniform over the workgroup
      if constexpr (CS == 1) {
        __syncthreads();
        stage.template store<MEANS>(sW, sMu);
        store_offsets();
        __syncthreads();
        if (c + 1 < c_end) {
          stage.template load<MEANS>(p.W, p.mu, c + 1);
          load_offsets(c + 1);
        }
      }
      const int st = CS == 4 ? t : 0;
      T b[4 * KB];
      whiten_center<T, KB, MEANS>(b, z, sMu + st * KP, K4, q);
      typename Tr::Acc y[KB];
      whiten_product<T, KB>(y, sW + st * KP * PITCH, b, K, K4, j, q);
      T carry = T(0);
#pragma unroll
      for (int rb = 0; rb < KB; ++rb) {
        if (rb * 16 < K) {   // uniform
          T pre[4];
          carry = gn_scan_block<T>(pre, y[rb], carry, q, j);
#pragma unroll
          for (int reg = 0; reg < 4; ++reg) {
            const T sc = T(-0.5) * pre[reg] + sOff[st * KP + rb * 16 + Tr::acc_row(q, reg)];
            if (sc != sc) nan = true;
            if constexpr (ARG) gn_take_arg(best[rb][reg], idx[rb][reg], sc, c);
            if constexpr (LSE) gn_take_lse(m[rb][reg], sum[rb][reg], sc);
          }
        }
      }
    }
  }

  // a NaN in any row of the sample, whichever quarter holds it
  int flag = nan ? 1 : 0;
  flag |= __shfl_xor(flag, 16, 64);
  flag |= __shfl_xor(flag, 32, 64);
  nan = flag != 0;
  const bool live = n < N;
  const bool split = p.splits > 1;
#pragma unroll
  for (int rb = 0; rb < KB; ++rb) {
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int k = rb * 16 + Tr::acc_row(q, reg);
      if (!live || k >= K) continue;
      if (split) {
        const size_t at = ((size_t)blockIdx.y * (size_t)N + (size_t)n) * K + k;
        p.p_idx[at] = nan ? -1 : (ARG ? idx[rb][reg] : 0);
        if constexpr (ARG) p.p_best[at] = best[rb][reg];
        if constexpr (LSE) {
          p.p_m[at] = m[rb][reg];
          p.p_sum[at] = sum[rb][reg];
        }
      } else {
        const size_t at = (size_t)n * K + k;
        if constexpr (ARG) p.argmax[at] = nan ? -1 : idx[rb][reg];
        if constexpr (LSE) p.lse[at] = nan ? math::nan<T>() : m[rb][reg] + math::log(sum[rb][reg]);
      }
    }
  }
  if (split) return;
  const unsigned long long bal = __ballot(q == 0 && live && nan);
  if (l == 0 && bal != 0) atomicAdd(p.nonfinite, __popcll(bal));
}

// one thread per (sample, k): the splits' partial reductions in the order s = 0, 1, ...
template <typename T>
__global__ __launch_bounds__(GW_THREADS) void gauss_nested_merge_kernel(const GnParams<T> p) {
  const size_t cells = (size_t)p.N * p.K;
  const size_t e = (size_t)blockIdx.x * GW_THREADS + threadIdx.x;
  bool count = false;
  if (e < cells) {
    const bool arg = p.argmax != nullptr, lse = p.lse != nullptr;
    int idx = p.p_idx[e];
    bool nan = idx < 0;
    T best = arg ? p.p_best[e] : T(0), m = lse ? p.p_m[e] : T(0), sum = lse ? p.p_sum[e] : T(0);
    if (nan) idx = INT_MAX;
    for (int s = 1; s < p.splits; ++s) {
      const size_t at = (size_t)s * cells + e;
      const int oi = p.p_idx[at];
      nan = nan || oi < 0;
      if (arg) gn_take_arg(best, idx, p.p_best[at], oi < 0 ? INT_MAX : oi);   // gs_merge's rule is gs_take's
      if (lse) gn_merge_lse(m, sum, p.p_m[at], p.p_sum[at]);
    }
    if (arg) p.argmax[e] = nan ? -1 : idx;
    if (lse) p.lse[e] = nan ? math::nan<T>() : m + math::log(sum);
    count = nan && e % (size_t)p.K == 0;   // a flagged sample is flagged in all K columns: counted in its first
  }
  const unsigned long long bal = __ballot(count);
  if ((threadIdx.x & 63) == 0 && bal != 0) atomicAdd(p.nonfinite, __popcll(bal));
}

// ---- the label pass ---------------------------------------------------------------------------------------------------------

template <typename T, bool MEANS>
__global__ __launch_bounds__(GW_ROWS) void gauss_nested_label_kernel(const T* __restrict__ Z, const long long* __restrict__ labels,
                                                                     long long N, const T* __restrict__ mu,
                                                                     const T* __restrict__ W, const double* __restrict__ offsets,
                                                                     int C, int K, const T* __restrict__ lse,
                                                                     T* __restrict__ ll_out, int* __restrict__ flags) {
  __shared__ T sD[GW_KMAX * GW_ROWS];   // [k][lane]: a lane reads back only what it wrote
  const int tid = threadIdx.x;
  const long long n = (long long)blockIdx.x * GW_ROWS + tid;
  const bool live = n < N;
  const long long lab = live ? labels[n] : 0;
  const bool in_range = lab >= 0 && lab < (long long)C;
  const int c = in_range ? (int)lab : 0;   // the label is data: checked before it addresses anything
  const double* off = offsets + (size_t)c * K;
  const bool prior0 = off[0] == -(double)INFINITY;   // log pi_c = -inf is in every offset_k
  for (int k = 0; k < K; ++k) {
    T d = T(0);
    if (live) {
      d = Z[(size_t)n * K + k];
      if constexpr (MEANS) d -= mu[(size_t)c * K + k];
    }
    sD[k * GW_ROWS + tid] = d;
  }
  const T* w = W + (size_t)c * K * K;
  double sq = 0.0;
  for (int i = 0; i < K; ++i) {
    double a = 0.0;
    for (int k = 0; k <= i; ++k) a += (double)w[i * K + k] * (double)sD[k * GW_ROWS + tid];
    sq += a * a;
    if (!live) continue;
    const T le = lse[(size_t)n * K + i];
    double ll = -0.5 * sq + off[i] - (double)le;
    if (C == 1) ll = 0.0;    // the posterior of the only class
    if (ll > 0.0) ll = 0.0;  // a log posterior; NaN stays
    if (!in_range || prior0 || le != le) ll = math::nan<double>();
    ll_out[(size_t)n * K + i] = (T)ll;
  }
  const unsigned long long out = __ballot(live && !in_range), zero = __ballot(live && in_range && prior0);
  if (tid == 0) {
    if (out != 0) atomicAdd(flags + 1, __popcll(out));
    if (zero != 0) atomicAdd(flags + 2, __popcll(zero));
  }
}

// ---- host -------------------------------------------------------------------------------------------------------------------

struct GnLayout {
  int groups_per_split, splits;
  size_t off_best, off_m, off_sum, off_idx, total;   // splits > 1: four (splits, N, K) arrays [best T][m T][sum T][idx int]
};

static bool gn_layout(long long N, int C, int K, int dtype, GnLayout* w) {
  if (!whiten_class_split(N, C, K, dtype, &w->groups_per_split, &w->splits)) return false;
  const size_t cells = w->splits > 1 ? (size_t)w->splits * (size_t)N * (size_t)K : 0;
  WorkspaceCursor ws;
  w->off_best = ws.take(cells * dtype_bytes(dtype));
  w->off_m = ws.take(cells * dtype_bytes(dtype));
  w->off_sum = ws.take(cells * dtype_bytes(dtype));
  w->off_idx = ws.take(cells * sizeof(int));
  w->total = ws.at < 16 ? 16 : ws.at;
  return true;
}

template <typename T>
static hipError_t run_nested(const void* Z, long long N, const void* mu, const void* W, const double* offsets, int C, int K,
                             long long* argmax, void* lse, int* nonfinite, char* ws, const GnLayout& lay,
                             hipStream_t stream) {
  GnParams<T> p{};
  p.Z = static_cast<const T*>(Z);
  p.N = N;
  p.mu = static_cast<const T*>(mu);
  p.W = static_cast<const T*>(W);
  p.offsets = offsets;
  p.C = C;
  p.K = K;
  p.argmax = argmax;
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
    constexpr int KB = decltype(kb)::value;
    constexpr bool MEANS = decltype(means)::value;
    if (argmax != nullptr && lse != nullptr)
      hipLaunchKernelGGL((gauss_nested_kernel<T, KB, MEANS, true, true>), grid, dim3(GW_THREADS), 0, stream, p);
    else if (argmax != nullptr)
      hipLaunchKernelGGL((gauss_nested_kernel<T, KB, MEANS, true, false>), grid, dim3(GW_THREADS), 0, stream, p);
    else
      hipLaunchKernelGGL((gauss_nested_kernel<T, KB, MEANS, false, true>), grid, dim3(GW_THREADS), 0, stream, p);
  });
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (lay.splits > 1) {   // few sample tiles (whiten_class_split): N K fits a grid by far
    const size_t cells = (size_t)N * K;
    hipLaunchKernelGGL((gauss_nested_merge_kernel<T>), dim3((unsigned)((cells + GW_THREADS - 1) / GW_THREADS)),
                       dim3(GW_THREADS), 0, stream, p);
    e = hipGetLastError();
  }
  return e;
}

}  // namespace sqfa

using namespace sqfa;

extern "C" size_t sqfa_gauss_scores_nested_workspace_bytes(long long N, int C, int K, int dtype) {
  GnLayout w;
  return gn_layout(N, C, K, dtype, &w) ? w.total : 0;
}

extern "C" int sqfa_gauss_class_factors_nested(const void* means, const void* cov, const double* log_priors, int C, int K,
                                               int dtype, void* W_out, double* offsets_out, int* bad_out, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const bool nulls = cov == nullptr || W_out == nullptr || offsets_out == nullptr || bad_out == nullptr || C < 1 || K < 1;
  const int rc = check_gauss_args("sqfa_gauss_class_factors_nested", nulls, "null covariances or outputs, C < 1 or K < 1",
                                  dtype, nullptr, K, false, 0, nullptr, 0);
  if (rc != SQFA_OK) return rc;
  if (hipMemsetAsync(bad_out, 0, sizeof(int), stream) != hipSuccess) return SQFA_ERR_LAUNCH;
  dispatch_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL((gauss_nested_factor_kernel<T>), dim3(C), dim3(64), 0, stream, static_cast<const T*>(means),
                       static_cast<const T*>(cov), log_priors, C, K, static_cast<T*>(W_out), offsets_out, bad_out);
  });
  return hipGetLastError() == hipSuccess ? SQFA_OK : SQFA_ERR_LAUNCH;
}

extern "C" int sqfa_gauss_scores_nested(const void* Z, long long N, const void* means, const void* W, const double* offsets,
                                        int C, int K, int dtype, long long* argmax_out, void* logsumexp_out,
                                        int* nonfinite_out, void* workspace, size_t workspace_bytes, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  GnLayout lay;
  const size_t need = gn_layout(N, C, K, dtype, &lay) ? lay.total : 0;
  const bool nulls = Z == nullptr || W == nullptr || offsets == nullptr || nonfinite_out == nullptr || N < 1 || C < 1 || K < 1;
  const int rc = check_gauss_args("sqfa_gauss_scores_nested", nulls,
                                  "null samples, factors, offsets or counter, N < 1, C < 1 or K < 1", dtype,
                                  argmax_out == nullptr && logsumexp_out == nullptr ? "no output asked for" : nullptr, K, true,
                                  need, workspace, workspace_bytes);
  if (rc != SQFA_OK) return rc;
  const hipError_t e = dispatch_dtype(dtype, [&](auto t) {
    return run_nested<decltype(t)>(Z, N, means, W, offsets, C, K, argmax_out, logsumexp_out, nonfinite_out,
                                   static_cast<char*>(workspace), lay, stream);
  });
  return e == hipSuccess ? SQFA_OK : SQFA_ERR_LAUNCH;
}

extern "C" int sqfa_gauss_label_scores_nested(const void* Z, const long long* labels, long long N, const void* means,
                                              const void* W, const double* offsets, int C, int K, int dtype,
                                              const void* logsumexp, void* ll_out, int* flags_out, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const bool nulls = Z == nullptr || labels == nullptr || W == nullptr || offsets == nullptr || logsumexp == nullptr ||
                     ll_out == nullptr || flags_out == nullptr || N < 1 || C < 1 || K < 1;
  const long long blocks = (N + GW_ROWS - 1) / GW_ROWS;
  const int rc = check_gauss_args("sqfa_gauss_label_scores_nested", nulls,
                                  "null samples, labels, factors, offsets, logsumexp or outputs, N < 1, C < 1 or K < 1", dtype,
                                  nullptr, K, false, 0, nullptr, 0);
  if (rc != SQFA_OK) return rc;
  if (blocks > (long long)INT_MAX) {
    set_last_error("sqfa_gauss_label_scores_nested: more than 2^31 - 1 sample tiles");
    return SQFA_ERR_UNSUPPORTED_M;
  }
  if (hipMemsetAsync(flags_out + 1, 0, 2 * sizeof(int), stream) != hipSuccess) return SQFA_ERR_LAUNCH;
  dispatch_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    const dim3 grid((unsigned)blocks), block(GW_ROWS);
    if (means != nullptr)
      hipLaunchKernelGGL((gauss_nested_label_kernel<T, true>), grid, block, 0, stream, static_cast<const T*>(Z), labels, N,
                         static_cast<const T*>(means), static_cast<const T*>(W), offsets, C, K,
                         static_cast<const T*>(logsumexp), static_cast<T*>(ll_out), flags_out);
    else
      hipLaunchKernelGGL((gauss_nested_label_kernel<T, false>), grid, block, 0, stream, static_cast<const T*>(Z), labels, N,
                         static_cast<const T*>(means), static_cast<const T*>(W), offsets, C, K,
                         static_cast<const T*>(logsumexp), static_cast<T*>(ll_out), flags_out);
  });
  return hipGetLastError() == hipSuccess ? SQFA_OK : SQFA_ERR_LAUNCH;
}
