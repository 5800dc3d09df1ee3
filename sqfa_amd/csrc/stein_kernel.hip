// stein_kernel.hip -- fused closure loss of the Stein divergence (Jensen-Bregman log-det divergence, S-divergence) between
// the n SPD matrices S_c, as the distance_fun of SecondMomentsSQFA:
//     S_ij = logdet((S_i + S_j)/2) - 1/2 logdet S_i - 1/2 logdet S_j
//     D_ij = S_ij  |  sqrt(S_ij + eps),  S_ij clamped at 0 from below,   loss = sum_{i>j} w_ij D_ij
// and its gradient  gradS_i = sum_{j != i} c_ij 1/2 (Sbar_ij^-1 - S_i^-1),  c_ij = w_ij dD/dS.  Cholesky factors only: no
// eigen-decomposition, no means.
//
// Three stages on the caller's stream:
//   1. spd_inverse_kernel (spd_class.hip, the per-class factor stage shared with jeffreys_kernel.hip): per class, Cholesky
//      in double: ld_c = logdet S_c (double) and P_c = S_c^-1 in the dtype, exactly symmetric.  A pivot that is not positive
//      gives ld_c = NaN and a NaN matrix.
//   1b. stein_logdet_kernel: ld_c once more, from the pair pass's own factorisation in the dtype (it replaces stage 1's
//      value: both sides of S_ij then carry the same rounding).
//   2. stein_pair_kernel: the pass over the ordered pairs.  A 256-thread workgroup owns ONE class i; its NS = 256 / G lane
//      groups of G lanes (a group never leaves its wave) take the classes j = s, s + NS, ...: NS pairs in flight per
//      workgroup.  Lane r of a group holds row r of Sbar = (S_i + S_j)/2 in registers (MMAX values; rows and columns beyond
//      m are those of the identity, so no loop has a bounds check and logdet and inverse are exact).  S_i sits in LDS, S_j
//      comes from global memory (by symmetry as column r: consecutive lanes, consecutive addresses).
//        - Cholesky Sbar = U^T U, right-looking on whole symmetric rows: step k broadcasts row k from lane k (one
//          cross-lane read per entry: v_readlane for G = 64, ds_bpermute below), every lane r > k updates its row.  Lane k
//          keeps its pivot; logdet Sbar = sum of log(pivot), one double log per lane and one group sum.
//        - lane r solves U^T y = e_r in the same loop (the same broadcasts) and, where a gradient is asked for, U x = y
//          after it: x is row r of Sbar^-1; acc_i += c_ij x.
//      Up to m = 16 acc_i lives in registers and the NS groups are combined through LDS at the end by a tree in a fixed
//      order; above, every group adds into its own (m,m) slice of the workspace and the finish kernel sums the slices in
//      that order.  One writer per address, no atomics, bitwise reproducible.  The workgroup also writes csum_i =
//      sum_j c_ij, its partial loss and counters.
//   3. stein_finish_kernel: gradS_i = 1/2 (sym(acc_i) - csum_i P_i), lower triangle in double, mirrored; then
//      launch_pair_loss_finalize (class_pair_loss.hip) for the loss and counters.
#include <hip/hip_runtime.h>

#include "../../include/sqfa_hip.h"
#include "class_pair_loss.hpp"
#include "pair_kernel.hpp"   // group_sum
#include "spd_class.hpp"     // stage 1

namespace sqfa {

struct SteinParams : PairLossParams {
  const void* S;      // (n,m,m)
  const double* ld;   // (n) logdet S_c (stage 1)
  void* acc;          // (slices,n,m,m) partial sums of sum_j c_ij Sbar_ij^-1, or nullptr (forward only)
  double* csum;       // (n) sum_j c_ij
  int sqrt_mode;
};

// The value is computed here and now.  x is read only where a gradient is asked for, and without this the compiler moves
// the forward solve behind that branch and keeps every broadcast of the factorisation alive for it (hundreds of registers).
__device__ __forceinline__ void st_pin(float& v) { asm volatile("" : "+v"(v)); }
__device__ __forceinline__ void st_pin(double& v) { asm volatile("" : "+v"(v)); }

// the value lane `k` of the caller's group of G lanes holds (k a compile-time constant after unrolling)
template <int G> __device__ __forceinline__ float st_bcast(float v, int k) {
  if constexpr (G == 64) return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), k));
  else return __shfl(v, k, G);
}
template <int G> __device__ __forceinline__ double st_bcast(double v, int k) {
  if constexpr (G == 64)
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), k), __builtin_amdgcn_readlane(__double2loint(v), k));
  else return __shfl(v, k, G);
}

// ---- stage 2: the pass over the ordered pairs ------------------------------------------------------------------------------
// Where acc_i lives: in registers up to MMAX = 16 (the groups are combined through LDS at the end); above, every group adds
// into its own (m,m) slice of the workspace (2 MMAX memory operations per lane and pair against MMAX^2 multiply-adds) and
// the finish kernel sums the slices in the order s = 0, 1, ...
template <int MMAX> constexpr bool stein_reg_acc() { return MMAX <= 16; }
// (n,m,m) slices of acc the pair pass writes: one where the accumulators are registers, one per lane group above
static int stein_slices(int m) { return m <= 16 ? 1 : (m <= 32 ? 256 / 32 : 256 / 64); }

template <typename T, int G, int MMAX, bool WEIGHTED>
__global__ __launch_bounds__(256) void stein_pair_kernel(const SteinParams p) {
  static_assert(MMAX <= G && G >= 4 && G <= 64 && 256 % G == 0, "one matrix row per lane, groups inside a wave");
  constexpr int NS = 256 / G;
  constexpr bool REG_ACC = stein_reg_acc<MMAX>();
  static_assert((NS & (NS - 1)) == 0, "the combine tree halves the groups");
  __shared__ T s_own[MMAX * G];                               // S_i, entry (c, r) at c G + r
  __shared__ T s_comb[REG_ACC ? (NS / 2) * MMAX * G : 1];     // the combine tree's hand-overs (REG_ACC)
  __shared__ double s_loss[NS], s_csum[NS];
  __shared__ int s_cnt[NS][2];
  const int tid = threadIdx.x, n = p.n, m = p.m, mm = m * m;
  const int lane = tid % G, s = tid / G;
  const int i = blockIdx.x;   // the grid has n workgroups
  const bool rvalid = lane < m;
  const int lanec = rvalid ? lane : 0;   // clamped: every address formed below is inside its array
  const T* S = static_cast<const T*>(p.S);
  const T* W = static_cast<const T*>(p.W);
  T* dist = static_cast<T*>(p.dist);
  const bool sqrt_mode = p.sqrt_mode != 0, want_grad = p.acc != nullptr;
  const T w = pair_weight<T>(p), eps = pair_eps<T>(p);

  for (int q = tid; q < MMAX * G; q += 256) {
    const int c = q / G, r = q % G;
    const bool ok = c < m && r < m;
    const T v = S[(size_t)i * mm + (ok ? c * m + r : 0)];
    s_own[q] = ok ? v : T(0);
  }
  __syncthreads();
  const double ld_i = p.ld[i];

  T acc[REG_ACC ? MMAX : 1];
#pragma unroll
  for (int c = 0; c < (REG_ACC ? MMAX : 1); ++c) acc[c] = T(0);
  // this group's slice of the workspace, entry (lane, c) at slice[c m] (the finish symmetrises)
  T* slice = want_grad ? static_cast<T*>(p.acc) + ((size_t)(REG_ACC ? 0 : s) * n + i) * mm + lanec : nullptr;
  if constexpr (!REG_ACC) {
    if (want_grad && rvalid)
      for (int c = 0; c < m; ++c) slice[c * m] = T(0);
  }
  double loss_acc = 0.0, csum = 0.0;
  int n_nan = 0, n_inf = 0;

  // every group makes the same number of rounds (the cross-lane reads below see whole waves); a group without a pair in its
  // last round, or on the diagonal, works on a clamped class and drops the result
#pragma unroll 1
  for (int j0 = 0; j0 < n; j0 += NS) {
    const int jr = j0 + s;
    const bool valid = jr < n && jr != i;   // uniform over the group
    const int j = jr < n ? jr : n - 1;
    const T* Sj = S + (size_t)j * mm + lanec;   // entry (c, lane) at Sj[c m]
    T a[MMAX], x[MMAX];
#pragma unroll
    for (int c = 0; c < MMAX; ++c) {
      const bool ok = rvalid && c < m;
      const T sj = Sj[ok ? c * m : 0];
      a[c] = ok ? T(0.5) * (s_own[c * G + lane] + sj) : (c == lane ? T(1) : T(0));
      x[c] = c == lane ? T(1) : T(0);
      if (c % 8 == 7) __builtin_amdgcn_sched_barrier(0);   // eight loads in flight, not MMAX
    }
    // Cholesky Sbar = U^T U and the forward solve U^T y = e_lane (y in x), step by step.  Lane k keeps row k as it stands
    // at step k, U[k][c] sqrt(pivot_k), and 1 / sqrt(pivot_k) beside it.
    T pivot = T(1), invd = T(1);
#pragma unroll
    for (int k = 0; k < MMAX; ++k) {
      __builtin_amdgcn_sched_barrier(0);   // one step's broadcasts in flight, not the whole factorisation's
      const T dk = st_bcast<G>(a[k], k);
      const T rinv = math::rsqrt(dk);   // 1 / U[k][k]; NaN for a negative pivot, inf for a zero one
      if (lane == k) {
        pivot = dk;
        invd = rinv;
      }
      const T lrk = lane > k ? a[k] * rinv : T(0);   // U[k][lane]; 0 leaves the rows up to k as they are
      x[k] *= rinv;
      const T xk = x[k];
#pragma unroll
      for (int c = k + 1; c < MMAX; ++c) {
        const T ukc = st_bcast<G>(a[c], k) * rinv;   // U[k][c]
        a[c] -= lrk * ukc;
        x[c] -= ukc * xk;
        st_pin(x[c]);
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    const double ldbar = group_sum<G>(log((double)pivot));
    const double Sd = ldbar - 0.5 * (ld_i + p.ld[j]);
    // S >= 0 mathematically; the difference of three rounded logarithms comes out negative for near-equal classes: taken as
    // 0 there, with derivative 0 (NaN stays NaN: the comparison is false for it)
    const bool clamped = Sd < 0.0;
    const T Sv = clamped ? T(0) : (T)Sd;
    T wij = w;
    if constexpr (WEIGHTED) wij = W[(size_t)i * n + j];
    T D, cij;
    if (sqrt_mode) {
      D = math::sqrt(Sv + eps);
      cij = clamped ? T(0) : T(0.5) * wij / D;
    } else {
      D = Sv;
      cij = clamped ? T(0) : wij;
    }
    if (want_grad) {   // uniform over the workgroup
      // backward solve U x = y, last row first: x becomes row `lane` of Sbar^-1
#pragma unroll
      for (int k = MMAX - 1; k >= 0; --k) {
        __builtin_amdgcn_sched_barrier(0);
        T v = T(0);
#pragma unroll
        for (int c = k + 1; c < MMAX; ++c) v += st_bcast<G>(a[c], k) * x[c];
        const T rk = st_bcast<G>(invd, k);
        x[k] = (x[k] - rk * v) * rk;
        st_pin(x[k]);
      }
      __builtin_amdgcn_sched_barrier(0);
      if (valid) {
        if constexpr (REG_ACC) {
#pragma unroll
          for (int c = 0; c < MMAX; ++c) acc[c] += cij * x[c];
        } else {
          if (rvalid) {
#pragma unroll
            for (int c = 0; c < MMAX; ++c)
              if (c < m) slice[c * m] += cij * x[c];
          }
        }
        csum += (double)cij;
      }
    }
    if (valid && j < i) {
      loss_acc += WEIGHTED ? (double)wij * (double)D : (double)D;
      if (D != D) ++n_nan;
      else if (D - D != T(0)) ++n_inf;
    }
    if (valid && dist != nullptr && lane == 0) dist[(size_t)i * n + j] = D;
  }

  // combine the NS groups: the scalars in the order s = 0, 1, ..., NS - 1, the register sums by a tree
  if (lane == 0) {
    s_loss[s] = loss_acc;
    s_csum[s] = csum;
    s_cnt[s][0] = n_nan;
    s_cnt[s][1] = n_inf;
  }
  if constexpr (REG_ACC) {
    if (want_grad) {
      // a tree in a fixed order: in the round of `stride` group s + stride hands its sums to group s, s a multiple of
      // 2 stride; log2(NS) rounds of two barriers, NS / (2 stride) hand-overs side by side
      for (int stride = 1; stride < NS; stride *= 2) {
        T* mine = s_comb + (s / (2 * stride)) * (MMAX * G) + lane;
        if (s % (2 * stride) == stride) {
#pragma unroll
          for (int c = 0; c < MMAX; ++c) mine[c * G] = acc[c];
        }
        __syncthreads();
        if (s % (2 * stride) == 0) {
#pragma unroll
          for (int c = 0; c < MMAX; ++c) acc[c] += mine[c * G];
        }
        __syncthreads();
      }
    }
  }
  __syncthreads();
  if (s != 0) return;
  if (lane == 0) {
    double l = 0.0, cs = 0.0;
    int c0 = 0, c1 = 0;
    for (int q = 0; q < NS; ++q) {
      l += s_loss[q];
      cs += s_csum[q];
      c0 += s_cnt[q][0];
      c1 += s_cnt[q][1];
    }
    p.loss_part[i] = WEIGHTED ? l : p.weight * l;   // weighted: w_ij went into the sum pair by pair
    p.cnt_part[2 * i] = c0;
    p.cnt_part[2 * i + 1] = c1;
    p.csum[i] = cs;
    if (dist != nullptr) dist[(size_t)i * n + i] = sqrt_mode ? math::sqrt(eps) : T(0);   // sqrt(|0| + eps), as the torch expression
  }
  if constexpr (REG_ACC) {
    if (!want_grad || !rvalid) return;
#pragma unroll
    for (int c = 0; c < MMAX; ++c)
      if (c < m) slice[c * m] = acc[c];
  }
}

// ---- stage 1b: ld_c again, by the pair pass's own arithmetic ----------------------------------------------------------------
// The pair pass takes logdet Sbar from its Cholesky in the dtype; ld_c from stage 1's double Cholesky differs from that by
// the rounding of the dtype's factorisation (float32: eps cond), which does not cancel in S_ij and exceeds S_ij for
// near-equal classes.  Here one lane group factors S_c = (S_c + S_c)/2 with the statements of the pair pass, so that both
// sides of the difference carry the same rounding and two bitwise equal classes are exactly 0 apart (the Gaussian pair
// kernel's pre-pass does the same for Bhattacharyya).  A pivot that is not positive gives NaN or -inf here too.
template <typename T, int G, int MMAX>
__global__ __launch_bounds__(256) void stein_logdet_kernel(const SteinParams p, double* __restrict__ ld_out) {
  constexpr int NS = 256 / G;
  const int tid = threadIdx.x, n = p.n, m = p.m, mm = m * m;
  const int lane = tid % G, s = tid / G;
  const bool rvalid = lane < m;
  const int lanec = rvalid ? lane : 0;
  const int cr = blockIdx.x * NS + s;
  const int cls = cr < n ? cr : n - 1;   // clamped: every group makes the same steps
  const T* Sc = static_cast<const T*>(p.S) + (size_t)cls * mm + lanec;
  T a[MMAX];
#pragma unroll
  for (int c = 0; c < MMAX; ++c) {
    const bool ok = rvalid && c < m;
    const T sj = Sc[ok ? c * m : 0];
    a[c] = ok ? T(0.5) * (sj + sj) : (c == lane ? T(1) : T(0));
    if (c % 8 == 7) __builtin_amdgcn_sched_barrier(0);
  }
  T pivot = T(1);
#pragma unroll
  for (int k = 0; k < MMAX; ++k) {
    __builtin_amdgcn_sched_barrier(0);
    const T dk = st_bcast<G>(a[k], k);
    const T rinv = math::rsqrt(dk);
    if (lane == k) pivot = dk;
    const T lrk = lane > k ? a[k] * rinv : T(0);
#pragma unroll
    for (int c = k + 1; c < MMAX; ++c) {
      const T ukc = st_bcast<G>(a[c], k) * rinv;
      a[c] -= lrk * ukc;
    }
  }
  __builtin_amdgcn_sched_barrier(0);
  const double ld = group_sum<G>(log((double)pivot));
  if (cr < n && lane == 0) ld_out[cr] = ld;
}

template <typename T, int G, int MMAX>
static hipError_t launch_stein_logdet(const SteinParams& p, double* ld_out, hipStream_t stream) {
  constexpr int NS = 256 / G;
  hipLaunchKernelGGL((stein_logdet_kernel<T, G, MMAX>), dim3((p.n + NS - 1) / NS), dim3(256), 0, stream, p, ld_out);
  return hipGetLastError();
}

// ---- stage 3: gradS_i = 1/2 (sym(acc_i) - csum_i P_i) ------------------------------------------------------------------------
// acc_i: the sum of the `slices` (n,m,m) slices of the pair pass, in the order s = 0, 1, ...
template <typename T>
__global__ __launch_bounds__(256) void stein_finish_kernel(const T* __restrict__ P, const T* __restrict__ acc, int slices,
                                                            const double* __restrict__ csum, T* __restrict__ grad, int m) {
  const int mm = m * m;
  const size_t base = (size_t)blockIdx.x * mm, stride = (size_t)gridDim.x * mm;
  const double cs = csum[blockIdx.x];
  for (int idx = threadIdx.x; idx < mm; idx += 256) {
    const int a = idx / m, b = idx % m;
    if (b > a) continue;
    double lo = 0.0, up = 0.0;
    for (int q = 0; q < slices; ++q) {
      lo += (double)acc[q * stride + base + a * m + b];
      up += (double)acc[q * stride + base + b * m + a];
    }
    const T v = (T)(0.5 * (0.5 * (lo + up) - cs * (double)P[base + idx]));
    grad[base + a * m + b] = v;
    grad[base + b * m + a] = v;
  }
}

template <typename T, int G, int MMAX>
static hipError_t launch_stein(const SteinParams& p, hipStream_t stream) {
  if (stein_slices(p.m) != (stein_reg_acc<MMAX>() ? 1 : 256 / G)) return hipErrorInvalidValue;   // the workspace layout's rule
  // stage 1b, the instantiation of the pair pass that follows: it replaces stage 1's ld_c
  const hipError_t e = launch_stein_logdet<T, G, MMAX>(p, const_cast<double*>(p.ld), stream);
  if (e != hipSuccess) return e;
  if (p.W != nullptr) hipLaunchKernelGGL((stein_pair_kernel<T, G, MMAX, true>), dim3(p.n), dim3(256), 0, stream, p);
  else hipLaunchKernelGGL((stein_pair_kernel<T, G, MMAX, false>), dim3(p.n), dim3(256), 0, stream, p);
  return hipGetLastError();
}

// lanes per group by matrix size: the smallest group that holds one row per lane
template <typename T>
static hipError_t dispatch_stein(const SteinParams& p, hipStream_t stream) {
  const int m = p.m;
  if (m <= 4) return launch_stein<T, 4, 4>(p, stream);
  if (m <= 8) return launch_stein<T, 8, 8>(p, stream);
  if (m <= 16) return launch_stein<T, 16, 16>(p, stream);
  if (m <= 24) return launch_stein<T, 32, 24>(p, stream);
  if (m <= 32) return launch_stein<T, 32, 32>(p, stream);
  if (m <= 48) return launch_stein<T, 64, 48>(p, stream);
  return launch_stein<T, 64, 64>(p, stream);
}

// workspace: [P (n,m,m) dtype] [acc (slices,n,m,m) dtype] [ld (n) double] [csum (n) double] [partial losses (n) double]
//            [counts (n,2) int]
struct SteinLayout {
  size_t off_p, off_acc, off_ld, off_csum, off_loss, off_cnt, total;   // total 0: no layout for these sizes
};
static SteinLayout stein_layout(int n, int m, int dtype) {
  SteinLayout w{};
  if (n < 2 || m < 1 || m > 64 || (dtype != SQFA_F32 && dtype != SQFA_F64)) return w;
  const size_t mat = (size_t)n * m * m;
  WorkspaceCursor ws;
  w.off_p = ws.take(mat * dtype_bytes(dtype));
  w.off_acc = ws.take(stein_slices(m) * mat * dtype_bytes(dtype));
  w.off_ld = ws.take((size_t)n * sizeof(double));
  w.off_csum = ws.take((size_t)n * sizeof(double));
  w.off_loss = ws.take((size_t)n * sizeof(double));
  w.off_cnt = ws.take((size_t)n * 2 * sizeof(int));
  w.total = ws.at;
  return w;
}
}  // namespace sqfa

using namespace sqfa;

extern "C" size_t sqfa_stein_workspace_bytes(int n, int m, int dtype) { return stein_layout(n, m, dtype).total; }

extern "C" int sqfa_stein_pairwise_loss(const void* S, int n, int m, int dtype, int sqrt_mode, double eps,
                                        const void* pair_weights, double uniform_weight, void* loss_out, void* gradS_out,
                                        void* dist_out, int* nonfinite_out, void* workspace, size_t workspace_bytes,
                                        void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const SteinLayout w = stein_layout(n, m, dtype);
  const int rc = check_pair_loss_args("sqfa_stein_pairwise_loss", "matrices", S == nullptr, n, m, dtype,
                                      sqrt_mode == 0 || sqrt_mode == 1, nullptr, w.total, "sqfa_stein_workspace_bytes",
                                      workspace, workspace_bytes);
  if (rc != SQFA_OK) return rc;
  unsigned char* ws = static_cast<unsigned char*>(workspace);
  const bool want_grad = gradS_out != nullptr;
  double* ld = reinterpret_cast<double*>(ws + w.off_ld);
  // 1. per-class inverses, and log-determinants (stage 1b writes them again: ld holds defined values whatever the dispatch)
  if (launch_spd_inverse(S, n, m, dtype, ws + w.off_p, ld, stream) != hipSuccess) return SQFA_ERR_LAUNCH;
  // 2. the pass over the ordered pairs
  SteinParams p{};
  p.S = S;
  p.ld = ld;
  p.acc = want_grad ? ws + w.off_acc : nullptr;
  p.csum = reinterpret_cast<double*>(ws + w.off_csum);
  p.sqrt_mode = sqrt_mode;
  fill_pair_loss_params(p, n, m, eps, pair_weights, uniform_weight, dist_out, reinterpret_cast<double*>(ws + w.off_loss),
                        reinterpret_cast<int*>(ws + w.off_cnt));
  if (dispatch_dtype(dtype, [&](auto t) { return dispatch_stein<decltype(t)>(p, stream); }) != hipSuccess)
    return SQFA_ERR_LAUNCH;
  // 3. the per-class finish
  if (want_grad) {
    dispatch_dtype(dtype, [&](auto t) {
      using T = decltype(t);
      hipLaunchKernelGGL((stein_finish_kernel<T>), dim3(n), dim3(256), 0, stream, reinterpret_cast<const T*>(ws + w.off_p),
                         static_cast<const T*>(p.acc), stein_slices(m), p.csum, static_cast<T*>(gradS_out), m);
    });
    if (hipGetLastError() != hipSuccess) return SQFA_ERR_LAUNCH;
  }
  // 4. loss and counters
  if (launch_pair_loss_finalize(p.loss_part, p.cnt_part, n, dtype, loss_out, nonfinite_out, stream) != hipSuccess)
    return SQFA_ERR_LAUNCH;
  return SQFA_OK;
}
