// gauss_whiten.hpp -- the whitened product y = W_c (z - mu_c) of the Gaussian class scores on the exact MFMA, once: the
// geometry, the LDS stage of W_c, the operand map, the order in which |y|^2 is summed, the class-split policy and the frame
// of the entry points.  gauss_scores_kernel (gauss_scores_kernel.hip), gl_sample_kernel and gl_class_kernel
// (gauss_log_loss_kernel.hip) are written on it: the log-loss gradients are only right because the two recompute a class
// score with exactly the bits the scores pass put into lse_n (DESIGN Q2), and they do because all three call
// whiten_product / whiten_sq_partial and a quarter reduction below, and nothing else, for the score.  (gl_class_kernel keeps
// W_c resident and forms its centred differences in a statement of its own: see there.)
//
// Geometry.  A workgroup is 256 threads = 4 waves of 16 samples; a lane (j = l & 15, q = l >> 4) keeps z[j][4 s + q] of its
// sample in registers.  Classes come in groups of 4; a workgroup of the sample-owned passes takes (64 samples, split of the
// class groups).  W_c is staged through LDS as [row][k], pitch 16 KB + 2 (rows on the lanes: banks all distinct, see
// class_points_kernel.hip), the next stage's global loads in flight during the MFMAs: 4 classes per stage up to K = 32, one
// class per stage above (34 KB of LDS at most).  Per class A[i][k] = W_c[i][k], B[k][j] = (z_j - mu_c)[k], the 16 x 16
// blocks of W_c above the diagonal skipped: register `reg` of row block rb in lane (j, q) is y[16 rb + acc_row(q, reg)][j].
// Sample tails, class tails and K not a multiple of 4 or 16 are exact zeros in registers / LDS; no address past a tensor's
// end is formed.
#pragma once
#include <hip/hip_runtime.h>
#include <stdio.h>

#include <climits>
#include <type_traits>

#include "../../include/sqfa_hip.h"
#include "class_pair_loss.hpp"   // dtype_bytes, set_last_error
#include "proj_traits.hpp"

namespace sqfa {

constexpr int GW_THREADS = 256;
constexpr int GW_ROWS = 64;         // samples per workgroup
constexpr int GW_KMAX = 64;
constexpr int GW_MAX_SPLIT = 16;    // class splits at most
constexpr int GW_TARGET_WG = 1024;  // workgroups asked for (four per CU) before the classes stop being split

template <typename T> __device__ __forceinline__ T gw_shfl_xor(T v, int mask) { return __shfl_xor(v, mask, 64); }

// the class groups g_lo .. g_hi - 1 that whiten_class_split (below) gives split `split`, and the end of their classes
struct WhitenClassRange {
  int g_lo, g_hi, c_end;   // the classes 4 g_lo .. c_end - 1
};
__device__ __forceinline__ WhitenClassRange whiten_class_range(int C, int groups_per_split, int split) {
  const int n_groups = (C + 3) / 4;
  const int g_lo = split * groups_per_split;
  const int g_hi = g_lo + groups_per_split < n_groups ? g_lo + groups_per_split : n_groups;
  return {g_lo, g_hi, 4 * g_hi < C ? 4 * g_hi : C};
}

// ---- the stage: CS classes from cb on, W through registers into LDS as [class][row][k]; rows and columns K.. stay zero.
// One per thread, built once with the end of the workgroup's classes; the kernel calls zero() once, then per stage
// barrier, store(), barrier, load() of the next stage, whose global loads are in flight during the MFMAs. ----------------

template <typename T, int KB> struct WhitenStage {
  static constexpr int CS = KB <= 2 ? 4 : 1;       // classes per stage
  static constexpr int KP = KB * 16;               // padded K
  static constexpr int PITCH = KP + 2;
  static constexpr int PER = CS * KB * KB;         // W values per thread and stage: CS K K <= CS KP KP = 256 PER
  static constexpr int W_ELEMS = CS * KP * PITCH;  // of sW
  static constexpr int MU_ELEMS = CS * KP;         // of sMu
  T wv[PER], mv = T(0);
  const int c_end, K, tid;   // the workgroup's classes end at c_end - 1
  const int kk;              // K K
  const size_t w_end;        // the end of those classes in W; both formed once, not per load

  __device__ __forceinline__ WhitenStage(int c_end, int K, int tid)
      : c_end(c_end), K(K), tid(tid), kk(K * K), w_end((size_t)c_end * kk) {}
  __device__ __forceinline__ void zero(T* sW) const {
    for (int i = tid; i < W_ELEMS; i += GW_THREADS) sW[i] = T(0);
  }
  // the classes cb .. cb + CS - 1 below c_end, global memory to registers
  template <bool MEANS> __device__ __forceinline__ void load(const T* __restrict__ W, const T* __restrict__ mu, int cb) {
    const size_t base = (size_t)cb * kk;
#pragma unroll
    for (int e = 0; e < PER; ++e) {
      const int idx = tid + e * GW_THREADS;
      const bool ok = idx < CS * kk && base + idx < w_end;
      const T v = W[ok ? base + idx : 0];
      wv[e] = ok ? v : T(0);
    }
    if constexpr (MEANS) {
      const int cls = tid / KP, k = tid % KP;
      const bool ok = tid < CS * KP && cb + cls < c_end && k < K;
      const T v = mu[ok ? (size_t)(cb + cls) * K + k : 0];
      mv = ok ? v : T(0);
    }
  }
  // registers to LDS (between two barriers of the caller)
  template <bool MEANS> __device__ __forceinline__ void store(T* sW, T* sMu) const {
    const int kk = K * K;   // formed here, not read from the member: the index arithmetic below then stays out of the class loop
#pragma unroll
    for (int e = 0; e < PER; ++e) {
      const int idx = tid + e * GW_THREADS;
      if (idx < CS * kk) {
        const int cls = idx / kk, rem = idx % kk;
        sW[cls * KP * PITCH + (rem / K) * PITCH + rem % K] = wv[e];
      }
    }
    if constexpr (MEANS) {
      if (tid < CS * KP) sMu[tid] = mv;
    }
  }
};

// ---- the product ------------------------------------------------------------------------------------------------------------

// this lane's sample: z[s] = Z[n][4 s + q], zeros past K and past N
template <typename T, int KB>
__device__ __forceinline__ void whiten_load_sample(T (&z)[4 * KB], const T* __restrict__ Z, long long n, long long N, int K,
                                                   int q) {
#pragma unroll
  for (int s = 0; s < 4 * KB; ++s) {
    const int k = 4 * s + q;
    const bool ok = n < N && k < K;
    const T v = Z[ok ? (size_t)n * K + k : 0];
    z[s] = ok ? v : T(0);
  }
}

// the centred differences b[s] = z[s] - m[4 s + q] (m: the class's mean in LDS, zeros from K on)
template <typename T, int KB, bool MEANS>
__device__ __forceinline__ void whiten_center(T (&b)[4 * KB], const T (&z)[4 * KB], const T* m, int K4, int q) {
#pragma unroll
  for (int s = 0; s < 4 * KB; ++s) {
    if constexpr (MEANS) b[s] = s < K4 ? z[s] - m[4 * s + q] : T(0);
    else b[s] = z[s];
  }
}

// acc += row block rb of y = W b, W in LDS with pitch PITCH; the blocks above the diagonal of W are zero: skipped
template <typename T, int KB>
__device__ __forceinline__ void whiten_row_block(typename ProjTraits<T>::Acc& acc, int rb, const T* w, const T (&b)[4 * KB],
                                                 int K4, int j, int q) {
  constexpr int PITCH = WhitenStage<T, KB>::PITCH;
#pragma unroll
  for (int s = 0; s < 4 * (rb + 1); ++s)
    if (s < K4) acc = ProjTraits<T>::mfma(w[(rb * 16 + j) * PITCH + 4 * s + q], b[s], acc);
}

// every row block of y (zeros from K on), and the lane's partial of |y|^2 in THE order: row blocks ascending, the 4
// registers of a block ascending, one running sum
template <typename T, int KB>
__device__ __forceinline__ T whiten_product(typename ProjTraits<T>::Acc (&y)[KB], const T* w, const T (&b)[4 * KB], int K,
                                            int K4, int j, int q) {
  T sq = T(0);
#pragma unroll
  for (int rb = 0; rb < KB; ++rb) {
    y[rb] = typename ProjTraits<T>::Acc{};
    if (rb * 16 < K) {
      whiten_row_block<T, KB>(y[rb], rb, w, b, K4, j, q);
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) sq += y[rb][reg] * y[rb][reg];
    }
  }
  return sq;
}

// the same partial where y itself is not kept
template <typename T, int KB>
__device__ __forceinline__ T whiten_sq_partial(const T* w, const T (&b)[4 * KB], int K, int K4, int j, int q) {
  typename ProjTraits<T>::Acc y[KB];
  return whiten_product<T, KB>(y, w, b, K, K4, j, q);
}

// The two reductions of the partials over the 4 lane quarters.  Both form (p_q + p_{q^2}) + (p_{q^1} + p_{q^3}) in lane
// quarter q (xor 32 flips bit 1 of q, xor 16 bit 0), and a + b commutes bit for bit: every quarter of the butterfly, and the
// one quarter that the transpose leaves a class in, hold the same bits.
//   the butterfly: one class, its sum in all 4 quarters
template <typename T> __device__ __forceinline__ T whiten_quarters_sum(T sq) {
  sq += gw_shfl_xor(sq, 32);
  sq += gw_shfl_xor(sq, 16);
  return sq;
}
//   reduce and transpose: 4 classes in 3 cross-lane moves, lane (j, q) ends with the sum of class q
template <typename T> __device__ __forceinline__ T whiten_quarters_transpose(const T (&part)[4], int q) {
  const bool hi = (q & 2) != 0, odd = (q & 1) != 0;
  const T r0 = gw_shfl_xor(hi ? part[0] : part[2], 32), r1 = gw_shfl_xor(hi ? part[1] : part[3], 32);
  const T a0 = (hi ? part[2] : part[0]) + r0, a1 = (hi ? part[3] : part[1]) + r1;
  return (odd ? a1 : a0) + gw_shfl_xor(odd ? a0 : a1, 16);
}

// ---- host -------------------------------------------------------------------------------------------------------------------

// The class-split policy of the sample-owned passes: the groups of 4 classes are split over up to 16 workgroups per sample
// tile while fewer than 1024 workgroups are there, no split empty.  false: sizes or dtype outside the kernels' range, or more
// than 2^31 - 1 sample tiles or classes.
inline bool whiten_class_split(long long N, int C, int K, int dtype, int* groups_per_split, int* splits_out) {
  if (N < 1 || C < 1 || K < 1 || K > GW_KMAX || (dtype != SQFA_F32 && dtype != SQFA_F64)) return false;
  const long long tiles = (N + GW_ROWS - 1) / GW_ROWS;
  if (tiles > (long long)INT_MAX || C > INT_MAX - 3) return false;
  const int groups = (C + 3) / 4;
  long long splits = (GW_TARGET_WG + tiles - 1) / tiles;
  if (splits > GW_MAX_SPLIT) splits = GW_MAX_SPLIT;
  if (splits > groups) splits = groups;
  if (splits < 1) splits = 1;
  const int per = (int)((groups + splits - 1) / splits);
  *groups_per_split = per;
  *splits_out = (groups + per - 1) / per;
  return true;
}

// f(std::integral_constant<int, KB>, std::bool_constant<MEANS>) with KB = ceil(K / 16) in 1 .. 4
template <typename F> inline void dispatch_kb(int K, bool means, F&& f) {
  auto with = [&](auto kb) {
    if (means) f(kb, std::true_type{});
    else f(kb, std::false_type{});
  };
  const int KB = (K + 15) / 16;
  if (KB == 1) with(std::integral_constant<int, 1>{});
  else if (KB == 2) with(std::integral_constant<int, 2>{});
  else if (KB == 3) with(std::integral_constant<int, 3>{});
  else with(std::integral_constant<int, 4>{});
}

// The argument checks of sqfa_gauss_class_factors, sqfa_gauss_scores, sqfa_gauss_log_loss and sqfa_gauss_log_loss_backward,
// in their order (as check_pair_loss_args): null pointers / sizes < 1 (`nulls_text` is the entry point's list of them),
// dtype, the entry point's own check (`own_error`: nullptr where it passes, else the text), K > 64, the layout (`need`
// bytes, 0 where it has none for these sizes), the workspace against <entry>_workspace_bytes.  An entry point without a
// workspace passes has_workspace = false and the checks end after K > 64.  SQFA_OK or the code to return;
// sqfa_hip_last_error() is cleared first.
inline int check_gauss_args(const char* entry, bool nulls, const char* nulls_text, int dtype, const char* own_error, int K,
                            bool has_workspace, size_t need, const void* workspace, size_t workspace_bytes) {
  auto fail = [&](int rc, const char* what, const char* rest = "") {
    char text[256];
    snprintf(text, sizeof(text), "%s: %s%s", entry, what, rest);
    set_last_error(text);
    return rc;
  };
  set_last_error("");
  if (nulls) return fail(SQFA_ERR_BAD_ARGUMENT, nulls_text);
  if (dtype != SQFA_F32 && dtype != SQFA_F64) return fail(SQFA_ERR_BAD_ARGUMENT, "dtype");
  if (own_error != nullptr) return fail(SQFA_ERR_BAD_ARGUMENT, own_error);
  if (K > GW_KMAX) return fail(SQFA_ERR_UNSUPPORTED_M, "K > 64");
  if (!has_workspace) return SQFA_OK;
  if (need == 0) return fail(SQFA_ERR_UNSUPPORTED_M, "more than 2^31 - 1 sample tiles or classes");
  if (workspace == nullptr || workspace_bytes < need) {
    char query[96];
    snprintf(query, sizeof(query), "%s_workspace_bytes", entry);
    return fail(SQFA_ERR_WORKSPACE, "workspace is null or smaller than ", query);
  }
  return SQFA_OK;
}

}  // namespace sqfa
