// gauss_topk_kernel.hip -- the k best classes of every sample, and the rank of its labelled class, from the Gaussian class
// scores of gauss_scores_kernel.hip without the (N, C) matrix.  Written on gauss_whiten.hpp alone: the geometry, the stage of
// W_c, the product y = W_c (z - mu_c), the order of its squares, the quarter reductions and the class splits are the
// scorer's, and a score is formed by the scorer's own statement T(-0.5) * tot + off with off = (T)offset[c], a padded class
// -inf by select: every score below has the bits sqfa_gauss_scores writes into scores_out (DESIGN Q4).
//
// The total order of (score, class): higher score first, equal scores: lower class index first.  No two distinct classes
// tie under it, so "the k first" and "how many come before the label" have one answer each.
//
// Launches (caller's stream; nothing allocated, synchronised or read back; no float atomics; every grid a function of
// (N, C, K, dtype, k) alone; bitwise reproducible, whichever optional outputs are asked for):
//   gauss_topk_kernel         the scorer's loop; every lane carries a list of KT (score, class) entries sorted by the order
//                             (KT the smallest of 1, 2, 4, 8 that is >= k; empty slots (-inf, INT_MAX)), a new score enters
//                             by compare-and-select insertion, the four lane quarters merge by a butterfly of list merges.
//   gauss_topk_merge_kernel   only where the classes are split: joins the (splits, N, KT) partial lists in split order.
//   gauss_label_score_kernel  t_n = score[n][y_n] with the scorer's bits: a one-wave workgroup takes its 16 samples in turn,
//                             stages W and mu of the sample's labelled class and runs the product on all 16 columns (column j
//                             of an MFMA product depends on column j of B alone); lane j = i keeps the result.
//   gauss_rank_kernel         the scorer's loop; every lane counts the classes c != y_n that come before (t_n, y_n).
//   gauss_rank_merge_kernel   only where the classes are split: integer sums of the (splits, N) partial counts.
// Labels are data: a label is range-checked before anything is addressed with it; an out-of-range label gathers class 0.
#include <hip/hip_runtime.h>

#include <climits>

#include "../../include/sqfa_hip.h"
#include "class_pair_loss.hpp"   // namespace math, dispatch_dtype, WorkspaceCursor
#include "gauss_whiten.hpp"

namespace sqfa {

constexpr int GT_KMAX = 8;        // list entries at most
constexpr int GT_LABEL_ROWS = 16; // samples of a gauss_label_score_kernel workgroup (one wave)

// ---- the scorer's loop --------------------------------------------------------------------------------------------------------

template <typename T> struct GtClasses {
  const T* Z;
  long long N;
  const T* mu;
  const T* W;
  const double* offset;
  int C, K;
  int groups_per_split, splits;   // groups of 4 classes
};

// take(score, c) for every class c < C of split blockIdx.y, in lane (j, q) for the classes 4 g + q, in ascending order
template <typename T, int KB, bool MEANS, typename F>
__device__ __forceinline__ void gt_for_each_score(const GtClasses<T>& p, const T (&z)[4 * KB], T* sW, T* sMu, F&& take) {
  using Stage = WhitenStage<T, KB>;
  constexpr int CS = Stage::CS, KP = Stage::KP, PITCH = Stage::PITCH;
  const int tid = threadIdx.x, l = tid & 63, q = l >> 4, j = l & 15;
  const int K = p.K, C = p.C, K4 = (K + 3) / 4;
  const auto [g_lo, g_hi, c_end] = whiten_class_range(C, p.groups_per_split, blockIdx.y);

  Stage stage(c_end, K, tid);
  stage.zero(sW);
  if (g_lo < g_hi) stage.template load<MEANS>(p.W, p.mu, 4 * g_lo);

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
    if (c_mine < C) take(sc, c_mine);
  }
}

// (a, ca) comes before (b, cb)
template <typename T> __device__ __forceinline__ bool gt_before(T a, int ca, T b, int cb) {
  return a > b || (a == b && ca < cb);
}

// ---- top-k --------------------------------------------------------------------------------------------------------------------

// KT (score, class) entries sorted by the order; a NaN score never enters (the sample is flagged instead)
template <typename T, int KT> struct GtList {
  T s[KT];
  int c[KT];
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int i = 0; i < KT; ++i) {
      s[i] = math::neg_inf<T>();
      c[i] = INT_MAX;
    }
  }
  // compare and select down the list: the entry that comes later moves on to the next slot, the last one drops out
  __device__ __forceinline__ void insert(T v, int cls) {
#pragma unroll
    for (int i = 0; i < KT; ++i) {
      const bool in = gt_before(v, cls, s[i], c[i]);
      const T vs = in ? s[i] : v;
      const int vc = in ? c[i] : cls;
      s[i] = in ? v : s[i];
      c[i] = in ? cls : c[i];
      v = vs;
      cls = vc;
    }
  }
};

template <typename T> struct GtTopkParams {
  GtClasses<T> cls;
  int k;
  long long* index;   // (N, k)
  T* score;           // (N, k) or nullptr
  int* nonfinite;
  // (splits, N, KT) each, splits > 1 only; p_idx[.][.][0] = -1: the sample's row holds a NaN
  T* p_score;
  int* p_idx;
};

template <typename T, int KT>
__device__ __forceinline__ void gt_write_topk(const GtTopkParams<T>& p, long long n, const GtList<T, KT>& list, bool nan) {
#pragma unroll
  for (int i = 0; i < KT; ++i) {
    if (i < p.k) {
      p.index[(size_t)n * p.k + i] = nan ? -1 : list.c[i];
      if (p.score != nullptr) p.score[(size_t)n * p.k + i] = nan ? math::nan<T>() : list.s[i];
    }
  }
}

template <typename T, int KB, bool MEANS, int KT>
__global__ __launch_bounds__(GW_THREADS) void gauss_topk_kernel(const GtTopkParams<T> p) {
  using Stage = WhitenStage<T, KB>;
  __shared__ T sW[Stage::W_ELEMS];
  __shared__ T sMu[Stage::MU_ELEMS];
  const int tid = threadIdx.x, l = tid & 63, wave = tid >> 6, q = l >> 4, j = l & 15;
  const long long N = p.cls.N;
  const long long n = (long long)blockIdx.x * GW_ROWS + wave * 16 + j;

  T z[4 * KB];
  whiten_load_sample<T, KB>(z, p.cls.Z, n, N, p.cls.K, q);

  GtList<T, KT> list;
  list.clear();
  bool nan = false;
  gt_for_each_score<T, KB, MEANS>(p.cls, z, sW, sMu, [&](T sc, int c) {
    if (sc != sc) nan = true;
    list.insert(sc, c);
  });

  // merge the quarters: a butterfly of list merges; the order has no ties between distinct classes, so both partners end
  // with the same KT entries in the same slots
#pragma unroll
  for (int mask = 16; mask <= 32; mask *= 2) {
    T os[KT];
    int oc[KT];
#pragma unroll
    for (int i = 0; i < KT; ++i) {
      os[i] = gw_shfl_xor(list.s[i], mask);
      oc[i] = __shfl_xor(list.c[i], mask, 64);
    }
#pragma unroll
    for (int i = 0; i < KT; ++i) list.insert(os[i], oc[i]);
    nan = nan || __shfl_xor(nan ? 1 : 0, mask, 64) != 0;
  }
  const bool writer = q == 0 && n < N;
  if (p.cls.splits > 1) {
    if (writer) {
      const size_t at = ((size_t)blockIdx.y * N + n) * KT;
#pragma unroll
      for (int i = 0; i < KT; ++i) {
        p.p_score[at + i] = list.s[i];
        p.p_idx[at + i] = nan && i == 0 ? -1 : list.c[i];
      }
    }
    return;
  }
  if (writer) gt_write_topk<T, KT>(p, n, list, nan);
  const unsigned long long bal = __ballot(writer && nan);
  if (l == 0 && bal != 0) atomicAdd(p.nonfinite, __popcll(bal));
}

// one thread per sample: the splits' partial lists in the order s = 0, 1, ...
template <typename T, int KT>
__global__ __launch_bounds__(GW_THREADS) void gauss_topk_merge_kernel(const GtTopkParams<T> p) {
  const long long N = p.cls.N;
  const long long n = (long long)blockIdx.x * GW_THREADS + threadIdx.x;
  bool nan = false;
  if (n < N) {
    GtList<T, KT> list;
    list.clear();
    for (int s = 0; s < p.cls.splits; ++s) {
      const size_t at = ((size_t)s * N + n) * KT;
      if (p.p_idx[at] < 0) nan = true;
#pragma unroll
      for (int i = 0; i < KT; ++i) list.insert(p.p_score[at + i], p.p_idx[at + i] < 0 ? INT_MAX : p.p_idx[at + i]);
    }
    gt_write_topk<T, KT>(p, n, list, nan);
  }
  const unsigned long long bal = __ballot(nan);
  if ((threadIdx.x & 63) == 0 && bal != 0) atomicAdd(p.nonfinite, __popcll(bal));
}

// ---- the label's rank -----------------------------------------------------------------------------------------------------------

template <typename T> struct GtRankParams {
  GtClasses<T> cls;
  const long long* labels;
  T* t;               // (N) workspace: score[n][y_n], NaN for a label outside [0, C)
  T* label_score;     // (N) or nullptr: a copy of t
  long long* rank;    // (N)
  int* flags;         // (2): NaN rows, labels outside [0, C)
  int* p_cnt;         // (splits, N), splits > 1 only; -1: the sample's row holds a NaN
};

// One wave, 16 samples.  For sample i in turn the labelled class's W and mu are staged in the layout of WhitenStage (one
// class: [row][k], pitch KP + 2, zeros from K on) and the product, its squares and the quarter sum are the scorer's on all 16
// columns; column i is sample i against its own class.
template <typename T, int KB, bool MEANS>
__global__ __launch_bounds__(64) void gauss_label_score_kernel(const GtRankParams<T> p) {
  constexpr int KP = KB * 16, PITCH = WhitenStage<T, KB>::PITCH;
  __shared__ T sW[KP * PITCH];
  __shared__ T sMu[KP];
  const int l = threadIdx.x, q = l >> 4, j = l & 15;
  const int K = p.cls.K, C = p.cls.C, K4 = (K + 3) / 4, kk = K * K;
  const long long N = p.cls.N;
  const long long n0 = (long long)blockIdx.x * GT_LABEL_ROWS, n = n0 + j;

  T z[4 * KB];
  whiten_load_sample<T, KB>(z, p.cls.Z, n, N, K, q);
  for (int i = l; i < KP * PITCH; i += 64) sW[i] = T(0);
  if (l < KP) sMu[l] = T(0);

  T keep = math::nan<T>();
#pragma unroll 1
  for (int i = 0; i < GT_LABEL_ROWS; ++i) {
    if (n0 + i >= N) break;   // uniform
    const long long y = p.labels[n0 + i];
    const bool inside = y >= 0 && y < C;
    const int c = inside ? (int)y : 0;
    __syncthreads();   // the previous class has been consumed (first pass: the zero fill is done)
    for (int idx = l; idx < kk; idx += 64) sW[(idx / K) * PITCH + idx % K] = p.cls.W[(size_t)c * kk + idx];
    if constexpr (MEANS) {
      if (l < K) sMu[l] = p.cls.mu[(size_t)c * K + l];
    }
    __syncthreads();
    T b[4 * KB];
    whiten_center<T, KB, MEANS>(b, z, sMu, K4, q);
    const T tot = whiten_quarters_sum(whiten_sq_partial<T, KB>(sW, b, K, K4, j, q));
    const T off = (T)p.cls.offset[c];
    const T sc = T(-0.5) * tot + off;
    if (j == i) keep = inside ? sc : math::nan<T>();
  }
  const bool writer = q == 0 && n < N;
  bool outside = false;
  if (writer) {
    const long long y = p.labels[n];
    outside = !(y >= 0 && y < C);
    p.t[n] = keep;
    if (p.label_score != nullptr) p.label_score[n] = keep;
  }
  const unsigned long long bal = __ballot(outside);
  if (l == 0 && bal != 0) atomicAdd(p.flags + 1, __popcll(bal));
}

template <typename T, int KB, bool MEANS>
__global__ __launch_bounds__(GW_THREADS) void gauss_rank_kernel(const GtRankParams<T> p) {
  using Stage = WhitenStage<T, KB>;
  __shared__ T sW[Stage::W_ELEMS];
  __shared__ T sMu[Stage::MU_ELEMS];
  const int tid = threadIdx.x, l = tid & 63, wave = tid >> 6, q = l >> 4, j = l & 15;
  const long long N = p.cls.N;
  const long long n = (long long)blockIdx.x * GW_ROWS + wave * 16 + j;

  T z[4 * KB];
  whiten_load_sample<T, KB>(z, p.cls.Z, n, N, p.cls.K, q);
  const long long y = n < N ? p.labels[n] : 0;
  const bool inside = y >= 0 && y < p.cls.C;
  const int yc = inside ? (int)y : -1;
  const T t = n < N ? p.t[n] : T(0);

  int cnt = 0;
  bool nan = false;
  gt_for_each_score<T, KB, MEANS>(p.cls, z, sW, sMu, [&](T sc, int c) {
    if (sc != sc) nan = true;
    if (c != yc && gt_before(sc, c, t, yc)) ++cnt;
  });

#pragma unroll
  for (int mask = 16; mask <= 32; mask *= 2) {
    cnt += __shfl_xor(cnt, mask, 64);
    nan = nan || __shfl_xor(nan ? 1 : 0, mask, 64) != 0;
  }
  const bool writer = q == 0 && n < N;
  if (p.cls.splits > 1) {
    if (writer) p.p_cnt[(size_t)blockIdx.y * N + n] = nan ? -1 : cnt;
    return;
  }
  if (writer) p.rank[n] = nan || !inside ? -1 : cnt;
  const unsigned long long bal = __ballot(writer && nan);
  if (l == 0 && bal != 0) atomicAdd(p.flags, __popcll(bal));
}

template <typename T>
__global__ __launch_bounds__(GW_THREADS) void gauss_rank_merge_kernel(const GtRankParams<T> p) {
  const long long N = p.cls.N;
  const long long n = (long long)blockIdx.x * GW_THREADS + threadIdx.x;
  bool nan = false;
  if (n < N) {
    long long cnt = 0;
    for (int s = 0; s < p.cls.splits; ++s) {
      const int part = p.p_cnt[(size_t)s * N + n];
      if (part < 0) nan = true;
      cnt += part;
    }
    const long long y = p.labels[n];
    const bool inside = y >= 0 && y < p.cls.C;
    p.rank[n] = nan || !inside ? -1 : cnt;
  }
  const unsigned long long bal = __ballot(nan);
  if ((threadIdx.x & 63) == 0 && bal != 0) atomicAdd(p.flags, __popcll(bal));
}

// ---- host ---------------------------------------------------------------------------------------------------------------------

static int gt_list_size(int k) { return k <= 1 ? 1 : k <= 2 ? 2 : k <= 4 ? 4 : GT_KMAX; }
static bool gt_k_ok(int k, int C) { return k >= 1 && k <= GT_KMAX && k <= C; }

// f(std::integral_constant<int, KT>) with KT = gt_list_size(k)
template <typename F> static void dispatch_kt(int k, F&& f) {
  const int KT = gt_list_size(k);
  if (KT == 1) f(std::integral_constant<int, 1>{});
  else if (KT == 2) f(std::integral_constant<int, 2>{});
  else if (KT == 4) f(std::integral_constant<int, 4>{});
  else f(std::integral_constant<int, GT_KMAX>{});
}

struct GtTopkLayout {
  int groups_per_split, splits;
  size_t off_score, off_idx, total;   // splits > 1: two (splits, N, KT) arrays [score T][idx int]
};

static bool gt_topk_layout(long long N, int C, int K, int dtype, int k, GtTopkLayout* w) {
  if (!gt_k_ok(k, C) || !whiten_class_split(N, C, K, dtype, &w->groups_per_split, &w->splits)) return false;
  const size_t cells = w->splits > 1 ? (size_t)w->splits * (size_t)N * (size_t)gt_list_size(k) : 0;
  WorkspaceCursor ws{1};
  w->off_score = ws.take(cells * dtype_bytes(dtype));
  w->off_idx = ws.take(cells * sizeof(int));
  w->total = ws.at < 16 ? 16 : ws.at;
  return true;
}

struct GtRankLayout {
  int groups_per_split, splits;
  size_t off_t, off_cnt, total;   // [t (N) T][splits > 1: cnt (splits, N) int]
};

static bool gt_rank_layout(long long N, int C, int K, int dtype, GtRankLayout* w) {
  if (!whiten_class_split(N, C, K, dtype, &w->groups_per_split, &w->splits)) return false;
  if ((N + GT_LABEL_ROWS - 1) / GT_LABEL_ROWS > (long long)INT_MAX) return false;   // the grid of the label pass
  WorkspaceCursor ws{1};
  w->off_t = ws.take((size_t)N * 8);   // 8 bytes per sample for either dtype: cnt stays aligned
  w->off_cnt = ws.take(w->splits > 1 ? (size_t)w->splits * (size_t)N * sizeof(int) : 0);
  w->total = ws.at < 16 ? 16 : ws.at;
  return true;
}

template <typename T>
static GtClasses<T> gt_classes(const void* Z, long long N, const void* mu, const void* W, const double* offset, int C, int K,
                               int groups_per_split, int splits) {
  GtClasses<T> c{};
  c.Z = static_cast<const T*>(Z);
  c.N = N;
  c.mu = static_cast<const T*>(mu);
  c.W = static_cast<const T*>(W);
  c.offset = offset;
  c.C = C;
  c.K = K;
  c.groups_per_split = groups_per_split;
  c.splits = splits;
  return c;
}

// One object per (element type, list size) holds the variants of gauss_topk_kernel (the Makefile compiles this file with
// -DSQFA_GT_SLICE_T=<type> -DSQFA_GT_SLICE_KT=<KT> for them, in parallel); the object without the macros holds the rank
// kernels and the entry points.
template <typename T, int KT>
hipError_t run_topk(const void* Z, long long N, const void* mu, const void* W, const double* offset, int C, int K, int k,
                    long long* index, void* score, int* nonfinite, char* ws, const GtTopkLayout& lay, hipStream_t stream) {
  GtTopkParams<T> p{};
  p.cls = gt_classes<T>(Z, N, mu, W, offset, C, K, lay.groups_per_split, lay.splits);
  p.k = k;
  p.index = index;
  p.score = static_cast<T*>(score);
  p.nonfinite = nonfinite;
  if (lay.splits > 1) {
    p.p_score = reinterpret_cast<T*>(ws + lay.off_score);
    p.p_idx = reinterpret_cast<int*>(ws + lay.off_idx);
  }
  hipError_t e = hipMemsetAsync(nonfinite, 0, sizeof(int), stream);
  if (e != hipSuccess) return e;
  const dim3 grid((unsigned)((N + GW_ROWS - 1) / GW_ROWS), (unsigned)lay.splits);
  dispatch_kb(K, mu != nullptr, [&](auto kb, auto means) {
    hipLaunchKernelGGL((gauss_topk_kernel<T, decltype(kb)::value, decltype(means)::value, KT>), grid, dim3(GW_THREADS), 0,
                       stream, p);
  });
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (lay.splits > 1) {
    hipLaunchKernelGGL((gauss_topk_merge_kernel<T, KT>), dim3((unsigned)((N + GW_THREADS - 1) / GW_THREADS)),
                       dim3(GW_THREADS), 0, stream, p);
    e = hipGetLastError();
  }
  return e;
}

#define SQFA_GT_RUN_TOPK(T, KT)                                                                                             \
  template hipError_t run_topk<T, KT>(const void*, long long, const void*, const void*, const double*, int, int, int,      \
                                      long long*, void*, int*, char*, const GtTopkLayout&, hipStream_t)
#ifdef SQFA_GT_SLICE_T
SQFA_GT_RUN_TOPK(SQFA_GT_SLICE_T, SQFA_GT_SLICE_KT);

}  // namespace sqfa
#else
extern SQFA_GT_RUN_TOPK(float, 1);
extern SQFA_GT_RUN_TOPK(float, 2);
extern SQFA_GT_RUN_TOPK(float, 4);
extern SQFA_GT_RUN_TOPK(float, 8);
extern SQFA_GT_RUN_TOPK(double, 1);
extern SQFA_GT_RUN_TOPK(double, 2);
extern SQFA_GT_RUN_TOPK(double, 4);
extern SQFA_GT_RUN_TOPK(double, 8);

template <typename T>
static hipError_t run_rank(const void* Z, const long long* labels, long long N, const void* mu, const void* W,
                           const double* offset, int C, int K, long long* rank, void* label_score, int* flags, char* ws,
                           const GtRankLayout& lay, hipStream_t stream) {
  GtRankParams<T> p{};
  p.cls = gt_classes<T>(Z, N, mu, W, offset, C, K, lay.groups_per_split, lay.splits);
  p.labels = labels;
  p.t = reinterpret_cast<T*>(ws + lay.off_t);
  p.label_score = static_cast<T*>(label_score);
  p.rank = rank;
  p.flags = flags;
  if (lay.splits > 1) p.p_cnt = reinterpret_cast<int*>(ws + lay.off_cnt);
  hipError_t e = hipMemsetAsync(flags, 0, 2 * sizeof(int), stream);
  if (e != hipSuccess) return e;
  const dim3 grid((unsigned)((N + GW_ROWS - 1) / GW_ROWS), (unsigned)lay.splits);
  dispatch_kb(K, mu != nullptr, [&](auto kb, auto means) {
    constexpr int KB = decltype(kb)::value;
    constexpr bool MEANS = decltype(means)::value;
    hipLaunchKernelGGL((gauss_label_score_kernel<T, KB, MEANS>), dim3((unsigned)((N + GT_LABEL_ROWS - 1) / GT_LABEL_ROWS)),
                       dim3(64), 0, stream, p);
    if (hipPeekAtLastError() == hipSuccess)
      hipLaunchKernelGGL((gauss_rank_kernel<T, KB, MEANS>), grid, dim3(GW_THREADS), 0, stream, p);
  });
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (lay.splits > 1) {
    hipLaunchKernelGGL((gauss_rank_merge_kernel<T>), dim3((unsigned)((N + GW_THREADS - 1) / GW_THREADS)), dim3(GW_THREADS), 0,
                       stream, p);
    e = hipGetLastError();
  }
  return e;
}

}  // namespace sqfa

using namespace sqfa;

extern "C" size_t sqfa_gauss_scores_topk_workspace_bytes(long long N, int C, int K, int dtype, int k) {
  GtTopkLayout w;
  return gt_topk_layout(N, C, K, dtype, k, &w) ? w.total : 0;
}

extern "C" int sqfa_gauss_scores_topk(const void* Z, long long N, const void* means, const void* W, const double* offset,
                                      int C, int K, int dtype, int k, long long* index_out, void* score_out,
                                      int* nonfinite_out, void* workspace, size_t workspace_bytes, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  GtTopkLayout lay;
  const size_t need = gt_topk_layout(N, C, K, dtype, k, &lay) ? lay.total : 0;
  const bool nulls = Z == nullptr || W == nullptr || offset == nullptr || index_out == nullptr || nonfinite_out == nullptr ||
                     N < 1 || C < 1 || K < 1;
  const int rc = check_gauss_args("sqfa_gauss_scores_topk", nulls,
                                  "null samples, factors, offsets, indices or counter, N < 1, C < 1 or K < 1", dtype,
                                  gt_k_ok(k, C) ? nullptr : "k outside [1, min(8, C)]", K, true, need, workspace,
                                  workspace_bytes);
  if (rc != SQFA_OK) return rc;
  hipError_t e = hipSuccess;
  dispatch_dtype(dtype, [&](auto t) {
    dispatch_kt(k, [&](auto kt) {
      e = run_topk<decltype(t), decltype(kt)::value>(Z, N, means, W, offset, C, K, k, index_out, score_out, nonfinite_out,
                                                     static_cast<char*>(workspace), lay, stream);
    });
  });
  return e == hipSuccess ? SQFA_OK : SQFA_ERR_LAUNCH;
}

extern "C" size_t sqfa_gauss_label_rank_workspace_bytes(long long N, int C, int K, int dtype) {
  GtRankLayout w;
  return gt_rank_layout(N, C, K, dtype, &w) ? w.total : 0;
}

extern "C" int sqfa_gauss_label_rank(const void* Z, const long long* labels, long long N, const void* means, const void* W,
                                     const double* offset, int C, int K, int dtype, long long* rank_out,
                                     void* label_score_out, int* flags_out, void* workspace, size_t workspace_bytes,
                                     void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  GtRankLayout lay;
  const size_t need = gt_rank_layout(N, C, K, dtype, &lay) ? lay.total : 0;
  const bool nulls = Z == nullptr || labels == nullptr || W == nullptr || offset == nullptr || rank_out == nullptr ||
                     flags_out == nullptr || N < 1 || C < 1 || K < 1;
  const int rc = check_gauss_args("sqfa_gauss_label_rank", nulls,
                                  "null samples, labels, factors, offsets, ranks or flags, N < 1, C < 1 or K < 1", dtype, nullptr,
                                  K, true, need, workspace, workspace_bytes);
  if (rc != SQFA_OK) return rc;
  const hipError_t e = dispatch_dtype(dtype, [&](auto t) {
    return run_rank<decltype(t)>(Z, labels, N, means, W, offset, C, K, rank_out, label_score_out, flags_out,
                                 static_cast<char*>(workspace), lay, stream);
  });
  return e == hipSuccess ? SQFA_OK : SQFA_ERR_LAUNCH;
}
#endif   // SQFA_GT_SLICE_T
