// log_euclidean_kernel.hip -- fused closure loss of the log-Euclidean distances (reference: src/sqfa/distances.py:92-138 as
// the distance_fun of SecondMomentsSQFA): for the n class logarithms L_c = log S_c
//     d2_ij = || L_i - L_j ||_F^2,   D_ij = d2_ij  |  sqrt(d2_ij + eps),   loss = w sum_{i>j} D_ij
//     G_i = d loss / d L_i = sum_{j != i} c_ij (L_i - L_j),   c_ij = 2 w  |  w / D_ij
// in ONE pass over the ordered pairs (an N-body pass over n vectors of m(m+1)/2 entries).  The logarithms come from the
// per-class stages of sqfa_spd_function, and G goes back to S through sqfa_spd_function_backward (sqfa_api.hip).
//
// Mapping: a 256-thread workgroup owns TI classes i; every class has NS lane groups of G lanes (TI NS G = 256, a group never
// leaves its wave).  Lane l of a group keeps E entries of the lower triangle of L_i in registers -- slots e < ED hold diagonal
// entries, the others strictly-lower ones, entry e G + l of each kind -- and E accumulators of G_i.  The logarithms of all j
// stream through LDS in tiles of TJ classes (same slot layout, zero padded, so the inner loop has no bounds checks); group s
// of a class takes the rows s, s + NS, ... of each tile.  Groups of different classes that share s read the same LDS
// addresses (broadcast), and a group's lanes read consecutive addresses: no bank conflicts inside a 32-lane half.
// Per pair: diff = L_i - L_j entry by entry (explicit differences: exact for close classes, where the Gram form
// |a|^2 + |b|^2 - 2ab and the form L_i sum(c) - sum(c L_j) of the gradient cancel the digits that matter),
// d2 = sum diag^2 + 2 sum lower^2 over the group (DPP / row-swap butterfly, group_sum of pair_kernel.hpp), then
// acc += c diff.  The pair i == j is skipped.  At the end the NS groups of a class are combined through LDS in the order
// s = 0, 1, ...: one writer per G_i, no atomics, bitwise reproducible.
// Weighted variant (template parameter WEIGHTED, sqfa_log_euclidean_pairwise_loss_weighted with a weight matrix): w becomes
// w_ij = W[i n + j].  The TI x TJ block of W that a tile needs travels with the tile -- gathered to registers while the
// previous tile is consumed (coalesced along j), stored to LDS between the same two barriers -- so the pair loop reads its
// weight from LDS next to the row of L_j and holds no global load.  Row i weighs every ordered pair (i, j) with its own
// w_ij and class j weighs the same pair with w_ji: W must be symmetric.
#include <hip/hip_runtime.h>

#include "../../include/sqfa_hip.h"
#include "class_pair_loss.hpp"
#include "pair_kernel.hpp"   // group_sum

namespace sqfa {

struct LogEucParams : PairLossParams {
  const void* L;      // (n,m,m) class logarithms
  void* G;            // (n,m,m) d loss / d L, full symmetric matrices, or nullptr (forward only)
  int sqrt_mode;
};

// Geometry of one row of the table below: G lanes per group, matrices up to MMAX x MMAX.
template <typename T, int G_, int MMAX_>
struct LogEucCfg {
  static constexpr int G = G_, MMAX = MMAX_;
  static constexpr int ED = (MMAX + G - 1) / G;                     // slots of diagonal entries per lane
  static constexpr int EO = (MMAX * (MMAX - 1) / 2 + G - 1) / G;    // slots of strictly-lower entries per lane
  static constexpr int E = ED + EO;
  static constexpr int PITCH = G * E;                                // entries of one class in LDS
  static constexpr int GROUPS = 256 / G;
  static constexpr size_t ROW_BYTES = (size_t)PITCH * sizeof(T);
  // classes per workgroup: enough groups of different classes side by side to fill a 32-lane half (they broadcast), more
  // where NS rows of a tile would not fit in 40 KiB
  static constexpr int ti() {
    int t = G >= 64 ? 1 : (G >= 16 ? 2 : 32 / G);
    while ((GROUPS / t) * ROW_BYTES > 40 * 1024 && t < GROUPS) t *= 2;
    return t;
  }
  static constexpr int TI = ti();
  static constexpr int NS = GROUPS / TI;
  static constexpr int rounds() {   // rows per group and tile: up to 8 while the tile stays within 32 KiB
    int r = (int)((32 * 1024) / (NS * ROW_BYTES));
    return r < 1 ? 1 : (r > 8 ? 8 : r);
  }
  static constexpr int TJ = NS * rounds();
  static constexpr size_t TILE_BYTES = (size_t)TJ * ROW_BYTES;
  static constexpr size_t COMB_BYTES = (size_t)TI * (NS > 1 ? NS - 1 : 1) * ROW_BYTES;   // the combine buffer reuses the tile
  static constexpr size_t BUF_BYTES = TILE_BYTES > COMB_BYTES ? TILE_BYTES : COMB_BYTES;
  static_assert(TI * NS * G == 256, "lane groups must fill the workgroup");
  static constexpr size_t W_BYTES = (size_t)TI * TJ * sizeof(T);   // weighted variant: the tile's block of pair weights
  static_assert(BUF_BYTES + W_BYTES + PITCH * sizeof(int) + 2048 <= 64 * 1024, "LDS per workgroup stays within 64 KiB");
};

template <typename Cfg, typename T, bool WEIGHTED>
__global__ __launch_bounds__(256) void log_euclidean_pair_kernel(const LogEucParams p) {
  constexpr int G = Cfg::G, ED = Cfg::ED, E = Cfg::E, PITCH = Cfg::PITCH, TI = Cfg::TI, NS = Cfg::NS, TJ = Cfg::TJ;
  __shared__ __align__(16) unsigned char s_buf[Cfg::BUF_BYTES];
  __shared__ int s_map[PITCH];        // slot position -> offset of the entry inside an m x m matrix, -1: padding
  __shared__ double s_loss[TI][NS];
  __shared__ int s_cnt[TI][NS][2];
  __shared__ T s_w[WEIGHTED ? TI * TJ : 1];   // weights of the current tile: row ti, column jj
  T* tile = reinterpret_cast<T*>(s_buf);
  const int tid = threadIdx.x, n = p.n, m = p.m, mm = m * m;
  const int lane = tid % G, gid = tid / G, ti = gid % TI, s = gid / TI;
  const int i = blockIdx.x * TI + ti;
  const bool ivalid = i < n;
  const T* L = static_cast<const T*>(p.L);

  const int n_lower = m * (m - 1) / 2;
  for (int pos = tid; pos < PITCH; pos += 256) {
    int off = -1;
    if (pos < ED * G) {
      if (pos < m) off = pos * m + pos;
    } else if (pos - ED * G < n_lower) {
      const int k = pos - ED * G;   // k-th strictly-lower entry, row-major: (r, c), c < r, k = r (r - 1) / 2 + c
      int r = (int)((1.0f + sqrtf(1.0f + 8.0f * (float)k)) * 0.5f);
      while (r * (r - 1) / 2 > k) --r;
      while ((r + 1) * r / 2 <= k) ++r;
      off = r * m + (k - r * (r - 1) / 2);
    }
    s_map[pos] = off;
  }
  __syncthreads();

  T li[E], acc[E];
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const int off = s_map[e * G + lane];
    li[e] = (ivalid && off >= 0) ? L[(size_t)i * mm + off] : T(0);
    acc[e] = T(0);
  }
  const T w = pair_weight<T>(p), eps = pair_eps<T>(p);
  const bool sqrt_mode = p.sqrt_mode != 0;
  T* dist = static_cast<T*>(p.dist);
  double loss_acc = 0.0;
  int n_nan = 0, n_inf = 0;

  // A tile is gathered from global memory (L2) into registers -- LOADS independent loads per thread, issued back to back --
  // while the previous tile is being consumed, and moved to LDS between two barriers.
  constexpr int LOADS = (TJ * PITCH + 255) / 256;
  constexpr int WLOADS = WEIGHTED ? (TI * TJ + 255) / 256 : 1;
  T stage[LOADS], wstage[WLOADS];
  const T* W = static_cast<const T*>(p.W);
  auto gather = [&](int j0) {
    if constexpr (WEIGHTED) {
#pragma unroll
      for (int u = 0; u < WLOADS; ++u) {
        const int q = tid + u * 256;
        const int it = blockIdx.x * TI + q / TJ, j = j0 + q % TJ;
        const bool valid = q < TI * TJ && it < n && j < n;
        const T v = W[valid ? (size_t)it * n + j : 0];
        wstage[u] = valid ? v : T(0);
      }
    }
#pragma unroll
    for (int u = 0; u < LOADS; ++u) {
      const int q = tid + u * 256;
      const int jj = q / PITCH, off = s_map[q < TJ * PITCH ? q % PITCH : 0], j = j0 + jj;
      const bool valid = q < TJ * PITCH && off >= 0 && j < n;
      const T v = L[valid ? (size_t)j * mm + off : 0];   // always a valid address: no branch around the load
      stage[u] = valid ? v : T(0);
    }
  };
  gather(0);
  for (int j0 = 0; j0 < n; j0 += TJ) {
    __syncthreads();   // the previous tile has been consumed
#pragma unroll
    for (int u = 0; u < LOADS; ++u) {
      const int q = tid + u * 256;
      if (q < TJ * PITCH) tile[q] = stage[u];
    }
    if constexpr (WEIGHTED) {
#pragma unroll
      for (int u = 0; u < WLOADS; ++u) {
        const int q = tid + u * 256;
        if (q < TI * TJ) s_w[q] = wstage[u];
      }
    }
    __syncthreads();
    if (j0 + TJ < n) gather(j0 + TJ);   // the next tile's loads are in flight during this tile's pairs
#pragma unroll 1
    for (int jj = s; jj < TJ; jj += NS) {
      const int j = j0 + jj;
      const T* row = tile + jj * PITCH + lane;
      T wij = w;
      if constexpr (WEIGHTED) wij = s_w[ti * TJ + jj];
      T diff[E];
      T dd = T(0), od = T(0);
#pragma unroll
      for (int e = 0; e < E; ++e) {
        diff[e] = li[e] - row[e * G];
        if (e < ED) dd += diff[e] * diff[e];
        else od += diff[e] * diff[e];
      }
      const T d2 = group_sum<G>(dd + T(2) * od);   // every lane of the group gets the total
      if (ivalid && j < n && j != i) {
        T D, c;
        if (sqrt_mode) {
          D = math::sqrt(d2 + eps);
          c = wij / D;
        } else {
          D = d2;
          c = T(2) * wij;
        }
#pragma unroll
        for (int e = 0; e < E; ++e) acc[e] += c * diff[e];
        if (j < i) {
          loss_acc += WEIGHTED ? (double)wij * (double)D : (double)D;
          if (D != D) ++n_nan;
          else if (D - D != T(0)) ++n_inf;
        }
        if (dist != nullptr && lane == 0) dist[(size_t)i * n + j] = D;
      }
    }
  }

  // combine the NS groups of each class in the order s = 0, 1, ..., NS - 1
  __syncthreads();
  if (lane == 0) {
    s_loss[ti][s] = loss_acc;
    s_cnt[ti][s][0] = n_nan;
    s_cnt[ti][s][1] = n_inf;
  }
  const bool want_grad = p.G != nullptr;
  if (want_grad && s > 0) {
    T* mine = tile + (size_t)(ti * (NS - 1) + (s - 1)) * PITCH + lane;
#pragma unroll
    for (int e = 0; e < E; ++e) mine[e * G] = acc[e];
  }
  __syncthreads();
  if (s != 0 || !ivalid) return;
  if (lane == 0) {
    double l = 0.0;
    int c0 = 0, c1 = 0;
    for (int q = 0; q < NS; ++q) {
      l += s_loss[ti][q];
      c0 += s_cnt[ti][q][0];
      c1 += s_cnt[ti][q][1];
    }
    p.loss_part[i] = WEIGHTED ? l : p.weight * l;   // weighted: w_ij went into the sum pair by pair
    p.cnt_part[2 * i] = c0;
    p.cnt_part[2 * i + 1] = c1;
    if (dist != nullptr) dist[(size_t)i * n + i] = sqrt_mode ? math::sqrt(eps) : T(0);   // as the reference: sqrt(0 + eps)
  }
  if (!want_grad) return;
  T* gout = static_cast<T*>(p.G) + (size_t)i * mm;
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const int off = s_map[e * G + lane];
    T tot = acc[e];
    for (int q = 1; q < NS; ++q) tot += tile[(size_t)(ti * (NS - 1) + (q - 1)) * PITCH + e * G + lane];
    if (off >= 0) {
      const int r = off / m, c = off % m;
      gout[off] = tot;
      gout[c * m + r] = tot;
    }
  }
}

template <typename T, int G, int MMAX>
static hipError_t launch_log_euclidean(const LogEucParams& p, hipStream_t stream) {
  using Cfg = LogEucCfg<T, G, MMAX>;
  if (p.W != nullptr)
    hipLaunchKernelGGL((log_euclidean_pair_kernel<Cfg, T, true>), dim3((p.n + Cfg::TI - 1) / Cfg::TI), dim3(256), 0, stream, p);
  else
    hipLaunchKernelGGL((log_euclidean_pair_kernel<Cfg, T, false>), dim3((p.n + Cfg::TI - 1) / Cfg::TI), dim3(256), 0, stream, p);
  return hipGetLastError();
}

// lanes per group by matrix size: the smallest row that holds m; lower triangle of m (m + 1) / 2 entries over G lanes
template <typename T>
static hipError_t dispatch_log_euclidean(const LogEucParams& p, hipStream_t stream) {
  const int m = p.m;
  if (m <= 4) return launch_log_euclidean<T, 4, 4>(p, stream);
  if (m <= 8) return launch_log_euclidean<T, 8, 8>(p, stream);
  if (m <= 16) return launch_log_euclidean<T, 8, 16>(p, stream);
  if (m <= 24) return launch_log_euclidean<T, 16, 24>(p, stream);
  if (m <= 32) return launch_log_euclidean<T, 32, 32>(p, stream);
  if (m <= 48) return launch_log_euclidean<T, 64, 48>(p, stream);
  return launch_log_euclidean<T, 64, 64>(p, stream);
}

// workspace: [sqfa_spd_function's] [L (n,m,m) dtype] [U (n,m,m) double] [lambda (n,m) double] [G (n,m,m) dtype]
//            [partial losses (n) double] [counts (n,2) int]
struct LogEucLayout {
  size_t spd_bytes, off_l, off_u, off_lam, off_g, off_loss, off_cnt, total;   // total 0: no layout for these sizes
};
static LogEucLayout log_euclidean_layout(int n, int m, int dtype) {
  LogEucLayout w{};
  if (n < 2 || m < 1 || m > 64 || (dtype != SQFA_F32 && dtype != SQFA_F64)) return w;
  w.spd_bytes = sqfa_spd_function_workspace_bytes(n, m, dtype);
  if (w.spd_bytes == 0) return w;
  const size_t mat = (size_t)n * m * m;
  WorkspaceCursor ws;
  ws.take(w.spd_bytes);   // sqfa_spd_function's own workspace comes first
  w.off_l = ws.take(mat * dtype_bytes(dtype));
  w.off_u = ws.take(mat * sizeof(double));
  w.off_lam = ws.take((size_t)n * m * sizeof(double));
  w.off_g = ws.take(mat * dtype_bytes(dtype));
  w.off_loss = ws.take((size_t)n * sizeof(double));
  w.off_cnt = ws.take((size_t)n * 2 * sizeof(int));
  w.total = ws.at;
  return w;
}
}  // namespace sqfa

using namespace sqfa;

extern "C" size_t sqfa_log_euclidean_workspace_bytes(int n, int m, int dtype) {
  return log_euclidean_layout(n, m, dtype).total;
}

extern "C" int sqfa_log_euclidean_pairwise_loss_weighted(const void* S, int n, int m, int dtype, int sqrt_mode, double eps,
                                                         const void* pair_weights, double uniform_weight, void* loss_out,
                                                         void* gradS_out, void* dist_out, int* nonfinite_out,
                                                         void* workspace, size_t workspace_bytes, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const LogEucLayout w = log_euclidean_layout(n, m, dtype);
  // (no name: this entry point leaves the text of sqfa_hip_last_error() to sqfa_spd_function)
  int rc = check_pair_loss_args(nullptr, nullptr, S == nullptr, n, m, dtype, sqrt_mode == 0 || sqrt_mode == 1, nullptr,
                                w.total, nullptr, workspace, workspace_bytes);
  if (rc != SQFA_OK) return rc;
  unsigned char* ws = static_cast<unsigned char*>(workspace);
  double* U = reinterpret_cast<double*>(ws + w.off_u);
  double* lam = reinterpret_cast<double*>(ws + w.off_lam);
  // 1. L = log S per class (Cholesky, class_eig_kernel, spd_function_kernel), U and lambda kept for the backward
  rc = sqfa_spd_function(S, n, m, dtype, SQFA_SPD_LOG, ws + w.off_l, U, lam, ws, w.spd_bytes, stream_);
  if (rc != SQFA_OK) return rc;
  // 2. the pass over the ordered pairs
  LogEucParams p{};
  p.L = ws + w.off_l;
  p.G = gradS_out != nullptr ? ws + w.off_g : nullptr;
  p.sqrt_mode = sqrt_mode;
  fill_pair_loss_params(p, n, m, eps, pair_weights, uniform_weight, dist_out, reinterpret_cast<double*>(ws + w.off_loss),
                        reinterpret_cast<int*>(ws + w.off_cnt));
  if (dispatch_dtype(dtype, [&](auto t) { return dispatch_log_euclidean<decltype(t)>(p, stream); }) != hipSuccess)
    return SQFA_ERR_LAUNCH;
  // 3. d loss / d S = Daleckii-Krein backward of the logarithm on G
  if (gradS_out != nullptr) {
    rc = sqfa_spd_function_backward(U, lam, p.G, n, m, dtype, SQFA_SPD_LOG, gradS_out, stream_);
    if (rc != SQFA_OK) return rc;
  }
  // 4. loss and counters
  if (launch_pair_loss_finalize(p.loss_part, p.cnt_part, n, dtype, loss_out, nonfinite_out, stream) != hipSuccess)
    return SQFA_ERR_LAUNCH;
  return SQFA_OK;
}

extern "C" int sqfa_log_euclidean_pairwise_loss(const void* S, int n, int m, int dtype, int sqrt_mode, double eps,
                                                double uniform_weight, void* loss_out, void* gradS_out, void* dist_out,
                                                int* nonfinite_out, void* workspace, size_t workspace_bytes, void* stream_) {
  return sqfa_log_euclidean_pairwise_loss_weighted(S, n, m, dtype, sqrt_mode, eps, nullptr, uniform_weight, loss_out,
                                                   gradS_out, dist_out, nonfinite_out, workspace, workspace_bytes, stream_);
}
