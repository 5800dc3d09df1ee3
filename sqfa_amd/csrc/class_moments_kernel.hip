// class_moments_kernel.hip -- per-class mean, covariance and second moment of labelled points (class_statistics of
// the reference, src/sqfa/statistics.py:8-124: a boolean mask, a mean, a centred X^T X / (n-1) and optional OAS
// shrinkage per class inside a Python loop) as a segmented, centred SYRK, and the same statistics accumulated over
// batches (Chan et al. pairwise merge of count / mean / centred sum; no raw second moments anywhere).
//
//   points (N,D) row-major; row_index (N) int64 or NULL: row k of class c is points[row_index[class_start[c] + k]]
//   (the indices of a stable sort of the labels: no sorted copy of the points), NULL = rows already grouped;
//   class_start (C+1) int64.  Class sizes are read on the device; every grid depends on C and D only.
//
// Launches (all on the caller's stream; nothing allocated, synchronised or read back; no atomics, every sum has a
// fixed order, every output element one writer: results are bitwise reproducible):
//   class_mean_kernel        one workgroup per (class, 32 columns): 8 row lanes x 8 independent double sums per column,
//                            added in a fixed order; mean = sum / n in double, stored in the dtype
//   class_syrk_kernel        one workgroup (4 waves) per (class, 64 x 64 tile of the LOWER block triangle).  The class's
//                            rows are walked in chunks of 32: x - mu (centred in the dtype, as the reference does) of the
//                            tile's two column ranges is staged in LDS as [row][col] (a diagonal tile stages one range)
//                            and BOTH operands of the exact MFMA (v_mfma_f32_16x16x4_f32 / v_mfma_f64_16x16x4_f64,
//                            proj_traits.hpp) are read from it: A[i][k] = s[k][i0+i], B[k][j] = s[k][j0+j].  Each wave
//                            owns a 32 x 32 quadrant = 2 x 2 accumulators; the next chunk's global loads (and the row
//                            indices of the one after) are in flight during the MFMAs.  Rows past the end of the
//                            class and columns past D are zeros.
//                            Epilogue (tile_epilogue): the tile goes through LDS once so that the tile AND its transpose
//                            are stored with the column on the lane (coalesced both ways); an off-diagonal tile is
//                            stored twice from the same values, so the (C,D,D) outputs are exactly symmetric.
//   class_oas_finish_kernel  sums the per-(class, tile) partials of tr S and sum S o S in a fixed order, forms rho
//                            (Chen et al. 2010, clamp at 1) in double, rewrites the class as (1-rho) S + rho tr/D I and
//                            writes the second moment in the same pass
//   class_shrinkage_finish_kernel  sqfa_class_shrinkage: the SYRK in its measuring mode (CM_MEASURE: the same chunk walk, MFMA,
//                            s = v / (n - 1) and per-tile partials, and NO store of anything of size (D,D)), then the same
//                            sum of the partials and the same rho, written as keep = 1 - rho and shift = rho tr / D per class
//   class_mean_merge_kernel  accumulate mode, after the SYRK (whose epilogue needs the old mean): means, counts
//   class_finalize_kernel    accumulator -> statistics: the epilogue above applied to tiles of M2
// LDS rows have a pitch of 80 elements: the 16 lanes of k and of k+1 that one MFMA operand read puts in one lane group
// land on disjoint halves of the banks (80 = 16 mod 32 floats, 160 = 32 mod 64 dwords for doubles).
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>

#include "../../include/sqfa_hip.h"
#include "proj_traits.hpp"

namespace sqfa {

constexpr int CM_TILE = 64;            // output tile edge
constexpr int CM_KC = 32;              // rows of the class per chunk
constexpr int CM_PITCH = 80;           // LDS row pitch of the staged chunk
constexpr int CM_TPITCH = 65;          // LDS row pitch of the finished tile
constexpr int CM_THREADS = 256;
constexpr int CM_PER_THREAD = CM_TILE * CM_KC / CM_THREADS;   // staged elements per thread and column range (8)
constexpr int CM_MEAN_COLS = 32;
constexpr int CM_MEAN_LANES = 8;

enum { CM_EMPIRICAL = SQFA_COV_EMPIRICAL, CM_OAS = SQFA_COV_OAS, CM_SCATTER = SQFA_COV_SCATTER, CM_ACCUMULATE = 3, CM_MEASURE = 4 };

__host__ __device__ inline int cm_tiles(int D) { return (D + CM_TILE - 1) / CM_TILE; }
__host__ __device__ inline size_t cm_tri_tiles(int D) { return (size_t)cm_tiles(D) * (cm_tiles(D) + 1) / 2; }

// tile t of the lower block triangle -> (ti >= tj), row-major over the triangle
__device__ __forceinline__ void cm_tile_of(int t, int* ti, int* tj) {
  int i = (int)((sqrt(8.0 * t + 1.0) - 1.0) * 0.5);
  while ((i + 1) * (i + 2) / 2 <= t) ++i;
  while (i * (i + 1) / 2 > t) --i;
  *ti = i;
  *tj = t - i * (i + 1) / 2;
}

__device__ __forceinline__ size_t cm_row(const long long* __restrict__ row_index, long long k) {
  return (size_t)(row_index != nullptr ? row_index[k] : k);
}

template <typename T>
__global__ __launch_bounds__(CM_THREADS) void class_mean_kernel(const T* __restrict__ points, int D,
                                                                const long long* __restrict__ row_index,
                                                                const long long* __restrict__ class_start,
                                                                T* __restrict__ means_out) {
  __shared__ double sSum[CM_MEAN_LANES][CM_MEAN_COLS];
  const int c = blockIdx.y, col = blockIdx.x * CM_MEAN_COLS + (threadIdx.x % CM_MEAN_COLS), lane = threadIdx.x / CM_MEAN_COLS;
  const long long start = class_start[c], n = class_start[c + 1] - start;
  constexpr int U = 8;   // independent sums (and rows in flight) per thread
  double a[U] = {};
  if (col < D) {
    long long k = lane;
    for (; k + (U - 1) * CM_MEAN_LANES < n; k += U * CM_MEAN_LANES) {
      size_t r[U];
      T x[U];
#pragma unroll
      for (int u = 0; u < U; ++u) r[u] = cm_row(row_index, start + k + u * CM_MEAN_LANES);
#pragma unroll
      for (int u = 0; u < U; ++u) x[u] = points[r[u] * D + col];
#pragma unroll
      for (int u = 0; u < U; ++u) a[u] += (double)x[u];
    }
    for (; k < n; k += CM_MEAN_LANES) a[0] += (double)points[cm_row(row_index, start + k) * D + col];
  }
  sSum[lane][threadIdx.x % CM_MEAN_COLS] = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
  __syncthreads();
  if (lane == 0 && col < D) {
    double s = 0.0;
    for (int q = 0; q < CM_MEAN_LANES; ++q) s += sSum[q][threadIdx.x];
    means_out[(size_t)c * D + col] = (T)(s / (double)n);   // n = 0: 0/0 = NaN, as the reference's mean of no rows
  }
}

// Everything the epilogue of one tile needs beside the tile itself.
template <typename T> struct TileOut {
  int mode;            // CM_*
  int D, i0, j0;       // tile origin: rows i0.., columns j0.. (i0 >= j0)
  double n;            // class size (CM_ACCUMULATE: unused)
  T w;                 // CM_ACCUMULATE: n_a n_b / (n_a + n_b)
  T* cov;              // this class's (D,D) output (CM_ACCUMULATE: M2, read and written; CM_MEASURE: never touched)
  T* second;           // or NULL
  double* partial;     // CM_OAS, CM_MEASURE: this tile's {tr S, sum S o S}
};

// One element: v = raw centred sum at (gi, gj); a, b = mean_i, mean_j; da, db = delta_i, delta_j.  Every product is
// commutative in (i, j), so the two lanes that compute (i, j) and (j, i) of a diagonal tile agree bit for bit.
template <typename T>
__device__ __forceinline__ void cm_emit(const TileOut<T>& o, T v, int gi, int gj, T a, T b, T da, T db, double weight,
                                        double* tr, double* sq) {
  const size_t at = (size_t)gi * o.D + gj;
  if (o.mode == CM_ACCUMULATE) {
    const T dd = da * db;
    o.cov[at] = o.cov[at] + (v + o.w * dd);
    return;
  }
  if (o.mode == CM_SCATTER) {
    o.cov[at] = v;
    return;
  }
  const T s = o.n < 1.0 ? (T)NAN : v / (T)(o.n - 1.0);   // n = 1: 0/0 = NaN; n = 0: NaN like the mean
  if (o.mode != CM_MEASURE) o.cov[at] = s;
  if (o.mode == CM_OAS || o.mode == CM_MEASURE) {
    if (gi == gj) *tr += (double)s;
    *sq += weight * (double)s * (double)s;
  } else if (o.second != nullptr) {
    const T ab = a * b;
    o.second[at] = s + ab;
  }
}

// sT: the finished 64 x 64 tile, [i - i0][j - j0] with pitch CM_TPITCH.  Stores it at (i, j) and, for an off-diagonal
// tile, at (j, i), the output column on the lane both times.
template <typename T>
__device__ __forceinline__ void tile_epilogue(const TileOut<T>& o, const T* sT, const T* sMuI, const T* sMuJ,
                                              const T* sDI, const T* sDJ, double* sRed) {
  const int tid = threadIdx.x;
  const bool diag = o.i0 == o.j0;
  double tr = 0.0, sq = 0.0;
  for (int idx = tid; idx < CM_TILE * CM_TILE; idx += CM_THREADS) {
    const int r = idx / CM_TILE, cc = idx % CM_TILE, gi = o.i0 + r, gj = o.j0 + cc;
    if (gi < o.D && gj < o.D) cm_emit(o, sT[r * CM_TPITCH + cc], gi, gj, sMuI[r], sMuJ[cc], sDI[r], sDJ[cc], diag ? 1.0 : 2.0, &tr, &sq);
  }
  if (!diag && o.mode != CM_MEASURE) {
    double tr2 = 0.0, sq2 = 0.0;   // the mirrored copy is not counted again
    for (int idx = tid; idx < CM_TILE * CM_TILE; idx += CM_THREADS) {
      const int r = idx / CM_TILE, cc = idx % CM_TILE, gj = o.j0 + r, gi = o.i0 + cc;
      if (gi < o.D && gj < o.D) cm_emit(o, sT[cc * CM_TPITCH + r], gj, gi, sMuJ[r], sMuI[cc], sDJ[r], sDI[cc], 0.0, &tr2, &sq2);
    }
  }
  if (o.mode == CM_OAS || o.mode == CM_MEASURE) {   // workgroup sum in a fixed order
    for (int off = 32; off > 0; off >>= 1) {
      tr += __shfl_down(tr, off);
      sq += __shfl_down(sq, off);
    }
    if ((tid & 63) == 0) {
      sRed[2 * (tid >> 6)] = tr;
      sRed[2 * (tid >> 6) + 1] = sq;
    }
    __syncthreads();
    if (tid == 0) {
      o.partial[0] = (sRed[0] + sRed[2]) + (sRed[4] + sRed[6]);
      o.partial[1] = (sRed[1] + sRed[3]) + (sRed[5] + sRed[7]);
    }
  }
}

// VEC: 16-byte loads (D % VW == 0 and an aligned base); otherwise one element per load.
template <typename T, bool VEC> struct ChunkLoad {
  using Tr = ProjTraits<T>;
  static constexpr int VW = VEC ? Tr::VW : 1;
  static constexpr int LANES_PER_ROW = CM_TILE / VW;               // threads across one row of 64 columns
  static constexpr int ROWS_PER_PASS = CM_THREADS / LANES_PER_ROW;
  static constexpr int PASSES = CM_KC / ROWS_PER_PASS;             // PASSES * VW = CM_PER_THREAD
  T v[CM_PER_THREAD];

  // this thread's rows of the chunk k0 .. k0+31 of the class (n rows from `start`): read a chunk before the points are,
  // so that a gathered row costs one memory latency per chunk, not two
  static __device__ __forceinline__ void index(size_t* rows, const long long* __restrict__ row_index, long long start,
                                               long long n, long long k0) {
    const int r0 = threadIdx.x / LANES_PER_ROW;
#pragma unroll
    for (int p = 0; p < PASSES; ++p) {
      const long long k = k0 + r0 + p * ROWS_PER_PASS;
      rows[p] = k < n ? cm_row(row_index, start + k) : 0;
    }
  }

  // rows k0 .. k0+31 of the class (`rows` from index()), columns c0 .. c0+63
  __device__ __forceinline__ void load(const T* __restrict__ points, int D, const size_t* rows, long long n, long long k0,
                                       int c0) {
    const int col = c0 + (threadIdx.x % LANES_PER_ROW) * VW, r0 = threadIdx.x / LANES_PER_ROW;
#pragma unroll
    for (int p = 0; p < PASSES; ++p) {
      const long long k = k0 + r0 + p * ROWS_PER_PASS;
      const bool in = k < n && col < D;   // VEC: D % VW == 0, so a vector is inside or outside as a whole
      if constexpr (VEC) {
        typename Tr::Vec x = {};
        if (in) x = *reinterpret_cast<const typename Tr::Vec*>(points + rows[p] * D + col);
#pragma unroll
        for (int e = 0; e < VW; ++e) v[p * VW + e] = x[e];
      } else {
        v[p] = in ? points[rows[p] * D + col] : (T)0;
      }
    }
  }

  // centred in the dtype; rows past the class and columns past D stay exact zeros
  __device__ __forceinline__ void store(T* s, const T* sMu, int D, long long n, long long k0, int c0) const {
    const int lc = (threadIdx.x % LANES_PER_ROW) * VW, r0 = threadIdx.x / LANES_PER_ROW;
#pragma unroll
    for (int p = 0; p < PASSES; ++p) {
      const int r = r0 + p * ROWS_PER_PASS;
      const bool row_in = k0 + r < n;
#pragma unroll
      for (int e = 0; e < VW; ++e)
        s[r * CM_PITCH + lc + e] = (row_in && c0 + lc + e < D) ? v[p * VW + e] - sMu[lc + e] : (T)0;
    }
  }
};

template <typename T, bool VEC>
__global__ __launch_bounds__(CM_THREADS) void class_syrk_kernel(const T* __restrict__ points, int D,
                                                                const long long* __restrict__ row_index,
                                                                const long long* __restrict__ class_start,
                                                                const T* __restrict__ mu, int mode, T* out, T* second,
                                                                double* __restrict__ partials,
                                                                const double* __restrict__ counts,
                                                                const T* __restrict__ run_means) {
  using Tr = ProjTraits<T>;
  __shared__ T smem[2 * CM_KC * CM_PITCH];   // the staged chunk (two column ranges), then the finished tile
  __shared__ T sMuI[CM_TILE], sMuJ[CM_TILE], sDI[CM_TILE], sDJ[CM_TILE];
  __shared__ double sRed[8];
  static_assert(CM_TILE * CM_TPITCH <= 2 * CM_KC * CM_PITCH, "the finished tile reuses the staging buffer");

  const int ntri = (int)cm_tri_tiles(D);
  const int c = blockIdx.x / ntri, t = blockIdx.x % ntri, tid = threadIdx.x;
  int ti, tj;
  cm_tile_of(t, &ti, &tj);
  const int i0 = ti * CM_TILE, j0 = tj * CM_TILE;
  const bool diag = ti == tj;
  const long long start = class_start[c], n = class_start[c + 1] - start;
  if (mode == CM_ACCUMULATE && n == 0) return;   // a class absent from the batch is left untouched

  TileOut<T> o;
  o.mode = mode;
  o.D = D;
  o.i0 = i0;
  o.j0 = j0;
  o.n = (double)n;
  o.w = (T)0;
  o.cov = out != nullptr ? out + (size_t)c * D * D : nullptr;
  o.second = second != nullptr ? second + (size_t)c * D * D : nullptr;
  o.partial = partials != nullptr ? partials + 2 * ((size_t)c * ntri + t) : nullptr;
  double n_a = 0.0;
  if (mode == CM_ACCUMULATE) {
    n_a = counts[c];
    o.w = n_a > 0.0 ? (T)(n_a * (double)n / (n_a + (double)n)) : (T)0;
  }
  if (tid < 2 * CM_TILE) {
    const int e = tid % CM_TILE, col = (tid < CM_TILE ? i0 : j0) + e;
    const T m = col < D ? mu[(size_t)c * D + col] : (T)0;
    T d = (T)0;
    if (mode == CM_ACCUMULATE && n_a > 0.0 && col < D) d = m - run_means[(size_t)c * D + col];
    (tid < CM_TILE ? sMuI : sMuJ)[e] = m;
    (tid < CM_TILE ? sDI : sDJ)[e] = d;
  }

  T* sI = smem;
  T* sJ = diag ? smem : smem + CM_KC * CM_PITCH;
  const int l = tid & 63, wave = tid >> 6, q = l >> 4, wi = (wave >> 1) * 32, wj = (wave & 1) * 32;
  typename Tr::Acc acc[2][2] = {};
  using Chunk = ChunkLoad<T, VEC>;
  Chunk ldI, ldJ;
  size_t rows[Chunk::PASSES];
  if (n > 0) {
    Chunk::index(rows, row_index, start, n, 0);
    ldI.load(points, D, rows, n, 0, i0);
    if (!diag) ldJ.load(points, D, rows, n, 0, j0);
    Chunk::index(rows, row_index, start, n, CM_KC);
  }
  for (long long k0 = 0; k0 < n; k0 += CM_KC) {
    __syncthreads();   // the previous chunk has been consumed (first pass: the means are in LDS)
    ldI.store(sI, sMuI, D, n, k0, i0);
    if (!diag) ldJ.store(sJ, sMuJ, D, n, k0, j0);
    __syncthreads();
    if (k0 + CM_KC < n) {
      ldI.load(points, D, rows, n, k0 + CM_KC, i0);
      if (!diag) ldJ.load(points, D, rows, n, k0 + CM_KC, j0);
      Chunk::index(rows, row_index, start, n, k0 + 2 * CM_KC);
    }
#pragma unroll
    for (int kk = 0; kk < CM_KC; kk += 4) {
      const T a0 = sI[(kk + q) * CM_PITCH + wi + (l & 15)], a1 = sI[(kk + q) * CM_PITCH + wi + 16 + (l & 15)];
      const T b0 = sJ[(kk + q) * CM_PITCH + wj + (l & 15)], b1 = sJ[(kk + q) * CM_PITCH + wj + 16 + (l & 15)];
      acc[0][0] = Tr::mfma(a0, b0, acc[0][0]);
      acc[0][1] = Tr::mfma(a0, b1, acc[0][1]);
      acc[1][0] = Tr::mfma(a1, b0, acc[1][0]);
      acc[1][1] = Tr::mfma(a1, b1, acc[1][1]);
    }
  }
  __syncthreads();
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int v = 0; v < 2; ++v)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg)
        smem[(wi + 16 * u + Tr::acc_row(q, reg)) * CM_TPITCH + wj + 16 * v + (l & 15)] = acc[u][v][reg];
  __syncthreads();
  tile_epilogue(o, smem, sMuI, diag ? sMuI : sMuJ, sDI, diag ? sDI : sDJ, sRed);
}

// accumulator -> statistics: tiles of M2 through the same epilogue (mode CM_EMPIRICAL or CM_OAS)
template <typename T>
__global__ __launch_bounds__(CM_THREADS) void class_finalize_kernel(const double* __restrict__ counts,
                                                                    const T* __restrict__ means,
                                                                    const T* __restrict__ m2, int D, int mode, T* out,
                                                                    T* second, double* __restrict__ partials) {
  __shared__ T sT[CM_TILE * CM_TPITCH];
  __shared__ T sMuI[CM_TILE], sMuJ[CM_TILE], sZero[CM_TILE];
  __shared__ double sRed[8];
  const int ntri = (int)cm_tri_tiles(D);
  const int c = blockIdx.x / ntri, t = blockIdx.x % ntri, tid = threadIdx.x;
  int ti, tj;
  cm_tile_of(t, &ti, &tj);
  const int i0 = ti * CM_TILE, j0 = tj * CM_TILE;
  TileOut<T> o;
  o.mode = mode;
  o.D = D;
  o.i0 = i0;
  o.j0 = j0;
  o.n = counts[c];
  o.w = (T)0;
  o.cov = out + (size_t)c * D * D;
  o.second = second != nullptr ? second + (size_t)c * D * D : nullptr;
  o.partial = partials != nullptr ? partials + 2 * ((size_t)c * ntri + t) : nullptr;
  if (tid < 2 * CM_TILE) {
    const int e = tid % CM_TILE, col = (tid < CM_TILE ? i0 : j0) + e;
    (tid < CM_TILE ? sMuI : sMuJ)[e] = col < D ? means[(size_t)c * D + col] : (T)0;
    if (tid < CM_TILE) sZero[e] = (T)0;
  }
  const T* src = m2 + (size_t)c * D * D;
  for (int idx = tid; idx < CM_TILE * CM_TILE; idx += CM_THREADS) {
    const int r = idx / CM_TILE, cc = idx % CM_TILE, gi = i0 + r, gj = j0 + cc;
    sT[r * CM_TPITCH + cc] = (gi < D && gj < D) ? src[(size_t)gi * D + gj] : (T)0;
  }
  __syncthreads();
  tile_epilogue(o, sT, sMuI, sMuJ, sZero, sZero, sRed);
}

// The OAS coefficients of one class from its per-tile partials, by the whole workgroup: the sums in a fixed order, rho
// (Chen et al. 2010, clamp at 1) in double, keep = 1 - rho and shift = rho tr / D rounded to the dtype.  The one place
// where they are formed: the dense statistics and sqfa_class_shrinkage get the same bits.
template <typename T>
__device__ __forceinline__ void cm_oas_coefficients(const double* __restrict__ p, int ntri, double n, int D, double* sTr,
                                                    double* sSq, T* keep, T* shift, double* rho_out) {
  const int tid = threadIdx.x;
  double tr = 0.0, sq = 0.0;
  for (int t = tid; t < ntri; t += CM_THREADS) {
    tr += p[2 * t];
    sq += p[2 * t + 1];
  }
  sTr[tid] = tr;
  sSq[tid] = sq;
  __syncthreads();
  for (int off = CM_THREADS / 2; off > 0; off >>= 1) {
    if (tid < off) {
      sTr[tid] += sTr[tid + off];
      sSq[tid] += sSq[tid + off];
    }
    __syncthreads();
  }
  tr = sTr[0];
  const double tr2 = sSq[0], d = (double)D;
  double rho = ((1.0 - 2.0 / d) * tr2 + tr * tr) / ((n + 1.0 - 2.0 / d) * (tr2 - tr * tr / d));
  if (rho > 1.0) rho = 1.0;   // NaN stays NaN, as torch.clamp keeps it
  *keep = (T)(1.0 - rho);
  *shift = (T)(rho * tr / d);
  *rho_out = rho;
}

template <typename T>
__global__ __launch_bounds__(CM_THREADS) void class_oas_finish_kernel(const double* __restrict__ partials,
                                                                      const long long* __restrict__ class_start,
                                                                      const double* __restrict__ counts,
                                                                      const T* __restrict__ means, int D, T* cov,
                                                                      T* second) {
  __shared__ double sTr[CM_THREADS], sSq[CM_THREADS];
  const int ntri = (int)cm_tri_tiles(D);
  const int c = blockIdx.y, tid = threadIdx.x;
  const double n = class_start != nullptr ? (double)(class_start[c + 1] - class_start[c]) : counts[c];
  T keep, shift;
  double rho;
  cm_oas_coefficients<T>(partials + 2 * (size_t)c * ntri, ntri, n, D, sTr, sSq, &keep, &shift, &rho);
  T* S = cov + (size_t)c * D * D;
  T* M = second != nullptr ? second + (size_t)c * D * D : nullptr;
  const T* mu = means + (size_t)c * D;
  const size_t total = (size_t)D * D;
  for (size_t e = (size_t)blockIdx.x * CM_THREADS + tid; e < total; e += (size_t)gridDim.x * CM_THREADS) {
    const int i = (int)(e / D), j = (int)(e % D);
    T s = keep * S[e];
    if (i == j) s = s + shift;
    S[e] = s;
    if (M != nullptr) {
      const T ab = mu[i] * mu[j];
      M[e] = s + ab;
    }
  }
}

// sqfa_class_shrinkage: one workgroup per class; a class below two points has no covariance to shrink: NaN throughout
template <typename T>
__global__ __launch_bounds__(CM_THREADS) void class_shrinkage_finish_kernel(const double* __restrict__ partials,
                                                                            const long long* __restrict__ class_start,
                                                                            int D, T* __restrict__ keep_out,
                                                                            T* __restrict__ shift_out,
                                                                            double* __restrict__ rho_out) {
  __shared__ double sTr[CM_THREADS], sSq[CM_THREADS];
  const int ntri = (int)cm_tri_tiles(D);
  const int c = blockIdx.x;
  const double n = (double)(class_start[c + 1] - class_start[c]);
  T keep, shift;
  double rho;
  cm_oas_coefficients<T>(partials + 2 * (size_t)c * ntri, ntri, n, D, sTr, sSq, &keep, &shift, &rho);
  if (threadIdx.x == 0) {
    const bool some = n >= 2.0;
    keep_out[c] = some ? keep : (T)NAN;
    shift_out[c] = some ? shift : (T)NAN;
    if (rho_out != nullptr) rho_out[c] = some ? rho : (double)NAN;
  }
}

// means += delta n_b / (n_a + n_b), counts += n_b; after the SYRK, whose epilogue reads the old mean and count
template <typename T>
__global__ __launch_bounds__(CM_THREADS) void class_mean_merge_kernel(const long long* __restrict__ class_start,
                                                                      const T* __restrict__ batch_means, int D,
                                                                      double* counts, T* means) {
  const int c = blockIdx.x;
  const double n_b = (double)(class_start[c + 1] - class_start[c]);
  if (n_b == 0.0) return;
  const double n_a = counts[c], tot = n_a + n_b;
  const T f = (T)(n_b / tot);
  for (int d = threadIdx.x; d < D; d += CM_THREADS) {
    const size_t at = (size_t)c * D + d;
    const T mb = batch_means[at];
    means[at] = n_a > 0.0 ? means[at] + (mb - means[at]) * f : mb;
  }
  __syncthreads();   // every thread has read counts[c]
  if (threadIdx.x == 0) counts[c] = tot;
}

struct CmLayout {
  size_t means_off, partials_off, total;
};

static bool cm_layout(int C, int D, int dtype, CmLayout* w) {
  if (C < 1 || D < 1 || (dtype != SQFA_F32 && dtype != SQFA_F64)) return false;
  if ((size_t)C * cm_tri_tiles(D) > (size_t)INT_MAX) return false;   // one workgroup per (class, tile) in grid.x
  if (C > 65535) return false;                                       // classes in grid.y of the small kernels
  const size_t esz = dtype == SQFA_F32 ? 4 : 8;
  w->means_off = 0;
  w->partials_off = ((size_t)C * D * esz + 15) & ~(size_t)15;
  w->total = w->partials_off + (size_t)C * cm_tri_tiles(D) * 2 * sizeof(double);
  return true;
}

template <typename T>
static void launch_syrk(const T* points, int D, const long long* row_index, const long long* class_start, int C,
                        const T* mu, int mode, T* out, T* second, double* partials, const double* counts,
                        const T* run_means, hipStream_t stream) {
  const unsigned grid = (unsigned)((size_t)C * cm_tri_tiles(D));
  const bool vec = (D % ProjTraits<T>::VW) == 0 && (reinterpret_cast<size_t>(points) & 15) == 0;
  if (vec)
    class_syrk_kernel<T, true><<<grid, CM_THREADS, 0, stream>>>(points, D, row_index, class_start, mu, mode, out, second,
                                                                 partials, counts, run_means);
  else
    class_syrk_kernel<T, false><<<grid, CM_THREADS, 0, stream>>>(points, D, row_index, class_start, mu, mode, out, second,
                                                                  partials, counts, run_means);
}

static unsigned cm_finish_blocks(int D) {
  const size_t want = ((size_t)D * D + 8 * CM_THREADS - 1) / (8 * CM_THREADS);
  return (unsigned)(want < 1 ? 1 : (want > 256 ? 256 : want));
}

template <typename T>
static void run_moments(const T* points, int D, const long long* row_index, const long long* class_start, int C,
                        int estimator, T* means_out, T* cov_out, T* second_out, char* ws, const CmLayout& w,
                        hipStream_t stream) {
  double* partials = reinterpret_cast<double*>(ws + w.partials_off);
  class_mean_kernel<T><<<dim3((D + CM_MEAN_COLS - 1) / CM_MEAN_COLS, C), CM_THREADS, 0, stream>>>(points, D, row_index,
                                                                                                 class_start, means_out);
  launch_syrk<T>(points, D, row_index, class_start, C, means_out, estimator, cov_out,
                 estimator == SQFA_COV_EMPIRICAL ? second_out : nullptr, estimator == SQFA_COV_OAS ? partials : nullptr,
                 nullptr, nullptr, stream);
  if (estimator == SQFA_COV_OAS)
    class_oas_finish_kernel<T><<<dim3(cm_finish_blocks(D), C), CM_THREADS, 0, stream>>>(partials, class_start, nullptr,
                                                                                       means_out, D, cov_out, second_out);
}

template <typename T>
static void run_update(const T* points, int D, const long long* row_index, const long long* class_start, int C,
                       double* counts, T* means, T* m2, char* ws, const CmLayout& w, hipStream_t stream) {
  T* batch_means = reinterpret_cast<T*>(ws + w.means_off);
  class_mean_kernel<T><<<dim3((D + CM_MEAN_COLS - 1) / CM_MEAN_COLS, C), CM_THREADS, 0, stream>>>(points, D, row_index,
                                                                                                 class_start, batch_means);
  launch_syrk<T>(points, D, row_index, class_start, C, batch_means, CM_ACCUMULATE, m2, nullptr, nullptr, counts, means, stream);
  class_mean_merge_kernel<T><<<C, CM_THREADS, 0, stream>>>(class_start, batch_means, D, counts, means);
}

template <typename T>
static void run_finalize(const double* counts, const T* means, const T* m2, int C, int D, int estimator, T* cov_out,
                         T* second_out, char* ws, const CmLayout& w, hipStream_t stream) {
  double* partials = reinterpret_cast<double*>(ws + w.partials_off);
  const unsigned grid = (unsigned)((size_t)C * cm_tri_tiles(D));
  class_finalize_kernel<T><<<grid, CM_THREADS, 0, stream>>>(counts, means, m2, D, estimator, cov_out,
                                                            estimator == SQFA_COV_EMPIRICAL ? second_out : nullptr,
                                                            estimator == SQFA_COV_OAS ? partials : nullptr);
  if (estimator == SQFA_COV_OAS)
    class_oas_finish_kernel<T><<<dim3(cm_finish_blocks(D), C), CM_THREADS, 0, stream>>>(partials, nullptr, counts, means, D,
                                                                                       cov_out, second_out);
}

}  // namespace sqfa

extern "C" size_t sqfa_class_moments_workspace_bytes(int C, int D, int dtype) {
  sqfa::CmLayout w;
  return sqfa::cm_layout(C, D, dtype, &w) ? w.total : 0;
}

extern "C" int sqfa_class_moments(const void* points, long long N, int D, const long long* row_index,
                                  const long long* class_start, int C, int dtype, int estimator, void* means_out,
                                  void* cov_out, void* second_out, void* workspace, size_t workspace_bytes, void* stream_) {
  using namespace sqfa;
  if (N < 0 || C < 1 || D < 1 || (points == nullptr && N > 0) || class_start == nullptr || means_out == nullptr ||
      cov_out == nullptr)
    return SQFA_ERR_BAD_ARGUMENT;
  if (dtype != SQFA_F32 && dtype != SQFA_F64) return SQFA_ERR_BAD_ARGUMENT;
  if (estimator != SQFA_COV_EMPIRICAL && estimator != SQFA_COV_OAS && estimator != SQFA_COV_SCATTER) return SQFA_ERR_BAD_ARGUMENT;
  CmLayout w;
  if (!cm_layout(C, D, dtype, &w)) return SQFA_ERR_UNSUPPORTED_M;
  if (workspace == nullptr || workspace_bytes < w.total) return SQFA_ERR_WORKSPACE;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  char* ws = static_cast<char*>(workspace);
  if (dtype == SQFA_F32)
    run_moments(static_cast<const float*>(points), D, row_index, class_start, C, estimator, static_cast<float*>(means_out),
                static_cast<float*>(cov_out), static_cast<float*>(second_out), ws, w, stream);
  else
    run_moments(static_cast<const double*>(points), D, row_index, class_start, C, estimator, static_cast<double*>(means_out),
                static_cast<double*>(cov_out), static_cast<double*>(second_out), ws, w, stream);
  return hipGetLastError() == hipSuccess ? SQFA_OK : SQFA_ERR_LAUNCH;
}

// the means alone (class_mean_kernel as sqfa_class_moments launches it: the same bits)
extern "C" int sqfa_class_means(const void* points, long long N, int D, const long long* row_index,
                                const long long* class_start, int C, int dtype, void* means_out, void* stream_) {
  using namespace sqfa;
  if (N < 0 || C < 1 || D < 1 || (points == nullptr && N > 0) || class_start == nullptr || means_out == nullptr)
    return SQFA_ERR_BAD_ARGUMENT;
  if (dtype != SQFA_F32 && dtype != SQFA_F64) return SQFA_ERR_BAD_ARGUMENT;
  if (C > 65535) return SQFA_ERR_UNSUPPORTED_M;   // classes in grid.y
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const dim3 grid((D + CM_MEAN_COLS - 1) / CM_MEAN_COLS, C);
  if (dtype == SQFA_F32)
    class_mean_kernel<float><<<grid, CM_THREADS, 0, stream>>>(static_cast<const float*>(points), D, row_index, class_start,
                                                              static_cast<float*>(means_out));
  else
    class_mean_kernel<double><<<grid, CM_THREADS, 0, stream>>>(static_cast<const double*>(points), D, row_index, class_start,
                                                               static_cast<double*>(means_out));
  return hipGetLastError() == hipSuccess ? SQFA_OK : SQFA_ERR_LAUNCH;
}

// keep = 1 - rho and shift = rho tr / D of the OAS shrinkage, measured from the points: the SYRK without its stores
extern "C" int sqfa_class_shrinkage(const void* points, long long N, int D, const long long* row_index,
                                    const long long* class_start, int C, int dtype, const void* means, void* keep_out,
                                    void* shift_out, double* rho_out, void* workspace, size_t workspace_bytes,
                                    void* stream_) {
  using namespace sqfa;
  if (N < 0 || C < 1 || D < 1 || (points == nullptr && N > 0) || class_start == nullptr || means == nullptr ||
      keep_out == nullptr || shift_out == nullptr)
    return SQFA_ERR_BAD_ARGUMENT;
  if (dtype != SQFA_F32 && dtype != SQFA_F64) return SQFA_ERR_BAD_ARGUMENT;
  CmLayout w;
  if (!cm_layout(C, D, dtype, &w)) return SQFA_ERR_UNSUPPORTED_M;
  if (workspace == nullptr || workspace_bytes < w.total) return SQFA_ERR_WORKSPACE;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  double* partials = reinterpret_cast<double*>(static_cast<char*>(workspace) + w.partials_off);
  if (dtype == SQFA_F32) {
    launch_syrk<float>(static_cast<const float*>(points), D, row_index, class_start, C, static_cast<const float*>(means),
                       CM_MEASURE, nullptr, nullptr, partials, nullptr, nullptr, stream);
    class_shrinkage_finish_kernel<float><<<C, CM_THREADS, 0, stream>>>(partials, class_start, D, static_cast<float*>(keep_out),
                                                                       static_cast<float*>(shift_out), rho_out);
  } else {
    launch_syrk<double>(static_cast<const double*>(points), D, row_index, class_start, C, static_cast<const double*>(means),
                        CM_MEASURE, nullptr, nullptr, partials, nullptr, nullptr, stream);
    class_shrinkage_finish_kernel<double><<<C, CM_THREADS, 0, stream>>>(partials, class_start, D, static_cast<double*>(keep_out),
                                                                        static_cast<double*>(shift_out), rho_out);
  }
  return hipGetLastError() == hipSuccess ? SQFA_OK : SQFA_ERR_LAUNCH;
}

extern "C" int sqfa_class_moments_update(const void* points, long long N, int D, const long long* row_index,
                                         const long long* class_start, int C, int dtype, double* counts, void* means,
                                         void* m2, void* workspace, size_t workspace_bytes, void* stream_) {
  using namespace sqfa;
  if (N < 0 || C < 1 || D < 1 || (points == nullptr && N > 0) || class_start == nullptr || counts == nullptr ||
      means == nullptr || m2 == nullptr)
    return SQFA_ERR_BAD_ARGUMENT;
  if (dtype != SQFA_F32 && dtype != SQFA_F64) return SQFA_ERR_BAD_ARGUMENT;
  CmLayout w;
  if (!cm_layout(C, D, dtype, &w)) return SQFA_ERR_UNSUPPORTED_M;
  if (workspace == nullptr || workspace_bytes < w.total) return SQFA_ERR_WORKSPACE;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  char* ws = static_cast<char*>(workspace);
  if (dtype == SQFA_F32)
    run_update(static_cast<const float*>(points), D, row_index, class_start, C, counts, static_cast<float*>(means),
               static_cast<float*>(m2), ws, w, stream);
  else
    run_update(static_cast<const double*>(points), D, row_index, class_start, C, counts, static_cast<double*>(means),
               static_cast<double*>(m2), ws, w, stream);
  return hipGetLastError() == hipSuccess ? SQFA_OK : SQFA_ERR_LAUNCH;
}

extern "C" int sqfa_class_moments_finalize(const double* counts, const void* means, const void* m2, int C, int D, int dtype,
                                           int estimator, void* cov_out, void* second_out, void* workspace,
                                           size_t workspace_bytes, void* stream_) {
  using namespace sqfa;
  if (C < 1 || D < 1 || counts == nullptr || means == nullptr || m2 == nullptr || cov_out == nullptr)
    return SQFA_ERR_BAD_ARGUMENT;
  if (dtype != SQFA_F32 && dtype != SQFA_F64) return SQFA_ERR_BAD_ARGUMENT;
  if (estimator != SQFA_COV_EMPIRICAL && estimator != SQFA_COV_OAS) return SQFA_ERR_BAD_ARGUMENT;
  CmLayout w;
  if (!cm_layout(C, D, dtype, &w)) return SQFA_ERR_UNSUPPORTED_M;
  if (workspace == nullptr || workspace_bytes < w.total) return SQFA_ERR_WORKSPACE;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  char* ws = static_cast<char*>(workspace);
  if (dtype == SQFA_F32)
    run_finalize(counts, static_cast<const float*>(means), static_cast<const float*>(m2), C, D, estimator,
                 static_cast<float*>(cov_out), static_cast<float*>(second_out), ws, w, stream);
  else
    run_finalize(counts, static_cast<const double*>(means), static_cast<const double*>(m2), C, D, estimator,
                 static_cast<double*>(cov_out), static_cast<double*>(second_out), ws, w, stream);
  return hipGetLastError() == hipSuccess ? SQFA_OK : SQFA_ERR_LAUNCH;
}
