// class_points_kernel.hip -- the class moments of the PROJECTED points, straight from the labelled points: what a
// closure needs of class_statistics (reference src/sqfa/statistics.py:8-124) followed by F cov_c F^T / F mu_c
// (transform_scatters, src/sqfa/model.py:172-188; conjugate_matrix, src/sqfa/linalg.py:19-45) without any (C,D,D)
// tensor:  F cov_c F^T = cov(F x | c),  F mu_c = mean(F x | c).  X is read once forward and once backward.
//
//   points (N,D) row-major; row_index (N) int64 or NULL and class_start (C+1) int64 as in class_moments_kernel.hip;
//   row_class (N) int64: the class of GROUPED row g (the sorted labels); means (C,D): sqfa_class_means.
//   zc (N,K): the centred features F (x - mu_class) in GROUPED order (row g belongs to points[row_index[g]]).
//
// Launches (caller's stream; nothing allocated, synchronised or read back; no atomics, every sum in a fixed order, every
// output element one writer: bitwise reproducible; every grid a function of (N, C, D, K) and n_groups alone):
//   class_project_kernel     A: one workgroup (4 waves) per 64 grouped rows.  Chunks of DC columns (64 float / 32 double)
//                            of x - mu (centred in the dtype BEFORE the product, the mean row of each row's own class)
//                            and of F are staged in LDS as [row][col]; wave w accumulates rows 16w..16w+15 x K on the exact
//                            MFMA (A[i][k] = xc[i][k], B[k][j] = F[j][k]); the next chunk's global loads are in flight
//                            during the MFMAs.  Pitch DC + 2: see CP_PITCH_A.
//   class_gram_kernel        B1: workgroup (class, split s): the raw Gram sum z z^T of the s-th share of the class's rows,
//                            16 x 16 tiles of the LOWER block triangle only, each written as computed and mirrored
//   class_feature_finish_kernel  B2: per class m = F mu (lane-strided sums, fixed shuffle tree), S = sum_s partial_s / (n - 1)
//                            in the order s = 0, 1, ..., noise on the diagonal, second = S + m m^T.  (i,j) and (j,i) are the
//                            same product chain, so S and second equal their transposes bit for bit.
//   class_weights_kernel     C: w_g = (G_c + G_c^T) z_g / (n_c - 1) per grouped row (zeros for n_c < 2), and, when the
//                            gradient of the feature means is given, C more "virtual rows" w_{N+c} = g_c (zeros for an
//                            empty class) whose point is the class mean itself
//   class_backward_kernel    D: workgroup (64-column stripe q, group p): sum over the virtual rows of group p of
//                            w_v (x_v - mu)^T (virtual rows >= N: w_v mu_c^T), 32 rows per chunk staged as [row][col],
//                            A[i][k] = w[k][i], B[k][j] = xc[k][j]; writes partial[p] (K, stripe).  The sum over p is the
//                            caller's (partial.sum(0) or sqfa_sphere_backward), as for sqfa_feature_scatters_backward.
// The shrunk entries (OAS: cov_c -> keep_c cov_c + shift_c I, the coefficients from sqfa_class_shrinkage) add one launch
// to each direction and run the kernels above with the coefficients:
//   filter_gram_kernel       forward, before B2: F F^T (K,K) once per call, one wave per element of the lower triangle
//                            (lane-strided sum over d, fixed shuffle tree), written at (i,j) and (j,i).  B2 then forms
//                            keep_c S + shift_c F F^T before the noise.
//   class_shrink_sum_kernel  backward, before C: H = sum over the classes with n_c >= 2 of shift_c (G_c + G_c^T), one
//                            workgroup per element (class-strided sums per thread, then a fixed tree).  C scales w_g by
//                            keep_c and appends K more virtual rows w_{N+C+k} = H[:,k] whose "point" in D is F[k,:]
//                            uncentred: D adds H F.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <type_traits>

#include "../../include/sqfa_hip.h"
#include "proj_traits.hpp"

namespace sqfa {

constexpr int CP_THREADS = 256;
constexpr int CP_KMAX = 64;        // filters
constexpr int CP_ROWS = 64;        // B: grouped rows per workgroup of kernel A
constexpr int CP_CHUNK = 32;       // rows per chunk of kernel D
constexpr int CP_STRIPE = 64;      // columns per workgroup of kernel D
constexpr int CP_GRAM_ROWS = 64;   // rows per chunk of kernel B1
constexpr int CP_MAX_SPLIT = 32;
// Tiles read with the ROW on the lane (kernel A: address (l & 15) * pitch + k + (l >> 4)): the 32 lanes of one LDS lane
// group are rows 0..15 x two consecutive k.  With pitch = 2 mod 32 elements they fall on banks 2 i + q (float) or on the
// bank pairs 4 i + 2 q, + 1 of the 64 (double, ds_read_b64): all distinct.
template <typename T> struct CpA {
  static constexpr int DC = 256 / (int)sizeof(T);   // columns per chunk: 64 float, 32 double
  static constexpr int PITCH = DC + 2;
};
// Tiles read with the COLUMN on the lane (kernels B1, D: address (k + (l >> 4)) * pitch + (l & 15)): rows k and k + 1 of
// one lane group must land on disjoint halves of the banks: pitch = 16 mod 32 elements, as class_moments_kernel.hip.
constexpr int CP_PITCH = 80;

__device__ __forceinline__ size_t cp_row(const long long* __restrict__ row_index, long long g) {
  return (size_t)(row_index != nullptr ? row_index[g] : g);
}

// A ROWS x COLS tile of rows given by pointer (sX[r], NULL = a row of zeros) minus, when CENTRE, the rows sM[r] (NULL = no
// centring), through registers into LDS as [row][col].  VEC: 16-byte loads (D % VW == 0, aligned bases); otherwise one
// element per load; the LDS image is the same.  Only the first rows_used rows (a multiple of RPP or more) are touched.
template <typename T, bool VEC, int ROWS, int COLS, int PITCH, bool CENTRE> struct TileLoad {
  using Tr = ProjTraits<T>;
  static constexpr int VW = VEC ? Tr::VW : 1;
  static constexpr int LPR = COLS / VW;              // threads across one row
  static constexpr int RPP = CP_THREADS / LPR;       // rows per pass
  static constexpr int PASSES = ROWS / RPP;
  static constexpr int PER = PASSES * VW;
  static_assert(CP_THREADS % LPR == 0 && ROWS % RPP == 0 && PASSES >= 1, "tile shape");
  T x[PER], m[CENTRE ? PER : 1];

  __device__ __forceinline__ void load(const T* const* sX, const T* const* sM, int D, int c0, int rows_used) {
    const int col = c0 + (threadIdx.x % LPR) * VW, r0 = threadIdx.x / LPR;
    const bool in = col < D;   // VEC: D % VW == 0, so a vector is inside or outside as a whole
#pragma unroll
    for (int p = 0; p < PASSES; ++p) {
      if (p * RPP < rows_used) {
        const int r = r0 + p * RPP;
        const T* xp = in ? sX[r] : nullptr;
        const T* mp = nullptr;
        if constexpr (CENTRE) mp = in ? sM[r] : nullptr;
        if constexpr (VEC) {
          typename Tr::Vec xv = {}, mv = {};
          if (xp != nullptr) xv = *reinterpret_cast<const typename Tr::Vec*>(xp + col);
          if (mp != nullptr) mv = *reinterpret_cast<const typename Tr::Vec*>(mp + col);
#pragma unroll
          for (int e = 0; e < VW; ++e) {
            x[p * VW + e] = xv[e];
            if constexpr (CENTRE) m[p * VW + e] = mv[e];
          }
        } else {
          x[p] = xp != nullptr ? xp[col] : (T)0;
          if constexpr (CENTRE) m[p] = mp != nullptr ? mp[col] : (T)0;
        }
      }
    }
  }

  // centred in the dtype; rows without a pointer and columns past D are exact zeros
  __device__ __forceinline__ void store(T* s, int rows_used) const {
    const int lc = (threadIdx.x % LPR) * VW, r0 = threadIdx.x / LPR;
#pragma unroll
    for (int p = 0; p < PASSES; ++p) {
      if (p * RPP < rows_used) {
        const int r = r0 + p * RPP;
#pragma unroll
        for (int e = 0; e < VW; ++e) {
          if constexpr (CENTRE)
            s[r * PITCH + lc + e] = x[p * VW + e] - m[p * VW + e];
          else
            s[r * PITCH + lc + e] = x[p * VW + e];
        }
      }
    }
  }
};

// ---- A: zc = (x - mu_class) F^T ------------------------------------------------------------------------------------------

template <typename T, bool VEC>
__global__ __launch_bounds__(CP_THREADS) void class_project_kernel(const T* __restrict__ points, long long N, int D,
                                                                   const long long* __restrict__ row_index,
                                                                   const long long* __restrict__ row_class,
                                                                   const T* __restrict__ means, const T* __restrict__ F,
                                                                   int K, T* __restrict__ zc) {
  using Tr = ProjTraits<T>;
  constexpr int DC = CpA<T>::DC, PA = CpA<T>::PITCH;
  __shared__ T sXt[CP_ROWS * PA], sFt[CP_KMAX * PA];
  __shared__ const T* sXp[CP_ROWS];
  __shared__ const T* sMp[CP_ROWS];
  __shared__ const T* sFp[CP_KMAX];
  const int tid = threadIdx.x, l = tid & 63, wave = tid >> 6, q = l >> 4;
  const long long g0 = (long long)blockIdx.x * CP_ROWS;
  const int KB = (K + 15) / 16, frows = KB * 16;
  if (tid < CP_ROWS) {
    const long long g = g0 + tid;
    const T* xp = nullptr;
    const T* mp = nullptr;
    if (g < N) {
      xp = points + cp_row(row_index, g) * (size_t)D;
      mp = means + (size_t)row_class[g] * D;
    }
    sXp[tid] = xp;
    sMp[tid] = mp;
    sFp[tid] = tid < K ? F + (size_t)tid * D : nullptr;
  }
  __syncthreads();
  TileLoad<T, VEC, CP_ROWS, DC, PA, true> ldX;
  TileLoad<T, VEC, CP_KMAX, DC, PA, false> ldF;
  typename Tr::Acc acc[4] = {};
  ldX.load(sXp, sMp, D, 0, CP_ROWS);
  ldF.load(sFp, nullptr, D, 0, frows);
  for (int c0 = 0; c0 < D; c0 += DC) {
    __syncthreads();   // the previous chunk has been consumed
    ldX.store(sXt, CP_ROWS);
    ldF.store(sFt, frows);
    __syncthreads();
    if (c0 + DC < D) {
      ldX.load(sXp, sMp, D, c0 + DC, CP_ROWS);
      ldF.load(sFp, nullptr, D, c0 + DC, frows);
    }
#pragma unroll
    for (int kk = 0; kk < DC; kk += 4) {
      const T a = sXt[(wave * 16 + (l & 15)) * PA + kk + q];
#pragma unroll
      for (int jb = 0; jb < 4; ++jb)
        if (jb < KB) acc[jb] = Tr::mfma(a, sFt[(jb * 16 + (l & 15)) * PA + kk + q], acc[jb]);
    }
  }
#pragma unroll
  for (int jb = 0; jb < 4; ++jb)
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const long long g = g0 + wave * 16 + Tr::acc_row(q, reg);
      const int col = jb * 16 + (l & 15);
      if (jb < KB && g < N && col < K) zc[(size_t)g * K + col] = acc[jb][reg];
    }
}

// ---- B1: the raw Gram sum of a share of one class's rows ---------------------------------------------------------------

// tile t of the lower block triangle -> (ti >= tj), row-major over the triangle (at most 10 tiles)
__device__ __forceinline__ void cp_tile_of(int t, int* ti, int* tj) {
  int i = 0;
  while ((i + 1) * (i + 2) / 2 <= t) ++i;
  *ti = i;
  *tj = t - i * (i + 1) / 2;
}

template <typename T>
__global__ __launch_bounds__(CP_THREADS) void class_gram_kernel(const T* __restrict__ zc,
                                                                const long long* __restrict__ class_start, int K,
                                                                int split, T* __restrict__ partial) {
  using Tr = ProjTraits<T>;
  __shared__ T sZ[CP_GRAM_ROWS * CP_PITCH];
  constexpr int PER = CP_GRAM_ROWS * CP_KMAX / CP_THREADS;   // 16
  const int c = blockIdx.x, s = blockIdx.y, tid = threadIdx.x, l = tid & 63, wave = tid >> 6, q = l >> 4;
  const long long start = class_start[c], n = class_start[c + 1] - start;
  const long long per = (n + split - 1) / split;
  const long long lo = (long long)s * per < n ? (long long)s * per : n, hi = lo + per < n ? lo + per : n;
  const long long rows = hi - lo;
  const int KB = (K + 15) / 16, ntile = KB * (KB + 1) / 2, chunk_elems = CP_GRAM_ROWS * K;
  const T* __restrict__ src = zc + (size_t)(start + lo) * K;   // the share's rows are contiguous: zc is in grouped order
  const long long total = rows * K;
  for (int i = tid; i < CP_GRAM_ROWS * CP_PITCH; i += CP_THREADS) sZ[i] = (T)0;   // columns K.. stay zero
  int ti[3], tj[3];
#pragma unroll
  for (int u = 0; u < 3; ++u) cp_tile_of(wave + 4 * u < ntile ? wave + 4 * u : 0, &ti[u], &tj[u]);
  typename Tr::Acc acc[3] = {};
  T v[PER];
  auto load = [&](long long k0) {
#pragma unroll
    for (int p = 0; p < PER; ++p) {
      const int idx = tid + p * CP_THREADS;
      const long long at = k0 * K + idx;
      v[p] = (idx < chunk_elems && at < total) ? src[at] : (T)0;
    }
  };
  if (rows > 0) load(0);
  for (long long k0 = 0; k0 < rows; k0 += CP_GRAM_ROWS) {
    __syncthreads();   // the previous chunk has been consumed (first pass: the zero fill is done)
#pragma unroll
    for (int p = 0; p < PER; ++p) {
      const int idx = tid + p * CP_THREADS;
      if (idx < chunk_elems) sZ[(idx / K) * CP_PITCH + idx % K] = v[p];
    }
    __syncthreads();
    if (k0 + CP_GRAM_ROWS < rows) load(k0 + CP_GRAM_ROWS);
#pragma unroll
    for (int kk = 0; kk < CP_GRAM_ROWS; kk += 4) {
#pragma unroll
      for (int u = 0; u < 3; ++u)
        if (wave + 4 * u < ntile)
          acc[u] = Tr::mfma(sZ[(kk + q) * CP_PITCH + ti[u] * 16 + (l & 15)], sZ[(kk + q) * CP_PITCH + tj[u] * 16 + (l & 15)],
                            acc[u]);
    }
  }
  T* out = partial + ((size_t)c * split + s) * K * K;
#pragma unroll
  for (int u = 0; u < 3; ++u)
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int i = ti[u] * 16 + Tr::acc_row(q, reg), j = tj[u] * 16 + (l & 15);
      if (wave + 4 * u < ntile && i < K && j < K) {
        out[i * K + j] = acc[u][reg];
        if (ti[u] != tj[u]) out[j * K + i] = acc[u][reg];   // the mirrored tile from the same values
      }
    }
}

// ---- shrunk forward: F F^T, once per call -------------------------------------------------------------------------------------

// wave (i, j <= i) of the lower triangle: sum_d F[i][d] F[j][d], lane-strided, fixed shuffle tree; one value, two stores
template <typename T>
__global__ __launch_bounds__(CP_THREADS) void filter_gram_kernel(const T* __restrict__ F, int D, int K,
                                                                 T* __restrict__ fft) {
  const int l = threadIdx.x & 63;
  const int t = blockIdx.x * (CP_THREADS / 64) + (threadIdx.x >> 6);   // wave-uniform
  if (t >= K * (K + 1) / 2) return;
  int i = 0;
  while ((i + 1) * (i + 2) / 2 <= t) ++i;
  const int j = t - i * (i + 1) / 2;
  const T* __restrict__ fi = F + (size_t)i * D;
  const T* __restrict__ fj = F + (size_t)j * D;
  T s = (T)0;
  for (int d = l; d < D; d += 64) s += fi[d] * fj[d];
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off);
  if (l == 0) {
    fft[i * K + j] = s;
    fft[j * K + i] = s;
  }
}

// ---- B2: feature means, covariance and second moment of one class --------------------------------------------------------

template <typename T>
__global__ __launch_bounds__(CP_THREADS) void class_feature_finish_kernel(const T* __restrict__ partial,
                                                                          const long long* __restrict__ class_start,
                                                                          const T* __restrict__ means,
                                                                          const T* __restrict__ F, int D, int K, int split,
                                                                          T noise, T* __restrict__ means_f,
                                                                          T* __restrict__ cov_f, T* __restrict__ second_f,
                                                                          const T* __restrict__ keep,
                                                                          const T* __restrict__ shift,
                                                                          const T* __restrict__ fft) {
  __shared__ T sM[CP_KMAX];
  const int c = blockIdx.x, tid = threadIdx.x, l = tid & 63, wave = tid >> 6;
  const double n = (double)(class_start[c + 1] - class_start[c]);
  const T* __restrict__ mu = means + (size_t)c * D;   // NaN for an empty class: so are m and everything below
  for (int k = wave; k < K; k += CP_THREADS / 64) {
    const T* __restrict__ f = F + (size_t)k * D;
    T s = (T)0;
    for (int d = l; d < D; d += 64) s += f[d] * mu[d];
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off);
    if (l == 0) {
      sM[k] = s;
      means_f[(size_t)c * K + k] = s;
    }
  }
  __syncthreads();
  const T* __restrict__ p = partial + (size_t)c * split * K * K;
  for (int e = tid; e < K * K; e += CP_THREADS) {
    T sum = p[e];
    for (int s = 1; s < split; ++s) sum += p[(size_t)s * K * K + e];
    T S = n < 1.0 ? (T)NAN : sum / (T)(n - 1.0);   // n = 1: 0/0 = NaN, as sqfa_class_moments
    const int i = e / K, j = e % K;
    if (keep != nullptr) {   // shrunk: the same chain at (i,j) and (j,i), fft symmetric bit for bit
      const T kept = keep[c] * S, shifted = shift[c] * fft[e];
      S = kept + shifted;
    }
    if (i == j) S += noise;
    cov_f[(size_t)c * K * K + e] = S;
    if (second_f != nullptr) {
      const T mm = sM[i] * sM[j];
      second_f[(size_t)c * K * K + e] = S + mm;
    }
  }
}

// ---- C: the backward weights of every virtual row -------------------------------------------------------------------------

template <typename T>
__global__ __launch_bounds__(CP_THREADS) void class_weights_kernel(const T* __restrict__ zc, long long N,
                                                                   const long long* __restrict__ row_class,
                                                                   const long long* __restrict__ class_start,
                                                                   const T* __restrict__ G, int ldg,
                                                                   const T* __restrict__ g_means, long long V, int K,
                                                                   T* __restrict__ w, int C,
                                                                   const T* __restrict__ keep,
                                                                   const T* __restrict__ H) {
  const long long e = (long long)blockIdx.x * CP_THREADS + threadIdx.x;
  if (e >= V * K) return;
  const long long v = e / K;
  const int a = (int)(e % K);
  T out = (T)0;
  if (v < N) {
    const long long c = row_class[v], n = class_start[c + 1] - class_start[c];
    if (n >= 2) {   // a class of one point has no covariance: it contributes nothing
      const T* __restrict__ Gc = G + (size_t)c * ldg * ldg;
      const T* __restrict__ z = zc + (size_t)v * K;
      T s = (T)0;
      for (int b = 0; b < K; ++b) s += (Gc[a * ldg + b] + Gc[b * ldg + a]) * z[b];
      out = s / (T)(n - 1);
      if (keep != nullptr) out = keep[c] * out;   // shrunk: cov_f holds keep_c times the sample covariance
    }
  } else if (v < N + C) {
    const long long c = v - N;
    if (g_means != nullptr && class_start[c + 1] - class_start[c] >= 1) out = g_means[(size_t)c * K + a];
  } else {
    out = H[(size_t)a * K + (v - N - C)];   // shrunk: filter row k = v - N - C carries the column H[:,k]
  }
  w[e] = out;
}

// ---- shrunk backward: H = sum_c shift_c (G_c + G_c^T) over the classes with a covariance --------------------------------

template <typename T>
__global__ __launch_bounds__(CP_THREADS) void class_shrink_sum_kernel(const T* __restrict__ G, int ldg,
                                                                      const long long* __restrict__ class_start,
                                                                      const T* __restrict__ shift, int C, int K,
                                                                      T* __restrict__ H) {
  __shared__ T sSum[CP_THREADS];
  const int e = blockIdx.x, a = e / K, b = e % K, tid = threadIdx.x;
  T s = (T)0;
  for (int c = tid; c < C; c += CP_THREADS) {
    if (class_start[c + 1] - class_start[c] >= 2) {   // by select: NaN in G and shift of the other classes is never read
      const T* __restrict__ Gc = G + (size_t)c * ldg * ldg;
      s += shift[c] * (Gc[a * ldg + b] + Gc[b * ldg + a]);
    }
  }
  sSum[tid] = s;
  __syncthreads();
  for (int off = CP_THREADS / 2; off > 0; off >>= 1) {
    if (tid < off) sSum[tid] += sSum[tid + off];
    __syncthreads();
  }
  if (tid == 0) H[e] = sSum[0];
}

// ---- D: partial[p] = sum over the virtual rows of group p of w (x - mu)^T ------------------------------------------------

// The body of both kernels D.  SHRUNK is a compile-time switch, not a NULL test on F: the float64 kernel sits at 256
// registers (two waves per SIMD), and the filter rows must not cost the empirical path a wave.
template <typename T, bool VEC, bool SHRUNK>
__device__ __forceinline__ void class_backward_body(const T* __restrict__ points, long long N, int D,
                                                    const long long* __restrict__ row_index,
                                                    const long long* __restrict__ row_class,
                                                    const long long* __restrict__ class_start, const T* __restrict__ means,
                                                    const T* __restrict__ w, int K, long long V, long long rows_per_group,
                                                    T* __restrict__ partial, int C, const T* __restrict__ F) {
  using Tr = ProjTraits<T>;
  __shared__ T sXt[CP_CHUNK * CP_PITCH], sWt[CP_CHUNK * CP_PITCH];
  __shared__ const T* sXp[2][CP_CHUNK];
  __shared__ const T* sMp[2][CP_CHUNK];
  constexpr int PER_W = CP_CHUNK * CP_KMAX / CP_THREADS;   // 8
  const int tid = threadIdx.x, l = tid & 63, wave = tid >> 6, q = l >> 4;
  const int c0 = blockIdx.x * CP_STRIPE, grp = blockIdx.y;
  const int KB = (K + 15) / 16, chunk_elems = CP_CHUNK * K;
  const long long v_lo = (long long)grp * rows_per_group < V ? (long long)grp * rows_per_group : V;
  const long long v_hi = v_lo + rows_per_group < V ? v_lo + rows_per_group : V;
  const long long w_end = v_hi * K;

  // the pointers of the rows v0 .. v0+31: a point and its class mean, or (v >= N) the mean of class v - N uncentred, or
  // (shrunk, v >= N + C) the filter v - N - C uncentred
  auto fill = [&](int buf, long long v0) {
    if (tid < CP_CHUNK) {
      const long long v = v0 + tid;
      const T* xp = nullptr;
      const T* mp = nullptr;
      if (v < v_hi) {
        if (v < N) {
          xp = points + cp_row(row_index, v) * (size_t)D;
          mp = means + (size_t)row_class[v] * D;
        } else {
          // one address expression for both kinds of row (filter k = v - N - C: F + k D = (F - C D) + (v - N) D): a branch
          // of its own for the filters costs the float64 kernel two registers and with them its second wave per SIMD
          const bool filter = SHRUNK && v >= N + C;
          const long long c = filter ? 0 : v - N;
          // an empty class's mean is NaN: a row of zeros
          if (filter || class_start[c + 1] - class_start[c] >= 1) xp = (filter ? F - (size_t)C * D : means) + (size_t)(v - N) * D;
        }
      }
      sXp[buf][tid] = xp;
      sMp[buf][tid] = mp;
    }
  };
  T wv[PER_W];
  auto load_w = [&](long long v0) {
#pragma unroll
    for (int p = 0; p < PER_W; ++p) {
      const int idx = tid + p * CP_THREADS;
      const long long at = v0 * K + idx;
      wv[p] = (idx < chunk_elems && at < w_end) ? w[at] : (T)0;
    }
  };

  for (int i = tid; i < CP_CHUNK * CP_PITCH; i += CP_THREADS) sWt[i] = (T)0;   // columns K.. stay zero
  fill(0, v_lo);
  __syncthreads();
  TileLoad<T, VEC, CP_CHUNK, CP_STRIPE, CP_PITCH, true> ld;
  typename Tr::Acc acc[4] = {};
  if (v_lo < v_hi) {
    ld.load(sXp[0], sMp[0], D, c0, CP_CHUNK);
    load_w(v_lo);
    fill(1, v_lo + CP_CHUNK);
  }
  int it = 0;
  for (long long v0 = v_lo; v0 < v_hi; v0 += CP_CHUNK, ++it) {
    __syncthreads();   // the previous chunk has been consumed; the pointers of the next one are visible
    ld.store(sXt, CP_CHUNK);
#pragma unroll
    for (int p = 0; p < PER_W; ++p) {
      const int idx = tid + p * CP_THREADS;
      if (idx < chunk_elems) sWt[(idx / K) * CP_PITCH + idx % K] = wv[p];
    }
    __syncthreads();
    if (v0 + CP_CHUNK < v_hi) {
      ld.load(sXp[(it + 1) & 1], sMp[(it + 1) & 1], D, c0, CP_CHUNK);
      load_w(v0 + CP_CHUNK);
      fill(it & 1, v0 + 2 * CP_CHUNK);   // read last by the loads of this chunk, issued before the barriers above
    }
#pragma unroll
    for (int kk = 0; kk < CP_CHUNK; kk += 4) {
      const T b = sXt[(kk + q) * CP_PITCH + wave * 16 + (l & 15)];
#pragma unroll
      for (int jb = 0; jb < 4; ++jb)
        if (jb < KB) acc[jb] = Tr::mfma(sWt[(kk + q) * CP_PITCH + jb * 16 + (l & 15)], b, acc[jb]);
    }
  }
  T* out = partial + (size_t)grp * K * D;
  const int d = c0 + wave * 16 + (l & 15);
#pragma unroll
  for (int jb = 0; jb < 4; ++jb)
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int k = jb * 16 + Tr::acc_row(q, reg);
      if (jb < KB && k < K && d < D) out[(size_t)k * D + d] = acc[jb][reg];
    }
}

template <typename T, bool VEC>
__global__ __launch_bounds__(CP_THREADS) void class_backward_kernel(const T* __restrict__ points, long long N, int D,
                                                                    const long long* __restrict__ row_index,
                                                                    const long long* __restrict__ row_class,
                                                                    const long long* __restrict__ class_start,
                                                                    const T* __restrict__ means, const T* __restrict__ w,
                                                                    int K, long long V, long long rows_per_group,
                                                                    T* __restrict__ partial) {
  class_backward_body<T, VEC, false>(points, N, D, row_index, row_class, class_start, means, w, K, V, rows_per_group, partial,
                                     0, nullptr);
}

// rows N + C .. N + C + K - 1 are the filters F[k,:] uncentred.  Two workgroups per CU asked for: without the bound the
// float64 instantiation takes 250 + 8 registers, two past the 256 of two waves per SIMD, and runs at half the occupancy.
template <typename T, bool VEC>
__global__ __launch_bounds__(CP_THREADS) void class_backward_shrunk_kernel(const T* __restrict__ points, long long N, int D,
                                                                           const long long* __restrict__ row_index,
                                                                           const long long* __restrict__ row_class,
                                                                           const long long* __restrict__ class_start,
                                                                           const T* __restrict__ means,
                                                                           const T* __restrict__ w, int K, long long V,
                                                                           long long rows_per_group, T* __restrict__ partial,
                                                                           int C, const T* __restrict__ F) {
  class_backward_body<T, VEC, true>(points, N, D, row_index, row_class, class_start, means, w, K, V, rows_per_group, partial, C,
                                    F);
}

// ---- host ------------------------------------------------------------------------------------------------------------------

struct CpLayout {
  int split;          // shares of a class in kernel B1
  size_t total;       // max(forward: Gram partials, backward: weights of the N + C virtual rows)
};

static bool cp_layout(long long N, int C, int D, int K, int dtype, CpLayout* w) {
  if (N < 0 || C < 1 || D < 1 || K < 1 || K > CP_KMAX || (dtype != SQFA_F32 && dtype != SQFA_F64)) return false;
  if (C > 65535) return false;   // as the class statistics: classes in grid.y of the mean kernel
  const long long V = N + C;
  if ((N + CP_ROWS - 1) / CP_ROWS > (long long)INT_MAX || (V * K + CP_THREADS - 1) / CP_THREADS > (long long)INT_MAX) return false;
  const size_t esz = dtype == SQFA_F32 ? 4 : 8;
  // a class of average size in shares of ~256 rows, and at least ~256 workgroups, but no share below 64 rows
  const long long avg = N / C;
  long long split = (avg + 255) / 256, fill = (256 + C - 1) / C, cap = (avg + 63) / 64;
  if (split < fill) split = fill;
  if (split > cap) split = cap;
  if (split > CP_MAX_SPLIT) split = CP_MAX_SPLIT;
  if (split < 1) split = 1;
  w->split = (int)split;
  const size_t fwd = (size_t)C * split * K * K * esz, bwd = (size_t)V * K * esz;
  w->total = fwd > bwd ? fwd : bwd;
  return true;
}

// The shrunk entries: F F^T (K,K) after the Gram partials forward; K more virtual rows and H (K,K) after them backward.
struct CpShrunkLayout {
  int split;
  size_t fft_off, h_off, total;
};

static bool cp_layout_shrunk(long long N, int C, int D, int K, int dtype, CpShrunkLayout* w) {
  CpLayout base;
  if (!cp_layout(N, C, D, K, dtype, &base)) return false;
  const long long V = N + C + K;
  if ((V * K + CP_THREADS - 1) / CP_THREADS > (long long)INT_MAX) return false;
  const size_t esz = dtype == SQFA_F32 ? 4 : 8;
  w->split = base.split;
  w->fft_off = (size_t)C * base.split * K * K * esz;
  w->h_off = (size_t)V * K * esz;
  const size_t fwd = w->fft_off + (size_t)K * K * esz, bwd = w->h_off + (size_t)K * K * esz;
  w->total = fwd > bwd ? fwd : bwd;
  return true;
}

template <typename T> static bool cp_vec(const void* points, const void* means, const void* F, int D) {
  return (D % ProjTraits<T>::VW) == 0 &&
         ((reinterpret_cast<size_t>(points) | reinterpret_cast<size_t>(means) | reinterpret_cast<size_t>(F)) & 15) == 0;
}

template <typename T>
static void run_feature_moments(const T* points, long long N, int D, const long long* row_index, const long long* row_class,
                                const long long* class_start, int C, const T* means, const T* F, int K, double noise,
                                T* zc, T* means_f, T* cov_f, T* second_f, char* ws, int split, hipStream_t stream,
                                const T* keep = nullptr, const T* shift = nullptr, T* fft = nullptr) {
  T* partial = reinterpret_cast<T*>(ws);
  if (N > 0) {
    const unsigned grid = (unsigned)((N + CP_ROWS - 1) / CP_ROWS);
    if (cp_vec<T>(points, means, F, D))
      class_project_kernel<T, true><<<grid, CP_THREADS, 0, stream>>>(points, N, D, row_index, row_class, means, F, K, zc);
    else
      class_project_kernel<T, false><<<grid, CP_THREADS, 0, stream>>>(points, N, D, row_index, row_class, means, F, K, zc);
  }
  class_gram_kernel<T><<<dim3(C, split), CP_THREADS, 0, stream>>>(zc, class_start, K, split, partial);
  if (keep != nullptr) {
    const int waves = K * (K + 1) / 2, per_block = CP_THREADS / 64;
    filter_gram_kernel<T><<<(waves + per_block - 1) / per_block, CP_THREADS, 0, stream>>>(F, D, K, fft);
  }
  class_feature_finish_kernel<T><<<C, CP_THREADS, 0, stream>>>(partial, class_start, means, F, D, K, split, (T)noise,
                                                               means_f, cov_f, second_f, keep, shift, fft);
}

template <typename T>
static void run_feature_backward(const T* points, long long N, int D, const long long* row_index, const long long* row_class,
                                 const long long* class_start, int C, const T* means, const T* zc, const T* G, int ldg,
                                 const T* g_means, int K, int n_groups, T* partial_out, char* ws, hipStream_t stream,
                                 const T* keep = nullptr, const T* shift = nullptr, const T* F = nullptr, T* H = nullptr) {
  T* wbuf = reinterpret_cast<T*>(ws);
  // shrunk: the class rows are always there (zeros without g_means), so that the filter rows start at N + C
  const long long V = keep != nullptr ? N + C + K : N + (g_means != nullptr ? C : 0);
  if (keep != nullptr) class_shrink_sum_kernel<T><<<K * K, CP_THREADS, 0, stream>>>(G, ldg, class_start, shift, C, K, H);
  if (V > 0)
    class_weights_kernel<T><<<(unsigned)((V * K + CP_THREADS - 1) / CP_THREADS), CP_THREADS, 0, stream>>>(
        zc, N, row_class, class_start, G, ldg, g_means, V, K, wbuf, C, keep, H);
  long long per = (V + n_groups - 1) / n_groups;
  per = (per + CP_CHUNK - 1) / CP_CHUNK * CP_CHUNK;
  const dim3 grid((D + CP_STRIPE - 1) / CP_STRIPE, n_groups);
  const bool vec = cp_vec<T>(points, means, F, D);
  if (keep != nullptr) {
    if (vec)
      class_backward_shrunk_kernel<T, true><<<grid, CP_THREADS, 0, stream>>>(points, N, D, row_index, row_class, class_start,
                                                                             means, wbuf, K, V, per, partial_out, C, F);
    else
      class_backward_shrunk_kernel<T, false><<<grid, CP_THREADS, 0, stream>>>(points, N, D, row_index, row_class, class_start,
                                                                              means, wbuf, K, V, per, partial_out, C, F);
  } else if (vec)
    class_backward_kernel<T, true><<<grid, CP_THREADS, 0, stream>>>(points, N, D, row_index, row_class, class_start, means,
                                                                    wbuf, K, V, per, partial_out);
  else
    class_backward_kernel<T, false><<<grid, CP_THREADS, 0, stream>>>(points, N, D, row_index, row_class, class_start, means,
                                                                     wbuf, K, V, per, partial_out);
}

// The plain and the shrunk entries over one implementation: `shrunk` selects the layout (cp_layout_shrunk) and asks for
// keep / shift (and F, backward); the plain entries pass nullptr for them.
static int feature_moments_impl(bool shrunk, const void* points, long long N, int D, const long long* row_index,
                                const long long* row_class, const long long* class_start, int C, const void* means,
                                const void* F, int K, int dtype, double noise, const void* keep, const void* shift,
                                void* zc_out, void* means_f_out, void* cov_f_out, void* second_f_out, void* workspace,
                                size_t workspace_bytes, void* stream_) {
  if (N < 0 || C < 1 || D < 1 || K < 1 || (N > 0 && (points == nullptr || row_class == nullptr || zc_out == nullptr)) ||
      class_start == nullptr || means == nullptr || F == nullptr || (shrunk && (keep == nullptr || shift == nullptr)) ||
      means_f_out == nullptr || cov_f_out == nullptr)
    return SQFA_ERR_BAD_ARGUMENT;
  if (dtype != SQFA_F32 && dtype != SQFA_F64) return SQFA_ERR_BAD_ARGUMENT;
  CpShrunkLayout w{};
  CpLayout plain;
  if (!(shrunk ? cp_layout_shrunk(N, C, D, K, dtype, &w) : cp_layout(N, C, D, K, dtype, &plain))) return SQFA_ERR_UNSUPPORTED_M;
  if (!shrunk) w.split = plain.split, w.total = plain.total;
  if (workspace == nullptr || workspace_bytes < w.total) return SQFA_ERR_WORKSPACE;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  char* ws = static_cast<char*>(workspace);
  auto run = [&](auto* element) {   // the dtype fork: called with a null float* / double*
    using T = std::remove_pointer_t<decltype(element)>;
    run_feature_moments(static_cast<const T*>(points), N, D, row_index, row_class, class_start, C, static_cast<const T*>(means),
                        static_cast<const T*>(F), K, noise, static_cast<T*>(zc_out), static_cast<T*>(means_f_out),
                        static_cast<T*>(cov_f_out), static_cast<T*>(second_f_out), ws, w.split, stream,
                        static_cast<const T*>(keep), static_cast<const T*>(shift),
                        shrunk ? reinterpret_cast<T*>(ws + w.fft_off) : nullptr);
  };
  if (dtype == SQFA_F32) run(static_cast<float*>(nullptr));
  else run(static_cast<double*>(nullptr));
  return hipGetLastError() == hipSuccess ? SQFA_OK : SQFA_ERR_LAUNCH;
}

static int feature_backward_impl(bool shrunk, const void* points, long long N, int D, const long long* row_index,
                                 const long long* row_class, const long long* class_start, int C, const void* means,
                                 const void* F, const void* zc, const void* G, int ldg, const void* g_means, const void* keep,
                                 const void* shift, int K, int dtype, int n_groups, void* partial_out, void* workspace,
                                 size_t workspace_bytes, void* stream_) {
  if (N < 0 || C < 1 || D < 1 || K < 1 || (N > 0 && (points == nullptr || row_class == nullptr || zc == nullptr)) ||
      class_start == nullptr || means == nullptr || G == nullptr ||
      (shrunk && (F == nullptr || keep == nullptr || shift == nullptr)) || ldg < K || n_groups < 1 || n_groups > 65535 ||
      partial_out == nullptr)
    return SQFA_ERR_BAD_ARGUMENT;
  if (dtype != SQFA_F32 && dtype != SQFA_F64) return SQFA_ERR_BAD_ARGUMENT;
  CpShrunkLayout w{};
  CpLayout plain;
  if (!(shrunk ? cp_layout_shrunk(N, C, D, K, dtype, &w) : cp_layout(N, C, D, K, dtype, &plain))) return SQFA_ERR_UNSUPPORTED_M;
  if (!shrunk) w.total = plain.total;
  if (workspace == nullptr || workspace_bytes < w.total) return SQFA_ERR_WORKSPACE;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  char* ws = static_cast<char*>(workspace);
  auto run = [&](auto* element) {   // the dtype fork: called with a null float* / double*
    using T = std::remove_pointer_t<decltype(element)>;
    run_feature_backward(static_cast<const T*>(points), N, D, row_index, row_class, class_start, C,
                         static_cast<const T*>(means), static_cast<const T*>(zc), static_cast<const T*>(G), ldg,
                         static_cast<const T*>(g_means), K, n_groups, static_cast<T*>(partial_out), ws, stream,
                         static_cast<const T*>(keep), static_cast<const T*>(shift), static_cast<const T*>(F),
                         shrunk ? reinterpret_cast<T*>(ws + w.h_off) : nullptr);
  };
  if (dtype == SQFA_F32) run(static_cast<float*>(nullptr));
  else run(static_cast<double*>(nullptr));
  return hipGetLastError() == hipSuccess ? SQFA_OK : SQFA_ERR_LAUNCH;
}

}  // namespace sqfa

extern "C" size_t sqfa_class_feature_moments_workspace_bytes(long long N, int C, int D, int K, int dtype) {
  sqfa::CpLayout w;
  if (!sqfa::cp_layout(N, C, D, K, dtype, &w)) return 0;
  return w.total < 16 ? 16 : w.total;
}

extern "C" int sqfa_class_feature_moments(const void* points, long long N, int D, const long long* row_index,
                                          const long long* row_class, const long long* class_start, int C,
                                          const void* means, const void* F, int K, int dtype, double noise, void* zc_out,
                                          void* means_f_out, void* cov_f_out, void* second_f_out, void* workspace,
                                          size_t workspace_bytes, void* stream_) {
  return sqfa::feature_moments_impl(false, points, N, D, row_index, row_class, class_start, C, means, F, K, dtype, noise,
                                    nullptr, nullptr, zc_out, means_f_out, cov_f_out, second_f_out, workspace,
                                    workspace_bytes, stream_);
}

extern "C" int sqfa_class_feature_moments_backward(const void* points, long long N, int D, const long long* row_index,
                                                   const long long* row_class, const long long* class_start, int C,
                                                   const void* means, const void* zc, const void* G, int ldg,
                                                   const void* g_means, int K, int dtype, int n_groups, void* partial_out,
                                                   void* workspace, size_t workspace_bytes, void* stream_) {
  return sqfa::feature_backward_impl(false, points, N, D, row_index, row_class, class_start, C, means, nullptr, zc, G, ldg,
                                     g_means, nullptr, nullptr, K, dtype, n_groups, partial_out, workspace, workspace_bytes,
                                     stream_);
}

// ---- the shrunk entries: cov_c -> keep_c cov_c + shift_c I in D-space (OAS; keep, shift from sqfa_class_shrinkage) ---------

extern "C" size_t sqfa_class_feature_moments_shrunk_workspace_bytes(long long N, int C, int D, int K, int dtype) {
  sqfa::CpShrunkLayout w;
  if (!sqfa::cp_layout_shrunk(N, C, D, K, dtype, &w)) return 0;
  return w.total < 16 ? 16 : w.total;
}

extern "C" int sqfa_class_feature_moments_shrunk(const void* points, long long N, int D, const long long* row_index,
                                                 const long long* row_class, const long long* class_start, int C,
                                                 const void* means, const void* F, int K, int dtype, double noise,
                                                 const void* keep, const void* shift, void* zc_out, void* means_f_out,
                                                 void* cov_f_out, void* second_f_out, void* workspace,
                                                 size_t workspace_bytes, void* stream_) {
  return sqfa::feature_moments_impl(true, points, N, D, row_index, row_class, class_start, C, means, F, K, dtype, noise, keep,
                                    shift, zc_out, means_f_out, cov_f_out, second_f_out, workspace, workspace_bytes, stream_);
}

extern "C" int sqfa_class_feature_moments_shrunk_backward(const void* points, long long N, int D, const long long* row_index,
                                                          const long long* row_class, const long long* class_start, int C,
                                                          const void* means, const void* F, const void* zc, const void* G,
                                                          int ldg, const void* g_means, const void* keep, const void* shift,
                                                          int K, int dtype, int n_groups, void* partial_out, void* workspace,
                                                          size_t workspace_bytes, void* stream_) {
  return sqfa::feature_backward_impl(true, points, N, D, row_index, row_class, class_start, C, means, F, zc, G, ldg, g_means,
                                     keep, shift, K, dtype, n_groups, partial_out, workspace, workspace_bytes, stream_);
}
