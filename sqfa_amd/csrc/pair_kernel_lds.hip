// pair_kernel_lds.hip -- the affine-invariant pair path for matrix sizes 64 < m <= 128 (gfx950).
//
// Past m = 64 the register-resident lane groups of pair_kernel.hpp no longer fit: one pair's matrix lives in LDS and a
// whole workgroup works on it ("K0L / K1L").  Padded size MR = round_up(m, 8) is a RUN-TIME value:
// one instantiation per element type (and per backward kind) covers every size of the range.
//
//   K0L  cholesky_lds_kernel   per class, in double: L (written as LT, columns contiguous, identity padded to MR), L^-1
//                              (packed lower triangle, as PairCfg::PACK_LINV), and -- first launch only -- the slab slot
//                              table row_start that finalize_kernel (K2) reads.
//   K1L  pair_lds_kernel       one workgroup per tile of TI x tj pairs, the pairs one after the other:
//        1. X = L_j^-1 L_i built in LDS, one thread per column (column-major, pitch MR + 1)
//        2. one-sided Jacobi on the columns of X, round-robin ordering: step s pairs columns (s + k, s - k) mod (MR - 1)
//           and (s, MR - 1); MR / 2 disjoint rotations per step, 4 lanes per rotation (rows split over the lanes), one
//           workgroup barrier per step.  Rotation test and sweep cap as the register kernels (tol2, early2, SQFA_MAX_SWEEPS).
//        3. lambda_k = |y_k|^2 (columns in place: eig_out's order), d2, D, loss, {NaN, inf}
//        4. backward: Z = L_j^-T Y in place (one thread per column), then for every lower-triangle entry (r, c)
//           sum_k Z_rk Z_ck cA_k (A side) and sum_k Z_rk Z_ck cB_k (B side) added to this tile's slab rows.  The
//           workgroup owns its slab rows and a thread always handles the same entries: read-add-write, no atomics,
//           deterministic.
//   K2 (finalize_kernel, sqfa_api.hip) reduces the slab unchanged.
#include <hip/hip_runtime.h>

#include "pair_kernel.hpp"
#include "pair_kernel_lds.hpp"

namespace sqfa {

namespace {

constexpr int kRowsPerLane = kLdsMaxDim / 4;  // rows of a column one of the 4 lanes of a rotation holds

// 1/sqrt(x) in double: hardware estimate + 2 Newton steps (as the Cholesky prologue of the register path)
__device__ __forceinline__ double rsqrt_nr(double x) {
  double y = __builtin_amdgcn_rsq(x);
  y = y * (1.5 - 0.5 * x * y * y);
  y = y * (1.5 - 0.5 * x * y * y);
  return y;
}

// sum over the 4 lanes of a rotation (every lane gets the same bits: the butterfly adds commute)
template <typename T> __device__ __forceinline__ T quad_sum(T v) {
  v += __shfl_xor(v, 1, 64);
  v += __shfl_xor(v, 2, 64);
  return v;
}

// sum over the workgroup in a fixed order (deterministic); red: one slot per wave; every thread gets the total
template <typename T> __device__ __forceinline__ T block_sum(T v, T* red) {
  v = wave_sum(v);
  const int wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[wave] = v;
  __syncthreads();
  T t = T(0);
  for (int w = 0; w < nw; ++w) t += red[w];
  return t;
}

// ---- K0L ------------------------------------------------------------------------------------------------------------
// One 256-thread workgroup per class; a[m][m+1] doubles in dynamic LDS (132 KB at m = 128).  Right-looking elimination
// on the unscaled columns (one barrier per pivot, as cholesky_kernel), columns scaled by 1/sqrt(pivot) at the end.  The
// inverse X = L^-1 is formed row by row IN PLACE: its strict lower triangle is stored transposed in the (unused) upper
// triangle of a, X[r][c] at a[c][r], its diagonal 1/L[r][r] in rd.  Two lanes per column, both in one wave.
// A non-SPD class yields NaN pivots and NaN factors, which surface as non-finite distances; never a fault.
template <typename T>
__global__ __launch_bounds__(256) void cholesky_lds_kernel(const T* __restrict__ S, int m, int MR, T* __restrict__ LT,
                                                           T* __restrict__ Linv, int* __restrict__ row_start, PairParams pp,
                                                           int TI) {
  if (row_start != nullptr && blockIdx.x == 0) write_row_start_table(pp, TI, row_start);
  extern __shared__ double lds_chol[];
  const int P = m + 1;
  double* a = lds_chol;           // a[r * P + c]
  double* rd = lds_chol + m * P;  // 1 / L[k][k]
  const int c = blockIdx.x, t = threadIdx.x;
  const T* s = S + (size_t)c * m * m;
  for (int idx = t; idx < m * m; idx += 256) a[(idx / m) * P + idx % m] = (double)s[idx];
  __syncthreads();
  for (int k = 0; k < m; ++k) {
    const double akk = a[k * P + k];
    double rk = __builtin_amdgcn_rcp(akk);
    rk = rk * (2.0 - akk * rk);
    rk = rk * (2.0 - akk * rk);
    if (!(akk > 0.0)) rk = __builtin_nan("");
    const int n = m - k - 1;
    for (int e = t; e < n * n; e += 256) {
      const int r = k + 1 + e / n, c2 = k + 1 + e % n;
      if (c2 <= r) a[r * P + c2] -= a[r * P + k] * a[c2 * P + k] * rk;
    }
    __syncthreads();
  }
  for (int k = t; k < m; k += 256) rd[k] = rsqrt_nr(a[k * P + k]);
  __syncthreads();
  for (int e = t; e < m * m; e += 256) {
    const int r = e / m, k = e % m;
    if (k <= r) a[r * P + k] *= rd[k];
  }
  __syncthreads();
  if (LT != nullptr) {
    T* lt = LT + (size_t)c * MR * MR;
    for (int idx = t; idx < MR * MR; idx += 256) {
      const int col = idx / MR, k = idx % MR;  // LT[col][k] = L[k][col]
      const double v = (col < m && k < m) ? (k >= col ? a[k * P + col] : 0.0) : (col == k ? 1.0 : 0.0);
      lt[idx] = (T)v;
    }
  }
  if (Linv == nullptr) return;
  {
    const int col = t >> 1, part = t & 1;
    for (int r = 1; r < m; ++r) {
      double acc = 0.0;
      if (col < r) {
        for (int k = col + part; k < r; k += 2) acc += a[r * P + k] * (k == col ? rd[col] : a[col * P + k]);
      }
      acc += __shfl_xor(acc, 1, 64);
      if (part == 0 && col < r) a[col * P + r] = -acc * rd[r];
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
    }
  }
  __syncthreads();
  T* li = Linv + (size_t)c * (MR * (MR + 1) / 2);
  for (int r = 0; r < MR; ++r) {
    for (int k = t; k <= r; k += 256) {
      const double v = (r < m) ? (k == r ? rd[r] : a[k * P + r]) : (k == r ? 1.0 : 0.0);
      li[tri_index(r, k)] = (T)v;
    }
  }
}

// ---- K1L ------------------------------------------------------------------------------------------------------------
// BW: the Bures-Wasserstein distance (sqfa_bw_pairwise), as pair_tile_kernel's BW (pair_kernel.hpp); LinvAll then holds R_j
template <typename T, bool EIG_BWD, bool BW = false>
__global__ __launch_bounds__(256) void pair_lds_kernel(const PairParams p, int TI, int MR, const T* __restrict__ LT,
                                                       const T* __restrict__ LinvAll, const T* __restrict__ Wt,
                                                       const T* __restrict__ EWt) {
  using R = Real<T>;
  extern __shared__ __align__(16) unsigned char lds_pair[];
  const int P = MR + 1;
  T* X = reinterpret_cast<T*>(lds_pair);  // column c of X at X + c * P
  T* s_lam = X + MR * P;
  T* s_cA = s_lam + MR;
  T* s_cB = s_cA + MR;
  T* s_red = s_cB + MR;  // one slot per wave
  const int nt = blockDim.x, tid = threadIdx.x;
  const int TRI = MR * (MR + 1) / 2, m = p.m, tj = p.tj;

  // my tile: the blockIdx.x-th tile of this shard in the compact grid (pair_kernel.hpp, tiles_in_row)
  int bi = 0, bj = 0;
  {
    int w = blockIdx.x;
    for (; bi < p.nbi; ++bi) {
      int first;
      const int cnt = shard_tiles_in_row(bi, tiles_in_row(bi, p.nbj, TI, tj, p.self_mode), p.shard_index,
                                         p.shard_count, &first);
      if (w < cnt) {
        bj = first + w * p.shard_count;
        break;
      }
      w -= cnt;
    }
    if (bi >= p.nbi) return;  // cannot happen for a grid sized by launch_pair_lds
  }
  const int i0 = bi * TI, j0 = bj * tj, tile = blockIdx.x;
  T* slab = p.want_grad ? static_cast<T*>(p.slab_grad) + (size_t)tile * (TI + tj) * TRI : nullptr;
  if (p.want_grad) {  // every slab row of the tile is defined; entry idx is always handled by thread idx % nt
    for (int row = 0; row < TI + tj; ++row)
      for (int idx = tid; idx < TRI; idx += nt) slab[(size_t)row * TRI + idx] = T(0);
    if constexpr (BW) {
      if (tid == 0)
        for (int jj = 0; jj < tj; ++jj) static_cast<T*>(p.slab_h)[(size_t)tile * tj + jj] = T(0);
    }
  }

  const T tol2 = R::kEps * R::kEps * T(MR);
  const T early2 = R::template early2<kLdsMaxDim>();
  const T scale = param_scale<T>(p), eps = param_eps<T>(p);
  const int half = MR / 2, grp = tid >> 2, q4 = tid & 3, cyc = MR - 1;
  T loss_acc = T(0);  // thread 0 only
  int n_nan = 0, n_inf = 0;

  for (int jj = 0; jj < tj; ++jj) {
    const int j = j0 + jj;
    if (j >= p.nB) break;
    const T* __restrict__ li = LinvAll + (size_t)j * TRI;
    for (int ii = 0; ii < TI; ++ii) {
      const int i = i0 + ii;
      if (i >= p.nA) break;
      if (p.self_mode && i <= j) continue;

      // ---- 1. X = L_j^-1 L_i: thread c owns column c; rows in descending order read no overwritten entry ----
      __syncthreads();  // the previous pair is done with X
      if (tid < MR) {
        T* xc = X + tid * P;
        const T* __restrict__ lt = LT + (size_t)i * MR * MR + (size_t)tid * MR;
        for (int k = 0; k < MR; ++k) xc[k] = lt[k];
        for (int r = MR - 1; r >= 0; --r) {
          const T* __restrict__ lr = li + tri_index(r, 0);  // same address in every lane
          if constexpr (BW && sizeof(T) == 4) {
            // BW float32: X = R_j F_i accumulated in double -- its rounding enters sum sigma_k directly (at m = 128 the
            // float32 sum put the distance at 1.3e-5 of the float64 value)
            double accd = 0.0;
            for (int k = 0; k <= r; ++k) accd = fma((double)lr[k], (double)xc[k], accd);
            xc[r] = (T)accd;
            continue;
          }
          T acc = T(0);
          for (int k = 0; k <= r; ++k) acc = R::fma_(lr[k], xc[k], acc);
          xc[r] = acc;
        }
      }
      __syncthreads();
      // BW: |X|_F^2 before the sweeps, in double (s_cA as reduction slots: not written before step 4).  The rotations preserve
      // it exactly in exact arithmetic; their float32 rounding drifts every column norm alike by ~1e-5 over ~10 sweeps of
      // MR - 1 steps, which the BW distance (sum sigma_k, not a log) would show directly -- step 3 rescales by the ratio.
      // The real columns are also scaled by a power of two (exact) to |X|_F^2 ~ m: the rotation test compares squared inner
      // products with eps^2 MR |x|^2 |y|^2, which underflows float32 for classes of size 1e-6 and stopped the sweeps early.
      double fro0 = 0.0, xs = 1.0;
      if constexpr (BW && sizeof(T) == 4) {
        double v = 0.0;
        if (tid < m) {
          const T* xc = X + tid * P;
          for (int r = 0; r < MR; ++r) v = fma((double)xc[r], (double)xc[r], v);
        }
        fro0 = block_sum(v, reinterpret_cast<double*>(s_cA));
        xs = exp2(rint(-0.5 * log2(fro0 / (double)m)));
        if (!(xs > 0.0 && xs < 1e30)) xs = 1.0;  // zero / non-finite classes: leave as they are
        fro0 *= xs * xs;
        if (tid < m) {
          T* xc = X + tid * P;
          for (int r = 0; r < MR; ++r) xc[r] *= (T)xs;
        }
        __syncthreads();
      }

      // ---- 2. one-sided Jacobi, round-robin ordering --------------------------------------------------------------
      int sweeps = 0;
      bool more = true;
      while (more && sweeps < SQFA_MAX_SWEEPS) {
        bool big = false;
        for (int s = 0; s < cyc; ++s) {
          if (grp < half) {
            int ca = s, cb = cyc;
            if (grp > 0) {
              ca = s + grp;
              if (ca >= cyc) ca -= cyc;
              cb = s - grp;
              if (cb < 0) cb += cyc;
            }
            T* xa = X + ca * P;
            T* xb = X + cb * P;
            T va[kRowsPerLane], vb[kRowsPerLane];
            T al = T(0), be = T(0), ga = T(0);
#pragma unroll
            for (int q = 0; q < kRowsPerLane; ++q) {
              const int r = q4 + 4 * q;
              va[q] = r < MR ? xa[r] : T(0);
              vb[q] = r < MR ? xb[r] : T(0);
              al = R::fma_(va[q], va[q], al);
              be = R::fma_(vb[q], vb[q], be);
              ga = R::fma_(va[q], vb[q], ga);
            }
            al = quad_sum(al);
            be = quad_sum(be);
            ga = quad_sum(ga);
            const T g2 = ga * ga, ab = al * be;
            big = big || (g2 > early2 * ab);
            if (g2 > tol2 * ab) {
              // zeta = cot 2 theta;  t = tan theta = sign(zeta) / (|zeta| + sqrt(1 + zeta^2))
              const T zeta = (be - al) / (T(2) * ga);
              const T az = R::abs_(zeta);
              const T tt = az > T(1) ? T(1) / (az * (T(1) + R::sqrt_(T(1) + T(1) / (az * az))))
                                     : T(1) / (az + R::sqrt_(T(1) + az * az));
              const T tn = R::copysign_(tt, zeta);
              const T cs = T(1) / R::sqrt_(T(1) + tn * tn), sn = cs * tn;
#pragma unroll
              for (int q = 0; q < kRowsPerLane; ++q) {
                const int r = q4 + 4 * q;
                if (r < MR) {
                  xa[r] = R::fma_(cs, va[q], -sn * vb[q]);
                  xb[r] = R::fma_(sn, va[q], cs * vb[q]);
                }
              }
            }
          }
          __syncthreads();
        }
        more = __syncthreads_or(big) != 0;
        ++sweeps;
      }
      if (p.sweep_counter != nullptr && tid == 0) {
        atomicAdd(&p.sweep_counter[0], (unsigned long long)sweeps);
        atomicAdd(&p.sweep_counter[1], 1ULL);
      }

      // ---- 3. eigenvalues, distance -------------------------------------------------------------------------------
      T part = T(0);
      if (tid < MR) {
        const T* xc = X + tid * P;
        T a = T(0);
        for (int r = 0; r < MR; ++r) a = R::fma_(xc[r], xc[r], a);
        const bool real_col = tid < m;  // identity-padded columns carry no signal
        const T lam = real_col ? (BW ? R::sqrt_(a) : a) : (BW ? T(0) : T(1));  // BW: sigma_k
        s_lam[tid] = lam;
        const T ll = real_col ? R::log_(lam) : T(0);
        part = BW ? lam : ll * ll;
      }
      double bw_sum = 0.0;  // BW: sum sigma_k in double (s_cA, not yet written for this pair, as the reduction slots)
      if constexpr (BW) {
        if constexpr (sizeof(T) == 4) {
          // the column norms in double, rescaled so that sum |y_k|^2 = |X|_F^2 of the unrotated X (see fro0)
          double ad = 0.0;
          if (tid < m) {
            T* xc = X + tid * P;
            for (int r = 0; r < MR; ++r) ad = fma((double)xc[r], (double)xc[r], ad);
            for (int r = 0; r < MR; ++r) xc[r] *= (T)(1.0 / xs);  // back to the true scale (exact) for step 4
          }
          const double corr = sqrt(fro0 / block_sum(ad, reinterpret_cast<double*>(s_cA))) / xs;
          const double sg = tid < m ? sqrt(ad) * corr : 0.0;
          if (tid < m) s_lam[tid] = (T)sg;
          bw_sum = block_sum(sg, reinterpret_cast<double*>(s_cA));
        } else {
          bw_sum = block_sum((double)part, reinterpret_cast<double*>(s_cA));
        }
      }
      const T d2 = BW ? T(p.trA[i] + p.trB[j] - 2.0 * bw_sum) : scale * block_sum(part, s_red);
      const T dist = p.sqrt_mode ? R::sqrt_((BW ? R::abs_(d2) : d2) + eps) : d2;
      if constexpr (BW) __syncthreads();  // every thread has read the reduction slots before step 4 writes s_cA
      T w;
      if (Wt != nullptr) {
        w = Wt[(size_t)i * p.nB + j];
        if (p.self_mode) w += Wt[(size_t)j * p.nB + i];
      } else {
        w = param_uniform_weight<T>(p);
      }
      if (tid == 0) {
        loss_acc += w * dist;
        n_nan += dist != dist;
        n_inf += dist == dist && !R::finite(dist);
        if (p.dist_out != nullptr) {
          T* D = static_cast<T*>(p.dist_out);
          D[(size_t)i * p.nB + j] = dist;
          if (p.self_mode) D[(size_t)j * p.nB + i] = dist;
        }
      }
      if (p.eig_out != nullptr && tid < m) {  // s_lam[tid] was written by this thread
        T* E = static_cast<T*>(p.eig_out);
        E[((size_t)i * p.nB + j) * m + tid] = s_lam[tid];
        if (p.self_mode) E[((size_t)j * p.nB + i) * m + tid] = T(1) / s_lam[tid];
      }

      // ---- 4. backward --------------------------------------------------------------------------------------------
      if (!p.want_grad) continue;
      T hc = T(0);  // BW: h = w dD/dbw2 (the same value in every thread)
      if constexpr (BW) {
        const T sg = d2 > T(0) ? T(1) : (d2 < T(0) ? T(-1) : T(0));
        hc = p.sqrt_mode ? w * sg * (T(0.5) / dist) : w;
        if (tid == 0) static_cast<T*>(p.slab_h)[(size_t)tile * tj + jj] += hc;
        // B side on y itself, before the back-transform (pair_tile_kernel): -h sum sigma^-1 y y^T, sandwiched by R_j^-1 after
        // the slab reduction
        if (tid < m) s_cB[tid] = -(hc / s_lam[tid]);
        __syncthreads();
        T* gbw = slab + (size_t)(TI + jj) * TRI;
        for (int idx = tid; idx < TRI; idx += nt) {
          int r = (int)((sqrtf(8.0f * (float)idx + 1.0f) - 1.0f) * 0.5f);
          while (tri_index(r, 0) > idx) --r;
          while (tri_index(r + 1, 0) <= idx) ++r;
          const int c = idx - tri_index(r, 0);
          if (r >= m) continue;
          T sb = T(0);
          for (int k = 0; k < m; ++k) sb = R::fma_(X[k * P + r] * X[k * P + c], s_cB[k], sb);
          gbw[idx] += sb;
        }
        __syncthreads();  // y is read before the back-transform overwrites it
      }
      if (tid < m) {
        const T lam = s_lam[tid];
        T cA, cB;
        if constexpr (EIG_BWD) {
          // d lambda_k/dA = u~ u~^T / lambda_k, d lambda_k/dB = -u~ u~^T; self mode also carries eig[j,i,k] = 1/lambda_k
          T wk = EWt[((size_t)i * p.nB + j) * m + tid];
          if (p.self_mode) wk -= EWt[((size_t)j * p.nB + i) * m + tid] / (lam * lam);
          cB = -wk;
          cA = wk / lam;
        } else {
          const T dd = p.sqrt_mode ? T(0.5) / dist : T(1);
          const T q = w * dd * scale * T(2) * R::log_(lam) / lam;
          cB = -q;
          cA = q / lam;
        }
        if constexpr (BW) {
          // sigma_k^-3 on u~ u~^T (pair_tile_kernel's BW coefficients); the B side is already in the slab
          const T rs = T(1) / lam;
          cB = T(0);
          cA = -(hc * rs) * (rs * rs);
        }
        s_cA[tid] = cA;
        s_cB[tid] = cB;
        // u~_k = L_j^-T y_k in place, rows ascending (row r reads rows q >= r only); rows >= m stay zero
        T* xc = X + tid * P;
        for (int r = 0; r < m; ++r) {
          T acc = T(0);
          for (int q = r; q < m; ++q) acc = R::fma_(li[tri_index(q, r)], xc[q], acc);
          xc[r] = acc;
        }
      }
      __syncthreads();
      T* ga = slab + (size_t)ii * TRI;
      T* gb = slab + (size_t)(TI + jj) * TRI;
      for (int idx = tid; idx < TRI; idx += nt) {
        int r = (int)((sqrtf(8.0f * (float)idx + 1.0f) - 1.0f) * 0.5f);
        while (tri_index(r, 0) > idx) --r;
        while (tri_index(r + 1, 0) <= idx) ++r;
        const int c = idx - tri_index(r, 0);
        if (r >= m) continue;  // padded entries: left at zero
        T sa = T(0), sb = T(0);
        for (int k = 0; k < m; ++k) {
          const T zz = X[k * P + r] * X[k * P + c];
          sa = R::fma_(zz, s_cA[k], sa);
          sb = R::fma_(zz, s_cB[k], sb);
        }
        if constexpr (BW) {
          if (r == c) sa += hc;  // identity term of the A side
        }
        ga[idx] += sa;
        if constexpr (!BW) gb[idx] += sb;
      }
    }
  }

  if (tid == 0) {
    static_cast<T*>(p.slab_loss)[tile] = loss_acc;
    p.slab_flag[2 * tile] = n_nan;
    p.slab_flag[2 * tile + 1] = n_inf;
  }
}

// dynamic LDS beyond the default limit must be allowed per kernel (the exact size: static + dynamic <= 160 KiB)
template <typename K> hipError_t allow_lds(K kernel, size_t bytes) {
  if (bytes <= 64 * 1024) return hipSuccess;
  return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

template <typename T>
hipError_t launch_prologue_t(const void* S, int n, int m, int MR, void* LT, void* Linv, int* row_start, const PairParams& p,
                             int TI, hipStream_t stream) {
  const size_t lds = ((size_t)m * (m + 1) + m) * sizeof(double);
  hipError_t e = allow_lds(cholesky_lds_kernel<T>, lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(cholesky_lds_kernel<T>, dim3(n), dim3(256), lds, stream, static_cast<const T*>(S), m, MR,
                     static_cast<T*>(LT), static_cast<T*>(Linv), row_start, p, TI);
  return hipGetLastError();
}

template <typename T>
hipError_t launch_pair_bw_t(const PairParams& p, int TI, int MR, hipStream_t stream) {
  long n_tiles = 0;
  for (int bi = 0; bi < p.nbi; ++bi) {
    int first;
    n_tiles += shard_tiles_in_row(bi, tiles_in_row(bi, p.nbj, TI, p.tj, p.self_mode), p.shard_index, p.shard_count, &first);
  }
  if (n_tiles == 0) return hipSuccess;
  const int threads = lds_pair_threads(MR);
  const size_t lds = lds_pair_shared_bytes(MR, sizeof(T));
  hipError_t e = allow_lds(pair_lds_kernel<T, false, true>, lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((pair_lds_kernel<T, false, true>), dim3((unsigned)n_tiles), dim3(threads), lds, stream, p, TI, MR,
                     static_cast<const T*>(p.LT), static_cast<const T*>(p.Linv), static_cast<const T*>(p.W),
                     static_cast<const T*>(nullptr));
  return hipGetLastError();
}

template <typename T>
hipError_t launch_pair_t(const PairParams& p, int TI, int MR, hipStream_t stream) {
  long n_tiles = 0;
  for (int bi = 0; bi < p.nbi; ++bi) {
    int first;
    n_tiles += shard_tiles_in_row(bi, tiles_in_row(bi, p.nbj, TI, p.tj, p.self_mode), p.shard_index, p.shard_count, &first);
  }
  if (n_tiles == 0) return hipSuccess;  // this shard owns no tile
  const int threads = lds_pair_threads(MR);
  const size_t lds = lds_pair_shared_bytes(MR, sizeof(T));
  const T* LT = static_cast<const T*>(p.LT);
  const T* Li = static_cast<const T*>(p.Linv);
  const T* W = static_cast<const T*>(p.W);
  const T* EW = static_cast<const T*>(p.EW);
  hipError_t e = p.EW != nullptr ? allow_lds(pair_lds_kernel<T, true>, lds) : allow_lds(pair_lds_kernel<T, false>, lds);
  if (e != hipSuccess) return e;
  if (p.EW != nullptr)
    hipLaunchKernelGGL((pair_lds_kernel<T, true>), dim3((unsigned)n_tiles), dim3(threads), lds, stream, p, TI, MR, LT, Li, W, EW);
  else
    hipLaunchKernelGGL((pair_lds_kernel<T, false>), dim3((unsigned)n_tiles), dim3(threads), lds, stream, p, TI, MR, LT, Li, W, EW);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_lds_prologue(int dtype_f64, const void* S, int n, int m, int MR, void* LT, void* Linv, int* row_start,
                               const PairParams& p, int TI, hipStream_t stream) {
  return dtype_f64 ? launch_prologue_t<double>(S, n, m, MR, LT, Linv, row_start, p, TI, stream)
                   : launch_prologue_t<float>(S, n, m, MR, LT, Linv, row_start, p, TI, stream);
}

hipError_t launch_pair_lds(int dtype_f64, const PairParams& p, int TI, int MR, hipStream_t stream) {
  return dtype_f64 ? launch_pair_t<double>(p, TI, MR, stream) : launch_pair_t<float>(p, TI, MR, stream);
}

hipError_t launch_pair_lds_bw(int dtype_f64, const PairParams& p, int TI, int MR, hipStream_t stream) {
  return dtype_f64 ? launch_pair_bw_t<double>(p, TI, MR, stream) : launch_pair_bw_t<float>(p, TI, MR, stream);
}

}  // namespace sqfa
