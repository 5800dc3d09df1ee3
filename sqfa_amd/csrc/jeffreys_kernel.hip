// jeffreys_kernel.hip -- fused closure loss of the Jeffreys divergence (the symmetric Kullback-Leibler divergence) between
// the n class Gaussians N(mu_c, Sigma_c), as the distance_fun of SQFA (with means) and SecondMomentsSQFA (mu == NULL):
// with the precisions P_c = Sigma_c^-1 and delta = mu_i - mu_j
//     J_ij = KL(i||j) + KL(j||i) = -1/2 <P_i - P_j, Sigma_i - Sigma_j> + 1/2 delta^T (P_i + P_j) delta
//     D_ij = J_ij  |  sqrt(J_ij + eps),  J_ij clamped at 0 from below,   loss = sum_{i>j} w_ij D_ij
// and its gradient wrt mu and Sigma.  The explicit-difference form is the one computed: the textbook form
// 1/2 [tr(P_j Sigma_i) + tr(P_i Sigma_j) - 2m] cancels the digits that matter for close classes (the same rule
// log_euclidean_kernel.hip follows).  A pair costs O(m^2): no per-pair factorisation.
//
// Three stages on the caller's stream:
//   1. spd_inverse_kernel (spd_class.hip, the per-class factor stage shared with stein_kernel.hip): P_c by Cholesky and
//      in-place triangular inverse, one 64-thread workgroup per class, double inside; P_c is written in the dtype, exactly
//      symmetric (one value per unordered index pair).  A pivot that is not positive gives a NaN matrix.
//   2. jeffreys_pair_kernel: an N-body pass over the ordered pairs.  A 256-thread workgroup owns TI classes i; every class has
//      NS lane groups of G lanes (TI NS G = 256, a group never leaves its wave).  Lane r of a group holds index r of the
//      symmetric matrices: the MMAX entries (c, r) of Sigma_i and P_i, and as many accumulators of
//          GSigma_i = sum_j -c_ij/2 (P_i - P_j),   GP_i = sum_j c_ij/2 (delta delta^T - (Sigma_i - Sigma_j)),
//      plus one entry of gmu_i = sum_j c_ij (P_i + P_j) delta, with c_ij = w_ij dD/dJ.  The matvec (P_i + P_j) delta is
//      lane-local and delta_c a broadcast read.  The records of all j (Sigma_j, P_j, mu_j; entry (c, r) at c G + r, zero
//      padded, so the inner loops have no bounds checks) stream through LDS in tiles of TJ classes; group s of a class takes
//      the rows s, s + NS, ... of each tile; the TI x TJ block of pair weights travels with the tile (WEIGHTED).  A group's
//      lanes read consecutive LDS addresses and groups of different classes that share s read the same ones (broadcast).
//      One group sum per pair (group_sum of pair_kernel.hpp).  Where 6 MMAX values fit the register budget the differences
//      of pass one are kept for the accumulation, else they are formed again from LDS.  The means-free case (MEANS false)
//      has no delta terms at all.  At the end the NS groups of a class are combined through LDS in the order s = 0, 1, ...:
//      one writer per class row, no atomics, bitwise reproducible.
//      float64 with m > 32 (BIG): one record is 48-64 KiB, so nothing is staged -- the lanes read Sigma_j, P_j and their own
//      class's rows from global memory (coalesced, L2 resident) and only the accumulators live in registers.
//   3. jeffreys_finish_kernel: gcov_i = GSigma_i - P_i sym(GP_i) P_i per class (the chain rule through the inverse), lower
//      triangle computed in double and mirrored; then launch_pair_loss_finalize (class_pair_loss.hip) for the loss and counters.
#include <hip/hip_runtime.h>

#include "../../include/sqfa_hip.h"
#include "class_pair_loss.hpp"
#include "pair_kernel.hpp"   // group_sum
#include "spd_class.hpp"     // stage 1

namespace sqfa {

struct JeffParams : PairLossParams {
  const void* mu;     // (n,m) or nullptr
  const void* cov;    // (n,m,m)
  const void* P;      // (n,m,m) precisions (stage 1)
  void* GS;           // (n,m,m) d loss / d Sigma at fixed P, or nullptr (forward only)
  void* GP;           // (n,m,m) d loss / d P
  void* gmu;          // (n,m) or nullptr
  int sqrt_mode;
};

// ---- stage 2: the pass over the ordered pairs ------------------------------------------------------------------------------
// Geometry of one row of the dispatch table: G lanes per group, matrices up to MMAX x MMAX (MMAX <= G).
template <typename T, int G_, int MMAX_, bool BIG_, bool MEANS_>
struct JeffCfg {
  static constexpr int G = G_, MMAX = MMAX_;
  static constexpr bool BIG = BIG_, MEANS = MEANS_;
  static_assert(MMAX <= G && G >= 4 && G <= 64, "one matrix index per lane");
  static constexpr int GROUPS = 256 / G;
  static constexpr int MAT = MMAX * G;                         // entries of one matrix of a record
  static constexpr int REC = 2 * MAT + (MEANS ? G : 0);        // Sigma_j, P_j, mu_j
  static constexpr int CREC = 2 * MAT + G;                     // accumulators of one group in the combine buffer
  static constexpr size_t BUDGET = 52 * 1024;
  // the differences of pass one stay in registers while 6 MMAX values keep one wave per SIMD without scratch
  static constexpr bool KEEP = !BIG && 6 * MMAX * (int)(sizeof(T) / 4) <= 200;
  // classes per workgroup: enough groups of different classes side by side to fill a 32-lane half (they broadcast), more
  // where NS records of a tile, or the TI records of the combine buffer, would not fit
  static constexpr int ti() {
    if (BIG) return GROUPS;
    int t = G >= 64 ? 1 : (G >= 16 ? 2 : 32 / G);
    while (t < GROUPS && ((GROUPS / t) * REC * sizeof(T) > BUDGET || t * CREC * sizeof(T) > BUDGET)) t *= 2;
    return t;
  }
  static constexpr int TI = ti();
  static constexpr int NS = GROUPS / TI;
  static constexpr int rounds() {   // records per group and tile: up to 8 while the tile stays within the budget
    if (BIG) return 1;
    int r = (int)(BUDGET / (NS * REC * sizeof(T)));
    return r < 1 ? 1 : (r > 8 ? 8 : r);
  }
  static constexpr int TJ = NS * rounds();
  static constexpr int TILE_ELEMS = BIG ? 1 : TJ * REC;
  static constexpr int COMB_ELEMS = NS > 1 ? TI * CREC : 1;    // the combine buffer reuses the tile
  static constexpr int BUF_ELEMS = TILE_ELEMS > COMB_ELEMS ? TILE_ELEMS : COMB_ELEMS;
  static_assert(TI * NS * G == 256, "lane groups must fill the workgroup");
  static_assert(!BIG || NS == 1, "the unstaged kernels combine nothing");
  static_assert((size_t)BUF_ELEMS * sizeof(T) + (size_t)TI * TJ * sizeof(T) + (size_t)TI * G * sizeof(T) + 2048 <= 64 * 1024,
                "LDS per workgroup stays within 64 KiB");
};

template <typename Cfg, typename T, bool WEIGHTED>
__global__ __launch_bounds__(256) void jeffreys_pair_kernel(const JeffParams p) {
  constexpr int G = Cfg::G, MMAX = Cfg::MMAX, MAT = Cfg::MAT, REC = Cfg::REC, CREC = Cfg::CREC;
  constexpr int TI = Cfg::TI, NS = Cfg::NS, TJ = Cfg::TJ;
  constexpr bool BIG = Cfg::BIG, MEANS = Cfg::MEANS, KEEP = Cfg::KEEP;
  __shared__ __align__(16) T tile[Cfg::BUF_ELEMS];
  __shared__ T s_w[WEIGHTED && !BIG ? TI * TJ : 1];   // weights of the current tile: row ti, column jj
  __shared__ T s_mui[MEANS && !BIG ? TI * G : 1];     // the means of the workgroup's classes, for the broadcast of delta_c
  __shared__ double s_loss[TI][NS];
  __shared__ int s_cnt[TI][NS][2];
  const int tid = threadIdx.x, n = p.n, m = p.m, mm = m * m;
  const int lane = tid % G, gid = tid / G, ti = gid % TI, s = gid / TI;
  const int i = blockIdx.x * TI + ti;
  const bool ivalid = i < n, rvalid = lane < m;
  const int ic = ivalid ? i : n - 1, lanec = rvalid ? lane : 0;   // clamped: every address formed below is inside its array
  const T* cov = static_cast<const T*>(p.cov);
  const T* P = static_cast<const T*>(p.P);
  const T* mu = static_cast<const T*>(p.mu);
  const T* W = static_cast<const T*>(p.W);
  const T* ownS = cov + (size_t)ic * mm + lanec;   // entry (c, lane) at ownS[c m]
  const T* ownP = P + (size_t)ic * mm + lanec;

  // this lane's entries of Sigma_i and P_i (the unstaged kernels read them again for every pair instead)
  T si[BIG ? 1 : MMAX], pi[BIG ? 1 : MMAX];
  if constexpr (!BIG) {
#pragma unroll
    for (int c = 0; c < MMAX; ++c) {
      const bool ok = ivalid && rvalid && c < m;
      const T a = ownS[ok ? c * m : 0], b = ownP[ok ? c * m : 0];
      si[c] = ok ? a : T(0);
      pi[c] = ok ? b : T(0);
    }
  }
  T mui_r = T(0);
  if constexpr (MEANS) {
    const T v = mu[(size_t)ic * m + lanec];
    mui_r = (ivalid && rvalid) ? v : T(0);
    if constexpr (!BIG) {
      if (s == 0) s_mui[ti * G + lane] = mui_r;
    }
  }
  T accS[MMAX], accP[MMAX];
#pragma unroll
  for (int c = 0; c < MMAX; ++c) accS[c] = accP[c] = T(0);
  T gmu_acc = T(0);

  const T w = pair_weight<T>(p), eps = pair_eps<T>(p);
  const bool sqrt_mode = p.sqrt_mode != 0, want_grad = p.GS != nullptr;
  T* dist = static_cast<T*>(p.dist);
  double loss_acc = 0.0;
  int n_nan = 0, n_inf = 0;

  for (int j0 = 0; j0 < n; j0 += TJ) {
    if constexpr (!BIG) {
      __syncthreads();   // the previous tile has been consumed
      for (int q = tid; q < TJ * REC; q += 256) {
        const int jj = q / REC, e = q % REC, j = j0 + jj;
        const int f = e % MAT, c = f / G, l = f % G;
        bool valid = j < n && c < m && l < m;
        const T* src = (e < MAT ? cov : P) + (valid ? (size_t)j * mm + c * m + l : 0);
        if constexpr (MEANS) {
          if (e >= 2 * MAT) {   // here f == l == e - 2 MAT
            valid = j < n && l < m;
            src = mu + (valid ? (size_t)j * m + l : 0);
          }
        }
        const T v = *src;   // always a valid address: no branch around the load
        tile[q] = valid ? v : T(0);
      }
      if constexpr (WEIGHTED) {
        for (int q = tid; q < TI * TJ; q += 256) {
          const int it = blockIdx.x * TI + q / TJ, j = j0 + q % TJ;
          const bool valid = it < n && j < n;
          const T v = W[valid ? (size_t)it * n + j : 0];
          s_w[q] = valid ? v : T(0);
        }
      }
      __syncthreads();
    }
#pragma unroll 1
    for (int jj = s; jj < TJ; jj += NS) {
      const int j = j0 + jj;
      const bool jvalid = j < n;
      const int jc = jvalid ? j : n - 1;
      // entry (c, lane) of Sigma_j / P_j at recS[c STRIDE] / recP[c STRIDE]
      const T* recS = BIG ? cov + (size_t)jc * mm + lanec : tile + jj * REC + lane;
      const T* recP = BIG ? P + (size_t)jc * mm + lanec : recS + MAT;
      const int STRIDE = BIG ? m : G;
      const T* muj = nullptr;
      const T* mui = nullptr;
      if constexpr (MEANS) {
        muj = BIG ? mu + (size_t)jc * m : tile + jj * REC + 2 * MAT;
        mui = BIG ? mu + (size_t)ic * m : s_mui + ti * G;
      }
      T wij = w;
      if constexpr (WEIGHTED) wij = BIG ? W[(size_t)ic * n + jc] : s_w[ti * TJ + jj];

      auto load = [&](const T* base, int c) -> T {   // BIG: global memory, padding masked; else LDS, zero padded
        if constexpr (BIG) {
          const bool ok = rvalid && c < m;
          const T v = base[ok ? c * STRIDE : 0];
          return ok ? v : T(0);
        } else {
          return base[c * STRIDE];
        }
      };
      auto delta = [&](int c) -> T {
        if constexpr (BIG) {
          const bool ok = c < m;
          const T a = mui[ok ? c : 0], b = muj[ok ? c : 0];
          return ok ? a - b : T(0);
        } else {
          return mui[c] - muj[c];
        }
      };

      T dr = T(0);
      if constexpr (MEANS) {
        const T b = BIG ? muj[lanec] : muj[lane];
        dr = rvalid ? mui_r - b : T(0);
      }
      // pass one: -<dP, dS> and y = (P_i + P_j) delta, entry `lane`
      T kP[KEEP ? MMAX : 1], kS[KEEP ? MMAX : 1], kD[KEEP && MEANS ? MMAX : 1];
      T part = T(0), y = T(0);
#pragma unroll
      for (int c = 0; c < MMAX; ++c) {
        const T pj = load(recP, c), sj = load(recS, c);
        const T pic = BIG ? load(ownP, c) : pi[c], sic = BIG ? load(ownS, c) : si[c];
        const T dP = pic - pj, dS = sic - sj;
        part -= dP * dS;
        if constexpr (MEANS) {
          const T dc = delta(c);
          y += (pic + pj) * dc;
          if constexpr (KEEP) kD[c] = dc;
        }
        if constexpr (KEEP) {
          kP[c] = dP;
          kS[c] = dS;
        }
      }
      if constexpr (MEANS) part += dr * y;
      const T Jr = T(0.5) * group_sum<G>(part);   // every lane of the group gets the total
      // J >= 0 mathematically: a rounded negative one (near-equal classes) is taken as 0 with derivative 0; NaN stays NaN
      const bool clamped = Jr < T(0);
      const T J = clamped ? T(0) : Jr;
      if (ivalid && jvalid && j != i) {
        T D, cij;
        if (sqrt_mode) {
          D = math::sqrt(J + eps);
          cij = clamped ? T(0) : T(0.5) * wij / D;
        } else {
          D = J;
          cij = clamped ? T(0) : wij;
        }
        if (want_grad) {
          const T h = T(0.5) * cij;
          // pass two: GSigma_i += -c/2 dP,  GP_i += c/2 (delta delta^T - dS),  gmu_i += c y
#pragma unroll
          for (int c = 0; c < MMAX; ++c) {
            T dP, dS;
            if constexpr (KEEP) {
              dP = kP[c];
              dS = kS[c];
            } else {
              dP = (BIG ? load(ownP, c) : pi[c]) - load(recP, c);
              dS = (BIG ? load(ownS, c) : si[c]) - load(recS, c);
            }
            accS[c] -= h * dP;
            if constexpr (MEANS) {
              T dc;
              if constexpr (KEEP) dc = kD[c];
              else dc = delta(c);
              accP[c] += h * (dr * dc - dS);
            } else {
              accP[c] -= h * dS;
            }
          }
          if constexpr (MEANS) gmu_acc += cij * y;
        }
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
  if constexpr (NS > 1) {
    if (want_grad) {   // uniform over the workgroup
      T* mine = tile + (size_t)ti * CREC + lane;
      for (int q = 1; q < NS; ++q) {
        if (s == q) {
#pragma unroll
          for (int c = 0; c < MMAX; ++c) {
            mine[c * G] = accS[c];
            mine[MAT + c * G] = accP[c];
          }
          mine[2 * MAT] = gmu_acc;
        }
        __syncthreads();
        if (s == 0) {
#pragma unroll
          for (int c = 0; c < MMAX; ++c) {
            accS[c] += mine[c * G];
            accP[c] += mine[MAT + c * G];
          }
          gmu_acc += mine[2 * MAT];
        }
        __syncthreads();
      }
    }
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
    if (dist != nullptr) dist[(size_t)i * n + i] = sqrt_mode ? math::sqrt(eps) : T(0);   // sqrt(0 + eps), as the torch expression
  }
  if (!want_grad || !rvalid) return;
  T* gs = static_cast<T*>(p.GS) + (size_t)i * mm + lane;
  T* gp = static_cast<T*>(p.GP) + (size_t)i * mm + lane;
#pragma unroll
  for (int c = 0; c < MMAX; ++c) {
    if (c < m) {
      gs[c * m] = accS[c];
      gp[c * m] = accP[c];
    }
  }
  if constexpr (MEANS) static_cast<T*>(p.gmu)[(size_t)i * m + lane] = gmu_acc;
}

// ---- stage 3: gcov_i = GSigma_i - P_i sym(GP_i) P_i -------------------------------------------------------------------------
// One workgroup per class.  Y = sym(GP_i) P_i goes through the (double) workspace, P_i sits in LDS.
template <typename T>
__global__ __launch_bounds__(256) void jeffreys_finish_kernel(const T* __restrict__ P, const T* __restrict__ GS,
                                                               const T* __restrict__ GP, double* __restrict__ Y,
                                                               T* __restrict__ gcov, int m) {
  __shared__ T sP[64 * 64];
  const int tid = threadIdx.x, mm = m * m;
  const size_t base = (size_t)blockIdx.x * mm;
  const T* gp = GP + base;
  double* y = Y + base;
  for (int idx = tid; idx < mm; idx += 256) sP[idx] = P[base + idx];
  __syncthreads();
  for (int idx = tid; idx < mm; idx += 256) {
    const int k = idx / m, b = idx % m;
    double acc = 0.0;
    for (int l = 0; l < m; ++l) acc += 0.5 * ((double)gp[k * m + l] + (double)gp[l * m + k]) * (double)sP[l * m + b];
    y[idx] = acc;
  }
  __threadfence_block();
  __syncthreads();
  for (int idx = tid; idx < mm; idx += 256) {
    const int a = idx / m, b = idx % m;
    if (b > a) continue;
    double acc = 0.0;
    for (int k = 0; k < m; ++k) acc += (double)sP[a * m + k] * y[k * m + b];
    const T v = (T)((double)GS[base + idx] - acc);
    gcov[base + a * m + b] = v;
    gcov[base + b * m + a] = v;
  }
}

template <typename T, int G, int MMAX, bool BIG>
static hipError_t launch_jeffreys(const JeffParams& p, hipStream_t stream) {
  using CfgM = JeffCfg<T, G, MMAX, BIG, true>;
  using CfgS = JeffCfg<T, G, MMAX, BIG, false>;
  const bool weighted = p.W != nullptr;
  if (p.mu != nullptr) {
    const dim3 grid((p.n + CfgM::TI - 1) / CfgM::TI);
    if (weighted) hipLaunchKernelGGL((jeffreys_pair_kernel<CfgM, T, true>), grid, dim3(256), 0, stream, p);
    else hipLaunchKernelGGL((jeffreys_pair_kernel<CfgM, T, false>), grid, dim3(256), 0, stream, p);
  } else {
    const dim3 grid((p.n + CfgS::TI - 1) / CfgS::TI);
    if (weighted) hipLaunchKernelGGL((jeffreys_pair_kernel<CfgS, T, true>), grid, dim3(256), 0, stream, p);
    else hipLaunchKernelGGL((jeffreys_pair_kernel<CfgS, T, false>), grid, dim3(256), 0, stream, p);
  }
  return hipGetLastError();
}

// lanes per group by matrix size: the smallest group that holds one index per lane; float64 above 32 is unstaged
template <typename T>
static hipError_t dispatch_jeffreys(const JeffParams& p, hipStream_t stream) {
  constexpr bool F64 = sizeof(T) == 8;
  const int m = p.m;
  if (m <= 4) return launch_jeffreys<T, 4, 4, false>(p, stream);
  if (m <= 8) return launch_jeffreys<T, 8, 8, false>(p, stream);
  if (m <= 16) return launch_jeffreys<T, 16, 16, false>(p, stream);
  if (m <= 24) return launch_jeffreys<T, 32, 24, false>(p, stream);
  if (m <= 32) return launch_jeffreys<T, 32, 32, false>(p, stream);
  if (m <= 48) return launch_jeffreys<T, 64, 48, F64>(p, stream);
  return launch_jeffreys<T, 64, 64, F64>(p, stream);
}

// workspace: [P (n,m,m) dtype] [GSigma (n,m,m) dtype] [GP (n,m,m) dtype] [Y (n,m,m) double] [partial losses (n) double]
//            [counts (n,2) int]
struct JeffLayout {
  size_t off_p, off_gs, off_gp, off_y, off_loss, off_cnt, total;   // total 0: no layout for these sizes
};
static JeffLayout jeffreys_layout(int n, int m, int dtype) {
  JeffLayout w{};
  if (n < 2 || m < 1 || m > 64 || (dtype != SQFA_F32 && dtype != SQFA_F64)) return w;
  const size_t mat = (size_t)n * m * m;
  WorkspaceCursor ws;
  w.off_p = ws.take(mat * dtype_bytes(dtype));
  w.off_gs = ws.take(mat * dtype_bytes(dtype));
  w.off_gp = ws.take(mat * dtype_bytes(dtype));
  w.off_y = ws.take(mat * sizeof(double));
  w.off_loss = ws.take((size_t)n * sizeof(double));
  w.off_cnt = ws.take((size_t)n * 2 * sizeof(int));
  w.total = ws.at;
  return w;
}
}  // namespace sqfa

using namespace sqfa;

extern "C" size_t sqfa_jeffreys_workspace_bytes(int n, int m, int dtype) { return jeffreys_layout(n, m, dtype).total; }

extern "C" int sqfa_jeffreys_pairwise_loss(const void* mu, const void* cov, int n, int m, int dtype, int sqrt_mode, double eps,
                                           const void* pair_weights, double uniform_weight, void* loss_out, void* gmu_out,
                                           void* gcov_out, void* dist_out, int* nonfinite_out, void* workspace,
                                           size_t workspace_bytes, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  // gradients: with means both or neither; without means gcov_out alone
  const bool grads_ok = mu != nullptr ? (gmu_out != nullptr) == (gcov_out != nullptr) : gmu_out == nullptr;
  const JeffLayout w = jeffreys_layout(n, m, dtype);
  const int rc = check_pair_loss_args("sqfa_jeffreys_pairwise_loss", "covariances", cov == nullptr, n, m, dtype,
                                      sqrt_mode == 0 || sqrt_mode == 1,
                                      grads_ok ? nullptr : "gmu_out and gcov_out go together, and gmu_out needs mu", w.total,
                                      "sqfa_jeffreys_workspace_bytes", workspace, workspace_bytes);
  if (rc != SQFA_OK) return rc;
  unsigned char* ws = static_cast<unsigned char*>(workspace);
  const bool want_grad = gcov_out != nullptr;
  // 1. per-class precisions
  if (launch_spd_inverse(cov, n, m, dtype, ws + w.off_p, nullptr, stream) != hipSuccess) return SQFA_ERR_LAUNCH;
  // 2. the pass over the ordered pairs
  JeffParams p{};
  p.mu = mu;
  p.cov = cov;
  p.P = ws + w.off_p;
  p.GS = want_grad ? ws + w.off_gs : nullptr;
  p.GP = want_grad ? ws + w.off_gp : nullptr;
  p.gmu = gmu_out;
  p.sqrt_mode = sqrt_mode;
  fill_pair_loss_params(p, n, m, eps, pair_weights, uniform_weight, dist_out, reinterpret_cast<double*>(ws + w.off_loss),
                        reinterpret_cast<int*>(ws + w.off_cnt));
  if (dispatch_dtype(dtype, [&](auto t) { return dispatch_jeffreys<decltype(t)>(p, stream); }) != hipSuccess)
    return SQFA_ERR_LAUNCH;
  // 3. the chain rule through the inverse
  if (want_grad) {
    dispatch_dtype(dtype, [&](auto t) {
      using T = decltype(t);
      hipLaunchKernelGGL((jeffreys_finish_kernel<T>), dim3(n), dim3(256), 0, stream, static_cast<const T*>(p.P),
                         static_cast<const T*>(p.GS), static_cast<const T*>(p.GP), reinterpret_cast<double*>(ws + w.off_y),
                         static_cast<T*>(gcov_out), m);
    });
    if (hipGetLastError() != hipSuccess) return SQFA_ERR_LAUNCH;
  }
  // 4. loss and counters
  if (launch_pair_loss_finalize(p.loss_part, p.cnt_part, n, dtype, loss_out, nonfinite_out, stream) != hipSuccess)
    return SQFA_ERR_LAUNCH;
  return SQFA_OK;
}
