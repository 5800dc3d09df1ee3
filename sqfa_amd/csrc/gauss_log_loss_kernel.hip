// gauss_log_loss_kernel.hip -- the log-loss of the Gaussian class scores (gauss_scores_kernel.hip) and its gradients.
// With W_c = L_c^-1, y_nc = W_c (z_n - mu_c), s_nc = -1/2 |y_nc|^2 + offset_c, lse_n = logsumexp_c s_nc and labels y_n:
//     ll_n = s_{n, y_n} - lse_n,   loss = -1/N sum_n ll_n
//     p_nc = exp(s_nc - lse_n),    r_nc = g (p_nc - [c == y_n]) / N        (g: the upstream scalar)
//     dloss/dz_n     = - sum_c W_c^T (r_nc y_nc)
//     dloss/dmu_c    =   W_c^T sum_n r_nc y_nc
//     dloss/dSigma_c = 1/2 W_c^T ( sum_n r_nc (y_nc y_nc^T - I) ) W_c
// always in the whitened-difference form.  The labelled class's r is formed as -g P_n / N with P_n = sum_{c != y_n} p_nc, the
// sum of the other posteriors, never as p - 1: where a sample is classified with near certainty, p - 1 is all rounding and
// the gradient, small as it is, would be noise.  With one class P_n is an empty sum: ll_n = 0 and every gradient 0 exactly.
//
// Launches (caller's stream; nothing allocated, synchronised or read back; no float atomics, every sum in a fixed order:
// bitwise reproducible; every grid and split a function of (N, C, K, dtype) alone):
//   forward   sqfa_gauss_scores with only the log-sum-exp asked for, then
//     gl_label_kernel     one sample per lane, 64 per workgroup.  The label is range-checked BEFORE anything is addressed
//                         with it: an out-of-range label is counted and its gathers go to class 0.  y = W_y (z - mu_y) on
//                         the lower triangle in double (N K^2 / 2 multiply-adds), ll_n, and the workgroup's sum of ll_n in
//                         double by a fixed tree.
//     gl_reduce_kernel    one workgroup: the partial sums in a fixed order, the flags, the loss.
//   backward, sample-owned (gradZ)
//     gl_sample_kernel    the geometry, stage and product of gauss_scores_kernel (gauss_whiten.hpp), all row blocks of y
//                         kept.  |y|^2 is summed over the quarters by that header's butterfly (the bits of the score the scores
//                         pass put into lse), r = g exp(s - lse) / N for c != label and 0 for the label (P_n += p), and the
//                         second product u[k][j] += sum_i W_c[i][k] (r y[i][j]) takes the contraction index
//                         i = 16 rb + acc_row(q, reg) for step (rb, reg) and quarter q: the accumulators of y are its B
//                         operand as they stand, and the A operand is read from the same LDS copy of W_c, rows on the
//                         quarters.  The zero blocks of W_c are skipped in both products.
//     gl_sample_finish_kernel  one sample per lane: P_n and u summed over the class splits in split order, the labelled
//                         class's term -g P_n / N W_y^T y on the VALU in double (label range-checked first), gradZ = -u.
//                         The pass runs whichever gradients are asked for: the class-owned pass reads P_n.
//   backward, class-owned (grad_means, grad_cov)
//     gl_class_kernel     workgroup (class c, split of the samples), W_c and mu_c resident in LDS, 4 waves that take
//                         16-sample tiles in turn.  y^T = (Z - mu)^T W^T, samples on the rows: register `reg` of column
//                         block ib in lane (i, q) is y[sample acc_row(q, reg)][16 ib + i], which is the A operand
//                         (y[.][i]) and, times r, the B operand of M_c += sum_n r y y^T with the samples as the
//                         contraction index; only the blocks on and below the diagonal are formed (this operand map is this
//                         kernel's own).  r comes from a second evaluation of y with the features on the rows, by
//                         gauss_whiten.hpp, so that the score has the bits of the scores pass; a cross-lane read brings it to
//                         the accumulator rows.  R_c = sum r and v_c = sum r y ride along on the VALU.
//                         The 4 waves' partials are added in wave order through LDS and written to the slab
//                         (sample splits, C, K^2 + K + 1).
//     gl_finish_kernel    one workgroup per class: the slab summed in split order in double (lower triangle, mirrored),
//                         grad_mu = W^T v, grad_cov = 1/2 W^T (M - R I) W in double, every entry (a, b) computed as the
//                         entry (max, min): exactly symmetric.
// gl_label_kernel forms z - mu in T and accumulates in double, gl_sample_finish_kernel forms the difference in double: two
// arithmetics, each with its bits, so the two VALU passes are not merged with each other or with the MFMA product.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>

#include "../../include/sqfa_hip.h"
#include "class_pair_loss.hpp"   // namespace math, dispatch_dtype, WorkspaceCursor
#include "gauss_whiten.hpp"

namespace sqfa {

constexpr int GL_CLASS_TARGET_WG = 2048;  // workgroups asked for by the class-owned pass
constexpr int GL_TILES_MIN = 16;          // 16-sample tiles per workgroup of the class-owned pass before the samples are split
constexpr int GL_MAX_SAMPLE_SPLIT = 1024;
constexpr size_t GL_SLAB_BYTES = (size_t)32 << 20;   // the slab stays below this while the samples are split

template <typename T> struct GlParams {
  const T* Z;
  const long long* labels;
  long long N;
  const T* mu;
  const T* W;
  const double* offset;
  int C, K;
  const T* lse;
  const T* upstream;   // (1) or nullptr (1)
  T* gradZ;
  T* grad_mu;
  T* grad_cov;
  int groups_per_split, class_splits;   // sample-owned pass: groups of 4 classes
  T* u_part;                            // (class_splits, N, K): u of the classes of a split, the labelled class left out
  T* P_part;                            // (class_splits, N): sum of p over those classes
  T* P;                                 // (N): P_n = sum_{c != y_n} p_nc = 1 - p_{n, y_n}
  long long tiles_per_split;            // class-owned pass: 16-sample tiles
  int sample_splits;
  T* slab;                              // (sample_splits, C, K K + K + 1): M (lower triangle), v, R
};

// ---- forward: the label pass ---------------------------------------------------------------------------------------------------

template <typename T, bool MEANS>
__global__ __launch_bounds__(GW_ROWS) void gl_label_kernel(const T* __restrict__ Z, const long long* __restrict__ labels,
                                                           long long N, const T* __restrict__ mu, const T* __restrict__ W,
                                                           const double* __restrict__ offset, int C, int K,
                                                           const T* __restrict__ lse, T* __restrict__ ll_out,
                                                           double* __restrict__ part, int* __restrict__ flags) {
  __shared__ T sD[GW_KMAX * GW_ROWS];   // [k][lane]: a lane reads back only what it wrote
  __shared__ double sSum[GW_ROWS];
  const int tid = threadIdx.x;
  const long long n = (long long)blockIdx.x * GW_ROWS + tid;
  const bool live = n < N;
  const long long lab = live ? labels[n] : 0;
  const bool in_range = lab >= 0 && lab < (long long)C;
  const int c = in_range ? (int)lab : 0;   // the label is data: checked before it addresses anything
  const double off = offset[c];
  const bool prior0 = off == -(double)INFINITY;
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
  }
  const T l = live ? lse[n] : T(0);
  double ll = -0.5 * sq + off - (double)l;
  if (C == 1) ll = 0.0;    // the posterior of the only class
  if (ll > 0.0) ll = 0.0;  // a log posterior; NaN stays
  const bool flagged = !in_range || prior0 || l != l;
  if (flagged) ll = math::nan<double>();
  if (live && ll_out != nullptr) ll_out[n] = (T)ll;
  sSum[tid] = live && !flagged ? ll : 0.0;
  __syncthreads();
  for (int s = GW_ROWS / 2; s > 0; s >>= 1) {
    if (tid < s) sSum[tid] += sSum[tid + s];
    __syncthreads();
  }
  if (tid == 0) part[blockIdx.x] = sSum[0];
  const unsigned long long out = __ballot(live && !in_range), zero = __ballot(live && in_range && prior0);
  if (tid == 0) {
    if (out != 0) atomicAdd(flags + 1, __popcll(out));
    if (zero != 0) atomicAdd(flags + 2, __popcll(zero));
  }
}

template <typename T>
__global__ __launch_bounds__(GW_THREADS) void gl_reduce_kernel(const double* __restrict__ part, long long n_parts, long long N,
                                                               const int* __restrict__ flags, T* __restrict__ loss_out) {
  __shared__ double sSum[GW_THREADS];
  const int tid = threadIdx.x;
  double s = 0.0;
  for (long long i = tid; i < n_parts; i += GW_THREADS) s += part[i];
  sSum[tid] = s;
  __syncthreads();
  for (int h = GW_THREADS / 2; h > 0; h >>= 1) {
    if (tid < h) sSum[tid] += sSum[tid + h];
    __syncthreads();
  }
  if (tid == 0) {
    const bool bad = flags[0] != 0 || flags[1] != 0 || flags[2] != 0;
    loss_out[0] = bad ? math::nan<T>() : (T)(-sSum[0] / (double)N);
  }
}

// ---- backward, sample-owned: gradZ ------------------------------------------------------------------------------------------

template <typename T, int KB, bool MEANS>
__global__ __launch_bounds__(GW_THREADS) void gl_sample_kernel(const GlParams<T> p) {
  using Tr = ProjTraits<T>;
  using Stage = WhitenStage<T, KB>;
  constexpr int CS = Stage::CS, KP = Stage::KP, PITCH = Stage::PITCH;
  __shared__ T sW[Stage::W_ELEMS];
  __shared__ T sMu[Stage::MU_ELEMS];
  const int tid = threadIdx.x, l = tid & 63, wave = tid >> 6, q = l >> 4, j = l & 15;
  const int K = p.K, C = p.C, K4 = (K + 3) / 4;
  const long long N = p.N;
  const long long n = (long long)blockIdx.x * GW_ROWS + wave * 16 + j;
  const auto [g_lo, g_hi, c_end] = whiten_class_range(C, p.groups_per_split, blockIdx.y);
  const bool live = n < N;

  T z[4 * KB];
  whiten_load_sample<T, KB>(z, p.Z, n, N, K, q);
  const T lse_n = p.lse[live ? n : 0];
  const long long lab = p.labels[live ? n : 0];   // only ever compared with a class index
  const T gs = (p.upstream != nullptr ? p.upstream[0] : T(1)) / (T)N;

  Stage stage(c_end, K, tid);
  stage.zero(sW);
  if (g_lo < g_hi) stage.template load<MEANS>(p.W, p.mu, 4 * g_lo);

  typename Tr::Acc u[KB];
#pragma unroll
  for (int kb = 0; kb < KB; ++kb) u[kb] = typename Tr::Acc{};
  T Pn = T(0);   // the same bits in the four quarters

#pragma unroll 1
  for (int g = g_lo; g < g_hi; ++g) {
    if constexpr (CS == 4) {
      __syncthreads();   // the previous stage has been consumed (first pass: the zero fill is done)
      stage.template store<MEANS>(sW, sMu);
      __syncthreads();
      if (g + 1 < g_hi) stage.template load<MEANS>(p.W, p.mu, 4 * (g + 1));
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int c = 4 * g + t;
      if (c >= c_end) continue;   // uniform over the workgroup
      if constexpr (CS == 1) {
        __syncthreads();
        stage.template store<MEANS>(sW, sMu);
        __syncthreads();
        if (c + 1 < c_end) stage.template load<MEANS>(p.W, p.mu, c + 1);
      }
      const T* w = sW + (CS == 4 ? t : 0) * KP * PITCH;
      T b[4 * KB];
      whiten_center<T, KB, MEANS>(b, z, sMu + (CS == 4 ? t : 0) * KP, K4, q);
      typename Tr::Acc y[KB];
      // the score in the bits that went into lse_n: exp(s - lse) is then as consistent as a softmax of stored scores, which
      // is what keeps r accurate where the posterior is nearly 1
      const T sq = whiten_quarters_sum(whiten_product<T, KB>(y, w, b, K, K4, j, q));
      const T off = (T)p.offset[c];
      const T sc = T(-0.5) * sq + off;
      const T post = lab == (long long)c ? T(0) : math::exp(sc - lse_n);   // the labelled class: gl_sample_finish_kernel
      const T r = live ? gs * post : T(0);
      Pn += post;
      // u[k][j] += sum_i W[i][k] (r y[i][j]): step (rb, reg) contracts over the rows i = 16 rb + acc_row(q, reg)
#pragma unroll
      for (int rb = 0; rb < KB; ++rb) {
        if (rb * 16 < K) {
#pragma unroll
          for (int reg = 0; reg < 4; ++reg) {
            const T bv = r * y[rb][reg];
            const T* wr = w + (rb * 16 + Tr::acc_row(q, reg)) * PITCH + j;
#pragma unroll
            for (int kb = 0; kb <= rb; ++kb) u[kb] = Tr::mfma(wr[kb * 16], bv, u[kb]);
          }
        }
      }
    }
  }

  if (!live) return;
  if (q == 0) p.P_part[(size_t)blockIdx.y * (size_t)N + n] = Pn;
  if (p.gradZ == nullptr) return;   // uniform: only P is wanted
  T* dst = p.u_part + (size_t)blockIdx.y * (size_t)N * K;
#pragma unroll
  for (int kb = 0; kb < KB; ++kb) {
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int k = kb * 16 + Tr::acc_row(q, reg);
      if (k < K) dst[(size_t)n * K + k] = u[kb][reg];
    }
  }
}

// One sample per lane, 64 per workgroup: P_n = the splits' sums of p in split order, and
//     gradZ_n = -(sum of the splits' u in split order) + g P_n / N  W_y^T W_y (z_n - mu_y)
// with the labelled class's term on the VALU in double (r_{n, y_n} = -g P_n / N: the sum of the other posteriors, not
// p - 1, which cancels where the posterior is nearly 1).  The label is range-checked before it addresses anything; an
// out-of-range label gathers class 0.
template <typename T, bool MEANS>
__global__ __launch_bounds__(GW_ROWS) void gl_sample_finish_kernel(const GlParams<T> p) {
  __shared__ double sY[GW_KMAX * GW_ROWS];   // [k][lane]: a lane reads back only what it wrote
  const int tid = threadIdx.x, K = p.K;
  const long long N = p.N;
  const long long n = (long long)blockIdx.x * GW_ROWS + tid;
  if (n >= N) return;   // no barrier below
  T Ps = p.P_part[n];
  for (int sp = 1; sp < p.class_splits; ++sp) Ps += p.P_part[(size_t)sp * (size_t)N + n];
  p.P[n] = Ps;
  if (p.gradZ == nullptr) return;
  const long long lab = p.labels[n];
  const int c = lab >= 0 && lab < (long long)p.C ? (int)lab : 0;
  for (int k = 0; k < K; ++k) {
    double d = (double)p.Z[(size_t)n * K + k];
    if constexpr (MEANS) d -= (double)p.mu[(size_t)c * K + k];
    sY[k * GW_ROWS + tid] = d;
  }
  const T* w = p.W + (size_t)c * K * K;
  for (int i = K - 1; i >= 0; --i) {   // y = W d in place: row i reads d_k, k <= i, and no later row reads slot i
    double a = 0.0;
    for (int k = 0; k <= i; ++k) a += (double)w[i * K + k] * sY[k * GW_ROWS + tid];
    sY[i * GW_ROWS + tid] = a;
  }
  const double scale = (double)(p.upstream != nullptr ? p.upstream[0] : T(1)) / (double)N * (double)Ps;
  const size_t total = (size_t)N * K;
  for (int k = 0; k < K; ++k) {
    double t = 0.0;
    for (int i = k; i < K; ++i) t += (double)w[i * K + k] * sY[i * GW_ROWS + tid];
    const size_t at = (size_t)n * K + k;
    T us = p.u_part[at];
    for (int sp = 1; sp < p.class_splits; ++sp) us += p.u_part[(size_t)sp * total + at];
    p.gradZ[at] = (T)(scale * t - (double)us);
  }
}

// ---- backward, class-owned: grad_means, grad_cov --------------------------------------------------------------------------

template <typename T, int KB, bool MEANS>
__global__ __launch_bounds__(GW_THREADS) void gl_class_kernel(const GlParams<T> p) {
  using Tr = ProjTraits<T>;
  constexpr int KP = WhitenStage<T, KB>::KP, PITCH = WhitenStage<T, KB>::PITCH;   // W_c resident, in the stage's image
  constexpr int NB = KB * (KB + 1) / 2;   // blocks of M on and below the diagonal
  __shared__ T sW[KP * PITCH];
  __shared__ T sMu[KP];
  __shared__ T sV[4 * KP];
  __shared__ T sR[4];
  const int tid = threadIdx.x, l = tid & 63, wave = tid >> 6, q = l >> 4, j = l & 15;
  const int K = p.K, C = p.C, K4 = (K + 3) / 4, kk = K * K;
  const long long N = p.N;
  const int c = blockIdx.x;

  for (int i = tid; i < KP * PITCH; i += GW_THREADS) {
    const int row = i / PITCH, col = i % PITCH;
    const bool ok = row < K && col < K;
    const T v = p.W[ok ? (size_t)c * kk + row * K + col : 0];
    sW[i] = ok ? v : T(0);
  }
  if (tid < KP) {
    T v = T(0);
    if constexpr (MEANS) {
      if (tid < K) v = p.mu[(size_t)c * K + tid];
    }
    sMu[tid] = v;
  }
  __syncthreads();

  const T off = (T)p.offset[c];
  const T gs = (p.upstream != nullptr ? p.upstream[0] : T(1)) / (T)N;
  const long long tiles = (N + 15) / 16;
  const long long t_lo = (long long)blockIdx.y * p.tiles_per_split;
  const long long t_hi = t_lo + p.tiles_per_split < tiles ? t_lo + p.tiles_per_split : tiles;

  typename Tr::Acc M[NB];
#pragma unroll
  for (int e = 0; e < NB; ++e) M[e] = typename Tr::Acc{};
  T v[KB], R = T(0);
#pragma unroll
  for (int ib = 0; ib < KB; ++ib) v[ib] = T(0);

#pragma unroll 1
  for (long long t = t_lo + wave; t < t_hi; t += 4) {
    const long long n = t * 16 + j;
    // whiten_load_sample and whiten_center in one statement (the same bits: sMu is zero from K on): through the two helpers
    // this kernel waits on every mean it reads and loses 7 to 12 % at K > 32 (profiles/gauss_whiten_refactor.txt)
    T b[4 * KB];
#pragma unroll
    for (int s = 0; s < 4 * KB; ++s) {
      const int k = 4 * s + q;
      const bool ok = n < N && k < K;
      const T zv = p.Z[ok ? (size_t)n * K + k : 0];
      b[s] = ok ? zv : T(0);
      if constexpr (MEANS) b[s] -= s < K4 ? sMu[k] : T(0);
    }
    // y^T = (Z - mu)^T W^T: register reg of block ib in lane (i, q) is y[sample acc_row(q, reg)][16 ib + i]
    typename Tr::Acc y[KB];
#pragma unroll
    for (int ib = 0; ib < KB; ++ib) {
      y[ib] = typename Tr::Acc{};
      if (ib * 16 < K) {
#pragma unroll
        for (int s = 0; s < 4 * (ib + 1); ++s)
          if (s < K4) y[ib] = Tr::mfma(b[s], sW[(ib * 16 + j) * PITCH + 4 * s + q], y[ib]);
      }
    }
    // r of sample j, with the score in the bits of the scores pass (see gl_sample_kernel): y = W (z - mu) with the features
    // on the rows once more
    const T sq = whiten_quarters_sum(whiten_sq_partial<T, KB>(sW, b, K, K4, j, q));
    const bool live = n < N;
    const T lse_n = p.lse[live ? n : 0];
    const long long lab = p.labels[live ? n : 0];   // only ever compared with a class index
    const T sc = T(-0.5) * sq + off;
    const T post = lab == (long long)c ? -p.P[live ? n : 0] : math::exp(sc - lse_n);   // r of the labelled class: -g P_n / N
    const T r_mine = live ? gs * post : T(0);
    T r[4];
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      r[reg] = __shfl(r_mine, Tr::acc_row(q, reg), 64);   // of the sample in this lane's accumulator row
      R += r[reg];
    }
#pragma unroll
    for (int ib = 0; ib < KB; ++ib) {
      if (ib * 16 < K) {
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) v[ib] += r[reg] * y[ib][reg];
#pragma unroll
        for (int i2 = 0; i2 <= ib; ++i2) {
#pragma unroll
          for (int reg = 0; reg < 4; ++reg)   // the samples acc_row(q, reg), q = 0 .. 3, are the contraction index
            M[ib * (ib + 1) / 2 + i2] = Tr::mfma(y[ib][reg], r[reg] * y[i2][reg], M[ib * (ib + 1) / 2 + i2]);
        }
      }
    }
  }

  // the quarters of v and R by a butterfly, then the 4 waves in wave order through LDS (W_c is no longer needed)
#pragma unroll
  for (int ib = 0; ib < KB; ++ib) {
    v[ib] += gw_shfl_xor(v[ib], 16);
    v[ib] += gw_shfl_xor(v[ib], 32);
  }
  R += gw_shfl_xor(R, 16);
  R += gw_shfl_xor(R, 32);
  if (q == 0) {
#pragma unroll
    for (int ib = 0; ib < KB; ++ib) sV[wave * KP + ib * 16 + j] = v[ib];
  }
  if (l == 0) sR[wave] = R;
  __syncthreads();
  for (int w = 0; w < 4; ++w) {
    if (wave == w) {
#pragma unroll
      for (int ib = 0; ib < KB; ++ib) {
#pragma unroll
        for (int i2 = 0; i2 <= ib; ++i2) {
#pragma unroll
          for (int reg = 0; reg < 4; ++reg) {
            T* d = sW + (ib * 16 + Tr::acc_row(q, reg)) * PITCH + i2 * 16 + j;
            const T mv = M[ib * (ib + 1) / 2 + i2][reg];
            *d = w == 0 ? mv : *d + mv;
          }
        }
      }
    }
    __syncthreads();
  }
  T* out = p.slab + ((size_t)blockIdx.y * C + c) * (size_t)(kk + K + 1);
  for (int idx = tid; idx < kk; idx += GW_THREADS) {
    const int row = idx / K, col = idx % K;
    if (col <= row) out[idx] = sW[row * PITCH + col];
  }
  if (tid < K) out[kk + tid] = ((sV[tid] + sV[KP + tid]) + sV[2 * KP + tid]) + sV[3 * KP + tid];
  if (tid == 0) out[kk + K] = ((sR[0] + sR[1]) + sR[2]) + sR[3];
}

// one workgroup per class: the slab in split order, grad_mu = W^T v, grad_cov = 1/2 W^T (M - R I) W, in double
template <typename T>
__global__ __launch_bounds__(GW_THREADS) void gl_finish_kernel(const GlParams<T> p) {
  __shared__ double sH[GW_KMAX * GW_KMAX];
  __shared__ double sv[GW_KMAX];
  __shared__ double sRc;
  const int tid = threadIdx.x, K = p.K, C = p.C, kk = K * K, c = blockIdx.x;
  const size_t per = (size_t)(kk + K + 1);
  const T* W = p.W + (size_t)c * kk;
  for (int idx = tid; idx < kk + K + 1; idx += GW_THREADS) {
    int at = idx;
    if (idx < kk) {
      const int row = idx / K, col = idx % K;
      at = row >= col ? idx : col * K + row;   // the lower triangle, mirrored
    }
    double s = 0.0;
    for (int sp = 0; sp < p.sample_splits; ++sp) s += (double)p.slab[((size_t)sp * C + c) * per + at];
    if (idx < kk) sH[idx] = s;
    else if (idx < kk + K) sv[idx - kk] = s;
    else sRc = s;
  }
  __syncthreads();
  if (p.grad_mu != nullptr && tid < K) {
    double s = 0.0;
    for (int i = tid; i < K; ++i) s += (double)W[i * K + tid] * sv[i];
    p.grad_mu[(size_t)c * K + tid] = (T)s;
  }
  if (p.grad_cov == nullptr) return;   // uniform
  constexpr int PER = GW_KMAX * GW_KMAX / GW_THREADS;
  double pv[PER];
#pragma unroll
  for (int e = 0; e < PER; ++e) {   // P = (M - R I) W
    const int idx = tid + e * GW_THREADS;
    pv[e] = 0.0;
    if (idx < kk) {
      const int a = idx / K, b = idx % K;
      double s = 0.0;
      for (int i = b; i < K; ++i) s += (sH[a * K + i] - (a == i ? sRc : 0.0)) * (double)W[i * K + b];
      pv[e] = s;
    }
  }
  __syncthreads();
#pragma unroll
  for (int e = 0; e < PER; ++e) {
    const int idx = tid + e * GW_THREADS;
    if (idx < kk) sH[idx] = pv[e];
  }
  __syncthreads();
#pragma unroll
  for (int e = 0; e < PER; ++e) {   // G = W^T P, the entry (a, b) computed as (max, min)
    const int idx = tid + e * GW_THREADS;
    if (idx < kk) {
      const int a0 = idx / K, b0 = idx % K;
      const int a = a0 >= b0 ? a0 : b0, b = a0 >= b0 ? b0 : a0;
      double s = 0.0;
      for (int i = a; i < K; ++i) s += (double)W[i * K + a] * sH[i * K + b];
      p.grad_cov[(size_t)c * kk + idx] = (T)(0.5 * s);
    }
  }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------

struct GlLayout {
  int groups_per_split, class_splits;
  long long tiles_per_split;
  int sample_splits;
  long long label_blocks;
  size_t scores_bytes, off_part, forward_total;   // forward: [the scores pass's workspace][label_blocks doubles]
  size_t off_upart, off_ppart, off_p, off_slab, backward_total;   // backward: [class_splits N K][class_splits N][N][slab]
};

static bool gl_layout(long long N, int C, int K, int dtype, GlLayout* w) {
  // the sample-owned pass: the class splits of the scores pass
  if (!whiten_class_split(N, C, K, dtype, &w->groups_per_split, &w->class_splits)) return false;
  const long long blocks = (N + GW_ROWS - 1) / GW_ROWS;
  w->scores_bytes = sqfa_gauss_scores_workspace_bytes(N, C, K, dtype);
  const size_t esz = dtype_bytes(dtype);
  // the class-owned pass: sample splits while workgroups are wanted, tiles are there and the slab stays small
  const long long tiles = (N + 15) / 16;
  const size_t per_class = ((size_t)K * K + K + 1) * esz;
  long long ss = (GL_CLASS_TARGET_WG + C - 1) / C;
  const long long by_work = (tiles + GL_TILES_MIN - 1) / GL_TILES_MIN;
  if (ss > by_work) ss = by_work;
  const long long by_slab = (long long)(GL_SLAB_BYTES / (per_class * (size_t)C));
  if (ss > by_slab) ss = by_slab;
  if (ss > GL_MAX_SAMPLE_SPLIT) ss = GL_MAX_SAMPLE_SPLIT;
  if (ss < 1) ss = 1;
  w->tiles_per_split = (tiles + ss - 1) / ss;
  w->sample_splits = (int)((tiles + w->tiles_per_split - 1) / w->tiles_per_split);   // no empty split
  w->label_blocks = blocks;
  WorkspaceCursor fw;
  fw.take(w->scores_bytes);
  w->off_part = fw.take((size_t)blocks * sizeof(double));
  w->forward_total = fw.at;
  WorkspaceCursor bw;
  w->off_upart = bw.take((size_t)w->class_splits * (size_t)N * K * esz);
  w->off_ppart = bw.take((size_t)w->class_splits * (size_t)N * esz);
  w->off_p = bw.take((size_t)N * esz);
  w->off_slab = bw.take((size_t)w->sample_splits * (size_t)C * per_class);
  w->backward_total = bw.at;
  return true;
}

template <typename T>
static hipError_t run_label_pass(const void* Z, const long long* labels, long long N, const void* mu, const void* W,
                                 const double* offset, int C, int K, void* loss, void* ll, const void* lse, int* flags,
                                 char* ws, const GlLayout& lay, hipStream_t stream) {
  double* part = reinterpret_cast<double*>(ws + lay.off_part);
  const dim3 grid((unsigned)lay.label_blocks), block(GW_ROWS);
  if (mu != nullptr)
    hipLaunchKernelGGL((gl_label_kernel<T, true>), grid, block, 0, stream, static_cast<const T*>(Z), labels, N,
                       static_cast<const T*>(mu), static_cast<const T*>(W), offset, C, K, static_cast<const T*>(lse),
                       static_cast<T*>(ll), part, flags);
  else
    hipLaunchKernelGGL((gl_label_kernel<T, false>), grid, block, 0, stream, static_cast<const T*>(Z), labels, N,
                       static_cast<const T*>(mu), static_cast<const T*>(W), offset, C, K, static_cast<const T*>(lse),
                       static_cast<T*>(ll), part, flags);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((gl_reduce_kernel<T>), dim3(1), dim3(GW_THREADS), 0, stream, part, lay.label_blocks, N, flags,
                     static_cast<T*>(loss));
  return hipGetLastError();
}

template <typename T>
static hipError_t run_backward(const void* Z, const long long* labels, long long N, const void* mu, const void* W,
                               const double* offset, int C, int K, const void* lse, const void* upstream, void* gradZ,
                               void* grad_mu, void* grad_cov, char* ws, const GlLayout& lay, hipStream_t stream) {
  GlParams<T> p{};
  p.Z = static_cast<const T*>(Z);
  p.labels = labels;
  p.N = N;
  p.mu = static_cast<const T*>(mu);
  p.W = static_cast<const T*>(W);
  p.offset = offset;
  p.C = C;
  p.K = K;
  p.lse = static_cast<const T*>(lse);
  p.upstream = static_cast<const T*>(upstream);
  p.gradZ = static_cast<T*>(gradZ);
  p.grad_mu = static_cast<T*>(grad_mu);
  p.grad_cov = static_cast<T*>(grad_cov);
  p.groups_per_split = lay.groups_per_split;
  p.class_splits = lay.class_splits;
  p.u_part = reinterpret_cast<T*>(ws + lay.off_upart);
  p.P_part = reinterpret_cast<T*>(ws + lay.off_ppart);
  p.P = reinterpret_cast<T*>(ws + lay.off_p);
  p.tiles_per_split = lay.tiles_per_split;
  p.sample_splits = lay.sample_splits;
  p.slab = reinterpret_cast<T*>(ws + lay.off_slab);
  // the sample-owned pass always runs: it also yields P_n, which the class-owned pass reads (without gradZ it stores no u)
  const bool class_pass = grad_mu != nullptr || grad_cov != nullptr;
  const dim3 sgrid((unsigned)lay.label_blocks, (unsigned)lay.class_splits);
  dispatch_kb(K, mu != nullptr, [&](auto kb, auto means) {
    hipLaunchKernelGGL((gl_sample_kernel<T, decltype(kb)::value, decltype(means)::value>), sgrid, dim3(GW_THREADS), 0, stream,
                       p);
  });
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const dim3 fgrid((unsigned)lay.label_blocks), fblock(GW_ROWS);
  if (mu != nullptr) hipLaunchKernelGGL((gl_sample_finish_kernel<T, true>), fgrid, fblock, 0, stream, p);
  else hipLaunchKernelGGL((gl_sample_finish_kernel<T, false>), fgrid, fblock, 0, stream, p);
  e = hipGetLastError();
  if (e != hipSuccess || !class_pass) return e;
  const dim3 cgrid((unsigned)C, (unsigned)lay.sample_splits);
  dispatch_kb(K, mu != nullptr, [&](auto kb, auto means) {
    hipLaunchKernelGGL((gl_class_kernel<T, decltype(kb)::value, decltype(means)::value>), cgrid, dim3(GW_THREADS), 0, stream,
                       p);
  });
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((gl_finish_kernel<T>), dim3((unsigned)C), dim3(GW_THREADS), 0, stream, p);
  return hipGetLastError();
}

}  // namespace sqfa

using namespace sqfa;

extern "C" size_t sqfa_gauss_log_loss_workspace_bytes(long long N, int C, int K, int dtype) {
  GlLayout w;
  return gl_layout(N, C, K, dtype, &w) ? w.forward_total : 0;
}

extern "C" size_t sqfa_gauss_log_loss_backward_workspace_bytes(long long N, int C, int K, int dtype) {
  GlLayout w;
  if (!gl_layout(N, C, K, dtype, &w)) return 0;
  return w.backward_total < 16 ? 16 : w.backward_total;
}

extern "C" int sqfa_gauss_log_loss_layout(long long N, int C, int K, int dtype, int* class_splits, int* groups_per_split,
                                          int* sample_splits, long long* tiles_per_split) {
  GlLayout w;
  if (class_splits == nullptr || groups_per_split == nullptr || sample_splits == nullptr || tiles_per_split == nullptr ||
      N < 1 || C < 1 || K < 1 || (dtype != SQFA_F32 && dtype != SQFA_F64))
    return SQFA_ERR_BAD_ARGUMENT;
  if (!gl_layout(N, C, K, dtype, &w)) return SQFA_ERR_UNSUPPORTED_M;
  *class_splits = w.class_splits;
  *groups_per_split = w.groups_per_split;
  *sample_splits = w.sample_splits;
  *tiles_per_split = w.tiles_per_split;
  return SQFA_OK;
}

extern "C" int sqfa_gauss_log_loss(const void* Z, const long long* labels, long long N, const void* means, const void* W,
                                   const double* offset, int C, int K, int dtype, void* loss_out,
                                   void* label_log_proba_out, void* logsumexp_out, int* flags_out, void* workspace,
                                   size_t workspace_bytes, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  GlLayout lay;
  const size_t need = gl_layout(N, C, K, dtype, &lay) ? lay.forward_total : 0;
  const bool nulls = Z == nullptr || labels == nullptr || W == nullptr || offset == nullptr || loss_out == nullptr ||
                     logsumexp_out == nullptr || flags_out == nullptr || N < 1 || C < 1 || K < 1;
  const int rc = check_gauss_args("sqfa_gauss_log_loss", nulls,
                                  "null samples, labels, factors, offsets, loss, logsumexp or flags, N < 1, C < 1 or K < 1", dtype,
                                  nullptr, K, true, need, workspace, workspace_bytes);
  if (rc != SQFA_OK) return rc;
  char* ws = static_cast<char*>(workspace);
  if (hipMemsetAsync(flags_out, 0, 3 * sizeof(int), stream) != hipSuccess) return SQFA_ERR_LAUNCH;
  // the log-sum-exp of every sample: the scores pass, which counts the samples with a NaN in their row into flags[0]
  const int status = sqfa_gauss_scores(Z, N, means, W, offset, C, K, dtype, nullptr, nullptr, nullptr, logsumexp_out, flags_out,
                                       ws, lay.scores_bytes, stream_);
  if (status != SQFA_OK) return status;
  const hipError_t e = dispatch_dtype(dtype, [&](auto t) {
    return run_label_pass<decltype(t)>(Z, labels, N, means, W, offset, C, K, loss_out, label_log_proba_out, logsumexp_out,
                                       flags_out, ws, lay, stream);
  });
  return e == hipSuccess ? SQFA_OK : SQFA_ERR_LAUNCH;
}

extern "C" int sqfa_gauss_log_loss_backward(const void* Z, const long long* labels, long long N, const void* means,
                                            const void* W, const double* offset, int C, int K, int dtype,
                                            const void* logsumexp, const void* upstream, void* gradZ_out,
                                            void* grad_means_out, void* grad_cov_out, void* workspace,
                                            size_t workspace_bytes, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  GlLayout lay;
  const size_t need = gl_layout(N, C, K, dtype, &lay) ? (lay.backward_total < 16 ? 16 : lay.backward_total) : 0;
  const bool nulls = Z == nullptr || labels == nullptr || W == nullptr || offset == nullptr || logsumexp == nullptr || N < 1 ||
                     C < 1 || K < 1;
  const char* own = nullptr;
  if (gradZ_out == nullptr && grad_means_out == nullptr && grad_cov_out == nullptr) own = "no gradient asked for";
  else if (means == nullptr && grad_means_out != nullptr) own = "grad_means_out without means";
  const int rc = check_gauss_args("sqfa_gauss_log_loss_backward", nulls,
                                  "null samples, labels, factors, offsets or logsumexp, N < 1, C < 1 or K < 1", dtype, own, K, true,
                                  need, workspace, workspace_bytes);
  if (rc != SQFA_OK) return rc;
  const hipError_t e = dispatch_dtype(dtype, [&](auto t) {
    return run_backward<decltype(t)>(Z, labels, N, means, W, offset, C, K, logsumexp, upstream, gradZ_out, grad_means_out,
                                     grad_cov_out, static_cast<char*>(workspace), lay, stream);
  });
  return e == hipSuccess ? SQFA_OK : SQFA_ERR_LAUNCH;
}
