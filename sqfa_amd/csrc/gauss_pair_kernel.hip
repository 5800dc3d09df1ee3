// gauss_pair_kernel.hip -- per-pair Gaussian terms behind the reference's "other" distance_fun
// operators (src/sqfa/distances.py:240-432): for every pair (i, j) of Gaussians
//     Sbar = (Sigma_i + Sigma_j) / 2 = R R^T,   delta = mu_i - mu_j
//     Q_ij  = delta^T Sbar^-1 delta     (mahalanobis_sq; /8 in bhattacharyya; acosh(1+Q/4) in fisher_rao_same_cov)
//     LD_ij = log det Sbar              (bhattacharyya / hellinger)
// and, given upstream gradients gQ, gLD (nA,nB), the gradient of sum_ij (gQ_ij Q_ij + gLD_ij LD_ij)
// with respect to the A side:
//     d/dmu_i    = sum_j gQ_ij 2 s_ij,                          s = Sbar^-1 delta
//     d/dSigma_i = sum_j 1/2 (-gQ_ij s s^T + gLD_ij Sbar^-1)
// The reference forms the (nA,nB,K,K) tensor of mean covariances and calls batched inv / logdet on
// it (1 GB at C=1000, K=16); here nothing larger than (nA,nB) is ever stored.
//
// Mapping: one workgroup per A class i; a lane group of G = pow2 >= m lanes (inside one wave) owns
// one pair at a time and walks j = group, group + NG, ...; lane r of the group owns row r.  The
// matrices live in LDS (run-time m, no register indexing): Cholesky (right-looking), forward
// substitution for Q, back substitution for s, R^-1 column by column for Sbar^-1.  Each group
// keeps its own gradient accumulator in LDS; groups are combined in a fixed order at the end
// (bitwise reproducible, no atomics).  The B-side gradient is the same launch with the roles
// swapped (the caller transposes gQ / gLD).
//
// Fused mode (sqfa_gauss_pairwise_loss, template parameter MODE = GAUSS_FUSED of both kernels, self case only): the pair's
// distance D (bhattacharyya / hellinger / mahalanobis[_sq]) and its partial derivatives are formed from q and ld the
// moment the pair is finished, so gQ / gLD are never read and no (C,C) matrix exists unless dist_out is asked for.
// Class row i accumulates  w D_ij (i > j)  and the gradient of every pair it belongs to from its own side; the term
// of the per-class log-determinants, -(1/4) (sum_j w dD/dBh_ij) Sigma_i^-1, uses the j == i step of the walk (Sbar_ii is
// Sigma_i exactly), which parks Sigma_i^-1 in the workspace until the row's sum is known.  MODE = GAUSS_PRE is the
// per-class pre-pass: the same Cholesky arithmetic on the pairs (c, c), writing logdet Sigma_c only.
// MODE = GAUSS_FUSED_W (sqfa_gauss_pairwise_loss_weighted with a weight matrix): w becomes w_ij = W[i n + j], read by the
// row's owner for every ordered pair -- W must be symmetric, since class j weighs the same pair with W[j n + i].  The
// register kernel reads a coalesced row segment per round (lane = class j), issued behind the factorisation and covered
// by the forward substitution; the LDS kernel reads one broadcast value per pair.
#include <hip/hip_runtime.h>
#include <stdio.h>

#include "../../include/sqfa_hip.h"
#include "class_pair_loss.hpp"
#include "pair_kernel.hpp"   // transposing tree reductions (tree_reduce_blocks), wave_sum

namespace sqfa {

// LDS of one wave is processed in program order; this only stops the compiler from moving LDS
// accesses across the hand-off between lanes of a group (all inside one wave)
__device__ __forceinline__ void group_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

template <int G, typename T> __device__ __forceinline__ T group_total(T v) {
#pragma unroll
  for (int d = 1; d < G; d <<= 1) v += __shfl_xor(v, d, 64);
  return v;
}

// The fused mode's fields are those of PairLossParams (class_pair_loss.hpp), declared here in the order the kernels below
// were tuned with: the order of the kernel arguments decides the scalar loads, and through the scalar spills of the register
// kernels their vector registers and occupancy (the common struct as a base costs gauss_pair_kernel<float, 64, GAUSS_FUSED>
// 24 VGPRs and a wave per SIMD).
struct GaussParams {
  const void *muA, *covA, *muB, *covB;
  const void *gQ, *gLD;      // (nA,nB) or nullptr
  void *Q, *LD;              // (nA,nB) or nullptr
  void *gmuA, *gcovA;        // (nA,m), (nA,m,m) or nullptr
  int nA, nB, m, ng;         // ng: lane groups per workgroup
  // fused mode only (B is A)
  int kind, n;               // SQFA_GAUSS_*; n: nA = nB again (it sits in the padding behind `kind`)
  double eps, weight;
  float epsf, weightf;       // the same two, rounded once on the host (scalar kernel arguments, no conversion per wave)
  void *ldc;                 // (n) logdet Sigma_c: written by the pre-pass, read by the fused pass
  void *sinv;                // (n,m,m) lower triangle of Sigma_i^-1, or nullptr (forward only / mahalanobis)
  void *dist;                // (n,n) or nullptr
  double *loss_part;         // (n) per-class partial losses
  int *cnt_part;             // (n,2) per-class {#NaN, #inf}
  const void *W;             // (n,n) symmetric per-pair weights (MODE = GAUSS_FUSED_W only; `weight` is then unused)
};

// GAUSS_FUSED_W: the fused mode with w_ij = W[i n + j] in place of the scalar weight -- an instantiation of its own, so
// that the uniform fused kernels stay the code they were
enum { GAUSS_PLAIN = 0, GAUSS_FUSED = 1, GAUSS_PRE = 2, GAUSS_FUSED_W = 3 };

// D and its partial derivatives from the pair terms: dQ = dD/dQ in total (through Bh too), dBh = dD/dBh (dD/dLD = dBh / 2,
// dD/dld_c = -dBh / 4).  On the diagonal the log-determinant term is exactly zero, as in the reference.  The term is >= 0
// mathematically and the difference of three rounded logarithms: where that comes out negative (near-equal classes) it is
// taken as 0 with derivative 0, so dBh is 0 there while dQ is not (NaN stays NaN: the comparison is false for it).
template <typename T>
__device__ __forceinline__ void gauss_distance(int kind, T eps, T q, T ld, T ldi, T ldj, bool diagonal, T& D, T& dQ, T& dBh) {
  if (kind == SQFA_GAUSS_MAHALANOBIS_SQ) {
    D = q; dQ = T(1); dBh = T(0);
  } else if (kind == SQFA_GAUSS_MAHALANOBIS) {
    D = math::sqrt(q + eps); dQ = T(0.5) / D; dBh = T(0);
  } else {
    const T det = diagonal ? T(0) : T(0.5) * (ld - T(0.5) * (ldi + ldj));
    const bool clamped = det < T(0);
    const T bh = q * T(0.125) + (clamped ? T(0) : det);
    if (kind == SQFA_GAUSS_BHATTACHARYYA) {
      D = bh; dBh = T(1);
    } else {
      const T e = math::exp(-bh);
      D = math::sqrt(T(1) - e + eps);
      dBh = T(0.5) * e / D;
    }
    dQ = T(0.125) * dBh;
    if (clamped) dBh = T(0);
  }
}

template <typename T, int G, int MODE = GAUSS_PLAIN>
__global__ void gauss_pair_kernel(const GaussParams p) {
  constexpr bool WEIGHTED = MODE == GAUSS_FUSED_W, FUSED = MODE == GAUSS_FUSED || WEIGHTED, PRE = MODE == GAUSS_PRE;
  extern __shared__ __align__(16) unsigned char smem_raw[];
  T* smem = reinterpret_cast<T*>(smem_raw);
  constexpr int LD_ = G + 1;                 // row pitch
  constexpr int MAT = G * LD_;
  constexpr int PER_GROUP = 3 * MAT + 2 * G;  // a, w, acc, s, accmu
  const int tid = threadIdx.x;
  const int grp = tid / G, r = tid % G;
  const int m = p.m;
  const bool live = grp < p.ng;   // a block is padded to whole waves: surplus groups own no LDS and no pair
  const bool active = live && r < m;
  const int i = blockIdx.x;
  T* a = smem + (size_t)(live ? grp : 0) * PER_GROUP;
  T* w = a + MAT;
  T* acc = w + MAT;
  T* sv = acc + MAT;
  T* accmu = sv + G;
  const T* muA = static_cast<const T*>(p.muA);
  const T* covA = static_cast<const T*>(p.covA);
  const T* muB = static_cast<const T*>(p.muB);
  const T* covB = static_cast<const T*>(p.covB);
  const T* gQ = static_cast<const T*>(p.gQ);
  const T* gLD = static_cast<const T*>(p.gLD);
  const bool want_grad = p.gcovA != nullptr;
  const int lane_base = (tid & 63) & ~(G - 1);  // first lane of my group inside the wave
  // Sbar^-1 is needed where logdet Sbar has a gradient
  const bool with_inv = FUSED ? p.kind <= SQFA_GAUSS_HELLINGER : gLD != nullptr;
  const T* ldc = static_cast<const T*>(p.ldc);
  const T fw0 = pair_weight<T>(p), feps = pair_eps<T>(p);
  T loss_acc = T(0), csum = T(0);   // fused: lane 0 of the group keeps the group's partial sums
  int n_nan = 0, n_inf = 0;

  if (want_grad && live) {
    for (int c = 0; c < G; ++c) acc[r * LD_ + c] = T(0);
  }
  T mu_acc = T(0);
  const T mu_i = active ? muA[(size_t)i * m + r] : T(0);
  const T* ci = covA + (size_t)i * m * m;

  // pre-pass: the single "pair" (i, i), on group 0
  for (int j = PRE ? (grp == 0 ? i : p.nB) : (live ? grp : p.nB); j < p.nB; j += PRE ? p.nB : p.ng) {
    const T* cj = covB + (size_t)j * m * m;
    T fw = fw0;
    if constexpr (WEIGHTED) fw = static_cast<const T*>(p.W)[(size_t)i * p.nB + j];   // one address per group: a broadcast read
    if (active) {
      for (int c = 0; c <= r; ++c) a[r * LD_ + c] = T(0.5) * (ci[r * m + c] + cj[r * m + c]);
    }
    T d = active ? mu_i - muB[(size_t)j * m + r] : T(0);
    group_sync();
    // ---- Cholesky Sbar = R R^T, in place (lower) --------------------------------------
    for (int k = 0; k < m; ++k) {
      const T piv = a[k * LD_ + k];
      const T rs = math::rsqrt(piv);   // non-positive pivot -> NaN everywhere downstream, never a fault
      T l = T(0);
      if (active && r >= k) {
        l = a[r * LD_ + k] * rs;
        a[r * LD_ + k] = l;
      }
      group_sync();
      if (active && r > k) {
        for (int c = k + 1; c <= r; ++c) a[r * LD_ + c] -= l * a[c * LD_ + k];
      }
      group_sync();
    }
    const T diag = active ? a[r * LD_ + r] : T(1);
    const T rdiag = T(1) / diag;
    const T ld = T(2) * group_total<G>(active ? math::log(diag) : T(0));
    // ---- z = R^-1 delta (column oriented) ----------------------------------------------
    T z = T(0);
    for (int k = 0; k < m; ++k) {
      const T zk = __shfl(d * rdiag, lane_base + k, 64);
      if (r == k) z = zk;
      if (active && r > k) d -= a[r * LD_ + k] * zk;
    }
    if constexpr (PRE) {
      if (r == 0) static_cast<T*>(p.ldc)[i] = ld;
      return;
    }
    const T q = group_total<G>(z * z);
    T gq, gl;
    if constexpr (FUSED) {
      T D, dQ, dBh;
      gauss_distance<T>(p.kind, feps, q, ld, with_inv ? ldc[i] : T(0), with_inv ? ldc[j] : T(0), j == i, D, dQ, dBh);
      gq = j != i ? fw * dQ : T(0);
      gl = j != i ? T(0.5) * fw * dBh : T(0);
      if (r == 0) {
        if (j != i) csum += fw * dBh;
        if (j < i) {   // each unordered pair counted once
          loss_acc += fw * D;
          n_nan += D != D;
          n_inf += D == D && __builtin_isinf(D);
        }
        if (p.dist != nullptr) static_cast<T*>(p.dist)[(size_t)i * p.nB + j] = D;
      }
    } else {
      if (r == 0) {
        if (p.Q != nullptr) static_cast<T*>(p.Q)[(size_t)i * p.nB + j] = q;
        if (p.LD != nullptr) static_cast<T*>(p.LD)[(size_t)i * p.nB + j] = ld;
      }
    }
    if (!want_grad) {
      group_sync();
      continue;
    }
    if constexpr (!FUSED) {
      gq = gQ != nullptr ? gQ[(size_t)i * p.nB + j] : T(0);
      gl = gLD != nullptr ? gLD[(size_t)i * p.nB + j] : T(0);
    }
    // ---- s = R^-T z (column oriented, from the last row up) -----------------------------
    T t = z, s = T(0);
    for (int k = m - 1; k >= 0; --k) {
      const T sk = __shfl(t * rdiag, lane_base + k, 64);
      if (r == k) s = sk;
      if (active && r < k) t -= a[k * LD_ + r] * sk;
    }
    sv[r] = s;
    mu_acc += T(2) * gq * s;
    // ---- W = R^-1: lane c owns column c ---------------------------------------------------
    if (with_inv) {
      if (active) {
        w[r * LD_ + r] = rdiag;
        for (int rr = r + 1; rr < m; ++rr) {
          T sum = T(0);
          for (int k = r; k < rr; ++k) sum += a[rr * LD_ + k] * w[k * LD_ + r];
          w[rr * LD_ + r] = -sum / a[rr * LD_ + rr];
        }
      }
    }
    group_sync();
    // ---- accumulate 1/2 (-gq s s^T + gl Sbar^-1), lower triangle, row r ---------------------
    if (active) {
      for (int c = 0; c <= r; ++c) {
        T v = -gq * s * sv[c];
        if (with_inv) {
          T inv = T(0);
          for (int k = r; k < m; ++k) inv += w[k * LD_ + r] * w[k * LD_ + c];
          v += gl * inv;
          if constexpr (FUSED) {
            if (j == i) static_cast<T*>(p.sinv)[((size_t)i * m + r) * m + c] = inv;   // Sbar_ii = Sigma_i
          }
        }
        acc[r * LD_ + c] += T(0.5) * v;
      }
    }
    group_sync();
  }

  T coef = T(0);   // fused: -(1/4) sum_j w dD/dBh_ij, the weight of Sigma_i^-1
  if constexpr (FUSED) {
    __shared__ T s_part[64][2];
    __shared__ int s_cnt[64][2];
    if (live && r == 0) {
      s_part[grp][0] = loss_acc;
      s_part[grp][1] = csum;
      s_cnt[grp][0] = n_nan;
      s_cnt[grp][1] = n_inf;
    }
    if (want_grad && live) accmu[r] = mu_acc;
    __syncthreads();
    T lsum = T(0), cs = T(0);
    int nn = 0, ni = 0;
    for (int g2 = 0; g2 < p.ng; ++g2) {
      lsum += s_part[g2][0];
      cs += s_part[g2][1];
      nn += s_cnt[g2][0];
      ni += s_cnt[g2][1];
    }
    if (tid == 0) {
      p.loss_part[i] = (double)lsum;
      p.cnt_part[2 * i] = nn;
      p.cnt_part[2 * i + 1] = ni;
    }
    if (!want_grad) return;
    coef = T(-0.25) * cs;
  } else {
    if (!want_grad) return;
    if (live) accmu[r] = mu_acc;
    __syncthreads();
  }
  // combine the groups in a fixed order; write the full symmetric gradient
  T* gcov = static_cast<T*>(p.gcovA) + (size_t)i * m * m;
  for (int e = tid; e < m * m; e += blockDim.x) {
    const int rr = e / m, cc = e % m;
    const int hi = rr > cc ? rr : cc, lo = rr > cc ? cc : rr;
    T sum = T(0);
    for (int g2 = 0; g2 < p.ng; ++g2) sum += smem[(size_t)g2 * PER_GROUP + 2 * MAT + hi * LD_ + lo];
    if constexpr (FUSED) {
      if (with_inv) sum += coef * static_cast<const T*>(p.sinv)[((size_t)i * m + hi) * m + lo];
    }
    gcov[e] = sum;
  }
  if (p.gmuA != nullptr) {
    T* gmu = static_cast<T*>(p.gmuA) + (size_t)i * m;
    for (int e = tid; e < m; e += blockDim.x) {
      T sum = T(0);
      for (int g2 = 0; g2 < p.ng; ++g2) sum += smem[(size_t)g2 * PER_GROUP + 3 * MAT + G + e];
      gmu[e] = sum;
    }
  }
}

template <typename T, int G, int MODE = GAUSS_PLAIN>
static hipError_t launch_gauss(const GaussParams& p0, hipStream_t stream) {
  GaussParams p = p0;
  const size_t per_group = (size_t)(3 * G * (G + 1) + 2 * G) * sizeof(T);
  int ng = MODE == GAUSS_PRE ? 1 : 256 / G;   // the pre-pass has one pair per class
  const size_t budget = 60 * 1024;
  while (ng > 1 && ng * per_group > budget) ng /= 2;
  if (ng > p.nB) {  // fewer pairs per class than groups: do not leave whole waves idle
    int need = 1;
    while (need < p.nB) need <<= 1;
    ng = need < ng ? need : ng;
    if (ng < 1) ng = 1;
  }
  p.ng = ng;
  const size_t lds = ng * per_group;
  if (lds > 48 * 1024) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&gauss_pair_kernel<T, G, MODE>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  int threads = ng * G;
  if (threads < 64) threads = 64;  // whole waves (extra lanes form idle groups: grp >= ng never owns a pair)
  hipLaunchKernelGGL((gauss_pair_kernel<T, G, MODE>), dim3(p.nA), dim3(threads), lds, stream, p);
  return hipGetLastError();
}


// ---------------------------------------------------------------------------------------------------------------
// Register-resident variant (round 3) for small matrices: ONE PAIR PER LANE.  The LDS kernel above walks a 16 x 16
// factorisation through ~50 dependent LDS round trips with 16 lanes per pair: 4.9 ms for the 10^6 ordered pairs of
// C=1000, K=16 (forward + backward, float32), two orders of magnitude above its arithmetic.  Here a lane holds the lower
// triangle of Sbar (M(M+1)/2 registers, M = 4 / 8 / 12 / 16, identity padded), factorises it in place with every loop
// unrolled (no cross-lane traffic at all), inverts the factor in place (W = R^-1, then Sbar^-1 = W^T W), and the 64
// pairs of a wave -- same class i, 64 consecutive classes j -- reduce their gradient contributions with the
// transposing tree reduction of the pair kernel (lane l finishes entries 64 I + l) into a per-wave LDS accumulator.
// One workgroup (4 waves) per class i walks over all j; the four accumulators are added in wave order at the end:
// bitwise reproducible, no atomics.  float32 up to m = 16 (136 + ~40 registers), float64 up to m = 8.
// entry IDX of a lane's gradient contribution, formed on the fly from Sbar^-1 (lower triangle, in `a`) and s (in `d`):
// IDX < TRI: d/dSigma entry; TRI <= IDX < TRI + M: d/dmu entry
template <typename T, int M> struct GradEntries {
  static constexpr int TRI = M * (M + 1) / 2;
  const T (&a)[TRI];
  const T (&d)[M];
  T gq, gl;
  bool with_inverse;
  template <int IDX> __device__ __forceinline__ T get() const {
    if constexpr (IDX < TRI) {
      constexpr int r = tri_row(IDX), c = IDX - r * (r + 1) / 2;
      const T outer = gq * d[r] * d[c];
      return T(0.5) * (with_inverse ? gl * a[IDX] - outer : -outer);
    } else if constexpr (IDX < TRI + M) {
      return T(2) * gq * d[IDX - TRI];
    } else {
      return T(0);
    }
  }
};

// (two workgroups per CU = 256 VGPRs: without the bound the scheduler batches all 2 x M(M+1)/2 loads of a round ahead of
// the arithmetic and takes 313 registers at M=16)
// EXACT: m == M (no identity padding: no selects, rows of M elements, 16-byte row loads when M % 4 == 0 (float32) / M % 2
// == 0 (float64) and the matrices are 16-byte aligned, which the launcher checks)
// (fused mode with identity padding in the kernel, MODE = GAUSS_FUSED && !EXACT: the selects of the padding plus the
// epilogue's scalars do not fit the budget of the twin; half the workgroups per CU instead of spills -- this variant only
// runs small problems, the host pads large ones to an EXACT size)
template <typename T, int M, bool EXACT, int MODE = GAUSS_PLAIN>
__global__ __launch_bounds__(256, ((M * (M + 1) / 2) * (int)(sizeof(T) / 4) <= 40 ? 4 : ((M * (M + 1) / 2) * (int)(sizeof(T) / 4) <= 140 ? 2 : 1))
                                   >> (((MODE == GAUSS_FUSED || MODE == GAUSS_FUSED_W) && !EXACT && (M * (M + 1) / 2) * (int)(sizeof(T) / 4) <= 140) ? 1 : 0))
void gauss_pair_reg_kernel(const GaussParams p) {
  constexpr bool WEIGHTED = MODE == GAUSS_FUSED_W, FUSED = MODE == GAUSS_FUSED || WEIGHTED, PRE = MODE == GAUSS_PRE;
  constexpr int TRI = M * (M + 1) / 2, NACC = TRI + M;
  __shared__ T s_acc[4][NACC | 1];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int i = blockIdx.x, m = p.m;
  const T* muA = static_cast<const T*>(p.muA);
  const T* covA = static_cast<const T*>(p.covA);
  const T* muB = static_cast<const T*>(p.muB);
  const T* covB = static_cast<const T*>(p.covB);
  const T* gQ = static_cast<const T*>(p.gQ);
  const T* gLD = static_cast<const T*>(p.gLD);
  const bool want_grad = p.gcovA != nullptr;
  if (want_grad) {
    for (int k = lane; k < NACC; k += 64) s_acc[wave][k] = T(0);   // wave-private: no block barrier needed
  }
  const T* ci = covA + (size_t)i * m * m;
  auto at = [](int r, int c) constexpr { return r * (r + 1) / 2 + c; };  // c <= r
  // Sbar^-1 is needed where logdet Sbar has a gradient
  const bool with_inv = FUSED ? p.kind <= SQFA_GAUSS_HELLINGER : gLD != nullptr;
  const T* ldc = static_cast<const T*>(p.ldc);
  const T fw0 = pair_weight<T>(p), feps = pair_eps<T>(p);
  T loss_acc = T(0), csum = T(0);   // fused: per-wave partial sums and counts (wave-uniform: scalar registers)
  int n_nan = 0, n_inf = 0;

  // pre-pass: one workgroup per 256 classes, lane = class c, the "pair" (c, c)
  const int rounds = PRE ? 1 : (p.nB + 255) / 256;
  for (int it = 0; it < rounds; ++it) {
    const int j = (PRE ? (int)blockIdx.x : it) * 256 + tid;
    const bool valid = j < p.nB;
    const T* cj = covB + (size_t)(valid ? j : 0) * m * m;
    // Sigma_i is the same in every round: hidden from loop-invariant code motion, or its 136 values would be kept in
    // registers across the whole loop (321 VGPRs and spills at M=16 instead of ~200)
    const T* cir = ci;
    if constexpr (PRE) cir = cj;
    else asm volatile("" : "+s"(cir));
    T a[TRI], d[M];
    // ---- Sbar = (Sigma_i + Sigma_j)/2 and its Cholesky factor R (lower, in place), ROW BY ROW: row r needs the finished
    //      rows above it and its own entries only, so the loads of a row sit next to their use (live set: the triangle
    //      built so far) ----
    T rdiag[M];
    T ld = T(0);
    constexpr int VW = 16 / (int)sizeof(T);
    struct alignas(16) RowVec { T v[VW]; };
#pragma unroll
    for (int r = 0; r < M; ++r) {
      T row[M];
      if constexpr (EXACT) {
        if constexpr (PRE) d[r] = T(0);
        else d[r] = muA[(size_t)i * M + r] - muB[(size_t)(valid ? j : 0) * M + r];
        if constexpr (M % VW == 0) {
#pragma unroll
          for (int c0 = 0; c0 <= r; c0 += VW) {
            const RowVec vi = *reinterpret_cast<const RowVec*>(cir + r * M + c0);
            const RowVec vj = *reinterpret_cast<const RowVec*>(cj + r * M + c0);
#pragma unroll
            for (int e = 0; e < VW; ++e) row[(c0 + e < M) ? c0 + e : 0] = T(0.5) * (vi.v[e] + vj.v[e]);
          }
        } else {
#pragma unroll
          for (int c = 0; c <= r; ++c) row[c] = T(0.5) * (cir[r * M + c] + cj[r * M + c]);
        }
      } else {
        const bool rr = r < m;
        const int rc = rr ? r : m - 1;   // clamped addresses, selected values: no branches
        const T dv = PRE ? T(0) : muA[(size_t)i * m + rc] - muB[(size_t)(valid ? j : 0) * m + rc];
        d[r] = rr ? dv : T(0);
#pragma unroll
        for (int c = 0; c <= r; ++c) {
          const int cc = c < m ? c : m - 1;
          const T v = T(0.5) * (cir[rc * m + cc] + cj[rc * m + cc]);
          row[c] = (rr && c < m) ? v : (r == c ? T(1) : T(0));
        }
      }
      // R[r][c] = (Sbar[r][c] - sum_{k<c} R[r][k] R[c][k]) / R[c][c];  R[r][r] = sqrt(Sbar[r][r] - sum_{k<r} R[r][k]^2)
#pragma unroll
      for (int c = 0; c < r; ++c) {
        T t = row[c];
#pragma unroll
        for (int k = 0; k < c; ++k) t -= row[k] * a[at(c, k)];
        row[c] = t * rdiag[c];
      }
      T piv = row[r];
#pragma unroll
      for (int k = 0; k < r; ++k) piv -= row[k] * row[k];
      const T rs = math::rsqrt(piv);   // non-positive pivot -> NaN downstream, never a fault
      rdiag[r] = rs;
      const T dk = piv * rs;
      ld += math::log(dk);
#pragma unroll
      for (int c = 0; c < r; ++c) a[at(r, c)] = row[c];
      a[at(r, r)] = dk;
    }
    ld *= T(2);
    if constexpr (PRE) {
      if (valid) static_cast<T*>(p.ldc)[j] = ld;
      return;
    }
    // weighted: lane = class j, one coalesced segment of row i of W per round; issued here, behind the factorisation (its
    // register peak) and ahead of the forward substitution, which covers the load
    T fw = fw0;
    if constexpr (WEIGHTED) fw = static_cast<const T*>(p.W)[valid ? (size_t)i * p.nB + j : (size_t)0];
    // ---- z = R^-1 delta, Q = |z|^2 ----
    T q = T(0);
#pragma unroll
    for (int k = 0; k < M; ++k) {
      T t = d[k];
#pragma unroll
      for (int c = 0; c < k; ++c) t -= a[at(k, c)] * d[c];
      d[k] = t * rdiag[k];   // d becomes z
      q += d[k] * d[k];
    }
    T gq, gl;
    if constexpr (FUSED) {
      T D, dQ, dBh;
      const T ldi = with_inv ? ldc[i] : T(0), ldj = with_inv ? ldc[valid ? j : 0] : T(0);
      gauss_distance<T>(p.kind, feps, q, ld, ldi, ldj, j == i, D, dQ, dBh);
      const bool off = valid && j != i, counted = valid && j < i;   // each unordered pair counted once
      gq = off ? fw * dQ : T(0);
      gl = off ? T(0.5) * fw * dBh : T(0);
      csum = wave_uniform(csum + wave_sum(off ? fw * dBh : T(0)));
      loss_acc = wave_uniform(loss_acc + wave_sum(counted ? fw * D : T(0)));
      n_nan += __popcll(__ballot(counted && D != D));
      n_inf += __popcll(__ballot(counted && D == D && __builtin_isinf(D)));
      if (valid && p.dist != nullptr) static_cast<T*>(p.dist)[(size_t)i * p.nB + j] = D;
      if (!want_grad) continue;
    } else {
      if (valid) {
        if (p.Q != nullptr) static_cast<T*>(p.Q)[(size_t)i * p.nB + j] = q;
        if (p.LD != nullptr) static_cast<T*>(p.LD)[(size_t)i * p.nB + j] = ld;
      }
      if (!want_grad) continue;
      gq = (valid && gQ != nullptr) ? gQ[(size_t)i * p.nB + j] : T(0);
      gl = (valid && gLD != nullptr) ? gLD[(size_t)i * p.nB + j] : T(0);
    }
    // ---- s = R^-T z (in place, from the last row up) ----
#pragma unroll
    for (int k = M - 1; k >= 0; --k) {
      T t = d[k];
#pragma unroll
      for (int r = k + 1; r < M; ++r) t -= a[at(r, k)] * d[r];
      d[k] = t * rdiag[k];   // d becomes s
    }
    if (with_inv) {
      // ---- W = R^-1 in place, column by column: column c of W needs R[r][k] for k >= c only, so it may overwrite
      //      column c of R as soon as it is complete ----
#pragma unroll
      for (int c = 0; c < M; ++c) {
        T wc[M];
        wc[c] = rdiag[c];
#pragma unroll
        for (int r = c + 1; r < M; ++r) {
          T sum = T(0);
#pragma unroll
          for (int k = c; k < r; ++k) sum += a[at(r, k)] * wc[k];
          wc[r] = -sum * rdiag[r];
        }
#pragma unroll
        for (int r = c; r < M; ++r) a[at(r, c)] = wc[r];
      }
      // ---- Sbar^-1 = W^T W in place, row by row: row r needs the rows k >= r of W, so it may overwrite row r ----
#pragma unroll
      for (int r = 0; r < M; ++r) {
        T row[M];
#pragma unroll
        for (int c = 0; c <= r; ++c) {
          T inv = T(0);
#pragma unroll
          for (int k = r; k < M; ++k) inv += a[at(k, r)] * a[at(k, c)];
          row[c] = inv;
        }
#pragma unroll
        for (int c = 0; c <= r; ++c) a[at(r, c)] = row[c];
      }
      if constexpr (FUSED) {
        if (valid && j == i) {   // Sbar_ii = Sigma_i: one lane of one round parks Sigma_i^-1 for the per-class term
          // (pitch M whatever m is: compile-time offsets; the workspace holds (m rounded up to 4)^2 elements per class)
          T* si = static_cast<T*>(p.sinv) + (size_t)i * (M * M);
#pragma unroll
          for (int r = 0; r < M; ++r) {
#pragma unroll
            for (int c = 0; c <= r; ++c) si[r * M + c] = a[at(r, c)];
          }
        }
      }
    }
    // ---- 1/2 (gl Sbar^-1 - gq s s^T) and 2 gq s, summed over the 64 pairs of the wave: lane l finishes entries 64 I + l ----
    {
      const GradEntries<T, M> prod{a, d, gq, gl, with_inv};
      T* acc = s_acc[wave];
      tree_reduce_blocks<6, 0, (NACC + 63) / 64, NACC, T>(prod, lane, [&](int idx, T v) { acc[idx] += v; });
    }
  }
  T coef = T(0);   // fused: -(1/4) sum_j w dD/dBh_ij, the weight of Sigma_i^-1
  if constexpr (FUSED) {
    __shared__ T s_part[4][2];
    __shared__ int s_cnt[4][2];
    if (lane == 0) {
      s_part[wave][0] = loss_acc;
      s_part[wave][1] = csum;
      s_cnt[wave][0] = n_nan;
      s_cnt[wave][1] = n_inf;
    }
    __syncthreads();
    if (tid == 0) {
      p.loss_part[i] = (double)(((s_part[0][0] + s_part[1][0]) + s_part[2][0]) + s_part[3][0]);
      p.cnt_part[2 * i] = s_cnt[0][0] + s_cnt[1][0] + s_cnt[2][0] + s_cnt[3][0];
      p.cnt_part[2 * i + 1] = s_cnt[0][1] + s_cnt[1][1] + s_cnt[2][1] + s_cnt[3][1];
    }
    if (!want_grad) return;
    coef = T(-0.25) * (((s_part[0][1] + s_part[1][1]) + s_part[2][1]) + s_part[3][1]);
  } else {
    if (!want_grad) return;
    __syncthreads();
  }
  T* gcov = static_cast<T*>(p.gcovA) + (size_t)i * m * m;
  for (int e = tid; e < m * m; e += 256) {
    const int rr = e / m, cc = e % m;
    const int hi = rr > cc ? rr : cc, lo = rr > cc ? cc : rr;
    const int idx = hi * (hi + 1) / 2 + lo;
    T sum = ((s_acc[0][idx] + s_acc[1][idx]) + s_acc[2][idx]) + s_acc[3][idx];
    if constexpr (FUSED) {
      if (with_inv) sum += coef * static_cast<const T*>(p.sinv)[(size_t)i * (M * M) + hi * M + lo];
    }
    gcov[e] = sum;
  }
  if (p.gmuA != nullptr) {
    T* gmu = static_cast<T*>(p.gmuA) + (size_t)i * m;
    for (int e = tid; e < m; e += 256)
      gmu[e] = ((s_acc[0][TRI + e] + s_acc[1][TRI + e]) + s_acc[2][TRI + e]) + s_acc[3][TRI + e];
  }
}

template <typename T, int M, int MODE = GAUSS_PLAIN>
static hipError_t launch_gauss_reg(const GaussParams& p, hipStream_t stream) {
  const bool aligned = (reinterpret_cast<size_t>(p.covA) % 16) == 0 && (reinterpret_cast<size_t>(p.covB) % 16) == 0;
  const dim3 grid(MODE == GAUSS_PRE ? (p.nA + 255) / 256 : p.nA);
  if (p.m == M && aligned)
    hipLaunchKernelGGL((gauss_pair_reg_kernel<T, M, true, MODE>), grid, dim3(256), 0, stream, p);
  else
    hipLaunchKernelGGL((gauss_pair_reg_kernel<T, M, false, MODE>), grid, dim3(256), 0, stream, p);
  return hipGetLastError();
}

// the kernel the plain entry point would pick for (dtype, m), in mode MODE
template <int MODE>
static hipError_t dispatch_gauss(const GaussParams& p, int dtype, hipStream_t stream) {
  const int m = p.m;
  if (dtype == SQFA_F32) {
    if (m <= 4) return launch_gauss_reg<float, 4, MODE>(p, stream);
    if (m <= 8) return launch_gauss_reg<float, 8, MODE>(p, stream);
    if (m <= 12) return launch_gauss_reg<float, 12, MODE>(p, stream);
    if (m <= 16) return launch_gauss_reg<float, 16, MODE>(p, stream);
    if (m <= 32) return launch_gauss<float, 32, MODE>(p, stream);
    return launch_gauss<float, 64, MODE>(p, stream);
  }
  if (m <= 4) return launch_gauss_reg<double, 4, MODE>(p, stream);
  if (m <= 8) return launch_gauss_reg<double, 8, MODE>(p, stream);
  if (m <= 12) return launch_gauss_reg<double, 12, MODE>(p, stream);
  if (m <= 16) return launch_gauss_reg<double, 16, MODE>(p, stream);
  if (m <= 32) return launch_gauss<double, 32, MODE>(p, stream);
  return launch_gauss<double, 64, MODE>(p, stream);
}
}  // namespace sqfa

using namespace sqfa;

extern "C" int sqfa_gauss_pair_terms(const void* muA, const void* covA, int nA, const void* muB, const void* covB,
                                     int nB, int m, int dtype, const void* gQ, const void* gLD, void* Q_out,
                                     void* LD_out, void* gmuA_out, void* gcovA_out, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  if (muA == nullptr || covA == nullptr || muB == nullptr || covB == nullptr || nA < 1 || nB < 1 || m < 1)
    return SQFA_ERR_BAD_ARGUMENT;
  if (dtype != SQFA_F32 && dtype != SQFA_F64) return SQFA_ERR_BAD_ARGUMENT;
  if (m > 64) return SQFA_ERR_UNSUPPORTED_M;
  if ((gmuA_out != nullptr) != (gcovA_out != nullptr)) return SQFA_ERR_BAD_ARGUMENT;
  if (gcovA_out != nullptr && gQ == nullptr && gLD == nullptr) return SQFA_ERR_BAD_ARGUMENT;
  GaussParams p{muA, covA, muB, covB, gQ, gLD, Q_out, LD_out, gmuA_out, gcovA_out, nA, nB, m, 1};
  hipError_t e;
#ifndef SQFA_GAUSS_REG
#define SQFA_GAUSS_REG 1   // 0: always the LDS kernel (development A/B)
#endif
#ifndef SQFA_GAUSS_REG_F64_MAX
#define SQFA_GAUSS_REG_F64_MAX 16   // float64 m > 8: the triangle needs 156 / 272 registers -- one wave per SIMD, part of it in AGPRs
#endif
  // small matrices: one pair per lane, everything in registers (float32 up to 16, float64 up to 8)
  if (SQFA_GAUSS_REG && dtype == SQFA_F32 && m <= 16) {
    if (m <= 4) e = launch_gauss_reg<float, 4>(p, stream);
    else if (m <= 8) e = launch_gauss_reg<float, 8>(p, stream);
    else if (m <= 12) e = launch_gauss_reg<float, 12>(p, stream);
    else e = launch_gauss_reg<float, 16>(p, stream);
    return e == hipSuccess ? SQFA_OK : SQFA_ERR_LAUNCH;
  }
  if (SQFA_GAUSS_REG && dtype == SQFA_F64 && m <= SQFA_GAUSS_REG_F64_MAX) {
    if (m <= 4) e = launch_gauss_reg<double, 4>(p, stream);
    else if (m <= 8) e = launch_gauss_reg<double, 8>(p, stream);
    else if (m <= 12) e = launch_gauss_reg<double, 12>(p, stream);
    else e = launch_gauss_reg<double, 16>(p, stream);
    return e == hipSuccess ? SQFA_OK : SQFA_ERR_LAUNCH;
  }
#define SQFA_GAUSS_DISPATCH(T)                                         \
  if (m <= 4) e = launch_gauss<T, 4>(p, stream);                       \
  else if (m <= 8) e = launch_gauss<T, 8>(p, stream);                  \
  else if (m <= 16) e = launch_gauss<T, 16>(p, stream);                \
  else if (m <= 32) e = launch_gauss<T, 32>(p, stream);                \
  else e = launch_gauss<T, 64>(p, stream);
  if (dtype == SQFA_F32) {
    SQFA_GAUSS_DISPATCH(float)
  } else {
    SQFA_GAUSS_DISPATCH(double)
  }
  return e == hipSuccess ? SQFA_OK : SQFA_ERR_LAUNCH;
}

// workspace of sqfa_gauss_pairwise_loss: [logdet Sigma_c (n)] [partial losses (n) double] [counts (n,2) int] [Sigma_c^-1 (n,m,m)]
struct GaussLayout {
  size_t off_ldc, off_loss, off_cnt, off_sinv, total;   // total 0: no layout for these sizes
};
static GaussLayout gauss_layout(int n, int m, int dtype) {
  GaussLayout w{};
  if (n < 2 || m < 1 || m > 64 || (dtype != SQFA_F32 && dtype != SQFA_F64)) return w;
  const size_t mp = ((size_t)m + 3) & ~(size_t)3;   // the register kernels park Sigma_c^-1 with their padded pitch
  WorkspaceCursor ws;
  w.off_ldc = ws.take((size_t)n * 8);   // 8 bytes per class whatever the dtype
  w.off_loss = ws.take((size_t)n * sizeof(double));
  w.off_cnt = ws.take((size_t)n * 2 * sizeof(int));
  w.off_sinv = ws.take((size_t)n * mp * mp * dtype_bytes(dtype));
  w.total = ws.at;
  return w;
}

extern "C" size_t sqfa_gauss_pairwise_workspace_bytes(int n, int m, int dtype) { return gauss_layout(n, m, dtype).total; }

extern "C" int sqfa_gauss_pairwise_loss_weighted(const void* mu, const void* cov, int n, int m, int dtype, int kind,
                                                 double eps, const void* pair_weights, double uniform_weight,
                                                 void* loss_out, void* gmu_out, void* gcov_out, void* dist_out,
                                                 int* nonfinite_out, void* workspace, size_t workspace_bytes,
                                                 void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const GaussLayout w = gauss_layout(n, m, dtype);
  // (no name: this entry point sets no text for sqfa_hip_last_error())
  const bool grads_ok = (gmu_out != nullptr) == (gcov_out != nullptr);
  const int rc = check_pair_loss_args(nullptr, nullptr, mu == nullptr || cov == nullptr, n, m, dtype,
                                      kind >= SQFA_GAUSS_BHATTACHARYYA && kind <= SQFA_GAUSS_MAHALANOBIS,
                                      grads_ok ? nullptr : "gmu_out and gcov_out go together", w.total, nullptr, workspace,
                                      workspace_bytes);
  if (rc != SQFA_OK) return rc;
  unsigned char* ws = static_cast<unsigned char*>(workspace);
  GaussParams p{mu, cov, mu, cov, nullptr, nullptr, nullptr, nullptr, gmu_out, gcov_out, n, n, m, 1};
  fill_pair_loss_params(p, n, m, eps, pair_weights, uniform_weight, dist_out, reinterpret_cast<double*>(ws + w.off_loss),
                        reinterpret_cast<int*>(ws + w.off_cnt));
  p.kind = kind;
  p.ldc = ws + w.off_ldc;
  p.sinv = ws + w.off_sinv;
  if (kind <= SQFA_GAUSS_HELLINGER) {   // per-class log-determinants first: every pair needs both of its classes'
    GaussParams pre = p;
    pre.gmuA = pre.gcovA = nullptr;
    if (dispatch_gauss<GAUSS_PRE>(pre, dtype, stream) != hipSuccess) return SQFA_ERR_LAUNCH;
  }
  const hipError_t e = pair_weights != nullptr ? dispatch_gauss<GAUSS_FUSED_W>(p, dtype, stream)
                                               : dispatch_gauss<GAUSS_FUSED>(p, dtype, stream);
  if (e != hipSuccess) return SQFA_ERR_LAUNCH;
  return launch_pair_loss_finalize(p.loss_part, p.cnt_part, n, dtype, loss_out, nonfinite_out, stream) == hipSuccess
             ? SQFA_OK : SQFA_ERR_LAUNCH;
}

extern "C" int sqfa_gauss_pairwise_loss(const void* mu, const void* cov, int n, int m, int dtype, int kind, double eps,
                                        double uniform_weight, void* loss_out, void* gmu_out, void* gcov_out,
                                        void* dist_out, int* nonfinite_out, void* workspace, size_t workspace_bytes,
                                        void* stream_) {
  return sqfa_gauss_pairwise_loss_weighted(mu, cov, n, m, dtype, kind, eps, nullptr, uniform_weight, loss_out, gmu_out,
                                           gcov_out, dist_out, nonfinite_out, workspace, workspace_bytes, stream_);
}
