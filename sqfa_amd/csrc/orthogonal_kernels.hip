// orthogonal_kernels.hip -- the orthogonal filter constraint (reference: src/sqfa/model.py:416-431 registers torch's
// orthogonal parametrization; torch.nn.utils.parametrizations._Orthogonal with orthogonal_map="householder" and a `base`
// matrix) in compact WY form, forward and backward, in place of tril -> column norms -> orgqr -> sign -> base @ Q and
// the autograd backward of each.
//
//   X (K,D) raw parameter, K < D;  V (D,K) = strictly-lower(X^T) + [I_K; 0];  s_i = int(X[i,i]) (not differentiated)
//   G = V^T V,  M = striu(G) + diag(G_ii / 2)  (= T^-1 of H_1 ... H_K = I - V T V^T),  W = M^-1 V_top^T  (upper triangular)
//   P = [I_K; 0] - V W,   F = (base (P * s))^T                                                       (K,D)
//   backward:  gP = (base^T gF^T) * s,  gW = -V^T gP,  Z = M^-T gW,  gM = -Z W^T,  S = striu(gM) + striu(gM)^T + diag(gM),
//              gV = -gP W^T + [Z^T; 0] + V S,   gX = strictly-lower(gV)^T  (exact zeros elsewhere)
//
// Launches (all on the caller's stream, nothing read back, no atomics; every sum over D has a fixed order):
//   orth_gram_kernel     one workgroup per block of 32 rows of V: partial G (and, backward, partial gW) in double -> workspace
//   orth_solve_kernel    ONE workgroup: sums the partials, solves for W (backward: also Z, S) in LDS, double whatever the dtype
//   orth_p_kernel        forward: P rows, 32 per workgroup
//   orth_product_kernel  the only part of any size: base (P * s) or base^T gF^T, 32 output rows per workgroup, the
//                        D-long sums walked in chunks of 64 through LDS (plain FMA), the next chunk's loads in flight
//   orth_gv_kernel       backward: gV -> gX, 16 rows of V per workgroup
// forward = gram, solve, p, product (4);  backward = product, gram, solve, gv (4).  The backward recomputes G, M and W
// from X: it needs nothing from a forward call's workspace.
#include <hip/hip_runtime.h>

#include "../../include/sqfa_hip.h"
#include "class_pair_loss.hpp"   // align256

namespace sqfa {

constexpr int ORTH_KMAX = 64;
constexpr int ORTH_ROWS = 32;     // rows of V per workgroup of the gram / p kernels
constexpr int ORTH_PITCH = 65;    // LDS row pitch of a (rows x K <= 64) tile
constexpr int ORTH_TR = 32;       // output rows per workgroup of the product
constexpr int ORTH_TD = 64;       // summation chunk of the product
constexpr int ORTH_GV_ROWS = 16;

// V[d][i] from the raw parameter
template <typename T> __device__ __forceinline__ double orth_v(const T* __restrict__ X, int D, int d, int i) {
  return d > i ? (double)X[(size_t)i * D + d] : (d == i ? 1.0 : 0.0);
}

// partial G[i][j] = sum_{d in block} V[d][i] V[d][j]; with gP (D,K): partial gW[i][j] = -sum_d V[d][i] gP[d][j]
template <typename T>
__global__ __launch_bounds__(256) void orth_gram_kernel(const T* __restrict__ X, const T* __restrict__ gP, int K, int D,
                                                        double* __restrict__ Gpart, double* __restrict__ gWpart) {
  __shared__ double sV[ORTH_ROWS * ORTH_PITCH];
  __shared__ double sG[ORTH_ROWS * ORTH_PITCH];
  const int tid = threadIdx.x, d0 = blockIdx.x * ORTH_ROWS;
  for (int idx = tid; idx < ORTH_ROWS * K; idx += 256) {
    const int dd = idx % ORTH_ROWS, i = idx / ORTH_ROWS, d = d0 + dd;
    sV[dd * ORTH_PITCH + i] = d < D ? orth_v(X, D, d, i) : 0.0;
  }
  if (gP != nullptr) {
    for (int idx = tid; idx < ORTH_ROWS * K; idx += 256) {
      const int dd = idx / K, k = idx % K, d = d0 + dd;
      sG[dd * ORTH_PITCH + k] = d < D ? (double)gP[(size_t)d * K + k] : 0.0;
    }
  }
  __syncthreads();
  const size_t out = (size_t)blockIdx.x * K * K;
  for (int e = tid; e < K * K; e += 256) {
    const int i = e / K, j = e % K;
    double g = 0.0, w = 0.0;
    for (int dd = 0; dd < ORTH_ROWS; ++dd) g += sV[dd * ORTH_PITCH + i] * sV[dd * ORTH_PITCH + j];
    Gpart[out + e] = g;
    if (gP != nullptr) {
      for (int dd = 0; dd < ORTH_ROWS; ++dd) w += sV[dd * ORTH_PITCH + i] * sG[dd * ORTH_PITCH + j];
      gWpart[out + e] = -w;
    }
  }
}

__device__ __forceinline__ double orth_sum_partials(const double* __restrict__ part, int nblk, size_t stride, int e) {
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;   // fixed association: reproducible
  int q = 0;
  for (; q + 4 <= nblk; q += 4) {
    a0 += part[(size_t)q * stride + e];
    a1 += part[(size_t)(q + 1) * stride + e];
    a2 += part[(size_t)(q + 2) * stride + e];
    a3 += part[(size_t)(q + 3) * stride + e];
  }
  for (; q < nblk; ++q) a0 += part[(size_t)q * stride + e];
  return (a0 + a1) + (a2 + a3);
}

// One workgroup.  sA = M, sB = V_top^T -> W (back substitution, one thread per column); W -> workspace.
// Backward (gWpart != nullptr): sB = gW -> Z = M^-T gW (forward substitution); Z -> workspace; sA = W^T;
// S = symmetric fill of gM = -Z W^T -> workspace.
template <typename T>
__global__ __launch_bounds__(256) void orth_solve_kernel(const T* __restrict__ X, int K, int D, int nblk,
                                                         const double* __restrict__ Gpart,
                                                         const double* __restrict__ gWpart, double* __restrict__ Wg,
                                                         double* __restrict__ Zg, double* __restrict__ Sg) {
  __shared__ double sA[ORTH_KMAX * ORTH_KMAX];
  __shared__ double sB[ORTH_KMAX * ORTH_KMAX];
  const int tid = threadIdx.x, KK = K * K;
  for (int e = tid; e < KK; e += 256) {
    const int i = e / K, j = e % K;
    const double g = orth_sum_partials(Gpart, nblk, (size_t)KK, e);
    sA[i * ORTH_KMAX + j] = j > i ? g : (j == i ? 0.5 * g : 0.0);
    sB[i * ORTH_KMAX + j] = orth_v(X, D, j, i);   // V_top^T[i][j] = V[j][i]
  }
  __syncthreads();
  if (tid < K) {
    const int k = tid;
    for (int j = K - 1; j >= 0; --j) {
      double r = sB[j * ORTH_KMAX + k];
      for (int l = j + 1; l < K; ++l) r -= sA[j * ORTH_KMAX + l] * sB[l * ORTH_KMAX + k];
      sB[j * ORTH_KMAX + k] = r / sA[j * ORTH_KMAX + j];
    }
  }
  __syncthreads();
  for (int e = tid; e < KK; e += 256) Wg[e] = sB[(e / K) * ORTH_KMAX + e % K];
  if (gWpart == nullptr) return;
  __syncthreads();
  for (int e = tid; e < KK; e += 256) sB[(e / K) * ORTH_KMAX + e % K] = orth_sum_partials(gWpart, nblk, (size_t)KK, e);
  __syncthreads();
  if (tid < K) {
    const int k = tid;
    for (int j = 0; j < K; ++j) {
      double r = sB[j * ORTH_KMAX + k];
      for (int l = 0; l < j; ++l) r -= sA[l * ORTH_KMAX + j] * sB[l * ORTH_KMAX + k];
      sB[j * ORTH_KMAX + k] = r / sA[j * ORTH_KMAX + j];
    }
  }
  __threadfence_block();
  __syncthreads();   // Z complete; W (written above by this workgroup) visible
  for (int e = tid; e < KK; e += 256) {
    const int b = e / K, k = e % K;
    Zg[e] = sB[b * ORTH_KMAX + k];
    sA[k * ORTH_KMAX + b] = Wg[e];   // W^T: the products below read it along b
  }
  __syncthreads();
  for (int e = tid; e < KK; e += 256) {
    const int a = e / K, b = e % K;
    if (a > b) continue;
    double g = 0.0;
    for (int k = 0; k < K; ++k) g += sB[a * ORTH_KMAX + k] * sA[k * ORTH_KMAX + b];
    Sg[a * K + b] = -g;
    Sg[b * K + a] = -g;
  }
}

// P[d][k] = [d == k] - sum_j V[d][j] W[j][k]   (D,K), dtype
template <typename T>
__global__ __launch_bounds__(256) void orth_p_kernel(const T* __restrict__ X, int K, int D, const double* __restrict__ Wg,
                                                     T* __restrict__ P) {
  __shared__ double sW[ORTH_KMAX * ORTH_PITCH];
  __shared__ double sV[ORTH_ROWS * ORTH_PITCH];
  const int tid = threadIdx.x, d0 = blockIdx.x * ORTH_ROWS;
  for (int e = tid; e < K * K; e += 256) sW[(e / K) * ORTH_PITCH + e % K] = Wg[e];
  for (int idx = tid; idx < ORTH_ROWS * K; idx += 256) {
    const int dd = idx % ORTH_ROWS, i = idx / ORTH_ROWS, d = d0 + dd;
    sV[dd * ORTH_PITCH + i] = d < D ? orth_v(X, D, d, i) : 0.0;
  }
  __syncthreads();
  for (int e = tid; e < ORTH_ROWS * K; e += 256) {
    const int dd = e / K, k = e % K, d = d0 + dd;
    if (d >= D) continue;
    double acc = d == k ? 1.0 : 0.0;
    for (int j = 0; j <= k; ++j) acc -= sV[dd * ORTH_PITCH + j] * sW[j * ORTH_PITCH + k];   // W[j][k] = 0 for j > k
    P[(size_t)d * K + k] = (T)acc;
  }
}

// out[r][k] = s_k sum_d A[r][d] B[d][k],  s_k = int(X[k][k])
//   TRANS 0 (forward):  A = base,   B = P (D,K) row-major,      out = F (K,D):   F[k][r]
//   TRANS 1 (backward): A = base^T, B[d][k] = gF[k][d] (K,D),   out = gP (D,K):  gP[r][k]
template <typename T, int TRANS>
__global__ __launch_bounds__(256) void orth_product_kernel(const T* __restrict__ base, const T* __restrict__ B,
                                                           const T* __restrict__ X, int K, int D, T* __restrict__ out) {
  __shared__ T sA[ORTH_TD * (ORTH_TR + 1)];
  __shared__ T sB[ORTH_TD * ORTH_PITCH];
  constexpr int NA = ORTH_TD * ORTH_TR / 256;   // 8
  constexpr int NB = ORTH_TD * ORTH_KMAX / 256; // 16
  const int tid = threadIdx.x, r0 = blockIdx.x * ORTH_TR;
  const int rr = tid % ORTH_TR, kq = tid / ORTH_TR;   // 32 rows x 8 filter slots; slot kq takes k = kq, kq + 8, ...
  const int nB = ORTH_TD * K;
  T ra[NA], rb[NB];
  auto fetch = [&](int d0) {
#pragma unroll
    for (int u = 0; u < NA; ++u) {
      int ar, ad;
      if (TRANS) { ar = tid % ORTH_TR; ad = tid / ORTH_TR + 8 * u; }
      else { ad = tid % ORTH_TD; ar = tid / ORTH_TD + 4 * u; }
      const int r = r0 + ar, d = d0 + ad;
      const bool ok = r < D && d < D;
      const size_t off = TRANS ? (size_t)d * D + r : (size_t)r * D + d;
      const T v = base[ok ? off : 0];
      ra[u] = ok ? v : T(0);
    }
#pragma unroll
    for (int u = 0; u < NB; ++u) {
      const int idx = tid + 256 * u;
      int bd, bk;
      if (TRANS) { bd = idx % ORTH_TD; bk = idx / ORTH_TD; }
      else { bd = idx / K; bk = idx % K; }
      const int d = d0 + bd;
      const bool ok = idx < nB && d < D;
      const size_t off = TRANS ? (size_t)bk * D + d : (size_t)d * K + bk;
      const T v = B[ok ? off : 0];
      rb[u] = ok ? v : T(0);
    }
  };
  auto stage = [&]() {
#pragma unroll
    for (int u = 0; u < NA; ++u) {
      int ar, ad;
      if (TRANS) { ar = tid % ORTH_TR; ad = tid / ORTH_TR + 8 * u; }
      else { ad = tid % ORTH_TD; ar = tid / ORTH_TD + 4 * u; }
      sA[ad * (ORTH_TR + 1) + ar] = ra[u];
    }
#pragma unroll
    for (int u = 0; u < NB; ++u) {
      const int idx = tid + 256 * u;
      int bd, bk;
      if (TRANS) { bd = idx % ORTH_TD; bk = idx / ORTH_TD; }
      else { bd = idx / K; bk = idx % K; }
      if (idx < nB) sB[bd * ORTH_PITCH + bk] = rb[u];
    }
  };
  T acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = T(0);
  fetch(0);
  for (int d0 = 0; d0 < D; d0 += ORTH_TD) {
    __syncthreads();   // the previous chunk has been consumed
    stage();
    __syncthreads();
    if (d0 + ORTH_TD < D) fetch(d0 + ORTH_TD);
    for (int dd = 0; dd < ORTH_TD; ++dd) {
      const T a = sA[dd * (ORTH_TR + 1) + rr];
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (8 * j < K) acc[j] += a * sB[dd * ORTH_PITCH + (kq + 8 * j < K ? kq + 8 * j : 0)];
    }
  }
  const int r = r0 + rr;
  if (r >= D) return;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int k = kq + 8 * j;
    if (k < K) {
      const T s = (T)(int)X[(size_t)k * D + k];
      if (TRANS) out[(size_t)r * K + k] = s * acc[j];
      else out[(size_t)k * D + r] = s * acc[j];
    }
  }
}

// gV[d][i] = -sum_k gP[d][k] W[i][k] + [d < K] Z[i][d] + sum_b V[d][b] S[b][i];  gX[i][d] = d > i ? gV[d][i] : 0
template <typename T>
__global__ __launch_bounds__(256) void orth_gv_kernel(const T* __restrict__ X, const T* __restrict__ gP, int K, int D,
                                                      const double* __restrict__ Wg, const double* __restrict__ Zg,
                                                      const double* __restrict__ Sg, T* __restrict__ gX) {
  __shared__ double sM[ORTH_KMAX * ORTH_PITCH];
  __shared__ double sV[ORTH_GV_ROWS * ORTH_PITCH];
  __shared__ double sG[ORTH_GV_ROWS * ORTH_PITCH];
  const int tid = threadIdx.x, d0 = blockIdx.x * ORTH_GV_ROWS;
  for (int e = tid; e < K * K; e += 256) sM[(e / K) * ORTH_PITCH + e % K] = Wg[e];
  for (int idx = tid; idx < ORTH_GV_ROWS * K; idx += 256) {
    const int dd = idx % ORTH_GV_ROWS, i = idx / ORTH_GV_ROWS, d = d0 + dd;
    sV[dd * ORTH_PITCH + i] = d < D ? orth_v(X, D, d, i) : 0.0;
    const int gd = idx / K, gk = idx % K;
    sG[gd * ORTH_PITCH + gk] = d0 + gd < D ? (double)gP[(size_t)(d0 + gd) * K + gk] : 0.0;
  }
  __syncthreads();
  constexpr int NE = ORTH_GV_ROWS * ORTH_KMAX / 256;   // 4
  double acc[NE];
#pragma unroll
  for (int u = 0; u < NE; ++u) {
    const int e = tid + 256 * u, dd = e % ORTH_GV_ROWS, i = e / ORTH_GV_ROWS;
    acc[u] = 0.0;
    if (i < K)
      for (int k = 0; k < K; ++k) acc[u] -= sG[dd * ORTH_PITCH + k] * sM[i * ORTH_PITCH + k];
  }
  __syncthreads();
  for (int e = tid; e < K * K; e += 256) sM[(e / K) * ORTH_PITCH + e % K] = Sg[e];
  __syncthreads();
#pragma unroll
  for (int u = 0; u < NE; ++u) {
    const int e = tid + 256 * u, dd = e % ORTH_GV_ROWS, i = e / ORTH_GV_ROWS, d = d0 + dd;
    if (i >= K || d >= D) continue;
    double g = acc[u];
    for (int b = 0; b < K; ++b) g += sV[dd * ORTH_PITCH + b] * sM[b * ORTH_PITCH + i];
    if (d < K) g += Zg[i * K + d];
    gX[(size_t)i * D + d] = d > i ? (T)g : T(0);
  }
}

// workspace: [G partials (nblk,K,K)] [gW partials (nblk,K,K)] [W] [Z] [S] (K,K) double; [P | gP (D,K) dtype]
struct OrthLayout {
  int nblk;
  size_t off_g, off_gw, off_w, off_z, off_s, off_p, total;
};
static bool orth_layout(int K, int D, int dtype, OrthLayout* out) {
  if (K < 1 || K > ORTH_KMAX || K >= D || (dtype != SQFA_F32 && dtype != SQFA_F64)) return false;
  OrthLayout w;
  w.nblk = (D + ORTH_ROWS - 1) / ORTH_ROWS;
  const size_t kk = (size_t)K * K * sizeof(double), esz = dtype == SQFA_F32 ? 4 : 8;
  size_t o = 0;
  w.off_g = o;  o = align256(o + (size_t)w.nblk * kk);
  w.off_gw = o; o = align256(o + (size_t)w.nblk * kk);
  w.off_w = o;  o = align256(o + kk);
  w.off_z = o;  o = align256(o + kk);
  w.off_s = o;  o = align256(o + kk);
  w.off_p = o;  o = align256(o + (size_t)D * K * esz);
  w.total = o;
  *out = w;
  return true;
}

static int orth_check(const void* X, const void* base, const void* io, const void* out, int K, int D, int dtype,
                      const void* workspace, size_t workspace_bytes, OrthLayout* w) {
  if (X == nullptr || base == nullptr || io == nullptr || out == nullptr) return SQFA_ERR_BAD_ARGUMENT;
  if (K < 1 || K >= D || (dtype != SQFA_F32 && dtype != SQFA_F64)) return SQFA_ERR_BAD_ARGUMENT;
  if (K > ORTH_KMAX) return SQFA_ERR_UNSUPPORTED_M;
  if (!orth_layout(K, D, dtype, w)) return SQFA_ERR_UNSUPPORTED_M;
  if (workspace == nullptr || workspace_bytes < w->total) return SQFA_ERR_WORKSPACE;
  return SQFA_OK;
}

template <typename T>
static hipError_t orth_forward(const void* X_, const void* base_, int K, int D, void* F_, unsigned char* ws,
                               const OrthLayout& w, hipStream_t stream) {
  const T* X = static_cast<const T*>(X_);
  double* Gpart = reinterpret_cast<double*>(ws + w.off_g);
  double* Wg = reinterpret_cast<double*>(ws + w.off_w);
  T* P = reinterpret_cast<T*>(ws + w.off_p);
  hipLaunchKernelGGL(orth_gram_kernel<T>, dim3(w.nblk), dim3(256), 0, stream, X, (const T*)nullptr, K, D, Gpart,
                     (double*)nullptr);
  hipLaunchKernelGGL(orth_solve_kernel<T>, dim3(1), dim3(256), 0, stream, X, K, D, w.nblk, (const double*)Gpart,
                     (const double*)nullptr, Wg, (double*)nullptr, (double*)nullptr);
  hipLaunchKernelGGL(orth_p_kernel<T>, dim3(w.nblk), dim3(256), 0, stream, X, K, D, (const double*)Wg, P);
  hipLaunchKernelGGL((orth_product_kernel<T, 0>), dim3((D + ORTH_TR - 1) / ORTH_TR), dim3(256), 0, stream,
                     static_cast<const T*>(base_), (const T*)P, X, K, D, static_cast<T*>(F_));
  return hipGetLastError();
}

template <typename T>
static hipError_t orth_backward(const void* X_, const void* base_, const void* gF_, int K, int D, void* gX_,
                                unsigned char* ws, const OrthLayout& w, hipStream_t stream) {
  const T* X = static_cast<const T*>(X_);
  double* Gpart = reinterpret_cast<double*>(ws + w.off_g);
  double* gWpart = reinterpret_cast<double*>(ws + w.off_gw);
  double* Wg = reinterpret_cast<double*>(ws + w.off_w);
  double* Zg = reinterpret_cast<double*>(ws + w.off_z);
  double* Sg = reinterpret_cast<double*>(ws + w.off_s);
  T* gP = reinterpret_cast<T*>(ws + w.off_p);
  hipLaunchKernelGGL((orth_product_kernel<T, 1>), dim3((D + ORTH_TR - 1) / ORTH_TR), dim3(256), 0, stream,
                     static_cast<const T*>(base_), static_cast<const T*>(gF_), X, K, D, gP);
  hipLaunchKernelGGL(orth_gram_kernel<T>, dim3(w.nblk), dim3(256), 0, stream, X, (const T*)gP, K, D, Gpart, gWpart);
  hipLaunchKernelGGL(orth_solve_kernel<T>, dim3(1), dim3(256), 0, stream, X, K, D, w.nblk, (const double*)Gpart,
                     (const double*)gWpart, Wg, Zg, Sg);
  hipLaunchKernelGGL(orth_gv_kernel<T>, dim3((D + ORTH_GV_ROWS - 1) / ORTH_GV_ROWS), dim3(256), 0, stream, X,
                     (const T*)gP, K, D, (const double*)Wg, (const double*)Zg, (const double*)Sg, static_cast<T*>(gX_));
  return hipGetLastError();
}

}  // namespace sqfa

using namespace sqfa;

extern "C" size_t sqfa_orthogonal_workspace_bytes(int K, int D, int dtype) {
  OrthLayout w;
  return orth_layout(K, D, dtype, &w) ? w.total : 0;
}

extern "C" int sqfa_orthogonal_forward(const void* X, const void* base, int K, int D, int dtype, void* F_out,
                                       void* workspace, size_t workspace_bytes, void* stream_) {
  OrthLayout w;
  const int rc = orth_check(X, base, X, F_out, K, D, dtype, workspace, workspace_bytes, &w);
  if (rc != SQFA_OK) return rc;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  unsigned char* ws = static_cast<unsigned char*>(workspace);
  const hipError_t e = dtype == SQFA_F32 ? orth_forward<float>(X, base, K, D, F_out, ws, w, stream)
                                         : orth_forward<double>(X, base, K, D, F_out, ws, w, stream);
  return e == hipSuccess ? SQFA_OK : SQFA_ERR_LAUNCH;
}

extern "C" int sqfa_orthogonal_backward(const void* X, const void* base, const void* gF, int K, int D, int dtype,
                                        void* gX_out, void* workspace, size_t workspace_bytes, void* stream_) {
  OrthLayout w;
  const int rc = orth_check(X, base, gF, gX_out, K, D, dtype, workspace, workspace_bytes, &w);
  if (rc != SQFA_OK) return rc;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  unsigned char* ws = static_cast<unsigned char*>(workspace);
  const hipError_t e = dtype == SQFA_F32 ? orth_backward<float>(X, base, gF, K, D, gX_out, ws, w, stream)
                                         : orth_backward<double>(X, base, gF, K, D, gX_out, ws, w, stream);
  return e == hipSuccess ? SQFA_OK : SQFA_ERR_LAUNCH;
}
