// pair_kernel_lds.hpp -- host-side interface of the LDS pair path (pair_kernel_lds.hip) for 64 < m <= 128.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace sqfa {

struct PairParams;

constexpr int kRegMaxDim = 64;    // largest size of the register-resident pair kernels (configs.hpp)
constexpr int kLdsMaxDim = 128;   // largest size of the LDS pair path

// padded size of the LDS path: identity padding to a multiple of 8 is exact (padded eigenvalues are 1)
inline int lds_padded_size(int m) { return (m + 7) / 8 * 8; }
// 4 lanes per rotation, MR / 2 rotations per step, whole waves
inline int lds_pair_threads(int MR) { return (2 * MR + 63) / 64 * 64; }
// X (MR columns, pitch MR + 1), lambda, two coefficient vectors, one reduction slot per wave
inline size_t lds_pair_shared_bytes(int MR, size_t esz) {
  return ((size_t)MR * (MR + 1) + 3 * (size_t)MR + lds_pair_threads(MR) / 64) * esz;
}

// K0L: Cholesky factor (LT, may be NULL) and packed inverse (Linv, may be NULL) of n classes S (n, m, m); row_start != NULL:
// block 0 also writes the slab slot table for the tiling in p (TI A classes per tile).
hipError_t launch_lds_prologue(int dtype_f64, const void* S, int n, int m, int MR, void* LT, void* Linv, int* row_start,
                               const PairParams& p, int TI, hipStream_t stream);
// K1L: the pair tiles of this shard (p.tj B classes per tile, TI A classes per tile)
hipError_t launch_pair_lds(int dtype_f64, const PairParams& p, int TI, int MR, hipStream_t stream);
// the same tiles for the Bures-Wasserstein distance (sqfa_bw_pairwise: p.Linv holds R_j, p.trA / trB / slab_h set)
hipError_t launch_pair_lds_bw(int dtype_f64, const PairParams& p, int TI, int MR, hipStream_t stream);

}  // namespace sqfa
