// sqfa_api.hip -- C ABI (include/sqfa_hip.h), per-class Cholesky prologue and slab reduction.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <mutex>
#include <utility>
#include <vector>

#include "../../include/sqfa_hip.h"
#include "class_pair_loss.hpp"   // align256
#include "configs.hpp"
#include "pair_kernel.hpp"
#include "pair_kernel_2d.hpp"
#include "pair_kernel_lds.hpp"

namespace sqfa {

// ---- per-configuration launchers (defined in pair_inst.hip translation units) -----------
#define SQFA_DECL_F32(T, MR, G, CPL, TJ, WV) \
  hipError_t launch_pair_f32_##MR(const PairParams&, hipStream_t);   \
  hipError_t launch_pair_bw_f32_##MR(const PairParams&, hipStream_t); \
  hipError_t launch_factor_f32_##MR(const PairParams&, hipStream_t); \
  hipError_t launch_prologue_f32_##MR(const PairParams&, const void*, void*, hipStream_t); \
  hipError_t launch_classeig_f32_##MR(const void*, int, int, double*, double*, hipStream_t);
#define SQFA_DECL_F64(T, MR, G, CPL, TJ, WV) \
  hipError_t launch_pair_f64_##MR(const PairParams&, hipStream_t);   \
  hipError_t launch_pair_bw_f64_##MR(const PairParams&, hipStream_t); \
  hipError_t launch_factor_f64_##MR(const PairParams&, hipStream_t); \
  hipError_t launch_prologue_f64_##MR(const PairParams&, const void*, void*, hipStream_t); \
  hipError_t launch_classeig_f64_##MR(const void*, int, int, double*, double*, hipStream_t);
SQFA_CONFIGS_F32(SQFA_DECL_F32)
SQFA_CONFIGS_F64(SQFA_DECL_F64)
#define SQFA_DECL_F32S(T, MR, G, CPL, TJ, WV) \
  hipError_t launch_pair_f32s_##MR(const PairParams&, hipStream_t);  \
  hipError_t launch_pair_bw_f32s_##MR(const PairParams&, hipStream_t); \
  hipError_t launch_factor_f32s_##MR(const PairParams&, hipStream_t); \
  hipError_t launch_prologue_f32s_##MR(const PairParams&, const void*, void*, hipStream_t);
SQFA_CONFIGS_F32_SMALL(SQFA_DECL_F32S)
#define SQFA_DECL_F64S(T, MR, G, CPL, TJ, WV) \
  hipError_t launch_pair_f64s_##MR(const PairParams&, hipStream_t);  \
  hipError_t launch_pair_bw_f64s_##MR(const PairParams&, hipStream_t); \
  hipError_t launch_factor_f64s_##MR(const PairParams&, hipStream_t); \
  hipError_t launch_prologue_f64s_##MR(const PairParams&, const void*, void*, hipStream_t);
SQFA_CONFIGS_F64_SMALL(SQFA_DECL_F64S)

#define SQFA_DECL2D_F32(T, MR, GC, CPL, TJ, WV, RS) \
  hipError_t launch_pair2d_f32_##MR(const PairParams&, hipStream_t); \
  hipError_t launch_pair2d_bw_f32_##MR(const PairParams&, hipStream_t); \
  hipError_t launch_factor2d_f32_##MR(const PairParams&, hipStream_t); \
  hipError_t launch_prologue2d_f32_##MR(const PairParams&, const void*, void*, hipStream_t); \
  hipError_t launch_classeig2d_f32_##MR(const void*, int, int, double*, double*, hipStream_t);
#define SQFA_DECL2D_F64(T, MR, GC, CPL, TJ, WV, RS) \
  hipError_t launch_pair2d_f64_##MR(const PairParams&, hipStream_t); \
  hipError_t launch_pair2d_bw_f64_##MR(const PairParams&, hipStream_t); \
  hipError_t launch_factor2d_f64_##MR(const PairParams&, hipStream_t); \
  hipError_t launch_prologue2d_f64_##MR(const PairParams&, const void*, void*, hipStream_t); \
  hipError_t launch_classeig2d_f64_##MR(const void*, int, int, double*, double*, hipStream_t);
SQFA_CONFIGS2D_F32(SQFA_DECL2D_F32)
SQFA_CONFIGS2D_F64(SQFA_DECL2D_F64)

struct Geometry {
  int dtype, MR, TJ, TI, WV;  // TJ: widest tile (B classes); a launch may use TJ/2, TJ/4 ... >= WV
  hipError_t (*launch)(const PairParams&, hipStream_t);
  hipError_t (*factor)(const PairParams&, hipStream_t);  // K0b, the class factor pass
  hipError_t (*eig)(const void*, int, int, double*, double*, hipStream_t);  // per-class eigen-decomposition (regular rows)
  hipError_t (*launch_bw)(const PairParams&, hipStream_t);  // the row's Bures-Wasserstein tile kernel
  hipError_t (*prologue)(const PairParams&, const void*, void*, hipStream_t);  // K0 + K0b of the A side in one launch (class_prologue_kernel); NULL: the row has none (no factor pass, or m > 24)
  bool mean_metric;       // the row's factor pass runs in the metric of the mean class (Cfg::MEAN_METRIC)
  long factor_min_pairs;  // Cfg::FACTOR_MIN_PAIRS: launches with fewer pairs per shard skip the factor pass
};
// One row of the table: the numbers come from the configuration type (PairCfg or PairCfg2D), the launchers by name.
template <typename Cfg>
static Geometry make_geometry(decltype(Geometry::launch) launch, decltype(Geometry::factor) factor, decltype(Geometry::eig) eig,
                              decltype(Geometry::launch_bw) launch_bw, decltype(Geometry::prologue) prologue) {
  return Geometry{sizeof(typename Cfg::type) == 4 ? SQFA_F32 : SQFA_F64, Cfg::MR, Cfg::TJ, Cfg::TI, Cfg::WAVES, launch, factor, eig,
                  launch_bw, has_class_prologue<Cfg>() ? prologue : nullptr, Cfg::MEAN_METRIC, Cfg::FACTOR_MIN_PAIRS};
}

// The geometry table: every whole-column row (pair_kernel.hpp) and every 2-D row (pair_kernel_2d.hpp: GC column lanes x 2
// row lanes per pair) of configs.hpp; a problem of size m runs on the smallest MR >= m.  A launch with few pairs (`pairs` =
// pairs per shard; < 0: not known, regular rows only) takes the small-launch row of that MR if there is one (configs.hpp,
// SQFA_CONFIGS_F32_SMALL).  geometry_mode: sqfa_airm_options::geometry_policy of the call (0 by pair count, 1 small-launch
// rows wherever one exists, -1 never) -- a per-call argument, no process-wide state.
static bool find_geometry(int m, int dtype, long pairs, Geometry* out, int geometry_mode = 0) {
  bool found = false;
  Geometry best{};
  auto consider = [&](const Geometry& g) {
    if (g.dtype == dtype && m <= g.MR && (!found || g.MR < best.MR)) {
      best = g;
      found = true;
    }
  };
  // same padded size, more lanes per pair; the per-class eigen-decomposition stays the regular row's
  auto consider_small = [&](Geometry g, long max_pairs) {
    g.eig = best.eig;
    if (g.dtype == dtype && g.MR == best.MR && (geometry_mode > 0 || pairs < max_pairs)) best = g;
  };
#define SQFA_ROW_F32(T, MR, G, CPL, TJ, WV) \
  consider(make_geometry<PairCfg<T, MR, G, CPL, TJ, WV>>(launch_pair_f32_##MR, launch_factor_f32_##MR, launch_classeig_f32_##MR, launch_pair_bw_f32_##MR, launch_prologue_f32_##MR));
#define SQFA_ROW_F64(T, MR, G, CPL, TJ, WV) \
  consider(make_geometry<PairCfg<T, MR, G, CPL, TJ, WV>>(launch_pair_f64_##MR, launch_factor_f64_##MR, launch_classeig_f64_##MR, launch_pair_bw_f64_##MR, launch_prologue_f64_##MR));
#define SQFA_ROW2D_F32(T, MR, GC, CPL, TJ, WV, RS) \
  consider(make_geometry<PairCfg2D<T, MR, GC, CPL, TJ, WV, RS>>(launch_pair2d_f32_##MR, launch_factor2d_f32_##MR, launch_classeig2d_f32_##MR, launch_pair2d_bw_f32_##MR, launch_prologue2d_f32_##MR));
#define SQFA_ROW2D_F64(T, MR, GC, CPL, TJ, WV, RS) \
  consider(make_geometry<PairCfg2D<T, MR, GC, CPL, TJ, WV, RS>>(launch_pair2d_f64_##MR, launch_factor2d_f64_##MR, launch_classeig2d_f64_##MR, launch_pair2d_bw_f64_##MR, launch_prologue2d_f64_##MR));
#define SQFA_ROW_F32S(T, MR, G, CPL, TJ, WV) \
  consider_small(make_geometry<PairCfg<T, MR, G, CPL, TJ, WV>>(launch_pair_f32s_##MR, launch_factor_f32s_##MR, nullptr, launch_pair_bw_f32s_##MR, launch_prologue_f32s_##MR), small_launch_max_pairs(MR));
#define SQFA_ROW_F64S(T, MR, G, CPL, TJ, WV) \
  consider_small(make_geometry<PairCfg<T, MR, G, CPL, TJ, WV>>(launch_pair_f64s_##MR, launch_factor_f64s_##MR, nullptr, launch_pair_bw_f64s_##MR, launch_prologue_f64s_##MR), small_launch_max_pairs_f64(MR));
  SQFA_CONFIGS_F32(SQFA_ROW_F32)
  SQFA_CONFIGS_F64(SQFA_ROW_F64)
  SQFA_CONFIGS2D_F32(SQFA_ROW2D_F32)
  SQFA_CONFIGS2D_F64(SQFA_ROW2D_F64)
  if (found && geometry_mode >= 0 && pairs >= 0) {
    SQFA_CONFIGS_F32_SMALL(SQFA_ROW_F32S)
    SQFA_CONFIGS_F64_SMALL(SQFA_ROW_F64S)
  }
  if (found) *out = best;
  return found;
}
static long pair_count(int nA, int nB, int shard_count) {  // pairs per shard of a call (nB == 0: self mode)
  const long p = nB == 0 ? (long)nA * (nA - 1) / 2 : (long)nA * nB;
  return p / (shard_count > 0 ? shard_count : 1);
}

// The per-class SPD functions (Cholesky + class_eig_kernel) exist for the register geometries only.
constexpr int kSpdMaxDim = kRegMaxDim;

static thread_local char g_last_error[256] = "";

// optional per-launch timing of the pair tile kernel with HIP events on the caller's stream
struct EventPair { hipEvent_t a, b; };
static std::atomic<bool> g_profile{false};
static std::vector<EventPair> g_events;
static std::mutex g_events_mutex;  // the event lists are shared by every host thread that calls into the library
}  // namespace sqfa
// shared with project_kernel.hip
bool sqfa_profile_enabled() { return sqfa::g_profile.load(); }
std::vector<std::pair<hipEvent_t, hipEvent_t>>& sqfa_project_events() {
  static std::vector<std::pair<hipEvent_t, hipEvent_t>> ev;
  return ev;
}
std::mutex& sqfa_project_events_mutex() {
  static std::mutex m;
  return m;
}
namespace sqfa {

struct WorkspaceLayout {
  size_t off_lt, off_linv, off_slab, off_loss, off_flag, off_rows, off_mean, total;
};
constexpr int kMeanParts = 32;   // class groups of the mean-class partial sums (mean_partial_kernel)

// Tiles of a shard for tiles of TI x tj classes (same enumeration as the kernels' compact grid).
static long shard_tiles(int nA, int nBeff, int TI, int tj, int self_mode, int shard_index, int shard_count) {
  const int nbi = (nA + TI - 1) / TI, nbj = (nBeff + tj - 1) / tj;
  long n = 0;
  for (int bi = 0; bi < nbi; ++bi) {
    int first;
    n += shard_tiles_in_row(bi, tiles_in_row(bi, nbj, TI, tj, self_mode), shard_index, shard_count, &first);
  }
  return n;
}

// Workgroups the chip holds at once (4 per CU for the 256-thread configurations); a launch with
// fewer tiles than this runs for one tile's latency however few they are, so tiles are narrowed.
static int resident_workgroups() {
  static int cached = 0;
  if (cached == 0) {
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    cached = 4 * (cus > 0 ? cus : 256);
  }
  return cached;
}

// Tile widths a launch may use: the configuration's TJ, and its halvings (down to the wave
// count) as long as the job then has at most 16 x the resident workgroups in tiles -- narrowing
// only ever helps launches that do not fill the chip, and the bound keeps the slab small.
static bool width_allowed(int nA, int nBeff, const Geometry& g, int tj, int self_mode) {
  if (tj == g.TJ) return true;
  if (tj < g.WV || tj < 1 || g.TJ % tj != 0) return false;
  return shard_tiles(nA, nBeff, g.TI, tj, self_mode, 0, 1) <= 16L * resident_workgroups();
}

// ... while the launch has fewer than SQFA_TILE_ROUNDS x the resident workgroups in tiles.  2 since round 3: a launch of
// just over one round of workgroups (m <= 8 at C=1000: ~1000 tiles of 64 x 8 pairs) ends with half the chip idle for
// one tile's duration; measured C=1000, m=8 0.218 -> 0.202 ms, m=4 likewise; sizes with >= 2 rounds are unaffected
// (m=16 1.050 vs 1.041-1.048 ms with the narrowest tiles: within noise, and they double the A-side slab).
#ifndef SQFA_TILE_ROUNDS
#define SQFA_TILE_ROUNDS 2
#endif
// Tile width a call with `shard_count` shards uses: halved while a shard's launch would leave workgroup
// slots empty.  Decided from the TOTAL tile count and shard_count only, so that every shard of a job
// picks the same tiling (tile ownership (bi + bj) % shard_count is defined on that tiling).
static int choose_tile_width(int nA, int nBeff, const Geometry& g, int self_mode, int shard_count) {
  int tj = g.TJ;
  while (tj % 2 == 0 && width_allowed(nA, nBeff, g, tj / 2, self_mode) &&
         shard_tiles(nA, nBeff, g.TI, tj, self_mode, 0, 1) / shard_count < (long)SQFA_TILE_ROUNDS * resident_workgroups())
    tj /= 2;
  return tj;
}

// The tiling and the workspace of one call: what every size query and every pairwise entry point derives, once, from
// (nA, nB, m, dtype, shard_count, geometry policy).  m <= 64 runs a register row of the geometry table (`g`), 64 < m <= 128
// the LDS pair path (pair_kernel_lds.hip: nothing of `g` is involved, no class factor pass).
struct PairPlan {
  int nA, m, dtype, shard_count;
  int nBeff, self_mode;  // B classes (self mode, nB == 0: the A classes)
  size_t esz;
  bool lds;
  int MR, TI, TJ, tj;    // padded size; A classes per tile; the widest tile and the width this call uses (B classes)
  int nbi, nbj;          // tile rows, and tile columns of width tj
  Geometry g;            // register rows only
  WorkspaceLayout w;
};

// Workspace of a register row for exactly the plan's tile width, or (any_width) for the narrowest tiles any call may
// choose: most tiles, largest slab.
static WorkspaceLayout layout(const PairPlan& pl, bool any_width) {
  WorkspaceLayout w;
  const Geometry& g = pl.g;
  const size_t mat = (size_t)g.MR * g.MR * pl.esz;
  const size_t tri = (size_t)g.MR * (g.MR + 1) / 2;
  size_t slab = 0, tiles = 0;
  for (int tj = g.TJ; tj >= 1 && width_allowed(pl.nA, pl.nBeff, g, tj, pl.self_mode); tj /= 2) {
    if (!any_width && tj != pl.tj) {
      if (tj % 2) break;
      continue;
    }
    // the slab holds the tiles one shard owns (compact numbering): the largest shard decides
    size_t owned = 0;
    for (int r = 0; r < pl.shard_count; ++r)
      owned = std::max(owned, (size_t)shard_tiles(pl.nA, pl.nBeff, g.TI, tj, pl.self_mode, r, pl.shard_count));
    slab = std::max(slab, owned * (size_t)(g.TI + tj) * tri * pl.esz);
    tiles = std::max(tiles, owned);
    if (tj % 2) break;
  }
  size_t o = 0;
  w.off_lt = o;   o = align256(o + (size_t)pl.nA * mat);
  w.off_linv = o; o = align256(o + (size_t)pl.nBeff * mat);  // (packed for MR >= 32: uses about half)
  w.off_slab = o; o = align256(o + slab);
  w.off_loss = o; o = align256(o + tiles * pl.esz);
  w.off_flag = o; o = align256(o + tiles * 2 * sizeof(int));
  w.off_rows = o; o = align256(o + ((size_t)pl.nbi + 1) * sizeof(int));
  // mean-metric factor pass: kMeanParts partial sums of the A classes (MR x MR doubles each), then Lbar^-1 (MR x MR doubles)
  w.off_mean = o; o = align256(o + (size_t)(kMeanParts + 1) * g.MR * g.MR * sizeof(double));
  w.total = o;
  return w;
}
// Workspace of the LDS path: the slab holds the tiles of the largest shard (one shard: every tile, enough for any shard count)
static WorkspaceLayout layout_lds(const PairPlan& pl) {
  WorkspaceLayout w;
  size_t owned = 0;
  for (int r = 0; r < pl.shard_count; ++r)
    owned = std::max(owned, (size_t)shard_tiles(pl.nA, pl.nBeff, pl.TI, pl.tj, pl.self_mode, r, pl.shard_count));
  const size_t tri = (size_t)pl.MR * (pl.MR + 1) / 2;
  size_t o = 0;
  w.off_lt = o;   o = align256(o + (size_t)pl.nA * pl.MR * pl.MR * pl.esz);
  w.off_linv = o; o = align256(o + (size_t)pl.nBeff * tri * pl.esz);  // packed lower triangles
  w.off_slab = o; o = align256(o + owned * (size_t)(pl.TI + pl.tj) * tri * pl.esz);
  w.off_loss = o; o = align256(o + owned * pl.esz);
  w.off_flag = o; o = align256(o + owned * 2 * sizeof(int));
  w.off_rows = o; o = align256(o + ((size_t)pl.nbi + 1) * sizeof(int));
  w.off_mean = o;  // no class factor pass above 64
  w.total = o;
  return w;
}

// LDS path: one workgroup per tile of TI x TJ pairs, the pairs one after the other.  Tiles start at 16 x 16 (the slab holds
// P (1/TI + 1/TJ) lower triangles for P pairs: 2.1 GB at C = 1000, m = 128, float32) and are halved, TJ first, while the
// job has fewer than kLdsMinTiles tiles, down to 2 x 2 (C = 100: 1 275 tiles).  The tiling depends on (nA, nB, m) only:
// every shard of a job uses the same one.
constexpr long kLdsMinTiles = 1024;  // 4 x the 256 CUs

// false: no kernel for matrices of size m.  nB == 0: self mode.  geometry_mode as find_geometry; any_width: see layout().
static bool make_plan(int nA, int nB, int m, int dtype, int shard_count, int geometry_mode, PairPlan* out,
                      bool any_width = false) {
  PairPlan pl{};
  pl.nA = nA;
  pl.m = m;
  pl.dtype = dtype;
  pl.shard_count = shard_count;
  pl.self_mode = nB == 0 ? 1 : 0;
  pl.nBeff = nB == 0 ? nA : nB;
  pl.esz = dtype == SQFA_F32 ? 4 : 8;
  pl.lds = m > kRegMaxDim;
  if (pl.lds) {
    if (m > kLdsMaxDim) return false;
    pl.MR = lds_padded_size(m);
    pl.TI = pl.TJ = 16;
    while (pl.TI * pl.TJ > 4 && shard_tiles(nA, pl.nBeff, pl.TI, pl.TJ, pl.self_mode, 0, 1) < kLdsMinTiles) {
      if (pl.TJ >= pl.TI) pl.TJ /= 2;
      else pl.TI /= 2;
    }
    pl.tj = pl.TJ;
  } else {
    if (!find_geometry(m, dtype, pair_count(nA, nB, shard_count), &pl.g, geometry_mode)) return false;
    pl.MR = pl.g.MR;
    pl.TI = pl.g.TI;
    pl.TJ = pl.g.TJ;
    pl.tj = choose_tile_width(nA, pl.nBeff, pl.g, pl.self_mode, shard_count);
  }
  pl.nbi = (nA + pl.TI - 1) / pl.TI;
  pl.nbj = (pl.nBeff + pl.tj - 1) / pl.tj;
  pl.w = pl.lds ? layout_lds(pl) : layout(pl, any_width);
  *out = pl;
  return true;
}

// ---- K0: per-class Cholesky factor and its inverse (always evaluated in double) ----------
// One 256-thread workgroup per class, matrix in LDS.  LT[c][col*MR + k] = L[k][col];
// Linv[c][r*MR + k] = (L^-1)[r][k] (MR < 32) or packed Linv[c][r(r+1)/2 + k], k <= r (MR >= 32).
// Both are padded to MR x MR with an identity block.
// A non-SPD input produces NaNs, which surface as non-finite distances (nonfinite_out),
// never as a fault.
//   Cholesky: right-looking, all (r,c) entries of the trailing block updated in parallel
//   per pivot column (one LDS round trip per entry and pivot instead of a serial row loop).
//   Inverse: X = L^-1 row by row; row r needs rows < r, columns are independent; the inner
//   sum runs over k in parallel chunks of 4 lanes per column.
// (fast_rsqrt, 1/sqrt(x) in double from the hardware estimate and two Newton steps: pair_kernel.hpp, shared with the fused prologue)

// Partial sums of the class matrices for the mean class of the mean-metric factor pass: block b adds the classes b, b + P,
// b + 2P, ... (P = gridDim.x) entry by entry in that order -- fixed association, bitwise reproducible.  out[b][m*m] doubles.
template <typename T>
__global__ __launch_bounds__(256) void mean_partial_kernel(const T* __restrict__ S, int n, int m, double* __restrict__ out) {
  const int b = blockIdx.x, P = gridDim.x;
  for (int e = threadIdx.x; e < m * m; e += 256) {
    double a0 = 0.0, a1 = 0.0;
    int c = b;
    for (; c + P < n; c += 2 * P) {
      a0 += (double)S[(size_t)c * m * m + e];
      a1 += (double)S[(size_t)(c + P) * m * m + e];
    }
    if (c < n) a0 += (double)S[(size_t)c * m * m + e];
    out[(size_t)b * m * m + e] = a0 + a1;
  }
}

// mean_parts != nullptr: ONE extra block (blockIdx.x == n_classes) factorises the mean of the classes (the sum of the
// n_parts partial sums / n_classes) and writes Lbar^-1 as MR x MR row-major doubles, identity padded, to mean_linv.
template <typename T, int MAXM>
__global__ __launch_bounds__(256) void cholesky_kernel(const T* __restrict__ S, int m, int MR,
                                                       T* __restrict__ LT, T* __restrict__ Linv,
                                                       int* __restrict__ row_start, PairParams pp, int TI,
                                                       int n_classes = 0, const double* __restrict__ mean_parts = nullptr,
                                                       int n_parts = 0, double* __restrict__ mean_linv = nullptr) {
  if (row_start != nullptr && blockIdx.x == 0) write_row_start_table(pp, TI, row_start);
  // LDS sized for the padded size class (MAXM >= m) so that small problems keep many
  // workgroups per CU resident
  __shared__ double a[MAXM][MAXM + 1];
  __shared__ double b[MAXM][MAXM + 1];
  __shared__ double rd[MAXM];  // 1 / L[k][k]
  const int c = blockIdx.x, t = threadIdx.x;
  const bool mean_block = mean_parts != nullptr && c == n_classes;
  if (mean_block) {
    const double inv_n = 1.0 / (double)n_classes;
    for (int idx = t; idx < m * m; idx += 256) {
      double acc = 0.0;
      for (int q = 0; q < n_parts; ++q) acc += mean_parts[(size_t)q * m * m + idx];
      a[idx / m][idx % m] = acc * inv_n;
      b[idx / m][idx % m] = 0.0;
    }
  } else {
    const T* s = S + (size_t)c * m * m;
    for (int idx = t; idx < m * m; idx += 256) {
      a[idx / m][idx % m] = (double)s[idx];
      b[idx / m][idx % m] = 0.0;
    }
  }
  __syncthreads();
  // Right-looking elimination on the UNSCALED columns, one workgroup barrier per pivot (round 3; three before: pivot, scaled
  // column, trailing update): step k only reads column k and the pivot, which no later step writes, and subtracts
  // a[r][k] a[c][k] / a[k][k] from the trailing block; the columns are scaled by 1/sqrt(pivot) once at the end.
  // (bw_prologue_kernel repeats this loop on its own array: as one shared routine the two kernels compiled to other code.)
  for (int k = 0; k < m; ++k) {
    const double akk = a[k][k];
    // a non-positive or NaN pivot poisons the trailing block: NaN here and everywhere downstream, as with the scaled form
    double rk = __builtin_amdgcn_rcp(akk);   // hardware estimate + two Newton steps instead of the IEEE divide sequence
    rk = rk * (2.0 - akk * rk);
    rk = rk * (2.0 - akk * rk);
    if (!(akk > 0.0)) rk = __builtin_nan("");
    const int n = m - k - 1;
    for (int e = t; e < n * n; e += 256) {
      const int r = k + 1 + e / n, c2 = k + 1 + e % n;
      if (c2 <= r) a[r][c2] -= a[r][k] * a[c2][k] * rk;
    }
    __syncthreads();
  }
  for (int k = t; k < m; k += 256) rd[k] = fast_rsqrt(a[k][k]);
  __syncthreads();
  for (int e = t; e < m * m; e += 256) {
    const int r = e / m, k = e % m;
    if (k <= r) a[r][k] *= rd[k];  // r == k: akk * rs = sqrt(akk)
  }
  __syncthreads();
  // inverse X = L^-1, row by row; 4 lanes per column (always inside one wave, so rows only
  // need the wave's own program order, no workgroup barrier)
  {
    const int col = t >> 2, part = t & 3;
    for (int r = 0; r < m; ++r) {
      double acc = 0.0;
      if (col < r) {
        for (int k = col + part; k < r; k += 4) acc += a[r][k] * b[k][col];
      }
      acc += __shfl_xor(acc, 1, 64);
      acc += __shfl_xor(acc, 2, 64);
      if (part == 0 && col <= r && col < m) b[r][col] = ((col == r ? 1.0 : 0.0) - acc) * rd[r];
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
    }
  }
  __syncthreads();
  if (mean_block) {
    for (int idx = t; idx < MR * MR; idx += 256) {
      const int r = idx / MR, k = idx % MR;
      mean_linv[idx] = (r < m && k < m) ? (k <= r ? b[r][k] : 0.0) : (r == k ? 1.0 : 0.0);
    }
    return;
  }
  const size_t base = (size_t)c * MR * MR;
  for (int idx = t; idx < MR * MR; idx += 256) {
    const int r = idx / MR, k = idx % MR;
    if (LT != nullptr) {  // here r = column of L, k = row of L
      double v = (r < m && k < m) ? (k >= r ? a[k][r] : 0.0) : (r == k ? 1.0 : 0.0);
      LT[base + idx] = (T)v;
    }
    if (Linv != nullptr) {
      double v = (r < m && k < m) ? (k <= r ? b[r][k] : 0.0) : (r == k ? 1.0 : 0.0);
      if (MR >= 32) {  // packed lower triangle (PairCfg::PACK_LINV): less LDS per wave in the pair kernel
        if (k <= r) Linv[(size_t)c * (MR * (MR + 1) / 2) + tri_index(r, k)] = (T)v;
      } else {
        Linv[base + idx] = (T)v;
      }
    }
  }
}

// ---- K2: fixed-order reduction of the tile slabs ------------------------------------------
__device__ inline bool tile_processed(const PairParams& p, int bi, int bj, int TI, int TJ) {
  if (p.shard_count > 1 && (bi + bj) % p.shard_count != p.shard_index) return false;
  if (p.self_mode && (bi * TI + TI - 1 <= bj * TJ)) return false;
  return true;
}

#ifndef SQFA_K2_THREADS
#define SQFA_K2_THREADS 512  // 1024 threads (7 summation groups per class instead of 3): 29 vs 28 us at c3, no gain
#endif
// Lower-triangle entries per workgroup of finalize_kernel, and its workgroups per class: small sizes (TRI <= 256, m <= 22)
// keep one workgroup per class.  The kernel and its launch (launch_finalize) both take the numbers from here.
__host__ __device__ constexpr int finalize_epb(int tri) { return tri <= 256 ? tri : 128; }
__host__ __device__ constexpr int finalize_bpc(int tri) { return (tri + finalize_epb(tri) - 1) / finalize_epb(tri); }
// the same for finalize_bw_kernel: 256 consecutive entries per workgroup
__host__ __device__ constexpr int finalize_bw_bpc(int tri) { return (tri + 255) / 256; }
template <typename T>
__global__ __launch_bounds__(SQFA_K2_THREADS) void finalize_kernel(const PairParams p, int TI, int TJ, int MR,
                                                       T* __restrict__ gradA, T* __restrict__ gradB,
                                                       T* __restrict__ loss_out, int* __restrict__ nonfinite_out) {
  const int tid = threadIdx.x;
  const int TRI = MR * (MR + 1) / 2;
  const int n_cls = p.nA + (p.self_mode ? 0 : p.nB);
  const int b = blockIdx.x;
  __shared__ T s_part[SQFA_K2_THREADS];
  // slab slot table (written by the Cholesky prologue) staged in LDS: read from global memory inside the
  // summation loops it put a second dependent L2 round trip in front of every slab load
  constexpr int ROWS_LDS = 2048;
  __shared__ int s_rows[ROWS_LDS];
  const bool rows_staged = p.nbi + 1 <= ROWS_LDS;
  if (rows_staged) {
    for (int k = tid; k <= p.nbi; k += SQFA_K2_THREADS) s_rows[k] = p.row_start[k];
  }
  __syncthreads();
  auto row_start_of = [&](int bi) { return rows_staged ? s_rows[bi] : p.row_start[bi]; };
  // K2 geometry: a class is split over BPC workgroups of EPB consecutive lower-triangle entries each; inside a
  // workgroup NG = THREADS / EPB thread groups each sum every NG-th contributing tile (a fixed subsequence),
  // then the NG partial sums are combined in group order: short dependent chains, bitwise reproducible.
  // (One workgroup per class with THREADS / TRI groups left m >= 32 -- 528 entries -- with ONE group walking
  // ~190 tiles serially: 275 us at C=1000, m=32.)
  // Small sizes (TRI <= 256, m <= 22) keep one workgroup per class (splitting 136 entries over two
  // workgroups cost 41 vs 30 us at m=16); m=32: 289 -> 199 us.
  const int EPB = finalize_epb(TRI), NG = SQFA_K2_THREADS / EPB;
  const int BPC = finalize_bpc(TRI);
  if (b < n_cls * BPC) {
    if (!p.want_grad) return;
    const int cls = b / BPC, e_in = tid % EPB, idx = (b % BPC) * EPB + e_in, grp = tid / EPB;
    const bool a_side = cls < p.nA;
    const int c = a_side ? cls : cls - p.nA;
    T* out = a_side ? gradA : gradB;
    if (out == nullptr) return;
    const T* slab = static_cast<const T*>(p.slab_grad);
    const size_t tile_stride = (size_t)(TI + TJ) * TRI;
    const int bi_a = c / TI, pi = c % TI, bj_b = c / TJ, pj = c % TJ;
    // Only the tiles this shard owns are visited (same enumeration as the pair kernel's grid):
    //   as A class: tiles (bi_a, first_a + k N), k < n_a   (row bi_a; self mode: up to the diagonal)
    //   as B class: tiles (first_b + k N, bj_b), k < n_b   (column bj_b; self mode: checked per tile)
    const int N = p.shard_count;
    int first_a = 0, n_a = 0, first_b = 0, n_b = 0;
    if (a_side) n_a = shard_tiles_in_row(bi_a, tiles_in_row(bi_a, p.nbj, TI, TJ, p.self_mode), p.shard_index, N, &first_a);
    if (!a_side || p.self_mode) {
      first_b = ((p.shard_index - bj_b) % N + N) % N;
      n_b = p.nbi > first_b ? (p.nbi - 1 - first_b) / N + 1 : 0;
    }
    T acc = T(0);
    if (idx < TRI && grp < NG) {
      // group `grp` sums every NG-th A-side tile and every NG-th B-side tile, four independent partial sums each:
      // the loads of a thread do not depend on each other, and one accumulator made the ~60 of them one chain
      // (c3: 30 -> 17 us, m=32: 202 -> 120 us).  Fixed association order: reproducible.  (Round 2 kept a single chain
      // for float64 so that the chaotic c5 trajectory golden stayed matched; round 3 pins filter parity at well-posed
      // points instead -- goldens G6c / G7e -- and float64 takes the same order as float32.)
      T a0 = T(0), a1 = T(0), a2 = T(0), a3 = T(0);
      {
        // the q-th owned tile of block-row bi_a (bj = first_a + q N) sits in slab slot row_start + q
        const T* base = slab + (size_t)row_start_of(bi_a) * tile_stride + (size_t)pi * TRI + idx;
        int q = grp;
        for (; q + 3 * NG < n_a; q += 4 * NG) {
          a0 += base[(size_t)q * tile_stride];
          a1 += base[(size_t)(q + NG) * tile_stride];
          a2 += base[(size_t)(q + 2 * NG) * tile_stride];
          a3 += base[(size_t)(q + 3 * NG) * tile_stride];
        }
        for (; q < n_a; q += NG) a0 += base[(size_t)q * tile_stride];
      }
      {
        auto b_tile = [&](int k) -> T {
          const int bi = first_b + k * N;
          if (!tile_processed(p, bi, bj_b, TI, TJ)) return T(0);
          int slot = row_start_of(bi) + bj_b;  // single shard: every tile of the row is owned
          if (N > 1) {
            const int first_in_row = ((p.shard_index - bi) % N + N) % N;
            slot = row_start_of(bi) + (bj_b - first_in_row) / N;
          }
          return slab[(size_t)slot * tile_stride + (size_t)(TI + pj) * TRI + idx];
        };
        int k = grp;
        for (; k + 3 * NG < n_b; k += 4 * NG) {
          a0 += b_tile(k);
          a1 += b_tile(k + NG);
          a2 += b_tile(k + 2 * NG);
          a3 += b_tile(k + 3 * NG);
        }
        for (; k < n_b; k += NG) a0 += b_tile(k);
      }
      acc = (a0 + a1) + (a2 + a3);
    }
    s_part[tid] = acc;   // [grp][entry]: tid = grp * EPB + e_in
    __syncthreads();
    if (grp == 0 && idx < TRI) {
      T tot = T(0);
      for (int g2 = 0; g2 < NG; ++g2) tot += s_part[g2 * EPB + e_in];
      int r = 0;
      while ((r + 1) * (r + 2) / 2 <= idx) ++r;
      const int cc = idx - r * (r + 1) / 2;
      if (r < p.m && cc < p.m) {
        out[(size_t)c * p.m * p.m + (size_t)r * p.m + cc] = tot;
        out[(size_t)c * p.m * p.m + (size_t)cc * p.m + r] = tot;
      }
    }
    return;
  }
  // last block: loss, flag, diagonals
  __shared__ double s_l[SQFA_K2_THREADS];
  __shared__ int s_f[SQFA_K2_THREADS];
  __shared__ int s_f2[SQFA_K2_THREADS];
  double l = 0.0;
  int f = 0, f2 = 0;
  const int ntiles = row_start_of(p.nbi);   // every slab slot belongs to a tile this shard processed
  for (int tix = tid; tix < ntiles; tix += SQFA_K2_THREADS) {
    l += (double)static_cast<const T*>(p.slab_loss)[tix];
    f += p.slab_flag[2 * tix];
    f2 += p.slab_flag[2 * tix + 1];
  }
  s_l[tid] = l;
  s_f[tid] = f;
  s_f2[tid] = f2;
  __syncthreads();
  for (int st = SQFA_K2_THREADS / 2; st > 0; st >>= 1) {
    if (tid < st) {
      s_l[tid] += s_l[tid + st];
      s_f[tid] += s_f[tid + st];
      s_f2[tid] += s_f2[tid + st];
    }
    __syncthreads();
  }
  if (tid == 0) {
    if (loss_out != nullptr) loss_out[0] = (T)s_l[0];
    if (nonfinite_out != nullptr) {
      nonfinite_out[0] = s_f[0];
      nonfinite_out[1] = s_f2[0];
    }
  }
  if (p.self_mode) {
    if (p.dist_out != nullptr) {
      T* D = static_cast<T*>(p.dist_out);
      const T dv = p.sqrt_mode ? (T)sqrt(p.eps) : T(0);
      for (int c = tid; c < p.nA; c += SQFA_K2_THREADS) D[(size_t)c * p.nB + c] = dv;
    }
    if (p.eig_out != nullptr) {
      T* E = static_cast<T*>(p.eig_out);
      for (int k = tid; k < p.nA * p.m; k += SQFA_K2_THREADS) {
        const int c = k / p.m, q = k % p.m;
        E[((size_t)c * p.nB + c) * p.m + q] = T(1);
      }
    }
  }
}

// ---- Bures-Wasserstein kernels (sqfa_bw_pairwise) -------------------------------------------------------------------
// K0 (B side): per class, in double, the LOWER triangular R with R^T R = S: R = J chol(J S J)^T J (J reverses the index
// order), written where the affine-invariant path keeps L^-1 (identity padded, packed lower triangle for MR >= 32 as
// PairCfg::PACK_LINV and the LDS path), R^-1 = J L^-T J (L = chol(J S J)) as m x m doubles (the sandwich of the B-side
// gradient) and the trace.  trace_only: the trace alone (the A side, whose factor comes from the unchanged Cholesky prologue).
// One 256-thread workgroup per class; a[m][m+1] + rd[m] doubles of dynamic LDS.  A non-SPD class yields NaN, never a fault.
template <typename T>
__global__ __launch_bounds__(256) void bw_prologue_kernel(const T* __restrict__ S, int m, int MR, T* __restrict__ Rout,
                                                          double* __restrict__ Sinv, double* __restrict__ trace) {
  extern __shared__ double lds_bw[];
  const int P = m + 1, c = blockIdx.x, t = threadIdx.x;
  double* a = lds_bw;           // a[r * P + k]
  double* rd = lds_bw + m * P;  // 1 / L[k][k], then scratch
  const T* s = S + (size_t)c * m * m;
  if (trace != nullptr) {
    if (t < 64) {  // one wave, fixed order: reproducible
      double v = 0.0;
      for (int k = t; k < m; k += 64) v += (double)s[(size_t)k * m + k];
      for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
      if (t == 0) trace[c] = v;
    }
  }
  if (Rout == nullptr && Sinv == nullptr) return;
  for (int idx = t; idx < m * m; idx += 256) {
    const int r = idx / m, k = idx % m;
    a[r * P + k] = (double)s[(size_t)(m - 1 - r) * m + (m - 1 - k)];
  }
  __syncthreads();
  for (int k = 0; k < m; ++k) {  // right-looking elimination on the unscaled columns (cholesky_kernel)
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
  for (int k = t; k < m; k += 256) rd[k] = fast_rsqrt(a[k * P + k]);
  __syncthreads();
  for (int e = t; e < m * m; e += 256) {
    const int r = e / m, k = e % m;
    if (k <= r) a[r * P + k] *= rd[k];  // a: L = chol(J S J), lower
  }
  __syncthreads();
  if (Rout != nullptr) {  // R[r][k] = L[m-1-k][m-1-r], k <= r
    const bool packed = MR >= 32;
    T* R = Rout + (size_t)c * (packed ? MR * (MR + 1) / 2 : MR * MR);
    for (int idx = t; idx < MR * MR; idx += 256) {
      const int r = idx / MR, k = idx % MR;
      if (packed && k > r) continue;
      const double v = (r < m && k < m) ? (k <= r ? a[(m - 1 - k) * P + (m - 1 - r)] : 0.0) : (r == k ? 1.0 : 0.0);
      R[packed ? tri_index(r, k) : idx] = (T)v;
    }
  }
  if (Sinv == nullptr) return;
  // X = L^-1 in place: strict lower triangle stored transposed in the upper triangle (X[r][q] at a[q][r]), diagonal in rd
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
  // R^-1 = J X^T J: R^-1[r][q] = X[m-1-q][m-1-r] (lower triangular, q <= r)
  double* si = Sinv + (size_t)c * m * m;
  for (int idx = t; idx < m * m; idx += 256) {
    const int r = idx / m, q = idx % m;
    const int u = m - 1 - q, v = m - 1 - r;  // X[u][v], u >= v
    si[idx] = q > r ? 0.0 : (u == v ? rd[u] : a[v * P + u]);
  }
}

// K2 of the gradient (BW): the A-side slab rows of every class (identity terms included) -> gradA, and the B-side rows
// -> G (m x m doubles, the bracket of the B-side gradient) with the sums of slab_h -> hsum.  Self mode: A side and B side of
// one class are reduced SEPARATELY (only the B side is sandwiched).  Workgroup b: class b / BPC (A classes first, then the
// nBeff B classes), 256 consecutive lower-triangle entries; every thread sums its entry over the owned tiles in the
// enumeration order of finalize_kernel, four partial sums: fixed order, bitwise reproducible.
template <typename T>
__global__ __launch_bounds__(256) void finalize_bw_kernel(const PairParams p, int TI, int TJ, int MR, T* __restrict__ gradA,
                                                          double* __restrict__ G, double* __restrict__ hsum) {
  const int TRI = MR * (MR + 1) / 2, BPC = finalize_bw_bpc(TRI);
  const int b = blockIdx.x, cls = b / BPC, idx = (b % BPC) * 256 + threadIdx.x;
  const bool a_side = cls < p.nA;
  const int c = a_side ? cls : cls - p.nA;
  const T* slab = static_cast<const T*>(p.slab_grad);
  const size_t tile_stride = (size_t)(TI + TJ) * TRI;
  const int N = p.shard_count;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  double hacc = 0.0;
  const bool h_thread = !a_side && b % BPC == 0 && threadIdx.x == 0;
  if (a_side) {
    const int bi_a = c / TI, pi = c % TI;
    int first;
    const int n_a = shard_tiles_in_row(bi_a, tiles_in_row(bi_a, p.nbj, TI, TJ, p.self_mode), p.shard_index, N, &first);
    if (idx < TRI)
      for (int q = 0; q < n_a; ++q) acc[q & 3] += (double)slab[(size_t)(p.row_start[bi_a] + q) * tile_stride + (size_t)pi * TRI + idx];
  } else {
    const int bj_b = c / TJ, pj = c % TJ;
    const int first_b = ((p.shard_index - bj_b) % N + N) % N;
    const int n_b = p.nbi > first_b ? (p.nbi - 1 - first_b) / N + 1 : 0;
    for (int k = 0; k < n_b; ++k) {
      const int bi = first_b + k * N;
      if (p.self_mode && (bi * TI + TI - 1 <= bj_b * TJ)) continue;  // tile_processed
      int slot = p.row_start[bi] + bj_b;
      if (N > 1) slot = p.row_start[bi] + (bj_b - ((p.shard_index - bi) % N + N) % N) / N;
      if (idx < TRI) acc[k & 3] += (double)slab[(size_t)slot * tile_stride + (size_t)(TI + pj) * TRI + idx];
      if (h_thread) hacc += (double)static_cast<const T*>(p.slab_h)[(size_t)slot * TJ + pj];
    }
    if (h_thread) hsum[c] = hacc;
  }
  if (idx >= TRI) return;
  int r = 0;
  while ((r + 1) * (r + 2) / 2 <= idx) ++r;
  const int cc = idx - r * (r + 1) / 2;
  if (r >= p.m) return;
  const double tot = (acc[0] + acc[1]) + (acc[2] + acc[3]);
  const int m = p.m;
  if (a_side) {
    if (gradA != nullptr) {
      gradA[(size_t)c * m * m + (size_t)r * m + cc] = (T)tot;
      gradA[(size_t)c * m * m + (size_t)cc * m + r] = (T)tot;
    }
  } else {
    G[(size_t)c * m * m + (size_t)r * m + cc] = tot;
    G[(size_t)c * m * m + (size_t)cc * m + r] = tot;
  }
}

// B-side gradient: grad_j = hsum_j I + R_j^-1 G_j R_j^-T (G_j = -sum h sigma^-1 y y^T reduced), in double; one workgroup
// per class, W = R^-1 G through the workspace.  accumulate: self mode adds it to the A-side gradient of the same class.
template <typename T>
__global__ __launch_bounds__(256) void bw_sandwich_kernel(int m, const double* __restrict__ Sinv, const double* __restrict__ G,
                                                          double* __restrict__ W, const double* __restrict__ hsum,
                                                          T* __restrict__ out, int accumulate) {
  const int c = blockIdx.x, t = threadIdx.x;
  const double* si = Sinv + (size_t)c * m * m;
  const double* g = G + (size_t)c * m * m;
  double* w = W + (size_t)c * m * m;
  for (int idx = t; idx < m * m; idx += 256) {
    const int r = idx / m, q = idx % m;
    double acc = 0.0;
    for (int k = 0; k < m; ++k) acc += si[r * m + k] * g[k * m + q];
    w[idx] = acc;
  }
  __syncthreads();
  const double hs = hsum[c];
  T* o = out + (size_t)c * m * m;
  for (int idx = t; idx < m * m; idx += 256) {
    const int r = idx / m, q = idx % m;
    if (q > r) continue;
    double acc = r == q ? hs : 0.0;
    for (int k = 0; k < m; ++k) acc += w[r * m + k] * si[q * m + k];
    if (accumulate) {
      o[r * m + q] = (T)((double)o[r * m + q] + acc);
      if (q != r) o[q * m + r] = (T)((double)o[q * m + r] + acc);
    } else {
      o[r * m + q] = (T)acc;
      o[q * m + r] = (T)acc;
    }
  }
}

// ---- per-class matrix functions f(S) = Q f(Lambda) Q^T and their backward -----------------------------------------------
// (spd_log / spd_sqrt of the reference, src/sqfa/linalg.py:121-141, 165-183: torch.linalg.eigh + einsum there.)
// One 256-thread workgroup per class; Q (m x m, eigenvectors as columns) and the small intermediates live in LDS as
// double whatever the problem's type; m <= 64.
__device__ __forceinline__ double spd_fn(int kind, double l) {
  return kind == SQFA_SPD_LOG ? log(l) : (kind == SQFA_SPD_SQRT ? sqrt(l) : 1.0 / sqrt(l));
}
// divided difference (f(a) - f(b)) / (a - b), f'(a) on the diagonal -- in forms that stay accurate when a ~ b
// (torch's eigh backward divides by a - b: inf / NaN for repeated eigenvalues; this is its limit)
__device__ __forceinline__ double spd_fn_dd(int kind, double a, double b) {
  if (kind == SQFA_SPD_SQRT) return 1.0 / (sqrt(a) + sqrt(b));
  if (kind == SQFA_SPD_INV_SQRT) {
    const double ra = sqrt(a), rb = sqrt(b);
    return -1.0 / (ra * rb * (ra + rb));
  }
  const double r = (a - b) / b;                     // log: log1p(r) / (r b)
  if (fabs(r) < 1e-8) return (1.0 - 0.5 * r) / b;
  return log1p(r) / (r * b);
}

template <typename T>
__global__ __launch_bounds__(256) void spd_function_kernel(const double* __restrict__ U, const double* __restrict__ lam, int m,
                                                           int kind, T* __restrict__ F) {
  extern __shared__ double sh[];   // q[m][m], f[m]
  double* q = sh;
  double* f = sh + m * m;
  const int c = blockIdx.x, t = threadIdx.x;
  for (int k = t; k < m * m; k += 256) q[k] = U[(size_t)c * m * m + k];
  for (int k = t; k < m; k += 256) f[k] = spd_fn(kind, lam[(size_t)c * m + k]);
  __syncthreads();
  for (int e = t; e < m * m; e += 256) {
    const int r = e / m, cc = e % m;
    if (cc > r) continue;
    double acc = 0.0;
    for (int k = 0; k < m; ++k) acc += f[k] * q[r * m + k] * q[cc * m + k];
    F[(size_t)c * m * m + r * m + cc] = (T)acc;
    F[(size_t)c * m * m + cc * m + r] = (T)acc;   // exactly symmetric
  }
}

// gradS = Q [ (Q^T sym(G) Q) o Gamma ] Q^T,  Gamma_kl = divided difference of f at (lambda_k, lambda_l)  (Daleckii-Krein)
template <typename T>
__global__ __launch_bounds__(256) void spd_function_backward_kernel(const double* __restrict__ U, const double* __restrict__ lam,
                                                                    const T* __restrict__ G, int m, int kind, T* __restrict__ gradS) {
  extern __shared__ double sh[];   // q[m][m], a[m][m], b[m][m], l[m]
  double* q = sh;
  double* a = sh + m * m;
  double* b = sh + 2 * m * m;
  double* l = sh + 3 * m * m;
  const int c = blockIdx.x, t = threadIdx.x;
  for (int k = t; k < m * m; k += 256) q[k] = U[(size_t)c * m * m + k];
  for (int k = t; k < m; k += 256) l[k] = lam[(size_t)c * m + k];
  for (int e = t; e < m * m; e += 256) {
    const int r = e / m, cc = e % m;
    a[e] = 0.5 * ((double)G[(size_t)c * m * m + r * m + cc] + (double)G[(size_t)c * m * m + cc * m + r]);
  }
  __syncthreads();
  for (int e = t; e < m * m; e += 256) {           // b = sym(G) Q
    const int r = e / m, k = e % m;
    double acc = 0.0;
    for (int j = 0; j < m; ++j) acc += a[r * m + j] * q[j * m + k];
    b[e] = acc;
  }
  __syncthreads();
  for (int e = t; e < m * m; e += 256) {           // a = (Q^T b) o Gamma
    const int k = e / m, k2 = e % m;
    double acc = 0.0;
    for (int j = 0; j < m; ++j) acc += q[j * m + k] * b[j * m + k2];
    a[e] = acc * spd_fn_dd(kind, l[k], l[k2]);
  }
  __syncthreads();
  for (int e = t; e < m * m; e += 256) {           // b = Q a
    const int r = e / m, k2 = e % m;
    double acc = 0.0;
    for (int k = 0; k < m; ++k) acc += q[r * m + k] * a[k * m + k2];
    b[e] = acc;
  }
  __syncthreads();
  for (int e = t; e < m * m; e += 256) {           // gradS = b Q^T  (lower triangle, mirrored: exactly symmetric)
    const int r = e / m, cc = e % m;
    if (cc > r) continue;
    double acc = 0.0;
    for (int k2 = 0; k2 < m; ++k2) acc += b[r * m + k2] * q[cc * m + k2];
    gradS[(size_t)c * m * m + r * m + cc] = (T)acc;
    gradS[(size_t)c * m * m + cc * m + r] = (T)acc;
  }
}

static int fail(int code, const char* what, hipError_t e) {
  snprintf(g_last_error, sizeof(g_last_error), "%s: %s", what, e == hipSuccess ? "" : hipGetErrorString(e));
  return code;
}

// for the entry points of other translation units (jeffreys_kernel.hip): the text sqfa_hip_last_error() returns
void set_last_error(const char* text) { snprintf(g_last_error, sizeof(g_last_error), "%s", text); }

static int clamp_policy(int v) { return v > 0 ? 1 : (v < 0 ? -1 : 0); }
static bool known_dtype(int dtype) { return dtype == SQFA_F32 || dtype == SQFA_F64; }

// ---- the stages of a pairwise call, shared by both metrics and both size ranges -------------------------------------------
// Argument checks: SQFA_OK, or the error code with the message set.
static int validate_pair_call(const void* A, int nA, const void* B, int nB, int m, int dtype, int shard_index, int shard_count,
                              const void* workspace) {
  g_last_error[0] = 0;
  if (A == nullptr || nA < 1 || m < 1 || nB < 0 || workspace == nullptr) return fail(SQFA_ERR_BAD_ARGUMENT, "null/size argument", hipSuccess);
  if (!known_dtype(dtype)) return fail(SQFA_ERR_BAD_ARGUMENT, "dtype", hipSuccess);
  if ((B == nullptr) != (nB == 0)) return fail(SQFA_ERR_BAD_ARGUMENT, "B and nB disagree", hipSuccess);
  if (shard_count < 1 || shard_index < 0 || shard_index >= shard_count) return fail(SQFA_ERR_BAD_ARGUMENT, "shard", hipSuccess);
  if (B == nullptr && nA < 2) return fail(SQFA_ERR_BAD_ARGUMENT, "self mode needs at least two classes", hipSuccess);
  if (m > kLdsMaxDim) return fail(SQFA_ERR_UNSUPPORTED_M, "matrix size not supported", hipSuccess);
  return SQFA_OK;
}

// The parameter block of a call on the workspace `ws`; the caller adds what belongs to its metric alone (affine-invariant:
// EW, eig_out, mean_linv; Bures-Wasserstein: trA, trB, slab_h).
static PairParams make_pair_params(const PairPlan& pl, char* ws, int shard_index, double scale, double eps, int sqrt_mode,
                                   const void* pair_weights, double uniform_weight, bool want_grad, void* dist_out,
                                   const sqfa_airm_options* options) {
  PairParams p;
  memset(&p, 0, sizeof(p));
  p.LT = ws + pl.w.off_lt;
  p.Linv = ws + pl.w.off_linv;
  p.W = pair_weights;
  p.slab_grad = ws + pl.w.off_slab;
  p.slab_loss = ws + pl.w.off_loss;
  p.slab_flag = reinterpret_cast<int*>(ws + pl.w.off_flag);
  p.row_start = reinterpret_cast<int*>(ws + pl.w.off_rows);
  p.dist_out = dist_out;
  p.sweep_counter = options ? options->sweep_counter : nullptr;
  p.nA = pl.nA;
  p.nB = pl.nBeff;
  p.m = pl.m;
  p.self_mode = pl.self_mode;
  p.sqrt_mode = sqrt_mode ? 1 : 0;
  p.want_grad = want_grad ? 1 : 0;
  p.shard_index = shard_index;
  p.shard_count = pl.shard_count;
  p.nbi = pl.nbi;
  p.nbj = pl.nbj;
  p.tj = pl.tj;
  p.factor_mode = pl.lds ? -1 : (options ? clamp_policy(options->class_factor_policy) : 0);  // no class factor pass above 64
  p.scale = scale;
  p.eps = eps;
  p.uniform_weight = uniform_weight;
  p.scale_f = (float)scale;
  p.eps_f = (float)eps;
  p.uniform_weight_f = (float)uniform_weight;
  return p;
}

// cholesky_kernel for n classes S (n, m, m) of element type `dtype`, LDS sized for the size class of m (m <= 64).
// mean_parts != NULL: one more block factorises the mean class (see the kernel).
static void launch_cholesky(int dtype, int m, hipStream_t stream, const void* S, int n, int MR, void* LT, void* Linv,
                            int* row_start, const PairParams& p, int TI, const double* mean_parts = nullptr, int n_parts = 0,
                            double* mean_linv = nullptr) {
  const int blocks = n + (mean_parts != nullptr ? 1 : 0);
  auto launch = [&](auto zero) {
    using T = decltype(zero);
    auto kernel = m <= 16 ? cholesky_kernel<T, 16> : (m <= 32 ? cholesky_kernel<T, 32> : cholesky_kernel<T, 64>);
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), 0, stream, static_cast<const T*>(S), m, MR, static_cast<T*>(LT),
                       static_cast<T*>(Linv), row_start, p, TI, n, mean_parts, n_parts, mean_linv);
  };
  if (dtype == SQFA_F32) launch(0.0f);
  else launch(0.0);
}

// K0 for one side of a call: the factor (LT, may be NULL) and the inverse factor (Linv, may be NULL) of n classes;
// row_start != NULL: the launch also writes the slab slot table.
static hipError_t launch_factors(const PairPlan& pl, const PairParams& p, hipStream_t stream, const void* S, int n, void* LT,
                                 void* Linv, int* row_start, const double* mean_parts = nullptr, int n_parts = 0,
                                 double* mean_linv = nullptr) {
  if (pl.lds) return launch_lds_prologue(pl.dtype == SQFA_F64, S, n, pl.m, pl.MR, LT, Linv, row_start, p, pl.TI, stream);
  launch_cholesky(pl.dtype, pl.m, stream, S, n, pl.MR, LT, Linv, row_start, p, pl.TI, mean_parts, n_parts, mean_linv);
  return hipGetLastError();
}

// Runs `launch` (K1) between two events on the stream when profiling is on (sqfa_airm_profile).  Event records do not
// belong in a captured graph: eager launches only.
template <typename F>
static hipError_t launch_profiled(hipStream_t stream, F launch) {
  bool prof = g_profile.load();
  if (prof) {
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(stream, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone) prof = false;
  }
  EventPair ev{};
  if (prof) {
    (void)hipEventCreate(&ev.a);
    (void)hipEventCreate(&ev.b);
    (void)hipEventRecord(ev.a, stream);
  }
  const hipError_t e = launch();
  if (prof) {
    (void)hipEventRecord(ev.b, stream);
    std::lock_guard<std::mutex> lock(g_events_mutex);
    g_events.push_back(ev);
  }
  return e;
}

// K2: finalize_kernel, finalize_bpc workgroups per class and one for the loss, the flags and the diagonals.
static hipError_t launch_finalize(const PairPlan& pl, const PairParams& p, void* gradA, void* gradB, void* loss, int* nonfinite,
                                  hipStream_t stream) {
  const int n_cls = p.nA + (p.self_mode ? 0 : p.nB);
  const dim3 grid(n_cls * finalize_bpc(pl.MR * (pl.MR + 1) / 2) + 1);
  auto launch = [&](auto zero) {
    using T = decltype(zero);
    hipLaunchKernelGGL(finalize_kernel<T>, grid, dim3(SQFA_K2_THREADS), 0, stream, p, pl.TI, pl.tj, pl.MR, static_cast<T*>(gradA),
                       static_cast<T*>(gradB), static_cast<T*>(loss), nonfinite);
  };
  if (pl.dtype == SQFA_F32) launch(0.0f);
  else launch(0.0);
  return hipGetLastError();
}

}  // namespace sqfa

using namespace sqfa;

extern "C" {

int sqfa_hip_version(void) { return 1000; }
const char* sqfa_hip_arch(void) { return "gfx950"; }
int sqfa_hip_max_dim(void) { return kLdsMaxDim; }
const char* sqfa_hip_last_error(void) { return g_last_error; }

int sqfa_airm_profile(int enable) {
  g_profile.store(enable != 0);
  return SQFA_OK;
}

int sqfa_airm_profile_read(double* tile_kernel_ms_total, int* launches) {
  double total = 0.0;
  int n = 0;
  std::lock_guard<std::mutex> lock(g_events_mutex);
  for (auto& ev : g_events) {
    float ms = 0.f;
    if (hipEventSynchronize(ev.b) == hipSuccess && hipEventElapsedTime(&ms, ev.a, ev.b) == hipSuccess) {
      total += ms;
      ++n;
    }
    (void)hipEventDestroy(ev.a);
    (void)hipEventDestroy(ev.b);
  }
  g_events.clear();
  if (tile_kernel_ms_total) *tile_kernel_ms_total = total;
  if (launches) *launches = n;
  return SQFA_OK;
}

int sqfa_project_profile_read(double* kernel_ms_total, int* launches) {
  double total = 0.0;
  int n = 0;
  std::lock_guard<std::mutex> lock(sqfa_project_events_mutex());
  for (auto& ev : sqfa_project_events()) {
    float ms = 0.f;
    if (hipEventSynchronize(ev.second) == hipSuccess && hipEventElapsedTime(&ms, ev.first, ev.second) == hipSuccess) {
      total += ms;
      ++n;
    }
    (void)hipEventDestroy(ev.first);
    (void)hipEventDestroy(ev.second);
  }
  sqfa_project_events().clear();
  if (kernel_ms_total) *kernel_ms_total = total;
  if (launches) *launches = n;
  return SQFA_OK;
}

int sqfa_airm_tiling(int nA, int nB, int m, int dtype, int* tile_i, int* tile_j, int* n_tiles_i,
                     int* n_tiles_j, int* padded_m) {
  if (nA < 1 || nB < 0 || m < 1 || !known_dtype(dtype)) return SQFA_ERR_BAD_ARGUMENT;
  PairPlan pl;
  if (!make_plan(nA, nB, m, dtype, 1, 0, &pl)) return SQFA_ERR_UNSUPPORTED_M;  // the widest tiles of an unsharded call
  if (tile_i) *tile_i = pl.TI;
  if (tile_j) *tile_j = pl.TJ;
  if (n_tiles_i) *n_tiles_i = pl.nbi;
  if (n_tiles_j) *n_tiles_j = (pl.nBeff + pl.TJ - 1) / pl.TJ;
  if (padded_m) *padded_m = pl.MR;
  return SQFA_OK;
}

size_t sqfa_airm_workspace_bytes(int nA, int nB, int m, int dtype) {
  if (nA < 1 || nB < 0 || m < 1 || !known_dtype(dtype)) return 0;
  // enough for any shard count, tile width and geometry policy: the regular row's and the small-launch row's layouts both fit
  PairPlan regular, small;
  if (!make_plan(nA, nB, m, dtype, 1, -1, &regular, true) || !make_plan(nA, nB, m, dtype, 1, 1, &small, true)) return 0;
  return std::max(regular.w.total, small.w.total);
}

// One call = dependent launches on the caller's stream:
//   prologue  the class factors and the slab slot table.  Register rows up to m = 24 whose class factor pass runs in the plain
//             metric: class_prologue_kernel, ONE launch for the A side (K0 + K0b fused; pair_kernel.hpp).  Otherwise K0 cholesky_kernel
//             (LDS path: cholesky_lds_kernel) and, where the pass runs, K0b class_factor_kernel / class_factor_mean_kernel (with
//             mean_partial_kernel in front).  Cross mode: one more cholesky_kernel launch for the B side (L^-1 only).
//   K1        pair_tile_kernel (pair_lds_kernel): every tile writes its partial gradients, loss and flags to the slab
//   K2        finalize_kernel: fixed-order reduction of the slab, loss, flags, diagonals
// sqfa_airm_options::launch_policy = -1 keeps K0 and K0b apart on every call; the results are bit-identical either way.
static int pairwise_impl(const void* A, int nA, const void* B, int nB, int m, int dtype, double scale,
                         double eps, int sqrt_mode, const void* pair_weights, double uniform_weight,
                         int shard_index, int shard_count, void* loss_out, void* gradA_out,
                         void* gradB_out, void* dist_out, void* eig_out, int* nonfinite_out,
                         void* workspace, size_t workspace_bytes, void* stream_, const void* eig_weights,
                         const sqfa_airm_options* options) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const int rc = validate_pair_call(A, nA, B, nB, m, dtype, shard_index, shard_count, workspace);
  if (rc != SQFA_OK) return rc;
  PairPlan pl;
  if (!make_plan(nA, nB, m, dtype, shard_count, options ? clamp_policy(options->geometry_policy) : 0, &pl))
    return fail(SQFA_ERR_UNSUPPORTED_M, "matrix size not supported", hipSuccess);
  if (workspace_bytes < pl.w.total) return fail(SQFA_ERR_WORKSPACE, "workspace too small", hipSuccess);
  char* ws = static_cast<char*>(workspace);
  PairParams p = make_pair_params(pl, ws, shard_index, scale, eps, sqrt_mode, pair_weights, uniform_weight, gradA_out != nullptr,
                                  dist_out, options);
  p.EW = eig_weights;
  p.eig_out = eig_out;

  // K0: factors.  Mean-metric factor pass (class_factor_mean_kernel): will K0b run, and on a size that has it?  Same rule as
  // launch_class_factors (the decision depends on (nA, nB, shard count, options) only: every shard of a job decides alike;
  // above 64 there is no geometry row and no factor pass: pl.g is all zero).
  const int mean_mode = options ? clamp_policy(options->mean_metric_policy) : 0;
  const bool want_mean = pl.g.mean_metric && mean_mode > 0 && p.factor_mode >= 0 &&
                         (p.factor_mode > 0 || pair_count(nA, nB, shard_count) >= pl.g.factor_min_pairs) && nA >= 2;
  double* mean_parts = reinterpret_cast<double*>(ws + pl.w.off_mean);
  double* mean_linv = mean_parts + (size_t)kMeanParts * pl.MR * pl.MR;
  const int n_parts = nA < kMeanParts ? nA : kMeanParts;
  if (want_mean) {
    if (dtype == SQFA_F32) hipLaunchKernelGGL(mean_partial_kernel<float>, dim3(n_parts), dim3(256), 0, stream, static_cast<const float*>(A), nA, m, mean_parts);
    else hipLaunchKernelGGL(mean_partial_kernel<double>, dim3(n_parts), dim3(256), 0, stream, static_cast<const double*>(A), nA, m, mean_parts);
    p.mean_linv = mean_linv;
  }
  // Will K0b run in the plain metric on a register row that has the fused prologue (m <= 24)?  Then the A side takes it (class_prologue_kernel:
  // factor, inverse, slot table and the factor pass's sweeps in one launch, bit-identical to the two it replaces) unless
  // launch_policy asks for the separate launches.  The rule is launch_class_factors' own.
  const int launch_policy = options ? options->launch_policy : 0;
  const bool fused_prologue = (launch_policy == 0 || (launch_policy > 0 && (launch_policy & SQFA_LAUNCH_FUSED_PROLOGUE))) && !pl.lds &&
                              pl.g.prologue != nullptr && !want_mean && p.factor_mode >= 0 &&
                              (p.factor_mode > 0 || pair_count(nA, nB, shard_count) >= pl.g.factor_min_pairs);
  hipError_t e;
  if (fused_prologue) {
    e = pl.g.prologue(p, A, pl.self_mode ? ws + pl.w.off_linv : nullptr, stream);
    if (e != hipSuccess) return fail(SQFA_ERR_LAUNCH, "class_prologue_kernel", e);
  } else {
    // the A-side launch also writes the slab slot table and carries the mean block
    e = launch_factors(pl, p, stream, A, nA, ws + pl.w.off_lt, pl.self_mode ? ws + pl.w.off_linv : nullptr, p.row_start,
                       want_mean ? mean_parts : nullptr, n_parts, mean_linv);
    if (e != hipSuccess) return fail(SQFA_ERR_LAUNCH, pl.lds ? "cholesky_lds_kernel" : "cholesky_kernel", e);
  }
  if (!pl.self_mode) {  // the B side stores L^-1 only and has no sweeps: cholesky_kernel on every path
    e = launch_factors(pl, p, stream, B, nB, nullptr, ws + pl.w.off_linv, nullptr);
    if (e != hipSuccess) return fail(SQFA_ERR_LAUNCH, pl.lds ? "cholesky_lds_kernel" : "cholesky_kernel", e);
  }
  if (!fused_prologue && pl.g.factor != nullptr) {  // K0b: orthogonalise the columns of each A-side factor (same stream: after the Cholesky launches)
    e = pl.g.factor(p, stream);
    if (e != hipSuccess) return fail(SQFA_ERR_LAUNCH, "class_factor_kernel", e);
  }

  // K1: pair tiles
  e = launch_profiled(stream, [&] { return pl.lds ? launch_pair_lds(dtype == SQFA_F64, p, pl.TI, pl.MR, stream) : pl.g.launch(p, stream); });
  if (e != hipSuccess) return fail(SQFA_ERR_LAUNCH, pl.lds ? "pair_lds_kernel" : "pair_tile_kernel", e);

  // K2: slab reduction
  e = launch_finalize(pl, p, gradA_out, gradB_out, loss_out, nonfinite_out, stream);
  if (e != hipSuccess) return fail(SQFA_ERR_LAUNCH, "finalize_kernel", e);
  return SQFA_OK;
}

// ---- sqfa_bw_pairwise ------------------------------------------------------------------------------------------------
// Workspace: the affine-invariant layout of the same problem (factors, slab, slot table), then
//   traces (nA + nB doubles) | slab_h (one value per B-side slab row: at most nbi (nB + TJ)) | hsum (nB doubles) |
//   R_j^-1, G_j, W_j (3 nB m^2 doubles)
struct BwExtra {
  size_t off_tr, off_h, off_hsum, off_sinv, off_g, off_w, total;
};
// widest tiling of a problem under any geometry policy: (most tile rows, widest tile); slab_h needs nbi (nB + TJ) entries
// for any narrower width
static void bw_tiles(int nA, int nB, int m, int dtype, int* nbi, int* TJ) {
  PairPlan regular, small;
  make_plan(nA, nB, m, dtype, 1, -1, &regular);
  make_plan(nA, nB, m, dtype, 1, 1, &small);
  *nbi = std::max(regular.nbi, small.nbi);
  *TJ = std::max(regular.TJ, small.TJ);
}
// (the caller has made a plan of the same problem: its size is supported)
static BwExtra bw_extra(size_t base, int nA, int nB, int m, int dtype) {
  const int nBeff = nB == 0 ? nA : nB;
  int nbi, TJ;
  bw_tiles(nA, nB, m, dtype, &nbi, &TJ);
  BwExtra x;
  size_t o = base;
  x.off_tr = o;   o = align256(o + (size_t)(nA + nBeff) * sizeof(double));
  x.off_h = o;    o = align256(o + (size_t)nbi * (nBeff + TJ) * sizeof(double));
  x.off_hsum = o; o = align256(o + (size_t)nBeff * sizeof(double));
  x.off_sinv = o; o = align256(o + (size_t)nBeff * m * m * sizeof(double));
  x.off_g = o;    o = align256(o + (size_t)nBeff * m * m * sizeof(double));
  x.off_w = o;    o = align256(o + (size_t)nBeff * m * m * sizeof(double));
  x.total = o;
  return x;
}

static int bw_impl(const void* A, int nA, const void* B, int nB, int m, int dtype, double eps, int sqrt_mode,
                   const void* pair_weights, double uniform_weight, int shard_index, int shard_count, void* loss_out,
                   void* gradA_out, void* gradB_out, void* dist_out, int* nonfinite_out, void* workspace,
                   size_t workspace_bytes, void* stream_, const sqfa_airm_options* options) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const int rc = validate_pair_call(A, nA, B, nB, m, dtype, shard_index, shard_count, workspace);
  if (rc != SQFA_OK) return rc;
  PairPlan pl;
  if (!make_plan(nA, nB, m, dtype, shard_count, options ? clamp_policy(options->geometry_policy) : 0, &pl))
    return fail(SQFA_ERR_UNSUPPORTED_M, "matrix size not supported", hipSuccess);
  const BwExtra x = bw_extra(pl.w.total, nA, nB, m, dtype);
  if (workspace_bytes < x.total) return fail(SQFA_ERR_WORKSPACE, "workspace too small", hipSuccess);
  char* ws = static_cast<char*>(workspace);
  double* tr = reinterpret_cast<double*>(ws + x.off_tr);
  double* sinv = reinterpret_cast<double*>(ws + x.off_sinv);
  PairParams p = make_pair_params(pl, ws, shard_index, 1.0, eps, sqrt_mode, pair_weights, uniform_weight, gradA_out != nullptr,
                                  dist_out, options);
  p.trA = tr;
  p.trB = pl.self_mode ? tr : tr + nA;
  p.slab_h = ws + x.off_h;

  // K0: A-side factors (the affine-invariant prologue; the launch also writes the slab slot table) ...
  hipError_t e = launch_factors(pl, p, stream, A, nA, ws + pl.w.off_lt, nullptr, p.row_start);
  if (e != hipSuccess) return fail(SQFA_ERR_LAUNCH, "cholesky_kernel", e);
  // ... and the BW prologue: R_j, R_j^-1 and traces of the B classes, traces of the A classes
  auto by_dtype = [&](auto launch) {  // launch(T()) with the element type of the call
    if (dtype == SQFA_F32) launch(0.0f);
    else launch(0.0);
    return hipGetLastError();
  };
  e = by_dtype([&](auto zero) {
    using T = decltype(zero);
    const size_t lds_bytes = ((size_t)m * (m + 1) + m) * sizeof(double);
    if (lds_bytes > 64 * 1024)
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(bw_prologue_kernel<T>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    auto launch = [&](const void* S, int n, void* R, double* si, double* trace) {
      hipLaunchKernelGGL(bw_prologue_kernel<T>, dim3(n), dim3(256), lds_bytes, stream, static_cast<const T*>(S), m, pl.MR,
                         static_cast<T*>(R), si, trace);
    };
    void* rslot = ws + pl.w.off_linv;
    if (pl.self_mode) launch(A, nA, rslot, sinv, tr);
    else { launch(A, nA, nullptr, nullptr, tr); launch(B, nB, rslot, sinv, tr + nA); }
  });
  if (e != hipSuccess) return fail(SQFA_ERR_LAUNCH, "bw_prologue_kernel", e);
  if (pl.g.factor != nullptr) {  // K0b on the A-side factors (plain metric: mean_metric_policy does not apply here)
    e = pl.g.factor(p, stream);
    if (e != hipSuccess) return fail(SQFA_ERR_LAUNCH, "class_factor_kernel", e);
  }

  // K1: pair tiles
  e = launch_profiled(stream, [&] { return pl.lds ? launch_pair_lds_bw(dtype == SQFA_F64, p, pl.TI, pl.MR, stream) : pl.g.launch_bw(p, stream); });
  if (e != hipSuccess) return fail(SQFA_ERR_LAUNCH, "pair_tile_kernel (Bures-Wasserstein)", e);

  // K2: loss, flags and the diagonal of dist_out through finalize_kernel (its class blocks return at once without
  // want_grad), then the gradient reduction and the B-side sandwich
  PairParams q = p;
  q.want_grad = 0;
  e = launch_finalize(pl, q, nullptr, nullptr, loss_out, nonfinite_out, stream);
  if (e != hipSuccess) return fail(SQFA_ERR_LAUNCH, "finalize_kernel", e);
  if (p.want_grad) {
    double* G = reinterpret_cast<double*>(ws + x.off_g);
    double* W = reinterpret_cast<double*>(ws + x.off_w);
    double* hs = reinterpret_cast<double*>(ws + x.off_hsum);
    void* outB = pl.self_mode ? gradA_out : gradB_out;
    e = by_dtype([&](auto zero) {
      using T = decltype(zero);
      hipLaunchKernelGGL(finalize_bw_kernel<T>, dim3((nA + pl.nBeff) * finalize_bw_bpc(pl.MR * (pl.MR + 1) / 2)), dim3(256), 0, stream,
                         p, pl.TI, pl.tj, pl.MR, static_cast<T*>(gradA_out), G, hs);
      if (outB != nullptr)
        hipLaunchKernelGGL(bw_sandwich_kernel<T>, dim3(pl.nBeff), dim3(256), 0, stream, m, sinv, G, W, hs, static_cast<T*>(outB),
                           pl.self_mode);
    });
    if (e != hipSuccess) return fail(SQFA_ERR_LAUNCH, "finalize_bw_kernel", e);
  }
  return SQFA_OK;
}

size_t sqfa_airm_workspace_bytes_sharded(int nA, int nB, int m, int dtype, int shard_count, int geometry_policy) {
  PairPlan pl;
  if (shard_count < 1 || nA < 1 || nB < 0 || m < 1 || !known_dtype(dtype) ||
      !make_plan(nA, nB, m, dtype, shard_count, clamp_policy(geometry_policy), &pl))
    return 0;
  return pl.w.total;
}

int sqfa_airm_pairwise(const void* A, int nA, const void* B, int nB, int m, int dtype, double scale,
                       double eps, int sqrt_mode, const void* pair_weights, double uniform_weight,
                       int shard_index, int shard_count, void* loss_out, void* gradA_out,
                       void* gradB_out, void* dist_out, void* eig_out, int* nonfinite_out,
                       void* workspace, size_t workspace_bytes, void* stream_) {
  return pairwise_impl(A, nA, B, nB, m, dtype, scale, eps, sqrt_mode, pair_weights, uniform_weight, shard_index,
                       shard_count, loss_out, gradA_out, gradB_out, dist_out, eig_out, nonfinite_out, workspace,
                       workspace_bytes, stream_, nullptr, nullptr);
}

int sqfa_airm_pairwise_opt(const void* A, int nA, const void* B, int nB, int m, int dtype, double scale,
                           double eps, int sqrt_mode, const void* pair_weights, double uniform_weight,
                           int shard_index, int shard_count, void* loss_out, void* gradA_out,
                           void* gradB_out, void* dist_out, void* eig_out, int* nonfinite_out,
                           void* workspace, size_t workspace_bytes, void* stream_, const sqfa_airm_options* options) {
  return pairwise_impl(A, nA, B, nB, m, dtype, scale, eps, sqrt_mode, pair_weights, uniform_weight, shard_index,
                       shard_count, loss_out, gradA_out, gradB_out, dist_out, eig_out, nonfinite_out, workspace,
                       workspace_bytes, stream_, nullptr, options);
}

int sqfa_airm_eigenvalues_backward(const void* A, int nA, const void* B, int nB, int m, int dtype,
                                   const void* eig_weights, void* gradA_out, void* gradB_out,
                                   void* workspace, size_t workspace_bytes, void* stream_,
                                   const sqfa_airm_options* options) {
  if (eig_weights == nullptr || gradA_out == nullptr) {
    g_last_error[0] = 0;
    return fail(SQFA_ERR_BAD_ARGUMENT, "eig_weights / gradA_out", hipSuccess);
  }
  return pairwise_impl(A, nA, B, nB, m, dtype, 1.0, 0.0, 0, nullptr, 0.0, 0, 1, nullptr, gradA_out, gradB_out,
                       nullptr, nullptr, nullptr, workspace, workspace_bytes, stream_, eig_weights, options);
}

size_t sqfa_bw_workspace_bytes(int nA, int nB, int m, int dtype) {
  const size_t base = sqfa_airm_workspace_bytes(nA, nB, m, dtype);
  return base == 0 ? 0 : bw_extra(align256(base), nA, nB, m, dtype).total;
}

size_t sqfa_bw_workspace_bytes_sharded(int nA, int nB, int m, int dtype, int shard_count, int geometry_policy) {
  const size_t base = sqfa_airm_workspace_bytes_sharded(nA, nB, m, dtype, shard_count, geometry_policy);
  return base == 0 ? 0 : bw_extra(align256(base), nA, nB, m, dtype).total;
}

int sqfa_bw_pairwise(const void* A, int nA, const void* B, int nB, int m, int dtype, double eps, int sqrt_mode,
                     const void* pair_weights, double uniform_weight, int shard_index, int shard_count, void* loss_out,
                     void* gradA_out, void* gradB_out, void* dist_out, int* nonfinite_out, void* workspace,
                     size_t workspace_bytes, void* stream_, const sqfa_airm_options* options) {
  return bw_impl(A, nA, B, nB, m, dtype, eps, sqrt_mode, pair_weights, uniform_weight, shard_index, shard_count, loss_out,
                 gradA_out, gradB_out, dist_out, nonfinite_out, workspace, workspace_bytes, stream_, options);
}

size_t sqfa_spd_function_workspace_bytes(int n, int m, int dtype) {
  Geometry g;
  if (n < 1 || m < 1 || !known_dtype(dtype) || !find_geometry(m, dtype, -1, &g, -1)) return 0;
  return align256((size_t)n * g.MR * g.MR * (dtype == SQFA_F32 ? 4 : 8));
}

int sqfa_spd_function(const void* S, int n, int m, int dtype, int kind, void* F_out, double* U_out, double* lam_out,
                      void* workspace, size_t workspace_bytes, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  g_last_error[0] = 0;
  if (S == nullptr || n < 1 || m < 1 || U_out == nullptr || lam_out == nullptr || workspace == nullptr)
    return fail(SQFA_ERR_BAD_ARGUMENT, "null/size argument", hipSuccess);
  if (dtype != SQFA_F32 && dtype != SQFA_F64) return fail(SQFA_ERR_BAD_ARGUMENT, "dtype", hipSuccess);
  if (kind != SQFA_SPD_LOG && kind != SQFA_SPD_SQRT && kind != SQFA_SPD_INV_SQRT) return fail(SQFA_ERR_BAD_ARGUMENT, "kind", hipSuccess);
  Geometry g;
  if (!find_geometry(m, dtype, -1, &g, -1) || g.eig == nullptr) return fail(SQFA_ERR_UNSUPPORTED_M, "matrix size not supported", hipSuccess);
  if (workspace_bytes < sqfa_spd_function_workspace_bytes(n, m, dtype)) return fail(SQFA_ERR_WORKSPACE, "workspace too small", hipSuccess);
  PairParams p;
  memset(&p, 0, sizeof(p));
  // Cholesky factor of every class, columns contiguous, identity padded to the size class (K0; double inside)
  launch_cholesky(dtype, m, stream, S, n, g.MR, workspace, nullptr, nullptr, p, g.TI);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(SQFA_ERR_LAUNCH, "cholesky_kernel", e);
  e = g.eig(workspace, n, m, U_out, lam_out, stream);
  if (e != hipSuccess) return fail(SQFA_ERR_LAUNCH, "class_eig_kernel", e);
  if (F_out != nullptr) {
    const size_t lds = ((size_t)m * m + m) * sizeof(double);
    if (dtype == SQFA_F32) hipLaunchKernelGGL(spd_function_kernel<float>, dim3(n), dim3(256), lds, stream, U_out, lam_out, m, kind, static_cast<float*>(F_out));
    else hipLaunchKernelGGL(spd_function_kernel<double>, dim3(n), dim3(256), lds, stream, U_out, lam_out, m, kind, static_cast<double*>(F_out));
    e = hipGetLastError();
    if (e != hipSuccess) return fail(SQFA_ERR_LAUNCH, "spd_function_kernel", e);
  }
  return SQFA_OK;
}

int sqfa_spd_function_backward(const double* U, const double* lam, const void* G, int n, int m, int dtype, int kind,
                               void* gradS_out, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  g_last_error[0] = 0;
  if (U == nullptr || lam == nullptr || G == nullptr || gradS_out == nullptr || n < 1 || m < 1)
    return fail(SQFA_ERR_BAD_ARGUMENT, "null/size argument", hipSuccess);
  if (dtype != SQFA_F32 && dtype != SQFA_F64) return fail(SQFA_ERR_BAD_ARGUMENT, "dtype", hipSuccess);
  if (kind != SQFA_SPD_LOG && kind != SQFA_SPD_SQRT && kind != SQFA_SPD_INV_SQRT) return fail(SQFA_ERR_BAD_ARGUMENT, "kind", hipSuccess);
  if (m > kSpdMaxDim) return fail(SQFA_ERR_UNSUPPORTED_M, "matrix size not supported", hipSuccess);
  const size_t lds = ((size_t)3 * m * m + m) * sizeof(double);   // 96.5 KB at m = 64
  if (dtype == SQFA_F32) {
    if (lds > 48 * 1024) (void)hipFuncSetAttribute(reinterpret_cast<const void*>(spd_function_backward_kernel<float>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(spd_function_backward_kernel<float>, dim3(n), dim3(256), lds, stream, U, lam, static_cast<const float*>(G), m, kind, static_cast<float*>(gradS_out));
  } else {
    if (lds > 48 * 1024) (void)hipFuncSetAttribute(reinterpret_cast<const void*>(spd_function_backward_kernel<double>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(spd_function_backward_kernel<double>, dim3(n), dim3(256), lds, stream, U, lam, static_cast<const double*>(G), m, kind, static_cast<double*>(gradS_out));
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(SQFA_ERR_LAUNCH, "spd_function_backward_kernel", e);
  return SQFA_OK;
}

}  // extern "C"
