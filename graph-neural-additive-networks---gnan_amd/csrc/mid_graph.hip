// One-launch forward and one-launch backward of a dense-coded graph of up to 448 nodes (csrc/small_graph.hip stops at 128: its
// last workgroup stages the whole [n][n] hop-code block in LDS — 174 KB at the 417 nodes of the largest Mutagenicity graph — and
// its backward keeps [D][n | 1] bins per wave).  The same model, the same arithmetic and the same orders as there; the graph is
// walked in TILES OF 64 ROWS, so that a [64][n] block of hop codes and a [64][64] block of row weights is all of the graph a
// workgroup holds at a time.  Post-rho shell normalisation (or none), a one-channel rho, D <= 64 shells, C <= 8.  Pre-rho
// normalisation (GNAN.py:65-67, `reserved` == GNAN_MID_PRE_RHO): kernels of their own, in the second half of this file.
//
// Forward
//   workgroup k < F : f_k on all nodes, in node blocks of 64 (small_graph_body.hpp's mlp_block), into part[k, node, :].
//   workgroup F     : lut[d] = rho(u_d).
//   the LAST workgroup to arrive adds the features in order (S, written out), then takes the row tiles in order: hop codes and
//   shell sizes of tile t + 1 are requested (into registers) before tile t is consumed from LDS; one thread per (row, channel)
//   walks the neighbours in ascending order; the read-out sum in row order; the counter goes back to zero.
// Backward
//   workgroup k < F : dS[j, c] = sum_i lut[code(i, j)] / max(cnt(i, code), 1) * dY[i, c] over the row tiles in ascending order
//                     (every feature workgroup forms it itself: nobody waits for anybody), then fmlp_bwd_body.hpp's feature_grads.
//   workgroup F + g : the table gradient of rows 32 g .. 32 g + 31 — a row per wave at a time, the neighbours' dot products
//                     binned by hop code in lane-private LDS columns ([D][65]), float64 across rows — left as float64 partials
//                     dlut[g][64] in the workspace; the last rho group to arrive adds the partials in group order and runs
//                     feature_grads on rho's D arguments.
// No workgroup waits for another: the only joins are "the last to arrive continues, everyone else returns".
#include <cstdint>

#include "mid_graph_tiles.hpp"

namespace {

using namespace gnan_mid;      // (and gnan_small): the tile constants and the tiles' way into LDS, shared with csrc/mid_graph_nam.hip

// ---- LDS plans (floats unless said otherwise): one size per kernel, the largest admitted shape --------------------------------
// forward, last workgroup: S [n, C] | Y [n, C] | lut [64] | row weights [64][64] | hop codes [64][row bytes]; the MLP phases use
// the first 2 * 64 * 64 floats as activation columns
constexpr int kFwdS = 0, kFwdY = kMidNodes * kMaxC, kFwdLut = 2 * kMidNodes * kMaxC, kFwdW = kFwdLut + kWave,
              kFwdCode = kFwdW + kTile * kWave;
constexpr int kCodeRowMax = 4 * ((kMidNodes / 4) | 1);                               // padded row of the forward's tile (below)
constexpr size_t kFwdDynBytes = static_cast<size_t>(kFwdCode) * 4 + static_cast<size_t>(kTile) * kCodeRowMax;
constexpr size_t kFwdStaticBytes = kWeightFloats * 4 + 16;                           // weight image + the arrival slot
static_assert(kFwdCode >= 2 * kMaxH * kWave, "the activation columns fit in front of the code tile");
// backward, feature workgroup: dY [n, C] | dS [n, C] | row weights [64][64] | hop codes [64][n] bytes
constexpr int kBwdDY = 0, kBwdG = kMidNodes * kMaxC, kBwdU = 2 * kMidNodes * kMaxC, kBwdCode = kBwdU + kTile * kWave;
constexpr size_t kBwdDynBytes = static_cast<size_t>(kBwdCode) * 4 + static_cast<size_t>(kTile) * kMidNodes;
// backward, rho group: S [n, C] | dY of the group's rows [32, C] | hop codes [32][n] bytes | bins [waves][D][65]
constexpr int kRhoS = 0, kRhoDY = kMidNodes * kMaxC, kRhoCode = kRhoDY + kRhoRows * kMaxC,
              kRhoBins = kRhoCode + kRhoRows * kMidNodes / 4;
constexpr int kRhoBinFloats = static_cast<int>(kBwdDynBytes / 4) - kRhoBins;
static_assert(kRhoBinFloats >= 2 * kMidD * kBinCols, "two waves' bins fit at 64 shells");
constexpr size_t kBwdStaticBytes = sizeof(gnan_bwd::RedBuffer) + kWaves * kWave * sizeof(double) + 2 * kWave * 4 + 16;

struct MidParams {
  const float* x;
  int64_t x_stride;
  int n, F;
  Mlp f, r;
  const uint8_t* code;
  int D;
  const int32_t* cnt;
  int64_t cnt_stride;
  float* S;
  float* lut;
  float* Y;
  float* Ysum;
  float* part;          // [F, n, C]
  unsigned* counter;    // zero before the first launch; the last workgroup zeroes it again
};

// ... and under training-mode Dropout of the shape functions (gnan_mid_graph_fwd_drop with p > 0)
struct MidDropParams : MidParams {
  gnan_bwd::Drop drop;
  const uint64_t* seed_dev;     // NULL (drop.seed came by value), or the device cell the seed is read from (gnan_mid_graph_fwd_drop_dev)
};

// P = MidParams: the Dropout-free instance, the code it was.  P = MidDropParams: a kernel of its own whose shape-function
// workgroups mask their hidden activations (mlp_block<true>; node = the row of x, feature = k).
template <class P>
__global__ __launch_bounds__(kThreads) void mid_graph_kernel(const P p) {
  constexpr bool DROP = std::is_same<P, MidDropParams>::value;
  extern __shared__ __attribute__((aligned(16))) float dyn[];
  __shared__ __attribute__((aligned(16))) float weights[kWeightFloats];
  __shared__ unsigned s_last;
  float* col_a = dyn;
  float* col_b = dyn + kMaxH * kWave;
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int k = blockIdx.x, n = p.n, C = p.f.C;
  const int blocks = (n + kTile - 1) / kTile;
  float out[kMaxC];
  const MlpLds wl = carve(weights);
  uint64_t seed = 0ull;                                // (Dropout only) by value, or from its device cell: one wave-uniform load
  if constexpr (DROP) seed = p.seed_dev ? *p.seed_dev : p.drop.seed;
  // the first tile's codes and shell sizes are requested now, by every workgroup (any may be the last): they fly during the MLPs
  TileRegs<kTile> regs;
  tile_fetch<kTile>(regs, p.code, p.cnt, p.cnt_stride, n, p.D, 0);
  if (k < p.F) {
    stage_weights(p.f, k, wl);
    float xv[kMidBlocks];
#pragma unroll
    for (int b = 0; b < kMidBlocks; ++b) {            // (all node blocks' inputs requested before the first MLP)
      const int j = b * kWave + lane;
      xv[b] = j < n ? p.x[static_cast<int64_t>(j) * p.x_stride + k] : 0.f;
    }
#pragma unroll
    for (int b = 0; b < kMidBlocks; ++b) {
      const int j = b * kWave + lane;
      if (b < blocks) {                               // (uniform)
        if constexpr (DROP) mlp_block<true>(p.f, wl, xv[b], col_a, col_b, lane, wave, out, p.drop, gnan::drop_base(seed, j, k));
        else mlp_block(p.f, wl, xv[b], col_a, col_b, lane, wave, out);
        if (wave == 0 && j < n)
          for (int c = 0; c < C; ++c) p.part[(static_cast<int64_t>(k) * n + j) * C + c] = out[c];
      }
    }
  } else {
    stage_weights(p.r, 0, wl);
    const float u = lane < p.D - 1 ? 1.0f / (static_cast<float>(lane) + 1.0f) : 0.f;     // graph.hop_inputs
    mlp_block(p.r, wl, u, col_a, col_b, lane, wave, out);
    if (wave == 0 && lane < p.D) p.lut[lane] = out[0];
  }
  // ---- join: the last workgroup to arrive finishes the graph -----------------------------------------------------------------
  if (!last_to_arrive(p.counter, gridDim.x, &s_last)) return;
  float* s_S = dyn + kFwdS;
  float* s_Y = dyn + kFwdY;
  float* s_lut = dyn + kFwdLut;
  float* s_w = dyn + kFwdW;
  uint8_t* s_code = reinterpret_cast<uint8_t*>(dyn + kFwdCode);
  const int nc = n * C;
  if (threadIdx.x < kWave) s_lut[threadIdx.x] = static_cast<int>(threadIdx.x) < p.D ? p.lut[threadIdx.x] : 0.f;
  // node sums: a thread per (node, channel) adds the features in order, eight terms in flight at a time
  for (int e = threadIdx.x; e < nc; e += kThreads) {
    float sum = 0.f;
    for (int k0 = 0; k0 < p.F; k0 += 8) {
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = k0 + u < p.F ? p.part[static_cast<int64_t>(k0 + u) * nc + e] : 0.f;
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (k0 + u < p.F) sum += v[u];
    }
    s_S[e] = sum;
    p.S[e] = sum;
  }
  const int row_bytes = (n & 3) == 0 ? 4 * ((n / 4) | 1) : n;
  for (int t = 0; t < blocks; ++t) {
    const int i0 = t * kTile;
    const int rows = n - i0 < kTile ? n - i0 : kTile;
    __syncthreads();                                  // (the tile before is consumed; first round: S and the table are in place)
    tile_store_codes<kTile, true>(regs, p.code, n, i0, s_code);
    tile_store_weights<kTile>(regs, s_lut, p.cnt != nullptr, p.D, s_w);
    if (t + 1 < blocks) tile_fetch<kTile>(regs, p.code, p.cnt, p.cnt_stride, n, p.D, i0 + kTile);
    __syncthreads();
    // one thread per (row, channel), neighbours in ascending order
    for (int e = threadIdx.x; e < rows * C; e += kThreads) {
      const int r = e / C, c = e % C;
      const uint8_t* codes = s_code + r * row_bytes;
      const float* wrow = s_w + r * kWave;
      float acc = 0.f;
#pragma unroll 8
      for (int j = 0; j < n; ++j) {                   // (unrolled: the code -> weight reads of eight neighbours overlap)
        int d = codes[j];
        d = d < p.D - 1 ? d : p.D - 1;
        acc = fmaf(wrow[d], s_S[j * C + c], acc);
      }
      s_Y[i0 * C + e] = acc;
      if (p.Y) p.Y[i0 * C + e] = acc;
    }
  }
  __syncthreads();
  if (p.Ysum && static_cast<int>(threadIdx.x) < C) {
    float s = 0.f;
#pragma unroll 8
    for (int i = 0; i < n; ++i) s += s_Y[i * C + threadIdx.x];
    p.Ysum[threadIdx.x] = s;
  }
  if (threadIdx.x == 0) *p.counter = 0u;
}

struct MidBwdParams {
  const float* x;
  int64_t x_stride;
  int n, F;
  gnan_bwd::Weights f, r;
  int f_mid, r_mid;          // L == 3
  const uint8_t* code;
  int D;
  const int32_t* cnt;
  int64_t cnt_stride;
  const float* S;
  const float* lut;
  const float* dY;
  const float* dYsum;
  int rho_groups;
  double* part;              // [rho_groups][64] partial table gradients
  unsigned* counter;         // arrivals of the rho groups
};

// fdrop: the forward's Dropout of the shape functions (thresh 0: none) — the feature workgroups recompute its masks; rho has none.
template <int C>
__device__ __forceinline__ void mid_graph_bwd_body(const MidBwdParams& p, float* dyn, gnan_bwd::Drop fdrop) {
  __shared__ gnan_bwd::RedBuffer red;
  __shared__ double s_part[kWaves][kWave];
  __shared__ float s_lut[kWave];
  __shared__ float s_dl[kWave];
  __shared__ unsigned s_last;
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int k = blockIdx.x, n = p.n, nc = p.n * C;
  const gnan_bwd::Drop nodrop{0u, 1.f, 0ull};
  if (k < p.F) {
    // ---- operand gradient of every node over the row tiles, then this feature's parameter gradients --------------------------
    float* s_dY = dyn + kBwdDY;
    float* s_g = dyn + kBwdG;
    float* s_u = dyn + kBwdU;
    uint8_t* s_code = reinterpret_cast<uint8_t*>(dyn + kBwdCode);
    const int blocks = (n + kTile - 1) / kTile;
    TileRegs<kTile> regs;
    tile_fetch<kTile>(regs, p.code, p.cnt, p.cnt_stride, n, p.D, 0);
    if (threadIdx.x < kWave) s_lut[threadIdx.x] = static_cast<int>(threadIdx.x) < p.D ? p.lut[threadIdx.x] : 0.f;
    for (int e = threadIdx.x; e < nc; e += kThreads) {
      s_dY[e] = p.dY ? p.dY[e] : p.dYsum[e % C];
      s_g[e] = 0.f;
    }
    for (int t = 0; t < blocks; ++t) {
      const int i0 = t * kTile;
      const int rows = n - i0 < kTile ? n - i0 : kTile;
      __syncthreads();
      tile_store_codes<kTile, false>(regs, p.code, n, i0, s_code);
      tile_store_weights<kTile>(regs, s_lut, p.cnt != nullptr, p.D, s_u);
      if (t + 1 < blocks) tile_fetch<kTile>(regs, p.code, p.cnt, p.cnt_stride, n, p.D, i0 + kTile);
      __syncthreads();
      for (int e = threadIdx.x; e < nc; e += kThreads) {          // thread (column j, channel): the tile's rows in ascending order
        const int j = e / C, c = e % C;
        float acc = s_g[e];
#pragma unroll 8
        for (int r = 0; r < rows; ++r) {
          int d = s_code[r * n + j];
          d = d < p.D - 1 ? d : p.D - 1;
          acc = fmaf(s_u[r * kWave + d], s_dY[(i0 + r) * C + c], acc);
        }
        s_g[e] = acc;
      }
    }
    __syncthreads();
    auto x_of = [&](int64_t node) { return p.x[node * p.x_stride + k]; };
    auto g_of = [&](int64_t node, int c) { return s_g[node * C + c]; };
    if (p.f_mid) gnan_bwd::feature_grads<C, true>(p.f, k, 0, n, 0, fdrop, x_of, g_of, red);
    else gnan_bwd::feature_grads<C, false>(p.f, k, 0, n, 0, fdrop, x_of, g_of, red);
    return;
  }
  // ---- table gradient of this group's rows -------------------------------------------------------------------------------------
  const int grp = k - p.F;
  const int i_lo = grp * kRhoRows;
  const int i_hi = i_lo + kRhoRows < n ? i_lo + kRhoRows : n;
  float* s_S = dyn + kRhoS;
  float* s_dY = dyn + kRhoDY;
  uint8_t* s_code = reinterpret_cast<uint8_t*>(dyn + kRhoCode);
  {
    TileRegs<kRhoRows> regs;
    tile_fetch<kRhoRows>(regs, p.code, nullptr, 0, n, p.D, i_lo);
    for (int e = threadIdx.x; e < nc; e += kThreads) s_S[e] = p.S[e];
    for (int e = threadIdx.x; e < (i_hi - i_lo) * C; e += kThreads) s_dY[e] = p.dY ? p.dY[i_lo * C + e] : p.dYsum[e % C];
    tile_store_codes<kRhoRows, false>(regs, p.code, n, i_lo, s_code);
  }
  const int nw = kWaves * p.D * kBinCols <= kRhoBinFloats ? kWaves : 2;      // waves that bin: as many as have room for [D][65]
  float* bins = dyn + kRhoBins + wave * p.D * kBinCols;
  double acc = 0.0;                                                        // lane d: dlut[d] over this wave's rows
  __syncthreads();
  for (int rr = 0; i_lo + nw * rr < i_hi; ++rr) {
    const int i = i_lo + nw * rr + wave;
    const bool live = wave < nw && i < i_hi;
    if (live) {
      for (int d = 0; d < p.D; ++d) bins[d * kBinCols + lane] = 0.f;
      float gy[C];
#pragma unroll
      for (int c = 0; c < C; ++c) gy[c] = s_dY[(i - i_lo) * C + c];
      const uint8_t* codes = s_code + (i - i_lo) * n;
      for (int j = lane; j < n; j += kWave) {          // (a lane owns its column of the bins: no other lane writes it)
        int d = codes[j];
        d = d < p.D - 1 ? d : p.D - 1;
        float v = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) v = fmaf(gy[c], s_S[j * C + c], v);
        bins[d * kBinCols + lane] += v;
      }
    }
    __syncthreads();
    if (live && lane < p.D) {
      float sum = 0.f;
#pragma unroll 8
      for (int l = 0; l < kWave; ++l) sum += bins[lane * kBinCols + l];
      if (p.cnt) {
        const int q = p.cnt[i * p.cnt_stride + lane];
        sum *= 1.f / static_cast<float>(q > 1 ? q : 1);
      }
      acc += static_cast<double>(sum);
    }
    __syncthreads();
  }
  s_part[wave][lane] = (wave < nw && lane < p.D) ? acc : 0.0;
  __syncthreads();
  if (wave == 0) p.part[grp * kWave + lane] = ((s_part[0][lane] + s_part[1][lane]) + s_part[2][lane]) + s_part[3][lane];
  // ---- join of the rho groups: the last to arrive adds the partials in group order, then rho's parameter gradients ------------
  if (!last_to_arrive(p.counter, static_cast<unsigned>(p.rho_groups), &s_last)) return;
  if (wave == 0) {
    double v[kRhoGroupsMid];
#pragma unroll
    for (int g = 0; g < kRhoGroupsMid; ++g) v[g] = g < p.rho_groups ? p.part[g * kWave + lane] : 0.0;
    double sum = 0.0;
#pragma unroll
    for (int g = 0; g < kRhoGroupsMid; ++g)
      if (g < p.rho_groups) sum += v[g];
    s_dl[lane] = static_cast<float>(sum);
  }
  if (threadIdx.x == 0) *p.counter = 0u;
  __syncthreads();
  auto u_of = [&](int64_t d) { return d < p.D - 1 ? 1.0f / (static_cast<float>(d) + 1.0f) : 0.f; };
  auto gl_of = [&](int64_t d, int) { return s_dl[d]; };
  if (p.r_mid) gnan_bwd::feature_grads<1, true>(p.r, 0, 0, p.D, 0, nodrop, u_of, gl_of, red);
  else gnan_bwd::feature_grads<1, false>(p.r, 0, 0, p.D, 0, nodrop, u_of, gl_of, red);
}

template <int C>
__global__ __launch_bounds__(kThreads) void mid_graph_bwd_kernel(const MidBwdParams p) {
  extern __shared__ __attribute__((aligned(16))) float dyn[];
  mid_graph_bwd_body<C>(p, dyn, gnan_bwd::Drop{0u, 1.f, 0ull});
}

// ... of a forward under Dropout (gnan_mid_graph_bwd_drop with p > 0)
template <int C>
__global__ __launch_bounds__(kThreads) void mid_graph_bwd_drop_kernel(const MidBwdParams p, gnan_bwd::Drop drop, const uint64_t* seed_dev) {
  extern __shared__ __attribute__((aligned(16))) float dyn[];
  if (seed_dev) drop.seed = *seed_dev;               // (gnan_mid_graph_bwd_drop_dev: the seed's device cell)
  mid_graph_bwd_body<C>(p, dyn, drop);
}

template <int C>
int launch_mid_bwd(const MidBwdParams& p, const gnan_bwd::Drop& drop, const uint64_t* seed_dev, hipStream_t st) {
  const dim3 grid(static_cast<unsigned>(p.F + p.rho_groups));
  if (drop.thresh != 0u) {                             // (the Dropout instances: kernels of their own, the others untouched)
    if (int rc = raise_dyn_lds<&mid_graph_bwd_drop_kernel<C>>(kBwdDynBytes, "mid_graph_bwd")) return rc;
    hipLaunchKernelGGL((mid_graph_bwd_drop_kernel<C>), grid, dim3(kThreads), kBwdDynBytes, st, p, drop, seed_dev);
    return gnan::check_launch("mid_graph_bwd_drop_kernel");
  }
  if (int rc = raise_dyn_lds<&mid_graph_bwd_kernel<C>>(kBwdDynBytes, "mid_graph_bwd")) return rc;
  hipLaunchKernelGGL((mid_graph_bwd_kernel<C>), grid, dim3(kThreads), kBwdDynBytes, st, p);
  return gnan::check_launch("mid_graph_bwd_kernel");
}

constexpr RouteLimits kMidCover = {kMidNodes, kMidD, kMaxC, false};      // what both entry points and the route query take

// =================================================================================================================================
// Pre-rho normalisation (GNAN.py:65-67; `reserved` == GNAN_MID_PRE_RHO): the weight of pair (i, j) is rho(u_d / max(cnt[i, d], 1)),
// rho AFTER the division — n * D arguments of rho instead of D, and `lut` is the rows' table [n, D].  Kernels of their own: the
// ones above stay the code they were.  The tiled twins of small_graph.hip's pre_rho paths (small_graph_body / small_graph_bwd_body),
// with their arithmetic and orders.
//
// Forward
//   workgroup k < F     : as above.
//   workgroup F + g     : rho at the arguments e = i * D + d of the passes g * T .. g * T + T - 1 (T = ceil(n / 64) row tiles; a pass
//                         is 64 consecutive arguments, argument e in lane e % 64), so a rho workgroup runs no more MLP passes than
//                         a feature workgroup does: R = ceil(ceil(n D / 64) / T) of them, 64 at 448 nodes x 64 shells.
//   the LAST to arrive  : the tile walk above; a tile's row weights are the rho workgroups' outputs lut[(i0 + r) * D + d], requested
//                         (into the tile registers) while the tile before is consumed.
// Backward
//   workgroup k < F     : the dS walk above with the tile's weights taken from the saved lut rows, then feature_grads.
//   workgroup F + g     : rows 32 g .. 32 g + 31 in the lane-private bins above; every (row, shell) is an argument of rho of its
//                         own: dl[(i - i_lo) * D + d] = the bin row's sum over the 64 lane columns in lane order (no division, no
//                         sum across rows; an empty shell: exactly 0).  The arguments u_d / max(cnt, 1) take the dead bins' place,
//                         feature_grads runs over the group's rows * D arguments into the group's slot of the workspace
//                         (kRhoSlot floats, small_graph.hip's layout) and the last group to arrive adds the slots in group order.
// =================================================================================================================================

// backward, rho group under pre-rho: S | dY | hop codes as above | dl [32][64] | bins [waves][D][65] (later: the arguments)
constexpr int kPreDl = kRhoBins, kPreBins = kPreDl + kRhoRows * kMidD;
constexpr int kPreBinFloats = static_cast<int>(kBwdDynBytes / 4) - kPreBins;
static_assert(kPreBinFloats >= 2 * kMidD * kBinCols, "two waves' bins fit behind the table gradient at 64 shells");
static_assert(kPreBinFloats >= kRhoRows * kMidD, "a group's arguments fit where its bins were");
constexpr size_t kPreBwdStaticBytes = sizeof(gnan_bwd::RedBuffer) + 16;
static_assert(kFwdDynBytes + kFwdStaticBytes <= 96 * 1024 && kBwdDynBytes + kBwdStaticBytes <= 96 * 1024 &&
              kBwdDynBytes + kPreBwdStaticBytes <= 96 * 1024, "two workgroups per compute unit");

// the row weights of a tile under pre-rho on their way to LDS: the bits of lut[(i0 + r) * D + d] in the tile registers' q ...
template <int ROWS>
__device__ __forceinline__ void tile_fetch_rows(TileRegs<ROWS>& r, const float* lut, int n, int D, int i0) {
  const int rows = n - i0 < ROWS ? n - i0 : ROWS;
#pragma unroll
  for (int u = 0; u < TileRegs<ROWS>::kCnt; ++u) {
    const int e = static_cast<int>(threadIdx.x) + u * kThreads;
    const int rr = e / kWave, d = e % kWave;
    r.q[u] = (rr < rows && d < D) ? __float_as_int(lut[(i0 + rr) * D + d]) : 0;
  }
}

// ... into LDS, [ROWS][64]
template <int ROWS>
__device__ __forceinline__ void tile_store_rows(const TileRegs<ROWS>& r, int D, float* s_w) {
#pragma unroll
  for (int u = 0; u < TileRegs<ROWS>::kCnt; ++u) {
    const int e = static_cast<int>(threadIdx.x) + u * kThreads;
    if (e % kWave < D) s_w[e] = __int_as_float(r.q[u]);
  }
}

// rho workgroups of the pre-rho forward: passes of 64 arguments, at most a feature workgroup's ceil(n / 64) each
inline int pre_rho_workgroups(int n, int D) {
  const int tiles = (n + kTile - 1) / kTile, passes = (n * D + kWave - 1) / kWave;
  return (passes + tiles - 1) / tiles;
}

// P as in mid_graph_kernel (MidDropParams: the shape functions' workgroups mask their hidden activations; rho's never do)
template <class P>
__global__ __launch_bounds__(kThreads) void mid_graph_pre_kernel(const P p) {
  constexpr bool DROP = std::is_same<P, MidDropParams>::value;
  extern __shared__ __attribute__((aligned(16))) float dyn[];
  __shared__ __attribute__((aligned(16))) float weights[kWeightFloats];
  __shared__ unsigned s_last;
  float* col_a = dyn;
  float* col_b = dyn + kMaxH * kWave;
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int k = blockIdx.x, n = p.n, C = p.f.C;
  const int blocks = (n + kTile - 1) / kTile;
  float out[kMaxC];
  const MlpLds wl = carve(weights);
  uint64_t seed = 0ull;
  if constexpr (DROP) seed = p.seed_dev ? *p.seed_dev : p.drop.seed;
  // the first tile's codes are requested now, by every workgroup (any may be the last); its weights exist only after the join
  TileRegs<kTile> regs;
  tile_fetch<kTile>(regs, p.code, nullptr, 0, n, p.D, 0);
  if (k < p.F) {                                       // (mid_graph_kernel's feature workgroup)
    stage_weights(p.f, k, wl);
    float xv[kMidBlocks];
#pragma unroll
    for (int b = 0; b < kMidBlocks; ++b) {
      const int j = b * kWave + lane;
      xv[b] = j < n ? p.x[static_cast<int64_t>(j) * p.x_stride + k] : 0.f;
    }
#pragma unroll
    for (int b = 0; b < kMidBlocks; ++b) {
      const int j = b * kWave + lane;
      if (b < blocks) {                               // (uniform)
        if constexpr (DROP) mlp_block<true>(p.f, wl, xv[b], col_a, col_b, lane, wave, out, p.drop, gnan::drop_base(seed, j, k));
        else mlp_block(p.f, wl, xv[b], col_a, col_b, lane, wave, out);
        if (wave == 0 && j < n)
          for (int c = 0; c < C; ++c) p.part[(static_cast<int64_t>(k) * n + j) * C + c] = out[c];
      }
    }
  } else {
    // rho at this workgroup's run of the n * D normalised distances (GNAN.py:66: torch.div(node_distances, normalization_matrix),
    // IEEE division — small_graph_body's expression), all shell sizes requested before the first MLP
    const int nd = n * p.D, passes = (nd + kWave - 1) / kWave;
    const int lo = (k - p.F) * blocks;
    int q[kMidBlocks];
#pragma unroll
    for (int b = 0; b < kMidBlocks; ++b) {
      const int e = (lo + b) * kWave + lane;
      q[b] = (b < blocks && e < nd) ? p.cnt[(e / p.D) * p.cnt_stride + e % p.D] : 1;
    }
    stage_weights(p.r, 0, wl);
#pragma unroll
    for (int b = 0; b < kMidBlocks; ++b) {
      if (b < blocks && lo + b < passes) {            // (uniform)
        const int e = (lo + b) * kWave + lane;
        const int d = e < nd ? e % p.D : 0;
        const float ud = d < p.D - 1 ? 1.0f / (static_cast<float>(d) + 1.0f) : 0.f;
        mlp_block(p.r, wl, ud / static_cast<float>(q[b] > 1 ? q[b] : 1), col_a, col_b, lane, wave, out);
        if (wave == 0 && e < nd) p.lut[e] = out[0];
      }
    }
  }
  // ---- join: the last workgroup to arrive finishes the graph -----------------------------------------------------------------
  if (!last_to_arrive(p.counter, gridDim.x, &s_last)) return;
  float* s_S = dyn + kFwdS;
  float* s_Y = dyn + kFwdY;
  float* s_w = dyn + kFwdW;
  uint8_t* s_code = reinterpret_cast<uint8_t*>(dyn + kFwdCode);
  const int nc = n * C;
  tile_fetch_rows<kTile>(regs, p.lut, n, p.D, 0);      // the first tile's weights: in flight during the node sums
  for (int e = threadIdx.x; e < nc; e += kThreads) {
    float sum = 0.f;
    for (int k0 = 0; k0 < p.F; k0 += 8) {
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = k0 + u < p.F ? p.part[static_cast<int64_t>(k0 + u) * nc + e] : 0.f;
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (k0 + u < p.F) sum += v[u];
    }
    s_S[e] = sum;
    p.S[e] = sum;
  }
  const int row_bytes = (n & 3) == 0 ? 4 * ((n / 4) | 1) : n;
  for (int t = 0; t < blocks; ++t) {
    const int i0 = t * kTile;
    const int rows = n - i0 < kTile ? n - i0 : kTile;
    __syncthreads();
    tile_store_codes<kTile, true>(regs, p.code, n, i0, s_code);
    tile_store_rows<kTile>(regs, p.D, s_w);
    if (t + 1 < blocks) {
      tile_fetch<kTile>(regs, p.code, nullptr, 0, n, p.D, i0 + kTile);
      tile_fetch_rows<kTile>(regs, p.lut, n, p.D, i0 + kTile);
    }
    __syncthreads();
    for (int e = threadIdx.x; e < rows * C; e += kThreads) {
      const int r = e / C, c = e % C;
      const uint8_t* codes = s_code + r * row_bytes;
      const float* wrow = s_w + r * kWave;
      float acc = 0.f;
#pragma unroll 8
      for (int j = 0; j < n; ++j) {
        int d = codes[j];
        d = d < p.D - 1 ? d : p.D - 1;
        acc = fmaf(wrow[d], s_S[j * C + c], acc);
      }
      s_Y[i0 * C + e] = acc;
      if (p.Y) p.Y[i0 * C + e] = acc;
    }
  }
  __syncthreads();
  if (p.Ysum && static_cast<int>(threadIdx.x) < C) {
    float s = 0.f;
#pragma unroll 8
    for (int i = 0; i < n; ++i) s += s_Y[i * C + threadIdx.x];
    p.Ysum[threadIdx.x] = s;
  }
  if (threadIdx.x == 0) *p.counter = 0u;
}

struct MidPreBwdParams : MidBwdParams {
  float* slots;              // [rho_groups][kRhoSlot] partial gradients of rho (`part` is unused)
};

template <int C>
__device__ __forceinline__ void mid_graph_pre_bwd_body(const MidPreBwdParams& p, float* dyn, gnan_bwd::Drop fdrop) {
  __shared__ gnan_bwd::RedBuffer red;
  __shared__ unsigned s_last;
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int k = blockIdx.x, n = p.n, nc = p.n * C;
  const gnan_bwd::Drop nodrop{0u, 1.f, 0ull};
  if (k < p.F) {
    // ---- mid_graph_bwd_body's operand gradient, the tiles' weights from the saved rows' table -------------------------------------
    float* s_dY = dyn + kBwdDY;
    float* s_g = dyn + kBwdG;
    float* s_u = dyn + kBwdU;
    uint8_t* s_code = reinterpret_cast<uint8_t*>(dyn + kBwdCode);
    const int blocks = (n + kTile - 1) / kTile;
    TileRegs<kTile> regs;
    tile_fetch<kTile>(regs, p.code, nullptr, 0, n, p.D, 0);
    tile_fetch_rows<kTile>(regs, p.lut, n, p.D, 0);
    for (int e = threadIdx.x; e < nc; e += kThreads) {
      s_dY[e] = p.dY ? p.dY[e] : p.dYsum[e % C];
      s_g[e] = 0.f;
    }
    for (int t = 0; t < blocks; ++t) {
      const int i0 = t * kTile;
      const int rows = n - i0 < kTile ? n - i0 : kTile;
      __syncthreads();
      tile_store_codes<kTile, false>(regs, p.code, n, i0, s_code);
      tile_store_rows<kTile>(regs, p.D, s_u);
      if (t + 1 < blocks) {
        tile_fetch<kTile>(regs, p.code, nullptr, 0, n, p.D, i0 + kTile);
        tile_fetch_rows<kTile>(regs, p.lut, n, p.D, i0 + kTile);
      }
      __syncthreads();
      for (int e = threadIdx.x; e < nc; e += kThreads) {          // thread (column j, channel): the tile's rows in ascending order
        const int j = e / C, c = e % C;
        float acc = s_g[e];
#pragma unroll 8
        for (int r = 0; r < rows; ++r) {
          int d = s_code[r * n + j];
          d = d < p.D - 1 ? d : p.D - 1;
          acc = fmaf(s_u[r * kWave + d], s_dY[(i0 + r) * C + c], acc);
        }
        s_g[e] = acc;
      }
    }
    __syncthreads();
    auto x_of = [&](int64_t node) { return p.x[node * p.x_stride + k]; };
    auto g_of = [&](int64_t node, int c) { return s_g[node * C + c]; };
    if (p.f_mid) gnan_bwd::feature_grads<C, true>(p.f, k, 0, n, 0, fdrop, x_of, g_of, red);
    else gnan_bwd::feature_grads<C, false>(p.f, k, 0, n, 0, fdrop, x_of, g_of, red);
    return;
  }
  // ---- table gradient of this group's rows: an entry per (row, shell) -----------------------------------------------------------
  const int grp = k - p.F;
  const int i_lo = grp * kRhoRows;
  const int i_hi = i_lo + kRhoRows < n ? i_lo + kRhoRows : n;
  const int count = (i_hi - i_lo) * p.D;              // this group's arguments of rho
  float* s_S = dyn + kRhoS;
  float* s_dY = dyn + kRhoDY;
  uint8_t* s_code = reinterpret_cast<uint8_t*>(dyn + kRhoCode);
  float* s_dl = dyn + kPreDl;
  float* s_arg = dyn + kPreBins;                       // (once the bins are dead)
  constexpr int kArgs = kRhoRows * kMidD / kThreads;
  int q[kArgs];                                        // the arguments' shell sizes: requested with everything else
  {
    TileRegs<kRhoRows> regs;
    tile_fetch<kRhoRows>(regs, p.code, nullptr, 0, n, p.D, i_lo);
#pragma unroll
    for (int u = 0; u < kArgs; ++u) {
      const int e = static_cast<int>(threadIdx.x) + u * kThreads;
      q[u] = e < count ? p.cnt[(i_lo + e / p.D) * p.cnt_stride + e % p.D] : 1;
    }
    for (int e = threadIdx.x; e < nc; e += kThreads) s_S[e] = p.S[e];
    for (int e = threadIdx.x; e < (i_hi - i_lo) * C; e += kThreads) s_dY[e] = p.dY ? p.dY[i_lo * C + e] : p.dYsum[e % C];
    tile_store_codes<kRhoRows, false>(regs, p.code, n, i_lo, s_code);
  }
  const int nw = kWaves * p.D * kBinCols <= kPreBinFloats ? kWaves : 2;     // waves that bin: as many as have room for [D][65]
  float* bins = dyn + kPreBins + wave * p.D * kBinCols;
  __syncthreads();
  for (int rr = 0; i_lo + nw * rr < i_hi; ++rr) {
    const int i = i_lo + nw * rr + wave;
    const bool live = wave < nw && i < i_hi;
    if (live) {
      for (int d = 0; d < p.D; ++d) bins[d * kBinCols + lane] = 0.f;
      float gy[C];
#pragma unroll
      for (int c = 0; c < C; ++c) gy[c] = s_dY[(i - i_lo) * C + c];
      const uint8_t* codes = s_code + (i - i_lo) * n;
      for (int j = lane; j < n; j += kWave) {          // (a lane owns its column of the bins: no other lane writes it)
        int d = codes[j];
        d = d < p.D - 1 ? d : p.D - 1;
        float v = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) v = fmaf(gy[c], s_S[j * C + c], v);
        bins[d * kBinCols + lane] += v;
      }
    }
    __syncthreads();
    if (live && lane < p.D) {
      float sum = 0.f;
#pragma unroll 8
      for (int l = 0; l < kWave; ++l) sum += bins[lane * kBinCols + l];
      s_dl[(i - i_lo) * p.D + lane] = sum;             // every (row, shell) is an argument of rho of its own
    }
    __syncthreads();
  }
#pragma unroll
  for (int u = 0; u < kArgs; ++u) {
    const int e = static_cast<int>(threadIdx.x) + u * kThreads;
    if (e < count) {
      const int d = e % p.D;
      const float ud = d < p.D - 1 ? 1.0f / (static_cast<float>(d) + 1.0f) : 0.f;
      s_arg[e] = ud / static_cast<float>(q[u] > 1 ? q[u] : 1);
    }
  }
  __syncthreads();
  // rho's parameter gradients over this group's arguments, into its slot (small_graph_bwd_body's slot layout)
  {
    auto ua_of = [&](int64_t e) { return s_arg[e]; };
    auto ga_of = [&](int64_t e, int) { return s_dl[e]; };
    float* slot = p.slots + static_cast<int64_t>(grp) * kRhoSlot;
    gnan_bwd::Weights w = p.r;
    w.d_w_mid = slot;
    w.d_w_first = slot + kMaxH * kMaxH; w.d_b_first = p.r.d_b_first ? slot + kMaxH * kMaxH + kMaxH : nullptr;
    w.d_b_mid = p.r.d_b_mid ? slot + kMaxH * kMaxH + 2 * kMaxH : nullptr; w.d_w_last = slot + kMaxH * kMaxH + 3 * kMaxH;
    w.d_b_last = p.r.d_b_last ? slot + kMaxH * kMaxH + 4 * kMaxH : nullptr;
    if (p.r_mid) gnan_bwd::feature_grads<1, true>(w, 0, 0, count, 0, nodrop, ua_of, ga_of, red);
    else gnan_bwd::feature_grads<1, false>(w, 0, 0, count, 0, nodrop, ua_of, ga_of, red);
  }
  // ---- join of the rho groups: the last to arrive adds the slots in group order (small_graph_bwd_body's join, 14 groups) ---------
  if (!last_to_arrive(p.counter, static_cast<unsigned>(p.rho_groups), &s_last)) return;
  const int H = p.r.H;
  float* const vec[5] = {p.r.d_w_first, p.r.d_b_first, p.r_mid ? p.r.d_b_mid : nullptr, p.r.d_w_last, p.r.d_b_last};
  float* const dW2 = p.r_mid ? p.r.d_w_mid : nullptr;
  for (int e4 = threadIdx.x; e4 < kRhoSlot / 4; e4 += kThreads) {
    float4 v[kRhoGroupsMid];                           // (all groups' terms requested together, 16 bytes each)
#pragma unroll
    for (int g = 0; g < kRhoGroupsMid; ++g) {
      const int gg = g < p.rho_groups ? g : 0;
      v[g] = *reinterpret_cast<const float4*>(p.slots + static_cast<int64_t>(gg) * kRhoSlot + 4 * e4);
    }
    float sum[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int g = 0; g < kRhoGroupsMid; ++g) {
      if (g < p.rho_groups) { sum[0] += v[g].x; sum[1] += v[g].y; sum[2] += v[g].z; sum[3] += v[g].w; }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int idx = 4 * e4 + u;
      if (idx < kMaxH * kMaxH) {
        if (dW2 && idx < H * H) dW2[idx] = sum[u];
      } else {
        const int t = (idx - kMaxH * kMaxH) / kMaxH, e = (idx - kMaxH * kMaxH) % kMaxH;
        if (vec[t] && e < (t == 4 ? 1 : H)) vec[t][e] = sum[u];
      }
    }
  }
  if (threadIdx.x == 0) *p.counter = 0u;
}

template <int C>
__global__ __launch_bounds__(kThreads) void mid_graph_pre_bwd_kernel(const MidPreBwdParams p) {
  extern __shared__ __attribute__((aligned(16))) float dyn[];
  mid_graph_pre_bwd_body<C>(p, dyn, gnan_bwd::Drop{0u, 1.f, 0ull});
}

// ... of a forward under Dropout
template <int C>
__global__ __launch_bounds__(kThreads) void mid_graph_pre_bwd_drop_kernel(const MidPreBwdParams p, gnan_bwd::Drop drop,
                                                                          const uint64_t* seed_dev) {
  extern __shared__ __attribute__((aligned(16))) float dyn[];
  if (seed_dev) drop.seed = *seed_dev;
  mid_graph_pre_bwd_body<C>(p, dyn, drop);
}

template <int C>
int launch_mid_pre_bwd(const MidPreBwdParams& p, const gnan_bwd::Drop& drop, const uint64_t* seed_dev, hipStream_t st) {
  const dim3 grid(static_cast<unsigned>(p.F + p.rho_groups));
  if (drop.thresh != 0u) {
    if (int rc = raise_dyn_lds<&mid_graph_pre_bwd_drop_kernel<C>>(kBwdDynBytes, "mid_graph_bwd")) return rc;
    hipLaunchKernelGGL((mid_graph_pre_bwd_drop_kernel<C>), grid, dim3(kThreads), kBwdDynBytes, st, p, drop, seed_dev);
    return gnan::check_launch("mid_graph_pre_bwd_drop_kernel");
  }
  if (int rc = raise_dyn_lds<&mid_graph_pre_bwd_kernel<C>>(kBwdDynBytes, "mid_graph_bwd")) return rc;
  hipLaunchKernelGGL((mid_graph_pre_bwd_kernel<C>), grid, dim3(kThreads), kBwdDynBytes, st, p);
  return gnan::check_launch("mid_graph_pre_bwd_kernel");
}

// `reserved` of both argument structs: 0, or GNAN_MID_PRE_RHO — which needs the shell sizes (refused as gnan_small_graph_fwd does)
template <class A>
int pre_rho_ok(const char* who, const A* a) {
  GNAN_REQUIRE(a->reserved == 0 || a->reserved == GNAN_MID_PRE_RHO, "%s: reserved must be 0 or %d = pre-rho (got reserved=%d)", who,
               GNAN_MID_PRE_RHO, a->reserved);
  if (a->reserved == GNAN_MID_PRE_RHO && a->cnt == nullptr)
    return gnan::fail(GNAN_ERR_UNSUPPORTED, "%s: pre-rho normalisation needs the shell sizes (got cnt=%p)", who,
                      static_cast<const void*>(a->cnt));
  return GNAN_OK;
}

}  // namespace

extern "C" size_t gnan_mid_graph_workspace_bytes(int32_t n, int32_t F, int32_t C) {
  return 16 + static_cast<size_t>(F) * n * C * sizeof(float);      // counter (own 16 bytes) | part [F, n, C]
}

extern "C" size_t gnan_mid_graph_bwd_workspace_bytes(int32_t n, int32_t D) {
  (void)D;
  return 16 + static_cast<size_t>((n + kRhoRows - 1) / kRhoRows) * kWave * sizeof(double);      // counter | dlut partials [groups][64]
}

extern "C" int gnan_mid_graph_describe(int32_t n, int32_t F, int32_t D, int32_t C, gnan_mid_graph_info* out) {
  GNAN_REQUIRE(out != nullptr, "mid_graph_describe: null out");
  gnan_small_mlp f{};
  f.L = 3; f.H = 1; f.C = C;
  if (int rc = shape_ok("mid_graph_describe", kMidCover, n, F, D, &f, nullptr)) return rc;
  out->row_tiles = (n + kTile - 1) / kTile;
  out->rho_groups = (n + kRhoRows - 1) / kRhoRows;
  out->fwd_grid = F + 1;
  out->bwd_grid = F + out->rho_groups;
  out->fwd_lds_bytes = static_cast<int32_t>(kFwdDynBytes + kFwdStaticBytes);
  out->bwd_lds_bytes = static_cast<int32_t>(kBwdDynBytes + kBwdStaticBytes);
  out->fwd_workspace_bytes = static_cast<int64_t>(gnan_mid_graph_workspace_bytes(n, F, C));
  out->bwd_workspace_bytes = static_cast<int64_t>(gnan_mid_graph_bwd_workspace_bytes(n, D));
  return GNAN_OK;
}

extern "C" size_t gnan_mid_graph_pre_bwd_workspace_bytes(int32_t n, int32_t D) {
  (void)D;
  return 16 + static_cast<size_t>((n + kRhoRows - 1) / kRhoRows) * kRhoSlot * sizeof(float);      // counter | slots [groups][kRhoSlot]
}

extern "C" int gnan_mid_graph_pre_describe(int32_t n, int32_t F, int32_t D, int32_t C, gnan_mid_graph_info* out) {
  if (int rc = gnan_mid_graph_describe(n, F, D, C, out)) return rc;
  out->fwd_grid = F + pre_rho_workgroups(n, D);
  out->bwd_lds_bytes = static_cast<int32_t>(kBwdDynBytes + kPreBwdStaticBytes);
  out->bwd_workspace_bytes = static_cast<int64_t>(gnan_mid_graph_pre_bwd_workspace_bytes(n, D));
  return GNAN_OK;
}

namespace {
// THE launcher of gnan_mid_graph_fwd (drop.thresh == 0), gnan_mid_graph_fwd_drop and gnan_mid_graph_fwd_drop_dev (seed_dev: the seed's
// device cell, else NULL)
int mid_fwd(const gnan_mid_graph_args* a, const gnan_bwd::Drop& drop, const uint64_t* seed_dev, gnan_stream_t stream) {
  if (int rc = pre_rho_ok("mid_graph", a)) return rc;
  if (int rc = shape_ok("mid_graph", kMidCover, a->n, a->F, a->D, &a->f, &a->rho)) return rc;
  GNAN_REQUIRE(a->x != nullptr, "mid_graph: null x");
  GNAN_REQUIRE(a->code != nullptr, "mid_graph: null code");
  GNAN_REQUIRE(reinterpret_cast<uintptr_t>(a->code) % 4 == 0, "mid_graph: code must be 4-byte aligned (got %p)",
               static_cast<const void*>(a->code));
  GNAN_REQUIRE(a->S && a->lut && (a->Y || a->Ysum), "mid_graph: null S / lut / outputs");
  GNAN_REQUIRE(mlp_ptrs_ok(&a->f) && mlp_ptrs_ok(&a->rho), "mid_graph: null weights");
  if (int rc = strides_ok("mid_graph", a)) return rc;
  if (int rc = workspace_ok("mid_graph", a, gnan_mid_graph_workspace_bytes(a->n, a->F, a->f.C))) return rc;
  MidDropParams p;
  fwd_fields(p, a, a->n);
  p.S = a->S; p.lut = a->lut; p.Y = a->Y; p.Ysum = a->Ysum;
  split_workspace(a->workspace, p.counter, p.part);
  if (a->reserved == GNAN_MID_PRE_RHO) {                // (kernels of their own: F + R workgroups)
    const dim3 pre_grid(static_cast<unsigned>(a->F + pre_rho_workgroups(a->n, a->D)));
    if (drop.thresh != 0u) {
      p.drop = drop; p.seed_dev = seed_dev;
      if (int rc = raise_dyn_lds<&mid_graph_pre_kernel<MidDropParams>>(kFwdDynBytes, "mid_graph")) return rc;
      hipLaunchKernelGGL(mid_graph_pre_kernel<MidDropParams>, pre_grid, dim3(kThreads), kFwdDynBytes, static_cast<hipStream_t>(stream), p);
      return gnan::check_launch("mid_graph_pre_kernel (Dropout)");
    }
    if (int rc = raise_dyn_lds<&mid_graph_pre_kernel<MidParams>>(kFwdDynBytes, "mid_graph")) return rc;
    hipLaunchKernelGGL(mid_graph_pre_kernel<MidParams>, pre_grid, dim3(kThreads), kFwdDynBytes, static_cast<hipStream_t>(stream),
                       static_cast<const MidParams&>(p));
    return gnan::check_launch("mid_graph_pre_kernel");
  }
  const dim3 grid(static_cast<unsigned>(a->F) + 1u);
  if (drop.thresh != 0u) {                             // (the Dropout instance: a kernel of its own, the other untouched)
    p.drop = drop; p.seed_dev = seed_dev;
    if (int rc = raise_dyn_lds<&mid_graph_kernel<MidDropParams>>(kFwdDynBytes, "mid_graph")) return rc;
    hipLaunchKernelGGL(mid_graph_kernel<MidDropParams>, grid, dim3(kThreads), kFwdDynBytes, static_cast<hipStream_t>(stream), p);
    return gnan::check_launch("mid_graph_kernel (Dropout)");
  }
  if (int rc = raise_dyn_lds<&mid_graph_kernel<MidParams>>(kFwdDynBytes, "mid_graph")) return rc;
  hipLaunchKernelGGL(mid_graph_kernel<MidParams>, grid, dim3(kThreads), kFwdDynBytes, static_cast<hipStream_t>(stream),
                     static_cast<const MidParams&>(p));
  return gnan::check_launch("mid_graph_kernel");
}
}  // namespace

extern "C" int gnan_mid_graph_fwd(const gnan_mid_graph_args* a, gnan_stream_t stream) {
  GNAN_REQUIRE(a != nullptr, "mid_graph: null args");
  return mid_fwd(a, gnan_bwd::Drop{0u, 1.f, 0ull}, nullptr, stream);
}

extern "C" int gnan_mid_graph_fwd_drop(const gnan_mid_graph_args* a, const gnan_small_dropout* d, gnan_stream_t stream) {
  GNAN_REQUIRE(a != nullptr, "mid_graph: null args");
  gnan_bwd::Drop drop;
  if (int rc = drop_ok("mid_graph", d, &drop)) return rc;
  return mid_fwd(a, drop, nullptr, stream);
}

extern "C" int gnan_mid_graph_fwd_drop_dev(const gnan_mid_graph_args* a, const gnan_small_dropout_dev* d, gnan_stream_t stream) {
  GNAN_REQUIRE(a != nullptr, "mid_graph: null args");
  gnan_bwd::Drop drop;
  const uint64_t* seed_dev = nullptr;
  if (int rc = drop_dev_ok("mid_graph", d, &drop, &seed_dev)) return rc;
  return mid_fwd(a, drop, seed_dev, stream);
}

namespace {
// THE launcher of gnan_mid_graph_bwd (drop.thresh == 0), gnan_mid_graph_bwd_drop and gnan_mid_graph_bwd_drop_dev
int mid_bwd(const gnan_mid_graph_bwd_args* a, const gnan_bwd::Drop& drop, const uint64_t* seed_dev, gnan_stream_t stream) {
  if (int rc = pre_rho_ok("mid_graph_bwd", a)) return rc;
  const bool pre = a->reserved == GNAN_MID_PRE_RHO;
  if (int rc = shape_ok("mid_graph_bwd", kMidCover, a->n, a->F, a->D, &a->f, &a->rho)) return rc;
  GNAN_REQUIRE(a->x != nullptr, "mid_graph_bwd: null x");
  GNAN_REQUIRE(a->code != nullptr, "mid_graph_bwd: null code");
  GNAN_REQUIRE(reinterpret_cast<uintptr_t>(a->code) % 4 == 0, "mid_graph_bwd: code must be 4-byte aligned (got %p)",
               static_cast<const void*>(a->code));
  GNAN_REQUIRE(a->S && a->lut && (a->dY || a->dYsum), "mid_graph_bwd: null S / lut / output gradient");
  GNAN_REQUIRE(mlp_ptrs_ok(&a->f) && mlp_ptrs_ok(&a->rho), "mid_graph_bwd: null weights");
  if (int rc = strides_ok("mid_graph_bwd", a)) return rc;
  GNAN_REQUIRE(grads_ok(&a->f, &a->df) && grads_ok(&a->rho, &a->drho),
               "mid_graph_bwd: a gradient pointer for every weight, and for a bias exactly where there is one");
  if (int rc = workspace_ok("mid_graph_bwd", a, pre ? gnan_mid_graph_pre_bwd_workspace_bytes(a->n, a->D)
                                                    : gnan_mid_graph_bwd_workspace_bytes(a->n, a->D))) return rc;
  GNAN_REQUIRE(reinterpret_cast<uintptr_t>(a->workspace) % 8 == 0, "mid_graph_bwd: workspace must be 8-byte aligned (got %p)", a->workspace);
  MidPreBwdParams p;
  bwd_fields(p, a, a->n, &a->df, &a->drho);
  p.S = a->S; p.lut = a->lut; p.dY = a->dY; p.dYsum = a->dYsum;
  p.rho_groups = (a->n + kRhoRows - 1) / kRhoRows;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (pre) {                                           // (kernels of their own: rho's partial gradients in slots)
    p.part = nullptr;
    split_workspace(a->workspace, p.counter, p.slots);
    return with_channels(a->f.C, [&](auto c) { return launch_mid_pre_bwd<decltype(c)::value>(p, drop, seed_dev, st); });
  }
  p.slots = nullptr;
  split_workspace(a->workspace, p.counter, p.part);
  return with_channels(a->f.C, [&](auto c) { return launch_mid_bwd<decltype(c)::value>(p, drop, seed_dev, st); });
}
}  // namespace

extern "C" int gnan_mid_graph_bwd(const gnan_mid_graph_bwd_args* a, gnan_stream_t stream) {
  GNAN_REQUIRE(a != nullptr, "mid_graph_bwd: null args");
  return mid_bwd(a, gnan_bwd::Drop{0u, 1.f, 0ull}, nullptr, stream);
}

extern "C" int gnan_mid_graph_bwd_drop(const gnan_mid_graph_bwd_args* a, const gnan_small_dropout* d, gnan_stream_t stream) {
  GNAN_REQUIRE(a != nullptr, "mid_graph_bwd: null args");
  gnan_bwd::Drop drop;
  if (int rc = drop_ok("mid_graph_bwd", d, &drop)) return rc;
  return mid_bwd(a, drop, nullptr, stream);
}

extern "C" int gnan_mid_graph_bwd_drop_dev(const gnan_mid_graph_bwd_args* a, const gnan_small_dropout_dev* d, gnan_stream_t stream) {
  GNAN_REQUIRE(a != nullptr, "mid_graph_bwd: null args");
  gnan_bwd::Drop drop;
  const uint64_t* seed_dev = nullptr;
  if (int rc = drop_dev_ok("mid_graph_bwd", d, &drop, &seed_dev)) return rc;
  return mid_bwd(a, drop, seed_dev, stream);
}
