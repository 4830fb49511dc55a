// The NAM read-out of a graph-level task (csrc/small_graph_nam.hip: models.py:358-384 with is_graph_task and readout_n_layers > 0)
// for dense-coded graphs of up to 448 nodes: the function, the arithmetic and the leftovers of small_graph_nam_kernel, with the graph
// walked in csrc/mid_graph.hip's TILES OF 64 ROWS (csrc/mid_graph_tiles.hpp), so that a [64][n] block of hop codes and a [64][64]
// block of row weights is all of the graph a workgroup holds at a time.
//   out[c] = sum_k nam_k(hidden[k])[c],  hidden[k] = sum_j colw[j] f_k(x[j, k]),  colw[j] = sum_i lut[d] / max(cnt[i, d], 1),
//   d = min(code[i, j], D - 1),  lut[d] = rho(u_d).  f and rho are one-wide; post-rho shell normalisation, or none.
//
// Forward, ONE launch of F workgroups, none of which waits:
//   workgroup k : rho on the D distances (a block of 64 inputs); colw over the row tiles in ascending row order — thread j owns
//                 column j (and j + 256), the tile's rows added in ascending order, the next tile's codes and shell sizes requested
//                 into registers before the current one is consumed (mid_graph_bwd_body's walk with C = 1, dY = 1); f_k on the
//                 nodes in blocks of 64 -> fx[k, :]; hidden[k]: lane l adds colw[j] * fx[j] (one fma each) over j = l, l + 64, ...
//                 in ascending order, then the butterfly over the lanes (xor 32, 16, ..., 1) — small_graph_nam_kernel's order;
//                 nam_k on it -> part[k, :].  Workgroup 0 also writes lut [D] and colw [n].
//   the LAST workgroup to arrive adds the features' parts in feature order into out [C] and zeroes the counter.
// Backward, ONE entry point, TWO launches on the caller's stream (stream order is their only dependency), no workgroup waits:
//   launch A, F workgroups    : nam_k's parameter gradients and d hidden[k] (feature_grads<CN, MID, true> on the single input), stored
//                               to the workspace; f_k's parameter gradients from g[j] = colw[j] * d hidden[k], colw as the forward left
//                               it.  No join.
//   launch B, ceil(n / 32)    : every group forms T[j] = sum_k d hidden[k] fx[k, j] itself, in feature order (chunks of 64 features);
//   rho groups                  then mid_graph_bwd_body's rho-group body with C = 1, S := T, dY = 1 — a row per wave at a time, T binned
//                               by hop code in lane-private LDS columns ([D][65]), the bin rows added in lane order, float64 across
//                               rows — left as float64 partials [group][64] in the workspace; the last group to arrive adds the
//                               partials in group order, zeroes the counter and runs feature_grads on rho's D arguments.
// Fixed orders throughout, no float atomics: two runs give the same bits.
#include <cstdint>

#include "mid_graph_tiles.hpp"

namespace {

using namespace gnan_mid;

// ---- LDS plans (floats unless said otherwise): one size per kernel, the largest admitted shape ----------------------------------------
// forward: colw [448] | fx [448] | { activation columns 2 x [64][64]  or  row weights [64][64] | hop codes [64][n] bytes }
constexpr int kNamColw = 0, kNamFx = kMidNodes, kNamCols = 2 * kMidNodes, kNamW = kNamCols, kNamCode = kNamW + kTile * kWave;
constexpr size_t kNamFwdDynBytes = static_cast<size_t>(kNamCode) * 4 + static_cast<size_t>(kTile) * kMidNodes;
constexpr size_t kNamFwdStaticBytes = (kWeightFloats + kWave) * 4 + 16;                  // weight image | lut | the arrival slot
static_assert(kNamFwdDynBytes >= static_cast<size_t>(kNamCols + 2 * kMaxH * kWave) * 4, "the activation columns fit where the tile was");
// backward A: colw [448]
constexpr size_t kNamADynBytes = static_cast<size_t>(kMidNodes) * 4;
constexpr size_t kNamAStaticBytes = sizeof(gnan_bwd::RedBuffer) + kMaxH * 4;              // reduction buffer | d hidden
// backward B: T [448] | hop codes [32][n] bytes | bins [waves][D][65]: all four waves bin up to 44 shells, two above
constexpr int kNamT = 0, kNamRhoCode = kMidNodes, kNamBins = kNamRhoCode + kRhoRows * kMidNodes / 4;
constexpr int kNamBinFloats = 11440;
static_assert(kNamBinFloats >= 2 * kMidD * kBinCols, "two waves' bins fit at 64 shells");
constexpr size_t kNamBDynBytes = static_cast<size_t>(kNamBins + kNamBinFloats) * 4;
constexpr size_t kNamBStaticBytes =                                                       // red | partials | table gradient | d hidden | slot
    sizeof(gnan_bwd::RedBuffer) + kWaves * kWave * sizeof(double) + kWave * 4 + kMaxH * 4 + 16;
static_assert(kNamFwdDynBytes + kNamFwdStaticBytes <= 96 * 1024 && kNamADynBytes + kNamAStaticBytes <= 96 * 1024 &&
              kNamBDynBytes + kNamBStaticBytes <= 96 * 1024, "two workgroups per compute unit");

struct MidNamParams {
  const float* x;
  int64_t x_stride;
  int n, F;
  Mlp f, r, nam;             // nam.L may be 1 (Linear(1, C): w_last [F, C])
  const uint8_t* code;
  int D;
  const int32_t* cnt;
  int64_t cnt_stride;
  float *fx, *lut, *hidden, *colw, *out, *part;
  unsigned* counter;         // zero before the first launch; the last workgroup zeroes it again
};

__global__ __launch_bounds__(kThreads) void mid_graph_nam_kernel(const MidNamParams p) {
  extern __shared__ __attribute__((aligned(16))) float dyn[];
  __shared__ __attribute__((aligned(16))) float weights[kWeightFloats];
  __shared__ float s_lut[kWave];
  __shared__ unsigned s_last;
  float* s_colw = dyn + kNamColw;
  float* s_fx = dyn + kNamFx;
  float* col_a = dyn + kNamCols;
  float* col_b = col_a + kMaxH * kWave;
  float* s_u = dyn + kNamW;
  uint8_t* s_code = reinterpret_cast<uint8_t*>(dyn + kNamCode);
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int k = blockIdx.x, n = p.n, D = p.D, C = p.nam.C;
  const int blocks = (n + kTile - 1) / kTile;
  const MlpLds wl = carve(weights);
  float out[kMaxC];
  // the first tile's codes and shell sizes and every node block's input are requested now: they fly during rho's MLP
  TileRegs<kTile> regs;
  tile_fetch<kTile>(regs, p.code, p.cnt, p.cnt_stride, n, D, 0);
  float xv[kMidBlocks];
#pragma unroll
  for (int b = 0; b < kMidBlocks; ++b) {
    const int j = b * kWave + lane;
    xv[b] = j < n ? p.x[static_cast<int64_t>(j) * p.x_stride + k] : 0.f;
  }
  // ---- rho on the distinct distances ------------------------------------------------------------------------------------------------
  stage_weights(p.r, 0, wl);
  {
    const float u = lane < D - 1 ? 1.0f / (static_cast<float>(lane) + 1.0f) : 0.f;      // graph.hop_inputs
    mlp_block(p.r, wl, u, col_a, col_b, lane, wave, out);
    if (wave == 0) {
      s_lut[lane] = lane < D ? out[0] : 0.f;
      if (k == 0 && lane < D) p.lut[lane] = out[0];
    }
  }
  for (int j = threadIdx.x; j < n; j += kThreads) s_colw[j] = 0.f;
  // ---- the column sums over the row tiles (mid_graph_bwd_body's walk with C = 1 and dY = 1: the product with 1 is exact) ------------------
  for (int t = 0; t < blocks; ++t) {
    const int i0 = t * kTile;
    const int rows = n - i0 < kTile ? n - i0 : kTile;
    __syncthreads();                                  // (the tile before is consumed; first round: the table is in place, the columns dead)
    tile_store_codes<kTile, false>(regs, p.code, n, i0, s_code);
    tile_store_weights<kTile>(regs, s_lut, p.cnt != nullptr, D, s_u);
    if (t + 1 < blocks) tile_fetch<kTile>(regs, p.code, p.cnt, p.cnt_stride, n, D, i0 + kTile);
    __syncthreads();
    for (int j = threadIdx.x; j < n; j += kThreads) {           // thread = column j: the tile's rows in ascending order
      float acc = s_colw[j];
#pragma unroll 8
      for (int r = 0; r < rows; ++r) {
        int d = s_code[r * n + j];
        d = d < D - 1 ? d : D - 1;
        acc += s_u[r * kWave + d];
      }
      s_colw[j] = acc;
    }
  }
  __syncthreads();                                    // (the tile is dead: the columns take its place)
  if (k == 0)
    for (int j = threadIdx.x; j < n; j += kThreads) p.colw[j] = s_colw[j];
  // ---- f_k on the nodes, hidden_k ---------------------------------------------------------------------------------------------------
  stage_weights(p.f, k, wl);
#pragma unroll
  for (int b = 0; b < kMidBlocks; ++b) {
    const int j = b * kWave + lane;
    if (b < blocks) {                                 // (uniform)
      mlp_block(p.f, wl, xv[b], col_a, col_b, lane, wave, out);
      if (wave == 0 && j < n) {
        s_fx[j] = out[0];
        p.fx[static_cast<int64_t>(k) * n + j] = out[0];
      }
    }
  }
  __syncthreads();
  float h = 0.f;
#pragma unroll
  for (int b = 0; b < kMidBlocks; ++b) {              // lane l: nodes l, l + 64, ... in ascending order
    const int j = b * kWave + lane;
    if (j < n) h = fmaf(s_colw[j], s_fx[j], h);
  }
#pragma unroll
  for (int off = kWave / 2; off >= 1; off >>= 1) h += __shfl_xor(h, off, kWave);      // the same sum in every lane of every wave
  if (threadIdx.x == 0) p.hidden[k] = h;
  // ---- NAM_k ------------------------------------------------------------------------------------------------------------------------
  if (p.nam.L == 1) {
    if (static_cast<int>(threadIdx.x) < C)
      p.part[k * C + threadIdx.x] = fmaf(p.nam.w_last[k * C + threadIdx.x], h, p.nam.b_last ? p.nam.b_last[k * C + threadIdx.x] : 0.f);
  } else {
    stage_weights(p.nam, k, wl);
    mlp_block(p.nam, wl, h, col_a, col_b, lane, wave, out);
    if (threadIdx.x == 0)
      for (int c = 0; c < C; ++c) p.part[k * C + c] = out[c];
  }
  // ---- join: the last workgroup adds the features in order (small_graph_nam_kernel's join; colw is dead: its first C floats are the sums) --
  if (!last_to_arrive(p.counter, gridDim.x, &s_last)) return;
  const int chunk = kWeightFloats / C * C;           // whole features per pass through the (now free) weight image
  for (int e0 = 0; e0 < p.F * C; e0 += chunk) {
    const int en = p.F * C - e0 < chunk ? p.F * C - e0 : chunk;
    __syncthreads();
    for (int e = threadIdx.x; e < en; e += kThreads) weights[e] = p.part[e0 + e];
    __syncthreads();
    if (static_cast<int>(threadIdx.x) < C) {
      float s = e0 == 0 ? 0.f : s_colw[threadIdx.x];
      for (int e = threadIdx.x; e < en; e += C) s += weights[e];
      s_colw[threadIdx.x] = s;
    }
  }
  __syncthreads();
  if (static_cast<int>(threadIdx.x) < C) p.out[threadIdx.x] = s_colw[threadIdx.x];
  if (threadIdx.x == 0) *p.counter = 0u;
}

// -----------------------------------------------------------------------------------------------------------------------------------------
struct MidNamBwdParams {
  const float* x;
  int64_t x_stride;
  int n, F;
  gnan_bwd::Weights f, r, nam;
  int f_mid, r_mid, nam_L;
  const uint8_t* code;
  int D;
  const int32_t* cnt;
  int64_t cnt_stride;
  const float *fx, *lut, *hidden, *colw, *d_out;
  int rho_groups;
  float* dh;                 // [F] workspace: d hidden_k, written by launch A, read by launch B
  double* part;              // [rho_groups][64] partial table gradients
  unsigned* counter;         // arrivals of the rho groups
};

// launch A: workgroup k — nam_k's gradients, d hidden_k, f_k's gradients
template <int CN>
__global__ __launch_bounds__(kThreads) void mid_graph_nam_bwd_feature_kernel(const MidNamBwdParams p) {
  __shared__ gnan_bwd::RedBuffer red;
  extern __shared__ __attribute__((aligned(16))) float dyn[];
  __shared__ float s_dh[kMaxH];
  float* s_colw = dyn;
  const int k = blockIdx.x, n = p.n;
  const gnan_bwd::Drop nodrop{0u, 1.f, 0ull};
  for (int j = threadIdx.x; j < n; j += kThreads) s_colw[j] = p.colw[j];
  // ---- NAM_k: parameter gradients and d hidden_k (small_graph_nam_bwd_kernel's) ------------------------------------------------------
  const float h = p.hidden[k];
  if (p.nam_L == 1) {
    if (static_cast<int>(threadIdx.x) < CN) {
      const float g = p.d_out[threadIdx.x];
      p.nam.d_w_last[k * CN + threadIdx.x] = g * h;
      if (p.nam.d_b_last) p.nam.d_b_last[k * CN + threadIdx.x] = g;
    }
    if (threadIdx.x == 0) {
      float s = 0.f;
      for (int c = 0; c < CN; ++c) s = fmaf(p.d_out[c], p.nam.w_last[k * CN + c], s);
      s_dh[0] = s;
    }
  } else {
    auto h_of = [&](int64_t) { return h; };
    auto go_of = [&](int64_t, int c) { return p.d_out[c]; };
    if (p.nam_L == 3) gnan_bwd::feature_grads<CN, true, true>(p.nam, k, 0, 1, 0, nodrop, h_of, go_of, red, s_dh);
    else gnan_bwd::feature_grads<CN, false, true>(p.nam, k, 0, 1, 0, nodrop, h_of, go_of, red, s_dh);
  }
  __syncthreads();
  const float dh = s_dh[0];
  if (threadIdx.x == 0) p.dh[k] = dh;                  // (launch B reads it: stream order)
  // ---- f_k's parameter gradients from dfx[j] = colw_j * d hidden_k ---------------------------------------------------------------------
  auto x_of = [&](int64_t node) { return p.x[node * p.x_stride + k]; };
  auto g_of = [&](int64_t node, int) { return s_colw[node] * dh; };
  if (p.f_mid) gnan_bwd::feature_grads<1, true>(p.f, k, 0, n, 0, nodrop, x_of, g_of, red);
  else gnan_bwd::feature_grads<1, false>(p.f, k, 0, n, 0, nodrop, x_of, g_of, red);
}

// launch B: rho group g — T, the table gradient of rows 32 g .. 32 g + 31; the last to arrive: rho's parameter gradients
__global__ __launch_bounds__(kThreads) void mid_graph_nam_bwd_rho_kernel(const MidNamBwdParams p) {
  extern __shared__ __attribute__((aligned(16))) float dyn[];
  __shared__ gnan_bwd::RedBuffer red;
  __shared__ double s_part[kWaves][kWave];
  __shared__ float s_dl[kWave];
  __shared__ float s_dh[kMaxH];
  __shared__ unsigned s_last;
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int grp = blockIdx.x, n = p.n;
  const int i_lo = grp * kRhoRows;
  const int i_hi = i_lo + kRhoRows < n ? i_lo + kRhoRows : n;
  float* s_T = dyn + kNamT;
  uint8_t* s_code = reinterpret_cast<uint8_t*>(dyn + kNamRhoCode);
  TileRegs<kRhoRows> regs;
  tile_fetch<kRhoRows>(regs, p.code, nullptr, 0, n, p.D, i_lo);
  // T_j = sum_k d hidden_k fx[k, j]: chunks of 64 features through LDS, features in ascending order (small_graph_nam_bwd_kernel's loop)
  for (int j = threadIdx.x; j < n; j += kThreads) s_T[j] = 0.f;
  for (int k0 = 0; k0 < p.F; k0 += kMaxH) {
    __syncthreads();
    if (static_cast<int>(threadIdx.x) < kMaxH && k0 + static_cast<int>(threadIdx.x) < p.F) s_dh[threadIdx.x] = p.dh[k0 + threadIdx.x];
    __syncthreads();
    const int kn = p.F - k0 < kMaxH ? p.F - k0 : kMaxH;
    for (int j = threadIdx.x; j < n; j += kThreads) {
      float t = s_T[j];
      for (int kk = 0; kk < kn; kk += 8) {            // eight features' terms requested together (a load -> fma loop waits for each)
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = kk + u < kn ? p.fx[static_cast<int64_t>(k0 + kk + u) * n + j] : 0.f;
#pragma unroll
        for (int u = 0; u < 8; ++u) t = fmaf(kk + u < kn ? s_dh[kk + u] : 0.f, v[u], t);
      }
      s_T[j] = t;
    }
  }
  tile_store_codes<kRhoRows, false>(regs, p.code, n, i_lo, s_code);
  // ---- table gradient of this group's rows (mid_graph_bwd_body's rho group with C = 1, S := T, dY = 1) -----------------------------------
  const int nw = kWaves * p.D * kBinCols <= kNamBinFloats ? kWaves : 2;      // waves that bin: as many as have room for [D][65]
  float* bins = dyn + kNamBins + wave * p.D * kBinCols;
  double acc = 0.0;                                                        // lane d: dlut[d] over this wave's rows
  __syncthreads();
  for (int rr = 0; i_lo + nw * rr < i_hi; ++rr) {
    const int i = i_lo + nw * rr + wave;
    const bool live = wave < nw && i < i_hi;
    if (live) {
      for (int d = 0; d < p.D; ++d) bins[d * kBinCols + lane] = 0.f;
      const uint8_t* codes = s_code + (i - i_lo) * n;
      for (int j = lane; j < n; j += kWave) {          // (a lane owns its column of the bins: no other lane writes it)
        int d = codes[j];
        d = d < p.D - 1 ? d : p.D - 1;
        bins[d * kBinCols + lane] += s_T[j];
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
  // ---- join of the rho groups: the last to arrive adds the partials in group order, then rho's parameter gradients ---------------------
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
  const gnan_bwd::Drop nodrop{0u, 1.f, 0ull};
  auto u_of = [&](int64_t d) { return d < p.D - 1 ? 1.0f / (static_cast<float>(d) + 1.0f) : 0.f; };
  auto gl_of = [&](int64_t d, int) { return s_dl[d]; };
  if (p.r_mid) gnan_bwd::feature_grads<1, true>(p.r, 0, 0, p.D, 0, nodrop, u_of, gl_of, red);
  else gnan_bwd::feature_grads<1, false>(p.r, 0, 0, p.D, 0, nodrop, u_of, gl_of, red);
}

template <int CN>
int launch_nam_feature_bwd(const MidNamBwdParams& p, hipStream_t st) {
  hipLaunchKernelGGL((mid_graph_nam_bwd_feature_kernel<CN>), dim3(static_cast<unsigned>(p.F)), dim3(kThreads), kNamADynBytes, st, p);
  return gnan::check_launch("mid_graph_nam_bwd_feature_kernel");
}

inline int rho_groups_of(int n) { return (n + kRhoRows - 1) / kRhoRows; }

// The cover of every entry point here, one refusal per violated limit, naming the limit and the value (shapes only; `f` NULL: a query
// about sizes and the read-out's channels alone)
int check_cover(const char* who, int n, int F, int D, int nam_C, const gnan_small_mlp* f, const gnan_small_mlp* rho,
                const gnan_small_mlp* nam) {
  GNAN_REQUIRE(n >= 1 && F >= 1 && D >= 1, "%s: bad sizes n=%d F=%d D=%d", who, n, F, D);
  if (n > kMidNodes) return gnan::fail(GNAN_ERR_UNSUPPORTED, "%s: covers n <= %d nodes (got n=%d)", who, kMidNodes, n);
  if (D < 2 || D > kMidD) return gnan::fail(GNAN_ERR_UNSUPPORTED, "%s: covers 2 <= D <= %d shells (got D=%d)", who, kMidD, D);
  if (nam_C < 1 || nam_C > kMaxC)
    return gnan::fail(GNAN_ERR_UNSUPPORTED, "%s: covers 1 <= C <= %d read-out channels (got nam.C=%d)", who, kMaxC, nam_C);
  if (f == nullptr) return GNAN_OK;
  const gnan_small_mlp* m[2] = {f, rho};
  const char* const name[2] = {"f", "rho"};
  for (int t = 0; t < 2; ++t) {
    if (m[t]->C != 1) return gnan::fail(GNAN_ERR_UNSUPPORTED, "%s: covers a one-wide %s (got %s.C=%d)", who, name[t], name[t], m[t]->C);
    if (m[t]->L != 2 && m[t]->L != 3)
      return gnan::fail(GNAN_ERR_UNSUPPORTED, "%s: covers L in {2, 3} (got %s.L=%d)", who, name[t], m[t]->L);
    if (m[t]->H < 1 || m[t]->H > kMaxH)
      return gnan::fail(GNAN_ERR_UNSUPPORTED, "%s: covers 1 <= H <= %d (got %s.H=%d)", who, kMaxH, name[t], m[t]->H);
  }
  if (nam->L < 1 || nam->L > 3) return gnan::fail(GNAN_ERR_UNSUPPORTED, "%s: covers L in {1, 2, 3} for the read-out (got nam.L=%d)", who, nam->L);
  if (nam->L != 1 && (nam->H < 1 || nam->H > kMaxH))
    return gnan::fail(GNAN_ERR_UNSUPPORTED, "%s: covers 1 <= H <= %d for the read-out (got nam.H=%d)", who, kMaxH, nam->H);
  return GNAN_OK;
}

// what both launching entry points ask of the graph's pointers and strides
template <class A>
int graph_ptrs_ok(const char* who, const A* a) {
  GNAN_REQUIRE(a->x != nullptr, "%s: null x", who);
  GNAN_REQUIRE(a->code != nullptr, "%s: null code", who);
  GNAN_REQUIRE(reinterpret_cast<uintptr_t>(a->code) % 4 == 0, "%s: code must be 4-byte aligned (got %p)", who,
               static_cast<const void*>(a->code));
  GNAN_REQUIRE(a->fx && a->lut && a->hidden, "%s: null fx / lut / hidden", who);
  GNAN_REQUIRE(a->colw != nullptr, "%s: null colw", who);
  GNAN_REQUIRE(mlp_ptrs_ok(&a->f) && mlp_ptrs_ok(&a->rho) && mlp_ptrs_ok(&a->nam), "%s: null weights", who);
  return strides_ok(who, a);
}

}  // namespace

extern "C" size_t gnan_mid_graph_nam_workspace_bytes(int32_t n, int32_t F, int32_t D, int32_t C) {
  (void)D;
  const size_t fwd = 16 + static_cast<size_t>(F) * C * sizeof(float);                        // counter (own 16 bytes) | part [F, C]
  const size_t bwd = 16 + static_cast<size_t>(rho_groups_of(n)) * kWave * sizeof(double)      // counter | dlut partials [groups][64]
                     + static_cast<size_t>(F) * sizeof(float);                               // | d hidden [F]
  return fwd > bwd ? fwd : bwd;
}

extern "C" int gnan_mid_graph_nam_describe(int32_t n, int32_t F, int32_t D, int32_t C, gnan_mid_graph_nam_info* out) {
  GNAN_REQUIRE(out != nullptr, "mid_graph_nam_describe: null out");
  if (int rc = check_cover("mid_graph_nam_describe", n, F, D, C, nullptr, nullptr, nullptr)) return rc;
  out->row_tiles = (n + kTile - 1) / kTile;
  out->rho_groups = rho_groups_of(n);
  out->fwd_grid = F;
  out->bwd_feature_grid = F;
  out->bwd_rho_grid = out->rho_groups;
  out->fwd_lds_bytes = static_cast<int32_t>(kNamFwdDynBytes + kNamFwdStaticBytes);
  const size_t a = kNamADynBytes + kNamAStaticBytes, b = kNamBDynBytes + kNamBStaticBytes;
  out->bwd_lds_bytes = static_cast<int32_t>(a > b ? a : b);
  out->fwd_workspace_bytes = static_cast<int64_t>(gnan_mid_graph_nam_workspace_bytes(n, F, D, C));
  out->bwd_workspace_bytes = out->fwd_workspace_bytes;      // (one size serves both directions)
  return GNAN_OK;
}

extern "C" int gnan_mid_graph_nam_fwd(const gnan_mid_graph_nam_args* a, gnan_stream_t stream) {
  GNAN_REQUIRE(a != nullptr, "mid_graph_nam: null args");
  if (int rc = check_cover("mid_graph_nam", a->n, a->F, a->D, a->nam.C, &a->f, &a->rho, &a->nam)) return rc;
  if (int rc = graph_ptrs_ok("mid_graph_nam", a)) return rc;
  GNAN_REQUIRE(a->out != nullptr, "mid_graph_nam: null out");
  if (int rc = workspace_ok("mid_graph_nam", a, gnan_mid_graph_nam_workspace_bytes(a->n, a->F, a->D, a->nam.C))) return rc;
  MidNamParams p;
  fwd_fields(p, a, a->n);
  p.nam = to_mlp(&a->nam);
  p.fx = a->fx; p.lut = a->lut; p.hidden = a->hidden; p.colw = a->colw; p.out = a->out;
  split_workspace(a->workspace, p.counter, p.part);
  if (int rc = raise_dyn_lds<&mid_graph_nam_kernel>(kNamFwdDynBytes, "mid_graph_nam")) return rc;
  hipLaunchKernelGGL(mid_graph_nam_kernel, dim3(static_cast<unsigned>(a->F)), dim3(kThreads), kNamFwdDynBytes,
                     static_cast<hipStream_t>(stream), p);
  return gnan::check_launch("mid_graph_nam_kernel");
}

extern "C" int gnan_mid_graph_nam_bwd(const gnan_mid_graph_nam_bwd_args* a, gnan_stream_t stream) {
  GNAN_REQUIRE(a != nullptr, "mid_graph_nam_bwd: null args");
  if (int rc = check_cover("mid_graph_nam_bwd", a->n, a->F, a->D, a->nam.C, &a->f, &a->rho, &a->nam)) return rc;
  if (int rc = graph_ptrs_ok("mid_graph_nam_bwd", a)) return rc;
  GNAN_REQUIRE(a->d_out != nullptr, "mid_graph_nam_bwd: null d_out");
  GNAN_REQUIRE(grads_ok(&a->f, &a->df) && grads_ok(&a->rho, &a->drho),
               "mid_graph_nam_bwd: a gradient pointer for every weight, and for a bias exactly where there is one");
  if (a->nam.L == 1)
    GNAN_REQUIRE(a->dnam.w_last && ((a->nam.b_last == nullptr) == (a->dnam.b_last == nullptr)),
                 "mid_graph_nam_bwd: gradient pointers of the one-layer read-out (its last layer's weight, and its bias exactly where there is one)");
  else
    GNAN_REQUIRE(grads_ok(&a->nam, &a->dnam),
                 "mid_graph_nam_bwd: a gradient pointer for every weight of the read-out, and for a bias exactly where there is one");
  if (int rc = workspace_ok("mid_graph_nam_bwd", a, gnan_mid_graph_nam_workspace_bytes(a->n, a->F, a->D, a->nam.C))) return rc;
  GNAN_REQUIRE(reinterpret_cast<uintptr_t>(a->workspace) % 8 == 0, "mid_graph_nam_bwd: workspace must be 8-byte aligned (got %p)", a->workspace);
  MidNamBwdParams p;
  bwd_fields(p, a, a->n, &a->df, &a->drho);
  p.nam = to_weights(&a->nam, &a->dnam); p.nam_L = a->nam.L;
  p.fx = a->fx; p.lut = a->lut; p.hidden = a->hidden; p.colw = a->colw; p.d_out = a->d_out;
  p.rho_groups = rho_groups_of(a->n);
  split_workspace(a->workspace, p.counter, p.part);
  p.dh = reinterpret_cast<float*>(p.part + static_cast<size_t>(p.rho_groups) * kWave);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (int rc = raise_dyn_lds<&mid_graph_nam_bwd_rho_kernel>(kNamBDynBytes, "mid_graph_nam_bwd")) return rc;
  if (int rc = with_channels(a->nam.C, [&](auto c) { return launch_nam_feature_bwd<decltype(c)::value>(p, st); })) return rc;
  hipLaunchKernelGGL(mid_graph_nam_bwd_rho_kernel, dim3(static_cast<unsigned>(p.rho_groups)), dim3(kThreads), kNamBDynBytes, st, p);
  return gnan::check_launch("mid_graph_nam_bwd_rho_kernel");
}
