// Attributions of a BATCH of small graphs by source node and by graph (include/gnan_hip.h has the definition):
//   V[j, d, c] = sum over the nodes i of j's graph with min(code_g[i, j], D-1) == d of wt(i, d, c)
//   B[j, d, w] = V[j, d, w % Cw] * S[j, w]          T[g, d, w] = sum over the nodes j of graph g, in node order, of B[j, d, w]
// The graphs are HopBlocks: packed [n_g, n_g] uint8 code blocks (row i = forward row, column j = source) with node_off / code_off.
// V does not depend on the operand column, so a block is walked ONCE, column-side.  Up to three launches whatever the number of
// graphs, no floating-point atomic, no arrival counter, no workgroup waits for another:
//
//   blocks_walk_kernel   one WORKGROUP per tile = 64 consecutive columns of one graph (workgroup g * col_tiles + t; a tile past the
//                        graph's last column leaves at once).  Lane l owns column j0 + l: a row's 64 codes are one coalesced read.
//                        The four waves take the rows i = wave, wave + 4, ... (four row slices), each lane adds into its OWN words
//                        of LDS, acc[wave][bin of the pass][lane]: bank = lane, plain read / add / write, no LDS atomic.  Bins are
//                        (shell, weight channel) = d * Cw + c, taken in passes of 64.  The weights of a row chunk (kRows rows x the
//                        pass's bins: the lut word, divided by max(cnt, 1) where counts are given) are the same for all 64
//                        columns: the workgroup stages them in LDS once per row chunk — one division per (row, bin), not per
//                        pair; a shared lut without counts is staged once per pass.  A pass ends with the four slices added in
//                        the fixed tree (s0 + s1) + (s2 + s3) and V[j, bin] stored to the workspace.
//   blocks_scale_kernel  B = V * S, a thread per (node, column) of one shell (grid.y = shell): coalesced read of S, coalesced
//                        write of B.  Only where B is asked for.
//   blocks_graph_kernel  T: a thread per (graph, shell, column) adds V * S over the graph's nodes in node order (an empty graph: 0).
//                        It reads V and S, never B, so T has the same bits with or without B.
//
// The bits of graph g's rows of B and of T[g] depend on g's own codes, weights and operand rows only: tiles, row slices and the
// node sum are laid out from the graph's own first node, whatever else the batch holds.
#include "common.hpp"

namespace {

constexpr int kThreads = 256, kWaves = 4, kLanes = 64, kPassBins = 64;
constexpr int kRows = 64;                    // rows per staged chunk of weights: sixteen per wave
constexpr int kFlight = 4;                   // code bytes a lane has in flight
constexpr int kScaleElems = 1024;            // (node, column) products per workgroup of the B epilogue

struct Params {
  const uint8_t* code;
  const int32_t* node_off;
  const int64_t* code_off;
  int64_t n_graphs, total_nodes;
  int col_tiles;               // tiles of 64 columns of the widest graph
  const float* S;
  int W;
  int64_t s_stride;
  const float* lut;
  int64_t lut_row_stride;
  int D, Cw;
  const int32_t* cnt;
  int64_t cnt_stride;
  float* B;
  int64_t b_stride;
  float* T;
  int64_t bins;                // D * Cw
  int cap;                     // bins of a pass held in LDS: min(bins, 64)
  int row_dep;                 // the weights differ from row to row (a per-row lut or counts)
  int npb;                     // nodes per workgroup of the B epilogue
  float* V;                    // [total_nodes, bins]
};

__global__ __launch_bounds__(kThreads) void blocks_walk_kernel(const Params p) {
  extern __shared__ float lds[];                     // acc [kWaves][cap][64] | wts [row_dep ? kRows : 1][cap]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t g = blockIdx.x / p.col_tiles;
  const int j0 = static_cast<int>(blockIdx.x - g * p.col_tiles) * kLanes;
  const int64_t n0 = p.node_off[g];
  const int n = static_cast<int>(p.node_off[g + 1] - n0);
  if (j0 >= n || n0 + n > p.total_nodes) return;     // the whole workgroup, before any barrier
  const uint8_t* code = p.code + p.code_off[g];
  const int j = j0 + lane;
  const bool live = j < n;
  float* acc = lds;
  float* wts = lds + kWaves * p.cap * kLanes;
  float* mine = acc + wave * p.cap * kLanes + lane;  // + bin * 64: this lane's word of a bin, in this wave's slice
  const int rest = p.D - 1;

  for (int64_t b0 = 0; b0 < p.bins; b0 += kPassBins) {
    const int nb = p.bins - b0 < kPassBins ? static_cast<int>(p.bins - b0) : kPassBins;
    for (int s = 0; s < nb; ++s) mine[s * kLanes] = 0.f;
    for (int r0 = 0; r0 < n; r0 += kRows) {
      const int nr = n - r0 < kRows ? n - r0 : kRows;
      __syncthreads();                               // the last chunk's readers are done with wts
      if (r0 == 0 || p.row_dep) {
        const int ne = (p.row_dep ? nr : 1) * nb;
        for (int e = threadIdx.x; e < ne; e += kThreads) {
          const int r = e / nb, s = e - r * nb;
          const int64_t bin = b0 + s;
          const int64_t i = n0 + r0 + r;
          float w = p.lut[i * p.lut_row_stride + bin];
          if (p.cnt) {
            const int c = p.cnt[i * p.cnt_stride + bin / p.Cw];
            w = w / static_cast<float>(c > 1 ? c : 1);
          }
          wts[r * p.cap + s] = w;
        }
      }
      __syncthreads();
      if (!live) continue;
      for (int r = wave; r < nr; r += kWaves * kFlight) {
        int cd[kFlight];
#pragma unroll
        for (int u = 0; u < kFlight; ++u) {
          const int ru = r + u * kWaves;
          cd[u] = ru < nr ? code[static_cast<int64_t>(r0 + ru) * n + j] : 0;
        }
#pragma unroll
        for (int u = 0; u < kFlight; ++u) {
          const int ru = r + u * kWaves;
          if (ru >= nr) break;
          const int d = cd[u] < rest ? cd[u] : rest;                       // 255 and listed codes past the cover: the rest shell
          const int64_t base = static_cast<int64_t>(d) * p.Cw - b0;        // bin of channel 0, relative to the pass
          const int c_lo = base < 0 ? static_cast<int>(-base) : 0;
          const int64_t c_end = static_cast<int64_t>(nb) - base;
          const int c_hi = c_end < p.Cw ? static_cast<int>(c_end) : p.Cw;
          const float* wrow = wts + (p.row_dep ? ru * p.cap : 0);
          for (int c = c_lo; c < c_hi; ++c) mine[(base + c) * kLanes] += wrow[base + c];
        }
      }
    }
    __syncthreads();
    // the four row slices in a fixed tree; thread -> (bin, lane): LDS reads without a conflict
    for (int e = threadIdx.x; e < nb * kLanes; e += kThreads) {
      const int s = e >> 6, l = e & 63;
      if (j0 + l >= n) continue;
      const float* a = acc + s * kLanes + l;
      const int64_t step = static_cast<int64_t>(p.cap) * kLanes;
      p.V[(n0 + j0 + l) * p.bins + b0 + s] = (a[0] + a[step]) + (a[2 * step] + a[3 * step]);
    }
    __syncthreads();                                 // before the next pass clears acc
  }
}

__global__ __launch_bounds__(kThreads) void blocks_scale_kernel(const Params p) {
  const int d = blockIdx.y;
  const int64_t q0 = static_cast<int64_t>(blockIdx.x) * p.npb;
  const int64_t left = p.total_nodes - q0;
  const int np = left < p.npb ? static_cast<int>(left) : p.npb;
  const int n = np * p.W;                            // npb * W <= max(kScaleElems, W)
  for (int le = threadIdx.x; le < n; le += kThreads) {
    const int pl = le / p.W, w = le - pl * p.W;
    const int64_t q = q0 + pl;
    p.B[q * p.b_stride + static_cast<int64_t>(d) * p.W + w] =
        p.V[q * p.bins + static_cast<int64_t>(d) * p.Cw + (w % p.Cw)] * p.S[q * p.s_stride + w];
  }
}

__global__ __launch_bounds__(kThreads) void blocks_graph_kernel(const Params p) {
  const int64_t dw = static_cast<int64_t>(p.D) * p.W;
  const int64_t e = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (e >= p.n_graphs * dw) return;
  const int64_t g = e / dw;
  const int64_t r = e - g * dw;
  const int d = static_cast<int>(r / p.W), w = static_cast<int>(r - static_cast<int64_t>(d) * p.W);
  int64_t q = p.node_off[g], q1 = p.node_off[g + 1];
  if (q1 > p.total_nodes) q1 = p.total_nodes;
  const float* v = p.V + static_cast<int64_t>(d) * p.Cw + (w % p.Cw);
  float t = 0.f;
  for (; q < q1; ++q) t += v[q * p.bins] * p.S[q * p.s_stride + w];          // node order
  p.T[e] = t;
}

int64_t bins_of(const gnan_attr_blocks_args* a) { return static_cast<int64_t>(a->D) * a->Cw; }

int cap_of(const gnan_attr_blocks_args* a) { return static_cast<int>(bins_of(a) < kPassBins ? bins_of(a) : kPassBins); }

int row_dep_of(const gnan_attr_blocks_args* a) { return a->lut_row_stride != 0 || a->cnt != nullptr; }

int64_t col_tiles_of(const gnan_attr_blocks_args* a) { return (static_cast<int64_t>(a->max_nodes) + kLanes - 1) / kLanes; }

int lds_bytes(const gnan_attr_blocks_args* a) {
  return (kWaves * kLanes + (row_dep_of(a) ? kRows : 1)) * cap_of(a) * static_cast<int>(sizeof(float));
}

// every refusal, on the host, before any HIP call
int validate(const gnan_attr_blocks_args* a, const char* who, bool launch) {
  GNAN_REQUIRE(a != nullptr, "%s: null args", who);
  GNAN_REQUIRE(a->n_graphs >= 0 && a->total_nodes >= 0 && a->max_nodes >= 0, "%s: negative size (n_graphs=%lld, total_nodes=%lld, max_nodes=%lld)",
               who, static_cast<long long>(a->n_graphs), static_cast<long long>(a->total_nodes), static_cast<long long>(a->max_nodes));
  GNAN_REQUIRE(a->max_nodes <= a->total_nodes, "%s: max_nodes=%lld above total_nodes=%lld", who, static_cast<long long>(a->max_nodes),
               static_cast<long long>(a->total_nodes));
  GNAN_REQUIRE(a->total_nodes == 0 || a->max_nodes >= 1, "%s: max_nodes=0 beside total_nodes=%lld", who, static_cast<long long>(a->total_nodes));
  GNAN_REQUIRE(a->W >= 1, "%s: W must be >= 1 (got %d)", who, a->W);
  if (a->D < 2 || a->D > GNAN_MAX_CODES)
    return gnan::fail(GNAN_ERR_UNSUPPORTED, "%s: covers 2 <= D <= %d hop codes (got D=%d)", who, GNAN_MAX_CODES, a->D);
  GNAN_REQUIRE(a->Cw >= 1 && a->W % a->Cw == 0, "%s: Cw must divide W (got Cw=%d, W=%d)", who, a->Cw, a->W);
  GNAN_REQUIRE(a->lut_row_stride == 0 || a->lut_row_stride >= bins_of(a), "%s: lut_row_stride must be 0 (one table) or at least D * Cw", who);
  GNAN_REQUIRE(a->s_stride >= a->W, "%s: operand row stride smaller than W", who);
  GNAN_REQUIRE(a->B == nullptr || a->b_stride >= static_cast<int64_t>(a->D) * a->W, "%s: output row stride smaller than D * W", who);
  GNAN_REQUIRE(a->cnt == nullptr || a->cnt_stride >= a->D, "%s: cnt row stride smaller than D", who);
  if (a->n_graphs > 0x7fffffffLL)
    return gnan::fail(GNAN_ERR_UNSUPPORTED, "%s: %lld graphs exceed an int32 (limit %lld): pass the graphs in batches", who,
                      static_cast<long long>(a->n_graphs), 0x7fffffffLL);
  if (a->n_graphs * col_tiles_of(a) > 0x7fffffffLL)
    return gnan::fail(GNAN_ERR_UNSUPPORTED, "%s: %lld graphs x %lld column tiles exceed one launch (limit %lld): pass the graphs in batches", who,
                      static_cast<long long>(a->n_graphs), static_cast<long long>(col_tiles_of(a)), 0x7fffffffLL);
  if (a->n_graphs * a->D * a->W > 0x7fffffffLL * kThreads)
    return gnan::fail(GNAN_ERR_UNSUPPORTED, "%s: %lld (graph, shell, column) sums exceed one launch (limit %lld): pass the graphs in batches", who,
                      static_cast<long long>(a->n_graphs * a->D * a->W), 0x7fffffffLL * kThreads);
  if (!launch) return GNAN_OK;
  GNAN_REQUIRE(a->B != nullptr || a->T != nullptr, "%s: both outputs are NULL (B and T)", who);
  GNAN_REQUIRE(a->n_graphs == 0 || (a->node_off && a->code_off), "%s: null node_off / code_off", who);
  GNAN_REQUIRE(a->total_nodes == 0 || (a->code && a->S && a->lut), "%s: null code / S / lut", who);
  const size_t need = gnan_attr_blocks_workspace_bytes(a);
  if (need && (a->workspace == nullptr || a->workspace_bytes < need))
    return gnan::fail(GNAN_ERR_WORKSPACE, "%s: workspace %zu B < required %zu B", who, a->workspace ? a->workspace_bytes : size_t{0}, need);
  GNAN_REQUIRE(need == 0 || reinterpret_cast<uintptr_t>(a->workspace) % 4 == 0, "%s: workspace must be 4-byte aligned", who);
  return GNAN_OK;
}

int launches_of(const gnan_attr_blocks_args* a) {
  if (a->n_graphs == 0) return 0;
  int n = 0;
  if (a->total_nodes > 0) n += 1 + (a->B != nullptr);                        // walk, scale
  if (a->T != nullptr) n += 1;                                               // node sum
  return n;
}

}  // namespace

extern "C" size_t gnan_attr_blocks_workspace_bytes(const gnan_attr_blocks_args* a) {
  if (a == nullptr || a->total_nodes <= 0 || a->D < 1 || a->Cw < 1) return 0;
  return static_cast<size_t>(a->total_nodes) * static_cast<size_t>(bins_of(a)) * sizeof(float);
}

extern "C" int gnan_attr_blocks_describe(const gnan_attr_blocks_args* a, gnan_attr_blocks_info* out) {
  GNAN_REQUIRE(out != nullptr, "attr_blocks_describe: null info");
  if (int rc = validate(a, "attr_blocks_describe", false)) return rc;
  out->tile_cols = kLanes;
  out->col_tiles = static_cast<int32_t>(col_tiles_of(a));
  out->bin_passes = static_cast<int32_t>((bins_of(a) + kPassBins - 1) / kPassBins);
  out->row_chunk = kRows;
  out->row_slices = kWaves;
  out->block_size = kThreads;
  out->launches = launches_of(a);
  out->lds_bytes = lds_bytes(a);
  out->n_tiles = a->n_graphs * col_tiles_of(a);
  out->v_bytes = gnan_attr_blocks_workspace_bytes(a);
  out->workspace_bytes = out->v_bytes;
  return GNAN_OK;
}

extern "C" int gnan_attr_blocks(const gnan_attr_blocks_args* a, gnan_stream_t stream) {
  if (int rc = validate(a, "attr_blocks", true)) return rc;
  if (a->n_graphs == 0) return GNAN_OK;
  Params p;
  p.code = a->code; p.node_off = a->node_off; p.code_off = a->code_off;
  p.n_graphs = a->n_graphs; p.total_nodes = a->total_nodes; p.col_tiles = static_cast<int>(col_tiles_of(a));
  p.S = a->S; p.W = a->W; p.s_stride = a->s_stride;
  p.lut = a->lut; p.lut_row_stride = a->lut_row_stride; p.D = a->D; p.Cw = a->Cw;
  p.cnt = a->cnt; p.cnt_stride = a->cnt_stride;
  p.B = a->B; p.b_stride = a->b_stride; p.T = a->T;
  p.bins = bins_of(a); p.cap = cap_of(a); p.row_dep = row_dep_of(a);
  p.npb = a->W >= kScaleElems ? 1 : kScaleElems / a->W;
  p.V = static_cast<float*>(a->workspace);
  hipStream_t st = static_cast<hipStream_t>(stream);
  auto blocks = [](int64_t n, int64_t per) { return static_cast<unsigned>((n + per - 1) / per); };
  if (p.total_nodes > 0) {
    const int lds = lds_bytes(a);
    if (lds > 64 * 1024) {
      hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(blocks_walk_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
      if (e != hipSuccess) return gnan::fail(GNAN_ERR_HIP, "attr_blocks: hipFuncSetAttribute: %s", hipGetErrorString(e));
    }
    hipLaunchKernelGGL(blocks_walk_kernel, dim3(static_cast<unsigned>(p.n_graphs * p.col_tiles)), dim3(kThreads), lds, st, p);
    if (int rc = gnan::check_launch("blocks_walk_kernel")) return rc;
    if (p.B) {
      hipLaunchKernelGGL(blocks_scale_kernel, dim3(blocks(p.total_nodes, p.npb), static_cast<unsigned>(p.D)), dim3(kThreads), 0, st, p);
      if (int rc = gnan::check_launch("blocks_scale_kernel")) return rc;
    }
  }
  if (p.T) {
    hipLaunchKernelGGL(blocks_graph_kernel, dim3(blocks(p.n_graphs * p.D * p.W, kThreads)), dim3(kThreads), 0, st, p);
    if (int rc = gnan::check_launch("blocks_graph_kernel")) return rc;
  }
  return GNAN_OK;
}
