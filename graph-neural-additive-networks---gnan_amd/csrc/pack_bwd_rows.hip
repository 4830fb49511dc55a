// The packing pass in front of gnan_spmm_bwd_narrow (gfx950): V[d * n + i, :] = [ dY_i / cnt(i, d) | dY_i / cnt(i, D-1) ],
// the packed operand of the narrow backward (csrc/spmm_grad.hip), and the one-channel rest-bucket sum q_sum.
// See include/gnan_hip.h for the contract.
#include "common.hpp"

namespace {
// partial[blockIdx.x] = the sum of `v` over the 256 threads of the workgroup (fixed tree, float64) — EVERY thread calls it.
// (the tree of gnan::sum_partials_256, csrc/common.hpp, over one value per thread and on an LDS array of its own: the two meet in
// block_sum_finish's last workgroup, and one array would need a barrier between them)
__device__ __forceinline__ void block_sum_to(double v, double* __restrict__ partial) {
  __shared__ double red[256];
  red[threadIdx.x] = v;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if (static_cast<int>(threadIdx.x) < st) red[threadIdx.x] += red[threadIdx.x + st];
    __syncthreads();
  }
  if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}

// ... and, with an arrival counter, the last workgroup of the pass adds the partials (pack_q_final_kernel's sum, same order)
__device__ __forceinline__ void block_sum_finish(double v, double* partial, unsigned* arrive, float* out) {
  block_sum_to(v, partial);
  if (arrive != nullptr && gnan::last_block(arrive)) {
    const double s_all = gnan::sum_partials_256(partial, static_cast<int64_t>(gridDim.x));
    if (threadIdx.x == 0) out[0] = static_cast<float>(s_all);
  }
}

// q_sum[0] = sum of the workgroups' partials (one workgroup, fixed order): sum_i dY_i / cnt(i, rest), what gnan_colsum over the
// packed rows' second halves returned — two launches and a strided 40-MB read on the 10M-node graph
__global__ __launch_bounds__(256) void pack_q_final_kernel(const double* __restrict__ partial, int64_t n_partial, float* __restrict__ q_sum) {
  const double s_all = gnan::sum_partials_256(partial, n_partial);   // (the order block_sum_finish's last workgroup adds them in)
  if (threadIdx.x == 0) q_sum[0] = static_cast<float>(s_all);
}

// V[d * n + i, :] = [ dY_i / cnt(i, d) | dY_i / cnt(i, D-1) ]  (the packed operand of gnan_spmm_bwd_narrow), zero padded.
// Thread = node: its gradient row and counts are read once, its D packed rows are one contiguous run of the output.
__global__ __launch_bounds__(256) void pack_bwd_rows_kernel(const float* __restrict__ dY, int64_t dy_stride, int W,
                                                            const int32_t* __restrict__ cnt, int64_t cnt_stride, int D,
                                                            int64_t n, int with_rest, float* __restrict__ V, int half,
                                                            const int64_t* __restrict__ hot, int64_t n_hot, int64_t o_begin,
                                                            double* q_partial, unsigned* q_arrive, float* q_sum) {
  double qs = 0.0;                                    // q_partial (W == 1): this thread's sum of dY_i / cnt(i, rest) over REAL nodes
  for (int64_t o = o_begin + static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; o < n + n_hot; o += static_cast<int64_t>(gridDim.x) * 256) {
    const int64_t i = o < n ? o : hot[o - n];         // packed rows [n, n + n_hot): second copies of the nodes hot[]
    float r_rest = 1.f;
    if (cnt) {
      const int k = cnt[i * cnt_stride + D - 1];
      r_rest = static_cast<float>(k > 1 ? k : 1);
    }
    // code-major: V[d * (n + n_hot) + o, :] — the rows of ONE hop code are contiguous, so the lines a pass over the code-1
    // pairs fetches hold sixteen useful rows each (node-major (o, d) rows: a third of every line was the never-gathered
    // rest code and the once-per-node self code) and the hot block of a code is 2 MB instead of 6
    for (int d = 0; d < D; ++d) {
      float* out = V + (static_cast<int64_t>(d) * (n + n_hot) + o) * 2 * half;
      float r = 1.f;
      if (cnt) {
        const int k = cnt[i * cnt_stride + d];
        r = static_cast<float>(k > 1 ? k : 1);
      }
      for (int w = 0; w < half; ++w) {
        const float g = w < W ? dY[i * dy_stride + w] : 0.f;
        out[w] = g / r;
        out[half + w] = with_rest ? g / r_rest : 0.f;
      }
    }
    if (q_partial && with_rest && o < n) qs += static_cast<double>(dY[i * dy_stride] / r_rest);
  }
  if (q_partial) block_sum_finish(qs, q_partial, q_arrive, q_sum);
}

// One-channel gradients (half == 1: packed rows of two floats) with shell counts and at most four codes — the shape of every
// sum-first training step: thread = TWO consecutive nodes, so that a node pair's counts are three 8-byte loads, its gradients
// one, and its packed rows of a code ONE 16-byte store (the one-node form above moves the 10M-node graph's 400 MB at 2.9 TB/s:
// 4- and 8-byte accesses).  Covers the nodes [0, n_pairs * 2); the tail and the hot copies go through the kernel above.
template <int D>
__global__ __launch_bounds__(256) void pack_bwd_pairs_kernel(const float* __restrict__ dY, const int32_t* __restrict__ cnt,
                                                             int64_t n, int64_t n_pairs, int with_rest, float* __restrict__ V,
                                                             const int64_t* __restrict__ hot, int64_t n_hot, int pair_blocks,
                                                             double* q_partial, unsigned* q_arrive, float* q_sum) {
  const int64_t rows_per_code = n + n_hot;
  double qs = 0.0;
  if (static_cast<int>(blockIdx.x) >= pair_blocks) {
    // the odd last node and the second copies of the nodes hot[] — in the SAME launch, next to the streaming part (a launch of
    // their own: 35 us behind the pairs' 61 on the 10M-node graph)
    const int64_t o = 2 * n_pairs + (static_cast<int64_t>(blockIdx.x) - pair_blocks) * 256 + threadIdx.x;
    if (o < rows_per_code) {
      const int64_t i = o < n ? o : hot[o - n];
      const float g = dY[i];
      int k[D];
#pragma unroll
      for (int d = 0; d < D; ++d) k[d] = cnt[i * D + d];
      const float q = with_rest ? g / static_cast<float>(k[D - 1] > 1 ? k[D - 1] : 1) : 0.f;
#pragma unroll
      for (int d = 0; d < D; ++d)
        *reinterpret_cast<float2*>(V + (static_cast<int64_t>(d) * rows_per_code + o) * 2) =
            make_float2(g / static_cast<float>(k[d] > 1 ? k[d] : 1), q);
      if (o < n) qs = static_cast<double>(q);
    }
    if (q_partial) block_sum_finish(qs, q_partial, q_arrive, q_sum);
    return;
  }
  for (int64_t t = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; t < n_pairs; t += static_cast<int64_t>(pair_blocks) * 256) {
    const float2 g = *reinterpret_cast<const float2*>(dY + 2 * t);
    int k[2 * D];                                         // (the pair's 2 D counts start 8-byte aligned whatever D is)
#pragma unroll
    for (int u = 0; u < D; ++u) {
      const int2 c = *reinterpret_cast<const int2*>(cnt + 2 * D * t + 2 * u);
      k[2 * u] = c.x; k[2 * u + 1] = c.y;
    }
    float r[2][D];
#pragma unroll
    for (int d = 0; d < D; ++d) {
      r[0][d] = static_cast<float>(k[d] > 1 ? k[d] : 1);
      r[1][d] = static_cast<float>(k[D + d] > 1 ? k[D + d] : 1);
    }
    const float q0 = with_rest ? g.x / r[0][D - 1] : 0.f, q1 = with_rest ? g.y / r[1][D - 1] : 0.f;
#pragma unroll
    for (int d = 0; d < D; ++d)
      *reinterpret_cast<float4*>(V + (static_cast<int64_t>(d) * rows_per_code + 2 * t) * 2) = make_float4(g.x / r[0][d], q0, g.y / r[1][d], q1);
    qs += static_cast<double>(q0) + static_cast<double>(q1);
  }
  if (q_partial) block_sum_finish(qs, q_partial, q_arrive, q_sum);
}
}  // namespace

// the launch gnan_spmm_pack_bwd_rows makes for these arguments: node pairs (pair_blocks > 0) or one node per thread
namespace {
struct PackGrid {
  bool pairs;
  int64_t n_pairs, pair_blocks, blocks;    // blocks: the whole grid
};
PackGrid pack_grid(const gnan_pack_bwd_rows_args* a) {
  PackGrid g{false, 0, 0, 0};
  const int64_t n = a->n, n_hot = a->n_hot;
  // node pairs (large graphs): needs the packed rows of every code to start 16-byte aligned ((n + n_hot) even) and dense inputs
  if (a->half == 1 && a->W == 1 && a->cnt != nullptr && a->cnt_stride == a->D && a->dy_stride == 1 && a->D >= 2 && a->D <= 4 &&
      n >= (int64_t(1) << 20) && (n + n_hot) % 2 == 0 && reinterpret_cast<uintptr_t>(a->dY) % 8 == 0 &&
      reinterpret_cast<uintptr_t>(a->cnt) % 8 == 0 && reinterpret_cast<uintptr_t>(a->V) % 16 == 0) {
    g.n_pairs = n / 2;
    g.pair_blocks = (g.n_pairs + 255) / 256;
    g.pair_blocks = g.pair_blocks > 65536 ? 65536 : g.pair_blocks;
    const int64_t tb = (n + n_hot - 2 * g.n_pairs + 255) / 256;
    if (tb < (int64_t(1) << 20)) {
      g.pairs = true;
      g.blocks = g.pair_blocks + tb;
      return g;
    }
  }
  g.blocks = (n + n_hot + 255) / 256;
  g.blocks = g.blocks > 65536 ? 65536 : g.blocks;
  return g;
}
}  // namespace

extern "C" size_t gnan_spmm_pack_bwd_rows_workspace_bytes(const gnan_pack_bwd_rows_args* a) {
  if (!a || a->q_sum == nullptr || a->n <= 0) return 0;
  return static_cast<size_t>(pack_grid(a).blocks) * sizeof(double);
}

extern "C" int gnan_spmm_pack_bwd_rows(const gnan_pack_bwd_rows_args* a, gnan_stream_t stream) {
  GNAN_REQUIRE(a != nullptr, "pack_bwd_rows: null args");
  const float* dY = a->dY;
  const int64_t dy_stride = a->dy_stride, cnt_stride = a->cnt_stride, n = a->n, n_hot = a->n_hot;
  const int32_t W = a->W, D = a->D, with_rest = a->with_rest, half = a->half;
  const int32_t* cnt = a->cnt;
  float* V = a->V;
  const int64_t* hot = a->hot;
  GNAN_REQUIRE(n >= 0 && W >= 1 && D >= 1 && half >= W && (half & (half - 1)) == 0, "pack_bwd_rows: bad sizes");
  GNAN_REQUIRE((dY && V) || n == 0, "pack_bwd_rows: null pointer");
  GNAN_REQUIRE(dy_stride >= W && (cnt == nullptr || cnt_stride >= D), "pack_bwd_rows: row stride smaller than the width");
  GNAN_REQUIRE(n_hot >= 0 && (n_hot == 0 || hot != nullptr), "pack_bwd_rows: n_hot without hot");
  GNAN_REQUIRE(a->q_sum == nullptr || (W == 1 && with_rest), "pack_bwd_rows: q_sum is the one-channel rest-bucket sum (W == 1, with_rest)");
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (n == 0) {
    if (a->q_sum) {
      hipLaunchKernelGGL(pack_q_final_kernel, dim3(1), dim3(256), 0, st, static_cast<const double*>(nullptr), static_cast<int64_t>(0), a->q_sum);
      return gnan::check_launch("pack_q_final_kernel");
    }
    return GNAN_OK;
  }
  const PackGrid pg = pack_grid(a);
  double* q_partial = nullptr;
  if (a->q_sum) {
    const size_t need = static_cast<size_t>(pg.blocks) * sizeof(double);
    if (a->q_workspace == nullptr || a->q_workspace_bytes < need)
      return gnan::fail(GNAN_ERR_WORKSPACE, "pack_bwd_rows: q workspace %zu B < required %zu B", a->q_workspace_bytes, need);
    GNAN_REQUIRE(reinterpret_cast<uintptr_t>(a->q_workspace) % 8 == 0, "pack_bwd_rows: q workspace must be 8-byte aligned");
    q_partial = static_cast<double*>(a->q_workspace);
  }
  // q_sum by the last workgroup of the packing launch where the caller lends an arrival counter (a fence per workgroup: small grids)
  unsigned* q_arrive = (q_partial && pg.blocks <= gnan::kMaxArriveBlocks) ? reinterpret_cast<unsigned*>(a->q_arrive) : nullptr;
  if (pg.pairs) {
    const dim3 grid(static_cast<unsigned>(pg.blocks)), block(256);
    const int pbi = static_cast<int>(pg.pair_blocks);
    if (D == 2) hipLaunchKernelGGL(pack_bwd_pairs_kernel<2>, grid, block, 0, st, dY, cnt, n, pg.n_pairs, with_rest, V, hot, n_hot, pbi, q_partial, q_arrive, a->q_sum);
    else if (D == 3) hipLaunchKernelGGL(pack_bwd_pairs_kernel<3>, grid, block, 0, st, dY, cnt, n, pg.n_pairs, with_rest, V, hot, n_hot, pbi, q_partial, q_arrive, a->q_sum);
    else hipLaunchKernelGGL(pack_bwd_pairs_kernel<4>, grid, block, 0, st, dY, cnt, n, pg.n_pairs, with_rest, V, hot, n_hot, pbi, q_partial, q_arrive, a->q_sum);
    if (int rc = gnan::check_launch("pack_bwd_pairs_kernel")) return rc;
  } else {
    hipLaunchKernelGGL(pack_bwd_rows_kernel, dim3(static_cast<unsigned>(pg.blocks)), dim3(256), 0, st,
                       dY, dy_stride, W, cnt, cnt_stride, D, n, with_rest, V, half, hot, n_hot, static_cast<int64_t>(0), q_partial,
                       q_arrive, a->q_sum);
    if (int rc = gnan::check_launch("pack_bwd_rows_kernel")) return rc;
  }
  if (q_partial && q_arrive == nullptr) {
    hipLaunchKernelGGL(pack_q_final_kernel, dim3(1), dim3(256), 0, st, q_partial, pg.blocks, a->q_sum);
    return gnan::check_launch("pack_q_final_kernel");
  }
  return GNAN_OK;
}
