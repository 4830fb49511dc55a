// The lone rows of the wide forward's self_sum route (gnan_spmm_args.lone_rows): the rows of the degree-sorted twin that list no pair
// — run L = 0 of the short-row runs, 62 % of the rows of a power-law graph once the self pair has left the adjacency.  Such a row's output is
//   Y[o] = fmaf(w_0 - w_rest, a_o, sum_c w_rest s_total[c])
// and nothing else.  short_tile<VEC, LPR, 0, true> (csrc/spmm_fwd_body.hpp) spends a lane group's serial row bodies, their shuffles and
// two awaited loads per row on it; here a THREAD takes a row: no shuffle, s_total staged once per workgroup, the row ids of a
// workgroup consecutive (the sort is stable, so run 0 lists its rows by ascending id: the reads of self_sum and the stores are near
// coalesced).  Same bits as the tile: the weights are derived as small_weights / short_tile derive them, and the rest sum repeats the tile's
// operations in the tile's order — per column fmaf(w_rest, s_total[c], 0.f); per lane of the tile's layout its four columns added in
// order onto 0.f, lanes at or beyond W contributing 0.f; the lane sums met by the balanced tree that the butterfly over offsets
// 1, 2, 4, ... LPR / 2 builds (float addition commutes, so which lane holds the left operand does not matter).
#include "spmm_common.hpp"

namespace {

constexpr int kLoneBlock = 256;   // rows (threads) per workgroup

// The tree over lanes [l0, l0 + N) of the tile's layout, N a power of two: lane l holds columns 4 l .. 4 l + 3 of the staged total.
template <int N>
__device__ __forceinline__ float lone_tree(const float* tot, const float w_rest, const int W, const int l0) {
  if constexpr (N == 1) {
    const float4 t = *reinterpret_cast<const float4*>(tot + 4 * l0);
    float y = 0.f;
    y += fmaf(w_rest, t.x, 0.f);
    y += fmaf(w_rest, t.y, 0.f);
    y += fmaf(w_rest, t.z, 0.f);
    y += fmaf(w_rest, t.w, 0.f);
    return 4 * l0 < W ? y : 0.f;     // (validate() / pick_tiling: W % 4 == 0 — a lane is inside or outside as a whole)
  } else {
    const float lo = lone_tree<N / 2>(tot, w_rest, W, l0);
    const float hi = lone_tree<N / 2>(tot, w_rest, W, l0 + N / 2);
    return lo + hi;
  }
}

template <int LPR>
__global__ __launch_bounds__(kLoneBlock) void spmm_lone_kernel(const Params p) {
  __shared__ __attribute__((aligned(16))) float tot[LPR * 4];
  for (int c = threadIdx.x; c < LPR * 4; c += kLoneBlock) tot[c] = (p.s_total != nullptr && c < p.W) ? p.s_total[c] : 0.f;
  __syncthreads();
  const int64_t q = p.short_row[0] + static_cast<int64_t>(blockIdx.x) * kLoneBlock + threadIdx.x;
  if (q >= p.short_row[0] + p.lone_n) return;
  const int64_t o = p.row_ids[q];
  const int rest = p.D - 1;
  const SmallW sw = small_weights(p, q);     // (scatter_out 2: slot q reads adjacency row q)
  float w_rest = 0.f, w_self = sw.w[0];
  float y = 0.f;
  if (p.s_total) {                           // the fold of rows_body / short_tile: w_0 - w_rest, and no self weight where code 0 IS the rest
    w_rest = sw.pick(rest);
    w_self = rest > 0 ? sw.w[0] - w_rest : 0.f;
    y = lone_tree<LPR>(tot, w_rest, p.W, 0);
  }
  p.Y[o * p.y_stride] = fmaf(w_self, self_term(p, o), y);
}

}  // namespace

int gnan::launch_lone(const gnan_spmm_args* a, int lpr, hipStream_t st) {
  if (!a->lone_rows) return GNAN_OK;
  Params p = make_params(a);
  // (pick_route(): the self_sum route is the packed small-D CSR walk read 16 B per lane — the variant whose tile plan names the lone rows)
  if (int rc = plan_tiles(p, 4, lpr, false, true, a->seg_max_per_class, a->hub_seg_max_per_class)) return rc;
  if (p.lone_n <= 0) return GNAN_OK;         // (no lone row, or no run is tiled: the rows stay where they were, and no empty grid)
  const int64_t nb = (p.lone_n + kLoneBlock - 1) / kLoneBlock;
  if (nb > 0x7fffffffLL) return gnan::fail(GNAN_ERR_UNSUPPORTED, "spmm: too many lone rows for one launch");
  const dim3 grid(static_cast<unsigned>(nb)), block(kLoneBlock);
  if (lpr == 16) hipLaunchKernelGGL(spmm_lone_kernel<16>, grid, block, 0, st, p);
  else if (lpr == 32) hipLaunchKernelGGL(spmm_lone_kernel<32>, grid, block, 0, st, p);
  else hipLaunchKernelGGL(spmm_lone_kernel<64>, grid, block, 0, st, p);
  return gnan::check_launch("spmm_lone_kernel");
}

int gnan::lone_blocks(int64_t lone_n) { return static_cast<int>((lone_n + kLoneBlock - 1) / kLoneBlock); }
