// The split-order sum of the shape functions' partial parameter gradients, shared by the three backward files
// (csrc/fmlp_bwd.hip, csrc/fmlp_bwd_mfma.hip, csrc/fmlp_mc.hip): each cuts a feature's nodes into ranges ("splits"), every split
// writes one block [w_first | b_first | w_mid | b_mid | w_last | b_last] of partial gradients into the workspace, and this
// kernel adds the blocks in split order — no atomics, the same bits on every run.
#pragma once
#include "common.hpp"

namespace gnan {

struct SplitReduceOuts {
  float* out[6];
  int64_t off[6];       // start of the tensor inside a split's block; off[t + 1] - off[t] elements
  int64_t end;          // block size
};

// out[i] = sum over the splits of partial[s * stride + i], in split order — all six gradient tensors in ONE launch (a launch per
// tensor was six launches behind a 15-us kernel on a few hundred inputs).
static __global__ __launch_bounds__(256) void fmlp_split_reduce_kernel(const float* __restrict__ partial, int64_t stride, int splits,
                                                                       const SplitReduceOuts r) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= r.end) return;
  float a = partial[i];
  for (int s = 1; s < splits; ++s) a += partial[static_cast<int64_t>(s) * stride + i];
  int t = 0;
#pragma unroll
  for (int u = 1; u < 6; ++u) t = i >= r.off[u] ? u : t;
  if (r.out[t]) r.out[t][i - r.off[t]] = a;
}

}  // namespace gnan
