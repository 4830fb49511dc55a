// Shape functions by exact piecewise-linear table look-up (gfx950).
//
// f_k is a ReLU MLP of a scalar, i.e. exactly piecewise linear; gnan_amd/pwl.py tabulates it per forward
// (anchor / value / slope per piece, ~130 pieces for H = 64, L = 3).  This kernel evaluates
//     f_k(x) = val[i] + slope[i] * (x - anchor[i]),   i = #{ breakpoints of f_k <= x }
// for every (node, feature): it replaces the F x L addmm/relu launches of GNAN.py:57-62 by N*F binary
// searches in LDS.  HBM-bound (x in, fx out), no matrix work at all.
//
// Mapping: a workgroup owns a contiguous block of nodes and a group of <= FG consecutive features whose
// tables it copies to LDS once (amortised over the node block).  Thread = (node, 4 features): one 16-B load,
// 4 searches in lock-step (independent LDS reads per step hide the LDS latency), one 16-B store; the 4 threads
// of a node cover one 64-B sector of x and of fx.
//
// This file: gnan_fpwl_fwd and its routing (direct index: csrc/fpwl_index.hip; one channel: csrc/fpwl_fast.hip; else the
// general kernel here) and the workspace queries.  The backward is csrc/fpwl_moments.hip; what they share, csrc/fpwl_common.hpp.
#include "fpwl_common.hpp"

namespace {
using namespace gnan::fpwl;

// SUM: out[n, c] = sum over features (f_sums, GNAN.py:157); FAST: C == 1, full groups, 16-B aligned rows;
// OUT16 (FAST, per-feature output only): store bf16 rows — the operand format of the bf16-storage aggregation.
// BS threads per workgroup: the LDS image of the tables is shared by BS / 64 waves, so a large workgroup is what buys
// occupancy here (25 KB of tables per 4 waves would cap a CU at 20 waves; per 8 waves it reaches the full 32).
template <int FG, bool SUM, bool FAST, bool OUT16 = false, int BS = 256>
__global__ __launch_bounds__(BS) void fpwl_kernel(const Params p) {
  constexpr int FPT = Map<FG, BS>::FPT, TPN = Map<FG, BS>::TPN, NODES = Map<FG, BS>::NODES;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  __shared__ int s_off[FG + 1];
  const int tid = threadIdx.x;
  const int q = tid % TPN;            // which feature quad of the group
  const int nl = tid / TPN;           // node slot inside a pass
  const int C = p.C;
  int64_t nb = blockIdx.x;
  int g_first = 0;
  if (!SUM) xcd_block(blockIdx.x, p.n_groups, nb, g_first);   // per-feature mode: a workgroup per (node block, group)
  const int64_t n_lo = nb * p.nodes_per_block;
  if (n_lo >= p.n) return;
  const int64_t n_hi = n_lo + p.nodes_per_block < p.n ? n_lo + p.nodes_per_block : p.n;
  const int g_lo = SUM ? 0 : g_first;
  const int g_hi = SUM ? p.n_groups : g_lo + 1;
  float* acc_l = smem + p.acc_offset;
  if (SUM && p.acc_offset) {
    for (int i = tid; i < C * NODES; i += BS) acc_l[i] = 0.f;
  }

  for (int g = g_lo; g < g_hi; ++g) {
    const int k0 = g * FG;
    const int nf = FAST ? FG : (p.F - k0 < FG ? p.F - k0 : FG);
    const int base = p.off[k0];
    const int tot = p.off[k0 + nf] - base;
    const int Cs = table_stride(C);
    float* anchor_l = smem;
    float* val_l = smem + tot;
    float* slope_l = val_l + static_cast<int64_t>(tot) * Cs;
    __syncthreads();  // previous group's searches are done with the LDS tables
    for (int i = tid; i < tot; i += BS) anchor_l[i] = p.anchor[base + i];
    if (Cs == C) {
      for (int i = tid; i < tot * C; i += BS) {
        val_l[i] = p.val[static_cast<int64_t>(base) * C + i];
        slope_l[i] = p.slope[static_cast<int64_t>(base) * C + i];
      }
    } else {
      for (int i = tid; i < tot * C; i += BS) {
        const int r = i / C, j = r * Cs + (i - r * C);
        val_l[j] = p.val[static_cast<int64_t>(base) * C + i];
        slope_l[j] = p.slope[static_cast<int64_t>(base) * C + i];
      }
    }
    if (tid <= nf) s_off[tid] = p.off[k0 + tid] - base;
    __syncthreads();
    int po[FPT], pn[FPT];
    bool live[FPT];
#pragma unroll
    for (int f = 0; f < FPT; ++f) {
      const int fg = q * FPT + f;
      live[f] = fg < nf;
      po[f] = live[f] ? s_off[fg] : 0;
      pn[f] = live[f] ? s_off[fg + 1] - s_off[fg] - 1 : 0;
    }

    float ps[FPT];  // this thread's share of the column sums of fx (rest-bucket total of the aggregation)
#pragma unroll
    for (int f = 0; f < FPT; ++f) ps[f] = 0.f;
    for (int64_t n = n_lo + nl; n < n_hi; n += NODES) {
      float xv[FPT];
      const float* xr = p.x + n * p.x_stride + k0 + q * FPT;
      if constexpr (FAST && FPT == 4) {
        const float4 t = *reinterpret_cast<const float4*>(xr);
        xv[0] = t.x; xv[1 % FPT] = t.y; xv[2 % FPT] = t.z; xv[3 % FPT] = t.w;
      } else {
#pragma unroll
        for (int f = 0; f < FPT; ++f) xv[f] = live[f] ? xr[f] : 0.f;
      }
      int idx[FPT];
      search<FPT>(anchor_l, po, pn, xv, p.step0, idx);
      float d[FPT];
#pragma unroll
      for (int f = 0; f < FPT; ++f) d[f] = xv[f] - anchor_l[idx[f]];

      if constexpr (SUM) {
        float* o = p.out + n * p.out_stride;
        // channels in chunks of CU: the run-time loop over C is not unrolled by the compiler, and one channel per iteration
        // is a chain of four dependent LDS round trips (table reads, accumulator read, write) — at one workgroup per CU
        // (C = 40: 129 KB of LDS) that chain, not bandwidth, set the kernel's time (arxiv-shaped C = 40: 2.3 ms)
        constexpr int CU = FAST ? 1 : 8;
        for (int c0 = 0; c0 < (FAST ? 1 : C); c0 += CU) {
          float a[CU];
#pragma unroll
          for (int u = 0; u < CU; ++u) {
            const int c = c0 + u < C ? c0 + u : C - 1;       // tail: an in-range read whose result is dropped
            a[u] = 0.f;
#pragma unroll
            for (int f = 0; f < FPT; ++f)
              if (live[f]) a[u] += fmaf(slope_l[idx[f] * Cs + c], d[f], val_l[idx[f] * Cs + c]);
          }
#pragma unroll
          for (int off = 1; off < TPN; off <<= 1)            // the node's TPN threads
#pragma unroll
            for (int u = 0; u < CU; ++u) a[u] += __shfl_xor(a[u], off);
          // groups run one after the other inside the workgroup and a node keeps its thread: no race
          if (q == 0) {
            if (p.acc_offset) {                              // many channels: accumulate on chip, store once
              float old[CU];
#pragma unroll
              for (int u = 0; u < CU; ++u) old[u] = acc_l[(c0 + u < C ? c0 + u : C - 1) * NODES + nl];
#pragma unroll
              for (int u = 0; u < CU; ++u)
                if (c0 + u < C) acc_l[(c0 + u) * NODES + nl] = old[u] + a[u];
            } else {
#pragma unroll
              for (int u = 0; u < CU; ++u)
                if (c0 + u < C) o[c0 + u] = g == 0 ? a[u] : o[c0 + u] + a[u];
            }
          }
        }
      } else {
        float* o = p.out + n * p.out_stride + static_cast<int64_t>(k0 + q * FPT) * C;
        if constexpr (FAST && FPT == 4) {
          float4 t;
          t.x = fmaf(slope_l[idx[0]], d[0], val_l[idx[0]]);
          t.y = fmaf(slope_l[idx[1 % FPT]], d[1 % FPT], val_l[idx[1 % FPT]]);
          t.z = fmaf(slope_l[idx[2 % FPT]], d[2 % FPT], val_l[idx[2 % FPT]]);
          t.w = fmaf(slope_l[idx[3 % FPT]], d[3 % FPT], val_l[idx[3 % FPT]]);
          if constexpr (OUT16) {
            t = store_bf16_quad(reinterpret_cast<uint16_t*>(p.out) + n * p.out_stride + (k0 + q * FPT), t);
          } else {
            *reinterpret_cast<float4*>(o) = t;
          }
          if (n < p.total_rows) { ps[0] += t.x; ps[1 % FPT] += t.y; ps[2 % FPT] += t.z; ps[3 % FPT] += t.w; }
        } else {
#pragma unroll
          for (int f = 0; f < FPT; ++f)
            if (live[f])
              for (int c = 0; c < C; ++c) o[f * C + c] = fmaf(slope_l[idx[f] * Cs + c], d[f], val_l[idx[f] * Cs + c]);
        }
      }
    }
    if constexpr (FAST && !SUM && FPT == 4) {
      // FAST: C == 1, tables take 3 floats per piece; the scratch lies behind them
      if (p.col_partial) block_column_sums<FG, BS>(smem + tot * 3, ps, p.col_partial, nb, p.F, k0);
    }
  }
  if (SUM && p.acc_offset) {
    __syncthreads();
    const int64_t n = n_lo + nl;
    if (n < n_hi)
      for (int c = q; c < C; c += TPN) p.out[n * p.out_stride + c] = acc_l[c * NODES + nl];
  }
}

// One workgroup per column: 256 threads stride over the per-workgroup partials, then a fixed-order tree.
__global__ __launch_bounds__(256) void fpwl_total_kernel(const double* __restrict__ partial, int blocks, int W,
                                                         float* __restrict__ total) {
  __shared__ double red[256];
  const int w = blockIdx.x;
  double s = 0.0;
  for (int b = threadIdx.x; b < blocks; b += 256) s += partial[static_cast<int64_t>(b) * W + w];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if (static_cast<int>(threadIdx.x) < st) red[threadIdx.x] += red[threadIdx.x + st];
    __syncthreads();
  }
  if (threadIdx.x == 0) total[w] = static_cast<float>(red[0]);
}

int launch_total(const double* partial, int64_t blocks, int F, float* total, hipStream_t st) {
  hipLaunchKernelGGL(fpwl_total_kernel, dim3(F), dim3(256), 0, st, partial, static_cast<int>(blocks), F, total);
  return gnan::check_launch("fpwl_total_kernel");
}

template <int FG, int BS>
int launch(Params p, size_t lds, hipStream_t st, float* total_out) {
  const size_t table_lds = lds;            // (1 + 2C) floats per piece of the largest group
  if (p.sum_features && p.C > 1) {        // accumulate the feature sum in LDS: one pass of nodes per workgroup
    if (lds + static_cast<size_t>(p.C) * Map<FG, BS>::NODES * sizeof(float) <= kMaxLds) {
      p.acc_offset = static_cast<int>(lds / sizeof(float));
      p.nodes_per_block = Map<FG, BS>::NODES;
    }
  }
  const int64_t bx = (p.n + p.nodes_per_block - 1) / p.nodes_per_block;
  const int64_t wgs = p.sum_features ? bx : (bx + 7) / 8 * 8 * p.n_groups;     // see xcd_block
  if (wgs > 0x7fffffffLL) return gnan::fail(GNAN_ERR_UNSUPPORTED, "fpwl: too many nodes for one launch");
  const dim3 grid(static_cast<unsigned>(wgs));
  if (p.acc_offset) lds += static_cast<size_t>(p.C) * Map<FG, BS>::NODES * sizeof(float);
  // FAST: one output channel, whole groups only, 16-B aligned x (and fx) rows
  const bool whole = p.F % FG == 0 && p.vec_x;                       // whole groups, 16-B aligned rows of x
  const bool ragged = FG % 4 == 0 && p.C == 1 && p.sum_features && !whole && !p.out_bf16 && !p.col_partial;
  const bool fast = FG % 4 == 0 && p.C == 1 && ((whole && (p.sum_features || p.vec_out)) || ragged);
  if (p.col_partial) {
    if (!fast || p.sum_features)
      return gnan::fail(GNAN_ERR_UNSUPPORTED, "fpwl: fused column sums need C == 1, F %% %d == 0, 16-B aligned rows, per-feature output", FG);
    lds += BS * 4 * sizeof(float);
  }
  if constexpr (FG % 4 == 0) {
    const int nstep = nstep_of(p.max_pieces);
    // trees + (val, slope) pairs + anchors in piece order (C == 1: 3 floats per piece); the column-sum scratch re-uses it
    size_t lds_fast = tree_words(FG, nstep) * sizeof(float) + table_lds;
    if (p.col_partial && lds_fast < BS * 4 * sizeof(float)) lds_fast = BS * 4 * sizeof(float);
    p.soff_offset = static_cast<int>(lds_fast / sizeof(float));
    lds_fast += (FG + 1) * sizeof(int);
    if (p.piece_out && !(fast && p.sum_features && nstep <= 8 && lds_fast <= kMaxLds))
      return gnan::fail(GNAN_ERR_UNSUPPORTED, "fpwl: piece_out needs the fast feature-sum kernel (C == 1, feature quads) and at most 256 pieces per feature");
    if (fast && nstep <= 10 && lds_fast <= kMaxLds) {
      if (int rc = launch_fast(p, FG, BS, nstep, ragged, wgs, lds_fast, st)) return rc;
      return p.col_partial ? launch_total(p.col_partial, bx, p.F, total_out, st) : GNAN_OK;
    }
  }
  if (p.piece_out) return gnan::fail(GNAN_ERR_UNSUPPORTED, "fpwl: piece_out needs the fast feature-sum kernel");
  auto go = [&](auto kernel) { return launch_with_lds(kernel, "fpwl_kernel", grid, BS, lds, st, p); };
  if (p.out_bf16) {
    if constexpr (FG % 4 == 0) {
      if (!fast || p.sum_features)
        return gnan::fail(GNAN_ERR_UNSUPPORTED, "fpwl: bf16 output needs C == 1, whole feature groups, aligned rows, per-feature mode");
      if (int rc = go(fpwl_kernel<FG, false, true, true, BS>)) return rc;
    } else {
      return gnan::fail(GNAN_ERR_UNSUPPORTED, "fpwl: bf16 output needs feature groups of >= 4");
    }
  } else {
    if (p.sum_features) return fast ? go(fpwl_kernel<FG, true, true, false, BS>) : go(fpwl_kernel<FG, true, false, false, BS>);
    if (int rc = fast ? go(fpwl_kernel<FG, false, true, false, BS>) : go(fpwl_kernel<FG, false, false, false, BS>)) return rc;
  }
  return p.col_partial ? launch_total(p.col_partial, bx, p.F, total_out, st) : GNAN_OK;
}

}  // namespace

extern "C" int gnan_fpwl_fwd(const gnan_fpwl_args* a, gnan_stream_t stream) {
  if (int rc = common_checks(a)) return rc;
  if (a->n == 0) return GNAN_OK;
  GNAN_REQUIRE(a->out && a->val && a->slope, "fpwl: null pointer");
  const int fg = a->features_per_group;
  const int64_t ow = a->sum_features ? a->C : static_cast<int64_t>(a->F) * a->C;
  GNAN_REQUIRE(a->out_stride >= ow, "fpwl: out row stride smaller than the output width");
  GNAN_REQUIRE(a->out_dtype == GNAN_F32 || a->out_dtype == GNAN_BF16, "fpwl: unknown out_dtype");
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (fg == 16 && !(a->total && a->sum_features) && index_applies(a)) {
    double* partial = nullptr;
    const int64_t ibx = (a->n + index_nodes_per_block(a) - 1) / index_nodes_per_block(a);
    if (a->total) {
      const size_t need = static_cast<size_t>(ibx) * a->F * sizeof(double);
      if (a->total_workspace == nullptr || a->total_workspace_bytes < need)
        return gnan::fail(GNAN_ERR_WORKSPACE, "fpwl: total workspace %zu B < required %zu B", a->total_workspace_bytes, need);
      partial = static_cast<double*>(a->total_workspace);
    }
    if (int rc = index_fwd(a, partial, st)) return rc;
    return partial ? launch_total(partial, ibx, a->F, a->total, st) : GNAN_OK;
  }
  if (a->sum_total)
    return gnan::fail(GNAN_ERR_UNSUPPORTED, "fpwl: sum_total is written by the group-split direct-index feature sum only");
  if (a->row_sum || a->row_keep)
    return gnan::fail(GNAN_ERR_UNSUPPORTED, "fpwl: row_sum / row_keep are served by the direct-index look-up in per-feature rows mode only");
  const size_t lds = static_cast<size_t>(a->max_group_pieces) * (1 + 2 * static_cast<size_t>(table_stride(a->C))) * sizeof(float);
  Params p = base_params(a);
  auto aligned = [](const void* ptr) { return (reinterpret_cast<uintptr_t>(ptr) % 16) == 0; };
  p.vec_x = fg % 4 == 0 && a->F % 4 == 0 && a->x_stride % 4 == 0 && aligned(a->x);
  p.vec_out = fg % 4 == 0 && a->F % 4 == 0 && a->out_stride % 4 == 0 && aligned(a->out);
  if (a->total) {
    const int64_t bx = (p.n + p.nodes_per_block - 1) / p.nodes_per_block;
    const size_t need = static_cast<size_t>(bx) * a->F * sizeof(double);
    if (a->total_workspace == nullptr || a->total_workspace_bytes < need)
      return gnan::fail(GNAN_ERR_WORKSPACE, "fpwl: total workspace %zu B < required %zu B", a->total_workspace_bytes, need);
    p.col_partial = static_cast<double*>(a->total_workspace);
  }
  // wide groups: 512-thread workgroups share one LDS image of the tables (A/B on C4: 1.92 -> 1.42 ms; 1024: 1.50 ms)
  // feature sum with many channels: the tables of a group are reloaded per pass of nodes, so the widest workgroup whose
  // [C][nodes] accumulators still fit LDS wins (arxiv-shaped, C = 40: one feature per group, 46 KB of tables per pass)
  if (a->sum_features && a->C > 1 && fg <= 4) {
    const int tpn = fg < 4 ? 1 : fg / 4;
    auto fits = [&](int bs) { return lds + static_cast<size_t>(a->C) * (bs / tpn) * sizeof(float) <= kMaxLds; };
    const int bs = fits(1024) ? 1024 : fits(512) ? 512 : 256;
    switch (fg * 10000 + bs) {
      case 11024: return launch<1, 1024>(p, lds, st, a->total);
      case 10512: return launch<1, 512>(p, lds, st, a->total);
      case 21024: return launch<2, 1024>(p, lds, st, a->total);
      case 20512: return launch<2, 512>(p, lds, st, a->total);
      case 41024: return launch<4, 1024>(p, lds, st, a->total);
      case 40512: return launch<4, 512>(p, lds, st, a->total);
      default: break;
    }
  }
  switch (fg) {
    case 1: return launch<1, 256>(p, lds, st, a->total);
    case 2: return launch<2, 256>(p, lds, st, a->total);
    case 4: return launch<4, 256>(p, lds, st, a->total);
    case 8: return launch<8, 512>(p, lds, st, a->total);
    default: return launch<16, 512>(p, lds, st, a->total);
  }
}

extern "C" size_t gnan_fpwl_sum_workspace_bytes(const gnan_fpwl_args* a) {
  if (!a || a->n <= 0 || a->features_per_group != 16 || (a->total && a->sum_features)) return 0;
  return index_sum_workspace_bytes(a);
}

extern "C" size_t gnan_fpwl_total_workspace_bytes(const gnan_fpwl_args* a) {
  if (!a || a->n <= 0) return 0;
  const Params p = base_params(a);
  int64_t bx = (p.n + p.nodes_per_block - 1) / p.nodes_per_block;
  if (a->features_per_group == 16 && index_applies(a)) {       // whichever kernel serves the call: room for both
    const int64_t ibx = (a->n + index_nodes_per_block(a) - 1) / index_nodes_per_block(a);
    if (ibx > bx) bx = ibx;
  }
  return static_cast<size_t>(bx) * a->F * sizeof(double);
}
