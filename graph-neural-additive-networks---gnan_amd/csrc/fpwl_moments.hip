// Backward of the table look-up (gfx950): per-piece moments of the upstream gradient
//   M[t, 0, c] = sum_{(n,k) in piece t} g[n,k,c]            M[t, 1, c] = sum g[n,k,c] * (x[n,k] - anchor[t])
// On a piece f_k is affine in x AND so is d f_k(x) / d theta (fixed activation pattern), hence the parameter
// gradient  sum_n g_n * df_k(x_n)/dtheta  depends on the nodes of a piece only through these two moments;
// gnan_amd/pwl.py turns them into exact parameter gradients by back-propagating through the tiny MLP at
// two points per piece.  Same traversal as the forward (csrc/fpwl.hip); bins live in LDS (ds_add) and are flushed with
// one global atomic per bin per workgroup.  Here: the general kernel (any C, any feature count, float or fixed-point bins), the
// fixed-point kernel with the tree search, the routing and the entry points; the one-channel kernel is csrc/fpwl_moments_c1_body.hpp.
#include "fpwl_common.hpp"

namespace {
using namespace gnan::fpwl;

template <int FG, int BS, bool FIXED>
__global__ __launch_bounds__(BS) void fpwl_moments_kernel(const MomentParams mp) {
  using bin_t = std::conditional_t<FIXED, unsigned long long, float>;
  constexpr int FPT = Map<FG, BS>::FPT, TPN = Map<FG, BS>::TPN, NODES = Map<FG, BS>::NODES;
  const Params& p = mp.f;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  __shared__ int s_off[FG + 1];
  const int tid = threadIdx.x;
  const int q = tid % TPN, nl = tid / TPN;
  const int C = p.C;
  const int64_t n_lo = static_cast<int64_t>(blockIdx.x) * p.nodes_per_block;
  const int64_t n_hi = n_lo + p.nodes_per_block < p.n ? n_lo + p.nodes_per_block : p.n;
  const int k0 = blockIdx.y * FG;
  const int nf = p.F - k0 < FG ? p.F - k0 : FG;
  const int base = p.off[k0];
  const int tot = p.off[k0 + nf] - base;
  float* anchor_l = smem;
  const int Rb = bin_stride(C);
  bin_t* bins = reinterpret_cast<bin_t*>(smem + (tot + 1) / 2 * 2);   // [tot][2][C] (+ 1 bin of padding per piece), 8-byte aligned
  for (int i = tid; i < tot; i += BS) anchor_l[i] = p.anchor[base + i];
  for (int i = tid; i < tot * Rb; i += BS) bins[i] = bin_t(0);
  double s0 = 1.0, s1 = 1.0;
  if constexpr (FIXED) { s0 = mp.scales[0]; s1 = mp.scales[1]; }
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
  for (int64_t n = n_lo + nl; n < n_hi; n += NODES) {
    float xv[FPT];
    const float* xr = p.x + n * p.x_stride + k0 + q * FPT;
#pragma unroll
    for (int f = 0; f < FPT; ++f) xv[f] = live[f] ? xr[f] : 0.f;
    int idx[FPT];
    search<FPT>(anchor_l, po, pn, xv, p.step0, idx);
    const float* gr = mp.g + n * mp.g_stride + (p.sum_features ? 0 : static_cast<int64_t>(k0 + q * FPT) * C);
    float d[FPT];
    bin_t* b[FPT];
#pragma unroll
    for (int f = 0; f < FPT; ++f) {
      d[f] = xv[f] - anchor_l[idx[f]];
      b[f] = bins + static_cast<int64_t>(idx[f]) * Rb;
    }
    // channel-major: in feature-sum mode a channel's gradient is read (and converted) once for the thread's features;
    // channels in chunks of 8 so that the (node-strided, i.e. uncoalesced) gradient loads of a chunk are in flight
    // together — one channel per iteration of the run-time loop waited a full memory latency per channel
    for (int c0 = 0; c0 < C; c0 += 8) {
      float gs[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) gs[u] = (p.sum_features && c0 + u < C) ? gr[c0 + u] : 0.f;
#pragma unroll
      for (int f = 0; f < FPT; ++f) {
        if (live[f]) {
          float gf[8];
#pragma unroll
          for (int u = 0; u < 8; ++u) gf[u] = p.sum_features ? gs[u] : (c0 + u < C ? gr[f * C + c0 + u] : 0.f);
#pragma unroll
          for (int u = 0; u < 8; ++u) {
            const int c = c0 + u;
            if (c < C) {
              if constexpr (FIXED) {
                atomicAdd(b[f] + c, fixed_bits(gf[u], s0));
                atomicAdd(b[f] + C + c, fixed_bits(gf[u] * d[f], s1));
              } else {
                atomicAdd(b[f] + c, gf[u]);
                atomicAdd(b[f] + C + c, gf[u] * d[f]);
              }
            }
          }
        }
      }
    }
  }
  __syncthreads();
  if constexpr (FIXED) flush_bins<BS>(bins, tot, C, Rb, mp.Mi + static_cast<int64_t>(base) * 2 * C);
  else flush_bins<BS>(bins, tot, C, Rb, mp.M + static_cast<int64_t>(base) * 2 * C);
}

// Fixed-point moments with the search of fpwl_fast_kernel (skewed breadth-first trees, 3 instructions per step; whole feature
// groups, <= 1023 pieces per feature).  With padded SORTED anchors, aligned alike for the four quads of a wave, 75 % of this
// kernel's LDS cycles were bank conflicts (SQ_LDS_BANK_CONFLICT 7.9e8 of SQ_LDS_IDX_ACTIVE 1.06e9 on C4).
// LDS = trees [FG][2^NSTEP] (+ skew) | 64-bit bins [tot][2][C] | anchors in piece order [tot] | group offsets.
template <int FG, int NSTEP, int BS>
__global__ __launch_bounds__(BS) void fpwl_moments_fast_kernel(const MomentParams mp) {
  static_assert(FG % 4 == 0, "feature quads");
  constexpr int FPT = 4, TPN = FG / FPT, NODES = BS / TPN, P2 = 1 << NSTEP;
  constexpr int kTreeWords = tree_words(FG, NSTEP);                     // even: the bins behind it are 8-byte aligned
  const Params& p = mp.f;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = threadIdx.x;
  const int q = tid % TPN, nl = tid / TPN;
  const int C = p.C;
  const int64_t n_lo = static_cast<int64_t>(blockIdx.x) * p.nodes_per_block;
  const int64_t n_hi = n_lo + p.nodes_per_block < p.n ? n_lo + p.nodes_per_block : p.n;
  const int k0 = blockIdx.y * FG;
  const int base = p.off[k0];
  const int tot = p.off[k0 + FG] - base;
  const int Rb = bin_stride(C);
  unsigned long long* bins = reinterpret_cast<unsigned long long*>(smem + kTreeWords);
  float* an_l = reinterpret_cast<float*>(bins + static_cast<int64_t>(tot) * Rb);
  int* s_off = reinterpret_cast<int*>(smem) + p.soff_offset;
  const unsigned lds_base = lds_address(smem);
  if (tid <= FG) s_off[tid] = p.off[k0 + tid] - base;
  for (int i = tid; i < tot * Rb; i += BS) bins[i] = 0ull;
  for (int i = tid; i < tot; i += BS) an_l[i] = p.anchor[base + i];
  __syncthreads();
  build_trees<FG, NSTEP, BS>(smem, s_off, p.anchor, base);
  __syncthreads();
  const TreeBase tb = tree_base<NSTEP>(lds_base, q);
  const int Q = tb.Q;
  int binoff[FPT];
#pragma unroll
  for (int f = 0; f < FPT; ++f) binoff[f] = s_off[q * FPT + f];
  const double s0 = mp.scales[0], s1 = mp.scales[1];
  for (int64_t n = n_lo + nl; n < n_hi; n += NODES) {
    const float* xr = p.x + n * p.x_stride + k0 + q * FPT;
    float xv[FPT];
    if (p.vec_x) {
      const float4 t = *reinterpret_cast<const float4*>(xr);
      xv[0] = t.x; xv[1] = t.y; xv[2] = t.z; xv[3] = t.w;
    } else {
#pragma unroll
      for (int f = 0; f < FPT; ++f) xv[f] = xr[f];
    }
    int a[FPT];
    tree_search<NSTEP>(tb, xv, a);
    const float* gr = mp.g + n * mp.g_stride + (p.sum_features ? 0 : static_cast<int64_t>(k0 + q * FPT) * C);
    float d[FPT];
    unsigned long long* b[FPT];
#pragma unroll
    for (int f = 0; f < FPT; ++f) {
      const int piece = binoff[f] + (((a[f] - Q) >> 2) - P2);
      d[f] = xv[f] - an_l[piece];
      b[f] = bins + static_cast<int64_t>(piece) * Rb;
    }
    // (the channel loop of fpwl_moments_kernel, every feature live; as a shared helper it changed the scalar registers of four
    //  general instances: profiles/r21_fpwl_split_code_objects.txt)
    for (int c0 = 0; c0 < C; c0 += 8) {
      float gs[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) gs[u] = (p.sum_features && c0 + u < C) ? gr[c0 + u] : 0.f;
#pragma unroll
      for (int f = 0; f < FPT; ++f) {
        float gf[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) gf[u] = p.sum_features ? gs[u] : (c0 + u < C ? gr[f * C + c0 + u] : 0.f);
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int c = c0 + u;
          if (c < C) {
            atomicAdd(b[f] + c, fixed_bits(gf[u], s0));
            atomicAdd(b[f] + C + c, fixed_bits(gf[u] * d[f], s1));
          }
        }
      }
    }
  }
  __syncthreads();
  flush_bins<BS>(bins, tot, C, Rb, mp.Mi + static_cast<int64_t>(base) * 2 * C);
}

template <int FG, int NSTEP, int BS>
int launch_moments_fast(MomentParams mp, hipStream_t st, gnan_fpwl_moments_info* probe) {
  Params& p = mp.f;
  const size_t pieces = static_cast<size_t>(p.max_group_pieces);
  size_t lds = tree_words(FG, NSTEP) * sizeof(float) + pieces * static_cast<size_t>(bin_stride(p.C)) * sizeof(unsigned long long) +
               pieces * sizeof(float);
  p.soff_offset = static_cast<int>(lds / sizeof(float));
  lds += (FG + 1) * sizeof(int);
  if (lds > kMaxLds) return -1;                          // caller falls back to the plain kernel
  if (probe) {
    fill_probe(probe, GNAN_FPWL_MOMENTS_FAST, NSTEP, p, BS / (FG / 4), BS, false, lds);
    return GNAN_OK;
  }
  const int64_t bx = (p.n + p.nodes_per_block - 1) / p.nodes_per_block;
  if (bx > 0x7fffffffLL) return gnan::fail(GNAN_ERR_UNSUPPORTED, "fpwl: too many nodes for one launch");
  return launch_with_lds(fpwl_moments_fast_kernel<FG, NSTEP, BS>, "fpwl_moments_fast_kernel",
                         dim3(static_cast<unsigned>(bx), static_cast<unsigned>(p.n_groups)), BS, lds, st, mp);
}

template <int FG, int BS>
int launch_moments(const MomentParams& mp_in, size_t lds, hipStream_t st, gnan_fpwl_moments_info* probe) {
  MomentParams mp = mp_in;
  if (mp.f.max_pieces > 256) mp.f.piece_in = nullptr;      // one byte per look-up: searched again instead
  const bool fixed = mp.Mi != nullptr;
  if constexpr (FG % 4 == 0) {
    const int nstep = nstep_of(mp.f.max_pieces);
    if (fixed && nstep <= 10) {                             // the tree kernels: fixed-point bins, at most 1024 pieces per feature
      const bool whole = mp.f.F % FG == 0 && mp.f.vec_x;
      // one channel: the C == 1 kernel, its RAGGED variant for a ragged feature count / unaligned rows
      // (GNAN_FPWL_MOMENTS_GENERAL keeps the kernels of this file: A/B aid, tests)
      if (mp.f.C == 1 && !mp.general_only) {
        const int rc = launch_moments_c1(mp, FG, BS, nstep, !whole, st, probe);
        if (rc != -1) return rc;
      }
      if (mp.f.F % FG == 0) {
        const int rc = by_nstep(nstep, [&](auto ns) { return launch_moments_fast<FG, decltype(ns)::value, BS>(mp, st, probe); });
        if (rc != -1) return rc;
      }
    }
  }
  if (probe) {
    fill_probe(probe, fixed ? GNAN_FPWL_MOMENTS_GENERAL_FIXED : GNAN_FPWL_MOMENTS_GENERAL_FLOAT, 0, mp.f, Map<FG, BS>::NODES, BS,
               false, lds);
    return GNAN_OK;
  }
  const Params& p = mp.f;
  const int64_t bx = (p.n + p.nodes_per_block - 1) / p.nodes_per_block;
  if (bx > 0x7fffffffLL) return gnan::fail(GNAN_ERR_UNSUPPORTED, "fpwl: too many nodes for one launch");
  const dim3 grid(static_cast<unsigned>(bx), static_cast<unsigned>(p.n_groups));
  if (fixed) return launch_with_lds(fpwl_moments_kernel<FG, BS, true>, "fpwl_moments_kernel", grid, BS, lds, st, mp);
  return launch_with_lds(fpwl_moments_kernel<FG, BS, false>, "fpwl_moments_kernel", grid, BS, lds, st, mp);
}

int moments_common(const gnan_fpwl_args* a, const float* grad, int64_t grad_stride, float* moments,
                   const double* scales, int64_t* moments_fixed, gnan_stream_t stream, gnan_fpwl_moments_info* probe = nullptr) {
  if (int rc = common_checks(a)) return rc;
  if (probe) *probe = gnan_fpwl_moments_info{};
  if (a->n == 0) return GNAN_OK;
  const int64_t gw = a->sum_features ? a->C : static_cast<int64_t>(a->F) * a->C;
  GNAN_REQUIRE(grad_stride >= gw, "fpwl_moments: grad row stride smaller than its width");
  MomentParams mp;
  mp.f = base_params(a);
  mp.g = grad; mp.g_stride = grad_stride; mp.M = moments;
  mp.scales = scales; mp.Mi = reinterpret_cast<unsigned long long*>(moments_fixed);
  mp.general_only = (a->flags & GNAN_FPWL_MOMENTS_GENERAL) != 0;
  mp.f.vec_x = a->features_per_group % 4 == 0 && a->F % 4 == 0 && a->x_stride % 4 == 0 &&
               reinterpret_cast<uintptr_t>(a->x) % 16 == 0;
  mp.vec_g = !a->sum_features && a->C == 1 && grad_stride % 4 == 0 && reinterpret_cast<uintptr_t>(grad) % 16 == 0;
  const size_t bin = moments_fixed ? sizeof(unsigned long long) : sizeof(float);
  const size_t pieces = static_cast<size_t>(a->max_group_pieces);
  const size_t lds = (pieces + 1) / 2 * 2 * sizeof(float) + pieces * static_cast<size_t>(bin_stride(a->C)) * bin;
  if (lds > kMaxLds)
    return gnan::fail(GNAN_ERR_UNSUPPORTED, "fpwl_moments: %zu B of bins per feature group exceed LDS", lds);
  hipStream_t st = static_cast<hipStream_t>(stream);
  // few features per group means many channels: tens of KB of bins per workgroup, so only a wide workgroup puts enough
  // waves on a CU (arxiv-shaped, C = 40: 91 KB of bins per feature -> one workgroup per CU)
  const bool wide = lds > 40 * 1024;
  switch (a->features_per_group) {
    case 1: return wide ? launch_moments<1, 1024>(mp, lds, st, probe) : launch_moments<1, 256>(mp, lds, st, probe);
    case 2: return wide ? launch_moments<2, 1024>(mp, lds, st, probe) : launch_moments<2, 256>(mp, lds, st, probe);
    case 4: return wide ? launch_moments<4, 1024>(mp, lds, st, probe) : launch_moments<4, 256>(mp, lds, st, probe);
    case 8: return launch_moments<8, 512>(mp, lds, st, probe);
    default: return launch_moments<16, 512>(mp, lds, st, probe);
  }
}
}  // namespace

extern "C" int gnan_fpwl_moments(const gnan_fpwl_args* a, const float* grad, int64_t grad_stride, float* moments,
                                 gnan_stream_t stream) {
  GNAN_REQUIRE(a == nullptr || a->n == 0 || (grad && moments), "fpwl_moments: null grad / moments");
  return moments_common(a, grad, grad_stride, moments, nullptr, nullptr, stream);
}

extern "C" int gnan_fpwl_moments_fixed(const gnan_fpwl_args* a, const float* grad, int64_t grad_stride,
                                       const double* scales, int64_t* moments, gnan_stream_t stream) {
  GNAN_REQUIRE(a == nullptr || a->n == 0 || (grad && moments && scales), "fpwl_moments_fixed: null grad / scales / moments");
  return moments_common(a, grad, grad_stride, nullptr, scales, moments, stream);
}

extern "C" int gnan_fpwl_moments_describe(const gnan_fpwl_args* a, const float* grad, int64_t grad_stride, int32_t fixed,
                                          gnan_fpwl_moments_info* out) {
  GNAN_REQUIRE(out != nullptr, "fpwl_moments describe: null output");
  // (the launchers tell the fixed-point call from the float one by its accumulator pointer: any non-null address, never read)
  static int64_t fixed_mark;
  return moments_common(a, grad, grad_stride, nullptr, nullptr, fixed ? &fixed_mark : nullptr, nullptr, out);
}

// The one-channel kernel and its launcher, compiled into THIS object, behind the kernels above: as an object of its own (or beside
// fpwl_kernel / fpwl_fast_kernel) the very same code took 3-5 % more device time on the searched route of the C4 shape, beside the
// other moment kernels it takes the parent's (profiles/r21_fpwl_split_ab.txt, section 9).
#include "fpwl_moments_c1_body.hpp"
