// The C == 1 work-horse of the table look-up (gfx950); routed by csrc/fpwl.hip.
//
// Two things bound the plain kernel (fpwl_kernel, csrc/fpwl.hip): vector instructions (68 per look-up, counted with
// SQ_INSTS_VALU) and LDS bank conflicts of the binary search (level s of a search over a sorted array probes 2^s
// addresses that are 2^(NSTEP-s) words apart: with 32 banks for ds_read_b32 that is one or two banks for every level
// but the last two, i.e. up to 8-way conflicts).  This variant searches the skewed breadth-first trees of
// csrc/fpwl_common.hpp (3 vector instructions per step, no bounds test); after NSTEP steps k - P2 is the piece: its anchor
// sits in a compact array at a + dA[f] and (val, slope) is one 8-byte read at 2 (a + dA[f]) + const.
// Same piece and same arithmetic per look-up as fpwl_kernel (val + slope * (x - anchor)), hence bit-identical results.
#include "fpwl_common.hpp"

namespace {
using namespace gnan::fpwl;

// LDS image of one feature group: [FG][P2] tree words (+ kTreeSkew words per quad), [tot] (val, slope) pairs, [tot] anchors
// in piece order.
template <int FG, int NSTEP, int BS>
__device__ __forceinline__ void load_tree_tables(const Params& p, float* smem, const int* s_off, int base, int tot) {
  const int tid = threadIdx.x;
  build_trees<FG, NSTEP, BS>(smem, s_off, p.anchor, base);
  constexpr int kTreeWords = tree_words(FG, NSTEP);
  float2* vs_l = reinterpret_cast<float2*>(smem + kTreeWords);
  float* an_l = smem + kTreeWords + 2 * tot;
  for (int i = tid; i < tot; i += BS) {
    vs_l[i] = make_float2(p.val[base + i], p.slope[base + i]);
    an_l[i] = p.anchor[base + i];
  }
}

// SUM: out[n] = sum over features (f_sums, GNAN.py:157); OUT16 (per-feature output only): store bf16 rows — the operand format
// of the bf16-storage aggregation.
// RAGGED (feature-sum mode only): F need not be a multiple of FG and the rows of x need not be 16-byte aligned — the
// reference's inputs are raw features + a ones column (129, 1434: pre_process_datasets.py:108), which sent every real
// feature matrix below the padding threshold to the general kernel (arxiv-shaped: 0.109 ms against ~0.05 ms).
// The last group is partial: its missing features get empty (NaN) trees, their x is not read and their terms are dropped.
template <int FG, bool SUM, bool OUT16, int NSTEP, int BS, bool RAGGED = false>
__global__ __launch_bounds__(BS) void fpwl_fast_kernel(const Params p) {
  static_assert(FG % 4 == 0, "feature quads");
  static_assert(!RAGGED || (SUM && !OUT16), "ragged feature counts: feature-sum mode");
  constexpr int FPT = 4, TPN = FG / FPT, NODES = BS / TPN, P2 = 1 << NSTEP;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  int* s_off = reinterpret_cast<int*>(smem) + p.soff_offset;       // [FG + 1], behind the tables
  const unsigned lds_base = lds_address(smem);
  const int tid = threadIdx.x;
  const int q = tid % TPN;
  const int nl = tid / TPN;
  int64_t nb = blockIdx.x;
  int g_first = 0;
  if (!SUM) xcd_block(blockIdx.x, p.n_groups, nb, g_first);
  const int64_t n_lo = nb * p.nodes_per_block;
  if (n_lo >= p.n) return;
  const int64_t n_hi = n_lo + p.nodes_per_block < p.n ? n_lo + p.nodes_per_block : p.n;
  const int g_lo = SUM ? 0 : g_first;
  const int g_hi = SUM ? p.n_groups : g_lo + 1;
  constexpr int kTreeBytes = tree_words(FG, NSTEP) * 4;   // (val, slope) pairs start behind the trees, the anchors behind them

  for (int g = g_lo; g < g_hi; ++g) {
    const int k0 = g * FG;
    const int nf = RAGGED ? (p.F - k0 < FG ? p.F - k0 : FG) : FG;     // live features of the group
    const int base = p.off[k0];
    const int tot = p.off[k0 + nf] - base;
    __syncthreads();                                // previous group's look-ups are done with the LDS tables
    if (tid <= FG) s_off[tid] = p.off[k0 + (tid < nf ? tid : nf)] - base;
    __syncthreads();
    load_tree_tables<FG, NSTEP, BS>(p, smem, s_off, base, tot);
    __syncthreads();
    const TreeBase tb = tree_base<NSTEP>(lds_base, q);
    const int Q = tb.Q;
    const int vs_minus_2an = static_cast<int>(lds_base) + kTreeBytes - 2 * (static_cast<int>(lds_base) + kTreeBytes + 8 * tot);
    int dA[FPT];
#pragma unroll
    for (int f = 0; f < FPT; ++f)
      dA[f] = static_cast<int>(lds_base) + kTreeBytes + 8 * tot + 4 * s_off[q * FPT + f] - 4 * P2 - Q;

    float ps[FPT] = {0.f, 0.f, 0.f, 0.f};           // column sums of the output (per-feature mode)
    bool live[FPT];
#pragma unroll
    for (int f = 0; f < FPT; ++f) live[f] = !RAGGED || q * FPT + f < nf;
    for (int64_t n = n_lo + nl; n < n_hi; n += NODES) {
      float xv[FPT];
      if constexpr (RAGGED) {
        const float* xr = p.x + n * p.x_stride + k0 + q * FPT;
#pragma unroll
        for (int f = 0; f < FPT; ++f) xv[f] = live[f] ? xr[f] : 0.f;
      } else {
        const float4 t = *reinterpret_cast<const float4*>(p.x + n * p.x_stride + k0 + q * FPT);
        xv[0] = t.x; xv[1] = t.y; xv[2] = t.z; xv[3] = t.w;
      }
      int a[FPT];
      tree_search<NSTEP>(tb, xv, a);
      float y[FPT];
#pragma unroll
      for (int f = 0; f < FPT; ++f) {
        const int pa = a[f] + dA[f];
        const float an = lds_f32(pa);
        const float2 vs = lds_f32x2(2 * pa + vs_minus_2an);
        y[f] = fmaf(vs.y, xv[f] - an, vs.x);
      }
      if constexpr (SUM) {
        if (p.piece_out) {                          // (uniform) keep the pieces for the backward pass: one byte per look-up
          // group-major [n_groups][n][FG]: the pass over a feature group writes one contiguous FG-byte run per node (node-
          // major [n, F] rows got a quarter of every line per pass: the stores doubled the kernel's time)
          unsigned packed = 0u;
#pragma unroll
          for (int f = 0; f < FPT; ++f) packed |= static_cast<unsigned>(((a[f] - Q) >> 2) - P2) << (8 * f);
          *reinterpret_cast<unsigned*>(p.piece_out + (static_cast<int64_t>(g) * p.n + n) * FG + q * FPT) = packed;
        }
        float acc = 0.f;
#pragma unroll
        for (int f = 0; f < FPT; ++f) acc += (!RAGGED || live[f]) ? y[f] : 0.f;
#pragma unroll
        for (int off = 1; off < TPN; off <<= 1) acc += __shfl_xor(acc, off);   // the node's TPN threads
        if (q == 0) {                               // groups run one after the other and a node keeps its thread
          float* o = p.out + n * p.out_stride;
          o[0] = g == 0 ? acc : o[0] + acc;
        }
      } else {
        float4 r = make_float4(y[0], y[1], y[2], y[3]);
        if constexpr (OUT16) {
          r = store_bf16_quad(reinterpret_cast<uint16_t*>(p.out) + n * p.out_stride + (k0 + q * FPT), r);
        } else {
          *reinterpret_cast<float4*>(p.out + n * p.out_stride + k0 + q * FPT) = r;
        }
        if (n < p.total_rows) { ps[0] += r.x; ps[1] += r.y; ps[2] += r.z; ps[3] += r.w; }
      }
    }
    if constexpr (!SUM) {
      // the tables are dead by now: the scratch takes their place (the host sizes LDS for both)
      if (p.col_partial) block_column_sums<FG, BS>(smem, ps, p.col_partial, nb, p.F, k0);
    }
  }
}

template <int FG, int BS>
int launch_fast_groups(const Params& p, int nstep, bool ragged, int64_t wgs, size_t lds, hipStream_t st) {
  return by_nstep(nstep, [&](auto ns) {
    constexpr int NS = decltype(ns)::value;
    auto go = [&](auto kernel) { return launch_with_lds(kernel, "fpwl_fast_kernel", dim3(static_cast<unsigned>(wgs)), BS, lds, st, p); };
    if (p.out_bf16) return p.sum_features ? gnan::fail(GNAN_ERR_UNSUPPORTED, "fpwl: bf16 output is per-feature only")
                                          : go(fpwl_fast_kernel<FG, false, true, NS, BS>);
    if (ragged) return go(fpwl_fast_kernel<FG, true, false, NS, BS, true>);
    return p.sum_features ? go(fpwl_fast_kernel<FG, true, false, NS, BS>) : go(fpwl_fast_kernel<FG, false, false, NS, BS>);
  });
}

}  // namespace

// The workgroups csrc/fpwl.hip plans for one output channel: 256 threads for groups of 4 features, 512 for 8 and 16.  (Its
// 512- and 1024-thread workgroups for groups of 4 serve the feature sum over SEVERAL channels only, which this kernel never is.)
int gnan::fpwl::launch_fast(const Params& p, int fg, int bs, int nstep, bool ragged, int64_t wgs, size_t lds, hipStream_t st) {
  if (fg == 4 && bs == 256) return launch_fast_groups<4, 256>(p, nstep, ragged, wgs, lds, st);
  if (fg == 8 && bs == 512) return launch_fast_groups<8, 512>(p, nstep, ragged, wgs, lds, st);
  if (fg == 16 && bs == 512) return launch_fast_groups<16, 512>(p, nstep, ragged, wgs, lds, st);
  return gnan::fail(GNAN_ERR_UNSUPPORTED, "fpwl: no fast kernel for groups of %d features in workgroups of %d threads", fg, bs);
}
