// What the table look-up kernels share (gfx950): csrc/fpwl.hip (forward, routing), fpwl_fast.hip, fpwl_moments.hip (with
// fpwl_moments_c1_body.hpp), fpwl_index.hip, fpwl_rows.hip and fpwl_input_grad.hip, one object each.  Device side: the kernel
// parameters, the thread map, the two searches (sorted array and skewed breadth-first tree), the XCD-aware workgroup map and the
// epilogues several kernels end with.  Host side: argument checks, the block-size cost model, the launch helpers and the
// declarations of the launchers that cross a file boundary.  Kernels stay in the anonymous namespace of their own file.
#pragma once
#include "common.hpp"

#include <cstdlib>
#include <type_traits>

namespace gnan::fpwl {

struct Params {
  const float* x;
  int64_t n, x_stride;
  int F, C;
  const int32_t* off;
  const float* anchor;
  const float* val;
  const float* slope;
  int step0;        // largest power of two <= max breakpoints per feature (0 if none)
  int n_groups;
  int nodes_per_block;
  int sum_features;
  int vec_x, vec_out;
  float* out;
  int64_t out_stride;
  double* col_partial;   // optional [gridDim.x, F]: per-workgroup column sums of the output (FAST, per-feature mode)
  int out_bf16;          // per-feature output stored as bf16 rows (FAST path only)
  uint8_t* piece_out;    // optional [n, F] (fast feature-sum kernel): the piece of every (node, feature) within its feature,
                         // kept for gnan_fpwl_moments_fixed(piece_in) — the backward pass then skips the search
  const uint8_t* piece_in;
  int64_t total_rows;    // column sums cover nodes [0, total_rows) only
  int max_pieces;        // largest piece count of one feature
  int max_group_pieces;  // largest piece count of one feature group
  int piece_stride;      // fpwl_moments_c1_kernel over kept pieces: bins of piece j of the group's feature f at [j * FG + f] (even, >= max_pieces)
  int soff_offset;       // tree kernels: float offset of the group-offset array in dynamic LDS
  int acc_offset;        // > 0 (sum over features, C > 1): float offset in dynamic LDS of the [C][NODES] accumulators;
                         // the workgroup then owns ONE pass of nodes and walks all feature groups for them
};

struct MomentParams {
  Params f;            // x, tables, grouping as in the forward (val / slope / out unused)
  const float* g;      // upstream gradient: [n, F*C] (per feature) or [n, C] (sum_features)
  int64_t g_stride;
  float* M;            // [T, 2, C], zeroed by the caller
  // fixed-point mode (FIXED): LDS float atomics run at ~200 G/s on gfx950 (a compare-and-swap loop), integer ones at
  // ~2500 G/s (tools/lds_atomic_rate.hip), so the bins hold round(v * 2^e) in 64-bit integers: 12x cheaper to update,
  // and — integer addition being associative — bit-reproducible.  scales = {2^e0, 2^e1} for M0 / M1 terms.
  const double* scales;
  unsigned long long* Mi;   // [T, 2, C] two's-complement sums, zeroed by the caller
  int vec_g;                // gradient rows may be read as 16-byte quads (C == 1, per-feature gradient)
  int general_only;         // GNAN_FPWL_MOMENTS_GENERAL: keep the general kernel where the one-channel kernel applies
};

// LDS row strides of the per-piece tables: an odd number of words per piece for C > 1.  The threads of a wavefront
// read channel c of DIFFERENT pieces (thread = node), i.e. addresses `piece * stride + c`: with stride = C = 40 those
// fall on 4 of the 32 banks (16-way conflicts; C = 32: one bank), and the 64-bit bins of the moment kernels, stride 2 C
// quad-words, on a single bank pair.  arxiv-shaped C = 40: look-up 2.33 -> 2.30 ms, moments 4.5 -> 4.0 ms (the structure, not the conflicts, was the bound: fpwl_rows.hip).
__host__ __device__ __forceinline__ int table_stride(int C) { return C > 1 ? (C | 1) : 1; }          // floats per (val | slope) row
__host__ __device__ __forceinline__ int bin_stride(int C) { return C > 1 ? 2 * C + 1 : 2; }          // bins per piece: [2][C] (+ 1)

// Thread = (node, feature quad): FPT = min(FG, 4) features per thread, TPN = FG / FPT threads per node, so a
// node's FG x values are one contiguous 16-B load per thread (a 64-B sector per node for FG = 16), the
// per-thread state is a handful of registers (8 waves/SIMD), and every thread runs FPT independent searches.
template <int FG, int BS = 256>
struct Map {
  static constexpr int FPT = FG < 4 ? FG : 4;
  static constexpr int TPN = FG / FPT;
  static constexpr int NODES = BS / TPN;  // nodes per workgroup pass
};

// Piece of feature f (group-relative, LDS tables): i = #{ j in 1..pn : anchor[po + j] <= x }, searched for
// the thread's FPT features in lock-step (FPT independent LDS reads per step).
template <int FPT>
__device__ __forceinline__ void search(const float* anchor_l, const int (&po)[FPT], const int (&pn)[FPT],
                                       const float (&xv)[FPT], int step0, int (&idx)[FPT]) {
#pragma unroll
  for (int f = 0; f < FPT; ++f) idx[f] = 0;
  for (int step = step0; step > 0; step >>= 1) {
#pragma unroll
    for (int f = 0; f < FPT; ++f) {
      const int j = idx[f] + step;
      const int jj = j <= pn[f] ? j : 0;  // out of range -> harmless in-range read
      const float a = anchor_l[po[f] + jj];
      idx[f] = (j <= pn[f] && a <= xv[f]) ? j : idx[f];
    }
  }
#pragma unroll
  for (int f = 0; f < FPT; ++f) idx[f] += po[f];
}

__device__ __forceinline__ unsigned bf16_bits(float f) {      // round-to-nearest-even, as torch.bfloat16
  const unsigned u = __float_as_uint(f);
  return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}

// Four values as one 8-byte store of bf16; returns what was stored, as floats: column sums must describe the operand the
// aggregation will actually read, the rounded values.
__device__ __forceinline__ float4 store_bf16_quad(uint16_t* o16, const float4 t) {
  const unsigned b0 = bf16_bits(t.x), b1 = bf16_bits(t.y), b2 = bf16_bits(t.z), b3 = bf16_bits(t.w);
  *reinterpret_cast<uint2*>(o16) = make_uint2(b0 | (b1 << 16), b2 | (b3 << 16));
  return make_float4(__uint_as_float(b0 << 16), __uint_as_float(b1 << 16), __uint_as_float(b2 << 16), __uint_as_float(b3 << 16));
}

// round(v * s) as a two's-complement 64-bit integer for a power of two s and |v * s| < 2^51: one fused multiply-add onto
// 1.5 * 2^52 leaves the integer in the low mantissa bits (round to nearest even, like __double2ll_rn, whose library
// routine costs ~10 float64 instructions — v_rndne, v_ldexp, v_floor, v_fma, two conversions).  gnan_fpwl_moment_scales
// caps its exponents so that every term stays below 2^50.
__device__ __forceinline__ unsigned long long fixed_bits_d(double v, double s) {
  const double d = fma(v, s, 6755399441055744.0);
  return static_cast<unsigned long long>(__double_as_longlong(d)) - 0x4338000000000000ull;
}
__device__ __forceinline__ unsigned long long fixed_bits(float v, double s) { return fixed_bits_d(static_cast<double>(v), s); }

// reads at raw LDS byte addresses (LDS base folded in once per group): addressing through the `smem` symbol costs a fourth
// instruction per search step, because its base is only resolved at link time
typedef __attribute__((address_space(3))) const float lds_cfloat;
typedef float f32x2_t __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) const f32x2_t lds_cfloat2;
__device__ __forceinline__ float lds_f32(int addr) { return *reinterpret_cast<lds_cfloat*>(static_cast<uintptr_t>(static_cast<unsigned>(addr))); }
__device__ __forceinline__ float2 lds_f32x2(int addr) {
  const f32x2_t v = *reinterpret_cast<lds_cfloat2*>(static_cast<uintptr_t>(static_cast<unsigned>(addr)));
  return make_float2(v.x, v.y);
}
__device__ __forceinline__ unsigned lds_address(float* smem) {
  return static_cast<unsigned>(reinterpret_cast<uintptr_t>((__attribute__((address_space(3))) float*)smem));
}

// ---------------------------------------------------------------------------------------------
// The tree search of the one-channel kernels.  Every feature's anchors sit in LDS as a complete search TREE in breadth-first
// (Eytzinger) order, padded to P2 = 2^NSTEP - 1 nodes: the 2^s nodes of level s are 2^s consecutive words, i.e. 2^s distinct
// banks up to level 5, and there is no bounds test in the loop.  The node is carried as an LDS *byte address* a = Q + 4k (Q: tree
// of the thread's first feature; the other three trees are reached through the immediate offset of the ds_read), so a step is
//     t = lds[a];  a = 2a + (t <= x ? 4 - Q : -Q)            (compare, select, shift-add: 3 vector instructions)
// and after NSTEP steps k - P2 is the piece.
// ---------------------------------------------------------------------------------------------
// Sorted index of node k (1 <= k < 2^NSTEP) of the complete breadth-first tree over the sorted entries 1 .. 2^NSTEP - 1.
template <int NSTEP>
__device__ __forceinline__ int tree_sorted_index(int k) {
  const int l = 31 - __clz(k);                       // level of the node, root = 0
  return (2 * (k - (1 << l)) + 1) << (NSTEP - 1 - l);
}

// Words of skew between the trees of consecutive feature QUADS.  One ds_read of the search serves the four quads of a
// wave (lane = (node, quad)), i.e. four different trees; were the trees aligned alike, their level-s nodes would share
// banks and every level would be a 4-way conflict (SQ_LDS_BANK_CONFLICT: 68 % of the kernel's LDS cycles).  With 8 words
// of skew the nodes of levels 0-3 of the four trees fall on 32 distinct banks and level 4 on each bank twice.
constexpr int kTreeSkew = 8;

// Words of the trees of one group of fg features (even: what lies behind them is 8-byte aligned).
__host__ __device__ constexpr int tree_words(int fg, int nstep) { return (fg << nstep) + (fg / 4) * kTreeSkew; }

// The trees of a group into LDS: feature f's at smem + f * P2 (+ skew), its anchors at anchor[base + s_off[f] ...).
template <int FG, int NSTEP, int BS>
__device__ __forceinline__ void build_trees(float* smem, const int* s_off, const float* anchor, int base) {
  constexpr int P2 = 1 << NSTEP;
  for (int i = threadIdx.x; i < FG * P2; i += BS) {
    const int f = i >> NSTEP, k = i & (P2 - 1);
    float v = __builtin_nanf("");          // padding: NaN <= x is false for EVERY x (+inf <= +inf would be true)
    if (k) {
      const int j = tree_sorted_index<NSTEP>(k);
      if (j < s_off[f + 1] - s_off[f]) v = anchor[base + s_off[f] + j];
    }
    smem[i + (f / 4) * kTreeSkew] = v;
  }
}

// Q: LDS byte address of the tree of quad q's first feature; nQ = -Q and nQ4 = 4 - Q in two opaque registers, which keeps
// the step at compare, select, shift-add.
struct TreeBase { int Q, nQ, nQ4; };
template <int NSTEP>
__device__ __forceinline__ TreeBase tree_base(unsigned lds_base, int q) {
  TreeBase t;
  t.Q = static_cast<int>(lds_base) + q * ((4 * (1 << NSTEP) + kTreeSkew) * 4);
  t.nQ = -t.Q;
  t.nQ4 = 4 - t.Q;
  asm volatile("" : "+v"(t.nQ), "+v"(t.nQ4));
  return t;
}

// The descent for the thread's four features in lock-step; a[f] ends at the tree address Q + 4 (P2 + piece).  (t by value: by
// reference every step compiled to the inverted compare.)  fpwl_moments_c1_kernel and fpwl_locate_tree_kernel, which also keep the
// last entry stepped right at (the piece's anchor), have their descent, tree base, tree build and block map written out: through
// these helpers their code was not the parent's (profiles/r21_fpwl_split_code_objects.txt).
template <int NSTEP>
__device__ __forceinline__ void tree_search(const TreeBase t, const float (&xv)[4], int (&a)[4]) {
  constexpr int P2 = 1 << NSTEP;
#pragma unroll
  for (int f = 0; f < 4; ++f) a[f] = t.Q + 4;       // node 1 = root
#pragma unroll
  for (int step = 0; step < NSTEP; ++step) {
#pragma unroll
    for (int f = 0; f < 4; ++f) {
      const float e = lds_f32(a[f] + f * (P2 * 4));
      a[f] = (a[f] << 1) + (e <= xv[f] ? t.nQ4 : t.nQ);
    }
  }
}

// Workgroup id -> (node block, feature group).  Linear workgroup ids go round-robin over the 8 XCDs, so (id % 8) picks the XCD
// and, inside it, the groups of one node block are adjacent in time: they read different 64-B sectors of the same x rows, whose
// 128-B lines are fetched into that XCD's L2 once.  Launches round the node blocks up to a multiple of 8.
__device__ __forceinline__ void xcd_block(int64_t id, int n_groups, int64_t& nb, int& grp) {
  grp = static_cast<int>((id >> 3) % n_groups);
  nb = ((id >> 3) / n_groups) * 8 + (id & 7);
}

// Column sums of a workgroup's output in fixed order: thread = (node slot, quad) holds ps[4], NODES node slots per feature are
// added in float64 into col_partial[nb, k0 + feature].  `red`: BS * 4 floats of LDS that are dead by now.
template <int FG, int BS>
__device__ __forceinline__ void block_column_sums(float* red, const float (&ps)[4], double* col_partial, int64_t nb, int F, int k0) {
  constexpr int FPT = 4, TPN = FG / FPT, NODES = BS / TPN;
  const int tid = threadIdx.x;
  __syncthreads();
#pragma unroll
  for (int f = 0; f < FPT; ++f) red[tid * FPT + f] = ps[f];
  __syncthreads();
  if (tid < FG) {
    const int qq = tid / FPT, ff = tid % FPT;
    double acc = 0.0;
    for (int s2 = 0; s2 < NODES; ++s2) acc += red[(s2 * TPN + qq) * FPT + ff];
    col_partial[nb * F + k0 + tid] = acc;
  }
}

// The bins of a workgroup ([tot] rows of Rb, [2][C] used) onto the global moments: one atomic per touched bin.
template <int BS, class bin_t>
__device__ __forceinline__ void flush_bins(const bin_t* bins, int tot, int C, int Rb, bin_t* out) {
  for (int i = threadIdx.x; i < tot * 2 * C; i += BS) {
    const bin_t v = bins[(i / (2 * C)) * Rb + i % (2 * C)];
    if (v != bin_t(0)) atomicAdd(out + i, v);
  }
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
constexpr size_t kMaxLds = 150 * 1024;     // what one workgroup's image may take of the CU's 160 KB

inline int nstep_of(int max_pieces) {      // tree depth: 2^nstep >= max_pieces, at least 6
  int nstep = 6;
  while ((1 << nstep) < max_pieces) ++nstep;
  return nstep;
}
inline int step0_of(int max_pieces) {      // sorted-array search: largest power of two <= max breakpoints per feature (0 if none)
  int step0 = 0;
  while ((step0 ? step0 * 2 : 1) <= max_pieces - 1) step0 = step0 ? step0 * 2 : 1;
  return step0;
}

// f(std::integral_constant<int, NSTEP>) for the tree depths the kernels are built for; callers check nstep <= 10 first.
template <class Fn>
auto by_nstep(int nstep, Fn&& f) {
  switch (nstep) {
    case 6: return f(std::integral_constant<int, 6>{});
    case 7: return f(std::integral_constant<int, 7>{});
    case 8: return f(std::integral_constant<int, 8>{});
    case 9: return f(std::integral_constant<int, 9>{});
    default: return f(std::integral_constant<int, 10>{});
  }
}

// Over 64 KB of dynamic LDS a kernel needs its attribute raised; then launch and check.
template <class Kernel, class P>
int launch_with_lds(Kernel kernel, const char* name, dim3 grid, int bs, size_t lds, hipStream_t st, const P& params) {
  if (lds > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       static_cast<int>(lds));
    if (e != hipSuccess) return gnan::fail(GNAN_ERR_HIP, "%s: hipFuncSetAttribute: %s", name, hipGetErrorString(e));
  }
  hipLaunchKernelGGL(kernel, grid, dim3(bs), lds, st, params);
  return gnan::check_launch(name);
}

// Nodes per workgroup along the node axis.  A workgroup first loads the LDS image of its feature group (worth `overhead`
// look-up rows: ~300 for a 16-feature group of the forward, ~600 for the one-channel moments, which also flush their bins), so
// blocks should be large; the L2 sharing of x lines between the groups of a node block wants them <= 4096 (measured on C4: 2048
// +6 %, 8192 +2 %, 16384 +7 %); and the grid should be a whole number of rounds of the workgroups the chip holds at once
// (LDS-limited: 3 per CU for 16-feature groups), which matters for shares of a few million rows (2.7M rows: 5.04 rounds of
// 2816-node blocks -> 4 rounds of 3584-node blocks, -15 %).  Small batches: ~1024 blocks of 256..4096 nodes.
inline int small_batch_block(int64_t n) {
  const int64_t npb = (n / 1024 + 255) / 256 * 256;
  return static_cast<int>(npb < 256 ? 256 : (npb > 4096 ? 4096 : npb));
}
inline int64_t resident_workgroups(size_t lds, int bs) {
  int per_cu = static_cast<int>((160 * 1024) / lds);
  if (per_cu > 2048 / bs) per_cu = 2048 / bs;
  if (per_cu < 1) per_cu = 1;
  return static_cast<int64_t>(gnan::cu_count()) * per_cu;
}
// The block size in [lo, hi] (steps of `unit`) with the fewest rounds x (block + overhead); ties go to the larger block.
// xcd_rounds: the launch rounds its node blocks up to a multiple of 8 (xcd_block) and the model counts them so.
inline int tuned_block(int64_t n, int64_t groups, int64_t resident, int lo, int hi, int unit, int overhead, bool xcd_rounds = false) {
  int64_t best_cost = -1;
  int best = lo;
  for (int npb = lo; npb <= hi; npb += unit) {
    const int64_t nbl = (n + npb - 1) / npb;
    const int64_t wgs = (xcd_rounds ? (nbl + 7) / 8 * 8 : nbl) * groups;
    const int64_t rounds = (wgs + resident - 1) / resident;
    const int64_t cost = rounds * (npb + overhead);
    if (best_cost < 0 || cost < best_cost || (cost == best_cost && npb > best)) { best_cost = cost; best = npb; }
  }
  return best;
}

// fpwl_moments_c1_kernel and fpwl_locate_tree_kernel: the image (trees + 64-bit bins) is zeroed / built at the start and
// flushed with one global atomic per touched bin at the end — worth ~600 rows — and x lines are shared between the
// groups of a node block in L2, so blocks of 1024..8192 nodes in whole rounds of the resident workgroups.
// (the same model from 16k nodes on: the arxiv-shaped graph, 169k nodes x 9 groups, ran 5958 workgroups of 256 nodes, each
//  paying the ~600 rows of image and flush: 70 % overhead and 25M global atomics onto 37k bins; one round of ~750 workgroups
//  of 2048 nodes instead)
inline int tuned_moment_block(int64_t n, int n_groups, size_t lds, int bs) {
  if (n < 16384) return small_batch_block(n);
  return tuned_block(n, n_groups, resident_workgroups(lds, bs), n < 262144 ? 256 : 1024, 8192, 128, 600);
}

inline int tuned_nodes_per_block(const gnan_fpwl_args* a, int n_groups) {
  const int fg = a->features_per_group;
  if (a->C != 1 || fg < 4 || a->n < 262144) return small_batch_block(a->n);     // general kernel / small inputs
  const size_t lds = (static_cast<size_t>(fg) << nstep_of(a->max_pieces)) * 4 + static_cast<size_t>(a->max_group_pieces) * 12 + 128;
  const int64_t groups = a->sum_features ? 1 : n_groups;   // feature-sum mode walks its groups inside one workgroup
  return tuned_block(a->n, groups, resident_workgroups(lds, fg >= 8 ? 512 : 256), 1024, 4096, 128, 300);
}

inline int common_checks(const gnan_fpwl_args* a) {
  GNAN_REQUIRE(a != nullptr, "fpwl: null args");
  GNAN_REQUIRE(a->n >= 0 && a->F >= 1 && a->C >= 1, "fpwl: bad sizes");
  if (a->n == 0) return GNAN_OK;
  GNAN_REQUIRE(a->x && a->off && a->anchor, "fpwl: null pointer");
  GNAN_REQUIRE(a->x_stride >= a->F, "fpwl: x row stride smaller than F");
  GNAN_REQUIRE(a->max_pieces >= 1 && a->max_group_pieces >= 1, "fpwl: max_pieces / max_group_pieces must be >= 1");
  const int fg = a->features_per_group;
  GNAN_REQUIRE(fg == 1 || fg == 2 || fg == 4 || fg == 8 || fg == 16, "fpwl: features_per_group must be 1, 2, 4, 8 or 16");
  const size_t lds = static_cast<size_t>(a->max_group_pieces) * (1 + 2 * static_cast<size_t>(table_stride(a->C))) * sizeof(float);
  if (lds > kMaxLds)
    return gnan::fail(GNAN_ERR_UNSUPPORTED, "fpwl: %zu B of tables per feature group exceed LDS; use fewer features per group",
                      lds);
  return GNAN_OK;
}

inline Params base_params(const gnan_fpwl_args* a) {
  Params p;
  p.x = a->x; p.n = a->n; p.x_stride = a->x_stride; p.F = a->F; p.C = a->C;
  p.off = a->off; p.anchor = a->anchor; p.val = a->val; p.slope = a->slope;
  p.step0 = step0_of(a->max_pieces);
  p.n_groups = (a->F + a->features_per_group - 1) / a->features_per_group;
  p.nodes_per_block = tuned_nodes_per_block(a, p.n_groups);
  p.sum_features = a->sum_features;
  p.vec_x = p.vec_out = 0;
  p.out = static_cast<float*>(a->out); p.out_stride = a->out_stride;
  p.col_partial = nullptr;
  p.max_pieces = a->max_pieces;
  p.max_group_pieces = a->max_group_pieces;
  p.piece_stride = 0;
  p.soff_offset = 0;
  p.total_rows = (a->total_rows > 0 && a->total_rows < a->n) ? a->total_rows : a->n;
  p.acc_offset = 0;
  p.out_bf16 = a->out_dtype == GNAN_BF16;
  p.piece_out = a->piece_out; p.piece_in = a->piece_in;
  return p;
}

// What a moment launcher tells gnan_fpwl_moments_describe: every launcher takes `probe` and, when it is set, fills it where it would
// otherwise set the kernel's attributes and launch (so the query reports the launch's own decisions, the LDS fall-backs included).
inline void fill_probe(gnan_fpwl_moments_info* probe, int kernel, int nstep, const Params& p, int nodes, int bs, bool kept, size_t lds) {
  *probe = gnan_fpwl_moments_info{};
  probe->kernel = kernel; probe->nstep = nstep; probe->nodes_per_block = p.nodes_per_block; probe->nodes_per_round = nodes;
  probe->block_size = bs; probe->pieces_kept = kept; probe->channel_chunk = p.C; probe->n_chunks = 1;
  probe->lds_bytes = static_cast<int32_t>(lds);
  probe->n_blocks = (p.n + p.nodes_per_block - 1) / p.nodes_per_block;
}

// ---------------------------------------------------------------------------------------------
// launchers that cross a file boundary (ordinary functions; the library's version script keeps them local)
// ---------------------------------------------------------------------------------------------
// csrc/fpwl_fast.hip: fpwl_fast_kernel for groups of fg features and bs threads, depth nstep <= 10; p.soff_offset and lds
// (trees + tables + offsets, or the column-sum scratch if larger) are the caller's (csrc/fpwl.hip: launch).
int launch_fast(const Params& p, int fg, int bs, int nstep, bool ragged, int64_t wgs, size_t lds, hipStream_t st);
// csrc/fpwl_moments_c1_body.hpp: fpwl_moments_c1_kernel; -1: its image exceeds LDS, the caller (csrc/fpwl_moments.hip) falls back
int launch_moments_c1(const MomentParams& mp, int fg, int bs, int nstep, bool ragged, hipStream_t st, gnan_fpwl_moments_info* probe);
// csrc/fpwl_index.hip: the direct-index look-up (one channel, whole 16-feature groups, aligned rows), routed by gnan_fpwl_fwd
bool index_applies(const gnan_fpwl_args* a);
int index_nodes_per_block(const gnan_fpwl_args* a);
int index_fwd(const gnan_fpwl_args* a, double* col_partial, hipStream_t st);   // col_partial: [node blocks][F] doubles or NULL
size_t index_sum_workspace_bytes(const gnan_fpwl_args* a);

}  // namespace gnan::fpwl
