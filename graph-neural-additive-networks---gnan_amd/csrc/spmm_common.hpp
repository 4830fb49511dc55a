// What the aggregation's translation units share (csrc/spmm.hip, csrc/spmm_fwd_body.hpp and its spmm_fwd_v*.hip objects,
// csrc/spmm_grad.hip): the kernels' argument record, operand and index loads, the weight tables, the hub-row slice steps that
// every kernel family takes, and the host side's validation and tiling.  Everything sits in the anonymous namespace (every
// object has its own copy, the kernels' mangled names carry it), so no kernel is defined here: a kernel lives in one .hip file.
#pragma once
#include "common.hpp"

#include <cstdlib>
#include <type_traits>

namespace {

using gnan::kWave;

struct Params {
  int64_t n_rows, n_cols;
  int64_t nnz;     // listed pairs (length of col / code), 0 = unknown: index runs are then read entry by entry
  const void* rowptr;
  int rowptr_is64;
  const int32_t* col;
  const uint8_t* code;
  const int32_t* row_ids;
  const void* S;   // fp32 rows, or bf16 rows when the kernels are instantiated with VEC == 8
  int W;
  int64_t s_stride;
  const float* lut;
  int64_t lut_row_stride;
  int D, Cw;
  const int32_t* cnt;
  int64_t cnt_stride;
  const float* s_total;
  int weight_by_col, minus_rest;
  int reduce_cr;  // > 0: store only the per-channel sums over columns w = c (mod reduce_cr)
  int scatter_out;  // output row q is stored at Y[row_ids[q]] (rows are PROCESSED in row_ids order, e.g. by degree)
  int s_by_code;    // the operand row of pair (i, c, d) is S[c * D + d]: one pre-weighted row per (node, hop code)
  int packed;       // col entries carry the hop code in their top kPackBits bits (code is not read)
  float* Y;
  int64_t y_stride;
  int64_t long_threshold;
  const int32_t* long_rows;
  const int32_t* long_slice_ptr;
  int n_long, n_slices, slice_edges;
  float* partial;  // [n_slices, 2, W]
  int64_t hot_lo;  // spmm_hot_kernel: operand rows [hot_lo, hot_lo + hot_n) are served from an LDS copy
  int hot_n;
  float* shell_out;  // [n_rows, D - 1] raw per-code sums of the operand over the row's pairs (W == 1, small-D route, a lane per row)
  // classed hub plan (gnan_spmm_args.cls_*): each wave of a slice workgroup takes one slice of the plan-owned packed index
  const int32_t* cls_index;
  const int64_t* cls_slice_start;
  const int32_t* cls_slice_row;
  const int32_t* cls_slot_slice;
  int cls_n_slots;
  int n_slice_blocks;  // workgroups in front of the row blocks: n_slices, or 8 ceil(queue / 4) with the classed plan (a wave per slice)
  // short-row tiles (gnan_spmm_args.short_*), set by launch() where the route serves the call: the n_tile_blocks workgroups behind
  // the slice blocks take the runs of rows of L = 0 .. short_lmax pairs, a tile per wave (tile t of the launch is tile
  // t - short_tile[L] of run L); the row blocks behind them start at row row_q0
  int short_lmax;
  int n_tile_blocks, n_tiles;
  int64_t row_q0;
  int64_t short_row[GNAN_SHORT_LMAX + 2], short_pair[GNAN_SHORT_LMAX + 1];
  int short_tile[GNAN_SHORT_LMAX + 1];
  // the rows' self term from outside (gnan_spmm_args.self_sum): [self_parts][n_rows] by output row, added in the read-out's epilogue
  const float* self_sum;
  int self_parts;
  // classed row segments (gnan_spmm_args.seg_*; the SELF instance alone reads them): rows [seg_q_lo, seg_q_hi) of the sorted copy are
  // taken a (row, column class) segment per lane group by the n_seg_blocks workgroups behind the slice blocks — workgroup b of that
  // range takes class b & 7 — and the row blocks skip them; a segment's float goes to seg_partial[(q - seg_q_lo) * 8 + class]
  const int32_t* seg_index;
  const int64_t* seg_start;
  const int32_t* seg_row;
  const int32_t* cls_seg_ptr;
  const uint8_t* seg_mask;
  float* seg_partial;
  int64_t seg_q_lo, seg_q_hi;
  int n_seg_blocks;
  // blocked hub segments (gnan_spmm_args.hub_*; the SELF instance alone reads them): rows [hub_q_lo, n_rows) are taken a (row, column
  // class, popularity block) segment per lane group by the n_hub_blocks workgroups at the launch's head — workgroup b takes class b & 7,
  // a class's queue is block-major — and neither sliced nor walked; a segment's float goes to hub_partial[hub_seg_slot[s]]
  const int32_t* hub_index;
  const int64_t* hub_seg_start;
  const int32_t* hub_seg_row;
  const int32_t* hub_seg_slot;
  const int32_t* hub_row_slot_ptr;
  const int32_t* hub_cls_seg_ptr;
  float* hub_partial;
  int64_t hub_q_lo;
  int n_hub, n_hub_blocks;
  // the lone rows a thread each (gnan_spmm_args.lone_rows; set by plan_tiles where run 0 is tiled on the SELF route): rows
  // [short_row[0], short_row[0] + lone_n) are spmm_lone_kernel's (csrc/spmm_lone.hip) and tile_lo = short_tile[1] is the first tile
  // that runs.  All three are read on the HOST only: the launch hands spmm_kernel the partition with the tiles numbered from tile_lo
  // (leave_lone_tiles) — read by the kernel, whether as one argument or three, they cost its SELF instances 12 B of scratch
  int lone;        // the request
  int64_t lone_n;
  int tile_lo;
};

__device__ __forceinline__ int64_t load_rowptr(const Params& p, int64_t i) {
  return p.rowptr_is64 ? static_cast<const int64_t*>(p.rowptr)[i]
                       : static_cast<int64_t>(static_cast<const int32_t*>(p.rowptr)[i]);
}

// Processing slot q -> adjacency row (index into rowptr / cnt / a per-row weight table) and output row.
//   no row_ids        : both q                         row_ids, scatter_out 0 : row_ids[q] -> q   (row subset)
//   scatter_out 1     : row_ids[q] -> row_ids[q]       (rows PROCESSED in row_ids order, e.g. by degree, stored in place)
//   scatter_out 2     : q -> row_ids[q]                (the adjacency itself is stored in processing order — a degree-sorted
//                       copy of the CSR — so that rowptr, cnt and the index pairs of neighbouring lane groups are adjacent)
__device__ __forceinline__ int64_t adj_row(const Params& p, int64_t q) {
  return (p.row_ids && p.scatter_out != 2) ? static_cast<int64_t>(p.row_ids[q]) : q;
}
__device__ __forceinline__ int64_t out_row(const Params& p, int64_t q, int64_t i) {
  return p.scatter_out == 2 ? static_cast<int64_t>(p.row_ids[q]) : (p.scatter_out ? i : q);
}

// a_i of gnan_spmm_args.self_sum for output row o: its parts in part order
__device__ __forceinline__ float self_term(const Params& p, int64_t o) {
  float a = p.self_sum[o];
  for (int k = 1; k < p.self_parts; ++k) a += p.self_sum[k * p.n_rows + o];
  return a;
}

template <int VEC>
struct Vec {
  float v[VEC];
};

template <int VEC>
__device__ __forceinline__ Vec<VEC> load_vec(const float* ptr) {
  Vec<VEC> r;
  if constexpr (VEC == 8) {
    const float4 a = *reinterpret_cast<const float4*>(ptr), b = *reinterpret_cast<const float4*>(ptr + 4);
    r.v[0] = a.x; r.v[1] = a.y; r.v[2] = a.z; r.v[3] = a.w; r.v[4] = b.x; r.v[5] = b.y; r.v[6] = b.z; r.v[7] = b.w;
  } else if constexpr (VEC == 4) {
    const float4 t = *reinterpret_cast<const float4*>(ptr);
    r.v[0] = t.x; r.v[1] = t.y; r.v[2] = t.z; r.v[3] = t.w;
  } else if constexpr (VEC == 2) {
    const float2 t = *reinterpret_cast<const float2*>(ptr);
    r.v[0] = t.x; r.v[1] = t.y;
  } else {
    r.v[0] = *ptr;
  }
  return r;
}

// A gathered operand chunk as it sits in registers while the load is in flight: bf16 rows stay packed (4 VGPRs for
// 8 values) until they are consumed, so the in-flight window of the bf16 mode costs no more registers than fp32.
template <int VEC>
struct Raw {
  Vec<VEC> f;
  __device__ __forceinline__ void zero() {
#pragma unroll
    for (int v = 0; v < VEC; ++v) f.v[v] = 0.f;
  }
  __device__ __forceinline__ void load(const void* S, int64_t row, int64_t stride, int col) {
    f = load_vec<VEC>(static_cast<const float*>(S) + row * stride + col);
  }
  __device__ __forceinline__ Vec<VEC> widen() const { return f; }
};

template <>
struct Raw<8> {
  uint4 t;
  __device__ __forceinline__ void zero() { t = make_uint4(0u, 0u, 0u, 0u); }
  __device__ __forceinline__ void load(const void* S, int64_t row, int64_t stride, int col) {
    t = *reinterpret_cast<const uint4*>(static_cast<const uint16_t*>(S) + row * stride + col);
  }
  __device__ __forceinline__ Vec<8> widen() const {
    Vec<8> r;
    const unsigned w[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      r.v[2 * i] = __uint_as_float(w[i] << 16);
      r.v[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
    }
    return r;
  }
};

// Operand rows: fp32 for VEC in {1, 4}; VEC == 8 is the bf16-storage mode (8 bf16 = one 16-B request per lane,
// widened to fp32 in registers; accumulation and output stay fp32).  A chunk that is consumed at once.
template <int VEC>
__device__ __forceinline__ Vec<VEC> load_operand(const void* S, int64_t row, int64_t stride, int col) {
  Raw<VEC> r;
  r.load(S, row, stride, col);
  return r.widen();
}

template <int VEC>
__device__ __forceinline__ void store_vec(float* ptr, const Vec<VEC>& r) {
  if constexpr (VEC == 8) {
    *reinterpret_cast<float4*>(ptr) = make_float4(r.v[0], r.v[1], r.v[2], r.v[3]);
    *reinterpret_cast<float4*>(ptr + 4) = make_float4(r.v[4], r.v[5], r.v[6], r.v[7]);
    return;
  }
  if constexpr (VEC == 4) {
    *reinterpret_cast<float4*>(ptr) = make_float4(r.v[0], r.v[1], r.v[2], r.v[3]);
  } else if constexpr (VEC == 2) {
    *reinterpret_cast<float2*>(ptr) = make_float2(r.v[0], r.v[1]);
  } else {
    *ptr = r.v[0];
  }
}

// Weights of adjacency row i for hop code d, for the VEC columns starting at column w0.
//   wt = lut[i*lrs + d*Cw + (w % Cw)] / max(cnt[i, d], 1)          (IEEE division, as torch.div)
template <int VEC>
__device__ __forceinline__ Vec<VEC> row_weights(const Params& p, int64_t i, int d, int w0) {
  Vec<VEC> w;
  const float* l = p.lut + i * p.lut_row_stride + static_cast<int64_t>(d) * p.Cw;
#pragma unroll
  for (int v = 0; v < VEC; ++v) w.v[v] = l[p.Cw == 1 ? 0 : (w0 + v) % p.Cw];
  if (p.cnt) {
    const int c = p.cnt[i * p.cnt_stride + d];
    const float r = static_cast<float>(c > 1 ? c : 1);
#pragma unroll
    for (int v = 0; v < VEC; ++v) w.v[v] = w.v[v] / r;
  }
  return w;
}

// Weight of one listed pair.  Forward: the table row is the output row i.  Transposed use
// (backward w.r.t. S): the table row is the neighbour c (weight_by_col) and the rest-bucket weight
// is subtracted (minus_rest), because d/dS_j of  wt_rest * (total - sum_listed S)  is  -wt_rest.
template <int VEC>
__device__ __forceinline__ Vec<VEC> edge_weights(const Params& p, int64_t i, int c, int d, int w0) {
  const int64_t r = p.weight_by_col ? static_cast<int64_t>(c) : i;
  Vec<VEC> w = row_weights<VEC>(p, r, d, w0);
  if (p.minus_rest) {
    const Vec<VEC> wr = row_weights<VEC>(p, r, p.D - 1, w0);
#pragma unroll
    for (int v = 0; v < VEC; ++v) w.v[v] -= wr.v[v];
  }
  return w;
}

// Per-row weight cache for the common truncated case (Cw == 1, D <= 4): four registers.  The empty asm statements
// keep the select chain a chain: left alone, the optimiser rewrites it as an indexed load from a 4-float stack array,
// which the backend then places in LDS (8 KB per workgroup and a ds_read + wait per listed pair).
struct SmallW {
  float w[4];
  __device__ __forceinline__ float pick(int d) const {
    float r = w[0];
    r = d == 1 ? w[1] : r;
    asm volatile("" : "+v"(r));
    r = d == 2 ? w[2] : r;
    asm volatile("" : "+v"(r));
    r = d >= 3 ? w[3] : r;
    return r;
  }
};

__device__ __forceinline__ SmallW small_weights(const Params& p, int64_t i) {
  SmallW s;
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    float v = 0.f;
    if (d < p.D) {
      v = p.lut[i * p.lut_row_stride + d];
      if (p.cnt) {
        const int c = p.cnt[i * p.cnt_stride + d];
        v = v / static_cast<float>(c > 1 ? c : 1);
      }
    }
    s.w[d] = v;
  }
  return s;
}

// The end of the combine kernels (spmm_seg_combine_kernel, spmm_hub_combine_kernel, spmm_stream_combine_kernel): row q's sum y of
// listed terms gets the rest and self terms and is stored,   Y[row] = fmaf(w_0 - w_rest, a_i, fmaf(w_rest, T, y))
// T the sum of s_total in float64 rounded once (a float32 chain over W columns would put more roundings on the rest term than a
// 5-pair row's bound counts), a_i as the other epilogues read it.  ONE_CODE (the stream): y is the raw sum of pairs of the one hop
// code `code` and takes their folded weight w_code - w_rest first; else y carries its weights already.  o = out_row(p, q, q) comes
// from the caller, read where each kernel read it before (ahead of the seg and stream kernels' sums, behind the hub kernel's butterfly):
// with the read in here the stream kernel's SGPR count moved.
template <bool ONE_CODE = false>
__device__ __forceinline__ void combine_store(const Params& p, int64_t q, int64_t o, float y, int code = 0) {
  double T = 0.0;
  for (int f = 0; f < p.W; ++f) T += static_cast<double>(p.s_total[f]);
  const int rest = p.D - 1;
  const SmallW sw = small_weights(p, q);
  const float w_rest = sw.pick(rest);
  const float w_self = rest > 0 ? sw.w[0] - w_rest : 0.f;    // (the fold of rows_body)
  if constexpr (ONE_CODE) y = (code < rest ? sw.pick(code) - w_rest : 0.f) * y;
  y = fmaf(w_rest, static_cast<float>(T), y);
  y = fmaf(w_self, self_term(p, o), y);
  p.Y[o * p.y_stride] = y;
}

// A lane's run of N consecutive (col, code) entries as wide loads: N * 4 bytes of column ids (4-byte aligned) and N bytes of
// hop codes (byte aligned; gfx950 runs HSA code in unaligned-access mode) instead of 2 N scalar loads.  With one lane per
// row (W = 1: 16 entries per lane and round) the scalar loads were 32 of the 48 memory instructions of a round, each
// touching ~20 different lines per wavefront.  The caller guarantees e0 + N <= nnz; entries past the row end are read
// (they belong to the next row) and ignored.
// Packed index entries: column id in the low 29 bits, hop code in the top 3 (graphs below 2^29 neighbours, D <= 8).  One
// 4-byte stream instead of a 4-byte and a 1-byte one: the index loads of a lane group are then ONE L2 request per round
// instead of two — 3 % of the W = 64 kernel's requests, 10 % of the bf16 kernel's (8 pairs per round, one request per row).
constexpr int kPackShift = 29;
constexpr unsigned kPackMask = (1u << kPackShift) - 1u;

// (explicit under-aligned vector loads into scalars: routed through __builtin_memcpy into the index arrays, the arrays were
// promoted to LDS — 16 KB per workgroup and a ds_read per listed pair; W = 1 on the arxiv-shaped graph: 37 us against 12)
typedef unsigned uint4_a4 __attribute__((ext_vector_type(4), aligned(4)));
typedef unsigned uint4_a1 __attribute__((ext_vector_type(4), aligned(1)));
typedef unsigned uint2_a1 __attribute__((ext_vector_type(2), aligned(1)));
typedef unsigned uint1_a1 __attribute__((aligned(1)));

template <int N>
__device__ __forceinline__ void load_col_run(const int32_t* col, int (&colv)[N]) {
  static_assert(N % 4 == 0, "whole quads of column ids");
#pragma unroll
  for (int r = 0; r < N; r += 4) {
    const uint4_a4 v = *reinterpret_cast<const uint4_a4*>(col + r);
    colv[r] = static_cast<int>(v.x); colv[r + 1] = static_cast<int>(v.y);
    colv[r + 2] = static_cast<int>(v.z); colv[r + 3] = static_cast<int>(v.w);
  }
}

template <int N>
__device__ __forceinline__ void load_index_run(const int32_t* col, const uint8_t* code, int (&colv)[N], int (&codev)[N]) {
  static_assert(N == 4 || N == 8 || N == 16, "whole dwords of codes");
  load_col_run<N>(col, colv);
  unsigned cw[4] = {0u, 0u, 0u, 0u};
  if constexpr (N == 16) {
    const uint4_a1 v = *reinterpret_cast<const uint4_a1*>(code);
    cw[0] = v.x; cw[1] = v.y; cw[2] = v.z; cw[3] = v.w;
  } else if constexpr (N == 8) {
    const uint2_a1 v = *reinterpret_cast<const uint2_a1*>(code);
    cw[0] = v.x; cw[1] = v.y;
  } else {
    cw[0] = *reinterpret_cast<const uint1_a1*>(code);
  }
#pragma unroll
  for (int r = 0; r < N; ++r) codev[r] = static_cast<int>((cw[r / 4] >> (8 * (r % 4))) & 0xffu);
}

// One step of a lane group's butterfly inside a DPP row of 16 lanes (seg_body, csrc/spmm_fwd_body.hpp; csrc/spmm_stream.hip)
template <int CTRL>
__device__ __forceinline__ float dpp_row(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, false));
}

// A lane group's butterfly (LPR >= 16 lanes, aligned: whole DPP rows): every lane ends with the sum of the group's values, added in the
// pairs that __shfl_xor with offsets 1, 2, 4, ... LPR / 2 adds.  After the two quad steps the four lanes of a quad hold one value, so
// row_half_mirror and row_mirror meet the same two numbers as the xor steps 4 and 8 — same bits, no LDS crossbar for the first four steps.
template <int LPR>
__device__ __forceinline__ float group_sum(float r) {
  static_assert(LPR >= 16, "whole DPP rows");
  r += dpp_row<0xB1>(r);    // quad_perm [1, 0, 3, 2]: lane ^ 1
  r += dpp_row<0x4E>(r);    // quad_perm [2, 3, 0, 1]: lane ^ 2
  r += dpp_row<0x141>(r);   // row_half_mirror: the other quad of the eight
  r += dpp_row<0x140>(r);   // row_mirror: the other half of the sixteen
#pragma unroll
  for (int off = 16; off < LPR; off <<= 1) r += __shfl_xor(r, off);
  return r;
}

// Short-row tiles (short_tile, csrc/spmm_fwd_body.hpp): rows of exactly L pairs that one lane group takes at a time
__host__ __device__ constexpr int short_rows_per_group(int L) { return L == 0 ? 8 : (8 / L > 0 ? 8 / L : 1); }

// The kernel variants that take tiles: fp32 rows of 16-B chunks, 16 lanes or more per row (W in (32, 256]).  The others stay
// within 8 waves/SIMD only without scratch: with the tile body the bf16 variants spilled 116-132 B, W = 32 (8 lanes) 8 B.
__host__ __device__ constexpr bool short_tiles_serve(int vec, int lpr, bool smalld, bool packed, bool bycode) {
  return vec == 4 && lpr >= 16 && smalld && packed && !bycode;
}

// ---------------------------------------------------------------------------------------------
// hub-row slices: the steps every kernel family takes
// ---------------------------------------------------------------------------------------------
// Which hub row owns slice s: the last r with long_slice_ptr[r] <= s ...
__device__ __forceinline__ int slice_owner(const Params& p, int s) {
  int a = 0, b = p.n_long;
  while (b - a > 1) {
    const int mid = (a + b) >> 1;
    if (p.long_slice_ptr[mid] <= s) a = mid; else b = mid;
  }
  return a;
}
// ... or, for a wave that walks a run of slices front to back, by stepping from the owner `a` of the slice before
__device__ __forceinline__ int slice_owner_from(const Params& p, int a, int s) {
  while (p.long_slice_ptr[a + 1] <= s) ++a;
  return a;
}
// ... and the pairs [lo, hi) of slice s of hub row a, adjacency row i (dense layout: the "pairs" of a row are all n_cols
// neighbours, the column is the position)
template <bool DENSE = false>
__device__ __forceinline__ void slice_range(const Params& p, int64_t i, int a, int s, int64_t& lo, int64_t& hi) {
  const int64_t row_lo = DENSE ? 0 : load_rowptr(p, i), row_hi = DENSE ? p.n_cols : load_rowptr(p, i + 1);
  lo = row_lo + static_cast<int64_t>(s - p.long_slice_ptr[a]) * p.slice_edges;
  hi = lo + p.slice_edges < row_hi ? lo + p.slice_edges : row_hi;
}

// ---------------------------------------------------------------------------------------------
// host side: validation, the kernels' argument record, tiling
// ---------------------------------------------------------------------------------------------
inline bool aligned(const void* ptr, size_t n) { return (reinterpret_cast<uintptr_t>(ptr) % n) == 0; }
constexpr int kHotLdsFloats = 16384;   // 64 KB of hot operand rows per workgroup (the default dynamic-LDS limit): two workgroups per CU

// the self_sum route as the classed rows, the blocked hubs and the pair stream need it: short-row runs declared, s_total set
inline bool self_route_with_tiles(const gnan_spmm_args* a) { return a->self_sum && a->s_total && a->short_lmax > 0; }

// does the pair stream end with hub rows (gnan_spmm_args.q_hub: rows [q_hub, stream_q_hi), a combine pass of their own)?
inline bool stream_takes_hubs(const gnan_spmm_args* a) { return a->stream_index && a->q_hub > 0 && a->q_hub < a->stream_q_hi; }

inline int validate(const gnan_spmm_args* a) {
  GNAN_REQUIRE(a != nullptr, "spmm: null args");
  GNAN_REQUIRE(a->n_rows >= 0 && a->n_cols >= 0, "spmm: negative size");
  GNAN_REQUIRE(a->W >= 1, "spmm: W must be >= 1 (got %d)", a->W);
  GNAN_REQUIRE(a->D >= 1 && a->D <= GNAN_MAX_CODES, "spmm: D must be in [1, %d] (got %d)", GNAN_MAX_CODES, a->D);
  GNAN_REQUIRE(a->Cw >= 1, "spmm: Cw must be >= 1");
  GNAN_REQUIRE(a->n_cols <= 0x7fffffffLL, "spmm: n_cols exceeds int32 column ids");
  if (a->n_rows == 0) return GNAN_OK;
  GNAN_REQUIRE(a->S && a->lut && a->Y && (a->code || a->packed_index), "spmm: null S / lut / Y / code");
  GNAN_REQUIRE((a->rowptr == nullptr) == (a->col == nullptr), "spmm: rowptr and col must both be set (CSR) or both NULL (dense)");
  GNAN_REQUIRE(a->s_stride >= a->W && (a->reduce_cr != 0 || a->y_stride >= a->W), "spmm: row stride smaller than W");
  if (a->s_dtype != GNAN_F32 && a->s_dtype != GNAN_BF16) return gnan::fail(GNAN_ERR_BAD_ARG, "spmm: unknown operand dtype %d", a->s_dtype);
  if (a->s_dtype == GNAN_BF16) {
    if (a->W % 8 != 0 || a->s_stride % 8 != 0 || reinterpret_cast<uintptr_t>(a->S) % 16 != 0 || a->rowptr == nullptr)
      return gnan::fail(GNAN_ERR_UNSUPPORTED, "spmm: bf16 operand rows need the CSR layout, W %% 8 == 0 and 16-B aligned rows");
    if (a->reduce_cr == 0 && (a->y_stride % 4 != 0 || reinterpret_cast<uintptr_t>(a->Y) % 16 != 0))
      return gnan::fail(GNAN_ERR_UNSUPPORTED, "spmm: bf16 operand rows need a 16-B aligned fp32 output");
    if (a->s_total && reinterpret_cast<uintptr_t>(a->s_total) % 16 != 0)
      return gnan::fail(GNAN_ERR_UNSUPPORTED, "spmm: s_total must be 16-B aligned");
  }
  GNAN_REQUIRE(!(a->weight_by_col && a->s_total), "spmm: weight_by_col excludes the rest-bucket term (add it outside)");
  GNAN_REQUIRE(!a->s_by_code || (a->rowptr != nullptr && a->s_total == nullptr && a->s_dtype == GNAN_F32),
               "spmm: s_by_code needs the CSR layout, fp32 rows and no rest-bucket term");
  if (a->s_by_code && a->W > 32)
    return gnan::fail(GNAN_ERR_UNSUPPORTED, "spmm: s_by_code covers operand rows of at most 32 columns (got W=%d)", a->W);
  GNAN_REQUIRE(!a->scatter_out || a->row_ids, "spmm: scatter_out needs row_ids");
  if (a->packed_index && (a->rowptr == nullptr || a->D > 4 || a->Cw != 1 || a->weight_by_col || a->minus_rest || a->s_by_code ||
                          a->n_cols > static_cast<int64_t>(kPackMask) + 1))
    return gnan::fail(GNAN_ERR_UNSUPPORTED, "spmm: packed index entries need the CSR layout, D <= 4, one weight channel, plain "
                      "forward weights and n_cols <= 2^29");
  if (a->self_sum && !(a->packed_index && a->scatter_out == 2 && a->s_dtype == GNAN_F32 && a->reduce_cr == 1 && a->lut_row_stride == 0 &&
                       a->self_parts >= 1 && a->hot_rows == 0 && a->shell_out == nullptr))
    return gnan::fail(GNAN_ERR_UNSUPPORTED, "spmm: self_sum is served over a packed degree-sorted copy (scatter_out 2) with a global "
                      "small-D table, fp32 rows and reduce_cr == 1 (self_parts >= 1)");
  GNAN_REQUIRE(!a->lone_rows || a->self_sum, "spmm: lone_rows (the rows without a pair, a thread each) is served on the self_sum route only");
  if (a->reduce_cr != 0) {
    const int cr = a->reduce_cr;
    if (!(cr == 1 || cr == 2 || cr == 4) || a->W % cr != 0)
      return gnan::fail(GNAN_ERR_UNSUPPORTED, "spmm: fused read-out needs reduce_cr in {1, 2, 4} dividing W (got %d, W=%d)",
                        cr, a->W);
    GNAN_REQUIRE(a->y_stride >= cr, "spmm: y_stride smaller than reduce_cr");
  }
  if (a->short_lmax != 0) {
    const int lm = a->short_lmax;
    GNAN_REQUIRE(lm > 0 && lm <= GNAN_SHORT_LMAX, "spmm: short_lmax must be in [0, %d] (got %d)", GNAN_SHORT_LMAX, lm);
    GNAN_REQUIRE(a->short_row && a->short_pair, "spmm: short_lmax > 0 needs the short_row / short_pair host arrays");
    GNAN_REQUIRE(a->rowptr != nullptr && a->scatter_out == 2 && a->short_row[0] == 0 && a->short_row[lm + 1] <= a->n_rows,
                 "spmm: short-row runs need a degree-sorted copy (CSR, scatter_out 2) and runs from row 0 within n_rows");
    for (int L = 0; L <= lm; ++L) {
      const int64_t n = a->short_row[L + 1] - a->short_row[L];
      const int64_t end = a->short_pair[L] + n * L;
      GNAN_REQUIRE(n >= 0 && a->short_pair[L] >= 0 && (a->nnz <= 0 || end <= a->nnz) && (L == lm || end == a->short_pair[L + 1]),
                   "spmm: short-row run %d is inconsistent (rows %lld, first pair %lld)", L, static_cast<long long>(n),
                   static_cast<long long>(a->short_pair[L]));
    }
  }
  if (a->seg_index) {
    // (one pair of requirements: the fields are read by the self_sum instance alone, over a well-formed plan)
    if (!self_route_with_tiles(a))
      return gnan::fail(GNAN_ERR_UNSUPPORTED, "spmm: classed row segments are served on the self_sum route (short-row runs declared, "
                        "s_total set) only");
    GNAN_REQUIRE(a->seg_start && a->seg_row && a->cls_seg_ptr && a->seg_mask && a->n_seg > 0 && a->seg_max_per_class > 0 &&
                 a->seg_max_per_class <= a->n_seg && a->seg_q_lo >= a->short_row[a->short_lmax + 1] && a->seg_q_lo < a->seg_q_hi &&
                 a->seg_q_hi <= a->n_rows && a->D <= 8,
                 "spmm: incomplete classed row plan (segments, a class table, a mask, rows behind the tiled runs within n_rows)");
  }
  if (a->hub_index) {
    // (read by the self_sum instance alone, in place of a hub-row plan)
    if (!(self_route_with_tiles(a) && a->n_long == 0 && a->cls_index == nullptr))
      return gnan::fail(GNAN_ERR_UNSUPPORTED, "spmm: blocked hub segments are served on the self_sum route (short-row runs declared, "
                        "s_total set) without a hub-row plan only");
    GNAN_REQUIRE(a->hub_seg_start && a->hub_seg_row && a->hub_seg_slot && a->hub_row_slot_ptr && a->hub_cls_seg_ptr && a->n_hub > 0 &&
                 a->n_hub_seg > 0 && a->hub_seg_max_per_class > 0 && a->hub_seg_max_per_class <= a->n_hub_seg && a->long_threshold > 0 &&
                 a->hub_q_lo >= a->short_row[a->short_lmax + 1] && a->hub_q_lo + a->n_hub == a->n_rows &&
                 (a->seg_index == nullptr || a->seg_q_hi <= a->hub_q_lo) && a->D <= 8,
                 "spmm: incomplete blocked hub plan (segments, slots, a class table, the hub rows the last n_hub of n_rows behind the "
                 "tiled and the classed rows, long_threshold set)");
  }
  if (a->stream_index) {
    // (read by the stream's own kernels and, as the skipped range, by the self_sum instance of spmm_kernel)
    if (!self_route_with_tiles(a))
      return gnan::fail(GNAN_ERR_UNSUPPORTED, "spmm: the pair stream is served on the self_sum route (short-row runs declared, s_total set) only");
    GNAN_REQUIRE(a->stream_chunk > 0 && a->stream_chunk % 16 == 0, "spmm: the pair stream's chunk must be a positive multiple of 16 (got %d)",
                 a->stream_chunk);
    GNAN_REQUIRE(a->seg_index == nullptr, "spmm: a pair stream and a classed row plan cannot both take rows [%lld, %lld)",
                 static_cast<long long>(a->stream_q_lo), static_cast<long long>(a->stream_q_hi));
    GNAN_REQUIRE(a->stream_cls_pair_ptr && a->stream_cls_chunk_ptr && a->stream_chunk_first_seg && a->stream_row_seg &&
                 a->stream_row_slot_ptr && a->n_stream_seg > 0 && a->stream_max_chunks_per_class > 0 &&
                 a->stream_q_lo >= a->short_row[a->short_lmax + 1] && a->stream_q_lo < a->stream_q_hi &&
                 a->stream_q_hi <= (a->hub_index ? a->hub_q_lo : a->n_rows) && a->stream_code >= 0 && a->stream_code < 4 && a->D <= 4,
                 "spmm: incomplete pair stream plan (class tables, chunk and slot tables, rows behind the tiled runs and before the hub "
                 "rows, one hop code below 4)");
    // the hub rows through the stream: its last rows, in place of a hub-row plan and of the blocked hub segments
    GNAN_REQUIRE(a->q_hub == 0 || (a->q_hub > a->stream_q_lo && a->q_hub <= a->stream_q_hi),
                 "spmm: q_hub must be 0 or a row in (stream_q_lo, stream_q_hi] (got %lld)", static_cast<long long>(a->q_hub));
    GNAN_REQUIRE(!stream_takes_hubs(a) || (a->stream_q_hi == a->n_rows && a->hub_index == nullptr && a->n_long == 0),
                 "spmm: hub rows in the pair stream need the stream to end at n_rows, no blocked hub segments and no hub-row plan");
  }   // (q_hub, at the struct's end, is read beside a pair stream only)
  if (a->n_long > 0) {
    GNAN_REQUIRE(a->rowptr != nullptr || (a->n_long == a->n_rows && a->long_threshold == 0),
                 "spmm: a row plan for the dense layout must slice every row (n_long == n_rows, long_threshold == 0)");
    GNAN_REQUIRE(a->long_rows && a->long_slice_ptr && a->slice_edges > 0 && a->n_slices > 0,
                 "spmm: incomplete long-row plan");
    if (a->cls_index) {
      GNAN_REQUIRE(a->rowptr != nullptr && a->cls_slice_start && a->cls_slice_row && a->cls_slot_slice && a->cls_n_slots > 0 &&
                   a->cls_n_slots % 8 == 0 && a->n_cols <= static_cast<int64_t>(kPackMask) + 1 && a->D <= 8,
                   "spmm: incomplete classed hub plan (CSR, slot table of a positive multiple of 8, n_cols <= 2^29, D <= 8)");
    }
  }
  return GNAN_OK;
}

// floats of the hub slices' partials at the head of the forward's workspace; the classed rows' [seg_q_hi - seg_q_lo, 8] floats follow,
// the blocked hub segments' [n_hub_seg] floats come last
inline size_t seg_partial_offset(const gnan_spmm_args* a) {
  return a->n_long > 0 ? static_cast<size_t>(a->n_slices) * 2 * static_cast<size_t>(a->W) : 0;
}
inline size_t hub_partial_offset(const gnan_spmm_args* a) {
  size_t floats = seg_partial_offset(a);
  if (a->seg_index && a->seg_q_hi > a->seg_q_lo) floats += static_cast<size_t>(a->seg_q_hi - a->seg_q_lo) * 8;
  return floats;
}
// ... and the pair stream's [n_stream_seg] floats behind those
inline size_t stream_partial_offset(const gnan_spmm_args* a) {
  size_t floats = hub_partial_offset(a);
  if (a->hub_index && a->n_hub_seg > 0) floats += static_cast<size_t>(a->n_hub_seg);
  return floats;
}

inline Params make_params(const gnan_spmm_args* a) {
  Params p;
  p.n_rows = a->n_rows; p.n_cols = a->n_cols; p.nnz = a->nnz > 0 ? a->nnz : 0;
  p.rowptr = a->rowptr; p.rowptr_is64 = a->rowptr_is64;
  p.col = a->col; p.code = a->code; p.row_ids = a->row_ids;
  p.S = a->S; p.W = a->W; p.s_stride = a->s_stride;
  p.lut = a->lut; p.lut_row_stride = a->lut_row_stride; p.D = a->D; p.Cw = a->Cw;
  p.cnt = a->cnt; p.cnt_stride = a->cnt_stride; p.s_total = a->s_total;
  p.weight_by_col = a->weight_by_col; p.minus_rest = a->minus_rest; p.reduce_cr = a->reduce_cr;
  p.scatter_out = a->scatter_out;
  p.s_by_code = a->s_by_code;
  p.packed = a->packed_index;
  p.Y = a->Y; p.y_stride = a->y_stride;
  p.long_threshold = a->n_long > 0 ? a->long_threshold : INT64_MAX;
  p.long_rows = a->long_rows; p.long_slice_ptr = a->long_slice_ptr;
  p.n_long = a->n_long > 0 ? a->n_long : 0;
  p.n_slices = a->n_long > 0 ? a->n_slices : 0;
  p.slice_edges = a->slice_edges;
  p.partial = static_cast<float*>(a->workspace);
  p.hot_lo = a->hot_lo; p.hot_n = a->hot_rows;
  p.shell_out = a->shell_out;
  const bool classed = a->n_long > 0 && a->cls_index != nullptr;
  p.cls_index = classed ? a->cls_index : nullptr;
  p.cls_slice_start = a->cls_slice_start; p.cls_slice_row = a->cls_slice_row; p.cls_slot_slice = a->cls_slot_slice;
  p.cls_n_slots = a->cls_n_slots;
  p.n_slice_blocks = classed ? 8 * ((a->cls_n_slots / 8 + 3) / 4) : p.n_slices;
  const bool runs = a->short_lmax > 0 && a->short_lmax <= GNAN_SHORT_LMAX && a->short_row && a->short_pair;  // (validate() checks them)
  p.self_sum = a->self_sum; p.self_parts = a->self_sum ? a->self_parts : 0;
  p.short_lmax = runs ? a->short_lmax : 0;
  p.seg_index = a->seg_index; p.seg_start = a->seg_start; p.seg_row = a->seg_row; p.cls_seg_ptr = a->cls_seg_ptr;
  p.seg_mask = a->seg_mask;
  p.seg_q_lo = p.seg_q_hi = 0;
  p.n_seg_blocks = 0;
  p.seg_partial = nullptr;
  if (a->seg_index) {   // (behind the hub slices' [n_slices, 2, W] partials: seg_partial_offset)
    p.seg_q_lo = a->seg_q_lo; p.seg_q_hi = a->seg_q_hi;
    p.seg_partial = static_cast<float*>(a->workspace) + seg_partial_offset(a);
  } else if (a->stream_index) {   // (validate(): no classed row plan beside it) the pair stream's rows: skipped by the row blocks alike
    p.seg_q_lo = a->stream_q_lo; p.seg_q_hi = a->stream_q_hi;     // (with hub rows in the stream: to n_rows — tile blocks alone are left)
  }
  p.hub_index = a->hub_index; p.hub_seg_start = a->hub_seg_start; p.hub_seg_row = a->hub_seg_row; p.hub_seg_slot = a->hub_seg_slot;
  p.hub_row_slot_ptr = a->hub_row_slot_ptr; p.hub_cls_seg_ptr = a->hub_cls_seg_ptr;
  p.hub_partial = nullptr;
  p.hub_q_lo = a->n_rows;
  p.n_hub = p.n_hub_blocks = 0;
  if (a->hub_index) {   // (validate(): no hub-row plan beside it; the row blocks still leave the hub rows out by their length)
    p.hub_q_lo = a->hub_q_lo; p.n_hub = a->n_hub;
    p.hub_partial = static_cast<float*>(a->workspace) + hub_partial_offset(a);
    p.long_threshold = a->long_threshold;
  }
  p.n_tile_blocks = p.n_tiles = 0;
  p.row_q0 = 0;
  p.lone = a->lone_rows != 0 && a->self_sum != nullptr;
  p.lone_n = 0;
  p.tile_lo = 0;
  for (int L = 0; L <= GNAN_SHORT_LMAX + 1; ++L) p.short_row[L] = L <= p.short_lmax + 1 && runs ? a->short_row[L] : 0;
  for (int L = 0; L <= GNAN_SHORT_LMAX; ++L) {
    p.short_pair[L] = L <= p.short_lmax && runs ? a->short_pair[L] : 0;
    p.short_tile[L] = 0;
  }
  return p;
}

// operand rows are read 16 B per lane when shape and alignment allow it, else 4 B per lane
inline void pick_tiling(const gnan_spmm_args* a, const float* out, int64_t out_stride, int* vec, int* lpr) {
  *vec = 1;
  if (a->W % 4 == 0 && a->s_stride % 4 == 0 && out_stride % 4 == 0 && aligned(a->S, 16) && aligned(out, 16) &&
      (!a->s_total || aligned(a->s_total, 16)))
    *vec = 4;
  *lpr = 1;
  while (*lpr * *vec < a->W && *lpr < kWave) *lpr <<= 1;
}

// The tile partition of a launch of the <vec, lpr> variant: which of the declared short-row runs the kernel takes in tiles, and where
// each run's tiles start.  The launch and gnan_spmm_fwd_describe both call this (and nothing else decides it).
inline int plan_tiles(Params& p, int vec, int lpr, bool dense, bool smalld, int seg_max = 0, int hub_seg_max = 0) {
  const int G = kWave / lpr;
  // short-row tiles: the packed small-D forward over a degree-sorted copy, one pass of the lane group over the columns
  if (short_tiles_serve(vec, lpr, smalld, p.packed, p.s_by_code) && p.short_lmax > 0 && !dense && p.scatter_out == 2 &&
      lpr * vec >= p.W && p.nnz > 0) {
    int64_t t = 0;
    for (int L = 0; L <= p.short_lmax; ++L) {
      p.short_tile[L] = static_cast<int>(t);
      const int64_t per = static_cast<int64_t>(G) * short_rows_per_group(L);
      t += (p.short_row[L + 1] - p.short_row[L] + per - 1) / per;
    }
    if (t > 0x7fffffffLL - 3) return gnan::fail(GNAN_ERR_UNSUPPORTED, "spmm: too many short-row tiles for one launch");
    p.n_tiles = static_cast<int>(t);
    p.n_tile_blocks = static_cast<int>((t + 3) / 4);
    p.row_q0 = p.short_row[p.short_lmax + 1];
    // the lone rows leave the tiles (the partition above is reported as it is; the launch drops run 0's tiles: leave_lone_tiles)
    if (p.lone && p.self_sum && p.short_row[1] > p.short_row[0]) {
      p.lone_n = p.short_row[1] - p.short_row[0];
      p.tile_lo = p.short_tile[1];         // (short_lmax >= 1: run 1's first tile is set)
    }
  } else {
    p.short_lmax = 0;
  }
  if (p.seg_index) {
    // classed row segments: the route validate() admits runs the tiled SELF instance; G segments per wave, 4 waves per workgroup,
    // as many workgroups per class as the longest class needs, interleaved so that blockIdx & 7 is the class
    if (!(p.short_lmax > 0 && p.self_sum && p.seg_q_lo >= p.row_q0))
      return gnan::fail(GNAN_ERR_UNSUPPORTED, "spmm: classed row segments need the tiled self_sum variant (fp32 rows of 16 lanes or more)");
    const int64_t per = 4 * static_cast<int64_t>(G);
    const int64_t nb = 8 * ((static_cast<int64_t>(seg_max) + per - 1) / per);
    if (nb > 0x3fffffffLL) return gnan::fail(GNAN_ERR_UNSUPPORTED, "spmm: too many row segments for one launch");
    p.n_seg_blocks = static_cast<int>(nb);
  }
  if (p.hub_index) {   // blocked hub segments: the same partition, their workgroups at the launch's head
    if (!(p.short_lmax > 0 && p.self_sum && p.hub_q_lo >= p.row_q0))
      return gnan::fail(GNAN_ERR_UNSUPPORTED, "spmm: blocked hub segments need the tiled self_sum variant (fp32 rows of 16 lanes or more)");
    const int64_t per = 4 * static_cast<int64_t>(G);
    const int64_t nb = 8 * ((static_cast<int64_t>(hub_seg_max) + per - 1) / per);
    if (nb > 0x3fffffffLL) return gnan::fail(GNAN_ERR_UNSUPPORTED, "spmm: too many hub segments for one launch");
    p.n_hub_blocks = static_cast<int>(nb);
  }
  return GNAN_OK;
}


// Tile workgroups of the launch once the lone rows have left (plan_tiles' tile_lo): run 0's tiles are not run, the others keep their
// order.  lone_tile_blocks: what is launched of n_tile_blocks; leave_lone_tiles: the same partition numbered from tile_lo, for the
// kernel — short_tile[1] becomes 0, so short_tiles() finds run 1 or a later one for every tile and run 0 is never entered.
inline int lone_tile_blocks(const Params& p) { return p.tile_lo > 0 ? (p.n_tiles - p.tile_lo + 3) / 4 : p.n_tile_blocks; }
inline void leave_lone_tiles(Params& p) {
  if (p.tile_lo <= 0) return;
  p.n_tile_blocks = lone_tile_blocks(p);
  p.n_tiles -= p.tile_lo;
  for (int L = 1; L <= p.short_lmax; ++L) p.short_tile[L] -= p.tile_lo;
  p.tile_lo = 0;
}

// The one switch over the lanes per row: f(std::integral_constant<int, LPR>{}) for lpr in {1, 2, ..., 64}.
template <class F>
int dispatch_lpr(int lpr, F&& f) {
  switch (lpr) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 4: return f(std::integral_constant<int, 4>{});
    case 8: return f(std::integral_constant<int, 8>{});
    case 16: return f(std::integral_constant<int, 16>{});
    case 32: return f(std::integral_constant<int, 32>{});
    default: return f(std::integral_constant<int, 64>{});
  }
}

// The hub-row slices' per-shell sums [n_slices, 4, W] at the head of a gradient workspace, rounded up to 16 bytes: the float64
// records behind them are read in 16-byte halves.
inline size_t slice_T_bytes(const gnan_spmm_args* a) {
  const size_t bytes = a->n_long > 0 ? static_cast<size_t>(a->n_slices) * 4 * static_cast<size_t>(a->W) * sizeof(float) : 0;
  return (bytes + 15) / 16 * 16;
}

// What gnan_spmm_fwd alone reads, refused by the other entry points (`who`): the self term (the gradients refuse it before
// validate(), which knows it on the forward's route only) and, behind validate(), the classed hub plan and the packed index
// (gnan_spmm_bwd_narrow reads a packed index itself).
inline int forward_only_self_sum(const gnan_spmm_args* a, const char* who) {
  GNAN_REQUIRE(a->self_sum == nullptr, "%s: self_sum is read by gnan_spmm_fwd only", who);
  return GNAN_OK;
}
inline int forward_only_index(const gnan_spmm_args* a, const char* who, bool reads_packed = false) {
  GNAN_REQUIRE(a->cls_index == nullptr, "%s: the classed hub plan is read by gnan_spmm_fwd only", who);
  GNAN_REQUIRE(a->hub_index == nullptr, "%s: blocked hub segments are read by gnan_spmm_fwd only", who);
  GNAN_REQUIRE(a->stream_index == nullptr, "%s: the pair stream is read by gnan_spmm_fwd only", who);
  GNAN_REQUIRE(reads_packed || !a->packed_index, "%s: packed index entries are read by gnan_spmm_fwd only", who);
  return GNAN_OK;
}

using gnan::cu_count;   // (csrc/common.hpp; the persistent kernels run two workgroups on each compute unit)
}  // namespace

namespace gnan {
// The forward's rows / tiles / slices launch for operand rows read VEC floats per lane (8: bf16 rows): csrc/spmm_fwd_body.hpp,
// one object per VEC (csrc/spmm_fwd_v1.hip, _v4, _v8).  The caller launches the hub rows' fix-up behind it.
template <int VEC>
int launch_lpr(const gnan_spmm_args* a, int lpr, bool dense, bool smalld, hipStream_t st);
// The pair stream (gnan_spmm_args.stream_*; csrc/spmm_stream.hip, an object of its own): the stream's kernel, launched ahead of
// spmm_kernel, and its combine, launched behind it; both return at once without a stream.  stream_blocks: the former's workgroups.
int stream_blocks(const gnan_spmm_args* a, int lpr);
int launch_stream(const gnan_spmm_args* a, int lpr, hipStream_t st);
int launch_stream_combine(const gnan_spmm_args* a, hipStream_t st);
// The lone rows (gnan_spmm_args.lone_rows; csrc/spmm_lone.hip, an object of its own): a thread per row of run 0, launched beside
// spmm_kernel — the two write disjoint rows.  Returns at once where plan_tiles names no lone row.
int launch_lone(const gnan_spmm_args* a, int lpr, hipStream_t st);
int lone_blocks(int64_t lone_n);      // its workgroups for plan_tiles' lone_n rows
}  // namespace gnan
