// Attributions by source node  B[p, d, w] = V[p, d, w % Cw] * S[j_p, w]  — the column-side sum of the aggregation's terms:
// V[p, d, c] adds the weights wt(i, d, c) of the requested rows i that see source j_p at hop d (include/gnan_hip.h has the
// definition and the rest-shell rule).  V does not depend on the operand column, so a column of the adjacency is walked ONCE
// and B = V (x) S is a streaming epilogue.  Up to seven launches, no floating-point atomic, no workgroup waits for another:
//
//   cols_fill_kernel / cols_count_kernel   row_ids given: mult[i] = how often forward row i is requested (integer atomicAdd on
//                        int32 words of the workspace; integer addition commutes, the counts do not depend on the order).
//   cols_total_kernel / cols_total_finish_kernel   rest_from_total: T[c] = sum_i mult[i] wt(i, D-1, c).  A block of kTRows
//                        forward rows per workgroup: a thread's rows in row order, the lanes by a butterfly, the waves in wave
//                        order; then the blocks in block order.
//   cols_walk_kernel     one WAVE per work item = one chunk of kChunk pairs of one requested source (the transposed adjacency:
//                        forward row id + code per pair, 5 B, read coalesced; a 4-B mult gather, a 4-B cnt gather and the lut
//                        word per pair).  A lane owns pairs (pair l of the chunk: lane l % 64), its accumulators are lane-private
//                        words in LDS, acc[wave][bin of the pass][lane]: bank = lane, a plain read / add / write of the lane's
//                        own word — no conflict, no LDS atomic, no barrier (a wave reads only what it wrote).  Bins are
//                        (shell, weight channel) = d * Cw + c, taken in passes of 64 (64 KiB of LDS at most; Cw = 1, D = 256: four
//                        passes, each re-walks the chunk).  A pass ends with the 64 lanes added by a fixed butterfly
//                        (xor 32, 16, .., 1); the raw sums go to V itself (a column of one chunk) or the item's slot of the workspace.
//                        Under rest_from_total a pair coded below D-1 also adds wt(i, D-1, c) to the rest bins (the listed sum), a
//                        pair coded >= D-1 adds nothing.
//   cols_combine_kernel  a thread per (source, bin): a long column's partials in chunk order; the rest bins become T - listed.
//   cols_scale_kernel    B = V * S, a thread per (source, column) of one shell (grid.y = shell): coalesced read of S, coalesced
//                        write of B, the product ONCE on the combined sum.
//
// A source's bits depend on its own pairs and on the set of requested rows (through mult and T) only: chunk boundaries are
// multiples of kChunk from the column's start whatever else is requested.
#include "common.hpp"

namespace {

constexpr int kThreads = 256, kWaves = 4, kLanes = 64, kPassBins = 64, kFlight = 8;
constexpr int kChunk = 512;                  // pairs per work item: eight per lane, one round of kFlight loads
constexpr int kTRows = 4096;                 // forward rows per workgroup of the T sum
constexpr int kScaleElems = 1024;            // (source, column) products per workgroup of the epilogue

struct Params {
  int64_t n_cols, n_src, n_rows;
  const void* rowptr_t;
  int rowptr_is64;
  const int32_t* row;
  const uint8_t* code;
  const int32_t* col_ids;
  const int32_t* row_ids;
  int64_t n_row_ids;
  const float* S;
  int W;
  int64_t s_stride;
  const float* lut;
  int64_t lut_row_stride;
  int D, Cw;
  const int32_t* cnt;
  int64_t cnt_stride;
  int rest_from_total;
  float* B;
  int64_t b_stride;
  const int32_t* item_ptr;     // [n_cols + 1] or NULL: every source has `uniform_chunks` items
  int64_t n_items;
  int uniform_chunks;
  int64_t bins;                // D * Cw
  int cap;                     // bins of a pass held in LDS: min(bins, 64)
  int64_t t_blocks;
  int spb;                     // sources per workgroup of the epilogue
  int32_t* mult;               // [n_rows] or NULL: every forward row once
  float* t_part;               // [t_blocks, Cw]
  float* T;                    // [Cw]
  float* V;                    // [n_cols, bins]
  float* part;                 // [n_items, bins] raw partial sums of the columns of more than one chunk
};

struct Item {
  int64_t q, first;            // requested source, its first work item
  int c, nch;                  // chunk of the column, chunks of the column
};

__device__ __forceinline__ Item locate(const Params& p, int64_t item) {
  Item it;
  if (p.item_ptr == nullptr) {
    it.q = item / p.uniform_chunks;
    it.nch = p.uniform_chunks;
    it.first = it.q * p.uniform_chunks;
  } else {
    // the last q with item_ptr[q] <= item; every source has at least one item, so q lies in [item - (n_items - n_cols), item]
    int64_t lo = item - (p.n_items - p.n_cols), hi = item < p.n_cols - 1 ? item : p.n_cols - 1;
    if (lo < 0) lo = 0;
    while (lo < hi) {
      const int64_t mid = (lo + hi + 1) >> 1;
      if (static_cast<int64_t>(p.item_ptr[mid]) <= item) lo = mid; else hi = mid - 1;
    }
    it.q = lo;
    it.first = p.item_ptr[lo];
    it.nch = p.item_ptr[lo + 1] - p.item_ptr[lo];
  }
  it.c = static_cast<int>(item - it.first);
  return it;
}

__device__ __forceinline__ void col_range(const Params& p, int64_t j, int64_t* lo, int64_t* hi) {
  if (p.rowptr_t == nullptr) {
    *lo = j * p.n_rows;
    *hi = *lo + p.n_rows;
  } else if (p.rowptr_is64) {
    *lo = static_cast<const int64_t*>(p.rowptr_t)[j];
    *hi = static_cast<const int64_t*>(p.rowptr_t)[j + 1];
  } else {
    *lo = static_cast<const int32_t*>(p.rowptr_t)[j];
    *hi = static_cast<const int32_t*>(p.rowptr_t)[j + 1];
  }
}

__device__ __forceinline__ float wave_sum(float v) {               // the 64 lanes in a fixed tree; every lane gets the sum
#pragma unroll
  for (int off = kLanes / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, kLanes);
  return v;
}

__global__ __launch_bounds__(kThreads) void cols_fill_kernel(int32_t* mult, int64_t n) {
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x; i < n; i += static_cast<int64_t>(gridDim.x) * kThreads) mult[i] = 0;
}

__global__ __launch_bounds__(kThreads) void cols_count_kernel(const Params p) {
  const int64_t q = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (q >= p.n_row_ids) return;
  const int64_t i = p.row_ids[q];
  if (i >= 0 && i < p.n_rows) atomicAdd(p.mult + i, 1);           // integer: the count does not depend on the order
}

// wt(i, d, c) * m; the division only where counts are given
__device__ __forceinline__ float weight(const Params& p, int64_t i, int d, int c, float den) {
  float wt = p.lut[i * p.lut_row_stride + static_cast<int64_t>(d) * p.Cw + c];
  if (p.cnt) wt = wt / den;
  return wt;
}

__device__ __forceinline__ float denominator(const Params& p, int64_t i, int d) {
  if (!p.cnt) return 1.f;
  const int n = p.cnt[i * p.cnt_stride + d];
  return static_cast<float>(n > 1 ? n : 1);
}

__global__ __launch_bounds__(kThreads) void cols_total_kernel(const Params p) {
  __shared__ float red[kWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t r0 = static_cast<int64_t>(blockIdx.x) * kTRows;
  const int64_t r1 = r0 + kTRows < p.n_rows ? r0 + kTRows : p.n_rows;
  const int rest = p.D - 1;
  for (int c = 0; c < p.Cw; ++c) {
    float a = 0.f;
    for (int64_t i = r0 + threadIdx.x; i < r1; i += kThreads) {
      const int m = p.mult ? p.mult[i] : 1;
      if (m > 0) a += static_cast<float>(m) * weight(p, i, rest, c, denominator(p, i, rest));
    }
    a = wave_sum(a);
    if (lane == 0) red[wave] = a;
    __syncthreads();
    if (threadIdx.x == 0) p.t_part[static_cast<int64_t>(blockIdx.x) * p.Cw + c] = ((red[0] + red[1]) + red[2]) + red[3];
    __syncthreads();
  }
}

// base[0] + base[stride] + ... + base[(n - 1) * stride], added strictly in that order, eight loads in flight (n >= 1)
__device__ __forceinline__ float ordered_sum(const float* base, int64_t stride, int64_t n) {
  float z = base[0];
  int64_t c = 1;
  for (; c + kFlight <= n; c += kFlight) {
    float t[kFlight];
#pragma unroll
    for (int u = 0; u < kFlight; ++u) t[u] = base[(c + u) * stride];
#pragma unroll
    for (int u = 0; u < kFlight; ++u) z += t[u];
  }
  for (; c < n; ++c) z += base[c * stride];
  return z;
}

__global__ __launch_bounds__(kThreads) void cols_total_finish_kernel(const Params p) {
  const int c = blockIdx.x * kThreads + threadIdx.x;
  if (c < p.Cw) p.T[c] = ordered_sum(p.t_part + c, p.Cw, p.t_blocks);
}

// the bins of shell d that fall into the pass [b0, b0 + nb): mine[(d * Cw + c - b0) * 64] += m * wt(i, d, c)
__device__ __forceinline__ void add_shell(const Params& p, float* mine, int64_t b0, int nb, int d, int64_t i, float m) {
  const int64_t base = static_cast<int64_t>(d) * p.Cw - b0;      // bin of channel 0, relative to the pass
  const int c_lo = base < 0 ? static_cast<int>(-base) : 0;
  const int64_t c_end = static_cast<int64_t>(nb) - base;
  const int c_hi = c_end < p.Cw ? static_cast<int>(c_end) : p.Cw;
  if (c_lo >= c_hi) return;
  const float den = denominator(p, i, d);
  for (int c = c_lo; c < c_hi; ++c) mine[(base + c) * kLanes] += m * weight(p, i, d, c, den);
}

__global__ __launch_bounds__(kThreads) void cols_walk_kernel(const Params p) {
  extern __shared__ float acc[];                     // [kWaves][cap][64]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t item = static_cast<int64_t>(blockIdx.x) * kWaves + wave;
  if (item >= p.n_items) return;                     // a whole wave; this kernel has no barrier
  const Item it = locate(p, item);
  const int64_t j = p.col_ids ? p.col_ids[it.q] : it.q;
  int64_t lo = 0, hi = 0;
  if (j >= 0 && j < p.n_src) col_range(p, j, &lo, &hi);
  // chunk c of the column: kChunk pairs from lo + c * kChunk; the column's LAST item takes whatever is left, so that an
  // understated chunk count costs time and never a pair
  int64_t b = lo + static_cast<int64_t>(it.c) * kChunk;
  if (b > hi) b = hi;
  int64_t e = b + kChunk;
  if (e > hi || it.c == it.nch - 1) e = hi;
  const bool dense = p.rowptr_t == nullptr;
  float* dst = it.nch == 1 ? p.V + it.q * p.bins : p.part + item * p.bins;
  float* mine = acc + static_cast<int64_t>(wave) * p.cap * kLanes + lane;     // + bin * 64: this lane's word of a bin
  const int rest = p.D - 1;

  for (int64_t b0 = 0; b0 < p.bins; b0 += kPassBins) {
    const int nb = p.bins - b0 < kPassBins ? static_cast<int>(p.bins - b0) : kPassBins;
    for (int s = 0; s < nb; ++s) mine[s * kLanes] = 0.f;
    for (int64_t p0 = b + lane; p0 < e; p0 += static_cast<int64_t>(kFlight) * kLanes) {
      int cd[kFlight], m[kFlight];
      int64_t ri[kFlight];
#pragma unroll
      for (int u = 0; u < kFlight; ++u) {
        const int64_t pp = p0 + static_cast<int64_t>(u) * kLanes;
        m[u] = 0;
        cd[u] = 0;
        ri[u] = 0;
        if (pp < e) {
          cd[u] = p.code[pp];
          ri[u] = dense ? pp - lo : static_cast<int64_t>(p.row[pp]);
          m[u] = 1;
        }
      }
      if (p.mult) {
#pragma unroll
        for (int u = 0; u < kFlight; ++u)
          if (m[u]) m[u] = p.mult[ri[u]];
      }
#pragma unroll
      for (int u = 0; u < kFlight; ++u) {
        if (m[u] <= 0) continue;
        const float fm = static_cast<float>(m[u]);
        if (cd[u] < rest) {
          add_shell(p, mine, b0, nb, cd[u], ri[u], fm);
          if (p.rest_from_total) add_shell(p, mine, b0, nb, rest, ri[u], fm);     // the listed sum, at the rest shell's weight
        } else if (!p.rest_from_total) {
          add_shell(p, mine, b0, nb, rest, ri[u], fm);                            // a code past the cover: the rest shell
        }
      }
    }
    float out = 0.f;
    for (int s = 0; s < nb; ++s) {
      const float t = wave_sum(mine[s * kLanes]);
      if (lane == s) out = t;
    }
    if (lane < nb) dst[b0 + lane] = out;
  }
}

__global__ __launch_bounds__(kThreads) void cols_combine_kernel(const Params p) {
  const int64_t e = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (e >= p.n_cols * p.bins) return;
  const int64_t q = e / p.bins, bin = e - q * p.bins;
  int64_t first = q * p.uniform_chunks;
  int64_t nch = p.uniform_chunks;
  if (p.item_ptr) {
    first = p.item_ptr[q];
    nch = p.item_ptr[q + 1] - p.item_ptr[q];
  }
  float v = nch > 1 ? ordered_sum(p.part + first * p.bins + bin, p.bins, nch) : p.V[e];
  const int64_t rest0 = static_cast<int64_t>(p.D - 1) * p.Cw;
  if (p.rest_from_total && bin >= rest0) v = p.T[bin - rest0] - v;
  p.V[e] = v;
}

__global__ __launch_bounds__(kThreads) void cols_scale_kernel(const Params p) {
  const int d = blockIdx.y;
  const int64_t q0 = static_cast<int64_t>(blockIdx.x) * p.spb;
  const int64_t left = p.n_cols - q0;
  const int np = left < p.spb ? static_cast<int>(left) : p.spb;
  const int n = np * p.W;                            // spb * W <= max(kScaleElems, W)
  for (int le = threadIdx.x; le < n; le += kThreads) {
    const int pl = le / p.W, w = le - pl * p.W;
    const int64_t q = q0 + pl;
    const int64_t j = p.col_ids ? p.col_ids[q] : q;
    float b = 0.f;
    if (j >= 0 && j < p.n_src) b = p.V[q * p.bins + static_cast<int64_t>(d) * p.Cw + (w % p.Cw)] * p.S[j * p.s_stride + w];
    p.B[q * p.b_stride + static_cast<int64_t>(d) * p.W + w] = b;
  }
}

int64_t longest_col(const gnan_attr_cols_args* a) { return a->rowptr_t == nullptr ? a->n_rows : a->max_col_pairs; }

int64_t chunks_of(int64_t pairs) { return pairs <= kChunk ? 1 : (pairs + kChunk - 1) / kChunk; }

int64_t item_count(const gnan_attr_cols_args* a) { return a->item_ptr ? a->n_items : a->n_cols * chunks_of(longest_col(a)); }

int64_t bins_of(const gnan_attr_cols_args* a) { return static_cast<int64_t>(a->D) * a->Cw; }

int64_t t_blocks_of(const gnan_attr_cols_args* a) {
  if (!a->rest_from_total) return 0;
  return a->n_rows <= 0 ? 1 : (a->n_rows + kTRows - 1) / kTRows;
}

int lds_bytes(const gnan_attr_cols_args* a) {
  const int64_t bins = bins_of(a);
  return kWaves * static_cast<int>(bins < kPassBins ? bins : kPassBins) * kLanes * static_cast<int>(sizeof(float));
}

// the workspace, in 4-byte words: mult | t_part | T | V | part
struct Layout {
  int64_t mult, t_part, T, V, part, words;
};

Layout layout_of(const gnan_attr_cols_args* a) {
  Layout l;
  const int64_t bins = bins_of(a), items = item_count(a);
  int64_t at = 0;
  l.mult = at;   at += a->n_row_ids >= 0 ? a->n_rows : 0;
  l.t_part = at; at += t_blocks_of(a) * a->Cw;
  l.T = at;      at += a->rest_from_total ? a->Cw : 0;
  l.V = at;      at += a->n_cols * bins;
  l.part = at;   at += items > a->n_cols ? items * bins : 0;
  l.words = at;
  return l;
}

// every refusal, on the host, before any HIP call
int validate(const gnan_attr_cols_args* a, const char* who, bool launch) {
  GNAN_REQUIRE(a != nullptr, "%s: null args", who);
  GNAN_REQUIRE(a->n_cols >= 0 && a->n_src >= 0 && a->n_rows >= 0, "%s: negative size (n_cols=%lld, n_src=%lld, n_rows=%lld)", who,
               static_cast<long long>(a->n_cols), static_cast<long long>(a->n_src), static_cast<long long>(a->n_rows));
  GNAN_REQUIRE(a->W >= 1, "%s: W must be >= 1 (got %d)", who, a->W);
  if (a->D < 2 || a->D > GNAN_MAX_CODES)
    return gnan::fail(GNAN_ERR_UNSUPPORTED, "%s: covers 2 <= D <= %d hop codes (got D=%d)", who, GNAN_MAX_CODES, a->D);
  GNAN_REQUIRE(a->Cw >= 1 && a->W % a->Cw == 0, "%s: Cw must divide W (got Cw=%d, W=%d)", who, a->Cw, a->W);
  GNAN_REQUIRE((a->rowptr_t == nullptr) == (a->row == nullptr), "%s: rowptr_t and row must both be set (CSR) or both NULL (dense)", who);
  GNAN_REQUIRE(a->lut_row_stride == 0 || a->lut_row_stride >= static_cast<int64_t>(a->D) * a->Cw,
               "%s: lut_row_stride must be 0 (one table) or at least D * Cw", who);
  GNAN_REQUIRE(a->s_stride >= a->W, "%s: operand row stride smaller than W", who);
  GNAN_REQUIRE(a->b_stride >= static_cast<int64_t>(a->D) * a->W, "%s: output row stride smaller than D * W", who);
  GNAN_REQUIRE(a->cnt == nullptr || a->cnt_stride >= a->D, "%s: cnt row stride smaller than D", who);
  GNAN_REQUIRE(a->nnz >= 0 && a->max_col_pairs >= 0, "%s: negative nnz / max_col_pairs", who);
  GNAN_REQUIRE(a->n_row_ids <= 0 || a->row_ids != nullptr, "%s: null row_ids beside n_row_ids=%lld", who, static_cast<long long>(a->n_row_ids));
  GNAN_REQUIRE(a->item_ptr == nullptr || a->n_items >= a->n_cols, "%s: item_ptr lists at least one work item per source (n_items=%lld, n_cols=%lld)",
               who, static_cast<long long>(a->n_items), static_cast<long long>(a->n_cols));
  if (item_count(a) > 0x7fffffffLL)
    return gnan::fail(GNAN_ERR_UNSUPPORTED, "%s: %lld work items exceed one launch (limit %lld): request the sources in batches", who,
                      static_cast<long long>(item_count(a)), 0x7fffffffLL);
  if (a->n_cols * bins_of(a) > 0x7fffffffLL * kThreads)
    return gnan::fail(GNAN_ERR_UNSUPPORTED, "%s: %lld (source, shell, channel) sums exceed one launch (limit %lld): request the sources in batches",
                      who, static_cast<long long>(a->n_cols * bins_of(a)), 0x7fffffffLL * kThreads);
  if (!launch) return GNAN_OK;
  GNAN_REQUIRE(a->code && a->S && a->lut && a->B, "%s: null code / S / lut / B", who);
  const size_t need = gnan_attr_cols_workspace_bytes(a);
  if (need && (a->workspace == nullptr || a->workspace_bytes < need))
    return gnan::fail(GNAN_ERR_WORKSPACE, "%s: workspace %zu B < required %zu B", who, a->workspace ? a->workspace_bytes : size_t{0}, need);
  GNAN_REQUIRE(need == 0 || reinterpret_cast<uintptr_t>(a->workspace) % 4 == 0, "%s: workspace must be 4-byte aligned", who);
  return GNAN_OK;
}

int launches_of(const gnan_attr_cols_args* a) {
  if (a->n_cols == 0) return 0;
  int n = 2;                                                                 // walk, scale
  if (a->n_row_ids >= 0) n += a->n_row_ids > 0 ? 2 : 1;                      // fill, count
  if (a->rest_from_total) n += 2;                                            // T by blocks, T
  if (a->rest_from_total || item_count(a) > a->n_cols) n += 1;               // combine
  return n;
}

}  // namespace

extern "C" size_t gnan_attr_cols_workspace_bytes(const gnan_attr_cols_args* a) {
  if (a == nullptr || a->n_cols <= 0 || a->W < 1 || a->D < 1 || a->Cw < 1 || a->n_rows < 0) return 0;
  return static_cast<size_t>(layout_of(a).words) * sizeof(float);
}

extern "C" int gnan_attr_cols_describe(const gnan_attr_cols_args* a, gnan_attr_cols_info* out) {
  GNAN_REQUIRE(out != nullptr, "attr_cols_describe: null info");
  if (int rc = validate(a, "attr_cols_describe", false)) return rc;
  out->chunk_pairs = kChunk;
  out->bin_passes = static_cast<int32_t>((bins_of(a) + kPassBins - 1) / kPassBins);
  out->block_size = kThreads;
  out->items_per_block = kWaves;
  out->launches = launches_of(a);
  out->lds_bytes = lds_bytes(a);
  out->t_block_rows = kTRows;
  out->t_blocks = t_blocks_of(a);
  out->max_col_chunks = chunks_of(longest_col(a));
  out->n_items = item_count(a);
  out->workspace_bytes = gnan_attr_cols_workspace_bytes(a);
  return GNAN_OK;
}

extern "C" int gnan_attr_cols(const gnan_attr_cols_args* a, gnan_stream_t stream) {
  if (int rc = validate(a, "attr_cols", true)) return rc;
  if (a->n_cols == 0) return GNAN_OK;
  const Layout l = layout_of(a);
  float* ws = static_cast<float*>(a->workspace);
  Params p;
  p.n_cols = a->n_cols; p.n_src = a->n_src; p.n_rows = a->n_rows;
  p.rowptr_t = a->rowptr_t; p.rowptr_is64 = a->rowptr_is64; p.row = a->row; p.code = a->code;
  p.col_ids = a->col_ids; p.row_ids = a->row_ids; p.n_row_ids = a->n_row_ids;
  p.S = a->S; p.W = a->W; p.s_stride = a->s_stride;
  p.lut = a->lut; p.lut_row_stride = a->lut_row_stride; p.D = a->D; p.Cw = a->Cw;
  p.cnt = a->cnt; p.cnt_stride = a->cnt_stride; p.rest_from_total = a->rest_from_total;
  p.B = a->B; p.b_stride = a->b_stride;
  p.item_ptr = a->item_ptr; p.n_items = item_count(a);
  p.uniform_chunks = static_cast<int>(chunks_of(longest_col(a)));
  p.bins = bins_of(a);
  p.cap = static_cast<int>(p.bins < kPassBins ? p.bins : kPassBins);
  p.t_blocks = t_blocks_of(a);
  p.spb = a->W >= kScaleElems ? 1 : kScaleElems / a->W;
  p.mult = a->n_row_ids >= 0 ? reinterpret_cast<int32_t*>(ws + l.mult) : nullptr;
  p.t_part = ws + l.t_part; p.T = ws + l.T; p.V = ws + l.V; p.part = ws + l.part;
  hipStream_t st = static_cast<hipStream_t>(stream);
  auto blocks = [](int64_t n, int64_t per) { return static_cast<unsigned>((n + per - 1) / per); };
  if (p.mult) {
    if (p.n_rows > 0) {
      const int64_t nb = (p.n_rows + kThreads - 1) / kThreads;
      hipLaunchKernelGGL(cols_fill_kernel, dim3(static_cast<unsigned>(nb < 4096 ? nb : 4096)), dim3(kThreads), 0, st, p.mult, p.n_rows);
      if (int rc = gnan::check_launch("cols_fill_kernel")) return rc;
    }
    if (p.n_row_ids > 0 && p.n_rows > 0) {
      hipLaunchKernelGGL(cols_count_kernel, dim3(blocks(p.n_row_ids, kThreads)), dim3(kThreads), 0, st, p);
      if (int rc = gnan::check_launch("cols_count_kernel")) return rc;
    }
  }
  if (p.rest_from_total) {
    hipLaunchKernelGGL(cols_total_kernel, dim3(static_cast<unsigned>(p.t_blocks)), dim3(kThreads), 0, st, p);
    if (int rc = gnan::check_launch("cols_total_kernel")) return rc;
    hipLaunchKernelGGL(cols_total_finish_kernel, dim3(blocks(p.Cw, kThreads)), dim3(kThreads), 0, st, p);
    if (int rc = gnan::check_launch("cols_total_finish_kernel")) return rc;
  }
  hipLaunchKernelGGL(cols_walk_kernel, dim3(blocks(p.n_items, kWaves)), dim3(kThreads), lds_bytes(a), st, p);
  if (int rc = gnan::check_launch("cols_walk_kernel")) return rc;
  if (p.rest_from_total || p.n_items > p.n_cols) {
    hipLaunchKernelGGL(cols_combine_kernel, dim3(blocks(p.n_cols * p.bins, kThreads)), dim3(kThreads), 0, st, p);
    if (int rc = gnan::check_launch("cols_combine_kernel")) return rc;
  }
  hipLaunchKernelGGL(cols_scale_kernel, dim3(blocks(p.n_cols, p.spb), static_cast<unsigned>(p.D)), dim3(kThreads), 0, st, p);
  return gnan::check_launch("cols_scale_kernel");
}
