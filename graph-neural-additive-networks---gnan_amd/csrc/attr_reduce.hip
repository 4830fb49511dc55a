// Attributions reduced over groups of rows: the moments  sum a, sum |a|, sum a^2  of gnan_attr_rows' terms a[q, d, w] over groups of
// requested rows, plus the same moments of a row's total over the shells — M [G, 3, D + 1, W] in float64 (include/gnan_hip.h has
// the definition).  The [R, D, W] array is never written.  Three launches, no atomics of any kind, no workgroup waits for another:
//
//   attr_reduce_long_kernel     rows of more than kChunk pairs only: one wave per (chunk of the row, tile of 64 operand columns)
//                               walks the chunk and leaves the raw shell sums in the workspace, [item, D, W] floats.
//   attr_reduce_block_kernel    one workgroup per (block of kBlockRows = 32 consecutive requested rows, tile of 64 columns).  A WAVE
//                               takes a row at a time (rows wave, wave + 4, ... of the block): lanes own operand columns (where
//                               W < 64, 64 / Wp pair slots share the row's pairs, as in attr_rows.hip), eight gathers in flight,
//                               lane-private float accumulators per shell in LDS.  Shells go in passes of kPass = 8.  When a pass of
//                               a row is complete the shell sums are combined in a fixed order (slots in slot order, or a long row's
//                               chunks in chunk order), the rest shell is formed from s_total, the weight is applied once, and the
//                               float32 term goes, as a double, into the wave's moments: 3 * 8 doubles in registers, plus the row's
//                               running total over the shells (a register; LDS between passes).  After the block's rows the four
//                               waves' moments are added in wave order through LDS and the block's partial is stored.
//   attr_reduce_combine_kernel  one workgroup of 16 waves per (group, 64 elements of [3, D + 1, W]): wave r adds the r-th run of
//                               consecutive blocks of the group in block order, the runs are added in run order.
//
// The sum of a shell's m pairs passes at most m - 1 rounded float additions whatever the slot / chunk tree (every accumulator starts
// at +0, 0 + x is exact), the weight adds a division and a product: the same k = m + 1 (m' + 2 for the rest shell from s_total) as
// attr_rows.hip.  A float's double square is exact, so the float64 additions are the only roundings after the term.
// A block's layout follows from its group's first row alone, so a group's bits depend on its own rows in their order only.
#include "common.hpp"

namespace {

constexpr int kThreads = 256, kWaves = 4, kTile = 64, kPass = 8, kFlight = 8;
constexpr int kChunk = 64;                   // pairs a wave walks for one row of its block (8 rounds of eight gathers at W >= 64); longer rows go
                                             // through the workspace in chunks of as many, a wave each (an R-MAT graph's first rows are all a few hundred
                                             // pairs long: with 512 pairs and blocks of 64 rows one wave walked 16 of them in turn, 1.53 ms for all rows of
                                             // the arxiv shape at W = 129 against 1.07 ms with 64 pairs and 32 rows)
constexpr int kBlockRows = 32;               // eight rows per wave: the slowest block's tail against 3 * (D + 1) * W doubles of partials per block
constexpr int kRuns = 16, kCombineThreads = kRuns * 64;
constexpr int kMom = 3 * kPass + 3;          // moments of a pass's shells + the all-distances slot

struct Params {
  int64_t n_rows, n_cols;
  const void* rowptr;
  int rowptr_is64;
  const int32_t* col;
  const uint8_t* code;
  const int32_t* row_ids;
  const float* S;
  int W;
  int64_t s_stride;
  const float* lut;
  int64_t lut_row_stride;
  int D, Cw;
  const int32_t* cnt;
  int64_t cnt_stride;
  const float* s_total;
  const int64_t* block_ptr;
  const int64_t* group_block_ptr;
  int64_t n_blocks, block_first;
  const int32_t* item_ptr;     // [n_rows + 1] or NULL: every row has `uniform_chunks` items (0: no row is long)
  int64_t item_first;
  int uniform_chunks;
  const float* ws_in;
  float* ws;                   // [this call's items, D, W] raw shell sums of the chunks of long rows
  double* partials;            // [n_blocks, 3, D + 1, W]
  double* M;
  int Wp, slots, tiles, passes, block_rows;
};

__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ void row_range(const Params& p, int64_t i, int64_t* lo, int64_t* hi) {
  if (p.rowptr == nullptr) {
    *lo = i * p.n_cols;
    *hi = *lo + p.n_cols;
  } else if (p.rowptr_is64) {
    *lo = static_cast<const int64_t*>(p.rowptr)[i];
    *hi = static_cast<const int64_t*>(p.rowptr)[i + 1];
  } else {
    *lo = static_cast<const int32_t*>(p.rowptr)[i];
    *hi = static_cast<const int32_t*>(p.rowptr)[i + 1];
  }
}

// the chunk items of requested row q: its first item and how many (0 or 1: the row is walked by one wave of the block kernel)
__device__ __forceinline__ void row_items(const Params& p, int64_t q, int64_t* first, int* nch) {
  if (p.item_ptr) {
    *first = p.item_ptr[q];
    *nch = p.item_ptr[q + 1] - p.item_ptr[q];
  } else {
    *first = q * p.uniform_chunks;
    *nch = p.uniform_chunks;
  }
}

// Pairs [b, e) of a row, shells sh0 .. sh0 + sh_n - 1, this lane's column: the slots of the wave share the pairs round-robin, eight
// gathers in flight; `mine` is the lane's own word of shell 0 of the pass (+ shell * 64).
__device__ __forceinline__ void wave_gather(const Params& p, float* mine, int64_t b, int64_t e, bool dense, int64_t col0,
                                            const float* Sw, int sh0, int sh_n, int slot) {
  const int rest = p.D - 1;
  for (int64_t p0 = b + slot; p0 < e; p0 += static_cast<int64_t>(kFlight) * p.slots) {
    int sh[kFlight];
    int64_t cj[kFlight];
    float v[kFlight];
#pragma unroll
    for (int u = 0; u < kFlight; ++u) {
      const int64_t pp = p0 + static_cast<int64_t>(u) * p.slots;
      sh[u] = -1;
      cj[u] = 0;
      if (pp < e) {
        const int cd = p.code[pp];
        sh[u] = (cd < rest ? cd : rest) - sh0;                                 // a code past the cover: the rest shell
        cj[u] = dense ? pp - col0 : static_cast<int64_t>(p.col[pp]);
      }
    }
#pragma unroll
    for (int u = 0; u < kFlight; ++u) v[u] = (sh[u] >= 0 && sh[u] < sh_n) ? Sw[cj[u] * p.s_stride] : 0.f;
#pragma unroll
    for (int u = 0; u < kFlight; ++u)
      if (sh[u] >= 0 && sh[u] < sh_n) mine[sh[u] * 64] += v[u];
  }
}

// the slots' sums of one shell in slot order
__device__ __forceinline__ float slot_sum(const float* src, int slots, int Wp) {
  float z = src[0];
  for (int sl = 1; sl < slots; ++sl) z += src[sl * Wp];
  return z;
}

// base[0] + base[stride] + ... + base[(n - 1) * stride], added strictly in that order, eight loads in flight (n >= 1)
__device__ __forceinline__ float ordered_sum(const float* base, int64_t stride, int n) {
  float z = base[0];
  int c = 1;
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

__global__ __launch_bounds__(64) void attr_reduce_long_kernel(const Params p) {
  __shared__ float acc[kPass * 64];
  const int lane = threadIdx.x;
  const int64_t item = p.item_first + blockIdx.x;
  int64_t q, first;
  int nch;
  if (p.item_ptr == nullptr) {
    q = item / p.uniform_chunks;
  } else {
    int64_t lo = 0, hi = p.n_rows - 1;                 // the last q with item_ptr[q] <= item
    while (lo < hi) {
      const int64_t mid = (lo + hi + 1) >> 1;
      if (static_cast<int64_t>(p.item_ptr[mid]) <= item) lo = mid; else hi = mid - 1;
    }
    q = lo;
  }
  row_items(p, q, &first, &nch);
  const int c = static_cast<int>(item - first);
  if (c < 0 || c >= nch) return;                       // an inconsistent plan: nothing to walk
  const int64_t i = p.row_ids ? p.row_ids[q] : q;
  int64_t lo, hi;
  row_range(p, i, &lo, &hi);
  // chunk c of the row: kChunk pairs from lo + c * kChunk; the row's LAST item takes whatever is left
  int64_t b = lo + static_cast<int64_t>(c) * kChunk;
  if (b > hi) b = hi;
  int64_t e = b + kChunk;
  if (e > hi || c == nch - 1) e = hi;
  const bool dense = p.rowptr == nullptr;
  float* dst = p.ws + (item - p.item_first) * (static_cast<int64_t>(p.D) * p.W);
  const int slot = lane / p.Wp, cit = lane - slot * p.Wp;
  float* mine = acc + lane;
  for (int tile = blockIdx.y; tile < p.tiles; tile += gridDim.y) {
    const int w = tile * kTile + cit;
    const bool live = w < p.W;
    for (int sh0 = 0; sh0 < p.D; sh0 += kPass) {
      const int sh_n = p.D - sh0 < kPass ? p.D - sh0 : kPass;
      for (int s = 0; s < sh_n; ++s) mine[s * 64] = 0.f;
      if (live) wave_gather(p, mine, b, e, dense, lo, p.S + w, sh0, sh_n, slot);
      wave_sync();
      if (live && slot == 0)
        for (int s = 0; s < sh_n; ++s) dst[static_cast<int64_t>(sh0 + s) * p.W + w] = slot_sum(acc + s * 64 + cit, p.slots, p.Wp);
      wave_sync();
    }
  }
}

__global__ __launch_bounds__(kThreads) void attr_reduce_block_kernel(const Params p) {
  extern __shared__ double smem[];
  const bool multi = p.passes > 1;
  const int rpw = p.block_rows / kWaves;               // rows of a block per wave
  double* comb = smem;                                 // [kMom][64]: the waves' moments, added in wave order
  double* ts = comb + kMom * 64;                       // [kWaves][rpw][64]: a row's running total between passes (multi-pass only)
  float* lst = reinterpret_cast<float*>(ts + (multi ? kWaves * rpw * 64 : 0));   // the same for the listed sum
  float* acc = lst + (multi ? kWaves * rpw * 64 : 0);  // [kWaves][kPass][64]
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);       // uniform: a row's range, id and items stay in scalar registers
  const int64_t block = p.block_first + blockIdx.x;
  int64_t r0 = p.block_ptr ? p.block_ptr[block] : block * p.block_rows;
  int64_t r1 = p.block_ptr ? p.block_ptr[block + 1] : r0 + p.block_rows;
  if (r0 < 0) r0 = 0;
  if (r1 > r0 + p.block_rows) r1 = r0 + p.block_rows;  // the per-row state in LDS holds block_rows rows
  if (r1 > p.n_rows) r1 = p.n_rows;
  const bool dense = p.rowptr == nullptr;
  const int slot = lane / p.Wp, cit = lane - slot * p.Wp;
  float* mine = acc + wave * kPass * 64 + lane;
  const int rest = p.D - 1;
  const int64_t dw = static_cast<int64_t>(p.D) * p.W;
  const int64_t d1w = static_cast<int64_t>(p.D + 1) * p.W;

  for (int tile = blockIdx.y; tile < p.tiles; tile += gridDim.y) {
    const int w = tile * kTile + cit;
    const bool live = w < p.W;
    const bool owner = live && slot == 0;
    double al0 = 0., al1 = 0., al2 = 0.;               // moments of the rows' totals over the shells
    for (int pass = 0; pass < p.passes; ++pass) {
      const int sh0 = pass * kPass;
      const int sh_n = p.D - sh0 < kPass ? p.D - sh0 : kPass;
      const bool last = pass == p.passes - 1;
      double m0[kPass], m1[kPass], m2[kPass];
#pragma unroll
      for (int s = 0; s < kPass; ++s) m0[s] = m1[s] = m2[s] = 0.;
      int k = 0;
      for (int64_t q = r0 + wave; q < r1; q += kWaves, ++k) {
        const int64_t i = p.row_ids ? p.row_ids[q] : q;
        int64_t lo, hi, first;
        int nch;
        row_range(p, i, &lo, &hi);
        row_items(p, q, &first, &nch);
        if (nch <= 1) {
          for (int s = 0; s < sh_n; ++s) mine[s * 64] = 0.f;
          if (live) wave_gather(p, mine, lo, hi, dense, lo, p.S + w, sh0, sh_n, slot);
        } else {                                       // a long row: its chunks' sums in chunk order, in the first slot's words (the other slots add +0)
          const float* part = p.ws_in + (first - p.item_first) * dw + static_cast<int64_t>(sh0) * p.W + w;
          for (int s = 0; s < sh_n; ++s) mine[s * 64] = (live && slot == 0) ? ordered_sum(part + static_cast<int64_t>(s) * p.W, dw, nch) : 0.f;
        }
        wave_sync();
        float listed = 0.f;                            // the shells below the rest shell, in shell order
        double t = 0.;                                 // the row's terms, in shell order
        const int cell = (wave * rpw + k) * 64 + lane;
        if (pass > 0) {
          listed = lst[cell];
          t = ts[cell];
        }
        if (live) {
          const float* wr = p.lut + i * p.lut_row_stride + (w % p.Cw);
#pragma unroll
          for (int s = 0; s < kPass; ++s) {
            if (s < sh_n) {
              const int d = sh0 + s;
              float z = slot_sum(acc + (wave * kPass + s) * 64 + cit, p.slots, p.Wp);
              if (d < rest) listed += z;
              else if (p.s_total) z = p.s_total[w] - listed;
              float wt = wr[static_cast<int64_t>(d) * p.Cw];
              if (p.cnt) {
                const int n = p.cnt[i * p.cnt_stride + d];
                wt = wt / static_cast<float>(n > 1 ? n : 1);
              }
              const double a = static_cast<double>(wt * z);            // the weight once, on the combined sum: attr_rows' term
              t += a;
              m0[s] += a;
              m1[s] += fabs(a);
              m2[s] += a * a;
            }
          }
        }
        if (last) {
          al0 += t;
          al1 += fabs(t);
          al2 += t * t;
        } else {
          lst[cell] = listed;
          ts[cell] = t;
        }
        wave_sync();
      }
      // the four waves in wave order: ((w0 + w1) + w2) + w3; the last one stores the block's partial
      double* out = p.partials + block * 3 * d1w + w;
      for (int wv = 0; wv < kWaves; ++wv) {
        if (wave == wv && owner) {
#pragma unroll
          for (int s = 0; s < kPass; ++s) {
            if (s < sh_n) {
#pragma unroll
              for (int j = 0; j < 3; ++j) {
                double v = j == 0 ? m0[s] : j == 1 ? m1[s] : m2[s];
                double* c = comb + (s * 3 + j) * 64 + lane;
                if (wv > 0) v = *c + v;
                if (wv < kWaves - 1) *c = v; else out[j * d1w + static_cast<int64_t>(sh0 + s) * p.W] = v;
              }
            }
          }
          if (last) {
#pragma unroll
            for (int j = 0; j < 3; ++j) {
              double v = j == 0 ? al0 : j == 1 ? al1 : al2;
              double* c = comb + (kPass * 3 + j) * 64 + lane;
              if (wv > 0) v = *c + v;
              if (wv < kWaves - 1) *c = v; else out[j * d1w + static_cast<int64_t>(p.D) * p.W] = v;
            }
          }
        }
        __syncthreads();
      }
    }
  }
}

__global__ __launch_bounds__(kCombineThreads) void attr_reduce_combine_kernel(const Params p, int64_t n_groups) {
  __shared__ double run_sum[kRuns * 64];
  const int lane = threadIdx.x & 63, run = threadIdx.x >> 6;
  const int64_t g = blockIdx.x;
  const int64_t E = 3 * static_cast<int64_t>(p.D + 1) * p.W;
  int64_t gb0 = p.group_block_ptr ? p.group_block_ptr[g] : 0;
  int64_t gb1 = p.group_block_ptr ? p.group_block_ptr[g + 1] : p.n_blocks;
  if (gb0 < 0) gb0 = 0;
  if (gb1 > p.n_blocks) gb1 = p.n_blocks;
  const int64_t nb = gb1 > gb0 ? gb1 - gb0 : 0;
  const int64_t per = (nb + kRuns - 1) / kRuns;
  int64_t b0 = gb0 + run * per, b1 = b0 + per;
  if (b1 > gb1) b1 = gb1;
  for (int64_t e0 = static_cast<int64_t>(blockIdx.y) * 64; e0 < E; e0 += static_cast<int64_t>(gridDim.y) * 64) {
    const int64_t e = e0 + lane;
    double z = 0.;
    if (e < E) {
      int64_t b = b0;
      for (; b + kFlight <= b1; b += kFlight) {
        double t[kFlight];
#pragma unroll
        for (int u = 0; u < kFlight; ++u) t[u] = p.partials[(b + u) * E + e];
#pragma unroll
        for (int u = 0; u < kFlight; ++u) z += t[u];
      }
      for (; b < b1; ++b) z += p.partials[b * E + e];
    }
    run_sum[run * 64 + lane] = z;
    __syncthreads();
    if (run == 0 && e < E) {
      double total = run_sum[lane];
      for (int r = 1; r < kRuns; ++r) total += run_sum[r * 64 + lane];
      p.M[g * E + e] = total;
    }
    __syncthreads();
  }
}

int next_pow2(int v) {
  int r = 1;
  while (r < v) r <<= 1;
  return r;
}

int block_rows_of(const gnan_attr_reduce_args*) { return kBlockRows; }

int64_t groups_of(const gnan_attr_reduce_args* a) { return a->group_ptr ? a->n_groups : 1; }

// blocks the plan must hold; group_ptr has been validated
int64_t expected_blocks(const gnan_attr_reduce_args* a) {
  const int64_t br = block_rows_of(a);
  if (a->group_ptr == nullptr) return (a->n_rows + br - 1) / br;
  int64_t n = 0;
  for (int64_t g = 0; g < a->n_groups; ++g) n += (a->group_ptr[g + 1] - a->group_ptr[g] + br - 1) / br;
  return n;
}

// position, in the list of requested rows, of the first row of block b (b == the block count: n_rows)
int64_t block_start(const gnan_attr_reduce_args* a, int64_t b) {
  const int64_t br = block_rows_of(a);
  if (a->group_ptr == nullptr) return b * br < a->n_rows ? b * br : a->n_rows;
  for (int64_t g = 0; g < a->n_groups; ++g) {
    const int64_t nb = (a->group_ptr[g + 1] - a->group_ptr[g] + br - 1) / br;
    if (b < nb) return a->group_ptr[g] + b * br;
    b -= nb;
  }
  return a->n_rows;
}

int uniform_chunks(const gnan_attr_reduce_args* a) {
  const int64_t pairs = a->rowptr == nullptr ? a->n_cols : a->max_row_pairs;
  return pairs <= kChunk ? 0 : static_cast<int>((pairs + kChunk - 1) / kChunk);
}

// this call's chunk items: the caller's range where it hands over item_ptr, else the uniform chunks of the rows of its blocks
void call_items(const gnan_attr_reduce_args* a, int64_t* first, int64_t* count) {
  if (a->item_ptr) {
    *first = a->item_first;
    *count = a->item_count;
    return;
  }
  const int64_t uc = uniform_chunks(a);
  int64_t b0 = a->block_first, b1 = a->block_first + a->block_count;
  const int64_t r0 = block_start(a, b0), r1 = block_start(a, b1);
  *first = r0 * uc;
  *count = (r1 - r0) * uc;
}

int lds_bytes(const gnan_attr_reduce_args* a) {
  int bytes = kMom * 64 * static_cast<int>(sizeof(double)) + kWaves * kPass * 64 * static_cast<int>(sizeof(float));
  if (a->D > kPass) bytes += block_rows_of(a) * 64 * static_cast<int>(sizeof(double) + sizeof(float));
  return bytes;
}

size_t partials_need(const gnan_attr_reduce_args* a, int64_t n_blocks) {
  return static_cast<size_t>(n_blocks) * 3 * (a->D + 1) * a->W * sizeof(double);
}

// every refusal, on the host, before any HIP call
int validate(const gnan_attr_reduce_args* a, const char* who, bool launch) {
  GNAN_REQUIRE(a != nullptr, "%s: null args", who);
  GNAN_REQUIRE(a->n_rows >= 0 && a->n_cols >= 0, "%s: negative size (n_rows=%lld, n_cols=%lld)", who,
               static_cast<long long>(a->n_rows), static_cast<long long>(a->n_cols));
  GNAN_REQUIRE(a->W >= 1, "%s: W must be >= 1 (got %d)", who, a->W);
  if (a->D < 2 || a->D > GNAN_MAX_CODES)
    return gnan::fail(GNAN_ERR_UNSUPPORTED, "%s: covers 2 <= D <= %d hop codes (got D=%d)", who, GNAN_MAX_CODES, a->D);
  GNAN_REQUIRE(a->Cw >= 1 && a->W % a->Cw == 0, "%s: Cw must divide W (got Cw=%d, W=%d)", who, a->Cw, a->W);
  GNAN_REQUIRE((a->rowptr == nullptr) == (a->col == nullptr), "%s: rowptr and col must both be set (CSR) or both NULL (dense)", who);
  GNAN_REQUIRE(a->lut_row_stride == 0 || a->lut_row_stride >= static_cast<int64_t>(a->D) * a->Cw,
               "%s: lut_row_stride must be 0 (one table) or at least D * Cw", who);
  GNAN_REQUIRE(a->s_stride >= a->W, "%s: operand row stride smaller than W", who);
  GNAN_REQUIRE(a->cnt == nullptr || a->cnt_stride >= a->D, "%s: cnt row stride smaller than D", who);
  GNAN_REQUIRE(a->max_row_pairs >= 0, "%s: negative max_row_pairs", who);
  if (a->group_ptr) {
    GNAN_REQUIRE(a->n_groups >= 0, "%s: negative n_groups", who);
    GNAN_REQUIRE(a->group_ptr[0] == 0, "%s: group_ptr must start at 0 (got %lld)", who, static_cast<long long>(a->group_ptr[0]));
    for (int64_t g = 0; g < a->n_groups; ++g)
      GNAN_REQUIRE(a->group_ptr[g + 1] >= a->group_ptr[g], "%s: group_ptr is not monotone at group %lld", who, static_cast<long long>(g));
    GNAN_REQUIRE(a->group_ptr[a->n_groups] == a->n_rows, "%s: group_ptr must end at the number of requested rows (got %lld, n_rows=%lld)",
                 who, static_cast<long long>(a->group_ptr[a->n_groups]), static_cast<long long>(a->n_rows));
  }
  if (!launch) return GNAN_OK;
  const int64_t nb = expected_blocks(a);
  GNAN_REQUIRE(a->n_blocks == nb, "%s: the plan must hold %lld blocks of at most %d rows (got n_blocks=%lld)", who,
               static_cast<long long>(nb), block_rows_of(a), static_cast<long long>(a->n_blocks));
  GNAN_REQUIRE(a->group_ptr == nullptr || (a->block_ptr && a->group_block_ptr), "%s: group_ptr needs block_ptr and group_block_ptr", who);
  GNAN_REQUIRE(a->block_first >= 0 && a->block_count >= 0 && a->block_first + a->block_count <= nb,
               "%s: blocks %lld .. +%lld outside the plan's %lld", who, static_cast<long long>(a->block_first),
               static_cast<long long>(a->block_count), static_cast<long long>(nb));
  GNAN_REQUIRE(a->item_ptr == nullptr || (a->item_first >= 0 && a->item_count >= 0), "%s: negative item range", who);
  int64_t i0, ic;
  call_items(a, &i0, &ic);
  if (ic > 0x7fffffffLL || a->block_count > 0x7fffffffLL)
    return gnan::fail(GNAN_ERR_UNSUPPORTED, "%s: %lld chunk items / %lld blocks exceed one launch (limit %lld): split the call at block boundaries",
                      who, static_cast<long long>(ic), static_cast<long long>(a->block_count), 0x7fffffffLL);
  GNAN_REQUIRE(groups_of(a) <= 0x7fffffffLL, "%s: %lld groups exceed one launch", who, static_cast<long long>(groups_of(a)));
  GNAN_REQUIRE(a->code && a->S && a->lut, "%s: null code / S / lut", who);
  GNAN_REQUIRE(a->partials != nullptr || nb == 0, "%s: null partials", who);
  GNAN_REQUIRE(a->partials_bytes >= partials_need(a, nb), "%s: partials %zu B < required %zu B", who, a->partials_bytes, partials_need(a, nb));
  GNAN_REQUIRE(!a->combine || a->M != nullptr || groups_of(a) == 0, "%s: null M", who);
  const size_t need = gnan_attr_reduce_workspace_bytes(a);
  if (need && (a->workspace == nullptr || a->workspace_bytes < need))
    return gnan::fail(GNAN_ERR_WORKSPACE, "%s: workspace %zu B < required %zu B", who, a->workspace ? a->workspace_bytes : size_t{0}, need);
  GNAN_REQUIRE(need == 0 || reinterpret_cast<uintptr_t>(a->workspace) % 4 == 0, "%s: workspace must be 4-byte aligned", who);
  return GNAN_OK;
}

// the block range of a describe call is whatever the caller filled in, cut to the plan
gnan_attr_reduce_args clamped(const gnan_attr_reduce_args* a) {
  gnan_attr_reduce_args c = *a;
  const int64_t nb = expected_blocks(a);
  if (c.block_first < 0) c.block_first = 0;
  if (c.block_first > nb) c.block_first = nb;
  if (c.block_count < 0) c.block_count = 0;
  if (c.block_first + c.block_count > nb) c.block_count = nb - c.block_first;
  if (c.item_first < 0) c.item_first = 0;
  if (c.item_count < 0) c.item_count = 0;
  return c;
}

}  // namespace

extern "C" size_t gnan_attr_reduce_workspace_bytes(const gnan_attr_reduce_args* a) {
  if (a == nullptr || a->n_rows <= 0 || a->W < 1 || a->D < 2) return 0;
  if (a->group_ptr) {                                  // block_start walks it: an invalid one sizes nothing
    if (a->n_groups < 0 || a->group_ptr[0] != 0 || a->group_ptr[a->n_groups] != a->n_rows) return 0;
    for (int64_t g = 0; g < a->n_groups; ++g)
      if (a->group_ptr[g + 1] < a->group_ptr[g]) return 0;
  }
  const gnan_attr_reduce_args c = clamped(a);
  int64_t i0, ic;
  call_items(&c, &i0, &ic);
  return static_cast<size_t>(ic) * a->D * a->W * sizeof(float);
}

extern "C" int gnan_attr_reduce_describe(const gnan_attr_reduce_args* a, gnan_attr_reduce_info* out) {
  GNAN_REQUIRE(out != nullptr, "attr_reduce_describe: null info");
  if (int rc = validate(a, "attr_reduce_describe", false)) return rc;
  const gnan_attr_reduce_args c = clamped(a);
  int64_t i0, ic;
  call_items(&c, &i0, &ic);
  const int64_t nb = expected_blocks(a);
  out->col_tiles = (a->W + kTile - 1) / kTile;
  out->shell_passes = (a->D + kPass - 1) / kPass;
  out->pass_shells = kPass;
  out->chunk_pairs = kChunk;
  out->block_rows = block_rows_of(a);
  out->block_size = kThreads;
  out->combine_runs = kRuns;
  out->launches = (ic > 0) + (c.block_count > 0) + (a->combine != 0 && groups_of(a) > 0);
  out->lds_bytes = lds_bytes(a);
  out->n_blocks = nb;
  out->n_long_items = ic;
  out->long_items_bytes = gnan_attr_reduce_workspace_bytes(a);
  out->partials_bytes = partials_need(a, nb);
  out->plan_int_bytes = (a->item_ptr ? static_cast<size_t>(a->n_rows + 1) * sizeof(int32_t) : 0) +
                        (a->block_ptr ? static_cast<size_t>(nb + 1) * sizeof(int64_t) : 0) +
                        (a->group_block_ptr ? static_cast<size_t>(groups_of(a) + 1) * sizeof(int64_t) : 0);
  return GNAN_OK;
}

extern "C" int gnan_attr_reduce(const gnan_attr_reduce_args* a, gnan_stream_t stream) {
  if (int rc = validate(a, "attr_reduce", true)) return rc;
  Params p;
  p.n_rows = a->n_rows; p.n_cols = a->n_cols; p.rowptr = a->rowptr; p.rowptr_is64 = a->rowptr_is64;
  p.col = a->col; p.code = a->code; p.row_ids = a->row_ids;
  p.S = a->S; p.W = a->W; p.s_stride = a->s_stride;
  p.lut = a->lut; p.lut_row_stride = a->lut_row_stride; p.D = a->D; p.Cw = a->Cw;
  p.cnt = a->cnt; p.cnt_stride = a->cnt_stride; p.s_total = a->s_total;
  p.block_ptr = a->block_ptr; p.group_block_ptr = a->group_block_ptr;
  p.n_blocks = a->n_blocks; p.block_first = a->block_first;
  p.item_ptr = a->item_ptr;
  int64_t ic;
  call_items(a, &p.item_first, &ic);
  p.uniform_chunks = a->item_ptr ? 0 : uniform_chunks(a);
  p.ws = static_cast<float*>(a->workspace);
  p.ws_in = p.ws;
  p.partials = a->partials; p.M = a->M;
  p.Wp = a->W >= kTile ? kTile : next_pow2(a->W);
  p.slots = kTile / p.Wp;
  p.tiles = (a->W + kTile - 1) / kTile;
  p.passes = (a->D + kPass - 1) / kPass;
  p.block_rows = block_rows_of(a);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const unsigned gy = static_cast<unsigned>(p.tiles < 65535 ? p.tiles : 65535);
  if (ic > 0) {
    hipLaunchKernelGGL(attr_reduce_long_kernel, dim3(static_cast<unsigned>(ic), gy), dim3(64), 0, st, p);
    if (int rc = gnan::check_launch("attr_reduce_long_kernel")) return rc;
  }
  if (a->block_count > 0) {
    hipLaunchKernelGGL(attr_reduce_block_kernel, dim3(static_cast<unsigned>(a->block_count), gy), dim3(kThreads), lds_bytes(a), st, p);
    if (int rc = gnan::check_launch("attr_reduce_block_kernel")) return rc;
  }
  const int64_t G = groups_of(a);
  if (a->combine && G > 0) {
    const int64_t ey = (3 * static_cast<int64_t>(a->D + 1) * a->W + 63) / 64;
    hipLaunchKernelGGL(attr_reduce_combine_kernel, dim3(static_cast<unsigned>(G), static_cast<unsigned>(ey < 65535 ? ey : 65535)),
                       dim3(kCombineThreads), 0, st, p, G);
    return gnan::check_launch("attr_reduce_combine_kernel");
  }
  return GNAN_OK;
}
