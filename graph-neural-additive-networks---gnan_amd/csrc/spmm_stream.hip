// The pair stream of the reference-order inference route (gnan_spmm_args.stream_*, HopGraph.pair_stream_plan): the rows between the tiles
// and the hubs as one queue of pairs per column class, sorted by the columns' popularity block and cut into chunks.
//
// seg_body (csrc/spmm_fwd_body.hpp) pays per segment for a row id, two bounds, a weight row and an index round of its own, and a wave runs
// as long as the longest of its segments: a segment per (row, class, block) of a row of 5 .. 512 pairs holds 1.4 .. 3.8 pairs, too few
// to carry that.  Here a lane group owns a CHUNK of the queue instead — its start is arithmetic — and walks it 16 entries per round
// whatever rows they belong to: no row id, no bounds, no weight is loaded (every pair of the stream carries one hop code, so the weight is
// applied once per row, in the combine).  A segment is a maximal run of one row inside a chunk; the entry that ends one carries bit 31,
// and there the group reduces its accumulators to ONE float.  The floats lie in QUEUE order — segment s of the plan's enumeration at
// partial[s], chunk t's k-th at partial[chunk_first_seg[t] + k] — so a class's partials form one region that its XCD writes nearly
// sequentially: lane kr of the group keeps the round's kr-th float and the round ends with one store of all of them.  The gathers of a
// batch are issued whatever segment they belong to, so they stay in flight across segment ends.
// Workgroup b takes class b & 7 (the XCD's L2 then holds one eighth of the hot operand rows) and its lane groups consecutive chunks, so
// a class's queue runs in popularity-block order, most listed first.  A code object of its own: the aggregation's other kernels keep
// their registers.  No LDS, no barrier, no atomics.
//
// The combine finds a row's floats through row_seg (the row's segments, in queue order).  A workgroup takes kCombineRows consecutive
// stream rows: their entries of row_seg are ONE range, which the workgroup walks in entry order, kCombineCap entries a tile — row_seg
// read coalesced, partial[row_seg[s]] gathered into the entry's place of an LDS tile.  A block's gathers fall into its few (class,
// block) windows of partial and are issued together, so a line is fetched once (a thread per row walking its own run touched the
// same lines again many iterations later, after other waves' traffic: 1.9 times the bytes).  Behind a barrier thread i adds its row's
// floats from the tile in row_seg order, keeping its sum and its place across tiles.  No atomics, nothing between workgroups.
//
// The range may run to the last row (gnan_spmm_args.q_hub): a class's queue then ends with the hub rows' pairs, which the stream's kernel
// takes like any other, and the hub rows — thousands of segments each — get a combine of their own, a wave per row
// (spmm_stream_hub_combine_kernel below); the combine above takes the rows in front of them.
#include "spmm_common.hpp"

namespace {

struct StreamParams {
  const float* S;
  int W;
  int64_t s_stride;
  const int32_t* index;
  const int32_t* cls_pair_ptr;
  const int32_t* cls_chunk_ptr;
  const int32_t* chunk_first_seg;
  const int32_t* row_seg;        // [n_seg] a row's segments (queue-order numbers), rows in turn
  const int32_t* row_slot_ptr;   // [n_rows + 1] into row_seg
  float* partial;     // [n_seg] in queue order
  int64_t q_lo;
  int n_rows;         // rows of the stream
  int n_seg;
  int chunk;
  int code;
};

constexpr unsigned kStreamLast = 1u << 31;

// (the lane group's sum over its LPR lanes: group_sum, csrc/spmm_common.hpp)
template <int LPR>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8)))
void spmm_stream_kernel(const StreamParams p) {
  static_assert(LPR >= 16, "a DPP row per lane group, one index entry per lane and round");
  constexpr int VEC = 4;
  constexpr int G = kWave / LPR;
  constexpr int IW = 16;    // index entries per round
  constexpr int FLY = 4;    // gathers in flight per lane
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x / kWave;
  const int sub = lane % LPR;
  const int slot = lane / LPR;
  const int cls = static_cast<int>(blockIdx.x) & 7;
  const int t0 = p.cls_chunk_ptr[cls];
  const int g = ((static_cast<int>(blockIdx.x) >> 3) * 4 + wave) * G + slot;    // the group's chunk of this class's queue
  if (g >= p.cls_chunk_ptr[cls + 1] - t0) return;   // (the whole group)
  const int64_t lo = p.cls_pair_ptr[cls] + static_cast<int64_t>(g) * p.chunk;
  const int64_t left = p.cls_pair_ptr[cls + 1] - lo;
  const int n = static_cast<int>(left < p.chunk ? left : p.chunk);    // (the class's last chunk may be short)
  const int32_t* idx = p.index + lo;
  const int seg0 = p.chunk_first_seg[t0 + g];
  const bool col_ok = sub * VEC < p.W;
  const float* Sl = p.S + (col_ok ? sub * VEC : 0);   // (a lane past the columns reads column 0, dropped below)
  Vec<VEC> acc;
#pragma unroll
  for (int v = 0; v < VEC; ++v) acc.v[v] = 0.f;
  int k = 0;                                           // segments of the chunk flushed so far
  int next = 0;
  if (sub < IW && sub < n) next = idx[sub];
  for (int base = 0; base < n; base += IW) {
    const int m = n - base < IW ? n - base : IW;
    const int ent = next;
    next = 0;
    if (sub < IW && base + IW + sub < n) next = idx[base + IW + sub];
    int kr = 0;                                        // ... of this round
    float keep = 0.f;                                  // lane kr: the float of the round's kr-th finished segment
#pragma unroll
    for (int j0 = 0; j0 < IW; j0 += FLY) {
      if (j0 >= m) break;
      Vec<VEC> sv[FLY];
#pragma unroll
      for (int u = 0; u < FLY; ++u) {   // no branch around a gather: a slot past the end reads the chunk's last row again, dropped below
        const int j = j0 + u < m ? j0 + u : m - 1;
        const unsigned en = static_cast<unsigned>(__shfl(ent, j, LPR));
        sv[u] = load_vec<VEC>(Sl + static_cast<int64_t>(en & kPackMask) * p.s_stride);
      }
#pragma unroll
      for (int u = 0; u < FLY; ++u) {
        const bool ok = j0 + u < m;
        const unsigned en = static_cast<unsigned>(__shfl(ent, ok ? j0 + u : m - 1, LPR));
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc.v[v] = ok ? acc.v[v] + sv[u].v[v] : acc.v[v];   // (a select: 0 * inf would be a NaN)
        if (ok && (en & kStreamLast)) {   // (uniform over the lane group)
          float r = (acc.v[0] + acc.v[1]) + (acc.v[2] + acc.v[3]);
          r = col_ok ? r : 0.f;
          r = group_sum<LPR>(r);
          keep = sub == kr ? r : keep;                 // (group_sum leaves the sum in every lane)
          ++kr;
#pragma unroll
          for (int v = 0; v < VEC; ++v) acc.v[v] = 0.f;
        }
      }
    }
    // a round ends at most IW segments: one store of their floats, consecutive in queue order
    if (sub < kr && seg0 + k + sub < p.n_seg) p.partial[seg0 + k + sub] = keep;
    k += kr;
  }
}

// combine: workgroup b takes the stream rows [b * kCombineRows, (b + 1) * kCombineRows), thread i row b * kCombineRows + i — the floats of
// its segments row_seg[row_slot_ptr[r] .. row_slot_ptr[r + 1]) in that order (the queue's: the chain the row-major slots gave), the one
// weight, the rest and self terms as spmm_seg_combine_kernel forms them:
//   Y[row] =fmaf(w_0 - w_rest, a_i, fmaf(w_rest, T, (w_code - w_rest) * (((p_0 + p_1) + p_2) + ...)))
// The block's entries [row_slot_ptr[r0], row_slot_ptr[r0 + rows)) pass through the LDS tile kCombineCap at a time, staged in entry order
// by all 256 threads (entry j of the tile by thread j & 255); a row may straddle a tile's edge, and a row of 512 pairs alone can list
// more entries than a tile holds.  Both barriers of a tile are reached by every thread (the trip count is the block's).
// One fixed shape per row, decided by the plan alone: bit-reproducible.
constexpr int kCombineRows = 256;    // stream rows per workgroup (at most the 256 threads)
constexpr int kCombineCap = 4096;    // entries per LDS tile (16 KB)

__global__ __launch_bounds__(256) void spmm_stream_combine_kernel(const Params p, const StreamParams sp) {
  static_assert(kCombineRows <= 256 && kCombineCap % 256 == 0, "a thread per row, whole passes of the workgroup over a tile");
  constexpr int FLY = 4;    // gathers in flight per thread
  __shared__ float tile[kCombineCap];
  const int t = static_cast<int>(threadIdx.x);
  const int r0 = static_cast<int>(blockIdx.x) * kCombineRows;
  const int rows = sp.n_rows - r0 < kCombineRows ? sp.n_rows - r0 : kCombineRows;    // (the last block may be short)
  const bool mine = t < rows;
  const int64_t q = sp.q_lo + r0 + (mine ? t : 0);
  const int64_t o = out_row(p, q, q);
  int s = 0, s1 = 0;    // the row's next entry and its end; a thread without a row adds nothing
  if (mine) { s = sp.row_slot_ptr[r0 + t]; s1 = sp.row_slot_ptr[r0 + t + 1]; }
  const int e0 = sp.row_slot_ptr[r0], e1 = sp.row_slot_ptr[r0 + rows];
  float y = 0.f;
  for (int base = e0; base < e1; base += kCombineCap) {
    const int m = e1 - base < kCombineCap ? e1 - base : kCombineCap;
    const int32_t* seg = sp.row_seg + base;
    for (int j0 = t; j0 < m; j0 += 256 * FLY) {
      int sg[FLY];
      float v[FLY];
#pragma unroll
      for (int u = 0; u < FLY; ++u) {   // no branch around a load: a slot past the end reads the tile's last entry again, dropped below
        const int j = j0 + 256 * u;
        sg[u] = seg[j < m ? j : m - 1];
      }
#pragma unroll
      for (int u = 0; u < FLY; ++u) v[u] = sp.partial[sg[u]];
#pragma unroll
      for (int u = 0; u < FLY; ++u) {
        const int j = j0 + 256 * u;
        if (j < m) tile[j] = v[u];
      }
    }
    __syncthreads();
    const int hi = s1 < base + m ? s1 : base + m;
    for (; s < hi; ++s) y += tile[s - base];
    __syncthreads();
  }
  if (mine) combine_store<true>(p, q, o, y, sp.code);
}

// combine of the hub rows at the stream's end (gnan_spmm_args.q_hub): stream rows [r_hub, sp.n_rows), a WAVE per row, four rows per
// workgroup, no barrier, no LDS.  Lane l adds partial[row_seg[s]] for s = s0 + l, s0 + l + 64, ... in that order (a hub row's segments of
// one (class, block) are consecutive floats of partial and row_seg is read coalesced), the 64 lane sums meet in spmm_hub_combine_kernel's
// fixed xor butterfly, then combine_store<true> as the rows above.  The longest C4 row owns some 7 000 segments — more than a hundred
// turns of a lane — so the loads run ahead of the adds: kHubFly gathers in flight per lane, the NEXT batch's row_seg entries requested
// before this batch's gathers are consumed (one exposed latency per batch, not two), the adds in index order whatever arrives first;
// and the waves take the rows LAST FIRST (the copy is degree-sorted: the longest rows start at once instead of forming the launch's
// tail).  One fixed shape per row, decided by the plan alone: bit-reproducible.
constexpr int kHubFly = 8;

__global__ __launch_bounds__(256) void spmm_stream_hub_combine_kernel(const Params p, const StreamParams sp, const int r_hub) {
  const int lane = threadIdx.x & (kWave - 1);
  const int k = static_cast<int>(blockIdx.x) * (blockDim.x / kWave) + static_cast<int>(threadIdx.x) / kWave;
  if (k >= sp.n_rows - r_hub) return;   // (the whole wave)
  const int r = sp.n_rows - 1 - k;
  const int s0 = sp.row_slot_ptr[r], s1 = sp.row_slot_ptr[r + 1];    // (the plan: s0 < s1 <= n_seg, a row of the stream owns a segment)
  float y = 0.f;
  int sg[kHubFly];
#pragma unroll
  for (int u = 0; u < kHubFly; ++u) {   // no branch around a load: an entry past the row's end reads its last entry again, dropped below
    const int j = s0 + lane + kWave * u;
    sg[u] = sp.row_seg[j < s1 ? j : s1 - 1];
  }
  for (int s = s0 + lane; s < s1; s += kWave * kHubFly) {
    float v[kHubFly];
#pragma unroll
    for (int u = 0; u < kHubFly; ++u) v[u] = sp.partial[sg[u]];
#pragma unroll
    for (int u = 0; u < kHubFly; ++u) {
      const int j = s + kWave * (kHubFly + u);
      sg[u] = sp.row_seg[j < s1 ? j : s1 - 1];
    }
#pragma unroll
    for (int u = 0; u < kHubFly; ++u) y = s + kWave * u < s1 ? y + v[u] : y;   // (a select: the dropped float may be anything)
  }
#pragma unroll
  for (int off = kWave / 2; off >= 1; off >>= 1) y += __shfl_xor(y, off);
  if (lane != 0) return;
  const int64_t q = sp.q_lo + r;
  combine_store<true>(p, q, out_row(p, q, q), y, sp.code);
}

StreamParams stream_params(const gnan_spmm_args* a) {
  StreamParams sp;
  sp.S = static_cast<const float*>(a->S); sp.W = a->W; sp.s_stride = a->s_stride;
  sp.index = a->stream_index; sp.cls_pair_ptr = a->stream_cls_pair_ptr; sp.cls_chunk_ptr = a->stream_cls_chunk_ptr;
  sp.chunk_first_seg = a->stream_chunk_first_seg; sp.row_seg = a->stream_row_seg; sp.row_slot_ptr = a->stream_row_slot_ptr;
  sp.partial = static_cast<float*>(a->workspace) + stream_partial_offset(a);
  sp.q_lo = a->stream_q_lo; sp.n_rows = static_cast<int>(a->stream_q_hi - a->stream_q_lo);
  sp.n_seg = a->n_stream_seg; sp.chunk = a->stream_chunk; sp.code = a->stream_code;
  return sp;
}

}  // namespace

// (validate(): the stream comes on the self_sum route, which pick_route() admits for 16 lanes or more only)
int gnan::stream_blocks(const gnan_spmm_args* a, int lpr) {
  if (a->stream_index == nullptr || lpr < 16) return 0;
  const int64_t per = 4 * static_cast<int64_t>(kWave / lpr);     // chunks per workgroup
  const int64_t nb = 8 * ((static_cast<int64_t>(a->stream_max_chunks_per_class) + per - 1) / per);
  return nb > 0x3fffffffLL ? -1 : static_cast<int>(nb);
}

int gnan::launch_stream(const gnan_spmm_args* a, int lpr, hipStream_t st) {
  if (a->stream_index == nullptr) return GNAN_OK;
  const int nb = stream_blocks(a, lpr);
  if (nb <= 0 || lpr * 4 < a->W || a->s_dtype != GNAN_F32)   // (one pass of the lane group over the columns, as the tiles)
    return gnan::fail(GNAN_ERR_UNSUPPORTED, "spmm: the pair stream needs fp32 rows read 16 B per lane by 16 lanes or more (W in (32, 256])");
  const StreamParams sp = stream_params(a);
  const dim3 grid(static_cast<unsigned>(nb)), block(256);
  if (lpr == 16) hipLaunchKernelGGL(spmm_stream_kernel<16>, grid, block, 0, st, sp);
  else if (lpr == 32) hipLaunchKernelGGL(spmm_stream_kernel<32>, grid, block, 0, st, sp);
  else hipLaunchKernelGGL(spmm_stream_kernel<64>, grid, block, 0, st, sp);
  return gnan::check_launch("spmm_stream_kernel");
}

int gnan::launch_stream_combine(const gnan_spmm_args* a, hipStream_t st) {
  if (a->stream_index == nullptr) return GNAN_OK;
  const Params p = make_params(a);
  StreamParams sp = stream_params(a);
  const int n_all = sp.n_rows;
  if (stream_takes_hubs(a)) sp.n_rows = static_cast<int>(a->q_hub - a->stream_q_lo);   // the rows in front of the hub rows (validate(): >= 1)
  const unsigned nb = static_cast<unsigned>((sp.n_rows + kCombineRows - 1) / kCombineRows);
  hipLaunchKernelGGL(spmm_stream_combine_kernel, dim3(nb), dim3(256), 0, st, p, sp);
  if (int rc = gnan::check_launch("spmm_stream_combine_kernel")) return rc;
  if (sp.n_rows == n_all) return GNAN_OK;
  const int r_hub = sp.n_rows;      // ... and the hub rows [r_hub, n_all) behind them, a wave each
  sp.n_rows = n_all;
  hipLaunchKernelGGL(spmm_stream_hub_combine_kernel, dim3(static_cast<unsigned>((n_all - r_hub + 3) / 4)), dim3(256), 0, st, p, sp, r_hub);
  return gnan::check_launch("spmm_stream_hub_combine_kernel");
}
