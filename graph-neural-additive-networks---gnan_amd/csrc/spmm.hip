// rho(distance)-weighted neighbourhood sum over a hop-coded adjacency (gfx950).
//
// Replaces GNAN.py:65-73 / models.py:368-376 (rho on N^2 pairs, normalisation, bmm, feature sum)
// and the per-node loop GNAN.py:159-170.  See include/gnan_hip.h for the contract.
//
// Mapping (wave64):  an operand row of W floats is covered by LPR lanes x VEC floats
// (16 lanes x float4 for W = 64: one 256-B row = one fully used 16-B/lane request).  A wave
// therefore holds G = 64/LPR independent lane groups:
//   * row blocks  : one group per output row, edges walked sequentially, index pairs fetched
//                   LPR at a time with one coalesced load and broadcast inside the group by
//                   ds_bpermute; no cross-lane reduction, the group stores its own row;
//   * slice blocks: hub rows (degree > long_threshold) are cut into slices; a 256-thread
//                   workgroup owns a slice, every wave streams 64 index pairs per load, its G
//                   groups stride over them, partial rows meet in LDS, and a fix-up kernel adds
//                   the slices in a fixed order (bit-reproducible, no float atomics).
// HBM-bound: per edge 4 B col + 1 B code + W*4 B gathered row; per row rowptr + W*4 B store.
//
// This file: the forward's entry points and routing, the persistent narrow kernel, the hub rows' fix-up, the combine passes of the
// classed rows and of the blocked hub segments, and the shell sums.
// spmm_kernel itself is csrc/spmm_fwd_body.hpp (an object per VEC), the pair stream's two kernels are csrc/spmm_stream.hip, the lone
// rows' kernel is csrc/spmm_lone.hip, the gradients are csrc/spmm_grad.hip, what they share is csrc/spmm_common.hpp.
#include "spmm_common.hpp"

namespace {

// ---------------------------------------------------------------------------------------------
// Narrow operand rows (W in {1, 2, 4} floats, the sum-first order of GNAN.py:157: S = f_sums) with the hottest rows in LDS.
//
// A W = 1 aggregation is one 4-byte gather per listed pair, and every gather is a request to the L2 (TCC): the kernel
// sits on the L2 request rate (10M-node R-MAT: 1.1e8 pairs in 1.0 ms = 109 G requests/s; the operand itself is 40 MB and
// never leaves the Infinity Cache).  A power-law graph sends a large share of those requests to very few rows — the
// 32 768 most listed of the 10M nodes receive 42 % of the pairs (tools/hot_coverage.py) — and the host already keeps a
// compact copy of the most listed rows behind the operand, most listed first, with the column ids of the degree-sorted
// copy pointing there (HopGraph.hot_columns).  This kernel loads the head of that copy (hot_n rows, 64 KB: the 16 384 most
// listed at W = 1, 32 % of the pairs) into LDS once per workgroup and serves their gathers from there: no L2 request at
// all for them.  Two 1024-thread workgroups per CU (32 waves, 64 VGPRs: the kernel is as much bound by the latency of its
// dependent rowptr -> index -> gather chains as by the request rate — with one workgroup and a 128-KB table it LOST 7 %),
// persistent: each loads the table once and then walks its share of the hub-row slices and of the row blocks (rows are
// degree-sorted: a round-robin share is balanced).  Sixteen waves = four "virtual" 4-wave workgroups, numbered like the
// blocks of spmm_kernel for the ordinary rows; hub slices share spmm_kernel's partial-sum layout and its fix-up kernel.
// 10M-node R-MAT, W = 1: 1.04 -> 0.91 ms.  One lane per row, the same arithmetic per row as spmm_kernel<VEC, 1, false, true, false, true>
// (weights folded with the rest bucket): ordinary rows come out bit-identical, hub rows add their pairs in another order.
// ---------------------------------------------------------------------------------------------
// Branch-free: a divergent `if (hot) ds_read else global_load` makes the compiler wait at every join, i.e. one gather in
// flight per lane (measured: 1.46 ms against 1.04 ms for the plain kernel).  Both loads are always issued — the hot lanes
// of the global load all read row hot_lo (one line: a single request per wavefront, an L1 hit), the cold lanes of the LDS
// read all read entry 0 (a broadcast) — and the value is selected afterwards.
template <int VEC>
__device__ __forceinline__ Vec<VEC> hot_gather(const Params& p, const float* hot, int c) {
  const int64_t r = static_cast<int64_t>(c) - p.hot_lo;
  const bool is_hot = r >= 0 && r < p.hot_n;
  const Vec<VEC> g = load_vec<VEC>(static_cast<const float*>(p.S) + (is_hot ? p.hot_lo : static_cast<int64_t>(c)) * VEC);
  const int rl = is_hot ? static_cast<int>(r) : 0;
  Vec<VEC> l;
  if constexpr (VEC == 4) {
    const float4 t = *reinterpret_cast<const float4*>(hot + rl * 4);
    l.v[0] = t.x; l.v[1] = t.y; l.v[2] = t.z; l.v[3] = t.w;
  } else if constexpr (VEC == 2) {
    const float2 t = *reinterpret_cast<const float2*>(hot + rl * 2);
    l.v[0] = t.x; l.v[1] = t.y;
  } else {
    l.v[0] = hot[rl];
  }
  Vec<VEC> out;
#pragma unroll
  for (int v = 0; v < VEC; ++v) out.v[v] = is_hot ? l.v[v] : g.v[v];
  return out;
}

template <int VEC>
__global__ __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(8, 8)))     // two workgroups = 32 waves per CU
void spmm_hot_kernel(const Params p) {
  extern __shared__ __attribute__((aligned(16))) float hot[];        // [hot_n * VEC]
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int sub = wave >> 2, w4 = wave & 3;                           // virtual 4-wave workgroup, wave inside it
  {
    const float* src = static_cast<const float*>(p.S) + p.hot_lo * p.s_stride;      // rows are contiguous: s_stride == W
    for (int i = tid; i < p.hot_n * VEC; i += 1024) hot[i] = src[i];
  }
  __syncthreads();
  const int rest = p.D - 1;

  // ---- hub-row slices: one WAVE per slice, a contiguous run of slices per wave -----------------------------------------
  // (a workgroup per slice as in spmm_kernel would leave 4 slices in flight per CU, and every slice starts with a chain of
  // dependent loads — which hub row, its bounds, its weights: 45 rounds of that chain cost 0.6 ms.  A wave walks its run
  // front to back, so the row of the next slice is found by stepping, not by searching; no barriers.  The partial sums of
  // a slice are added in lane order by a fixed butterfly: deterministic, though not in spmm_kernel's order.)
  {
    const int n_waves = static_cast<int>(gridDim.x) * 16;
    const int per = (p.n_slices + n_waves - 1) / n_waves;
    const int gw = static_cast<int>(blockIdx.x) * 16 + wave;
    const int s_lo = gw * per, s_hi = s_lo + per < p.n_slices ? s_lo + per : p.n_slices;
    int a = 0;
    if (s_lo < s_hi) a = slice_owner(p, s_lo);
    for (int sidx = s_lo; sidx < s_hi; ++sidx) {
      a = slice_owner_from(p, a, sidx);
      const int64_t q = p.long_rows[a];
      const int64_t i = adj_row(p, q);
      int64_t lo, hi;
      slice_range(p, i, a, sidx, lo, hi);
      const SmallW sw = small_weights(p, i);
      Vec<VEC> acc, all;
#pragma unroll
      for (int v = 0; v < VEC; ++v) acc.v[v] = all.v[v] = 0.f;
      constexpr int SF = 8;                              // pairs in flight per lane
      for (int64_t base = lo + lane; base < hi; base += SF * kWave) {
        unsigned ce[SF];
#pragma unroll
        for (int k = 0; k < SF; ++k) {
          const int64_t e = base + static_cast<int64_t>(k) * kWave;
          ce[k] = e < hi ? static_cast<unsigned>(p.col[e]) : 0u;
        }
        // no branch around a gather (a guarded region ends in s_waitcnt 0: one gather in flight): pairs past the end read the
        // first hot row — an LDS hit, no request — and are dropped by a select
        Vec<VEC> sv[SF];
#pragma unroll
        for (int k = 0; k < SF; ++k) {
          const bool ok = base + static_cast<int64_t>(k) * kWave < hi;
          sv[k] = hot_gather<VEC>(p, hot, ok ? static_cast<int>(ce[k] & kPackMask) : static_cast<int>(p.hot_lo));
        }
#pragma unroll
        for (int k = 0; k < SF; ++k) {
          const bool ok = base + static_cast<int64_t>(k) * kWave < hi;
          int d = static_cast<int>(ce[k] >> kPackShift);
          d = d < rest ? d : rest;
          const float w = sw.pick(d);
#pragma unroll
          for (int v = 0; v < VEC; ++v) {
            acc.v[v] = ok ? fmaf(w, sv[k].v[v], acc.v[v]) : acc.v[v];
            all.v[v] = ok ? all.v[v] + sv[k].v[v] : all.v[v];
          }
        }
      }
#pragma unroll
      for (int off = 1; off < kWave; off <<= 1) {
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
          acc.v[v] += __shfl_xor(acc.v[v], off);
          all.v[v] += __shfl_xor(all.v[v], off);
        }
      }
      if (lane == 0) {
        float* out = p.partial + static_cast<int64_t>(sidx) * 2 * p.W;
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
          out[v] = acc.v[v];
          out[p.W + v] = all.v[v];
        }
      }
    }
  }

  // ---- ordinary rows: virtual workgroup = 256 rows, one lane per row (as rows_body<VEC, 1, false, true, false, true>) ----
  const int64_t n_vblocks = (p.n_rows + 255) / 256;
  for (int64_t vb = static_cast<int64_t>(blockIdx.x) * 4 + sub; vb < n_vblocks; vb += static_cast<int64_t>(gridDim.x) * 4) {
    const int64_t q = (vb * 4 + w4) * kWave + lane;
    if (q >= p.n_rows) continue;
    const int64_t i = adj_row(p, q);
    const int64_t lo = load_rowptr(p, i), hi = load_rowptr(p, i + 1);
    if (hi - lo > p.long_threshold) continue;           // hub row: sliced above
    SmallW sw = small_weights(p, i);
    float w_rest = 0.f;
    if (p.s_total) {   // (the same fold: rows_body, csrc/spmm_fwd_body.hpp)
      w_rest = sw.pick(rest);
#pragma unroll
      for (int d = 0; d < 4; ++d) sw.w[d] = d < rest ? sw.w[d] - w_rest : 0.f;
    }
    Vec<VEC> acc;
#pragma unroll
    for (int v = 0; v < VEC; ++v) acc.v[v] = 0.f;
    for (int64_t base = lo; base < hi; base += 16) {
      int colv[16];
      if (base + 16 <= p.nnz) {
        load_col_run<16>(p.col + base, colv);
      } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) colv[r] = base + r < hi ? p.col[base + r] : 0;
      }
      const int m = static_cast<int>(hi - base < 16 ? hi - base : 16);
      constexpr int FLY = VEC == 1 ? 8 : (VEC == 2 ? 4 : 2);      // gathers in flight per lane (64 VGPRs: 8 waves per SIMD)
#pragma unroll
      for (int j0 = 0; j0 < 16; j0 += FLY) {
        if (j0 >= m) break;
        Vec<VEC> sv[FLY];
        int d[FLY];
#pragma unroll
        for (int u = 0; u < FLY; ++u) {
          const unsigned ce = static_cast<unsigned>(colv[j0 + u]);
          d[u] = static_cast<int>(ce >> kPackShift);
          d[u] = d[u] < rest ? d[u] : rest;
          // (no branch around a gather, see the slice loop: entries past the row end read the first hot row from LDS)
          sv[u] = hot_gather<VEC>(p, hot, j0 + u < m ? static_cast<int>(ce & kPackMask) : static_cast<int>(p.hot_lo));
        }
#pragma unroll
        for (int u = 0; u < FLY; ++u) {
          const float w = sw.pick(d[u]);
#pragma unroll
          for (int v = 0; v < VEC; ++v) acc.v[v] = j0 + u < m ? fmaf(w, sv[u].v[v], acc.v[v]) : acc.v[v];
        }
      }
    }
    if (p.s_total) {
      const Vec<VEC> tot = load_vec<VEC>(p.s_total);
#pragma unroll
      for (int v = 0; v < VEC; ++v) acc.v[v] = fmaf(w_rest, tot.v[v], acc.v[v]);
    }
    store_vec<VEC>(p.Y + out_row(p, q, i) * p.y_stride, acc);
  }
}

// fix-up: add a hub row's slices in a fixed order, apply the rest-bucket term, store the row.
// One WAVE per hub row, four rows per workgroup, no barriers: a power-law graph has tens of thousands of hub rows with
// one or two slices each (R-MAT 10M/100M: 33 068 rows, 45 284 slices, at most 114 per row), so a workgroup per row was
// bound by the workgroup launch rate (0.10 ms).  Lane = column (64 columns per pass); narrower operands put
// K = 64 / W' lanes on a column (W' = W rounded up to a power of two), lane k takes slices k, k + K, ...; loads are
// issued eight at a time; the K partial sums meet in a fixed butterfly.  One fixed order per row: bit-reproducible.
__global__ __launch_bounds__(256) void spmm_long_fixup_kernel(const Params p) {
  const int lane = threadIdx.x & (kWave - 1);
  const int r = blockIdx.x * (blockDim.x / kWave) + threadIdx.x / kWave;
  if (r >= p.n_long) return;
  const int64_t q = p.long_rows[r];
  const int64_t i = adj_row(p, q);
  const int s0 = p.long_slice_ptr[r], s1 = p.long_slice_ptr[r + 1];
  int wp = 1;
  while (wp < p.W && wp < kWave) wp <<= 1;
  const int K = kWave / wp;              // slice lanes per column
  const int k = lane / wp;
  float chan = 0.f;                      // lane c < reduce_cr accumulates channel c over the column passes
  for (int w0 = 0; w0 < p.W; w0 += kWave) {
    const int w = w0 + lane % wp;
    float acc = 0.f, all = 0.f;
    if (w < p.W) {
      const float* src = p.partial + w;
      const int64_t row = 2 * static_cast<int64_t>(p.W);
      int s = s0 + k;
      for (; s + 7 * K < s1; s += 8 * K) {
        float a[8], b[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          a[u] = src[(s + u * K) * row];
          b[u] = src[(s + u * K) * row + p.W];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          acc += a[u];
          all += b[u];
        }
      }
      for (; s < s1; s += K) {
        acc += src[s * row];
        all += src[s * row + p.W];
      }
    }
    for (int off = wp; off < kWave; off <<= 1) {   // slice lanes of a column: fixed butterfly, every lane ends with the sum
      acc += __shfl_xor(acc, off);
      all += __shfl_xor(all, off);
    }
    const bool owner = k == 0 && w < p.W;
    if (owner) {
      if (p.s_total) {
        const Vec<1> wr = row_weights<1>(p, i, p.D - 1, w);
        acc = fmaf(wr.v[0], p.s_total[w] - all, acc);
      }
      if (p.reduce_cr == 0) p.Y[out_row(p, q, i) * p.y_stride + w] = acc;
    }
    if (p.reduce_cr) {  // fixed butterfly: offsets stay multiples of reduce_cr, so channels never mix
      float v = owner ? acc : 0.f;
      for (int off = kWave / 2; off >= p.reduce_cr; off >>= 1) v += __shfl_xor(v, off);
      chan += v;
    }
  }
  if (p.reduce_cr && lane < p.reduce_cr) {
    if (p.self_sum) {    // (validate(): reduce_cr == 1, one weight channel) the self pair's term, as the rows' epilogue adds it
      float w = row_weights<1>(p, i, 0, 0).v[0];
      if (p.s_total) w -= row_weights<1>(p, i, p.D - 1, 0).v[0];
      chan = fmaf(w, self_term(p, out_row(p, q, i)), chan);
    }
    p.Y[out_row(p, q, i) * p.y_stride + lane] = chan;
  }
}

// the hub rows' fix-up behind a launch that left their slices in p.partial (spmm_kernel, spmm_hot_kernel)
int launch_fixup(const Params& p, hipStream_t st) {
  if (p.n_slices <= 0) return GNAN_OK;
  hipLaunchKernelGGL(spmm_long_fixup_kernel, dim3(static_cast<unsigned>((p.n_long + 3) / 4)), dim3(256), 0, st, p);
  return gnan::check_launch("spmm_long_fixup_kernel");
}

// combine: the classed rows' segments (seg_body, csrc/spmm_fwd_body.hpp) -> the rows' read-out.  One thread per classed row:
//   Y[row] = fmaf(w_0 - w_rest, a_i, fmaf(w_rest, T, ((p0 + p1) + (p2 + p3)) + ((p4 + p5) + (p6 + p7))))
// p_c the row's partial of class c where the mask says it exists (else 0: the workspace is never cleared), T and a_i by
// combine_store (csrc/spmm_common.hpp).  One fixed shape per row: bit-reproducible.
__global__ __launch_bounds__(256) void spmm_seg_combine_kernel(const Params p) {
  const int64_t r = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (r >= p.seg_q_hi - p.seg_q_lo) return;
  const int64_t q = p.seg_q_lo + r;
  const int64_t o = out_row(p, q, q);
  const unsigned mask = p.seg_mask[r];
  const float4 a = *reinterpret_cast<const float4*>(p.seg_partial + r * 8);
  const float4 b = *reinterpret_cast<const float4*>(p.seg_partial + r * 8 + 4);
  const float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
  float c[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) c[k] = (mask >> k) & 1u ? v[k] : 0.f;
  combine_store(p, q, o, ((c[0] + c[1]) + (c[2] + c[3])) + ((c[4] + c[5]) + (c[6] + c[7])));
}

int launch_seg_combine(const Params& p, hipStream_t st) {
  if (p.seg_index == nullptr) return GNAN_OK;
  const int64_t n = p.seg_q_hi - p.seg_q_lo;
  hipLaunchKernelGGL(spmm_seg_combine_kernel, dim3(static_cast<unsigned>((n + 255) / 256)), dim3(256), 0, st, p);
  return gnan::check_launch("spmm_seg_combine_kernel");
}

// combine of the blocked hub segments (seg_body<.., HUB>): one WAVE per hub row r, four rows per workgroup, no barrier.  Lane l adds the
// row's slots hub_row_slot_ptr[r] + l, + l + 64, ... in turn (a serial chain), the 64 lane sums meet in a fixed xor butterfly, then
//   Y[row] = fmaf(w_0 - w_rest, a_i, fmaf(w_rest, T, sum))
// with T, the weights and a_i exactly as spmm_seg_combine_kernel reads them.  The slots are the ROW-major enumeration of the row's
// segments, so the order of the adds depends on the plan alone, not on the queues: bit-reproducible, no atomics.
__global__ __launch_bounds__(256) void spmm_hub_combine_kernel(const Params p) {
  const int lane = threadIdx.x & (kWave - 1);
  const int r = blockIdx.x * (blockDim.x / kWave) + threadIdx.x / kWave;
  if (r >= p.n_hub) return;
  const int s0 = p.hub_row_slot_ptr[r], s1 = p.hub_row_slot_ptr[r + 1];
  float y = 0.f;
  for (int s = s0 + lane; s < s1; s += kWave) y += p.hub_partial[s];
#pragma unroll
  for (int off = kWave / 2; off >= 1; off >>= 1) y += __shfl_xor(y, off);
  if (lane != 0) return;
  const int64_t q = p.hub_q_lo + r;
  combine_store(p, q, out_row(p, q, q), y);
}

int launch_hub_combine(const Params& p, hipStream_t st) {
  if (p.hub_index == nullptr) return GNAN_OK;
  hipLaunchKernelGGL(spmm_hub_combine_kernel, dim3(static_cast<unsigned>((p.n_hub + 3) / 4)), dim3(256), 0, st, p);
  return gnan::check_launch("spmm_hub_combine_kernel");
}

// can the persistent hot-row kernel take this call?  (what the host wrapper sets up: functional.spmm_launch, narrow walk)
bool hot_kernel_applies(const gnan_spmm_args* a) {
  const int W = a->W;
  return a->hot_rows > 0 && a->cls_index == nullptr && a->rowptr != nullptr && a->packed_index && a->s_dtype == GNAN_F32 && (W == 1 || W == 2 || W == 4) &&
         a->s_stride == W && a->Cw == 1 && a->D <= 4 && !a->weight_by_col && !a->minus_rest && !a->s_by_code && a->reduce_cr == 0 &&
         aligned(a->S, 16) && aligned(a->Y, 4 * static_cast<size_t>(W)) && a->y_stride % W == 0 &&
         (!a->s_total || aligned(a->s_total, 4 * static_cast<size_t>(W))) && a->hot_lo >= 0 &&
         a->hot_lo + a->hot_rows <= a->n_cols && static_cast<int64_t>(a->hot_rows) * W <= kHotLdsFloats && a->nnz > 0;
}

template <int VEC>
int launch_hot(const Params& p, hipStream_t st) {
  const size_t lds = static_cast<size_t>(p.hot_n) * VEC * sizeof(float);
  hipLaunchKernelGGL((spmm_hot_kernel<VEC>), dim3(static_cast<unsigned>(cu_count()) * 2), dim3(1024), lds, st, p);
  if (int rc = gnan::check_launch("spmm_hot_kernel")) return rc;
  return launch_fixup(p, st);
}

// ---------------------------------------------------------------------------------------------
// shell sums:  T[q, d, :] = sum_{e in row, code_e == d} S[col_e, :]   (and the rest bucket)
// Needed only by the backward pass (gradient w.r.t. the weight table):  dwt[q, d, c] =
// sum_{w = c mod Cw} dY[q, w] * T[q, d, w].  Same traversal as the rows kernel; a lane owns its
// columns of T[q, :, :], so plain read-modify-write on global memory is race-free.
// ---------------------------------------------------------------------------------------------
template <int VEC, int LPR, bool DENSE>
__global__ __launch_bounds__(256) void spmm_shell_sums_kernel(const Params p) {
  constexpr int G = kWave / LPR;
  constexpr int TILE = LPR * VEC;
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x / kWave;
  const int sub = lane % LPR;
  const int slot = lane / LPR;
  const int64_t q = (static_cast<int64_t>(blockIdx.x) * (blockDim.x / kWave) + wave) * G + slot;
  if (q >= p.n_rows) return;
  const int64_t i = adj_row(p, q);
  int64_t lo, hi, code_base;
  if constexpr (DENSE) {
    lo = 0; hi = p.n_cols; code_base = i * p.n_cols;
  } else {
    lo = load_rowptr(p, i); hi = load_rowptr(p, i + 1); code_base = 0;
  }
  const int rest = p.D - 1;
  float* T = p.Y + q * static_cast<int64_t>(p.D) * p.W;
  for (int w0 = 0; w0 < p.W; w0 += TILE) {
    const int cw = w0 + sub * VEC;
    const bool col_ok = cw < p.W;
    Vec<VEC> all;
#pragma unroll
    for (int v = 0; v < VEC; ++v) all.v[v] = 0.f;
    for (int64_t base = lo; base < hi; base += LPR) {
      const int64_t e = base + sub;
      int colv = 0, codev = 0;
      if (e < hi) {
        if constexpr (!DENSE) colv = p.col[e];
        codev = p.code[code_base + e];
      }
      const int m = static_cast<int>(hi - base < LPR ? hi - base : LPR);
      for (int j = 0; j < m; ++j) {
        int c;
        if constexpr (DENSE) c = static_cast<int>(base) + j; else c = __shfl(colv, j, LPR);
        int d = __shfl(codev, j, LPR);
        d = d < rest ? d : rest;
        if (col_ok) {
          const Vec<VEC> sv = load_operand<VEC>(p.S, c, p.s_stride, cw);
          float* t = T + static_cast<int64_t>(d) * p.W + cw;
          Vec<VEC> cur = load_vec<VEC>(t);
#pragma unroll
          for (int v = 0; v < VEC; ++v) { cur.v[v] += sv.v[v]; all.v[v] += sv.v[v]; }
          store_vec<VEC>(t, cur);
        }
      }
    }
    if (col_ok && p.s_total) {
      const Vec<VEC> tot = load_vec<VEC>(p.s_total + cw);
      Vec<VEC> r;
#pragma unroll
      for (int v = 0; v < VEC; ++v) r.v[v] = tot.v[v] - all.v[v];
      store_vec<VEC>(T + static_cast<int64_t>(rest) * p.W + cw, r);
    }
  }
}

template <int VEC, int LPR>
int launch_shell(const Params& p, bool dense, hipStream_t st) {
  constexpr int G = kWave / LPR;
  const int rows_per_block = 4 * G;
  const int64_t blocks = (p.n_rows + rows_per_block - 1) / rows_per_block;
  if (blocks > 0x7fffffffLL) return gnan::fail(GNAN_ERR_UNSUPPORTED, "shell_sums: too many rows for one launch");
  const dim3 grid(static_cast<unsigned>(blocks)), block(256);
  if (dense) {
    hipLaunchKernelGGL((spmm_shell_sums_kernel<VEC, LPR, true>), grid, block, 0, st, p);
  } else {
    hipLaunchKernelGGL((spmm_shell_sums_kernel<VEC, LPR, false>), grid, block, 0, st, p);
  }
  return gnan::check_launch("spmm_shell_sums_kernel");
}

template <int VEC>
int launch_shell_lpr(const Params& p, int lpr, bool dense, hipStream_t st) {
  return dispatch_lpr(lpr, [&](auto L) { return launch_shell<VEC, decltype(L)::value>(p, dense, st); });
}

// Which kernel variant serves a (validated) forward call: gnan_spmm_fwd launches what this picks, gnan_spmm_fwd_describe reports it.
struct Route {
  int vec, lpr;
  bool dense, smalld, hot;
};

int pick_route(const gnan_spmm_args* a, Route* r) {
  r->dense = a->rowptr == nullptr;
  r->smalld = !r->dense && a->Cw == 1 && a->D <= 4 && !a->weight_by_col && !a->minus_rest;
  r->hot = false;
  if (a->reduce_cr) {
    pick_tiling(a, static_cast<const float*>(a->S), a->s_stride, &r->vec, &r->lpr);  // narrow output: scalar stores
  } else {
    pick_tiling(a, a->Y, a->y_stride, &r->vec, &r->lpr);
  }
  if (a->s_dtype == GNAN_BF16) {       // (validate(): CSR layout only)
    r->vec = 8;
    r->lpr = 1;
    while (r->lpr * 8 < a->W && r->lpr < kWave) r->lpr <<= 1;
    return GNAN_OK;
  }
  if (a->shell_out != nullptr) {
    const bool ok = r->smalld && a->W == 1 && a->n_slices == 0 && a->reduce_cr == 0 && !a->s_by_code && a->s_dtype == GNAN_F32 &&
                    a->hot_rows == 0 && r->vec == 1 && r->lpr == 1;
    if (!ok)
      return gnan::fail(GNAN_ERR_UNSUPPORTED, "spmm: shell_out serves a one-column fp32 operand on the small-D CSR route without hub-row "
                                              "slices, fused read-out or hot rows");
  }
  if (a->self_sum != nullptr && !(r->smalld && short_tiles_serve(r->vec, r->lpr, r->smalld, a->packed_index != 0, a->s_by_code != 0)))
    return gnan::fail(GNAN_ERR_UNSUPPORTED, "spmm: self_sum is served for fp32 rows read 16 B per lane by 16 lanes or more (W in (32, 256], "
                                            "16-B aligned rows)");
  r->hot = r->smalld && hot_kernel_applies(a);   // narrow rows, hottest operand rows in LDS (persistent workgroups)
  return GNAN_OK;
}

}  // namespace

extern "C" size_t gnan_spmm_fwd_workspace_bytes(const gnan_spmm_args* a) {
  if (!a) return 0;
  size_t floats = hub_partial_offset(a);                               // the hub slices' partials, then the classed rows'
  if (a->hub_index && a->n_hub_seg > 0) floats += static_cast<size_t>(a->n_hub_seg);   // ... then the blocked hub segments'
  if (a->stream_index && a->n_stream_seg > 0) floats += static_cast<size_t>(a->n_stream_seg);   // ... then the pair stream's
  return floats * sizeof(float);
}

extern "C" int gnan_spmm_shell_sums(const gnan_spmm_args* a, gnan_stream_t stream) {
  if (int rc = validate(a)) return rc;
  if (int rc = forward_only_index(a, "shell_sums")) return rc;
  if (int rc = forward_only_self_sum(a, "shell_sums")) return rc;
  if (a->n_rows == 0) return GNAN_OK;
  GNAN_REQUIRE(!a->weight_by_col, "shell_sums: weight_by_col has no meaning here");
  if (a->s_dtype != GNAN_F32) return gnan::fail(GNAN_ERR_UNSUPPORTED, "shell_sums: fp32 operand rows only (no backward for bf16 storage)");
  const Params p = make_params(a);
  int vec, lpr;
  pick_tiling(a, a->Y, a->W, &vec, &lpr);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const bool dense = a->rowptr == nullptr;
  return vec == 4 ? launch_shell_lpr<4>(p, lpr, dense, st) : launch_shell_lpr<1>(p, lpr, dense, st);
}

extern "C" int gnan_spmm_fwd_describe(const gnan_spmm_args* a, gnan_spmm_launch_info* out) {
  GNAN_REQUIRE(out != nullptr, "spmm describe: null output");
  if (int rc = validate(a)) return rc;
  *out = gnan_spmm_launch_info{};
  if (a->n_rows == 0) return GNAN_OK;
  Route r;
  if (int rc = pick_route(a, &r)) return rc;
  out->vec = r.vec; out->lpr = r.lpr; out->smalld = r.smalld; out->dense = r.dense;
  out->kernel = r.hot ? GNAN_SPMM_KERNEL_HOT : GNAN_SPMM_KERNEL_ROWS;
  if (r.hot) return GNAN_OK;
  Params p = make_params(a);
  if (int rc = plan_tiles(p, r.vec, r.lpr, r.dense, r.smalld, a->seg_max_per_class, a->hub_seg_max_per_class)) return rc;
  out->n_seg_blocks = p.n_seg_blocks; out->n_segs = p.n_seg_blocks > 0 ? a->n_seg : 0;
  out->n_hub_seg_blocks = p.n_hub_blocks; out->n_hub_segs = p.n_hub_blocks > 0 ? a->n_hub_seg : 0;
  out->n_stream_blocks = gnan::stream_blocks(a, r.lpr); out->n_stream_segs = out->n_stream_blocks > 0 ? a->n_stream_seg : 0;
  out->classed = p.cls_index != nullptr;
  out->n_slice_blocks = p.n_slice_blocks; out->n_tile_blocks = p.n_tile_blocks; out->n_tiles = p.n_tiles;
  out->row_q0 = p.row_q0;
  for (int L = 0; L <= GNAN_SHORT_LMAX; ++L) out->short_tile[L] = p.short_tile[L];
  out->n_lone_rows = p.lone_n; out->n_lone_blocks = gnan::lone_blocks(p.lone_n); out->n_tile_blocks_skipped = p.n_tile_blocks - lone_tile_blocks(p);
  return GNAN_OK;
}

extern "C" int gnan_spmm_fwd(const gnan_spmm_args* a, gnan_stream_t stream) {
  if (int rc = validate(a)) return rc;
  if (a->n_rows == 0) return GNAN_OK;
  const size_t need = gnan_spmm_fwd_workspace_bytes(a);
  if (need > 0 && (a->workspace == nullptr || a->workspace_bytes < need))
    return gnan::fail(GNAN_ERR_WORKSPACE, "spmm: workspace %zu B < required %zu B", a->workspace_bytes, need);
  // (for the hot kernel and the fix-up; launch_lpr builds its own record with the tile plan: Params is of the anonymous namespace and
  // does not cross translation units, and the fix-up reads none of the tile fields)
  const Params p = make_params(a);
  Route r;
  if (int rc = pick_route(a, &r)) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (r.hot) return a->W == 1 ? launch_hot<1>(p, st) : (a->W == 2 ? launch_hot<2>(p, st) : launch_hot<4>(p, st));
  if (int rc0 = gnan::launch_stream(a, r.lpr, st)) return rc0;     // (the pair stream's phase comes first in time)
  const int rc = r.vec == 8 ? gnan::launch_lpr<8>(a, r.lpr, r.dense, r.smalld, st)
                            : (r.vec == 4 ? gnan::launch_lpr<4>(a, r.lpr, r.dense, r.smalld, st) : gnan::launch_lpr<1>(a, r.lpr, r.dense, r.smalld, st));
  if (rc) return rc;
  if (r.vec == 4 && r.smalld) {      // (validate(): the flag comes with self_sum, which pick_route() admits on this variant only)
    if (int rc2 = gnan::launch_lone(a, r.lpr, st)) return rc2;      // the lone rows, beside spmm_kernel: disjoint output rows
  }
  if (int rc2 = launch_fixup(p, st)) return rc2;
  if (int rc2 = launch_hub_combine(p, st)) return rc2;
  if (int rc2 = launch_seg_combine(p, st)) return rc2;
  return gnan::launch_stream_combine(a, st);
}
