// The wide forward's kernel and its launch: row blocks, short-row tiles, classed row segments and hub-row slices of spmm_kernel<VEC, LPR, ...>
// (the mapping: csrc/spmm.hip).  Compiled once per VEC — csrc/spmm_fwd_v1.hip, _v4 and _v8 instantiate gnan::launch_lpr<VEC>
// over this body — so that the 100 instances build as three objects side by side.
#pragma once
#include "spmm_common.hpp"

namespace {

// ---------------------------------------------------------------------------------------------
// rows kernel: one LPR-lane group per output row
// ---------------------------------------------------------------------------------------------
template <int VEC, int LPR, bool DENSE, bool SMALLD, bool BYCODE, bool PACKED = false, bool SELF = false>
__device__ __forceinline__ void rows_body(const Params& p, const int64_t block_id) {
  constexpr int G = kWave / LPR;     // groups (rows) per wave
  constexpr int TILE = LPR * VEC;    // operand columns one pass covers
  // gathers in flight per lane.  fp32 rows: 1, 2, 3 and 4 measure the same (4.68-4.76 ms on C4: at 8 waves/SIMD the
  // kernel sits on the L2 request rate, not on latency), 8 costs registers, hence waves.  bf16 rows: 2 fits
  // the 64-VGPR budget of 8 waves/SIMD without scratch: 2.93 -> 2.71 ms (1: 2.77, 3: 2.70, 4: 2.93).
  constexpr int UNROLL = VEC == 8 ? 2 : 4;
  constexpr int IW = LPR >= 8 ? LPR : 16;  // index pairs fetched per round by one group (narrow rows: 16)
  constexpr int IPL = IW / LPR;            // ... per lane
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x / kWave;
  const int sub = lane % LPR;
  const int slot = lane / LPR;
  int64_t q = p.row_q0 + (block_id * (blockDim.x / kWave) + wave) * G + slot;
  if constexpr (SELF) {   // rows [seg_q_lo, seg_q_hi) are taken in segments (seg_body); both are 0 without a classed row plan
    if (q >= p.seg_q_lo) q += p.seg_q_hi - p.seg_q_lo;
  }
  if (q >= p.n_rows) return;
  const int64_t i = adj_row(p, q);
  int64_t lo, hi, code_base;
  if constexpr (DENSE) {
    lo = 0;
    hi = p.n_cols;
    code_base = i * p.n_cols;
  } else {
    lo = load_rowptr(p, i);
    hi = load_rowptr(p, i + 1);
    code_base = 0;
    if (hi - lo > p.long_threshold) return;  // hub row: long kernel
  }
  const int rest = p.D - 1;
  // SMALLD folds the rest bucket into the listed weights:  sum_d w_d s + w_rest (total - sum s)
  //   = sum_d (w_d - w_rest) s + w_rest total,  so no second accumulator for the listed operand rows is needed.
  SmallW sw;
  float w_rest = 0.f;
  if constexpr (SMALLD) {
    sw = small_weights(p, i);
    if (p.s_total) {   // (the same fold: spmm_hot_kernel, csrc/spmm.hip)
      w_rest = sw.pick(rest);
#pragma unroll
      for (int d = 0; d < 4; ++d) sw.w[d] = d < rest ? sw.w[d] - w_rest : 0.f;
    }
  }
  float red[4] = {0.f, 0.f, 0.f, 0.f};  // fused feature sum (reduce_cr in {1, 2, 4}): channel partials of this lane
  // a training forward of a one-column operand keeps the raw per-code sums of its rows (gnan_spmm_args.shell_out): a lane owns a
  // row here, so three more accumulators and a select per pair
  constexpr bool kShell = SMALLD && VEC == 1 && LPR == 1 && !BYCODE && !DENSE;
  float sh[3] = {0.f, 0.f, 0.f};
  // (uniform) one weight per pair from a per-neighbour table, no counts, no rest subtraction: see the index loads below
  const bool pair_weights = !SMALLD && !DENSE && p.weight_by_col && p.Cw == 1 && p.cnt == nullptr && !p.minus_rest && p.lut_row_stride != 0;

  for (int w0 = 0; w0 < p.W; w0 += TILE) {
    const int cw = w0 + sub * VEC;
    const bool col_ok = cw < p.W;
    Vec<VEC> acc, all;
#pragma unroll
    for (int v = 0; v < VEC; ++v) acc.v[v] = all.v[v] = 0.f;

    // The group fetches IW = max(LPR, 16) index pairs per round — IPL per lane — so that narrow operand
    // rows (few lanes per group) still see 16 gathers between two dependent index loads.
    for (int64_t base = lo; base < hi; base += IW) {
      int colv[IPL], codev[IPL];   // (the same index round: the row blocks of spmm_lut_grad_kernel, csrc/spmm_grad.hip)
      bool wide = false;
      if constexpr (!DENSE && IPL % 4 == 0) {
        const int64_t e0 = base + sub * IPL;
        wide = e0 + IPL <= p.nnz;
        if (wide) {
          if constexpr (PACKED) load_col_run<IPL>(p.col + e0, colv);
          else load_index_run<IPL>(p.col + e0, p.code + e0, colv, codev);
        }
      }
      if (!wide) {
#pragma unroll
        for (int r = 0; r < IPL; ++r) {
          const int64_t e = base + sub * IPL + r;
          colv[r] = codev[r] = 0;
          if (e < hi) {
            if constexpr (!DENSE) colv[r] = p.col[e];
            if constexpr (!PACKED) codev[r] = p.code[code_base + e];
          }
        }
      }
      if constexpr (PACKED) {
#pragma unroll
        for (int r = 0; r < IPL; ++r) {
          codev[r] = static_cast<int>(static_cast<unsigned>(colv[r]) >> kPackShift);
          colv[r] = static_cast<int>(static_cast<unsigned>(colv[r]) & kPackMask);
        }
      }
      const int m = static_cast<int>(hi - base < IW ? hi - base : IW);
      // Per-neighbour weight table (the wide backward pass: weight = wt[c, d], one channel): the lane that holds a pair's index
      // entry fetches its weight too — ONE load instruction per round and group — and hands it out by shuffle like the column id.
      // Read inside the pair loop it was a second memory instruction per pair and lane: 133 -> 271 us on the arxiv shape.
      float wv[IPL];
      if constexpr (!SMALLD) {
#pragma unroll
        for (int r = 0; r < IPL; ++r) {
          wv[r] = 0.f;
          if (pair_weights && base + sub * IPL + r < hi) {
            const int dd = codev[r] < rest ? codev[r] : rest;
            wv[r] = p.lut[static_cast<int64_t>(colv[r]) * p.lut_row_stride + dd];
          }
        }
      }
      // IPL > 1: fully unrolled so that the register index j % IPL is static; IPL == 1: plain runtime loop
#pragma unroll(IPL > 1 ? IW / UNROLL : 1)
      for (int j0 = 0; j0 < (IPL > 1 ? IW : m); j0 += UNROLL) {
        if (IPL > 1 && j0 >= m) break;
        Raw<VEC> s[UNROLL];
        int d[UNROLL], c[UNROLL];
        float wp[UNROLL];
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
          const int j = j0 + u;              // compile-time after unrolling: lane j / IPL holds it in register j % IPL
          if constexpr (DENSE) {
            c[u] = static_cast<int>(base) + j;
          } else {
            c[u] = __shfl(colv[j % IPL], j / IPL, LPR);
          }
          d[u] = __shfl(codev[j % IPL], j / IPL, LPR);
          d[u] = d[u] < rest ? d[u] : rest;
          if constexpr (!SMALLD) wp[u] = __shfl(wv[j % IPL], j / IPL, LPR);
          s[u].zero();
          if (j < m && col_ok)
            s[u].load(p.S, BYCODE ? static_cast<int64_t>(c[u]) * p.D + d[u] : static_cast<int64_t>(c[u]), p.s_stride, cw);
        }
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
          if (j0 + u < m) {
            const Vec<VEC> sv = s[u].widen();
            if constexpr (SMALLD) {
              const float w = sw.pick(d[u]);
#pragma unroll
              for (int v = 0; v < VEC; ++v) acc.v[v] = fmaf(w, sv.v[v], acc.v[v]);
              if constexpr (kShell) {
                sh[0] += d[u] == 0 ? sv.v[0] : 0.f;
                sh[1] += d[u] == 1 ? sv.v[0] : 0.f;
                sh[2] += d[u] == 2 ? sv.v[0] : 0.f;
              }
            } else {
              Vec<VEC> w;
              if (pair_weights) {
#pragma unroll
                for (int v = 0; v < VEC; ++v) w.v[v] = wp[u];
              } else {
                w = edge_weights<VEC>(p, i, c[u], d[u], cw);
              }
#pragma unroll
              for (int v = 0; v < VEC; ++v) {
                acc.v[v] = fmaf(w.v[v], sv.v[v], acc.v[v]);
                all.v[v] += sv.v[v];
              }
            }
          }
        }
      }
    }
    if (col_ok) {
      if (p.s_total) {
        const Vec<VEC> tot = load_vec<VEC>(p.s_total + cw);
        if constexpr (SMALLD) {
#pragma unroll
          for (int v = 0; v < VEC; ++v) acc.v[v] = fmaf(w_rest, tot.v[v], acc.v[v]);
        } else {
          const Vec<VEC> wr = row_weights<VEC>(p, i, rest, cw);
#pragma unroll
          for (int v = 0; v < VEC; ++v) acc.v[v] = fmaf(wr.v[v], tot.v[v] - all.v[v], acc.v[v]);
        }
      }
      if (p.reduce_cr == 0) {
        store_vec<VEC>(p.Y + out_row(p, q, i) * p.y_stride + cw, acc);
      } else {
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
          const int ch = (cw + v) & (p.reduce_cr - 1);  // reduce_cr is a power of two
#pragma unroll
          for (int c = 0; c < 4; ++c) red[c] += ch == c ? acc.v[v] : 0.f;
        }
      }
    }
  }
  if constexpr (kShell) {
    if (p.shell_out) {
      float* t = p.shell_out + out_row(p, q, i) * (p.D - 1);
      for (int dd = 0; dd < p.D - 1; ++dd) t[dd] = dd == 0 ? sh[0] : (dd == 1 ? sh[1] : sh[2]);
    }
  }
  if (p.reduce_cr) {
    // read-out fused into the epilogue (GNAN.py:72-73): add the channel partials of the group's lanes (the same epilogue: short_tile)
#pragma unroll
    for (int off = 1; off < LPR; off <<= 1) {
#pragma unroll
      for (int c = 0; c < 4; ++c) red[c] += __shfl_xor(red[c], off);
    }
    if (sub == 0) {
      if constexpr (SELF) {   // (validate(): reduce_cr == 1) the self pair's term, its weight folded like a listed one
        red[0] = fmaf(sw.w[0], self_term(p, out_row(p, q, i)), red[0]);
      }
      for (int c = 0; c < p.reduce_cr; ++c) p.Y[out_row(p, q, i) * p.y_stride + c] = red[c];
    }
  }
}

// ---------------------------------------------------------------------------------------------
// short-row tiles: R rows of exactly L pairs per lane group, many rows per wave
// ---------------------------------------------------------------------------------------------
// A row of the degree-sorted copy with one to four pairs (82 % of the rows of a power-law graph) costs rows_body a wave's start,
// a rowptr load and one round of gathers for four rows.  In a run of rows of one length L, row q's pairs start at
// short_pair[L] + (q - short_row[L]) L: a tile needs no rowptr, loads the index entries of all its rows with one coalesced load
// and has the gathers of R rows (R L of them, at most 8 per lane) in flight before the first is consumed.
// Rows [qg, qg + R) (those below q_end) of run L, their first pair at e: per row exactly rows_body's arithmetic under SMALLD &&
// PACKED with one pass over the columns (the launch guarantees LPR VEC >= W and LPR >= 8): the folded weights (w_d - w_rest),
// fmaf over the row's pairs in order, fmaf(w_rest, tot, acc), then the fused read-out's channel sums and butterfly.
template <int VEC, int LPR, int L, bool SELF>
__device__ __forceinline__ void short_tile(const Params& p, int64_t qg, int64_t q_end, int64_t e) {
  constexpr int R = short_rows_per_group(L);
  constexpr int NP = R * L;                    // pairs of the group (<= 8 <= LPR: one index entry per lane)
  constexpr int KW = (4 * R + LPR - 1) / LPR;  // weight registers per lane: (row r, code d) lives in lane (4 r + d) % LPR, register 4 r / LPR
  static_assert(LPR >= 8 && LPR % 4 == 0 && NP <= LPR && R <= LPR, "one index entry and one output row per lane");
  const int sub = (threadIdx.x & (kWave - 1)) % LPR;
  const int nr = static_cast<int>(q_end - qg < R ? q_end - qg : R);
  if (nr <= 0) return;  // (the whole group)
  const int rest = p.D - 1;
  const int cw = sub * VEC;
  const bool col_ok = cw < p.W;
  unsigned ent = 0u;
  if constexpr (NP > 0) {
    if (sub < nr * L) ent = static_cast<unsigned>(p.col[e + sub]);
  }
  int orow = 0;
  if (sub < nr) orow = p.row_ids[qg + sub];
  float wv[KW], wrv[KW];
#pragma unroll
  for (int k = 0; k < KW; ++k) {
    const int idx = sub + k * LPR, r = idx >> 2, d = idx & 3;
    float v = 0.f;
    if (r < nr && d < p.D) {
      v = p.lut[(qg + r) * p.lut_row_stride + d];
      if (p.cnt) {
        const int c = p.cnt[(qg + r) * p.cnt_stride + d];
        v = v / static_cast<float>(c > 1 ? c : 1);
      }
    }
    const float wr = __shfl(v, (sub & ~3) + rest, LPR);  // w_rest of this lane's row (before the fold)
    wrv[k] = 0.f;
    if (p.s_total) {
      wrv[k] = wr;
      v = d < rest ? v - wr : 0.f;
    }
    wv[k] = v;
  }
  Raw<VEC> s[NP > 0 ? NP : 1];
#pragma unroll
  for (int j = 0; j < NP; ++j) {
    const unsigned en = static_cast<unsigned>(__shfl(static_cast<int>(ent), j, LPR));
    s[j].zero();
    if (j < nr * L && col_ok) s[j].load(p.S, static_cast<int64_t>(en & kPackMask), p.s_stride, cw);
  }
  // SELF: what the rows' epilogues read is requested here, once and ahead of the row loop — the lane's columns of s_total (the same for
  // every row) and, by lane sub < nr, the self term of its row — so that no load is waited for inside the loop.  Not the self terms
  // of run L = 1: eight gathers in flight and eight rows' weights held — with a ninth value live through the loop the 16-lane instance
  // (W <= 64) spilled 12 B of scratch at 8 waves/SIMD, wherever the read was placed; that run reads a_i in its row's epilogue
  constexpr bool kSelfAhead = SELF && L != 1;
  Vec<VEC> tot_all;
  float a_self = 0.f;
#pragma unroll
  for (int v = 0; v < VEC; ++v) tot_all.v[v] = 0.f;
  if constexpr (SELF) {
    if (col_ok && p.s_total) tot_all = load_vec<VEC>(p.s_total + cw);
  }
  if constexpr (kSelfAhead) {
    if (sub < nr) a_self = self_term(p, orow);
  }
#pragma unroll
  for (int r = 0; r < R; ++r) {
    if (r >= nr) break;
    Vec<VEC> acc;
#pragma unroll
    for (int v = 0; v < VEC; ++v) acc.v[v] = 0.f;
#pragma unroll
    for (int l = 0; l < L; ++l) {
      // the pair's weight: its code from the index entry (fetched again rather than held through the gathers: registers)
      int d = static_cast<int>(static_cast<unsigned>(__shfl(static_cast<int>(ent), r * L + l, LPR)) >> kPackShift);
      d = d < rest ? d : rest;
      const float w = __shfl(wv[4 * r / LPR], (4 * r) % LPR + d, LPR);
      const Vec<VEC> sv = s[r * L + l].widen();
#pragma unroll
      for (int v = 0; v < VEC; ++v) acc.v[v] = fmaf(w, sv.v[v], acc.v[v]);
    }
    const float w_rest = __shfl(wrv[4 * r / LPR], (4 * r) % LPR, LPR);
    const int64_t o = __shfl(orow, r, LPR);
    if constexpr (SELF) {
      // (validate(): reduce_cr == 1) one channel sum: the additions of the general epilogue below for that case, in the same order —
      // the rest term, the lane's columns onto 0.f, the group's butterfly (group_sum: the same pairs), the self term
      float y = 0.f;
      if (col_ok) {
        if (p.s_total) {
#pragma unroll
          for (int v = 0; v < VEC; ++v) acc.v[v] = fmaf(w_rest, tot_all.v[v], acc.v[v]);
        }
#pragma unroll
        for (int v = 0; v < VEC; ++v) y += acc.v[v];
      }
      y = group_sum<LPR>(y);
      const float w_self = __shfl(wv[4 * r / LPR], (4 * r) % LPR, LPR);   // row r's folded code-0 weight sits in lane 4 r
      if constexpr (kSelfAhead) {
        const float a = __shfl(a_self, r, LPR);
        if (sub == 0) p.Y[o * p.y_stride] = fmaf(w_self, a, y);
      } else {
        if (sub == 0) p.Y[o * p.y_stride] = fmaf(w_self, self_term(p, o), y);
      }
    } else {
      float red[4] = {0.f, 0.f, 0.f, 0.f};
      if (col_ok) {
        if (p.s_total) {
          const Vec<VEC> tot = load_vec<VEC>(p.s_total + cw);
#pragma unroll
          for (int v = 0; v < VEC; ++v) acc.v[v] = fmaf(w_rest, tot.v[v], acc.v[v]);
        }
        if (p.reduce_cr == 0) {
          store_vec<VEC>(p.Y + o * p.y_stride + cw, acc);
        } else {
#pragma unroll
          for (int v = 0; v < VEC; ++v) {
            const int ch = (cw + v) & (p.reduce_cr - 1);  // reduce_cr is a power of two
#pragma unroll
            for (int c = 0; c < 4; ++c) red[c] += ch == c ? acc.v[v] : 0.f;
          }
        }
      }
      if (p.reduce_cr) {   // (rows_body's epilogue, for output row o)
#pragma unroll
        for (int off = 1; off < LPR; off <<= 1) {
#pragma unroll
          for (int c = 0; c < 4; ++c) red[c] += __shfl_xor(red[c], off);
        }
        if (sub == 0) {
          for (int c = 0; c < p.reduce_cr; ++c) p.Y[o * p.y_stride + c] = red[c];
        }
      }
    }
  }
}

// Tile t of the launch: find its run (static indices only: a dynamically indexed kernel argument would go to scratch).
template <int VEC, int LPR, bool SELF>
__device__ __forceinline__ void short_tiles(const Params& p, int t) {
  if (t >= p.n_tiles) return;
  int L = 0;
  int64_t k = t, q0 = 0, q1 = p.short_row[1], e0 = p.short_pair[0];
#pragma unroll
  for (int l = 1; l <= GNAN_SHORT_LMAX; ++l) {
    if (l <= p.short_lmax && t >= p.short_tile[l]) {
      L = l; k = t - p.short_tile[l]; q0 = p.short_row[l]; q1 = p.short_row[l + 1]; e0 = p.short_pair[l];
    }
  }
  constexpr int G = kWave / LPR;
  const int slot = (threadIdx.x & (kWave - 1)) / LPR;
#define GNAN_SHORT_CASE(LL)                                                                       \
  case LL: {                                                                                      \
    constexpr int R = short_rows_per_group(LL);                                              \
    const int64_t qg = q0 + (k * G + slot) * R;                                                   \
    short_tile<VEC, LPR, LL, SELF>(p, qg, q1, e0 + (qg - q0) * LL);                                     \
    break;                                                                                        \
  }
  switch (L) {
    GNAN_SHORT_CASE(0) GNAN_SHORT_CASE(1) GNAN_SHORT_CASE(2) GNAN_SHORT_CASE(3) GNAN_SHORT_CASE(4)
    GNAN_SHORT_CASE(5) GNAN_SHORT_CASE(6) GNAN_SHORT_CASE(7) GNAN_SHORT_CASE(8)
    default: break;
  }
#undef GNAN_SHORT_CASE
}

// ---------------------------------------------------------------------------------------------
// classed row segments: one lane group per (row, column class) of the rows the classed row plan names
// ---------------------------------------------------------------------------------------------
// The row walk spreads every often-listed operand row over all eight L2s (a workgroup's XCD is blockIdx & 7, its rows list any
// column).  Here the pairs of row q whose column falls in class c = col & 7 are one segment, the segments of class c are taken by the
// workgroups with blockIdx & 7 == c, and so each XCD's L2 holds one eighth of the hot rows.  The read-out is fused on this route
// (reduce_cr == 1), so a segment's result is ONE float — the lane group's share of the row's feature sum — stored at
// seg_partial[(q - seg_q_lo) * 8 + c]; the combine pass (spmm_seg_combine_kernel, csrc/spmm.hip) adds a row's classes, the rest term
// and the self term.  Weights as rows_body folds them under SMALLD; 16 index entries per round, four gathers in flight,
// no branch around a gather: a slot past the segment's end reads the segment's last row again (an L1 hit) and is dropped by a select.
// No LDS, no barrier, no atomics; the lane butterfly's first four steps are DPP row operations (group_sum, csrc/spmm_common.hpp).

// HUB: the blocked hub segments (gnan_spmm_args.hub_*) — the same body over the hub plan's arrays; the float goes to the segment's slot
// of the row-major enumeration, hub_partial[hub_seg_slot[s]] (spmm_hub_combine_kernel, csrc/spmm.hip, adds a row's slots).
template <int VEC, int LPR, bool HUB = false>
__device__ __forceinline__ void seg_body(const Params& p, const int blk) {
  static_assert(LPR >= 16 && VEC == 4, "a DPP row per lane group, one index entry per lane and round");
  constexpr int G = kWave / LPR;
  constexpr int IW = 16;    // index entries per round
  constexpr int FLY = 4;    // gathers in flight per lane: 8 spills 8 B of scratch at 8 waves/SIMD (64 VGPRs), 4 fits (63)
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x / kWave;
  const int sub = lane % LPR;
  const int slot = lane / LPR;
  const int cls = blk & 7;
  const int32_t* cls_ptr = HUB ? p.hub_cls_seg_ptr : p.cls_seg_ptr;
  const int64_t* start = HUB ? p.hub_seg_start : p.seg_start;
  const int s = cls_ptr[cls] + ((blk >> 3) * 4 + wave) * G + slot;
  if (s >= cls_ptr[cls + 1]) return;   // (the whole group)
  const int64_t q = (HUB ? p.hub_seg_row : p.seg_row)[s];
  const int64_t lo = start[s];
  const int n = static_cast<int>(start[s + 1] - lo);     // (a row of at most long_threshold pairs; a hub segment of at most the plan's cap)
  const int32_t* idx = (HUB ? p.hub_index : p.seg_index) + lo;
  const int rest = p.D - 1;
  SmallW sw = small_weights(p, q);           // (scatter_out 2: slot q reads adjacency row q)
  {
    const float w_rest = sw.pick(rest);      // (validate(): s_total is set)
#pragma unroll
    for (int d = 0; d < 4; ++d) sw.w[d] = d < rest ? sw.w[d] - w_rest : 0.f;
  }
  const bool col_ok = sub * VEC < p.W;
  const float* Sl = static_cast<const float*>(p.S) + (col_ok ? sub * VEC : 0);   // (a lane past the columns reads column 0, dropped below)
  Vec<VEC> acc;
#pragma unroll
  for (int v = 0; v < VEC; ++v) acc.v[v] = 0.f;
  for (int base = 0; base < n; base += IW) {
    const int m = n - base < IW ? n - base : IW;
    int ent = 0;
    if (sub < m) ent = idx[base + sub];
#pragma unroll
    for (int j0 = 0; j0 < IW; j0 += FLY) {
      if (j0 >= m) break;
      Vec<VEC> sv[FLY];
#pragma unroll
      for (int u = 0; u < FLY; ++u) {
        const int j = j0 + u < m ? j0 + u : m - 1;
        const unsigned en = static_cast<unsigned>(__shfl(ent, j, LPR));
        sv[u] = load_vec<VEC>(Sl + static_cast<int64_t>(en & kPackMask) * p.s_stride);
      }
#pragma unroll
      for (int u = 0; u < FLY; ++u) {
        const bool ok = j0 + u < m;
        const int j = ok ? j0 + u : m - 1;
        int d = static_cast<int>(static_cast<unsigned>(__shfl(ent, j, LPR)) >> kPackShift);
        d = d < rest ? d : rest;
        const float w = ok ? sw.pick(d) : 0.f;     // (a slot past the end: weight 0 would still turn an inf into a NaN, hence the select)
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc.v[v] = ok ? fmaf(w, sv[u].v[v], acc.v[v]) : acc.v[v];
      }
    }
  }
  float r = 0.f;
#pragma unroll
  for (int v = 0; v < VEC; ++v) r += acc.v[v];
  r = col_ok ? r : 0.f;
  r = group_sum<LPR>(r);
  if constexpr (HUB) {
    if (sub == 0) p.hub_partial[p.hub_seg_slot[s]] = r;
  } else {
    if (sub == 0) p.seg_partial[(q - p.seg_q_lo) * 8 + cls] = r;
  }
}

// ---------------------------------------------------------------------------------------------
// long kernel: one 256-thread workgroup per slice of a hub row (classed hub plan: one wave per slice, one class per workgroup)
// ---------------------------------------------------------------------------------------------
template <int VEC, int LPR, bool SMALLD, bool DENSE, bool BYCODE, bool PACKED = false>
__device__ __forceinline__ void slice_body(const Params& p, const int blk) {
  constexpr int G = kWave / LPR;
  constexpr int TILE = LPR * VEC;
  constexpr int NW = 4;  // waves per workgroup
  __shared__ float red[NW][2][TILE];
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x / kWave;
  const int sub = lane % LPR;
  const int slot = lane / LPR;
  // classed plan (CSR only): the block's queue entry names the slice, the slice its range of the plan's packed index and its hub slot
  const bool classed = !DENSE && p.cls_index != nullptr;
  int s = blk, a = 0;
  int64_t lo, hi;
  if (classed) {
    // one slice per WAVE: the waves of block blk take entries 4 (blk >> 3) .. + 3 of class blk & 7's queue (a class's slices
    // are short — 175 pairs on average on C4 — and a workgroup per slice idled three waves and paid an LDS reduction for each)
    const int e = ((blk >> 3) * NW + wave) * 8 + (blk & 7);
    s = e < p.cls_n_slots ? p.cls_slot_slice[e] : -1;
    if (s < 0) return;                      // past the end of this class's queue (no barrier follows on this path)
    a = p.cls_slice_row[s];
    lo = p.cls_slice_start[s];
    hi = p.cls_slice_start[s + 1];
  } else {
    a = slice_owner(p, s);
  }
  const int64_t q = p.long_rows[a];
  const int64_t i = adj_row(p, q);
  const int64_t code_base = DENSE ? i * p.n_cols : 0;
  if (!classed) slice_range<DENSE>(p, i, a, s, lo, hi);   // (dense layout: the codes of row i sit at i * n_cols)
  const int32_t* idx = classed ? p.cls_index : p.col;
  const int rest = p.D - 1;
  SmallW sw;
  if constexpr (SMALLD) sw = small_weights(p, i);

  for (int w0 = 0; w0 < p.W; w0 += TILE) {
    const int cw = w0 + sub * VEC;
    const bool col_ok = cw < p.W;
    Vec<VEC> acc, all;
#pragma unroll
    for (int v = 0; v < VEC; ++v) acc.v[v] = all.v[v] = 0.f;
    // wave `wave` takes 64-edge chunks wave, wave+NW, ... (classed plan: the wave's own slice, every chunk)
    const int64_t step = classed ? kWave : NW * kWave;
    for (int64_t base = lo + (classed ? 0 : static_cast<int64_t>(wave) * kWave); base < hi; base += step) {
      const int64_t e = base + lane;
      int colv = 0, codev = 0;
      if (e < hi) {
        colv = DENSE ? static_cast<int>(e) : idx[e];
        if constexpr (!PACKED && !DENSE) {
          if (!classed) codev = p.code[e];
        } else if constexpr (!PACKED) {
          codev = p.code[code_base + e];
        }
      }
      if (PACKED || classed) {
        codev = static_cast<int>(static_cast<unsigned>(colv) >> kPackShift);
        colv = static_cast<int>(static_cast<unsigned>(colv) & kPackMask);
      }
      const int m = static_cast<int>(hi - base < kWave ? hi - base : kWave);
#pragma unroll 4
      for (int t = 0; t < LPR; ++t) {
        const int j = slot + t * G;
        const int c = __shfl(colv, j);
        int d = __shfl(codev, j);
        d = d < rest ? d : rest;
        if (j < m && col_ok) {
          const Vec<VEC> sv = load_operand<VEC>(p.S, BYCODE ? static_cast<int64_t>(c) * p.D + d : static_cast<int64_t>(c), p.s_stride, cw);
          if constexpr (SMALLD) {
            const float w = sw.pick(d);
#pragma unroll
            for (int v = 0; v < VEC; ++v) acc.v[v] = fmaf(w, sv.v[v], acc.v[v]);
          } else {
            const Vec<VEC> w = edge_weights<VEC>(p, i, c, d, cw);
#pragma unroll
            for (int v = 0; v < VEC; ++v) acc.v[v] = fmaf(w.v[v], sv.v[v], acc.v[v]);
          }
#pragma unroll
          for (int v = 0; v < VEC; ++v) all.v[v] += sv.v[v];
        }
      }
    }
    // groups of one wave -> group 0 (fixed butterfly order), then waves -> LDS -> wave 0
#pragma unroll
    for (int off = LPR; off < kWave; off <<= 1) {
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        acc.v[v] += __shfl_xor(acc.v[v], off);
        all.v[v] += __shfl_xor(all.v[v], off);
      }
    }
    if (classed) {
      if (slot == 0 && col_ok) {
        float* out = p.partial + static_cast<int64_t>(s) * 2 * p.W;
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
          out[cw + v] = acc.v[v];
          out[p.W + cw + v] = all.v[v];
        }
      }
      continue;
    }
    __syncthreads();
    if (slot == 0) {
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        red[wave][0][sub * VEC + v] = acc.v[v];
        red[wave][1][sub * VEC + v] = all.v[v];
      }
    }
    __syncthreads();
    if (wave == 0 && slot == 0 && col_ok) {
      float* out = p.partial + static_cast<int64_t>(s) * 2 * p.W;
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        float x = 0.f, y = 0.f;
#pragma unroll
        for (int w = 0; w < NW; ++w) {
          x += red[w][0][sub * VEC + v];
          y += red[w][1][sub * VEC + v];
        }
        out[cw + v] = x;
        out[p.W + cw + v] = y;
      }
    }
  }
}

// One launch covers everything: workgroups [0, n_slices) take the hub-row slices (they start first,
// so the long-latency slices overlap the bulk) — or (SELF) the blocked hub segments, a class's queue in popularity-block order — then
// (SELF) the classed rows' segments, then the tiles; the rest take 4*G ordinary rows each.
// BYCODE (operand row = (neighbour, hop code), the narrow-operand backward) is a template parameter: as a run-time
// flag its address arithmetic cost the W = 64 kernels 4 VGPRs and the bf16 variant 20 B of scratch (bf16 rows 2.85 -> 3.35 ms).
// SELF (the route short_tiles_serve describes, reduce_cr == 1): the rows' self term from gnan_spmm_args.self_sum in the read-out's
// epilogue.  A template parameter like BYCODE: as a run-time branch it cost the W = 32, 128 and 256 variants 12-20 B of scratch.
template <int VEC, int LPR, bool DENSE, bool SMALLD, bool BYCODE = false, bool PACKED = false, bool SELF = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu((SMALLD && LPR >= 8) ? 8 : 1)))
void spmm_kernel(const Params p) {
  static_assert(!SELF || short_tiles_serve(VEC, LPR, SMALLD, PACKED, BYCODE), "the self term: on the route the tiles serve");
  if constexpr (!DENSE) {
    if (static_cast<int>(blockIdx.x) < p.n_slice_blocks) {
      slice_body<VEC, LPR, SMALLD, false, BYCODE, PACKED>(p, static_cast<int>(blockIdx.x));
      return;
    }
    int front = p.n_slice_blocks;       // workgroups ahead of the tile blocks
    if constexpr (SELF) {               // (plan_tiles() leaves n_hub_blocks / n_seg_blocks 0 without a blocked hub / classed row plan)
      if (static_cast<int>(blockIdx.x) < front + p.n_hub_blocks) {   // (validate(): no slice blocks then — these are the launch's first)
        seg_body<VEC, LPR, true>(p, static_cast<int>(blockIdx.x) - front);
        return;
      }
      front += p.n_hub_blocks;
      if (static_cast<int>(blockIdx.x) < front + p.n_seg_blocks) {
        seg_body<VEC, LPR>(p, static_cast<int>(blockIdx.x) - front);
        return;
      }
      front += p.n_seg_blocks;
    }
    if constexpr (short_tiles_serve(VEC, LPR, SMALLD, PACKED, BYCODE)) {   // (launch() leaves n_tile_blocks 0 for every other variant)
      if (static_cast<int>(blockIdx.x) < front + p.n_tile_blocks) {
        short_tiles<VEC, LPR, SELF>(p, (static_cast<int>(blockIdx.x) - front) * (blockDim.x / kWave) + threadIdx.x / kWave);
        return;
      }
    }
    rows_body<VEC, LPR, false, SMALLD, BYCODE, PACKED, SELF>(p, static_cast<int64_t>(blockIdx.x) - front - p.n_tile_blocks);
  } else {
    if (p.n_slices > 0) {      // few rows, many neighbours: every row is cut into slices, there are no row blocks
      slice_body<VEC, LPR, SMALLD, true, false>(p, static_cast<int>(blockIdx.x));
      return;
    }
    rows_body<VEC, LPR, true, SMALLD, false>(p, static_cast<int64_t>(blockIdx.x));
  }
}

template <int VEC, int LPR>
int launch(const gnan_spmm_args* a, bool dense, bool smalld, hipStream_t st) {
  constexpr int G = kWave / LPR;
  const int rows_per_block = 4 * G;
  Params p = make_params(a);
  if (int rc = plan_tiles(p, VEC, LPR, dense, smalld, a->seg_max_per_class, a->hub_seg_max_per_class)) return rc;
  leave_lone_tiles(p);     // (the lone rows: csrc/spmm_lone.hip)
  const int n_slices = p.n_slices;
  // (the classed rows are taken in segments; so are the rows from hub_q_lo on, n_rows without a blocked hub plan)
  const int64_t walked = p.hub_q_lo - p.row_q0 - (p.seg_q_hi - p.seg_q_lo);
  const int64_t blocks = dense && n_slices > 0
                             ? n_slices
                             : (walked + rows_per_block - 1) / rows_per_block + p.n_slice_blocks + p.n_hub_blocks + p.n_seg_blocks +
                                   p.n_tile_blocks;
  if (blocks > 0x7fffffffLL) return gnan::fail(GNAN_ERR_UNSUPPORTED, "spmm: too many rows for one launch");
  if (blocks == 0) return GNAN_OK;   // (every row is the pair stream's and no run is tiled: nothing for this kernel, and no empty grid)
  const dim3 grid(static_cast<unsigned>(blocks)), block(256);
  if (p.s_by_code) {
    if constexpr (VEC <= 4 && VEC * LPR <= 32) {  // validate(): fp32 rows of at most 32 columns, CSR layout
      if (smalld) {
        hipLaunchKernelGGL((spmm_kernel<VEC, LPR, false, true, true>), grid, block, 0, st, p);
      } else {
        hipLaunchKernelGGL((spmm_kernel<VEC, LPR, false, false, true>), grid, block, 0, st, p);
      }
    } else {
      return gnan::fail(GNAN_ERR_UNSUPPORTED, "spmm: s_by_code covers operand rows of at most 32 columns");
    }
  } else if (dense) {
    if constexpr (VEC != 8) {   // validate(): bf16 rows come with the CSR layout
      hipLaunchKernelGGL((spmm_kernel<VEC, LPR, true, false>), grid, block, 0, st, p);
    } else {
      return gnan::fail(GNAN_ERR_UNSUPPORTED, "spmm: bf16 operand rows need the CSR layout, W %% 8 == 0 and 16-B aligned rows");
    }
  } else if (smalld) {
    if (p.packed && p.self_sum != nullptr) {
      if constexpr (short_tiles_serve(VEC, LPR, true, true, false)) {
        hipLaunchKernelGGL((spmm_kernel<VEC, LPR, false, true, false, true, true>), grid, block, 0, st, p);
      } else {
        return gnan::fail(GNAN_ERR_UNSUPPORTED, "spmm: self_sum is served for fp32 rows read 16 B per lane by 16 lanes or more");
      }
    } else if (p.packed) {
      hipLaunchKernelGGL((spmm_kernel<VEC, LPR, false, true, false, true>), grid, block, 0, st, p);
    } else {
      hipLaunchKernelGGL((spmm_kernel<VEC, LPR, false, true>), grid, block, 0, st, p);
    }
  } else {
    hipLaunchKernelGGL((spmm_kernel<VEC, LPR, false, false>), grid, block, 0, st, p);
  }
  return gnan::check_launch("spmm_kernel");
}

}  // namespace

template <int VEC>
int gnan::launch_lpr(const gnan_spmm_args* a, int lpr, bool dense, bool smalld, hipStream_t st) {
  return dispatch_lpr(lpr, [&](auto L) { return launch<VEC, decltype(L)::value>(a, dense, smalld, st); });
}
