// The aggregation's gradients (gfx950): the weight table's gradient without the per-shell sums (spmm_lut_grad_kernel, CSR and
// dense layout) and the narrow operand's backward over the transposed adjacency (spmm_lut_grad_kernel<.., true>,
// spmm_bwd_hot_kernel).  The forward is csrc/spmm.hip, what the two share csrc/spmm_common.hpp, the packing pass in front of
// gnan_spmm_bwd_narrow csrc/pack_bwd_rows.hip.  See include/gnan_hip.h for the contract.
#include "spmm_common.hpp"

namespace {

// ---------------------------------------------------------------------------------------------
// Gradient w.r.t. the weight table without materialising the per-shell sums (truncated-hop case: D <= 4, Cw == 1).
//   dwt[q, d] = inv(q, d) * sum_w dY[q, w] * T[q, d, w],   T[q, d, :] = sum of the operand rows of q's hop-d pairs,
//   T[q, rest, :] = total - sum_{d < rest} T[q, d, :]  (or the listed rest pairs when there is no rest bucket).
// Same traversal as the forward kernel (gather the operand rows once), four accumulators per lane instead of one,
// contracted with the row's dY in the epilogue; spmm_shell_sums_kernel + torch needed a [n, D, W] tensor and one
// global read-modify-write per listed pair for this.  Rows / hub slices / fix-up as in the forward.  With
// `reduce_rows` the rows' contributions meet in fixed-order float64 partials (workgroup, then grid): dlut[d].
// ---------------------------------------------------------------------------------------------
struct GradParams {
  const float* dY;       // [n_rows, dy_channels]; column w of the operand pairs with dY[q, w % dy_channels]
  int64_t dy_stride;
  int dy_channels;
  float* dwt;            // per-row mode: [n_rows, D]
  double* blk;           // reduce mode: [n_row_blocks + n_long, 4]
  float* slice_T;        // [n_slices, 4, W]
  int reduce_rows;
  int64_t n_row_blocks;
  // BWD mode (gnan_spmm_bwd_narrow): the traversal runs over the TRANSPOSED adjacency, p.S holds one row per (neighbour,
  // hop code), 2 * half wide: [ dY_i / cnt(i, d) | dY_i / cnt(i, rest) ]; row j's own operand row S_j is contracted with
  // the per-code sums for the table gradient and the same sums, weighted by the table, are its operand gradient
  const float* s_rows;   // [n_rows, w_real] operand rows of the OUTPUT rows
  int64_t s_rows_stride;
  int half, w_real;      // p.W == 2 * half (half a power of two >= w_real)
  float* dS;             // [n_rows, w_real]
  int64_t ds_stride;
  int with_rest;
  const float* ds_add;   // optional [w_real]: added to every row of dS (the rest bucket's column-sum term) ...
  const float* ds_scale; // ... times this device scalar when given (rho(0) = lut[rest]: the caller hands over the bare column sums)
  const float* rest_total;   // optional [w_real], with rest_q [w_real]: dlut[D - 1] += <rest_total, rest_q> in the final pass
  const float* rest_q;
  int hot_code_lo, hot_codes;   // spmm_bwd_hot_kernel: packed rows [hot_lo, hot_lo + hot_n) of these code blocks are served from LDS
};

// BWD epilogue of one row for this lane's VEC columns: lanes of the first half hold A_d = sum over the row's code-d pairs
// of dY / cnt(., d), their partners (half columns further) Q = sum over ALL pairs of dY / cnt(., rest).
//   dS_j = sum_{d < rest} lut[d] A_d - lut[rest] Q        dlut[d] += <S_j, A_d>      dlut[rest] -= <S_j, Q>
template <int VEC, int LPR>
__device__ __forceinline__ void bwd_finish(const Params& p, const GradParams& gp, int64_t oq, int cw,
                                           Vec<VEC> (&t)[4], float (&pd)[4]) {
  const int rest = p.D - 1;
  const bool listed_rest = !gp.with_rest;        // no rest bucket: code D-1 is an ordinary listed shell
  float all[VEC];
#pragma unroll
  for (int v = 0; v < VEC; ++v) all[v] = t[0].v[v] + t[1].v[v] + t[2].v[v] + t[3].v[v];
#pragma unroll
  for (int v = 0; v < VEC; ++v) {
    // Q of this column: the partner lane's sum over all codes (same v) — or, with one lane per row (rows of 2 or 4
    // floats), the value `half` positions further in this lane's own vector
    float q;
    if constexpr (LPR == 1) q = all[(v + VEC / 2) % VEC];
    else q = __shfl_xor(all[v], LPR / 2);
    const int w = cw + v;
    if (w < gp.w_real) {
      const float sj = gp.s_rows[oq * gp.s_rows_stride + w];
      float ds = 0.f;
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        if (d < rest || (listed_rest && d == rest)) {
          ds = fmaf(p.lut[d], t[d].v[v], ds);
          pd[d] = fmaf(sj, t[d].v[v], pd[d]);
        }
      }
      if (gp.with_rest) {
        ds = fmaf(-p.lut[rest], q, ds);
        pd[rest & 3] = fmaf(-sj, q, pd[rest & 3]);
      }
      if (gp.ds_add) ds += gp.ds_scale ? __fmul_rn(*gp.ds_scale, gp.ds_add[w]) : gp.ds_add[w];
      gp.dS[oq * gp.ds_stride + w] = ds;
    }
  }
}

template <int VEC>
__device__ __forceinline__ void grad_finish(const Params& p, const GradParams& gp, int64_t i, int64_t oq, int cw,
                                            bool col_ok, Vec<VEC> (&t)[4], float (&pd)[4]) {
  // contract this lane's columns of T with dY and fold the rest bucket
  const int rest = p.D - 1;
  if (col_ok) {
    Vec<VEC> dy;
#pragma unroll
    for (int v = 0; v < VEC; ++v) dy.v[v] = gp.dY[oq * gp.dy_stride + (cw + v) % gp.dy_channels];
    if (p.s_total) {
      const Vec<VEC> tot = load_vec<VEC>(p.s_total + cw);
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        float lower = 0.f;
#pragma unroll
        for (int d = 0; d < 4; ++d) lower += d < rest ? t[d].v[v] : 0.f;
#pragma unroll
        for (int d = 0; d < 4; ++d) t[d].v[v] = d == rest ? tot.v[v] - lower : t[d].v[v];
      }
    }
#pragma unroll
    for (int d = 0; d < 4; ++d)
#pragma unroll
      for (int v = 0; v < VEC; ++v) pd[d] = fmaf(dy.v[v], t[d].v[v], pd[d]);
  }
}

__device__ __forceinline__ float grad_inv(const Params& p, int64_t i, int d) {
  if (!p.cnt || d >= p.D) return d < p.D ? 1.f : 0.f;
  const int c = p.cnt[i * p.cnt_stride + d];
  return 1.f / static_cast<float>(c > 1 ? c : 1);
}

template <int VEC, int LPR, bool BWD = false>
__global__ __launch_bounds__(256) void spmm_lut_grad_kernel(const Params p, const GradParams gp) {
  constexpr int G = kWave / LPR;
  constexpr int TILE = LPR * VEC;
  constexpr int NW = 4;
  __shared__ float red[NW][4][TILE];            // slice blocks: waves -> wave 0
  __shared__ float rowsum[NW * G][4];           // row blocks: the groups' dwt for the workgroup partial
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x / kWave;
  const int sub = lane % LPR;
  const int slot = lane / LPR;
  const int rest = p.D - 1;

  if (static_cast<int>(blockIdx.x) < p.n_slices) {
    // ---- hub-row slice: per-shell sums of this slice -> slice_T[s] ------------------------------
    const int s = blockIdx.x;
    const int a = slice_owner(p, s);
    const int64_t q = p.long_rows[a];
    const int64_t i = adj_row(p, q);
    int64_t lo, hi;
    slice_range(p, i, a, s, lo, hi);
    for (int w0 = 0; w0 < p.W; w0 += TILE) {
      const int cw = w0 + sub * VEC;
      const bool col_ok = cw < p.W;
      Vec<VEC> t[4];
#pragma unroll
      for (int d = 0; d < 4; ++d)
#pragma unroll
        for (int v = 0; v < VEC; ++v) t[d].v[v] = 0.f;
      for (int64_t base = lo + static_cast<int64_t>(wave) * kWave; base < hi; base += NW * kWave) {
        const int64_t e = base + lane;
        int colv = 0, codev = 0;
        if (e < hi) { colv = p.col[e]; codev = p.code[e]; }
        const int m = static_cast<int>(hi - base < kWave ? hi - base : kWave);
#pragma unroll 4
        for (int tt = 0; tt < LPR; ++tt) {
          const int j = slot + tt * G;
          const int c = __shfl(colv, j);
          int d = __shfl(codev, j);
          d = d < rest ? d : rest;
          if (j < m && col_ok) {
            const Vec<VEC> sv = load_operand<VEC>(p.S, BWD ? static_cast<int64_t>(d) * p.n_cols + c : static_cast<int64_t>(c), p.s_stride, cw);
#pragma unroll
            for (int dd = 0; dd < 4; ++dd)
#pragma unroll
              for (int v = 0; v < VEC; ++v) t[dd].v[v] += d == dd ? sv.v[v] : 0.f;
          }
        }
      }
#pragma unroll
      for (int off = LPR; off < kWave; off <<= 1)
#pragma unroll
        for (int d = 0; d < 4; ++d)
#pragma unroll
          for (int v = 0; v < VEC; ++v) t[d].v[v] += __shfl_xor(t[d].v[v], off);
      __syncthreads();
      if (slot == 0)
#pragma unroll
        for (int d = 0; d < 4; ++d)
#pragma unroll
          for (int v = 0; v < VEC; ++v) red[wave][d][sub * VEC + v] = t[d].v[v];
      __syncthreads();
      if (wave == 0 && slot == 0 && col_ok) {
        float* out = gp.slice_T + static_cast<int64_t>(s) * 4 * p.W;
#pragma unroll
        for (int d = 0; d < 4; ++d)
#pragma unroll
          for (int v = 0; v < VEC; ++v) {
            float x = 0.f;
#pragma unroll
            for (int w = 0; w < NW; ++w) x += red[w][d][sub * VEC + v];
            out[d * p.W + cw + v] = x;
          }
      }
    }
    return;
  }

  // ---- row block: one LPR-lane group per output row ------------------------------------------------
  const int64_t block_id = static_cast<int64_t>(blockIdx.x) - p.n_slices;
  const int64_t q = (block_id * NW + wave) * G + slot;
  float pd[4] = {0.f, 0.f, 0.f, 0.f};
  int64_t i = 0, oq = 0;
  bool live = q < p.n_rows;
  if (live) {
    i = adj_row(p, q);
    oq = out_row(p, q, i);
    const int64_t lo = load_rowptr(p, i), hi = load_rowptr(p, i + 1);
    live = hi - lo <= p.long_threshold;                 // hub rows: slices + fix-up
    if (live) {
      for (int w0 = 0; w0 < p.W; w0 += TILE) {
        const int cw = w0 + sub * VEC;
        const bool col_ok = cw < p.W;
        Vec<VEC> t[4];
#pragma unroll
        for (int d = 0; d < 4; ++d)
#pragma unroll
          for (int v = 0; v < VEC; ++v) t[d].v[v] = 0.f;
        // as in the forward: IW index pairs per round (IPL per lane), so narrow rows still see 16 gathers between
        // two dependent index loads
        constexpr int IW = LPR >= 8 ? LPR : 16;
        constexpr int IPL = IW / LPR;
        for (int64_t base = lo; base < hi; base += IW) {
          int colv[IPL], codev[IPL];   // (the same index round: rows_body, csrc/spmm_fwd_body.hpp)
          bool wide = false;
          if constexpr (IPL % 4 == 0) {
            const int64_t e0 = base + sub * IPL;
            wide = e0 + IPL <= p.nnz;
            if (wide) load_index_run<IPL>(p.col + e0, p.code + e0, colv, codev);
          }
          if (!wide) {
#pragma unroll
            for (int r = 0; r < IPL; ++r) {
              const int64_t e = base + sub * IPL + r;
              colv[r] = codev[r] = 0;
              if (e < hi) { colv[r] = p.col[e]; codev[r] = p.code[e]; }
            }
          }
          const int m = static_cast<int>(hi - base < IW ? hi - base : IW);
#pragma unroll(IPL > 1 ? IW / 4 : 1)
          for (int j0 = 0; j0 < (IPL > 1 ? IW : m); j0 += 4) {
            if (IPL > 1 && j0 >= m) break;
            Vec<VEC> sv[4];
            int d[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
              const int j = j0 + u;
              const int c = __shfl(colv[j % IPL], j / IPL, LPR);
              d[u] = __shfl(codev[j % IPL], j / IPL, LPR);
              d[u] = d[u] < rest ? d[u] : rest;
#pragma unroll
              for (int v = 0; v < VEC; ++v) sv[u].v[v] = 0.f;
              if (j < m && col_ok)
                sv[u] = load_operand<VEC>(p.S, BWD ? static_cast<int64_t>(d[u]) * p.n_cols + c : static_cast<int64_t>(c), p.s_stride, cw);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
              if (j0 + u < m)
#pragma unroll
                for (int dd = 0; dd < 4; ++dd)
#pragma unroll
                  for (int v = 0; v < VEC; ++v) t[dd].v[v] += d[u] == dd ? sv[u].v[v] : 0.f;
          }
        }
        if constexpr (BWD) bwd_finish<VEC, LPR>(p, gp, oq, cw, t, pd);       // one pass: 2 * half == LPR * VEC
        else grad_finish<VEC>(p, gp, i, oq, cw, col_ok, t, pd);
      }
#pragma unroll
      for (int off = 1; off < LPR; off <<= 1)
#pragma unroll
        for (int d = 0; d < 4; ++d) pd[d] += __shfl_xor(pd[d], off);
      if constexpr (!BWD) {
#pragma unroll
        for (int d = 0; d < 4; ++d) pd[d] *= grad_inv(p, i, d);
      }
      if (!gp.reduce_rows && sub == 0)
        for (int d = 0; d < p.D; ++d) gp.dwt[oq * p.D + d] = pd[d];
    }
  }
  if (gp.reduce_rows) {
    if (sub == 0)
#pragma unroll
      for (int d = 0; d < 4; ++d) rowsum[wave * G + slot][d] = live ? pd[d] : 0.f;
    __syncthreads();
    if (threadIdx.x < 4) {
      double acc = 0.0;
      for (int r = 0; r < NW * G; ++r) acc += rowsum[r][threadIdx.x];
      gp.blk[block_id * 4 + threadIdx.x] = acc;
    }
  }
}

// hub rows: add the slices in order, contract with dY, scale; one workgroup per hub row
template <bool BWD = false>
__global__ __launch_bounds__(256) void spmm_lut_grad_fixup_kernel(const Params p, const GradParams gp) {
  // one wave per hub row (four rows per workgroup, no barriers), as in spmm_long_fixup_kernel: lane = column, operands
  // narrower than a wave put K = 64 / W' lanes on a column, lane k takes slices k, k + K, ...
  const int lane = threadIdx.x & (kWave - 1);
  const int r = blockIdx.x * (blockDim.x / kWave) + threadIdx.x / kWave;
  if (r >= p.n_long) return;
  const int64_t q = p.long_rows[r];
  const int64_t i = adj_row(p, q);
  const int64_t oq = out_row(p, q, i);
  const int s0 = p.long_slice_ptr[r], s1 = p.long_slice_ptr[r + 1];
  const int rest = p.D - 1;
  int wp = 1;
  while (wp < p.W && wp < kWave) wp <<= 1;
  const int K = kWave / wp;
  const int k = lane / wp;
  double pd[4] = {0.0, 0.0, 0.0, 0.0};
  for (int w0 = 0; w0 < p.W; w0 += kWave) {
    const int w = w0 + lane % wp;
    float t[4] = {0.f, 0.f, 0.f, 0.f};
    if (w < p.W) {
      int s = s0 + k;
      for (; s + K < s1; s += 2 * K) {     // two slices = eight independent loads at a time
        float a[4], b[4];
#pragma unroll
        for (int d = 0; d < 4; ++d) {
          a[d] = gp.slice_T[(static_cast<int64_t>(s) * 4 + d) * p.W + w];
          b[d] = gp.slice_T[(static_cast<int64_t>(s + K) * 4 + d) * p.W + w];
        }
#pragma unroll
        for (int d = 0; d < 4; ++d) t[d] = (t[d] + a[d]) + b[d];
      }
      for (; s < s1; s += K)
#pragma unroll
        for (int d = 0; d < 4; ++d) t[d] += gp.slice_T[(static_cast<int64_t>(s) * 4 + d) * p.W + w];
    }
    for (int off = wp; off < kWave; off <<= 1)   // slice lanes of a column: fixed butterfly, every lane ends with the sum
#pragma unroll
      for (int d = 0; d < 4; ++d) t[d] += __shfl_xor(t[d], off);
    if constexpr (BWD) {
      // one pass (2 * half <= 64 columns): the lane `half` columns further holds this column's Q
      const float all = t[0] + t[1] + t[2] + t[3];
      const float qv = __shfl_xor(all, gp.half);
      if (k == 0 && w < gp.w_real) {
        const float sj = gp.s_rows[oq * gp.s_rows_stride + w];
        float ds = 0.f;
#pragma unroll
        for (int d = 0; d < 4; ++d)
          if (d < rest || (!gp.with_rest && d == rest)) {
            ds = fmaf(p.lut[d], t[d], ds);
            pd[d] += static_cast<double>(sj) * t[d];
          }
        if (gp.with_rest) {
          ds = fmaf(-p.lut[rest], qv, ds);
          pd[rest & 3] -= static_cast<double>(sj) * qv;
        }
        if (gp.ds_add) ds += gp.ds_scale ? __fmul_rn(*gp.ds_scale, gp.ds_add[w]) : gp.ds_add[w];
        gp.dS[oq * gp.ds_stride + w] = ds;
      }
    } else if (k == 0 && w < p.W) {
      if (p.s_total) {
        float lower = 0.f;
#pragma unroll
        for (int d = 0; d < 4; ++d) lower += d < rest ? t[d] : 0.f;
#pragma unroll
        for (int d = 0; d < 4; ++d) t[d] = d == rest ? p.s_total[w] - lower : t[d];
      }
      const float dy = gp.dY[oq * gp.dy_stride + w % gp.dy_channels];
#pragma unroll
      for (int d = 0; d < 4; ++d) pd[d] += static_cast<double>(dy) * t[d];
    }
  }
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1)
#pragma unroll
    for (int d = 0; d < 4; ++d) pd[d] += __shfl_xor(pd[d], off);
  if (lane < 4) {
    const int d = lane;
    double mine = pd[0];
    mine = d == 1 ? pd[1] : mine;
    mine = d == 2 ? pd[2] : mine;
    mine = d == 3 ? pd[3] : mine;
    const double v = BWD ? mine : mine * grad_inv(p, i, d);
    if (gp.reduce_rows) gp.blk[(gp.n_row_blocks + r) * 4 + d] = v;
    else if (d < p.D) gp.dwt[oq * p.D + d] = static_cast<float>(v);
  }
}

// dlut[d] = sum over the workgroup / hub-row partials, fixed order
// (+ <tot, q> over w floats on entry D - 1 when tot is given: the rest bucket's column-sum term, gnan_spmm_bwd_narrow)
__global__ __launch_bounds__(1024) void spmm_lut_grad_final_kernel(const double* __restrict__ blk, int64_t n, int D,
                                                                   float* __restrict__ out, const float* __restrict__ tot = nullptr,
                                                                   const float* __restrict__ q = nullptr, int w = 0) {
  // one 1024-thread workgroup: a thread adds whole [4] records (32 contiguous bytes), eight loads in flight; the partials
  // meet in a fixed tree.  (Four 256-thread workgroups walking 72k records of a 10M-node graph one by one took 95 us.)
  __shared__ double red[4][1024];
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  const double2* rec = reinterpret_cast<const double2*>(blk);
  int64_t b = threadIdx.x;
  for (; b + 7 * 1024 < n; b += 8 * 1024) {
    double2 lo[8], hi[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      lo[u] = rec[(b + u * 1024) * 2];
      hi[u] = rec[(b + u * 1024) * 2 + 1];
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      s[0] += lo[u].x; s[1] += lo[u].y; s[2] += hi[u].x; s[3] += hi[u].y;
    }
  }
  for (; b < n; b += 1024) {
    const double2 lo = rec[b * 2], hi = rec[b * 2 + 1];
    s[0] += lo.x; s[1] += lo.y; s[2] += hi.x; s[3] += hi.y;
  }
#pragma unroll
  for (int d = 0; d < 4; ++d) red[d][threadIdx.x] = s[d];
  __syncthreads();
  for (int st = 512; st > 0; st >>= 1) {
    if (static_cast<int>(threadIdx.x) < st)
#pragma unroll
      for (int d = 0; d < 4; ++d) red[d][threadIdx.x] += red[d][threadIdx.x + st];
    __syncthreads();
  }
  if (static_cast<int>(threadIdx.x) < D && threadIdx.x < 4) {
    double v = red[threadIdx.x][0];
    if (tot && static_cast<int>(threadIdx.x) == D - 1)
      for (int c = 0; c < w; ++c) v = fma(static_cast<double>(tot[c]), static_cast<double>(q[c]), v);
    out[threadIdx.x] = static_cast<float>(v);
  }
}

template <int VEC, int LPR, bool BWD = false>
int launch_lut_grad(const Params& p, GradParams gp, hipStream_t st, float* dlut) {
  constexpr int G = kWave / LPR;
  const int64_t row_blocks = (p.n_rows + 4 * G - 1) / (4 * G);
  gp.n_row_blocks = row_blocks;
  const int64_t blocks = row_blocks + p.n_slices;
  if (blocks > 0x7fffffffLL) return gnan::fail(GNAN_ERR_UNSUPPORTED, "lut_grad: too many rows for one launch");
  hipLaunchKernelGGL((spmm_lut_grad_kernel<VEC, LPR, BWD>), dim3(static_cast<unsigned>(blocks)), dim3(256), 0, st, p, gp);
  if (int rc = gnan::check_launch("spmm_lut_grad_kernel")) return rc;
  if (p.n_slices > 0) {
    hipLaunchKernelGGL(spmm_lut_grad_fixup_kernel<BWD>, dim3(static_cast<unsigned>((p.n_long + 3) / 4)), dim3(256), 0, st, p, gp);
    if (int rc = gnan::check_launch("spmm_lut_grad_fixup_kernel")) return rc;
  }
  if (gp.reduce_rows) {
    hipLaunchKernelGGL(spmm_lut_grad_final_kernel, dim3(1), dim3(1024), 0, st, gp.blk, row_blocks + p.n_long, p.D, dlut, gp.rest_total,
                       gp.rest_q, gp.w_real);
    return gnan::check_launch("spmm_lut_grad_final_kernel");
  }
  return GNAN_OK;
}

// ---------------------------------------------------------------------------------------------
// spmm_bwd_hot_kernel — spmm_lut_grad_kernel<2, 1, true> (one-channel operands: packed rows of 2 floats, one lane per row)
// the way spmm_hot_kernel runs the forward: the degree-sorted copy of the TRANSPOSED adjacency read as one packed index
// stream, persistent 1024-thread workgroups (two per CU), and the packed rows of the most listed nodes — [hot_lo,
// hot_lo + hot_n) of the code blocks [hot_code_lo, hot_code_lo + hot_codes) of V — served from a 64-KB LDS copy.
// Ordinary rows: the arithmetic of spmm_lut_grad_kernel pair by pair (dS bit-identical); the table gradient's partials
// are per WAVE — 64 rows at a time through a fixed float64 butterfly, added up over the wave's blocks: one record per
// wave of the grid, so the order is fixed for a given device (the grid is two workgroups per CU); hub-row slices are summed
// by one wave each (fixed butterfly) and finished by spmm_lut_grad_fixup_kernel<true>.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ Vec<2> bwd_hot_gather(const Params& p, const GradParams& gp, const float2* hot, int c, int d) {
  // branch-free, as hot_gather: both loads are issued, the hot lanes of the global load share one row
  const int r = c - static_cast<int>(p.hot_lo);
  const int dl = d - gp.hot_code_lo;
  const bool is_hot = static_cast<unsigned>(r) < static_cast<unsigned>(p.hot_n) &&
                      static_cast<unsigned>(dl) < static_cast<unsigned>(gp.hot_codes);
  const int64_t row = is_hot ? static_cast<int64_t>(gp.hot_code_lo) * p.n_cols + p.hot_lo
                             : static_cast<int64_t>(d) * p.n_cols + c;
  const float2 g = *reinterpret_cast<const float2*>(static_cast<const float*>(p.S) + row * 2);
  const float2 l = hot[is_hot ? dl * p.hot_n + r : 0];
  Vec<2> out;
  out.v[0] = is_hot ? l.x : g.x;
  out.v[1] = is_hot ? l.y : g.y;
  return out;
}

__global__ __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(8, 8)))
void spmm_bwd_hot_kernel(const Params p, const GradParams gp) {
  extern __shared__ __attribute__((aligned(16))) float2 hot2[];      // [hot_codes][hot_n]
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int sub = wave >> 2, w4 = wave & 3;
  for (int i = tid; i < gp.hot_codes * p.hot_n; i += 1024) {
    const int dl = i / p.hot_n, r = i - dl * p.hot_n;
    hot2[i] = *reinterpret_cast<const float2*>(static_cast<const float*>(p.S) +
                                               (static_cast<int64_t>(gp.hot_code_lo + dl) * p.n_cols + p.hot_lo + r) * 2);
  }
  __syncthreads();
  const int rest = p.D - 1;
  const int idle_c = static_cast<int>(p.hot_lo), idle_d = gp.hot_code_lo;   // what a pair past the end reads: no request

  // ---- hub-row slices: one wave per slice, a contiguous run of slices per wave (see spmm_hot_kernel) --------------------
  {
    const int n_waves = static_cast<int>(gridDim.x) * 16;
    const int per = (p.n_slices + n_waves - 1) / n_waves;
    const int gw = static_cast<int>(blockIdx.x) * 16 + wave;
    const int s_lo = gw * per, s_hi = s_lo + per < p.n_slices ? s_lo + per : p.n_slices;
    int a = 0;
    if (s_lo < s_hi) a = slice_owner(p, s_lo);
    for (int sidx = s_lo; sidx < s_hi; ++sidx) {
      a = slice_owner_from(p, a, sidx);
      const int64_t i = adj_row(p, p.long_rows[a]);
      int64_t lo, hi;
      slice_range(p, i, a, sidx, lo, hi);
      Vec<2> t[4];
#pragma unroll
      for (int d = 0; d < 4; ++d) t[d].v[0] = t[d].v[1] = 0.f;
      constexpr int SF = 4;                              // pairs in flight per lane
      for (int64_t base = lo + lane; base < hi; base += SF * kWave) {
        unsigned ce[SF];
#pragma unroll
        for (int k = 0; k < SF; ++k) {
          const int64_t e = base + static_cast<int64_t>(k) * kWave;
          ce[k] = e < hi ? static_cast<unsigned>(p.col[e]) : 0u;
        }
        Vec<2> sv[SF];
        int dk[SF];
#pragma unroll
        for (int k = 0; k < SF; ++k) {
          const bool ok = base + static_cast<int64_t>(k) * kWave < hi;
          int d = static_cast<int>(ce[k] >> kPackShift);
          d = d < rest ? d : rest;
          dk[k] = ok ? d : -1;
          sv[k] = bwd_hot_gather(p, gp, hot2, ok ? static_cast<int>(ce[k] & kPackMask) : idle_c, ok ? d : idle_d);
        }
#pragma unroll
        for (int k = 0; k < SF; ++k)
#pragma unroll
          for (int dd = 0; dd < 4; ++dd) {
            t[dd].v[0] += dk[k] == dd ? sv[k].v[0] : 0.f;
            t[dd].v[1] += dk[k] == dd ? sv[k].v[1] : 0.f;
          }
      }
#pragma unroll
      for (int off = 1; off < kWave; off <<= 1)
#pragma unroll
        for (int d = 0; d < 4; ++d) {
          t[d].v[0] += __shfl_xor(t[d].v[0], off);
          t[d].v[1] += __shfl_xor(t[d].v[1], off);
        }
      if (lane < 8) {                                    // slice_T[s][d][w], W == 2: lane = 2 d + w
        float x = t[0].v[0];
#pragma unroll
        for (int d = 0; d < 4; ++d)
#pragma unroll
          for (int v = 0; v < 2; ++v) x = lane == 2 * d + v ? t[d].v[v] : x;
        gp.slice_T[static_cast<int64_t>(sidx) * 8 + lane] = x;
      }
    }
  }

  // ---- ordinary rows: one lane per row, virtual 256-row blocks as in spmm_hot_kernel --------------------------------------
  const int64_t n_vblocks = (p.n_rows + 255) / 256;
  double run = 0.0;                                      // lane d < 4: this wave's share of dlut[d], 64 rows at a time
  for (int64_t vb = static_cast<int64_t>(blockIdx.x) * 4 + sub; vb < n_vblocks; vb += static_cast<int64_t>(gridDim.x) * 4) {
    const int64_t q = (vb * 4 + w4) * kWave + lane;
    float pd[4] = {0.f, 0.f, 0.f, 0.f};
    bool live = q < p.n_rows;
    int64_t lo = 0, hi = 0, oq = 0;
    if (live) {
      const int64_t i = adj_row(p, q);
      oq = out_row(p, q, i);
      lo = load_rowptr(p, i);
      hi = load_rowptr(p, i + 1);
      live = hi - lo <= p.long_threshold;               // hub row: sliced above, finished by the fix-up kernel
    }
    if (live) {
      Vec<2> t[4];
#pragma unroll
      for (int d = 0; d < 4; ++d) t[d].v[0] = t[d].v[1] = 0.f;
      constexpr int RUN = 8;                             // index entries per round (16 as in the forward: spills at 64 VGPRs)
      for (int64_t base = lo; base < hi; base += RUN) {
        int colv[RUN];
        if (base + RUN <= p.nnz) {
          load_col_run<RUN>(p.col + base, colv);
        } else {
#pragma unroll
          for (int r = 0; r < RUN; ++r) colv[r] = base + r < hi ? p.col[base + r] : 0;
        }
        const int m = static_cast<int>(hi - base < RUN ? hi - base : RUN);
        constexpr int FLY = 4;
#pragma unroll
        for (int j0 = 0; j0 < RUN; j0 += FLY) {
          if (j0 >= m) break;
          Vec<2> sv[FLY];
          int d[FLY];
#pragma unroll
          for (int u = 0; u < FLY; ++u) {
            const unsigned ce = static_cast<unsigned>(colv[j0 + u]);
            const bool ok = j0 + u < m;
            int dd = static_cast<int>(ce >> kPackShift);
            dd = dd < rest ? dd : rest;
            d[u] = ok ? dd : -1;
            sv[u] = bwd_hot_gather(p, gp, hot2, ok ? static_cast<int>(ce & kPackMask) : idle_c, ok ? dd : idle_d);
          }
#pragma unroll
          for (int u = 0; u < FLY; ++u)
#pragma unroll
            for (int dd = 0; dd < 4; ++dd) {
              t[dd].v[0] += d[u] == dd ? sv[u].v[0] : 0.f;
              t[dd].v[1] += d[u] == dd ? sv[u].v[1] : 0.f;
            }
        }
      }
      bwd_finish<2, 1>(p, gp, oq, 0, t, pd);
    }
    // the table gradient's partial of these 64 rows: float64, fixed butterfly
    double s[4];
#pragma unroll
    for (int d = 0; d < 4; ++d) s[d] = live ? static_cast<double>(pd[d]) : 0.0;
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1)
#pragma unroll
      for (int d = 0; d < 4; ++d) s[d] += __shfl_xor(s[d], off);
    double mine = s[0];
    mine = lane == 1 ? s[1] : mine;
    mine = lane == 2 ? s[2] : mine;
    mine = lane == 3 ? s[3] : mine;
    run += mine;
  }
  if (lane < 4) gp.blk[(static_cast<int64_t>(blockIdx.x) * 16 + wave) * 4 + lane] = run;
}

// does gnan_spmm_bwd_narrow run on spmm_bwd_hot_kernel?  (packed index stream: only that kernel reads it)
bool bwd_hot_applies(const gnan_spmm_args* a) { return a->packed_index && a->W == 2; }

int bwd_hot_grid() { return cu_count() * 2; }     // two workgroups per CU

size_t bwd_hot_blk_entries(const gnan_spmm_args* a) {    // one record per wave of the grid + one per hub row
  return static_cast<size_t>(bwd_hot_grid()) * 16 + static_cast<size_t>(a->n_long > 0 ? a->n_long : 0);
}

int launch_bwd_hot(const Params& p, GradParams gp, hipStream_t st, float* dlut) {
  const int grid = bwd_hot_grid();
  size_t lds = static_cast<size_t>(gp.hot_codes) * p.hot_n * 2 * sizeof(float);
  lds = lds < 16 ? 16 : lds;                      // the idle LDS read of a launch without hot rows
  gp.n_row_blocks = static_cast<int64_t>(grid) * 16;
  hipLaunchKernelGGL(spmm_bwd_hot_kernel, dim3(static_cast<unsigned>(grid)), dim3(1024), lds, st, p, gp);
  if (int rc = gnan::check_launch("spmm_bwd_hot_kernel")) return rc;
  if (p.n_slices > 0) {
    hipLaunchKernelGGL(spmm_lut_grad_fixup_kernel<true>, dim3(static_cast<unsigned>((p.n_long + 3) / 4)), dim3(256), 0, st, p, gp);
    if (int rc = gnan::check_launch("spmm_lut_grad_fixup_kernel")) return rc;
  }
  hipLaunchKernelGGL(spmm_lut_grad_final_kernel, dim3(1), dim3(1024), 0, st, gp.blk, gp.n_row_blocks + p.n_long, p.D, dlut,
                     gp.rest_total, gp.rest_q, gp.w_real);
  return gnan::check_launch("spmm_lut_grad_final_kernel");
}

// ---------------------------------------------------------------------------------------------
// Table gradient on the DENSE layout (every pair listed, up to 256 hop codes; Cw == 1, global table):
//   dlut[d] = sum_q inv(q, d) * sum_{j : code(q, j) == d} < dY[q, :], S[j, :] >
// — what gnan_spmm_shell_sums + six framework launches computed through a [n, D, W] tensor of read-modify-writes in
// global memory (Cora-shaped: 0.59 ms of a 2.7-ms training step; a 30-node graph: 8 of its 34 launches).  One wave per
// row: lane l takes neighbours l, l + 64, ..., forms the W-term dot product and adds it to ITS column of the wave's
// [D][64] LDS bins (no atomics, no conflicts by construction); lane d then adds bin row d front to back, scales by
// 1 / count and keeps a float64 running sum over the wave's rows.  One record per wave, a fixed-order final pass:
// bit-reproducible.
// ---------------------------------------------------------------------------------------------
constexpr int kBinStride = kWave + 1;        // bin rows one bank apart: lane d's walk along row d does not collide with lane d + 1's

__global__ __launch_bounds__(256) void dense_lut_grad_kernel(const Params p, const GradParams gp, int waves_total) {
  extern __shared__ __attribute__((aligned(16))) float dense_bins[];    // [waves per block][D][65]
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int wpb = blockDim.x / kWave;
  float* mine = dense_bins + static_cast<size_t>(wave) * p.D * kBinStride;
  const int rest = p.D - 1;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};      // codes lane, lane + 64, lane + 128, lane + 192
  for (int64_t base = static_cast<int64_t>(blockIdx.x) * wpb; base < p.n_rows; base += waves_total) {
    const int64_t q = base + wave;
    const bool live = q < p.n_rows;
    const int64_t i = live ? adj_row(p, q) : 0;
    for (int d = 0; d < p.D; ++d) mine[d * kBinStride + lane] = 0.f;
    if (live) {
      const float* dy = gp.dY + q * gp.dy_stride;
      const uint8_t* codes = p.code + i * p.n_cols;
      for (int64_t j = lane; j < p.n_cols; j += kWave) {
        int d = codes[j];
        d = d < rest ? d : rest;
        const float* srow = static_cast<const float*>(p.S) + j * p.s_stride;
        float dot = 0.f;
        for (int w = 0; w < p.W; ++w) dot = fmaf(dy[w % gp.dy_channels], srow[w], dot);
        mine[d * kBinStride + lane] += dot;
      }
    }
    __syncthreads();                           // (uniform trip count: every wave of the block sees the same `base`)
    if (live) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int d = lane + k * kWave;
        if (d < p.D) {
          float s = 0.f;
          for (int l = 0; l < kWave; ++l) s += mine[d * kBinStride + l];
          if (p.cnt) {
            const int c = p.cnt[i * p.cnt_stride + d];
            s *= 1.f / static_cast<float>(c > 1 ? c : 1);
          }
          acc[k] += static_cast<double>(s);
        }
      }
    }
    __syncthreads();
  }
  const int64_t gw = static_cast<int64_t>(blockIdx.x) * wpb + wave;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int d = lane + k * kWave;
    if (d < p.D && gw < waves_total) gp.blk[gw * p.D + d] = acc[k];
  }
}

// one workgroup per hop code: 256 threads stride over the waves' records, then a fixed tree
__global__ __launch_bounds__(256) void dense_lut_grad_final_kernel(const double* __restrict__ blk, int waves_total, int D,
                                                                   float* __restrict__ out) {
  __shared__ double red[256];
  const int d = blockIdx.x;
  double s = 0.0;
  for (int w = threadIdx.x; w < waves_total; w += 256) s += blk[static_cast<int64_t>(w) * D + d];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if (static_cast<int>(threadIdx.x) < st) red[threadIdx.x] += red[threadIdx.x + st];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[d] = static_cast<float>(red[0]);
}

bool dense_lut_grad_applies(const gnan_spmm_args* a, int32_t reduce_rows) {
  return a->rowptr == nullptr && a->Cw == 1 && a->D <= 256 && reduce_rows && a->s_dtype == GNAN_F32 && !a->weight_by_col &&
         a->s_total == nullptr && a->lut_row_stride == 0 && !a->s_by_code;
}

int dense_lut_grad_waves(const gnan_spmm_args* a) {      // one wave per row up to 2048 waves
  return static_cast<int>(a->n_rows < 2048 ? (a->n_rows < 1 ? 1 : a->n_rows) : 2048);
}

int launch_dense_lut_grad(const Params& p, GradParams gp, const gnan_spmm_args* a, hipStream_t st, float* dlut) {
  const size_t per_wave = static_cast<size_t>(p.D) * kBinStride * sizeof(float);
  int wpb = static_cast<int>((64 * 1024) / per_wave);
  wpb = wpb < 1 ? 1 : (wpb > 4 ? 4 : wpb);
  int waves = dense_lut_grad_waves(a);
  waves = (waves + wpb - 1) / wpb * wpb;                    // whole workgroups
  const size_t lds = per_wave * wpb;
  if (lds > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(dense_lut_grad_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       static_cast<int>(lds));
    if (e != hipSuccess) return gnan::fail(GNAN_ERR_HIP, "lut_grad: hipFuncSetAttribute: %s", hipGetErrorString(e));
  }
  hipLaunchKernelGGL(dense_lut_grad_kernel, dim3(static_cast<unsigned>(waves / wpb)), dim3(wpb * kWave), lds, st, p, gp, waves);
  if (int rc = gnan::check_launch("dense_lut_grad_kernel")) return rc;
  hipLaunchKernelGGL(dense_lut_grad_final_kernel, dim3(static_cast<unsigned>(p.D)), dim3(256), 0, st, gp.blk, waves, p.D, dlut);
  return gnan::check_launch("dense_lut_grad_final_kernel");
}

__global__ void zero_floats_kernel(float* out, int n) {     // (a kernel: captured memsets replay wrongly on ROCm 7.2)
  for (int i = threadIdx.x; i < n; i += blockDim.x) out[i] = 0.f;
}

template <int VEC>
int launch_lut_grad_lpr(const Params& p, const GradParams& gp, int lpr, hipStream_t st, float* dlut) {
  return dispatch_lpr(lpr, [&](auto L) { return launch_lut_grad<VEC, decltype(L)::value>(p, gp, st, dlut); });
}

size_t lut_grad_blk_entries(const gnan_spmm_args* a, int vec, int lpr) {
  const int G = kWave / lpr;
  return static_cast<size_t>((a->n_rows + 4 * G - 1) / (4 * G)) + static_cast<size_t>(a->n_long > 0 ? a->n_long : 0);
}

}  // namespace

static size_t lut_grad_workspace_bytes(const gnan_spmm_args* a, int32_t reduce_rows) {
  if (!a || a->n_rows <= 0) return 0;
  if (dense_lut_grad_applies(a, reduce_rows))              // one [D] float64 record per wave (rounded up to whole workgroups)
    return (static_cast<size_t>(dense_lut_grad_waves(a)) + 4) * static_cast<size_t>(a->D) * sizeof(double);
  int vec, lpr;
  pick_tiling(a, static_cast<const float*>(a->S), a->s_stride, &vec, &lpr);
  size_t bytes = slice_T_bytes(a);
  if (reduce_rows) bytes += lut_grad_blk_entries(a, vec, lpr) * 4 * sizeof(double);
  return bytes;
}

extern "C" size_t gnan_spmm_lut_grad_workspace_bytes(const gnan_spmm_lut_grad_args* g) {
  return g ? lut_grad_workspace_bytes(&g->spmm, g->reduce_rows) : 0;
}

extern "C" int gnan_spmm_lut_grad(const gnan_spmm_lut_grad_args* g, gnan_stream_t stream) {
  GNAN_REQUIRE(g != nullptr, "lut_grad: null args");
  if (int rc = forward_only_self_sum(&g->spmm, "lut_grad")) return rc;
  const gnan_spmm_args* a = &g->spmm;
  const float* dY = g->dY;
  const int64_t dy_stride = g->dy_stride;
  const int32_t dy_channels = g->dy_channels, reduce_rows = g->reduce_rows;
  float* dwt = g->dwt;
  void* workspace = g->workspace;
  const size_t workspace_bytes = g->workspace_bytes;
  if (int rc = validate(a)) return rc;
  if (int rc = forward_only_index(a, "lut_grad")) return rc;
  GNAN_REQUIRE(dwt != nullptr, "lut_grad: null output");
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (a->n_rows == 0) {
    if (reduce_rows) {
      hipLaunchKernelGGL(zero_floats_kernel, dim3(1), dim3(64), 0, st, dwt, a->D);
      return gnan::check_launch("zero_floats_kernel");
    }
    return GNAN_OK;
  }
  GNAN_REQUIRE(dY != nullptr && dy_channels >= 1 && dy_stride >= dy_channels, "lut_grad: bad dY");
  if (dense_lut_grad_applies(a, reduce_rows)) {
    GNAN_REQUIRE(a->W % dy_channels == 0, "lut_grad: dy_channels must be a divisor of W");
    const size_t need = lut_grad_workspace_bytes(a, reduce_rows);
    if (workspace == nullptr || workspace_bytes < need)
      return gnan::fail(GNAN_ERR_WORKSPACE, "lut_grad: workspace %zu B < required %zu B", workspace_bytes, need);
    const Params p = make_params(a);
    GradParams gp{};
    gp.dY = dY; gp.dy_stride = dy_stride; gp.dy_channels = dy_channels; gp.dwt = dwt; gp.reduce_rows = 1;
    gp.blk = static_cast<double*>(workspace);
    return launch_dense_lut_grad(p, gp, a, st, dwt);
  }
  if (a->rowptr == nullptr || a->D > 4 || a->Cw != 1 || a->s_dtype != GNAN_F32 || a->weight_by_col)
    return gnan::fail(GNAN_ERR_UNSUPPORTED, "lut_grad: needs the CSR layout with D <= 4 — or the dense layout with a global table, "
                      "reduce_rows and no rest-bucket total —, one weight channel and fp32 operand rows");
  GNAN_REQUIRE(a->W % dy_channels == 0, "lut_grad: dy_channels must divide W");
  const size_t need = lut_grad_workspace_bytes(a, reduce_rows);
  if (need > 0 && (workspace == nullptr || workspace_bytes < need))
    return gnan::fail(GNAN_ERR_WORKSPACE, "lut_grad: workspace %zu B < required %zu B", workspace_bytes, need);
  const Params p = make_params(a);
  int vec, lpr;
  pick_tiling(a, static_cast<const float*>(a->S), a->s_stride, &vec, &lpr);
  GradParams gp;
  gp.dY = dY; gp.dy_stride = dy_stride; gp.dy_channels = dy_channels; gp.dwt = dwt; gp.reduce_rows = reduce_rows;
  gp.ds_add = nullptr; gp.ds_scale = nullptr; gp.rest_total = nullptr; gp.rest_q = nullptr; gp.w_real = 0;
  gp.slice_T = static_cast<float*>(workspace);
  gp.blk = reinterpret_cast<double*>(static_cast<char*>(workspace) + slice_T_bytes(a));
  gp.n_row_blocks = 0;
  return vec == 4 ? launch_lut_grad_lpr<4>(p, gp, lpr, st, dwt) : launch_lut_grad_lpr<1>(p, gp, lpr, st, dwt);
}

static size_t bwd_narrow_workspace_bytes(const gnan_spmm_args* a) {
  if (!a || a->n_rows <= 0) return 0;
  const int half = a->W / 2;
  const int vec = half <= 2 ? 2 * (half < 1 ? 1 : half) : 4;
  const int lpr = a->W / vec >= 1 ? a->W / vec : 1;
  size_t bytes = slice_T_bytes(a);
  const size_t entries = bwd_hot_applies(a) ? bwd_hot_blk_entries(a) : lut_grad_blk_entries(a, vec, lpr);
  return bytes + entries * 4 * sizeof(double);
}

extern "C" size_t gnan_spmm_bwd_narrow_workspace_bytes(const gnan_spmm_bwd_narrow_args* g) {
  return g ? bwd_narrow_workspace_bytes(&g->spmm) : 0;
}

extern "C" int gnan_spmm_bwd_narrow(const gnan_spmm_bwd_narrow_args* g, gnan_stream_t stream) {
  GNAN_REQUIRE(g != nullptr, "bwd_narrow: null args");
  if (int rc = forward_only_self_sum(&g->spmm, "bwd_narrow")) return rc;
  const gnan_spmm_args* a = &g->spmm;
  const float* s_rows = g->s_rows;
  const int64_t s_rows_stride = g->s_rows_stride, ds_stride = g->ds_stride;
  const int32_t w_real = g->w_real, with_rest = g->with_rest;
  float* dS = g->dS;
  float* dlut = g->dlut;
  void* workspace = g->workspace;
  const size_t workspace_bytes = g->workspace_bytes;
  if (int rc = validate(a)) return rc;
  if (int rc = forward_only_index(a, "bwd_narrow", true)) return rc;
  GNAN_REQUIRE(!a->packed_index || a->W == 2, "bwd_narrow: packed index entries are read for one-channel operands only (W == 2)");
  GNAN_REQUIRE(dS != nullptr && dlut != nullptr && (s_rows != nullptr || a->n_rows == 0), "bwd_narrow: null pointer");
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (a->rowptr == nullptr || a->D > 4 || a->Cw != 1 || a->s_dtype != GNAN_F32 || a->lut_row_stride != 0 || a->cnt != nullptr)
    return gnan::fail(GNAN_ERR_UNSUPPORTED, "bwd_narrow: needs the CSR layout, D <= 4, one global weight channel, fp32 rows, no cnt");
  const int half = a->W / 2;
  if (a->W < 2 || a->W > 64 || (a->W & (a->W - 1)) != 0 || w_real < 1 || w_real > half || a->s_stride != a->W)
    return gnan::fail(GNAN_ERR_UNSUPPORTED, "bwd_narrow: operand rows must be 2 * half floats, half a power of two in [w_real, 32] (got W=%d, w_real=%d)", a->W, w_real);
  GNAN_REQUIRE(s_rows_stride >= w_real && ds_stride >= w_real, "bwd_narrow: row stride smaller than the width");
  GNAN_REQUIRE((g->rest_total == nullptr) == (g->rest_q == nullptr), "bwd_narrow: rest_total and rest_q come together");
  GNAN_REQUIRE(g->rest_total == nullptr || with_rest, "bwd_narrow: rest_total without a rest bucket");
  if (a->n_rows == 0) {
    hipLaunchKernelGGL(zero_floats_kernel, dim3(1), dim3(64), 0, st, dlut, a->D);
    return gnan::check_launch("zero_floats_kernel");
  }
  const size_t need = bwd_narrow_workspace_bytes(a);
  if (need > 0 && (workspace == nullptr || workspace_bytes < need))
    return gnan::fail(GNAN_ERR_WORKSPACE, "bwd_narrow: workspace %zu B < required %zu B", workspace_bytes, need);
  const Params p = make_params(a);
  // the two halves of a row must sit in different lanes, partner = lane + LPR / 2: VEC = min(4, half), LPR = 2 * half / VEC
  if (reinterpret_cast<uintptr_t>(a->S) % 16 != 0)
    return gnan::fail(GNAN_ERR_UNSUPPORTED, "bwd_narrow: operand rows must be 16-byte aligned");
  GradParams gp;
  gp.dY = nullptr; gp.dy_stride = 0; gp.dy_channels = 1; gp.dwt = dlut; gp.reduce_rows = 1;
  gp.slice_T = static_cast<float*>(workspace);
  gp.blk = reinterpret_cast<double*>(static_cast<char*>(workspace) + slice_T_bytes(a));
  gp.n_row_blocks = 0;
  gp.s_rows = s_rows; gp.s_rows_stride = s_rows_stride; gp.half = half; gp.w_real = w_real;
  gp.dS = dS; gp.ds_stride = ds_stride; gp.with_rest = with_rest; gp.ds_add = g->ds_add;
  gp.ds_scale = g->ds_add ? g->ds_add_scale : nullptr;
  gp.rest_total = g->rest_total; gp.rest_q = g->rest_q;
  gp.hot_code_lo = 0; gp.hot_codes = 0;
  if (bwd_hot_applies(a)) {
    // one-channel operands over a packed index stream: the persistent kernel, with the head of the appended hot rows in LDS
    Params ph = p;
    if (a->hot_rows > 0) {
      GNAN_REQUIRE(g->hot_codes >= 1 && g->hot_code_lo >= 0 && g->hot_code_lo + g->hot_codes <= a->D,
                   "bwd_narrow: hot code blocks outside [0, D)");
      GNAN_REQUIRE(a->hot_lo >= 0 && a->hot_lo + a->hot_rows <= a->n_cols, "bwd_narrow: hot rows outside the packed rows");
      GNAN_REQUIRE(static_cast<int64_t>(a->hot_rows) * g->hot_codes * 2 <= kHotLdsFloats, "bwd_narrow: hot rows exceed 64 KB of LDS");
      gp.hot_code_lo = g->hot_code_lo; gp.hot_codes = g->hot_codes;
    } else {
      ph.hot_lo = 0; ph.hot_n = 0;
    }
    return launch_bwd_hot(ph, gp, st, dlut);
  }
  switch (half) {      // one lane per row while a row is one 8- or 16-byte load (64 rows per wavefront instead of 32)
    case 1: return launch_lut_grad<2, 1, true>(p, gp, st, dlut);
    case 2: return launch_lut_grad<4, 1, true>(p, gp, st, dlut);
    case 4: return launch_lut_grad<4, 2, true>(p, gp, st, dlut);
    case 8: return launch_lut_grad<4, 4, true>(p, gp, st, dlut);
    case 16: return launch_lut_grad<4, 8, true>(p, gp, st, dlut);
    default: return launch_lut_grad<4, 16, true>(p, gp, st, dlut);
  }
}
