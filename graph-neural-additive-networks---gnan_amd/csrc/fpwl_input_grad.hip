// Input gradients of the shape functions on the table path (gfx950): autograd through GNAN.py:57-62 w.r.t. x.
//
// f_k is piecewise linear in x[n, k], so its input gradient is one table look-up per (node, feature):
//     gx[n, k] = sum_c g[n, k, c] * dfdx[off[k] + i, c],     i = #{ breakpoints of f_k <= x[n, k] }
// with the piece i the forward pass put the node on.  Two kernels:
//
//   pwl_dfdx_kernel        dfdx [T, C]: the derivative of every piece, taken where the parameter gradients take the
//                          piece's activation masks (csrc/piece_points.hpp) — forward mode in float64 through the
//                          hidden layers, strict masks z > 0, one rounding.  The table's `slope` is NOT that number on a
//                          point piece [a, nextafter(a)): there it is the divided difference right of a kink, while
//                          autograd differentiates AT the kink with relu'(0) = 0 (zero biases + one-hot features: most
//                          look-ups).  One workgroup per feature, weights in LDS, a wave per piece, lane = hidden unit.
//   fpwl_input_grad_kernel the look-up: a workgroup owns a block of nodes and a feature group of the table plan, stages
//                          the group's anchors and dfdx rows in LDS ((1 + C) floats per piece: less than the forward's
//                          image), thread = (node, up to 4 features) searches as csrc/fpwl.hip:fpwl_kernel does (search<FPT>,
//                          csrc/fpwl_common.hpp) and sums the channels by a chain of fused multiply-adds.  x in, gx out, the
//                          gradient rows once: ~8 B per look-up with one channel.  No atomics, no cross-thread sums:
//                          bit-reproducible, and a NaN stays in the element it belongs to.
#include "fpwl_common.hpp"
#include "piece_points.hpp"

namespace {
using namespace gnan::fpwl;

// ---------------------------------------------------------------------------------------------------------------------
// per-piece derivatives
// ---------------------------------------------------------------------------------------------------------------------
constexpr int kDfdxWaves = 16;   // a feature has ~130-250 pieces: 9-16 rounds; each round is a latency chain of L - 1 layers

struct DfdxParams {
  const int32_t* off;
  const float* anchor;
  int64_t T;
  const float* w1;
  const float* b1;
  const float* Wm;      // [L - 2, F, H, H]
  const float* bm;      // [L - 2, F, H]
  const float* Wl;      // [F, C, H]
  int F, L, H, C;
  float* dfdx;
  int wl_in_lds;        // the last layer's rows are staged in LDS (row stride H + 1), else read from global memory
  int n_zero_blocks;    // workgroups behind the F feature workgroups: they zero rows [off[F], T)
};

// Dynamic LDS: [kDfdxWaves][2 buffers][h | d][H] float64, then float: w1 [H], b1 [H], Wm [L - 2][H][H + 1], bm [L - 2][H],
// Wl [C][H + 1] (wl_in_lds).  A wave takes pieces wave, wave + kDfdxWaves, ...; every wave runs the same number of rounds, so the
// barriers between the layers are uniform.
__global__ __launch_bounds__(64 * kDfdxWaves) void pwl_dfdx_kernel(const DfdxParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  constexpr int BS = 64 * kDfdxWaves;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int H = p.H, C = p.C, HS = H + 1, NM = p.L - 2;
  if (static_cast<int>(blockIdx.x) >= p.F) {
    const int64_t lo = static_cast<int64_t>(p.off[p.F]) * C, hi = p.T * C;
    for (int64_t e = lo + (static_cast<int64_t>(blockIdx.x) - p.F) * BS + tid; e < hi; e += static_cast<int64_t>(p.n_zero_blocks) * BS)
      p.dfdx[e] = 0.f;
    return;
  }
  const int k = blockIdx.x;
  double* hd = reinterpret_cast<double*>(smem_raw);
  float* w1_l = reinterpret_cast<float*>(hd + kDfdxWaves * 4 * H);
  float* b1_l = w1_l + H;
  float* Wm_l = b1_l + H;
  float* bm_l = Wm_l + NM * H * HS;
  float* Wl_l = bm_l + NM * H;
  for (int i = tid; i < H; i += BS) {
    w1_l[i] = p.w1[static_cast<int64_t>(k) * H + i];
    b1_l[i] = p.b1 ? p.b1[static_cast<int64_t>(k) * H + i] : 0.f;
  }
  for (int l = 0; l < NM; ++l) {
    const float* W = p.Wm + (static_cast<int64_t>(l) * p.F + k) * H * H;
    for (int e = tid; e < H * H; e += BS) Wm_l[l * H * HS + (e / H) * HS + e % H] = W[e];
    for (int i = tid; i < H; i += BS) bm_l[l * H + i] = p.bm ? p.bm[(static_cast<int64_t>(l) * p.F + k) * H + i] : 0.f;
  }
  const float* Wl_g = p.Wl + static_cast<int64_t>(k) * C * H;
  if (p.wl_in_lds)
    for (int e = tid; e < C * H; e += BS) Wl_l[(e / H) * HS + e % H] = Wl_g[e];
  __syncthreads();
  const float* Wl = p.wl_in_lds ? Wl_l : Wl_g;       // (flat addressing: either memory)
  const int WS = p.wl_in_lds ? HS : H;
  const int base = p.off[k], P = p.off[k + 1] - base;
  const int rounds = P > 0 ? (P + kDfdxWaves - 1) / kDfdxWaves : 0;
  double* buf0 = hd + wave * 4 * H;                    // [h | d] of the layer just evaluated
  double* buf1 = buf0 + 2 * H;
  for (int r = 0; r < rounds; ++r) {
    const int li_raw = r * kDfdxWaves + wave;
    const bool active = li_raw < P && static_cast<int64_t>(base) + li_raw < p.T;
    const int li = active ? li_raw : P - 1;            // idle waves repeat the last piece and store nothing
    double a, xi;
    gnan::piece_points(p.anchor + base, li, P, &a, &xi);
    double* cur = buf0;
    double* nxt = buf1;
    for (int i = lane; i < H; i += 64) {
      const double w = static_cast<double>(w1_l[i]);
      const double z = fma(w, xi, static_cast<double>(b1_l[i]));
      const bool on = z > 0.0;
      cur[i] = on ? z : 0.0;
      cur[H + i] = on ? w : 0.0;
    }
    __syncthreads();
    for (int l = 0; l < NM; ++l) {
      for (int j = lane; j < H; j += 64) {
        const float* row = Wm_l + l * H * HS + j * HS;
        // four independent chains each: the sums are latency-bound (float64 fma behind an LDS read), not throughput-bound
        double zq[4] = {static_cast<double>(bm_l[l * H + j]), 0.0, 0.0, 0.0}, dq[4] = {0.0, 0.0, 0.0, 0.0};
        int i = 0;
        for (; i + 3 < H; i += 4) {
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const double w = static_cast<double>(row[i + u]);
            zq[u] = fma(w, cur[i + u], zq[u]);
            dq[u] = fma(w, cur[H + i + u], dq[u]);
          }
        }
        for (; i < H; ++i) {
          const double w = static_cast<double>(row[i]);
          zq[0] = fma(w, cur[i], zq[0]);
          dq[0] = fma(w, cur[H + i], dq[0]);
        }
        const double z = (zq[0] + zq[1]) + (zq[2] + zq[3]), dz = (dq[0] + dq[1]) + (dq[2] + dq[3]);
        const bool on = z > 0.0;
        nxt[j] = on ? z : 0.0;
        nxt[H + j] = on ? dz : 0.0;
      }
      __syncthreads();
      double* t = cur; cur = nxt; nxt = t;
    }
    for (int c = lane; c < C; c += 64) {
      const float* row = Wl + static_cast<int64_t>(c) * WS;
      double sq[4] = {0.0, 0.0, 0.0, 0.0};
      int i = 0;
      for (; i + 3 < H; i += 4) {
#pragma unroll
        for (int u = 0; u < 4; ++u) sq[u] = fma(static_cast<double>(row[i + u]), cur[H + i + u], sq[u]);
      }
      for (; i < H; ++i) sq[0] = fma(static_cast<double>(row[i]), cur[H + i], sq[0]);
      const double s = (sq[0] + sq[1]) + (sq[2] + sq[3]);
      if (active) p.dfdx[(static_cast<int64_t>(base) + li) * C + c] = static_cast<float>(s);
    }
    __syncthreads();                                   // the next round rewrites the buffers
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// the look-up
// ---------------------------------------------------------------------------------------------------------------------
struct InputGradParams {
  const float* x;
  int64_t n, x_stride;
  int F, C;
  const int32_t* off;
  const float* anchor;
  const float* dfdx;
  int step0;             // largest power of two <= max breakpoints per feature (0 if none)
  int n_groups;
  int nodes_per_block;
  int sum_features;
  int max_group_pieces;  // pieces the LDS image holds
  const float* grad;
  int64_t grad_stride;
  float* gx;
  int64_t gx_stride;
};

struct Plan {
  int block_size, nodes_per_block, n_groups, vec;
  size_t lds;
  int64_t n_blocks;
};

// Thread = (node, FPT features): Map (csrc/fpwl_common.hpp).  VEC: FPT == 4 and a quad of x / gx is one 16-byte request.
template <int FG, int BS, bool VEC>
__global__ __launch_bounds__(BS) void fpwl_input_grad_kernel(const InputGradParams p) {
  constexpr int FPT = Map<FG, BS>::FPT, TPN = Map<FG, BS>::TPN, NODES = Map<FG, BS>::NODES;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  __shared__ int s_off[FG + 1];
  const int tid = threadIdx.x;
  const int q = tid % TPN, nl = tid / TPN;
  const int C = p.C, Cs = table_stride(C);
  int g;
  int64_t nb;
  xcd_block(blockIdx.x, p.n_groups, nb, g);
  const int64_t n_lo = nb * p.nodes_per_block;
  if (n_lo >= p.n) return;
  const int64_t n_hi = n_lo + p.nodes_per_block < p.n ? n_lo + p.nodes_per_block : p.n;
  const int k0 = g * FG;
  const int nf = p.F - k0 < FG ? p.F - k0 : FG;
  const int base = p.off[k0];
  int tot = p.off[k0 + nf] - base;
  tot = tot < p.max_group_pieces ? tot : p.max_group_pieces;      // never beyond the image the launch reserved
  float* anchor_l = smem;
  float* d_l = smem + p.max_group_pieces;
  for (int i = tid; i < tot; i += BS) anchor_l[i] = p.anchor[base + i];
  if (Cs == C) {
    for (int i = tid; i < tot * C; i += BS) d_l[i] = p.dfdx[static_cast<int64_t>(base) * C + i];
  } else {
    for (int i = tid; i < tot * C; i += BS) {
      const int r = i / C;
      d_l[r * Cs + (i - r * C)] = p.dfdx[static_cast<int64_t>(base) * C + i];
    }
  }
  if (tid <= nf) {
    const int o = p.off[k0 + tid] - base;
    s_off[tid] = o < tot ? o : tot;
  }
  __syncthreads();
  int po[FPT], pn[FPT];
  bool live[FPT];
#pragma unroll
  for (int f = 0; f < FPT; ++f) {
    const int fg = q * FPT + f;
    live[f] = fg < nf;
    po[f] = live[f] ? s_off[fg] : 0;
    pn[f] = live[f] ? s_off[fg + 1] - s_off[fg] - 1 : 0;
    pn[f] = pn[f] > 0 ? pn[f] : 0;
    live[f] = live[f] && s_off[fg + 1] > s_off[fg];
  }
  for (int64_t n = n_lo + nl; n < n_hi; n += NODES) {
    float xv[FPT];
    const float* xr = p.x + n * p.x_stride + k0 + q * FPT;
    if constexpr (VEC) {
      if (live[0]) {
        const float4 t = *reinterpret_cast<const float4*>(xr);
        xv[0] = t.x; xv[1 % FPT] = t.y; xv[2 % FPT] = t.z; xv[3 % FPT] = t.w;
      } else {
#pragma unroll
        for (int f = 0; f < FPT; ++f) xv[f] = 0.f;
      }
    } else {
#pragma unroll
      for (int f = 0; f < FPT; ++f) xv[f] = live[f] ? xr[f] : 0.f;
    }
    // i = #{ j in 1..pn : anchor[po + j] <= x }: search<FPT> (csrc/fpwl_common.hpp), FPT features in lock-step.  Written out:
    // through the helper fpwl_input_grad_kernel<4, 256, false> took 78 registers for 80 and all instances other code
    // (profiles/r21_fpwl_split_code_objects.txt)
    int idx[FPT];
#pragma unroll
    for (int f = 0; f < FPT; ++f) idx[f] = 0;
    for (int step = p.step0; step > 0; step >>= 1) {
#pragma unroll
      for (int f = 0; f < FPT; ++f) {
        const int j = idx[f] + step;
        const int jj = j <= pn[f] ? j : 0;
        const float a = anchor_l[po[f] + jj];
        idx[f] = (j <= pn[f] && a <= xv[f]) ? j : idx[f];
      }
    }
    float acc[FPT];
#pragma unroll
    for (int f = 0; f < FPT; ++f) {
      idx[f] = (idx[f] + po[f]) * Cs;
      acc[f] = 0.f;
    }
    const float* gr = p.grad + n * p.grad_stride;
    if (p.sum_features) {
      for (int c = 0; c < C; ++c) {
        const float gc = gr[c];
#pragma unroll
        for (int f = 0; f < FPT; ++f) acc[f] = fmaf(gc, d_l[idx[f] + c], acc[f]);
      }
    } else {
      const float* gq = gr + static_cast<int64_t>(k0 + q * FPT) * C;
#pragma unroll
      for (int f = 0; f < FPT; ++f) {
        if (live[f])
          for (int c = 0; c < C; ++c) acc[f] = fmaf(gq[f * C + c], d_l[idx[f] + c], acc[f]);
      }
    }
    float* o = p.gx + n * p.gx_stride + k0 + q * FPT;
    if constexpr (VEC) {
      if (live[0]) *reinterpret_cast<float4*>(o) = make_float4(acc[0], acc[1 % FPT], acc[2 % FPT], acc[3 % FPT]);
    } else {
#pragma unroll
      for (int f = 0; f < FPT; ++f)
        if (live[f]) o[f] = acc[f];
    }
  }
}

template <int FG, int BS>
int launch_input_grad(const InputGradParams& p, const Plan& plan, hipStream_t st) {
  const int64_t wgs = (plan.n_blocks + 7) / 8 * 8 * p.n_groups;      // see xcd_block
  if (wgs > 0x7fffffffLL) return gnan::fail(GNAN_ERR_UNSUPPORTED, "fpwl_input_grad: too many nodes for one launch");
  auto go = [&](auto kernel) { return launch_with_lds(kernel, "fpwl_input_grad_kernel", dim3(static_cast<unsigned>(wgs)), BS, plan.lds, st, p); };
  if constexpr (FG % 4 == 0) {
    if (plan.vec) return go(fpwl_input_grad_kernel<FG, BS, true>);
  }
  return go(fpwl_input_grad_kernel<FG, BS, false>);
}

// Validation and plan of a call: shared by the launch and by the query, which stops short of the launch.
int plan_input_grad(const gnan_fpwl_input_grad_args* a, Plan* plan) {
  GNAN_REQUIRE(a != nullptr, "fpwl_input_grad: null args");
  GNAN_REQUIRE(a->n >= 0 && a->F >= 1 && a->C >= 1, "fpwl_input_grad: bad sizes");
  *plan = Plan{};
  if (a->n == 0) return GNAN_OK;
  GNAN_REQUIRE(a->max_pieces >= 1 && a->max_group_pieces >= 1, "fpwl_input_grad: max_pieces / max_group_pieces must be >= 1");
  const int fg = a->features_per_group;
  GNAN_REQUIRE(fg == 1 || fg == 2 || fg == 4 || fg == 8 || fg == 16, "fpwl_input_grad: features_per_group must be 1, 2, 4, 8 or 16");
  const size_t cs = static_cast<size_t>(table_stride(a->C));
  const size_t image = static_cast<size_t>(a->max_group_pieces) * (1 + 2 * cs) * sizeof(float);   // the forward's (pwl.oversize)
  if (image > 150 * 1024)
    return gnan::fail(GNAN_ERR_UNSUPPORTED, "fpwl_input_grad: %zu B of tables per feature group exceed the thread-per-node look-up's LDS image", image);
  GNAN_REQUIRE(a->x && a->off && a->anchor && a->dfdx && a->grad && a->gx, "fpwl_input_grad: null pointer");
  GNAN_REQUIRE(a->x_stride >= a->F && a->gx_stride >= a->F, "fpwl_input_grad: x / gx row stride smaller than F");
  const int64_t gw = a->sum_features ? a->C : static_cast<int64_t>(a->F) * a->C;
  GNAN_REQUIRE(a->grad_stride >= gw, "fpwl_input_grad: grad row stride smaller than the gradient width");
  auto aligned = [](const void* ptr) { return (reinterpret_cast<uintptr_t>(ptr) % 16) == 0; };
  plan->block_size = fg >= 8 ? 512 : 256;
  plan->nodes_per_block = small_batch_block(a->n);
  plan->n_groups = (a->F + fg - 1) / fg;
  plan->vec = fg % 4 == 0 && a->F % 4 == 0 && a->x_stride % 4 == 0 && a->gx_stride % 4 == 0 && aligned(a->x) && aligned(a->gx);
  plan->lds = static_cast<size_t>(a->max_group_pieces) * (1 + cs) * sizeof(float);
  plan->n_blocks = (a->n + plan->nodes_per_block - 1) / plan->nodes_per_block;
  return GNAN_OK;
}

}  // namespace

extern "C" int gnan_fpwl_input_grad_describe(const gnan_fpwl_input_grad_args* a, gnan_fpwl_input_grad_info* out) {
  GNAN_REQUIRE(out != nullptr, "fpwl_input_grad_describe: null out");
  *out = gnan_fpwl_input_grad_info{};
  Plan plan;
  if (int rc = plan_input_grad(a, &plan)) return rc;
  if (a->n == 0) return GNAN_OK;
  out->block_size = plan.block_size;
  out->nodes_per_block = plan.nodes_per_block;
  out->features_per_group = a->features_per_group;
  out->lds_bytes = static_cast<int32_t>(plan.lds);
  out->vec = plan.vec;
  out->n_groups = plan.n_groups;
  out->n_blocks = plan.n_blocks;
  return GNAN_OK;
}

extern "C" int gnan_fpwl_input_grad(const gnan_fpwl_input_grad_args* a, gnan_stream_t stream) {
  Plan plan;
  if (int rc = plan_input_grad(a, &plan)) return rc;
  if (a->n == 0) return GNAN_OK;
  InputGradParams p;
  p.x = a->x; p.n = a->n; p.x_stride = a->x_stride; p.F = a->F; p.C = a->C;
  p.off = a->off; p.anchor = a->anchor; p.dfdx = a->dfdx;
  p.step0 = step0_of(a->max_pieces);
  p.n_groups = plan.n_groups;
  p.nodes_per_block = plan.nodes_per_block;
  p.sum_features = a->sum_features ? 1 : 0;
  p.max_group_pieces = a->max_group_pieces;
  p.grad = a->grad; p.grad_stride = a->grad_stride;
  p.gx = a->gx; p.gx_stride = a->gx_stride;
  hipStream_t st = static_cast<hipStream_t>(stream);
  switch (a->features_per_group) {
    case 1: return launch_input_grad<1, 256>(p, plan, st);
    case 2: return launch_input_grad<2, 256>(p, plan, st);
    case 4: return launch_input_grad<4, 256>(p, plan, st);
    case 8: return launch_input_grad<8, 512>(p, plan, st);
    default: return launch_input_grad<16, 512>(p, plan, st);
  }
}

extern "C" int gnan_pwl_piece_dfdx(const gnan_pwl_dfdx_args* a, gnan_stream_t stream) {
  GNAN_REQUIRE(a != nullptr, "pwl_piece_dfdx: null args");
  GNAN_REQUIRE(a->F >= 1 && a->H >= 1 && a->C >= 1 && a->T >= 0, "pwl_piece_dfdx: bad sizes");
  if (a->L < 2 || a->L > 4) return gnan::fail(GNAN_ERR_UNSUPPORTED, "pwl_piece_dfdx: kernel covers L in {2, 3, 4} (got %d)", a->L);
  if (a->C > 4096 || a->H > (a->L >= 3 ? 64 : 128))
    return gnan::fail(GNAN_ERR_UNSUPPORTED, "pwl_piece_dfdx: H <= %d and C <= 4096 (got H=%d, C=%d)", a->L >= 3 ? 64 : 128, a->H, a->C);
  GNAN_REQUIRE(a->off && a->anchor && a->w_first && a->w_last && a->dfdx, "pwl_piece_dfdx: null pointer");
  if (a->L >= 3) GNAN_REQUIRE(a->w_mid != nullptr, "pwl_piece_dfdx: L >= 3 needs w_mid");
  DfdxParams p;
  p.off = a->off; p.anchor = a->anchor; p.T = a->T;
  p.w1 = a->w_first; p.b1 = a->b_first; p.Wm = a->w_mid; p.bm = a->b_mid; p.Wl = a->w_last;
  p.F = a->F; p.L = a->L; p.H = a->H; p.C = a->C; p.dfdx = a->dfdx;
  const size_t H = a->H, C = a->C, NM = a->L - 2;
  size_t lds = kDfdxWaves * 4 * H * sizeof(double) + (2 * H + NM * H * (H + 1) + NM * H) * sizeof(float);
  p.wl_in_lds = C * (H + 1) * sizeof(float) <= 32 * 1024;
  if (p.wl_in_lds) lds += C * (H + 1) * sizeof(float);
  const int64_t zero_work = (a->T * a->C + 64 * kDfdxWaves * 8 - 1) / (64 * kDfdxWaves * 8);
  p.n_zero_blocks = static_cast<int>(zero_work < 1 ? 1 : (zero_work > 64 ? 64 : zero_work));
  if (lds > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(pwl_dfdx_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       static_cast<int>(lds));
    if (e != hipSuccess) return gnan::fail(GNAN_ERR_HIP, "pwl_piece_dfdx: hipFuncSetAttribute: %s", hipGetErrorString(e));
  }
  hipLaunchKernelGGL(pwl_dfdx_kernel, dim3(a->F + p.n_zero_blocks), dim3(64 * kDfdxWaves), lds, static_cast<hipStream_t>(stream), p);
  return gnan::check_launch("pwl_dfdx_kernel");
}
