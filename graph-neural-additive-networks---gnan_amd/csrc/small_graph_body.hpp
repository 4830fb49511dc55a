// Pieces the one-launch graph routes share (csrc/small_graph.hip, csrc/small_graph_nam.hip, csrc/mid_graph.hip): the LDS image of
// one scalar MLP's weights, its evaluation on a block of 64 inputs by four waves, and — at the end — the host side of their entry
// points: the conversions of the C ABI's gnan_small_mlp, the ONE validator of sizes and MLP shapes (a route's limits are a
// RouteLimits next to its entry points), the pointer test, and the launch helpers.
#pragma once
#include <type_traits>

#include "common.hpp"
#include "fmlp_bwd_body.hpp"

namespace gnan_small {

using gnan::kWave;

struct Mlp {
  int L, H, C;
  const float *w_first, *b_first, *w_mid, *b_mid, *w_last, *b_last;
};

constexpr int kMaxH = 64, kMaxC = 8, kWaves = 4, kMaxNodes = 128;     // nodes: NB blocks of 64 (kernels are built for NB = 1 and 2)

// LDS image of one scalar MLP's weights (scalar loads straight from memory made every inner-loop step wait ~150 cycles for
// its weights: 33 us for a 30-node graph; read as LDS broadcasts the same loop is bound by LDS issue)
struct MlpLds {
  float* w1;   // [H]
  float* b1;   // [H]
  float* w2;   // [H, H]
  float* b2;   // [H]
  float* w3;   // [C, H]
  float* b3;   // [C]
};

__device__ __forceinline__ MlpLds carve(float* base) {
  MlpLds w;
  w.w2 = base;
  w.w1 = base + kMaxH * kMaxH;
  w.b1 = w.w1 + kMaxH;
  w.b2 = w.b1 + kMaxH;
  w.w3 = w.b2 + kMaxH;
  w.b3 = w.w3 + kMaxC * kMaxH;
  return w;
}
constexpr int kWeightFloats = kMaxH * kMaxH + 3 * kMaxH + kMaxC * kMaxH + kMaxC;

// (every load is issued before the first LDS store: a load -> store loop keeps ONE load in flight, and a cold load costs
// more than a microsecond — sixteen of them in a row were most of the kernel's time)
__device__ __forceinline__ void stage_weights(const Mlp& m, int k, const MlpLds& w) {
  const int H = m.H, C = m.C, tid = threadIdx.x;
  constexpr int kPer = kMaxH * kMaxH / (kWaves * kWave);           // 16 hidden-to-hidden weights per thread
  float v2[kPer], v3[2];
  const float* w2 = m.L == 3 ? m.w_mid + static_cast<int64_t>(k) * H * H : nullptr;
#pragma unroll
  for (int t = 0; t < kPer; ++t) {
    const int i = tid + t * (kWaves * kWave);
    v2[t] = (w2 && i < H * H) ? w2[i] : 0.f;
  }
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int i = tid + t * (kWaves * kWave);
    v3[t] = i < C * H ? m.w_last[static_cast<int64_t>(k) * C * H + i] : 0.f;
  }
  const bool hid = tid < H;
  const float a1 = hid ? m.w_first[k * H + tid] : 0.f;
  const float a2 = (hid && m.b_first) ? m.b_first[k * H + tid] : 0.f;
  const float a3 = (hid && m.L == 3 && m.b_mid) ? m.b_mid[k * H + tid] : 0.f;
  const float a4 = (tid < C && m.b_last) ? m.b_last[k * C + tid] : 0.f;
#pragma unroll
  for (int t = 0; t < kPer; ++t) {
    const int i = tid + t * (kWaves * kWave);
    if (i < H * H) w.w2[i] = v2[t];
  }
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int i = tid + t * (kWaves * kWave);
    if (i < C * H) w.w3[i] = v3[t];
  }
  if (hid) { w.w1[tid] = a1; w.b1[tid] = a2; w.b2[tid] = a3; }
  if (tid < C) w.b3[tid] = a4;
  __syncthreads();
}

// One scalar MLP on the 64 inputs of this node block: lane = input, the four waves split every hidden layer's units;
// activations live in LDS columns a / b ([H][64]).  Wave 0 ends with the C outputs of its lane in out[].
// DROP: training-mode Dropout behind every hidden ReLU (csrc/dropout.hpp) — `dbase` is the lane's drop_base(seed, node, feature),
// hidden layer 0 is the one written into column a, layer 1 the one written into nxt: the coordinates of gnan_fmlp_fwd,
// gnan_fmlp_bwd and gnan_dropout_mask.  The shape functions' workgroups only: rho carries no Dropout.
template <bool DROP = false>
__device__ __forceinline__ void mlp_block(const Mlp& m, const MlpLds& w, float xv, float* a, float* b, int lane, int wave,
                                          float (&out)[kMaxC], gnan_bwd::Drop drop = gnan_bwd::Drop{0u, 1.f, 0ull}, uint32_t dbase = 0u) {
  const int H = m.H, C = m.C;
  for (int j = wave; j < H; j += kWaves) {
    float h = fmaxf(fmaf(xv, w.w1[j], w.b1[j]), 0.f);
    if constexpr (DROP) h = gnan::drop_keep(dbase, 0, j, drop.thresh) ? h * drop.scale : 0.f;
    a[j * kWave + lane] = h;
  }
  __syncthreads();
  float* cur = a;
  float* nxt = b;
  if (m.L == 3) {                                    // the one hidden-to-hidden layer: rows of w2 = output units
    const int per = (H + kWaves - 1) / kWaves;       // a contiguous run of output units per wave, four at a time
    const int o_lo = wave * per, o_hi = o_lo + per < H ? o_lo + per : H;
    for (int o0 = o_lo; o0 < o_hi; o0 += 4) {
      float acc[4];
      const float* row[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int o = o0 + t < o_hi ? o0 + t : o_hi - 1;             // clamp: uniform, keeps the reads in range
        acc[t] = w.b2[o];
        row[t] = w.w2 + o * H;
      }
      if ((H & 3) == 0) {                              // four inputs per step: the weights as 16-byte LDS broadcasts
#pragma unroll 4
        for (int i = 0; i < H; i += 4) {
          float h[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) h[u] = cur[(i + u) * kWave + lane];
#pragma unroll
          for (int t = 0; t < 4; ++t) {
            const float4 w4 = *reinterpret_cast<const float4*>(row[t] + i);
            acc[t] = fmaf(w4.x, h[0], acc[t]);
            acc[t] = fmaf(w4.y, h[1], acc[t]);
            acc[t] = fmaf(w4.z, h[2], acc[t]);
            acc[t] = fmaf(w4.w, h[3], acc[t]);
          }
        }
      } else {
#pragma unroll 16
        for (int i = 0; i < H; ++i) {
          const float h = cur[i * kWave + lane];
#pragma unroll
          for (int t = 0; t < 4; ++t) acc[t] = fmaf(row[t][i], h, acc[t]);
        }
      }
#pragma unroll
      for (int t = 0; t < 4; ++t)
        if (o0 + t < o_hi) {
          float h = fmaxf(acc[t], 0.f);
          if constexpr (DROP) h = gnan::drop_keep(dbase, 1, o0 + t, drop.thresh) ? h * drop.scale : 0.f;
          nxt[(o0 + t) * kWave + lane] = h;
        }
    }
    __syncthreads();
    float* t = cur; cur = nxt; nxt = t;
  }
  if (wave == 0) {
    for (int c = 0; c < C; ++c) {
      float acc = w.b3[c];
#pragma unroll 16
      for (int i = 0; i < H; ++i) acc = fmaf(w.w3[c * H + i], cur[i * kWave + lane], acc);
      out[c] = acc;
    }
  }
  __syncthreads();                                   // the columns are free for the next node block
}

// Pre-rho backward (small_graph.hip, mid_graph.hip): rho's arguments are split by rows over workgroups, each of which leaves its
// share of rho's gradients in a slot of the workspace — W2's 64 x 64 (H x H, compact), then five vectors of 64: w_first, b_first,
// b_mid, w_last, b_last — and the last to arrive adds the slots in group order.
constexpr int kRhoSlot = kMaxH * kMaxH + 5 * kMaxH;

constexpr int small_cols_floats(int nb) {
  const int nodes = 64 * nb;
  const int tables = 2 * nodes * kMaxC + 256 * kMaxC + nodes * kWave + nodes * nodes / 4;
  return tables > 2 * kMaxH * kWave ? tables : 2 * kMaxH * kWave;
}

// Is this workgroup the last of `expected` to arrive at `counter`?  ONE thread releases the workgroup's results (the barrier before
// it orders the other threads' stores before its fence) and, in the last workgroup, acquires the others'.  An agent-scope fence
// is an L2 write-back / invalidate on this multi-die part: executed by every wave — 4 waves x 2 fences x the 512 workgroups of a
// 32-graph batch — they queued up behind each other for 50 of the launch's 68 us.
__device__ __forceinline__ bool last_to_arrive(unsigned* counter, unsigned expected, unsigned* s_slot) {
  __syncthreads();
  if (threadIdx.x == 0) {
    __threadfence();
    *s_slot = atomicAdd(counter, 1u);
  }
  __syncthreads();
  if (*s_slot != expected - 1) return false;
  if (threadIdx.x == 0) __threadfence();
  __syncthreads();
  return true;
}

inline gnan_bwd::Weights to_weights(const gnan_small_mlp* m, const gnan_small_mlp_grads* g) {
  gnan_bwd::Weights w;
  w.H = m->H;
  w.w_first = m->w_first; w.b_first = m->b_first; w.w_mid = m->L == 3 ? m->w_mid : nullptr; w.b_mid = m->L == 3 ? m->b_mid : nullptr;
  w.w_last = m->w_last; w.b_last = m->b_last;
  w.d_w_first = g->w_first; w.d_b_first = g->b_first; w.d_w_mid = g->w_mid; w.d_b_mid = g->b_mid; w.d_w_last = g->w_last;
  w.d_b_last = g->b_last;
  return w;
}

inline bool grads_ok(const gnan_small_mlp* m, const gnan_small_mlp_grads* g) {
  return g->w_first && g->w_last && (m->L == 2 || g->w_mid) && ((m->b_first == nullptr) == (g->b_first == nullptr)) &&
         (m->L == 2 || ((m->b_mid == nullptr) == (g->b_mid == nullptr))) && ((m->b_last == nullptr) == (g->b_last == nullptr));
}

inline Mlp to_mlp(const gnan_small_mlp* m) {
  Mlp r;
  r.L = m->L; r.H = m->H; r.C = m->C;
  r.w_first = m->w_first; r.b_first = m->b_first; r.w_mid = m->w_mid; r.b_mid = m->b_mid; r.w_last = m->w_last; r.b_last = m->b_last;
  return r;
}

// ---- host side of the entry points (csrc/small_graph.hip, csrc/small_graph_nam.hip, csrc/mid_graph.hip) ------------------------------

// A route's cover, as data next to its entry points: the most nodes, the most shells, the most output channels of f, and whether rho
// may have one channel per output channel of f besides the one channel every route takes.
struct RouteLimits {
  int max_nodes, max_shells, max_c;
  bool rho_per_channel;
};

// What every launching entry point refuses first: sizes and MLP shapes outside the route's cover — one refusal per violated limit,
// naming the limit and the value.  Shapes only: pointers are mlp_ptrs_ok's.  (f or rho may be NULL: a query about sizes alone.)
inline int shape_ok(const char* who, const RouteLimits& lim, int n, int F, int D, const gnan_small_mlp* f, const gnan_small_mlp* rho) {
  GNAN_REQUIRE(n >= 1 && F >= 1 && D >= 1, "%s: bad sizes n=%d F=%d D=%d", who, n, F, D);
  if (n > lim.max_nodes) return gnan::fail(GNAN_ERR_UNSUPPORTED, "%s: covers n <= %d nodes (got n=%d)", who, lim.max_nodes, n);
  if (D > lim.max_shells) return gnan::fail(GNAN_ERR_UNSUPPORTED, "%s: covers D <= %d shells (got D=%d)", who, lim.max_shells, D);
  if (f && (f->C < 1 || f->C > lim.max_c))
    return gnan::fail(GNAN_ERR_UNSUPPORTED, "%s: covers 1 <= C <= %d output channels (got C=%d)", who, lim.max_c, f->C);
  if (rho && rho->C != 1 && !(lim.rho_per_channel && f && rho->C == f->C))
    return gnan::fail(GNAN_ERR_UNSUPPORTED, "%s: covers a one-channel rho%s (got rho.C=%d)", who,
                      lim.rho_per_channel ? " or a channel per output channel" : "", rho->C);
  const gnan_small_mlp* m[2] = {f, rho};
  for (int t = 0; t < 2; ++t) {
    if (m[t] == nullptr) continue;
    if (m[t]->L != 2 && m[t]->L != 3)
      return gnan::fail(GNAN_ERR_UNSUPPORTED, "%s: covers L in {2, 3} (got L=%d for %s)", who, m[t]->L, t ? "rho" : "f");
    if (m[t]->H < 1 || m[t]->H > kMaxH)
      return gnan::fail(GNAN_ERR_UNSUPPORTED, "%s: covers 1 <= H <= %d (got H=%d for %s)", who, kMaxH, m[t]->H, t ? "rho" : "f");
  }
  return GNAN_OK;
}

// The Dropout record of the *_drop entry points, checked on the host before anything else of theirs: NULL, p outside [0, 1) (NaN
// included) and a non-zero reserved word are refused.  out->thresh == 0 (p == 0, or p below 2^-32): the plain kernels.
inline int drop_ok(const char* who, const gnan_small_dropout* d, gnan_bwd::Drop* out) {
  GNAN_REQUIRE(d != nullptr, "%s: null dropout record", who);
  GNAN_REQUIRE(d->p >= 0.f && d->p < 1.f, "%s: dropout p must be in [0, 1) (got p=%g)", who, static_cast<double>(d->p));
  GNAN_REQUIRE(d->reserved == 0, "%s: dropout reserved must be 0 (got reserved=%d)", who, d->reserved);
  out->thresh = gnan::drop_threshold(d->p);
  out->scale = out->thresh != 0u ? 1.f / (1.f - d->p) : 1.f;
  out->seed = d->seed;
  return GNAN_OK;
}

// ... and of the *_drop_dev entry points, whose seed lives in a device cell (gnan_dropout_seed_set writes it; a captured step reads
// a fresh one at every replay): the same refusals in the same order, then a NULL cell.  The kernels read *seed; out->seed stays 0.
inline int drop_dev_ok(const char* who, const gnan_small_dropout_dev* d, gnan_bwd::Drop* out, const uint64_t** seed) {
  GNAN_REQUIRE(d != nullptr, "%s: null dropout record", who);
  const gnan_small_dropout by_value = {d->p, d->reserved, 0ull};
  if (int rc = drop_ok(who, &by_value, out)) return rc;
  GNAN_REQUIRE(d->seed != nullptr, "%s: null dropout seed cell", who);
  *seed = d->seed;
  return GNAN_OK;
}

// THE pointer test of a stack whose shape was accepted (L == 1: the NAM read-out's Linear(1, C), only its last layer exists)
inline bool mlp_ptrs_ok(const gnan_small_mlp* m) { return m->w_last && (m->L == 1 || (m->w_first && (m->L == 2 || m->w_mid))); }

template <class A>
int strides_ok(const char* who, const A* a) {
  GNAN_REQUIRE(a->x_stride >= a->F, "%s: row stride x_stride=%lld smaller than F=%d", who, static_cast<long long>(a->x_stride), a->F);
  GNAN_REQUIRE(a->cnt == nullptr || a->cnt_stride >= a->D, "%s: row stride cnt_stride=%lld smaller than D=%d", who,
               static_cast<long long>(a->cnt_stride), a->D);
  return GNAN_OK;
}

template <class A>
int workspace_ok(const char* who, const A* a, size_t need) {
  if (a->workspace == nullptr || a->workspace_bytes < need)
    return gnan::fail(GNAN_ERR_WORKSPACE, "%s: workspace %zu B < required %zu B", who, a->workspace_bytes, need);
  return GNAN_OK;
}

// fn(std::integral_constant<int, C>) for the kernels' output-channel counts 1 .. 8 (the validator refused everything else)
template <class Fn>
int with_channels(int C, Fn&& fn) {
  switch (C) {
    case 1: return fn(std::integral_constant<int, 1>{});
    case 2: return fn(std::integral_constant<int, 2>{});
    case 3: return fn(std::integral_constant<int, 3>{});
    case 4: return fn(std::integral_constant<int, 4>{});
    case 5: return fn(std::integral_constant<int, 5>{});
    case 6: return fn(std::integral_constant<int, 6>{});
    case 7: return fn(std::integral_constant<int, 7>{});
    default: return fn(std::integral_constant<int, 8>{});
  }
}

// Raise a kernel's dynamic-LDS limit: once per kernel instance, at its first use (the eager warm-up of a step that is captured
// later — never inside a capture); the first result is remembered and a failure is reported on every call.
template <auto Kernel>
int raise_dyn_lds(size_t bytes, const char* who) {
  static const hipError_t attr =
      hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(bytes));
  if (attr != hipSuccess) return gnan::fail(GNAN_ERR_HIP, "%s: hipFuncSetAttribute: %s", who, hipGetErrorString(attr));
  return GNAN_OK;
}

// The fields the ABI structs of every route share, into a kernel's parameter record: the forward's (weights only) ...
template <class P, class A>
void graph_fields(P& p, const A* a, int n) {
  p.x = a->x; p.x_stride = a->x_stride; p.n = n; p.F = a->F;
  p.code = a->code; p.D = a->D; p.cnt = a->cnt; p.cnt_stride = a->cnt_stride;
}
template <class P, class A>
void fwd_fields(P& p, const A* a, int n) {
  graph_fields(p, a, n);
  p.f = to_mlp(&a->f); p.r = to_mlp(&a->rho);
}
// ... and the backward's (weights and where their gradients go)
template <class P, class A>
void bwd_fields(P& p, const A* a, int n, const gnan_small_mlp_grads* df, const gnan_small_mlp_grads* drho) {
  graph_fields(p, a, n);
  p.f = to_weights(&a->f, df); p.r = to_weights(&a->rho, drho);
  p.f_mid = a->f.L == 3; p.r_mid = a->rho.L == 3;
}

// a one-graph workspace: the first 16 bytes the arrival counter, the rest the partials
template <class T>
void split_workspace(void* workspace, unsigned*& counter, T*& part) {
  counter = static_cast<unsigned*>(workspace);
  part = reinterpret_cast<T*>(static_cast<char*>(workspace) + 16);
}

}  // namespace gnan_small
