// Parameter gradients of the three-layer shape functions on the matrix cores (gfx950): gnan_fmlp_bwd's result for batches
// past its reach (one wave per node there), with the forward's training-mode Dropout (csrc/dropout.hpp) recomputed from
// (p, seed) — nothing of size [n, F, H] is ever written.
//
//   f_k(x) = W3 d2(relu(W2 d1(relu(w1 x + b1)) + b2)) + b3          L == 3, H <= 64, C <= 8; d1, d2: keep * 1 / (1 - p)
//   given g[n, c] = dLoss / d f_k(x[n, k])[c]:   d{w1, b1, W2, b2, W3, b3} of every feature k, summed over the nodes.
//
// Grid (feature, node split) as gnan_fmlp_bwd; a workgroup has 4 waves and each wave walks 32-node tiles of its split.  The
// layouts are fmlp_mfma_kernel's (csrc/fmlp.hip): v_mfma_f32_32x32x2_f32 computes D[unit, node] = A[unit, k] B[k, node], the
// lane is the node, and an accumulator (unit 32 t + drow(r, half) in register r) is the next product's B operand once the K
// order of the packed A fragments is permuted by kperm.  Per tile:
//   h1 straight into the B operand; z2 = W2 h1 + b2 from the packed W2 in LDS; h2 = d2(relu(z2))
//   dh2 = W3^T g in the lane (C <= 8);  dz2 = dh2 [h2 > 0] / (1 - p)
//   dh1 = W2^T dz2 from the packed W2^T in LDS (B = dz2, already in accumulator order);  dz1 = dh1 [h1 > 0] / (1 - p)
//   dW2 += dz2 h1^T and dW3 += g h2^T contract over the NODE, which is the lane: the wave transposes its [unit][32 nodes]
//   tiles through a private LDS slab (written lane = node, read lane = unit) and runs them as MFMA with K = node; dW2 stays in
//   HT^2 x 16 accumulator registers over all tiles of the split, dW3 (g padded to one 32-row tile) in HT x 16.
//   dw1, db1, db2, db3 are lane sums, reduced over the lanes once at the end (fixed butterfly).
// The four waves' sums meet in LDS in wave order, the splits' in gnan::fmlp_split_reduce_kernel in split order: no atomics, the same
// bits on every run.  Rows past the split's end take x = 0 and g = 0: every product they enter is exactly 0.
#include "common.hpp"
#include "dropout.hpp"
#include "fmlp_split_reduce.hpp"

namespace {

using gnan::kWave;
using f32x16 = __attribute__((ext_vector_type(16))) float;

// accumulator row and K permutation of csrc/fmlp.hip (the packed fragments of both files follow them)
__host__ __device__ constexpr int drow(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }
__host__ __device__ constexpr int kperm(int s, int h) { return 32 * (s / 16) + drow(s % 16, h); }

constexpr int kST = 36;        // slab row stride in floats: 32 nodes + 4 (rows stay 16-byte aligned for the b128 reads)
constexpr int kCmax = 8;

struct Params {
  const float* x;
  int64_t n, x_stride;
  int F, H, C;
  const float *w_first, *b_first, *w_mid, *b_mid, *w_last;
  int sum_features;
  const float* grad;
  int64_t grad_stride;
  float *d_w_first, *d_b_first, *d_w_mid, *d_b_mid, *d_w_last, *d_b_last;
  int64_t nodes_per_split;   // blockIdx.y walks nodes [y * nodes_per_split, (y + 1) * nodes_per_split): a multiple of 128
  int64_t split_stride;      // floats between the gradient blocks of consecutive splits (0: one split, final outputs)
  uint32_t drop_thresh;
  float drop_scale;
  uint64_t drop_seed;
  const uint64_t* seed_dev;   // NULL (drop_seed came by value), or the device cell the seed is read from (the *_dev entry points); NULL whenever drop_thresh == 0
};

__host__ __device__ constexpr int slab_floats(int HP) { return 2 * HP * kST + kCmax * kST; }          // per wave
__host__ __device__ constexpr int red_floats(int HP) { return HP * HP + kCmax * HP + 3 * HP + kCmax; }  // per wave
__host__ __device__ constexpr int vec_floats(int HP) { return 2 * HP + HP + kCmax * HP; }              // {w1, b1} | b2 | W3
__host__ __device__ constexpr int lds_floats(int HP) { return 2 * HP * HP + vec_floats(HP) + 4 * slab_floats(HP); }

// lanes of one half (32 nodes) -> every lane of the half holds the sum; fixed order
__device__ __forceinline__ float half_sum(float v) {
#pragma unroll
  for (int off = 16; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

template <int HT, int CT, bool DROP>
__global__ __launch_bounds__(256) void fmlp_bwd_mfma_kernel(const Params p) {
  constexpr int HP = 32 * HT, KS = 16 * HT, KS4 = 4 * HT;
  constexpr int SLAB = slab_floats(HP), RED = red_floats(HP);
  static_assert(RED <= SLAB, "the waves' sums meet in the slabs");
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* w2p = smem;                         // A fragments of W2    (z2 = W2 h1)
  float* w2tp = w2p + HP * HP;               // A fragments of W2^T  (dh1 = W2^T dz2)
  float* vec = w2tp + HP * HP;               // {w1, b1}[kperm(s, h)] | b2 | W3[c][:]   (zero padded to HP)
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x / kWave;
  const int half = lane >> 5, nl = lane & 31;
  float* slab_a = vec + vec_floats(HP) + wave * SLAB;   // [HP][kST]: dz2
  float* slab_b = slab_a + HP * kST;                     // [HP][kST]: h2, then h1
  float* slab_g = slab_b + HP * kST;                     // [8][kST]:  g
  const int k = blockIdx.x;
  const int H = p.H, C = p.C;
  uint64_t seed = 0;
  if constexpr (DROP) seed = p.seed_dev ? *p.seed_dev : p.drop_seed;   // one wave-uniform load (gnan_fmlp_bwd_mfma_dev: the seed's device cell)

  // the feature's weights into LDS, in fmlp_pack_kernel's order
  {
    const float* W2 = p.w_mid + static_cast<int64_t>(k) * H * H;
    for (int idx = threadIdx.x; idx < HP * HP; idx += 256) {
      const int t_out = idx / (KS4 * 256);
      const int rem = idx % (KS4 * 256);
      const int s4 = rem / 256, ln = (rem % 256) / 4, e = rem % 4;
      const int row = 32 * t_out + (ln & 31);
      const int col = kperm(4 * s4 + e, ln >> 5);
      const bool in = row < H && col < H;
      w2p[idx] = in ? W2[row * H + col] : 0.f;
      w2tp[idx] = in ? W2[col * H + row] : 0.f;
    }
    for (int j = threadIdx.x; j < vec_floats(HP); j += 256) {
      float v = 0.f;
      if (j < 2 * HP) {
        const int hid = kperm(j / 4, (j / 2) % 2);
        if (hid < H) v = (j % 2) ? (p.b_first ? p.b_first[k * H + hid] : 0.f) : p.w_first[k * H + hid];
      } else if (j < 3 * HP) {
        const int hid = j - 2 * HP;
        if (hid < H && p.b_mid) v = p.b_mid[k * H + hid];
      } else {
        const int c = (j - 3 * HP) / HP, hid = (j - 3 * HP) % HP;
        if (c < C && hid < H) v = p.w_last[(static_cast<int64_t>(k) * C + c) * H + hid];
      }
      vec[j] = v;
    }
  }
  __syncthreads();
  const float* b2 = vec + 2 * HP;
  const float* w3 = vec + 3 * HP;

  f32x16 acc_w2[HT][HT];     // dW2[32 ta + drow(r, half)][32 tb + nl]
  f32x16 acc_w3[HT];         // dW3[drow(r, half)][32 tb + nl]  (rows >= C are zero)
  float s_w1[KS], s_b1[KS], s_b2[KS], s_b3[CT];   // lane sums, unit 32 t + drow(r, half) at [16 t + r]
#pragma unroll
  for (int ta = 0; ta < HT; ++ta) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      acc_w3[ta][r] = 0.f;
#pragma unroll
      for (int tb = 0; tb < HT; ++tb) acc_w2[ta][tb][r] = 0.f;
    }
  }
#pragma unroll
  for (int s = 0; s < KS; ++s) s_w1[s] = s_b1[s] = s_b2[s] = 0.f;
#pragma unroll
  for (int c = 0; c < CT; ++c) s_b3[c] = 0.f;

  const int64_t n_lo = static_cast<int64_t>(blockIdx.y) * p.nodes_per_split;
  const int64_t n_hi = n_lo + p.nodes_per_split < p.n ? n_lo + p.nodes_per_split : p.n;
  const int64_t goff = p.sum_features ? 0 : static_cast<int64_t>(k) * C;
  const float dscale = DROP ? p.drop_scale : 1.f;

  for (int64_t node0 = n_lo + 32 * wave; node0 < n_hi; node0 += 128) {
    const int64_t node = node0 + nl;
    const bool valid = node < n_hi;
    const float xv = valid ? p.x[node * p.x_stride + k] : 0.f;
    float g[CT];
#pragma unroll
    for (int c = 0; c < CT; ++c) g[c] = (valid && c < C) ? p.grad[node * p.grad_stride + goff + c] : 0.f;
    uint32_t dbase = 0u;
    if constexpr (DROP) dbase = gnan::drop_base(seed, node, k);

    // ---- forward: h1 into the B operand, z2 on the matrix cores, h2
    float h1[KS];
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      const float2 wb = *reinterpret_cast<const float2*>(vec + (s * 2 + half) * 2);
      h1[s] = fmaxf(fmaf(xv, wb.x, wb.y), 0.f);
      if constexpr (DROP) h1[s] = gnan::drop_keep(dbase, 0, kperm(s, 0) + 4 * half, p.drop_thresh) ? h1[s] * dscale : 0.f;
    }
    float h2[KS];
    {
      f32x16 acc[HT];
#pragma unroll
      for (int t = 0; t < HT; ++t) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float4 b4 = *reinterpret_cast<const float4*>(b2 + 32 * t + 8 * q + 4 * half);
          acc[t][4 * q + 0] = b4.x; acc[t][4 * q + 1] = b4.y; acc[t][4 * q + 2] = b4.z; acc[t][4 * q + 3] = b4.w;
        }
      }
#pragma unroll
      for (int s4 = 0; s4 < KS4; ++s4) {
#pragma unroll
        for (int t = 0; t < HT; ++t) {
          const float4 a4 = *reinterpret_cast<const float4*>(w2p + ((t * KS4 + s4) * 64 + lane) * 4);
          acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.x, h1[4 * s4 + 0], acc[t], 0, 0, 0);
          acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.y, h1[4 * s4 + 1], acc[t], 0, 0, 0);
          acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.z, h1[4 * s4 + 2], acc[t], 0, 0, 0);
          acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.w, h1[4 * s4 + 3], acc[t], 0, 0, 0);
        }
      }
#pragma unroll
      for (int t = 0; t < HT; ++t) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          h2[16 * t + r] = fmaxf(acc[t][r], 0.f);
          if constexpr (DROP)
            h2[16 * t + r] = gnan::drop_keep(dbase, 1, 32 * t + drow(r, 0) + 4 * half, p.drop_thresh) ? h2[16 * t + r] * dscale : 0.f;
        }
      }
    }

    // ---- dW3 += g h2^T with K = node: g and h2 through the slabs.  K step s contracts nodes s (lane half 0) and 16 + s
    // (half 1); a lane reads its unit's sixteen nodes as four b128.  The slabs are the wave's own: LDS keeps a wave's accesses
    // in order, the fences keep the compiler from moving them.
#pragma unroll
    for (int t = 0; t < HT; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) slab_b[(32 * t + drow(r, 0) + 4 * half) * kST + nl] = h2[16 * t + r];
    if (half == 0) {
#pragma unroll
      for (int c = 0; c < CT; ++c) slab_g[c * kST + nl] = g[c];
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float4 a4 = make_float4(0.f, 0.f, 0.f, 0.f);
      if (nl < CT) a4 = *reinterpret_cast<const float4*>(slab_g + nl * kST + 16 * half + 4 * q);
#pragma unroll
      for (int tb = 0; tb < HT; ++tb) {
        const float4 b4 = *reinterpret_cast<const float4*>(slab_b + (32 * tb + nl) * kST + 16 * half + 4 * q);
        acc_w3[tb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.x, b4.x, acc_w3[tb], 0, 0, 0);
        acc_w3[tb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.y, b4.y, acc_w3[tb], 0, 0, 0);
        acc_w3[tb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.z, b4.z, acc_w3[tb], 0, 0, 0);
        acc_w3[tb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.w, b4.w, acc_w3[tb], 0, 0, 0);
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();

    // ---- dz2 = (W3^T g) [h2 > 0] / (1 - p)   (h2 > 0 iff z2 > 0 and the unit was kept), in accumulator order
    float dz2[KS];
#pragma unroll
    for (int t = 0; t < HT; ++t) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        float d[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < CT; ++c) {
          const float4 w4 = *reinterpret_cast<const float4*>(w3 + c * HP + 32 * t + 8 * q + 4 * half);
          d[0] = fmaf(w4.x, g[c], d[0]); d[1] = fmaf(w4.y, g[c], d[1]);
          d[2] = fmaf(w4.z, g[c], d[2]); d[3] = fmaf(w4.w, g[c], d[3]);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int i = 16 * t + 4 * q + e;
          dz2[i] = h2[i] > 0.f ? d[e] * dscale : 0.f;
          s_b2[i] += dz2[i];
        }
      }
    }

    // ---- dW2 += dz2 h1^T with K = node
#pragma unroll
    for (int t = 0; t < HT; ++t) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = (32 * t + drow(r, 0) + 4 * half) * kST + nl;
        slab_a[row] = dz2[16 * t + r];
        slab_b[row] = h1[16 * t + r];
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float4 a4[HT], b4[HT];
#pragma unroll
      for (int t = 0; t < HT; ++t) {
        a4[t] = *reinterpret_cast<const float4*>(slab_a + (32 * t + nl) * kST + 16 * half + 4 * q);
        b4[t] = *reinterpret_cast<const float4*>(slab_b + (32 * t + nl) * kST + 16 * half + 4 * q);
      }
#pragma unroll
      for (int ta = 0; ta < HT; ++ta) {
#pragma unroll
        for (int tb = 0; tb < HT; ++tb) {
          acc_w2[ta][tb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[ta].x, b4[tb].x, acc_w2[ta][tb], 0, 0, 0);
          acc_w2[ta][tb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[ta].y, b4[tb].y, acc_w2[ta][tb], 0, 0, 0);
          acc_w2[ta][tb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[ta].z, b4[tb].z, acc_w2[ta][tb], 0, 0, 0);
          acc_w2[ta][tb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[ta].w, b4[tb].w, acc_w2[ta][tb], 0, 0, 0);
        }
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();

    // ---- dh1 = W2^T dz2 on the matrix cores; dz1 = dh1 [h1 > 0] / (1 - p); the first layer's sums
    {
      f32x16 acc[HT];
#pragma unroll
      for (int t = 0; t < HT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
#pragma unroll
      for (int s4 = 0; s4 < KS4; ++s4) {
#pragma unroll
        for (int t = 0; t < HT; ++t) {
          const float4 a4 = *reinterpret_cast<const float4*>(w2tp + ((t * KS4 + s4) * 64 + lane) * 4);
          acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.x, dz2[4 * s4 + 0], acc[t], 0, 0, 0);
          acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.y, dz2[4 * s4 + 1], acc[t], 0, 0, 0);
          acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.z, dz2[4 * s4 + 2], acc[t], 0, 0, 0);
          acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.w, dz2[4 * s4 + 3], acc[t], 0, 0, 0);
        }
      }
#pragma unroll
      for (int t = 0; t < HT; ++t) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float dz1 = h1[16 * t + r] > 0.f ? acc[t][r] * dscale : 0.f;
          s_b1[16 * t + r] += dz1;
          s_w1[16 * t + r] = fmaf(dz1, xv, s_w1[16 * t + r]);
        }
      }
    }
#pragma unroll
    for (int c = 0; c < CT; ++c) s_b3[c] += g[c];
  }

  // ---- the wave's sums into its slab (no other wave touches it), then the four waves in wave order
  float* red = slab_a;
  constexpr int o_w3 = HP * HP, o_w1 = o_w3 + kCmax * HP, o_b1 = o_w1 + HP, o_b2 = o_b1 + HP, o_b3 = o_b2 + HP;
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int ta = 0; ta < HT; ++ta) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = 32 * ta + drow(r, 0) + 4 * half;
#pragma unroll
      for (int tb = 0; tb < HT; ++tb) red[row * HP + 32 * tb + nl] = acc_w2[ta][tb][r];
      const float w1s = half_sum(s_w1[16 * ta + r]), b1s = half_sum(s_b1[16 * ta + r]), b2s = half_sum(s_b2[16 * ta + r]);
      if (nl == 0) {
        red[o_w1 + row] = w1s;
        red[o_b1 + row] = b1s;
        red[o_b2 + row] = b2s;
      }
    }
  }
#pragma unroll
  for (int tb = 0; tb < HT; ++tb)
#pragma unroll
    for (int r = 0; r < 4; ++r) red[o_w3 + (r + 4 * half) * HP + 32 * tb + nl] = acc_w3[tb][r];    // rows drow(r, half) < 8
#pragma unroll
  for (int c = 0; c < kCmax; ++c) {
    float b3s = 0.f;
    if (c < CT) b3s = half_sum(s_b3[c < CT ? c : 0]);
    if (lane == 0) red[o_b3 + c] = b3s;
  }
  __syncthreads();
  const float* all = vec + vec_floats(HP);
  const int64_t so = static_cast<int64_t>(blockIdx.y) * p.split_stride;     // this split's block of partial gradients
  for (int idx = threadIdx.x; idx < RED; idx += 256) {
    float a = all[idx];
#pragma unroll
    for (int w = 1; w < 4; ++w) a += all[w * SLAB + idx];
    if (idx < o_w3) {
      const int jo = idx / HP, ji = idx % HP;
      if (jo < H && ji < H) p.d_w_mid[so + (static_cast<int64_t>(k) * H + jo) * H + ji] = a;
    } else if (idx < o_w1) {
      const int c = (idx - o_w3) / HP, j = (idx - o_w3) % HP;
      if (c < C && j < H) p.d_w_last[so + (static_cast<int64_t>(k) * C + c) * H + j] = a;
    } else if (idx < o_b3) {
      const int which = (idx - o_w1) / HP, j = (idx - o_w1) % HP;
      float* dst = which == 0 ? p.d_w_first : (which == 1 ? p.d_b_first : p.d_b_mid);
      if (dst && j < H) dst[so + static_cast<int64_t>(k) * H + j] = a;
    } else {
      const int c = idx - o_b3;
      if (p.d_b_last && c < C) p.d_b_last[so + static_cast<int64_t>(k) * C + c] = a;
    }
  }
}

// the splits' blocks meet in split order: gnan::fmlp_split_reduce_kernel (csrc/fmlp_split_reduce.hpp)
using ReduceOuts = gnan::SplitReduceOuts;

// Node ranges per feature: enough workgroups to fill the chip twice over (one workgroup per CU: the LDS), at least one
// 32-node tile per wave each.
int node_splits(int64_t n, int F) {
  int64_t want = (512 + F - 1) / F;
  const int64_t most = (n + 127) / 128;
  if (want > most) want = most;
  if (want > 1024) want = 1024;
  return want < 1 ? 1 : static_cast<int>(want);
}

int64_t block_floats(const gnan_fmlp_bwd_args* a) {       // one split's gradients: [w_first | b_first | w_mid | b_mid | w_last | b_last]
  const int64_t F = a->F, H = a->H, C = a->C;
  return 2 * F * H + F * H * H + F * H + F * C * H + F * C;
}

template <int HT, int CT>
int launch(const Params& p, unsigned splits, hipStream_t st) {
  constexpr size_t lds = static_cast<size_t>(lds_floats(32 * HT)) * sizeof(float);
  static_assert(lds <= 160 * 1024, "LDS of one workgroup");
  auto go = [&](auto kernel) {
    if (lds > 64 * 1024) {
      hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                         static_cast<int>(lds));
      if (e != hipSuccess) return gnan::fail(GNAN_ERR_HIP, "fmlp_bwd_mfma: hipFuncSetAttribute: %s", hipGetErrorString(e));
    }
    hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>(p.F), splits), dim3(256), lds, st, p);
    return gnan::check_launch("fmlp_bwd_mfma_kernel");
  };
  return p.drop_thresh != 0u ? go(fmlp_bwd_mfma_kernel<HT, CT, true>) : go(fmlp_bwd_mfma_kernel<HT, CT, false>);
}

template <int HT>
int launch_ct(const Params& p, unsigned splits, hipStream_t st) {
  if (p.C <= 1) return launch<HT, 1>(p, splits, st);
  if (p.C <= 2) return launch<HT, 2>(p, splits, st);
  if (p.C <= 4) return launch<HT, 4>(p, splits, st);
  return launch<HT, 8>(p, splits, st);
}

}  // namespace

// THE launcher of gnan_fmlp_bwd_mfma (seed_dev == NULL) and gnan_fmlp_bwd_mfma_dev (seed_dev: the seed's device cell, NULL for p == 0)
static int fmlp_bwd_mfma(const gnan_fmlp_bwd_args* a, const uint64_t* seed_dev, gnan_stream_t stream) {
  GNAN_REQUIRE(a != nullptr, "fmlp_bwd_mfma: null args");
  GNAN_REQUIRE(a->n >= 0 && a->F >= 1, "fmlp_bwd_mfma: bad sizes");
  if (a->L != 3 || a->H < 1 || a->H > 64 || a->C < 1 || a->C > kCmax)
    return gnan::fail(GNAN_ERR_UNSUPPORTED, "fmlp_bwd_mfma: covers L == 3, H <= 64, C <= %d (got L=%d H=%d C=%d)", kCmax, a->L, a->H,
                      a->C);
  GNAN_REQUIRE(a->w_first && a->w_last && a->d_w_first && a->d_w_last, "fmlp_bwd_mfma: null weight / gradient pointer");
  GNAN_REQUIRE(a->w_mid && a->d_w_mid, "fmlp_bwd_mfma: L == 3 needs w_mid and d_w_mid");
  GNAN_REQUIRE((a->b_first == nullptr) == (a->d_b_first == nullptr) && (a->b_mid == nullptr) == (a->d_b_mid == nullptr) &&
                   (a->b_last == nullptr) == (a->d_b_last == nullptr),
               "fmlp_bwd_mfma: a bias gradient is wanted exactly where there is a bias");
  const int64_t gw = a->sum_features ? a->C : static_cast<int64_t>(a->F) * a->C;
  GNAN_REQUIRE(a->n == 0 || (a->x && a->grad && a->x_stride >= a->F && a->grad_stride >= gw), "fmlp_bwd_mfma: bad x / grad");
  GNAN_REQUIRE(a->dropout_p >= 0.f && a->dropout_p < 1.f, "fmlp_bwd_mfma: dropout_p must be in [0, 1)");
  Params p;
  p.x = a->x; p.n = a->n; p.x_stride = a->x_stride; p.F = a->F; p.H = a->H; p.C = a->C;
  p.w_first = a->w_first; p.b_first = a->b_first; p.w_mid = a->w_mid; p.b_mid = a->b_mid; p.w_last = a->w_last;
  p.sum_features = a->sum_features; p.grad = a->grad; p.grad_stride = a->grad_stride;
  p.d_w_first = a->d_w_first; p.d_b_first = a->d_b_first; p.d_w_mid = a->d_w_mid; p.d_b_mid = a->d_b_mid;
  p.d_w_last = a->d_w_last; p.d_b_last = a->d_b_last;
  p.drop_thresh = a->dropout_p > 0.f ? gnan::drop_threshold(a->dropout_p) : 0u;
  p.drop_scale = a->dropout_p > 0.f ? 1.f / (1.f - a->dropout_p) : 1.f;
  p.drop_seed = a->dropout_seed;
  p.seed_dev = p.drop_thresh != 0u ? seed_dev : nullptr;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int splits = a->n > 0 ? node_splits(a->n, a->F) : 1;
  const int64_t blk = block_floats(a);
  const int64_t F = a->F, H = a->H, C = a->C;
  const int64_t off_b1 = F * H, off_w2 = 2 * F * H, off_b2 = off_w2 + F * H * H, off_w3 = off_b2 + F * H, off_b3 = off_w3 + F * C * H;
  p.nodes_per_split = (a->n + 127) / 128 * 128;
  if (p.nodes_per_split == 0) p.nodes_per_split = 128;
  p.split_stride = 0;
  if (splits > 1) {
    const size_t need = static_cast<size_t>(splits) * blk * sizeof(float);
    if (a->workspace == nullptr || a->workspace_bytes < need)
      return gnan::fail(GNAN_ERR_WORKSPACE, "fmlp_bwd_mfma: workspace %zu B < required %zu B", a->workspace_bytes, need);
    float* ws = static_cast<float*>(a->workspace);
    p.nodes_per_split = ((a->n + splits - 1) / splits + 127) / 128 * 128;
    p.split_stride = blk;
    p.d_w_first = ws;
    p.d_b_first = a->d_b_first ? ws + off_b1 : nullptr;
    p.d_w_mid = ws + off_w2;
    p.d_b_mid = a->d_b_mid ? ws + off_b2 : nullptr;
    p.d_w_last = ws + off_w3;
    p.d_b_last = a->d_b_last ? ws + off_b3 : nullptr;
  }
  const unsigned sp = static_cast<unsigned>(splits);
  const int rc = a->H <= 32 ? launch_ct<1>(p, sp, st) : launch_ct<2>(p, sp, st);
  if (rc || splits == 1) return rc;
  ReduceOuts r;
  r.out[0] = a->d_w_first; r.out[1] = a->d_b_first; r.out[2] = a->d_w_mid; r.out[3] = a->d_b_mid; r.out[4] = a->d_w_last;
  r.out[5] = a->d_b_last;
  r.off[0] = 0; r.off[1] = off_b1; r.off[2] = off_w2; r.off[3] = off_b2; r.off[4] = off_w3; r.off[5] = off_b3;
  r.end = blk;
  hipLaunchKernelGGL(gnan::fmlp_split_reduce_kernel, dim3(static_cast<unsigned>((blk + 255) / 256)), dim3(256), 0, st,
                     static_cast<const float*>(a->workspace), blk, splits, r);
  return gnan::check_launch("fmlp_split_reduce_kernel");
}

extern "C" int gnan_fmlp_bwd_mfma(const gnan_fmlp_bwd_args* a, gnan_stream_t stream) { return fmlp_bwd_mfma(a, nullptr, stream); }

extern "C" int gnan_fmlp_bwd_mfma_dev(const gnan_fmlp_bwd_args* a, const uint64_t* seed_cell, gnan_stream_t stream) {
  const uint64_t* seed_dev = nullptr;
  if (int rc = gnan::seed_cell_ok("fmlp_bwd_mfma_dev", a, seed_cell, &seed_dev)) return rc;
  return fmlp_bwd_mfma(a, seed_dev, stream);
}

extern "C" size_t gnan_fmlp_bwd_mfma_workspace_bytes(const gnan_fmlp_bwd_args* a) {
  if (!a || a->n <= 0 || a->F < 1 || a->L != 3 || a->H < 1 || a->C < 1) return 0;
  const int splits = node_splits(a->n, a->F);
  return splits > 1 ? static_cast<size_t>(splits) * block_floats(a) * sizeof(float) : 0;
}
