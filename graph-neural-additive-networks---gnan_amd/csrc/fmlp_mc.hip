// The shape functions with MANY output channels (9 <= C <= 64: the 40-class arxiv model of the reference's run.sh) on the
// matrix cores (gfx950), forward and parameter-gradient backward, with the training-mode Dropout of csrc/dropout.hpp.
//
// fmlp_mfma_kernel (csrc/fmlp.hip) and fmlp_bwd_mfma_kernel (csrc/fmlp_bwd_mfma.hip) treat the last layer as C <= 8 dot products
// in the lane; with up to 64 channels that is H C lane FMAs per node and up to 64 registers of g.  Here the last layer is a third
// matrix product (v_mfma_f32_32x32x2_f32 like the hidden layers; drow / kperm as in those two files), over channel tiles of 32
// rows: CT32 = ceil(C / 32) in {1, 2}, padded with zeros.
//
// Forward, fmlp_mc_fwd_kernel (3 <= L <= 4, H <= 64, 1 <= C <= 64): fmlp_mfma_kernel up to the last hidden layer, whose
// activations are the B operand in accumulator order already; out[c, node] = W3[c, :] h[:, node] with W3 packed as A fragments the
// way a mid layer is (rows = channels, kperm order in K).  With sum_features the CT32 x 16 accumulators carry over the features of
// the chunk and b_last is summed once (thread c sums channel c's bias over the chunk, handed out through LDS at the end).
// Stores: an accumulator register quad 4 q .. 4 q + 3 of lane half h is the four CONSECUTIVE channels 32 t + 8 q + 4 h .. + 3 of
// the lane's node, so a lane stores 16 bytes per quad (global_store_dwordx4, the two halves side by side: 32 contiguous bytes per
// row and instruction) where C, the row stride and the base allow, and dwords otherwise.  No LDS transpose: the kernel has no
// LDS to spare next to two double-buffered weight images, and a barrier per feature would sit in the MFMA stream.
//
// Backward, fmlp_mc_bwd_kernel (L == 3, H <= 64, 1 <= C <= 64; parameter gradients): fmlp_bwd_mfma_kernel with
//   g in LDS only (the wave's slab [32 CT32][kST], channel-major; rows >= C and nodes past the end are zeros);
//   dh2 = W3^T g an MFMA with K = channel: W3^T packed as A fragments in LDS, B read from the g slab a K step at a time;
//   dW3 += g h2^T in CT32 x HT tiles of 16 accumulators; d_b_last from the A fragments of that product (a lane holds channel
//   nl's sixteen nodes of its half: summed in the lane, halves added at the end — fixed order, no atomics);
//   of h2 and h1 only the sign bits (one register each) are kept once the values are in the slabs.
// The four waves' sums meet in LDS in wave order — over the weight images, which nobody reads any more — and the splits' in
// gnan::fmlp_split_reduce_kernel in split order.
#include "common.hpp"
#include "dropout.hpp"
#include "fmlp_split_reduce.hpp"

namespace {

using gnan::kWave;
using f32x16 = __attribute__((ext_vector_type(16))) float;

// accumulator row and K permutation of csrc/fmlp.hip (the packed fragments of all three files follow them)
__host__ __device__ constexpr int drow(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }
__host__ __device__ constexpr int kperm(int s, int h) { return 32 * (s / 16) + drow(s % 16, h); }

constexpr int kCmax = 64;          // forward cover
constexpr int kCmaxBwd = 64;       // backward cover
constexpr size_t kLdsMax = 163840; // LDS of one workgroup

// =============================================================================================
// forward
// =============================================================================================
struct FwdParams {
  const float* x;
  int64_t n, x_stride;
  int F, L, H, C;
  const float *w_first, *b_first, *w_mid, *b_mid, *w_last, *b_last;
  int sum_features;
  float* out;
  int64_t out_stride;
  int feat_chunk;        // features per gridDim.y chunk (even)
  float* sum_partial;    // [chunks, n, C] or nullptr (single chunk)
  uint32_t drop_thresh;
  float drop_scale;
  uint64_t drop_seed;
  const uint64_t* seed_dev;   // NULL (drop_seed came by value), or the device cell the seed is read from (the *_dev entry points); NULL whenever drop_thresh == 0
};

// floats per feature in the packed stream: mid layers | W3 | {w1, b1} | b_mid | b_last, padded to whole 1-KiB pieces per wave
__host__ __device__ constexpr int fwd_feature_floats(int HT, int NMID, int CT32) {
  return (NMID * 32 * HT * 32 * HT + 32 * CT32 * 32 * HT + 64 * HT + NMID * 32 * HT + 32 * CT32 + 1023) & ~1023;
}

template <int NCH>
__device__ __forceinline__ void stage_feature(const float* __restrict__ src, float* lds_dst, int lane, int wave) {
  static_assert(NCH % 4 == 0, "pieces are dealt evenly to the 4 waves");
#pragma unroll
  for (int c = 0; c < NCH / 4; ++c) {
    const int ch = c * 4 + wave;  // wave-uniform
    __builtin_amdgcn_global_load_lds(src + (ch * 64 + lane) * 4,
                                     (__attribute__((address_space(3))) void*)(lds_dst + ch * 256), 16, 0, 0);
  }
}

//   mid[m][t_out][s / 4][lane][s % 4] = W_m[32 t_out + (lane & 31)][kperm(s, lane >> 5)]       (as fmlp_pack_kernel)
//   w3[t_c][s / 4][lane][s % 4]       = W3[32 t_c + (lane & 31)][kperm(s, lane >> 5)]           (rows = channels)
//   vec = { {w1, b1}[kperm(s, h)] for s, h } | b_mid[m][:] | b_last[:]                          (zero padded)
__global__ __launch_bounds__(256) void fmlp_mc_pack_kernel(const FwdParams p, float* __restrict__ packed, int HT, int NMID, int CT32) {
  const int k = blockIdx.x;
  const int H = p.H, C = p.C, F = p.F;
  const int HP = 32 * HT, KS4 = 4 * HT;
  const int midf = NMID * HP * HP, w3f = 32 * CT32 * HP;
  const int fs = fwd_feature_floats(HT, NMID, CT32);
  float* out = packed + static_cast<int64_t>(k) * fs;
  for (int idx = threadIdx.x; idx < fs; idx += blockDim.x) {
    float v = 0.f;
    if (idx < midf + w3f) {
      const bool last = idx >= midf;
      int rem = last ? idx - midf : idx % (HP * HP);
      const int m = last ? 0 : idx / (HP * HP);
      const int t_out = rem / (KS4 * 256);
      rem %= KS4 * 256;
      const int s4 = rem / 256, lane = (rem % 256) / 4, e = rem % 4;
      const int row = 32 * t_out + (lane & 31);
      const int col = kperm(4 * s4 + e, lane >> 5);
      if (last) {
        if (row < C && col < H) v = p.w_last[(static_cast<int64_t>(k) * C + row) * H + col];
      } else if (row < H && col < H) {
        v = p.w_mid[((static_cast<int64_t>(m) * F + k) * H + row) * H + col];
      }
    } else {
      int j = idx - midf - w3f;
      if (j < 64 * HT) {
        const int hid = kperm(j / 4, (j / 2) % 2);
        if (hid < H) v = (j % 2) ? (p.b_first ? p.b_first[k * H + hid] : 0.f) : p.w_first[k * H + hid];
      } else if ((j -= 64 * HT) < NMID * HP) {
        const int m = j / HP, hid = j % HP;
        if (hid < H && p.b_mid) v = p.b_mid[(static_cast<int64_t>(m) * F + k) * H + hid];
      } else if ((j -= NMID * HP) < 32 * CT32) {
        if (j < C && p.b_last) v = p.b_last[k * C + j];
      }
    }
    out[idx] = v;
  }
}

// four consecutive channels c0 .. c0 + 3 of one row
__device__ __forceinline__ void store_quad(float* row, int c0, int C, bool vec_ok, float a, float b, float c, float d) {
  if (c0 >= C) return;
  if (vec_ok) {                                        // C % 4 == 0: the quad is whole
    *reinterpret_cast<float4*>(row + c0) = make_float4(a, b, c, d);
  } else {
    row[c0] = a;
    if (c0 + 1 < C) row[c0 + 1] = b;
    if (c0 + 2 < C) row[c0 + 2] = c;
    if (c0 + 3 < C) row[c0 + 3] = d;
  }
}

// DROP as in fmlp_mfma_kernel: the same coordinates, every DROP statement under `if constexpr`.  Two workgroups per CU (256
// registers) wherever two of the double-buffered weight images fit in LDS; where only one does, the registers of one.
template <int HT, int NMID, int CT32, bool SUM, int NT, bool DROP>
__global__ __launch_bounds__(256, 4 * sizeof(float) * fwd_feature_floats(HT, NMID, CT32) <= kLdsMax ? 2 : 1) void fmlp_mc_fwd_kernel(const FwdParams p, const float* __restrict__ packed) {
  constexpr int HP = 32 * HT, KS = 16 * HT, KS4 = 4 * HT, CP = 32 * CT32;
  constexpr int MIDF = NMID * HP * HP, W3F = CP * HP;
  constexpr int FS = fwd_feature_floats(HT, NMID, CT32);
  constexpr int NCH = FS / 256;  // wave-wide 1-KiB pieces per feature
  extern __shared__ __attribute__((aligned(16))) float smem[];  // 2 * FS floats
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x / kWave;
  const int half = lane >> 5, nl = lane & 31;
  const int C = p.C;
  uint64_t seed = 0;
  if constexpr (DROP) seed = p.seed_dev ? *p.seed_dev : p.drop_seed;   // one wave-uniform load (gnan_fmlp_mc_fwd_dev: the seed's device cell)
  const int64_t tile0 = (static_cast<int64_t>(blockIdx.x) * 4 + wave) * NT;
  int64_t node[NT];
  bool valid[NT];
  float xcur[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    node[nt] = (tile0 + nt) * 32 + nl;
    valid[nt] = node[nt] < p.n;
    xcur[nt] = valid[nt] ? p.x[node[nt] * p.x_stride + blockIdx.y * p.feat_chunk] : 0.f;
  }
  const int k_lo = blockIdx.y * p.feat_chunk;
  const int k_hi = k_lo + p.feat_chunk < p.F ? k_lo + p.feat_chunk : p.F;
  // where the rows go, and whether a lane may store 16 bytes at a time there
  float* dst = p.out;
  int64_t dst_stride = p.out_stride;
  if (SUM && p.sum_partial) {
    dst = p.sum_partial + static_cast<int64_t>(blockIdx.y) * p.n * C;
    dst_stride = C;
  }
  const bool vec_ok = (C & 3) == 0 && (dst_stride & 3) == 0 && (reinterpret_cast<uintptr_t>(dst) & 15) == 0;
  stage_feature<NCH>(packed + static_cast<int64_t>(k_lo) * FS, smem, lane, wave);
  __syncthreads();

  f32x16 osum[SUM ? NT : 1][CT32];     // SUM: out[32 t + drow(r, half)][node] over the chunk's features
  float bsum = 0.f;                    // SUM: thread c < CP sums b_last[c] over the chunk's features
#pragma unroll
  for (int nt = 0; nt < (SUM ? NT : 1); ++nt)
#pragma unroll
    for (int t = 0; t < CT32; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) osum[nt][t][r] = 0.f;

  auto feature_step = [&](const int k, const float* __restrict__ buf, float* __restrict__ nbuf) {
    const float* w3 = buf + MIDF;
    const float* vec = w3 + W3F;
    const float* bl = vec + 64 * HT + NMID * HP;
    const int kn = k + 1 < k_hi ? k + 1 : k;
    float xnext[NT];
    stage_feature<NCH>(packed + static_cast<int64_t>(kn) * FS, nbuf, lane, wave);
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) xnext[nt] = valid[nt] ? p.x[node[nt] * p.x_stride + kn] : 0.f;

#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      float B[KS];
      const float xv = xcur[nt];
      uint32_t dbase = 0u;
      if constexpr (DROP) dbase = gnan::drop_base(seed, node[nt], k);
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        const float2 wb = *reinterpret_cast<const float2*>(vec + (s * 2 + half) * 2);
        B[s] = fmaxf(fmaf(xv, wb.x, wb.y), 0.f);
        if constexpr (DROP) B[s] = gnan::drop_keep(dbase, 0, kperm(s, 0) + 4 * half, p.drop_thresh) ? B[s] * p.drop_scale : 0.f;
      }
#pragma unroll
      for (int m = 0; m < NMID; ++m) {
        f32x16 acc[HT];
        const float* bm = vec + 64 * HT + m * HP;
#pragma unroll
        for (int t = 0; t < HT; ++t) {
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const float4 b4 = *reinterpret_cast<const float4*>(bm + 32 * t + 8 * q + 4 * half);
            acc[t][4 * q + 0] = b4.x; acc[t][4 * q + 1] = b4.y; acc[t][4 * q + 2] = b4.z; acc[t][4 * q + 3] = b4.w;
          }
        }
        const float* wm = buf + m * HP * HP;
#pragma unroll
        for (int s4 = 0; s4 < KS4; ++s4) {
#pragma unroll
          for (int t = 0; t < HT; ++t) {
            const float4 a4 = *reinterpret_cast<const float4*>(wm + ((t * KS4 + s4) * 64 + lane) * 4);
            acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.x, B[4 * s4 + 0], acc[t], 0, 0, 0);
            acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.y, B[4 * s4 + 1], acc[t], 0, 0, 0);
            acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.z, B[4 * s4 + 2], acc[t], 0, 0, 0);
            acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.w, B[4 * s4 + 3], acc[t], 0, 0, 0);
          }
        }
#pragma unroll
        for (int t = 0; t < HT; ++t)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            B[16 * t + r] = fmaxf(acc[t][r], 0.f);
            if constexpr (DROP)
              B[16 * t + r] = gnan::drop_keep(dbase, m + 1, 32 * t + drow(r, 0) + 4 * half, p.drop_thresh) ? B[16 * t + r] * p.drop_scale : 0.f;
          }
      }
      // last layer on the matrix cores: out[channel, node] += W3[channel, :] h[:, node]
      f32x16(&o)[CT32] = osum[SUM ? nt : 0];
      if constexpr (!SUM) {
#pragma unroll
        for (int t = 0; t < CT32; ++t)
#pragma unroll
          for (int r = 0; r < 16; ++r) o[t][r] = 0.f;
      }
#pragma unroll
      for (int s4 = 0; s4 < KS4; ++s4) {
#pragma unroll
        for (int t = 0; t < CT32; ++t) {
          const float4 a4 = *reinterpret_cast<const float4*>(w3 + ((t * KS4 + s4) * 64 + lane) * 4);
          o[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.x, B[4 * s4 + 0], o[t], 0, 0, 0);
          o[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.y, B[4 * s4 + 1], o[t], 0, 0, 0);
          o[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.z, B[4 * s4 + 2], o[t], 0, 0, 0);
          o[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.w, B[4 * s4 + 3], o[t], 0, 0, 0);
        }
      }
      if constexpr (!SUM) {
        if (valid[nt]) {
          float* row = dst + node[nt] * dst_stride + static_cast<int64_t>(k) * C;
#pragma unroll
          for (int t = 0; t < CT32; ++t) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              const int c0 = 32 * t + 8 * q + 4 * half;
              const float4 b4 = *reinterpret_cast<const float4*>(bl + c0);
              store_quad(row, c0, C, vec_ok, o[t][4 * q + 0] + b4.x, o[t][4 * q + 1] + b4.y, o[t][4 * q + 2] + b4.z,
                         o[t][4 * q + 3] + b4.w);
            }
          }
        }
      }
    }
    if constexpr (SUM) {
      if (threadIdx.x < CP) bsum += bl[threadIdx.x];
    }
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) xcur[nt] = xnext[nt];
    __syncthreads();  // drains the LDS-DMA (vmcnt(0)) and publishes the next feature's buffer
  };
  for (int k = k_lo; k < k_hi; k += 2) {
    feature_step(k, smem, smem + FS);
    if (k + 1 < k_hi) feature_step(k + 1, smem + FS, smem);
  }
  if constexpr (SUM) {
    if (threadIdx.x < CP) smem[threadIdx.x] = bsum;    // (the last step's barrier is behind every read and every LDS-DMA)
    __syncthreads();
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      if (valid[nt]) {
        float* row = dst + node[nt] * dst_stride;
#pragma unroll
        for (int t = 0; t < CT32; ++t) {
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int c0 = 32 * t + 8 * q + 4 * half;
            const float4 b4 = *reinterpret_cast<const float4*>(smem + c0);
            store_quad(row, c0, C, vec_ok, osum[nt][t][4 * q + 0] + b4.x, osum[nt][t][4 * q + 1] + b4.y,
                       osum[nt][t][4 * q + 2] + b4.z, osum[nt][t][4 * q + 3] + b4.w);
          }
        }
      }
    }
  }
}

// out[n, c] = sum over feature chunks of sum_partial[chunk, n, c], in chunk order (deterministic).
__global__ __launch_bounds__(256) void fmlp_mc_chunk_sum_kernel(const FwdParams p, int chunks) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= p.n * p.C) return;
  float a = 0.f;
  for (int ch = 0; ch < chunks; ++ch) a += p.sum_partial[static_cast<int64_t>(ch) * p.n * p.C + i];
  p.out[(i / p.C) * p.out_stride + i % p.C] = a;
}

// 32-node tiles per wave: two while the registers of two interleaved tiles fit under 256 (two workgroups per CU), one for H > 32
constexpr int tiles_per_wave(int HT) { return HT == 1 ? 2 : 1; }

bool fwd_cover(const gnan_fmlp_args* a) { return a->L >= 3 && a->L <= 4 && a->H >= 1 && a->H <= 64 && a->C >= 1 && a->C <= kCmax; }

// Feature chunks (gridDim.y) as csrc/fmlp.hip: enough workgroups for ~4 per CU when the node axis alone is too short.
int feature_chunks(int64_t n, int F, int H) {
  const int64_t per_block = 4 * tiles_per_wave(H <= 32 ? 1 : 2) * 32;
  const int64_t node_blocks = (n + per_block - 1) / per_block;
  int64_t chunks = (1024 + node_blocks - 1) / node_blocks;
  const int64_t max_chunks = (F + 1) / 2;          // at least two features per chunk (double-buffered pairs)
  chunks = chunks < 1 ? 1 : (chunks > max_chunks ? max_chunks : chunks);
  return static_cast<int>(chunks);
}

size_t fwd_packed_bytes(const gnan_fmlp_args* a) {
  return static_cast<size_t>(a->F) * fwd_feature_floats(a->H <= 32 ? 1 : 2, a->L - 2, a->C <= 32 ? 1 : 2) * sizeof(float);
}

template <int HT, int NMID, int CT32>
int launch_fwd(const FwdParams& p, const float* packed, hipStream_t st) {
  constexpr size_t lds = 2 * static_cast<size_t>(fwd_feature_floats(HT, NMID, CT32)) * sizeof(float);
  static_assert(lds <= kLdsMax, "LDS of one workgroup");
  constexpr int kNT = tiles_per_wave(HT);
  const int64_t nodes_per_block = 4 * kNT * 32;
  const int64_t blocks = (p.n + nodes_per_block - 1) / nodes_per_block;
  if (blocks > 0x7fffffffLL) return gnan::fail(GNAN_ERR_UNSUPPORTED, "fmlp_mc_fwd: too many nodes for one launch");
  const int chunks = (p.F + p.feat_chunk - 1) / p.feat_chunk;
  auto go = [&](auto kernel) {
    if (lds > 64 * 1024) {
      hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                         static_cast<int>(lds));
      if (e != hipSuccess) return gnan::fail(GNAN_ERR_HIP, "fmlp_mc_fwd: hipFuncSetAttribute: %s", hipGetErrorString(e));
    }
    hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>(blocks), static_cast<unsigned>(chunks)), dim3(256), lds, st, p, packed);
    return gnan::check_launch("fmlp_mc_fwd_kernel");
  };
  const bool drop = p.drop_thresh != 0u;              // p == 0: the plain instance, which never hashes
  if (!p.sum_features)
    return drop ? go(fmlp_mc_fwd_kernel<HT, NMID, CT32, false, kNT, true>) : go(fmlp_mc_fwd_kernel<HT, NMID, CT32, false, kNT, false>);
  if (int rc = drop ? go(fmlp_mc_fwd_kernel<HT, NMID, CT32, true, kNT, true>) : go(fmlp_mc_fwd_kernel<HT, NMID, CT32, true, kNT, false>))
    return rc;
  if (p.sum_partial) {
    const int64_t total = p.n * p.C;
    hipLaunchKernelGGL(fmlp_mc_chunk_sum_kernel, dim3(static_cast<unsigned>((total + 255) / 256)), dim3(256), 0, st, p, chunks);
    return gnan::check_launch("fmlp_mc_chunk_sum_kernel");
  }
  return GNAN_OK;
}

template <int HT, int NMID>
int launch_fwd_ct(const FwdParams& p, const float* packed, hipStream_t st) {
  return p.C <= 32 ? launch_fwd<HT, NMID, 1>(p, packed, st) : launch_fwd<HT, NMID, 2>(p, packed, st);
}

// =============================================================================================
// backward
// =============================================================================================
constexpr int kST = 36;        // slab row stride in floats: 32 nodes + 4 (rows stay 16-byte aligned for the b128 reads)

struct BwdParams {
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

__host__ __device__ constexpr int slab_floats(int HP, int CP) { return (2 * HP + CP) * kST; }                  // per wave
__host__ __device__ constexpr int red_floats(int HP, int CP) { return HP * HP + CP * HP + 3 * HP + CP; }       // per wave
__host__ __device__ constexpr int bwd_lds_floats(int HP, int CP) {   // W2 | W2^T | W3^T | {w1, b1}, b2 | four slabs
  return 2 * HP * HP + HP * CP + 3 * HP + 4 * slab_floats(HP, CP);
}
// Channel tiles of the instance that runs (H, C): ceil(C / 32) — but with H > 32 and Dropout the one-tile instance does not fit
// the register file (the compiler's resource report: scratch), so those shapes run the two-tile instance on zero-padded channels.
int bwd_channel_tiles(int H, int C, bool drop) { return (C > 32 || (H > 32 && drop)) ? 2 : 1; }
size_t bwd_lds_bytes(int H, int C, bool drop) {
  return sizeof(float) * bwd_lds_floats(H <= 32 ? 32 : 64, 32 * bwd_channel_tiles(H, C, drop));
}

// lanes of one half (32 nodes) -> every lane of the half holds the sum; fixed order
__device__ __forceinline__ float half_sum(float v) {
#pragma unroll
  for (int off = 16; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

__device__ __forceinline__ void wave_lds_fence() {     // the slabs are the wave's own: LDS keeps a wave's accesses in order,
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // the fence keeps the compiler from moving them
  __builtin_amdgcn_wave_barrier();
}

template <int HT, int CT32, bool DROP>
__global__ __launch_bounds__(256) void fmlp_mc_bwd_kernel(const BwdParams p) {
  constexpr int HP = 32 * HT, KS = 16 * HT, KS4 = 4 * HT, CP = 32 * CT32, KC4 = 4 * CT32;
  constexpr int SLAB = slab_floats(HP, CP), RED = red_floats(HP, CP);
  static_assert(4 * RED <= bwd_lds_floats(HP, CP), "the waves' sums meet in the workgroup's LDS");
  static_assert(KS <= 32, "one sign bit per unit in a 32-bit register");
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* w2p = smem;                         // A fragments of W2    (z2 = W2 h1)
  float* w2tp = w2p + HP * HP;               // A fragments of W2^T  (dh1 = W2^T dz2)
  float* w3tp = w2tp + HP * HP;              // A fragments of W3^T  (dh2 = W3^T g), K = channel: step s is channels 2 s, 2 s + 1
  float* vec = w3tp + HP * CP;               // {w1, b1}[kperm(s, h)] | b2
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x / kWave;
  const int half = lane >> 5, nl = lane & 31;
  float* slab_a = vec + 3 * HP + wave * SLAB;           // [HP][kST]: dz2
  float* slab_b = slab_a + HP * kST;                     // [HP][kST]: h2, then h1
  float* slab_g = slab_b + HP * kST;                     // [CP][kST]: g, channel-major
  const int k = blockIdx.x;
  const int H = p.H, C = p.C;
  uint64_t seed = 0;
  if constexpr (DROP) seed = p.seed_dev ? *p.seed_dev : p.drop_seed;   // one wave-uniform load (gnan_fmlp_mc_bwd_dev: the seed's device cell)

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
    const float* W3 = p.w_last + static_cast<int64_t>(k) * C * H;
    for (int idx = threadIdx.x; idx < HP * CP; idx += 256) {
      const int t_out = idx / (KC4 * 256);
      const int rem = idx % (KC4 * 256);
      const int s4 = rem / 256, ln = (rem % 256) / 4, e = rem % 4;
      const int unit = 32 * t_out + (ln & 31);
      const int ch = 2 * (4 * s4 + e) + (ln >> 5);
      w3tp[idx] = (unit < H && ch < C) ? W3[ch * H + unit] : 0.f;
    }
    for (int j = threadIdx.x; j < 3 * HP; j += 256) {
      float v = 0.f;
      if (j < 2 * HP) {
        const int hid = kperm(j / 4, (j / 2) % 2);
        if (hid < H) v = (j % 2) ? (p.b_first ? p.b_first[k * H + hid] : 0.f) : p.w_first[k * H + hid];
      } else {
        const int hid = j - 2 * HP;
        if (hid < H && p.b_mid) v = p.b_mid[k * H + hid];
      }
      vec[j] = v;
    }
  }
  __syncthreads();
  const float* b2 = vec + 2 * HP;

  f32x16 acc_w2[HT][HT];       // dW2[32 ta + drow(r, half)][32 tb + nl]
  f32x16 acc_w3[CT32][HT];     // dW3[32 tc + drow(r, half)][32 tb + nl]  (rows >= C are zero)
  float s_w1[KS], s_b1[KS];             // lane sums, unit 32 t + drow(r, half) at [16 t + r]
  float s_b2[HT], s_b3[CT32];           // unit 32 t + nl / channel 32 tc + nl over the nodes 16 half .. 16 half + 15 of every tile
#pragma unroll
  for (int r = 0; r < 16; ++r) {
#pragma unroll
    for (int tb = 0; tb < HT; ++tb) {
#pragma unroll
      for (int ta = 0; ta < HT; ++ta) acc_w2[ta][tb][r] = 0.f;
#pragma unroll
      for (int tc = 0; tc < CT32; ++tc) acc_w3[tc][tb][r] = 0.f;
    }
  }
#pragma unroll
  for (int s = 0; s < KS; ++s) s_w1[s] = s_b1[s] = 0.f;
#pragma unroll
  for (int t = 0; t < HT; ++t) s_b2[t] = 0.f;
#pragma unroll
  for (int tc = 0; tc < CT32; ++tc) s_b3[tc] = 0.f;

  const int64_t n_lo = static_cast<int64_t>(blockIdx.y) * p.nodes_per_split;
  const int64_t n_hi = n_lo + p.nodes_per_split < p.n ? n_lo + p.nodes_per_split : p.n;
  const int64_t goff = p.sum_features ? 0 : static_cast<int64_t>(k) * C;
  const float dscale = DROP ? p.drop_scale : 1.f;

  for (int64_t node0 = n_lo + 32 * wave; node0 < n_hi; node0 += 128) {
    const int64_t node = node0 + nl;
    const bool valid = node < n_hi;
    const float xv = valid ? p.x[node * p.x_stride + k] : 0.f;
    // ---- g into the slab, channel-major: lane half h takes the channels 2 j + h of its node
    {
      const float* grow = p.grad + (valid ? node * p.grad_stride + goff : 0);
#pragma unroll
      for (int j = 0; j < CP / 2; ++j) {
        const int ch = 2 * j + half;
        slab_g[ch * kST + nl] = (valid && ch < C) ? grow[ch] : 0.f;
      }
    }
    uint32_t dbase = 0u;
    if constexpr (DROP) dbase = gnan::drop_base(seed, node, k);

    // ---- forward: h1 into the B operand, z2 on the matrix cores, h2 into the slab (its sign bits stay)
    float h1[KS];
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      const float2 wb = *reinterpret_cast<const float2*>(vec + (s * 2 + half) * 2);
      h1[s] = fmaxf(fmaf(xv, wb.x, wb.y), 0.f);
      if constexpr (DROP) h1[s] = gnan::drop_keep(dbase, 0, kperm(s, 0) + 4 * half, p.drop_thresh) ? h1[s] * dscale : 0.f;
    }
    uint32_t pos2 = 0u;       // bit 16 t + r: h2 of unit 32 t + drow(r, half) is positive (z2 > 0 and the unit was kept)
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
          float h2 = fmaxf(acc[t][r], 0.f);
          if constexpr (DROP) h2 = gnan::drop_keep(dbase, 1, 32 * t + drow(r, 0) + 4 * half, p.drop_thresh) ? h2 * dscale : 0.f;
          slab_b[(32 * t + drow(r, 0) + 4 * half) * kST + nl] = h2;
          pos2 |= (h2 > 0.f ? 1u : 0u) << (16 * t + r);
        }
      }
    }
    wave_lds_fence();

    // ---- dW3 += g h2^T with K = node.  K step s contracts nodes s (lane half 0) and 16 + s (half 1); a lane reads its
    // channel's and its unit's sixteen nodes as four b128.  The g fragments also give d_b_last.
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float4 a4[CT32];
#pragma unroll
      for (int tc = 0; tc < CT32; ++tc) {
        a4[tc] = *reinterpret_cast<const float4*>(slab_g + (32 * tc + nl) * kST + 16 * half + 4 * q);
        s_b3[tc] += (a4[tc].x + a4[tc].y) + (a4[tc].z + a4[tc].w);
      }
#pragma unroll
      for (int tb = 0; tb < HT; ++tb) {
        const float4 b4 = *reinterpret_cast<const float4*>(slab_b + (32 * tb + nl) * kST + 16 * half + 4 * q);
#pragma unroll
        for (int tc = 0; tc < CT32; ++tc) {
          acc_w3[tc][tb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[tc].x, b4.x, acc_w3[tc][tb], 0, 0, 0);
          acc_w3[tc][tb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[tc].y, b4.y, acc_w3[tc][tb], 0, 0, 0);
          acc_w3[tc][tb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[tc].z, b4.z, acc_w3[tc][tb], 0, 0, 0);
          acc_w3[tc][tb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[tc].w, b4.w, acc_w3[tc][tb], 0, 0, 0);
        }
      }
    }

    // ---- dz2 = (W3^T g) [h2 > 0] / (1 - p): an MFMA with K = channel, B from the g slab, the result in accumulator order
    float dz2[KS];
    {
      f32x16 acc[HT];
#pragma unroll
      for (int t = 0; t < HT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
#pragma unroll
      for (int s4 = 0; s4 < KC4; ++s4) {
        float b[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) b[e] = slab_g[(2 * (4 * s4 + e) + half) * kST + nl];
#pragma unroll
        for (int t = 0; t < HT; ++t) {
          const float4 a4 = *reinterpret_cast<const float4*>(w3tp + ((t * KC4 + s4) * 64 + lane) * 4);
          acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.x, b[0], acc[t], 0, 0, 0);
          acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.y, b[1], acc[t], 0, 0, 0);
          acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.z, b[2], acc[t], 0, 0, 0);
          acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.w, b[3], acc[t], 0, 0, 0);
        }
      }
#pragma unroll
      for (int t = 0; t < HT; ++t) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int i = 16 * t + r;
          dz2[i] = ((pos2 >> i) & 1u) ? acc[t][r] * dscale : 0.f;
        }
      }
    }
    wave_lds_fence();

    // ---- dW2 += dz2 h1^T with K = node (the dz2 fragments also give d_b_mid); of h1 the sign bits stay
    uint32_t pos1 = 0u;
#pragma unroll
    for (int t = 0; t < HT; ++t) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = (32 * t + drow(r, 0) + 4 * half) * kST + nl;
        slab_a[row] = dz2[16 * t + r];
        slab_b[row] = h1[16 * t + r];
        pos1 |= (h1[16 * t + r] > 0.f ? 1u : 0u) << (16 * t + r);
      }
    }
    wave_lds_fence();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float4 a4[HT], b4[HT];
#pragma unroll
      for (int t = 0; t < HT; ++t) {
        a4[t] = *reinterpret_cast<const float4*>(slab_a + (32 * t + nl) * kST + 16 * half + 4 * q);
        b4[t] = *reinterpret_cast<const float4*>(slab_b + (32 * t + nl) * kST + 16 * half + 4 * q);
        s_b2[t] += (a4[t].x + a4[t].y) + (a4[t].z + a4[t].w);
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
    wave_lds_fence();

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
          const int i = 16 * t + r;
          const float dz1 = ((pos1 >> i) & 1u) ? acc[t][r] * dscale : 0.f;
          s_b1[i] += dz1;
          s_w1[i] = fmaf(dz1, xv, s_w1[i]);
        }
      }
    }
  }

  // ---- every wave is done with the weight images and the slabs: the waves' sums go over them, wave w at [w * RED], then the
  // four are added in wave order
  __syncthreads();
  float* red = smem + wave * RED;
  constexpr int o_w3 = HP * HP, o_w1 = o_w3 + CP * HP, o_b1 = o_w1 + HP, o_b2 = o_b1 + HP, o_b3 = o_b2 + HP;
#pragma unroll
  for (int ta = 0; ta < HT; ++ta) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = 32 * ta + drow(r, 0) + 4 * half;
#pragma unroll
      for (int tb = 0; tb < HT; ++tb) red[row * HP + 32 * tb + nl] = acc_w2[ta][tb][r];
      const float w1s = half_sum(s_w1[16 * ta + r]), b1s = half_sum(s_b1[16 * ta + r]);
      if (nl == 0) {
        red[o_w1 + row] = w1s;
        red[o_b1 + row] = b1s;
      }
    }
    const float b2s = s_b2[ta] + __shfl_xor(s_b2[ta], 32);
    if (half == 0) red[o_b2 + 32 * ta + nl] = b2s;
  }
#pragma unroll
  for (int tc = 0; tc < CT32; ++tc) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
#pragma unroll
      for (int tb = 0; tb < HT; ++tb) red[o_w3 + (32 * tc + drow(r, 0) + 4 * half) * HP + 32 * tb + nl] = acc_w3[tc][tb][r];
    }
    const float b3s = s_b3[tc] + __shfl_xor(s_b3[tc], 32);
    if (half == 0) red[o_b3 + 32 * tc + nl] = b3s;
  }
  __syncthreads();
  const int64_t so = static_cast<int64_t>(blockIdx.y) * p.split_stride;     // this split's block of partial gradients
  for (int idx = threadIdx.x; idx < RED; idx += 256) {
    float a = smem[idx];
#pragma unroll
    for (int w = 1; w < 4; ++w) a += smem[w * RED + idx];
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

bool bwd_cover(const gnan_fmlp_bwd_args* a) { return a->L == 3 && a->H >= 1 && a->H <= 64 && a->C >= 1 && a->C <= kCmaxBwd; }

// Node ranges per feature as csrc/fmlp_bwd_mfma.hip: enough workgroups to fill the chip twice over (one workgroup per CU: the
// LDS), at least one 32-node tile per wave each.
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

template <int HT, int CT32>
int launch_bwd(const BwdParams& p, unsigned splits, hipStream_t st) {
  constexpr size_t lds = static_cast<size_t>(bwd_lds_floats(32 * HT, 32 * CT32)) * sizeof(float);
  static_assert(lds <= kLdsMax, "LDS of one workgroup");
  auto go = [&](auto kernel) {
    if (lds > 64 * 1024) {
      hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                         static_cast<int>(lds));
      if (e != hipSuccess) return gnan::fail(GNAN_ERR_HIP, "fmlp_mc_bwd: hipFuncSetAttribute: %s", hipGetErrorString(e));
    }
    hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>(p.F), splits), dim3(256), lds, st, p);
    return gnan::check_launch("fmlp_mc_bwd_kernel");
  };
  if constexpr (HT == 2 && CT32 == 1) {               // (bwd_channel_tiles: never asked for with Dropout)
    return go(fmlp_mc_bwd_kernel<HT, CT32, false>);
  } else {
    return p.drop_thresh != 0u ? go(fmlp_mc_bwd_kernel<HT, CT32, true>) : go(fmlp_mc_bwd_kernel<HT, CT32, false>);
  }
}

template <int HT>
int launch_bwd_ct(const BwdParams& p, unsigned splits, hipStream_t st) {
  return bwd_channel_tiles(p.H, p.C, p.drop_thresh != 0u) == 1 ? launch_bwd<HT, 1>(p, splits, st) : launch_bwd<HT, 2>(p, splits, st);
}

}  // namespace

extern "C" size_t gnan_fmlp_mc_fwd_workspace_bytes(const gnan_fmlp_args* a) {
  if (!a || a->n < 0 || a->F < 1 || !fwd_cover(a)) return 0;
  size_t bytes = fwd_packed_bytes(a);
  if (a->sum_features && a->n > 0) {                  // room for the per-chunk partial sums
    const int chunks = feature_chunks(a->n, a->F, a->H);
    if (chunks > 1) bytes += static_cast<size_t>(chunks) * a->n * a->C * sizeof(float);
  }
  return bytes;
}

// THE launcher of gnan_fmlp_mc_fwd (seed_dev == NULL) and gnan_fmlp_mc_fwd_dev (seed_dev: the seed's device cell, NULL for p == 0)
static int fmlp_mc_fwd(const gnan_fmlp_args* a, const uint64_t* seed_dev, gnan_stream_t stream) {
  GNAN_REQUIRE(a != nullptr, "fmlp_mc_fwd: null args");
  GNAN_REQUIRE(a->n >= 0 && a->F >= 1, "fmlp_mc_fwd: bad sizes");
  if (!fwd_cover(a))
    return gnan::fail(GNAN_ERR_UNSUPPORTED, "fmlp_mc_fwd: covers 3 <= L <= 4, H <= 64, C <= %d (got L=%d H=%d C=%d)", kCmax, a->L, a->H,
                      a->C);
  if (a->n == 0) return GNAN_OK;
  GNAN_REQUIRE(a->x && a->out && a->w_first && a->w_mid && a->w_last, "fmlp_mc_fwd: null x / out / weight pointer");
  GNAN_REQUIRE(a->x_stride >= a->F, "fmlp_mc_fwd: x row stride smaller than F");
  const int64_t ow = a->sum_features ? a->C : static_cast<int64_t>(a->F) * a->C;
  GNAN_REQUIRE(a->out_stride >= ow, "fmlp_mc_fwd: out row stride smaller than the output width");
  GNAN_REQUIRE(a->dropout_p >= 0.f && a->dropout_p < 1.f, "fmlp_mc_fwd: dropout_p must be in [0, 1)");
  const size_t need = gnan_fmlp_mc_fwd_workspace_bytes(a);
  if (a->workspace == nullptr || a->workspace_bytes < need)
    return gnan::fail(GNAN_ERR_WORKSPACE, "fmlp_mc_fwd: workspace %zu B < required %zu B", a->workspace ? a->workspace_bytes : size_t{0},
                      need);
  GNAN_REQUIRE(reinterpret_cast<uintptr_t>(a->workspace) % 16 == 0, "fmlp_mc_fwd: workspace must be 16-byte aligned");

  FwdParams p;
  p.x = a->x; p.n = a->n; p.x_stride = a->x_stride;
  p.F = a->F; p.L = a->L; p.H = a->H; p.C = a->C;
  p.w_first = a->w_first; p.b_first = a->b_first; p.w_mid = a->w_mid; p.b_mid = a->b_mid;
  p.w_last = a->w_last; p.b_last = a->b_last;
  p.sum_features = a->sum_features; p.out = a->out; p.out_stride = a->out_stride;
  const bool drop = a->dropout_p > 0.f;
  p.drop_thresh = drop ? gnan::drop_threshold(a->dropout_p) : 0u;
  p.drop_scale = drop ? 1.f / (1.f - a->dropout_p) : 1.f;
  p.drop_seed = a->dropout_seed;
  p.seed_dev = p.drop_thresh != 0u ? seed_dev : nullptr;
  const int chunks = feature_chunks(p.n, p.F, p.H);
  p.feat_chunk = (p.F + chunks - 1) / chunks;
  p.feat_chunk += p.feat_chunk & 1;                  // even: chunks start on a double-buffer pair boundary
  const int real_chunks = (p.F + p.feat_chunk - 1) / p.feat_chunk;
  float* packed = static_cast<float*>(a->workspace);
  p.sum_partial = (p.sum_features && real_chunks > 1)
                      ? reinterpret_cast<float*>(reinterpret_cast<char*>(packed) + fwd_packed_bytes(a))
                      : nullptr;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int HT = p.H <= 32 ? 1 : 2, NMID = p.L - 2, CT32 = p.C <= 32 ? 1 : 2;
  hipLaunchKernelGGL(fmlp_mc_pack_kernel, dim3(p.F), dim3(256), 0, st, p, packed, HT, NMID, CT32);
  if (int rc = gnan::check_launch("fmlp_mc_pack_kernel")) return rc;
  if (HT == 1) return NMID == 1 ? launch_fwd_ct<1, 1>(p, packed, st) : launch_fwd_ct<1, 2>(p, packed, st);
  return NMID == 1 ? launch_fwd_ct<2, 1>(p, packed, st) : launch_fwd_ct<2, 2>(p, packed, st);
}

extern "C" int gnan_fmlp_mc_fwd(const gnan_fmlp_args* a, gnan_stream_t stream) { return fmlp_mc_fwd(a, nullptr, stream); }

extern "C" int gnan_fmlp_mc_fwd_dev(const gnan_fmlp_args* a, const uint64_t* seed_cell, gnan_stream_t stream) {
  const uint64_t* seed_dev = nullptr;
  if (int rc = gnan::seed_cell_ok("fmlp_mc_fwd_dev", a, seed_cell, &seed_dev)) return rc;
  return fmlp_mc_fwd(a, seed_dev, stream);
}

extern "C" size_t gnan_fmlp_mc_bwd_workspace_bytes(const gnan_fmlp_bwd_args* a) {
  if (!a || a->n <= 0 || a->F < 1 || !bwd_cover(a)) return 0;
  const int splits = node_splits(a->n, a->F);
  return splits > 1 ? static_cast<size_t>(splits) * block_floats(a) * sizeof(float) : 0;
}

// THE launcher of gnan_fmlp_mc_bwd (seed_dev == NULL) and gnan_fmlp_mc_bwd_dev (seed_dev: the seed's device cell, NULL for p == 0)
static int fmlp_mc_bwd(const gnan_fmlp_bwd_args* a, const uint64_t* seed_dev, gnan_stream_t stream) {
  GNAN_REQUIRE(a != nullptr, "fmlp_mc_bwd: null args");
  GNAN_REQUIRE(a->n >= 0 && a->F >= 1, "fmlp_mc_bwd: bad sizes");
  if (!bwd_cover(a))
    return gnan::fail(GNAN_ERR_UNSUPPORTED, "fmlp_mc_bwd: covers L == 3, H <= 64, C <= %d (got L=%d H=%d C=%d)", kCmaxBwd, a->L, a->H,
                      a->C);
  const size_t lds_need = bwd_lds_bytes(a->H, a->C, a->dropout_p > 0.f);
  if (lds_need > kLdsMax)
    return gnan::fail(GNAN_ERR_UNSUPPORTED, "fmlp_mc_bwd: H=%d C=%d needs %zu B of LDS (> %zu B)", a->H, a->C, lds_need, kLdsMax);
  GNAN_REQUIRE(a->w_first && a->w_last && a->d_w_first && a->d_w_last, "fmlp_mc_bwd: null weight / gradient pointer");
  GNAN_REQUIRE(a->w_mid && a->d_w_mid, "fmlp_mc_bwd: L == 3 needs w_mid and d_w_mid");
  GNAN_REQUIRE((a->b_first == nullptr) == (a->d_b_first == nullptr) && (a->b_mid == nullptr) == (a->d_b_mid == nullptr) &&
                   (a->b_last == nullptr) == (a->d_b_last == nullptr),
               "fmlp_mc_bwd: a bias gradient is wanted exactly where there is a bias");
  const int64_t gw = a->sum_features ? a->C : static_cast<int64_t>(a->F) * a->C;
  GNAN_REQUIRE(a->n == 0 || (a->x && a->grad && a->x_stride >= a->F && a->grad_stride >= gw), "fmlp_mc_bwd: bad x / grad");
  GNAN_REQUIRE(a->dropout_p >= 0.f && a->dropout_p < 1.f, "fmlp_mc_bwd: dropout_p must be in [0, 1)");
  BwdParams p;
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
      return gnan::fail(GNAN_ERR_WORKSPACE, "fmlp_mc_bwd: workspace %zu B < required %zu B", a->workspace ? a->workspace_bytes : size_t{0},
                        need);
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
  const int rc = a->H <= 32 ? launch_bwd_ct<1>(p, sp, st) : launch_bwd_ct<2>(p, sp, st);
  if (rc || splits == 1) return rc;
  gnan::SplitReduceOuts r;
  r.out[0] = a->d_w_first; r.out[1] = a->d_b_first; r.out[2] = a->d_w_mid; r.out[3] = a->d_b_mid; r.out[4] = a->d_w_last;
  r.out[5] = a->d_b_last;
  r.off[0] = 0; r.off[1] = off_b1; r.off[2] = off_w2; r.off[3] = off_b2; r.off[4] = off_w3; r.off[5] = off_b3;
  r.end = blk;
  hipLaunchKernelGGL(gnan::fmlp_split_reduce_kernel, dim3(static_cast<unsigned>((blk + 255) / 256)), dim3(256), 0, st,
                     static_cast<const float*>(a->workspace), blk, splits, r);
  return gnan::check_launch("fmlp_split_reduce_kernel");
}

extern "C" int gnan_fmlp_mc_bwd(const gnan_fmlp_bwd_args* a, gnan_stream_t stream) { return fmlp_mc_bwd(a, nullptr, stream); }

extern "C" int gnan_fmlp_mc_bwd_dev(const gnan_fmlp_bwd_args* a, const uint64_t* seed_cell, gnan_stream_t stream) {
  const uint64_t* seed_dev = nullptr;
  if (int rc = gnan::seed_cell_ok("fmlp_mc_bwd_dev", a, seed_cell, &seed_dev)) return rc;
  return fmlp_mc_bwd(a, seed_dev, stream);
}
