// C == 1 specialisation of the fixed-point moments of the table path (gfx950); routed by csrc/fpwl_moments.hip, which includes this
// file at its end: one object for the moment kernels (why: see there).
//
// The general kernels there spend, per (node, feature) and AFTER the search, a dependent global load of the gradient (the
// channel loop is a run-time loop), two library float64 -> int64 conversions and a random LDS read of the piece's anchor: five
// dependent memory latencies per node and 4 waves per SIMD (58 KB of LDS per 512 threads).  Here the gradient travels with the x
// row (one request each, issued together), the anchor of the piece is the last tree entry the search stepped right at (one
// v_cndmask per step, no anchor array in LDS: 50 KB per workgroup, three workgroups = 6 waves per SIMD), the bins are two arrays
// [2][tot] (8-byte stride: the 64-bit atomics of a wave spread over all banks; interleaved (M0, M1) pairs used every other bank
// pair; over the forward's kept pieces: piece-major), a conversion is fixed_bits() and the workgroup map is the forward's (the
// groups of a node block run back to back on one XCD and share the 128-B lines of x in its L2).
#pragma once
#include "fpwl_common.hpp"

namespace {
using namespace gnan::fpwl;

// SUMF: the gradient is [n, 1] (feature sum) and its M0 term is converted once per node; otherwise [n, F] and read as one
// 16-byte load next to x.  RAGGED: partial last group / unaligned rows, as fpwl_fast_kernel's (csrc/fpwl_fast.hip).
template <int FG, int NSTEP, int BS, bool SUMF, bool RAGGED = false>
__global__ __launch_bounds__(BS) void fpwl_moments_c1_kernel(const MomentParams mp) {
  static_assert(FG % 4 == 0, "feature quads");
  constexpr int FPT = 4, TPN = FG / FPT, NODES = BS / TPN, P2 = 1 << NSTEP;
  constexpr int kTreeWords = tree_words(FG, NSTEP);                     // even: the bins behind it are 8-byte aligned
  const Params& p = mp.f;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = threadIdx.x;
  const int q = tid % TPN, nl = tid / TPN;
  // The steps this kernel shares with the other tree kernels (block map, tree build, tree base, the descent — which here also keeps the
  // last entry stepped right at) are written out, so that every instance is the parent's instruction for instruction.  That did NOT
  // buy back the 3-5 % the searched route had lost — the object the kernel is compiled into did (csrc/fpwl_moments.hip, at the end);
  // whether the helpers of csrc/fpwl_common.hpp could come back here is open (profiles/r21_fpwl_split_code_objects.txt).
  const int64_t id = blockIdx.x;                                        // (id % 8) = XCD, groups of a node block adjacent inside it
  const int grp = static_cast<int>((id >> 3) % p.n_groups);
  const int64_t nb = ((id >> 3) / p.n_groups) * 8 + (id & 7);
  const int64_t n_lo = nb * p.nodes_per_block;
  if (n_lo >= p.n) return;
  const int64_t n_hi = n_lo + p.nodes_per_block < p.n ? n_lo + p.nodes_per_block : p.n;
  const int k0 = grp * FG;
  const int nf = RAGGED ? (p.F - k0 < FG ? p.F - k0 : FG) : FG;       // live features of the group
  const int base = p.off[k0];
  const int tot = p.off[k0 + nf] - base;
  const bool saved = p.piece_in != nullptr;          // (uniform) the forward pass kept the pieces: no trees, no search
  const bool kept = !RAGGED && saved && (SUMF || mp.vec_g);   // ... and the loop below bins them piece-major, from offset 0
  const int PM = p.piece_stride;
  unsigned long long* bins = reinterpret_cast<unsigned long long*>(smem + (kept ? 0 : kTreeWords));   // [2][tot] | [2][PM][FG]
  int* s_off = reinterpret_cast<int*>(smem) + p.soff_offset;
  const unsigned lds_base = lds_address(smem);
  if (tid <= FG) s_off[tid] = p.off[k0 + (tid < nf ? tid : nf)] - base;
  for (int i = tid; i < (kept ? 2 * FG * PM : 2 * tot); i += BS) bins[i] = 0ull;
  __syncthreads();
  if (kept) {
    // nothing to stage: the anchors are read once per piece at the flush, from memory
  } else if (saved) {
    for (int i = tid; i < tot; i += BS) smem[i] = p.anchor[base + i];       // anchors in piece order (tot <= FG * P2)
  } else {
    for (int i = tid; i < FG * P2; i += BS) {        // (build_trees)
      const int f = i >> NSTEP, k = i & (P2 - 1);
      float v = __builtin_nanf("");          // padding: NaN <= x is false for EVERY x (+inf <= +inf would be true)
      if (k) {
        const int j = tree_sorted_index<NSTEP>(k);
        if (j < s_off[f + 1] - s_off[f]) v = p.anchor[base + s_off[f] + j];
      }
      smem[i + (f / FPT) * kTreeSkew] = v;
    }
  }
  __syncthreads();
  const int Q = static_cast<int>(lds_base) + q * ((FPT * P2 + kTreeSkew) * 4);   // tree of the thread's first feature
  int nQ = -Q, nQ4 = 4 - Q;
  asm volatile("" : "+v"(nQ), "+v"(nQ4));           // two opaque registers: compare, select, shift-add per step
  int binoff[FPT];
  float a0[FPT];                                    // anchor of piece 0 (what the search keeps when it never steps right)
  bool live[FPT];
#pragma unroll
  for (int f = 0; f < FPT; ++f) {
    live[f] = !RAGGED || q * FPT + f < nf;
    binoff[f] = s_off[q * FPT + f] - P2;
    a0[f] = live[f] ? p.anchor[base + s_off[q * FPT + f]] : 0.f;
  }
  const double s0 = mp.scales[0], s1 = mp.scales[1];
  if constexpr (!RAGGED) {
    if (saved && (SUMF || mp.vec_g)) {
      // The forward kept the pieces: no search.  Binned here are sum g and sum g * x (the product exact in float64) — two LDS
      // atomics per look-up and NOTHING the wave has to wait for (reading the piece's anchor first put an LDS round trip in
      // front of every pair of atomics: the LDS pipe sat idle 40 % of the time, profiles/r04_sq_train.txt); the anchor enters
      // once per piece and workgroup, when the bins are flushed: M1 = sum g (x - a) = sum g x - a sum g.  The x / gradient /
      // pieces of the next TWO rounds are in flight while a round is binned (unconditional loads from a clamped address — a
      // guarded load hides the loads in flight from the compiler, which then waits for all of them).  In this branch the bins
      // are piece-major, [2][piece_stride][FG] from LDS offset 0 (no trees, no anchors in LDS): see the loop.
      int64_t n = n_lo + nl;
      const int rot = nl & 3;
      if (n < n_hi) {
        const int64_t last = n_hi - 1;
        const uint8_t* pin = p.piece_in + static_cast<int64_t>(grp) * p.n * FG + q * FPT;
        const float* xin = p.x + k0 + q * FPT;
        const float* gin = SUMF ? mp.g : mp.g + k0 + q * FPT;
        struct Round { float4 x; unsigned pc; float4 g; };
        // unconditional loads from a clamped node (see above); three rounds are in flight, each in registers of its own: a
        // "next = far" hand-over at the end of the loop body made every iteration wait for the loads it had just issued
        auto fetch = [&](int64_t m) {
          m = m < n_hi ? m : last;
          Round rd;
          rd.x = *reinterpret_cast<const float4*>(xin + m * p.x_stride);
          rd.pc = *reinterpret_cast<const unsigned*>(pin + m * FG);
          if constexpr (SUMF) { rd.g.x = gin[m * mp.g_stride]; rd.g.y = rd.g.z = rd.g.w = rd.g.x; }
          else rd.g = *reinterpret_cast<const float4*>(gin + m * mp.g_stride);
          return rd;
        };
        auto bin = [&](const Round& rd) {
          const float4 cx = rd.x, cg = rd.g;
          const unsigned cp = rd.pc;
          const float xv[FPT] = {cx.x, cx.y, cx.z, cx.w};
          const float gv[FPT] = {cg.x, cg.y, cg.z, cg.w};
          // Two things keep the lanes of one wave-wide atomic apart (72 % of the LDS-active cycles were bank conflicts,
          // profiles/r04f_sq_train.txt; real data sits in a handful of pieces per feature, and atomics that meet in a bank pair —
          // on one address or not — are served one after the other):
          //  * issue slot s takes feature r = (s + node) % 4 of the thread's quad, so an instruction spreads over the bins of all
          //    FG features, 64 / FG nodes each, instead of four features x sixteen nodes (4.36 -> 4.16 ms per C4 training step);
          //  * the bins are piece-major, [piece][feature]: a feature owns the bank pairs f and f + 16 whatever pieces its nodes
          //    fall into, so lanes of different features never meet (conflict cycles 1.7e8 -> 9e6 per launch).
          // Integer adds: the sums are the same bit for bit.  With the conflicts gone the loop is bound by its vector
          // instructions: the rotation selects x (32 bits) before the product, the piece by a variable bit-field extract,
          // and g * 2^e1 is formed once per node (a power of two: the fused multiply-add rounds the same real number).
          double gs1 = 0.0;
          unsigned long long t0 = 0ull;
          if constexpr (SUMF) {
            gs1 = static_cast<double>(gv[0]) * s1;
            t0 = fixed_bits(gv[0], s0);
          }
#pragma unroll
          for (int s = 0; s < FPT; ++s) {
            const int r = (s + rot) & 3;
            const bool odd = (r & 1) != 0, up = (r & 2) != 0;      // (two selects by the bits of r: a chain of r == k tests
            const float xlo = odd ? xv[1] : xv[0], xhi = odd ? xv[3] : xv[2];   //  is lowered to a switch with branches)
            const float xr = up ? xhi : xlo;
            const int ix = static_cast<int>(__builtin_amdgcn_ubfe(cp, 8u * static_cast<unsigned>(r), 8u)) * FG + (q * FPT + r);
            unsigned long long v0 = t0;
            double gr = gs1;
            if constexpr (!SUMF) {
              const float glo = odd ? gv[1] : gv[0], ghi = odd ? gv[3] : gv[2];
              const float gsel = up ? ghi : glo;
              v0 = fixed_bits(gsel, s0);
              gr = static_cast<double>(gsel) * s1;
            }
            const unsigned long long v1 = fixed_bits_d(gr, static_cast<double>(xr));
            atomicAdd(bins + ix, v0);
            atomicAdd(bins + FG * PM + ix, v1);
          }
        };
        Round ra = fetch(n), rb = fetch(n + NODES), rc = fetch(n + 2 * NODES);
        for (; n < n_hi; n += 3 * NODES) {
          bin(ra);
          ra = fetch(n + 3 * NODES);
          if (n + NODES < n_hi) bin(rb);
          rb = fetch(n + 4 * NODES);
          if (n + 2 * NODES < n_hi) bin(rc);
          rc = fetch(n + 5 * NODES);
        }
      }
      __syncthreads();
      unsigned long long* out = mp.Mi + static_cast<int64_t>(base) * 2;      // [T][2]
      const double ratio = s1 / s0;
      for (int i = tid; i < tot; i += BS) {
        int f = 0;
#pragma unroll
        for (int k = 1; k < FG; ++k) f += s_off[k] <= i ? 1 : 0;              // the feature of piece i (s_off ascending)
        const int b = (i - s_off[f]) * FG + f;
        const long long m0 = static_cast<long long>(bins[b]), m1x = static_cast<long long>(bins[FG * PM + b]);
        if (m0 != 0 || m1x != 0) {
          // (float64: relative error 2^-53 of |a sum g| per workgroup and piece — the same in every run: the node blocks are fixed)
          const long long m1 = m1x - __double2ll_rn(static_cast<double>(p.anchor[base + i]) * static_cast<double>(m0) * ratio);
          if (m0 != 0) atomicAdd(out + 2 * i, static_cast<unsigned long long>(m0));
          if (m1 != 0) atomicAdd(out + 2 * i + 1, static_cast<unsigned long long>(m1));
        }
      }
      return;
    }
  }
  for (int64_t n = n_lo + nl; n < n_hi; n += NODES) {
    float xv[FPT];
    if constexpr (RAGGED) {
      const float* xr = p.x + n * p.x_stride + k0 + q * FPT;
#pragma unroll
      for (int f = 0; f < FPT; ++f) xv[f] = live[f] ? xr[f] : 0.f;
    } else {
      const float4 t = *reinterpret_cast<const float4*>(p.x + n * p.x_stride + k0 + q * FPT);
      xv[0] = t.x; xv[1] = t.y; xv[2] = t.z; xv[3] = t.w;
    }
    float gv[FPT];
    if constexpr (SUMF) {
      gv[0] = gv[1] = gv[2] = gv[3] = mp.g[n * mp.g_stride];
    } else {
      const float* gr = mp.g + n * mp.g_stride + k0 + q * FPT;
      if (!RAGGED && mp.vec_g) {
        const float4 g4 = *reinterpret_cast<const float4*>(gr);
        gv[0] = g4.x; gv[1] = g4.y; gv[2] = g4.z; gv[3] = g4.w;
      } else {
#pragma unroll
        for (int f = 0; f < FPT; ++f) gv[f] = live[f] ? gr[f] : 0.f;
      }
    }
    int a[FPT];
    float last[FPT];
    if (saved) {
      const unsigned packed = *reinterpret_cast<const unsigned*>(p.piece_in + (static_cast<int64_t>(grp) * p.n + n) * FG + q * FPT);
#pragma unroll
      for (int f = 0; f < FPT; ++f) {
        const int pc = static_cast<int>((packed >> (8 * f)) & 0xffu);
        a[f] = Q + ((pc + P2) << 2);                // the tree address the search would have ended at
        last[f] = live[f] ? smem[binoff[f] + P2 + pc] : 0.f;
      }
    } else {
#pragma unroll
      for (int f = 0; f < FPT; ++f) {
        a[f] = Q + 4;                               // node 1 = root
        last[f] = a0[f];
      }
#pragma unroll
      for (int step = 0; step < NSTEP; ++step) {
#pragma unroll
        for (int f = 0; f < FPT; ++f) {
          const float e = lds_f32(a[f] + f * (P2 * 4));
          const bool right = e <= xv[f];
          a[f] = (a[f] << 1) + (right ? nQ4 : nQ);
          last[f] = right ? e : last[f];
        }
      }
    }
    int idx[FPT];
    unsigned long long t0[FPT], t1[FPT];
#pragma unroll
    for (int f = 0; f < FPT; ++f) {
      idx[f] = (!RAGGED || live[f]) ? binoff[f] + ((a[f] - Q) >> 2) : -1;
      t0[f] = fixed_bits(gv[SUMF ? 0 : f], s0);
      t1[f] = fixed_bits(gv[f] * (xv[f] - last[f]), s1);
    }
    const int rot = nl & 3;                            // (issue slots rotated over the quad's features: see the kept-pieces loop)
#pragma unroll
    for (int s = 0; s < FPT; ++s) {
      const int r = (s + rot) & 3;
      const int ix = r == 0 ? idx[0] : (r == 1 ? idx[1] : (r == 2 ? idx[2] : idx[3]));
      const unsigned long long v0 = SUMF ? t0[0] : (r == 0 ? t0[0] : (r == 1 ? t0[1] : (r == 2 ? t0[2] : t0[3])));
      const unsigned long long v1 = r == 0 ? t1[0] : (r == 1 ? t1[1] : (r == 2 ? t1[2] : t1[3]));
      if (!RAGGED || ix >= 0) {
        atomicAdd(bins + ix, v0);
        atomicAdd(bins + tot + ix, v1);
      }
    }
  }
  __syncthreads();
  unsigned long long* out = mp.Mi + static_cast<int64_t>(base) * 2;      // [T][2]
  for (int i = tid; i < 2 * tot; i += BS) {
    const unsigned long long v = bins[i];
    const int m = i >= tot ? 1 : 0;
    if (v != 0ull) atomicAdd(out + 2 * (i - m * tot) + m, v);
  }
}

template <int FG, int NSTEP, int BS, bool RAGGED>
int launch_c1(MomentParams mp, hipStream_t st, gnan_fpwl_moments_info* probe) {
  Params& p = mp.f;
  const size_t pieces = static_cast<size_t>(p.max_group_pieces);
  size_t lds = tree_words(FG, NSTEP) * sizeof(float) + pieces * 2 * sizeof(unsigned long long);
  p.piece_stride = (p.max_pieces + 1) & ~1;
  const bool saved = p.piece_in != nullptr;
  const bool kept = !RAGGED && saved && (p.sum_features || mp.vec_g);    // piece-major bins from offset 0, no trees
  if (kept) lds = static_cast<size_t>(2) * FG * p.piece_stride * sizeof(unsigned long long);
  p.soff_offset = static_cast<int>(lds / sizeof(float));
  lds += (FG + 1) * sizeof(int);
  if (lds > kMaxLds) return -1;                          // caller falls back to the general kernels
  p.nodes_per_block = tuned_moment_block(p.n, p.n_groups, lds, BS);
  if (probe) {                                           // (the branches of the kernel, by the conditions it tests)
    const int kernel = RAGGED ? GNAN_FPWL_MOMENTS_C1_RAGGED
                              : (!saved ? GNAN_FPWL_MOMENTS_C1_SEARCH : (kept ? GNAN_FPWL_MOMENTS_C1_KEPT : GNAN_FPWL_MOMENTS_C1_SAVED));
    fill_probe(probe, kernel, NSTEP, p, BS / (FG / 4), BS, saved, lds);
    return GNAN_OK;
  }
  const int64_t bx = ((p.n + p.nodes_per_block - 1) / p.nodes_per_block + 7) / 8 * 8;   // whole rounds of the 8 XCDs
  if (bx * p.n_groups > 0x7fffffffLL) return gnan::fail(GNAN_ERR_UNSUPPORTED, "fpwl: too many nodes for one launch");
  const dim3 grid(static_cast<unsigned>(bx * p.n_groups));
  if (p.sum_features) return launch_with_lds(fpwl_moments_c1_kernel<FG, NSTEP, BS, true, RAGGED>, "fpwl_moments_c1_kernel", grid, BS, lds, st, mp);
  return launch_with_lds(fpwl_moments_c1_kernel<FG, NSTEP, BS, false, RAGGED>, "fpwl_moments_c1_kernel", grid, BS, lds, st, mp);
}

template <int FG, int BS>
int launch_c1_groups(const MomentParams& mp, int nstep, bool ragged, hipStream_t st, gnan_fpwl_moments_info* probe) {
  return by_nstep(nstep, [&](auto ns) {
    constexpr int NS = decltype(ns)::value;
    return ragged ? launch_c1<FG, NS, BS, true>(mp, st, probe) : launch_c1<FG, NS, BS, false>(mp, st, probe);
  });
}

}  // namespace

// the workgroups csrc/fpwl_moments.hip plans for whole feature quads: 512 threads were three workgroups (24 waves) per CU; 640
// (30 waves): +13 %/+6 %, 1024 (32 waves): +-0 on C4
int gnan::fpwl::launch_moments_c1(const MomentParams& mp, int fg, int bs, int nstep, bool ragged, hipStream_t st,
                                  gnan_fpwl_moments_info* probe) {
  if (fg == 4 && bs == 256) return launch_c1_groups<4, 256>(mp, nstep, ragged, st, probe);
  if (fg == 4 && bs == 1024) return launch_c1_groups<4, 1024>(mp, nstep, ragged, st, probe);
  if (fg == 8 && bs == 512) return launch_c1_groups<8, 512>(mp, nstep, ragged, st, probe);
  if (fg == 16 && bs == 512) return launch_c1_groups<16, 512>(mp, nstep, ragged, st, probe);
  return gnan::fail(GNAN_ERR_UNSUPPORTED, "fpwl_moments: no one-channel kernel for groups of %d features in workgroups of %d threads", fg, bs);
}
