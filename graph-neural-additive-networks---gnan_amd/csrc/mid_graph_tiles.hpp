// The row tiles of the one-launch routes for dense-coded graphs of 129 to 448 nodes (csrc/mid_graph.hip, csrc/mid_graph_nam.hip): the
// tile constants, a tile's hop codes and shell sizes on their way from memory to registers (requested a tile ahead) and from registers
// to LDS.  One copy for both files.
#pragma once
#include <cstdint>

#include "small_graph_body.hpp"

namespace gnan_mid {

using namespace gnan_small;

constexpr int kMidNodes = 448;                       // 7 row tiles
constexpr int kTile = 64;                            // rows per tile
constexpr int kMidBlocks = kMidNodes / kTile;
constexpr int kMidD = kWave;                         // shells (lane = shell in the table steps)
constexpr int kRhoRows = 32;                         // rows per rho group of the backward: 14 groups at 448 nodes
constexpr int kRhoGroupsMid = kMidNodes / kRhoRows;
constexpr int kThreads = kWaves * kWave;
constexpr int kBinCols = kWave + 1;                  // odd stride of the lane-private bin columns

// A tile's hop codes and shell sizes on their way from memory to LDS: ROWS rows of n codes are ROWS * n consecutive bytes that start
// on a 4-byte boundary (ROWS is a multiple of 4), fetched as words; shell sizes as [ROWS][64].
template <int ROWS>
struct TileRegs {
  static constexpr int kWords = ROWS * kMidNodes / 4 / kThreads;
  static constexpr int kCnt = ROWS * kWave / kThreads;
  uint32_t w[kWords];
  int q[kCnt];
};

template <int ROWS>
__device__ __forceinline__ void tile_fetch(TileRegs<ROWS>& r, const uint8_t* code, const int32_t* cnt, int64_t cnt_stride, int n, int D,
                                           int i0) {
  const int rows = n - i0 < ROWS ? n - i0 : ROWS;
  const int words = rows * n / 4;
  const uint32_t* cw = reinterpret_cast<const uint32_t*>(code + static_cast<int64_t>(i0) * n);
#pragma unroll
  for (int u = 0; u < TileRegs<ROWS>::kWords; ++u) {
    const int i = static_cast<int>(threadIdx.x) + u * kThreads;
    r.w[u] = i < words ? cw[i] : 0u;
  }
#pragma unroll
  for (int u = 0; u < TileRegs<ROWS>::kCnt; ++u) {
    const int e = static_cast<int>(threadIdx.x) + u * kThreads;
    const int rr = e / kWave, d = e % kWave;
    r.q[u] = (cnt && rr < rows && d < D) ? cnt[(i0 + rr) * cnt_stride + d] : 1;
  }
}

// ... into LDS.  PAD: rows of n % 4 == 0 codes start `row_bytes` = 4 * (n / 4 | 1) apart (the forward's threads walk a row each:
// with rows 448 bytes apart sixteen of them would share a bank); every other n keeps the rows back to back (row_bytes = n).
template <int ROWS, bool PAD>
__device__ __forceinline__ void tile_store_codes(const TileRegs<ROWS>& r, const uint8_t* code, int n, int i0, uint8_t* s_code) {
  const int rows = n - i0 < ROWS ? n - i0 : ROWS;
  const int bytes = rows * n, words = bytes / 4;
  uint32_t* dw = reinterpret_cast<uint32_t*>(s_code);
  const bool pad = PAD && (n & 3) == 0;
  const int row_words = n / 4, pad_words = row_words | 1;
#pragma unroll
  for (int u = 0; u < TileRegs<ROWS>::kWords; ++u) {
    const int i = static_cast<int>(threadIdx.x) + u * kThreads;
    if (i < words) dw[pad ? (i / row_words) * pad_words + i % row_words : i] = r.w[u];
  }
  // (n * rows not a multiple of 4: the last one to three codes of the graph's last tile)
  for (int i = words * 4 + static_cast<int>(threadIdx.x); i < bytes; i += kThreads) s_code[i] = code[static_cast<int64_t>(i0) * n + i];
}

// row weights lut[d] / max(cnt[i, d], 1) of the tile's rows, [ROWS][64]
template <int ROWS>
__device__ __forceinline__ void tile_store_weights(const TileRegs<ROWS>& r, const float* s_lut, bool with_cnt, int D, float* s_w) {
#pragma unroll
  for (int u = 0; u < TileRegs<ROWS>::kCnt; ++u) {
    const int e = static_cast<int>(threadIdx.x) + u * kThreads;
    const int d = e % kWave;
    if (d < D) {
      const float l = s_lut[d];
      s_w[e] = with_cnt ? l / static_cast<float>(r.q[u] > 1 ? r.q[u] : 1) : l;
    }
  }
}

}  // namespace gnan_mid
