// All-pairs hop codes of MANY small graphs from one edge list (gfx950) — the batch counterpart of csrc/bfs.hip.
//
// bfs.hip gives a workgroup to every SOURCE of one graph and keeps its queues in global memory: right for one graph of a few
// thousand nodes, ten framework launches and a host read per graph for a data set of 30-node molecules.  Here a whole batch is
// three launches, whatever the number of graphs:
//   1. clear       the bit matrices, max_hop and status;
//   2. edges       a thread per edge validates it and sets ONE bit (atomicOr) of its graph's in-adjacency bit matrix — row dst,
//                  bit src; n_g rows of ceil(n_g / 64) 64-bit words.  No sort, no unique: duplicates OR to the same bit;
//   3. BFS         a workgroup per TILE (one graph, up to 64 consecutive sources) copies the graph's matrix into LDS once (row
//                  stride padded to an odd word count: at 64-word-aligned sizes all lanes of a pull step would read one bank) and
//                  each of its four waves walks its sources one at a time, level-synchronous, as a PULL: lane l stands for node
//                  64 b + l, which joins level d + 1 iff it is unseen and its in-adjacency row meets the frontier bitset.  The
//                  wave's ballot IS word b of the next frontier: no atomics, no queue.  The frontier lives in registers (lane w
//                  holds word w, read back with v_readlane), a lane's seen flags are one bit per block of 64 nodes.
// Every byte of a code row is stored exactly once, by the lane that owns the node (on joining, or 255 at the end); max_hop is an
// atomicMax: order-free, so the outputs are bit-reproducible.  gnan_shell_counts_blocks then counts the rows' codes into the
// packed [n_g, max_hop_g + 2] tables, a wave per row.
#include "common.hpp"

namespace {

constexpr int kMaxNodes = GNAN_BFS_BLOCKS_MAX_NODES;
constexpr int kTileSources = 64;      // sources per BFS workgroup
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / gnan::kWave;
static_assert(kMaxNodes % 64 == 0 && kMaxNodes / 64 <= 32, "a lane's seen flags are one 32-bit word: a bit per block of 64 nodes");

__host__ __device__ constexpr int words_of(int n) { return (n + 63) >> 6; }
__host__ __device__ constexpr int stride_of(int n) { return words_of(n) | 1; }                 // LDS row stride: odd
constexpr size_t lds_bytes(int max_nodes) { return static_cast<size_t>(max_nodes) * stride_of(max_nodes) * sizeof(uint64_t); }
static_assert(lds_bytes(kMaxNodes) <= 40 * 1024, "four BFS workgroups per compute unit whatever the batch holds");

struct Params {
  const int64_t* src;
  const int64_t* dst;
  int64_t n_edges, n_nodes;
  const int32_t* graph_of;
  const int32_t* node_off;
  const int64_t* code_off;
  const int64_t* bit_off;
  const int32_t* tile_graph;
  const int32_t* tile_src;
  int32_t n_tiles, n_graphs, max_nodes, max_hops;
  int64_t bit_words;
  uint8_t* code;
  int32_t* max_hop;
  int32_t* status;
  unsigned long long* bits;
};

__global__ __launch_bounds__(kThreads) void bfs_blocks_clear_kernel(const Params p) {
  const int64_t step = static_cast<int64_t>(gridDim.x) * kThreads;
  const int64_t first = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  for (int64_t i = first; i < p.bit_words; i += step) p.bits[i] = 0ull;
  for (int64_t i = first; i < p.n_graphs; i += step) p.max_hop[i] = 0;
  if (first < 2) p.status[first] = 0;
}

__global__ __launch_bounds__(kThreads) void bfs_blocks_edges_kernel(const Params p) {
  const int64_t step = static_cast<int64_t>(gridDim.x) * kThreads;
  int flags = 0;
  for (int64_t e = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x; e < p.n_edges; e += step) {
    const int64_t s = p.src[e], t = p.dst[e];
    if (s < 0 || s >= p.n_nodes || t < 0 || t >= p.n_nodes) { flags |= 4; continue; }
    const int g = p.graph_of[s];
    if (g < 0 || g >= p.n_graphs) { flags |= 4; continue; }
    if (p.graph_of[t] != g) { flags |= 2; continue; }
    const int64_t base = p.node_off[g];
    const int64_t n = p.node_off[g + 1] - base;
    const int64_t ls = s - base, lt = t - base;
    if (ls < 0 || ls >= n || lt < 0 || lt >= n) { flags |= 4; continue; }          // graph_of contradicts node_off
    if (n > p.max_nodes) continue;                                                  // the caller's (gnan_bfs_dense)
    atomicOr(&p.bits[p.bit_off[g] + lt * words_of(static_cast<int>(n)) + (ls >> 6)], 1ull << (ls & 63));
  }
  if (flags) atomicOr(&p.status[0], flags);
}

// word w (wave-uniform) of a bitset whose word i sits in lane i
__device__ __forceinline__ unsigned long long word_of(unsigned long long x, int w) {
  const unsigned lo = static_cast<unsigned>(__builtin_amdgcn_readlane(static_cast<int>(x), w));
  const unsigned hi = static_cast<unsigned>(__builtin_amdgcn_readlane(static_cast<int>(x >> 32), w));
  return (static_cast<unsigned long long>(hi) << 32) | lo;
}

__global__ __launch_bounds__(kThreads) void bfs_blocks_kernel(const Params p) {
  extern __shared__ __align__(16) unsigned long long adj[];        // [n, Ws]: in-adjacency rows of the tile's graph
  const int tid = threadIdx.x;
  const int g = p.tile_graph[blockIdx.x];
  const int src0 = p.tile_src[blockIdx.x];
  if (g < 0 || g >= p.n_graphs) return;
  const int n = p.node_off[g + 1] - p.node_off[g];
  if (n < 1 || n > p.max_nodes || src0 < 0 || src0 >= n) return;   // (workgroup-uniform: nobody is left at the barrier)
  const int W = words_of(n), Ws = W | 1;
  const unsigned long long* bits = p.bits + p.bit_off[g];
  for (int i = tid; i < n * W; i += kThreads) adj[(i / W) * Ws + i % W] = bits[i];
  __syncthreads();

  const int wave = tid >> 6, lane = tid & 63;
  const int src_end = src0 + kTileSources < n ? src0 + kTileSources : n;
  const unsigned pad = 64 * (W - 1) + lane >= n ? 1u << (W - 1) : 0u;     // lanes past the last node: "seen" from the start
  int deepest = 0;
  bool over = false;
  for (int s = src0 + wave; s < src_end; s += kWaves) {
    uint8_t* row = p.code + p.code_off[g] + static_cast<int64_t>(s) * n;
    unsigned long long cur = lane == (s >> 6) ? 1ull << (s & 63) : 0ull;      // lane w: word w of the frontier
    unsigned seen = pad | (lane == (s & 63) ? 1u << (s >> 6) : 0u);            // bit b: node 64 b + lane
    if (lane == (s & 63)) row[s] = 0;
    int d = 0;
    while (d < p.max_hops) {
      const bool store = d + 1 < 255;                  // hop 255 collides with the "unreachable" code
      unsigned long long nxt = 0ull;
      bool any = false;
      for (int b = 0; b < W; ++b) {
        const bool unseen = !((seen >> b) & 1u);
        if (__ballot(unseen) == 0ull) continue;         // (wave-uniform, as every branch around word_of: v_readlane wants all lanes)
        const int v = 64 * b + lane < n ? 64 * b + lane : n - 1;
        const unsigned long long* r = adj + v * Ws;
        unsigned long long acc = 0ull;
        for (int w = 0; w < W; ++w) acc |= r[w] & word_of(cur, w);      // (no skip of empty words: the reads stay in flight together)
        const bool hit = unseen && acc != 0ull;
        const unsigned long long joined = __ballot(hit);
        if (joined) {
          any = true;
          if (hit && store) {
            seen |= 1u << b;
            row[64 * b + lane] = static_cast<uint8_t>(d + 1);
          }
          if (lane == b) nxt = joined;
        }
      }
      if (!any) break;
      if (!store) { over = true; break; }
      cur = nxt;
      ++d;
    }
    deepest = d > deepest ? d : deepest;
    for (int b = 0; b < W; ++b)
      if (!((seen >> b) & 1u)) row[64 * b + lane] = 255;
  }
  if (lane == 0) {
    if (deepest) {
      atomicMax(&p.max_hop[g], deepest);
      atomicMax(&p.status[1], deepest);
    }
    if (over) atomicOr(&p.status[0], 1);
  }
}

struct CountParams {
  const uint8_t* code;
  const int32_t* graph_of;
  int64_t n_nodes;
  const int32_t* node_off;
  const int64_t* code_off;
  const int64_t* cnt_off;
  const int32_t* max_hop;
  int32_t n_graphs, max_nodes;
  int32_t* cnt;
};

__global__ __launch_bounds__(kThreads) void shell_counts_blocks_kernel(const CountParams p) {
  __shared__ int hist[kWaves][GNAN_MAX_CODES];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t node = static_cast<int64_t>(blockIdx.x) * kWaves + wave;
  int g = -1, n = 0, i = 0;
  if (node < p.n_nodes) {
    g = p.graph_of[node];
    if (g >= 0 && g < p.n_graphs) {
      n = p.node_off[g + 1] - p.node_off[g];
      i = static_cast<int>(node - p.node_off[g]);
    }
  }
  const bool live = n >= 1 && n <= p.max_nodes && i >= 0 && i < n;
  for (int d = lane; d < GNAN_MAX_CODES; d += 64) hist[wave][d] = 0;
  __syncthreads();
  if (live) {
    const uint8_t* row = p.code + p.code_off[g] + static_cast<int64_t>(i) * n;
    for (int j = lane; j < n; j += 64) atomicAdd(&hist[wave][row[j]], 1);
  }
  __syncthreads();
  if (live) {
    int D = p.max_hop[g] + 2;
    D = D < 2 ? 2 : (D > GNAN_MAX_CODES ? GNAN_MAX_CODES : D);
    int32_t* out = p.cnt + p.cnt_off[g] + static_cast<int64_t>(i) * D;
    for (int d = lane; d < D - 1; d += 64) out[d] = hist[wave][d];
    if (lane == 0) out[D - 1] = hist[wave][GNAN_MAX_CODES - 1];
  }
}

}  // namespace

extern "C" size_t gnan_bfs_blocks_workspace_bytes(const int32_t* sizes, int32_t n_graphs) {
  size_t words = 0;
  if (sizes == nullptr) return 0;
  for (int32_t g = 0; g < n_graphs; ++g)
    if (sizes[g] >= 1 && sizes[g] <= kMaxNodes) words += static_cast<size_t>(sizes[g]) * words_of(sizes[g]);
  return words * sizeof(uint64_t);
}

extern "C" int gnan_bfs_blocks(const gnan_bfs_blocks_args* a, gnan_stream_t stream) {
  GNAN_REQUIRE(a != nullptr, "bfs_blocks: null args");
  GNAN_REQUIRE(a->n_graphs >= 0 && a->n_nodes >= 0 && a->n_edges >= 0 && a->n_tiles >= 0 && a->max_nodes >= 0,
               "bfs_blocks: negative size (n_graphs=%d n_nodes=%lld n_edges=%lld n_tiles=%d max_nodes=%d)", a->n_graphs,
               static_cast<long long>(a->n_nodes), static_cast<long long>(a->n_edges), a->n_tiles, a->max_nodes);
  if (a->n_graphs == 0) return GNAN_OK;
  if (a->max_nodes > kMaxNodes)
    return gnan::fail(GNAN_ERR_UNSUPPORTED, "bfs_blocks: covers graphs of at most %d nodes (got max_nodes=%d)", kMaxNodes, a->max_nodes);
  GNAN_REQUIRE(a->max_hops >= 1, "bfs_blocks: max_hops must be >= 1 (got %d)", a->max_hops);
  GNAN_REQUIRE(a->graph_of && a->node_off && a->code_off && a->bit_off && a->sizes && a->max_hop && a->status && a->workspace,
               "bfs_blocks: null pointer");
  GNAN_REQUIRE(a->n_edges == 0 || (a->src && a->dst), "bfs_blocks: null edge list");
  GNAN_REQUIRE(a->n_tiles == 0 || (a->tile_graph && a->tile_src && a->code), "bfs_blocks: null tile list or code");
  const size_t need = gnan_bfs_blocks_workspace_bytes(a->sizes, a->n_graphs);
  if (a->workspace_bytes < need)
    return gnan::fail(GNAN_ERR_WORKSPACE, "bfs_blocks: workspace %zu B < required %zu B", a->workspace_bytes, need);
  Params p;
  p.src = a->src; p.dst = a->dst; p.n_edges = a->n_edges; p.n_nodes = a->n_nodes; p.graph_of = a->graph_of;
  p.node_off = a->node_off; p.code_off = a->code_off; p.bit_off = a->bit_off; p.tile_graph = a->tile_graph;
  p.tile_src = a->tile_src; p.n_tiles = a->n_tiles; p.n_graphs = a->n_graphs; p.max_nodes = a->max_nodes;
  p.max_hops = a->max_hops > 255 ? 255 : a->max_hops;
  p.bit_words = static_cast<int64_t>(need / sizeof(uint64_t));
  p.code = a->code; p.max_hop = a->max_hop; p.status = a->status;
  p.bits = static_cast<unsigned long long*>(a->workspace);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int64_t to_clear = p.bit_words > p.n_graphs ? p.bit_words : p.n_graphs;
  const int64_t clear_blocks = (to_clear + kThreads - 1) / kThreads;
  hipLaunchKernelGGL(bfs_blocks_clear_kernel, dim3(static_cast<unsigned>(clear_blocks < 2048 ? (clear_blocks < 1 ? 1 : clear_blocks) : 2048)),
                     dim3(kThreads), 0, st, p);
  if (int rc = gnan::check_launch("bfs_blocks_clear_kernel")) return rc;
  if (p.n_edges > 0) {
    const int64_t edge_blocks = (p.n_edges + kThreads - 1) / kThreads;
    hipLaunchKernelGGL(bfs_blocks_edges_kernel, dim3(static_cast<unsigned>(edge_blocks < 4096 ? edge_blocks : 4096)), dim3(kThreads), 0,
                       st, p);
    if (int rc = gnan::check_launch("bfs_blocks_edges_kernel")) return rc;
  }
  if (p.n_tiles > 0 && p.max_nodes > 0) {
    hipLaunchKernelGGL(bfs_blocks_kernel, dim3(static_cast<unsigned>(p.n_tiles)), dim3(kThreads), lds_bytes(p.max_nodes), st, p);
    if (int rc = gnan::check_launch("bfs_blocks_kernel")) return rc;
  }
  return GNAN_OK;
}

extern "C" int gnan_shell_counts_blocks(const gnan_shell_counts_blocks_args* a, gnan_stream_t stream) {
  GNAN_REQUIRE(a != nullptr, "shell_counts_blocks: null args");
  GNAN_REQUIRE(a->n_graphs >= 0 && a->n_nodes >= 0 && a->max_nodes >= 0, "shell_counts_blocks: negative size (n_graphs=%d n_nodes=%lld max_nodes=%d)",
               a->n_graphs, static_cast<long long>(a->n_nodes), a->max_nodes);
  if (a->n_graphs == 0 || a->n_nodes == 0) return GNAN_OK;
  if (a->max_nodes > kMaxNodes)
    return gnan::fail(GNAN_ERR_UNSUPPORTED, "shell_counts_blocks: covers graphs of at most %d nodes (got max_nodes=%d)", kMaxNodes,
                      a->max_nodes);
  GNAN_REQUIRE(a->code && a->graph_of && a->node_off && a->code_off && a->cnt_off && a->max_hop && a->cnt, "shell_counts_blocks: null pointer");
  GNAN_REQUIRE((a->n_nodes + kWaves - 1) / kWaves <= 0x7fffffffLL, "shell_counts_blocks: too many rows for one launch");
  CountParams p;
  p.code = a->code; p.graph_of = a->graph_of; p.n_nodes = a->n_nodes; p.node_off = a->node_off; p.code_off = a->code_off;
  p.cnt_off = a->cnt_off; p.max_hop = a->max_hop; p.n_graphs = a->n_graphs; p.max_nodes = a->max_nodes; p.cnt = a->cnt;
  hipLaunchKernelGGL(shell_counts_blocks_kernel, dim3(static_cast<unsigned>((p.n_nodes + kWaves - 1) / kWaves)), dim3(kThreads), 0,
                     static_cast<hipStream_t>(stream), p);
  return gnan::check_launch("shell_counts_blocks_kernel");
}
