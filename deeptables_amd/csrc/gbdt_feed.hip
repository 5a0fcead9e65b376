// gbdt_feed.hip — the GBM leaf features inside a resident feed (ops.gbdt_bin_feed / gbdt_leaves_feed; models/preprocessor.py
// GbmLeavesEncoder.fit_feed / transform_feed).  The trees of gbdt.hip are fitted on exactly the columns a feed holds — the
// row-major int32 id block [N][F] and the row-major float32 continuous blocks — so binning reads those blocks where they lie and
// the leaf ids are written straight into the widened blocks: no column is uploaded, no [T][N] leaf matrix is read back.
//
// k_bin_feed.  One launch replaces P dt_gbdt_bin launches and the dt_gbdt_pack launch.  A block of 256 threads walks row tiles of
// DT_GBDT_FEED_ROWS = 256 rows (grid-stride, at most DT_GBDT_FEED_GRID = 256 blocks: one per CU, a block's LDS is most of a CU's).
// Features go in groups of up to DT_GBDT_FEED_GROUP = 64 (the 39 of the documented layout are one group):
//   LDS   edges  float64 [G][255]   the group's edge lists, loaded once per block and group, shared by all its tiles
//         counts int32   [G8]       edges per feature, clamped to [0, 255]
//         stage  uint8   [G8][264]  the tile's bins, FEATURE-major (row stride 264: 8-byte aligned, 66 words = 2 banks off)
//         64 features: 130 560 + 256 + 16 896 = 147 712 bytes of the 160 KiB
//   read  the part of a block's tile that belongs to the group is `rows` runs of `w` consecutive words (the whole slab when the
//         group holds the whole block): element e of it is (row e / w, column e % w), adjacent threads take adjacent elements,
//         so the loads coalesce without a staging pass for the raw values
//   bin   the number of edges <= (double)x by a fixed 8-trip search over the feature's list in LDS (255 < 2^8); NaN: the count
//   out   packed [N][P8]: thread -> (row, 8-byte word): eight stage bytes, one aligned 8-byte store, adjacent threads adjacent
//         words of a row; bins [P][N]: thread -> (feature, row): one byte, adjacent threads adjacent rows of one feature — the
//         transpose happens in LDS, both global writes are contiguous runs.  Features beyond P inside the last word are zero.
// No atomics, no block waits on another.
//
// k_leaves_feed.  k_predict_leaves' walk — grid (row tiles, tree tiles), a tile's node arrays in LDS, one thread per (row, tree),
// adjacent threads adjacent trees — with the tile's packed rows staged in LDS too (64 rows x P8 bytes; every (row, tree) thread
// reads its row up to L - 1 times) and the result written into a feed block: int32 [N][F + T] behind a copy of the old id block
// (the blocks of tree tile 0 copy their rows' F ids in the same launch), or float32 [N][T].
#include "common.h"
#include "optim_dev.h"

namespace dt {

constexpr int kFeedThreads = 256;
constexpr int kFeedRows = DT_GBDT_FEED_ROWS;
constexpr int kFeedGroup = DT_GBDT_FEED_GROUP;
constexpr int kFeedEdges = DT_GBDT_FEED_EDGES;
constexpr int kFeedStride = kFeedRows + 8;               // bytes between two features of the staged tile
constexpr int kFeedSources = DT_GBDT_FEED_MAX_BLOCKS + 1;
static_assert(kFeedRows == kFeedThreads && kFeedGroup % 8 == 0 && kFeedStride % 8 == 0, "tile geometry");
static_assert(kFeedEdges < 256, "a bin is one byte and the search has 8 trips");

// source 0 is the id block (int32), sources 1.. are the float32 blocks; first[s] is the feature number of its column 0
struct FeedSources {
    const void* ptr[kFeedSources];
    int32_t width[kFeedSources];
    int32_t first[kFeedSources];
    int32_t n;
};

__host__ __device__ inline size_t bin_feed_lds(int G) {
    const int G8 = (G + 7) / 8 * 8;
    return (size_t)G * kFeedEdges * sizeof(double) + (size_t)G8 * sizeof(int32_t) + (size_t)G8 * kFeedStride;
}

__global__ __launch_bounds__(kFeedThreads) void k_bin_feed(FeedSources src, int64_t N, int P, int group,
                                                            const double* __restrict__ edges, const int32_t* __restrict__ n_edges,
                                                            uint8_t* __restrict__ bins, uint8_t* __restrict__ packed) {
    extern __shared__ double lds_edges[];                 // [group][255], then counts [G8], then stage [G8][kFeedStride]
    const int group8 = (group + 7) / 8 * 8, P8 = (P + 7) / 8 * 8;
    int32_t* counts = reinterpret_cast<int32_t*>(lds_edges + (size_t)group * kFeedEdges);
    uint8_t* stage = reinterpret_cast<uint8_t*>(counts + group8);
    const int64_t tiles = (N + kFeedRows - 1) / kFeedRows;
    for (int g0 = 0; g0 < P; g0 += group) {
        const int G = P - g0 < group ? P - g0 : group;    // features of this group; G8 covers the zero padding of the last word
        const int G8 = (G + 7) / 8 * 8;
        for (int g = threadIdx.x; g < G8; g += kFeedThreads) {
            const int n = g < G ? n_edges[g0 + g] : 0;
            counts[g] = n < 0 ? 0 : (n > kFeedEdges ? kFeedEdges : n);
        }
        __syncthreads();
        for (int e = threadIdx.x; e < G * kFeedEdges; e += kFeedThreads)
            if (e % kFeedEdges < counts[e / kFeedEdges]) lds_edges[e] = edges[(int64_t)g0 * kFeedEdges + e];
        for (int e = threadIdx.x; e < (G8 - G) * kFeedStride; e += kFeedThreads) stage[G * kFeedStride + e] = 0;
        __syncthreads();
        for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
            const int64_t r0 = tile * kFeedRows;
            const int rows = N - r0 < kFeedRows ? (int)(N - r0) : kFeedRows;
            for (int s = 0; s < src.n; ++s) {
                // the columns [c0, c1) of source s are the features [first + c0, first + c1) of this group
                const int width = src.width[s], first = src.first[s];
                const int c0 = g0 > first ? g0 - first : 0, c1 = g0 + G - first < width ? g0 + G - first : width;
                if (c1 <= c0) continue;
                const int w = c1 - c0, total = rows * w;
                for (int e = threadIdx.x; e < total; e += kFeedThreads) {
                    const int row = e / w, col = c0 + e - row * w;
                    const int64_t at = (r0 + row) * width + col;
                    const double v = s == 0 ? (double)((const int32_t*)src.ptr[s])[at] : (double)((const float*)src.ptr[s])[at];
                    const int g = first + col - g0, n = counts[g];
                    const double* list = lds_edges + g * kFeedEdges;
                    int lo = n;                            // a NaN: the last bin
                    if (v == v) {
                        lo = 0;
#pragma unroll
                        for (int t = 7; t >= 0; --t) {
                            const int probe = lo + (1 << t);
                            if (probe <= n && list[probe - 1] <= v) lo = probe;
                        }
                    }
                    stage[g * kFeedStride + row] = (uint8_t)lo;
                }
            }
            __syncthreads();
            const int words = G8 / 8;
            for (int e = threadIdx.x; e < rows * words; e += kFeedThreads) {
                const int row = e / words, wd = e - row * words;
                uint64_t word = 0;
#pragma unroll
                for (int j = 0; j < 8; ++j) word |= (uint64_t)stage[(8 * wd + j) * kFeedStride + row] << (8 * j);
                *reinterpret_cast<uint64_t*>(packed + (r0 + row) * P8 + g0 + 8 * wd) = word;
            }
            for (int e = threadIdx.x; e < G * rows; e += kFeedThreads) {
                const int g = e / rows, row = e - g * rows;
                bins[(int64_t)(g0 + g) * N + r0 + row] = stage[g * kFeedStride + row];
            }
            __syncthreads();
        }
    }
}

// grid (row tiles, tree tiles); dynamic LDS: nodes [tile][L - 1] x (feat, bin, left, right), n_nodes [tile], then the tile's
// packed rows [DT_GBDT_PREDICT_ROWS][P8] when `staged`
template <bool DENSE>
__global__ __launch_bounds__(kFeedThreads) void k_leaves_feed(const uint8_t* __restrict__ packed, int64_t N, int P8, int T, int L, int tile,
                                                               int staged, const int32_t* __restrict__ node_feat,
                                                               const int32_t* __restrict__ node_bin, const int32_t* __restrict__ node_child,
                                                               const int32_t* __restrict__ n_nodes, const int32_t* __restrict__ ids, int F,
                                                               void* __restrict__ out) {
    extern __shared__ int32_t nodes[];
    const int M = L - 1, t0 = blockIdx.y * tile;
    const int nt = T - t0 < tile ? T - t0 : tile;
    for (int e = threadIdx.x; e < nt * M; e += kFeedThreads) {
        const int64_t s = (int64_t)t0 * M + e;
        nodes[4 * e] = node_feat[s]; nodes[4 * e + 1] = node_bin[s];
        nodes[4 * e + 2] = node_child[2 * s]; nodes[4 * e + 3] = node_child[2 * s + 1];
    }
    int32_t* nn = nodes + 4 * tile * M;
    for (int e = threadIdx.x; e < nt; e += kFeedThreads) nn[e] = n_nodes[t0 + e];
    const int64_t r0 = (int64_t)blockIdx.x * DT_GBDT_PREDICT_ROWS;
    const int rows = N - r0 < DT_GBDT_PREDICT_ROWS ? (int)(N - r0) : DT_GBDT_PREDICT_ROWS;
    const uint8_t* x0 = packed + r0 * P8;                  // the tile's rows: rows * P8 contiguous bytes, 8-byte aligned
    if (staged) {
        uint64_t* lx = reinterpret_cast<uint64_t*>(nn + ((tile + 1) & ~1));
        for (int e = threadIdx.x; e < rows * (P8 / 8); e += kFeedThreads) lx[e] = reinterpret_cast<const uint64_t*>(x0)[e];
        x0 = reinterpret_cast<const uint8_t*>(lx);
    }
    const int64_t W = (int64_t)F + T;
    if (!DENSE && blockIdx.y == 0)
        for (int e = threadIdx.x; e < rows * F; e += kFeedThreads) {
            const int row = e / F, c = e - row * F;
            ((int32_t*)out)[(r0 + row) * W + c] = ids[(r0 + row) * F + c];
        }
    __syncthreads();
    for (int e = threadIdx.x; e < rows * nt; e += kFeedThreads) {
        const int row = e / nt, t = e - row * nt;
        const uint8_t* x = x0 + (int64_t)row * P8;
        const int32_t* nd = nodes + 4 * t * M;
        int leaf = 0, cur = 0;
        if (nn[t] > 0) {
            for (int depth = 0; depth < M; ++depth) {      // a tree of M nodes is at most M deep
                const int f = (unsigned)nd[4 * cur] < (unsigned)P8 ? nd[4 * cur] : 0;
                const int c = nd[4 * cur + 2 + (x[f] > nd[4 * cur + 1] ? 1 : 0)];
                if (c < 0) { leaf = ~c; break; }
                cur = c < M ? c : 0;
            }
        }
        if (DENSE) ((float*)out)[(r0 + row) * T + t0 + t] = (float)leaf;
        else ((int32_t*)out)[(r0 + row) * W + F + t0 + t] = leaf;
    }
}

}  // namespace dt

using namespace dt;

extern "C" int dt_gbdt_bin_feed(const int32_t* ids, int F, const void* const* blocks, const int32_t* widths, int n_blocks, int64_t N,
                                const double* edges, const int32_t* n_edges, void* bins, void* packed, void* stream) {
    const char* who = "dt_gbdt_bin_feed";
    DT_REQUIRE(N >= 0 && N <= DT_GBDT_MAX_ROWS && F >= 0 && n_blocks >= 0 && n_blocks <= DT_GBDT_FEED_MAX_BLOCKS,
               "%s: bad sizes N=%lld F=%d n_blocks=%d (at most %d float blocks)", who, (long long)N, F, n_blocks, DT_GBDT_FEED_MAX_BLOCKS);
    DT_REQUIRE(n_blocks == 0 || (blocks && widths), "%s: null block table", who);
    DT_REQUIRE(F == 0 || N == 0 || (ids && aligned_to(ids, 4)), "%s: null or misaligned id block", who);
    FeedSources src;
    memset(&src, 0, sizeof(src));
    int64_t P = F;
    src.n = 1;
    src.ptr[0] = ids; src.width[0] = F; src.first[0] = 0;
    for (int b = 0; b < n_blocks; ++b) {
        DT_REQUIRE(widths[b] >= 1 && widths[b] <= DT_GBDT_MAX_FEATURES, "%s: block %d has %d columns", who, b, widths[b]);
        DT_REQUIRE(N == 0 || (blocks[b] && aligned_to(blocks[b], 4)), "%s: block %d: null or misaligned pointer", who, b);
        src.ptr[src.n] = blocks[b]; src.width[src.n] = widths[b]; src.first[src.n] = (int32_t)P;
        P += widths[b];
        ++src.n;
    }
    DT_REQUIRE(P >= 1 && P <= DT_GBDT_MAX_FEATURES, "%s: P=%lld features outside [1, %d]", who, (long long)P, DT_GBDT_MAX_FEATURES);
    if (N == 0) return DT_OK;
    DT_REQUIRE(edges && n_edges && bins && packed, "%s: null pointer", who);
    DT_REQUIRE(aligned_to(edges, 8) && aligned_to(n_edges, 4) && aligned_to(packed, 8), "%s: misaligned pointer", who);
    const int group = P < kFeedGroup ? (int)P : kFeedGroup;
    const size_t lds = bin_feed_lds(group);
    const int64_t tiles = (N + kFeedRows - 1) / kFeedRows;
    hipFuncSetAttribute((const void*)k_bin_feed, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(k_bin_feed, dim3((unsigned)(tiles < DT_GBDT_FEED_GRID ? tiles : DT_GBDT_FEED_GRID)), dim3(kFeedThreads), lds,
                       as_stream(stream), src, N, (int)P, group, edges, n_edges, (uint8_t*)bins, (uint8_t*)packed);
    return launch_status(who);
}

extern "C" int dt_gbdt_leaves_feed(const void* packed, int64_t N, int P, int T, int L, const int32_t* node_feat, const int32_t* node_bin,
                                   const int32_t* node_child, const int32_t* n_nodes, const int32_t* ids, int F, int mode, void* out,
                                   void* stream) {
    const char* who = "dt_gbdt_leaves_feed";
    DT_REQUIRE(N >= 0 && N <= DT_GBDT_MAX_ROWS && P >= 1 && P <= DT_GBDT_MAX_FEATURES && T >= 1 && L >= 2 && L <= DT_GBDT_MAX_LEAVES,
               "%s: bad sizes N=%lld P=%d T=%d num_leaves=%d", who, (long long)N, P, T, L);
    DT_REQUIRE(mode == DT_GBDT_FEED_EMBEDDING || mode == DT_GBDT_FEED_DENSE, "%s: unknown mode %d", who, mode);
    DT_REQUIRE(F >= 0 && F <= DT_GBDT_MAX_FEATURES && (mode == DT_GBDT_FEED_EMBEDDING || F == 0),
               "%s: F=%d (a dense block has no id columns)", who, F);
    DT_REQUIRE(N <= INT64_MAX / 4 / ((int64_t)T + F), "%s: N=%lld x (F + T)=%lld overflows", who, (long long)N, (long long)T + F);
    if (N == 0) return DT_OK;
    DT_REQUIRE(packed && node_feat && node_bin && node_child && n_nodes && out && (F == 0 || ids), "%s: null pointer", who);
    DT_REQUIRE(aligned_to(packed, 8) && aligned_to(node_feat, 4) && aligned_to(node_bin, 4) && aligned_to(node_child, 4) &&
               aligned_to(n_nodes, 4) && aligned_to(out, 4) && aligned_to(ids, 4), "%s: misaligned pointer", who);
    const int P8 = (P + 7) / 8 * 8;
    const int per_tree = 16 * (L - 1) + 4;                // bytes of LDS per tree of a tile
    int tile = DT_GBDT_PREDICT_LDS_BYTES / per_tree;      // >= 2 for every L <= DT_GBDT_MAX_LEAVES
    if (tile > T) tile = T;
    if (tile > kFeedThreads) tile = kFeedThreads;
    const int staged = DT_GBDT_PREDICT_ROWS * P8 <= DT_GBDT_FEED_STAGE_BYTES ? 1 : 0;
    const size_t lds = (size_t)4 * tile * (L - 1) * 4 + (size_t)((tile + 1) & ~1) * 4 + (staged ? (size_t)DT_GBDT_PREDICT_ROWS * P8 : 0);
    const int64_t row_tiles = (N + DT_GBDT_PREDICT_ROWS - 1) / DT_GBDT_PREDICT_ROWS;
    DT_REQUIRE(row_tiles <= INT32_MAX && (T + tile - 1) / tile <= 65535, "%s: grid too large", who);
    const dim3 grid((unsigned)row_tiles, (T + tile - 1) / tile);
    if (mode == DT_GBDT_FEED_DENSE) {
        hipFuncSetAttribute((const void*)k_leaves_feed<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL(k_leaves_feed<true>, grid, dim3(kFeedThreads), lds, as_stream(stream), (const uint8_t*)packed, N, P8, T, L, tile,
                           staged, node_feat, node_bin, node_child, n_nodes, ids, F, out);
    } else {
        hipFuncSetAttribute((const void*)k_leaves_feed<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL(k_leaves_feed<false>, grid, dim3(kFeedThreads), lds, as_stream(stream), (const uint8_t*)packed, N, P8, T, L, tile,
                           staged, node_feat, node_bin, node_child, n_nodes, ids, F, out);
    }
    return launch_status(who);
}
