// gradclip.hip — keras.optimizers' clipvalue / clipnorm / global_clipnorm on the device (gfx950, wave64), and the row-sparse
// table gradient with its duplicate lookups summed (dt_rows_coalesce), which a norm or an element clamp of the true per-row
// gradient needs: clip(a + b) is not clip(a) + clip(b), and |a + b| is not the norm of the lookups side by side.
//
// The rules are those of metrics.hip and regularizer.hip: no float atomics, no block waits for another (what one needs from
// the others was written by an EARLIER launch), every sum runs in an order fixed by the sizes and the id pattern, nothing is
// allocated, there is no host synchronisation, and every scalar a later kernel needs (sums, counts) is read from device
// memory: a captured hipGraph of the step replays correctly.
//
// Coalesce.  keys = row id (a skipped lookup: 2^32 - 1, which sorts last), values = lookup position; dt_metric_sort_pairs is
// stable, so a row's lookups keep their order.  Then, over the sorted keys: k_co_tile_counts (segment heads and valid keys
// per tile) -> k_co_tile_scan (one block: exclusive scan of the tiles, the totals) -> k_co_apply (head p of segment j:
// seg_start[j] = p, out_rows[j] = key; seg_of[p] = j for every valid p; out_rows[p] = -1 behind the last segment).
// k_co_chunk_sum: the sorted positions are cut into chunks of kChunk = 512; a block takes one chunk, and one thread per
// (piece, 4 columns) adds the piece's value rows in order, a piece being the part of one segment inside the chunk.  A segment
// inside one chunk is finished there; one that spans chunks leaves a partial per chunk (slot 2b: the piece that came in from
// chunk b - 1, slot 2b + 1: the piece that goes on into chunk b + 1) and k_co_final adds them in chunk order — so a hot row
// with thousands of lookups is 512-row walks in parallel plus one short walk over its partials.  k_co_final also zero-fills
// the rows behind the last segment.
//
// Sums of squares: regularizer.hip's scheme (descriptors as kernel arguments, 32 tensors per launch; a block sums one chunk of
// 4096 elements in float64 in a fixed order; then one block per tensor adds its partials in index order).  Per field of a
// coalesced table: the rows are sorted, a field is one contiguous range found by binary search; DT_FIELD_SUMSQ_PARTS blocks
// take a slice of it each, then one thread per field adds the slices in order.
//
// Clip: written once (clip_one) with contraction off; the scale comes from the device sums.
#include <math.h>
#include "common.h"

namespace dt {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr int kItems = 16;
constexpr int kTile = kThreads * kItems;          // positions per block of the head scan
constexpr int kChunk = 512;                       // sorted positions per block of the sum: dt_rows_coalesce_chunk()
constexpr int kFieldParts = DT_FIELD_SUMSQ_PARTS;  // slices a field's sum of squares is taken in
constexpr int kFieldsInLds = 1024;                // dt_rows_clip keeps up to this many fields' offsets and norms in LDS
constexpr int kMulti = 32;                        // tensors per launch
constexpr int kElems = 4096;                      // elements per block of the dense kernels (= dt_reg_chunk())
constexpr int kMaxBlocks = 2048;                  // grid-stride kernels
constexpr int kMaxD = 1 << 16;
constexpr int64_t kMaxN = (int64_t)1 << 31;
constexpr int64_t kMaxElems = (int64_t)1 << 40;
constexpr int64_t kMaxV = ((int64_t)1 << 32) - 1;
constexpr uint32_t kSkip = 0xFFFFFFFFu;

inline int64_t a256(int64_t b) { return (b + 255) & ~(int64_t)255; }
inline int64_t tiles_of(int64_t n) { return (n + kTile - 1) / kTile; }
inline int64_t chunks_of(int64_t n) { return (n + kChunk - 1) / kChunk; }
inline int64_t elem_blocks(int64_t n) { return (n + kElems - 1) / kElems; }
inline bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }
inline unsigned stride_blocks(int64_t items) {
    const int64_t b = (items + kThreads - 1) / kThreads;
    return (unsigned)(b < kMaxBlocks ? (b > 0 ? b : 1) : kMaxBlocks);
}

// ---- block helpers (kThreads threads; every thread of the block calls them) ----------------------------------------------
__device__ __forceinline__ uint32_t block_excl_scan_u32(uint32_t v, uint32_t* total, uint32_t* sh) {
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    uint32_t incl = v;
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
        const uint32_t t = __shfl_up(incl, o, kWave);
        if (lane >= o) incl += t;
    }
    if (lane == kWave - 1) sh[wave] = incl;
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
        const uint32_t s = sh[w];
        if (w < wave) before += s;
        all += s;
    }
    __syncthreads();
    *total = all;
    return before + incl - v;
}
// sum over the block in a fixed order (lanes by halving, then the waves in order); every thread returns it
template <typename T>
__device__ __forceinline__ T block_sum(T v, T* sh) {
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) v += __shfl_down(v, o, kWave);
    if ((threadIdx.x & (kWave - 1)) == 0) sh[threadIdx.x / kWave] = v;
    __syncthreads();
    T all = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) all += sh[w];
    __syncthreads();
    return all;
}

// ---- coalesce ---------------------------------------------------------------------------------------------------------------
struct CoWs {
    uint32_t *keys, *pos, *seg_start, *seg_of, *tile_heads, *tile_valid, *meta;     // meta: [0] segments [1] valid keys
    char* sort_ws;
    float* partial;
};

int64_t sort_bytes(int64_t n) { return n > 0 ? dt_metric_sort_workspace_bytes(n) : 0; }

int64_t co_ws_bytes(int64_t n, int D) {
    return 4 * a256(4 * n) + a256(sort_bytes(n)) + 2 * a256(4 * tiles_of(n)) + 256 + a256(2 * chunks_of(n) * (int64_t)D * 4);
}

CoWs co_ws(void* ws, int64_t n) {
    char* w = reinterpret_cast<char*>(ws);
    CoWs c;
    c.keys = reinterpret_cast<uint32_t*>(w); w += a256(4 * n);
    c.pos = reinterpret_cast<uint32_t*>(w); w += a256(4 * n);
    c.seg_start = reinterpret_cast<uint32_t*>(w); w += a256(4 * n);
    c.seg_of = reinterpret_cast<uint32_t*>(w); w += a256(4 * n);
    c.sort_ws = w; w += a256(sort_bytes(n));
    c.tile_heads = reinterpret_cast<uint32_t*>(w); w += a256(4 * tiles_of(n));
    c.tile_valid = reinterpret_cast<uint32_t*>(w); w += a256(4 * tiles_of(n));
    c.meta = reinterpret_cast<uint32_t*>(w); w += 256;
    c.partial = reinterpret_cast<float*>(w);
    return c;
}

__global__ __launch_bounds__(kThreads) void k_co_keys(const int64_t* __restrict__ rows, int64_t n, int64_t V,
                                                      uint32_t* __restrict__ keys, uint32_t* __restrict__ pos) {
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) {
        const int64_t r = rows[i];
        keys[i] = (r >= 0 && r < V) ? (uint32_t)r : kSkip;
        pos[i] = (uint32_t)i;
    }
}

__device__ __forceinline__ bool is_head(const uint32_t* __restrict__ keys, int64_t p) {
    const uint32_t k = keys[p];
    return k != kSkip && (p == 0 || keys[p - 1] != k);
}

__global__ __launch_bounds__(kThreads) void k_co_tile_counts(const uint32_t* __restrict__ keys, int64_t n,
                                                             uint32_t* __restrict__ tile_heads, uint32_t* __restrict__ tile_valid) {
    __shared__ uint32_t sh[kWaves];
    const int64_t lo = (int64_t)blockIdx.x * kTile;
    uint32_t heads = 0, valid = 0;
#pragma unroll
    for (int k = 0; k < kItems; ++k) {
        const int64_t p = lo + k * kThreads + threadIdx.x;
        if (p < n) {
            heads += is_head(keys, p);
            valid += keys[p] != kSkip;
        }
    }
    heads = block_sum<uint32_t>(heads, sh);
    valid = block_sum<uint32_t>(valid, sh);
    if (threadIdx.x == 0) {
        tile_heads[blockIdx.x] = heads;
        tile_valid[blockIdx.x] = valid;
    }
}

// one block: tile_heads becomes its exclusive scan; meta[0] = segments, meta[1] = valid keys, count[0] = segments
__global__ __launch_bounds__(kThreads) void k_co_tile_scan(uint32_t* __restrict__ tile_heads, const uint32_t* __restrict__ tile_valid,
                                                           int64_t tiles, uint32_t* __restrict__ meta, int64_t* __restrict__ count) {
    __shared__ uint32_t sh[kWaves];
    uint32_t base = 0, valid = 0;
    for (int64_t t0 = 0; t0 < tiles; t0 += kThreads) {
        const int64_t t = t0 + threadIdx.x;
        const uint32_t v = t < tiles ? tile_heads[t] : 0u;
        const uint32_t u = t < tiles ? tile_valid[t] : 0u;
        uint32_t total;
        const uint32_t ex = block_excl_scan_u32(v, &total, sh);
        if (t < tiles) tile_heads[t] = base + ex;
        base += total;
        valid += block_sum<uint32_t>(u, sh);
    }
    if (threadIdx.x == 0) {
        meta[0] = base;
        meta[1] = valid;
        count[0] = (int64_t)base;
    }
}

// thread t of a tile owns the kItems consecutive positions lo + t * kItems ..; keys come in and segment ids go out through LDS
// (coalesced both ways; one pad word per kItems keeps the threads' walks on different banks)
__device__ __forceinline__ int padded(int i) { return i + (i >> 4); }
static_assert(kItems == 16, "padded(): one pad word per 16");

__global__ __launch_bounds__(kThreads) void k_co_apply(const uint32_t* __restrict__ keys, int64_t n,
                                                       const uint32_t* __restrict__ tile_base, const uint32_t* __restrict__ meta,
                                                       uint32_t* __restrict__ seg_start, uint32_t* __restrict__ seg_of,
                                                       int64_t* __restrict__ out_rows) {
    __shared__ uint32_t sh[kWaves];
    __shared__ uint32_t s_key[kTile + kTile / kItems + 2];      // s_key[padded(i) + 1]: key of tile_lo + i; s_key[0]: of tile_lo - 1
    __shared__ uint32_t s_seg[kTile + kTile / kItems + 1];
    const int64_t tile_lo = (int64_t)blockIdx.x * kTile;
    const int cnt = n - tile_lo < kTile ? (int)(n - tile_lo) : kTile;
    const int64_t count = meta[0];
    for (int i = threadIdx.x; i < cnt; i += kThreads) s_key[padded(i) + 1] = keys[tile_lo + i];
    if (threadIdx.x == 0) s_key[0] = tile_lo > 0 ? keys[tile_lo - 1] : kSkip;      // (position 0: any valid key is a head)
    __syncthreads();
    const int lo = threadIdx.x * kItems;
    uint32_t prev = lo < cnt ? (lo == 0 ? s_key[0] : s_key[padded(lo - 1) + 1]) : kSkip;
    const uint32_t first_prev = prev;
    uint32_t mine = 0;
#pragma unroll
    for (int k = 0; k < kItems; ++k) {
        if (lo + k < cnt) {
            const uint32_t key = s_key[padded(lo + k) + 1];
            mine += key != kSkip && key != prev;
            prev = key;
        }
    }
    uint32_t total;
    uint32_t j = tile_base[blockIdx.x] + block_excl_scan_u32(mine, &total, sh);      // segments that start before `lo`
    prev = first_prev;
#pragma unroll
    for (int k = 0; k < kItems; ++k) {
        if (lo + k >= cnt) break;
        const uint32_t key = s_key[padded(lo + k) + 1];
        if (key != kSkip && key != prev) {
            seg_start[j] = (uint32_t)(tile_lo + lo + k);
            out_rows[j] = (int64_t)key;                    // (j < count; the fill below writes p >= count: no two writers)
            ++j;
        }
        prev = key;
        s_seg[padded(lo + k)] = key == kSkip ? kSkip : j - 1;      // (a valid key has a head at or before it: j >= 1)
    }
    __syncthreads();
    for (int i = threadIdx.x; i < cnt; i += kThreads) {
        seg_of[tile_lo + i] = s_seg[padded(i)];
        if (tile_lo + i >= count) out_rows[tile_lo + i] = -1;
    }
}

template <bool VEC>
__device__ __forceinline__ void add_row(float* acc, const float* __restrict__ src) {
    if (VEC) {
        const float4 q = *reinterpret_cast<const float4*>(src);
        acc[0] += q.x; acc[1] += q.y; acc[2] += q.z; acc[3] += q.w;
    } else {
        acc[0] += src[0];
    }
}
template <bool VEC>
__device__ __forceinline__ void put_row(float* __restrict__ dst, const float* acc) {
    if (VEC)
        *reinterpret_cast<float4*>(dst) = make_float4(acc[0], acc[1], acc[2], acc[3]);
    else
        dst[0] = acc[0];
}

// block b: the sorted positions [b * kChunk, ..); one thread per (piece, column group) walks the piece in order
template <bool VEC>
__global__ __launch_bounds__(kThreads) void k_co_chunk_sum(const uint32_t* __restrict__ seg_of, const uint32_t* __restrict__ seg_start,
                                                           const uint32_t* __restrict__ meta, const uint32_t* __restrict__ spos,
                                                           const float* __restrict__ values, int D, int64_t n,
                                                           float* __restrict__ out_vals, float* __restrict__ partial) {
    __shared__ uint32_t s_seg[kChunk + 1];                 // s_seg[i + 1]: the segment of position lo + i; s_seg[0]: of lo - 1
    __shared__ uint32_t s_pos[kChunk];
    const int64_t lo = (int64_t)blockIdx.x * kChunk;
    const int cnt = n - lo < kChunk ? (int)(n - lo) : kChunk;
    for (int i = threadIdx.x; i < cnt; i += kThreads) {
        s_seg[i + 1] = seg_of[lo + i];
        s_pos[i] = spos[lo + i];
    }
    if (threadIdx.x == 0) s_seg[0] = lo > 0 ? seg_of[lo - 1] : kSkip;
    __syncthreads();
    const int64_t count = meta[0], n_valid = meta[1];
    const int CG = VEC ? D / 4 : D, W = VEC ? 4 : 1;
    const int items = cnt * CG;
    for (int item = threadIdx.x; item < items; item += kThreads) {
        const int pl = item / CG, cg = item - pl * CG;
        const uint32_t seg = s_seg[pl + 1];
        if (seg == kSkip) continue;
        const bool head = s_seg[pl] != seg;
        if (!(head || pl == 0)) continue;                  // a piece starts at a segment's head or at the chunk's first position
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        int q = pl;
        for (; q < cnt && s_seg[q + 1] == seg; ++q) add_row<VEC>(acc, values + (int64_t)s_pos[q] * D + cg * W);
        const int64_t seg_end = (int64_t)seg + 1 < count ? (int64_t)seg_start[seg + 1] : n_valid;
        const bool whole = head && lo + q == seg_end;
        float* dst = whole ? out_vals + (int64_t)seg * D : partial + (2 * (int64_t)blockIdx.x + (head ? 1 : 0)) * D;
        put_row<VEC>(dst + cg * W, acc);
    }
}

// row j of the output: zero behind the last segment; a segment that spans chunks: its partials in chunk order
template <bool VEC>
__global__ __launch_bounds__(kThreads) void k_co_final(const uint32_t* __restrict__ seg_start, const uint32_t* __restrict__ meta,
                                                       const float* __restrict__ partial, int D, int64_t n,
                                                       float* __restrict__ out_vals) {
    const int64_t count = meta[0], n_valid = meta[1];
    const int CG = VEC ? D / 4 : D, W = VEC ? 4 : 1;
    const int64_t items = n * CG;
    for (int64_t item = (int64_t)blockIdx.x * kThreads + threadIdx.x; item < items; item += (int64_t)gridDim.x * kThreads) {
        const int64_t j = item / CG;
        const int cg = (int)(item - j * CG);
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        if (j < count) {
            const int64_t s = seg_start[j], e = j + 1 < count ? (int64_t)seg_start[j + 1] : n_valid;
            const int64_t b0 = s / kChunk, b1 = (e - 1) / kChunk;
            if (b1 == b0) continue;                        // finished inside its chunk
            add_row<VEC>(acc, partial + (2 * b0 + 1) * D + cg * W);
            for (int64_t b = b0 + 1; b <= b1; ++b) add_row<VEC>(acc, partial + 2 * b * D + cg * W);
        }
        put_row<VEC>(out_vals + j * D + cg * W, acc);
    }
}

// ---- sums of squares ----------------------------------------------------------------------------------------------------------
struct SumsqMulti {
    const float* x[kMulti];
    int64_t n[kMulti];
    int block_start[kMulti + 1];
    int count;
};

// sum of squares of m floats at x in float64: thread t owns the groups of four t, t + 256, ..; the same elements in the same
// order whether a group is read as one float4 or as four floats
__device__ __forceinline__ double sumsq_range(const float* __restrict__ x, int64_t m) {
    const bool vec = (reinterpret_cast<uintptr_t>(x) & 15) == 0;
    double s = 0;
    for (int64_t g = threadIdx.x; g * 4 < m; g += kThreads) {
        float e[4] = {0.f, 0.f, 0.f, 0.f};
        const int64_t left = m - g * 4;
        if (vec && left >= 4) {
            const float4 q = *reinterpret_cast<const float4*>(x + g * 4);
            e[0] = q.x; e[1] = q.y; e[2] = q.z; e[3] = q.w;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < left) e[k] = x[g * 4 + k];
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const double v = (double)e[k];
            s += v * v;
        }
    }
    return s;
}

__global__ __launch_bounds__(kThreads) void k_sumsq_partial(SumsqMulti d, double* __restrict__ partial) {
    __shared__ double sh[kWaves];
    int t = 0;
    while (t + 1 < d.count && (int)blockIdx.x >= d.block_start[t + 1]) ++t;
    const int64_t lo = (int64_t)(blockIdx.x - d.block_start[t]) * kElems;
    const int64_t rest = d.n[t] - lo;
    const double s = block_sum<double>(sumsq_range(d.x[t] + lo, rest < kElems ? rest : kElems), sh);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// block t: tensor t's partials in index order (thread u takes u, u + 256, .., then the fixed tree); an empty tensor gives 0
__global__ __launch_bounds__(kThreads) void k_sumsq_total(SumsqMulti d, const double* __restrict__ partial, double* __restrict__ sums) {
    __shared__ double sh[kWaves];
    const int t = blockIdx.x;
    double s = 0;
    for (int i = d.block_start[t] + threadIdx.x; i < d.block_start[t + 1]; i += kThreads) s += partial[i];
    s = block_sum<double>(s, sh);
    if (threadIdx.x == 0) sums[t] = s;
}

// first index in [0, cnt) whose row is >= `row` (rows ascending)
__device__ __forceinline__ int64_t lower_bound_rows(const int64_t* __restrict__ rows, int64_t cnt, int64_t row) {
    int64_t lo = 0, hi = cnt;
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (rows[mid] < row) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// block (f, part): the part-th slice of field f's elements; slices start a multiple of four elements into the field
__global__ __launch_bounds__(kThreads) void k_field_partial(const int64_t* __restrict__ out_rows, const float* __restrict__ out_vals,
                                                            int64_t n, int D, const int64_t* __restrict__ count,
                                                            const int64_t* __restrict__ row_offset, int F, int64_t V,
                                                            double* __restrict__ partial) {
    __shared__ double sh[kWaves];
    const int f = blockIdx.x / kFieldParts, part = blockIdx.x - f * kFieldParts;
    int64_t cnt = count[0];
    cnt = cnt < 0 ? 0 : (cnt > n ? n : cnt);
    const int64_t lo = lower_bound_rows(out_rows, cnt, row_offset[f]);
    const int64_t hi = f + 1 < F ? lower_bound_rows(out_rows, cnt, row_offset[f + 1]) : lower_bound_rows(out_rows, cnt, V);
    const int64_t m = hi > lo ? (hi - lo) * D : 0;
    const int64_t per = ((m + kFieldParts - 1) / kFieldParts + 3) & ~(int64_t)3;
    const int64_t a = part * per < m ? part * per : m, b = a + per < m ? a + per : m;
    const double s = block_sum<double>(sumsq_range(out_vals + lo * D + a, b - a), sh);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// thread f: field f's parts in index order
__global__ __launch_bounds__(kThreads) void k_field_total(const double* __restrict__ partial, int F, double* __restrict__ sums) {
    const int f = blockIdx.x * kThreads + threadIdx.x;
    if (f >= F) return;
    double s = 0;
#pragma unroll 4
    for (int p = 0; p < kFieldParts; ++p) s += partial[f * kFieldParts + p];
    sums[f] = s;
}

// ---- clip -----------------------------------------------------------------------------------------------------------------------
struct ClipMulti {
    float* g[kMulti];
    int64_t n[kMulti];
    int sum_index[kMulti];
    int block_start[kMulti + 1];
    int count;
};

// what an element is turned into: `a` is c (value), max(n_v, c) (norm) or the scale s (global)
__device__ __forceinline__ float clip_one(float g, int mode, float c, float a) {
#pragma clang fp contract(off)
    if (mode == DT_CLIP_VALUE) return g < -c ? -c : (g > c ? c : g);
    if (mode == DT_CLIP_NORM) {
        const float t = g * c;
        return t / a;
    }
    return g * a;
}

// all sums in index order, by one thread
__device__ __forceinline__ double sum_in_order(const double* __restrict__ sums, int n_sums) {
    double s = 0;
    for (int i = 0; i < n_sums; ++i) s += sums[i];
    return s;
}

// the second operand of clip_one; every thread of the block calls it (global mode: thread 0 adds, LDS hands it round)
__device__ __forceinline__ float clip_operand(int mode, float c, const double* __restrict__ sums, int n_sums, int index,
                                              double* sh) {
#pragma clang fp contract(off)
    if (mode == DT_CLIP_VALUE) return c;
    if (mode == DT_CLIP_NORM) {
        const float nv = (float)sqrt(sums[index]);
        return (nv > c || nv != nv) ? nv : c;              // max(n_v, c); a NaN norm stays one
    }
    if (threadIdx.x == 0) sh[0] = sum_in_order(sums, n_sums);
    __syncthreads();
    const float N = (float)sqrt(sh[0]);
    const float a = 1.0f / N, b = 1.0f / c;
    const float s = c * (a < b ? a : b);
    return s + (N - N);                                    // Keras: finite N: + 0; Inf / NaN: NaN
}

__global__ __launch_bounds__(kThreads) void k_grad_clip(ClipMulti d, int mode, float c, const double* __restrict__ sums, int n_sums) {
    __shared__ double sh[1];
    int t = 0;
    while (t + 1 < d.count && (int)blockIdx.x >= d.block_start[t + 1]) ++t;
    const float a = clip_operand(mode, c, sums, n_sums, d.sum_index[t], sh);
    const int64_t lo = (int64_t)(blockIdx.x - d.block_start[t]) * kElems;
    const int64_t rest = d.n[t] - lo;
    const int m = rest < kElems ? (int)rest : kElems;
    float* __restrict__ g = d.g[t] + lo;
    const int nv = (reinterpret_cast<uintptr_t>(g) & 15) == 0 ? m / 4 : 0;
    for (int i = threadIdx.x; i < nv; i += kThreads) {
        float4 q = reinterpret_cast<float4*>(g)[i];
        q.x = clip_one(q.x, mode, c, a);
        q.y = clip_one(q.y, mode, c, a);
        q.z = clip_one(q.z, mode, c, a);
        q.w = clip_one(q.w, mode, c, a);
        reinterpret_cast<float4*>(g)[i] = q;
    }
    for (int i = nv * 4 + threadIdx.x; i < m; i += kThreads) g[i] = clip_one(g[i], mode, c, a);
}

__global__ __launch_bounds__(kThreads) void k_rows_clip(int mode, float c, const int64_t* __restrict__ out_rows,
                                                        float* __restrict__ out_vals, int64_t n, int D,
                                                        const int64_t* __restrict__ count, const int64_t* __restrict__ row_offset,
                                                        int F, const double* __restrict__ sums, int sum_base, int n_sums) {
    __shared__ double sh[1];
    __shared__ int64_t s_off[kFieldsInLds];                // DT_CLIP_NORM, F <= kFieldsInLds: the fields' first rows ...
    __shared__ float s_op[kFieldsInLds];                   // ... and max(n_v, c) of each, worked out once per block
    const float all = clip_operand(mode == DT_CLIP_NORM ? DT_CLIP_VALUE : mode, c, sums, n_sums, 0, sh);
    const bool staged = mode == DT_CLIP_NORM && F <= kFieldsInLds;
    if (staged) {
        for (int f = threadIdx.x; f < F; f += kThreads) {
            s_off[f] = row_offset[f];
            s_op[f] = clip_operand(DT_CLIP_NORM, c, sums, n_sums, sum_base + f, sh);
        }
        __syncthreads();
    }
    int64_t cnt = count[0];
    cnt = cnt < 0 ? 0 : (cnt > n ? n : cnt);
    const int64_t items = cnt * D;
    for (int64_t item = (int64_t)blockIdx.x * kThreads + threadIdx.x; item < items; item += (int64_t)gridDim.x * kThreads) {
        float a = all;
        if (mode == DT_CLIP_NORM) {
            const int64_t row = out_rows[item / D];
            int lo = 0, hi = F;                            // the last field whose first row is <= row
            while (hi - lo > 1) {
                const int mid = (lo + hi) / 2;
                if ((staged ? s_off[mid] : row_offset[mid]) <= row) lo = mid; else hi = mid;
            }
            a = staged ? s_op[lo] : clip_operand(DT_CLIP_NORM, c, sums, n_sums, sum_base + lo, sh);
        }
        out_vals[item] = clip_one(out_vals[item], mode, c, a);
    }
}

__global__ void k_clip_norm_out(int mode, const double* __restrict__ sums, int n_sums, double* __restrict__ norm_out) {
    if (threadIdx.x == 0 && blockIdx.x == 0) norm_out[0] = mode == DT_CLIP_VALUE ? 0.0 : sqrt(sum_in_order(sums, n_sums));
}

inline bool clip_args_ok(int mode, float c) {
    return mode >= DT_CLIP_VALUE && mode <= DT_CLIP_GLOBAL_NORM && c > 0.f && c <= 3.402823466e38f;       // (false for a NaN)
}

}  // namespace
}  // namespace dt

using namespace dt;

extern "C" int dt_rows_coalesce_chunk(void) { return kChunk; }

extern "C" int64_t dt_rows_coalesce_workspace_bytes(int64_t n, int D) {
    DT_REQUIRE(n >= 0 && n < kMaxN, "dt_rows_coalesce_workspace_bytes: n = %lld outside [0, 2^31)", (long long)n);
    DT_REQUIRE(D >= 1 && D <= kMaxD, "dt_rows_coalesce_workspace_bytes: D = %d outside [1, %d]", D, kMaxD);
    return co_ws_bytes(n, D);
}

extern "C" int dt_rows_coalesce(const int64_t* rows, const float* values, int64_t n, int D, int64_t V, int64_t* out_rows,
                                float* out_vals, int64_t* count, void* ws, void* stream) {
    DT_REQUIRE(n >= 0 && n < kMaxN, "dt_rows_coalesce: n = %lld outside [0, 2^31)", (long long)n);
    DT_REQUIRE(D >= 1 && D <= kMaxD, "dt_rows_coalesce: D = %d outside [1, %d]", D, kMaxD);
    DT_REQUIRE(V >= 1 && V <= kMaxV, "dt_rows_coalesce: V = %lld: row ids must be below 2^32 - 1 (32-bit sort keys)", (long long)V);
    DT_REQUIRE(count && aligned(count, 8), "dt_rows_coalesce: null or misaligned count");
    hipStream_t st = as_stream(stream);
    if (n == 0) {
        if (hipMemsetAsync(count, 0, sizeof(int64_t), st) != hipSuccess) return launch_status("dt_rows_coalesce");
        return DT_OK;
    }
    DT_REQUIRE(rows && values && out_rows && out_vals, "dt_rows_coalesce: null pointer");
    DT_REQUIRE(aligned(rows, 8) && aligned(out_rows, 8), "dt_rows_coalesce: rows / out_rows are not 8-byte aligned");
    DT_REQUIRE(aligned(values, 4) && aligned(out_vals, 4), "dt_rows_coalesce: values / out_vals are not 4-byte aligned");
    DT_REQUIRE(ws, "dt_rows_coalesce: null workspace (dt_rows_coalesce_workspace_bytes)");
    DT_REQUIRE(aligned(ws, 16), "dt_rows_coalesce: the workspace is not 16-byte aligned");
    const CoWs c = co_ws(ws, n);
    const int64_t tiles = tiles_of(n), chunks = chunks_of(n);
    const bool vec = D % 4 == 0 && aligned(values, 16) && aligned(out_vals, 16);        // (the partials are 256-byte aligned)
    hipLaunchKernelGGL(k_co_keys, dim3(stride_blocks(n)), dim3(kThreads), 0, st, rows, n, V, c.keys, c.pos);
    const int rc = dt_metric_sort_pairs(c.keys, c.pos, n, c.keys, c.pos, c.sort_ws, stream);
    if (rc != DT_OK) return rc;
    hipLaunchKernelGGL(k_co_tile_counts, dim3((unsigned)tiles), dim3(kThreads), 0, st, (const uint32_t*)c.keys, n, c.tile_heads,
                       c.tile_valid);
    hipLaunchKernelGGL(k_co_tile_scan, dim3(1), dim3(kThreads), 0, st, c.tile_heads, (const uint32_t*)c.tile_valid, tiles, c.meta,
                       count);
    hipLaunchKernelGGL(k_co_apply, dim3((unsigned)tiles), dim3(kThreads), 0, st, (const uint32_t*)c.keys, n,
                       (const uint32_t*)c.tile_heads, (const uint32_t*)c.meta, c.seg_start, c.seg_of, out_rows);
    const int64_t items = n * (vec ? D / 4 : D);
    if (vec) {
        hipLaunchKernelGGL(k_co_chunk_sum<true>, dim3((unsigned)chunks), dim3(kThreads), 0, st, (const uint32_t*)c.seg_of,
                           (const uint32_t*)c.seg_start, (const uint32_t*)c.meta, (const uint32_t*)c.pos, values, D, n, out_vals,
                           c.partial);
        hipLaunchKernelGGL(k_co_final<true>, dim3(stride_blocks(items)), dim3(kThreads), 0, st, (const uint32_t*)c.seg_start,
                           (const uint32_t*)c.meta, (const float*)c.partial, D, n, out_vals);
    } else {
        hipLaunchKernelGGL(k_co_chunk_sum<false>, dim3((unsigned)chunks), dim3(kThreads), 0, st, (const uint32_t*)c.seg_of,
                           (const uint32_t*)c.seg_start, (const uint32_t*)c.meta, (const uint32_t*)c.pos, values, D, n, out_vals,
                           c.partial);
        hipLaunchKernelGGL(k_co_final<false>, dim3(stride_blocks(items)), dim3(kThreads), 0, st, (const uint32_t*)c.seg_start,
                           (const uint32_t*)c.meta, (const float*)c.partial, D, n, out_vals);
    }
    return launch_status("dt_rows_coalesce");
}

extern "C" int64_t dt_grad_sumsq_workspace_bytes(int count, const int64_t* n) {
    if (count < 0 || (count > 0 && !n)) return DT_ERR_INVALID_ARG;
    int64_t blocks = 0;
    for (int t = 0; t < count; ++t) {
        if (n[t] < 0 || n[t] >= kMaxElems) return DT_ERR_INVALID_ARG;
        blocks += elem_blocks(n[t]);
    }
    return (blocks > 0 ? blocks : 1) * (int64_t)sizeof(double);
}

extern "C" int dt_grad_sumsq(int count, const float* const* g, const int64_t* n, double* sums, void* ws, void* stream) {
    DT_REQUIRE(count >= 0, "dt_grad_sumsq: negative tensor count %d", count);
    if (count == 0) return DT_OK;
    DT_REQUIRE(g && n, "dt_grad_sumsq: null descriptor array");
    DT_REQUIRE(sums && aligned(sums, 8), "dt_grad_sumsq: null or misaligned sums");
    int64_t all_blocks = 0;
    for (int t = 0; t < count; ++t) {                     // everything is validated before the first launch
        DT_REQUIRE(n[t] >= 0 && n[t] < kMaxElems, "dt_grad_sumsq: tensor %d: bad size %lld", t, (long long)n[t]);
        DT_REQUIRE(n[t] == 0 || g[t], "dt_grad_sumsq: tensor %d: null pointer with n > 0", t);
        DT_REQUIRE(n[t] == 0 || aligned(g[t], 4), "dt_grad_sumsq: tensor %d: misaligned pointer", t);
        all_blocks += elem_blocks(n[t]);
    }
    DT_REQUIRE(all_blocks < kMaxN, "dt_grad_sumsq: %lld chunks in one call", (long long)all_blocks);
    DT_REQUIRE(all_blocks == 0 || (ws && aligned(ws, 8)), "dt_grad_sumsq: null or misaligned workspace");
    hipStream_t st = as_stream(stream);
    double* partial = reinterpret_cast<double*>(ws);
    int64_t done = 0;
    for (int c0 = 0; c0 < count; c0 += kMulti) {
        SumsqMulti d;
        d.count = 0;
        int blocks = 0;
        for (int t = c0; t < count && t < c0 + kMulti; ++t) {
            const int k = d.count++;
            d.x[k] = g[t]; d.n[k] = n[t];
            d.block_start[k] = blocks;
            blocks += (int)elem_blocks(n[t]);
        }
        d.block_start[d.count] = blocks;
        if (blocks > 0) hipLaunchKernelGGL(k_sumsq_partial, dim3(blocks), dim3(kThreads), 0, st, d, partial + done);
        hipLaunchKernelGGL(k_sumsq_total, dim3(d.count), dim3(kThreads), 0, st, d, (const double*)(partial + done), sums + c0);
        done += blocks;
    }
    return launch_status("dt_grad_sumsq");
}

extern "C" int dt_rows_field_sumsq(const int64_t* out_rows, const float* out_vals, int64_t n, int D, const int64_t* count,
                                   const int64_t* row_offset, int F, int64_t V, double* sums, void* ws, void* stream) {
    DT_REQUIRE(n >= 0 && n < kMaxN, "dt_rows_field_sumsq: n = %lld outside [0, 2^31)", (long long)n);
    DT_REQUIRE(D >= 1 && D <= kMaxD, "dt_rows_field_sumsq: D = %d outside [1, %d]", D, kMaxD);
    DT_REQUIRE(F >= 1 && F <= (1 << 20), "dt_rows_field_sumsq: F = %d outside [1, 2^20]", F);
    DT_REQUIRE(V >= 1 && V <= kMaxV, "dt_rows_field_sumsq: V = %lld outside [1, 2^32 - 1]", (long long)V);
    DT_REQUIRE(count && row_offset && sums, "dt_rows_field_sumsq: null pointer");
    DT_REQUIRE(aligned(count, 8) && aligned(row_offset, 8) && aligned(sums, 8), "dt_rows_field_sumsq: misaligned count / row_offset / sums");
    DT_REQUIRE(n == 0 || (out_rows && out_vals), "dt_rows_field_sumsq: null pointer");
    DT_REQUIRE(aligned(out_rows, 8) && aligned(out_vals, 4), "dt_rows_field_sumsq: misaligned out_rows / out_vals");
    DT_REQUIRE(ws && aligned(ws, 8), "dt_rows_field_sumsq: null or misaligned workspace (F * DT_FIELD_SUMSQ_PARTS doubles)");
    double* partial = reinterpret_cast<double*>(ws);
    hipLaunchKernelGGL(k_field_partial, dim3((unsigned)F * kFieldParts), dim3(kThreads), 0, as_stream(stream), out_rows, out_vals, n,
                       D, count, row_offset, F, V, partial);
    hipLaunchKernelGGL(k_field_total, dim3((unsigned)ceil_div(F, kThreads)), dim3(kThreads), 0, as_stream(stream),
                       (const double*)partial, F, sums);
    return launch_status("dt_rows_field_sumsq");
}

extern "C" int dt_grad_clip(int mode, float c, int count, float* const* g, const int64_t* n, const int* sum_index,
                            const double* sums, int n_sums, double* norm_out, void* stream) {
    DT_REQUIRE(clip_args_ok(mode, c), "dt_grad_clip: mode %d / c = %g: the mode is DT_CLIP_*, c a finite number > 0", mode, (double)c);
    DT_REQUIRE(count >= 0 && n_sums >= 0, "dt_grad_clip: negative count %d / n_sums %d", count, n_sums);
    DT_REQUIRE(count == 0 || (g && n), "dt_grad_clip: null descriptor array");
    DT_REQUIRE(mode == DT_CLIP_VALUE || (sums && aligned(sums, 8)), "dt_grad_clip: null or misaligned sums");
    DT_REQUIRE(mode != DT_CLIP_NORM || count == 0 || sum_index, "dt_grad_clip: DT_CLIP_NORM without sum_index");
    DT_REQUIRE(aligned(norm_out, 8), "dt_grad_clip: misaligned norm_out");
    int64_t all_blocks = 0;
    for (int t = 0; t < count; ++t) {
        DT_REQUIRE(n[t] >= 0 && n[t] < kMaxElems, "dt_grad_clip: tensor %d: bad size %lld", t, (long long)n[t]);
        DT_REQUIRE(n[t] == 0 || g[t], "dt_grad_clip: tensor %d: null pointer with n > 0", t);
        DT_REQUIRE(n[t] == 0 || aligned(g[t], 4), "dt_grad_clip: tensor %d: misaligned pointer", t);
        DT_REQUIRE(mode != DT_CLIP_NORM || (sum_index[t] >= 0 && sum_index[t] < n_sums),
                   "dt_grad_clip: tensor %d: sum_index %d outside [0, %d)", t, mode == DT_CLIP_NORM ? sum_index[t] : 0, n_sums);
        all_blocks += elem_blocks(n[t]);
    }
    DT_REQUIRE(all_blocks < kMaxN, "dt_grad_clip: %lld chunks in one call", (long long)all_blocks);
    hipStream_t st = as_stream(stream);
    if (norm_out) hipLaunchKernelGGL(k_clip_norm_out, dim3(1), dim3(kWave), 0, st, mode, sums, n_sums, norm_out);
    for (int c0 = 0; c0 < count; c0 += kMulti) {
        ClipMulti d;
        d.count = 0;
        int blocks = 0;
        for (int t = c0; t < count && t < c0 + kMulti; ++t) {
            if (n[t] == 0) continue;
            const int k = d.count++;
            d.g[k] = g[t]; d.n[k] = n[t]; d.sum_index[k] = mode == DT_CLIP_NORM ? sum_index[t] : 0;
            d.block_start[k] = blocks;
            blocks += (int)elem_blocks(n[t]);
        }
        d.block_start[d.count] = blocks;
        if (blocks == 0) continue;
        hipLaunchKernelGGL(k_grad_clip, dim3(blocks), dim3(kThreads), 0, st, d, mode, c, sums, n_sums);
    }
    return launch_status("dt_grad_clip");
}

extern "C" int dt_rows_clip(int mode, float c, const int64_t* out_rows, float* out_vals, int64_t n, int D, const int64_t* count,
                            const int64_t* row_offset, int F, int64_t V, const double* sums, int sum_base, int n_sums,
                            double* norm_out, void* stream) {
    DT_REQUIRE(clip_args_ok(mode, c), "dt_rows_clip: mode %d / c = %g: the mode is DT_CLIP_*, c a finite number > 0", mode, (double)c);
    DT_REQUIRE(n >= 0 && n < kMaxN, "dt_rows_clip: n = %lld outside [0, 2^31)", (long long)n);
    DT_REQUIRE(D >= 1 && D <= kMaxD, "dt_rows_clip: D = %d outside [1, %d]", D, kMaxD);
    DT_REQUIRE(F >= 1 && F <= (1 << 20), "dt_rows_clip: F = %d outside [1, 2^20]", F);
    DT_REQUIRE(V >= 1 && V <= kMaxV, "dt_rows_clip: V = %lld outside [1, 2^32 - 1]", (long long)V);
    DT_REQUIRE(n_sums >= 0 && sum_base >= 0, "dt_rows_clip: negative n_sums %d / sum_base %d", n_sums, sum_base);
    DT_REQUIRE(mode == DT_CLIP_VALUE || (sums && aligned(sums, 8)), "dt_rows_clip: null or misaligned sums");
    DT_REQUIRE(mode != DT_CLIP_NORM || (int64_t)sum_base + F <= n_sums, "dt_rows_clip: sum_base %d + F %d > n_sums %d", sum_base, F,
               n_sums);
    DT_REQUIRE(mode != DT_CLIP_NORM || (row_offset && aligned(row_offset, 8)), "dt_rows_clip: null or misaligned row_offset");
    DT_REQUIRE(aligned(norm_out, 8), "dt_rows_clip: misaligned norm_out");
    DT_REQUIRE(n == 0 || (out_rows && out_vals && count), "dt_rows_clip: null pointer");
    DT_REQUIRE(aligned(out_rows, 8) && aligned(out_vals, 4) && aligned(count, 8), "dt_rows_clip: misaligned out_rows / out_vals / count");
    hipStream_t st = as_stream(stream);
    if (norm_out) hipLaunchKernelGGL(k_clip_norm_out, dim3(1), dim3(kWave), 0, st, mode, sums, n_sums, norm_out);
    if (n == 0) return launch_status("dt_rows_clip");
    hipLaunchKernelGGL(k_rows_clip, dim3(stride_blocks(n * D)), dim3(kThreads), 0, st, mode, c, out_rows, out_vals, n, D, count,
                       row_offset, F, sums, sum_base, n_sums);
    return launch_status("dt_rows_clip");
}
