// metrics.hip — epoch metrics on the device (gfx950, wave64): a stable LSD radix sort of (uint32 key, uint32 value) pairs,
// the exact binary ROC AUC on top of it, and the reductions behind accuracy / MSE / MAE.
//
// Replaces the end of every epoch of DeepModel.fit / evaluate (deepmodel.py: concatenate the outputs, copy them to the host,
// sklearn.metrics.roc_auc_score = one single-threaded host sort).  Everything below is integer or fixed-order arithmetic, so
// a call's result is bit-reproducible from run to run.
//
// No block ever waits for another block: there is no look-back, no grid barrier and no flag to spin on.  Whatever one block
// needs from the others (digit counts, tile sums) was written by an EARLIER launch, and every loop is bounded by n.
//
// Sort: 8-bit digits, 4 passes, each pass three launches over tiles of kTile consecutive elements:
//   k_sort_hist     counts[digit][tile] (LDS histogram) and totals[pass][digit] (integer atomics: order-independent)
//   k_sort_scan     block d: base = sum of totals[< d], then the exclusive scan of row d of counts -> global offsets
//   k_sort_scatter  wave w of a tile owns the w-th quarter of it; after the waves' own digit counts are known every wave
//                   has its start per digit, and walks its quarter 64 elements at a time: the rank of an element is the
//                   number of LOWER lanes with the same digit (8 __ballot rounds, 64-bit masks) plus the wave's running
//                   counter of that digit in LDS.  Equal digits therefore keep their input order: the pass is stable.
// AUC (k_auc_*): keys = order-preserving uint32 of the score (-0.0 -> +0.0 first), values = 1 for label 1, else 0; after the
//   sort a reduce-then-scan over tiles (three launches) gives, for every group of equal keys, where it starts and how many
//   negatives precede it; one thread per group then adds pos_g * (2 * negs_before_g + neg_g) into U2 (64-bit integers).
// Sums (k_sums_partial, k_score_*, k_ap_partial; dt_metric_sums, dt_score_*): the hit count with the squared and absolute
//   errors, log loss with the precision / recall counts, MSLE / MAPE, top-k hits with the categorical cross-entropy, and
//   average precision from the AUC's group arrays — float64 from the float32 inputs.  One scheme for all of them: a block
//   writes its partial words behind the result words (score_partial), and k_score_final, one block, adds them in block order.
#include "common.h"

namespace dt {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr int kItems = 16;                      // elements per thread and tile
constexpr int kTile = kThreads * kItems;        // 4096: dt_metric_sort_tile()
constexpr int kWaveSpan = kTile / kWaves;       // consecutive elements one wave of the scatter owns
constexpr int kRounds = kWaveSpan / kWave;
constexpr int kDigits = 256;
constexpr int kPasses = 4;
constexpr int kMaxBlocks = 2048;                // grid-stride kernels
constexpr int64_t kMaxN = (int64_t)1 << 31;

typedef unsigned long long u64;

inline int64_t a256(int64_t b) { return (b + 255) & ~(int64_t)255; }
inline int64_t tiles_of(int64_t n) { return (n + kTile - 1) / kTile; }

// ---- block helpers (kThreads threads; every thread of the block calls them) ----------------------------------------------
template <typename T>
__device__ __forceinline__ T wave_incl_scan(T v, int lane) {
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
        const T t = __shfl_up(v, o, kWave);
        if (lane >= o) v += t;
    }
    return v;
}
// exclusive scan over the block in thread order; *total = the block's sum.  sh: kWaves words of LDS, free again on return
template <typename T>
__device__ __forceinline__ T block_excl_scan(T v, T* total, T* sh) {
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const T incl = wave_incl_scan(v, lane);
    if (lane == kWave - 1) sh[wave] = incl;
    __syncthreads();
    T before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
        const T s = sh[w];
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

// ---- sort ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_sort_hist(const uint32_t* __restrict__ keys, int64_t n, int64_t tiles, int shift,
                                                        uint32_t* __restrict__ counts, uint32_t* __restrict__ totals) {
    __shared__ uint32_t h[kDigits];
    const int64_t tile = blockIdx.x;
    h[threadIdx.x] = 0;
    __syncthreads();
    const int64_t base = tile * kTile;
#pragma unroll 4
    for (int j = 0; j < kItems; ++j) {
        const int64_t i = base + j * kThreads + threadIdx.x;
        if (i < n) atomicAdd(&h[(keys[i] >> shift) & (kDigits - 1)], 1u);
    }
    __syncthreads();
    const uint32_t c = h[threadIdx.x];
    counts[(int64_t)threadIdx.x * tiles + tile] = c;
    if (c) atomicAdd(&totals[threadIdx.x], c);
}

// grid = kDigits blocks; block d turns row d of counts into the global start of (digit d, tile t)
__global__ __launch_bounds__(kThreads) void k_sort_scan(uint32_t* __restrict__ counts, const uint32_t* __restrict__ totals,
                                                        int64_t tiles) {
    __shared__ uint32_t sh[kWaves];
    const int d = blockIdx.x;
    uint32_t carry = block_sum<uint32_t>((int)threadIdx.x < d ? totals[threadIdx.x] : 0u, sh);
    uint32_t* row = counts + (int64_t)d * tiles;
    for (int64_t c0 = 0; c0 < tiles; c0 += kThreads * 4) {
        const int64_t j0 = c0 + (int64_t)threadIdx.x * 4;
        uint32_t v[4], s = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            v[k] = j0 + k < tiles ? row[j0 + k] : 0u;
            s += v[k];
        }
        uint32_t all;
        uint32_t run = carry + block_excl_scan<uint32_t>(s, &all, sh);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (j0 + k < tiles) row[j0 + k] = run;
            run += v[k];
        }
        carry += all;
    }
}

__global__ __launch_bounds__(kThreads) void k_sort_scatter(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ vals,
                                                           uint32_t* __restrict__ keys_out, uint32_t* __restrict__ vals_out,
                                                           const uint32_t* __restrict__ offsets, int64_t n, int64_t tiles,
                                                           int shift) {
    __shared__ uint32_t cnt[kWaves][kDigits];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const int64_t tile = blockIdx.x;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) cnt[w][threadIdx.x] = 0;
    __syncthreads();
    const int64_t base = tile * kTile + (int64_t)wave * kWaveSpan;
    for (int r = 0; r < kRounds; ++r) {
        const int64_t i = base + r * kWave + lane;
        if (i < n) atomicAdd(&cnt[wave][(keys[i] >> shift) & (kDigits - 1)], 1u);
    }
    __syncthreads();
    {   // thread = digit: where each wave's elements of this digit start
        uint32_t off = offsets[(int64_t)threadIdx.x * tiles + tile];
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            const uint32_t c = cnt[w][threadIdx.x];
            cnt[w][threadIdx.x] = off;
            off += c;
        }
    }
    __syncthreads();
    // the wave's own counters from here on: one wave's LDS operations complete in program order, volatile keeps that order
    volatile uint32_t* mine = cnt[wave];
    const u64 below = ((u64)1 << lane) - 1;
    for (int r = 0; r < kRounds; ++r) {
        const int64_t i = base + r * kWave + lane;
        const bool valid = i < n;
        const uint32_t key = valid ? keys[i] : 0u;
        const uint32_t val = valid ? vals[i] : 0u;
        const uint32_t d = (key >> shift) & (kDigits - 1);
        u64 peers = __ballot(valid);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const bool bit = (d >> b) & 1u;
            const u64 m = __ballot(bit);
            peers &= bit ? m : ~m;
        }
        if (valid) {
            const uint32_t pos = mine[d] + (uint32_t)__popcll(peers & below);
            if ((peers >> lane) == 1) mine[d] = pos + 1;        // the highest lane of the group holds its last element
            if ((int64_t)pos < n) {
                keys_out[pos] = key;
                vals_out[pos] = val;
            }
        }
    }
}

int sort_pairs(const uint32_t* keys, const uint32_t* vals, int64_t n, uint32_t* keys_out, uint32_t* vals_out, void* ws,
               hipStream_t st, const char* what) {
    const int64_t tiles = tiles_of(n);
    char* w = reinterpret_cast<char*>(ws);
    uint32_t* tkeys = reinterpret_cast<uint32_t*>(w);
    uint32_t* tvals = reinterpret_cast<uint32_t*>(w + a256(4 * n));
    uint32_t* counts = reinterpret_cast<uint32_t*>(w + 2 * a256(4 * n));
    uint32_t* totals = reinterpret_cast<uint32_t*>(w + 2 * a256(4 * n) + a256(4 * kDigits * tiles));
    if (hipMemsetAsync(totals, 0, sizeof(uint32_t) * kPasses * kDigits, st) != hipSuccess) return launch_status(what);
    const uint32_t *ik = keys, *iv = vals;
    for (int p = 0; p < kPasses; ++p) {
        uint32_t* ok = (p & 1) ? keys_out : tkeys;       // in -> tmp -> out -> tmp -> out
        uint32_t* ov = (p & 1) ? vals_out : tvals;
        hipLaunchKernelGGL(k_sort_hist, dim3((unsigned)tiles), dim3(kThreads), 0, st, ik, n, tiles, 8 * p, counts,
                           totals + p * kDigits);
        hipLaunchKernelGGL(k_sort_scan, dim3(kDigits), dim3(kThreads), 0, st, counts, totals + p * kDigits, tiles);
        hipLaunchKernelGGL(k_sort_scatter, dim3((unsigned)tiles), dim3(kThreads), 0, st, ik, iv, ok, ov, counts, n, tiles,
                           8 * p);
        ik = ok;
        iv = ov;
    }
    return launch_status(what);
}

int64_t sort_ws_bytes(int64_t n) { return 2 * a256(4 * n) + a256(4 * kDigits * tiles_of(n)) + a256(4 * kPasses * kDigits); }

// ---- AUC ----------------------------------------------------------------------------------------------------------------
// out5: U2, P, N, nonfinite, bad_label
__global__ __launch_bounds__(kThreads) void k_auc_keys(const float* __restrict__ score, const float* __restrict__ label,
                                                       int64_t n, uint32_t* __restrict__ keys, uint32_t* __restrict__ vals,
                                                       u64* __restrict__ out5) {
    __shared__ uint32_t sh[kWaves];
    uint32_t pos = 0, neg = 0, nonfinite = 0, bad = 0;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) {
        uint32_t b = __float_as_uint(score[i]);
        if ((b & 0x7f800000u) == 0x7f800000u) ++nonfinite;
        if (b == 0x80000000u) b = 0;
        keys[i] = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
        const float y = label[i];
        const uint32_t is_pos = y == 1.0f;
        if (!is_pos && !(y == 0.0f)) ++bad;
        vals[i] = is_pos;
        pos += is_pos;
        neg += 1u - is_pos;
    }
    // a thread sees at most n / kThreads + 1 elements: 32 bits hold the block's counts
    pos = block_sum<uint32_t>(pos, sh);
    neg = block_sum<uint32_t>(neg, sh);
    nonfinite = block_sum<uint32_t>(nonfinite, sh);
    bad = block_sum<uint32_t>(bad, sh);
    if (threadIdx.x == 0) {
        if (pos) atomicAdd(&out5[1], (u64)pos);
        if (neg) atomicAdd(&out5[2], (u64)neg);
        if (nonfinite) atomicAdd(&out5[3], (u64)nonfinite);
        if (bad) atomicAdd(&out5[4], (u64)bad);
    }
}

// (negatives << 32 | group starts) of the kItems consecutive elements of a thread; flags: bit j = element j starts a group,
// bit 16 + j = element j is a negative
__device__ __forceinline__ u64 auc_thread_items(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ vals,
                                                int64_t i0, int64_t n, uint32_t* flags) {
    uint32_t prev = (i0 > 0 && i0 <= n) ? keys[i0 - 1] : 0u;
    uint32_t negs = 0, starts = 0, f = 0;
#pragma unroll
    for (int j = 0; j < kItems; ++j) {
        const int64_t i = i0 + j;
        if (i < n) {
            const uint32_t k = keys[i];
            const uint32_t start = (i == 0) || (k != prev);
            const uint32_t neg = vals[i] == 0u;
            f |= (start << j) | (neg << (16 + j));
            starts += start;
            negs += neg;
            prev = k;
        }
    }
    *flags = f;
    return ((u64)negs << 32) | starts;
}

__global__ __launch_bounds__(kThreads) void k_auc_tile_sums(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ vals,
                                                            int64_t n, u64* __restrict__ tile_sums) {
    __shared__ u64 sh[kWaves];
    uint32_t flags;
    const int64_t i0 = (int64_t)blockIdx.x * kTile + (int64_t)threadIdx.x * kItems;
    const u64 s = block_sum<u64>(auc_thread_items(keys, vals, i0, n, &flags), sh);
    if (threadIdx.x == 0) tile_sums[blockIdx.x] = s;
}

// one block: tile_sums -> exclusive prefix; meta[0] = groups, meta[1] = negatives
__global__ __launch_bounds__(kThreads) void k_auc_tile_scan(u64* __restrict__ tile_sums, int64_t tiles, uint32_t* __restrict__ meta) {
    __shared__ u64 sh[kWaves];
    u64 carry = 0;
    for (int64_t c0 = 0; c0 < tiles; c0 += kThreads) {
        const int64_t j = c0 + threadIdx.x;
        const u64 v = j < tiles ? tile_sums[j] : 0;
        u64 all;
        const u64 e = carry + block_excl_scan<u64>(v, &all, sh);
        if (j < tiles) tile_sums[j] = e;
        carry += all;
    }
    if (threadIdx.x == 0) {
        meta[0] = (uint32_t)carry;
        meta[1] = (uint32_t)(carry >> 32);
    }
}

// every group start i -> group_start[g] = i, group_negs_before[g] = negatives among [0, i)
__global__ __launch_bounds__(kThreads) void k_auc_groups(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ vals,
                                                         int64_t n, const u64* __restrict__ tile_prefix,
                                                         uint32_t* __restrict__ group_start, uint32_t* __restrict__ group_negs_before) {
    __shared__ u64 sh[kWaves];
    uint32_t flags;
    const int64_t i0 = (int64_t)blockIdx.x * kTile + (int64_t)threadIdx.x * kItems;
    const u64 mine = auc_thread_items(keys, vals, i0, n, &flags);
    u64 all;
    const u64 e = tile_prefix[blockIdx.x] + block_excl_scan<u64>(mine, &all, sh);
    uint32_t g = (uint32_t)e, negs = (uint32_t)(e >> 32);
#pragma unroll
    for (int j = 0; j < kItems; ++j) {
        if ((flags >> j) & 1u) {
            if ((int64_t)g < n) {
                group_start[g] = (uint32_t)(i0 + j);
                group_negs_before[g] = negs;
            }
            ++g;
        }
        negs += (flags >> (16 + j)) & 1u;
    }
}

__global__ __launch_bounds__(kThreads) void k_auc_u2(const uint32_t* __restrict__ group_start, const uint32_t* __restrict__ group_negs_before,
                                                     const uint32_t* __restrict__ meta, int64_t n, u64* __restrict__ out5) {
    __shared__ u64 sh[kWaves];
    int64_t groups = meta[0];
    if (groups > n) groups = n;
    const uint32_t all_negs = meta[1];
    u64 u2 = 0;
    for (int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x; g < groups; g += (int64_t)gridDim.x * kThreads) {
        const uint32_t s = group_start[g], nb = group_negs_before[g];
        const uint32_t e = g + 1 < groups ? group_start[g + 1] : (uint32_t)n;
        const uint32_t nb1 = g + 1 < groups ? group_negs_before[g + 1] : all_negs;
        const u64 neg = nb1 - nb, pos = (u64)(e - s) - neg;
        u2 += pos * (2 * (u64)nb + neg);
    }
    u2 = block_sum<u64>(u2, sh);
    if (threadIdx.x == 0 && u2) atomicAdd(&out5[0], u2);
}

int64_t auc_ws_bytes(int64_t n) { return 2 * a256(4 * n) + sort_ws_bytes(n) + a256(8 * tiles_of(n)) + 256; }

inline bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }
inline unsigned stride_blocks(int64_t n) {
    const int64_t b = (n + kThreads - 1) / kThreads;
    return (unsigned)(b < kMaxBlocks ? b : kMaxBlocks);
}

// ---- the partial / final scheme of every float64 sum below -----------------------------------------------------------------
// A block adds what it saw in a fixed order and writes its partial words behind the result words of `out` (W result words,
// then W words per block); k_score_final, one block, adds the partials in block order.  The block count is a function of the
// shape alone, so the same input gives the same bits.
constexpr int kScoreBlocks = DT_SCORE_BLOCKS;
static_assert(kScoreBlocks <= kThreads, "k_score_final: one thread per partial");
static_assert(DT_METRIC_SUMS_BLOCKS == DT_SCORE_BLOCKS && DT_METRIC_SUMS_WORDS == 3 + 3 * kScoreBlocks &&
              DT_SCORE_BINARY_WORDS == 5 + 5 * kScoreBlocks && DT_SCORE_REGRESSION_WORDS == 2 + 2 * kScoreBlocks &&
              DT_SCORE_CATEGORICAL_WORDS == 2 + 2 * kScoreBlocks && DT_SCORE_RANKING_WORDS == 6 + kScoreBlocks, "out layouts");

// ceil(work / per_block) blocks, at most kScoreBlocks
inline int score_blocks(int64_t work, int64_t per_block) {
    const int64_t b = (work + per_block - 1) / per_block;
    return (int)(b < kScoreBlocks ? b : kScoreBlocks);
}

__device__ __forceinline__ void score_partial(u64* __restrict__ out, int W, int k, u64 v) { out[W + W * blockIdx.x + k] = v; }
__device__ __forceinline__ void score_partial(u64* __restrict__ out, int W, int k, double v) {
    out[W + W * blockIdx.x + k] = (u64)__double_as_longlong(v);
}

// NI integer words, then ND float64 words
template <int NI, int ND>
__global__ __launch_bounds__(kThreads) void k_score_final(u64* __restrict__ out, int blocks) {
    [[maybe_unused]] __shared__ u64 shi[kWaves];
    __shared__ double shd[kWaves];
    constexpr int W = NI + ND;
    const bool live = (int)threadIdx.x < blocks;          // blocks <= kScoreBlocks <= kThreads
    const u64* part = out + W + W * threadIdx.x;
#pragma unroll
    for (int k = 0; k < NI; ++k) {
        const u64 s = block_sum<u64>(live ? part[k] : 0, shi);
        if (threadIdx.x == 0) out[k] = s;
    }
#pragma unroll
    for (int k = NI; k < W; ++k) {
        const double s = block_sum<double>(live ? __longlong_as_double((long long)part[k]) : 0.0, shd);
        if (threadIdx.x == 0) out[k] = (u64)__double_as_longlong(s);
    }
}

// the class a `v > best` scan from class 0 ends on: the first maximum, as numpy.argmax (class 0 when the row leads with a NaN)
__device__ __forceinline__ int first_max(const float* __restrict__ row, int C) {
    int best = 0;
    float bv = row[0];
    for (int c = 1; c < C; ++c) {
        const float v = row[c];
        if (v > bv) { bv = v; best = c; }
    }
    return best;
}

// ---- accuracy / MSE / MAE -------------------------------------------------------------------------------------------------
// out: hits (int64), sum (p-y)^2, sum |p-y| (double)
__global__ __launch_bounds__(kThreads) void k_sums_partial(const float* __restrict__ y_true, const float* __restrict__ y_prob,
                                                           int64_t n, u64* __restrict__ out) {
    __shared__ u64 shi[kWaves];
    __shared__ double shd[kWaves];
    u64 hits = 0;
    double se = 0.0, ae = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) {
        const float p = y_prob[i], y = y_true[i];
        hits += (long long)(p > 0.5f) == (long long)y;
        const double d = (double)p - (double)y;
        se += d * d;
        ae += fabs(d);
    }
    hits = block_sum<u64>(hits, shi);
    se = block_sum<double>(se, shd);
    ae = block_sum<double>(ae, shd);
    if (threadIdx.x == 0) {
        score_partial(out, 3, 0, hits);
        score_partial(out, 3, 1, se);
        score_partial(out, 3, 2, ae);
    }
}

// rows whose argmax (first_max) equals the label; ONEHOT: the label is the argmax of the y_true row
template <int KIND>
__global__ __launch_bounds__(kThreads) void k_argmax_hits(const float* __restrict__ y_prob, const float* __restrict__ y_true,
                                                          int64_t n, int C, u64* __restrict__ out) {
    __shared__ uint32_t sh[kWaves];
    uint32_t hits = 0;
    for (int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x; r < n; r += (int64_t)gridDim.x * kThreads) {
        const int best = first_max(y_prob + r * C, C);
        if (KIND == DT_METRIC_Y_ONEHOT)
            hits += best == first_max(y_true + r * C, C);
        else
            hits += (float)best == y_true[r];
    }
    hits = block_sum<uint32_t>(hits, sh);
    if (threadIdx.x == 0 && hits) atomicAdd(out, (u64)hits);
}

// ---- scores: log loss, precision / recall counts, top-k hits, MSLE / MAPE, average precision -------------------------------
constexpr int kThreadRowMaxC = DT_SCORE_THREAD_ROW_MAX_C;     // a thread per row up to here, a wave per row beyond
constexpr double kClipLo = (double)1e-7f;                     // Keras' epsilon as float32 ...
constexpr double kClipHi = (double)(1.0f - 1e-7f);            // ... and 1 - epsilon, subtracted in float32 (0.99999988...)

// numpy.clip(p, lo, hi): a NaN fails both comparisons and comes out as it went in (fmin / fmax would drop it)
__device__ __forceinline__ double clip_prob(double p) { return p < kClipLo ? kClipLo : (p > kClipHi ? kClipHi : p); }
// numpy.maximum(x, lo), NaN kept
__device__ __forceinline__ double at_least_lo(double x) { return x < kClipLo ? kClipLo : x; }
__device__ __forceinline__ double quiet_nan() { return __longlong_as_double(0x7ff8000000000000LL); }
// the class a float label names, -1 when it names none of [0, C) (a NaN too)
__device__ __forceinline__ int label_class(float y, int C) { return (y >= 0.0f && (double)y < (double)C) ? (int)y : -1; }

// out: TP, FP, FN, TN (int64), sum of -(y log q + (1 - y) log(1 - q)) (double); LABELS: y = (class of the row == column)
template <int KIND>
__global__ __launch_bounds__(kThreads) void k_score_binary(const float* __restrict__ y_true, const float* __restrict__ y_prob,
                                                           int64_t total, int C, u64* __restrict__ out) {
    __shared__ uint32_t shc[kWaves];
    __shared__ double shd[kWaves];
    uint32_t tp = 0, fp = 0, fn = 0, tn = 0;
    double ce = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (int64_t)gridDim.x * kThreads) {
        const float pf = y_prob[i];
        double y;
        if (KIND == DT_METRIC_Y_LABELS) {
            const int64_t r = i / C;
            y = label_class(y_true[r], C) == (int)(i - r * C) ? 1.0 : 0.0;
        } else {
            y = (double)y_true[i];
        }
        const uint32_t pp = pf > 0.5f, yp = y != 0.0;
        tp += pp & yp;
        fp += pp & (yp ^ 1u);
        fn += (pp ^ 1u) & yp;
        tn += (pp ^ 1u) & (yp ^ 1u);
        const double q = clip_prob((double)pf);
        // a hard label makes one of the two products an exact zero (q is finite inside [lo, hi]): that logarithm is skipped
        const bool sane = q == q;
        const double a = (sane && y == 0.0) ? 0.0 : y * log(q);
        const double b = (sane && y == 1.0) ? 0.0 : (1.0 - y) * log(1.0 - q);
        ce += -(a + b);
    }
    // a thread sees at most total / kThreads + 1 elements: 32 bits hold the block's counts
    tp = block_sum<uint32_t>(tp, shc);
    fp = block_sum<uint32_t>(fp, shc);
    fn = block_sum<uint32_t>(fn, shc);
    tn = block_sum<uint32_t>(tn, shc);
    ce = block_sum<double>(ce, shd);
    if (threadIdx.x == 0) {
        score_partial(out, 5, 0, (u64)tp);
        score_partial(out, 5, 1, (u64)fp);
        score_partial(out, 5, 2, (u64)fn);
        score_partial(out, 5, 3, (u64)tn);
        score_partial(out, 5, 4, ce);
    }
}

// out: sum (log(max(p, lo) + 1) - log(max(y, lo) + 1))^2, sum |y - p| / max(|y|, lo)
__global__ __launch_bounds__(kThreads) void k_score_regression(const float* __restrict__ y_true, const float* __restrict__ y_pred,
                                                               int64_t n, u64* __restrict__ out) {
    __shared__ double shd[kWaves];
    double sl = 0.0, pe = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) {
        const double p = (double)y_pred[i], y = (double)y_true[i];
        const double d = log(at_least_lo(p) + 1.0) - log(at_least_lo(y) + 1.0);
        sl += d * d;
        pe += fabs(y - p) / at_least_lo(fabs(y));
    }
    sl = block_sum<double>(sl, shd);
    pe = block_sum<double>(pe, shd);
    if (threadIdx.x == 0) {
        score_partial(out, 2, 0, sl);
        score_partial(out, 2, 1, pe);
    }
}

// the row pass: out = rows whose target class is among the k best (int64), sum of the rows' categorical cross-entropy.
// target: the label, or the first_max of the one-hot row.
// A thread per row: every sum over the classes runs in class order.
template <int KIND>
__global__ __launch_bounds__(kThreads) void k_score_rows_thread(const float* __restrict__ y_prob, const float* __restrict__ y_true,
                                                                int64_t n, int C, int k, u64* __restrict__ out) {
    __shared__ uint32_t shc[kWaves];
    __shared__ double shd[kWaves];
    uint32_t hits = 0;
    double ce = 0.0;
    for (int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x; r < n; r += (int64_t)gridDim.x * kThreads) {
        const float* p = y_prob + r * C;
        const float* t = y_true + r * C;                 // (ONEHOT only)
        double s = 0.0;
        for (int c = 0; c < C; ++c) s += (double)p[c];
        const int target = KIND == DT_METRIC_Y_ONEHOT ? first_max(t, C) : label_class(y_true[r], C);
        if (target >= 0) {
            const float pt = p[target];
            int above = 0;
            for (int c = 0; c < C; ++c) above += p[c] > pt;
            hits += (pt == pt) && above < k;
        }
        if (KIND == DT_METRIC_Y_ONEHOT) {
            double acc = 0.0;
            for (int c = 0; c < C; ++c) {
                const double y = (double)t[c], q = clip_prob((double)p[c] / s);
                if (!(y == 0.0 && q == q)) acc += y * log(q);         // (0 * a finite logarithm: skipped)
            }
            ce += -acc;
        } else {
            ce += target >= 0 ? -log(clip_prob((double)p[target] / s)) : quiet_nan();
        }
    }
    hits = block_sum<uint32_t>(hits, shc);
    ce = block_sum<double>(ce, shd);
    if (threadIdx.x == 0) {
        score_partial(out, 2, 0, (u64)hits);
        score_partial(out, 2, 1, ce);
    }
}

// lane 0 gets partial[0] of: for o = 32, 16, ... 1: partial[l] += partial[l + o] for l < o
__device__ __forceinline__ double wave_tree_sum(double v) {
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) v += __shfl_down(v, o, kWave);
    return v;
}

// A wave per row, for wide rows: lane l takes classes l, l + 64, ... in that order, and the lanes' partial sums are added by
// wave_tree_sum.  Counts and the target class do not depend on the order.
template <int KIND>
__global__ __launch_bounds__(kThreads) void k_score_rows_wave(const float* __restrict__ y_prob, const float* __restrict__ y_true,
                                                              int64_t n, int C, int k, u64* __restrict__ out) {
    __shared__ uint32_t shc[kWaves];
    __shared__ double shd[kWaves];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    constexpr int kNone = 0x7fffffff;
    uint32_t hits = 0;          // lane 0 of every wave counts for its rows
    double ce = 0.0;
    for (int64_t r = (int64_t)blockIdx.x * kWaves + wave; r < n; r += (int64_t)gridDim.x * kWaves) {
        const float* p = y_prob + r * C;
        const float* t = y_true + r * C;                 // (ONEHOT only)
        double s = 0.0;
        for (int c = lane; c < C; c += kWave) s += (double)p[c];
        s = __shfl(wave_tree_sum(s), 0, kWave);
        int target;
        if (KIND == DT_METRIC_Y_ONEHOT) {
            // the scan's answer without the scan: class 0 if t[0] is a NaN, else the lowest class holding the largest non-NaN value
            int bi = kNone;
            float bv = 0.f;
            for (int c = lane; c < C; c += kWave) {
                const float v = t[c];
                if (v == v && (bi == kNone || v > bv)) { bv = v; bi = c; }
            }
#pragma unroll
            for (int o = kWave / 2; o > 0; o >>= 1) {
                const float ov = __shfl_down(bv, o, kWave);
                const int oi = __shfl_down(bi, o, kWave);
                if (oi != kNone && (bi == kNone || ov > bv || (ov == bv && oi < bi))) { bv = ov; bi = oi; }
            }
            target = __shfl(bi, 0, kWave);
            const float t0 = t[0];
            if (target == kNone || t0 != t0) target = 0;
        } else {
            target = label_class(y_true[r], C);
        }
        bool hit = false;
        if (target >= 0) {
            const float pt = p[target];
            int above = 0;
            for (int c = lane; c < C; c += kWave) above += p[c] > pt;
#pragma unroll
            for (int o = kWave / 2; o > 0; o >>= 1) above += __shfl_down(above, o, kWave);
            hit = (pt == pt) && above < k;      // (lane 0's `above` is the row's)
        }
        double loss;
        if (KIND == DT_METRIC_Y_ONEHOT) {
            double acc = 0.0;
            for (int c = lane; c < C; c += kWave) {
                const double y = (double)t[c], q = clip_prob((double)p[c] / s);
                if (!(y == 0.0 && q == q)) acc += y * log(q);
            }
            loss = -wave_tree_sum(acc);
        } else {
            loss = target >= 0 ? -log(clip_prob((double)p[target] / s)) : quiet_nan();
        }
        if (lane == 0) {
            hits += hit;
            ce += loss;
        }
    }
    if (lane != 0) ce = 0.0;
    hits = block_sum<uint32_t>(hits, shc);
    ce = block_sum<double>(ce, shd);
    if (threadIdx.x == 0) {
        score_partial(out, 2, 0, (u64)hits);
        score_partial(out, 2, 1, ce);
    }
}

// average precision over the groups k_auc_groups compacted (ascending score): group g holds pos_g positives, TPcum = the
// positives at or above it, n - start = everything at or above it.  out6: dt_metric_auc's five words (P is complete: an
// earlier launch counted it), then from word 5 on the scheme's one float64 word: the sum of pos_g * TPcum / (n - start).
__global__ __launch_bounds__(kThreads) void k_ap_partial(const uint32_t* __restrict__ group_start, const uint32_t* __restrict__ group_negs_before,
                                                         const uint32_t* __restrict__ meta, int64_t n, u64* __restrict__ out6) {
    __shared__ double shd[kWaves];
    int64_t groups = meta[0];
    if (groups > n) groups = n;
    const uint32_t all_negs = meta[1];
    const u64 P = out6[1];
    double acc = 0.0;
    for (int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x; g < groups; g += (int64_t)gridDim.x * kThreads) {
        const uint32_t s = group_start[g], nb = group_negs_before[g];
        const uint32_t e = g + 1 < groups ? group_start[g + 1] : (uint32_t)n;
        const uint32_t nb1 = g + 1 < groups ? group_negs_before[g + 1] : all_negs;
        const u64 pos = (u64)(e - s) - (nb1 - nb);
        if (pos) acc += (double)pos * (double)(P - (s - nb)) / (double)(n - s);
    }
    acc = block_sum<double>(acc, shd);
    if (threadIdx.x == 0) score_partial(out6 + 5, 1, 0, acc);
}

struct AucArrays {
    uint32_t *group_start, *group_negs, *meta;
};

// dt_metric_auc's launches; the compacted group arrays stay in the workspace
int auc_launches(const float* score, const float* label, int64_t n, void* ws, u64* out, hipStream_t st, const char* what,
                 AucArrays* arrays) {
    const int64_t tiles = tiles_of(n);
    char* w = reinterpret_cast<char*>(ws);
    uint32_t* keys = reinterpret_cast<uint32_t*>(w);
    uint32_t* vals = reinterpret_cast<uint32_t*>(w + a256(4 * n));
    char* sort_ws = w + 2 * a256(4 * n);
    u64* tile_sums = reinterpret_cast<u64*>(sort_ws + sort_ws_bytes(n));
    uint32_t* meta = reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(tile_sums) + a256(8 * tiles));
    // the sort's two scratch arrays are free once it has finished: the groups' starts and negatives-before live there
    uint32_t* group_start = reinterpret_cast<uint32_t*>(sort_ws);
    uint32_t* group_negs = reinterpret_cast<uint32_t*>(sort_ws + a256(4 * n));
    if (hipMemsetAsync(out, 0, 5 * sizeof(u64), st) != hipSuccess) return launch_status(what);
    hipLaunchKernelGGL(k_auc_keys, dim3(stride_blocks(n)), dim3(kThreads), 0, st, score, label, n, keys, vals, out);
    int rc = sort_pairs(keys, vals, n, keys, vals, sort_ws, st, what);       // in place: pass 0 reads, pass 1 writes
    if (rc != DT_OK) return rc;
    hipLaunchKernelGGL(k_auc_tile_sums, dim3((unsigned)tiles), dim3(kThreads), 0, st, keys, vals, n, tile_sums);
    hipLaunchKernelGGL(k_auc_tile_scan, dim3(1), dim3(kThreads), 0, st, tile_sums, tiles, meta);
    hipLaunchKernelGGL(k_auc_groups, dim3((unsigned)tiles), dim3(kThreads), 0, st, keys, vals, n, tile_sums, group_start,
                       group_negs);
    hipLaunchKernelGGL(k_auc_u2, dim3(stride_blocks(n)), dim3(kThreads), 0, st, group_start, group_negs, meta, n, out);
    arrays->group_start = group_start;
    arrays->group_negs = group_negs;
    arrays->meta = meta;
    return launch_status(what);
}

}  // namespace
}  // namespace dt

using namespace dt;

extern "C" int dt_metric_sort_tile(void) { return kTile; }

extern "C" int64_t dt_metric_sort_workspace_bytes(int64_t n) {
    DT_REQUIRE(n >= 0 && n < kMaxN, "dt_metric_sort_workspace_bytes: n = %lld outside [0, 2^31)", (long long)n);
    return sort_ws_bytes(n);
}

extern "C" int dt_metric_sort_pairs(const uint32_t* keys, const uint32_t* vals, int64_t n, uint32_t* keys_out,
                                    uint32_t* vals_out, void* ws, void* stream) {
    DT_REQUIRE(n >= 0 && n < kMaxN, "dt_metric_sort_pairs: n = %lld outside [0, 2^31)", (long long)n);
    if (n == 0) return DT_OK;
    DT_REQUIRE(keys && vals && keys_out && vals_out, "dt_metric_sort_pairs: null pointer");
    DT_REQUIRE(ws, "dt_metric_sort_pairs: null workspace (dt_metric_sort_workspace_bytes)");
    DT_REQUIRE(aligned(keys, 4) && aligned(vals, 4) && aligned(keys_out, 4) && aligned(vals_out, 4),
               "dt_metric_sort_pairs: keys / values are not 4-byte aligned");
    DT_REQUIRE(aligned(ws, 16), "dt_metric_sort_pairs: the workspace is not 16-byte aligned");
    return sort_pairs(keys, vals, n, keys_out, vals_out, ws, as_stream(stream), "dt_metric_sort_pairs");
}

// ---- the argument checks of the passes, in one order: n, then (n > 0) null pointers, then alignments -------------------------
static int check_n(const char* what, int64_t n) {
    DT_REQUIRE(n >= 0 && n < kMaxN, "%s: n = %lld outside [0, 2^31)", what, (long long)n);
    return DT_OK;
}

// a, b: the two float arrays, `names` in the message; has_ws: the pass takes the workspace <what>_workspace_bytes sizes.
// Nothing is looked at when n == 0: the call is a no-op.
static int check_pointers(const char* what, int64_t n, const void* a, const void* b, const char* names, const void* out,
                          const char* out_name, bool has_ws = false, const void* ws = nullptr) {
    if (n == 0) return DT_OK;
    DT_REQUIRE(a && b && out, "%s: null pointer", what);
    if (has_ws) DT_REQUIRE(ws, "%s: null workspace (%s_workspace_bytes)", what, what);
    DT_REQUIRE(aligned(a, 4) && aligned(b, 4), "%s: %s are not 4-byte aligned", what, names);
    DT_REQUIRE(aligned(out, 8), "%s: %s is not 8-byte aligned", what, out_name);
    if (has_ws) DT_REQUIRE(aligned(ws, 16), "%s: the workspace is not 16-byte aligned", what);
    return DT_OK;
}

// the element-wise and row passes; on success *total = n * C
static int score_args(const char* what, const void* y_true, const void* y_prob, int64_t n, int C, int min_C, const void* out,
                      int64_t* total) {
    int rc = check_n(what, n);
    if (rc != DT_OK) return rc;
    DT_REQUIRE(C >= min_C, "%s: C = %d, at least %d here", what, C, min_C);
    DT_REQUIRE(n * (int64_t)C < kMaxN, "%s: n * C = %lld x %d overflows 2^31 elements", what, (long long)n, C);
    *total = n * (int64_t)C;
    return check_pointers(what, n, y_true, y_prob, "y_true / y_prob", out, "out");
}

// the two ranking passes, which share a workspace size
static int64_t ranking_ws_bytes(const char* what, int64_t n) { return check_n(what, n) == DT_OK ? auc_ws_bytes(n) : DT_ERR_INVALID_ARG; }
static int ranking_args(const char* what, const void* score, const void* label, int64_t n, const void* ws, const void* out,
                        const char* out_name) {
    int rc = check_n(what, n);
    return rc != DT_OK ? rc : check_pointers(what, n, score, label, "score / label", out, out_name, true, ws);
}

extern "C" int64_t dt_metric_auc_workspace_bytes(int64_t n) { return ranking_ws_bytes("dt_metric_auc_workspace_bytes", n); }
extern "C" int64_t dt_score_ranking_workspace_bytes(int64_t n) { return ranking_ws_bytes("dt_score_ranking_workspace_bytes", n); }

extern "C" int dt_metric_auc(const float* score, const float* label, int64_t n, void* ws, int64_t* out5, void* stream) {
    int rc = ranking_args("dt_metric_auc", score, label, n, ws, out5, "out5");
    if (rc != DT_OK || n == 0) return rc;
    AucArrays arrays;
    return auc_launches(score, label, n, ws, reinterpret_cast<u64*>(out5), as_stream(stream), "dt_metric_auc", &arrays);
}

extern "C" int dt_score_ranking(const float* score, const float* label, int64_t n, void* ws, void* out, void* stream) {
    int rc = ranking_args("dt_score_ranking", score, label, n, ws, out, "out");
    if (rc != DT_OK || n == 0) return rc;
    hipStream_t st = as_stream(stream);
    u64* o = reinterpret_cast<u64*>(out);
    AucArrays a;
    rc = auc_launches(score, label, n, ws, o, st, "dt_score_ranking", &a);
    if (rc != DT_OK) return rc;
    const int blocks = score_blocks(n, 4 * kThreads);        // (the number of groups is the device's to know: at most n)
    hipLaunchKernelGGL(k_ap_partial, dim3((unsigned)blocks), dim3(kThreads), 0, st, a.group_start, a.group_negs, a.meta, n, o);
    hipLaunchKernelGGL((k_score_final<0, 1>), dim3(1), dim3(kThreads), 0, st, o + 5, blocks);
    return launch_status("dt_score_ranking");
}

extern "C" int dt_score_binary(const float* y_true, const float* y_prob, int y_kind, int64_t n, int C, void* out, void* stream) {
    DT_REQUIRE(y_kind == DT_METRIC_Y_LABELS || y_kind == DT_METRIC_Y_ONEHOT, "dt_score_binary: unknown y_kind %d", y_kind);
    int64_t total;
    int rc = score_args("dt_score_binary", y_true, y_prob, n, C, y_kind == DT_METRIC_Y_LABELS ? 2 : 1, out, &total);
    if (rc != DT_OK || n == 0) return rc;
    hipStream_t st = as_stream(stream);
    u64* o = reinterpret_cast<u64*>(out);
    const int blocks = score_blocks(total, 4 * kThreads);
    if (y_kind == DT_METRIC_Y_LABELS)
        hipLaunchKernelGGL(k_score_binary<DT_METRIC_Y_LABELS>, dim3((unsigned)blocks), dim3(kThreads), 0, st, y_true, y_prob, total, C, o);
    else
        hipLaunchKernelGGL(k_score_binary<DT_METRIC_Y_ONEHOT>, dim3((unsigned)blocks), dim3(kThreads), 0, st, y_true, y_prob, total, C, o);
    hipLaunchKernelGGL((k_score_final<4, 1>), dim3(1), dim3(kThreads), 0, st, o, blocks);
    return launch_status("dt_score_binary");
}

extern "C" int dt_score_regression(const float* y_true, const float* y_pred, int64_t n, void* out, void* stream) {
    int64_t total;
    int rc = score_args("dt_score_regression", y_true, y_pred, n, 1, 1, out, &total);
    if (rc != DT_OK || n == 0) return rc;
    hipStream_t st = as_stream(stream);
    u64* o = reinterpret_cast<u64*>(out);
    const int blocks = score_blocks(n, 4 * kThreads);
    hipLaunchKernelGGL(k_score_regression, dim3((unsigned)blocks), dim3(kThreads), 0, st, y_true, y_pred, n, o);
    hipLaunchKernelGGL((k_score_final<0, 2>), dim3(1), dim3(kThreads), 0, st, o, blocks);
    return launch_status("dt_score_regression");
}

extern "C" int dt_score_categorical(const float* y_prob, const float* y_true, int y_kind, int64_t n, int C, int k, void* out,
                                    void* stream) {
    DT_REQUIRE(y_kind == DT_METRIC_Y_LABELS || y_kind == DT_METRIC_Y_ONEHOT, "dt_score_categorical: unknown y_kind %d", y_kind);
    DT_REQUIRE(k >= 1, "dt_score_categorical: k = %d, top-k needs k >= 1", k);
    int64_t total;
    int rc = score_args("dt_score_categorical", y_true, y_prob, n, C, 2, out, &total);
    if (rc != DT_OK || n == 0) return rc;
    hipStream_t st = as_stream(stream);
    u64* o = reinterpret_cast<u64*>(out);
    const bool wide = C > kThreadRowMaxC;
    const int blocks = score_blocks(n, wide ? kWaves : kThreads);
    const bool onehot = y_kind == DT_METRIC_Y_ONEHOT;
    if (wide && onehot)
        hipLaunchKernelGGL(k_score_rows_wave<DT_METRIC_Y_ONEHOT>, dim3((unsigned)blocks), dim3(kThreads), 0, st, y_prob, y_true, n, C, k, o);
    else if (wide)
        hipLaunchKernelGGL(k_score_rows_wave<DT_METRIC_Y_LABELS>, dim3((unsigned)blocks), dim3(kThreads), 0, st, y_prob, y_true, n, C, k, o);
    else if (onehot)
        hipLaunchKernelGGL(k_score_rows_thread<DT_METRIC_Y_ONEHOT>, dim3((unsigned)blocks), dim3(kThreads), 0, st, y_prob, y_true, n, C, k, o);
    else
        hipLaunchKernelGGL(k_score_rows_thread<DT_METRIC_Y_LABELS>, dim3((unsigned)blocks), dim3(kThreads), 0, st, y_prob, y_true, n, C, k, o);
    hipLaunchKernelGGL((k_score_final<1, 1>), dim3(1), dim3(kThreads), 0, st, o, blocks);
    return launch_status("dt_score_categorical");
}

extern "C" int dt_metric_sums(const float* y_true, const float* y_prob, int64_t n, void* out, void* stream) {
    int64_t total;
    int rc = score_args("dt_metric_sums", y_true, y_prob, n, 1, 1, out, &total);
    if (rc != DT_OK || n == 0) return rc;
    hipStream_t st = as_stream(stream);
    u64* o = reinterpret_cast<u64*>(out);
    const int blocks = score_blocks(n, 4 * kThreads);
    hipLaunchKernelGGL(k_sums_partial, dim3((unsigned)blocks), dim3(kThreads), 0, st, y_true, y_prob, n, o);
    hipLaunchKernelGGL((k_score_final<1, 2>), dim3(1), dim3(kThreads), 0, st, o, blocks);
    return launch_status("dt_metric_sums");
}

extern "C" int dt_metric_argmax_hits(const float* y_prob, const float* y_true, int y_kind, int64_t n, int C, int64_t* out,
                                     void* stream) {
    int rc = check_n("dt_metric_argmax_hits", n);
    if (rc != DT_OK) return rc;
    DT_REQUIRE(C >= 2, "dt_metric_argmax_hits: C = %d, a multiclass output has at least 2 columns", C);
    DT_REQUIRE(y_kind == DT_METRIC_Y_LABELS || y_kind == DT_METRIC_Y_ONEHOT, "dt_metric_argmax_hits: unknown y_kind %d", y_kind);
    rc = check_pointers("dt_metric_argmax_hits", n, y_prob, y_true, "y_prob / y_true", out, "out");
    if (rc != DT_OK || n == 0) return rc;
    hipStream_t st = as_stream(stream);
    if (hipMemsetAsync(out, 0, sizeof(int64_t), st) != hipSuccess) return launch_status("dt_metric_argmax_hits");
    u64* o = reinterpret_cast<u64*>(out);
    if (y_kind == DT_METRIC_Y_ONEHOT)
        hipLaunchKernelGGL(k_argmax_hits<DT_METRIC_Y_ONEHOT>, dim3(stride_blocks(n)), dim3(kThreads), 0, st, y_prob, y_true, n, C, o);
    else
        hipLaunchKernelGGL(k_argmax_hits<DT_METRIC_Y_LABELS>, dim3(stride_blocks(n)), dim3(kThreads), 0, st, y_prob, y_true, n, C, o);
    return launch_status("dt_metric_argmax_hits");
}
