// prep_fit.hip — the preprocessor's fit on the device: the profile of every raw numeric column of a frame
// (models/preprocessor.py: DefaultPreprocessor.fit_feed; ops.column_profile, ops.column_order_stats).
//
// Everything the fit needs of a numeric column — nunique, the typing decision, the distinct values a label encoder sees, min,
// max, the mean's sum, the quantile edges' neighbours — is read off ONE object: the column's sorted distinct values with their
// counts.  That object is a sort and a run-length pass.  All C columns of a frame (one N) go through every launch together: the
// column is grid dimension y, so 39 columns cost the launches of one.
//
// Keys.  An element becomes an ORDERED key: an unsigned 64-bit word whose integer order is the column's numeric order.
//   bool, uintW   the value, zero-extended
//   intW          the W-byte two's complement word with its sign bit flipped, zero-extended  (int8 -128 -> 0x00, 127 -> 0xFF)
//   float32/64    the IEEE bits, negative: all bits flipped, else: the sign bit set; zero-extended.  -0.0 is the key just below
//                 +0.0 (they stay two keys), every NaN is the one key 0xFFC00000 / 0xFFF8000000000000, above +inf: NaN sorts last.
//   The map is a bijection on the non-NaN values of the dtype, so the raw value (and dt_prep_transform's LOOKUP key) is
//   recovered exactly from a key (key_value below; ops.profile_values on the host).  A W-byte dtype has W key bytes: the digits
//   above are zero by construction and are never looked at.
//
// Sort: LSD radix, 8-bit digits, keys only, stable, ping-pong between two [C][N] buffers.
//   k_profile_keys  (grid tiles x C) writes the keys and, in the same read, ALL W digit histograms of its tile into LDS
//                   (integer LDS atomics), adds them to totals[c][digit place][256] (integer global atomics: the sum does not
//                   depend on the order) and leaves the tile's float64 sum.  A wave whose 64 elements share the digit — the rule
//                   for the high bytes of an int64 id column — adds ONE popcount instead of 64 colliding atomics (hist_add).
//   k_profile_plan  (grid C) a digit place whose histogram has a single non-empty bin cannot change the order: its pass is DEAD.
//                   plan[c] = the mask of LIVE places.  It also adds the tiles' sums in tile order.
//   per place p = 0..7, three launches that return at once for a column whose place p is dead:
//     k_sort_hist     counts[c][digit][tile]                                     (LDS atomics, hist_add)
//     k_sort_scan     block (digit d, column c): base = the totals of the digits below d, then the exclusive scan of row d
//     k_sort_scatter  wave w owns the w-th quarter of a tile; the rank of an element among its wave's 64 is the number of LOWER
//                     lanes with the same digit (8 ballots), plus the wave's running counter of the digit: equal digits keep
//                     their order, the pass is stable.
//   A column's source buffer of pass p is A or B by the parity of its live places below p, its sorted keys end in A or B by the
//   parity of all its live places: a bool or int8 column sorts in at most 1 pass, float32 in at most 4, an int64 column of ids
//   below 65 536 in 2; only a column that really uses all 64 bits pays 8.
//   No block ever waits for another block: offsets come from the scan LAUNCH between the histogram and the scatter, there is no
//   look-back, flag or grid barrier, and every loop is bounded by N.  The launch count is fixed: 2 + 24 + 4 (+ 1 for ranks).
//
// Run-length pass over the sorted keys (NaN keys are last and start no run): k_rle_sums (per tile: run starts, NaNs; the one
//   place where +0.0 follows -0.0), k_rle_scan (per column: exclusive tile prefix; the counts, nunique, min and max keys),
//   k_rle_emit + k_rle_counts (columns with at most `cap` distinct keys: the keys and their counts, compacted in order).
// Sum: float64 over the non-NaN values, fixed order (csrc/loss_sum.h's scheme): a thread adds its elements in index order, lanes
//   combine by halving, waves in order, tiles in order — the same bits on every run.
// Order statistics: k_order_stats reads up to 32 ranks per column of the virtual sequence "non-NaN values ascending with
//   nan_count copies of `fill` at its rank" (what np.quantile sorts after imputation): one fixed-trip binary search per rank.
#include "common.h"
#include "optim_dev.h"

namespace dt {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr int kItems = 16;                          // elements per thread and tile
constexpr int kTile = DT_PROFILE_TILE;
constexpr int kWaveSpan = kTile / kWaves;           // consecutive elements one wave of the scatter owns
constexpr int kRounds = kWaveSpan / kWave;
constexpr int kDigits = 256;
constexpr int kPlaces = 8;
constexpr int kStat = DT_PROFILE_STAT_WORDS;
constexpr int kRanks = DT_PROFILE_MAX_RANKS;
constexpr int64_t kMaxN = (int64_t)1 << 31;
static_assert(kTile == kThreads * kItems && kRanks <= kWave, "tile geometry");

typedef unsigned long long u64;

constexpr u64 kNan32 = 0xFFC00000ull, kNan64 = 0xFFF8000000000000ull;      // the ordered NaN keys

inline int64_t a256(int64_t b) { return (b + 255) & ~(int64_t)255; }
inline int64_t tiles_of(int64_t n) { return (n + kTile - 1) / kTile; }

// the workspace: A, B [C][N] keys | counts [C][256][tiles] | totals [C][8][256] | sums [C][tiles] f64 | tile_sums [C][tiles] |
// plan [C] | zero_pair [C] | starts [C][cap].  Only `starts`, the LAST region, depends on cap: dt_column_order_stats finds A, B and
// plan with layout(N, C, 0) in a workspace dt_column_profile filled with any cap.  Keep cap-sized regions behind everything it reads.
struct Layout {
    int64_t a, b, counts, totals, sums, tile_sums, plan, zero_pair, starts, bytes;
};
inline Layout layout(int64_t N, int C, int cap) {
    const int64_t T = tiles_of(N);
    Layout L;
    L.a = 0;
    L.b = L.a + a256(8 * N * C);
    L.counts = L.b + a256(8 * N * C);
    L.totals = L.counts + a256(4 * (int64_t)C * kDigits * T);
    L.sums = L.totals + a256(4 * (int64_t)C * kPlaces * kDigits);
    L.tile_sums = L.sums + a256(8 * (int64_t)C * T);
    L.plan = L.tile_sums + a256(8 * (int64_t)C * T);
    L.zero_pair = L.plan + a256(4 * (int64_t)C);
    L.starts = L.zero_pair + a256(4 * (int64_t)C);
    L.bytes = L.starts + a256(8 * (int64_t)C * cap);
    return L;
}

// ---- dtype helpers ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int key_bytes(int dtype) {
    switch (dtype) {
        case DT_PREP_BOOL: case DT_PREP_I8: case DT_PREP_U8: return 1;
        case DT_PREP_I16: case DT_PREP_U16: return 2;
        case DT_PREP_I32: case DT_PREP_U32: case DT_PREP_F32: return 4;
        case DT_PREP_I64: case DT_PREP_U64: case DT_PREP_F64: return 8;
        default: return 0;
    }
}

__device__ __forceinline__ u64 ordered_key(const void* src, int dtype, int64_t i) {
    switch (dtype) {
        case DT_PREP_BOOL: return (u64)(((const uint8_t*)src)[i] != 0);
        case DT_PREP_I8: return (u64)(uint8_t)(((const uint8_t*)src)[i] ^ 0x80u);
        case DT_PREP_I16: return (u64)(uint16_t)(((const uint16_t*)src)[i] ^ 0x8000u);
        case DT_PREP_I32: return (u64)(((const uint32_t*)src)[i] ^ 0x80000000u);
        case DT_PREP_I64: return ((const u64*)src)[i] ^ 0x8000000000000000ull;
        case DT_PREP_U8: return (u64)((const uint8_t*)src)[i];
        case DT_PREP_U16: return (u64)((const uint16_t*)src)[i];
        case DT_PREP_U32: return (u64)((const uint32_t*)src)[i];
        case DT_PREP_U64: return ((const u64*)src)[i];
        case DT_PREP_F32: {
            const uint32_t b = ((const uint32_t*)src)[i];
            if ((b & 0x7FFFFFFFu) > 0x7F800000u) return kNan32;
            return (u64)((b & 0x80000000u) ? ~b : (b | 0x80000000u));
        }
        case DT_PREP_F64: {
            const u64 b = ((const u64*)src)[i];
            if ((b & 0x7FFFFFFFFFFFFFFFull) > 0x7FF0000000000000ull) return kNan64;
            return (b & 0x8000000000000000ull) ? ~b : (b | 0x8000000000000000ull);
        }
        default: return 0;
    }
}

__device__ __forceinline__ bool is_nan_key(u64 k, int dtype) {
    return (dtype == DT_PREP_F32 && k == kNan32) || (dtype == DT_PREP_F64 && k == kNan64);
}

// the value of a non-NaN key as a double (ints: one correctly rounded conversion; float32: exact)
__device__ __forceinline__ double key_value(u64 k, int dtype) {
    switch (dtype) {
        case DT_PREP_I8: return (double)((int64_t)k - 0x80);
        case DT_PREP_I16: return (double)((int64_t)k - 0x8000);
        case DT_PREP_I32: return (double)((int64_t)k - 0x80000000ll);
        case DT_PREP_I64: return __ll2double_rn((long long)(k ^ 0x8000000000000000ull));
        case DT_PREP_U64: return __ull2double_rn(k);
        case DT_PREP_F32: {
            const uint32_t o = (uint32_t)k;
            return (double)__uint_as_float((o & 0x80000000u) ? (o ^ 0x80000000u) : ~o);
        }
        case DT_PREP_F64: return __longlong_as_double((long long)((k & 0x8000000000000000ull) ? (k ^ 0x8000000000000000ull) : ~k));
        default: return (double)k;              // bool, uint8 .. uint32
    }
}

// ---- block helpers (kThreads threads; every thread of the block calls them) ------------------------------------------------------
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

// one wave adds its valid lanes' digits to an LDS histogram; every lane of the wave calls it.  When all valid lanes hold one
// digit, its first valid lane adds their number: one atomic instead of 64 on one address.
__device__ __forceinline__ void hist_add(uint32_t* h, uint32_t d, bool valid, int lane) {
    const u64 act = __ballot(valid);
    if (!act) return;                                       // (wave-uniform)
    const int first = __ffsll((long long)act) - 1;
    const uint32_t d0 = __shfl(d, first, kWave);
    if (__ballot(valid && d == d0) == act) {
        if (lane == first) atomicAdd(&h[d0], (uint32_t)__popcll(act));
    } else if (valid) {
        atomicAdd(&h[d], 1u);
    }
}

// where pass p of a column reads and writes; false: the place is dead for this column
__device__ __forceinline__ bool pass_buffers(uint32_t mask, int p, u64* a, u64* b, const u64** in, u64** out) {
    if (!((mask >> p) & 1u)) return false;
    const bool odd = __popc(mask & ((1u << p) - 1u)) & 1;
    *in = odd ? b : a;
    *out = odd ? a : b;
    return true;
}
__device__ __forceinline__ const u64* sorted_keys(uint32_t mask, const u64* a, const u64* b) { return (__popc(mask) & 1) ? b : a; }

// ---- keys, all digit histograms, the tile's sum ---------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_profile_keys(const void* const* __restrict__ srcs, const int32_t* __restrict__ dtypes,
                                                           int64_t N, int64_t tiles, u64* __restrict__ keys,
                                                           uint32_t* __restrict__ totals, double* __restrict__ sums) {
    __shared__ uint32_t h[kPlaces][kDigits];
    __shared__ double shd[kWaves];
    const int c = blockIdx.y, lane = threadIdx.x & (kWave - 1);
    const int64_t tile = blockIdx.x;
    const int dtype = dtypes[c];
    const int W = key_bytes(dtype);
    const void* src = srcs[c];
    for (int p = 0; p < W; ++p) h[p][threadIdx.x] = 0;
    __syncthreads();
    u64* out = keys + (int64_t)c * N;
    double s = 0.0;
    for (int j = 0; j < kItems; ++j) {
        const int64_t i = tile * kTile + j * kThreads + threadIdx.x;
        const bool valid = i < N && W > 0;
        const u64 k = valid ? ordered_key(src, dtype, i) : 0;
        if (valid) {
            out[i] = k;
            if (!is_nan_key(k, dtype)) s += key_value(k, dtype);
        }
        for (int p = 0; p < W; ++p) hist_add(h[p], (uint32_t)(k >> (8 * p)) & (kDigits - 1), valid, lane);
    }
    __syncthreads();
    for (int p = 0; p < W; ++p) {
        const uint32_t n = h[p][threadIdx.x];
        if (n) atomicAdd(&totals[((int64_t)c * kPlaces + p) * kDigits + threadIdx.x], n);
    }
    s = block_sum<double>(s, shd);
    if (threadIdx.x == 0) sums[(int64_t)c * tiles + tile] = s;
}

// grid = C blocks: the live places of the column, the column's sum; stats words 5 (sum), 6 (live mask), 7 (0)
__global__ __launch_bounds__(kThreads) void k_profile_plan(const int32_t* __restrict__ dtypes, int64_t N, int64_t tiles,
                                                           const uint32_t* __restrict__ totals, const double* __restrict__ sums,
                                                           uint32_t* __restrict__ plan, uint32_t* __restrict__ zero_pair,
                                                           int64_t* __restrict__ stats) {
    __shared__ double shd[kWaves];
    const int c = blockIdx.x;
    const int W = key_bytes(dtypes[c]);
    uint32_t mask = 0;
    for (int p = 0; p < W; ++p) {
        const uint32_t n = totals[((int64_t)c * kPlaces + p) * kDigits + threadIdx.x];
        if (!__syncthreads_or((int64_t)n == N)) mask |= 1u << p;
    }
    double s = 0.0;
    for (int64_t t = threadIdx.x; t < tiles; t += kThreads) s += sums[(int64_t)c * tiles + t];
    s = block_sum<double>(s, shd);
    if (threadIdx.x == 0) {
        plan[c] = mask;
        zero_pair[c] = 0;
        stats[(int64_t)c * kStat + 5] = (int64_t)__double_as_longlong(s);
        stats[(int64_t)c * kStat + 6] = (int64_t)mask;
        stats[(int64_t)c * kStat + 7] = 0;
    }
}

// ---- one pass of the sort ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_sort_hist(u64* __restrict__ a, u64* __restrict__ b, const uint32_t* __restrict__ plan,
                                                        int64_t N, int64_t tiles, int p, uint32_t* __restrict__ counts) {
    __shared__ uint32_t h[kDigits];
    const int c = blockIdx.y, lane = threadIdx.x & (kWave - 1);
    const int64_t tile = blockIdx.x;
    const u64* in;
    u64* out;
    if (!pass_buffers(plan[c], p, a + (int64_t)c * N, b + (int64_t)c * N, &in, &out)) return;
    h[threadIdx.x] = 0;
    __syncthreads();
    for (int j = 0; j < kItems; ++j) {
        const int64_t i = tile * kTile + j * kThreads + threadIdx.x;
        const bool valid = i < N;
        const u64 k = valid ? in[i] : 0;
        hist_add(h, (uint32_t)(k >> (8 * p)) & (kDigits - 1), valid, lane);
    }
    __syncthreads();
    counts[((int64_t)c * kDigits + threadIdx.x) * tiles + tile] = h[threadIdx.x];
}

// grid = (kDigits, C); block (d, c) turns row d of the column's counts into the start of (digit d, tile t) inside the column
__global__ __launch_bounds__(kThreads) void k_sort_scan(uint32_t* __restrict__ counts, const uint32_t* __restrict__ totals,
                                                        const uint32_t* __restrict__ plan, int64_t tiles, int p) {
    __shared__ uint32_t sh[kWaves];
    const int d = blockIdx.x, c = blockIdx.y;
    if (!((plan[c] >> p) & 1u)) return;
    const uint32_t* tot = totals + ((int64_t)c * kPlaces + p) * kDigits;
    uint32_t carry = block_sum<uint32_t>((int)threadIdx.x < d ? tot[threadIdx.x] : 0u, sh);
    uint32_t* row = counts + ((int64_t)c * kDigits + d) * tiles;
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

__global__ __launch_bounds__(kThreads) void k_sort_scatter(u64* __restrict__ a, u64* __restrict__ b, const uint32_t* __restrict__ plan,
                                                           const uint32_t* __restrict__ offsets, int64_t N, int64_t tiles, int p) {
    __shared__ uint32_t cnt[kWaves][kDigits];
    const int c = blockIdx.y, lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const int64_t tile = blockIdx.x;
    const u64* in;
    u64* out;
    if (!pass_buffers(plan[c], p, a + (int64_t)c * N, b + (int64_t)c * N, &in, &out)) return;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) cnt[w][threadIdx.x] = 0;
    __syncthreads();
    const int shift = 8 * p;
    const int64_t base = tile * kTile + (int64_t)wave * kWaveSpan;
    for (int r = 0; r < kRounds; ++r) {
        const int64_t i = base + r * kWave + lane;
        const bool valid = i < N;
        const u64 k = valid ? in[i] : 0;
        hist_add(cnt[wave], (uint32_t)(k >> shift) & (kDigits - 1), valid, lane);
    }
    __syncthreads();
    {   // thread = digit: where each wave's elements of this digit start
        uint32_t off = offsets[((int64_t)c * kDigits + threadIdx.x) * tiles + tile];
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            const uint32_t n = cnt[w][threadIdx.x];
            cnt[w][threadIdx.x] = off;
            off += n;
        }
    }
    __syncthreads();
    // The wave's own counters from here on; no other wave touches cnt[wave].  Lanes holding the same digit form a group (`peers`);
    // groups of different digits touch different words.  Inside a group every lane LOADS mine[d] and only then the group's
    // highest lane STORES the advanced counter: the load precedes the store in program order, one wave's LDS operations
    // complete in program order, and volatile keeps the compiler from reordering or caching them.  The next round's loads
    // follow this round's stores the same way.  Order kept: lane, then round, then wave, then tile — the input order.
    volatile uint32_t* mine = cnt[wave];
    const u64 below = ((u64)1 << lane) - 1;
    for (int r = 0; r < kRounds; ++r) {
        const int64_t i = base + r * kWave + lane;
        const bool valid = i < N;
        const u64 key = valid ? in[i] : 0;
        const uint32_t d = (uint32_t)(key >> shift) & (kDigits - 1);
        u64 peers = __ballot(valid);
#pragma unroll
        for (int bit = 0; bit < 8; ++bit) {
            const bool on = (d >> bit) & 1u;
            const u64 m = __ballot(on);
            peers &= on ? m : ~m;
        }
        if (valid) {
            const uint32_t pos = mine[d] + (uint32_t)__popcll(peers & below);
            if ((peers >> lane) == 1) mine[d] = pos + 1;        // the highest lane of the group holds its last element
            if ((int64_t)pos < N) out[pos] = key;               // (offsets are a permutation of [0, N): the guard only keeps a
                                                                // corrupted workspace from becoming a store out of bounds)
        }
    }
}

// ---- run lengths ------------------------------------------------------------------------------------------------------------------
// (NaNs << 32 | run starts) of the kItems consecutive sorted elements of a thread; bit j of *flags: element j starts a run;
// *zero_pair: the +0.0 run starts right behind a -0.0
__device__ __forceinline__ u64 rle_thread_items(const u64* __restrict__ keys, int64_t i0, int64_t N, int dtype, uint32_t* flags,
                                                bool* zero_pair) {
    const bool f32 = dtype == DT_PREP_F32, f64 = dtype == DT_PREP_F64;
    const u64 plus0 = f32 ? 0x80000000ull : 0x8000000000000000ull, minus0 = plus0 - 1;
    u64 prev = (i0 > 0 && i0 <= N) ? keys[i0 - 1] : 0;
    uint32_t starts = 0, nans = 0, f = 0;
    bool zp = false;
#pragma unroll
    for (int j = 0; j < kItems; ++j) {
        const int64_t i = i0 + j;
        if (i < N) {
            const u64 k = keys[i];
            const bool nan = is_nan_key(k, dtype);
            const uint32_t start = !nan && (i == 0 || k != prev);
            zp |= (f32 || f64) && start && i > 0 && k == plus0 && prev == minus0;
            f |= start << j;
            starts += start;
            nans += nan;
            prev = k;
        }
    }
    *flags = f;
    *zero_pair = zp;
    return ((u64)nans << 32) | starts;
}

__global__ __launch_bounds__(kThreads) void k_rle_sums(const u64* __restrict__ a, const u64* __restrict__ b,
                                                       const uint32_t* __restrict__ plan, const int32_t* __restrict__ dtypes, int64_t N,
                                                       int64_t tiles, u64* __restrict__ tile_sums, uint32_t* __restrict__ zero_pair) {
    __shared__ u64 sh[kWaves];
    const int c = blockIdx.y;
    const u64* keys = sorted_keys(plan[c], a + (int64_t)c * N, b + (int64_t)c * N);
    uint32_t flags;
    bool zp;
    const int64_t i0 = (int64_t)blockIdx.x * kTile + (int64_t)threadIdx.x * kItems;
    const u64 s = block_sum<u64>(rle_thread_items(keys, i0, N, dtypes[c], &flags, &zp), sh);
    if (threadIdx.x == 0) tile_sums[(int64_t)c * tiles + blockIdx.x] = s;
    if (zp) zero_pair[c] = 1;                   // (one place per column at most)
}

// grid = C blocks: tile_sums -> exclusive prefix; stats words 0 .. 4
__global__ __launch_bounds__(kThreads) void k_rle_scan(const u64* __restrict__ a, const u64* __restrict__ b,
                                                       const uint32_t* __restrict__ plan, int64_t N, int64_t tiles,
                                                       u64* __restrict__ tile_sums, const uint32_t* __restrict__ zero_pair,
                                                       int64_t* __restrict__ stats) {
    __shared__ u64 sh[kWaves];
    const int c = blockIdx.x;
    u64* row = tile_sums + (int64_t)c * tiles;
    u64 carry = 0;
    for (int64_t c0 = 0; c0 < tiles; c0 += kThreads) {
        const int64_t j = c0 + threadIdx.x;
        const u64 v = j < tiles ? row[j] : 0;
        u64 all;
        const u64 e = carry + block_excl_scan<u64>(v, &all, sh);
        if (j < tiles) row[j] = e;
        carry += all;
    }
    if (threadIdx.x == 0) {
        const u64* keys = sorted_keys(plan[c], a + (int64_t)c * N, b + (int64_t)c * N);
        const int64_t distinct = (int64_t)(uint32_t)carry, nans = (int64_t)(carry >> 32);
        const int64_t m = N - nans;
        int64_t* st = stats + (int64_t)c * kStat;
        st[0] = distinct;
        st[1] = nans;
        st[2] = distinct - (zero_pair[c] ? 1 : 0);
        st[3] = (m > 0 && m <= N) ? (int64_t)keys[0] : 0;
        st[4] = (m > 0 && m <= N) ? (int64_t)keys[m - 1] : 0;
    }
}

// columns with at most cap distinct keys: run g -> dkeys[c][g] and starts[c][g]
__global__ __launch_bounds__(kThreads) void k_rle_emit(const u64* __restrict__ a, const u64* __restrict__ b,
                                                       const uint32_t* __restrict__ plan, const int32_t* __restrict__ dtypes, int64_t N,
                                                       int64_t tiles, const u64* __restrict__ tile_prefix,
                                                       const int64_t* __restrict__ stats, int cap, u64* __restrict__ dkeys,
                                                       int64_t* __restrict__ starts) {
    __shared__ u64 sh[kWaves];
    const int c = blockIdx.y;
    if (stats[(int64_t)c * kStat] > cap) return;
    const u64* keys = sorted_keys(plan[c], a + (int64_t)c * N, b + (int64_t)c * N);
    uint32_t flags;
    bool zp;
    const int64_t i0 = (int64_t)blockIdx.x * kTile + (int64_t)threadIdx.x * kItems;
    const u64 mine = rle_thread_items(keys, i0, N, dtypes[c], &flags, &zp);
    u64 all;
    const u64 e = tile_prefix[(int64_t)c * tiles + blockIdx.x] + block_excl_scan<u64>(mine, &all, sh);
    int64_t g = (int64_t)(uint32_t)e;
#pragma unroll
    for (int j = 0; j < kItems; ++j) {
        if ((flags >> j) & 1u) {
            if (g < cap) {
                dkeys[(int64_t)c * cap + g] = keys[i0 + j];         // (a set flag means i0 + j < N)
                starts[(int64_t)c * cap + g] = i0 + j;
            }
            ++g;
        }
    }
}

// grid = (ceil(cap / kThreads), C): the length of run g
__global__ __launch_bounds__(kThreads) void k_rle_counts(const int64_t* __restrict__ stats, const int64_t* __restrict__ starts, int64_t N,
                                                         int cap, int64_t* __restrict__ dcounts) {
    const int c = blockIdx.y;
    const int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int64_t distinct = stats[(int64_t)c * kStat], nans = stats[(int64_t)c * kStat + 1];
    if (distinct > cap || g >= distinct) return;                    // g < distinct <= cap
    const int64_t* s = starts + (int64_t)c * cap;
    dcounts[(int64_t)c * cap + g] = (g + 1 < distinct ? s[g + 1] : N - nans) - s[g];
}

// ---- order statistics -------------------------------------------------------------------------------------------------------------
// grid = C blocks of one wave: lane r answers ranks[c][r]
__global__ __launch_bounds__(kWave) void k_order_stats(const u64* __restrict__ a, const u64* __restrict__ b,
                                                       const uint32_t* __restrict__ plan, const int32_t* __restrict__ dtypes, int64_t N,
                                                       const int64_t* __restrict__ stats, const int64_t* __restrict__ ranks,
                                                       const double* __restrict__ fills, double* __restrict__ out) {
    const int c = blockIdx.x, r = threadIdx.x;
    if (r >= kRanks) return;
    const int dtype = dtypes[c];
    const u64* keys = sorted_keys(plan[c], a + (int64_t)c * N, b + (int64_t)c * N);
    int64_t nans = stats[(int64_t)c * kStat + 1];
    if (nans < 0 || nans > N) nans = N;
    const int64_t m = N - nans, rank = ranks[(int64_t)c * kRanks + r];
    const double fill = fills[c];
    double v = __longlong_as_double(0x7ff8000000000000LL);
    if (rank >= 0 && rank < N) {
        int64_t lo = 0;                         // how many of the m values are < fill: 31 halvings cover N < 2^31
        if (nans > 0)
            for (int t = 30; t >= 0; --t) {
                const int64_t probe = lo + ((int64_t)1 << t);
                if (probe <= m && key_value(keys[probe - 1], dtype) < fill) lo = probe;
            }
        if (nans > 0 && rank >= lo && rank < lo + nans) v = fill;
        else v = key_value(keys[(nans > 0 && rank >= lo + nans) ? rank - nans : rank], dtype);
    }
    out[(int64_t)c * kRanks + r] = v;
}

int check_shape(const char* who, int64_t N, int C) {
    DT_REQUIRE(N >= 0 && N < kMaxN, "%s: N = %lld outside [0, 2^31)", who, (long long)N);
    DT_REQUIRE(C >= 1, "%s: C = %d, at least one column", who, C);
    DT_UNSUPPORTED(C > DT_PROFILE_MAX_COLS, "%s: C = %d columns, at most %d in one call", who, C, DT_PROFILE_MAX_COLS);
    return DT_OK;
}

int check_dtypes(const char* who, const int32_t* dtypes_host, int C) {
    for (int c = 0; c < C; ++c)
        DT_REQUIRE(dtypes_host[c] >= 0 && dtypes_host[c] < DT_PREP_DTYPE_COUNT, "%s: column %d: unknown dtype code %d", who, c,
                   dtypes_host[c]);
    return DT_OK;
}

}  // namespace
}  // namespace dt

using namespace dt;

extern "C" int64_t dt_column_profile_workspace_bytes(int64_t N, int C, int cap) {
    const char* who = "dt_column_profile_workspace_bytes";
    int rc = check_shape(who, N, C);
    if (rc != DT_OK) return rc;
    DT_REQUIRE(cap >= 0, "%s: cap = %d", who, cap);
    return layout(N, C, cap).bytes;
}

extern "C" int dt_column_profile(const void* const* srcs, const int32_t* dtypes, const void* const* srcs_host,
                                 const int32_t* dtypes_host, int64_t N, int C, int cap, int64_t* stats, uint64_t* distinct_keys,
                                 int64_t* distinct_counts, void* ws, void* stream) {
    const char* who = "dt_column_profile";
    int rc = check_shape(who, N, C);
    if (rc != DT_OK) return rc;
    DT_REQUIRE(cap >= 0, "%s: cap = %d", who, cap);
    DT_REQUIRE(srcs && dtypes && srcs_host && dtypes_host && stats, "%s: null pointer", who);
    DT_REQUIRE(cap == 0 || (distinct_keys && distinct_counts), "%s: null distinct_keys / distinct_counts with cap = %d", who, cap);
    DT_REQUIRE(aligned_to(srcs, 8) && aligned_to(dtypes, 4) && aligned_to(stats, 8) && aligned_to(distinct_keys, 8) &&
               aligned_to(distinct_counts, 8), "%s: misaligned pointer", who);
    rc = check_dtypes(who, dtypes_host, C);
    if (rc != DT_OK) return rc;
    static const int width[DT_PREP_DTYPE_COUNT] = {1, 1, 2, 4, 8, 1, 2, 4, 8, 4, 8};
    for (int c = 0; c < C; ++c) {
        DT_REQUIRE(srcs_host[c] || N == 0, "%s: column %d: null source", who, c);
        DT_REQUIRE(aligned_to(srcs_host[c], width[dtypes_host[c]]), "%s: column %d: misaligned source", who, c);
    }
    if (N == 0) return DT_OK;
    DT_REQUIRE(ws, "%s: null workspace (dt_column_profile_workspace_bytes)", who);
    DT_REQUIRE(aligned_to(ws, 16), "%s: the workspace is not 16-byte aligned", who);
    hipStream_t st = as_stream(stream);
    const Layout L = layout(N, C, cap);
    char* w = reinterpret_cast<char*>(ws);
    u64 *a = reinterpret_cast<u64*>(w + L.a), *b = reinterpret_cast<u64*>(w + L.b);
    uint32_t* counts = reinterpret_cast<uint32_t*>(w + L.counts);
    uint32_t* totals = reinterpret_cast<uint32_t*>(w + L.totals);
    double* sums = reinterpret_cast<double*>(w + L.sums);
    u64* tile_sums = reinterpret_cast<u64*>(w + L.tile_sums);
    uint32_t* plan = reinterpret_cast<uint32_t*>(w + L.plan);
    uint32_t* zero_pair = reinterpret_cast<uint32_t*>(w + L.zero_pair);
    int64_t* starts = reinterpret_cast<int64_t*>(w + L.starts);
    const int64_t tiles = tiles_of(N);
    const dim3 by_tile((unsigned)tiles, (unsigned)C), block(kThreads);
    if (hipMemsetAsync(totals, 0, sizeof(uint32_t) * C * kPlaces * kDigits, st) != hipSuccess) return launch_status(who);
    hipLaunchKernelGGL(k_profile_keys, by_tile, block, 0, st, srcs, dtypes, N, tiles, a, totals, sums);
    hipLaunchKernelGGL(k_profile_plan, dim3((unsigned)C), block, 0, st, dtypes, N, tiles, totals, sums, plan, zero_pair, stats);
    for (int p = 0; p < kPlaces; ++p) {
        hipLaunchKernelGGL(k_sort_hist, by_tile, block, 0, st, a, b, plan, N, tiles, p, counts);
        hipLaunchKernelGGL(k_sort_scan, dim3(kDigits, (unsigned)C), block, 0, st, counts, totals, plan, tiles, p);
        hipLaunchKernelGGL(k_sort_scatter, by_tile, block, 0, st, a, b, plan, counts, N, tiles, p);
    }
    hipLaunchKernelGGL(k_rle_sums, by_tile, block, 0, st, a, b, plan, dtypes, N, tiles, tile_sums, zero_pair);
    hipLaunchKernelGGL(k_rle_scan, dim3((unsigned)C), block, 0, st, a, b, plan, N, tiles, tile_sums, zero_pair, stats);
    if (cap > 0) {
        hipLaunchKernelGGL(k_rle_emit, by_tile, block, 0, st, a, b, plan, dtypes, N, tiles, tile_sums, stats, cap,
                           reinterpret_cast<u64*>(distinct_keys), starts);
        hipLaunchKernelGGL(k_rle_counts, dim3((unsigned)((cap + kThreads - 1) / kThreads), (unsigned)C), block, 0, st, stats, starts,
                           N, cap, distinct_counts);
    }
    return launch_status(who);
}

extern "C" int dt_column_order_stats(const void* ws, const int32_t* dtypes, const int32_t* dtypes_host, int64_t N, int C,
                                     const int64_t* stats, const int64_t* ranks, const double* fills, double* out, void* stream) {
    const char* who = "dt_column_order_stats";
    int rc = check_shape(who, N, C);
    if (rc != DT_OK) return rc;
    DT_REQUIRE(N >= 1, "%s: N = 0: an empty column has no order statistics", who);
    DT_REQUIRE(ws && dtypes && dtypes_host && stats && ranks && fills && out, "%s: null pointer", who);
    DT_REQUIRE(aligned_to(ws, 16) && aligned_to(dtypes, 4) && aligned_to(stats, 8) && aligned_to(ranks, 8) && aligned_to(fills, 8) &&
               aligned_to(out, 8), "%s: misaligned pointer", who);
    rc = check_dtypes(who, dtypes_host, C);
    if (rc != DT_OK) return rc;
    const Layout L = layout(N, C, 0);
    const char* w = reinterpret_cast<const char*>(ws);
    hipLaunchKernelGGL(k_order_stats, dim3((unsigned)C), dim3(kWave), 0, as_stream(stream), reinterpret_cast<const u64*>(w + L.a),
                       reinterpret_cast<const u64*>(w + L.b), reinterpret_cast<const uint32_t*>(w + L.plan), dtypes, N, stats, ranks,
                       fills, out);
    return launch_status(who);
}
