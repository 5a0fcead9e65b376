// gbdt.hip — a histogram gradient-boosted tree trainer and leaf predictor: the GBM leaf features of
// models/preprocessor.py GbmLeavesEncoder (ModelConfig.apply_gbm_features; ops.gbdt_grow_tree / gbdt_gradients /
// gbdt_predict_leaves).  LightGBM's algorithm in outline (binned features, leaf-wise growth, histogram subtraction); it is not
// compared with a LightGBM run.
//
// Exact by construction.  Gradients and hessians are quantised once per round to int32 (q = rint(v * 2^S), |q| < 2^24), a
// histogram entry is (sum qg int64, sum qh int64, count int32).  Integer sums do not depend on the order of addition, so the
// histograms are built with LDS and global INTEGER atomics; there is no float atomic.  Gains, leaf values and the comparison
// of gains are float64 arithmetic on those integers with + - * / only, each correctly rounded and never contracted, in one
// written order: numpy gives the same bits.  The partition of a leaf's rows is a stable count-and-scatter, so the row-index
// arrays, and with them everything else, are the same on every run.
//
// Data.  bins uint8 [P][N] feature-major (what the partition reads: ONE feature over a leaf's rows) and `packed`, the same
// matrix row-major [N][P8] (P8 = P rounded up to 8): the rows of a leaf are scattered, so the histogram kernel wants all
// features of a row next to each other — a group of DT_GBDT_HIST_GROUP = 8 features is one aligned 8-byte load per row
// instead of eight single-byte loads from eight cache lines.  idx int32 [2][N]: the rows of leaf l are
// idx[buf_l][begin_l .. begin_l + count_l); a split scatters the parent's segment into the SAME range of the other buffer
// (left rows first), so no copy back is needed and untouched leaves stay where they are.
//
// One tree is a fixed sequence of launches, none of which reads anything back: the device decides and later launches of a
// finished tree return at once (state[S_DONE]).
//   k_tree_begin   idx = 0..N-1, histograms cleared, leaf table = {root}, tree arrays reset
//   k_hist         the histogram of one segment: a block takes DT_GBDT_HIST_ROWS rows x 8 features, 8 x 256 entries of
//                  20 bytes = 40 KiB of LDS (4 blocks per CU), LDS 64-bit integer atomics, then one 64-bit global integer
//                  add per non-empty entry.  Root: all rows.  Otherwise only the SMALLER child, into the new leaf's slot;
//   k_hist_sub     the sibling is parent - child, element-wise (the left child keeps the parent's slot)
//   k_split        one block per new leaf, a wave per feature: each lane takes 4 bins, a wave scan gives the prefix sums, the
//                  lane forms the float64 gains of its 4 thresholds; ties: lower bin, then lower feature.  -> the leaf's record
//   k_grow_pick    one wave: the leaf with the largest gain (ties: lower id) becomes a node; child leaves and the job for the
//                  next launches are written to the leaf table / state
//   k_part_count, k_part_scatter   stable two-pass partition of the chosen segment by bins[f][row] <= bin
//   k_leaf_update  leaf values -lr * G / (H + lambda) (float64, rounded once to float32), scores += value, row -> leaf id
//
// Multiclass (softmax boosting, ops.gbdt_gradients_softmax / gbdt_grow_trees).  The K class trees of a round share the bin
// matrix, the packed rows and the launch sequence; only gradients, partitions and decisions differ.  So every kernel body above
// is a __device__ function of a dt_gbdt_ws, the single-tree kernels and the k_*_mc kernels are thin wrappers over it, and the
// _mc wrappers take the class from blockIdx.z and form that class's view of a dt_gbdt_mc (class 0's dt_gbdt_ws plus the
// element strides between classes; 272 bytes, passed by value).  All K trees grow in lock-step: a round costs the launches of
// ONE tree plus one k_gbdt_grad_softmax, a class that is finished returns at once while the others go on, and the host still
// reads nothing back.  Memory for K classes: 8 N K bytes of row indices and K L P 256 20 bytes of histograms (K = 10, 31
// leaves, 39 features: 62 MB), 8 N K bytes of quantised gradients.
#include "common.h"
#include "optim_dev.h"

#pragma clang fp contract(off)

namespace dt {

constexpr int kBins = DT_GBDT_BINS;
constexpr int kGroup = DT_GBDT_HIST_GROUP;
constexpr int kHistRows = DT_GBDT_HIST_ROWS;
constexpr int kThreads = 256;
constexpr int kPartPer = 8;                              // consecutive rows per thread of a partition chunk
constexpr int kPartChunk = DT_GBDT_PART_CHUNK;
static_assert(kPartChunk == kThreads * kPartPer, "a partition chunk is one block");
static_assert(kGroup == 8, "a feature group is one 8-byte load of the packed matrix");
static_assert(sizeof(dt_gbdt_ws) == DT_GBDT_WS_BYTES, "ops.py packs the workspace descriptor by this layout");
static_assert(sizeof(dt_gbdt_mc) == DT_GBDT_MC_BYTES && offsetof(dt_gbdt_mc, base) == 0, "ops.py packs the class-batched descriptor too");

// state words
enum { S_NLEAVES, S_DONE, S_LEAF, S_NEW, S_FEAT, S_BIN, S_BEGIN, S_COUNT, S_BUF, S_CL, S_SMALL, S_NNODES };
// leaf table words (int64 each)
enum { LF_BEGIN, LF_COUNT, LF_BUF, LF_WHERE, LF_G, LF_H, LF_GAIN, LF_FEAT, LF_BIN, LF_CL };
static_assert(S_NNODES < DT_GBDT_STATE_WORDS && LF_CL < DT_GBDT_LEAF_WORDS, "table sizes");

__device__ __forceinline__ double pow2(int e) {          // 2^e for |e| <= 1022
    return __longlong_as_double((long long)(1023 + e) << 52);
}

__device__ __forceinline__ int64_t shfl_up64(int64_t v, int d) {
    const int lo = __shfl_up((int)(uint32_t)v, d, 64), hi = __shfl_up((int)(v >> 32), d, 64);
    return (int64_t)(((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo);
}
__device__ __forceinline__ int64_t shfl64(int64_t v, int lane) {
    const int lo = __shfl((int)(uint32_t)v, lane, 64), hi = __shfl((int)(v >> 32), lane, 64);
    return (int64_t)(((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo);
}

// ---- binning -------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double gbdt_value(const void* src, int dtype, int64_t i) {
    switch (dtype) {
        case DT_PREP_I32: return (double)((const int32_t*)src)[i];
        case DT_PREP_I64: return __ll2double_rn(((const int64_t*)src)[i]);
        case DT_PREP_F32: return (double)((const float*)src)[i];
        default: return ((const double*)src)[i];
    }
}

__global__ __launch_bounds__(kThreads) void k_gbdt_bin(const void* __restrict__ src, int dtype, int64_t N,
                                                        const double* __restrict__ edges, int n_edges, uint8_t* __restrict__ out) {
    const int trips = n_edges > 0 ? 32 - __clz(n_edges) : 0;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < N; i += (int64_t)gridDim.x * kThreads) {
        const double v = gbdt_value(src, dtype, i);
        int lo = n_edges;                                 // a NaN: the last bin
        if (v == v) {
            lo = 0;                                       // the number of edges <= v, a fixed-trip search
            for (int t = trips - 1; t >= 0; --t) {
                const int probe = lo + (1 << t);
                if (probe <= n_edges && edges[probe - 1] <= v) lo = probe;
            }
        }
        out[i] = (uint8_t)lo;
    }
}

// packed[row][4 w .. 4 w + 3] = bins[4 w + k][row] (0 beyond P): adjacent lanes take adjacent rows, so the reads coalesce
__global__ __launch_bounds__(kThreads) void k_gbdt_pack(const uint8_t* __restrict__ bins, int64_t N, int P, int W,
                                                         uint32_t* __restrict__ packed) {
    const int64_t total = N * W;
    for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < total; e += (int64_t)gridDim.x * kThreads) {
        const int w = (int)(e / N);
        const int64_t row = e - (int64_t)w * N;
        uint32_t word = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int f = 4 * w + k;
            if (f < P) word |= (uint32_t)bins[(int64_t)f * N + row] << (8 * k);
        }
        packed[row * W + w] = word;
    }
}

// ---- gradients -------------------------------------------------------------------------------------------------------------
// regression, first launch: max |s - y| over the rows as the bit pattern of a non-negative double (ordered as integers)
__global__ __launch_bounds__(kThreads) void k_gbdt_absmax(const float* __restrict__ s, const float* __restrict__ y, int64_t N,
                                                           unsigned long long* __restrict__ slot) {
    __shared__ unsigned long long part[kThreads / kWave];
    unsigned long long m = 0;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < N; i += (int64_t)gridDim.x * kThreads) {
        const double g = fabs((double)s[i] - (double)y[i]);
        const unsigned long long b = (unsigned long long)__double_as_longlong(g);
        if (g == g && b > m) m = b;
    }
    for (int o = 32; o >= 1; o >>= 1) {
        const unsigned long long other = (unsigned long long)shfl64((int64_t)m, (threadIdx.x & 63) ^ o);
        if (other > m) m = other;
    }
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kThreads / kWave; ++w) if (part[w] > m) m = part[w];
        if (m) atomicMax(slot, m);
    }
}

// the exponent S with max * 2^S in [2^22, 2^23): max = f * 2^e, f in [0.5, 1), S = 23 - e; 0 for a zero, subnormal or
// non-finite max
__device__ __forceinline__ int scale_exponent(unsigned long long maxbits) {
    const int be = (int)((maxbits >> 52) & 0x7FF);
    if (be == 0 || be == 0x7FF) return 0;
    const int S = 23 - (be - 1022);
    return S > 1000 ? 1000 : (S < -1000 ? -1000 : S);
}

__global__ __launch_bounds__(kThreads) void k_gbdt_grad(int objective, const float* __restrict__ s, const float* __restrict__ y,
                                                         int64_t N, const unsigned long long* __restrict__ slot,
                                                         int32_t* __restrict__ sexp, int32_t* __restrict__ qg,
                                                         int32_t* __restrict__ qh) {
    const int Sg = objective == DT_GBDT_BINARY ? 23 : scale_exponent(*slot);
    const int Sh = objective == DT_GBDT_BINARY ? 25 : 0;
    if (blockIdx.x == 0 && threadIdx.x == 0) { sexp[0] = Sg; sexp[1] = Sh; }
    const double kg = pow2(Sg), kh = pow2(Sh);
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < N; i += (int64_t)gridDim.x * kThreads) {
        double g, h;
        if (objective == DT_GBDT_BINARY) {
            const double p = 1.0 / (1.0 + exp(-(double)s[i]));
            g = p - (double)y[i];
            h = p * (1.0 - p);
        } else {
            g = (double)s[i] - (double)y[i];
            h = 1.0;
        }
        const double a = rint(g * kg), b = rint(h * kh);
        qg[i] = a == a ? (int32_t)a : 0;
        qh[i] = b == b ? (int32_t)b : 0;
    }
}

// softmax cross-entropy, K class-major score rows [K][N]: one thread per row, its K scores read with stride N (the lanes of a
// wave read consecutive rows of one class, so every load and store coalesces).  The scores are read three times (max, sum,
// write) and the exponentials formed twice instead of holding K values per thread: K is a run-time number up to 64, 64 float64
// in registers are 128 VGPRs and need a compile-time K, while the re-reads hit the cache and the kernel is one launch of a
// round that issues ~180 more.  float64 in the written order: m = max, e = exp(s - m), Z = sum in class order, p = e / Z,
// g = p - [y == k], h = (K / (K - 1)) (p (1 - p)) (LightGBM's factor); h <= 0.375 for K >= 3, so |qh| < 2^24.
__global__ __launch_bounds__(kThreads) void k_gbdt_grad_softmax(const float* __restrict__ s, const float* __restrict__ y, int64_t N,
                                                                 int K, int32_t* __restrict__ sexp, int32_t* __restrict__ qg,
                                                                 int32_t* __restrict__ qh) {
    if (blockIdx.x == 0 && threadIdx.x == 0) { sexp[0] = 23; sexp[1] = 25; }
    const double kg = pow2(23), kh = pow2(25), factor = (double)K / (double)(K - 1);
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < N; i += (int64_t)gridDim.x * kThreads) {
        double m = (double)s[i];
        for (int k = 1; k < K; ++k) {
            const double v = (double)s[(int64_t)k * N + i];
            if (v > m) m = v;
        }
        double Z = 0.0;
        for (int k = 0; k < K; ++k) Z += exp((double)s[(int64_t)k * N + i] - m);
        const float label = y[i];                         // a NaN or a value outside [0, K) equals no class number
        for (int k = 0; k < K; ++k) {
            const double p = exp((double)s[(int64_t)k * N + i] - m) / Z;
            const double g = p - (label == (float)k ? 1.0 : 0.0);
            const double h = factor * (p * (1.0 - p));
            const double a = rint(g * kg), b = rint(h * kh);
            qg[(int64_t)k * N + i] = a == a ? (int32_t)a : 0;
            qh[(int64_t)k * N + i] = b == b ? (int32_t)b : 0;
        }
    }
}

// ---- one tree --------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void tree_begin_body(const dt_gbdt_ws& ws) {
    const int64_t stride = (int64_t)gridDim.x * kThreads, t0 = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    for (int64_t i = t0; i < ws.N; i += stride) ws.idx[i] = (int32_t)i;
    const int64_t entries = (int64_t)ws.L * ws.P * kBins;
    for (int64_t e = t0; e < entries; e += stride) { ws.hg[e] = 0; ws.hh[e] = 0; ws.hc[e] = 0; }
    if (blockIdx.x == 0) {
        for (int i = threadIdx.x; i < ws.L * DT_GBDT_LEAF_WORDS; i += kThreads) ws.leaf[i] = i % DT_GBDT_LEAF_WORDS == LF_FEAT ? -1 : 0;
        for (int i = threadIdx.x; i < ws.L; i += kThreads) ws.leaf_value[i] = 0.f;
        for (int i = threadIdx.x; i < ws.L - 1; i += kThreads) {
            ws.node_feat[i] = 0; ws.node_bin[i] = 0; ws.node_child[2 * i] = ~0; ws.node_child[2 * i + 1] = ~0;
        }
        for (int i = threadIdx.x; i < DT_GBDT_STATE_WORDS; i += kThreads) ws.state[i] = i == S_NLEAVES ? 1 : 0;
        __syncthreads();
        if (threadIdx.x == 0) {
            ws.leaf[LF_COUNT] = ws.N;
            ws.leaf[LF_WHERE] = -1;
            *ws.n_nodes = 0;
        }
    }
}

// grid (row chunks, feature groups).  root: the whole of buffer 0 into slot 0; otherwise the smaller child into slot S_NEW
__device__ __forceinline__ void hist_body(const dt_gbdt_ws& ws, int root) {
    __shared__ unsigned long long lg[kGroup * kBins], lh[kGroup * kBins];
    __shared__ unsigned int lc[kGroup * kBins];
    int64_t begin = 0, count = ws.N;
    int buf = 0, slot = 0;
    if (!root) {
        if (ws.state[S_DONE]) return;
        const int cl = ws.state[S_CL], small = ws.state[S_SMALL];
        begin = (int64_t)ws.state[S_BEGIN] + (small ? cl : 0);
        count = small ? ws.state[S_COUNT] - cl : cl;
        buf = 1 - ws.state[S_BUF];
        slot = ws.state[S_NEW];
    }
    const int64_t r0 = (int64_t)blockIdx.x * kHistRows;
    if (r0 >= count) return;
    const int64_t r1 = r0 + kHistRows < count ? r0 + kHistRows : count;
    for (int e = threadIdx.x; e < kGroup * kBins; e += kThreads) { lg[e] = 0; lh[e] = 0; lc[e] = 0; }
    __syncthreads();
    const int W = (ws.P + 7) / 8 * 2;                     // words per packed row
    const int f0 = blockIdx.y * kGroup;
    const int32_t* idx = ws.idx + (int64_t)buf * ws.N + begin;
    for (int64_t i = r0 + threadIdx.x; i < r1; i += kThreads) {
        const int64_t r = idx[i];
        const unsigned long long g = (unsigned long long)(long long)ws.qg[r], h = (unsigned long long)(long long)ws.qh[r];
        const uint2 w = *(const uint2*)(ws.packed + r * W + blockIdx.y * 2);
#pragma unroll
        for (int j = 0; j < kGroup; ++j) {
            if (f0 + j < ws.P) {
                const int b = ((j < 4 ? w.x : w.y) >> (8 * (j & 3))) & 0xFF;
                atomicAdd(&lg[j * kBins + b], g);
                atomicAdd(&lh[j * kBins + b], h);
                atomicAdd(&lc[j * kBins + b], 1u);
            }
        }
    }
    __syncthreads();
    const int64_t base = ((int64_t)slot * ws.P + f0) * kBins;
    for (int e = threadIdx.x; e < kGroup * kBins; e += kThreads) {
        if (f0 + e / kBins < ws.P && lc[e] != 0) {
            atomicAdd((unsigned long long*)ws.hg + base + e, lg[e]);
            atomicAdd((unsigned long long*)ws.hh + base + e, lh[e]);
            atomicAdd((unsigned int*)ws.hc + base + e, lc[e]);
        }
    }
}

// slot S_NEW holds the smaller child.  It is the right child: parent slot -= it.  It is the left child: swap roles.
__device__ __forceinline__ void hist_sub_body(const dt_gbdt_ws& ws) {
    if (ws.state[S_DONE]) return;
    const int64_t n = (int64_t)ws.P * kBins;
    const int64_t pa = (int64_t)ws.state[S_LEAF] * n, nw = (int64_t)ws.state[S_NEW] * n;
    const bool small_right = ws.state[S_SMALL] != 0;
    for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < n; e += (int64_t)gridDim.x * kThreads) {
        const int64_t g = ws.hg[nw + e], h = ws.hh[nw + e];
        const int32_t c = ws.hc[nw + e];
        if (small_right) {
            ws.hg[pa + e] -= g; ws.hh[pa + e] -= h; ws.hc[pa + e] -= c;
        } else {
            ws.hg[nw + e] = ws.hg[pa + e] - g; ws.hh[nw + e] = ws.hh[pa + e] - h; ws.hc[nw + e] = ws.hc[pa + e] - c;
            ws.hg[pa + e] = g; ws.hh[pa + e] = h; ws.hc[pa + e] = c;
        }
    }
}

struct SplitGain {
    double sg, sh, lambda, min_gain;
    // GL^2 / (HL + lambda) + GR^2 / (HR + lambda) - G^2 / (H + lambda) in this order; false: a denominator is not positive or the
    // gain does not exceed min_gain
    __device__ __forceinline__ bool operator()(int64_t GL, int64_t HL, int64_t G, int64_t H, double* gain) const {
        const double gl = __dmul_rn(__ll2double_rn(GL), sg), gr = __dmul_rn(__ll2double_rn(G - GL), sg), gt = __dmul_rn(__ll2double_rn(G), sg);
        const double hl = __dadd_rn(__dmul_rn(__ll2double_rn(HL), sh), lambda);
        const double hr = __dadd_rn(__dmul_rn(__ll2double_rn(H - HL), sh), lambda);
        const double ht = __dadd_rn(__dmul_rn(__ll2double_rn(H), sh), lambda);
        if (!(hl > 0.0 && hr > 0.0 && ht > 0.0)) return false;
        const double v = __dsub_rn(__dadd_rn(__ddiv_rn(__dmul_rn(gl, gl), hl), __ddiv_rn(__dmul_rn(gr, gr), hr)),
                                   __ddiv_rn(__dmul_rn(gt, gt), ht));
        *gain = v;
        return v > min_gain;
    }
};

// one block per leaf to evaluate (root: leaf 0; otherwise S_LEAF and S_NEW); wave w takes features w, w + 4, ...
__device__ __forceinline__ void split_body(const dt_gbdt_ws& ws, int root) {
    __shared__ double w_gain[kThreads / kWave];
    __shared__ int w_feat[kThreads / kWave], w_bin[kThreads / kWave], w_cl[kThreads / kWave];
    __shared__ int64_t w_tot[2];
    if (!root && ws.state[S_DONE]) return;
    const int leaf = root ? 0 : ws.state[blockIdx.x == 0 ? S_LEAF : S_NEW];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int minc = ws.min_child > 1 ? ws.min_child : 1;
    const SplitGain gain_of{pow2(-ws.sexp[0]), pow2(-ws.sexp[1]), ws.lambda, ws.min_gain};
    double best = 0.0;
    int bfeat = -1, bbin = 0, bcl = 0;                    // the wave's best so far (uniform over the wave)
    for (int f = wave; f < ws.P; f += kThreads / kWave) {
        const int64_t base = ((int64_t)leaf * ws.P + f) * kBins + 4 * lane;
        int64_t g[4], h[4];
        int32_t c[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) { g[k] = ws.hg[base + k]; h[k] = ws.hh[base + k]; c[k] = ws.hc[base + k]; }
        int64_t pg = g[0] + g[1] + g[2] + g[3], ph = h[0] + h[1] + h[2] + h[3];
        int32_t pc = c[0] + c[1] + c[2] + c[3];
        const int64_t mine_g = pg, mine_h = ph;
        const int32_t mine_c = pc;
        for (int d = 1; d < 64; d <<= 1) {                // inclusive scan over the lanes
            const int64_t og = shfl_up64(pg, d), oh = shfl_up64(ph, d);
            const int32_t oc = __shfl_up(pc, d, 64);
            if (lane >= d) { pg += og; ph += oh; pc += oc; }
        }
        const int64_t G = shfl64(pg, 63), H = shfl64(ph, 63);
        const int32_t C = __shfl(pc, 63, 64);
        if (f == 0 && lane == 0) { w_tot[0] = G; w_tot[1] = H; }
        int64_t GL = pg - mine_g, HL = ph - mine_h;
        int32_t CL = pc - mine_c;
        double lgain = 0.0;
        int lbin = -1, lcl = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {                     // threshold t = 4 lane + k: bins <= t go left
            GL += g[k]; HL += h[k]; CL += c[k];
            double v;
            if (4 * lane + k < kBins - 1 && CL >= minc && C - CL >= minc && gain_of(GL, HL, G, H, &v) && (lbin < 0 || v > lgain)) {
                lgain = v; lbin = 4 * lane + k; lcl = CL;
            }
        }
        for (int o = 32; o >= 1; o >>= 1) {               // max gain, ties to the lower bin
            const double og = __longlong_as_double(shfl64(__double_as_longlong(lgain), lane ^ o));
            const int ob = __shfl(lbin, lane ^ o, 64), oc = __shfl(lcl, lane ^ o, 64);
            if (ob >= 0 && (lbin < 0 || og > lgain || (og == lgain && ob < lbin))) { lgain = og; lbin = ob; lcl = oc; }
        }
        if (lbin >= 0 && (bfeat < 0 || lgain > best)) { best = lgain; bfeat = f; bbin = lbin; bcl = lcl; }
    }
    if (lane == 0) { w_gain[wave] = best; w_feat[wave] = bfeat; w_bin[wave] = bbin; w_cl[wave] = bcl; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kThreads / kWave; ++w)
            if (w_feat[w] >= 0 && (bfeat < 0 || w_gain[w] > best || (w_gain[w] == best && w_feat[w] < bfeat))) {
                best = w_gain[w]; bfeat = w_feat[w]; bbin = w_bin[w]; bcl = w_cl[w];
            }
        int64_t* lf = ws.leaf + (int64_t)leaf * DT_GBDT_LEAF_WORDS;
        lf[LF_G] = w_tot[0]; lf[LF_H] = w_tot[1];
        lf[LF_GAIN] = __double_as_longlong(best); lf[LF_FEAT] = bfeat; lf[LF_BIN] = bbin; lf[LF_CL] = bcl;
    }
}

// one wave: choose the leaf, append the node, describe the two children and the job of the next launches
__device__ __forceinline__ void grow_pick_body(const dt_gbdt_ws& ws) {
    if (ws.state[S_DONE]) return;
    const int lane = threadIdx.x, n = ws.state[S_NLEAVES];
    double best = 0.0;
    int bl = -1;
    for (int l = lane; l < n; l += kWave) {
        const int64_t* lf = ws.leaf + (int64_t)l * DT_GBDT_LEAF_WORDS;
        const double v = __longlong_as_double(lf[LF_GAIN]);
        if (lf[LF_FEAT] >= 0 && (bl < 0 || v > best)) { best = v; bl = l; }
    }
    for (int o = 32; o >= 1; o >>= 1) {
        const double og = __longlong_as_double(shfl64(__double_as_longlong(best), lane ^ o));
        const int ol = __shfl(bl, lane ^ o, 64);
        if (ol >= 0 && (bl < 0 || og > best || (og == best && ol < bl))) { best = og; bl = ol; }
    }
    if (lane != 0) return;
    if (n >= ws.L || bl < 0) { ws.state[S_DONE] = 1; return; }
    int64_t* lf = ws.leaf + (int64_t)bl * DT_GBDT_LEAF_WORDS;
    int64_t* nf = ws.leaf + (int64_t)n * DT_GBDT_LEAF_WORDS;
    const int k = ws.state[S_NNODES], feat = (int)lf[LF_FEAT], bin = (int)lf[LF_BIN], cl = (int)lf[LF_CL];
    const int begin = (int)lf[LF_BEGIN], count = (int)lf[LF_COUNT], buf = (int)lf[LF_BUF], where = (int)lf[LF_WHERE];
    ws.node_feat[k] = feat; ws.node_bin[k] = bin;
    ws.node_child[2 * k] = ~bl; ws.node_child[2 * k + 1] = ~n;
    if (where >= 0) ws.node_child[where] = k;
    lf[LF_COUNT] = cl; lf[LF_BUF] = 1 - buf; lf[LF_WHERE] = 2 * k; lf[LF_FEAT] = -1;
    nf[LF_BEGIN] = begin + cl; nf[LF_COUNT] = count - cl; nf[LF_BUF] = 1 - buf; nf[LF_WHERE] = 2 * k + 1; nf[LF_FEAT] = -1;
    ws.state[S_LEAF] = bl; ws.state[S_NEW] = n; ws.state[S_FEAT] = feat; ws.state[S_BIN] = bin;
    ws.state[S_BEGIN] = begin; ws.state[S_COUNT] = count; ws.state[S_BUF] = buf; ws.state[S_CL] = cl;
    ws.state[S_SMALL] = count - cl < cl ? 1 : 0;
    ws.state[S_NLEAVES] = n + 1; ws.state[S_NNODES] = k + 1;
    *ws.n_nodes = k + 1;
}

// the block's sum of v (every thread gets it); `red` holds one word per wave
__device__ __forceinline__ int block_sum(int v, int* red) {
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    int s = 0;
    for (int w = 0; w < kThreads / kWave; ++w) s += red[w];
    return s;
}

// chunk c = rows [c * kPartChunk, ...) of the chosen segment, thread t its rows t * 8 .. t * 8 + 7: part[c] = lefts of the chunk
__device__ __forceinline__ void part_count_body(const dt_gbdt_ws& ws) {
    __shared__ int red[kThreads / kWave];
    if (ws.state[S_DONE]) return;
    const int64_t count = ws.state[S_COUNT], base = (int64_t)blockIdx.x * kPartChunk;
    if (base >= count) return;
    const int32_t* src = ws.idx + (int64_t)ws.state[S_BUF] * ws.N + ws.state[S_BEGIN];
    const uint8_t* col = ws.bins + (int64_t)ws.state[S_FEAT] * ws.N;
    const int bin = ws.state[S_BIN];
    int mine = 0;
    for (int k = 0; k < kPartPer; ++k) {
        const int64_t i = base + (int64_t)threadIdx.x * kPartPer + k;
        if (i < count) mine += col[src[i]] <= bin ? 1 : 0;
    }
    const int total = block_sum(mine, red);
    if (threadIdx.x == 0) ws.part[blockIdx.x] = total;
}

__device__ __forceinline__ void part_scatter_body(const dt_gbdt_ws& ws) {
    __shared__ int red[kThreads / kWave], wave_tot[kThreads / kWave];
    if (ws.state[S_DONE]) return;
    const int64_t count = ws.state[S_COUNT], base = (int64_t)blockIdx.x * kPartChunk;
    if (base >= count) return;
    const int64_t begin = ws.state[S_BEGIN];
    const int buf = ws.state[S_BUF], bin = ws.state[S_BIN], cl = ws.state[S_CL];
    const int32_t* src = ws.idx + (int64_t)buf * ws.N + begin;
    int32_t* dst = ws.idx + (int64_t)(1 - buf) * ws.N + begin;
    const uint8_t* col = ws.bins + (int64_t)ws.state[S_FEAT] * ws.N;
    int before = 0;                                       // lefts in the chunks before this one
    for (int c = threadIdx.x; c < (int)blockIdx.x; c += kThreads) before += ws.part[c];
    before = block_sum(before, red);
    int32_t row[kPartPer];
    unsigned flags = 0;
    int mine = 0;
    const int64_t i0 = base + (int64_t)threadIdx.x * kPartPer;
    for (int k = 0; k < kPartPer; ++k) {
        if (i0 + k < count) {
            row[k] = src[i0 + k];
            if (col[row[k]] <= bin) { flags |= 1u << k; ++mine; }
        }
    }
    int incl = mine;                                      // lefts of the threads before this one in the block
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(incl, d, 64);
        if (lane >= d) incl += o;
    }
    if (lane == 63) wave_tot[wave] = incl;
    __syncthreads();
    int lefts = before + incl - mine;
    for (int w = 0; w < wave; ++w) lefts += wave_tot[w];
    for (int k = 0; k < kPartPer; ++k) {
        const int64_t i = i0 + k;
        if (i >= count) break;
        const bool left = (flags >> k) & 1u;
        const int64_t pos = left ? lefts : cl + (i - lefts);
        if (pos < count) dst[pos] = row[k];               // (always, when S_CL is the histogram's count of these flags)
        lefts += left ? 1 : 0;
    }
}

__device__ __forceinline__ void leaf_update_body(const dt_gbdt_ws& ws, float* __restrict__ scores, int32_t* __restrict__ row_leaf) {
    extern __shared__ int64_t tab[];                      // per leaf: begin, end, buf, value bits
    const int n = ws.state[S_NLEAVES];
    const double sg = pow2(-ws.sexp[0]), sh = pow2(-ws.sexp[1]);
    for (int l = threadIdx.x; l < n; l += kThreads) {
        const int64_t* lf = ws.leaf + (int64_t)l * DT_GBDT_LEAF_WORDS;
        const double den = __dadd_rn(__dmul_rn(__ll2double_rn(lf[LF_H]), sh), ws.lambda);
        const double v = den > 0.0 ? -__dmul_rn(ws.lr, __ddiv_rn(__dmul_rn(__ll2double_rn(lf[LF_G]), sg), den)) : 0.0;
        const float vf = __double2float_rn(v);
        tab[4 * l] = lf[LF_BEGIN]; tab[4 * l + 1] = lf[LF_BEGIN] + lf[LF_COUNT]; tab[4 * l + 2] = lf[LF_BUF];
        tab[4 * l + 3] = __float_as_int(vf);
        if (blockIdx.x == 0) ws.leaf_value[l] = vf;
    }
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < ws.N; i += (int64_t)gridDim.x * kThreads) {
        for (int l = 0; l < n; ++l) {
            if (i >= tab[4 * l] && i < tab[4 * l + 1]) {
                const int64_t r = ws.idx[tab[4 * l + 2] * ws.N + i];
                row_leaf[r] = l;
                scores[r] = __fadd_rn(scores[r], __int_as_float((int)tab[4 * l + 3]));
                break;
            }
        }
    }
}

// ---- the launches: one tree, or the K class trees of a softmax round in lock-step --------------------------------------------
// class c's view of a class-batched workspace: the shared bins / packed / sexp / sizes / parameters, its own everything else
__device__ __forceinline__ dt_gbdt_ws class_view(const dt_gbdt_mc& m, int c) {
    dt_gbdt_ws ws = m.base;
    ws.qg += c * m.q_stride; ws.qh += c * m.q_stride;
    ws.idx += c * m.idx_stride;
    ws.hg += c * m.hist_stride; ws.hh += c * m.hist_stride; ws.hc += c * m.hist_stride;
    ws.leaf += c * m.leaf_stride;
    ws.state += c * m.state_stride;
    ws.part += c * m.part_stride;
    ws.node_feat += c * m.node_stride; ws.node_bin += c * m.node_stride; ws.node_child += 2 * c * m.node_stride;
    ws.leaf_value += c * m.value_stride;
    ws.n_nodes += c * m.nn_stride;
    return ws;
}

__global__ __launch_bounds__(kThreads) void k_tree_begin(dt_gbdt_ws ws) { tree_begin_body(ws); }
__global__ __launch_bounds__(kThreads) void k_hist(dt_gbdt_ws ws, int root) { hist_body(ws, root); }
__global__ __launch_bounds__(kThreads) void k_hist_sub(dt_gbdt_ws ws) { hist_sub_body(ws); }
__global__ __launch_bounds__(kThreads) void k_split(dt_gbdt_ws ws, int root) { split_body(ws, root); }
__global__ __launch_bounds__(kWave) void k_grow_pick(dt_gbdt_ws ws) { grow_pick_body(ws); }
__global__ __launch_bounds__(kThreads) void k_part_count(dt_gbdt_ws ws) { part_count_body(ws); }
__global__ __launch_bounds__(kThreads) void k_part_scatter(dt_gbdt_ws ws) { part_scatter_body(ws); }
__global__ __launch_bounds__(kThreads) void k_leaf_update(dt_gbdt_ws ws, float* __restrict__ scores, int32_t* __restrict__ row_leaf) {
    leaf_update_body(ws, scores, row_leaf);
}

// the same bodies with the class as blockIdx.z: x and y keep their single-tree meaning, a finished class's blocks return at once
__global__ __launch_bounds__(kThreads) void k_tree_begin_mc(dt_gbdt_mc m) { tree_begin_body(class_view(m, blockIdx.z)); }
__global__ __launch_bounds__(kThreads) void k_hist_mc(dt_gbdt_mc m, int root) { hist_body(class_view(m, blockIdx.z), root); }
__global__ __launch_bounds__(kThreads) void k_hist_sub_mc(dt_gbdt_mc m) { hist_sub_body(class_view(m, blockIdx.z)); }
__global__ __launch_bounds__(kThreads) void k_split_mc(dt_gbdt_mc m, int root) { split_body(class_view(m, blockIdx.z), root); }
__global__ __launch_bounds__(kWave) void k_grow_pick_mc(dt_gbdt_mc m) { grow_pick_body(class_view(m, blockIdx.z)); }
__global__ __launch_bounds__(kThreads) void k_part_count_mc(dt_gbdt_mc m) { part_count_body(class_view(m, blockIdx.z)); }
__global__ __launch_bounds__(kThreads) void k_part_scatter_mc(dt_gbdt_mc m) { part_scatter_body(class_view(m, blockIdx.z)); }
__global__ __launch_bounds__(kThreads) void k_leaf_update_mc(dt_gbdt_mc m, float* __restrict__ scores, int32_t* __restrict__ row_leaf) {
    const int64_t c = blockIdx.z;
    leaf_update_body(class_view(m, blockIdx.z), scores + c * m.row_stride, row_leaf + c * m.row_stride);
}

// ---- prediction ------------------------------------------------------------------------------------------------------------
// grid (row tiles, tree tiles); the node arrays of `tile` trees sit in LDS; one thread walks one (row, tree); adjacent
// threads take adjacent trees of one row, so the stores of out [N][T] coalesce and the row's packed bins are shared
__global__ __launch_bounds__(kThreads) void k_predict_leaves(const uint8_t* __restrict__ packed, int64_t N, int P8, int T, int L,
                                                              int tile, const int32_t* __restrict__ node_feat,
                                                              const int32_t* __restrict__ node_bin, const int32_t* __restrict__ node_child,
                                                              const int32_t* __restrict__ n_nodes, int32_t* __restrict__ out) {
    extern __shared__ int32_t nodes[];                    // [tile][L - 1] x (feat, bin, left, right), then n_nodes [tile]
    const int M = L - 1, t0 = blockIdx.y * tile;
    const int nt = T - t0 < tile ? T - t0 : tile;
    for (int e = threadIdx.x; e < nt * M; e += kThreads) {
        const int64_t s = (int64_t)t0 * M + e;
        nodes[4 * e] = node_feat[s]; nodes[4 * e + 1] = node_bin[s];
        nodes[4 * e + 2] = node_child[2 * s]; nodes[4 * e + 3] = node_child[2 * s + 1];
    }
    int32_t* nn = nodes + 4 * tile * M;
    for (int e = threadIdx.x; e < nt; e += kThreads) nn[e] = n_nodes[t0 + e];
    __syncthreads();
    const int64_t r0 = (int64_t)blockIdx.x * DT_GBDT_PREDICT_ROWS;
    const int64_t rows = N - r0 < DT_GBDT_PREDICT_ROWS ? N - r0 : DT_GBDT_PREDICT_ROWS;
    for (int64_t e = threadIdx.x; e < rows * nt; e += kThreads) {
        const int64_t row = r0 + e / nt;
        const int t = (int)(e % nt);
        const uint8_t* x = packed + row * P8;
        const int32_t* nd = nodes + 4 * t * M;
        int leaf = 0, cur = 0;
        if (nn[t] > 0) {
            for (int depth = 0; depth < M; ++depth) {     // a tree of M nodes is at most M deep
                const int f = (unsigned)nd[4 * cur] < (unsigned)P8 ? nd[4 * cur] : 0;
                const int c = nd[4 * cur + 2 + (x[f] > nd[4 * cur + 1] ? 1 : 0)];
                if (c < 0) { leaf = ~c; break; }
                cur = c < M ? c : 0;
            }
        }
        out[row * T + t0 + t] = leaf;
    }
}

static int check_ws(const char* who, const dt_gbdt_ws* ws) {
    DT_REQUIRE(ws, "%s: null workspace descriptor", who);
    DT_REQUIRE(ws->N >= 1 && ws->N <= DT_GBDT_MAX_ROWS, "%s: N=%lld outside [1, %d]", who, (long long)ws->N, DT_GBDT_MAX_ROWS);
    DT_REQUIRE(ws->P >= 1 && ws->P <= DT_GBDT_MAX_FEATURES, "%s: P=%d outside [1, %d]", who, ws->P, DT_GBDT_MAX_FEATURES);
    DT_REQUIRE(ws->L >= 2 && ws->L <= DT_GBDT_MAX_LEAVES, "%s: num_leaves=%d outside [2, %d]", who, ws->L, DT_GBDT_MAX_LEAVES);
    DT_REQUIRE(ws->min_child >= 0, "%s: min_child_samples=%d", who, ws->min_child);
    DT_REQUIRE(ws->lambda >= 0.0 && ws->min_gain >= 0.0 && ws->lr == ws->lr, "%s: reg_lambda and min_split_gain must be >= 0", who);
    DT_REQUIRE(ws->bins && ws->packed && ws->qg && ws->qh && ws->sexp && ws->idx && ws->hg && ws->hh && ws->hc && ws->leaf &&
               ws->state && ws->part && ws->node_feat && ws->node_bin && ws->node_child && ws->leaf_value && ws->n_nodes,
               "%s: null pointer in the workspace descriptor", who);
    DT_REQUIRE(aligned_to(ws->packed, 8) && aligned_to(ws->hg, 8) && aligned_to(ws->hh, 8) && aligned_to(ws->leaf, 8) &&
               aligned_to(ws->qg, 4) && aligned_to(ws->qh, 4) && aligned_to(ws->idx, 4) && aligned_to(ws->hc, 4),
               "%s: misaligned pointer in the workspace descriptor", who);
    return DT_OK;
}

// the class-batched descriptor: class 0's view passes check_ws, and no class's tables reach into the next class's
static int check_mc(const char* who, const dt_gbdt_mc* m) {
    DT_REQUIRE(m, "%s: null workspace descriptor", who);
    const int rc = check_ws(who, &m->base);
    if (rc != DT_OK) return rc;
    const dt_gbdt_ws& ws = m->base;
    DT_REQUIRE(m->K >= 1 && m->K <= DT_GBDT_MAX_CLASSES, "%s: K=%d outside [1, %d]", who, m->K, DT_GBDT_MAX_CLASSES);
    const int64_t hist = (int64_t)ws.L * ws.P * kBins, chunks = (ws.N + kPartChunk - 1) / kPartChunk;
    DT_REQUIRE(m->q_stride >= ws.N && m->idx_stride >= 2 * ws.N && m->hist_stride >= hist &&
               m->leaf_stride >= (int64_t)ws.L * DT_GBDT_LEAF_WORDS && m->state_stride >= DT_GBDT_STATE_WORDS &&
               m->part_stride >= chunks && m->node_stride >= ws.L - 1 && m->value_stride >= ws.L && m->nn_stride >= 1 &&
               m->row_stride >= ws.N, "%s: a class stride is smaller than one class's table", who);
    return DT_OK;
}

static unsigned grid_for(int64_t items, int per_block, int64_t cap) {
    int64_t b = (items + per_block - 1) / per_block;
    return (unsigned)(b < 1 ? 1 : (b > cap ? cap : b));
}

}  // namespace dt

using namespace dt;

extern "C" int dt_gbdt_bin(const void* src, int dtype, int64_t N, const double* edges, int n_edges, void* out, void* stream) {
    const char* who = "dt_gbdt_bin";
    DT_REQUIRE(N >= 0 && n_edges >= 0 && n_edges < kBins, "%s: bad sizes N=%lld n_edges=%d (at most %d)", who, (long long)N, n_edges,
               kBins - 1);
    DT_REQUIRE(dtype == DT_PREP_I32 || dtype == DT_PREP_I64 || dtype == DT_PREP_F32 || dtype == DT_PREP_F64,
               "%s: dtype code %d is not int32, int64, float32 or float64", who, dtype);
    if (N == 0) return DT_OK;
    DT_REQUIRE(src && out && (edges || n_edges == 0), "%s: null pointer", who);
    DT_REQUIRE(aligned_to(src, dtype == DT_PREP_I32 || dtype == DT_PREP_F32 ? 4 : 8) && aligned_to(edges, 8), "%s: misaligned pointer", who);
    hipLaunchKernelGGL(k_gbdt_bin, dim3(grid_for(N, kThreads, 4096)), dim3(kThreads), 0, as_stream(stream), src, dtype, N, edges,
                       n_edges, (uint8_t*)out);
    return launch_status(who);
}

extern "C" int dt_gbdt_pack(const void* bins, int64_t N, int P, void* packed, void* stream) {
    const char* who = "dt_gbdt_pack";
    DT_REQUIRE(N >= 0 && N <= DT_GBDT_MAX_ROWS && P >= 1 && P <= DT_GBDT_MAX_FEATURES, "%s: bad sizes N=%lld P=%d", who, (long long)N, P);
    if (N == 0) return DT_OK;
    DT_REQUIRE(bins && packed && aligned_to(packed, 8), "%s: null or misaligned pointer", who);
    const int W = (P + 7) / 8 * 2;
    hipLaunchKernelGGL(k_gbdt_pack, dim3(grid_for(N * W, kThreads, 8192)), dim3(kThreads), 0, as_stream(stream), (const uint8_t*)bins, N,
                       P, W, (uint32_t*)packed);
    return launch_status(who);
}

extern "C" int dt_gbdt_grad(int objective, const float* scores, const float* y, int64_t N, void* max_slot, int32_t* sexp, int32_t* qg,
                            int32_t* qh, void* stream) {
    const char* who = "dt_gbdt_grad";
    DT_REQUIRE(objective == DT_GBDT_BINARY || objective == DT_GBDT_REGRESSION, "%s: unknown objective %d", who, objective);
    DT_REQUIRE(N >= 1, "%s: N=%lld", who, (long long)N);
    DT_REQUIRE(scores && y && sexp && qg && qh && max_slot, "%s: null pointer", who);
    DT_REQUIRE(aligned_to(scores, 4) && aligned_to(y, 4) && aligned_to(sexp, 4) && aligned_to(qg, 4) && aligned_to(qh, 4) &&
               aligned_to(max_slot, 8), "%s: misaligned pointer", who);
    const unsigned grid = grid_for(N, kThreads, 2048);
    if (objective == DT_GBDT_REGRESSION) {
        hipLaunchKernelGGL(k_gbdt_absmax, dim3(grid), dim3(kThreads), 0, as_stream(stream), scores, y, N, (unsigned long long*)max_slot);
        const int rc = launch_status(who);
        if (rc != DT_OK) return rc;
    }
    hipLaunchKernelGGL(k_gbdt_grad, dim3(grid), dim3(kThreads), 0, as_stream(stream), objective, scores, y, N,
                       (const unsigned long long*)max_slot, sexp, qg, qh);
    return launch_status(who);
}

extern "C" int dt_gbdt_tree_begin(const dt_gbdt_ws* ws, void* stream) {
    const char* who = "dt_gbdt_tree_begin";
    const int rc = check_ws(who, ws);
    if (rc != DT_OK) return rc;
    const int64_t items = ws->N > (int64_t)ws->L * ws->P * kBins ? ws->N : (int64_t)ws->L * ws->P * kBins;
    hipLaunchKernelGGL(k_tree_begin, dim3(grid_for(items, kThreads, 2048)), dim3(kThreads), 0, as_stream(stream), *ws);
    return launch_status(who);
}

extern "C" int dt_gbdt_hist(const dt_gbdt_ws* ws, int root, void* stream) {
    const char* who = "dt_gbdt_hist";
    const int rc = check_ws(who, ws);
    if (rc != DT_OK) return rc;
    const int64_t rows = root ? ws->N : ws->N / 2;        // the smaller child has at most half of its parent's rows
    if (rows > 0) {
        hipLaunchKernelGGL(k_hist, dim3(grid_for(rows, kHistRows, INT32_MAX), (ws->P + kGroup - 1) / kGroup), dim3(kThreads), 0,
                           as_stream(stream), *ws, root ? 1 : 0);
        const int rc2 = launch_status(who);
        if (rc2 != DT_OK) return rc2;
    }
    if (!root) hipLaunchKernelGGL(k_hist_sub, dim3(grid_for((int64_t)ws->P * kBins, kThreads, 1024)), dim3(kThreads), 0, as_stream(stream), *ws);
    return launch_status(who);
}

extern "C" int dt_gbdt_split(const dt_gbdt_ws* ws, int root, void* stream) {
    const char* who = "dt_gbdt_split";
    const int rc = check_ws(who, ws);
    if (rc != DT_OK) return rc;
    hipLaunchKernelGGL(k_split, dim3(root ? 1 : 2), dim3(kThreads), 0, as_stream(stream), *ws, root ? 1 : 0);
    return launch_status(who);
}

extern "C" int dt_gbdt_grow(const dt_gbdt_ws* ws, void* stream) {
    const char* who = "dt_gbdt_grow";
    int rc = check_ws(who, ws);
    if (rc != DT_OK) return rc;
    hipLaunchKernelGGL(k_grow_pick, dim3(1), dim3(kWave), 0, as_stream(stream), *ws);
    if ((rc = launch_status(who)) != DT_OK) return rc;
    const unsigned chunks = grid_for(ws->N, kPartChunk, INT32_MAX);
    hipLaunchKernelGGL(k_part_count, dim3(chunks), dim3(kThreads), 0, as_stream(stream), *ws);
    if ((rc = launch_status(who)) != DT_OK) return rc;
    hipLaunchKernelGGL(k_part_scatter, dim3(chunks), dim3(kThreads), 0, as_stream(stream), *ws);
    return launch_status(who);
}

extern "C" int dt_gbdt_leaf_update(const dt_gbdt_ws* ws, float* scores, int32_t* row_leaf, void* stream) {
    const char* who = "dt_gbdt_leaf_update";
    const int rc = check_ws(who, ws);
    if (rc != DT_OK) return rc;
    DT_REQUIRE(scores && row_leaf && aligned_to(scores, 4) && aligned_to(row_leaf, 4), "%s: null or misaligned pointer", who);
    hipLaunchKernelGGL(k_leaf_update, dim3(grid_for(ws->N, kThreads, 2048)), dim3(kThreads), (size_t)ws->L * 4 * sizeof(int64_t),
                       as_stream(stream), *ws, scores, row_leaf);
    return launch_status(who);
}

extern "C" int dt_gbdt_grad_softmax(const float* scores, const float* y, int64_t N, int K, int32_t* sexp, int32_t* qg, int32_t* qh,
                                    void* stream) {
    const char* who = "dt_gbdt_grad_softmax";
    DT_UNSUPPORTED(K < 3 || K > DT_GBDT_MAX_CLASSES, "%s: K=%d outside [3, %d] (two classes are the binary objective)", who, K,
                   DT_GBDT_MAX_CLASSES);
    DT_REQUIRE(N >= 1 && N <= DT_GBDT_MAX_ROWS, "%s: N=%lld", who, (long long)N);
    DT_REQUIRE(scores && y && sexp && qg && qh, "%s: null pointer", who);
    DT_REQUIRE(aligned_to(scores, 4) && aligned_to(y, 4) && aligned_to(sexp, 4) && aligned_to(qg, 4) && aligned_to(qh, 4),
               "%s: misaligned pointer", who);
    hipLaunchKernelGGL(k_gbdt_grad_softmax, dim3(grid_for(N, kThreads, 2048)), dim3(kThreads), 0, as_stream(stream), scores, y, N, K,
                       sexp, qg, qh);
    return launch_status(who);
}

// the class-batched launches: the grids of the single-tree entry points with K as the z dimension
extern "C" int dt_gbdt_mc_tree_begin(const dt_gbdt_mc* m, void* stream) {
    const char* who = "dt_gbdt_mc_tree_begin";
    const int rc = check_mc(who, m);
    if (rc != DT_OK) return rc;
    const dt_gbdt_ws* ws = &m->base;
    const int64_t items = ws->N > (int64_t)ws->L * ws->P * kBins ? ws->N : (int64_t)ws->L * ws->P * kBins;
    hipLaunchKernelGGL(k_tree_begin_mc, dim3(grid_for(items, kThreads, 2048), 1, m->K), dim3(kThreads), 0, as_stream(stream), *m);
    return launch_status(who);
}

extern "C" int dt_gbdt_mc_hist(const dt_gbdt_mc* m, int root, void* stream) {
    const char* who = "dt_gbdt_mc_hist";
    const int rc = check_mc(who, m);
    if (rc != DT_OK) return rc;
    const dt_gbdt_ws* ws = &m->base;
    const int64_t rows = root ? ws->N : ws->N / 2;
    if (rows > 0) {
        hipLaunchKernelGGL(k_hist_mc, dim3(grid_for(rows, kHistRows, INT32_MAX), (ws->P + kGroup - 1) / kGroup, m->K), dim3(kThreads), 0,
                           as_stream(stream), *m, root ? 1 : 0);
        const int rc2 = launch_status(who);
        if (rc2 != DT_OK) return rc2;
    }
    if (!root) hipLaunchKernelGGL(k_hist_sub_mc, dim3(grid_for((int64_t)ws->P * kBins, kThreads, 1024), 1, m->K), dim3(kThreads), 0,
                                  as_stream(stream), *m);
    return launch_status(who);
}

extern "C" int dt_gbdt_mc_split(const dt_gbdt_mc* m, int root, void* stream) {
    const char* who = "dt_gbdt_mc_split";
    const int rc = check_mc(who, m);
    if (rc != DT_OK) return rc;
    hipLaunchKernelGGL(k_split_mc, dim3(root ? 1 : 2, 1, m->K), dim3(kThreads), 0, as_stream(stream), *m, root ? 1 : 0);
    return launch_status(who);
}

extern "C" int dt_gbdt_mc_grow(const dt_gbdt_mc* m, void* stream) {
    const char* who = "dt_gbdt_mc_grow";
    int rc = check_mc(who, m);
    if (rc != DT_OK) return rc;
    hipLaunchKernelGGL(k_grow_pick_mc, dim3(1, 1, m->K), dim3(kWave), 0, as_stream(stream), *m);
    if ((rc = launch_status(who)) != DT_OK) return rc;
    const unsigned chunks = grid_for(m->base.N, kPartChunk, INT32_MAX);
    hipLaunchKernelGGL(k_part_count_mc, dim3(chunks, 1, m->K), dim3(kThreads), 0, as_stream(stream), *m);
    if ((rc = launch_status(who)) != DT_OK) return rc;
    hipLaunchKernelGGL(k_part_scatter_mc, dim3(chunks, 1, m->K), dim3(kThreads), 0, as_stream(stream), *m);
    return launch_status(who);
}

extern "C" int dt_gbdt_mc_leaf_update(const dt_gbdt_mc* m, float* scores, int32_t* row_leaf, void* stream) {
    const char* who = "dt_gbdt_mc_leaf_update";
    const int rc = check_mc(who, m);
    if (rc != DT_OK) return rc;
    DT_REQUIRE(scores && row_leaf && aligned_to(scores, 4) && aligned_to(row_leaf, 4), "%s: null or misaligned pointer", who);
    hipLaunchKernelGGL(k_leaf_update_mc, dim3(grid_for(m->base.N, kThreads, 2048), 1, m->K), dim3(kThreads),
                       (size_t)m->base.L * 4 * sizeof(int64_t), as_stream(stream), *m, scores, row_leaf);
    return launch_status(who);
}

extern "C" int dt_gbdt_predict_leaves(const void* packed, int64_t N, int P, int T, int L, const int32_t* node_feat,
                                      const int32_t* node_bin, const int32_t* node_child, const int32_t* n_nodes, int32_t* out,
                                      void* stream) {
    const char* who = "dt_gbdt_predict_leaves";
    DT_REQUIRE(N >= 0 && N <= DT_GBDT_MAX_ROWS && P >= 1 && P <= DT_GBDT_MAX_FEATURES && T >= 1 && L >= 2 && L <= DT_GBDT_MAX_LEAVES,
               "%s: bad sizes N=%lld P=%d T=%d num_leaves=%d", who, (long long)N, P, T, L);
    DT_REQUIRE(N <= INT64_MAX / 4 / T, "%s: N=%lld x T=%d overflows", who, (long long)N, T);
    if (N == 0) return DT_OK;
    DT_REQUIRE(packed && node_feat && node_bin && node_child && n_nodes && out, "%s: null pointer", who);
    DT_REQUIRE(aligned_to(node_feat, 4) && aligned_to(node_bin, 4) && aligned_to(node_child, 4) && aligned_to(n_nodes, 4) &&
               aligned_to(out, 4), "%s: misaligned pointer", who);
    const int per_tree = 16 * (L - 1) + 4;                // bytes of LDS per tree of a tile
    int tile = DT_GBDT_PREDICT_LDS_BYTES / per_tree;      // >= 2 for every L <= DT_GBDT_MAX_LEAVES
    if (tile > T) tile = T;
    if (tile > kThreads) tile = kThreads;
    const int64_t row_tiles = (N + DT_GBDT_PREDICT_ROWS - 1) / DT_GBDT_PREDICT_ROWS;
    DT_REQUIRE(row_tiles <= INT32_MAX && (T + tile - 1) / tile <= 65535, "%s: grid too large", who);
    hipLaunchKernelGGL(k_predict_leaves, dim3((unsigned)row_tiles, (T + tile - 1) / tile), dim3(kThreads), (size_t)tile * per_tree,
                       as_stream(stream), (const uint8_t*)packed, N, (P + 7) / 8 * 8, T, L, tile, node_feat, node_bin, node_child, n_nodes,
                       out);
    return launch_status(who);
}
