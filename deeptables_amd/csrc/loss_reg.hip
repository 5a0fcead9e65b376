// loss_reg.hip — the regression losses of Keras (Huber, log-cosh, MSLE, MAPE, Poisson) and the GHM-C loss of the layers
// module on the device (gfx950, wave64): value and gradient in a few launches (include/dt_hip.h: dt_loss_reg, dt_ghmc).
//
// dt_loss_reg has dt_loss' element-wise geometry (loss_sum.h): a block of 256 threads takes 2048 consecutive elements of the
// flat [rows * classes] array, thread t the elements t, t + 256, ... (coalesced); per-element math is float32, every sum is
// float64 in a fixed order, one double per block goes into the workspace and k_loss_total adds them; one block that covers the
// problem writes the loss itself.  No float atomics, nothing zeroed beforehand, the same bits with and without dz.
//
// log-cosh: Keras writes e + softplus(-2e) - ln 2, which cancels for small e (the value is e^2 / 2, the float32 form carries
// ~1e-7 absolute).  Here log cosh e = log1p(2 sinh^2(e / 2)) for |e| < 10 — no cancellation, relative accuracy of a few ulp at
// every magnitude — and |e| - ln 2 above, where exp(-2|e|) < 2^-28 of the result.
//
// dt_ghmc (GHMCLoss.calc) works over the n = rows * classes elements, 2048 per block:
//   pass 1  k_ghmc_count   the bin of every element from g = |sigmoid(z) - t| (arithmetic guess, corrected against the two
//                          float32 edges), integer counts per bin by LDS atomics, written at the block's index; with a mask
//                          also the count of mask > 0
//   pass 2  k_ghmc_bins    one block: the counts added in index order (exact integers), nvalid, tot, the in-place momentum
//                          update of acc_sum for the non-empty bins, the bin weights into the workspace
//   pass 3  k_ghmc_elem    the bin again by the same instructions, f = BCE from the logit, the float64 partial of f w, dz
//   pass 4  k_ghmc_total   the partials in order, divided by tot
// and a problem that one block covers is one launch (k_ghmc_one: the same steps behind block barriers).  The only atomics are
// integer LDS atomics, whose result does not depend on their order.
#include "loss_sum.h"

namespace dt {
namespace {

constexpr int64_t kMaxRows = (int64_t)1 << 31;
constexpr int64_t kMaxElems = (int64_t)1 << 40;   // rows * classes: the block count of a launch stays below 2^31
constexpr float kEps = 1e-7f;                     // keras.backend.epsilon()
constexpr float kLn2 = 0.6931471805599453f;
constexpr float kLogCoshSwitch = 10.f;

inline bool shape_ok(int64_t rows, int classes) {
    return rows >= 1 && rows < kMaxRows && classes >= 1 && classes <= DT_LOSS_MAX_CLASSES && rows * classes < kMaxElems;
}
inline int64_t elem_blocks(int64_t n) { return (n + kElemChunk - 1) / kElemChunk; }

// ---------------------------------------------------------------------------------------------------------------------------
// the five element-wise kinds
// ---------------------------------------------------------------------------------------------------------------------------
struct RegArgs {
    const float* p;          // predictions [rows * classes]
    const float* t;
    const float* w;          // [rows] or null
    float* dz;               // [rows * classes] or null
    float* loss;             // [1]
    double* partial;         // one double per block
    int64_t n;
    int classes;
    int final;               // the launch has one block, which writes the loss itself
    float delta;             // Huber
    float scale;             // fl(1 / (rows classes)): dz = w_b * scale * g
    double inv;              // the same in double: loss = inv * sum
};

template <int KIND>
__device__ __forceinline__ void reg_elem(float p, float t, float delta, float* f, float* g) {
    if (KIND == DT_LOSS_HUBER) {
        const float e = p - t, a = fabsf(e);
        const bool quad = a <= delta;
        *f = quad ? 0.5f * e * e : delta * a - 0.5f * delta * delta;
        *g = quad ? e : (e > 0.f ? delta : -delta);
    } else if (KIND == DT_LOSS_LOG_COSH) {
        const float e = p - t, a = fabsf(e);
        const float s = sinhf(0.5f * fminf(a, kLogCoshSwitch));
        *f = a < kLogCoshSwitch ? log1pf(2.f * s * s) : a - kLn2;
        *g = tanhf(e);
    } else if (KIND == DT_LOSS_MSLE) {
        const float pc = fmaxf(p, kEps), tc = fmaxf(t, kEps);
        const float d = log1pf(pc) - log1pf(tc);
        *f = d * d;
        *g = p >= kEps ? 2.f * d / (pc + 1.f) : 0.f;
    } else if (KIND == DT_LOSS_MAPE) {
        const float e = p - t;
        const float d = fmaxf(fabsf(t), kEps);
        *f = 100.f * fabsf(e) / d;
        *g = e > 0.f ? 100.f / d : (e < 0.f ? -100.f / d : 0.f);
    } else {                                                           // DT_LOSS_POISSON
        const float q = p + kEps;
        *f = p - t * logf(q);                                          // q < 0: NaN, as in Keras
        *g = 1.f - t / q;
    }
}

template <int KIND>
__global__ __launch_bounds__(kThreads) void k_loss_reg(RegArgs a) {
    __shared__ double sh[kWaves];
    const int64_t lo = (int64_t)blockIdx.x * kElemChunk;
    const int64_t rest = a.n - lo;
    const int m = rest < kElemChunk ? (int)rest : kElemChunk;          // >= 1: the host counts ceil(n / kElemChunk) blocks
    const int C = a.classes;
    double s = 0;
    for (int i = threadIdx.x; i < m; i += kThreads) {
        const int64_t e = lo + i;                                       // < n
        const float wb = a.w ? a.w[e / C] : 1.f;                        // e / C < rows
        float f, g;
        reg_elem<KIND>(a.p[e], a.t[e], a.delta, &f, &g);
        s += (double)wb * (double)f;
        if (a.dz) a.dz[e] = (wb * a.scale) * g;
    }
    s = wave_sum_f64(s);
    const double all = waves_in_order(s, sh);
    if (threadIdx.x == 0) {
        if (a.final) a.loss[0] = (float)(all * a.inv);
        else a.partial[blockIdx.x] = all;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// GHM-C
// ---------------------------------------------------------------------------------------------------------------------------
constexpr int kMaxBins = DT_GHMC_MAX_BINS;

// the workspace behind the per-block partials: per-block counts [blocks][bins + 1] (the last one: mask > 0), then the tables
struct GhmcTables {
    float w[kMaxBins + 1];       // the bin weights; [bins]: the weight of an element in no bin, 0 / nvalid
    float wdz[kMaxBins + 1];     // w / tot
    float tot;
    float pad;
};

struct GhmcArgs {
    const float* z;
    const float* t;
    const float* mask;           // [n] or null
    float* acc;                  // [bins], momentum > 0
    float* loss;
    float* dz;                   // [n] or null
    double* partial;             // [blocks]
    unsigned* counts;            // [blocks][bins + 1]
    GhmcTables* tab;
    int64_t n;
    int64_t blocks;
    int bins;
    float momentum, one_minus;   // one_minus = fl(1 - momentum) as the caller rounds it
};

// edge[b] = L_b = fl(b / bins) for b < bins, which is also R_{b-1}; edge[bins] = R_{bins-1} = fl(1 + 1e-6)
__device__ __forceinline__ void ghmc_edges(float* edge, int bins) {
    for (int b = threadIdx.x; b <= bins; b += kThreads)
        edge[b] = b < bins ? (float)((double)b / (double)bins) : (float)(1.0 + 1e-6);
}

// the bin of an element, or `bins` when it lies in none (g > 1 + 1e-6: an ignored target; a NaN) or is masked out
__device__ __forceinline__ int ghmc_bin(float z, float t, const float* mask, int64_t e, const float* edge, int bins,
                                        float* diff) {
    const float d = sigmoid_f(z) - t;
    *diff = d;
    const float g = fabsf(d);
    if (mask && !(mask[e] > 0.f)) return bins;
    if (!(g < edge[bins])) return bins;
    int b = (int)(g * (float)bins);
    b = b < bins - 1 ? b : bins - 1;
    if (g < edge[b]) --b;                                              // (g >= 0 = edge[0]: b stays >= 0)
    else if (g >= edge[b + 1]) ++b;                                    // (g < edge[bins]: b stays < bins)
    return (g >= edge[b] && g < edge[b + 1]) ? b : bins;
}

__device__ __forceinline__ void ghmc_count_block(const GhmcArgs& a, const float* edge, unsigned* hist, int64_t lo, int m) {
    for (int i = threadIdx.x; i < m; i += kThreads) {
        const int64_t e = lo + i;
        float d;
        const int b = ghmc_bin(a.z[e], a.t[e], a.mask, e, edge, a.bins, &d);
        if (b < a.bins) atomicAdd(&hist[b], 1u);
        if (a.mask && a.mask[e] > 0.f) atomicAdd(&hist[a.bins], 1u);
    }
}

// from the total counts in cnt[0 .. bins] (LDS) to the tables in `w`, `wdz` (LDS, bins + 1 entries) and *tot; updates acc_sum
__device__ __forceinline__ void ghmc_weights(const GhmcArgs& a, const unsigned long long* cnt, int* nvalid_sh, float* w,
                                             float* wdz, float* tot_sh) {
    const int bins = a.bins;
    if (threadIdx.x == 0) {
        int nv = 0;
        for (int b = 0; b < bins; ++b) nv += cnt[b] > 0;
        *nvalid_sh = nv;
        const float tot = a.mask ? (float)cnt[bins] : (float)(double)a.n;
        *tot_sh = fmaxf(tot, 1.f);
    }
    __syncthreads();
    const float nvalid = (float)*nvalid_sh, tot = *tot_sh;
    for (int b = threadIdx.x; b <= bins; b += kThreads) {
        float wb;
        if (b == bins) {
            wb = 0.f / nvalid;                                         // nothing in any bin: NaN, as the torch chain gives
        } else {
            const float num = (float)cnt[b];
            float denom = num;
            if (a.momentum > 0.f) {
                denom = a.acc[b];
                if (cnt[b] > 0) {
                    denom = __fadd_rn(__fmul_rn(a.momentum, denom), __fmul_rn(a.one_minus, num));
                    a.acc[b] = denom;
                }
            }
            wb = __fdiv_rn(__fdiv_rn(tot, denom), nvalid);
        }
        w[b] = wb;
        wdz[b] = wb / tot;
    }
    __syncthreads();
}

__device__ __forceinline__ double ghmc_elem_block(const GhmcArgs& a, const float* edge, const float* w, const float* wdz,
                                                  int64_t lo, int m) {
    double s = 0;
    for (int i = threadIdx.x; i < m; i += kThreads) {
        const int64_t e = lo + i;
        const float z = a.z[e], t = a.t[e];
        float d;
        const int b = ghmc_bin(z, t, a.mask, e, edge, a.bins, &d);
        const float f = fmaxf(z, 0.f) - z * t + log1pf(expf(-fabsf(z)));
        s += (double)f * (double)w[b];
        if (a.dz) a.dz[e] = wdz[b] * d;
    }
    return wave_sum_f64(s);
}

__global__ __launch_bounds__(kThreads) void k_ghmc_count(GhmcArgs a) {
    __shared__ float edge[kMaxBins + 1];
    __shared__ unsigned hist[kMaxBins + 1];
    ghmc_edges(edge, a.bins);
    for (int b = threadIdx.x; b <= a.bins; b += kThreads) hist[b] = 0u;
    __syncthreads();
    const int64_t lo = (int64_t)blockIdx.x * kElemChunk;
    const int64_t rest = a.n - lo;
    ghmc_count_block(a, edge, hist, lo, rest < kElemChunk ? (int)rest : kElemChunk);
    __syncthreads();
    unsigned* out = a.counts + (int64_t)blockIdx.x * (a.bins + 1);
    for (int b = threadIdx.x; b <= a.bins; b += kThreads) out[b] = hist[b];
}

__global__ __launch_bounds__(kThreads) void k_ghmc_bins(GhmcArgs a) {
    __shared__ unsigned long long cnt[kMaxBins + 1];
    __shared__ float w[kMaxBins + 1], wdz[kMaxBins + 1];
    __shared__ int nvalid;
    __shared__ float tot;
    const int stride = a.bins + 1;
    for (int b = threadIdx.x; b <= a.bins; b += kThreads) {
        unsigned long long c = 0;
        for (int64_t k = 0; k < a.blocks; ++k) c += a.counts[k * stride + b];
        cnt[b] = c;
    }
    __syncthreads();
    ghmc_weights(a, cnt, &nvalid, w, wdz, &tot);
    for (int b = threadIdx.x; b <= a.bins; b += kThreads) {
        a.tab->w[b] = w[b];
        a.tab->wdz[b] = wdz[b];
    }
    if (threadIdx.x == 0) a.tab->tot = tot;
}

__global__ __launch_bounds__(kThreads) void k_ghmc_elem(GhmcArgs a) {
    __shared__ float edge[kMaxBins + 1], w[kMaxBins + 1], wdz[kMaxBins + 1];
    __shared__ double sh[kWaves];
    ghmc_edges(edge, a.bins);
    for (int b = threadIdx.x; b <= a.bins; b += kThreads) {
        w[b] = a.tab->w[b];
        wdz[b] = a.tab->wdz[b];
    }
    __syncthreads();
    const int64_t lo = (int64_t)blockIdx.x * kElemChunk;
    const int64_t rest = a.n - lo;
    const double s = ghmc_elem_block(a, edge, w, wdz, lo, rest < kElemChunk ? (int)rest : kElemChunk);
    const double all = waves_in_order(s, sh);
    if (threadIdx.x == 0) a.partial[blockIdx.x] = all;
}

__global__ __launch_bounds__(kThreads) void k_ghmc_total(const double* __restrict__ partial, int64_t count,
                                                         const GhmcTables* __restrict__ tab, float* __restrict__ loss) {
    __shared__ double sh[kWaves];
    double s = 0;
    for (int64_t i = threadIdx.x; i < count; i += kThreads) s += partial[i];
    s = wave_sum_f64(s);
    const double all = waves_in_order(s, sh);
    if (threadIdx.x == 0) loss[0] = (float)(all / (double)tab->tot);
}

// n <= kElemChunk: the four passes in one block
__global__ __launch_bounds__(kThreads) void k_ghmc_one(GhmcArgs a) {
    __shared__ float edge[kMaxBins + 1], w[kMaxBins + 1], wdz[kMaxBins + 1];
    __shared__ unsigned hist[kMaxBins + 1];
    __shared__ unsigned long long cnt[kMaxBins + 1];
    __shared__ double sh[kWaves];
    __shared__ int nvalid;
    __shared__ float tot;
    ghmc_edges(edge, a.bins);
    for (int b = threadIdx.x; b <= a.bins; b += kThreads) hist[b] = 0u;
    __syncthreads();
    ghmc_count_block(a, edge, hist, 0, (int)a.n);
    __syncthreads();
    for (int b = threadIdx.x; b <= a.bins; b += kThreads) cnt[b] = hist[b];
    __syncthreads();
    ghmc_weights(a, cnt, &nvalid, w, wdz, &tot);
    const double s = ghmc_elem_block(a, edge, w, wdz, 0, (int)a.n);
    const double all = waves_in_order(s, sh);
    if (threadIdx.x == 0) a.loss[0] = (float)(all / (double)tot);
}

inline bool ghmc_shape_ok(int64_t n, int bins) { return n >= 1 && n < kMaxElems && bins >= 1 && bins <= kMaxBins; }
inline int64_t ghmc_counts_bytes(int64_t blocks, int bins) {
    return ((blocks * (bins + 1) * (int64_t)sizeof(unsigned) + 7) / 8) * 8;
}

}  // namespace
}  // namespace dt

using namespace dt;

extern "C" int64_t dt_loss_reg_workspace_bytes(int64_t rows, int classes) {
    if (!shape_ok(rows, classes)) {
        set_error("dt_loss_reg_workspace_bytes: rows %lld, classes %d outside 1 <= rows < 2^31, 1 <= classes <= %d",
                  (long long)rows, classes, DT_LOSS_MAX_CLASSES);
        return DT_ERR_INVALID_ARG;
    }
    return elem_blocks(rows * classes) * (int64_t)sizeof(double);
}

extern "C" int dt_loss_reg(int kind, const float* p, const float* t, const float* w, int64_t rows, int classes, float delta,
                           float* loss, float* dz, void* workspace, void* stream) {
    DT_REQUIRE(kind >= DT_LOSS_HUBER && kind <= DT_LOSS_POISSON, "dt_loss_reg: unknown kind %d", kind);
    DT_REQUIRE(shape_ok(rows, classes), "dt_loss_reg: rows %lld, classes %d outside 1 <= rows < 2^31, 1 <= classes <= %d",
               (long long)rows, classes, DT_LOSS_MAX_CLASSES);
    DT_REQUIRE(p && t && loss, "dt_loss_reg: null predictions, targets or loss");
    DT_REQUIRE(workspace && (reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "dt_loss_reg: null or misaligned workspace");
    DT_REQUIRE(((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(t) | reinterpret_cast<uintptr_t>(w) |
                 reinterpret_cast<uintptr_t>(loss) | reinterpret_cast<uintptr_t>(dz)) & 3) == 0,
               "dt_loss_reg: misaligned pointer");
    DT_REQUIRE(kind != DT_LOSS_HUBER || (delta > 0.f && delta <= 3.0e38f), "dt_loss_reg: delta %g is not finite and > 0",
               (double)delta);
    RegArgs a;
    a.p = p; a.t = t; a.w = w; a.dz = dz; a.loss = loss;
    a.partial = reinterpret_cast<double*>(workspace);
    a.n = rows * classes; a.classes = classes; a.delta = delta;
    a.inv = 1.0 / ((double)rows * (double)classes);
    a.scale = (float)a.inv;
    const int64_t blocks = elem_blocks(a.n);
    a.final = blocks == 1;
    hipStream_t st = as_stream(stream);
    const dim3 grid((unsigned)blocks), block(kThreads);
    switch (kind) {
        case DT_LOSS_HUBER: hipLaunchKernelGGL(k_loss_reg<DT_LOSS_HUBER>, grid, block, 0, st, a); break;
        case DT_LOSS_LOG_COSH: hipLaunchKernelGGL(k_loss_reg<DT_LOSS_LOG_COSH>, grid, block, 0, st, a); break;
        case DT_LOSS_MSLE: hipLaunchKernelGGL(k_loss_reg<DT_LOSS_MSLE>, grid, block, 0, st, a); break;
        case DT_LOSS_MAPE: hipLaunchKernelGGL(k_loss_reg<DT_LOSS_MAPE>, grid, block, 0, st, a); break;
        default: hipLaunchKernelGGL(k_loss_reg<DT_LOSS_POISSON>, grid, block, 0, st, a); break;
    }
    if (blocks > 1)
        hipLaunchKernelGGL(k_loss_total, dim3(1), dim3(kThreads), 0, st, (const double*)a.partial, blocks, a.inv, loss);
    return launch_status("dt_loss_reg");
}

extern "C" int64_t dt_ghmc_workspace_bytes(int64_t n, int bins) {
    if (!ghmc_shape_ok(n, bins)) {
        set_error("dt_ghmc_workspace_bytes: n %lld, bins %d outside 1 <= n < 2^40, 1 <= bins <= %d", (long long)n, bins,
                  kMaxBins);
        return DT_ERR_INVALID_ARG;
    }
    const int64_t blocks = elem_blocks(n);
    return blocks * (int64_t)sizeof(double) + ghmc_counts_bytes(blocks, bins) + (int64_t)sizeof(GhmcTables);
}

extern "C" int dt_ghmc(const float* z, const float* t, const float* mask, int64_t n, int bins, float momentum,
                       float one_minus_momentum, float* acc_sum, float* loss, float* dz, void* workspace, void* stream) {
    DT_REQUIRE(ghmc_shape_ok(n, bins), "dt_ghmc: n %lld, bins %d outside 1 <= n < 2^40, 1 <= bins <= %d", (long long)n, bins,
               kMaxBins);
    DT_REQUIRE(z && t && loss, "dt_ghmc: null logits, targets or loss");
    DT_REQUIRE(workspace && (reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "dt_ghmc: null or misaligned workspace");
    DT_REQUIRE(((reinterpret_cast<uintptr_t>(z) | reinterpret_cast<uintptr_t>(t) | reinterpret_cast<uintptr_t>(mask) |
                 reinterpret_cast<uintptr_t>(acc_sum) | reinterpret_cast<uintptr_t>(loss) | reinterpret_cast<uintptr_t>(dz)) &
                3) == 0, "dt_ghmc: misaligned pointer");
    DT_REQUIRE(momentum >= 0.f && momentum < 1.f, "dt_ghmc: momentum %g outside [0, 1)", (double)momentum);
    DT_REQUIRE(momentum == 0.f || (one_minus_momentum > 0.f && one_minus_momentum <= 1.f),
               "dt_ghmc: 1 - momentum %g outside (0, 1]", (double)one_minus_momentum);
    DT_REQUIRE(momentum == 0.f || acc_sum, "dt_ghmc: momentum > 0 needs acc_sum");
    GhmcArgs a;
    a.z = z; a.t = t; a.mask = mask; a.acc = acc_sum; a.loss = loss; a.dz = dz;
    a.n = n; a.bins = bins; a.momentum = momentum; a.one_minus = one_minus_momentum;
    a.blocks = elem_blocks(n);
    char* ws = reinterpret_cast<char*>(workspace);
    a.partial = reinterpret_cast<double*>(ws);
    a.counts = reinterpret_cast<unsigned*>(ws + a.blocks * (int64_t)sizeof(double));
    a.tab = reinterpret_cast<GhmcTables*>(ws + a.blocks * (int64_t)sizeof(double) + ghmc_counts_bytes(a.blocks, bins));
    hipStream_t st = as_stream(stream);
    if (a.blocks == 1) {
        hipLaunchKernelGGL(k_ghmc_one, dim3(1), dim3(kThreads), 0, st, a);
        return launch_status("dt_ghmc");
    }
    const dim3 grid((unsigned)a.blocks), block(kThreads);
    hipLaunchKernelGGL(k_ghmc_count, grid, block, 0, st, a);
    hipLaunchKernelGGL(k_ghmc_bins, dim3(1), block, 0, st, a);
    hipLaunchKernelGGL(k_ghmc_elem, grid, block, 0, st, a);
    hipLaunchKernelGGL(k_ghmc_total, dim3(1), block, 0, st, (const double*)a.partial, a.blocks, (const GhmcTables*)a.tab, loss);
    return launch_status("dt_ghmc");
}
