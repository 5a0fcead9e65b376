// loss_reg.hip — the regression losses of Keras (Huber, log-cosh, MSLE, MAPE, Poisson) and the GHM-C loss of the layers
// module on the device (gfx950, wave64): value and gradient in a few launches (include/dt_hip.h: dt_loss_reg, dt_ghmc).
//
// dt_loss_reg is k_loss_elem of loss_sum.h, dt_loss' element-wise kernel, over the five terms of this file: per-element math is
// float32, every sum is float64 in a fixed order, one double per block goes into the workspace and k_loss_total adds them; one
// block that covers the problem writes the loss itself.  No float atomics, nothing zeroed beforehand, the same bits with and
// without dz.
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
//   pass 3  k_ghmc_elem    the bin again by the same instructions, f = BCE from the logit (BceTerm of loss_sum.h, as is
//                          sigmoid(z) - t of both passes), the float64 partial of f w, dz
//   pass 4  k_ghmc_total   the partials in order, divided by tot
// and a problem that one block covers is one launch (k_ghmc_one: the same steps behind block barriers).  The only atomics are
// integer LDS atomics, whose result does not depend on their order.
#include "loss_sum.h"

namespace dt {
namespace {

constexpr float kLn2 = 0.6931471805599453f;
constexpr float kLogCoshSwitch = 10.f;

// the five element-wise kinds: (f, g) of a prediction p and its target t
template <int KIND>
struct RegTerm : NoTail {
    float delta;             // Huber
    __device__ __forceinline__ void operator()(float p, float t, float* f, float* g) const {
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
};

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

// the bin of element e, or `bins` when it lies in none (g > 1 + 1e-6: an ignored target; a NaN) or is masked out; leaves the
// element's BCE term in *f and sigmoid(z) - t in *diff
__device__ __forceinline__ int ghmc_bin(const GhmcArgs& a, int64_t e, const float* edge, float* f, float* diff) {
    BceTerm{}(a.z[e], a.t[e], f, diff);
    const float* mask = a.mask;
    const int bins = a.bins;
    const float g = fabsf(*diff);
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
        float f, d;
        const int b = ghmc_bin(a, e, edge, &f, &d);
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
        float f, d;
        const int b = ghmc_bin(a, e, edge, &f, &d);
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
    if (int rc = check_buffers("dt_loss_reg", "predictions", p, t, loss, workspace, addr(w) | addr(dz))) return rc;
    DT_REQUIRE(kind != DT_LOSS_HUBER || (delta > 0.f && delta <= 3.0e38f), "dt_loss_reg: delta %g is not finite and > 0",
               (double)delta);
    const ElemArgs a = elem_args(p, t, w, rows, classes, loss, dz, workspace);
    hipStream_t st = as_stream(stream);
    switch (kind) {
        case DT_LOSS_HUBER: launch_elem(a, RegTerm<DT_LOSS_HUBER>{{}, delta}, st); break;
        case DT_LOSS_LOG_COSH: launch_elem(a, RegTerm<DT_LOSS_LOG_COSH>{{}, delta}, st); break;
        case DT_LOSS_MSLE: launch_elem(a, RegTerm<DT_LOSS_MSLE>{{}, delta}, st); break;
        case DT_LOSS_MAPE: launch_elem(a, RegTerm<DT_LOSS_MAPE>{{}, delta}, st); break;
        default: launch_elem(a, RegTerm<DT_LOSS_POISSON>{{}, delta}, st); break;
    }
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
    if (int rc = check_buffers("dt_ghmc", "logits", z, t, loss, workspace, addr(mask) | addr(acc_sum) | addr(dz))) return rc;
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
