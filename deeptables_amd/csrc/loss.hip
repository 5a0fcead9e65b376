// loss.hip — the losses of a train step on the device (gfx950, wave64): value and gradient with respect to the logits in at
// most two launches, with Keras' SUM_OVER_BATCH_SIZE reduction and per-row weights (include/dt_hip.h: dt_loss).
//
// Two geometries, both of 256 threads, neither assumes that `classes` is small:
//   element-wise kinds (BCE, MSE, MAE, BINARY_FOCAL): a block takes kElemChunk consecutive elements of the flat [rows * classes]
//     array, thread t the elements t, t + 256, ... of the chunk (coalesced); the row of an element (for its weight) is e / classes.
//   categorical kinds (CCE, CATEGORICAL_FOCAL): one wave per row, the lanes stride the classes.  classes <= 64 keeps the lane's
//     logit and target in registers (one read); above, the passes (row maximum, sum of exponentials, loss and sum g p, dz)
//     re-read the row, which the first pass left in the cache.  A block takes kRowsPerBlock rows, one per wave — or, when one
//     block covers the problem, all of them, wave w the rows w, w + 4, ...
// Per-element and per-row math is float32.  Every sum is float64 in a fixed order: a thread / lane adds its elements in index
// order, the lanes of a wave combine by halving, the waves of a block in order, and ONE double per block goes into the caller's
// workspace at the block's index; k_loss_total adds the partials (thread t takes t, t + 256, ... in index order, then the same
// tree), scales and writes the float32 loss.  A problem that one block covers is finished by that block: one launch.  No float
// atomics, no block waits for another, nothing is zeroed beforehand: the same input gives the same bits, and the loss is
// computed by the same instructions whether dz is written or not.
//
// Stable forms: BCE max(z,0) - z t + log1p(exp(-|z|)); softmax through the row maximum with log p = (z - m) - log sum exp(z - m)
// (never log(softmax)); 1 - p of a softmax entry as -expm1(log p); 1 - sigmoid(z) as sigmoid(-z); log sigmoid(z) as -softplus(-z).
#include "loss_sum.h"

namespace dt {
namespace {

constexpr int kRowsPerBlock = kWaves;         // rows per block of the categorical kinds
constexpr int kOneRows = 64;                  // categorical kinds: one block takes the whole problem up to this many rows ...
constexpr int kOneElems = 16384;              // ... and this many elements
constexpr int64_t kMaxRows = (int64_t)1 << 31;
constexpr int64_t kMaxElems = (int64_t)1 << 40;   // rows * classes: the block count of a launch stays below 2^31

constexpr float kEps = 1e-7f;                            // keras.backend.epsilon()
constexpr float kOneMinusEps = 0.9999999f;               // fl(1 - 1e-7)
constexpr float kLogEps = -16.11809565095832f;           // ln(1e-7)
constexpr float kLogOneMinusEps = -1.0000000500000003e-7f;   // ln(1 - 1e-7)
constexpr float kZClamp = 16.118095550958320f;           // ln((1 - eps) / eps): sigmoid(z) leaves [eps, 1 - eps] beyond it

struct LossArgs {
    const float* z;
    const float* t;
    const float* w;          // [rows] or null
    float* dz;               // [rows * classes] or null
    float* loss;             // [1]
    double* partial;         // one double per block
    int64_t rows;
    int64_t n;               // rows * classes
    int classes;
    int kind;
    int rows_per_block;      // categorical kinds
    int final;               // the launch has one block, which writes the loss itself
    float gamma, alpha;
    float scale;             // fl(1 / rows) (categorical kinds) or fl(1 / (rows classes)): dz = w_b * scale * dl/dz
    double inv;              // the same in double: loss = inv * sum
    double c1, c0;           // BINARY_FOCAL: the constant an element with t != 1 / t != 0 adds (sign of the loss included)
};

__device__ __forceinline__ void finish_block(const LossArgs& a, double block_sum) {
    if (threadIdx.x == 0) {
        if (a.final) a.loss[0] = (float)(block_sum * a.inv);
        else a.partial[blockIdx.x] = block_sum;
    }
}

__device__ __forceinline__ float softplus_f(float z) { return fmaxf(z, 0.f) + log1pf(expf(-fabsf(z))); }

// one side of the binary focal loss for an element whose target selects it.  (p, q) = (sigmoid(z), sigmoid(-z)) for t == 1 and
// swapped for t == 0; zs = z for t == 1 and -z for t == 0, so that p = sigmoid(zs); coef = alpha or 1 - alpha.
//   f = -coef qh^gamma log ph          (the element's term of the loss, its sign included)
//   g = -p q coef (-gamma qh^(gamma-1) log ph + qh^gamma / ph), the derivative with respect to zs; 0 where the clamp is active
__device__ __forceinline__ void binary_focal_side(float zs, float coef, float gamma, float* f, float* g) {
    if (fabsf(zs) > kZClamp) {
        const float ph_log = zs < 0.f ? kLogEps : kLogOneMinusEps;
        const float qh = zs < 0.f ? kOneMinusEps : kEps;
        *f = -coef * powf(qh, gamma) * ph_log;
        *g = 0.f;
        return;
    }
    const float p = sigmoid_f(zs), q = sigmoid_f(-zs);
    const float logp = -softplus_f(-zs);
    const float qg = powf(q, gamma);
    *f = -coef * qg * logp;
    const float a = gamma != 0.f ? -gamma * powf(q, gamma - 1.f) * logp : 0.f;
    *g = -(p * q) * coef * (a + qg / p);
}

__global__ __launch_bounds__(kThreads) void k_loss_elem(LossArgs a) {
    __shared__ double sh[kWaves];
    const int64_t lo = (int64_t)blockIdx.x * kElemChunk;
    const int64_t rest = a.n - lo;
    const int m = rest < kElemChunk ? (int)rest : kElemChunk;          // >= 1: the host counts ceil(n / kElemChunk) blocks
    const int C = a.classes;
    const float invC_scale = a.scale;
    double s = 0;
    int n_not1 = 0, n_not0 = 0;
    for (int i = threadIdx.x; i < m; i += kThreads) {
        const int64_t e = lo + i;                                       // < n
        const float z = a.z[e], t = a.t[e];
        const float wb = a.w ? a.w[e / C] : 1.f;                        // e / C < rows
        float f, g;
        switch (a.kind) {
            case DT_LOSS_BCE:
                f = fmaxf(z, 0.f) - z * t + log1pf(expf(-fabsf(z)));
                g = sigmoid_f(z) - t;
                break;
            case DT_LOSS_MSE: {
                const float d = z - t;
                f = d * d;
                g = 2.f * d;
                break;
            }
            case DT_LOSS_MAE: {
                const float d = z - t;
                f = fabsf(d);
                g = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
                break;
            }
            default: {                                                  // DT_LOSS_BINARY_FOCAL
                f = 0.f;
                g = 0.f;
                if (t == 1.f) {
                    binary_focal_side(z, a.alpha, a.gamma, &f, &g);
                } else if (t == 0.f) {
                    binary_focal_side(-z, 1.f - a.alpha, a.gamma, &f, &g);
                    g = -g;                                             // d/dz of a function of -z
                }
                n_not1 += t != 1.f;
                n_not0 += t != 0.f;
                break;
            }
        }
        s += (double)wb * (double)f;
        if (a.dz) a.dz[e] = (wb * invC_scale) * g;
    }
    if (a.kind == DT_LOSS_BINARY_FOCAL) s += (double)n_not1 * a.c1 + (double)n_not0 * a.c0;
    s = wave_sum_f64(s);
    finish_block(a, waves_in_order(s, sh));
}

// focal term of one class from log p (unclamped) and its target: f = alpha (1 - ph)^gamma (-t log ph),
// g = alpha t [gamma (1 - ph)^(gamma-1) log ph - (1 - ph)^gamma / ph], 0 where the clamp is active
__device__ __forceinline__ void cat_focal_class(float lp, float t, float gamma, float alpha, float* f, float* g) {
    *f = 0.f;
    *g = 0.f;
    if (t == 0.f) return;                       // both carry the factor t
    if (lp < kLogEps) {
        *f = alpha * powf(kOneMinusEps, gamma) * (-t * kLogEps);
    } else if (lp > kLogOneMinusEps) {
        *f = alpha * powf(kEps, gamma) * (-t * kLogOneMinusEps);
    } else {
        const float x = -expm1f(lp);            // 1 - p, in [eps, 1 - eps]
        const float p = expf(lp);
        const float xg = powf(x, gamma);
        *f = alpha * xg * (-t * lp);
        const float a = gamma != 0.f ? gamma * powf(x, gamma - 1.f) * lp : 0.f;
        *g = alpha * t * (a - xg / p);
    }
}

// one row of a categorical kind by one wave; returns the row's loss l_b (every lane), writes dz of the row when asked.
// REG: classes <= 64, the lane's class lives in registers.
template <bool REG>
__device__ __forceinline__ double cat_row(const LossArgs& a, const float* __restrict__ zr, const float* __restrict__ tr,
                                          float* __restrict__ dzr, float row_scale, int lane) {
    const int C = a.classes;
    float z0 = 0.f, t0 = 0.f;
    if (REG && lane < C) {
        z0 = zr[lane];
        t0 = tr[lane];
    }
    auto Z = [&](int c) { return REG ? z0 : zr[c]; };
    auto T = [&](int c) { return REG ? t0 : tr[c]; };
    float m = -INFINITY;
    for (int c = lane; c < C; c += kWave) m = fmaxf(m, Z(c));
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, kWave));
    double se = 0, ts = 0;
    for (int c = lane; c < C; c += kWave) {
        se += (double)expf(Z(c) - m);
        ts += (double)T(c);
    }
    se = wave_sum_f64(se);
    const float log_se = logf((float)se);
    double l = 0;
    if (a.kind == DT_LOSS_CCE) {
        const float tsum = (float)wave_sum_f64(ts);
        for (int c = lane; c < C; c += kWave) {
            const float lp = (Z(c) - m) - log_se;
            const float t = T(c);
            l += (double)(-t * lp);
            if (dzr) dzr[c] = row_scale * (tsum * expf(lp) - t);
        }
        return wave_sum_f64(l);
    }
    double gp = 0;                              // DT_LOSS_CATEGORICAL_FOCAL
    for (int c = lane; c < C; c += kWave) {
        const float lp = (Z(c) - m) - log_se;
        float f, g;
        cat_focal_class(lp, T(c), a.gamma, a.alpha, &f, &g);
        l += (double)f;
        if (g != 0.f) gp += (double)(g * expf(lp));
    }
    l = wave_sum_f64(l);
    if (dzr) {
        const float gps = (float)wave_sum_f64(gp);
        for (int c = lane; c < C; c += kWave) {
            const float lp = (Z(c) - m) - log_se;
            float f, g;
            cat_focal_class(lp, T(c), a.gamma, a.alpha, &f, &g);
            dzr[c] = row_scale * (expf(lp) * (g - gps));
        }
    }
    return l;
}

template <bool REG>
__global__ __launch_bounds__(kThreads) void k_loss_rows(LossArgs a) {
    __shared__ double sh[kWaves];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const int64_t row0 = (int64_t)blockIdx.x * a.rows_per_block;
    const int64_t rest = a.rows - row0;
    const int64_t row_end = row0 + (rest < a.rows_per_block ? rest : (int64_t)a.rows_per_block);       // <= rows
    double acc = 0;
    for (int64_t r = row0 + wave; r < row_end; r += kWaves) {            // wave-uniform
        const float wb = a.w ? a.w[r] : 1.f;
        const int64_t off = r * a.classes;
        acc += (double)wb * cat_row<REG>(a, a.z + off, a.t + off, a.dz ? a.dz + off : nullptr, wb * a.scale, lane);
    }
    finish_block(a, waves_in_order(acc, sh));
}

inline bool is_categorical(int kind) { return kind == DT_LOSS_CCE || kind == DT_LOSS_CATEGORICAL_FOCAL; }
inline bool shape_ok(int64_t rows, int classes) {
    // (rows * classes < 2^43: no overflow, and at most 2^32 / 2 blocks only below 2^42 elements — held to 2^40)
    return rows >= 1 && rows < kMaxRows && classes >= 1 && classes <= DT_LOSS_MAX_CLASSES && rows * classes < kMaxElems;
}
inline int64_t elem_blocks(int64_t rows, int classes) { return (rows * classes + kElemChunk - 1) / kElemChunk; }
inline int64_t row_blocks(int64_t rows, int classes) {
    if (rows <= kOneRows && rows * classes <= kOneElems) return 1;
    return (rows + kRowsPerBlock - 1) / kRowsPerBlock;
}

}  // namespace
}  // namespace dt

using namespace dt;

extern "C" int64_t dt_loss_workspace_bytes(int64_t rows, int classes) {
    if (!shape_ok(rows, classes)) {
        set_error("dt_loss_workspace_bytes: rows %lld, classes %d outside 1 <= rows < 2^31, 1 <= classes <= %d", (long long)rows,
                  classes, DT_LOSS_MAX_CLASSES);
        return DT_ERR_INVALID_ARG;
    }
    const int64_t e = elem_blocks(rows, classes), r = row_blocks(rows, classes);      // whichever kind is asked for
    return (e > r ? e : r) * (int64_t)sizeof(double);
}

extern "C" int dt_loss(int kind, const float* z, const float* t, const float* w, int64_t rows, int classes, float gamma,
                       float alpha, float* loss, float* dz, void* workspace, void* stream) {
    DT_REQUIRE(kind >= DT_LOSS_BCE && kind <= DT_LOSS_CATEGORICAL_FOCAL, "dt_loss: unknown kind %d", kind);
    DT_REQUIRE(shape_ok(rows, classes), "dt_loss: rows %lld, classes %d outside 1 <= rows < 2^31, 1 <= classes <= %d",
               (long long)rows, classes, DT_LOSS_MAX_CLASSES);
    DT_REQUIRE(!is_categorical(kind) || classes >= 2, "dt_loss: a categorical loss needs classes >= 2, got %d", classes);
    DT_REQUIRE(z && t && loss, "dt_loss: null logits, targets or loss");
    DT_REQUIRE(workspace && (reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "dt_loss: null or misaligned workspace");
    DT_REQUIRE(((reinterpret_cast<uintptr_t>(z) | reinterpret_cast<uintptr_t>(t) | reinterpret_cast<uintptr_t>(w) |
                 reinterpret_cast<uintptr_t>(loss) | reinterpret_cast<uintptr_t>(dz)) & 3) == 0, "dt_loss: misaligned pointer");
    DT_REQUIRE(kind != DT_LOSS_BINARY_FOCAL || !w,
               "dt_loss: the binary focal loss is a mean over all elements, a per-row weight has no place in it");
    const bool focal = kind == DT_LOSS_BINARY_FOCAL || kind == DT_LOSS_CATEGORICAL_FOCAL;
    DT_REQUIRE(!focal || (gamma >= 0.f && gamma <= 1e6f && alpha == alpha), "dt_loss: gamma %g outside [0, 1e6] or alpha NaN",
               (double)gamma);
    LossArgs a;
    a.z = z; a.t = t; a.w = w; a.dz = dz; a.loss = loss;
    a.partial = reinterpret_cast<double*>(workspace);
    a.rows = rows; a.classes = classes; a.n = rows * classes; a.kind = kind;
    a.gamma = gamma; a.alpha = alpha;
    a.rows_per_block = kRowsPerBlock;
    a.c1 = a.c0 = 0;
    const double per = is_categorical(kind) ? (double)rows : (double)rows * (double)classes;
    a.inv = 1.0 / per;
    a.scale = (float)a.inv;
    if (kind == DT_LOSS_BINARY_FOCAL) {
        const double k = pow(1e-7, (double)gamma) * log1p(-1e-7);          // eps^gamma log(1 - eps) < 0; the loss carries -1
        a.c1 = -(double)alpha * k;
        a.c0 = -(1.0 - (double)alpha) * k;
    }
    hipStream_t st = as_stream(stream);
    int64_t blocks;
    if (is_categorical(kind)) {
        blocks = row_blocks(rows, classes);
        if (blocks == 1) a.rows_per_block = (int)rows;                      // <= kOneRows
        a.final = blocks == 1;
        if (classes <= kWave) hipLaunchKernelGGL(k_loss_rows<true>, dim3((unsigned)blocks), dim3(kThreads), 0, st, a);
        else hipLaunchKernelGGL(k_loss_rows<false>, dim3((unsigned)blocks), dim3(kThreads), 0, st, a);
    } else {
        blocks = elem_blocks(rows, classes);
        a.final = blocks == 1;
        hipLaunchKernelGGL(k_loss_elem, dim3((unsigned)blocks), dim3(kThreads), 0, st, a);
    }
    if (blocks > 1)
        hipLaunchKernelGGL(k_loss_total, dim3(1), dim3(kThreads), 0, st, (const double*)a.partial, blocks, a.inv, loss);
    return launch_status("dt_loss");
}
