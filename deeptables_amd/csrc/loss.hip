// loss.hip — the losses of a train step on the device (gfx950, wave64): value and gradient with respect to the logits in at
// most two launches, with Keras' SUM_OVER_BATCH_SIZE reduction and per-row weights (include/dt_hip.h: dt_loss).
//
// Two geometries, both of 256 threads, neither assumes that `classes` is small:
//   element-wise kinds (BCE, MSE, MAE, BINARY_FOCAL): k_loss_elem of loss_sum.h over a term of this file (BCE's is there, GHM-C
//     shares it): a block takes kElemChunk consecutive elements of the flat [rows * classes] array.
//   categorical kinds (CCE, CATEGORICAL_FOCAL): one wave per row, the lanes stride the classes.  classes <= 64 keeps the lane's
//     logit and target in registers (one read); above, the passes (row maximum, sum of exponentials, loss and sum g p, dz)
//     re-read the row, which the first pass left in the cache.  A block takes kRowsPerBlock rows, one per wave — or, when one
//     block covers the problem, all of them, wave w the rows w, w + 4, ...
// Per-element and per-row math is float32.  Every sum is float64 in the fixed order of loss_sum.h, one double per block into the
// caller's workspace, k_loss_total behind it; a problem that one block covers is finished by that block: one launch.  No float
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

constexpr float kOneMinusEps = 0.9999999f;               // fl(1 - 1e-7)
constexpr float kLogEps = -16.11809565095832f;           // ln(1e-7)
constexpr float kLogOneMinusEps = -1.0000000500000003e-7f;   // ln(1 - 1e-7)
constexpr float kZClamp = 16.118095550958320f;           // ln((1 - eps) / eps): sigmoid(z) leaves [eps, 1 - eps] beyond it

struct RowArgs : ElemArgs {   // the categorical kinds: scale and inv are 1 / rows
    int64_t rows;
    int rows_per_block;
    int kind;
    float gamma, alpha;
};

template <int KIND>            // DT_LOSS_MSE, DT_LOSS_MAE
struct DiffTerm : NoTail {
    __device__ __forceinline__ void operator()(float z, float t, float* f, float* g) const {
        const float d = z - t;
        *f = KIND == DT_LOSS_MSE ? d * d : fabsf(d);
        *g = KIND == DT_LOSS_MSE ? 2.f * d : (d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f));
    }
};

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

struct BinaryFocalTerm {
    float gamma, alpha;
    double c1, c0;                    // the constant an element with t != 1 / t != 0 adds (sign of the loss included)
    int n_not1, n_not0;               // the thread's counts of such elements: 0 at the launch

    __device__ __forceinline__ void operator()(float z, float t, float* f, float* g) {
        *f = 0.f;
        *g = 0.f;
        if (t == 1.f) {
            binary_focal_side(z, alpha, gamma, f, g);
        } else if (t == 0.f) {
            binary_focal_side(-z, 1.f - alpha, gamma, f, g);
            *g = -*g;                                                   // d/dz of a function of -z
        }
        n_not1 += t != 1.f;
        n_not0 += t != 0.f;
    }
    __device__ __forceinline__ void tail(double* s) const { *s += (double)n_not1 * c1 + (double)n_not0 * c0; }
};

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
__device__ __forceinline__ double cat_row(const RowArgs& a, const float* __restrict__ zr, const float* __restrict__ tr,
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
__global__ __launch_bounds__(kThreads) void k_loss_rows(RowArgs a) {
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
    const int64_t e = elem_blocks(rows * classes), r = row_blocks(rows, classes);      // whichever kind is asked for
    return (e > r ? e : r) * (int64_t)sizeof(double);
}

extern "C" int dt_loss(int kind, const float* z, const float* t, const float* w, int64_t rows, int classes, float gamma,
                       float alpha, float* loss, float* dz, void* workspace, void* stream) {
    DT_REQUIRE(kind >= DT_LOSS_BCE && kind <= DT_LOSS_CATEGORICAL_FOCAL, "dt_loss: unknown kind %d", kind);
    DT_REQUIRE(shape_ok(rows, classes), "dt_loss: rows %lld, classes %d outside 1 <= rows < 2^31, 1 <= classes <= %d",
               (long long)rows, classes, DT_LOSS_MAX_CLASSES);
    DT_REQUIRE(!is_categorical(kind) || classes >= 2, "dt_loss: a categorical loss needs classes >= 2, got %d", classes);
    if (int rc = check_buffers("dt_loss", "logits", z, t, loss, workspace, addr(w) | addr(dz))) return rc;
    DT_REQUIRE(kind != DT_LOSS_BINARY_FOCAL || !w,
               "dt_loss: the binary focal loss is a mean over all elements, a per-row weight has no place in it");
    const bool focal = kind == DT_LOSS_BINARY_FOCAL || kind == DT_LOSS_CATEGORICAL_FOCAL;
    DT_REQUIRE(!focal || (gamma >= 0.f && gamma <= 1e6f && alpha == alpha), "dt_loss: gamma %g outside [0, 1e6] or alpha NaN",
               (double)gamma);
    const ElemArgs e = elem_args(z, t, w, rows, classes, loss, dz, workspace);
    hipStream_t st = as_stream(stream);
    switch (kind) {
        case DT_LOSS_BCE: launch_elem(e, BceTerm{}, st); break;
        case DT_LOSS_MSE: launch_elem(e, DiffTerm<DT_LOSS_MSE>{}, st); break;
        case DT_LOSS_MAE: launch_elem(e, DiffTerm<DT_LOSS_MAE>{}, st); break;
        case DT_LOSS_BINARY_FOCAL: {
            const double k = pow(1e-7, (double)gamma) * log1p(-1e-7);      // eps^gamma log(1 - eps) < 0; the loss carries -1
            launch_elem(e, BinaryFocalTerm{gamma, alpha, -(double)alpha * k, -(1.0 - (double)alpha) * k, 0, 0}, st);
            break;
        }
        default: {                                                          // the categorical kinds
            const int64_t blocks = row_blocks(rows, classes);
            RowArgs a{e, rows, blocks == 1 ? (int)rows : kRowsPerBlock, kind, gamma, alpha};      // (one block: rows <= kOneRows)
            a.inv = 1.0 / (double)rows;
            a.scale = (float)a.inv;
            a.final = blocks == 1;
            if (classes <= kWave) hipLaunchKernelGGL(k_loss_rows<true>, dim3((unsigned)blocks), dim3(kThreads), 0, st, a);
            else hipLaunchKernelGGL(k_loss_rows<false>, dim3((unsigned)blocks), dim3(kThreads), 0, st, a);
            launch_total(a, blocks, st);
        }
    }
    return launch_status("dt_loss");
}
