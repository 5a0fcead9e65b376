// cell.hip — the tail of a DNN tower cell, `Activation -> (Dropout)` (deepnets.py:401-427, :430-452), as ONE streaming launch
// forward and ONE backward over x [N, C] fp32 (gfx950, wave64):
//
//   out = keep(seed, salt, row, col) * act(x)                    dt_cell_fwd
//   dx  = g * keep(seed, salt, row, col) * act'(.)               dt_cell_bwd
//
// keep is 0 or 1 / (1 - rate), decided by a 32-bit counter hash of (seed word, per-layer salt, row, column): the backward
// recomputes it from the same seed word, so no mask tensor exists.  The seed word is read from DEVICE memory by the kernel:
// drawing it costs no host synchronisation and a captured graph draws a fresh one at every replay.  rate == 0 runs no hash;
// rate == 1 multiplies by 0 (no 1 / 0 scale), as torch's dropout does.
//
// act' is taken from ONE saved [N, C] tensor: the OUTPUT for the activations whose derivative follows from it (codes 0-8
// through act_grad_from_y of common.h, relu6, leaky_relu, hard_sigmoid), the INPUT for gelu, silu, mish and hard_silu.  With
// 0 < rate < 1 the caller hands over the input for every activation (`saved_is_input`): act(x) scaled by fl(1 / (1 - rate))
// no longer decides y < 6 or y < 1 exactly, and the input is the tensor the producing Dense keeps for its own backward anyway.
//
// Geometry: 256 threads, a unit of work is one 16-byte vector (4 floats) when n = N C >= 4 and every base address is 16-byte
// aligned, else one float; min(ceil(units / 256), kMaxBlocks) blocks walk the units with a grid stride; the n % 4 elements
// behind the last whole vector are taken by the first threads of block 0.  (row, col) of a thread's first element come from
// one 32-bit division (the first pass covers < 2^22 elements) and then advance by the stride's (rows, cols): no division in
// the loop, and no flat element index enters the hash — rows and columns are separate 32-bit words.
//
// Numerics: every activation and derivative is finite for finite |x| <= 80 and takes its limit beyond (sigmoid(-100),
// silu(-100), mish(-100), gelu(-100) -> signed zeros, gelu(-10) = -7.6e-23 keeps its digits; softplus(100) = 100;
// exponential(89) = inf is the function's value);
// NaN in gives NaN out, in both directions, whatever the keep decision (0 * NaN).  At a kink (0; 6; +-3) the derivative is the
// one torch's CPU autograd takes for the definition deeptables_amd.functional.get_activation registers.
#include <math.h>

#include "cell_hash.h"
#include "common.h"

namespace dt {
namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 2048;              // 256 CUs x 8 blocks: one grid pass covers kMaxBlocks * kThreads units
constexpr int64_t kMaxElems = (int64_t)1 << 40;

typedef float cell_f4 __attribute__((ext_vector_type(4)));

// (the dropout hash: cell_hash.h, shared with csrc/emb_dropout.hip)

// ---- activations -------------------------------------------------------------------------------------------------------
constexpr float kLeakySlope = 0.2f;                    // [ext] keras.activations.leaky_relu's default negative_slope
constexpr float kInvSqrt2 = 0.70710678118654752f;
constexpr float kInvSqrt2Pi = 0.39894228040143268f;
constexpr float kBelowOne = 0x1.fffffep-1f;            // the largest float below 1
constexpr float kMishLinear = 20.f;                    // tanh(softplus(x)) rounds to 1 from here on (1 - it < 2 e^-2x)

__device__ __forceinline__ bool is_input_kind(int act) {
    return act == DT_CELL_ACT_SILU || act == DT_CELL_ACT_GELU || act == DT_CELL_ACT_MISH || act == DT_CELL_ACT_HARD_SILU;
}

// sigmoid(x) and sigmoid(-x) without cancellation: sigmoid(-100) = +0, never NaN for a finite x
__device__ __forceinline__ void sigmoid_pair(float x, float* s, float* sm) {
    const float e = expf(-fabsf(x));
    const float a = 1.f / (1.f + e), b = e / (1.f + e);
    *s = x >= 0.f ? a : b;
    *sm = x >= 0.f ? b : a;
}
// Phi(x) = P(Z <= x) through erfc on the side where it is small: gelu(-10) keeps its digits, gelu(-100) = -0
__device__ __forceinline__ float normal_cdf(float x) {
    const float h = 0.5f * erfcf(fabsf(x) * kInvSqrt2);
    return x < 0.f ? h : 1.f - h;
}
// t = tanh(softplus(x)) = w / (w + 2), w = e^x (e^x + 2): no cancellation for x << 0 (t ~ e^x), 1 for x >= kMishLinear;
// u = 1 - t^2 = 4 (w + 1) / (w + 2)^2
__device__ __forceinline__ void mish_parts(float x, float* t, float* u) {
    if (x >= kMishLinear) { *t = 1.f; *u = 0.f; return; }
    const float n = expf(x);
    const float w = n * (n + 2.f), d = 1.f / (w + 2.f);
    *t = w * d;
    *u = 4.f * (w + 1.f) * d * d;
}
__device__ __forceinline__ float hard_sigmoid_f(float x) {        // [ext] relu6(x + 3) / 6
    float y = fminf(fmaxf(x + 3.f, 0.f), 6.f) / 6.f;
    // fl(x + 3) is 6 for the float just below 3: keep y < 1 <=> x < 3, which is what the backward reads off the output
    if (x < 3.f) y = fminf(y, kBelowOne);
    return y;
}

__device__ __forceinline__ float cell_act(float x, int act) {
    float y;
    switch (act) {
        case DT_CELL_ACT_RELU6: y = fminf(fmaxf(x, 0.f), 6.f); break;                          // [ext]
        case DT_CELL_ACT_LEAKY_RELU: y = x > 0.f ? x : kLeakySlope * x; break;                 // [ext]
        case DT_CELL_ACT_SILU: { float s, sm; sigmoid_pair(x, &s, &sm); y = x * s; break; }    // [ext] = swish
        case DT_CELL_ACT_GELU: y = x * normal_cdf(x); break;                                   // [ext] exact erf form
        case DT_CELL_ACT_MISH: { float t, u; mish_parts(x, &t, &u); y = x * t; break; }        // [ext] x tanh(softplus(x))
        case DT_CELL_ACT_HARD_SIGMOID: y = hard_sigmoid_f(x); break;
        case DT_CELL_ACT_HARD_SILU: y = x * (fminf(fmaxf(x + 3.f, 0.f), 6.f) / 6.f); break;    // [ext] = hard_swish
        default: y = act_apply(x, act); break;                                                 // codes 0-8 (common.h)
    }
    return x != x ? x : y;             // v_max / v_min drop a NaN operand: relu(NaN) must stay NaN
}

// d act / dx from the output y (output kinds)
__device__ __forceinline__ float cell_grad_from_y(float y, int act) {
    switch (act) {
        case DT_CELL_ACT_RELU6: return (y > 0.f && y < 6.f) ? 1.f : 0.f;
        case DT_CELL_ACT_LEAKY_RELU: return y > 0.f ? 1.f : kLeakySlope;
        case DT_CELL_ACT_HARD_SIGMOID: return (y > 0.f && y < 1.f) ? (1.f / 6.f) : 0.f;
        default: return act_grad_from_y(y, act);
    }
}
// d act / dx from the input x (input kinds)
__device__ __forceinline__ float cell_grad_from_x(float x, int act) {
    switch (act) {
        case DT_CELL_ACT_SILU: {                       // s (1 + x (1 - s)), 1 - s as sigmoid(-x)
            float s, sm;
            sigmoid_pair(x, &s, &sm);
            return s * (1.f + x * sm);
        }
        case DT_CELL_ACT_GELU: return normal_cdf(x) + x * (kInvSqrt2Pi * expf(-0.5f * x * x));
        case DT_CELL_ACT_MISH: {                       // t + x (1 - t^2) sigmoid(x)
            float t, u, s, sm;
            mish_parts(x, &t, &u);
            sigmoid_pair(x, &s, &sm);
            return t + x * u * s;
        }
        default:                                       // DT_CELL_ACT_HARD_SILU: 0 | x / 3 + 0.5 | 1, the middle piece on (-3, 3)
            return x <= -3.f ? 0.f : (x < 3.f ? x / 3.f + 0.5f : 1.f);
    }
}
__device__ __forceinline__ float cell_grad(float s, int act, bool saved_is_input) {
    float d;
    if (is_input_kind(act)) d = cell_grad_from_x(s, act);
    else d = cell_grad_from_y(saved_is_input ? cell_act(s, act) : s, act);
    return s != s ? s : d;
}

// ---- the kernels -------------------------------------------------------------------------------------------------------
struct CellArgs {
    const float* x;            // forward: the input; backward: the saved tensor
    const float* g;            // backward: the incoming gradient
    float* out;                // forward: out; backward: dx
    const unsigned* seed;      // device, read when hashed
    int64_t n;                 // N C
    unsigned C;
    int act;
    int saved_is_input;
    unsigned salt, thr;
    float scale;               // hashed: 1 / (1 - rate); else the factor of every element (1, or 0 at rate == 1)
    unsigned step_rows, step_cols;     // the grid stride in elements, as (rows, cols) of C
};

// position of the element a thread works on, advanced without a division
struct CellPos {
    unsigned row, col;
    __device__ __forceinline__ void next(unsigned C) {                 // one element on
        if (++col == C) { col = 0; ++row; }
    }
    __device__ __forceinline__ void jump(const CellArgs& a) {          // one grid stride on
        row += a.step_rows;
        col += a.step_cols;
        if (col >= a.C) { col -= a.C; ++row; }
    }
};

template <bool BWD>
__device__ __forceinline__ float cell_one(const CellArgs& a, float x, float g, float k) {
    if (!BWD) return cell_act(x, a.act) * k;
    return (g * k) * cell_grad(x, a.act, a.saved_is_input != 0);
}

// W = 4: 16-byte units (every pointer 16-byte aligned) and a scalar tail; W = 1: float units.  HASH: 0 < rate < 1.
template <int W, bool HASH, bool BWD>
__global__ __launch_bounds__(kThreads) void k_cell(CellArgs a) {
    const int64_t units = a.n / W;
    const int64_t tid = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * kThreads;
    unsigned head = 0;
    CellPos p = {0, 0};
    if (HASH) {
        head = cell_hash_head(a.seed[0], a.salt);
        const unsigned e0 = (unsigned)tid * W;                          // < kMaxBlocks * kThreads * 4 = 2^21
        p.row = e0 / a.C;
        p.col = e0 % a.C;
    }
    for (int64_t u = tid; u < units; u += stride) {                      // u * W + W <= n
        float k[W];
        if (HASH) {
            CellPos q = p;
#pragma unroll
            for (int j = 0; j < W; ++j) {
                k[j] = cell_hash_tail(head, q.row, q.col) >= a.thr ? a.scale : 0.f;
                q.next(a.C);
            }
            p.jump(a);
        } else {
#pragma unroll
            for (int j = 0; j < W; ++j) k[j] = a.scale;
        }
        if (W == 4) {
            const cell_f4 xv = reinterpret_cast<const cell_f4*>(a.x)[u];
            cell_f4 gv = {0.f, 0.f, 0.f, 0.f}, ov;
            if (BWD) gv = reinterpret_cast<const cell_f4*>(a.g)[u];
#pragma unroll
            for (int j = 0; j < 4; ++j) ov[j] = cell_one<BWD>(a, xv[j], gv[j], k[j]);
            reinterpret_cast<cell_f4*>(a.out)[u] = ov;
        } else {
            a.out[u] = cell_one<BWD>(a, a.x[u], BWD ? a.g[u] : 0.f, k[0]);
        }
    }
    if (W == 4) {                                                        // the n % 4 elements behind the last vector
        const int64_t e = units * 4 + tid;
        if (tid < 4 && e < a.n) {
            float k = a.scale;
            if (HASH) k = cell_hash_tail(head, (unsigned)(e / a.C), (unsigned)(e % a.C)) >= a.thr ? a.scale : 0.f;
            a.out[e] = cell_one<BWD>(a, a.x[e], BWD ? a.g[e] : 0.f, k);
        }
    }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }

template <bool BWD>
int cell_launch(const char* what, const float* g, const float* x, int saved_is_input, int64_t N, int C, int act, float rate,
                const unsigned* seed, unsigned salt, float* out, void* stream) {
    DT_REQUIRE(act >= 0 && act < DT_CELL_ACT_COUNT, "%s: unknown activation code %d", what, act);
    DT_REQUIRE(N >= 1 && N < ((int64_t)1 << 31) && C >= 1 && N * (int64_t)C < kMaxElems,
               "%s: N %lld, C %d outside 1 <= N < 2^31, C >= 1, N C < 2^40", what, (long long)N, C);
    DT_REQUIRE(rate >= 0.f && rate <= 1.f, "%s: rate %g outside [0, 1]", what, (double)rate);
    DT_REQUIRE(x && out && (!BWD || g), "%s: null tensor", what);
    DT_REQUIRE(aligned4(x) && aligned4(out) && aligned4(g) && aligned4(seed), "%s: misaligned pointer", what);
    const bool hash = rate > 0.f && rate < 1.f;
    DT_REQUIRE(!hash || seed, "%s: 0 < rate < 1 needs the seed word", what);
    CellArgs a;
    a.x = x; a.g = g; a.out = out; a.seed = seed;
    a.n = N * (int64_t)C;
    a.C = (unsigned)C;
    a.act = act;
    a.saved_is_input = saved_is_input;
    a.salt = salt;
    a.thr = cell_threshold(rate);
    a.scale = hash ? 1.f / (1.f - rate) : (rate == 1.f ? 0.f : 1.f);
    const bool vec = a.n >= 4 && aligned16(x) && aligned16(out) && (!BWD || aligned16(g));
    const int W = vec ? 4 : 1;
    const int64_t units = a.n / W;
    const int64_t want = (units + kThreads - 1) / kThreads;
    const unsigned blocks = (unsigned)(want < kMaxBlocks ? want : kMaxBlocks);
    const uint64_t step = (uint64_t)blocks * kThreads * W;               // <= 2^21 elements
    a.step_rows = (unsigned)(step / a.C);
    a.step_cols = (unsigned)(step % a.C);
    hipStream_t st = as_stream(stream);
    if (vec) {
        if (hash) hipLaunchKernelGGL((k_cell<4, true, BWD>), dim3(blocks), dim3(kThreads), 0, st, a);
        else hipLaunchKernelGGL((k_cell<4, false, BWD>), dim3(blocks), dim3(kThreads), 0, st, a);
    } else {
        if (hash) hipLaunchKernelGGL((k_cell<1, true, BWD>), dim3(blocks), dim3(kThreads), 0, st, a);
        else hipLaunchKernelGGL((k_cell<1, false, BWD>), dim3(blocks), dim3(kThreads), 0, st, a);
    }
    return launch_status(what);
}

}  // namespace
}  // namespace dt

using namespace dt;

extern "C" unsigned dt_cell_dropout_hash(unsigned seed, unsigned salt, unsigned row, unsigned col) {
    return cell_hash_tail(cell_hash_head(seed, salt), row, col);
}

extern "C" unsigned dt_cell_dropout_threshold(float rate) { return cell_threshold(rate); }

extern "C" int64_t dt_cell_pass_elems(void) { return (int64_t)kMaxBlocks * kThreads * 4; }

extern "C" int dt_cell_saves_input(int act) {
    DT_REQUIRE(act >= 0 && act < DT_CELL_ACT_COUNT, "dt_cell_saves_input: unknown activation code %d", act);
    return act == DT_CELL_ACT_SILU || act == DT_CELL_ACT_GELU || act == DT_CELL_ACT_MISH || act == DT_CELL_ACT_HARD_SILU;
}

extern "C" int dt_cell_fwd(const float* x, int64_t N, int C, int act, float rate, const unsigned* seed, unsigned salt,
                           float* out, void* stream) {
    return cell_launch<false>("dt_cell_fwd", nullptr, x, 1, N, C, act, rate, seed, salt, out, stream);
}

extern "C" int dt_cell_bwd(const float* g, const float* saved, int saved_is_input, int64_t N, int C, int act, float rate,
                           const unsigned* seed, unsigned salt, float* dx, void* stream) {
    const bool needs_input = act == DT_CELL_ACT_SILU || act == DT_CELL_ACT_GELU || act == DT_CELL_ACT_MISH ||
                             act == DT_CELL_ACT_HARD_SILU;
    DT_REQUIRE(!needs_input || saved_is_input, "dt_cell_bwd: activation code %d takes its derivative from the input", act);
    DT_REQUIRE(saved_is_input || !(rate > 0.f && rate < 1.f),
               "dt_cell_bwd: with 0 < rate < 1 the saved tensor is the input (the scaled output does not decide the kinks)");
    return cell_launch<true>("dt_cell_bwd", g, saved, saved_is_input != 0, N, C, act, rate, seed, salt, dx, stream);
}
