// loss_sum.h — what the loss translation units (loss.hip, loss_reg.hip) share: the shape domain, the checks on an entry's
// buffers, the fixed-order float64 sums, and the ONE element-wise kernel.
//
// Geometry: 256 threads; a block of the element-wise kinds takes kElemChunk consecutive elements of the flat [rows * classes]
// array, thread t the elements t, t + 256, ... of the chunk (coalesced); the row of an element (for its weight) is e / classes.
// Sums: a thread / lane adds its elements in index order, the lanes of a wave combine by halving, the waves of a block in order,
// ONE double per block goes into the caller's workspace at the block's index, and k_loss_total adds the partials (thread t takes
// t, t + 256, ... in index order, then the same tree), scales and writes the float32 loss.  One block that covers the problem
// writes the loss itself: one launch.
//
// k_loss_elem<Term> is that skeleton; a kind is a term functor: the kind's scalars, `operator()(z, t, &f, &g)` = the element's
// loss term and its derivative in z (float32), and `tail(&s)` = what a thread adds to its sum behind its elements — nothing
// (NoTail) but for the binary focal loss.
#pragma once
#include <math.h>

#include "common.h"

namespace dt {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr int kElemChunk = 2048;              // elements per block of the element-wise kinds
constexpr int64_t kMaxRows = (int64_t)1 << 31;
constexpr int64_t kMaxElems = (int64_t)1 << 40;   // rows * classes: the block count of a launch stays below 2^31
constexpr float kEps = 1e-7f;                 // keras.backend.epsilon()

inline bool shape_ok(int64_t rows, int classes) {
    // (rows * classes < 2^43: no overflow, and at most 2^32 / 2 blocks only below 2^42 elements — held to 2^40)
    return rows >= 1 && rows < kMaxRows && classes >= 1 && classes <= DT_LOSS_MAX_CLASSES && rows * classes < kMaxElems;
}
inline int64_t elem_blocks(int64_t n) { return (n + kElemChunk - 1) / kElemChunk; }

inline uintptr_t addr(const void* p) { return reinterpret_cast<uintptr_t>(p); }

// the checks every entry makes on its buffers, under the entry's name: `inputs` is what it calls z, `others` the addresses of
// its further float arrays, or-ed
inline int check_buffers(const char* entry, const char* inputs, const void* z, const void* t, const void* loss,
                         const void* workspace, uintptr_t others) {
    DT_REQUIRE(z && t && loss, "%s: null %s, targets or loss", entry, inputs);
    DT_REQUIRE(workspace && (addr(workspace) & 7) == 0, "%s: null or misaligned workspace", entry);
    DT_REQUIRE(((addr(z) | addr(t) | addr(loss) | others) & 3) == 0, "%s: misaligned pointer", entry);
    return DT_OK;
}

// lanes by halving; every lane returns lane 0's total
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) v += __shfl_down(v, o, kWave);
    return __shfl(v, 0, kWave);
}

// the waves' values in order; thread 0 holds the block's sum
__device__ __forceinline__ double waves_in_order(double wave_value, double* sh) {
    if ((threadIdx.x & (kWave - 1)) == 0) sh[threadIdx.x / kWave] = wave_value;
    __syncthreads();
    double all = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) all += sh[w];
    return all;
}

__device__ __forceinline__ float sigmoid_f(float z) {
    const float e = expf(-fabsf(z));
    return z >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
}

__global__ __launch_bounds__(kThreads) void k_loss_total(const double* __restrict__ partial, int64_t count, double inv,
                                                         float* __restrict__ loss) {
    __shared__ double sh[kWaves];
    double s = 0;
    for (int64_t i = threadIdx.x; i < count; i += kThreads) s += partial[i];
    s = wave_sum_f64(s);
    const double all = waves_in_order(s, sh);
    if (threadIdx.x == 0) loss[0] = (float)(all * inv);
}

struct ElemArgs {
    const float* z;          // logits / predictions [rows * classes]
    const float* t;
    const float* w;          // [rows] or null
    float* dz;               // [rows * classes] or null
    float* loss;             // [1]
    double* partial;         // one double per block
    int64_t n;               // rows * classes
    int classes;
    int final;               // the launch has one block, which writes the loss itself
    float scale;             // fl(1 / (rows classes)) (categorical kinds: fl(1 / rows)): dz = w_b * scale * dl/dz
    double inv;              // the same in double: loss = inv * sum
};

// a mean over all rows * classes elements
inline ElemArgs elem_args(const float* z, const float* t, const float* w, int64_t rows, int classes, float* loss, float* dz,
                          void* workspace) {
    ElemArgs a;
    a.z = z; a.t = t; a.w = w; a.dz = dz; a.loss = loss;
    a.partial = reinterpret_cast<double*>(workspace);
    a.n = rows * classes; a.classes = classes; a.final = 0;
    a.inv = 1.0 / ((double)rows * (double)classes);
    a.scale = (float)a.inv;
    return a;
}

__device__ __forceinline__ void finish_block(const ElemArgs& a, double block_sum) {
    if (threadIdx.x == 0) {
        if (a.final) a.loss[0] = (float)(block_sum * a.inv);
        else a.partial[blockIdx.x] = block_sum;
    }
}

struct NoTail {
    __device__ __forceinline__ void tail(double*) const {}
};

// the stable form max(z,0) - z t + log1p(exp(-|z|)) and sigmoid(z) - t: DT_LOSS_BCE, and GHM-C's element
struct BceTerm : NoTail {
    __device__ __forceinline__ void operator()(float z, float t, float* f, float* g) const {
        *f = fmaxf(z, 0.f) - z * t + log1pf(expf(-fabsf(z)));
        *g = sigmoid_f(z) - t;
    }
};

template <class Term>
__global__ __launch_bounds__(kThreads) void k_loss_elem(ElemArgs a, Term term) {
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
        term(a.z[e], a.t[e], &f, &g);
        s += (double)wb * (double)f;
        if (a.dz) a.dz[e] = (wb * a.scale) * g;
    }
    term.tail(&s);
    s = wave_sum_f64(s);
    finish_block(a, waves_in_order(s, sh));
}

// behind a launch of `blocks` blocks that left their partials: their sum
inline void launch_total(const ElemArgs& a, int64_t blocks, hipStream_t st) {
    if (blocks > 1)
        hipLaunchKernelGGL(k_loss_total, dim3(1), dim3(kThreads), 0, st, (const double*)a.partial, blocks, a.inv, a.loss);
}

template <class Term>
inline void launch_elem(ElemArgs a, const Term& term, hipStream_t st) {
    const int64_t blocks = elem_blocks(a.n);
    a.final = blocks == 1;
    hipLaunchKernelGGL(k_loss_elem<Term>, dim3((unsigned)blocks), dim3(kThreads), 0, st, a, term);
    launch_total(a, blocks, st);
}

}  // namespace
}  // namespace dt
