// regularizer.hip — keras.regularizers.L1L2 on the device (gfx950, wave64): the penalty l1 * sum|x| + l2 * sum x^2 of up to
// N tensors in one call, and its gradient go * (l1 * sign(x) + 2 * l2 * x) for the same N tensors in one launch.
//
// Both are bandwidth bound (one read per element for the penalty, one read and one write for the gradient).  The tensors'
// descriptors travel as kernel arguments in chunks of kRegMax (optim.hip's k_adam_multi scheme: no device-side table to keep
// in sync, replayable from a hipGraph); a block finds its tensor by scanning the block offsets.
//
// Penalty, two launches.  k_reg_partial: a block takes one chunk of kRegChunk consecutive elements of one tensor; thread t owns
// the groups of four elements t, t + 256, ... of the chunk and adds |x| and x * x in float64 (x * x is exact in double) in that
// order — the same elements in the same order whether the group is read as one float4 or as four floats, so an unaligned view
// gives the bits of an aligned one.  The block's sums are combined in a fixed order (lanes by halving, then the waves in order)
// and ONE double, l1 * S1 + l2 * S2, goes into the caller's workspace at the block's global index.  k_reg_total: one block
// adds the partials (thread t takes t, t + 256, ... in index order, then the same fixed tree) and writes the total as a
// double and as its float32 rounding.  No float atomics, no block waits for another: the same input gives the same bits.
// A coefficient that is zero contributes no term at all (Keras: `if self.l1:`), so l1 = 0 does not turn an Inf into a NaN.
//
// Gradient, one launch per kRegMax tensors.  The formula is written once (reg_grad_one) with contraction off; float4 where the
// input and output pointers allow it, scalars for the unaligned head, the tail and every tensor whose pointers disagree.
#include "common.h"

namespace dt {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr int kRegMax = 32;                       // tensors per launch
constexpr int kRegChunk = 4096;                   // elements per block: dt_reg_chunk()
constexpr int64_t kRegMaxN = (int64_t)1 << 40;    // per tensor; the block count of a launch is checked separately

struct RegPenaltyMulti {
    const float* x[kRegMax];
    int64_t n[kRegMax];
    double l1[kRegMax];
    double l2[kRegMax];
    int block_start[kRegMax + 1];
    int count;
};

struct RegGradMulti {
    const float* x[kRegMax];
    float* out[kRegMax];
    int64_t n[kRegMax];
    float l1[kRegMax];
    float two_l2[kRegMax];
    int head[kRegMax];           // scalar elements in front of the float4 body; -1: the whole tensor goes the scalar way
    int block_start[kRegMax + 1];
    int count;
};

inline int64_t chunks_of(int64_t n) { return (n + kRegChunk - 1) / kRegChunk; }

// sum over the block in a fixed order (lanes by halving, then the waves in order); thread 0's value is the block's
__device__ __forceinline__ double block_sum_f64(double v, double* sh) {
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) v += __shfl_down(v, o, kWave);
    if ((threadIdx.x & (kWave - 1)) == 0) sh[threadIdx.x / kWave] = v;
    __syncthreads();
    double all = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) all += sh[w];
    __syncthreads();
    return all;
}

__global__ __launch_bounds__(kThreads) void k_reg_partial(RegPenaltyMulti d, double* __restrict__ partial) {
    __shared__ double sh[kWaves];
    int t = 0;
    while (t + 1 < d.count && (int)blockIdx.x >= d.block_start[t + 1]) ++t;
    const float* __restrict__ x = d.x[t];
    const int64_t lo = (int64_t)(blockIdx.x - d.block_start[t]) * kRegChunk;
    const int64_t rest = d.n[t] - lo;
    const int m = rest < kRegChunk ? (int)rest : kRegChunk;        // >= 1: the host counts ceil(n / kRegChunk) blocks
    const bool vec = (reinterpret_cast<uintptr_t>(x + lo) & 15) == 0;
    double s1 = 0, s2 = 0;
    for (int g = threadIdx.x; g * 4 < m; g += kThreads) {
        float e[4] = {0.f, 0.f, 0.f, 0.f};
        const int left = m - g * 4;
        if (vec && left >= 4) {
            const float4 q = *reinterpret_cast<const float4*>(x + lo + g * 4);
            e[0] = q.x; e[1] = q.y; e[2] = q.z; e[3] = q.w;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < left) e[k] = x[lo + g * 4 + k];
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {            // (a slot past the end holds +0: |0| and 0 * 0 add nothing)
            const double v = (double)e[k];
            s1 += fabs(v);
            s2 += v * v;
        }
    }
    s1 = block_sum_f64(s1, sh);
    s2 = block_sum_f64(s2, sh);
    if (threadIdx.x == 0) {
        double p = 0;
        if (d.l1[t] != 0) p += d.l1[t] * s1;
        if (d.l2[t] != 0) p += d.l2[t] * s2;
        partial[blockIdx.x] = p;
    }
}

__global__ __launch_bounds__(kThreads) void k_reg_total(const double* __restrict__ partial, int64_t count,
                                                        double* __restrict__ total, float* __restrict__ total_f32) {
    __shared__ double sh[kWaves];
    double s = 0;
    for (int64_t i = threadIdx.x; i < count; i += kThreads) s += partial[i];
    s = block_sum_f64(s, sh);
    if (threadIdx.x == 0) {
        total[0] = s;
        total_f32[0] = (float)s;
    }
}

// the gradient of one element, in this fp32 order and with no contraction: t = fl(fl(2 l2) x), u = +-l1 or 0 (sign(+-0) = 0,
// a NaN has no sign and propagates through t), r = fl(u + t), fl(go r)
__device__ __forceinline__ float reg_grad_one(float x, float l1, float two_l2, float go) {
#pragma clang fp contract(off)
    const float t = two_l2 * x;
    const float u = x > 0.f ? l1 : (x < 0.f ? -l1 : 0.f);
    const float r = u + t;
    return go * r;
}
__device__ __forceinline__ float reg_grad_acc(float g, float v) {
#pragma clang fp contract(off)
    return g + v;
}

template <bool ACC>
__global__ __launch_bounds__(kThreads) void k_reg_grad(RegGradMulti d, const float* __restrict__ go_ptr) {
    int t = 0;
    while (t + 1 < d.count && (int)blockIdx.x >= d.block_start[t + 1]) ++t;
    const float* __restrict__ x = d.x[t];
    float* __restrict__ out = d.out[t];
    const int64_t n = d.n[t];
    const float l1 = d.l1[t], two_l2 = d.two_l2[t], go = go_ptr[0];
    const bool vec = d.head[t] >= 0;
    const int64_t head = vec ? d.head[t] : 0;
    const int64_t c = blockIdx.x - d.block_start[t];
    if (c == 0 && (int64_t)threadIdx.x < head) {          // head <= 3 and head <= n
        const float v = reg_grad_one(x[threadIdx.x], l1, two_l2, go);
        out[threadIdx.x] = ACC ? reg_grad_acc(out[threadIdx.x], v) : v;
    }
    const int64_t lo = head + c * kRegChunk;
    const int64_t rest = n - lo;
    const int m = rest < kRegChunk ? (rest > 0 ? (int)rest : 0) : kRegChunk;
    const int nv = vec ? m / 4 : 0;
    for (int g = threadIdx.x; g < nv; g += kThreads) {
        const float4 q = *reinterpret_cast<const float4*>(x + lo + g * 4);
        float4 r;
        r.x = reg_grad_one(q.x, l1, two_l2, go);
        r.y = reg_grad_one(q.y, l1, two_l2, go);
        r.z = reg_grad_one(q.z, l1, two_l2, go);
        r.w = reg_grad_one(q.w, l1, two_l2, go);
        float4* o = reinterpret_cast<float4*>(out + lo + g * 4);
        if (ACC) {
            const float4 a = *o;
            r.x = reg_grad_acc(a.x, r.x);
            r.y = reg_grad_acc(a.y, r.y);
            r.z = reg_grad_acc(a.z, r.z);
            r.w = reg_grad_acc(a.w, r.w);
        }
        *o = r;
    }
    for (int i = nv * 4 + threadIdx.x; i < m; i += kThreads) {
        const float v = reg_grad_one(x[lo + i], l1, two_l2, go);
        out[lo + i] = ACC ? reg_grad_acc(out[lo + i], v) : v;
    }
}

// blocks of the gradient launch for one tensor: the float4 body starts `head` elements in, block 0 also takes the head
inline int64_t grad_blocks(int64_t n, int head) {
    if (n == 0) return 0;
    const int64_t h = head > 0 ? head : 0;
    return n > h ? chunks_of(n - h) : 1;
}

}  // namespace
}  // namespace dt

using namespace dt;

extern "C" int dt_reg_chunk(void) { return kRegChunk; }

extern "C" int64_t dt_reg_penalty_workspace_bytes(int count, const int64_t* n) {
    if (count < 0 || (count > 0 && !n)) return DT_ERR_INVALID_ARG;
    int64_t blocks = 0;
    for (int t = 0; t < count; ++t) {
        if (n[t] < 0 || n[t] >= kRegMaxN) return DT_ERR_INVALID_ARG;
        blocks += chunks_of(n[t]);
    }
    return (blocks > 0 ? blocks : 1) * (int64_t)sizeof(double);
}

extern "C" int dt_reg_penalty(int count, const float* const* x, const int64_t* n, const double* l1, const double* l2,
                              void* workspace, double* total, float* total_f32, void* stream) {
    DT_REQUIRE(count >= 0, "dt_reg_penalty: negative tensor count %d", count);
    DT_REQUIRE(count == 0 || (x && n && l1 && l2), "dt_reg_penalty: null descriptor array");
    DT_REQUIRE(total && total_f32, "dt_reg_penalty: null output");
    DT_REQUIRE((reinterpret_cast<uintptr_t>(total) & 7) == 0 && (reinterpret_cast<uintptr_t>(total_f32) & 3) == 0,
               "dt_reg_penalty: misaligned output");
    int64_t all_blocks = 0;
    for (int t = 0; t < count; ++t) {                     // everything is validated before the first launch
        DT_REQUIRE(n[t] >= 0 && n[t] < kRegMaxN, "dt_reg_penalty: tensor %d: bad size %lld", t, (long long)n[t]);
        DT_REQUIRE(n[t] == 0 || x[t], "dt_reg_penalty: tensor %d: null pointer with n > 0", t);
        DT_REQUIRE((reinterpret_cast<uintptr_t>(x[t]) & 3) == 0, "dt_reg_penalty: tensor %d: misaligned pointer", t);
        all_blocks += chunks_of(n[t]);
    }
    DT_REQUIRE(all_blocks < ((int64_t)1 << 31), "dt_reg_penalty: %lld chunks in one call", (long long)all_blocks);
    DT_REQUIRE(all_blocks == 0 || (workspace && (reinterpret_cast<uintptr_t>(workspace) & 7) == 0),
               "dt_reg_penalty: null or misaligned workspace");
    hipStream_t st = as_stream(stream);
    double* partial = reinterpret_cast<double*>(workspace);
    int64_t done = 0;
    for (int c0 = 0; c0 < count; c0 += kRegMax) {
        RegPenaltyMulti d;
        d.count = 0;
        int blocks = 0;
        for (int t = c0; t < count && t < c0 + kRegMax; ++t) {
            if (n[t] == 0) continue;                      // an empty member contributes nothing
            const int k = d.count++;
            d.x[k] = x[t]; d.n[k] = n[t]; d.l1[k] = l1[t]; d.l2[k] = l2[t];
            d.block_start[k] = blocks;
            blocks += (int)chunks_of(n[t]);
        }
        d.block_start[d.count] = blocks;
        if (blocks == 0) continue;
        hipLaunchKernelGGL(k_reg_partial, dim3(blocks), dim3(kThreads), 0, st, d, partial + done);
        done += blocks;
    }
    hipLaunchKernelGGL(k_reg_total, dim3(1), dim3(kThreads), 0, st, (const double*)partial, all_blocks, total, total_f32);
    return launch_status("dt_reg_penalty");
}

extern "C" int dt_reg_grad(int count, const float* const* x, float* const* out, const int64_t* n, const float* l1,
                           const float* l2, const float* go, int accumulate, void* stream) {
    DT_REQUIRE(count >= 0, "dt_reg_grad: negative tensor count %d", count);
    DT_REQUIRE(count == 0 || (x && out && n && l1 && l2), "dt_reg_grad: null descriptor array");
    DT_REQUIRE(go, "dt_reg_grad: null upstream gradient");
    int64_t all_blocks = 0;
    for (int t = 0; t < count; ++t) {
        DT_REQUIRE(n[t] >= 0 && n[t] < kRegMaxN, "dt_reg_grad: tensor %d: bad size %lld", t, (long long)n[t]);
        DT_REQUIRE(n[t] == 0 || (x[t] && out[t]), "dt_reg_grad: tensor %d: null pointer with n > 0", t);
        DT_REQUIRE(((reinterpret_cast<uintptr_t>(x[t]) | reinterpret_cast<uintptr_t>(out[t])) & 3) == 0,
                   "dt_reg_grad: tensor %d: misaligned pointer", t);
        all_blocks += chunks_of(n[t]) + 1;
    }
    DT_REQUIRE(all_blocks < ((int64_t)1 << 31), "dt_reg_grad: %lld chunks in one call", (long long)all_blocks);
    hipStream_t st = as_stream(stream);
    for (int c0 = 0; c0 < count; c0 += kRegMax) {
        RegGradMulti d;
        d.count = 0;
        int blocks = 0;
        for (int t = c0; t < count && t < c0 + kRegMax; ++t) {
            if (n[t] == 0) continue;
            const int k = d.count++;
            const uintptr_t xa = reinterpret_cast<uintptr_t>(x[t]), oa = reinterpret_cast<uintptr_t>(out[t]);
            // float4 needs the input and the output 16-byte aligned at the same element
            int head = ((xa ^ oa) & 15) == 0 ? (int)(((16 - (xa & 15)) & 15) / 4) : -1;
            if (head > n[t]) head = (int)n[t];
            d.x[k] = x[t]; d.out[k] = out[t]; d.n[k] = n[t]; d.l1[k] = l1[t]; d.two_l2[k] = 2.0f * l2[t];
            d.head[k] = head;
            d.block_start[k] = blocks;
            blocks += (int)grad_blocks(n[t], head);
        }
        d.block_start[d.count] = blocks;
        if (blocks == 0) continue;
        if (accumulate)
            hipLaunchKernelGGL(k_reg_grad<true>, dim3(blocks), dim3(kThreads), 0, st, d, go);
        else
            hipLaunchKernelGGL(k_reg_grad<false>, dim3(blocks), dim3(kThreads), 0, st, d, go);
    }
    return launch_status("dt_reg_grad");
}
