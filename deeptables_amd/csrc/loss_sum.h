// loss_sum.h — the block geometry and the fixed-order float64 sums shared by the loss translation units (loss.hip,
// loss_reg.hip): 256 threads, a thread / lane adds its elements in index order, the lanes of a wave combine by halving, the
// waves of a block in order, ONE double per block goes into the caller's workspace, and k_loss_total adds the partials.
#pragma once
#include <math.h>

#include "common.h"

namespace dt {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr int kElemChunk = 2048;              // elements per block of the element-wise kinds

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

}  // namespace
}  // namespace dt
