// coalition.hip — the three device stages of KernelSHAP on a resident feed (utils/shap.py, ops.coalition_fill / coalition_mean /
// shap_solve).
//
// An explained row x, Nb background rows bg and S coalitions (bit-packed masks: bit g % 32 of word g / 32 of a coalition's W
// words holds player g) give S Nb synthetic rows per feed block; the model scores them; their outputs are averaged over the
// background per coalition; the Shapley values are a fixed linear map of those averages.
//     dt_coalition_fill   out[(s - s0) Nb + b, c] = bit(masks[s], group[c]) ? x[c] : bg[b, c]        for s in [s0, s1)
//     dt_coalition_mean   ey[seg, o] = (1 / Nb) sum_b out[seg Nb + b, o]                              float32 in, float64 out
//     dt_shap_solve       y'_s = ey_s - e0 - z_{s, M-1} (fx - e0);  phi_j = sum_s P[j, s] y'_s  (j < M - 1);
//                         phi_{M-1} = (fx - e0) - sum_j phi_j                                        all float64
// fill moves 4-byte words and never interprets them (int32 ids and float32 values alike: NaN payloads, -0.0 and denormals
// survive).  One thread per word (a uint4 of four where C % 4 == 0 and x, bg and out are 16-byte aligned: the four selects
// stay per word), 256-thread blocks, a grid-stride loop under kCoalitionMaxBlocks blocks, 64-bit element indices.  group[c]
// == -1: the column always takes the background word.  The entry point checks a HOST copy of group against [-1, M) before
// the launch; the kernel reads the device copy and treats anything outside [0, M) as -1, so no value of it can index past
// a coalition's W words.
//
// mean and solve sum in a FIXED order so that the bits are the same on every run: one wave per sum, lane l adds the terms
// l, l + 64, l + 128, ... in that order, then a six-step butterfly (xor 32, 16, 8, 4, 2, 1) that leaves the same value in every
// lane.  No atomics.  A NaN term makes its own sum NaN and no other.
#include "common.h"
#include "optim_dev.h"

namespace dt {

constexpr int kCoalitionMaxBlocks = 2048;      // as kColumnMaxBlocks (feed_columns.hip)
constexpr int kWavesPerBlock = 4;              // 256 threads

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ bool coalition_bit(const uint32_t* __restrict__ mask, int g, int M) {
    return g >= 0 && g < M && ((mask[g >> 5] >> (g & 31)) & 1u);
}

// total = rows * C words
__global__ __launch_bounds__(256) void k_coalition_fill(const uint32_t* __restrict__ x, const uint32_t* __restrict__ bg,
                                                         const uint32_t* __restrict__ masks, const int32_t* __restrict__ group,
                                                         uint32_t* __restrict__ out, int64_t s0, int64_t Nb, int64_t C, int M,
                                                         int W, int64_t total) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += stride) {
        const int64_t row = e / C, c = e - row * C;
        const int64_t s = row / Nb, b = row - s * Nb;
        out[e] = coalition_bit(masks + (s0 + s) * W, group[c], M) ? x[c] : bg[b * C + c];
    }
}

// C4 = C / 4 uint4 per row; total = rows * C4
__global__ __launch_bounds__(256) void k_coalition_fill4(const uint4* __restrict__ x, const uint4* __restrict__ bg,
                                                          const uint32_t* __restrict__ masks, const int32_t* __restrict__ group,
                                                          uint4* __restrict__ out, int64_t s0, int64_t Nb, int64_t C4, int M,
                                                          int W, int64_t total) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += stride) {
        const int64_t row = e / C4, c4 = e - row * C4;
        const int64_t s = row / Nb, b = row - s * Nb;
        const uint32_t* mask = masks + (s0 + s) * W;
        const uint4 xv = x[c4];
        uint4 v = bg[b * C4 + c4];
        const int32_t* g = group + c4 * 4;
        if (coalition_bit(mask, g[0], M)) v.x = xv.x;
        if (coalition_bit(mask, g[1], M)) v.y = xv.y;
        if (coalition_bit(mask, g[2], M)) v.z = xv.z;
        if (coalition_bit(mask, g[3], M)) v.w = xv.w;
        out[e] = v;
    }
}

// one wave per (segment, output); nsums = nseg * O
__global__ __launch_bounds__(256) void k_coalition_mean(const float* __restrict__ out, int64_t nsums, int64_t Nb, int64_t O,
                                                         double* __restrict__ ey) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    const int64_t stride = (int64_t)gridDim.x * kWavesPerBlock;
    for (int64_t i = wave; i < nsums; i += stride) {
        const int64_t seg = i / O, o = i - seg * O;
        const float* at = out + seg * Nb * O + o;
        double acc = 0.0;
        for (int64_t b = lane; b < Nb; b += 64) acc += (double)at[b * O];
        acc = wave_sum_f64(acc);
        if (lane == 0) ey[i] = acc / (double)Nb;
    }
}

// one block per (explained row, output): its waves take the players j < M - 1 in turn, then wave 0 closes the sum
__global__ __launch_bounds__(256) void k_shap_solve(const double* __restrict__ P, const uint32_t* __restrict__ masks,
                                                     const double* __restrict__ ey, const double* __restrict__ fx,
                                                     const double* __restrict__ e0, double* __restrict__ phi, int64_t RO,
                                                     int64_t S, int64_t O, int M, int W) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int last = M - 1;
    for (int64_t ro = blockIdx.x; ro < RO; ro += gridDim.x) {
        const int64_t r = ro / O, o = ro - r * O;
        const double base = e0[o], delta = fx[ro] - base;
        const double* eyr = ey + r * S * O + o;
        double* out = phi + ro * M;
        for (int j = wave; j < last; j += kWavesPerBlock) {
            const double* Pj = P + (int64_t)j * S;
            double acc = 0.0;
            for (int64_t s = lane; s < S; s += 64) {
                const bool z = (masks[s * W + (last >> 5)] >> (last & 31)) & 1u;
                const double y = (eyr[s * O] - base) - (z ? delta : 0.0);
                acc += Pj[s] * y;
            }
            acc = wave_sum_f64(acc);
            if (lane == 0) out[j] = acc;
        }
        __syncthreads();                    // the block's own stores to out[0 .. M-2] are visible to wave 0
        if (wave == 0) {
            double acc = 0.0;
            for (int j = lane; j < last; j += 64) acc += out[j];
            acc = wave_sum_f64(acc);
            if (lane == 0) out[last] = delta - acc;
        }
        __syncthreads();
    }
}

inline unsigned coalition_grid(int64_t blocks) {
    return (unsigned)(blocks < kCoalitionMaxBlocks ? blocks : kCoalitionMaxBlocks);
}

constexpr int64_t kMaxWords = (int64_t)1 << 62;

}  // namespace dt

using namespace dt;

extern "C" int dt_coalition_fill(const void* x, const void* bg, int64_t Nb, int C, const uint32_t* masks, int64_t S, int M,
                                 int64_t s0, int64_t s1, const int32_t* group, const int32_t* group_host, void* out,
                                 void* stream) {
    const char* who = "dt_coalition_fill";
    DT_REQUIRE(Nb >= 0 && C >= 0 && S >= 0 && M >= 1, "%s: bad sizes Nb=%lld C=%d S=%lld M=%d", who, (long long)Nb, C,
               (long long)S, M);
    DT_REQUIRE(s0 >= 0 && s0 <= s1 && s1 <= S, "%s: coalitions [%lld, %lld) of %lld", who, (long long)s0, (long long)s1,
               (long long)S);
    DT_REQUIRE(x && bg && masks && group && group_host && out, "%s: null pointer", who);
    DT_REQUIRE(aligned_to(x, 4) && aligned_to(bg, 4) && aligned_to(masks, 4) && aligned_to(group, 4) &&
               aligned_to(group_host, 4) && aligned_to(out, 4), "%s: misaligned pointer", who);
    const int64_t rows = (s1 - s0) * Nb;
    DT_REQUIRE(Nb == 0 || s1 - s0 <= kMaxWords / Nb, "%s: (s1 - s0) Nb overflows", who);
    DT_REQUIRE(C == 0 || rows <= kMaxWords / C, "%s: (s1 - s0) Nb C overflows", who);
    for (int c = 0; c < C; ++c)
        DT_REQUIRE(group_host[c] >= -1 && group_host[c] < M, "%s: group[%d] = %d is outside [-1, %d)", who, c,
                   (int)group_host[c], M);
    if (rows == 0 || C == 0) return DT_OK;
    const int W = (M + 31) / 32;
    if (C % 4 == 0 && aligned_to(x, 16) && aligned_to(bg, 16) && aligned_to(out, 16)) {
        const int64_t total = rows * (C / 4);
        hipLaunchKernelGGL(k_coalition_fill4, dim3(coalition_grid((total + 255) / 256)), dim3(256), 0, as_stream(stream),
                           (const uint4*)x, (const uint4*)bg, masks, group, (uint4*)out, s0, Nb, (int64_t)(C / 4), M, W, total);
    } else {
        const int64_t total = rows * C;
        hipLaunchKernelGGL(k_coalition_fill, dim3(coalition_grid((total + 255) / 256)), dim3(256), 0, as_stream(stream),
                           (const uint32_t*)x, (const uint32_t*)bg, masks, group, (uint32_t*)out, s0, Nb, (int64_t)C, M, W,
                           total);
    }
    return launch_status(who);
}

extern "C" int dt_coalition_mean(const float* out, int64_t nseg, int64_t Nb, int O, double* ey, void* stream) {
    const char* who = "dt_coalition_mean";
    DT_REQUIRE(nseg >= 0 && Nb >= 1 && O >= 0, "%s: bad sizes nseg=%lld Nb=%lld O=%d", who, (long long)nseg, (long long)Nb, O);
    DT_REQUIRE(out && ey, "%s: null pointer", who);
    DT_REQUIRE(aligned_to(out, 4) && aligned_to(ey, 8), "%s: misaligned pointer", who);
    DT_REQUIRE(O == 0 || nseg <= kMaxWords / O, "%s: nseg O overflows", who);
    DT_REQUIRE(nseg * (O ? O : 1) <= kMaxWords / Nb, "%s: nseg Nb O overflows", who);
    const int64_t nsums = nseg * O;
    if (nsums == 0) return DT_OK;
    hipLaunchKernelGGL(k_coalition_mean, dim3(coalition_grid((nsums + kWavesPerBlock - 1) / kWavesPerBlock)), dim3(256), 0,
                       as_stream(stream), out, nsums, Nb, (int64_t)O, ey);
    return launch_status(who);
}

extern "C" int dt_shap_solve(const double* P, const uint32_t* masks, int64_t S, int M, const double* ey, const double* fx,
                             const double* e0, int64_t R, int O, double* phi, void* stream) {
    const char* who = "dt_shap_solve";
    DT_REQUIRE(S >= 1 && M >= 2 && R >= 0 && O >= 0, "%s: bad sizes S=%lld M=%d R=%lld O=%d", who, (long long)S, M,
               (long long)R, O);
    DT_REQUIRE(P && masks && ey && fx && e0 && phi, "%s: null pointer", who);
    DT_REQUIRE(aligned_to(P, 8) && aligned_to(masks, 4) && aligned_to(ey, 8) && aligned_to(fx, 8) && aligned_to(e0, 8) &&
               aligned_to(phi, 8), "%s: misaligned pointer", who);
    DT_REQUIRE(S <= kMaxWords / M, "%s: S M overflows", who);
    DT_REQUIRE(O == 0 || R <= kMaxWords / O, "%s: R O overflows", who);
    const int64_t RO = R * O;
    DT_REQUIRE(RO == 0 || (RO <= kMaxWords / S && RO <= kMaxWords / M), "%s: R O S overflows", who);
    if (RO == 0) return DT_OK;
    hipLaunchKernelGGL(k_shap_solve, dim3(coalition_grid(RO)), dim3(256), 0, as_stream(stream), P, masks, ey, fx, e0, phi, RO, S,
                       (int64_t)O, M, (M + 31) / 32);
    return launch_status(who);
}
