// feed_rows.hip — rows of a device-resident feed block gathered and scattered, and the mean of K output buffers
// (models/cross_validation.py: ops.take_rows, ops.put_rows, ops.ensemble_mean).
//
// A feed block is a row-major [N, C] array of 4-byte words (int32 ids or float32 values).  k-fold cross-validation cuts each
// fold's training and validation feeds out of ONE resident feed, writes a fold's outputs into the rows of the out-of-fold
// buffer the fold validated, and averages the fold models' outputs:
//     dt_rows_take       out[i, :] = block[idx[i], :]     i < n   (block is only read; repeats allowed; n may exceed N)
//     dt_rows_put        block[idx[i], :] = src[i, :]     i < n   (a row idx does not name keeps its bits)
//     dt_ensemble_mean   out[e] = mean over k < K of parts[k][e]  (float64 sum / K, or float32 sum of p_k / K)
// Words are moved, never interpreted: NaN payloads, -0.0 and denormals survive take and put.
//
// Launch: 256-thread blocks, one thread per word of [n, C], the threads of a row adjacent so its C contiguous words leave in
// one request, a grid-stride loop under kRowsMaxBlocks blocks, 64-bit element indices.  Where C is a multiple of 4 and both
// pointers 16-byte aligned the word is a uint4 (every count divided by 4).  A block of threads starts at element `base`: the
// row of `base` is ONE 64-bit division per block and pass (uniform), every thread's row and column follow from a 32-bit
// division of its offset inside that row (< C + 256).
// An idx entry outside [0, N) is a caller error that must not become a fault: take writes a row of zero words, put skips the
// row.  Duplicate entries in put's idx are a caller error too: one of the rows wins, word by word.
// The mean takes its K pointers in the kernel's argument struct (no table on the device, nothing to copy: safe to capture);
// each thread sums its element in the order k = 0..K-1 (the float64 sum from +0, the float32 sum from its first quotient, as
// numpy's `acc = zeros; acc += p` and `mean = p0 / K; mean += p / K` do), no atomics: the same bits on every run.
#include "common.h"
#include "optim_dev.h"

namespace dt {

constexpr int kRowsMaxBlocks = 2048;        // 256 CUs x 8 resident blocks of 256 threads; the kernels stride over the rest
constexpr int kMeanMaxParts = 64;

__device__ inline void zero_word(uint32_t& v) { v = 0u; }
__device__ inline void zero_word(uint4& v) { v = make_uint4(0u, 0u, 0u, 0u); }

// total = n * C elements of T
template <typename T>
__global__ __launch_bounds__(256) void k_rows_take(const T* __restrict__ block, int64_t N, uint32_t C,
                                                    const int64_t* __restrict__ idx, T* __restrict__ out, int64_t total) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t base = (int64_t)blockIdx.x * 256; base < total; base += stride) {
        const int64_t i0 = base / C;
        const uint32_t off = (uint32_t)(base - i0 * C) + threadIdx.x;
        const int64_t e = base + threadIdx.x;
        if (e < total) {
            const uint32_t di = off / C, w = off - di * C;
            const int64_t p = idx[i0 + di];
            T v;
            zero_word(v);
            if (p >= 0 && p < N) v = block[p * C + w];
            out[e] = v;
        }
    }
}

template <typename T>
__global__ __launch_bounds__(256) void k_rows_put(T* __restrict__ block, int64_t N, uint32_t C,
                                                   const int64_t* __restrict__ idx, const T* __restrict__ src, int64_t total) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t base = (int64_t)blockIdx.x * 256; base < total; base += stride) {
        const int64_t i0 = base / C;
        const uint32_t off = (uint32_t)(base - i0 * C) + threadIdx.x;
        const int64_t e = base + threadIdx.x;
        if (e < total) {
            const uint32_t di = off / C, w = off - di * C;
            const int64_t p = idx[i0 + di];
            if (p >= 0 && p < N) block[p * C + w] = src[e];
        }
    }
}

struct MeanParts {
    const float* p[kMeanMaxParts];
};

// MODE 0: float64 (sum of (double)p_k) / K;  MODE 1: float32 sum of p_k / (float)K, the division correctly rounded
template <int MODE>
__global__ __launch_bounds__(256) void k_ensemble_mean(MeanParts parts, int K, int64_t total, void* __restrict__ out) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += stride) {
        if (MODE == 0) {
            double acc = 0.0;
            for (int k = 0; k < K; ++k) acc += (double)parts.p[k][e];
            ((double*)out)[e] = acc / (double)K;
        } else {
            const float fk = (float)K;
            float acc = __fdiv_rn(parts.p[0][e], fk);
            for (int k = 1; k < K; ++k) acc += __fdiv_rn(parts.p[k][e], fk);
            ((float*)out)[e] = acc;
        }
    }
}

static int rows_args(const char* who, const void* block, int64_t N, int C, const int64_t* idx, int64_t n, const void* other) {
    DT_REQUIRE(N >= 0 && C >= 1 && n >= 0, "%s: bad sizes N=%lld C=%d n=%lld", who, (long long)N, C, (long long)n);
    DT_REQUIRE(block && idx && other, "%s: null pointer", who);
    DT_REQUIRE(aligned_to(block, 4) && aligned_to(other, 4), "%s: misaligned pointer", who);
    DT_REQUIRE(aligned_to(idx, 8), "%s: misaligned idx", who);
    return DT_OK;
}

inline bool rows_vec4(const void* block, int C, const void* other) {
    return C % 4 == 0 && aligned_to(block, 16) && aligned_to(other, 16);
}

inline unsigned rows_grid(int64_t total) {
    const int64_t blocks = (total + 255) / 256;
    return (unsigned)(blocks < kRowsMaxBlocks ? blocks : kRowsMaxBlocks);
}

}  // namespace dt

using namespace dt;

extern "C" int dt_rows_take(const void* block, int64_t N, int C, const int64_t* idx, int64_t n, void* out, void* stream) {
    const char* who = "dt_rows_take";
    if (int rc = rows_args(who, block, N, C, idx, n, out)) return rc;
    if (n == 0) return DT_OK;
    if (rows_vec4(block, C, out)) {
        const int64_t total = n * (C / 4);
        hipLaunchKernelGGL((k_rows_take<uint4>), dim3(rows_grid(total)), dim3(256), 0, as_stream(stream), (const uint4*)block, N,
                           (uint32_t)(C / 4), idx, (uint4*)out, total);
    } else {
        const int64_t total = n * C;
        hipLaunchKernelGGL((k_rows_take<uint32_t>), dim3(rows_grid(total)), dim3(256), 0, as_stream(stream),
                           (const uint32_t*)block, N, (uint32_t)C, idx, (uint32_t*)out, total);
    }
    return launch_status(who);
}

extern "C" int dt_rows_put(void* block, int64_t N, int C, const int64_t* idx, int64_t n, const void* src, void* stream) {
    const char* who = "dt_rows_put";
    if (int rc = rows_args(who, block, N, C, idx, n, src)) return rc;
    if (n == 0 || N == 0) return DT_OK;
    if (rows_vec4(block, C, src)) {
        const int64_t total = n * (C / 4);
        hipLaunchKernelGGL((k_rows_put<uint4>), dim3(rows_grid(total)), dim3(256), 0, as_stream(stream), (uint4*)block, N,
                           (uint32_t)(C / 4), idx, (const uint4*)src, total);
    } else {
        const int64_t total = n * C;
        hipLaunchKernelGGL((k_rows_put<uint32_t>), dim3(rows_grid(total)), dim3(256), 0, as_stream(stream), (uint32_t*)block, N,
                           (uint32_t)C, idx, (const uint32_t*)src, total);
    }
    return launch_status(who);
}

extern "C" int dt_ensemble_mean(const void* const* parts_host, int K, int64_t total, int mode, void* out, void* stream) {
    const char* who = "dt_ensemble_mean";
    DT_REQUIRE(K >= 1 && K <= kMeanMaxParts, "%s: K=%d parts, 1 to %d are served", who, K, kMeanMaxParts);
    DT_REQUIRE(total >= 0, "%s: bad size total=%lld", who, (long long)total);
    DT_REQUIRE(mode == 0 || mode == 1, "%s: unknown mode %d (0: float64 mean, 1: float32 running mean)", who, mode);
    DT_REQUIRE(parts_host && out, "%s: null pointer", who);
    DT_REQUIRE(aligned_to(out, mode == 0 ? 8 : 4), "%s: misaligned out", who);
    MeanParts parts;
    for (int k = 0; k < kMeanMaxParts; ++k) parts.p[k] = nullptr;
    for (int k = 0; k < K; ++k) {
        DT_REQUIRE(parts_host[k], "%s: null pointer (part %d)", who, k);
        DT_REQUIRE(aligned_to(parts_host[k], 4), "%s: misaligned part %d", who, k);
        parts.p[k] = (const float*)parts_host[k];
    }
    if (total == 0) return DT_OK;
    if (mode == 0)
        hipLaunchKernelGGL((k_ensemble_mean<0>), dim3(rows_grid(total)), dim3(256), 0, as_stream(stream), parts, K, total, out);
    else
        hipLaunchKernelGGL((k_ensemble_mean<1>), dim3(rows_grid(total)), dim3(256), 0, as_stream(stream), parts, K, total, out);
    return launch_status(who);
}
