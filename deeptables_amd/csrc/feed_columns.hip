// feed_columns.hip — permute columns of a device-resident feed block in place (utils/feature_importance.py, ops.permute_columns).
//
// A feed block is a row-major [N, C] array of 4-byte words (int32 ids or float32 values).  Permutation importance shuffles the
// rows of `width` adjacent columns, scores, and puts the original values back:
//     dt_column_gather   out[i, w] = block[perm[i], col0 + w]          (block is only read)
//     dt_column_swap     block[i, col0 + w] <-> buf[i, w]               (every word is read and written by ONE thread)
// gather into buf, then swap: the block holds the permuted columns and buf the originals; the same swap again restores the
// block bit for bit.  In two launches no thread reads a row another thread is overwriting.  Words are moved, never
// interpreted: NaN payloads, -0.0 and denormals survive.
//
// Launch: 256-thread blocks, one thread per word of [N, width] (width == 1: one thread per row; wider: the threads of a row are
// adjacent, so its `width` contiguous words leave in one request), a grid-stride loop under kColumnMaxBlocks blocks, 64-bit
// element indices (N C exceeds 2^31 at bench size).  perm, out and buf are read / written in thread order.  Where col0, width
// and C are multiples of 4 and the pointers 16-byte aligned the word is a uint4 (T = uint4, every count divided by 4).
// A perm entry outside [0, N) is a caller error that must not become a fault: that thread reads its own row instead.
#include "common.h"
#include "optim_dev.h"

namespace dt {

constexpr int kColumnMaxBlocks = 2048;      // 256 CUs x 8 resident blocks of 256 threads; the kernels stride over the rest

// total = N * width elements of T; ONE: width == 1 (no division)
template <typename T, bool ONE>
__global__ __launch_bounds__(256) void k_column_gather(const T* __restrict__ block, int64_t N, int64_t C, int64_t col0,
                                                        int64_t width, const int64_t* __restrict__ perm,
                                                        T* __restrict__ out, int64_t total) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += stride) {
        const int64_t i = ONE ? e : e / width;
        const int64_t w = ONE ? 0 : e - i * width;
        int64_t p = perm[i];
        if (p < 0 || p >= N) p = i;
        out[e] = block[p * C + col0 + w];
    }
}

template <typename T, bool ONE>
__global__ __launch_bounds__(256) void k_column_swap(T* __restrict__ block, int64_t C, int64_t col0, int64_t width,
                                                      T* __restrict__ buf, int64_t total) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += stride) {
        const int64_t i = ONE ? e : e / width;
        const int64_t w = ONE ? 0 : e - i * width;
        T* at = block + i * C + col0 + w;
        const T mine = *at, theirs = buf[e];
        *at = theirs;
        buf[e] = mine;
    }
}

static int column_args(const char* who, const void* block, int64_t N, int C, int col0, int width, const void* other) {
    DT_REQUIRE(N >= 0 && C >= 1 && width >= 1 && col0 >= 0, "%s: bad sizes N=%lld C=%d col0=%d width=%d", who, (long long)N, C,
               col0, width);
    DT_REQUIRE((int64_t)col0 + width <= C, "%s: columns [%d, %lld) of a block with %d", who, col0, (long long)col0 + width, C);
    DT_REQUIRE(block && other, "%s: null pointer", who);
    DT_REQUIRE(aligned_to(block, 4) && aligned_to(other, 4), "%s: misaligned pointer", who);
    return DT_OK;
}

inline bool column_vec4(const void* block, int C, int col0, int width, const void* other) {
    return C % 4 == 0 && col0 % 4 == 0 && width % 4 == 0 && aligned_to(block, 16) && aligned_to(other, 16);
}

inline unsigned column_grid(int64_t total) {
    const int64_t blocks = (total + 255) / 256;
    return (unsigned)(blocks < kColumnMaxBlocks ? blocks : kColumnMaxBlocks);
}

}  // namespace dt

using namespace dt;

extern "C" int dt_column_gather(const void* block, int64_t N, int C, int col0, int width, const int64_t* perm, void* out,
                                void* stream) {
    const char* who = "dt_column_gather";
    if (int rc = column_args(who, block, N, C, col0, width, out)) return rc;
    DT_REQUIRE(perm, "%s: null pointer", who);
    DT_REQUIRE(aligned_to(perm, 8), "%s: misaligned perm", who);
    if (N == 0) return DT_OK;
    if (column_vec4(block, C, col0, width, out)) {
        const int64_t w4 = width / 4, total = N * w4;
        if (w4 == 1)
            hipLaunchKernelGGL((k_column_gather<uint4, true>), dim3(column_grid(total)), dim3(256), 0, as_stream(stream),
                               (const uint4*)block, N, (int64_t)(C / 4), (int64_t)(col0 / 4), w4, perm, (uint4*)out, total);
        else
            hipLaunchKernelGGL((k_column_gather<uint4, false>), dim3(column_grid(total)), dim3(256), 0, as_stream(stream),
                               (const uint4*)block, N, (int64_t)(C / 4), (int64_t)(col0 / 4), w4, perm, (uint4*)out, total);
    } else {
        const int64_t total = N * width;
        if (width == 1)
            hipLaunchKernelGGL((k_column_gather<uint32_t, true>), dim3(column_grid(total)), dim3(256), 0, as_stream(stream),
                               (const uint32_t*)block, N, (int64_t)C, (int64_t)col0, (int64_t)width, perm, (uint32_t*)out,
                               total);
        else
            hipLaunchKernelGGL((k_column_gather<uint32_t, false>), dim3(column_grid(total)), dim3(256), 0, as_stream(stream),
                               (const uint32_t*)block, N, (int64_t)C, (int64_t)col0, (int64_t)width, perm, (uint32_t*)out,
                               total);
    }
    return launch_status(who);
}

extern "C" int dt_column_swap(void* block, int64_t N, int C, int col0, int width, void* buf, void* stream) {
    const char* who = "dt_column_swap";
    if (int rc = column_args(who, block, N, C, col0, width, buf)) return rc;
    if (N == 0) return DT_OK;
    if (column_vec4(block, C, col0, width, buf)) {
        const int64_t w4 = width / 4, total = N * w4;
        if (w4 == 1)
            hipLaunchKernelGGL((k_column_swap<uint4, true>), dim3(column_grid(total)), dim3(256), 0, as_stream(stream),
                               (uint4*)block, (int64_t)(C / 4), (int64_t)(col0 / 4), w4, (uint4*)buf, total);
        else
            hipLaunchKernelGGL((k_column_swap<uint4, false>), dim3(column_grid(total)), dim3(256), 0, as_stream(stream),
                               (uint4*)block, (int64_t)(C / 4), (int64_t)(col0 / 4), w4, (uint4*)buf, total);
    } else {
        const int64_t total = N * width;
        if (width == 1)
            hipLaunchKernelGGL((k_column_swap<uint32_t, true>), dim3(column_grid(total)), dim3(256), 0, as_stream(stream),
                               (uint32_t*)block, (int64_t)C, (int64_t)col0, (int64_t)width, (uint32_t*)buf, total);
        else
            hipLaunchKernelGGL((k_column_swap<uint32_t, false>), dim3(column_grid(total)), dim3(256), 0, as_stream(stream),
                               (uint32_t*)block, (int64_t)C, (int64_t)col0, (int64_t)width, (uint32_t*)buf, total);
    }
    return launch_status(who);
}
