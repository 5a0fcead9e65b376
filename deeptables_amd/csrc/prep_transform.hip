// prep_transform.hip — the fitted preprocessor's transform on the device: raw frame columns in, one block of a resident feed out
// (models/preprocessor.py: DefaultPreprocessor.transform_feed; ops.prep_transform).
//
// Sources are column-major: one contiguous array per raw column, each in its own dtype (bool, int8..64, uint8..64, float32,
// float64).  The output is ONE row-major [N, C] block of 4-byte words (int32 ids or float32 values).  Column j of the block is
// described by cols[j] (dt_prep_col, include/dt_hip.h) and is one of
//     LOOKUP  key = the raw value widened to 64 bits (ints sign-extended, uints and bool zero-extended, float32 bits
//             zero-extended, float64 bits, every NaN the canonical quiet NaN); the id of the key in (keys ascending, ids), or
//             `miss` when the key is not in the table.                             MultiLabelEncoder on a numeric column
//     CONT    v = (double)x; IMPUTE and v is NaN: v = fill; SCALE: v = (v - min) / range, both correctly rounded in float64;
//             the word is (float)v.                                                 ColumnImputer, MinMaxScalerTransformer
//     BIN     v as CONT before its last cast; the number of edges <= v, n_edges for a NaN.     np.searchsorted(side='right')
//     COPY    the low 32 bits of an integer source.                                `.astype(int64)` then `.to(int32)`
// Every operation is integer or correctly rounded IEEE float64 arithmetic on one element: no atomics, no reductions, the same
// bits on every run and the bits of the host path.
//
// The shape of the work is a transpose.  A block of 256 threads takes a tile of kPrepTileRows = 256 rows.  For each output column
// of a chunk of kPrepChunkCols = 32 columns, thread t reads row t of the source (adjacent lanes, adjacent elements: coalesced),
// computes its word and stores it at tile[t][j].  A tile row is 33 words, so the 64 lanes of a wave, 33 words apart, fall on 64
// different LDS banks (64 banks of 4 bytes; 33 is odd).  After a barrier the chunk's words leave in output order: a tile whose
// chunk covers whole rows (C <= 32) is ONE contiguous run of rows * C words, otherwise every row contributes a contiguous run
// of the chunk's width.  Where the run lengths and the pointer allow it (C % 4 == 0, out 16-byte aligned; chunk starts are
// multiples of 32) a thread stores a uint4 — four words of one row — otherwise single words.  Tiles are taken in a grid-stride
// loop under kPrepMaxBlocks blocks, rows are 64-bit.  The table search is a fixed-trip binary search: the trip count is the bit
// length of n_keys, uniform over the block, lanes differ only in the data they compare.  Keys, ids and edges are read from
// global memory (L2 holds a table of any realistic size; the upper levels of the search are shared by every lane).
// The descriptors come twice: a host copy, which the entry validates, and the device copy the kernel reads.  The kernel never
// trusts a field for control flow it cannot survive: an unknown dtype or op gives a zero word, negative or null tables are empty.
#include "common.h"
#include "optim_dev.h"

namespace dt {

constexpr int kPrepThreads = 256;
constexpr int kPrepTileRows = DT_PREP_TILE_ROWS;        // one row per thread and column
constexpr int kPrepChunkCols = DT_PREP_CHUNK_COLS;
constexpr int kPrepTilePitch = kPrepChunkCols + 1;      // odd: lanes a row apart hit different banks
constexpr int kPrepMaxBlocks = DT_PREP_MAX_BLOCKS;      // 256 CUs x 4 resident blocks (33 KiB of LDS each)
static_assert(kPrepTileRows == kPrepThreads, "one thread per tile row");
static_assert(sizeof(dt_prep_col) == DT_PREP_COL_BYTES, "ops.py packs the descriptor by this layout");
static_assert(kPrepChunkCols % 4 == 0, "chunk starts must keep the 16-byte alignment of a row");

constexpr uint64_t kNanKey32 = 0x7FC00000ull, kNanKey64 = 0x7FF8000000000000ull;

// the raw element as the 64-bit LOOKUP key
__device__ __forceinline__ uint64_t prep_key(const void* src, int dtype, int64_t i) {
    switch (dtype) {
        case DT_PREP_BOOL: return (uint64_t)(((const uint8_t*)src)[i] != 0);
        case DT_PREP_I8: return (uint64_t)(int64_t)((const int8_t*)src)[i];
        case DT_PREP_I16: return (uint64_t)(int64_t)((const int16_t*)src)[i];
        case DT_PREP_I32: return (uint64_t)(int64_t)((const int32_t*)src)[i];
        case DT_PREP_I64: return (uint64_t)((const int64_t*)src)[i];
        case DT_PREP_U8: return (uint64_t)((const uint8_t*)src)[i];
        case DT_PREP_U16: return (uint64_t)((const uint16_t*)src)[i];
        case DT_PREP_U32: return (uint64_t)((const uint32_t*)src)[i];
        case DT_PREP_U64: return ((const uint64_t*)src)[i];
        case DT_PREP_F32: {
            const uint32_t b = ((const uint32_t*)src)[i];
            return (b & 0x7FFFFFFFu) > 0x7F800000u ? kNanKey32 : (uint64_t)b;
        }
        case DT_PREP_F64: {
            const uint64_t b = ((const uint64_t*)src)[i];
            return (b & 0x7FFFFFFFFFFFFFFFull) > 0x7FF0000000000000ull ? kNanKey64 : b;
        }
        default: return 0;
    }
}

// the raw element as a double (ints: one correctly rounded conversion; float32: exact)
__device__ __forceinline__ double prep_value(const void* src, int dtype, int64_t i) {
    switch (dtype) {
        case DT_PREP_BOOL: return ((const uint8_t*)src)[i] != 0 ? 1.0 : 0.0;
        case DT_PREP_I8: return (double)((const int8_t*)src)[i];
        case DT_PREP_I16: return (double)((const int16_t*)src)[i];
        case DT_PREP_I32: return (double)((const int32_t*)src)[i];
        case DT_PREP_I64: return __ll2double_rn(((const int64_t*)src)[i]);
        case DT_PREP_U8: return (double)((const uint8_t*)src)[i];
        case DT_PREP_U16: return (double)((const uint16_t*)src)[i];
        case DT_PREP_U32: return (double)((const uint32_t*)src)[i];
        case DT_PREP_U64: return __ull2double_rn(((const uint64_t*)src)[i]);
        case DT_PREP_F32: return (double)((const float*)src)[i];
        case DT_PREP_F64: return ((const double*)src)[i];
        default: return 0.0;
    }
}

__device__ __forceinline__ double prep_scaled(const dt_prep_col& c, int64_t i) {
    double v = prep_value(c.src, c.dtype, i);
    if ((c.flags & DT_PREP_IMPUTE) && v != v) v = c.fill;
    if (c.flags & DT_PREP_SCALE) v = __ddiv_rn(__dsub_rn(v, c.min), c.range);
    return v;
}

// how many of the n ascending entries are <= x: `trips` = bit length of n halvings, the same for every lane
template <typename T>
__device__ __forceinline__ int count_le(const T* __restrict__ a, int n, int trips, T x) {
    int lo = 0;
    for (int t = trips - 1; t >= 0; --t) {
        const int probe = lo + (1 << t);
        if (probe <= n && a[probe - 1] <= x) lo = probe;
    }
    return lo;
}

__device__ __forceinline__ int bit_length(int n) { return n > 0 ? 32 - __clz(n) : 0; }

__device__ __forceinline__ uint32_t prep_word(const dt_prep_col& c, int64_t i) {
    if (!c.src || c.dtype < 0 || c.dtype >= DT_PREP_DTYPE_COUNT) return 0u;
    switch (c.op) {
        case DT_PREP_LOOKUP: {
            const int n = (c.keys && c.ids && c.n_keys > 0) ? c.n_keys : 0;
            const uint64_t k = prep_key(c.src, c.dtype, i);
            const int le = count_le<uint64_t>(c.keys, n, bit_length(n), k);
            return (uint32_t)((le > 0 && c.keys[le - 1] == k) ? c.ids[le - 1] : c.miss);
        }
        case DT_PREP_CONT: return __float_as_uint(__double2float_rn(prep_scaled(c, i)));
        case DT_PREP_BIN: {
            const int n = (c.edges && c.n_edges > 0) ? c.n_edges : 0;
            const double v = prep_scaled(c, i);
            return (uint32_t)(v != v ? n : count_le<double>(c.edges, n, bit_length(n), v));
        }
        case DT_PREP_COPY: return c.dtype <= DT_PREP_U64 ? (uint32_t)prep_key(c.src, c.dtype, i) : 0u;
        default: return 0u;
    }
}

// VEC: uint4 stores (C % 4 == 0 and out 16-byte aligned)
template <bool VEC>
__global__ __launch_bounds__(kPrepThreads) void k_prep_transform(int64_t N, const dt_prep_col* __restrict__ cols, int C,
                                                                  uint32_t* __restrict__ out) {
    __shared__ uint32_t tile[kPrepTileRows * kPrepTilePitch];
    const int t = threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * kPrepTileRows;
    for (int64_t r0 = (int64_t)blockIdx.x * kPrepTileRows; r0 < N; r0 += stride) {
        const int rows = (int)(N - r0 < kPrepTileRows ? N - r0 : kPrepTileRows);
        for (int c0 = 0; c0 < C; c0 += kPrepChunkCols) {
            const int cw = C - c0 < kPrepChunkCols ? C - c0 : kPrepChunkCols;
            if (t < rows)
                for (int j = 0; j < cw; ++j) tile[t * kPrepTilePitch + j] = prep_word(cols[c0 + j], r0 + t);
            __syncthreads();
            // the chunk's words in output order: row r, columns c0 .. c0 + cw - 1 at out[(r0 + r) * C + c0 ...]
            uint32_t* dst = out + r0 * C + c0;
            if (VEC) {
                const int q = cw / 4, total = rows * q;
                for (int e = t; e < total; e += kPrepThreads) {
                    const int r = e / q, w = (e - r * q) * 4;
                    const uint32_t* s = tile + r * kPrepTilePitch + w;
                    *(uint4*)(dst + (int64_t)r * C + w) = make_uint4(s[0], s[1], s[2], s[3]);
                }
            } else {
                const int total = rows * cw;
                for (int e = t; e < total; e += kPrepThreads) {
                    const int r = e / cw, w = e - r * cw;
                    dst[(int64_t)r * C + w] = tile[r * kPrepTilePitch + w];
                }
            }
            __syncthreads();
        }
    }
}

}  // namespace dt

using namespace dt;

extern "C" int dt_prep_transform(int64_t N, const dt_prep_col* cols, const dt_prep_col* cols_host, int C, int out_kind, void* out,
                                 void* stream) {
    const char* who = "dt_prep_transform";
    DT_REQUIRE(N >= 0 && C >= 1, "%s: bad sizes N=%lld C=%d", who, (long long)N, C);
    DT_REQUIRE(N <= INT64_MAX / 4 / C, "%s: N=%lld x C=%d words overflow", who, (long long)N, C);
    DT_REQUIRE(out_kind == DT_PREP_OUT_I32 || out_kind == DT_PREP_OUT_F32, "%s: unknown out_kind %d (0: int32, 1: float32)", who,
               out_kind);
    DT_REQUIRE(cols && cols_host && out, "%s: null pointer", who);
    DT_REQUIRE(aligned_to(cols, 8) && aligned_to(cols_host, 8), "%s: misaligned descriptors", who);
    DT_REQUIRE(aligned_to(out, 4), "%s: misaligned out", who);
    static const int width[DT_PREP_DTYPE_COUNT] = {1, 1, 2, 4, 8, 1, 2, 4, 8, 4, 8};
    for (int j = 0; j < C; ++j) {
        const dt_prep_col& c = cols_host[j];
        DT_REQUIRE(c.dtype >= 0 && c.dtype < DT_PREP_DTYPE_COUNT, "%s: column %d: unknown dtype code %d", who, j, c.dtype);
        DT_REQUIRE(c.op >= DT_PREP_LOOKUP && c.op <= DT_PREP_COPY, "%s: column %d: unknown op code %d", who, j, c.op);
        DT_REQUIRE(out_kind == DT_PREP_OUT_F32 ? c.op == DT_PREP_CONT : c.op != DT_PREP_CONT,
                   "%s: column %d: op %d does not write a%s block", who, j, c.op, out_kind == DT_PREP_OUT_F32 ? " float32" : "n int32");
        DT_REQUIRE(c.op != DT_PREP_COPY || c.dtype <= DT_PREP_U64, "%s: column %d: COPY of a float source", who, j);
        DT_REQUIRE((c.flags & ~(DT_PREP_IMPUTE | DT_PREP_SCALE)) == 0, "%s: column %d: unknown flags 0x%x", who, j, c.flags);
        DT_REQUIRE(c.n_keys >= 0 && c.n_edges >= 0, "%s: column %d: n_keys=%d n_edges=%d", who, j, c.n_keys, c.n_edges);
        DT_REQUIRE(c.src || N == 0, "%s: column %d: null source", who, j);
        DT_REQUIRE(aligned_to(c.src, width[c.dtype]), "%s: column %d: misaligned source", who, j);
        if (c.op == DT_PREP_LOOKUP && c.n_keys > 0) {
            DT_REQUIRE(c.keys && c.ids, "%s: column %d: null table", who, j);
            DT_REQUIRE(aligned_to(c.keys, 8) && aligned_to(c.ids, 4), "%s: column %d: misaligned table", who, j);
        }
        if (c.op == DT_PREP_BIN && c.n_edges > 0) {
            DT_REQUIRE(c.edges, "%s: column %d: null edges", who, j);
            DT_REQUIRE(aligned_to(c.edges, 8), "%s: column %d: misaligned edges", who, j);
        }
    }
    if (N == 0) return DT_OK;
    const int64_t tiles = (N + kPrepTileRows - 1) / kPrepTileRows;
    const unsigned grid = (unsigned)(tiles < kPrepMaxBlocks ? tiles : kPrepMaxBlocks);
    if (C % 4 == 0 && aligned_to(out, 16))
        hipLaunchKernelGGL((k_prep_transform<true>), dim3(grid), dim3(kPrepThreads), 0, as_stream(stream), N, cols, C, (uint32_t*)out);
    else
        hipLaunchKernelGGL((k_prep_transform<false>), dim3(grid), dim3(kPrepThreads), 0, as_stream(stream), N, cols, C,
                           (uint32_t*)out);
    return launch_status(who);
}
