// emb_dropout.hip — the embedding gather with its SpatialDropout1D inside the launch (deeptables/models/layers.py:878-880,
// :900-902: one SpatialDropout1D per column on a [B, 1, D] slice, i.e. element dropout with 1 / (1 - rate) scaling), and the
// backward that re-applies the mask where the row gradients are produced (gfx950, wave64):
//
//   out[b, f, d]    = table[row(b, f), d] * keep(b, col_base[f] + d)                    dt_embedding_drop_fwd
//   values[r, d]    = g[r, d] * keep(b, col_base[f] + d)                                dt_embedding_drop_bwd, sparse
//   grad_table[row(b, f), d] += g[r, d] * keep(b, col_base[f] + d)                      dt_embedding_drop_bwd, dense
//
// keep is the cell hash (cell_hash.h): 0 or fl(1 / (1 - rate)) by hash(seed word, salt, row = b, col) >= threshold(rate), the
// column being the element's position in the concatenation of ALL of the layer's outputs — col_base[f] is where column f of
// this packed table starts there.  A layer with several packed tables (one per output width) therefore uses the slices of one
// layer-wide mask, ops.cell_dropout_keep(seed, salt, B, sum(output_dims), rate), whatever the grouping.  The seed word is read
// from DEVICE memory: a captured graph sees a fresh word at every replay, and the backward needs the rows and that word only.
//
// Geometry: 256 threads; a unit is one 16-byte vector of a looked-up row when D % 4 == 0 and the bases are 16-byte aligned
// (any lane count D / 4, a power of two or not), else one float; thread -> (lookup r, unit c) in a grid-stride loop of at
// most kMaxBlocks blocks, as the plain gather (k_gather_vec4).  head = hash(seed, salt) once per thread, the row word once per
// unit, one mix per element.  The dense backward always works on floats: consecutive lanes add to consecutive dwords, the
// shape k_scatter_add_rows gives the float atomics.  All index arithmetic is 32-bit: lookups * units < 2^31 is required.
#include "cell_hash.h"
#include "common.h"

namespace dt {
namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 256 * 16;          // the plain gather's cap

typedef float drop_f4 __attribute__((ext_vector_type(4)));

struct DropArgs {
    const unsigned* seed;      // device
    const int* col_base;       // device [F]
    unsigned salt, thr;
    float scale;               // fl(1 / (1 - rate))
};

// (lookup, unit, batch row, field) of flat unit t
struct DropPos {
    unsigned r, c, b, f;
    __device__ __forceinline__ DropPos(unsigned t, unsigned U, unsigned F) {
        r = t / U; c = t - r * U;
        b = r / F; f = r - b * F;
    }
};

__device__ __forceinline__ float drop_keep(const DropArgs& a, unsigned row_word, unsigned col) {
    return cell_hash_col(row_word, col) >= a.thr ? a.scale : 0.f;
}

// W = 4: U = D / 4 vectors per lookup; W = 1: U = D floats per lookup.  total = lookups * U < 2^31.
template <int KIND, int W>
__global__ __launch_bounds__(kThreads) void k_gather_drop(const void* __restrict__ idx, const float* __restrict__ table,
                                                          const int64_t* __restrict__ row_offset,
                                                          const int32_t* __restrict__ vocab, unsigned total, unsigned F,
                                                          unsigned U, DropArgs a, float* __restrict__ out,
                                                          int64_t* __restrict__ rows_out, int* __restrict__ oob_count) {
    const unsigned head = cell_hash_head(a.seed[0], a.salt);
    const unsigned stride = gridDim.x * kThreads;                       // <= 2^20: t + stride stays below 2^32
    for (unsigned t = blockIdx.x * kThreads + threadIdx.x; t < total; t += stride) {
        const DropPos p(t, U, F);
        const int id = load_id<KIND>(idx, p.r);
        const bool ok = (unsigned)id < (unsigned)vocab[p.f];
        const int64_t row = ok ? row_offset[p.f] + id : (int64_t)-1;
        const unsigned rw = cell_hash_row(head, p.b);
        const unsigned col = (unsigned)a.col_base[p.f] + p.c * W;
        if (W == 4) {
            drop_f4 v = {0.f, 0.f, 0.f, 0.f};
            if (ok) v = reinterpret_cast<const drop_f4*>(table)[row * U + p.c];
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] *= drop_keep(a, rw, col + j);
            reinterpret_cast<drop_f4*>(out)[t] = v;
        } else {
            const float v = ok ? table[row * U + p.c] : 0.f;
            out[t] = v * drop_keep(a, rw, col);
        }
        if (p.c == 0) {
            if (rows_out) rows_out[p.r] = row;
            if (!ok && oob_count) atomicAdd(oob_count, 1);
        }
    }
}

// DENSE (W = 1 only): dst = grad_table, rows < 0 skipped; else dst = values [lookups, D]
template <int W, bool DENSE>
__global__ __launch_bounds__(kThreads) void k_drop_bwd(const int64_t* __restrict__ rows, const float* __restrict__ g,
                                                       unsigned total, unsigned F, unsigned U, DropArgs a,
                                                       float* __restrict__ dst) {
    const unsigned head = cell_hash_head(a.seed[0], a.salt);
    const unsigned stride = gridDim.x * kThreads;
    for (unsigned t = blockIdx.x * kThreads + threadIdx.x; t < total; t += stride) {
        const DropPos p(t, U, F);
        const unsigned rw = cell_hash_row(head, p.b);
        const unsigned col = (unsigned)a.col_base[p.f] + p.c * W;
        if (DENSE) {
            const int64_t row = rows[p.r];
            if (row >= 0) atomicAdd(dst + row * U + p.c, g[t] * drop_keep(a, rw, col));
        } else if (W == 4) {
            drop_f4 v = reinterpret_cast<const drop_f4*>(g)[t];
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] *= drop_keep(a, rw, col + j);
            reinterpret_cast<drop_f4*>(dst)[t] = v;
        } else {
            dst[t] = g[t] * drop_keep(a, rw, col);
        }
    }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }

// the checks both entry points share; fills `a`
int drop_args(const char* what, int B, int F, int D, float rate, const int* seed, unsigned salt, const int* col_base,
              DropArgs* a) {
    DT_REQUIRE(B >= 0 && F >= 0 && D > 0, "%s: bad sizes B=%d F=%d D=%d", what, B, F, D);
    DT_REQUIRE(rate > 0.f && rate < 1.f, "%s: rate %g outside (0, 1): without a mask the plain gather serves", what, (double)rate);
    DT_REQUIRE((int64_t)B * F * D < ((int64_t)1 << 31), "%s: B F D = %lld is not below 2^31", what, (long long)B * F * D);
    if (B == 0 || F == 0) return DT_OK;
    DT_REQUIRE(seed && col_base, "%s: null seed word or col_base", what);
    DT_REQUIRE(aligned4(seed) && aligned4(col_base), "%s: misaligned pointer", what);
    a->seed = reinterpret_cast<const unsigned*>(seed);
    a->col_base = col_base;
    a->salt = salt;
    a->thr = cell_threshold(rate);
    a->scale = 1.f / (1.f - rate);
    return DT_OK;
}

inline unsigned drop_blocks(unsigned total) {
    const unsigned want = (total + kThreads - 1) / kThreads;
    return want < (unsigned)kMaxBlocks ? want : (unsigned)kMaxBlocks;
}

}  // namespace
}  // namespace dt

using namespace dt;

extern "C" int64_t dt_embedding_drop_pass_units(void) { return (int64_t)kMaxBlocks * kThreads; }

extern "C" int dt_embedding_drop_fwd(const void* idx, int idx_kind, const float* table, const int64_t* row_offset,
                                     const int32_t* vocab, int B, int F, int D, float rate, const int* seed, unsigned salt,
                                     const int* col_base, float* out, int64_t* rows_out, int* oob_count, void* stream) {
    DropArgs a;
    const int rc = drop_args("dt_embedding_drop_fwd", B, F, D, rate, seed, salt, col_base, &a);
    if (rc != DT_OK) return rc;
    DT_REQUIRE(idx_kind == DT_IDX_F32 || idx_kind == DT_IDX_I32, "dt_embedding_drop_fwd: idx_kind %d", idx_kind);
    if (B == 0 || F == 0) return DT_OK;
    DT_REQUIRE(idx && table && row_offset && vocab && out, "dt_embedding_drop_fwd: null pointer");
    DT_REQUIRE(aligned4(idx) && aligned4(table) && aligned4(out), "dt_embedding_drop_fwd: misaligned pointer");
    const bool vec = D % 4 == 0 && aligned16(table) && aligned16(out);
    const unsigned U = vec ? D / 4 : D, total = (unsigned)B * F * U;
    const dim3 grid(drop_blocks(total)), block(kThreads);
    hipStream_t st = as_stream(stream);
#define DT_DROP_FWD(KIND, W)                                                                                               \
    hipLaunchKernelGGL((k_gather_drop<KIND, W>), grid, block, 0, st, idx, table, row_offset, vocab, total, (unsigned)F, U, a, \
                       out, rows_out, oob_count)
    if (idx_kind == DT_IDX_F32) {
        if (vec) DT_DROP_FWD(DT_IDX_F32, 4); else DT_DROP_FWD(DT_IDX_F32, 1);
    } else {
        if (vec) DT_DROP_FWD(DT_IDX_I32, 4); else DT_DROP_FWD(DT_IDX_I32, 1);
    }
#undef DT_DROP_FWD
    return launch_status("dt_embedding_drop_fwd");
}

extern "C" int dt_embedding_drop_bwd(const int64_t* rows, const float* grad_out, int B, int F, int D, float rate,
                                     const int* seed, unsigned salt, const int* col_base, float* values, float* grad_table,
                                     void* stream) {
    DropArgs a;
    const int rc = drop_args("dt_embedding_drop_bwd", B, F, D, rate, seed, salt, col_base, &a);
    if (rc != DT_OK) return rc;
    DT_REQUIRE((values != nullptr) != (grad_table != nullptr),
               "dt_embedding_drop_bwd: exactly one of values (sparse mode) and grad_table (dense mode) is given");
    if (B == 0 || F == 0) return DT_OK;
    DT_REQUIRE(grad_out && (values || rows), "dt_embedding_drop_bwd: null pointer");
    DT_REQUIRE(aligned4(grad_out) && aligned4(values) && aligned4(grad_table) && (reinterpret_cast<uintptr_t>(rows) & 7) == 0,
               "dt_embedding_drop_bwd: misaligned pointer");
    hipStream_t st = as_stream(stream);
    const bool vec = !grad_table && D % 4 == 0 && aligned16(grad_out) && aligned16(values);
    const unsigned U = vec ? D / 4 : D, total = (unsigned)B * F * U;
    const dim3 grid(drop_blocks(total)), block(kThreads);
    if (grad_table)
        hipLaunchKernelGGL((k_drop_bwd<1, true>), grid, block, 0, st, rows, grad_out, total, (unsigned)F, U, a, grad_table);
    else if (vec)
        hipLaunchKernelGGL((k_drop_bwd<4, false>), grid, block, 0, st, rows, grad_out, total, (unsigned)F, U, a, values);
    else
        hipLaunchKernelGGL((k_drop_bwd<1, false>), grid, block, 0, st, rows, grad_out, total, (unsigned)F, U, a, values);
    return launch_status("dt_embedding_drop_bwd");
}
