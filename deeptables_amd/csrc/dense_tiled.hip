// dense_tiled.hip — Keras `Dense` forward/backward for the shapes dense.hip refuses (its [rows x K] LDS slab stops at
// 150 KB): the first Dense of FiBiNet's tower (deepnets.py:374-386, K = 10,413), FGCNN's recombination Dense
// (layers.py:161-242, 2,912 -> 832 and 1,792 -> 416), FGCNN's tower (deepnets.py:401-427, K = 1,677) and any user tower
// with a wide first layer.  One kernel, k_dense_tiled, whose tiles depend on neither K nor M, computes all three products
// on v_mfma_f32_32x32x2_f32 (exact fp32: an fmaf chain over the contraction index, the instruction dense.hip uses):
//   forward  y  [N,M]  = act(x W + bias)         A = x  (contraction-contiguous), B = W (column-contiguous)
//   grad_x      [N,K]  = G W^T                   A = G  (contraction-contiguous, masked), B = W read transposed by the
//                                                staging loads (contraction-contiguous): no transpose pass, no workspace
//   grad_W      [K,M] += x^T G, grad_b += colsum(G)   A = x, B = G (both row-contiguous along the output index, G masked);
//                                                the batch is split over blockIdx.z when K x M alone gives too few
//                                                blocks, partial tiles merged with float atomics
// with G = grad_y * act'(y) formed while grad_y is staged.
//
// Block = 256 threads = 2 x 2 waves.  Output tile 128 x 128 (each wave 2 x 2 MFMA tiles of 32 x 32) when that alone
// gives >= 256 blocks, else 64 x 64 (one MFMA tile per wave) so that short-and-wide outputs still fill the 256 CUs.  The
// contraction is walked in steps of 32: both operand panels are staged as [32][tile (+1)] floats in LDS, double
// buffered (the next step's global loads are issued before this step's MFMAs and written to the other buffer after them:
// one barrier per step).  A panel whose source is contraction-contiguous is transposed on the way in (row stride
// tile + 1: the transposing ds_write_b32 and the operand ds_read_b32 are both bank-conflict free); 16-byte global loads
// are used only when the source's row length is a multiple of 4 and its base 16-byte aligned.
//   LDS per block:   2 buffers x 2 panels x 32 x 129 x 4 B = 66,048 B (128 x 128);  33,280 B (64 x 64): constants,
//                    independent of K and M; two blocks per CU either way.
//   registers:       128 x 128: 64 accumulators (AGPRs) + 48 staging (16 A, 16 B, 16 y of the masked operand) + operands and
//                    addresses = 126 .. 166 VGPRs + 64 AGPRs <= 256: two waves per SIMD;  64 x 64: 16 accumulators + 24
//                    staging = 80 .. 96 VGPRs + 16 AGPRs.  No spills.
// Edges (N / K / M not multiples of the tile): loads go unconditionally to a clamped address and the value is zeroed
// when it is written to LDS; stores are guarded.  Element offsets are 64-bit (N K > 2^31 at 212,992 x 10,413).
#include "common.h"

namespace dt {
namespace {

typedef float tl_f16 __attribute__((ext_vector_type(16)));
typedef float tl_f4 __attribute__((ext_vector_type(4)));
constexpr int kTK = 32;   // contraction indices per step (16 MFMAs per 32 x 32 tile)

__device__ __forceinline__ float tl_dact(float g, float y, int act) {
    return (act == DT_ACT_RELU && !(y > 0.f)) ? 0.f : g;
}

// One operand panel of one contraction step: [kTK][BR] values, BR = the tile's extent along the output index.
//   KC  = true : source is contraction-contiguous, src[(r0 + r) * ld + k]  -> transposed into panel[k][r], LD = BR + 1
//   KC  = false: source is output-contiguous,      src[k * ld + r0 + r]     -> copied into     panel[k][r], LD = BR
// load() only issues the global loads (clamped addresses); store() zeroes what lies outside [0, R) x [., kend), applies
// the relu mask and writes LDS, so the loads stay in flight across the MFMAs between the two.
template <bool KC, int BR>
struct Panel {
    static constexpr int NV = BR / 8;            // floats per thread per step
    static constexpr int LD = KC ? BR + 1 : BR;
    static constexpr int Q = BR / 4;             // 16-byte groups per panel row (KC = false)

    static __device__ __forceinline__ void load(const float* __restrict__ src, int64_t ld, int r0, int R, int k0, int Kc,
                                                bool vec, float (&v)[NV]) {
        const int tid = threadIdx.x;
        if (KC) {
            if (vec) {
                const int kc = min(k0 + 4 * (tid & 7), Kc - 4);
#pragma unroll
                for (int e = 0; e < NV / 4; ++e) {
                    const int row = min(r0 + (tid >> 3) + 32 * e, R - 1);
                    const tl_f4 q = *reinterpret_cast<const tl_f4*>(src + (int64_t)row * ld + kc);
                    v[4 * e] = q.x; v[4 * e + 1] = q.y; v[4 * e + 2] = q.z; v[4 * e + 3] = q.w;
                }
            } else {
                const int kc = min(k0 + (tid & 31), Kc - 1);
#pragma unroll
                for (int e = 0; e < NV; ++e) {
                    const int row = min(r0 + (tid >> 5) + 8 * e, R - 1);
                    v[e] = src[(int64_t)row * ld + kc];
                }
            }
        } else {
            if (vec) {
                const int col = min(r0 + 4 * (tid % Q), R - 4);
#pragma unroll
                for (int e = 0; e < NV / 4; ++e) {
                    const int k = min(k0 + tid / Q + (256 / Q) * e, Kc - 1);
                    const tl_f4 q = *reinterpret_cast<const tl_f4*>(src + (int64_t)k * ld + col);
                    v[4 * e] = q.x; v[4 * e + 1] = q.y; v[4 * e + 2] = q.z; v[4 * e + 3] = q.w;
                }
            } else {
                const int col = min(r0 + tid % BR, R - 1);
#pragma unroll
                for (int e = 0; e < NV; ++e) {
                    const int k = min(k0 + tid / BR + (256 / BR) * e, Kc - 1);
                    v[e] = src[(int64_t)k * ld + col];
                }
            }
        }
    }

    template <bool MASKED>
    static __device__ __forceinline__ void store(float* __restrict__ panel, int r0, int R, int k0, int kend, bool vec,
                                                 const float (&v)[NV], const float (&y)[NV], int mask_act) {
        const int tid = threadIdx.x;
        if (KC) {
            if (vec) {
                const int kk = 4 * (tid & 7);
                const bool kok = k0 + kk < kend;      // kend and k0 are multiples of 4 here: the four share one answer
#pragma unroll
                for (int e = 0; e < NV / 4; ++e) {
                    const int rl = (tid >> 3) + 32 * e;
                    const bool ok = kok && r0 + rl < R;
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        float val = v[4 * e + c];
                        if (MASKED) val = tl_dact(val, y[4 * e + c], mask_act);
                        panel[(kk + c) * LD + rl] = ok ? val : 0.f;
                    }
                }
            } else {
                const int kk = tid & 31;
                const bool kok = k0 + kk < kend;
#pragma unroll
                for (int e = 0; e < NV; ++e) {
                    const int rl = (tid >> 5) + 8 * e;
                    float val = v[e];
                    if (MASKED) val = tl_dact(val, y[e], mask_act);
                    panel[kk * LD + rl] = (kok && r0 + rl < R) ? val : 0.f;
                }
            }
        } else {
            if (vec) {
                const int cl = 4 * (tid % Q);
                const bool cok = r0 + cl < R;         // R is a multiple of 4 here
#pragma unroll
                for (int e = 0; e < NV / 4; ++e) {
                    const int kk = tid / Q + (256 / Q) * e;
                    const bool ok = cok && k0 + kk < kend;
                    tl_f4 q;
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        float val = v[4 * e + c];
                        if (MASKED) val = tl_dact(val, y[4 * e + c], mask_act);
                        q[c] = ok ? val : 0.f;
                    }
                    *reinterpret_cast<tl_f4*>(panel + kk * LD + cl) = q;
                }
            } else {
                const int cl = tid % BR;
                const bool cok = r0 + cl < R;
#pragma unroll
                for (int e = 0; e < NV; ++e) {
                    const int kk = tid / BR + (256 / BR) * e;
                    float val = v[e];
                    if (MASKED) val = tl_dact(val, y[e], mask_act);
                    panel[kk * LD + cl] = (cok && k0 + kk < kend) ? val : 0.f;
                }
            }
        }
    }
};

// ---------------------------------------------------------------------------------------------------------------------
// C[R, Cc] (=|+=) A[R, Kc] . B[Kc, Cc]      grid (row tiles, column tiles, contraction splits)
//   AKC / BKC : the operand's source is contraction-contiguous (see Panel)
//   MASK      : 0 none, 1 A = A * act'(Y), 2 B = B * act'(Y); Y has the masked operand's layout
//   ACC       : false: C = act(A B + bias);  true: C += A B (plain when `atomic` == 0, float atomics otherwise) and
//               gb[col] += column sums of B, from the blocks of row tile 0
//   WT        : MFMA tiles per wave in each direction (block tile = 64 WT x 64 WT)
// ---------------------------------------------------------------------------------------------------------------------
template <bool AKC, bool BKC, int MASK, bool ACC, int WT>
__global__ __launch_bounds__(256) void k_dense_tiled(const float* __restrict__ A, int64_t lda,
                                                     const float* __restrict__ B, int64_t ldb,
                                                     const float* __restrict__ Y, int mask_act,
                                                     const float* __restrict__ bias, int act, int R, int Cc, int Kc,
                                                     int steps_per_split, int vecA, int vecB, float* __restrict__ C,
                                                     int64_t ldc, float* __restrict__ gb, int atomic) {
    constexpr int BT = 64 * WT;
    using PA = Panel<AKC, BT>;
    using PB = Panel<BKC, BT>;
    constexpr int NV = PA::NV;
    constexpr int PSZ = kTK * (BT + 1);          // floats per panel slot (a multiple of 4: slots stay 16-byte aligned)
    extern __shared__ __attribute__((aligned(16))) float tl_lds[];   // [2 buffers][A panel | B panel]

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int s = lane >> 5, c = lane & 31;
    const int wr = wave >> 1, wc = wave & 1;
    const int r0 = blockIdx.x * BT, c0 = blockIdx.y * BT;
    const int kbeg = blockIdx.z * steps_per_split * kTK;
    const int kend = min(Kc, kbeg + steps_per_split * kTK);
    const int steps = (kend - kbeg + kTK - 1) / kTK;
    const bool va4 = vecA != 0, vb4 = vecB != 0;
    const bool use_y = MASK != 0 && mask_act == DT_ACT_RELU;
    const bool want_b = ACC && gb != nullptr && blockIdx.x == 0 && wr == 0;

    tl_f16 acc[WT][WT];
#pragma unroll
    for (int i = 0; i < WT; ++i)
#pragma unroll
        for (int j = 0; j < WT; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    float bsum[WT];
#pragma unroll
    for (int j = 0; j < WT; ++j) bsum[j] = 0.f;

    float va[NV], vb[NV], vy[NV];
#pragma unroll
    for (int e = 0; e < NV; ++e) vy[e] = 1.f;

    PA::load(A, lda, r0, R, kbeg, Kc, va4, va);
    PB::load(B, ldb, c0, Cc, kbeg, Kc, vb4, vb);
    if (use_y) {
        if (MASK == 1) PA::load(Y, lda, r0, R, kbeg, Kc, va4, vy);
        else PB::load(Y, ldb, c0, Cc, kbeg, Kc, vb4, vy);
    }
    PA::template store<MASK == 1>(tl_lds, r0, R, kbeg, kend, va4, va, vy, mask_act);
    PB::template store<MASK == 2>(tl_lds + PSZ, c0, Cc, kbeg, kend, vb4, vb, vy, mask_act);
    __syncthreads();

    for (int t = 0; t < steps; ++t) {
        const bool more = t + 1 < steps;
        const int kn = kbeg + (t + 1) * kTK;
        if (more) {
            PA::load(A, lda, r0, R, kn, Kc, va4, va);
            PB::load(B, ldb, c0, Cc, kn, Kc, vb4, vb);
            if (use_y) {
                if (MASK == 1) PA::load(Y, lda, r0, R, kn, Kc, va4, vy);
                else PB::load(Y, ldb, c0, Cc, kn, Kc, vb4, vy);
            }
        }
        const float* pa = tl_lds + (t & 1) * 2 * PSZ + s * PA::LD + wr * 32 * WT + c;
        const float* pb = tl_lds + (t & 1) * 2 * PSZ + PSZ + s * PB::LD + wc * 32 * WT + c;
#pragma unroll
        for (int i = 0; i < kTK / 2; ++i) {
            float a[WT], b[WT];
#pragma unroll
            for (int u = 0; u < WT; ++u) {
                a[u] = pa[2 * i * PA::LD + 32 * u];
                b[u] = pb[2 * i * PB::LD + 32 * u];
            }
            if (ACC) {
#pragma unroll
                for (int u = 0; u < WT; ++u) bsum[u] += b[u];
            }
#pragma unroll
            for (int u = 0; u < WT; ++u)
#pragma unroll
                for (int w = 0; w < WT; ++w)
                    acc[u][w] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u], b[w], acc[u][w], 0, 0, 0);
        }
        if (more) {
            float* nxt = tl_lds + ((t + 1) & 1) * 2 * PSZ;
            PA::template store<MASK == 1>(nxt, r0, R, kn, kend, va4, va, vy, mask_act);
            PB::template store<MASK == 2>(nxt + PSZ, c0, Cc, kn, kend, vb4, vb, vy, mask_act);
        }
        __syncthreads();
    }

    // ---- epilogue: acc[u][w][r] is C[r0 + 32 (wr WT + u) + (r & 3) + 8 (r >> 2) + 4 s][c0 + 32 (wc WT + w) + c] ----
#pragma unroll
    for (int w = 0; w < WT; ++w) {
        const int col = c0 + 32 * (wc * WT + w) + c;
        if (col >= Cc) continue;
        const float bv = (!ACC && bias) ? bias[col] : 0.f;
#pragma unroll
        for (int u = 0; u < WT; ++u) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = r0 + 32 * (wr * WT + u) + (r & 3) + 8 * (r >> 2) + 4 * s;
                if (row >= R) continue;
                float* dst = C + (int64_t)row * ldc + col;
                if (ACC) {
                    if (atomic) atomicAdd(dst, acc[u][w][r]);
                    else *dst += acc[u][w][r];
                } else {
                    float v = acc[u][w][r] + bv;
                    if (act == DT_ACT_RELU) v = fmaxf(v, 0.f);
                    *dst = v;
                }
            }
        }
    }
    if (ACC) {
#pragma unroll
        for (int w = 0; w < WT; ++w) {
            float bs = bsum[w];
            bs += __shfl_xor(bs, 32, 64);        // the two contraction parities of the step
            const int col = c0 + 32 * (wc * WT + w) + c;
            if (want_b && s == 0 && col < Cc) atomicAdd(gb + col, bs);
        }
    }
}

constexpr int kFillBlocks = 256;   // one block per CU of the MI355X

inline size_t tiled_lds(int wt) { return (size_t)2 * 2 * kTK * (64 * wt + 1) * sizeof(float); }
inline int tiled_wt(int R, int Cc) { return (int64_t)ceil_div(R, 128) * ceil_div(Cc, 128) >= kFillBlocks ? 2 : 1; }
inline bool vec_ok(const void* p, const void* q, int64_t ld) {
    return ld % 4 == 0 && (((uintptr_t)p | (uintptr_t)q) % 16) == 0;
}

// grad_W's batch split: until the grid has ~2 blocks per CU, >= 256 rows per split, every split owning at least one step
struct BatchSplit {
    int splits, per;   // gridDim.z, contraction steps of kTK per split
};
inline BatchSplit tiled_batch_split(int N, int64_t tiles) {
    const int total_steps = ceil_div(N, kTK);
    int splits = 1;
    if (tiles < kFillBlocks) {
        splits = (int)((2 * kFillBlocks + tiles - 1) / tiles);
        const int most = ceil_div(N, 256);
        if (splits > most) splits = most;
    }
    const int per = ceil_div(total_steps, splits);
    return BatchSplit{ceil_div(total_steps, per), per};
}

template <bool AKC, bool BKC, int MASK, bool ACC>
void launch_tiled(hipStream_t st, int wt, dim3 grid, const float* A, int64_t lda, const float* B, int64_t ldb,
                  const float* Y, int mask_act, const float* bias, int act, int R, int Cc, int Kc, int steps_per_split,
                  int vecA, int vecB, float* C, int64_t ldc, float* gb, int atomic) {
    const size_t lds = tiled_lds(wt);
    if (wt == 2) {
        auto k = k_dense_tiled<AKC, BKC, MASK, ACC, 2>;
        hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL(k, grid, dim3(256), lds, st, A, lda, B, ldb, Y, mask_act, bias, act, R, Cc, Kc, steps_per_split,
                           vecA, vecB, C, ldc, gb, atomic);
    } else {
        auto k = k_dense_tiled<AKC, BKC, MASK, ACC, 1>;
        hipLaunchKernelGGL(k, grid, dim3(256), lds, st, A, lda, B, ldb, Y, mask_act, bias, act, R, Cc, Kc, steps_per_split,
                           vecA, vecB, C, ldc, gb, atomic);
    }
}

}  // namespace
}  // namespace dt

using namespace dt;

extern "C" int dt_dense_tiled_supported(int N, int K, int M) {
    if (N <= 0 || K <= 0 || M < 2) return 0;
    return ceil_div(K, 64) <= 65535 && ceil_div(M, 64) <= 65535;   // column tiles ride on gridDim.y
}

extern "C" int64_t dt_dense_tiled_workspace_bytes(int N, int K, int M) {
    (void)N; (void)K; (void)M;
    return 0;   // W is read transposed by the staging loads; the batch splits merge with atomics
}

extern "C" int dt_dense_tiled_geometry(int N, int K, int M, int product, int* tile, int* splits, int* steps_per_split) {
    DT_REQUIRE(product >= 0 && product <= 2, "dt_dense_tiled_geometry: product %d (0 forward, 1 grad_x, 2 grad_W)", product);
    DT_UNSUPPORTED(!dt_dense_tiled_supported(N, K, M), "dt_dense_tiled_geometry: N=%d K=%d M=%d", N, K, M);
    const int R = product == 2 ? K : N, Cc = product == 1 ? K : M, Kc = product == 0 ? K : product == 1 ? M : N;
    const int wt = tiled_wt(R, Cc), bt = 64 * wt;
    BatchSplit sp{1, ceil_div(Kc, kTK)};
    if (product == 2) sp = tiled_batch_split(N, (int64_t)ceil_div(K, bt) * ceil_div(M, bt));
    if (tile) *tile = bt;
    if (splits) *splits = sp.splits;
    if (steps_per_split) *steps_per_split = sp.per;
    return DT_OK;
}

extern "C" int dt_dense_tiled_fwd(const float* x, const float* W, const float* bias, int act, int N, int K, int M,
                                  float* y, void* stream) {
    DT_REQUIRE(N >= 0 && K > 0 && M > 0, "dt_dense_tiled_fwd: bad sizes N=%d K=%d M=%d", N, K, M);
    DT_REQUIRE(act == DT_ACT_LINEAR || act == DT_ACT_RELU, "dt_dense_tiled_fwd: act %d", act);
    if (N == 0) return DT_OK;
    DT_REQUIRE(x && W && y, "dt_dense_tiled_fwd: null pointer");
    DT_UNSUPPORTED(!dt_dense_tiled_supported(N, K, M), "dt_dense_tiled_fwd: N=%d K=%d M=%d (M == 1: dt_dense_fwd)", N, K, M);
    const int wt = tiled_wt(N, M), bt = 64 * wt;
    launch_tiled<true, false, 0, false>(as_stream(stream), wt, dim3(ceil_div(N, bt), ceil_div(M, bt), 1), x, K, W, M,
                                        nullptr, DT_ACT_LINEAR, bias, act, N, M, K, ceil_div(K, kTK), vec_ok(x, x, K),
                                        vec_ok(W, W, M), y, M, nullptr, 0);
    return launch_status("dt_dense_tiled_fwd");
}

extern "C" int dt_dense_tiled_bwd(const float* x, const float* W, const float* y, const float* grad_y, int act, int N,
                                  int K, int M, float* grad_x, float* grad_W, float* grad_b, void* ws, void* stream) {
    (void)ws;
    DT_REQUIRE(N >= 0 && K > 0 && M > 0, "dt_dense_tiled_bwd: bad sizes N=%d K=%d M=%d", N, K, M);
    DT_REQUIRE(act == DT_ACT_LINEAR || act == DT_ACT_RELU, "dt_dense_tiled_bwd: act %d", act);
    if (N == 0) return DT_OK;
    DT_REQUIRE(x && W && y && grad_y && grad_W, "dt_dense_tiled_bwd: null pointer");
    DT_UNSUPPORTED(!dt_dense_tiled_supported(N, K, M), "dt_dense_tiled_bwd: N=%d K=%d M=%d (M == 1: dt_dense_bwd)", N, K, M);
    hipStream_t st = as_stream(stream);
    if (grad_x) {   // grad_x [N,K] = G [N,M] . W^T: W[k][m] is contraction-contiguous for this product
        const int wt = tiled_wt(N, K), bt = 64 * wt;
        launch_tiled<true, true, 1, false>(st, wt, dim3(ceil_div(N, bt), ceil_div(K, bt), 1), grad_y, M, W, M, y, act,
                                           nullptr, DT_ACT_LINEAR, N, K, M, ceil_div(M, kTK), vec_ok(grad_y, y, M),
                                           vec_ok(W, W, M), grad_x, K, nullptr, 0);
    }
    // grad_W [K,M] += x^T [K,N] . G [N,M], the batch split over blockIdx.z (tiled_batch_split)
    const int wt = tiled_wt(K, M), bt = 64 * wt;
    const BatchSplit sp = tiled_batch_split(N, (int64_t)ceil_div(K, bt) * ceil_div(M, bt));
    launch_tiled<false, false, 2, true>(st, wt, dim3(ceil_div(K, bt), ceil_div(M, bt), sp.splits), x, K, grad_y, M, y,
                                        act, nullptr, DT_ACT_LINEAR, K, M, N, sp.per, vec_ok(x, x, K), vec_ok(grad_y, y, M),
                                        grad_W, M, grad_b, sp.splits > 1);
    return launch_status("dt_dense_tiled_bwd");
}
