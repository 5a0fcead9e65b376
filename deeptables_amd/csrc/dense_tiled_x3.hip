// dense_tiled_x3.hip — the tiled Keras `Dense` of dense_tiled.hip on the bf16 matrix cores: the same three products under
// the same contract (y = act(x W + b); grad_x = G W^T OVERWRITTEN, may be NULL; grad_W += x^T G and grad_b += colsum(G)
// ACCUMULATED, grad_b may be NULL; G = grad_y * act'(y) formed while grad_y is staged; fp32 tensors in HBM, fp32
// accumulation, 64-bit element offsets, no transpose pass over W, no workspace), with the operands split into bf16 parts
// (x3_mfma.h) on their way from the staging registers into LDS.  Nothing pre-split is ever written to HBM.
//   DT_DENSE_X3   forward: three parts per operand, six products a1 b1 + (a1 b2 + a2 b1) + (a1 b3 + a2 b2 + a3 b1): the
//                 dropped terms are 2^-24 of a product (class fp32);  grad_x / grad_W: two parts, three products (b17)
//   DT_DENSE_BF16 one part, one product, everywhere (class bf16)
// grad_b is summed from the masked fp32 values in the staging registers, before they are split: fp32 in both modes.
//
// One kernel, k_dense_x3<AKC, BKC, MASK, ACC, NP, WT>, on v_mfma_f32_32x32x16_bf16.  Block = 256 threads = 2 x 2 waves;
// output tile 128 x 128 (each wave 2 x 2 MFMA tiles) when that alone gives >= 256 blocks, else 64 x 64 — the rule of
// dense_tiled.hip, so a shape reaches the same tile and the same batch split of grad_W in both families.  The contraction
// is walked in steps of 32 (two MFMAs deep).  Per step each thread stages BT / 64 runs of 8 consecutive contraction
// indices of one output row per operand: two 16-byte global loads where the source is contraction-contiguous (only 4-byte
// alignment is relied on: odd row lengths such as K = 10,413 take the same loads), eight dword loads coalesced across the
// lanes where it is output-contiguous (W in the forward, x and G in grad_W); the last, partial step of a contraction
// always takes clamped dword loads.  The run is masked, split, and written as ONE 16-byte ds_write per part into
// panel[part][row][32 k (+ 8 pad)] bf16: the operand of lane (c, s) for k-half i is the 16 bytes at row c, k = 16 i + 8 s,
// and the 80-byte row stride puts the 16 lanes of every ds_read_b128 group on 16 different 16-byte slots (5 row mod 16 is
// a bijection): conflict-free.  The next step's global loads are issued before this step's MFMAs and split and written
// after them.  64 x 64: two panel buffers, one barrier per step (the buffer written was last read a barrier ago).
// 128 x 128: one buffer and two barriers per step (two would leave room for one block per CU only); the two blocks
// per CU overlap each other's staging.
//   LDS per block:  buffers x 2 panels x NP parts x BT x 80 B = 61,440 B at NP = 3, 40,960 at NP = 2, 20,480 at NP = 1,
//                   at either tile (128 x 128 x 1 buffer, 64 x 64 x 2 buffers).  Independent of N, K and M.
//   registers (-Rpass-analysis=kernel-resource-usage, gfx950; VGPRs + AGPRs; scratch 0 in all twelve instances):
//                   128 x 128: forward 110 + 64 (NP = 3) / 80 + 64 (NP = 1), grad_x 126 + 64 / 100 + 64, grad_W 136 + 64
//                   (both): two waves per SIMD (three for the NP = 1 forward and grad_x) = the two blocks per CU the LDS
//                   leaves room for;  64 x 64: forward 64 + 16 / 53 + 16, grad_x 62 + 16, grad_W 80 + 16: five to seven.
// Edges (N / K / M not multiples of the tile): loads go unconditionally to a clamped address and the value is zeroed
// before it is split; stores are guarded.
// Non-finite values: a part of +-inf or NaN is itself in the high part, and its LOW parts are set to zero instead of
// v - (float)hi = inf - inf = NaN.  A finite neighbour therefore only ever meets the non-finite value itself, in the
// same products the fp32 kernel forms with it: an inf in x[r][k] reaches row r of y and row k of grad_W, a NaN in W[k][m]
// column m of y and column k of grad_x, nothing else.  (inf times a zero low part is NaN where the fp32 kernel has inf:
// inside the row or column that is poisoned anyway.)  The same rule covers a finite value beyond bf16's largest
// (|v| >= 3.3962e38), whose high part rounds to inf.  A NaN pre-activation under relu stores fmaxf(NaN, 0) = 0 and
// passes no gradient (!(y > 0)), as dense_tiled.hip.
#include "common.h"
#include "x3_mfma.h"

namespace dt {
namespace {

typedef floatx4 dx_f4u __attribute__((aligned(4)));   // a 16-byte load that relies on a float's alignment only
constexpr int kXK = 32;     // contraction indices per step (two 32x32x16 MFMAs per tile and product)
constexpr int kXLD = 40;    // bf16 per panel row: 32 + 8 pad = 80 bytes

__device__ __forceinline__ float dx_dact(float g, float y, int act) {
    return (act == DT_ACT_RELU && !(y > 0.f)) ? 0.f : g;
}

// One operand panel of one contraction step: [NP parts][BR rows][kXLD] bf16, BR = the tile's extent along the output index.
// A thread's item e is a run of 8 contraction indices [8 kg, 8 kg + 8) of one row rl:
//   KC = true : source is contraction-contiguous, src[(r0 + rl) * ld + k];  item = (rl = idx / 4, kg = idx % 4)
//   KC = false: source is output-contiguous,      src[k * ld + r0 + rl];    item = (rl = idx % BR, kg = idx / BR)
// with idx = tid + 256 e.  load() only issues the global loads (clamped addresses); store() zeroes what lies outside
// [0, R) x [., kend), applies the relu mask, splits and writes LDS, so the loads stay in flight across the MFMAs.
template <bool KC, int BR>
struct XPanel {
    static constexpr int NI = BR / 64;           // items per thread per step
    static constexpr int PART = BR * kXLD;       // bf16 elements per part

    static __device__ __forceinline__ void item(int e, int& rl, int& kg) {
        const int idx = threadIdx.x + 256 * e;
        if (KC) { rl = idx >> 2; kg = idx & 3; }
        else { rl = idx % BR; kg = idx / BR; }
    }

    // full: k0 + kXK <= Kc (block-uniform)
    static __device__ __forceinline__ void load(const float* __restrict__ src, int64_t ld, int r0, int R, int k0, int Kc,
                                                bool full, float (&v)[NI][8]) {
#pragma unroll
        for (int e = 0; e < NI; ++e) {
            int rl, kg;
            item(e, rl, kg);
            const int row = min(r0 + rl, R - 1);
            const int kb = k0 + 8 * kg;
            if (KC) {
                const float* p = src + (int64_t)row * ld;
                if (full) {
                    const dx_f4u q0 = *reinterpret_cast<const dx_f4u*>(p + kb);       // 4-byte aligned dwordx4
                    const dx_f4u q1 = *reinterpret_cast<const dx_f4u*>(p + kb + 4);
#pragma unroll
                    for (int j = 0; j < 4; ++j) { v[e][j] = q0[j]; v[e][4 + j] = q1[j]; }
                } else {
#pragma unroll
                    for (int j = 0; j < 8; ++j) v[e][j] = p[min(kb + j, Kc - 1)];
                }
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j) v[e][j] = src[(int64_t)min(kb + j, Kc - 1) * ld + row];
            }
        }
    }

    template <bool MASKED, int NP>
    static __device__ __forceinline__ void store(__bf16* __restrict__ panel, int r0, int R, int k0, int kend,
                                                 const float (&v)[NI][8], const float (&y)[NI][8], int mask_act,
                                                 float& gsum) {
#pragma unroll
        for (int e = 0; e < NI; ++e) {
            int rl, kg;
            item(e, rl, kg);
            const bool rok = r0 + rl < R;
            const int kb = k0 + 8 * kg;
            float w[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                float val = v[e][j];
                if (MASKED) val = dx_dact(val, y[e][j], mask_act);
                w[j] = (rok && kb + j < kend) ? val : 0.f;
                if (MASKED) gsum += w[j];
            }
            x3_b8 h, m, l;
            if (NP == 3) x3_split3(w, h, m, l);
            else if (NP == 2) x3_split2(w, h, m);
            else {
#pragma unroll
                for (int j = 0; j < 8; ++j) h[j] = (__bf16)w[j];
            }
            if (NP > 1) {
                // a non-finite high part (inf, NaN, or a finite value that rounds to inf) keeps no low parts: inf - inf
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    if (!(fabsf((float)h[j]) < __builtin_huge_valf())) {
                        m[j] = (__bf16)0.f;
                        if (NP == 3) l[j] = (__bf16)0.f;
                    }
                }
            }
            __bf16* dst = panel + rl * kXLD + 8 * kg;
            *reinterpret_cast<x3_b8*>(dst) = h;
            if (NP >= 2) *reinterpret_cast<x3_b8*>(dst + PART) = m;
            if (NP == 3) *reinterpret_cast<x3_b8*>(dst + 2 * PART) = l;
        }
    }
};

// ---------------------------------------------------------------------------------------------------------------------
// C[R, Cc] (=|+=) A[R, Kc] . B[Kc, Cc]      grid (row tiles, column tiles, contraction splits)
//   AKC / BKC : the operand's source is contraction-contiguous (see XPanel)
//   MASK      : 0 none, 1 A = A * act'(Y), 2 B = B * act'(Y); Y has the masked operand's layout
//   ACC       : false: C = act(A B + bias);  true: C += A B (plain when `atomic` == 0, float atomics otherwise) and
//               gb[col] += column sums of B in fp32, from the blocks of row tile 0
//   NP        : bf16 parts per operand: 3 (six products), 2 (three products), 1 (one product)
//   WT        : MFMA tiles per wave in each direction (block tile = 64 WT x 64 WT)
// ---------------------------------------------------------------------------------------------------------------------
template <bool AKC, bool BKC, int MASK, bool ACC, int NP, int WT>
__global__ __launch_bounds__(256) void k_dense_x3(const float* __restrict__ A, int64_t lda, const float* __restrict__ B,
                                                  int64_t ldb, const float* __restrict__ Y, int mask_act,
                                                  const float* __restrict__ bias, int act, int R, int Cc, int Kc,
                                                  int steps_per_split, float* __restrict__ C, int64_t ldc,
                                                  float* __restrict__ gb, int atomic) {
    constexpr int BT = 64 * WT;
    using PA = XPanel<AKC, BT>;
    using PB = XPanel<BKC, BT>;
    constexpr int NI = PA::NI;
    constexpr int PART = PA::PART;
    constexpr int NBUF = WT == 1 ? 2 : 1;        // 64 x 64: double buffered, one barrier per step
    constexpr int BUF = 2 * NP * PART;           // bf16 elements per buffer
    extern __shared__ __attribute__((aligned(16))) __bf16 dx_lds[];   // [NBUF][A panel: NP parts | B panel: NP parts]
    __bf16* const lds_a = dx_lds;
    __bf16* const lds_b = dx_lds + NP * PART;

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int s = lane >> 5, c = lane & 31;
    const int wr = wave >> 1, wc = wave & 1;
    const int r0 = blockIdx.x * BT, c0 = blockIdx.y * BT;
    const int kbeg = blockIdx.z * steps_per_split * kXK;
    const int kend = min(Kc, kbeg + steps_per_split * kXK);
    const int steps = (kend - kbeg + kXK - 1) / kXK;
    const bool use_y = MASK != 0 && mask_act == DT_ACT_RELU;

    floatx16 acc[WT][WT];
#pragma unroll
    for (int i = 0; i < WT; ++i)
#pragma unroll
        for (int j = 0; j < WT; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    float va[NI][8], vb[NI][8], vy[NI][8];
#pragma unroll
    for (int e = 0; e < NI; ++e)
#pragma unroll
        for (int j = 0; j < 8; ++j) vy[e][j] = 1.f;
    float gsum = 0.f, unused = 0.f;

    {
        const bool full = kbeg + kXK <= Kc;
        PA::load(A, lda, r0, R, kbeg, Kc, full, va);
        PB::load(B, ldb, c0, Cc, kbeg, Kc, full, vb);
        if (use_y) {
            if (MASK == 1) PA::load(Y, lda, r0, R, kbeg, Kc, full, vy);
            else PB::load(Y, ldb, c0, Cc, kbeg, Kc, full, vy);
        }
        PA::template store<MASK == 1, NP>(lds_a, r0, R, kbeg, kend, va, vy, mask_act, unused);
        PB::template store<MASK == 2, NP>(lds_b, c0, Cc, kbeg, kend, vb, vy, mask_act, gsum);
    }
    __syncthreads();

    const int poff_a = (wr * 32 * WT + c) * kXLD + 8 * s, poff_b = (wc * 32 * WT + c) * kXLD + 8 * s;
    for (int t = 0; t < steps; ++t) {
        const bool more = t + 1 < steps;
        const int kn = kbeg + (t + 1) * kXK;
        if (more) {
            const bool full = kn + kXK <= Kc;
            PA::load(A, lda, r0, R, kn, Kc, full, va);
            PB::load(B, ldb, c0, Cc, kn, Kc, full, vb);
            if (use_y) {
                if (MASK == 1) PA::load(Y, lda, r0, R, kn, Kc, full, vy);
                else PB::load(Y, ldb, c0, Cc, kn, Kc, full, vy);
            }
        }
        const int cur = NBUF == 2 ? (t & 1) * BUF : 0, nxt = NBUF == 2 ? ((t + 1) & 1) * BUF : 0;
        const __bf16* pa = lds_a + cur + poff_a;
        const __bf16* pb = lds_b + cur + poff_b;
#pragma unroll
        for (int i = 0; i < kXK / 16; ++i) {
            x3_b8 a[NP][WT], b[NP][WT];
#pragma unroll
            for (int p = 0; p < NP; ++p)
#pragma unroll
                for (int u = 0; u < WT; ++u) {
                    a[p][u] = x3_ld8(pa + p * PART + 32 * u * kXLD + 16 * i);
                    b[p][u] = x3_ld8(pb + p * PART + 32 * u * kXLD + 16 * i);
                }
#pragma unroll
            for (int u = 0; u < WT; ++u)
#pragma unroll
                for (int w = 0; w < WT; ++w) {
                    // the smallest products first: p + q = 2 (six products only), then 1, then the leading one
#pragma unroll
                    for (int o = (NP == 3 ? 2 : NP - 1); o >= 0; --o)
#pragma unroll
                        for (int p = 0; p <= o; ++p)
                            acc[u][w] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[p][u], b[o - p][w], acc[u][w], 0, 0, 0);
                }
        }
        if (NBUF == 1) __syncthreads();                   // every wave has read this step's panels
        if (more) {
            PA::template store<MASK == 1, NP>(lds_a + nxt, r0, R, kn, kend, va, vy, mask_act, unused);
            PB::template store<MASK == 2, NP>(lds_b + nxt, c0, Cc, kn, kend, vb, vy, mask_act, gsum);
        }
        if (NBUF == 2 || more) __syncthreads();           // two buffers: the one written was last read a barrier ago
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
    if (ACC && MASK == 2) {
        // grad_b: every thread's items share one column (tid % BT) of the B panel; 256 / BT threads per column.  The last
        // barrier of the loop has passed: the panels are free.
        if (gb != nullptr && blockIdx.x == 0) {           // block-uniform
            float* red = reinterpret_cast<float*>(dx_lds);
            red[threadIdx.x] = gsum;
            __syncthreads();
            if (threadIdx.x < BT) {
                float tot = 0.f;
#pragma unroll
                for (int q = 0; q < 256 / BT; ++q) tot += red[threadIdx.x + BT * q];
                const int col = c0 + threadIdx.x;
                if (col < Cc) atomicAdd(gb + col, tot);
            }
        }
    }
}

constexpr int kXFillBlocks = 256;   // one block per CU of the MI355X

inline int x3_parts(int mode, int product) { return mode == DT_DENSE_BF16 ? 1 : product == 0 ? 3 : 2; }
inline size_t x3_lds(int wt, int np) { return (size_t)(wt == 1 ? 2 : 1) * 2 * np * 64 * wt * kXLD * sizeof(__bf16); }
inline int x3_wt(int R, int Cc) { return (int64_t)ceil_div(R, 128) * ceil_div(Cc, 128) >= kXFillBlocks ? 2 : 1; }

// grad_W's batch split: until the grid has ~2 blocks per CU, >= 256 rows per split, every split owning at least one step
struct XSplit {
    int splits, per;   // gridDim.z, contraction steps of kXK per split
};
inline XSplit x3_batch_split(int N, int64_t tiles) {
    const int total_steps = ceil_div(N, kXK);
    int splits = 1;
    if (tiles < kXFillBlocks) {
        splits = (int)((2 * kXFillBlocks + tiles - 1) / tiles);
        const int most = ceil_div(N, 256);
        if (splits > most) splits = most;
    }
    const int per = ceil_div(total_steps, splits);
    return XSplit{ceil_div(total_steps, per), per};
}

// what one product launches with: everything the geometry query reports and the launches use
struct XGeom {
    int R, Cc, Kc, wt, splits, per;
};
inline XGeom x3_geometry(int N, int K, int M, int product) {
    XGeom g;
    g.R = product == 2 ? K : N;
    g.Cc = product == 1 ? K : M;
    g.Kc = product == 0 ? K : product == 1 ? M : N;
    g.wt = x3_wt(g.R, g.Cc);
    g.splits = 1;
    g.per = ceil_div(g.Kc, kXK);
    if (product == 2) {
        const XSplit sp = x3_batch_split(N, (int64_t)ceil_div(K, 64 * g.wt) * ceil_div(M, 64 * g.wt));
        g.splits = sp.splits;
        g.per = sp.per;
    }
    return g;
}

template <bool AKC, bool BKC, int MASK, bool ACC, int NP>
void launch_x3(hipStream_t st, const XGeom& g, const float* A, int64_t lda, const float* B, int64_t ldb, const float* Y,
               int mask_act, const float* bias, int act, float* C, int64_t ldc, float* gb) {
    const size_t lds = x3_lds(g.wt, NP);
    const int bt = 64 * g.wt;
    const dim3 grid(ceil_div(g.R, bt), ceil_div(g.Cc, bt), g.splits);
    if (g.wt == 2) {
        hipLaunchKernelGGL((k_dense_x3<AKC, BKC, MASK, ACC, NP, 2>), grid, dim3(256), lds, st, A, lda, B, ldb, Y, mask_act,
                           bias, act, g.R, g.Cc, g.Kc, g.per, C, ldc, gb, g.splits > 1);
    } else {
        hipLaunchKernelGGL((k_dense_x3<AKC, BKC, MASK, ACC, NP, 1>), grid, dim3(256), lds, st, A, lda, B, ldb, Y, mask_act,
                           bias, act, g.R, g.Cc, g.Kc, g.per, C, ldc, gb, g.splits > 1);
    }
}

inline bool x3_mode_ok(int mode) { return mode == DT_DENSE_X3 || mode == DT_DENSE_BF16; }

}  // namespace
}  // namespace dt

using namespace dt;

extern "C" int dt_dense_x3_supported(int N, int K, int M, int mode) {
    if (!x3_mode_ok(mode)) return 0;
    if (N <= 0 || K <= 0 || M < 2) return 0;
    return ceil_div(K, 64) <= 65535 && ceil_div(M, 64) <= 65535;   // column tiles ride on gridDim.y
}

extern "C" int64_t dt_dense_x3_workspace_bytes(int N, int K, int M, int mode) {
    (void)N; (void)K; (void)M; (void)mode;
    return 0;   // the parts are formed on the way into LDS; the batch splits merge with atomics
}

extern "C" int dt_dense_x3_geometry(int N, int K, int M, int mode, int product, int* tile_rows, int* tile_cols, int* splits,
                                    int* steps_per_split) {
    DT_REQUIRE(product >= 0 && product <= 2, "dt_dense_x3_geometry: product %d (0 forward, 1 grad_x, 2 grad_W)", product);
    DT_REQUIRE(x3_mode_ok(mode), "dt_dense_x3_geometry: mode %d (DT_DENSE_X3, DT_DENSE_BF16)", mode);
    DT_UNSUPPORTED(!dt_dense_x3_supported(N, K, M, mode), "dt_dense_x3_geometry: N=%d K=%d M=%d", N, K, M);
    const XGeom g = x3_geometry(N, K, M, product);
    if (tile_rows) *tile_rows = 64 * g.wt;
    if (tile_cols) *tile_cols = 64 * g.wt;
    if (splits) *splits = g.splits;
    if (steps_per_split) *steps_per_split = g.per;
    return DT_OK;
}

extern "C" int dt_dense_x3_fwd(const float* x, const float* W, const float* bias, int act, int N, int K, int M, float* y,
                               int mode, void* ws, void* stream) {
    (void)ws;
    DT_REQUIRE(N >= 0 && K > 0 && M > 0, "dt_dense_x3_fwd: bad sizes N=%d K=%d M=%d", N, K, M);
    DT_REQUIRE(act == DT_ACT_LINEAR || act == DT_ACT_RELU, "dt_dense_x3_fwd: act %d", act);
    DT_REQUIRE(x3_mode_ok(mode), "dt_dense_x3_fwd: mode %d (DT_DENSE_X3, DT_DENSE_BF16)", mode);
    if (N == 0) return DT_OK;
    DT_REQUIRE(x && W && y, "dt_dense_x3_fwd: null pointer");
    DT_UNSUPPORTED(!dt_dense_x3_supported(N, K, M, mode), "dt_dense_x3_fwd: N=%d K=%d M=%d (M == 1: dt_dense_fwd)", N, K, M);
    hipStream_t st = as_stream(stream);
    const XGeom g = x3_geometry(N, K, M, 0);
    if (mode == DT_DENSE_X3)
        launch_x3<true, false, 0, false, 3>(st, g, x, K, W, M, nullptr, DT_ACT_LINEAR, bias, act, y, M, nullptr);
    else
        launch_x3<true, false, 0, false, 1>(st, g, x, K, W, M, nullptr, DT_ACT_LINEAR, bias, act, y, M, nullptr);
    return launch_status("dt_dense_x3_fwd");
}

extern "C" int dt_dense_x3_bwd(const float* x, const float* W, const float* y, const float* grad_y, int act, int N, int K,
                               int M, float* grad_x, float* grad_W, float* grad_b, int mode, void* ws, void* stream) {
    (void)ws;
    DT_REQUIRE(N >= 0 && K > 0 && M > 0, "dt_dense_x3_bwd: bad sizes N=%d K=%d M=%d", N, K, M);
    DT_REQUIRE(act == DT_ACT_LINEAR || act == DT_ACT_RELU, "dt_dense_x3_bwd: act %d", act);
    DT_REQUIRE(x3_mode_ok(mode), "dt_dense_x3_bwd: mode %d (DT_DENSE_X3, DT_DENSE_BF16)", mode);
    if (N == 0) return DT_OK;
    DT_REQUIRE(x && W && y && grad_y && grad_W, "dt_dense_x3_bwd: null pointer");
    DT_UNSUPPORTED(!dt_dense_x3_supported(N, K, M, mode), "dt_dense_x3_bwd: N=%d K=%d M=%d (M == 1: dt_dense_bwd)", N, K, M);
    hipStream_t st = as_stream(stream);
    if (grad_x) {   // grad_x [N,K] = G [N,M] . W^T: W[k][m] is contraction-contiguous for this product
        const XGeom g = x3_geometry(N, K, M, 1);
        if (mode == DT_DENSE_X3)
            launch_x3<true, true, 1, false, 2>(st, g, grad_y, M, W, M, y, act, nullptr, DT_ACT_LINEAR, grad_x, K, nullptr);
        else
            launch_x3<true, true, 1, false, 1>(st, g, grad_y, M, W, M, y, act, nullptr, DT_ACT_LINEAR, grad_x, K, nullptr);
    }
    // grad_W [K,M] += x^T [K,N] . G [N,M], the batch split over blockIdx.z (x3_batch_split)
    const XGeom g = x3_geometry(N, K, M, 2);
    if (mode == DT_DENSE_X3)
        launch_x3<false, false, 2, true, 2>(st, g, x, K, grad_y, M, y, act, nullptr, DT_ACT_LINEAR, grad_W, M, grad_b);
    else
        launch_x3<false, false, 2, true, 1>(st, g, x, K, grad_y, M, y, act, nullptr, DT_ACT_LINEAR, grad_W, M, grad_b);
    return launch_status("dt_dense_x3_bwd");
}
