// pnn_infer.hip — fused PNN inference (dt_pnn_infer*, include/dt_hip.h): each of the product nets 'pnn_nets', 'ipnn_nets'
// and 'opnn_nets', alone in config.nets, scored with ONE launch per predict batch after one `prepare` launch per call.
//
// At inference Dropout is the identity, BatchNormalization a per-column affine map, and a row's logit depends on that row
// alone.  Per row, over the P = F (F - 1) / 2 pairs p = (i, j), i < j (itertools.combinations order):
//   inner_p = x_i . x_j                                                          (InnerProduct.call, layers.py:473-487)
//   outer_p = sum_{a,d} K[a,p,d] x_i[d] x_j[a]  'mat'  |  sum_d x_i[d] x_j[d] K[p,d]  'vec'  |  .. K[p]  'num'   (:543-581)
//   tower input = [inner ++ outer ++ Xn],  Xn = (concat(embeddings, dense) - mm) scale + beta   (deepnets.py:111-160)
// The products are formed from the RAW rows; only the F D + Nd columns behind them are normalised.
//
// A block of 512 threads owns a tile of 32 batch rows (k_infer's tile, infer_x3.h) and strides over the tiles:
//   1. gather: the tile's F table rows and Nd dense values -> the fp32 slab [32][F D + Nd (+ pad)] in LDS (ids decoded as
//      DT_IDX_*; an out-of-range id reads a zero row and is counted once).  A wave has the ids, then the table rows, of its
//      four rows in flight together.
//   2. the first Dense's K = Cp + F D + Nd dimension in chunks of 128 columns.  A chunk is COMPUTED into the chunk buffer as
//      three bf16 parts [3][32][128 + 16] and then multiplied: wave w owns hidden units [16 w, 16 w + 16) and both row halves,
//      its 2 x 3 accumulators stay in registers over all chunks (k_infer's GEMM1 with the K loop cut into chunks).
//        inner / 'vec' / 'num' columns   one thread per (row, column): a dot over D from the slab
//        'mat' columns                   one wave per pair, EXACT fp32 on the matrix core (v_mfma_f32_16x16x4_f32, as
//                                        k_afm_infer): C^T [a x rows] = K_p [a x d] . X_i^T [d x rows], so the lane that holds
//                                        row n's U[n][4 g .. 4 g + 3] multiplies them with x_j[n][4 g ..] (one 16-byte LDS
//                                        read) and two permlane swaps end the sum over a.  K_p [D][D] was re-laid pair-major
//                                        by `prepare`: a wave reads it once from L2, contiguously, for both row halves.
//        embedding / dense columns       (x - mm) scale + beta with the centring kept, as k_infer
//      By default the tower's products are the six split-bf16 products of x3_mfma.h (the fp32 class); ONE
//      (DT_INFER_TOWER_BF16) keeps the leading product only.  The product layers are exact fp32 in both modes.
//   3. cell 1's epilogue (infer_cell1, as GEMM1's step and the lookup setup from infer_common.h), then GEMM2, cell 2's
//      epilogue and task_output's vector in k_infer's text (infer_x3.h), the bias and the activation through infer_store.
//      The fp32 H1 tile takes the chunk buffer's place in LDS.
// Only the logit (and the activated output) is written.
//
// LDS (bytes): slab 128 RS, RS = F D + roundup(Nd, 8) + 4 (4 x odd: 16 rows on 16 distinct bank quads) | input BN 12 (F D + Nd)
// | pair table 4 P | chunk buffer 27,648 | w3 partial sums 512.  F = 26, D = 16, Nd = 13: 91 KB; the most, F = 64, D = 8,
// Nd = 64: 117 KB.  One block per CU.
#include "infer_common.h"

namespace dt {

constexpr int kPnnThreads = 512;
constexpr int kPnnKC = 128;                  // columns of a chunk = 4 K steps of 32
constexpr int kPnnXS = kPnnKC + 16;          // bf16 row stride of the chunk buffer (k_infer's CP + 16)
constexpr int kPnnXP = kTM * kPnnXS;         // one part

// offsets (floats) inside the workspace dt_pnn_infer_prepare writes
struct PnnWsLayout {
    int64_t stamp, w1b, w2b, bn, cell1, cell2, w3, head, kp, total;
    int P, Cp, CB, CBP, K, KP;
};
__host__ __device__ inline PnnWsLayout pnn_ws_layout(int F, int D, int Nd, int products, int kt) {
    PnnWsLayout w;
    int64_t o = 0;
    auto take = [&](int64_t n) { int64_t r = o; o += (n + 3) & ~(int64_t)3; return r; };
    const bool outer = (products & DT_PNN_OUTER) != 0;
    w.P = F * (F - 1) / 2;
    w.Cp = w.P * (((products & DT_PNN_INNER) ? 1 : 0) + (outer ? 1 : 0));
    w.CB = F * D + Nd;
    w.CBP = (w.CB + 3) & ~3;
    w.K = w.Cp + w.CB;
    w.KP = (w.K + kPnnKC - 1) / kPnnKC * kPnnKC;
    w.stamp = take(4);                               // what the workspace was prepared for: pnn_stamp0 / pnn_stamp1
    w.w1b = take((int64_t)3 * w.KP * kH1 / 2);       // 3 bf16 parts of [KP][128], lane-major as k_infer_prep's W1B
    w.w2b = take((int64_t)3 * kH1 * kH2 / 2);        // 3 bf16 parts of [128][64], lane-major
    w.bn = take((int64_t)3 * w.CBP);                 // input BN: mm | gamma / sqrt(mv + eps) | beta
    w.cell1 = take(3 * kH1);                         // tower cell 1: ctr | scl | sft, zero beyond H1
    w.cell2 = take(3 * kH2);
    w.w3 = take(kH2);                                // task_output's kernel [H2]
    w.head = take(4);                                // 1, b_out
    w.kp = take(!outer ? 0 : kt == DT_OP_KERNEL_MAT ? (int64_t)w.P * D * D : kt == DT_OP_KERNEL_VEC ? (int64_t)w.P * D : w.P);
    w.total = o;
    return w;
}
// The workspace's first two words name what it was prepared for.  They sit at offset 0 whatever the layout, so a launch
// with other (F, D, Nd, products, kernel_type) sees it before it reads anything else and scores every row NaN.
__host__ __device__ inline int pnn_stamp0(int F, int D, int Nd) { return 0x50000000 | F | (D << 8) | (Nd << 16); }
__host__ __device__ inline int pnn_stamp1(int products, int kt) { return 0x4E000000 | products | (kt << 4); }
__host__ __device__ inline int pnn_row_stride(int F, int D, int Nd) { return F * D + ((Nd + 7) & ~7) + 4; }
inline size_t pnn_infer_lds(int F, int D, int Nd) {
    const int P4 = (F * (F - 1) / 2 + 3) & ~3, CBP = (F * D + Nd + 3) & ~3;
    return ((size_t)kTM * pnn_row_stride(F, D, Nd) + (size_t)3 * CBP + P4 + 4 * kTM) * sizeof(float) + (size_t)3 * kPnnXP * 2;
}

struct PnnPrepArgs {
    const float* opk;                 // the outer kernel: 'mat' [D][P][D] | 'vec' [P][D] | 'num' [P][1]; NULL without DT_PNN_OUTER
    const float *gamma, *beta, *mm, *mv;
    float eps;
    const float* W1; int ld1, H1;
    const float* W2; int ld2, H2;
    const float *b[2], *cg[2], *cb[2], *cm[2], *cv[2];      // per tower cell, as InferPrepArgs
    float ceps[2];
    const float *w3, *bout;
    int F, D, Nd, products, kt;
};

// one thread per item of every layout; grid-stride.  Every value is read here, at call time.
__global__ __launch_bounds__(256) void k_pnn_infer_prep(PnnPrepArgs a, float* __restrict__ ws) {
    const PnnWsLayout wl = pnn_ws_layout(a.F, a.D, a.Nd, a.products, a.kt);
    const int64_t stride = (int64_t)gridDim.x * blockDim.x, t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t0 == 0) {
        reinterpret_cast<int*>(ws)[wl.stamp] = pnn_stamp0(a.F, a.D, a.Nd);
        reinterpret_cast<int*>(ws)[wl.stamp + 1] = pnn_stamp1(a.products, a.kt);
        ws[wl.head] = 1.f;
        ws[wl.head + 1] = a.bout ? a.bout[0] : 0.f;
    }
    __bf16* w1b = reinterpret_cast<__bf16*>(ws + wl.w1b);
    __bf16* w2b = reinterpret_cast<__bf16*>(ws + wl.w2b);
    const int64_t n1 = (int64_t)wl.KP * kH1, n2 = (int64_t)kH1 * kH2;     // elements of one part
    auto split_store = [](const float (&v)[8], __bf16* dst, int64_t lo) {
        x3_b8 h, m, l;
        x3_split3(v, h, m, l);
        *reinterpret_cast<x3_b8*>(dst) = h;
        *reinterpret_cast<x3_b8*>(dst + lo) = m;
        *reinterpret_cast<x3_b8*>(dst + 2 * lo) = l;
    };
    // W1B: lane (n, g) of wave w at step s holds W1[32 s + 8 g + j][16 w + n]; zero beyond K rows / H1 columns.  W1's rows
    // are in the chunk order already: products (inner, then outer), embeddings, dense.
    const int64_t n1b = (int64_t)(wl.KP >> 5) * 512;
    for (int64_t e = t0; e < n1b; e += stride) {
        const int l = (int)(e & 63), w = (int)((e >> 6) & 7), st = (int)(e >> 9);
        const int k0 = 32 * st + 8 * (l >> 4), n = 16 * w + (l & 15);
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = (k0 + j < wl.K && n < a.H1) ? a.W1[(int64_t)(k0 + j) * a.ld1 + n] : 0.f;
        split_store(v, w1b + e * 8, n1);
    }
    for (int64_t e = t0; e < 1024; e += stride) {
        const int l = (int)(e & 63), t = (int)((e >> 6) & 3), st = (int)(e >> 8);
        const int k0 = 32 * st + 8 * (l >> 4), n = 16 * t + (l & 15);
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = (k0 + j < a.H1 && n < a.H2) ? a.W2[(int64_t)(k0 + j) * a.ld2 + n] : 0.f;
        split_store(v, w2b + e * 8, n2);
    }
    for (int64_t c = t0; c < wl.CBP; c += stride) {
        float mm = 0.f, sc = 0.f, be = 0.f;
        if (c < wl.CB) {
            mm = a.mm[c];
            sc = (a.gamma ? a.gamma[c] : 1.f) * (1.0f / sqrtf(a.mv[c] + a.eps));
            be = a.beta ? a.beta[c] : 0.f;
        }
        ws[wl.bn + c] = mm; ws[wl.bn + wl.CBP + c] = sc; ws[wl.bn + 2 * wl.CBP + c] = be;
    }
    for (int64_t e = t0; e < kH1 + kH2; e += stride) {
        const int cell = e < kH1 ? 0 : 1, n = (int)(cell ? e - kH1 : e), W = cell ? kH2 : kH1, H = cell ? a.H2 : a.H1;
        float* dst = ws + (cell ? wl.cell2 : wl.cell1);
        float ctr = 0.f, scl = 0.f, sft = 0.f;
        if (n < H) {
            const float bias = a.b[cell] ? a.b[cell][n] : 0.f;
            if (a.cm[cell]) {
                ctr = a.cm[cell][n] - bias;
                scl = (a.cg[cell] ? a.cg[cell][n] : 1.f) * (1.0f / sqrtf(a.cv[cell][n] + a.ceps[cell]));
                sft = a.cb[cell] ? a.cb[cell][n] : 0.f;
            } else {
                ctr = -bias; scl = 1.f;
            }
        }
        dst[n] = ctr; dst[W + n] = scl; dst[2 * W + n] = sft;
    }
    for (int64_t e = t0; e < kH2; e += stride) ws[wl.w3 + e] = e < a.H2 ? a.w3[e] : 0.f;
    if (a.products & DT_PNN_OUTER) {
        const int D = a.D, P = wl.P;
        if (a.kt == DT_OP_KERNEL_MAT) {      // K [a][p][d] -> K_p [p][a][d]
            const int64_t n = (int64_t)P * D * D;
            for (int64_t e = t0; e < n; e += stride) {
                const int d = (int)(e % D), av = (int)((e / D) % D);
                const int64_t p = e / ((int64_t)D * D);
                ws[wl.kp + e] = a.opk[((int64_t)av * P + p) * D + d];
            }
        } else {
            const int64_t n = a.kt == DT_OP_KERNEL_VEC ? (int64_t)P * D : P;
            for (int64_t e = t0; e < n; e += stride) ws[wl.kp + e] = a.opk[e];
        }
    }
}

struct PnnIo {
    const void* idx;
    int kind;
    const floatx4* table;
    const int64_t* row_offset;
    const int32_t* vocab;
    const float* dense;
    float* logit;
    float* out;              // NULL: logits only
    int* oob;                // NULL: not counted
    int sigmoid;
};

// one value -> its three bf16 parts in the chunk buffer (ONE: the leading part is all GEMM1 reads)
template <bool ONE>
__device__ __forceinline__ void pnn_put(__bf16* dst, float v) {
    const __bf16 a = (__bf16)v;
    dst[0] = a;
    if constexpr (!ONE) {
        const float r1 = v - (float)a;
        const __bf16 b = (__bf16)r1;
        dst[kPnnXP] = b;
        dst[2 * kPnnXP] = (__bf16)(r1 - (float)b);
    }
}

template <int D, bool ONE>
__global__ __launch_bounds__(kPnnThreads) void k_pnn_infer(PnnIo io, int64_t B, int F, int Nd, int products, int kt,
                                                          const float* __restrict__ ws) {
    constexpr int KS = D / 4, AT = (D + 15) / 16, LPR = D / 4, LSH = LPR == 1 ? 0 : LPR == 2 ? 1 : LPR == 4 ? 2 : LPR == 8 ? 3 : 4;
    constexpr int HF = kH1 + 4, NSTC = kPnnKC / 32;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n16 = lane & 15, kg = lane >> 4;
    {
        const int* stamp = reinterpret_cast<const int*>(ws);
        if (stamp[0] != pnn_stamp0(F, D, Nd) || stamp[1] != pnn_stamp1(products, kt)) {      // block-uniform: before any barrier
            const float nan = __int_as_float(0x7fc00000);
            for (int64_t r = (int64_t)blockIdx.x * blockDim.x + tid; r < B; r += (int64_t)gridDim.x * blockDim.x) {
                io.logit[r] = nan;
                if (io.out) io.out[r] = nan;
            }
            return;
        }
    }
    const PnnWsLayout wl = pnn_ws_layout(F, D, Nd, products, kt);
    const int FD = F * D, RS = pnn_row_stride(F, D, Nd), P = wl.P, Cp = wl.Cp, K = wl.K, CBP = wl.CBP;
    const bool inner = (products & DT_PNN_INNER) != 0, outer = (products & DT_PNN_OUTER) != 0;
    const bool mat = outer && kt == DT_OP_KERNEL_MAT;
    float* slab = lds;                                                     // [32][RS] the raw rows: embeddings | dense
    float* bnl = slab + kTM * RS;                                          // [3][CBP]
    int* tab = reinterpret_cast<int*>(bnl + 3 * CBP);                      // [P] i | j << 16
    __bf16* xb = reinterpret_cast<__bf16*>(tab + ((P + 3) & ~3));          // [3][32][kPnnXS]
    float* h1f = reinterpret_cast<float*>(xb);                             // [32][HF], after the last chunk
    float* zp = reinterpret_cast<float*>(xb + 3 * kPnnXP);                 // [4][32]
    const float* kpw = ws + wl.kp;

    for (int e = tid; e < 3 * CBP; e += kPnnThreads) bnl[e] = ws[wl.bn + e];
    for (int i = tid; i < F; i += kPnnThreads) {
        const int p0 = i * (2 * F - i - 1) / 2;                            // pairs before row i, itertools.combinations order
        for (int j = i + 1; j < F; ++j) tab[p0 + j - i - 1] = i | (j << 16);
    }
    // the lane's two lookups: field, vocabulary size, first table row — the same for every batch row
    const int NV = F * LPR, c4 = lane & (LPR - 1);
    int fld[2], voc[2];
    int64_t roff[2];
    bool in[2];
    infer_lookup_setup(io.vocab, io.row_offset, lane, NV, LSH, fld, voc, roff, in);

    const int64_t tiles = (B + kTM - 1) / kTM;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t m0 = tile * kTM;
        // ---- gather: wave w takes rows w, w + 8, w + 16, w + 24; unconditional loads from clamped addresses ----
        {
            int id[4][2];
            floatx4 v[4][2];
            float dv[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int64_t m = min(m0 + wave + 8 * q, B - 1);
#pragma unroll
                for (int t = 0; t < 2; ++t)
                    id[q][t] = io.kind == DT_IDX_F32 ? load_id<DT_IDX_F32>(io.idx, m * F + fld[t])
                                                     : load_id<DT_IDX_I32>(io.idx, m * F + fld[t]);
                dv[q] = lane < Nd ? io.dense[m * Nd + lane] : 0.f;
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const bool live = m0 + wave + 8 * q < B;
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    const bool ok = (unsigned)id[q][t] < (unsigned)voc[t];
                    v[q][t] = io.table[(ok ? roff[t] + id[q][t] : (int64_t)0) * LPR + c4];
                    if (!ok || !live) v[q][t] = floatx4{0.f, 0.f, 0.f, 0.f};         // an out-of-range id: the zero row
                    if (c4 == 0 && in[t] && live && !ok && io.oob) atomicAdd(io.oob, 1);     // counted once per lookup
                }
                if (!live) dv[q] = 0.f;
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                float* row = slab + (wave + 8 * q) * RS;
#pragma unroll
                for (int t = 0; t < 2; ++t)
                    if (in[t]) st4(row + 4 * (lane + 64 * t), v[q][t]);
                if (lane < Nd) row[FD + lane] = dv[q];
            }
        }
        lds_barrier();

        // ---- the first Dense over K in chunks: compute the chunk, multiply it ----
        floatx4 c1[2], c2[2], c3[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) { c1[t] = floatx4{0.f, 0.f, 0.f, 0.f}; c2[t] = c1[t]; c3[t] = c1[t]; }
        const __bf16* w1b = reinterpret_cast<const __bf16*>(ws + wl.w1b) + ((int64_t)wave * 64 + lane) * 8;
        const int64_t lo1 = (int64_t)wl.KP * kH1;
        for (int k0 = 0; k0 < wl.KP; k0 += kPnnKC) {
            // the elementwise columns: thread -> (row, column), 64 consecutive columns of a row per wave
            for (int e = tid; e < kTM * kPnnKC; e += kPnnThreads) {
                const int col = e & (kPnnKC - 1), row = e >> 7, k = k0 + col;
                const float* xr = slab + row * RS;
                float val = 0.f;
                if (k < Cp) {
                    const bool is_outer = !inner || k >= P;
                    const int p = k >= P ? k - P : k;
                    if (is_outer && mat) continue;                         // the matrix-core columns below
                    const int pe = tab[p];
                    const float *xi = xr + (pe & 0xffff) * D, *xj = xr + (pe >> 16) * D;
                    if (!is_outer) {
#pragma unroll
                        for (int q = 0; q < D / 4; ++q) {
                            const floatx4 u = ld4(xi + 4 * q), w = ld4(xj + 4 * q);
#pragma unroll
                            for (int r = 0; r < 4; ++r) val += u[r] * w[r];
                        }
                    } else if (kt == DT_OP_KERNEL_VEC) {
#pragma unroll
                        for (int q = 0; q < D / 4; ++q) {
                            const floatx4 u = ld4(xi + 4 * q), w = ld4(xj + 4 * q), kv = ld4(kpw + (int64_t)p * D + 4 * q);
#pragma unroll
                            for (int r = 0; r < 4; ++r) val += (u[r] * w[r]) * kv[r];
                        }
                    } else {
                        const float kv = kpw[p];
#pragma unroll
                        for (int q = 0; q < D / 4; ++q) {
                            const floatx4 u = ld4(xi + 4 * q), w = ld4(xj + 4 * q);
#pragma unroll
                            for (int r = 0; r < 4; ++r) val += (u[r] * w[r]) * kv;
                        }
                    }
                } else if (k < K) {
                    const int c = k - Cp;
                    val = (xr[c] - bnl[c]) * bnl[CBP + c] + bnl[2 * CBP + c];
                }
                pnn_put<ONE>(xb + row * kPnnXS + col, val);
            }
            // the 'mat' columns of the chunk: one wave per pair, both row halves on one K_p
            if (mat) {
                const int first = Cp - P;
                const int lo = max(k0, first), hi = min(k0 + kPnnKC, Cp);
                for (int k = lo + wave; k < hi; k += 8) {
                    const int p = k - first;
                    const int pe = tab[p];
                    const int io_ = (pe & 0xffff) * D, jo = (pe >> 16) * D;
                    float ka[AT][KS];
#pragma unroll
                    for (int t = 0; t < AT; ++t) {
                        const int ar = 16 * t + n16;
                        ld_chunk<KS>(kpw + ((int64_t)p * D + min(ar, D - 1)) * D + kg * KS, ka[t]);
                        if constexpr (D < 16) {
                            if (ar >= D) {
#pragma unroll
                                for (int s = 0; s < KS; ++s) ka[t][s] = 0.f;
                            }
                        }
                    }
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        const float* xr = slab + (16 * h + n16) * RS;
                        float xi[KS];
                        ld_chunk<KS>(xr + io_ + kg * KS, xi);
                        floatx4 acc[AT];
#pragma unroll
                        for (int t = 0; t < AT; ++t) acc[t] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                        for (int s = 0; s < KS; ++s)
#pragma unroll
                            for (int t = 0; t < AT; ++t)
                                acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(ka[t][s], xi[s], acc[t], 0, 0, 0);
                        float sum = 0.f;
#pragma unroll
                        for (int t = 0; t < AT; ++t) {
                            const bool va = 16 * t + 4 * kg < D;
                            const floatx4 xj = ld4(xr + jo + (va ? 16 * t + 4 * kg : 0));
#pragma unroll
                            for (int r = 0; r < 4; ++r) sum += va ? acc[t][r] * xj[r] : 0.f;
                        }
                        sum = row_pair16(sum, false);                      // over the four lane groups: all of a
                        if (kg == 0) pnn_put<ONE>(xb + (16 * h + n16) * kPnnXS + (k - k0), sum);
                    }
                }
            }
            lds_barrier();
            {
                const __bf16* arow0 = xb + n16 * kPnnXS + 8 * kg;
                const __bf16* arow1 = xb + (16 + n16) * kPnnXS + 8 * kg;
                const __bf16* wb = w1b + (int64_t)(k0 >> 5) * 4096;
#pragma unroll
                for (int s = 0; s < NSTC; ++s) {
                    if (k0 + 32 * s >= K) break;                           // beyond the last column: zeros
                    x3_b8 a[2][3], b[3];
#pragma unroll
                    for (int q = 0; q < (ONE ? 1 : 3); ++q) {
                        b[q] = x3_ld8(wb + q * lo1 + (int64_t)s * 4096);
                        a[0][q] = x3_ld8(arow0 + q * kPnnXP + 32 * s);
                        a[1][q] = x3_ld8(arow1 + q * kPnnXP + 32 * s);
                    }
                    infer_mfma6<ONE>(a, b, c1, c2, c3);
                }
            }
            lds_barrier();
        }

        // ---- cell 1's epilogue -> the fp32 H1 tile ----
        infer_cell1(c1, c2, c3, ws + wl.cell1, h1f, wave, n16, kg);
        lds_barrier();

        // ---- GEMM2 (k_infer's): row half mt2, columns [16 nt2, +16); then task_output's vector ----
        {
            const int mt2 = wave & 1, nt2 = wave >> 1;
            const __bf16* w2b = reinterpret_cast<const __bf16*>(ws + wl.w2b);
            const int64_t lo2 = (int64_t)kH1 * kH2;
            floatx4 d1 = {0.f, 0.f, 0.f, 0.f}, d2 = d1, d3 = d1;
            const float* arow = h1f + (16 * mt2 + n16) * HF + 8 * kg;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const __bf16* bp = w2b + (((int64_t)g * 4 + nt2) * 64 + lane) * 8;
                const x3_b8 b0 = x3_ld8(bp), b1 = x3_ld8(bp + lo2), b2 = x3_ld8(bp + 2 * lo2);
                float v[8];
                x3_ld8f(arow + 32 * g, v);
                x3_b8 a1, a2, a3;
                x3_split3(v, a1, a2, a3);
                X3_MFMA(d1, a1, b0);
                X3_LO(d2, a1, b1);
                X3_LO(d3, a1, b2);
                X3_LO(d2, a2, b0);
                X3_LO(d3, a2, b1);
                X3_LO(d3, a3, b0);
            }
            const float* cv2 = ws + wl.cell2;
            const int col = 16 * nt2 + n16;
            const float ctr = cv2[col], scl = cv2[kH2 + col], sft = cv2[2 * kH2 + col], w3v = ws[wl.w3 + col];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float h2 = fmaxf((((d3[r] + d2[r]) + d1[r]) - ctr) * scl + sft, 0.f);
                const float zr = group_sum<16>(h2 * w3v);
                if (n16 == 0) zp[nt2 * kTM + 16 * mt2 + 4 * kg + r] = zr;
            }
        }
        lds_barrier();

        // ---- the output unit: the tower alone, so task_output's kernel was its vector and the output weight is 1 ----
        if (wave == 0 && lane < kTM && m0 + lane < B) {
            const float pt = (zp[lane] + zp[kTM + lane]) + (zp[2 * kTM + lane] + zp[3 * kTM + lane]);
            const float lg = pt * ws[wl.head] + ws[wl.head + 1];
            infer_store(io.logit, io.out, io.sigmoid, m0 + lane, lg);
        }
        // (the next tile's gather writes the slab only; zp is read again two barriers from here)
    }
}

}  // namespace dt

using namespace dt;

static bool pnn_shape_ok(int F, int D, int Nd, int products, int kt) {
    if (F < 2 || F > 64 || Nd < 0 || Nd > 64) return false;
    if (D != 4 && D != 8 && D != 16 && D != 32 && D != 64) return false;
    if (F * D > 512) return false;
    if (products < 1 || products > (DT_PNN_INNER | DT_PNN_OUTER)) return false;
    if ((products & DT_PNN_OUTER) && kt != DT_OP_KERNEL_MAT && kt != DT_OP_KERNEL_VEC && kt != DT_OP_KERNEL_NUM) return false;
    return true;
}
// the kernel type is ignored without an outer layer: one layout, one stamp
static int pnn_kt(int products, int kt) { return (products & DT_PNN_OUTER) ? kt : 0; }

extern "C" int dt_pnn_infer_supported(int F, int D, int Nd, int H1, int H2, int cells, int products, int kernel_type) {
    if (!pnn_shape_ok(F, D, Nd, products, kernel_type)) return 0;
    return (H1 >= 1 && H1 <= kH1 && H2 >= 1 && H2 <= kH2 && (cells & ~3) == 0) ? 1 : 0;
}

extern "C" int64_t dt_pnn_infer_workspace_bytes(int F, int D, int Nd, int products, int kernel_type) {
    if (!pnn_shape_ok(F, D, Nd, products, kernel_type)) return -1;
    return pnn_ws_layout(F, D, Nd, products, pnn_kt(products, kernel_type)).total * (int64_t)sizeof(float);
}

extern "C" int dt_pnn_infer_prepare(int F, int D, int Nd, int products, int kernel_type, const float* op_kernel,
                                    const float* bn_gamma, const float* bn_beta, const float* bn_mean, const float* bn_var,
                                    float bn_eps, const float* W1, int ld1, int H1, const float* b1, const float* W2, int ld2,
                                    int H2, const float* b2, int cells, const float* c1_gamma, const float* c1_beta,
                                    const float* c1_mean, const float* c1_var, float c1_eps, const float* c2_gamma,
                                    const float* c2_beta, const float* c2_mean, const float* c2_var, float c2_eps,
                                    const float* w3, const float* b_out, void* workspace, void* stream) {
    const char* who = "dt_pnn_infer_prepare";
    DT_UNSUPPORTED(!dt_pnn_infer_supported(F, D, Nd, H1, H2, cells, products, kernel_type),
                   "%s: unsupported F=%d D=%d Nd=%d tower %d x %d cells %d products 0x%x kernel_type %d", who, F, D, Nd, H1, H2,
                   cells, products, kernel_type);
    DT_REQUIRE(ld1 >= H1 && ld2 >= H2, "%s: leading dimensions ld1=%d ld2=%d below the widths", who, ld1, ld2);
    DT_REQUIRE(workspace && bn_mean && bn_var && W1 && W2 && w3, "%s: null pointer", who);
    DT_REQUIRE(!(products & DT_PNN_OUTER) == !op_kernel, "%s: products 0x%x and op_kernel %s", who, products,
               op_kernel ? "given" : "null");
    DT_REQUIRE((uintptr_t)workspace % 16 == 0, "%s: workspace must be 16-byte aligned", who);
    PnnPrepArgs a{op_kernel, bn_gamma, bn_beta, bn_mean, bn_var, bn_eps, W1, ld1, H1, W2, ld2, H2,
                  {b1, b2}, {c1_gamma, c2_gamma}, {c1_beta, c2_beta}, {c1_mean, c2_mean}, {c1_var, c2_var},
                  {c1_eps, c2_eps}, w3, b_out, F, D, Nd, products, pnn_kt(products, kernel_type)};
    if (const int rc = infer_check_cells(who, cells, a.cm, a.cv)) return rc;
    const PnnWsLayout wl = pnn_ws_layout(F, D, Nd, products, a.kt);
    const int64_t items = max((int64_t)(wl.KP >> 5) * 512, (int64_t)wl.P * D * D);
    const int blocks = (int)min((items + 255) / 256, (int64_t)2048);
    hipLaunchKernelGGL(k_pnn_infer_prep, dim3(blocks), dim3(256), 0, as_stream(stream), a, static_cast<float*>(workspace));
    return launch_status(who);
}

#define DT_PNN_L(DV)                                                                                                       \
    case DV:                                                                                                               \
        if (one) {                                                                                                         \
            hipFuncSetAttribute((const void*)k_pnn_infer<DV, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);  \
            hipLaunchKernelGGL((k_pnn_infer<DV, true>), dim3(blocks), dim3(kPnnThreads), lds, st, io, B, F, Nd, products, kt, \
                               static_cast<const float*>(workspace));                                                      \
        } else {                                                                                                           \
            hipFuncSetAttribute((const void*)k_pnn_infer<DV, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
            hipLaunchKernelGGL((k_pnn_infer<DV, false>), dim3(blocks), dim3(kPnnThreads), lds, st, io, B, F, Nd, products, kt, \
                               static_cast<const float*>(workspace));                                                      \
        }                                                                                                                  \
        break;

extern "C" int dt_pnn_infer(const void* idx, int idx_kind, const float* table, const int64_t* row_offset, const int32_t* vocab,
                            const float* dense, int64_t B, int F, int D, int Nd, int products, int kernel_type,
                            const void* workspace, float* logit_out, float* out, int* oob_count, int flags, void* stream) {
    const char* who = "dt_pnn_infer";
    DT_UNSUPPORTED(!pnn_shape_ok(F, D, Nd, products, kernel_type), "%s: unsupported F=%d D=%d Nd=%d products 0x%x kernel_type %d",
                   who, F, D, Nd, products, kernel_type);
    DT_REQUIRE(idx_kind == DT_IDX_F32 || idx_kind == DT_IDX_I32, "%s: idx_kind %d", who, idx_kind);
    DT_REQUIRE((flags & ~(DT_INFER_SIGMOID | DT_INFER_TOWER_BF16)) == 0, "%s: flags 0x%x", who, flags);
    DT_REQUIRE(B >= 0 && B < (1LL << 31), "%s: bad batch", who);
    if (B == 0) return DT_OK;
    if (const int rc = infer_check_io(who, idx, table, row_offset, vocab, workspace, logit_out, Nd == 0 || dense)) return rc;
    const size_t lds = pnn_infer_lds(F, D, Nd);
    DT_UNSUPPORTED(lds > 160 * 1024, "%s: the tile needs %zu B of LDS", who, lds);
    const int64_t tiles = (B + kTM - 1) / kTM;
    const int blocks = tiles < DT_PNN_INFER_MAX_BLOCKS ? (int)tiles : DT_PNN_INFER_MAX_BLOCKS;
    const bool one = (flags & DT_INFER_TOWER_BF16) != 0;
    const int kt = pnn_kt(products, kernel_type);
    hipStream_t st = as_stream(stream);
    const PnnIo io{idx, idx_kind, reinterpret_cast<const floatx4*>(table), row_offset, vocab, dense, logit_out, out, oob_count,
                   (flags & DT_INFER_SIGMOID) ? 1 : 0};
    switch (D) { DT_PNN_L(4) DT_PNN_L(8) DT_PNN_L(16) DT_PNN_L(32) DT_PNN_L(64) }
    return launch_status(who);
}
