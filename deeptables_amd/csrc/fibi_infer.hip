// fibi_infer.hip — fused FiBiNet inference (dt_fibi_infer*, include/dt_hip.h): the net 'fibi_dnn_nets' alone in config.nets
// (deepnets.FiBiNet), scored with ONE launch per predict batch after one `prepare` launch per call.
//
// At inference Dropout is the identity, BatchNormalization a per-column affine map, and a row's logit depends on that row
// alone.  Per row, with the F gathered table rows x_i [D] (deepnets.py:344-386):
//   SENET (layers.py:245-308)      z_i = mean | max over D of x_i;  a1 = relu(z K1 + b1) [R];  a2 = relu(a1 K2 + b2) [F]
//   BilinearInteraction (:311-382) over the P = F (F - 1) / 2 pairs p = (i, j), i < j (itertools.combinations order), with
//                                  q = p 'field_interaction' | i 'field_each' | 0 'field_all':
//     senet half  out[p, :] = a2_i a2_j ((x_i . Ws_q) * x_j)      (senet_bilinear_layer on v_i = a2_i x_i: v never exists)
//     raw half    out[P + p, :] = (x_i . Wr_q) * x_j              (embedding_bilinear_layer, its own weights)
//   tower input = [senet half, P D columns pair-major | raw half, P D columns | the Nd RAW dense values]: fibi_dnn_nets
//   concatenates dense_layer itself — no input BatchNormalization (bn_concat_emb_dense) is part of this graph.
//
// A block of 512 threads owns a tile of 32 batch rows and strides over the tiles; the shape is k_pnn_infer's:
//   1. gather (infer_gather_tile): the tile's F table rows and Nd dense values -> the fp32 slab [32][F D + Nd (+ pad)].
//   2. SENET on the vector ALU in plain fp32, once per tile: z and a1 in the (still unused) chunk buffer, a2 [32][F] in LDS.
//   3. the first Dense's K = 2 P D + Nd dimension in chunks of 128 columns = 128 / D blocks of one pair each (P D and 128 are
//      multiples of D, so a block never straddles a chunk or the two halves; a chunk may hold the end of the senet half and
//      the start of the raw half, and the last ones hold the dense columns and zero padding).  A chunk is COMPUTED into the
//      chunk buffer as three bf16 parts [3][32][128 + 16] and multiplied at once: wave w owns hidden units [16 w, 16 w + 16)
//      and both row halves, its 2 x 3 accumulators stay in registers over all chunks.
//        a pair block   one wave per (block, 16-column tile t of it): C^T [a x rows] = W_q^T [a x d] . X_i^T [d x rows], EXACT
//                       fp32 on the matrix core (v_mfma_f32_16x16x4_f32, as k_pnn_infer's 'mat' and k_afm_infer): the lane
//                       that holds row n's U[n][16 t + 4 g .. + 3] multiplies them with x_j[n][16 t + 4 g ..] (one 16-byte LDS
//                       read) and, in the senet half, with a2_i a2_j, and stores four columns.  W_q was transposed by
//                       `prepare`: a wave reads its [16][D] piece once from L2, contiguously, for both row halves.  D = 4 and
//                       D = 8 run the same text on a zero-padded 16-row tile.
//        dense columns  one thread per (row, column), zero beyond K
//      By default the tower's products are the six split-bf16 products of x3_mfma.h (the fp32 class); ONE
//      (DT_INFER_TOWER_BF16) keeps the leading product of GEMM1 only.  SENET and the bilinear products are exact fp32 in
//      both modes.
//   4. cell 1's epilogue, GEMM2, cell 2's epilogue and task_output's vector (infer_common.h), the bias and the activation
//      through infer_store.  The fp32 H1 tile takes the chunk buffer's place in LDS.
// Only the logit (and the activated output) is written.  'field_each' / 'field_all' recompute x_i . W_q per pair: the
// per-field products are not cached, so no LDS is spent on them.
//
// LDS (bytes): slab 128 RS, RS = F D + roundup(Nd, 8) + 4 (4 x odd: 16 rows on 16 distinct bank quads) | a2 128 (F | 1) |
// pair table 4 P | chunk buffer 27,648 | w3 partial sums 512.  F = 26, D = 16, Nd = 13: 89 KB; the most, F = 64, D = 8,
// Nd = 64: 119 KB.  One block per CU at the benchmark shape.
#include "infer_common.h"

namespace dt {

constexpr int kFibiThreads = 512;
constexpr int kFibiKC = 128;                 // columns of a chunk = 4 K steps of 32
constexpr int kFibiXS = kFibiKC + 16;        // bf16 row stride of the chunk buffer (k_infer's CP + 16)
constexpr int kFibiXP = kTM * kFibiXS;       // one part

__host__ __device__ inline int fibi_nw(int F, int bt) {
    return bt == DT_BILINEAR_FIELD_INTERACTION ? F * (F - 1) / 2 : bt == DT_BILINEAR_FIELD_EACH ? F - 1 : 1;
}

// offsets (floats) inside the workspace dt_fibi_infer_prepare writes
struct FibiWsLayout {
    int64_t stamp, w1b, w2b, cell1, cell2, w3, head, k1, b1, k2, b2, wts, wtr, total;
    int P, K, KP;
};
__host__ __device__ inline FibiWsLayout fibi_ws_layout(int F, int D, int Nd, int bt, int R) {
    FibiWsLayout w;
    int64_t o = 0;
    auto take = [&](int64_t n) { int64_t r = o; o += (n + 3) & ~(int64_t)3; return r; };
    w.P = F * (F - 1) / 2;
    w.K = 2 * w.P * D + Nd;
    w.KP = (w.K + kFibiKC - 1) / kFibiKC * kFibiKC;
    const int64_t nwdd = (int64_t)fibi_nw(F, bt) * D * D;
    w.stamp = take(4);                               // what the workspace was prepared for: fibi_stamp0 / fibi_stamp1
    w.w1b = take((int64_t)3 * w.KP * kH1 / 2);       // 3 bf16 parts of [KP][128], lane-major as k_infer_prep's W1B
    w.w2b = take((int64_t)3 * kH1 * kH2 / 2);        // 3 bf16 parts of [128][64], lane-major
    w.cell1 = take(3 * kH1);                         // tower cell 1: ctr | scl | sft, zero beyond H1
    w.cell2 = take(3 * kH2);
    w.w3 = take(kH2);                                // task_output's kernel [H2]
    w.head = take(4);                                // 1, b_out
    w.k1 = take((int64_t)F * R);                     // SENET: att1 kernel [F][R], bias [R]; att2 kernel [R][F], bias [F]
    w.b1 = take(R);
    w.k2 = take((int64_t)R * F);
    w.b2 = take(F);
    w.wts = take(nwdd);                              // senet_bilinear_layer's W, each [D][D] transposed: [q][a][d]
    w.wtr = take(nwdd);                              // embedding_bilinear_layer's
    w.total = o;
    return w;
}
// The workspace's first two words name what it was prepared for.  They sit at offset 0 whatever the layout, so a launch
// with other (F, D, Nd, bilinear_type, R) sees it before it reads anything else and scores every row NaN.
__host__ __device__ inline int fibi_stamp0(int F, int D, int Nd) { return 0x46000000 | F | (D << 8) | (Nd << 16); }
__host__ __device__ inline int fibi_stamp1(int bt, int R) { return 0x42000000 | bt | (R << 4); }
__host__ __device__ inline int fibi_row_stride(int F, int D, int Nd) { return F * D + ((Nd + 7) & ~7) + 4; }
inline size_t fibi_infer_lds(int F, int D, int Nd) {
    const int P4 = (F * (F - 1) / 2 + 3) & ~3;
    return ((size_t)kTM * fibi_row_stride(F, D, Nd) + (size_t)kTM * (F | 1) + P4 + 4 * kTM) * sizeof(float) +
           (size_t)3 * kFibiXP * 2;
}

struct FibiPrepArgs {
    const float *k1, *b1, *k2, *b2;   // SENET's two Dense layers (a bias may be NULL)
    const float *Ws, *Wr;             // the two stacked bilinear W [nW][D][D]
    const float* W1; int ld1, H1;
    const float* W2; int ld2, H2;
    const float *b[2], *cg[2], *cb[2], *cm[2], *cv[2];      // per tower cell, as InferPrepArgs
    float ceps[2];
    const float *w3, *bout;
    int F, D, Nd, bt, R;
};

// one thread per item of every layout; grid-stride.  Every value is read here, at call time.
__global__ __launch_bounds__(256) void k_fibi_infer_prep(FibiPrepArgs a, float* __restrict__ ws) {
    const FibiWsLayout wl = fibi_ws_layout(a.F, a.D, a.Nd, a.bt, a.R);
    const int64_t stride = (int64_t)gridDim.x * blockDim.x, t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t0 == 0) {
        reinterpret_cast<int*>(ws)[wl.stamp] = fibi_stamp0(a.F, a.D, a.Nd);
        reinterpret_cast<int*>(ws)[wl.stamp + 1] = fibi_stamp1(a.bt, a.R);
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
    // are in the chunk order already: senet half, raw half, dense.
    const int64_t n1b = (int64_t)(wl.KP >> 5) * 512;
    for (int64_t e = t0; e < n1b; e += stride) {
        const int l = (int)(e & 63), w = (int)((e >> 6) & 7);
        const int64_t st = e >> 9;
        const int64_t k0 = 32 * st + 8 * (l >> 4);
        const int n = 16 * w + (l & 15);
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = (k0 + j < wl.K && n < a.H1) ? a.W1[(k0 + j) * a.ld1 + n] : 0.f;
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
    const int FR = a.F * a.R;
    for (int64_t e = t0; e < FR; e += stride) { ws[wl.k1 + e] = a.k1[e]; ws[wl.k2 + e] = a.k2[e]; }
    for (int64_t e = t0; e < a.R; e += stride) ws[wl.b1 + e] = a.b1 ? a.b1[e] : 0.f;
    for (int64_t e = t0; e < a.F; e += stride) ws[wl.b2 + e] = a.b2 ? a.b2[e] : 0.f;
    // W [q][d][a] -> W^T [q][a][d]: the A operand's rows are the output columns a
    const int D = a.D;
    const int64_t nw = (int64_t)fibi_nw(a.F, a.bt) * D * D;
    for (int64_t e = t0; e < nw; e += stride) {
        const int d = (int)(e % D), av = (int)((e / D) % D);
        const int64_t q = e / ((int64_t)D * D);
        const int64_t src = (q * D + d) * D + av;
        ws[wl.wts + e] = a.Ws[src];
        ws[wl.wtr + e] = a.Wr[src];
    }
}

struct FibiIo {
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

// values -> their three bf16 parts in the chunk buffer (ONE: the leading part is all GEMM1 reads)
template <bool ONE>
__device__ __forceinline__ void fibi_put(__bf16* dst, float v) {
    const __bf16 a = (__bf16)v;
    dst[0] = a;
    if constexpr (!ONE) {
        const float r1 = v - (float)a;
        const __bf16 b = (__bf16)r1;
        dst[kFibiXP] = b;
        dst[2 * kFibiXP] = (__bf16)(r1 - (float)b);
    }
}
template <bool ONE>
__device__ __forceinline__ void fibi_put4(__bf16* dst, const floatx4 v) {      // dst 8-byte aligned
    x3_b4 h, md, lo;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const __bf16 a = (__bf16)v[e];
        const float r1 = v[e] - (float)a;
        const __bf16 b = (__bf16)r1;
        h[e] = a; md[e] = b; lo[e] = (__bf16)(r1 - (float)b);
    }
    *reinterpret_cast<x3_b4*>(dst) = h;
    if constexpr (!ONE) {
        *reinterpret_cast<x3_b4*>(dst + kFibiXP) = md;
        *reinterpret_cast<x3_b4*>(dst + 2 * kFibiXP) = lo;
    }
}

template <int D, bool ONE>
__global__ __launch_bounds__(kFibiThreads) void k_fibi_infer(FibiIo io, int64_t B, int F, int Nd, int bt, int pool, int R,
                                                            const float* __restrict__ ws) {
    constexpr int KS = D / 4, AT = (D + 15) / 16, LPR = D / 4, LSH = LPR == 1 ? 0 : LPR == 2 ? 1 : LPR == 4 ? 2 : LPR == 8 ? 3 : 4;
    constexpr int NSTC = kFibiKC / 32, NB = kFibiKC / D, NU = NB * AT;     // blocks of a chunk; (block, column tile) units
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n16 = lane & 15, kg = lane >> 4;
    {
        const int* stamp = reinterpret_cast<const int*>(ws);
        if (stamp[0] != fibi_stamp0(F, D, Nd) || stamp[1] != fibi_stamp1(bt, R)) {      // block-uniform: before any barrier
            const float nan = __int_as_float(0x7fc00000);
            for (int64_t r = (int64_t)blockIdx.x * blockDim.x + tid; r < B; r += (int64_t)gridDim.x * blockDim.x) {
                io.logit[r] = nan;
                if (io.out) io.out[r] = nan;
            }
            return;
        }
    }
    const FibiWsLayout wl = fibi_ws_layout(F, D, Nd, bt, R);
    const int FD = F * D, RS = fibi_row_stride(F, D, Nd), P = wl.P, PD2 = 2 * P * D, K = wl.K, FS = F | 1;
    float* slab = lds;                                                     // [32][RS] the raw rows: embeddings | dense
    float* a2l = slab + kTM * RS;                                          // [32][FS] SENET's per-row field weights
    int* tab = reinterpret_cast<int*>(a2l + kTM * FS);                     // [P] i | j << 16
    __bf16* xb = reinterpret_cast<__bf16*>(tab + ((P + 3) & ~3));          // [3][32][kFibiXS]
    float* zl = reinterpret_cast<float*>(xb);                              // [32][F] | a1 [32][R], before the first chunk
    float* a1l = zl + kTM * F;
    float* h1f = reinterpret_cast<float*>(xb);                             // [32][HF], after the last chunk
    float* zp = reinterpret_cast<float*>(xb + 3 * kFibiXP);                // [4][32]
    const float *wts = ws + wl.wts, *wtr = ws + wl.wtr;

    for (int i = tid; i < F; i += kFibiThreads) {
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
        infer_gather_tile<LPR>(io, m0, B, F, Nd, FD, RS, slab, wave, lane, c4, fld, voc, roff, in);
        lds_barrier();

        // ---- SENET, plain fp32: z = pool over D, a1 = relu(z K1 + b1), a2 = relu(a1 K2 + b2) ----
        for (int e = tid; e < kTM * F; e += kFibiThreads) {
            const int row = e / F, f = e - row * F;
            const float* x = slab + row * RS + f * D;
            float z;
            if (pool == DT_FIBI_POOL_MAX) {
                z = x[0];
#pragma unroll
                for (int d = 1; d < D; ++d) z = fmaxf(z, x[d]);
            } else {
                z = 0.f;
#pragma unroll
                for (int d = 0; d < D; ++d) z += x[d];
                z *= 1.0f / D;
            }
            zl[e] = z;
        }
        lds_barrier();
        for (int e = tid; e < kTM * R; e += kFibiThreads) {
            const int row = e / R, r = e - row * R;
            float acc = 0.f;
            for (int f = 0; f < F; ++f) acc += zl[row * F + f] * ws[wl.k1 + f * R + r];
            a1l[e] = fmaxf(acc + ws[wl.b1 + r], 0.f);
        }
        lds_barrier();
        for (int e = tid; e < kTM * F; e += kFibiThreads) {
            const int row = e / F, f = e - row * F;
            float acc = 0.f;
            for (int r = 0; r < R; ++r) acc += a1l[row * R + r] * ws[wl.k2 + r * F + f];
            a2l[row * FS + f] = fmaxf(acc + ws[wl.b2 + f], 0.f);
        }
        lds_barrier();

        // ---- the first Dense over K in chunks: compute the chunk, multiply it ----
        floatx4 c1[2], c2[2], c3[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) { c1[t] = floatx4{0.f, 0.f, 0.f, 0.f}; c2[t] = c1[t]; c3[t] = c1[t]; }
        const __bf16* w1b = reinterpret_cast<const __bf16*>(ws + wl.w1b) + ((int64_t)wave * 64 + lane) * 8;
        const int64_t lo1 = (int64_t)wl.KP * kH1;
        for (int k0 = 0; k0 < wl.KP; k0 += kFibiKC) {
            // the pair blocks of the chunk: one wave per (block, column tile), both row halves on one W_q^T piece
            const int g0 = k0 / D;
            for (int u = wave; u < NU; u += 8) {
                const int b = u / AT, t = u - b * AT, g = g0 + b;
                if (g >= 2 * P) continue;                                  // the dense columns / padding below
                const bool se = g < P;
                const int p = se ? g : g - P;
                const int pe = tab[p];
                const int fi = pe & 0xffff, fj = pe >> 16;
                const int q = bt == DT_BILINEAR_FIELD_INTERACTION ? p : bt == DT_BILINEAR_FIELD_EACH ? fi : 0;
                const int ar = 16 * t + n16;
                float ka[KS];
                ld_chunk<KS>((se ? wts : wtr) + ((int64_t)q * D + min(ar, D - 1)) * D + kg * KS, ka);
                if constexpr (D < 16) {
                    if (ar >= D) {
#pragma unroll
                        for (int s = 0; s < KS; ++s) ka[s] = 0.f;
                    }
                }
                const bool va = 16 * t + 4 * kg < D;                       // (D < 16: the padded tile's rows beyond D)
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int row = 16 * h + n16;
                    const float* xr = slab + row * RS;
                    float xi[KS];
                    ld_chunk<KS>(xr + fi * D + kg * KS, xi);
                    floatx4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int s = 0; s < KS; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(ka[s], xi[s], acc, 0, 0, 0);
                    if (va) {
                        const floatx4 xj = ld4(xr + fj * D + 16 * t + 4 * kg);
                        floatx4 v = acc * xj;
                        if (se) v *= a2l[row * FS + fi] * a2l[row * FS + fj];
                        fibi_put4<ONE>(xb + row * kFibiXS + b * D + 16 * t + 4 * kg, v);
                    }
                }
            }
            // the dense columns and the zero padding behind them: thread -> (row, column)
            if (k0 + kFibiKC > PD2) {
                for (int e = tid; e < kTM * kFibiKC; e += kFibiThreads) {
                    const int col = e & (kFibiKC - 1), row = e >> 7, k = k0 + col;
                    if (k < PD2) continue;
                    fibi_put<ONE>(xb + row * kFibiXS + col, k < K ? slab[row * RS + FD + (k - PD2)] : 0.f);
                }
            }
            lds_barrier();
            {
                const __bf16* arow0 = xb + n16 * kFibiXS + 8 * kg;
                const __bf16* arow1 = xb + (16 + n16) * kFibiXS + 8 * kg;
                const __bf16* wb = w1b + (int64_t)(k0 >> 5) * 4096;
#pragma unroll
                for (int s = 0; s < NSTC; ++s) {
                    if (k0 + 32 * s >= K) break;                           // beyond the last column: zeros
                    x3_b8 a[2][3], b[3];
#pragma unroll
                    for (int q = 0; q < (ONE ? 1 : 3); ++q) {
                        b[q] = x3_ld8(wb + q * lo1 + (int64_t)s * 4096);
                        a[0][q] = x3_ld8(arow0 + q * kFibiXP + 32 * s);
                        a[1][q] = x3_ld8(arow1 + q * kFibiXP + 32 * s);
                    }
                    infer_mfma6<ONE>(a, b, c1, c2, c3);
                }
            }
            lds_barrier();
        }

        // ---- cell 1's epilogue -> the fp32 H1 tile; GEMM2, cell 2's epilogue and task_output's vector ----
        infer_cell1(c1, c2, c3, ws + wl.cell1, h1f, wave, n16, kg);
        lds_barrier();
        infer_gemm2_w3(h1f, reinterpret_cast<const __bf16*>(ws + wl.w2b), ws + wl.cell2, ws + wl.w3, zp, wave, lane, n16, kg);
        lds_barrier();

        // ---- the output unit: the tower alone, so task_output's kernel was its vector and the output weight is 1 ----
        if (wave == 0 && lane < kTM && m0 + lane < B) {
            const float pt = (zp[lane] + zp[kTM + lane]) + (zp[2 * kTM + lane] + zp[3 * kTM + lane]);
            const float lg = pt * ws[wl.head] + ws[wl.head + 1];
            infer_store(io.logit, io.out, io.sigmoid, m0 + lane, lg);
        }
        // (the next tile's gather writes the slab only; z / a1 overwrite the H1 tile one barrier later, zp is read again
        // many barriers from here)
    }
}

}  // namespace dt

using namespace dt;

static bool fibi_shape_ok(int F, int D, int Nd, int bt, int R) {
    if (F < 2 || F > 64 || Nd < 1 || Nd > 64) return false;
    if (D != 4 && D != 8 && D != 16 && D != 32 && D != 64) return false;
    if (F * D > 512) return false;
    if (bt != DT_BILINEAR_FIELD_INTERACTION && bt != DT_BILINEAR_FIELD_EACH && bt != DT_BILINEAR_FIELD_ALL) return false;
    return R >= 1 && R <= 64;              // (SENET's reduction_num = max(F / ratio, 1) <= F)
}
static bool fibi_pool_ok(int pool) { return pool == DT_FIBI_POOL_MEAN || pool == DT_FIBI_POOL_MAX; }

extern "C" int dt_fibi_infer_supported(int F, int D, int Nd, int H1, int H2, int cells, int bilinear_type, int pooling_op, int R) {
    if (!fibi_shape_ok(F, D, Nd, bilinear_type, R) || !fibi_pool_ok(pooling_op)) return 0;
    return (H1 >= 1 && H1 <= kH1 && H2 >= 1 && H2 <= kH2 && (cells & ~3) == 0) ? 1 : 0;
}

extern "C" int64_t dt_fibi_infer_workspace_bytes(int F, int D, int Nd, int bilinear_type, int R) {
    if (!fibi_shape_ok(F, D, Nd, bilinear_type, R)) return -1;
    return fibi_ws_layout(F, D, Nd, bilinear_type, R).total * (int64_t)sizeof(float);
}

extern "C" int dt_fibi_infer_prepare(int F, int D, int Nd, int bilinear_type, int R, const float* se_k1, const float* se_b1,
                                     const float* se_k2, const float* se_b2, const float* W_senet, const float* W_raw,
                                     const float* W1, int ld1, int H1, const float* b1, const float* W2, int ld2, int H2,
                                     const float* b2, int cells, const float* c1_gamma, const float* c1_beta,
                                     const float* c1_mean, const float* c1_var, float c1_eps, const float* c2_gamma,
                                     const float* c2_beta, const float* c2_mean, const float* c2_var, float c2_eps,
                                     const float* w3, const float* b_out, void* workspace, void* stream) {
    const char* who = "dt_fibi_infer_prepare";
    DT_UNSUPPORTED(!dt_fibi_infer_supported(F, D, Nd, H1, H2, cells, bilinear_type, DT_FIBI_POOL_MEAN, R),
                   "%s: unsupported F=%d D=%d Nd=%d tower %d x %d cells %d bilinear_type %d R=%d", who, F, D, Nd, H1, H2, cells,
                   bilinear_type, R);
    DT_REQUIRE(ld1 >= H1 && ld2 >= H2, "%s: leading dimensions ld1=%d ld2=%d below the widths", who, ld1, ld2);
    DT_REQUIRE(workspace && se_k1 && se_k2 && W_senet && W_raw && W1 && W2 && w3, "%s: null pointer", who);
    DT_REQUIRE((uintptr_t)workspace % 16 == 0, "%s: workspace must be 16-byte aligned", who);
    FibiPrepArgs a{se_k1, se_b1, se_k2, se_b2, W_senet, W_raw, W1, ld1, H1, W2, ld2, H2,
                   {b1, b2}, {c1_gamma, c2_gamma}, {c1_beta, c2_beta}, {c1_mean, c2_mean}, {c1_var, c2_var},
                   {c1_eps, c2_eps}, w3, b_out, F, D, Nd, bilinear_type, R};
    if (const int rc = infer_check_cells(who, cells, a.cm, a.cv)) return rc;
    const FibiWsLayout wl = fibi_ws_layout(F, D, Nd, bilinear_type, R);
    const int64_t items = max((int64_t)(wl.KP >> 5) * 512, (int64_t)fibi_nw(F, bilinear_type) * D * D);
    const int blocks = (int)min((items + 255) / 256, (int64_t)2048);
    hipLaunchKernelGGL(k_fibi_infer_prep, dim3(blocks), dim3(256), 0, as_stream(stream), a, static_cast<float*>(workspace));
    return launch_status(who);
}

#define DT_FIBI_L(DV)                                                                                                      \
    case DV:                                                                                                               \
        if (one) {                                                                                                         \
            hipFuncSetAttribute((const void*)k_fibi_infer<DV, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
            hipLaunchKernelGGL((k_fibi_infer<DV, true>), dim3(blocks), dim3(kFibiThreads), lds, st, io, B, F, Nd,          \
                               bilinear_type, pooling_op, R, static_cast<const float*>(workspace));                        \
        } else {                                                                                                           \
            hipFuncSetAttribute((const void*)k_fibi_infer<DV, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
            hipLaunchKernelGGL((k_fibi_infer<DV, false>), dim3(blocks), dim3(kFibiThreads), lds, st, io, B, F, Nd,         \
                               bilinear_type, pooling_op, R, static_cast<const float*>(workspace));                        \
        }                                                                                                                  \
        break;

extern "C" int dt_fibi_infer(const void* idx, int idx_kind, const float* table, const int64_t* row_offset, const int32_t* vocab,
                             const float* dense, int64_t B, int F, int D, int Nd, int bilinear_type, int pooling_op, int R,
                             const void* workspace, float* logit_out, float* out, int* oob_count, int flags, void* stream) {
    const char* who = "dt_fibi_infer";
    DT_UNSUPPORTED(!fibi_shape_ok(F, D, Nd, bilinear_type, R) || !fibi_pool_ok(pooling_op),
                   "%s: unsupported F=%d D=%d Nd=%d bilinear_type %d pooling_op %d R=%d", who, F, D, Nd, bilinear_type,
                   pooling_op, R);
    DT_REQUIRE(idx_kind == DT_IDX_F32 || idx_kind == DT_IDX_I32, "%s: idx_kind %d", who, idx_kind);
    DT_REQUIRE((flags & ~(DT_INFER_SIGMOID | DT_INFER_TOWER_BF16)) == 0, "%s: flags 0x%x", who, flags);
    DT_REQUIRE(B >= 0 && B < (1LL << 31), "%s: bad batch", who);
    if (B == 0) return DT_OK;
    if (const int rc = infer_check_io(who, idx, table, row_offset, vocab, workspace, logit_out, dense != nullptr)) return rc;
    const size_t lds = fibi_infer_lds(F, D, Nd);
    DT_UNSUPPORTED(lds > 160 * 1024, "%s: the tile needs %zu B of LDS", who, lds);
    const int64_t tiles = (B + kTM - 1) / kTM;
    const int blocks = tiles < DT_FIBI_INFER_MAX_BLOCKS ? (int)tiles : DT_FIBI_INFER_MAX_BLOCKS;
    const bool one = (flags & DT_INFER_TOWER_BF16) != 0;
    hipStream_t st = as_stream(stream);
    const FibiIo io{idx, idx_kind, reinterpret_cast<const floatx4*>(table), row_offset, vocab, dense, logit_out, out, oob_count,
                    (flags & DT_INFER_SIGMOID) ? 1 : 0};
    switch (D) { DT_FIBI_L(4) DT_FIBI_L(8) DT_FIBI_L(16) DT_FIBI_L(32) DT_FIBI_L(64) }
    return launch_status(who);
}
