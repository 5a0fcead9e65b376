// infer_x3.h — DeepFM / DCN inference as ONE launch per batch (dt_deepfm_infer / dt_dcn_infer), plus the launch that writes
// the weight layouts it reads (dt_*_infer_prepare).  Included by infer.hip (the host side).
// dt_stack_infer runs the same launches for every subset of {linear, fm_nets, dnn_nets}: k_infer with the absent terms
// compiled out (template NETS) when there is a tower, k_infer_sparse (end of this file; no tile, no LDS) when there is none.
//
// At inference nothing in the graph reaches across the batch (reference deepmodel.py predict / evaluate = keras
// Model.predict): BatchNormalization normalises with its moving statistics (a per-column affine map), Dropout is the
// identity, and a row's logit depends on that row alone.  So the whole forward of a 32-row tile runs in one block:
//   gather + linear + FM (as kernel A, k_sparse_fwd) -> Xn = (X - mm) scale + beta in LDS as three bf16 parts ->
//   GEMM1 (Dense H1, six split-bf16 products, cell epilogue, relu) -> GEMM2 (Dense H2, same) -> w3 -> [DCN: the Cross
//   network's closed form on the same Xn parts] -> the output unit, its activation.
// No batch sums, no election, no atomics (except the optional out-of-range counter), no finishing launch.
//
// Precision: the tower's products are those of k_tower_x3's forward — six split-bf16 products per operand pair (all 24
// mantissa bits, the fp32 class: tests/precision.py CLAIMS gives tower/f32 and tower/bf16x3 the same forward class, so the
// 'f32' mode is served by this path too), or the leading product only (ONE: the 1e-2 'bf16' class).  The Cross network's
// scalars keep their six products in both modes (the logits reach +-160).
//
// The cell epilogue of tower cell i is h = relu((acc - ctr) scl + sft) per column: (-b, 1, 0) for Dense with bias (exactly
// acc + b, as the training tile), (mm - b, gamma / sqrt(mv + eps), beta) for Dense -> BatchNormalization.  The input BN
// keeps its centring the same way, x^ = (x - mm) scale + beta: folded to x scale + shift it would cancel when |mm| >> sigma.
//
// LDS plan (bytes), CP = 64 NCH:  xb  3 * 32 * (CP + 16) * 2   the Xn tile as three bf16 parts (GEMM1 / the Cross P block)
//                                 h1f 32 * (128 + 4) * 4        H1 fp32 (GEMM2's A operand)
//                                 zp  4 * 32 * 4 | lf 32 * 4    the four column tiles' w3 partial sums | linear + FM per row
//                                 DCN: pb 2 * 48 * 16 * 4       the two K halves of P = [Xn ; b_j] . [w_l, w3c]
// CP = 576 (C = 544): 131 KB (DeepFM), 140 KB (DCN) — the split tile serves every C the step's dims accept.
#pragma once
#include "infer_common.h"

namespace dt {

constexpr int kInferThreads = 512;
constexpr int kNetAll = DT_NET_LINEAR | DT_NET_FM | DT_NET_DNN;   // the DeepFM graph; DCN's layouts are those of DT_NET_DNN

// the prepared weights (dt_*_infer_prepare): offsets (floats) inside the inference workspace
struct InferWsLayout {
    int64_t w1b, w2b, bn, cell1, cell2, w3, head, wlin, cwp, total;
};
// nets: the DT_NET_* mask of the graph (DCN, L > 0: a tower and no `linear`, whatever else the mask says) — a region the
// nets do not need takes no space
__host__ __device__ inline InferWsLayout infer_ws_layout(int CP, int L, int nets) {
    InferWsLayout w;
    int64_t o = 0;
    auto take = [&](int64_t n) { int64_t r = o; o += (n + 3) & ~(int64_t)3; return r; };
    const int t = (nets & DT_NET_DNN) ? 1 : 0;     // the tower's regions
    w.w1b = take(t * (int64_t)3 * CP * kH1 / 2);   // 3 bf16 parts of [CP][128], lane-major as X3Weights.W1B
    w.w2b = take(t * (int64_t)3 * kH1 * kH2 / 2);  // 3 bf16 parts of [128][64], lane-major as X3Weights.W2B
    w.bn = take(t * (int64_t)3 * CP);              // input BN: mm | gamma / sqrt(mv + eps) | beta, zero beyond C
    w.cell1 = take(t * (int64_t)3 * kH1);          // tower cell 1: ctr | scl | sft, zero beyond H1
    w.cell2 = take(t * (int64_t)3 * kH2);          // tower cell 2
    w.w3 = take(t * kH2);                          // the tower's output kernel (dense_logit_dnn_nets; task_output's dnn part when
                                                   // the tower is the only net or DCN's)
    w.head = take(4);                              // w_out, b_out
    w.wlin = take((L == 0 && (nets & DT_NET_LINEAR)) ? CP : 0);    // linear_logit's kernel [F + Nd]
    w.cwp = take(L > 0 ? (int64_t)(2 * L + 1) * CP : 0);   // DCN: cross kernels | cross biases | w3c, [2 L + 1][CP], zero beyond C
    w.total = o;
    return w;
}
__host__ __device__ constexpr size_t infer_lds_bytes(int CP, bool dcn) {
    return (size_t)3 * kTM * (CP + 16) * 2 + (size_t)kTM * (kH1 + 4) * 4 + (size_t)(4 * kTM + kTM) * 4 +
           (dcn ? (size_t)2 * 48 * 16 * 4 : 0);
}

struct InferPrepArgs {
    const float *wlin, *gamma, *beta, *mm, *mv;
    float eps;
    const float* W1; int ld1, H1;
    const float* W2; int ld2, H2;
    // per tower cell: Dense bias (NULL: none), BatchNormalization (gamma, beta, moving mean / variance; mm NULL: no BN), eps
    const float *b[2], *cg[2], *cb[2], *cm[2], *cv[2];
    float ceps[2];
    const float *w3, *wout, *bout;    // DCN: w3 = task_output's kernel [C + H2] (cross part first), wout NULL (= 1)
    const float *cw, *cb_;            // DCN: cross kernels / biases [L][C]
    int L;
    int nets;                         // DT_NET_* mask (DCN: DT_NET_DNN): only the regions these nets read are written
};

// one thread per item of every layout; grid-stride
__global__ __launch_bounds__(256) void k_infer_prep(DeepFmDims dm, InferPrepArgs a, float* __restrict__ ws) {
    const InferWsLayout wl = infer_ws_layout(dm.CP, a.L, a.nets);
    const int stride = (int)(gridDim.x * blockDim.x);
    const int t0 = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (t0 == 0) {
        ws[wl.head] = a.wout ? a.wout[0] : 1.f;
        ws[wl.head + 1] = a.bout ? a.bout[0] : 0.f;
    }
    if (a.nets & DT_NET_LINEAR)
        for (int c = t0; c < dm.CP; c += stride) ws[wl.wlin + c] = c < dm.F + dm.Nd ? a.wlin[c] : 0.f;
    if (!(a.nets & DT_NET_DNN)) return;      // no tower: the head and the linear kernel are all k_infer_sparse reads
    __bf16* w1b = reinterpret_cast<__bf16*>(ws + wl.w1b);
    __bf16* w2b = reinterpret_cast<__bf16*>(ws + wl.w2b);
    const int64_t n1 = (int64_t)dm.CP * kH1, n2 = (int64_t)kH1 * kH2;     // elements of one part
    auto split_store = [](const float (&v)[8], __bf16* dst, int64_t lo) {
        x3_b8 h, m, l;
        x3_split3(v, h, m, l);
        *reinterpret_cast<x3_b8*>(dst) = h;
        *reinterpret_cast<x3_b8*>(dst + lo) = m;
        *reinterpret_cast<x3_b8*>(dst + 2 * lo) = l;
    };
    // W1B: lane (n, g) of wave w at step s holds W1[32 s + 8 g + j][16 w + n]; zero beyond C rows / H1 columns
    const int n1b = (dm.CP >> 5) * 512;
    for (int e = t0; e < n1b; e += stride) {
        const int l = e & 63, w = (e >> 6) & 7, st = e >> 9;
        const int k0 = 32 * st + 8 * (l >> 4), n = 16 * w + (l & 15);
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = (k0 + j < dm.C && n < a.H1) ? a.W1[(int64_t)(k0 + j) * a.ld1 + n] : 0.f;
        split_store(v, w1b + (int64_t)e * 8, n1);
    }
    // W2B: lane (n, g) of column tile t at step s holds W2[32 s + 8 g + j][16 t + n]; zero beyond H1 rows / H2 columns
    for (int e = t0; e < 1024; e += stride) {
        const int l = e & 63, t = (e >> 6) & 3, st = e >> 8;
        const int k0 = 32 * st + 8 * (l >> 4), n = 16 * t + (l & 15);
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = (k0 + j < a.H1 && n < a.H2) ? a.W2[(int64_t)(k0 + j) * a.ld2 + n] : 0.f;
        split_store(v, w2b + (int64_t)e * 8, n2);
    }
    // input BatchNormalization over the moving statistics (Keras inference): mm | scale | beta
    for (int c = t0; c < dm.CP; c += stride) {
        float mm = 0.f, sc = 0.f, be = 0.f;
        if (c < dm.C) {
            mm = a.mm[c];
            sc = (a.gamma ? a.gamma[c] : 1.f) * (1.0f / sqrtf(a.mv[c] + a.eps));
            be = a.beta ? a.beta[c] : 0.f;
        }
        ws[wl.bn + c] = mm; ws[wl.bn + dm.CP + c] = sc; ws[wl.bn + 2 * dm.CP + c] = be;
    }
    // the two tower cells' epilogues
    for (int e = t0; e < kH1 + kH2; e += stride) {
        const int cell = e < kH1 ? 0 : 1, n = cell ? e - kH1 : e, W = cell ? kH2 : kH1, H = cell ? a.H2 : a.H1;
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
    for (int e = t0; e < kH2; e += stride) ws[wl.w3 + e] = e < a.H2 ? a.w3[(a.L > 0 ? dm.C : 0) + e] : 0.f;
    if (a.L > 0) {
        const int nv = (2 * a.L + 1) * dm.CP;
        for (int e = t0; e < nv; e += stride) {
            const int v = e / dm.CP, col = e - v * dm.CP;
            const float* src = v < a.L ? a.cw + (int64_t)v * dm.C : v < 2 * a.L ? a.cb_ + (int64_t)(v - a.L) * dm.C : a.w3;
            ws[wl.cwp + e] = col < dm.C ? src[col] : 0.f;
        }
    }
}

struct InferIo {
    const void* idx;
    int kind;
    const float4* table;
    const int64_t* row_offset;
    const int32_t* vocab;
    const float* dense;
    float* logit;
    float* out;              // NULL: logits only
    int* oob;                // NULL: not counted
    int sigmoid;             // out = sigmoid(logit) (binary task), else out = logit (regression)
    // xDeepFM's tower launch (k_infer<.., XD = true>): the tile's raw embedding rows [B][F D / 4] = the CIN's x0, and
    // linear + tower . w3 per row, before the output unit
    float4* x0;
    float* partial;
};

// sum over the lanes that share lane % g (g = D / 4, a power of two, runtime): every lane ends with its group's total
__device__ __forceinline__ float infer_sum_strided(float v, int g) {
    for (int o = 32; o >= g; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// NETS: the nets beside the tower (DT_NET_DNN is always in it) — `linear`'s sum and `fm_nets`' sum-square reduction are
// compiled in per net; a graph without `linear` reads no wlin and runs no wave_sum for it, one without `fm_nets` runs none of
// the eight infer_sum_strided chains.  The logit is (linear + fm + tower) w_out + b_out over the terms present.
// XD (xDeepFM, NETS = DT_NET_LINEAR | DT_NET_DNN): the launch also stores the rows it gathered (before the input BN: the CIN
// reads the concatenated embeddings themselves, deepnets.py:69-81) to io.x0, so the table is gathered once per batch, and
// writes io.partial[m] = linear + tower . w3 instead of running the output unit (k_xdeepfm_head adds the CIN's logit first).
template <int NCH, int LC = 0, bool ONE = false, int NETS = kNetAll, bool XD = false>   // LC = kCrossMax: DCN (NETS unused)
__global__ __launch_bounds__(kInferThreads) void k_infer(InferIo io, DeepFmDims dm, const float* __restrict__ ws, int L) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int CP = 64 * NCH, NST = CP / 32, XSB = CP + 16, HF = kH1 + 4, XP = kTM * XSB;
    constexpr bool LIN = LC == 0 && (NETS & DT_NET_LINEAR), FM = LC == 0 && (NETS & DT_NET_FM);
    const InferWsLayout wl = infer_ws_layout(CP, LC ? L : 0, NETS);      // (DCN: L > 0 leaves no room for `linear`)
    char* base = reinterpret_cast<char*>(lds);
    __bf16* xb = reinterpret_cast<__bf16*>(base);                          // [3][32][XSB]
    float* h1f = reinterpret_cast<float*>(base + (size_t)3 * XP * 2);      // [32][HF]
    float* zp = h1f + kTM * HF;                                            // [4][32]
    float* lf = zp + 4 * kTM;                                              // [32]
    float* pb = lf + kTM;                                                  // DCN: [2][48][16]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n16 = lane & 15, kg = lane >> 4;
    const int m0 = blockIdx.x * kTM;
    const float* bnv = ws + wl.bn;

    // ---- gather: wave w takes rows w, w + 8, w + 16, w + 24 of the tile; linear + FM from the raw rows (kernel A's sums),
    //      then Xn = (X - mm) scale + beta, split into three bf16 parts on the way into LDS ----
    {
        const int LPR = dm.D >> 2, NV = dm.F * LPR, FD = dm.F * dm.D;
        const int c = lane & (LPR - 1);
        for (int rr = wave; rr < kTM; rr += 8) {
            const int m = m0 + rr;
            float4 v[2] = {make_float4(0.f, 0.f, 0.f, 0.f), make_float4(0.f, 0.f, 0.f, 0.f)};
            float lp = 0.f, ts = 0.f;
            if (m < dm.B) {
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    const int j = lane + 64 * t;
                    if (j < NV) {
                        const int f = j / LPR;
                        const int id = io.kind == DT_IDX_F32 ? load_id<DT_IDX_F32>(io.idx, (int64_t)m * dm.F + f)
                                                             : load_id<DT_IDX_I32>(io.idx, (int64_t)m * dm.F + f);
                        if ((unsigned)id < (unsigned)io.vocab[f]) {
                            v[t] = io.table[(io.row_offset[f] + id) * LPR + c];
                        } else if (c == 0 && io.oob) {
                            atomicAdd(io.oob, 1);
                        }
                        if (LIN) lp += ((v[t].x + v[t].y) + (v[t].z + v[t].w)) * ws[wl.wlin + f];
                        if constexpr (XD) io.x0[(int64_t)m * NV + j] = v[t];      // (an out-of-range id: the zero row)
                    }
                }
                if (LIN) {
                    if (lane < dm.Nd) lp += io.dense[(int64_t)m * dm.Nd + lane] * ws[wl.wlin + dm.F + lane];
                }
                if (FM) {
                    float4 S, Q;
                    S.x = infer_sum_strided(v[0].x + v[1].x, LPR); S.y = infer_sum_strided(v[0].y + v[1].y, LPR);
                    S.z = infer_sum_strided(v[0].z + v[1].z, LPR); S.w = infer_sum_strided(v[0].w + v[1].w, LPR);
                    Q.x = infer_sum_strided(v[0].x * v[0].x + v[1].x * v[1].x, LPR);
                    Q.y = infer_sum_strided(v[0].y * v[0].y + v[1].y * v[1].y, LPR);
                    Q.z = infer_sum_strided(v[0].z * v[0].z + v[1].z * v[1].z, LPR);
                    Q.w = infer_sum_strided(v[0].w * v[0].w + v[1].w * v[1].w, LPR);
                    ts = lane < LPR ? ((S.x * S.x - Q.x) + (S.y * S.y - Q.y)) + ((S.z * S.z - Q.z) + (S.w * S.w - Q.w)) : 0.f;
                    ts = wave_sum(ts);
                }
                if (LIN) lp = wave_sum(lp);
            }
            if ((LIN || FM) && lane == 0) lf[rr] = LIN && FM ? lp + 0.5f * ts : LIN ? lp : 0.5f * ts;   // Add([linear, fm, ..]): linear + fm first
            // the row's CP columns in 4-column pieces: embeddings (this lane's gathered pieces), dense columns, zero padding
            for (int q = lane; q < CP / 4; q += 64) {
                floatx4 x = {0.f, 0.f, 0.f, 0.f};
                if (m < dm.B) {
                    if (q < NV) {
                        const float4 s = q < 64 ? v[0] : v[1];
                        x = floatx4{s.x, s.y, s.z, s.w};
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const int k = 4 * q + e - FD;
                            x[e] = k < dm.Nd ? io.dense[(int64_t)m * dm.Nd + k] : 0.f;
                        }
                    }
                }
                const floatx4 xn = (x - ld4(bnv + 4 * q)) * ld4(bnv + CP + 4 * q) + ld4(bnv + 2 * CP + 4 * q);
                x3_b4 h, md, lo;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const __bf16 a = (__bf16)xn[e];
                    const float r1 = xn[e] - (float)a;
                    const __bf16 b = (__bf16)r1;
                    h[e] = a; md[e] = b; lo[e] = (__bf16)(r1 - (float)b);
                }
                __bf16* dst = xb + rr * XSB + 4 * q;
                *reinterpret_cast<x3_b4*>(dst) = h;
                *reinterpret_cast<x3_b4*>(dst + XP) = md;
                *reinterpret_cast<x3_b4*>(dst + 2 * XP) = lo;
            }
        }
    }
    lds_barrier();

    // ---- GEMM1: wave w owns hidden units [16w, 16w+16), both row halves (k_tower_x3's GEMM1 without its backward copies) ----
    {
        floatx4 c1[2], c2[2], c3[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) { c1[t] = floatx4{0.f, 0.f, 0.f, 0.f}; c2[t] = c1[t]; c3[t] = c1[t]; }
        const __bf16* w1b = reinterpret_cast<const __bf16*>(ws + wl.w1b) + ((int64_t)wave * 64 + lane) * 8;
        const int64_t lo1 = (int64_t)CP * kH1;
        const __bf16* arow0 = xb + n16 * XSB + 8 * kg;
        const __bf16* arow1 = xb + (16 + n16) * XSB + 8 * kg;
#pragma unroll
        for (int s = 0; s < NST; ++s) {
            x3_b8 a[2][3], b[3];
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                b[q] = x3_ld8(w1b + q * lo1 + (int64_t)s * 4096);
                a[0][q] = x3_ld8(arow0 + q * XP + 32 * s);
                a[1][q] = x3_ld8(arow1 + q * XP + 32 * s);
            }
            infer_mfma6<ONE>(a, b, c1, c2, c3);
        }
        if constexpr (LC > 0) {
            // ---- Cross, part 1 (k_tower_x3's: P = [Xn ; b_0 .. b_{L-1}] . [w_0 .. w_{L-1} w3c], 48 x 16, K = CP, six products in
            //      both modes).  Waves 0..5: row tile w % 3 (0, 1: the Xn parts in LDS; 2: the bias vectors) x K half w / 3 ----
            if (wave < 6) {
                const float* cwp = ws + wl.cwp;
                const int mt = wave % 3, kh = wave / 3;
                const int s0 = kh * (NST / 2), s1 = kh ? NST : NST / 2;
                const float* brow = cwp + (int64_t)(n16 < L ? n16 : 2 * L) * CP + 8 * kg;
                const float bmask = n16 <= L ? 1.f : 0.f;
                const float* arow2 = cwp + (int64_t)(L + min(n16, L - 1)) * CP + 8 * kg;
                const float amask2 = n16 < L ? 1.f : 0.f;
                floatx4 q1 = {0.f, 0.f, 0.f, 0.f}, q2 = q1, q3 = q1;
                for (int st = s0; st < s1; ++st) {
                    float bv[8];
                    x3_ld8f(brow + 32 * st, bv);
#pragma unroll
                    for (int e = 0; e < 8; ++e) bv[e] *= bmask;
                    x3_b8 b1, b2, b3, a1, a2, a3;
                    x3_split3(bv, b1, b2, b3);
                    if (mt < 2) {
                        const __bf16* ap = xb + (16 * mt + n16) * XSB + 32 * st + 8 * kg;
                        a1 = x3_ld8(ap); a2 = x3_ld8(ap + XP); a3 = x3_ld8(ap + 2 * XP);
                    } else {
                        float av[8];
                        x3_ld8f(arow2 + 32 * st, av);
#pragma unroll
                        for (int e = 0; e < 8; ++e) av[e] *= amask2;
                        x3_split3(av, a1, a2, a3);
                    }
                    X3_MFMA(q3, a1, b3); X3_MFMA(q3, a2, b2); X3_MFMA(q3, a3, b1);
                    X3_MFMA(q2, a1, b2); X3_MFMA(q2, a2, b1);
                    X3_MFMA(q1, a1, b1);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) pb[(kh * 48 + 16 * mt + 4 * kg + r) * 16 + n16] = (q3[r] + q2[r]) + q1[r];
            }
        }
        infer_cell1(c1, c2, c3, ws + wl.cell1, h1f, wave, n16, kg);
    }
    lds_barrier();

    // ---- GEMM2 (six products, A split from the fp32 H1 tile on the fly): row half mt2, columns [16 nt2, +16); then w3 ----
    {
        const int mt2 = wave & 1, nt2 = wave >> 1;
        const __bf16* w2b = reinterpret_cast<const __bf16*>(ws + wl.w2b);
        const int64_t lo2 = (int64_t)kH1 * kH2;
        floatx4 c1 = {0.f, 0.f, 0.f, 0.f}, c2 = c1, c3 = c1;
        const float* arow = h1f + (16 * mt2 + n16) * HF + 8 * kg;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const __bf16* bp = w2b + (((int64_t)g * 4 + nt2) * 64 + lane) * 8;
            const x3_b8 b0 = x3_ld8(bp), b1 = x3_ld8(bp + lo2), b2 = x3_ld8(bp + 2 * lo2);
            float v[8];
            x3_ld8f(arow + 32 * g, v);
            x3_b8 a1, a2, a3;
            x3_split3(v, a1, a2, a3);
            X3_MFMA(c1, a1, b0);
            X3_LO(c2, a1, b1);
            X3_LO(c3, a1, b2);
            X3_LO(c2, a2, b0);
            X3_LO(c3, a2, b1);
            X3_LO(c3, a3, b0);
        }
        const float* cv2 = ws + wl.cell2;
        const int col = 16 * nt2 + n16;
        const float ctr = cv2[col], scl = cv2[kH2 + col], sft = cv2[2 * kH2 + col], w3v = ws[wl.w3 + col];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float h2 = fmaxf((((c3[r] + c2[r]) + c1[r]) - ctr) * scl + sft, 0.f);
            const float zr = group_sum<16>(h2 * w3v);
            if (n16 == 0) zp[nt2 * kTM + 16 * mt2 + 4 * kg + r] = zr;
        }
    }
    lds_barrier();

    // ---- the output unit (wave 0; lanes 32..63 mirror rows 0..31 and write nothing) ----
    if (wave == 0) {
        const int c = lane & 31, s = lane >> 5;
        const int m = m0 + c;
        float zc = 0.f;
        if constexpr (LC > 0) {
            // Cross, part 2 (k_tower_x3's): the L scalar steps of row c, x_l = a_l x0 + c_l:
            //   s_l = a_l p_l + q_l,  a_{l+1} = a_l + s_l,  q_l = (b_0 + .. + b_{l-1}) . Wc_l,  z_c = a_L (x0 . w3c) + c_L . w3c
            float pr[LC + 1], gq[LC][LC + 1];
#pragma unroll
            for (int l = 0; l <= LC; ++l) pr[l] = pb[c * 16 + l] + pb[48 * 16 + c * 16 + l];
#pragma unroll
            for (int j = 0; j < LC; ++j)
#pragma unroll
                for (int l = 0; l <= LC; ++l) gq[j][l] = pb[(32 + j) * 16 + l] + pb[48 * 16 + (32 + j) * 16 + l];
            float a = 1.f;
#pragma unroll
            for (int l = 0; l <= LC; ++l) {
                float q = 0.f;
#pragma unroll
                for (int j = 0; j < LC; ++j)
                    if (j < l) q += gq[j][l];
                if (l < L) a += a * pr[l] + q;
                else if (l == L) zc = a * pr[l] + q;
            }
        }
        if constexpr (XD) {
            if (s == 0 && m < dm.B) {
                const float pt = (zp[c] + zp[kTM + c]) + (zp[2 * kTM + c] + zp[3 * kTM + c]);
                io.partial[m] = LIN ? lf[c] + pt : pt;
            }
            return;
        }
        if (s == 0 && m < dm.B) {
            const float pt = (zp[c] + zp[kTM + c]) + (zp[2 * kTM + c] + zp[3 * kTM + c]);
            const float zz = LC ? zc + pt                      // Dense(1)(Concatenate([cross, dnn])) (deepnets.py:194-207)
                                : (LIN || FM) ? lf[c] + pt     // Add([linear, fm, dnn]) order
                                              : pt;            // the tower alone
            const float lg = zz * ws[wl.head] + ws[wl.head + 1];
            infer_store(io.logit, io.out, io.sigmoid, m, lg);
        }
    }
}

// ---- graphs without a tower (`linear` and / or `fm_nets`): neither bn_concat_emb_dense nor a GEMM is in the graph — both
//      nets read the raw embedding rows — so there is no 32-row tile to build.  One wave = one row, as kernel A
//      (k_sparse_fwd): the row's <= 128 float4 lookups stay in two registers per lane, the sums run over the wave, lane 0
//      writes the logit and the activated output.  No LDS, no barrier.  A gather is two dependent round trips (ids / vocabulary
//      / row offsets, then the table rows) and nothing else happens here, so the kernel lives on occupancy: 256-thread blocks
//      (four rows, one wave per SIMD) with < 64 VGPRs and <= 80 SGPRs are admitted eight to a CU = the CU's 32 waves; B = 8192
//      is 8192 waves = one full residency of 256 CUs, and a block that finishes frees its four slots at once (a 1024-thread
//      block as kernel A's, which needs its 16 rows in LDS for the batch statistics, would hold them until its slowest row).
//      Every load is unconditional from a clamped address and zeroed afterwards, as in kernel A: guarded loads close each
//      slot's region with a full wait. ----
constexpr int kInferSparseRows = 4;

template <int NETS>
__global__ __launch_bounds__(64 * kInferSparseRows) void k_infer_sparse(InferIo io, DeepFmDims dm, const float* __restrict__ ws) {
    constexpr bool LIN = (NETS & DT_NET_LINEAR) != 0, FM = (NETS & DT_NET_FM) != 0;
    const InferWsLayout wl = infer_ws_layout(dm.CP, 0, NETS);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int m = blockIdx.x * kInferSparseRows + wave;
    if (m >= dm.B) return;
    const int LPR = dm.D >> 2, NV = dm.F * LPR, lsh = __ffs(LPR) - 1;
    const int c = lane & (LPR - 1);
    const float wout = ws[wl.head], bout = ws[wl.head + 1];
    int id[2], voc[2], fld[2];
    int64_t roff[2];
    bool in[2], ok[2];
    float wf[2] = {0.f, 0.f};
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int j = lane + 64 * t;
        in[t] = j < NV;
        fld[t] = min(j, NV - 1) >> lsh;
        id[t] = io.kind == DT_IDX_F32 ? load_id<DT_IDX_F32>(io.idx, (int64_t)m * dm.F + fld[t])
                                      : load_id<DT_IDX_I32>(io.idx, (int64_t)m * dm.F + fld[t]);
        voc[t] = io.vocab[fld[t]];
        roff[t] = io.row_offset[fld[t]];
        if (LIN) wf[t] = ws[wl.wlin + fld[t]];
    }
    float dv = 0.f, wd = 0.f;      // the continuous columns' share of `linear`: lane k < Nd takes column k
    if (LIN && lane < dm.Nd) {
        dv = io.dense[(int64_t)m * dm.Nd + lane];
        wd = ws[wl.wlin + dm.F + lane];
    }
    float4 v[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        ok[t] = in[t] && (unsigned)id[t] < (unsigned)voc[t];
        v[t] = io.table[(ok[t] ? roff[t] + id[t] : (int64_t)0) * LPR + c];
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        if (!ok[t]) v[t] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (c == 0 && in[t] && !ok[t] && io.oob) atomicAdd(io.oob, 1);     // counted once per lookup, as in k_infer
    }
    float lp = 0.f, ts = 0.f;
    if (LIN) {          // k_infer's order: the two lookups, then the continuous column
#pragma unroll
        for (int t = 0; t < 2; ++t)
            if (in[t]) lp += ((v[t].x + v[t].y) + (v[t].z + v[t].w)) * wf[t];
        lp += dv * wd;
        lp = wave_sum(lp);
    }
    if (FM) {           // 0.5 sum_d ((sum_f e)^2 - sum_f e^2), k_infer's sums
        float4 S, Q;
        S.x = infer_sum_strided(v[0].x + v[1].x, LPR); S.y = infer_sum_strided(v[0].y + v[1].y, LPR);
        S.z = infer_sum_strided(v[0].z + v[1].z, LPR); S.w = infer_sum_strided(v[0].w + v[1].w, LPR);
        Q.x = infer_sum_strided(v[0].x * v[0].x + v[1].x * v[1].x, LPR);
        Q.y = infer_sum_strided(v[0].y * v[0].y + v[1].y * v[1].y, LPR);
        Q.z = infer_sum_strided(v[0].z * v[0].z + v[1].z * v[1].z, LPR);
        Q.w = infer_sum_strided(v[0].w * v[0].w + v[1].w * v[1].w, LPR);
        ts = lane < LPR ? ((S.x * S.x - Q.x) + (S.y * S.y - Q.y)) + ((S.z * S.z - Q.z) + (S.w * S.w - Q.w)) : 0.f;
        ts = wave_sum(ts);
    }
    if (lane == 0) {
        const float zz = LIN && FM ? lp + 0.5f * ts : LIN ? lp : 0.5f * ts;     // Add([linear, fm]) / the single net
        const float lg = zz * wout + bout;
        infer_store(io.logit, io.out, io.sigmoid, m, lg);
    }
}

// ---- xDeepFM's head (reference layers.py:713-734 + deepmodel.py:286-301): what split-pool, cat, the exFM_out Dense, add_logits,
//      task_output and the activation do in eight launches.  Of every CIN layer's output y_k [B][L_k][D] only sum_D of the
//      direct-connect channels [lo_k, L_k) is used (lo_k = 0 with direct=True and for the last layer, else L_k / 2), and that
//      only through its dot product with exFM_out's kernel: logit_cin = sum_k sum_l wex[off_k + l - lo_k] sum_d y_k[b][l][d] + bex.
//      Tens of megabytes of y and no flops, so one wave = one row: the row's pooled channels of a layer are one contiguous
//      run of (L_k - lo_k) D floats that the wave reads as float4s, lane after lane (64 lanes x 16 B = 1 KiB per instruction),
//      four loads in flight per lane; every lane weighs its piece's four-term sum with the channel's weight, wave_sum ends the
//      row.  The order of the sums depends on the row alone, not on B.  256-thread blocks (four rows), no LDS. ----
constexpr int kXdMaxLayers = DT_XDEEPFM_MAX_LAYERS;
constexpr int kXdHeadRows = 4;

struct XdHeadArgs {
    const float* y[kXdMaxLayers];
    int L[kXdMaxLayers], lo[kXdMaxLayers], woff[kXdMaxLayers];     // channels, first pooled channel, its weight's offset in wex
    int n;
    const float* wex;            // [sum_k (L_k - lo_k)] exFM_out's kernel | 1 float bias (prepared workspace)
    const float* bex;
    const float* head;           // w_out, b_out (InferWsLayout.head)
    const float* partial;        // [B] linear + tower
    float* logit;
    float* out;
    int sigmoid;
    int B, D;
};

__global__ __launch_bounds__(64 * kXdHeadRows) void k_xdeepfm_head(XdHeadArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int m = blockIdx.x * kXdHeadRows + wave;
    if (m >= a.B) return;
    const int lsh = __ffs(a.D >> 2) - 1;                 // float4 pieces per channel = D / 4, a power of two
    float acc = 0.f;
    for (int k = 0; k < a.n; ++k) {
        const int n4 = (a.L[k] - a.lo[k]) << lsh;        // float4 pieces of the pooled run
        const float4* src = reinterpret_cast<const float4*>(a.y[k] + ((int64_t)m * a.L[k] + a.lo[k]) * a.D);
        const float* w = a.wex + a.woff[k];
        int q = lane;
        for (; q + 192 < n4; q += 256) {
            const float4 v0 = src[q], v1 = src[q + 64], v2 = src[q + 128], v3 = src[q + 192];
            const float w0 = w[q >> lsh], w1 = w[(q + 64) >> lsh], w2 = w[(q + 128) >> lsh], w3 = w[(q + 192) >> lsh];
            acc += ((v0.x + v0.y) + (v0.z + v0.w)) * w0;
            acc += ((v1.x + v1.y) + (v1.z + v1.w)) * w1;
            acc += ((v2.x + v2.y) + (v2.z + v2.w)) * w2;
            acc += ((v3.x + v3.y) + (v3.z + v3.w)) * w3;
        }
        for (; q < n4; q += 64) {
            const float4 v0 = src[q];
            acc += ((v0.x + v0.y) + (v0.z + v0.w)) * w[q >> lsh];
        }
    }
    acc = wave_sum(acc);
    if (lane == 0) {
        const float zz = a.partial[m] + (acc + a.bex[0]);       // Add([linear, cin, dnn]) over the two terms the launches hand over
        const float lg = zz * a.head[0] + a.head[1];
        infer_store(a.logit, a.out, a.sigmoid, m, lg);
    }
}

// one thread per element of exFM_out's kernel and bias -> the workspace (dt_xdeepfm_infer_prepare)
__global__ __launch_bounds__(256) void k_xdeepfm_prep(const float* __restrict__ wex, const float* __restrict__ bex, int P,
                                                      float* __restrict__ dst) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e < P) dst[e] = wex[e];
    else if (e == P) dst[((P + 3) & ~3)] = bex ? bex[0] : 0.f;
}

}  // namespace dt
