// fgcnn_infer.hip — fused FGCNN inference (dt_fgcnn_infer*, include/dt_hip.h): the net 'fgcnn_dnn_nets' alone in config.nets
// (deepnets.FGCNN), scored with 2 depth + 1 launches per predict batch after one `prepare` launch per call.
//
// At inference Dropout is the identity, BatchNormalization a per-column affine map, and a row's logit depends on that row
// alone.  Per row, with the F gathered table rows as the channels-last map [F_1 = F][D][C_1 = 1] (deepnets.py:227-261,
// layers.py:161-242), block k = 1 .. depth with (filters, height h, pool p, new filters nf):
//   conv     z[f][d][o] = b[o] + sum_{t < h, c < C_k} map[f + t - (h - 1) / 2][d][c] k[t][c][o]   (zero beyond the map: 'same',
//            the padding split (h - 1) / 2 before, the rest after), tanh
//   pool     over p fields, stride p, 'same' with -inf: Fp = ceil(F_k / p) windows, window i = fields [i p - qb, i p - qb + p)
//            inside the map, qb = (Fp p - F_k) / 2.  tanh is monotone, so the kernel takes the maximum of z and one tanh.
//   recomb   feats_k = tanh(flatten(pooled [Fp][D][filters]) . Wr [Fp D filters][F_k D nf] + br), read as [F_k nf][D]
//   next     map = pooled, F_{k+1} = Fp, C_{k+1} = filters
//   tower input = [feats_1 | .. | feats_depth | the F D raw embedding columns | the Nd RAW dense values]: no input
//   BatchNormalization (bn_concat_emb_dense) is part of this graph.
//
// Launches per batch (all 512 threads):
//   k_fg_conv (one per block)    a block owns TR batch rows: their map goes to LDS (block 1: the table gather of
//       infer_gather_tile, 32 rows; later blocks: the pooled map of the block before from the scratch, channel stride padded
//       to an odd count so that the D lanes of a read hit distinct banks), a thread owns one (row, pooled field, d) and all
//       (<= 16) filters: the h C taps are read from LDS, the kernel — zero-padded to 16 filters by `prepare` — from uniform
//       addresses, plain fp32 FMAs; max over the window, bias, tanhf, stored channels-last.  Neither the taps matrix nor a
//       padded map exists anywhere.
//   k_fg_recomb (one per block)  the heavy GEMM [B][K = Fp D filters] . [K][N = F_k D nf] on the matrix core with the six
//       split-bf16 products of x3_mfma.h (the fp32 class): a block owns 64 rows x 128 columns (grid y = the column chunks),
//       K runs in chunks of 128: the next chunk's rows are in flight from the scratch while this one is split into its three
//       bf16 parts in LDS and multiplied; wave w owns columns [16 w, 16 w + 16) and the four row quarters, the weights come
//       lane-major from the layout `prepare` packed.  Bias, tanhf, stored into the row's feature block of the scratch.
//   k_fg_tower                   k_fibi_infer's shape on a 32-row tile: gather the raw rows and dense values into the slab,
//       the first Dense's K = sum N_k + F D + Nd in chunks of 128 columns — copied from the feature scratch or the slab, never
//       assembled in memory — then cell 1, GEMM2, cell 2, task_output's vector, the bias and the activation (infer_common.h).
// The scratch (pooled maps, features) is the caller's, batch-sized.  The workspace starts with the shape it was prepared
// for; every launch compares it with its own arguments before it reads anything else.
#include "infer_common.h"

namespace dt {

constexpr int kFgThreads = 512;
constexpr int kFgMaxDepth = DT_FGCNN_INFER_MAX_DEPTH;
constexpr int kFgCO = 16;                    // filters the conv kernel is padded to
constexpr int kFgKC = 128;                   // columns of a K chunk = 4 K steps of 32
constexpr int kFgXS = kFgKC + 16;            // bf16 row stride of a chunk buffer
constexpr int kFgXP = kTM * kFgXS;           // one part of the tower's chunk buffer (32 rows)
constexpr int kFgRM = 64;                    // rows of a recombination tile
constexpr int kFgRXP = kFgRM * kFgXS;        // one part of its chunk buffer

struct FgShape {
    int F, D, Nd, depth;
    int filt[kFgMaxDepth], h[kFgMaxDepth], pool[kFgMaxDepth], nf[kFgMaxDepth];
};
struct FgDims {
    int Fin[kFgMaxDepth], Cin[kFgMaxDepth], Fp[kFgMaxDepth], K[kFgMaxDepth], N[kFgMaxDepth];
    int SN, KT, KTP;                         // sum of N, the tower's K and K rounded up to the chunk
};
// entry k of a per-block array by selects: a runtime index would send the whole struct to scratch memory
template <class T>
__host__ __device__ __forceinline__ T fg_at(const T (&a)[kFgMaxDepth], int k) {
    static_assert(kFgMaxDepth == 3, "three selects");
    return k == 0 ? a[0] : k == 1 ? a[1] : a[2];
}
__host__ __device__ inline FgDims fg_dims(const FgShape& s) {
    FgDims d{};
    int F = s.F, C = 1;
#pragma unroll
    for (int k = 0; k < kFgMaxDepth; ++k) {
        if (k >= s.depth) continue;
        d.Fin[k] = F; d.Cin[k] = C;
        d.Fp[k] = (F + s.pool[k] - 1) / s.pool[k];
        d.K[k] = d.Fp[k] * s.D * s.filt[k];
        d.N[k] = F * s.D * s.nf[k];
        d.SN += d.N[k];
        F = d.Fp[k]; C = s.filt[k];
    }
    d.KT = d.SN + s.F * s.D + s.Nd;
    d.KTP = (d.KT + kFgKC - 1) / kFgKC * kFgKC;
    return d;
}

// offsets (floats) inside the workspace dt_fgcnn_infer_prepare writes
struct FgWs {
    int64_t stamp, convw[kFgMaxDepth], convb[kFgMaxDepth], rw[kFgMaxDepth], rb[kFgMaxDepth], w1b, w2b, cell1, cell2, w3, head,
        total;
    int steps[kFgMaxDepth], NC[kFgMaxDepth];  // K steps of 32 and 128-column chunks of a recombination weight
};
__host__ __device__ inline FgWs fg_ws_layout(const FgShape& s, const FgDims& d) {
    FgWs w{};
    int64_t o = 0;
    auto take = [&](int64_t n) { int64_t r = o; o += (n + 3) & ~(int64_t)3; return r; };
    w.stamp = take(8);                                   // what the workspace was prepared for: fg_stamp
#pragma unroll
    for (int k = 0; k < kFgMaxDepth; ++k) {
        if (k >= s.depth) continue;
        w.steps[k] = (d.K[k] + 31) / 32;
        w.NC[k] = (d.N[k] + 127) / 128;
        w.convw[k] = take((int64_t)s.h[k] * d.Cin[k] * kFgCO);      // [h][C][16], zero beyond the filters
        w.convb[k] = take(kFgCO);
        w.rw[k] = take((int64_t)3 * w.NC[k] * w.steps[k] * 4096 / 2);     // 3 bf16 parts of [NC][steps][8 waves][64 lanes][8]
        w.rb[k] = take((int64_t)w.NC[k] * 128);
    }
    w.w1b = take((int64_t)3 * d.KTP * kH1 / 2);          // 3 bf16 parts of [KTP][128], lane-major as k_infer_prep's W1B
    w.w2b = take((int64_t)3 * kH1 * kH2 / 2);
    w.cell1 = take(3 * kH1);                             // tower cell 1: ctr | scl | sft, zero beyond H1
    w.cell2 = take(3 * kH2);
    w.w3 = take(kH2);                                    // task_output's kernel [H2]
    w.head = take(4);                                    // 1, b_out
    w.total = o;
    return w;
}
// The workspace's first eight words name what it was prepared for.  They sit at offset 0 whatever the layout, so a launch
// with another (F, D, Nd, block parameters) sees it before it reads anything else.
__host__ __device__ inline int fg_stamp(const FgShape& s, int i) {
    if (i == 0) return 0x47000000 | s.F | (s.D << 8) | (s.Nd << 16);
    if (i == 1) return 0x43000000 | s.depth;
    const int k = i - 2;
    if (k < s.depth && k < kFgMaxDepth)
        return 0x4E000000 | fg_at(s.filt, k) | (fg_at(s.h, k) << 8) | (fg_at(s.pool, k) << 16) | (fg_at(s.nf, k) << 20);
    return 0;
}
__device__ __forceinline__ bool fg_stamp_ok(const float* ws, const FgShape& s) {
    const int* st = reinterpret_cast<const int*>(ws);
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 2 + kFgMaxDepth; ++i) ok = ok && st[i] == fg_stamp(s, i);
    return ok;
}
__host__ __device__ inline int fg_tower_rs(int F, int D, int Nd) { return F * D + ((Nd + 7) & ~7) + 4; }
inline size_t fg_tower_lds(int F, int D, int Nd) {
    return ((size_t)kTM * fg_tower_rs(F, D, Nd) + 4 * kTM) * sizeof(float) + (size_t)3 * kFgXP * 2;
}

struct FgPrepArgs {
    const float *ck[kFgMaxDepth], *cb[kFgMaxDepth], *rk[kFgMaxDepth], *rbias[kFgMaxDepth];   // per block (a bias may be NULL)
    const float* W1; int ld1, H1;
    const float* W2; int ld2, H2;
    const float *b[2], *cg[2], *cbt[2], *cm[2], *cv[2];      // per tower cell, as InferPrepArgs
    float ceps[2];
    const float *w3, *bout;
    FgShape sh;
};

__device__ __forceinline__ void fg_split_store(const float (&v)[8], __bf16* dst, int64_t lo) {
    x3_b8 h, m, l;
    x3_split3(v, h, m, l);
    *reinterpret_cast<x3_b8*>(dst) = h;
    *reinterpret_cast<x3_b8*>(dst + lo) = m;
    *reinterpret_cast<x3_b8*>(dst + 2 * lo) = l;
}

// one thread per item of every layout; grid-stride.  Every value is read here, at call time.
__global__ __launch_bounds__(256) void k_fg_infer_prep(FgPrepArgs a, float* __restrict__ ws) {
    const FgDims dm = fg_dims(a.sh);
    const FgWs wl = fg_ws_layout(a.sh, dm);
    const int64_t stride = (int64_t)gridDim.x * blockDim.x, t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t0 < 8) reinterpret_cast<int*>(ws)[wl.stamp + t0] = fg_stamp(a.sh, (int)t0);
    if (t0 == 0) {
        ws[wl.head] = 1.f;
        ws[wl.head + 1] = a.bout ? a.bout[0] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < kFgMaxDepth; ++k) {
        if (k >= a.sh.depth) continue;
        const int filt = a.sh.filt[k], hc = a.sh.h[k] * dm.Cin[k], K = dm.K[k], N = dm.N[k], steps = wl.steps[k];
        for (int64_t e = t0; e < (int64_t)hc * kFgCO; e += stride) {
            const int o = (int)(e & (kFgCO - 1)), tc = (int)(e >> 4);
            ws[wl.convw[k] + e] = o < filt ? a.ck[k][(int64_t)tc * filt + o] : 0.f;
        }
        for (int64_t e = t0; e < kFgCO; e += stride) ws[wl.convb[k] + e] = (e < filt && a.cb[k]) ? a.cb[k][e] : 0.f;
        for (int64_t e = t0; e < (int64_t)wl.NC[k] * 128; e += stride) ws[wl.rb[k] + e] = (e < N && a.rbias[k]) ? a.rbias[k][e] : 0.f;
        // lane (n, g) of wave w at step st of column chunk nc holds Wr[32 st + 8 g + j][128 nc + 16 w + n]; zero beyond K / N
        __bf16* rw = reinterpret_cast<__bf16*>(ws + wl.rw[k]);
        const int64_t nv = (int64_t)wl.NC[k] * steps * 512, lo = nv * 8;
        for (int64_t e = t0; e < nv; e += stride) {
            const int l = (int)(e & 63), w = (int)((e >> 6) & 7);
            const int64_t g = e >> 9;
            const int st = (int)(g % steps), nc = (int)(g / steps);
            const int k0 = 32 * st + 8 * (l >> 4), n = 128 * nc + 16 * w + (l & 15);
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = (k0 + j < K && n < N) ? a.rk[k][(int64_t)(k0 + j) * N + n] : 0.f;
            fg_split_store(v, rw + e * 8, lo);
        }
    }
    // the tower's layouts, as k_fibi_infer_prep's
    __bf16* w1b = reinterpret_cast<__bf16*>(ws + wl.w1b);
    __bf16* w2b = reinterpret_cast<__bf16*>(ws + wl.w2b);
    const int64_t n1 = (int64_t)dm.KTP * kH1, n2 = (int64_t)kH1 * kH2;
    const int64_t n1b = (int64_t)(dm.KTP >> 5) * 512;
    for (int64_t e = t0; e < n1b; e += stride) {
        const int l = (int)(e & 63), w = (int)((e >> 6) & 7);
        const int64_t st = e >> 9;
        const int64_t k0 = 32 * st + 8 * (l >> 4);
        const int n = 16 * w + (l & 15);
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = (k0 + j < dm.KT && n < a.H1) ? a.W1[(k0 + j) * a.ld1 + n] : 0.f;
        fg_split_store(v, w1b + e * 8, n1);
    }
    for (int64_t e = t0; e < 1024; e += stride) {
        const int l = (int)(e & 63), t = (int)((e >> 6) & 3), st = (int)(e >> 8);
        const int k0 = 32 * st + 8 * (l >> 4), n = 16 * t + (l & 15);
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = (k0 + j < a.H1 && n < a.H2) ? a.W2[(int64_t)(k0 + j) * a.ld2 + n] : 0.f;
        fg_split_store(v, w2b + e * 8, n2);
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
                sft = a.cbt[cell] ? a.cbt[cell][n] : 0.f;
            } else {
                ctr = -bias; scl = 1.f;
            }
        }
        dst[n] = ctr; dst[W + n] = scl; dst[2 * W + n] = sft;
    }
    for (int64_t e = t0; e < kH2; e += stride) ws[wl.w3 + e] = e < a.H2 ? a.w3[e] : 0.f;
}

struct FgIo {
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

// ---- convolution + max pooling of block k.  LPR > 0: block 1, the map is the gathered table rows (TR = 32, RS = F D + 4,
//      channel stride 1); LPR = 0: the map is `src` [B][Fin D Cin], channel stride CS = Cin | 1, RS = Fin D CS ----
template <int LPR>
__global__ __launch_bounds__(kFgThreads) void k_fg_conv(FgIo io, const float* __restrict__ src, float* __restrict__ dst, int64_t B,
                                                       FgShape sh, int k, int TR, int RS, const float* __restrict__ ws) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    if (!fg_stamp_ok(ws, sh)) return;                    // block-uniform, before any barrier: the tower launch scores NaN
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const FgDims dm = fg_dims(sh);
    const FgWs wl = fg_ws_layout(sh, dm);
    const int D = sh.D, dsh = __ffs(D) - 1, Fin = fg_at(dm.Fin, k), Cin = fg_at(dm.Cin, k), Fp = fg_at(dm.Fp, k),
              filt = fg_at(sh.filt, k), h = fg_at(sh.h, k), pool = fg_at(sh.pool, k);
    const int CS = LPR ? 1 : (Cin | 1), pb = (h - 1) / 2, qb = (Fp * pool - Fin) / 2, FpD = Fp * D, Kout = fg_at(dm.K, k);
    const int msize = Fin * D * Cin;
    const float* cw = ws + fg_at(wl.convw, k);
    const float* cbias = ws + fg_at(wl.convb, k);

    int fld[2], voc[2];
    int64_t roff[2];
    bool in[2];
    const int c4 = LPR ? lane & (LPR - 1) : 0;
    if constexpr (LPR > 0) {
        constexpr int LSH = LPR == 1 ? 0 : LPR == 2 ? 1 : LPR == 4 ? 2 : LPR == 8 ? 3 : 4;
        infer_lookup_setup(io.vocab, io.row_offset, lane, sh.F * LPR, LSH, fld, voc, roff, in);
    }
    const int64_t tiles = (B + TR - 1) / TR;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t m0 = tile * TR;
        if constexpr (LPR > 0) {
            infer_gather_tile<LPR>(io, m0, B, sh.F, 0, sh.F * D, RS, lds, wave, lane, c4, fld, voc, roff, in);
        } else {
            for (int e = tid; e < TR * msize; e += kFgThreads) {
                const int row = e / msize, j = e - row * msize, pos = j / Cin, c = j - pos * Cin;
                lds[row * RS + pos * CS + c] = m0 + row < B ? src[(m0 + row) * (int64_t)msize + j] : 0.f;
            }
        }
        lds_barrier();
        for (int e = tid; e < TR * FpD; e += kFgThreads) {
            const int row = e / FpD, r = e - row * FpD, fp = r >> dsh, d = r & (D - 1);
            if (m0 + row >= B) continue;
            float mx[kFgCO];
#pragma unroll
            for (int o = 0; o < kFgCO; ++o) mx[o] = -INFINITY;
            for (int j = 0; j < pool; ++j) {
                const int f = fp * pool + j - qb;
                const bool okf = (unsigned)f < (unsigned)Fin;
                float acc[kFgCO];
#pragma unroll
                for (int o = 0; o < kFgCO; ++o) acc[o] = 0.f;
                for (int t = 0; t < h; ++t) {
                    const int ff = f + t - pb;
                    const bool ok = okf && (unsigned)ff < (unsigned)Fin;
                    const float* xp = lds + row * RS + (((ok ? ff : 0) << dsh) + d) * CS;
                    const float* wp = cw + t * Cin * kFgCO;
                    for (int c = 0; c < Cin; ++c) {
                        const float x = ok ? xp[c] : 0.f;
#pragma unroll
                        for (int o = 0; o < kFgCO; ++o) acc[o] = fmaf(x, wp[c * kFgCO + o], acc[o]);
                    }
                }
#pragma unroll
                for (int o = 0; o < kFgCO; ++o) mx[o] = okf ? fmaxf(mx[o], acc[o]) : mx[o];
            }
            float* out = dst + (m0 + row) * (int64_t)Kout + (int64_t)r * filt;
#pragma unroll
            for (int o = 0; o < kFgCO; ++o)
                if (o < filt) out[o] = tanhf(mx[o] + cbias[o]);
        }
        lds_barrier();                                   // the next tile's map overwrites this one's
    }
}

// four values -> their three bf16 parts in a chunk buffer whose parts are XP elements apart (dst 8-byte aligned)
template <bool ONE>
__device__ __forceinline__ void fg_put4(__bf16* dst, const floatx4 v, int XP) {
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
        *reinterpret_cast<x3_b4*>(dst + XP) = md;
        *reinterpret_cast<x3_b4*>(dst + 2 * XP) = lo;
    }
}

// ---- recombination Dense of block k: feats[:, foff + n] = tanh(A [B][K] . Wr [K][N] + br), 64 rows x 128 columns per block ----
__global__ __launch_bounds__(kFgThreads) void k_fg_recomb(const float* __restrict__ A, float* __restrict__ feats, int64_t B,
                                                         FgShape sh, int k, const float* __restrict__ ws) {
    constexpr bool ONE = false;
    __shared__ __attribute__((aligned(16))) __bf16 xb[3 * kFgRXP];
    if (!fg_stamp_ok(ws, sh)) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n16 = lane & 15, kg = lane >> 4;
    const FgDims dm = fg_dims(sh);
    const FgWs wl = fg_ws_layout(sh, dm);
    const int K = fg_at(dm.K, k), N = fg_at(dm.N, k), steps = fg_at(wl.steps, k), nc = blockIdx.y;
    const int foff = (k > 0 ? dm.N[0] : 0) + (k > 1 ? dm.N[1] : 0);
    const int64_t lo = (int64_t)fg_at(wl.NC, k) * steps * 4096;
    const __bf16* wb =
        reinterpret_cast<const __bf16*>(ws + fg_at(wl.rw, k)) + (((int64_t)nc * steps) * 512 + wave * 64 + lane) * 8;
    const int col = 128 * nc + 16 * wave + n16;
    const float bv = ws[fg_at(wl.rb, k) + col];          // (zero-padded to the chunk)
    // this thread's four 16-byte pieces of a chunk: rows lr + 16 q, columns 4 lc ..
    const int lr = tid >> 5, lc = tid & 31;

    const int64_t tiles = (B + kFgRM - 1) / kFgRM;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t m0 = tile * kFgRM;
        floatx4 c1[4], c2[4], c3[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) { c1[t] = floatx4{0.f, 0.f, 0.f, 0.f}; c2[t] = c1[t]; c3[t] = c1[t]; }
        floatx4 nx[4];
        auto fetch = [&](int k0) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int64_t m = m0 + lr + 16 * q;
                const int kk = k0 + 4 * lc;
                const bool ok = m < B && kk < K;         // (K is a multiple of 4: a piece is inside or outside)
                nx[q] = ld4(A + (ok ? m * K + kk : (int64_t)0));
                if (!ok) nx[q] = floatx4{0.f, 0.f, 0.f, 0.f};
            }
        };
        fetch(0);
        for (int k0 = 0; k0 < K; k0 += kFgKC) {
#pragma unroll
            for (int q = 0; q < 4; ++q) fg_put4<false>(xb + (lr + 16 * q) * kFgXS + 4 * lc, nx[q], kFgRXP);
            lds_barrier();
            if (k0 + kFgKC < K) fetch(k0 + kFgKC);       // in flight under the products below
            const __bf16* wk = wb + (int64_t)(k0 >> 5) * 4096;
#pragma unroll
            for (int s = 0; s < kFgKC / 32; ++s) {
                if (k0 + 32 * s >= K) break;
                x3_b8 b[3];
#pragma unroll
                for (int q = 0; q < 3; ++q) b[q] = x3_ld8(wk + q * lo + (int64_t)s * 4096);
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const __bf16* ar = xb + (16 * t + n16) * kFgXS + 8 * kg + 32 * s;
                    const x3_b8 a0 = x3_ld8(ar), a1 = x3_ld8(ar + kFgRXP), a2 = x3_ld8(ar + 2 * kFgRXP);
                    X3_MFMA(c1[t], a0, b[0]);
                    X3_LO(c2[t], a0, b[1]);
                    X3_LO(c3[t], a0, b[2]);
                    X3_LO(c2[t], a1, b[0]);
                    X3_LO(c3[t], a1, b[1]);
                    X3_LO(c3[t], a2, b[0]);
                }
            }
            lds_barrier();
        }
        if (col < N) {
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int64_t m = m0 + 16 * t + 4 * kg + r;
                    if (m < B) feats[m * dm.SN + foff + col] = tanhf(((c3[t][r] + c2[t][r]) + c1[t][r]) + bv);
                }
        }
    }
}

// ---- the tower on [feats | raw rows | raw dense], task_output, the activation: k_fibi_infer's shape ----
template <int D, bool ONE>
__global__ __launch_bounds__(kFgThreads) void k_fg_tower(FgIo io, const float* __restrict__ feats, int64_t B, FgShape sh,
                                                        const float* __restrict__ ws) {
    constexpr int LPR = D / 4, LSH = LPR == 1 ? 0 : LPR == 2 ? 1 : LPR == 4 ? 2 : LPR == 8 ? 3 : 4;
    constexpr int NSTC = kFgKC / 32;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n16 = lane & 15, kg = lane >> 4;
    if (!fg_stamp_ok(ws, sh) || sh.D != D) {             // block-uniform: before any barrier
        const float nan = __int_as_float(0x7fc00000);
        for (int64_t r = (int64_t)blockIdx.x * blockDim.x + tid; r < B; r += (int64_t)gridDim.x * blockDim.x) {
            io.logit[r] = nan;
            if (io.out) io.out[r] = nan;
        }
        return;
    }
    const FgDims dm = fg_dims(sh);
    const FgWs wl = fg_ws_layout(sh, dm);
    const int F = sh.F, Nd = sh.Nd, FD = F * D, RS = fg_tower_rs(F, D, Nd), SN = dm.SN, K = dm.KT;
    float* slab = lds;                                                     // [32][RS] the raw rows: embeddings | dense
    __bf16* xb = reinterpret_cast<__bf16*>(slab + kTM * RS);               // [3][32][kFgXS]
    float* h1f = reinterpret_cast<float*>(xb);                             // [32][HF], after the last chunk
    float* zp = reinterpret_cast<float*>(xb + 3 * kFgXP);                  // [4][32]

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

        floatx4 c1[2], c2[2], c3[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) { c1[t] = floatx4{0.f, 0.f, 0.f, 0.f}; c2[t] = c1[t]; c3[t] = c1[t]; }
        const __bf16* w1b = reinterpret_cast<const __bf16*>(ws + wl.w1b) + ((int64_t)wave * 64 + lane) * 8;
        const int64_t lo1 = (int64_t)dm.KTP * kH1;
        for (int k0 = 0; k0 < dm.KTP; k0 += kFgKC) {
            // the chunk: thread -> (row, 4 columns); the generated features from the scratch, the rest from the slab
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int e = tid + kFgThreads * u, row = e >> 5, kk = k0 + 4 * (e & 31);
                floatx4 v = {0.f, 0.f, 0.f, 0.f};
                if (kk < SN) {                           // (SN is a multiple of 4)
                    if (m0 + row < B) v = ld4(feats + (m0 + row) * (int64_t)SN + kk);
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        if (kk + i < K) v[i] = slab[row * RS + (kk + i - SN)];
                }
                fg_put4<ONE>(xb + row * kFgXS + 4 * (e & 31), v, kFgXP);
            }
            lds_barrier();
            {
                const __bf16* arow0 = xb + n16 * kFgXS + 8 * kg;
                const __bf16* arow1 = xb + (16 + n16) * kFgXS + 8 * kg;
                const __bf16* wb = w1b + (int64_t)(k0 >> 5) * 4096;
#pragma unroll
                for (int s = 0; s < NSTC; ++s) {
                    if (k0 + 32 * s >= K) break;                           // beyond the last column: zeros
                    x3_b8 a[2][3], b[3];
#pragma unroll
                    for (int q = 0; q < (ONE ? 1 : 3); ++q) {
                        b[q] = x3_ld8(wb + q * lo1 + (int64_t)s * 4096);
                        a[0][q] = x3_ld8(arow0 + q * kFgXP + 32 * s);
                        a[1][q] = x3_ld8(arow1 + q * kFgXP + 32 * s);
                    }
                    infer_mfma6<ONE>(a, b, c1, c2, c3);
                }
            }
            lds_barrier();
        }

        infer_cell1(c1, c2, c3, ws + wl.cell1, h1f, wave, n16, kg);
        lds_barrier();
        infer_gemm2_w3(h1f, reinterpret_cast<const __bf16*>(ws + wl.w2b), ws + wl.cell2, ws + wl.w3, zp, wave, lane, n16, kg);
        lds_barrier();

        // the output unit: the tower alone, so task_output's kernel was its vector and the output weight is 1
        if (wave == 0 && lane < kTM && m0 + lane < B) {
            const float pt = (zp[lane] + zp[kTM + lane]) + (zp[2 * kTM + lane] + zp[3 * kTM + lane]);
            const float lg = pt * ws[wl.head] + ws[wl.head + 1];
            infer_store(io.logit, io.out, io.sigmoid, m0 + lane, lg);
        }
        lds_barrier();                                   // (the next tile's first chunk overwrites the H1 tile)
    }
}

}  // namespace dt

using namespace dt;

static bool fg_shape(int F, int D, int Nd, int depth, const int* filters, const int* heights, const int* pools,
                     const int* new_filters, FgShape* out) {
    if (F < 2 || F > 64 || Nd < 0 || Nd > 64) return false;
    if (D != 4 && D != 8 && D != 16 && D != 32 && D != 64) return false;
    if (F * D > 512) return false;
    if (depth < 1 || depth > kFgMaxDepth || !filters || !heights || !pools || !new_filters) return false;
    FgShape s{};
    s.F = F; s.D = D; s.Nd = Nd; s.depth = depth;
    for (int k = 0; k < depth; ++k) {
        if (filters[k] < 1 || filters[k] > kFgCO || heights[k] < 1 || heights[k] > 9 || pools[k] < 1 || pools[k] > 3 ||
            new_filters[k] < 1 || new_filters[k] > 3)
            return false;
        s.filt[k] = filters[k]; s.h[k] = heights[k]; s.pool[k] = pools[k]; s.nf[k] = new_filters[k];
    }
    *out = s;
    return true;
}

extern "C" int dt_fgcnn_infer_supported(int F, int D, int Nd, int H1, int H2, int cells, int depth, const int* filters,
                                        const int* heights, const int* pools, const int* new_filters) {
    FgShape s;
    if (!fg_shape(F, D, Nd, depth, filters, heights, pools, new_filters, &s)) return 0;
    return (H1 >= 1 && H1 <= kH1 && H2 >= 1 && H2 <= kH2 && (cells & ~3) == 0) ? 1 : 0;
}

extern "C" int64_t dt_fgcnn_infer_workspace_bytes(int F, int D, int Nd, int depth, const int* filters, const int* heights,
                                                  const int* pools, const int* new_filters) {
    FgShape s;
    if (!fg_shape(F, D, Nd, depth, filters, heights, pools, new_filters, &s)) return -1;
    return fg_ws_layout(s, fg_dims(s)).total * (int64_t)sizeof(float);
}

extern "C" int dt_fgcnn_infer_prepare(int F, int D, int Nd, int depth, const int* filters, const int* heights, const int* pools,
                                      const int* new_filters, const float* const* conv_kernels, const float* const* conv_biases,
                                      const float* const* rec_kernels, const float* const* rec_biases, const float* W1, int ld1,
                                      int H1, const float* b1, const float* W2, int ld2, int H2, const float* b2, int cells,
                                      const float* c1_gamma, const float* c1_beta, const float* c1_mean, const float* c1_var,
                                      float c1_eps, const float* c2_gamma, const float* c2_beta, const float* c2_mean,
                                      const float* c2_var, float c2_eps, const float* w3, const float* b_out, void* workspace,
                                      void* stream) {
    const char* who = "dt_fgcnn_infer_prepare";
    FgShape s;
    DT_UNSUPPORTED(!fg_shape(F, D, Nd, depth, filters, heights, pools, new_filters, &s) ||
                       !dt_fgcnn_infer_supported(F, D, Nd, H1, H2, cells, depth, filters, heights, pools, new_filters),
                   "%s: unsupported F=%d D=%d Nd=%d depth %d tower %d x %d cells %d or block parameters", who, F, D, Nd, depth,
                   H1, H2, cells);
    DT_REQUIRE(ld1 >= H1 && ld2 >= H2, "%s: leading dimensions ld1=%d ld2=%d below the widths", who, ld1, ld2);
    DT_REQUIRE(workspace && conv_kernels && conv_biases && rec_kernels && rec_biases && W1 && W2 && w3, "%s: null pointer", who);
    DT_REQUIRE((uintptr_t)workspace % 16 == 0, "%s: workspace must be 16-byte aligned", who);
    FgPrepArgs a{};
    for (int k = 0; k < depth; ++k) {
        DT_REQUIRE(conv_kernels[k] && rec_kernels[k], "%s: block %d: null kernel", who, k + 1);
        a.ck[k] = conv_kernels[k]; a.cb[k] = conv_biases[k]; a.rk[k] = rec_kernels[k]; a.rbias[k] = rec_biases[k];
    }
    a.W1 = W1; a.ld1 = ld1; a.H1 = H1; a.W2 = W2; a.ld2 = ld2; a.H2 = H2;
    a.b[0] = b1; a.b[1] = b2;
    a.cg[0] = c1_gamma; a.cg[1] = c2_gamma; a.cbt[0] = c1_beta; a.cbt[1] = c2_beta;
    a.cm[0] = c1_mean; a.cm[1] = c2_mean; a.cv[0] = c1_var; a.cv[1] = c2_var;
    a.ceps[0] = c1_eps; a.ceps[1] = c2_eps;
    a.w3 = w3; a.bout = b_out; a.sh = s;
    if (const int rc = infer_check_cells(who, cells, a.cm, a.cv)) return rc;
    const FgDims dm = fg_dims(s);
    const FgWs wl = fg_ws_layout(s, dm);
    int64_t items = (int64_t)(dm.KTP >> 5) * 512;
    for (int k = 0; k < depth; ++k) items = max(items, (int64_t)wl.NC[k] * wl.steps[k] * 512);
    const int blocks = (int)min((items + 255) / 256, (int64_t)2048);
    hipLaunchKernelGGL(k_fg_infer_prep, dim3(blocks), dim3(256), 0, as_stream(stream), a, static_cast<float*>(workspace));
    return launch_status(who);
}

// the checks the three per-batch entry points share; -> DT_OK with *s filled
static int fg_batch_check(const char* who, int64_t B, int F, int D, int Nd, int depth, const int* filters, const int* heights,
                          const int* pools, const int* new_filters, FgShape* s) {
    DT_UNSUPPORTED(!fg_shape(F, D, Nd, depth, filters, heights, pools, new_filters, s),
                   "%s: unsupported F=%d D=%d Nd=%d depth %d or block parameters", who, F, D, Nd, depth);
    DT_REQUIRE(B >= 0 && B < (1LL << 31), "%s: bad batch", who);
    return DT_OK;
}

// rows per conv tile of a later block: the map of TR rows stays within 96 KB of LDS, and TR is the count that leaves the
// fewest threads of the last pass over the (row, pooled field, d) items idle
static int fg_conv_rows(int RS, int FpD) {
    const int most = max(1, min(32, 24576 / RS));
    int best = 1;
    double beff = 0.0;
    for (int tr = 1; tr <= most; ++tr) {
        const int items = tr * FpD;
        const double eff = (double)items / ((items + kFgThreads - 1) / kFgThreads * kFgThreads);
        if (eff >= beff) { beff = eff; best = tr; }
    }
    return best;
}

#define DT_FG_CONV1(LV)                                                                                                     \
    case 4 * LV:                                                                                                            \
        hipFuncSetAttribute((const void*)k_fg_conv<LV>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);              \
        hipLaunchKernelGGL((k_fg_conv<LV>), dim3(blocks), dim3(kFgThreads), lds, st, io, prev, pooled_out, B, s, block, TR, \
                           RS, static_cast<const float*>(workspace));                                                      \
        break;

extern "C" int dt_fgcnn_infer_conv(int block, const void* idx, int idx_kind, const float* table, const int64_t* row_offset,
                                   const int32_t* vocab, const float* prev, int64_t B, int F, int D, int Nd, int depth,
                                   const int* filters, const int* heights, const int* pools, const int* new_filters,
                                   const void* workspace, float* pooled_out, void* stream) {
    const char* who = "dt_fgcnn_infer_conv";
    FgShape s;
    if (const int rc = fg_batch_check(who, B, F, D, Nd, depth, filters, heights, pools, new_filters, &s)) return rc;
    DT_REQUIRE(block >= 0 && block < depth, "%s: block %d of %d", who, block, depth);
    DT_REQUIRE(idx_kind == DT_IDX_F32 || idx_kind == DT_IDX_I32, "%s: idx_kind %d", who, idx_kind);
    if (B == 0) return DT_OK;
    DT_REQUIRE(workspace && pooled_out, "%s: null pointer", who);
    DT_REQUIRE((uintptr_t)workspace % 16 == 0, "%s: workspace must be 16-byte aligned", who);
    const FgDims dm = fg_dims(s);
    hipStream_t st = as_stream(stream);
    const FgIo io{idx, idx_kind, reinterpret_cast<const floatx4*>(table), row_offset, vocab, nullptr, nullptr, nullptr, nullptr, 0};
    if (block == 0) {
        DT_REQUIRE(idx && table && row_offset && vocab, "%s: null pointer", who);
        DT_REQUIRE((uintptr_t)table % 16 == 0, "%s: table must be 16-byte aligned", who);
        const int TR = kTM, RS = F * D + 4;
        const size_t lds = (size_t)TR * RS * sizeof(float);
        const int64_t tiles = (B + TR - 1) / TR;
        const int blocks = tiles < DT_FGCNN_INFER_MAX_BLOCKS ? (int)tiles : DT_FGCNN_INFER_MAX_BLOCKS;
        switch (D) { DT_FG_CONV1(1) DT_FG_CONV1(2) DT_FG_CONV1(4) DT_FG_CONV1(8) DT_FG_CONV1(16) }
    } else {
        DT_REQUIRE(prev, "%s: block %d needs the pooled map of the block before", who, block + 1);
        const int RS = dm.Fin[block] * D * (dm.Cin[block] | 1), TR = fg_conv_rows(RS, dm.Fp[block] * D);
        const size_t lds = (size_t)TR * RS * sizeof(float);
        DT_UNSUPPORTED(lds > 160 * 1024, "%s: the tile needs %zu B of LDS", who, lds);
        const int64_t tiles = (B + TR - 1) / TR;
        const int blocks = tiles < DT_FGCNN_INFER_MAX_BLOCKS ? (int)tiles : DT_FGCNN_INFER_MAX_BLOCKS;
        hipFuncSetAttribute((const void*)k_fg_conv<0>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL((k_fg_conv<0>), dim3(blocks), dim3(kFgThreads), lds, st, io, prev, pooled_out, B, s, block, TR, RS,
                           static_cast<const float*>(workspace));
    }
    return launch_status(who);
}

extern "C" int dt_fgcnn_infer_recomb(int block, const float* pooled, int64_t B, int F, int D, int Nd, int depth,
                                     const int* filters, const int* heights, const int* pools, const int* new_filters,
                                     const void* workspace, float* feats, void* stream) {
    const char* who = "dt_fgcnn_infer_recomb";
    FgShape s;
    if (const int rc = fg_batch_check(who, B, F, D, Nd, depth, filters, heights, pools, new_filters, &s)) return rc;
    DT_REQUIRE(block >= 0 && block < depth, "%s: block %d of %d", who, block, depth);
    if (B == 0) return DT_OK;
    DT_REQUIRE(workspace && pooled && feats, "%s: null pointer", who);
    DT_REQUIRE(((uintptr_t)workspace | (uintptr_t)pooled) % 16 == 0, "%s: workspace / pooled must be 16-byte aligned", who);
    const FgDims dm = fg_dims(s);
    const int64_t tiles = (B + kFgRM - 1) / kFgRM;
    const int blocks = tiles < DT_FGCNN_INFER_MAX_BLOCKS ? (int)tiles : DT_FGCNN_INFER_MAX_BLOCKS;
    hipLaunchKernelGGL(k_fg_recomb, dim3(blocks, (dm.N[block] + 127) / 128), dim3(kFgThreads), 0, as_stream(stream), pooled, feats,
                       B, s, block, static_cast<const float*>(workspace));
    return launch_status(who);
}

#define DT_FG_TOWER(DV)                                                                                                    \
    case DV:                                                                                                               \
        if (one) {                                                                                                         \
            hipFuncSetAttribute((const void*)k_fg_tower<DV, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);  \
            hipLaunchKernelGGL((k_fg_tower<DV, true>), dim3(blocks), dim3(kFgThreads), lds, st, io, feats, B, s,           \
                               static_cast<const float*>(workspace));                                                      \
        } else {                                                                                                           \
            hipFuncSetAttribute((const void*)k_fg_tower<DV, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
            hipLaunchKernelGGL((k_fg_tower<DV, false>), dim3(blocks), dim3(kFgThreads), lds, st, io, feats, B, s,          \
                               static_cast<const float*>(workspace));                                                      \
        }                                                                                                                  \
        break;

extern "C" int dt_fgcnn_infer_tower(const void* idx, int idx_kind, const float* table, const int64_t* row_offset,
                                    const int32_t* vocab, const float* dense, const float* feats, int64_t B, int F, int D, int Nd,
                                    int depth, const int* filters, const int* heights, const int* pools, const int* new_filters,
                                    const void* workspace, float* logit_out, float* out, int* oob_count, int flags, void* stream) {
    const char* who = "dt_fgcnn_infer_tower";
    FgShape s;
    if (const int rc = fg_batch_check(who, B, F, D, Nd, depth, filters, heights, pools, new_filters, &s)) return rc;
    DT_REQUIRE(idx_kind == DT_IDX_F32 || idx_kind == DT_IDX_I32, "%s: idx_kind %d", who, idx_kind);
    DT_REQUIRE((flags & ~(DT_INFER_SIGMOID | DT_INFER_TOWER_BF16)) == 0, "%s: flags 0x%x", who, flags);
    if (B == 0) return DT_OK;
    if (const int rc = infer_check_io(who, idx, table, row_offset, vocab, workspace, logit_out, dense != nullptr || Nd == 0))
        return rc;
    DT_REQUIRE(feats && (uintptr_t)feats % 16 == 0, "%s: feats must be a 16-byte aligned buffer", who);
    const size_t lds = fg_tower_lds(F, D, Nd);
    DT_UNSUPPORTED(lds > 160 * 1024, "%s: the tile needs %zu B of LDS", who, lds);
    const int64_t tiles = (B + kTM - 1) / kTM;
    const int blocks = tiles < DT_FGCNN_INFER_MAX_BLOCKS ? (int)tiles : DT_FGCNN_INFER_MAX_BLOCKS;
    const bool one = (flags & DT_INFER_TOWER_BF16) != 0;
    hipStream_t st = as_stream(stream);
    const FgIo io{idx, idx_kind, reinterpret_cast<const floatx4*>(table), row_offset, vocab, dense, logit_out, out, oob_count,
                  (flags & DT_INFER_SIGMOID) ? 1 : 0};
    switch (D) { DT_FG_TOWER(4) DT_FG_TOWER(8) DT_FG_TOWER(16) DT_FG_TOWER(32) DT_FG_TOWER(64) }
    return launch_status(who);
}
