// afm_infer.hip — fused AFM inference (dt_afm_infer*, include/dt_hip.h): nets 'afm_nets' alone or Add-stacked with 'linear'
// and / or 'fm_nets' scored with ONE launch per predict batch, after one `prepare` launch per call.
//
// At inference Dropout is the identity and a row's logit depends on that row alone.  AFM.call (layers.py:786-807) per row, over
// the P = F (F - 1) / 2 pairs p = (i, j), i < j:
//   bi_p = x_i * x_j            a_p = act(bi_p Wa + ba)            l_p = a_p . h            out = (sum_p softmax(l)_p bi_p) . w_do
// dense_out is linear and has no bias, so with t_p = bi_p . w_do the output is sum_p softmax(l)_p t_p: the pooled [D] vector
// is never formed.  One pass over the pairs keeps a running max m, s = sum e^(l_p - m) and a = sum e^(l_p - m) t_p (online
// softmax) and divides once — no [P] score buffer, no second pass.
//
// One wave = one batch row (as k_infer_sparse, infer_x3.h, whose gather this is: ids decoded as DT_IDX_*, unconditional
// loads from clamped addresses, an out-of-range id reads a zero row and is counted).  The row's <= 128 float4 lookups arrive
// in two registers per lane; `linear` and `fm_nets` are formed from them behind the compile-time net mask, then they go to
// the wave's LDS slab [F][D + 4] so that any lane can read any field.
//
// The attention product on the matrix core, EXACT fp32 (v_mfma_f32_16x16x4_f32; the path dense.hip takes): per tile of 16
// pairs C^T [HP x 16] = Wa^T [HP x D] . bi^T [D x 16], i.e. the A operand is the attention kernel (rows = hidden units, held
// in registers for the wave's whole life) and the B operand the tile's pair products (columns = pairs), so the lane that
// formed pair n's products also receives pair n's activations: lane (n = lane & 15, g = lane >> 4)
//   B, k-step s:   bi[n][d = g D/4 + s]     (the k order is the same permutation for A and B: a contiguous D/4 chunk per lane
//   A, k-step s:   Wa[d = g D/4 + s][16 t + n]                 group, so x_i / x_j are read 16 bytes at a time)
//   C, register r: pre-activation of hidden unit 16 t + 4 g + r of pair n   (the accumulator starts at ba)
// l_p and t_p are then sums over the lane's registers and over the four lane groups (two permlane swaps each).  Every lane
// group keeps the same 16 running softmax states (one per n); the 16 meet once per row.
// The pairs' (i, j) come from a table `prepare` wrote (slab offsets, 4 bytes per pair, copied to LDS once per block),
// padded to a multiple of 16 with pairs that are masked out of the softmax.
//
// Launch: blocks of DT_AFM_INFER_ROWS = 4 waves (one per SIMD), at most DT_AFM_INFER_MAX_BLOCKS = 1024 = 4 per CU, so a
// SIMD holds 4 waves: enough to cover the 40-cycle dependent-accumulator latency of the fp32 MFMA (issue 32) and the gather.
// A wave strides over the rows with the table rows of its next row and the ids of the one after in flight.
// LDS (bytes) = 4 (P16 + 4 F (D + 4)): F = 26, D = 16: 9,664; the most, F = 128, D = 4: 48,896.  Registers: DESIGN.md §3.1b.
#include "infer_common.h"

namespace dt {

constexpr int kAfmRows = DT_AFM_INFER_ROWS;
constexpr int kAfmPad = 4;                  // floats between the slab's rows: D + 4 keeps 16 consecutive fields on 16 slots
constexpr float kAfmNeg = -3.0e38f;         // a masked pair's logit; the running max starts here

// offsets (floats) inside the workspace dt_afm_infer_prepare writes; HP = the compiled attention width (16 / 32 / 64)
struct AfmWsLayout {
    int stamp, wa, ba, hv, wdo, head, wlin, tab, total;
    int P, P16;
};
__host__ __device__ inline AfmWsLayout afm_ws_layout(int F, int D, int Nd, int HP, int nets) {
    AfmWsLayout w;
    int o = 0;
    auto take = [&](int n) { int r = o; o += (n + 3) & ~3; return r; };
    w.P = F * (F - 1) / 2;
    w.P16 = (w.P + 15) & ~15;
    w.stamp = take(4);                                       // what the workspace was prepared for: afm_stamp0 / afm_stamp1
    w.wa = take(D * HP);                                     // Wa [D][HP], zero beyond H
    w.ba = take(HP);                                         // ba [HP]
    w.hv = take(HP);                                         // projection_h [HP]
    w.wdo = take(D);                                         // afm_layer_dense_out's kernel [D]
    w.head = take(4);                                        // w_out, b_out
    w.wlin = take((nets & DT_NET_LINEAR) ? F + Nd : 0);      // linear_logit's kernel [F + Nd]
    w.tab = take(w.P16);                                     // per pair: (i S) | (j S) << 16, S = D + 4; zero beyond P
    w.total = o;
    return w;
}
// The workspace's first two words name the shape and nets it was prepared for.  They sit at offset 0 whatever the layout,
// so a launch whose (F, D, Nd, H, nets) are not the prepared ones sees it before it reads anything else — and scores every
// row NaN instead of reading weights from where another layout put them.
__host__ __device__ inline int afm_stamp0(int F, int D, int HP) { return 0x41000000 | F | (D << 8) | (HP << 16); }
__host__ __device__ inline int afm_stamp1(int Nd, int nets) { return 0x46000000 | nets | (Nd << 8); }
inline int afm_hp(int H) { return H <= 16 ? 16 : (H <= 32 ? 32 : 64); }
inline size_t afm_infer_lds(int F, int D) {
    return ((size_t)((F * (F - 1) / 2 + 15) & ~15) + (size_t)kAfmRows * F * (D + kAfmPad)) * sizeof(float);
}
static bool afm_nets_ok(int nets) { return (nets & DT_NET_AFM) && (nets & ~(DT_NET_AFM | DT_NET_LINEAR | DT_NET_FM)) == 0; }

struct AfmPrepArgs {
    const float *Wa, *ba, *h, *wdo, *wlin, *wout, *bout;
    int F, D, Nd, H, HP, nets;
};

// one thread per item of every region; grid-stride.  Every value is read here, at call time.
__global__ __launch_bounds__(256) void k_afm_infer_prep(AfmPrepArgs a, float* __restrict__ ws) {
    const AfmWsLayout wl = afm_ws_layout(a.F, a.D, a.Nd, a.HP, a.nets);
    const int stride = (int)(gridDim.x * blockDim.x), t0 = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (t0 == 0) {
        reinterpret_cast<int*>(ws)[wl.stamp] = afm_stamp0(a.F, a.D, a.HP);
        reinterpret_cast<int*>(ws)[wl.stamp + 1] = afm_stamp1(a.Nd, a.nets);
        ws[wl.head] = a.wout[0];
        ws[wl.head + 1] = a.bout ? a.bout[0] : 0.f;
    }
    for (int e = t0; e < a.D * a.HP; e += stride) {
        const int d = e / a.HP, h = e - d * a.HP;
        ws[wl.wa + e] = h < a.H ? a.Wa[d * a.H + h] : 0.f;
    }
    for (int e = t0; e < a.HP; e += stride) {
        ws[wl.ba + e] = (a.ba && e < a.H) ? a.ba[e] : 0.f;
        ws[wl.hv + e] = e < a.H ? a.h[e] : 0.f;
    }
    for (int e = t0; e < a.D; e += stride) ws[wl.wdo + e] = a.wdo[e];
    if (a.nets & DT_NET_LINEAR)
        for (int e = t0; e < a.F + a.Nd; e += stride) ws[wl.wlin + e] = a.wlin[e];
    int* tab = reinterpret_cast<int*>(ws + wl.tab);
    const int S = a.D + kAfmPad;
    for (int i = t0; i < a.F; i += stride) {
        const int p0 = i * (2 * a.F - i - 1) / 2;            // pairs before row i, itertools.combinations order
        for (int j = i + 1; j < a.F; ++j) tab[p0 + j - i - 1] = (i * S) | ((j * S) << 16);
    }
    for (int e = wl.P + t0; e < wl.P16; e += stride) tab[e] = 0;
}

struct AfmIo {
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

__device__ __forceinline__ void afm_fence() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

template <int D, int HT, int NETS>
__global__ __launch_bounds__(64 * kAfmRows) void k_afm_infer(AfmIo io, int B, int F, int Nd, int act,
                                                            const float* __restrict__ ws) {
    constexpr bool LIN = (NETS & DT_NET_LINEAR) != 0, FM = (NETS & DT_NET_FM) != 0;
    constexpr int KS = D / 4, HP = 16 * HT, S = D + kAfmPad;
    constexpr int LPR = D / 4, LSH = LPR == 1 ? 0 : LPR == 2 ? 1 : LPR == 4 ? 2 : LPR == 8 ? 3 : 4;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const AfmWsLayout wl = afm_ws_layout(F, D, Nd, HP, NETS);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = lane & 15, g = lane >> 4;
    {
        const int* stamp = reinterpret_cast<const int*>(ws);
        if (stamp[0] != afm_stamp0(F, D, HP) || stamp[1] != afm_stamp1(Nd, NETS)) {       // block-uniform: before the barrier
            const float nan = __int_as_float(0x7fc00000);
            for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < B; r += (int64_t)gridDim.x * blockDim.x) {
                io.logit[r] = nan;
                if (io.out) io.out[r] = nan;
            }
            return;
        }
    }
    int* tab = reinterpret_cast<int*>(lds);
    float* slab = lds + wl.P16 + wave * F * S;
    {
        const int* src = reinterpret_cast<const int*>(ws + wl.tab);
        for (int e = threadIdx.x; e < wl.P16; e += blockDim.x) tab[e] = src[e];
    }
    // the lane's share of the attention weights, for every row it scores
    float wa[KS][HT], wdo[KS];
    floatx4 bav[HT], hvv[HT];
#pragma unroll
    for (int s = 0; s < KS; ++s) {
        wdo[s] = ws[wl.wdo + g * KS + s];
#pragma unroll
        for (int t = 0; t < HT; ++t) wa[s][t] = ws[wl.wa + (g * KS + s) * HP + 16 * t + n];
    }
#pragma unroll
    for (int t = 0; t < HT; ++t) {
        bav[t] = ld4(ws + wl.ba + 16 * t + 4 * g);
        hvv[t] = ld4(ws + wl.hv + 16 * t + 4 * g);
    }
    const float wout = ws[wl.head], bout = ws[wl.head + 1];
    const bool simple = act == DT_ACT_LINEAR || act == DT_ACT_RELU;
    const float lo = act == DT_ACT_RELU ? 0.f : -INFINITY;
    // the lane's two lookups: field, vocabulary size, first table row, `linear` weight — the same for every batch row
    const int NV = F * LPR, c = lane & (LPR - 1);
    int fld[2], voc[2];
    int64_t roff[2];
    bool in[2];
    float wf[2] = {0.f, 0.f};
    infer_lookup_setup(io.vocab, io.row_offset, lane, NV, LSH, fld, voc, roff, in);
#pragma unroll
    for (int t = 0; t < 2; ++t)
        if (LIN) wf[t] = ws[wl.wlin + fld[t]];
    const bool has_dense = LIN && lane < Nd;       // the continuous columns' share of `linear`: lane k < Nd takes column k
    const float wd = has_dense ? ws[wl.wlin + F + lane] : 0.f;
    __syncthreads();                               // the pair table; the only barrier: nothing below reads another wave's data

    auto load_ids = [&](int64_t row, int (&id)[2]) {
#pragma unroll
        for (int t = 0; t < 2; ++t)
            id[t] = io.kind == DT_IDX_F32 ? load_id<DT_IDX_F32>(io.idx, row * F + fld[t])
                                          : load_id<DT_IDX_I32>(io.idx, row * F + fld[t]);
    };
    auto gather = [&](int64_t row, const int (&id)[2], floatx4 (&v)[2], unsigned& ok, float& dv) {
        ok = 0;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const bool o = in[t] && (unsigned)id[t] < (unsigned)voc[t];
            ok |= (o ? 1u : 0u) << t;
            v[t] = io.table[(o ? roff[t] + id[t] : (int64_t)0) * LPR + c];
            if (c == 0 && in[t] && !o && io.oob) atomicAdd(io.oob, 1);       // counted once per lookup
        }
        dv = has_dense ? io.dense[row * Nd + lane] : 0.f;
    };

    const int64_t nw = (int64_t)gridDim.x * kAfmRows;
    int64_t b = (int64_t)blockIdx.x * kAfmRows + wave;
    floatx4 v[2], vn[2];
    unsigned okc = 0, okn = 0;
    float dv = 0.f, dvn = 0.f;
    int idn[2] = {0, 0};
    if (b < B) {
        int id0[2];
        load_ids(b, id0);
        gather(b, id0, v, okc, dv);
    }
    if (b + nw < B) load_ids(b + nw, idn);
    const int tiles = wl.P16 >> 4;
    for (; b < B; b += nw) {
        // the chain is ids -> table rows, so two rows are in flight behind the one being scored
        const bool more = b + nw < B;
        if (more) gather(b + nw, idn, vn, okn, dvn);
        if (b + 2 * nw < B) load_ids(b + 2 * nw, idn);
#pragma unroll
        for (int t = 0; t < 2; ++t)
            if (!((okc >> t) & 1u)) v[t] = floatx4{0.f, 0.f, 0.f, 0.f};     // an out-of-range id: the zero row
        float lp = 0.f, ts = 0.f;
        if (LIN) {          // k_infer_sparse's order: the two lookups, then the continuous column
#pragma unroll
            for (int t = 0; t < 2; ++t)
                if (in[t]) lp += ((v[t].x + v[t].y) + (v[t].z + v[t].w)) * wf[t];
            lp += dv * wd;
            lp = wave_sum(lp);
        }
        if (FM) {           // 0.5 sum_d ((sum_f e)^2 - sum_f e^2), k_infer_sparse's sums
            floatx4 Sv, Qv;
            Sv.x = wave_sum_strided<LPR>(v[0].x + v[1].x); Sv.y = wave_sum_strided<LPR>(v[0].y + v[1].y);
            Sv.z = wave_sum_strided<LPR>(v[0].z + v[1].z); Sv.w = wave_sum_strided<LPR>(v[0].w + v[1].w);
            Qv.x = wave_sum_strided<LPR>(v[0].x * v[0].x + v[1].x * v[1].x);
            Qv.y = wave_sum_strided<LPR>(v[0].y * v[0].y + v[1].y * v[1].y);
            Qv.z = wave_sum_strided<LPR>(v[0].z * v[0].z + v[1].z * v[1].z);
            Qv.w = wave_sum_strided<LPR>(v[0].w * v[0].w + v[1].w * v[1].w);
            ts = lane < LPR ? ((Sv.x * Sv.x - Qv.x) + (Sv.y * Sv.y - Qv.y)) + ((Sv.z * Sv.z - Qv.z) + (Sv.w * Sv.w - Qv.w)) : 0.f;
            ts = wave_sum(ts);
        }
        afm_fence();                                // the previous row's slab reads are done
#pragma unroll
        for (int t = 0; t < 2; ++t)
            if (in[t]) st4(slab + fld[t] * S + 4 * c, v[t]);
        afm_fence();
        float m = kAfmNeg, sm = 0.f, am = 0.f;      // the running softmax of the pairs 16 k + n
        for (int tile = 0; tile < tiles; ++tile) {
            const int p = 16 * tile + n;
            const int e = tab[p];
            const bool valid = p < wl.P;
            float xi[KS], xj[KS], bi[KS];
            ld_chunk<KS>(slab + (e & 0xffff) + g * KS, xi);
            ld_chunk<KS>(slab + (e >> 16) + g * KS, xj);
            floatx4 acc[HT];
#pragma unroll
            for (int t = 0; t < HT; ++t) acc[t] = bav[t];
            float tp = 0.f;
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                bi[s] = xi[s] * xj[s];
                tp += bi[s] * wdo[s];
#pragma unroll
                for (int t = 0; t < HT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[s][t], bi[s], acc[t], 0, 0, 0);
            }
            float lg = 0.f;
            if (simple) {
#pragma unroll
                for (int t = 0; t < HT; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r) lg += fmaxf(acc[t][r], lo) * hvv[t][r];
            } else {
#pragma unroll
                for (int t = 0; t < HT; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r) lg += act_apply(acc[t][r], act) * hvv[t][r];
            }
            lg = row_pair16(lg, false);             // over the four lane groups: all hidden units / all of D
            tp = row_pair16(tp, false);
            // online softmax: one of e^(m - m') and e^(l - m') is 1
            const float l = valid ? lg : kAfmNeg;
            const float d = l - m;
            const float x = expf(-fabsf(d));
            if (d > 0.f) {
                sm = sm * x + 1.f;
                am = am * x + tp;
                m = l;
            } else {
                sm += valid ? x : 0.f;
                am += valid ? x * tp : 0.f;
            }
        }
        // the 16 states meet (every lane group holds the same 16: the sums are 4 x, which the quotient does not see)
        const float M = wave_max(m);
        const float f = expf(m - M);
        const float sT = wave_sum(sm * f), aT = wave_sum(am * f);
        if (lane == 0) {
            float zz = aT / sT;
            if (LIN) zz += lp;
            if (FM) zz += 0.5f * ts;
            const float lgt = zz * wout + bout;
            infer_store(io.logit, io.out, io.sigmoid, b, lgt);
        }
        if (more) {
            v[0] = vn[0]; v[1] = vn[1];
            okc = okn;
            dv = dvn;
        }
    }
}

}  // namespace dt

using namespace dt;

extern "C" int dt_afm_infer_supported(int F, int D, int Nd, int H, int act, int nets) {
    DeepFmDims dm; int lpr;
    if (F < 2 || H < 1 || H > 64 || act < 0 || act >= DT_ACT_COUNT || !afm_nets_ok(nets)) return 0;
    return deepfm_dims(1, F, D, Nd, &dm, &lpr) ? 1 : 0;
}

extern "C" int64_t dt_afm_infer_workspace_bytes(int F, int D, int Nd, int H, int nets) {
    if (!dt_afm_infer_supported(F, D, Nd, H, DT_ACT_RELU, nets)) return -1;
    return (int64_t)afm_ws_layout(F, D, Nd, afm_hp(H), nets).total * (int64_t)sizeof(float);
}

extern "C" int dt_afm_infer_prepare(int F, int D, int Nd, int H, int nets, const float* Wa, const float* ba, const float* h,
                                    const float* w_do, const float* w_lin, const float* w_out, const float* b_out,
                                    void* workspace, void* stream) {
    DT_UNSUPPORTED(!dt_afm_infer_supported(F, D, Nd, H, DT_ACT_RELU, nets),
                   "dt_afm_infer_prepare: unsupported F=%d D=%d Nd=%d H=%d nets=0x%x", F, D, Nd, H, nets);
    DT_REQUIRE(Wa && h && w_do && w_out && workspace, "dt_afm_infer_prepare: null pointer (Wa, h, w_do, w_out, workspace)");
    DT_REQUIRE(!(nets & DT_NET_LINEAR) == !w_lin, "dt_afm_infer_prepare: nets 0x%x and w_lin %s", nets, w_lin ? "given" : "null");
    DT_REQUIRE((uintptr_t)workspace % 16 == 0, "dt_afm_infer_prepare: workspace must be 16-byte aligned");
    const AfmPrepArgs a{Wa, ba, h, w_do, w_lin, w_out, b_out, F, D, Nd, H, afm_hp(H), nets};
    const int items = max(max(D * a.HP, F + Nd), 16);
    hipLaunchKernelGGL(k_afm_infer_prep, dim3(ceil_div(items, 256)), dim3(256), 0, as_stream(stream), a,
                       static_cast<float*>(workspace));
    return launch_status("dt_afm_infer_prepare");
}

#define DT_AFM_L(DV, HTV, NV)                                                                                         \
    hipLaunchKernelGGL((k_afm_infer<DV, HTV, NV>), dim3(blocks), dim3(64 * kAfmRows), lds, st, io, (int)B, F, Nd, act, \
                       static_cast<const float*>(workspace))
#define DT_AFM_N(DV, HTV)                                                           \
    switch (nets & (DT_NET_LINEAR | DT_NET_FM)) {                                   \
        case 0: DT_AFM_L(DV, HTV, DT_NET_AFM); break;                               \
        case DT_NET_LINEAR: DT_AFM_L(DV, HTV, DT_NET_AFM | DT_NET_LINEAR); break;   \
        case DT_NET_FM: DT_AFM_L(DV, HTV, DT_NET_AFM | DT_NET_FM); break;           \
        default: DT_AFM_L(DV, HTV, DT_NET_AFM | DT_NET_LINEAR | DT_NET_FM); break;  \
    }
#define DT_AFM_H(DV)                              \
    case DV:                                      \
        if (H <= 16) { DT_AFM_N(DV, 1) }          \
        else if (H <= 32) { DT_AFM_N(DV, 2) }     \
        else { DT_AFM_N(DV, 4) }                  \
        break;

extern "C" int dt_afm_infer(const void* idx, int idx_kind, const float* table, const int64_t* row_offset,
                            const int32_t* vocab, const float* dense, int64_t B, int F, int D, int Nd, int H, int nets, int act,
                            const void* workspace, float* logit_out, float* out, int* oob_count, int flags, void* stream) {
    DT_UNSUPPORTED(!dt_afm_infer_supported(F, D, Nd, H, act, nets),
                   "dt_afm_infer: unsupported F=%d D=%d Nd=%d H=%d act=%d nets=0x%x", F, D, Nd, H, act, nets);
    DT_REQUIRE(idx_kind == DT_IDX_F32 || idx_kind == DT_IDX_I32, "dt_afm_infer: idx_kind %d", idx_kind);
    DT_REQUIRE((flags & ~DT_INFER_SIGMOID) == 0, "dt_afm_infer: flags %#x (DT_INFER_SIGMOID or 0)", flags);
    if (B == 0) return DT_OK;
    DT_REQUIRE(B > 0 && B < (1LL << 31), "dt_afm_infer: bad batch");
    if (const int rc = infer_check_io("dt_afm_infer", idx, table, row_offset, vocab, workspace, logit_out,
                                      !(nets & DT_NET_LINEAR) || Nd == 0 || dense)) return rc;
    const size_t lds = afm_infer_lds(F, D);
    DT_UNSUPPORTED(lds > 64 * 1024, "dt_afm_infer: needs %zu B of LDS", lds);
    const int64_t want = (B + kAfmRows - 1) / kAfmRows;
    const int blocks = want < DT_AFM_INFER_MAX_BLOCKS ? (int)want : DT_AFM_INFER_MAX_BLOCKS;
    hipStream_t st = as_stream(stream);
    const AfmIo io{idx, idx_kind, reinterpret_cast<const floatx4*>(table), row_offset, vocab, dense, logit_out, out, oob_count,
                   (flags & DT_INFER_SIGMOID) ? 1 : 0};
    switch (D) { DT_AFM_H(4) DT_AFM_H(8) DT_AFM_H(16) DT_AFM_H(32) DT_AFM_H(64) }
    return launch_status("dt_afm_infer");
}
