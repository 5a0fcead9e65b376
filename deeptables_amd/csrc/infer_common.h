// infer_common.h — what the fused inference plans' translation units spell once (infer.hip + infer_x3.h, afm_infer.hip,
// pnn_infer.hip, fibi_infer.hip; autoint.hip for the output store): the host-side checks of the entry points, the output
// store, the gather's lookup setup and the 32-row tile's gather, and GEMM1's six-product step, cell 1's epilogue and GEMM2
// with cell 2's epilogue of the 32-row tower tile.
// Every device function is __forceinline__: no function symbol is added to the device code.
#pragma once
#include "x3_mfma.h"

namespace dt {

// ---- host: checks the entry points share ----

// `prepare`: a tower cell with batch norm (bit i of `cells`) needs its moving statistics; one without reads none
inline int infer_check_cells(const char* who, int cells, const float* (&cm)[2], const float* (&cv)[2]) {
    for (int i = 0; i < 2; ++i) {
        if (cells & (1 << i)) {
            DT_REQUIRE(cm[i] && cv[i], "%s: tower cell %d has batch norm but no moving statistics", who, i + 1);
        } else {
            cm[i] = nullptr;
        }
    }
    return DT_OK;
}

// the per-batch entry points, after their own idx_kind / flags / B checks: pointers, dense, alignment — in this order
inline int infer_check_io(const char* who, const void* idx, const float* table, const int64_t* row_offset,
                          const int32_t* vocab, const void* workspace, const float* logit_out, bool dense_ok) {
    DT_REQUIRE(idx && table && row_offset && vocab && workspace && logit_out, "%s: null pointer", who);
    DT_REQUIRE(dense_ok, "%s: dense is null", who);
    DT_REQUIRE(((uintptr_t)table | (uintptr_t)workspace) % 16 == 0, "%s: table / workspace must be 16-byte aligned", who);
    return DT_OK;
}

// row m's logit and, where asked for (out != NULL), its activation
__device__ __forceinline__ void infer_store(float* logit, float* out, int sigmoid, int64_t m, float lg) {
    logit[m] = lg;
    if (out) out[m] = sigmoid ? 1.0f / (1.0f + expf(-lg)) : lg;
}

// ---- the gather: a lane's two lookups of a row's NV = F D / 4 float4 pieces (j = lane + 64 t; 1 << lsh pieces per field) —
//      field, vocabulary size and first table row are the same for every batch row.  A lane beyond NV reads the last
//      field's (clamped address) and is masked by in[t]. ----
__device__ __forceinline__ void infer_lookup_setup(const int32_t* vocab, const int64_t* row_offset, int lane, int NV, int lsh,
                                                   int (&fld)[2], int (&voc)[2], int64_t (&roff)[2], bool (&in)[2]) {
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int j = lane + 64 * t;
        in[t] = j < NV;
        fld[t] = min(j, NV - 1) >> lsh;
        voc[t] = vocab[fld[t]];
        roff[t] = row_offset[fld[t]];
    }
}

// the gather of a 32-row tile into an fp32 slab [32][RS] in LDS (k_pnn_infer, k_fibi_infer; 512 threads): wave w takes rows
// w, w + 8, w + 16, w + 24 and has their ids, then their table rows, in flight together; unconditional loads from clamped
// addresses.  A row's F D embedding columns are followed by its Nd dense values; a row beyond B is all zeros.  An
// out-of-range id reads the zero row and is counted once per lookup.  IO: the kernel's argument block (idx, kind, table as
// floatx4, dense, oob).
template <int LPR, class IO>
__device__ __forceinline__ void infer_gather_tile(const IO& io, int64_t m0, int64_t B, int F, int Nd, int FD, int RS, float* slab,
                                                  int wave, int lane, int c4, const int (&fld)[2], const int (&voc)[2],
                                                  const int64_t (&roff)[2], const bool (&in)[2]) {
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

// ---- the tower on a 32-row tile, 512 threads (k_infer, k_pnn_infer, k_fibi_infer): lane = (n16, kg), HF = kH1 + 4 ----

// GEMM1, one K step of 32: the six split-bf16 products (ONE: the leading one) of the two row halves a[t][part] with the
// wave's 16 hidden units b[part] into the three accumulator classes
template <bool ONE>
__device__ __forceinline__ void infer_mfma6(const x3_b8 (&a)[2][3], const x3_b8 (&b)[3], floatx4 (&c1)[2], floatx4 (&c2)[2],
                                            floatx4 (&c3)[2]) {
    X3_MFMA(c1[0], a[0][0], b[0]); X3_MFMA(c1[1], a[1][0], b[0]);
    X3_LO(c2[0], a[0][0], b[1]); X3_LO(c2[1], a[1][0], b[1]);
    X3_LO(c3[0], a[0][0], b[2]); X3_LO(c3[1], a[1][0], b[2]);
    X3_LO(c2[0], a[0][1], b[0]); X3_LO(c2[1], a[1][1], b[0]);
    X3_LO(c3[0], a[0][1], b[1]); X3_LO(c3[1], a[1][1], b[1]);
    X3_LO(c3[0], a[0][2], b[0]); X3_LO(c3[1], a[1][2], b[0]);
}

// cell 1's epilogue (cv1: ctr | scl | sft): H1 in the C layout (column 16 wave + n16, rows 16 t + 4 kg + r) -> fp32 in LDS
__device__ __forceinline__ void infer_cell1(const floatx4 (&c1)[2], const floatx4 (&c2)[2], const floatx4 (&c3)[2],
                                            const float* cv1, float* h1f, int wave, int n16, int kg) {
    constexpr int HF = kH1 + 4;
    const int col = 16 * wave + n16;
    const float ctr = cv1[col], scl = cv1[kH1 + col], sft = cv1[2 * kH1 + col];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r)
            h1f[(16 * t + 4 * kg + r) * HF + col] = fmaxf((((c3[t][r] + c2[t][r]) + c1[t][r]) - ctr) * scl + sft, 0.f);
}

// GEMM2 (k_infer's: six products, A split from the fp32 H1 tile on the fly), cell 2's epilogue (cv2: ctr | scl | sft) and the
// tower's output vector w3: wave -> row half mt2 = wave & 1, columns [16 nt2, +16), nt2 = wave >> 1; the four column tiles'
// partial sums of h2 . w3 per row -> zp [4][32].  w2b: the three bf16 parts of [128][64], lane-major.
__device__ __forceinline__ void infer_gemm2_w3(const float* h1f, const __bf16* w2b, const float* cv2, const float* w3,
                                               float* zp, int wave, int lane, int n16, int kg) {
    constexpr int HF = kH1 + 4;
    constexpr bool ONE = false;              // (X3_LO: GEMM2 keeps its six products in every mode, as k_infer's)
    const int mt2 = wave & 1, nt2 = wave >> 1;
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
    const int col = 16 * nt2 + n16;
    const float ctr = cv2[col], scl = cv2[kH2 + col], sft = cv2[2 * kH2 + col], w3v = w3[col];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const float h2 = fmaxf((((d3[r] + d2[r]) + d1[r]) - ctr) * scl + sft, 0.f);
        const float zr = group_sum<16>(h2 * w3v);
        if (n16 == 0) zp[nt2 * kTM + 16 * mt2 + 4 * kg + r] = zr;
    }
}

}  // namespace dt
