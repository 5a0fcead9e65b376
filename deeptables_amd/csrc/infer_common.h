// infer_common.h — what the fused inference plans' translation units spell once (infer.hip + infer_x3.h, afm_infer.hip,
// pnn_infer.hip; autoint.hip for the output store): the host-side checks of the entry points, the output store, the
// gather's lookup setup, and GEMM1's six-product step and cell 1's epilogue of the 32-row tower tile.
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

// ---- the tower on a 32-row tile, 512 threads (k_infer, k_pnn_infer): lane = (n16, kg), HF = kH1 + 4 ----

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

}  // namespace dt
