// x3_mfma.h — the split-bf16 ("bf16 x 3") operand primitives of the tile kernels: an fp32 value as two or three bf16 parts,
// 8-element operand loads, and the v_mfma_f32_16x16x32_bf16 product.  Why and how the parts are combined: tower_x3.h.
#pragma once
#include "tile_common.h"

namespace dt {

typedef __bf16 x3_b8 __attribute__((ext_vector_type(8)));
typedef __bf16 x3_b4 __attribute__((ext_vector_type(4)));

// a = h + l (16 mantissa bits) / a = h + m + l (all 24: exact)
__device__ __forceinline__ void x3_split2(const float (&v)[8], x3_b8& h, x3_b8& l) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const __bf16 a = (__bf16)v[e];
        h[e] = a;
        l[e] = (__bf16)(v[e] - (float)a);
    }
}
__device__ __forceinline__ void x3_split3(const float (&v)[8], x3_b8& h, x3_b8& m, x3_b8& l) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const __bf16 a = (__bf16)v[e];
        const float r1 = v[e] - (float)a;
        const __bf16 b = (__bf16)r1;
        h[e] = a; m[e] = b;
        l[e] = (__bf16)(r1 - (float)b);
    }
}
__device__ __forceinline__ x3_b8 x3_ld8(const __bf16* p) { return *reinterpret_cast<const x3_b8*>(p); }
__device__ __forceinline__ void x3_ld8f(const float* p, float (&v)[8]) {
    const floatx4 a = ld4(p), b = ld4(p + 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) { v[e] = a[e]; v[4 + e] = b[e]; }
}
#define X3_MFMA(acc, a, b) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc, 0, 0, 0)
// the lower-order products of a split operand pair: left out in plain-bf16 mode (template ONE, DT_STEP_TOWER_BF16)
#define X3_LO(acc, a, b)        \
    do {                        \
        if constexpr (!ONE) X3_MFMA(acc, a, b); \
    } while (0)

}  // namespace dt
