// tile_common.h — what the fused train step (deepfm.hip, tower_x3.h) and the fused inference plans (infer.hip, infer_x3.h)
// share: the step's shape, the tower's fixed sizes, the 16-byte vector helpers, the phase stamps, the sharded batch sums
// and the argument blocks of the tile kernels.
#pragma once
#include "common.h"

namespace dt {

typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef float floatx4 __attribute__((ext_vector_type(4)));

constexpr int kH1 = 128;  // dnn_params hidden_units[0]
constexpr int kH2 = 64;   // dnn_params hidden_units[1]
constexpr int kTM = 32;   // rows per MLP tile

struct DeepFmDims {
    int B, F, D, Nd, C, CP;  // C = F*D+Nd; CP = C rounded up to 64: row stride of X and the padded GEMM K
};
constexpr int kMaxC = 544;       // the largest C deepfm_dims accepts
constexpr int kCrossMax = 8;    // cross layers the fused DCN step takes

__device__ __forceinline__ floatx4 ld4(const float* p) { return *reinterpret_cast<const floatx4*>(p); }
__device__ __forceinline__ void st4(float* p, floatx4 v) { *reinterpret_cast<floatx4*>(p) = v; }
// KS consecutive floats (16-byte aligned for KS >= 4, 8-byte for KS = 2)
template <int KS>
__device__ __forceinline__ void ld_chunk(const float* p, float (&o)[KS]) {
    if constexpr (KS >= 4) {
#pragma unroll
        for (int q = 0; q < KS / 4; ++q) {
            const floatx4 v = ld4(p + 4 * q);
            o[4 * q] = v.x; o[4 * q + 1] = v.y; o[4 * q + 2] = v.z; o[4 * q + 3] = v.w;
        }
    } else if constexpr (KS == 2) {
        const float2 v = *reinterpret_cast<const float2*>(p);
        o[0] = v.x; o[1] = v.y;
    } else {
        o[0] = p[0];
    }
}
// Write-through (sc1) 16-byte store for data the NEXT kernel reads: a plain store leaves the line dirty in this XCD's L2 and
// the kernel boundary then waits for the write-back of everything the launch dirtied (~1 us per 6 MB: the row update's
// 41 MB, the tile kernel's 26 MB); written through, the bytes leave while the kernel still computes.  Inline asm: hipcc
// does not count it (nothing waits on a store) and the trailing s_nop keeps the data registers alive until it has read them.
__device__ __forceinline__ void st4_wt(float* p, floatx4 v) {
    asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" ::"v"(p), "v"(v) : "memory");
}
__device__ __forceinline__ void st4_sel(float* p, floatx4 v, bool wt) {
    if (wt) st4_wt(p, v); else st4(p, v);
}

// phase timestamps (s_memtime, shader cycles) of wave 0 of every block: ws region `stamps` [blocks][16] u64,
// read back by tools/phase_times.py; costs one scalar load + store per phase
#define DT_STAMP(buf, slot)                                                            \
    do {                                                                               \
        if ((buf) && threadIdx.x == 0)                                                 \
            (buf)[(int64_t)blockIdx.x * 16 + (slot)] = __builtin_amdgcn_s_memtime();    \
    } while (0)

// ---------------------------------------------------------------------------------------------
// Batch-wide sums without a reduction launch (round 5).  Two sets of accumulators live in the workspace as DOUBLES, split
// into shards so that at most 64 blocks meet on one cache line (a wave's atomic covers whole lines: ~55 line requests per
// block, against the 1.3 K stores + the 5 us reduction launch + its boundary they replace):
//   bnacc [kBnShards][2][CP]   sum_b x and sum_b x^2 of every column of the concat row X (kernel A adds, kernel C's prologue
//                              forms mean / variance in double: E[x^2] - mean^2 loses 2 log2(|mean| / sigma) of 53 bits)
//   racc  [kRecShards][stride] the tile kernel's per-tile record entries (Part3: db1, db2, dw3, d w_out, d b_out, loss, the
//                              d w_lin column sums, the two BN-backward sums sdx / sdxx, DCN's cross record)
// racc: every addend is an fp32 value and a shard entry is the double sum of at most 64 of them (B = 8192), which is EXACT
// unless their magnitudes span more than 2^23 — the totals do not depend on the order the blocks arrive in.  bnacc: the
// addends are a block's 16-row sums formed in double (x^2 of an fp32 value is exact in double); their order of arrival can
// move a total by an ulp of a DOUBLE, which survives the rounding to fp32 with probability ~1e-9 per value.  Either way the
// fp32 results are the same from run to run (what the per-tile records + reduction launch guaranteed before; checked: four
// runs of a step bit-identical, tools/r5/dbg_elect.py).
// Life cycle: kernel A zeroes racc (kernel C of the same step adds into it); the launch after kernel C zeroes bnacc for the
// NEXT step's kernel A — the workspace must be zero-filled once before its first use (dt_deepfm_workspace_bytes).
constexpr int kBnShards = 8;
constexpr int kRecShards = 4;
__device__ __forceinline__ void radd(double* p, float v) { unsafeAtomicAdd(p, (double)v); }

struct MlpParams {
    const float *b1, *W2, *b2, *w3, *wo, *bo, *gamma, *mean, *rstd, *sc, *betap;
    const float *W1, *W1L, *W2L, *W2TL;   // original W1 [C][128]; lane-major operand layouts written by k_prep (see k_mlp_fwd3)
    // BatchNormalization's statistics inside kernel C: the batch sums kernel A accumulated (bnacc [kBnShards][2][CP] doubles),
    // the layer's beta, eps / momentum, the moving statistics (updated by block 0, may be NULL) and the padded vectors C
    // publishes for kernels E and D
    const double* bnacc;
    const float* beta;
    float eps, momentum;
    float *moving_mean, *moving_var, *mean_w, *rstd_w, *sc_w, *betap_w;
    float* gammap_w;      // this step's gamma, published like betap: the finishing launch (k_finish_step) reads gamma / beta while
                          // it UPDATES the parameters themselves in other blocks
};

// per-tile partial sums written by C and reduced by E (layout of one tile's record, floats; contiguous).  DCN (L > 0
// cross layers): no slin; G[0..L] (CP floats each: G_l = Xhat^T coeff_l over the tile's rows, see the cross backward of
// kernel C) and one CP-float block of scalars follow: [l] = sum_r coeff_l, [16 + l] = sum_r A_{l+1}, [31] = sum_r dz.
// Pipelined step (G3, see k_mlp_fwd3): two more CP-float vectors per tile, sdx = sum_r dXn[r] and sdxx = sum_r dXn[r] xhat[r]
// over the tile's rows (the two batch sums of BatchNormalization's backward).  Since round 5 every entry is ADDED into the
// sharded double-precision sums `racc` (radd) instead of being written per tile and reduced by a launch of its own.
struct Part3 {
    int slin, db1, db2, dw3, dwo, dbo, loss, cross, sdx, sdxx, n, stride;
};
__host__ __device__ inline Part3 part3_layout(int CP, int L = 0, int g3 = 0) {
    Part3 l;
    l.slin = 0; l.db1 = L > 0 ? 0 : CP; l.db2 = l.db1 + kH1; l.dw3 = l.db2 + kH2;
    l.dwo = l.dw3 + kH2; l.dbo = l.dwo + 1; l.loss = l.dbo + 1;
    l.cross = (l.loss + 1 + 3) & ~3;
    l.n = L > 0 ? l.cross + (L + 2) * CP : l.loss + 1;
    l.sdx = l.sdxx = -1;
    if (g3) {
        l.sdx = (l.n + 3) & ~3;
        l.sdxx = l.sdx + CP;
        l.n = l.sdxx + CP;
    }
    l.stride = (l.n + 3) & ~3;
    return l;
}

// DCN arguments of the tile kernels (cw == NULL: DeepFM)
struct DcnArgs {
    const float *cw, *cb;        // Cross kernels / biases [L][C] (layers.py:423-426, stacked)
    const float* w3c;            // cross part [C] of the kernel applied to Concatenate([cross, dnn])
    int L;
    float* dXc;                  // [B][CP] d loss / d Xn through the cross network (kernel C -> kernel D)
    int mse;                     // loss: 0 = BinaryCrossentropy on the sigmoid output, 1 = MeanSquaredError on the linear output
    int wt;                      // pipelined step: write-through stores of the tile's outputs (st4_wt)
    const float* sw;             // [B] per-row loss weights (Keras sample_weight x class_weight; loss = sum_b w_b l_b / B), NULL: 1
    // DCN: the tile's cross vectors G_0 .. G_L [CP each] leave as a per-tile record [tiles][gstride] (plain stores) and are
    // summed over the tiles where they are finished (the finishing launch's column blocks).  As atomics into the record
    // shards they made the tile kernel 86 us instead of 35: 3.1 K scattered elements per tile = ~800 line requests per block,
    // 64 blocks deep on every line.  (The DeepFM record is 1.6 K elements in whole lines: +1.5 us.)
    float* gpart;
    int gstride;
};

// the shapes every fused plan takes: D a multiple of 4 with D / 4 a power of two, at most 128 lookups of 16 bytes per row
inline bool deepfm_dims(int B, int F, int D, int Nd, DeepFmDims* dm, int* lpr) {
    if (B <= 0 || F <= 0 || D <= 0 || Nd < 0 || D % 4) return false;
    const int l = D / 4;
    if (l < 1 || l > 64 || (l & (l - 1))) return false;
    if (F * l > 128 || Nd > 64) return false;
    dm->B = B; dm->F = F; dm->D = D; dm->Nd = Nd;
    dm->C = F * D + Nd;
    dm->CP = (dm->C + 63) & ~63;
    if (dm->C > 544 || D > 64) return false;
    *lpr = l;
    return true;
}

}  // namespace dt
