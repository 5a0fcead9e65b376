// fgcnn_train.hip — the convolution + activation + max pooling of one FGCNN block for the layer path, forward and backward
// (dt_fg_conv_pool_*, include/dt_hip.h; reference layers.py:220-225: Conv2D((h,1), 'same') -> activation ->
// MaxPooling2D((p,1), 'same')).  Everything is contiguous fp32, channels-last: the map x [B][F][D][C], the kernel in the
// Keras layout [h][1][C][filters], pooled [B][Fp][D][filters], sel (one byte per pooled value) [B][Fp][D][filters].
//
//   z[b,f,d,o]      = bias[o] + sum_{t < h, c < C} x[b, f + t - pb, d, c] k[t][c][o],  pb = (h - 1) / 2, zero beyond the map
//   window i        = fields [i p - qb, i p - qb + p) inside the map, Fp = ceil(F / p) windows, qb = (Fp p - F) / 2
//   pooled[b,i,d,o] = act(max_f z): the four activations are non-decreasing, so the maximum is taken over z and the
//                     activation runs once per window; ties go to the first field; sel = that field's offset in its window
//   dz[b,f,d,o]     = grad_pooled[b,i,d,o] act'(pooled[b,i,d,o]) at the selected field of each window, 0 elsewhere
//   grad_bias[o] = sum dz,  grad_kernel[t][c][o] = sum_{b,f,d} x[b,f+t-pb,d,c] dz[b,f,d,o],
//   grad_x[b,g,d,c] = sum_{t,o} dz[b,g-t+pb,d,o] k[t][c][o]
//
// Neither the taps matrix [B F D][h C] nor a padded map exists anywhere: a block of 256 threads owns a tile of TR batch rows
// whose map sits in LDS with the channel stride C | 1 (odd: the D lanes of a read hit distinct banks), the kernel sits
// beside it zero-padded to 16 filters and to a multiple of four channels ([h][CP][16], read from block-uniform addresses
// as four 16-byte broadcasts), and the taps are read from the map.  Plain fp32 fmaf chains throughout (the exact fp32 class), 64-bit element offsets, a
// grid-stride loop over the tiles of a grid capped at kCpMaxBlocks.
//
//   k_fgcp_fwd     a thread owns one (row, window, d) and all filters: per in-map field of the window the chain over t
//                  then c, loads unconditional from clamped addresses and zeroed afterwards; strict > keeps the first field,
//                  a NaN pre-activation makes the window NaN (as torch.amax).
//   k_fgcp_bwd     per tile: the map and dz go to LDS — dz densified over the window (zeros off the selected field) with 20
//                  floats per (f, d): 16-byte aligned, and 16 consecutive positions land on 16 distinct 4-bank slots — so
//                  both products are regular correlations with no data-dependent addressing.  Staging: thread (group of
//                  positions, filter) — coalesced loads of pooled / grad_pooled / sel, four positions in flight, and the
//                  thread's grad_bias sum is one register.  grad_x: a thread owns one (row, g, d) and the channels (the
//                  template parameter CQ = ceil(C / 4) sizes the chain).  grad_kernel: a thread owns one (t, c) and all
//                  filters for a slice of the tile's (row, f) pairs and keeps its sums in registers over all the block's
//                  tiles.  At the end the slices are summed in LDS in slice order and the block stores its partial into
//                  the workspace [grid][h C filters + filters].
//   k_fgcp_reduce  sums the partials in block order (in double) and overwrites grad_kernel / grad_bias: no float atomics,
//                  so the result is bit-identical from run to run.
//
// Scalar registers: the backward kernel's three phases share one scalar file, and with the straightforward text hipcc
// spilled up to 96 of them.  The empty `asm volatile("" : "+v"(..))` statements in both kernels move block-uniform values that
// only enter lane arithmetic into vector registers (and one of them ends a live range inside the backward's staging loop).  They were
// tuned against the resource report (-Rpass-analysis=kernel-resource-usage) of HIP 7.2 / AMD clang 22.0.0git (roc-7.2.0):
// nothing spills there (DESIGN.md §3.5 has the table).  Another compiler may need fewer of them, or other ones — read the
// report again after a toolchain change.
//
// LDS rule of the domain (bytes): 64 h CP + 64 + F D (4 (C | 1) + 80) <= 65536, CP = C rounded up to a multiple of 4 — the
// padded kernel and bias, one row's map and its dz.  Tile rows: as many as fit, at most what gives the 256 threads one
// item each, at most kCpMaxRows.
#include "common.h"

namespace dt {

typedef float cp_f4 __attribute__((ext_vector_type(4)));

constexpr int kCpThreads = 256;
constexpr int kCpCO = 16;                    // filters the kernel is padded to in LDS
constexpr int kCpDS = 20;                    // floats of dz per (f, d)
constexpr int kCpMaxBlocks = 512;            // grid cap: two blocks per CU
constexpr int kCpMaxRows = 32;               // tile rows cap
constexpr int kCpLdsFloats = 65536 / 4;
constexpr int kCpRed = kCpThreads * kCpCO;   // floats of the end-of-block reduction scratch (aliases the tile)

struct CpShape {
    int F, D, C, filt, h, pool, act;
};
// what the kernels derive from the shape, computed once on the host
struct CpDims {
    int F, D, C, filt, h, pool, act;
    int Fp, pb, qb, CS, CP, TR;
    int64_t tiles;
};
inline CpDims cp_dims(const CpShape& s, int TR, int64_t B) {
    CpDims d{s.F, s.D, s.C, s.filt, s.h, s.pool, s.act};
    d.Fp = (s.F + s.pool - 1) / s.pool;
    d.pb = (s.h - 1) / 2;
    d.qb = (d.Fp * s.pool - s.F) / 2;
    d.CS = s.C | 1;
    d.CP = (s.C + 3) & ~3;
    d.TR = TR;
    d.tiles = (B + TR - 1) / TR;
    return d;
}

inline int64_t cp_head_floats(const CpShape& s) { return (int64_t)s.h * ((s.C + 3) & ~3) * kCpCO + kCpCO; }
inline int64_t cp_map_floats(const CpShape& s) { return (int64_t)s.F * s.D * (s.C | 1); }
inline int64_t cp_dz_floats(const CpShape& s) { return (int64_t)s.F * s.D * kCpDS; }

inline bool cp_ok(const CpShape& s) {
    if (s.C < 1 || s.C > 16 || s.filt < 1 || s.filt > 16 || s.h < 1 || s.h > 16 || s.pool < 1 || s.pool > 8) return false;
    if (s.F < 1 || s.D < 1 || s.F > kCpLdsFloats || s.D > kCpLdsFloats) return false;
    if (s.act != DT_ACT_LINEAR && s.act != DT_ACT_RELU && s.act != DT_ACT_SIGMOID && s.act != DT_ACT_TANH) return false;
    return cp_head_floats(s) + cp_map_floats(s) + cp_dz_floats(s) <= kCpLdsFloats;
}
inline int cp_rows(int64_t fit, int items_per_row) {
    int64_t want = (kCpThreads + items_per_row - 1) / items_per_row;
    if (want > fit) want = fit;
    if (want > kCpMaxRows) want = kCpMaxRows;
    return want < 1 ? 1 : (int)want;
}
inline int cp_rows_fwd(const CpShape& s) {
    const int Fp = (s.F + s.pool - 1) / s.pool;
    return cp_rows((kCpLdsFloats - cp_head_floats(s)) / cp_map_floats(s), Fp * s.D);
}
inline int cp_rows_bwd(const CpShape& s) {
    return cp_rows((kCpLdsFloats - cp_head_floats(s)) / (cp_map_floats(s) + cp_dz_floats(s)), s.F * s.D);
}
inline int cp_grid(int64_t B, int TR) {
    const int64_t tiles = (B + TR - 1) / TR;
    return (int)(tiles < kCpMaxBlocks ? tiles : kCpMaxBlocks);
}
inline size_t cp_lds_fwd(const CpShape& s, int TR) { return (size_t)(cp_head_floats(s) + TR * cp_map_floats(s)) * sizeof(float); }
inline size_t cp_lds_bwd(const CpShape& s, int TR) {
    int64_t tile = TR * (cp_map_floats(s) + cp_dz_floats(s));
    if (tile < kCpRed) tile = kCpRed;
    return (size_t)(cp_head_floats(s) + tile) * sizeof(float);
}

// every index here is non-negative: the unsigned division needs no sign handling
__device__ __forceinline__ int cp_div(int a, int b) { return (int)((unsigned)a / (unsigned)b); }

// the kernel [h][C][filters] -> LDS [h][CP][16], zero beyond the channels and the filters; the bias (NULL: zeros) behind it
__device__ __forceinline__ void cp_stage_kernel(float* __restrict__ kl, const float* __restrict__ kw,
                                                const float* __restrict__ bias, int h, int C, int CP, int filt, int tid) {
#pragma nounroll
    for (int e = tid; e < h * CP * kCpCO; e += kCpThreads) {
        const int o = e & (kCpCO - 1), tc = e >> 4, t = cp_div(tc, CP), c = tc - t * CP;
        const bool in = c < C && o < filt;
        const float v = kw[in ? (t * C + c) * filt + o : 0];
        kl[e] = in ? v : 0.f;
    }
    if (tid < kCpCO) {
        const float v = bias ? bias[tid < filt ? tid : 0] : 0.f;
        kl[h * CP * kCpCO + tid] = tid < filt ? v : 0.f;
    }
}

// `rows` rows of the map [F D C] from `src` -> LDS, channel stride CS, row stride RS; n = TR * msize elements, the rows
// beyond `rows` are zero
__device__ __forceinline__ void cp_stage_map(float* __restrict__ map, const float* __restrict__ src, int n, int rows,
                                             int msize, int C, int CS, int RS, int tid) {
#pragma nounroll
    for (int e = tid; e < n; e += kCpThreads) {
        const int row = cp_div(e, msize), j = e - row * msize, pos = cp_div(j, C), c = j - pos * C;
        const bool in = row < rows;
        const float v = src[in ? e : 0];
        map[row * RS + pos * CS + c] = in ? v : 0.f;
    }
}

__device__ __forceinline__ void cp_fma16(float (&acc)[kCpCO], float x, const float* __restrict__ w) {
    const cp_f4* w4 = reinterpret_cast<const cp_f4*>(w);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const cp_f4 k = w4[q];
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[4 * q + e] = fmaf(x, k[e], acc[4 * q + e]);
    }
}

// the domain the entry points admit (cp_ok), told to the compiler: no loop below needs a zero-trip guard
__device__ __forceinline__ void cp_assume_domain(int F, int D, int C, int filt, int h, int pool) {
    __builtin_assume(F >= 1 && D >= 1);
    __builtin_assume(C >= 1 && C <= 16);
    __builtin_assume(filt >= 1 && filt <= kCpCO);
    __builtin_assume(h >= 1 && h <= 16);
    __builtin_assume(pool >= 1 && pool <= 8);
}

template <int ACT>
__global__ __launch_bounds__(kCpThreads) void k_fgcp_fwd(const float* __restrict__ x, const float* __restrict__ kw,
                                                        const float* __restrict__ bias, int64_t B, CpDims s,
                                                        float* __restrict__ pooled, uint8_t* __restrict__ sel) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x;
    const int F = s.F, D = s.D, C = s.C, filt = s.filt, h = s.h, pool = s.pool;
    cp_assume_domain(F, D, C, filt, h, pool);
    const int CS = s.CS, CP = s.CP, Fp = s.Fp, pb = s.pb, qb = s.qb, TR = s.TR;
    const int msize = F * D * C, RS = F * D * CS, FpD = Fp * D;
    // sizes that only enter lane arithmetic, in vector registers too (see the header: scalar registers)
    int Fv = F, Dv = D, FpDv = FpD, pbv = pb, qbv = qb, poolv = pool, CSv = CS, RSv = RS;
    asm volatile("" : "+v"(Fv), "+v"(Dv), "+v"(FpDv), "+v"(pbv), "+v"(qbv), "+v"(poolv), "+v"(CSv), "+v"(RSv));
    float* kl = lds;                                     // [h][CP][16], CP = C rounded up to 4
    const float* bl = lds + h * CP * kCpCO;
    float* map = lds + h * CP * kCpCO + kCpCO;
    cp_stage_kernel(kl, kw, bias, h, C, CP, filt, tid);
    const int64_t tiles = s.tiles;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t m0 = tile * TR;
        const int rows = B - m0 < TR ? (int)(B - m0) : TR;
        cp_stage_map(map, x + m0 * msize, TR * msize, rows, msize, C, CS, RS, tid);
        lds_barrier();
#pragma nounroll
        for (int e = tid; e < rows * FpD; e += kCpThreads) {
            const int row = cp_div(e, FpDv), r = e - row * FpDv, i = cp_div(r, Dv), d = r - i * Dv;
            float mx[kCpCO];
            int sl[kCpCO];
            const int j0 = qbv - i * poolv > 0 ? qbv - i * poolv : 0;      // the window's first in-map offset
#pragma unroll
            for (int o = 0; o < kCpCO; ++o) { mx[o] = -INFINITY; sl[o] = j0; }
#pragma nounroll
            for (int j = 0; j < pool; ++j) {
                const int f = i * poolv + j - qbv;
                if ((unsigned)f >= (unsigned)Fv) continue;
                float acc[kCpCO];
#pragma unroll
                for (int o = 0; o < kCpCO; ++o) acc[o] = bl[o];
#pragma nounroll
                for (int t = 0; t < h; ++t) {
                    const int ff = f + t - pbv;
                    const bool ok = (unsigned)ff < (unsigned)Fv;
                    const float* xp = map + row * RSv + ((ok ? ff : 0) * Dv + d) * CSv;
                    const float* wp = kl + t * CP * kCpCO;
#pragma nounroll
                    for (int c = 0; c < C; ++c) {
                        const float v = xp[c];
                        cp_fma16(acc, ok ? v : 0.f, wp + c * kCpCO);
                    }
                }
#pragma unroll
                for (int o = 0; o < kCpCO; ++o) {
                    // strict: a tie keeps the earlier field.  A NaN is taken and then kept (no later value compares
                    // greater, and only a NaN replaces it): the window's maximum is NaN, as torch.amax has it
                    const bool take = acc[o] > mx[o] || acc[o] != acc[o];
                    mx[o] = take ? acc[o] : mx[o];
                    sl[o] = take ? j : sl[o];
                }
            }
            const int64_t at = ((m0 + row) * FpD + r) * filt;
#pragma unroll
            for (int o = 0; o < kCpCO; ++o) mx[o] = act_apply(mx[o], ACT);
#pragma unroll
            for (int o = 0; o < kCpCO; ++o) {
                if (o >= filt) break;
                pooled[at + o] = mx[o];
            }
            if (sel) {
#pragma unroll
                for (int o = 0; o < kCpCO; ++o) {
                    if (o >= filt) break;
                    sel[at + o] = (uint8_t)sl[o];
                }
            }
        }
        lds_barrier();                                   // the next tile's map overwrites this one's
    }
}

// CQ = ceil(C / 4): the grad_x chain runs over 4 CQ channels (the kernel's rows beyond C are zero)
template <int CQ>
__global__ __launch_bounds__(kCpThreads) void k_fgcp_bwd(const float* __restrict__ x, const float* __restrict__ kw,
                                                        const float* __restrict__ pooled, const uint8_t* __restrict__ sel,
                                                        const float* __restrict__ gp, int64_t B, CpDims s,
                                                        float* __restrict__ gx, float* __restrict__ ws) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int CP = 4 * CQ;
    const int tid = threadIdx.x;
    const int F = s.F, D = s.D, C = s.C, filt = s.filt, h = s.h, pool = s.pool;
    cp_assume_domain(F, D, C, filt, h, pool);
    __builtin_assume(C > CP - 4 && C <= CP);
    const int CS = s.CS, Fp = s.Fp, pb = s.pb, qb = s.qb, TR = s.TR;
    const int hC = h * C, FD = F * D, msize = FD * C, RS = FD * CS, FpD = Fp * D;
    // C in a vector register: the three tail-channel tests of the grad_x stores are then lane compares at their stores
    // instead of three block-uniform masks that would stay live in scalar registers through the whole kernel
    int Cv = C;
    asm volatile("" : "+v"(Cv));
    // The sizes that only enter lane arithmetic, in vector registers as well: LDS keeps this kernel at a few waves per SIMD,
    // so vector registers are plentiful, while the block-uniform state of three phases would not fit the scalar file.
    int Fv = F, Dv = D, FDv = FD, FpDv = FpD, pbv = pb, qbv = qb, poolv = pool, filtv = filt, CSv = CS, RSv = RS, msizev = msize;
    asm volatile("" : "+v"(Fv), "+v"(Dv), "+v"(FDv), "+v"(FpDv), "+v"(pbv), "+v"(qbv));
    asm volatile("" : "+v"(poolv), "+v"(filtv), "+v"(CSv), "+v"(RSv), "+v"(msizev));
    float* kl = lds;                                     // [h][CP][16]
    float* dz = lds + h * CP * kCpCO + kCpCO;            // [TR][F D][20]; 16-byte aligned
    float* map = dz + TR * FD * kCpDS;                   // [TR][F D][CS]
    cp_stage_kernel(kl, kw, nullptr, h, C, CP, filt, tid);

    // the grad_kernel product: nsl slices of hC threads, thread (slice, tc = t C + c) sums over the (row, f) pairs
    // slice, slice + nsl, ... of every tile
    const int nsl = cp_div(kCpThreads, hC);                     // >= 1: h C <= 256
    const int slice = cp_div(tid, hC), tc = tid - slice * hC, kt = cp_div(tc, C), kc = tc - kt * C;
    const bool kact = slice < nsl;
    float gk[kCpCO];
#pragma unroll
    for (int o = 0; o < kCpCO; ++o) gk[o] = 0.f;
    // the dz staging: thread (position group tid / 16, filter o = tid % 16) — its grad_bias sum is one register
    const int so = tid & (kCpCO - 1), sg = tid >> 4;
    float gb = 0.f;
    // act'(y) as the forms listed beside DT_ACT_* in the header, picked once: a0 + y (a1 + a2 y) — linear 1, sigmoid
    // y (1 - y), tanh 1 - y y — and for relu the step y > 0 (athr = 0; +inf otherwise: never taken).  Kept in vector
    // registers so that the choice costs the staging loop no scalar state.
    float a0 = s.act == DT_ACT_LINEAR || s.act == DT_ACT_TANH ? 1.f : 0.f, a1 = s.act == DT_ACT_SIGMOID ? 1.f : 0.f;
    float a2 = s.act == DT_ACT_SIGMOID || s.act == DT_ACT_TANH ? -1.f : 0.f, athr = s.act == DT_ACT_RELU ? 0.f : INFINITY;
    asm volatile("" : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(athr));

    const int64_t tiles = s.tiles;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t m0 = tile * TR;
        const int rows = B - m0 < TR ? (int)(B - m0) : TR;
        cp_stage_map(map, x + m0 * msize, TR * msize, rows, msizev, Cv, CSv, RSv, tid);
        // dz, densified: every in-map field of window (row, i, d) gets dz at the selected offset and 0 elsewhere, the
        // filters beyond `filt` 0.  Four positions per thread and pass, their loads issued together.
#pragma nounroll
        for (int e0 = sg; e0 < TR * FpD; e0 += 4 * (kCpThreads / kCpCO)) {
            float y[4], g[4];
            int sj[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {                        // unconditional loads from clamped addresses
                const int e = e0 + k * (kCpThreads / kCpCO), row = cp_div(e, FpDv);
                const bool in = row < rows && so < filtv;         // e >= TR FpD: row >= TR >= rows
                const int64_t at = in ? ((m0 + row) * FpD + (e - row * FpDv)) * filt + so : 0;
                y[k] = pooled[at]; g[k] = gp[at]; sj[k] = sel[at];
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                int e = e0 + k * (kCpThreads / kCpCO);
                asm volatile("" : "+v"(e));                      // derived again: no lane mask stays live across the loads
                if (e >= TR * FpD) break;
                const int row = cp_div(e, FpDv), r = e - row * FpDv, i = cp_div(r, Dv), d = r - i * Dv;
                float dy = fmaf(y[k], fmaf(a2, y[k], a1), a0);
                dy = y[k] > athr ? 1.f : dy;
                const float v = (row < rows && so < filtv) ? g[k] * dy : 0.f;
                gb += v;
#pragma nounroll
                for (int j = 0; j < pool; ++j) {
                    const int f = i * poolv + j - qbv;
                    if ((unsigned)f < (unsigned)Fv) dz[((row * Fv + f) * Dv + d) * kCpDS + so] = sj[k] == j ? v : 0.f;
                }
            }
        }
        lds_barrier();
        if (gx) {
            // grad_x: a thread owns one (row, g, d) and the channels; per tap the 16 dz of field g - t + pb
#pragma nounroll
            for (int e = tid; e < rows * FD; e += kCpThreads) {
                const int row = cp_div(e, FDv), r = e - row * FDv, g = cp_div(r, Dv), d = r - g * Dv;
                float acc[CP];
#pragma unroll
                for (int c = 0; c < CP; ++c) acc[c] = 0.f;
#pragma nounroll
                for (int t = 0; t < h; ++t) {
                    const int f = g - t + pbv;
                    const bool ok = (unsigned)f < (unsigned)Fv;
                    const cp_f4* dp = reinterpret_cast<const cp_f4*>(dz + ((row * Fv + (ok ? f : 0)) * Dv + d) * kCpDS);
                    float z[kCpCO];
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const cp_f4 w = dp[q];
#pragma unroll
                        for (int k = 0; k < 4; ++k) z[4 * q + k] = ok ? w[k] : 0.f;
                    }
                    const cp_f4* w4 = reinterpret_cast<const cp_f4*>(kl + t * CP * kCpCO);
#pragma unroll
                    for (int c = 0; c < CP; ++c) {
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const cp_f4 k4 = w4[4 * c + q];
#pragma unroll
                            for (int k = 0; k < 4; ++k) acc[c] = fmaf(z[4 * q + k], k4[k], acc[c]);
                        }
                    }
                }
                const int64_t at = ((m0 + row) * FD + r) * C;
#pragma unroll
                for (int c = 0; c < CP; ++c)
                    if (c < CP - 3 || c < Cv) gx[at + c] = acc[c];
            }
        }
        if (kact) {
#pragma nounroll
            for (int q = slice; q < rows * F; q += nsl) {
                const int row = cp_div(q, Fv), f = q - row * Fv, ff = f + kt - pbv;
                if ((unsigned)ff >= (unsigned)Fv) continue;       // a tap beyond the map adds nothing
                const float* xp = map + row * RSv + ff * Dv * CSv + kc;
                const float* dp = dz + q * D * kCpDS;
#pragma nounroll
                for (int d = 0; d < D; ++d) cp_fma16(gk, xp[d * CS], dp + d * kCpDS);
            }
        }
        lds_barrier();                                   // the next tile's map and dz overwrite these
    }

    // the block's partial: slices summed in slice order, then the staging threads' grad_bias sums in group order
    float* red = dz;
    float* part = ws + (int64_t)blockIdx.x * (hC * filt + filt);
    if (kact) {
        cp_f4* dst = reinterpret_cast<cp_f4*>(red + (tc * nsl + slice) * kCpCO);
#pragma unroll
        for (int q = 0; q < 4; ++q) dst[q] = cp_f4{gk[4 * q], gk[4 * q + 1], gk[4 * q + 2], gk[4 * q + 3]};
    }
    lds_barrier();
#pragma nounroll
    for (int e = tid; e < hC * filt; e += kCpThreads) {
        const int c2 = cp_div(e, filt), o = e - c2 * filt;
        float a = 0.f;
#pragma nounroll
        for (int k = 0; k < nsl; ++k) a += red[(c2 * nsl + k) * kCpCO + o];
        part[e] = a;
    }
    lds_barrier();
    red[tid] = gb;                                       // [group][o]
    lds_barrier();
    if (tid < filt) {
        float b = 0.f;
        for (int k = 0; k < kCpThreads / kCpCO; ++k) b += red[k * kCpCO + tid];
        part[hC * filt + tid] = b;
    }
}

// grad_kernel / grad_bias = the partials summed in block order
__global__ __launch_bounds__(kCpThreads) void k_fgcp_reduce(const float* __restrict__ ws, int nblk, int nk, int nb,
                                                           float* __restrict__ gk, float* __restrict__ gb) {
    const int e = blockIdx.x * kCpThreads + threadIdx.x, n = nk + nb;
    if (e >= n) return;
    double a = 0.0;
#pragma unroll 8
    for (int b = 0; b < nblk; ++b) a += (double)ws[(int64_t)b * n + e];
    if (e < nk) gk[e] = (float)a;
    else if (gb) gb[e - nk] = (float)a;
}

}  // namespace dt

using namespace dt;

extern "C" int dt_fg_conv_pool_supported(int F, int D, int C, int filters, int h, int pool, int act) {
    return cp_ok(CpShape{F, D, C, filters, h, pool, act}) ? 1 : 0;
}

extern "C" int64_t dt_fg_conv_pool_workspace_bytes(int64_t B, int F, int D, int C, int filters, int h, int pool) {
    const CpShape s{F, D, C, filters, h, pool, DT_ACT_LINEAR};
    if (B < 0 || !cp_ok(s)) return -1;
    if (B == 0) return 0;
    return (int64_t)cp_grid(B, cp_rows_bwd(s)) * (h * C * filters + filters) * (int64_t)sizeof(float);
}

extern "C" int dt_fg_conv_pool_geometry(int F, int D, int C, int filters, int h, int pool, int backward, int* tile_rows,
                                        int* max_blocks) {
    const CpShape s{F, D, C, filters, h, pool, DT_ACT_LINEAR};
    DT_UNSUPPORTED(!cp_ok(s), "dt_fg_conv_pool_geometry: F=%d D=%d C=%d filters=%d h=%d pool=%d is outside the domain", F, D, C,
                   filters, h, pool);
    if (tile_rows) *tile_rows = backward ? cp_rows_bwd(s) : cp_rows_fwd(s);
    if (max_blocks) *max_blocks = kCpMaxBlocks;
    return DT_OK;
}

extern "C" int dt_fg_conv_pool_fwd(const float* x, const float* kernel, const float* bias, int64_t B, int F, int D, int C,
                                      int filters, int h, int pool, int act, float* pooled, uint8_t* sel, void* stream) {
    const CpShape s{F, D, C, filters, h, pool, act};
    DT_REQUIRE(B >= 0, "dt_fg_conv_pool_fwd: bad batch size B=%lld", (long long)B);
    DT_UNSUPPORTED(!cp_ok(s), "dt_fg_conv_pool_fwd: F=%d D=%d C=%d filters=%d h=%d pool=%d act=%d is outside the domain", F,
                   D, C, filters, h, pool, act);
    if (B == 0) return DT_OK;
    DT_REQUIRE(x && kernel && pooled, "dt_fg_conv_pool_fwd: null pointer");
    const int TR = cp_rows_fwd(s);
    const size_t lds = cp_lds_fwd(s, TR);
#define DT_CP_FWD(ACTV)                                                                                                     \
    do {                                                                                                                   \
        hipFuncSetAttribute((const void*)k_fgcp_fwd<ACTV>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);          \
        hipLaunchKernelGGL(k_fgcp_fwd<ACTV>, dim3(cp_grid(B, TR)), dim3(kCpThreads), lds, as_stream(stream), x, kernel, bias, \
                           B, cp_dims(s, TR, B), pooled, sel);                                                                         \
    } while (0)
    switch (act) {
        case DT_ACT_RELU: DT_CP_FWD(DT_ACT_RELU); break;
        case DT_ACT_SIGMOID: DT_CP_FWD(DT_ACT_SIGMOID); break;
        case DT_ACT_TANH: DT_CP_FWD(DT_ACT_TANH); break;
        default: DT_CP_FWD(DT_ACT_LINEAR); break;
    }
#undef DT_CP_FWD
    return launch_status("dt_fg_conv_pool_fwd");
}

extern "C" int dt_fg_conv_pool_bwd(const float* x, const float* kernel, const float* pooled, const uint8_t* sel,
                                      const float* grad_pooled, int64_t B, int F, int D, int C, int filters, int h, int pool,
                                      int act, float* grad_x, float* grad_kernel, float* grad_bias, void* workspace,
                                      void* stream) {
    const CpShape s{F, D, C, filters, h, pool, act};
    DT_REQUIRE(B >= 0, "dt_fg_conv_pool_bwd: bad batch size B=%lld", (long long)B);
    DT_UNSUPPORTED(!cp_ok(s), "dt_fg_conv_pool_bwd: F=%d D=%d C=%d filters=%d h=%d pool=%d act=%d is outside the domain", F,
                   D, C, filters, h, pool, act);
    if (B == 0) return DT_OK;
    DT_REQUIRE(x && kernel && pooled && sel && grad_pooled && grad_kernel && workspace, "dt_fg_conv_pool_bwd: null pointer");
    const int TR = cp_rows_bwd(s), grid = cp_grid(B, TR), nk = h * C * filters;
    const size_t lds = cp_lds_bwd(s, TR);
    float* ws = static_cast<float*>(workspace);
#define DT_CP_BWD(CQV)                                                                                                      \
    do {                                                                                                                   \
        hipFuncSetAttribute((const void*)k_fgcp_bwd<CQV>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);           \
        hipLaunchKernelGGL(k_fgcp_bwd<CQV>, dim3(grid), dim3(kCpThreads), lds, as_stream(stream), x, kernel, pooled, sel,   \
                           grad_pooled, B, cp_dims(s, TR, B), grad_x, ws);                                                 \
    } while (0)
    switch ((C + 3) / 4) {
        case 1: DT_CP_BWD(1); break;
        case 2: DT_CP_BWD(2); break;
        case 3: DT_CP_BWD(3); break;
        default: DT_CP_BWD(4); break;
    }
#undef DT_CP_BWD
    hipLaunchKernelGGL(k_fgcp_reduce, dim3(ceil_div(nk + filters, kCpThreads)), dim3(kCpThreads), 0, as_stream(stream),
                       (const float*)ws, grid, nk, filters, grad_kernel, grad_bias);
    return launch_status("dt_fg_conv_pool_bwd");
}
