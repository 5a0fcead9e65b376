// mha.hip — per-row multi-head FIELD self-attention core.
//
// Replaces the op chain of MultiheadAttention.call, deeptables/models/layers.py:129-145:
//   split heads on the last axis / concat on batch, QK^T, / sqrt(d_h), softmax, (dropout),
//   .V, merge heads.   "Sequence length" is the field count F (26 at the Criteo shape), heads
//   are d_h = D/H wide (8), so one attention problem is a 26x26 score tile: far too small for
//   a matrix-core tile per problem, and the Q/K/V/residual projections (the FLOP-heavy part,
//   plain Dense layers in the reference) stay library GEMMs.  One lane owns one
//   (batch row, head, field) task; K/V rows of a (b,h) are wave-broadcast 16-byte loads out of
//   L1.  Nothing of size [B,H,F,F] touches HBM: the forward saves only each score row's
//   maximum m and 1 / l (l the normaliser), the backward recomputes the probabilities (flash-attention style)
//   as exp(s - m) * (1 / l): bit for bit the forward's own weights.  Not from m + log l in one float: that sum is
//   rounded at the size of the scores (2^-24 * 1e6 = 0.06 for fields scaled 1e3), so p came back off by up to that
//   much (1.4 % in grad_v on the 1e-3 .. 1e3 fields test).  The scaled score is rounded to a float of its own
//   (score(): no fma of the dot product into s - m), so m IS one of the s_j, exp(s_j - m) is exactly 1 for it,
//   l >= 1, and a saturated softmax row has the weight 1.0f in both directions, as in the reference's softmax.
#include "common.h"

namespace dt {

// attention-weight dropout (layers.py:141): the keep-mask hash of csrc/autoint.hip (same function, same seeds)
__device__ __forceinline__ float mha_keep(unsigned seed, unsigned thr, unsigned b, unsigned h, unsigned i, unsigned j,
                                          float inv_keep) {
    unsigned x = seed ^ (b * 0x9E3779B1u) ^ ((h * 64u * 64u + i * 64u + j) * 0x85EBCA77u);
    x ^= x >> 16; x *= 0x7FEB352Du; x ^= x >> 15; x *= 0x846CA68Bu; x ^= x >> 16;
    return x >= thr ? inv_keep : 0.f;
}

template <int DHMAX, bool VEC4>
struct RowIO {
    // load d_h floats of row `p` into r[]
    static __device__ __forceinline__ void load(const float* __restrict__ p, int dh, float* r) {
        if (VEC4) {
#pragma unroll
            for (int d = 0; d < DHMAX; d += 4) {
                if (d < dh) {
                    const float4 v = *reinterpret_cast<const float4*>(p + d);
                    r[d] = v.x; r[d + 1] = v.y; r[d + 2] = v.z; r[d + 3] = v.w;
                }
            }
        } else {
#pragma unroll
            for (int d = 0; d < DHMAX; ++d) r[d] = d < dh ? p[d] : 0.f;
        }
    }
    static __device__ __forceinline__ void store(float* __restrict__ p, int dh, const float* r) {
        if (VEC4) {
#pragma unroll
            for (int d = 0; d < DHMAX; d += 4)
                if (d < dh)
                    *reinterpret_cast<float4*>(p + d) = make_float4(r[d], r[d + 1], r[d + 2], r[d + 3]);
        } else {
#pragma unroll
            for (int d = 0; d < DHMAX; ++d)
                if (d < dh) p[d] = r[d];
        }
    }
};

template <int DHMAX>
__device__ __forceinline__ float dotn(const float* a, const float* b, int dh) {
    float s = 0.f;
#pragma unroll
    for (int d = 0; d < DHMAX; ++d)
        if (d < dh) s += a[d] * b[d];
    return s;
}

// the scaled score as a float of its own.  The empty asm makes the rounded product opaque to the compiler: dot * scale - m
// would otherwise be contracted into one fma on the unrounded product (-ffp-contract=fast is hipcc's default, and
// __fmul_rn is a plain multiplication to it), and the row maximum would no longer be one of the scores the exponentials see.
template <int DHMAX>
__device__ __forceinline__ float score(const float* a, const float* b, int dh, float scale) {
    float s = dotn<DHMAX>(a, b, dh) * scale;
    asm("" : "+v"(s));
    return s;
}

template <int DHMAX, bool VEC4>
__global__ __launch_bounds__(256) void k_mha_fwd(const float* __restrict__ q,
                                                 const float* __restrict__ k,
                                                 const float* __restrict__ v, int B, int F, int D,
                                                 int H, int ld, float scale, float* __restrict__ out,
                                                 float* __restrict__ lse, float* __restrict__ stats,
                                                 unsigned drop_thr, float inv_keep, unsigned seed) {
    const int dh = D / H;
    const int64_t total = (int64_t)B * H * F;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const int i = (int)(t % F);
    const int h = (int)((t / F) % H);
    const int64_t b = t / ((int64_t)F * H);
    const int64_t base = b * F * D + (int64_t)h * dh;   // out: contiguous rows of D
    const int64_t ib = b * F * ld + (int64_t)h * dh;    // q / k / v: rows `ld` floats apart
    float qi[DHMAX], kr[DHMAX], acc[DHMAX];
#pragma unroll
    for (int d = 0; d < DHMAX; ++d) { qi[d] = 0.f; kr[d] = 0.f; acc[d] = 0.f; }
    RowIO<DHMAX, VEC4>::load(q + ib + (int64_t)i * ld, dh, qi);
    float m = -INFINITY;
    for (int j = 0; j < F; ++j) {
        RowIO<DHMAX, VEC4>::load(k + ib + (int64_t)j * ld, dh, kr);
        m = fmaxf(m, score<DHMAX>(qi, kr, dh, scale));
    }
    float l = 0.f;
    for (int j = 0; j < F; ++j) {
        RowIO<DHMAX, VEC4>::load(k + ib + (int64_t)j * ld, dh, kr);
        const float p = expf(score<DHMAX>(qi, kr, dh, scale) - m);
        l += p;
        const float pk = drop_thr ? p * mha_keep(seed, drop_thr, (unsigned)b, h, i, j, inv_keep) : p;
        RowIO<DHMAX, VEC4>::load(v + ib + (int64_t)j * ld, dh, kr);
#pragma unroll
        for (int d = 0; d < DHMAX; ++d)
            if (d < dh) acc[d] += pk * kr[d];
    }
    const float inv = 1.0f / l;
#pragma unroll
    for (int d = 0; d < DHMAX; ++d) acc[d] *= inv;
    RowIO<DHMAX, VEC4>::store(out + base + (int64_t)i * D, dh, acc);
    if (lse) lse[t] = m + logf(l);
    if (stats) { stats[2 * t] = m; stats[2 * t + 1] = inv; }
}

// The backward is two launches, one lane per (batch row, head, field) in each.  dS_ij = p_ij (dP_ij keep_ij - delta_i) scale with
// dP_ij = dO_i . v_j and delta_i = sum_j p_ij keep_ij dP_ij.  delta is summed from the same p and dP the difference uses, as the
// softmax backward does, and NOT taken as dO_i . O_i from the stored output: for a row whose softmax is nearly one-hot the
// difference dP_ij - delta_i is (1 - p_ij) dP_ij, the rounding of dP_ij cancels in it when delta is that sum, and does not
// when delta comes through O (2^-24 |dP| left in a difference of 2e-4 |dP|: 2,600 x 2^-24 in a grad_k row at logits x 30).

// launch 1: row r as a QUERY -> delta[r], grad_q[r] = sum_j dS_rj k_j
template <int DHMAX, bool VEC4>
__global__ __launch_bounds__(256) void k_mha_bwd_q(
    const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
    const float* __restrict__ stats, const float* __restrict__ gout, int B, int F, int D, int H, int ld, int ldg,
    float scale, float* __restrict__ gq, float* __restrict__ delta, unsigned drop_thr, float inv_keep, unsigned seed) {
    const int dh = D / H;
    const int64_t total = (int64_t)B * H * F;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const int r = (int)(t % F);
    const int h = (int)((t / F) % H);
    const int64_t b = t / ((int64_t)F * H);
    const int64_t base = b * F * D + (int64_t)h * dh;     // grad_out: contiguous rows of D
    const int64_t ib = b * F * ld + (int64_t)h * dh;      // q / k / v rows `ld` apart
    const int64_t gb = b * F * ldg + (int64_t)h * dh;     // grad_q rows `ldg` apart
    using IO = RowIO<DHMAX, VEC4>;
    float qr[DHMAX], go[DHMAX], kj[DHMAX], vj[DHMAX], acc[DHMAX];
#pragma unroll
    for (int d = 0; d < DHMAX; ++d) { qr[d] = go[d] = kj[d] = vj[d] = acc[d] = 0.f; }
    IO::load(q + ib + (int64_t)r * ld, dh, qr);       // q_r
    IO::load(gout + base + (int64_t)r * D, dh, go);    // dO_r
    const float m_r = stats[2 * t], inv_r = stats[2 * t + 1];   // t = (b * H + h) * F + r
    float delta_r = 0.f;
    for (int j = 0; j < F; ++j) {
        IO::load(k + ib + (int64_t)j * ld, dh, kj);
        IO::load(v + ib + (int64_t)j * ld, dh, vj);
        const float p = expf(score<DHMAX>(qr, kj, dh, scale) - m_r) * inv_r;
        const float kp = drop_thr ? mha_keep(seed, drop_thr, (unsigned)b, h, r, j, inv_keep) : 1.f;
        delta_r += p * (dotn<DHMAX>(go, vj, dh) * kp);
    }
    for (int j = 0; j < F; ++j) {
        IO::load(k + ib + (int64_t)j * ld, dh, kj);
        IO::load(v + ib + (int64_t)j * ld, dh, vj);
        const float p = expf(score<DHMAX>(qr, kj, dh, scale) - m_r) * inv_r;
        const float kp = drop_thr ? mha_keep(seed, drop_thr, (unsigned)b, h, r, j, inv_keep) : 1.f;
        const float ds = p * (dotn<DHMAX>(go, vj, dh) * kp - delta_r) * scale;
#pragma unroll
        for (int d = 0; d < DHMAX; ++d)
            if (d < dh) acc[d] += ds * kj[d];
    }
    IO::store(gq + gb + (int64_t)r * ldg, dh, acc);
    delta[t] = delta_r;
}

// launch 2: row r as a KEY/VALUE -> grad_k[r] = sum_i dS_ir q_i ; grad_v[r] = sum_i p_ir keep_ir dO_i
template <int DHMAX, bool VEC4>
__global__ __launch_bounds__(256) void k_mha_bwd_kv(
    const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
    const float* __restrict__ stats, const float* __restrict__ delta, const float* __restrict__ gout,
    int B, int F, int D, int H, int ld, int ldg, float scale, float* __restrict__ gk, float* __restrict__ gv,
    unsigned drop_thr, float inv_keep, unsigned seed) {
    const int dh = D / H;
    const int64_t total = (int64_t)B * H * F;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const int r = (int)(t % F);
    const int h = (int)((t / F) % H);
    const int64_t b = t / ((int64_t)F * H);
    const int64_t base = b * F * D + (int64_t)h * dh;
    const int64_t ib = b * F * ld + (int64_t)h * dh;
    const int64_t gb = b * F * ldg + (int64_t)h * dh;     // grad_k / grad_v rows `ldg` apart
    const int64_t lbase = (b * H + h) * F;
    using IO = RowIO<DHMAX, VEC4>;
    float kr[DHMAX], vr[DHMAX], qi[DHMAX], go[DHMAX], ak[DHMAX], av[DHMAX];
#pragma unroll
    for (int d = 0; d < DHMAX; ++d) { kr[d] = vr[d] = qi[d] = go[d] = ak[d] = av[d] = 0.f; }
    IO::load(k + ib + (int64_t)r * ld, dh, kr);      // k_r
    IO::load(v + ib + (int64_t)r * ld, dh, vr);      // v_r
    for (int i = 0; i < F; ++i) {
        IO::load(q + ib + (int64_t)i * ld, dh, qi);      // q_i
        IO::load(gout + base + (int64_t)i * D, dh, go);   // dO_i
        const float p = expf(score<DHMAX>(qi, kr, dh, scale) - stats[2 * (lbase + i)]) * stats[2 * (lbase + i) + 1];
        const float kp = drop_thr ? mha_keep(seed, drop_thr, (unsigned)b, h, i, r, inv_keep) : 1.f;
        const float dP = dotn<DHMAX>(go, vr, dh) * kp;
#pragma unroll
        for (int d = 0; d < DHMAX; ++d)
            if (d < dh) av[d] += p * kp * go[d];
        const float ds = p * (dP - delta[lbase + i]) * scale;
#pragma unroll
        for (int d = 0; d < DHMAX; ++d)
            if (d < dh) ak[d] += ds * qi[d];
    }
    IO::store(gk + gb + (int64_t)r * ldg, dh, ak);
    IO::store(gv + gb + (int64_t)r * ldg, dh, av);
}

}  // namespace dt

using namespace dt;

#define DT_MHA_LAUNCH(KERNEL, DHM, ...)                                                           \
    do {                                                                                          \
        if (vec4)                                                                                 \
            hipLaunchKernelGGL((KERNEL<DHM, true>), grid, dim3(256), 0, st, __VA_ARGS__);         \
        else                                                                                      \
            hipLaunchKernelGGL((KERNEL<DHM, false>), grid, dim3(256), 0, st, __VA_ARGS__);        \
    } while (0)

static inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// The shape domain, one answer for both directions.  Widest head: 64 floats in the forward (three row arrays per lane), 32 in
// the backward (seven; at 64 they would spill).  Attention dropout: F <= 64, the hash's counter is h * 4096 + i * 64 + j.
constexpr int kMhaFwdMaxDh = 64, kMhaBwdMaxDh = 32, kMhaDropMaxF = 64;

static bool mha_sizes_ok(int B, int F, int D, int H) { return B >= 0 && F > 0 && D > 0 && H > 0 && D % H == 0; }

// 1: dt_mha_core_fwd AND dt_mha_core_bwd take (F, D, H) with (dropout != 0) or without attention dropout, so a layer can train
// through them; 0: at least one of them returns DT_ERR_UNSUPPORTED (or the sizes are invalid)
extern "C" int dt_mha_core_supported(int F, int D, int H, int dropout) {
    if (!mha_sizes_ok(0, F, D, H)) return 0;
    if (D / H > kMhaBwdMaxDh) return 0;
    return (dropout && F > kMhaDropMaxF) ? 0 : 1;
}

extern "C" int dt_mha_core_fwd(const float* q, const float* k, const float* v, int B, int F, int D,
                               int H, int ld, float dropout_rate, unsigned seed, float* out, float* lse,
                               float* stats, void* stream) {
    unsigned thr; float inv_keep;
    DT_REQUIRE(autoint_drop(dropout_rate, &thr, &inv_keep), "dt_mha_core_fwd: dropout_rate %f", dropout_rate);
    DT_REQUIRE(mha_sizes_ok(B, F, D, H), "dt_mha_core_fwd: bad sizes B=%d F=%d D=%d H=%d", B, F, D, H);
    DT_REQUIRE(ld >= D, "dt_mha_core_fwd: row stride %d < D=%d", ld, D);
    const int dh = D / H;
    DT_UNSUPPORTED(dh > kMhaFwdMaxDh, "dt_mha_core_fwd: head width %d > %d", dh, kMhaFwdMaxDh);
    DT_UNSUPPORTED(thr != 0 && F > kMhaDropMaxF, "dt_mha_core_fwd: attention dropout supports up to %d fields (F=%d)",
                   kMhaDropMaxF, F);
    if (B == 0) return DT_OK;
    DT_REQUIRE(q && k && v && out, "dt_mha_core_fwd: null pointer");
    // float4 rows: every row start a multiple of four floats from a 16-byte aligned base
    const bool vec4 = (dh % 4 == 0) && (D % 4 == 0) && (ld % 4 == 0) &&
                      aligned16(q) && aligned16(k) && aligned16(v) && aligned16(out);
    const float scale = 1.0f / sqrtf((float)dh);
    const int64_t total = (int64_t)B * H * F;
    dim3 grid((unsigned)((total + 255) / 256));
    hipStream_t st = as_stream(stream);
    if (dh <= 4) DT_MHA_LAUNCH(k_mha_fwd, 4, q, k, v, B, F, D, H, ld, scale, out, lse, stats, thr, inv_keep, seed);
    else if (dh <= 8) DT_MHA_LAUNCH(k_mha_fwd, 8, q, k, v, B, F, D, H, ld, scale, out, lse, stats, thr, inv_keep, seed);
    else if (dh <= 16) DT_MHA_LAUNCH(k_mha_fwd, 16, q, k, v, B, F, D, H, ld, scale, out, lse, stats, thr, inv_keep, seed);
    else if (dh <= 32) DT_MHA_LAUNCH(k_mha_fwd, 32, q, k, v, B, F, D, H, ld, scale, out, lse, stats, thr, inv_keep, seed);
    else DT_MHA_LAUNCH(k_mha_fwd, 64, q, k, v, B, F, D, H, ld, scale, out, lse, stats, thr, inv_keep, seed);
    return launch_status("dt_mha_core_fwd");
}

// the two launches of the backward for one DHMAX bracket
#define DT_MHA_BWD(DHM)                                                                                              \
    do {                                                                                                             \
        DT_MHA_LAUNCH(k_mha_bwd_q, DHM, q, k, v, stats, grad_out, B, F, D, H, ld, ldg, scale, grad_q, ws, thr,       \
                      inv_keep, seed);                                                                               \
        DT_MHA_LAUNCH(k_mha_bwd_kv, DHM, q, k, v, stats, ws, grad_out, B, F, D, H, ld, ldg, scale, grad_k, grad_v,   \
                      thr, inv_keep, seed);                                                                          \
    } while (0)

extern "C" int dt_mha_core_bwd(const float* q, const float* k, const float* v, const float* stats,
                               const float* grad_out, int B, int F, int D, int H, int ld, int ldg,
                               float dropout_rate, unsigned seed, float* grad_q, float* grad_k, float* grad_v,
                               float* ws, void* stream) {
    unsigned thr; float inv_keep;
    DT_REQUIRE(autoint_drop(dropout_rate, &thr, &inv_keep), "dt_mha_core_bwd: dropout_rate %f", dropout_rate);
    DT_REQUIRE(mha_sizes_ok(B, F, D, H), "dt_mha_core_bwd: bad sizes B=%d F=%d D=%d H=%d", B, F, D, H);
    DT_REQUIRE(ld >= D && ldg >= D, "dt_mha_core_bwd: row stride %d or %d < D=%d", ld, ldg, D);
    const int dh = D / H;
    DT_UNSUPPORTED(dh > kMhaBwdMaxDh, "dt_mha_core_bwd: head width %d > %d", dh, kMhaBwdMaxDh);
    DT_UNSUPPORTED(thr != 0 && F > kMhaDropMaxF, "dt_mha_core_bwd: attention dropout supports up to %d fields (F=%d)",
                   kMhaDropMaxF, F);
    if (B == 0) return DT_OK;
    DT_REQUIRE(q && k && v && stats && grad_out && grad_q && grad_k && grad_v && ws, "dt_mha_core_bwd: null pointer");
    const bool vec4 = (dh % 4 == 0) && (D % 4 == 0) && (ld % 4 == 0) && (ldg % 4 == 0) &&
                      aligned16(q) && aligned16(k) && aligned16(v) && aligned16(grad_out) &&
                      aligned16(grad_q) && aligned16(grad_k) && aligned16(grad_v);
    const float scale = 1.0f / sqrtf((float)dh);
    const int64_t total = (int64_t)B * H * F;
    dim3 grid((unsigned)((total + 255) / 256));
    hipStream_t st = as_stream(stream);
    if (dh <= 4) DT_MHA_BWD(4);
    else if (dh <= 8) DT_MHA_BWD(8);
    else if (dh <= 16) DT_MHA_BWD(16);
    else DT_MHA_BWD(32);
    return launch_status("dt_mha_core_bwd");
}
