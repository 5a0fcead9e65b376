// optim_slots.hip — the slot optimizers: Adagrad, RMSprop, momentum SGD, Adamax and Ftrl steps (Keras 3 formulas; float32
// state, one update per element, one or two slots per element).
//
//   Adagrad (keras.optimizers.Adagrad):                acc += g*g ;  p -= lr*g / (sqrt(acc) + eps)       (acc starts at
//                                                      initial_accumulator_value)
//   RMSprop (keras.optimizers.RMSprop, momentum 0, not centered):
//                                                      rms = rho*rms + (1-rho)*g*g ;  p -= lr*g / (sqrt(rms) + eps)
//   SGD, momentum mu != 0 (keras.optimizers.SGD):      m = mu*m - lr*g ;  p += m            (nesterov: p += mu*m - lr*g)
//   Adamax (keras.optimizers.Adamax), t 1-based:       m += (g - m)*(1 - b1) ;  u = max(b2*u, |g|)
//                                                      p -= lr*m / ((1 - b1^t)*(u + eps))
//   Ftrl (keras.optimizers.Ftrl), l2' = l2 + beta/(2 lr) folded by the host, a = -learning_rate_power:
//       g' = g + 2*l2_shrinkage*p ;  n' = n + g*g ;  linear += g' - (n'^a - n^a)/lr * p
//       q  = n'^a/lr + 2*l2' ;  p = (clip(linear, -l1, l1) - linear)/q ;  n = n'
//     q == 0 (n' == 0: an accumulator that starts at 0, a zero gradient, no l2 / beta) writes p = 0 where Keras writes NaN:
//     the zero pads of a flat group stay 0.  a == 0.5 (the default) takes sqrtf, any other a powf: chosen per launch.
//
// No bias correction by the host: the learning rate is a plain kernel argument, and the step state is Adam's (AdamState), of
// which only t and the arrival counters are used.  ONE family of launches, the kind a template argument: dense (float4 body,
// scalar tail), multi-tensor (chunks of 32 tensors), and the row update behind the unchanged merge of duplicate lookups
// (rows_merge, optim.hip), whose trailing blocks carry one dense update and whose last launch advances the step counter.
// Every form of an optimizer's update goes through ONE function compiled without contraction, so that they agree bit for bit.
// RMSprop's row update alone has an owner kernel of its own (k_rms_rows_owner): its per-row stamps need a block barrier.
#include <stdlib.h>
#include "common.h"
#include "adam_dev.h"
#include "optim_dev.h"

namespace dt {

enum SlotKind { kAdagrad = 0, kRmsprop = 1, kSgdm = 2, kSgdmNesterov = 3, kAdamax = 4, kFtrlSqrt = 5, kFtrlPow = 6 };

template <int K>
struct SlotTraits {
    static constexpr int slots = K >= kAdamax ? 2 : 1;
};

struct SlotHp {                 // Adagrad: c2 = epsilon | RMSprop: c0 = rho, c2 = epsilon | SGD: c0 = momentum
    float lr;                   // Adamax: c0 = beta_1, c1 = beta_2, c2 = epsilon
    float c0, c1, c2, c3;       // Ftrl: c0 = -learning_rate_power, c1 = l1, c2 = l2 + beta/(2 lr), c3 = l2_shrinkage
};

// corr: Adamax's 1 - beta_1^t of the step this launch belongs to (slot_read_corr); unused by the others
template <int K>
__device__ __forceinline__ void slot_update(float& p, float& s0, float& s1, float g, const SlotHp& h, float corr) {
#pragma clang fp contract(off)
    if (K == kAdagrad || K == kRmsprop) {
        s0 = K == kRmsprop ? h.c0 * s0 + (1.f - h.c0) * (g * g) : s0 + g * g;
        p -= h.lr * g / (sqrtf(s0) + h.c2);
    } else if (K == kSgdm || K == kSgdmNesterov) {
        s0 = h.c0 * s0 - h.lr * g;
        p = K == kSgdm ? p + s0 : p + (h.c0 * s0 - h.lr * g);
    } else if (K == kAdamax) {
        s0 = s0 + (g - s0) * (1.f - h.c0);
        s1 = fmaxf(h.c1 * s1, fabsf(g));
        p = p - (h.lr * s0) / (corr * (s1 + h.c2));
    } else {
        const float gs = g + 2.f * h.c3 * p;
        const float n2 = s0 + g * g;
        const float pw_new = K == kFtrlSqrt ? sqrtf(n2) : powf(n2, h.c0);
        const float pw_old = K == kFtrlSqrt ? sqrtf(s0) : powf(s0, h.c0);
        // n'^a - n^a without the cancellation of two nearly equal powers (a small gradient on a grown accumulator loses all
        // but a few bits there, and linear keeps that error for good): sqrt(n') - sqrt(n) = g^2 / (sqrt(n') + sqrt(n));
        // n'^a - n^a = n^a * expm1(a * log1p(g^2 / n)) for n > 0
        float dpw;
        if (K == kFtrlSqrt) {
            const float sum = pw_new + pw_old;
            dpw = sum > 0.f ? (g * g) / sum : 0.f;
        } else {
            dpw = s0 > 0.f ? pw_old * expm1f(h.c0 * log1pf((g * g) / s0)) : pw_new - pw_old;
        }
        s1 = s1 + gs - dpw / h.lr * p;
        const float q = pw_new / h.lr + 2.f * h.c2;
        const float clipped = fminf(fmaxf(s1, -h.c1), h.c1);
        p = q == 0.f ? 0.f : (clipped - s1) / q;
        s0 = n2;
    }
}

// step_read_t, then (Adamax) 1 - beta_1^t from the DEVICE t: one powf per block, handed to the block through LDS.  A captured
// graph replays the launch with its host arguments frozen, so the power cannot be a host value.
template <int K>
__device__ __forceinline__ float slot_read_corr(AdamState* st, int advance, unsigned& ticket, const SlotHp& h) {
    if (K != kAdamax) {
        step_read_t(st, advance, ticket);
        return 1.f;
    }
    // step_read_t with the power taken by the thread that reads t, ahead of the one barrier
    __shared__ float s_corr;
    ticket = kNoTicket;
    if (!st) return 1.f - h.c0;                               // (refused by the host: t = 1)
    if (threadIdx.x == 0) {
        s_corr = 1.f - powf(h.c0, (float)st->t);
        if (advance) ticket = 0u;
    }
    __syncthreads();
    return s_corr;
}

struct SlotTail {              // a dense update: n elements of p / g / slot 0 / slot 1; vec: all of them 16-byte aligned
    float* p;
    const float* g;
    float* s0;
    float* s1;                  // unused by the one-slot kinds
    int64_t n;
    int vec;
};

// float4 body, scalar tail
template <int K>
__device__ __forceinline__ void slot_dense_range(const SlotTail& d, int64_t first, int64_t stride, const SlotHp& h,
                                                 float corr) {
    constexpr bool two = SlotTraits<K>::slots == 2;
    const int64_t n4 = d.vec ? d.n >> 2 : 0;
    for (int64_t i = first; i < n4; i += stride) {
        const float4 g4 = reinterpret_cast<const float4*>(d.g)[i];
        float4 a4 = reinterpret_cast<float4*>(d.s0)[i], p4 = reinterpret_cast<float4*>(d.p)[i];
        float4 b4 = make_float4(0.f, 0.f, 0.f, 0.f);
        if (two) b4 = reinterpret_cast<float4*>(d.s1)[i];
        slot_update<K>(p4.x, a4.x, b4.x, g4.x, h, corr);
        slot_update<K>(p4.y, a4.y, b4.y, g4.y, h, corr);
        slot_update<K>(p4.z, a4.z, b4.z, g4.z, h, corr);
        slot_update<K>(p4.w, a4.w, b4.w, g4.w, h, corr);
        reinterpret_cast<float4*>(d.s0)[i] = a4;
        if (two) reinterpret_cast<float4*>(d.s1)[i] = b4;
        reinterpret_cast<float4*>(d.p)[i] = p4;
    }
    for (int64_t i = 4 * n4 + first; i < d.n; i += stride) {
        float ai = d.s0[i], bi = two ? d.s1[i] : 0.f, pi = d.p[i];
        slot_update<K>(pi, ai, bi, d.g[i], h, corr);
        d.s0[i] = ai;
        if (two) d.s1[i] = bi;
        d.p[i] = pi;
    }
}

template <int K>
__global__ __launch_bounds__(256) void k_slot_dense(SlotTail d, SlotHp h, AdamState* __restrict__ st, int advance) {
    unsigned ticket;
    const float corr = slot_read_corr<K>(st, advance, ticket, h);
    slot_dense_range<K>(d, (int64_t)blockIdx.x * blockDim.x + threadIdx.x, (int64_t)gridDim.x * blockDim.x, h, corr);
    step_finish(st, ticket);
}

struct SlotMulti {              // k_adam_multi's descriptor (optim.hip) with the slots' names
    float* p[kMultiMax];
    const float* g[kMultiMax];
    float* s0[kMultiMax];
    float* s1[kMultiMax];
    int n[kMultiMax];
    int block_start[kMultiMax + 1];
    int count;
};

template <int K>
__global__ __launch_bounds__(256) void k_slot_multi(SlotMulti d, SlotHp h, AdamState* __restrict__ st, int advance) {
    constexpr bool two = SlotTraits<K>::slots == 2;
    unsigned ticket;
    const float corr = slot_read_corr<K>(st, advance, ticket, h);
    int t = 0;
    while (t + 1 < d.count && (int)blockIdx.x >= d.block_start[t + 1]) ++t;
    const int first = (int)(blockIdx.x - d.block_start[t]) * kMultiPerBlock + (int)threadIdx.x;
    const int end = min(d.n[t], (int)(blockIdx.x - d.block_start[t] + 1) * kMultiPerBlock);
    for (int i = first; i < end; i += 256) {
        float ai = d.s0[t][i], bi = two ? d.s1[t][i] : 0.f, pi = d.p[t][i];
        slot_update<K>(pi, ai, bi, d.g[t][i], h, corr);
        d.s0[t][i] = ai;
        if (two) d.s1[t][i] = bi;
        d.p[t][i] = pi;
    }
    step_finish(st, ticket);
}

// Row update after the merge (rows_merge, optim.hip): the owner occurrence of every distinct row updates that table row and
// its slot record, for every kind but RMSprop (k_rms_rows_owner below).  T = min(D / VW, 256) threads per row and 256 / T
// whole rows per block, rows with more than 256 pieces walked: a row never straddles two blocks.  The two slots of a row are
// s0 + row * sstride and s1 + row * sstride: with ONE [V, 2, D] record (s1 = s0 + D, sstride = 2 D) they share a 128-byte
// line at D = 16 and the update touches two random locations per row.
// The loads of a piece — gradient, slots, weights — are all issued before its arithmetic.
template <int K, int VW>
__global__ __launch_bounds__(256) void k_slot_rows_owner(float* __restrict__ table, float* __restrict__ s0,
                                                          float* __restrict__ s1, const int64_t* __restrict__ rows,
                                                          const float* __restrict__ values, int64_t n, int D,
                                                          unsigned long long* __restrict__ hslots,
                                                          const int* __restrict__ mark, SlotHp h,
                                                          AdamState* __restrict__ st, int row_blocks, SlotTail tail,
                                                          int advance, int sstride) {
    constexpr bool two = SlotTraits<K>::slots == 2;
    unsigned ticket;
    const float corr = slot_read_corr<K>(st, advance, ticket, h);
    if ((int)blockIdx.x >= row_blocks) {      // trailing blocks: one dense update (the model's flat buffer)
        slot_dense_range<K>(tail, (int64_t)(blockIdx.x - row_blocks) * blockDim.x + threadIdx.x,
                            (int64_t)(gridDim.x - row_blocks) * blockDim.x, h, corr);
        step_finish(st, ticket);
        return;
    }
    const int lpr = D / VW;                                   // pieces (VW floats) per row
    const int T = lpr < 256 ? lpr : 256, rpb = 256 / T;
    const int r = (int)threadIdx.x / T, q0 = (int)threadIdx.x - r * T;
    const int64_t occ = (int64_t)blockIdx.x * rpb + r;
    int hs = -1;
    int64_t row = 0;
    if (r < rpb && occ < n) {
        row = rows[occ];
        hs = mark ? mark[occ] : (row >= 0 ? 0 : -1);          // no mark: rows are already distinct
    }
    if (hs >= 0) {
        const float* gsrc = values + occ * D;
        float* prow = table + row * D;
        float* arow = s0 + row * sstride;
        float* brow = two ? s1 + row * sstride : nullptr;
        for (int q = q0; q < lpr; q += T) {                   // (more than 256 pieces per row: the thread walks the rest)
            float gi[VW], ai[VW], bi[VW], pi[VW];
            if (VW == 4) {
                *reinterpret_cast<float4*>(gi) = *reinterpret_cast<const float4*>(gsrc + q * 4);
                *reinterpret_cast<float4*>(ai) = *reinterpret_cast<const float4*>(arow + q * 4);
                if (two) *reinterpret_cast<float4*>(bi) = *reinterpret_cast<const float4*>(brow + q * 4);
                *reinterpret_cast<float4*>(pi) = *reinterpret_cast<const float4*>(prow + q * 4);
            } else {
                gi[0] = gsrc[q]; ai[0] = arow[q]; pi[0] = prow[q];
                if (two) bi[0] = brow[q];
            }
#pragma unroll
            for (int k = 0; k < VW; ++k) {
                if (!two) bi[k] = 0.f;
                slot_update<K>(pi[k], ai[k], bi[k], gi[k], h, corr);
            }
            if (VW == 4) {
                *reinterpret_cast<float4*>(arow + q * 4) = *reinterpret_cast<float4*>(ai);
                if (two) *reinterpret_cast<float4*>(brow + q * 4) = *reinterpret_cast<float4*>(bi);
                *reinterpret_cast<float4*>(prow + q * 4) = *reinterpret_cast<float4*>(pi);
            } else {
                arow[q] = ai[0]; prow[q] = pi[0];
                if (two) brow[q] = bi[0];
            }
        }
        if (q0 == 0 && hslots) hslots[hs] = 0ULL;             // global-hash merge: leave the hash empty for the next step
    }
    step_finish(st, ticket);
}

// RMSprop's lazy decay: s *= rho^idle for a row that sat out `idle` steps.  Short gaps repeat the multiplication the dense
// decay makes every step (the same bits); longer ones take one powf.
constexpr int kExactDecay = 8;
__device__ __forceinline__ float decay_factor(float rho, int idle) {
    return idle > kExactDecay ? powf(rho, (float)idle) : 1.f;
}
__device__ __forceinline__ float decayed(float s, float rho, int idle, float factor) {
    if (idle > kExactDecay) return s * factor;
    for (int k = 0; k < idle; ++k) s *= rho;
    return s;
}

// RMSprop's row update: k_slot_rows_owner's geometry and dense tail, and per-row stamps.  `stamp` holds the step at which a
// row's rms was last written; every thread of the row reads it, rms first takes the decay of the steps the row sat out,
// rho^(t - stamp - 1) (decayed), and the row's first thread writes the new stamp only behind the block's barrier.  The first
// piece's loads are issued ahead of that barrier.
template <int VW>
__global__ __launch_bounds__(256) void k_rms_rows_owner(float* __restrict__ table, float* __restrict__ slot,
                                                        int* __restrict__ stamp, const int64_t* __restrict__ rows,
                                                        const float* __restrict__ values, int64_t n, int D,
                                                        unsigned long long* __restrict__ hslots,
                                                        const int* __restrict__ mark, SlotHp h, AdamState* __restrict__ st,
                                                        int row_blocks, SlotTail tail, int advance, int sstride, int tstride) {
    unsigned ticket;
    const int t = step_read_t(st, advance, ticket);
    if ((int)blockIdx.x >= row_blocks) {      // trailing blocks: one dense update (the model's flat buffer)
        slot_dense_range<kRmsprop>(tail, (int64_t)(blockIdx.x - row_blocks) * blockDim.x + threadIdx.x,
                                   (int64_t)(gridDim.x - row_blocks) * blockDim.x, h, 1.f);
        step_finish(st, ticket);
        return;
    }
    const float rho = h.c0;
    const int lpr = D / VW;                                   // pieces (VW floats) per row
    const int T = lpr < 256 ? lpr : 256, rpb = 256 / T;
    const int r = (int)threadIdx.x / T, q0 = (int)threadIdx.x - r * T;
    const int64_t occ = (int64_t)blockIdx.x * rpb + r;
    int hs = -1;
    int64_t row = 0;
    if (r < rpb && occ < n) {
        row = rows[occ];
        hs = mark ? mark[occ] : (row >= 0 ? 0 : -1);          // no mark: rows are already distinct
    }
    const bool live = hs >= 0;
    int idle = 0;
    float decay = 1.f;
    float gi[VW], si[VW], pi[VW];
    // the first piece's loads are in flight together with the stamp's
    if (live) {
        const float* gsrc = values + occ * D + q0 * VW;
        if (VW == 4) {
            *reinterpret_cast<float4*>(gi) = *reinterpret_cast<const float4*>(gsrc);
            *reinterpret_cast<float4*>(si) = *reinterpret_cast<const float4*>(slot + row * sstride + q0 * VW);
            *reinterpret_cast<float4*>(pi) = *reinterpret_cast<const float4*>(table + row * D + q0 * VW);
        } else {
            gi[0] = gsrc[0]; si[0] = slot[row * sstride + q0]; pi[0] = table[row * D + q0];
        }
        idle = t - 1 - stamp[row * tstride];
        decay = decay_factor(rho, idle);
    }
    __syncthreads();              // every thread of the block has its row's stamp before any of them is rewritten
    if (live) {
        float unused = 0.f;       // (the second slot of the two-slot kinds)
        for (int q = q0;;) {
#pragma unroll
            for (int k = 0; k < VW; ++k) {
                si[k] = decayed(si[k], rho, idle, decay);
                slot_update<kRmsprop>(pi[k], si[k], unused, gi[k], h, 1.f);
            }
            if (VW == 4) {
                *reinterpret_cast<float4*>(slot + row * sstride + q * VW) = *reinterpret_cast<float4*>(si);
                *reinterpret_cast<float4*>(table + row * D + q * VW) = *reinterpret_cast<float4*>(pi);
            } else {
                slot[row * sstride + q] = si[0]; table[row * D + q] = pi[0];
            }
            q += T;
            if (q >= lpr) break;  // (more than 256 pieces per row: the thread walks the rest)
#pragma unroll
            for (int k = 0; k < VW; ++k) {
                gi[k] = values[occ * D + q * VW + k]; si[k] = slot[row * sstride + q * VW + k];
                pi[k] = table[row * D + q * VW + k];
            }
        }
        if (q0 == 0) {
            stamp[row * tstride] = t;
            if (hslots) hslots[hs] = 0ULL;                    // global-hash merge: leave the hash empty for the next step
        }
    }
    step_finish(st, ticket);
}

// RMSprop: the decay pending on every row (rho^(steps done - stamp)) applied to rms, then every stamp = steps done.  Two
// launches, so that no thread reads a stamp another has rewritten.
__global__ __launch_bounds__(256) void k_rms_materialize(float* __restrict__ rms, const int* __restrict__ stamp, int64_t V,
                                                         int D, int sstride, int tstride, float rho,
                                                         const AdamState* __restrict__ st) {
    const int done = st->t - 1;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < V * D; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = i / D;
        const int idle = done - stamp[row * tstride];
        if (idle > 0) {
            float* s = rms + row * sstride + (i - row * D);
            *s = decayed(*s, rho, idle, decay_factor(rho, idle));
        }
    }
}
__global__ __launch_bounds__(256) void k_rms_restamp(int* __restrict__ stamp, int64_t V, int tstride,
                                                     const AdamState* __restrict__ st) {
    const int done = st->t - 1;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < V; i += (int64_t)gridDim.x * blockDim.x)
        stamp[i * tstride] = done;
}

// ---- host side ---------------------------------------------------------------------------------------------------------------
// the float4 body needs 16-byte aligned arrays; arrays that are only float aligned take the scalar loop
static SlotTail slot_tail(int nslots, float* p, const float* g, float* s0, float* s1, int64_t n) {
    const bool vec = aligned_to(p, 16) && aligned_to(g, 16) && aligned_to(s0, 16) && (nslots < 2 || aligned_to(s1, 16));
    return SlotTail{p, g, s0, s1, n, vec ? 1 : 0};
}

template <int K>
static int slot_dense_step(const char* who, float* p, const float* g, float* s0, float* s1, int64_t n, const SlotHp& h,
                           void* state, int advance, void* stream) {
    constexpr int NS = SlotTraits<K>::slots;
    DT_REQUIRE(n >= 0, "%s: n < 0", who);
    DT_REQUIRE(K == kAdamax ? (n == 0 && !advance) || state != nullptr : (!advance || state != nullptr),
               K == kAdamax ? "%s: the step number is read from the device state" : "%s: advance needs the device state", who);
    if (n == 0) return advance ? dt_adam_advance(state, 0.f, 0.f, 0.f, stream) : DT_OK;
    DT_REQUIRE(p && g && s0 && (NS < 2 || s1), "%s: null pointer", who);
    DT_REQUIRE(aligned_to(p, 4) && aligned_to(g, 4) && aligned_to(s0, 4) && (NS < 2 || aligned_to(s1, 4)),
               "%s: pointers must be float aligned", who);
    int64_t blocks = (n / 4 + 255) / 256 + 1;
    if (blocks > 256 * 16) blocks = 256 * 16;
    hipLaunchKernelGGL(k_slot_dense<K>, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream),
                       slot_tail(NS, p, g, s0, s1, n), h, (AdamState*)state, advance);
    return launch_status(who);
}

template <int K>
static int slot_multi_step(const char* who, int count, float* const* p, const float* const* g, float* const* s0,
                           float* const* s1, const int64_t* n, const SlotHp& h, void* state, int advance, void* stream) {
    constexpr int NS = SlotTraits<K>::slots;
    DT_REQUIRE(count >= 0 && (count == 0 || (p && g && s0 && (NS < 2 || s1) && n)), "%s: bad arguments", who);
    DT_REQUIRE(!advance || state, "%s: advance needs the device state", who);
    bool any = false;
    for (int t = 0; t < count; ++t) {       // every tensor is checked before the first chunk is launched
        DT_REQUIRE(n[t] >= 0 && n[t] < (1LL << 31) && (n[t] == 0 || (p[t] && g[t] && s0[t] && (NS < 2 || s1[t]))) &&
                       aligned_to(p[t], 4) && aligned_to(g[t], 4) && aligned_to(s0[t], 4) && (NS < 2 || aligned_to(s1[t], 4)),
                   "%s: tensor %d: bad size, null or misaligned pointer", who, t);
        any = any || n[t] > 0;
    }
    DT_REQUIRE(K != kAdamax || !any || state, "%s: the step number is read from the device state", who);
    bool launched = false, advanced = false;
    for (int c0 = 0; c0 < count; c0 += kMultiMax) {
        SlotMulti d;
        d.count = count - c0 < kMultiMax ? count - c0 : kMultiMax;
        int blocks = 0;
        for (int t = 0; t < d.count; ++t) {
            d.p[t] = p[c0 + t]; d.g[t] = g[c0 + t]; d.s0[t] = s0[c0 + t]; d.s1[t] = NS < 2 ? nullptr : s1[c0 + t];
            d.n[t] = (int)n[c0 + t];
            d.block_start[t] = blocks;
            blocks += (int)((n[c0 + t] + kMultiPerBlock - 1) / kMultiPerBlock);
        }
        d.block_start[d.count] = blocks;
        if (blocks == 0) continue;
        const bool last_chunk = c0 + kMultiMax >= count;
        hipLaunchKernelGGL(k_slot_multi<K>, dim3(blocks), dim3(256), 0, as_stream(stream), d, h, (AdamState*)state,
                           (advance && last_chunk) ? 1 : 0);
        launched = true;
        advanced = advance && last_chunk;
    }
    if (advance && !advanced) return dt_adam_advance(state, 0.f, 0.f, 0.f, stream);
    return launched ? launch_status(who) : DT_OK;
}

// stamp, stamp_stride: RMSprop's per-row stamps (the other kinds pass none); its row update reads the step number from the
// device state, as every launch of Adamax does
template <int K>
static int slot_rows_step(const char* who, float* table, float* s0, float* s1, int* stamp, const int64_t* rows, float* values,
                          int64_t n_rows, int D, int fields, void* slots, int64_t n_slots, int* mark, const SlotHp& h,
                          void* state, float* dense_p, const float* dense_g, float* dense_s0, float* dense_s1,
                          int64_t dense_n, int advance, int slot_stride, int stamp_stride, void* stream) {
    constexpr int NS = SlotTraits<K>::slots;
    DT_REQUIRE(n_rows >= 0 && D > 0 && fields >= -1 && dense_n >= 0, "%s: bad sizes", who);
    DT_REQUIRE(slot_stride >= D, "%s: slot_stride %d < D = %d", who, slot_stride, D);
    DT_REQUIRE(K != kRmsprop || state, "%s: the step number is read from the device state", who);
    DT_REQUIRE(dense_n == 0 || (dense_p && dense_g && dense_s0 && (NS < 2 || dense_s1)), "%s: null dense tail", who);
    DT_REQUIRE(aligned_to(dense_p, 4) && aligned_to(dense_g, 4) && aligned_to(dense_s0, 4) && aligned_to(dense_s1, 4),
               "%s: dense tail pointers must be float aligned", who);
    if (n_rows == 0)      // nothing sparse this step: the tail (and the advance) run as a plain dense step
        return slot_dense_step<K>(who, dense_p, dense_g, dense_s0, dense_s1, dense_n, h, state, advance, stream);
    DT_REQUIRE(K == kAdamax ? state != nullptr : (!advance || state != nullptr),
               K == kAdamax ? "%s: the step number is read from the device state" : "%s: advance needs the device state", who);
    DT_REQUIRE(table && s0 && (NS < 2 || s1) && rows && values && (K != kRmsprop || stamp), "%s: null pointer", who);
    DT_REQUIRE(n_rows < (1LL << 31), "%s: %lld occurrences do not fit the 32-bit slot field", who, (long long)n_rows);
    const bool vec = D % 4 == 0;
    const size_t al = vec ? 16 : 4;
    DT_REQUIRE(aligned_to(table, al) && aligned_to(s0, al) && (NS < 2 || aligned_to(s1, al)) && aligned_to(values, al) &&
                   (!vec || slot_stride % 4 == 0),
               K <= kRmsprop ? "%s: table, slot and values must be %d-byte aligned (D = %d, slot_stride = %d)"
                             : "%s: table, slots and values must be %d-byte aligned (D = %d, slot_stride = %d)",
               who, (int)al, D, slot_stride);
    // the two slots of a row must not overlap: separate arrays, or one record with s1 at least D floats behind s0
    DT_REQUIRE(NS < 2 || s1 >= s0 + D || s0 >= s1 + D, "%s: the slots of a row overlap", who);
    DT_REQUIRE(aligned_to(rows, 8) && aligned_to(slots, 8) && aligned_to(mark, 4), "%s: misaligned rows / slots / mark", who);
    DT_REQUIRE(K != kRmsprop || (aligned_to(stamp, 4) && stamp_stride >= 1), "%s: misaligned stamp or stamp_stride < 1", who);
    hipStream_t st = as_stream(stream);
    unsigned long long* gslots = nullptr;
    int* mk = mark;
    if (const int rc = rows_merge(who, rows, values, n_rows, D, fields, slots, n_slots, mark, st, &gslots, &mk)) return rc;
    const SlotTail tail = slot_tail(NS, dense_p, dense_g, dense_s0, dense_s1, dense_n);
    int tail_blocks = (int)((dense_n / 4 + 255) / 256) + (dense_n ? 1 : 0);
    if (tail_blocks > 1024) tail_blocks = 1024;
    const int lpr = vec ? D / 4 : D;
    const int rpb = 256 / (lpr < 256 ? lpr : 256);
    const int row_blocks = (int)((n_rows + rpb - 1) / rpb);
    const dim3 grid((unsigned)(row_blocks + tail_blocks));
    if constexpr (K == kRmsprop) {
        if (vec)
            hipLaunchKernelGGL(k_rms_rows_owner<4>, grid, dim3(256), 0, st, table, s0, stamp, rows, values, n_rows, D, gslots, mk,
                               h, (AdamState*)state, row_blocks, tail, advance, slot_stride, stamp_stride);
        else
            hipLaunchKernelGGL(k_rms_rows_owner<1>, grid, dim3(256), 0, st, table, s0, stamp, rows, values, n_rows, D, gslots, mk,
                               h, (AdamState*)state, row_blocks, tail, advance, slot_stride, stamp_stride);
    } else {
        if (vec)
            hipLaunchKernelGGL((k_slot_rows_owner<K, 4>), grid, dim3(256), 0, st, table, s0, s1, rows, values, n_rows, D,
                               gslots, mk, h, (AdamState*)state, row_blocks, tail, advance, slot_stride);
        else
            hipLaunchKernelGGL((k_slot_rows_owner<K, 1>), grid, dim3(256), 0, st, table, s0, s1, rows, values, n_rows, D,
                               gslots, mk, h, (AdamState*)state, row_blocks, tail, advance, slot_stride);
    }
    return launch_status(who);
}

static bool ftrl_hp(const char* who, float lr, float lr_power, float l1, float l2, float l2_shrinkage, SlotHp* h) {
    if (!(lr > 0.f) || !(lr_power <= 0.f) || !(l1 >= 0.f) || !(l2 >= 0.f) || !(l2_shrinkage >= 0.f)) {
        set_error("%s: needs lr > 0, lr_power <= 0 and non-negative l1 / l2 / l2_shrinkage", who);
        return false;
    }
    *h = SlotHp{lr, -lr_power, l1, l2, l2_shrinkage};
    return true;
}

}  // namespace dt

using namespace dt;

// the kind is chosen once per launch: SGD's nesterov form, Ftrl's sqrtf (learning_rate_power == -0.5) against powf
#define DT_SGDM(call) (nesterov ? call<kSgdmNesterov> : call<kSgdm>)
#define DT_FTRL(call) (lr_power == -0.5f ? call<kFtrlSqrt> : call<kFtrlPow>)

extern "C" int dt_adagrad_dense_step(float* p, const float* g, float* acc, int64_t n, float lr, float eps, void* state,
                                     int advance, void* stream) {
    const SlotHp h{lr, 0.f, 0.f, eps, 0.f};
    return slot_dense_step<kAdagrad>("dt_adagrad_dense_step", p, g, acc, nullptr, n, h, state, advance, stream);
}

extern "C" int dt_adagrad_multi_step(int count, float* const* p, const float* const* g, float* const* acc, const int64_t* n,
                                     float lr, float eps, void* state, int advance, void* stream) {
    const SlotHp h{lr, 0.f, 0.f, eps, 0.f};
    return slot_multi_step<kAdagrad>("dt_adagrad_multi_step", count, p, g, acc, nullptr, n, h, state, advance, stream);
}

extern "C" int dt_adagrad_rows_step(float* table, float* acc, const int64_t* rows, float* values, int64_t n_rows, int D,
                                    int fields, void* slots, int64_t n_slots, int* mark, float lr, float eps, void* state,
                                    float* dense_p, const float* dense_g, float* dense_acc, int64_t dense_n, int advance,
                                    int slot_stride, void* stream) {
    const SlotHp h{lr, 0.f, 0.f, eps, 0.f};
    return slot_rows_step<kAdagrad>("dt_adagrad_rows_step", table, acc, nullptr, nullptr, rows, values, n_rows, D, fields, slots,
                                    n_slots, mark, h, state, dense_p, dense_g, dense_acc, nullptr, dense_n, advance, slot_stride,
                                    1, stream);
}

extern "C" int dt_rmsprop_dense_step(float* p, const float* g, float* rms, int64_t n, float lr, float rho, float eps,
                                     void* state, int advance, void* stream) {
    const SlotHp h{lr, rho, 0.f, eps, 0.f};
    return slot_dense_step<kRmsprop>("dt_rmsprop_dense_step", p, g, rms, nullptr, n, h, state, advance, stream);
}

extern "C" int dt_rmsprop_multi_step(int count, float* const* p, const float* const* g, float* const* rms, const int64_t* n,
                                     float lr, float rho, float eps, void* state, int advance, void* stream) {
    const SlotHp h{lr, rho, 0.f, eps, 0.f};
    return slot_multi_step<kRmsprop>("dt_rmsprop_multi_step", count, p, g, rms, nullptr, n, h, state, advance, stream);
}

extern "C" int dt_rmsprop_rows_step(float* table, float* rms, int* stamp, const int64_t* rows, float* values, int64_t n_rows,
                                    int D, int fields, void* slots, int64_t n_slots, int* mark, float lr, float rho, float eps,
                                    void* state, float* dense_p, const float* dense_g, float* dense_rms, int64_t dense_n,
                                    int advance, int slot_stride, int stamp_stride, void* stream) {
    const SlotHp h{lr, rho, 0.f, eps, 0.f};
    return slot_rows_step<kRmsprop>("dt_rmsprop_rows_step", table, rms, nullptr, stamp, rows, values, n_rows, D, fields, slots,
                                    n_slots, mark, h, state, dense_p, dense_g, dense_rms, nullptr, dense_n, advance, slot_stride,
                                    stamp_stride, stream);
}

extern "C" int dt_rmsprop_rows_materialize(float* rms, int* stamp, int64_t V, int D, int slot_stride, int stamp_stride,
                                           float rho, const void* state, void* stream) {
    DT_REQUIRE(V >= 0 && D > 0 && slot_stride >= D && stamp_stride >= 1, "dt_rmsprop_rows_materialize: bad sizes");
    if (V == 0) return DT_OK;
    DT_REQUIRE(rms && stamp && state, "dt_rmsprop_rows_materialize: null pointer");
    DT_REQUIRE(aligned_to(rms, 4) && aligned_to(stamp, 4), "dt_rmsprop_rows_materialize: misaligned pointer");
    hipStream_t st = as_stream(stream);
    int64_t blocks = (V * D + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(k_rms_materialize, dim3((unsigned)blocks), dim3(256), 0, st, rms, stamp, V, D, slot_stride, stamp_stride,
                       rho, (const AdamState*)state);
    blocks = (V + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(k_rms_restamp, dim3((unsigned)blocks), dim3(256), 0, st, stamp, V, stamp_stride, (const AdamState*)state);
    return launch_status("dt_rmsprop_rows_materialize");
}

extern "C" int dt_sgdm_dense_step(float* p, const float* g, float* mom, int64_t n, float lr, float momentum, int nesterov,
                                  void* state, int advance, void* stream) {
    const SlotHp h{lr, momentum, 0.f, 0.f, 0.f};
    return DT_SGDM(slot_dense_step)("dt_sgdm_dense_step", p, g, mom, nullptr, n, h, state, advance, stream);
}

extern "C" int dt_sgdm_multi_step(int count, float* const* p, const float* const* g, float* const* mom, const int64_t* n,
                                  float lr, float momentum, int nesterov, void* state, int advance, void* stream) {
    const SlotHp h{lr, momentum, 0.f, 0.f, 0.f};
    return DT_SGDM(slot_multi_step)("dt_sgdm_multi_step", count, p, g, mom, nullptr, n, h, state, advance, stream);
}

extern "C" int dt_sgdm_rows_step(float* table, float* mom, const int64_t* rows, float* values, int64_t n_rows, int D,
                                 int fields, void* slots, int64_t n_slots, int* mark, float lr, float momentum, int nesterov,
                                 void* state, float* dense_p, const float* dense_g, float* dense_mom, int64_t dense_n,
                                 int advance, int slot_stride, void* stream) {
    const SlotHp h{lr, momentum, 0.f, 0.f, 0.f};
    return DT_SGDM(slot_rows_step)("dt_sgdm_rows_step", table, mom, nullptr, nullptr, rows, values, n_rows, D, fields, slots,
                                   n_slots, mark, h, state, dense_p, dense_g, dense_mom, nullptr, dense_n, advance, slot_stride,
                                   1, stream);
}

extern "C" int dt_adamax_dense_step(float* p, const float* g, float* m, float* u, int64_t n, float lr, float beta1,
                                    float beta2, float eps, void* state, int advance, void* stream) {
    const SlotHp h{lr, beta1, beta2, eps, 0.f};
    return slot_dense_step<kAdamax>("dt_adamax_dense_step", p, g, m, u, n, h, state, advance, stream);
}

extern "C" int dt_adamax_multi_step(int count, float* const* p, const float* const* g, float* const* m, float* const* u,
                                    const int64_t* n, float lr, float beta1, float beta2, float eps, void* state,
                                    int advance, void* stream) {
    const SlotHp h{lr, beta1, beta2, eps, 0.f};
    return slot_multi_step<kAdamax>("dt_adamax_multi_step", count, p, g, m, u, n, h, state, advance, stream);
}

extern "C" int dt_adamax_rows_step(float* table, float* m, float* u, const int64_t* rows, float* values, int64_t n_rows,
                                   int D, int fields, void* slots, int64_t n_slots, int* mark, float lr, float beta1,
                                   float beta2, float eps, void* state, float* dense_p, const float* dense_g, float* dense_m,
                                   float* dense_u, int64_t dense_n, int advance, int slot_stride, void* stream) {
    const SlotHp h{lr, beta1, beta2, eps, 0.f};
    return slot_rows_step<kAdamax>("dt_adamax_rows_step", table, m, u, nullptr, rows, values, n_rows, D, fields, slots, n_slots,
                                   mark, h, state, dense_p, dense_g, dense_m, dense_u, dense_n, advance, slot_stride, 1, stream);
}

extern "C" int dt_ftrl_dense_step(float* p, const float* g, float* accum, float* linear, int64_t n, float lr, float lr_power,
                                  float l1, float l2, float l2_shrinkage, void* state, int advance, void* stream) {
    SlotHp h;
    if (!ftrl_hp("dt_ftrl_dense_step", lr, lr_power, l1, l2, l2_shrinkage, &h)) return DT_ERR_INVALID_ARG;
    return DT_FTRL(slot_dense_step)("dt_ftrl_dense_step", p, g, accum, linear, n, h, state, advance, stream);
}

extern "C" int dt_ftrl_multi_step(int count, float* const* p, const float* const* g, float* const* accum,
                                  float* const* linear, const int64_t* n, float lr, float lr_power, float l1, float l2,
                                  float l2_shrinkage, void* state, int advance, void* stream) {
    SlotHp h;
    if (!ftrl_hp("dt_ftrl_multi_step", lr, lr_power, l1, l2, l2_shrinkage, &h)) return DT_ERR_INVALID_ARG;
    return DT_FTRL(slot_multi_step)("dt_ftrl_multi_step", count, p, g, accum, linear, n, h, state, advance, stream);
}

extern "C" int dt_ftrl_rows_step(float* table, float* accum, float* linear, const int64_t* rows, float* values,
                                 int64_t n_rows, int D, int fields, void* slots, int64_t n_slots, int* mark, float lr,
                                 float lr_power, float l1, float l2, float l2_shrinkage, void* state, float* dense_p,
                                 const float* dense_g, float* dense_accum, float* dense_linear, int64_t dense_n, int advance,
                                 int slot_stride, void* stream) {
    SlotHp h;
    if (!ftrl_hp("dt_ftrl_rows_step", lr, lr_power, l1, l2, l2_shrinkage, &h)) return DT_ERR_INVALID_ARG;
    return DT_FTRL(slot_rows_step)("dt_ftrl_rows_step", table, accum, linear, nullptr, rows, values, n_rows, D, fields, slots,
                                   n_slots, mark, h, state, dense_p, dense_g, dense_accum, dense_linear, dense_n, advance,
                                   slot_stride, 1, stream);
}
