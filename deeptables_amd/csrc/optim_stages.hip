// optim_stages.hip — the two stages of keras.optimizers' BaseOptimizer that sit around every optimizer's update: decoupled
// weight decay ahead of it (`weight_decay`, BaseOptimizer._apply_weight_decay) and the exponential moving average of the
// weights behind it (`use_ema` / `ema_momentum`), float32, each formula in ONE function compiled without contraction:
//
//   decay                       p = p - (p * wd) * lr                 (lr: the optimizer's plain learning rate)
//   average, step t (1-based)   a = m_eff * a + (1 - m_eff) * p       m_eff = 0 at t == 1, ema_momentum afterwards
//   a row that sat out k steps  a = w + m^k * (a - w)                 (k dense average steps on its constant weight w)
//
// The stage counts its own steps on the device (StageState: plain SGD has no step state to borrow), so a captured graph replays
// every launch with the right m_eff and the right stamps; dt_stage_advance, a one-thread launch, ends the step.
// Dense tensors: multi-tensor launches over (pointer, n) regions in chunks of kMultiMax, k_slot_multi's geometry
// (optim_slots.hip), a float4 body with a scalar tail where the region's pointers are 16-byte aligned and scalar otherwise.
// Row-sparse tables: one launch ahead of the row update and one behind it over the DISTINCT rows dt_rows_coalesce emits
// (ascending, then -1: skipped), k_slot_rows_owner's row geometry.  The average of such a table is exact with respect to the
// weights' own trajectory: an int32 stamp per row holds the step at which the row's average was last written, and the launch
// ahead of the update first applies the k = t - 1 - stamp steps the row sat out — RMSprop's stamps (k_rms_rows_owner) with the
// weight in the place of zero.  No host synchronisation anywhere.
#include <stdlib.h>
#include "common.h"
#include "optim_dev.h"

namespace dt {

struct StageState {             // DT_STAGE_STATE_BYTES
    int done;                   // steps the stage has completed: the step in flight is done + 1
    int pad[3];
};

__device__ __forceinline__ float decay_one(float p, float wd, float lr) {
#pragma clang fp contract(off)
    return p - (p * wd) * lr;
}

__device__ __forceinline__ float ema_one(float a, float p, float m) {
#pragma clang fp contract(off)
    return m * a + (1.f - m) * p;
}

// m^idle as RMSprop's lazy decay takes rho^idle (decay_factor / decayed of optim_slots.hip, kept as a copy: that translation
// unit's bits are pinned by its golden test): short gaps repeat the multiplication a dense step makes, longer ones one powf
constexpr int kExactSteps = 8;
__device__ __forceinline__ float idle_factor(float m, int idle) {
    return idle > kExactSteps ? powf(m, (float)idle) : 1.f;
}
__device__ __forceinline__ float catch_up(float a, float w, float m, int idle, float factor) {
#pragma clang fp contract(off)
    if (idle <= 0) return a;
    float d = a - w;
    if (idle > kExactSteps) {
        d = d * factor;
    } else {
        for (int k = 0; k < idle; ++k) d = d * m;
    }
    return w + d;
}

__global__ void k_stage_state_init(StageState* st, int done) {
    st->done = done;
    st->pad[0] = st->pad[1] = st->pad[2] = 0;
}
__global__ void k_stage_advance(StageState* st) { st->done = st->done + 1; }

struct StageMulti {             // SlotMulti of optim_slots.hip: a: the averages (unused by the decay)
    float* p[kMultiMax];
    float* a[kMultiMax];
    int n[kMultiMax];
    int vec[kMultiMax];         // p (and a) 16-byte aligned: the float4 body
    int block_start[kMultiMax + 1];
    int count;
};

// EMA = false: the decay of p; true: the average a of p (p is only read)
template <bool EMA>
__global__ __launch_bounds__(256) void k_stage_multi(StageMulti d, float c0, float c1, const StageState* __restrict__ st) {
    int t = 0;
    while (t + 1 < d.count && (int)blockIdx.x >= d.block_start[t + 1]) ++t;
    float m = 0.f;
    if (EMA) m = st->done == 0 ? 0.f : c0;
    const int b0 = (int)(blockIdx.x - d.block_start[t]) * kMultiPerBlock;
    const int end = min(d.n[t], b0 + kMultiPerBlock);
    float* p = d.p[t];
    float* a = d.a[t];
    const int n4 = d.vec[t] ? (end - b0) >> 2 : 0;              // (b0 is a multiple of 1024: the block's start is aligned too)
    for (int i = (int)threadIdx.x; i < n4; i += 256) {
        float4 p4 = reinterpret_cast<float4*>(p + b0)[i];
        if (EMA) {
            float4 a4 = reinterpret_cast<float4*>(a + b0)[i];
            a4.x = ema_one(a4.x, p4.x, m); a4.y = ema_one(a4.y, p4.y, m);
            a4.z = ema_one(a4.z, p4.z, m); a4.w = ema_one(a4.w, p4.w, m);
            reinterpret_cast<float4*>(a + b0)[i] = a4;
        } else {
            p4.x = decay_one(p4.x, c0, c1); p4.y = decay_one(p4.y, c0, c1);
            p4.z = decay_one(p4.z, c0, c1); p4.w = decay_one(p4.w, c0, c1);
            reinterpret_cast<float4*>(p + b0)[i] = p4;
        }
    }
    for (int i = b0 + 4 * n4 + (int)threadIdx.x; i < end; i += 256) {
        if (EMA) a[i] = ema_one(a[i], p[i], m);
        else p[i] = decay_one(p[i], c0, c1);
    }
}

// the field of a packed table's row: the last f with row_offset[f] <= row (row_offset ascending from 0)
__device__ __forceinline__ int field_of(const int64_t* __restrict__ row_offset, int F, int64_t row) {
    int lo = 0, hi = F - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (row_offset[mid] <= row) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// Ahead of the row update (PRE): the average catches up with the steps the row sat out, then the row decays — unless its
// field is switched off (field_on, NULL: every field decays).  Behind it (!PRE): the step's own average step, and the stamp.
// T = min(D / VW, 256) threads per row and 256 / T whole rows per block, rows with more than 256 pieces walked: a row never
// straddles two blocks.  Stamps are read ahead of the update and written behind it: no launch does both.
template <bool PRE, int VW>
__global__ __launch_bounds__(256) void k_stage_rows(float* __restrict__ table, float* __restrict__ avg, int* __restrict__ stamp,
                                                    const int64_t* __restrict__ rows, int64_t n, int D, int64_t V,
                                                    const int64_t* __restrict__ row_offset,
                                                    const int* __restrict__ field_on, int F, int decay, float wd, float lr,
                                                    float mom, const StageState* __restrict__ st) {
    const int lpr = D / VW;                                   // pieces (VW floats) per row
    const int T = lpr < 256 ? lpr : 256, rpb = 256 / T;
    const int r = (int)threadIdx.x / T, q0 = (int)threadIdx.x - r * T;
    const int64_t occ = (int64_t)blockIdx.x * rpb + r;
    if (r >= rpb || occ >= n) return;
    const int64_t row = rows[occ];
    if (row < 0 || row >= V) return;                          // the -1 behind the distinct rows
    const int done = avg ? st->done : 0;
    int idle = 0;
    float factor = 1.f, m = 0.f;
    if (PRE) {
        if (avg) {
            idle = done - stamp[row];
            factor = idle_factor(mom, idle);
        }
        if (decay && field_on) decay = field_on[field_of(row_offset, F, row)];
    } else {
        m = done == 0 ? 0.f : mom;
    }
    float* prow = table + row * D;
    float* arow = avg ? avg + row * D : nullptr;
    for (int q = q0; q < lpr; q += T) {                       // (more than 256 pieces per row: the thread walks the rest)
        float pi[VW], ai[VW];
        if (VW == 4) {
            *reinterpret_cast<float4*>(pi) = *reinterpret_cast<const float4*>(prow + q * 4);
            if (avg) *reinterpret_cast<float4*>(ai) = *reinterpret_cast<const float4*>(arow + q * 4);
        } else {
            pi[0] = prow[q];
            if (avg) ai[0] = arow[q];
        }
#pragma unroll
        for (int k = 0; k < VW; ++k) {
            if (PRE) {
                if (avg) ai[k] = catch_up(ai[k], pi[k], mom, idle, factor);
                if (decay) pi[k] = decay_one(pi[k], wd, lr);
            } else {
                ai[k] = ema_one(ai[k], pi[k], m);
            }
        }
        if (VW == 4) {
            if (avg && (!PRE || idle > 0)) *reinterpret_cast<float4*>(arow + q * 4) = *reinterpret_cast<float4*>(ai);
            if (PRE && decay) *reinterpret_cast<float4*>(prow + q * 4) = *reinterpret_cast<float4*>(pi);
        } else {
            if (avg && (!PRE || idle > 0)) arow[q] = ai[0];
            if (PRE && decay) prow[q] = pi[0];
        }
    }
    if (!PRE && q0 == 0) stamp[row] = done + 1;
}

// The steps pending on every row applied to its average, then every stamp = steps done.  Two launches, so that no thread
// reads a stamp another has rewritten (k_rms_materialize / k_rms_restamp).
__global__ __launch_bounds__(256) void k_stage_materialize(const float* __restrict__ table, float* __restrict__ avg,
                                                           const int* __restrict__ stamp, int64_t V, int D, float mom,
                                                           const StageState* __restrict__ st) {
    const int done = st->done;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < V * D; i += (int64_t)gridDim.x * blockDim.x) {
        const int idle = done - stamp[i / D];
        if (idle > 0) avg[i] = catch_up(avg[i], table[i], mom, idle, idle_factor(mom, idle));
    }
}
__global__ __launch_bounds__(256) void k_stage_restamp(int* __restrict__ stamp, int64_t V, const StageState* __restrict__ st) {
    const int done = st->done;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < V; i += (int64_t)gridDim.x * blockDim.x)
        stamp[i] = done;
}

// ---- host side ---------------------------------------------------------------------------------------------------------------
template <bool EMA>
static int stage_multi(const char* who, int count, float* const* p, float* const* a, const int64_t* n, float c0, float c1,
                       const void* state, void* stream) {
    DT_REQUIRE(count >= 0 && (count == 0 || (p && n && (!EMA || a))), "%s: bad arguments", who);
    DT_REQUIRE(!EMA || count == 0 || state, "%s: the step number is read from the device state", who);
    for (int t = 0; t < count; ++t)          // every tensor is checked before the first chunk is launched
        DT_REQUIRE(n[t] >= 0 && n[t] < (1LL << 31) && (n[t] == 0 || (p[t] && (!EMA || a[t]))) && aligned_to(p[t], 4) &&
                       (!EMA || aligned_to(a[t], 4)),
                   "%s: tensor %d: bad size, null or misaligned pointer", who, t);
    bool launched = false;
    for (int c = 0; c < count; c += kMultiMax) {
        StageMulti d;
        d.count = count - c < kMultiMax ? count - c : kMultiMax;
        int blocks = 0;
        for (int t = 0; t < d.count; ++t) {
            d.p[t] = p[c + t];
            d.a[t] = EMA ? a[c + t] : nullptr;
            d.n[t] = (int)n[c + t];
            d.vec[t] = aligned_to(d.p[t], 16) && (!EMA || aligned_to(d.a[t], 16)) ? 1 : 0;
            d.block_start[t] = blocks;
            blocks += (int)((n[c + t] + kMultiPerBlock - 1) / kMultiPerBlock);
        }
        d.block_start[d.count] = blocks;
        if (blocks == 0) continue;
        hipLaunchKernelGGL(k_stage_multi<EMA>, dim3(blocks), dim3(256), 0, as_stream(stream), d, c0, c1,
                           (const StageState*)state);
        launched = true;
    }
    return launched ? launch_status(who) : DT_OK;
}

template <bool PRE>
static int stage_rows(const char* who, float* table, float* avg, int* stamp, const int64_t* rows, int64_t n, int D, int64_t V,
                      const int64_t* row_offset, const int* field_on, int F, int decay, float wd, float lr, float mom,
                      const void* state, void* stream) {
    DT_REQUIRE(n >= 0 && D > 0 && V >= 0 && F >= 0, "%s: bad sizes", who);
    if (n == 0 || V == 0 || (!avg && !decay)) return DT_OK;
    DT_REQUIRE(n < (1LL << 31), "%s: %lld rows do not fit the 32-bit grid", who, (long long)n);
    DT_REQUIRE(table && rows, "%s: null pointer", who);
    DT_REQUIRE(!avg || (stamp && state), "%s: an average needs its stamps and the device state", who);
    DT_REQUIRE(!field_on || (row_offset && F >= 1), "%s: field_on needs row_offset and F >= 1", who);
    const bool vec = D % 4 == 0;
    const size_t al = vec ? 16 : 4;
    DT_REQUIRE(aligned_to(table, al) && aligned_to(avg, al), "%s: table and average must be %d-byte aligned (D = %d)", who,
               (int)al, D);
    DT_REQUIRE(aligned_to(rows, 8) && aligned_to(row_offset, 8) && aligned_to(stamp, 4) && aligned_to(field_on, 4),
               "%s: misaligned rows / row_offset / stamp / field_on", who);
    const int lpr = vec ? D / 4 : D;
    const int rpb = 256 / (lpr < 256 ? lpr : 256);
    const dim3 grid((unsigned)((n + rpb - 1) / rpb));
    if (vec)
        hipLaunchKernelGGL((k_stage_rows<PRE, 4>), grid, dim3(256), 0, as_stream(stream), table, avg, stamp, rows, n, D, V,
                           row_offset, field_on, F, decay, wd, lr, mom, (const StageState*)state);
    else
        hipLaunchKernelGGL((k_stage_rows<PRE, 1>), grid, dim3(256), 0, as_stream(stream), table, avg, stamp, rows, n, D, V,
                           row_offset, field_on, F, decay, wd, lr, mom, (const StageState*)state);
    return launch_status(who);
}

static bool finite_nonneg(float v) { return v >= 0.f && v <= 3.402823466e38f; }

}  // namespace dt

using namespace dt;

extern "C" int dt_stage_state_init(void* state, int steps_done, void* stream) {
    DT_REQUIRE(state && aligned_to(state, 4) && steps_done >= 0, "dt_stage_state_init: bad arguments");
    hipLaunchKernelGGL(k_stage_state_init, dim3(1), dim3(1), 0, as_stream(stream), (StageState*)state, steps_done);
    return launch_status("dt_stage_state_init");
}

extern "C" int dt_stage_advance(void* state, void* stream) {
    DT_REQUIRE(state && aligned_to(state, 4), "dt_stage_advance: null or misaligned state");
    hipLaunchKernelGGL(k_stage_advance, dim3(1), dim3(1), 0, as_stream(stream), (StageState*)state);
    return launch_status("dt_stage_advance");
}

extern "C" int dt_decay_multi(int count, float* const* p, const int64_t* n, float weight_decay, float lr, void* stream) {
    DT_REQUIRE(finite_nonneg(weight_decay) && lr == lr, "dt_decay_multi: weight_decay must be a finite number >= 0");
    return stage_multi<false>("dt_decay_multi", count, p, nullptr, n, weight_decay, lr, nullptr, stream);
}

extern "C" int dt_ema_multi(int count, const float* const* p, float* const* avg, const int64_t* n, float momentum,
                            const void* state, void* stream) {
    DT_REQUIRE(momentum >= 0.f && momentum <= 1.f, "dt_ema_multi: momentum must be in [0, 1]");
    return stage_multi<true>("dt_ema_multi", count, const_cast<float* const*>(p), avg, n, momentum, 0.f, state, stream);
}

extern "C" int dt_rows_stage_pre(float* table, float* avg, const int* stamp, const int64_t* rows, int64_t n, int D, int64_t V,
                                 const int64_t* row_offset, const int* field_on, int F, int decay, float weight_decay,
                                 float lr, float momentum, const void* state, void* stream) {
    DT_REQUIRE(!decay || (finite_nonneg(weight_decay) && lr == lr),
               "dt_rows_stage_pre: weight_decay must be a finite number >= 0");
    DT_REQUIRE(!avg || (momentum >= 0.f && momentum <= 1.f), "dt_rows_stage_pre: momentum must be in [0, 1]");
    return stage_rows<true>("dt_rows_stage_pre", table, avg, const_cast<int*>(stamp), rows, n, D, V, row_offset, field_on, F,
                            decay ? 1 : 0, weight_decay, lr, momentum, state, stream);
}

extern "C" int dt_rows_stage_post(const float* table, float* avg, int* stamp, const int64_t* rows, int64_t n, int D, int64_t V,
                                  float momentum, const void* state, void* stream) {
    DT_REQUIRE(momentum >= 0.f && momentum <= 1.f, "dt_rows_stage_post: momentum must be in [0, 1]");
    DT_REQUIRE(n <= 0 || V <= 0 || avg, "dt_rows_stage_post: null average");
    return stage_rows<false>("dt_rows_stage_post", const_cast<float*>(table), avg, stamp, rows, n, D, V, nullptr, nullptr, 0, 0,
                             0.f, 0.f, momentum, state, stream);
}

extern "C" int dt_ema_rows_materialize(const float* table, float* avg, int* stamp, int64_t V, int D, float momentum,
                                       const void* state, void* stream) {
    DT_REQUIRE(V >= 0 && D > 0, "dt_ema_rows_materialize: bad sizes");
    DT_REQUIRE(momentum >= 0.f && momentum <= 1.f, "dt_ema_rows_materialize: momentum must be in [0, 1]");
    if (V == 0) return DT_OK;
    DT_REQUIRE(table && avg && stamp && state, "dt_ema_rows_materialize: null pointer");
    DT_REQUIRE(aligned_to(table, 4) && aligned_to(avg, 4) && aligned_to(stamp, 4), "dt_ema_rows_materialize: misaligned pointer");
    hipStream_t st = as_stream(stream);
    int64_t blocks = (V * D + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(k_stage_materialize, dim3((unsigned)blocks), dim3(256), 0, st, table, avg, stamp, V, D, momentum,
                       (const StageState*)state);
    blocks = (V + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(k_stage_restamp, dim3((unsigned)blocks), dim3(256), 0, st, stamp, V, (const StageState*)state);
    return launch_status("dt_ema_rows_materialize");
}
