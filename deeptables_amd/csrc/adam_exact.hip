// adam_exact.hip — Keras' DENSE Adam result on a row-sparse table (training.KerasAdam(exact_rows=True)).
//
// keras.optimizers.Adam applies its step to the densified embedding gradient (deepmodel.py:319-322): a row that was not looked
// up has gradient 0 and still takes the step,
//     m = b1*m ;  v = b2*v ;  p -= lr_t * m / (sqrt(v) + eps) ,   lr_t = lr * sqrt(1 - b2^t) / (1 - b1^t)   (t 1-based)
// Here such a row waits.  An int32 stamp per row holds the number of steps the row's p, m and v are current through; a row
// that is needed while c steps are complete owes k = c - stamp idle steps, and pays them before anything reads it:
//   * dt_adam_rows_catchup, ahead of the gather of a batch, for the rows the batch looks up,
//   * dt_adam_rows_materialize for every row of the table,
//   * dt_adam_rows_stamp, behind the step's row update (dt_adam_rows_step_seg, unchanged: for a row that is current it IS
//     Keras' dense step), marks the updated rows current through the step just completed.
// The idle steps have no closed form (eps, lr_t), but the loop is short: successive terms shrink by at most
// rho = sup_t (lr_{t+1} / lr_t) * b1 / sqrt(b2) < 1 (the host refuses other betas), so once a term leaves p unchanged and is
// below 2^-26 |p| no later one can change p either.  From there only m and v owe the rest of their decay: one
// powf each.  b1^t and b2^t are running products seeded by one powf each.  Every formula is evaluated in the order written,
// without contraction.  c is read from the DEVICE step state (AdamState.t - 1), so a captured graph replays these launches.
#include "common.h"
#include "adam_dev.h"
#include "optim_dev.h"

namespace dt {

struct ExactHp {
    float lr, b1, b2, eps;
};

constexpr float kExactExit = 1.f / 67108864.f;      // 2^-26

// VW elements of one row pay k idle steps; their state is current through step s (the steps paid are s + 1 .. s + k).
// No memory operation in here: lanes of a wave leave the loop at different trips, which costs ALU time only.
template <int VW>
__device__ __forceinline__ void adam_idle_steps(float (&p)[VW], float (&m)[VW], float (&v)[VW], int s, int k,
                                                const ExactHp& h) {
#pragma clang fp contract(off)
    float c1 = powf(h.b1, (float)s), c2 = powf(h.b2, (float)s);      // b1^t, b2^t as running products
    int paid[VW];                                                    // idle steps whose term was applied; -1: still in the loop
#pragma unroll
    for (int e = 0; e < VW; ++e) paid[e] = -1;
    for (int j = 0; j < k; ++j) {
        c1 *= h.b1;
        c2 *= h.b2;
        const float lr_t = h.lr * sqrtf(1.f - c2) / (1.f - c1);
        bool any = false;
#pragma unroll
        for (int e = 0; e < VW; ++e) {
            if (paid[e] >= 0) continue;
            m[e] = h.b1 * m[e];
            v[e] = h.b2 * v[e];
            const float term = lr_t * m[e] / (sqrtf(v[e]) + h.eps);
            const float pn = p[e] - term;
            const bool same = pn == p[e];
            p[e] = pn;
            if (term == 0.f || (same && fabsf(term) < kExactExit * fabsf(pn)))
                paid[e] = j + 1;
            else
                any = true;
        }
        if (!any) break;
    }
#pragma unroll
    for (int e = 0; e < VW; ++e) {
        const int rest = paid[e] < 0 ? 0 : k - paid[e];
        if (rest > 0) {
            m[e] *= powf(h.b1, (float)rest);
            v[e] *= powf(h.b2, (float)rest);
        }
    }
}

// One thread group per row, k_slot_rows_owner's geometry (optim_slots.hip): T = min(D / VW, 256) threads per row, 256 / T whole
// rows per block, a row never straddles two blocks.  The group's first lane claims the row — an integer atomicExch of its
// stamp to c — and hands the old value to the group through LDS.  Old value c: another group of this launch owns the row (a row
// looked up twice in the batch) or nothing is pending: the group leaves.  Whatever reads the row is a later launch of the
// stream, so duplicates need no merge.
// KIND = DT_IDX_*: the rows are the batch's lookups [n = B F], resolved as the gather resolves them (an id outside
// [0, vocab[f]) touches nothing).  KIND = -1: the rows are 0 .. n - 1 (the sweep); a lane whose m and v are all zero — every
// lane of a row that was never looked up — stores nothing.
template <int VW, int KIND>
__global__ __launch_bounds__(256) void k_adam_catchup(float* __restrict__ table, float* __restrict__ m,
                                                      float* __restrict__ v, int* __restrict__ stamp,
                                                      const void* __restrict__ idx, const int64_t* __restrict__ row_offset,
                                                      const int32_t* __restrict__ vocab, int64_t n, int F, int D, int64_t V,
                                                      int sstride, ExactHp h, const AdamState* __restrict__ st) {
    __shared__ int s_old[256];
    const int c = st->t - 1;                                  // steps completed
    const int lpr = D / VW;                                   // pieces (VW floats) per row
    const int T = lpr < 256 ? lpr : 256, rpb = 256 / T;
    const int r = (int)threadIdx.x / T, q0 = (int)threadIdx.x - r * T;
    // (the trip count is the same for every thread of a block: the barrier below is reached by all of them)
    for (int64_t base = (int64_t)blockIdx.x * rpb; base < n; base += (int64_t)gridDim.x * rpb) {
        const int64_t occ = base + r;
        int64_t row = -1;
        if (r < rpb && occ < n) {
            if (KIND < 0) {
                row = occ;
            } else {
                const int f = (int)(occ % F);
                const int id = load_id<(KIND < 0 ? DT_IDX_I32 : KIND)>(idx, occ);
                if ((unsigned)id < (unsigned)vocab[f]) row = row_offset[f] + id;
            }
            if (row >= V) row = -1;
        }
        if (row >= 0 && q0 == 0) s_old[r] = atomicExch(stamp + row, c);
        __syncthreads();
        const int old = row >= 0 ? s_old[r] : c;
        __syncthreads();                                      // (the next trip's claim rewrites s_old)
        const int k = c - old;
        if (k <= 0) continue;
        float* prow = table + row * D;
        float* mrow = m + row * sstride;
        float* vrow = v + row * sstride;
        for (int q = q0; q < lpr; q += T) {                   // (more than 256 pieces per row: the thread walks the rest)
            float pi[VW], mi[VW], vi[VW];
            if (VW == 4) {
                *reinterpret_cast<float4*>(mi) = *reinterpret_cast<const float4*>(mrow + q * 4);
                *reinterpret_cast<float4*>(vi) = *reinterpret_cast<const float4*>(vrow + q * 4);
                *reinterpret_cast<float4*>(pi) = *reinterpret_cast<const float4*>(prow + q * 4);
            } else {
                mi[0] = mrow[q]; vi[0] = vrow[q]; pi[0] = prow[q];
            }
            bool zero = true;
#pragma unroll
            for (int e = 0; e < VW; ++e) zero = zero && mi[e] == 0.f && vi[e] == 0.f;
            if (zero) continue;                               // m = v = 0 owes nothing: every term is 0
            adam_idle_steps<VW>(pi, mi, vi, old, k, h);
            if (VW == 4) {
                *reinterpret_cast<float4*>(mrow + q * 4) = *reinterpret_cast<float4*>(mi);
                *reinterpret_cast<float4*>(vrow + q * 4) = *reinterpret_cast<float4*>(vi);
                *reinterpret_cast<float4*>(prow + q * 4) = *reinterpret_cast<float4*>(pi);
            } else {
                mrow[q] = mi[0]; vrow[q] = vi[0]; prow[q] = pi[0];
            }
        }
    }
}

// stamp[row] = the steps completed, for the rows the step just updated (the step's last update has advanced the state)
__global__ __launch_bounds__(256) void k_adam_stamp(int* __restrict__ stamp, const int64_t* __restrict__ rows, int64_t n,
                                                    int64_t V, const AdamState* __restrict__ st) {
    const int done = st->t - 1;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = rows[i];
        if (row >= 0 && row < V) stamp[row] = done;
    }
}

static bool exact_hp_ok(float lr, float b1, float b2, float eps) {
    return lr >= 0.f && b1 >= 0.f && b1 < 1.f && b2 > 0.f && b2 < 1.f && eps >= 0.f && b1 * b1 < b2;
}

template <int KIND>
static int catchup_launch(const char* who, float* table, float* m, float* v, int* stamp, const void* idx,
                          const int64_t* row_offset, const int32_t* vocab, int64_t n, int F, int D, int64_t V, int slot_stride,
                          float lr, float b1, float b2, float eps, const void* state, void* stream) {
    DT_REQUIRE(n >= 0 && D > 0 && V >= 0 && slot_stride >= D, "%s: bad sizes", who);
    DT_REQUIRE(exact_hp_ok(lr, b1, b2, eps), "%s: needs lr >= 0, eps >= 0, 0 <= beta1 < 1, 0 < beta2 < 1 and beta1 < sqrt(beta2)", who);
    if (n == 0 || V == 0) return DT_OK;
    DT_REQUIRE(table && m && v && stamp && state, "%s: null pointer", who);
    DT_REQUIRE(aligned_to(table, 4) && aligned_to(m, 4) && aligned_to(v, 4) && aligned_to(stamp, 4) && aligned_to(state, 4),
               "%s: misaligned pointer", who);
    DT_REQUIRE(v >= m + D || m >= v + D, "%s: the slots of a row overlap", who);
    const bool vec = D % 4 == 0 && slot_stride % 4 == 0 && aligned_to(table, 16) && aligned_to(m, 16) && aligned_to(v, 16);
    const int lpr = vec ? D / 4 : D;
    const int rpb = 256 / (lpr < 256 ? lpr : 256);
    int64_t blocks = (n + rpb - 1) / rpb;
    if (blocks > 256 * 256) blocks = 256 * 256;               // (the kernel strides over the rest)
    const ExactHp h{lr, b1, b2, eps};
    const dim3 grid((unsigned)blocks);
    if (vec)
        hipLaunchKernelGGL((k_adam_catchup<4, KIND>), grid, dim3(256), 0, as_stream(stream), table, m, v, stamp, idx, row_offset,
                           vocab, n, F, D, V, slot_stride, h, (const AdamState*)state);
    else
        hipLaunchKernelGGL((k_adam_catchup<1, KIND>), grid, dim3(256), 0, as_stream(stream), table, m, v, stamp, idx, row_offset,
                           vocab, n, F, D, V, slot_stride, h, (const AdamState*)state);
    return launch_status(who);
}

}  // namespace dt

using namespace dt;

extern "C" int dt_adam_exact_supported(int D) { return D >= 1 ? 1 : 0; }

extern "C" int dt_adam_rows_catchup(float* table, float* m, float* v, int slot_stride, int* stamp, const void* idx,
                                    int idx_kind, const int64_t* row_offset, const int32_t* vocab, int B, int F, int D,
                                    int64_t V, float lr, float beta1, float beta2, float eps, const void* state,
                                    void* stream) {
    const char* who = "dt_adam_rows_catchup";
    DT_REQUIRE(B >= 0 && F >= 0, "%s: bad sizes B=%d F=%d", who, B, F);
    DT_REQUIRE(idx_kind == DT_IDX_F32 || idx_kind == DT_IDX_I32, "%s: idx_kind %d", who, idx_kind);
    const int64_t n = (int64_t)B * F;
    DT_REQUIRE(n == 0 || (idx && row_offset && vocab), "%s: null pointer", who);
    DT_REQUIRE(aligned_to(idx, 4) && aligned_to(row_offset, 8) && aligned_to(vocab, 4), "%s: misaligned ids / row_offset / vocab",
               who);
    if (idx_kind == DT_IDX_F32)
        return catchup_launch<DT_IDX_F32>(who, table, m, v, stamp, idx, row_offset, vocab, n, F, D, V, slot_stride, lr, beta1,
                                          beta2, eps, state, stream);
    return catchup_launch<DT_IDX_I32>(who, table, m, v, stamp, idx, row_offset, vocab, n, F, D, V, slot_stride, lr, beta1, beta2,
                                      eps, state, stream);
}

extern "C" int dt_adam_rows_materialize(float* table, float* m, float* v, int slot_stride, int* stamp, int64_t V, int D,
                                        float lr, float beta1, float beta2, float eps, const void* state, void* stream) {
    return catchup_launch<-1>("dt_adam_rows_materialize", table, m, v, stamp, nullptr, nullptr, nullptr, V, 1, D, V, slot_stride,
                              lr, beta1, beta2, eps, state, stream);
}

extern "C" int dt_adam_rows_stamp(int* stamp, const int64_t* rows, int64_t n, int64_t V, const void* state, void* stream) {
    DT_REQUIRE(n >= 0 && V >= 0, "dt_adam_rows_stamp: bad sizes");
    if (n == 0 || V == 0) return DT_OK;
    DT_REQUIRE(stamp && rows && state, "dt_adam_rows_stamp: null pointer");
    DT_REQUIRE(aligned_to(stamp, 4) && aligned_to(rows, 8) && aligned_to(state, 4), "dt_adam_rows_stamp: misaligned pointer");
    int64_t blocks = (n + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(k_adam_stamp, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), stamp, rows, n, V,
                       (const AdamState*)state);
    return launch_status("dt_adam_rows_stamp");
}
