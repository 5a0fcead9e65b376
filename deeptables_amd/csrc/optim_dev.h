// optim_dev.h — what the optimizer translation units (optim.hip, optim_slots.hip) share beyond adam_dev.h: the step counter's
// read / advance for optimizers without a device-side rate, the multi-tensor launch geometry and pass 1 of every row step.
#pragma once
#include "common.h"
#include "adam_dev.h"

namespace dt {

// Several parameter tensors in ONE launch: the tensor descriptors travel as kernel arguments, a block finds its tensor by
// scanning the block offsets (k_adam_multi of optim.hip, k_slot_multi of optim_slots.hip)
constexpr int kMultiMax = 32;
constexpr int kMultiPerBlock = 1024;          // elements per block (256 threads x 4)

// t of the update this launch belongs to (1-based), read once per block; the step's last launch takes the arrival tickets
// (adam_finish's scheme) and its last block advances t
__device__ __forceinline__ int step_read_t(AdamState* st, int advance, unsigned& ticket) {
    __shared__ int s_t;
    ticket = kNoTicket;
    if (!st) return 0;
    if (threadIdx.x == 0) {
        s_t = st->t;
        if (advance) ticket = 0u;
    }
    __syncthreads();
    return s_t;
}
__device__ __forceinline__ void step_finish(AdamState* st, unsigned ticket) {
    if (ticket == kNoTicket) return;
    const unsigned k = blockIdx.x % kAdamSub;
    const unsigned expect = (gridDim.x + kAdamSub - 1 - k) / kAdamSub;
    if (atomicAdd(&st->sub[k], 1u) == expect - 1) {
        st->sub[k] = 0u;
        const unsigned groups = gridDim.x < (unsigned)kAdamSub ? gridDim.x : (unsigned)kAdamSub;
        if (atomicAdd(&st->done, 1u) == groups - 1) {
            st->done = 0u;
            st->t = st->t + 1;
        }
    }
}

inline bool aligned_to(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// Pass 1 of every row step (optim.hip: k_rows_dedupe / k_rows_dedupe_fields): merges the duplicate lookups of a row into its
// first occurrence (field-local LDS hashes or the global hash).  -> *gslots: the global hash the owners must clear (NULL: not
// used), *mk: the owner marks (NULL: fields = -1, the rows are already distinct and nothing is launched).  `who` names the
// entry point in the error text.
int rows_merge(const char* who, const int64_t* rows, float* values, int64_t n_rows, int D, int fields, void* slots,
               int64_t n_slots, int* mark, hipStream_t st, unsigned long long** gslots, int** mk);

}  // namespace dt
