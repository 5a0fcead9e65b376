// cell_hash.h — the counter hash of the dropout masks that need no mask tensor (csrc/cell.hip, csrc/emb_dropout.hip):
// an element is kept iff hash(seed word, per-layer salt, row, col) >= threshold(rate).  Rows and columns are separate 32-bit
// words, so no flat element index enters the hash, and the word is built head -> row -> col: a kernel computes each stage
// once for everything that shares it.  ops.cell_dropout_hash / cell_dropout_threshold are the Python mirrors.
#pragma once

namespace dt {

__host__ __device__ inline unsigned cell_mix(unsigned x) {           // the finalizer of ai_hash (csrc/autoint.hip)
    x ^= x >> 16; x *= 0x7FEB352Du; x ^= x >> 15; x *= 0x846CA68Bu; x ^= x >> 16;
    return x;
}
// the part that is the same for every element of a launch
__host__ __device__ inline unsigned cell_hash_head(unsigned seed, unsigned salt) { return cell_mix(seed ^ (salt * 0x9E3779B1u)); }
// row, then column, each through a bijection of the running word: two elements of one launch collide only by chance
__host__ __device__ inline unsigned cell_hash_row(unsigned head, unsigned row) { return cell_mix(head ^ (row * 0x85EBCA77u)); }
__host__ __device__ inline unsigned cell_hash_col(unsigned row_word, unsigned col) { return cell_mix(row_word ^ (col * 0xC2B2AE3Du)); }
__host__ __device__ inline unsigned cell_hash_tail(unsigned head, unsigned row, unsigned col) {
    return cell_hash_col(cell_hash_row(head, row), col);
}
// keep iff hash >= thr, thr = rate * 2^32 saturated
inline unsigned cell_threshold(float rate) {
    const double t = (double)rate * 4294967296.0;
    return t >= 4294967295.0 ? 4294967295u : (t <= 0.0 ? 0u : (unsigned)t);
}

}  // namespace dt
