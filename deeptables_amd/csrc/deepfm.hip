// deepfm.hip — the whole DeepFM / DCN train step (forward + loss + backward + Keras Adam) as FOUR fused launches
// (five for a step that prepares itself; rounds 3-4: six).
//
// DeepFM = nets ['linear','fm_nets','dnn_nets'] (deeptables/models/deepnets.py:15) assembled by
// DeepModel.__build_model (deeptables/models/deepmodel.py:259-317):
//   emb   = MultiColumnEmbedding(cat)                                   layers.py:889-904
//   x     = Concatenate([Flatten(Concatenate(emb)), dense])             deepmodel.py:269-274,348-353
//   xn    = BatchNormalization('bn_concat_emb_dense')(x)                deepmodel.py:359
//   lin   = Dense(1,no bias)(Concatenate([sum_D(emb), dense]))          deepnets.py:43-66
//   fm    = FM()(Concatenate(emb, axis=1))                              layers.py:53-62
//   dnn   = Dense(1,no bias)(relu(Dense(64)(relu(Dense(128)(xn)))))     deepnets.py:401-427, deepmodel.py:291-292
//   logit = Dense(1, bias)(Add([lin, fm, dnn]))  (sigmoid applied by the loss)   deepmodel.py:296-297,455
// The reference runs this as ~100 small TF ops per step; the layer-by-layer path of this repo as ~60 launches.  Here
// (details in front of the kernels):
//   A   k_sparse_fwd    gather + FM + linear + concat row X + field sums S + the batch sums of BatchNormalization (double
//                       atomics into sharded accumulators: bnacc); chained steps: + the NEXT step's packed rows
//   [B  k_prep          the in-step dedupe's election + the tile kernel's weight layouts — only in a step that was not
//                       prepared by the one before it (DT_STEP_PREPARED)]
//   C   k_tower_x3      (tower_x3.h; exact fp32: k_mlp_fwd3) mean / rstd from bnacc, BN, Dense128, Dense64, logits, loss, dz,
//                       dH2, dH1, dXn = dH1 W1^T with the two BN-backward column sums; the tile's record sums -> racc (atomics)
//   E|D k_wgrad_rows    waves 0-3: Xhat^T dH1 and H1^T dH2 batch slices (fp32 MFMA), then the NEXT step's election (chained);
//                       waves 4-7: row gradients + in-place Keras Adam of the rows looked up once
//   F   k_finish_step   segments (rows looked up several times), record entries + slices -> dense gradients + Adam, the NEXT
//                       step's bf16 weight layouts (chained), the step state
// Dense gradients are deterministic: per-slice partials + one pass, and the batch sums are double-precision atomics of fp32
// addends (exact unless their magnitudes span 2^23: the totals do not depend on the order of arrival).
#include <stdlib.h>
#include "tile_common.h"
#include "tower_x3.h"
#include "adam_dev.h"

namespace dt {

typedef float floatx4_t __attribute__((ext_vector_type(4)));

// accumulator buffer layout (floats), zeroed once per step by one memset
struct DeepFmAccum {
    int64_t dW1, dW2, db1, db2, dw3, dwo, dbo, loss, dgamma, dbeta, dwlin, slin, total;
    // DCN (cross layers L > 0; see dt_dcn_train_step): dw3 then holds the [C + 64] kernel applied to Concatenate([cross, dnn]) (cross
    // part first, Concatenate([cross, dnn]) order) and dw3d points at its dnn part; cross kernels / biases [L][C];
    // scratch: the cross path's two BN-backward column sums
    int64_t dw3d, dcw, dcb, sumc, sumcx;
};
__host__ __device__ inline DeepFmAccum deepfm_accum_layout(int C, int CP, int F, int Nd, int L = 0) {
    DeepFmAccum a;
    int64_t o = 0;
    a.dW1 = o; o += (int64_t)C * kH1;
    a.dW2 = o; o += (int64_t)kH1 * kH2;
    a.db1 = o; o += kH1;
    a.db2 = o; o += kH2;
    a.dw3 = o; o += (L > 0 ? C : 0);
    a.dw3d = o; o += kH2;
    a.dwo = o; o += 1;
    a.dbo = o; o += 1;
    a.loss = o; o += 2;
    a.dgamma = o; o += CP;   // = sum_b dXn * xhat   (also the BN-backward column sum)
    a.dbeta = o; o += CP;    // = sum_b dXn
    a.dwlin = o; o += (L > 0 ? 0 : F + Nd);
    a.dcw = o; o += (int64_t)L * C;
    a.dcb = o; o += (int64_t)L * C;
    o = (o + 3) & ~(int64_t)3;
    a.slin = o; o += (L > 0 ? 0 : CP);     // scratch: sum_b dz * X per column (field-reduced into dwlin by kernel E')
    a.sumc = o; o += (L > 0 ? CP : 0);
    a.sumcx = o; o += (L > 0 ? CP : 0);
    a.total = (o + 3) & ~(int64_t)3;
    return a;
}

// Optional row dedupe inside the step (dt_deepfm_train_step, dedupe_ws != NULL): the sparse gradient leaves the step as
//   * (rows_out, grad_rows) entries for the rows looked up ONCE in the batch, and
//   * SEGMENTS for the rows looked up several times: (table row, offset, count) + a list of the lookups (occurrences)
//     whose gradient rows have to be summed; every member of a segment reports row -1 in rows_out,
// so the row-sparse optimizer needs no dedupe pass and nothing in the step adds into a shared row: kernel D stores
// every lookup's gradient row plainly, the optimizer's segment waves sum a row's members (one wave per row, 16 rows
// per load) and update the row (dt_adam_rows_step_seg).
//   A: writes the looked-up rows a second time, field-major (rows_fm [F][B]; a block's 16 batch rows fill whole lines).
//   B (extra blocks of k_prep, one per (field, hash partition), all partitions of a field on one XCD): an LDS hash of
//      8192 64-bit slots (row+1) << 24 | count — CAS to claim, atomicAdd to count; B <= 8192 lookups per field always
//      fit.  Slots with count >= 2 become segments in the block's private region of the segment / list arrays (a block
//      scan places them), then every member appends itself through the slot's cursor.
// History (numbers in DESIGN.md): a global hash filled with 64-bit CAS inside kernel A (~10 us of device-scope round
// trips in the gather's chain); a direct-mapped election table (2 x 213K partial-line write-backs per step, ~15 us);
// LDS election with the duplicates atomically added into an owner's row by kernel D — fine for uniform ids, but under
// Zipf ids the hot rows serialised on their owner's 16 addresses (D 20 -> 68 us).
// embedding_dropout (config.py:84; SpatialDropout1D on every [B,1,D] embedding, layers.py:878-880 = element dropout with
// 1/(1-p) scaling): keep-mask from a counter hash of (seed, batch row, packed column f*D+d), the same in kernel A
// (values) and kernel D (gradients).  The seed lives on the device and is advanced by kernel D, so a captured graph of
// the step draws a new mask at every replay.
struct EmbDrop {
    unsigned thr;            // drop iff hash < thr; 0 = no dropout
    float inv_keep;
    unsigned* seed;          // device word
    // ModelConfig.dense_dropout (reference config.py:83; Dropout on the continuous inputs, reference deepmodel.py:429-430 'dropout_dense_input'):
    // the same counter hash on the packed columns F*D + k of the concat row, its own rate; 0 = none.  Forward only: the
    // continuous inputs take no gradient.
    unsigned thr_dense;
    float inv_keep_dense;
};
__host__ __device__ inline unsigned emb_drop_hash(unsigned seed, unsigned b, unsigned col) {
    unsigned x = seed ^ (b * 0x9E3779B1u) ^ (col * 0x85EBCA77u);
    x ^= x >> 16; x *= 0x7FEB352Du; x ^= x >> 15; x *= 0x846CA68Bu; x ^= x >> 16;
    return x;
}
__device__ __forceinline__ float4 emb_drop4(float4 v, unsigned seed, unsigned thr, float inv_keep, unsigned b, unsigned col) {
    v.x = emb_drop_hash(seed, b, col) >= thr ? v.x * inv_keep : 0.f;
    v.y = emb_drop_hash(seed, b, col + 1) >= thr ? v.y * inv_keep : 0.f;
    v.z = emb_drop_hash(seed, b, col + 2) >= thr ? v.z * inv_keep : 0.f;
    v.w = emb_drop_hash(seed, b, col + 3) >= thr ? v.w * inv_keep : 0.f;
    return v;
}

constexpr int kElectSlots = 8192;     // LDS hash of one election block (64 KB); batches up to this size keep per-block segment regions
struct DedupeWs {
    int64_t* rows_fm;            // [F][B] scratch (NULL: no dedupe)
    int parts_log2;              // hash partitions per field
    // segments of the rows looked up more than once (see above), one private region per election block e (no global
    // counter: a device-scope atomicAdd in the middle of the block cost ~2 us): nseg[e] segments at seg_*[e * kSegCap ..],
    // their lookups at seg_list[e * B ..]
    int* nseg;                   // [elect blocks]
    int64_t* seg_row;            // [elect blocks][kSegCap]
    int* seg_off;                // first entry in seg_list (absolute)
    int* seg_cnt;
    int* seg_list;               // [elect blocks][B] lookups (b*F + f)
    // B > kElectSlots: regions are per FIELD (seg_* [fields padded to 8][B / 2], seg_list [fields padded to 8][B]); a block
    // reserves its share through these cursors (seg_cur doubles as the consumers' nseg array); NULL: per-block regions
    int *seg_cur, *list_cur;
    int* overflow;               // lookups that found their election table full (see elect_block); NULL: not counted
    // ... and kernel A stores one BYTE per lookup, the row's hash partition (0xff: id out of range / beyond B), field-major
    // with pid_stride (B rounded up to 8) bytes per field: what the election blocks scan instead of the 8-byte rows
    unsigned char* pid_fm;
    int pid_stride;
};
constexpr int kSegCap = kElectSlots / 2;     // a block's rows with >= 2 lookups: at most B / 2
// Chained steps (dt_*_train_step_adam's `next_*` arguments): what step n does for step n + 1 while its own launches run —
// kernel A packs the next ids' rows, the weight-gradient launch's matrix waves run the next election in their idle time, the
// finishing launch writes the tile kernel's weight layouts from the weights it has just updated.  Step n + 1 then runs with
// DT_STEP_PREPARED: no prep launch at all (four launches).  idx == NULL: not chained.
struct StepNext {
    const void* idx;             // [B][F] ids of the next step (same kind as this step's)
    int64_t* rows_out;           // the next step's rows_out
    DedupeWs dd;                 // ... and its dedupe workspace
    int eblocks;                 // its election blocks
};
__device__ __forceinline__ unsigned elect_hash(int64_t row) { return ((unsigned)row ^ (unsigned)(row >> 32)) * 0x9E3779B1u; }
// partition of a row among 2^parts_log2: the top bits of the hash (the low 13 bits pick the slot)
__device__ __forceinline__ int elect_part(unsigned h, int parts_log2) { return (int)((h >> 13) >> (19 - parts_log2)); }

// the record shards (racc: tile_common.h) as the finishing launches read them
struct RecSrc {
    const double* racc;          // [kRecShards][stride]
    int stride;
};
__device__ __forceinline__ float rec_sum(const RecSrc& r, int e) {
    double v = 0.0;
#pragma unroll
    for (int sh = 0; sh < kRecShards; ++sh) v += r.racc[(int64_t)sh * r.stride + e];
    return (float)v;
}

// ---------------------------------------------------------------------------------------------
// A: sparse forward.  One wave = one batch row, 16 waves (16 rows) per block: 8192 waves at B = 8192, all
//    resident at once (2 blocks of 1024 threads per CU) so the two dependent HBM round trips of a gather
//    (ids -> table rows) overlap across 32 waves per CU.  The block's 16 rows meet in LDS for the BN statistics.
// ---------------------------------------------------------------------------------------------
constexpr int kRowsPerBlockA = 16;

template <int KIND, int LPR, int RPB>
__global__ __launch_bounds__(64 * RPB) void k_sparse_fwd(
    const void* __restrict__ idx, const float4* __restrict__ table, const int64_t* __restrict__ row_offset,
    const int32_t* __restrict__ vocab, const float* __restrict__ dense, const float* __restrict__ wlin,
    DeepFmDims dm, float* __restrict__ X, float* __restrict__ lin_out, float* __restrict__ fm_out,
    int64_t* __restrict__ rows_out, int* __restrict__ oob, double* __restrict__ bnacc, DedupeWs dd,
    float* __restrict__ grad_rows, float* __restrict__ S_out, EmbDrop drop, unsigned long long* stamps,
    double* __restrict__ racc_zero, int racc_n, StepNext nx) {
    __shared__ __attribute__((aligned(16))) float rowbuf[RPB][kMaxC];
    DT_STAMP(stamps, 0);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = lane & (LPR - 1);
    const int NV = dm.F * LPR;  // float4 per row (<= 128)
    const int D = 4 * LPR;
    const int b = blockIdx.x * RPB + wave;
    if (b < dm.B) {
        // two dependent memory round trips for BOTH of the lane's float4 slots: (ids, vocabulary sizes, row offsets), then
        // the two table rows.  Every load is unconditional from a clamped (valid) address and zeroed afterwards: guarded
        // loads made the compiler close each slot's region with s_waitcnt vmcnt(0) — six round trips in a row (round 2's
        // ISA reading).
        int id[2], voc[2], fld[2], idn[2];
        int64_t roff[2];
        bool in[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int j = lane + 64 * t;
            in[t] = j < NV;
            fld[t] = min(j, NV - 1) / LPR;
            id[t] = load_id<KIND>(idx, (int64_t)b * dm.F + fld[t]);
            // chained steps (StepNext): the NEXT step's ids travel in the same round trip — its packed rows are written below, so
            // that its election can run inside this step's weight-gradient launch
            idn[t] = nx.idx ? load_id<KIND>(nx.idx, (int64_t)b * dm.F + fld[t]) : 0;
            voc[t] = vocab[fld[t]];
            roff[t] = row_offset[fld[t]];
        }
        float dv = lane < dm.Nd ? dense[(int64_t)b * dm.Nd + lane] : 0.f;
        if (drop.thr_dense)          // Dropout on the continuous inputs: they feed the concat row, its BN statistics and `linear`
            dv = emb_drop_hash(*drop.seed, (unsigned)b, (unsigned)(dm.F * D + lane)) >= drop.thr_dense ? dv * drop.inv_keep_dense : 0.f;
        float4 v[2];
        int64_t row[2];
        bool ok[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            ok[t] = in[t] && (unsigned)id[t] < (unsigned)voc[t];
            row[t] = ok[t] ? roff[t] + id[t] : (int64_t)-1;
            v[t] = table[(ok[t] ? row[t] : 0) * LPR + c];
        }
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            if (!ok[t]) v[t] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (c == 0 && in[t]) {
                const int64_t occ = (int64_t)b * dm.F + fld[t];
                if (dd.rows_fm) dd.rows_fm[(int64_t)fld[t] * dm.B + b] = row[t];     // for the election blocks (see DedupeWs)
                if (dd.rows_fm && dd.pid_fm)                  // B > kElectSlots: + the row's partition byte (what the blocks scan)
                    dd.pid_fm[(int64_t)fld[t] * dd.pid_stride + b] =
                        ok[t] ? (unsigned char)elect_part(elect_hash(row[t]), dd.parts_log2) : (unsigned char)0xff;
                if (rows_out) rows_out[occ] = row[t];         // (NULL: a pre-elected step, dt_deepfm_preelect wrote them)
                if (!ok[t] && oob) atomicAdd(oob, 1);
                if (nx.idx) {
                    const int64_t rn = (unsigned)idn[t] < (unsigned)voc[t] ? roff[t] + idn[t] : (int64_t)-1;
                    nx.rows_out[occ] = rn;
                    nx.dd.rows_fm[(int64_t)fld[t] * dm.B + b] = rn;
                }
            }
        }
        DT_STAMP(stamps, 1);
        if (drop.thr) {
            const unsigned seed = *drop.seed;
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const int j = lane + 64 * t;
                if (j < NV) v[t] = emb_drop4(v[t], seed, drop.thr, drop.inv_keep, (unsigned)b, (unsigned)(4 * j));
            }
        }
        float lp = (wlin && lane < dm.Nd) ? dv * wlin[dm.F + lane] : 0.f;
        float4 S = make_float4(0.f, 0.f, 0.f, 0.f), Q = S;
        float* xrow = X + (int64_t)b * dm.CP;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int j = lane + 64 * t;
            const float4 x = v[t];
            if (j < NV) {
                *reinterpret_cast<float4*>(xrow + 4 * j) = x;
                *reinterpret_cast<float4*>(&rowbuf[wave][4 * j]) = x;
                if (wlin) lp += ((x.x + x.y) + (x.z + x.w)) * wlin[j / LPR];
            }
            S.x += x.x; S.y += x.y; S.z += x.z; S.w += x.w;
            Q.x += x.x * x.x; Q.y += x.y * x.y; Q.z += x.z * x.z; Q.w += x.w * x.w;
        }
        DT_STAMP(stamps, 2);
        for (int k = lane; k < dm.CP - dm.F * D; k += 64)   // dense columns, then zero padding up to CP
            xrow[dm.F * D + k] = k < dm.Nd ? dv : 0.f;
        if (lane < dm.Nd) rowbuf[wave][dm.F * D + lane] = dv;
        S.x = wave_sum_strided<LPR>(S.x); S.y = wave_sum_strided<LPR>(S.y);
        S.z = wave_sum_strided<LPR>(S.z); S.w = wave_sum_strided<LPR>(S.w);
        Q.x = wave_sum_strided<LPR>(Q.x); Q.y = wave_sum_strided<LPR>(Q.y);
        Q.z = wave_sum_strided<LPR>(Q.z); Q.w = wave_sum_strided<LPR>(Q.w);
        if (S_out && lane < LPR) *reinterpret_cast<float4*>(S_out + (int64_t)b * D + 4 * lane) = S;   // S[b][d] = sum_f E[b,f,d]
        float ts = ((S.x * S.x - Q.x) + (S.y * S.y - Q.y)) + ((S.z * S.z - Q.z) + (S.w * S.w - Q.w));
        ts = group_sum<LPR>(ts);
        lp = wave_sum(lp);
        if (lane == 0) {
            fm_out[b] = 0.5f * ts;
            lin_out[b] = lp;
        }
        DT_STAMP(stamps, 3);
    }
    __syncthreads();
    DT_STAMP(stamps, 4);
    // ---- BN statistics: this block's rows enter the batch sums (see bnacc above); no return value: nobody waits ----
    const int nrows = min(RPB, dm.B - (int)blockIdx.x * RPB);
    double* acc = bnacc + (int64_t)((int)blockIdx.x & (kBnShards - 1)) * 2 * dm.CP;
    for (int col = threadIdx.x; col < dm.C; col += blockDim.x) {
        double sum = 0.0, sq = 0.0;
        for (int w = 0; w < nrows; ++w) {
            const double x = (double)rowbuf[w][col];
            sum += x;
            sq += x * x;
        }
        unsafeAtomicAdd(acc + col, sum);
        unsafeAtomicAdd(acc + dm.CP + col, sq);
    }
    // the record accumulators of this step's tile kernel start from zero
    for (int i = (int)blockIdx.x * (int)blockDim.x + (int)threadIdx.x; i < racc_n; i += (int)(gridDim.x * blockDim.x))
        racc_zero[i] = 0.0;
    if (blockIdx.x == 0 && dd.seg_cur && (int)threadIdx.x < ((dm.F + 7) & ~7)) {     // the election's region cursors (B > kElectSlots)
        dd.seg_cur[threadIdx.x] = 0;
        dd.list_cur[threadIdx.x] = 0;
    }
    DT_STAMP(stamps, 5);
}

// ---------------------------------------------------------------------------------------------
// B: the in-step dedupe's election + the MFMA operand layouts of W1 / W2 / W2^T (see the round-2 tower notes below).
//    (Rounds 1-4 also ran level 1 of the BatchNormalization reduction here; the batch sums are kernel A's atomics now.)
// ---------------------------------------------------------------------------------------------
struct PrepOut {
    float *W1L, *W2L, *W2TL;                      // MFMA operand layouts of W1 / W2 / W2^T (k_mlp_fwd3)
    const float* W2;
    // split-bf16 tower (tower_x3.h; NULL: not that mode): the bf16 halves of W1 / W2 in the layouts of X3Weights
    __bf16 *x3_W1B, *x3_W1R, *x3_W2B, *x3_W2R;
    int64_t x3_w1b_lo, x3_w1r_lo, x3_w2b_lo, x3_w2r_lo;
    // ... and, for DCN, the layer vectors padded to CP: [2 L + 1][CP] = cross kernels | cross biases | w3c (NULL: DeepFM)
    float* x3_cwp;
    const float *cw, *cb, *w3c;
    int L;
};

// One election block of the in-step dedupe (see DedupeWs): block e = (field, hash partition) of a grid whose ids keep
// e % 8 = the XCD.  Reads the field's row list rows_fm [F][B], turns the rows looked up several times into segments and
// marks their members -1 in rows_out.  `eslots`: kElectSlots 64-bit LDS slots + bitmap + scan scratch.
//   NT    threads that run it: 1024 = a whole block of the prep launch (hardware barriers), 256 = the four matrix waves of a
//         weight-gradient block running the NEXT step's election in their idle time (k_wgrad_rows; they meet at an LDS counter:
//         the block's memory waves must not be held at a hardware barrier)
//   BIG   false: B <= kElectSlots, round 4's layout — private segment / list regions per block (no global counter: a
//         returning device-scope atomic in the middle of the chain costs ~2 us), the field's lookups in chunks of NT x kElU
//         (one chunk with 1024 threads: a lookup's slot stays in a register for pass 3).
//         true: any batch size.  ~4096 lookups per block (half of the table); the block does not read the field's B rows
//         (8 B each, eblocks x B x 8 bytes of L2 traffic: 184 us at B = 65536) but the partition BYTE kernel A stored per
//         lookup (pid_fm), and fetches a row only where the byte matches; its segments / list entries go to its FIELD's region
//         through two returning atomics (dd.seg_cur / dd.list_cur, zeroed by the launch that wrote rows_fm) — per-block
//         regions would take eblocks x B entries.
// Termination: a block holds at most kElectSlots distinct rows.  B <= kElectSlots guarantees it; beyond that a partition
// would have to be 2x over-full of DISTINCT rows (expected 4096, sigma 64) — a lookup that finds the table full is counted
// in dd.overflow (the host checks it: fused.FusedDeepFM.check_dedupe) and keeps its own row (-> updated as if looked up once).
constexpr int kElU = 8;               // lookups per thread and chunk, all loads in flight
constexpr int kElectList = 16384;     // elect_block_big's LDS list of a block's lookups (64 KB next to the 66 KB table: one block per CU).
                                      // Twice the table: a hot row's lookups share ONE slot — with Zipf(1.05) ids at B = 65536 the top
                                      // row's 5 K lookups + the partition's other 4 K overflowed an 8192-entry list into the slow paths
                                      // (the prep launch 130 us instead of 75)
struct ElectSync {
    unsigned* cnt;                    // LDS word of the soft barrier (NT = 256), zeroed by the caller
    unsigned target;
};
template <int NT, bool SOFT>
__device__ __forceinline__ void elect_barrier(ElectSync& sy) {
    if constexpr (SOFT) {
        // LDS operations of a wave complete in order: the arrival (ds_add) follows everything the wave wrote before it
        sy.target += NT / 64;
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if ((threadIdx.x & 63) == 0) atomicAdd(sy.cnt, 1u);
        while (*reinterpret_cast<volatile unsigned*>(sy.cnt) < sy.target) __builtin_amdgcn_s_sleep(1);
        asm volatile("" ::: "memory");
    } else {
        __syncthreads();
    }
}

// pass 1 for ONE lookup of this block's partition: claim (CAS) / count (atomicAdd); the SECOND lookup of a row flags its
// slot in the bitmap.  -> the slot, or -1 (BOUNDED only) when the table is full
template <bool BOUNDED>
__device__ __forceinline__ int elect_insert(unsigned long long* eslots, unsigned* multi, int64_t row, unsigned h) {
    const unsigned long long key = (unsigned long long)(row + 1) << 24;
    unsigned slot = h & (kElectSlots - 1);
    for (int probes = 0;; ++probes) {                          // B <= kElectSlots distinct rows always terminate
        if (BOUNDED && probes >= kElectSlots) return -1;
        const unsigned long long prev = atomicCAS(&eslots[slot], 0ULL, key | 1ULL);
        if (prev == 0ULL) break;
        if ((prev >> 24) == (unsigned long long)(row + 1)) {
            const unsigned long long old = atomicAdd(&eslots[slot], 1ULL);
            if ((old & 0xffffffULL) == 1ULL) atomicOr(&multi[slot >> 5], 1u << (slot & 31));
            break;
        }
        slot = (slot + 1) & (kElectSlots - 1);
    }
    return (int)slot;
}
// pass 3's lookup of a row's slot (the first probe hits unless the row was displaced in pass 1); -1: never placed
__device__ __forceinline__ int elect_find(const unsigned long long* eslots, int64_t row, unsigned h) {
    const unsigned long long key = (unsigned long long)(row + 1);
    unsigned sl = h & (kElectSlots - 1);
    unsigned long long v = eslots[sl];
    for (int probes = 0; (v >> 24) != key && v != 0ULL && probes < kElectSlots; ++probes) {
        sl = (sl + 1) & (kElectSlots - 1);
        v = eslots[sl];
    }
    return (v >> 24) == key ? (int)sl : -1;
}

// pass 2: the flagged slots become segments.  Thread t < 256 owns bitmap word t (slots [32t, 32t + 32)); one exclusive scan
// over those 256 threads of (segments, list entries) — packed in 32 bits for B <= 8192, 64 bits beyond (a large batch's
// hot rows take more than 64 K entries): shuffles inside a wave, the wave totals through LDS.  (Walking all 8192 slots
// instead cost 2.6 us per block; with uniform ids ~2 are flagged.)  -> base1, the block's first list entry (absolute);
// leaves every flagged slot as key | flag | cursor.  Ends with a barrier.
template <int NT, bool SOFT, bool BIG>
__device__ __forceinline__ int elect_segments(unsigned long long* eslots, unsigned* multi, int* scan, const DedupeWs& dd, int B,
                                              int f, int e, int tid, ElectSync& sy) {
    typedef typename std::conditional<BIG, unsigned long long, unsigned>::type acc_t;
    constexpr int kSh = BIG ? 32 : 16;
    const int lane = tid & 63, wv = tid >> 6;
    static_assert(kElectSlots / 32 == 256 && NT >= 256, "one bitmap word per thread of the first four waves");
    unsigned word = tid < kElectSlots / 32 ? multi[tid] : 0u;
    acc_t own = 0;
    for (unsigned w = word; w; w &= w - 1) {
        const int slot = 32 * tid + (__ffs((int)w) - 1);
        own += ((acc_t)1 << kSh) + (acc_t)(eslots[slot] & 0xffffffULL);
    }
    acc_t incl = own;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const acc_t t = __shfl_up(incl, o, 64);
        if (lane >= o) incl += t;
    }
    acc_t* scanw = reinterpret_cast<acc_t*>(scan);            // [4] wave totals (ints 0..7); ints 8, 9: region bases
    if (lane == 63 && wv < 4) scanw[wv] = incl;
    elect_barrier<NT, SOFT>(sy);
    acc_t before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const acc_t t = scanw[w];
        if (w < wv) before += t;
        total += t;
    }
    const int nsegs = (int)(total >> kSh), nlist = (int)(total & (((acc_t)1 << kSh) - 1));
    int base0, base1;                                         // first segment / first list entry of this block (absolute)
    if constexpr (BIG) {                                      // the field's region, placed by two returning atomics
        if (tid == 0) {
            const int cap = B >> 1;                           // a field's rows with >= 2 lookups: at most B / 2
            const int s0 = nsegs ? atomicAdd(&dd.seg_cur[f], nsegs) : 0;
            const int l0 = nlist ? atomicAdd(&dd.list_cur[f], nlist) : 0;
            scan[8] = f * cap + s0;
            scan[9] = f * B + l0;
        }
        elect_barrier<NT, SOFT>(sy);
        base0 = scan[8]; base1 = scan[9];
    } else {
        if (tid == 0) dd.nseg[e] = nsegs;
        base0 = e * kSegCap; base1 = e * B;
    }
    const acc_t excl = before + incl - own;
    int sidx = base0 + (int)(excl >> kSh), lrel = (int)(excl & (((acc_t)1 << kSh) - 1));
    for (unsigned w = word; w; w &= w - 1) {
        const int slot = 32 * tid + (__ffs((int)w) - 1);
        const unsigned long long v = eslots[slot];
        const int c = (int)(v & 0xffffffULL);
        dd.seg_row[sidx] = (int64_t)(v >> 24) - 1;
        dd.seg_off[sidx] = base1 + lrel;
        dd.seg_cnt[sidx] = c;
        eslots[slot] = (v & ~0xffffffULL) | 0x800000ULL | (unsigned long long)lrel;    // flag + cursor
        ++sidx; lrel += c;
    }
    elect_barrier<NT, SOFT>(sy);
    return base1;
}
// pass 3 for one lookup: a member of a segment appends itself and leaves rows_out
__device__ __forceinline__ void elect_append(unsigned long long* eslots, int slot, const DedupeWs& dd, int base1, int b, int F,
                                             int f, int64_t* __restrict__ rows_out) {
    if (!(eslots[slot] & 0x800000ULL)) return;                // looked up once
    const int64_t occ = (int64_t)b * F + f;
    const unsigned long long old = atomicAdd(&eslots[slot], 1ULL);
    dd.seg_list[base1 + (int)(old & 0x7fffffULL)] = (int)occ;
    rows_out[occ] = -1;
}

// B <= kElectSlots.  U = lookups per thread and chunk: NT x U >= 8192 keeps the whole field in one chunk (one round trip, slots in
// registers) — 8 for a 1024-thread block, 32 for the 256 hosted threads
template <int NT, bool SOFT, int U = kElU>
__device__ __forceinline__ void elect_block(unsigned long long* eslots, const DedupeWs& dd, int B, int F, int e, int tid,
                                            int64_t* __restrict__ rows_out, ElectSync& sy) {
    unsigned* multi = reinterpret_cast<unsigned*>(eslots + kElectSlots);      // [kElectSlots / 32]
    int* scan = reinterpret_cast<int*>(multi + kElectSlots / 32);             // [16]: wave totals | region bases
    // XCD-aware ids (workgroups go round-robin over the 8 XCDs): every partition block of a field runs on XCD f % 8,
    // so the field's row list is fetched into ONE L2 instead of eight
    const int j = e >> 3, part = j & ((1 << dd.parts_log2) - 1);
    const int f = 8 * (j >> dd.parts_log2) + (e & 7);
    if (f >= F) {
        if (tid == 0) dd.nseg[e] = 0;
        return;
    }
    const int64_t* rf = dd.rows_fm + (int64_t)f * B;
    constexpr int kChunk = NT * U;
    const int nchunks = (B + kChunk - 1) / kChunk;
    int64_t rowv[U];
    int myslot[U];
    auto load_chunk = [&](int ch) {                           // all of the thread's row loads of the chunk in flight
#pragma unroll
        for (int u = 0; u < U; ++u) rowv[u] = rf[min(ch * kChunk + tid + NT * u, B - 1)];
    };
    auto mine = [&](int ch, int u, unsigned& h) {             // is lookup u of the chunk one of this block's?
        const int64_t row = rowv[u];
        if (ch * kChunk + tid + NT * u >= B || row < 0) return false;
        h = elect_hash(row);
        return elect_part(h, dd.parts_log2) == part;
    };
    load_chunk(0);
    for (int i = tid; i < kElectSlots; i += NT) eslots[i] = 0ULL;
    for (int i = tid; i < kElectSlots / 32; i += NT) multi[i] = 0u;
    elect_barrier<NT, SOFT>(sy);
    for (int ch = 0; ch < nchunks; ++ch) {
        if (ch) load_chunk(ch);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            unsigned h;
            myslot[u] = mine(ch, u, h) ? elect_insert<false>(eslots, multi, rowv[u], h) : -1;
        }
    }
    elect_barrier<NT, SOFT>(sy);
    const int base1 = elect_segments<NT, SOFT, false>(eslots, multi, scan, dd, B, f, e, tid, sy);
    // pass 3 (one chunk: a lookup's slot is still in its register; several: it finds the slot again by probing)
    for (int ch = 0; ch < nchunks; ++ch) {
        if (nchunks > 1) load_chunk(ch);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            int slot = myslot[u];
            if (nchunks > 1) {
                unsigned h;
                slot = mine(ch, u, h) ? elect_find(eslots, rowv[u], h) : -1;
            }
            if (slot >= 0) elect_append(eslots, slot, dd, base1, ch * kChunk + tid + NT * u, F, f, rows_out);
        }
    }
}

// Any batch size (the prep launch takes this one beyond kElectSlots rows).  A block reading its field's B rows (8 B each) made
// the launch 184 us at B = 65536 — eblocks x B x 8 bytes of L2 traffic in chunks of dependent round trips.  Here:
//   * ~4096 lookups per block (half of the table's slots: a quarter of the blocks), and kernel A stores one BYTE per lookup —
//     its row's partition (pid_fm) — which is all a block scans: B bytes, every load of the thread in flight at once;
//   * the lookups whose byte matches are compacted into an LDS list (mlist, 32 KB: a launch with such blocks runs one per CU)
//     and only THEIR rows are fetched — one round trip in pass 1, one (L2-warm) in pass 3;
//   * segments / list entries go to the FIELD's region through two returning atomics (dd.seg_cur / dd.list_cur, zeroed by the
//     launch that wrote rows_fm): per-block regions would take eblocks x B entries.
// Termination / capacity: the table holds kElectSlots DISTINCT rows (a partition's expected 4096 lookups, sigma 64, would have
// to be 2x over-full of distinct rows: what does not fit is counted in dd.overflow — the host checks it,
// fused.FusedDeepFM.check_dedupe — and keeps its own row).  The list holds kElectList lookups; a hot row's thousands of
// lookups beyond that take the slow paths noted below, nothing is lost.
template <int NT, bool SOFT>
__device__ __forceinline__ void elect_block_big(unsigned long long* eslots, const DedupeWs& dd, int B, int F, int e, int tid,
                                                int64_t* __restrict__ rows_out, ElectSync& sy) {
    unsigned* multi = reinterpret_cast<unsigned*>(eslots + kElectSlots);      // [kElectSlots / 32]
    int* scan = reinterpret_cast<int*>(multi + kElectSlots / 32);             // [16]: wave totals | region bases | [12] list length
    int* mlist = scan + 16;                                                   // [kElectList] batch rows of this block's lookups
    unsigned* mcount = reinterpret_cast<unsigned*>(scan + 12);
    const int j = e >> 3, part = j & ((1 << dd.parts_log2) - 1);
    const int f = 8 * (j >> dd.parts_log2) + (e & 7);
    if (f >= F) return;
    const int64_t* rf = dd.rows_fm + (int64_t)f * B;
    const unsigned char* pf = dd.pid_fm + (int64_t)f * dd.pid_stride;
    for (int i = tid; i < kElectSlots; i += NT) eslots[i] = 0ULL;
    for (int i = tid; i < kElectSlots / 32; i += NT) multi[i] = 0u;
    if (tid == 0) *mcount = 0u;
    elect_barrier<NT, SOFT>(sy);
    // scan: 16 partition bytes per load, four loads in flight per thread.  A block's lookups beyond the list's capacity (a hot
    // row: with Zipf ids one row takes 8 % of a field's lookups — 5 K of 65,536, all in ONE partition) are inserted right here,
    // one dependent row load each; pass 3 then walks the partition bytes again instead of the list (`spilled`)
    int lost = 0;
    for (int b0 = tid * 16; b0 < B; b0 += NT * 64) {
        uint4 pv[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int bb = b0 + q * NT * 16;
            pv[q] = bb < B ? *reinterpret_cast<const uint4*>(pf + bb) : make_uint4(~0u, ~0u, ~0u, ~0u);   // (pid_stride: B rounded up to 16)
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const unsigned w[4] = {pv[q].x, pv[q].y, pv[q].z, pv[q].w};
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const int b = b0 + q * NT * 16 + k;
                // (one returning LDS atomic per match.  Taking a wave's slots with one atomic — 16 ballots + prefix counts per load
                // — was measured slower: the prep launch 49.8 vs 43.4 us at B = 32768, 87.6 vs 74.5 us at 65536, tools/r5/call16.sh)
                if ((int)((w[k >> 2] >> (8 * (k & 3))) & 0xffu) == part && b < B) {
                    const unsigned pos = atomicAdd(mcount, 1u);
                    if (pos < (unsigned)kElectList) {
                        mlist[pos] = b;
                    } else {
                        const int64_t row = rf[b];
                        if (elect_insert<true>(eslots, multi, row, elect_hash(row)) < 0) ++lost;
                    }
                }
            }
        }
    }
    elect_barrier<NT, SOFT>(sy);
    const unsigned found = *mcount;
    const int n = (int)min(found, (unsigned)kElectList);
    const bool spilled = found > (unsigned)kElectList;
    // pass 1 over the compact list: kElU rows per thread in flight
    for (int i0 = tid; i0 < n; i0 += NT * kElU) {
        int bq[kElU];
        int64_t rowv[kElU];
#pragma unroll
        for (int u = 0; u < kElU; ++u) {
            const int i = i0 + NT * u;
            bq[u] = i < n ? mlist[i] : -1;
            rowv[u] = rf[bq[u] >= 0 ? bq[u] : 0];
        }
#pragma unroll
        for (int u = 0; u < kElU; ++u)
            if (bq[u] >= 0 && elect_insert<true>(eslots, multi, rowv[u], elect_hash(rowv[u])) < 0) ++lost;
    }
    if (lost && dd.overflow) atomicAdd(dd.overflow, lost);
    elect_barrier<NT, SOFT>(sy);
    const int base1 = elect_segments<NT, SOFT, true>(eslots, multi, scan, dd, B, f, e, tid, sy);
    if (!spilled) {
        for (int i0 = tid; i0 < n; i0 += NT * kElU) {
            int bq[kElU];
            int64_t rowv[kElU];
#pragma unroll
            for (int u = 0; u < kElU; ++u) {
                const int i = i0 + NT * u;
                bq[u] = i < n ? mlist[i] : -1;
                rowv[u] = rf[bq[u] >= 0 ? bq[u] : 0];
            }
#pragma unroll
            for (int u = 0; u < kElU; ++u) {
                if (bq[u] < 0) continue;
                const int slot = elect_find(eslots, rowv[u], elect_hash(rowv[u]));
                if (slot >= 0) elect_append(eslots, slot, dd, base1, bq[u], F, f, rows_out);
            }
        }
    } else {
        // the list did not hold every lookup of the partition: pass 3 from the partition bytes (a row load per match)
        for (int b0 = tid * 16; b0 < B; b0 += NT * 16) {
            const uint4 pv = *reinterpret_cast<const uint4*>(pf + b0);
            const unsigned w[4] = {pv.x, pv.y, pv.z, pv.w};
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const int b = b0 + k;
                if ((int)((w[k >> 2] >> (8 * (k & 3))) & 0xffu) == part && b < B) {
                    const int64_t row = rf[b];
                    const int slot = elect_find(eslots, row, elect_hash(row));
                    if (slot >= 0) elect_append(eslots, slot, dd, base1, b, F, f, rows_out);
                }
            }
        }
    }
}
constexpr size_t kElectLds = (size_t)kElectSlots * 8 + kElectSlots / 32 * sizeof(unsigned) + 16 * sizeof(int);
constexpr size_t kElectLdsBig = kElectLds + (size_t)kElectList * sizeof(int);

// the election alone (dt_deepfm_preelect: the ids-only half of a step, run ahead of it)
__global__ __launch_bounds__(1024) void k_elect(DedupeWs dd, DeepFmDims dm, int64_t* __restrict__ rows_out) {
    extern __shared__ unsigned long long eslots_dyn[];
    ElectSync sy{nullptr, 0u};
    if (dd.seg_cur)
        elect_block_big<1024, false>(eslots_dyn, dd, dm.B, dm.F, (int)blockIdx.x, (int)threadIdx.x, rows_out, sy);
    else
        elect_block<1024, false>(eslots_dyn, dd, dm.B, dm.F, (int)blockIdx.x, (int)threadIdx.x, rows_out, sy);
}

// ids -> packed table rows (-1 = id out of range), row-major rows_out [B][F] (what the row-gradient epilogue reads) and
// field-major rows_fm [F][B] (what the election reads): a block takes 64 batch rows, both sides in contiguous segments
template <int KIND>
__global__ __launch_bounds__(256) void k_rows_of_ids(const void* __restrict__ idx, const int64_t* __restrict__ row_offset,
                                                     const int32_t* __restrict__ vocab, DeepFmDims dm,
                                                     int64_t* __restrict__ rows_out, int64_t* __restrict__ rows_fm,
                                                     int* __restrict__ seg_cur, int* __restrict__ list_cur,
                                                     unsigned char* __restrict__ pid_fm, int pid_stride, int parts_log2) {
    __shared__ int64_t tile[64][129];             // F <= 128
    if (blockIdx.x == 0 && seg_cur && (int)threadIdx.x < ((dm.F + 7) & ~7)) { seg_cur[threadIdx.x] = 0; list_cur[threadIdx.x] = 0; }
    const int b0 = blockIdx.x * 64;
    const int nb = min(64, dm.B - b0);
    for (int e = threadIdx.x; e < nb * dm.F; e += blockDim.x) {
        const int r = e / dm.F, f = e - r * dm.F;
        const int id = load_id<KIND>(idx, (int64_t)(b0 + r) * dm.F + f);
        const int64_t row = (unsigned)id < (unsigned)vocab[f] ? row_offset[f] + id : (int64_t)-1;
        rows_out[(int64_t)(b0 + r) * dm.F + f] = row;
        tile[r][f] = row;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < dm.F * 64; e += blockDim.x) {
        const int f = e >> 6, r = e & 63;
        if (r < nb) {
            rows_fm[(int64_t)f * dm.B + b0 + r] = tile[r][f];
            if (pid_fm)
                pid_fm[(int64_t)f * pid_stride + b0 + r] =
                    tile[r][f] >= 0 ? (unsigned char)elect_part(elect_hash(tile[r][f]), parts_log2) : (unsigned char)0xff;
        }
    }
}

__global__ __launch_bounds__(1024) void k_prep(DeepFmDims dm, const float* __restrict__ W1, PrepOut o, int layout_blocks,
                                               DedupeWs dd, int64_t* __restrict__ rows_out) {
    // block order: election | weight layouts — the election (loads, LDS hash, scan, three barriers) is the longest chain of
    // the launch and starts first; its block ids keep id % 8 = the XCD (elect_blocks is a multiple of 8)
    constexpr int bn_blocks = 0;
    const int elect_blocks = (int)gridDim.x - layout_blocks;
    const int bid = (int)blockIdx.x - elect_blocks;          // < 0: election block
    if (bid < 0) {   // the dedupe's election (see DedupeWs): block = (field, hash partition)
        extern __shared__ unsigned long long eslots_dyn[];
        ElectSync sy{nullptr, 0u};
        if (dd.seg_cur)
            elect_block_big<1024, false>(eslots_dyn, dd, dm.B, dm.F, (int)blockIdx.x, (int)threadIdx.x, rows_out, sy);
        else
            elect_block<1024, false>(eslots_dyn, dd, dm.B, dm.F, (int)blockIdx.x, (int)threadIdx.x, rows_out, sy);
        return;
    }
    if (bid >= bn_blocks && o.x3_W1B) {  // weight layouts of the split-bf16 tower (tower_x3.h): hi | lo halves, 16 bytes per store
        const int wb = bid - bn_blocks, nwb = layout_blocks;
        typedef __bf16 b8 __attribute__((ext_vector_type(8)));
        // v = p0 + p1 (+ p2): bf16 parts, each the rounding of what the parts before it left (three parts: exact)
        auto split8 = [](const float (&v)[8], __bf16* dst, int64_t stride, int parts) {
            b8 q[3];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                float r = v[j];
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const __bf16 a = (__bf16)r;
                    q[k][j] = a;
                    r -= (float)a;
                }
            }
            for (int k = 0; k < parts; ++k) *reinterpret_cast<b8*>(dst + k * stride) = q[k];
        };
        const int nst = dm.CP >> 5;
        // One item of each of the four layouts per thread and pass, every load of the pass requested before the first store:
        // ONE memory round trip per pass (four loops after each other cost four, and made this the launch's longest chain)
        const int n1b = nst * 512, n1r = dm.CP * 16, n2b = 4 * 4 * 64, n2r = kH1 * kH2 / 8;
        const int nmax = n1b > n1r ? n1b : n1r;
        for (int e = wb * blockDim.x + threadIdx.x; e < nmax; e += nwb * blockDim.x) {
            float v1[8], v2[8], v3[8], v4[8];
            const bool a1 = e < n1b, a2 = e < n1r, a3 = e < n2b, a4 = e < n2r;
            if (a1) {        // W1B (3 parts): lane (n, g) of wave w at step s holds W1[32 s + 8 g + j][16 w + n]
                const int l = e & 63, w = (e >> 6) & 7, st = e >> 9;
                const int k0 = 32 * st + 8 * (l >> 4), n = 16 * w + (l & 15);
#pragma unroll
                for (int j = 0; j < 8; ++j) v1[j] = k0 + j < dm.C ? W1[(int64_t)(k0 + j) * kH1 + n] : 0.f;
            }
            if (a2) {        // W1R (2 parts): row-major copy [CP][128], rows >= C zero
                const int r = e >> 4, k8 = e & 15;
#pragma unroll
                for (int j = 0; j < 8; ++j) v2[j] = r < dm.C ? W1[(int64_t)r * kH1 + 8 * k8 + j] : 0.f;
            }
            if (a3) {        // W2B (3 parts): lane (n, g) of column tile t at step s holds W2[32 s + 8 g + j][16 t + n]
                const int l = e & 63, t = (e >> 6) & 3, st = e >> 8;
                const int k0 = 32 * st + 8 * (l >> 4), n = 16 * t + (l & 15);
#pragma unroll
                for (int j = 0; j < 8; ++j) v3[j] = o.W2[(k0 + j) * kH2 + n];
            }
            if (a4) {        // W2R (2 parts): row-major copy [128][64]
#pragma unroll
                for (int j = 0; j < 8; ++j) v4[j] = o.W2[(int64_t)e * 8 + j];
            }
            if (a1) split8(v1, o.x3_W1B + (int64_t)e * 8, o.x3_w1b_lo, 3);
            if (a2) split8(v2, o.x3_W1R + (int64_t)e * 8, o.x3_w1r_lo, 2);
            if (a3) split8(v3, o.x3_W2B + (int64_t)e * 8, o.x3_w2b_lo, 3);
            if (a4) split8(v4, o.x3_W2R + (int64_t)e * 8, o.x3_w2r_lo, 2);
        }
        if (o.x3_cwp) {
            const int nv = (2 * o.L + 1) * dm.CP;
            for (int e = wb * blockDim.x + threadIdx.x; e < nv; e += nwb * blockDim.x) {
                const int v = e / dm.CP, col = e - v * dm.CP;
                const float* src = v < o.L ? o.cw + (int64_t)v * dm.C : v < 2 * o.L ? o.cb + (int64_t)(v - o.L) * dm.C : o.w3c;
                o.x3_cwp[e] = col < dm.C ? src[col] : 0.f;
            }
        }
        return;
    }
    if (bid >= bn_blocks) {  // weight layouts
        const int wb = bid - bn_blocks, nwb = layout_blocks;
        // W1L: float4 j of lane (c = l%32, s = l/32) of wave w in k-group g = W1[8g + 4s + j][32w + c]  (k_mlp_fwd3 GEMM1)
        floatx4_t* w1l = reinterpret_cast<floatx4_t*>(o.W1L);
        const int n4 = dm.CP * kH1 / 4;
        for (int e = wb * blockDim.x + threadIdx.x; e < n4; e += nwb * blockDim.x) {
            const int c = e & 31, s = (e >> 5) & 1, w = (e >> 6) & 3, g = e >> 8;
            const int k0 = 8 * g + 4 * s, n = 32 * w + c;
            floatx4_t v;
            v.x = k0 + 0 < dm.C ? W1[(int64_t)(k0 + 0) * kH1 + n] : 0.f;
            v.y = k0 + 1 < dm.C ? W1[(int64_t)(k0 + 1) * kH1 + n] : 0.f;
            v.z = k0 + 2 < dm.C ? W1[(int64_t)(k0 + 2) * kH1 + n] : 0.f;
            v.w = k0 + 3 < dm.C ? W1[(int64_t)(k0 + 3) * kH1 + n] : 0.f;
            w1l[e] = v;
        }
        // W2L: float4 j of lane (n = l%16, q = l/16) of wave w in k-group G = W2[16G + 4q + j][16w + n]  (GEMM2, 16x16x4)
        floatx4_t* w2l = reinterpret_cast<floatx4_t*>(o.W2L);
        for (int e = wb * blockDim.x + threadIdx.x; e < kH1 * kH2 / 4; e += nwb * blockDim.x) {
            const int l = e & 63, w = (e >> 6) & 3, G = e >> 8;
            const int k0 = 16 * G + 4 * (l >> 4), n = 16 * w + (l & 15);
            floatx4_t v;
            v.x = o.W2[(k0 + 0) * kH2 + n]; v.y = o.W2[(k0 + 1) * kH2 + n];
            v.z = o.W2[(k0 + 2) * kH2 + n]; v.w = o.W2[(k0 + 3) * kH2 + n];
            w2l[e] = v;
        }
        // W2TL: float4 j of lane (c = l%32, s = l/32) of wave w in k-group g = W2[32w + c][8g + 4s + j]  (dH1 = dH2 . W2^T)
        floatx4_t* w2tl = reinterpret_cast<floatx4_t*>(o.W2TL);
        for (int e = wb * blockDim.x + threadIdx.x; e < kH1 * kH2 / 4; e += nwb * blockDim.x) {
            const int l = e & 63, w = (e >> 6) & 3, g = e >> 8;
            w2tl[e] = *reinterpret_cast<const floatx4_t*>(o.W2 + (32 * w + (l & 31)) * kH2 + 8 * g + 4 * (l >> 5));
        }
        return;
    }
}


// =============================================================================================
// Round-2 dense tower.  What round 1's kernels taught (phase stamps, tools/phase_times.py):
//   * a wave issues in order and an MFMA holds its issue slot until the matrix pipe accepts it, so with ONE wave
//     per SIMD every LDS read or global load placed "just before use" idles the pipe for its whole latency: all
//     operand reads here are placed half a chunk (16 MFMAs) or more ahead of their use;
//   * a burst of global loads blocks the issuing wave until the CU's memory pipeline has taken them (~20 cycles
//     per wave-instruction, shared by the 4 SIMDs; ~100+ when every CU bursts at once): loads are issued one or
//     two at a time BETWEEN groups of MFMAs, two chunks ahead, never as a prologue burst;
//   * the memory pipeline's cost is per wave-instruction, not per byte: every operand is a 16-byte (or 8-byte)
//     vector.  An MFMA contraction index may be permuted freely as long as A and B agree, so a lane takes FOUR
//     consecutive k (one float4) and spends them on four consecutive MFMA steps:
//       32x32x2: lane (c = l%32, s = l/32), step 4g+j  <->  k = 8g + 4s + j
//       16x16x4: lane (n = l%16, q = l/16), step 4G+j  <->  k = 16G + 4q + j
//     weights come from L2 in lane-major re-layouts written once per step by k_prep (W1L, W2L, W2TL) or, for
//     dXn = dH1 . W1^T, straight from the ROW-major W1 whose rows are the k-contiguous vectors needed.
// (The launch list of round 2 that stood here — C k_mlp_fwd3, E k_wgrad3, E' k_bn_grads, D k_dx_sparse_bwd — is history:
// the file's header has today's.  k_mlp_fwd3 below is the exact-fp32 tile kernel of `dnn_params['mfma_dtype'] = 'f32'` and of
// forward-only calls; the default tile kernel is tower_x3.h.)
// =============================================================================================
typedef float floatx2 __attribute__((ext_vector_type(2)));
constexpr int kPad = 4;      // LDS row pad in floats: stride == 4 (mod 64) -> the 16-byte operand reads of 16 rows hit 64 distinct banks
constexpr int kH2S = kH2 + kPad;

// mean / biased variance of column `col` of the batch from kernel A's sums (double; see bnacc)
__device__ __forceinline__ void bn_stats_col(const double* __restrict__ bnacc, int CP, int B, int col, float& mean, float& var) {
    double sx = 0.0, sq = 0.0;
#pragma unroll
    for (int sh = 0; sh < kBnShards; ++sh) {
        sx += bnacc[(int64_t)sh * 2 * CP + col];
        sq += bnacc[(int64_t)sh * 2 * CP + CP + col];
    }
    const double invB = 1.0 / (double)B;          // (uniform: one division per wave on the scalar-ish path, not per column)
    const double m = sx * invB;
    const double v = sq * invB - m * m;
    mean = (float)m;
    var = v > 0.0 ? (float)v : 0.f;
}

constexpr int kCrossScal = 48 * 16;                                  // floats of the P / Gram block (k_mlp_fwd3 crP)
constexpr int kCrossLds = kTM + kCrossScal + 2 * kTM * 16;          // DCN's LDS next to the layer vectors: zcs | crP | crA | crF

// C: MLP forward + top of the backward on a 32-row tile; NCH = CP / 64 column chunks.
// LC = 0: DeepFM (z = linear + fm + dnn).  LC = kCrossMax: DCN (z = w3c . cross(Xn) + dnn): the Cross network's forward and
// backward run on the Xn tile in LDS, one wave per row (lanes along the columns), between the tower's phases.
// G3 (the pipelined step, dt_deepfm_train_step with DT_STEP_PIPELINED): the tile's dXn = dH1 . W1^T runs HERE as well, on
// the dH1 tile the kernel still holds (16x16x4 MFMA, W1 rows straight from L2 as in kernel D), and leaves as whole rows
// (dxn_out [rows][CP]) together with the tile's two BN-backward partial sums sum_r dXn and sum_r dXn xhat (Part3 sdx /
// sdxx).  The batch sums dgamma / dbeta then come from ONE small reduction of the tile records instead of from the
// weight-gradient GEMM (M = Xhat^T dH1 -> rowdot(W1, M)): kernel E leaves the step's dependent chain and the row-gradient
// kernel becomes a streaming epilogue (k_wgrad_rows below).
template <int NCH, int LC, bool G3 = false>
__global__ __launch_bounds__(256) void k_mlp_fwd3(const float* __restrict__ X, MlpParams p, DeepFmDims dm,
                                                  const float* __restrict__ lin, const float* __restrict__ fm,
                                                  const float* __restrict__ y, float* __restrict__ H1,
                                                  float* __restrict__ dH1, float* __restrict__ dH2,
                                                  float* __restrict__ z_out, float* __restrict__ logit_out,
                                                  float* __restrict__ dlogit, float* __restrict__ dz_out,
                                                  double* __restrict__ part, unsigned long long* stamps, DcnArgs dc,
                                                  float* __restrict__ dxn_out) {
    // G3 with LC > 0 (DCN): the cross network's share of dXn, sum_l coeff[r][l] Wc_l, enters the same GEMM as 16 more K steps
    // (A = the coefficient tile crF, B = the layer vectors in LDS) — round 2 formed it on the VALU (12 K cycles) and sent it
    // through HBM (dXc, 14.7 MB written and re-read)
    extern __shared__ __attribute__((aligned(16))) float lds[];
    DT_STAMP(stamps, 0);
    constexpr int CP = 64 * NCH, XS = CP + kPad, HS = kH1 + kPad;
    float* xs = lds;                   // [32][XS] Xn tile; reused for the 4 waves' d w_lin partials at the end
    float* bnp = xs + kTM * XS;        // [4][CP]  mean | gamma*rstd | beta | rstd
    float* h1s = bnp + 4 * CP;         // [32][HS] H1, later dH1
    float* dh2s = h1s + kTM * HS;      // [32][kH2S] dH2
    float* zp = dh2s + kTM * kH2S;     // [4][32]  per-wave partial dnn logits
    float* dzs = zp + 4 * kTM;         // [32]
    float* zcs = dzs + kTM;            // DCN: [32] w3c . cross(Xn) per row
    float* crP = zcs + kTM;            // DCN: [48][16] P[r][l] = Xn[r] . Wc_l (rows 0..31), b_j . Wc_l (rows 32 + j); Wc_L = w3c
    float* crA = crP + kCrossScal;     // DCN: [32][16] a_l of every row (x_l = a_l x0 + c_l)
    float* crF = crA + kTM * 16;       // DCN: [32][16] coeff[r][l] = d loss / d P[r][l]
    float* cwL = crF + kTM * 16;       // DCN: [L][CP] cross kernels | [L][CP] cross biases | [CP] w3c, zero beyond C
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int s = lane >> 5, c = lane & 31, n16 = lane & 15, kq = lane >> 4;
    const int m0 = blockIdx.x * kTM;
    const Part3 pl = part3_layout(dm.CP, LC ? dc.L : 0, G3 ? 1 : 0);
    double* prec = part + (int64_t)((int)blockIdx.x & (kRecShards - 1)) * pl.stride;     // this tile's record entries are ADDED (racc)

    // ---- prologue: chunks 0 and 1 of X and W1L (everything else is issued inside the GEMM) ----
    const int qcol = 4 * (tid & 15), srow = tid >> 4;      // staging: this thread owns 4 columns of rows srow, srow + 16
    floatx4 xv[NCH][2];                                    // raw X, kept to the end (d w_lin partial sums)
    auto xload1 = [&](int j, int u) {       // unconditional: the workspace rows of a ragged last tile are zero (host memset)
        xv[j][u] = ld4(X + (int64_t)(m0 + srow + 16 * u) * CP + 64 * j + qcol);
    };
    const floatx4* w1l = reinterpret_cast<const floatx4*>(p.W1L) + wave * 64 + lane;     // + 256 per k-group g
    floatx4 bq[3][8];
    xload1(0, 0); xload1(0, 1);
#pragma unroll
    for (int g8 = 0; g8 < 8; ++g8) bq[0][g8] = w1l[g8 * 256];
    if (NCH > 1) {
        xload1(NCH > 1 ? 1 : 0, 0); xload1(NCH > 1 ? 1 : 0, 1);
#pragma unroll
        for (int g8 = 0; g8 < 8; ++g8) bq[1][g8] = w1l[(8 + g8) * 256];
    }
    DT_STAMP(stamps, 6);
    // BN statistics behind the loads just issued: mean / rstd of this thread's columns from kernel A's batch sums (every
    // block for itself: 16 L2-resident 8-byte loads per column)
    float bnv[4][(CP + 255) / 256];
#pragma unroll
    for (int i = 0; i < (CP + 255) / 256; ++i) {
        const int col = tid + 256 * i;
        bnv[0][i] = 0.f; bnv[1][i] = 0.f; bnv[2][i] = 0.f; bnv[3][i] = 0.f;
        float rstd = 0.f, var = 0.f;
        if (col < dm.C) {
            bn_stats_col(p.bnacc, dm.CP, dm.B, col, bnv[0][i], var);
            rstd = 1.0f / sqrtf(var + p.eps);
            bnv[1][i] = rstd * p.gamma[col];
            bnv[2][i] = p.beta[col];
            bnv[3][i] = rstd;
        }
        if (blockIdx.x == 0 && col < CP) {         // published for kernels E / D (launched after this one) + moving statistics
            p.mean_w[col] = bnv[0][i]; p.rstd_w[col] = rstd; p.sc_w[col] = bnv[1][i]; p.betap_w[col] = bnv[2][i];
            p.gammap_w[col] = col < dm.C ? p.gamma[col] : 0.f;
            if (col < dm.C) {
                if (p.moving_mean) p.moving_mean[col] = p.moving_mean[col] * p.momentum + bnv[0][i] * (1.f - p.momentum);
                if (p.moving_var) p.moving_var[col] = p.moving_var[col] * p.momentum + var * (1.f - p.momentum);
            }
        }
    }
#pragma unroll
    for (int i = 0; i < (CP + 255) / 256; ++i) {
        const int col = tid + 256 * i;
        if (col < CP) { bnp[col] = bnv[0][i]; bnp[CP + col] = bnv[1][i]; bnp[2 * CP + col] = bnv[2][i]; bnp[3 * CP + col] = bnv[3][i]; }
    }
    lds_barrier();
    DT_STAMP(stamps, 7);
    // Xn = BN(X) is formed on the way into LDS
    floatx4 bnq[3];
    auto bnread = [&](int j) {
        bnq[0] = ld4(bnp + 64 * j + qcol);
        bnq[1] = ld4(bnp + CP + 64 * j + qcol);
        bnq[2] = ld4(bnp + 2 * CP + 64 * j + qcol);
    };
    auto xwrite = [&](int j) {
        st4(xs + srow * XS + 64 * j + qcol, (xv[j][0] - bnq[0]) * bnq[1] + bnq[2]);
        st4(xs + (srow + 16) * XS + 64 * j + qcol, (xv[j][1] - bnq[0]) * bnq[1] + bnq[2]);
    };
    bnread(0);
    xwrite(0);
    lds_barrier();
    DT_STAMP(stamps, 1);

    // ---- GEMM1: [32 x CP] . [CP x 128]; wave w owns hidden units [32w, 32w+32); two accumulator chains ----
    floatx16 acc, acc2;
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc[r] = 0.f; acc2[r] = 0.f; }
    floatx4 w2q[8];                    // GEMM2's B operand: fetched in the load slots of the last chunk
    {
        const floatx4* w2l = reinterpret_cast<const floatx4*>(p.W2L) + wave * 64 + lane;
        const float* arow = xs + c * XS + 4 * s;
        floatx4 aq[2][4];
        auto aread = [&](int j, int h) {
#pragma unroll
            for (int i = 0; i < 4; ++i) aq[h][i] = ld4(arow + 64 * j + 32 * h + 8 * i);
        };
        auto half = [&](int j, int h) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const floatx4 a = aq[h][i];
                const floatx4 b = bq[j % 3][4 * h + i];
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc, 0, 0, 0);
                acc2 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc2, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, acc, 0, 0, 0);
                acc2 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, acc2, 0, 0, 0);
                // one or two loads per four MFMAs: chunk j+2's operands (or, in the last chunk, GEMM2's)
                if (j + 2 < NCH) {
                    bq[(j + 2) % 3][4 * h + i] = w1l[(8 * (j + 2) + 4 * h + i) * 256];
                    if (i == 0) xload1(j + 2 < NCH ? j + 2 : 0, h);
                } else if (j == NCH - 1) {
                    w2q[4 * h + i] = w2l[(4 * h + i) * 256];
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        };
        aread(0, 0);
#pragma unroll
        for (int j = 0; j < NCH; ++j) {
            aread(j, 1);
            if (j + 1 < NCH) bnread(j + 1);
            __builtin_amdgcn_sched_barrier(0);
            half(j, 0);
            if (j + 1 < NCH) {
                xwrite(j + 1);          // chunk j+1 lands in LDS between the two halves of chunk j
                lds_barrier();
                aread(j + 1, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
            half(j, 1);
        }
    }
    DT_STAMP(stamps, 2);
    // operands needed after GEMM2 (their latency hides under it)
    floatx4 w2tq[8];
    {
        const floatx4* w2tl = reinterpret_cast<const floatx4*>(p.W2TL) + wave * 64 + lane;
#pragma unroll
        for (int g = 0; g < 8; ++g) w2tq[g] = w2tl[g * 256];
    }
    const float bias1 = p.b1[32 * wave + c];
    const float b2v = p.b2[16 * wave + n16], w3v = p.w3[16 * wave + n16];
    // DCN: this thread's share of the cross vectors (kernels | biases | w3c), on its way to LDS behind GEMM2
    constexpr int kStage = LC ? ((2 * LC + 1) * CP + 255) / 256 : 1;
    float cst[kStage];
    if constexpr (LC > 0) {
        const int nv = (2 * dc.L + 1) * CP;
#pragma unroll
        for (int u = 0; u < kStage; ++u) {
            const int e = min(tid + 256 * u, nv - 1);
            const int v = e / CP, col = min(e - v * CP, dm.C - 1);
            const float* src = v < dc.L ? dc.cw + (int64_t)v * dm.C : v < 2 * dc.L ? dc.cb + (int64_t)(v - dc.L) * dm.C : dc.w3c;
            cst[u] = src[col];
        }
    }
    float linv = 0.f, fmv = 0.f, yv = 0.f, wov = 0.f, bov = 0.f, swv = 1.f;
    if (wave == 0) {
        wov = p.wo[0];
        bov = p.bo ? p.bo[0] : 0.f;
        if (lane < 32 && m0 + lane < dm.B) {
            if (LC == 0) { linv = lin[m0 + lane]; fmv = fm[m0 + lane]; }
            yv = y[m0 + lane];
            if (dc.sw) swv = dc.sw[m0 + lane];
        }
    }
    float h1r[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = (r & 3) + 8 * (r >> 2) + 4 * s;
        h1r[r] = fmaxf((acc[r] + acc2[r]) + bias1, 0.f);
        h1s[row * HS + 32 * wave + c] = h1r[r];
    }
    lds_barrier();
    DT_STAMP(stamps, 3);

    // ---- GEMM2: [32 x 128] . [128 x 64] on 16x16x4 tiles: wave w owns columns [16w, 16w+16), both row halves ----
    float h2r[8];
    {
        floatx4 a0[8], a1[8];
#pragma unroll
        for (int G = 0; G < 8; ++G) {
            a0[G] = ld4(h1s + n16 * HS + 16 * G + 4 * kq);
            a1[G] = ld4(h1s + (16 + n16) * HS + 16 * G + 4 * kq);
        }
        // H1 leaves for HBM (k_wgrad3 reads it) as whole rows, from LDS
        floatx4 hrow[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) hrow[u] = ld4(h1s + (tid >> 5) * HS + 4 * (tid & 31) + 8 * u * HS);
        floatx4 c0 = {0.f, 0.f, 0.f, 0.f}, c1 = c0;
#pragma unroll
        for (int G = 0; G < 8; ++G) {
            const floatx4 b = w2q[G];
            c0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[G].x, b.x, c0, 0, 0, 0);
            c1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[G].x, b.x, c1, 0, 0, 0);
            c0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[G].y, b.y, c0, 0, 0, 0);
            c1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[G].y, b.y, c1, 0, 0, 0);
            c0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[G].z, b.z, c0, 0, 0, 0);
            c1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[G].z, b.z, c1, 0, 0, 0);
            c0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[G].w, b.w, c0, 0, 0, 0);
            c1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[G].w, b.w, c1, 0, 0, 0);
            if (G < 4) {
                const int m = m0 + (tid >> 5) + 8 * G;
                if (m < dm.B) st4_sel(H1 + (int64_t)m * kH1 + 4 * (tid & 31), hrow[G], G3 && dc.wt);
            }
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int row = 16 * (q >> 2) + 4 * kq + (q & 3);
            h2r[q] = fmaxf(((q >> 2) ? c1[q & 3] : c0[q & 3]) + b2v, 0.f);
            const float v = group_sum<16>(h2r[q] * w3v);
            if (n16 == 0) zp[wave * kTM + row] = v;
        }
    }
    if constexpr (LC > 0) {
        // ---- Cross forward (layers.py:428-436): x_{l+1} = x0 (x_l . w_l) + b_l + x_l.  By induction x_l = a_l x0 + c_l with
        //      a per-row SCALAR a_l and a row-independent vector c_l = b_0 + .. + b_{l-1}:
        //          s_l = x_l . w_l = a_l p_l + q_l,   p_l = x0 . w_l,   q_l = c_l . w_l,   a_{l+1} = a_l + s_l,  a_0 = 1
        //      so the whole network is ONE skinny GEMM P = Xn [32 x CP] . [w_0 .. w_{L-1} w3c] (fp32 MFMA 16x16x4; a third row
        //      tile holds the biases, giving the Gram entries b_j . w_l that make up q_l) and L scalar steps per row; the
        //      output only meets w3c:  z_c = w3c . x_L = a_L (x0 . w3c) + c_L . w3c.  (Round 2's first version walked the
        //      layers on the VALU with wave reductions per row and layer: 11.4 K cycles forward, 45 K backward.)
        {
            const int nv = (2 * dc.L + 1) * CP;
#pragma unroll
            for (int u = 0; u < kStage; ++u) {
                const int e = tid + 256 * u;
                if (e < nv) cwL[e] = (e % CP) < dm.C ? cst[u] : 0.f;
            }
        }
        lds_barrier();
        DT_STAMP(stamps, 9);
        float* pb = h1s;                   // [4][48][16] K-quarter partials (H1's LDS copy is dead until the backward)
        {
            const int L = dc.L;
            const float* brow = n16 < L ? cwL + n16 * CP : cwL + 2 * L * CP;      // B operand column n16: w_l, w3c, then zero
            const float bmask = n16 <= L ? 1.f : 0.f;
            const float* a2row = cwL + (L + min(n16, L - 1)) * CP;                // third row tile: the bias vectors
            const float a2mask = n16 < L ? 1.f : 0.f;
            floatx4 c0 = {0.f, 0.f, 0.f, 0.f}, c1 = c0, c2 = c0;
            const int kb = wave * (CP / 4);                                       // this wave's quarter of K (16 * NCH columns)
#pragma unroll
            for (int G = 0; G < NCH; ++G) {
                const int k = kb + 16 * G + 4 * kq;
                const floatx4 b = ld4(brow + k) * bmask;
                const floatx4 a0 = ld4(xs + n16 * XS + k), a1 = ld4(xs + (16 + n16) * XS + k);
                const floatx4 a2 = ld4(a2row + k) * a2mask;
                c0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.x, b.x, c0, 0, 0, 0);
                c1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.x, b.x, c1, 0, 0, 0);
                c2 = __builtin_amdgcn_mfma_f32_16x16x4f32(a2.x, b.x, c2, 0, 0, 0);
                c0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.y, b.y, c0, 0, 0, 0);
                c1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.y, b.y, c1, 0, 0, 0);
                c2 = __builtin_amdgcn_mfma_f32_16x16x4f32(a2.y, b.y, c2, 0, 0, 0);
                c0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.z, b.z, c0, 0, 0, 0);
                c1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.z, b.z, c1, 0, 0, 0);
                c2 = __builtin_amdgcn_mfma_f32_16x16x4f32(a2.z, b.z, c2, 0, 0, 0);
                c0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.w, b.w, c0, 0, 0, 0);
                c1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.w, b.w, c1, 0, 0, 0);
                c2 = __builtin_amdgcn_mfma_f32_16x16x4f32(a2.w, b.w, c2, 0, 0, 0);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {                                          // C layout: row 4 kq + i, column n16
                pb[wave * kCrossScal + (4 * kq + i) * 16 + n16] = c0[i];
                pb[wave * kCrossScal + (16 + 4 * kq + i) * 16 + n16] = c1[i];
                pb[wave * kCrossScal + (32 + 4 * kq + i) * 16 + n16] = c2[i];
            }
        }
        lds_barrier();
        for (int e = tid; e < kCrossScal; e += 256)
            crP[e] = (pb[e] + pb[kCrossScal + e]) + (pb[2 * kCrossScal + e] + pb[3 * kCrossScal + e]);
        lds_barrier();
        if (wave == 0 && lane < kTM) {                         // the L scalar steps of row `lane`, everything in registers
            const int L = dc.L;                                // (register arrays: compile-time indices only, L is a guard)
            static_assert(LC + 1 <= 12, "three float4 per row of crP");
            float pr[12], gq[LC][12];
            {
                const floatx4 t0 = ld4(crP + lane * 16), t1 = ld4(crP + lane * 16 + 4), t2 = ld4(crP + lane * 16 + 8);
#pragma unroll
                for (int e = 0; e < 4; ++e) { pr[e] = t0[e]; pr[4 + e] = t1[e]; pr[8 + e] = t2[e]; }
            }
#pragma unroll
            for (int j = 0; j < LC; ++j) {                     // Gram rows b_j . Wc_l (the same address in every lane: broadcast)
                const floatx4 t0 = ld4(crP + (32 + j) * 16), t1 = ld4(crP + (32 + j) * 16 + 4), t2 = ld4(crP + (32 + j) * 16 + 8);
#pragma unroll
                for (int e = 0; e < 4; ++e) { gq[j][e] = t0[e]; gq[j][4 + e] = t1[e]; gq[j][8 + e] = t2[e]; }
            }
            float a = 1.f, zc = 0.f;
#pragma unroll
            for (int l = 0; l <= LC; ++l) {
                float q = 0.f;                                 // q_l = (b_0 + .. + b_{l-1}) . Wc_l
#pragma unroll
                for (int j = 0; j < LC; ++j)
                    if (j < l) q += gq[j][l];
                if (l < L) {
                    crA[lane * 16 + l] = a;
                    a += a * pr[l] + q;
                } else if (l == L) {
                    crA[lane * 16 + l] = a;
                    zc = a * pr[l] + q;                        // z_c = w3c . x_L = a_L (x0 . w3c) + c_L . w3c
                }
            }
            zcs[lane] = zc;
        }
    }
    lds_barrier();
    DT_STAMP(stamps, 4);

    // ---- logits, loss, dlogit, dz (wave 0) ----
    if (wave == 0) {
        const int m = m0 + c;
        float loss = 0.f, dl = 0.f, zz = 0.f;
        if (m < dm.B) {
            const float pt = (zp[c] + zp[kTM + c]) + (zp[2 * kTM + c] + zp[3 * kTM + c]);
            zz = LC ? zcs[c] + pt                   // Dense(1)(Concatenate([cross, dnn])) (deepnets.py:194-207)
                    : (linv + fmv) + pt;             // Add([linear, fm, dnn]) order
            const float lg = zz * wov + bov;
            if (dc.mse) {        // regression task (deepmodel.py:130-131, 216): 'mse' on the linear task_output
                const float df = lg - yv;
                loss = df * df;
                dl = 2.0f * df / (float)dm.B;
            } else {
                const float pr = 1.0f / (1.0f + expf(-lg));
                loss = fmaxf(lg, 0.f) - lg * yv + log1pf(expf(-fabsf(lg)));
                dl = (pr - yv) / (float)dm.B;
            }
            loss *= swv;         // Keras: per-sample loss times its weight, summed, divided by the batch size
            dl *= swv;
            if (s == 0) {
                z_out[m] = zz;
                logit_out[m] = lg;
                dlogit[m] = dl;
                dz_out[m] = dl * wov;
            }
        }
        if (s == 0) dzs[c] = dl * wov;
        if (s == 1) { loss = 0.f; dl = 0.f; }        // lanes 32..63 mirror rows 0..31 (linv/fmv/yv are zero there)
        float aw = dl * zz, ab = dl;                 // d task_output kernel / bias
        loss = wave_sum(loss); aw = wave_sum(aw); ab = wave_sum(ab);
        if (lane == 0) { radd(prec + pl.loss, loss / (float)dm.B); radd(prec + pl.dwo, aw); radd(prec + pl.dbo, ab); }
    }
    lds_barrier();
    DT_STAMP(stamps, 5);

    // ---- top of the backward: dH2 (C layout of GEMM2), its column sums, dH1 = relu'(dH2 . W2^T) ----
    {
        float sb = 0.f, sw = 0.f;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int row = 16 * (q >> 2) + 4 * kq + (q & 3);
            const float dzv = dzs[row];
            const float g = h2r[q] > 0.f ? dzv * w3v : 0.f;
            dh2s[row * kH2S + 16 * wave + n16] = g;
            sb += g;
            sw += dzv * h2r[q];
        }
        sb += __shfl_xor(sb, 16, 64); sw += __shfl_xor(sw, 16, 64);
        sb += __shfl_xor(sb, 32, 64); sw += __shfl_xor(sw, 32, 64);
        if (kq == 0) { radd(prec + pl.db2 + 16 * wave + n16, sb); radd(prec + pl.dw3 + 16 * wave + n16, sw); }
    }
    lds_barrier();
    {
        floatx4 a[8];
#pragma unroll
        for (int g = 0; g < 8; ++g) a[g] = ld4(dh2s + c * kH2S + 8 * g + 4 * s);
        // dH2 leaves for HBM (k_wgrad3 reads it) as whole rows
        floatx4 drow[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) drow[u] = ld4(dh2s + ((tid >> 4) + 16 * u) * kH2S + 4 * (tid & 15));
        floatx16 da, db;
#pragma unroll
        for (int r = 0; r < 16; ++r) { da[r] = 0.f; db[r] = 0.f; }
#pragma unroll
        for (int g = 0; g < 8; ++g) {
            da = __builtin_amdgcn_mfma_f32_32x32x2f32(a[g].x, w2tq[g].x, da, 0, 0, 0);
            db = __builtin_amdgcn_mfma_f32_32x32x2f32(a[g].y, w2tq[g].y, db, 0, 0, 0);
            da = __builtin_amdgcn_mfma_f32_32x32x2f32(a[g].z, w2tq[g].z, da, 0, 0, 0);
            db = __builtin_amdgcn_mfma_f32_32x32x2f32(a[g].w, w2tq[g].w, db, 0, 0, 0);
            if (g < 2) {
                const int m = m0 + (tid >> 4) + 16 * g;
                if (m < dm.B) st4_sel(dH2 + (int64_t)m * kH2 + 4 * (tid & 15), drow[g], G3 && dc.wt);
            }
        }
        float colsum = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = (r & 3) + 8 * (r >> 2) + 4 * s;
            const float g = h1r[r] > 0.f ? da[r] + db[r] : 0.f;
            h1s[row * HS + 32 * wave + c] = g;       // H1's LDS copy is dead: every read of it sits before the last barrier
            colsum += g;
        }
        colsum += __shfl_xor(colsum, 32, 64);
        if (s == 0) radd(prec + pl.db1 + 32 * wave + c, colsum);
    }
    // d linear_logit kernel: sum_rows dz * X (raw) for this thread's 4 columns of every chunk, rows srow and srow+16;
    // the 4 row groups of a wave meet by shuffles, the 4 waves in LDS (the Xn tile is dead)
    if constexpr (LC == 0) {
        const float dza = dzs[srow], dzb = dzs[srow + 16];
#pragma unroll
        for (int j = 0; j < NCH; ++j) {
            floatx4 v = xv[j][0] * dza + xv[j][1] * dzb;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float t = v[e];
                t += __shfl_xor(t, 16, 64);
                t += __shfl_xor(t, 32, 64);
                v[e] = t;
            }
            if (kq == 0) st4(xs + wave * CP + 64 * j + qcol, v);
        }
    }
    lds_barrier();
#pragma unroll
    for (int u = 0; u < 4; ++u) {                    // dH1 leaves for HBM as whole rows
        const int r = (tid >> 5) + 8 * u;
        if (m0 + r < dm.B) st4_sel(dH1 + (int64_t)(m0 + r) * kH1 + 4 * (tid & 31), ld4(h1s + r * HS + 4 * (tid & 31)), G3 && dc.wt);
    }
    if constexpr (LC == 0) {
        for (int col = tid; col < CP; col += 256)
            radd(prec + pl.slin + col, (xs[col] + xs[CP + col]) + (xs[2 * CP + col] + xs[3 * CP + col]));
    } else {
        // ---- Cross backward in the closed form of the forward (x_L = a_L x0 + c_L, g = dz w3c):
        //   per row, scalars only:  A_L = d/d a_L = g . x0 = dz P[r][L];  for l = L-1 .. 0:  coeff_l = d/d p_l = A_{l+1} a_l,
        //                           A_l = A_{l+1} (1 + p_l);  coeff_L = dz a_L  (the weight of w3c in d/d x0)
        //   dXn_cross[r] = sum_l coeff[r][l] Wc_l                      -> HBM, kernel D adds it to dH1 . W1^T
        //   G_l = sum_r coeff[r][l] xhat[r]  (fp32 MFMA, K = the 32 rows)   -> the tile record, with the scalar sums
        //         Sco_l = sum_r coeff[r][l],  SA_l = sum_r A_{l+1},  Sdz = sum_r dz   (ones^T . M on the MFMA as well)
        //   Kernel E' finishes per column:  d w_l = gamma G_l + beta Sco_l + SA_l c_l,  d w3c likewise with Sdz c_L,
        //   d b_j = Sdz w3c + sum_{l > j} SA_l w_l,  and the cross path's two BN-backward sums  sum_l Sco_l Wc_l,  sum_l Wc_l G_l.
        const int L = dc.L;
        double* rec = prec + pl.cross;
        DT_STAMP(stamps, 10);
        float* crS = crA;                  // [32][16] A_{l+1} of every row (columns 0..L-1) and dz (column 15); a row's a_l are
                                           // in registers before its lane overwrites them
        if (wave == 0 && lane < kTM) {
            const int r = lane;
            float pr[12], av[12];
            {
                const floatx4 t0 = ld4(crP + r * 16), t1 = ld4(crP + r * 16 + 4), t2 = ld4(crP + r * 16 + 8);
                const floatx4 u0 = ld4(crA + r * 16), u1 = ld4(crA + r * 16 + 4), u2 = ld4(crA + r * 16 + 8);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    pr[e] = t0[e]; pr[4 + e] = t1[e]; pr[8 + e] = t2[e];
                    av[e] = u0[e]; av[4 + e] = u1[e]; av[8 + e] = u2[e];
                }
            }
            const float dzv = dzs[r];
            float pL = 0.f, aL = 0.f;
#pragma unroll
            for (int l = 0; l <= LC; ++l) { pL = l == L ? pr[l] : pL; aL = l == L ? av[l] : aL; }
            float cf[16], sa[16];
#pragma unroll
            for (int l = 0; l < 16; ++l) { cf[l] = 0.f; sa[l] = 0.f; }
            float A = dzv * pL;
#pragma unroll
            for (int l = LC - 1; l >= 0; --l) {
                if (l < L) {
                    cf[l] = A * av[l];
                    sa[l] = A;
                    A *= 1.f + pr[l];
                }
            }
#pragma unroll
            for (int l = 0; l <= LC; ++l) cf[l] = l == L ? dzv * aL : cf[l];
            sa[15] = dzv;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                st4(crF + r * 16 + 4 * e, floatx4{cf[4 * e], cf[4 * e + 1], cf[4 * e + 2], cf[4 * e + 3]});
                st4(crS + r * 16 + 4 * e, floatx4{sa[4 * e], sa[4 * e + 1], sa[4 * e + 2], sa[4 * e + 3]});
            }
        }
        // xhat = (X - mean) rstd replaces Xn in the tile (every read of Xn lies before the barrier above)
#pragma unroll
        for (int j = 0; j < NCH; ++j) {
            const floatx4 mu = ld4(bnp + 64 * j + qcol), rs = ld4(bnp + 3 * CP + 64 * j + qcol);
            st4(xs + srow * XS + 64 * j + qcol, (xv[j][0] - mu) * rs);
            st4(xs + (srow + 16) * XS + 64 * j + qcol, (xv[j][1] - mu) * rs);
        }
        lds_barrier();
        DT_STAMP(stamps, 11);
        if constexpr (!G3) {   // dXn_cross: wave w owns rows 8 w .. 8 w + 7, lanes run along the columns (256-byte row segments to HBM)
            float wc[LC + 1][NCH];
#pragma unroll
            for (int l = 0; l <= LC; ++l) {
                const float* src = l < L ? cwL + l * CP : cwL + 2 * L * CP;
#pragma unroll
                for (int k = 0; k < NCH; ++k) wc[l][k] = l <= L ? src[64 * k + lane] : 0.f;
            }
            // no `l <= L` guard: the coefficient columns beyond L are zero and so is wc[l] (round 2's ISA reading: the
            // guards became 62 branches, each guarded term read its coefficient with a scalar ds_read_b32 + s_waitcnt — 72
            // exposed LDS latencies per wave).  A row's coefficients arrive as three 16-byte broadcast reads, the next
            // row's before this row's stores.
            static_assert(LC + 1 <= 12, "three float4 of coefficients per row");
            floatx4 cq[2][3];
            {
                const int row0 = wave * (kTM / 4);
                cq[0][0] = ld4(crF + row0 * 16); cq[0][1] = ld4(crF + row0 * 16 + 4); cq[0][2] = ld4(crF + row0 * 16 + 8);
            }
#pragma unroll
            for (int r8 = 0; r8 < kTM / 4; ++r8) {
                const int row = wave * (kTM / 4) + r8;
                const int64_t m = m0 + row;
                if (r8 + 1 < kTM / 4) {
                    cq[(r8 + 1) & 1][0] = ld4(crF + (row + 1) * 16);
                    cq[(r8 + 1) & 1][1] = ld4(crF + (row + 1) * 16 + 4);
                    cq[(r8 + 1) & 1][2] = ld4(crF + (row + 1) * 16 + 8);
                }
                float acc[NCH];
#pragma unroll
                for (int k = 0; k < NCH; ++k) acc[k] = 0.f;
#pragma unroll
                for (int l = 0; l <= LC; ++l) {
                    const float cf = cq[r8 & 1][l >> 2][l & 3];
#pragma unroll
                    for (int k = 0; k < NCH; ++k) acc[k] += cf * wc[l][k];
                }
                if (m < dm.B) {
#pragma unroll
                    for (int k = 0; k < NCH; ++k) dc.dXc[m * CP + 64 * k + lane] = acc[k];
                }
            }
        }
        if (wave == 3) {   // the scalar sums over the tile's rows: ones^T . [coeff | A, dz] on the MFMA (every output row equal)
            floatx4 d1 = {0.f, 0.f, 0.f, 0.f}, d2 = d1;
#pragma unroll
            for (int st = 0; st < 8; ++st) {
                d1 = __builtin_amdgcn_mfma_f32_16x16x4f32(1.f, crF[(4 * st + kq) * 16 + n16], d1, 0, 0, 0);
                d2 = __builtin_amdgcn_mfma_f32_16x16x4f32(1.f, crS[(4 * st + kq) * 16 + n16], d2, 0, 0, 0);
            }
            if (kq == 0) { radd(rec + (L + 1) * CP + n16, d1[0]); radd(rec + (L + 1) * CP + 16 + n16, d2[0]); }
        }
        {   // G = Xhat^T . coeff: wave w owns the 16-column tiles w, w + 4, ..; K = the tile's 32 rows (8 steps)
            float bop[8];
#pragma unroll
            for (int st = 0; st < 8; ++st) bop[st] = crF[(4 * st + kq) * 16 + n16];
#pragma unroll
            for (int t = 0; t < NCH; ++t) {
                const int ct = wave + 4 * t;
                floatx4 d = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int st = 0; st < 8; ++st)
                    d = __builtin_amdgcn_mfma_f32_16x16x4f32(xs[(4 * st + kq) * XS + 16 * ct + n16], bop[st], d, 0, 0, 0);
                if (n16 <= L) {                                   // C layout: Xhat column 16 ct + 4 kq + i, coefficient n16
                    st4(dc.gpart + (int64_t)blockIdx.x * dc.gstride + n16 * CP + 16 * ct + 4 * kq, d);
                }
            }
        }
        DT_STAMP(stamps, 12);
    }
    DT_STAMP(stamps, 8);
    if constexpr (G3) {
        // ---- dXn = dH1 . W1^T on the tile (see the kernel's head).  xs <- xhat = (X - mean) rstd (the d w_lin partials in
        //      it have been read), A = the dH1 tile in h1s (both 16-row halves share a W1 operand), wave w owns the
        //      16-column blocks w, w + 4, ..; block k's epilogue (partial sums; dXn replaces xhat in place) is issued
        //      between the MFMA groups of block k + 1.
        // 32x32x2 tiles (half as many matrix instructions per flop as 16x16x4: with ONE wave per SIMD every instruction
        // issued between two MFMAs is a bubble of the pipe — the 16x16x4 form of this loop ran at 58 % of the pipe's rate,
        // 24.7 K cycles for 14.3 K of MFMA work).  K permutation as in GEMM1: lane (c, s), step 4g + j <-> k = 8g + 4s + j,
        // so A = 16 float4 of row c of the dH1 tile and B = 16 float4 of row `col` of the row-major W1.
        const int nblk = (dm.C + 31) >> 5;
        auto w1row = [&](int blk) {          // row `col` of W1 [C][128], this lane's 4 k of every 8 (clamped: never stored)
            const int col = min(32 * blk + c, dm.C - 1);
            return p.W1 + (int64_t)col * kH1 + 4 * s;
        };
        floatx4 bW[2][16];
        if (wave < nblk) {       // the first block's W1 operand is on its way while the tile is re-staged
            const float* wrow = w1row(wave);
#pragma unroll
            for (int g = 0; g < 16; ++g) bW[0][g] = ld4(wrow + 8 * g);
        }
        lds_barrier();
        if constexpr (LC == 0) {     // (DCN: the cross backward above has already put xhat there)
#pragma unroll
            for (int j = 0; j < NCH; ++j) {
                const floatx4 mu = ld4(bnp + 64 * j + qcol), rs = ld4(bnp + 3 * CP + 64 * j + qcol);
                st4(xs + srow * XS + 64 * j + qcol, (xv[j][0] - mu) * rs);
                st4(xs + (srow + 16) * XS + 64 * j + qcol, (xv[j][1] - mu) * rs);
            }
        }
        // DCN: A operand of the 16 extra K steps = row c of the coefficient tile crF [32][16] (k = 8 g + 4 s + j as above)
        floatx4 aC[2] = {floatx4{0.f, 0.f, 0.f, 0.f}, floatx4{0.f, 0.f, 0.f, 0.f}};
        if constexpr (LC > 0) {
            aC[0] = ld4(crF + c * 16 + 4 * s);
            aC[1] = ld4(crF + c * 16 + 8 + 4 * s);
        }
        floatx4 aA[16];
#pragma unroll
        for (int g = 0; g < 16; ++g) aA[g] = ld4(h1s + c * HS + 8 * g + 4 * s);
        lds_barrier();
        DT_STAMP(stamps, 13);
        // one epilogue slice (accumulator register r of 16) of block `blk`: the lane holds column 32 blk + c of row
        // (r % 4) + 8 (r / 4) + 4 s
        float s1 = 0.f, s2 = 0.f;
        auto epi_addr = [&](int blk, int r) { return xs + ((r & 3) + 8 * (r >> 2) + 4 * s) * XS + 32 * blk + c; };
        auto epi_q = [&](int blk, float gx, int r, float xh) {
            s1 += gx;
            s2 += gx * xh;
            *epi_addr(blk, r) = gx;
        };
        auto epi_end = [&](int blk) {
            const int col = 32 * blk + c;
            const float a = s1 + __shfl_xor(s1, 32, 64), b = s2 + __shfl_xor(s2, 32, 64);      // the two row halves (s = 0, 1)
            if (s == 0 && col < dm.C) { radd(prec + pl.sdx + col, a); radd(prec + pl.sdxx + col, b); }
            s1 = 0.f; s2 = 0.f;
        };
        // block `blk` from W1 buffer `buf` into `out`; the previous block's 16 epilogue slices ride between the 16 groups
        auto mm3 = [&](int buf, int blk, floatx16& out, int pblk, const floatx16& prev) {
            floatx16 a1, a2;
#pragma unroll
            for (int r = 0; r < 16; ++r) { a1[r] = 0.f; a2[r] = 0.f; }
            const bool more = blk + 4 < nblk;
            const float* wnext = w1row(blk + 4);
#pragma unroll
            for (int g = 0; g < 16; ++g) {
                // the previous block's slice g: its xhat read is issued BEFORE this group's MFMAs and consumed after them
                const float xh = pblk >= 0 ? *epi_addr(pblk, g) : 0.f;
                __builtin_amdgcn_sched_barrier(0);
                const floatx4 a = aA[g], b = bW[buf][g];
                a1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, a1, 0, 0, 0);
                a2 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, a2, 0, 0, 0);
                a1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, a1, 0, 0, 0);
                a2 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, a2, 0, 0, 0);
                if (more) bW[buf ^ 1][g] = ld4(wnext + 8 * g);        // the next block's W1 operand, one load per 4 MFMAs
                if (pblk >= 0) epi_q(pblk, prev[g], g, xh);
                __builtin_amdgcn_sched_barrier(0);
            }
            if constexpr (LC > 0) {
                // + sum_l coeff[r][l] Wc_l[col]: B = the layer vectors of this column from LDS (cwL: kernels | biases | w3c,
                // zero beyond C), Wc_L = w3c, nothing beyond L (the coefficient columns there are zero as well)
                const int L = dc.L, col = 32 * blk + c;
#pragma unroll
                for (int g2 = 0; g2 < 2; ++g2) {
                    float bw[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int l = 8 * g2 + 4 * s + j;
                        const float* src = l < L ? cwL + l * CP : cwL + 2 * L * CP;
                        const float v = src[col];
                        bw[j] = l <= L ? v : 0.f;
                    }
                    a1 = __builtin_amdgcn_mfma_f32_32x32x2f32(aC[g2].x, bw[0], a1, 0, 0, 0);
                    a2 = __builtin_amdgcn_mfma_f32_32x32x2f32(aC[g2].y, bw[1], a2, 0, 0, 0);
                    a1 = __builtin_amdgcn_mfma_f32_32x32x2f32(aC[g2].z, bw[2], a1, 0, 0, 0);
                    a2 = __builtin_amdgcn_mfma_f32_32x32x2f32(aC[g2].w, bw[3], a2, 0, 0, 0);
                }
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) out[r] = a1[r] + a2[r];
            if (pblk >= 0) epi_end(pblk);
        };
        {
            // buffer ids and result registers are literals: everything stays in registers (nblk <= 17: C <= 544 -> at most
            // 5 blocks per wave)
            floatx16 ra, rb;
#pragma unroll
            for (int r = 0; r < 16; ++r) { ra[r] = 0.f; rb[r] = 0.f; }
            int last = -1;
            if (wave < nblk) { mm3(0, wave, ra, -1, rb); last = wave; }
            if (wave + 4 < nblk) { mm3(1, wave + 4, rb, wave, ra); last = wave + 4; }
            if (wave + 8 < nblk) { mm3(0, wave + 8, ra, wave + 4, rb); last = wave + 8; }
            if (wave + 12 < nblk) { mm3(1, wave + 12, rb, wave + 8, ra); last = wave + 12; }
            if (wave + 16 < nblk) { mm3(0, wave + 16, ra, wave + 12, rb); last = wave + 16; }
            if (last >= 0) {                 // the last block's epilogue (its results: ra for an even count of blocks before it)
                const bool in_a = (((last - wave) >> 2) & 1) == 0;
                float xh[16];
#pragma unroll
                for (int r = 0; r < 16; ++r) xh[r] = *epi_addr(last, r);
#pragma unroll
                for (int r = 0; r < 16; ++r) epi_q(last, in_a ? ra[r] : rb[r], r, xh[r]);
                epi_end(last);
            }
        }
        lds_barrier();
        DT_STAMP(stamps, 14);
        // the tile's dXn rows leave as whole rows (the F*D embedding columns: the dense inputs need no gradient)
        const int fq = (dm.F * dm.D) >> 2;                 // 16-byte pieces per row (<= 128): 256 / fq rows per pass
        const int rgs = 256 / fq, rg = tid / fq, q = tid - rg * fq;
        if (rg < rgs) {
            for (int row = rg; row < kTM; row += rgs)
                if (m0 + row < dm.B) st4_sel(dxn_out + (int64_t)(m0 + row) * CP + 4 * q, ld4(xs + row * XS + 4 * q), dc.wt);
        }
        DT_STAMP(stamps, 15);
    }
}

// E: weight gradients on 64x128 macro tiles = 2x4 MFMA tiles whose rows / columns INTERLEAVE (tile (t,u) holds outputs
// (2i+t, 4j+u)), so ONE 8-byte load per lane feeds two tiles' worth of A and ONE 16-byte load four tiles' worth of B:
// two loads per EIGHT MFMAs, issued between the MFMA groups two chunks ahead.
//   macro a < CP/64 : M[64a .., :] = Xhat[:, 64a ..]^T dH1        (Xhat = (X - mean) rstd formed on the operand)
//   macro CP/64     : dW2^T = dH2^T H1  (the same loop with A = dH2 [64 cols], B = H1 [128 cols]; E' transposes)
// Each macro tile is split over `row_blocks` batch slices (blocks); a block's 4 waves take quarters of the slice and
// meet in LDS; the block's partial tile goes to `wpart` [macro][slice][64*128] with plain coalesced stores and E'
// adds the slices up — no atomics, no zero-fill, deterministic.  The first `nred_blocks` blocks reduce the per-tile
// partial sums C left in `part` (a block owns 64 consecutive record entries).
constexpr int kWgCh = 4;     // K steps (= 2 batch rows each) per operand chunk

// the optimizer's dense half for the step's last launch (k_finish_step): flat parameter / slot buffers laid out like the
// accumulator buffer (fused.py: "parameters mirror the gradient layout"), p == NULL: gradients only
struct DenseAdam {
    float *p, *m, *v;
    float lr_t, b1, b2, eps;
};

// Where record entry e (Part3 order) lands in the gradient buffer: -1 = nowhere (pads; the d w_lin column sums and DCN's
// cross record, which the finishing launch's column blocks read from the shards themselves and finish per column)
__device__ __forceinline__ int64_t record_dst(int e, const Part3& pl, const DeepFmAccum& al, const DeepFmDims& dm, int Lc) {
    if (e < pl.db1) return -1;                                   // slin (DeepFM; DCN: empty)
    if (e < pl.db2) return al.db1 + (e - pl.db1);
    if (e < pl.dw3) return al.db2 + (e - pl.db2);
    if (e < pl.dwo) return al.dw3d + (e - pl.dw3);
    if (e == pl.dwo) return al.dwo;
    if (e == pl.dbo) return al.dbo;
    if (e == pl.loss) return al.loss;
    if (pl.sdx >= 0 && e >= pl.sdx) {                            // the BN-backward batch sums = dbeta | dgamma
        const bool xx = e >= pl.sdxx;
        const int col = e - (xx ? pl.sdxx : pl.sdx);
        return col < dm.C ? (xx ? al.dgamma : al.dbeta) + col : -1;
    }
    return -1;
}

// One thread finishes record entry e: the shards' sum -> the gradient buffer, and (da.p != NULL: k_finish_step) the
// Keras-Adam update of that dense element — db1, db2, the dnn part of dw3, d w_out, d b_out, dgamma, dbeta; the `loss` word
// is a pad of the parameter buffer and takes none.
__device__ __forceinline__ void finish_record_entry(int e, const RecSrc& rs, const Part3& pl, const DeepFmAccum& al,
                                                    const DeepFmDims& dm, int Lc, float* __restrict__ accum,
                                                    const DenseAdam& da) {
    if (e >= pl.n) return;
    const int64_t dst = record_dst(e, pl, al, dm, Lc);
    if (dst < 0) return;
    const bool upd = da.p && dst != al.loss && dst != al.loss + 1;
    float pp = 0.f, pm = 0.f, pv = 0.f;            // the optimizer's operands travel with the shards: one round trip, not two
    if (upd) { pp = da.p[dst]; pm = da.m[dst]; pv = da.v[dst]; }
    const float v = rec_sum(rs, e);
    accum[dst] = v;
    if (upd) {
        const float mi = da.b1 * pm + (1.f - da.b1) * v;
        const float vi = da.b2 * pv + (1.f - da.b2) * v * v;
        da.m[dst] = mi;
        da.v[dst] = vi;
        da.p[dst] = pp - da.lr_t * mi / (sqrtf(vi) + da.eps);
    }
}

// heavy block `hid` of the weight-gradient GEMMs, run by the block's first 256 threads (4 waves); they meet once, at the
// hardware barrier or — soft_cnt: an LDS word the caller zeroed — at a counter only they touch
__device__ __forceinline__ void wgrad_heavy(float* red, int hid, const float* __restrict__ X, const MlpParams& p,
                                            const DeepFmDims& dm, const float* __restrict__ H1,
                                            const float* __restrict__ dH1, const float* __restrict__ dH2, int row_blocks,
                                            int rows_per_block, float* __restrict__ wpart,
                                            unsigned long long* stamps_all, unsigned* soft_cnt = nullptr) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int s = lane >> 5, c = lane & 31;
    unsigned long long* stamps = stamps_all ? stamps_all + (int64_t)(hid - (int)blockIdx.x) * 16 : nullptr;   // DT_STAMP adds blockIdx.x * 16
    DT_STAMP(stamps, 0);
    const int nmac1 = dm.CP >> 6, nmac = nmac1 + 1;
    // XCD-aware (macro tile, slice) ids: all macro tiles of one batch slice read the same rows of X / dH1 / H1 / dH2,
    // so a slice's blocks share id % 8 and each XCD's L2 holds 1/8 of those arrays
    int mac, rb;
    if ((row_blocks & 7) == 0) {
        const int xcd = hid & 7, j = hid >> 3, per = row_blocks >> 3;
        mac = j % nmac;
        rb = xcd * per + j / nmac;
    } else {
        mac = hid % nmac;
        rb = hid / nmac;
    }
    const int rq = rows_per_block >> 2;                 // rows per wave (even)
    const int r_begin = rb * rows_per_block + wave * rq;
    const int r_end = min(dm.B, r_begin + rq);
    const bool first = mac < nmac1;
    const float* pa; const float* pb; int sa, sb;
    floatx2 mu = {0.f, 0.f}, rs = {1.f, 1.f};
    if (first) {
        const int ca = 64 * mac + 2 * c;
        pa = X + ca; sa = dm.CP; pb = dH1; sb = kH1;
        mu = *reinterpret_cast<const floatx2*>(p.mean + ca);
        rs = *reinterpret_cast<const floatx2*>(p.rstd + ca);
    } else {
        pa = dH2 + 2 * c; sa = kH2; pb = H1; sb = kH1;
    }
    pa += (int64_t)s * sa;
    pb += (int64_t)s * sb + 4 * c;
    floatx16 acc[2][4];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[t][u][r] = 0.f;
    {
        floatx2 aq[3][kWgCh];
        floatx4 bq[3][kWgCh];
        constexpr int span = 2 * kWgCh;                   // rows per chunk
        const int nfull = max(0, r_end - r_begin) / span;
        auto load1 = [&](int buf, int ch, int i) {
            const int row = r_begin + ch * span + 2 * i;
            aq[buf][i] = *reinterpret_cast<const floatx2*>(pa + (int64_t)row * sa);
            bq[buf][i] = ld4(pb + (int64_t)row * sb);
        };
        auto step = [&](floatx2 av, floatx4 bv) {
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, bv.x, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, bv.y, acc[0][1], 0, 0, 0);
            acc[0][2] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, bv.z, acc[0][2], 0, 0, 0);
            acc[0][3] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, bv.w, acc[0][3], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, bv.x, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, bv.y, acc[1][1], 0, 0, 0);
            acc[1][2] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, bv.z, acc[1][2], 0, 0, 0);
            acc[1][3] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, bv.w, acc[1][3], 0, 0, 0);
        };
        // chunk ch runs from buffer `buf` while chunk ch+2's loads are issued into buffer (buf + 2) % 3, one K step's
        // pair of loads after each group of eight MFMAs
        auto run = [&](int buf, int ch) {
            const bool pre = ch + 2 < nfull;
#pragma unroll
            for (int i = 0; i < kWgCh; ++i) {
                step((aq[buf][i] - mu) * rs, bq[buf][i]);
                if (pre) load1((buf + 2) % 3, ch + 2, i);
                __builtin_amdgcn_sched_barrier(0);
            }
        };
        if (nfull > 0) {
#pragma unroll
            for (int i = 0; i < kWgCh; ++i) load1(0, 0, i);
        }
        if (nfull > 1) {
#pragma unroll
            for (int i = 0; i < kWgCh; ++i) load1(1, 1, i);
        }
        DT_STAMP(stamps, 1);
        for (int ch = 0; ch < nfull; ch += 3) {
            run(0, ch);
            if (ch == 0) DT_STAMP(stamps, 2);
            if (ch + 1 >= nfull) break;
            run(1, ch + 1);
            if (ch + 2 >= nfull) break;
            run(2, ch + 2);
        }
        DT_STAMP(stamps, 3);
        for (int base = r_begin + nfull * span; base < r_end; base += 2) {      // ragged tail, one K step at a time
            floatx2 av = {0.f, 0.f};
            floatx4 bv = {0.f, 0.f, 0.f, 0.f};
            if (base + s < r_end) {
                av = (*reinterpret_cast<const floatx2*>(pa + (int64_t)base * sa) - mu) * rs;
                bv = ld4(pb + (int64_t)base * sb);
            }
            step(av, bv);
        }
    }
    // the four waves' partial macro tiles meet in LDS (four 32 KB slots): entry (2i+t)*128 + (4j+u)
    auto put = [&](float* slot) {
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int i = (r & 3) + 8 * (r >> 2) + 4 * s;
                st4(slot + (2 * i + t) * 128 + 4 * c, floatx4{acc[t][0][r], acc[t][1][r], acc[t][2][r], acc[t][3][r]});
            }
    };
    put(red + wave * 8192);
    if (soft_cnt) {
        // the four matrix waves meet WITHOUT the hardware barrier (which would also wait for the block's memory waves,
        // k_wgrad_rows): LDS operations of a wave complete in order, so a wave's arrival (ds_add) follows its partial tile
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if (lane == 0) atomicAdd(soft_cnt, 1u);
        while (*reinterpret_cast<volatile unsigned*>(soft_cnt) < 4u) __builtin_amdgcn_s_sleep(1);
        asm volatile("" ::: "memory");
    } else {
        __syncthreads();
    }
    DT_STAMP(stamps, 4);
    float* dst = wpart + ((int64_t)mac * row_blocks + rb) * 8192;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int e = 4 * (tid + 256 * u);
        st4(dst + e, (ld4(red + e) + ld4(red + 8192 + e)) + (ld4(red + 16384 + e) + ld4(red + 24576 + e)));
    }
    DT_STAMP(stamps, 5);
}

// Round 6: the same heavy block on the bf16 matrix cores.  Measured first (tools/r6/call8.sh, the K loop compiled out): the
// fp32-MFMA GEMM keeps the matrix waves away from the row epilogue for ~28 K of its ~69 K cycles — without it the launch takes
// 33.0 us instead of 41.6, the step 92.9 us instead of 101.9.  v_mfma_f32_32x32x16_bf16 contracts 16 batch rows per
// instruction at 16x the fp32 rate; a lane (c = l % 32, s = l / 32) holds the 8 rows 16 ch + 8 s + j of its columns, i.e. the
// same row loads as above with another row-to-lane assignment.  PARTS = 2 (the default tower mode, DT_STEP_TOWER_X3): both
// operands as hi + lo (16 mantissa bits), products hi hi + hi lo + lo hi, fp32 accumulation — 2^-17 per product, the
// precision of the tile kernel's backward products (dW within ~1e-5 of its largest entry); PARTS = 1 (DT_STEP_TOWER_BF16):
// plain bf16.  The exact-fp32 tower keeps wgrad_heavy.
typedef __bf16 wg_b8 __attribute__((ext_vector_type(8)));
template <int PARTS>
__device__ __forceinline__ void wgrad_heavy_bf16(float* red, int hid, const float* __restrict__ X, const MlpParams& p,
                                                 const DeepFmDims& dm, const float* __restrict__ H1,
                                                 const float* __restrict__ dH1, const float* __restrict__ dH2, int row_blocks,
                                                 int rows_per_block, float* __restrict__ wpart, unsigned* soft_cnt) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int s = lane >> 5, c = lane & 31;
    const int nmac1 = dm.CP >> 6, nmac = nmac1 + 1;
    int mac, rb;
    if ((row_blocks & 7) == 0) {
        const int xcd = hid & 7, j = hid >> 3, per = row_blocks >> 3;
        mac = j % nmac;
        rb = xcd * per + j / nmac;
    } else {
        mac = hid % nmac;
        rb = hid / nmac;
    }
    const int rq = rows_per_block >> 2;                 // rows per wave (a multiple of 2; 64 at B = 8192)
    const int r_begin = rb * rows_per_block + wave * rq;
    const int r_end = min(dm.B, r_begin + rq);
    const bool first = mac < nmac1;
    const float* pa; const float* pb; int sa, sb;
    floatx2 mu = {0.f, 0.f}, rs = {1.f, 1.f};
    if (first) {
        const int ca = 64 * mac + 2 * c;
        pa = X + ca; sa = dm.CP; pb = dH1; sb = kH1;
        mu = *reinterpret_cast<const floatx2*>(p.mean + ca);
        rs = *reinterpret_cast<const floatx2*>(p.rstd + ca);
    } else {
        pa = dH2 + 2 * c; sa = kH2; pb = H1; sb = kH1;
    }
    pb += 4 * c;
    floatx16 acc[2][4];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[t][u][r] = 0.f;
    // a chunk = 16 batch rows: this lane's 8 rows are r0 + 8 s + j.  Every load is unconditional from a clamped (valid) row;
    // rows beyond the wave's share contribute zeros
    floatx2 av[8];
    floatx4 bv[8];
    auto load_chunk = [&](int r0) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int row = min(r0 + 8 * s + j, dm.B - 1);
            av[j] = *reinterpret_cast<const floatx2*>(pa + (int64_t)row * sa);
            bv[j] = ld4(pb + (int64_t)row * sb);
        }
    };
    auto split8 = [](const float (&v)[8], wg_b8& hi, wg_b8& lo) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const __bf16 h = (__bf16)v[e];
            hi[e] = h;
            if constexpr (PARTS == 2) lo[e] = (__bf16)(v[e] - (float)h);
        }
    };
    if (r_begin < r_end) load_chunk(r_begin);
    for (int r0 = r_begin; r0 < r_end; r0 += 16) {
        wg_b8 ah[2], al[2], bh[4], bl[4];
        {
            float va[2][8], vb[4][8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const bool ok = r0 + 8 * s + j < r_end;
                const floatx2 a = ok ? (av[j] - mu) * rs : floatx2{0.f, 0.f};
                const floatx4 b = ok ? bv[j] : floatx4{0.f, 0.f, 0.f, 0.f};
                va[0][j] = a.x; va[1][j] = a.y;
                vb[0][j] = b.x; vb[1][j] = b.y; vb[2][j] = b.z; vb[3][j] = b.w;
            }
#pragma unroll
            for (int t = 0; t < 2; ++t) split8(va[t], ah[t], al[t]);
#pragma unroll
            for (int u = 0; u < 4; ++u) split8(vb[u], bh[u], bl[u]);
        }
        if (r0 + 16 < r_end) load_chunk(r0 + 16);           // the next chunk's rows fly under this chunk's products
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if constexpr (PARTS == 2) {
                    acc[t][u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[t], bl[u], acc[t][u], 0, 0, 0);
                    acc[t][u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[t], bh[u], acc[t][u], 0, 0, 0);
                }
                acc[t][u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[t], bh[u], acc[t][u], 0, 0, 0);
            }
    }
    // the four waves' partial macro tiles meet in LDS exactly as in wgrad_heavy (same accumulator layout)
    auto put = [&](float* slot) {
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int i = (r & 3) + 8 * (r >> 2) + 4 * s;
                st4(slot + (2 * i + t) * 128 + 4 * c, floatx4{acc[t][0][r], acc[t][1][r], acc[t][2][r], acc[t][3][r]});
            }
    };
    put(red + wave * 8192);
    if (soft_cnt) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if (lane == 0) atomicAdd(soft_cnt, 1u);
        while (*reinterpret_cast<volatile unsigned*>(soft_cnt) < 4u) __builtin_amdgcn_s_sleep(1);
        asm volatile("" ::: "memory");
    } else {
        __syncthreads();
    }
    float* dst = wpart + ((int64_t)mac * row_blocks + rb) * 8192;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int e = 4 * (tid + 256 * u);
        st4(dst + e, (ld4(red + e) + ld4(red + 8192 + e)) + (ld4(red + 16384 + e) + ld4(red + 24576 + e)));
    }
}

// E': adds up the batch slices of E and finishes the BN / W1 gradients.  With M = Xhat^T dH1 and db1 = colsum(dH1):
//   dgamma = sum_b dXn xhat = rowdot(W1, M)      dbeta = sum_b dXn = W1 . db1      dW1 = gamma M + beta (x) db1
// (dXn = dH1 W1^T is linear in dH1, so its two batch sums need no pass over it).  One wave per column of X; the
// waves after those transpose-sum dW2 (one per dH2 column); block 0 also folds the reduced sum_b dz X into
// d linear_logit kernel: field f = its D columns, dense k = one column.
// DCN: the tile kernel's per-tile cross records (DcnArgs.gpart [tiles][stride], stride = (L + 1) CP) and their sums over the
// tiles, gsum [(L + 1) CP]: formed by the matrix waves of the weight-gradient launch (reduce_gpart), read by the finishing launch
struct GPart {
    const float* part;
    int stride, tiles;
    float* gsum;
};
// matrix waves of weight-gradient block `blk` (256 threads, soft barriers: see k_wgrad_rows): entries [16 blk, 16 blk + 16) of the
// cross record summed over the tiles — thread = (entry, group of tiles), 16 partials per entry meet in LDS
__device__ __forceinline__ void reduce_gpart(const GPart& gp, float* lds, int blk, int nblk, int tid, ElectSync& sy) {
    const int ee = tid & 15, tg = tid >> 4;
    for (int e0 = 16 * blk; e0 < gp.stride; e0 += 16 * nblk) {
        float acc = 0.f;
        for (int t0 = tg; t0 < gp.tiles; t0 += 16 * 8) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int t = t0 + 16 * u;
                const float x = gp.part[(int64_t)min(t, gp.tiles - 1) * gp.stride + e0 + ee];       // unconditional, clamped
                v[u] = t < gp.tiles ? x : 0.f;
            }
            acc += ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
        }
        elect_barrier<256, true>(sy);                 // the LDS words below are free (the election / the partial tiles are done)
        lds[tg * 16 + ee] = acc;
        elect_barrier<256, true>(sy);
        if (tid < 16) {
            float t = 0.f;
#pragma unroll
            for (int g = 0; g < 16; ++g) t += lds[g * 16 + tid];
            gp.gsum[e0 + tid] = t;
        }
    }
}
// Chained steps: the split-bf16 tile kernel's weight layouts (X3Weights, tower_x3.h) written by the finishing launch from the
// weights it has just updated — the prep launch's layout blocks of the NEXT step (k_prep writes the same values from the
// same fp32 weights: every part is the bf16 rounding of what the parts before it left).  W1B == NULL: not written.
struct X3Lay {
    __bf16 *W1B, *W1R, *W2B, *W2R;
    int64_t w1b_lo, w1r_lo, w2b_lo, w2r_lo;
    float* cwp;                  // DCN: [2 L + 1][CP] fp32 copies of the cross kernels | biases | w3c
};
__device__ __forceinline__ void x3_parts(float v, __bf16 (&q)[3]) {
    float r = v;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const __bf16 a = (__bf16)r;
        q[k] = a;
        r -= (float)a;
    }
}

__device__ __forceinline__ void bn_grads2_body(const float* __restrict__ W1, const float* __restrict__ gamma,
                                               const float* __restrict__ beta, const DeepFmDims& dm, float* accum,
                                               const DeepFmAccum& al, const float* __restrict__ wpart, int row_blocks,
                                               int Lc, const float* __restrict__ cw, const float* __restrict__ cb,
                                               const float* __restrict__ w3c, const RecSrc& rs, const Part3& pl,
                                               floatx2 (*sm)[64], float* slin_s, const DenseAdam& da, int blk, const GPart& gp,
                                               const X3Lay& lay = X3Lay{nullptr, nullptr, nullptr, nullptr, 0, 0, 0, 0, nullptr}) {
    // (what the tile kernel summed over the batch — db1, the d w_lin column sums, DCN's cross record — is read from the
    // record shards here: no launch stands between kernel C and this one for them)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (blk == 0 && Lc == 0) {
        // d linear_logit kernel: field f = the sum of its D columns of sum_b dz X.  Every column sum is fetched by its own
        // thread (ONE round trip for the block; a thread walking its field's D columns made D dependent ones — the longest
        // chain of the launch), the fields are added up from LDS.
        float* sl = reinterpret_cast<float*>(slin_s);
        for (int c = threadIdx.x; c < dm.C; c += blockDim.x) sl[c] = rec_sum(rs, pl.slin + c);
        __syncthreads();
        for (int q = threadIdx.x; q < dm.F + dm.Nd; q += blockDim.x) {
            float v = 0.f;
            if (q < dm.F) {
                for (int d = 0; d < dm.D; ++d) v += sl[q * dm.D + d];
            } else {
                v = sl[dm.F * dm.D + (q - dm.F)];
            }
            accum[al.dwlin + q] = v;
            if (da.p) adam_one(da.p, da.m, da.v, al.dwlin + q, v, da.lr_t, da.b1, da.b2, da.eps);
        }
    }
    // one block per column (of X, then of dH2); its 4 waves add up every 4th batch slice with all loads in flight
    const int col = blk;
    const bool w2 = col >= dm.C;
    const int mac = w2 ? (dm.CP >> 6) : (col >> 6), row = w2 ? col - dm.C : (col & 63);
    const float* src = wpart + (int64_t)mac * row_blocks * 8192 + row * 128 + 2 * lane;
    // wave 0's operands of the final formulas travel with the slices (one memory round trip per block, not two)
    floatx2 w = {0.f, 0.f}, d = {0.f, 0.f};
    float ga = 0.f, be = 0.f;
    typedef double doublex2 __attribute__((ext_vector_type(2)));
    doublex2 dq[kRecShards];         // db1[2 lane, 2 lane + 1] of every shard: requested here, summed behind the slices' loads
#pragma unroll
    for (int sh = 0; sh < kRecShards; ++sh) dq[sh] = doublex2{0.0, 0.0};
    if (wave == 0 && !w2) {
        w = *reinterpret_cast<const floatx2*>(W1 + (int64_t)col * kH1 + 2 * lane);
#pragma unroll
        for (int sh = 0; sh < kRecShards; ++sh)
            dq[sh] = *reinterpret_cast<const doublex2*>(rs.racc + (int64_t)sh * rs.stride + pl.db1 + 2 * lane);
        ga = gamma[col]; be = beta[col];
    }
    // the optimizer's p / m / v of the two elements wave 0 finishes: fetched with the slices (k_finish_step), not after them
    const int64_t e0 = w2 ? al.dW2 + (int64_t)(2 * lane) * kH2 + row : al.dW1 + (int64_t)col * kH1 + 2 * lane;
    const int64_t e1 = w2 ? e0 + kH2 : e0 + 1;
    float pp[2] = {0.f, 0.f}, pm[2] = {0.f, 0.f}, pv[2] = {0.f, 0.f};
    if (da.p && wave == 0) {
        pp[0] = da.p[e0]; pp[1] = da.p[e1]; pm[0] = da.m[e0]; pm[1] = da.m[e1]; pv[0] = da.v[e0]; pv[1] = da.v[e1];
    }
    float pnew[2] = {0.f, 0.f};                   // the two updated weights (chained steps: their bf16 parts go to the layouts)
    auto adam2 = [&](float g0, float g1) {       // Keras Adam on elements e0, e1 from the prefetched slots
        const float g[2] = {g0, g1};
        const int64_t ei[2] = {e0, e1};
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const float mi = da.b1 * pm[k] + (1.f - da.b1) * g[k];
            const float vi = da.b2 * pv[k] + (1.f - da.b2) * g[k] * g[k];
            da.m[ei[k]] = mi;
            da.v[ei[k]] = vi;
            pnew[k] = pp[k] - da.lr_t * mi / (sqrtf(vi) + da.eps);
            da.p[ei[k]] = pnew[k];
        }
    };
    floatx2 v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int sl = wave + 4 * u;
        v[u] = floatx2{0.f, 0.f};
        if (sl < row_blocks) v[u] = *reinterpret_cast<const floatx2*>(src + (int64_t)sl * 8192);
    }
    floatx2 m = ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
    for (int sl = wave + 32; sl < row_blocks; sl += 4) m += *reinterpret_cast<const floatx2*>(src + (int64_t)sl * 8192);
    sm[wave][lane] = m;
    __syncthreads();
    if (wave != 0) return;
    m = (sm[0][lane] + sm[1][lane]) + (sm[2][lane] + sm[3][lane]);
    {
        doublex2 t = dq[0];
#pragma unroll
        for (int sh = 1; sh < kRecShards; ++sh) t += dq[sh];
        d = floatx2{(float)t[0], (float)t[1]};
    }
    if (w2) {       // row `row` of dW2^T: dW2[k][row] for k = 2 lane, 2 lane + 1
        accum[e0] = m.x;
        accum[e1] = m.y;
        if (da.p) adam2(m.x, m.y);
        if (da.p && lay.W1B) {
            // W2[k][n = row], k = 2 lane + i.  W2R: row-major [128][64]; W2B: element j of lane (n % 16, g), step s, column tile t
            // = W2[32 s + 8 g + j][16 t + n % 16] — k = 2 lane, 2 lane + 1 are neighbours j, j + 1 of one lane's 8
            __bf16 q0[3], q1[3];
            x3_parts(pnew[0], q0);
            x3_parts(pnew[1], q1);
            const int k0 = 2 * lane, n = row;
            const int64_t ib = ((((int64_t)(k0 >> 5) * 4 + (n >> 4)) * 64) + ((k0 >> 3) & 3) * 16 + (n & 15)) * 8 + (k0 & 7);
#pragma unroll
            for (int pt = 0; pt < 3; ++pt) {
                typedef __bf16 b2 __attribute__((ext_vector_type(2)));
                *reinterpret_cast<b2*>(lay.W2B + pt * lay.w2b_lo + ib) = b2{q0[pt], q1[pt]};
            }
#pragma unroll
            for (int pt = 0; pt < 2; ++pt) {
                lay.W2R[pt * lay.w2r_lo + (int64_t)k0 * kH2 + n] = q0[pt];
                lay.W2R[pt * lay.w2r_lo + (int64_t)(k0 + 1) * kH2 + n] = q1[pt];
            }
        }
        return;
    }
    const float dg = wave_sum(w.x * m.x + w.y * m.y);
    const float db = wave_sum(w.x * d.x + w.y * d.y);
    const float ga_b = ga, be_b = be;
    {
        const floatx2 g = floatx2{ga * m.x + be * d.x, ga * m.y + be * d.y};
        *reinterpret_cast<floatx2*>(accum + e0) = g;
        if (da.p) adam2(g.x, g.y);
        if (da.p && lay.W1B) {
            // W1[k = col][n], n = 2 lane + i.  W1R: row-major [CP][128]; W1B: element j of lane (n % 16, g), step s, wave w
            // = W1[32 s + 8 g + j][16 w + n % 16]
            __bf16 q0[3], q1[3];
            x3_parts(pnew[0], q0);
            x3_parts(pnew[1], q1);
            const int k = col, n0 = 2 * lane;
            const int64_t kb = ((int64_t)(k >> 5) * 8) * 64 * 8 + (((k >> 3) & 3) * 16) * 8 + (k & 7);
            const int64_t i0 = kb + ((int64_t)(n0 >> 4) * 64 + (n0 & 15)) * 8, i1 = kb + ((int64_t)((n0 + 1) >> 4) * 64 + ((n0 + 1) & 15)) * 8;
#pragma unroll
            for (int pt = 0; pt < 3; ++pt) {
                lay.W1B[pt * lay.w1b_lo + i0] = q0[pt];
                lay.W1B[pt * lay.w1b_lo + i1] = q1[pt];
            }
#pragma unroll
            for (int pt = 0; pt < 2; ++pt) {
                typedef __bf16 b2 __attribute__((ext_vector_type(2)));
                *reinterpret_cast<b2*>(lay.W1R + pt * lay.w1r_lo + (int64_t)k * kH1 + n0) = b2{q0[pt], q1[pt]};
            }
        }
    }
    if (Lc) {
        // DCN: lane l <= Lc finishes layer l of this column (lane Lc: the w3c entry) — the gradients, and in
        // k_finish_step their Adam update, of the 2 Lc + 1 elements run side by side (one lane walking them took 13
        // dependent round trips: 19 us for the launch).  The BN-backward sums are the tile kernel's (sdx / sdxx).
        // Cross record (see the cross backward of kernel C): vectors G_0 .. G_L [CP] | scalars [32]: Sco_l at l, SA_l at 16 + l, Sdz at 31
        const int scal = pl.cross + (Lc + 1) * dm.CP;
        // every shard sum this column needs is requested at once (lane j holds SA_j / Sco_j; a lane walking them one after
        // the other paid Lc dependent round trips)
        const int l = lane;
        const float sa_mine = l < Lc ? rec_sum(rs, scal + 16 + l) : 0.f;
        const float sco_mine = l <= Lc ? rec_sum(rs, scal + l) : 0.f;
        const float G = l <= Lc ? gp.gsum[(int64_t)l * dm.CP + col] : 0.f;     // (summed over the tiles by the weight-gradient launch)
        const float sdz = rec_sum(rs, scal + 31);
        float cl = 0.f, suf = 0.f;                            // c_l = b_0 + .. + b_{l-1};  sum_{j > l} SA_j w_j
        for (int j = 0; j < Lc; ++j) {
            const float saj = __shfl(sa_mine, j, 64);
            const float bj = cb[(int64_t)j * dm.C + col], wj = cw[(int64_t)j * dm.C + col];
            if (j < l) cl += bj;
            if (j > l) suf += saj * wj;
        }
        if (l <= Lc) {
            const int64_t ig = l < Lc ? al.dcw + (int64_t)l * dm.C + col : al.dw3 + col;
            const float gw = ga_b * G + be_b * sco_mine + (l < Lc ? sa_mine : sdz) * cl;
            const float gb = sdz * w3c[col] + suf;                // d b_l (l < Lc)
            accum[ig] = gw;
            if (l < Lc) accum[al.dcb + (int64_t)l * dm.C + col] = gb;
            if (da.p) {
                adam_one(da.p, da.m, da.v, ig, gw, da.lr_t, da.b1, da.b2, da.eps);
                if (l < Lc) adam_one(da.p, da.m, da.v, al.dcb + (int64_t)l * dm.C + col, gb, da.lr_t, da.b1, da.b2, da.eps);
                if (lay.cwp) {       // chained steps: the padded fp32 copies [cross kernels | cross biases | w3c] the tile kernel reads
                    lay.cwp[(int64_t)(l < Lc ? l : 2 * Lc) * dm.CP + col] = da.p[ig];
                    if (l < Lc) lay.cwp[(int64_t)(Lc + l) * dm.CP + col] = da.p[al.dcb + (int64_t)l * dm.C + col];
                }
            }
        }
    }
}

__global__ __launch_bounds__(256) void k_bn_grads2(const float* __restrict__ W1, const float* __restrict__ gamma,
                                                   const float* __restrict__ beta, DeepFmDims dm, float* accum,
                                                   DeepFmAccum al, const float* __restrict__ wpart, int row_blocks,
                                                   int Lc, const float* __restrict__ cw, const float* __restrict__ cb,
                                                   const float* __restrict__ w3c, RecSrc rs, int col_blocks, GPart gp) {
    // blocks [0, col_blocks): one per column (E'); the blocks behind them: the record entries -> the gradient buffer
    __shared__ floatx2 sm[4][64];
    __shared__ float slin_s[kMaxC];
    const DenseAdam none{nullptr, nullptr, nullptr, 0.f, 0.f, 0.f, 0.f};
    const Part3 pl = part3_layout(dm.CP, Lc, 1);
    if ((int)blockIdx.x < col_blocks)
        bn_grads2_body(W1, gamma, beta, dm, accum, al, wpart, row_blocks, Lc, cw, cb, w3c, rs, pl, sm, slin_s, none, (int)blockIdx.x, gp);
    else
        finish_record_entry(((int)blockIdx.x - col_blocks) * (int)blockDim.x + (int)threadIdx.x, rs, pl, al, dm, Lc, accum, none);
}

// forward-only calls: the record entries (the loss) -> the gradient buffer, and the BN accumulators back to zero for the next
// step's kernel A (a backward step does that in its weight-gradient launch)
__global__ __launch_bounds__(256) void k_finish_records(DeepFmDims dm, float* accum, DeepFmAccum al, int Lc, RecSrc rs,
                                                        double* __restrict__ bnacc_zero, int bnacc_n) {
    const DenseAdam none{nullptr, nullptr, nullptr, 0.f, 0.f, 0.f, 0.f};
    const Part3 pl = part3_layout(dm.CP, Lc, 0);
    const int i = (int)blockIdx.x * (int)blockDim.x + (int)threadIdx.x;
    finish_record_entry(i, rs, pl, al, dm, Lc, accum, none);
    for (int j = i; j < bnacc_n; j += (int)(gridDim.x * blockDim.x)) bnacc_zero[j] = 0.0;
}

// F: the LAST launch of the pipelined step when the optimizer is handed in (dt_deepfm_train_step_adam with the dense
// buffers): kernel E' with the Keras-Adam update of every dense element applied where its gradient is finished, the
// vectors the record reduction finished (db1 .. dbeta) in `small_blocks` further blocks, the segments of the rows looked
// up several times (optim.hip's walk) in the trailing blocks, and the step state advanced by the last block to arrive —
// round 2's E' (6.7 us) and optimizer launch (the dependent chain of the segment walk + the dense tail, 9.6 us) side by
// side in one launch.
struct FinishSeg {
    SegTail seg;
    float *table, *m, *v;
    const float* values;
    int sstride, D;
};
__global__ __launch_bounds__(256) void k_finish_step(const float* __restrict__ W1, const float* __restrict__ gamma,
                                                     const float* __restrict__ beta, DeepFmDims dm, float* accum,
                                                     DeepFmAccum al, const float* __restrict__ wpart, int row_blocks,
                                                     DenseAdam da, AdamState* __restrict__ st, float lr, int col_blocks,
                                                     int small_blocks, int seg_blocks, FinishSeg fs, int Lc,
                                                     const float* __restrict__ cw, const float* __restrict__ cb,
                                                     const float* __restrict__ w3c, RecSrc rs, X3Lay lay, GPart gp,
                                                     const float* __restrict__ lr_snap) {
    __shared__ floatx2 sm[4][64];
    __shared__ float slin_s[kMaxC];
    const Part3 pl = part3_layout(dm.CP, Lc, 1);
    // every thread reads lr_t itself (a uniform scalar load, consumed at the end of its dependency chain) instead of one
    // thread + an LDS broadcast behind a barrier at the block's start — one dependent round trip less per block; the
    // barrier before the arrival ticket guarantees every wave of the block HAS read it when the state may advance
    // block order: segments | small vectors | columns — the segment walk is the launch's longest dependent chain (record ->
    // list + p, m, v -> members' rows -> stores) and starts first
    const int sb = (int)blockIdx.x < seg_blocks ? (int)blockIdx.x : -1;
    const int b = sb >= 0 ? col_blocks + small_blocks : (int)blockIdx.x - seg_blocks < small_blocks
                      ? col_blocks + ((int)blockIdx.x - seg_blocks) : (int)blockIdx.x - seg_blocks - small_blocks;
    int nseg0 = 0;
    if (sb >= 0 && fs.seg.nseg) nseg0 = fs.seg.nseg[(sb * (int)(blockDim.x >> 6) + (int)(threadIdx.x >> 6)) % fs.seg.regions];
    // the step's rate: the copy the weight-gradient launch left (lr_snap), never the state itself — see the end of this kernel
    if (lr_snap) da.lr_t = *lr_snap; else if (st) da.lr_t = st->lr_t;
    if (b < col_blocks) {
        bn_grads2_body(W1, gamma, beta, dm, accum, al, wpart, row_blocks, Lc, cw, cb, w3c, rs, pl, sm, slin_s, da, b, gp, lay);
    } else if (b < col_blocks + small_blocks) {
        // one thread per record entry: db1 | db2 | dw3 (dnn part) | dwo | dbo | loss | dbeta | dgamma — summed over the shards,
        // stored, updated (the d w_lin entries — DCN: the cross kernels / biases — belong to the column blocks above)
        finish_record_entry((b - col_blocks) * (int)blockDim.x + (int)threadIdx.x, rs, pl, al, dm, Lc, accum, da);
    } else if (fs.seg.nseg) {
        adam_segments<true>(fs.seg, seg_blocks, nseg0, fs.table, fs.m, fs.v, fs.values, fs.D, da.lr_t, da.b1, da.b2, da.eps,
                      fs.sstride, sb);
    }
    // The device step state advances HERE.  Rounds 2-5 let the last block to arrive do it (an arrival ticket per block, so
    // that every block had read lr_t from the state before it moved): measured in round 6 (tools/r6/call14.sh, call15.sh) the
    // 2550 tickets of this launch cost 7 us in an otherwise empty launch and 2.2-2.7 us of the step (40 arrivals queue on each
    // of the 64 counters, and a queued returning atomic takes ~350 ns).  With the rate read from lr_snap nobody in this launch
    // reads the state, so one thread may advance it at any time.
    if (lr_snap) {
        if (blockIdx.x == 0 && threadIdx.x == 0 && st) {
            const int t = st->t + 1;
            st->t = t;
            st->lr_t = adam_lr_t(lr, da.b1, da.b2, t);
        }
    } else {
        __syncthreads();
        adam_finish(st, threadIdx.x == 0 ? 0u : kNoTicket, lr, da.b1, da.b2);
    }
}

// advances the dropout seed once per step (after kernel D: every reader of this step's value has finished)
__global__ void k_emb_drop_advance(unsigned* seed) { *seed = *seed * 1664525u + 1013904223u; }

// ---------------------------------------------------------------------------------------------
// Pipelined step, launch E+D: the weight-gradient GEMMs (MFMA-bound) and the row-gradient epilogue + the row-sparse
// Adam update of the rows looked up once (bound by random 64 / 128-byte records) in ONE launch of 512-thread blocks,
// one per CU: waves 0-3 run a heavy block of the weight-gradient GEMMs (wgrad_heavy), waves 4-7 the epilogue of the block's share of the 32-row
// tiles — one matrix wave and one memory wave per SIMD, neither waiting for the other.  With dXn and the two BN
// batch sums already there (kernel C + the record reduction), a lookup's gradient is elementwise:
//   dX[c]            = gamma rstd (dXn - mean_b(dXn) - xhat mean_b(dXn xhat))
//   grad_rows[b,f,d] = dX[b,f*D+d] + dz[b] w_lin[f] + dz[b] (S[b,d] - E[b,f,d])
// and, when the optimizer's slots are handed in (RowsAdam; single process, in-step dedupe on), the Keras-Adam
// read-modify-write of p and [m|v] follows at once for every lookup whose row appears ONCE in the batch
// (rows_out >= 0: known from the election since k_prep); only the members of segments (rows_out == -1) still store
// their gradient row for the optimizer launch to sum.  That removes 13.6 MB written + 13.6 MB re-read and the
// 28.8 us row-update launch from the dependent chain (VERDICT r2 #3 iii).
// Mapping of the memory waves: thread = one 16-byte piece (f, c) of a batch row, 256 / (F D/4) rows in flight per pass,
// so the per-column constants are loaded once per thread and every wave-load covers contiguous 16-byte pieces of a
// row of dXn / X; kRowsUB lookups per thread with all their loads in flight (ids -> streaming operands -> p, m, v).
// ---------------------------------------------------------------------------------------------
struct RowsAdam {
    float *table, *m, *v;        // table == NULL: no in-step update, every lookup stores its gradient row
    int sstride;                 // floats between the slot records of consecutive rows (D: separate m / v arrays; 2 D: [V,2,D])
    const float* lr_t_dev;       // device-resident bias-corrected rate (AdamState), or NULL -> lr_t_host
    float lr_t_host, b1, b2, eps;
};
struct RowsEpi {
    const float *dXn, *X, *dz, *S, *wlin, *sc, *mean, *rstd;
    RecSrc rs;                   // the tile kernel's record shards: sdx / sdxx = the two BN-backward batch sums
    int sdx, sdxx;
    const int64_t* rows_out;
    float* grad_rows;
    float grad_scale;
    int field_major;
};
constexpr int kRowsUB = 4;
constexpr int kRowsStage = 2;        // passes per pipeline stage of the fast body (two stages in flight = kRowsUB passes)

// one stage of the fast body: a chunk of kRowsStage passes with every load of it issued
struct RowsStage {
    int64_t row[kRowsStage];
    floatx4 gx[kRowsStage], xr[kRowsStage], sv[kRowsStage], mv[kRowsStage], vv[kRowsStage];
    float dzv[kRowsStage];
    int bb[kRowsStage];
    bool ok[kRowsStage];
    bool live;                       // the stage's work ticket lies inside the block's share (wave-uniform)
};

// One WAVE's share of the epilogue.  A wave covers the 16-byte pieces of one batch row (F D/4 <= 64: several rows per pass)
// or one half of them (F D/4 in (64, 128]: `parts` = 2, wave w takes half w % 2), so its per-column constants are
// loaded once; work = chunks of kRowsUB passes pulled from an LDS counter per part (`work`), shared by every wave of the
// block that runs this function — the block's memory waves from the start, its matrix waves once their GEMM is stored
// (k_wgrad_rows): with B = 8192 the matrix waves are done after ~28 K of the memory waves' ~69 K cycles.
// FAST: the combination DeepModel.fit runs, fixed at compile time by the launch site — the in-step Adam (ad.table), no
// embedding dropout (drop.thr == 0), row-major gradient rows.  Its loads are unconditional and sit in one basic block per
// stage, and it runs as a two-stage software pipeline over chunks of kRowsStage passes: while a wave does the arithmetic and
// the stores of chunk i, every load of chunk i + 1 (ticket -> ids -> streaming operands -> m, v) is already in flight, and
// each wait for one of them counts only operations issued before the stores of chunk i.  (What is left per stage: the wait
// for the ids of chunk i + 1 also covers the stores of chunk i - 1, issued just before them.  Measured at B = 8192, uniform
// ids: 2 passes per stage 91.4 us per step, 3: 91.7, 4: 92.0; the specialised body without the pipeline 94.4, before 94.7.)
// No read-after-write hazard
// between chunks: a row with rows_out >= 0 occurs once in the batch (the election), segment members only store their own
// gradient row.  (The one exception, an election overflow at B > 8192, is invalid already and flagged by check_dedupe.)
// Every other combination takes the generic body.
template <bool DCN, bool FAST>
__device__ __forceinline__ void rows_epilogue_wave(unsigned* work, int first_tile, int tile_stride, const DeepFmDims& dm,
                                                   const RowsEpi& a, const RowsAdam& ad, const EmbDrop& drop) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int LPR = dm.D >> 2, TPR = dm.F * LPR;           // 16-byte pieces per embedding vector / per batch row (<= 128)
    const int parts = TPR > 64 ? 2 : 1;
    const int lpp = (TPR + parts - 1) / parts;             // lanes a row (or its half) takes
    const int rpw = parts == 1 ? 64 / TPR : 1;             // batch rows per pass of the wave
    const int part = wv & (parts - 1);
    const int rsub = lane / lpp, pl = lane - rsub * lpp;
    const int piece = min(part * lpp + pl, TPR - 1);
    const bool active = rsub < rpw && part * lpp + pl < TPR;
    const int f = piece / LPR, c = piece - f * LPR;
    const int col = 4 * piece;                             // = f * D + 4 c
    const int tiles = (dm.B + kTM - 1) / kTM;
    const int chunk_rows = rpw * (FAST ? kRowsStage : kRowsUB), chunks = (kTM + chunk_rows - 1) / chunk_rows;
    int dshift = 0;
    while ((1 << dshift) < dm.D) ++dshift;
    const floatx4 ca = ld4(a.sc + col), cmu = ld4(a.mean + col);
    // the per-column constants of BatchNormalization's backward, cm1 = mean_b(dXn), cm2 = rstd mean_b(dXn xhat), straight from
    // the shards of the tile kernel's record sums (rounds 3-4: a reduction launch between kernel C and this one wrote them)
    floatx4 c1, c2;
    {
        typedef double doublex2 __attribute__((ext_vector_type(2)));
        doublex2 s1[2] = {{0.0, 0.0}, {0.0, 0.0}}, s2[2] = {{0.0, 0.0}, {0.0, 0.0}};
#pragma unroll
        for (int sh = 0; sh < kRecShards; ++sh) {
            const double* q = a.rs.racc + (int64_t)sh * a.rs.stride;
            s1[0] += *reinterpret_cast<const doublex2*>(q + a.sdx + col);
            s1[1] += *reinterpret_cast<const doublex2*>(q + a.sdx + col + 2);
            s2[0] += *reinterpret_cast<const doublex2*>(q + a.sdxx + col);
            s2[1] += *reinterpret_cast<const doublex2*>(q + a.sdxx + col + 2);
        }
        const floatx4 rsd = ld4(a.rstd + col);
        const float invN = 1.0f / (float)dm.B;
        c1 = floatx4{(float)s1[0][0], (float)s1[0][1], (float)s1[1][0], (float)s1[1][1]} * invN;
        c2 = rsd * floatx4{(float)s2[0][0], (float)s2[0][1], (float)s2[1][0], (float)s2[1][1]} * invN;
    }
    const float wl = DCN ? 0.f : a.wlin[f];
    const float lr_t = ad.lr_t_dev ? *ad.lr_t_dev : ad.lr_t_host;
    if constexpr (FAST) {
        // pulls the next work ticket and issues every load of its chunk, all from clamped (valid) addresses — also for a
        // ticket past the end (live = false), whose results the wave discards before it leaves
        auto fetch = [&](RowsStage& s) {
            unsigned it = 0;
            if (lane == 0) it = atomicAdd(&work[part], 1u);
            it = __builtin_amdgcn_readfirstlane(it);
            const int ti = (int)(it / (unsigned)chunks), ch = (int)(it - (unsigned)ti * (unsigned)chunks);
            const int tile = first_tile + ti * tile_stride;
            s.live = tile < tiles;
            const int b0 = min(tile, tiles) * kTM;
#pragma unroll
            for (int k = 0; k < kRowsStage; ++k) {
                const int r = ch * chunk_rows + k * rpw + rsub;
                s.ok[k] = s.live && active && r < kTM && b0 + r < dm.B;
                s.bb[k] = min(b0 + min(r, kTM - 1), dm.B - 1);
                s.row[k] = a.rows_out[(int64_t)s.bb[k] * dm.F + f];
            }
#pragma unroll
            for (int k = 0; k < kRowsStage; ++k) {
                s.gx[k] = ld4(a.dXn + (int64_t)s.bb[k] * dm.CP + col);
                s.xr[k] = ld4(a.X + (int64_t)s.bb[k] * dm.CP + col);
                if (!DCN) {
                    s.sv[k] = ld4(a.S + ((int64_t)s.bb[k] << dshift) + 4 * c);
                    s.dzv[k] = a.dz[s.bb[k]];
                }
            }
#pragma unroll
            for (int k = 0; k < kRowsStage; ++k) {
                const int64_t rr = (s.ok[k] && s.row[k] >= 0) ? s.row[k] : 0;
                s.mv[k] = ld4(ad.m + rr * ad.sstride + 4 * c);
                s.vv[k] = ld4(ad.v + rr * ad.sstride + 4 * c);
            }
        };
        // the arithmetic and the stores of a fetched chunk; p is the X tile's copy of the table row (see the generic body).
        // Only the stores are divergent.
        auto finish = [&](const RowsStage& s) {
#pragma unroll
            for (int k = 0; k < kRowsStage; ++k) {
                floatx4 g = ca * (s.gx[k] - c1 - (s.xr[k] - cmu) * c2);
                if (!DCN) g = g + s.dzv[k] * wl + s.dzv[k] * (s.sv[k] - s.xr[k]);
                // Keras Adam (optim.hip): m, v, p of this 16-byte piece of the row
                floatx4 mi = s.mv[k], vi = s.vv[k], pi = s.xr[k];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    mi[e] = ad.b1 * mi[e] + (1.f - ad.b1) * g[e];
                    vi[e] = ad.b2 * vi[e] + (1.f - ad.b2) * g[e] * g[e];
                    pi[e] -= lr_t * mi[e] / (sqrtf(vi[e]) + ad.eps);
                }
                if (s.ok[k] && s.row[k] >= 0) {
                    st4(ad.m + s.row[k] * ad.sstride + 4 * c, mi);
                    st4(ad.v + s.row[k] * ad.sstride + 4 * c, vi);
                    st4(ad.table + (s.row[k] << dshift) + 4 * c, pi);
                } else if (s.ok[k]) {                      // segment members: the lookup's own gradient row
                    st4(a.grad_rows + (((int64_t)s.bb[k] * dm.F + f) << dshift) + 4 * c, g);
                }
            }
        };
        // two stages, unrolled by hand so that no stage's registers are copied (a copy would wait for the loads it moves)
        RowsStage s0, s1;
        fetch(s0);
        for (;;) {
            if (!s0.live) break;
            fetch(s1);
            finish(s0);
            if (!s1.live) break;
            fetch(s0);
            finish(s1);
        }
        return;
    }
    const unsigned dseed = drop.thr ? *drop.seed : 0u;
    for (;;) {
        unsigned it = 0;
        if (lane == 0) it = atomicAdd(&work[part], 1u);
        it = __builtin_amdgcn_readfirstlane(it);
        const int ti = (int)(it / (unsigned)chunks), ch = (int)(it - (unsigned)ti * (unsigned)chunks);
        const int tile = first_tile + ti * tile_stride;
        if (tile >= tiles) break;
        const int b0 = tile * kTM;
        {
            int64_t row[kRowsUB];
            floatx4 gx[kRowsUB], xr[kRowsUB], sv[kRowsUB];
            float dzv[kRowsUB];
            bool ok[kRowsUB];
            int bb[kRowsUB];
            // every load is unconditional from a clamped (valid) address; the results of lanes that are not `ok` are unused
#pragma unroll
            for (int k = 0; k < kRowsUB; ++k) {
                const int r = ch * chunk_rows + k * rpw + rsub;
                ok[k] = active && r < kTM && b0 + r < dm.B;
                bb[k] = min(b0 + min(r, kTM - 1), dm.B - 1);
                row[k] = a.rows_out[(int64_t)bb[k] * dm.F + f];
            }
#pragma unroll
            for (int k = 0; k < kRowsUB; ++k) {
                gx[k] = ld4(a.dXn + (int64_t)bb[k] * dm.CP + col);
                xr[k] = ld4(a.X + (int64_t)bb[k] * dm.CP + col);
                if (!DCN) {
                    sv[k] = ld4(a.S + ((int64_t)bb[k] << dshift) + 4 * c);
                    dzv[k] = a.dz[bb[k]];
                }
            }
            floatx4 pv[kRowsUB], mv[kRowsUB], vv[kRowsUB];
            bool upd[kRowsUB];
#pragma unroll
            for (int k = 0; k < kRowsUB; ++k) {
                upd[k] = ok[k] && ad.table && row[k] >= 0;
                if (ad.table) {
                    const int64_t rr = upd[k] ? row[k] : 0;
                    // without embedding dropout the X tile holds the looked-up table rows bit for bit (kernel A copied them,
                    // nothing has written the table since): p needs no second random read — 5 random accesses per row, not 6
                    pv[k] = drop.thr ? ld4(ad.table + (rr << dshift) + 4 * c) : xr[k];
                    mv[k] = ld4(ad.m + rr * ad.sstride + 4 * c);
                    vv[k] = ld4(ad.v + rr * ad.sstride + 4 * c);
                }
            }
#pragma unroll
            for (int k = 0; k < kRowsUB; ++k) {
                floatx4 g = ca * (gx[k] - c1 - (xr[k] - cmu) * c2);
                if (!DCN) g = g + dzv[k] * wl + dzv[k] * (sv[k] - xr[k]);
                if (drop.thr) {          // gradient through the dropped embedding: the same keep-mask as the forward
                    float4 t4 = make_float4(g.x, g.y, g.z, g.w);
                    t4 = emb_drop4(t4, dseed, drop.thr, drop.inv_keep, (unsigned)bb[k], (unsigned)col);
                    g = floatx4{t4.x, t4.y, t4.z, t4.w};
                }
                if (upd[k]) {            // Keras Adam (optim.hip): m, v, p of this 16-byte piece of the row
                    floatx4 mi = mv[k], vi = vv[k], pi = pv[k];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        mi[e] = ad.b1 * mi[e] + (1.f - ad.b1) * g[e];
                        vi[e] = ad.b2 * vi[e] + (1.f - ad.b2) * g[e] * g[e];
                        pi[e] -= lr_t * mi[e] / (sqrtf(vi[e]) + ad.eps);
                    }
                    st4(ad.m + row[k] * ad.sstride + 4 * c, mi);
                    st4(ad.v + row[k] * ad.sstride + 4 * c, vi);
                    st4(ad.table + (row[k] << dshift) + 4 * c, pi);
                } else if (ok[k]) {
                    if (a.field_major)   // model-parallel tables: [F,B,D], already divided by the world size
                        st4(a.grad_rows + (((int64_t)f * dm.B + bb[k]) << dshift) + 4 * c, g * a.grad_scale);
                    else                 // segment members (and, without RowsAdam, every lookup): the lookup's own row
                        st4(a.grad_rows + (((int64_t)bb[k] * dm.F + f) << dshift) + 4 * c, g);
                }
            }
        }
    }
}

// WM: the weight-gradient GEMMs on fp32 MFMA (0), plain bf16 (1) or split-bf16 (2: wgrad_heavy_bf16); FAST: the row epilogue's
// specialised body (rows_epilogue_wave)
template <bool DCN, int WM = 0, bool FAST = false>
__global__ __launch_bounds__(512) void k_wgrad_rows(const float* __restrict__ X, MlpParams p, DeepFmDims dm,
                                                    const float* __restrict__ H1, const float* __restrict__ dH1,
                                                    const float* __restrict__ dH2, int row_blocks, int rows_per_block,
                                                    float* __restrict__ wpart, unsigned long long* stamps_all,
                                                    RowsEpi ep, RowsAdam ad, EmbDrop drop,
                                                    unsigned long long* stamps_rows, int matrix_waves_join,
                                                    double* __restrict__ bnacc_zero, int bnacc_n, StepNext nx, GPart gp,
                                                    float* __restrict__ lr_snap) {
    extern __shared__ __attribute__((aligned(16))) float red[];       // [4][64*128]: the matrix waves' partial macro tiles
    __shared__ unsigned arrived, work[2], ecnt;
    if (threadIdx.x == 0) { arrived = 0u; work[0] = 0u; work[1] = 0u; ecnt = 0u; }
    __syncthreads();          // the only hardware barrier: the two halves never wait for each other afterwards
    if (threadIdx.x < 256) {
        if constexpr (WM == 0)
            wgrad_heavy(red, (int)blockIdx.x, X, p, dm, H1, dH1, dH2, row_blocks, rows_per_block, wpart, stamps_all, &arrived);
        else
            wgrad_heavy_bf16<WM>(red, (int)blockIdx.x, X, p, dm, H1, dH1, dH2, row_blocks, rows_per_block, wpart, &arrived);
        ElectSync sy{&ecnt, 0u};
        if (DCN && gp.part) reduce_gpart(gp, red, (int)blockIdx.x, (int)gridDim.x, (int)threadIdx.x, sy);
        if (nx.idx) {
            // chained steps: the NEXT step's election (ids only: kernel A of this step packed its rows) on the four matrix
            // waves, in the 64 KB of LDS their partial tiles just left — a launch of its own costs 9 us of the step's chain
            // (k_prep), here it takes time the matrix waves would have spent helping with the row epilogue
            for (int e = (int)blockIdx.x; e < nx.eblocks; e += (int)gridDim.x) {
                elect_barrier<256, true>(sy);                     // every wave is done with the LDS (partial tiles / the table before)
                elect_block<256, true, 32>(reinterpret_cast<unsigned long long*>(red), nx.dd, dm.B, dm.F, e, (int)threadIdx.x,
                                           nx.rows_out, sy);
            }
        }
        // the GEMM's partial tile is stored: the matrix waves take their share of what is left of the epilogue
        if (matrix_waves_join) rows_epilogue_wave<DCN, FAST>(work, (int)blockIdx.x, (int)gridDim.x, dm, ep, ad, drop);
        if (stamps_all && threadIdx.x == 0) stamps_all[(int64_t)blockIdx.x * 16 + 6] = __builtin_amdgcn_s_memtime();
    } else {
        if (stamps_rows && threadIdx.x == 256) stamps_rows[(int64_t)blockIdx.x * 16] = __builtin_amdgcn_s_memtime();
        // kernel C (the only reader of this step's BN batch sums) is done: the accumulators go back to zero for the next kernel A
        for (int j = (int)blockIdx.x * 256 + ((int)threadIdx.x - 256); j < bnacc_n; j += (int)gridDim.x * 256) bnacc_zero[j] = 0.0;
        // the finishing launch reads the step's rate from this copy, so that ONE of its threads may advance the device state
        // at any time (see k_finish_step: no arrival tickets)
        if (lr_snap && blockIdx.x == 0 && threadIdx.x == 256) *lr_snap = ad.lr_t_dev ? *ad.lr_t_dev : ad.lr_t_host;
        rows_epilogue_wave<DCN, FAST>(work, (int)blockIdx.x, (int)gridDim.x, dm, ep, ad, drop);
        if (stamps_rows && threadIdx.x == 256) stamps_rows[(int64_t)blockIdx.x * 16 + 3] = __builtin_amdgcn_s_memtime();
    }
}

}  // namespace dt

using namespace dt;

extern "C" int dt_deepfm_supported(int B, int F, int D, int Nd, int H1, int H2) {
    DeepFmDims dm; int lpr;
    return (H1 == kH1 && H2 == kH2 && deepfm_dims(B, F, D, Nd, &dm, &lpr)) ? 1 : 0;
}

// workspace layout (floats)
struct DeepFmWs {
    int64_t X, H1, dH1, dH2, lin, fm, z, dz, dlogit, mean, rstd, sc, betap, W1L, W2L, W2TL, S, wpart, bnacc, racc, stamps, dXc, dXn,
        gammap, x3, total;
    int64_t bnacc_n, racc_n;          // doubles
    int64_t gpart, gsum;
    int64_t lrsnap;                   // the step's bias-corrected rate, copied by the weight-gradient launch for the finishing one
};
static DeepFmWs deepfm_ws_layout(const DeepFmDims& dm, int L = 0) {     // L > 0: DCN with L cross layers
    DeepFmWs w;
    int64_t o = 0;
    auto take = [&](int64_t n) { int64_t r = o; o += (n + 3) & ~(int64_t)3; return r; };
    const int tiles = ceil_div(dm.B, kTM);
    const int64_t rows = (int64_t)tiles * kTM;
    w.X = take(rows * dm.CP);
    w.H1 = take(rows * kH1);
    w.dH1 = take(rows * kH1);
    w.dH2 = take(rows * kH2);
    w.lin = take(rows); w.fm = take(rows); w.z = take(rows); w.dz = take(rows); w.dlogit = take(rows);
    w.mean = take(dm.CP); w.rstd = take(dm.CP); w.sc = take(dm.CP); w.betap = take(dm.CP);
    w.W1L = take((int64_t)dm.CP * kH1);
    w.W2L = take((int64_t)kH1 * kH2);
    w.W2TL = take((int64_t)kH1 * kH2);
    w.S = take(rows * dm.D);                        // S[b][d] = sum_f E[b,f,d] (kernel A -> kernel D)
    w.wpart = take((int64_t)256 * 8192);            // wgrad_heavy's per-slice partial macro tiles (<= 256 heavy blocks)
    // the batch-sum accumulators (doubles; see bnacc / racc in front of kernel A): zero before the first step, kept by the steps
    w.bnacc_n = (int64_t)kBnShards * 2 * dm.CP;
    w.bnacc = take(2 * w.bnacc_n);
    w.racc_n = (int64_t)kRecShards * part3_layout(dm.CP, L, 1).stride;
    w.racc = take(2 * w.racc_n);
    w.gpart = take(L > 0 ? (int64_t)tiles * (L + 1) * dm.CP : 0);      // DCN: per-tile cross vectors G_0 .. G_L (DcnArgs.gpart)
    w.gsum = take(L > 0 ? (int64_t)(L + 1) * dm.CP : 0);               // ... and their sums over the tiles
    w.stamps = take((int64_t)5 * tiles * 16 * 2);   // u64 [3 tile kernels][tiles][16] + kernel A [2 * tiles][16]
    w.dXc = take(L > 0 ? rows * dm.CP : 0);         // DCN: d loss / d Xn through the cross network (kernel C -> kernel D)
    w.dXn = take(rows * dm.CP);                     // pipelined step: dXn = dH1 . W1^T [+ the cross term] (kernel C -> the row-gradient epilogue)
    w.gammap = take(dm.CP);
    w.lrsnap = take(4);
    // split-bf16 tower: W1B (3 bf16 parts of CP x 128) | W1R (2 parts) | W2B (3 parts of 128 x 64) | W2R (2 parts)
    w.x3 = take((5 * (int64_t)dm.CP * kH1 + 5 * (int64_t)kH1 * kH2 + 1) / 2 + (2 * kCrossMax + 1) * (int64_t)dm.CP);
    w.total = o;
    return w;
}

extern "C" int64_t dt_deepfm_workspace_bytes(int B, int F, int D, int Nd) {
    DeepFmDims dm; int lpr;
    if (!deepfm_dims(B, F, D, Nd, &dm, &lpr)) return -1;
    return deepfm_ws_layout(dm).total * (int64_t)sizeof(float);
}

extern "C" int64_t dt_deepfm_stamps_offset_floats(int B, int F, int D, int Nd) {
    DeepFmDims dm; int lpr;
    if (!deepfm_dims(B, F, D, Nd, &dm, &lpr)) return -1;
    return deepfm_ws_layout(dm).stamps;
}

extern "C" int64_t dt_deepfm_accum_floats(int F, int D, int Nd) {
    const int C = F * D + Nd, CP = (C + 63) & ~63;
    return deepfm_accum_layout(C, CP, F, Nd).total;
}

// offsets (in floats) of each gradient inside the accumulator buffer, in the order:
// dW1, dW2, db1, db2, dw3, dwo, dbo, loss, dgamma, dbeta, dwlin
extern "C" int dt_deepfm_accum_offsets(int F, int D, int Nd, int64_t* out11) {
    const int C = F * D + Nd, CP = (C + 63) & ~63;
    const DeepFmAccum a = deepfm_accum_layout(C, CP, F, Nd);
    const int64_t v[11] = {a.dW1, a.dW2, a.db1, a.db2, a.dw3, a.dwo, a.dbo, a.loss, a.dgamma, a.dbeta, a.dwlin};
    for (int i = 0; i < 11; ++i) out11[i] = v[i];
    return DT_OK;
}

extern "C" unsigned dt_deepfm_dropout_hash(unsigned seed, unsigned b, unsigned col) { return emb_drop_hash(seed, b, col); }

extern "C" int64_t dt_deepfm_dedupe_slots(int B, int F) {
    return (int64_t)B * F;          // lookups per step (the value dt_*_train_step expects as dedupe_slots)
}

// byte offsets inside dedupe_ws: rows_fm | nseg | seg_row | seg_off | seg_cnt | seg_list | total
struct DedupeLayout {
    int64_t rows_fm, nseg, seg_row, seg_off, seg_cnt, seg_list, list_cur, overflow, pid, total;
    int pid_stride;
    int eblocks, parts_log2;
    int regions, cap;            // what a consumer of the segments walks: `regions` regions of up to `cap` segments, nseg[region]
    bool by_field;               // B > kElectSlots: regions = fields (padded to 8), filled through cursors (nseg = the segment cursors)
};
static DedupeLayout dedupe_layout(int B, int F) {
    const int64_t n = (int64_t)B * F;
    DedupeLayout l;
    l.by_field = B > kElectSlots;
    l.parts_log2 = 0;
    // ~1024 lookups per election block up to B = 8192 (the launch's chain is the block's); beyond: ~4096 (half of the table's
    // slots — the scan of the partition bytes is per block)
    while (((l.by_field ? 4096 : 1024) << l.parts_log2) < B) ++l.parts_log2;
    const int fpad = ((F + 7) >> 3) << 3;                    // fields padded to 8 (XCD-aware ids)
    l.eblocks = fpad << l.parts_log2;
    l.regions = l.by_field ? fpad : l.eblocks;
    l.cap = l.by_field ? (B >> 1) : kSegCap;
    int64_t o = 0;
    auto take = [&](int64_t bytes) { int64_t r = o; o += (bytes + 15) & ~(int64_t)15; return r; };
    l.rows_fm = take(n * 8); l.nseg = take((int64_t)l.regions * 4);
    l.seg_row = take((int64_t)l.regions * l.cap * 8); l.seg_off = take((int64_t)l.regions * l.cap * 4);
    l.seg_cnt = take((int64_t)l.regions * l.cap * 4); l.seg_list = take((int64_t)l.regions * B * 4);
    l.list_cur = take((int64_t)fpad * 4);
    l.overflow = take(16);
    l.pid_stride = (B + 15) & ~15;
    l.pid = take(l.by_field ? (int64_t)fpad * l.pid_stride : 0);
    l.total = o;
    return l;
}
// the device view of a dedupe workspace
static DedupeWs dedupe_view(void* dedupe_ws, const DedupeLayout& dl) {
    char* base = reinterpret_cast<char*>(dedupe_ws);
    DedupeWs dd{reinterpret_cast<int64_t*>(base + dl.rows_fm), dl.parts_log2, reinterpret_cast<int*>(base + dl.nseg),
                reinterpret_cast<int64_t*>(base + dl.seg_row), reinterpret_cast<int*>(base + dl.seg_off),
                reinterpret_cast<int*>(base + dl.seg_cnt), reinterpret_cast<int*>(base + dl.seg_list),
                dl.by_field ? reinterpret_cast<int*>(base + dl.nseg) : nullptr,
                dl.by_field ? reinterpret_cast<int*>(base + dl.list_cur) : nullptr,
                reinterpret_cast<int*>(base + dl.overflow),
                dl.by_field ? reinterpret_cast<unsigned char*>(base + dl.pid) : nullptr, dl.pid_stride};
    return dd;
}

extern "C" int64_t dt_deepfm_dedupe_bytes(int B, int F) { return dedupe_layout(B, F).total; }

// what the optimizer consumes (dt_adam_rows_step_seg): byte offsets of nseg (int32 [regions]), seg_row (int64
// [regions][cap]), seg_off, seg_cnt (int32 [regions][cap]), seg_list (int32), then regions and cap
extern "C" int dt_deepfm_dedupe_segments(int B, int F, int64_t* out7) {
    const DedupeLayout l = dedupe_layout(B, F);
    out7[0] = l.nseg; out7[1] = l.seg_row; out7[2] = l.seg_off; out7[3] = l.seg_cnt; out7[4] = l.seg_list;
    out7[5] = l.regions; out7[6] = l.cap;
    return DT_OK;
}

// byte offset of the overflow counter inside dedupe_ws (int32; zero-filled with the workspace): lookups that found their
// election table full — possible only for B > 8192 with pathologically colliding ids; non-zero = that step's duplicate
// handling was incomplete (fused.FusedDeepFM.check_dedupe raises)
extern "C" int64_t dt_deepfm_dedupe_overflow_offset(int B, int F) { return dedupe_layout(B, F).overflow; }

// The ids-only half of a step's in-step dedupe, run AHEAD of the step (another stream, an earlier point of a captured graph):
// rows_out [B][F] <- the packed table row of every lookup (-1: id out of range, or a member of a segment), dedupe_ws <- the
// segments.  The step itself then runs with phases | DT_STEP_PREELECTED on the same idx / rows_out / dedupe_ws.
extern "C" int dt_deepfm_preelect(const void* idx, int idx_kind, const int64_t* row_offset, const int32_t* vocab, int B,
                                  int F, int64_t* rows_out, void* dedupe_ws, int64_t dedupe_slots, void* stream) {
    DT_REQUIRE(idx && row_offset && vocab && rows_out && dedupe_ws && B > 0 && F > 0 && F <= 128,
               "dt_deepfm_preelect: bad arguments");
    DT_REQUIRE(idx_kind == DT_IDX_F32 || idx_kind == DT_IDX_I32, "dt_deepfm_preelect: idx_kind %d", idx_kind);
    DT_REQUIRE(dedupe_slots == (int64_t)B * F, "dt_deepfm_preelect: dedupe_slots=%lld must be dt_deepfm_dedupe_slots(B, F)",
               (long long)dedupe_slots);
    DT_UNSUPPORTED((int64_t)B * F >= (1LL << 23), "dt_deepfm_preelect: the in-step dedupe takes up to 2^23 lookups (B=%d, F=%d)", B, F);
    DT_REQUIRE((uintptr_t)dedupe_ws % 16 == 0, "dt_deepfm_preelect: dedupe_ws must be 16-byte aligned");
    hipStream_t st = as_stream(stream);
    const DedupeLayout dl = dedupe_layout(B, F);
    const DedupeWs dd = dedupe_view(dedupe_ws, dl);
    DeepFmDims dm{B, F, 0, 0, 0, 0};
    if (idx_kind == DT_IDX_F32)
        hipLaunchKernelGGL(k_rows_of_ids<DT_IDX_F32>, dim3(ceil_div(B, 64)), dim3(256), 0, st, idx, row_offset, vocab, dm, rows_out,
                           dd.rows_fm, dd.seg_cur, dd.list_cur, dd.pid_fm, dd.pid_stride, dd.parts_log2);
    else
        hipLaunchKernelGGL(k_rows_of_ids<DT_IDX_I32>, dim3(ceil_div(B, 64)), dim3(256), 0, st, idx, row_offset, vocab, dm, rows_out,
                           dd.rows_fm, dd.seg_cur, dd.list_cur, dd.pid_fm, dd.pid_stride, dd.parts_log2);
    const size_t ldsB = dl.by_field ? kElectLdsBig : kElectLds;
    hipFuncSetAttribute((const void*)k_elect, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsB);
    hipLaunchKernelGGL(k_elect, dim3(dl.eblocks), dim3(1024), ldsB, st, dd, dm, rows_out);
    return launch_status("dt_deepfm_preelect");
}

// dt_deepfm_train_step_adam with the optimizer's dense half as well: the flat parameter / slot buffers (laid out like accum),
// the step state to advance and the base learning rate
struct StepDense {
    float *p, *m, *v;
    int64_t n_flat;
    void* state;
    float lr;
};

// chained steps (see StepNext): the next step's ids and the buffers its election fills
struct StepChain {
    const void* next_idx;
    int64_t* next_rows_out;
    void* next_dedupe_ws;
};
// a step of this shape / these phases can be chained (prepare its successor, run prepared): the in-step optimizer on the
// split-bf16 tile kernel, a batch the register-resident election takes
static bool step_chains(const DeepFmDims& dm, int phases, bool with_dense, bool with_dedupe) {
    const bool x3_flag = (phases & (DT_STEP_TOWER_X3 | DT_STEP_TOWER_BF16)) != 0;
    return (phases & 0xf) == 2 && !(phases & (DT_STEP_SKIP_FINISH | DT_STEP_FINISH_ONLY)) && x3_flag && dm.CP <= 512 &&
           x3_fits(dm.CP) && with_dense && with_dedupe && dm.B <= kElectSlots && (int64_t)dm.B * dm.F < (1LL << 23);
}

// 1 when dt_deepfm_train_step_adam / dt_dcn_train_step_adam with these phases (and dense_n > 0, dedupe_ws) can prepare its
// successor (next_idx) and run prepared (DT_STEP_PREPARED)
extern "C" int dt_deepfm_step_chains(int B, int F, int D, int Nd, int phases) {
    DeepFmDims dm; int lpr;
    if (!deepfm_dims(B, F, D, Nd, &dm, &lpr)) return 0;
    return step_chains(dm, phases, true, true) ? 1 : 0;
}

// ---- launch-boundary trace of an EAGER step (bench.py's per-kernel split; never enabled inside a stream capture) ----
// dt_step_trace(1): every fused train step this thread enqueues afterwards records a HIP event on its stream in front of
// its first launch and behind each of its launch groups (A [+ the prep launch] | C | E||D | F); dt_step_trace_read waits
// for the last traced step and returns the four intervals, averaged over the (up to 32) steps traced since the switch was
// set.  Events belong to the thread (created on first use).
namespace {
constexpr int kTraceEvents = 5, kTraceSteps = 32;
thread_local bool g_trace_on = false;
thread_local int g_trace_step = -1;                       // steps traced since dt_step_trace(1) - 1
thread_local int g_trace_have[kTraceSteps];               // boundaries recorded of the step in each ring entry
thread_local hipEvent_t g_trace_ev[kTraceSteps][kTraceEvents];
thread_local bool g_trace_init = false;
inline void trace_mark(int i, hipStream_t st) {
    if (!g_trace_on) return;
    if (!g_trace_init) {
        for (int s = 0; s < kTraceSteps; ++s) {
            g_trace_have[s] = 0;
            for (int e = 0; e < kTraceEvents; ++e) g_trace_ev[s][e] = nullptr;
        }
        g_trace_init = true;
    }
    if (i == 0) { ++g_trace_step; g_trace_have[g_trace_step % kTraceSteps] = 0; }
    if (g_trace_step < 0) return;
    const int s = g_trace_step % kTraceSteps;
    if (g_trace_have[s] != i) return;                     // a step shape without this boundary: the entry stays incomplete
    if (!g_trace_ev[s][i]) hipEventCreate(&g_trace_ev[s][i]);
    hipEventRecord(g_trace_ev[s][i], st);
    g_trace_have[s] = i + 1;
}
}  // namespace

extern "C" int dt_step_trace(int enable) {
    g_trace_on = enable != 0;
    g_trace_step = -1;
    if (g_trace_init) for (int s = 0; s < kTraceSteps; ++s) g_trace_have[s] = 0;
    return DT_OK;
}

extern "C" int dt_step_trace_read(float* us_host, int n, int* steps_host) {
    DT_REQUIRE(us_host && n >= kTraceEvents - 1, "dt_step_trace_read: us_host must take %d floats", kTraceEvents - 1);
    double sum[kTraceEvents - 1] = {0, 0, 0, 0};
    int steps = 0;
    if (g_trace_init && g_trace_step >= 0) {
        const int last = g_trace_step % kTraceSteps;
        if (g_trace_have[last] == kTraceEvents && hipEventSynchronize(g_trace_ev[last][kTraceEvents - 1]) != hipSuccess) {
            dt::set_error("dt_step_trace_read: hipEventSynchronize failed");
            return DT_ERR_LAUNCH;
        }
        for (int s = 0; s < kTraceSteps; ++s) {
            if (g_trace_have[s] != kTraceEvents) continue;
            bool ok = true;
            float ms[kTraceEvents - 1];
            for (int i = 0; i + 1 < kTraceEvents && ok; ++i)
                ok = hipEventElapsedTime(&ms[i], g_trace_ev[s][i], g_trace_ev[s][i + 1]) == hipSuccess;
            if (!ok) continue;                            // (an entry whose step has not finished: only older than `last`)
            for (int i = 0; i + 1 < kTraceEvents; ++i) sum[i] += ms[i] * 1e3;
            ++steps;
        }
    }
    DT_REQUIRE(steps > 0, "dt_step_trace_read: no traced step with the in-step optimizer on this thread "
               "(dt_step_trace(1), then dt_deepfm_train_step_adam / dt_dcn_train_step_adam)");
    for (int i = 0; i + 1 < kTraceEvents; ++i) us_host[i] = (float)(sum[i] / steps);
    if (steps_host) *steps_host = steps;
    return DT_OK;
}

// the step both entry points run: DeepFM (cross == NULL) or DCN (cross kernels / biases [Lc][C]; w3 = the [C + 64] kernel
// applied to Concatenate([cross, dnn]), w_lin unused)
static int tower_train_step(
    const void* idx, int idx_kind, const float* table, const int64_t* row_offset, const int32_t* vocab,
    const float* dense, const float* y, int B, int F, int D, int Nd,
    const float* w_lin, const float* bn_gamma, const float* bn_beta, float* bn_moving_mean,
    float* bn_moving_var, float bn_eps, float bn_momentum, const float* W1, const float* b1, const float* W2,
    const float* b2, const float* w3, const float* w_out, const float* b_out,
    float* logit_out, int64_t* rows_out, float* grad_rows, float* accum, void* workspace, int* oob_count,
    void* dedupe_ws, int64_t dedupe_slots, float grad_rows_scale, int grad_rows_field_major, int phases,
    float embedding_dropout, unsigned* dropout_seed, float dense_input_dropout,
    const float* sample_weight, void* stream, const float* cross_w, const float* cross_b, int Lc,
    const RowsAdam* adam = nullptr, const StepDense* sdense = nullptr, const StepChain* chain = nullptr) {
    DeepFmDims dm; int lpr;
    DT_UNSUPPORTED(!deepfm_dims(B, F, D, Nd, &dm, &lpr), "dt_deepfm_train_step: unsupported shape B=%d F=%d D=%d Nd=%d",
                   B, F, D, Nd);
    const bool dcn = Lc > 0;
    DT_REQUIRE(idx && table && row_offset && vocab && y && (dcn || w_lin) && bn_gamma && bn_beta && W1 && b1 && W2 && b2 &&
                   w3 && w_out && logit_out && rows_out && grad_rows && accum && workspace,
               "dt_deepfm_train_step: null pointer");
    DT_REQUIRE(Nd == 0 || dense, "dt_deepfm_train_step: dense is null");
    DT_REQUIRE(idx_kind == DT_IDX_F32 || idx_kind == DT_IDX_I32, "dt_deepfm_train_step: idx_kind %d", idx_kind);
    hipStream_t st = as_stream(stream);
    const DeepFmWs wl = deepfm_ws_layout(dm, Lc);
    const DeepFmAccum al = deepfm_accum_layout(dm.C, dm.CP, F, Nd, Lc);
    float* ws = reinterpret_cast<float*>(workspace);
    const int mse = (phases & DT_STEP_LOSS_MSE) ? 1 : 0;
    // DT_STEP_SKIP_FINISH / DT_STEP_FINISH_ONLY: the pipelined backward step without / as only its last launch (E': the dense
    // gradients' last level), so that a caller whose row gradients leave through a collective (row-owned tables) can start
    // that collective behind the row-gradient launch and let E' run beside it
    const bool skip_finish = (phases & DT_STEP_SKIP_FINISH) != 0, finish_only = (phases & DT_STEP_FINISH_ONLY) != 0;
    const bool bf16_flag = (phases & DT_STEP_TOWER_BF16) != 0;       // plain bf16: the split kernel with the leading products only
    const bool x3_flag = (phases & DT_STEP_TOWER_X3) != 0 || bf16_flag;
    const bool prepared = (phases & DT_STEP_PREPARED) != 0;      // election + weight layouts done by the previous step's launches
    const bool preelected = (phases & DT_STEP_PREELECTED) != 0 || prepared;
    const int phases_all = phases;
    const bool stamps_flag = (phases & DT_STEP_STAMPS) != 0;
    phases &= 0xf;
    DT_REQUIRE(!(skip_finish && finish_only), "dt_deepfm_train_step: DT_STEP_SKIP_FINISH and DT_STEP_FINISH_ONLY together");
    const DcnArgs dca{cross_w, cross_b, w3, Lc, ws + wl.dXc, mse, 0, sample_weight, ws + wl.gpart, (Lc + 1) * dm.CP};
    const GPart gpt{dcn ? ws + wl.gpart : nullptr, (Lc + 1) * dm.CP, ceil_div(B, kTM), ws + wl.gsum};
    MlpParams mp{b1, W2, b2, dcn ? w3 + dm.C : w3, w_out, b_out, bn_gamma, ws + wl.mean, ws + wl.rstd, ws + wl.sc, ws + wl.betap,
                 W1, ws + wl.W1L, ws + wl.W2L, ws + wl.W2TL,
                 reinterpret_cast<const double*>(ws + wl.bnacc), bn_beta, bn_eps, bn_momentum, bn_moving_mean, bn_moving_var,
                 ws + wl.mean, ws + wl.rstd, ws + wl.sc, ws + wl.betap, ws + wl.gammap};
    DT_REQUIRE(((uintptr_t)W1 | (uintptr_t)W2 | (uintptr_t)(dcn ? W2 : w3) | (uintptr_t)accum) % 16 == 0,
               "dt_deepfm_train_step: W1 / W2 / w3 / accum must be 16-byte aligned");
    const int tiles = ceil_div(B, kTM);
    DedupeWs dd{nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr};
    DT_REQUIRE(!(dedupe_ws && grad_rows_field_major), "dt_deepfm_train_step: dedupe and field-major row gradients "
                                                      "are mutually exclusive");
    if (dedupe_ws && phases >= 2) {          // forward-only calls have no sparse gradient to dedupe
        DT_REQUIRE(dedupe_slots == (int64_t)B * F, "dt_deepfm_train_step: dedupe_slots=%lld must be "
                   "dt_deepfm_dedupe_slots(B, F)", (long long)dedupe_slots);
        DT_UNSUPPORTED((int64_t)B * F >= (1LL << 23), "dt_deepfm_train_step: the in-step dedupe takes up to 2^23 lookups (B=%d, F=%d)",
                       B, F);
        DT_REQUIRE((uintptr_t)dedupe_ws % 16 == 0, "dt_deepfm_train_step: dedupe_ws must be 16-byte aligned");
        dd = dedupe_view(dedupe_ws, dedupe_layout(B, F));
    }
    DT_REQUIRE(!preelected || (dd.rows_fm && !grad_rows_field_major),
               "dt_deepfm_train_step: DT_STEP_PREELECTED needs a backward step with dedupe_ws (filled by dt_deepfm_preelect)");
    if (B % kTM) {       // ragged last tile: its workspace rows beyond B are read (unmasked) by the tile kernels -> keep them zero
        const int64_t pad = (int64_t)tiles * kTM - B;
        hipMemsetAsync(ws + wl.X + (int64_t)B * dm.CP, 0, (size_t)pad * dm.CP * sizeof(float), st);
        hipMemsetAsync(ws + wl.dH1 + (int64_t)B * kH1, 0, (size_t)pad * kH1 * sizeof(float), st);
    }
    EmbDrop drop{0u, 1.f, dropout_seed, 0u, 1.f};
    if (dense_input_dropout > 0.f && Nd > 0) {
        DT_REQUIRE(dense_input_dropout < 1.f && dropout_seed, "dt_deepfm_train_step: dense_input_dropout %f needs a rate < 1 "
                                                               "and the device seed word", dense_input_dropout);
        const double t = (double)dense_input_dropout * 4294967296.0;
        drop.thr_dense = t >= 4294967295.0 ? 4294967295u : (unsigned)t;
        if (drop.thr_dense == 0) drop.thr_dense = 1;
        drop.inv_keep_dense = 1.0f / (1.0f - dense_input_dropout);
    }
    if (embedding_dropout > 0.f) {
        DT_REQUIRE(embedding_dropout < 1.f && dropout_seed, "dt_deepfm_train_step: embedding_dropout %f needs a rate < 1 and "
                                                             "the device seed word", embedding_dropout);
        const double t = (double)embedding_dropout * 4294967296.0;
        drop.thr = t >= 4294967295.0 ? 4294967295u : (unsigned)t;
        if (drop.thr == 0) drop.thr = 1;
        drop.inv_keep = 1.0f / (1.0f - embedding_dropout);
    }
    // phase timestamps (phases | DT_STEP_STAMPS; tools/phase_times.py reads the workspace region back)
    unsigned long long* stamps = stamps_flag ? reinterpret_cast<unsigned long long*>(ws + wl.stamps) : nullptr;
    // the pipelined launch sequence of every backward step: A B C+dXn R [E|D+Adam] E'
    const bool pipe = phases >= 2;
    DT_REQUIRE(!(skip_finish || finish_only) || (pipe && !adam),
               "dt_deepfm_train_step: DT_STEP_SKIP_FINISH / DT_STEP_FINISH_ONLY belong to the pipelined backward step without "
               "the in-step optimizer");
    auto wgrad_row_blocks = [&]() {      // batch slices of the weight-gradient launch: one 512-thread block per CU
        const int nmac = (dm.CP >> 6) + 1;
        int rb = 256 / nmac;
        if (rb >= 8) rb &= ~7;
        while (rb > 1 && (B + rb - 1) / rb < 64) rb >>= 1;
        return rb < 1 ? 1 : rb;
    };
    if (finish_only) {
        const int rec_blocks_f = ceil_div(part3_layout(dm.CP, Lc, 1).n, 256);
        const RecSrc rsrc_f{reinterpret_cast<const double*>(ws + wl.racc), part3_layout(dm.CP, Lc, 1).stride};
        hipLaunchKernelGGL(k_bn_grads2, dim3(dm.C + kH2 + rec_blocks_f), dim3(256), 0, st, W1, bn_gamma, bn_beta, dm,
                           accum, al, ws + wl.wpart, wgrad_row_blocks(), Lc, cross_w, cross_b, w3, rsrc_f, dm.C + kH2, gpt);
        if (drop.thr || drop.thr_dense) hipLaunchKernelGGL(k_emb_drop_advance, dim3(1), dim3(1), 0, st, dropout_seed);
        return launch_status(dcn ? "dt_dcn_train_step" : "dt_deepfm_train_step");
    }
    DT_REQUIRE(!adam || (pipe && dd.rows_fm && !grad_rows_field_major),
               "dt_deepfm_train_step_adam: the in-step row update needs a backward step with the in-step dedupe (dedupe_ws) "
               "and row-major row gradients");

    // chained steps: both directions need a step the chain covers (dt_deepfm_step_chains)
    const bool chains = step_chains(dm, phases_all, adam && sdense, dd.rows_fm != nullptr);
    DT_REQUIRE(!prepared || chains, "dt_deepfm_train_step: DT_STEP_PREPARED on a step that cannot be chained (dt_deepfm_step_chains)");
    DT_REQUIRE(!(chain && chain->next_idx) || (chains && chain->next_rows_out && chain->next_dedupe_ws),
               "dt_deepfm_train_step_adam: next_idx on a step that cannot be chained, or without next_rows_out / next_dedupe_ws");
    StepNext nx{nullptr, nullptr, dd, 0};
    if (chain && chain->next_idx) {
        DT_REQUIRE((uintptr_t)chain->next_dedupe_ws % 16 == 0 && chain->next_dedupe_ws != dedupe_ws && chain->next_rows_out != rows_out,
                   "dt_deepfm_train_step_adam: the next step needs its own rows_out / dedupe_ws (16-byte aligned)");
        const DedupeLayout dln = dedupe_layout(B, F);
        nx.idx = chain->next_idx;
        nx.rows_out = chain->next_rows_out;
        nx.dd = dedupe_view(chain->next_dedupe_ws, dln);
        nx.eblocks = dln.eblocks;
    }
    // every host-side check sits in front of the first launch: kernel A adds into bnacc, and a step abandoned behind it
    // would hand the next step on this workspace a dirty accumulator (the workspace's zero-on-entry invariant)
    const size_t ldsC = ((size_t)kTM * (dm.CP + kPad) + 4 * dm.CP + kTM * (kH1 + kPad) + kTM * kH2S + 5 * kTM +
                         (dcn ? kCrossLds + (2 * Lc + 1) * dm.CP : 0)) * sizeof(float);
    DT_UNSUPPORTED(ldsC > 160 * 1024, "dt_dcn_train_step: the tile kernel needs %zu B of LDS", ldsC);
    if (adam && sdense) {
        const int64_t want_flat = dcn ? al.dcb + (int64_t)Lc * dm.C : al.dwlin + F + Nd;
        DT_REQUIRE(sdense->n_flat == want_flat, "dt_deepfm_train_step_adam: dense_n=%lld, the flat buffers hold "
                   "%lld floats (the accumulator layout up to its last gradient)", (long long)sdense->n_flat,
                   (long long)want_flat);
    }
    // A (a pre-elected step: rows_out / rows_fm and the segments exist already — kernel A writes neither, the prep launch
    //    has no election blocks)
    DedupeWs ddA = dd;
    if (preelected) { ddA.rows_fm = nullptr; ddA.seg_cur = nullptr; ddA.list_cur = nullptr; ddA.pid_fm = nullptr; }
    const int blocksA = ceil_div(B, kRowsPerBlockA);
    double* bnacc = reinterpret_cast<double*>(ws + wl.bnacc);
    double* racc = reinterpret_cast<double*>(ws + wl.racc);
#define DT_A(KIND, L)                                                                                        \
    hipLaunchKernelGGL((k_sparse_fwd<KIND, L, kRowsPerBlockA>), dim3(blocksA), dim3(64 * kRowsPerBlockA), 0, st, idx, \
                       (const float4*)table, row_offset, vocab, dense, w_lin, dm, ws + wl.X, ws + wl.lin, ws + wl.fm, \
                       preelected ? (int64_t*)nullptr : rows_out, oob_count, bnacc, ddA, grad_rows, ws + wl.S, drop, \
                       stamps ? stamps + (int64_t)tiles * 48 : nullptr, racc, (int)wl.racc_n, nx)
#define DT_A_L(KIND)                                                                  \
    switch (lpr) {                                                                    \
        case 1: DT_A(KIND, 1); break; case 2: DT_A(KIND, 2); break;                   \
        case 4: DT_A(KIND, 4); break; case 8: DT_A(KIND, 8); break;                   \
        default: DT_A(KIND, 16); break;                                               \
    }
    trace_mark(0, st);
    if (idx_kind == DT_IDX_F32) { DT_A_L(DT_IDX_F32) } else { DT_A_L(DT_IDX_I32) }
#undef DT_A_L
#undef DT_A
    // B
    // split-bf16 tower (DT_STEP_TOWER_X3): the DeepFM tile kernel of the pipelined backward step (DCN keeps the fp32 kernel)
    const bool x3 = x3_flag && pipe && dm.CP <= 512 && x3_fits(dm.CP);      // (wider rows: the fp32 tile kernel)
    __bf16* x3base = reinterpret_cast<__bf16*>(ws + wl.x3);
    const int64_t n1 = (int64_t)dm.CP * kH1, n2 = (int64_t)kH1 * kH2;            // elements of one part
    __bf16 *x3_w1b = x3base, *x3_w1r = x3base + 3 * n1, *x3_w2b = x3base + 5 * n1, *x3_w2r = x3base + 5 * n1 + 3 * n2;
    float* x3_cwp = ws + wl.x3 + (5 * n1 + 5 * n2 + 1) / 2;
    const X3Weights xw{x3_w1b, n1, x3_w1r, n1, x3_w2b, n2, x3_w2r, n2, x3_cwp};
    PrepOut po{ws + wl.W1L, ws + wl.W2L,
               ws + wl.W2TL, W2, x3 ? x3_w1b : nullptr, x3_w1r, x3_w2b, x3_w2r, n1, n1, n2, n2,
               x3 && dcn ? x3_cwp : nullptr, cross_w, cross_b, w3, Lc};
    const int elect_blocks = (dd.rows_fm && !preelected) ? ((((F + 7) >> 3) << 3) << dd.parts_log2) : 0;      // fields padded to 8 (XCD-aware ids)
    const size_t ldsB = elect_blocks ? (dd.seg_cur ? kElectLdsBig : kElectLds) : 0;
    if (ldsB) hipFuncSetAttribute((const void*)k_prep, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsB);
    // (a prepared step has neither an election nor layouts left to do: no prep launch)
    if (!prepared) hipLaunchKernelGGL(k_prep, dim3(56 + elect_blocks), dim3(1024), ldsB, st, dm, W1, po, 56, dd, rows_out);
    trace_mark(1, st);
    // C (always with the top of the backward: its extra outputs are simply unused by a forward-only call)
    {
#define DT_C(N)                                                                                                     \
    case N:                                                                                                         \
        if (dcn && pipe) {                                                                                          \
            hipFuncSetAttribute((const void*)k_mlp_fwd3<N, kCrossMax, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsC); \
            hipLaunchKernelGGL((k_mlp_fwd3<N, kCrossMax, true>), dim3(tiles), dim3(256), ldsC, st, ws + wl.X, mp, dm, \
                               ws + wl.lin, ws + wl.fm, y, ws + wl.H1, ws + wl.dH1, ws + wl.dH2, ws + wl.z,         \
                               logit_out, ws + wl.dlogit, ws + wl.dz, racc, stamps, dca, ws + wl.dXn);      \
        } else if (dcn) {                                                                                           \
            hipFuncSetAttribute((const void*)k_mlp_fwd3<N, kCrossMax>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsC); \
            hipLaunchKernelGGL((k_mlp_fwd3<N, kCrossMax>), dim3(tiles), dim3(256), ldsC, st, ws + wl.X, mp, dm,     \
                               ws + wl.lin, ws + wl.fm, y, ws + wl.H1, ws + wl.dH1, ws + wl.dH2, ws + wl.z,         \
                               logit_out, ws + wl.dlogit, ws + wl.dz, racc, stamps, dca, nullptr);          \
        } else if (pipe) {                                                                                          \
            hipFuncSetAttribute((const void*)k_mlp_fwd3<N, 0, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsC); \
            hipLaunchKernelGGL((k_mlp_fwd3<N, 0, true>), dim3(tiles), dim3(256), ldsC, st, ws + wl.X, mp, dm, ws + wl.lin, \
                               ws + wl.fm, y, ws + wl.H1, ws + wl.dH1, ws + wl.dH2, ws + wl.z, logit_out,           \
                               ws + wl.dlogit, ws + wl.dz, racc, stamps, dca, ws + wl.dXn);                 \
        } else {                                                                                                    \
            hipFuncSetAttribute((const void*)k_mlp_fwd3<N, 0>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsC); \
            hipLaunchKernelGGL((k_mlp_fwd3<N, 0>), dim3(tiles), dim3(256), ldsC, st, ws + wl.X, mp, dm, ws + wl.lin, \
                               ws + wl.fm, y, ws + wl.H1, ws + wl.dH1, ws + wl.dH2, ws + wl.z, logit_out,           \
                               ws + wl.dlogit, ws + wl.dz, racc, stamps, dca, nullptr);                     \
        }                                                                                                           \
        break;
#define DT_CXL(N, LCV, ONEV)                                                                                        \
    do {                                                                                                            \
        hipFuncSetAttribute((const void*)k_tower_x3<N, LCV, ONEV>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsX); \
        hipLaunchKernelGGL((k_tower_x3<N, LCV, ONEV>), dim3(tiles), dim3(512), ldsX, st, ws + wl.X, mp, xw, dm,     \
                           ws + wl.lin, ws + wl.fm, y, ws + wl.H1, ws + wl.dH1, ws + wl.dH2, ws + wl.z,             \
                           logit_out, ws + wl.dlogit, ws + wl.dz, racc, stamps, dca, ws + wl.dXn);          \
    } while (0)
#define DT_CX(N)                                                                                                    \
    case N: {                                                                                                       \
        const size_t ldsX = x3_lds_bytes(64 * N, dcn);                                                              \
        if (dcn) { if (bf16_flag) DT_CXL(N, kCrossMax, true); else DT_CXL(N, kCrossMax, false); }                   \
        else { if (bf16_flag) DT_CXL(N, 0, true); else DT_CXL(N, 0, false); }                                       \
    } break;
        if (x3) {        // the split-bf16 tower (tower_x3.h)
            switch (dm.CP >> 6) { DT_CX(1) DT_CX(2) DT_CX(3) DT_CX(4) DT_CX(5) DT_CX(6) DT_CX(7) DT_CX(8) }
        } else {
            switch (dm.CP >> 6) { DT_C(1) DT_C(2) DT_C(3) DT_C(4) DT_C(5) DT_C(6) DT_C(7) DT_C(8) DT_C(9) }
        }
#undef DT_CX
#undef DT_CXL
#undef DT_C
    }
    trace_mark(2, st);
    const Part3 pl3 = part3_layout(dm.CP, Lc, pipe ? 1 : 0);
    const RecSrc rsrc{racc, pl3.stride};                  // (the shard stride is the producing tile kernel's: its own layout's)
    const int rec_blocks = ceil_div(pl3.n, 256);          // one thread per record entry (finish_record_entry)
    if (pipe) {
        // (rounds 3-4 ran a reduction launch R here: the tile kernel's record entries are atomics into racc now, and their
        // consumers — the row epilogue's two per-column constants, the finishing launch — sum the shards themselves)
        // E + D: one 512-thread block per CU (see k_wgrad_rows)
        const int nmac = (dm.CP >> 6) + 1;
        const int row_blocks = wgrad_row_blocks();
        const int rows_per_block = ((B + row_blocks - 1) / row_blocks + 7) & ~7;
        const size_t ldsE = (size_t)4 * 8192 * sizeof(float);
        const RowsEpi ep{ws + wl.dXn, ws + wl.X, ws + wl.dz, ws + wl.S, w_lin, ws + wl.sc, ws + wl.mean, ws + wl.rstd,
                         rsrc, pl3.sdx, pl3.sdxx, rows_out, grad_rows, grad_rows_scale, grad_rows_field_major};
        // (measured in round 3: write-through row-update stores 118.1 vs 114.5 us per step, write-through tile outputs no
        // change — the kernel boundaries do not wait for this data: plain stores; the row epilogue has no write-through arm)
        RowsAdam ad = adam ? *adam : RowsAdam{nullptr, nullptr, nullptr, 0, nullptr, 0.f, 0.f, 0.f, 0.f};
        const int join_env = 1;            // the matrix waves join the row epilogue once their tile is stored
        // the weight-gradient GEMMs follow the tower's mode: exact fp32 MFMA with the exact tower, split-bf16 (two parts, like
        // the tile kernel's backward products) with the split tower, plain bf16 in the 1e-2 mode; stamped diagnostics keep fp32
        const int wm = (!x3 || stamps) ? 0 : bf16_flag ? 1 : 2;
        // the row epilogue's specialised body (rows_epilogue_wave<.., FAST>): what DeepModel.fit runs — the in-step Adam, no
        // embedding dropout, row-major gradient rows; everything else takes the generic body
        const bool fast_rows = ad.table && !drop.thr && !grad_rows_field_major;
#define DT_ED(DCNV, WMV, FASTV)                                                                                           \
    do {                                                                                                                  \
        hipFuncSetAttribute((const void*)k_wgrad_rows<DCNV, WMV, FASTV>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsE); \
        hipLaunchKernelGGL((k_wgrad_rows<DCNV, WMV, FASTV>), dim3(nmac * row_blocks), dim3(512), ldsE, st, ws + wl.X, mp, dm, \
                           ws + wl.H1, ws + wl.dH1, ws + wl.dH2, row_blocks, rows_per_block, ws + wl.wpart,                \
                           stamps ? stamps + (int64_t)tiles * 32 : nullptr, ep, ad, drop,                                 \
                           stamps ? stamps + (int64_t)tiles * 16 : nullptr, join_env, bnacc, (int)wl.bnacc_n, nx, gpt,    \
                           (adam && sdense) ? ws + wl.lrsnap : nullptr);                                               \
    } while (0)
#define DT_ED_W(DCNV, FASTV)                                                                                              \
    do { if (wm == 0) DT_ED(DCNV, 0, FASTV); else if (wm == 1) DT_ED(DCNV, 1, FASTV); else DT_ED(DCNV, 2, FASTV); } while (0)
        if (dcn) { if (fast_rows) DT_ED_W(true, true); else DT_ED_W(true, false); }
        else { if (fast_rows) DT_ED_W(false, true); else DT_ED_W(false, false); }
#undef DT_ED_W
#undef DT_ED
        trace_mark(3, st);
        if (adam && sdense) {
            // F: E' + the dense Adam + the segments + the state's advance in one launch (k_finish_step)
            // 512 blocks: 1.5 us faster with uniform ids (878 segments), 1024: 4.6 us faster with Zipf ids (15 K segments)
            const int seg_blocks = 1024;
            const int small_blocks = rec_blocks;
            const DedupeLayout dl = dedupe_layout(B, F);
            const FinishSeg fs{SegTail{dd.nseg, dd.seg_row, dd.seg_off, dd.seg_cnt, dd.seg_list, dl.regions, dl.cap},
                               adam->table, adam->m, adam->v, grad_rows, adam->sstride, D};
            const DenseAdam da{sdense->p, sdense->m, sdense->v, adam->lr_t_host, adam->b1, adam->b2, adam->eps};
            // chained steps: the next step's weight layouts, from the weights this launch updates
            const X3Lay lay = nx.idx ? X3Lay{x3_w1b, x3_w1r, x3_w2b, x3_w2r, n1, n1, n2, n2, dcn ? x3_cwp : nullptr}
                                     : X3Lay{nullptr, nullptr, nullptr, nullptr, 0, 0, 0, 0, nullptr};
            // gamma / beta: this step's values as kernel C published them (other blocks of the launch update the parameters)
            hipLaunchKernelGGL(k_finish_step, dim3(dm.C + kH2 + small_blocks + seg_blocks), dim3(256), 0, st, W1, ws + wl.gammap,
                               ws + wl.betap, dm, accum, al, ws + wl.wpart, row_blocks, da, (AdamState*)sdense->state, sdense->lr,
                               dm.C + kH2, small_blocks, seg_blocks, fs, Lc, cross_w, cross_b, w3, rsrc, lay, gpt, ws + wl.lrsnap);
            trace_mark(4, st);
        } else if (!skip_finish) {
            // E': slices added up, dW1 / dW2 / d w_lin finished; the record entries (db1 .. dgamma / dbeta) -> accum
            hipLaunchKernelGGL(k_bn_grads2, dim3(dm.C + kH2 + rec_blocks), dim3(256), 0, st, W1, bn_gamma, bn_beta, dm,
                               accum, al, ws + wl.wpart, row_blocks, Lc, cross_w, cross_b, w3, rsrc, dm.C + kH2, gpt);
        }
        if ((drop.thr || drop.thr_dense) && !skip_finish)
            hipLaunchKernelGGL(k_emb_drop_advance, dim3(1), dim3(1), 0, st, dropout_seed);
    } else {
        // forward only: reduce just the loss (the other reduced entries are ignored by the caller)
        hipLaunchKernelGGL(k_finish_records, dim3(max(rec_blocks, 8)), dim3(256), 0, st, dm, accum, al, Lc, rsrc, bnacc,
                           (int)wl.bnacc_n);
    }
    return launch_status(dcn ? "dt_dcn_train_step" : "dt_deepfm_train_step");
}

extern "C" int dt_deepfm_train_step(
    const void* idx, int idx_kind, const float* table, const int64_t* row_offset, const int32_t* vocab,
    const float* dense, const float* y, int B, int F, int D, int Nd,
    const float* w_lin, const float* bn_gamma, const float* bn_beta, float* bn_moving_mean,
    float* bn_moving_var, float bn_eps, float bn_momentum, const float* W1, const float* b1, const float* W2,
    const float* b2, const float* w3, const float* w_out, const float* b_out,
    float* logit_out, int64_t* rows_out, float* grad_rows, float* accum, void* workspace, int* oob_count,
    void* dedupe_ws, int64_t dedupe_slots, float grad_rows_scale, int grad_rows_field_major, int phases,
    float embedding_dropout, unsigned* dropout_seed, float dense_input_dropout,
    const float* sample_weight, void* stream) {
    DT_REQUIRE(w_lin, "dt_deepfm_train_step: null pointer");
    return tower_train_step(idx, idx_kind, table, row_offset, vocab, dense, y, B, F, D, Nd, w_lin, bn_gamma, bn_beta,
                            bn_moving_mean, bn_moving_var, bn_eps, bn_momentum, W1, b1, W2, b2, w3, w_out, b_out, logit_out,
                            rows_out, grad_rows, accum, workspace, oob_count, dedupe_ws, dedupe_slots, grad_rows_scale,
                            grad_rows_field_major, phases, embedding_dropout, dropout_seed, dense_input_dropout, sample_weight, stream, nullptr, nullptr, 0);
}

// the optimizer half of dt_deepfm_train_step_adam / dt_dcn_train_step_adam: its argument checks (the messages name the
// entry point `what`) and the records tower_train_step takes
struct StepAdam {
    RowsAdam ad;
    StepDense sd;
    StepChain ch;
};
static int step_adam_args(const char* what, float* table, int D, void* dedupe_ws, int phases, float* adam_m, float* adam_v,
                          int slot_stride, void* adam_state, float lr_t, float beta1, float beta2, float eps, float* dense_p,
                          float* dense_m, float* dense_v, int64_t dense_n, float lr, const void* next_idx,
                          int64_t* next_rows_out, void* next_dedupe_ws, StepAdam* out) {
    DT_REQUIRE(table && adam_m && adam_v, "%s: null pointer", what);
    DT_REQUIRE(dense_n == 0 || (dense_p && dense_m && dense_v && adam_state),
               "%s: the dense half needs the flat buffers and the device step state", what);
    DT_REQUIRE((phases & 0xf) == 2 && dedupe_ws, "%s: a backward step (phases 2) with dedupe_ws", what);
    DT_REQUIRE(slot_stride == D || slot_stride == 2 * D, "%s: slot_stride %d (D or 2 D)", what, slot_stride);
    DT_REQUIRE(((uintptr_t)table | (uintptr_t)adam_m | (uintptr_t)adam_v) % 16 == 0,
               "%s: table / slots must be 16-byte aligned", what);
    out->ad = RowsAdam{table, adam_m, adam_v, slot_stride, adam_state ? adam_state_lr_t(adam_state) : nullptr, lr_t, beta1,
                       beta2, eps};
    out->sd = StepDense{dense_p, dense_m, dense_v, dense_n, adam_state, lr};
    out->ch = StepChain{next_idx, next_rows_out, next_dedupe_ws};
    return DT_OK;
}

// the step with the row-sparse Keras-Adam update of the rows looked up ONCE applied inside it (k_wgrad_rows): `table` is
// updated in place, adam_m / adam_v are its slots (slot_stride floats between consecutive rows' records: D for two
// [V,D] arrays, 2 D for one [V,2,D] array), adam_state the device-resident step state of dt_adam_state_init (NULL:
// lr_t is the host value).  dense_n == 0: rows looked up several times leave as segments exactly as in
// dt_deepfm_train_step and are updated — with the dense parameters — by dt_adam_rows_step_seg(fields = -2), which also
// advances the state.  dense_n > 0 (= the accumulator layout up to d w_lin; dense_p / dense_m / dense_v: the model's flat
// parameter buffer and its slots, laid out like accum): the WHOLE optimizer step runs here — the step's last launch
// finishes the dense gradients, updates every dense element, walks the segments and advances the state (k_finish_step).
extern "C" int dt_deepfm_train_step_adam(
    const void* idx, int idx_kind, float* table, const int64_t* row_offset, const int32_t* vocab,
    const float* dense, const float* y, int B, int F, int D, int Nd,
    const float* w_lin, const float* bn_gamma, const float* bn_beta, float* bn_moving_mean,
    float* bn_moving_var, float bn_eps, float bn_momentum, const float* W1, const float* b1, const float* W2,
    const float* b2, const float* w3, const float* w_out, const float* b_out,
    float* logit_out, int64_t* rows_out, float* grad_rows, float* accum, void* workspace, int* oob_count,
    void* dedupe_ws, int64_t dedupe_slots, int phases, float embedding_dropout, unsigned* dropout_seed, float dense_input_dropout,
    const float* sample_weight,
    float* adam_m, float* adam_v, int slot_stride, void* adam_state, float lr_t, float beta1, float beta2,
    float eps, float* dense_p, float* dense_m, float* dense_v, int64_t dense_n, float lr,
    const void* next_idx, int64_t* next_rows_out, void* next_dedupe_ws, void* stream) {
    DT_REQUIRE(w_lin, "dt_deepfm_train_step_adam: null pointer");
    StepAdam a;
    const int rc = step_adam_args("dt_deepfm_train_step_adam", table, D, dedupe_ws, phases, adam_m, adam_v, slot_stride,
                                  adam_state, lr_t, beta1, beta2, eps, dense_p, dense_m, dense_v, dense_n, lr, next_idx,
                                  next_rows_out, next_dedupe_ws, &a);
    if (rc != DT_OK) return rc;
    return tower_train_step(idx, idx_kind, table, row_offset, vocab, dense, y, B, F, D, Nd, w_lin, bn_gamma, bn_beta,
                            bn_moving_mean, bn_moving_var, bn_eps, bn_momentum, W1, b1, W2, b2, w3, w_out, b_out, logit_out,
                            rows_out, grad_rows, accum, workspace, oob_count, dedupe_ws, dedupe_slots, 1.0f, 0, phases,
                            embedding_dropout, dropout_seed, dense_input_dropout, sample_weight, stream, nullptr, nullptr, 0, &a.ad,
                            dense_n > 0 ? &a.sd : nullptr, &a.ch);
}

// ---- DCN (nets ['dcn_nets'], deepnets.py:194-207): the same step with the Cross network (layers.py:428-436) in place of
//      the linear + FM terms ----
extern "C" int dt_dcn_supported(int B, int F, int D, int Nd, int H1, int H2, int L) {
    DeepFmDims dm; int lpr;
    if (!dt_deepfm_supported(B, F, D, Nd, H1, H2) || L < 1 || L > kCrossMax) return 0;
    if (!deepfm_dims(B, F, D, Nd, &dm, &lpr)) return 0;
    const size_t ldsC = ((size_t)kTM * (dm.CP + kPad) + 4 * dm.CP + kTM * (kH1 + kPad) + kTM * kH2S + 5 * kTM + kCrossLds +
                         (2 * L + 1) * dm.CP) * sizeof(float);
    const int FD16 = ((F * D + 15) >> 4) << 4;
    const size_t ldsD = ((size_t)kTM * (kH1 + kPad) + 2 * kTM * (dm.CP + kPad) + kTM * D + 4 * FD16 + kTM + ((F + 3) & ~3)) *
                        sizeof(float);
    return ldsC <= 160 * 1024 && ldsD <= 160 * 1024;
}

extern "C" int64_t dt_dcn_workspace_bytes(int B, int F, int D, int Nd, int L) {
    DeepFmDims dm; int lpr;
    if (!deepfm_dims(B, F, D, Nd, &dm, &lpr) || L < 1 || L > kCrossMax) return -1;
    return deepfm_ws_layout(dm, L).total * (int64_t)sizeof(float);
}

extern "C" int64_t dt_dcn_stamps_offset_floats(int B, int F, int D, int Nd, int L) {
    DeepFmDims dm; int lpr;
    if (!deepfm_dims(B, F, D, Nd, &dm, &lpr) || L < 1 || L > kCrossMax) return -1;
    return deepfm_ws_layout(dm, L).stamps;
}

extern "C" int64_t dt_dcn_accum_floats(int F, int D, int Nd, int L) {
    const int C = F * D + Nd, CP = (C + 63) & ~63;
    return deepfm_accum_layout(C, CP, F, Nd, L).total;
}

// offsets (floats) inside the accumulator buffer, in the order:
// dW1, dW2, db1, db2, dw3 [C + 64], dwo, dbo, loss, dgamma, dbeta, d cross kernels [L][C], d cross biases [L][C]
extern "C" int dt_dcn_accum_offsets(int F, int D, int Nd, int L, int64_t* out12) {
    const int C = F * D + Nd, CP = (C + 63) & ~63;
    const DeepFmAccum a = deepfm_accum_layout(C, CP, F, Nd, L);
    const int64_t v[12] = {a.dW1, a.dW2, a.db1, a.db2, a.dw3, a.dwo, a.dbo, a.loss, a.dgamma, a.dbeta, a.dcw, a.dcb};
    for (int i = 0; i < 12; ++i) out12[i] = v[i];
    return DT_OK;
}

// dt_dcn_train_step with the optimizer step inside (see dt_deepfm_train_step_adam): dense_n = dt_dcn_accum_offsets' d cross_b
// offset + L * C floats
extern "C" int dt_dcn_train_step_adam(
    const void* idx, int idx_kind, float* table, const int64_t* row_offset, const int32_t* vocab,
    const float* dense, const float* y, int B, int F, int D, int Nd,
    const float* cross_w, const float* cross_b, int L, const float* bn_gamma, const float* bn_beta,
    float* bn_moving_mean, float* bn_moving_var, float bn_eps, float bn_momentum, const float* W1, const float* b1,
    const float* W2, const float* b2, const float* w3, const float* w_out, const float* b_out,
    float* logit_out, int64_t* rows_out, float* grad_rows, float* accum, void* workspace, int* oob_count,
    void* dedupe_ws, int64_t dedupe_slots, int phases, float embedding_dropout, unsigned* dropout_seed, float dense_input_dropout,
    const float* sample_weight,
    float* adam_m, float* adam_v, int slot_stride, void* adam_state, float lr_t, float beta1, float beta2,
    float eps, float* dense_p, float* dense_m, float* dense_v, int64_t dense_n, float lr,
    const void* next_idx, int64_t* next_rows_out, void* next_dedupe_ws, void* stream) {
    DT_REQUIRE(cross_w && cross_b, "dt_dcn_train_step_adam: null pointer");
    DT_UNSUPPORTED(L < 1 || L > kCrossMax, "dt_dcn_train_step_adam: %d cross layers (1..%d)", L, kCrossMax);
    StepAdam a;
    const int rc = step_adam_args("dt_dcn_train_step_adam", table, D, dedupe_ws, phases, adam_m, adam_v, slot_stride,
                                  adam_state, lr_t, beta1, beta2, eps, dense_p, dense_m, dense_v, dense_n, lr, next_idx,
                                  next_rows_out, next_dedupe_ws, &a);
    if (rc != DT_OK) return rc;
    return tower_train_step(idx, idx_kind, table, row_offset, vocab, dense, y, B, F, D, Nd, nullptr, bn_gamma, bn_beta,
                            bn_moving_mean, bn_moving_var, bn_eps, bn_momentum, W1, b1, W2, b2, w3, w_out, b_out, logit_out,
                            rows_out, grad_rows, accum, workspace, oob_count, dedupe_ws, dedupe_slots, 1.0f, 0, phases,
                            embedding_dropout, dropout_seed, dense_input_dropout, sample_weight, stream, cross_w, cross_b, L, &a.ad,
                            dense_n > 0 ? &a.sd : nullptr, &a.ch);
}

extern "C" int dt_dcn_train_step(
    const void* idx, int idx_kind, const float* table, const int64_t* row_offset, const int32_t* vocab,
    const float* dense, const float* y, int B, int F, int D, int Nd,
    const float* cross_w, const float* cross_b, int L, const float* bn_gamma, const float* bn_beta,
    float* bn_moving_mean, float* bn_moving_var, float bn_eps, float bn_momentum, const float* W1, const float* b1,
    const float* W2, const float* b2, const float* w3, const float* w_out, const float* b_out,
    float* logit_out, int64_t* rows_out, float* grad_rows, float* accum, void* workspace, int* oob_count,
    void* dedupe_ws, int64_t dedupe_slots, int phases, float embedding_dropout, unsigned* dropout_seed, float dense_input_dropout,
    const float* sample_weight, void* stream) {
    DT_REQUIRE(cross_w && cross_b, "dt_dcn_train_step: null pointer");
    DT_UNSUPPORTED(L < 1 || L > kCrossMax, "dt_dcn_train_step: %d cross layers (1..%d)", L, kCrossMax);
    return tower_train_step(idx, idx_kind, table, row_offset, vocab, dense, y, B, F, D, Nd, nullptr, bn_gamma, bn_beta,
                            bn_moving_mean, bn_moving_var, bn_eps, bn_momentum, W1, b1, W2, b2, w3, w_out, b_out, logit_out,
                            rows_out, grad_rows, accum, workspace, oob_count, dedupe_ws, dedupe_slots, 1.0f, 0, phases,
                            embedding_dropout, dropout_seed, dense_input_dropout, sample_weight, stream, cross_w, cross_b, L);
}
