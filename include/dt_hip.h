/*
 * dt_hip.h — C-ABI of libdt_hip.so: the MI355X (gfx950 / CDNA4) kernels behind the
 * DeepTables `deeptables.models.layers` hot path.
 *
 * The reference (DataCanvasIO/DeepTables) is 100 % Python on TensorFlow/Keras and has no FFI
 * of its own; the "boundary" it exposes for this path is the Keras `Layer.call` of each class
 * in deeptables/models/layers.py.  Every entry point below replaces the TF op sequence of one
 * `call` (forward) and of its autodiff (backward); the citation next to each declaration is
 * the reference code it replaces (paths relative to the reference checkout).
 *
 * Conventions
 *   - plain C, no C++/torch types.  All pointers are DEVICE pointers (HBM) unless the name
 *     ends in `_host`.  The caller owns every buffer (in the Python host these are
 *     torch.Tensor storages); the library never allocates, frees or synchronises.
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*; NULL = default
 *     stream), stateless and re-entrant.  Launches are hipGraph-capturable.
 *   - all tensors are dense, row-major, contiguous, fp32 unless stated; sizes are explicit.
 *   - return value: DT_OK (0) or a negative DT_ERR_* code; dt_last_error() returns a
 *     thread-local human readable message for the last failing call on this thread.
 *   - "idx_kind": categorical ids arrive either as float32 (the reference's tf.data contract,
 *     utils/dataset_generator.py:41-42; cast with truncation exactly like
 *     keras.ops.cast(inputs,'int32'), models/layers.py:893-895) or as int32 (fast path).
 *   - out-of-range ids read as a zero row (TF-GPU embedding_lookup behaviour) and are counted
 *     into the optional `oob_count` device counter so the host can raise like TF-CPU does.
 */
#ifndef DT_HIP_H
#define DT_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DT_OK 0
#define DT_ERR_INVALID_ARG (-1)   /* bad size / null pointer / unsupported combination   */
#define DT_ERR_UNSUPPORTED (-2)   /* shape outside what the kernels are specialised for   */
#define DT_ERR_LAUNCH (-3)        /* hipGetLastError() != hipSuccess after a launch       */

#define DT_IDX_F32 0
#define DT_IDX_I32 1

#define DT_ACT_LINEAR 0
#define DT_ACT_RELU 1
/* keras.activations the CIN / AFM kernels also fuse (layers.py:709, :783 `Activation(name)`); each derivative is a
 * function of the OUTPUT, so the backward needs no pre-activation: */
#define DT_ACT_SIGMOID 2      /* y (1 - y) */
#define DT_ACT_TANH 3         /* 1 - y^2 */
#define DT_ACT_ELU 4          /* alpha = 1: y > 0 ? 1 : y + 1 */
#define DT_ACT_SELU 5         /* y > 0 ? scale : y + scale alpha */
#define DT_ACT_SOFTPLUS 6     /* 1 - exp(-y) */
#define DT_ACT_SOFTSIGN 7     /* (1 - |y|)^2 */
#define DT_ACT_EXPONENTIAL 8  /* y */
#define DT_ACT_COUNT 9

#define DT_OP_KERNEL_MAT 0
#define DT_OP_KERNEL_VEC 1
#define DT_OP_KERNEL_NUM 2

/* ---- library --------------------------------------------------------------------------- */
int dt_version(void);                 /* ABI version, currently 1 */
const char* dt_last_error(void);      /* thread-local message of the last failing call */
const char* dt_build_arch(void);      /* "gfx950" */
const char* dt_source_hash(void);     /* sha256[:16] of the sources this binary was built from (__graft_entry__.source_hash) */
/* hipGraphUpload of an instantiated graph (hipGraphExec_t) onto `stream`: the compiled train loop (deeptables_amd/compiled.py,
 * Keras steps_per_execution, deepmodel.py:319-346) uploads its captured k-step graph once, so that the first replay costs
 * what every later one costs.  Goes through this library's HIP runtime, i.e. the one the host framework loaded.        */
int dt_graph_upload(void* graph_exec, void* stream);
/* Launch-boundary trace of the fused train step (measurement plumbing, bench.py's `kernel_split_us`): after dt_step_trace(1)
 * every dt_deepfm_train_step_adam / dt_dcn_train_step_adam this thread enqueues EAGERLY (never inside a stream capture)
 * records a HIP event on its stream in front of its first launch and behind each launch group — A (+ the prep launch of an
 * unprepared step) | C | E||D | F, the four launches that replace the ~100 TF ops of one keras train step
 * (deepmodel.py:114-129).  dt_step_trace_read waits for the last traced step and writes the four intervals in
 * microseconds, averaged over the steps traced since dt_step_trace(1) (the last 32 at most), to us_host[0..3] (HOST
 * pointer, n >= 4) and their number to *steps_host (HOST, may be NULL).  dt_step_trace(0) switches the recording off.  */
int dt_step_trace(int enable);
int dt_step_trace_read(float* us_host, int n, int* steps_host);

/* ---- a2  MultiColumnEmbedding.call  (models/layers.py:889-904) -------------------------- *
 * All F columns live in ONE packed table [sum_f vocab_f, D]; column f starts at row
 * row_offset[f] and has vocab[f] rows (same D for every column; per-column D is handled by
 * the host with one call per D-group).
 *   idx        [B,F]  float32 or int32 (idx_kind)
 *   out        [B,F,D]           out[b,f,:] = table[row_offset[f] + int(idx[b,f]), :]
 *   rows_out   [B,F] int64 or NULL: the resolved packed row per lookup (the `indices` half
 *              of TF's IndexedSlices gradient); -1 for an out-of-range id.
 * The gather is a bit-exact copy.                                                           */
int dt_embedding_fwd(const void* idx, int idx_kind, const float* table,
                     const int64_t* row_offset, const int32_t* vocab,
                     int B, int F, int D, float* out, int64_t* rows_out,
                     int* oob_count, void* stream);

/* Backward of the gather into a DENSE gradient table (TF densifies IndexedSlices for
 * optimizers without a sparse path): grad_table[rows[b,f],:] += grad_out[b,f,:].
 * grad_table must be zeroed by the caller.  Rows < 0 are skipped.                           */
int dt_embedding_bwd_dense(const int64_t* rows, const float* grad_out, int n_lookups, int D,
                           float* grad_table, void* stream);

/* The gather with the layer's embedding dropout inside the launch (csrc/emb_dropout.hip): MultiColumnEmbedding's one
 * SpatialDropout1D per column on its [B,1,D] output (models/layers.py:878-880, :900-902; VarLenColumnEmbedding's on the
 * [B,1,L*D] output, :953-954, :962-963), i.e. element dropout with 1 / (1 - rate) scaling, forward and backward.
 *   out[b,f,d] = table[row,d] * keep(b, col_base[f] + d),  keep = fl(1 / (1 - fl(rate))) where
 *   dt_cell_dropout_hash(seed[0], salt, b, col_base[f] + d) >= dt_cell_dropout_threshold(rate), else 0
 * — the cell hash (dt_cell_fwd), no third hash family and no mask tensor.  col_base: DEVICE int [F], the position of column
 * f's first element in the concatenation of ALL of the layer's outputs in column order, so the packed tables of one layer
 * (one call per D-group) use the slices of ONE [B, sum D] mask.  seed: DEVICE, one word, read by the kernel (a captured graph
 * sees a fresh word at every replay); the backward recomputes keep from the same word and salt.
 * dt_embedding_drop_fwd: every other argument, rows_out, oob_count and the zero row / row -1 of an out-of-range id as
 *   dt_embedding_fwd; the kept values are the table's bits times the scale.
 * dt_embedding_drop_bwd: ONE launch, exactly one of the two outputs non-NULL:
 *   values     [B*F, D]  sparse mode: values[r,:] = grad_out[r,:] * keep — with rows the (indices, values) gradient pair
 *   grad_table           dense mode:  grad_table[rows[r],:] += grad_out[r,:] * keep by float atomicAdd, rows < 0 skipped;
 *                        zeroed by the caller; no masked intermediate exists.  rows may be NULL in sparse mode.
 * 16-byte lanes for every D % 4 == 0 with 16-byte aligned table / out (grad_out / values), a power of two or not; floats for
 * any other D and for the dense mode (consecutive lanes add to consecutive dwords).  A grid-stride loop over at most
 * dt_embedding_drop_pass_units() units (16-byte lanes or floats) per pass.  Domain: 0 < rate < 1 (rate 0 is dt_embedding_fwd),
 * B F D < 2^31 (32-bit index arithmetic); outside it, a null or misaligned pointer: DT_ERR_INVALID_ARG before any launch.   */
int64_t dt_embedding_drop_pass_units(void);
int dt_embedding_drop_fwd(const void* idx, int idx_kind, const float* table, const int64_t* row_offset,
                          const int32_t* vocab, int B, int F, int D, float rate, const int* seed, unsigned salt,
                          const int* col_base, float* out, int64_t* rows_out, int* oob_count, void* stream);
int dt_embedding_drop_bwd(const int64_t* rows, const float* grad_out, int B, int F, int D, float rate, const int* seed,
                          unsigned salt, const int* col_base, float* values, float* grad_table, void* stream);

/* ---- a4  FM.call  (models/layers.py:53-62) ----------------------------------------------- *
 *   x [B,F,D] -> out [B]  = 0.5 * sum_d[(sum_f x)^2 - sum_f x^2]
 *   backward: grad_x[b,f,d] = grad_out[b] * (S[b,d] - x[b,f,d]),  S = sum_f x               */
int dt_fm_fwd(const float* x, int B, int F, int D, float* out, void* stream);
int dt_fm_bwd(const float* x, const float* grad_out, int B, int F, int D, float* grad_x,
              void* stream);

/* ---- a2+a3+a4 fused: embedding gather + linear field-sum + FM --------------------------- *
 * (models/layers.py:889-904 + models/deepnets.py:43-66 `linear` + models/layers.py:53-62)
 *   emb_out   [B,F,D]  gathered rows (bit-exact)                       (may be NULL)
 *   concat_out[B, F*D+Nd] = [flatten(emb), dense]  (deepmodel.py:269-274,348-353; may be NULL)
 *   field_sum [B,F]    s[b,f] = sum_d emb[b,f,d]   (deepnets.py:51)    (may be NULL)
 *   fm_out    [B]      FM second-order term                            (may be NULL)
 *   dense     [B,Nd]   continuous inputs (only read when concat_out != NULL; Nd may be 0)   */
int dt_embed_fm_linear_fwd(const void* idx, int idx_kind, const float* table,
                           const int64_t* row_offset, const int32_t* vocab,
                           const float* dense, int B, int F, int D, int Nd,
                           float* emb_out, float* concat_out, float* field_sum, float* fm_out,
                           int64_t* rows_out, int* oob_count, void* stream);

/* Fused backward of the three consumers of the embedding block.  Any grad input may be NULL.
 *   grad_rows[b,f,d] = g_concat[b, f*D+d] + g_field_sum[b,f] + g_fm[b]*(S[b,d]-emb[b,f,d])
 *                      (+ g_emb[b,f,d])
 * `emb` is the saved forward activation [B,F,D] (or the re-gathered rows).
 * g_concat has row stride concat_stride (= F*D+Nd) floats.                                  */
int dt_embed_fm_linear_bwd(const float* emb, const float* g_emb, const float* g_concat,
                           int concat_stride, const float* g_field_sum, const float* g_fm,
                           int B, int F, int D, float* grad_rows, void* stream);

/* ---- a5  BatchNormalization on concat_emb_dense (models/deepmodel.py:348-361, Keras BN) -- *
 * Training forward over x [N,C] (N = batch, or batch*fields for MultiheadAttention's BN):
 *   mean/var: biased batch statistics (two-pass-accurate, Chan-merged Welford)
 *   y = gamma*(x-mean)*rsqrt(var+eps)+beta
 *   moving_mean = moving_mean*momentum + mean*decay          (same for var; biased var)
 *   decay = 1-momentum, rounded to float from the DOUBLE as Keras does: (float)(1.0 - 0.99) is 0.01f, where
 *   1.f - 0.99f is 9.5e-7 off it
 * save_mean/save_rstd [C] are written for the backward.  ws: workspace of
 * dt_bn_workspace_bytes(N,C) bytes.                                                          */
int64_t dt_bn_workspace_bytes(int N, int C);
int dt_bn_train_fwd(const float* x, int N, int C, const float* gamma, const float* beta,
                    float eps, float momentum, float decay, float* moving_mean, float* moving_var,
                    float* y, float* save_mean, float* save_rstd, void* ws, void* stream);
int dt_bn_infer_fwd(const float* x, int N, int C, const float* gamma, const float* beta,
                    float eps, const float* moving_mean, const float* moving_var, float* y,
                    void* stream);
/*   grad_x = gamma*rstd*(g - mean_N(g) - xhat*mean_N(g*xhat));  grad_gamma=sum g*xhat; grad_beta=sum g */
int dt_bn_train_bwd(const float* x, const float* grad_y, int N, int C, const float* gamma,
                    const float* save_mean, const float* save_rstd, float* grad_x,
                    float* grad_gamma, float* grad_beta, void* ws, void* stream);
/* reduction half of dt_bn_train_bwd only: sums [2C] = sum_n grad_y | sum_n grad_y * xhat (also grad_beta / grad_gamma) */
int dt_bn_train_bwd_stats(const float* x, const float* grad_y, int N, int C, const float* save_mean,
                          const float* save_rstd, float* sums, float* grad_gamma, float* grad_beta, void* ws, void* stream);

/* ---- a8  Cross.call  (models/layers.py:428-436) ------------------------------------------ *
 *   x [B,C]; w,b [L,C] (kernels_l / bias_l, each (C,1) in Keras, stacked)
 *   x_{l+1} = x_0 * (x_l . w_l) + x_l + b_l ; out = x_L [B,C]
 *   save_s [B,L]: the per-layer scalars s_l = x_l . w_l (all the backward needs besides x).  */
int dt_cross_fwd(const float* x, const float* w, const float* b, int B, int C, int L,
                 float* out, float* save_s, void* stream);
/*   grad_w, grad_b [L,C] are ACCUMULATED (+=): zero them first.  ws: workspace of
 *   dt_cross_workspace_bytes(B,C,L) bytes (per-block partial sums; no global float atomics). */
int64_t dt_cross_workspace_bytes(int B, int C, int L);
int dt_cross_bwd(const float* x, const float* w, const float* b, const float* save_s,
                 const float* grad_out, int B, int C, int L, float* grad_x, float* grad_w,
                 float* grad_b, void* ws, void* stream);

/* ---- a9  InnerProduct.call  (models/layers.py:473-487) ----------------------------------- *
 *   x [B,F,D] -> out [B,P], P=F(F-1)/2, pairs (i<j) row-major: out[b,p]=<x[b,i],x[b,j]>     */
int dt_inner_product_fwd(const float* x, int B, int F, int D, float* out, void* stream);
int dt_inner_product_bwd(const float* x, const float* grad_out, int B, int F, int D,
                         float* grad_x, void* stream);

/* ---- a10 OuterProduct.call  (models/layers.py:543-581) ----------------------------------- *
 *   kernel_type mat: K [D,P,D]  out[b,p] = sum_a sum_d x[b,i,d]*K[a,p,d]*x[b,j,a]
 *               vec: K [P,D]    out[b,p] = sum_d x[b,i,d]*x[b,j,d]*K[p,d]
 *               num: K [P,1]    out[b,p] = K[p]*sum_d x[b,i,d]*x[b,j,d]
 *   grad_kernel is ACCUMULATED with atomics: zero it first.                                  */
int dt_outer_product_fwd(const float* x, const float* kernel, int kernel_type, int B, int F,
                         int D, float* out, void* stream);
int dt_outer_product_bwd(const float* x, const float* kernel, int kernel_type,
                         const float* grad_out, int B, int F, int D, float* grad_x,
                         float* grad_kernel, void* stream);

/* ---- a11 CIN layer  (models/layers.py:689-710) -------------------------------------------- *
 * One CIN layer: y[b,l,d] = act( sum_{i<F0, j<Hk} x0[b,i,d] * xk[b,j,d] * W[i*Hk+j, l] + bias[l] )
 *   x0 [B,F0,D], xk [B,Hk,D] (batch strides x0_bstride / xk_bstride in floats, so xk can be the
 *   [:, :Hk] channel slice of the previous layer's [B,L,D] output when direct=False),
 *   W [F0*Hk, L] (Keras filter f_k with the leading 1 squeezed),
 *   bias [L] or NULL, y [B,L,D] (already in the transposed layout of layers.py:710).
 * Exact-fp32 MFMA (v_mfma_f32_32x32x2_f32); the Z = x0 (x) xk tensor is generated on the fly
 * in LDS and never written to HBM.
 * Backward (G = grad_y * act'(y)): grad_x0, grad_xk (ACCUMULATED: caller zeroes or passes the
 * running gradient), grad_W [F0*Hk, L] and grad_bias [L] (ACCUMULATED: zero first).          */
int dt_cin_layer_fwd(const float* x0, const float* xk, const float* W, const float* bias,
                     int act, int B, int F0, int Hk, int L, int D, int64_t x0_bstride,
                     int64_t xk_bstride, float* y, void* stream);
int dt_cin_layer_bwd(const float* x0, const float* xk, const float* W, const float* y,
                     const float* grad_y, int act, int B, int F0, int Hk, int L, int D,
                     int64_t x0_bstride, int64_t xk_bstride, float* grad_x0, float* grad_xk,
                     float* grad_W, float* grad_bias, void* stream);
/* the same with a workspace (dt_cin_bwd_workspace_bytes, 16-byte aligned): the weight-gradient kernel's batch splits store
 * their partial [K][L] tiles there and one reduction adds them to grad_W — no float atomics (16.7 M per layer at the
 * Criteo shape), deterministic.  In this form grad_x0, grad_xk and grad_W are OVERWRITTEN (no zero-fill by the caller);
 * grad_bias is still accumulated. */
int64_t dt_cin_bwd_workspace_bytes(int B, int F0, int Hk, int L, int D);
int dt_cin_layer_bwd_ws(const float* x0, const float* xk, const float* W, const float* y,
                        const float* grad_y, int act, int B, int F0, int Hk, int L, int D,
                        int64_t x0_bstride, int64_t xk_bstride, float* grad_x0, float* grad_xk,
                        float* grad_W, float* grad_bias, void* ws, void* stream);
/* CIN `direct=False` split (layers.py:713-721, :726): of a layer's output y [B,L,D] the channels [half, L) leave the stack and
 * only their sum over D is used.  dt_cin_pool: pooled [B, L-half] = sum_D y[:, half:, :] (half = 0: every channel — the last
 * layer).  dt_cin_pool_bwd: the layer's incoming gradient gy [B,L,D] in one pass = concat(g_hidden [B,half,D] or zeros
 * when NULL, g_pooled [B,L-half] broadcast over D or zeros when NULL).  D % 4 == 0. */
int dt_cin_pool(const float* y, int64_t B, int L, int D, int half, float* pooled, void* stream);
int dt_cin_pool_bwd(const float* g_hidden, const float* g_pooled, int64_t B, int L, int D, int half, float* gy, void* stream);

/* ---- a12 MultiheadAttention core (models/layers.py:129-145) ------------------------------- *
 * q,k,v [B,F,D] (already relu(Dense(x)), layers.py:123-125); H heads split on the last axis
 * (d_h = D/H); out[b,:,h] = softmax(q_h k_h^T / sqrt(d_h)) v_h, heads merged back on the last
 * axis -> out [B,F,D].  Nothing of size [B,H,F,F] is written: the forward saves only
 * stats [B,H,F,2] = (m, 1 / l) of each scaled score row (its maximum and the inverse of sum_j exp(s_j - m)) and the backward
 * recomputes the probabilities as exp(s - m) * (1 / l), bit for bit the forward's weights.  lse [B,H,F] = m + log l is an output for
 * callers that want it; the backward does not take it (one float cannot hold m + log l to better than 2^-24 |m|, and that
 * much error in every probability is 1 % once the scores reach 1e5).  Either of lse and stats may be NULL (inference).
 * The backward is two launches: ws [B,H,F] floats receives delta_i = sum_j p_ij keep_ij (dO_i . v_j) from the first.
 * ld: distance in floats between consecutive field rows of q/k/v (D when contiguous; 4D when they are column
 * blocks of one fused [B,F,4D] projection output); ldg: the same for grad_q/grad_k/grad_v.
 * dropout_rate / seed: Dropout on the attention weights (layers.py:141) with the keep-mask of dt_autoint_dropout_hash
 * (F <= 64 then) >= dt_autoint_dropout_threshold(dropout_rate); 0 at inference.
 * Shape domain: head width D/H <= 64 in the forward and <= 32 in the backward, F <= 64 with dropout; outside it both
 * return DT_ERR_UNSUPPORTED before any launch.  dt_mha_core_supported(F, D, H, dropout != 0) = 1 iff BOTH directions
 * take the shape (what a layer that trains needs).  Rows are moved as float4 when d_h, D, ld (and ldg) are multiples of 4
 * and every row pointer is 16-byte aligned, one float at a time otherwise: both give the same bits.     */
int dt_mha_core_supported(int F, int D, int H, int dropout);
int dt_mha_core_fwd(const float* q, const float* k, const float* v, int B, int F, int D, int H, int ld,
                    float dropout_rate, unsigned seed, float* out, float* lse, float* stats, void* stream);
int dt_mha_core_bwd(const float* q, const float* k, const float* v, const float* stats, const float* grad_out,
                    int B, int F, int D, int H, int ld, int ldg, float dropout_rate, unsigned seed,
                    float* grad_q, float* grad_k, float* grad_v, float* ws, void* stream);

/* ---- a13 optimizer step (Keras Adam, models/deepmodel.py:321-322) ------------------------- *
 * Keras semantics: lr_t = lr*sqrt(1-b2^t)/(1-b1^t); m,v EMA; p -= lr_t*m/(sqrt(v)+eps).
 * Dense: n contiguous floats.
 * Rows: row-sparse ("lazy") variant over the step's sparse gradient (rows [n] packed row ids, -1 = skipped;
 * values [n,D]): duplicate lookups of a row are merged INTO `values` (the first occurrence's row receives the
 * sum) through an open-addressing hash — slots: dt_adam_rows_slots(n) 8-byte entries, all zero on entry and
 * left all zero on return; mark: n int32 scratch — then every distinct row's p/m/v is updated once.
 * fields > 0 promises that rows is laid out [.., fields] over a packed table whose fields own disjoint row
 * ranges (MultiColumnEmbedding): each field then dedupes in LDS (one workgroup per field, up to 8192 lookups
 * per field) and `slots` is not touched.  fields = -1: the rows are already distinct (e.g. deduplicated by
 * dt_deepfm_train_step) — no dedupe pass, slots/mark may be NULL.
 * `state` (DT_ADAM_STATE_BYTES = 272 device bytes, may be NULL): {int32 t = the step the NEXT update uses, float
 * lr_t for that step, block-arrival counters}.  When given, lr_t is READ FROM THE DEVICE instead of the scalar argument, so a
 * captured hipGraph of the whole step replays correctly.  dt_adam_state_init writes it for `steps_done` completed
 * steps; the state is advanced (t += 1, lr_t recomputed) either by dt_adam_advance or — with no launch of its own —
 * by the last block of a dt_adam_dense_step / dt_adam_rows_step called with advance != 0, which must be the LAST
 * launch of the step.  dt_adam_rows_step can carry one dense update (dense_* arrays, dense_n elements; 0 = none) in
 * trailing blocks of its row kernel, so a model with one big table and one flat dense buffer updates in ONE launch.
 * Row slots m / v: two separate [V, D] arrays, or the two halves of ONE [V, 2, D] array (pass v == m + D): a row's m
 * and v then share a 128-byte line. */
#define DT_ADAM_STATE_BYTES 272
int dt_adam_state_init(void* state, float lr, float beta1, float beta2, int steps_done, void* stream);
int dt_adam_advance(void* state, float lr, float beta1, float beta2, void* stream);
int dt_adam_dense_step(float* p, const float* g, float* m, float* v, int64_t n, float lr_t,
                       float beta1, float beta2, float eps, void* state, int advance, float lr, void* stream);
/* `count` dense tensors in one launch (chunks of 32): HOST arrays of device pointers / element counts. */
int dt_adam_multi_step(int count, float* const* p, const float* const* g, float* const* m, float* const* v,
                       const int64_t* n, float lr_t, float beta1, float beta2, float eps, void* state, int advance,
                       float lr, void* stream);
int64_t dt_adam_rows_slots(int64_t n_rows);
int dt_adam_rows_step(float* table, float* m, float* v, const int64_t* rows, float* values, int64_t n_rows,
                      int D, int fields, void* slots, int64_t n_slots, int* mark, float lr_t, float beta1,
                      float beta2, float eps, void* state, float* dense_p, const float* dense_g, float* dense_m,
                      float* dense_v, int64_t dense_n, int advance, float lr, void* stream);
/* dt_adam_rows_step + SEGMENTS (seg_nseg != NULL; D = 4 * 2^k): rows looked up several times arrive in seg_regions
 * regions of seg_cap slots: region e holds seg_nseg[e] segments (read on the device) at index s = e * seg_cap + i:
 * (seg_row[s], seg_off[s], seg_cnt[s]) with seg_list[seg_off .. +seg_cnt) naming the `values` rows to sum.  Their
 * entries of `rows` must be -1.  The waves of the same launch sum a segment's members and apply the update to its table
 * row: no lookup adds into a shared gradient row.  slot_stride: floats between a row's m (and v) of consecutive table rows —
 * D: m and v are two [V, D] arrays; 2 D: ONE [V, 2, D] array, v = m + D (a row's m and v in one 128-byte line).  Stated by
 * the caller, as in dt_deepfm_train_step_adam (dt_adam_rows_step, without the argument, infers 2 D from v == m + D).   */
/* dt_rows_compact — the "bucketed sparse embedding gradient" of the data-parallel exchange (replaces what
 * tf.distribute.MirroredStrategy all-gathers for an IndexedSlices gradient, deepmodel.py:88-103): a fused step's sparse
 * gradient (rows looked up once as entries of (rows, values), rows looked up several times as segments — dt_deepfm_train_step)
 * becomes UNIQUE (row, summed gradient * scale) entries packed at the front of out_rows [cap] / out_vals [cap, D];
 * unused slots hold row -1.  counter2 (two device ints, zeroed by the caller once): [0] = entries produced by THIS call
 * (reset by every call), [1] = entries dropped because they did not fit `cap`, a RUNNING total over all calls (check it on
 * the host outside the step, at any later time).  seg_* as in dt_adam_rows_step_seg (seg_nseg NULL: no segments). */
/* dt_rows_merge_segments — the same bucket without packing (no slot counter): in place, every segment's members are summed
 * into the gradient row of its FIRST member, whose entry of `rows` gets the table row back (the other members keep -1):
 * (rows, values) then holds one entry per distinct row of the rank in its original [.., fields] layout. */
int dt_rows_merge_segments(int64_t* rows, float* values, int D, const int* seg_nseg, const int64_t* seg_row,
                           const int* seg_off, const int* seg_cnt, const int* seg_list, int seg_regions, int seg_cap,
                           void* stream);
int dt_rows_compact(const int64_t* rows, const float* values, int64_t n_rows, int D, const int* seg_nseg,
                    const int64_t* seg_row, const int* seg_off, const int* seg_cnt, const int* seg_list,
                    int seg_regions, int seg_cap, float scale, int64_t cap, int64_t* out_rows, float* out_vals,
                    int* counter2, void* stream);
int dt_adam_rows_step_seg(float* table, float* m, float* v, const int64_t* rows, float* values, int64_t n_rows, int D,
                          int fields, void* slots, int64_t n_slots, int* mark, float lr_t, float beta1, float beta2,
                          float eps, void* state, float* dense_p, const float* dense_g, float* dense_m, float* dense_v,
                          int64_t dense_n, int advance, float lr, const int* seg_nseg, const int64_t* seg_row,
                          const int* seg_off, const int* seg_cnt, const int* seg_list, int seg_regions, int seg_cap,
                          int slot_stride, void* stream);

/* BinaryCrossentropy on a sigmoid output, evaluated from the logits as Keras does in graph mode (deepmodel.py:326-328;
 * the `task_output` activation, deepmodel.py:436-457): loss [1] = mean(max(z,0) - z*y + log1p(exp(-|z|))) and
 * dz [n] = (sigmoid(z) - y) / n in one launch (the op chain is ~16 element-wise launches otherwise).            */
int dt_bce_logits(const float* z, const float* y, int64_t n, float* loss, float* dz, void* stream);

/* keras.optimizers.SGD (momentum 0), selectable through ModelConfig.optimizer (deepmodel.py:319-323):
 * p -= lr*g; the rows variant applies the (rows, values) gradient directly (duplicate rows add up).   */
int dt_sgd_dense_step(float* p, const float* g, int64_t n, float lr, void* stream);
int dt_sgd_rows_step(float* table, const int64_t* rows, const float* values, int64_t n_rows, int D, float lr,
                     void* stream);

/* keras.optimizers.Adagrad(learning_rate=1e-3, initial_accumulator_value=0.1, epsilon=1e-7) and
 * keras.optimizers.RMSprop(learning_rate=1e-3, rho=0.9, momentum=0, epsilon=1e-7, centered=False), selectable through
 * ModelConfig.optimizer (deepmodel.py:319-345, "str or object"):
 *     Adagrad: acc += g*g                  ; p -= lr * g / (sqrt(acc) + eps)     (the caller fills acc with its initial value)
 *     RMSprop: rms = rho*rms + (1-rho)*g*g ; p -= lr * g / (sqrt(rms) + eps)     (rms starts at 0)
 * One slot per element.  `state`: the device step state of dt_adam_state_init (DT_ADAM_STATE_BYTES; only t and the arrival
 * counters are used, pass beta1 = beta2 = 0): the LAST launch of a step is called with advance != 0 and its last block
 * advances t; dt_adam_advance advances a step that launches nothing.
 * Dense (replaces one keras `_resource_apply_dense` per variable): n contiguous floats, float4 body when p, g and the slot
 * are 16-byte aligned, the scalar loop otherwise; pointers that are not float aligned are refused.  The multi forms take
 * `count` tensors (HOST arrays of device pointers / element counts) in launches of 32 tensors.
 * Rows (replaces `_resource_apply_sparse` behind `_deduplicate_indexed_slices`): rows / values / fields / slots / n_slots /
 * mark and the dense tail exactly as dt_adam_rows_step (fields >= -1; the same merge of duplicate lookups into `values`);
 * the owner of every distinct row then updates the table row and its slot record: slot + row * slot_stride, slot_stride >= D
 * floats.  Any D > 0; with D % 4 == 0 table, slot and values must be 16-byte aligned and slot_stride % 4 == 0.  Rows that
 * were not looked up keep p and, for Adagrad, acc bit for bit: that IS Keras' result (their gradient is zero).
 * RMSprop rows decay lazily and exactly: stamp[row * stamp_stride] (int32, 0 at first) is the step at which the row's rms
 * was last written; a looked-up row first takes rms *= rho^(t - stamp - 1), t read from `state` (required), then the
 * update, and its stamp becomes t.  The stamp may live in its own [V] array (stamp_stride 1) or inside the slot record
 * (stamp = (int*)(rms + D), stamp_stride = slot_stride >= D + 1).  dt_rmsprop_rows_materialize applies the decay pending
 * on every row, rho^(steps done - stamp), and sets every stamp to the steps done: rms then holds Keras' dense slot, and the
 * next step is unchanged by it.                                                                                          */
int dt_adagrad_dense_step(float* p, const float* g, float* acc, int64_t n, float lr, float eps, void* state, int advance,
                          void* stream);
int dt_rmsprop_dense_step(float* p, const float* g, float* rms, int64_t n, float lr, float rho, float eps, void* state,
                          int advance, void* stream);
int dt_adagrad_multi_step(int count, float* const* p, const float* const* g, float* const* acc, const int64_t* n, float lr,
                          float eps, void* state, int advance, void* stream);
int dt_rmsprop_multi_step(int count, float* const* p, const float* const* g, float* const* rms, const int64_t* n, float lr,
                          float rho, float eps, void* state, int advance, void* stream);
int dt_adagrad_rows_step(float* table, float* acc, const int64_t* rows, float* values, int64_t n_rows, int D, int fields,
                         void* slots, int64_t n_slots, int* mark, float lr, float eps, void* state, float* dense_p,
                         const float* dense_g, float* dense_acc, int64_t dense_n, int advance, int slot_stride, void* stream);
int dt_rmsprop_rows_step(float* table, float* rms, int* stamp, const int64_t* rows, float* values, int64_t n_rows, int D,
                         int fields, void* slots, int64_t n_slots, int* mark, float lr, float rho, float eps, void* state,
                         float* dense_p, const float* dense_g, float* dense_rms, int64_t dense_n, int advance,
                         int slot_stride, int stamp_stride, void* stream);
int dt_rmsprop_rows_materialize(float* rms, int* stamp, int64_t V, int D, int slot_stride, int stamp_stride, float rho,
                                const void* state, void* stream);

/* keras.optimizers.SGD with momentum != 0, keras.optimizers.Adamax and keras.optimizers.Ftrl (Keras 3's formulas), selectable
 * through ModelConfig.optimizer (csrc/optim_slots.hip).  Arguments as in their dt_adagrad_* counterparts — the same `state`
 * (dt_adam_state_init with beta1 = beta2 = 0; the last launch of a step has advance != 0), the same float4 body / scalar loop
 * for dense arrays, the same chunks of 32 tensors, the same rows / values / fields / slots / n_slots / mark and dense tail —
 * with the second slot behind the first wherever a slot is passed and the hyperparameters in place of (lr, eps).
 *     SGD:    m = momentum*m - lr*g ; p += m                           (nesterov != 0: p += momentum*m - lr*g); m starts at 0
 *     Adamax: m += (g - m)*(1 - beta1) ; u = max(beta2*u, |g|) ; p -= lr*m / ((1 - beta1^t)*(u + eps));        m, u start at 0
 *             t (1-based) is read from `state` on the device (required wherever an element is updated): a captured graph
 *             replays the launch with the right power.
 *     Ftrl:   g' = g + 2*l2_shrinkage*p ; n' = accum + g*g ; linear += g' - (n'^a - accum^a)/lr * p,   a = -lr_power
 *             q = n'^a/lr + 2*l2 ; p = (clip(linear, -l1, l1) - linear)/q ; accum = n'
 *             `l2` is l2_regularization_strength + beta/(2 lr), folded by the caller; the caller fills accum with
 *             initial_accumulator_value, linear with 0.  q == 0 (n' == 0 and l2 == 0) writes p = 0 where Keras writes NaN.
 *             lr_power == -0.5 takes sqrtf, any other lr_power <= 0 powf.  lr <= 0, lr_power > 0 or a negative l1 / l2 /
 *             l2_shrinkage is refused.  With g == 0 the formula does NOT leave p alone (p is a function of linear and accum).
 * Rows: the two slots of table row r are slot0 + r * slot_stride and slot1 + r * slot_stride (slot_stride >= D floats), so
 * they may be two [V, D] arrays (slot_stride D) or ONE [V, 2, D] record (slot1 = slot0 + D, slot_stride 2 D: two random
 * locations per row).  Only the looked-up rows are updated (duplicates summed first); every other row keeps p and its slots
 * bit for bit — momentum does not coast, u does not decay, Ftrl's shrinkage is not applied: TensorFlow's sparse apply, a
 * deviation from the dense formulas of the kind of Adam's lazy rows.                                                         */
int dt_sgdm_dense_step(float* p, const float* g, float* mom, int64_t n, float lr, float momentum, int nesterov, void* state,
                       int advance, void* stream);
int dt_sgdm_multi_step(int count, float* const* p, const float* const* g, float* const* mom, const int64_t* n, float lr,
                       float momentum, int nesterov, void* state, int advance, void* stream);
int dt_sgdm_rows_step(float* table, float* mom, const int64_t* rows, float* values, int64_t n_rows, int D, int fields,
                      void* slots, int64_t n_slots, int* mark, float lr, float momentum, int nesterov, void* state,
                      float* dense_p, const float* dense_g, float* dense_mom, int64_t dense_n, int advance, int slot_stride,
                      void* stream);
int dt_adamax_dense_step(float* p, const float* g, float* m, float* u, int64_t n, float lr, float beta1, float beta2,
                         float eps, void* state, int advance, void* stream);
int dt_adamax_multi_step(int count, float* const* p, const float* const* g, float* const* m, float* const* u,
                         const int64_t* n, float lr, float beta1, float beta2, float eps, void* state, int advance,
                         void* stream);
int dt_adamax_rows_step(float* table, float* m, float* u, const int64_t* rows, float* values, int64_t n_rows, int D,
                        int fields, void* slots, int64_t n_slots, int* mark, float lr, float beta1, float beta2, float eps,
                        void* state, float* dense_p, const float* dense_g, float* dense_m, float* dense_u, int64_t dense_n,
                        int advance, int slot_stride, void* stream);
int dt_ftrl_dense_step(float* p, const float* g, float* accum, float* linear, int64_t n, float lr, float lr_power, float l1,
                       float l2, float l2_shrinkage, void* state, int advance, void* stream);
int dt_ftrl_multi_step(int count, float* const* p, const float* const* g, float* const* accum, float* const* linear,
                       const int64_t* n, float lr, float lr_power, float l1, float l2, float l2_shrinkage, void* state,
                       int advance, void* stream);
int dt_ftrl_rows_step(float* table, float* accum, float* linear, const int64_t* rows, float* values, int64_t n_rows, int D,
                      int fields, void* slots, int64_t n_slots, int* mark, float lr, float lr_power, float l1, float l2,
                      float l2_shrinkage, void* state, float* dense_p, const float* dense_g, float* dense_accum,
                      float* dense_linear, int64_t dense_n, int advance, int slot_stride, void* stream);

/* ---- Keras Dense (deepnets.dnn deepnets.py:401-427; Dense(1) logits / task_output deepmodel.py:291-292,455;
 *      Q/K/V/residual projections layers.py:104-108) --------------------------------------------------- *
 *   y [N,M] = act(x [N,K] . W [K,M] + bias [M]|NULL),  act in {DT_ACT_LINEAR, DT_ACT_RELU}.
 *   fp32 MFMA for M >= 2, one-wave-per-row GEMV for M == 1 (vendor GEMMs pick pathological tiles at these
 *   shapes, see profiles/).  Backward: G = grad_y * act'(y); grad_x = G W^T (may be NULL), grad_W += x^T G and
 *   grad_b += colsum(G) are ACCUMULATED (zero them first); ws: dt_dense_workspace_bytes(N,K,M) bytes.        */
int dt_dense_supported(int N, int K, int M);
int64_t dt_dense_workspace_bytes(int N, int K, int M);
/* the launch geometry, for tests and tools that have to reach one launch path, from the helpers the launches use.  product:
 *   0 forward, 1 grad_x (M >= 2): out = {column waves NBW, rows per block, grid, dynamic LDS bytes, pipelined 16-step chunks,
 *     trips of the guarded remainder loop (an odd row length's last step included), 1 where the row length permits 16-byte
 *     staging loads (the launch also asks for 16-byte aligned pointers), 0};
 *   2 grad_W (M >= 2): out = {32 x 32 tiles, batch splits, rows per split, 0...};
 *   3 Dense(1) forward: out = {grid, 0...};   4 Dense(1) backward: out = {rows per block, blocks, blocks of the reduce, 0...}.
 * out: HOST int[8]; no launch; DT_ERR_UNSUPPORTED outside dt_dense_supported or for a product of the other M */
int dt_dense_geometry(int N, int K, int M, int product, int* out);
int dt_dense_fwd(const float* x, const float* W, const float* bias, int act, int N, int K, int M, float* y,
                 void* stream);
int dt_dense_bwd(const float* x, const float* W, const float* y, const float* grad_y, int act, int N, int K,
                 int M, float* grad_x, float* grad_W, float* grad_b, void* ws, void* stream);

/* ---- Keras Dense, tiled: every 2-D shape with M >= 2 (the tower's first Dense deepnets.py:401-427 at K = 1,677; FGCNN's
 *      recombination Dense layers.py:161-242 at 2,912 -> 832; FiBiNet's tower deepnets.py:374-386 at K = 10,413) ---- *
 *   The same contract as dt_dense_fwd / dt_dense_bwd (grad_x OVERWRITTEN, may be NULL; grad_W / grad_b ACCUMULATED,
 *   grad_b may be NULL) for the shapes dt_dense_supported refuses: fixed 128 x 128 / 64 x 64 output tiles on the same
 *   exact-fp32 MFMA, the contraction walked in steps of 32 through double-buffered LDS panels, so neither K nor M is
 *   bounded (csrc/dense_tiled.hip).  dt_dense_tiled_supported: 1 for N > 0, K > 0, M >= 2 (M == 1 stays with the GEMV
 *   kernels of dt_dense_*).  ws: dt_dense_tiled_workspace_bytes(N,K,M) bytes — 0 today, ws may then be NULL.          */
int dt_dense_tiled_supported(int N, int K, int M);
int64_t dt_dense_tiled_workspace_bytes(int N, int K, int M);
/* the launch geometry, for tests and tools that have to reach one tile size or one batch split: product = 0 forward
 * (N x M output), 1 grad_x (N x K), 2 grad_W (K x M); *tile = 64 or 128 (the output tile's edge), *splits = gridDim.z (1 for
 * products 0 and 1; > 1: grad_W's partial tiles merge with float atomics), *steps_per_split = contraction steps of 32 per
 * split.  HOST pointers, any may be NULL; no launch; DT_ERR_UNSUPPORTED outside dt_dense_tiled_supported */
int dt_dense_tiled_geometry(int N, int K, int M, int product, int* tile, int* splits, int* steps_per_split);
int dt_dense_tiled_fwd(const float* x, const float* W, const float* bias, int act, int N, int K, int M, float* y,
                       void* stream);
int dt_dense_tiled_bwd(const float* x, const float* W, const float* y, const float* grad_y, int act, int N, int K,
                       int M, float* grad_x, float* grad_W, float* grad_b, void* ws, void* stream);

/* ---- Keras Dense, tiled, on the bf16 matrix cores (csrc/dense_tiled_x3.hip): the contract, the shape domain and the tile
 *      rule of dt_dense_tiled_*, with the operands split into bf16 parts while they are staged into LDS (nothing pre-split
 *      is written to HBM; fp32 tensors, fp32 accumulation).  mode (dnn_params / fgcnn_params['dense_mfma_dtype']):
 *        DT_DENSE_X3    forward: three parts per operand, six products (fp32 class: 2 x 2^-24 on cond_rms);
 *                       grad_x / grad_W: two parts, three products (2^-17 per product)
 *        DT_DENSE_BF16  one bf16 product everywhere (north_star's 1e-2 mode)
 *      grad_b is an fp32 column sum of G in both modes; the relu mask reads the stored fp32 y.  A non-finite operand
 *      poisons the row / column the fp32 kernel would poison and nothing else (its low parts are zero, not inf - inf).
 *   dt_dense_x3_supported: 1 for a known mode and N > 0, K > 0, M >= 2.  ws: dt_dense_x3_workspace_bytes(N,K,M,mode)
 *   bytes — 0 today, ws may then be NULL.  Validation as dt_dense_tiled_*; an unknown mode is DT_ERR_INVALID_ARG.      */
#define DT_DENSE_X3 1
#define DT_DENSE_BF16 2
int dt_dense_x3_supported(int N, int K, int M, int mode);
int64_t dt_dense_x3_workspace_bytes(int N, int K, int M, int mode);
/* the launch geometry: product = 0 forward (N x M output), 1 grad_x (N x K), 2 grad_W (K x M); *tile_rows x *tile_cols =
 * the output tile (64 x 64 or 128 x 128), *splits = gridDim.z (1 for products 0 and 1; > 1: grad_W's partial tiles merge
 * with float atomics), *steps_per_split = contraction steps of 32 per split.  HOST pointers, any may be NULL; no launch;
 * computed by the helper the launches use; DT_ERR_UNSUPPORTED outside dt_dense_x3_supported */
int dt_dense_x3_geometry(int N, int K, int M, int mode, int product, int* tile_rows, int* tile_cols, int* splits,
                         int* steps_per_split);
int dt_dense_x3_fwd(const float* x, const float* W, const float* bias, int act, int N, int K, int M, float* y, int mode,
                    void* ws, void* stream);
int dt_dense_x3_bwd(const float* x, const float* W, const float* y, const float* grad_y, int act, int N, int K, int M,
                    float* grad_x, float* grad_W, float* grad_b, int mode, void* ws, void* stream);

/* ---- FGCNN block, training: Conv2D((h,1), 'same') -> activation -> MaxPooling2D((pool,1), 'same') of FGCNN.call
 *      (layers.py:161-242, the three layers at :220-225) in one launch each way (csrc/fgcnn_train.hip) ------------------ *
 *   All tensors contiguous fp32, channels-last: x [B][F][D][C], kernel in the Keras layout [h][1][C][filters], bias
 *   [filters] | NULL, pooled [B][Fp][D][filters] with Fp = ceil(F / pool).
 *     z[b,f,d,o] = bias[o] + sum_{t<h, c<C} x[b, f+t-pb, d, c] kernel[t][c][o], pb = (h-1)/2, taps beyond the map are zero
 *     window i = fields [i pool - qb, i pool - qb + pool) inside the map, qb = (Fp pool - F) / 2
 *     pooled[b,i,d,o] = act(max_f z) (the activations of the domain are non-decreasing: one activation per window); ties
 *     go to the first field; a NaN pre-activation makes the window's maximum NaN (as torch.amax).  sel [B][Fp][D][filters], one byte each = the offset of the selected field inside its window;
 *     sel == NULL (no gradient needed): not stored.
 *   Backward: dz = grad_pooled act'(pooled) at the selected field of each window (act' as listed beside DT_ACT_*), 0
 *     elsewhere; grad_x[b,g,d,c] = sum_{t,o} dz[b,g-t+pb,d,o] kernel[t][c][o] (NULL: skipped), grad_kernel[t][c][o] =
 *     sum_{b,f,d} x[b,f+t-pb,d,c] dz[b,f,d,o], grad_bias[o] = sum dz (NULL: skipped) — all three OVERWRITTEN.  The batch
 *     reduction uses no float atomics: every block stores its partial sums into `workspace`
 *     (dt_fg_conv_pool_workspace_bytes bytes, -1 outside the domain) and a second launch on the same stream adds them in
 *     block order, so the result is bit-identical from run to run.  Plain fp32 FMAs with fp32 accumulation (the partials
 *     are added in double): the exact fp32 class both ways.
 *   Domain (dt_fg_conv_pool_supported): 1 <= C, filters, h <= 16, 1 <= pool <= 8, F >= 1, D >= 1 (any D), act in
 *     {DT_ACT_LINEAR, DT_ACT_RELU, DT_ACT_SIGMOID, DT_ACT_TANH}, and one batch row's map plus its dz fit the LDS tile beside
 *     the padded kernel, in bytes:  64 h CP + 64 + F D (4 (C | 1) + 80) <= 65536 with CP = C rounded up to a multiple of 4.
 *   B = 0 launches nothing and looks at no pointer; a shape outside the domain is DT_ERR_UNSUPPORTED, a null pointer
 *   DT_ERR_INVALID_ARG, both before the first launch.  No alignment beyond that of a float is relied on.  (The names
 *   start with dt_fg_conv_: the dt_fgcnn_ prefix is the inference family's, dt_fgcnn_infer*, alone.)                    */
int dt_fg_conv_pool_supported(int F, int D, int C, int filters, int h, int pool, int act);
int64_t dt_fg_conv_pool_workspace_bytes(int64_t B, int F, int D, int C, int filters, int h, int pool);
/* the launch geometry, for tests and tools that have to reach the grid-stride loops: *tile_rows = the batch rows of one
 * tile of the forward (backward = 0) or backward (backward != 0) launch, *max_blocks = the cap of either grid (a launch has
 * min(ceil(B / tile_rows), max_blocks) blocks); HOST pointers, either may be NULL; DT_ERR_UNSUPPORTED outside the domain */
int dt_fg_conv_pool_geometry(int F, int D, int C, int filters, int h, int pool, int backward, int* tile_rows,
                             int* max_blocks);
int dt_fg_conv_pool_fwd(const float* x, const float* kernel, const float* bias, int64_t B, int F, int D, int C,
                           int filters, int h, int pool, int act, float* pooled, uint8_t* sel, void* stream);
int dt_fg_conv_pool_bwd(const float* x, const float* kernel, const float* pooled, const uint8_t* sel,
                           const float* grad_pooled, int64_t B, int F, int D, int C, int filters, int h, int pool, int act,
                           float* grad_x, float* grad_kernel, float* grad_bias, void* workspace, void* stream);

/* ---- CIN layer, bf16-MFMA mode (opt-in; north_star "logits within 1e-2 bf16") --------------------------------------- *
 * Same contract as dt_cin_layer_fwd / dt_cin_layer_bwd, computed on v_mfma_f32_32x32x16_bf16 (bf16 operands, fp32
 * accumulation): results within 1e-2 of the float64 oracle instead of 1e-4.  ws: dt_cin_bf16_workspace_bytes(F0, Hk, L)
 * bytes (bf16 re-layouts of W, rebuilt by every call).  L <= 256, Hk <= 128, F0 <= 128.  dt_cin_layer_bwd_bf16 OVERWRITES
 * grad_x0 / grad_xk (no zero fill needed, as dt_cin_layer_bwd_ws); grad_W / grad_bias accumulate as in dt_cin_layer_bwd. */
int64_t dt_cin_bf16_workspace_bytes(int F0, int Hk, int L);
int dt_cin_layer_fwd_bf16(const float* x0, const float* xk, const float* W, const float* bias, int act, int B, int F0,
                          int Hk, int L, int D, int64_t x0_bstride, int64_t xk_bstride, float* y, void* ws, void* stream);
int dt_cin_layer_bwd_bf16(const float* x0, const float* xk, const float* W, const float* y, const float* grad_y, int act,
                          int B, int F0, int Hk, int L, int D, int64_t x0_bstride, int64_t xk_bstride, float* grad_x0,
                          float* grad_xk, float* grad_W, float* grad_bias, void* ws, void* stream);
/* ---- CIN layer, SPLIT-bf16 mode (cin_params['mfma_dtype'] = 'bf16x3'): the same contract and kernels with every fp32 operand
 * split into bf16 parts and the partial products on v_mfma_f32_32x32x16_bf16, fp32 accumulate — forward: three parts (all 24
 * mantissa bits), six products, fp32-class outputs and relu decisions; backward: two parts, three products (2^-17 per
 * product).  Held to the exact kernels' bars (1e-4 / 2e-4 against the float64 oracle).  ws: dt_cin_bf16x3_workspace_bytes. */
int64_t dt_cin_bf16x3_workspace_bytes(int F0, int Hk, int L);
int dt_cin_layer_fwd_bf16x3(const float* x0, const float* xk, const float* W, const float* bias, int act, int B, int F0,
                            int Hk, int L, int D, int64_t x0_bstride, int64_t xk_bstride, float* y, void* ws, void* stream);
int dt_cin_layer_bwd_bf16x3(const float* x0, const float* xk, const float* W, const float* y, const float* grad_y, int act,
                            int B, int F0, int Hk, int L, int D, int64_t x0_bstride, int64_t xk_bstride, float* grad_x0,
                            float* grad_xk, float* grad_W, float* grad_bias, void* ws, void* stream);

/* ---- AutoInt interacting layer (MultiheadAttention.call, layers.py:119-153) minus its BatchNormalization -------- *
 * x [B,F,D]; Wq/Wk/Wv/Wr [D,D] and bq/bk/bv/br [D]: kernels / biases of dense_Q, dense_K, dense_V, dense_residual
 * (Wr = br = NULL: use_residual False).  Forward: a [B,F,D] = relu(concat_h(softmax(Q_h K_h^T/sqrt(d_h)) V_h) + R) with
 * Q,K,V,R = relu(x W + b); nothing else is written (lse may be NULL; [B,H,F] log-sum-exp when given).
 * Backward: g = gradient w.r.t. a, a = the forward output.  Outputs, each optional (NULL = not produced):
 *   dX [B,F,D]; dY [B,F,NP*D] = gradient w.r.t. the PRE-activations of q | k | v [| residual] (NP = 4 or 3), from which
 *   dt_dense_bwd(x, ., ., dY, DT_ACT_LINEAR, .., grad_x = NULL) forms the kernel / bias gradients (batch reductions).
 * bn_mean != NULL: g is the gradient w.r.t. the layer's BatchNormalization output y = BN(a) (layers.py:151) and the BN
 * backward is applied while g is read: bn_gamma [D] (NULL = 1), bn_mean / bn_rstd [D] the saved batch statistics, bn_sums
 * [2D] = sum_g | sum_gx from dt_bn_train_bwd_stats.
 * dropout_rate: Dropout on the attention weights (layers.py:141), keep-mask = dt_autoint_dropout_hash(seed, b, h,
 * query, key) >= rate * 2^32, kept weights scaled by 1/(1-rate); pass 0 at inference.  fp32 MFMA (16x16x4); F <= 32,
 * D in {16, 32}, d_h in {4, 8, 16} (dt_autoint_supported); other shapes: dt_dense_fwd + dt_mha_core_fwd.
 * mfma_mode (every entry point of the layer; autoint_params['mfma_dtype']): DT_AI_F32 — exact fp32 MFMA throughout;
 * DT_AI_BF16 (D = 32) — north_star's "1e-2 bf16" mode: the projection-shaped products on v_mfma_f32_16x16x32_bf16 with fp32
 * accumulation — x Wcat (and its recomputation in the backward) with two-part operands (three products, 2^-17: the relu
 * decisions stay the oracle's), dX = dY Wcat^T and the weight gradient x^T dY with plain bf16 operands; scores, softmax and
 * BatchNormalization stay fp32.  Results within 1e-2 of the oracle (of each tensor's largest entry). */
/* prev_a / prev_mean / prev_rstd / prev_sums (dt_autoint_bwd, dt_autoint_bwd_w; all NULL = off): when this layer's input x is
 * y_prev = BatchNormalization(a_prev) of the interacting layer below it (deepnets.py:219-221 stacks them), the two batch sums
 * of THAT BatchNormalization's backward — sum_b dX and sum_b dX xhat_prev per channel, what dt_bn_train_bwd_stats(a_prev, dX)
 * computes — are added (doubles) into prev_sums [2 D] = sum_g | sum_gx while dX leaves; the caller zeroes prev_sums first. */
/* xn_mean / xn_rstd / xn_gamma / xn_beta [D] (every entry point of the layer that reads x; xn_mean = NULL: off; xn_gamma /
 * xn_beta may be NULL = 1 / 0): x is handed over UN-normalised — x = a_prev, the output of the interacting layer below BEFORE
 * its BatchNormalization — and normalised while it is loaded, x_used = (x - mean) rstd gamma + beta.  The layer below is then
 * called with dt_autoint_fwd_bn(out_y = NULL): its statistics are finished, its normalised output is never written.  dX stays
 * the gradient w.r.t. the NORMALISED input (what the layer below's backward expects as g with bn_mean set); with prev_a, pass
 * prev_a = x, prev_mean = xn_mean, prev_rstd = xn_rstd. */
#define DT_AI_F32 0
#define DT_AI_BF16 1
/* DT_AI_BF16X2 (D = 32): split-bf16 — three-part operands (all 24 mantissa bits, six products) in x Wcat and its
 * recomputation, two-part operands (16 bits, three products) in dX and the weight gradient: held to the exact kernels' bars
 * (2e-5 forward, 1e-4 gradients against the float64 oracle) at 6/16 resp. 3/16 of the fp32-MFMA time of those products. */
#define DT_AI_BF16X2 2
int dt_autoint_supported(int F, int D, int H);
unsigned dt_autoint_dropout_hash(unsigned seed, unsigned b, unsigned h, unsigned i, unsigned j);
/* the keep threshold of the layer's and of dt_mha_core's attention dropout: float32(rate) * 2^32 saturated to 2^32 - 1, at
 * least 1 for a rate > 0; 0 for rate <= 0 (no dropout) */
unsigned dt_autoint_dropout_threshold(float rate);
int dt_autoint_fwd(const float* x, const float* Wq, const float* Wk, const float* Wv, const float* Wr, const float* bq,
                   const float* bk, const float* bv, const float* br, int64_t B, int F, int D, int H,
                   float dropout_rate, unsigned seed, float* out_a, float* lse, const float* xn_mean, const float* xn_rstd,
                   const float* xn_gamma, const float* xn_beta, int mfma_mode, void* stream);
int dt_autoint_bwd(const float* x, const float* Wq, const float* Wk, const float* Wv, const float* Wr, const float* bq,
                   const float* bk, const float* bv, const float* br, const float* a, const float* g, int64_t B, int F,
                   int D, int H, float dropout_rate, unsigned seed, const float* bn_gamma, const float* bn_mean,
                   const float* bn_rstd, const float* bn_sums, float* dY, float* dX, const float* prev_a, const float* prev_mean,
                   const float* prev_rstd, double* prev_sums, const float* xn_mean, const float* xn_rstd,
                   const float* xn_gamma, const float* xn_beta, int mfma_mode, void* stream);
/* dt_autoint_fwd_bn — dt_autoint_fwd followed by the layer's training-mode BatchNormalization (layers.py:151) in two
 * launches instead of four: the attention kernel's epilogue leaves per-block sums of (a - moving_mean) and its square, the
 * second launch adds them up in its prologue, normalises (out_y = BN(out_a)), writes save_mean / save_rstd [D] for the
 * backward and moves moving_mean / moving_var (Keras: moving = moving * momentum + batch * (1 - momentum), biased batch
 * variance).  workspace: dt_autoint_fwd_bn_workspace_bytes(B, D) bytes.
 * out_y = NULL: statistics only (one block finishes them) — for a layer whose consumer normalises on load (xn_* above).
 * zero_sums [2 D] doubles (may be NULL): zeroed by the second launch — the accumulators the layer above will pass as prev_sums. */
int64_t dt_autoint_fwd_bn_workspace_bytes(int64_t B, int D);
int dt_autoint_fwd_bn(const float* x, const float* Wq, const float* Wk, const float* Wv, const float* Wr, const float* bq,
                      const float* bk, const float* bv, const float* br, int64_t B, int F, int D, int H,
                      float dropout_rate, unsigned seed, const float* gamma, const float* beta, float eps, float momentum,
                      float* moving_mean, float* moving_var, float* out_a, float* out_y, float* save_mean,
                      float* save_rstd, void* workspace, const float* xn_mean, const float* xn_rstd, const float* xn_gamma,
                      const float* xn_beta, double* zero_sums, int mfma_mode, void* stream);
/* dt_autoint_bwd_w — the same backward with the kernel / bias gradients of dense_Q | dense_K | dense_V [| dense_residual]
 * (layers.py:104-108; in the reference: four MatMul + BiasAddGrad ops over [B*F, D]) accumulated inside the launch from the
 * pre-activation gradients while they are in LDS, plus one small reduction launch: dY never reaches HBM and no
 * dt_dense_bwd follows.  gW [NP][D][D] (the Keras kernels' layout, one after the other), gb [NP][D]: OVERWRITTEN.
 * F <= 28.  workspace: dt_autoint_bwd_workspace_bytes(B, D) bytes (per-block partials).
 * bn_sums_f64 [2 D] (may be NULL; then bn_sums is used): the BatchNormalization-backward sums as the DOUBLES the layer above
 * left in its prev_sums — read as they are, no conversion launch; bn_grads [2 D] (may be NULL): the same two sums as floats =
 * the gradients of beta | gamma, written by the reduction launch.
 * g_rank1_w [F D] (may be NULL): the incoming gradient is rank one — g is then [B] (one value per batch row) and
 * dL/dy[b][i][c] = g[b] g_rank1_w[i D + c]: the layer's flattened output feeds a single Dense(1) (dt_autoint_head_*). */
int64_t dt_autoint_bwd_workspace_bytes(int64_t B, int D);
int dt_autoint_bwd_w(const float* x, const float* Wq, const float* Wk, const float* Wv, const float* Wr, const float* bq,
                     const float* bk, const float* bv, const float* br, const float* a, const float* g, int64_t B, int F,
                     int D, int H, float dropout_rate, unsigned seed, const float* bn_gamma, const float* bn_mean,
                     const float* bn_rstd, const float* bn_sums, float* dX, float* gW, float* gb, void* workspace,
                     const float* prev_a, const float* prev_mean, const float* prev_rstd, double* prev_sums,
                     const float* xn_mean, const float* xn_rstd, const float* xn_gamma, const float* xn_beta,
                     const double* bn_sums_f64, float* bn_grads, const float* g_rank1_w, int mfma_mode, void* stream);
/* dt_autoint_head_* — the head of the AutoInt graph, BatchNormalization(top interacting layer) -> Flatten -> Dense(1)
 * (deepnets.py:222-224, deepmodel.py:131-143 `task_output` / `dense_logit_*`), without the normalised tensor: a [B, K = F D]
 * is the top layer's UN-normalised output (dt_autoint_fwd_bn with out_y = NULL), xn_* its pending normalisation (as above),
 * w [K] / bias [1] (may be NULL) the Dense(1).  fwd: z [B] = (s a + t) . w + bias.  bwd: gz [B] = gradient w.r.t. z; gW [K],
 * gb [1] (may be NULL): OVERWRITTEN; bn_sums [2 D] doubles: the two batch sums of the pending normalisation's backward for
 * dL/dy = gz w are ADDED (zero before the step: dt_autoint_fwd_bn's zero_sums) — the top layer's backward is then dt_autoint_bwd_w(g = gz, g_rank1_w = w, bn_sums_f64 = bn_sums) and no
 * [B,F,D] gradient tensor exists.  K <= 1024, D divides 64 and K; workspace: dt_autoint_head_workspace_bytes(B, K) bytes. */
int64_t dt_autoint_head_workspace_bytes(int64_t B, int K);
int dt_autoint_head_fwd(const float* a, const float* w, const float* bias, const float* xn_mean, const float* xn_rstd,
                        const float* xn_gamma, const float* xn_beta, int64_t B, int K, int D, float* z, void* stream);
int dt_autoint_head_bwd(const float* a, const float* w, const float* gz, const float* xn_mean, const float* xn_rstd,
                        const float* xn_gamma, const float* xn_beta, int64_t B, int K, int D, float* gW, float* gb,
                        double* bn_sums, void* workspace, void* stream);

/* ---- input feed: batch assembly on the device (replaces `tf.data.Dataset.from_tensor_slices(...).shuffle().batch()` of
 *      utils/dataset_generator.py:36-72 for a table resident in HBM; deeptables_amd/compiled.py) -------------------- *
 * n_rows rows named by sel (int64 indices into every source block) are copied from each of n_blocks row-major blocks into
 * the matching destination: dst[b][i, :] = src[b][sel[i], :].  src / dst / row_bytes are HOST arrays (n_blocks <= 8 entries;
 * device pointers, bytes per row, multiples of 4): ONE launch assembles the ids, the continuous columns and the labels
 * (+ weights) of k train steps.  cursor (DT_FEED_CURSOR_WORDS device int64 words, zero-initialised; may be NULL): the rows
 * are sel[cursor[0] + i] and cursor[0] advances by n_rows behind the gather (the last block to finish does it; the other
 * words are the blocks' arrival tickets, zero again when the call's launch ends) — `sel` is then the epoch's whole row
 * order and a captured hipGraph of the call walks it by itself, replay after replay, with no host work in between.   */
#define DT_FEED_CURSOR_WORDS 528
int dt_feed_gather(const int64_t* sel, int64_t n_rows, int n_blocks, const void* const* src, void* const* dst,
                   const int* row_bytes, int64_t* cursor, void* stream);

/* ---- model-parallel tables: owner-side gather (parallel.ShardedEmbeddingStrategy; the role the sharded
 *      embedding_lookup of a parameter-server strategy plays) ------------------------------------------- *
 * idx_all [W,B,F] ids of all W minibatches; this rank owns fields [f_begin, f_end) of the packed table.
 * out [W, F_own, B, D] (each rank's piece contiguous, field-major), rows_out [W, F_own, B] packed rows (-1 = id out
 * of range -> zero row).                                                                                 */
int dt_embedding_gather_owned(const void* idx_all, int idx_kind, const float* table, const int64_t* row_offset,
                              const int32_t* vocab, int W, int B, int F, int f_begin, int f_end, int D, float* out,
                              int64_t* rows_out, int* oob_count, void* stream);

/* ---- f3: AFM attention pooling (AFM.call layers.py:789-807) ---------------------------------------- *
 * x [B,F,D]; P = F(F-1)/2 pairs in itertools.combinations order (layers.py:790-795).
 *   bi[p] = x_i*x_j ; a = act(bi . Wa [D,H] + ba [H]|NULL) (dense_attention, layers.py:776-778) ;
 *   score = softmax_p(a . pv [H]) (layers.py:799-800) ; out [B,D] = sum_p score[p] bi[p] (layers.py:801).
 * score [B,P] is saved for the backward.  The trailing Dropout + Dense(1) (layers.py:803-806) are host
 * layers.  Parameter gradients are ACCUMULATED (zero them first).                                      */
int dt_afm_fwd(const float* x, const float* Wa, const float* ba, const float* pv, int act, int B, int F, int D,
               int H, float* out, float* score, void* stream);
int dt_afm_bwd(const float* x, const float* Wa, const float* ba, const float* pv, const float* score,
               const float* grad_out, int act, int B, int F, int D, int H, float* grad_x, float* grad_Wa,
               float* grad_ba, float* grad_pv, void* stream);

/* ---- f3: BilinearInteraction (FiBiNet; layers.py:363-377) --------------------------------------- *
 * out [B,P,D]: out[b,p,:] = (x_i . W_q) * x_j with W [nW,D,D]:
 *   wtype 0 'field_interaction' q = p (nW = P), 1 'field_each' q = i (nW = F-1, layers.py:352-354),
 *   2 'field_all' q = 0 (nW = 1).  grad_W is ACCUMULATED.                                              */
int dt_bilinear_fwd(const float* x, const float* W, int wtype, int B, int F, int D, float* out, void* stream);
int dt_bilinear_bwd(const float* x, const float* W, const float* grad_out, int wtype, int B, int F, int D,
                    float* grad_x, float* grad_W, void* stream);

/* ---- f3: SENET squeeze / re-weight (layers.py:291-302) --------------------------------------------- *
 * pool: z [B,F] = mean_d x (use_max 0) | max_d x (use_max 1, argmax [B,F] saved: first maximum wins, as
 * the gradient of tf.reduce_max on ties is not used by the parity tests); scale: out = x * a[:, :, None]. */
int dt_field_pool_fwd(const float* x, int B, int F, int D, int use_max, float* z, int* argmax, void* stream);
int dt_field_pool_bwd(const float* grad_z, const int* argmax, int B, int F, int D, int use_max, float* grad_x,
                      void* stream);
int dt_field_scale_fwd(const float* x, const float* a, int B, int F, int D, float* out, void* stream);
int dt_field_scale_bwd(const float* x, const float* a, const float* grad_out, int B, int F, int D, float* grad_x,
                       float* grad_a, void* stream);

/* ---- fused DeepFM train step (nets ['linear','fm_nets','dnn_nets'], deepnets.py:15) ------------- *
 * The graph DeepModel.__build_model assembles for DeepFM (deepmodel.py:259-317) — embedding gather,
 * concat + BatchNormalization('bn_concat_emb_dense'), linear, FM, Dense(128)-relu-Dense(64)-relu,
 * the per-net Dense(1) logits, Add, Dense(1) output, BinaryCrossentropy (from logits, mean over B)
 * — forward AND backward in the launches csrc/deepfm.hip's header lists (A, prep, C, E||D, finish).  Hidden sizes are fixed to the
 * ModelConfig default dnn_params ((128,0,False),(64,0,False)), relu; dt_deepfm_supported() says
 * whether a shape is covered (else the host uses the per-layer entry points above).
 *   W1 [C,128] b1 [128] W2 [128,64] b2 [64] w3 [64] (dense_logit_dnn_nets) w_out [1] b_out [1]|NULL
 *   w_lin [F+Nd] (linear_logit), bn_* [C] with C = F*D+Nd.
 * Outputs: logit_out [B]; rows_out [B,F] + grad_rows [B,F,D] = the embedding table's sparse gradient
 * (IndexedSlices indices/values); accum: dt_deepfm_accum_floats() floats holding every dense gradient
 * and the mean loss at the offsets reported by dt_deepfm_accum_offsets() in the order
 * dW1, dW2, db1, db2, dw3, dw_out, db_out, loss, dgamma, dbeta, dw_lin (zeroed by the call).
 * phases: 1 = forward only (logits + loss), 2 = forward + backward; OR-ed with DT_STEP_LOSS_MSE the loss is
 * MeanSquaredError on the linear output (regression task, deepmodel.py:130-131) instead of BinaryCrossentropy.
 * dedupe_ws (may be NULL; 16-byte aligned): dt_deepfm_dedupe_bytes(B,F) bytes of scratch, zero-filled once before
 * its first use; dedupe_slots = dt_deepfm_dedupe_slots(B,F).  When given (and phases == 2) the step
 * resolves duplicate lookups itself: a table row
 * looked up ONCE keeps its (rows_out, grad_rows) entry; a row looked up several times becomes a SEGMENT — every one of
 * its lookups reports -1 in rows_out (their grad_rows entries still hold the per-lookup gradients) and the segment
 * arrays inside dedupe_ws (dt_deepfm_dedupe_segments -> byte offsets of nseg, seg_row, seg_off, seg_cnt, seg_list,
 * then the number of regions and their capacity) say which grad_rows entries to sum for which row.
 * dt_adam_rows_step_seg consumes exactly that (fields = -1: no dedupe pass).
 * grad_rows_field_major != 0 (model-parallel tables, no dedupe_ws): grad_rows is written as [F,B,D] and multiplied
 * by grad_rows_scale (1/world size), ready for the all-to-all back to the row owners.
 * phases | DT_STEP_SKIP_FINISH: a backward step without its LAST launch (the last level of the dense gradients): every
 * row gradient is final when the call's launches are, so the collective that carries them to the row owners can start
 * there; the same call with phases | DT_STEP_FINISH_ONLY (same arguments) then issues only that last launch, which runs
 * beside the collective.  accum is complete after the second call.
 * phases | DT_STEP_TOWER_X3 (backward steps of dt_deepfm_train_step / dt_dcn_train_step / _adam): the Dense tower's four GEMMs of the tile kernel
 * (Dense128, Dense64, dH1 = dH2 W2^T, dXn = dH1 W1^T; deepnets.py:401-427) run on v_mfma_f32_16x16x32_bf16 with SPLIT
 * operands and fp32 accumulation (csrc/tower_x3.h): forward a = a1 + a2 + a3 (three bf16 parts = all 24 mantissa bits,
 * six products, the dropped terms 2^-24 of the product: fp32-class logits and relu decisions), backward a = a_hi + a_lo
 * (16 bits, three products, 2^-17 per product).  6/16 resp. 3/16 of the fp32-MFMA time.  Weights are split once per step
 * by the prep launch, activations while they are staged.
 * phases | DT_STEP_TOWER_BF16 (north_star's "1e-2 bf16" mode for the tower; backward steps, DeepFM and DCN): the same kernel
 * with ONE bf16 product per operand pair — plain bf16 operands, fp32 accumulation; logits and gradients within 1e-2 of the
 * float64 oracle (of each tensor's largest entry) instead of 1e-4.  The Cross network's scalar recurrences keep six products.
 * phases | DT_STEP_PREELECTED: rows_out and dedupe_ws were filled for THIS idx by dt_deepfm_preelect — the step's ids-only
 * work (packed rows of the lookups, the election of the rows looked up several times) ran ahead of it, on another stream or at
 * an earlier point of a captured graph (deeptables_amd/compiled.py: the elections of steps 2..k of an execution run beside
 * step 1), and is left out of the step's gather and prep launches.                                                */
#define DT_STEP_LOSS_MSE 0x10
#define DT_STEP_SKIP_FINISH 0x20
#define DT_STEP_FINISH_ONLY 0x40
#define DT_STEP_TOWER_X3 0x80
#define DT_STEP_PREELECTED 0x100
#define DT_STEP_TOWER_BF16 0x200
/* phases | DT_STEP_STAMPS (diagnostic): wave 0 of every block of the step's kernels writes s_memtime phase stamps into the
 * workspace region at dt_deepfm_stamps_offset_floats() (tools/phase_times.py reads them back).  The library reads no
 * environment variables: every switch of a call is in its arguments. */
#define DT_STEP_STAMPS 0x400
/* Chained steps (dt_deepfm_train_step_adam / dt_dcn_train_step_adam, dt_deepfm_step_chains() == 1): a step given the NEXT
 * step's ids (next_idx, the same kind and shape as idx; next_rows_out / next_dedupe_ws: that step's own buffers) does the
 * next step's ids-only and weight-only work inside its own launches — kernel A packs the next ids' table rows, the
 * weight-gradient launch's matrix waves run the next election in their idle time, the finishing launch writes the tile
 * kernel's bf16 weight layouts from the weights it has just updated.  The next call then passes phases | DT_STEP_PREPARED
 * with idx = that next_idx, rows_out = that next_rows_out, dedupe_ws = that next_dedupe_ws and the same workspace, and runs
 * FOUR launches (no prep launch).  Nothing may touch the dense weights or the two buffers between the two calls.
 * deeptables_amd/compiled.py chains the k steps of one captured execution this way; the first step of an execution prepares
 * itself (five launches).  Keras' steps_per_execution is the reference's counterpart (deepmodel.py:319-346). */
#define DT_STEP_PREPARED 0x800
int dt_deepfm_step_chains(int B, int F, int D, int Nd, int phases);
int dt_deepfm_preelect(const void* idx, int idx_kind, const int64_t* row_offset, const int32_t* vocab, int B, int F,
                       int64_t* rows_out, void* dedupe_ws, int64_t dedupe_slots, void* stream);
int64_t dt_deepfm_dedupe_slots(int B, int F);
int64_t dt_deepfm_dedupe_bytes(int B, int F);
int dt_deepfm_dedupe_segments(int B, int F, int64_t* out7_host);
/* Byte offset inside dedupe_ws of an int32 that counts the lookups whose election block found its 8192-slot table full
 * (possible only for B > 8192 and > 8192 distinct rows of one field in one of its B / 1024 hash partitions; such a lookup is
 * updated as if its row were looked up once).  dedupe_ws must be ZERO-FILLED once before its first use; the counter only
 * grows: non-zero after a step = that step's duplicate handling was incomplete.  Any batch size with B F < 2^23 is taken:
 * batches beyond 8192 rows place their segments in per-FIELD regions (dt_deepfm_dedupe_segments reports regions / capacity). */
int64_t dt_deepfm_dedupe_overflow_offset(int B, int F);
int dt_deepfm_supported(int B, int F, int D, int Nd, int H1, int H2);

/* ---- fused DCN train step (nets ['dcn_nets']: Cross || DNN on BN(concat(embeddings, dense)), deepnets.py:194-207;
 * Cross.call layers.py:428-436; the reference runs it as ~120 TF ops per step).  The same launches as
 * dt_deepfm_train_step with the Cross network's forward and backward inside the tile kernel:
 *   z = Dense(1, no bias)(Concatenate([cross(xn), relu(Dense64(relu(Dense128(xn))))])),  logit = Dense(1)(z).
 * cross_w / cross_b [L][C] = the layer's L kernels / biases stacked (L <= 8); w3 [C + 64] = the kernel applied to
 * Concatenate([cross, dnn]) (cross part first).  With 'dcn_nets' as the ONLY net the reference feeds the concatenation
 * straight into task_output (deepmodel.py:286-301): pass its kernel as w3, a constant 1 as w_out and its bias as b_out.  accum: dt_dcn_accum_floats() floats, offsets from dt_dcn_accum_offsets()
 * in the order dW1, dW2, db1, db2, dw3, dw_out, db_out, loss, dgamma, dbeta, d cross_w, d cross_b.  Everything else as
 * dt_deepfm_train_step (workspace: dt_dcn_workspace_bytes).                                                        */
int dt_dcn_supported(int B, int F, int D, int Nd, int H1, int H2, int L);
int64_t dt_dcn_workspace_bytes(int B, int F, int D, int Nd, int L);
int64_t dt_dcn_stamps_offset_floats(int B, int F, int D, int Nd, int L);   /* DT_STEP_STAMPS diagnostics */
int64_t dt_dcn_accum_floats(int F, int D, int Nd, int L);
int dt_dcn_accum_offsets(int F, int D, int Nd, int L, int64_t* out12_host);
int dt_dcn_train_step(const void* idx, int idx_kind, const float* table, const int64_t* row_offset,
                      const int32_t* vocab, const float* dense, const float* y, int B, int F, int D, int Nd,
                      const float* cross_w, const float* cross_b, int L, const float* bn_gamma, const float* bn_beta,
                      float* bn_moving_mean, float* bn_moving_var, float bn_eps, float bn_momentum, const float* W1,
                      const float* b1, const float* W2, const float* b2, const float* w3, const float* w_out,
                      const float* b_out, float* logit_out, int64_t* rows_out, float* grad_rows, float* accum,
                      void* workspace, int* oob_count, void* dedupe_ws, int64_t dedupe_slots, int phases,
                      float embedding_dropout, unsigned* dropout_seed, float dense_input_dropout,
                      const float* sample_weight, void* stream);
/* dt_dcn_train_step with the optimizer step inside — arguments and semantics as dt_deepfm_train_step_adam (dense_n = the
 * offset of d cross_b + L * C floats of the dt_dcn_accum_offsets layout). */
int dt_dcn_train_step_adam(const void* idx, int idx_kind, float* table, const int64_t* row_offset,
                           const int32_t* vocab, const float* dense, const float* y, int B, int F, int D, int Nd,
                           const float* cross_w, const float* cross_b, int L, const float* bn_gamma, const float* bn_beta,
                           float* bn_moving_mean, float* bn_moving_var, float bn_eps, float bn_momentum, const float* W1,
                           const float* b1, const float* W2, const float* b2, const float* w3, const float* w_out,
                           const float* b_out, float* logit_out, int64_t* rows_out, float* grad_rows, float* accum,
                           void* workspace, int* oob_count, void* dedupe_ws, int64_t dedupe_slots, int phases,
                           float embedding_dropout, unsigned* dropout_seed, float dense_input_dropout,
                           const float* sample_weight, float* adam_m, float* adam_v, int slot_stride,
                           void* adam_state, float lr_t, float beta1, float beta2, float eps, float* dense_p,
                           float* dense_m, float* dense_v, int64_t dense_n, float lr, const void* next_idx,
                           int64_t* next_rows_out, void* next_dedupe_ws, void* stream);
/* workspace: dt_deepfm_workspace_bytes() bytes, 16-byte aligned, ZERO-FILLED ONCE before its first use (hipMemset / torch.zeros):
 * it holds the step's batch-sum accumulators (BatchNormalization's sum x / sum x^2 per column, the tile kernel's record sums),
 * which the launches add into with double-precision atomics and hand back zeroed — a step leaves the invariant as it found it,
 * so the same workspace serves every following call (any phases) without further initialisation. */
int64_t dt_deepfm_workspace_bytes(int B, int F, int D, int Nd);
int64_t dt_deepfm_accum_floats(int F, int D, int Nd);
/* debugging aid: offset (floats) of the per-block phase timestamps written with phases | DT_STEP_STAMPS */
int64_t dt_deepfm_stamps_offset_floats(int B, int F, int D, int Nd);
int dt_deepfm_accum_offsets(int F, int D, int Nd, int64_t* out11_host);
int dt_deepfm_train_step(const void* idx, int idx_kind, const float* table, const int64_t* row_offset,
                         const int32_t* vocab, const float* dense, const float* y, int B, int F, int D,
                         int Nd, const float* w_lin, const float* bn_gamma, const float* bn_beta,
                         float* bn_moving_mean, float* bn_moving_var, float bn_eps, float bn_momentum,
                         const float* W1, const float* b1, const float* W2, const float* b2,
                         const float* w3, const float* w_out, const float* b_out, float* logit_out,
                         int64_t* rows_out, float* grad_rows, float* accum, void* workspace,
                         int* oob_count, void* dedupe_ws, int64_t dedupe_slots, float grad_rows_scale,
                         int grad_rows_field_major, int phases, float embedding_dropout, unsigned* dropout_seed,
                         float dense_input_dropout, const float* sample_weight, void* stream);
/* dt_deepfm_train_step_adam — the same step with the optimizer's row-sparse update fused into it (replaces, for the looked-up
 * table rows, the `apply_gradients` half of keras.Model.train_step that DeepModel.fit drives, deepmodel.py:114-129 with
 * the Adam of :321-322).  `table` is updated IN PLACE for every row looked up exactly once in the batch (Keras-Adam
 * read-modify-write of p and its slots adam_m / adam_v right where the row's gradient is formed: the gradient row never
 * reaches HBM); slot_stride = floats between the slot records of consecutive rows (D: two [V,D] arrays, 2 D: one
 * [V,2,D] array with v == m + D); adam_state = the device step state of dt_adam_state_init (lr_t is read from it; NULL:
 * the scalar lr_t).  Needs phases == 2 (| DT_STEP_LOSS_MSE) and dedupe_ws: rows looked up several times leave as
 * segments (their members' gradient rows in grad_rows, rows_out == -1).
 * dense_n == 0: the segments are updated, together with the dense parameters and the state's advance, by
 * dt_adam_rows_step_seg(..., fields = -2, ...) — which skips the entries of `rows` (already applied here).
 * dense_n > 0: dense_p / dense_m / dense_v are the model's flat dense parameter buffer and its Adam slots, laid out like
 * accum (dense_n = the offset of d w_lin + F + Nd floats); the step's last launch then also applies Keras Adam to every
 * dense element where its gradient is finished, walks the segments and advances adam_state (lr = the base learning
 * rate): the call IS keras.Model.train_step — forward, loss, backward and apply_gradients — and no optimizer launch
 * follows. */
int dt_deepfm_train_step_adam(const void* idx, int idx_kind, float* table, const int64_t* row_offset,
                              const int32_t* vocab, const float* dense, const float* y, int B, int F, int D,
                              int Nd, const float* w_lin, const float* bn_gamma, const float* bn_beta,
                              float* bn_moving_mean, float* bn_moving_var, float bn_eps, float bn_momentum,
                              const float* W1, const float* b1, const float* W2, const float* b2,
                              const float* w3, const float* w_out, const float* b_out, float* logit_out,
                              int64_t* rows_out, float* grad_rows, float* accum, void* workspace,
                              int* oob_count, void* dedupe_ws, int64_t dedupe_slots, int phases,
                              float embedding_dropout, unsigned* dropout_seed, float dense_input_dropout,
                              const float* sample_weight, float* adam_m, float* adam_v,
                              int slot_stride, void* adam_state, float lr_t, float beta1, float beta2, float eps,
                              float* dense_p, float* dense_m, float* dense_v, int64_t dense_n, float lr,
                              const void* next_idx, int64_t* next_rows_out, void* next_dedupe_ws, void* stream);
/* embedding_dropout > 0 (ModelConfig.embedding_dropout, config.py:84: SpatialDropout1D on every [B,1,D] embedding =
 * element dropout scaled by 1/(1-p)): element (b, f, d) is kept iff dt_deepfm_dropout_hash(*dropout_seed, b, f*D+d) >=
 * p * 2^32.  *dropout_seed is a DEVICE word, advanced by the step itself (so a captured graph draws a fresh mask at every
 * replay); pass 0 / NULL at inference.
 * dense_input_dropout > 0 (ModelConfig.dense_dropout, config.py:83: the Dropout 'dropout_dense_input' on the concatenated
 * continuous inputs, deepmodel.py:429-430): continuous value (b, k) is kept iff dt_deepfm_dropout_hash(*dropout_seed, b,
 * F*D + k) >= p * 2^32 and scaled by 1/(1-p), where the step packs it into the concat row — `linear`, the BN statistics
 * and the tower all see the masked value, as in the reference graph.
 * sample_weight [B] or NULL (keras.Model.fit's sample_weight x class_weight, deepmodel.py:114-129 passes both through):
 * loss = sum_b w_b * l_b / B and every gradient follows from d loss / d logit_b = w_b * (...) / B (Keras
 * SUM_OVER_BATCH_SIZE reduction of the weighted per-sample losses). */
unsigned dt_deepfm_dropout_hash(unsigned seed, unsigned b, unsigned col);

/* ---- fused DeepFM / DCN inference (csrc/infer.hip; kernels: csrc/infer_x3.h).
 * ONE launch per predict batch (replaces, for the graphs dt_*_infer_supported takes, the
 * layer-by-layer forward that the reference's DeepModel.predict / evaluate run through keras Model.predict / evaluate,
 * deepmodel.py:134-175).  At inference BatchNormalization normalises with its moving statistics (Keras BN inference:
 * (x - moving_mean) / sqrt(moving_variance + eps) * gamma + beta), Dropout is the identity and every row's logit depends
 * on that row only, so a 32-row tile runs gather, linear + FM (DeepFM) or the Cross network (DCN, dcn_nets), the input BN,
 * the two-cell tower of deepnets.py:401-427 on matrix cores, the output unit and its activation in one block.
 *   dt_*_infer_supported: the step's field / width domain (as dt_deepfm_supported: D in {4, .., 64} a power of two,
 *     F D / 4 <= 128, Nd <= 64, C = F D + Nd <= 544; DCN: L in 1..8) at any batch size; H1 <= 128, H2 <= 64 relu cells;
 *     cells = the tower cells with batch norm (bit 0: cell 1, bit 1: cell 2; Dense without bias -> BN -> relu).
 *   dt_*_infer_prepare: the weights -> workspace (dt_*_infer_workspace_bytes bytes, 16-byte aligned), one launch on
 *     `stream`; call it again whenever a weight or moving statistic changed.  W1 [C][ld1] / W2 [H1][ld2] with leading
 *     dimensions (contiguous, or views into wider zero-padded slabs); per cell its Dense bias (NULL: none) and, with its bit
 *     in `cells`, its BatchNormalization's gamma / beta (NULL: 1 / 0), moving mean / variance and eps.  DeepFM: w_lin
 *     [F + Nd] = linear_logit's kernel, w3 [H2] = dense_logit_dnn_nets' kernel, w_out / b_out = task_output's (b_out NULL:
 *     no bias).  DCN (dcn_nets alone): cross_w / cross_b [L][C], w3 [C + H2] = task_output's kernel (cross part first),
 *     w_out NULL (= 1), b_out = task_output's bias or NULL.
 *   dt_*_infer: one batch of B >= 0 rows (ids as in dt_deepfm_train_step, out-of-range ids read a zero row and are counted
 *     into *oob_count when it is given) -> logit_out [B] and, if out != NULL, out [B] = sigmoid(logit) with DT_INFER_SIGMOID
 *     (binary task) or the logit (regression).  flags | DT_INFER_TOWER_BF16: the tower's products on plain bf16 operands
 *     (the 1e-2 class); default: split-bf16 with six products per operand pair, the fp32 class (it also serves the 'f32'
 *     mode).  The Cross network's scalars keep six products in both modes. */
#define DT_INFER_SIGMOID 0x1
#define DT_INFER_TOWER_BF16 0x2
int dt_deepfm_infer_supported(int F, int D, int Nd, int H1, int H2, int cells);
int dt_dcn_infer_supported(int F, int D, int Nd, int H1, int H2, int cells, int L);
int64_t dt_deepfm_infer_workspace_bytes(int F, int D, int Nd);
int64_t dt_dcn_infer_workspace_bytes(int F, int D, int Nd, int L);
int dt_deepfm_infer_prepare(int F, int D, int Nd, const float* w_lin, const float* bn_gamma, const float* bn_beta,
                            const float* bn_mean, const float* bn_var, float bn_eps, const float* W1, int ld1, int H1,
                            const float* b1, const float* W2, int ld2, int H2, const float* b2, int cells,
                            const float* c1_gamma, const float* c1_beta, const float* c1_mean, const float* c1_var,
                            float c1_eps, const float* c2_gamma, const float* c2_beta, const float* c2_mean,
                            const float* c2_var, float c2_eps, const float* w3, const float* w_out, const float* b_out,
                            void* workspace, void* stream);
int dt_dcn_infer_prepare(int F, int D, int Nd, const float* cross_w, const float* cross_b, int L, const float* bn_gamma,
                         const float* bn_beta, const float* bn_mean, const float* bn_var, float bn_eps, const float* W1,
                         int ld1, int H1, const float* b1, const float* W2, int ld2, int H2, const float* b2, int cells,
                         const float* c1_gamma, const float* c1_beta, const float* c1_mean, const float* c1_var,
                         float c1_eps, const float* c2_gamma, const float* c2_beta, const float* c2_mean,
                         const float* c2_var, float c2_eps, const float* w3, const float* w_out, const float* b_out,
                         void* workspace, void* stream);
int dt_deepfm_infer(const void* idx, int idx_kind, const float* table, const int64_t* row_offset, const int32_t* vocab,
                    const float* dense, int B, int F, int D, int Nd, const void* workspace, float* logit_out, float* out,
                    int* oob_count, int flags, void* stream);
int dt_dcn_infer(const void* idx, int idx_kind, const float* table, const int64_t* row_offset, const int32_t* vocab,
                 const float* dense, int B, int F, int D, int Nd, int L, const void* workspace, float* logit_out,
                 float* out, int* oob_count, int flags, void* stream);

/* ---- fused inference for every Add-stacked subset of {linear, fm_nets, dnn_nets}: the launches of dt_deepfm_infer* with
 * the graph's nets as a mask (replaces, for the graphs dt_stack_infer_supported takes, the layer-by-layer forward of the
 * reference's DeepModel.predict / evaluate, deepmodel.py:134-175, over the graph deepmodel.py:286-301 assembles from
 * deepnets.py:43-66 `linear`, 84-96 `fm_nets`, 163-169 `dnn_nets`).  nets = a non-empty mask of DT_NET_*, the order of
 * config.nets does not matter: logit = (linear + fm + tower, over the terms present) w_out + b_out.
 *   With DT_NET_DNN the 32-row tile kernel of dt_deepfm_infer runs with the absent terms compiled out (DT_NET_LINEAR |
 *   DT_NET_FM | DT_NET_DNN is dt_deepfm_infer's own kernel); without it neither the input BatchNormalization nor a GEMM is
 *   in the graph and a gather-and-reduce kernel runs, one wave per row, no LDS.  H1 / H2 / cells and every tower argument
 *   are ignored then, DT_INFER_TOWER_BF16 has nothing to act on.
 *   The mask sits where dt_dcn_infer* carry L (after Nd; last in _supported); the other arguments of
 *   dt_stack_infer_prepare are dt_deepfm_infer_prepare's.  w_lin may be NULL when and only when the mask has no
 *   DT_NET_LINEAR; bn_mean / bn_var / W1 / W2 / w3 may be NULL when and only when it has no DT_NET_DNN.  Two or more nets:
 *   w3 [H2] = dense_logit_dnn_nets' kernel, w_out = task_output's [1][1] kernel.  One net: there is no dense_logit layer and
 *   no Add — DT_NET_DNN alone: w3 [H2] = task_output's kernel and w_out NULL (= 1; NULL only in this case); DT_NET_LINEAR or
 *   DT_NET_FM alone: w_out = task_output's [1][1] kernel.  b_out = task_output's bias or NULL.
 *   dt_stack_infer's other arguments are dt_deepfm_infer's; the workspace is the one dt_stack_infer_prepare wrote for the same
 *   mask and dims (dt_stack_infer_workspace_bytes: only the regions the nets read). */
#define DT_NET_LINEAR 0x1
#define DT_NET_FM 0x2
#define DT_NET_DNN 0x4
int dt_stack_infer_supported(int F, int D, int Nd, int H1, int H2, int cells, int nets);
int64_t dt_stack_infer_workspace_bytes(int F, int D, int Nd, int nets);
int dt_stack_infer_prepare(int F, int D, int Nd, int nets, const float* w_lin, const float* bn_gamma, const float* bn_beta,
                           const float* bn_mean, const float* bn_var, float bn_eps, const float* W1, int ld1, int H1,
                           const float* b1, const float* W2, int ld2, int H2, const float* b2, int cells,
                           const float* c1_gamma, const float* c1_beta, const float* c1_mean, const float* c1_var,
                           float c1_eps, const float* c2_gamma, const float* c2_beta, const float* c2_mean,
                           const float* c2_var, float c2_eps, const float* w3, const float* w_out, const float* b_out,
                           void* workspace, void* stream);
int dt_stack_infer(const void* idx, int idx_kind, const float* table, const int64_t* row_offset,
                   const int32_t* vocab, const float* dense, int B, int F, int D, int Nd, int nets, const void* workspace,
                   float* logit_out, float* out, int* oob_count, int flags, void* stream);

/* ---- one CIN layer's forward on a filter packed ONCE (inference).  dt_cin_layer_fwd_bf16 / _bf16x3 re-lay W as bf16 parts of
 * W^T on every call (one extra launch); at inference the filter does not change between batches, so dt_cin_pack writes that
 * layout once and dt_cin_layer_fwd_packed runs the layer's kernel on it — the same launch on the same values as the entry of
 * the same mode (reference layers.py:689-710), bit for bit.  mode: DT_CIN_F32 (dt_cin_layer_fwd, which reads W as it is:
 * `packed` is a copy of W), DT_CIN_BF16 (dt_cin_layer_fwd_bf16), DT_CIN_BF16X3 (dt_cin_layer_fwd_bf16x3).
 *   dt_cin_fwd_supported: 1 when the forward of `mode` takes the shape at every batch size (bf16 modes: F0 <= 128, Hk <= 128,
 *     L <= 256 and the tiles fit the LDS; exact mode: D <= 128 and the tiles fit), else 0.
 *   dt_cin_packed_bytes: size of `packed` (16-byte aligned, a multiple of 16), -1 for bad sizes / mode.
 *   dt_cin_layer_fwd_packed: dt_cin_layer_fwd's arguments with `packed` for W. */
#define DT_CIN_F32 0
#define DT_CIN_BF16 1
#define DT_CIN_BF16X3 2
int dt_cin_fwd_supported(int mode, int F0, int Hk, int L, int D, int act);
int64_t dt_cin_packed_bytes(int mode, int F0, int Hk, int L);
int dt_cin_pack(int mode, const float* W, int F0, int Hk, int L, void* packed, void* stream);
int dt_cin_layer_fwd_packed(int mode, const float* x0, const float* xk, const void* packed, const float* bias, int act, int B,
                            int F0, int Hk, int L, int D, int64_t x0_bstride, int64_t xk_bstride, float* y, void* stream);

/* ---- fused xDeepFM inference: 2 + n_layers launches per predict batch (replaces, for the graph dt_xdeepfm_infer_supported
 * takes, the layer-by-layer forward of the reference's DeepModel.predict / evaluate, deepmodel.py:134-175, over nets
 * ['linear', 'cin_nets', 'dnn_nets'] in any order, Add-stacked: deepnets.py:43-66 `linear`, 69-81 `cin_nets`, 163-169
 * `dnn_nets`, layers.py:638-734 CIN, deepmodel.py:286-301 the head).
 *   The CIN is n_layers layers of layer_sizes[k] filters (HOST array of ints); direct = cin_params['direct'] (0: the first
 *   half of every layer but the last feeds the next layer, the second half is pooled; the last layer and, with direct = 1,
 *   every layer is pooled whole, layers.py:713-721); cin_mode = DT_CIN_* (the layer kernels' precision mode).
 *   dt_xdeepfm_infer_supported: dt_stack_infer_supported's domain for DT_NET_LINEAR | DT_NET_DNN, F <= 64, 1 ..
 *     DT_XDEEPFM_MAX_LAYERS layers that dt_cin_fwd_supported takes (F0 = F, Hk = F then the previous layer's share, act =
 *     cin_params['activation']), even sizes where direct = 0 halves them, use_residual = 0 and reduce_D = 0; else 0.
 *   dt_xdeepfm_infer_prepare (once per predict / evaluate; replaces nothing of the reference: it writes what the launches
 *     read): dt_deepfm_infer_prepare's arguments up to b_out — w3 = dense_logit_dnn_nets' kernel, w_out / b_out =
 *     task_output's (b_out NULL: no bias) — then the CIN: cin_W = HOST array of n_layers device pointers, layer k's filter
 *     [F Hk][layer_sizes[k]]; w_ex [P] / b_ex (NULL: none) = the exFM_out Dense's kernel and bias, P = the pooled channels.
 *     workspace: dt_xdeepfm_infer_workspace_bytes bytes, 16-byte aligned.
 *   Per batch of B >= 0 rows, in this order on one stream:
 *   dt_xdeepfm_infer_tower (replaces the embedding gather, linear_logit, bn_concat_emb_dense, the two tower cells and
 *     dense_logit_dnn_nets: deepnets.py:43-66, 163-169, 401-427): dt_stack_infer's launch for DT_NET_LINEAR | DT_NET_DNN that
 *     also stores the rows it gathered, x0_out [B][F][D] (the CIN's input; an out-of-range id: zeros, counted once into
 *     *oob_count), and writes partial_out [B] = linear + tower . w3 instead of the output.  flags: DT_INFER_TOWER_BF16 or 0.
 *   dt_xdeepfm_infer_cin (replaces one pass of the loop of layers.py:689-718): layer `layer` on its packed filter: y
 *     [B][layer_sizes[layer]][D] = act(conv(outer(x0, xk)) + bias) with xk = x0 for layer 0, else the leading channels of
 *     y_prev = layer - 1's output (read in place).  bias [layer_sizes[layer]] or NULL.
 *   dt_xdeepfm_infer_head (replaces layers.py:720-734 — reduce_sum over D, concat, exFM_out — and deepmodel.py:286-301 — Add,
 *     task_output, the activation): y = HOST array of the n_layers outputs -> logit_out [B] = (partial + (pooled . w_ex +
 *     b_ex)) w_out + b_out and, if out != NULL, out [B] = sigmoid(logit) with DT_INFER_SIGMOID or the logit. */
#define DT_XDEEPFM_MAX_LAYERS 8
int dt_xdeepfm_infer_supported(int F, int D, int Nd, int H1, int H2, int cells, int n_layers, const int* layer_sizes,
                               int direct, int use_residual, int reduce_D, int act, int cin_mode);
int64_t dt_xdeepfm_infer_workspace_bytes(int F, int D, int Nd, int n_layers, const int* layer_sizes, int direct, int cin_mode);
int dt_xdeepfm_infer_prepare(int F, int D, int Nd, const float* w_lin, const float* bn_gamma, const float* bn_beta,
                             const float* bn_mean, const float* bn_var, float bn_eps, const float* W1, int ld1, int H1,
                             const float* b1, const float* W2, int ld2, int H2, const float* b2, int cells,
                             const float* c1_gamma, const float* c1_beta, const float* c1_mean, const float* c1_var,
                             float c1_eps, const float* c2_gamma, const float* c2_beta, const float* c2_mean,
                             const float* c2_var, float c2_eps, const float* w3, const float* w_out, const float* b_out,
                             int n_layers, const int* layer_sizes, int direct, int cin_mode, const float* const* cin_W,
                             const float* w_ex, const float* b_ex, void* workspace, void* stream);
int dt_xdeepfm_infer_tower(const void* idx, int idx_kind, const float* table, const int64_t* row_offset, const int32_t* vocab,
                           const float* dense, int B, int F, int D, int Nd, const void* workspace, float* x0_out,
                           float* partial_out, int* oob_count, int flags, void* stream);
int dt_xdeepfm_infer_cin(int layer, const float* x0, const float* y_prev, const float* bias, int act, int B, int F, int D,
                         int Nd, int n_layers, const int* layer_sizes, int direct, int cin_mode, const void* workspace,
                         float* y, void* stream);
int dt_xdeepfm_infer_head(const float* const* y, const float* partial, int B, int F, int D, int Nd, int n_layers,
                          const int* layer_sizes, int direct, int cin_mode, const void* workspace, float* logit_out,
                          float* out, int flags, void* stream);

/* ---- fused AutoInt inference: ONE launch per predict batch (csrc/autoint.hip k_autoint_infer; replaces, for nets =
 * ['autoint_nets'] alone, the layer-by-layer forward of the reference's DeepModel.predict / evaluate, deepmodel.py:134-175:
 * the embedding gather (layers.py:889-904), deepnets.py:210-224 `autoint_nets` — per interacting layer MultiheadAttention.call,
 * layers.py:119-153, with its BatchNormalization :151 on the moving statistics and its Dropout :141 as the identity — Flatten,
 * and the head deepmodel.py:131-143 / 286-301: task_output over [F D] and the activation).
 *   A wave keeps one batch row in its LDS slab from the gather to the logit; every layer's weights sit in the block's LDS.
 *   All n_layers layers share F, D, H, NP and mfma_mode (DT_AI_*: the projections are the layer kernel's own products).
 *   dt_autoint_infer_supported: 1 iff dt_autoint_supported(F, D, H), mfma_mode is valid for D (the bf16 modes: D = 32), 1 <=
 *     n_layers <= DT_AUTOINT_INFER_MAX_LAYERS, use_residual in {0, 1}, and four waves' slabs plus all layers' weights fit the
 *     160 KiB of LDS: D = 32 takes up to 5 layers (6 do not fit), D = 16 all DT_AUTOINT_INFER_MAX_LAYERS.
 *   dt_autoint_infer_workspace_bytes: size of `workspace` (16-byte aligned), -1 outside that domain.
 *   dt_autoint_infer_prepare (once per predict / evaluate, one launch; replaces nothing of the reference: it writes what the
 *     batch launches read, from the values the tensors hold at call time): Wq / Wk / Wv / Wr, bq / bk / bv / br = HOST arrays
 *     of n_layers device pointers, layer l's dense_Q / dense_K / dense_V / dense_residual kernel [D][D] and bias [D]
 *     (use_residual = False: Wr / br NULL or arrays of NULLs -> NP = 3); bn_gamma / bn_beta / bn_mean / bn_var = HOST arrays of
 *     the layers' BatchNormalization gamma, beta (arrays or entries may be NULL: 1 / 0), moving_mean, moving_variance [D];
 *     bn_eps their epsilon; w_out [F D] / b_out (NULL: none) = task_output's kernel and bias.  The TOP layer's
 *     normalisation is folded into the head here: w'[i D + c] = s[c] w_out[i D + c], c0 = sum t[c] w_out[i D + c] + b_out
 *     (s = gamma / sqrt(var + eps), t = beta - mean s); the layers below keep (s, t) and are normalised when the next
 *     layer loads them.
 *   dt_autoint_infer (per batch of B >= 0 rows, B < 2^31; B = 0: no launch): ids [B][F] (idx_kind = DT_IDX_*; an id outside
 *     [0, vocab[f]) reads a zero row and is counted once into *oob_count when it is given) -> logit_out [B] and, if out !=
 *     NULL, out [B] = sigmoid(logit) with flags = DT_INFER_SIGMOID or the logit with flags = 0.  NP = 4 with the residual
 *     projection, else 3, as prepared.  The grid is at most DT_AUTOINT_INFER_MAX_BLOCKS blocks of 8 / 6 / 4 waves (the most
 *     that fit the LDS); a wave strides over the batch rows. */
#define DT_AUTOINT_INFER_MAX_LAYERS 8
#define DT_AUTOINT_INFER_MAX_BLOCKS 256
int dt_autoint_infer_supported(int F, int D, int H, int n_layers, int use_residual, int mfma_mode);
int64_t dt_autoint_infer_workspace_bytes(int F, int D, int n_layers);
int dt_autoint_infer_prepare(int F, int D, int n_layers, const float* const* Wq, const float* const* Wk,
                             const float* const* Wv, const float* const* Wr, const float* const* bq, const float* const* bk,
                             const float* const* bv, const float* const* br, const float* const* bn_gamma,
                             const float* const* bn_beta, const float* const* bn_mean, const float* const* bn_var,
                             float bn_eps, const float* w_out, const float* b_out, void* workspace, void* stream);
int dt_autoint_infer(const void* idx, int idx_kind, const float* table, const int64_t* row_offset, const int32_t* vocab,
                     int64_t B, int F, int D, int H, int n_layers, int NP, const void* workspace, float* logit_out, float* out,
                     int* oob_count, int flags, int mfma_mode, void* stream);

/* ---- fused AFM inference: ONE launch per predict batch (csrc/afm_infer.hip k_afm_infer; replaces, for nets = 'afm_nets'
 * alone or Add-stacked with 'linear' and / or 'fm_nets', the layer-by-layer forward of the reference's DeepModel.predict /
 * evaluate: the embedding gather (layers.py:889-904), deepnets.py:99-108 `afm_nets` = AFM.call layers.py:786-807 — the pair
 * products, the attention Dense and its activation, projection_h, the softmax over the pairs, the weighted sum, Dropout as the
 * identity, the Dense(1, no bias) — deepnets.py:43-66 `linear`, deepnets.py:84-96 `fm_nets`, and the head deepmodel.py:286-301:
 * Add, task_output [1][1], the activation).
 *   nets = DT_NET_AFM, optionally | DT_NET_LINEAR | DT_NET_FM.  The AFM layer's output is [B, 1]: it enters Add as it is (no
 *   dense_logit layer), so logit = (linear + fm + afm over the nets present) w_out + b_out.
 *   One wave scores one batch row: the row's F table rows go to the wave's LDS slab, then for every tile of 16 pairs p = (i, j)
 *   bi_p = x_i * x_j meets the attention kernel on the exact-fp32 matrix core (v_mfma_f32_16x16x4_f32), l_p = act(bi_p Wa + ba) . h
 *   and t_p = bi_p . w_do feed an online softmax (running max, sum e^(l - m), sum e^(l - m) t): afm = sum_p softmax(l)_p t_p.
 *   Nothing but the logit (and the output) is written: no score buffer, no pooled vector.
 *   dt_afm_infer_supported: 1 iff F >= 2, (F, D, Nd) are dims the fused plans take (D in {4, 8, 16, 32, 64}, F D <= 512,
 *     Nd <= 64), 1 <= H <= 64 (the attention factor; compiled widths 16 / 32 / 64), act a DT_ACT_* code and nets a mask
 *     as above.
 *   dt_afm_infer_workspace_bytes: size of `workspace` (16-byte aligned), -1 outside that domain.
 *   dt_afm_infer_prepare (once per predict / evaluate, one launch; replaces nothing of the reference: it writes what the batch
 *     launches read, from the values the tensors hold at call time): Wa [D][H] / ba [H] (NULL: 0) = dense_afm_attention's kernel
 *     and bias, h [H] = projection_h, w_do [D] = afm_layer_dense_out's kernel — all zero-padded to the compiled width —
 *     w_lin [F + Nd] = linear_logit's kernel (NULL when and only when nets has no DT_NET_LINEAR), w_out / b_out =
 *     task_output's [1][1] kernel and bias (b_out NULL: none); also the table of the pairs' (i, j).
 *   dt_afm_infer (per batch of B >= 0 rows, B < 2^31; B = 0: no launch): ids [B][F] (idx_kind = DT_IDX_*; an id outside
 *     [0, vocab[f]) reads a zero row and is counted once into *oob_count when it is given), dense [B][Nd] (read only with
 *     DT_NET_LINEAR and Nd > 0, else it may be NULL) -> logit_out [B] and, if out != NULL, out [B] = sigmoid(logit) with flags
 *     = DT_INFER_SIGMOID or the logit with flags = 0.  H, nets as prepared; act = the attention activation (DT_ACT_*).  The
 *     workspace carries the (F, D, Nd, compiled width of H, nets) it was prepared for: a launch with other values reads no
 *     weight and writes NaN into every logit and output.  The
 *     grid is at most DT_AFM_INFER_MAX_BLOCKS blocks of DT_AFM_INFER_ROWS waves; a wave strides over the batch rows. */
#define DT_NET_AFM 0x8
#define DT_AFM_INFER_ROWS 4
#define DT_AFM_INFER_MAX_BLOCKS 1024
int dt_afm_infer_supported(int F, int D, int Nd, int H, int act, int nets);
int64_t dt_afm_infer_workspace_bytes(int F, int D, int Nd, int H, int nets);
int dt_afm_infer_prepare(int F, int D, int Nd, int H, int nets, const float* Wa, const float* ba, const float* h,
                         const float* w_do, const float* w_lin, const float* w_out, const float* b_out, void* workspace,
                         void* stream);
int dt_afm_infer(const void* idx, int idx_kind, const float* table, const int64_t* row_offset, const int32_t* vocab,
                 const float* dense, int64_t B, int F, int D, int Nd, int H, int nets, int act, const void* workspace,
                 float* logit_out, float* out, int* oob_count, int flags, void* stream);

/* ---- fused PNN inference: ONE launch per predict batch (csrc/pnn_infer.hip k_pnn_infer; replaces, for each of the nets
 * 'pnn_nets' / 'ipnn_nets' / 'opnn_nets' alone in config.nets, the layer-by-layer forward of the reference's DeepModel.predict /
 * evaluate: the embedding gather (layers.py:889-904), InnerProduct.call layers.py:473-487, OuterProduct.call layers.py:543-581,
 * the input BatchNormalization on its moving statistics, deepnets.py:111-160 — Concatenate(products ++ [xn]), the two-cell relu
 * tower deepnets.py:401-427 with Dropout as the identity — and the head deepmodel.py:286-301: a single net, so no dense_logit
 * layer and no Add; task_output's [H2][1] kernel is the tower's output vector and the output weight is 1).
 *   products = a non-empty mask DT_PNN_INNER | DT_PNN_OUTER; kernel_type = DT_OP_KERNEL_* of the outer layer, ignored without
 *   DT_PNN_OUTER.  P = F (F - 1) / 2 pairs in itertools.combinations order; Cp = P x the number of product layers.  The first
 *   Dense's rows: the product columns (inner first, then outer), the F D embedding columns, the Nd dense columns.  The
 *   products are formed from the raw table rows; only the last F D + Nd columns are normalised.
 *   A block owns a 32-row tile: the rows go to LDS once, the first Dense's K = Cp + F D + Nd runs in chunks of 128 columns
 *   that are computed into LDS and multiplied at once ('mat': K_p . X_i^T on the exact-fp32 matrix core, then the row-wise
 *   dot with x_j; the other products and the normalisation elementwise), the accumulators stay in registers over all chunks.
 *   The product layers are exact fp32 in both tower modes.
 *   dt_pnn_infer_supported: 1 iff 2 <= F <= 64, D in {4, 8, 16, 32, 64}, F D <= 512, 0 <= Nd <= 64, 1 <= H1 <= 128,
 *     1 <= H2 <= 64, cells a mask of bits 0 / 1 (as dt_deepfm_infer_supported), products as above and kernel_type valid when
 *     DT_PNN_OUTER is set.
 *   dt_pnn_infer_workspace_bytes: size of `workspace` (16-byte aligned), -1 outside that domain.
 *   dt_pnn_infer_prepare (once per predict / evaluate, one launch; replaces nothing of the reference: it writes what the batch
 *     launches read, from the values the tensors hold at call time): op_kernel = the outer layer's kernel, 'mat' [D][P][D] |
 *     'vec' [P][D] | 'num' [P][1] (NULL when and only when products has no DT_PNN_OUTER; 'mat' is re-laid pair-major), the
 *     input BN over the F D + Nd columns, W1 [Cp + F D + Nd][ld1], W2 and the two cells' bias / BN arguments as
 *     dt_deepfm_infer_prepare, w3 [H2] = task_output's kernel, b_out = its bias or NULL.
 *   dt_pnn_infer (per batch of B >= 0 rows, B < 2^31; B = 0: no launch): ids [B][F] (idx_kind = DT_IDX_*; an id outside
 *     [0, vocab[f]) reads a zero row and is counted once into *oob_count when it is given), dense [B][Nd] (NULL with Nd = 0)
 *     -> logit_out [B] and, if out != NULL, out [B] = sigmoid(logit) with DT_INFER_SIGMOID or the logit.  flags |
 *     DT_INFER_TOWER_BF16: the two tower GEMMs on plain bf16 operands.  The workspace carries the (F, D, Nd, products,
 *     kernel_type) it was prepared for: a launch with other values reads no weight and writes NaN into every logit and
 *     output.  The grid is at most DT_PNN_INFER_MAX_BLOCKS blocks, strided over the 32-row tiles. */
#define DT_PNN_INNER 0x1
#define DT_PNN_OUTER 0x2
#define DT_PNN_INFER_MAX_BLOCKS 512
int dt_pnn_infer_supported(int F, int D, int Nd, int H1, int H2, int cells, int products, int kernel_type);
int64_t dt_pnn_infer_workspace_bytes(int F, int D, int Nd, int products, int kernel_type);
int dt_pnn_infer_prepare(int F, int D, int Nd, int products, int kernel_type, const float* op_kernel, const float* bn_gamma,
                         const float* bn_beta, const float* bn_mean, const float* bn_var, float bn_eps, const float* W1, int ld1,
                         int H1, const float* b1, const float* W2, int ld2, int H2, const float* b2, int cells,
                         const float* c1_gamma, const float* c1_beta, const float* c1_mean, const float* c1_var, float c1_eps,
                         const float* c2_gamma, const float* c2_beta, const float* c2_mean, const float* c2_var, float c2_eps,
                         const float* w3, const float* b_out, void* workspace, void* stream);
int dt_pnn_infer(const void* idx, int idx_kind, const float* table, const int64_t* row_offset, const int32_t* vocab,
                 const float* dense, int64_t B, int F, int D, int Nd, int products, int kernel_type, const void* workspace,
                 float* logit_out, float* out, int* oob_count, int flags, void* stream);

/* ---- fused FiBiNet inference: ONE launch per predict batch (csrc/fibi_infer.hip k_fibi_infer; replaces, for the net
 * 'fibi_dnn_nets' alone in config.nets (deepnets.FiBiNet), the layer-by-layer forward of the reference's DeepModel.predict /
 * evaluate: the embedding gather (layers.py:889-904), SENET.call layers.py:245-308, the two BilinearInteraction.call
 * layers.py:311-382, deepnets.py:344-386 — Concatenate of the two [P][D] blocks, Flatten, Concatenate with the RAW dense
 * values, the two-cell relu tower deepnets.py:401-427 with Dropout as the identity — and the head deepmodel.py:286-301: a
 * single net, so no dense_logit layer and no Add; task_output's [H2][1] kernel is the tower's output vector and the output
 * weight is 1).  bn_concat_emb_dense is not part of this graph and is not applied.
 *   bilinear_type = DT_BILINEAR_* (ops.BILINEAR_TYPES' codes); pooling_op = DT_FIBI_POOL_*; R = SENET's reduction_num =
 *   max(F / reduction_ratio, 1).  P = F (F - 1) / 2 pairs (i, j), i < j, in itertools.combinations order; a pair's weight is
 *   W[p] 'field_interaction' | W[i] 'field_each' | W[0] 'field_all'.  The first Dense's rows: the senet half (P D columns,
 *   pair-major: a2_i a2_j ((x_i . Ws) * x_j)), the raw half (P D columns: (x_i . Wr) * x_j), the Nd dense columns.
 *   A block owns a 32-row tile: the rows go to LDS once, SENET's a2 [F] per row is computed once per tile in plain fp32, the
 *   first Dense's K = 2 P D + Nd runs in chunks of 128 columns that are computed into LDS (W^T . X_i^T on the exact-fp32 matrix
 *   core, then the elementwise products) and multiplied at once; the accumulators stay in registers over all chunks.  SENET
 *   and the bilinear products are exact fp32 in both tower modes.
 *   dt_fibi_infer_supported: 1 iff 2 <= F <= 64, D in {4, 8, 16, 32, 64}, F D <= 512, 1 <= Nd <= 64 (the net concatenates the
 *     dense input unconditionally), 1 <= R <= 64, 1 <= H1 <= 128, 1 <= H2 <= 64, cells a mask of bits 0 / 1 (as
 *     dt_deepfm_infer_supported), bilinear_type and pooling_op one of their codes.
 *   dt_fibi_infer_workspace_bytes: size of `workspace` (16-byte aligned; about 8 MB at F = 26, D = 16, 25 MB at F = 64, D = 8),
 *     -1 outside the shape domain.
 *   dt_fibi_infer_prepare (once per predict / evaluate, one launch; it writes what the batch launches read, from the values
 *     the tensors hold at call time): SENET's att1 kernel [F][R] and bias [R], att2 kernel [R][F] and bias [F] (a bias may be
 *     NULL), the stacked W [nW][D][D] of senet_bilinear_layer and of embedding_bilinear_layer (nW = P | F - 1 | 1; each
 *     matrix is stored transposed), W1 [2 P D + Nd][ld1], W2 and the two cells' bias / BN arguments as
 *     dt_deepfm_infer_prepare, w3 [H2] = task_output's kernel, b_out = its bias or NULL.
 *   dt_fibi_infer (per batch of B >= 0 rows, B < 2^31; B = 0: no launch, no pointer is looked at): ids [B][F] (idx_kind =
 *     DT_IDX_*; an id outside [0, vocab[f]) reads a zero row and is counted once into *oob_count when it is given), dense
 *     [B][Nd] -> logit_out [B] and, if out != NULL, out [B] = sigmoid(logit) with DT_INFER_SIGMOID or the logit.  flags |
 *     DT_INFER_TOWER_BF16: the first tower GEMM on plain bf16 operands.  The workspace carries the (F, D, Nd, bilinear_type, R)
 *     it was prepared for: a launch with other values reads no weight and writes NaN into every logit and output.  The
 *     launch is refused when the tile needs more than 160 KB of LDS (no shape of the domain does).  The grid is at most
 *     DT_FIBI_INFER_MAX_BLOCKS blocks, strided over the 32-row tiles. */
#define DT_BILINEAR_FIELD_INTERACTION 0
#define DT_BILINEAR_FIELD_EACH 1
#define DT_BILINEAR_FIELD_ALL 2
#define DT_FIBI_POOL_MEAN 0
#define DT_FIBI_POOL_MAX 1
#define DT_FIBI_INFER_MAX_BLOCKS 512
int dt_fibi_infer_supported(int F, int D, int Nd, int H1, int H2, int cells, int bilinear_type, int pooling_op, int R);
int64_t dt_fibi_infer_workspace_bytes(int F, int D, int Nd, int bilinear_type, int R);
int dt_fibi_infer_prepare(int F, int D, int Nd, int bilinear_type, int R, const float* se_k1, const float* se_b1,
                          const float* se_k2, const float* se_b2, const float* W_senet, const float* W_raw, const float* W1,
                          int ld1, int H1, const float* b1, const float* W2, int ld2, int H2, const float* b2, int cells,
                          const float* c1_gamma, const float* c1_beta, const float* c1_mean, const float* c1_var, float c1_eps,
                          const float* c2_gamma, const float* c2_beta, const float* c2_mean, const float* c2_var, float c2_eps,
                          const float* w3, const float* b_out, void* workspace, void* stream);
int dt_fibi_infer(const void* idx, int idx_kind, const float* table, const int64_t* row_offset, const int32_t* vocab,
                  const float* dense, int64_t B, int F, int D, int Nd, int bilinear_type, int pooling_op, int R,
                  const void* workspace, float* logit_out, float* out, int* oob_count, int flags, void* stream);

/* ---- fused FGCNN inference: 2 depth + 1 launches per predict batch (csrc/fgcnn_infer.hip; replaces, for the net
 * 'fgcnn_dnn_nets' alone in config.nets (deepnets.FGCNN), the layer-by-layer forward of the reference's DeepModel.predict /
 * evaluate: the embedding gather (layers.py:889-904), deepnets.py:227-261 — expand_dims, the FGCNN blocks (FGCNN.call
 * layers.py:161-242: Conv2D((h, 1), 'same', tanh), MaxPooling2D((p, 1), 'same'), Flatten, the recombination Dense with tanh,
 * the reshape), Concatenate of the generated features and the raw embeddings — deepnets.py:326-341: Flatten, Concatenate with
 * the RAW dense values, the two-cell relu tower deepnets.py:401-427 with Dropout as the identity — and the head
 * deepmodel.py:286-301: a single net, so no dense_logit layer and no Add; task_output's [H2][1] kernel is the tower's output
 * vector and the output weight is 1).  bn_concat_emb_dense is not part of this graph and is not applied.
 *   depth = the number of FGCNN blocks; filters / heights / pools / new_filters = HOST int arrays of `depth` entries
 *   (fgcnn_params' fg_filters, fg_heights, fg_pool_heights, fg_new_feat_filters).  F_1 = F, C_1 = 1; block k maps
 *   [F_k][D][C_k] to the pooled map [Fp_k = ceil(F_k / pool_k)][D][filters_k] and to N_k = F_k D new_filters_k generated
 *   columns; F_(k+1) = Fp_k, C_(k+1) = filters_k.  'same' padding as the reference splits it: total / 2 before, the rest
 *   after; the pooling pads with -inf, so a short window takes the maximum of the fields it has.  The first Dense's rows: the
 *   generated columns of block 1 .. depth, the F D embedding columns, the Nd dense columns.
 *   Per batch: dt_fgcnn_infer_conv and dt_fgcnn_infer_recomb once per block, in block order, then dt_fgcnn_infer_tower — one
 *   launch each, every one this library's own kernel.  The convolution reads its taps from the map in LDS (plain fp32 FMAs;
 *   no taps matrix and no padded map is written), the recombination Dense and the tower's two GEMMs run on the matrix core
 *   with the six split-bf16 products (the fp32 class), tanh is libm's tanhf.  Between the launches only the pooled maps
 *   [B][Fp_k D filters_k] and the generated features [B][sum N_k] live in memory, in buffers the caller owns; the tower reads
 *   its input in chunks from the features and the rows it gathers itself.
 *   dt_fgcnn_infer_supported: 1 iff 2 <= F <= 64, D in {4, 8, 16, 32, 64}, F D <= 512, 0 <= Nd <= 64, 1 <= depth <= 3, every
 *     filters in 1 .. 16, height in 1 .. 9 (either parity, also above F_k), pool in 1 .. 3 (also not dividing F_k), new_filters
 *     in 1 .. 3, 1 <= H1 <= 128, 1 <= H2 <= 64, cells a mask of bits 0 / 1 (as dt_deepfm_infer_supported).
 *   dt_fgcnn_infer_workspace_bytes: size of `workspace` (16-byte aligned; about 21 MB at F = 26, D = 16 with the default
 *     blocks: the packed recombination weights), -1 outside the shape domain.
 *   dt_fgcnn_infer_prepare (once per predict / evaluate, one launch; it writes what the batch launches read, from the values
 *     the tensors hold at call time): conv_kernels / conv_biases / rec_kernels / rec_biases = HOST arrays of `depth` device
 *     pointers: conv2d_kernel [h][1][C_k][filters] and conv2d_bias [filters], the recombination Dense's kernel
 *     [Fp_k D filters][N_k] and bias [N_k], all contiguous (a bias may be NULL); W1 [sum N_k + F D + Nd][ld1], W2 and the two
 *     cells' bias / BN arguments as dt_deepfm_infer_prepare, w3 [H2] = task_output's kernel, b_out = its bias or NULL.
 *   dt_fgcnn_infer_conv (block = 0 .. depth - 1): block 0 gathers ids [B][F] (idx_kind = DT_IDX_*; an id outside
 *     [0, vocab[f]) reads a zero row; it is counted by dt_fgcnn_infer_tower alone) and `prev` is ignored; a later block reads
 *     `prev` = the pooled map of the block before and ignores the gather arguments -> pooled_out [B][Fp D filters].
 *   dt_fgcnn_infer_recomb: pooled [B][Fp D filters] of `block` -> that block's N_k columns of feats [B][sum N_k].
 *   dt_fgcnn_infer_tower: ids, dense [B][Nd] (NULL with Nd = 0), feats -> logit_out [B] and, if out != NULL, out [B] =
 *     sigmoid(logit) with DT_INFER_SIGMOID or the logit.  flags | DT_INFER_TOWER_BF16: the first tower GEMM on plain bf16
 *     operands; the blocks stay in the fp32 class.  An out-of-range id is counted once into *oob_count when it is given.
 *   All three: B >= 0 rows, B < 2^31; B = 0: no launch, no pointer is looked at.  The workspace carries the (F, D, Nd, block
 *   parameters) it was prepared for: a launch with other values reads no weight; the conv / recomb launches then write
 *   nothing and the tower launch writes NaN into every logit and output.  Each grid is at most DT_FGCNN_INFER_MAX_BLOCKS
 *   blocks (times the 128-column chunks of N_k for the recombination), strided over the row tiles (32 rows; 64 for the
 *   recombination; up to 32 for the convolution of a later block). */
#define DT_FGCNN_INFER_MAX_BLOCKS 512
#define DT_FGCNN_INFER_MAX_DEPTH 3
int dt_fgcnn_infer_supported(int F, int D, int Nd, int H1, int H2, int cells, int depth, const int* filters, const int* heights,
                             const int* pools, const int* new_filters);
int64_t dt_fgcnn_infer_workspace_bytes(int F, int D, int Nd, int depth, const int* filters, const int* heights, const int* pools,
                                       const int* new_filters);
int dt_fgcnn_infer_prepare(int F, int D, int Nd, int depth, const int* filters, const int* heights, const int* pools,
                           const int* new_filters, const float* const* conv_kernels, const float* const* conv_biases,
                           const float* const* rec_kernels, const float* const* rec_biases, const float* W1, int ld1, int H1,
                           const float* b1, const float* W2, int ld2, int H2, const float* b2, int cells, const float* c1_gamma,
                           const float* c1_beta, const float* c1_mean, const float* c1_var, float c1_eps, const float* c2_gamma,
                           const float* c2_beta, const float* c2_mean, const float* c2_var, float c2_eps, const float* w3,
                           const float* b_out, void* workspace, void* stream);
int dt_fgcnn_infer_conv(int block, const void* idx, int idx_kind, const float* table, const int64_t* row_offset,
                        const int32_t* vocab, const float* prev, int64_t B, int F, int D, int Nd, int depth, const int* filters,
                        const int* heights, const int* pools, const int* new_filters, const void* workspace, float* pooled_out,
                        void* stream);
int dt_fgcnn_infer_recomb(int block, const float* pooled, int64_t B, int F, int D, int Nd, int depth, const int* filters,
                          const int* heights, const int* pools, const int* new_filters, const void* workspace, float* feats,
                          void* stream);
int dt_fgcnn_infer_tower(const void* idx, int idx_kind, const float* table, const int64_t* row_offset, const int32_t* vocab,
                         const float* dense, const float* feats, int64_t B, int F, int D, int Nd, int depth, const int* filters,
                         const int* heights, const int* pools, const int* new_filters, const void* workspace, float* logit_out,
                         float* out, int* oob_count, int flags, void* stream);

/* Epoch metrics on the device (csrc/metrics.hip): what DeepModel.fit / evaluate compute at the end of every epoch from the
 * concatenated outputs (deepmodel.py:471-475, 526-530; sklearn.metrics.roc_auc_score and numpy on the host before).  All
 * results are integer or fixed-order sums: the same input gives the same bits.  No block of any launch waits for another
 * block; what one needs from the others comes from an earlier launch.  Common rules: n == 0 is a no-op that looks at no
 * pointer; n < 0 and n >= 2^31 are DT_ERR_INVALID_ARG, as are a null pointer, a null workspace, a float / uint32 array that
 * is not 4-byte aligned, a 64-bit output that is not 8-byte aligned and a workspace that is not 16-byte aligned, all before
 * the first launch.  The *_workspace_bytes queries return DT_ERR_INVALID_ARG for an n outside [0, 2^31).
 *
 * dt_metric_sort_pairs: stable least-significant-digit radix sort of (keys[i], vals[i]) by key, ascending: 8-bit digits, 4
 *   passes, per pass a histogram per tile of dt_metric_sort_tile() elements, an exclusive scan over (digit-major, tile-minor)
 *   counts and a stable scatter (13 launches: one memset + 4 x 3 kernels).  Pairs with equal keys keep their input order.
 *   keys / vals are not written; keys_out / vals_out may be the inputs themselves (in place).  ws: dt_metric_sort_workspace_
 *   bytes(n) bytes, contents irrelevant before and after.
 * dt_metric_auc: exact binary ROC AUC counts for score [n] and label [n] (0 / 1).  out5 (int64, written by the call):
 *     [0] U2 = sum over groups g of equal score of pos_g * (2 * negatives with a lower score + neg_g)
 *     [1] P = labels equal to 1      [2] N = n - P      [3] scores that are NaN or +-Inf      [4] labels that are neither 0 nor 1
 *   AUC = U2 / (2 P N): the probability that a positive outscores a negative, ties counting one half — roc_auc_score's
 *   value.  -0.0 and +0.0 tie.  The caller returns nan for P == 0, N == 0 or out5[3] > 0 (roc_auc_score raises there) and
 *   takes its host path when out5[4] > 0 (such labels are counted as negatives here).  19 launches: 2 memsets, the key
 *   transform, the sort's 12, tile sums, their scan, the groups' compaction and one thread per group.
 * dt_metric_sums: out (DT_METRIC_SUMS_WORDS 8-byte words; the first three are the result, the rest scratch):
 *     [0] int64  count of (y_prob > 0.5) == (int64)y_true     [1] double sum (y_prob - y_true)^2     [2] double sum |y_prob - y_true|
 *   differences, squares and sums in float64; per-block partials (at most DT_METRIC_SUMS_BLOCKS, a function of n alone), then
 *   one block adds them in a fixed order: no float atomics.  2 launches.
 * dt_metric_argmax_hits: out[0] (int64) = rows r of y_prob [n, C] whose argmax (the first maximum, as numpy.argmax) equals
 *   the label: y_true [n] holding the class as a float (DT_METRIC_Y_LABELS) or the argmax of row r of a one-hot y_true [n, C]
 *   (DT_METRIC_Y_ONEHOT).  C >= 2.  2 launches (memset + kernel).                                                       */
#define DT_METRIC_Y_LABELS 0
#define DT_METRIC_Y_ONEHOT 1
#define DT_METRIC_SUMS_BLOCKS 256
#define DT_METRIC_SUMS_WORDS 771
int dt_metric_sort_tile(void);
int64_t dt_metric_sort_workspace_bytes(int64_t n);
int dt_metric_sort_pairs(const uint32_t* keys, const uint32_t* vals, int64_t n, uint32_t* keys_out, uint32_t* vals_out, void* ws,
                         void* stream);
int64_t dt_metric_auc_workspace_bytes(int64_t n);
int dt_metric_auc(const float* score, const float* label, int64_t n, void* ws, int64_t* out5, void* stream);
int dt_metric_sums(const float* y_true, const float* y_prob, int64_t n, void* out, void* stream);
int dt_metric_argmax_hits(const float* y_prob, const float* y_true, int y_kind, int64_t n, int C, int64_t* out, void* stream);

/* More epoch metrics on the device (csrc/metrics.hip): log loss, precision / recall, top-k accuracy, MSLE / MAPE and average
 * precision, i.e. the rest of what the `metrics=[...]` of deepmodel.py's compile (:324-338) names and its fit / evaluate report
 * (:471-475, :526-530; keras.metrics and sklearn on the host before).  The rules of the dt_metric_* block hold: no block
 * waits for another, integer results are exact, float64 sums are per-block partials (at most DT_SCORE_BLOCKS, a function of
 * the shape alone) added by one block in a fixed order, so the same input gives the same bits.  Every `out` is an array of
 * 8-byte words: the result words first, the partials behind them (scratch).  Everything is computed in float64 from the
 * float32 inputs; lo = (double)1e-7f, hi = (double)(1.0f - 1e-7f); clip(x) = numpy.clip(x, lo, hi) and max(x, lo) =
 * numpy.maximum: a NaN stays a NaN.  Refused with DT_ERR_INVALID_ARG before any launch: n outside [0, 2^31), n * C of 2^31
 * and more, C below 2 (below 1 for dt_score_binary's element-wise form), k < 1, an unknown y_kind, a null pointer or
 * workspace, a float array off 4-byte alignment, an `out` off 8-byte alignment, a workspace off 16-byte alignment.  n == 0 is
 * a no-op that looks at no pointer.  A float label names class (int)label when 0 <= label < C and no class otherwise.
 *
 * dt_score_binary: over the n * C elements of y_prob; y_kind DT_METRIC_Y_ONEHOT: y_true has n * C elements too (binary [n],
 *   multilabel or one-hot [n, C]; soft labels allowed), DT_METRIC_Y_LABELS: y_true [n] labels, y = (label's class == column).
 *   out (DT_SCORE_BINARY_WORDS): [0] TP [1] FP [2] FN [3] TN (int64; predicted positive: p > 0.5, label positive: y != 0)
 *   [4] double sum of -(y log q + (1 - y) log(1 - q)), q = clip(p).  2 launches.
 * dt_score_regression: out (DT_SCORE_REGRESSION_WORDS): [0] double sum (log(max(p, lo) + 1) - log(max(y, lo) + 1))^2
 *   [1] double sum |y - p| / max(|y|, lo).  2 launches.
 * dt_score_categorical: rows of y_prob [n, C] against y_true [n] (DT_METRIC_Y_LABELS) or [n, C] (DT_METRIC_Y_ONEHOT).  The
 *   target class is the label's, or the first maximum of the y_true row (`v > best` from class 0 on).  out
 *   (DT_SCORE_CATEGORICAL_WORDS): [0] int64 rows with fewer than k classes scoring above the target (in_top_k: ties across
 *   the boundary are all in; a NaN target score, or a label naming no class, misses) [1] double sum over rows of
 *   -sum_c y_c log(clip(p_c / s)), s = sum_c p_c (LABELS: -log(clip(p_label / s)), NaN for a label naming no class).
 *   C <= DT_SCORE_THREAD_ROW_MAX_C: a thread per row, both sums in class order.  Wider: a wave per row, lane l adds classes
 *   l, l + 64, ... in that order, then partial[l] += partial[l + o] for o = 32, 16, ... 1.  2 launches.
 * dt_score_ranking: dt_metric_auc (same workspace layout, same kernels, same five words) plus average precision from the
 *   compacted groups of equal score.  out (DT_SCORE_RANKING_WORDS): [0..4] dt_metric_auc's out5 [5] double sum over groups
 *   of pos_g * TPcum_g / (n - start_g), TPcum_g = positives scoring at least the group's, n - start_g = rows scoring at least
 *   it; AP = out[5] / P = sklearn.metrics.average_precision_score.  The caller returns nan and takes its host path where
 *   it does for AUC.  21 launches: dt_metric_auc's 19, the groups' terms, their sum.                                     */
#define DT_SCORE_BLOCKS 256
#define DT_SCORE_BINARY_WORDS 1285
#define DT_SCORE_REGRESSION_WORDS 514
#define DT_SCORE_CATEGORICAL_WORDS 514
#define DT_SCORE_RANKING_WORDS 262
#define DT_SCORE_THREAD_ROW_MAX_C 32
int dt_score_binary(const float* y_true, const float* y_prob, int y_kind, int64_t n, int C, void* out, void* stream);
int dt_score_regression(const float* y_true, const float* y_pred, int64_t n, void* out, void* stream);
int dt_score_categorical(const float* y_prob, const float* y_true, int y_kind, int64_t n, int C, int k, void* out, void* stream);
int64_t dt_score_ranking_workspace_bytes(int64_t n);
int dt_score_ranking(const float* score, const float* label, int64_t n, void* ws, void* out, void* stream);

/* keras.regularizers.L1L2 on the device (csrc/regularizer.hip): penalty and gradient of `count` float32 tensors per call, tensor
 * t being (x[t], n[t] elements, l1[t], l2[t]).  x / out / n / l1 / l2 are HOST arrays (of device pointers, sizes and
 * coefficients); the descriptors travel as kernel arguments, 32 tensors per launch.  Common rules: a member with n == 0
 * contributes nothing and its pointer is not looked at; count == 0 is valid; a negative count, a negative n (or one of 2^40
 * and more), a null pointer with n > 0, a null descriptor array, a null or misaligned output / workspace are
 * DT_ERR_INVALID_ARG before the first launch.  No alignment beyond that of a float is asked of x / out.  NaN / Inf propagate.
 *
 * dt_reg_penalty: total[0] (double) = sum over t of l1[t] * sum|x| + l2[t] * sum x^2, total_f32[0] its float32 rounding.  A
 *   coefficient equal to zero adds no term (Keras' `if self.l1:`).  Launch 1 (one per 32 tensors): a block sums one chunk of
 *   dt_reg_chunk() elements in float64 in a fixed order and writes one double into `workspace`
 *   (dt_reg_penalty_workspace_bytes(count, n) bytes, 8-byte aligned, contents irrelevant before and after); launch 2: one
 *   block adds the partials in index order with a fixed tree.  No float atomics, no block waits for another: the same
 *   input gives the same bits, and an unaligned view gives the bits of an aligned copy.
 * dt_reg_grad: out[t][i] = go * (l1 * sign(x) + 2 * l2 * x) for every element (one launch per 32 tensors), in this fp32 order
 *   with no contraction: t = fl(fl(2 l2) x); u = +l1, -l1 or 0 (sign(+-0) = 0); r = fl(u + t); fl(go r).  accumulate != 0:
 *   out[t][i] = fl(out[t][i] + that) instead.  go: DEVICE pointer to the upstream scalar, read by the kernel (no host
 *   synchronisation; replays inside a captured graph).  float4 where x[t] and out[t] reach 16-byte alignment at the same
 *   element, scalars before that, for the tail and otherwise: every route gives the same bits.  out[t] must not overlap
 *   another member's out or any x except in place (out[t] == x[t]).                                                     */
int dt_reg_chunk(void);
int64_t dt_reg_penalty_workspace_bytes(int count, const int64_t* n);
int dt_reg_penalty(int count, const float* const* x, const int64_t* n, const double* l1, const double* l2, void* workspace,
                   double* total, float* total_f32, void* stream);
int dt_reg_grad(int count, const float* const* x, float* const* out, const int64_t* n, const float* l1, const float* l2,
                const float* go, int accumulate, void* stream);

/* The losses of a train step on the device (csrc/loss.hip), from the LOGITS z [rows, classes] (the `task_output` Dense before
 * its activation), the float32 target t [rows, classes] and Keras' sample_weight x class_weight per row w [rows] (NULL: 1).
 * Replaces keras.losses.BinaryCrossentropy / CategoricalCrossentropy / MeanSquaredError / MeanAbsoluteError selected by
 * deepmodel.py:324-338 and layers.py:1006-1017 (BinaryFocalLoss) / :1062-1076 (CategoricalFocalLoss), with reduction
 * SUM_OVER_BATCH_SIZE: loss[0] = sum_b w_b l_b / rows and dz = (w_b / rows) dl_b/dz (dz NULL: the value only), eps = 1e-7:
 *   DT_LOSS_BCE    l_b = mean_c max(z,0) - z t + log1p(exp(-|z|))               dl/dz = (sigmoid(z) - t) / classes
 *   DT_LOSS_CCE    l_b = -sum_c t_c log p_c, p = softmax(z), log p = z - lse     dl/dz = (sum_k t_k) p_c - t_c
 *   DT_LOSS_MSE    l_b = mean_c (z - t)^2                                        dl/dz = 2 (z - t) / classes
 *   DT_LOSS_MAE    l_b = mean_c |z - t|                                          dl/dz = sign(z - t) / classes, sign(0) = 0
 *   DT_LOSS_CATEGORICAL_FOCAL  l_b = sum_c alpha (1 - ph_c)^gamma (-t_c log ph_c), ph = clamp(softmax(z), eps, 1 - eps);
 *                  dl/dz_k = p_k (g_k - sum_c g_c p_c), g_c = alpha t_c [gamma (1 - ph_c)^(gamma-1) log ph_c - (1 - ph_c)^gamma / ph_c]
 *                  and g_c = 0 where the clamp is active; 1 - p is formed as -expm1(log p)
 *   DT_LOSS_BINARY_FOCAL  not a per-row loss (w must be NULL): with p = sigmoid(z), q = sigmoid(-z) clamped to [eps, 1 - eps],
 *                  loss = -(1 / (rows classes)) sum [T1 + T0], T1 = alpha qh^gamma log ph where t == 1, else the constant
 *                  alpha eps^gamma log(1 - eps); T0 = (1 - alpha) ph^gamma log qh where t == 0, else (1 - alpha) eps^gamma
 *                  log(1 - eps); the constants are added in float64 as count x constant.  dz = -(1 / (rows classes)) p q
 *                  [(t==1) alpha (-gamma qh^(gamma-1) log ph + qh^gamma / ph) + (t==0)(1 - alpha)(gamma ph^(gamma-1) log qh -
 *                  ph^gamma / qh)], zero where the clamp is active (|z| > ln((1 - eps) / eps)).
 * Per-element and per-row math is float32; every sum over classes, elements and rows is float64 in a fixed order (lanes by
 * halving, waves in order, partials in index order): no float atomics, no block waits for another, the same input gives
 * the same bits in loss and dz, and dz = NULL gives the bits of loss.  At most two launches: per-block partials into
 * `workspace` (dt_loss_workspace_bytes(rows, classes) bytes, 8-byte aligned, contents irrelevant before and after), then one
 * block adds them; one launch when one block covers the problem.  gamma / alpha are read by the focal kinds only.
 * Domain: 1 <= rows < 2^31, 1 <= classes <= DT_LOSS_MAX_CLASSES, classes >= 2 for the categorical kinds, gamma >= 0; a kind,
 * shape or gamma outside it, a null z / t / loss / workspace, a misaligned pointer or a w with DT_LOSS_BINARY_FOCAL are
 * DT_ERR_INVALID_ARG before the first launch (dt_loss_workspace_bytes returns it for a shape outside the domain).        */
#define DT_LOSS_BCE 0
#define DT_LOSS_CCE 1
#define DT_LOSS_MSE 2
#define DT_LOSS_MAE 3
#define DT_LOSS_BINARY_FOCAL 4
#define DT_LOSS_CATEGORICAL_FOCAL 5
#define DT_LOSS_MAX_CLASSES 4096
int64_t dt_loss_workspace_bytes(int64_t rows, int classes);
int dt_loss(int kind, const float* z, const float* t, const float* w, int64_t rows, int classes, float gamma, float alpha,
            float* loss, float* dz, void* workspace, void* stream);

/* The regression losses of Keras 3 on the device (csrc/loss_reg.hip): keras.losses.Huber / LogCosh /
 * MeanSquaredLogarithmicError / MeanAbsolutePercentageError / Poisson on the model OUTPUT p [rows, classes] (the regression
 * task's `task_output`, which has no activation), the target t [rows, classes] and the per-row weight w [rows] (NULL: 1), with
 * reduction SUM_OVER_BATCH_SIZE: loss[0] = sum_b w_b mean_c f / rows, dz = w_b g / (rows classes) (dz NULL: the value only);
 * e = p - t, eps = float32(1e-7):
 *   DT_LOSS_HUBER     f = 0.5 e^2 where |e| <= delta, else delta |e| - 0.5 delta^2      g = e, else delta sign(e)
 *   DT_LOSS_LOG_COSH  f = log cosh e, formed as log1p(2 sinh^2(e / 2)) below |e| = 10 and |e| - ln 2 above (Keras' e +
 *                     softplus(-2e) - ln 2 cancels for small e)                          g = tanh e
 *   DT_LOSS_MSLE      f = (a - b)^2, a = log1p(max(p, eps)), b = log1p(max(t, eps))      g = 2 (a - b) / (max(p, eps) + 1) where
 *                     p >= eps, else 0
 *   DT_LOSS_MAPE      f = 100 |e| / max(|t|, eps)                                        g = 100 sign(e) / max(|t|, eps), sign(0) = 0
 *   DT_LOSS_POISSON   f = p - t log(p + eps)  (NaN for p + eps < 0, as in Keras)         g = 1 - t / (p + eps)
 * Geometry, sums, determinism, workspace rules and domain are dt_loss' (at most two launches, one double per block of 2048
 * elements in `workspace`, dt_loss_reg_workspace_bytes(rows, classes) bytes, 8-byte aligned).  delta is read by DT_LOSS_HUBER
 * only and must be finite and > 0.  The kind codes continue dt_loss' so that a code names one loss; each entry point takes
 * only its own.                                                                                                              */
#define DT_LOSS_HUBER 6
#define DT_LOSS_LOG_COSH 7
#define DT_LOSS_MSLE 8
#define DT_LOSS_MAPE 9
#define DT_LOSS_POISSON 10
int64_t dt_loss_reg_workspace_bytes(int64_t rows, int classes);
int dt_loss_reg(int kind, const float* p, const float* t, const float* w, int64_t rows, int classes, float delta, float* loss,
                float* dz, void* workspace, void* stream);

/* GHMCLoss.calc (layers.py:1111-1163) on the device (csrc/loss_reg.hip), over the n elements of the logits z, the targets t and
 * the optional mask (NULL: is_mask False; an element counts where mask > 0).  g = |sigmoid(z) - t| in float32 puts an element
 * into bin b iff L_b <= g < R_b, L_b = float32(b / bins), R_b = float32((b + 1) / bins), R_{bins-1} = float32(1 + 1e-6); an
 * element in no bin (a target of -1) or masked out has weight 0 and gradient 0.  The counts are exact integers (LDS integer
 * atomics per block, added in block order); tot = max(n, 1) or max(#mask > 0, 1); nvalid = the number of non-empty bins; with
 * momentum > 0 acc_sum [bins] is updated IN PLACE for the non-empty bins, acc_b = fl(fl(momentum acc_b) + fl(one_minus_momentum
 * count_b)) (one_minus_momentum: float32(1 - momentum) as the caller rounds it), and the bin weight is w_b = fl(fl(tot /
 * denom_b) / nvalid), denom_b = acc_b or count_b at momentum 0.
 *   loss[0] = sum_e w_bin(e) (max(z,0) - z t + log1p(exp(-|z|))) / tot        (float64 sum in a fixed order)
 *   dz[e]   = w_bin(e) (sigmoid(z) - t) / tot                                  (NULL: the value only; the weights carry no gradient)
 * nvalid = 0 gives NaN, as the torch chain does.  At most four launches (counts, bins, elements, total), one when n <= 2048; the
 * same bits on every run.  workspace: dt_ghmc_workspace_bytes(n, bins) bytes, 8-byte aligned, contents irrelevant before and
 * after.  Domain: 1 <= n < 2^40, 1 <= bins <= DT_GHMC_MAX_BINS, 0 <= momentum < 1, acc_sum non-null when momentum > 0; anything
 * else, a null z / t / loss / workspace or a misaligned pointer is DT_ERR_INVALID_ARG before the first launch.              */
#define DT_GHMC_MAX_BINS 256
int64_t dt_ghmc_workspace_bytes(int64_t n, int bins);
int dt_ghmc(const float* z, const float* t, const float* mask, int64_t n, int bins, float momentum, float one_minus_momentum,
            float* acc_sum, float* loss, float* dz, void* workspace, void* stream);

/* ---- the tail of a DNN tower cell: Activation -> (Dropout) in one launch each way (csrc/cell.hip) ------------------------ *
 * Over x [N, C] fp32:  out = keep * act(x)  and  dx = g * keep * act'(.), keep = 0 or 1 / (1 - rate) by the counter hash
 * dt_cell_dropout_hash(seed[0], salt, row, col) >= dt_cell_dropout_threshold(rate) — recomputed by the backward from the same
 * DEVICE seed word, so no mask tensor exists; salt tells the cells of one forward apart.  rate == 0 runs no hash and reads
 * no seed (NULL allowed); rate == 1 multiplies by 0, as torch's dropout does.
 * act: a DT_ACT_* code (0-8, evaluated by the helpers the CIN / AFM kernels use) or one of the cell's own codes below, which
 * only these two entry points take.  [ext] Keras 3 definitions: relu6 min(max(x,0),6); leaky_relu x > 0 ? x : 0.2 x; silu =
 * swish x sigmoid(x); gelu the exact erf form; mish x tanh(softplus(x)); hard_sigmoid relu6(x + 3) / 6; hard_silu = hard_swish
 * x hard_sigmoid(x).
 * The backward takes act' from ONE saved tensor: the forward's OUTPUT for codes 0-8, relu6, leaky_relu and hard_sigmoid when
 * rate is 0 or 1 (saved_is_input = 0), the forward's INPUT for silu, gelu, mish and hard_silu (dt_cell_saves_input = 1) and
 * for every code when 0 < rate < 1 (saved_is_input = 1; anything else is DT_ERR_INVALID_ARG).  At a kink the derivative is
 * the one torch's autograd takes: relu, relu6 0 at 0 and at 6; leaky_relu 0.2 at 0; hard_sigmoid 0 at +-3; hard_silu 0 at
 * -3 and 1 at 3.  NaN in gives NaN out both ways; every value and derivative is finite for finite |x| <= 80.
 * 16-byte loads and stores when N C >= 4 and every tensor is 16-byte aligned, floats otherwise; a grid-stride loop of at most
 * 2048 blocks: dt_cell_pass_elems() elements per grid pass of the 16-byte path.  Domain: 1 <= N < 2^31, C >= 1, N C < 2^40,
 * 0 <= rate <= 1; outside it, an unknown code, a null or misaligned pointer: DT_ERR_INVALID_ARG before any launch.          */
#define DT_CELL_ACT_RELU6 9
#define DT_CELL_ACT_LEAKY_RELU 10
#define DT_CELL_ACT_SILU 11
#define DT_CELL_ACT_GELU 12
#define DT_CELL_ACT_MISH 13
#define DT_CELL_ACT_HARD_SIGMOID 14
#define DT_CELL_ACT_HARD_SILU 15
#define DT_CELL_ACT_COUNT 16
unsigned dt_cell_dropout_hash(unsigned seed, unsigned salt, unsigned row, unsigned col);
unsigned dt_cell_dropout_threshold(float rate);
int64_t dt_cell_pass_elems(void);
int dt_cell_saves_input(int act);
int dt_cell_fwd(const float* x, int64_t N, int C, int act, float rate, const unsigned* seed, unsigned salt, float* out,
                void* stream);
int dt_cell_bwd(const float* g, const float* saved, int saved_is_input, int64_t N, int C, int act, float rate,
                const unsigned* seed, unsigned salt, float* dx, void* stream);

/* Gradient clipping on the device (csrc/gradclip.hip): keras.optimizers' clipvalue / clipnorm / global_clipnorm
 * (BaseOptimizer._clip_gradients) ahead of any optimizer step, and the row-sparse table gradient with its duplicate lookups
 * summed, which a norm or an element clamp of the TRUE per-row gradient needs.  Common rules: no float atomics, no block
 * waits for another, every sum runs in an order fixed by the sizes and the id pattern alone (the same input gives the same
 * bits), nothing is allocated, there is no host synchronisation, and every scalar a later kernel needs (sums, counts) is read
 * from DEVICE memory, so a captured graph replays correctly.  Every argument is checked before the first launch: a negative
 * size, a null pointer with something to do, a float / int64 / double array that is not aligned to its element, a null
 * workspace or one that is not 16-byte aligned, an unknown mode and a c that is not a finite number > 0 are
 * DT_ERR_INVALID_ARG.  A "variable" is one Keras variable: a dense tensor, or one field's row range of a packed table.
 *
 * dt_rows_coalesce: (rows int64 [n], values [n, D]) -> out_rows [n]: the distinct row ids ascending, then -1; out_vals [n, D]:
 *   each distinct row's summed gradient, the tail exactly 0 (a sum of squares over all n D floats is the table's);
 *   count[0] (int64, device) = distinct rows.  A row id outside [0, V) is a skipped lookup (-1 is the usual spelling).
 *   V, the table's row count, must be in [1, 2^32 - 1]: ids are sort keys of 32 bits, 2^32 - 1 marks a skipped lookup.
 *   n in [0, 2^31); n == 0 writes count[0] = 0 and looks at nothing else; any D >= 1 (16-byte pieces where D % 4 == 0 and
 *   values / out_vals are 16-byte aligned; every route gives the same bits).  Built on dt_metric_sort_pairs keyed on the row
 *   id with the lookup position as the value (stable: a row's lookups keep their order), then a scan of the segment heads
 *   and a sum through that inverted index: the sorted positions are cut into chunks of dt_rows_coalesce_chunk() = 512; inside
 *   a chunk every row's lookups are added in order; a row that spans chunks gets one partial per chunk and the partials are
 *   added in chunk order — a hot row with thousands of lookups is never one thread's walk.  rows / values are not written
 *   and must not overlap the outputs.  ws: dt_rows_coalesce_workspace_bytes(n, D) bytes.  19 launches.
 * dt_grad_sumsq: sums[t] (double, device, [count]) = sum of g[t][i]^2 over n[t] elements, squares and sums in float64 (the
 *   multi-tensor form of dt_reg_penalty: g / n are HOST arrays, 32 tensors per launch pair; a block sums one chunk of
 *   dt_reg_chunk() elements in a fixed order, one block per tensor adds its partials in index order).  An empty tensor
 *   gives 0.  ws: dt_grad_sumsq_workspace_bytes(count, n) bytes, 8-byte aligned.
 * dt_rows_field_sumsq: for a coalesced table (out_rows ascending then -1, count[0] distinct rows): sums[f] (double, device,
 *   [F]) = sum of squares of the rows in [row_offset[f], row_offset[f + 1]) (the last field ends at V); row_offset: DEVICE
 *   int64 [F], ascending from 0.  A field is one contiguous range of the sorted rows, found by binary search on the
 *   device; DT_FIELD_SUMSQ_PARTS blocks per field sum one slice each, one thread per field adds the slices in index order
 *   (2 launches).  A field with no lookup gives 0.  ws: F * DT_FIELD_SUMSQ_PARTS doubles, 8-byte aligned.
 * dt_grad_clip / dt_rows_clip: in place, mode DT_CLIP_*; c: the host constant; sums: the DEVICE array of n_sums doubles the
 *   calls above filled, one per variable (not read by DT_CLIP_VALUE, may be NULL there):
 *     DT_CLIP_VALUE        g = g < -c ? -c : (g > c ? c : g)                           (NaN stays NaN)
 *     DT_CLIP_NORM         n_v = (float)sqrt(sums[v]);  g = fl(fl(g c) / max(n_v, c))
 *     DT_CLIP_GLOBAL_NORM  N = (float)sqrt(sums[0] + sums[1] + ... in index order);  s = fl(c min(fl(1 / N), fl(1 / c))) +
 *                          (N - N);  g = fl(g s): a non-finite N makes every gradient NaN, as Keras does
 *   dt_grad_clip: tensor t is variable sum_index[t] (HOST int array; unused for the other modes, may be NULL there); 32
 *   tensors per launch.  dt_rows_clip: row out_rows[j], j < count[0], belongs to the field f with row_offset[f] <= row <
 *   row_offset[f + 1], which is variable sum_base + f.  norm_out (device double, or NULL): receives sqrt of the sum of all
 *   n_sums entries (0 for DT_CLIP_VALUE).                                                                                  */
#define DT_CLIP_VALUE 0
#define DT_CLIP_NORM 1
#define DT_CLIP_GLOBAL_NORM 2
#define DT_FIELD_SUMSQ_PARTS 32
int dt_rows_coalesce_chunk(void);
int64_t dt_rows_coalesce_workspace_bytes(int64_t n, int D);
int dt_rows_coalesce(const int64_t* rows, const float* values, int64_t n, int D, int64_t V, int64_t* out_rows, float* out_vals,
                     int64_t* count, void* ws, void* stream);
int64_t dt_grad_sumsq_workspace_bytes(int count, const int64_t* n);
int dt_grad_sumsq(int count, const float* const* g, const int64_t* n, double* sums, void* ws, void* stream);
int dt_rows_field_sumsq(const int64_t* out_rows, const float* out_vals, int64_t n, int D, const int64_t* count,
                        const int64_t* row_offset, int F, int64_t V, double* sums, void* ws, void* stream);
int dt_grad_clip(int mode, float c, int count, float* const* g, const int64_t* n, const int* sum_index, const double* sums,
                 int n_sums, double* norm_out, void* stream);
int dt_rows_clip(int mode, float c, const int64_t* out_rows, float* out_vals, int64_t n, int D, const int64_t* count,
                 const int64_t* row_offset, int F, int64_t V, const double* sums, int sum_base, int n_sums, double* norm_out,
                 void* stream);

/* keras.optimizers' `weight_decay` and `use_ema` / `ema_momentum` (BaseOptimizer._apply_weight_decay ahead of every
 * optimizer's update, the moving average of the weights behind it) as stages around any dt_*_step (csrc/optim_stages.hip).
 * float32, each formula evaluated in this order without contraction:
 *     decay                       p = p - (p * weight_decay) * lr                (lr: the optimizer's plain learning rate)
 *     average, step t (1-based)   a = m * a + (1 - m) * p,  m = 0 at t == 1, momentum afterwards
 *     a row idle for k steps      a = w + momentum^k * (a - w)     (k average steps on a constant weight w; k <= 8: the
 *                                 multiplication repeated, beyond: powf; k == 0 leaves a as it is)
 * `state` (DT_STAGE_STATE_BYTES device bytes): {int32 done = the steps the stage has completed}, written by
 * dt_stage_state_init, read on the device by every launch that averages (a captured graph replays them) and advanced by
 * dt_stage_advance, the LAST launch of a step.  Nothing here synchronises with the host or allocates.  Every argument is
 * checked before the first launch: negative sizes, null pointers with something to do, misaligned arrays, a weight_decay
 * that is not a finite number >= 0 and a momentum outside [0, 1] are DT_ERR_INVALID_ARG.
 * dt_decay_multi / dt_ema_multi: `count` regions (p[t], n[t]) — p / avg / n are HOST arrays, 32 regions per launch, 1024
 *   elements per block; a region whose pointers are 16-byte aligned takes 16-byte pieces and a scalar tail, any other the
 *   scalar loop (the same bits).  An excluded variable is simply not in the list.
 * dt_rows_stage_pre / dt_rows_stage_post: around the row update of a packed table [V, D], over rows [n]: the DISTINCT row
 *   ids dt_rows_coalesce emits (ascending, then -1: skipped, as is any id outside [0, V)).  16-byte pieces where D % 4 == 0
 *   (table and avg 16-byte aligned then), min(D / 4 or D, 256) threads per row, a row never straddles a block.
 *   pre:  avg != NULL: the row's average first catches up with the k = done - stamp[row] steps it sat out; then, decay != 0:
 *         the row decays — unless field_on (DEVICE int32 [F], NULL: all on) is 0 for the field f with row_offset[f] <= row <
 *         row_offset[f + 1] (row_offset: DEVICE int64 [F] ascending from 0; one column's `embeddings_i`).
 *   post: the step's average of the updated row, then stamp[row] = done + 1.
 *   Rows that were not looked up keep weight, average and stamp bit for bit.
 * dt_ema_rows_materialize: the catch-up for every row of the table, then every stamp = done (2 launches).                 */
#define DT_STAGE_STATE_BYTES 16
int dt_stage_state_init(void* state, int steps_done, void* stream);
int dt_stage_advance(void* state, void* stream);
int dt_decay_multi(int count, float* const* p, const int64_t* n, float weight_decay, float lr, void* stream);
int dt_ema_multi(int count, const float* const* p, float* const* avg, const int64_t* n, float momentum, const void* state,
                 void* stream);
int dt_rows_stage_pre(float* table, float* avg, const int* stamp, const int64_t* rows, int64_t n, int D, int64_t V,
                      const int64_t* row_offset, const int* field_on, int F, int decay, float weight_decay, float lr,
                      float momentum, const void* state, void* stream);
int dt_rows_stage_post(const float* table, float* avg, int* stamp, const int64_t* rows, int64_t n, int D, int64_t V,
                       float momentum, const void* state, void* stream);
int dt_ema_rows_materialize(const float* table, float* avg, int* stamp, int64_t V, int D, float momentum, const void* state,
                            void* stream);

/* Keras' DENSE Adam result on a row-sparse table (csrc/adam_exact.hip; training.KerasAdam(exact_rows=True)).  The reference's
 * default optimizer, keras.optimizers.Adam(learning_rate=0.001) (deepmodel.py:319-322), is applied to the densified embedding
 * gradient: a row that was not looked up has gradient 0 and still takes every step t (1-based),
 *     m = beta1 m;  v = beta2 v;  p = p - lr_t m / (sqrt(v) + eps),   lr_t = lr sqrt(1 - beta2^t) / (1 - beta1^t).
 * Here such a row waits: stamp (int32 [V]) holds the number of steps its p, m and v are current through, and a row that is
 * needed while c = AdamState.t - 1 steps are complete (read from the DEVICE `state` of dt_adam_state_init, so a captured
 * graph replays these launches) first pays the k = c - stamp[row] idle steps above.  float32, every formula in the order
 * written without contraction; beta1^t and beta2^t are running products seeded by one powf each; an element leaves the loop
 * at the first step whose term is 0, or leaves p unchanged and is below 2^-26 |p| (no later term can change p: they shrink by
 * sup_t (lr_{t+1} / lr_t) beta1 / sqrt(beta2) < 1, which the caller has checked), and its m and v take the rest of their
 * decay as one powf each.  m, v: the row's slots at m + row * slot_stride and v + row * slot_stride (one [V, 2, D] record:
 * v = m + D, slot_stride = 2 D; two arrays: slot_stride = D).  16-byte pieces where D % 4 == 0, slot_stride % 4 == 0 and
 * table, m and v are 16-byte aligned, floats otherwise; min(pieces, 256) threads per row, a row never straddles a block.
 * Nothing synchronises with the host or allocates.  Negative sizes, null or misaligned pointers with something to do,
 * overlapping slots, an unknown idx_kind and betas outside 0 <= beta1 < 1, 0 < beta2 < 1, beta1 < sqrt(beta2) are
 * DT_ERR_INVALID_ARG before any launch.
 * dt_adam_exact_supported(D): 1 for the D these entry points take (every D >= 1).
 * dt_adam_rows_catchup: ahead of the gather of a batch, with the gather's own (idx, idx_kind, row_offset, vocab, B, F): one
 *   thread group per lookup; an id outside [0, vocab[f]) or a row >= V touches nothing.  The group's first lane claims the
 *   row by an integer atomicExch of stamp[row] to c; when the old value is c already (another lookup of the row in this
 *   batch owns it, or nothing is pending) the group leaves, so duplicates need no merge: what reads the row is a later launch.
 * dt_adam_rows_materialize: the same for every row of the table (every stamp = c afterwards); a row whose m and v are all
 *   zero — never looked up — is restamped without its weights being written.
 * dt_adam_rows_stamp: behind the step's last row update (dt_adam_rows_step_seg, which for a row that is current IS Keras'
 *   dense step and has advanced the state): stamp[row] = AdamState.t - 1 for rows [n] (int64; -1 and ids >= V skipped).    */
int dt_adam_exact_supported(int D);
int dt_adam_rows_catchup(float* table, float* m, float* v, int slot_stride, int* stamp, const void* idx, int idx_kind,
                         const int64_t* row_offset, const int32_t* vocab, int B, int F, int D, int64_t V, float lr,
                         float beta1, float beta2, float eps, const void* state, void* stream);
int dt_adam_rows_materialize(float* table, float* m, float* v, int slot_stride, int* stamp, int64_t V, int D, float lr,
                             float beta1, float beta2, float eps, const void* state, void* stream);
int dt_adam_rows_stamp(int* stamp, const int64_t* rows, int64_t n, int64_t V, const void* state, void* stream);

/* Columns of a device-resident feed block permuted in place (csrc/feed_columns.hip; ops.permute_columns, the device path of
 * utils/feature_importance.py).  block: row-major [N, C] of 4-byte words — int32 ids or float32 values, moved and never
 * interpreted, so NaN payloads, -0.0 and denormals survive; the columns are [col0, col0 + width).
 * dt_column_gather: out[i, w] = block[perm[i], col0 + w] for out [N, width]; perm: DEVICE int64 [N].  An entry outside
 *   [0, N) is not dereferenced: that row keeps its own value.  block is only read.
 * dt_column_swap: block[i, col0 + w] <-> buf[i, w] for buf [N, width]; each word is read and written by one thread.
 * gather into buf, then swap: the block holds the permuted columns and buf the originals; the same swap again restores the
 * block bit for bit.  One thread per word of [N, width] (16-byte words where C, col0 and width are multiples of 4 and both
 * pointers 16-byte aligned), 256-thread blocks, a grid-stride loop under 2048 blocks, 64-bit element indices.  Nothing
 * synchronises with the host or allocates.  N < 0, C < 1, width < 1, col0 < 0, col0 + width > C and a null or misaligned
 * pointer are DT_ERR_INVALID_ARG before any launch; N == 0 is DT_OK without one.                                             */
int dt_column_gather(const void* block, int64_t N, int C, int col0, int width, const int64_t* perm, void* out, void* stream);
int dt_column_swap(void* block, int64_t N, int C, int col0, int width, void* buf, void* stream);

/* KernelSHAP on a device-resident feed (csrc/coalition.hip; ops.coalition_fill / coalition_mean / shap_solve, the device path of
 * utils/shap.py).  Replaces deeptables/utils/shap.py:11-29 (DeepTablesExplainer: shap.KernelExplainer over `model_fn`, which
 * builds a DataFrame of hybrid rows per call and runs DeepTable.predict on it): the hybrid rows are written into feed blocks on
 * the device, the model's outputs are averaged over the background there and the constrained regression is a product with a
 * matrix the host computes once per coalition plan.
 * masks: DEVICE uint32 [S, W], W = (M + 31) / 32: bit g % 32 of word g / 32 of coalition s holds player g of M.
 * dt_coalition_fill (replaces shap.py:23-25, the frame of hybrid rows): x [C], bg [Nb, C], out [(s1 - s0) Nb, C] are 4-byte
 *   words (int32 ids or float32 values, moved and never interpreted);
 *   out[(s - s0) Nb + b, c] = bit(masks[s], group[c]) ? x[c] : bg[b, c] for s in [s0, s1).  group: DEVICE int32 [C], the player
 *   that owns column c, or -1 for a column that always takes the background word; group_host: a HOST copy of it, checked
 *   against [-1, M) before the launch (the kernel itself treats a value outside [0, M) as -1, so it cannot index past a
 *   coalition's words).  One thread per word (16-byte words where C % 4 == 0 and x, bg, out are 16-byte aligned), 256-thread
 *   blocks, a grid-stride loop under 2048 blocks, 64-bit element indices.
 * dt_coalition_mean (replaces the mean over the background inside shap.py:28, KernelExplainer's `eyVal`):
 *   ey[seg, o] = (1 / Nb) sum_b out[seg Nb + b, o] for out float32 [nseg Nb, O], ey float64 [nseg, O]; one wave per sum, lane l
 *   adds rows l, l + 64, ... in order, then a fixed six-step butterfly: no atomics, the same bits on every run; NaN propagates.
 * dt_shap_solve (replaces the weighted regression inside shap.py:28, KernelExplainer.solve, without its L1 selection):
 *   for ey float64 [R, S, O], fx float64 [R, O], e0 float64 [O], P float64 [M - 1, S]:
 *   y'_s = ey_s - e0 - bit(masks[s], M - 1) (fx - e0); phi[r, o, j] = sum_s P[j, s] y'_s for j < M - 1 (the order of
 *   dt_coalition_mean); phi[r, o, M - 1] = (fx - e0) - sum_j phi[r, o, j].  phi: float64 [R, O, M].
 * Nothing synchronises with the host or allocates.  Negative sizes, M < 1 (solve: M < 2, S < 1), Nb < 1 for the mean, s0 > s1
 * or s1 > S, a null or misaligned pointer and a group_host entry outside [-1, M) are DT_ERR_INVALID_ARG before any launch;
 * empty sizes (s0 == s1, Nb == 0 or C == 0 for the fill; nseg == 0 or O == 0; R == 0 or O == 0) are DT_OK without one.       */
int dt_coalition_fill(const void* x, const void* bg, int64_t Nb, int C, const uint32_t* masks, int64_t S, int M, int64_t s0,
                      int64_t s1, const int32_t* group, const int32_t* group_host, void* out, void* stream);
int dt_coalition_mean(const float* out, int64_t nseg, int64_t Nb, int O, double* ey, void* stream);
int dt_shap_solve(const double* P, const uint32_t* masks, int64_t S, int M, const double* ey, const double* fx, const double* e0,
                  int64_t R, int O, double* phi, void* stream);

/* Rows of a device-resident feed block gathered and scattered, and the mean of K output buffers (csrc/feed_rows.hip;
 * ops.take_rows / put_rows / ensemble_mean, the device path of models/cross_validation.py).  block: row-major [N, C] of 4-byte
 * words — int32 ids or float32 values, moved and never interpreted; idx: DEVICE int64 [n].
 * dt_rows_take (replaces deeptables/models/deeptable.py:449, `tb.select_df(X, train_idx)`, `y[train_idx]` and their validation
 *   twins, a pandas slice per fold): out[i, :] = block[idx[i], :] for out [n, C], i < n.  Repeats are allowed and n may exceed N;
 *   block is only read.  An entry outside [0, N) is not dereferenced: its row of out is zero words.
 * dt_rows_put (replaces deeptable.py:455, `oof_proba[idx] = fold_oof_proba` on the host): block[idx[i], :] = src[i, :] for src
 *   [n, C].  A row idx does not name keeps its bits; an entry outside [0, N) is skipped; duplicate entries are a caller error
 *   (one of them wins, nothing faults).
 * dt_ensemble_mean (replaces deeptable.py:456-465, the running `proba_mean += fold_proba / num_folds`, and deeptable.py:549-552,
 *   predict_proba's `proba_avg += proba; proba_avg /= len(models)`): parts_host is a HOST array of K DEVICE pointers to float32
 *   [total], 1 <= K <= 64, which travel in the kernel's argument struct (no table copy: the launch can be captured).
 *   mode 0: out float64 [total] = (sum_k (double)p_k) / K; mode 1: out float32 [total] = sum_k (p_k / (float)K) in float32 with a
 *   correctly rounded division.  Each thread sums its element in the order k = 0..K-1 (mode 0 from +0, mode 1 from its first
 *   quotient): no atomics, the same bits on every run.  Parts may alias each other.
 * One thread per word (16-byte words where C % 4 == 0 and both pointers are 16-byte aligned), 256-thread blocks, a grid-stride
 * loop under 2048 blocks, 64-bit element indices.  Nothing synchronises with the host or allocates.  N < 0, C < 1, n < 0,
 * K outside [1, 64], total < 0, an unknown mode and a null or misaligned pointer are DT_ERR_INVALID_ARG before any launch;
 * n == 0 (put: N == 0 as well) and total == 0 are DT_OK without one.                                                         */
int dt_rows_take(const void* block, int64_t N, int C, const int64_t* idx, int64_t n, void* out, void* stream);
int dt_rows_put(void* block, int64_t N, int C, const int64_t* idx, int64_t n, const void* src, void* stream);
int dt_ensemble_mean(const void* const* parts_host, int K, int64_t total, int mode, void* out, void* stream);

/* The fitted preprocessor's transform on the device (csrc/prep_transform.hip; ops.prep_transform, the device path of
 * models/preprocessor.py DefaultPreprocessor.transform_feed; replaces deeptables/models/preprocessor.py:249-260, `transform_X`'s
 * pandas steps, and utils/dataset_generator.py:36-72 on numeric columns).  Sources are column-major, one contiguous DEVICE array
 * [N] per raw column in the column's own dtype; the output is one row-major [N, C] block of a resident feed, int32
 * (DT_PREP_OUT_I32) or float32 (DT_PREP_OUT_F32).  Column j of the block is what cols[j] describes:
 *   DT_PREP_LOOKUP  the raw value widened to a 64-bit key — ints sign-extended, uints and bool zero-extended, float32 bits
 *     zero-extended, float64 bits, every NaN the canonical quiet NaN (0x7FC00000 / 0x7FF8000000000000) — searched in
 *     keys (uint64 [n_keys], ascending); a hit at p gives ids[p], a miss gives `miss`.  n_keys may be 0.
 *   DT_PREP_CONT    v = (double)x; flags & DT_PREP_IMPUTE and v is NaN: v = fill; flags & DT_PREP_SCALE: v = (v - min) / range
 *     in float64, each operation correctly rounded; the word is (float)v.  Integers go int -> double -> float.
 *   DT_PREP_BIN     v as for CONT before its last cast; the word is the number of edges (float64 [n_edges], ascending) <= v,
 *     n_edges for a NaN — np.searchsorted(edges, v, side='right').  n_edges may be 0.
 *   DT_PREP_COPY    the low 32 bits of an integer (or bool) source: `.astype(int64)` followed by `.to(int32)`.
 * An int32 block takes LOOKUP, BIN and COPY columns, a float32 block CONT columns.
 * cols is the DEVICE copy of the descriptors the kernel reads, cols_host the HOST copy the entry validates (the same C
 * descriptors; the pointers inside both are device pointers).  One launch per block: 256-thread blocks, a tile of
 * DT_PREP_TILE_ROWS rows by DT_PREP_CHUNK_COLS columns staged through LDS so that sources are read and rows are written
 * coalesced (16-byte stores where C % 4 == 0 and out is 16-byte aligned), a grid-stride loop under DT_PREP_MAX_BLOCKS blocks,
 * 64-bit row indices, a fixed-trip binary search, no atomics: the same bits on every run.  Nothing synchronises with the host
 * or allocates.  N < 0, C < 1, an unknown out_kind, a null or misaligned pointer, and in cols_host an unknown dtype or op code,
 * an op that does not fit out_kind, COPY of a float source, unknown flags, n_keys < 0 or n_edges < 0, a null source (N > 0), a
 * null or misaligned table of a non-empty LOOKUP / BIN are DT_ERR_INVALID_ARG before any launch; N == 0 is DT_OK without one.
 * The kernel itself gives a zero word for a dtype or op code it does not know and treats a null or negative table as empty. */
#define DT_PREP_BOOL 0
#define DT_PREP_I8 1
#define DT_PREP_I16 2
#define DT_PREP_I32 3
#define DT_PREP_I64 4
#define DT_PREP_U8 5
#define DT_PREP_U16 6
#define DT_PREP_U32 7
#define DT_PREP_U64 8
#define DT_PREP_F32 9
#define DT_PREP_F64 10
#define DT_PREP_DTYPE_COUNT 11
#define DT_PREP_LOOKUP 0
#define DT_PREP_CONT 1
#define DT_PREP_BIN 2
#define DT_PREP_COPY 3
#define DT_PREP_IMPUTE 0x1
#define DT_PREP_SCALE 0x2
#define DT_PREP_OUT_I32 0
#define DT_PREP_OUT_F32 1
#define DT_PREP_TILE_ROWS 256
#define DT_PREP_CHUNK_COLS 32
#define DT_PREP_MAX_BLOCKS 1024
#define DT_PREP_COL_BYTES 80
typedef struct dt_prep_col {
    const void* src;        /* device [N] of `dtype` */
    const uint64_t* keys;   /* LOOKUP: device uint64 [n_keys], ascending */
    const int32_t* ids;     /* LOOKUP: device int32 [n_keys] */
    const double* edges;    /* BIN: device float64 [n_edges], ascending */
    double fill, min, range;
    int32_t dtype, op, n_keys, n_edges, miss, flags;
} dt_prep_col;
int dt_prep_transform(int64_t N, const dt_prep_col* cols, const dt_prep_col* cols_host, int C, int out_kind, void* out,
                      void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DT_HIP_H */
