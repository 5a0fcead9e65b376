# -*- coding:utf-8 -*-
"""Fused train-step plans: when the graph DeepModel assembled is one the library has a whole-step
kernel sequence for, `DeepModel.train_step` runs that instead of the layer-by-layer autograd
path.  Same weights, same gradients (tests/test_fused_gpu.py checks both against the oracle).

DeepFM (nets ['linear','fm_nets','dnn_nets'], deepnets.py:15) -> `dt_deepfm_train_step`
(csrc/deepfm.hip): four launches (five for a step that prepares itself) instead of ~60, the optimizer inside them, the
sparse gradient deduplicated in the step; consecutive steps of a captured execution are CHAINED (`can_chain`); under
`parallel.ShardedEmbeddingStrategy` the same kernels run on rows gathered by their owning ranks.
"""
import ctypes
import os

import torch

from . import _lib
from ._lib import check, lib, ptr, stream_ptr
from .ops import SparseRowGrad, autoint_mfma_mode
from .utils import consts

def _step_loss(dm):
    """loss flag of the fused steps: 0 = binary task with BinaryCrossentropy, DT_STEP_LOSS_MSE = regression task with
    'mse' (deepmodel.py:126-141), None = a task / loss the steps do not take"""
    ln = getattr(dm, 'loss_name', None)
    if dm.task == consts.TASK_BINARY and ln == 'binary_crossentropy':
        return 0
    if dm.task == consts.TASK_REGRESSION and ln in ('mse', 'mean_squared_error'):
        return _lib.DT_STEP_LOSS_MSE
    return None


TILE_H1, TILE_H2 = 128, 64         # the tower widths the step's kernels are compiled for (csrc/tile_common.h kH1 / kH2)


def _tower_widths(dnn_params):
    """(H1, H2) when the tower is one the fused steps take — two Dense(bias) -> relu cells without dropout / batch norm
    whose widths fit the compiled 128 x 64 tile (deepnets.py:401-427) — else None.  Narrower towers run on the same
    kernels: the plan stores W1 / b1 / W2 / b2 / w3 inside zero-padded [C,128] / [128] / [128,64] / [64] / [64] slabs and
    the model's parameters are the leading blocks of those slabs (views).  A padded unit has zero weights and bias, so
    its activation, every gradient that touches it and its Adam moments stay exactly zero."""
    hu = tuple(tuple(h) for h in dnn_params.get('hidden_units', ()))
    if len(hu) != 2 or any(len(h) != 3 for h in hu):
        return None
    (h1, d1, bn1), (h2, d2, bn2) = hu
    if d1 or d2 or bn1 or bn2 or not (1 <= int(h1) <= TILE_H1 and 1 <= int(h2) <= TILE_H2):
        return None
    if dnn_params.get('activation', 'relu') != 'relu' or dnn_params.get('custom_dnn_fn') is not None:
        return None
    return int(h1), int(h2)


def _tower_mfma_flag(dnn_params):
    """`dnn_params['mfma_dtype']` (or DT_AMD_TOWER_DTYPE): 'bf16x3' (default) = the tile kernel's four GEMMs on split-bf16
    matrix cores (csrc/tower_x3.h, DT_STEP_TOWER_X3: three bf16 parts = all 24 mantissa bits in the forward, two parts in the
    backward, fp32 accumulate — measured at the exact kernels' parity bars), 'f32' = exact-fp32 MFMA,
    'bf16' = plain bf16 operands (1e-2 of the oracle: an opt-in precision mode) -> the `phases` bit of the fused step"""
    mode = dnn_params.get('mfma_dtype') or os.environ.get('DT_AMD_TOWER_DTYPE', 'bf16x3')
    if mode in ('f32', 'fp32', 'float32'):
        return 0
    if mode == 'bf16x3':
        return _lib.DT_STEP_TOWER_X3
    if mode in ('bf16', 'bfloat16'):         # north_star's "1e-2 bf16": one bf16 product per operand pair (opt-in)
        return _lib.DT_STEP_TOWER_BF16
    raise ValueError(f"dnn_params['mfma_dtype'] = {mode!r}: 'f32', 'bf16x3' or 'bf16'")


def _mirror_in_flat(flat_params, accum, grad_views):
    """Moves every parameter of `grad_views` [(param, view of accum)] to the same place of `flat_params` (same offset,
    shape and strides as its gradient view) -> members for KerasAdam.register_flat_group."""
    members = []
    for p, gview in grad_views:
        off = (gview.data_ptr() - accum.data_ptr()) // 4
        assert tuple(gview.shape) == tuple(p.shape), (tuple(gview.shape), tuple(p.shape))
        pview = torch.as_strided(flat_params, tuple(gview.shape), tuple(gview.stride()), off)
        with torch.no_grad():
            pview.copy_(p.data)
        p.data = pview
        members.append((p, off, p.numel(), (tuple(gview.shape), tuple(gview.stride()))))
    return members


def _dedupe_in_step(plan, B, backward):
    """The in-step dedupe hands the rows looked up several times to the optimizer as SEGMENTS: only for an optimizer that
    takes them, a single process (the data-parallel exchange gathers plain (rows, values)), and row-sparse tables."""
    if not (backward and plan.dedupe and B * plan.F < (1 << 23)):
        return False
    opt = getattr(plan.dm, 'optimizer', None)
    if not getattr(opt, 'supports_row_segments', False):
        return False
    st = plan.dm.config.distribute_strategy
    if st is not None and (int(getattr(st, 'world_size', 1)) > 1 or getattr(st, 'force_dp', False)):
        # data parallel: only with an exchange that packs the segments into unique (row, summed gradient) entries before
        # the all-gather (parallel.DataParallelStrategy.allgather_sparse); DT_AMD_DP_DEDUPE=0: per-lookup entries on the wire
        if not getattr(st, 'compacts_segments', False) or getattr(st, 'sharded_embeddings', False) or \
                os.environ.get('DT_AMD_DP_DEDUPE', '1') == '0':
            return False
    return not plan.emb.uses_dense_grad(plan.D)


def _rows_in_step(plan, B, backward, apply_rows):
    """The pipelined DeepFM step can apply the optimizer's row-sparse update to the rows looked up once INSIDE the step
    (dt_deepfm_train_step_adam): only when the caller promises `optimizer.step()` follows at once (DeepModel.train_step),
    the in-step dedupe is on (single process, row-sparse table), the optimizer is the library's KerasAdam with
    nothing between the gradient and its update (no pending all-reduce hook), and DT_AMD_ROWS_IN_STEP != 0."""
    if not (apply_rows and backward and plan.dm.model.training and _dedupe_in_step(plan, B, backward)):
        return None
    if os.environ.get('DT_AMD_ROWS_IN_STEP', '1') == '0':
        return None
    opt = getattr(plan.dm, 'optimizer', None)
    if not getattr(opt, 'supports_rows_in_step', False) or getattr(opt, 'pre_dense_hook', None) is not None:
        return None
    return opt


def _segments(buf, B, F):
    seg = buf.get('segments')
    if seg is None:
        offs = (ctypes.c_int64 * 7)()
        check(lib().dt_deepfm_dedupe_segments(B, F, ctypes.cast(offs, ctypes.c_void_p)), 'dt_deepfm_dedupe_segments')
        raw = buf['dedupe'].view(torch.uint8)
        E, cap = int(offs[5]), int(offs[6])
        seg = (raw[offs[0]:offs[0] + 4 * E].view(torch.int32), raw[offs[1]:offs[1] + 8 * E * cap].view(torch.int64),
               raw[offs[2]:offs[2] + 4 * E * cap].view(torch.int32), raw[offs[3]:offs[3] + 4 * E * cap].view(torch.int32),
               raw[offs[4]:offs[4] + 4 * E * B].view(torch.int32), E, cap)
        buf['segments'] = seg
    return seg


def fused_enabled():
    return os.environ.get('DT_AMD_FUSED', '1') != '0'


def _row_weights(sample_weight, y):
    """Keras fit's sample_weight x class_weight as the [B] fp32 vector the step's loss block reads (None: unweighted)."""
    if sample_weight is None:
        return None
    w = sample_weight.reshape(-1).to(device=y.device, dtype=torch.float32).contiguous()
    if w.shape[0] != y.shape[0]:
        raise ValueError(f'sample_weight has {w.shape[0]} entries for {y.shape[0]} rows')
    return w


def _step_dims(dm, net_layers, tower=_tower_widths):
    """(batch hint, F, D, Nd), the leading arguments of dt_*_supported, when the graph passes the checks both fused steps
    share — fixed-length columns, a loss the steps take, dropout rates in [0, 1), a tower of the compiled tile (`tower`:
    the predicate of the steps or, for the inference plans, _infer_tower; None: a graph without a tower, which has no
    bn_concat_emb_dense either), the layers `net_layers` besides the embedding / BN / output ones, one embedding group,
    at most one continuous column — else None"""
    c = dm.config
    if dm.var_len_categorical_columns or _step_loss(dm) is None:
        return None
    if not (0 <= float(c.dense_dropout or 0) < 1) or not (0 <= float(c.embedding_dropout or 0) < 1):
        return None
    if tower is not None and tower(c.dnn_params) is None:
        return None
    L = dm.model.layers_by_name
    base = ('emb_categorical_vars_all', 'task_output') + (('bn_concat_emb_dense',) if tower is not None else ())
    if any(n not in L for n in base + tuple(net_layers)):
        return None
    emb = L['emb_categorical_vars_all']
    if len(emb.groups) != 1 or len(dm.continuous_columns or []) > 1:
        return None
    Nd = sum(col.input_dim for col in (dm.continuous_columns or []))
    return max(int(getattr(dm, '_batch_hint', 0) or 0), 1), len(emb.input_dims), emb.groups[0][0], Nd


class FusedDeepFM:
    """Whole-step executor for the DeepFM graph.  Holds the static workspace / gradient buffers.  FusedDCN runs the same
    executor; the net-specific parts are the declarations and hooks marked 'net:' below."""

    NETS = {'linear', 'fm_nets', 'dnn_nets'}
    takes_sample_weight = True                # the loss block scales each row's loss / dlogit (csrc/tile_common.h DcnArgs.sw)
    # net: entry points dt_<PREFIX>_accum_floats / _accum_offsets / _workspace_bytes / _train_step / _train_step_adam, the
    # accumulator entries in dt_<PREFIX>_accum_offsets' order, the tower's two Dense layers
    PREFIX = 'deepfm'
    ACC_NAMES = ('dW1', 'dW2', 'db1', 'db2', 'dw3', 'dwo', 'dbo', 'loss', 'dgamma', 'dbeta', 'dwlin')
    TOWER = ('dnn_dense_1', 'dnn_dense_2')
    STEP_EXTRA = (1.0, 0)                     # dt_deepfm_train_step's grad_rows_scale, grad_rows_field_major
    ROW_OWNED = True                          # run() takes parallel.ShardedEmbeddingStrategy's row-owned path

    @classmethod
    def eligible(cls, dm):
        c = dm.config
        try:
            if set(c.nets) != cls.NETS or len(c.nets) != 3 or c.stacking_op != consts.STACKING_OP_ADD:
                return False
            dims = _step_dims(dm, cls.TOWER + ('linear_logit', 'dense_logit_dnn_nets', 'fm_layer'))
            return dims is not None and bool(lib().dt_deepfm_supported(*dims, 128, 64))
        except Exception:
            return False

    # -- net: layers, accumulator layout, gradient views and step arguments --------------------------------------------
    def _net_layers(self, L):
        self.lin = L['linear_logit']
        self.dl = L['dense_logit_dnn_nets']

    def _dims(self):
        return self.F, self.D, self.Nd

    def _net_grad_views(self, H2):
        """-> ([(parameter, its gradient's view of accum)] of the net's own parameters, floats of the flat group)"""
        a, o, n = self.accum, self.off, self.F + self.Nd
        return [(self.dl.kernel, a[o['dw3']:o['dw3'] + H2].view(H2, 1)),
                (self.out.kernel, a[o['dwo']:o['dwo'] + 1].view(1, 1)),
                (self.lin.kernel, a[o['dwlin']:o['dwlin'] + n].view(n, 1))], o['dwlin'] + n

    def _net_args(self):
        """the arguments between Nd and bn_gamma"""
        return (ptr(self.lin.kernel),)

    def _head_weights(self):
        """(w3, w_out)"""
        return ptr(self.dl.kernel), ptr(self.out.kernel)

    # -------------------------------------------------------------------------------------------------------------------
    def __init__(self, dm):
        self.dm = dm
        L = dm.model.layers_by_name
        self.emb = L['emb_categorical_vars_all']
        self.bn = L['bn_concat_emb_dense']
        self.d1, self.d2 = L[self.TOWER[0]], L[self.TOWER[1]]
        self.out = L['task_output']
        self.D = self.emb.groups[0][0]
        self.F = len(self.emb.input_dims)
        self.Nd = sum(col.input_dim for col in (dm.continuous_columns or []))
        self.C = self.F * self.D + self.Nd
        self.key = f'd{self.D}'
        self.device = self.emb.tables[self.key].device
        self._net_layers(L)
        n_acc = self._entry('accum_floats')(*self._dims())
        offs = (ctypes.c_int64 * len(self.ACC_NAMES))()
        check(self._entry('accum_offsets')(*self._dims(), ctypes.cast(offs, ctypes.c_void_p)),
              f'dt_{self.PREFIX}_accum_offsets')
        self.off = dict(zip(self.ACC_NAMES, [int(v) for v in offs]))
        self.accum = torch.zeros(n_acc, dtype=torch.float32, device=self.device)
        self._bufs = {}
        a, o, C = self.accum, self.off, self.C
        H1, H2 = _tower_widths(dm.config.dnn_params)       # <= the compiled tile: the slabs are zero padded
        net_views, n_flat = self._net_grad_views(H2)
        self.grad_views = [
            (self.d1.kernel, a[o['dW1']:o['dW1'] + C * TILE_H1].view(C, TILE_H1)[:, :H1]),
            (self.d2.kernel, a[o['dW2']:o['dW2'] + TILE_H1 * TILE_H2].view(TILE_H1, TILE_H2)[:H1, :H2]),
            (self.d1.bias, a[o['db1']:o['db1'] + H1]),
            (self.d2.bias, a[o['db2']:o['db2'] + H2]),
            (self.bn.gamma, a[o['dgamma']:o['dgamma'] + C]),
            (self.bn.beta, a[o['dbeta']:o['dbeta'] + C]),
        ] + net_views
        if self.out.bias is not None:
            self.grad_views.append((self.out.bias, a[o['dbo']:o['dbo'] + 1]))
        self.loss_view = a[o['loss']:o['loss'] + 1]
        # embedding_dropout (config.py:84): element dropout inside the step's kernels; the seed word lives on the device
        # and is advanced by the step (a captured graph draws a new mask at every replay)
        self.emb_dropout = float(dm.config.embedding_dropout or 0)
        # dense_dropout (config.py:83): Dropout on the continuous input columns, masked where kernel A packs them
        self.dense_dropout = float(dm.config.dense_dropout or 0) if self.Nd else 0.0
        seed = int(torch.randint(1, 2 ** 31 - 1, (1,)).item())
        self.drop_seed = torch.tensor([seed], dtype=torch.int32, device=self.device)
        # duplicate lookups are resolved inside the step (kernels A and G) unless DT_AMD_FUSED_DEDUPE=0
        self.dedupe = os.environ.get('DT_AMD_FUSED_DEDUPE', '1') != '0'
        self.tower_flag = _tower_mfma_flag(dm.config.dnn_params)
        # diagnostic: s_memtime phase stamps into the workspace (tools/phase_times.py sets DT_AMD_STEP_STAMPS=1)
        self.diag_flag = _lib.DT_STEP_STAMPS if os.environ.get('DT_AMD_STEP_STAMPS') == '1' else 0
        # Parameters mirror the gradient layout in one flat buffer, so the optimizer updates every dense layer of
        # the model with ONE launch over (flat_params, accum) instead of one launch per tensor.
        self.flat_params = torch.zeros_like(self.accum)
        members = _mirror_in_flat(self.flat_params, a, self.grad_views)
        opt = getattr(dm, 'optimizer', None)
        if opt is not None and hasattr(opt, 'register_flat_group'):
            opt.register_flat_group(self.flat_params, self.accum, members, n_flat)
        dm.model._dt_flat_grad = self.accum     # lets DataParallelStrategy all-reduce the gradients in place

    def _entry(self, what):
        return getattr(lib(), f'dt_{self.PREFIX}_{what}')

    def _buffers(self, B):
        b = self._bufs.get(B)
        if b is None:
            nbytes = self._entry('workspace_bytes')(B, *self._dims())
            if nbytes < 0:
                raise _lib.DtHipError(f'fused {type(self).__name__[len("Fused"):]} step: unsupported shape')
            dev = self.device
            b = {'ws': torch.zeros((nbytes + 3) // 4, dtype=torch.float32, device=dev),   # zero-filled once: the batch-sum accumulators
                 'logit': torch.empty((B, 1), dtype=torch.float32, device=dev),
                 'grad_rows': torch.empty((B, self.F, self.D), dtype=torch.float32, device=dev),
                 **self._id_state(B)}
            self._bufs[B] = b
        return b

    def _id_state(self, B):
        """the lookups' rows and the in-step dedupe's scratch: field-major rows + the segment arrays (csrc/deepfm.hip
        DedupeWs)"""
        return {'rows': torch.empty((B, self.F), dtype=torch.int64, device=self.device),
                'dedupe': torch.zeros((lib().dt_deepfm_dedupe_bytes(B, self.F) + 7) // 8, dtype=torch.int64,
                                      device=self.device),
                'dedupe_slots': lib().dt_deepfm_dedupe_slots(B, self.F)}

    # -- per-slot id state: the compiled loop (compiled.CompiledTrainLoop) keeps k steps in one hipGraph and runs the ids-only
    #    work of steps 2..k ahead of them; every captured step then needs its OWN rows / segment buffers --------------------
    def _slot_buffers(self, B, slot):
        buf = self._buffers(B)
        if not slot:
            return buf
        slots = buf.setdefault('slots', {})
        if slot not in slots:
            slots[slot] = self._id_state(B)
        return slots[slot]

    def check_dedupe(self):
        """Host check of the in-step dedupe (reads one word per batch size back: call it outside the step — `DeepModel.fit`
        does at the end of every epoch, bench.py after the timed region): raises when an election block of a batch beyond
        8192 rows found its 8192-slot table full, i.e. some duplicate lookups of that step were treated as distinct rows.
        Needs > 8192 distinct rows of ONE field hashing to ONE of its B / 1024 partitions: not reachable by chance."""
        for B, buf in self._bufs.items():
            if not isinstance(B, int) or 'dedupe' not in buf:
                continue
            off = int(lib().dt_deepfm_dedupe_overflow_offset(B, self.F))
            bufs = [buf] + list(buf.get('slots', {}).values())
            for b in bufs:
                n = int(b['dedupe'].view(torch.int32)[off // 4].item())
                if n:
                    raise _lib.DtHipError(f'in-step dedupe: {n} lookups found their election table full (batch {B})')

    def can_preelect(self, B):
        """the step's ids-only half can run ahead of it (dt_deepfm_preelect): in-step dedupe on, single process"""
        st = self.dm.config.distribute_strategy
        # OFF by default (DT_AMD_PREELECT=1 turns it on).  Measured (tools/r4/call7.sh): a forked branch of a captured hipGraph
        # does not run beside the main branch on this stack — the executor ran the nine elections first, on one queue, then
        # alternated queues per step with ~9.5 us joins: 131.9 us per step against 109.5 us with every step electing for
        # itself.  The entry point stays for a caller that owns a second stream outside a graph.
        return bool(st is None and _dedupe_in_step(self, B, True) and os.environ.get('DT_AMD_PREELECT', '0') == '1')

    def preelect(self, idx, slot):
        """rows + segments of batch `idx` into slot `slot`'s buffers, on the current stream; the step that follows is run
        with `run(..., slot=slot, preelected=True)`"""
        B = idx.shape[0]
        sb = self._slot_buffers(B, slot)
        idx = idx.contiguous()
        kind = _lib.DT_IDX_F32 if idx.dtype == torch.float32 else _lib.DT_IDX_I32
        if idx.dtype not in (torch.float32, torch.int32):
            raise ValueError('preelect: ids must be float32 or int32')
        check(lib().dt_deepfm_preelect(ptr(idx), kind, ptr(getattr(self.emb, f'row_offset_{self.key}')),
                                       ptr(getattr(self.emb, f'vocab_{self.key}')), B, self.F, ptr(sb['rows']),
                                       ptr(sb['dedupe']), sb['dedupe_slots'], stream_ptr()), 'dt_deepfm_preelect')

    # -- the arguments of the step's entry points ------------------------------------------------------------------------
    def _phases(self, backward=True, part=0, pre=0, diag=True):
        """the `phases` word: forward (1) or backward (2) step | the split-finish part | the loss | pre-elected / prepared
        bits | the tower's matrix-core mode and (diag) the phase stamps, for a backward step other than the finish alone"""
        phases = (2 if backward else 1) | part | _step_loss(self.dm) | pre
        if backward and part != _lib.DT_STEP_FINISH_ONLY:
            phases |= self.tower_flag | (self.diag_flag if diag else 0)
        return phases

    def _head(self, ids, kind, rows_src, dense, y, B, logit, rows, buf, oob, dedupe, dedupe_slots):
        """the arguments every step entry point starts with, up to dedupe_slots; rows_src = (table, row_offset, vocab)"""
        training, bn = self.dm.model.training, self.bn
        return (ptr(ids), kind, *[ptr(t) for t in rows_src], ptr(dense), ptr(y), B, self.F, self.D, self.Nd,
                *self._net_args(), ptr(bn.gamma), ptr(bn.beta), ptr(bn.moving_mean) if training else None,
                ptr(bn.moving_variance) if training else None, float(bn.epsilon), float(bn.momentum), ptr(self.d1.kernel),
                ptr(self.d1.bias), ptr(self.d2.kernel), ptr(self.d2.bias), *self._head_weights(), ptr(self.out.bias),
                ptr(logit), ptr(rows), ptr(buf['grad_rows']), ptr(self.accum), ptr(buf['ws']), oob, dedupe, dedupe_slots)

    def _tail(self, phases, sw):
        """phases and the per-step inputs that follow it in every entry point"""
        training = self.dm.model.training
        return (phases, self.emb_dropout if training else 0.0, ptr(self.drop_seed),
                self.dense_dropout if training else 0.0, ptr(sw))

    # -- model-parallel tables (parallel.ShardedEmbeddingStrategy) --------------------------------------
    def _sharded_buffers(self, B, st):
        key = ('sharded', B)
        sb = self._bufs.get(key)
        if sb is None:
            dev, F, D, W = self.device, self.F, self.D, st.world_size
            s, e = st.field_bounds(F)[st.rank]
            Fo = e - s
            f_idx = torch.arange(F, device=dev, dtype=torch.int32)
            b_idx = torch.arange(B, device=dev, dtype=torch.int32)
            sb = {'Fo': Fo, 's': s, 'e': e,
                  # the received rows [F,B,D] are read by the fused step as a "table" of F*B rows: id(b,f) = f*B + b
                  'iota': (f_idx[None, :] * B + b_idx[:, None]).contiguous(),
                  'zero_off': torch.zeros(F, dtype=torch.int64, device=dev),
                  'fb_vocab': torch.full((F,), F * B, dtype=torch.int32, device=dev),
                  'emb_own': torch.empty((W * Fo * B, 1, D), dtype=torch.float32, device=dev),
                  'rows_own': torch.empty((W * Fo * B, 1), dtype=torch.int64, device=dev),
                  'emb_T': torch.empty((F * B, D), dtype=torch.float32, device=dev),
                  'grad_own': torch.empty((W * Fo * B, D), dtype=torch.float32, device=dev),
                  'rows_dummy': torch.empty((B, F), dtype=torch.int64, device=dev)}
            self._bufs[key] = sb
        return sb

    def _run_sharded(self, idx, dense, y, st, sample_weight=None):
        """One train step with the table rows owned per field by the ranks of `st` (see ShardedEmbeddingStrategy):
        ids all-gather -> owner gather -> all-to-all -> the same fused kernels on the local minibatch (reading the
        received rows) -> all-to-all of the row gradients -> the owner's sparse gradient.  Three pieces so that a caller
        can capture the kernels between the collectives into hipGraphs (bench.py): `sharded_pre` (collectives + the
        owner's gather, eager), `sharded_core` (the step's kernels: capturable), `sharded_post` (collective, eager)."""
        self.sharded_pre(idx, st)
        if os.environ.get('DT_AMD_SHARDED_OVERLAP', '0') != '1':
            out = self.sharded_core(idx.shape[0], dense, y, st, sample_weight)
            self.sharded_post(idx.shape[0], st)
            return out
        # opt-in (DT_AMD_SHARDED_OVERLAP=1): the row gradients are final one launch before the step is, so their all-to-all
        # can start there and the step's last launch (the dense gradients' last level, ~7 us) run beside it.  Measured at
        # world size 1 through RCCL (gpurun_out/r3c23): 214 us against 171 us for the plain order — the two stream
        # hand-overs cost more than the launch they hide — so the plain order is the default.
        out = self.sharded_core(idx.shape[0], dense, y, st, sample_weight, part=_lib.DT_STEP_SKIP_FINISH)
        work = self.sharded_post(idx.shape[0], st, async_op=True)
        self.sharded_core(idx.shape[0], dense, y, st, sample_weight, part=_lib.DT_STEP_FINISH_ONLY)
        if work is not None:
            work.wait()               # stream-ordered: the launches that follow (the owner's row update) see the received rows
        return out

    def sharded_pre(self, idx, st):
        B, F, D, W = idx.shape[0], self.F, self.D, st.world_size
        sb = self._sharded_buffers(B, st)
        if idx.dtype != torch.int32:
            idx = idx.to(torch.int32)             # float ids: truncation, as the gather's own cast
        table = self.emb.tables[self.key]
        row_offset = getattr(self.emb, f'row_offset_{self.key}')
        vocab = getattr(self.emb, f'vocab_{self.key}')
        s, e, Fo = sb['s'], sb['e'], sb['Fo']
        idx_all = st.gather_all_ids(idx.contiguous())                                 # [W, B, F] int32
        check(lib().dt_embedding_gather_owned(ptr(idx_all), _lib.DT_IDX_I32, ptr(table), ptr(row_offset), ptr(vocab),
                                              W, B, F, s, e, D, ptr(sb['emb_own']), ptr(sb['rows_own']),
                                              ptr(self.emb.oob_count) if self.emb.check_oob else None, stream_ptr()),
              'dt_embedding_gather_owned')
        st.forward_exchange(sb['emb_own'].view(W, Fo, B, D), F, B, out=sb['emb_T'])

    def sharded_core(self, B, dense, y, st, sample_weight=None, part=0):
        """the fused step's launches on the received rows (no collective inside: a hipGraph can hold them)"""
        buf = self._buffers(B)
        sb = self._sharded_buffers(B, st)
        dense = None if dense is None else dense.contiguous()
        y = y.reshape(-1).contiguous()
        sw = _row_weights(sample_weight, y)
        head = self._head(sb['iota'], _lib.DT_IDX_I32, (sb['emb_T'], sb['zero_off'], sb['fb_vocab']), dense, y, B,
                          buf['logit'], sb['rows_dummy'], buf, None, None, 0)
        check(lib().dt_deepfm_train_step(*head, 1.0 / st.world_size, 1, *self._tail(self._phases(part=part), sw),
                                         stream_ptr()), 'dt_deepfm_train_step')
        for p, g in self.grad_views:
            p.grad = g
        self.dm.model._dt_sharded_step = True
        return self.loss_view, buf['logit']

    def sharded_post(self, B, st, async_op=False):
        # the loss is a mean over the LOCAL minibatch, the global objective the mean over W of them: the step already
        # wrote the row gradients field-major [F,B,D] and divided by W
        F, D = self.F, self.D
        buf = self._buffers(B)
        sb = self._sharded_buffers(B, st)
        if async_op:
            grad_own, work = st.backward_exchange(buf['grad_rows'].view(F, B, D), F, B, out=sb['grad_own'], async_op=True)
        else:
            grad_own, work = st.backward_exchange(buf['grad_rows'].view(F, B, D), F, B, out=sb['grad_own']), None
        self.emb.sparse_grads[self.key] = [SparseRowGrad(sb['rows_own'].view(-1), grad_own.view(-1, D), fields=0)]
        return work

    def _whole_in_step(self, opt):
        """the optimizer's flat dense group is this plan's: the step's last launch runs the whole optimizer step"""
        table = self.emb.tables[self.key]
        flat = getattr(opt, '_flat', None)
        return bool(flat is not None and flat[0] is self.flat_params and flat[1] is self.accum and
                    os.environ.get('DT_AMD_STEP_IN_STEP', '1') != '0' and
                    all(id(p) in flat[5] for p in opt.params if p is not table))

    def can_chain(self, B):
        """consecutive steps of one captured execution can be CHAINED (csrc/deepfm.hip StepNext): step i packs step i + 1's
        rows, runs its election on the weight-gradient launch's idle matrix waves and writes the tile kernel's weight layouts
        from the weights it has just updated — step i + 1 then has no prep launch (four launches).  Single process, in-step
        dedupe and optimizer, split-bf16 tower, B <= 8192; DT_AMD_CHAIN=0 turns it off."""
        if os.environ.get('DT_AMD_CHAIN', '1') == '0' or self.dm.config.distribute_strategy is not None:
            return False
        opt = _rows_in_step(self, B, True, True) if _dedupe_in_step(self, B, True) else None
        if opt is None or not self._whole_in_step(opt):
            return False
        return bool(lib().dt_deepfm_step_chains(B, self.F, self.D, self.Nd, self._phases(diag=False)))

    def _id_buffers(self, idx, backward, dedupe, opt, slot, preelected, next_ids, prepared):
        """-> (this step's rows / segment buffers, its pre-elected / prepared bits, the pointers of the next step's ids, rows
        and segment buffers when this step prepares it)"""
        B = idx.shape[0]
        ids = self._slot_buffers(B, slot) if (slot and dedupe) else self._buffers(B)
        pre = _lib.DT_STEP_PREELECTED if (preelected and dedupe and backward) else 0
        if preelected and not pre:
            raise _lib.DtHipError('a pre-elected step needs the in-step dedupe (backward, single process)')
        nxt = (None, None, None)
        if prepared or next_ids is not None:
            if opt is None or not dedupe:
                raise _lib.DtHipError('chained steps need the in-step dedupe and optimizer (can_chain)')
            if prepared:
                pre |= _lib.DT_STEP_PREPARED
            if next_ids is not None:
                nidx, nslot = next_ids
                if nidx.dtype != idx.dtype or nidx.shape != idx.shape or not nidx.is_contiguous() or not nslot or nslot == slot:
                    raise ValueError('next_ids: (contiguous ids like this step\'s, a slot of their own)')
                nb = self._slot_buffers(B, nslot)
                nxt = (ptr(nidx), ptr(nb['rows']), ptr(nb['dedupe']))
        return ids, pre, nxt

    def run(self, idx, dense, y, backward=True, apply_rows=False, sample_weight=None, logit_out=None, slot=0,
            preelected=False, next_ids=None, prepared=False):
        """-> (loss [1] view, logit [B,1]).  slot / preelected: the compiled loop's per-step id buffers (`preelect`).
        next_ids / prepared (chained steps, `can_chain`): next_ids = (ids of the following step, its slot) — this step prepares
        it; prepared: this step was prepared by the one before it (slot's buffers hold its rows / segments).  logit_out: a caller-owned [B,1] fp32 buffer the step writes its logits to (the
        compiled loop keeps one per captured step) instead of the plan's own.  With backward=True fills `.grad` of every dense parameter
        (views of one static buffer) and registers the embedding table's sparse gradient.  apply_rows=True: the caller
        runs `optimizer.step()` right after this call, so the step may update the table rows looked up once itself
        (`_rows_in_step`); the registered sparse gradient then carries `fields = -2` (segments only)."""
        st = self.dm.config.distribute_strategy
        if self.ROW_OWNED and backward and getattr(st, 'sharded_embeddings', False) and st.active and \
                not self.emb.uses_dense_grad(self.D):
            return self._run_sharded(idx, dense, y, st, sample_weight)
        self.dm.model._dt_sharded_step = False
        B = idx.shape[0]
        buf = self._buffers(B)
        idx = idx.contiguous()
        kind = _lib.DT_IDX_F32 if idx.dtype == torch.float32 else _lib.DT_IDX_I32
        if idx.dtype not in (torch.float32, torch.int32):
            idx = idx.to(torch.int32)
        dense = None if dense is None else dense.contiguous()
        y = y.reshape(-1).contiguous()
        sw = _row_weights(sample_weight, y)
        table = self.emb.tables[self.key]
        logit = buf['logit']
        if logit_out is not None:
            if logit_out.shape != logit.shape or logit_out.dtype != logit.dtype or not logit_out.is_contiguous():
                raise ValueError(f'logit_out must be a contiguous float32 {tuple(logit.shape)} tensor')
            logit = logit_out
        dedupe = _dedupe_in_step(self, B, backward)
        opt = _rows_in_step(self, B, backward, apply_rows)
        ids, pre, nxt = self._id_buffers(idx, backward, dedupe, opt, slot, preelected, next_ids, prepared)
        head = self._head(idx, kind, (table, getattr(self.emb, f'row_offset_{self.key}'),
                                      getattr(self.emb, f'vocab_{self.key}')), dense, y, B, logit, ids['rows'], buf,
                          ptr(self.emb.oob_count) if self.emb.check_oob else None,
                          ptr(ids['dedupe']) if dedupe else None, buf['dedupe_slots'])
        if opt is not None:
            # the rows looked up once are updated where their gradient is formed (csrc/deepfm.hip k_wgrad_rows); when the
            # optimizer's flat dense group is this plan's, the step's last launch runs the rest of the optimizer step too
            # (dense elements, segments, the state's advance: k_finish_step) and `optimizer.step()` has nothing left to do
            slots = opt._st(table, rows=True)
            whole = self._whole_in_step(opt)
            flat = opt._flat
            dn = (ptr(flat[0]), ptr(flat[2]), ptr(flat[3]), int(flat[4]), float(opt.lr)) if whole else (None, None, None, 0, 0.0)
            check(self._entry('train_step_adam')(
                *head, *self._tail(self._phases(pre=pre), sw), ptr(slots['m']), ptr(slots['v']), int(slots['m'].stride(0)),
                ptr(opt._state_tensor(table.device)), 0.0, opt.b1, opt.b2, opt.eps, *dn, *nxt, stream_ptr()),
                f'dt_{self.PREFIX}_train_step_adam')
            if whole:
                opt.applied_in_step()
        else:
            check(self._entry('train_step')(*head, *self.STEP_EXTRA, *self._tail(self._phases(backward, pre=pre), sw),
                                            stream_ptr()), f'dt_{self.PREFIX}_train_step')
        if backward:
            for p, g in self.grad_views:
                p.grad = g
            # with the in-step dedupe: rows looked up once keep their entry, the others travel as segments; fields = -2:
            # the entries of `rows` were applied inside the step, the optimizer only walks the segments
            self.emb.sparse_grads[self.key] = [SparseRowGrad(ids['rows'].view(-1), buf['grad_rows'].view(-1, self.D),
                                                             fields=(-2 if opt is not None else -1) if dedupe else None,
                                                             segments=_segments(ids, B, self.F) if dedupe else None)]
            if self.emb.uses_dense_grad(self.D):
                # small tables keep exact dense-Adam semantics: densify the row gradients
                g = torch.zeros_like(table)
                check(lib().dt_embedding_bwd_dense(ptr(ids['rows']), ptr(buf['grad_rows']), B * self.F, self.D,
                                                   ptr(g), stream_ptr()), 'dt_embedding_bwd_dense')
                table.grad = g
                self.emb.sparse_grads.pop(self.key, None)
        return self.loss_view, logit


class FusedDCN(FusedDeepFM):
    """Whole-step executor for the DCN graph (nets ['dcn_nets'], deepnets.py:194-207): the DeepFM kernel sequence with the
    Cross network (layers.py:428-436) running on the BN'd tile inside the tower kernel -> `dt_dcn_train_step`."""

    NETS = {'dcn_nets'}
    PREFIX = 'dcn'
    ACC_NAMES = ('dW1', 'dW2', 'db1', 'db2', 'dw3', 'dwo', 'dbo', 'loss', 'dgamma', 'dbeta', 'dcw', 'dcb')
    TOWER = ('dcn_dense_1', 'dcn_dense_2')
    STEP_EXTRA = ()
    ROW_OWNED = False

    @classmethod
    def eligible(cls, dm):
        c = dm.config
        try:
            # a single net: Concatenate([cross, dnn]) feeds task_output directly (deepmodel.py:286-301), no dense_logit_*
            if list(c.nets) != ['dcn_nets'] or 'dense_logit_dcn_nets' in dm.model.layers_by_name:
                return False
            st = c.distribute_strategy
            if getattr(st, 'sharded_embeddings', False) and getattr(st, 'active', False):
                return False                      # row-owned tables: the layer-by-layer path
            dims = _step_dims(dm, cls.TOWER + ('dcn_cross_layer',))
            if dims is None:
                return False
            nl = int(dm.model.layers_by_name['dcn_cross_layer'].num_cross_layer)
            return bool(lib().dt_dcn_supported(*dims, 128, 64, nl))
        except Exception:
            return False

    def _net_layers(self, L):
        self.cross = L['dcn_cross_layer']
        self.nl = int(self.cross.num_cross_layer)
        self.one = torch.ones(4, dtype=torch.float32, device=self.device)     # the step's w_out: task_output is its w3

    def _dims(self):
        return self.F, self.D, self.Nd, self.nl

    def _net_grad_views(self, H2):
        # W1 / W2 precede the [C + 64] output kernel in the flat group, so they keep their 16-byte alignment whatever C is
        # (the kernels read w3 with scalar loads)
        a, o, C, nl = self.accum, self.off, self.C, self.nl
        return [(self.out.kernel, a[o['dw3']:o['dw3'] + C + H2].view(C + H2, 1)),      # [w3c | w3d], w3d's pad at the end
                (self.cross.kernel_stack, a[o['dcw']:o['dcw'] + nl * C].view(nl, C)),
                (self.cross.bias_stack, a[o['dcb']:o['dcb'] + nl * C].view(nl, C))], o['dcb'] + nl * C

    def _net_args(self):
        return ptr(self.cross.kernel_stack), ptr(self.cross.bias_stack), self.nl

    def _head_weights(self):
        return ptr(self.out.kernel), ptr(self.one)


def make_fused_plan(dm):
    if not fused_enabled() or dm.model is None:
        return None
    if dm.model.has_regularizers():
        return None         # the fused DeepFM / DCN steps have no penalty term: a regularised model trains on the layer path
    if FusedDeepFM.eligible(dm):
        return FusedDeepFM(dm)
    if FusedDCN.eligible(dm):
        return FusedDCN(dm)
    return None


# ---- inference -----------------------------------------------------------------------------------------------------------
def predict_enabled():
    """the inference plans are on unless DT_AMD_FUSED=0 or DT_AMD_FUSED_PREDICT=0"""
    return fused_enabled() and os.environ.get('DT_AMD_FUSED_PREDICT', '1') != '0'


def _infer_tower(dnn_params):
    """(H1, H2, cells) when the tower is one the inference kernels take — two relu cells whose widths fit the compiled
    128 x 64 tile, as for the steps, but with any dropout rate (the identity at inference) and with or without batch norm
    (Dense without bias -> BatchNormalization -> relu, deepnets.py:401-427; at inference a per-column affine map):
    cells = bit i set when cell i + 1 has one — else None"""
    hu = tuple(tuple(h) for h in dnn_params.get('hidden_units', ()))
    if len(hu) != 2 or any(len(h) != 3 for h in hu):
        return None
    (h1, d1, bn1), (h2, d2, bn2) = hu
    if not (0 <= float(d1 or 0) < 1 and 0 <= float(d2 or 0) < 1) or not (1 <= int(h1) <= TILE_H1 and 1 <= int(h2) <= TILE_H2):
        return None
    if dnn_params.get('activation', 'relu') != 'relu' or dnn_params.get('custom_dnn_fn') is not None:
        return None
    return int(h1), int(h2), (1 if bn1 else 0) | (2 if bn2 else 0)


class InferDeepFM:
    """Inference plan for the DeepFM graph: `prepare` writes the weight layouts (one launch, csrc/infer_x3.h k_infer_prep)
    from the parameters as they are at that moment, `infer` scores one batch (one launch, k_infer).  Needs nothing of the
    training plan: it builds no FusedDeepFM, re-homes no parameter and touches no optimizer state; every pointer, leading
    dimension, moving statistic and epsilon is read in `prepare`, so it follows a training plan that re-homes the tower
    afterwards.  InferDCN runs the same code; the net-specific parts are marked 'net:'."""

    # net: entry points dt_<PREFIX>_infer*, the tower's layer prefix, the layers besides embedding / BN / output
    NETS = FusedDeepFM.NETS
    PREFIX = 'deepfm'
    CELL = 'dnn'
    NET_LAYERS = ('linear_logit', 'dense_logit_dnn_nets', 'fm_layer')

    @classmethod
    def _graph_ok(cls, dm):
        c = dm.config
        return set(c.nets) == cls.NETS and len(c.nets) == 3 and c.stacking_op == consts.STACKING_OP_ADD

    @classmethod
    def eligible(cls, dm):
        c = dm.config
        try:
            if not cls._graph_ok(dm) or getattr(c.distribute_strategy, 'sharded_embeddings', False):
                return False
            tower = _infer_tower(c.dnn_params)
            dims = _step_dims(dm, (f'{cls.CELL}_dense_1', f'{cls.CELL}_dense_2') + cls.NET_LAYERS, _infer_tower)
            return dims is not None and bool(cls._supported(dm, dims[1:], tower))
        except Exception:
            return False

    @classmethod
    def _supported(cls, dm, dims, tower):
        return lib().dt_deepfm_infer_supported(*dims, *tower)

    def _net_layers(self, L):
        self.lin = L['linear_logit']
        self.dl = L['dense_logit_dnn_nets']

    def _dims(self):
        return self.F, self.D, self.Nd

    def _net_args(self):
        """dt_*_infer_prepare's arguments between Nd and bn_gamma"""
        return (ptr(self.lin.kernel),)

    def _head_weights(self):
        """(w3, w_out) of dt_*_infer_prepare"""
        return ptr(self.dl.kernel), ptr(self.out.kernel)

    # -------------------------------------------------------------------------------------------------------------------
    def __init__(self, dm):
        self.dm = dm
        L = dm.model.layers_by_name
        self.emb = L['emb_categorical_vars_all']
        self.out = L['task_output']
        self.D = self.emb.groups[0][0]
        self.F = len(self.emb.input_dims)
        self.Nd = sum(col.input_dim for col in (dm.continuous_columns or []))
        self.key = f'd{self.D}'
        self.device = self.emb.tables[self.key].device
        self._tower_layers(L)
        self._net_layers(L)
        nbytes = self._entry('infer_workspace_bytes')(*self._dims())
        if nbytes < 0:
            raise _lib.DtHipError(f'{type(self).__name__}: unsupported shape')
        self.ws = torch.zeros((nbytes + 3) // 4, dtype=torch.float32, device=self.device)
        self.flags = 0

    def _entry(self, what):
        return getattr(lib(), f'dt_{self.PREFIX}_{what}')

    def _tower_layers(self, L):
        self.bn = L['bn_concat_emb_dense']
        self.cells = [(L[f'{self.CELL}_dense_{i}'], L.get(f'{self.CELL}_bn_{i}')) for i in (1, 2)]

    def _tower_args(self):
        """dt_*_infer_prepare's arguments from bn_gamma to c2_eps: the input BN and the two tower cells as they are now"""
        bn = self.bn
        return (ptr(bn.gamma), ptr(bn.beta), ptr(bn.moving_mean), ptr(bn.moving_variance), float(bn.epsilon)) + \
            self._cell_args()

    def _cell_args(self):
        """dt_*_infer_prepare's arguments from W1 to c2_eps: the two tower cells as they are now"""
        def ld(w):
            if w.dim() != 2 or w.stride(1) != 1:
                raise _lib.DtHipError(f'inference plan: tower kernel with strides {tuple(w.stride())}')
            return int(w.stride(0))

        def cell_bn(b):
            if b is None:
                return None, None, None, None, 0.0
            return ptr(b.gamma), ptr(b.beta), ptr(b.moving_mean), ptr(b.moving_variance), float(b.epsilon)

        (d1, bn1), (d2, bn2) = self.cells
        cells = (1 if bn1 is not None else 0) | (2 if bn2 is not None else 0)
        return (ptr(d1.kernel), ld(d1.kernel), int(d1.kernel.shape[1]), ptr(d1.bias),
                ptr(d2.kernel), ld(d2.kernel), int(d2.kernel.shape[1]), ptr(d2.bias), cells, *cell_bn(bn1), *cell_bn(bn2))

    def _sigmoid(self):
        """DT_INFER_SIGMOID when the output activation is the sigmoid (the binary task), else 0"""
        return _lib.DT_INFER_SIGMOID if self.dm.output_activation == 'sigmoid' else 0

    def _tower_flags(self):
        """dt_*_infer's flags of a plan with a tower: the output activation and the tower's precision mode
        (`_tower_mfma_flag`: 'bf16' -> DT_INFER_TOWER_BF16; 'bf16x3' and 'f32' both run the six-product forward, which is in
        the fp32 class)"""
        mode = _tower_mfma_flag(self.dm.config.dnn_params)
        return self._sigmoid() | (_lib.DT_INFER_TOWER_BF16 if mode == _lib.DT_STEP_TOWER_BF16 else 0)

    def _gather_args(self, idx, kind):
        """the five arguments every dt_*_infer starts with: ids, their DT_IDX_* kind, table, row offsets, vocabulary sizes"""
        return (ptr(idx), kind, ptr(self.emb.tables[self.key]), ptr(getattr(self.emb, f'row_offset_{self.key}')),
                ptr(getattr(self.emb, f'vocab_{self.key}')))

    def _oob(self):
        """the out-of-range counter, or None when the embedding layer does not count"""
        return ptr(self.emb.oob_count) if self.emb.check_oob else None

    def prepare(self):
        """the current weights and moving statistics -> the workspace layouts, one launch on the current stream; also reads
        the precision mode and the output activation (the flags of the `infer` calls that follow)"""
        self.flags = self._tower_flags()
        check(self._entry('infer_prepare')(
            self.F, self.D, self.Nd, *self._net_args(), *self._tower_args(),
            *self._head_weights(), ptr(self.out.bias), ptr(self.ws), stream_ptr()), f'dt_{self.PREFIX}_infer_prepare')

    @staticmethod
    def _batch_args(idx, dense, logit, out):
        """(B, ids as contiguous float32 / int32, their DT_IDX_* kind, dense as contiguous float32 or None) of one `infer`
        call; refuses output buffers that are not contiguous float32 of B rows"""
        B = idx.shape[0]
        idx = idx.contiguous()
        if idx.dtype not in (torch.float32, torch.int32):
            idx = idx.to(torch.int32)
        kind = _lib.DT_IDX_F32 if idx.dtype == torch.float32 else _lib.DT_IDX_I32
        dense = None if dense is None else dense.to(torch.float32).contiguous()
        for t in (logit, out):
            if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != B):
                raise ValueError(f'infer: outputs must be contiguous float32 buffers of {B} rows')
        return B, idx, kind, dense

    def infer(self, idx, dense, logit, out=None):
        """one batch: ids [B, F], dense [B, Nd] or None -> logit [B, 1] and, if given, out [B, 1] = the activated output
        (contiguous float32 device buffers, e.g. row slices of one buffer for the whole call).  After `prepare`."""
        B, idx, kind, dense = self._batch_args(idx, dense, logit, out)
        check(self._entry('infer')(
            *self._gather_args(idx, kind), ptr(dense), B, *self._dims(), ptr(self.ws), ptr(logit), ptr(out), self._oob(),
            self.flags, stream_ptr()), f'dt_{self.PREFIX}_infer')

    def run_batches(self, data, batch_size, activate=True, each=None):
        """`prepare` once, then one `infer` per batch of `data` (training.TableBatches, in order) into ONE device buffer ->
        (logits [n, 1], activated outputs [n, 1] or None).  each(logit, out, y) is called with every batch's slices."""
        n = data.n
        logit = torch.empty((n, 1), dtype=torch.float32, device=self.device)
        out = torch.empty_like(logit) if activate else None
        self.prepare()
        r = 0
        for ins, yb in data.iterate(batch_size, False, drop_remainder=False):
            b = int(ins[0].shape[0])
            lg, o = logit[r:r + b], None if out is None else out[r:r + b]
            self.infer(ins[0], ins[1] if len(ins) > 1 else None, lg, o)
            if each is not None:
                each(lg, o, yb)
            r += b
        return logit, out


class InferDCN(InferDeepFM):
    """Inference plan for the DCN graph (nets ['dcn_nets'] alone, deepnets.py:194-207): the Cross network runs on the
    normalised tile inside the same launch."""

    NETS = {'dcn_nets'}
    PREFIX = 'dcn'
    CELL = 'dcn'
    NET_LAYERS = ('dcn_cross_layer',)

    @classmethod
    def _graph_ok(cls, dm):
        return list(dm.config.nets) == ['dcn_nets'] and 'dense_logit_dcn_nets' not in dm.model.layers_by_name

    @classmethod
    def _supported(cls, dm, dims, tower):
        nl = int(dm.model.layers_by_name['dcn_cross_layer'].num_cross_layer)
        return lib().dt_dcn_infer_supported(*dims, *tower, nl)

    def _net_layers(self, L):
        self.cross = L['dcn_cross_layer']
        self.nl = int(self.cross.num_cross_layer)

    def _dims(self):
        return self.F, self.D, self.Nd, self.nl

    def _net_args(self):
        return ptr(self.cross.kernel_stack), ptr(self.cross.bias_stack), self.nl

    def _head_weights(self):
        return ptr(self.out.kernel), None


class InferStack(InferDeepFM):
    """Inference plan for every other Add-stacked combination of 'linear', 'fm_nets' and 'dnn_nets', in any order in
    config.nets — ModelConfig's default ['dnn_nets'], WideDeep, the plain FM model ['linear', 'fm_nets'], ... (the full
    DeepFM graph stays InferDeepFM's): the same two launches behind the DT_NET_* mask (dt_stack_infer*).  With a tower the
    tile kernel runs with the absent terms compiled out; without one neither bn_concat_emb_dense nor a GEMM is in the graph
    and a gather-and-reduce kernel scores one row per wave (csrc/infer_x3.h k_infer_sparse).

    The head follows deepmodel.py:286-301.  Two or more nets: every net is reduced to one logit (dense_logit_dnn_nets,
    no bias, for the tower), Add, task_output [1, 1].  One net: no dense_logit_* layer and no Add — task_output is applied
    to the net's output, so for ['dnn_nets'] its [H2, 1] kernel is the tower's vector and the output weight is 1."""

    PREFIX = 'stack'
    NET_BITS = {'linear': _lib.DT_NET_LINEAR, 'fm_nets': _lib.DT_NET_FM, 'dnn_nets': _lib.DT_NET_DNN}
    FULL = _lib.DT_NET_LINEAR | _lib.DT_NET_FM | _lib.DT_NET_DNN

    @classmethod
    def _mask(cls, dm):
        """the DT_NET_* mask of config.nets; 0 when a net is not one of the three, is named twice, or all three are there"""
        nets = list(dm.config.nets)
        if any(not isinstance(n, str) or n not in cls.NET_BITS for n in nets):
            return 0
        mask = 0
        for n in nets:
            if mask & cls.NET_BITS[n]:
                return 0
            mask |= cls.NET_BITS[n]
        return 0 if mask == cls.FULL else mask

    @classmethod
    def _net_layer_names(cls, mask, n_nets):
        names = ()
        if mask & _lib.DT_NET_LINEAR:
            names += ('linear_logit',)
        if mask & _lib.DT_NET_FM:
            names += ('fm_layer',)
        if mask & _lib.DT_NET_DNN:
            # (a last cell of width 1 in a graph of several nets has no dense_logit_dnn_nets: refused, as by InferDeepFM)
            names += ('dnn_dense_1', 'dnn_dense_2') + (('dense_logit_dnn_nets',) if n_nets > 1 else ())
        return names

    @classmethod
    def eligible(cls, dm):
        """_step_dims' checks with the tower and its layers asked for only when 'dnn_nets' is among the nets"""
        c = dm.config
        try:
            mask = cls._mask(dm)
            if not mask or c.stacking_op != consts.STACKING_OP_ADD or getattr(c.distribute_strategy, 'sharded_embeddings', False):
                return False
            has_tower = bool(mask & _lib.DT_NET_DNN)
            dims = _step_dims(dm, cls._net_layer_names(mask, len(c.nets)), _infer_tower if has_tower else None)
            if dims is None:
                return False
            tower = _infer_tower(c.dnn_params) if has_tower else (0, 0, 0)
            if tuple(dm.model.layers_by_name['task_output'].kernel.shape) != (tower[1] if mask == _lib.DT_NET_DNN else 1, 1):
                return False
            return bool(lib().dt_stack_infer_supported(*dims[1:], *tower, mask))
        except Exception:
            return False

    def _tower_layers(self, L):
        self.mask = self._mask(self.dm)
        self.bn = self.cells = None
        if self.mask & _lib.DT_NET_DNN:
            super()._tower_layers(L)

    def _net_layers(self, L):
        self.lin = L['linear_logit'] if self.mask & _lib.DT_NET_LINEAR else None
        self.dl = L.get('dense_logit_dnn_nets')

    def _dims(self):
        return self.F, self.D, self.Nd, self.mask

    def _net_args(self):
        return self.mask, ptr(self.lin.kernel) if self.lin is not None else None

    def _tower_args(self):
        if self.cells is None:         # no tower: bn_gamma .. c2_eps are not read
            return (None, None, None, None, 0.0, None, 0, 0, None, None, 0, 0, None, 0) + (None, None, None, None, 0.0) * 2
        return super()._tower_args()

    def _head_weights(self):
        if self.mask == _lib.DT_NET_DNN:          # the tower alone: task_output's [H2, 1] kernel is its vector, w_out = 1
            return ptr(self.out.kernel), None
        return ptr(self.dl.kernel) if self.mask & _lib.DT_NET_DNN else None, ptr(self.out.kernel)


def _cin_mode(cin):
    """the CIN layer's precision mode (cin_params['mfma_dtype'] / DT_AMD_CIN_DTYPE, as the layer holds it now) -> DT_CIN_*:
    the entry point whose kernel the layer path runs in that mode (ops.cin_layer)"""
    mode = cin.mfma_dtype
    if mode == 'bf16x3':
        return _lib.DT_CIN_BF16X3
    if mode in ('bf16', 'bfloat16'):
        return _lib.DT_CIN_BF16
    if mode in ('float32', 'fp32', 'f32'):
        return _lib.DT_CIN_F32
    raise ValueError(f'CIN mfma_dtype {mode!r}: expected float32, bf16x3 or bf16')


class InferXDeepFM(InferDeepFM):
    """Inference plan for the xDeepFM graph (nets 'linear', 'cin_nets', 'dnn_nets', each once, in any order, Add-stacked;
    deepnets.py:21): 2 + len(cross_layer_size) launches per batch (dt_xdeepfm_infer_*, csrc/infer_x3.h) —
      tower: InferStack's tile launch for linear + dnn_nets, which also stores the embedding rows it gathered (x0, the CIN's
             input) and hands over linear + tower . w3 instead of the output;
      cin:   one CIN layer kernel per layer — the layer path's own kernel of the mode in force — on a filter packed in
             `prepare` (the layer path re-packs it on every call), reading the previous layer's output in place;
      head:  sum over D of the direct-connect channels, the exFM_out Dense, Add, task_output, the activation.
    Refused (the layer path runs): what InferStack refuses for a graph with a tower, more than 64 fields, use_residual,
    reduce_D, a CIN shape outside the layer kernels' domain, any other combination of nets with 'cin_nets'."""

    NETS = {'linear', 'cin_nets', 'dnn_nets'}
    PREFIX = 'xdeepfm'
    NET_LAYERS = ('linear_logit', 'dense_logit_dnn_nets')

    @staticmethod
    def _cin_layer(dm):
        from .models.layers import CIN
        found = [l for l in dm.model.layers_by_name.values() if isinstance(l, CIN)]
        return found[0] if len(found) == 1 else None

    @staticmethod
    def _cin_shape(cin):
        """(n_layers, layer sizes as a host int array, direct)"""
        sizes = [int(v) for v in cin.cross_layer_size]
        return len(sizes), (ctypes.c_int * len(sizes))(*sizes), 1 if cin.direct else 0

    @classmethod
    def _supported(cls, dm, dims, tower):
        cin = cls._cin_layer(dm)
        if cin is None or tuple(dm.model.layers_by_name['task_output'].kernel.shape) != (1, 1):
            return False
        n, sizes, direct = cls._cin_shape(cin)
        return lib().dt_xdeepfm_infer_supported(*dims, *tower, n, ctypes.cast(sizes, ctypes.c_void_p), direct,
                                                1 if cin.use_residual else 0, 1 if cin.reduce_D else 0,
                                                _lib.act_code(cin.activation, 'CIN'), _cin_mode(cin))

    def _net_layers(self, L):
        super()._net_layers(L)
        self.cin = self._cin_layer(self.dm)
        self.n_layers, self.sizes, self.direct = self._cin_shape(self.cin)
        self.cin_mode = _cin_mode(self.cin)
        self.cin_act = _lib.act_code(self.cin.activation, 'CIN')
        self.cin_bias = [None] * self.n_layers
        self._scratch = None

    def _cin_dims(self):
        return self.n_layers, ctypes.cast(self.sizes, ctypes.c_void_p), self.direct, self.cin_mode

    def _dims(self):
        """dt_xdeepfm_infer_workspace_bytes' arguments"""
        return (self.F, self.D, self.Nd) + self._cin_dims()

    def prepare(self):
        """the tower's layouts as InferDeepFM.prepare, then the CIN as it is now: its precision mode, every layer's filter
        (packed for that mode's kernel), the exFM_out Dense's kernel and bias — one call"""
        self.flags = self._tower_flags()
        self.cin_mode = _cin_mode(self.cin)
        nbytes = self._entry('infer_workspace_bytes')(*self._dims())
        if nbytes < 0:
            raise _lib.DtHipError('InferXDeepFM: unsupported shape')
        if nbytes > self.ws.numel() * 4:           # the mode changed to one with a larger packed filter
            self.ws = torch.zeros((nbytes + 3) // 4, dtype=torch.float32, device=self.device)
        cin, ex = self.cin, self.cin.exFM_out
        self.cin_bias = [ptr(cin.bias[k]) if cin.use_bias else None for k in range(self.n_layers)]
        filters = (ctypes.c_void_p * self.n_layers)(*[cin.f_[k].data_ptr() for k in range(self.n_layers)])
        check(self._entry('infer_prepare')(
            self.F, self.D, self.Nd, *self._net_args(), *self._tower_args(), *self._head_weights(), ptr(self.out.bias),
            *self._cin_dims(), ctypes.cast(filters, ctypes.c_void_p), ptr(ex.kernel), ptr(ex.bias), ptr(self.ws),
            stream_ptr()), 'dt_xdeepfm_infer_prepare')

    def _alloc_scratch(self, rows):
        """x0 [rows, F, D], partial [rows] and every CIN layer's output [rows, L_k, D] for batches of up to `rows` rows"""
        dev, f32 = self.device, torch.float32
        y = [torch.empty((rows, int(l), self.D), dtype=f32, device=dev) for l in self.sizes]
        return {'rows': rows, 'x0': torch.empty((rows, self.F, self.D), dtype=f32, device=dev),
                'partial': torch.empty((rows,), dtype=f32, device=dev), 'y': y,
                'y_ptrs': (ctypes.c_void_p * self.n_layers)(*[t.data_ptr() for t in y])}

    def infer(self, idx, dense, logit, out=None):
        """one batch, as InferDeepFM.infer: the tower launch, one launch per CIN layer, the head.  Inside `run_batches` the
        scratch is the call's; a lone call allocates its own."""
        B, idx, kind, dense = self._batch_args(idx, dense, logit, out)
        sc = self._scratch
        if sc is None or sc['rows'] < B:
            sc = self._alloc_scratch(B)
        dims, cin_dims, ws, st = (self.F, self.D, self.Nd), self._cin_dims(), ptr(self.ws), stream_ptr()
        check(self._entry('infer_tower')(
            *self._gather_args(idx, kind), ptr(dense), B, *dims, ws, ptr(sc['x0']), ptr(sc['partial']), self._oob(),
            self.flags & _lib.DT_INFER_TOWER_BF16, st), 'dt_xdeepfm_infer_tower')
        for k in range(self.n_layers):
            check(self._entry('infer_cin')(k, ptr(sc['x0']), ptr(sc['y'][k - 1]) if k else None, self.cin_bias[k],
                                           self.cin_act, B, *dims, *cin_dims, ws, ptr(sc['y'][k]), st), 'dt_xdeepfm_infer_cin')
        check(self._entry('infer_head')(ctypes.cast(sc['y_ptrs'], ctypes.c_void_p), ptr(sc['partial']), B, *dims, *cin_dims, ws,
                                        ptr(logit), ptr(out), self.flags & _lib.DT_INFER_SIGMOID, st), 'dt_xdeepfm_infer_head')

    def run_batches(self, data, batch_size, activate=True, each=None):
        """InferDeepFM.run_batches with the scratch (x0, partial, the CIN layers' outputs) allocated once for the call"""
        self._scratch = self._alloc_scratch(max(1, min(int(batch_size), int(data.n))))
        try:
            return super().run_batches(data, batch_size, activate=activate, each=each)
        finally:
            self._scratch = None


class InferAutoInt(InferDeepFM):
    """Inference plan for the AutoInt graph (nets ['autoint_nets'] alone, deepnets.py:210-224): ONE launch per batch
    (dt_autoint_infer, csrc/autoint.hip k_autoint_infer) — the table gather, every interacting layer with its inference
    BatchNormalization, Flatten, task_output and the activation; a wave keeps its batch row in LDS from the gather to the
    logit.  `prepare` hands the layers' tensors over as they are at that moment (host arrays of device pointers, one launch):
    the plan holds no copy of any parameter between calls.  The net does not read the continuous columns, so `dense` is
    ignored (never dereferenced).
    Refused (the layer path runs): multiclass, 'autoint_nets' beside any other net, concat stacking, var-len columns, several
    embedding groups, sharded embeddings, interacting layers that differ in their parameters, shapes outside
    dt_autoint_supported (F <= 32, embedding size 16 / 32, d_h in {4, 8, 16}), more layers than the LDS holds, a precision mode
    the embedding size does not take, DT_AMD_FUSED=0 / DT_AMD_FUSED_PREDICT=0."""

    PREFIX = 'autoint'

    @staticmethod
    def _mha_layers(dm):
        from .models.layers import MultiheadAttention
        return [l for l in dm.model.layers_by_name.values() if isinstance(l, MultiheadAttention)]

    @staticmethod
    def _mode(mha, D):
        """the layers' precision mode as the layer path reads it (raises for a request the embedding size does not take)"""
        return autoint_mfma_mode(mha[0].params.get('mfma_dtype'), D)

    @classmethod
    def eligible(cls, dm):
        c = dm.config
        try:
            if list(c.nets) != ['autoint_nets'] or c.stacking_op != consts.STACKING_OP_ADD or \
                    getattr(c.distribute_strategy, 'sharded_embeddings', False):
                return False
            dims = _step_dims(dm, (), tower=None)
            mha = cls._mha_layers(dm)
            if dims is None or not mha:
                return False
            _, F, D, _ = dims
            first = mha[0]
            same = all(l.params == first.params and l.num_heads == first.num_heads and l.num_units == D and
                       bool(l.use_residual) == bool(first.use_residual) and
                       float(l.batch_normalize.epsilon) == float(first.batch_normalize.epsilon) for l in mha)
            if not same or len(mha) != int(c.autoint_params['num_attention']):
                return False
            if tuple(dm.model.layers_by_name['task_output'].kernel.shape) != (F * D, 1):
                return False
            return bool(lib().dt_autoint_infer_supported(F, D, int(first.num_heads), len(mha), 1 if first.use_residual else 0,
                                                         cls._mode(mha, D)))
        except Exception:
            return False

    def _tower_layers(self, L):
        self.bn = self.cells = None

    def _net_layers(self, L):
        self.mha = self._mha_layers(self.dm)
        self.n_layers = len(self.mha)
        self.H = int(self.mha[0].num_heads)
        self.NP, self.mode = 4 if self.mha[0].use_residual else 3, _lib.DT_AI_F32

    def _dims(self):
        """dt_autoint_infer_workspace_bytes' arguments"""
        return self.F, self.D, self.n_layers

    def prepare(self):
        """the layers' tensors as they are now -> the workspace (= the kernel's LDS image), one launch; also reads the
        precision mode, the residual switch and the output activation (the arguments of the `infer` calls that follow)"""
        n = self.n_layers
        self.flags = self._sigmoid()
        self.mode = self._mode(self.mha, self.D)
        res = bool(self.mha[0].use_residual)
        self.NP = 4 if res else 3

        def arr(tensors):
            return ctypes.cast((ctypes.c_void_p * n)(*[None if t is None else t.data_ptr() for t in tensors]), ctypes.c_void_p)

        projs = [[l.dense_Q, l.dense_K, l.dense_V, l.dense_residual if res else None] for l in self.mha]
        kernels = [arr([None if p[k] is None else p[k].kernel for p in projs]) for k in range(4)]
        biases = [arr([None if p[k] is None else p[k].bias for p in projs]) for k in range(4)]
        bns = [l.batch_normalize for l in self.mha]
        stats = [arr([getattr(b, a) for b in bns]) for a in ('gamma', 'beta', 'moving_mean', 'moving_variance')]
        check(self._entry('infer_prepare')(self.F, self.D, n, *kernels, *biases, *stats, float(bns[0].epsilon),
                                           ptr(self.out.kernel), ptr(self.out.bias), ptr(self.ws), stream_ptr()),
              'dt_autoint_infer_prepare')

    def infer(self, idx, dense, logit, out=None):
        """one batch, as InferDeepFM.infer: ids [B, F] -> logit [B, 1] and, if given, out [B, 1]; `dense` is not read"""
        B, idx, kind, _ = self._batch_args(idx, None, logit, out)
        check(self._entry('infer')(
            *self._gather_args(idx, kind), B, self.F, self.D, self.H, self.n_layers, self.NP, ptr(self.ws), ptr(logit),
            ptr(out), self._oob(), self.flags, self.mode, stream_ptr()), 'dt_autoint_infer')


class InferAFM(InferDeepFM):
    """Inference plan for the AFM graphs: 'afm_nets' alone (deepnets.AFM) or Add-stacked with 'linear' and / or 'fm_nets',
    each net once, in any order in config.nets — ['linear', 'afm_nets'] is the AFM paper's model.  ONE launch per batch
    (dt_afm_infer, csrc/afm_infer.hip k_afm_infer): the table gather, `linear` and `fm_nets` from the raw rows, the AFM
    layer (pair products, attention Dense on the exact-fp32 matrix core, online softmax over the pairs, dense_out), Add,
    task_output and the activation; one wave per batch row, nothing written but the logit and the output.

    The head follows deepmodel.py:286-301.  The AFM layer's output is [B, 1], so beside other nets it has no dense_logit
    layer and enters Add as it is; alone, task_output's [1, 1] kernel is applied to it directly.  `prepare` hands the
    tensors over as they are at that moment: the plan holds no copy of a parameter between calls.  `dense` is dereferenced
    only when 'linear' is among the nets.
    Refused (the layer path runs): multiclass, any other net beside these three, a net named twice, concat stacking,
    var-len columns, several embedding groups, more than one continuous column, sharded embeddings, fewer than two
    categorical fields (there is no AFM layer then), shapes outside dt_afm_infer_supported (embedding size in {4, 8, 16, 32,
    64}, F D <= 512, hidden_factor <= 64), an attention activation the AFM kernels do not fuse, a dropout_rate outside
    [0, 1), DT_AMD_FUSED=0 / DT_AMD_FUSED_PREDICT=0."""

    PREFIX = 'afm'
    NET_BITS = {'afm_nets': _lib.DT_NET_AFM, 'linear': _lib.DT_NET_LINEAR, 'fm_nets': _lib.DT_NET_FM}

    @classmethod
    def _mask(cls, dm):
        """the DT_NET_* mask of config.nets; 0 when a net is not one of the three, is named twice, or 'afm_nets' is absent"""
        mask = 0
        for n in list(dm.config.nets):
            if not isinstance(n, str) or n not in cls.NET_BITS or mask & cls.NET_BITS[n]:
                return 0
            mask |= cls.NET_BITS[n]
        return mask if mask & _lib.DT_NET_AFM else 0

    @staticmethod
    def _act(afm):
        """the attention activation as the layer path reads it -> DT_ACT_* (raises for one the kernels do not fuse)"""
        return _lib.act_code(afm.activation_function, 'AFM')

    @classmethod
    def eligible(cls, dm):
        c = dm.config
        try:
            mask = cls._mask(dm)
            if not mask or c.stacking_op != consts.STACKING_OP_ADD or getattr(c.distribute_strategy, 'sharded_embeddings', False):
                return False
            names = ('afm_layer',) + (('linear_logit',) if mask & _lib.DT_NET_LINEAR else ()) + \
                (('fm_layer',) if mask & _lib.DT_NET_FM else ())
            dims = _step_dims(dm, names, tower=None)
            if dims is None:
                return False
            L = dm.model.layers_by_name
            afm = L['afm_layer']
            if not 0 <= float(afm.dropout_rate or 0) < 1 or tuple(L['task_output'].kernel.shape) != (1, 1):
                return False
            return bool(lib().dt_afm_infer_supported(*dims[1:], int(afm.hidden_factor), cls._act(afm), mask))
        except Exception:
            return False

    def _tower_layers(self, L):
        self.mask = self._mask(self.dm)
        self.bn = self.cells = None

    def _net_layers(self, L):
        self.afm = L['afm_layer']
        self.lin = L['linear_logit'] if self.mask & _lib.DT_NET_LINEAR else None
        self.H = int(self.afm.hidden_factor)
        self.act = self._act(self.afm)

    def _dims(self):
        """dt_afm_infer_workspace_bytes' arguments"""
        return self.F, self.D, self.Nd, self.H, self.mask

    def prepare(self):
        """the AFM layer's, linear_logit's and task_output's tensors as they are now -> the workspace, one launch; also reads
        the attention activation and the output activation (the arguments of the `infer` calls that follow)"""
        afm, att = self.afm, self.afm.dense_attention
        self.flags = self._sigmoid()
        self.act = self._act(afm)
        check(self._entry('infer_prepare')(
            *self._dims(), ptr(att.kernel), ptr(att.bias), ptr(afm.attention_p), ptr(afm.dense_out.kernel),
            ptr(self.lin.kernel) if self.lin is not None else None, ptr(self.out.kernel), ptr(self.out.bias), ptr(self.ws),
            stream_ptr()), 'dt_afm_infer_prepare')

    def infer(self, idx, dense, logit, out=None):
        """one batch, as InferDeepFM.infer; `dense` reaches the kernel only when 'linear' is among the nets"""
        B, idx, kind, dense = self._batch_args(idx, dense if self.lin is not None else None, logit, out)
        check(self._entry('infer')(
            *self._gather_args(idx, kind), ptr(dense), B, *self._dims(), self.act, ptr(self.ws), ptr(logit), ptr(out),
            self._oob(), self.flags, stream_ptr()), 'dt_afm_infer')


class InferPNN(InferDeepFM):
    """Inference plan for the product nets: 'pnn_nets' (deepnets.PNN: inner ++ outer ++ xn -> tower), 'ipnn_nets' (inner ++
    xn) or 'opnn_nets' (outer ++ xn), each alone in config.nets, with every outer_product_kernel_type.  ONE launch per batch
    (dt_pnn_infer, csrc/pnn_infer.hip k_pnn_infer): the table gather, the product layers from the raw rows ('mat' on the
    exact-fp32 matrix core), the input BatchNormalization of the embedding and dense columns, the tower, task_output and the
    activation; neither the field stack, the products nor their concatenation is written.

    The head follows deepmodel.py:286-301 for a single net: no dense_logit layer and no Add, task_output's [H2, 1] kernel is
    the tower's output vector and the output weight is 1.  `prepare` hands the tensors over as they are at that moment: the
    plan holds no copy of a parameter between calls.
    Refused (the layer path runs): multiclass, a product net beside any other net or two of them, concat stacking, fewer than
    two categorical fields (the net is absent), var-len columns, several embedding groups, sharded embeddings, a tower outside
    `_infer_tower`, a task_output kernel that is not [H2, 1], shapes outside dt_pnn_infer_supported (2 <= F <= 64, embedding
    size in {4, 8, 16, 32, 64}, F D <= 512, Nd <= 64), DT_AMD_FUSED=0 / DT_AMD_FUSED_PREDICT=0."""

    PREFIX = 'pnn'
    # net -> (the tower's layer prefix, inner product layer, outer product layer)
    PRODUCT_NETS = {'pnn_nets': ('pnn', 'pnn_inner_product_layer', 'pnn_outer_product_layer'),
                    'ipnn_nets': ('ipnn', 'inner_product_layer', None),
                    'opnn_nets': ('opnn', None, 'outer_product_layer')}

    @classmethod
    def _net(cls, dm):
        """(cell, inner layer name, outer layer name) of the single product net in config.nets, else None"""
        nets = list(dm.config.nets)
        if len(nets) != 1 or not isinstance(nets[0], str):
            return None
        return cls.PRODUCT_NETS.get(nets[0])

    @staticmethod
    def _products(L, inner, outer):
        """(DT_PNN_* mask, DT_OP_KERNEL_* of the outer layer as it is now or 0)"""
        mask = (_lib.DT_PNN_INNER if inner else 0) | (_lib.DT_PNN_OUTER if outer else 0)
        return mask, _lib.DT_OP_KERNEL[L[outer].kernel_type] if outer else 0

    @classmethod
    def eligible(cls, dm):
        c = dm.config
        try:
            net = cls._net(dm)
            if net is None or c.stacking_op != consts.STACKING_OP_ADD or \
                    getattr(c.distribute_strategy, 'sharded_embeddings', False):
                return False
            cell, inner, outer = net
            names = (f'{cell}_dense_1', f'{cell}_dense_2') + tuple(n for n in (inner, outer) if n)
            dims = _step_dims(dm, names, _infer_tower)
            if dims is None:
                return False
            L = dm.model.layers_by_name
            tower = _infer_tower(c.dnn_params)
            _, F, D, Nd = dims
            mask, kt = cls._products(L, inner, outer)
            P = F * (F - 1) // 2
            rows = P * (bool(inner) + bool(outer)) + F * D + Nd
            if tuple(L['task_output'].kernel.shape) != (tower[1], 1) or int(L[f'{cell}_dense_1'].kernel.shape[0]) != rows:
                return False
            if outer and tuple(L[outer].kernel.shape) != {0: (D, P, D), 1: (P, D), 2: (P, 1)}[kt]:
                return False
            return bool(lib().dt_pnn_infer_supported(F, D, Nd, *tower, mask, kt))
        except Exception:
            return False

    def _tower_layers(self, L):
        self.CELL, self.inner_name, self.outer_name = self._net(self.dm)
        super()._tower_layers(L)

    def _net_layers(self, L):
        self.op = L[self.outer_name] if self.outer_name else None
        self.products, self.kt = self._products(L, self.inner_name, self.outer_name)

    def _dims(self):
        """dt_pnn_infer_workspace_bytes' arguments"""
        return self.F, self.D, self.Nd, self.products, self.kt

    def _net_args(self):
        return self.products, self.kt, ptr(self.op.kernel) if self.op is not None else None

    def _head_weights(self):
        return (ptr(self.out.kernel),)          # w3: the tower alone, the output weight is 1


class InferFiBiNet(InferDeepFM):
    """Inference plan for the FiBiNet graph: 'fibi_dnn_nets' alone in config.nets (deepnets.FiBiNet), with every bilinear_type
    and both senet_pooling_op values.  ONE launch per batch (dt_fibi_infer, csrc/fibi_infer.hip k_fibi_infer): the table
    gather, SENET, both bilinear layers from the raw rows (on the exact-fp32 matrix core; the SENET-scaled stack is never
    formed), the tower on [senet half | raw half | the raw dense values], task_output and the activation; neither the field
    stack, the bilinear blocks nor their concatenation is written.  The dense values enter the tower raw: bn_concat_emb_dense
    is not part of this graph, and the plan applies none.

    The head follows deepmodel.py:286-301 for a single net: task_output's [H2, 1] kernel is the tower's output vector and the
    output weight is 1.  `prepare` hands the tensors over as they are at that moment — the bilinear type, the pooling op, the
    tower mode and the output activation are read there: the plan holds no copy of a parameter between calls.
    Refused (the layer path runs): multiclass, 'fibi_dnn_nets' beside any other net, 'fibi_nets', concat stacking, fewer than
    two categorical fields or no dense input (the net is absent), var-len columns, several embedding groups, sharded
    embeddings, a tower outside `_infer_tower`, a task_output kernel that is not [H2, 1], more or fewer than one SENET / senet
    bilinear / embedding bilinear layer, shapes outside dt_fibi_infer_supported (2 <= F <= 64, embedding size in {4, 8, 16, 32,
    64}, F D <= 512, 1 <= Nd <= 64), DT_AMD_FUSED=0 / DT_AMD_FUSED_PREDICT=0."""

    PREFIX = 'fibi'
    CELL = 'fibi_dnn'

    @staticmethod
    def _fibi_layers(dm):
        """(SENET, senet bilinear, embedding bilinear): the layers carry a counter in their names, so they are found by prefix
        and type — exactly one of each, else None"""
        from .models.layers import SENET, BilinearInteraction
        found = []
        for prefix, kind in (('senet_layer_', SENET), ('senet_bilinear_layer_', BilinearInteraction),
                             ('embedding_bilinear_layer_', BilinearInteraction)):
            hits = [l for n, l in dm.model.layers_by_name.items()
                    if n.startswith(prefix) and n[len(prefix):].isdigit() and isinstance(l, kind)]
            if len(hits) != 1:
                return None
            found.append(hits[0])
        return tuple(found)

    @staticmethod
    def _codes(se, bs, br):
        """(DT_BILINEAR_* of the two bilinear layers as BilinearInteraction.call reads it, DT_FIBI_POOL_*, R) as they are now"""
        from .ops import BILINEAR_TYPES
        kinds = {b.bilinear_type if b.bilinear_type in ('field_all', 'field_each') else 'field_interaction' for b in (bs, br)}
        if len(kinds) != 1:
            raise ValueError('the two bilinear layers differ in their bilinear_type')
        pool = _lib.DT_FIBI_POOL_MAX if se.pooling_op == 'max' else _lib.DT_FIBI_POOL_MEAN
        return BILINEAR_TYPES[kinds.pop()], pool, int(se.reduction_num)

    @classmethod
    def eligible(cls, dm):
        c = dm.config
        try:
            nets = list(c.nets)
            if len(nets) != 1 or not isinstance(nets[0], str) or nets[0] != 'fibi_dnn_nets':
                return False
            if c.stacking_op != consts.STACKING_OP_ADD or getattr(c.distribute_strategy, 'sharded_embeddings', False):
                return False
            # (tower=None: this graph reads no bn_concat_emb_dense, so _step_dims must not ask for one)
            dims = _step_dims(dm, (f'{cls.CELL}_dense_1', f'{cls.CELL}_dense_2'), tower=None)
            found = cls._fibi_layers(dm)
            tower = _infer_tower(c.dnn_params)
            if dims is None or found is None or tower is None:
                return False
            se, bs, br = found
            L = dm.model.layers_by_name
            _, F, D, Nd = dims
            bt, pool, R = cls._codes(se, bs, br)
            P = F * (F - 1) // 2
            if tuple(L['task_output'].kernel.shape) != (tower[1], 1) or \
                    int(L[f'{cls.CELL}_dense_1'].kernel.shape[0]) != 2 * P * D + Nd:
                return False
            nw = (P, F - 1, 1)[bt]
            if tuple(bs.W.shape) != (nw, D, D) or tuple(br.W.shape) != (nw, D, D):
                return False
            if tuple(se.dense_att1.kernel.shape) != (F, R) or tuple(se.dense_att2.kernel.shape) != (R, F):
                return False
            return bool(lib().dt_fibi_infer_supported(F, D, Nd, *tower, bt, pool, R))
        except Exception:
            return False

    def _tower_layers(self, L):
        self.bn = None                          # (bn_concat_emb_dense is not part of this graph)
        self.cells = [(L[f'{self.CELL}_dense_{i}'], L.get(f'{self.CELL}_bn_{i}')) for i in (1, 2)]

    def _net_layers(self, L):
        self.se, self.bs, self.br = self._fibi_layers(self.dm)
        self.bt, self.pool, self.R = self._codes(self.se, self.bs, self.br)

    def _dims(self):
        """dt_fibi_infer_workspace_bytes' arguments"""
        return self.F, self.D, self.Nd, self.bt, self.R

    def prepare(self):
        """the SENET, bilinear, tower and task_output tensors as they are now -> the workspace, one launch; also reads the
        bilinear type, the pooling op, R, the tower's precision mode and the output activation (the arguments of the `infer`
        calls that follow)"""
        se, bs, br = self.se, self.bs, self.br
        self.flags = self._tower_flags()
        self.bt, self.pool, self.R = self._codes(se, bs, br)
        nbytes = self._entry('infer_workspace_bytes')(*self._dims())
        if nbytes < 0:
            raise _lib.DtHipError('InferFiBiNet: unsupported shape')
        if nbytes > self.ws.numel() * 4:           # the bilinear type changed to one with a larger layout
            self.ws = torch.zeros((nbytes + 3) // 4, dtype=torch.float32, device=self.device)
        for t in (se.dense_att1.kernel, se.dense_att2.kernel, bs.W, br.W):
            if not t.is_contiguous():
                raise _lib.DtHipError(f'inference plan: SENET / bilinear weight with strides {tuple(t.stride())}')
        check(self._entry('infer_prepare')(
            *self._dims(), ptr(se.dense_att1.kernel), ptr(se.dense_att1.bias), ptr(se.dense_att2.kernel),
            ptr(se.dense_att2.bias), ptr(bs.W), ptr(br.W), *self._cell_args(), ptr(self.out.kernel), ptr(self.out.bias),
            ptr(self.ws), stream_ptr()), 'dt_fibi_infer_prepare')

    def infer(self, idx, dense, logit, out=None):
        """one batch, as InferDeepFM.infer"""
        B, idx, kind, dense = self._batch_args(idx, dense, logit, out)
        check(self._entry('infer')(
            *self._gather_args(idx, kind), ptr(dense), B, self.F, self.D, self.Nd, self.bt, self.pool, self.R, ptr(self.ws),
            ptr(logit), ptr(out), self._oob(), self.flags, stream_ptr()), 'dt_fibi_infer')


class InferFGCNN(InferDeepFM):
    """Inference plan for the FGCNN graph: 'fgcnn_dnn_nets' alone in config.nets (deepnets.FGCNN), with any block list of
    fgcnn_params inside the library's domain.  2 depth + 1 launches per batch (csrc/fgcnn_infer.hip), every one the
    library's own kernel:
      conv:   per block, the (h, 1) convolution with its taps read from the map in LDS (block 1 gathers the table rows
              itself), tanh and the max pooling -> the pooled map [B, Fp D filters];
      recomb: per block, the recombination Dense on the matrix core (split-bf16, the fp32 class) on a weight packed in
              `prepare`, tanh -> the block's columns of the generated features [B, sum F_k D nf_k];
      tower:  the gather again, the tower on [generated features | raw embedding rows | raw dense values] in K chunks,
              task_output and the activation.
    The pooled maps and the generated features live in a batch-sized scratch owned by the call (`run_batches`; a lone
    `infer` allocates its own); neither the taps matrix, a padded map nor the tower's input is written.  The dense values
    enter the tower raw: bn_concat_emb_dense is not part of this graph.  The head follows deepmodel.py:286-301 for a single
    net: task_output's [H2, 1] kernel is the tower's output vector.  `prepare` hands every tensor over as it is at that
    moment; the tower's precision mode acts on the tower only, the blocks stay in the fp32 class.
    Refused (the layer path runs): multiclass, 'fgcnn_dnn_nets' beside any other net, every other fgcnn_* / fg_nets net,
    concat stacking, fewer than two categorical fields (the net is absent), var-len columns, several embedding groups,
    sharded embeddings, a tower outside `_infer_tower`, a block whose activation is not tanh, a layer count or a weight
    shape that does not follow from (F, D, fgcnn_params), shapes outside dt_fgcnn_infer_supported (2 <= F <= 64, embedding
    size in {4, 8, 16, 32, 64}, F D <= 512, Nd <= 64, 1 to 3 blocks, filters <= 16, heights <= 9, pool heights <= 3, new
    filters <= 3), DT_AMD_FUSED=0 / DT_AMD_FUSED_PREDICT=0."""

    PREFIX = 'fgcnn'
    CELL = 'fgcnn_dnn'

    @staticmethod
    def _blocks(dm):
        """the layers.FGCNN layers in creation order"""
        from .models.layers import FGCNN
        return [l for l in dm.model.layers_by_name.values() if isinstance(l, FGCNN)]

    @staticmethod
    def _params(blocks):
        """(filters, heights, pool heights, new filters) of the blocks as they are now, each a tuple of ints"""
        return (tuple(int(b.filters) for b in blocks), tuple(int(b.kernel_height) for b in blocks),
                tuple(int(b.pool_height) for b in blocks), tuple(int(b.new_filters) for b in blocks))

    @staticmethod
    def _block_dims(F, D, params):
        """per block (F_k, C_k, Fp_k, K_k = Fp_k D filters_k, N_k = F_k D nf_k)"""
        dims, C = [], 1
        for filt, _, pool, nf in zip(*params):
            Fp = -(-F // pool)
            dims.append((F, C, Fp, Fp * D * filt, F * D * nf))
            F, C = Fp, filt
        return dims

    @staticmethod
    def _host_arrays(params):
        """depth and the four HOST int arrays of dt_fgcnn_infer_* (kept alive by the caller)"""
        depth = len(params[0])
        arrs = tuple((ctypes.c_int * depth)(*p) for p in params)
        return arrs, (depth,) + tuple(ctypes.cast(a, ctypes.c_void_p) for a in arrs)

    @classmethod
    def eligible(cls, dm):
        c = dm.config
        try:
            nets = list(c.nets)
            if len(nets) != 1 or not isinstance(nets[0], str) or nets[0] != 'fgcnn_dnn_nets':
                return False
            if c.stacking_op != consts.STACKING_OP_ADD or getattr(c.distribute_strategy, 'sharded_embeddings', False):
                return False
            # (tower=None: this graph reads no bn_concat_emb_dense, so _step_dims must not ask for one)
            dims = _step_dims(dm, (f'{cls.CELL}_dense_1', f'{cls.CELL}_dense_2'), tower=None)
            tower = _infer_tower(c.dnn_params)
            blocks = cls._blocks(dm)
            if dims is None or tower is None or not blocks:
                return False
            from .models.deepnets import _FG_DEFAULTS
            want = tuple(tuple(int(v) for v in c.fgcnn_params.get(k, d)) for k, d in _FG_DEFAULTS)
            depth = min(len(w) for w in want)
            params = cls._params(blocks)
            if len(blocks) != depth or params != tuple(w[:depth] for w in want):
                return False
            if any(b.activation != 'tanh' for b in blocks):
                return False
            _, F, D, Nd = dims
            bd = cls._block_dims(F, D, params)
            for b, (Fk, Ck, Fp, K, N), filt, h in zip(blocks, bd, params[0], params[1]):
                if tuple(b.conv_kernel.shape) != (h, 1, Ck, filt) or tuple(b.conv_bias.shape) != (filt,):
                    return False
                if tuple(b.dense_output.kernel.shape) != (K, N):
                    return False
                if b.dense_output.bias is not None and tuple(b.dense_output.bias.shape) != (N,):
                    return False
            L = dm.model.layers_by_name
            if tuple(L['task_output'].kernel.shape) != (tower[1], 1) or \
                    int(L[f'{cls.CELL}_dense_1'].kernel.shape[0]) != sum(d[4] for d in bd) + F * D + Nd:
                return False
            keep, args = cls._host_arrays(params)
            return bool(lib().dt_fgcnn_infer_supported(F, D, Nd, *tower, *args))
        except Exception:
            return False

    def _tower_layers(self, L):
        self.bn = None                          # (bn_concat_emb_dense is not part of this graph)
        self.cells = [(L[f'{self.CELL}_dense_{i}'], L.get(f'{self.CELL}_bn_{i}')) for i in (1, 2)]

    def _net_layers(self, L):
        self.blocks = self._blocks(self.dm)
        self._read_params()
        self._scratch = None

    def _read_params(self):
        self.params = self._params(self.blocks)
        self.depth = len(self.blocks)
        self._arrays, self._shape_args = self._host_arrays(self.params)

    def _dims(self):
        """dt_fgcnn_infer_workspace_bytes' arguments"""
        return (self.F, self.D, self.Nd) + self._shape_args

    def prepare(self):
        """the blocks', the tower's and task_output's tensors as they are now -> the workspace, one launch; also reads the
        block parameters, the tower's precision mode and the output activation (the arguments of the launches that follow)"""
        self.flags = self._tower_flags()
        self._read_params()
        nbytes = self._entry('infer_workspace_bytes')(*self._dims())
        if nbytes < 0:
            raise _lib.DtHipError('InferFGCNN: unsupported shape')
        if nbytes > self.ws.numel() * 4:           # the block parameters changed to ones with a larger layout
            self.ws = torch.zeros((nbytes + 3) // 4, dtype=torch.float32, device=self.device)
        tensors = [(b.conv_kernel, b.conv_bias, b.dense_output.kernel, b.dense_output.bias) for b in self.blocks]
        for group in tensors:
            for t in group:
                if t is not None and not t.is_contiguous():
                    raise _lib.DtHipError(f'inference plan: FGCNN weight with strides {tuple(t.stride())}')
        host = [(ctypes.c_void_p * self.depth)(*[None if g[i] is None else g[i].data_ptr() for g in tensors])
                for i in range(4)]
        check(self._entry('infer_prepare')(
            *self._dims(), *[ctypes.cast(h, ctypes.c_void_p) for h in host], *self._cell_args(), ptr(self.out.kernel),
            ptr(self.out.bias), ptr(self.ws), stream_ptr()), 'dt_fgcnn_infer_prepare')

    def _alloc_scratch(self, rows):
        """every block's pooled map [rows, Fp D filters] and the generated features [rows, sum N_k] for batches of up to
        `rows` rows, for the block parameters in force"""
        bd = self._block_dims(self.F, self.D, self.params)
        dev, f32 = self.device, torch.float32
        return {'rows': rows, 'params': self.params,
                'pooled': [torch.empty((rows, d[3]), dtype=f32, device=dev) for d in bd],
                'feats': torch.empty((rows, sum(d[4] for d in bd)), dtype=f32, device=dev)}

    def infer(self, idx, dense, logit, out=None):
        """one batch, as InferDeepFM.infer: conv and recomb per block, then the tower.  Inside `run_batches` the scratch is
        the call's; a lone call allocates its own."""
        B, idx, kind, dense = self._batch_args(idx, dense, logit, out)
        if B == 0:
            return
        sc = self._scratch
        if sc is None or sc['rows'] < B or sc['params'] != self.params:
            sc = self._alloc_scratch(B)
        gather, dims, ws, st = self._gather_args(idx, kind), self._dims(), ptr(self.ws), stream_ptr()
        for k in range(self.depth):
            check(self._entry('infer_conv')(k, *gather, ptr(sc['pooled'][k - 1]) if k else None, B, *dims, ws,
                                            ptr(sc['pooled'][k]), st), 'dt_fgcnn_infer_conv')
            check(self._entry('infer_recomb')(k, ptr(sc['pooled'][k]), B, *dims, ws, ptr(sc['feats']), st),
                  'dt_fgcnn_infer_recomb')
        check(self._entry('infer_tower')(*gather, ptr(dense), ptr(sc['feats']), B, *dims, ws, ptr(logit), ptr(out), self._oob(),
                                         self.flags, st), 'dt_fgcnn_infer_tower')

    def run_batches(self, data, batch_size, activate=True, each=None):
        """InferDeepFM.run_batches with the scratch (pooled maps, generated features) allocated once for the call"""
        self._read_params()
        self._scratch = self._alloc_scratch(max(1, min(int(batch_size), int(data.n))))
        try:
            return super().run_batches(data, batch_size, activate=activate, each=each)
        finally:
            self._scratch = None


def make_inference_plan(dm):
    if not predict_enabled() or dm.model is None:
        return None
    for plan in (InferDeepFM, InferDCN, InferStack, InferXDeepFM, InferAutoInt, InferAFM, InferPNN,
                 InferFiBiNet, InferFGCNN):
        if plan.eligible(dm):
            return plan(dm)
    return None
