# -*- coding:utf-8 -*-
"""Train-step glue around the layers hot path: losses, Keras-semantics Adam
(dense + row-sparse embedding update, HIP kernels), batching, and the data-parallel
gradient exchange hook (epoch metrics: metrics.py).  This is what `keras.Model.fit` does for the reference
(deeptables/models/deepmodel.py:114-129, :319-346)."""
import ctypes
import math

import numpy as np
import torch

import os

from . import _lib
from ._lib import check, lib, ptr, stream_ptr
from .utils import consts

# `DeepModel.fit(steps_per_execution=None)` falls back to this (Keras' `model.compile(steps_per_execution=...)`,
# deepmodel.py:319-346): 'auto' = k consecutive train steps per captured hipGraph (compiled.CompiledTrainLoop) when the
# graph has a fused whole-step plan and the feed is device resident, eager steps otherwise; an int forces k; 1 = eager
DEFAULT_STEPS_PER_EXECUTION = os.environ.get('DT_AMD_STEPS_PER_EXECUTION', 'auto')
if DEFAULT_STEPS_PER_EXECUTION != 'auto':
    DEFAULT_STEPS_PER_EXECUTION = int(DEFAULT_STEPS_PER_EXECUTION)


# ---------------------------------------------------------------------------------------------
# optimizers with slots and a device-resident step state: Adam, Adagrad, RMSprop
# ---------------------------------------------------------------------------------------------
DT_ADAM_STATE_WORDS = 272 // 4        # DT_ADAM_STATE_BYTES (include/dt_hip.h) in int32 words

CLIP_KEYS = ('clipnorm', 'clipvalue', 'global_clipnorm')
_CLIP_MODES = {'clipvalue': _lib.DT_CLIP_VALUE, 'clipnorm': _lib.DT_CLIP_NORM, 'global_clipnorm': _lib.DT_CLIP_GLOBAL_NORM}


def check_clip(clipnorm=None, clipvalue=None, global_clipnorm=None):
    """Keras' three clip arguments -> (key, c) or None: at most one may be set, and it must be a finite number > 0"""
    given = [(k, v) for k, v in zip(CLIP_KEYS, (clipnorm, clipvalue, global_clipnorm)) if v is not None]
    if len(given) > 1:
        raise ValueError(f'Only one of `clipnorm`, `clipvalue` and `global_clipnorm` can be set, got {dict(given)}')
    for k, v in given:
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or not v > 0:
            raise ValueError(f'`{k}` must be a finite number greater than 0 (or None: off), got {v!r}')
    return (given[0][0], float(given[0][1])) if given else None


class _GradClip:
    """keras.optimizers' `clipnorm` / `clipvalue` / `global_clipnorm` (BaseOptimizer._clip_gradients) for every optimizer here:
    ONE stage at the head of `step()` (csrc/gradclip.hip), ahead of an update that is the unclipped optimizer's, bit for bit.
    A variable is a Keras variable: a dense parameter, one column's `embeddings_i` (one field's row range of a packed
    table), a VarLenColumnEmbedding table.  A table's gradient is its dense gradient: duplicate lookups are summed first
    (dt_rows_coalesce), rows not looked up have gradient 0 and every formula maps 0 to 0, so they are never touched.
    With a clip set no fused step may apply an update (`supports_row_segments` / `supports_rows_in_step` are False and
    DeepModel.fused_plan() is None): training runs layer by layer."""

    _clip = None                      # (key, c)
    last_global_norm = None           # 0-dim float64 device tensor: sqrt(sum over the variables of sum g^2) of the last step
    _row_segments = False
    _rows_in_step = False

    @property
    def supports_row_segments(self):
        """takes SparseRowGrad.segments"""
        return self._row_segments and self._clip is None

    @property
    def supports_rows_in_step(self):
        """a fused step may apply the update of the rows looked up once itself (fields = -2)"""
        return self._rows_in_step and self._clip is None

    clip = property(lambda self: self._clip, doc='(key, c) of the clip that is set, or None')
    clipnorm = property(lambda self: self._clip_value('clipnorm'))
    clipvalue = property(lambda self: self._clip_value('clipvalue'))
    global_clipnorm = property(lambda self: self._clip_value('global_clipnorm'))

    def _clip_value(self, key):
        return self._clip[1] if self._clip is not None and self._clip[0] == key else None

    def _set_clip(self, clipnorm=None, clipvalue=None, global_clipnorm=None):
        self._clip = check_clip(clipnorm, clipvalue, global_clipnorm)

    def _clip_hp(self):
        """the part of `hyperparameters()` that says how gradients are clipped: empty when they are not"""
        return {} if self._clip is None else {self._clip[0]: self._clip[1]}

    def _load_clip_hp(self, hp):
        """`set_hyperparameters`: clip keys in `hp` replace the setting as a whole -> hp without them"""
        if any(k in hp for k in CLIP_KEYS):
            self._set_clip(**{k: hp.get(k) for k in CLIP_KEYS})
        return {k: v for k, v in hp.items() if k not in CLIP_KEYS}

    # -- the stage ------------------------------------------------------------------------------------------
    def _clip_buffer(self, name, numel, dtype, device):
        """persistent scratch of the stage (a captured graph holds its address): grown, never shrunk"""
        bufs = self.__dict__.setdefault('_clip_bufs', {})
        t = bufs.get(name)
        if t is None or t.numel() < numel or t.device != device:
            t = torch.empty(max(int(numel), 1), dtype=dtype, device=device)
            bufs[name] = t
        return t

    def _field_rows(self, layer, key, table):
        """(host list [row_offset_0, .., V], device int64 [F]) of a packed table: where each column's variable starts"""
        cache = self.__dict__.setdefault('_clip_fields', {})
        hit = cache.get((id(layer), key))
        if hit is None or hit[1].device != table.device:
            dev_offs = getattr(layer, f'row_offset_{key}', None)
            if hasattr(layer, 'input_dims') and hasattr(layer, 'groups'):
                offs, o = [], 0
                for i in dict(layer.groups)[table.shape[1]]:
                    offs.append(o)
                    o += int(layer.input_dims[i])
            elif dev_offs is not None:
                offs = [int(v) for v in dev_offs.tolist()]          # (once per table, at the first clipped step)
            else:
                offs = [0]
            if dev_offs is None or dev_offs.device != table.device or dev_offs.dtype != torch.int64:
                dev_offs = torch.tensor(offs, dtype=torch.int64, device=table.device)
            hit = (offs + [int(table.shape[0])], dev_offs.contiguous())
            cache[(id(layer), key)] = hit
        return hit

    def _flat_regions(self):
        """[(element offset, span)] of a registered flat group's members inside the flat gradient.  A strided member (a
        narrow tower inside a zero-padded slab) counts with the pads it encloses: their gradient is 0."""
        regions = []
        for off, cnt, layout in self._flat_members:
            span = cnt if layout is None else 1 + sum((s - 1) * st for s, st in zip(*layout))
            regions.append((int(off), int(span)))
        end = 0
        for off, span in sorted(regions):
            if off < end or off + span > self._flat[4]:
                raise ValueError('gradient clipping: two members of the flat group interleave, so a member is no region of it')
            end = off + span
        return regions

    def _coalesce(self, table, grads):
        """dt_rows_coalesce of a table's sparse gradient pieces into the stage's persistent buffers -> (out_rows [n]: the
        distinct rows ascending, then -1; out_vals [n, D]: their summed gradients; count: device int64 [1]; n)"""
        h = lib()
        V, D = table.shape
        device = table.device
        rows = torch.cat([g.rows.reshape(-1) for g in grads]) if len(grads) > 1 else grads[0].rows.reshape(-1)
        vals = torch.cat([g.values.reshape(-1, D) for g in grads]) if len(grads) > 1 else grads[0].values.reshape(-1, D)
        rows, vals = rows.contiguous(), vals.contiguous()
        n = rows.numel()
        tag = f'{id(table)}'
        out_rows = self._clip_buffer(tag + '/rows', n, torch.int64, device)[:n]
        out_vals = self._clip_buffer(tag + '/vals', n * D, torch.float32, device)[:n * D].view(n, D)
        count = self._clip_buffer(tag + '/count', 1, torch.int64, device)
        need = int(h.dt_rows_coalesce_workspace_bytes(n, D))
        if need < 0:
            check(need, 'dt_rows_coalesce_workspace_bytes')
        ws = self._clip_buffer(tag + '/ws', need, torch.uint8, device)
        check(h.dt_rows_coalesce(ptr(rows), ptr(vals), n, D, V, ptr(out_rows), ptr(out_vals), ptr(count), ptr(ws), stream_ptr()),
              'dt_rows_coalesce')
        return out_rows, out_vals, count, n

    def clip_gradients(self):
        """The clip stage of `step()`: afterwards every `.grad` (contiguous, clipped in place) and every table's
        `sparse_grads` entry (ONE piece: the distinct rows ascending, then -1, with their summed and clipped gradients,
        fields = -1) are what the unclipped optimizer is given.  No host synchronisation; replays in a captured graph."""
        self._step_coalesced = {}                          # id(table) -> (out_rows, n): the tables this step's clip coalesced
        if self._clip is None:
            return
        key, c = self._clip
        mode = _CLIP_MODES[key]
        h, st = lib(), stream_ptr()
        regions = []                                       # (address, elements) of the dense variables
        flat_ids = ()
        flat = getattr(self, '_flat', None)
        if flat is not None:
            fg, members = flat[1], flat[5]
            with_grad = [p for p in self.params if id(p) in members and p.grad is not None]
            if len(with_grad) == len(members):
                outside = [p for p in with_grad if p.grad.data_ptr() != fg.data_ptr() + 4 * members[id(p)]]
                if len(outside) == len(members):
                    fg.zero_()
                for p in outside:                          # (what step() would do: the stage needs it done first)
                    view = self._flat_grad_view(p)
                    view.copy_(p.grad.reshape(view.shape))
                    p.grad = view
                regions += [(fg.data_ptr() + 4 * off, span) for off, span in self._flat_regions()]
                flat_ids = members
        tables = {id(layer.tables[k]): (layer, k) for layer in self.embedding_layers for k in getattr(layer, 'tables', {})}
        device = None
        for p in self.params:
            if p.grad is None:
                continue
            device = p.device
            if id(p) in flat_ids:
                continue
            if not p.grad.is_contiguous():
                p.grad = p.grad.contiguous()
            g = p.grad
            if id(p) in tables and p.dim() == 2:           # a packed table with a dense gradient: one variable per column
                offs, D = self._field_rows(*tables[id(p)], p)[0], p.shape[1]
                regions += [(g.data_ptr() + 4 * lo * D, (hi - lo) * D) for lo, hi in zip(offs[:-1], offs[1:])]
            else:
                regions.append((g.data_ptr(), g.numel()))
        from .ops import SparseRowGrad
        sparse, n_sums = [], len(regions)
        for layer in self.embedding_layers:
            for k, grads in list(layer.sparse_grads.items()):
                if not grads:
                    continue
                if any(getattr(g, 'segments', None) is not None or getattr(g, 'fields', None) == -2 for g in grads):
                    raise ValueError(f'{self._name}: gradient clipping takes plain (rows, values) sparse gradients: no segments, no '
                                     f'rows applied inside a fused step')
                table = layer.tables[k]
                V, D = table.shape
                device = table.device
                out_rows, out_vals, count, n = self._coalesce(table, grads)
                self._step_coalesced[id(table)] = (out_rows, n)
                offs_dev = self._field_rows(layer, k, table)[1]
                sparse.append((layer, k, out_rows, out_vals, count, n, D, V, offs_dev, n_sums))
                n_sums += offs_dev.numel()
        if device is None:
            return
        R = len(regions)
        gs = ctypes.cast((ctypes.c_void_p * max(R, 1))(*[a for a, _ in regions]), ctypes.c_void_p)
        ns = ctypes.cast((ctypes.c_int64 * max(R, 1))(*[int(m) for _, m in regions]), ctypes.c_void_p)
        idx = ctypes.cast((ctypes.c_int * max(R, 1))(*range(R)), ctypes.c_void_p)
        sums = self._clip_buffer('sums', n_sums, torch.float64, device)
        if self.last_global_norm is None or self.last_global_norm.device != device:
            self.last_global_norm = torch.zeros((), dtype=torch.float64, device=device)
        if mode != _lib.DT_CLIP_VALUE:
            need = int(h.dt_grad_sumsq_workspace_bytes(R, ns))
            if need < 0:
                check(need, 'dt_grad_sumsq_workspace_bytes')
            ws = self._clip_buffer('sumsq_ws', (need + 7) // 8, torch.float64, device)
            check(h.dt_grad_sumsq(R, gs, ns, ptr(sums), ptr(ws), st), 'dt_grad_sumsq')
            for layer, k, out_rows, out_vals, count, n, D, V, offs_dev, base in sparse:
                parts = self._clip_buffer(f'{id(layer.tables[k])}/parts', offs_dev.numel() * _lib.DT_FIELD_SUMSQ_PARTS,
                                          torch.float64, device)
                check(h.dt_rows_field_sumsq(ptr(out_rows), ptr(out_vals), n, D, ptr(count), ptr(offs_dev), offs_dev.numel(), V,
                                            ctypes.c_void_p(sums.data_ptr() + 8 * base), ptr(parts), st), 'dt_rows_field_sumsq')
        check(h.dt_grad_clip(mode, c, R, gs, ns, idx, ptr(sums), n_sums, ptr(self.last_global_norm), st), 'dt_grad_clip')
        for layer, k, out_rows, out_vals, count, n, D, V, offs_dev, base in sparse:
            check(h.dt_rows_clip(mode, c, ptr(out_rows), ptr(out_vals), n, D, ptr(count), ptr(offs_dev), offs_dev.numel(), V,
                                 ptr(sums), base, n_sums, None, st), 'dt_rows_clip')
            layer.sparse_grads[k] = [SparseRowGrad(out_rows, out_vals, fields=-1)]


STAGE_KEYS = ('weight_decay', 'use_ema', 'ema_momentum')
DT_STAGE_STATE_WORDS = 16 // 4        # DT_STAGE_STATE_BYTES (include/dt_hip.h) in int32 words


def _is_number(v):
    return isinstance(v, (int, float)) and not isinstance(v, bool)


def check_stages(weight_decay=None, use_ema=False, ema_momentum=0.99, ema_overwrite_frequency=None):
    """Keras' base-optimizer arguments -> (weight_decay or None, use_ema, ema_momentum): the decay a finite number >= 0 (None:
    off), the momentum in [0, 1]; `ema_overwrite_frequency` is not supported"""
    if weight_decay is not None and not (_is_number(weight_decay) and math.isfinite(weight_decay) and weight_decay >= 0):
        raise ValueError(f'`weight_decay` must be a finite number >= 0 (or None: off), got {weight_decay!r}')
    if not isinstance(use_ema, (bool, np.bool_)):
        raise ValueError(f'`use_ema` must be True or False, got {use_ema!r}')
    if not (_is_number(ema_momentum) and 0 <= ema_momentum <= 1):
        raise ValueError(f'`ema_momentum` must be in the range [0, 1], got {ema_momentum!r}')
    if ema_overwrite_frequency is not None:
        raise ValueError(f'`ema_overwrite_frequency` is not supported (got {ema_overwrite_frequency!r}): the weights are '
                         f'overwritten with their average once, by `finalize_variable_values()` at the end of `fit`')
    return (None if weight_decay is None else float(weight_decay)), bool(use_ema), float(ema_momentum)


class _StepStages(_GradClip):
    """keras.optimizers' `weight_decay` (BaseOptimizer._apply_weight_decay; `Adam(weight_decay=...)` is AdamW) and `use_ema` /
    `ema_momentum` for every optimizer here, as stages around an update that is the plain optimizer's, bit for bit
    (csrc/optim_stages.hip).  `step()` runs: the clip stage, the decay p = p - (p*wd)*lr of every variable that is not
    excluded (the gradient was taken at the un-decayed p), the update, then a = m*a + (1 - m)*p with m = 0 at the stage's first
    step, and the stage's own device-resident step count goes up by one.  A variable is a Keras variable, as in `_GradClip`.
    Row-sparse tables (a sparse gradient: above DENSE_GRAD_MAX_ELEMS): duplicates are summed first (dt_rows_coalesce), and
      * only the looked-up rows decay — a deviation of the `_RowSparseOptimizer` kind: a row that was not looked up keeps its
        weight.  (Catching it up when it is looked up again would be wrong: that step's forward has read it already.)
      * the average is exact with respect to the weights as they moved here: a row that is not looked up has a constant
        weight w, so the k average steps it missed are a = w + m^k*(a - w), applied when the row is looked up next (an int32
        stamp per row holds the step its average was last written at) or by `materialize()` for all rows at once.
    With either argument set no fused step may apply an update (`supports_row_segments` / `supports_rows_in_step` are False and
    DeepModel.fused_plan() is None).  Averages are kept like slots: a flat group's are views of one flat buffer, zero pads
    stay zero, checkpoint.save_model stores them next to the slots."""

    weight_decay = None
    use_ema = False
    ema_momentum = 0.99
    _stage_dev = None                 # the stage's device-resident step count (DT_STAGE_STATE_BYTES)
    _stage_started = False
    _var_names = None                 # {checkpoint name: tensor}, or a callable that returns it

    @property
    def stages(self):
        """either argument is set: `step()` runs more than the plain optimizer's launches"""
        return self.weight_decay is not None or self.use_ema

    @property
    def supports_row_segments(self):
        return _GradClip.supports_row_segments.fget(self) and not self.stages

    @property
    def supports_rows_in_step(self):
        return _GradClip.supports_rows_in_step.fget(self) and not self.stages

    def _set_stages(self, weight_decay=None, use_ema=False, ema_momentum=0.99, ema_overwrite_frequency=None):
        self.weight_decay, self.use_ema, self.ema_momentum = check_stages(weight_decay, use_ema, ema_momentum,
                                                                          ema_overwrite_frequency)
        self._averages = {}           # id(param) -> its average, in the shape of the parameter
        self._stamps = {}             # id(table) -> int32 [V]: the step each row's average was last written at
        self._wd_tensors = []         # exclude_from_weight_decay(var_list=...)
        self._wd_patterns = []        # ... (var_names=...)
        self._wd_resolved = None      # the tensors the patterns name, looked up at the first step

    def _stage_hp(self):
        """the part of `hyperparameters()` that belongs to the stages: only what is set"""
        hp = {} if self.weight_decay is None else {'weight_decay': self.weight_decay}
        if self.use_ema:
            hp.update(use_ema=True, ema_momentum=self.ema_momentum)
        return hp

    def _base_hp(self):
        return dict(self._clip_hp(), **self._stage_hp())

    def _load_stage_hp(self, hp):
        """`set_hyperparameters`: stage keys in `hp` update the setting -> hp without them"""
        if any(k in hp for k in STAGE_KEYS):
            self.weight_decay, self.use_ema, self.ema_momentum = check_stages(
                hp.get('weight_decay', self.weight_decay), hp.get('use_ema', self.use_ema),
                hp.get('ema_momentum', self.ema_momentum))
        return {k: v for k, v in hp.items() if k not in STAGE_KEYS}

    def _load_base_hp(self, hp):
        return self._load_stage_hp(self._load_clip_hp(hp))

    # -- which variables decay -------------------------------------------------------------------------------
    def set_variable_names(self, names):
        """{`layer/weight`: tensor} (checkpoint.named_weights), or a callable returning it: what `exclude_from_weight_decay(
        var_names=...)` matches against.  DeepModel binds its model's names when it compiles the optimizer."""
        self._var_names = names

    def variable_names(self):
        names = self._var_names
        return dict(names() if callable(names) else names or {})

    def exclude_from_weight_decay(self, var_list=None, var_names=None):
        """Keras' BaseOptimizer.exclude_from_weight_decay: the parameters of `var_list` (a dense parameter, a packed table, one
        column's `embeddings_i`) and every variable whose checkpoint name `layer/weight` matches (`re.search`) one of the patterns
        `var_names` do not decay.  Only before the first `step()`."""
        if self._stage_started:
            raise ValueError('exclude_from_weight_decay() can only be called before the first step()')
        import re
        for pattern in var_names or []:
            re.compile(pattern)
        self._wd_tensors += [v.data if isinstance(v, torch.nn.Parameter) else v for v in (var_list or [])]
        self._wd_patterns += list(var_names or [])
        self._wd_resolved = None

    def _excluded_tensors(self):
        if self._wd_resolved is None:
            import re
            named = []
            if self._wd_patterns:
                names = self.variable_names()
                if not names:
                    raise ValueError('exclude_from_weight_decay(var_names=...) needs the variables\' names: compile the optimizer '
                                     'through DeepModel or call set_variable_names({name: tensor})')
                named = [t for name, t in names.items() if any(re.search(p, name) for p in self._wd_patterns)]
            self._wd_resolved = named
        return self._wd_tensors + self._wd_resolved

    def decay_exclusions(self, names=None):
        """the exclusions as patterns over checkpoint names (what a checkpoint stores): the patterns given, and `^name$` for
        every named variable inside a tensor of `var_list`"""
        import re
        names = self.variable_names() if names is None else names
        spans = [(t.data_ptr(), t.data_ptr() + 4 * self._span(t)) for t in self._wd_tensors]
        inside = [name for name, t in names.items() if t.is_floating_point() and
                  any(lo <= t.data_ptr() and t.data_ptr() + 4 * self._span(t) <= hi for lo, hi in spans)]
        return list(self._wd_patterns) + ['^' + re.escape(name) + '$' for name in inside]

    def _load_decay_exclusions(self, patterns):
        self._wd_tensors, self._wd_patterns, self._wd_resolved = [], list(patterns), None

    @staticmethod
    def _span(t):
        """elements between the first and the last element of t, both included (a strided block counts with what it encloses)"""
        return 1 + sum((s - 1) * st for s, st in zip(t.shape, t.stride())) if t.numel() else 0

    def _decays(self, skip, address, elements):
        return not any(lo <= address and address + 4 * elements <= hi for lo, hi in skip)

    # -- the stage's step count ------------------------------------------------------------------------------
    def _stage_state(self, device):
        if self._stage_dev is None or self._stage_dev.device != device:
            done = 0 if self._stage_dev is None else int(self._stage_dev[0].item())
            self._stage_dev = torch.zeros(DT_STAGE_STATE_WORDS, dtype=torch.int32, device=device)
            check(lib().dt_stage_state_init(ptr(self._stage_dev), done, stream_ptr()), 'dt_stage_state_init')
        return self._stage_dev

    @property
    def stage_t(self):
        """steps the stages have run (device resident; the moving average's t)"""
        return 0 if self._stage_dev is None else int(self._stage_dev[0].item())

    @stage_t.setter
    def stage_t(self, value):
        if not self.params:
            return
        self._materialize_averages()       # what is pending belongs to the old count
        check(lib().dt_stage_state_init(ptr(self._stage_state(self.params[0].device)), int(value), stream_ptr()),
              'dt_stage_state_init')
        for stamp in self._stamps.values():
            stamp.copy_(self._stage_dev[:1].expand(stamp.shape[0]))

    # -- averages --------------------------------------------------------------------------------------------
    def _flat_average(self):
        fa = self._averages.get('flat')
        if fa is None or fa.shape != self._flat[0].shape:
            fa = self._averages['flat'] = self._flat[0].detach().clone()
        return fa

    def _average_of(self, p):
        """the average of parameter p (created as a copy of p): a view of the flat average for a flat-group member"""
        a = self._averages.get(id(p))
        if a is None:
            flat = getattr(self, '_flat', None)
            if flat is not None and id(p) in flat[5]:
                a = torch.as_strided(self._flat_average(), tuple(p.data.shape), tuple(p.data.stride()),
                                     (p.data.data_ptr() - flat[0].data_ptr()) // 4)
            else:
                a = p.data.detach().clone(memory_format=torch.contiguous_format)
            self._averages[id(p)] = a
        return a

    def _rehome_flat_averages(self):
        """`register_flat_group`: the members' averages become views of one flat buffer (existing values are kept)"""
        if not self._averages:
            return
        self._averages.pop('flat', None)
        for p in self.params:
            if id(p) in self._flat[5]:
                old = self._averages.pop(id(p), None)
                if old is not None:
                    self._average_of(p).copy_(old.reshape(p.shape))

    def _row_stamps(self, table):
        """the stamps of a row-sparse table's average: a new array says that nothing is pending"""
        stamp = self._stamps.get(id(table))
        if stamp is None:
            stamp = self._stage_state(table.device)[:1].expand(table.shape[0]).contiguous()
            self._stamps[id(table)] = stamp
        return stamp

    def _materialize_averages(self):
        for p in getattr(self, 'params', ()):
            stamp, a = self._stamps.get(id(p)), self._averages.get(id(p))
            if stamp is not None and a is not None:
                check(lib().dt_ema_rows_materialize(ptr(p.data), ptr(a), ptr(stamp), p.shape[0], p.shape[1], self.ema_momentum,
                                                    ptr(self._stage_state(p.device)), stream_ptr()), 'dt_ema_rows_materialize')

    def materialize(self):
        """bring every row-sparse table's average up to the steps done (a pending catch-up is applied, the rows restamped)"""
        self._materialize_averages()

    def average(self, p):
        """the moving average of p — a parameter, or a view of one (a column's `embeddings_i`) — in its shape; None before its
        first averaged step.  A row-sparse table's average is materialised first."""
        self._materialize_averages()
        a = self._averages.get(id(p))
        if a is not None or not torch.is_tensor(p):
            return a
        from .checkpoint import _inside, _slot_piece
        for q in self.params:
            if id(q) in self._averages and _inside(p, q.data):
                return _slot_piece(self._averages[id(q)], (p.data_ptr() - q.data_ptr()) // 4, p)
        return None

    def finalize_variable_values(self):
        """Keras' BaseOptimizer.finalize_variable_values: with `use_ema`, every variable is overwritten with its average
        (DeepModel.fit calls it once after the last epoch)"""
        if not self.use_ema:
            return
        self._materialize_averages()
        with torch.no_grad():
            for p in self.params:
                a = self._averages.get(id(p))
                if a is not None:
                    p.data.copy_(a)

    # -- the stages --------------------------------------------------------------------------------------------
    def _stage_buffer(self, name, build):
        bufs = self.__dict__.setdefault('_stage_bufs', {})
        if name not in bufs:
            bufs[name] = build()
        return bufs[name]

    @staticmethod
    def _host_arrays(regions):
        """[(address, ..., elements)] -> one ctypes array of addresses per leading column and one of the sizes"""
        R = len(regions)
        cols = [ctypes.cast((ctypes.c_void_p * R)(*[r[c] for r in regions]), ctypes.c_void_p)
                for c in range(len(regions[0]) - 1)]
        return cols + [ctypes.cast((ctypes.c_int64 * R)(*[int(r[-1]) for r in regions]), ctypes.c_void_p)]

    def _stage_tables(self):
        return {id(layer.tables[k]): (layer, k) for layer in self.embedding_layers for k in getattr(layer, 'tables', {})}

    def _stages_before(self):
        """Behind the clip stage and ahead of the update: every table's sparse gradient becomes ONE coalesced piece (fields =
        -1) unless the clip stage made it one, the looked-up rows' averages catch up and the rows decay, the dense variables
        decay.  -> what `_stages_after` needs.  No host synchronisation; replays in a captured graph."""
        from .ops import SparseRowGrad
        h, st = lib(), stream_ptr()
        self._stage_started = True
        wd, lr = self.weight_decay, float(self.lr)
        skip = [(t.data_ptr(), t.data_ptr() + 4 * self._span(t)) for t in self._excluded_tensors()] if wd is not None else []
        tables = self._stage_tables()
        flat = getattr(self, '_flat', None)
        members = flat[5] if flat is not None else {}
        if flat is not None and sum(1 for p in self.params if id(p) in members and p.grad is not None) != len(members):
            flat, members = None, {}
        singles = [p for p in self.params if p.grad is not None and id(p) not in members]
        rows_ctx = []
        for layer in self.embedding_layers:
            for k, grads in list(layer.sparse_grads.items()):
                if not grads:
                    continue
                table = layer.tables[k]
                V, D = table.shape
                done = getattr(self, '_step_coalesced', {}).get(id(table))
                if done is None:
                    if any(getattr(g, 'segments', None) is not None or getattr(g, 'fields', None) == -2 for g in grads):
                        raise ValueError(f'{self._name}: weight_decay / use_ema take plain (rows, values) sparse gradients: no '
                                         f'segments, no rows applied inside a fused step')
                    out_rows, out_vals, count, n = self._coalesce(table, grads)
                    layer.sparse_grads[k] = [SparseRowGrad(out_rows, out_vals, fields=-1)]
                else:
                    out_rows, n = done
                offs, offs_dev = self._field_rows(layer, k, table)
                on = [self._decays(skip, table.data_ptr() + 4 * lo * D, (hi - lo) * D) for lo, hi in zip(offs[:-1], offs[1:])]
                decay = wd is not None and any(on)
                field_on = None
                if decay and not all(on):
                    field_on = self._stage_buffer(f'{id(table)}/on/{on}', lambda: torch.tensor(on, dtype=torch.int32,
                                                                                                 device=table.device))
                avg = stamp = sp = None
                if self.use_ema:
                    sp = self._stage_state(table.device)
                    avg, stamp = self._average_of(table), self._row_stamps(table)
                check(h.dt_rows_stage_pre(ptr(table.data), ptr(avg), ptr(stamp), ptr(out_rows), n, D, V, ptr(offs_dev),
                                          ptr(field_on), offs_dev.numel(), 1 if decay else 0, wd or 0.0, lr, self.ema_momentum,
                                          ptr(sp), st), 'dt_rows_stage_pre')
                rows_ctx.append((table, avg, stamp, out_rows, n, D, V))
        if wd is not None:
            regions, back = [], []
            if flat is not None:
                regions += [(flat[0].data_ptr() + 4 * off, span) for off, span in self._flat_regions()]
            for p in singles:
                if id(p) in tables and p.dim() == 2 and p.data.is_contiguous():     # a packed table with a dense gradient
                    offs, D = self._field_rows(*tables[id(p)], p)[0], p.shape[1]
                    regions += [(p.data_ptr() + 4 * lo * D, (hi - lo) * D) for lo, hi in zip(offs[:-1], offs[1:])]
                elif p.data.is_contiguous():
                    regions.append((p.data_ptr(), p.numel()))
                elif self._decays(skip, p.data_ptr(), self._span(p.data)):
                    # a strided parameter on its own (only some members of a flat group carry a gradient): through a copy
                    pc = p.data.contiguous()
                    back.append((p, pc))
                    regions.append((pc.data_ptr(), pc.numel()))
            regions = [r for r in regions if r[1] > 0 and self._decays(skip, *r)]
            if regions:
                check(h.dt_decay_multi(len(regions), *self._host_arrays(regions), wd, lr, st), 'dt_decay_multi')
            for p, pc in back:
                p.data.copy_(pc)
        return flat, singles, rows_ctx

    def _stages_after(self, ctx):
        """Behind the update: the looked-up rows' and the dense variables' averages take this step, the stage's count goes up"""
        if not self.use_ema:
            return
        h, st = lib(), stream_ptr()
        flat, singles, rows_ctx = ctx
        device = None
        for table, avg, stamp, out_rows, n, D, V in rows_ctx:
            device = table.device
            check(h.dt_rows_stage_post(ptr(table.data), ptr(avg), ptr(stamp), ptr(out_rows), n, D, V, self.ema_momentum,
                                       ptr(self._stage_state(device)), st), 'dt_rows_stage_post')
        regions, back = [], []
        if flat is not None:
            regions.append((flat[0].data_ptr(), self._flat_average().data_ptr(), flat[4]))
            for p in self.params:
                if id(p) in flat[5]:
                    self._average_of(p)
        for p in singles:
            a = self._average_of(p)
            if id(p) in self._stamps:
                raise ValueError(f'{self._name}: use_ema: a table whose average is kept row by row (it had sparse gradients) '
                                 f'got a dense gradient')
            pc = p.data if p.data.is_contiguous() else p.data.contiguous()
            ac = a if a.is_contiguous() else a.contiguous()
            if ac is not a:
                back.append((a, ac))
            regions.append((pc.data_ptr(), ac.data_ptr(), p.numel(), pc))
        regions = [r for r in regions if r[2] > 0]
        if regions:
            device = flat[0].device if flat is not None else singles[0].device
            check(h.dt_ema_multi(len(regions), *self._host_arrays([r[:3] for r in regions]), self.ema_momentum,
                                 ptr(self._stage_state(device)), st), 'dt_ema_multi')
        for a, ac in back:
            a.copy_(ac)
        if device is None:
            return
        check(h.dt_stage_advance(ptr(self._stage_state(device)), st), 'dt_stage_advance')


class _DeviceOptimizer(_StepStages):
    """The step driver KerasAdam, Adagrad, RMSprop, Ftrl, Adamax and MomentumSGD share.  One protocol — `zero_grad(flat=...)`, `step()`,
    `register_flat_group`, `pre_dense_hook`, `state`, `t` — and one launch order: the dense tensors in one multi-tensor
    launch (a registered flat group is ONE tensor: the fused train-step plans keep parameters and gradients of all dense
    layers in two contiguous buffers), then one row launch per packed table with a sparse gradient
    (MultiColumnEmbedding.sparse_grads), the last of which carries one dense update in its trailing blocks and advances the
    step state.  The step counter (and Adam's lr_t) live on the device (dt_adam_state_init / dt_adam_advance), so a
    captured hipGraph of the step replays with the right step.
    A subclass names its slots (`slot_names`, `slot_init`) and its entry points (`_entry`, `_hpargs()`; RMSprop's stamps go
    through `_rows_extra`), from which `_dense_call`, `_multi_call` and `_rows_call` are built — KerasAdam, whose entry points
    take other arguments, spells the three out — and, where a table's slots have a layout of their own, `_new_slot` / `_st`,
    `materialize` / `_restamp`."""

    _entry = None                     # stem of the library's entry points: dt_<_entry>_{dense,multi,rows}_step
    _row_segments = False            # `supports_row_segments` while no clip is set: takes SparseRowGrad.segments
    _rows_in_step = False             # `supports_rows_in_step` ...: a fused step may apply the update of the rows looked up once
    slot_names = ()                   # the slots' names: their keys in `state[id(p)]` and in a checkpoint
    slot_init = 0.0                   # the slots' initial value: one number, or one per slot (a tuple matching slot_names)

    def __init__(self, params, embedding_layers, clipnorm=None, clipvalue=None, global_clipnorm=None, weight_decay=None,
                 use_ema=False, ema_momentum=0.99, ema_overwrite_frequency=None):
        self._set_clip(clipnorm, clipvalue, global_clipnorm)
        self._set_stages(weight_decay, use_ema, ema_momentum, ema_overwrite_frequency)
        self.params = [p for p in params if p.requires_grad]
        self.state = {}
        self.embedding_layers = list(embedding_layers)
        self._dev_state = None        # device-resident step state (DT_ADAM_STATE_BYTES)
        # optional callable run right before the dense updates of a step (after the table updates were launched):
        # the data-parallel strategy uses it to wait for an all-reduce it started asynchronously
        self.pre_dense_hook = None
        self._flat = None             # (flat_param, flat_grad, slot 0, slot 1 or None, n, {id(param): offset})
        self._flat_views = None       # [(param, grad view)] when gradients may be accumulated straight into flat_grad

    def _betas(self):
        """(beta_1, beta_2) of the bias correction the device state keeps (lr_t); none: (0, 0)"""
        return 0.0, 0.0

    # -- step counter (device resident: int32 t_next, float lr_t, block-arrival counters) -----------------
    def _state_tensor(self, device):
        if self._dev_state is None:
            self._dev_state = torch.zeros(DT_ADAM_STATE_WORDS, dtype=torch.int32, device=device)
            check(lib().dt_adam_state_init(ptr(self._dev_state), self.lr, *self._betas(), 0, stream_ptr()),
                  'dt_adam_state_init')
        return self._dev_state

    @property
    def t(self):
        """number of completed steps (keras `optimizer.iterations`)"""
        return 0 if self._dev_state is None else int(self._dev_state[0].item()) - 1

    @t.setter
    def t(self, value):
        if not self.params:
            return
        self.materialize()                 # pending decay belongs to the old step count
        check(lib().dt_adam_state_init(ptr(self._state_tensor(self.params[0].device)), self.lr, *self._betas(), int(value),
                                       stream_ptr()), 'dt_adam_state_init')
        self._restamp()

    def materialize(self):
        """make every slot Keras' slot (RMSprop applies the decay pending on the rows of its row-sparse tables) and every
        average current (`_StepStages.materialize`)"""
        self._materialize_averages()

    def _restamp(self):
        pass

    # -- slots --------------------------------------------------------------------------------------------
    def _slot_inits(self):
        v = self.slot_init
        return tuple(v) if isinstance(v, (tuple, list)) else (v,) * len(self.slot_names)

    def _new_slot(self, p, rows):
        return {k: torch.full_like(p, v) for k, v in zip(self.slot_names, self._slot_inits())}

    def _st(self, p, rows=False):
        """slots of parameter p.  rows=True: in the layout of the row-sparse table update"""
        s = self.state.get(id(p))
        if s is None:
            s = self._new_slot(p, rows and p.dim() == 2)
            self.state[id(p)] = s
        return s

    def register_flat_group(self, flat_param, flat_grad, members, n, grad_views=False):
        """members: [(param, offset, numel[, (shape, strides)])] whose .data are views of flat_param and whose fused-plan
        gradients are the matching views of flat_grad (contiguous unless shape / strides are given: a fused plan keeps
        narrow towers inside zero-padded slabs).  Their slots become the same views of one flat buffer per slot (existing
        state is kept).  grad_views=True: `zero_grad()` zeroes flat_grad and hands its views out as `.grad` (generic
        autograd path)."""
        slots = [torch.full_like(flat_param, v) for v in self._slot_inits()]

        def view_of(flat, p, off, cnt, layout):
            if layout is None:
                return flat[off:off + cnt].view(p.shape)
            return torch.as_strided(flat, layout[0], layout[1], off)
        members = [(mb[0], mb[1], mb[2], mb[3] if len(mb) > 3 else None) for mb in members]
        for p, off, cnt, layout in members:
            old = self.state.get(id(p))
            new = {k: view_of(flat, p, off, cnt, layout) for k, flat in zip(self.slot_names, slots)}
            if old is not None:
                for k, view in new.items():
                    view.copy_(old[k].reshape(p.shape))
            self.state[id(p)] = new
        self._flat = (flat_param, flat_grad, slots[0], slots[1] if len(slots) > 1 else None, int(n),
                      {id(p): off for p, off, _, _ in members})
        self._flat_members = [(off, cnt, layout) for _, off, cnt, layout in members]       # (clip_gradients: the variables)
        self._flat_views = [(p, view_of(flat_grad, p, off, cnt, layout)) for p, off, cnt, layout in members] \
            if grad_views else None
        for p, off, cnt, layout in members:
            p._dt_grad_view = None
        self._rehome_flat_averages()
        if grad_views:                       # same tensor objects in both places (`p.grad is p._dt_grad_view`)
            for p, view in self._flat_views:
                p._dt_grad_view = view

    def _flat_grad_view(self, p):
        """flat-group member p's view of the flat GRADIENT buffer (same offset / shape / strides as its data)"""
        fp, fg = self._flat[0], self._flat[1]
        return torch.as_strided(fg, tuple(p.data.shape), tuple(p.data.stride()), (p.data.data_ptr() - fp.data_ptr()) // 4)

    def zero_grad(self, flat=True):
        """flat=True: members of the registered flat group get their (zeroed) views of the flat gradient buffer as
        `.grad` — backward kernels and autograd accumulate straight into it; flat=False: the caller (a fused step)
        fills the flat buffer itself."""
        for p in self.params:
            p.grad = None
        if flat and self._flat is not None and self._flat_views is not None:
            self._flat[1].zero_()
            for p, view in self._flat_views:
                p.grad = view
        for layer in self.embedding_layers:
            layer.sparse_grads.clear()

    # -- the three launches.  ss: one entry per slot; tail: a dense item, (None, None, (None, ..), 0) for none.  The slot
    # optimizers' entry points (csrc/optim_slots.hip) share one argument order: the slots behind the parameter, the
    # hyperparameters in the middle --
    def _hpargs(self):
        """the hyperparameters, in the order dt_<_entry>_*_step take them"""
        raise NotImplementedError

    def _rows_extra(self, s):
        """what dt_<_entry>_rows_step takes beyond the shared arguments: (pointers behind the slots, ints behind slot_stride)"""
        return (), ()

    def _call(self, form, *args):
        name = f'dt_{self._entry}_{form}_step'
        check(getattr(lib(), name)(*args), name)

    def _dense_call(self, p, g, ss, n, sp, advance, st):
        self._call('dense', ptr(p), ptr(g), *map(ptr, ss), n, *self._hpargs(), sp, advance, st)

    def _multi_call(self, T, ps, gs, ss, ns, sp, advance, st):
        self._call('multi', T, ps, gs, *ss, ns, *self._hpargs(), sp, advance, st)

    def _rows_call(self, table, s, rows, values, n, D, fields, slots, n_slots, mark, sp, tail, advance, seg, st):
        ss = [s[k] for k in self.slot_names]
        behind_slots, behind_stride = self._rows_extra(s)
        self._call('rows', ptr(table.data), *map(ptr, ss), *behind_slots, ptr(rows), ptr(values), n, D, fields, ptr(slots),
                   n_slots, ptr(mark), *self._hpargs(), sp, ptr(tail[0]), ptr(tail[1]), *map(ptr, tail[2]), tail[3], advance,
                   int(ss[0].stride(0)), *behind_stride, st)

    def _dense_launch(self, dense, sp, st, advance):
        """All dense tensors of the step in one launch (the library takes them in chunks of 32 tensors)."""
        if not dense:
            return
        if len(dense) == 1:
            pp, gg, ss, n = dense[0]
            self._dense_call(pp, gg, ss, n, sp, 1 if advance else 0, st)
            return
        T = len(dense)
        arr = ctypes.c_void_p * T
        cols = [[d[0] for d in dense], [d[1] for d in dense]] + [[d[2][k] for d in dense] for k in range(len(self.slot_names))]
        ps, gs, *ss = (ctypes.cast(arr(*[t.data_ptr() for t in col]), ctypes.c_void_p) for col in cols)
        ns = ctypes.cast((ctypes.c_int64 * T)(*[int(d[3]) for d in dense]), ctypes.c_void_p)
        self._multi_call(T, ps, gs, ss, ns, sp, 1 if advance else 0, st)

    def step(self):
        if not self.params:
            return
        sp = ptr(self._state_tensor(self.params[0].device))
        st = stream_ptr()
        if self._clip is not None or self.stages:
            # the clip stage sees the gradients the update is given: after a pending exchange has landed
            hook, self.pre_dense_hook = self.pre_dense_hook, None
            if hook is not None:
                hook()
            self.clip_gradients()
        # weight decay ahead of the update, the moving average behind it: the update between them is the plain optimizer's
        stages = self._stages_before() if self.stages else None
        # every launch of the step reads the device state; the LAST one advances it (no extra launch)
        dense = []                                        # (param, grad, (slot, ..), n)
        flat_done = set()
        if self._flat is not None:
            fp, fg, fs0, fs1, n, members = self._flat
            with_grad = [p for p in self.params if id(p) in members and p.grad is not None]
            if len(with_grad) == len(members):
                # gradients that are NOT the members' views of the flat gradient buffer (the layer-by-layer path after a
                # fused plan re-homed the parameters: a weighted step, DT_AMD_FUSED toggled, ...) are scattered into it:
                # members of a plan with a narrow tower are STRIDED views of zero-padded slabs (fused._mirror_in_flat),
                # which the per-tensor kernels — they take (pointer, numel) — must not see one by one.  Pads have a zero
                # gradient (and zero moments): they stay exactly as they are.
                in_flat = {id(p) for p in with_grad if p.grad.data_ptr() == fg.data_ptr() + 4 * members[id(p)]}
                if len(in_flat) != len(members):
                    if not in_flat:
                        fg.zero_()
                    for p in with_grad:
                        if id(p) not in in_flat:
                            view = self._flat_grad_view(p)
                            view.copy_(p.grad.reshape(view.shape))
                dense.append((fp, fg, (fs0,) if fs1 is None else (fs0, fs1), n))       # one launch
                flat_done = set(members)
        deferred = []                                     # (param, slots, contiguous copies) of strided tensors
        for p in self.params:
            if p.grad is None or id(p) in flat_done:
                continue
            s = self._st(p)
            ss = tuple(s[k] for k in self.slot_names)
            if p.data.is_contiguous() and all(x.is_contiguous() for x in ss):
                dense.append((p.data, p.grad.contiguous(), ss, p.numel()))
            else:
                # a strided parameter / slot on its own (only some members of a flat group carry a gradient): update
                # contiguous copies and write them back after the launches below
                pc, sc = p.data.contiguous(), tuple(x.contiguous() for x in ss)
                dense.append((pc, p.grad.contiguous(), sc, p.numel()))
                deferred.append((p, ss, pc, sc))
        sparse = [(layer, key, grads) for layer in self.embedding_layers for key, grads in layer.sparse_grads.items()]
        # launch order: dense updates that cannot ride along, then the table updates; the last table update carries
        # one dense update (normally the model's flat buffer) in its trailing blocks and advances the state
        hook, self.pre_dense_hook = self.pre_dense_hook, None
        dense_after = hook is not None and bool(sparse)     # table updates first, overlapping the pending reduce
        tail = dense.pop(0) if (sparse and dense and not dense_after) else None
        if hook is not None and not dense_after:
            hook()
        if not dense_after:
            self._dense_launch(dense, sp, st, advance=not sparse)
        if not sparse and not dense:
            check(lib().dt_adam_advance(sp, self.lr, *self._betas(), st), 'dt_adam_advance')
        for i, (layer, key, grads) in enumerate(sparse):
            table = layer.tables[key]
            s = self._st(table, rows=True)
            D = table.shape[1]
            segmented = any(getattr(g, 'segments', None) is not None for g in grads)
            in_step = any(getattr(g, 'fields', None) == -2 for g in grads)
            if (segmented and not self.supports_row_segments) or (in_step and not self.supports_rows_in_step):
                raise ValueError(f'{self._name}: a sparse gradient with segments or rows applied inside the step')
            if len(grads) == 1:
                rows, values = grads[0].rows, grads[0].values
            else:
                rows = torch.cat([g.rows.reshape(-1) for g in grads])
                values = torch.cat([g.values.reshape(-1, D) for g in grads])
            n = rows.numel()
            fields = len(dict(layer.groups)[D]) if hasattr(layer, 'groups') else 0
            hints = {getattr(g, 'fields', None) for g in grads}
            if hints != {None}:                           # an explicit layout promise overrides the layer default
                fields = hints.pop() if len(hints) == 1 else 0
                fields = 0 if fields is None else int(fields)
            if fields == -2 and len(grads) != 1:
                raise ValueError('a sparse gradient whose rows were applied inside the step cannot be concatenated')
            if fields == -1 and len(grads) != 1:
                fields = 0                                # distinct within each piece only
            values = values if values.is_contiguous() else values.contiguous()
            if fields in (-1, -2):
                slots = mark = None
                n_slots = 0
            else:
                n_slots = lib().dt_adam_rows_slots(n)
                if s.get('n_slots', 0) < n_slots or s['mark'].numel() < n:
                    s['slots'] = torch.zeros(n_slots, dtype=torch.int64, device=table.device)
                    s['mark'] = torch.empty(n, dtype=torch.int32, device=table.device)
                    s['n_slots'] = n_slots
                slots, mark, n_slots = s['slots'], s['mark'], s['n_slots']
            is_last = i == len(sparse) - 1 and not (dense_after and dense)
            tl = tail if (is_last and tail is not None) else (None, None, (None,) * len(self.slot_names), 0)
            seg = grads[0].segments if (segmented and len(grads) == 1) else None
            if segmented and seg is None:
                raise ValueError('a segmented sparse gradient cannot be concatenated with other pieces')
            self._rows_call(table, s, rows, values, n, D, fields, slots, n_slots, mark, sp, tl, 1 if is_last else 0, seg, st)
        if dense_after:
            hook()
            self._dense_launch(dense, sp, st, advance=True)
        for p, ss, pc, sc in deferred:
            p.data.copy_(pc)
            for x, xc in zip(ss, sc):
                x.copy_(xc)
        if stages is not None:
            self._stages_after(stages)
        for layer in self.embedding_layers:
            layer.sparse_grads.clear()


class KerasAdam(_DeviceOptimizer):
    """keras.optimizers.Adam(learning_rate=1e-3, beta_1=.9, beta_2=.999, epsilon=1e-7):
        lr_t = lr*sqrt(1-b2^t)/(1-b1^t);  p -= lr_t*m/(sqrt(v)+eps).
    Dense parameters: one fused HIP launch for all of them — or for a whole registered flat group.
    Packed embedding tables with a sparse gradient: duplicate lookups merged through a per-step hash of the row ids, then
    a row-sparse ("lazy") update of only the rows touched this step — a documented deviation from Keras' dense
    semantics for tables too large to sweep every step.

    exact_rows=True closes that deviation (csrc/adam_exact.hip): Keras gives a row that was not looked up
    gradient 0 and still moves it — m and v decay, the weight coasts on the decayed momentum.  Here such a row waits: an int32
    stamp per row holds the number of steps its weight and slots are current through, and the k idle steps it owes are paid
    before anything reads it — by a launch ahead of the gather for the rows a batch looks up (the embedding layers'
    `pre_lookup` hook, in training and in evaluation alike), by `materialize()` for all rows at once (DeepModel calls it before
    an inference plan reads the tables and before it saves).  The row update itself is the lazy path's: for a row that is
    current it IS Keras' dense step.  Weights are Keras' after every step, m and v to rounding.  No fused step runs in this
    mode (`supports_row_segments` / `supports_rows_in_step` are False, DeepModel.fused_plan() is None), and it is refused
    together with `weight_decay`, `use_ema` or a distribute_strategy, whose lazy-row rules would need a joint definition."""

    _row_segments = True              # dt_adam_rows_step_seg
    _rows_in_step = True
    slot_names = ('m', 'v')
    _name = 'Adam'
    exact_rows = False
    _pending = False                  # exact_rows: a step ran since the last sweep (`materialize()` costs nothing otherwise)

    def __init__(self, params, embedding_layers=(), learning_rate=1e-3, beta_1=0.9, beta_2=0.999, epsilon=1e-7,
                 clipnorm=None, clipvalue=None, global_clipnorm=None, weight_decay=None, use_ema=False, ema_momentum=0.99,
                 ema_overwrite_frequency=None, exact_rows=False):
        super().__init__(params, embedding_layers, clipnorm, clipvalue, global_clipnorm, weight_decay, use_ema, ema_momentum,
                         ema_overwrite_frequency)
        self.lr, self.b1, self.b2, self.eps = learning_rate, beta_1, beta_2, epsilon
        self._applied_in_step = False  # a fused step ran this step's whole update itself (applied_in_step)
        self._set_exact_rows(exact_rows)

    def _betas(self):
        return self.b1, self.b2

    # -- exact_rows ---------------------------------------------------------------------------------------
    @staticmethod
    def idle_term_ratio(beta_1, beta_2):
        """rho = sup_t (lr_{t+1} / lr_t) * beta_1 / sqrt(beta_2): the most by which the term lr_t m / (sqrt(v) + eps) of an idle
        row can grow from one step to the next (m shrinks by beta_1, sqrt(v) + eps by sqrt(beta_2) at the most).  rho < 1 is
        what lets the catch-up loop stop early.  lr_t / lr = sqrt(1 - beta_2^t) / (1 - beta_1^t) tends to 1: the supremum is
        taken over the steps until both powers are below 1e-18 (four million steps at the most), and 1 for all later ones."""
        b1, b2 = float(beta_1), float(beta_2)
        if not (0.0 <= b1 < 1.0 and 0.0 < b2 < 1.0):
            return math.inf
        if b1 == 0.0:
            return 0.0
        n = int(min(math.ceil(math.log(1e-18) / math.log(max(b1, b2))) + 2, 1 << 22))
        t = np.arange(1, n + 1, dtype=np.float64)
        lr_t = np.sqrt(-np.expm1(t * math.log(b2))) / -np.expm1(t * math.log(b1))
        return float(max(1.0, (lr_t[1:] / lr_t[:-1]).max()) * b1 / math.sqrt(b2))

    def _set_exact_rows(self, on):
        if not isinstance(on, (bool, np.bool_)):
            raise ValueError(f'`exact_rows` must be True or False, got {on!r}')
        on = bool(on)
        if on:
            if self.stages:
                which = '`weight_decay`' if self.weight_decay is not None else '`use_ema`'
                raise ValueError(f'Adam: `exact_rows` with {which}: the decay and the moving average of a row that waits for its '
                                 f'idle steps have no definition yet; use one or the other')
            rho = self.idle_term_ratio(self.b1, self.b2)
            if not rho < 1.0:
                raise ValueError(f'Adam: `exact_rows` needs beta_1 < sqrt(beta_2) with room to spare: the idle steps of a row are '
                                 f'summed until their terms stop moving the weight, and with beta_1={self.b1!r}, '
                                 f'beta_2={self.b2!r} a term can be {rho:.4g} times the one before it (the bound must be < 1)')
        if on != self.exact_rows:
            import functools
            if not on:
                self.materialize()             # what is pending belongs to the mode that is being left
                for s in self.state.values():
                    s.pop('stamp', None)
            for layer in self.embedding_layers:
                layer.pre_lookup = functools.partial(self._pre_lookup, layer) if on else None
        self.exact_rows = on

    @property
    def supports_row_segments(self):
        return _StepStages.supports_row_segments.fget(self) and not self.exact_rows

    @property
    def supports_rows_in_step(self):
        return _StepStages.supports_rows_in_step.fget(self) and not self.exact_rows

    def _pre_lookup(self, layer, key, idx):
        """the layers' hook, ahead of the gather of `idx` [B, F] from `layer.tables[key]`: the rows the batch looks up pay
        the idle steps they owe (dt_adam_rows_catchup).  No host synchronisation; replays in a captured graph."""
        table = layer.tables[key]
        if not table.requires_grad or not table.is_cuda:
            return
        s = self._st(table, rows=True)
        idx = idx.contiguous()
        from .ops import _idx_kind
        B, F = idx.shape
        V, D = table.shape
        check(lib().dt_adam_rows_catchup(ptr(table.data), ptr(s['m']), ptr(s['v']), int(s['m'].stride(0)), ptr(s['stamp']),
                                         ptr(idx), _idx_kind(idx), ptr(getattr(layer, f'row_offset_{key}')),
                                         ptr(getattr(layer, f'vocab_{key}')), B, F, D, V, self.lr, self.b1, self.b2, self.eps,
                                         ptr(self._state_tensor(table.device)), stream_ptr()), 'dt_adam_rows_catchup')

    def _materialize_one(self, p, s):
        check(lib().dt_adam_rows_materialize(ptr(p.data), ptr(s['m']), ptr(s['v']), int(s['m'].stride(0)), ptr(s['stamp']),
                                             p.shape[0], p.shape[1], self.lr, self.b1, self.b2, self.eps,
                                             ptr(self._state_tensor(p.device)), stream_ptr()), 'dt_adam_rows_materialize')

    def materialize(self):
        """exact_rows: every row of every row-sparse table pays the idle steps it owes — weights, m and v are Keras' for the
        steps done, every stamp is current.  Free while no step ran since the last sweep."""
        if self._pending:
            for p in self.params:
                s = self.state.get(id(p))
                if s is not None and 'stamp' in s:
                    self._materialize_one(p, s)
            self._pending = False
        self._materialize_averages()

    def steps_replayed(self):
        """a captured graph that holds this optimizer's step was replayed (compiled.CompiledTrainLoop): `step()` did not run
        on the host, yet rows are pending again"""
        self._pending = self.exact_rows

    def _restamp(self):
        for p in self.params:
            s = self.state.get(id(p))
            if s is not None and 'stamp' in s:
                s['stamp'].copy_((self._dev_state[:1] - 1).expand(p.shape[0]))

    def hyperparameters(self):
        """what travels with a checkpoint: the clip, decay and average settings and `exact_rows`, each only when set (Adam's
        other arguments are the constructor's, as they were)"""
        return dict(self._base_hp(), **({'exact_rows': True} if self.exact_rows else {}))

    def set_hyperparameters(self, hp):
        before = (self._clip, self.weight_decay, self.use_ema, self.ema_momentum)
        rest = self._load_base_hp(hp)
        try:
            want = bool(rest.get('exact_rows', self.exact_rows))
            if want != self.exact_rows or (want and self.stages):
                self._set_exact_rows(want)      # (raises when the stages just loaded do not go with the mode)
        except ValueError:
            self._clip, self.weight_decay, self.use_ema, self.ema_momentum = before     # a refused update changes nothing
            raise

    def _new_slot(self, p, rows):
        """rows (the row-sparse table update): m and v of a row side by side in ONE [V, 2, D] array (a 128-byte line at
        D = 16), so the update touches two random locations per row instead of three; `m` / `v` are its strided views.
        exact_rows: and `stamp`, int32 [V], created as the steps done: nothing is pending on a new slot."""
        if not rows:
            return super()._new_slot(p, rows)
        mv = torch.zeros((p.shape[0], 2, p.shape[1]), dtype=p.dtype, device=p.device)
        s = {'m': mv[:, 0, :], 'v': mv[:, 1, :], 'mv': mv}
        if self.exact_rows:
            s['stamp'] = (self._state_tensor(p.device)[:1] - 1).expand(p.shape[0]).contiguous()
        return s

    def _st(self, p, rows=False):
        s = self.state.get(id(p))
        if s is not None and not rows and 'mv' in s:          # the dense update needs contiguous slots: convert back
            if 'stamp' in s:                                  # ... of a table that is current
                self._materialize_one(p, s)
            self.state[id(p)] = {'m': s['m'].contiguous(), 'v': s['v'].contiguous()}
        elif s is not None and rows and self.exact_rows and p.dim() == 2 and 'stamp' not in s:
            old, s = s, self._new_slot(p, True)               # slots from before the mode (or a dense update): current
            s['m'].copy_(old['m'].reshape(p.shape))
            s['v'].copy_(old['v'].reshape(p.shape))
            self.state[id(p)] = s
        return super()._st(p, rows)

    def zero_grad(self, flat=True):
        # _forward_backward(apply_rows=True) is a promise that step() follows at once: the rows looked up once were already
        # updated inside the step.  A gradient of that kind still pending here means the promise was broken (the segments and
        # the dense parameters never got their half of the update): fail loudly instead of training on half-applied steps
        if not self._applied_in_step:
            for layer in self.embedding_layers:
                for grads in layer.sparse_grads.values():
                    if any(getattr(g, 'fields', None) == -2 for g in grads):
                        raise RuntimeError('_forward_backward(apply_rows=True) was not followed by optimizer.step(): the '
                                           'table rows looked up once are updated, the segments and dense parameters are not')
        self._applied_in_step = False
        super().zero_grad(flat)

    def applied_in_step(self):
        """A fused train step (fused.FusedDeepFM with dt_deepfm_train_step_adam) has applied THIS step's whole update —
        table rows, segments, every dense element — and advanced the device step state inside its own launches: the
        `step()` call that follows only drops the gradients."""
        self._applied_in_step = True

    def step(self):
        if self.params and self._applied_in_step:
            self._applied_in_step = False
            for layer in self.embedding_layers:
                layer.sparse_grads.clear()
            return
        if not (self.exact_rows and self.params):
            super().step()
            return
        # exact_rows: the rows this step updates are current through it once its last update has advanced the state — a launch
        # of its own, so that a forward that no step follows leaves consistent stamps too
        updated = [(layer.tables[key], [g.rows for g in grads]) for layer in self.embedding_layers
                   for key, grads in layer.sparse_grads.items() if grads]
        self._pending = True
        super().step()
        for table, pieces in updated:
            s = self.state.get(id(table))
            if s is None or 'stamp' not in s:
                continue
            for rows in pieces:
                rows = rows.reshape(-1)
                rows = rows if rows.is_contiguous() else rows.contiguous()
                check(lib().dt_adam_rows_stamp(ptr(s['stamp']), ptr(rows), rows.numel(), table.shape[0],
                                               ptr(self._state_tensor(table.device)), stream_ptr()), 'dt_adam_rows_stamp')

    def _dense_call(self, p, g, ss, n, sp, advance, st):
        check(lib().dt_adam_dense_step(ptr(p), ptr(g), ptr(ss[0]), ptr(ss[1]), n, 0.0, self.b1, self.b2, self.eps, sp, advance,
                                       self.lr, st), 'dt_adam_dense_step')

    def _multi_call(self, T, ps, gs, ss, ns, sp, advance, st):
        check(lib().dt_adam_multi_step(T, ps, gs, ss[0], ss[1], ns, 0.0, self.b1, self.b2, self.eps, sp, advance, self.lr, st),
              'dt_adam_multi_step')

    def _rows_call(self, table, s, rows, values, n, D, fields, slots, n_slots, mark, sp, tail, advance, seg, st):
        sg = [ptr(t) for t in seg[:5]] + [int(seg[5]), int(seg[6])] if seg is not None else [None] * 5 + [0, 0]
        check(lib().dt_adam_rows_step_seg(ptr(table.data), ptr(s['m']), ptr(s['v']), ptr(rows), ptr(values), n, D, fields,
                                          ptr(slots), n_slots, ptr(mark), 0.0, self.b1, self.b2, self.eps, sp, ptr(tail[0]),
                                          ptr(tail[1]), ptr(tail[2][0]), ptr(tail[2][1]), tail[3], advance, self.lr, *sg,
                                          int(s['m'].stride(0)), st), 'dt_adam_rows_step_seg')


class SGD(_StepStages):
    """keras.optimizers.SGD(learning_rate=0.01, momentum=0.0, nesterov=False).  momentum == 0: p -= lr*g, one launch per
    tensor and per sparse-gradient piece, no state.  momentum != 0: `SGD(...)` returns a `MomentumSGD`, which runs on the
    step driver (one slot `momentum`); both answer to the name 'SGD'."""

    _name = 'SGD'

    def __new__(cls, params=(), embedding_layers=(), learning_rate=0.01, momentum=0.0, nesterov=False, clipnorm=None,
                clipvalue=None, global_clipnorm=None, weight_decay=None, use_ema=False, ema_momentum=0.99,
                ema_overwrite_frequency=None):
        if not 0 <= momentum <= 1:
            raise ValueError(f'`momentum` must be in the range [0, 1], got {momentum!r}')
        if cls is SGD and momentum != 0:
            return MomentumSGD(params, embedding_layers, learning_rate, momentum, nesterov, clipnorm, clipvalue, global_clipnorm,
                               weight_decay, use_ema, ema_momentum, ema_overwrite_frequency)
        return super().__new__(cls)

    def __init__(self, params, embedding_layers=(), learning_rate=0.01, momentum=0.0, nesterov=False, clipnorm=None,
                 clipvalue=None, global_clipnorm=None, weight_decay=None, use_ema=False, ema_momentum=0.99,
                 ema_overwrite_frequency=None):
        self._set_clip(clipnorm, clipvalue, global_clipnorm)
        self._set_stages(weight_decay, use_ema, ema_momentum, ema_overwrite_frequency)
        self.lr = learning_rate
        self.params = [p for p in params if p.requires_grad]
        self.embedding_layers = list(embedding_layers)

    def hyperparameters(self):
        return dict({'learning_rate': self.lr, 'momentum': 0.0, 'nesterov': False}, **self._base_hp())

    def set_hyperparameters(self, hp):
        self.lr = float(self._load_base_hp(hp).get('learning_rate', self.lr))

    def zero_grad(self):
        for p in self.params:
            p.grad = None
        for layer in self.embedding_layers:
            layer.sparse_grads.clear()

    def step(self):
        st = stream_ptr()
        self.clip_gradients()
        stages = self._stages_before() if self.stages else None
        for p in self.params:
            if p.grad is not None:
                g = p.grad.contiguous()
                check(lib().dt_sgd_dense_step(ptr(p.data), ptr(g), p.numel(), self.lr, st), 'dt_sgd_dense_step')
        for layer in self.embedding_layers:
            for key, grads in layer.sparse_grads.items():
                table = layer.tables[key]
                for gr in grads:
                    vals = gr.values if gr.values.is_contiguous() else gr.values.contiguous()
                    check(lib().dt_sgd_rows_step(ptr(table.data), ptr(gr.rows), ptr(vals), gr.rows.numel(),
                                                 table.shape[1], self.lr, st), 'dt_sgd_rows_step')
        if stages is not None:
            self._stages_after(stages)
        for layer in self.embedding_layers:
            layer.sparse_grads.clear()


class _SlotOptimizer(_DeviceOptimizer):
    """What keras.optimizers.Adagrad and RMSprop (momentum 0) share beyond the step driver: ONE slot per element, no bias
    correction, and hyperparameters that travel with a checkpoint.  Unlike Adam's, their row-sparse update IS Keras' result
    (a row that was not looked up has a zero gradient and does not move).  The row entry points take no segments: the fused
    DeepFM / DCN plans run forward + backward, hand over plain (rows, values) and leave the whole update to `step()`, as
    they do for SGD."""

    def __init__(self, params, embedding_layers, learning_rate, epsilon, clipnorm=None, clipvalue=None, global_clipnorm=None,
                 weight_decay=None, use_ema=False, ema_momentum=0.99, ema_overwrite_frequency=None):
        super().__init__(params, embedding_layers, clipnorm, clipvalue, global_clipnorm, weight_decay, use_ema, ema_momentum,
                         ema_overwrite_frequency)
        self.lr, self.eps = float(learning_rate), float(epsilon)

    def slot(self, p):
        """the slot of parameter p as Keras holds it (shape of p), or None before p's first update"""
        self.materialize()
        s = self.state.get(id(p))
        return None if s is None else s[self.slot_names[0]]

    def hyperparameters(self):
        return dict({'learning_rate': self.lr, 'epsilon': self.eps}, **self._base_hp())

    def set_hyperparameters(self, hp):
        hp = self._load_base_hp(hp)
        self.lr, self.eps = float(hp.get('learning_rate', self.lr)), float(hp.get('epsilon', self.eps))


class Adagrad(_SlotOptimizer):
    """keras.optimizers.Adagrad(learning_rate=1e-3, initial_accumulator_value=0.1, epsilon=1e-7):
        acc += g*g;  p -= lr*g/(sqrt(acc)+eps),  acc starts at initial_accumulator_value.
    Row-sparse tables: duplicate lookups summed (Keras `_deduplicate_indexed_slices`), every looked-up row updated once;
    the other rows keep p and acc bit for bit."""

    _name = 'Adagrad'
    _entry = 'adagrad'
    slot_names = ('acc',)

    def __init__(self, params, embedding_layers=(), learning_rate=1e-3, initial_accumulator_value=0.1, epsilon=1e-7,
                 clipnorm=None, clipvalue=None, global_clipnorm=None, weight_decay=None, use_ema=False, ema_momentum=0.99,
                 ema_overwrite_frequency=None):
        if initial_accumulator_value < 0:
            raise ValueError(f'initial_accumulator_value must be non-negative, got {initial_accumulator_value}')
        super().__init__(params, embedding_layers, learning_rate, epsilon, clipnorm, clipvalue, global_clipnorm, weight_decay,
                         use_ema, ema_momentum, ema_overwrite_frequency)
        self.initial_accumulator_value = self.slot_init = float(initial_accumulator_value)

    def hyperparameters(self):
        return dict(super().hyperparameters(), initial_accumulator_value=self.initial_accumulator_value)

    def _hpargs(self):
        return self.lr, self.eps


class RMSprop(_SlotOptimizer):
    """keras.optimizers.RMSprop(learning_rate=1e-3, rho=0.9, momentum=0.0, epsilon=1e-7, centered=False):
        rms = rho*rms + (1-rho)*g*g;  p -= lr*g/(sqrt(rms)+eps),  rms starts at 0.
    momentum != 0 and centered=True use another formula and are refused.
    Row-sparse tables: Keras decays rms of EVERY row each step and moves the looked-up rows.  Here a row's decay waits until
    the row is looked up again: an int32 stamp per row holds the step at which its rms was last written, and the row update
    first applies rho^(t - stamp - 1).  The looked-up rows' weights are Keras' after every step; `materialize()` applies what
    is pending on all rows, after which `rms` is Keras' slot (`slot(p)` and checkpoint.save_model call it)."""

    _name = 'RMSprop'
    _entry = 'rmsprop'
    slot_names = ('rms',)
    # where a row-sparse table's stamps live: False: an int32 [V] array of their own (rms rows stay 16 D bytes apart:
    # one 128-byte line at D = 32); True: the last 16 bytes of a [V, D + 4] slot record.  DESIGN.md §3.6 has the measurement.
    stamp_in_record = False

    def __init__(self, params, embedding_layers=(), learning_rate=1e-3, rho=0.9, momentum=0.0, epsilon=1e-7, centered=False,
                 clipnorm=None, clipvalue=None, global_clipnorm=None, weight_decay=None, use_ema=False, ema_momentum=0.99,
                 ema_overwrite_frequency=None):
        if momentum != 0 or centered:
            raise ValueError('RMSprop: momentum != 0 and centered=True are not supported (Keras switches to another '
                             f'update formula for them); got momentum={momentum!r}, centered={centered!r}')
        super().__init__(params, embedding_layers, learning_rate, epsilon, clipnorm, clipvalue, global_clipnorm, weight_decay,
                         use_ema, ema_momentum, ema_overwrite_frequency)
        self.rho, self.momentum, self.centered = float(rho), 0.0, False

    def hyperparameters(self):
        return dict(super().hyperparameters(), rho=self.rho, momentum=0.0, centered=False)

    def set_hyperparameters(self, hp):
        super().set_hyperparameters(hp)
        self.rho = float(hp.get('rho', self.rho))

    def _new_slot(self, p, rows):
        if not rows:
            return super()._new_slot(p, rows)
        V, D = p.shape
        if self.stamp_in_record:
            rec = torch.zeros((V, D + 4), dtype=p.dtype, device=p.device)
            s = {'rms': rec[:, :D], 'stamp': rec[:, D].view(torch.int32), 'rec': rec}
        else:
            s = {'rms': torch.zeros_like(p), 'stamp': torch.zeros(V, dtype=torch.int32, device=p.device)}
        s['stamp'].copy_((self._state_tensor(p.device)[:1] - 1).expand(V))       # nothing is pending on a new slot
        return s

    def _st(self, p, rows=False):
        s = self.state.get(id(p))
        if s is not None and not rows and 'stamp' in s:       # a dense update of a table that has row-sparse slots
            self._materialize_one(p, s)
            s = {'rms': s['rms'].contiguous()}
            self.state[id(p)] = s
        elif s is not None and rows and p.dim() == 2 and 'stamp' not in s:
            old, s = s, self._new_slot(p, True)
            s['rms'].copy_(old['rms'].reshape(p.shape))
            self.state[id(p)] = s
        return super()._st(p, rows)

    def _materialize_one(self, p, s):
        rms, stamp = s['rms'], s['stamp']
        check(lib().dt_rmsprop_rows_materialize(ptr(rms), ptr(stamp), p.shape[0], p.shape[1], int(rms.stride(0)),
                                                int(stamp.stride(0)), self.rho, ptr(self._state_tensor(p.device)),
                                                stream_ptr()), 'dt_rmsprop_rows_materialize')

    def materialize(self):
        for p in self.params:
            s = self.state.get(id(p))
            if s is not None and 'stamp' in s:
                self._materialize_one(p, s)
        self._materialize_averages()

    def _restamp(self):
        for p in self.params:
            s = self.state.get(id(p))
            if s is not None and 'stamp' in s:
                s['stamp'].copy_((self._dev_state[:1] - 1).expand(p.shape[0]))

    def _hpargs(self):
        return self.lr, self.rho, self.eps

    def _rows_extra(self, s):
        return (ptr(s['stamp']),), (int(s['stamp'].stride(0)),)


class _RowSparseOptimizer(_DeviceOptimizer):
    """What momentum SGD, Adamax and Ftrl (csrc/optim_slots.hip) share beyond the step driver: one or two slots per element,
    each with its own initial value, and hyperparameters that travel with a checkpoint.

    Their row-sparse update is NOT Keras' dense result — a deviation of the kind of Adam's "lazy" rows (`KerasAdam`), and
    unlike Adagrad's.  Only the looked-up rows are updated, duplicates summed first; every other row keeps its weights and
    its slots bit for bit: its momentum does not coast, Adamax's `u` does not decay, and Ftrl neither shrinks it nor
    recomputes it from (`linear`, `accumulator`).  That is TensorFlow's sparse apply, and what a table too large to sweep
    every step needs; it takes no stamps and no `materialize()`.  A table with a DENSE gradient follows the formulas
    literally, on every row.

    The two slots of a row-sparse table live in ONE [V, 2, D] record (as `KerasAdam._new_slot`): a row update touches two
    random locations, not three; the named slots are its strided views.  The row entry points take no segments: the fused
    DeepFM / DCN plans run forward + backward and hand plain (rows, values) to `step()`."""

    _hp = ()                          # constructor arguments beyond (params, embedding_layers), in order

    def _new_slot(self, p, rows):
        if not rows or len(self.slot_names) != 2:
            return super()._new_slot(p, rows)
        rec = torch.empty((p.shape[0], 2, p.shape[1]), dtype=p.dtype, device=p.device)
        for k, v in enumerate(self._slot_inits()):
            rec[:, k, :].fill_(v)
        return {self.slot_names[0]: rec[:, 0, :], self.slot_names[1]: rec[:, 1, :], 'rec': rec}

    def _st(self, p, rows=False):
        s = self.state.get(id(p))
        if s is not None and not rows and 'rec' in s:         # the dense update needs contiguous slots: convert back
            self.state[id(p)] = {k: s[k].contiguous() for k in self.slot_names}
        elif s is not None and rows and p.dim() == 2 and len(self.slot_names) == 2 and 'rec' not in s:
            old, s = s, self._new_slot(p, True)
            for k in self.slot_names:
                s[k].copy_(old[k].reshape(p.shape))
            self.state[id(p)] = s
        return super()._st(p, rows)

    def slot(self, p, name=None):
        """the slot `name` (default: the first) of parameter p in the shape of p, or None before p's first update"""
        s = self.state.get(id(p))
        return None if s is None else s[name or self.slot_names[0]]

    def hyperparameters(self):
        return dict({k: getattr(self, k) for k in self._hp}, **self._base_hp())

    def set_hyperparameters(self, hp):
        unknown = sorted(set(hp) - set(self._hp) - set(CLIP_KEYS) - set(STAGE_KEYS))
        if unknown:
            raise ValueError(f'{self._name}: unknown hyperparameters {unknown} (accepted: '
                             f'{list(self._hp + CLIP_KEYS + STAGE_KEYS)})')
        check_clip(**{k: hp.get(k) for k in CLIP_KEYS})                   # a refused update changes nothing
        check_stages(**{k: hp[k] for k in STAGE_KEYS if k in hp})
        self._check(**dict({k: getattr(self, k) for k in self._hp},
                           **{k: v for k, v in hp.items() if k not in CLIP_KEYS + STAGE_KEYS}))
        hp = self._load_base_hp(hp)
        for k, v in hp.items():
            setattr(self, k, type(getattr(self, k))(v))

    @staticmethod
    def _check(**hp):
        pass

    @property
    def lr(self):
        return self.learning_rate


class MomentumSGD(_RowSparseOptimizer):
    """keras.optimizers.SGD(learning_rate=0.01, momentum, nesterov=False) with momentum != 0 (what `SGD(...)` returns then):
        m = momentum*m - lr*g;  p += m          (nesterov: p += momentum*m - lr*g),  m starts at 0.
    Row-sparse tables: see `_RowSparseOptimizer` — rows that were not looked up do not coast on their momentum."""

    _name = 'SGD'
    _entry = 'sgdm'
    slot_names = ('momentum',)
    _hp = ('learning_rate', 'momentum', 'nesterov')

    def __init__(self, params, embedding_layers=(), learning_rate=0.01, momentum=0.9, nesterov=False, clipnorm=None,
                 clipvalue=None, global_clipnorm=None, weight_decay=None, use_ema=False, ema_momentum=0.99,
                 ema_overwrite_frequency=None):
        self._check(momentum=momentum)
        super().__init__(params, embedding_layers, clipnorm, clipvalue, global_clipnorm, weight_decay, use_ema, ema_momentum,
                         ema_overwrite_frequency)
        self.learning_rate, self.momentum, self.nesterov = float(learning_rate), float(momentum), bool(nesterov)

    @staticmethod
    def _check(momentum=0.9, **_):
        if not 0 < momentum <= 1:
            raise ValueError(f'`momentum` must be in the range (0, 1] on the momentum path ([0, 1] for SGD), got {momentum!r}')

    def _hpargs(self):
        return self.learning_rate, self.momentum, int(self.nesterov)


class Adamax(_RowSparseOptimizer):
    """keras.optimizers.Adamax(learning_rate=1e-3, beta_1=0.9, beta_2=0.999, epsilon=1e-7):
        m += (g - m)*(1 - beta_1);  u = max(beta_2*u, |g|);  p -= lr*m / ((1 - beta_1^t)*(u + eps)),  m and u start at 0.
    beta_1^t is computed on the device from the device-resident step count, so a captured graph replays with the right power.
    Row-sparse tables: see `_RowSparseOptimizer` — m and u of rows that were not looked up do not decay."""

    _name = 'Adamax'
    _entry = 'adamax'
    slot_names = ('m', 'u')
    _hp = ('learning_rate', 'beta_1', 'beta_2', 'epsilon')

    def __init__(self, params, embedding_layers=(), learning_rate=1e-3, beta_1=0.9, beta_2=0.999, epsilon=1e-7,
                 clipnorm=None, clipvalue=None, global_clipnorm=None, weight_decay=None, use_ema=False, ema_momentum=0.99,
                 ema_overwrite_frequency=None):
        super().__init__(params, embedding_layers, clipnorm, clipvalue, global_clipnorm, weight_decay, use_ema, ema_momentum,
                         ema_overwrite_frequency)
        self.learning_rate, self.beta_1, self.beta_2, self.epsilon = float(learning_rate), float(beta_1), float(beta_2), \
            float(epsilon)

    def _hpargs(self):
        return self.learning_rate, self.beta_1, self.beta_2, self.epsilon


class Ftrl(_RowSparseOptimizer):
    """keras.optimizers.Ftrl(learning_rate=1e-3, learning_rate_power=-0.5, initial_accumulator_value=0.1,
    l1_regularization_strength=0, l2_regularization_strength=0, l2_shrinkage_regularization_strength=0, beta=0); slots
    `accumulator` (n, starts at initial_accumulator_value) and `linear` (starts at 0); with l2' = l2 + beta/(2 lr):
        g' = g + 2*l2_shrinkage*p;  n' = n + g^2;  linear += g' - (n'^(-lr_power) - n^(-lr_power))/lr * p
        q = n'^(-lr_power)/lr + 2*l2';  p = (clip(linear, -l1, l1) - linear)/q;  n = n'
    Three things to know:
      * With g == 0 the formula does not leave p alone: the weight is a function of (linear, n), and a never-trained weight
        with a zero gradient becomes exactly 0.  The dense path follows the formula literally.  The row-sparse path updates
        the looked-up rows only (`_RowSparseOptimizer`): a deviation from Keras' dense semantics, as Adam's lazy rows are.
      * q == 0 (n' == 0: initial_accumulator_value = 0, g = 0, l2 = beta = 0 — the zero pads of a fused plan's flat
        group) writes p = 0 where Keras writes NaN.
      * learning_rate_power == -0.5, the default, takes sqrtf; any other power <= 0 powf."""

    _name = 'Ftrl'
    _entry = 'ftrl'
    slot_names = ('accumulator', 'linear')
    _hp = ('learning_rate', 'learning_rate_power', 'initial_accumulator_value', 'l1_regularization_strength',
           'l2_regularization_strength', 'l2_shrinkage_regularization_strength', 'beta')

    def __init__(self, params, embedding_layers=(), learning_rate=1e-3, learning_rate_power=-0.5,
                 initial_accumulator_value=0.1, l1_regularization_strength=0.0, l2_regularization_strength=0.0,
                 l2_shrinkage_regularization_strength=0.0, beta=0.0, clipnorm=None, clipvalue=None, global_clipnorm=None,
                 weight_decay=None, use_ema=False, ema_momentum=0.99, ema_overwrite_frequency=None):
        hp = dict(zip(self._hp, (learning_rate, learning_rate_power, initial_accumulator_value, l1_regularization_strength,
                                 l2_regularization_strength, l2_shrinkage_regularization_strength, beta)))
        self._check(**hp)
        super().__init__(params, embedding_layers, clipnorm, clipvalue, global_clipnorm, weight_decay, use_ema, ema_momentum,
                         ema_overwrite_frequency)
        for k, v in hp.items():
            setattr(self, k, float(v))

    @staticmethod
    def _check(**hp):
        if hp['initial_accumulator_value'] < 0:
            raise ValueError(f"`initial_accumulator_value` needs to be positive or zero, got {hp['initial_accumulator_value']!r}")
        if hp['learning_rate_power'] > 0:
            raise ValueError(f"`learning_rate_power` needs to be negative or zero, got {hp['learning_rate_power']!r}")
        for k in ('l1_regularization_strength', 'l2_regularization_strength', 'l2_shrinkage_regularization_strength', 'beta'):
            if hp[k] < 0:
                raise ValueError(f'`{k}` needs to be positive or zero, got {hp[k]!r}')

    @property
    def slot_init(self):
        return self.initial_accumulator_value, 0.0

    def _hpargs(self):
        l2 = self.l2_regularization_strength + self.beta / (2.0 * self.learning_rate)
        return (self.learning_rate, self.learning_rate_power, self.l1_regularization_strength, l2,
                self.l2_shrinkage_regularization_strength)


OPTIMIZERS = {'adam': KerasAdam, 'sgd': SGD, 'adagrad': Adagrad, 'rmsprop': RMSprop, 'ftrl': Ftrl, 'adamax': Adamax}


def _config_keys(cls):
    """the hyperparameters `cls` takes by name: its constructor's arguments behind (params, embedding_layers)"""
    import inspect
    return [k for k in inspect.signature(cls.__init__).parameters if k not in ('self', 'params', 'embedding_layers')]


def make_optimizer(spec, params, embedding_layers):
    """spec: 'auto' / None (Adam), a name of OPTIMIZERS in any letter case (Keras' defaults), Keras' serialised form
    {'class_name': 'Ftrl', 'config': {'l1_regularization_strength': 1e-4}} for any of them (an unknown key of `config`
    raises), or a callable (params, embedding_layers) -> optimizer."""
    if spec == 'auto' or spec is None:
        return KerasAdam(params, embedding_layers)
    if isinstance(spec, str) and spec.lower() in OPTIMIZERS:
        return OPTIMIZERS[spec.lower()](params, embedding_layers)
    if isinstance(spec, dict) and isinstance(spec.get('class_name'), str) and spec['class_name'].lower() in OPTIMIZERS:
        cls, config = OPTIMIZERS[spec['class_name'].lower()], dict(spec.get('config') or {})
        unknown = sorted(set(config) - set(_config_keys(cls)))
        if unknown:
            raise ValueError(f"optimizer {spec['class_name']!r}: unknown config keys {unknown} (accepted: {_config_keys(cls)})")
        return cls(params, embedding_layers, **config)
    if callable(spec):
        return spec(params, embedding_layers)
    raise ValueError(f"Unsupported optimizer: {spec!r} (accepted: 'auto', {', '.join(repr(k) for k in OPTIMIZERS)}, "
                     f"{{'class_name': <one of these names>, 'config': {{...}}}}, or a callable (params, embedding_layers) "
                     f'-> optimizer)')


def flatten_dense_parameters(model, optimizer, exclude=()):
    """Re-home every trainable dense parameter of `model` in ONE flat buffer (and its gradient in another), so that
    backward kernels accumulate in place (ops._grad_target), a data-parallel exchange is one all-reduce of the flat
    gradient and the optimizer is one launch.  `exclude`: parameters that stay on their own (embedding tables).
    Returns (flat_param, flat_grad) or None when the optimizer has no flat-group support."""
    if not hasattr(optimizer, 'register_flat_group'):
        return None
    skip = {id(p) for p in exclude}
    members, off = [], 0
    params = [p for p in model.parameters() if p.requires_grad and id(p) not in skip and p.dtype == torch.float32]
    if not params:
        return None
    for p in params:
        members.append((p, off, p.numel()))
        off += (p.numel() + 63) // 64 * 64            # 256-byte aligned starts (float4 / MFMA operand loads)
    device = params[0].device
    flat_param = torch.zeros(off, dtype=torch.float32, device=device)
    flat_grad = torch.zeros(off, dtype=torch.float32, device=device)
    with torch.no_grad():
        for p, o, n in members:
            flat_param[o:o + n].copy_(p.data.reshape(-1))
            p.data = flat_param[o:o + n].view(p.shape)
    optimizer.register_flat_group(flat_param, flat_grad, members, off, grad_views=True)
    return flat_param, flat_grad


class History:
    def __init__(self):
        self.history = {}
        self.epoch = []

    def add(self, epoch, logs):
        self.epoch.append(epoch)
        for k, v in logs.items():
            self.history.setdefault(k, []).append(v)


# ---------------------------------------------------------------------------------------------
# data feed (replaces utils/dataset_generator.py:36-72 for in-memory frames)
# ---------------------------------------------------------------------------------------------
def host_targets(y, task=None, num_classes=None, sample_weight=None):
    """y as a feed carries it, on the host: float32, one-hot for integer multiclass labels, the per-row weights as the LAST
    column -> (tensor or None, y's own rank without the weight column)"""
    if y is None:
        return None, None
    y = np.asarray(y)
    if task == consts.TASK_MULTICLASS and y.ndim == 1:
        y = np.eye(num_classes, dtype=np.float32)[y.astype(np.int64)]
    y_host = torch.as_tensor(np.ascontiguousarray(y, dtype=np.float32))
    y_ndim = y_host.dim()                      # weights ride as an extra column: remember y's own rank
    if sample_weight is not None:
        w = torch.as_tensor(np.ascontiguousarray(np.asarray(sample_weight).reshape(-1), dtype=np.float32))
        if w.shape[0] != y_host.shape[0]:
            raise ValueError(f'sample_weight has {w.shape[0]} entries for {y_host.shape[0]} rows')
        y_host = torch.cat([y_host.reshape(y_host.shape[0], -1), w[:, None]], 1).contiguous()
    return y_host, y_ndim


class TableBatches:
    """Input feed for in-memory frames (replaces `to_dataset`, utils/dataset_generator.py:36-72, which
    converts whole frames through `.tolist()` into tf.constants and feeds float32 ids).

    Ids are int32 end to end.  Two modes, same batches for the same seed:
      * resident (default when the table fits `max_resident_bytes`): the whole table lives in HBM, a shuffled epoch
        is one `randperm` on the device and every batch an index-select — no host work per step;
      * streamed: the table stays in PINNED host memory; batch k+1 is gathered on the host into a ring of pinned
        staging buffers and copied with an async H2D on a side stream while batch k trains; the compute stream
        waits on the copy's event only.
    Yields ([cat ids [B,F] int32, var-len id blocks..., dense blocks...], y)."""

    def __init__(self, X, y, categorical_columns, continuous_columns, device, task=None, num_classes=None,
                 cat_dtype=torch.int32, var_len_categorical_columns=None, resident=None,
                 max_resident_bytes=32 << 30, ring=3, sample_weight=None):
        self.n = len(X)
        self.weighted = sample_weight is not None      # per-row loss weights ride as the LAST column of y
        self.y_ndim = None
        self.device = torch.device(device)
        get = (lambda cols: X[cols].values) if hasattr(X, 'columns') else None
        host = []          # [(kind, host tensor)] in model input order: cat, var-len..., dense... (deepmodel.py:310)
        if categorical_columns:
            names = [c.name for c in categorical_columns]
            arr = get(names) if get else np.asarray(X['cat'])
            host.append(('cat', torch.as_tensor(np.ascontiguousarray(arr).astype(np.int64)).to(cat_dtype)))
        for c in var_len_categorical_columns or []:       # padded id lists, [N, max_elements_length]
            col = X[c.name]
            arr = np.array(col.tolist() if hasattr(col, 'tolist') else list(col))
            host.append(('var', torch.as_tensor(np.ascontiguousarray(arr).astype(np.int64)).to(cat_dtype)))
        for c in continuous_columns or []:
            arr = get(list(c.column_names)) if get else np.asarray(X[c.name])
            host.append(('cont', torch.as_tensor(np.ascontiguousarray(arr, dtype=np.float32))))
        y_host, self.y_ndim = host_targets(y, task, num_classes, sample_weight)
        nbytes = sum(t.numel() * t.element_size() for _, t in host) + (0 if y_host is None else y_host.numel() * 4)
        self.resident = (nbytes <= max_resident_bytes) if resident is None else bool(resident)
        self.kinds = [k for k, _ in host]
        if self.resident:
            self.blocks = [t.to(self.device) for _, t in host]
            self.y = None if y_host is None else y_host.to(self.device)
        else:
            pin = self.device.type == 'cuda'
            self.blocks = [t.pin_memory() if pin else t for _, t in host]
            self.y = None if y_host is None else (y_host.pin_memory() if pin else y_host)
            self._ring = max(2, int(ring))
            self._staging = None
            self._copy_stream = torch.cuda.Stream(self.device) if pin else None

    @classmethod
    def from_device(cls, blocks, kinds, y=None, y_ndim=None, weighted=False):
        """A resident feed over tensors that already live on the device (a synthetic table generated there, bench.py):
        blocks in model input order (cat ids int32 [N,F], var-len id blocks, continuous blocks float32), kinds the matching
        'cat' / 'var' / 'cont' tags, y float32 [N] or [N, outputs] (its last column the per-row weight when `weighted`)."""
        self = cls.__new__(cls)
        self.n = int(blocks[0].shape[0])
        self.weighted = bool(weighted)
        self.device = blocks[0].device
        self.kinds = list(kinds)
        self.blocks = [b.contiguous() for b in blocks]
        self.y = None if y is None else y.contiguous()
        self.y_ndim = y_ndim if y_ndim is not None else (None if y is None else y.dim())
        self.resident = True
        return self

    # kept for callers that look at the pieces
    @property
    def cat(self):
        return self.blocks[self.kinds.index('cat')] if 'cat' in self.kinds else None

    @property
    def var_lens(self):
        return [b for k, b in zip(self.kinds, self.blocks) if k == 'var']

    @property
    def conts(self):
        return [b for k, b in zip(self.kinds, self.blocks) if k == 'cont']

    def batch(self, sel):
        return [b[sel] for b in self.blocks], (None if self.y is None else self.y[sel])

    def _permutation(self, generator):
        """The same permutation in both modes: drawn on the device when there is one."""
        if self.device.type == 'cuda':
            return torch.randperm(self.n, device=self.device, generator=generator)
        return torch.randperm(self.n, generator=generator)

    def iterate(self, batch_size, shuffle, drop_remainder, generator=None):
        n = self.n
        stop = (n // batch_size) * batch_size if drop_remainder else n
        perm = self._permutation(generator) if shuffle else None
        if self.resident:
            for s in range(0, stop, batch_size):
                e = min(s + batch_size, n)
                yield self.batch(perm[s:e] if shuffle else slice(s, e))
            return
        yield from self._stream(batch_size, stop, None if perm is None else perm.cpu())

    # -- streamed mode ---------------------------------------------------------------------------------
    def _alloc_staging(self, batch_size):
        pin = self._copy_stream is not None
        srcs = self.blocks + ([] if self.y is None else [self.y])
        self._staging = []
        for _ in range(self._ring):
            hostbufs = [torch.empty((batch_size,) + tuple(t.shape[1:]), dtype=t.dtype, pin_memory=pin) for t in srcs]
            devbufs = [torch.empty_like(h, device=self.device) for h in hostbufs]
            ev = torch.cuda.Event() if pin else None
            self._staging.append((hostbufs, devbufs, ev, [None]))
        self._staging_batch = batch_size

    def _stage(self, slot, s, e, perm_host):
        """host gather into the slot's pinned buffers + async H2D on the copy stream; records the slot's event"""
        hostbufs, devbufs, ev, consumed = self._staging[slot]
        srcs = self.blocks + ([] if self.y is None else [self.y])
        k = e - s
        if consumed[0] is not None:
            consumed[0].synchronize()         # the step that used this slot's device buffers must be done
        for src, hb in zip(srcs, hostbufs):
            if perm_host is None:
                hb[:k].copy_(src[s:e])
            else:
                torch.index_select(src, 0, perm_host[s:e], out=hb[:k])
        if self._copy_stream is not None:
            with torch.cuda.stream(self._copy_stream):
                for hb, db in zip(hostbufs, devbufs):
                    db[:k].copy_(hb[:k], non_blocking=True)
                ev.record(self._copy_stream)
        else:
            for hb, db in zip(hostbufs, devbufs):
                db[:k].copy_(hb[:k])
        return k

    def _stream(self, batch_size, stop, perm_host):
        if self._staging is None or self._staging_batch != batch_size:
            self._alloc_staging(batch_size)
        starts = list(range(0, stop, batch_size))
        sizes = {}
        depth = self._ring - 1
        for j in range(min(depth, len(starts))):                       # prime the ring
            sizes[j] = self._stage(j % self._ring, starts[j], min(starts[j] + batch_size, self.n), perm_host)
        for i, s in enumerate(starts):
            slot = i % self._ring
            hostbufs, devbufs, ev, consumed = self._staging[slot]
            if ev is not None:
                torch.cuda.current_stream(self.device).wait_event(ev)  # compute waits for this batch's copy only
            k = sizes.pop(i)
            outs = [d[:k] for d in devbufs]
            nxt = i + depth
            if nxt < len(starts):                                      # overlap: stage a later batch now
                sizes[nxt] = self._stage(nxt % self._ring, starts[nxt], min(starts[nxt] + batch_size, self.n),
                                         perm_host)
            yb = outs.pop() if self.y is not None else None
            try:
                yield outs, yb
            finally:
                # mark where the consumer finished with the slot — also when it stops at this batch and closes the
                # generator (fit breaks out at steps_per_epoch): the next iterate() must not restage the slot against a
                # stale event while this step's kernels may still read the device buffers
                if ev is not None:
                    done = torch.cuda.Event()
                    done.record(torch.cuda.current_stream(self.device))
                    consumed[0] = done
