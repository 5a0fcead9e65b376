# -*- coding:utf-8 -*-
"""Float64 numpy restatement of Keras 3's `BaseOptimizer._clip_gradients` as csrc/gradclip.hip defines it (include/dt_hip.h):
what tests/test_gradclip_host.py pins on hand-computed cases and tests/test_gradclip_gpu.py compares the kernels against.

A variable is one Keras variable: a dense tensor, or one column's row range of a packed table.  A table's gradient is its
DENSE gradient: duplicate lookups of a row summed, rows not looked up 0 (every formula maps 0 to 0).  Nothing here rounds to
float32 except the constant c, which the library takes as a float: the bars of the GPU tests count the kernels' own roundings."""
import numpy as np

MODES = ('clipvalue', 'clipnorm', 'global_clipnorm')


def c32(c):
    """the constant as the kernels receive it"""
    return float(np.float32(c))


def coalesce(rows, values):
    """(rows int64 [n], -1 = skipped; values [n, D]) -> (out_rows [n]: the distinct rows ascending, then -1; out_vals [n, D]
    float64: each distinct row's summed gradient, the tail 0)"""
    rows = np.asarray(rows, dtype=np.int64).reshape(-1)
    values = np.asarray(values, dtype=np.float64).reshape(rows.size, -1)
    valid = rows >= 0
    uniq, inverse = np.unique(rows[valid], return_inverse=True)
    out_rows = np.full(rows.size, -1, dtype=np.int64)
    out_rows[:uniq.size] = uniq
    out_vals = np.zeros_like(values)
    np.add.at(out_vals, inverse, values[valid])
    return out_rows, out_vals


def sumsq(g):
    return float(np.sum(np.square(np.asarray(g, dtype=np.float64))))


def field_sumsq(out_rows, out_vals, row_offset, V):
    """one sum of squares per field of a coalesced table; field f owns the rows [row_offset[f], row_offset[f + 1]), the last
    one up to V"""
    edges = list(row_offset) + [V]
    out_rows, out_vals = np.asarray(out_rows), np.asarray(out_vals, dtype=np.float64)
    return [sumsq(out_vals[(out_rows >= lo) & (out_rows < hi)]) for lo, hi in zip(edges[:-1], edges[1:])]


def field_of(rows, row_offset):
    """index of the field each row id (>= 0) belongs to"""
    return np.searchsorted(np.asarray(row_offset), np.asarray(rows), side='right') - 1


def clip_value(g, c):
    g, c = np.asarray(g, dtype=np.float64), c32(c)
    return np.where(g < -c, -c, np.where(g > c, c, g))            # NaN stays NaN


def clip_norm(g, S, c):
    """g of a variable whose sum of squares is S (an array: per element); S = 0 leaves g as it is"""
    g, c = np.asarray(g, dtype=np.float64), c32(c)
    with np.errstate(invalid='ignore'):
        return g * c / np.maximum(np.sqrt(np.asarray(S, dtype=np.float64)), c)


def global_scale(S_all, c):
    """S_all: every variable's sum of squares -> (N, s): g <- g * s.  A non-finite N makes s NaN, as Keras does"""
    c = c32(c)
    N = float(np.sqrt(np.sum(np.asarray(S_all, dtype=np.float64))))
    with np.errstate(divide='ignore', invalid='ignore'):
        s = c * np.minimum(np.float64(1.0) / N, 1.0 / c) + (N - N)
    return N, float(s)


def clip_variables(mode, c, variables):
    """variables: list of float arrays, one per variable -> the clipped list (float64)"""
    S = [sumsq(v) for v in variables]
    if mode == 'clipvalue':
        return [clip_value(v, c) for v in variables]
    if mode == 'clipnorm':
        return [clip_norm(v, s, c) for v, s in zip(variables, S)]
    _, s = global_scale(S, c)
    with np.errstate(invalid='ignore'):
        return [np.asarray(v, dtype=np.float64) * s for v in variables]
