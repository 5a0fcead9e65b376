# -*- coding:utf-8 -*-
"""What the dt_score_* entry points of csrc/metrics.hip compute, restated in numpy and Python integers: Keras 3's log loss,
precision / recall, top-k accuracy, MSLE and MAPE, and sklearn's average precision.  Everything in float64 from the float32
inputs, logarithms by math.log, sums by math.fsum (exact, rounded once), counts as integers.  Sums over the classes of a row
restate the kernel's order.  The GPU tests hold the kernels to these: integers exactly, float64 sums within the bounds
derived at the end of this module; tests/test_scores_host.py holds THIS module to sklearn."""
import math

import numpy as np

from tests import metrics_reference as R

LO = float(np.float32(1e-7))                           # Keras' epsilon in float32
HI = float(np.float32(1) - np.float32(1e-7))           # 1 - epsilon, subtracted in float32: 0.99999988079...
U = 2.0 ** -53                                         # one correctly rounded float64 operation, relative
LOG_ULP_DEVICE = 1      # HIP's double-precision log: 1 ulp in the accuracy table of the HIP math API documentation as published
#                         (a ROCm install carries no copy of it to read the figure from; it is OCML's own as well)
LOG_ULP_HOST = 1        # math.log = the C library's log


def _log(a):
    """math.log over an array; every argument here is positive, +Inf or NaN"""
    a = np.asarray(a, dtype=np.float64)
    return np.array([math.log(v) for v in a.reshape(-1).tolist()], dtype=np.float64).reshape(a.shape)


def _fsum(a):
    a = np.asarray(a, dtype=np.float64).reshape(-1)
    return math.fsum(a.tolist()) if np.isfinite(a).all() else float(a.sum())


def clip(x):
    """numpy.clip(x, LO, HI): a NaN stays a NaN"""
    return np.clip(np.asarray(x, dtype=np.float64), LO, HI)


def label_classes(y, C):
    """the class a float label names ((int) label when 0 <= label < C), -1 where it names none (a NaN too)"""
    y = np.asarray(y, dtype=np.float32).reshape(-1)
    with np.errstate(invalid='ignore'):
        ok = (y >= 0) & (y.astype(np.float64) < C)
    return np.where(ok, np.where(ok, y, 0).astype(np.int64), -1)


def first_max(t):
    """the class a `v > best` scan from class 0 ends on, per row"""
    t = np.asarray(t, dtype=np.float32)
    idx = np.zeros(t.shape[0], dtype=np.int64)
    for r in range(t.shape[0]):
        best = t[r, 0]
        for c in range(1, t.shape[1]):
            if t[r, c] > best:
                best, idx[r] = t[r, c], c
    return idx


def first_max_fast(t):
    t = np.asarray(t, dtype=np.float32)
    best, idx = t[:, 0].copy(), np.zeros(t.shape[0], dtype=np.int64)
    for c in range(1, t.shape[1]):
        m = t[:, c] > best
        best, idx = np.where(m, t[:, c], best), np.where(m, c, idx)
    return idx


# ---- the element-wise pass -------------------------------------------------------------------------------------------------
def expand_labels(y_true, C):
    """[n] labels -> [n, C] one-hot float32; a label naming no class gives a row of zeros"""
    return (label_classes(y_true, C)[:, None] == np.arange(C)[None, :]).astype(np.float32)


def binary_words(y_true, y_prob):
    """(TP, FP, FN, TN, sum of -(y log q + (1 - y) log(1 - q))) over all elements; y_true with y_prob's size, or [n] labels
    against [n, C] (expanded)"""
    p = np.asarray(y_prob, dtype=np.float32)
    y = np.asarray(y_true, dtype=np.float32)
    if y.size != p.size:
        y = expand_labels(y, p.shape[1])
    y, p = y.reshape(-1), p.reshape(-1)
    pp, yp = p > np.float32(0.5), y != 0
    counts = (int((pp & yp).sum()), int((pp & ~yp).sum()), int((~pp & yp).sum()), int((~pp & ~yp).sum()))
    y64, q = y.astype(np.float64), clip(p)
    with np.errstate(all='ignore'):
        term = -(y64 * _log(q) + (1.0 - y64) * _log(1.0 - q))
    return counts + (_fsum(term),)


def ratio(num, den):
    return num / den if den else 0.0


# ---- the regression pass ---------------------------------------------------------------------------------------------------
def regression_sums(y_true, y_pred):
    """(sum (log(max(p, LO) + 1) - log(max(y, LO) + 1))^2, sum |y - p| / max(|y|, LO), K) with K = sum (|a| + |b|) |a - b|
    over the two logarithms a, b of every MSLE term: the cancellation weight of msle_bound"""
    y = np.asarray(y_true, dtype=np.float32).astype(np.float64).reshape(-1)
    p = np.asarray(y_pred, dtype=np.float32).astype(np.float64).reshape(-1)
    with np.errstate(all='ignore'):
        a, b = _log(np.maximum(p, LO) + 1.0), _log(np.maximum(y, LO) + 1.0)
        d = a - b
        return _fsum(d * d), _fsum(np.abs(y - p) / np.maximum(np.abs(y), LO)), _fsum((np.abs(a) + np.abs(b)) * np.abs(d))


# ---- the row pass ----------------------------------------------------------------------------------------------------------
def row_sum(x, thread_row_max_c):
    """sum over the classes of every row of x [n, C] (float64) in the kernel's order: class order up to thread_row_max_c
    classes; beyond, lane l of 64 adds classes l, l + 64, ... in that order, then partial[l] += partial[l + o] for o = 32 ... 1"""
    n, C = x.shape
    if C <= thread_row_max_c:
        s = np.zeros(n)
        for c in range(C):
            s = s + x[:, c]
        return s
    J = (C + 63) // 64
    xp = np.zeros((n, J * 64))
    xp[:, :C] = x                                       # (adding 0.0 changes no sum)
    part = np.zeros((n, 64))
    for j in range(J):
        part = part + xp[:, 64 * j:64 * (j + 1)]
    o = 32
    while o:
        part[:, :o] = part[:, :o] + part[:, o:2 * o]
        o //= 2
    return part[:, 0].copy()


def categorical_words(y_prob, y_true, k, thread_row_max_c):
    """(rows whose target class has fewer than k classes scoring above it, sum over rows of the categorical cross-entropy);
    y_true [n, C] (target: first_max of the row) or [n] labels"""
    p32 = np.asarray(y_prob, dtype=np.float32)
    y = np.asarray(y_true, dtype=np.float32)
    n, C = p32.shape
    onehot = y.shape == p32.shape
    target = first_max_fast(y) if onehot else label_classes(y, C)
    rows, valid = np.arange(n), target >= 0
    with np.errstate(all='ignore'):
        pt = p32[rows, np.maximum(target, 0)]
        above = (p32 > pt[:, None]).sum(1)
        hits = int((valid & (pt == pt) & (above < k)).sum())
        p = p32.astype(np.float64)
        s = row_sum(p, thread_row_max_c)
        q = clip(p / s[:, None])
        if onehot:
            y64 = y.astype(np.float64)
            need = (y64 != 0) | (q != q)                # elsewhere the product is an exact zero
            terms = np.zeros((n, C))
            terms[need] = y64[need] * _log(q[need])
            loss = -row_sum(terms, thread_row_max_c)
        else:
            loss = np.full(n, np.nan)
            loss[valid] = -_log(q[rows[valid], target[valid]])
    return hits, _fsum(loss)


def top_k_brute_force(y_prob, target, k):
    """rows whose target is inside the k best when classes tied with it are all let in: sort the row, take the k-th best
    score, a hit scores at least that (and is not a NaN)"""
    hits = 0
    for row, t in zip(np.asarray(y_prob, dtype=np.float32).tolist(), target):
        if t < 0 or row[t] != row[t]:
            continue
        finite = sorted((v for v in row if v == v), reverse=True)
        hits += len(finite) <= k or row[t] >= finite[k - 1]
    return hits


# ---- ranking ---------------------------------------------------------------------------------------------------------------
def ranking_words(score, label):
    """(U2, P, N, nonfinite, bad_label, sum over groups of pos_g * TPcum_g / (n - start_g), number of groups): the groups of
    equal key in ascending order, the terms float(pos_g) * float(TPcum_g) / float(n - start_g) in float64"""
    score = np.ascontiguousarray(score, dtype=np.float32).reshape(-1)
    label = np.ascontiguousarray(label, dtype=np.float32).reshape(-1)
    n = score.shape[0]
    words = R.auc_words_fast(score, label)
    pos = (label == 1.0)
    k, v = R.stable_sort_pairs(R.score_keys(score), pos.astype(np.uint32))
    start = np.flatnonzero(np.concatenate(([True], k[1:] != k[:-1])))
    negs_before = np.concatenate(([0], np.cumsum(v == 0, dtype=np.int64)))
    end = np.concatenate((start[1:], [n]))
    nb = negs_before[start]
    pos_g = (end - start) - (negs_before[end] - nb)
    tp_cum = words[1] - (start - nb)
    terms = pos_g.astype(np.float64) * tp_cum.astype(np.float64) / (n - start).astype(np.float64)
    return words + (math.fsum(terms[pos_g > 0].tolist()), int(start.shape[0]))


def average_precision(score, label):
    u2, P, N, nonfinite, bad, total, _ = ranking_words(score, label)
    return float('nan') if P == 0 or nonfinite else total / P


# ---- bounds ----------------------------------------------------------------------------------------------------------------
# A float64 sum of T non-negative terms added in any order differs from their exact sum by at most (T - 1) U relative, and fsum
# rounds once: T U.  A term that costs e correctly rounded operations on each side adds e U per side; the constant 4 of
# (T + 4 + e) U (metrics_reference.sum_bound's) takes the reference's side for every e used below, as the lines show.  One
# ulp of a logarithm is 2 U.
def sum_bound(T, e):
    return (T + 4 + e) * U


# dt_score_binary's sum: two logarithms and two multiplications per term.  Device side: each product carries its logarithm's
# 2 LOG_ULP_DEVICE U and its own U, their sum one more U (1 - y and 1 - q are exact for float32 y in [0, 1] and q in
# [LO, HI]); the reference's side 2 LOG_ULP_HOST U + 2 U; together 8 U <= (4 + E_BCE) U.
E_BCE = 2 * (LOG_ULP_DEVICE + LOG_ULP_HOST) + 2
# dt_score_categorical's sum: s is the same float64 on both sides (the same additions in the same order) and so is q, a
# correctly rounded quotient; one logarithm and (one-hot) one multiplication per row: 3 U a side.  The inner sum of a
# one-hot row adds exact zeros; its C terms are counted in T all the same: T = n + C.
E_CCE = (LOG_ULP_DEVICE + LOG_ULP_HOST) + 1
# MAPE: one subtraction and one division; average precision: one multiplication and one division
E_MAPE = 2
E_AP = 2


def msle_bound(n, total, K):
    """absolute bound for the MSLE sum.  A term is d^2 with d = a - b the difference of two logarithms: the logarithms' errors
    (2 LOG_ULP_DEVICE U on the device, 2 LOG_ULP_HOST U in the reference, each relative to |a| or |b|, not to |d|) move d by
    up to 2 (LOG_ULP_DEVICE + LOG_ULP_HOST) U (|a| + |b|) and d^2 by twice that times |d|: 4 (...) U K over all terms with
    K = sum (|a| + |b|) |d|.  What is left is relative to d^2: the subtraction and the square, 3 U a side, e = 6."""
    return sum_bound(n, 6) * total + 4 * (LOG_ULP_DEVICE + LOG_ULP_HOST) * U * K
