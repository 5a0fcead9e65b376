# -*- coding:utf-8 -*-
"""What csrc/metrics.hip computes, restated in numpy and Python integers: the order-preserving key of a float32 score, the
stable sort, the five words of dt_metric_auc and the float64 sums of dt_metric_sums.  The GPU tests hold the kernels to these
exactly (integers) or to the rounding bound of a float64 sum; tests/test_metrics_host.py holds THIS module to a brute-force
pair count and to sklearn.metrics.roc_auc_score."""
import math

import numpy as np


def score_keys(score):
    """uint32 keys whose unsigned order is the order of the float32 scores: -0.0 becomes +0.0 (they tie), then the bits of a
    negative float are all flipped and a non-negative one gets its sign bit set"""
    b = np.ascontiguousarray(score, dtype=np.float32).view(np.uint32).copy()
    b[b == np.uint32(0x80000000)] = 0
    neg = (b & np.uint32(0x80000000)) != 0
    return np.where(neg, ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def stable_sort_pairs(keys, vals):
    order = np.argsort(np.asarray(keys, dtype=np.uint32), kind='stable')
    return np.asarray(keys)[order], np.asarray(vals)[order]


def auc_words(score, label):
    """(U2, P, N, nonfinite, bad_label) as Python integers: U2 = sum over groups of equal key of
    pos_g * (2 * negatives in lower groups + neg_g); a label other than 1 counts as a negative"""
    score = np.ascontiguousarray(score, dtype=np.float32).reshape(-1)
    label = np.ascontiguousarray(label, dtype=np.float32).reshape(-1)
    n = score.shape[0]
    keys = score_keys(score)
    pos = (label == 1.0)
    nonfinite = int((~np.isfinite(score)).sum())
    bad = int((~pos & ~(label == 0.0)).sum())
    P = int(pos.sum())
    if n == 0:
        return 0, 0, 0, 0, 0
    k, v = stable_sort_pairs(keys, pos.astype(np.uint32))
    start = np.flatnonzero(np.concatenate(([True], k[1:] != k[:-1])))
    negs_before = np.concatenate(([0], np.cumsum(v == 0, dtype=np.int64)))
    end = np.concatenate((start[1:], [n]))
    u2 = 0
    for s, e in zip(start.tolist(), end.tolist()):
        nb = int(negs_before[s])
        neg_g = int(negs_before[e]) - nb
        u2 += ((e - s) - neg_g) * (2 * nb + neg_g)
    return u2, P, n - P, nonfinite, bad


def auc_words_fast(score, label):
    """auc_words with the group loop vectorised (object-free int64 is enough below 2^31 rows: U2 < 2^61); used at the
    large sizes, and checked against auc_words in the host tests"""
    score = np.ascontiguousarray(score, dtype=np.float32).reshape(-1)
    label = np.ascontiguousarray(label, dtype=np.float32).reshape(-1)
    n = score.shape[0]
    if n == 0:
        return 0, 0, 0, 0, 0
    pos = (label == 1.0)
    k, v = stable_sort_pairs(score_keys(score), pos.astype(np.uint32))
    start = np.flatnonzero(np.concatenate(([True], k[1:] != k[:-1])))
    negs_before = np.concatenate(([0], np.cumsum(v == 0, dtype=np.int64)))
    end = np.concatenate((start[1:], [n]))
    nb = negs_before[start]
    neg_g = negs_before[end] - nb
    u2 = int(np.sum(((end - start) - neg_g) * (2 * nb + neg_g), dtype=np.int64))
    P = int(pos.sum())
    return u2, P, n - P, int((~np.isfinite(score)).sum()), int((~pos & ~(label == 0.0)).sum())


def auc(score, label):
    """exact ROC AUC = U2 / (2 P N); nan with one class only or a NaN / Inf score (where roc_auc_score raises)"""
    u2, P, N, nonfinite, _ = auc_words_fast(score, label)
    if P == 0 or N == 0 or nonfinite:
        return float('nan')
    return u2 / (2 * P * N)


def brute_force_u2(score, label):
    """twice the number of (positive, negative) pairs the positive wins, a tie counting one half: O(n^2), float compares"""
    score = np.asarray(score, dtype=np.float32)
    pos = score[np.asarray(label) == 1.0]
    neg = score[np.asarray(label) != 1.0]
    u2 = 0
    for p in pos.tolist():
        u2 += 2 * int((neg < p).sum()) + int((neg == p).sum())
    return u2


def sums(y_true, y_prob):
    """(hits, sum (p - y)^2, sum |p - y|): differences and squares in float64 from the float32 inputs, the sums exact
    (math.fsum) and rounded once"""
    y = np.ascontiguousarray(y_true, dtype=np.float32).reshape(-1)
    p = np.ascontiguousarray(y_prob, dtype=np.float32).reshape(-1)
    hits = int(((p > np.float32(0.5)).astype(np.int64) == y.astype(np.int64)).sum())
    d = p.astype(np.float64) - y.astype(np.float64)
    return hits, math.fsum((d * d).tolist()), math.fsum(np.abs(d).tolist())


def sum_bound(n):
    """relative bound between the device's float64 sum of n non-negative terms and sums(): n correctly rounded additions in
    any order, each term computed in float64 from float32 inputs"""
    return (n + 4) * 2.0 ** -53


def argmax_hits(y_prob, y_true):
    y_prob, y_true = np.asarray(y_prob), np.asarray(y_true)
    yt = y_true.argmax(-1) if y_true.ndim == 2 else y_true
    return int((y_prob.argmax(-1) == yt).sum())
