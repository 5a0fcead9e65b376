# -*- coding:utf-8 -*-
"""CPU: every class bar of tests/precision.py tells its class from the one below it, at the contraction lengths the GPU
tests run (the tower's 64 / 128 and padded CP = 448, CIN's F0 Hk from 16 to 1664, AutoInt's D = 32): the numpy emulation of
a class (tests/test_split_bf16_arithmetic.py's exact bf16 rounding and splits) passes its own bar and fails the bar of the
class above it."""
import numpy as np
import pytest
import torch

from tests import precision as P
from tests.test_split_bf16_arithmetic import split

KS = [16, 32, 64, 128, 448, 676, 1664]


def _emulate(K, seed=0, n=512, m=64):
    """{class emulation: cond_rms} for one [n, K] x [K, m] product with fp32 accumulation"""
    rng = np.random.RandomState(seed + K)
    a = rng.randn(n, K).astype(np.float32)
    b = (rng.randn(K, m) / np.sqrt(K)).astype(np.float32)
    exact = a.astype(np.float64) @ b.astype(np.float64)
    scale = np.abs(a).astype(np.float64) @ np.abs(b).astype(np.float64)

    def kept(parts, order):
        ap, _ = split(a, parts)
        bp, _ = split(b, parts)
        acc = np.zeros((n, m), np.float32)
        for p in range(parts):
            for q in range(parts):
                if p + q <= order:
                    acc = (acc + ap[p] @ bp[q]).astype(np.float32)
        return acc
    out = {'fp32': a @ b, 'six': kept(3, 2), 'three': kept(2, 1), 'one': kept(1, 0)}
    return {k: P.cond_rms(torch.from_numpy(v), torch.from_numpy(exact), torch.from_numpy(scale)) for k, v in out.items()}


@pytest.mark.parametrize('K', KS)
def test_each_bar_accepts_its_class_and_rejects_the_next_one_down(K):
    e = _emulate(K)
    assert e['fp32'] <= P.COND_BAR['fp32'] and e['six'] <= P.COND_BAR['fp32'], e
    assert e['three'] > P.COND_BAR['fp32'], e                  # a 16-bit forward fails the fp32 class
    assert e['three'] <= P.COND_BAR['b17'], e
    assert e['one'] > P.COND_BAR['b17'], e                     # an 8-bit backward fails the 16-bit class
    assert e['one'] <= P.COND_BAR['bf16'], e


@pytest.mark.parametrize('K', KS)
def test_the_bars_keep_a_margin_on_both_sides(K):
    """a bar sits above its own class and below the next class down, with room on both sides (the separations the
    comments of precision.py quote)"""
    e = _emulate(K, seed=1)
    assert P.COND_BAR['fp32'] >= 4 * max(e['fp32'], e['six']), e
    assert P.COND_BAR['b17'] >= 4 * e['three'] and e['one'] >= 8 * P.COND_BAR['b17'], e
    assert P.COND_BAR['bf16'] >= 4 * e['one'], e
    assert e['three'] >= 1.4 * P.COND_BAR['fp32'] and P.COND_BAR['fp32'] >= 4 * e['six'], e


def test_cond_scale_of_a_product_is_the_sum_of_absolute_terms():
    a = torch.tensor([[1.0, -2.0]], dtype=torch.float64)
    b = torch.tensor([[3.0], [4.0]], dtype=torch.float64)
    s, (sa, sb) = P.abs_scale(lambda x, y: x @ y, (a, b), torch.tensor([[-1.0]], dtype=torch.float64))
    assert s.item() == 11.0 and sa.tolist() == [[3.0, 4.0]] and sb.tolist() == [[1.0], [2.0]]


def test_row_rel_sees_an_error_confined_to_a_small_row():
    ref = torch.tensor([[100.0, -50.0], [1e-3, 2e-3]], dtype=torch.float64)
    got = ref.clone()
    got[1, 1] += 1e-7                                             # 5e-5 of its own row, 1e-9 of the tensor's max
    assert P.max_rel(got, ref) < 1e-8 and P.l2_rel(got, ref) < 1e-8
    assert abs(P.row_rel(got, ref) - 5e-5) < 1e-9


def test_every_claim_names_a_class_with_bars():
    for (kernel, mode), (fwd, bwd) in P.CLAIMS.items():
        assert fwd in P.COND_BAR and bwd in P.COND_BAR and fwd in P.STEP_BAR and bwd in P.STEP_BAR, (kernel, mode)
    # a kernel's backward never claims more than its forward: the forward's relu decisions bound what the backward can show
    order = ['bf16', 'b17', 'fp32']
    assert all(order.index(b) <= order.index(f) for f, b in P.CLAIMS.values())
