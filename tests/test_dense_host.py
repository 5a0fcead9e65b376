# -*- coding:utf-8 -*-
"""CPU: the LDS-slab Dense entry points (csrc/dense.hip) — the geometry every named case of tests/dense_support.py is there
to reach, the shape predicate at its three LDS limits, the workspace size, the argument validation, and grad_W's row
ownership over the batch split.  No launch happens here."""
import ctypes

import pytest
import torch

from tests.dense_support import (D1, D1_BWD, D1_FWD, FWD, GRAD_W, GRAD_X, LDS_LIMIT, LIMITS, MFMA, WGRAD, cdiv, geometry,
                                 wgrad_rows)


def _lib():
    from deeptables_amd import _lib
    return _lib


def test_geometry_of_the_named_cases():
    """every case has the geometry tests/dense_support.py claims, and dt_dense_supported takes it"""
    h = _lib().lib()
    for table in (MFMA, WGRAD):
        for name, ((N, K, M, _), fwd, gx, gw) in table.items():
            assert h.dt_dense_supported(N, K, M) == 1 and M >= 2, name
            assert (geometry(N, K, M, FWD), geometry(N, K, M, GRAD_X), geometry(N, K, M, GRAD_W)) == (fwd, gx, gw), name
    for name, ((N, K, M, _), fwd, bwd) in D1.items():
        assert h.dt_dense_supported(N, K, M) == 1 and M == 1, name
        assert (geometry(N, K, M, D1_FWD), geometry(N, K, M, D1_BWD)) == (fwd, bwd), name


def test_the_named_cases_reach_what_the_issue_lists():
    """the branch coverage the table at the top of tests/test_dense_edges_gpu.py states, from the asserted geometries"""
    launches = {}                       # (nbw, N) of every k_dense_mfma launch, forward and grad_x
    for (N, K, M, _), fwd, gx, _ in list(MFMA.values()) + list(WGRAD.values()):
        for g, Kd, Mo in ((fwd, K, M), (gx, M, K)):
            nbw, rows, grid, lds, nch, rem, vec = g
            assert rows * nbw == 128 and grid == cdiv(N, rows) and lds == rows * ((Kd + 1) | 1) * 4 <= LDS_LIMIT
            assert nch == Kd // 32 and 16 * nch + rem == (Kd + 1) // 2 and vec == (Kd % 4 == 0)
            assert nbw == {1: 1, 2: 2, 3: 2}.get(cdiv(Mo, 32), 4)
    for name, ((N, K, M, _), fwd, gx, _) in MFMA.items():
        launches.setdefault('fwd', set()).add((fwd[0], N))
        launches.setdefault('gx', set()).add((gx[0], N))
    for which in ('fwd', 'gx'):         # N at rows-per-block - 1, rows-per-block, + 1 and 1, for each block height
        for nbw in (1, 2, 4):
            rows = 128 // nbw
            got = {N for w, N in launches[which] if w == nbw}
            assert {1, rows - 1, rows, rows + 1} <= got, (which, nbw, got)
    fwd_shapes = {(K, M) for (_, K, M, _), *_ in MFMA.values()}
    assert {M for _, M in fwd_shapes} >= {2, 32, 33, 65, 96, 97, 128, 129}
    assert {K for K, _ in fwd_shapes} >= {1, 2, 3, 31, 32, 33, 64, 66, 96, 97, 128, 161}
    nch = {g[4] for _, fwd, gx, _ in MFMA.values() for g in (fwd, gx)}
    assert nch >= {0, 1, 2, 3, 4, 5} and any(n >= 5 and n % 2 == 1 for n in nch)
    both = [(K % 4 == 0, M % 4 == 0) for K, M in fwd_shapes]
    assert (True, True) in both and (False, False) in both and (True, False) in both
    # grad_W: the wave-level shapes of the row ranges the issue lists
    def waves(name):
        (N, K, M, _), _, _, (tiles, splits, rps) = WGRAD[name]
        assert tiles == cdiv(K, 32) * cdiv(M, 32)
        return splits, [max(0, e - b) for b, e in wgrad_rows(N, splits, rps).values()]
    assert waves('w_n5') == (1, [2, 2, 1, 0])                                   # an empty last wave
    assert waves('w_n128') == (1, [32] * 4)                                     # one full chunk per wave
    assert waves('w_n200') == (1, [50] * 4)                                     # a full chunk and a guarded one
    assert waves('w_n512') == (2, [64] * 8)                                     # two full chunks per wave
    assert waves('w_n513') == (2, [66] * 7 + [513 - 264 - 3 * 66])              # rounded-up split, last wave short
    assert waves('w_n1030')[0] == 4 and waves('w_n1030')[1][-1] == 1030 - 3 * 264 - 3 * 66
    assert any(K % 32 and M % 32 for (_, K, M, _), *_ in WGRAD.values())
    # Dense(1)
    assert {K for (_, K, _, _), *_ in D1.values()} >= {1, 2, 3, 4, 5, 8, 63, 64, 65, 129, 257, 1028}
    assert {N for (N, _, _, _), *_ in D1.values()} >= {1, 3, 4, 5, 16385, 32769, 65537}
    assert {bwd[1] for _, _, bwd in D1.values()} >= {1, 2, 4, 5, 61, 64, 65, 129}
    assert {bwd[0] for _, _, bwd in D1.values()} >= {32, 33, 64}
    last = {(N - (bwd[1] - 1) * bwd[0], K % 4 == 0) for (N, K, _, _), _, bwd in D1.values()}
    assert last >= {(1, True), (2, True), (3, True), (32, True)}                # the unrolled-by-4 loop's tails, 16-byte path
    assert D1['d1_n16385_k8'][1] == (4096,) and 16385 > 4 * 4096                # the forward's grid-stride loop, second trip
    assert all(K <= 8 for (N, K, _, _), *_ in D1.values() if N > 5000)


def test_the_three_lds_limits_and_their_first_refused_neighbours():
    h = _lib().lib()
    want = {'lim4': (1198, 97), 'lim2': (598, 33), 'lim1': (298, 2), 'lim4_gx': (97, 1198)}
    for name in LIMITS:
        (N, K, M, _), fwd, gx, _ = MFMA[name]
        assert (K, M) == want[name]
        assert h.dt_dense_supported(N, K, M) == 1
        big = fwd if name != 'lim4_gx' else gx
        rows = big[1]
        assert big[3] <= LDS_LIMIT < big[3] + 2 * rows * 4        # the odd row stride grows two floats at a time
        if name != 'lim4_gx':
            assert h.dt_dense_supported(N, K + 1, M) == 0, name
            assert h.dt_dense_tiled_supported(N, K + 1, M) == 1
        else:
            assert h.dt_dense_supported(N, K, M + 1) == 0
    # the limit depends on the output's column blocks: one block fewer, and the same K is refused
    assert h.dt_dense_supported(130, 1198, 96) == 0 and h.dt_dense_supported(130, 598, 32) == 0
    out = (ctypes.c_int * 8)(*([-1] * 8))
    assert h.dt_dense_geometry(130, 1199, 97, FWD, out) == -2 and list(out) == [-1] * 8
    assert b'dt_dense_geometry' in h.dt_last_error()


def test_workspace_is_the_partial_rows_or_the_transposed_kernel():
    h = _lib().lib()
    for (N, K, M, _), _, (rpb, blocks, _) in D1.values():
        assert blocks == cdiv(N, rpb)
        assert h.dt_dense_workspace_bytes(N, K, M) == 4 * blocks * (K + 4)
    for table in (MFMA, WGRAD):
        for (N, K, M, _), *_ in table.values():
            assert h.dt_dense_workspace_bytes(N, K, M) == 4 * K * M


def test_argument_validation_without_a_gpu():
    """bad sizes, a bad activation code, null pointers and a missing workspace are rejected before any launch"""
    L = _lib()
    h = L.lib()
    for N, K, M in [(-1, 4, 4), (4, 0, 4), (4, 4, 0), (4, -2, 4), (4, 4, -1), (4, 0, 1)]:
        assert h.dt_dense_fwd(None, None, None, L.DT_ACT_RELU, N, K, M, None, None) == -1, (N, K, M)
        assert b'dt_dense_fwd' in h.dt_last_error()
        assert h.dt_dense_bwd(None, None, None, None, L.DT_ACT_RELU, N, K, M, None, None, None, None, None) == -1
        assert b'dt_dense_bwd' in h.dt_last_error()
    one = torch.zeros(64)
    p = L.ptr(one)
    for M in (1, 4):
        assert h.dt_dense_fwd(p, p, None, 7, 4, 4, M, p, None) == -1                       # act
        assert b'act' in h.dt_last_error()
        assert h.dt_dense_bwd(p, p, p, p, 2, 4, 4, M, p, p, p, p, None) == -1
        assert b'act' in h.dt_last_error()
        for hole in range(3):                                                              # x, W, y
            args = [p, p, p]
            args[hole] = None
            assert h.dt_dense_fwd(args[0], args[1], None, L.DT_ACT_RELU, 4, 4, M, args[2], None) == -1, hole
            assert b'null' in h.dt_last_error()
        for hole in range(5):                                                              # x, W, y, grad_y, grad_W
            args = [p] * 5
            args[hole] = None
            assert h.dt_dense_bwd(args[0], args[1], args[2], args[3], L.DT_ACT_LINEAR, 4, 4, M, p, args[4], p, p,
                                  None) == -1, hole
            assert b'null' in h.dt_last_error()
    # the workspace: the Dense(1) backward always needs it, the MFMA one for grad_x
    assert h.dt_dense_bwd(p, p, p, p, L.DT_ACT_LINEAR, 4, 4, 1, None, p, None, None, None) == -1
    assert b'workspace' in h.dt_last_error()
    assert h.dt_dense_bwd(p, p, p, p, L.DT_ACT_LINEAR, 4, 4, 4, p, p, None, None, None) == -1
    assert b'workspace' in h.dt_last_error()
    # a slab past the LDS limit is refused, not launched
    assert h.dt_dense_fwd(p, p, None, L.DT_ACT_LINEAR, 4, 1199, 97, p, None) == -2
    assert h.dt_dense_bwd(p, p, p, p, L.DT_ACT_LINEAR, 4, 97, 1199, p, p, None, p, None) == -2
    # an empty batch is a no-op that touches no pointer
    for M in (1, 4):
        assert h.dt_dense_fwd(None, None, None, L.DT_ACT_RELU, 0, 4, M, None, None) == 0
        assert h.dt_dense_bwd(None, None, None, None, L.DT_ACT_RELU, 0, 4, M, None, None, None, None, None) == 0


def test_geometry_argument_validation():
    h = _lib().lib()
    out = (ctypes.c_int * 8)(*([-1] * 8))
    for product in (-1, 5):
        assert h.dt_dense_geometry(64, 32, 32, product, out) == -1
        assert b'dt_dense_geometry' in h.dt_last_error() and b'product' in h.dt_last_error()
    assert h.dt_dense_geometry(64, 32, 32, FWD, None) == -1
    for shape in [(0, 4, 4), (4, -3, 4), (4, 4, 0), (70, 1204, 132)]:
        assert h.dt_dense_supported(*shape) == 0
        assert h.dt_dense_geometry(*shape, FWD, out) == -2, shape
        assert 'N=%d K=%d M=%d' % shape in h.dt_last_error().decode()
    for shape, product in [((64, 32, 1), FWD), ((64, 32, 1), GRAD_W), ((64, 32, 2), D1_FWD), ((64, 32, 2), D1_BWD)]:
        assert h.dt_dense_geometry(*shape, product, out) == -2, (shape, product)           # a product of the other family
    assert list(out) == [-1] * 8


@pytest.mark.parametrize('K,M,tiles', [(33, 7, 2), (32, 32, 1), (40, 70, 6), (64, 64, 4), (128, 97, 16), (1198, 97, 152)])
def test_grad_w_rows_are_owned_once(K, M, tiles):
    """k_dense_wgrad's row ranges, modelled from the geometry query's (splits, rows per split): every row in [0, N) belongs to
    exactly one (split, wave), a wave's range begins on an even row (its MFMA steps take rows in pairs), the splits are the
    host's (1024 / tiles, at most 512, halved while a split would hold fewer than 256 rows)"""
    sweep = sorted({N for c in (256, 512, 1024) for N in range(c - 9, c + 10)} | {1, 2, 5, 7, 8, 9, 31, 33, 2047, 2048, 2049, 4100})
    first = min(512, max(1, 1024 // tiles))
    for N in sweep:
        t, splits, rps = geometry(N, K, M, GRAD_W)
        assert t == tiles == cdiv(K, 32) * cdiv(M, 32)
        assert 1 <= splits <= first
        assert splits == 1 or N // splits >= 256
        assert splits == first or N // (2 * splits + 1) < 256          # halved (2 s or 2 s + 1 -> s) no further than needed
        assert rps % 8 == 0 and rps - 8 < cdiv(N, splits) <= rps
        owners = [0] * N
        for (split, wave), (b, e) in wgrad_rows(N, splits, rps).items():
            assert b % 2 == 0
            for row in range(b, e):
                owners[row] += 1
        assert owners == [1] * N, (N, K, M)


def test_every_named_case_owns_its_rows_once():
    for table in (WGRAD, MFMA):
        for name, ((N, K, M, _), _, _, want) in table.items():
            tiles, splits, rps = geometry(N, K, M, GRAD_W)
            assert (tiles, splits, rps) == want
            owners = [0] * N
            for b, e in wgrad_rows(N, splits, rps).values():
                for row in range(b, e):
                    owners[row] += 1
            assert owners == [1] * N, name
