# -*- coding:utf-8 -*-
"""Shared by the host and the GPU tests of csrc/dense.hip: the geometry query as a Python call, and the named cases with the
geometry each of them is there to reach (tests/test_dense_host.py asserts it without a GPU, tests/test_dense_edges_gpu.py
runs them).  The table of which case reaches which branch of the kernels is at the top of tests/test_dense_edges_gpu.py."""
import ctypes

FWD, GRAD_X, GRAD_W, D1_FWD, D1_BWD = 0, 1, 2, 3, 4
WORDS = {FWD: 7, GRAD_X: 7, GRAD_W: 3, D1_FWD: 1, D1_BWD: 3}       # meaningful words of dt_dense_geometry's out[8]
LDS_LIMIT = 150 * 1024


def geometry(N, K, M, product):
    """what dt_dense_geometry says the launch of one product uses:
      FWD, GRAD_X  (column waves NBW, rows per block, grid, dynamic LDS bytes, pipelined chunks nch, trips of the guarded
                   remainder loop — the odd-K step included —, 1 where the row length permits 16-byte staging)
      GRAD_W       (32 x 32 tiles, batch splits, rows per split)
      D1_FWD       (grid,)
      D1_BWD       (rows per block, blocks, blocks of the reduce)"""
    from deeptables_amd import _lib
    out = (ctypes.c_int * 8)(*([-1] * 8))
    _lib.check(_lib.lib().dt_dense_geometry(N, K, M, product, out), 'dt_dense_geometry')
    assert all(v == 0 for v in out[WORDS[product]:])
    return tuple(out[:WORDS[product]])


def cdiv(a, b):
    return -(-a // b)


# name -> ((N, K, M, bias), geometry of the forward, of grad_x, of grad_W).  grad_x is the forward's kernel with K and M
# swapped and the relu mask applied while staging, so every case reaches two MFMA geometries.
#   f<w>_n<N>: the forward runs NBW = w column waves at batch N;  g<w>_n<N>: grad_x does;  lim*: dt_dense_supported's limits
MFMA = {
    'f1_n127': ((127, 31, 2, True), (1, 128, 1, 16896, 0, 16, 0), (1, 128, 1, 1536, 0, 1, 0), (1, 1, 128)),
    'f1_n128': ((128, 32, 32, True), (1, 128, 1, 16896, 1, 0, 1), (1, 128, 1, 16896, 1, 0, 1), (1, 1, 128)),
    'f1_n129': ((129, 33, 32, False), (1, 128, 2, 17920, 1, 1, 0), (2, 64, 3, 8448, 1, 0, 1), (2, 1, 136)),
    'f1_n1': ((1, 3, 2, True), (1, 128, 1, 2560, 0, 2, 0), (1, 128, 1, 1536, 0, 1, 0), (1, 1, 8)),
    'f2_n63': ((63, 64, 33, True), (2, 64, 1, 16640, 2, 0, 1), (2, 64, 1, 8960, 1, 1, 0), (4, 1, 64)),
    'f2_n64': ((64, 66, 96, False), (2, 64, 1, 17152, 2, 1, 0), (2, 64, 1, 24832, 3, 0, 1), (9, 1, 64)),
    'f2_n65': ((65, 96, 65, True), (2, 64, 2, 24832, 3, 0, 1), (2, 64, 2, 17152, 2, 1, 0), (9, 1, 72)),
    'f2_n1': ((1, 2, 33, True), (2, 64, 1, 768, 0, 1, 0), (1, 128, 1, 17920, 1, 1, 0), (2, 1, 8)),
    'f2_vec': ((65, 64, 96, True), (2, 64, 2, 16640, 2, 0, 1), (2, 64, 2, 24832, 3, 0, 1), (6, 1, 72)),
    'f4_n31': ((31, 97, 97, True), (4, 32, 1, 12672, 3, 1, 0), (4, 32, 1, 12672, 3, 1, 0), (16, 1, 32)),
    'f4_n32': ((32, 128, 128, True), (4, 32, 1, 16512, 4, 0, 1), (4, 32, 1, 16512, 4, 0, 1), (16, 1, 32)),
    'f4_n33': ((33, 161, 129, False), (4, 32, 2, 20864, 5, 1, 0), (4, 32, 2, 16768, 4, 1, 0), (30, 1, 40)),
    'f4_n1': ((1, 1, 97, True), (4, 32, 1, 384, 0, 1, 0), (1, 128, 1, 50688, 3, 1, 0), (4, 1, 8)),
    'g1_n129': ((129, 3, 66, False), (2, 64, 3, 1280, 0, 2, 0), (1, 128, 2, 34304, 2, 1, 0), (3, 1, 136)),
    'g2_n1': ((1, 33, 2, True), (1, 128, 1, 17920, 1, 1, 0), (2, 64, 1, 768, 0, 1, 0), (2, 1, 8)),
    'g4_n1': ((1, 97, 3, False), (1, 128, 1, 50688, 3, 1, 0), (4, 32, 1, 640, 0, 2, 0), (4, 1, 8)),
    'lim4': ((130, 1198, 97, True), (4, 32, 5, 153472, 37, 7, 0), (4, 32, 5, 12672, 3, 1, 0), (152, 1, 136)),
    'lim2': ((65, 598, 33, True), (2, 64, 2, 153344, 18, 11, 0), (4, 32, 3, 4480, 1, 1, 0), (38, 1, 72)),
    'lim1': ((129, 298, 2, False), (1, 128, 2, 153088, 9, 5, 0), (4, 32, 5, 384, 0, 1, 0), (10, 1, 136)),
    'lim4_gx': ((33, 97, 1198, True), (4, 32, 2, 12672, 3, 1, 0), (4, 32, 2, 153472, 37, 7, 0), (152, 1, 40)),
}
# the largest K (M for lim4_gx) the slab holds at each NBW; one more is refused
LIMITS = ('lim4', 'lim2', 'lim1', 'lim4_gx')

# grad_W's row ranges: same layout.  Four waves take quarters of a split's rows, 32 rows per chunk.
WGRAD = {
    'w_n5': ((5, 33, 5, True), (1, 128, 1, 17920, 1, 1, 0), (2, 64, 1, 1792, 0, 3, 0), (2, 1, 8)),
    'w_n128': ((128, 32, 32, True), (1, 128, 1, 16896, 1, 0, 1), (1, 128, 1, 16896, 1, 0, 1), (1, 1, 128)),
    'w_n200': ((200, 40, 70, True), (2, 64, 4, 10496, 1, 4, 1), (2, 64, 4, 18176, 2, 3, 0), (6, 1, 200)),
    'w_n512': ((512, 64, 32, True), (1, 128, 4, 33280, 2, 0, 1), (2, 64, 8, 8448, 1, 0, 1), (2, 2, 256)),
    'w_n513': ((513, 32, 33, False), (2, 64, 9, 8448, 1, 0, 1), (1, 128, 5, 17920, 1, 1, 0), (2, 2, 264)),
    'w_n1030': ((1030, 33, 7, True), (1, 128, 9, 17920, 1, 1, 0), (2, 64, 17, 2304, 0, 4, 0), (2, 4, 264)),
    'w_nogb': ((200, 40, 70, True), (2, 64, 4, 10496, 1, 4, 1), (2, 64, 4, 18176, 2, 3, 0), (6, 1, 200)),
    'w_autoint': ((300, 16, 48, True), (2, 64, 5, 4352, 0, 8, 1), (1, 128, 3, 25088, 1, 8, 1), (2, 1, 304)),
}

# Dense(1): name -> ((N, K, 1, bias), geometry of the forward, of the backward)
D1 = {
    'd1_n1_k5': ((1, 5, 1, True), (1,), (32, 1, 1)),
    'd1_n3_k64': ((3, 64, 1, False), (1,), (32, 1, 2)),
    'd1_n4_k65': ((4, 65, 1, True), (1,), (32, 1, 2)),
    'd1_n5_k129': ((5, 129, 1, True), (2,), (32, 1, 3)),
    'd1_n33_k4': ((33, 4, 1, True), (9,), (32, 2, 1)),
    'd1_n64_k8': ((64, 8, 1, True), (16,), (32, 2, 1)),
    'd1_n98_k1028': ((98, 1028, 1, False), (25,), (32, 4, 17)),
    'd1_n131_k63': ((131, 63, 1, True), (33,), (32, 5, 1)),
    'd1_n1925_k1': ((1925, 1, 1, True), (482,), (32, 61, 1)),
    'd1_n2048_k2': ((2048, 2, 1, True), (512,), (32, 64, 1)),
    'd1_n2050_k3': ((2050, 3, 1, False), (513,), (32, 65, 1)),
    'd1_n4100_k257': ((4100, 257, 1, True), (1025,), (32, 129, 5)),
    'd1_n16385_k8': ((16385, 8, 1, True), (4096,), (32, 513, 1)),
    'd1_n32769_k8': ((32769, 8, 1, True), (4096,), (33, 993, 1)),
    'd1_n65537_k5': ((65537, 5, 1, False), (4096,), (64, 1025, 1)),
    'd1_nogx': ((131, 8, 1, True), (33,), (32, 5, 1)),
    'd1_nogb': ((131, 63, 1, True), (33,), (32, 5, 1)),
}

# how a case is called, where not "every pointer given, relu": gx / gb False -> grad_x / grad_b = NULL;  autoint -> ops.py's
# AutoInt projection call: grad_x = NULL, ws = NULL, act = linear, W and y aliased to grad_y
OPTIONS = {'w_nogb': dict(gb=False), 'w_autoint': dict(autoint=True), 'd1_nogx': dict(gx=False), 'd1_nogb': dict(gb=False)}

# the cases that run under a linear activation as well (the mask is then the identity: grad_x stages grad_y itself)
LINEAR_TOO = {'f1_n127', 'f1_n128', 'f2_n63', 'f2_n64', 'f4_n32', 'f4_n33', 'g4_n1', 'lim2', 'w_n5', 'w_n513',
              'd1_n1_k5', 'd1_n3_k64', 'd1_n4_k65', 'd1_n5_k129', 'd1_n33_k4', 'd1_n98_k1028', 'd1_n131_k63', 'd1_n16385_k8'}

# representatives of the guard-band, accumulate, misalignment and reproducibility tests
GUARDED = ('f1_n127', 'f2_n65', 'f4_n33', 'w_n513', 'd1_n98_k1028', 'd1_n131_k63')
ACCUMULATE = ('f2_n65', 'w_n513', 'd1_n64_k8', 'd1_n131_k63')
MISALIGNED = ('f2_vec', 'f4_n32', 'd1_n64_k8', 'd1_n98_k1028')
REPEATED = ('f1_n129', 'f2_vec', 'f4_n33', 'w_n513', 'd1_n98_k1028', 'd1_n4100_k257')


def case(name):
    """-> (N, K, M, bias), options"""
    for table in (MFMA, WGRAD, D1):
        if name in table:
            return table[name][0], OPTIONS.get(name, {})
    raise KeyError(name)


def wgrad_rows(N, splits, rows_per_split):
    """k_dense_wgrad's row ownership: {(split, wave): (r_begin, r_end)} — a split's rows in quarters, the end clipped to N
    (r_end < r_begin: an empty range)"""
    rq = rows_per_split >> 2
    out = {}
    for split in range(splits):
        for wave in range(4):
            r_begin = split * rows_per_split + wave * rq
            out[(split, wave)] = (r_begin, min(N, r_begin + rq))
    return out
