# -*- coding:utf-8 -*-
"""GPU: the slot optimizers' kernels (csrc/optim_slots.hip: Adagrad, RMSprop, momentum SGD, Adamax, Ftrl) compute, bit for bit,
what the two kernel families they were merged from computed.  tests/golden/optimizer_steps_parent.npz was recorded by
tools/make_optimizer_golden.py on an MI355X from the build of the last commit with both families (csrc/optim.hip's k_slot_* and
csrc/optim2.hip's k_slot2_*); the calls (tests/optimizer_family_cases.py) are replayed here on the current build.

Per output array — every weight, slot, stamp and dense-tail array and the step counter of every case — the fixture holds a
16-byte digest of its bytes instead of the array (the arrays come to 5.5 MB); equal digests are equal bytes, and the
arrays are checked to be finite, so this asserts no less than `torch.equal`.  The inputs' hash is checked first: a drift of
the seeded generators fails as "inputs differ", not as a kernel failure."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import optimizer_family_cases as C

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'optimizer_steps_parent.npz')
ROW_NAMES = tuple(C.KINDS) + ('rmsprop_in_record',)
LEGS = [f'dense/{k}' for k in C.KINDS] + [f'multi/{k}' for k in C.KINDS] + [f'rows/{k}' for k in ROW_NAMES]


@functools.lru_cache(maxsize=None)
def _golden():
    z = np.load(GOLDEN)
    return str(z['inputs_hash']), dict(zip((str(n) for n in z['names']), z['digests']))


@functools.lru_cache(maxsize=None)
def _replayed():
    from deeptables_amd import _lib
    return C.run(_lib.lib())


def test_inputs_are_the_recorded_ones():
    assert _replayed()[0] == _golden()[0], 'inputs differ: the seeded generators no longer give what the fixture was recorded from'
    assert sorted(_replayed()[1]) == sorted(_golden()[1]), 'the cases differ from the recorded ones'


def test_every_leg_is_covered():
    names = list(_golden()[1])
    assert all(any(n.startswith(leg + '/') for leg in LEGS) for n in names)
    for leg in LEGS:
        mine = [n for n in names if n.startswith(leg + '/')]
        assert mine, leg
        if leg.startswith('rows/'):       # D x fields x tail, and the two-slot kinds' second slot, RMSprop's stamps
            assert len({n.rsplit('/', 1)[0] for n in mine if '/materialized' not in n}) == \
                len(C.ROW_SHAPES) * len(C.ROW_FIELDS) * 2


@pytest.mark.parametrize('leg', LEGS)
def test_same_bits_as_the_recorded_build(leg):
    assert _replayed()[0] == _golden()[0], 'inputs differ'
    want, got = _golden()[1], _replayed()[1]
    names = [n for n in want if n.startswith(leg + '/')]
    assert names
    for n in names:
        if got[n].is_floating_point():
            assert torch.isfinite(got[n]).all(), n
    differing = [n for n in names if not np.array_equal(C.digest(got[n]), want[n])]
    assert not differing, f'{len(differing)} of {len(names)} arrays differ from the recorded build: {differing[:8]}'
