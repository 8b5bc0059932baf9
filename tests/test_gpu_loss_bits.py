"""The bits of the loss kernels, pinned: photometric_forward / _backward and training_loss_forward / _backward with every extra give, on the
inputs of tests/loss_bits_cases.py, exactly what tests/golden/loss_bits.npz holds -- outputs recorded (tools/record_loss_bits.py) from the
kernels as they were when the plain and the training pair were two separate copies.  The other loss tests compare the kernels with each other
and with counted bounds; an edit that moves both pairs the same way passes them and fails here."""
import functools
import os

import numpy as np
import pytest

import loss_bits_cases as cases

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "loss_bits.npz")


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(GOLDEN) as f:
        return {k: f[k] for k in f.files}


def test_fixture_holds_every_expected_entry_and_no_other():
    g = golden()
    assert sorted(g) == sorted(cases.keys())
    for k, v in g.items():
        shape, call, output = k.split(".")
        raw = shape == cases.shape_id(cases.RAW_SHAPE) or output in cases.ALWAYS_RAW
        assert (v.dtype == np.float32 and v.size > 0) if raw else (v.dtype == np.uint8 and v.shape == (32,)), k


@pytest.mark.parametrize("shape", cases.SHAPES, ids=cases.shape_id)
def test_both_loss_pairs_give_the_recorded_bits(shape):
    g = golden()
    got = cases.entries(shape, cases.run(shape))
    assert len(got) == sum(len(o) for o in cases.OUTPUTS.values())
    for k, v in got.items():
        assert k in g, f"{k} is not in the fixture"
        want = g[k]
        assert v.dtype == want.dtype and v.shape == want.shape, k
        if v.dtype == np.float32:   # bits, not values: -0.0 is not 0.0 here
            v, want = v.view(np.uint32), want.view(np.uint32)
        assert np.array_equal(v, want), f"{k}: {int((v != want).sum())} of {v.size} {'floats' if v.dtype == np.uint32 else 'digest bytes'} differ"
