"""The dropout mask specification on the CPU: the numpy reference (tests/dropout_ref.py, written
from DESIGN.md §4) against Philox4x32-10's known answers, the library's host reference
(jmt_dropout_reference, compiled from the header the kernels use) against the numpy one, and the
statistics of the mask."""
import math

import numpy as np
import pytest

from jmt import ops

from tests import dropout_ref as R

KAT = [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     "d16cfe09 94fdcceb 5001e420 24126ea1"),
]


@pytest.mark.parametrize("ctr,key,want", KAT, ids=["zeros", "ones", "pi"])
def test_philox_known_answers(ctr, key, want):
    got = " ".join("%08x" % int(w) for w in R.philox4x32_10(ctr, key))
    assert got == want


def test_philox_is_vectorised():
    ctr = [np.array([c[0][i] for c in KAT], dtype=np.uint64) for i in range(4)]
    key = [np.array([c[1][i] for c in KAT], dtype=np.uint64) for i in range(2)]
    out = R.philox4x32_10(ctr, key)
    for j, (_, _, want) in enumerate(KAT):
        assert " ".join("%08x" % int(w[j]) for w in out) == want


def test_threshold_and_scale():
    assert R.threshold(0.0) == 0 and R.scale(0.0) == 1.0
    assert R.threshold(0.5) == 1 << 31 and R.scale(0.5) == 2.0
    # the rate is the float32 argument, not the Python double
    assert R.threshold(0.1) == int(float(np.float32(0.1)) * 2.0 ** 32)
    assert R.threshold(0.999) < 1 << 32


SEED = 0x1234_5678_9ABC_DEF0


@pytest.mark.parametrize("shape", [(1, 4, 4), (65, 256, 128), (130, 260, 128)],
                         ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("p", [(0.0, 0.0), (0.1, 0.5), (0.999, 0.25)], ids=str)
@pytest.mark.parametrize("call", [0, 2 ** 32 - 1], ids=["call0", "callmax"])
def test_library_reference_equals_numpy(shape, p, call):
    rows, cols, split = shape
    ctr = (SEED & 0xFFFFFFFF, SEED >> 32, call, 3)
    got = ops.dropout_reference(ctr, rows, cols, split, *p)
    want = R.mask(ctr, rows, cols, split, *p)
    assert got.dtype == np.float32 and got.shape == (rows, cols)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    if p == (0.0, 0.0):
        assert np.all(got == 1.0)
    else:
        for half, ph in ((got[:, :split], p[0]), (got[:, split:], p[1])):
            assert set(np.unique(half)) <= {np.float32(0.0), R.scale(ph)}


def test_library_reference_rejects_bad_arguments():
    from jmt._lib import JMTError
    for args in [((1, 2, 3, 4), 1, 6, 4, 0.1, 0.1), ((1, 2, 3, 4), 1, 8, 6, 0.1, 0.1),
                 ((1, 2, 3, 4), 1, 8, 4, 1.0, 0.1), ((1, 2, 3, 4), 1, 8, 4, 0.1, -0.5)]:
        with pytest.raises(JMTError):
            ops.dropout_reference(*args)


def _within(frac, expect, n):
    return abs(frac - expect) <= 4.5 * math.sqrt(expect * (1.0 - expect) / n)


def test_mask_statistics():
    """4096 x 256, p = (0.1, 0.5): each half keeps 1 - p of its elements, and the masks of two
    consecutive calls, and of two streams, agree where independent masks would (p^2 + (1-p)^2),
    all within 4.5 sigma of the binomial.  The seed is fixed; the numpy reference alone passes
    the same bounds at it (checked below on both implementations)."""
    rows, cols, split, p = 4096, 256, 128, (0.1, 0.5)
    lo, hi, c = SEED & 0xFFFFFFFF, SEED >> 32, 41
    n = rows * split
    for ref in (lambda ctr: R.mask(ctr, rows, cols, split, *p),
                lambda ctr: ops.dropout_reference(ctr, rows, cols, split, *p)):
        base = ref((lo, hi, c, 0)) != 0
        nxt = ref((lo, hi, c + 1, 0)) != 0
        oth = ref((lo, hi, c, 1)) != 0
        for half, ph in ((slice(0, split), p[0]), (slice(split, cols), p[1])):
            assert _within(base[:, half].mean(), 1.0 - ph, n)
            agree = ph * ph + (1.0 - ph) ** 2
            assert _within((base[:, half] == nxt[:, half]).mean(), agree, n)
            assert _within((base[:, half] == oth[:, half]).mean(), agree, n)
