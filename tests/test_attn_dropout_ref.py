"""The attention dropout mask specification on the CPU: the library's host reference
(jmt_attn_dropout_reference, compiled from the header the kernels use) against the numpy
restatement of tests/attn_drop_ref.py, the rate quantisation, and the statistics of the mask."""
import math

import numpy as np
import pytest

from jmt import ops
from jmt._lib import JMTError

from tests import attn_drop_ref as A

SEED = 0x1234_5678_9ABC_DEF0
BLOCKS = [(SEED & 0xFFFFFFFF, SEED >> 32, 0, 0), (0xDEADBEEF, 0x01234567, 2 ** 32 - 1, 3)]
RATES = [0.1, 0.25, 0.5]


@pytest.mark.parametrize("shape", [(1, 1, 1), (3, 9, 17), (5, 6, 130), (2, 65, 7)],
                         ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("p", RATES, ids=str)
@pytest.mark.parametrize("ctr", BLOCKS, ids=["block0", "block1"])
def test_library_reference_equals_numpy(shape, p, ctr):
    NH, Lq, Lk = shape
    got = ops.attn_dropout_reference(ctr, NH, Lq, Lk, p)
    want = A.mask(ctr, NH, Lq, Lk, p)
    assert got.dtype == np.float32 and got.shape == (NH, Lq, Lk)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert set(np.unique(got)) <= {np.float32(0.0), A.scale(p)}


def test_threshold_and_effective_rate():
    # T8 = floor(256 p + 1/2) of the float32 rate; p_eff = T8 / 256; s = 1 / (1 - p_eff) in fp32
    assert [A.threshold(p) for p in RATES] == [26, 64, 128]
    for p, t8 in zip(RATES, (26, 64, 128)):
        assert ops.attn_dropout_rate(p) == t8 / 256.0 == A.rate(p)
        assert A.scale(p) == np.float32(1.0) / np.float32(1.0 - t8 / 256.0)
    from jmt import functional as JF
    assert JF.attn_dropout_rate(0.1) == 26 / 256.0
    assert ops.attn_dropout_rate(0.0) == 0.0
    assert ops.attn_dropout_rate(255.4 / 256) == 255 / 256.0
    for bad in (255.5 / 256, 0.999, 1.0, -0.1):
        with pytest.raises(JMTError):
            ops.attn_dropout_rate(bad)
        with pytest.raises(JMTError):
            ops.attn_dropout_reference(BLOCKS[0], 1, 4, 4, bad)


@pytest.mark.parametrize("p", RATES, ids=str)
def test_dropped_share(p):
    """Over 2^20 elements the dropped share is within 5 sigma of p_eff (not of p)."""
    NH, Lq, Lk = 16, 256, 256
    n = NH * Lq * Lk
    assert n >= 2 ** 20
    pe = A.rate(p)
    for ref in (ops.attn_dropout_reference, A.mask):
        dropped = float((ref(BLOCKS[0], NH, Lq, Lk, p) == 0).mean())
        assert abs(dropped - pe) <= 5.0 * math.sqrt(pe * (1.0 - pe) / n), (dropped, pe)


def test_multiplier_does_not_depend_on_lk():
    a = ops.attn_dropout_reference(BLOCKS[1], 3, 9, 130, 0.25)
    for Lk in (1, 7, 17, 64, 129):
        b = ops.attn_dropout_reference(BLOCKS[1], 3, 9, Lk, 0.25)
        assert np.array_equal(a[:, :, :Lk], b)


def test_call_and_stream_change_the_mask():
    lo, hi, call, stream = BLOCKS[0]
    base = ops.attn_dropout_reference((lo, hi, call, stream), 4, 64, 64, 0.5)
    for other in ((lo, hi, call + 1, stream), (lo, hi, call, stream + 1), (lo + 1, hi, call, stream)):
        m = ops.attn_dropout_reference(other, 4, 64, 64, 0.5)
        agree = float(((m == 0) == (base == 0)).mean())
        # independent masks at p = 1/2 agree on half the elements (n = 2^14: 5 sigma = 0.02)
        assert abs(agree - 0.5) <= 0.02, agree


def test_rate_below_one_512th_keeps_everything():
    for p in (0.0, 1.0 / 1024, np.nextafter(np.float32(1.0 / 512), np.float32(0.0))):
        assert ops.attn_dropout_rate(p) == 0.0
        m = ops.attn_dropout_reference(BLOCKS[0], 2, 9, 17, p)
        assert np.all(m == np.float32(1.0))
    assert ops.attn_dropout_rate(1.0 / 512) == 1 / 256.0


def test_module_and_config_plumbing():
    """MultiheadAttention keeps its rate and reports it while training only;
    set_attention_dropout reaches every attention module; the config key is optional."""
    from jmt import config, nn as jnn
    m = jnn.MultiheadAttention(512, 8, dropout=0.3)
    assert m.dropout == 0.3 and m.drop_rate() == 0.3 and m.eval().drop_rate() == 0.0
    assert jnn.MultiheadAttention(512, 8).dropout == 0.0
    with pytest.raises(JMTError):
        jnn.MultiheadAttention(512, 8, dropout=1.0)
    mp = dict(v_dropout=0.0, a_dropout=0.0, num_heads=8, num_layers=1,
              joint_modalities="TRANSFORMER", output_format="FC")
    rates = lambda model: {a.dropout for a in model.modules()
                           if isinstance(a, jnn.MultiheadAttention)}
    assert rates(config.fusion_model({"model_params": mp})) == {0.0}
    model = config.fusion_model({"model_params": dict(mp, attn_dropout=0.25)})
    assert rates(model) == {0.25}
    assert rates(jnn.set_attention_dropout(model, 0.0)) == {0.0}
    with pytest.raises(JMTError):
        jnn.set_attention_dropout(model, 1.5)
