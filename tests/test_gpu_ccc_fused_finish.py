"""jmt_ccc_stats_finish(_add) — the CCC statistics and the one-rank finish in one launch —
against jmt_ccc_stats followed by jmt_ccc_finish(_add)(world = 1): stats, loss and coef bit for
bit (the finish is one compiled device function that both kernels call; the statistics block is
the same code).  Kinds 0 and 1; k = 1, 2, 64; n = 1 (no variance: kind 1 returns early with coef
zeroed), 2, 1023 / 1024 (one element per thread, one short of it), 24,577 (one past the
24 x 1024 register-cached elements); with `add`; every label ignored (kind 1).  Outputs start as
NaN between NaN guards, which must come back untouched; and CCCLossFn takes the fused launch
without a group and gives the same loss and gradient as with JMT_CCC_FUSED_FINISH=0."""
import math

import pytest
import torch

from jmt import functional as JF
from jmt import ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
GUARD = 16
IGNORE = -5.0
I64 = torch.int64


def _buf(n, dtype):
    flat = torch.full((GUARD + n + GUARD,), math.nan, dtype=dtype, device=DEV)
    v = flat[GUARD:GUARD + n]
    v.gflat = flat
    return v


def _guards_ok(*views):
    for v in views:
        n = v.numel()
        assert bool(torch.isnan(v.gflat[:GUARD]).all()) and \
            bool(torch.isnan(v.gflat[GUARD + n:]).all())


def _bits(t):
    return t.cpu().view(torch.int32 if t.dtype == torch.float32 else I64)


@pytest.fixture(scope="module")
def data():
    """(pred (n, k) fp32, labels) per (n, k), made once; labels in [-1, 1] with ~1/7 ignored."""
    out = {}
    g = torch.Generator().manual_seed(11)
    for n in (1, 2, 1023, 1024, 24577):
        for k in (1, 2, 64):
            pred = torch.randn(n, k, generator=g) * (0.5 if k == 1 else 2.0)
            lab = torch.rand(n, generator=g) * 2 - 1
            lab[torch.rand(n, generator=g) < 1 / 7] = IGNORE
            out[n, k] = (pred.to(DEV), lab.to(DEV))
    return out


def _both(kind, k, pred, lab, bs, eps, add):
    n = lab.numel()
    s2, l2, c2 = _buf(8, torch.float64), _buf(1, torch.float32), _buf(8, torch.float64)
    ops.ccc_stats(kind, pred, lab, k, IGNORE, -1.0, 1.0, s2)
    ops.ccc_finish(kind, 1, s2, bs, eps, l2, c2, add=add)
    s1, l1, c1 = _buf(8, torch.float64), _buf(1, torch.float32), _buf(8, torch.float64)
    ops.ccc_stats_finish(kind, pred, lab, k, IGNORE, -1.0, 1.0, s1, bs, eps, l1, c1, add=add)
    torch.cuda.synchronize()
    _guards_ok(s1, l1, c1, s2, l2, c2)
    assert torch.equal(_bits(s1), _bits(s2)), (n, k, s1.tolist(), s2.tolist())
    assert torch.equal(_bits(l1), _bits(l2)), (n, k, float(l1), float(l2))
    assert torch.equal(_bits(c1), _bits(c2)), (n, k, c1.tolist(), c2.tolist())
    return l1, c1


@pytest.mark.parametrize("with_add", [False, True], ids=["plain", "add"])
@pytest.mark.parametrize("n", [1, 2, 1023, 1024, 24577])
@pytest.mark.parametrize("k", [1, 2, 64])
@pytest.mark.parametrize("kind", [0, 1])
def test_fused_finish_matches_two_kernels(kind, k, n, with_add, data):
    if kind == 1 and k > 1:
        k_pred = data[n, k][0][:, :1].contiguous()      # kind 1 has no bins: k = 1 of this draw
        pred, kk = k_pred, 1
    else:
        pred, kk = data[n, k][0], k
    lab = data[n, k][1]
    add = torch.full((1,), 0.625, dtype=torch.float32, device=DEV) if with_add else None
    bs = 1 if kind == 0 else (-1 if k == 2 else 1)      # kind 1: also the summed pre-mask count
    loss, coef = _both(kind, kk, pred, lab, bs, 1e-8 if kind == 0 else 0.0, add)
    if kind == 1 and n == 1:
        # at most one valid element: loss 0 (+ add), coef zeroed apart from the two means
        assert float(loss) == (0.625 if with_add else 0.0)
        c = coef.cpu().tolist()
        assert c[0] == c[1] == c[2] == c[5] == c[6] == c[7] == 0.0
    elif n >= 1023:
        assert math.isfinite(float(loss)) and float(coef[5]) == 1.0


@pytest.mark.parametrize("n", [2, 1024, 24577])
def test_fused_finish_all_labels_ignored(n, data):
    pred = data[n, 1][0]
    lab = torch.full((n,), IGNORE, device=DEV)
    loss, coef = _both(1, 1, pred, lab, 1, 0.0, None)
    assert float(loss) == 0.0 and coef.cpu().tolist() == [0.0] * 8


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_fused_finish_16bit_predictions(dtype, data):
    pred, lab = data[24577, 2]
    _both(0, 2, pred.to(dtype), lab.clamp(min=-1.0), 1, 1e-8, None)


def test_loss_function_takes_the_fused_launch():
    """CCCLossFn without a group: one launch with the switch on, the same bits with it off."""
    torch.manual_seed(5)
    pred0 = torch.randn(1, 1500, device=DEV)
    lab = torch.rand(1, 1500, device=DEV) * 2 - 1
    lab[0, ::9] = IGNORE
    calls = []
    orig = ops.ccc_stats_finish

    def spy(*a, **kw):
        calls.append(1)
        return orig(*a, **kw)

    res = {}
    ops.ccc_stats_finish = spy
    try:
        for on in (False, True):
            JF.set_ccc_fused_finish(on)
            p = pred0.clone().requires_grad_(True)
            first = JF.ccc_loss_ignore(p, lab, ignore=IGNORE)
            total = JF.ccc_loss(p, lab.clamp(min=-1.0), add=first)
            total.backward()
            torch.cuda.synchronize()
            res[on] = (first.detach().clone(), total.detach().clone(), p.grad.clone())
            assert len(calls) == (2 if on else 0)
    finally:
        ops.ccc_stats_finish = orig
        JF.set_ccc_fused_finish(True)
    for a, b in zip(res[False], res[True]):
        assert torch.equal(_bits(a), _bits(b))
