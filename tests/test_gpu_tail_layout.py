"""The head and loss tail of Two_transformers with its three layout switches — JMT_HEAD_PERM (the
head kernels write the seq-first predictions in their logical order), JMT_CCC_FUSED_FINISH (CCC
statistics and finish in one launch), JMT_STACK_INPLACE (the video projection and the normalised
audio written into their slots of the stacked X) — all on against all off: none changes an
output element's arithmetic, so outputs, loss and every parameter gradient are equal bit for bit,
eager and under one captured-graph replay, and the eager step's kernel list loses exactly the
launches the switches remove.  B = 3, T = 7 is under one wave of head rows; B = 2, T = 130 is
260 rows: five head blocks, the last one partial."""
import pytest
import torch

from jmt import functional as JF
from jmt.graph import GraphedStep
from jmt.optim import FusedSGD, used_parameters
from oracle.hashinit import init_module_

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
CD = torch.bfloat16


def _switches(on):
    JF.set_head_perm(on)
    JF.set_ccc_fused_finish(on)
    JF.set_stack_inplace(on)


def _setup(B, T, fmt="FC"):
    """A fresh hash-initialised model and one forward + backward into the optimizer's flat
    gradient buffer (zeroed first; no parameter update, so every call computes the same step)."""
    from models.two_transformers import Two_transformers
    from losses.loss import CCCLoss
    m = Two_transformers(0.0, 0.0, 1, 1, "TRANSFORMER", fmt, 2048)
    init_module_(m, "")
    m = m.to(DEV)
    g = torch.Generator(device=DEV).manual_seed(7)
    audio = torch.randn(B, T, 512, device=DEV, generator=g)
    video = torch.randn(B, T, 2048, device=DEV, generator=g)
    lv = (torch.rand(B, T, device=DEV, generator=g) * 2 - 1).view(-1, B * T)
    la = (torch.rand(B, T, device=DEV, generator=g) * 2 - 1).view(-1, B * T)
    crit = CCCLoss(1)
    seen = {}

    def fwd_bwd():
        with JF.compute_mode(CD):
            vo, ao = m(audio, video)
            seen["contiguous"] = vo.is_contiguous() and ao.is_contiguous()
            seen["shape"] = tuple(vo.shape)
            if fmt == "FC":         # seq-first (T, B) predictions against (T, B)-ordered labels
                loss = crit(vo.view(-1, B * T), lv) + crit(ao.view(-1, B * T), la)
            else:
                loss = crit(vo.reshape(-1, B * T), lv) + crit(ao.reshape(-1, B * T), la)
            loss.backward()
        return loss, vo, ao

    params = used_parameters(lambda: fwd_bwd()[0], list(m.parameters()))
    opt = FusedSGD(params, lr=1e-2, momentum=0.9, shadow_dtype=CD)

    def step():
        opt.zero_grad(force=True)
        loss, vo, ao = fwd_bwd()
        return loss.detach(), vo.detach(), ao.detach()

    return step, opt, seen, m


def _run(B, T, on, graphed, fmt="FC"):
    _switches(on)
    try:
        step, opt, seen, _ = _setup(B, T, fmt)
        step()                                   # (the weights' 16-bit copies are cast once)
        if graphed:
            gs = GraphedStep(step).capture(warmup=1)
            opt.flat_g.fill_(float("nan"))
            out = gs.replay()
        else:
            out = step()
        torch.cuda.synchronize()
        return [o.clone() for o in out] + [opt.flat_g.clone()], seen
    finally:
        _switches(True)


@pytest.fixture(scope="module")
def off_eager():
    """The switch-off eager step per shape, computed once."""
    return {(B, T): _run(B, T, False, False) for B, T in ((3, 7), (2, 130))}


@pytest.mark.parametrize("graphed", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("B,T", [(3, 7), (2, 130)])
def test_switches_keep_every_bit(B, T, graphed, off_eager):
    ref, seen0 = off_eager[B, T]
    got, seen1 = _run(B, T, True, graphed)
    assert seen1["shape"] == (T, B) and seen1["contiguous"] and seen0["contiguous"]
    assert not bool(torch.isnan(got[3]).any()) and float(got[3].abs().max()) > 0
    for name, r, g in zip(("loss", "vouts", "aouts", "gradients"), ref, got):
        assert r.shape == g.shape and torch.equal(r, g), name
    if graphed:     # and the switch-off capture replays the same bits
        got0, _ = _run(B, T, False, True)
        for r, g in zip(ref, got0):
            assert torch.equal(r, g)


def _kernel_names(fn):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]


def _both_bf16(name):
    """copy_rows_vec_kernel<__bf16, __bf16>, demangled or not (DF16b is __bf16's mangling)"""
    return name.count("bf16") >= 2 or name.count("DF16b") >= 2


def test_eager_step_loses_the_eight_launches():
    """(Split-K pinned to 1 in both arms: at 260 rows the encoder's accumulating input-gradient
    GEMM would otherwise split K and copy its bf16 addend into the output first — a
    copy_rows_vec_kernel<bf16, bf16> of the GEMM plan that the training shapes do not launch.)"""
    from jmt import ops
    names = {}
    auto = ops.auto_splits
    for on in (False, True):
        _switches(on)
        ops.auto_splits = lambda *a: 1
        try:
            step, _, _, _ = _setup(2, 130)
            step()
            names[on] = _kernel_names(step)
        finally:
            ops.auto_splits = auto
            _switches(True)
    if not names[True] or not names[False]:
        pytest.skip("torch.profiler recorded no device kernels")
    count = lambda on, pred: sum(1 for n in names[on] if pred(n))
    t2d = lambda n: "copy2d_kernel" in n
    rows = lambda n: "copy_rows_vec_kernel" in n and _both_bf16(n)
    fin = lambda n: "ccc_finish_kernel" in n
    # off: the four transposing copies of the head, the two slot copies, the two finishes
    assert count(False, t2d) - count(True, t2d) == 4 and count(True, t2d) == 0
    assert count(False, rows) - count(True, rows) == 2 and count(True, rows) == 0
    assert count(False, fin) == 2 and count(True, fin) == 0
    assert count(True, lambda n: "ccc_stats_finish_kernel" in n) == 2
    assert len(names[False]) - len(names[True]) == 8


def test_fusion_module_with_separate_inputs():
    """mm_transformer called directly: nothing was written into a stacked buffer, the two inputs
    are copied into it as before, under either setting."""
    res = {}
    for on in (False, True):
        _switches(on)
        try:
            _, _, _, m = _setup(2, 9)
            mm = m.mm_transformer
            g = torch.Generator(device=DEV).manual_seed(3)
            v = torch.randn(2, 9, 512, device=DEV, generator=g).to(CD).requires_grad_(True)
            p = torch.randn(2, 9, 512, device=DEV, generator=g).to(CD).requires_grad_(True)
            for q in mm.parameters():
                q.grad = None
            with JF.compute_mode(CD):
                av = mm(v, p)
                av.float().square().sum().backward()
            torch.cuda.synchronize()
            res[on] = [av.detach().clone(), v.grad.clone(), p.grad.clone()] + \
                [q.grad.clone() for q in mm.parameters() if q.grad is not None]
        finally:
            _switches(True)
    assert len(res[True]) == len(res[False]) > 3
    for a, b in zip(res[False], res[True]):
        assert a.shape == b.shape and torch.equal(a, b)


def test_self_atten_head_unchanged():
    """SELF_ATTEN returns batch-first (B, T) predictions: no row map; the slots and the fused
    finish still apply."""
    ref, _ = _run(2, 9, False, False, fmt="SELF_ATTEN")
    got, seen = _run(2, 9, True, False, fmt="SELF_ATTEN")
    assert seen["shape"] == (2, 9)
    for r, g in zip(ref, got):
        assert r.shape == g.shape and torch.equal(r, g)
