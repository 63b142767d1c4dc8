"""jmt_opt_tick + jmt_adam_step (csrc/adam.hip), FusedAdam, GradScaler + FusedAdam and the SGD
step with a device-resident lr.

Accuracy bound of the Adam kernel (and of FusedAdam): with the same seeded fp32 inputs,
    max|x_kernel - x_fp64| <= 4 * max|x_torch_fp32 - x_fp64| + 1e-12
for x in {param, exp_avg, exp_avg_sq}, where x_fp64 is torch.optim.Adam on the CPU in float64 and
x_torch_fp32 the same class in float32.  Both error terms are computed here, nothing is
hard-coded; the factor 4 allows for fma contraction and the order of the divide and sqrt (an
independently associated fp32 restatement of the update sits at a ratio of 1.0: one ulp of p)."""
import math

import pytest
import torch

from jmt import _lib, ops
from jmt.optim import FusedAdam, FusedSGD, GradScaler

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
LR, BETAS, EPS = 1e-3, (0.9, 0.999), 1e-8


def _grads(shape, steps, gen, zero_mask=None):
    """Gradients whose magnitudes span 1e-4 .. 1 (log-uniform per element)."""
    out = []
    for _ in range(steps):
        g = torch.randn(shape, generator=gen) * 10.0 ** (-4.0 * torch.rand(shape, generator=gen))
        if zero_mask is not None:
            g[zero_mask] = 0.0
        out.append(g)
    return out


def _torch_adam(p0s, grads, dtype, amsgrad, wd, steps):
    """torch.optim.Adam on the CPU in `dtype`; returns per-parameter (p, exp_avg, exp_avg_sq)."""
    ps = [torch.nn.Parameter(p.clone().to(dtype)) for p in p0s]
    opt = torch.optim.Adam(ps, lr=LR, betas=BETAS, eps=EPS, weight_decay=wd, amsgrad=amsgrad,
                           foreach=False)
    for k in range(steps):
        for p, g in zip(ps, grads[k]):
            p.grad = g.clone().to(dtype)
        opt.step()
    return [(p.detach().double(), opt.state[p]["exp_avg"].double(),
             opt.state[p]["exp_avg_sq"].double()) for p in ps]


def _check_bound(what, mine, ref32, ref64):
    e_mine = float((mine.double().cpu() - ref64).abs().max())
    e_torch = float((ref32 - ref64).abs().max())
    print(f"{what}: kernel err {e_mine:.3e}  torch fp32 err {e_torch:.3e}  "
          f"ratio {e_mine / max(e_torch, 1e-300):.2f}")
    assert e_mine <= 4.0 * e_torch + 1e-12, (what, e_mine, e_torch)


def _adam_call(n, p, g, m, v, vmax, state, wd, zero_grad, shadow, gs=1.0, amp=None):
    ptr = lambda t: t.data_ptr() if t is not None else None
    _lib.call("jmt_opt_tick", state.data_ptr(), BETAS[0], BETAS[1], ptr(amp), ops.stream())
    _lib.call("jmt_adam_step", n, p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(),
              ptr(vmax), state.data_ptr(), BETAS[0], BETAS[1], EPS, wd, gs, ptr(amp),
              int(zero_grad), ptr(shadow), ops.dt(shadow) if shadow is not None else _lib.BF16,
              ops.stream())


# 3: the scalar tail only; 64: one padded parameter; 10007: vector body + tail; 2_100_003: more
# than one grid pass of 2048 x 256 x 4 elements, so the grid-stride loop iterates
@pytest.mark.parametrize("wd", [0.0, 1e-4], ids=["wd0", "wd1e-4"])
@pytest.mark.parametrize("amsgrad", [False, True], ids=["adam", "amsgrad"])
@pytest.mark.parametrize("n", [3, 64, 10007, 2_100_003])
def test_adam_kernel_matches_torch(n, amsgrad, wd):
    steps = 6
    gen = torch.Generator().manual_seed(1234 + n)
    p0 = torch.randn(n, generator=gen)
    zero_mask = (torch.arange(n) % 7) == 3           # elements that never receive a gradient
    grads = _grads((n,), steps, gen, zero_mask)
    (p64, m64, v64), = _torch_adam([p0], [[g] for g in grads], torch.float64, amsgrad, wd, steps)
    (p32, m32, v32), = _torch_adam([p0], [[g] for g in grads], torch.float32, amsgrad, wd, steps)

    # bf16 shadow + fused zeroing for plain Adam, f16 shadow + the gradient kept for AMSGrad
    zero_grad = not amsgrad
    sdt = torch.float16 if amsgrad else torch.bfloat16
    p = p0.to(DEV)
    g = torch.empty(n, device=DEV)
    m, v = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    vmax = torch.zeros(n, device=DEV) if amsgrad else None
    shadow = torch.zeros(n, dtype=sdt, device=DEV)
    state = torch.tensor([LR, 0, 0, 0, 0, 0, 0, 0], dtype=torch.float32, device=DEV)
    for k in range(steps):
        g.copy_(grads[k])
        _adam_call(n, p, g, m, v, vmax, state, wd, zero_grad, shadow)
        if zero_grad:
            assert int(torch.count_nonzero(g)) == 0, k
        else:
            assert torch.equal(g.cpu(), grads[k]), k
    torch.cuda.synchronize()

    _check_bound(f"param n={n}", p, p32, p64)
    _check_bound(f"exp_avg n={n}", m, m32, m64)
    _check_bound(f"exp_avg_sq n={n}", v, v32, v64)
    if amsgrad:
        assert bool((vmax >= v).all())
    if wd == 0.0:
        assert torch.equal(p.cpu()[zero_mask], p0[zero_mask])
    assert torch.equal(shadow, p.to(sdt))
    # the tick: step count, step_size = lr / (1 - b1^t) and sqrt(1 - b2^t), rounded once
    st = state.cpu()
    lr32 = float(torch.tensor(LR, dtype=torch.float32))
    want = torch.tensor([lr32, steps, lr32 / (1 - BETAS[0] ** steps),
                         math.sqrt(1 - BETAS[1] ** steps), 0, 0, 0, 0], dtype=torch.float32)
    assert torch.equal(st[[0, 1, 4, 5, 6, 7]], want[[0, 1, 4, 5, 6, 7]])
    assert torch.allclose(st[2:4], want[2:4], rtol=2.0 ** -22, atol=0.0), (st, want)


def test_adam_kernel_found_inf_skips_but_zeroes():
    n = 1031
    gen = torch.Generator().manual_seed(5)
    p = torch.randn(n, generator=gen).to(DEV)
    g = torch.randn(n, generator=gen).to(DEV)
    m, v = torch.rand(n, device=DEV), torch.rand(n, device=DEV)
    shadow = p.bfloat16()
    state = torch.tensor([LR, 2, 0.1, 0.2, 0, 0, 0, 0], dtype=torch.float32, device=DEV)
    amp = torch.tensor([8.0, 0.125, 1.0, 0.0, 0.0], device=DEV)       # found_inf set
    before = [t.clone() for t in (p, m, v, shadow, state)]
    _adam_call(n, p, g, m, v, None, state, 0.0, False, shadow, amp=amp)
    assert int(torch.count_nonzero(g)) > 0                           # no zeroing asked
    _adam_call(n, p, g, m, v, None, state, 0.0, True, shadow, amp=amp)
    assert int(torch.count_nonzero(g)) == 0
    for a, b in zip((p, m, v, shadow, state), before):
        assert torch.equal(a, b)


SHAPES = [(37, 5), (1000,), (3, 129)]


def _ragged(seed, steps):
    gen = torch.Generator().manual_seed(seed)
    p0 = [torch.randn(s, generator=gen) for s in SHAPES]
    grads = [[_grads(s, 1, gen)[0] for s in SHAPES] for _ in range(steps)]
    return p0, grads


def _feed(params, gs):
    for p, g in zip(params, gs):
        p.grad.copy_(g)


def test_fused_adam_ragged_parameters():
    steps, wd = 5, 1e-4
    p0, grads = _ragged(11, steps)
    ref64 = _torch_adam(p0, grads, torch.float64, True, wd, steps)
    ref32 = _torch_adam(p0, grads, torch.float32, True, wd, steps)
    params = [torch.nn.Parameter(p.clone().to(DEV)) for p in p0]
    opt = FusedAdam(params, lr=LR, betas=BETAS, eps=EPS, weight_decay=wd, amsgrad=True,
                    shadow_dtype=torch.bfloat16)
    # what jmt.dist.GradBucketer relies on
    assert opt.params == params and opt.numel == 192 + 1024 + 448
    assert opt.offsets == [0, 192, 1216] and opt.flat_g.numel() == opt.numel
    sd = None
    for k in range(steps):
        opt.zero_grad()
        _feed(params, grads[k])
        opt.step()
        if k == 2:
            sd = opt.state_dict()
    torch.cuda.synchronize()
    pad = torch.ones(opt.numel, dtype=torch.bool)
    for i, (p, off) in enumerate(zip(params, opt.offsets)):
        k = p.numel()
        pad[off:off + k] = False
        assert p.data_ptr() == opt.flat_p[off:].data_ptr()
        _check_bound(f"param[{i}]", p.detach(), ref32[i][0], ref64[i][0])
        _check_bound(f"exp_avg[{i}]", opt.exp_avg[off:off + k].view_as(p), ref32[i][1],
                     ref64[i][1])
        _check_bound(f"exp_avg_sq[{i}]", opt.exp_avg_sq[off:off + k].view_as(p), ref32[i][2],
                     ref64[i][2])
    pad = pad.to(DEV)
    assert int(torch.count_nonzero(opt.flat_p[pad])) == 0
    assert int(torch.count_nonzero(opt.shadow[pad].float())) == 0
    assert torch.equal(opt.shadow, opt.flat_p.bfloat16())
    assert float(opt.state[1]) == steps

    # resume from the state after step 3 in a fresh optimizer: bit-identical continuation
    params2 = [torch.nn.Parameter(torch.zeros_like(p)) for p in params]
    opt2 = FusedAdam(params2, lr=123.0, betas=BETAS, eps=EPS, weight_decay=wd, amsgrad=True,
                     shadow_dtype=torch.bfloat16)
    opt2.load_state_dict(sd)
    assert opt2.get_lr() == LR and float(opt2.state[1]) == 3
    for k in range(3, steps):
        opt2.zero_grad()
        _feed(params2, grads[k])
        opt2.step()
    for name in ("flat_p", "exp_avg", "exp_avg_sq", "max_exp_avg_sq", "state", "shadow"):
        assert torch.equal(getattr(opt2, name), getattr(opt, name)), name


def test_gradscaler_with_fused_adam():
    """tests/test_gpu_amp.py's scenario with Adam: 9 steps, overflow at {0, 4, 5}, init_scale
    1024, growth interval 2, against torch.amp.GradScaler + torch.optim.Adam on the device."""
    steps, bad_steps, wd = 9, {0, 4, 5}, 1e-4
    gen = torch.Generator().manual_seed(0)
    p0 = [torch.randn(s, generator=gen) for s in SHAPES]
    grads = [[torch.randn(s, generator=gen) for s in SHAPES] for _ in range(steps)]
    ref = [torch.nn.Parameter(p.clone().to(DEV)) for p in p0]
    ropt = torch.optim.Adam(ref, lr=LR, betas=BETAS, eps=EPS, weight_decay=wd)
    rsc = torch.amp.GradScaler("cuda", init_scale=1024.0, growth_interval=2)
    mine = [torch.nn.Parameter(p.clone().to(DEV)) for p in p0]
    opt = FusedAdam(mine, lr=LR, betas=BETAS, eps=EPS, weight_decay=wd)
    sc = GradScaler(init_scale=1024.0, growth_interval=2, device=DEV)
    scales, applied = [], 0
    for k in range(steps):
        rsc.scale(torch.zeros((), device=DEV))      # torch creates its scale tensor lazily here
        s_ref, s_mine = rsc.get_scale(), sc.get_scale()
        assert s_ref == s_mine, (k, s_ref, s_mine)
        scales.append(s_mine)
        for i, (pr, pm) in enumerate(zip(ref, mine)):
            gk = grads[k][i].to(DEV) * s_ref
            if k in bad_steps and i == len(ref) - 1:
                gk[0] = float("inf") if k % 2 else float("nan")
            pr.grad = gk.clone()
            pm.grad.copy_(gk)
        before = [t.clone() for t in (opt.state, opt.exp_avg, opt.exp_avg_sq, opt.flat_p)]
        rsc.step(ropt)
        rsc.update()
        sc.step(opt)
        sc.update()
        if k in bad_steps:
            for a, b in zip((opt.state, opt.exp_avg, opt.exp_avg_sq, opt.flat_p), before):
                assert torch.equal(a, b), k
        else:
            applied += 1
        assert float(opt.state[1]) == applied
        for pr, pm in zip(ref, mine):
            maxp = float(pr.detach().abs().max())
            ulp = 2.0 ** (math.floor(math.log2(maxp)) - 23)
            err = float((pr.detach() - pm.detach()).abs().max())
            assert err <= 4 * ulp, (k, err, ulp)
    assert rsc.get_scale() == sc.get_scale()
    assert min(scales) < 1024.0 and max(scales) > 512.0     # backed off and grew again


# ------------------------------------------------------------------ SGD with a device lr

def _sgd_pair(fuse_zero_grad, seed=3):
    gen = torch.Generator().manual_seed(seed)
    p0 = [torch.randn(s, generator=gen) for s in SHAPES]
    kw = dict(momentum=0.9, dampening=0.0, weight_decay=1e-4, nesterov=True,
              shadow_dtype=torch.bfloat16, fuse_zero_grad=fuse_zero_grad)
    pa = [torch.nn.Parameter(p.clone().to(DEV)) for p in p0]
    pb = [torch.nn.Parameter(p.clone().to(DEV)) for p in p0]
    return pa, pb, kw, gen


def _same(a, b):
    for name in ("flat_p", "buf", "shadow", "flat_g"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name


@pytest.mark.parametrize("fuse_zero_grad", [False, True], ids=["keep_grad", "fused_zero"])
def test_sgd_device_lr_equals_baked_lr(fuse_zero_grad):
    pa, pb, kw, gen = _sgd_pair(fuse_zero_grad)
    baked = FusedSGD(pa, lr=1e-2, **kw)
    dev = FusedSGD(pb, lr=1e-2, device_lr=True, **kw)
    assert baked.state is None and dev.state.shape == (8,)
    grads = [[torch.randn(s, generator=gen).to(DEV) for s in SHAPES] for _ in range(5)]
    for k in range(4):
        for o, ps in ((baked, pa), (dev, pb)):
            o.zero_grad()
            _feed(ps, grads[k])
            o.step()
        _same(baked, dev)
    if fuse_zero_grad:
        assert int(torch.count_nonzero(dev.flat_g)) == 0

    # a new lr on the device == a fresh baked-lr optimizer handed the same state
    dev.set_lr(1e-3)
    assert dev.get_lr() == 1e-3
    pc = [torch.nn.Parameter(p.detach().clone()) for p in pb]
    fresh = FusedSGD(pc, lr=1e-3, **kw)
    fresh.buf.copy_(dev.buf)
    fresh.first = False
    for o, ps in ((fresh, pc), (dev, pb)):
        o.zero_grad()
        _feed(ps, grads[4])
        o.step()
    _same(fresh, dev)
    assert not torch.equal(dev.flat_p, baked.flat_p)


def test_sgd_device_lr_with_gradscaler_equals_baked_lr():
    pa, pb, kw, gen = _sgd_pair(True, seed=4)
    baked = FusedSGD(pa, lr=1e-2, **kw)
    dev = FusedSGD(pb, lr=1e-2, device_lr=True, **kw)
    sa = GradScaler(init_scale=64.0, growth_interval=2, device=DEV)
    sb = GradScaler(init_scale=64.0, growth_interval=2, device=DEV)
    for k in range(4):
        gs = [torch.randn(s, generator=gen).to(DEV) * 64.0 for s in SHAPES]
        if k == 1:
            gs[0][0, 0] = float("inf")              # a skipped step: both leave everything be
        for o, ps, sc in ((baked, pa, sa), (dev, pb, sb)):
            o.zero_grad(force=True)
            _feed(ps, gs)
            sc.step(o)
            sc.update()
        _same(baked, dev)
        assert torch.equal(sa.state, sb.state)


def test_sgd_state_dict_round_trip():
    pa, pb, kw, gen = _sgd_pair(False, seed=6)
    a = FusedSGD(pa, lr=1e-2, device_lr=True, **kw)
    grads = [[torch.randn(s, generator=gen).to(DEV) for s in SHAPES] for _ in range(3)]
    for k in range(2):
        a.zero_grad()
        _feed(pa, grads[k])
        a.step()
    a.set_lr(3e-3)
    sd = a.state_dict()
    b = FusedSGD(pb, lr=1.0, device_lr=True, **kw)
    b.load_state_dict(sd)
    assert b.get_lr() == 3e-3 and b.first is False
    for o, ps in ((a, pa), (b, pb)):
        o.zero_grad()
        _feed(ps, grads[2])
        o.step()
    _same(a, b)
    with pytest.raises(ValueError):
        FusedSGD([torch.nn.Parameter(torch.zeros(8, device=DEV))], lr=1.0).load_state_dict(sd)
