"""A captured training step (jmt/graph.py) with the optimizer state on the device: FusedAdam
replays like it steps eagerly, and a learning-rate schedule stepped between replays reaches the
captured step without re-capture (the lr is read from the device state block, not baked into the
graph as a kernel argument).  Model and shapes as tests/test_gpu_graph.py (B=4, T=37)."""
import pytest
import torch

from jmt import functional as JF
from jmt.graph import GraphedStep
from jmt.lr_scheduler import MyStepLR
from jmt.optim import FusedAdam, FusedSGD, GradScaler, used_parameters
from oracle.hashinit import init_module_

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
CDS = pytest.mark.parametrize("cd", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])


def _make_opt(kind, params, cd):
    shadow = cd if cd != torch.float32 else None
    if kind == "adam":
        return FusedAdam(params, lr=1e-3, weight_decay=1e-4, shadow_dtype=shadow)
    return FusedSGD(params, lr=1e-2, momentum=0.9, dampening=0.0, weight_decay=1e-4,
                    nesterov=True, shadow_dtype=shadow, device_lr=(kind == "sgd_dev"))


def _setup(cd, kind, scaler=False, B=4, T=37):
    from models.two_transformers import Two_transformers
    from models.fc_layer import FcLayer
    from losses.loss import CCCLoss
    m = Two_transformers(0.0, 0.0, 1, 1, "TRANSFORMER", "FC", 2048)
    fc = FcLayer(1024, 512)
    init_module_(m, "")
    init_module_(fc, "fc.")
    m, fc = m.to(DEV), fc.to(DEV)
    g = torch.Generator(device=DEV).manual_seed(7)
    audio = torch.randn(B, T, 1024, device=DEV, generator=g)
    video = torch.randn(B, T, 2048, device=DEV, generator=g)
    lv = (torch.rand(B, T, device=DEV, generator=g) * 2 - 1).view(-1, B * T)
    la = (torch.rand(B, T, device=DEV, generator=g) * 2 - 1).view(-1, B * T)
    crit = CCCLoss(1)
    sc = GradScaler(init_scale=256.0, growth_interval=1000, device=DEV) if scaler else None

    def fwd_bwd():
        with JF.compute_mode(cd):
            vo, ao = m(fc(audio), video)
            loss = crit(vo.view(-1, B * T), lv) + crit(ao.view(-1, B * T), la)
            (sc.scale(loss) if sc is not None else loss).backward()
        return loss

    params = used_parameters(fwd_bwd, list(m.parameters()) + list(fc.parameters()))
    opt = _make_opt(kind, params, cd)

    def step():
        opt.zero_grad()
        loss = fwd_bwd()
        if sc is not None:
            sc.step(opt)
            sc.update()
        else:
            opt.step()
        return loss.detach()

    return step, opt


@CDS
def test_adam_graph_replay_matches_eager(cd):
    step_e, opt_e = _setup(cd, "adam")
    for _ in range(2):
        step_e()
    eager = [float(step_e()) for _ in range(3)]
    torch.cuda.synchronize()
    pe = opt_e.flat_p.clone()

    step_g, opt_g = _setup(cd, "adam")
    step_g()
    gs = GraphedStep(step_g).capture(warmup=1)
    graphed = [float(gs.replay()) for _ in range(3)]
    torch.cuda.synchronize()
    assert graphed == eager, (graphed, eager)
    assert torch.equal(opt_g.flat_p, pe)
    assert float(opt_g.state[1]) == 5 and torch.equal(opt_g.state, opt_e.state)


def _eager_run(cd, kind, scheduled):
    """2 warm-up steps, 2 steps, (the schedule moves,) 2 steps."""
    step, opt = _setup(cd, kind)
    sched = MyStepLR(opt, step_size=1, gamma=0.1, min_lr=1e-7)
    for _ in range(4):
        step()
    if scheduled:
        sched.step()
    for _ in range(2):
        step()
    torch.cuda.synchronize()
    return opt.flat_p.clone(), opt.get_lr()


@CDS
@pytest.mark.parametrize("kind", ["sgd_dev", "adam"])
def test_schedule_reaches_the_captured_step(cd, kind):
    step, opt = _setup(cd, kind)
    base = opt.get_lr()
    sched = MyStepLR(opt, step_size=1, gamma=0.1, min_lr=1e-7)
    step()
    gs = GraphedStep(step).capture(warmup=1)
    for _ in range(2):
        gs.replay()
    sched.step()                                   # between replays, no re-capture
    assert opt.get_lr() == pytest.approx(0.1 * base)
    for _ in range(2):
        gs.replay()
    torch.cuda.synchronize()
    assert float(opt.state[0]) == float(torch.tensor(opt.get_lr(), dtype=torch.float32))

    followed, lr_f = _eager_run(cd, kind, scheduled=True)
    frozen, lr_0 = _eager_run(cd, kind, scheduled=False)
    assert lr_f == opt.get_lr() and lr_0 == base
    assert torch.equal(opt.flat_p, followed)
    assert not torch.equal(opt.flat_p, frozen)


def test_baked_lr_is_frozen_in_the_graph():
    """The contrast the device lr exists for: without it set_lr() changes the host value only
    and the captured step keeps the lr it was captured with (FusedSGD.set_lr's docstring)."""
    cd = torch.float32
    step, opt = _setup(cd, "sgd")
    step()
    gs = GraphedStep(step).capture(warmup=1)
    for _ in range(2):
        gs.replay()
    opt.set_lr(1e-3)
    for _ in range(2):
        gs.replay()
    torch.cuda.synchronize()
    frozen, _ = _eager_run(cd, "sgd_dev", scheduled=False)
    assert opt.get_lr() == 1e-3 and torch.equal(opt.flat_p, frozen)


def test_captured_gradscaler_adam_counts_steps():
    step, opt = _setup(torch.bfloat16, "adam", scaler=True)
    gs = GraphedStep(step).capture(warmup=1)
    n0 = float(opt.state[1])
    assert n0 == 1                                  # the capture's own warm-up step
    opt.state[1:2].fill_(0.0)
    for _ in range(3):
        gs.replay()
    torch.cuda.synchronize()
    assert float(opt.state[1]) == 3
